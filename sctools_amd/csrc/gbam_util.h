// gbam_util.h -- what every stage of the device BAM decoder (gbam.hip) shares: the payload's constants and
// little-endian reads, the error path (gfail, HIPOK: device memory exhausted declines the file to the
// host decoder), device buffers counted against SCT_GBAM_MAX_DEVICE_BYTES, the caller's device
// restored on return, the scan and launch-grid helpers and the copy stream of the window inflate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <hipcub/hipcub.hpp>
#include <string>

#include "../../include/sct_bam.h"
#include "../../include/sct_gbam.h"

namespace gb {

constexpr uint64_t kUnknown = ~0ull, kBadWalk = ~0ull - 1;
constexpr uint32_t kScan = 1u << 18;  // bytes a member's start guess looks through
constexpr int kStartRounds = 512;      // record-start repair rounds before the file goes to the host decoder
constexpr uint64_t kPad = 1u << 16;   // readable bytes after the file image and after U

__device__ __forceinline__ uint32_t u16(const uint8_t* U, uint64_t p) { return U[p] | (uint32_t)U[p + 1] << 8; }
__device__ __forceinline__ uint32_t u32(const uint8_t* U, uint64_t p) {
  return U[p] | (uint32_t)U[p + 1] << 8 | (uint32_t)U[p + 2] << 16 | (uint32_t)U[p + 3] << 24;
}

}  // namespace gb

namespace {
using namespace gb;

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

thread_local std::string g_gerr;
int gfail(int code, const char* msg) {
  g_gerr = msg;
  return code;
}

// A device allocation that fails declines the file to the host decoder (SCT_GBAM_HOST) instead of
// failing the decode: a BAM too large for the device's memory is still a valid input.
#define HIPOK(x)                                                                            \
  do {                                                                                      \
    hipError_t e_ = (x);                                                                    \
    if (e_ == hipErrorOutOfMemory) {                                                        \
      (void)hipGetLastError();                                                              \
      return gfail(SCT_GBAM_HOST, "device memory exhausted: the host decoder takes the file"); \
    }                                                                                       \
    if (e_ != hipSuccess) return gfail(SCT_BAM_EIO, hipGetErrorString(e_));                 \
  } while (0)

// SCT_GBAM_MAX_DEVICE_BYTES (tests): a cap on the device bytes the process's decodes hold at once;
// an allocation past it fails as hipMalloc does when HBM is exhausted.
uint64_t device_cap() {  // read per allocation (a few per decode): tests change it between calls
  const char* v = getenv("SCT_GBAM_MAX_DEVICE_BYTES");
  return v && *v ? (uint64_t)strtoull(v, nullptr, 10) : ~0ull;
}
std::atomic<uint64_t> g_held{0};  // device bytes held by DevBufs

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  size_t bytes = 0;
  hipError_t alloc(size_t count) {
    free();
    const size_t b = std::max<size_t>(count, 1) * sizeof(T);
    if (g_held + b > device_cap()) return hipErrorOutOfMemory;
    const hipError_t e = hipMalloc(&p, b);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    n = count;
    bytes = b;
    g_held += b;
    return hipSuccess;
  }
  void free() {
    if (p) {
      (void)hipFree(p);
      g_held -= bytes;
    }
    p = nullptr;
    n = 0;
    bytes = 0;
  }
  void swap(DevBuf& o) {  // (a grown buffer takes the old one's place; the old one is freed with `o`)
    std::swap(p, o.p);
    std::swap(n, o.n);
    std::swap(bytes, o.bytes);
  }
  ~DevBuf() { free(); }
};

// the caller thread's current device, restored when an entry point returns (the library switches to
// the handle's device; the caller's own work must not move with it)
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

template <class I, class O>
hipError_t exclusive_sum(I* in, O* out, uint64_t n, hipStream_t st, DevBuf<uint8_t>& tmp) {
  size_t bytes = 0;
  // 64-bit item counts (rocPRIM scans size_t items): parse_begin admits tables of 2^31 slots
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (size_t)n, st);
  if (e != hipSuccess) return e;
  if (tmp.n < bytes) {
    e = tmp.alloc(bytes);
    if (e != hipSuccess) return e;
  }
  return hipcub::DeviceScan::ExclusiveSum(tmp.p, bytes, in, out, (size_t)n, st);
}

inline unsigned grid(uint64_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }

constexpr int kCopyChunks = 8;
struct CopyStream {  // a non-blocking copy stream and one event per piece
  hipStream_t s = nullptr;
  hipEvent_t ev[kCopyChunks] = {};
  hipError_t init(hipStream_t) {
    hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    for (int k = 0; k < kCopyChunks && e == hipSuccess; k++) e = hipEventCreateWithFlags(&ev[k], hipEventDisableTiming);
    return e;
  }
  ~CopyStream() {  // (the consumer stream's waits are enqueued; destruction is deferred past them)
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    if (s) (void)hipStreamDestroy(s);
  }
};

}  // namespace
