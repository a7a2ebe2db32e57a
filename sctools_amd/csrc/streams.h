// streams.h -- host only: the metric step's side streams and events (StepStreams), the per-device
// pool they come from, and the early readback.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include <mutex>
#include <utility>
#include <vector>

#include "util.h"

namespace sct {

// ---------------- the per-device pool of side-stream pairs ----------------
// Pairs (s2, s3) are created once and reused (round 4: creating them per call cost ~0.6 ms of host
// time before the first Welford launch).  A call holds its pair until it returns, so concurrent
// pipelines on one device get pairs of their own (round 5: a shared pair queued one pipeline's head
// kernel behind another's, and the start gate then held the second pipeline's key pass for its
// whole time-out).
constexpr int kMaxSideDevices = 64;
struct SidePool {
  std::mutex mu;
  std::vector<std::pair<hipStream_t, hipStream_t>> free[kMaxSideDevices];
  int in_use[kMaxSideDevices] = {};  // pairs held by running calls, per device
};
inline SidePool& side_pool() {
  static SidePool p;
  return p;
}
// *alone: no other call on this device holds a pair (so no other pipeline's Welford kernels can
// share a hardware queue with this one's)
inline hipError_t side_streams(int dev, hipStream_t* s2, hipStream_t* s3, bool* alone) {  // (`dev` is current)
  if (dev < 0 || dev >= kMaxSideDevices) return hipErrorInvalidDevice;
  SidePool& p = side_pool();
  {
    std::lock_guard<std::mutex> g(p.mu);
    *alone = p.in_use[dev] == 0;
    if (!p.free[dev].empty()) {
      *s2 = p.free[dev].back().first;
      *s3 = p.free[dev].back().second;
      p.free[dev].pop_back();
      p.in_use[dev]++;
      return hipSuccess;
    }
  }
  hipStream_t a = nullptr, b = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&a, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&b, hipStreamNonBlocking);
  if (e != hipSuccess) {
    if (a) (void)hipStreamDestroy(a);
    return e;
  }
  *s2 = a;
  *s3 = b;
  std::lock_guard<std::mutex> g(p.mu);
  p.in_use[dev]++;
  return hipSuccess;
}
inline void side_streams_release(int dev, hipStream_t s2, hipStream_t s3) {
  SidePool& p = side_pool();
  std::lock_guard<std::mutex> g(p.mu);
  p.free[dev].emplace_back(s2, s3);
  p.in_use[dev]--;
}

// ---------------- early readback ----------------
// readback (util.h) split in two: the copy is queued (readback_start) and waited for later
// (readback_finish), so the kernels queued in between keep the device busy while the host waits for
// the copy.  One per host thread, through the thread's own pinned buffer and event.  `pending`: a copy
// started and not finished; readback_start and ~StepStreams wait for it, so none outlives its call.
struct EarlyReadback {
  void* buf = nullptr;
  hipEvent_t ev = nullptr;
  bool pending = false;
  ~EarlyReadback() {
    if (buf) (void)hipHostFree(buf);
    if (ev) (void)hipEventDestroy(ev);
  }
};
inline EarlyReadback& early_readback() {
  static thread_local EarlyReadback rb;
  return rb;
}
inline void readback_settle() {
  EarlyReadback& rb = early_readback();
  if (rb.pending) (void)hipEventSynchronize(rb.ev);
  rb.pending = false;
}
inline int readback_start(const void* src, size_t bytes, hipStream_t s) {
  EarlyReadback& rb = early_readback();
  if (bytes > PinnedReadback::kCap)
    return fail(SCT_EINVAL, "readback of %zu bytes exceeds %zu", bytes, PinnedReadback::kCap);
  readback_settle();
  if (!rb.buf) HIPCHK(hipHostMalloc(&rb.buf, PinnedReadback::kCap, hipHostMallocPortable));
  if (!rb.ev) HIPCHK(hipEventCreateWithFlags(&rb.ev, hipEventDisableTiming));
  HIPCHK(hipMemcpyAsync(rb.buf, src, bytes, hipMemcpyDeviceToHost, s));
  const hipError_t e = hipEventRecord(rb.ev, s);
  if (e != hipSuccess) (void)hipStreamSynchronize(s);  // no event to wait on: the copy ends here
  HIPCHK(e);
  rb.pending = true;
  return SCT_OK;
}
inline int readback_finish(void* dst, size_t bytes) {
  EarlyReadback& rb = early_readback();
  if (!rb.pending) return fail(SCT_EINVAL, "internal: readback_finish without readback_start");
  rb.pending = false;
  HIPCHK(hipEventSynchronize(rb.ev));
  memcpy(dst, rb.buf, bytes);
  return SCT_OK;
}

// ---------------- StepStreams ----------------
// The one owner of a metric step's side streams and events.  side[0] and side[1] are the (s2, s3)
// pair of the pool, taken at most once per call (open) and held until the call returns.  Ordering:
//   fork(i, from)  side[i] waits for what is queued on `from` so far
//   join(i)        the caller's stream waits for what is queued on side[i] so far
// use(i) hands side[i] out for a launch and flags it as carrying unjoined work; mark(i, &ev) records
// the end of that work early, for a later join(i, ev) or wait_caller(ev).  Every event is created by
// record() and destroyed with the owner.  drain() synchronizes the side streams with unjoined work,
// so after an early return (an error, or the global-sort redo that reuses the workspace) nothing
// still writes into the caller's buffers; on the success path every stream is joined by an event.
struct StepStreams {
  hipStream_t caller;
  int dev = -1;
  hipStream_t side[2] = {nullptr, nullptr};
  bool unjoined[2] = {false, false};
  bool alone = true;  // no other call on this device held a pair when this one was taken
  std::vector<hipEvent_t> evs;

  explicit StepStreams(hipStream_t c) : caller(c) {}
  StepStreams(const StepStreams&) = delete;
  bool is_open() const { return side[0] != nullptr; }
  hipError_t open() {  // on the caller's stream's device; the thread's current device is restored
    if (is_open()) return hipSuccess;
    int prev = 0;
    hipError_t e = hipStreamGetDevice(caller, &dev);
    if (e == hipSuccess) e = hipGetDevice(&prev);
    if (e != hipSuccess) return e;
    if (prev != dev && (e = hipSetDevice(dev)) != hipSuccess) return e;
    e = side_streams(dev, &side[0], &side[1], &alone);
    if (e != hipSuccess) side[0] = side[1] = nullptr;
    if (prev != dev) (void)hipSetDevice(prev);
    return e;
  }
  hipStream_t use(int i) {
    unjoined[i] = true;
    return side[i];
  }
  hipError_t record(hipStream_t on, hipEvent_t* ev) {
    hipError_t e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    evs.push_back(*ev);
    return hipEventRecord(*ev, on);
  }
  hipError_t fork(int i, hipStream_t from, hipEvent_t* at = nullptr) {
    hipEvent_t ev = nullptr;
    hipError_t e = record(from, &ev);
    if (e == hipSuccess) e = hipStreamWaitEvent(side[i], ev, 0);
    if (at) *at = ev;
    return e;
  }
  hipError_t mark(int i, hipEvent_t* at) { return record(side[i], at); }
  hipError_t wait_caller(hipEvent_t ev) { return hipStreamWaitEvent(caller, ev, 0); }
  hipError_t join(int i, hipEvent_t at = nullptr) {
    hipError_t e = at ? hipSuccess : mark(i, &at);
    if (e == hipSuccess) e = wait_caller(at);
    if (e == hipSuccess) unjoined[i] = false;
    return e;
  }
  hipError_t drain() {
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2; i++) {
      if (!unjoined[i]) continue;
      const hipError_t ei = hipStreamSynchronize(side[i]);
      if (ei != hipSuccess) e = ei;
      unjoined[i] = false;
    }
    return e;
  }
  ~StepStreams() {
    (void)drain();
    readback_settle();
    for (hipEvent_t ev : evs) (void)hipEventDestroy(ev);
    if (is_open()) side_streams_release(dev, side[0], side[1]);
  }
};

}  // namespace sct
