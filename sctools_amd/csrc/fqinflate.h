// fqinflate.h -- the sct_fq_bgzf_scan / sct_fq_inflate calls of libsct_fastq.so
// (include/sct_fastq_inflate.h): BGZF-compressed FASTQ inflated on gfx950.
//
//   host    bgzf_scan   hops the gzip member headers of a mapped file (the rule of bgzf.h's
//                       scan_blocks, stricter about what is left over), no zlib
//   device  k_inflate   inflate.h as libsct_gbam.so runs it, included and not edited: one wave
//                       per member
//           k_fq_crc32  one wave per member: the gzip CRC-32 of the payload where k_inflate just
//                       wrote it, against the member's trailer; then the two-word summary
//
// THE CRC.  A member's n bytes are cut into 64 slices of L = ceil(n / 64) bytes aligned to the
// member's END, so the short slice is lane 0's and reads as if it had zero bytes in front: a raw
// remainder (register starting at 0, no final xor) does not change under leading zeros.  Each lane
// runs a slicing-by-4 table CRC over its slice (16-byte loads where the address allows), giving
// raw remainders r_0 .. r_63, and the member's raw remainder is
//     sum_i  r_i * x^(8 L (63 - i))   mod P
// which the wave folds in six steps: at step k the lane at the right end of every group of 2^(k+1)
// takes the partner 2^k lanes to its left times x^(8 L 2^k) and adds its own; the operator is
// squared from step to step.  "times x^m mod P" is a 32-step shift-and-add in GF(2) on the
// bit-reflected representation (bit 31 is x^0), the polynomial arithmetic zlib's crc32_combine
// uses, so there are no 32x32 matrices to keep.  The register's start value 0xffffffff and the
// final xor are applied at the end: crc = raw ^ (0xffffffff * x^(8 n)) ^ 0xffffffff.
//
// The tables (4 x 256 words) are built in LDS by the wave itself.  A lookup is indexed by data
// bytes xor-ed with the running remainder, so the 64 lanes of a read fall on the 64 banks about at
// random (two to four deep); the inflate before it, one symbol at a time, is the longer kernel.
//
// Everything of the CRC is __host__ __device__ (as tsround.h), so tests/native/fqcrc.cpp runs the
// same slices and the same fold on the host against zlib.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SCT_FQI_HD __host__ __device__ __forceinline__
#else
#define SCT_FQI_HD static inline
#endif

namespace fqi {

constexpr uint32_t kPoly = 0xEDB88320u;  // the gzip polynomial, bit-reflected
constexpr uint32_t kLanes = 64;

// entry i of slicing table 0: the remainder of byte i followed by nothing
SCT_FQI_HD uint32_t crc_byte_entry(uint32_t i) {
  uint32_t c = i;
  for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1) ? kPoly : 0);
  return c;
}

// table[k][i], k = 1..3, from table[k - 1][i] and table 0: one more zero byte behind
SCT_FQI_HD uint32_t crc_next_entry(uint32_t prev, const uint32_t* t0) { return (prev >> 8) ^ t0[prev & 0xff]; }

// fills tab[4 * 256]; `lane` of `lanes` callers (1 on the host); `sync` between the tables
template <typename Sync>
SCT_FQI_HD void crc_build_tables(uint32_t* tab, uint32_t lane, uint32_t lanes, Sync sync) {
  for (uint32_t i = lane; i < 256; i += lanes) tab[i] = crc_byte_entry(i);
  sync();
  for (uint32_t k = 1; k < 4; k++) {
    for (uint32_t i = lane; i < 256; i += lanes) tab[k * 256 + i] = crc_next_entry(tab[(k - 1) * 256 + i], tab);
    sync();
  }
}

SCT_FQI_HD uint32_t crc_step_byte(uint32_t r, uint8_t b, const uint32_t* tab) { return (r >> 8) ^ tab[(r ^ b) & 0xff]; }

SCT_FQI_HD uint32_t crc_step_word(uint32_t r, uint32_t w, const uint32_t* tab) {
  r ^= w;  // little-endian: the word's low byte is the first byte
  return tab[768 + (r & 0xff)] ^ tab[512 + ((r >> 8) & 0xff)] ^ tab[256 + ((r >> 16) & 0xff)] ^ tab[r >> 24];
}

// raw remainder (start 0, no final xor) of p[0, n)
SCT_FQI_HD uint32_t crc_raw(const uint8_t* p, uint32_t n, const uint32_t* tab) {
  uint32_t r = 0, i = 0;
  while (i < n && ((uintptr_t)(p + i) & 15)) r = crc_step_byte(r, p[i++], tab);
  for (; i + 16 <= n; i += 16) {
    uint32_t w[4];
#if defined(__HIP_DEVICE_COMPILE__)
    const uint4 v = *reinterpret_cast<const uint4*>(p + i);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
#else
    memcpy(w, p + i, 16);
#endif
    r = crc_step_word(r, w[0], tab);
    r = crc_step_word(r, w[1], tab);
    r = crc_step_word(r, w[2], tab);
    r = crc_step_word(r, w[3], tab);
  }
  while (i < n) r = crc_step_byte(r, p[i++], tab);
  return r;
}

// a * b mod P, both in the reflected representation (bit 31 is x^0)
SCT_FQI_HD uint32_t gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int k = 0; k < 32; k++) {
    p ^= (a & (0x80000000u >> k)) ? b : 0;
    b = (b >> 1) ^ ((b & 1) ? kPoly : 0);
  }
  return p;
}

// x^bits mod P
SCT_FQI_HD uint32_t gf_xpow(uint64_t bits) {
  uint32_t result = 0x80000000u, base = 0x40000000u;  // 1, x
  while (bits) {
    if (bits & 1) result = gf_mul(result, base);
    base = gf_mul(base, base);
    bits >>= 1;
  }
  return result;
}

// bytes of a lane's slice of an n-byte member
SCT_FQI_HD uint32_t crc_slice_len(uint32_t n) { return (n + kLanes - 1) / kLanes; }

// lane's slice [*lo, *hi) of [0, n): slices of L bytes aligned to n, clipped at 0
SCT_FQI_HD void crc_slice(uint32_t n, uint32_t lane, uint32_t* lo, uint32_t* hi) {
  const int64_t L = crc_slice_len(n);
  const int64_t b = (int64_t)n - (int64_t)(kLanes - lane) * L, e = b + L;
  *lo = (uint32_t)(b < 0 ? 0 : b);
  *hi = (uint32_t)(e < 0 ? 0 : e);
}

// one fold step at the right end of a pair of groups: the left group's remainder moved along by
// the right group's length (times `op`), plus the right group's
SCT_FQI_HD uint32_t crc_fold(uint32_t left, uint32_t right, uint32_t op) { return gf_mul(op, left) ^ right; }

// the gzip CRC-32 of an n-byte message from its raw remainder
SCT_FQI_HD uint32_t crc_finish(uint32_t raw, uint32_t n) {
  return raw ^ gf_mul(gf_xpow(8ull * n), 0xffffffffu) ^ 0xffffffffu;
}

// The kernel's computation on the host: the 64 slices one after the other, then the same fold.
inline uint32_t crc32_as_the_wave(const uint8_t* p, uint32_t n) {
  struct Tables {
    uint32_t t[1024];
    Tables() { crc_build_tables(t, 0, 1, [] {}); }
  };
  static const Tables tables;
  const uint32_t* tab = tables.t;
  uint32_t r[kLanes];
  for (uint32_t lane = 0; lane < kLanes; lane++) {
    uint32_t lo, hi;
    crc_slice(n, lane, &lo, &hi);
    r[lane] = crc_raw(p + lo, hi - lo, tab);
  }
  uint32_t op = gf_xpow(8ull * crc_slice_len(n));
  for (uint32_t s = 1; s < kLanes; s <<= 1) {
    for (uint32_t lane = 0; lane < kLanes; lane++)
      if ((lane & (2 * s - 1)) == 2 * s - 1) r[lane] = crc_fold(r[lane - s], r[lane], op);
    op = gf_mul(op, op);
  }
  return crc_finish(r[kLanes - 1], n);
}

}  // namespace fqi

#if defined(__HIPCC__)

#include <hip/hip_runtime.h>

#include "../../include/sct_fastq_inflate.h"
#include "inflate.h"  // gb::k_inflate, gb::Member, gb::ST_*: shared with gbam.hip, not edited here
#include "liberr.h"

namespace fqi {

static_assert(sizeof(sct_fq_member_t) == sizeof(gb::Member) && sizeof(gb::Member) == 24, "one member layout");
static_assert(SCT_FQ_ST_CRC > gb::ST_OVERRUN, "the CRC status is none of the inflate's");
constexpr int64_t kSlack = SCT_FQ_INFLATE_SLACK;

inline uint16_t rd16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// One wave per member.  A member the inflate declined keeps its status; one that inflated gets
// SCT_FQ_ST_CRC where the payload's CRC-32 is not the stored one.  Lane 0 then counts the member
// into the summary if it is not OK.
__global__ __launch_bounds__(64) void k_fq_crc32(const uint8_t* __restrict__ text, const gb::Member* __restrict__ mem,
                                                  const uint32_t* __restrict__ stored, uint32_t* __restrict__ status,
                                                  uint32_t* __restrict__ summary) {
  __shared__ uint32_t tab[1024];
  const uint32_t lane = threadIdx.x, m = blockIdx.x;
  uint32_t st = status[m];
  if (st == gb::ST_OK) {  // (block-uniform)
    const gb::Member M = mem[m];
    const uint32_t n = M.isize;
    crc_build_tables(tab, lane, kLanes, [] { __syncthreads(); });
    uint32_t lo, hi;
    crc_slice(n, lane, &lo, &hi);
    uint32_t r = crc_raw(text + M.out_off + lo, hi - lo, tab);
    uint32_t op = gf_xpow(8ull * crc_slice_len(n));
#pragma unroll
    for (uint32_t s = 1; s < kLanes; s <<= 1) {
      const uint32_t left = (uint32_t)__shfl_up((int)r, s, kLanes);
      if ((lane & (2 * s - 1)) == 2 * s - 1) r = crc_fold(left, r, op);
      op = gf_mul(op, op);
    }
    const int differs = crc_finish(r, n) != stored[m];  // (lane 63 holds the member's remainder)
    if (__shfl(differs, kLanes - 1, kLanes)) st = SCT_FQ_ST_CRC;
  }
  if (lane == 0 && st != gb::ST_OK) {
    status[m] = st;
    atomicAdd(&summary[0], 1u);
    atomicMin(&summary[1], m);
  }
}

// the workspace: Member[n], then the stored CRCs
size_t inflate_workspace_of(int64_t n) { return (size_t)(n > 0 ? n : 1) * (sizeof(gb::Member) + sizeof(uint32_t)); }

}  // namespace fqi

extern "C" {

int sct_fq_bgzf_scan(const uint8_t* file, int64_t size, int64_t from, int64_t max_members, sct_fq_member_t* members,
                     uint32_t* crcs, int64_t* n_members, int64_t* stopped_at) {
  using namespace fqi;
  g_err.clear();
  if (!n_members || !stopped_at) return fail(SCT_FQ_EINVAL, "NULL n_members or stopped_at");
  *n_members = 0;
  *stopped_at = from;
  if (size < 0 || from < 0 || from > size || max_members < 0) return fail(SCT_FQ_EINVAL, "bad size, from or max_members");
  if (size > 0 && !file) return fail(SCT_FQ_EINVAL, "NULL file");
  if (max_members > 0 && (!members || !crcs)) return fail(SCT_FQ_EINVAL, "NULL members or crcs");
  uint64_t off = (uint64_t)from, out = 0;
  const uint64_t end = (uint64_t)size;
  int64_t k = 0;
  while (off < end && k < max_members) {
    const uint8_t* h = file + off;
    bool ok = end - off >= 18 && h[0] == 31 && h[1] == 139 && h[2] == 8 && (h[3] & 4);
    uint32_t csize = 0, xlen = 0;
    if (ok) {
      xlen = rd16(h + 10);
      ok = 12 + (uint64_t)xlen <= end - off;
    }
    if (ok) {
      int64_t bsize = -1;
      uint64_t p = 12;
      while (p + 4 <= 12 + (uint64_t)xlen) {
        const uint16_t slen = rd16(h + p + 2);
        if (h[p] == 66 && h[p + 1] == 67 && slen == 2 && p + 6 <= 12 + (uint64_t)xlen) bsize = rd16(h + p + 4);
        p += 4 + (uint64_t)slen;
      }
      csize = (uint32_t)(bsize + 1);
      // the member lies within the file and holds its header, its extra field and its trailer
      ok = bsize >= 0 && off + csize <= end && csize >= 12 + xlen + 8;
    }
    if (ok) ok = rd32(h + csize - 4) <= SCT_FQ_MAX_ISIZE;
    if (!ok) {
      *n_members = k;
      *stopped_at = (int64_t)off;
      return fail(SCT_FQ_ENOTBGZF, "not BGZF at byte %llu", (unsigned long long)off);
    }
    const uint32_t isize = rd32(h + csize - 4);
    members[k] = sct_fq_member_t{off + 12 + xlen, out, csize - 12 - xlen - 8, isize};
    crcs[k] = rd32(h + csize - 8);
    out += isize;
    off += csize;
    k++;
  }
  *n_members = k;
  *stopped_at = (int64_t)off;
  return SCT_FQ_OK;
}

uint32_t sct_fq_crc32(const uint8_t* data, int64_t n) {
  if (n <= 0 || !data) return 0;
  return fqi::crc32_as_the_wave(data, (uint32_t)n);
}

int sct_fq_inflate_workspace_size(int64_t n_members, size_t* bytes) {
  g_err.clear();
  if (!bytes) return fail(SCT_FQ_EINVAL, "NULL bytes");
  if (n_members < 0) return fail(SCT_FQ_EINVAL, "negative n_members");
  *bytes = fqi::inflate_workspace_of(n_members);
  return SCT_FQ_OK;
}

int sct_fq_inflate(const uint8_t* comp, int64_t comp_bytes, int64_t comp_capacity, const sct_fq_member_t* members,
                   const uint32_t* crcs, int64_t n_members, uint8_t* text, int64_t text_capacity, int64_t text_off,
                   void* workspace, size_t workspace_bytes, uint32_t* status, uint32_t* summary, void* stream) {
  using namespace fqi;
  g_err.clear();
  if (n_members < 0 || n_members > 0x7fffffff) return fail(SCT_FQ_EINVAL, "n_members %lld outside 0..2^31-1", (long long)n_members);
  if (comp_bytes < 0 || text_capacity < 0 || text_off < 0 || text_off > text_capacity)
    return fail(SCT_FQ_EINVAL, "negative size, or text_off outside the text buffer");
  if (!summary || ((uintptr_t)summary & 3)) return fail(SCT_FQ_EINVAL, "summary is NULL or not 4-byte aligned");
  if (n_members > 0) {
    if (!comp || ((uintptr_t)comp & 3)) return fail(SCT_FQ_EINVAL, "comp is NULL or not 4-byte aligned");
    if (comp_capacity < comp_bytes || comp_capacity - comp_bytes < kSlack)
      return fail(SCT_FQ_ESIZE, "comp holds %lld bytes of %lld: the inflate reads ahead, %lld bytes of slack are needed",
                  (long long)comp_bytes, (long long)comp_capacity, (long long)kSlack);
    if (!members || !crcs) return fail(SCT_FQ_EINVAL, "NULL members or crcs");
    if (!status || ((uintptr_t)status & 3)) return fail(SCT_FQ_EINVAL, "status is NULL or not 4-byte aligned");
    if (!workspace || ((uintptr_t)workspace & 7)) return fail(SCT_FQ_EINVAL, "workspace is NULL or not 8-byte aligned");
    if (workspace_bytes < inflate_workspace_of(n_members))
      return fail(SCT_FQ_ESIZE, "workspace of %zu bytes, %zu needed for %lld members", workspace_bytes,
                  inflate_workspace_of(n_members), (long long)n_members);
    const uint64_t room = (uint64_t)(text_capacity - text_off);
    for (int64_t i = 0; i < n_members; i++) {
      const sct_fq_member_t& m = members[i];
      if (m.isize > SCT_FQ_MAX_ISIZE) return fail(SCT_FQ_EINVAL, "member %lld: isize %u is no BGZF member's", (long long)i, m.isize);
      if (m.in_off > (uint64_t)comp_bytes || m.clen > (uint64_t)comp_bytes - m.in_off)
        return fail(SCT_FQ_EINVAL, "member %lld: its deflate data leaves the %lld compressed bytes", (long long)i, (long long)comp_bytes);
      if (m.out_off > room || m.isize > room - m.out_off)
        return fail(SCT_FQ_EINVAL, "member %lld: its payload leaves the text buffer", (long long)i);
      if (m.isize > 0 && !text) return fail(SCT_FQ_EINVAL, "NULL text");
    }
  }
  hipStream_t s = (hipStream_t)stream;
  SCT_LIB_HIP(SCT_FQ_EHIP, hipMemsetAsync(summary, 0, sizeof(uint32_t), s));
  SCT_LIB_HIP(SCT_FQ_EHIP, hipMemsetAsync(summary + 1, 0xff, sizeof(uint32_t), s));
  if (n_members == 0) return SCT_FQ_OK;
  gb::Member* d_mem = (gb::Member*)workspace;
  uint32_t* d_crc = (uint32_t*)(d_mem + n_members);
  SCT_LIB_HIP(SCT_FQ_EHIP, hipMemsetAsync(const_cast<uint8_t*>(comp) + comp_bytes, 0, (size_t)kSlack, s));
  SCT_LIB_HIP(SCT_FQ_EHIP, hipMemcpyAsync(d_mem, members, (size_t)n_members * sizeof(gb::Member), hipMemcpyHostToDevice, s));
  SCT_LIB_HIP(SCT_FQ_EHIP, hipMemcpyAsync(d_crc, crcs, (size_t)n_members * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  uint8_t* dst = text ? text + text_off : text;
  hipLaunchKernelGGL(gb::k_inflate, dim3((unsigned)n_members), dim3(64), 0, s, comp, (const gb::Member*)d_mem, dst, status);
  SCT_LIB_HIP(SCT_FQ_EHIP, hipGetLastError());
  hipLaunchKernelGGL(k_fq_crc32, dim3((unsigned)n_members), dim3(64), 0, s, (const uint8_t*)dst, (const gb::Member*)d_mem,
                     (const uint32_t*)d_crc, status, summary);
  SCT_LIB_HIP(SCT_FQ_EHIP, hipGetLastError());
  return SCT_FQ_OK;
}

}  // extern "C"

#endif  // __HIPCC__
