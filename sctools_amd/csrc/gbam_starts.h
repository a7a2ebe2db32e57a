// gbam_starts.h -- finding the record starts of an inflated window: per member a guessed start (plausible,
// k_guess), the walk along block_size (k_walk), and the repair rounds that replace a guess by the
// previous member's landing until every start agrees (k_agree, k_fix); the host side that drives them
// in pass 1 (prove_window: starts proven, records counted, the carry taken) and in pass 2
// (restart_window: a window inflated again and walked from its proven starts).
#pragma once
#include <string>
#include <vector>

#include "gbam_util.h"
#include "gbam_window.h"

namespace gb {

// four records chain from p the way alignment records do (SAM/BAM spec 4.2): a hint only --
// k_walk's agreement check decides
// open_end: U ends inside a record that continues in the next window (a chain reaching the end
// cannot be disproved)
// (every field is checked before a record running past U is accepted, so an arbitrary offset whose
// first four bytes read as a huge block_size does not pass for a start at an open end; U has kPad
// readable bytes past ulen)
__device__ bool plausible(const uint8_t* U, uint64_t ulen, uint64_t p, bool open_end) {
  for (int j = 0; j < 4; j++) {
    if (p == ulen) return true;
    if (p + 36 > ulen) return open_end && j > 0;
    const uint32_t bs = u32(U, p);
    if (bs < 33 || bs > (1u << 28)) return false;
    const uint64_t d = p + 4;
    if ((int32_t)u32(U, d) < -1 || (int32_t)u32(U, d + 4) < -1) return false;
    const uint32_t lrn = U[d + 8];
    if (lrn == 0 || 32 + lrn > bs) return false;
    if (d + 32 + lrn > ulen) return open_end && j > 0;
    if (U[d + 32 + lrn - 1] != 0) return false;
    for (uint32_t q = 0; q + 1 < lrn; q++) {
      const uint32_t c = U[d + 32 + q];
      if (c < 33 || c > 126) return false;
    }
    const uint64_t need = 32ull + lrn + 4ull * u16(U, d + 12) + (u32(U, d + 16) + 1ull) / 2 + u32(U, d + 16);
    if (need > bs) return false;
    if (p + 4 + bs > ulen) return open_end;  // the rest of this record is in the next window
    p = d + bs;
  }
  return true;
}

// S[m] for members mH < m < n_mem: the first plausible record start at or after O[m] (member mH
// too when H is kUnknown: a part's first record, proven later against the previous part's walk).
// check_end: the walk must land exactly on ulen (S[n_mem]); else the end is found, not checked.
// open_end: U ends inside a record that continues in the next window.
__global__ void k_guess(const uint8_t* __restrict__ U, uint64_t ulen, const uint64_t* __restrict__ O, uint32_t mH,
                        uint32_t n_mem, uint64_t H, uint64_t* __restrict__ S, uint32_t open_end, uint32_t check_end) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m == 0) S[n_mem] = check_end ? ulen : kUnknown;
  if (m < mH || m >= n_mem) return;
  if (m == mH && H != kUnknown) {
    S[m] = H;
    return;
  }
  const uint64_t p0 = O[m];
  uint64_t s = p0 >= ulen ? ulen : kUnknown;
  const uint64_t e = min(ulen, p0 + kScan);
  for (uint64_t p = p0; p < e; p++)
    if (plausible(U, ulen, p, open_end != 0)) {
      s = p;
      break;
    }
  S[m] = s;
}

// Walk member m's records from S[m] up to the first start at or after O[m+1]: cnt[m] records,
// land[m+1] the landing (kBadWalk: a record runs past U), last[m] the start of its last record.
// With `starts`, write the offsets.  open_end: a walk stops at a record running past U (it continues
// in the next window) and lands on its start.
__global__ void k_walk(const uint8_t* __restrict__ U, uint64_t ulen, const uint64_t* __restrict__ O, uint32_t mH,
                       uint32_t n_mem, const uint64_t* __restrict__ S, uint32_t* __restrict__ cnt,
                       uint64_t* __restrict__ land, uint64_t* __restrict__ starts, const uint64_t* __restrict__ base,
                       uint64_t* __restrict__ last, uint32_t open_end) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n_mem) return;
  if (m < mH) {
    cnt[m] = 0;
    land[m + 1] = kUnknown;
    if (last) last[m] = kUnknown;
    return;
  }
  uint64_t p = S[m];
  if (p == kUnknown) {
    cnt[m] = 0;
    land[m + 1] = kUnknown;
    if (last) last[m] = kUnknown;
    return;
  }
  const uint64_t end = O[m + 1];
  const bool open = open_end != 0;  // (a long record may cut through several members)
  uint32_t n = 0;
  uint64_t lp = kUnknown;
  uint64_t* out = starts ? starts + base[m] : nullptr;
  while (p < end) {
    if (p + 4 > ulen) {
      p = open ? p : kBadWalk;
      break;
    }
    const uint64_t bs = u32(U, p);
    if (p + 4 + bs > ulen) {
      p = open ? p : kBadWalk;
      break;
    }
    if (out) out[n] = p;
    lp = p;
    n++;
    p += 4 + bs;
  }
  cnt[m] = n;
  land[m + 1] = p;
  if (last) last[m] = lp;
}

// ag[m]: member m's start agrees with its predecessor's landing this round (mH: exact by
// construction).  Computed before k_fix rewrites any start.
__global__ void k_agree(uint32_t mH, uint32_t n_mem, const uint64_t* __restrict__ S,
                        const uint64_t* __restrict__ land, uint8_t* __restrict__ ag) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m > n_mem) return;
  ag[m] = m < mH ? 0 : (m == mH || land[m] == S[m]) ? 1 : 0;
}

// Replace a start that disagrees with its predecessor's landing -- only when the predecessor's own
// start agreed (a landing walked from a wrong start would carry the error forward one member per
// round); count the disagreements (S[n_mem] = ulen is fixed: a landing elsewhere stays one).
// Each round the agreeing prefix from mH grows past at least one more member, and a run of k
// wrong guesses takes k rounds.
__global__ void k_fix(uint32_t mH, uint32_t n_mem, uint64_t* __restrict__ S, const uint64_t* __restrict__ land,
                      const uint8_t* __restrict__ ag, uint32_t* __restrict__ n_bad) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m <= mH || m > n_mem) return;
  const uint64_t l = land[m];
  if (l == S[m]) return;
  if (m == n_mem && S[m] == kUnknown) return;  // an open end (the record continues in the next window)
  if (m < n_mem && ag[m - 1] && l != kUnknown && l != kBadWalk) S[m] = l;
  atomicAdd(n_bad, 1u);
}

__global__ void k_u32_to_u64(const uint32_t* __restrict__ a, uint64_t* __restrict__ b, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) b[i] = a[i];
}

}  // namespace gb

namespace {

// The walk members' offsets in window w's payload: member 0 begins at 0 (its carry), the others
// where their payload lands; the end is where the window's own members end (the lookahead holds no
// record of the window's, only the rest of one cut at the end).
std::vector<uint64_t> walk_offsets(const sct_gbam* G, const WinInfo& w) {
  const uint32_t nm = w.m_hi - w.m_lo;
  std::vector<uint64_t> o(nm + 1);
  for (uint32_t k = 0; k <= nm; k++) o[k] = k == 0 ? 0 : w.carry.size() + G->O[w.m_lo + k] - G->O[w.m_lo];
  return o;
}
inline uint64_t abs_of(const sct_gbam* G, const WinInfo& w, uint64_t x) { return G->O[w.m_lo] - w.carry.size() + x; }

// Pass 1 on the inflated window: prove the members' record starts (guess, walk, repair rounds),
// count the records, and take the carry for the next window.  With `starts` (one window), also
// write every record start.
int prove_window(sct_gbam* G, WinInfo& w, WinInfo* next, DevBuf<uint64_t>* starts) {
  hipStream_t st = G->st;
  const uint32_t nm = w.m_hi - w.m_lo;
  const uint32_t open = w.last ? 0u : 1u, check = w.check ? 1u : 0u;
  const std::vector<uint64_t> Oh = walk_offsets(G, w);
  DevBuf<uint64_t> d_O, d_S, d_land, d_base, d_last;
  DevBuf<uint32_t> d_cnt, d_flag;
  DevBuf<uint8_t> d_ag;
  HIPOK(d_O.alloc(nm + 1));
  HIPOK(d_S.alloc(nm + 1));
  HIPOK(d_land.alloc(nm + 1));
  HIPOK(d_last.alloc(nm));
  HIPOK(d_cnt.alloc(nm));
  HIPOK(d_base.alloc(nm + 1));
  HIPOK(d_ag.alloc(nm + 1));
  HIPOK(d_flag.alloc(1));
  HIPOK(hipMemcpyAsync(d_O.p, Oh.data(), (nm + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_guess, dim3(grid(nm, 64)), dim3(64), 0, st, G->u.p, w.ulen, d_O.p, w.mH, nm, w.H, d_S.p, open,
                     check);
  int rounds = 0;
  for (;; rounds++) {
    if (rounds == kStartRounds) return gfail(SCT_GBAM_HOST, "record starts did not converge");
    hipLaunchKernelGGL(k_walk, dim3(grid(nm, 64)), dim3(64), 0, st, G->u.p, w.ulen, d_O.p, w.mH, nm, d_S.p, d_cnt.p,
                       d_land.p, (uint64_t*)nullptr, (const uint64_t*)nullptr, d_last.p, open);
    HIPOK(hipMemsetAsync(d_flag.p, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_agree, dim3(grid(nm + 1, 256)), dim3(256), 0, st, w.mH, nm, (const uint64_t*)d_S.p,
                       (const uint64_t*)d_land.p, d_ag.p);
    hipLaunchKernelGGL(k_fix, dim3(grid(nm + 1, 256)), dim3(256), 0, st, w.mH, nm, d_S.p, d_land.p,
                       (const uint8_t*)d_ag.p, d_flag.p);
    uint32_t nbad = 0;
    HIPOK(hipMemcpyAsync(&nbad, d_flag.p, sizeof(nbad), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    if (nbad == 0) break;
    uint64_t lastland = 0;
    HIPOK(hipMemcpy(&lastland, d_land.p + nm, sizeof(lastland), hipMemcpyDeviceToHost));
    // only the final landing disagrees and every start before it is proven: a truncated record
    if (w.check && nbad == 1 && lastland != w.ulen && rounds > 0) {
      uint64_t s_last = 0;
      HIPOK(hipMemcpy(&s_last, d_S.p + nm - 1, sizeof(s_last), hipMemcpyDeviceToHost));
      if (s_last != kUnknown) return gfail(SCT_GBAM_HOST, "truncated BAM record");
    }
  }
  G->t[sct_gbam::T_START_ROUNDS] += rounds;
  std::vector<uint32_t> cnt(nm);
  std::vector<uint64_t> last(nm);
  w.S.resize(nm + 1);
  uint64_t land_end = 0;
  HIPOK(hipMemcpyAsync(cnt.data(), d_cnt.p, nm * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPOK(hipMemcpyAsync(last.data(), d_last.p, nm * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIPOK(hipMemcpyAsync(w.S.data(), d_S.p, (nm + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIPOK(hipMemcpyAsync(&land_end, d_land.p + nm, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIPOK(hipStreamSynchronize(st));
  uint64_t total = 0, lastrec = kUnknown;
  for (uint32_t k = 0; k < nm; k++) {
    total += cnt[k];
    if (cnt[k]) lastrec = last[k];
  }
  if (w.has_prev && total == 0) return gfail(SCT_GBAM_HOST, "record starts did not converge");
  w.n_rec = total - (w.has_prev ? 1 : 0);
  if (&w == &G->win.front()) G->first_abs = w.S[w.mH] == kUnknown ? -1 : (int64_t)abs_of(G, w, w.S[w.mH]);
  if (w.last) {
    if (land_end == kUnknown || land_end == kBadWalk) return gfail(SCT_GBAM_HOST, "a part's last record runs past its lookahead");
    G->land_abs = (int64_t)abs_of(G, w, land_end);
  }
  if (next) {  // the carry: from the last complete record (or the cut record alone) to the end
    if (lastrec == kUnknown) return gfail(SCT_GBAM_HOST, "a BAM record longer than a decode window");
    const uint64_t from = lastrec;
    next->carry.resize(w.ulen - from);
    if (!next->carry.empty())
      HIPOK(hipMemcpy(&next->carry[0], G->u.p + from, w.ulen - from, hipMemcpyDeviceToHost));
    next->has_prev = true;
    next->mH = 0;
    next->H = 0;
  }
  if (starts) {
    std::vector<uint64_t> base(nm + 1, 0);
    for (uint32_t k = 0; k < nm; k++) base[k + 1] = base[k] + cnt[k];
    HIPOK(starts->alloc(total));
    HIPOK(hipMemcpyAsync(d_base.p, base.data(), (nm + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_walk, dim3(grid(nm, 64)), dim3(64), 0, st, G->u.p, w.ulen, d_O.p, w.mH, nm, d_S.p, d_cnt.p,
                       d_land.p, starts->p, (const uint64_t*)d_base.p, (uint64_t*)nullptr, open);
    HIPOK(hipStreamSynchronize(st));
  }
  return SCT_BAM_OK;
}

// Pass 2 of a window that pass 1 did not keep: inflate it again and write its record starts from the
// proven member starts (no guesses).  *total: records in the window's payload (a carried one included).
int restart_window(sct_gbam* G, WinInfo& w, DevBuf<uint64_t>& starts, uint64_t* total) {
  int rc = inflate_window(G, w, true);
  if (rc) return rc;
  const double t1 = now();
  hipStream_t st = G->st;
  const uint32_t nm = w.m_hi - w.m_lo;
  const uint32_t open = w.last ? 0u : 1u;
  const std::vector<uint64_t> Oh = walk_offsets(G, w);
  DevBuf<uint64_t> d_O, d_S, d_land, d_base, d_cnt64;
  DevBuf<uint32_t> d_cnt;
  DevBuf<uint8_t> tmp;
  HIPOK(d_O.alloc(nm + 1));
  HIPOK(d_S.alloc(nm + 1));
  HIPOK(d_land.alloc(nm + 1));
  HIPOK(d_cnt.alloc(nm));
  HIPOK(d_cnt64.alloc(nm + 1));
  HIPOK(d_base.alloc(nm + 1));
  HIPOK(hipMemcpyAsync(d_O.p, Oh.data(), (nm + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIPOK(hipMemcpyAsync(d_S.p, w.S.data(), (nm + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_walk, dim3(grid(nm, 64)), dim3(64), 0, st, G->u.p, w.ulen, d_O.p, w.mH, nm, d_S.p, d_cnt.p,
                     d_land.p, (uint64_t*)nullptr, (const uint64_t*)nullptr, (uint64_t*)nullptr, open);
  HIPOK(hipMemsetAsync(d_cnt64.p + nm, 0, sizeof(uint64_t), st));
  hipLaunchKernelGGL(k_u32_to_u64, dim3(grid(nm, 256)), dim3(256), 0, st, d_cnt.p, d_cnt64.p, nm);
  HIPOK(exclusive_sum(d_cnt64.p, d_base.p, nm + 1, st, tmp));
  uint64_t n = 0;
  HIPOK(hipMemcpyAsync(&n, d_base.p + nm, sizeof(n), hipMemcpyDeviceToHost, st));
  HIPOK(hipStreamSynchronize(st));
  if (n != w.n_rec + (w.has_prev ? 1 : 0)) return gfail(SCT_BAM_EIO, "a window's record count changed between passes");
  if (starts.n < n) HIPOK(starts.alloc(n));
  hipLaunchKernelGGL(k_walk, dim3(grid(nm, 64)), dim3(64), 0, st, G->u.p, w.ulen, d_O.p, w.mH, nm, d_S.p, d_cnt.p,
                     d_land.p, starts.p, (const uint64_t*)d_base.p, (uint64_t*)nullptr, open);
  HIPOK(hipGetLastError());
  *total = n;
  G->t[sct_gbam::T_RECORD_STARTS] += now() - t1;
  return SCT_BAM_OK;
}

}  // namespace
