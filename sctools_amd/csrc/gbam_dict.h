// gbam_dict.h -- the three dictionaries (CB / UB / GE, or the tags a mode names).  On the device: the
// open-addressing tables the parse kernels intern into (Dicts, intern), their growth and the move of a
// window's strings to the arena (k_rehash, k_promote), and the kernels that turn slot ids into ranks.  On
// the host: the tables' state over a parse (ParseState, parse_begin, ensure_tables, promote) and the
// ranking that ends every parse (dictionaries_impl).
#pragma once
#include <string>
#include <string_view>
#include <thread>
#include <vector>

#include "gbam_util.h"
#include "gbam_window.h"

namespace gb {

// Interning tables.  An entry is (off << 28) | (len << 16) | 16 hash bits, off 35 bits, bit 63
// set when the string lies in the window payload U (else in the arena A, where k_promote moves the
// strings a window inserted before its payload is replaced).  Inserts of a window are listed in
// newl[k] (newc[2k] entries, newc[2k + 1] bytes) for k_promote; newl null: no list (one window).
struct Dicts {
  unsigned long long* table[3];
  uint64_t mask[3];
  const uint8_t* A;
  uint32_t* newl[3];
  unsigned long long* newc;
};
constexpr unsigned long long kInU = 1ull << 63;
__device__ __forceinline__ uint64_t ent_off(unsigned long long e) { return (e & ~kInU) >> 28; }
__device__ __forceinline__ uint32_t ent_len(unsigned long long e) { return (uint32_t)(e >> 16) & 0xfff; }
__device__ __forceinline__ const uint8_t* ent_src(unsigned long long e, const uint8_t* U, const uint8_t* A) {
  return (e & kInU) ? U : A;
}

__device__ __forceinline__ uint64_t hash_str(const uint8_t* U, uint64_t off, uint32_t n) {
  uint64_t h = 1469598103934665603ull;
  for (uint32_t k = 0; k < n; k++) h = (h ^ U[off + k]) * 1099511628211ull;
  h ^= h >> 29;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 32;
  return h;
}

__device__ __forceinline__ bool str_eq2(const uint8_t* X, uint64_t a, const uint8_t* U, uint64_t b, uint32_t n) {
  for (uint32_t k = 0; k < n; k++)
    if (X[a + k] != U[b + k]) return false;
  return true;
}

// slot id of the string U[off, off+n) (inserted if new); -1: not internable here (host)
__device__ int32_t intern(const Dicts& D, int k, const uint8_t* U, uint64_t off, uint32_t n) {
  unsigned long long* __restrict__ table = D.table[k];
  const uint64_t mask = D.mask[k];
  if (n > 4095 || off >= (1ull << 35)) return -1;
  for (uint32_t j = 0; j < n; j++)
    if (U[off + j] >= 0x80) return -1;  // "replace"-decoded bytes: ranked on the host path
  const uint64_t h = hash_str(U, off, n);
  const uint64_t tag = (h >> 48) | 1;  // never 0 with off, n -- the empty slot is 0
  const unsigned long long mine = kInU | (off << 28) | ((uint64_t)n << 16) | tag;
  uint64_t slot = h & mask;
  while (true) {
    unsigned long long cur = __hip_atomic_load(&table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0) {
      const unsigned long long prev = atomicCAS(&table[slot], 0ull, mine);
      if (prev == 0) {
        if (D.newl[k]) {  // listed for k_promote
          D.newl[k][atomicAdd(&D.newc[2 * k], 1ull)] = (uint32_t)slot;
          atomicAdd(&D.newc[2 * k + 1], (unsigned long long)n);
        }
        return (int32_t)slot;
      }
      cur = prev;
    }
    if ((cur & 0xffff) == tag && ent_len(cur) == n && str_eq2(ent_src(cur, U, D.A), ent_off(cur), U, off, n))
      return (int32_t)slot;
    slot = (slot + 1) & mask;
  }
}

// The strings a window inserted move to the arena (its payload is about to be replaced): entry i of
// the list gets arena bytes at *cursor (any order) and its table entry is rewritten to point there.
__global__ void k_promote(unsigned long long* __restrict__ table, const uint32_t* __restrict__ list, uint64_t n_new,
                          const uint8_t* __restrict__ U, uint8_t* __restrict__ A,
                          unsigned long long* __restrict__ cursor) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_new) return;
  const uint32_t slot = list[i];
  const unsigned long long e = table[slot];
  const uint32_t n = ent_len(e);
  const uint64_t src = ent_off(e);
  const uint64_t dst = atomicAdd(cursor, (unsigned long long)n);
  for (uint32_t k = 0; k < n; k++) A[dst + k] = U[src + k];
  table[slot] = (dst << 28) | (e & 0xfffffffull);
}

// A table grown to twice (or more) its capacity: every entry re-inserted (its hash recomputed from
// its bytes), map[old slot] = new slot, for k_remap_slots over the columns already written.
__global__ void k_rehash(const unsigned long long* __restrict__ old, uint64_t old_cap,
                         unsigned long long* __restrict__ tab, uint64_t mask, const uint8_t* __restrict__ U,
                         const uint8_t* __restrict__ A, int32_t* __restrict__ map) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= old_cap) return;
  const unsigned long long e = old[i];
  if (!e) return;
  const uint64_t h = hash_str(ent_src(e, U, A), ent_off(e), ent_len(e));
  uint64_t slot = h & mask;
  while (atomicCAS(&tab[slot], 0ull, e) != 0ull) slot = (slot + 1) & mask;  // every entry is distinct
  map[i] = (int32_t)slot;
}
__global__ void k_apply_map(int32_t* __restrict__ col, uint64_t n, const int32_t* __restrict__ map) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) col[i] = map[col[i]];
}
__global__ void k_remap_slots(int32_t* __restrict__ col, uint64_t n, const int32_t* __restrict__ map) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t v = col[i];
  if (v >= 0) col[i] = map[v];
}

// ---------------- dictionaries ----------------
__global__ void k_occupied(const unsigned long long* __restrict__ table, uint64_t cap, uint32_t* __restrict__ occ) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cap) occ[i] = table[i] != 0;
}
__global__ void k_compact(const unsigned long long* __restrict__ table, uint64_t cap,
                          const uint32_t* __restrict__ dense, uint64_t* __restrict__ uent,
                          uint32_t* __restrict__ ulen) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  const unsigned long long v = table[i];
  if (!v) return;
  uent[dense[i]] = v;
  ulen[dense[i]] = ent_len(v);
}
__global__ void k_pack(const uint8_t* __restrict__ U, const uint8_t* __restrict__ A, const uint64_t* __restrict__ uent,
                       const uint64_t* __restrict__ boff, uint32_t n, uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long e = uent[i];
  const uint8_t* src = ent_src(e, U, A);
  const uint64_t s = ent_off(e), o = boff[i];
  for (uint32_t k = 0; k < ent_len(e); k++) out[o + k] = src[s + k];
}
// Dictionaries ranked on the device (round 4): a string of <= 16 bytes compares in Python's order
// (code points = bytes for the ASCII the device path admits) exactly as its big-endian, zero-padded
// 16-byte key (no dictionary string holds a NUL), so two stable 64-bit radix sorts (low word, then
// high) give the ranks.  *too_long: some string is longer (the host sort ranks that dictionary).
__global__ void k_strkey(const uint8_t* __restrict__ U, const uint8_t* __restrict__ A,
                         const uint64_t* __restrict__ uent, uint32_t n, uint64_t* __restrict__ khi,
                         uint64_t* __restrict__ klo, uint32_t* __restrict__ idx, uint32_t* __restrict__ too_long) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long e = uent[i];
  const uint32_t len = ent_len(e);
  if (len > 16) atomicOr(too_long, 1u);
  const uint8_t* src = ent_src(e, U, A) + ent_off(e);
  uint64_t hi = 0, lo = 0;
  for (uint32_t k = 0; k < 16 && k < len; k++) {
    const uint64_t b = src[k];
    if (k < 8)
      hi |= b << (56 - 8 * k);
    else
      lo |= b << (56 - 8 * (k - 8));
  }
  khi[i] = hi;
  klo[i] = lo;
  idx[i] = i;
}
__global__ void k_gather_key(const uint64_t* __restrict__ key, const uint32_t* __restrict__ idx, uint32_t n,
                             uint64_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = key[idx[i]];
}
// ranked order -> rank of every dense id, and the entries / lengths in ranked order
__global__ void k_rank_order(const uint32_t* __restrict__ order, const uint64_t* __restrict__ uent, uint32_t n,
                             int32_t hn, int32_t* __restrict__ rank, uint64_t* __restrict__ uent2,
                             uint32_t* __restrict__ ulen2) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint32_t i = order[r];
  rank[i] = (int32_t)r + hn;
  const unsigned long long e = uent[i];
  uent2[r] = e;
  ulen2[r] = ent_len(e);
}

__global__ void k_remap(int32_t* __restrict__ col, uint64_t n, const uint32_t* __restrict__ dense,
                        const int32_t* __restrict__ rank) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t v = col[i];
  col[i] = v < 0 ? 0 : rank[dense[v]];
}

}  // namespace gb

namespace {

// Python's sorted() on the strings bytes[off[i], off[i + 1]): their indices in ranked order
std::vector<uint32_t> rank_strings(const std::string& bytes, const std::vector<uint64_t>& off) {
  const size_t n = off.size() - 1;
  std::vector<uint32_t> order(n);
  for (size_t i = 0; i < n; i++) order[i] = (uint32_t)i;
  auto sv = [&](uint32_t i) { return std::string_view(bytes.data() + off[i], off[i + 1] - off[i]); };
  auto less = [&](uint32_t a, uint32_t b) { return sv(a) < sv(b); };
  const size_t T = std::min<size_t>(16, std::max<size_t>(1, n / 65536));
  if (T <= 1) {
    std::sort(order.begin(), order.end(), less);
  } else {  // sorted chunks, merged pairwise
    std::vector<size_t> cut(T + 1);
    for (size_t t = 0; t <= T; t++) cut[t] = n * t / T;
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; t++)
      th.emplace_back([&, t] { std::sort(order.begin() + cut[t], order.begin() + cut[t + 1], less); });
    for (auto& x : th) x.join();
    for (size_t w = 1; w < T; w *= 2) {
      th.clear();
      for (size_t t = 0; t + w < T; t += 2 * w) {
        const size_t a = cut[t], m = cut[t + w], b = cut[std::min(T, t + 2 * w)];
        th.emplace_back([&, a, m, b] {
          std::inplace_merge(order.begin() + a, order.begin() + m, order.begin() + b, less);
        });
      }
      for (auto& x : th) x.join();
    }
  }
  return order;
}

// The three device hash tables (2^k slots each) and the parse flags: [0] a record needs the host
// decoder, [1..3] some record lacks CB / UB / GE.  Several windows: tables grown before a window
// that could fill them past half (k_rehash), new strings listed and moved to the arena after each
// window (k_promote).
struct ParseState {
  uint64_t cap[3] = {1024, 1024, 1024};
  uint64_t used[3] = {0, 0, 0};  // entries
  DevBuf<unsigned long long> tab[3];
  DevBuf<uint8_t> arena;
  uint64_t arena_used = 0;
  DevBuf<uint32_t> newl[3];
  DevBuf<unsigned long long> newc;
  Dicts D{};
  DevBuf<uint32_t> flags;
  uint32_t fl[4] = {0, 0, 0, 0};
};

int parse_begin(sct_gbam* G, ParseState& P) {
  HIPOK(hipSetDevice(G->device));
  uint64_t biggest = 0;
  for (const WinInfo& w : G->win) biggest = std::max<uint64_t>(biggest, w.n_rec);
  const uint64_t first = G->kept ? (uint64_t)G->n : biggest;
  for (int k = 0; k < 3; k++) {
    while (P.cap[k] < 2 * first) P.cap[k] <<= 1;
    if (P.cap[k] > (1ull << 31)) return gfail(SCT_GBAM_HOST, "too many records for the device tables");
    HIPOK(P.tab[k].alloc(P.cap[k]));
    HIPOK(hipMemsetAsync(P.tab[k].p, 0, P.cap[k] * sizeof(unsigned long long), G->st));
    P.D.table[k] = P.tab[k].p;
    P.D.mask[k] = P.cap[k] - 1;
    if (!G->kept) {
      HIPOK(P.newl[k].alloc(biggest + 1));
      P.D.newl[k] = P.newl[k].p;
    }
  }
  if (!G->kept) {
    HIPOK(P.newc.alloc(6));
    HIPOK(hipMemsetAsync(P.newc.p, 0, 6 * sizeof(unsigned long long), G->st));
    P.D.newc = P.newc.p;
    HIPOK(P.arena.alloc(1 << 20));
  }
  P.D.A = P.arena.p;
  HIPOK(P.flags.alloc(4));
  HIPOK(hipMemsetAsync(P.flags.p, 0, 4 * sizeof(uint32_t), G->st));
  return SCT_BAM_OK;
}

// Before a window of `n_rec` records: every table keeps at most half its slots filled even if all
// the window's strings are new; a grown table renumbers its slots in the columns already written.
int ensure_tables(sct_gbam* G, ParseState& P, int32_t* const colk[3], uint64_t written, uint64_t n_rec) {
  hipStream_t st = G->st;
  for (int k = 0; k < 3; k++) {
    uint64_t cap = P.cap[k];
    while (cap < 2 * (P.used[k] + n_rec)) cap <<= 1;
    if (cap == P.cap[k]) continue;
    if (cap > (1ull << 31)) return gfail(SCT_GBAM_HOST, "too many distinct strings for the device tables");
    DevBuf<unsigned long long> nt;
    DevBuf<int32_t> map;
    HIPOK(nt.alloc(cap));
    HIPOK(map.alloc(P.cap[k]));
    HIPOK(hipMemsetAsync(nt.p, 0, cap * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_rehash, dim3(grid(P.cap[k], 256)), dim3(256), 0, st, P.tab[k].p, P.cap[k], nt.p, cap - 1,
                       G->u.p, P.arena.p, map.p);
    if (written)
      hipLaunchKernelGGL(k_remap_slots, dim3(grid(written, 256)), dim3(256), 0, st, colk[k], written, map.p);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(st));
    P.tab[k].swap(nt);
    P.cap[k] = cap;
    P.D.table[k] = P.tab[k].p;
    P.D.mask[k] = cap - 1;
  }
  return SCT_BAM_OK;
}

// After a window's parse: its new strings move from the payload to the arena.
int promote(sct_gbam* G, ParseState& P) {
  hipStream_t st = G->st;
  unsigned long long c[6];
  HIPOK(hipMemcpyAsync(c, P.newc.p, sizeof(c), hipMemcpyDeviceToHost, st));
  HIPOK(hipStreamSynchronize(st));
  const uint64_t bytes = c[1] + c[3] + c[5];
  if (P.arena_used + bytes > P.arena.n) {
    DevBuf<uint8_t> na;
    HIPOK(na.alloc(std::max<uint64_t>(2 * P.arena.n, P.arena_used + bytes)));
    if (P.arena_used) HIPOK(hipMemcpyAsync(na.p, P.arena.p, P.arena_used, hipMemcpyDeviceToDevice, st));
    HIPOK(hipStreamSynchronize(st));
    P.arena.swap(na);
    P.D.A = P.arena.p;
  }
  if (P.arena_used + bytes >= (1ull << 35)) return gfail(SCT_GBAM_HOST, "dictionary strings past 32 GB");
  DevBuf<unsigned long long> cursor;
  HIPOK(cursor.alloc(1));
  unsigned long long cur = P.arena_used;
  HIPOK(hipMemcpyAsync(cursor.p, &cur, sizeof(cur), hipMemcpyHostToDevice, st));
  for (int k = 0; k < 3; k++)
    if (c[2 * k])
      hipLaunchKernelGGL(k_promote, dim3(grid(c[2 * k], 256)), dim3(256), 0, st, P.tab[k].p, P.newl[k].p,
                         (uint64_t)c[2 * k], G->u.p, P.arena.p, cursor.p);
  HIPOK(hipGetLastError());
  HIPOK(hipMemsetAsync(P.newc.p, 0, 6 * sizeof(unsigned long long), st));
  HIPOK(hipStreamSynchronize(st));
  for (int k = 0; k < 3; k++) P.used[k] += c[2 * k];
  P.arena_used += bytes;
  return SCT_BAM_OK;
}

// ---------------- ranking: slot ids -> ranks in Python's sorted() order, the missing value first ----------------
// What ranking one dictionary works on: its table compacted to dense ids, the order found for them, and the
// column of slot ids.  Per dictionary: compact_table, the order (rank_on_device, or rank_on_host when a string
// is longer than 16 bytes), finish_ranked.
struct DictRank {
  int k = 0;                    // which dictionary
  int32_t hn = 0;               // 1: some record lacks the tag -- rank 0 is the missing value
  int32_t* col = nullptr;       // the column: a slot id per record, or < 0 for the missing value
  uint64_t nu = 0;              // distinct strings
  DevBuf<uint32_t> occ, dense;  // per slot: occupied; its dense id
  DevBuf<uint64_t> uent, boff;  // per dense id: the table entry; the string's offset among the packed ones (nu + 1)
  DevBuf<uint32_t> ulen;        // ... and its length (nu + 1: a last 0, for the scan's total)
  DevBuf<uint32_t> order;       // the dense ids in ranked order
  // rank_on_device's keys, second index buffer and flag: freed with the rest, after the tail's last wait (a
  // hipFree between the sorts and the tail would wait for the device there)
  DevBuf<uint64_t> khi, klo, kt;
  DevBuf<uint32_t> ib, flag;
  DevBuf<uint8_t>& tmp;         // scan and sort scratch, shared by the three dictionaries
  explicit DictRank(DevBuf<uint8_t>& scratch) : tmp(scratch) {}
};
constexpr int kRankOnHost = 1000;  // rank_on_device: a string is too long for its keys (no error)

int compact_table(sct_gbam* G, ParseState& P, DictRank& R) {
  hipStream_t st = G->st;
  const uint64_t cap = P.cap[R.k];
  HIPOK(R.occ.alloc(cap));
  HIPOK(R.dense.alloc(cap));
  hipLaunchKernelGGL(k_occupied, dim3(grid(cap, 256)), dim3(256), 0, st, P.tab[R.k].p, cap, R.occ.p);
  HIPOK(exclusive_sum(R.occ.p, R.dense.p, cap, st, R.tmp));
  uint32_t last[2] = {0, 0};
  HIPOK(hipMemcpyAsync(&last[0], R.dense.p + cap - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPOK(hipMemcpyAsync(&last[1], R.occ.p + cap - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPOK(hipStreamSynchronize(st));
  R.nu = (uint64_t)last[0] + last[1];
  HIPOK(R.uent.alloc(R.nu));
  HIPOK(R.ulen.alloc(R.nu + 1));
  HIPOK(R.boff.alloc(R.nu + 1));
  HIPOK(hipMemsetAsync(R.ulen.p + R.nu, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_compact, dim3(grid(cap, 256)), dim3(256), 0, st, P.tab[R.k].p, cap, R.dense.p, R.uent.p,
                     R.ulen.p);
  return SCT_BAM_OK;
}

// R.order on the device (gb::k_strkey): kRankOnHost if a string is longer than 16 bytes.
int rank_on_device(sct_gbam* G, ParseState& P, DictRank& R) {
  hipStream_t st = G->st;
  const uint32_t nu = (uint32_t)R.nu;
  DevBuf<uint64_t>&khi = R.khi, &klo = R.klo, &kt = R.kt;
  DevBuf<uint32_t>&ia = R.order, &ib = R.ib, &flag = R.flag;
  HIPOK(khi.alloc(nu));
  HIPOK(klo.alloc(nu));
  HIPOK(kt.alloc(nu));
  HIPOK(ia.alloc(nu));
  HIPOK(ib.alloc(nu));
  HIPOK(flag.alloc(1));
  HIPOK(hipMemsetAsync(flag.p, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_strkey, dim3(grid(nu, 256)), dim3(256), 0, st, G->u.p, P.arena.p, R.uent.p, nu, khi.p, klo.p,
                     ia.p, flag.p);
  uint32_t too_long = 0;
  HIPOK(hipMemcpyAsync(&too_long, flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPOK(hipStreamSynchronize(st));
  if (too_long) return kRankOnHost;
  // stable LSD: by the low word, then by the high word
  size_t tb = 0;
  HIPOK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, klo.p, kt.p, ia.p, ib.p, (int)nu, 0, 64, st));
  if (R.tmp.n < tb) HIPOK(R.tmp.alloc(tb));
  HIPOK(hipcub::DeviceRadixSort::SortPairs(R.tmp.p, tb, klo.p, kt.p, ia.p, ib.p, (int)nu, 0, 64, st));
  hipLaunchKernelGGL(k_gather_key, dim3(grid(nu, 256)), dim3(256), 0, st, khi.p, ib.p, nu, klo.p);
  HIPOK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, klo.p, kt.p, ib.p, ia.p, (int)nu, 0, 64, st));
  if (R.tmp.n < tb) HIPOK(R.tmp.alloc(tb));
  HIPOK(hipcub::DeviceRadixSort::SortPairs(R.tmp.p, tb, klo.p, kt.p, ib.p, ia.p, (int)nu, 0, 64, st));
  return SCT_BAM_OK;
}

// R.order from the host: the strings packed as they lie in the table, copied over and sorted there.
int rank_on_host(sct_gbam* G, ParseState& P, DictRank& R) {
  hipStream_t st = G->st;
  const uint64_t nu = R.nu;
  R.khi.free(), R.klo.free(), R.kt.free(), R.ib.free(), R.flag.free();  // (what a declined device ranking left)
  HIPOK(exclusive_sum(R.ulen.p, R.boff.p, nu + 1, st, R.tmp));
  std::vector<uint64_t> hoff(nu + 1);
  HIPOK(hipMemcpyAsync(hoff.data(), R.boff.p, (nu + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIPOK(hipStreamSynchronize(st));
  const uint64_t total = hoff[nu];
  DevBuf<uint8_t> packed;
  HIPOK(packed.alloc(total));
  if (nu)
    hipLaunchKernelGGL(k_pack, dim3(grid(nu, 256)), dim3(256), 0, st, G->u.p, P.arena.p, R.uent.p, R.boff.p,
                       (uint32_t)nu, packed.p);
  std::string bytes(total, '\0');
  if (total) HIPOK(hipMemcpyAsync(&bytes[0], packed.p, total, hipMemcpyDeviceToHost, st));
  HIPOK(hipStreamSynchronize(st));
  const std::vector<uint32_t> order = rank_strings(bytes, hoff);
  HIPOK(R.order.alloc(nu));
  if (nu) HIPOK(hipMemcpyAsync(R.order.p, order.data(), nu * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIPOK(hipStreamSynchronize(st));  // (`order` leaves scope)
  return SCT_BAM_OK;
}

// The tail both routes share: the strings packed in ranked order and copied, with their offsets, to
// G->dict_bytes / dict_off (after the missing value's empty entry where there is one), and the column's slot ids
// turned into ranks.
int finish_ranked(sct_gbam* G, ParseState& P, DictRank& R) {
  hipStream_t st = G->st;
  const uint32_t nu = (uint32_t)R.nu;
  const uint64_t n = (uint64_t)G->n;
  DevBuf<int32_t> rank_d;
  DevBuf<uint64_t> uent2;
  HIPOK(rank_d.alloc(nu));
  HIPOK(uent2.alloc(nu));
  // the ranks, and the entries and lengths in ranked order; then their byte offsets
  if (nu)
    hipLaunchKernelGGL(k_rank_order, dim3(grid(nu, 256)), dim3(256), 0, st, R.order.p, R.uent.p, nu, R.hn, rank_d.p,
                       uent2.p, R.ulen.p);
  HIPOK(exclusive_sum(R.ulen.p, R.boff.p, (uint64_t)nu + 1, st, R.tmp));
  uint64_t total = 0;
  HIPOK(hipMemcpyAsync(&total, R.boff.p + nu, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIPOK(hipStreamSynchronize(st));
  DevBuf<uint8_t> packed;
  HIPOK(packed.alloc(total));
  if (nu)
    hipLaunchKernelGGL(k_pack, dim3(grid(nu, 256)), dim3(256), 0, st, G->u.p, P.arena.p, uent2.p, R.boff.p, nu,
                       packed.p);
  std::string& db = G->dict_bytes[R.k];
  std::vector<int64_t>& dof = G->dict_off[R.k];
  db.assign(total, '\0');
  dof.assign((size_t)nu + 1 + (R.hn ? 1 : 0), 0);
  if (total) HIPOK(hipMemcpyAsync(&db[0], packed.p, total, hipMemcpyDeviceToHost, st));
  static_assert(sizeof(int64_t) == sizeof(uint64_t), "offsets copied as they are");
  HIPOK(hipMemcpyAsync(dof.data() + (R.hn ? 1 : 0), R.boff.p, ((size_t)nu + 1) * sizeof(uint64_t),
                       hipMemcpyDeviceToHost, st));
  if (n) hipLaunchKernelGGL(k_remap, dim3(grid(n, 256)), dim3(256), 0, st, R.col, n, R.dense.p, rank_d.p);
  HIPOK(hipGetLastError());
  HIPOK(hipStreamSynchronize(st));
  return SCT_BAM_OK;
}

// The interned ids -> ranks in Python's sorted() order (None first), and the ranked strings.
int dictionaries_impl(sct_gbam* G, ParseState& P, int32_t* const colk[3]) {
  const double t1 = now();
  DevBuf<uint8_t> tmp;
  for (int k = 0; k < 3; k++) {
    DictRank R(tmp);
    R.k = k, R.col = colk[k];
    R.hn = G->has_none[k] = P.fl[1 + k] ? 1 : 0;
    int rc = compact_table(G, P, R);
    if (rc) return rc;
    rc = R.nu > 0 && R.nu < (1ull << 31) ? rank_on_device(G, P, R) : kRankOnHost;
    if (rc == kRankOnHost) rc = rank_on_host(G, P, R);
    if (rc) return rc;
    rc = finish_ranked(G, P, R);
    if (rc) return rc;
  }
  G->t[sct_gbam::T_DICTIONARIES] = now() - t1;
  return SCT_BAM_OK;
}

}  // namespace
