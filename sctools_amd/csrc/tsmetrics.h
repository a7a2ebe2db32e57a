// tsmetrics.h -- the native TagSort gatherer (fastqpreprocessing/src/metricgatherer.cpp) on
// records already sorted by (first, second, third) tag rank.
//
// The reference walks the sorted lines once (MetricGatherer::ingestLine, metricgatherer.cpp:152-200):
// lines whose first tag is dropped are skipped; a row is closed before a line whose first tag
// differs from `prev`, the first tag of the last MAPPED line counted so far (empty at the start).
// Rows are therefore delimited by per-entity facts, where an entity is a run of one kept first tag:
//   start[e], end[e]  the entity's records,
//   fm[e]             its first mapped record (kTsNoMapped if none),
//   prev[e]           the nearest earlier entity with a mapped record (-1 if none): the value of
//                     `prev` for every record of e up to and including fm[e].
// With prev[e] >= 0, each record of e up to fm[e] closes a row named prev[e] (so every unmapped
// read that begins an entity is a row of its own); with prev[e] < 0 (the leading entities) no
// record of e closes anything.  A scan over the ENTITIES (dictionary sized, not record sized)
// turns this into each entity's first row, and a record's row is a formula of these five values.
//
// Kernels:
//   ts_mark     per record: start / end / fm of its entity; checks the order and the id ranges
//   ts_ent_scan one block:  prev[e] (running max) and rowbase[e] (running sum) over the entities
//   ts_records  per record: its row; the row's start and name; its four stream values; the integer counters (molecules from
//               triplet run heads, fragments by a scan of short triplet runs or a hash table for
//               long ones, the second / third tag histogram through a hash table)
//   ts_frag_slots / ts_k1_slots  per table slot: distinct keys, keys seen once / more than once
//   ts_chains   one wave (block) per row: count, sum += x, sum2 += x * x of the four float streams in
//               record order, x = the six-digit text round trip of the float32 ratio (tsround.h),
//               computed per record by ts_records so that the serial walk only adds
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "tsround.h"
#include "util.h"

namespace sct {

constexpr int kTsFragScan = 32;  // triplet runs up to this long resolve their fragments by scanning the run
constexpr int32_t kTsNoMapped = 0x7F7F7F7F;  // fm[e] of an entity without a mapped record (a byte fill)
constexpr uint32_t kTsEmpty = 0xFFFFFFFFu;   // free hash slot (a byte fill)
constexpr int kTsFlush = 17;                 // columns 0 .. 16 of a row are per-record sums
constexpr int kTsScanPer = 8, kTsScanBlock = 1024;
constexpr uint32_t kTsSkipped = 0xFFFFFFFFu;  // xv[i].x of a dropped record (no ts_roundtrip result: tsround.h)

struct TsEnt {
  int32_t* start;
  int32_t* end;
  int32_t* fm;
  int32_t* prev;
  int32_t* rowbase;
};

struct TsCtl {
  long long boundaries;         // rows closed before the last one
  long long last_mapped;        // the last entity with a mapped record (-1: none): the final row's name
  unsigned long long unsorted;  // first record ordered before its predecessor (~0: none)
  unsigned long long bad_id;    // first record with an id outside its dictionary (~0: none)
};

struct TsTable {
  uint32_t* owner;  // record index of the slot's key, kTsEmpty if free
  uint32_t* cnt;    // records with that key
  uint32_t mask;    // slots - 1 (a power of two >= 2 * n_records)
};

struct TsLayout {
  size_t start, end, fm, prev, rowbase, ctl, row_start, xv, f_owner, f_cnt, k_owner, k_cnt, total;
  uint32_t slots;
};

inline TsLayout ts_layout(int64_t n, int64_t n_first, int64_t capacity) {
  TsLayout L{};
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += align_up(bytes);
    return o;
  };
  const size_t ne = (size_t)(n_first > 0 ? n_first : 1);
  L.start = take(4 * ne), L.end = take(4 * ne), L.fm = take(4 * ne), L.prev = take(4 * ne), L.rowbase = take(4 * ne);
  L.ctl = take(sizeof(TsCtl));
  L.row_start = take(4 * (size_t)(capacity + 1));
  L.xv = take(16 * (size_t)(n > 0 ? n : 1));
  uint64_t slots = 1024;
  while (slots < 2 * (uint64_t)n) slots <<= 1;
  L.slots = (uint32_t)slots;
  L.f_owner = take(4 * slots), L.f_cnt = take(4 * slots), L.k_owner = take(4 * slots), L.k_cnt = take(4 * slots);
  L.total = off;
  return L;
}

__device__ __forceinline__ uint32_t ts_mix(uint32_t h) {
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  h *= 0x297A2D39u;
  h ^= h >> 15;
  return h;
}

// ---- per record: the entity's extent and first mapped record; order and id checks ----
__global__ void __launch_bounds__(kBlock) k_ts_mark(sct_records_t r, int64_t n, uint32_t n_first, uint32_t n_second,
                                                    uint32_t n_third, const uint8_t* __restrict__ drop, TsEnt ent,
                                                    TsCtl* __restrict__ ctl) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t e = r.cell[i], u = r.umi[i], g = r.gene[i];
  if ((uint32_t)e >= n_first || (uint32_t)u >= n_second || (uint32_t)g >= n_third) {
    atomicMin(&ctl->bad_id, (unsigned long long)i);
    return;
  }
  int32_t pe = -1;
  bool p_unmapped = true;
  if (i > 0) {
    pe = r.cell[i - 1];
    const int32_t pu = r.umi[i - 1], pg = r.gene[i - 1];
    if (pe > e || (pe == e && (pu > u || (pu == u && pg > g)))) atomicMin(&ctl->unsorted, (unsigned long long)i);
    p_unmapped = (r.bits[i - 1] & SCT_B_UNMAPPED) != 0;
  }
  if (drop[e]) return;
  const bool head = pe != e;
  if (head) ent.start[e] = (int32_t)i;
  if (i == n - 1 || r.cell[i + 1] != e) ent.end[e] = (int32_t)(i + 1);
  // (the plain, possibly stale read only skips atomics that could not lower the value: fm[e] never
  // grows.  Without it the 5 % of a 10M-record entity's records that begin a mapped stretch all hit one
  // address: 21.7 ms at 100M records in gene order, 3.9 ms with it)
  if (!(r.bits[i] & SCT_B_UNMAPPED) && (head || p_unmapped) && (int32_t)i < ent.fm[e]) atomicMin(&ent.fm[e], (int32_t)i);
}

// ---- one block over the entities: prev[e], rowbase[e], the totals ----
__global__ void __launch_bounds__(kTsScanBlock) k_ts_ent_scan(TsEnt ent, int32_t n_first, TsCtl* __restrict__ ctl) {
  __shared__ uint32_t s_max[kTsScanBlock / kWave];
  __shared__ long long s_sum[kTsScanBlock / kWave + 1];
  __shared__ uint32_t s_carry;
  uint32_t carry = 0;  // 1 + the last entity with a mapped record so far
  long long rows = 0;  // rows closed so far
  for (int64_t base = 0; base < n_first; base += kTsScanBlock * kTsScanPer) {
    const int64_t e0 = base + (int64_t)threadIdx.x * kTsScanPer;
    uint32_t hm[kTsScanPer];
    int32_t st[kTsScanPer], fm[kTsScanPer];
    uint32_t lmax = 0;
#pragma unroll
    for (int k = 0; k < kTsScanPer; k++) {
      const int64_t e = e0 + k;
      st[k] = e < n_first ? ent.start[e] : -1;
      fm[k] = e < n_first ? ent.fm[e] : kTsNoMapped;
      hm[k] = (st[k] >= 0 && fm[k] != kTsNoMapped) ? (uint32_t)(e + 1) : 0u;
      lmax = hm[k] > lmax ? hm[k] : lmax;
    }
    const uint32_t before = block_exclusive_max_n<kTsScanBlock>(lmax, s_max);
    uint32_t run = before > carry ? before : carry;
    long long nb[kTsScanPer], lsum = 0;
#pragma unroll
    for (int k = 0; k < kTsScanPer; k++) {
      const int64_t e = e0 + k;
      nb[k] = 0;
      if (e < n_first) {
        ent.prev[e] = (int32_t)run - 1;
        if (st[k] >= 0 && run > 0) {
          const int32_t last = ent.end[e] - 1;
          nb[k] = (long long)((fm[k] < last ? fm[k] : last) - st[k] + 1);
        }
      }
      lsum += nb[k];
      run = hm[k] > run ? hm[k] : run;
    }
    long long total = 0;
    long long ex = block_exclusive_scan_n<kTsScanBlock, long long>(lsum, &total, s_sum);
#pragma unroll
    for (int k = 0; k < kTsScanPer; k++) {
      const int64_t e = e0 + k;
      // row ids are int32: the caller's capacity check (rows <= capacity < 2^31) runs before they are used
      if (e < n_first) ent.rowbase[e] = (int32_t)(rows + ex);
      ex += nb[k];
    }
    if (threadIdx.x == kTsScanBlock - 1) s_carry = run;
    __syncthreads();
    carry = s_carry;
    rows += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ctl->boundaries = rows;
    ctl->last_mapped = (long long)carry - 1;
  }
}

// the row of kept record i of entity e
__device__ __forceinline__ int32_t ts_row(const TsEnt& ent, int32_t e, int32_t i) {
  const int32_t rb = ent.rowbase[e];
  if (ent.prev[e] < 0) return rb;
  const int32_t fm = ent.fm[e];
  return rb + (i < fm ? i : fm) - ent.start[e] + 1;
}

// Counts record i (weight w) under its key: the slot's owner is the first record that claimed it;
// `same(o)` says whether record o has i's key.  The table has >= 2 n slots, so a probe ends.
template <typename Same>
__device__ __forceinline__ void ts_insert(const TsTable& t, uint32_t h, uint32_t i, uint32_t w, Same same) {
  uint32_t p = h & t.mask;
  for (;;) {
    const uint32_t o = atomicCAS(&t.owner[p], kTsEmpty, i);
    if (o == kTsEmpty || o == i || same(o)) {
      atomicAdd(&t.cnt[p], w);
      return;
    }
    p = (p + 1) & t.mask;
  }
}

// Wave-cooperative add of per-lane counters v[0..K) into column i of row `row` (per lane): one
// wave-uniform iteration per distinct row among the members, the members' values summed over the
// wave and added by lanes 0..K-1 with one atomic instruction.  Every lane must call it.
template <int K>
__device__ __forceinline__ void ts_flush(int32_t (&v)[K], bool member, int32_t row, int64_t* __restrict__ out) {
  static_assert(K <= kWave, "one lane per column");
  const int lane = threadIdx.x & (kWave - 1);
  uint64_t pending = __ballot(member);
  while (pending) {
    const int lead = __ffsll((unsigned long long)pending) - 1;
    const int32_t rl = __shfl(row, lead);
    const bool in = member && row == rl;
    int64_t mine = 0;
#pragma unroll
    for (int i = 0; i < K; i++) {
      const int32_t tot = wave_sum_dpp(in ? v[i] : 0);
      mine = (lane == i) ? (int64_t)tot : mine;
    }
    if (lane < K && mine)
      atomicAdd((unsigned long long*)&out[(int64_t)rl * SCT_TS_NI + lane], (unsigned long long)mine);
    pending &= ~__ballot(in);
  }
}

// ---- per record: row, row start and name, counters, fragments, the tag histogram ----
template <bool kCell>
__global__ void __launch_bounds__(kBlock) k_ts_records(sct_records_t r, int64_t n, const uint8_t* __restrict__ drop,
                                                       const uint8_t* __restrict__ mito, TsEnt ent,
                                                       int32_t* __restrict__ row_start, TsTable ft, TsTable kt,
                                                       uint4* __restrict__ xv, int64_t* __restrict__ out) {
  const int64_t i64 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  const bool live = i64 < n;
  const int32_t i = (int32_t)i64;
  const int32_t last = (int32_t)(n - 1);
  const int32_t e = live ? r.cell[i] : 0;
  const bool kept = live && !drop[e];
  int32_t v[kTsFlush];
#pragma unroll
  for (int k = 0; k < kTsFlush; k++) v[k] = 0;
  int32_t row = -1, tag = 0;
  if (live && !kept) xv[i] = make_uint4(kTsSkipped, 0u, 0u, 0u);
  if (kept) {
    {  // the four stream values the gatherer sees, for ts_chains
      const uint32_t gl = r.gq_len[i];
      xv[i] = make_uint4(ts_roundtrip(r.uy_gt30[i], r.uy_len[i]), ts_roundtrip(r.gq_gt30[i], gl),
                         ts_roundtrip(r.gq_sum[i], gl), ts_roundtrip(r.cy_gt30[i], r.cy_len[i]));
    }
    const int32_t u = r.umi[i], g = r.gene[i];
    const int32_t prev = ent.prev[e], fm = ent.fm[e];
    const bool bnd = prev >= 0 && i <= fm;  // this record closes a row named prev
    row = ts_row(ent, e, i);
    if (bnd) {
      row_start[row] = i;
      out[(int64_t)(row - 1) * SCT_TS_NI + SCT_TS_I_NAME] = prev;
    }
    tag = kCell ? g : u;
    const uint32_t bits = r.bits[i];
    const uint32_t xf = r.xf[i];
    // a triplet run: equal (first, second, third) inside one row; a record that closes a row begins a run.
    // For a record j of this record's run: is j + 1 / j - 1 in the run too?
    const auto same_as_next = [&](int32_t j) {
      return j < last && r.cell[j + 1] == e && r.umi[j + 1] == u && r.gene[j + 1] == g && !(prev >= 0 && j + 1 <= fm);
    };
    const auto same_as_prev = [&](int32_t j) {
      return j > 0 && r.cell[j - 1] == e && r.umi[j - 1] == u && r.gene[j - 1] == g && !(prev >= 0 && j <= fm);
    };
    const bool head = !same_as_prev(i);
    const bool tail = !same_as_next(i);
    v[SCT_TS_I_N_READS] = 1;
    v[SCT_TS_I_PERFECT_MOLECULE_BARCODES] = (bits & SCT_B_PERFECT_UMI) ? 1 : 0;
    v[SCT_TS_I_N_MOLECULES] = head;
    v[SCT_TS_I_MOLECULES_SINGLE] = head && tail;
    if (kCell) {
      v[SCT_TS_I_PERFECT_CELL_BARCODES] = (bits & SCT_B_PERFECT_CB) ? 1 : 0;
      v[SCT_TS_I_READS_MAPPED_INTERGENIC] = xf == SCT_XF_INTERGENIC;
      v[SCT_TS_I_READS_UNMAPPED] = xf == SCT_XF_ABSENT;
      v[SCT_TS_I_N_MITO_MOLECULES] = mito[g] ? 1 : 0;
    }
    if (!(bits & SCT_B_UNMAPPED)) {
      v[SCT_TS_I_READS_MAPPED_EXONIC] = xf == SCT_XF_CODING;
      v[SCT_TS_I_READS_MAPPED_INTRONIC] = xf == SCT_XF_INTRONIC;
      v[SCT_TS_I_READS_MAPPED_UTR] = xf == SCT_XF_UTR;
      v[SCT_TS_I_READS_MAPPED_UNIQUELY] = (bits & SCT_B_NH1) ? 1 : 0;
      v[SCT_TS_I_READS_MAPPED_MULTIPLE] = (bits & SCT_B_NH1) ? 0 : 1;
      v[SCT_TS_I_DUPLICATE_READS] = (bits & SCT_B_DUPLICATE) ? 1 : 0;
      v[SCT_TS_I_SPLICED_READS] = (bits & SCT_B_SPLICED) ? 1 : 0;
      // fragments: distinct (reference, position, strand) among the run's mapped records
      const int32_t ref = r.ref[i], pos = r.pos[i];
      const uint32_t rev = bits & SCT_B_REVERSE;
      const auto same_frag = [&](int32_t j) {
        const uint32_t bj = r.bits[j];
        return !(bj & SCT_B_UNMAPPED) && (bj & SCT_B_REVERSE) == rev && r.ref[j] == ref && r.pos[j] == pos;
      };
      // the run is scanned when it has at most kTsFragScan records: a steps back to its head, then
      // up to kTsFragScan - 1 - a steps forward to its tail (every record of a run decides alike)
      int a = 0, b = 0;
      bool at_head = head, at_tail = tail, before = false, after = false;
      for (int32_t j = i; !at_head && a < kTsFragScan - 1;) {
        j--, a++;
        before |= same_frag(j);
        at_head = !same_as_prev(j);
      }
      if (at_head)
        for (int32_t j = i; !at_tail && a + b < kTsFragScan - 1;) {
          j++, b++;
          after |= same_frag(j);
          at_tail = !same_as_next(j);
        }
      if (at_head && at_tail) {
        v[SCT_TS_I_N_FRAGMENTS] = !before;
        v[SCT_TS_I_FRAGMENTS_SINGLE] = !before && !after;
      } else {
        // a longer run: at most one per triplet (the records that close rows are runs of one), so the
        // triplet stands for the run in the key
        const uint32_t h = ts_mix(frag_hash(ref, pos, rev) ^ ((uint32_t)e * 0x9E3779B1u) ^
                                  ts_mix((uint32_t)u * 0x85EBCA77u ^ (uint32_t)g));
        ts_insert(ft, h, (uint32_t)i, 1u, [&](uint32_t o) {
          return r.cell[o] == e && r.umi[o] == u && r.gene[o] == g && same_frag((int32_t)o);
        });
      }
    }
  }
  // the histogram of the third (cell) or second (gene) tag per row: neighbouring lanes with one key insert once
  const int32_t prow = __shfl_up(row, 1), ptag = __shfl_up(tag, 1);
  const bool leader = kept && (lane == 0 || prow != row || ptag != tag);
  const uint64_t brk = __ballot(leader) | ~__ballot(kept);
  if (leader) {
    const uint64_t rest = lane == kWave - 1 ? 0ull : brk >> (lane + 1);
    const uint32_t w = rest ? (uint32_t)__ffsll((unsigned long long)rest) : (uint32_t)(kWave - lane);
    const uint32_t h = ts_mix((uint32_t)row * 0x9E3779B1u ^ ts_mix((uint32_t)tag * 0x85EBCA77u + 1u));
    ts_insert(kt, h, (uint32_t)i, w, [&](uint32_t o) {
      const int32_t eo = r.cell[o];
      return (kCell ? r.gene[o] : r.umi[o]) == tag && ts_row(ent, eo, (int32_t)o) == row;
    });
  }
  ts_flush<kTsFlush>(v, kept, row, out);
}

__global__ void __launch_bounds__(kBlock) k_ts_frag_slots(sct_records_t r, TsEnt ent, TsTable t,
                                                          int64_t* __restrict__ out) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;  // slots <= 2^32 / 2: no overflow
  if (p > t.mask) return;
  const uint32_t o = t.owner[p];
  if (o == kTsEmpty) return;
  int64_t* row = out + (int64_t)ts_row(ent, r.cell[o], (int32_t)o) * SCT_TS_NI;
  atomicAdd((unsigned long long*)&row[SCT_TS_I_N_FRAGMENTS], 1ull);
  if (t.cnt[p] == 1) atomicAdd((unsigned long long*)&row[SCT_TS_I_FRAGMENTS_SINGLE], 1ull);
}

template <bool kCell>
__global__ void __launch_bounds__(kBlock) k_ts_k1_slots(sct_records_t r, const uint8_t* __restrict__ mito, TsEnt ent,
                                                        TsTable t, int64_t* __restrict__ out) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p > t.mask) return;
  const uint32_t o = t.owner[p];
  if (o == kTsEmpty) return;
  int64_t* row = out + (int64_t)ts_row(ent, r.cell[o], (int32_t)o) * SCT_TS_NI;
  atomicAdd((unsigned long long*)&row[SCT_TS_I_N_K1], 1ull);
  if (t.cnt[p] > 1) atomicAdd((unsigned long long*)&row[SCT_TS_I_K1_MULTIPLE], 1ull);
  if (kCell && mito[r.gene[o]]) atomicAdd((unsigned long long*)&row[SCT_TS_I_N_MITO_GENES], 1ull);
}

// ---- one wave per row: the four streams' sums in record order ----
// ts_records left every record's four values (float32 patterns; kTsSkipped for a dropped record) in
// xv.  The wave takes 64 records at a time, packs the kept ones' values as doubles into LDS, and while
// the next 64 are on their way from memory lane s < 4 walks stream s's sum chain and lane 4 + s its
// sum-of-squares chain over the slice: one add per record and chain, in record order.  x * x of a
// float32 value is exact in double, so sum2 += x * x rounds once, fused or not.
__global__ void __launch_bounds__(kWave) k_ts_chains(const uint4* __restrict__ xv, int64_t n, int64_t rows,
                                                      const int32_t* __restrict__ row_start,
                                                      double* __restrict__ sums) {
  __shared__ double s_x[4][kWave];
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;  // a block is one wave: the barriers below are wave-uniform
  const int64_t lo = row == 0 ? 0 : row_start[row];
  const int64_t hi = row + 1 < rows ? row_start[row + 1] : n;
  const int st = lane & 3;
  const bool square = lane >= 4;
  const uint4 none = make_uint4(kTsSkipped, 0u, 0u, 0u);
  double acc = 0.0;
  long long count = 0;
  uint4 cur = lo + lane < hi ? xv[lo + lane] : none;
  for (int64_t base = lo; base < hi; base += kWave) {
    const bool kept = cur.x != kTsSkipped;
    const uint64_t km = __ballot(kept);
    const int k = __popcll(km);
    if (kept) {
      const int at = __popcll(km & ((1ull << lane) - 1));
      s_x[0][at] = (double)__uint_as_float(cur.x);
      s_x[1][at] = (double)__uint_as_float(cur.y);
      s_x[2][at] = (double)__uint_as_float(cur.z);
      s_x[3][at] = (double)__uint_as_float(cur.w);
    }
    __syncthreads();
    const int64_t nx = base + kWave + lane;
    cur = nx < hi ? xv[nx] : none;  // in flight during the walk
    const double* xs = &s_x[st][0];
#pragma unroll 8
    for (int j = 0; j < k; j++) {
      const double x = xs[j];
      acc += square ? x * x : x;
    }
    count += k;
    __syncthreads();
  }
  if (lane < 8) sums[row * SCT_TS_NF + st * 3 + (square ? 2 : 1)] = acc;
  if (lane < 4) sums[row * SCT_TS_NF + st * 3] = (double)count;
}

}  // namespace sct
