// fqprocess.h -- the sct_fqp_* calls of libsct_fastq.so (include/sct_fastq_process.h): whole lines
// of a counted window, the output shard of every record, a stable partition by shard and the
// output records.  Included at the end of fastq.hip, whose tile scheme, helpers and error state
// it shares.
//
//   k_fqp_lines    one block per 16 KiB tile, as k_extract: the tile's '\n's are listed in LDS by
//                  rank; the '\n' of rank k ends line first[tile] + k, and that line begins after
//                  the '\n' of rank k - 1.  For the tile's first '\n' that one lies in an earlier
//                  tile: the block looks for it backwards from the tile's first byte, 4 KiB (one
//                  16-byte group per thread) at a time -- one step unless a line is longer than
//                  that.  Eight lanes share a line: they look for the identifier's first space
//                  and for a quality byte below 33, eight bytes per lane and step.
//   k_fqp_check    one thread per record: the flags that follow from the three lengths.
//   k_fqp_shard    one block per 256 rows, both columns staged in LDS with 16-byte loads; a thread
//                  hashes its row (libstdc++'s _Hash_bytes) and classes it; three atomics per block.
//   k_fqp_hist     one block per tile of 256 records: records and output bytes per shard in LDS,
//                  flushed with plain stores to [tile][shard].
//   k_fqp_scan     one block per shard walks the tiles 256 at a time: exclusive scan in place, the
//                  shard totals.
//   k_fqp_offsets  one block per tile: a record's offset is its tile's base in its shard plus the
//                  sizes of the tile's earlier records of the same shard (a walk over the tile in
//                  LDS, every lane reading the same word: 128 broadcast reads per record on average).
//   k_fqp_emit_*   sixteen lanes per record, eight bytes per lane and step along each line; in the
//                  tag block two lanes per tag, all eight tags at once.
//
// No kernel keeps a global atomic per record, and every sum is over integers: the output is a
// function of the input.  Plain C++, vector stores.
#include <algorithm>

#include "../../include/sct_fastq_process.h"

namespace {

constexpr int kFqpLineLanes = 8;
constexpr int kFqpLineGroups = kBlock / kFqpLineLanes;
constexpr int kFqpBack = kBlock * 16;  // bytes of one backward step
static_assert(kTile % kFqpBack == 0, "the backward steps start at a tile's first byte and never pass byte 0");
constexpr int kFqpPlanTile = SCT_FQP_PLAN_TILE;
static_assert(kFqpPlanTile == kBlock, "one record per thread in the partition kernels");
constexpr int kFqpMaxShards = SCT_FQP_MAX_SHARDS;
constexpr int kFqpMaxL = SCT_FQP_MAX_BARCODE;
constexpr int kFqpEmitLanes = 16;
constexpr int kFqpEmitRecords = kBlock / kFqpEmitLanes;

struct FqpLinesArgs {
  const uint8_t* text;
  int64_t n;
  int64_t n_records;
  int64_t tiles;
  const uint64_t* first;
  const uint32_t* cnt;
  int64_t* off;
  int32_t* len;
  uint32_t* flags;
  unsigned long long* first_flagged;
};

__device__ __forceinline__ void fqp_raise(uint32_t* flags, unsigned long long* first_flagged, int64_t r, uint32_t bits) {
  atomicOr(flags + (r >> 2), bits << (8 * (int)(r & 3)));
  atomicMin(first_flagged, (unsigned long long)r);
}

// the eight bytes at text[at, at + 8) as a little-endian word; bytes at and past `end` read as `fill`
__device__ __forceinline__ uint64_t fqp_load8(const uint8_t* __restrict__ text, int64_t at, int64_t end, uint8_t fill) {
  uint64_t word;
  if (at + 8 <= end) {
    __builtin_memcpy(&word, text + at, 8);
    return word;
  }
  word = 0x0101010101010101ull * fill;
  for (int i = 0; i < 8; i++)
    if (at + i < end) word = (word & ~(0xffull << (8 * i))) | ((uint64_t)text[at + i] << (8 * i));
  return word;
}

__device__ __forceinline__ int32_t fqp_len32(int64_t v) { return (int32_t)min(v, (int64_t)INT32_MAX); }

__global__ void __launch_bounds__(kBlock) k_fqp_lines(const FqpLinesArgs a) {
  const int64_t base = (int64_t)blockIdx.x * kTile;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
  uint4 m[kGroups];
#pragma unroll
  for (int j = 0; j < kGroups; j++)
    m[j] = group_masks(load_group(a.text, base + ((int64_t)j * kBlock + tid) * 16, a.n));
  __shared__ uint32_t s_seg[kGroups * (kBlock / kWave)];
  __shared__ uint16_t s_off[kRound];
  __shared__ int s_back;
  uint32_t rank0[kGroups];
#pragma unroll
  for (int j = 0; j < kGroups; j++) {
    const uint32_t c = group_count(m[j]);
    const uint32_t incl = wave_inclusive(c);
    rank0[j] = incl - c;
    if (lane == kWave - 1) s_seg[j * (kBlock / kWave) + w] = incl;
  }
  if (tid == 0) s_back = -1;
  __syncthreads();
  uint32_t total = 0;
#pragma unroll
  for (int i = 0; i < kGroups * (kBlock / kWave); i++) {
    const uint32_t x = s_seg[i];
#pragma unroll
    for (int j = 0; j < kGroups; j++)
      if (i < j * (kBlock / kWave) + w) rank0[j] += x;
    total += x;
  }
  if (total == 0) return;  // (the whole block: no line ends here)
  // the last '\n' before the tile, -1 if there is none
  int64_t prev = -1;
  for (int64_t hi = base; hi > 0; hi -= kFqpBack) {
    const int64_t at = hi - kFqpBack + (int64_t)tid * 16;  // >= 0: hi is a multiple of kFqpBack
    const uint4 mk = group_masks(load_group(a.text, at, a.n));
    const uint32_t words[4] = {mk.x, mk.y, mk.z, mk.w};
    for (int q = 3; q >= 0; q--)
      if (words[q]) {
        atomicMax(&s_back, tid * 16 + 4 * q + ((31 - __clz((int)words[q])) >> 3));
        break;
      }
    __syncthreads();
    const int found = s_back;
    __syncthreads();  // nobody adds to s_back again before everybody has read it
    if (found >= 0) {
      prev = hi - kFqpBack + found;
      break;
    }
  }
  const uint64_t first = a.first[blockIdx.x];
  const uint64_t newlines = a.first[a.tiles - 1] + a.cnt[a.tiles - 1];
  // the last record's quality line has no '\n' (the last window of a stream): the '+' line's thread takes it
  const bool open_end = a.n_records > 0 && (uint64_t)(4 * a.n_records - 1) >= newlines;
  const int g = tid / kFqpLineLanes, l = tid % kFqpLineLanes;
  for (uint32_t round = 0; round < total; round += kRound) {
#pragma unroll
    for (int j = 0; j < kGroups; j++) {
      uint32_t rank = rank0[j];
      const uint32_t words[4] = {m[j].x, m[j].y, m[j].z, m[j].w};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        uint32_t bits = words[q];
        while (bits) {
          const int b = (__ffs((int)bits) - 1) >> 3;
          bits &= bits - 1;
          if (rank >= round && rank < round + kRound) s_off[rank - round] = (uint16_t)((j * kBlock + tid) * 16 + 4 * q + b);
          rank++;
        }
      }
    }
    __syncthreads();
    const uint32_t here = min((uint32_t)kRound, total - round);
    for (uint32_t k = g; k < here; k += kFqpLineGroups) {
      const int64_t p = base + s_off[k];  // the '\n' that ends line `line`
      const uint64_t line = first + round + k;
      const int64_t r = (int64_t)(line >> 2);
      int kind = (int)(line & 3);
      if (r >= a.n_records) continue;
      int64_t start = (k > 0 ? base + s_off[k - 1] : prev) + 1, end = p;
      if (kind == 2) {
        if (!(open_end && r == a.n_records - 1)) continue;
        kind = 3, start = p + 1, end = a.n;
      } else if (end > start && a.text[end - 1] == '\r') {
        end--;
      }
      if (kind == 1) {
        if (l == 0) a.off[3 * r + 1] = start, a.len[3 * r + 1] = fqp_len32(end - start);
        continue;
      }
      if (kind == 3) {
        uint32_t low = 0;
        for (int64_t c = start + l * 8; c < end; c += kFqpLineLanes * 8) {
          const uint64_t word = fqp_load8(a.text, c, end, 33);
#pragma unroll
          for (int i = 0; i < 8; i++) low |= (uint32_t)((uint8_t)(word >> (8 * i)) < 33);
        }
#pragma unroll
        for (int o = kFqpLineLanes / 2; o > 0; o >>= 1) low |= __shfl_xor(low, o, kFqpLineLanes);
        if (l == 0) {
          a.off[3 * r + 2] = start, a.len[3 * r + 2] = fqp_len32(end - start);
          if (low) fqp_raise(a.flags, a.first_flagged, r, SCT_FQP_LOW_QUALITY);
        }
        continue;
      }
      // the name line: the identifier follows the '@' and ends before the first space
      const bool at_sign = start < end && a.text[start] == '@';
      const int64_t id0 = start + (at_sign ? 1 : 0);
      const int64_t look = min(end, id0 + SCT_FQP_MAX_IDENTIFIER + 1);
      int64_t space = INT64_MAX;
      for (int64_t c = id0 + l * 8; c < look; c += kFqpLineLanes * 8) {
        const uint64_t word = fqp_load8(a.text, c, look, 0);
#pragma unroll
        for (int i = 7; i >= 0; i--)
          if ((uint8_t)(word >> (8 * i)) == ' ' && c + i < look) space = c + i;
        if (space != INT64_MAX) break;  // (the lane's later bytes lie further on)
      }
#pragma unroll
      for (int o = kFqpLineLanes / 2; o > 0; o >>= 1) space = min(space, (int64_t)__shfl_xor((long long)space, o, kFqpLineLanes));
      if (l == 0) {
        a.off[3 * r] = id0, a.len[3 * r] = fqp_len32((space != INT64_MAX ? space : end) - id0);
        if (!at_sign) fqp_raise(a.flags, a.first_flagged, r, SCT_FQP_BAD_NAME);
      }
    }
    prev = base + s_off[here - 1];
    __syncthreads();  // the next round overwrites s_off
  }
}

__global__ void __launch_bounds__(kBlock) k_fqp_check(const int32_t* __restrict__ len, int64_t n_records,
                                                      uint32_t* __restrict__ flags, unsigned long long* first_flagged) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= n_records) return;
  const int32_t id = len[3 * r], seq = len[3 * r + 1], qual = len[3 * r + 2];
  uint32_t bits = 0;
  if (id < 1 || id > SCT_FQP_MAX_IDENTIFIER) bits |= SCT_FQP_BAD_IDENTIFIER;
  if (seq < 1) bits |= SCT_FQP_EMPTY_SEQUENCE;
  if (seq != qual) bits |= SCT_FQP_LENGTH_MISMATCH;
  if (bits) fqp_raise(flags, first_flagged, r, bits);
}

// ---- shard ----

__device__ __forceinline__ uint64_t fqp_shift_mix(uint64_t v) { return v ^ (v >> 47); }

// libstdc++'s _Hash_bytes (64-bit) of `len` bytes with the seed of std::hash<std::string>
__device__ __forceinline__ uint64_t fqp_hash(const uint8_t* s, int len) {
  const uint64_t mul = 0xc6a4a7935bd1e995ull;
  uint64_t h = 0xc70f6907ull ^ ((uint64_t)len * mul);
  int at = 0;
  for (; at + 8 <= len; at += 8) {
    uint64_t d = 0;
    for (int i = 0; i < 8; i++) d |= (uint64_t)s[at + i] << (8 * i);
    h ^= fqp_shift_mix(d * mul) * mul;
    h *= mul;
  }
  if (len & 7) {
    uint64_t d = 0;
    for (int i = 0; at + i < len; i++) d |= (uint64_t)s[at + i] << (8 * i);
    h ^= d;
    h *= mul;
  }
  h = fqp_shift_mix(h) * mul;
  return fqp_shift_mix(h);
}

__global__ void __launch_bounds__(kBlock) k_fqp_shard(const uint8_t* __restrict__ raw, const uint8_t* __restrict__ corrected,
                                                      const int32_t* __restrict__ index, int64_t n, int L, uint32_t n_shards,
                                                      int32_t* __restrict__ shard, unsigned long long* __restrict__ counts) {
  __shared__ uint4 s_raw4[kBlock * kFqpMaxL / 16];
  __shared__ uint4 s_cor4[kBlock * kFqpMaxL / 16];
  __shared__ uint32_t s_class[3];
  const uint8_t* s_raw = reinterpret_cast<const uint8_t*>(s_raw4);
  const uint8_t* s_cor = reinterpret_cast<const uint8_t*>(s_cor4);
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kBlock;
  const int rows = (int)min((int64_t)kBlock, n - row0);
  const int groups = (rows * L + 15) >> 4;  // at most kBlock * kFqpMaxL / 16
  for (int g = tid; g < groups; g += kBlock) {
    s_raw4[g] = load_group(raw, row0 * L + (int64_t)g * 16, n * L);
    if (corrected) s_cor4[g] = load_group(corrected, row0 * L + (int64_t)g * 16, n * L);
  }
  if (tid < 3) s_class[tid] = 0;
  __syncthreads();
  if (tid < rows) {
    const bool correctable = index && corrected && index[row0 + tid] >= 0;
    const uint8_t* mine = s_raw + tid * L;
    int klass = 2;
    if (correctable) {
      const uint8_t* fixed = s_cor + tid * L;
      bool same = true;
      for (int j = 0; j < L; j++) same &= fixed[j] == mine[j];
      klass = same ? 0 : 1;
      mine = fixed;
    }
    shard[row0 + tid] = (int32_t)(fqp_hash(mine, L) % n_shards);
    atomicAdd(&s_class[klass], 1u);
  }
  __syncthreads();
  if (tid < 3 && s_class[tid]) atomicAdd(&counts[tid], (unsigned long long)s_class[tid]);
}

// ---- plan ----

struct FqpRecords {
  int64_t n;
  const uint8_t* r2_text;
  int64_t r2_bytes;
  const int64_t* r2_off;
  const int32_t* r2_len;
  const uint8_t* i1_text;
  int64_t i1_bytes;
  const int64_t* i1_off;
  const int32_t* i1_len;
  const uint8_t *cr, *cy, *ur, *uy, *cb;
  const int32_t* cb_index;
  const int32_t* shard;
  int32_t Lc, Lu, n_shards, format;
};

__device__ __forceinline__ int64_t fqp_len(const int32_t* len, int64_t at) { return (int64_t)max(len[at], 0); }

__device__ __forceinline__ int fqp_shard_of(const FqpRecords& a, int64_t i) {
  return min(max(a.shard[i], 0), a.n_shards - 1);  // (a shard outside the range would index past the tables)
}

__device__ __forceinline__ bool fqp_has_cb(const FqpRecords& a, int64_t i) { return a.cb_index && a.cb && a.cb_index[i] >= 0; }

// the bytes of record i's outputs: the BAM record, or the R1 text and the R2 text
__device__ __forceinline__ void fqp_sizes(const FqpRecords& a, int64_t i, int64_t* s0, int64_t* s1) {
  const int64_t id = fqp_len(a.r2_len, 3 * i), seq = fqp_len(a.r2_len, 3 * i + 1), qual = fqp_len(a.r2_len, 3 * i + 2);
  if (a.format == SCT_FQP_BAM) {
    int64_t s = 36 + id + 1 + (seq + 1) / 2 + seq + 5 + 2 * (4 + a.Lc) + 2 * (4 + a.Lu);
    if (a.i1_len) s += 8 + fqp_len(a.i1_len, 3 * i + 1) + fqp_len(a.i1_len, 3 * i + 2);
    if (fqp_has_cb(a, i)) s += 4 + a.Lc;
    *s0 = s, *s1 = 0;
  } else {
    *s0 = id + 2 + 2 * (a.Lc + a.Lu + 1) + 2;
    *s1 = id + 2 + seq + 1 + 2 + qual + 1;
  }
}

struct FqpPlanSpace {
  unsigned long long *b0, *b1;  // [tile][shard] bytes of output 0 and 1 (b1 NULL in BAM mode)
  uint32_t* cnt;                // [tile][shard] records
};

__global__ void __launch_bounds__(kBlock) k_fqp_hist(const FqpRecords a, const FqpPlanSpace ws) {
  __shared__ uint32_t s_cnt[kFqpMaxShards];
  __shared__ unsigned long long s_b0[kFqpMaxShards], s_b1[kFqpMaxShards];
  const int tid = threadIdx.x;
  for (int s = tid; s < a.n_shards; s += kBlock) s_cnt[s] = 0, s_b0[s] = 0, s_b1[s] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kFqpPlanTile + tid;
  if (i < a.n) {
    int64_t s0, s1;
    fqp_sizes(a, i, &s0, &s1);
    const int s = fqp_shard_of(a, i);
    atomicAdd(&s_cnt[s], 1u);
    atomicAdd(&s_b0[s], (unsigned long long)s0);
    if (ws.b1) atomicAdd(&s_b1[s], (unsigned long long)s1);
  }
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * a.n_shards;
  for (int s = tid; s < a.n_shards; s += kBlock) {
    ws.cnt[row + s] = s_cnt[s];
    ws.b0[row + s] = s_b0[s];
    if (ws.b1) ws.b1[row + s] = s_b1[s];
  }
}

// One block per shard walks the tiles 256 at a time: an exclusive scan of the shard's column of
// [tile][shard] in place (a wave scan, the four wave totals through LDS, a running carry), and the
// shard's totals.  The loads of a round are independent of one another; only the carry goes from
// round to round.
__global__ void __launch_bounds__(kBlock) k_fqp_scan(const FqpPlanSpace ws, int64_t tiles, int n_shards,
                                                     int64_t* __restrict__ shard_counts, int64_t* __restrict__ shard_bytes) {
  constexpr int kWaves = kBlock / kWave;
  __shared__ unsigned long long s_w[3][kWaves];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
  unsigned long long carry[3] = {0, 0, 0};
  for (int64_t t0 = 0; t0 < tiles; t0 += kBlock) {
    const int64_t t = t0 + tid, at = t * n_shards + s;
    unsigned long long v[3] = {0, 0, 0}, incl[3];
    if (t < tiles) {
      v[0] = ws.cnt[at], v[1] = ws.b0[at];
      if (ws.b1) v[2] = ws.b1[at];
    }
#pragma unroll
    for (int q = 0; q < 3; q++) {
      incl[q] = wave_inclusive(v[q]);
      if (lane == kWave - 1) s_w[q][w] = incl[q];
    }
    __syncthreads();
    unsigned long long before[3], total[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
      before[q] = carry[q], total[q] = 0;
#pragma unroll
      for (int i = 0; i < kWaves; i++) {
        const unsigned long long x = s_w[q][i];
        if (i < w) before[q] += x;
        total[q] += x;
      }
      carry[q] += total[q];
    }
    if (t < tiles) {
      ws.b0[at] = before[1] + incl[1] - v[1];
      if (ws.b1) ws.b1[at] = before[2] + incl[2] - v[2];
    }
    __syncthreads();  // the next round overwrites s_w
  }
  if (tid == 0) {
    shard_counts[s] = (int64_t)carry[0];
    shard_bytes[s] = (int64_t)carry[1];
    if (ws.b1) shard_bytes[n_shards + s] = (int64_t)carry[2];
  }
}

__global__ void __launch_bounds__(kBlock) k_fqp_offsets(const FqpRecords a, const FqpPlanSpace ws, int64_t* __restrict__ offsets) {
  __shared__ int s_shard[kFqpPlanTile];
  __shared__ long long s_s0[kFqpPlanTile], s_s1[kFqpPlanTile];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kFqpPlanTile + tid;
  int s = -1;
  int64_t s0 = 0, s1 = 0;
  if (i < a.n) {
    fqp_sizes(a, i, &s0, &s1);
    s = fqp_shard_of(a, i);
  }
  s_shard[tid] = s, s_s0[tid] = s0, s_s1[tid] = s1;
  __syncthreads();
  if (i >= a.n) return;
  const int64_t at = (int64_t)blockIdx.x * a.n_shards + s;
  int64_t o0 = (int64_t)ws.b0[at], o1 = ws.b1 ? (int64_t)ws.b1[at] : 0;
  for (int j = 0; j < tid; j++)
    if (s_shard[j] == s) o0 += s_s0[j], o1 += s_s1[j];
  offsets[i] = o0;
  if (ws.b1) offsets[a.n + i] = o1;
}

// ---- emit ----

// lanes l of `lanes` copy src[0, len) to dst, eight bytes per lane and step
__device__ __forceinline__ void fqp_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, int64_t len, int l, int lanes) {
  for (int64_t c = (int64_t)l * 8; c < len; c += (int64_t)lanes * 8) {
    if (c + 8 <= len) {
      uint64_t word;
      __builtin_memcpy(&word, src + c, 8);
      __builtin_memcpy(dst + c, &word, 8);
    } else {
      for (int64_t b = c; b < len; b++) dst[b] = src[b];
    }
  }
}

__device__ __forceinline__ bool fqp_line_ok(int64_t off, int64_t len, int64_t n_bytes) { return off >= 0 && off + len <= n_bytes; }

struct FqpLines {  // record i's lines
  int64_t id_off, id, seq_off, seq, qual_off, qual;
  int64_t sr_off, sr, sy_off, sy;  // I1's sequence and quality line
  bool ok;
};

__device__ __forceinline__ FqpLines fqp_lines_of(const FqpRecords& a, int64_t i) {
  FqpLines x;
  x.id_off = a.r2_off[3 * i], x.seq_off = a.r2_off[3 * i + 1], x.qual_off = a.r2_off[3 * i + 2];
  x.id = fqp_len(a.r2_len, 3 * i), x.seq = fqp_len(a.r2_len, 3 * i + 1), x.qual = fqp_len(a.r2_len, 3 * i + 2);
  x.ok = fqp_line_ok(x.id_off, x.id, a.r2_bytes) && fqp_line_ok(x.seq_off, x.seq, a.r2_bytes) &&
         fqp_line_ok(x.qual_off, x.qual, a.r2_bytes);
  x.sr_off = x.sr = x.sy_off = x.sy = 0;
  if (a.i1_len) {
    x.sr_off = a.i1_off[3 * i + 1], x.sy_off = a.i1_off[3 * i + 2];
    x.sr = fqp_len(a.i1_len, 3 * i + 1), x.sy = fqp_len(a.i1_len, 3 * i + 2);
    x.ok = x.ok && fqp_line_ok(x.sr_off, x.sr, a.i1_bytes) && fqp_line_ok(x.sy_off, x.sy, a.i1_bytes);
  }
  return x;
}

__global__ void __launch_bounds__(kBlock) k_fqp_emit_bam(const FqpRecords a, const int64_t* __restrict__ offsets,
                                                         const int64_t* __restrict__ shard_base, uint8_t* __restrict__ out,
                                                         int64_t out_bytes, unsigned long long* __restrict__ error) {
  __shared__ uint8_t s_nib[256];  // the 4-bit code of a base
  const int tid = threadIdx.x;
  s_nib[tid] = 15;
  __syncthreads();
  if (tid < 16) {
    const char c = "=ACMGRSVTWYHKDBN"[tid];
    s_nib[(uint8_t)c] = (uint8_t)tid;
    if (c >= 'A' && c <= 'Z') s_nib[(uint8_t)(c + 32)] = (uint8_t)tid;
  }
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kFqpEmitRecords + tid / kFqpEmitLanes;
  const int l = tid % kFqpEmitLanes;
  if (i >= a.n) return;
  const FqpLines x = fqp_lines_of(a, i);
  int64_t size, unused;
  fqp_sizes(a, i, &size, &unused);
  const int64_t pos = shard_base[fqp_shard_of(a, i)] + offsets[i];
  if (!x.ok || x.id > SCT_FQP_MAX_IDENTIFIER || pos < 0 || pos + size > out_bytes || size - 4 > (int64_t)UINT32_MAX) {
    if (l == 0) atomicAdd(error, 1ull);
    return;
  }
  uint8_t* o = out + pos;
  if (l < 9) {
    uint32_t v = 0xffffffffu;  // refID, pos, next_refID, next_pos
    if (l == 0) v = (uint32_t)(size - 4);
    if (l == 3) v = ((uint32_t)SCT_FQP_BAM_BIN << 16) | (uint32_t)(x.id + 1);  // bin, mapq 0, l_read_name
    if (l == 4) v = 4u << 16;                                                 // flag 4, n_cigar_op 0
    if (l == 5) v = (uint32_t)x.seq;
    if (l == 8) v = 0;  // tlen
    __builtin_memcpy(o + 4 * l, &v, 4);
  }
  o += 36;
  fqp_copy(o, a.r2_text + x.id_off, x.id, l, kFqpEmitLanes);
  if (l == kFqpEmitLanes - 1) o[x.id] = 0;
  o += x.id + 1;
  const uint8_t* seq = a.r2_text + x.seq_off;
  for (int64_t c = (int64_t)l * 8; c < x.seq; c += kFqpEmitLanes * 8) {  // eight bases to four bytes
    if (c + 8 <= x.seq) {
      uint64_t word;
      __builtin_memcpy(&word, seq + c, 8);
      uint32_t packed = 0;
#pragma unroll
      for (int b = 0; b < 4; b++)
        packed |= (uint32_t)((s_nib[(uint8_t)(word >> (16 * b))] << 4) | s_nib[(uint8_t)(word >> (16 * b + 8))]) << (8 * b);
      __builtin_memcpy(o + c / 2, &packed, 4);
    } else {
      for (int64_t b = c; b < x.seq; b += 2)
        o[b / 2] = (uint8_t)((s_nib[seq[b]] << 4) | (b + 1 < x.seq ? s_nib[seq[b + 1]] : 0));
    }
  }
  o += (x.seq + 1) / 2;
  const uint8_t* qual = a.r2_text + x.qual_off;
  const int64_t both = min(x.seq, x.qual);
  for (int64_t c = (int64_t)l * 8; c < x.seq; c += kFqpEmitLanes * 8) {
    if (c + 8 <= both) {
      uint64_t word, less = 0;
      __builtin_memcpy(&word, qual + c, 8);
#pragma unroll
      for (int b = 0; b < 8; b++) less |= (uint64_t)(uint8_t)((uint8_t)(word >> (8 * b)) - 33) << (8 * b);
      __builtin_memcpy(o + c, &less, 8);
    } else {
      for (int64_t b = c; b < min(c + 8, x.seq); b++) o[b] = b < both ? (uint8_t)(qual[b] - 33) : (uint8_t)0xff;
    }
  }
  o += x.seq;
  // the tags: two lanes each
  const int tag = l >> 1, half = l & 1;
  const bool has_i1 = a.i1_len != nullptr, has_cb = fqp_has_cb(a, i);
  const int64_t cell = 4 + a.Lc, umi = 4 + a.Lu;
  const int64_t sr_at = 5 + 2 * cell + 2 * umi, sy_at = sr_at + (has_i1 ? 4 + x.sr : 0), cb_at = sy_at + (has_i1 ? 4 + x.sy : 0);
  const char* name = "RG";
  const uint8_t* src = nullptr;
  int64_t at = 0, len = 1;
  bool present = true;
  switch (tag) {
    case 0: break;
    case 1: name = "CR", src = a.cr + i * a.Lc, at = 5, len = a.Lc; break;
    case 2: name = "CY", src = a.cy + i * a.Lc, at = 5 + cell, len = a.Lc; break;
    case 3: name = "UR", src = a.ur + i * a.Lu, at = 5 + 2 * cell, len = a.Lu; break;
    case 4: name = "UY", src = a.uy + i * a.Lu, at = 5 + 2 * cell + umi, len = a.Lu; break;
    case 5: name = "SR", src = a.i1_text + x.sr_off, at = sr_at, len = x.sr, present = has_i1; break;
    case 6: name = "SY", src = a.i1_text + x.sy_off, at = sy_at, len = x.sy, present = has_i1; break;
    default: name = "CB", src = a.cb + i * a.Lc, at = cb_at, len = a.Lc, present = has_cb; break;
  }
  if (!present) return;
  uint8_t* d = o + at;
  if (half == 0) {
    d[0] = (uint8_t)name[0], d[1] = (uint8_t)name[1], d[2] = 'Z';
    if (tag == 0) d[3] = 'A';
  } else {
    d[3 + len] = 0;
  }
  if (tag != 0) fqp_copy(d + 3, src, len, half, 2);
}

__global__ void __launch_bounds__(kBlock) k_fqp_emit_fastq(const FqpRecords a, const int64_t* __restrict__ offsets,
                                                           const int64_t* __restrict__ shard_base, uint8_t* __restrict__ out1,
                                                           int64_t out1_bytes, uint8_t* __restrict__ out2, int64_t out2_bytes,
                                                           unsigned long long* __restrict__ error) {
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kFqpEmitRecords + tid / kFqpEmitLanes;
  const int l = tid % kFqpEmitLanes;
  if (i >= a.n) return;
  const FqpLines x = fqp_lines_of(a, i);
  int64_t size1, size2;
  fqp_sizes(a, i, &size1, &size2);
  const int s = fqp_shard_of(a, i);
  const int64_t pos1 = shard_base[s] + offsets[i], pos2 = shard_base[a.n_shards + s] + offsets[a.n + i];
  if (!x.ok || pos1 < 0 || pos1 + size1 > out1_bytes || pos2 < 0 || pos2 + size2 > out2_bytes) {
    if (l == 0) atomicAdd(error, 1ull);
    return;
  }
  const uint8_t* id = a.r2_text + x.id_off;
  const int last = kFqpEmitLanes - 1;
  {  // @id \n CR UR \n + \n CY UY \n
    uint8_t* o = out1 + pos1;
    const int64_t bc = a.Lc + a.Lu;
    if (l == last) o[0] = '@', o[1 + x.id] = '\n';
    fqp_copy(o + 1, id, x.id, l, kFqpEmitLanes);
    o += x.id + 2;
    fqp_copy(o, a.cr + i * a.Lc, a.Lc, l, kFqpEmitLanes);
    fqp_copy(o + a.Lc, a.ur + i * a.Lu, a.Lu, (l + 8) % kFqpEmitLanes, kFqpEmitLanes);
    if (l == last) o[bc] = '\n', o[bc + 1] = '+', o[bc + 2] = '\n', o[bc + 3 + bc] = '\n';
    o += bc + 3;
    fqp_copy(o, a.cy + i * a.Lc, a.Lc, (l + 4) % kFqpEmitLanes, kFqpEmitLanes);
    fqp_copy(o + a.Lc, a.uy + i * a.Lu, a.Lu, (l + 12) % kFqpEmitLanes, kFqpEmitLanes);
  }
  {  // @id \n seq \n + \n qual \n
    uint8_t* o = out2 + pos2;
    if (l == last) o[0] = '@', o[1 + x.id] = '\n';
    fqp_copy(o + 1, id, x.id, l, kFqpEmitLanes);
    o += x.id + 2;
    fqp_copy(o, a.r2_text + x.seq_off, x.seq, l, kFqpEmitLanes);
    if (l == last) o[x.seq] = '\n', o[x.seq + 1] = '+', o[x.seq + 2] = '\n', o[x.seq + 3 + x.qual] = '\n';
    o += x.seq + 3;
    fqp_copy(o, a.r2_text + x.qual_off, x.qual, l, kFqpEmitLanes);
  }
}

// ---- host ----

bool fqp_misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

int fqp_check_records(const sct_fqp_records_t* r, int32_t format, FqpRecords* a) {
  if (!r) return fail(SCT_FQ_EINVAL, "NULL records");
  if (r->format != SCT_FQP_BAM && r->format != SCT_FQP_FASTQ) return fail(SCT_FQ_EINVAL, "format %d is neither BAM nor FASTQ", r->format);
  if (format >= 0 && r->format != format) return fail(SCT_FQ_EINVAL, "records of format %d given to the call for format %d", r->format, format);
  if (r->n < 0 || r->n > ((int64_t)1 << 38)) return fail(SCT_FQ_EINVAL, "%lld records: outside 0..2^38", (long long)r->n);
  if (r->n_shards < 1 || r->n_shards > kFqpMaxShards) return fail(SCT_FQ_EINVAL, "n_shards %d outside 1..%d", r->n_shards, kFqpMaxShards);
  if (r->cell_length < 1 || r->cell_length > kFqpMaxL) return fail(SCT_FQ_EINVAL, "cell_length %d outside 1..%d", r->cell_length, kFqpMaxL);
  if (r->umi_length < 0 || r->umi_length > 255) return fail(SCT_FQ_EINVAL, "umi_length %d outside 0..255", r->umi_length);
  if (r->r2_bytes < 0 || r->i1_bytes < 0) return fail(SCT_FQ_EINVAL, "negative text size");
  const bool any_i1 = r->i1_text || r->i1_off || r->i1_len;
  if (r->n > 0) {
    if (!r->r2_text || !r->r2_off || !r->r2_len) return fail(SCT_FQ_EINVAL, "NULL R2 text or lines");
    if (any_i1 && (!r->i1_text || !r->i1_off || !r->i1_len)) return fail(SCT_FQ_EINVAL, "I1 text and lines are given together or not at all");
    if (!r->cr || !r->cy || (r->umi_length > 0 && (!r->ur || !r->uy))) return fail(SCT_FQ_EINVAL, "NULL barcode column");
    if ((r->cb == nullptr) != (r->cb_index == nullptr)) return fail(SCT_FQ_EINVAL, "cb and cb_index are given together or not at all");
    if (!r->shard) return fail(SCT_FQ_EINVAL, "NULL shard");
  }
  if (fqp_misaligned(r->r2_off, 7) || fqp_misaligned(r->i1_off, 7)) return fail(SCT_FQ_EINVAL, "line offsets are not 8-byte aligned");
  if (fqp_misaligned(r->r2_len, 3) || fqp_misaligned(r->i1_len, 3) || fqp_misaligned(r->cb_index, 3) || fqp_misaligned(r->shard, 3))
    return fail(SCT_FQ_EINVAL, "line lengths, cb_index or shard are not 4-byte aligned");
  a->n = r->n;
  a->r2_text = r->r2_text, a->r2_bytes = r->r2_bytes, a->r2_off = r->r2_off, a->r2_len = r->r2_len;
  a->i1_text = r->i1_text, a->i1_bytes = r->i1_bytes, a->i1_off = r->i1_off, a->i1_len = r->i1_len;
  a->cr = r->cr, a->cy = r->cy, a->ur = r->ur, a->uy = r->uy, a->cb = r->cb;
  a->cb_index = r->cb_index, a->shard = r->shard;
  a->Lc = r->cell_length, a->Lu = r->umi_length, a->n_shards = r->n_shards, a->format = r->format;
  return SCT_FQ_OK;
}

int64_t fqp_plan_tiles(int64_t n) { return (n + kFqpPlanTile - 1) / kFqpPlanTile; }

size_t fqp_plan_bytes(int64_t n, int32_t n_shards, int32_t format) {
  const size_t cells = (size_t)std::max<int64_t>(fqp_plan_tiles(n), 1) * (size_t)n_shards;
  return cells * (format == SCT_FQP_FASTQ ? 20 : 12);
}

}  // namespace

extern "C" {

int sct_fqp_lines(const uint8_t* text, int64_t n_bytes, int64_t n_records, const void* workspace,
                  size_t workspace_bytes, int64_t* line_off, int32_t* line_len, uint8_t* flags,
                  sct_fq_result_t* result, void* stream) {
  g_err.clear();
  const int rc = check_window(text, n_bytes, workspace, workspace_bytes, result);
  if (rc) return rc;
  if (n_records < 0) return fail(SCT_FQ_EINVAL, "negative n_records");
  if (n_records > n_bytes / 3 + 1) return fail(SCT_FQ_EINVAL, "%lld records cannot be in %lld bytes", (long long)n_records, (long long)n_bytes);
  if (n_records > 0) {
    if (!line_off || fqp_misaligned(line_off, 7)) return fail(SCT_FQ_EINVAL, "line_off is NULL or not 8-byte aligned");
    if (!line_len || fqp_misaligned(line_len, 3)) return fail(SCT_FQ_EINVAL, "line_len is NULL or not 4-byte aligned");
    if (!flags || fqp_misaligned(flags, 3)) return fail(SCT_FQ_EINVAL, "flags is NULL or not 4-byte aligned");
  }
  hipStream_t s = (hipStream_t)stream;
  SCT_LIB_HIP(SCT_FQ_EHIP, hipMemsetAsync(&result->first_flagged, 0xff, sizeof(int64_t), s));
  if (n_records == 0) return SCT_FQ_OK;
  SCT_LIB_HIP(SCT_FQ_EHIP, hipMemsetAsync(flags, 0, (size_t)((n_records + 3) & ~(int64_t)3), s));
  // a line that no '\n' of the window ends (a caller's n_records past the count) reads as empty and is flagged
  SCT_LIB_HIP(SCT_FQ_EHIP, hipMemsetAsync(line_off, 0, (size_t)n_records * 3 * sizeof(int64_t), s));
  SCT_LIB_HIP(SCT_FQ_EHIP, hipMemsetAsync(line_len, 0, (size_t)n_records * 3 * sizeof(int32_t), s));
  const int64_t tiles = tiles_of(n_bytes);
  FqpLinesArgs a{};
  a.text = text, a.n = n_bytes, a.n_records = n_records, a.tiles = tiles;
  a.first = (const uint64_t*)workspace;
  a.cnt = (const uint32_t*)(a.first + (tiles > 0 ? tiles : 1));
  a.off = line_off, a.len = line_len, a.flags = (uint32_t*)flags;
  a.first_flagged = (unsigned long long*)&result->first_flagged;
  if (tiles > 0) {
    hipLaunchKernelGGL(k_fqp_lines, dim3((unsigned)tiles), dim3(kBlock), 0, s, a);
    SCT_LIB_HIP(SCT_FQ_EHIP, hipGetLastError());
  }
  hipLaunchKernelGGL(k_fqp_check, dim3((unsigned)((n_records + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                     (const int32_t*)line_len, n_records, a.flags, a.first_flagged);
  SCT_LIB_HIP(SCT_FQ_EHIP, hipGetLastError());
  return SCT_FQ_OK;
}

int sct_fqp_shard(const uint8_t* raw, const uint8_t* corrected, const int32_t* index, int64_t n, int32_t L,
                  int32_t n_shards, int32_t* shard, int64_t* counts, void* stream) {
  g_err.clear();
  if (L < 1 || L > kFqpMaxL) return fail(SCT_FQ_EINVAL, "L %d outside 1..%d", L, kFqpMaxL);
  if (n_shards < 1 || n_shards > kFqpMaxShards) return fail(SCT_FQ_EINVAL, "n_shards %d outside 1..%d", n_shards, kFqpMaxShards);
  if (n < 0 || n > ((int64_t)1 << 38)) return fail(SCT_FQ_EINVAL, "%lld rows: outside 0..2^38", (long long)n);
  if (n > 0 && !raw) return fail(SCT_FQ_EINVAL, "NULL raw");
  if (fqp_misaligned(raw, 15) || fqp_misaligned(corrected, 15)) return fail(SCT_FQ_EINVAL, "raw or corrected is not 16-byte aligned");
  if ((corrected == nullptr) != (index == nullptr)) return fail(SCT_FQ_EINVAL, "corrected and index are given together or not at all");
  if (fqp_misaligned(index, 3)) return fail(SCT_FQ_EINVAL, "index is not 4-byte aligned");
  if (n > 0 && (!shard || fqp_misaligned(shard, 3))) return fail(SCT_FQ_EINVAL, "shard is NULL or not 4-byte aligned");
  if (!counts || fqp_misaligned(counts, 7)) return fail(SCT_FQ_EINVAL, "counts is NULL or not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  SCT_LIB_HIP(SCT_FQ_EHIP, hipMemsetAsync(counts, 0, 3 * sizeof(int64_t), s));
  if (n == 0) return SCT_FQ_OK;
  hipLaunchKernelGGL(k_fqp_shard, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, raw, corrected, index, n,
                     (int)L, (uint32_t)n_shards, shard, (unsigned long long*)counts);
  SCT_LIB_HIP(SCT_FQ_EHIP, hipGetLastError());
  return SCT_FQ_OK;
}

int sct_fqp_plan_workspace_size(int64_t n, int32_t n_shards, int32_t format, size_t* bytes) {
  g_err.clear();
  if (!bytes) return fail(SCT_FQ_EINVAL, "NULL bytes");
  if (n < 0 || n > ((int64_t)1 << 38)) return fail(SCT_FQ_EINVAL, "%lld records: outside 0..2^38", (long long)n);
  if (n_shards < 1 || n_shards > kFqpMaxShards) return fail(SCT_FQ_EINVAL, "n_shards %d outside 1..%d", n_shards, kFqpMaxShards);
  if (format != SCT_FQP_BAM && format != SCT_FQP_FASTQ) return fail(SCT_FQ_EINVAL, "format %d is neither BAM nor FASTQ", format);
  *bytes = fqp_plan_bytes(n, n_shards, format);
  return SCT_FQ_OK;
}

int sct_fqp_plan(const sct_fqp_records_t* records, void* workspace, size_t workspace_bytes, int64_t* offsets,
                 int64_t* shard_counts, int64_t* shard_bytes, void* stream) {
  g_err.clear();
  FqpRecords a{};
  const int rc = fqp_check_records(records, -1, &a);
  if (rc) return rc;
  const int K = a.format == SCT_FQP_FASTQ ? 2 : 1;
  if (!workspace || fqp_misaligned(workspace, 7)) return fail(SCT_FQ_EINVAL, "workspace is NULL or not 8-byte aligned");
  const size_t need = fqp_plan_bytes(a.n, a.n_shards, a.format);
  if (workspace_bytes < need) return fail(SCT_FQ_ESIZE, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
  if (a.n > 0 && (!offsets || fqp_misaligned(offsets, 7))) return fail(SCT_FQ_EINVAL, "offsets is NULL or not 8-byte aligned");
  if (!shard_counts || !shard_bytes || fqp_misaligned(shard_counts, 7) || fqp_misaligned(shard_bytes, 7))
    return fail(SCT_FQ_EINVAL, "shard_counts or shard_bytes is NULL or not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (a.n == 0) {
    SCT_LIB_HIP(SCT_FQ_EHIP, hipMemsetAsync(shard_counts, 0, (size_t)a.n_shards * sizeof(int64_t), s));
    SCT_LIB_HIP(SCT_FQ_EHIP, hipMemsetAsync(shard_bytes, 0, (size_t)K * a.n_shards * sizeof(int64_t), s));
    return SCT_FQ_OK;
  }
  const int64_t tiles = fqp_plan_tiles(a.n);
  const size_t cells = (size_t)tiles * (size_t)a.n_shards;
  FqpPlanSpace ws{};
  ws.b0 = (unsigned long long*)workspace;
  ws.b1 = K == 2 ? ws.b0 + cells : nullptr;
  ws.cnt = (uint32_t*)(ws.b0 + (size_t)K * cells);
  hipLaunchKernelGGL(k_fqp_hist, dim3((unsigned)tiles), dim3(kBlock), 0, s, a, ws);
  SCT_LIB_HIP(SCT_FQ_EHIP, hipGetLastError());
  hipLaunchKernelGGL(k_fqp_scan, dim3((unsigned)a.n_shards), dim3(kBlock), 0, s, ws, tiles, (int)a.n_shards, shard_counts,
                     shard_bytes);
  SCT_LIB_HIP(SCT_FQ_EHIP, hipGetLastError());
  hipLaunchKernelGGL(k_fqp_offsets, dim3((unsigned)tiles), dim3(kBlock), 0, s, a, ws, offsets);
  SCT_LIB_HIP(SCT_FQ_EHIP, hipGetLastError());
  return SCT_FQ_OK;
}

int sct_fqp_emit_bam(const sct_fqp_records_t* records, const int64_t* offsets, const int64_t* shard_base, uint8_t* out,
                     int64_t out_bytes, int64_t* error, void* stream) {
  g_err.clear();
  FqpRecords a{};
  const int rc = fqp_check_records(records, SCT_FQP_BAM, &a);
  if (rc) return rc;
  if (!error || fqp_misaligned(error, 7)) return fail(SCT_FQ_EINVAL, "error is NULL or not 8-byte aligned");
  if (out_bytes < 0) return fail(SCT_FQ_EINVAL, "negative out_bytes");
  if (a.n > 0 && (!offsets || !shard_base || fqp_misaligned(offsets, 7) || fqp_misaligned(shard_base, 7)))
    return fail(SCT_FQ_EINVAL, "offsets or shard_base is NULL or not 8-byte aligned");
  if (a.n > 0 && out_bytes > 0 && !out) return fail(SCT_FQ_EINVAL, "NULL out");
  hipStream_t s = (hipStream_t)stream;
  SCT_LIB_HIP(SCT_FQ_EHIP, hipMemsetAsync(error, 0, sizeof(int64_t), s));
  if (a.n == 0) return SCT_FQ_OK;
  hipLaunchKernelGGL(k_fqp_emit_bam, dim3((unsigned)((a.n + kFqpEmitRecords - 1) / kFqpEmitRecords)), dim3(kBlock), 0, s, a,
                     offsets, shard_base, out, out_bytes, (unsigned long long*)error);
  SCT_LIB_HIP(SCT_FQ_EHIP, hipGetLastError());
  return SCT_FQ_OK;
}

int sct_fqp_emit_fastq(const sct_fqp_records_t* records, const int64_t* offsets, const int64_t* shard_base,
                       uint8_t* out1, int64_t out1_bytes, uint8_t* out2, int64_t out2_bytes, int64_t* error,
                       void* stream) {
  g_err.clear();
  FqpRecords a{};
  const int rc = fqp_check_records(records, SCT_FQP_FASTQ, &a);
  if (rc) return rc;
  if (!error || fqp_misaligned(error, 7)) return fail(SCT_FQ_EINVAL, "error is NULL or not 8-byte aligned");
  if (out1_bytes < 0 || out2_bytes < 0) return fail(SCT_FQ_EINVAL, "negative out_bytes");
  if (a.n > 0 && (!offsets || !shard_base || fqp_misaligned(offsets, 7) || fqp_misaligned(shard_base, 7)))
    return fail(SCT_FQ_EINVAL, "offsets or shard_base is NULL or not 8-byte aligned");
  if (a.n > 0 && ((out1_bytes > 0 && !out1) || (out2_bytes > 0 && !out2))) return fail(SCT_FQ_EINVAL, "NULL out");
  hipStream_t s = (hipStream_t)stream;
  SCT_LIB_HIP(SCT_FQ_EHIP, hipMemsetAsync(error, 0, sizeof(int64_t), s));
  if (a.n == 0) return SCT_FQ_OK;
  hipLaunchKernelGGL(k_fqp_emit_fastq, dim3((unsigned)((a.n + kFqpEmitRecords - 1) / kFqpEmitRecords)), dim3(kBlock), 0, s, a,
                     offsets, shard_base, out1, out1_bytes, out2, out2_bytes, (unsigned long long*)error);
  SCT_LIB_HIP(SCT_FQ_EHIP, hipGetLastError());
  return SCT_FQ_OK;
}

}  // extern "C"
