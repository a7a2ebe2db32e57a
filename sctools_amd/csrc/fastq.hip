// fastq.hip -- libsct_fastq.so: FASTQ text to fixed-width barcode columns
// (include/sct_fastq.h), gfx950, wave64.
//
// The text is cut into 16 KiB tiles, one 256-thread block each; a thread reads four 16-byte
// groups, group j of thread t at byte (j * 256 + t) * 16 of the tile, so every load instruction
// of a wave covers 1 KiB of consecutive text.  A '\n' is found four at a time with the
// zero-byte trick on the 32-bit words of a group.
//
//   pass 1  k_count    '\n' per tile
//           k_scan     one 1024-thread block: exclusive scan of the tile counts (the number of
//                      every tile's first line), the line and record totals, and the byte after
//                      the '\n' that ends the last complete record
//   pass 2  k_extract  re-reads the tile, ranks its '\n's (wave scan per group, 16 segment
//                      totals through LDS), lists their offsets in LDS by rank, and lets four
//                      lanes act on the line that FOLLOWS a '\n': after line 4r the sequence,
//                      after 4r+2 the quality, after 4r+3 the next record's name.
//
// There is no per-line offset array in device memory: the text is read twice and the only
// intermediate is 12 bytes per tile.  csrc/scan.h is not used: its launches go through the
// engine's profiler scopes and error state (util.h), which this library does not link, and the
// scan here is over at most n_bytes / 16384 counts, which one block does in one kernel together
// with the totals.
//
// Nothing here writes memory with anything but plain vector stores and vector atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sct_fastq.h"
#include "liberr.h"  // g_err, fail(), SCT_LIB_HIP

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kGroups = 4;  // 16-byte groups per thread
constexpr int64_t kTile = SCT_FQ_TILE_BYTES;
static_assert(kTile == (int64_t)kBlock * kGroups * 16, "a tile is what one block reads");
constexpr int kScanBlock = 1024;
static_assert(kTile == (int64_t)kScanBlock * 16, "k_scan reads one tile with one group per thread");

int64_t tiles_of(int64_t n_bytes) { return (n_bytes + kTile - 1) / kTile; }

// the workspace: first[tiles] (uint64), then cnt[tiles] (uint32)
size_t workspace_bytes_of(int64_t tiles) { return (size_t)(tiles > 0 ? tiles : 1) * 12 + 4; }

// 0x80 in every byte of `w` that is '\n', exact (no carry between bytes)
__device__ __forceinline__ uint32_t newline_mask(uint32_t w) {
  const uint32_t v = w ^ 0x0A0A0A0Au;
  return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v | 0x7F7F7F7Fu);
}

// the 16 bytes at `off` (a multiple of 16); bytes at and past `n` read as zero
__device__ __forceinline__ uint4 load_group(const uint8_t* __restrict__ text, int64_t off, int64_t n) {
  if (off + 16 <= n) return *reinterpret_cast<const uint4*>(text + off);
  uint32_t w[4] = {0, 0, 0, 0};
  for (int b = 0; b < 16; b++)
    if (off + b < n) w[b >> 2] |= (uint32_t)text[off + b] << (8 * (b & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ uint4 group_masks(uint4 v) {
  return make_uint4(newline_mask(v.x), newline_mask(v.y), newline_mask(v.z), newline_mask(v.w));
}

__device__ __forceinline__ uint32_t group_count(uint4 m) { return __popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w); }

template <typename T>
__device__ __forceinline__ T wave_inclusive(T v) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const T t = __shfl_up(v, o, kWave);
    if (lane >= o) v += t;
  }
  return v;
}

__global__ void __launch_bounds__(kBlock) k_count(const uint8_t* __restrict__ text, int64_t n,
                                                  uint32_t* __restrict__ cnt) {
  const int64_t base = (int64_t)blockIdx.x * kTile;
  uint4 v[kGroups];
#pragma unroll
  for (int j = 0; j < kGroups; j++) v[j] = load_group(text, base + ((int64_t)j * kBlock + threadIdx.x) * 16, n);
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < kGroups; j++) c += group_count(group_masks(v[j]));
  __shared__ uint32_t s_w[kBlock / kWave];
  c = wave_inclusive(c);
  if ((threadIdx.x & (kWave - 1)) == kWave - 1) s_w[threadIdx.x / kWave] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < kBlock / kWave; w++) t += s_w[w];
    cnt[blockIdx.x] = t;
  }
}

// block-wide exclusive scan over kScanBlock threads; *total is the block's sum
__device__ __forceinline__ uint64_t scan_block(uint64_t v, uint64_t* total, uint64_t* s_w) {
  const int w = threadIdx.x / kWave;
  const uint64_t incl = wave_inclusive(v);
  __syncthreads();  // s_w may still be read from the previous use
  if ((threadIdx.x & (kWave - 1)) == kWave - 1) s_w[w] = incl;
  __syncthreads();
  uint64_t before = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < kScanBlock / kWave; i++) {
    const uint64_t x = s_w[i];
    if (i < w) before += x;
    tot += x;
  }
  *total = tot;
  return before + incl - v;
}

__global__ void __launch_bounds__(kScanBlock) k_scan(const uint8_t* __restrict__ text, int64_t n, int is_last,
                                                     int64_t tiles, const uint32_t* __restrict__ cnt,
                                                     uint64_t* __restrict__ first, sct_fq_result_t* __restrict__ result) {
  __shared__ uint64_t s_w[kScanBlock / kWave];
  __shared__ int64_t s_tile;
  __shared__ int64_t s_consumed;
  const int tid = threadIdx.x;
  uint64_t carry = 0;
  for (int64_t base = 0; base < tiles; base += kScanBlock) {
    const int64_t t = base + tid;
    const uint64_t v = t < tiles ? cnt[t] : 0;
    uint64_t tot;
    const uint64_t ex = scan_block(v, &tot, s_w);
    if (t < tiles) first[t] = carry + ex;
    carry += tot;
  }
  const uint64_t newlines = carry;
  const uint64_t lines = newlines + ((is_last && n > 0 && text[n - 1] != '\n') ? 1 : 0);
  const uint64_t records = lines >> 2;
  if (tid == 0) s_tile = -1, s_consumed = 0;
  __syncthreads();  // also orders the writes of first[] before the reads below
  if (records > 0) {
    const uint64_t k = 4 * records - 1;  // the line that ends the last complete record
    if (k >= newlines) {                 // it is the unterminated last line
      if (tid == 0) s_consumed = n;
    } else {
      for (int64_t t = tid; t < tiles; t += kScanBlock) {
        const uint64_t f = first[t];
        if (f <= k && k < f + cnt[t]) s_tile = t;  // exactly one tile holds '\n' number k
      }
      __syncthreads();
      const int64_t tile = s_tile;
      if (tile >= 0) {  // (always)
        const uint64_t rank = k - first[tile];
        const int64_t off = tile * kTile + (int64_t)tid * 16;
        const uint4 m = group_masks(load_group(text, off, n));
        const uint32_t c = group_count(m);
        uint64_t tot;
        const uint64_t ex = scan_block(c, &tot, s_w);
        if (ex <= rank && rank < ex + c) {
          uint32_t skip = (uint32_t)(rank - ex);
          const uint32_t words[4] = {m.x, m.y, m.z, m.w};
          for (int q = 0; q < 4; q++) {
            uint32_t bits = words[q];
            while (bits) {
              const int b = (__ffs((int)bits) - 1) >> 3;
              bits &= bits - 1;
              if (skip-- == 0) s_consumed = off + 4 * q + b + 1;
            }
          }
        }
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    result->n_records = (int64_t)records;
    result->consumed = s_consumed;
    result->n_lines = (int64_t)lines;
    result->first_flagged = -1;
  }
}

struct ExtractArgs {
  const uint8_t* text;
  int64_t n;
  int64_t n_records;
  const uint64_t* first;
  uint32_t* flags;                    // one byte per record, addressed as words for the atomics
  unsigned long long* first_flagged;  // starts as ~0 (-1): an unsigned minimum
  int32_t n_spans, max_end;
  int32_t start[SCT_FQ_MAX_SPANS], end[SCT_FQ_MAX_SPANS];
  uint8_t* seq[SCT_FQ_MAX_SPANS];
  uint8_t* qual[SCT_FQ_MAX_SPANS];
};

__device__ __forceinline__ void raise_flag(const ExtractArgs& a, int64_t r, uint32_t bit) {
  atomicOr(a.flags + (r >> 2), bit << (8 * (int)(r & 3)));
  atomicMin(a.first_flagged, (unsigned long long)r);
}

constexpr int kTaskLanes = 4;                         // lanes that share one line
constexpr int kTaskGroups = kBlock / kTaskLanes;      // lines in flight per block
constexpr int kTaskBytes = 8;                         // consecutive bytes per lane and step: 32 bytes of a line per step
constexpr int kRound = 4096;                          // '\n' offsets held in LDS at a time

// One block per tile.  The '\n's of the tile are ranked as in the header comment and their offsets
// written to LDS by rank; then four lanes share one '\n' and the line that follows it (64 lines in
// flight per block): each lane loads eight consecutive bytes of the line (32 bytes of the line per
// step, one trip to memory), the four agree on where the line ends, and each stores its bytes to
// the columns, as one 8-byte store where they fall into one span.
// (The first version let the lane that owns a '\n' copy its line byte by byte: ~5 lanes of a wave
// active through ~400 dependent loads per tile, 49 ms for 2.2 GB of 10x text.)
__global__ void __launch_bounds__(kBlock) k_extract(const ExtractArgs a) {
  const int64_t base = (int64_t)blockIdx.x * kTile;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
  if (blockIdx.x == 0 && tid == 0 && a.n_records > 0 && a.text[0] != '@') raise_flag(a, 0, SCT_FQ_BAD_NAME);
  uint4 m[kGroups];
#pragma unroll
  for (int j = 0; j < kGroups; j++)
    m[j] = group_masks(load_group(a.text, base + ((int64_t)j * kBlock + tid) * 16, a.n));
  // rank of this thread's first '\n' of group j within the tile: the segments (j, wave) are in text order
  __shared__ uint32_t s_seg[kGroups * (kBlock / kWave)];
  __shared__ uint16_t s_off[kRound];
  uint32_t rank0[kGroups];
#pragma unroll
  for (int j = 0; j < kGroups; j++) {
    const uint32_t c = group_count(m[j]);
    const uint32_t incl = wave_inclusive(c);
    rank0[j] = incl - c;
    if (lane == kWave - 1) s_seg[j * (kBlock / kWave) + w] = incl;
  }
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
  const uint64_t first = a.first[blockIdx.x];
  const int g = tid / kTaskLanes, l = tid % kTaskLanes;
  for (uint32_t round = 0; round < total; round += kRound) {  // (one round unless the tile is mostly blank lines)
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
    for (uint32_t k = g; k < here; k += kTaskGroups) {
      const int64_t p = base + s_off[k];  // a '\n'; it ends line `line` of the window
      const uint64_t line = first + round + k;
      const int64_t r = (int64_t)(line >> 2);
      const int kind = (int)(line & 3);
      if (kind == 3) {  // the next record's name follows
        if (l == 0 && r + 1 < a.n_records && (p + 1 >= a.n || a.text[p + 1] != '@')) raise_flag(a, r + 1, SCT_FQ_BAD_NAME);
        continue;
      }
      if (kind == 1 || r >= a.n_records) continue;
      // record r's sequence (kind 0) or quality (kind 2) line starts at p + 1; all the line's lanes are here
      int32_t line_end = INT32_MAX;  // the line's length where it is shorter than max_end
      for (int32_t c = 0; c < a.max_end; c += kTaskLanes * kTaskBytes) {
        const int32_t j0 = c + l * kTaskBytes;  // this lane's bytes of the line: [j0, j0 + 8)
        uint64_t word = 0x0A0A0A0A0A0A0A0Aull;
        if (j0 < a.max_end) {
          const int64_t at = p + 1 + j0;
          if (at + kTaskBytes <= a.n) {
            __builtin_memcpy(&word, a.text + at, kTaskBytes);  // (any alignment: one load where the target allows it)
          } else {
#pragma unroll
            for (int i = 0; i < kTaskBytes; i++)
              if (at + i < a.n) word = (word & ~(0xffull << (8 * i))) | ((uint64_t)a.text[at + i] << (8 * i));
          }
        }
        const uint64_t nl = (uint64_t)newline_mask((uint32_t)word) | ((uint64_t)newline_mask((uint32_t)(word >> 32)) << 32);
        int32_t mine = nl ? j0 + ((__ffsll((long long)nl) - 1) >> 3) : INT32_MAX;
        if (mine >= a.max_end) mine = INT32_MAX;
#pragma unroll
        for (int o = kTaskLanes / 2; o > 0; o >>= 1) mine = min(mine, __shfl_xor(mine, o, kTaskLanes));
        line_end = min(line_end, mine);
#pragma unroll
        for (int i = 0; i < kTaskBytes; i++)
          if (j0 + i >= line_end) word &= ~(0xffull << (8 * i));  // zero bytes from the line's end on
#pragma unroll
        for (int s = 0; s < SCT_FQ_MAX_SPANS; s++) {
          if (s >= a.n_spans) continue;
          const int32_t lo = max(j0, a.start[s]), hi = min(j0 + kTaskBytes, a.end[s]);
          if (lo >= hi) continue;
          uint8_t* dst = (kind == 0 ? a.seq[s] : a.qual[s]) + r * (int64_t)(a.end[s] - a.start[s]) + (lo - a.start[s]);
          if (hi - lo == kTaskBytes) {
            __builtin_memcpy(dst, &word, kTaskBytes);
          } else {
            for (int32_t j = lo; j < hi; j++) dst[j - lo] = (uint8_t)(word >> (8 * (j - j0)));
          }
        }
      }
      if (l == 0 && line_end != INT32_MAX) raise_flag(a, r, kind == 0 ? SCT_FQ_SHORT_SEQUENCE : SCT_FQ_SHORT_QUALITY);
    }
    __syncthreads();  // the next round overwrites s_off
  }
}

int check_window(const uint8_t* text, int64_t n_bytes, const void* workspace, size_t workspace_bytes,
                 const sct_fq_result_t* result) {
  if (n_bytes < 0) return fail(SCT_FQ_EINVAL, "negative n_bytes");
  if (n_bytes > 0 && !text) return fail(SCT_FQ_EINVAL, "NULL text");
  if ((uintptr_t)text & 15) return fail(SCT_FQ_EINVAL, "text is not 16-byte aligned");
  if (!workspace || ((uintptr_t)workspace & 7)) return fail(SCT_FQ_EINVAL, "workspace is NULL or not 8-byte aligned");
  if (!result || ((uintptr_t)result & 7)) return fail(SCT_FQ_EINVAL, "result is NULL or not 8-byte aligned");
  if (tiles_of(n_bytes) > 0x7fffffff) return fail(SCT_FQ_EINVAL, "window of %lld bytes has too many tiles", (long long)n_bytes);
  const size_t need = workspace_bytes_of(tiles_of(n_bytes));
  if (workspace_bytes < need)
    return fail(SCT_FQ_ESIZE, "workspace of %zu bytes, %zu needed for %lld text bytes", workspace_bytes, need,
                (long long)n_bytes);
  return SCT_FQ_OK;
}

}  // namespace

extern "C" {

const char* sct_fq_last_error(void) { return g_err.c_str(); }

int sct_fq_workspace_size(int64_t n_bytes, size_t* bytes) {
  g_err.clear();
  if (!bytes) return fail(SCT_FQ_EINVAL, "NULL bytes");
  if (n_bytes < 0) return fail(SCT_FQ_EINVAL, "negative n_bytes");
  *bytes = workspace_bytes_of(tiles_of(n_bytes));
  return SCT_FQ_OK;
}

int sct_fq_count(const uint8_t* text, int64_t n_bytes, int32_t is_last, void* workspace, size_t workspace_bytes,
                 sct_fq_result_t* result, void* stream) {
  g_err.clear();
  const int rc = check_window(text, n_bytes, workspace, workspace_bytes, result);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t tiles = tiles_of(n_bytes);
  uint64_t* first = (uint64_t*)workspace;
  uint32_t* cnt = (uint32_t*)(first + (tiles > 0 ? tiles : 1));
  if (tiles > 0) {
    hipLaunchKernelGGL(k_count, dim3((unsigned)tiles), dim3(kBlock), 0, s, text, n_bytes, cnt);
    SCT_LIB_HIP(SCT_FQ_EHIP, hipGetLastError());
  }
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanBlock), 0, s, text, n_bytes, is_last ? 1 : 0, tiles,
                     (const uint32_t*)cnt, first, result);
  SCT_LIB_HIP(SCT_FQ_EHIP, hipGetLastError());
  return SCT_FQ_OK;
}

int sct_fq_extract(const uint8_t* text, int64_t n_bytes, int64_t n_records, const void* workspace,
                   size_t workspace_bytes, const sct_fq_span_t* spans, int32_t n_spans, uint8_t* const* seq_cols,
                   uint8_t* const* qual_cols, uint8_t* flags, sct_fq_result_t* result, void* stream) {
  g_err.clear();
  const int rc = check_window(text, n_bytes, workspace, workspace_bytes, result);
  if (rc) return rc;
  if (n_records < 0) return fail(SCT_FQ_EINVAL, "negative n_records");
  if (n_spans < 1 || n_spans > SCT_FQ_MAX_SPANS) return fail(SCT_FQ_EINVAL, "n_spans %d outside 1..%d", n_spans, SCT_FQ_MAX_SPANS);
  if (!spans || !seq_cols || !qual_cols) return fail(SCT_FQ_EINVAL, "NULL spans or column list");
  // every complete record has three '\n' before its quality line ends: more records than that cannot be in the text
  if (n_records > n_bytes / 3 + 1) return fail(SCT_FQ_EINVAL, "%lld records cannot be in %lld bytes", (long long)n_records, (long long)n_bytes);
  ExtractArgs a{};
  a.text = text;
  a.n = n_bytes;
  a.n_records = n_records;
  a.first = (const uint64_t*)workspace;
  a.flags = (uint32_t*)flags;
  a.first_flagged = (unsigned long long*)&result->first_flagged;
  a.n_spans = n_spans;
  for (int s = 0; s < n_spans; s++) {
    if (spans[s].start < 0 || spans[s].end <= spans[s].start)
      return fail(SCT_FQ_EINVAL, "span %d [%d, %d) is empty or negative", s, spans[s].start, spans[s].end);
    if (n_records > 0 && (!seq_cols[s] || !qual_cols[s])) return fail(SCT_FQ_EINVAL, "NULL column of span %d", s);
    a.start[s] = spans[s].start;
    a.end[s] = spans[s].end;
    a.seq[s] = seq_cols[s];
    a.qual[s] = qual_cols[s];
    if (spans[s].end > a.max_end) a.max_end = spans[s].end;
  }
  if (n_records > 0 && (!flags || ((uintptr_t)flags & 3))) return fail(SCT_FQ_EINVAL, "flags is NULL or not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  SCT_LIB_HIP(SCT_FQ_EHIP, hipMemsetAsync(&result->first_flagged, 0xff, sizeof(int64_t), s));
  if (n_records == 0) return SCT_FQ_OK;
  SCT_LIB_HIP(SCT_FQ_EHIP, hipMemsetAsync(flags, 0, (size_t)((n_records + 3) & ~(int64_t)3), s));
  if (n_bytes == 0) return SCT_FQ_OK;  // no tile, nothing to fill
  hipLaunchKernelGGL(k_extract, dim3((unsigned)tiles_of(n_bytes)), dim3(kBlock), 0, s, a);
  SCT_LIB_HIP(SCT_FQ_EHIP, hipGetLastError());
  return SCT_FQ_OK;
}

}  // extern "C"

#include "fqmetrics.h"  // the sct_fqm_* calls (include/sct_fastq_metrics.h)
#include "fqprocess.h"  // the sct_fqp_* calls (include/sct_fastq_process.h)
#include "fqinflate.h"  // sct_fq_bgzf_scan, sct_fq_inflate (include/sct_fastq_inflate.h)
