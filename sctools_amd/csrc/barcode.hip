// barcode.hip -- libsct_barcode.so: whitelist barcode correction and all-pairs Hamming
// statistics (include/sct_barcode.h), gfx950, wave64.
//
// The correction table is an open-addressing hash table in device memory: 16-byte slots
// {code, raw, fin}, power-of-two slot count at load factor <= 0.5, linear probing, so one probe
// is one 16-byte load.  `raw` is the largest file index of the slot's code; `fin` the largest
// file index among the code and its 3*L whitelist neighbours, i.e. the answer for a query that
// is on the whitelist.  A copy of the codes in file order follows the slots (index -> barcode),
// then a presence filter of one bit per hashed code that keeps most neighbour candidates of a
// query off the list away from the slot array (DESIGN.md section 13 has the counters).
//
// Nothing here writes memory with anything but plain vector stores and vector atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sct_barcode.h"
#include "liberr.h"  // g_err, fail(), SCT_LIB_HIP

namespace {

constexpr uint64_t kEmpty = ~0ull;
constexpr int kBlock = 256;
constexpr int kWave = 64;

struct alignas(16) Slot {
  uint64_t code;
  int32_t raw;
  int32_t fin;
};
static_assert(sizeof(Slot) == 16, "one probe is one 16-byte load");

// slots of an n-entry whitelist: the power of two >= 2n (load factor <= 0.5), at least 64
uint64_t slots_for(int64_t n) {
  uint64_t s = 64;
  while (s < 2ull * (uint64_t)n) s <<= 1;
  return s;
}

// bits of the presence filter of an n-entry whitelist: the power of two >= 16n, at least 2^16
uint64_t filter_bits_for(int64_t n) {
  uint64_t b = 1ull << 16;
  while (b < 16ull * (uint64_t)n) b <<= 1;
  return b;
}

__device__ __forceinline__ uint64_t mix(uint64_t x) {  // splitmix64 finalizer
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

__device__ __forceinline__ Slot load_slot(const Slot* t, uint64_t i) {
  const uint4 v = *reinterpret_cast<const uint4*>(t + i);
  Slot s;
  s.code = (uint64_t)v.x | ((uint64_t)v.y << 32);
  s.raw = (int32_t)v.z;
  s.fin = (int32_t)v.w;
  return s;
}

// the slot of `code`: (raw, fin), or (-1, -1) when the code is not in the table.  The table is
// at most half full, so the scan ends at an empty slot; the bound only keeps a buffer that no
// build filled from spinning a wave forever.
__device__ __forceinline__ int2 probe(const Slot* t, uint64_t mask, uint64_t code) {
  uint64_t i = mix(code) & mask;
  for (uint64_t k = 0; k <= mask; k++) {
    const Slot s = load_slot(t, i);
    if (s.code == code) return make_int2(s.raw, s.fin);
    if (s.code == kEmpty) break;
    i = (i + 1) & mask;
  }
  return make_int2(-1, -1);
}

// The presence filter: one bit per hashed code (the hash's top bits; the slot index takes its low
// bits), set for every whitelist code.  It has no false negatives, so a clear bit answers "not on
// the whitelist" without touching the table; it is sized to stay in an XCD's L2 where the slot
// array cannot (2 MiB against 32 MiB at 737,280 barcodes).
struct Filter {
  const uint32_t* words;
  int shift;  // 64 - log2(bits)
};

__device__ __forceinline__ bool maybe_present(const Filter& f, uint64_t code) {
  const uint64_t bit = mix(code) >> f.shift;
  return (f.words[bit >> 5] >> (bit & 31)) & 1;
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, kWave));
  return v;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, kWave);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, kWave);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// The whole wave searches the neighbours of one code `q` (wave-uniform): the largest raw index
// among the candidates present, or -1.  n_pos < 0: the 3*L single substitutions of q, candidate
// c = (position c / 3, xor (c % 3) + 1).  n_pos >= 0: q holds 0 at position n_pos (an 'N' in the
// query) and the candidates are the 4 bases there.  ceil(candidates / 64) rounds of one probe
// per lane, then a max over the wave.  A candidate goes to the table only if the filter has its bit.
__device__ __forceinline__ int wave_neighbour_max(const Slot* t, uint64_t mask, const Filter& f, uint64_t q, int L,
                                                  int n_pos, int lane) {
  int best = -1;
  if (n_pos < 0) {
    for (int c = lane; c < 3 * L; c += kWave) {
      const int pos = c / 3, k = c % 3 + 1;
      const uint64_t cand = q ^ ((uint64_t)k << (2 * (L - 1 - pos)));
      if (maybe_present(f, cand)) best = max(best, probe(t, mask, cand).x);
    }
  } else if (lane < 4) {
    const uint64_t cand = q | ((uint64_t)lane << (2 * (L - 1 - n_pos)));
    if (maybe_present(f, cand)) best = probe(t, mask, cand).x;
  }
  return wave_max(best);
}

// ---------------- table build ----------------
__global__ void __launch_bounds__(kBlock) bc_fill_empty(uint4* t, uint64_t n_slots) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n_slots) t[i] = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);  // kEmpty, -1, -1
}

// pass 1: every entry claims the slot of its code; the slot keeps the largest file index
__global__ void __launch_bounds__(kBlock) bc_insert(const uint64_t* __restrict__ codes, int64_t n, uint64_t code_mask,
                                                    Slot* t, uint64_t mask, uint64_t* codes_copy, uint32_t* filter,
                                                    int filter_shift) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t code = codes[i] & code_mask;
  codes_copy[i] = code;
  const uint64_t bit = mix(code) >> filter_shift;
  atomicOr(&filter[bit >> 5], 1u << (bit & 31));
  uint64_t s = mix(code) & mask;
  for (uint64_t k = 0; k <= mask; k++) {  // (ends at the first free slot: the table is at most half full)
    const unsigned long long prev =
        atomicCAS(reinterpret_cast<unsigned long long*>(&t[s].code), (unsigned long long)kEmpty, (unsigned long long)code);
    if (prev == kEmpty || prev == code) {
      atomicMax(&t[s].raw, (int32_t)i);
      return;
    }
    s = (s + 1) & mask;
  }
}

// pass 2: every occupied slot's final index = max(raw of itself and of every neighbour present).
// One slot per lane; the wave then searches the neighbours of each occupied lane's code together.
// (fin is written, raw only read: a separate launch after pass 1, so every raw is complete.)
__global__ void __launch_bounds__(kBlock) bc_finalize(Slot* t, uint64_t n_slots, Filter f, int L) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;  // n_slots is a multiple of 64: whole waves
  const int lane = threadIdx.x & (kWave - 1);
  const uint64_t mask = n_slots - 1;
  Slot s;
  s.code = kEmpty, s.raw = -1, s.fin = -1;
  if (i < n_slots) s = load_slot(t, i);
  int fin = s.raw;
  uint64_t todo = __ballot(s.code != kEmpty);
  while (todo) {
    const int src = __ffsll((unsigned long long)todo) - 1;
    todo &= todo - 1;
    const uint64_t q = shfl64(s.code, src);
    const int r = wave_neighbour_max(t, mask, f, q, L, -1, lane);
    if (lane == src) fin = max(fin, r);
  }
  if (i < n_slots && s.code != kEmpty) t[i].fin = fin;
}

// ---------------- correction ----------------
// One query per lane: load, encode, count the bytes outside ACGT, exact probe.  The lanes that
// need a neighbour search are then taken one by one from a ballot and searched by the whole wave.
template <bool kL16>
__global__ void __launch_bounds__(kBlock) bc_correct(const Slot* __restrict__ t, uint64_t mask, Filter f,
                                                     const uint64_t* __restrict__ wl_codes,
                                                     const uint8_t* __restrict__ raw, int64_t n, int L,
                                                     int32_t* __restrict__ out_index, uint8_t* __restrict__ out_corrected) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  const bool live = i < n;
  uint64_t code = 0;
  int n_other = 0, n_pos = -1;  // bytes outside ACGT; position of the last 'N' among them
  bool only_n = true;
  uint4 v = make_uint4(0, 0, 0, 0);
  auto take = [&](uint32_t b, int j) {
    const bool acgt = b == 'A' || b == 'C' || b == 'G' || b == 'T';
    code = (code << 2) | (acgt ? ((b >> 1) & 3) : 0);  // A=0 C=1 T=2 G=3
    if (!acgt) {
      n_other++;
      only_n = only_n && b == 'N';
      n_pos = j;
    }
  };
  if (live) {
    if (kL16) {
      v = reinterpret_cast<const uint4*>(raw)[i];  // one dwordx4 load per query
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 16; j++) take((w[j >> 2] >> (8 * (j & 3))) & 0xff, j);
    } else {
      const uint8_t* p = raw + i * (int64_t)L;
      for (int j = 0; j < L; j++) take(p[j], j);
    }
  }
  int idx = -1;
  int mode = 0;  // 0 none, 1 all 3L neighbours, 2 the 4 bases at n_pos
  bool self = false;  // the query is the corrected barcode
  if (live && n_other == 0) {
    const int2 r = probe(t, mask, code);
    if (r.x >= 0) {
      idx = r.y;
      self = r.y == r.x;
    } else {
      mode = 1;
    }
  } else if (live && n_other == 1 && only_n) {
    mode = 2;
  }
  uint64_t todo = __ballot(mode != 0);
  while (todo) {
    const int src = __ffsll((unsigned long long)todo) - 1;
    todo &= todo - 1;
    const uint64_t q = shfl64(code, src);
    const int m = __shfl(mode, src, kWave);
    const int np = __shfl(n_pos, src, kWave);
    const int r = wave_neighbour_max(t, mask, f, q, L, m == 2 ? np : -1, lane);
    if (lane == src) idx = r;
  }
  if (!live) return;
  out_index[i] = idx;
  if (!out_corrected) return;
  if (idx >= 0 && !self) {  // the corrected barcode's bases, decoded from the whitelist copy
    const uint64_t c = wl_codes[idx];
    if (kL16) {
      uint32_t w[4];
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const uint32_t b = (0x47544341u >> (8 * ((c >> (2 * (15 - j))) & 3))) & 0xff;  // "ACTG"
        w[j >> 2] = (j & 3) ? (w[j >> 2] | (b << (8 * (j & 3)))) : b;
      }
      v = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
      uint8_t* o = out_corrected + i * (int64_t)L;
      for (int j = 0; j < L; j++) o[j] = (uint8_t)((0x47544341u >> (8 * ((c >> (2 * (L - 1 - j))) & 3))) & 0xff);
      return;
    }
  }
  if (kL16) {
    reinterpret_cast<uint4*>(out_corrected)[i] = v;
  } else {  // the raw bytes passed through
    const uint8_t* p = raw + i * (int64_t)L;
    uint8_t* o = out_corrected + i * (int64_t)L;
    for (int j = 0; j < L; j++) o[j] = p[j];
  }
}

// ---------------- all-pairs Hamming histogram ----------------
// Block (bx, by), bx >= by, counts the pairs (row in tile by, column in tile bx): the column tile
// sits in LDS and is read as a broadcast, each thread keeps kRows row codes in registers.  Every
// thread counts into its own LDS bins (bin-major, so the 64 lanes of a wave touch 64 different
// banks whatever distances they hold); bin kBins collects the pairs that do not count (i >= j on
// the diagonal tile, the padding past n).  A thread adds at most kRows * kTile to a bin: 32 bits
// are enough there; the block's sums leave with one 64-bit atomic per bin.
constexpr int kTile = 1024;
constexpr int kRows = kTile / kBlock;
constexpr int kBins = SCT_BC_HIST_BINS;

__global__ void __launch_bounds__(kBlock) bc_pair_hist(const uint64_t* __restrict__ codes, int64_t n,
                                                       unsigned long long* __restrict__ hist) {
  const int bx = blockIdx.x, by = blockIdx.y;
  if (bx < by) return;
  __shared__ uint64_t cols[kTile];
  __shared__ uint32_t bins[(kBins + 1) * kBlock];
  const int tid = threadIdx.x;
  const int64_t col0 = (int64_t)bx * kTile, row0 = (int64_t)by * kTile;
  for (int k = tid; k < kTile; k += kBlock) cols[k] = col0 + k < n ? codes[col0 + k] : 0;
  for (int k = tid; k < (kBins + 1) * kBlock; k += kBlock) bins[k] = 0;
  uint64_t a[kRows];
  int64_t ai[kRows];
#pragma unroll
  for (int r = 0; r < kRows; r++) {
    ai[r] = row0 + r * kBlock + tid;
    a[r] = ai[r] < n ? codes[ai[r]] : 0;
    if (ai[r] >= n) ai[r] = INT64_MAX;  // never below a column index: counts nowhere
  }
  __syncthreads();
  const int n_cols = (int)min((int64_t)kTile, n - col0);
  uint32_t* mine = bins + tid;
  for (int j = 0; j < n_cols; j++) {
    const uint64_t b = cols[j];
    const int64_t bj = col0 + j;
#pragma unroll
    for (int r = 0; r < kRows; r++) {
      const uint64_t d = a[r] ^ b;
      const int dist = __popcll((d | (d >> 1)) & 0x5555555555555555ull);
      mine[(ai[r] < bj ? dist : kBins) * kBlock] += 1;
    }
  }
  __syncthreads();
  if (tid < kBins) {
    unsigned long long s = 0;
    for (int k = 0; k < kBlock; k++) s += bins[tid * kBlock + k];
    if (s) atomicAdd(&hist[tid], s);
  }
}

}  // namespace

extern "C" {

const char* sct_bc_last_error(void) { return g_err.c_str(); }

int sct_bc_table_size(int64_t n_whitelist, size_t* bytes) {
  g_err.clear();
  if (!bytes) return fail(SCT_BC_EINVAL, "bytes is NULL");
  if (n_whitelist < 0 || n_whitelist > INT32_MAX) return fail(SCT_BC_EINVAL, "n_whitelist %lld outside 0..2^31-1", (long long)n_whitelist);
  *bytes = (size_t)slots_for(n_whitelist) * sizeof(Slot) + (size_t)n_whitelist * sizeof(uint64_t) +
           (size_t)(filter_bits_for(n_whitelist) / 8);
  return SCT_BC_OK;
}

static int check_table(const void* table, int64_t n_whitelist, int32_t L) {
  if (L < 1 || L > SCT_BC_MAX_CORRECT_LENGTH)
    return fail(SCT_BC_EINVAL, "barcode length %d outside 1..%d", L, SCT_BC_MAX_CORRECT_LENGTH);
  if (n_whitelist < 0 || n_whitelist > INT32_MAX) return fail(SCT_BC_EINVAL, "n_whitelist %lld outside 0..2^31-1", (long long)n_whitelist);
  if (!table || ((uintptr_t)table & 15)) return fail(SCT_BC_EINVAL, "table is NULL or not 16-byte aligned");
  return SCT_BC_OK;
}

int sct_bc_table_build(const uint64_t* codes, int64_t n_whitelist, int32_t L, void* table, size_t table_bytes,
                       void* stream) {
  g_err.clear();
  int rc = check_table(table, n_whitelist, L);
  if (rc) return rc;
  if (n_whitelist > 0 && !codes) return fail(SCT_BC_EINVAL, "codes is NULL");
  size_t need = 0;
  if ((rc = sct_bc_table_size(n_whitelist, &need))) return rc;
  if (table_bytes < need)
    return fail(SCT_BC_ESIZE, "table buffer of %zu bytes, %zu needed for %lld barcodes", table_bytes, need, (long long)n_whitelist);
  hipStream_t st = (hipStream_t)stream;
  const uint64_t n_slots = slots_for(n_whitelist);
  Slot* t = (Slot*)table;
  uint64_t* copy = (uint64_t*)(t + n_slots);
  uint32_t* filter = (uint32_t*)(copy + n_whitelist);
  const uint64_t filter_bits = filter_bits_for(n_whitelist);
  const int filter_shift = 64 - __builtin_ctzll(filter_bits);
  const uint64_t code_mask = (1ull << (2 * L)) - 1;
  const unsigned sb = (unsigned)((n_slots + kBlock - 1) / kBlock);
  SCT_LIB_HIP(SCT_BC_EHIP, hipMemsetAsync(filter, 0, filter_bits / 8, st));
  hipLaunchKernelGGL(bc_fill_empty, dim3(sb), dim3(kBlock), 0, st, (uint4*)table, n_slots);
  if (n_whitelist > 0) {
    const unsigned nb = (unsigned)((n_whitelist + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(bc_insert, dim3(nb), dim3(kBlock), 0, st, codes, n_whitelist, code_mask, t, n_slots - 1, copy, filter,
                       filter_shift);
    hipLaunchKernelGGL(bc_finalize, dim3(sb), dim3(kBlock), 0, st, t, n_slots, Filter{filter, filter_shift}, (int)L);
  }
  SCT_LIB_HIP(SCT_BC_EHIP, hipGetLastError());
  return SCT_BC_OK;
}

int sct_bc_correct(const void* table, int64_t n_whitelist, const uint8_t* raw, int64_t n, int32_t L,
                   int32_t* out_index, uint8_t* out_corrected, void* stream) {
  g_err.clear();
  int rc = check_table(table, n_whitelist, L);
  if (rc) return rc;
  if (n < 0) return fail(SCT_BC_EINVAL, "n %lld is negative", (long long)n);
  if (n == 0) return SCT_BC_OK;
  if (!raw || !out_index) return fail(SCT_BC_EINVAL, "raw or out_index is NULL");
  const int64_t blocks = (n + kBlock - 1) / kBlock;
  if (blocks > INT32_MAX) return fail(SCT_BC_EINVAL, "n %lld exceeds one launch (2^31-1 blocks of %d)", (long long)n, kBlock);
  const uint64_t n_slots = slots_for(n_whitelist);
  const Slot* t = (const Slot*)table;
  const uint64_t* copy = (const uint64_t*)(t + n_slots);
  const Filter f{(const uint32_t*)(copy + n_whitelist), 64 - __builtin_ctzll(filter_bits_for(n_whitelist))};
  hipStream_t st = (hipStream_t)stream;
  const bool l16 = L == 16 && !((uintptr_t)raw & 15) && !((uintptr_t)out_corrected & 15);
  if (l16)
    hipLaunchKernelGGL(bc_correct<true>, dim3((unsigned)blocks), dim3(kBlock), 0, st, t, n_slots - 1, f, copy, raw, n, (int)L,
                       out_index, out_corrected);
  else
    hipLaunchKernelGGL(bc_correct<false>, dim3((unsigned)blocks), dim3(kBlock), 0, st, t, n_slots - 1, f, copy, raw, n, (int)L,
                       out_index, out_corrected);
  SCT_LIB_HIP(SCT_BC_EHIP, hipGetLastError());
  return SCT_BC_OK;
}

int sct_bc_pair_hist(const uint64_t* codes, int64_t n, int32_t L, uint64_t* hist, void* stream) {
  g_err.clear();
  if (L < 1 || L > SCT_BC_MAX_PAIR_LENGTH) return fail(SCT_BC_EINVAL, "barcode length %d outside 1..%d", L, SCT_BC_MAX_PAIR_LENGTH);
  if (n < 0 || n > (1ll << 22)) return fail(SCT_BC_EINVAL, "n %lld outside 0..2^22", (long long)n);
  if (!hist || (n > 0 && !codes)) return fail(SCT_BC_EINVAL, "codes or hist is NULL");
  hipStream_t st = (hipStream_t)stream;
  SCT_LIB_HIP(SCT_BC_EHIP, hipMemsetAsync(hist, 0, kBins * sizeof(uint64_t), st));
  if (n < 2) return SCT_BC_OK;
  const unsigned nt = (unsigned)((n + kTile - 1) / kTile);  // <= 4096: the grid is nt x nt blocks, never n^2
  hipLaunchKernelGGL(bc_pair_hist, dim3(nt, nt), dim3(kBlock), 0, st, codes, n, (unsigned long long*)hist);
  SCT_LIB_HIP(SCT_BC_EHIP, hipGetLastError());
  return SCT_BC_OK;
}

}  // extern "C"
