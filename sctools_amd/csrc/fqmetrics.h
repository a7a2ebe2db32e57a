// fqmetrics.h -- the sct_fqm_* calls of libsct_fastq.so (include/sct_fastq_metrics.h): reads per
// distinct barcode in an open-addressing table in device memory, and the per-position base
// counts of the same column.  Included at the end of fastq.hip, whose error state (liberr.h) it
// shares.
//
//   k_fqm_accumulate  one 256-thread block per tile of 512 rows.  The tile (512 * L bytes, 16-byte
//                     aligned for every L) is staged in LDS with 16-byte loads.  Then
//                       - the matrix: thread t owns position t % L of rows t / L, t / L + 256 / L, ...
//                         (the threads of a wave read consecutive LDS bytes), keeps six counters in
//                         registers, adds the non-zero ones to a block matrix in LDS, and the block
//                         sends one global atomic per non-zero (position, class);
//                       - the table: thread t packs rows t and t + 256 into keys.  Equal keys of a
//                         tile are first summed in LDS: a row tries to claim the slot of its key's
//                         hash in a 512-slot direct-mapped key table with ONE compare-and-swap.
//                         The row that claims it OWNS the key and keeps it in a register; a row
//                         that finds its own key there adds one to the slot's counter and is done;
//                         a row that finds another key goes to the global table by itself.  After a
//                         barrier every owner inserts its key with 1 + the slot's counter.  A key
//                         that holds 5 % of the rows (poly-G reads) thus costs one global atomic per
//                         tile instead of ~25 on one address (28 -> 4 ms for
//                         20M rows, nothing lost on a column without such a key).
//                         A global probe first LOADS the slot's key: a key that is there already
//                         costs one atomic (the count), a new one two (the claim, the count).  A
//                         stale load is harmless: a slot's key changes once, from empty, so a stale
//                         "empty" only sends the thread to the compare-and-swap, which tells.
//                     New keys are counted per block in LDS and reach result->n_distinct as one
//                     atomic per block.
//   k_fqm_init        one 16-byte store per slot.
//   k_fqm_rehash      one thread per old slot, the same insert with the slot's count.
//   k_fqm_compact     one thread per slot; a wave reserves its output range with one atomic.
//
// Every probe loop runs at most n_slots times and no thread waits for another.
#include "../../include/sct_fastq_metrics.h"

namespace {

constexpr int kFqmBlock = 256;
constexpr int kFqmRows = SCT_FQM_TILE_ROWS;
constexpr int kFqmMaxL = SCT_FQM_MAX_LENGTH;
constexpr int kFqmClasses = SCT_FQM_PWM_CLASSES;
constexpr unsigned long long kFqmEmpty = SCT_FQM_EMPTY_KEY;
constexpr int64_t kFqmMaxSlots = (int64_t)1 << 36;  // 1 TiB of table: past any device, and the grids stay below 2^31 blocks
constexpr int kFqmPer = kFqmRows / kFqmBlock;  // rows a thread packs and inserts
constexpr int kFqmAgg = 512;                // slots of the block's key table in LDS
static_assert(kFqmRows % 16 == 0, "every tile starts 16-byte aligned for any L");
static_assert(kFqmRows % kFqmBlock == 0, "a thread inserts kFqmRows / kFqmBlock rows");
static_assert(kFqmMaxL * kFqmClasses <= kFqmBlock, "one thread per (position, class) in the flush");
static_assert(3 * kFqmMaxL < 64, "the key leaves bit 63 clear");

struct FqmSlot {
  unsigned long long key, count;
};
static_assert(sizeof(FqmSlot) == SCT_FQM_SLOT_BYTES, "a slot is 16 bytes");

__device__ __forceinline__ uint64_t fqm_mix(uint64_t k) {  // (the 64-bit finalizer of MurmurHash3)
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// Adds `add` to the count of `key`, claiming a slot for a new key (*claimed).  False: no slot in
// n_slots probes, nothing added.
__device__ __forceinline__ bool fqm_add(FqmSlot* __restrict__ table, uint64_t mask, unsigned long long key,
                                        unsigned long long add, bool* claimed) {
  uint64_t slot = fqm_mix(key) & mask;
  for (uint64_t probe = 0; probe <= mask; probe++) {
    unsigned long long cur = __hip_atomic_load(&table[slot].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kFqmEmpty) {
      cur = atomicCAS(&table[slot].key, kFqmEmpty, key);
      if (cur == kFqmEmpty) {
        *claimed = true;
        cur = key;
      }
    }
    if (cur == key) {
      atomicAdd(&table[slot].count, add);
      return true;
    }
    slot = (slot + 1) & mask;
  }
  return false;
}

// the key code of an upper-case base, 7 for any other byte
__device__ __forceinline__ uint32_t fqm_code(uint32_t b) {
  return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'N' ? 3u : b == 'T' ? 4u : 7u;
}

// the matrix class of a byte: A C G T N in either case, 5 for any other byte
__device__ __forceinline__ uint32_t fqm_class(uint32_t b) {
  const uint32_t u = b & 0xDFu;  // 'a' -> 'A'; no other byte becomes a letter it was not
  return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : u == 'N' ? 4u : 5u;
}

__global__ void __launch_bounds__(kFqmBlock) k_fqm_accumulate(const uint8_t* __restrict__ col, int64_t n, int L,
                                                              FqmSlot* __restrict__ table, uint64_t mask,
                                                              unsigned long long* __restrict__ pwm,
                                                              int64_t* __restrict__ exceptions,
                                                              sct_fqm_result_t* __restrict__ result) {
  __shared__ uint4 s_tile4[kFqmRows * kFqmMaxL / 16];
  __shared__ uint32_t s_pwm[kFqmMaxL * kFqmClasses];
  __shared__ uint32_t s_distinct, s_dropped;
  __shared__ unsigned long long s_akey[kFqmAgg];  // the tile's keys by hash, direct-mapped: the first row to come owns the slot
  __shared__ uint32_t s_acnt[kFqmAgg];            // rows of the same key that came after the owner
  const uint8_t* s_tile = reinterpret_cast<const uint8_t*>(s_tile4);
  const int tid = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kFqmRows;
  const int rows = (int)min((int64_t)kFqmRows, n - row0);
  const int groups = (rows * L + 15) >> 4;  // at most kFqmRows * kFqmMaxL / 16
  for (int g = tid; g < groups; g += kFqmBlock) s_tile4[g] = load_group(col, row0 * L + (int64_t)g * 16, n * L);
  if (tid < L * kFqmClasses) s_pwm[tid] = 0;
  if (tid == 0) s_distinct = 0, s_dropped = 0;
  for (int at = tid; at < kFqmAgg; at += kFqmBlock) s_akey[at] = kFqmEmpty, s_acnt[at] = 0;
  __syncthreads();

  const int per = kFqmBlock / L;  // rows per sweep of the block
  if (tid < per * L) {
    const int pos = tid % L;
    uint32_t cnt[kFqmClasses] = {0, 0, 0, 0, 0, 0};
    for (int r = tid / L; r < rows; r += per) {
      const uint32_t c = fqm_class(s_tile[r * L + pos]);
#pragma unroll
      for (int k = 0; k < kFqmClasses; k++) cnt[k] += c == (uint32_t)k;
    }
#pragma unroll
    for (int k = 0; k < kFqmClasses; k++)
      if (cnt[k]) atomicAdd(&s_pwm[pos * kFqmClasses + k], cnt[k]);
  }

  unsigned long long own_key[kFqmPer];
  int own_at[kFqmPer];
#pragma unroll
  for (int i = 0; i < kFqmPer; i++) {
    own_at[i] = -1;
    const int r = tid + i * kFqmBlock;
    if (r >= rows) continue;
    unsigned long long key = 0;
    uint32_t bad = 0;
    for (int j = 0; j < L; j++) {
      const uint32_t c = fqm_code(s_tile[r * L + j]);
      bad |= c == 7u;
      key = (key << 3) | (c & 7u);
    }
    if (bad) {
      const unsigned long long at = atomicAdd((unsigned long long*)&result->n_exceptions, 1ull);
      exceptions[at] = row0 + r;
      continue;
    }
    const int at = (int)((uint32_t)fqm_mix(key) & (kFqmAgg - 1));
    const unsigned long long prev = atomicCAS(&s_akey[at], kFqmEmpty, key);
    if (prev == kFqmEmpty) {
      own_at[i] = at;
      own_key[i] = key;
    } else if (prev == key) {
      atomicAdd(&s_acnt[at], 1u);
    } else {
      bool claimed = false;
      if (!fqm_add(table, mask, key, 1ull, &claimed)) atomicAdd(&s_dropped, 1u);
      if (claimed) atomicAdd(&s_distinct, 1u);
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kFqmPer; i++) {
    if (own_at[i] < 0) continue;
    const uint32_t c = 1u + s_acnt[own_at[i]];
    bool claimed = false;
    if (!fqm_add(table, mask, own_key[i], (unsigned long long)c, &claimed)) atomicAdd(&s_dropped, c);
    if (claimed) atomicAdd(&s_distinct, 1u);
  }
  __syncthreads();
  if (tid < L * kFqmClasses && s_pwm[tid]) atomicAdd(&pwm[tid], (unsigned long long)s_pwm[tid]);
  if (tid == 0) {
    if (s_distinct) atomicAdd((unsigned long long*)&result->n_distinct, (unsigned long long)s_distinct);
    if (s_dropped) atomicAdd((unsigned long long*)&result->error, (unsigned long long)s_dropped);
  }
}

// every slot {empty key, count 0}, one 16-byte store each
__global__ void __launch_bounds__(kFqmBlock) k_fqm_init(uint4* __restrict__ table, int64_t n_slots) {
  const int64_t i = (int64_t)blockIdx.x * kFqmBlock + threadIdx.x;
  if (i < n_slots) table[i] = make_uint4(0xffffffffu, 0xffffffffu, 0u, 0u);
}

__global__ void __launch_bounds__(kFqmBlock) k_fqm_rehash(const FqmSlot* __restrict__ old_table, int64_t old_slots,
                                                          FqmSlot* __restrict__ new_table, uint64_t mask,
                                                          sct_fqm_result_t* __restrict__ result) {
  const int64_t i = (int64_t)blockIdx.x * kFqmBlock + threadIdx.x;
  if (i >= old_slots) return;
  const FqmSlot s = old_table[i];
  if (s.key == kFqmEmpty) return;
  bool claimed = false;
  if (!fqm_add(new_table, mask, s.key, s.count, &claimed)) atomicAdd((unsigned long long*)&result->error, 1ull);
}

__global__ void __launch_bounds__(kFqmBlock) k_fqm_compact(const FqmSlot* __restrict__ table, int64_t n_slots,
                                                           uint64_t* __restrict__ keys, int64_t* __restrict__ counts,
                                                           int64_t capacity, sct_fqm_result_t* __restrict__ result) {
  const int64_t i = (int64_t)blockIdx.x * kFqmBlock + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  FqmSlot s{kFqmEmpty, 0};
  if (i < n_slots) s = table[i];
  const bool occupied = s.key != kFqmEmpty;
  const unsigned long long ballot = __ballot(occupied);
  if (!ballot) return;
  const int leader = __ffsll((long long)ballot) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd((unsigned long long*)&result->n_compacted, (unsigned long long)__popcll(ballot));
  base = (unsigned long long)__shfl((long long)base, leader, kWave);
  if (!occupied) return;
  const int64_t at = (int64_t)base + __popcll(ballot & ((1ull << lane) - 1));
  if (at < capacity) {
    keys[at] = s.key;
    counts[at] = (int64_t)s.count;
  } else {
    atomicAdd((unsigned long long*)&result->error, 1ull);
  }
}

int fqm_check_table(const void* table, int64_t n_slots, size_t table_bytes, const char* what) {
  if (n_slots < SCT_FQM_MIN_SLOTS || n_slots > kFqmMaxSlots || (n_slots & (n_slots - 1)))
    return fail(SCT_FQM_EINVAL, "%s: n_slots %lld is not a power of two in %d..2^36", what, (long long)n_slots,
                SCT_FQM_MIN_SLOTS);
  if (!table || ((uintptr_t)table & 15)) return fail(SCT_FQM_EINVAL, "%s is NULL or not 16-byte aligned", what);
  const size_t need = (size_t)n_slots * SCT_FQM_SLOT_BYTES;
  if (table_bytes < need) return fail(SCT_FQM_ESIZE, "%s of %zu bytes, %zu needed for %lld slots", what, table_bytes, need, (long long)n_slots);
  return SCT_FQM_OK;
}

int fqm_check_result(const sct_fqm_result_t* result) {
  if (!result || ((uintptr_t)result & 7)) return fail(SCT_FQM_EINVAL, "result is NULL or not 8-byte aligned");
  return SCT_FQM_OK;
}

}  // namespace

extern "C" {

const char* sct_fqm_last_error(void) { return g_err.c_str(); }

int sct_fqm_table_size(int64_t n_slots, size_t* bytes) {
  g_err.clear();
  if (!bytes) return fail(SCT_FQM_EINVAL, "NULL bytes");
  if (n_slots < SCT_FQM_MIN_SLOTS || n_slots > kFqmMaxSlots || (n_slots & (n_slots - 1)))
    return fail(SCT_FQM_EINVAL, "n_slots %lld is not a power of two in %d..2^36", (long long)n_slots, SCT_FQM_MIN_SLOTS);
  *bytes = (size_t)n_slots * SCT_FQM_SLOT_BYTES;
  return SCT_FQM_OK;
}

int sct_fqm_table_init(void* table, int64_t n_slots, size_t table_bytes, void* stream) {
  g_err.clear();
  const int rc = fqm_check_table(table, n_slots, table_bytes, "table");
  if (rc) return rc;
  hipLaunchKernelGGL(k_fqm_init, dim3((unsigned)((n_slots + kFqmBlock - 1) / kFqmBlock)), dim3(kFqmBlock), 0,
                     (hipStream_t)stream, (uint4*)table, n_slots);
  SCT_LIB_HIP(SCT_FQM_EHIP, hipGetLastError());
  return SCT_FQM_OK;
}

int sct_fqm_accumulate(const uint8_t* col, int64_t n, int32_t L, void* table, int64_t n_slots, size_t table_bytes,
                       int64_t* pwm, int64_t* exceptions, sct_fqm_result_t* result, void* stream) {
  g_err.clear();
  if (L < 1 || L > SCT_FQM_MAX_LENGTH) return fail(SCT_FQM_EINVAL, "L %d outside 1..%d", L, SCT_FQM_MAX_LENGTH);
  if (n < 0) return fail(SCT_FQM_EINVAL, "negative n");
  if (n > ((int64_t)1 << 40)) return fail(SCT_FQM_EINVAL, "%lld rows are more than 2^40", (long long)n);
  if (n > 0 && !col) return fail(SCT_FQM_EINVAL, "NULL col");
  if ((uintptr_t)col & 15) return fail(SCT_FQM_EINVAL, "col is not 16-byte aligned");
  int rc = fqm_check_table(table, n_slots, table_bytes, "table");
  if (rc) return rc;
  if (!pwm || ((uintptr_t)pwm & 7)) return fail(SCT_FQM_EINVAL, "pwm is NULL or not 8-byte aligned");
  if (n > 0 && (!exceptions || ((uintptr_t)exceptions & 7))) return fail(SCT_FQM_EINVAL, "exceptions is NULL or not 8-byte aligned");
  if ((rc = fqm_check_result(result))) return rc;
  hipStream_t s = (hipStream_t)stream;
  SCT_LIB_HIP(SCT_FQM_EHIP, hipMemsetAsync(&result->n_exceptions, 0, sizeof(int64_t), s));
  if (n == 0) return SCT_FQM_OK;
  const int64_t tiles = (n + kFqmRows - 1) / kFqmRows;
  hipLaunchKernelGGL(k_fqm_accumulate, dim3((unsigned)tiles), dim3(kFqmBlock), 0, s, col, n, (int)L, (FqmSlot*)table,
                     (uint64_t)(n_slots - 1), (unsigned long long*)pwm, exceptions, result);
  SCT_LIB_HIP(SCT_FQM_EHIP, hipGetLastError());
  return SCT_FQM_OK;
}

int sct_fqm_rehash(const void* old_table, int64_t old_slots, size_t old_bytes, void* new_table, int64_t new_slots,
                   size_t new_bytes, sct_fqm_result_t* result, void* stream) {
  g_err.clear();
  int rc = fqm_check_table(old_table, old_slots, old_bytes, "old table");
  if (rc) return rc;
  if ((rc = fqm_check_table(new_table, new_slots, new_bytes, "new table"))) return rc;
  if (old_table == new_table) return fail(SCT_FQM_EINVAL, "old and new table are the same");
  if ((rc = fqm_check_result(result))) return rc;
  hipLaunchKernelGGL(k_fqm_rehash, dim3((unsigned)((old_slots + kFqmBlock - 1) / kFqmBlock)), dim3(kFqmBlock), 0,
                     (hipStream_t)stream, (const FqmSlot*)old_table, old_slots, (FqmSlot*)new_table,
                     (uint64_t)(new_slots - 1), result);
  SCT_LIB_HIP(SCT_FQM_EHIP, hipGetLastError());
  return SCT_FQM_OK;
}

int sct_fqm_compact(const void* table, int64_t n_slots, size_t table_bytes, uint64_t* keys, int64_t* counts,
                    int64_t capacity, sct_fqm_result_t* result, void* stream) {
  g_err.clear();
  int rc = fqm_check_table(table, n_slots, table_bytes, "table");
  if (rc) return rc;
  if (capacity < 0) return fail(SCT_FQM_EINVAL, "negative capacity");
  if (capacity > 0 && (!keys || !counts || (((uintptr_t)keys | (uintptr_t)counts) & 7)))
    return fail(SCT_FQM_EINVAL, "keys or counts is NULL or not 8-byte aligned");
  if ((rc = fqm_check_result(result))) return rc;
  hipStream_t s = (hipStream_t)stream;
  SCT_LIB_HIP(SCT_FQM_EHIP, hipMemsetAsync(&result->n_compacted, 0, sizeof(int64_t), s));
  hipLaunchKernelGGL(k_fqm_compact, dim3((unsigned)((n_slots + kFqmBlock - 1) / kFqmBlock)), dim3(kFqmBlock), 0, s,
                     (const FqmSlot*)table, n_slots, keys, counts, capacity, result);
  SCT_LIB_HIP(SCT_FQM_EHIP, hipGetLastError());
  return SCT_FQM_OK;
}

}  // extern "C"
