/* sct_barcode.h -- whitelist barcode correction and barcode-set statistics on the GPU
 * (libsct_barcode.so, HIP, gfx950).
 *
 * Replaces the reference's sctools.barcode hot paths: the Python dict of every single-base
 * error of every whitelist barcode with one dict lookup per record
 * (ErrorsToCorrectBarcodesMap, barcode.py:311-335 and 357-379) and the itertools.combinations
 * loop over all barcode pairs (Barcodes.summarize_hamming_distances, barcode.py:73-103).
 *
 * Barcodes are 2 bits per base in a uint64_t in the reference's TwoBit code
 * (encodings.py:154-185): A=0, C=1, T=2, G=3, first base in the highest of the 2*L bits.
 *
 * The rule the dict implements (later writers overwrite earlier ones, barcode.py:323-335):
 *   corrected(x) = the whitelist barcode with the LARGEST file index among those at Hamming
 *   distance <= 1 from x, or none.  A query byte outside ACGT matches only if it is the one
 *   such byte and it is 'N' (the candidates are then the 4 substitutions at that position).
 *
 * Conventions as include/sctools_gpu.h: plain device pointers, sizes and a hipStream_t;
 * caller-owned buffers with a size query; 0 on success, a negative code with
 * sct_bc_last_error() otherwise.  Nothing is launched when a call returns an error.
 */
#ifndef SCT_BARCODE_H
#define SCT_BARCODE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCT_BC_OK 0
#define SCT_BC_EINVAL -1 /* NULL pointer, length outside the limits, negative count */
#define SCT_BC_ESIZE -2  /* the caller's table buffer is too small                   */
#define SCT_BC_EHIP -3   /* a HIP call failed                                         */

#define SCT_BC_MAX_CORRECT_LENGTH 31 /* a 62-bit code leaves ~0 free for "empty slot" */
#define SCT_BC_MAX_PAIR_LENGTH 32
#define SCT_BC_HIST_BINS 33 /* Hamming distances 0..32 */

/* Message of the calling thread's last error ("" if none). */
const char* sct_bc_last_error(void);

/* Bytes of the correction table of an `n_whitelist`-entry whitelist: a power-of-two number of
 * 16-byte slots {uint64 code, int32 raw index, int32 final index} at load factor <= 0.5,
 * followed by a copy of the n_whitelist codes in file order (index -> barcode, for the
 * corrected bytes) and a presence filter of one bit per hashed code (a power of two >= 16 bits
 * per barcode), which answers most neighbour candidates from L2 without a probe. */
int sct_bc_table_size(int64_t n_whitelist, size_t* bytes);

/* Builds the table in `table` (device, 16-byte aligned, `table_bytes` >= sct_bc_table_size)
 * from `codes` (device, n_whitelist TwoBit codes in file order, barcode length L in 1..31):
 * what _prepare_single_base_error_hash_table (barcode.py:311-335) builds as a dict of
 * (1 + 4*L) keys per barcode.  Pass 1: every entry claims the slot of its code and the slot
 * keeps the largest file index (atomic max), so a duplicate line counts with its later index.
 * Every entry also sets its bit of the presence filter.
 * Pass 2: every occupied slot probes its 3*L neighbours and stores final = max(raw index of
 * itself and of every neighbour present).  Bits of a code above 2*L are ignored. */
int sct_bc_table_build(const uint64_t* codes, int64_t n_whitelist, int32_t L, void* table, size_t table_bytes,
                       void* stream);

/* get_corrected_barcode for every row of `raw` (barcode.py:284-308; the record loop of
 * correct_bam, barcode.py:371-378).  `raw` is n x L ASCII bytes, row-major (a BAM's CR
 * values); `table` was built for the same n_whitelist and L.  out_index[i] (int32) is the
 * whitelist file index of the corrected barcode, or -1 (the dict's KeyError).  out_corrected
 * (may be NULL) is n x L bytes: the corrected barcode, or the raw bytes passed through where
 * there is none (correct_bam's `except KeyError` branch).  A barcode on the whitelist costs one
 * probe (its final index); any other costs 3*L filter tests (4 with one N) and a probe for each
 * that passes, spread over the wave. */
int sct_bc_correct(const void* table, int64_t n_whitelist, const uint8_t* raw, int64_t n, int32_t L,
                   int32_t* out_index, uint8_t* out_corrected, void* stream);

/* Barcodes.summarize_hamming_distances' distances (barcode.py:87-90) as a histogram:
 * hist[d] (device, uint64[SCT_BC_HIST_BINS], overwritten) = the number of unordered pairs
 * i < j of the n codes (device, L in 1..32, n <= 2^22) at Hamming distance d, exact. */
int sct_bc_pair_hist(const uint64_t* codes, int64_t n, int32_t L, uint64_t* hist, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCT_BARCODE_H */
