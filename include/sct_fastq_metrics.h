/* sct_fastq_metrics.h -- reads per distinct barcode and per-position base counts on the GPU
 * (libsct_fastq.so, HIP, gfx950).
 *
 * Replaces the per-read loop of the reference's fastq_metrics tool
 * (fastqpreprocessing/src/fastq_metrics.cpp: one unordered_map<string,int> and one switch per
 * base): a barcode column as sct_fq_extract (include/sct_fastq.h) writes it, uint8 [n, L]
 * row-major ASCII, goes into an open-addressing count table in device memory and into a
 * position weight matrix.
 *
 * The key.  Three bits per base in a uint64_t, the first base in the highest of the 3 * L bits,
 * with A=0 C=1 G=2 N=3 T=4: numeric key order is the byte order of the barcodes.  L is
 * 1..SCT_FQM_MAX_LENGTH (21): at L = 21 bit 63 is clear, and code 7 never occurs, so ~0 is the
 * empty slot.  A row with any byte outside upper-case ACGTN is an EXCEPTION ROW: it is not
 * inserted; its row index goes into the caller's list and the caller counts it on the host.
 *
 * The table.  n_slots slots of 16 bytes, {uint64 key, uint64 count}, n_slots a power of two of
 * at least SCT_FQM_MIN_SLOTS; linear probing from a mix of the key; the key claimed by a 64-bit
 * compare-and-swap, the count raised by an atomic add.
 *
 * THE GROWTH RULE (the caller's duty): before a column of n rows is accumulated, the table has
 * at least 2 * (D + n) slots, D being result->n_distinct so far; otherwise the caller
 * sct_fqm_rehash-es into the next power of two that has.  The table is then never more than
 * half full and a full table cannot occur.  Every probe loop is bounded by n_slots all the same:
 * a row (or a moved slot) that finds no place is dropped and counted in result->error, which
 * exists to show that this did not happen.  No kernel here waits on another thread.
 *
 * Conventions as include/sct_fastq.h: plain device pointers, sizes and a hipStream_t;
 * caller-owned buffers with a size query; 0 on success, a negative code with
 * sct_fqm_last_error() otherwise.  Nothing is launched when a call returns an error.
 */
#ifndef SCT_FASTQ_METRICS_H
#define SCT_FASTQ_METRICS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCT_FQM_OK 0
#define SCT_FQM_EINVAL -1 /* NULL or misaligned pointer, negative size, L or n_slots out of range */
#define SCT_FQM_ESIZE -2  /* the caller's table buffer is too small                                 */
#define SCT_FQM_EHIP -3   /* a HIP call failed                                                      */

#define SCT_FQM_MAX_LENGTH 21
#define SCT_FQM_MIN_SLOTS 64
#define SCT_FQM_SLOT_BYTES 16
#define SCT_FQM_TILE_ROWS 512 /* rows per 256-thread block of sct_fqm_accumulate */
#define SCT_FQM_PWM_CLASSES 6 /* A C G T N other */
#define SCT_FQM_EMPTY_KEY UINT64_MAX

/* The result block, in device memory, 8-byte aligned, zeroed by the caller before a table's
 * first call.  n_distinct and error run on from call to call; n_exceptions and n_compacted are
 * set anew by the call that writes them. */
typedef struct sct_fqm_result {
  int64_t n_distinct;   /* slots claimed by sct_fqm_accumulate so far                        */
  int64_t n_exceptions; /* exception rows of the last sct_fqm_accumulate                     */
  int64_t n_compacted;  /* occupied slots the last sct_fqm_compact met                       */
  int64_t error;        /* rows or slots dropped for want of a slot or of output room: 0     */
} sct_fqm_result_t;

/* Message of the calling thread's last error ("" if none). */
const char* sct_fqm_last_error(void);

/* Bytes of a table of n_slots slots. */
int sct_fqm_table_size(int64_t n_slots, size_t* bytes);

/* Empties `table` (device, 16-byte aligned, table_bytes >= the size query's answer). */
int sct_fqm_table_init(void* table, int64_t n_slots, size_t table_bytes, void* stream);

/* Reads the column `col` (device, 16-byte aligned, n x L bytes, n >= 0; may be NULL when n is 0)
 * once.  Per byte it adds one to pwm[position][class] (device, int64 [L][6], classes A C G T N
 * other; lower case counts as upper case here, as in the reference's recordChunk; the caller
 * zeroes it once).  Per row it adds one to the count of the row's key in `table`, claiming a
 * slot and raising result->n_distinct for a new key; an exception row instead goes into
 * `exceptions` (device, int64, room for n entries, in any order) and result->n_exceptions.
 * The growth rule above is the caller's. */
int sct_fqm_accumulate(const uint8_t* col, int64_t n, int32_t L, void* table, int64_t n_slots, size_t table_bytes,
                       int64_t* pwm, int64_t* exceptions, sct_fqm_result_t* result, void* stream);

/* Adds every occupied slot of `old_table`, with its count, into `new_table`, which is
 * initialised (or holds keys already: equal keys are summed) and has room by the growth rule. */
int sct_fqm_rehash(const void* old_table, int64_t old_slots, size_t old_bytes, void* new_table, int64_t new_slots,
                   size_t new_bytes, sct_fqm_result_t* result, void* stream);

/* Writes the occupied slots' keys and counts densely, in any order, into `keys` and `counts`
 * (device, room for `capacity` entries each; result->n_distinct entries are enough).
 * result->n_compacted is the number of occupied slots; those past `capacity` are not written
 * and raise result->error. */
int sct_fqm_compact(const void* table, int64_t n_slots, size_t table_bytes, uint64_t* keys, int64_t* counts,
                    int64_t capacity, sct_fqm_result_t* result, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCT_FASTQ_METRICS_H */
