/* sct_fastq.h -- FASTQ text to fixed-width barcode columns on the GPU
 * (libsct_fastq.so, HIP, gfx950).
 *
 * Replaces the per-record loop under the reference's Attach10xBarcodes / AttachBarcodes: group
 * four lines (fastq.py:217-244 over reader.py:129-147), slice the sequence and the quality line
 * once per barcode (extract_barcode, fastq.py:252-278).  Here a window of decompressed FASTQ
 * text in device memory becomes one n x (end - start) byte column per barcode and line, the
 * layout sct_bc_correct (include/sct_barcode.h) takes as `raw`.
 *
 * The record rule is the reference's:
 *   - a line ends at '\n'; a last line without '\n' is still a line, but only in the last window
 *     of a stream (`is_last`);
 *   - record r is lines 4r .. 4r+3, whatever they contain; blank lines count as lines; a
 *     trailing group of fewer than four lines is dropped;
 *   - a barcode is bytes [start, end) of the sequence line and of the quality line, counted from
 *     the first byte of the line.  CRLF files therefore need no special handling (the '\r' sits
 *     at the line's end).  Lone-CR line ends are NOT supported: such a file is one long line.
 *
 * Two calls, count then fill.  sct_fq_count says how many complete records the window holds and
 * where the last of them ends; the caller sizes the columns, calls sct_fq_extract on the same
 * window and carries the bytes from `consumed` on into the next window.
 *
 * Conventions as include/sct_barcode.h: plain device pointers, sizes and a hipStream_t;
 * caller-owned buffers with a size query; 0 on success, a negative code with
 * sct_fq_last_error() otherwise.  Nothing is launched when a call returns an error.
 */
#ifndef SCT_FASTQ_H
#define SCT_FASTQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCT_FQ_OK 0
#define SCT_FQ_EINVAL -1 /* NULL or misaligned pointer, negative size, bad span */
#define SCT_FQ_ESIZE -2  /* the caller's workspace is too small                 */
#define SCT_FQ_EHIP -3   /* a HIP call failed                                   */

#define SCT_FQ_MAX_SPANS 4
#define SCT_FQ_TILE_BYTES 16384 /* text bytes per 256-thread block */

#define SCT_FQ_SHORT_SEQUENCE 1 /* flags bit 0: the sequence line is shorter than the largest `end` */
#define SCT_FQ_SHORT_QUALITY 2  /* flags bit 1: the same for the quality line                        */
#define SCT_FQ_BAD_NAME 4       /* flags bit 2: the name line does not begin with '@'                */

/* The result block, in device memory, 8-byte aligned.  sct_fq_count writes n_records, consumed
 * and n_lines and sets first_flagged to -1; sct_fq_extract writes first_flagged only. */
typedef struct sct_fq_result {
  int64_t n_records;     /* complete records in the window */
  int64_t consumed;      /* byte offset just past the last complete record (0 when there is none) */
  int64_t n_lines;       /* lines in the window (an unterminated last line counts only with is_last) */
  int64_t first_flagged; /* smallest record index with a non-zero flag, or -1 */
} sct_fq_result_t;

typedef struct sct_fq_span {
  int32_t start, end; /* 0 <= start < end */
} sct_fq_span_t;

/* Message of the calling thread's last error ("" if none). */
const char* sct_fq_last_error(void);

/* Bytes of the workspace of an `n_bytes` window: per tile the number of the tile's first line
 * (uint64) and its '\n' count (uint32).  sct_fq_count fills it, sct_fq_extract reads it. */
int sct_fq_workspace_size(int64_t n_bytes, size_t* bytes);

/* Counts the lines of `text` (device, 16-byte aligned, n_bytes >= 0; may be NULL when n_bytes is
 * 0) into `result` and leaves every tile's first line number in `workspace` (device, 8-byte
 * aligned).  Pass 1 counts '\n' per tile; one block scans the tile counts and finds the byte
 * after the '\n' that ends line 4 * n_records - 1 (n_bytes when that line is the unterminated
 * last one). */
int sct_fq_count(const uint8_t* text, int64_t n_bytes, int32_t is_last, void* workspace, size_t workspace_bytes,
                 sct_fq_result_t* result, void* stream);

/* Fills the columns of the first `n_records` records of the window sct_fq_count just counted
 * (same text, n_bytes and workspace; n_records <= result->n_records).  `spans`, `seq_cols` and
 * `qual_cols` are host arrays of n_spans (1..SCT_FQ_MAX_SPANS) entries, read before the call
 * returns; seq_cols[s] and qual_cols[s] are device buffers of n_records x (end - start) bytes,
 * row-major.  `flags` (device, 4-byte aligned, capacity n_records rounded up to a multiple of 4
 * bytes) gets SCT_FQ_* bits per record; a line shorter than the largest `end` leaves zero bytes
 * in its columns from the line's end on.  result->first_flagged is the first flagged record.
 * Pass 2 re-reads every tile and ranks its '\n's: the '\n' ending line 4r is followed by record
 * r's sequence line, whose slices are read from global memory (a slice may run past the tile),
 * the '\n' ending line 4r+2 by the quality line, and the '\n' ending line 4r+3 by the next name,
 * which must begin with '@' (byte 0 of the window for record 0). */
int sct_fq_extract(const uint8_t* text, int64_t n_bytes, int64_t n_records, const void* workspace,
                   size_t workspace_bytes, const sct_fq_span_t* spans, int32_t n_spans, uint8_t* const* seq_cols,
                   uint8_t* const* qual_cols, uint8_t* flags, sct_fq_result_t* result, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCT_FASTQ_H */
