/* sct_fastq_inflate.h -- BGZF-compressed FASTQ inflated on the GPU (libsct_fastq.so, HIP, gfx950).
 *
 * A BGZF file (bgzip, samtools fastq, this project's own FASTQ shards) is a run of gzip members
 * of at most 64 KiB, each of which says how long it is.  The host hops the member headers
 * (sct_fq_bgzf_scan, no zlib), copies the compressed bytes of a run of whole members to the
 * device, and sct_fq_inflate turns them into text where sct_fq_count (include/sct_fastq.h) reads
 * it: one wavefront per member inflates it (k_inflate, the kernel libsct_gbam.so uses for BAM),
 * then one wavefront per member computes the gzip CRC-32 of the payload where the inflate just
 * wrote it and compares it with the member's trailer.  Nothing is trusted that the host's gzip
 * would have checked: a member's status says whether its deflate stream, its ISIZE and its CRC
 * held.
 *
 * THE SLACK CONTRACT.  k_inflate reads the compressed bytes as 32-bit words from a 4-byte aligned
 * base and loads up to three refills of its ring (1.5 KiB) beyond the word it is decoding.  The
 * compressed buffer must therefore be 4-byte aligned and hold SCT_FQ_INFLATE_SLACK readable bytes
 * behind the `comp_bytes` in use; sct_fq_inflate zeroes them and refuses, without launching, a
 * buffer whose capacity does not have them.
 *
 * Conventions as include/sct_fastq.h: plain device pointers, sizes and a hipStream_t; a size
 * query for the workspace; 0 or a negative SCT_FQ_* code with sct_fq_last_error(); nothing is
 * launched when a call returns an error.
 */
#ifndef SCT_FASTQ_INFLATE_H
#define SCT_FASTQ_INFLATE_H

#include <stddef.h>
#include <stdint.h>

#include "sct_fastq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCT_FQ_ENOTBGZF -4 /* sct_fq_bgzf_scan: the bytes at *stopped_at are no whole BGZF member */

#define SCT_FQ_INFLATE_SLACK 65536 /* readable bytes behind the compressed bytes, zeroed by sct_fq_inflate */
#define SCT_FQ_MAX_ISIZE 65536     /* a BGZF member holds at most this much */

/* Member status words: 0 the payload is in place and its CRC holds, 1..9 the inflate's verdict
 * (block type, stored length, code counts, code sets, code lengths, symbol, distance, size, read
 * past the member's end), 10 the payload inflated and its CRC-32 is not the trailer's. */
#define SCT_FQ_ST_OK 0
#define SCT_FQ_ST_CRC 10

/* One member of a run: where its raw deflate data begins in the compressed buffer, where its
 * payload goes (counted from the call's destination), and the two lengths. */
typedef struct sct_fq_member {
  uint64_t in_off;
  uint64_t out_off;
  uint32_t clen;
  uint32_t isize;
} sct_fq_member_t;

/* Walks the gzip member headers of the file image `file` (host memory, `size` bytes) from byte
 * `from`, for at most `max_members` members.  A member is BGZF when it begins 1f 8b 08 with FLG
 * bit 2 set, carries the subfield 'B' 'C' with SLEN 2 anywhere in its extra field, its BSIZE + 1
 * bytes lie within the file and hold the header, the trailer and no less, and its ISIZE is at most
 * SCT_FQ_MAX_ISIZE.  members[i].in_off is the file offset of member i's deflate data, out_off the
 * payload bytes of the members before it in this call, crcs[i] its stored CRC-32.  *n_members is
 * the number written and *stopped_at the file offset behind the last of them: `size` when the
 * file was walked to its end.  Returns SCT_FQ_ENOTBGZF ("not BGZF at byte N") when the bytes at
 * *stopped_at are anything else -- a plain gzip member, a member cut short, a BSIZE past the end,
 * trailing bytes; the members before it are still reported. */
int sct_fq_bgzf_scan(const uint8_t* file, int64_t size, int64_t from, int64_t max_members, sct_fq_member_t* members,
                     uint32_t* crcs, int64_t* n_members, int64_t* stopped_at);

/* The gzip CRC-32 of `n` bytes on the host, by the routine the device kernel runs (64 slices
 * aligned to the data's end, folded in six steps). */
uint32_t sct_fq_crc32(const uint8_t* data, int64_t n);

/* Bytes of the device workspace of a run of `n_members`: the member table and the stored CRCs. */
int sct_fq_inflate_workspace_size(int64_t n_members, size_t* bytes);

/* Inflates the `n_members` members of `members` (host array; in_off counted from `comp`) from the
 * compressed bytes `comp` (device, 4-byte aligned, `comp_bytes` in use, `comp_capacity` >=
 * comp_bytes + SCT_FQ_INFLATE_SLACK allocated) into text + text_off + out_off, and checks every
 * payload against `crcs` (host array).  The two host arrays are checked before the call returns
 * and copied to the workspace on the stream: they stay unchanged until the stream has passed the
 * call (from pinned memory the copy does not wait for the host).  `status` (device, n_members
 * words) gets each member's SCT_FQ_ST_*; `summary` (device, 2 words, 4-byte aligned) the number of
 * members whose status is not 0 and the index of the first of them (0xffffffff: none).  A member
 * whose in_off + clen exceeds comp_bytes or whose text_off + out_off + isize exceeds
 * `text_capacity`, or whose isize exceeds SCT_FQ_MAX_ISIZE, is refused with SCT_FQ_EINVAL. */
int sct_fq_inflate(const uint8_t* comp, int64_t comp_bytes, int64_t comp_capacity, const sct_fq_member_t* members,
                   const uint32_t* crcs, int64_t n_members, uint8_t* text, int64_t text_capacity, int64_t text_off,
                   void* workspace, size_t workspace_bytes, uint32_t* status, uint32_t* summary, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCT_FASTQ_INFLATE_H */
