/* sct_fastq_process.h -- FASTQ triples to sharded unaligned BAM / FASTQ records on the GPU
 * (the sct_fqp_* calls of libsct_fastq.so, HIP, gfx950).
 *
 * The device side of the reference's fastqprocess / fastq_slideseq (fastqpreprocessing/src/
 * fastq_common.cpp): whole lines of R2 (and I1), the output shard of every record from the hash
 * of its bucket barcode, a stable partition of the records by shard, and the output records
 * themselves, written where the partition puts them.  The host deflates what comes back.
 *
 *   sct_fqp_lines        text window (counted by sct_fq_count)  ->  offset and length of the
 *                        identifier, sequence and quality line of every record, and flags
 *   sct_fqp_shard        raw / corrected cell barcode columns    ->  shard per record, the
 *                        reference's three counts
 *   sct_fqp_plan         line lengths, shards                    ->  byte offset of every record
 *                        within its shard in input order; records and bytes per shard
 *   sct_fqp_emit_bam     everything above                        ->  BAM records
 *   sct_fqp_emit_fastq                                           ->  R1 and R2 FASTQ text
 *
 * Conventions as include/sct_fastq.h: plain device pointers, sizes and a hipStream_t;
 * caller-owned buffers with a size query; 0 on success, a negative SCT_FQ_* code with
 * sct_fq_last_error() otherwise.  Nothing is launched when a call returns an error.  All
 * offsets are 64-bit.
 */
#ifndef SCT_FASTQ_PROCESS_H
#define SCT_FASTQ_PROCESS_H

#include "sct_fastq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags of sct_fqp_lines, one byte per record */
#define SCT_FQP_BAD_NAME 1         /* the name line does not begin with '@'                     */
#define SCT_FQP_BAD_IDENTIFIER 2   /* the identifier is empty or longer than 254 bytes          */
#define SCT_FQP_EMPTY_SEQUENCE 4   /* the sequence line is empty                                */
#define SCT_FQP_LENGTH_MISMATCH 8  /* sequence and quality line differ in length                */
#define SCT_FQP_LOW_QUALITY 16     /* a quality byte is below 33                                */

#define SCT_FQP_MAX_IDENTIFIER 254 /* l_read_name is a uint8 that counts the NUL */
#define SCT_FQP_MAX_SHARDS 1024
#define SCT_FQP_MAX_BARCODE 31 /* SCT_BC_MAX_CORRECT_LENGTH */
#define SCT_FQP_PLAN_TILE 256  /* records per block of the partition */

#define SCT_FQP_BAM 0
#define SCT_FQP_FASTQ 1

#define SCT_FQP_BAM_BIN 4680 /* reg2bin(-1, 0): the bin of an unplaced read */

/* Whole lines.  For every one of the first `n_records` records of the window sct_fq_count just
 * counted (same text, n_bytes and workspace), line_off[3r + k] / line_len[3r + k] (device, 8- and
 * 4-byte aligned, 3 * n_records entries) get the byte offset in `text` and the length of
 *   k = 0  the identifier: the name line without its '@', up to the first space (the whole line
 *          where it does not begin with '@');
 *   k = 1  the sequence line;
 *   k = 2  the quality line.
 * One '\r' directly before the '\n' is not part of a line.  `flags` (device, 4-byte aligned,
 * n_records rounded up to a multiple of 4 bytes) gets SCT_FQP_* bits, result->first_flagged the
 * smallest flagged record or -1.  An identifier with no space in its first 255 bytes is reported
 * with the length of the rest of its line and flagged. */
int sct_fqp_lines(const uint8_t* text, int64_t n_bytes, int64_t n_records, const void* workspace,
                  size_t workspace_bytes, int64_t* line_off, int32_t* line_len, uint8_t* flags,
                  sct_fq_result_t* result, void* stream);

/* The shard of every record.  `raw` is the n x L cell barcode column (device, 16-byte aligned);
 * `corrected` (same shape and alignment) and `index` (int32 [n], 4-byte aligned) are the outputs of
 * sct_bc_correct, both NULL without a whitelist.  The bucket barcode is the corrected row where
 * index >= 0, else the raw row; shard[i] = hash(bucket) % n_shards with the hash that
 * std::hash<std::string> is under libstdc++ on x86-64 (_Hash_bytes, seed 0xc70f6907).
 * counts (device int64 [3], 8-byte aligned) is SET to: correctable with corrected == raw,
 * correctable and different, uncorrectable.  1 <= L <= 31, 1 <= n_shards <= 1024. */
int sct_fqp_shard(const uint8_t* raw, const uint8_t* corrected, const int32_t* index, int64_t n, int32_t L,
                  int32_t n_shards, int32_t* shard, int64_t* counts, void* stream);

/* What plan and emit read, a host struct of device pointers read before the call returns. */
typedef struct sct_fqp_records {
  int64_t n;               /* records */
  const uint8_t* r2_text;  /* the R2 window */
  int64_t r2_bytes;
  const int64_t* r2_off; /* sct_fqp_lines of it: 3 per record */
  const int32_t* r2_len;
  const uint8_t* i1_text; /* the same for I1; all four NULL / 0 without an I1 (no SR, SY) */
  int64_t i1_bytes;
  const int64_t* i1_off;
  const int32_t* i1_len;
  const uint8_t* cr; /* n x cell_length: cell barcode bases and qualities (sct_fq_extract) */
  const uint8_t* cy;
  const uint8_t* ur; /* n x umi_length (may be NULL when umi_length is 0) */
  const uint8_t* uy;
  const uint8_t* cb;       /* n x cell_length corrected barcode, NULL without a whitelist */
  const int32_t* cb_index; /* record i gets CB where cb_index[i] >= 0; NULL without a whitelist */
  const int32_t* shard;    /* sct_fqp_shard */
  int32_t cell_length;     /* 1..31 */
  int32_t umi_length;      /* 0..255 */
  int32_t n_shards;        /* 1..1024 */
  int32_t format;          /* SCT_FQP_BAM or SCT_FQP_FASTQ */
} sct_fqp_records_t;

/* Bytes of sct_fqp_plan's workspace: per tile of SCT_FQP_PLAN_TILE records and per shard a record
 * count and one (BAM) or two (FASTQ) byte totals. */
int sct_fqp_plan_workspace_size(int64_t n, int32_t n_shards, int32_t format, size_t* bytes);

/* Sizes and a stable partition.  Let K be 1 in BAM mode and 2 in FASTQ mode (the R1 text, the R2
 * text).  offsets (device int64 [K * n]) gets at [k * n + i] the byte offset of record i's output k
 * within its shard, the records of a shard in input order; shard_counts (int64 [n_shards]) the
 * records per shard; shard_bytes (int64 [K * n_shards]) at [k * n_shards + s] the bytes of shard
 * s's output k.  All 8-byte aligned.  The result is a function of the input alone: a histogram
 * per tile in LDS flushed with plain stores, a block scan per shard over the tiles, and a rank inside
 * the tile that walks the tile in order. */
int sct_fqp_plan(const sct_fqp_records_t* records, void* workspace, size_t workspace_bytes, int64_t* offsets,
                 int64_t* shard_counts, int64_t* shard_bytes, void* stream);

/* The BAM records: record i at out + shard_base[shard[i]] + offsets[i] (shard_base: device int64
 * [n_shards], the caller's exclusive scan of shard_bytes).  block_size, refID -1, pos -1,
 * l_read_name, mapq 0, bin 4680, n_cigar_op 0, flag 4, l_seq, next_refID -1, next_pos -1, tlen 0,
 * the identifier and a NUL, the sequence in 4-bit codes, the qualities minus 33, then the Z tags
 * RG=A CR CY UR UY [SR SY] [CB].  A record that would end past out_bytes, or whose lines end past
 * their text, is not written and *error (device int64, SET by the call) counts it. */
int sct_fqp_emit_bam(const sct_fqp_records_t* records, const int64_t* offsets, const int64_t* shard_base, uint8_t* out,
                     int64_t out_bytes, int64_t* error, void* stream);

/* The FASTQ texts: "@id\nCR+UR\n+\nCY+UY\n" at out1 + shard_base[s] + offsets[i] and
 * "@id\nseq\n+\nqual\n" at out2 + shard_base[n_shards + s] + offsets[n + i]. */
int sct_fqp_emit_fastq(const sct_fqp_records_t* records, const int64_t* offsets, const int64_t* shard_base,
                       uint8_t* out1, int64_t out1_bytes, uint8_t* out2, int64_t out2_bytes, int64_t* error,
                       void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCT_FASTQ_PROCESS_H */
