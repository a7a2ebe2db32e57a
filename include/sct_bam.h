/* sct_bam.h -- native BAM -> columnar decoder for the metric path (host C++, zlib, OpenMP).
 *
 * Replaces the per-record pysam reads of the reference's aggregation loop
 * (MetricAggregator.parse_molecule, aggregator.py:251-334; CellMetrics.parse_extra_fields,
 * aggregator.py:507-530; pysam 0.16 AlignedSegment.query_alignment_qualities /
 * get_cigar_stats) with one parallel pass: BGZF blocks are inflated concurrently,
 * records are parsed concurrently, and the CB / UB / GE tag strings are dictionary-encoded
 * to ids that are ranks of the sorted strings with a missing tag first (ids compare as the
 * strings compare).  Output: the 32-byte-per-record SoA columns of include/sctools_gpu.h.
 *
 * The decode validates exactly as sctools_amd.columnar.columnarize (and so the reference):
 * the FIRST offending record in file order decides the error, reported as a code below
 * and a message (the Python layer raises the reference's exception types).
 */
#ifndef SCT_BAM_H
#define SCT_BAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCT_BAM_OK 0
#define SCT_BAM_EIO -1          /* cannot open / read / inflate the file            */
#define SCT_BAM_EFORMAT -2      /* not a BAM file or a truncated record             */
#define SCT_BAM_KEYERROR -10    /* a required tag is missing (KeyError)             */
#define SCT_BAM_TYPEERROR -11   /* missing base qualities (TypeError)               */
#define SCT_BAM_ZERODIV -12     /* empty quality string (ZeroDivisionError)         */
#define SCT_BAM_VALUEERROR -13  /* invalid clipping, or a record beyond the 32-byte columnar limits */
#define SCT_BAM_EMPTY -14       /* no records (RuntimeError: StopIteration in iter_tag_groups) */
#define SCT_BAM_MISSING_TAG -15 /* sct_bam_split: a record carries none of the tags (RuntimeError, bam.py:286-289) */
#define SCT_BAM_ETYPED -16      /* sct_bam_decode*: a dictionary tag holds a float or array value (or, for
                                 * SCT_BAM_SORT_KEYS, an integer): decode with the Python reader instead */

#define SCT_BAM_CELL_METRICS 0 /* require CY (and CR where CB is present), as CellMetrics does   */
#define SCT_BAM_GENE_METRICS 1 /* records of multi-gene GE values are not validated (gatherer.py:210-212) */
#define SCT_BAM_COUNT_MATRIX 2 /* CountMatrix.from_sorted_tagged_bam (count.py:134-328): only the cell /
                                * molecule / gene tags, XF and the query name are read, nothing is
                                * validated, an empty file is 0 records, and the "qhead" column is set */

#define SCT_BAM_SORT_KEYS 3   /* TagSortBam / VerifyBamSort keys (bam.py:638-724): the three dictionary tags
                                * (a missing tag and an empty value are both id 0: get_tag_or_default's "")
                                * and the query name, ranked into a fourth dictionary (column "qname",
                                * int32); nothing is validated, an empty file is 0 records */

#define SCT_BAM_TAGSORT 4     /* the native TagSort's per-read rule (fastqpreprocessing/src/htslib_tagsort.cpp:
                                * 106-218) on the three named string tags (barcode, umi, gene): nothing is
                                * validated; a missing tag and the value "-" are the missing id; the unmapped
                                * bit is refID == -1; the gq_* columns cover all base qualities; CY / UY
                                * lengths of 0 are kept; the perfect-barcode bits are strcmp(tag or "None",
                                * CR / UR or ""); an empty file is 0 records */

#define SCT_BAM_TAG_CB 0
#define SCT_BAM_TAG_UB 1
#define SCT_BAM_TAG_GE 2
#define SCT_BAM_QNAME 3 /* SCT_BAM_SORT_KEYS: the query-name dictionary */

typedef struct sct_bam sct_bam_t;

/* Decode `path` (BAM).  n_threads <= 0: all cores.  On success *out owns the columns and
 * dictionaries until sct_bam_close.  On a validation error *out is NULL, *bad_record (if
 * set) is the offending record's index, and sct_bam_last_error() holds the message. */
int sct_bam_decode(const char* path, int32_t metric_mode, int32_t n_threads, sct_bam_t** out,
                   int64_t* bad_record);

/* As sct_bam_decode, with the three dictionary tags named by `tags` (6 characters: cell,
 * molecule, gene tag, e.g. "CBUBGE" -- the CreateCountMatrix -c / -m / -g options,
 * platform.py:402-429).  The metric modes require "CBUBGE". */
int sct_bam_decode_tags(const char* path, int32_t metric_mode, const char* tags, int32_t n_threads,
                        sct_bam_t** out, int64_t* bad_record);

/* Message of the calling thread's last error ("" if none). */
const char* sct_bam_last_error(void);

/* Number of records. */
int64_t sct_bam_n(const sct_bam_t* b);

/* Host pointer to a column by name (the sct_records_t field names: "cell", "umi", "gene",
 * "ref", "pos", "gq_sum", "gq_len", "gq_gt30", "bits", "xf", "cy_gt30", "cy_len",
 * "uy_gt30", "uy_len"), or "qhead" (uint8: 1 where the record's query name differs from the
 * previous record's -- the itertools.groupby of count.py:83-86 -- SCT_BAM_COUNT_MATRIX only),
 * or "qname" (int32 rank of the query name, SCT_BAM_SORT_KEYS only);
 * NULL for an unknown name.  Valid until sct_bam_close. */
const void* sct_bam_column(const sct_bam_t* b, const char* name);

/* Dictionary of tag `which` (SCT_BAM_TAG_*, or SCT_BAM_QNAME): *n entries in id order; entry i is the UTF-8
 * string bytes[offsets[i] .. offsets[i + 1]); *has_none = 1 when id 0 is the missing value
 * (its bytes are empty). */
int sct_bam_dictionary(const sct_bam_t* b, int32_t which, int64_t* n, const char** bytes,
                       const int64_t** offsets, int32_t* has_none);

void sct_bam_close(sct_bam_t* b);

/* SplitBam (bam.split, bam.py:361-488; platform.py:153-223): the records of the input BAMs
 * into chunk files `<out_prefix>_<k>.bam`, k = 0 .. *n_out - 1, every barcode in exactly one
 * chunk.  A record's barcode is the value of the first of the `n_tags` two-character tags in
 * `tags` (priority order, e.g. "CBCR") it carries; records with none raise
 * SCT_BAM_MISSING_TAG when raise_missing, else they are dropped.  Barcodes are ranked in
 * string order and chunk k gets the barcodes of rank k (mod n_subfiles when there are more
 * barcodes than chunks), so *n_out = min(#barcodes, n_subfiles).  Records keep their file
 * order; several inputs (same reference list) are concatenated in input order.  Each chunk is
 * a BGZF file: the first input's header, the records (deflate `level` 0-9, 6 as htslib's
 * default), the EOF member.  n_threads <= 0: all cores.  On an error *bad_record (if set) is
 * the offending record's index over all inputs. */
int sct_bam_split(const char* const* in_paths, int32_t n_in, const char* out_prefix, const char* tags,
                  int32_t n_tags, int32_t n_subfiles, int32_t raise_missing, int32_t level, int32_t n_threads,
                  int32_t* n_out, int64_t* bad_record);

/* TagSortBam's output (platform.py:60-97, pysam writes the sorted records under the input's
 * header): the records of `in_path` written to `out_path` in the order `perm` gives
 * (perm[k] = the input index of output record k, a permutation of 0..n-1), byte for byte,
 * as BGZF (header members, 0xff00-byte record members, EOF) at zlib `level`. */
int sct_bam_write_order(const char* in_path, const char* out_path, const int64_t* perm, int64_t n, int32_t level,
                        int32_t n_threads);

/* ErrorsToCorrectBarcodesMap.correct_bam's host side (barcode.py:357-379: pysam get_tag("CR") per
 * record, set_tag("CB"), write): one string tag of every record as a fixed-length column, and the
 * file written back with another tag set from such a column.
 *
 * sct_bam_tag_collect inflates `in_path` and keeps its records until sct_bam_tag_close.  For every
 * record it finds the first `src_tag` (two characters, e.g. "CR") and the first `dst_tag` ("CB")
 * the record may already carry.  A record without `src_tag` is SCT_BAM_KEYERROR (the reference's
 * second get_tag raises it), a non-string value SCT_BAM_ETYPED; the first such record in file
 * order decides and *bad_record (if set) is its index.  Nothing has been written by then. */
typedef struct sct_bam_tags sct_bam_tags_t;
int sct_bam_tag_collect(const char* in_path, const char* src_tag, const char* dst_tag, int32_t L, int32_t n_threads,
                        sct_bam_tags_t** out, int64_t* bad_record);

/* Number of records. */
int64_t sct_bam_tag_n(const sct_bam_tags_t* t);

/* n x L bytes, row-major: record i's source value where it has exactly L bytes, zeros elsewhere. */
const uint8_t* sct_bam_tag_values(const sct_bam_tags_t* t);

/* The records whose source value has another length: *n of them, their indices (ascending) and
 * their values, entry k = bytes[offsets[k] .. offsets[k + 1]). */
int sct_bam_tag_others(const sct_bam_tags_t* t, int64_t* n, const int64_t** records, const char** bytes,
                       const int64_t** offsets);

/* Writes every collected record to `out_path` under the input's header with `dst_tag`:Z set: the
 * first `dst_tag` the record carried is removed and the new one appended as the last tag (what
 * pysam's set_tag does); every other byte of the record is unchanged.  Record i's value is row i
 * of `values` (n x L) where its source value has L bytes; for the k-th other record it is
 * other_bytes[other_offsets[k] .. other_offsets[k + 1]), or, with those NULL, its own source
 * value (correct_bam's `except KeyError` pass-through).  BGZF output as sct_bam_write_order's. */
int sct_bam_tag_write(const sct_bam_tags_t* t, const char* out_path, const char* dst_tag, const uint8_t* values,
                      const char* other_bytes, const int64_t* other_offsets, int32_t level, int32_t n_threads);

void sct_bam_tag_close(sct_bam_tags_t* t);

/* bam.Tagger.tag's host side (bam.py:208-233: zip the tag generators with the records, set_tag
 * every yielded tag, write): string tags attached to the records of a BAM from byte columns, a
 * window of records at a time.
 *
 * sct_bam_attach_open inflates `in_path`, keeps its records until sct_bam_attach_close, and
 * writes the input's header to `out_path` (BGZF at zlib `level`, members as sct_bam_write_order's;
 * n_threads <= 0: all cores). */
typedef struct sct_bam_attach sct_bam_attach_t;
int sct_bam_attach_open(const char* in_path, const char* out_path, int32_t level, int32_t n_threads,
                        sct_bam_attach_t** out);

/* Number of records of the input. */
int64_t sct_bam_attach_n(const sct_bam_attach_t* h);

/* Writes the next `n` input records.  `tag_names` is 2 * n_tags characters.  For each record,
 * every listed tag is set in order with pysam's set_tag semantics: the first existing occurrence
 * of that tag is cut out and TAG:Z:value is appended as the last tag (so a tag listed twice keeps
 * the later value); every other byte of the record is unchanged.  values[t] is n x strides[t]
 * bytes, row-major; lengths[t] is int32[n], the bytes of row i that are the value, or NULL (as
 * `lengths` itself may be) for "all strides[t]".  A length of -1 means record i does not get tag
 * t.  If fewer than n records remain in the input it writes those; *n_written (if set) is the
 * number written.  Nothing is appended when the call returns an error. */
int sct_bam_attach_write(sct_bam_attach_t* h, int64_t n, int32_t n_tags, const char* tag_names,
                         const uint8_t* const* values, const int64_t* strides, const int32_t* const* lengths,
                         int64_t* n_written);

/* Writes the last member and the EOF member, closes the output and frees the handle.  The input
 * records that no call wrote are not copied (the zip of bam.py:229 ends with its shortest input). */
int sct_bam_attach_close(sct_bam_attach_t* h);

/* The shard writer of FastqProcess (bamshards.cpp): `n` BGZF files that grow together.
 *
 * sct_bam_shards_open creates paths[0..n).  headers[i] (`headers` itself may be NULL) is file i's
 * SAM header text, written as a BAM header with no references in members of its own; a file
 * without one gets no header at all and holds the appended bytes alone (a .fastq.gz shard: a BGZF
 * file is a multi-member gzip).  If a file cannot be created, those created before it are removed. */
typedef struct sct_bam_shards sct_bam_shards_t;
int sct_bam_shards_open(const char* const* paths, const char* const* headers, int32_t n, int32_t level,
                        int32_t n_threads, sct_bam_shards_t** out);

/* Appends data[bounds[i] .. bounds[i + 1]) to file i, for every i (bounds has n + 1 entries and
 * does not decrease).  Full 0xff00-byte members are deflated in parallel and written; the rest
 * waits for the next call, so the members do not depend on how the caller cut the stream.  On an
 * I/O error every file is removed and only close or abort may follow. */
int sct_bam_shards_append(sct_bam_shards_t* h, const uint8_t* data, const int64_t* bounds);

/* Writes every file's last member and EOF member, closes the files and frees the handle.  On an
 * error every file is removed. */
int sct_bam_shards_close(sct_bam_shards_t* h);

/* Closes and removes every file and frees the handle. */
void sct_bam_shards_abort(sct_bam_shards_t* h);

#ifdef __cplusplus
}
#endif

#endif /* SCT_BAM_H */
