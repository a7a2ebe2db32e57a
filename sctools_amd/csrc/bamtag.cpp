// bamtag.cpp -- the host side of ErrorsToCorrectBarcodesMap.correct_bam (barcode.py:357-379):
// collect one string tag of every record into a fixed-length column, and write the file back with
// another tag set from such a column (include/sct_bam.h, sct_bam_tag_*).
//
// The reference reads each record through pysam, looks its CR up in a dict and writes it back with
// set_tag("CB").  Here pass 1 inflates the file (BGZF blocks in parallel, bgzf.h), finds every
// record's source tag and the destination tag it may already carry, and fills the n x L column
// the device lookup takes; pass 2 rebuilds every record -- the old destination tag cut out, the
// new one appended as the last tag (pysam's set_tag), every other byte as it was -- and hands the
// stream to the writer of sct_bam_write_order (bamwrite.h).  The inflated records stay in memory
// between the passes, as they do for TagSortBam.
//
// sct_bam_attach_* is bam.Tagger.tag's host side (bam.py:208-233): the input is inflated once, then
// every call rebuilds the next n records with the listed string tags set from byte columns and
// appends them to the output, whose BGZF members are written as they fill (bamwrite.h).
#include <fcntl.h>
#include <omp.h>
#include <stdlib.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/sct_bam.h"
#include "bamwrite.h"
#include "bgzf.h"

struct sct_bam_tags {
  std::string header;            // magic .. references, uncompressed
  std::vector<uint8_t> data;     // the whole inflated stream
  std::vector<uint64_t> starts;  // record starts (at the block_size field) in data
  std::vector<uint32_t> dst_off, dst_len;  // the destination tag the record carries (offset from the record start, bytes), len 0 = none
  std::vector<uint32_t> src_off, src_len;  // the source tag's value
  int32_t L = 0;
  std::vector<uint8_t> values;  // n x L: the source tag's value where it has L bytes, else zeros
  std::vector<uint8_t> fits;    // 1 where it has
  std::vector<int64_t> other_rec, other_off;  // records whose value has another length, and their values
  std::string other_bytes;
};

struct sct_bam_attach {
  std::vector<uint8_t> data;     // the whole inflated input
  std::vector<uint64_t> starts;  // record starts (at the block_size field) in data
  int64_t next = 0;              // the next input record to write
  int n_threads = 1;
  BamStreamWriter writer;
};

namespace {

int inflate_file(const char* path, std::vector<uint8_t>& data, int n_threads) {
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return fail(SCT_BAM_EIO, "cannot open %s", path);
  struct stat st;
  if (fstat(fd, &st) != 0 || st.st_size == 0) {
    close(fd);
    return fail(SCT_BAM_EFORMAT, "%s is empty", path);
  }
  const uint64_t size = (uint64_t)st.st_size;
  void* p = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
  close(fd);
  if (p == MAP_FAILED) return fail(SCT_BAM_EIO, "cannot map %s", path);
  struct Unmap {
    void* p;
    uint64_t n;
    ~Unmap() { munmap(p, n); }
  } unmap{p, size};
  const uint8_t* f = (const uint8_t*)p;
  std::vector<Block> blocks;
  int rc = scan_blocks(f, size, blocks);
  if (rc) return rc;
  std::vector<uint64_t> dst(blocks.size() + 1, 0);
  for (size_t k = 0; k < blocks.size(); k++) dst[k + 1] = dst[k] + blocks[k].isize;
  data.resize(dst.back());
  int bad = 0;
#pragma omp parallel num_threads(n_threads) reduction(| : bad)
  {
    z_stream z;
    memset(&z, 0, sizeof(z));
    inflateInit2(&z, -15);
#pragma omp for schedule(dynamic, 4)
    for (long k = 0; k < (long)blocks.size(); k++)
      if (blocks[k].isize && !inflate_block(f, blocks[k], data.data() + dst[k], z)) bad = 1;
    inflateEnd(&z);
  }
  if (bad) return fail(SCT_BAM_EIO, "cannot inflate a BGZF block of %s", path);
  return SCT_BAM_OK;
}

}  // namespace

extern "C" {

int sct_bam_tag_collect(const char* in_path, const char* src_tag, const char* dst_tag, int32_t L, int32_t n_threads,
                        sct_bam_tags_t** out, int64_t* bad_record) {
  g_err.clear();
  if (out) *out = nullptr;
  if (bad_record) *bad_record = -1;
  if (!in_path || !src_tag || !dst_tag || !out) return fail(SCT_BAM_EIO, "NULL argument");
  if (strlen(src_tag) != 2 || strlen(dst_tag) != 2) return fail(SCT_BAM_VALUEERROR, "tags are two-character names");
  if (L < 0) return fail(SCT_BAM_VALUEERROR, "negative value length");
  if (n_threads <= 0) n_threads = omp_get_max_threads();
  std::unique_ptr<sct_bam_tags> h(new sct_bam_tags);
  h->L = L;
  int rc = inflate_file(in_path, h->data, n_threads);
  if (rc) return rc;
  const uint8_t* d = h->data.data();
  const size_t len = h->data.size();
  if (len < 12 || memcmp(d, "BAM\1", 4) != 0) return fail(SCT_BAM_EFORMAT, "%s is not a BAM file", in_path);
  size_t off = 8 + (size_t)rd32(d + 4);
  if (off + 4 > len) return fail(SCT_BAM_EFORMAT, "truncated BAM header in %s", in_path);
  const uint32_t n_ref = rd32(d + off);
  off += 4;
  for (uint32_t r = 0; r < n_ref; r++) {
    if (off + 4 > len) return fail(SCT_BAM_EFORMAT, "truncated BAM header in %s", in_path);
    off += 4 + (size_t)rd32(d + off) + 4;
  }
  if (off > len) return fail(SCT_BAM_EFORMAT, "truncated BAM header in %s", in_path);
  h->header.assign((const char*)d, off);
  while (off + 4 <= len) {
    const uint32_t bs = rd32(d + off);
    if (off + 4 + bs > len) break;
    h->starts.push_back(off);
    off += 4 + (size_t)bs;
  }
  if (off != len) return fail(SCT_BAM_EFORMAT, "truncated BAM record at the end of %s", in_path);
  const int64_t n = (int64_t)h->starts.size();
  h->dst_off.assign(n, 0), h->dst_len.assign(n, 0), h->src_off.assign(n, 0), h->src_len.assign(n, 0);
  h->values.assign((size_t)n * L, 0);
  h->fits.assign(n, 0);
  // per record: the first source tag (get_tag) and the first destination tag (the one set_tag replaces)
  int64_t first_bad = INT64_MAX, first_missing = INT64_MAX, first_typed = INT64_MAX;
#pragma omp parallel for num_threads(n_threads) schedule(static) reduction(min : first_bad, first_missing, first_typed)
  for (int64_t i = 0; i < n; i++) {
    const uint8_t* rec = d + h->starts[i];
    const uint32_t bs = rd32(rec);
    const uint8_t* b = rec + 4;
    uint64_t p = 32;
    if (bs >= 32) p += (uint64_t)b[8] + 4ull * rd16(b + 12) + ((uint64_t)rd32(b + 16) + 1) / 2 + rd32(b + 16);
    if (bs < 32 || p > bs) {
      first_bad = std::min(first_bad, i);
      continue;
    }
    const uint8_t* end = b + bs;
    const uint8_t* q = b + p;
    bool have_src = false, have_dst = false, ok = true;
    while (q + 3 <= end) {
      const char t = (char)q[2];
      TagVal v;
      const size_t w = read_tag(q + 3, end, t, &v);
      if (!w) {
        ok = false;
        break;
      }
      if (!have_src && q[0] == (uint8_t)src_tag[0] && q[1] == (uint8_t)src_tag[1]) {
        have_src = true;
        if (!v.is_str) {
          first_typed = std::min(first_typed, i);
        } else {
          h->src_off[i] = (uint32_t)((const uint8_t*)v.s - rec);
          h->src_len[i] = (uint32_t)v.n;
          if ((int64_t)v.n == L) {
            h->fits[i] = 1;
            memcpy(h->values.data() + (size_t)i * L, v.s, L);
          }
        }
      }
      if (!have_dst && q[0] == (uint8_t)dst_tag[0] && q[1] == (uint8_t)dst_tag[1]) {
        have_dst = true;
        h->dst_off[i] = (uint32_t)(q - rec);
        h->dst_len[i] = (uint32_t)(3 + w);
      }
      q += 3 + w;
    }
    if (!ok || q != end) first_bad = std::min(first_bad, i);
    else if (!have_src) first_missing = std::min(first_missing, i);
  }
  // the first offending record in file order decides
  const int64_t first = std::min(first_bad, std::min(first_missing, first_typed));
  if (first != INT64_MAX) {
    if (bad_record) *bad_record = first;
    if (first == first_bad) return fail(SCT_BAM_EFORMAT, "malformed BAM record %lld in %s", (long long)first, in_path);
    if (first == first_missing) return fail(SCT_BAM_KEYERROR, "tag '%s' not present", src_tag);
    return fail(SCT_BAM_ETYPED, "tag '%s' of record %lld is not a string", src_tag, (long long)first);
  }
  h->other_off.push_back(0);
  for (int64_t i = 0; i < n; i++)
    if (!h->fits[i]) {
      h->other_rec.push_back(i);
      h->other_bytes.append((const char*)d + h->starts[i] + h->src_off[i], h->src_len[i]);
      h->other_off.push_back((int64_t)h->other_bytes.size());
    }
  *out = h.release();
  return SCT_BAM_OK;
}

int64_t sct_bam_tag_n(const sct_bam_tags_t* h) { return h ? (int64_t)h->starts.size() : 0; }

const uint8_t* sct_bam_tag_values(const sct_bam_tags_t* h) { return h ? h->values.data() : nullptr; }

int sct_bam_tag_others(const sct_bam_tags_t* h, int64_t* n, const int64_t** records, const char** bytes,
                       const int64_t** offsets) {
  g_err.clear();
  if (!h || !n || !records || !bytes || !offsets) return fail(SCT_BAM_EIO, "NULL argument");
  *n = (int64_t)h->other_rec.size();
  *records = h->other_rec.data();
  *bytes = h->other_bytes.data();
  *offsets = h->other_off.data();
  return SCT_BAM_OK;
}

int sct_bam_tag_write(const sct_bam_tags_t* h, const char* out_path, const char* dst_tag, const uint8_t* values,
                      const char* other_bytes, const int64_t* other_offsets, int32_t level, int32_t n_threads) {
  g_err.clear();
  if (!h || !out_path || !dst_tag) return fail(SCT_BAM_EIO, "NULL argument");
  if (strlen(dst_tag) != 2) return fail(SCT_BAM_VALUEERROR, "tags are two-character names");
  if (level < 0 || level > 9) return fail(SCT_BAM_EIO, "compression level %d outside 0..9", level);
  if (n_threads <= 0) n_threads = omp_get_max_threads();
  const int64_t n = (int64_t)h->starts.size();
  const int32_t L = h->L;
  if (n > 0 && L > 0 && !values) return fail(SCT_BAM_EIO, "NULL values");
  const bool own_others = !other_bytes || !other_offsets;  // the records' own values pass through
  const char* ob = own_others ? h->other_bytes.data() : other_bytes;
  const int64_t* oo = own_others ? h->other_off.data() : other_offsets;
  // the value of record i: (pointer, bytes)
  std::vector<int64_t> other_at(n, -1);
  for (size_t k = 0; k < h->other_rec.size(); k++) other_at[h->other_rec[k]] = (int64_t)k;
  for (size_t k = 0; k < h->other_rec.size(); k++)
    if (oo[k + 1] < oo[k] || memchr(ob + oo[k], 0, (size_t)(oo[k + 1] - oo[k])))
      return fail(SCT_BAM_VALUEERROR, "a tag value holds a NUL byte or its offsets run backwards");
  const uint8_t* d = h->data.data();
  const int T = n_threads;
  std::vector<uint64_t> part(T + 1, 0);
  auto value_len = [&](int64_t i) -> uint64_t {
    return h->fits[i] ? (uint64_t)L : (uint64_t)(oo[other_at[i] + 1] - oo[other_at[i]]);
  };
  int bad = 0;
#pragma omp parallel num_threads(T) reduction(| : bad)
  {
    const int t = omp_get_thread_num();
    const int64_t lo = n * t / T, hi = n * (t + 1) / T;
    uint64_t sz = 0;
    for (int64_t i = lo; i < hi; i++) {
      if (h->fits[i] && memchr(values + (size_t)i * L, 0, L)) bad = 1;
      sz += 4 + (uint64_t)rd32(d + h->starts[i]) - h->dst_len[i] + 3 + value_len(i) + 1;
    }
    part[t + 1] = sz;
  }
  if (bad) return fail(SCT_BAM_VALUEERROR, "a tag value holds a NUL byte");
  for (int t = 0; t < T; t++) part[t + 1] += part[t];
  std::vector<uint8_t> out(part[T]);
#pragma omp parallel num_threads(T)
  {
    const int t = omp_get_thread_num();
    const int64_t lo = n * t / T, hi = n * (t + 1) / T;
    uint8_t* o = out.data() + part[t];
    for (int64_t i = lo; i < hi; i++) {
      const uint8_t* rec = d + h->starts[i];
      const uint32_t bs = rd32(rec);
      const uint64_t vl = value_len(i);
      const uint32_t nbs = (uint32_t)(bs - h->dst_len[i] + 3 + vl + 1);
      memcpy(o, &nbs, 4);
      o += 4;
      if (h->dst_len[i]) {  // cut the old tag out
        const uint32_t a = h->dst_off[i], b = a + h->dst_len[i];
        memcpy(o, rec + 4, a - 4);
        o += a - 4;
        memcpy(o, rec + b, 4 + bs - b);
        o += 4 + bs - b;
      } else {
        memcpy(o, rec + 4, bs);
        o += bs;
      }
      *o++ = (uint8_t)dst_tag[0];
      *o++ = (uint8_t)dst_tag[1];
      *o++ = 'Z';
      memcpy(o, h->fits[i] ? (const void*)(values + (size_t)i * L) : (const void*)(ob + oo[other_at[i]]), vl);
      o += vl;
      *o++ = 0;
    }
  }
  return write_bam_file(out_path, h->header, out.data(), out.size(), level, n_threads);
}

void sct_bam_tag_close(sct_bam_tags_t* h) { delete h; }

// ---- bam.Tagger.tag (bam.py:208-233): string tags attached from columns, a window at a time ----

int sct_bam_attach_open(const char* in_path, const char* out_path, int32_t level, int32_t n_threads,
                        sct_bam_attach_t** out) {
  g_err.clear();
  if (out) *out = nullptr;
  if (!in_path || !out_path || !out) return fail(SCT_BAM_EIO, "NULL argument");
  if (level < 0 || level > 9) return fail(SCT_BAM_EIO, "compression level %d outside 0..9", level);
  if (n_threads <= 0) n_threads = omp_get_max_threads();
  std::unique_ptr<sct_bam_attach> h(new sct_bam_attach);
  h->n_threads = n_threads;
  int rc = inflate_file(in_path, h->data, n_threads);
  if (rc) return rc;
  const uint8_t* d = h->data.data();
  const size_t len = h->data.size();
  if (len < 12 || memcmp(d, "BAM\1", 4) != 0) return fail(SCT_BAM_EFORMAT, "%s is not a BAM file", in_path);
  size_t off = 8 + (size_t)rd32(d + 4);
  if (off + 4 > len) return fail(SCT_BAM_EFORMAT, "truncated BAM header in %s", in_path);
  const uint32_t n_ref = rd32(d + off);
  off += 4;
  for (uint32_t r = 0; r < n_ref; r++) {
    if (off + 4 > len) return fail(SCT_BAM_EFORMAT, "truncated BAM header in %s", in_path);
    off += 4 + (size_t)rd32(d + off) + 4;
  }
  if (off > len) return fail(SCT_BAM_EFORMAT, "truncated BAM header in %s", in_path);
  const std::string header((const char*)d, off);
  while (off + 4 <= len) {
    const uint32_t bs = rd32(d + off);
    if (off + 4 + bs > len) break;
    h->starts.push_back(off);
    off += 4 + (size_t)bs;
  }
  if (off != len) return fail(SCT_BAM_EFORMAT, "truncated BAM record at the end of %s", in_path);
  rc = h->writer.open(out_path, header, level, n_threads);
  if (rc) return rc;
  *out = h.release();
  return SCT_BAM_OK;
}

int64_t sct_bam_attach_n(const sct_bam_attach_t* h) { return h ? (int64_t)h->starts.size() : 0; }

int sct_bam_attach_write(sct_bam_attach_t* h, int64_t n, int32_t n_tags, const char* tag_names,
                         const uint8_t* const* values, const int64_t* strides, const int32_t* const* lengths,
                         int64_t* n_written) {
  g_err.clear();
  if (n_written) *n_written = 0;
  if (!h || n < 0 || n_tags < 0) return fail(SCT_BAM_EIO, "NULL handle or negative count");
  if (n_tags > 0 && (!tag_names || !values || !strides || strlen(tag_names) != 2 * (size_t)n_tags))
    return fail(SCT_BAM_VALUEERROR, "tags are %d two-character names", n_tags);
  const int64_t first = h->next;
  const int64_t m = std::min<int64_t>(n, (int64_t)h->starts.size() - first);
  for (int32_t t = 0; t < n_tags; t++) {
    if (strides[t] < 0 || (m > 0 && strides[t] > 0 && !values[t])) return fail(SCT_BAM_EIO, "NULL values of tag %d", t);
  }
  const uint8_t* d = h->data.data();
  const int T = h->n_threads;
  std::vector<std::vector<uint8_t>> part(T);
  int bad = 0;  // 1 malformed record, 2 NUL byte, 4 length outside -1..stride
  // a loop over the T parts: every part is built whatever number of threads the runtime grants
#pragma omp parallel for num_threads(T) schedule(static, 1) reduction(| : bad)
  for (int tn = 0; tn < T; tn++) {
    const int64_t lo = m * tn / T, hi = m * (tn + 1) / T;
    std::vector<uint8_t>& o = part[tn];
    std::vector<uint8_t> aux;
    for (int64_t i = lo; i < hi; i++) {
      const uint8_t* rec = d + h->starts[first + i];
      const uint32_t bs = rd32(rec);
      const uint8_t* b = rec + 4;
      uint64_t p = 32;
      if (bs >= 32) p += (uint64_t)b[8] + 4ull * rd16(b + 12) + ((uint64_t)rd32(b + 16) + 1) / 2 + rd32(b + 16);
      if (bs < 32 || p > bs) {
        bad |= 1;
        continue;
      }
      aux.assign(b + p, b + bs);
      for (int32_t t = 0; t < n_tags; t++) {
        const int64_t vl = lengths && lengths[t] ? (int64_t)lengths[t][i] : strides[t];
        if (vl == -1) continue;  // record i does not get tag t
        if (vl < 0 || vl > strides[t]) {
          bad |= 4;
          continue;
        }
        const uint8_t* v = values[t] + (size_t)i * strides[t];
        if (vl && memchr(v, 0, (size_t)vl)) bad |= 2;
        // set_tag: the first occurrence is cut out, the new value goes last
        size_t q = 0;
        while (q + 3 <= aux.size()) {
          const size_t w = read_tag(aux.data() + q + 3, aux.data() + aux.size(), (char)aux[q + 2], nullptr);
          if (!w) {
            bad |= 1;
            break;
          }
          if (aux[q] == (uint8_t)tag_names[2 * t] && aux[q + 1] == (uint8_t)tag_names[2 * t + 1]) {
            aux.erase(aux.begin() + (ptrdiff_t)q, aux.begin() + (ptrdiff_t)(q + 3 + w));
            break;
          }
          q += 3 + w;
        }
        aux.push_back((uint8_t)tag_names[2 * t]);
        aux.push_back((uint8_t)tag_names[2 * t + 1]);
        aux.push_back('Z');
        aux.insert(aux.end(), v, v + vl);
        aux.push_back(0);
      }
      const uint32_t nbs = (uint32_t)(p + aux.size());
      const uint8_t* nb = (const uint8_t*)&nbs;
      o.insert(o.end(), nb, nb + 4);
      o.insert(o.end(), b, b + p);
      o.insert(o.end(), aux.begin(), aux.end());
    }
  }
  if (bad & 1) return fail(SCT_BAM_EFORMAT, "malformed BAM record among records %lld..%lld", (long long)first, (long long)(first + m));
  if (bad & 4) return fail(SCT_BAM_VALUEERROR, "a tag length is outside -1..stride");
  if (bad & 2) return fail(SCT_BAM_VALUEERROR, "a tag value holds a NUL byte");
  std::vector<uint8_t>& pending = h->writer.pending();
  for (int tn = 0; tn < T; tn++) pending.insert(pending.end(), part[tn].begin(), part[tn].end());
  h->next += m;
  if (n_written) *n_written = m;
  return h->writer.flush_full();
}

int sct_bam_attach_close(sct_bam_attach_t* h) {
  g_err.clear();
  if (!h) return SCT_BAM_OK;
  const int rc = h->writer.finish();
  delete h;
  return rc;
}

}  // extern "C"
