// bamshards.cpp -- the shard writer of FastqProcess (include/sct_bam.h, sct_bam_shards_*): N output
// files that grow together.  Every append hands over one host buffer that holds the new bytes of
// all N files back to back (N + 1 bounds), as the device partition leaves them; each file's bytes
// go to its BamStreamWriter (bamwrite.h), which deflates every full 0xff00-byte member in parallel
// and keeps the rest for the next call.  The writers of a handle share one pool of deflate states
// (one per thread), so 1024 shards cost no more memory than one.  A file with a header is a BAM
// (magic, the SAM text, no references); a file without one holds the appended bytes alone -- the
// fastq.gz shards: a BGZF file is a valid multi-member gzip.
//
// If anything fails, every file the run created is removed: on a failed open or append the handle
// is left in a state where only close/abort is valid, and both then remove the files.
#include <omp.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/sct_bam.h"
#include "bamwrite.h"
#include "bgzf.h"

struct sct_bam_shards {
  std::vector<std::string> paths;
  std::vector<z_stream> pool;  // n_threads deflate states that the writers share: they deflate one after the other
  std::vector<std::unique_ptr<BamStreamWriter>> writers;  // one per created file
  bool failed = false;
  ~sct_bam_shards() {
    writers.clear();
    for (auto& z : pool) deflateEnd(&z);
  }
  void remove_all() {
    writers.clear();  // closes the files
    for (const auto& p : paths) remove(p.c_str());
    paths.clear();
  }
};

extern "C" {

int sct_bam_shards_open(const char* const* paths, const char* const* headers, int32_t n, int32_t level,
                        int32_t n_threads, sct_bam_shards_t** out) {
  g_err.clear();
  if (out) *out = nullptr;
  if (!paths || !out) return fail(SCT_BAM_EIO, "NULL argument");
  if (n < 1 || n > 65536) return fail(SCT_BAM_VALUEERROR, "%d output files: outside 1..65536", n);
  if (level < 0 || level > 9) return fail(SCT_BAM_EIO, "compression level %d outside 0..9", level);
  if (n_threads <= 0) n_threads = omp_get_max_threads();
  for (int32_t i = 0; i < n; i++)
    if (!paths[i]) return fail(SCT_BAM_EIO, "NULL path %d", i);
  std::unique_ptr<sct_bam_shards> h(new sct_bam_shards);
  h->pool.resize(n_threads);
  for (auto& z : h->pool) {
    memset(&z, 0, sizeof(z));
    deflateInit2(&z, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
  }
  for (int32_t i = 0; i < n; i++) {
    std::string header;
    if (headers && headers[i]) {
      const uint32_t l_text = (uint32_t)strlen(headers[i]), n_ref = 0;
      header.assign("BAM\1", 4);
      header.append((const char*)&l_text, 4);
      header.append(headers[i], l_text);
      header.append((const char*)&n_ref, 4);
    }
    std::unique_ptr<BamStreamWriter> w(new BamStreamWriter);
    const int rc = w->open(paths[i], header, level, n_threads, &h->pool);  // (removes its own file when it fails)
    if (rc) {
      const std::string why = g_err;
      h->remove_all();
      g_err = why;
      return rc;
    }
    h->paths.push_back(paths[i]);
    h->writers.push_back(std::move(w));
  }
  *out = h.release();
  return SCT_BAM_OK;
}

int sct_bam_shards_append(sct_bam_shards_t* h, const uint8_t* data, const int64_t* bounds) {
  g_err.clear();
  if (!h || !bounds) return fail(SCT_BAM_EIO, "NULL argument");
  if (h->failed) return fail(SCT_BAM_EIO, "an earlier call on these shards failed");
  const size_t n = h->writers.size();
  for (size_t i = 0; i < n; i++)
    if (bounds[i] < 0 || bounds[i + 1] < bounds[i]) return fail(SCT_BAM_VALUEERROR, "shard bounds run backwards at %zu", i);
  if (bounds[n] > bounds[0] && !data) return fail(SCT_BAM_EIO, "NULL data");
  for (size_t i = 0; i < n; i++) {
    if (bounds[i + 1] == bounds[i]) continue;
    std::vector<uint8_t>& pending = h->writers[i]->pending();
    pending.insert(pending.end(), data + bounds[i], data + bounds[i + 1]);
    const int rc = h->writers[i]->flush_full();
    if (rc) {
      const std::string why = g_err;
      h->failed = true;
      h->remove_all();
      g_err = why;
      return rc;
    }
  }
  return SCT_BAM_OK;
}

int sct_bam_shards_close(sct_bam_shards_t* h) {
  g_err.clear();
  if (!h) return SCT_BAM_OK;
  std::unique_ptr<sct_bam_shards> own(h);
  if (h->failed) return fail(SCT_BAM_EIO, "an earlier call on these shards failed");
  for (size_t i = 0; i < h->writers.size(); i++) {
    const int rc = h->writers[i]->finish();
    if (rc) {
      const std::string why = g_err;
      h->remove_all();
      g_err = why;
      return rc;
    }
  }
  return SCT_BAM_OK;
}

void sct_bam_shards_abort(sct_bam_shards_t* h) {
  if (!h) return;
  h->remove_all();
  delete h;
}

}  // extern "C"
