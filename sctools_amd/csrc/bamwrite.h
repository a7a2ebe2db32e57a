// bamwrite.h -- the BGZF writer path of libsct_bam.so's whole-file outputs (sct_bam_write_order,
// sct_bam_tag_write): the header in its own members, as htslib writes it, then the record bytes
// in 0xff00-byte members deflated in parallel, then the EOF member.  Host C++ (zlib, OpenMP).
#pragma once
#include <omp.h>

#include <algorithm>

#include "../../include/sct_bam.h"
#include "bgzf.h"

namespace {

inline int write_bam_file(const char* out_path, const std::string& header, const uint8_t* body, size_t body_bytes,
                          int level, int n_threads) {
  std::vector<z_stream> zs(n_threads);
  for (auto& z : zs) {
    memset(&z, 0, sizeof(z));
    deflateInit2(&z, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
  }
  struct ZEnd {
    std::vector<z_stream>& zs;
    ~ZEnd() {
      for (auto& z : zs) deflateEnd(&z);
    }
  } zend{zs};
  FILE* f = fopen(out_path, "wb");
  if (!f) return fail(SCT_BAM_EIO, "cannot create %s", out_path);
  struct Closer {
    FILE*& f;
    ~Closer() {
      if (f) fclose(f);
    }
  } closer{f};
  int bad = 0;
  for (int pass = 0; pass < 2; pass++) {
    const uint8_t* src = pass == 0 ? (const uint8_t*)header.data() : body;
    const size_t total = pass == 0 ? header.size() : body_bytes;
    const size_t np = (total + kBgzfMaxInput - 1) / kBgzfMaxInput;
    std::vector<std::vector<uint8_t>> z(np);
#pragma omp parallel for num_threads(n_threads) schedule(dynamic, 1) reduction(| : bad)
    for (long k = 0; k < (long)np; k++) {
      const size_t o = (size_t)k * kBgzfMaxInput;
      if (!bgzf_block(src + o, std::min(kBgzfMaxInput, total - o), level, zs[omp_get_thread_num()], z[k])) bad = 1;
    }
    if (bad) return fail(SCT_BAM_EIO, "deflate failed");
    for (size_t k = 0; k < np; k++)
      if (fwrite(z[k].data(), 1, z[k].size(), f) != z[k].size()) return fail(SCT_BAM_EIO, "cannot write %s", out_path);
  }
  if (fwrite(kBgzfEof, 1, sizeof(kBgzfEof), f) != sizeof(kBgzfEof)) return fail(SCT_BAM_EIO, "cannot write %s", out_path);
  FILE* g = f;
  f = nullptr;
  if (fclose(g) != 0) return fail(SCT_BAM_EIO, "cannot close %s", out_path);
  return SCT_BAM_OK;
}

// The same layout written piece by piece (sct_bam_attach_*): open() writes the header members,
// append() takes record bytes and writes every full 0xff00-byte member (deflated in parallel),
// keeping the rest for the next call, so the members do not depend on how the caller cut the
// stream; finish() writes the last partial member and the EOF member.
class BamStreamWriter {
 public:
  ~BamStreamWriter() {
    for (auto& z : own_) deflateEnd(&z);
    if (f_) fclose(f_);
  }
  // `shared`, when given, is a pool of at least n_threads raw-deflate states at `level` that outlives
  // the writer and that no other writer uses at the same time (sct_bam_shards_*: one pool per handle)
  int open(const char* out_path, const std::string& header, int level, int n_threads,
           std::vector<z_stream>* shared = nullptr) {
    path_ = out_path;
    level_ = level;
    n_threads_ = n_threads;
    if (shared) {
      zs_ = shared;
    } else {
      own_.resize(n_threads);
      for (auto& z : own_) {
        memset(&z, 0, sizeof(z));
        deflateInit2(&z, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
      }
      zs_ = &own_;
    }
    f_ = fopen(out_path, "wb");
    if (!f_) return fail(SCT_BAM_EIO, "cannot create %s", out_path);
    const int rc = write_members((const uint8_t*)header.data(), header.size());
    if (rc) {  // the file this call created is not left behind with part of a header
      fclose(f_);
      f_ = nullptr;
      remove(out_path);
    }
    return rc;
  }
  std::vector<uint8_t>& pending() { return pending_; }
  // writes the full members of pending()
  int flush_full() {
    const size_t full = pending_.size() / kBgzfMaxInput * kBgzfMaxInput;
    if (!full) return SCT_BAM_OK;
    const int rc = write_members(pending_.data(), full);
    pending_.erase(pending_.begin(), pending_.begin() + (ptrdiff_t)full);
    return rc;
  }
  int finish() {
    int rc = write_members(pending_.data(), pending_.size());
    pending_.clear();
    if (rc) return rc;
    if (fwrite(kBgzfEof, 1, sizeof(kBgzfEof), f_) != sizeof(kBgzfEof)) return fail(SCT_BAM_EIO, "cannot write %s", path_.c_str());
    FILE* g = f_;
    f_ = nullptr;
    if (fclose(g) != 0) return fail(SCT_BAM_EIO, "cannot close %s", path_.c_str());
    return SCT_BAM_OK;
  }

 private:
  int write_members(const uint8_t* src, size_t total) {
    const size_t np = (total + kBgzfMaxInput - 1) / kBgzfMaxInput;
    std::vector<std::vector<uint8_t>> z(np);
    int bad = 0;
#pragma omp parallel for num_threads(n_threads_) schedule(dynamic, 1) reduction(| : bad)
    for (long k = 0; k < (long)np; k++) {
      const size_t o = (size_t)k * kBgzfMaxInput;
      if (!bgzf_block(src + o, std::min(kBgzfMaxInput, total - o), level_, (*zs_)[omp_get_thread_num()], z[k])) bad = 1;
    }
    if (bad) return fail(SCT_BAM_EIO, "deflate failed");
    for (size_t k = 0; k < np; k++)
      if (fwrite(z[k].data(), 1, z[k].size(), f_) != z[k].size()) return fail(SCT_BAM_EIO, "cannot write %s", path_.c_str());
    return SCT_BAM_OK;
  }
  std::string path_;
  int level_ = 6, n_threads_ = 1;
  std::vector<z_stream> own_;
  std::vector<z_stream>* zs_ = nullptr;
  std::vector<uint8_t> pending_;
  FILE* f_ = nullptr;
};

}  // namespace
