// gbam.hip -- BAM -> columnar decode on the device (include/sct_gbam.h): libsct_gbam.so.
//
//   1. host: map the file, hop the BGZF member headers (bgzf.h scan_blocks), inflate the first
//      member(s) with zlib only far enough to find where the header ends (H);
//   2. copy the compressed file to HBM once; k_inflate (inflate.h): one wave per member, every
//      payload lands at its prefix-sum offset in one contiguous buffer U;
//   3. record starts: k_guess picks, per member, the first offset from which four records chain
//      plausibly; k_walk follows block_size from each member's start to the first start in the
//      next member; a guess that disagrees with the previous member's landing is replaced by it
//      and the walk repeats (the member holding H starts exactly, so agreement everywhere proves
//      every start by induction); a second walk writes the record offsets;
//   4. k_parse: one lane per record -- the validation and fields of bamdec.cpp parse_record
//      (sct_bam.h), and CB / UB / GE interned in open-addressing tables (one 64-bit CAS per
//      insert: the string's offset in U, its length and 16 hash bits); k_parse_count: the
//      count-matrix mode (three named tags, XF, the query-name group head); k_parse_tagsort: the
//      native TagSort's per-read rule (bamdec.cpp parse_tagsort_record), the whole-read quality
//      sums taken by 16 lanes per record;
//   5. per dictionary the occupied slots are compacted, the distinct strings packed and copied to
//      the host, sorted there (Python's sorted() order, the missing tag first) and the rank of
//      every slot copied back; k_remap turns slot ids into ranks.
// Anything the device path does not reproduce exactly returns SCT_GBAM_HOST (the caller decodes
// with sct_bam_decode, whose first-offending-record error is the reference's exception).
//
// The stages live in headers of their own: gbam_util.h (errors, device buffers), gbam_window.h (the
// handle, windows, steps 1-2), gbam_starts.h (step 3), gbam_parse.h (step 4), gbam_dict.h (the tables of
// step 4 and step 5).  This file opens a part (open_impl) and holds the C entry points.
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <memory>
#include <string>
#include <string_view>
#include <vector>

#include "../../include/sct_bam.h"
#include "../../include/sct_gbam.h"
#include "bgzf.h"
#include "gbam_dict.h"
#include "gbam_parse.h"
#include "gbam_starts.h"
#include "gbam_util.h"
#include "gbam_window.h"

namespace {

// Part `part` of `n_parts`: the members from the first one starting at or after part/n_parts of the
// file's bytes to the next part's first (part 0 also takes the header's members).  Its records are
// those starting in its members' payload; the first one at first_start (a payload offset), or, when
// first_start < 0, where a start is guessed and proven from inside the part -- the caller checks it
// against the previous part's landing (sct_gbam_part_bounds) and reopens the part on a mismatch.
int open_impl(const char* path, int32_t part, int32_t n_parts, int64_t first_start, int32_t device, void* stream,
              sct_gbam_t** out, int64_t* n_records) {
  const double t0 = now();
  std::unique_ptr<sct_gbam> G(new sct_gbam());
  G->device = device;
  G->st = (hipStream_t)stream;
  G->part = part;
  G->n_parts = n_parts;
  HIPOK(hipSetDevice(device));
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return gfail(SCT_GBAM_HOST, "cannot open");
  struct stat sb;
  if (fstat(fd, &sb) != 0 || sb.st_size == 0) {
    close(fd);
    return gfail(SCT_GBAM_HOST, "empty file");
  }
  const uint64_t fsize = (uint64_t)sb.st_size;
  const uint8_t* f = (const uint8_t*)mmap(nullptr, fsize, PROT_READ, MAP_PRIVATE, fd, 0);
  close(fd);
  if (f == MAP_FAILED) return gfail(SCT_GBAM_HOST, "cannot map");
  G->f = f;
  G->fsize = fsize;
  prefault(f, fsize);
  std::vector<Block>& blocks = G->blocks;
  if (scan_blocks(f, fsize, blocks) != SCT_BAM_OK) return gfail(SCT_GBAM_HOST, "not BGZF");
  uint64_t H = 0;
  if (!header_end(f, blocks, &H)) return gfail(SCT_GBAM_HOST, "no BAM header");
  const uint32_t n_mem = (uint32_t)blocks.size();
  G->O.assign(n_mem + 1, 0);
  uint64_t ulen = 0;
  for (uint32_t k = 0; k < n_mem; k++) {
    const Block& b = blocks[k];
    const uint16_t xlen = rd16(f + b.off + 10);
    if (b.csize < 12u + xlen + 8u) return gfail(SCT_GBAM_HOST, "short member");
    if (b.isize > 65536) return gfail(SCT_GBAM_HOST, "member larger than 64 KB");
    G->O[k] = ulen;
    ulen += b.isize;
  }
  G->O[n_mem] = ulen;
  G->ulen = ulen;
  G->H = H;
  if (H >= ulen) return gfail(SCT_GBAM_HOST, "no records");  // the host path's empty-file error
  uint32_t mH = 0;
  while (mH + 1 < n_mem && G->O[mH + 1] <= H) mH++;
  // the part's members (byte-balanced; part 0 keeps the header's)
  auto cut = [&](int32_t p) -> uint32_t {
    if (p <= 0) return 0;
    if (p >= n_parts) return n_mem;
    const uint64_t want = fsize * (uint64_t)p / (uint64_t)n_parts;
    uint32_t m = (uint32_t)(std::lower_bound(blocks.begin(), blocks.end(), want,
                                             [](const Block& b, uint64_t v) { return b.off < v; }) -
                            blocks.begin());
    return std::max<uint32_t>(m, std::min<uint32_t>(n_mem, mH + 1));
  };
  G->pm_lo = cut(part);
  G->pm_hi = std::max(G->pm_lo, cut(part + 1));
  if (G->pm_lo == G->pm_hi) {
    // an empty part (more parts than members, or a header longer than the part's share): no
    // records, and transparent to the landing chain -- it starts and lands where it is told to
    // (the previous part's landing may lie past its member boundary), else at that boundary
    G->first_abs = G->land_abs = first_start >= 0 ? first_start : (int64_t)G->O[G->pm_lo];
    G->t[sct_gbam::T_MAP_SCAN] = now() - t0;
    *n_records = 0;
    *out = G.release();
    return SCT_BAM_OK;
  }
  uint32_t wmH = 0;
  uint64_t wH = kUnknown;
  if (part == 0) {
    wmH = mH;
    wH = H;
  } else if (first_start >= 0) {
    if ((uint64_t)first_start < G->O[G->pm_lo] || (uint64_t)first_start > G->O[G->pm_hi])
      return gfail(SCT_BAM_EIO, "first_start outside the part");
    wH = (uint64_t)first_start - G->O[G->pm_lo];
  }
  plan_windows(G.get(), wmH, wH, window_bytes());
  G->t[sct_gbam::T_MAP_SCAN] = now() - t0;
  G->t[sct_gbam::T_MEMBERS] = G->pm_hi - G->pm_lo;

  // pass 1: every window inflated, its member starts proven, its records counted
  const bool one = G->win.size() == 1;
  uint64_t n = 0;
  for (size_t k = 0; k < G->win.size(); k++) {
    WinInfo& w = G->win[k];
    int rc = inflate_window(G.get(), w, true);
    if (rc) return rc;
    const double t1 = now();
    rc = prove_window(G.get(), w, k + 1 < G->win.size() ? &G->win[k + 1] : nullptr, one ? &G->starts : nullptr);
    if (rc) return rc;
    w.base = n;
    n += w.n_rec;
    G->t[sct_gbam::T_RECORD_STARTS] += now() - t1;
  }
  G->kept = one;
  if (one) G->in.free();
  if (n == 0 && n_parts == 1) return gfail(SCT_GBAM_HOST, "no records");
  G->n = (int64_t)n;
  *n_records = (int64_t)n;
  *out = G.release();
  return SCT_BAM_OK;
}

}  // namespace

extern "C" {

const char* sct_gbam_last_error(void) { return g_gerr.c_str(); }

int sct_gbam_open(const char* path, int32_t device, void* stream, sct_gbam_t** out, int64_t* n_records) {
  return sct_gbam_open_part(path, 0, 1, -1, device, stream, out, n_records);
}

int sct_gbam_open_part(const char* path, int32_t part, int32_t n_parts, int64_t first_start, int32_t device,
                       void* stream, sct_gbam_t** out, int64_t* n_records) {
  g_gerr.clear();
  if (out) *out = nullptr;
  if (n_records) *n_records = 0;
  if (!path || !out || !n_records) return gfail(SCT_BAM_EIO, "NULL argument");
  if (n_parts < 1 || part < 0 || part >= n_parts) return gfail(SCT_BAM_EIO, "part outside [0, n_parts)");
  DeviceGuard guard;
  return open_impl(path, part, n_parts, first_start, device, stream, out, n_records);
}

int sct_gbam_part_bounds(const sct_gbam_t* h, int64_t* first_start, int64_t* end_landing) {
  if (!h || !first_start || !end_landing) return gfail(SCT_BAM_EIO, "NULL argument");
  *first_start = h->first_abs;
  *end_landing = h->land_abs;
  return SCT_BAM_OK;
}

// The parts' ranked dictionaries `which` merged (sorted union, the missing tag first if any part
// has it): parts[0] then holds the merged one, remap[p][i] = the merged id of part p's id i.
int sct_gbam_merge_dictionaries(sct_gbam_t* const* parts, int32_t n_parts, int32_t which, int32_t* const* remap) {
  if (!parts || n_parts < 1 || which < 0 || which > 2 || !remap) return gfail(SCT_BAM_EIO, "bad arguments");
  for (int32_t p = 0; p < n_parts; p++)
    if (!parts[p] || !remap[p]) return gfail(SCT_BAM_EIO, "NULL part or remap");
  int32_t hn = 0;
  for (int32_t p = 0; p < n_parts; p++) hn |= parts[p]->has_none[which];
  using SV = std::string_view;
  struct Cur {
    int32_t p;
    int64_t i, n;
  };
  auto name = [&](int32_t p, int64_t i) {
    const sct_gbam* h = parts[p];
    const std::vector<int64_t>& o = h->dict_off[which];
    return SV(h->dict_bytes[which].data() + o[i], (size_t)(o[i + 1] - o[i]));
  };
  std::vector<Cur> cur;
  for (int32_t p = 0; p < n_parts; p++) {
    const sct_gbam* h = parts[p];
    const int64_t n = h->dict_off[which].empty() ? 0 : (int64_t)h->dict_off[which].size() - 1;
    int64_t i = 0;
    if (h->has_none[which] && n > 0) remap[p][i++] = 0;  // the missing tag: merged id 0
    cur.push_back(Cur{p, i, n});
  }
  std::string bytes;
  std::vector<int64_t> off{0};
  if (hn) off.push_back(0);
  // k-way merge (the parts' lists are sorted and duplicate-free)
  auto greater = [&](const Cur& a, const Cur& b) { return name(b.p, b.i) < name(a.p, a.i); };
  std::vector<Cur> heap;
  for (const Cur& c : cur)
    if (c.i < c.n) heap.push_back(c);
  std::make_heap(heap.begin(), heap.end(), greater);
  int32_t id = hn ? 0 : -1;
  std::string last;
  bool have = false;
  while (!heap.empty()) {
    std::pop_heap(heap.begin(), heap.end(), greater);
    Cur c = heap.back();
    heap.pop_back();
    const SV v = name(c.p, c.i);
    if (!have || v != SV(last)) {
      bytes.append(v.data(), v.size());
      off.push_back((int64_t)bytes.size());
      last.assign(v.data(), v.size());
      have = true;
      id++;
    }
    remap[c.p][c.i] = id;
    if (++c.i < c.n) {
      heap.push_back(c);
      std::push_heap(heap.begin(), heap.end(), greater);
    }
  }
  parts[0]->dict_bytes[which] = std::move(bytes);
  parts[0]->dict_off[which] = std::move(off);
  parts[0]->has_none[which] = hn;
  return SCT_BAM_OK;
}

// column[i] = remap[column[i]] on the part's device and stream (n_ids entries of host `remap`).
int sct_gbam_remap(sct_gbam_t* h, const int32_t* remap, int64_t n_ids, void* column, int64_t n) {
  g_gerr.clear();
  if (!h || (!remap && n_ids) || (!column && n)) return gfail(SCT_BAM_EIO, "NULL argument");
  if (n == 0) return SCT_BAM_OK;
  DeviceGuard guard;
  HIPOK(hipSetDevice(h->device));
  DevBuf<int32_t> d;
  HIPOK(d.alloc((size_t)std::max<int64_t>(n_ids, 1)));
  if (n_ids) HIPOK(hipMemcpyAsync(d.p, remap, (size_t)n_ids * sizeof(int32_t), hipMemcpyHostToDevice, h->st));
  hipLaunchKernelGGL(k_apply_map, dim3(grid((uint64_t)n, 256)), dim3(256), 0, h->st, (int32_t*)column, (uint64_t)n,
                     (const int32_t*)d.p);
  HIPOK(hipGetLastError());
  HIPOK(hipStreamSynchronize(h->st));
  return SCT_BAM_OK;
}

int sct_gbam_parse(sct_gbam_t* h, int32_t metric_mode, void* const* columns) {
  g_gerr.clear();
  if (!h || !columns) return gfail(SCT_BAM_EIO, "NULL argument");
  if (metric_mode != SCT_BAM_CELL_METRICS && metric_mode != SCT_BAM_GENE_METRICS)
    return gfail(SCT_BAM_EIO, "the device decode reads the cell and gene metric modes");
  for (int k = 0; k < 14; k++)
    if (!columns[k]) return gfail(SCT_BAM_EIO, "NULL column");
  DeviceGuard guard;
  return parse_impl(h, metric_mode, columns);
}

int sct_gbam_parse_count(sct_gbam_t* h, const char* tags, void* const* columns) {
  g_gerr.clear();
  if (!h || !tags || !columns) return gfail(SCT_BAM_EIO, "NULL argument");
  for (int k = 0; k < 6; k++)
    if (!tags[k]) return gfail(SCT_BAM_EIO, "tags: six characters (cell, molecule, gene tag names)");
  for (int k = 0; k < 5; k++)
    if (!columns[k]) return gfail(SCT_BAM_EIO, "NULL column");
  DeviceGuard guard;
  return parse_count_impl(h, tags, columns);
}

int sct_gbam_parse_tagsort(sct_gbam_t* h, const char* tags, void* const* columns) {
  g_gerr.clear();
  if (!h || !tags || !columns) return gfail(SCT_BAM_EIO, "NULL argument");
  for (int k = 0; k < 6; k++)
    if (!tags[k]) return gfail(SCT_BAM_EIO, "tags: six characters (barcode, umi, gene tag names)");
  for (int k = 0; k < 14; k++)
    if (!columns[k]) return gfail(SCT_BAM_EIO, "NULL column");
  DeviceGuard guard;
  return parse_tagsort_impl(h, tags, columns);
}

int sct_gbam_dictionary(const sct_gbam_t* h, int32_t which, int64_t* n, const char** bytes, const int64_t** offsets,
                        int32_t* has_none) {
  if (!h || which < 0 || which > 2 || !n || !bytes || !offsets || !has_none) return gfail(SCT_BAM_EIO, "bad arguments");
  *n = h->dict_off[which].empty() ? 0 : (int64_t)h->dict_off[which].size() - 1;
  *bytes = h->dict_bytes[which].data();
  *offsets = h->dict_off[which].data();
  *has_none = h->has_none[which];
  return SCT_BAM_OK;
}

int sct_gbam_read_inflated(const sct_gbam_t* h, uint64_t off, uint64_t n, void* dst, uint64_t* total) {
  if (!h) return gfail(SCT_BAM_EIO, "NULL handle");
  if (total) *total = h->ulen;
  if (!n) return SCT_BAM_OK;
  if (!dst || off > h->ulen || n > h->ulen - off) return gfail(SCT_BAM_EIO, "range outside the payload");
  if (!h->kept) return gfail(SCT_BAM_EIO, "the payload is decoded window by window: not resident");
  DeviceGuard guard;
  HIPOK(hipSetDevice(h->device));
  HIPOK(hipMemcpy(dst, h->u.p + off, n, hipMemcpyDeviceToHost));
  return SCT_BAM_OK;
}

int sct_gbam_timing(const sct_gbam_t* h, double* t8) {
  if (!h || !t8) return gfail(SCT_BAM_EIO, "NULL argument");
  for (int k = 0; k < 8; k++) t8[k] = h->t[k];
  return SCT_BAM_OK;
}

int64_t sct_gbam_windows(const sct_gbam_t* h) { return h ? (int64_t)h->win.size() : 0; }

void sct_gbam_close(sct_gbam_t* h) {
  if (!h) return;
  DeviceGuard guard;
  (void)hipSetDevice(h->device);
  delete h;
}

}  // extern "C"
