// gbam_window.h -- the decode handle and its windows: what a window is (WinInfo), the handle every stage
// reads (struct sct_gbam, with the names of its timers), how a part's members are cut into windows
// (window_bytes, plan_windows), how one window's members reach the device and inflate there
// (inflate_window, inflate.h k_inflate), and the host's two reads of the mapped file before that
// (prefault, header_end).
#pragma once
#include <sys/mman.h>

#include <string>
#include <thread>
#include <vector>

#include "bgzf.h"
#include "gbam_util.h"
#include "inflate.h"

namespace gb {

// the members' inflate statuses folded into one mask (bit s: some member ended with status s)
__global__ void k_any(const uint32_t* __restrict__ st, uint32_t n, uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && st[i] != ST_OK) atomicOr(flag, 1u << (st[i] & 15));
}

}  // namespace gb

// One window: a range of BGZF members inflated together into U, after `carry` -- the bytes of the
// previous window from its last complete record on (that record, already parsed, gives the next
// record's query-name comparison in count mode; the rest is the record the window boundary cut).
// A file that fits the device is one window, inflated once (pass 1 keeps its payload and record
// starts for the parse); a larger one is inflated window by window twice: pass 1 (sct_gbam_open)
// proves every member's first record start and counts the records, pass 2 (sct_gbam_parse) inflates
// each window again, walks from the proven starts and parses -- the device holds one window's
// compressed bytes and payload, the columns and the dictionaries, never the whole file.
struct WinInfo {
  uint32_t m_lo = 0, m_hi = 0;  // members [m_lo, m_hi)
  uint32_t mH = 0;              // first walk member whose start is known (window 0: the header's member)
  uint64_t H = 0;               // that start (window 0: the header end; later windows: 0, the carry)
  uint64_t ulen = 0;            // carry + the members' payload
  bool has_prev = false;        // the carry begins with the previous window's last record
  bool last = false;            // the part's last window: no carry, records complete in U
  bool check = false;           // ... and the file's: its last record must end exactly at ulen
  uint32_t m_look = 0;          // members [m_hi, m_look) inflated after the window's own: a part's last
                                // window reads on into the next part for its records cut at the end
  uint64_t n_rec = 0;           // records this window parses (a carried record excluded)
  uint64_t base = 0;            // global index of its first parsed record
  std::vector<uint64_t> S;      // proven walk-member starts (pass 2 walks from them)
  std::string carry;            // the carry bytes (host copy)
};

struct sct_gbam {
  int device = 0;
  hipStream_t st = nullptr;
  int32_t part = 0, n_parts = 1;
  uint32_t pm_lo = 0, pm_hi = 0;  // the part's members
  int64_t first_abs = -1, land_abs = -1;  // payload offsets: its first record, the first record after it
  const uint8_t* f = nullptr;  // the mapped file (kept for pass 2)
  uint64_t fsize = 0;
  std::vector<Block> blocks;
  std::vector<uint64_t> O;  // payload offset of every member (n_mem + 1)
  std::vector<WinInfo> win;
  DevBuf<uint8_t> in, u;    // a window's compressed bytes and payload
  DevBuf<uint64_t> starts;  // one window: pass 1's record starts
  bool kept = false;        // one window: u and starts already hold the file
  uint64_t ulen = 0, H = 0;
  int64_t n = 0;
  std::string dict_bytes[3];
  std::vector<int64_t> dict_off[3];
  int32_t has_none[3] = {0, 0, 0};
  // sct_gbam_timing's eight entries, in the order of gbam.py STAGES: seconds, but for the last two
  enum Timer {
    T_MAP_SCAN, T_H2D, T_INFLATE, T_RECORD_STARTS, T_PARSE_INTERN, T_DICTIONARIES, T_MEMBERS, T_START_ROUNDS
  };
  double t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  ~sct_gbam() {
    if (f) munmap((void*)f, fsize);
  }
};

namespace {

// the byte offset where the alignments start: magic, l_text, text, n_ref, references
// (SAM/BAM spec 4.2); the leading members are inflated on the host until it is known.
// false: not a BAM header (the host path reports it).
bool header_end(const uint8_t* f, const std::vector<Block>& blocks, uint64_t* H) {
  std::vector<uint8_t> buf;
  z_stream z;
  memset(&z, 0, sizeof(z));
  if (inflateInit2(&z, -15) != Z_OK) return false;
  bool ok = false;
  for (size_t k = 0; k < blocks.size(); k++) {
    const size_t at = buf.size();
    buf.resize(at + blocks[k].isize);
    if (blocks[k].isize && !inflate_block(f, blocks[k], buf.data() + at, z)) break;
    const size_t len = buf.size();
    if (len < 12) continue;
    if (memcmp(buf.data(), "BAM\1", 4) != 0) break;
    uint64_t off = 8 + (uint64_t)rd32(buf.data() + 4);
    if (off + 4 > len) continue;
    const uint32_t n_ref = rd32(buf.data() + off);
    off += 4;
    bool done = true;
    for (uint32_t r = 0; r < n_ref && done; r++) {
      if (off + 4 > len) done = false;
      else off += 4 + (uint64_t)rd32(buf.data() + off) + 4;
    }
    if (!done || off > len) continue;
    *H = off;
    ok = true;
    break;
  }
  inflateEnd(&z);
  return ok;
}

// The mapping's page-table entries made in parallel (a large file in the page cache): the member
// scan (open_impl) and the copies to the device then run without a page fault every few members.
void prefault(const uint8_t* f, uint64_t fsize) {
  constexpr uint64_t kPage = 4096, kMin = 64ull << 20;
  if (fsize < kMin) return;
  const unsigned T = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::thread> th;
  std::atomic<uint64_t> sink{0};
  for (unsigned t = 0; t < T; t++)
    th.emplace_back([&, t] {
      const uint64_t lo = fsize * t / T / kPage * kPage, hi = fsize * (t + 1) / T;
      uint64_t acc = 0;
      for (uint64_t o = lo; o < hi; o += kPage) acc += ((const volatile uint8_t*)f)[o];
      sink += acc;
    });
  for (auto& x : th) x.join();
}

// Payload bytes per window: SCT_GBAM_WINDOW_BYTES, else a quarter of the device's free memory (the
// payload plus its compressed image then stay well inside it; a file under that is one window).
uint64_t window_bytes() {
  const char* v = getenv("SCT_GBAM_WINDOW_BYTES");
  if (v && *v) return std::max<uint64_t>(1, strtoull(v, nullptr, 10));
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr == 0) return 1ull << 30;
  return std::max<uint64_t>(64ull << 20, std::min<uint64_t>(fr / 4, 16ull << 30));
}

// Windows of whole members of the part [pm_lo, pm_hi), each at most `wb` payload bytes (at least
// one member); window 0 reaches at least one member past mH (the header's).  The last window of a
// part that is not the file's last reads on kLookahead payload bytes into the next part's members.
constexpr uint64_t kLookahead = 1u << 18;
void plan_windows(sct_gbam* G, uint32_t mH, uint64_t H, uint64_t wb) {
  const uint32_t n_mem = (uint32_t)G->blocks.size(), hi = G->pm_hi;
  G->win.clear();
  uint32_t m = G->pm_lo;
  while (m < hi) {
    WinInfo w;
    w.m_lo = m;
    uint64_t sz = 0;
    const uint32_t min_hi = G->win.empty() ? std::min(hi, G->pm_lo + mH + 2) : m + 1;
    while (m < hi && (m < min_hi || sz + G->blocks[m].isize <= wb)) sz += G->blocks[m++].isize;
    w.m_hi = w.m_look = m;
    G->win.push_back(std::move(w));
  }
  if (G->win.empty()) return;
  WinInfo& l = G->win.back();
  l.last = true;
  l.check = hi == n_mem;
  for (uint64_t sz = 0; l.m_look < n_mem && sz < kLookahead; l.m_look++) sz += G->blocks[l.m_look].isize;
  G->win[0].mH = mH;
  G->win[0].H = H;
}

// Inflate window w into G->u: the carry, then its members (copied in pieces on a copy stream while
// the members of the pieces already there inflate on st).  false: a member did not inflate (host).
int inflate_window(sct_gbam* G, WinInfo& w, bool timed) {
  hipStream_t st = G->st;
  const uint32_t nm = w.m_look - w.m_lo;  // the window's members and its lookahead
  const uint64_t c = w.carry.size();
  const uint64_t b0 = G->blocks[w.m_lo].off;
  const uint64_t b1 = w.m_look < G->blocks.size() ? G->blocks[w.m_look].off : G->fsize;
  w.ulen = c + (G->O[w.m_look] - G->O[w.m_lo]);
  double t1 = now();
  if (G->in.n < b1 - b0 + kPad) HIPOK(G->in.alloc(b1 - b0 + kPad));
  HIPOK(hipMemsetAsync(G->in.p + (b1 - b0), 0, kPad, st));
  if (G->u.n < w.ulen + kPad) HIPOK(G->u.alloc(w.ulen + kPad));
  HIPOK(hipMemsetAsync(G->u.p + w.ulen, 0, kPad, st));
  if (c) HIPOK(hipMemcpyAsync(G->u.p, w.carry.data(), c, hipMemcpyHostToDevice, st));
  std::vector<Member> mem(nm);
  for (uint32_t k = 0; k < nm; k++) {
    const Block& b = G->blocks[w.m_lo + k];
    const uint16_t xlen = rd16(G->f + b.off + 10);
    mem[k].in_off = b.off + 12 + xlen - b0;
    mem[k].clen = b.csize - 12 - xlen - 8;
    mem[k].isize = b.isize;
    mem[k].out_off = c + G->O[w.m_lo + k] - G->O[w.m_lo];
  }
  DevBuf<Member> d_mem;
  DevBuf<uint32_t> d_stat, d_flag;
  HIPOK(d_mem.alloc(nm));
  HIPOK(d_stat.alloc(nm));
  HIPOK(d_flag.alloc(1));
  HIPOK(hipMemcpyAsync(d_mem.p, mem.data(), nm * sizeof(Member), hipMemcpyHostToDevice, st));
  HIPOK(hipMemsetAsync(d_flag.p, 0, sizeof(uint32_t), st));
  CopyStream cs;
  HIPOK(cs.init(st));
  uint32_t m0 = 0;
  for (int k = 0; k < kCopyChunks && m0 < nm; k++) {
    // members [m0, m1): about 1 / kCopyChunks of the window each; a member's read-ahead past its own
    // bytes may see the next piece unwritten (never consumed: the stream ends inside the member)
    const uint64_t want = b0 + (b1 - b0) * (uint64_t)(k + 1) / kCopyChunks;
    uint32_t m1 = m0 + 1;
    while (m1 < nm && G->blocks[w.m_lo + m1].off < want) m1++;
    if (k == kCopyChunks - 1) m1 = nm;
    const uint64_t p0 = G->blocks[w.m_lo + m0].off - b0;
    const uint64_t p1 = (m1 < nm ? G->blocks[w.m_lo + m1].off : b1) - b0;
    HIPOK(hipMemcpyAsync(G->in.p + p0, G->f + b0 + p0, p1 - p0, hipMemcpyHostToDevice, cs.s));
    HIPOK(hipEventRecord(cs.ev[k], cs.s));
    HIPOK(hipStreamWaitEvent(st, cs.ev[k], 0));
    hipLaunchKernelGGL(k_inflate, dim3(m1 - m0), dim3(64), 0, st, G->in.p, d_mem.p + m0, G->u.p, d_stat.p + m0);
    HIPOK(hipGetLastError());
    m0 = m1;
  }
  if (timed) G->t[sct_gbam::T_H2D] += now() - t1;  // the copy (this thread waits for the pageable pieces)
  t1 = now();
  hipLaunchKernelGGL(k_any, dim3(grid(nm, 256)), dim3(256), 0, st, d_stat.p, nm, d_flag.p);
  uint32_t bad = 0;
  HIPOK(hipMemcpyAsync(&bad, d_flag.p, sizeof(bad), hipMemcpyDeviceToHost, st));
  HIPOK(hipStreamSynchronize(st));
  if (timed) G->t[sct_gbam::T_INFLATE] += now() - t1;  // the inflate left after the last piece arrived
  if (bad) {
    char msg[96];
    snprintf(msg, sizeof(msg), "a BGZF member did not inflate on the device (status mask 0x%x)", bad);
    return gfail(SCT_GBAM_HOST, msg);
  }
  return SCT_BAM_OK;
}

}  // namespace
