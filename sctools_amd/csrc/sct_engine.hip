// sct_engine.hip -- MI355X (gfx950) per-cell / per-gene metric engine: host pipeline + C-ABI.
//
// Replaces the per-record Python loop of the reference
// (GatherCellMetrics / GatherGeneMetrics.extract_metrics, gatherer.py:116-232,
// driving MetricAggregator.parse_molecule, aggregator.py:236-334, and
// finalize, aggregator.py:342-387, 463-490, 571-578):
//
//   segment.h   entity runs (bam.iter_tag_groups, bam.py:492-540) and packed
//               64-bit keys [run | k1 | k2 | fragment hash], bits trimmed to the
//               dictionary sizes (cell: k1 = gene, k2 = umi; gene: k1 = cell)
//   bucket.h    distinct counts: per-entity MSD bucket partition of the keys
//               [k1 | k2 | fragment hash] until every bucket fits a tile, then an
//               LDS sort + neighbour pass per tile (the default path)
//   radix.h     device-wide LSD radix sort of (key, record index) -- the path for
//               keys too wide for bucket.h (k1 + k2 > 40 bits)
//   reduce.h    one pass over the globally sorted keys: Counter results from key runs
//   gene.h      gene buckets -> per-gene partial rows (LDS bins)
//   finalize.h  partial rows -> output rows; sequential Welford float path
//   tagsort.h   TagSortBam orders on the device; countmat.h  CountMatrix (CSR)
//   comm.h      RCCL all-reduce of gene partials (replaces MergeGeneMetrics, merge.py:74-191)
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared ... -lrccl.
// -ffp-contract=off keeps every Welford operation separately rounded, as Python does.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "comm.h"
#include "common.h"
#include "countmat.h"
#include "exchange.h"
#include "finalize.h"
#include "fixedpt.h"
#include "bucket.h"
#include "gene.h"
#include "radix.h"
#include "reduce.h"
#include "segment.h"
#include "streams.h"
#include "tagsort.h"
#include "tsmetrics.h"
#include "util.h"

using namespace sct;

namespace {

constexpr int64_t kEntHistMax = 1 << 18;  // entities whose first partition level is planned (k_level1_plan)

struct Layout {
  size_t tile_cnt, scalars, scan_sums, pay_a, pay_b, half, counts, offsets, ent_start, partials;
  size_t gcounts, gcursor, gtoff, gwork, dflags, gpay, seen, zero_mito, ent_hist, l1_toff, l1_tslot;
  size_t head_bits, bdesc, bent, seg_a, seg_b, work_a, work_b, seg_hist, seg_cur, giants, bigs, wctl, worder, wx, total;
  int64_t num_tiles, num_chunks, max_ent, max_gene_work, max_seg, max_work, count_cap;
  int n_buckets;
  bool gene;
};

Layout layout_for(const sct_plan_t* plan) {
  Layout L;
  const int64_t n = plan->n_records > 0 ? plan->n_records : 0;
  const int64_t n1 = n > 0 ? n : 1;
  L.num_tiles = cdiv(n1, kTile);
  const int64_t m = (int64_t)kRadix * cdiv(n1, kSortTile);  // radix counts of the global-sort path
  L.num_chunks = cdiv(m, kScanChunk);
  L.count_cap = m;
  L.max_ent = plan->max_entities > 0 ? plan->max_entities : n1;
  L.gene = plan->mode == SCT_MODE_GENE_GROUPED || (plan->flags & SCT_PLAN_GENE_PARTIALS);
  L.n_buckets = (int)cdiv(plan->n_gene_ids > 0 ? plan->n_gene_ids : 1, kGenesPerBucket);
  L.max_gene_work = L.n_buckets + cdiv(n1, kGeneChunk) + 1;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t o = off;
    off += align_up(bytes);
    return o;
  };
  // the prefix [0, scalars + 256) is all sct_count_entities touches
  L.tile_cnt = take(sizeof(uint64_t) * (size_t)(L.num_tiles + 1));
  L.scalars = take(256);
  L.scan_sums = take(sizeof(uint64_t) * (size_t)(L.num_chunks + 1));
  // the bucket path's 16-byte payloads (Pay), ping-pong A / B; the global-sort path splits each
  // into its keys (u64) and values (u32): A = [keys a | values a], B = [keys b | values b]
  L.half = align_up(sizeof(uint64_t) * (size_t)n1);
  L.pay_a = take(2 * L.half);
  L.pay_b = take(2 * L.half);
  L.counts = take(sizeof(uint32_t) * (size_t)m);
  L.offsets = take(sizeof(uint32_t) * (size_t)m);
  L.ent_start = take(sizeof(int64_t) * (size_t)(L.max_ent + 1));
  L.head_bits = take(sizeof(uint64_t) * (size_t)cdiv(n1, 64));  // one bit per record: run heads (k_heads)
  L.partials = take(sizeof(int64_t) * SCT_NP * (size_t)L.max_ent);
  L.gcounts = take(L.gene ? sizeof(uint32_t) * (size_t)L.n_buckets : 0);  // records per gene bucket
  L.gcursor = take(L.gene ? sizeof(uint32_t) * (size_t)L.n_buckets : 0);
  L.gtoff = take(L.gene ? sizeof(uint32_t) * (size_t)L.n_buckets * (size_t)cdiv(n1, kEmitTile) : 0);
  L.gwork = take(L.gene ? sizeof(int64_t) * 3 * (size_t)L.max_gene_work : 0);
  L.dflags = take(L.gene ? sizeof(uint16_t) * (size_t)n1 : 0);
  L.gpay = take(L.gene ? sizeof(GenePayload) * (size_t)n1 : 0);
  L.seen = take(L.gene ? sizeof(uint32_t) * (size_t)(plan->n_cell_ids > 0 ? plan->n_cell_ids : 1) : 0);
  L.zero_mito = take(L.gene ? (size_t)(plan->n_gene_ids > 0 ? plan->n_gene_ids : 1) : 0);
  // the planned first partition level (segment.h k_level1_plan): digit counts per entity (1 KB each;
  // larger plans run level 1 as the other levels), each key-pass tile's offsets and slots
  const bool l1 = L.max_ent <= kEntHistMax;
  L.ent_hist = take(l1 ? sizeof(uint32_t) * kRadix * (size_t)L.max_ent : 0);
  L.l1_toff = take(l1 ? sizeof(uint32_t) * kL1Slots * kRadix * (size_t)cdiv(n1, kKTile) : 0);
  L.l1_tslot = take(l1 ? sizeof(uint2) * (size_t)cdiv(n1, kKTile) : 0);
  // bucket.h: segments have > kBCap records and are disjoint within a level (and giants overall)
  L.max_seg = n1 / (kBCap + 1) + 2;
  L.max_work = n1 / kChunk + L.max_seg + 2;
  L.bdesc = take(sizeof(uint16_t) * (size_t)n1);
  L.bent = take(sizeof(uint32_t) * (size_t)n1);
  L.seg_a = take(sizeof(Seg) * (size_t)L.max_seg);
  L.seg_b = take(sizeof(Seg) * (size_t)L.max_seg);
  L.work_a = take(sizeof(Work) * (size_t)L.max_work);
  L.work_b = take(sizeof(Work) * (size_t)L.max_work);
  L.seg_hist = take(sizeof(uint32_t) * kRadix * (size_t)L.max_seg);
  L.seg_cur = take(sizeof(uint32_t) * kRadix * (size_t)L.max_seg);
  L.giants = take(sizeof(Seg) * (size_t)L.max_seg);
  L.bigs = take(sizeof(Seg) * (size_t)L.max_seg);
  const bool welford = plan->float_mode == SCT_FLOAT_WELFORD;
  L.wctl = take(welford ? 2 * sizeof(WelfordCtl) : 0);  // the main queue and the head group's
  L.worder = take(welford ? sizeof(uint32_t) * (size_t)L.max_ent : 0);
  L.wx = take(welford ? sizeof(double) * 4 * (size_t)(n1 + kWfPad) : 0);  // every record's stream values
  L.total = off;
  return L;
}

size_t count_bytes(const Layout& L) { return L.scalars + 256; }

BucketCtl* bucket_ctl(void* ws, const Layout& L) {
  return reinterpret_cast<BucketCtl*>(at<uint64_t>(ws, L.scalars) + 8);
}
// level 0's (n_seg, n_work) when the first partition level is planned before the key pass
uint32_t* level0_ctr(void* ws, const Layout& L) { return reinterpret_cast<uint32_t*>(at<uint64_t>(ws, L.scalars) + 12); }
static_assert(sizeof(BucketCtl) <= 32, "BucketCtl at scalars + 64 B ends before the level-0 counters at + 96 B");

int check_plan(const sct_plan_t* plan, const sct_records_t* rec) {
  if (!plan) return fail(SCT_EINVAL, "plan is NULL");
  if (plan->mode < SCT_MODE_CELL || plan->mode > SCT_MODE_GENE_GROUPED)
    return fail(SCT_EINVAL, "unknown mode %d", plan->mode);
  if (plan->float_mode != SCT_FLOAT_EXACT_SUM && plan->float_mode != SCT_FLOAT_WELFORD)
    return fail(SCT_EINVAL, "unknown float_mode %d", plan->float_mode);
  if (plan->float_mode == SCT_FLOAT_WELFORD && plan->mode == SCT_MODE_GENE_GROUPED)
    return fail(SCT_EINVAL, "SCT_FLOAT_WELFORD needs a RUN mode (record order defines Welford order)");
  if ((plan->flags & SCT_PLAN_GENE_PARTIALS) && plan->mode != SCT_MODE_CELL)
    return fail(SCT_EINVAL, "SCT_PLAN_GENE_PARTIALS needs SCT_MODE_CELL");
  if (plan->n_records < 0 || plan->n_records > (int64_t)0x7FFFFFFF)
    return fail(SCT_EINVAL, "n_records %lld out of range [0, 2^31)", (long long)plan->n_records);
  if ((plan->mode == SCT_MODE_GENE_GROUPED || (plan->flags & SCT_PLAN_GENE_PARTIALS)) &&
      plan->float_mode != SCT_FLOAT_EXACT_SUM)
    return fail(SCT_EINVAL, "grouped gene partials need SCT_FLOAT_EXACT_SUM");
  if (plan->n_cell_ids <= 0 || plan->n_gene_ids <= 0 || plan->n_umi_ids <= 0)
    return fail(SCT_EINVAL, "dictionary sizes must be positive");
  if (cdiv(plan->n_gene_ids, kGenesPerBucket) > kMaxGeneBuckets)
    return fail(SCT_EINVAL, "n_gene_ids %d exceeds %d", plan->n_gene_ids, kGenesPerBucket * kMaxGeneBuckets);
  if (rec) {
    if (rec->n != plan->n_records) return fail(SCT_EINVAL, "records.n != plan.n_records");
    if (rec->n > 0 && (!rec->cell || !rec->umi || !rec->gene || !rec->ref || !rec->pos || !rec->gq_sum ||
                       !rec->gq_len || !rec->gq_gt30 || !rec->bits || !rec->xf || !rec->cy_gt30 ||
                       !rec->cy_len || !rec->uy_gt30 || !rec->uy_len))
      return fail(SCT_EINVAL, "a record column pointer is NULL");
  }
  return SCT_OK;
}

// ---------------- the metric step ----------------
// Its switches (tests and experiments; DESIGN.md §16 lists what each turns off and the test that
// uses it), read once per call: the tests flip them between calls of one process.
bool env_is(const char* name, char v) {
  const char* x = getenv(name);
  return x && x[0] == v;
}
int env_int_in(const char* name, int lo, int hi) {  // 0 when unset or outside [lo, hi]
  const int v = getenv(name) ? atoi(getenv(name)) : 0;
  return v >= lo && v <= hi ? v : 0;
}
struct StepSwitches {  // (constructing one reads the environment)
  bool no_early_big = env_is("SCT_NO_EARLY_BIG", '1');
  bool no_level_big = env_is("SCT_NO_LEVEL_BIG", '1');
  bool big_beside_hash = env_is("SCT_BIG_BESIDE_HASH", '1');
  bool no_wf_gate = env_is("SCT_NO_WF_GATE", '1');
  bool no_l1_plan = env_is("SCT_NO_L1_PLAN", '1');
  bool force_global_sort = env_is("SCT_FORCE_GLOBAL_SORT", '1');
  bool no_prefill = env_is("SCT_NO_PREFILL", '1');
  bool no_side = env_is("SCT_NO_SIDE", '1');
  bool no_side_fin = env_is("SCT_NO_SIDE_FIN", '1');
  bool lanes_fused = getenv("SCT_STREAM_LANES") && !strcmp(getenv("SCT_STREAM_LANES"), "fused");  // else "pre"
  // 1..8: every entity's first level on that many bits, not the width its size asks for (8: rounds < 7)
  int l1_bits = env_int_in("SCT_L1_BITS", 1, kRadixBits);
};

// The views a kernel template is instantiated for: F(cell view, gene partials) over (true, true),
// (true, false), (false, false) -- gene runs never emit gene partials -- and F(cell view).
// Further arguments are passed on to F.
#define SCT_VIEW3(cell, gene, F, ...)                       \
  do {                                                      \
    if ((cell) && (gene)) { F(true, true, ##__VA_ARGS__); } \
    else if (cell) { F(true, false, ##__VA_ARGS__); }       \
    else { F(false, false, ##__VA_ARGS__); }                \
  } while (0)
#define SCT_VIEW2(cell, F) \
  do {                     \
    if (cell) { F(true); } \
    else { F(false); }     \
  } while (0)

// heads + scan of the entity column; with `dup_check`, also flags cell ids seen in two runs.
// Copies (n_entities, dup flag) to the host and synchronizes.
// pre: a fill queued behind the count's copy (round 6: it runs while the host waits for the count)
// publish (the pipeline: the workspace is a whole one, not sct_count_entities' prefix; round 7): the
// head bitmap and, queued behind the scan, the entity starts, also written while the host waits
struct CountOpts {
  bool dup_check = false, publish = false;
  int32_t n_ids = 0;
  FillBatch* pre = nullptr;
};
int count_runs(const int32_t* ent, int64_t n, void* ws, const Layout& L, const CountOpts& o, int64_t* n_ent,
               bool* dup, hipStream_t s) {
  const int64_t tiles = cdiv(n, kTile);
  uint64_t* tc = at<uint64_t>(ws, L.tile_cnt);
  uint64_t* sc = at<uint64_t>(ws, L.scalars);
  uint64_t* hb = o.publish ? at<uint64_t>(ws, L.head_bits) : nullptr;
  uint32_t* seen = o.dup_check ? at<uint32_t>(ws, L.seen) : nullptr;
  FillBatch fb;
  if (seen) fb.add(seen, sizeof(uint32_t) * (size_t)o.n_ids);
  fb.add(sc, 2 * sizeof(uint64_t));
  if (int rc = launch_fills(fb, s)) return rc;
  if (((uintptr_t)ent & 15) == 0) {
    LAUNCH_N("heads", n, k_heads4, dim3((unsigned)tiles), dim3(kBlock), s, ent, n, tc, seen, (uint32_t)o.n_ids, sc + 1, hb);
  } else {
    LAUNCH_N("heads", n, k_heads, dim3((unsigned)tiles), dim3(kBlock), s, ent, n, tc, seen, (uint32_t)o.n_ids, sc + 1, hb);
  }
  LAUNCH("scan", k_scan_wide, dim3(1), dim3(kScanWide), s, tc, tiles, sc);
  if (o.publish) {
    LAUNCH("ent_starts", k_ent_starts, dim3((unsigned)cdiv(tiles, kWaves)), dim3(kBlock), s, (const uint64_t*)hb,
           (const uint64_t*)tc, (const uint64_t*)sc, n, L.max_ent, at<int64_t>(ws, L.ent_start));
  }
  uint64_t host[2] = {0, 0};
  if (o.pre) {
    if (int rb = readback_start(sc, sizeof(host), s)) return rb;
    if (int rc = launch_fills(*o.pre, s)) return rc;
    if (int rb = readback_finish(host, sizeof(host))) return rb;
  } else {
    if (int rb = readback(host, sc, sizeof(host), s)) return rb;
  }
  *n_ent = (int64_t)host[0];
  if (dup) *dup = host[1] & 1;
  if (host[1] & 2) return fail(SCT_EINVAL, "an entity id lies outside [0, %d)", o.n_ids);
  return SCT_OK;
}

// Key bits (a pure host function).  Bucket path (default): [k1' | k2 | hash], KB <= kMaxKeyBits,
// entities implied by the record ranges.  Global-sort path: [run | k1' | k2 | hash], padded to whole
// radix digits.  *used: the bits before the hash.
int plan_key_bits(bool bucket, int64_t n_ent, Bits* b, int* used) {  // (b->k1, b->k2 are set)
  if (bucket) {
    b->e = 0;
    *used = b->k1 + b->k2;
    b->h = kMaxKeyBits - *used < 8 ? kMaxKeyBits - *used : 8;
  } else {
    b->e = bitlen((uint64_t)n_ent);
    *used = b->e + b->k1 + b->k2;
    if (*used > 63) return fail(SCT_EINVAL, "packed key needs %d bits (> 63)", *used);
    // fill the last radix digit with fragment-hash bits (same pass count), every shift < 64
    const int padded = ((*used + kRadixBits - 1) / kRadixBits) * kRadixBits;
    b->h = (padded > 63 ? 63 : padded) - *used;
    if (b->h > 32) b->h = 32;
  }
  if (b->k1 > 0) {  // spread neighbouring k1 ids over the top key digits (odd multiplier, bijective)
    b->mul = 0x9E3779B1u & b->k1_mask();
    b->mul |= 1u;
    uint32_t inv = b->mul;  // Newton: inverse mod 2^32, then mod 2^k1
    for (int it = 0; it < 5; it++) inv *= 2u - b->mul * inv;
    b->inv = inv & b->k1_mask();
  }
  return SCT_OK;
}

// One call of the RUN-mode pipeline (entity = runs of the cell column, or of the gene column in gene
// mode; GROUPED runs the cell view).  It writes partial rows into the workspace, output rows if
// out_i / out_f are set, and grouped gene partials (cell view) if gene_partials is set.
struct StepCall {
  const sct_plan_t* plan;
  const sct_records_t* rec;
  const uint8_t* gene_is_mito;
  void* ws;
  size_t ws_bytes;
  int64_t* out_i;
  double* out_f;
  int64_t capacity;
  int64_t* n_rows;
  int64_t* gene_partials;
  hipStream_t s;
};

// What the stages of one step share: the call, switches, streams, path flags and workspace pointers.
struct Step {
  const StepCall& c;
  const StepSwitches& sw;
  const Layout L;
  StepStreams st{c.s};
  void* const ws = c.ws;
  const hipStream_t s = c.s;
  const int64_t n = c.rec->n;
  int64_t n_ent = 0;
  const bool cell = c.plan->mode != SCT_MODE_GENE, gene = c.gene_partials != nullptr;
  const bool exact = c.plan->float_mode == SCT_FLOAT_EXACT_SUM;
  const bool streams = exact && c.out_i;  // exact mean / variance lanes of the output rows beside the keys
  // bucket: the bucket path, not the global sort.  plannable: its first partition level can be planned
  // before the key pass -- the digit comes from k1 alone (segment.h k_level1_plan), so the key pass
  // writes the level-1 children itself; planned: and there are entities.
  bool bucket, plannable, planned = false;
  bool use_side = false;  // the side stream of the planned bucket path with exact floats (round 6)
  bool split = false;     // the stream lanes in their own kernel on the pair's second stream (round 8)
  Bits b;
  int used = 0;
  const KeyCols kc{cell ? c.rec->gene : c.rec->cell, c.rec->umi,
                   (uint32_t)(cell ? c.plan->n_gene_ids : c.plan->n_cell_ids), (uint32_t)c.plan->n_umi_ids};
  const RecCols rc{c.rec->ref,  c.rec->pos,     c.rec->gq_sum, c.rec->gq_len,  c.rec->gq_gt30, c.rec->bits,
                   c.rec->xf,   c.rec->cy_gt30, c.rec->cy_len, c.rec->uy_gt30, c.rec->uy_len};
  // the bucket path's payloads are the global-sort path's keys and values (layout_for)
  const SortBuffers B{at<uint64_t>(ws, L.pay_a), at<uint64_t>(ws, L.pay_b), at<uint32_t>(ws, L.pay_a + L.half),
                      at<uint32_t>(ws, L.pay_b + L.half), at<uint32_t>(ws, L.counts), at<uint32_t>(ws, L.offsets),
                      at<uint64_t>(ws, L.scan_sums), L.count_cap};
  L1Plan l1{};
  const uint8_t* mito = c.gene_is_mito;
  hipEvent_t plan_done = nullptr, lanes_done = nullptr;
  // the workspace.  toff: the key-pass tiles' offsets (tile offsets are per kTile); hbits, ent_start:
  // run heads (one bit per record) and entity starts (+ the sentinel ent_start[n_ent] = n): count_runs
  const uint64_t *toff = at<uint64_t>(ws, L.tile_cnt), *hbits = at<uint64_t>(ws, L.head_bits);
  const int64_t* ent_start = at<int64_t>(ws, L.ent_start);
  int64_t* partials = at<int64_t>(ws, L.partials);
  uint32_t *gcounts = gene ? at<uint32_t>(ws, L.gcounts) : nullptr, *gtoff = gene ? at<uint32_t>(ws, L.gtoff) : nullptr;
  uint32_t* gcur = gene ? at<uint32_t>(ws, L.gcursor) : nullptr;
  int64_t *gwork = gene ? at<int64_t>(ws, L.gwork) : nullptr, *n_gwork = at<int64_t>(ws, L.scalars) + 4;
  uint16_t* dflags = gene ? at<uint16_t>(ws, L.dflags) : nullptr;
  // gene payload format: narrow (8 B) unless an operand does not fit (checked by the exact-stream
  // pass; without it the wide format is used)
  uint32_t* gwide = reinterpret_cast<uint32_t*>(at<uint64_t>(ws, L.scalars) + 16);
  BucketCtl* ctl = bucket_ctl(ws, L);
  uint32_t* ctr0 = level0_ctr(ws, L);
  Pay *pa = at<Pay>(ws, L.pay_a), *pb = at<Pay>(ws, L.pay_b);
  uint16_t* bdesc = at<uint16_t>(ws, L.bdesc);
  uint32_t* bent = at<uint32_t>(ws, L.bent);
  Seg* seg[2] = {at<Seg>(ws, L.seg_a), at<Seg>(ws, L.seg_b)};
  Work* work[2] = {at<Work>(ws, L.work_a), at<Work>(ws, L.work_b)};
  uint32_t *hist = at<uint32_t>(ws, L.seg_hist), *cur = at<uint32_t>(ws, L.seg_cur);
  Seg *giants = at<Seg>(ws, L.giants), *bigs = at<Seg>(ws, L.bigs);

  Step(const StepCall& call, const StepSwitches& w, const Layout& lay, bool allow_bucket) : c(call), sw(w), L(lay) {
    b.k1 = bitlen((uint64_t)kc.n_k1);
    b.k2 = bitlen((uint64_t)kc.n_k2);
    bucket = allow_bucket && b.k1 + b.k2 <= kMaxKeyBits && !sw.force_global_sort;
    plannable = bucket && L.max_ent <= kEntHistMax && b.k1 >= kRadixBits && !sw.no_l1_plan;
  }
};

// 1. entity runs.  The bucket descriptors (2 bytes per record, the step's largest fill) are zeroed
// while the host waits for the entity count, when the first partition level will be planned.
int count_stage(Step& S) {
  const StepCall& c = S.c;
  const bool prefill = S.plannable && !S.sw.no_prefill && S.n > 0;
  FillBatch pre;
  if (prefill) pre.add(S.bdesc, sizeof(uint16_t) * (size_t)S.n);
  bool dup = false;
  const CountOpts o{S.gene, true, c.plan->n_cell_ids, prefill ? &pre : nullptr};
  if (int rc = count_runs(S.cell ? c.rec->cell : c.rec->gene, S.n, c.ws, S.L, o, &S.n_ent, &dup, S.s)) return rc;
  if (dup) return fail(SCT_EINVAL, "grouped gene partials need cell-sorted records (a cell id forms two runs)");
  if (S.n_ent > S.L.max_ent)
    return fail(SCT_ENOMEM, "%lld entities exceed plan.max_entities %lld", (long long)S.n_ent, (long long)S.L.max_ent);
  if (c.out_i && S.n_ent > c.capacity)
    return fail(SCT_EINVAL, "%lld entities exceed output capacity %lld", (long long)S.n_ent, (long long)c.capacity);
  S.planned = S.plannable && S.n_ent > 0;
  S.use_side = S.planned && S.exact && !S.sw.no_side;
  // SCT_STREAM_LANES=fused keeps the lanes in the key pass, and so does a call that finds another
  // call's pair in use on the device (fork_lanes)
  S.split = S.use_side && S.streams && S.n > 0 && !S.sw.lanes_fused;
  if (S.planned)
    S.l1 = L1Plan{at<uint32_t>(S.ws, S.L.ent_hist), at<uint32_t>(S.ws, S.L.l1_toff), at<uint2>(S.ws, S.L.l1_tslot),
                  S.pb, S.sw.l1_bits};
  return SCT_OK;
}

// 3. every buffer the step zeroes before its first kernel, in one launch
int fills_stage(Step& S) {
  const sct_plan_t* plan = S.c.plan;
  FillBatch fb;
  if (S.cell && !S.mito) {
    uint8_t* z = at<uint8_t>(S.ws, S.L.zero_mito);
    fb.add(z, (size_t)plan->n_gene_ids);
    S.mito = z;
  }
  fb.add(S.partials, sizeof(int64_t) * SCT_NP * (size_t)S.n_ent);
  if (S.gene) {
    fb.add(S.gcounts, sizeof(uint32_t) * (size_t)S.L.n_buckets);
    fb.add(S.c.gene_partials, sizeof(int64_t) * SCT_NP * (size_t)plan->n_gene_ids);  // (written by gene_reduce only)
  }
  fb.add(S.ctl, sizeof(BucketCtl));
  fb.add(S.gwide, sizeof(uint32_t), S.streams ? 0 : 1);
  if (S.planned) {  // the level-1 plan's buffers (bucket_level1_plan); bdesc unless count_stage zeroed it
    if (S.sw.no_prefill) fb.add(S.bdesc, sizeof(uint16_t) * (size_t)S.n);
    fb.add(S.ctr0, 3 * sizeof(uint32_t));
    fb.add(S.l1.hist, sizeof(uint32_t) * kRadix * (size_t)S.n_ent);
  }
  return launch_fills(fb, S.s);
}

// 4. Round 8: on the planned bucket path with exact floats the quality-stream lanes run as a kernel
// of their own (segment.h k_stream_lanes) on the pair's second stream, and the key pass without
// them.  They fork here (the fills zeroed the partial rows and gwide): beside the level-1 plan and
// its classification, which are latency-bound, and whatever is left beside the key pass.  (A fork
// after the key pass, beside the partition levels >= 2, measured no gain: the early big buckets fill
// that stretch)  A call that finds another call's pair in use on the device
// keeps the one launch (the pool would then open further streams, and a process has 4 hardware
// queues).
int fork_lanes(Step& S) {
  if (!S.split) return SCT_OK;
  HIPCHK(S.st.open());
  HIPCHK(S.st.fork(0, S.s));  // (the pair's first stream has forked here too since it was opened here)
  S.split = S.st.alone;
  if (!S.split) return SCT_OK;
  HIPCHK(S.st.fork(1, S.s));
  hipStream_t sp = S.st.use(1);
  const dim3 tgrid((unsigned)cdiv(S.n, kKTile));
  uint32_t* gw = S.gene ? S.gwide : nullptr;
#define SCT_LANES(C) \
  LAUNCH_N("stream_lanes", S.n, k_stream_lanes<C>, tgrid, dim3(kBlock), sp, S.rc, S.n, S.toff, S.hbits, S.partials, gw)
  SCT_VIEW2(S.cell, SCT_LANES);
#undef SCT_LANES
  HIPCHK(S.st.mark(1, &S.lanes_done));
  return SCT_OK;
}

// 5. The first partition level planned before the key pass (segment.h k_level1_plan): run ids and
// per-entity digit counts, level 0, then level 1's classification with a grid sized for the most
// segments there can be (the device count bounds it): l1.hist then holds every segment child's start.
// No host wait: level 1's counts, final after its classification, are copied now and read by
// bucket_distinct while the key pass runs (no host wait between the key pass and level 2).
// (its buffers -- bdesc, the level-0 counters, l1.hist -- were zeroed by fills_stage)
int bucket_level1_plan(Step& S) {
  const Bits& b = S.b;
  const int64_t n = S.n, n_ent = S.n_ent;
  hipStream_t s = S.s;
  const int KB = b.k1 + b.k2 + b.h;
  LAUNCH_N("level1_plan", n, k_level1_plan, dim3((unsigned)cdiv(n, kKTile)), dim3(kBlock), s, S.hbits,
           S.kc.k1, S.kc.n_k1, n, S.toff, b, S.ent_start, S.l1);
  LAUNCH("bucket_level0", k_bucket_level0, dim3((unsigned)cdiv(n_ent, kBlock)), dim3(kBlock), s,
         S.ent_start, n_ent, n, S.bdesc, S.bent, S.seg[0], S.work[0], S.bigs, S.ctl, S.ctr0);
  const int64_t max_seg = n_ent < n / (kBigCap + 1) + 1 ? n_ent : n / (kBigCap + 1) + 1;
  if (max_seg > S.L.max_seg) return fail(SCT_ENOMEM, "level 1: %lld segments exceed the workspace", (long long)max_seg);
  LAUNCH("bucket_classify", k_bucket_classify, dim3((unsigned)max_seg), dim3(kBlock), s, (const Seg*)S.seg[0],
         S.l1.hist, S.cur, S.l1.bits, b.k1, b.k1 + b.k2, KB, 1, 1, S.bdesc, S.bent, S.seg[1], S.work[1], S.giants,
         S.bigs, S.ctl, (const uint32_t*)S.ctr0);
  return readback_start(S.ctl, sizeof(BucketCtl), s);
}

// 6 / 8. Sequential Welford (SCT_FLOAT_WELFORD): big entities one wave each (largest first), small
// ones a lane each.  It needs only the entity starts, the input columns and its own workspace, and
// writes only the mean / variance slots of the output rows (k_finalize writes the others), so it runs
// on the side streams from the moment the entity starts exist, beside the key pass' successors
// (bucket partition, hash tiles) on the caller's stream: the head kernels on s2, the rest on s3.
// finalize_stage joins both.
int welford_stage(Step& S) {
  const Layout& L = S.L;
  void* ws = S.ws;
  const int64_t n = S.n, n_ent = S.n_ent;
  const int64_t* ent_start = S.ent_start;
  double* out_f = S.c.out_f;
  StepStreams& st = S.st;
  HIPCHK(st.open());
  HIPCHK(st.fork(0, S.s));
  hipStream_t s = S.s, s2 = st.use(0), s3 = st.use(1);
  const dim3 egrid((unsigned)cdiv(n_ent, kBlock));
  if (n >= kWfWave) {
    WelfordCtl* wc = at<WelfordCtl>(ws, L.wctl);
    WelfordCtl* wch = wc + 1;  // the head group's queue
    uint32_t* worder = at<uint32_t>(ws, L.worder);
    HIPCHK(hipMemsetAsync(wc, 0, 2 * sizeof(WelfordCtl), s2));
    LAUNCH("welford_bins", k_welford_bins, egrid, dim3(kBlock), s2, ent_start, n_ent, n, wc);
    LAUNCH("welford_order", k_welford_order, egrid, dim3(kBlock), s2, ent_start, n_ent, n, wc, worder);
    LAUNCH("welford_split", k_welford_split, dim3(1), dim3(kWave), s2, wc, wch);
    // the rest on s3: every record's samples, then the other groups' chains and the small entities
    hipEvent_t split_done = nullptr;
    HIPCHK(st.fork(1, s2, &split_done));
    double* xs = at<double>(ws, L.wx);
    const dim3 xgrid((unsigned)cdiv(n, kBlock));
    const dim3 hgrid((unsigned)kWfBlocks);
    // Round 5: the head kernel's blocks each need a whole CU (k_welford_head2), which a flood of
    // other blocks keeps from them: inside the pipeline its blocks started ~1.4 ms after the launch
    // (config 2).  The key pass (the caller's stream) and the sample pass (s3) first wait on the
    // device, boundedly, for the head blocks to be resident (k_wf_gate).  A scheduling aid only: on
    // the time-out they go on, and nothing waits on them.
    // Round 6: the head kernels are submitted before the gates, so a gate that lands on
    // the head stream's hardware queue (4 per process) sits behind them instead of holding them up
    // for its whole time-out; and the gates are left out when another call on this device holds a
    // side-stream pair (concurrent pipelines: their head blocks compete for the same CUs, so one
    // pipeline's gate could wait on CUs another pipeline holds).
    const uint32_t* started = &wch->started;
    constexpr unsigned kHeadBlocks = (unsigned)(kWfHeadEnts / kW2Ents);
    const bool gate = st.alone && !S.sw.no_wf_gate;
#define SCT_WF_HEAD(C)                                                                                            \
  LAUNCH("welford_x_head", k_welford_x_ents<C>, hgrid, dim3(kBlock), s2, S.rc, ent_start, n_ent, n,               \
         (const uint32_t*)worder, (const WelfordCtl*)wch, xs);                                                    \
  LAUNCH_N("welford_head", n, k_welford_head2<C>, dim3(kHeadBlocks), dim3(kW2Waves * kWave), s2, ent_start, n_ent, \
           n, (const uint32_t*)worder, wch, (const double*)xs, out_f)
    SCT_VIEW2(S.cell, SCT_WF_HEAD);
#undef SCT_WF_HEAD
    if (gate) {
      HIPCHK(st.wait_caller(split_done));
      LAUNCH("welford_gate", k_wf_gate, dim3(1), dim3(kWave), s, started, kHeadBlocks, kWfGateTicks);
      LAUNCH("welford_gate", k_wf_gate, dim3(1), dim3(kWave), s3, started, kHeadBlocks, kWfGateTicks);
    }
#define SCT_WF_REST(C)                                                                                           \
  LAUNCH_N("welford_x", n, k_welford_x<C>, xgrid, dim3(kBlock), s3, S.rc, n, xs, ent_start, n_ent,               \
           (const uint32_t*)worder, (const uint32_t*)&wch->n_big);                                               \
  LAUNCH_N("welford_chains", n, k_welford_chains<C>, dim3(kWfBlocks), dim3(kBlock), s3, ent_start, n_ent, n,     \
           (const uint32_t*)worder, wc, (const double*)xs, out_f)
    SCT_VIEW2(S.cell, SCT_WF_REST);
#undef SCT_WF_REST
  } else {
    HIPCHK(st.fork(1, s2));
  }
#define SCT_WF(C) LAUNCH("welford", k_welford<C>, egrid, dim3(kBlock), s3, S.rc, ent_start, n_ent, n, out_f)
  SCT_VIEW2(S.cell, SCT_WF);
#undef SCT_WF
  return SCT_OK;
}

// 7. input order: runs, keys, additive metrics (+ gene-bucket counts per tile; kStreams: + the lanes)
template <bool kBucket, bool kStreams>
int launch_build_keys(Step& S) {
  const dim3 tgrid((unsigned)cdiv(S.n, kKTile));
  uint64_t* keys = S.B.ka;  // (the bucket path writes Pay records through `keys`: the same buffer)
  void* vals = kBucket ? nullptr : (void*)S.B.va;
  const size_t shm = sizeof(uint32_t) * (size_t)S.L.n_buckets;  // the gene view's bucket counts
#define SCT_KEYS(C, G)                                                                                            \
  LAUNCH_SHM_N("build_keys", S.n, (k_build_keys_run<C, G, kBucket, kStreams>), tgrid, dim3(kBlock), (G) ? shm : 0, \
               S.s, S.kc, S.rc, S.mito, S.n, S.toff, S.b, keys, vals, S.hbits, S.ent_start, S.partials, S.gcounts, \
               S.L.n_buckets, &S.ctl->err, S.gwide, S.gtoff, S.l1)
  SCT_VIEW3(S.cell, S.gene, SCT_KEYS);
#undef SCT_KEYS
  return SCT_OK;
}
int key_pass(Step& S) {
  const bool lanes = S.streams && !S.split;
  if (S.bucket) return lanes ? launch_build_keys<true, true>(S) : launch_build_keys<true, false>(S);
  if (int rc = lanes ? launch_build_keys<false, true>(S) : launch_build_keys<false, false>(S)) return rc;
  uint32_t err = 0;  // the bucket path reads the flag at its first level sync
  if (int rb = readback(&err, &S.ctl->err, sizeof(err), S.s)) return rb;
  if (err & 2) return fail(SCT_EINVAL, "a gene / cell / umi id lies outside its dictionary size");
  return SCT_OK;
}

// 9. Round 6: a side stream forked after the key pass (planned bucket path, exact floats) runs the
// gene view's plan and the big buckets of levels 0-1 beside the partition levels >= 2 and the
// hash tiles, and the cell rows' finalize beside the gene view
int launch_gene_plan(Step& S, hipStream_t on) {
  LAUNCH_SHM("gene_plan", k_gene_plan, dim3(1), dim3(kBlock), 2 * sizeof(uint32_t) * (size_t)(S.L.n_buckets + 1), on,
             (const uint32_t*)S.gcounts, S.L.n_buckets, S.gcur, S.gwork, S.n_gwork);
  return SCT_OK;
}
int fork_side(Step& S) {
  if (!S.use_side) return SCT_OK;
  HIPCHK(S.st.open());
  HIPCHK(S.st.fork(0, S.s));
  if (!S.gene) return SCT_OK;
  if (int rc = launch_gene_plan(S, S.st.use(0))) return rc;
  HIPCHK(S.st.mark(0, &S.plan_done));
  return SCT_OK;
}

int launch_big(Step& S, uint32_t cnt, const Seg* bg, hipStream_t st) {
  const dim3 bgrid(cnt);
#define SCT_BIG(C, G, W) \
  LAUNCH("big_bucket", (k_big_bucket<C, G, W>), bgrid, dim3(kBigBlock), st, bg, S.pa, S.pb, S.b, S.partials, S.dflags)
  if (S.b.k1 > kNarrowK1Bits) SCT_VIEW3(S.cell, S.gene, SCT_BIG, true);
  else SCT_VIEW3(S.cell, S.gene, SCT_BIG, false);
#undef SCT_BIG
  return SCT_OK;
}

// 10, bucket path (bucket.h): level 0 classification, MSD levels until no segment exceeds kBCap,
// then the hash-tile pass (+ giants).  One host wait per level to size the next level's launches,
// for a copy queued right after the classification: the level's scatter runs meanwhile.
// planned: level 0 and level 1 ran before the key pass (bucket_level1_plan), and the key pass wrote
// the level-1 children: the loop starts at level 2.
// Returns kRedoGlobalSort (not an error code) when build_keys saw a mapped ref id the payload cannot
// hold: the caller then reruns on the global-sort path.
constexpr int kRedoGlobalSort = 1;
int bucket_distinct(Step& S) {
  const Layout& L = S.L;
  const Bits& b = S.b;
  const int64_t n = S.n;
  hipStream_t s = S.s;
  StepStreams& st = S.st;
  BucketCtl* ctl = S.ctl;
  if (n == 0) return SCT_OK;
  const int KB = b.k1 + b.k2 + b.h;
  int level = S.planned ? 2 : 1, c = S.planned ? 1 : 0;  // (each segment carries its own depth: bucket.h Seg)
  if (!S.planned) {
    HIPCHK(hipMemsetAsync(S.bdesc, 0, sizeof(uint16_t) * (size_t)n, s));
    HIPCHK(hipMemsetAsync(ctl, 0, offsetof(BucketCtl, err), s));  // keeps ctl->err from build_keys
    HIPCHK(hipMemsetAsync(&ctl->n_big, 0, sizeof(uint32_t), s));
    LAUNCH("bucket_level0", k_bucket_level0, dim3((unsigned)cdiv(S.n_ent, kBlock)), dim3(kBlock), s,
           S.ent_start, S.n_ent, n, S.bdesc, S.bent, S.seg[0], S.work[0], S.bigs, ctl, &ctl->n_seg);
  }
  BucketCtl h{};
  // planned: the level-1 counts were read back early (bucket_level1_plan: queued before the key pass),
  // so the host sizes level 2 while the key pass still runs; the key pass's error flag is read with the
  // next level's counts (kernels before that stay in bounds: ids are clamped, ref ids masked)
  bool err_pending = false;
  if (S.planned) {
    if (int rb = readback_finish(&h, sizeof(h))) return rb;
    err_pending = true;
  }
  if (!S.planned || h.n_seg == 0) {
    if (int rb = readback(&h, ctl, sizeof(h), s)) return rb;
    err_pending = false;
  }
  const auto err_check = [&]() -> int {
    if (h.err & 2) return fail(SCT_EINVAL, "a gene / cell / umi id lies outside its dictionary size");
    return h.err ? kRedoGlobalSort : SCT_OK;
  };
  if (!err_pending)
    if (int e = err_check()) return e;
  // Round 6: the big buckets of levels 0 and 1 (their records are final once the key pass has run)
  // start on the side stream right away, beside levels >= 2, whose small partition kernels leave most
  // CUs idle; the caller's stream waits for them after the hash-tile launch.  Big buckets, level
  // segments and terminal buckets are disjoint record ranges, and the partial rows are summed
  // with atomics, so the order between the streams does not matter.
  const bool side_big = S.use_side && !S.sw.no_early_big;
  const bool early_big = side_big && h.n_big > 0 && h.n_seg > 0;
  uint32_t big_done = 0;
  if (early_big) {
    if (int r = launch_big(S, h.n_big, S.bigs, st.use(0))) return r;
    big_done = h.n_big;
  }
  while (h.n_seg > 0) {
    if ((int64_t)h.n_seg > L.max_seg || (int64_t)h.n_work > L.max_work)
      return fail(SCT_ENOMEM, "bucket level %d: %u segments / %u work items exceed the workspace", level, h.n_seg,
                  h.n_work);
    const int src = (level - 1) & 1;
    const Pay* pin = src ? S.pb : S.pa;
    Pay* pout = src ? S.pa : S.pb;
    HIPCHK(hipMemsetAsync(S.hist, 0, sizeof(uint32_t) * kRadix * (size_t)h.n_seg, s));
    LAUNCH("bucket_hist", k_bucket_hist, dim3(h.n_work), dim3(kBlock), s, pin, (const Seg*)S.seg[c],
           (const Work*)S.work[c], KB, S.hist);
    HIPCHK(hipMemsetAsync(ctl, 0, 2 * sizeof(uint32_t), s));  // next level's n_seg, n_work
    LAUNCH("bucket_classify", k_bucket_classify, dim3(h.n_seg), dim3(kBlock), s, (const Seg*)S.seg[c], S.hist, S.cur,
           0, b.k1, b.k1 + b.k2, KB, level & 1, 0, S.bdesc, S.bent, S.seg[c ^ 1], S.work[c ^ 1], S.giants, S.bigs, ctl,
           (const uint32_t*)nullptr);
    // the next level's counts are final after classify: read them while the scatter runs
    if (int rb = readback_start(ctl, sizeof(h), s)) return rb;
    const uint32_t n_work = h.n_work;
    LAUNCH("bucket_scatter", k_bucket_scatter, dim3(n_work), dim3(kSBlock), s, pin, pout, (const Seg*)S.seg[c],
           (const Work*)S.work[c], KB, S.cur);
    if (int rb = readback_finish(&h, sizeof(h))) return rb;
    if (err_pending) {
      err_pending = false;
      if (int e = err_check()) return e;
    }
    // this level's big buckets (written by its scatter) join the side stream when another level follows
    if (side_big && h.n_seg > 0 && h.n_big > big_done && !S.sw.no_level_big) {
      HIPCHK(st.fork(0, s));
      if (int r = launch_big(S, h.n_big - big_done, S.bigs + big_done, st.use(0))) return r;
      big_done = h.n_big;
    }
    c ^= 1;
    level++;
  }
  const dim3 tgrid((unsigned)cdiv(n, kWin));
  // the early big buckets finish before the hash tiles start (SCT_BIG_BESIDE_HASH=1: they may run into
  // them; the hash tiles' 40 KB blocks then hold every CU's LDS and the big buckets' 80 KB blocks wait)
  const bool join_first = big_done > 0 && !S.sw.big_beside_hash;
  if (join_first) HIPCHK(st.join(0));
#define SCT_HASH(C, G, W)                                                                                     \
  LAUNCH_N("hash_tile", n, (k_hash_tile<C, G, W>), tgrid, dim3(kHBlock), s, S.bdesc, S.bent, S.pa, S.pb, n, b, \
           S.partials, S.dflags)
  if (b.k1 > kNarrowK1Bits) SCT_VIEW3(S.cell, S.gene, SCT_HASH, true);
  else SCT_VIEW3(S.cell, S.gene, SCT_HASH, false);
#undef SCT_HASH
  // (round 4: the big buckets on a side stream beside the hash tiles measured the same step time,
  // 5.26 ms either way, profiles/r04/e_l1fast_gbam_dicts/var/); round 6: those of levels 0-1 already
  // run beside levels >= 2 (above), so only the later levels' big buckets are launched here
  if (big_done > 0 && !join_first) HIPCHK(st.join(0));
  if (h.n_big > big_done)
    if (int rc = launch_big(S, h.n_big - big_done, S.bigs + big_done, s)) return rc;
  if (h.n_giant > 0) {
    const dim3 ggrid(h.n_giant);
#define SCT_GIANT(C, G) \
  LAUNCH("bucket_giant", (k_bucket_giant<C, G>), ggrid, dim3(kBlock), s, S.giants, S.pa, S.pb, S.partials, S.dflags)
    SCT_VIEW3(S.cell, S.gene, SCT_GIANT);
#undef SCT_GIANT
  }
  return SCT_OK;
}

// 10, global-sort path: LSD radix sort of (key, record index), then one pass over the sorted keys
int sorted_distinct(Step& S) {
  int which = 0;
  if (int rc = radix_sort(S.B, S.n, S.used + S.b.h, &which, S.s)) return rc;
  const uint64_t* keys = which ? S.B.kb : S.B.ka;
  const uint32_t* vals = which ? S.B.vb : S.B.va;
  const dim3 rgrid((unsigned)cdiv(S.n, kReduceTile));
#define SCT_REDUCE(C, G)                                                                                         \
  LAUNCH_N("reduce_sorted", S.n, (k_reduce_sorted<C, G>), rgrid, dim3(kBlock), S.s, keys, vals, S.n, S.rc, S.mito, \
           S.b, S.partials, S.dflags)
  SCT_VIEW3(S.cell, S.gene, SCT_REDUCE);
#undef SCT_REDUCE
  return SCT_OK;
}

// 12. partial rows -> output rows, beside the gene view when there is a side stream; the Welford
// streams (welford_stage) are joined here
int finalize_stage(Step& S) {
  if (!S.c.out_i) return SCT_OK;
  const bool side_fin = S.use_side && S.gene && !S.sw.no_side_fin;
  if (side_fin) HIPCHK(S.st.fork(0, S.s));
  hipStream_t fs = side_fin ? S.st.use(0) : S.s;
  LAUNCH("finalize", k_finalize, dim3((unsigned)cdiv(S.n_ent * kFinThreads, kBlock)), dim3(kBlock), fs,
         (const int64_t*)S.partials, S.n_ent, S.cell ? SCT_MODE_CELL : SCT_MODE_GENE, S.exact ? 1 : 0,
         S.ent_start, S.c.out_i, S.c.out_f);
  if (!S.exact) {
    HIPCHK(S.st.join(0));
    HIPCHK(S.st.join(1));
  }
  return SCT_OK;
}

// 13. gene view: bucket starts, payload emission (input order), bucket reduction
int gene_stage(Step& S) {
  if (!S.gene) return SCT_OK;
  const Layout& L = S.L;
  const int64_t n = S.n;
  void* gpay = at<GenePayload>(S.ws, L.gpay);
  if (S.plan_done) HIPCHK(S.st.wait_caller(S.plan_done));
  else if (int rc = launch_gene_plan(S, S.s)) return rc;
  static_assert(kEmitTile == kKTile, "gene_emit tiles are the key pass's tiles (gtoff)");
  const int staged = L.n_buckets <= kEmitStagedBuckets ? 1 : 0;
  LAUNCH_SHM_N("gene_emit", n, k_gene_emit, dim3((unsigned)cdiv(n, kEmitTile)), dim3(kBlock),
               (staged ? 3 : 2) * sizeof(uint32_t) * (size_t)L.n_buckets, S.s, S.c.rec->gene, S.rc,
               (const uint16_t*)S.dflags, n, (const uint32_t*)S.gcur, (const uint32_t*)S.gtoff, L.n_buckets,
               (const uint32_t*)S.gwide, staged, gpay);
  LAUNCH_N("gene_reduce", n, k_gene_reduce, dim3((unsigned)L.max_gene_work), dim3(kBlock), S.s, (const void*)gpay,
           (const int64_t*)S.gwork, (const int64_t*)S.n_gwork, S.c.plan->n_gene_ids, (const uint32_t*)S.gwide,
           S.c.gene_partials);
  return SCT_OK;
}

int run_step(const StepCall& c, const StepSwitches& sw, bool allow_bucket) {
  const Layout L = layout_for(c.plan);
  if (!c.ws || c.ws_bytes < L.total) return fail(SCT_ENOMEM, "workspace too small (%zu < %zu)", c.ws_bytes, L.total);
  Step S(c, sw, L, allow_bucket);
  if (int rc = count_stage(S)) return rc;                                                     // 1
  if (int rc = plan_key_bits(S.bucket, S.n_ent, &S.b, &S.used)) return rc;                    // 2
  if (int rc = fills_stage(S)) return rc;                                                     // 3
  if (int rc = fork_lanes(S)) return rc;                                                      // 4
  if (S.planned)
    if (int rc = bucket_level1_plan(S)) return rc;                                            // 5
  // Welford (the drop-in default): forked as soon as the entity starts exist -- after the level-1
  // plan when there is one (round 4: the head group's chains then start before the key pass),
  // else after the key pass
  const bool welford = !S.exact && c.out_i;
  if (welford && S.planned)
    if (int rc = welford_stage(S)) return rc;                                                 // 6
  if (int rc = key_pass(S)) return rc;                                                        // 7
  if (welford && !S.planned)
    if (int rc = welford_stage(S)) return rc;                                                 // 8
  if (int rc = fork_side(S)) return rc;                                                       // 9
  // 10. distinct counts (+ per-record distinct events for the gene view)
  if (int rc = S.bucket ? bucket_distinct(S) : sorted_distinct(S)) {
    if (rc != kRedoGlobalSort) return rc;
    // a mapped ref id does not fit the bucket payload: redo on the global-sort path, which reuses the
    // workspace, under the switches this pass read
    HIPCHK(S.st.drain());
    return run_step(c, sw, false);
  }
  // 11. the stream lanes are complete before the rows' finalize reads their slots, on whichever
  // stream it runs, and before k_gene_emit reads gwide
  if (S.split) HIPCHK(S.st.join(1, S.lanes_done));
  if (int rc = finalize_stage(S)) return rc;                                                  // 12
  if (int rc = gene_stage(S)) return rc;                                                      // 13
  if (S.use_side) HIPCHK(S.st.join(0));                                                       // 14
  if (c.n_rows) *c.n_rows = S.n_ent;
  return SCT_OK;
}

int pipeline(const StepCall& c) { return run_step(c, StepSwitches{}, true); }

// ---- tag sort ----
struct SortLayout {
  size_t recs, recs2, ka, kb, va, vb, counts, offsets, sums, bad, lka, lkb, lva, lvb, longs, tctl, gseg, total;
  int64_t count_cap;
};

struct CountLayout {
  size_t ka, kb, va, vb, counts, offsets, sums, flags_a, offs_a, flags_b, offs_b, pair_cell, pair_col, pair_tri;
  size_t cell_first, cell_npairs, cell_pstart, row_of, row_pairs, scalars, total;
  int64_t count_cap;
};

CountLayout count_layout(const sct_count_input_t* in) {
  CountLayout L;
  const int64_t n1 = in->n > 0 ? in->n : 1;
  const int64_t c1 = in->n_cell_ids > 0 ? in->n_cell_ids : 1;
  const int64_t m = n1 > c1 ? n1 : c1;  // the record sort and the cell-order sort share buffers
  const int64_t cm = (int64_t)kRadix * cdiv(m, kSortTile);
  L.count_cap = cm;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t o = off;
    off += align_up(bytes);
    return o;
  };
  L.ka = take(8 * (size_t)m);
  L.kb = take(8 * (size_t)m);
  L.va = take(4 * (size_t)m);
  L.vb = take(4 * (size_t)m);
  L.counts = take(4 * (size_t)cm);
  L.offsets = take(4 * (size_t)cm);
  L.sums = take(8 * (size_t)(cdiv(cm > m ? cm : m, kScanChunk) + 1));
  L.flags_a = take(4 * (size_t)n1);
  L.offs_a = take(4 * (size_t)n1);
  L.flags_b = take(4 * (size_t)n1);
  L.offs_b = take(4 * (size_t)n1);
  L.pair_cell = take(4 * (size_t)n1);
  L.pair_col = take(4 * (size_t)n1);
  L.pair_tri = take(4 * (size_t)n1);
  L.cell_first = take(4 * (size_t)c1);
  L.cell_npairs = take(4 * (size_t)c1);
  L.cell_pstart = take(4 * (size_t)c1);
  L.row_of = take(4 * (size_t)c1);
  L.row_pairs = take(4 * (size_t)c1);
  L.scalars = take(6 * sizeof(uint64_t));
  L.total = off;
  return L;
}

SortLayout sort_layout(int64_t n) {
  SortLayout L;
  const int64_t n1 = n > 0 ? n : 1;
  // The digit counts serve two tilings: the row passes (kRowTile) and radix_sort (kSortTile, the
  // tiebreak and multi-round paths).  Round 3 sized them by kRowTile alone, which only held while
  // both tiles were 2048 items: a 1024-item kSortTile overflowed `counts` into `offsets`, the scan
  // then read its own output, and the downsweep wrote through garbage offsets (the illegal memory
  // access of the SCT_SORT_ITEMS=4 build).  radix_sort now also checks its capacity.
  const int64_t row_tiles = cdiv(n1, kRowTile), sort_tiles = cdiv(n1, kSortTile);
  int64_t tiles = row_tiles > sort_tiles ? row_tiles : sort_tiles;
  const int64_t seg_tiles = cdiv(n1, kSegTile) + kMsdRadix;  // the group sort's segmented passes (tagsort.h)
  tiles = tiles > seg_tiles ? tiles : seg_tiles;
  const int64_t msd_tiles = cdiv(n1, kMsdTile) * (kMsdRadix / kRadix);  // and its MSD pass (kMsdRadix digits)
  tiles = tiles > msd_tiles ? tiles : msd_tiles;
  const int64_t m = (int64_t)kRadix * tiles;
  L.count_cap = m;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t o = off;
    off += align_up(bytes);
    return o;
  };
  L.recs = take(sizeof(PackedRec) * (size_t)n1);
  L.recs2 = take(sizeof(PackedRec) * (size_t)n1);
  L.ka = take(sizeof(uint64_t) * (size_t)n1);
  L.kb = take(sizeof(uint64_t) * (size_t)n1);
  L.va = take(sizeof(uint32_t) * (size_t)n1);
  L.vb = take(sizeof(uint32_t) * (size_t)n1);
  L.counts = take(sizeof(uint32_t) * (size_t)m);
  L.offsets = take(sizeof(uint32_t) * (size_t)m);
  L.sums = take(sizeof(uint64_t) * (size_t)(cdiv(m, kScanChunk) + 1));
  L.bad = take(sizeof(uint64_t));
  // tiebreak fix-up of runs longer than kTieShort (tagsort.h): compact keys / values, run list
  L.lka = take(sizeof(uint64_t) * (size_t)n1);
  L.lkb = take(sizeof(uint64_t) * (size_t)n1);
  L.lva = take(sizeof(uint32_t) * (size_t)n1);
  L.lvb = take(sizeof(uint32_t) * (size_t)n1);
  L.longs = take(sizeof(uint4) * (size_t)(n1 / (kTieShort + 1) + 1));
  L.tctl = take(4 * sizeof(uint32_t));
  L.gseg = take((3 * kMsdRadix + 1) * sizeof(uint32_t));
  L.total = off;
  return L;
}

// the order's fields, most significant first (+ the tiebreak, least significant)
int order_fields(int32_t order, const sct_plan_t* plan, bool tie, int32_t n_tie, KeyField* f, int* nf) {
  const KeyField cell{0, bitlen((uint64_t)plan->n_cell_ids)}, umi{1, bitlen((uint64_t)plan->n_umi_ids)},
      gene{2, bitlen((uint64_t)plan->n_gene_ids)};
  int k = 0;
  if (order == SCT_ORDER_CELL) {
    f[k++] = cell;
  } else if (order == SCT_ORDER_CELL_UMI_GENE) {
    f[k++] = cell, f[k++] = umi, f[k++] = gene;
  } else if (order == SCT_ORDER_GENE_CELL_UMI) {
    f[k++] = gene, f[k++] = cell, f[k++] = umi;
  } else {
    return fail(SCT_EINVAL, "unknown sort order %d", order);
  }
  if (tie) {
    if (n_tie <= 0) return fail(SCT_EINVAL, "n_tiebreak_ids must be positive");
    f[k++] = KeyField{3, bitlen((uint64_t)n_tie)};
  }
  *nf = k;
  return SCT_OK;
}

int check_sort_args(const sct_plan_t* plan, const sct_records_t* rec) {
  if (!plan || !rec) return fail(SCT_EINVAL, "NULL plan or records");
  if (plan->n_records < 0 || plan->n_records > (int64_t)0x7FFFFFFF)
    return fail(SCT_EINVAL, "n_records %lld out of range [0, 2^31)", (long long)plan->n_records);
  if (rec->n != plan->n_records) return fail(SCT_EINVAL, "records.n != plan.n_records");
  if (plan->n_cell_ids <= 0 || plan->n_gene_ids <= 0 || plan->n_umi_ids <= 0)
    return fail(SCT_EINVAL, "dictionary sizes must be positive");
  return SCT_OK;
}

}  // namespace

// ======================================================================================
// C-ABI
// ======================================================================================

extern "C" {

int sct_abi_version(void) { return SCT_ABI_VERSION; }

const char* sct_last_error(void) { return last_error().c_str(); }

int sct_profile_enable(int on) {
  prof_on() = on != 0;
  return SCT_OK;
}

int sct_profile_only(const char* kernel_name) {
  prof_only() = kernel_name ? kernel_name : "";
  return SCT_OK;
}

int sct_profile_read_items(const char** names, double* ms, int64_t* launches, int64_t* items, int max_kernels) {
  // waits for the recorded events, returns per-kernel totals, and resets the counters
  static thread_local std::vector<std::string> held;
  held.clear();
  int k = 0;
  for (auto& e : prof_entries()) {
    double tot = 0.0;
    for (auto& pr : e.ev) {
      float t = 0.f;
      if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&t, pr.first, pr.second) == hipSuccess)
        tot += t;
      (void)hipEventDestroy(pr.first);
      (void)hipEventDestroy(pr.second);
    }
    held.push_back(e.name);
    if (k < max_kernels) {
      if (ms) ms[k] = tot;
      if (launches) launches[k] = (int64_t)e.ev.size();
      if (items) items[k] = e.items;
    }
    k++;
  }
  for (int i = 0; i < k && i < max_kernels; i++)
    if (names) names[i] = held[i].c_str();
  prof_entries().clear();
  return k;
}

int sct_profile_read(const char** names, double* ms, int64_t* launches, int max_kernels) {
  return sct_profile_read_items(names, ms, launches, nullptr, max_kernels);
}

int sct_workspace_size(const sct_plan_t* plan, size_t* bytes) {
  int rc = check_plan(plan, nullptr);
  if (rc) return rc;
  if (!bytes) return fail(SCT_EINVAL, "bytes is NULL");
  *bytes = layout_for(plan).total;
  return SCT_OK;
}

int sct_count_entities(const sct_plan_t* plan, const sct_records_t* rec, void* workspace, size_t workspace_bytes,
                       int64_t* n_entities, void* stream) {
  last_error().clear();
  int rc = check_plan(plan, rec);
  if (rc) return rc;
  if (!n_entities) return fail(SCT_EINVAL, "n_entities is NULL");
  if (plan->mode == SCT_MODE_GENE_GROUPED) {
    *n_entities = plan->n_gene_ids;
    return SCT_OK;
  }
  if (rec->n == 0) {
    *n_entities = 0;
    return SCT_OK;
  }
  sct_plan_t p1 = *plan;
  p1.max_entities = 1;
  p1.flags = 0;
  const Layout L = layout_for(&p1);
  if (!workspace || workspace_bytes < count_bytes(L))
    return fail(SCT_ENOMEM, "workspace too small for counting (%zu < %zu)", workspace_bytes, count_bytes(L));
  return count_runs(plan->mode == SCT_MODE_CELL ? rec->cell : rec->gene, rec->n, workspace, L, CountOpts{}, n_entities,
                    nullptr, (hipStream_t)stream);
}

int sct_compute_metrics(const sct_plan_t* plan, const sct_records_t* rec, const uint8_t* gene_is_mito,
                        const uint8_t* gene_is_multi, void* workspace, size_t workspace_bytes, int64_t* out_ints,
                        double* out_floats, int64_t capacity, int64_t* n_rows, void* stream) {
  (void)gene_is_multi;  // multi-gene rows are dropped by the caller (gatherer.py:210-212)
  last_error().clear();
  int rc = check_plan(plan, rec);
  if (rc) return rc;
  if (plan->mode == SCT_MODE_GENE_GROUPED)
    return fail(SCT_EINVAL, "sct_compute_metrics handles RUN modes; use sct_gene_partials for GROUPED");
  if (!n_rows || !out_ints || !out_floats) return fail(SCT_EINVAL, "NULL output");
  if (plan->mode == SCT_MODE_CELL && !gene_is_mito) return fail(SCT_EINVAL, "gene_is_mito is NULL");
  if (rec->n == 0) {
    *n_rows = 0;
    return SCT_OK;
  }
  return pipeline(StepCall{plan, rec, gene_is_mito, workspace, workspace_bytes, out_ints, out_floats, capacity, n_rows,
                           nullptr, (hipStream_t)stream});
}

int sct_gene_partials(const sct_plan_t* plan, const sct_records_t* rec, void* workspace, size_t workspace_bytes,
                      int64_t* partials, void* stream) {
  last_error().clear();
  int rc = check_plan(plan, rec);
  if (rc) return rc;
  if (plan->mode != SCT_MODE_GENE_GROUPED) return fail(SCT_EINVAL, "sct_gene_partials needs SCT_MODE_GENE_GROUPED");
  if (plan->float_mode != SCT_FLOAT_EXACT_SUM) return fail(SCT_EINVAL, "GROUPED partials need SCT_FLOAT_EXACT_SUM");
  if (!partials) return fail(SCT_EINVAL, "partials is NULL");
  hipStream_t s = (hipStream_t)stream;
  if (rec->n == 0) {
    HIPCHK(hipMemsetAsync(partials, 0, sizeof(int64_t) * SCT_NP * (size_t)plan->n_gene_ids, s));
    return SCT_OK;
  }
  return pipeline(StepCall{plan, rec, nullptr, workspace, workspace_bytes, nullptr, nullptr, 0, nullptr, partials, s});
}

int sct_cell_metrics_gene_partials(const sct_plan_t* plan, const sct_records_t* rec, const uint8_t* gene_is_mito,
                                   void* workspace, size_t workspace_bytes, int64_t* out_ints, double* out_floats,
                                   int64_t capacity, int64_t* n_rows, int64_t* gene_partials, void* stream) {
  last_error().clear();
  int rc = check_plan(plan, rec);
  if (rc) return rc;
  if (plan->mode != SCT_MODE_CELL || !(plan->flags & SCT_PLAN_GENE_PARTIALS))
    return fail(SCT_EINVAL, "needs SCT_MODE_CELL with SCT_PLAN_GENE_PARTIALS");
  if (!n_rows || !out_ints || !out_floats || !gene_partials || !gene_is_mito) return fail(SCT_EINVAL, "NULL argument");
  hipStream_t s = (hipStream_t)stream;
  if (rec->n == 0) {
    *n_rows = 0;
    HIPCHK(hipMemsetAsync(gene_partials, 0, sizeof(int64_t) * SCT_NP * (size_t)plan->n_gene_ids, s));
    return SCT_OK;
  }
  return pipeline(StepCall{plan, rec, gene_is_mito, workspace, workspace_bytes, out_ints, out_floats, capacity, n_rows,
                           gene_partials, s});
}

int sct_tag_sort_workspace_size(const sct_plan_t* plan, size_t* bytes) {
  if (!plan || !bytes) return fail(SCT_EINVAL, "NULL argument");
  *bytes = sort_layout(plan->n_records).total;
  return SCT_OK;
}

int sct_tag_sort(const sct_plan_t* plan, const sct_records_t* in, const int32_t* tiebreak, int32_t n_tiebreak_ids,
                 int32_t order, const sct_records_t* out, void* workspace, size_t workspace_bytes, void* stream) {
  last_error().clear();
  int rc = check_sort_args(plan, in);
  if (rc) return rc;
  if (!out || out->n != in->n) return fail(SCT_EINVAL, "out must hold records.n records");
  KeyField f[4];
  int nf = 0;
  rc = order_fields(order, plan, tiebreak != nullptr, n_tiebreak_ids, f, &nf);
  if (rc) return rc;
  const int64_t n = in->n;
  if (n == 0) return SCT_OK;
  const SortLayout L = sort_layout(n);
  if (!workspace || workspace_bytes < L.total)
    return fail(SCT_ENOMEM, "workspace too small (%zu < %zu)", workspace_bytes, L.total);
  hipStream_t s = (hipStream_t)stream;
  uint4* recs = at<uint4>(workspace, L.recs);
  if (order == SCT_ORDER_CELL && !tiebreak) {  // whole rows through 8-bit LSD passes, no gathers
    const int bits = f[0].bits;
    const int passes = bits > kRadixBits ? (bits + kRadixBits - 1) / kRadixBits : 1;
    const int64_t tiles = cdiv(n, kRowTile);
    uint32_t* counts = at<uint32_t>(workspace, L.counts);
    uint32_t* offsets = at<uint32_t>(workspace, L.offsets);
    uint64_t* sums = at<uint64_t>(workspace, L.sums);
    uint4* rows[2] = {recs, at<uint4>(workspace, L.recs2)};
    int32_t* keys[2] = {at<int32_t>(workspace, L.ka), at<int32_t>(workspace, L.kb)};
    for (int ps = 0; ps < passes; ps++) {
      const int shift = ps * kRadixBits;
      const bool first = ps == 0, last = ps == passes - 1;
      const int32_t* hkey = first ? in->cell : keys[(ps - 1) & 1];
      LAUNCH_N("tag_row_hist", n, k_row_hist, dim3((unsigned)tiles), dim3(kBlock), s, hkey, n, shift, tiles, counts);
      rc = scan_counts(counts, (int64_t)kRadix * tiles, offsets, sums, s);
      if (rc) return rc;
      const uint4* rin = first ? nullptr : rows[(ps - 1) & 1];
      uint4* rout = rows[ps & 1];
      int32_t* kout = keys[ps & 1];
#define SCT_ROWS(A, Z)                                                                                              \
  LAUNCH_N("tag_row_scatter", n, (k_row_scatter<A, Z>), dim3((unsigned)tiles), dim3(kBlock), s, *in, rin, rout, kout, \
         *out, n, shift, tiles, (const uint32_t*)offsets)
      if (first && last) {
        SCT_ROWS(true, true);
      } else if (first) {
        SCT_ROWS(true, false);
      } else if (last) {
        SCT_ROWS(false, true);
      } else {
        SCT_ROWS(false, false);
      }
#undef SCT_ROWS
    }
    return SCT_OK;
  }
  SortBuffers B{at<uint64_t>(workspace, L.ka), at<uint64_t>(workspace, L.kb), at<uint32_t>(workspace, L.va),
                at<uint32_t>(workspace, L.vb), at<uint32_t>(workspace, L.counts), at<uint32_t>(workspace, L.offsets),
                at<uint64_t>(workspace, L.sums), L.count_cap};
  const dim3 grid((unsigned)cdiv(n, kBlock));
  // (CB, UB, GE[, query name]) by groups (tagsort.h, round 6): an LSD sort of (cell, top umi bits) only,
  // then every group sorted inside its own positions
  if (order == SCT_ORDER_CELL_UMI_GENE && !env_is("SCT_TAG_GROUP_SORT", '0')) {
    GroupBits gb{};
    gb.c = f[0].bits, gb.u = f[1].bits, gb.g = f[2].bits, gb.t = tiebreak ? f[3].bits : 0;
    const int ub_min = gb.u + gb.g + gb.t - 52 > 0 ? gb.u + gb.g + gb.t - 52 : 0;  // W fits 52 bits
    const int passes = (gb.c + ub_min + kRadixBits - 1) / kRadixBits;
    if (ub_min <= gb.u && passes <= 4) {
      const bool msd = gb.c + ub_min > kRadixBits && !env_is("SCT_TAG_GROUP_MSD", '0');
      // K1 is filled to the width its passes sort anyway (smaller groups for free): LSD, whole 8-bit
      // digits; MSD, the kMsdBits-bit top digit plus the fewest 8-bit segmented passes (<= 32 bits)
      int kw = kRadixBits * passes;
      if (msd) {
        const int segp = gb.c + ub_min > kMsdBits ? (gb.c + ub_min - kMsdBits + kRadixBits - 1) / kRadixBits : 0;
        kw = kMsdBits + kRadixBits * segp < 32 ? kMsdBits + kRadixBits * segp : 32;
      }
      gb.ub = kw - gb.c < gb.u ? kw - gb.c : gb.u;
      gb.ul = gb.u - gb.ub;
      uint4* longs = at<uint4>(workspace, L.longs);
      uint32_t* tctl = at<uint32_t>(workspace, L.tctl);
      HIPCHK(hipMemsetAsync(tctl, 0, 4 * sizeof(uint32_t), s));
      int which = 0;
      const int kbits = gb.c + gb.ub;
      const uint32_t* keys = nullptr;
      const uint32_t* perm = nullptr;
      if (msd) {
        // rows written once in the order of K1's top digit, then the rest of K1 inside those buckets
        const int sh_top = kbits > kMsdBits ? kbits - kMsdBits : 0;
        const int64_t mt = cdiv(n, kMsdTile);
        const int64_t tmax = cdiv(n, kSegTile) + kMsdRadix;
        if ((int64_t)kMsdRadix * mt > L.count_cap || (int64_t)kRadix * tmax > L.count_cap)
          return fail(SCT_EINVAL, "group sort: digit counts exceed the workspace");
        uint32_t* ka32 = reinterpret_cast<uint32_t*>(B.ka);
        uint32_t* kb32 = reinterpret_cast<uint32_t*>(B.kb);
        uint32_t* gseg = at<uint32_t>(workspace, L.gseg);
        LAUNCH_N("tag_group_hist", n, k_gmsd_hist, dim3((unsigned)mt), dim3(kBlock), s, in->cell, in->umi, n, gb,
                 sh_top, mt, B.counts, tctl);
        rc = scan_counts(B.counts, (int64_t)kMsdRadix * mt, B.offsets, B.sums, s);
        if (rc) return rc;
        LAUNCH_N("tag_group_msd", n, k_gmsd_scatter, dim3((unsigned)mt), dim3(kBlock), s, *in, tiebreak, n, gb, sh_top,
                 mt, (const uint32_t*)B.offsets, recs, ka32);
        LAUNCH("tag_group_plan", k_gseg_plan, dim3(1), dim3(kBlock), s, (const uint32_t*)B.offsets, mt, n, gseg);
        const int passes = (sh_top + kRadixBits - 1) / kRadixBits;
        int cur = 0;
        for (int ps = 0; ps < passes; ps++) {
          const uint32_t* kin = cur ? kb32 : ka32;
          const uint32_t* vin = cur ? B.vb : B.va;
          uint32_t* kout = cur ? ka32 : kb32;
          uint32_t* vout = cur ? B.va : B.vb;
          LAUNCH_N("radix_upsweep", n, k_gseg_upsweep, dim3((unsigned)tmax), dim3(kBlock), s, kin, ps * kRadixBits,
                   (const uint32_t*)gseg, B.counts);
          rc = scan_counts(B.counts, (int64_t)kRadix * tmax, B.offsets, B.sums, s);
          if (rc) return rc;
          if (ps == 0) {
            LAUNCH_N("radix_downsweep", n, k_gseg_downsweep<true>, dim3((unsigned)tmax), dim3(kBlock), s, kin, vin,
                     kout, vout, ps * kRadixBits, (const uint32_t*)gseg, (const uint32_t*)B.offsets);
          } else {
            LAUNCH_N("radix_downsweep", n, k_gseg_downsweep<false>, dim3((unsigned)tmax), dim3(kBlock), s, kin, vin,
                     kout, vout, ps * kRadixBits, (const uint32_t*)gseg, (const uint32_t*)B.offsets);
          }
          cur ^= 1;
        }
        keys = cur ? kb32 : ka32;
        perm = cur ? B.vb : B.va;
        if (passes == 0)  // the top digit was all of K1: the rows are in K1 order already
          LAUNCH("tag_group_iota", k_iota, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), s, B.va, n);
      } else {
        LAUNCH_N("tag_group_keys", n, k_pack_group_keys, grid, dim3(kBlock), s, *in, n, gb, tiebreak, recs,
                 reinterpret_cast<uint32_t*>(B.ka), tctl);
        if (kbits > 0) {
          rc = radix_sort32(B, n, kbits, &which, s, true);
        } else {  // one group: the values are the positions
          LAUNCH("tag_group_iota", k_iota, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), s, B.va, n);
        }
        if (rc) return rc;
        keys = reinterpret_cast<const uint32_t*>(which ? B.kb : B.ka);
        perm = which ? B.vb : B.va;
      }
      uint2* glong = reinterpret_cast<uint2*>(longs);
      LAUNCH_N("tag_group_wave", n, k_group_wave, grid, dim3(kBlock), s, keys, perm, (const uint4*)recs, n, gb, *out,
               glong, tctl);
      uint32_t h[3] = {0, 0, 0};
      if (int rb = readback(h, tctl, sizeof(h), s)) return rb;
      if (!h[1] && !h[2]) {
        if (h[0])
          LAUNCH("tag_group_long", k_group_long, dim3(h[0]), dim3(kBlock), s, keys, perm, (const uint4*)recs, gb,
                 (const uint2*)glong, *out);
        return SCT_OK;
      }
      // a group past kGroupCap records or a cell id the key cannot hold: the general path below
    }
  }
  int field_bits = 0;
  for (int i = 0; i < nf - (tiebreak ? 1 : 0); i++) field_bits += f[i].bits;
  if (!(tiebreak && field_bits <= 64)) LAUNCH_N("tag_pack", n, k_pack, grid, dim3(kBlock), s, *in, recs);
  if (tiebreak && field_bits <= 64) {
    // one radix sort on the tag fields, then the query-name order inside runs of equal fields
    RoundKey rk{};
    rk.nf = nf - 1;
    rk.bits = field_bits;
    for (int i = 0; i < rk.nf; i++) rk.f[i] = f[i];
    const int tie_top = f[nf - 1].bits;  // the tiebreak's width
    int th = (field_bits + kRadixBits - 1) / kRadixBits * kRadixBits - field_bits;  // free bits of the last digit
    if (th > tie_top) th = tie_top;
    if (field_bits + th > 64) th = 64 - field_bits;
    LAUNCH_N("tag_pack_keys", n, k_pack_field_keys, grid, dim3(kBlock), s, *in, n, rk, tiebreak, tie_top, th, recs,
             B.ka, B.va);
    int which = 0;
    rc = radix_sort(B, n, field_bits + th, &which, s);
    if (rc) return rc;
    const uint64_t* keys = which ? B.kb : B.ka;
    uint32_t* perm = which ? B.vb : B.va;
    uint4* longs = at<uint4>(workspace, L.longs);
    uint32_t* tctl = at<uint32_t>(workspace, L.tctl);
    HIPCHK(hipMemsetAsync(tctl, 0, 2 * sizeof(uint32_t), s));
    uint32_t* pos_of = at<uint32_t>(workspace, L.recs2);  // the row buffer is free on this path
    LAUNCH("tag_ties", k_tie_wave2, grid, dim3(kBlock), s, keys, perm, tiebreak, n, longs, tctl);
    uint32_t h[2] = {0, 0};
    if (int rb = readback(h, tctl, sizeof(h), s)) return rb;
    if (h[0] > 0) {  // runs longer than kTieShort: (run, tiebreak) radix sort of their records
      const int tie_bits = bitlen((uint64_t)n_tiebreak_ids);
      SortBuffers LB{at<uint64_t>(workspace, L.lka), at<uint64_t>(workspace, L.lkb), at<uint32_t>(workspace, L.lva),
                     at<uint32_t>(workspace, L.lvb), B.counts, B.offsets, B.sums, B.count_cap};
      LAUNCH("tag_long_keys", k_long_keys, dim3(h[0]), dim3(kBlock), s, (const uint4*)longs, (const uint32_t*)perm,
             tiebreak, tie_bits, LB.ka, LB.va, pos_of);
      int w2 = 0;
      rc = radix_sort(LB, (int64_t)h[1], bitlen((uint64_t)h[1]) + tie_bits, &w2, s);
      if (rc) return rc;
      LAUNCH("tag_long_scatter", k_long_scatter, dim3((unsigned)cdiv(h[1], kBlock)), dim3(kBlock), s,
             (const uint32_t*)pos_of, (const uint32_t*)(w2 ? LB.vb : LB.va), (int64_t)h[1], perm);
    }
    LAUNCH_N("tag_unpack", n, k_unpack, grid, dim3(kBlock), s, (const uint4*)recs, (const uint32_t*)perm, n, *out);
    return SCT_OK;
  }
  // rounds: fields from the least significant end, packed greedily into <= 64-bit keys
  const uint32_t* perm = nullptr;
  int hi = nf;  // fields [lo, hi) of the next round (most significant first)
  while (hi > 0) {
    int lo = hi, bits = 0;
    while (lo > 0 && bits + f[lo - 1].bits <= 64) bits += f[--lo].bits;
    RoundKey rk{};
    rk.nf = hi - lo;
    rk.bits = bits;
    for (int i = 0; i < rk.nf; i++) rk.f[i] = f[lo + i];
    LAUNCH_N("tag_keys", n, k_round_keys, grid, dim3(kBlock), s, (const uint4*)recs, tiebreak, perm, n, rk, B.ka, B.va);
    int which = 0;
    rc = radix_sort(B, n, bits, &which, s);
    if (rc) return rc;
    perm = which ? B.vb : B.va;
    hi = lo;
  }
  LAUNCH_N("tag_unpack", n, k_unpack, grid, dim3(kBlock), s, (const uint4*)recs, perm, n, *out);
  return SCT_OK;
}

// ---- cell bins for the exchange between devices (exchange.h; SplitBam's bins, bam.py:439-480) ----

int sct_bin_workspace_size(const sct_plan_t* plan, int32_t n_bins, size_t* bytes) {
  last_error().clear();
  if (!plan || !bytes) return fail(SCT_EINVAL, "NULL argument");
  if (n_bins < 1 || n_bins > SCT_MAX_BINS) return fail(SCT_EINVAL, "n_bins %d outside [1, %d]", n_bins, SCT_MAX_BINS);
  const int64_t tiles = cdiv(plan->n_records > 0 ? plan->n_records : 1, kBinTile);
  const int64_t m = (int64_t)n_bins * tiles;
  *bytes = 2 * align_up(sizeof(uint32_t) * (size_t)m) + align_up(sizeof(uint64_t) * (size_t)(cdiv(m, kScanChunk) + 1));
  return SCT_OK;
}

int sct_bin_records(const sct_plan_t* plan, const sct_records_t* in, const int32_t* tiebreak,
                    const uint8_t* bin_of_cell, int32_t n_bins, const sct_records_t* out, int32_t* tiebreak_out,
                    int64_t* bin_counts, void* workspace, size_t workspace_bytes, void* stream) {
  last_error().clear();
  int rc = check_sort_args(plan, in);
  if (rc) return rc;
  if (!out || out->n != in->n) return fail(SCT_EINVAL, "out must hold records.n records");
  if (n_bins < 1 || n_bins > SCT_MAX_BINS) return fail(SCT_EINVAL, "n_bins %d outside [1, %d]", n_bins, SCT_MAX_BINS);
  if (!bin_counts) return fail(SCT_EINVAL, "bin_counts is NULL");
  if ((tiebreak == nullptr) != (tiebreak_out == nullptr))
    return fail(SCT_EINVAL, "tiebreak and tiebreak_out: both or neither");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = in->n;
  if (n == 0) {
    HIPCHK(hipMemsetAsync(bin_counts, 0, sizeof(int64_t) * (size_t)n_bins, s));
    return SCT_OK;
  }
  size_t need = 0;
  rc = sct_bin_workspace_size(plan, n_bins, &need);
  if (rc) return rc;
  if (!workspace || workspace_bytes < need) return fail(SCT_ENOMEM, "workspace too small (%zu < %zu)", workspace_bytes, need);
  const int64_t tiles = cdiv(n, kBinTile);
  const int64_t m = (int64_t)n_bins * tiles;
  uint32_t* counts = (uint32_t*)workspace;
  uint32_t* offsets = (uint32_t*)((uint8_t*)workspace + align_up(sizeof(uint32_t) * (size_t)m));
  uint64_t* sums = (uint64_t*)((uint8_t*)workspace + 2 * align_up(sizeof(uint32_t) * (size_t)m));
  const uint32_t nb = (uint32_t)n_bins, nc = (uint32_t)plan->n_cell_ids;
  const int bin_bits = bitlen((uint64_t)n_bins);  // bits of the bin values 0 .. n_bins - 1
  LAUNCH_N("bin_hist", n, k_bin_hist, dim3((unsigned)tiles), dim3(kBlock), s, in->cell, n, bin_of_cell, nb, nc, tiles,
           counts);
  rc = scan_counts(counts, m, offsets, sums, s);
  if (rc) return rc;
  if (tiebreak) {
    LAUNCH_N("bin_scatter", n, k_bin_scatter<true>, dim3((unsigned)tiles), dim3(kBlock), s, *in, tiebreak, *out,
             tiebreak_out, n, bin_of_cell, nb, nc, bin_bits, tiles, (const uint32_t*)offsets);
  } else {
    LAUNCH_N("bin_scatter", n, k_bin_scatter<false>, dim3((unsigned)tiles), dim3(kBlock), s, *in, tiebreak, *out,
             tiebreak_out, n, bin_of_cell, nb, nc, bin_bits, tiles, (const uint32_t*)offsets);
  }
  LAUNCH("bin_totals", k_bin_totals, dim3(1), dim3(kBlock), s, (const uint32_t*)offsets, tiles, nb, n, bin_counts);
  return SCT_OK;
}

int sct_verify_sort(const sct_plan_t* plan, const sct_records_t* rec, const int32_t* tiebreak, int32_t order,
                    void* workspace, size_t workspace_bytes, int64_t* first_violation, void* stream) {
  last_error().clear();
  int rc = check_sort_args(plan, rec);
  if (rc) return rc;
  if (!first_violation) return fail(SCT_EINVAL, "first_violation is NULL");
  KeyField f[4];
  int nf = 0;
  rc = order_fields(order, plan, false, 0, f, &nf);
  if (rc) return rc;
  *first_violation = -1;
  if (rec->n < 2) return SCT_OK;
  const SortLayout L = sort_layout(rec->n);
  if (!workspace || workspace_bytes < L.total)
    return fail(SCT_ENOMEM, "workspace too small (%zu < %zu)", workspace_bytes, L.total);
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* bad = at<unsigned long long>(workspace, L.bad);
  const unsigned long long none = (unsigned long long)rec->n;
  HIPCHK(hipMemsetAsync(bad, 0xFF, sizeof(unsigned long long), s));  // no violation: ~0
  for (int i = nf; i < 3; i++) f[i] = KeyField{0, 0};
  LAUNCH("tag_verify", k_verify_order, dim3((unsigned)cdiv(rec->n - 1, kBlock)), dim3(kBlock), s, *rec, tiebreak,
         f[0], f[1], f[2], nf, bad);
  unsigned long long h = 0;
  if (int rb = readback(&h, bad, sizeof(h), s)) return rb;
  *first_violation = h >= none ? -1 : (int64_t)h;
  return SCT_OK;
}

int sct_count_matrix_workspace_size(const sct_count_input_t* in, size_t* bytes) {
  last_error().clear();
  if (!in || !bytes) return fail(SCT_EINVAL, "NULL argument");
  *bytes = count_layout(in).total;
  return SCT_OK;
}

int sct_count_matrix(const sct_count_input_t* in, sct_count_output_t* out, void* workspace, size_t workspace_bytes,
                     void* stream) {
  last_error().clear();
  if (!in || !out) return fail(SCT_EINVAL, "NULL argument");
  out->n_rows = out->nnz = out->n_sorted = 0;
  out->unknown_record = -1;
  const int64_t n = in->n;
  if (n < 0 || n >= (int64_t)0x7FFFFFFF) return fail(SCT_EINVAL, "records must be in [0, 2^31 - 1)");
  if (in->n_cell_ids < 0 || in->n_umi_ids < 0 || in->n_gene_ids < 0 || in->n_cols < 0)
    return fail(SCT_EINVAL, "negative dictionary size");
  if (!out->indptr) return fail(SCT_EINVAL, "indptr is NULL");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    HIPCHK(hipMemsetAsync(out->indptr, 0, sizeof(int32_t), s));
    HIPCHK(hipStreamSynchronize(s));
    return SCT_OK;
  }
  if (!in->cell || !in->umi || !in->gene || !in->xf || !in->qhead || !in->gene_col || !out->row_cell ||
      !out->indices || !out->data)
    return fail(SCT_EINVAL, "NULL column");
  CountKey K;
  K.cbits = bitlen((uint64_t)in->n_cell_ids);
  K.colbits = bitlen((uint64_t)(in->n_cols > 0 ? in->n_cols : 1));
  K.ubits = bitlen((uint64_t)in->n_umi_ids);
  K.total = K.cbits + K.colbits + K.ubits;
  if (K.total > 63)
    return fail(SCT_EINVAL, "cell (%d) + column (%d) + molecule (%d) id bits exceed 63", K.cbits, K.colbits, K.ubits);
  const CountLayout L = count_layout(in);
  if (!workspace || workspace_bytes < L.total)
    return fail(SCT_ENOMEM, "workspace too small (%zu < %zu)", workspace_bytes, L.total);
  const int64_t nc = in->n_cell_ids;
  SortBuffers B{at<uint64_t>(workspace, L.ka), at<uint64_t>(workspace, L.kb), at<uint32_t>(workspace, L.va),
                at<uint32_t>(workspace, L.vb), at<uint32_t>(workspace, L.counts), at<uint32_t>(workspace, L.offsets),
                at<uint64_t>(workspace, L.sums), L.count_cap};
  uint32_t* fa = at<uint32_t>(workspace, L.flags_a);
  uint32_t* oa = at<uint32_t>(workspace, L.offs_a);
  uint32_t* fb = at<uint32_t>(workspace, L.flags_b);
  uint32_t* ob = at<uint32_t>(workspace, L.offs_b);
  int32_t* pair_cell = at<int32_t>(workspace, L.pair_cell);
  int32_t* pair_col = at<int32_t>(workspace, L.pair_col);
  uint32_t* pair_tri = at<uint32_t>(workspace, L.pair_tri);
  uint32_t* cell_first = at<uint32_t>(workspace, L.cell_first);
  uint32_t* cell_npairs = at<uint32_t>(workspace, L.cell_npairs);
  uint32_t* cell_pstart = at<uint32_t>(workspace, L.cell_pstart);
  uint32_t* row_of = at<uint32_t>(workspace, L.row_of);
  uint32_t* row_pairs = at<uint32_t>(workspace, L.row_pairs);
  // scalars: [0] unknown record, [1] kept groups, [2] pairs, [3] triples, [4] rows, [5] err
  uint64_t* sc = at<uint64_t>(workspace, L.scalars);
  HIPCHK(hipMemsetAsync(cell_first, 0xFF, sizeof(uint32_t) * (size_t)(nc ? nc : 1), s));
  HIPCHK(hipMemsetAsync(sc, 0xFF, sizeof(uint64_t), s));
  HIPCHK(hipMemsetAsync(sc + 1, 0, 5 * sizeof(uint64_t), s));
  CountCols c{in->cell, in->umi,     in->gene,       in->xf,         in->qhead,      in->gene_col, n,
              in->n_cell_ids, in->n_umi_ids, in->n_gene_ids, in->cell_none, in->umi_none, in->n_cols};
  // 1. molecule keys of the counted groups, compacted
  LAUNCH("count_groups", k_cm_groups, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), s, c, K, B.kb, fa, cell_first,
         (unsigned long long*)sc, (uint32_t*)(sc + 5));
  int rc = scan_counts(fa, n, oa, B.sums, s);
  if (rc) return rc;
  LAUNCH("count_compact", k_cm_compact, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), s, (const uint64_t*)B.kb,
         (const uint32_t*)fa, (const uint32_t*)oa, n, B.ka, B.va, sc + 1);
  uint64_t h[6];
  if (int rb = readback(h, sc, sizeof(h), s)) return rb;
  if (h[5]) return fail(SCT_EINVAL, "a dictionary id is outside its dictionary");
  if (h[0] != ~0ull) {
    out->unknown_record = (int64_t)h[0];
    return SCT_OK;
  }
  const int64_t m = (int64_t)h[1];
  out->n_sorted = m;
  int64_t nnz = 0, n_rows = 0;
  uint64_t n_triples = 0;
  if (m > 0) {
    // 2. sort; triples and (cell, column) pairs numbered by scans
    int which = 0;
    rc = radix_sort(B, m, K.total, &which, s);
    if (rc) return rc;
    const uint64_t* sorted = which ? B.kb : B.ka;
    const dim3 grid((unsigned)cdiv(m, kBlock));
    LAUNCH("count_heads", k_cm_heads, grid, dim3(kBlock), s, sorted, m, K, fa, fb);
    rc = scan_counts(fa, m, oa, B.sums, s);
    if (rc) return rc;
    rc = scan_counts(fb, m, ob, B.sums, s);
    if (rc) return rc;
    LAUNCH("count_emit", k_cm_emit, grid, dim3(kBlock), s, sorted, m, K, (const uint32_t*)fb, (const uint32_t*)ob,
           (const uint32_t*)fa, (const uint32_t*)oa, pair_cell, pair_col, pair_tri, cell_pstart, sc + 2);
    // 3. row order: counted cells by the record index of their first counted molecule
    LAUNCH("count_rowkeys", k_cm_rowkeys, dim3((unsigned)cdiv(nc, kBlock)), dim3(kBlock), s,
           (const uint32_t*)cell_first, (int32_t)nc, B.ka, B.va, sc + 4);
    if (int rb = readback(h, sc, sizeof(h), s)) return rb;
    nnz = (int64_t)h[2];
    n_triples = h[3];
    n_rows = (int64_t)h[4];
    LAUNCH("count_cells", k_cm_cells, dim3((unsigned)cdiv(nnz, kBlock)), dim3(kBlock), s, (const int32_t*)pair_cell,
           nnz, (const uint32_t*)cell_pstart, cell_npairs);
    rc = radix_sort(B, nc, 32, &which, s);
    if (rc) return rc;
    const uint32_t* cells = which ? B.vb : B.va;
    LAUNCH("count_rows", k_cm_rows, dim3((unsigned)cdiv(n_rows, kBlock)), dim3(kBlock), s, cells, n_rows,
           (const uint32_t*)cell_npairs, out->row_cell, row_of, row_pairs);
    rc = scan_counts(row_pairs, n_rows, (uint32_t*)out->indptr, B.sums, s);
    if (rc) return rc;
    LAUNCH("count_scatter", k_cm_scatter, dim3((unsigned)cdiv(nnz, kBlock)), dim3(kBlock), s, nnz, n_triples,
           (const int32_t*)pair_cell, (const int32_t*)pair_col, (const uint32_t*)pair_tri,
           (const uint32_t*)cell_pstart, (const uint32_t*)row_of, (const int32_t*)out->indptr, out->indices,
           out->data);
  }
  LAUNCH("count_tail", k_cm_set_tail, dim3(1), dim3(kWave), s, out->indptr, n_rows, nnz);
  HIPCHK(hipStreamSynchronize(s));
  out->n_rows = n_rows;
  out->nnz = nnz;
  return SCT_OK;
}

int sct_finalize_partials(int32_t mode, const int64_t* partials, int64_t rows, int64_t* out_ints, double* out_floats,
                          void* stream) {
  last_error().clear();
  if (mode < SCT_MODE_CELL || mode > SCT_MODE_GENE_GROUPED) return fail(SCT_EINVAL, "unknown mode %d", mode);
  if (rows < 0 || (rows > 0 && (!partials || !out_ints || !out_floats)))
    return fail(SCT_EINVAL, "bad finalize arguments");
  if (rows == 0) return SCT_OK;
  hipStream_t s = (hipStream_t)stream;
  LAUNCH("finalize", k_finalize, dim3((unsigned)cdiv(rows * kFinThreads, kBlock)), dim3(kBlock), s, partials, rows, (int)mode, 1,
         (const int64_t*)nullptr, out_ints, out_floats);
  return SCT_OK;
}

// ---- native TagSort metrics (tsmetrics.h) ----
static int ts_check_plan(const sct_plan_t* plan, int64_t* capacity) {
  if (!plan) return fail(SCT_EINVAL, "NULL plan");
  // the hash tables have the power of two >= 2 n slots, indexed with 32 bits
  if (plan->n_records < 0 || plan->n_records > (int64_t)1 << 30)
    return fail(SCT_EINVAL, "n_records %lld out of range [0, 2^30]", (long long)plan->n_records);
  if (plan->mode != SCT_MODE_CELL && plan->mode != SCT_MODE_GENE)
    return fail(SCT_EINVAL, "TagSort metrics: mode must be SCT_MODE_CELL or SCT_MODE_GENE, not %d", plan->mode);
  if (plan->n_cell_ids <= 0 || plan->n_gene_ids <= 0 || plan->n_umi_ids <= 0)
    return fail(SCT_EINVAL, "dictionary sizes must be positive");
  if (plan->max_entities < 0 || plan->max_entities > plan->n_records + 1)
    return fail(SCT_EINVAL, "capacity (max_entities) %lld outside [0, n_records + 1]", (long long)plan->max_entities);
  *capacity = plan->max_entities ? plan->max_entities : plan->n_records + 1;
  return SCT_OK;
}

int sct_tagsort_metrics_workspace_size(const sct_plan_t* plan, size_t* bytes) {
  int64_t capacity = 0;
  int rc = ts_check_plan(plan, &capacity);
  if (rc) return rc;
  if (!bytes) return fail(SCT_EINVAL, "bytes is NULL");
  *bytes = ts_layout(plan->n_records, plan->n_cell_ids, capacity).total;
  return SCT_OK;
}

int sct_tagsort_metrics(const sct_plan_t* plan, const sct_records_t* rec, const uint8_t* first_drop,
                        const uint8_t* third_is_mito, void* workspace, size_t workspace_bytes, int64_t* out_ints,
                        double* out_sums, int64_t* n_rows, void* stream) {
  last_error().clear();
  int64_t capacity = 0;
  int rc = ts_check_plan(plan, &capacity);
  if (rc) return rc;
  if (!rec || rec->n != plan->n_records) return fail(SCT_EINVAL, "records.n != plan.n_records");
  if (!first_drop || !out_ints || !out_sums || !n_rows) return fail(SCT_EINVAL, "NULL argument");
  const bool cell = plan->mode == SCT_MODE_CELL;
  if (cell && !third_is_mito) return fail(SCT_EINVAL, "third_is_mito is NULL");
  const int64_t n = rec->n;
  const TsLayout L = ts_layout(n, plan->n_cell_ids, capacity);
  if (!workspace || workspace_bytes < L.total)
    return fail(SCT_ENOMEM, "workspace too small (%zu < %zu)", workspace_bytes, L.total);
  hipStream_t s = (hipStream_t)stream;
  const size_t ne = (size_t)plan->n_cell_ids;
  TsEnt ent{at<int32_t>(workspace, L.start), at<int32_t>(workspace, L.end), at<int32_t>(workspace, L.fm),
            at<int32_t>(workspace, L.prev), at<int32_t>(workspace, L.rowbase)};
  TsCtl* ctl = at<TsCtl>(workspace, L.ctl);
  int32_t* row_start = at<int32_t>(workspace, L.row_start);
  uint4* xv = at<uint4>(workspace, L.xv);
  TsTable ft{at<uint32_t>(workspace, L.f_owner), at<uint32_t>(workspace, L.f_cnt), L.slots - 1};
  TsTable kt{at<uint32_t>(workspace, L.k_owner), at<uint32_t>(workspace, L.k_cnt), L.slots - 1};
  FillBatch fb;
  fb.add(ent.start, 4 * ne, 0xFF);
  fb.add(ent.end, 4 * ne, 0);
  fb.add(ent.fm, 4 * ne, 0x7F);
  fb.add(ctl, sizeof(TsCtl), 0xFF);
  fb.add(ft.owner, 4 * (size_t)L.slots, 0xFF);
  fb.add(ft.cnt, 4 * (size_t)L.slots, 0);
  fb.add(kt.owner, 4 * (size_t)L.slots, 0xFF);
  fb.add(kt.cnt, 4 * (size_t)L.slots, 0);
  rc = launch_fills(fb, s);
  if (rc) return rc;
  const unsigned rec_blocks = (unsigned)cdiv(n, kBlock);
  if (n > 0) {
    LAUNCH_N("ts_mark", n, k_ts_mark, dim3(rec_blocks), dim3(kBlock), s, *rec, n, (uint32_t)plan->n_cell_ids,
             (uint32_t)plan->n_umi_ids, (uint32_t)plan->n_gene_ids, first_drop, ent, ctl);
  }
  LAUNCH_N("ts_ent_scan", plan->n_cell_ids, k_ts_ent_scan, dim3(1), dim3(kTsScanBlock), s, ent, plan->n_cell_ids, ctl);
  TsCtl h;
  rc = readback(&h, ctl, sizeof(h), s);
  if (rc) return rc;
  if (h.bad_id != ~0ull) return fail(SCT_EINVAL, "record %llu has a tag id outside its dictionary", h.bad_id);
  if (h.unsorted != ~0ull)
    return fail(SCT_EINVAL, "records are not sorted by (first, second, third): record %llu is before its predecessor",
                h.unsorted);
  const int64_t rows = h.boundaries + 1;
  *n_rows = rows;
  if (rows > capacity)
    return fail(SCT_ENOMEM, "%lld rows exceed the capacity of %lld", (long long)rows, (long long)capacity);
  fb.add(out_ints, sizeof(int64_t) * SCT_TS_NI * (size_t)rows, 0);
  fb.add(out_sums, sizeof(double) * SCT_TS_NF * (size_t)rows, 0);
  rc = launch_fills(fb, s);
  if (rc) return rc;
  // the final row's name; the closed rows' names come from the records that close them
  HIPCHK(hipMemcpyAsync(&out_ints[(rows - 1) * SCT_TS_NI + SCT_TS_I_NAME], &ctl->last_mapped, sizeof(int64_t),
                        hipMemcpyDeviceToDevice, s));
  if (n > 0) {
    const unsigned slot_blocks = (unsigned)(L.slots / kBlock);
#define SCT_TS_RECORDS(C)                                                                                     \
  LAUNCH_N("ts_records", n, (k_ts_records<C>), dim3(rec_blocks), dim3(kBlock), s, *rec, n, first_drop, third_is_mito, \
           ent, row_start, ft, kt, xv, out_ints)
    SCT_VIEW2(cell, SCT_TS_RECORDS);
#undef SCT_TS_RECORDS
    LAUNCH_N("ts_frag_slots", L.slots, k_ts_frag_slots, dim3(slot_blocks), dim3(kBlock), s, *rec, ent, ft, out_ints);
#define SCT_TS_K1(C)                                                                                              \
  LAUNCH_N("ts_k1_slots", L.slots, (k_ts_k1_slots<C>), dim3(slot_blocks), dim3(kBlock), s, *rec, third_is_mito, ent, kt, \
           out_ints)
    SCT_VIEW2(cell, SCT_TS_K1);
#undef SCT_TS_K1
    LAUNCH_N("ts_chains", n, k_ts_chains, dim3((unsigned)rows), dim3(kWave), s, (const uint4*)xv, n, rows,
             (const int32_t*)row_start, out_sums);
  }
  HIPCHK(hipStreamSynchronize(s));
  return SCT_OK;
}

}  // extern "C"
