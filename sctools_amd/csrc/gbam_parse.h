// gbam_parse.h -- records to columns.  On the device: a tag's value (DTag, tag_value), the pieces the three
// parse kernels share -- a record's fields (Rec, rec_open), the three dictionary keys interned (intern_keys),
// XF's code (xf_code), a row stored (Row, store) -- and the kernels themselves, each with its own walk over the
// tags (a shared one cost registers, scratch memory or time: DESIGN.md section 16) and its own mode's rule:
// k_parse (the cell and gene metric modes), k_parse_count (the count matrix), k_parse_tagsort (the native
// TagSort).  On the host: the columns bound from the caller's pointers, pass 2 over the windows
// (parse_windows) and the three modes' entry points.
#pragma once
#include "gbam_dict.h"
#include "gbam_starts.h"
#include "gbam_util.h"
#include "gbam_window.h"

namespace gb {

// bits / xf codes: include/sctools_gpu.h, sctools_amd/columnar.py
enum : uint32_t {
  B_UNMAPPED = 1u << 0, B_REVERSE = 1u << 1, B_DUPLICATE = 1u << 2, B_SPLICED = 1u << 3, B_NH1 = 1u << 4,
  B_PERFECT_UMI = 1u << 5, B_HAS_CB = 1u << 6, B_PERFECT_CB = 1u << 7
};
enum : uint32_t { XF_ABSENT = 0, XF_CODING, XF_INTRONIC, XF_UTR, XF_INTERGENIC, XF_OTHER };
enum : uint32_t { TV_NONE = 0, TV_STR = 1, TV_INT = 2, TV_RAW = 3 };

struct DTag {
  uint32_t kind;  // TV_*
  uint64_t off;   // value bytes in U (strings)
  uint32_t n;     // string length
  int64_t i;      // integer value
};

__device__ __forceinline__ bool str_eq(const uint8_t* U, uint64_t a, uint64_t b, uint32_t n) {
  for (uint32_t k = 0; k < n; k++)
    if (U[a + k] != U[b + k]) return false;
  return true;
}
// Python == of two present tag values where at least one is a string
__device__ __forceinline__ bool val_eq_str(const uint8_t* U, const DTag& a, const DTag& b) {
  return a.kind == TV_STR && b.kind == TV_STR && a.n == b.n && str_eq(U, a.off, b.off, a.n);
}
__device__ __forceinline__ bool lit_eq(const uint8_t* U, uint64_t off, uint32_t n, const char* s, uint32_t sn) {
  if (n != sn) return false;
  for (uint32_t k = 0; k < n; k++)
    if (U[off + k] != (uint8_t)s[k]) return false;
  return true;
}
// the code of an XF string (the metric modes' and TagSort's four alignment locations)
__device__ __forceinline__ uint32_t xf_code(const uint8_t* U, uint64_t off, uint32_t n) {
  if (lit_eq(U, off, n, "CODING", 6)) return XF_CODING;
  if (lit_eq(U, off, n, "INTRONIC", 8)) return XF_INTRONIC;
  if (lit_eq(U, off, n, "UTR", 3)) return XF_UTR;
  if (lit_eq(U, off, n, "INTERGENIC", 10)) return XF_INTERGENIC;
  return XF_OTHER;
}

// bytes of a tag value of type t at U[p..end) (bgzf.h read_tag), 0 = unknown type or truncated
__device__ uint32_t tag_value(const uint8_t* U, uint64_t p, uint64_t end, uint32_t t, DTag* v) {
  const uint64_t room = end > p ? end - p : 0;
  uint32_t w = 0;
  switch (t) {
    case 'Z':
    case 'H': {
      uint64_t q = p;
      while (q < end && U[q]) q++;
      if (q >= end) return 0;
      if (v) v->kind = TV_STR, v->off = p, v->n = (uint32_t)(q - p);
      return (uint32_t)(q - p + 1);
    }
    case 'A':
      if (room < 1) return 0;
      if (v) v->kind = TV_STR, v->off = p, v->n = 1;
      return 1;
    case 'c': case 'C': w = 1; break;
    case 's': case 'S': w = 2; break;
    case 'i': case 'I': case 'f': w = 4; break;
    case 'd': w = 8; break;
    case 'B': {
      if (room < 5) return 0;
      const uint32_t sub = U[p];
      const uint32_t ew = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2
                        : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
      if (!ew) return 0;
      const uint64_t len = 5 + (uint64_t)u32(U, p + 1) * ew;
      if (len > room) return 0;
      if (v) v->kind = TV_RAW, v->off = p, v->n = 0;
      return (uint32_t)len;
    }
    default:
      return 0;
  }
  if (w > room) return 0;
  if (v) {
    v->off = p, v->n = 0;
    switch (t) {
      case 'c': v->kind = TV_INT, v->i = (int8_t)U[p]; break;
      case 'C': v->kind = TV_INT, v->i = U[p]; break;
      case 's': v->kind = TV_INT, v->i = (int16_t)u16(U, p); break;
      case 'S': v->kind = TV_INT, v->i = u16(U, p); break;
      case 'i': v->kind = TV_INT, v->i = (int32_t)u32(U, p); break;
      case 'I': v->kind = TV_INT, v->i = u32(U, p); break;
      default: v->kind = TV_RAW; break;
    }
  }
  return w;
}

// ---------------- the pieces the three kernels share ----------------
// A record's fixed fields and where its parts lie in U (SAM/BAM spec 4.2).
struct Rec {
  uint64_t d, end;  // its data (after block_size) and one past it
  uint32_t l_read_name, n_cigar, flag, l_seq;
  uint64_t cig, qual, tag0;  // the CIGAR operations, the qualities, the first tag
  int32_t ref, pos;
};
// false: the record does not hold what it announces (before any loop bounded by its fields)
__device__ __forceinline__ bool rec_open(const uint8_t* U, const uint64_t* __restrict__ starts, uint64_t r, Rec* R) {
  const uint64_t p = starts[r];
  const uint32_t bs = u32(U, p);
  const uint64_t d = p + 4;
  R->d = d;
  R->end = d + bs;
  if (bs < 32) return false;
  R->ref = (int32_t)u32(U, d), R->pos = (int32_t)u32(U, d + 4);
  R->l_read_name = U[d + 8];
  R->n_cigar = u16(U, d + 12), R->flag = u16(U, d + 14);
  R->l_seq = u32(U, d + 16);
  R->cig = d + 32 + R->l_read_name;
  R->qual = R->cig + 4ull * R->n_cigar + (R->l_seq + 1ull) / 2;
  R->tag0 = R->qual + R->l_seq;
  return R->tag0 <= R->end;
}

// Key k's string U[off[k], off[k] + n[k]) interned where has[k], else flags[1 + k] raised (some record lacks
// the tag: the dictionary gets its None); ids[k] the slot, -1 without.  true: a string the device does not
// intern (the host decoder takes the file).
__device__ __forceinline__ bool intern_keys(const Dicts& D, uint32_t* __restrict__ flags, const uint8_t* U,
                                            const bool has[3], const uint64_t off[3], const uint32_t n[3],
                                            int32_t ids[3]) {
  bool host = false;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    ids[k] = -1;
    if (has[k]) host |= (ids[k] = intern(D, k, U, off[k], n[k])) < 0;
    else atomicOr(&flags[1 + k], 1u);
  }
  return host;
}

struct Cols {
  int32_t *cell, *umi, *gene, *ref, *pos;
  uint16_t *gq_sum, *gq_len, *gq_gt30;
  uint8_t *bits, *xf, *cy_gt30, *cy_len, *uy_gt30, *uy_len;
};
struct Row {  // one record's values, in the columns' order
  int32_t cell, umi, gene, ref, pos;
  uint32_t gq_sum, gq_len, gq_gt30, bits, xf, cy_gt30, cy_len, uy_gt30, uy_len;
};
__device__ __forceinline__ void store(const Cols& C, uint64_t r, const Row& w) {
  C.cell[r] = w.cell, C.umi[r] = w.umi, C.gene[r] = w.gene;
  C.ref[r] = w.ref, C.pos[r] = w.pos;
  C.gq_sum[r] = (uint16_t)w.gq_sum, C.gq_len[r] = (uint16_t)w.gq_len, C.gq_gt30[r] = (uint16_t)w.gq_gt30;
  C.bits[r] = (uint8_t)w.bits, C.xf[r] = (uint8_t)w.xf;
  C.cy_gt30[r] = (uint8_t)w.cy_gt30, C.cy_len[r] = (uint8_t)w.cy_len;
  C.uy_gt30[r] = (uint8_t)w.uy_gt30, C.uy_len[r] = (uint8_t)w.uy_len;
}

// ---------------- the metric modes ----------------
// One lane per record: bamdec.cpp parse_record (same checks, same order of outcomes); any
// record the host would reject or key differently sets *host.
__global__ void k_parse(const uint8_t* __restrict__ U, const uint64_t* __restrict__ starts, uint64_t n,
                        uint32_t is_cell, Cols C, Dicts D, uint32_t* __restrict__ flags) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  bool host = false;
  do {
    Rec R;
    if (!rec_open(U, starts, r, &R)) { host = true; break; }
    const uint32_t n_cigar = R.n_cigar, l_seq = R.l_seq;
    const uint64_t cig = R.cig, qual = R.qual;
    DTag cb{}, cr{}, cy{}, ub{}, ur{}, uy{}, ge{}, xf{}, nh{};
    // a name given twice: its last value counts
    uint64_t q = R.tag0;
    while (q + 3 <= R.end) {
      const uint32_t ab = (uint32_t)U[q] << 8 | U[q + 1], t = U[q + 2];
      q += 3;
      DTag v{};
      const uint32_t used = tag_value(U, q, R.end, t, &v);
      if (!used) { host = true; break; }
      q += used;
      if (ab == ('C' << 8 | 'B')) cb = v;
      else if (ab == ('C' << 8 | 'R')) cr = v;
      else if (ab == ('C' << 8 | 'Y')) cy = v;
      else if (ab == ('U' << 8 | 'B')) ub = v;
      else if (ab == ('U' << 8 | 'R')) ur = v;
      else if (ab == ('U' << 8 | 'Y')) uy = v;
      else if (ab == ('G' << 8 | 'E')) ge = v;
      else if (ab == ('X' << 8 | 'F')) xf = v;
      else if (ab == ('N' << 8 | 'H')) nh = v;
    }
    if (host) break;
    // dictionary values other than strings are keyed by the host path
    if ((cb.kind && cb.kind != TV_STR) || (ub.kind && ub.kind != TV_STR) || (ge.kind && ge.kind != TV_STR)) {
      host = true;
      break;
    }
    bool validate = is_cell;
    if (!is_cell) {
      bool comma = false;
      for (uint32_t k = 0; k < ge.n && ge.kind; k++) comma |= U[ge.off + k] == ',';
      validate = !comma;
    }
    uint32_t bits = 0, cg = 0, cl = 0, ug = 0, ul = 0;
    if (is_cell) {
      if (cy.kind != TV_STR || cy.n == 0) { host = true; break; }
      for (uint32_t k = 0; k < cy.n; k++) cg += U[cy.off + k] > 63;
      cl = cy.n;
      if (cb.kind) {
        bits |= B_HAS_CB;
        if (!cr.kind) { host = true; break; }
        if (val_eq_str(U, cr, cb)) bits |= B_PERFECT_CB;
      }
    } else if (cb.kind) {
      bits |= B_HAS_CB;
    }
    bool do_uy = validate;
    if (!validate && uy.kind) {
      if (uy.kind == TV_STR) do_uy = uy.n > 0;
      else if (uy.kind == TV_INT && uy.i != 0) { host = true; break; }
    }
    if (do_uy) {
      if (uy.kind != TV_STR || uy.n == 0) { host = true; break; }
      for (uint32_t k = 0; k < uy.n; k++) ug += U[uy.off + k] > 63;
      ul = uy.n;
    }
    if (ur.kind && ub.kind && val_eq_str(U, ur, ub)) bits |= B_PERFECT_UMI;
    const bool aq_none = l_seq == 0 || U[qual] == 0xff;
    uint32_t q0 = 0, q1 = 0;
    if (!aq_none) {
      uint32_t start = 0;
      for (uint32_t k = 0; k < n_cigar; k++) {
        const uint32_t c = u32(U, cig + 4ull * k), op = c & 0xf, len = c >> 4;
        if (op == 5) {
          if (start != 0 && start != l_seq) { host = true; break; }
        } else if (op == 4) {
          start += len;
        } else {
          break;
        }
      }
      if (host) break;
      uint32_t qend = l_seq;
      for (int k = (int)n_cigar - 1; k > 0; k--) {
        const uint32_t c = u32(U, cig + 4ull * k), op = c & 0xf, len = c >> 4;
        if (op == 5) {
          if (qend != l_seq) { host = true; break; }
        } else if (op == 4) {
          qend -= len;
        } else {
          break;
        }
      }
      if (host) break;
      q0 = start;
      q1 = qend < start ? start : qend;
    }
    if (validate && (aq_none || q1 == q0)) { host = true; break; }
    uint32_t x = XF_ABSENT;
    if (xf.kind) x = xf.kind == TV_STR ? xf_code(U, xf.off, xf.n) : XF_OTHER;
    if (R.flag & 0x4) {
      bits |= B_UNMAPPED;
    } else {
      if (validate && (!xf.kind || !nh.kind)) { host = true; break; }
      if (nh.kind == TV_INT && nh.i == 1) bits |= B_NH1;
      uint64_t n_len = 0;
      for (uint32_t k = 0; k < n_cigar; k++) {
        const uint32_t c = u32(U, cig + 4ull * k);
        if ((c & 0xf) == 3) n_len += c >> 4;
      }
      if (n_len) bits |= B_SPLICED;
    }
    if (R.flag & 0x10) bits |= B_REVERSE;
    if (R.flag & 0x400) bits |= B_DUPLICATE;
    uint32_t s = 0, g = 0;
    for (uint32_t k = q0; k < q1; k++) {
      const uint32_t v = U[qual + k];
      s += v;
      g += v > 30;
    }
    if (q1 - q0 > 0xffff || s > 0xffff || cl > 0xff || ul > 0xff) { host = true; break; }
    const bool has[3] = {cb.kind != 0, ub.kind != 0, ge.kind != 0};
    const uint64_t off[3] = {cb.off, ub.off, ge.off};
    const uint32_t len[3] = {cb.n, ub.n, ge.n};
    int32_t ids[3];
    host = intern_keys(D, flags, U, has, off, len, ids);
    if (host) break;
    store(C, r, Row{ids[0], ids[1], ids[2], R.ref, R.pos, s, q1 - q0, g, bits, x, cg, cl, ug, ul});
  } while (false);
  if (host) atomicOr(&flags[0], 1u);
}

// ---------------- count mode ----------------
// One lane per record: bamdec.cpp parse_count_record (count.py:222-270 reads the three named
// dictionary tags, XF and the query name; no validation) plus the itertools.groupby head flag of
// count.py:83-86 -- the record's query name differs from the previous record's.  tags: the
// three tag names as (a << 8 | b).
struct CountCols {
  int32_t *cell, *umi, *gene;
  uint8_t *xf, *qhead;
};
// has_prev: starts[-1] is the previous window's last record (the query-name comparison of record 0)
__global__ void k_parse_count(const uint8_t* __restrict__ U, const uint64_t* __restrict__ starts, uint64_t n,
                              uint32_t tcb, uint32_t tub, uint32_t tge, CountCols C, Dicts D,
                              uint32_t* __restrict__ flags, uint32_t has_prev) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  bool host = false;
  do {
    Rec R;
    if (!rec_open(U, starts, r, &R) || R.l_read_name == 0) { host = true; break; }
    DTag cb{}, ub{}, ge{}, xf{};
    // its last value counts; not else-if: a tag name may be given for two roles, as on the host
    uint64_t q = R.tag0;
    while (q + 3 <= R.end) {
      const uint32_t a = U[q], b = U[q + 1], t = U[q + 2];
      q += 3;
      DTag v{};
      const uint32_t used = tag_value(U, q, R.end, t, &v);
      if (!used) { host = true; break; }
      q += used;
      const uint32_t ab = a << 8 | b;
      if (ab == tcb) cb = v;
      if (ab == tub) ub = v;
      if (ab == tge) ge = v;
      if (ab == ('X' << 8 | 'F')) xf = v;
    }
    if (host) break;
    if ((cb.kind && cb.kind != TV_STR) || (ub.kind && ub.kind != TV_STR) || (ge.kind && ge.kind != TV_STR)) {
      host = true;  // integer / float / array values: the host's str() of them, or its ETYPED
      break;
    }
    uint32_t x = XF_ABSENT;  // (the count matrix asks one thing of XF: is it INTERGENIC)
    if (xf.kind) x = xf.kind == TV_STR && lit_eq(U, xf.off, xf.n, "INTERGENIC", 10) ? XF_INTERGENIC : XF_OTHER;
    uint32_t head = 1;
    if (r || has_prev) {
      const uint64_t pp = starts[r - 1] + 4, p = R.d - 4;
      const uint32_t lrn = R.l_read_name;
      // the previous record's name lies before this record (a malformed previous record sets
      // *host on its own lane, and then head is not used)
      if (U[pp + 8] == lrn && pp + 32 + lrn <= p) head = !str_eq(U, pp + 32, R.d + 32, lrn - 1);
    }
    const bool has[3] = {cb.kind != 0, ub.kind != 0, ge.kind != 0};
    const uint64_t off[3] = {cb.off, ub.off, ge.off};
    const uint32_t len[3] = {cb.n, ub.n, ge.n};
    int32_t ids[3];
    host = intern_keys(D, flags, U, has, off, len, ids);
    if (host) break;
    C.cell[r] = ids[0], C.umi[r] = ids[1], C.gene[r] = ids[2];
    C.xf[r] = (uint8_t)x, C.qhead[r] = (uint8_t)head;
  } while (false);
  if (host) atomicOr(&flags[0], 1u);
}

// ---------------- TagSort mode ----------------
// bamdec.cpp parse_tagsort_record; htslib_tagsort.cpp:106-218.  A tag's FIRST
// occurrence (bam_aux_get), kept as an offset from the record's data: st 0 not seen, 1 a Z / H
// string, 2 any other type (get_Ztag_or_default then reads it as missing).
struct TsTag {
  uint32_t off, n, st;
};
__device__ __forceinline__ void ts_first(TsTag& dst, uint32_t off, uint32_t n, uint32_t st) {
  if (!dst.st) dst.off = off, dst.n = n, dst.st = st;
}
// a string tag as get_Ztag_or_default gives it: another type and the value "-" are the default
__device__ __forceinline__ bool ts_present(const uint8_t* U, uint64_t d, const TsTag& v) {
  return v.st == 1 && !(v.n == 1 && U[d + v.off] == '-');
}
// strcmp(tag or "None", raw or "") == 0 (a Z value holds no NUL, so its length is its strlen)
__device__ __forceinline__ bool ts_perfect(const uint8_t* U, uint64_t d, bool has_tag, const TsTag& tag, bool has_raw,
                                           const TsTag& raw) {
  const uint32_t an = has_tag ? tag.n : 4, bn = has_raw ? raw.n : 0;
  if (an != bn) return false;
  if (has_tag) return str_eq(U, d + tag.off, d + raw.off, bn);
  const char none[4] = {'N', 'o', 'n', 'e'};
  for (uint32_t k = 0; k < bn; k++)
    if (U[d + raw.off + k] != (uint8_t)none[k]) return false;
  return true;
}

// Whole-read quality sums, 16 lanes per record: lane group g (lanes 16g .. 16g + 15 of the wave)
// takes the records of its own 16 lanes one after the other, every lane one aligned 8-byte word of
// the quality bytes [q0, q0 + len) per step (U is a hipMalloc pointer, so a payload offset that is
// a multiple of 8 is an aligned address).  The bytes of a word outside the range are masked off;
// a word reaching past the resident payload (ulen) is not loaded: its bytes before ulen are read
// one by one.  All 64 lanes call it (len 0: nothing to read); lane l returns its own record's
// sum and count of bytes > 30.
__device__ __forceinline__ void ts_quality(const uint8_t* __restrict__ U, uint64_t ulen, uint64_t qoff, uint32_t qlen,
                                           uint32_t* sum, uint32_t* gt30) {
  const uint32_t sub = threadIdx.x & 15;
  uint32_t my_s = 0, my_g = 0;
  for (uint32_t it = 0; it < 16; it++) {
    const uint32_t lo = __shfl((uint32_t)qoff, (int)it, 16), hi = __shfl((uint32_t)(qoff >> 32), (int)it, 16);
    const uint32_t len = __shfl(qlen, (int)it, 16);
    const uint64_t q0 = (uint64_t)hi << 32 | lo, q1 = q0 + len;
    uint32_t s = 0, g = 0;
    for (uint64_t w = (q0 & ~7ull) + 8ull * sub; w < q1; w += 128) {
      uint64_t x = 0;
      if (w + 8 <= ulen) {
        x = *reinterpret_cast<const uint64_t*>(U + w);
      } else {
        for (uint32_t j = 0; j < 8 && w + j < ulen; j++) x |= (uint64_t)U[w + j] << (8 * j);
      }
      const uint32_t a = q0 > w ? (uint32_t)(q0 - w) : 0;       // first byte of the word in range: 0..7
      const uint32_t b = q1 - w < 8 ? (uint32_t)(q1 - w) : 8;   // one past the last: 1..8
      uint64_t m = ~0ull << (8 * a);
      if (b < 8) m &= (1ull << (8 * b)) - 1;
      x &= m;
      s = __builtin_amdgcn_sad_u8((uint32_t)x, 0u, s);
      s = __builtin_amdgcn_sad_u8((uint32_t)(x >> 32), 0u, s);
      // byte > 30: bit 7 of (low seven bits + 97), or the byte's own bit 7
      const uint64_t t = (((x & 0x7f7f7f7f7f7f7f7full) + 0x6161616161616161ull) | x) & 0x8080808080808080ull;
      g += __popcll(t);
    }
    for (int o = 8; o > 0; o >>= 1) {
      s += __shfl_xor(s, o, 16);
      g += __shfl_xor(g, o, 16);
    }
    if (sub == it) my_s = s, my_g = g;
  }
  *sum = my_s, *gt30 = my_g;
}

// One lane per record's tags and fields, 16 lanes per record's qualities.  tcb / tub / tge: the
// barcode, umi and gene tag names as (a << 8 | b); ulen: the resident payload's length.  Every
// record agrees with parse_tagsort_record or sets flags[0] (the host decoder takes the file).
__global__ void k_parse_tagsort(const uint8_t* __restrict__ U, uint64_t ulen, const uint64_t* __restrict__ starts,
                                uint64_t n, uint32_t tcb, uint32_t tub, uint32_t tge, Cols C, Dicts D,
                                uint32_t* __restrict__ flags) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool host = false, ok = false;
  Rec R{};
  if (r < n) {
    ok = rec_open(U, starts, r, &R) && R.l_seq <= 0xffff;  // ... and within the columns' width
    host = !ok;
  }
  uint32_t s = 0, g = 0;
  ts_quality(U, ulen, ok ? R.qual : 0, ok ? R.l_seq : 0, &s, &g);  // (the whole wave: no lane has left)
  if (ok) do {
    const uint64_t d = R.d;
    TsTag cb{}, ub{}, ge{}, cr{}, cy{}, ur{}, uy{}, xf{};
    uint32_t nh = 0;  // 1: the first NH is an integer 1; 2: it is anything else
    // a name given twice: its first value counts
    uint64_t q = R.tag0;
    while (q + 3 <= R.end) {
      const uint32_t ab = (uint32_t)U[q] << 8 | U[q + 1], t = U[q + 2];
      q += 3;
      DTag v{};
      const uint32_t used = tag_value(U, q, R.end, t, &v);
      if (!used) { host = true; break; }
      const uint32_t voff = (uint32_t)(q - d), st = t == 'Z' || t == 'H' ? 1 : 2;
      q += used;
      // each role on its own: a named tag may itself be CR or UR
      if (ab == tcb) ts_first(cb, voff, v.n, st);
      if (ab == tub) ts_first(ub, voff, v.n, st);
      if (ab == tge) ts_first(ge, voff, v.n, st);
      if (ab == ('C' << 8 | 'R')) ts_first(cr, voff, v.n, st);
      if (ab == ('C' << 8 | 'Y')) ts_first(cy, voff, v.n, st);
      if (ab == ('U' << 8 | 'R')) ts_first(ur, voff, v.n, st);
      if (ab == ('U' << 8 | 'Y')) ts_first(uy, voff, v.n, st);
      if (ab == ('X' << 8 | 'F')) ts_first(xf, voff, v.n, st);
      if (ab == ('N' << 8 | 'H') && !nh) nh = v.kind == TV_INT && v.i == 1 ? 1 : 2;
    }
    if (host) break;
    if (cb.st == 2 || ub.st == 2 || ge.st == 2) { host = true; break; }  // bam_aux2Z of a typed value: the host's ETYPED
    const bool has_cb = ts_present(U, d, cb), has_ub = ts_present(U, d, ub), has_ge = ts_present(U, d, ge);
    const bool has_cr = ts_present(U, d, cr), has_ur = ts_present(U, d, ur);
    uint32_t bits = 0, cg = 0, cl = 0, ug = 0, ul = 0;
    if (has_cb) bits |= B_HAS_CB;
    if (ts_perfect(U, d, has_cb, cb, has_cr, cr)) bits |= B_PERFECT_CB;
    if (ts_perfect(U, d, has_ub, ub, has_ur, ur)) bits |= B_PERFECT_UMI;
    if (ts_present(U, d, cy)) {
      cl = cy.n;
      if (cl > 0xff) { host = true; break; }
      for (uint32_t k = 0; k < cl; k++) cg += (uint8_t)(U[d + cy.off + k] - 33) > 30;  // uint8_t: below 33 wraps
    }
    if (ts_present(U, d, uy)) {
      ul = uy.n;
      if (ul > 0xff) { host = true; break; }
      for (uint32_t k = 0; k < ul; k++) ug += (int)U[d + uy.off + k] - 33 > 30;  // int: below 33 does not count
    }
    uint32_t x = XF_ABSENT;
    if (ts_present(U, d, xf) && xf.n > 0) x = xf_code(U, d + xf.off, xf.n);
    if (R.ref == -1) bits |= B_UNMAPPED;  // (the flag's 0x4 is not read)
    if (nh == 1) bits |= B_NH1;
    for (uint32_t k = 0; k < R.n_cigar; k++) {
      const uint32_t c = u32(U, R.cig + 4ull * k);
      if ((c & 0xf) == 3 && (c >> 4) != 0) {
        bits |= B_SPLICED;
        break;
      }
    }
    if (R.flag & 0x10) bits |= B_REVERSE;
    if (R.flag & 0x400) bits |= B_DUPLICATE;
    if (s > 0xffff) { host = true; break; }
    const bool has[3] = {has_cb, has_ub, has_ge};
    const uint64_t off[3] = {d + cb.off, d + ub.off, d + ge.off};
    const uint32_t len[3] = {cb.n, ub.n, ge.n};
    int32_t ids[3];
    host = intern_keys(D, flags, U, has, off, len, ids);
    if (host) break;
    store(C, r, Row{ids[0], ids[1], ids[2], R.ref, R.pos, s, R.l_seq, g, bits, x, cg, cl, ug, ul});
  } while (false);
  if (host) atomicOr(&flags[0], 1u);
}

}  // namespace gb

// ---------------- host ----------------
namespace {

// the caller's column pointers, in the order of include/sct_gbam.h; and the columns from record `base` on
Cols cols_from(void* const* c) {
  Cols C;
  C.cell = (int32_t*)c[0], C.umi = (int32_t*)c[1], C.gene = (int32_t*)c[2];
  C.ref = (int32_t*)c[3], C.pos = (int32_t*)c[4];
  C.gq_sum = (uint16_t*)c[5], C.gq_len = (uint16_t*)c[6], C.gq_gt30 = (uint16_t*)c[7];
  C.bits = (uint8_t*)c[8], C.xf = (uint8_t*)c[9], C.cy_gt30 = (uint8_t*)c[10];
  C.cy_len = (uint8_t*)c[11], C.uy_gt30 = (uint8_t*)c[12], C.uy_len = (uint8_t*)c[13];
  return C;
}
Cols at(const Cols& C, uint64_t base) {
  Cols W = C;
  W.cell += base, W.umi += base, W.gene += base, W.ref += base, W.pos += base;
  W.gq_sum += base, W.gq_len += base, W.gq_gt30 += base, W.bits += base, W.xf += base;
  W.cy_gt30 += base, W.cy_len += base, W.uy_gt30 += base, W.uy_len += base;
  return W;
}
CountCols count_cols_from(void* const* c) {
  CountCols C;
  C.cell = (int32_t*)c[0], C.umi = (int32_t*)c[1], C.gene = (int32_t*)c[2];
  C.xf = (uint8_t*)c[3], C.qhead = (uint8_t*)c[4];
  return C;
}
CountCols at(const CountCols& C, uint64_t base) {
  CountCols W = C;
  W.cell += base, W.umi += base, W.gene += base, W.xf += base, W.qhead += base;
  return W;
}
// tag name k of the six characters a mode is given, as the kernels compare it: (a << 8 | b)
uint32_t tag_code(const char* tags, int k) { return (uint32_t)(uint8_t)tags[2 * k] << 8 | (uint8_t)tags[2 * k + 1]; }

int parse_flags(sct_gbam* G, ParseState& P) {
  HIPOK(hipGetLastError());
  HIPOK(hipMemcpyAsync(P.fl, P.flags.p, sizeof(P.fl), hipMemcpyDeviceToHost, G->st));
  HIPOK(hipStreamSynchronize(G->st));
  if (P.fl[0]) return gfail(SCT_GBAM_HOST, "a record needs the host decoder");
  return SCT_BAM_OK;
}

// Pass 2 over the windows: `launch(w, starts of its parsed records, count, has_prev)` parses one
// window's records into the columns at w.base.
template <class Launch>
int parse_windows(sct_gbam* G, ParseState& P, int32_t* const colk[3], Launch launch) {
  if (G->kept) {
    const double t0 = now();
    launch(G->win[0], G->starts.p, (uint64_t)G->n, false);
    const int rc = parse_flags(G, P);
    G->t[sct_gbam::T_PARSE_INTERN] = now() - t0;
    return rc;
  }
  DevBuf<uint64_t> starts;
  for (WinInfo& w : G->win) {
    uint64_t total = 0;
    int rc = restart_window(G, w, starts, &total);
    if (rc) return rc;
    const double t0 = now();
    rc = ensure_tables(G, P, colk, w.base, w.n_rec);
    if (rc) return rc;
    const uint64_t skip = w.has_prev ? 1 : 0;
    if (w.n_rec) launch(w, starts.p + skip, w.n_rec, w.has_prev);
    rc = parse_flags(G, P);
    if (rc) return rc;
    rc = promote(G, P);
    if (rc) return rc;
    G->t[sct_gbam::T_PARSE_INTERN] += now() - t0;
  }
  G->in.free();
  return SCT_BAM_OK;
}

int parse_impl(sct_gbam* G, int32_t metric_mode, void* const* cols) {
  ParseState P;
  int rc = parse_begin(G, P);
  if (rc) return rc;
  const Cols C = cols_from(cols);
  int32_t* const colk[3] = {C.cell, C.umi, C.gene};
  const uint32_t is_cell = metric_mode == SCT_BAM_CELL_METRICS ? 1u : 0u;
  rc = parse_windows(G, P, colk, [&](const WinInfo& w, const uint64_t* starts, uint64_t n, bool) {
    hipLaunchKernelGGL(k_parse, dim3(grid(n, 256)), dim3(256), 0, G->st, G->u.p, starts, n, is_cell, at(C, w.base),
                       P.D, P.flags.p);
  });
  if (rc) return rc;
  return dictionaries_impl(G, P, colk);
}

int parse_count_impl(sct_gbam* G, const char* tags, void* const* cols) {
  ParseState P;
  int rc = parse_begin(G, P);
  if (rc) return rc;
  const CountCols C = count_cols_from(cols);
  int32_t* const colk[3] = {C.cell, C.umi, C.gene};
  rc = parse_windows(G, P, colk, [&](const WinInfo& w, const uint64_t* starts, uint64_t n, bool has_prev) {
    hipLaunchKernelGGL(k_parse_count, dim3(grid(n, 256)), dim3(256), 0, G->st, G->u.p, starts, n, tag_code(tags, 0),
                       tag_code(tags, 1), tag_code(tags, 2), at(C, w.base), P.D, P.flags.p, has_prev ? 1u : 0u);
  });
  if (rc) return rc;
  return dictionaries_impl(G, P, colk);
}

int parse_tagsort_impl(sct_gbam* G, const char* tags, void* const* cols) {
  ParseState P;
  int rc = parse_begin(G, P);
  if (rc) return rc;
  const Cols C = cols_from(cols);
  int32_t* const colk[3] = {C.cell, C.umi, C.gene};
  rc = parse_windows(G, P, colk, [&](const WinInfo& w, const uint64_t* starts, uint64_t n, bool) {
    hipLaunchKernelGGL(k_parse_tagsort, dim3(grid(n, 256)), dim3(256), 0, G->st, G->u.p, w.ulen, starts, n,
                       tag_code(tags, 0), tag_code(tags, 1), tag_code(tags, 2), at(C, w.base), P.D, P.flags.p);
  });
  if (rc) return rc;
  return dictionaries_impl(G, P, colk);
}

}  // namespace
