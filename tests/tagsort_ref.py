"""
Python restatements of the reference's native TagSort, written from its source
(``fastqpreprocessing/src``), for the tests of ``sctools_amd.tagsort``:

``read_fields``     the per-read stage (``htslib_tagsort.cpp:106-218``) of one BAM record;
``gather``          the gatherer (``metricgatherer.cpp:152-231``, ``tagsort.cpp:210-273``) and its
                    output (``metricgatherer.cpp:101-150, 278-325, 355-365``) over sorted reads;
``lines_of``        the 17-field text lines the reference's per-read stage writes for such reads.

``gather`` is checked byte for byte against CSVs recorded from the reference's own gatherer
(``tests/golden/tagsort_native``), which is what lets the GPU tests trust it on random input.  The
text round trip of the float32 ratios is glibc's own (``tests/native/tsround.cpp``).
"""
import ctypes
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = os.path.join(HERE, "golden", "tagsort_native")

INT_FIELDS = ("pos", "strand", "cy_gt30", "cy_len", "gq_sum", "gq_len", "gq_gt30", "nh", "perfect_umi", "spliced",
              "dup", "perfect_cb", "uy_gt30", "uy_len")
STR_FIELDS = ("first", "second", "third", "ref", "xf")

_lib = None


def tsround_lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(os.path.join(HERE, "native", "libtsround.so"))
        _lib.ts_roundtrip_pairs.restype = ctypes.c_int
        _lib.ts_roundtrip_pairs.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int64] + [ctypes.c_void_p] * 2
    return _lib


def roundtrip(num, den):
    """(ts_roundtrip bits, glibc bits): uint32 arrays of the float32 patterns for the integer pairs."""
    a = np.ascontiguousarray(num, dtype=np.uint32)
    b = np.ascontiguousarray(den, dtype=np.uint32)
    got, want = np.empty_like(a), np.empty_like(a)
    tsround_lib().ts_roundtrip_pairs(a.ctypes.data, b.ctypes.data, a.size, got.ctypes.data, want.ctypes.data)
    return got, want


def seen_value(num, den):
    """strtof(sprintf("%g", float32(num) / float32(den))) by glibc, as float64 arrays."""
    return roundtrip(num, den)[1].view(np.float32).astype(np.float64)


def g6(num, den) -> str:
    """``operator<<(float)`` of the float32 quotient: what the per-read stage writes."""
    with np.errstate(all="ignore"):
        q = np.float32(num) / np.float32(den)
    if q != q:
        return "-nan"  # 0 / 0 on x86
    return "%g" % float(q)


# ---------------------------------------------------------------------------------------------
# per read (htslib_tagsort.cpp:106-218)
# ---------------------------------------------------------------------------------------------
def read_fields(rec, tags=("CB", "UB", "GE")):
    """The fields of one record (``query_name``, ``flag``, ``reference_id``, ``pos``, ``cigar`` [(op, len)],
    ``l_seq``, ``_qual`` bytes or None, ``_tags`` dict) as the integer columns of the 32-byte record."""
    def ztag(key, default):
        v = rec._tags.get(key)
        if not isinstance(v, str) or v == "-":
            return default
        return v

    barcode, umi, gene = (ztag(t, None) for t in tags)
    cr, cy, ur, uy, xf = ztag("CR", ""), ztag("CY", ""), ztag("UR", ""), ztag("UY", ""), ztag("XF", "")
    qual = rec._qual if rec._qual is not None else b"\xff" * rec.l_seq
    nh = rec._tags.get("NH")
    return {
        "barcode": barcode, "umi": umi, "gene": gene,
        "perfect_cb": int((barcode if barcode is not None else "None") == cr),
        "perfect_umi": int((umi if umi is not None else "None") == ur),
        "cy_gt30": sum(((ord(c) - 33) & 0xFF) > 30 for c in cy), "cy_len": len(cy),
        "uy_gt30": sum((ord(c) - 33) > 30 for c in uy), "uy_len": len(uy),
        "xf": xf, "nh1": int(isinstance(nh, int) and nh == 1),
        "mapped": int(rec.reference_id != -1), "ref": rec.reference_id, "pos": rec.pos,
        "strand": int(bool(rec.flag & 0x10)), "dup": int(bool(rec.flag & 0x400)),
        "spliced": int(any(op == 3 and ln != 0 for op, ln in rec.cigar)),
        "gq_sum": sum(qual), "gq_len": rec.l_seq, "gq_gt30": sum(q > 30 for q in qual),
    }


# ---------------------------------------------------------------------------------------------
# lines (what the per-read stage writes, htslib_tagsort.cpp: the 17 tab-separated fields)
# ---------------------------------------------------------------------------------------------
def lines_of(c):
    """The text lines of reads given as columns (STR_FIELDS: lists of str, ``ref`` "*" for an unmapped
    read; INT_FIELDS: ints; ``nh`` is the NH value, -1 when missing)."""
    out = []
    for k in range(len(c["first"])):
        out.append("\t".join([
            c["first"][k], c["second"][k], c["third"][k], c["ref"][k], c["xf"][k], str(c["pos"][k]),
            str(c["strand"][k]), "0", g6(c["cy_gt30"][k], c["cy_len"][k]), g6(c["gq_sum"][k], c["gq_len"][k]),
            g6(c["gq_gt30"][k], c["gq_len"][k]), str(c["nh"][k]), str(c["perfect_umi"][k]), str(c["spliced"][k]),
            str(c["dup"][k]), str(c["perfect_cb"][k]), g6(c["uy_gt30"][k], c["uy_len"][k])]))
    return out


# ---------------------------------------------------------------------------------------------
# the gatherer
# ---------------------------------------------------------------------------------------------
class _Stat:  # OnlineGaussianSufficientStatistic (metricgatherer.h:17-58)
    def __init__(self):
        self.count, self.sum, self.sum2 = 0.0, 0.0, 0.0

    def update(self, x):
        self.count += 1.0
        self.sum += x
        self.sum2 += x * x

    def mean(self):
        return self.sum / self.count if self.count else float("nan")

    def variance(self):
        if self.count < 2:
            return -1.0
        return self.sum2 / (self.count - 1) - (self.sum / self.count) * (self.sum / (self.count - 1))


def _p10(x) -> str:  # ostream << setprecision(10)
    x = float(x)
    if x != x:
        return "-nan"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    return "%.10g" % x


def _to_nan(x) -> str:
    with np.errstate(all="ignore"):
        f = np.float32(x)
    return "nan" if f == np.float32(-1) else _p10(float(f))


def _per(a, b) -> str:
    if b == 0:
        return "-1"
    with np.errstate(all="ignore"):
        return _p10(float(np.float32(a) / np.float32(b)))


COMMON = ("n_reads,noise_reads,perfect_molecule_barcodes,reads_mapped_exonic,reads_mapped_intronic,reads_mapped_utr,"
          "reads_mapped_uniquely,reads_mapped_multiple,duplicate_reads,spliced_reads,antisense_reads,"
          "molecule_barcode_fraction_bases_above_30_mean,molecule_barcode_fraction_bases_above_30_variance,"
          "genomic_reads_fraction_bases_quality_above_30_mean,genomic_reads_fraction_bases_quality_above_30_variance,"
          "genomic_read_quality_mean,genomic_read_quality_variance,n_molecules,n_fragments,reads_per_molecule,"
          "reads_per_fragment,fragments_per_molecule,fragments_with_single_read_evidence,"
          "molecules_with_single_read_evidence")
CELL = ("perfect_cell_barcodes,reads_mapped_intergenic,reads_unmapped,reads_mapped_too_many_loci,"
        "cell_barcode_fraction_bases_above_30_variance,cell_barcode_fraction_bases_above_30_mean,n_genes,"
        "genes_detected_multiple_observations,n_mitochondrial_genes,n_mitochondrial_molecules,"
        "pct_mitochondrial_molecules")
GENE = "number_cells_detected_multiple,number_cells_expressing"


def gather(c, metric_type, mito=frozenset()):
    """The metrics CSV of sorted reads.  ``c``: ``first`` / ``second`` / ``third`` (str), ``ref`` (any hashable,
    "*" for an unmapped read), ``xf`` (str), the INT_FIELDS, all sequences of one length."""
    n = len(c["first"])
    x_cy = seen_value(c["cy_gt30"], c["cy_len"]).tolist()
    x_gq = seen_value(c["gq_sum"], c["gq_len"]).tolist()
    x_gqf = seen_value(c["gq_gt30"], c["gq_len"]).tolist()
    x_uy = seen_value(c["uy_gt30"], c["uy_len"]).tolist()
    cell = metric_type == "cell"
    out = ["," + COMMON + "," + (CELL if cell else GENE) + "\n"]
    st = {}

    def clear():
        st.update(n_reads=0, frag={}, mol={}, uy=_Stat(), perfect_umi=0, gqf=_Stat(), gq=_Stat(), exonic=0,
                  intronic=0, utr=0, unique=0, multiple=0, dup=0, spliced=0, cy=_Stat(), perfect_cb=0,
                  intergenic=0, unmapped=0, k1={})

    def emit(name):
        mol, frag = st["mol"], st["frag"]
        f = [name, str(st["n_reads"]), "0", str(st["perfect_umi"]), str(st["exonic"]), str(st["intronic"]),
             str(st["utr"]), str(st["unique"]), str(st["multiple"]), str(st["dup"]), str(st["spliced"]), "0",
             _p10(st["uy"].mean()), _to_nan(st["uy"].variance()), _p10(st["gqf"].mean()),
             _to_nan(st["gqf"].variance()), _to_nan(st["gq"].mean()), _to_nan(st["gq"].variance()),
             str(len(mol)), str(len(frag)), _per(st["n_reads"], len(mol)), _per(st["n_reads"], len(frag)),
             _per(len(frag), len(mol)), str(sum(v == 1 for v in frag.values())),
             str(sum(v == 1 for v in mol.values()))]
        k1 = st["k1"]
        multi = sum(v > 1 for v in k1.values())
        if cell:
            n_mito_genes = sum(g in mito for g in k1)
            n_mito = sum(v for g, v in k1.items() if g in mito)
            pct = 0.0
            if n_mito > 0:
                pct = (n_mito // sum(k1.values())) * 100.0
            f += [str(st["perfect_cb"]), str(st["intergenic"]), str(st["unmapped"]), "0",
                  _to_nan(st["cy"].variance()), _p10(st["cy"].mean()), str(len(k1)), str(multi), str(n_mito_genes),
                  str(n_mito), _p10(pct)]
        else:
            f += [str(multi), str(len(k1))]
        out.append(",".join(f) + "\n")

    clear()
    prev = ""
    first, second, third = c["first"], c["second"], c["third"]
    for k in range(n):
        cur = first[k]
        if cur == "None":
            continue
        if not cell and "," in cur:
            continue
        tags = cur + "-" + second[k] + "-" + third[k]
        if prev != cur and prev != "":
            emit(prev)
            clear()
        st["n_reads"] += 1
        st["mol"][tags] = st["mol"].get(tags, 0) + 1
        st["uy"].update(x_uy[k])
        st["perfect_umi"] += c["perfect_umi"][k]
        st["gqf"].update(x_gqf[k])
        st["gq"].update(x_gq[k])
        if cell:
            st["cy"].update(x_cy[k])
            st["perfect_cb"] += c["perfect_cb"][k]
            xf = c["xf"][k]
            if xf != "":
                if xf == "INTERGENIC":
                    st["intergenic"] += 1
            else:
                st["unmapped"] += 1
            st["k1"][third[k]] = st["k1"].get(third[k], 0) + 1
        else:
            st["k1"][second[k]] = st["k1"].get(second[k], 0) + 1
        if c["ref"][k] == "*":
            continue
        key = (c["ref"][k], c["pos"][k], c["strand"][k] == 1, tags)
        st["frag"][key] = st["frag"].get(key, 0) + 1
        xf = c["xf"][k]
        if xf == "CODING":
            st["exonic"] += 1
        elif xf == "INTRONIC":
            st["intronic"] += 1
        elif xf == "UTR":
            st["utr"] += 1
        if c["nh"][k] == 1:
            st["unique"] += 1
        else:
            st["multiple"] += 1
        st["dup"] += c["dup"][k]
        st["spliced"] += c["spliced"][k]
        prev = cur
    emit(prev)
    return "".join(out)


# ---------------------------------------------------------------------------------------------
# fixtures and engine columns
# ---------------------------------------------------------------------------------------------
def case_names():
    return sorted(f[:-5] for f in os.listdir(FIXTURES) if f.endswith(".json"))


def load_case(name):
    with open(os.path.join(FIXTURES, name + ".json")) as f:
        return json.load(f)


def recorded(name, metric_type):
    """The CSV recorded from the reference's gatherer, or None when the case has none for this type."""
    p = os.path.join(FIXTURES, "%s.%s.csv" % (name, metric_type))
    if not os.path.exists(p):
        return None
    with open(p, newline="") as f:
        return f.read()


XF_CODE = {"": 0, "CODING": 1, "INTRONIC": 2, "UTR": 3, "INTERGENIC": 4}


def engine_arrays(c):
    """(arrays, names): the reads as the decoder's ``tagsort`` mode would give them, with the first / second /
    third strings in the barcode / umi / gene role (so ``tag_order`` is the default) and dictionaries in
    sorted order with no missing entry ("None" is a string like any other here)."""
    n = len(c["first"])
    arrays, names = {}, []
    for col, key in (("cell", "first"), ("umi", "second"), ("gene", "third")):
        uniq = sorted(set(c[key]), key=lambda s: s.encode())
        idx = {s: i for i, s in enumerate(uniq)}
        arrays[col] = np.fromiter((idx[s] for s in c[key]), dtype=np.int32, count=n)
        names.append(uniq)
    refs = sorted(set(r for r in c["ref"] if r != "*"), key=str)
    ridx = {r: i for i, r in enumerate(refs)}
    arrays["ref"] = np.fromiter((ridx.get(r, -1) if r != "*" else -1 for r in c["ref"]), dtype=np.int32, count=n)
    arrays["pos"] = np.asarray(c["pos"], dtype=np.int32).reshape(n)
    bits = np.zeros(n, dtype=np.uint8)
    bits |= np.fromiter((r == "*" for r in c["ref"]), dtype=np.uint8, count=n) * np.uint8(0x01)
    bits |= (np.asarray(c["strand"], dtype=np.uint8).reshape(n) & 1) * np.uint8(0x02)
    bits |= (np.asarray(c["dup"], dtype=np.uint8).reshape(n) & 1) * np.uint8(0x04)
    bits |= (np.asarray(c["spliced"], dtype=np.uint8).reshape(n) & 1) * np.uint8(0x08)
    bits |= (np.asarray(c["nh"]).reshape(n) == 1).astype(np.uint8) * np.uint8(0x10)
    bits |= (np.asarray(c["perfect_umi"], dtype=np.uint8).reshape(n) & 1) * np.uint8(0x20)
    bits |= (np.asarray(c["perfect_cb"], dtype=np.uint8).reshape(n) & 1) * np.uint8(0x80)
    arrays["bits"] = bits
    arrays["xf"] = np.fromiter((XF_CODE.get(x, 5) for x in c["xf"]), dtype=np.uint8, count=n)
    for k in ("gq_sum", "gq_len", "gq_gt30"):
        arrays[k] = np.asarray(c[k], dtype=np.uint16).reshape(n)
    for k in ("cy_gt30", "cy_len", "uy_gt30", "uy_len"):
        arrays[k] = np.asarray(c[k], dtype=np.uint8).reshape(n)
    return arrays, names


def stable_sorted(c):
    """The reads in the reference's order: by (first, second, third) as byte strings, ties in input order."""
    n = len(c["first"])
    order = sorted(range(n), key=lambda k: (c["first"][k].encode(), c["second"][k].encode(), c["third"][k].encode()))
    return {k: [v[i] for i in order] for k, v in c.items()}


def columns_from_arrays(arrays, names, roles=("barcode", "umi", "gene")):
    """Decoder-style arrays (ids into ``names``: barcode, umi, gene dictionaries, ``None`` = a missing tag)
    as the gatherer's columns with the roles in (first, second, third) position; input order kept."""
    by_role = {"barcode": ("cell", 0), "umi": ("umi", 1), "gene": ("gene", 2)}
    n = len(arrays["cell"])
    c = {}
    for slot, role in zip(("first", "second", "third"), roles):
        col, which = by_role[role]
        strings = ["None" if s is None else s for s in names[which]]
        c[slot] = [strings[i] for i in np.asarray(arrays[col]).tolist()]
    bits = np.asarray(arrays["bits"]).astype(np.int64)
    c["ref"] = ["*" if b & 1 else int(r) for b, r in zip(bits.tolist(), np.asarray(arrays["ref"]).tolist())]
    rev = {v: k for k, v in XF_CODE.items()}
    c["xf"] = [rev.get(int(x), "OTHER") for x in np.asarray(arrays["xf"]).tolist()]
    c["pos"] = np.asarray(arrays["pos"]).tolist()
    c["strand"] = ((bits >> 1) & 1).tolist()
    c["dup"] = ((bits >> 2) & 1).tolist()
    c["spliced"] = ((bits >> 3) & 1).tolist()
    c["nh"] = np.where((bits >> 4) & 1, 1, -1).tolist()
    c["perfect_umi"] = ((bits >> 5) & 1).tolist()
    c["perfect_cb"] = ((bits >> 7) & 1).tolist()
    for k in ("gq_sum", "gq_len", "gq_gt30", "cy_gt30", "cy_len", "uy_gt30", "uy_len"):
        c[k] = np.asarray(arrays[k]).astype(np.int64).tolist()
    assert n == len(c["first"])
    return c
