"""The device decoder's per-record rule in the metric modes (csrc/gbam_parse.h k_parse) and in count mode
(k_parse_count) on crafted records, against the host decoder (bamnative.decode): one small file per case, and
for every file what ``test_gbam.same_as_host`` asserts -- the host decoder accepts it and the device's columns
and names equal the host's exactly, or the host decoder raises and ``gbam.decode`` returns None.

Every record is well formed as BAM (its block_size is right, what it announces lies inside it, the file ends on
a record boundary): the cases probe the rule -- tag types, repeated tags, the quality strings, the CIGAR
trimming, the columns' widths, the query-name group head -- not the bounds checks."""
import struct

import numpy as np
import pytest

import test_gbam as TG
import test_tagsort_native_cpu as TC
from sctools_amd import bamnative, gbam
from test_gbam_tagsort import raw_record, write_raw

pytestmark = pytest.mark.gpu

CUG = ("CB", "UB", "GE")
MODES = ("cell", "gene")
Q10 = bytes([40, 31, 30, 2, 0, 41, 12, 35, 33, 30])
F32 = struct.pack("<f", 1.5)
ARRAY = b"Bi" + struct.pack("<iii", 2, 1, 2)


def rec(name, tags=TC.FULL, **kw):
    """TC._rec with real qualities (its default, 0xff bytes, is a case of its own here)."""
    l_seq = kw.get("l_seq", 10)
    kw.setdefault("qual", Q10 if l_seq == 10 else bytes([35]) * l_seq)
    if "cigar" not in kw and l_seq != 10:
        kw["cigar"] = ((0, l_seq),) if l_seq else ()
    return TC._rec(name, tags, **kw)


def blob(x) -> bytes:
    return x if isinstance(x, bytes) else raw_record(x)


def write_case(path, probes):
    """Two plain records, the case's records, one plain record."""
    write_raw(path, [blob(x) for x in [rec("good0"), rec("good1")] + list(probes) + [rec("good2")]])


def same_as_host(path, mode, tags=None):
    """test_gbam.same_as_host, for the modes that take tag names too."""
    kw = {} if tags is None else {"tags": tags}
    try:
        want = bamnative.decode(path, mode, **kw)
    except Exception as e:  # noqa: BLE001 -- the host decoder's error for this file
        want = e
    got = gbam.decode(path, mode, **kw)
    print(mode, tags, "host:", repr(want) if isinstance(want, Exception) else "accepts",
          "device:", "declines (%s)" % gbam.last_error() if got is None else "decodes")
    if isinstance(want, Exception):
        assert got is None, (path, mode, want)
        return None
    assert got is not None, (path, mode, gbam.last_error())
    cols, names = got
    arrays, want_names = want
    assert [list(x) for x in names] == [list(x) for x in want_names]
    for c in (gbam.COUNT_COLUMNS if mode == "count" else arrays):
        a = arrays[c]
        g = cols[c].cpu().numpy().view(a.dtype)
        assert np.array_equal(g, a), (path, mode, c, g, a)
    return cols


def typed(tag):
    """The tag as A, C, i, f and B (an int32 array)."""
    w = TC._without(tag)
    return [
        (tag + "_A", [raw_record(rec("t", w), back=tag.encode() + b"AX")]),
        (tag + "_C", [raw_record(rec("t", w), back=tag.encode() + b"C\x07")]),
        (tag + "_i", [rec("t", TC._without(**{tag: 7}))]),
        (tag + "_f", [raw_record(rec("t", w), back=tag.encode() + b"f" + F32)]),
        (tag + "_B", [raw_record(rec("t", w), back=tag.encode() + ARRAY)]),
    ]


TYPED = typed("CB") + typed("UB") + typed("GE")

# ---- the metric modes ----
TAG_CASES = TYPED + [
    # a name given twice: the last occurrence counts
    ("cb_twice", [raw_record(rec("t"), back=b"CBZGGGG\x00")]),
    ("cb_twice_front", [raw_record(rec("t"), front=b"CBZGGGG\x00")]),
    ("cb_then_typed", [raw_record(rec("t"), back=b"CBC\x07")]),
    ("typed_then_cb", [raw_record(rec("t"), front=b"CBC\x07")]),
    ("ge_twice_comma_last", [raw_record(rec("t"), back=b"GEZG1,G2\x00")]),
    ("ge_twice_comma_first", [raw_record(rec("t"), front=b"GEZG1,G2\x00")]),
    ("nh_twice", [raw_record(rec("t"), back=b"NHi" + struct.pack("<i", 5))]),
    ("nh_twice_front", [raw_record(rec("t"), front=b"NHi" + struct.pack("<i", 5))]),
    ("xf_twice", [raw_record(rec("t"), back=b"XFZUTR\x00")]),
    ("cy_twice_empty_last", [raw_record(rec("t"), back=b"CYZ\x00")]),
    ("uy_twice", [raw_record(rec("t"), back=b"UYZII\x00")]),
    ("cr_twice", [raw_record(rec("t"), back=b"CRZTTTT\x00")]),
    ("ur_twice", [raw_record(rec("t"), back=b"URZTTT\x00")]),
    # XF
    ("xf_coding", [rec("t", TC._without(XF="CODING"))]),
    ("xf_intronic", [rec("t", TC._without(XF="INTRONIC"))]),
    ("xf_utr", [rec("t", TC._without(XF="UTR"))]),
    ("xf_intergenic", [rec("t", TC._without(XF="INTERGENIC"))]),
    ("xf_all_four", [rec("t%d" % k, TC._without(XF=x)) for k, x in enumerate(("CODING", "INTRONIC", "UTR",
                                                                              "INTERGENIC"))]),
    ("xf_other", [rec("t", TC._without(XF="SOMETHING"))]),
    ("xf_prefix", [rec("t", TC._without(XF="CODIN")), rec("u", TC._without(XF="CODINGS"))]),
    ("xf_empty", [rec("t", TC._without(XF=""))]),
    ("xf_char", [raw_record(rec("t", TC._without("XF")), back=b"XFAC")]),
    ("xf_int", [rec("t", TC._without(XF=3))]),
    ("xf_absent", [rec("t", TC._without("XF"))]),
    # NH
    ("nh_C1", [raw_record(rec("t", TC._without("NH")), back=b"NHC\x01")]),
    ("nh_i1", [rec("t", TC._without(NH=1))]),
    ("nh_i2", [rec("t", TC._without(NH=2))]),
    ("nh_Z", [rec("t", TC._without(NH="1"))]),
    ("nh_f", [raw_record(rec("t", TC._without("NH")), back=b"NHf" + struct.pack("<f", 1.0))]),
    ("nh_missing", [rec("t", TC._without("NH"))]),
    # bytes the device does not intern
    ("cb_high_byte", [rec("t", TC._without(CB="AC\xe9T"))]),
    ("ub_high_byte", [rec("t", TC._without(UB="T\x80T"))]),
    ("ge_high_byte", [rec("t", TC._without(GE="G\xff"))]),
    ("cr_high_byte", [rec("t", TC._without(CR="AC\xe9T"))]),
]

QUALITY_TAG_CASES = [
    ("cy_missing", [rec("t", TC._without("CY"))]),
    ("cy_empty", [rec("t", TC._without(CY=""))]),
    ("cy_int", [rec("t", TC._without(CY=3))]),
    ("cb_without_cr", [rec("t", TC._without("CR"))]),
    ("no_cb_no_cr", [rec("t", TC._without("CB", "CR"))]),
    ("cr_equals_cb", [rec("t", TC._without(CR="ACGT"))]),
    ("cr_differs_from_cb", [rec("t", TC._without(CR="ACGA"))]),
    ("cr_longer_than_cb", [rec("t", TC._without(CR="ACGTA"))]),
    ("cr_int", [rec("t", TC._without(CR=5))]),
    ("ur_equals_ub", [rec("t", TC._without(UR="TTT"))]),
    ("ur_int", [rec("t", TC._without(UR=5))]),
    ("ub_missing", [rec("t", TC._without("UB"))]),
    ("ge_missing", [rec("t", TC._without("GE"))]),
    ("cy_255", [rec("t", TC._without(CY="I" * 255))]),
    ("cy_256", [rec("t", TC._without(CY="I" * 256))]),
    ("uy_255", [rec("t", TC._without(UY="I" * 255))]),
    ("uy_256", [rec("t", TC._without(UY="I" * 256))]),
    ("cy_uy_threshold_bytes", [rec("t", TC._without(CY="?@A\x7f!", UY="@?~ "))]),
]
for _gene, _ge in (("one_gene", "G1"), ("comma_gene", "G1,G2")):
    QUALITY_TAG_CASES += [
        ("uy_missing_" + _gene, [rec("t", TC._without("UY", GE=_ge))]),
        ("uy_empty_" + _gene, [rec("t", TC._without(UY="", GE=_ge))]),
        ("uy_int0_" + _gene, [rec("t", TC._without(UY=0, GE=_ge))]),
        ("uy_int5_" + _gene, [rec("t", TC._without(UY=5, GE=_ge))]),
        ("uy_C0_" + _gene, [raw_record(rec("t", TC._without("UY", GE=_ge)), back=b"UYC\x00")]),
        ("uy_float_" + _gene, [rec("t", TC._without(UY=0.0, GE=_ge))]),
        ("uy_256_" + _gene, [rec("t", TC._without(UY="I" * 256, GE=_ge))]),
    ]

Q12 = bytes([40, 40, 40, 10, 10, 10, 10, 10, 35, 35, 31, 30])
CIGAR_CASES = [
    ("soft_clips_both_ends", [rec("t", l_seq=12, qual=Q12, cigar=((4, 3), (0, 7), (4, 2)))]),
    ("soft_clip_leading", [rec("t", l_seq=12, qual=Q12, cigar=((4, 3), (0, 9)))]),
    ("soft_clip_trailing", [rec("t", l_seq=12, qual=Q12, cigar=((0, 10), (4, 2)))]),
    ("two_soft_clips_leading", [rec("t", l_seq=12, qual=Q12, cigar=((4, 1), (4, 2), (0, 9)))]),
    ("hard_clip_leading", [rec("t", l_seq=12, qual=Q12, cigar=((5, 4), (0, 12)))]),
    ("hard_clip_trailing", [rec("t", l_seq=12, qual=Q12, cigar=((0, 12), (5, 4)))]),
    ("hard_then_soft_both_ends", [rec("t", l_seq=12, qual=Q12, cigar=((5, 4), (4, 3), (0, 7), (4, 2), (5, 1)))]),
    ("hard_after_soft_leading", [rec("t", l_seq=12, qual=Q12, cigar=((4, 3), (5, 4), (0, 9)))]),
    ("hard_before_soft_trailing", [rec("t", l_seq=12, qual=Q12, cigar=((0, 10), (5, 4), (4, 2)))]),
    ("hard_after_full_soft", [rec("t", l_seq=12, qual=Q12, cigar=((4, 12), (5, 4)))]),
    ("only_soft_clip", [rec("t", l_seq=12, qual=Q12, cigar=((4, 12),))]),
    ("only_two_soft_clips", [rec("t", l_seq=12, qual=Q12, cigar=((4, 5), (4, 7)))]),
    ("only_hard_clips", [rec("t", l_seq=12, qual=Q12, cigar=((5, 5), (5, 7)))]),
    ("soft_clips_crossing", [rec("t", l_seq=12, qual=Q12, cigar=((4, 8), (0, 1), (4, 8)))]),
    ("no_cigar", [rec("t", l_seq=12, qual=Q12, cigar=())]),
    ("n_zero", [rec("t", cigar=((0, 5), (3, 0), (0, 5)))]),
    ("n_real", [rec("t", cigar=((0, 5), (3, 700), (0, 5)))]),
    ("n_first_op", [rec("t", cigar=((3, 9), (0, 10)))]),
]

RECORD_CASES = [
    ("l_seq_0", [rec("t", l_seq=0)]),
    ("qual_all_ff", [rec("t", qual=b"\xff" * 10)]),
    ("qual_first_ff", [rec("t", qual=b"\xff" + Q10[1:])]),
    ("qual_second_ff", [rec("t", qual=Q10[:1] + b"\xff" + Q10[2:])]),
    ("unmapped_no_xf_nh", [rec("t", TC._without("XF", "NH"), flag=0x4)]),
    ("unmapped_flag_ref_set", [rec("t", flag=0x4, ref=2)]),
    ("ref_none_flag_clear", [rec("t", flag=0, ref=-1, pos=-1)]),
    ("mapped_no_xf_nh", [rec("t", TC._without("XF", "NH"))]),
    ("mapped_no_xf_nh_comma_gene", [rec("t", TC._without("XF", "NH", GE="G1,G2"))]),
    ("mapped_no_xf", [rec("t", TC._without("XF"))]),
    ("reverse", [rec("t", flag=0x10)]),
    ("duplicate", [rec("t", flag=0x400)]),
    ("reverse_duplicate_unmapped", [rec("t", flag=0x10 | 0x400 | 0x4)]),
    ("qual_sum_ffff", [rec("t", l_seq=258, qual=bytes([0]) + bytes([255]) * 257)]),
    ("qual_sum_10000", [rec("t", l_seq=258, qual=bytes([1]) + bytes([255]) * 257)]),
    ("aligned_len_ffff", [rec("t", l_seq=0xffff, qual=bytes([1]) * 0xffff)]),
    ("aligned_len_10000", [rec("t", l_seq=0x10000, qual=bytes(0x10000))]),
    ("aligned_len_ffff_of_10001", [rec("t", l_seq=0x10001, qual=bytes(0x10001), cigar=((4, 2), (0, 0xffff)))]),
]

METRIC_CASES = TAG_CASES + QUALITY_TAG_CASES + CIGAR_CASES + RECORD_CASES
assert len({c[0] for c in METRIC_CASES}) == len(METRIC_CASES)

# Files the host decoder accepts and the device declines on purpose (gbam.decode returns None and the caller
# decodes on the host): an integer dictionary value, which the host decoder keys by its str(), and a dictionary
# byte >= 0x80, which the device does not rank.  Asserted exactly, not by same_as_host.
DECLINED = {t + k for t in CUG for k in ("_C", "_i")} | {"cb_then_typed", "cb_for_two_roles_typed", "cb_high_byte",
                                                           "ub_high_byte", "ge_high_byte"}


def declined_by_design(path, mode, tags=None):
    """The host decoder accepts the file; the device declines it at the parse, for a record."""
    kw = {} if tags is None else {"tags": tags}
    arrays, _ = bamnative.decode(path, mode, **kw)
    assert len(arrays["cell"]) == 4
    assert gbam.decode(path, mode, **kw) is None
    assert gbam.last_error() == "a record needs the host decoder"


def check(case, path, mode, tags=None):
    (declined_by_design if case[0] in DECLINED else same_as_host)(path, mode, tags)


def params(cases):
    return [pytest.param(c, id=c[0]) for c in cases]


@pytest.mark.parametrize("mode", MODES)
def test_plain_records_decode(mode, tmp_path):
    """The records every case file is built around are themselves decoded on the device."""
    path = str(tmp_path / "plain.bam")
    write_case(path, [])
    assert same_as_host(path, mode) is not None


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", params(METRIC_CASES))
def test_metric_record(case, mode, tmp_path):
    path = str(tmp_path / "case.bam")
    write_case(path, case[1])
    check(case, path, mode)


# ---- count mode ----
def named(*names, tags=TC.FULL):
    return [rec(n, tags) for n in names]


COUNT_CASES = [(n, r, CUG) for n, r in TYPED] + [
    ("cb_for_two_roles", [rec("t")], ("CB", "CB", "GE")),
    ("cb_for_two_roles_typed", [rec("t", TC._without(CB=7))], ("CB", "CB", "GE")),
    ("raw_tags", [rec("t")], ("CR", "UR", "GE")),
    ("xf_as_a_role", [rec("t")], ("CB", "UB", "XF")),
    ("cb_twice", [raw_record(rec("t"), back=b"CBZGGGG\x00")], CUG),
    ("cb_then_typed", [raw_record(rec("t"), back=b"CBC\x07")], CUG),
    ("typed_then_cb", [raw_record(rec("t"), front=b"CBC\x07")], CUG),
    ("cb_missing", [rec("t", TC._without("CB"))], CUG),
    ("all_three_missing", [rec("t", TC._without("CB", "UB", "GE"))], CUG),
    ("cb_high_byte", [rec("t", TC._without(CB="AC\xe9T"))], CUG),
    ("xf_intergenic", [rec("t", TC._without(XF="INTERGENIC"))], CUG),
    ("xf_other", [rec("t", TC._without(XF="INTRONIC")), rec("u", TC._without(XF="INTERGENI"))], CUG),
    ("xf_char", [raw_record(rec("t", TC._without("XF")), back=b"XFAI")], CUG),
    ("xf_int", [rec("t", TC._without(XF=4))], CUG),
    ("xf_absent", [rec("t", TC._without("XF"))], CUG),
    ("xf_twice", [raw_record(rec("t", TC._without(XF="INTERGENIC")), back=b"XFZUTR\x00")], CUG),
    ("name_of_one_byte", named("", "", "a"), CUG),
    ("equal_names", named("qa", "qa", "qa"), CUG),
    ("equal_names_as_neighbours", named("good1", "good1", "good2"), CUG),
    ("last_byte_differs", named("qa", "qb", "qb", "qa"), CUG),
    ("first_byte_differs", named("aq", "bq"), CUG),
    ("lengths_differ", named("qa", "qab", "qa", "q", "qa"), CUG),
    ("no_tags_no_cigar", [rec("t", {}, l_seq=0), rec("t", {}, l_seq=0)], CUG),
]
assert len({c[0] for c in COUNT_CASES}) == len(COUNT_CASES)


def test_plain_records_decode_in_count_mode(tmp_path):
    path = str(tmp_path / "plain.bam")
    write_case(path, [])
    cols = same_as_host(path, "count", CUG)
    assert cols is not None and cols["qhead"].tolist() == [1, 1, 1]


@pytest.mark.parametrize("case", params(COUNT_CASES))
def test_count_record(case, tmp_path):
    path = str(tmp_path / "case.bam")
    write_case(path, case[1])
    check(case, path, "count", case[2])


def test_count_head_flag_across_windows(tmp_path, monkeypatch):
    """Query-name groups of one to three records in members of 997 bytes and windows of 6000: window after
    window begins inside a group, at a group's head, or with a name one byte off the carried record's."""
    names = []
    for g in range(90):
        names += ["g%02d%s" % (g // 2, "ab"[g % 2])] * (1 + g % 3)
    one = str(tmp_path / "one.bam")
    write_raw(one, [raw_record(rec(n, TC._without(CB="ACG" + "ACGT"[k % 4]))) for k, n in enumerate(names)])
    path = str(tmp_path / "windows.bam")
    TG.rebgzf(TG.payload(one), path, level=6, block=997)
    monkeypatch.setenv("SCT_GBAM_WINDOW_BYTES", "6000")
    t = {}
    assert gbam.decode(path, "count", tags=CUG, timings=t) is not None, gbam.last_error()
    assert t["windows"] >= 3, t
    cols = same_as_host(path, "count", CUG)
    want = [1] + [int(a != b) for a, b in zip(names, names[1:])]
    assert cols["qhead"].tolist() == want and 1 < sum(want) < len(want)


def test_cases_are_well_formed(tmp_path):
    """Every crafted record announces what it holds: the lengths in its fixed part and in its tags add up to
    its block_size exactly."""
    for name, probes, *_ in METRIC_CASES + COUNT_CASES:
        for x in probes:
            b = blob(x)
            bs, = struct.unpack_from("<i", b, 0)
            assert bs == len(b) - 4, name
            lrn, n_cigar, l_seq = b[12], struct.unpack_from("<H", b, 16)[0], struct.unpack_from("<i", b, 20)[0]
            assert lrn >= 1 and b[36 + lrn - 1] == 0, name
            q = 36 + lrn + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
            while q < len(b):
                t = chr(b[q + 2])
                q += 3
                if t in "ZH":
                    q = b.index(b"\x00", q) + 1
                elif t == "B":
                    assert chr(b[q]) == "i", name
                    q += 5 + 4 * struct.unpack_from("<i", b, q + 1)[0]
                else:
                    q += {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}[t]
            assert q == len(b), name
