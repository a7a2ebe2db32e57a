"""sctools_amd.barcode / sctools_amd.encodings on the host (no GPU).

The expectations under tests/golden/barcode/ were written by the reference's own classes
(tests/golden/make_barcode_golden.py): ``corrections.json.gz`` holds, per whitelist, the answer of
the reference's error dict for every query (null = KeyError), ``pair_stats.json`` its base
frequencies, diversity and TwoBit samples.  ``get_corrected_barcode`` is answered from the host
index here and must agree on every query; the GPU path is held to the same file in
test_gpu_barcode.py.
"""
import ctypes
import gzip
import json
import os
import random
import re
import warnings
from collections import OrderedDict

import numpy as np
import pytest

import bamwriter
from sctools_amd import bam, bamnative, barcode
from sctools_amd.encodings import TwoBit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "barcode")
WHITELISTS = ["1k-august-2016.txt", "crafted_L8.txt", "crafted_L5_nonewline.txt", "crafted_L21.txt"]
CORRECTIONS = json.load(gzip.open(os.path.join(GOLD, "corrections.json.gz"), "rt"))
STATS = json.load(open(os.path.join(GOLD, "pair_stats.json")))


def from_whitelist(name):
    return barcode.ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(os.path.join(GOLD, name))


@pytest.mark.parametrize("name", WHITELISTS)
def test_get_corrected_barcode_equals_the_reference_on_every_query(name):
    m = from_whitelist(name)
    assert len(CORRECTIONS[name]) > 400
    wrong = []
    for query, expected in CORRECTIONS[name]:
        try:
            got = m.get_corrected_barcode(query)
        except KeyError:
            got = None
        if got != expected:
            wrong.append((query, expected, got))
    assert not wrong, wrong[:10]


def test_fixture_covers_the_ambiguous_cases():
    # whitelist entries corrected to a later neighbour, N queries, and misses
    lines = [ln[:-1] for ln in open(os.path.join(GOLD, "crafted_L8.txt"))]
    pairs = CORRECTIONS["crafted_L8.txt"]
    assert sum(1 for q, c in pairs if q in lines and c is not None and c != q) >= 20
    assert len(lines) != len(set(lines))  # duplicate lines
    assert any("N" in q and c is not None for q, c in pairs)
    assert any(c is None for q, c in pairs)


def test_constructor_type_error():
    with pytest.raises(TypeError):
        barcode.ErrorsToCorrectBarcodesMap(["ACGT"])
    with pytest.raises(TypeError):
        barcode.ErrorsToCorrectBarcodesMap("ACGT")
    with pytest.raises(TypeError):
        barcode.Barcodes(["ACGT"], 4)


def test_mapping_is_used_as_given():
    given = OrderedDict([("AAAA", "AAAA"), ("AAAC", "AAAA"), ("anything", "else")])
    m = barcode.ErrorsToCorrectBarcodesMap(given)
    assert m.get_corrected_barcode("AAAC") == "AAAA"
    assert m.get_corrected_barcode("anything") == "else"
    with pytest.raises(KeyError):
        m.get_corrected_barcode("AAAG")  # not derived: the mapping is a dict, not a whitelist
    with pytest.raises(TypeError):
        m.correct_barcodes(np.zeros((1, 4), dtype=np.uint8))


def test_unterminated_last_line_loses_its_base(tmp_path):
    p = tmp_path / "wl.txt"
    p.write_text("ACGTA\nTTTTT\nGGGCC")
    m = barcode.ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(str(p))
    assert m.whitelist == ["ACGTA", "TTTTT", "GGGC"]
    assert m.barcode_length == 5
    assert m.get_corrected_barcode("GGGC") == "GGGC"
    with pytest.raises(KeyError):
        m.get_corrected_barcode("GGGCC")
    # the bundled fixture ends the same way
    assert not open(os.path.join(GOLD, "crafted_L5_nonewline.txt")).read().endswith("\n")
    assert len(from_whitelist("crafted_L5_nonewline.txt").whitelist[-1]) == 4


def test_lines_of_another_length_go_to_the_side_map(tmp_path):
    p = tmp_path / "wl.txt"
    p.write_text("ACGT\nACG\nTTTTTT\nACGA\nNCG\n")
    m = barcode.ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(str(p))
    assert m.barcode_length == 4
    assert m.get_corrected_barcode("ACGT") == "ACGA"  # a later neighbour wins
    assert m.get_corrected_barcode("ACG") == "NCG"  # "NCG" (line 5) writes its error "ACG" after line 2 did
    assert m.get_corrected_barcode("NCG") == "NCG"
    assert m.get_corrected_barcode("ACC") == "ACG"
    assert m.get_corrected_barcode("TTTNTT") == "TTTTTT"
    for miss in ("TTTTT", "AC", "", "TTNNTT", "acg"):
        with pytest.raises(KeyError):
            m.get_corrected_barcode(miss)


def test_whitelist_line_outside_acgt_follows_the_reference(tmp_path):
    # the reference's bundled list ends with "NAGGTGCCAGACACTT": such a line is kept, as the dict keeps it
    assert open(os.path.join(GOLD, "1k-august-2016.txt")).read().split()[-1].startswith("N")
    p = tmp_path / "n.txt"
    p.write_text("ACGT\nACNT\nacgt\n")
    m = barcode.ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(str(p))
    assert m.get_corrected_barcode("ACGT") == "ACNT"  # ACNT's error at position 2, written later
    assert m.get_corrected_barcode("ACNT") == "ACNT"
    assert m.get_corrected_barcode("ACTT") == "ACNT"
    assert m.get_corrected_barcode("AAGT") == "ACGT"
    assert m.get_corrected_barcode("Ncgt") == "acgt"
    assert m.get_corrected_barcode("ANNT") == "ACNT"  # one substitution (C -> N) away from the line itself
    with pytest.raises(KeyError):
        m.get_corrected_barcode("NNNT")


def test_whitelist_value_errors(tmp_path):
    p = tmp_path / "l32.txt"
    p.write_text("ACGT" * 8 + "\n")
    with pytest.raises(ValueError, match="31"):
        barcode.ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(str(p))
    p = tmp_path / "l31.txt"
    p.write_text("ACGT" * 8)  # the unterminated line reads as 31 bases
    assert barcode.ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(str(p)).barcode_length == 31
    with pytest.raises(ValueError, match="32"):
        barcode.Barcodes({0: 1, 1: 1}, 33).summarize_hamming_distances()


@pytest.mark.parametrize("name", WHITELISTS)
def test_twobit_against_the_reference(name):
    s = STATS[name]
    coder = TwoBit(s["barcode_length"])
    assert s["twobit"]
    for text, code, decoded, gc in s["twobit"]:
        assert TwoBit.encode(text.encode()) == code
        assert TwoBit.encode(text.lower().encode()) == code
        assert coder.decode(code) == decoded.encode() == text.encode()
        assert coder.gc_content(code) == gc
    for a, b, d in s["hamming"]:
        assert TwoBit.hamming_distance(a, b) == d
        assert TwoBit.hamming_distance(b, a) == d
    assert TwoBit.hamming_distance(5, 5) == 0


def test_twobit_ambiguity_and_invalid_bytes():
    for _ in range(20):
        assert 0 <= TwoBit.encode(b"N") <= 3
        assert TwoBit.encode(b"ANA") & 0b110011 == 0
    assert TwoBit.encode(b"") == 0
    for bad in (b"AC-T", b"X", b"AC T", b"AC1"):
        with pytest.raises(KeyError):
            TwoBit.encode(bad)
    assert barcode.encode_array(np.frombuffer(b"ACGTTGCA", dtype=np.uint8).reshape(2, 4)).tolist() == \
        [TwoBit.encode(b"ACGT"), TwoBit.encode(b"TGCA")]


@pytest.mark.parametrize("name", WHITELISTS)
def test_base_frequency_and_diversity_equal_the_reference(name):
    s = STATS[name]
    random.seed(2016)  # the fixture's seed: the 1k list's last line starts with N, which TwoBit draws a base for
    b = barcode.Barcodes.from_whitelist(os.path.join(GOLD, name), s["barcode_length"])
    assert len(b) == s["n_barcodes"]
    freq = b.base_frequency()
    assert freq.dtype == np.uint64 and freq.shape == (s["barcode_length"], 4)
    assert freq.tolist() == s["base_frequency"]
    div = b.effective_diversity()
    want = np.array([float(v) for v in s["effective_diversity"]])
    assert div.shape == want.shape
    assert np.all(np.abs(div - want) <= 1e-15)
    with pytest.raises(NotImplementedError):
        b.base_frequency(weighted=True)
    with pytest.raises(NotImplementedError):
        b.effective_diversity(weighted=True)


def test_barcodes_container():
    b = barcode.Barcodes.from_iterable_strings(["ACGT", "ACGT", "TTTT"], 4)
    code = TwoBit.encode(b"ACGT")
    assert code in b and b[code] == 2 and len(b) == 2 and sorted(b) == sorted([code, TwoBit.encode(b"TTTT")])
    assert dict(barcode.Barcodes.from_iterable_bytes([b"ACGT", b"TTTT", b"ACGT"], 4)._mapping) == dict(b._mapping)
    assert dict(barcode.Barcodes.from_iterable_encoded([code, code], 4)._mapping) == {code: 2}


def test_summary_from_histogram_is_numpy_percentile_and_mean():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 4, 5, 8, 1001, 4098):
        d = rng.integers(0, 17, size=n)
        hist = np.bincount(d, minlength=33)
        got = barcode.summary_from_histogram(hist)
        want = list(np.percentile(d, [0, 25, 50, 75, 100])) + [np.mean(d)]
        assert list(got.values()) == want
        assert list(got) == ["minimum", "25th percentile", "median", "75th percentile", "maximum", "average"]


def test_summary_of_fewer_than_two_barcodes_is_numpys():
    # no pair: the empty list goes to numpy on the host, as in the reference; no GPU is needed
    for given in ({}, {5: 1}):
        b = barcode.Barcodes(given, 16)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            try:
                want = list(np.percentile([], [0, 25, 50, 75, 100])) + [np.mean([])]
            except Exception as e:  # numpy decides; whatever it does, the class does
                with pytest.raises(type(e)):
                    b.summarize_hamming_distances()
            else:
                got = b.summarize_hamming_distances()
                assert np.array_equal(np.array(list(got.values())), np.array(want), equal_nan=True)


def test_header_declares_exactly_the_exported_functions():
    text = open(os.path.join(ROOT, "include", "sct_barcode.h")).read()
    names = sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(sct_bc_\w+)\(", text, flags=re.M)))
    assert names == sorted(barcode.EXPORTED)
    lib = barcode.load()
    for name in names:
        assert hasattr(lib, name), name


def test_size_query_and_argument_checks_need_no_gpu():
    lib = barcode.load()
    nbytes = ctypes.c_size_t(0)
    assert lib.sct_bc_table_size(737280, ctypes.byref(nbytes)) == 0
    # load factor <= 0.5: at least 2 slots of 16 bytes per barcode, and the 8-byte copy of each code
    assert nbytes.value >= 737280 * (2 * 16 + 8)
    assert lib.sct_bc_table_size(-1, ctypes.byref(nbytes)) < 0
    assert b"n_whitelist" in lib.sct_bc_last_error()
    # rejected before anything touches a device: bad length, short buffer, misaligned table
    assert lib.sct_bc_table_build(None, 4, 32, ctypes.c_void_p(16), 1 << 20, None) < 0
    assert b"length" in lib.sct_bc_last_error()
    assert lib.sct_bc_table_build(ctypes.c_void_p(16), 4, 16, ctypes.c_void_p(16), 64 * 16 + 4 * 8 - 1, None) == -2
    assert b"needed" in lib.sct_bc_last_error()
    assert lib.sct_bc_correct(ctypes.c_void_p(8), 4, None, 0, 16, None, None, None) < 0
    assert lib.sct_bc_pair_hist(None, 2, 33, ctypes.c_void_p(16), None) < 0
    assert lib.sct_bc_pair_hist(None, (1 << 22) + 1, 16, ctypes.c_void_p(16), None) < 0


def _records(n):
    src = os.path.join(ROOT, "tests", "golden", "bam", "test_r2_tagged.bam")
    out = []
    for r in bam.open_alignments(src):
        out.append(r)
        if len(out) == n:
            break
    return out


def test_correct_bam_without_cr_raises_keyerror_and_writes_nothing(tmp_path):
    recs = _records(6)
    for k, r in enumerate(recs):
        r._tags = dict(r._tags)
        r._tags["CR"] = "ACGTACGTACGTACGT"
    del recs[4]._tags["CR"]
    src, dst = str(tmp_path / "in.bam"), str(tmp_path / "out.bam")
    bamwriter.write_bam(src, recs)
    m = from_whitelist("1k-august-2016.txt")
    with pytest.raises(KeyError, match="CR"):
        m.correct_bam(src, dst)
    assert not os.path.exists(dst)


def test_tag_column_collects_and_rewrites(tmp_path):
    # the host side of correct_bam alone: CB replaced or appended as the last tag, all else unchanged
    recs = _records(40)
    crs = []
    for k, r in enumerate(recs):
        tags = OrderedDict((t, v) for t, v in r._tags.items() if t not in ("CR", "CB"))
        cr = ("ACGT" * 4)[: 16 if k % 5 else 12]
        if k % 3 == 0:  # an existing CB in the middle of the tags
            items = list(tags.items())
            tags = OrderedDict(items[:1] + [("CB", "OLDVALUE")] + items[1:])
        tags["CR"] = cr
        if k % 4 == 0:
            tags["ZZ"] = "after"
        r._tags = tags
        crs.append(cr)
    src, dst = str(tmp_path / "in.bam"), str(tmp_path / "out.bam")
    bamwriter.write_bam(src, recs)
    with bamnative.TagColumn(src, "CR", "CB", 16) as col:
        assert col.n == len(recs)
        values = col.values()
        assert [bytes(v) for v in values] == [c.encode() if len(c) == 16 else bytes(16) for c in crs]
        assert col.others() == [c for c in crs if len(c) != 16]
        new = np.frombuffer(b"TTTTGGGGCCCCAAAA", dtype=np.uint8)
        col.write(dst, np.tile(new, (col.n, 1)))
    out = list(bam.open_alignments(dst))
    assert bam.read_header(dst) == bam.read_header(src)
    assert len(out) == len(recs)
    src_stream = gzip.open(src, "rb").read()
    expected = src_stream[:len(src_stream) - sum(len(bamwriter.record_bytes(r)) for r in recs)]  # the header
    for a, b, cr in zip(recs, out, crs):
        want = [(t, v) for t, v in a._tags.items() if t != "CB"] + [("CB", "TTTTGGGGCCCCAAAA" if len(cr) == 16 else cr)]
        assert list(b._tags.items()) == want
        for f in ("query_name", "flag", "reference_id", "pos", "mapq", "cigar", "l_seq", "_qual"):
            assert getattr(a, f) == getattr(b, f), f
        a._tags = OrderedDict(want)
        expected += bamwriter.record_bytes(a)
    assert gzip.open(dst, "rb").read() == expected  # every byte but the moved tag is the input's
    assert open(dst, "rb").read().endswith(bamwriter._EOF)
