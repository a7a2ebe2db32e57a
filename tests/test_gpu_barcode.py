"""sctools_amd.barcode on the GPU: the correction table and lookup kernels, the all-pairs Hamming
histogram, correct_bam and the C-ABI of include/sct_barcode.h.

Expectations come from the reference's own results (tests/golden/barcode/, written by
tests/golden/make_barcode_golden.py), from a dict built by the reference's rule inside this file,
and from numpy; ``get_corrected_barcode`` (host) is used only where it is itself held to the
fixture on every query by test_barcode_cpu.py.
"""
import ctypes
import gzip
import json
import os
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch

import bamwriter
from sctools_amd import bam, barcode
from sctools_amd.__main__ import main as cli_main
from sctools_amd.encodings import TwoBit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "barcode")
WHITELISTS = ["1k-august-2016.txt", "crafted_L8.txt", "crafted_L5_nonewline.txt", "crafted_L21.txt"]
CORRECTIONS = json.load(gzip.open(os.path.join(GOLD, "corrections.json.gz"), "rt"))
STATS = json.load(open(os.path.join(GOLD, "pair_stats.json")))
_MAPS = {}


def from_whitelist(name):
    if name not in _MAPS:
        _MAPS[name] = barcode.ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(os.path.join(GOLD, name))
    return _MAPS[name]


def write_whitelist(tmp_path, lines, name="wl.txt"):
    p = tmp_path / name
    p.write_text("".join(b + "\n" for b in lines))
    return barcode.ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(str(p))


def rule_dict(lines):
    """The reference's rule, restated: filled in file order, later writers overwrite; value = file index."""
    out = {}
    for i, w in enumerate(lines):
        out[w] = i
        for pos in range(len(w)):
            for e in "ACGTN":
                if e != w[pos]:
                    out[w[:pos] + e + w[pos + 1:]] = i
    return out


def as_rows(queries, length):
    return np.array([q.encode("latin-1") for q in queries], dtype="S%d" % length)


def check_against(m, queries, expected_index):
    """indices and corrected bytes of one correct_barcodes call against expected file indices (-1: none)"""
    length = m.barcode_length
    rows = as_rows(queries, length)
    index, corrected = m.correct_barcodes(rows, return_corrected=True)
    assert index.dtype == np.int32 and index.shape == (len(queries),)
    assert corrected.dtype == np.uint8 and corrected.shape == (len(queries), length)
    expected_index = np.asarray(expected_index, dtype=np.int32)
    wrong = np.flatnonzero(index != expected_index)
    assert wrong.size == 0, [(queries[i], int(index[i]), int(expected_index[i])) for i in wrong[:10]]
    want = [m.whitelist[i] if i >= 0 else q for q, i in zip(queries, expected_index)]
    got = [bytes(r).decode("latin-1") for r in corrected]
    bad = [(q, g, w) for q, g, w in zip(queries, got, want) if g != w]
    assert not bad, bad[:10]
    assert np.array_equal(m.correct_barcodes(rows), index)  # without the corrected bytes: the same indices


def last_index(m):
    out = {}
    for i, b in enumerate(m.whitelist):
        out[b] = i
    return out


@pytest.mark.parametrize("name", WHITELISTS)
def test_every_fixture_query_of_the_whitelist_length(name):
    m = from_whitelist(name)
    at = last_index(m)
    pairs = [(q, c) for q, c in CORRECTIONS[name] if len(q) == m.barcode_length]
    assert len(pairs) > 400
    check_against(m, [q for q, _ in pairs], [at[c] if c is not None else -1 for _, c in pairs])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_wave_and_block_edges(n):
    m = from_whitelist("1k-august-2016.txt")
    at = last_index(m)
    pairs = [(q, c) for q, c in CORRECTIONS["1k-august-2016.txt"] if len(q) == 16]
    pairs = [pairs[(k * 7) % len(pairs)] for k in range(n)]
    check_against(m, [q for q, _ in pairs], [at[c] if c is not None else -1 for _, c in pairs])


def _crafted(rng, length, n_seeds):
    lines = []
    for k in range(n_seeds):
        a = "".join(rng.choice("ACGT") for _ in range(length))
        lines.append(a)
        if k % 2 == 0:
            pos = rng.randrange(length)
            lines.append(a[:pos] + rng.choice([b for b in "ACGT" if b != a[pos]]) + a[pos + 1:])
        if k % 5 == 0:
            lines.append(a)
    rng.shuffle(lines)
    return lines


def _queries(rng, lines, per_line=6):
    length = len(lines[0])
    out = list(lines) + ["N" * length, lines[0].lower()]
    for w in lines:
        for _ in range(per_line):
            q = list(w)
            for _ in range(rng.choice([1, 1, 1, 2])):
                q[rng.randrange(length)] = rng.choice("ACGTN")
            out.append("".join(q))
    return out


@pytest.mark.parametrize("length", [1, 5, 8, 16, 21, 31])
def test_barcode_lengths(tmp_path, length):
    rng = random.Random(length)
    lines = ["A", "G"] if length == 1 else _crafted(rng, length, 40)
    m = write_whitelist(tmp_path, lines)
    assert m.barcode_length == length
    rule = rule_dict(lines)
    queries = _queries(rng, lines) + (list("ACGTNacgt-") if length == 1 else [])
    check_against(m, queries, [rule.get(q, -1) for q in queries])


def test_whitelists_of_one_and_two_entries(tmp_path):
    one = write_whitelist(tmp_path, ["ACGTACGTACGTACGT"], "one.txt")
    queries = ["ACGTACGTACGTACGT", "ACGTACGTACGTACGA", "NCGTACGTACGTACGT", "ACGTACGTACGTACAA", "TTTTTTTTTTTTTTTT",
               "ACGTACGTNCGTACGN", "acgtacgtacgtacgt"]
    check_against(one, queries, [0, 0, 0, -1, -1, -1, -1])
    two = write_whitelist(tmp_path, ["ACGTACGTACGTACGT", "ACGTACGTACGTACGA"], "two.txt")
    # the first entry has a later neighbour: it is corrected to it, and so is everything they share
    check_against(two, queries + ["ACGTACGTACGTACGC", "CCGTACGTACGTACGT", "CCGTACGTACGTACGA", "ACGTACGTACGTACGN"],
                  [1, 1, 0, 1, -1, -1, -1, 1, 0, 1, 1])  # ...ACAA is one substitution from the second entry


def test_dense_table_with_duplicates(tmp_path):
    rng = np.random.default_rng(8)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    lines = [bytes(r).decode() for r in bases[rng.integers(0, 4, size=(20000, 8))]]
    assert len(set(lines)) < len(lines)  # 20,000 draws from 65,536: duplicates are certain
    m = write_whitelist(tmp_path, lines)
    acgtn = np.frombuffer(b"ACGTN", dtype=np.uint8)
    queries = [bytes(r).decode() for r in acgtn[rng.choice(5, size=(50000, 8), p=[.24, .24, .24, .24, .04])]] + lines
    rows = as_rows(queries, 8)
    index, corrected = m.correct_barcodes(rows, return_corrected=True)
    host = np.empty(len(queries), dtype=np.int32)
    for k, q in enumerate(queries):
        try:
            host[k] = m._whitelist.lookup(q)
        except KeyError:
            host[k] = -1
    assert np.array_equal(index, host)
    assert (host >= 0).mean() > 0.5 and (host < 0).sum() > 100
    # independent of both code paths: the rule's own dict, on a subset
    rule = rule_dict(lines)
    subset = rng.choice(len(queries), size=2000, replace=False)
    assert [int(index[k]) for k in subset] == [rule.get(queries[k], -1) for k in subset]
    for k in subset:
        want = lines[index[k]] if index[k] >= 0 else queries[k]
        assert bytes(corrected[k]).decode() == want


def _one_error(rng, w):
    pos = rng.randrange(len(w))
    return w[:pos] + rng.choice([b for b in "ACGT" if b != w[pos]]) + w[pos + 1:]


def test_every_lane_misses_and_one_lane_per_wave_misses():
    m = from_whitelist("1k-august-2016.txt")
    rng = random.Random(5)
    good = [w for w in m.whitelist if set(w) <= set("ACGT")]
    every = [_one_error(rng, good[k % len(good)]) for k in range(1024)]
    one = [good[k % len(good)] if k % 64 != 17 else _one_error(rng, good[k % len(good)]) for k in range(1024)]
    rule = rule_dict(m.whitelist)
    for queries in (every, one):
        check_against(m, queries, [rule.get(q, -1) for q in queries])
    # the list's minimum pair distance is 2: an error of one barcode is no other barcode
    assert all(q not in good for q in every)


def test_device_tensors_and_strided_input():
    m = from_whitelist("crafted_L8.txt")
    at = last_index(m)
    pairs = [(q, c) for q, c in CORRECTIONS["crafted_L8.txt"] if len(q) == 8][:700]
    rows = as_rows([q for q, _ in pairs], 8).view(np.uint8).reshape(len(pairs), 8)
    want = torch.tensor([at[c] if c is not None else -1 for _, c in pairs], dtype=torch.int32)
    dev = torch.device("cuda", torch.cuda.current_device())
    index, corrected = m.correct_barcodes(torch.from_numpy(rows).to(dev), return_corrected=True)
    assert index.is_cuda and corrected.is_cuda and index.dtype == torch.int32 and corrected.dtype == torch.uint8
    assert torch.equal(index.cpu(), want)
    host_index = m.correct_barcodes(torch.from_numpy(rows))
    assert not host_index.is_cuda and torch.equal(host_index, want)
    # strided views: every second row, and a transposed [L, n] buffer; copied, never read through the wrong strides
    wide = torch.zeros((len(pairs), 2, 8), dtype=torch.uint8, device=dev)
    wide[:, 0] = torch.from_numpy(rows).to(dev)
    view = wide[:, 0]
    assert not view.is_contiguous()
    i2, c2 = m.correct_barcodes(view, return_corrected=True)
    assert torch.equal(i2.cpu(), want) and torch.equal(c2, corrected)
    transposed = torch.from_numpy(np.ascontiguousarray(rows.T)).to(dev).T
    assert not transposed.is_contiguous()
    assert torch.equal(m.correct_barcodes(transposed).cpu(), want)
    assert np.array_equal(m.correct_barcodes(np.asfortranarray(rows)), want.numpy())
    for bad in (rows[:, :7], rows.astype(np.int8), rows.reshape(-1)):
        with pytest.raises(ValueError):
            m.correct_barcodes(bad)


# ---------------- pair statistics ----------------
@pytest.mark.parametrize("name", WHITELISTS)
def test_summarize_hamming_distances_equals_the_reference(name):
    s = STATS[name]
    random.seed(2016)  # the fixture's seed: TwoBit draws a base for the N that starts the 1k list's last line
    b = barcode.Barcodes.from_whitelist(os.path.join(GOLD, name), s["barcode_length"])
    got = b.summarize_hamming_distances()
    assert list(got) == ["minimum", "25th percentile", "median", "75th percentile", "maximum", "average"]
    for key, value in s["summarize_hamming_distances"].items():
        assert got[key] == float(value), key


def numpy_pair_histogram(codes):
    codes = np.asarray(codes, dtype=np.uint64)
    hist = np.zeros(33, dtype=np.uint64)
    for i in range(len(codes) - 1):
        d = codes[i] ^ codes[i + 1:]
        d = (d | (d >> np.uint64(1))) & np.uint64(0x5555555555555555)
        dist = np.unpackbits(d.view(np.uint8)).reshape(len(d), 64).sum(axis=1)
        hist += np.bincount(dist, minlength=33).astype(np.uint64)
    return hist


@pytest.mark.parametrize("n,length", [(2, 16), (1023, 16), (1024, 16), (1025, 16), (3000, 16), (1500, 32), (700, 3)])
def test_pair_histogram_equals_numpy(n, length):
    rng = np.random.default_rng(n + length)
    codes = rng.integers(0, 1 << 62, size=n, dtype=np.uint64) << np.uint64(2) | rng.integers(0, 4, size=n, dtype=np.uint64)
    if length < 32:
        codes &= np.uint64((1 << (2 * length)) - 1)
    got = barcode.pair_histogram(codes, length)
    assert got.dtype == np.uint64 and got.shape == (33,)
    assert int(got.sum()) == n * (n - 1) // 2
    assert np.array_equal(got, numpy_pair_histogram(codes))


# ---------------- correct_bam ----------------
def test_correct_bam_and_cli(tmp_path):
    m = from_whitelist("1k-august-2016.txt")
    good = [w for w in m.whitelist if set(w) <= set("ACGT")]
    rng = random.Random(11)
    source = list(bam.open_alignments(os.path.join(ROOT, "tests", "golden", "bam", "test_r2_tagged.bam")))
    rule = rule_dict(m.whitelist)
    recs, expected = [], []
    for k in range(20000):
        r = source[k % len(source)]
        r = bam.BamRecord("%s_%d" % (r.query_name, k), r.flag, r.reference_id, r.pos, r.mapq, r.cigar, r.l_seq, r._qual,
                          OrderedDict((t, v) for t, v in r._tags.items() if t not in ("CR", "CB")))
        w = good[rng.randrange(len(good))]
        case = k % 8
        if case == 0:
            cr, cb = w, w  # exact
        elif case == 1:
            cr, cb = _one_error(rng, w), w  # one substitution
        elif case == 2:
            pos = rng.randrange(16)
            cr, cb = w[:pos] + "N" + w[pos + 1:], w
        elif case == 3:
            cr = _one_error(rng, w[:8]) + _one_error(rng, w[8:])  # double error: passed through
            cb = cr
        elif case == 4:
            cr = cb = w.lower()
        elif case == 5:
            cr = cb = w[:rng.choice([0, 7, 15])] if k % 16 == 5 else w + "A"  # another length
        elif case == 6:
            cr, cb = w, w
            items = list(r._tags.items())
            r._tags = OrderedDict(items[:2] + [("CB", "STALESTALESTALE1")] + items[2:])  # an existing CB
        else:
            cr, cb = _one_error(rng, w), w
            r._tags["CB"] = "AAAA"
            r._tags.move_to_end("CB", last=False)
        r._tags["CR"] = cr
        if k % 3 == 0:
            r._tags["ZZ"] = "tail"  # a tag after CR
        recs.append(r)
        if case in (0, 4, 5, 6):
            assert (m.whitelist[rule[cr]] if cr in rule else cr) == cb
        expected.append(m.whitelist[rule[cr]] if cr in rule else cr)  # (two list entries at distance 2 share errors)
    assert sum(1 for r, cb in zip(recs, expected) if r._tags["CR"] != cb) > 7000
    src, dst, dst_cli = str(tmp_path / "in.bam"), str(tmp_path / "out.bam"), str(tmp_path / "cli.bam")
    bamwriter.write_bam(src, recs)
    m.correct_bam(src, dst)
    assert bam.read_header(dst) == bam.read_header(src)
    out = list(bam.open_alignments(dst))
    assert len(out) == len(recs)
    for a, b, cb in zip(recs, out, expected):
        tags = list(b._tags.items())
        assert tags[-1] == ("CB", cb), (a._tags, tags)
        assert tags[:-1] == [(t, v) for t, v in a._tags.items() if t != "CB"]
        for f in ("query_name", "flag", "reference_id", "pos", "mapq", "cigar", "l_seq", "_qual"):
            assert getattr(a, f) == getattr(b, f), f
    data = open(dst, "rb").read()
    assert data.endswith(bamwriter._EOF)
    assert data.count(b"\x1f\x8b\x08\x04") > 10  # several BGZF members
    assert cli_main(["CorrectBarcodes", "-i", src, "-o", dst_cli, "--whitelist", os.path.join(GOLD, "1k-august-2016.txt"),
                     "--device", str(torch.cuda.current_device())]) == 0
    assert open(dst_cli, "rb").read() == data


# ---------------- the C-ABI ----------------
def test_c_abi_directly():
    lib = barcode.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = ["ACGTACGT", "ACGTACGA", "TTTTTTTT", "ACGTACGT"]
    codes = torch.tensor([TwoBit.encode(b.encode()) for b in lines], dtype=torch.int64, device=dev)
    nbytes = ctypes.c_size_t(0)
    assert lib.sct_bc_table_size(len(lines), ctypes.byref(nbytes)) == 0
    assert nbytes.value == 64 * 16 + len(lines) * 8 + (1 << 16) // 8  # slots, codes in file order, presence filter
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    table = torch.full((nbytes.value,), 0x5A, dtype=torch.uint8, device=dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    # one byte short: a negative code, a message, and nothing launched (the buffer keeps its fill)
    assert lib.sct_bc_table_build(ptr(codes), len(lines), 8, ptr(table), nbytes.value - 1, stream) == -2
    assert b"needed" in lib.sct_bc_last_error()
    torch.cuda.synchronize()
    assert bool((table == 0x5A).all())
    assert lib.sct_bc_table_build(ptr(codes), len(lines), 8, ptr(table), nbytes.value, stream) == 0
    queries = [b"ACGTACGT", b"ACGTACGA", b"ACGTACGC", b"TTTTTTTN", b"TTTTTTAA", b"ACGTACGN", b"tttttttt"]
    raw = torch.tensor(list(b"".join(queries)), dtype=torch.uint8, device=dev)
    index = torch.full((len(queries),), -7, dtype=torch.int32, device=dev)
    corrected = torch.zeros(len(queries) * 8, dtype=torch.uint8, device=dev)
    assert lib.sct_bc_correct(ptr(table), len(lines), ptr(raw), len(queries), 8, ptr(index), ptr(corrected), stream) == 0
    assert index.tolist() == [3, 3, 3, 2, -1, 3, -1]
    assert bytes(corrected.cpu().numpy()) == b"ACGTACGT" * 3 + b"TTTTTTTT" + b"TTTTTTAA" + b"ACGTACGT" + b"tttttttt"
    assert lib.sct_bc_correct(ptr(table), len(lines), ptr(raw), len(queries), 8, ptr(index), None, stream) == 0
    assert index.tolist() == [3, 3, 3, 2, -1, 3, -1]
    assert lib.sct_bc_correct(ptr(table), len(lines), ptr(raw), len(queries), 32, ptr(index), None, stream) < 0
    assert b"length" in lib.sct_bc_last_error()
    hist = torch.full((33,), -1, dtype=torch.int64, device=dev)
    assert lib.sct_bc_pair_hist(ptr(codes), len(lines), 8, ptr(hist), stream) == 0
    want = [0] * 33
    # the duplicate pair; each copy against ACGTACGA; TTTTTTTT shares two Ts with ACGTACGT and one with ACGTACGA
    want[0], want[1], want[6], want[7] = 1, 2, 2, 1
    assert hist.tolist() == want
