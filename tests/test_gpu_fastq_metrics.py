"""FastqMetrics on the GPU: the ``sct_fqm_*`` calls on one column, ``FastqMetrics.compute`` on text
and on the bundled R1 file, and the command end to end.

The reference binary needs libStatGen and gzstream, which are not at hand, so the expectation is
:func:`restate` below: Python slices of the sequence lines, a ``Counter`` per kind, and a
per-position count by the reference's ``recordChunk`` rule (either case counts as the base, any
other byte as ``other``).

Count tables are compared by the rule of the module's docstring: the multiset of (count, barcode)
pairs is the restatement's, counts do not increase, and barcodes ascend within equal counts.
Matrices, ``other`` and ``n_records`` are compared exactly.  Wherever the input is upper-case
``ACGTN`` only, no row may have gone to the host and the device's error word is 0: the host counter
must not stand in for a broken device path.
"""
import ctypes
import functools
import gzip
import os
from collections import Counter

import numpy as np
import pytest

from sctools_amd import fastq_metrics
from sctools_amd.__main__ import main as cli_main

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R1 = os.path.join(ROOT, "tests", "golden", "fastq", "test_r1.fastq")
R = fastq_metrics.R
CLEAN = frozenset(b"ACGTN")
BASES = np.frombuffer(b"ACGTN", dtype=np.uint8)


# ---- the restatement ----

def matrix(rows, length):
    """(int64 [length, 5] of A C G T N in either case, int64 [length] of every other byte)."""
    pwm, other = np.zeros((length, 5), dtype=np.int64), np.zeros(length, dtype=np.int64)
    for row in rows:
        for i, b in enumerate(row.upper()):
            at = b"ACGTN".find(bytes([b]))
            if at >= 0:
                pwm[i, at] += 1
            else:
                other[i] += 1
    return pwm, other


def restate(sequences, structure):
    """Per kind (C, M): (Counter of the raw barcodes, matrix, other, rows with a byte outside ACGTN)."""
    out, at, cuts = [], 0, {"C": [], "M": []}
    for type_, length in fastq_metrics.parse_read_structure(structure):
        if type_ in cuts:
            cuts[type_].append(slice(at, at + length))
        at += length
    for kind in "CM":
        rows = [b"".join(s[c] for c in cuts[kind]) for s in sequences]
        length = sum(c.stop - c.start for c in cuts[kind])
        out.append((Counter(rows),) + matrix(rows, length) + (sum(1 for r in rows if not set(r) <= CLEAN),))
    return out


def sequences_of(text: bytes):
    lines = text.split(b"\n")
    return [lines[4 * r + 1] for r in range(len(lines) // 4)]


@functools.lru_cache(maxsize=None)
def golden(structure, copies=1):
    sequences = sequences_of(open(R1, "rb").read()) * copies
    assert len(sequences) == 100 * copies
    return len(sequences), restate(sequences, structure)


def check_counts(rows, counts, want: Counter):
    got = [(int(c), bytes(r)) for c, r in zip(counts, rows)]
    assert Counter(got) == Counter((c, k) for k, c in want.items())
    assert got == sorted(got, key=lambda x: (-x[0], x[1]))


def check_result(result, n_records, want, clean):
    (c_counts, c_pwm, c_other, c_exc), (m_counts, m_pwm, m_other, m_exc) = want
    if clean:
        assert c_exc == 0 and m_exc == 0  # the generator's side first
        assert result.n_host_rows == 0
    assert result.n_records == n_records
    assert result.n_host_rows == c_exc + m_exc
    check_counts(result.barcodes, result.barcode_counts, c_counts)
    check_counts(result.umis, result.umi_counts, m_counts)
    assert np.array_equal(result.barcode_pwm, c_pwm) and np.array_equal(result.umi_pwm, m_pwm)
    assert np.array_equal(result.barcode_other, c_other) and np.array_equal(result.umi_other, m_other)
    assert result.barcode_counts.dtype == np.int64 and result.barcodes.dtype == np.uint8
    assert result.barcode_pwm.shape == (c_pwm.shape[0], 5) and result.umi_other.shape == (m_pwm.shape[0],)


# ---- one column through the C-ABI ----

def run_column(col: np.ndarray, n_slots=None):
    """``(Counter key -> count, pwm [L, 6], result words, exception rows)`` of one sct_fqm_accumulate and one
    sct_fqm_compact over ``col`` (uint8 [n, L])."""
    import torch

    lib = fastq_metrics.load()
    dev = torch.device("cuda", 0)
    n, length = col.shape
    n_slots = n_slots or fastq_metrics.next_slots(fastq_metrics.MIN_SLOTS, 0, n)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t.numel() else None  # noqa: E731
    nbytes = ctypes.c_size_t(0)
    fastq_metrics.check(lib.sct_fqm_table_size(n_slots, ctypes.byref(nbytes)))
    assert nbytes.value == 16 * n_slots
    table = torch.full((nbytes.value,), 0x55, dtype=torch.uint8, device=dev)
    fastq_metrics.check(lib.sct_fqm_table_init(p(table), n_slots, table.numel(), None))
    d_col = torch.from_numpy(col.copy()).to(dev)
    pwm = torch.zeros((length, 6), dtype=torch.int64, device=dev)
    exceptions = torch.full((n,), -1, dtype=torch.int64, device=dev)
    result = torch.zeros(4, dtype=torch.int64, device=dev)
    fastq_metrics.check(lib.sct_fqm_accumulate(p(d_col), n, length, p(table), n_slots, table.numel(), p(pwm),
                                               p(exceptions), p(result), None))
    torch.cuda.synchronize(dev)
    distinct, n_exceptions = int(result[0].cpu()), int(result[1].cpu())
    keys = torch.full((distinct + 1,), -7, dtype=torch.int64, device=dev)
    counts = torch.full((distinct + 1,), -7, dtype=torch.int64, device=dev)
    fastq_metrics.check(lib.sct_fqm_compact(p(table), n_slots, table.numel(), p(keys), p(counts), distinct, p(result), None))
    torch.cuda.synchronize(dev)
    words = [int(x) for x in result.cpu()]
    assert words[2] == distinct and int(keys[distinct].cpu()) == -7 and int(counts[distinct].cpu()) == -7
    rows = fastq_metrics.decode_keys(keys[:distinct].cpu().numpy().view(np.uint64), length)
    got = Counter()
    for r, c in zip(rows, counts[:distinct].cpu().numpy()):
        assert bytes(r) not in got
        got[bytes(r)] = int(c)
    return got, pwm.cpu().numpy(), words, sorted(exceptions[:n_exceptions].cpu().tolist())


def check_column(col: np.ndarray, n_slots=None):
    rows = [bytes(r) for r in col]
    want_pwm, want_other = matrix(rows, col.shape[1])
    dirty = [i for i, r in enumerate(rows) if not set(r) <= CLEAN]
    got, pwm, (distinct, n_exceptions, compacted, error), exceptions = run_column(col, n_slots)
    assert error == 0
    assert exceptions == dirty and n_exceptions == len(dirty)
    want = Counter(r for r in rows if set(r) <= CLEAN)
    assert got == want and distinct == len(want)
    assert np.array_equal(pwm[:, :5], want_pwm) and np.array_equal(pwm[:, 5], want_other)
    return got


def drawn_column(n, length, seed):
    """n rows of upper-case ACGTN, drawn from about n / 3 keys so that keys repeat."""
    rng = np.random.default_rng(seed)
    pool = BASES[rng.integers(0, 5, (max(1, n // 3), length))]
    return np.ascontiguousarray(pool[rng.integers(0, len(pool), n)]).reshape(n, length)


@pytest.mark.parametrize("length", [1, 7, 16, 21])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, R - 1, R, R + 1, 3 * R + 7])
def test_one_column_through_the_c_abi(n, length):
    check_column(drawn_column(n, length, seed=1000 * n + length))


def test_all_rows_equal():
    col = np.tile(np.frombuffer(b"GGGGGGGGGGGGGGGG", dtype=np.uint8), (5000, 1))
    assert check_column(col) == Counter({b"G" * 16: 5000})


@pytest.mark.parametrize("length", [16, 21])
def test_all_rows_distinct(length):
    rng = np.random.default_rng(7)
    col = np.unique(BASES[rng.integers(0, 5, (3 * R + 7 + 200, length))], axis=0)[:3 * R + 7]
    col = np.ascontiguousarray(col[rng.permutation(len(col))])
    assert len(col) == 3 * R + 7
    got = check_column(col)
    assert len(got) == len(col) and set(got.values()) == {1}
    if length == 21:  # the key's highest bits: T first and T last
        edge = np.tile(np.frombuffer(b"T" * 21, dtype=np.uint8), (3, 1))
        edge[1, 0], edge[2, 20] = ord("A"), ord("N")
        assert check_column(edge) == Counter({b"T" * 21: 1, b"A" + b"T" * 20: 1, b"T" * 20 + b"N": 1})


def test_table_at_exactly_the_growth_rules_size_and_with_dirty_rows():
    col = drawn_column(R, 9, seed=5)
    check_column(col, n_slots=2 * R)
    col[3, 2], col[R - 1, 8], col[77, 0], col[78, 4] = ord("a"), ord("."), ord("*"), ord("n")
    check_column(col, n_slots=2 * R)
    check_column(np.full((70, 3), ord("c"), dtype=np.uint8))  # nothing but exception rows


def test_windows_grow_and_rehash_the_table():
    import torch

    rng = np.random.default_rng(11)
    keys = np.unique(BASES[rng.integers(0, 5, (1400, 12))], axis=0)[:1000]
    assert len(keys) == 1000
    col = np.ascontiguousarray(np.concatenate([keys, keys, keys[:300]])[rng.permutation(2300)])
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev):
        kind = fastq_metrics._KindAccumulator(12, 64, dev)
        sizes = [kind.n_slots]
        for at in range(0, len(col), 100):
            kind.add(torch.from_numpy(col[at:at + 100]).to(dev))
            assert kind.n_slots >= 2 * kind.distinct  # the growth rule held for the window just added
            sizes.append(kind.n_slots)
        rows, counts, pwm, other = kind.finish()
    assert sizes[0] == 64 and sizes[-1] == 4096 and len(set(sizes)) >= 5  # 64, 256, 512, 1024, 2048, 4096
    assert kind.host_rows == 0 and kind.distinct == 1000 and int(kind.result[3].cpu()) == 0
    want = Counter(bytes(r) for r in col)
    check_counts(rows, counts, want)
    assert sorted(counts.tolist()) == [2] * 700 + [3] * 300
    want_pwm, want_other = matrix(list(want.elements()), 12)
    assert np.array_equal(pwm, want_pwm) and np.array_equal(other, want_other) and not other.any()


# ---- FastqMetrics.compute ----

def fastq_text(sequences):
    return b"".join(b"@read:%d\n%s\n+\n%s\n" % (i, s, b"F" * len(s)) for i, s in enumerate(sequences))


def test_lower_case_and_other_bytes_are_counted_on_the_host(tmp_path, capsys):
    rng = np.random.default_rng(3)
    pool = [bytes(BASES[rng.integers(0, 5, 12)]) for _ in range(40)]
    sequences = [pool[i] for i in rng.integers(0, 40, 3000)]
    dirty = {}
    for i in rng.choice(3000, 300, replace=False):
        s = bytearray(sequences[i])
        where = int(rng.integers(0, 12))
        s[where] = [s[where] | 0x20, ord("."), ord("*")][int(rng.integers(0, 3))]
        if rng.random() < 0.3:
            s = bytearray(bytes(s).lower())  # a whole read in lower case: both kinds' rows are exceptions
        sequences[i] = dirty[i] = bytes(s)
    path = str(tmp_path / "dirty.fastq")
    open(path, "wb").write(fastq_text(sequences))
    want = restate(sequences, "7C5M")
    assert want[0][3] + want[1][3] >= 300 and want[0][3] > 0 and want[1][3] > 0
    assert want[0][2].sum() + want[1][2].sum() > 0  # some '.' and '*'
    result = fastq_metrics.FastqMetrics(path, "7C5M").compute(window_bytes=20000, initial_slots=64)
    check_result(result, 3000, want, clean=False)
    assert result.n_host_rows == sum(1 for s in sequences if not set(s[:7]) <= CLEAN) \
        + sum(1 for s in sequences if not set(s[7:]) <= CLEAN)
    lower = Counter(s[:7] for s in dirty.values() if s[:7].islower())
    assert lower and all(int(result.barcode_counts[[bytes(r) for r in result.barcodes].index(k)]) == c
                         for k, c in lower.items())
    assert result.barcode_pwm.sum() + result.barcode_other.sum() == 3000 * 7  # lower case folded into the matrix
    assert "%d bytes" % (want[0][2].sum() + want[1][2].sum()) in capsys.readouterr().err


@pytest.mark.parametrize("structure", ["16C10M", "8C18X6C9M1X"])
def test_compute_on_the_bundled_r1(structure, tmp_path):
    if structure == "8C18X6C9M1X":
        # The bundled reads have 26 bases and this structure's UMI ends at base 41: on the bundled file
        # the short read raises (the module's first departure).  The structure is run on the same
        # reads, each lengthened to 42 bases with a stretch of its own.
        with pytest.raises(ValueError, match=r"record 0\b.*sequence line has 26 bytes"):
            fastq_metrics.FastqMetrics(R1, structure).compute()
        sequences = [s + s[5:21] for s in sequences_of(open(R1, "rb").read())]
        path = str(tmp_path / "long.fastq")
        open(path, "wb").write(fastq_text(sequences))
        gz = path + ".gz"
        gzip.open(gz, "wb").write(open(path, "rb").read())
        want1, want2 = restate(sequences, structure), restate(sequences * 2, structure)
    else:
        path, gz = R1, R1 + ".gz"
        want1, want2 = golden(structure)[1], golden(structure, 2)[1]
    first = None
    for window in (64, 1000, 16384, 1 << 20):
        result = fastq_metrics.FastqMetrics(path, structure).compute(window_bytes=window, initial_slots=64)
        check_result(result, 100, want1, clean=True)
        if first is None:
            first = result
        for name in ("barcodes", "barcode_counts", "umis", "umi_counts", "barcode_pwm", "umi_pwm"):
            assert np.array_equal(getattr(result, name), getattr(first, name)), (name, window)
    check_result(fastq_metrics.FastqMetrics([gz], structure).compute(window_bytes=1000), 100, want1, clean=True)
    both = fastq_metrics.FastqMetrics([path, path], structure).compute(window_bytes=16384, initial_slots=64)
    check_result(both, 200, want2, clean=True)
    assert np.array_equal(both.barcode_counts, 2 * first.barcode_counts) and np.array_equal(both.barcodes, first.barcodes)


@pytest.mark.parametrize("structure", ["16C", "16X10M", "3X21C"])
def test_only_one_kind(structure):
    n, want = golden(structure)
    result = fastq_metrics.FastqMetrics(R1, structure).compute(window_bytes=4096)
    check_result(result, n, want, clean=True)
    absent = (result.umis, result.umi_counts, result.umi_pwm) if "M" not in structure else \
        (result.barcodes, result.barcode_counts, result.barcode_pwm)
    assert absent[0].shape == (1, 0) and absent[1].tolist() == [100] and absent[2].shape == (0, 5)


def test_no_records(tmp_path):
    path = str(tmp_path / "empty.fastq")
    open(path, "wb").close()
    result = fastq_metrics.FastqMetrics(path, "16C10M").compute()
    check_result(result, 0, restate([], "16C10M"), clean=True)
    assert result.barcodes.shape == (0, 16) and result.umi_pwm.shape == (10, 5) and not result.umi_pwm.any()
    only_c = fastq_metrics.FastqMetrics(path, "16C").compute()
    assert only_c.umis.shape == (0, 0) and only_c.umi_counts.shape == (0,)


def test_too_long_a_barcode_raises_before_reading():
    with pytest.raises(ValueError, match="limit is 21"):
        fastq_metrics.FastqMetrics("/no/such/file.fastq", "22C")


def test_a_short_sequence_line_raises_naming_its_record(tmp_path):
    sequences = sequences_of(open(R1, "rb").read())
    sequences[57] = sequences[57][:20]
    path = str(tmp_path / "short.fastq")
    open(path, "wb").write(fastq_text(sequences))
    for window in (1000, 1 << 20):
        with pytest.raises(ValueError, match=r"record 57\b.*sequence line has 20 bytes"):
            fastq_metrics.FastqMetrics(path, "16C10M").compute(window_bytes=window)
    assert fastq_metrics.FastqMetrics(path, "16C4M").compute().n_records == 100  # 20 bases are enough here


def test_cli_end_to_end(tmp_path):
    prefix = str(tmp_path / "sample")
    assert cli_main(["FastqMetrics", "--R1", R1, "--R1", R1 + ".gz", "--read-structure", "16C10M", "--sample-id", prefix,
                     "--white-list", "/not/read", "--device", "0"]) == 0
    assert sorted(os.listdir(tmp_path)) == ["sample.barcode_distribution_XC.txt", "sample.barcode_distribution_XM.txt",
                                            "sample.numReads_perCell_XC.txt", "sample.numReads_perCell_XM.txt"]
    n, want = golden("16C10M", 2)
    for kind, (counts, pwm, other, _) in zip("CM", want):
        lines = open("%s.numReads_perCell_X%s.txt" % (prefix, kind), "rb").read().split(b"\n")
        assert lines.pop() == b""
        pairs = [ln.split(b"\t") for ln in lines]
        assert all(len(p) == 2 for p in pairs)
        check_counts([p[1] for p in pairs], [int(p[0]) for p in pairs], counts)
        assert sum(int(p[0]) for p in pairs) == n
        text = "position\tA\tC\tG\tT\tN\n" + "".join("%d\t%s\n" % (i + 1, "\t".join(str(v) for v in row))
                                                    for i, row in enumerate(pwm.tolist()))
        assert open("%s.barcode_distribution_X%s.txt" % (prefix, kind)).read() == text
