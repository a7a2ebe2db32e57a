"""BGZF FASTQ on the GPU, the parts that need none: the member scan (``sct_fq_bgzf_scan``), the CRC
routine of ``csrc/fqinflate.h`` on the host (``tests/native/libfqcrc.so``: the slices, tables and fold the
``k_fq_crc32`` kernel runs) against ``zlib.crc32``, and the ``inflate`` argument of the classes and commands.
"""
import ctypes
import gzip
import os
import random
import struct
import zlib

import numpy as np
import pytest

import deflate_craft as C
from sctools_amd import bam, fastq, fastq_metrics, fastq_process, platform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CRC_LIB = os.path.join(ROOT, "tests", "native", "libfqcrc.so")
R1 = os.path.join(ROOT, "tests", "golden", "fastq", "test_r1.fastq")


def deflate(data: bytes, level: int = 6) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def members_of(payloads):
    """[(member bytes, payload)] by the tests' own BGZF writer."""
    return [(C.bgzf_member(deflate(p), p), p) for p in payloads]


def expected_table(parts):
    """What the scan must report for members written back to back: offsets, lengths, CRCs."""
    rows, at, out = [], 0, 0
    for member, payload in parts:
        xlen = struct.unpack_from("<H", member, 10)[0]
        rows.append((at + 12 + xlen, out, len(member) - 12 - xlen - 8, len(payload), zlib.crc32(payload)))
        at += len(member)
        out += len(payload)
    return rows, at


def scan_rows(data: bytes):
    members, crcs, stopped, reason = fastq.bgzf_scan(data)
    rows = [(int(m["in_off"]), int(m["out_off"]), int(m["clen"]), int(m["isize"]), int(c)) for m, c in zip(members, crcs)]
    return rows, stopped, reason


def test_scan_reports_the_writers_own_offsets_lengths_and_crcs():
    rng = random.Random(5)
    # (65536 incompressible bytes do not fit a member: the largest one holds bytes of a 16-letter alphabet)
    parts = members_of([rng.randbytes(n) for n in (1, 997, 65280, 300)] + [bytes(rng.choices(b"ACGTNacgtn#IF:@+", k=65536))]
                       + [b"ACGT\n" * 5000])
    parts.append((C.BGZF_EOF, b""))
    data = b"".join(m for m, _ in parts)
    want, end = expected_table(parts)
    rows, stopped, reason = scan_rows(data)
    assert reason is None and stopped == end == len(data)
    assert rows == want


def test_scan_finds_bc_among_other_subfields():
    payload = b"@r\nACGT\n+\nIIII\n"
    raw = deflate(payload)
    before, after = b"XA" + struct.pack("<H", 3) + b"abc", b"ZZ" + struct.pack("<H", 0) + b"YB" + struct.pack("<H", 5) + b"12345"
    xlen = len(before) + 6 + len(after)
    total = 12 + xlen + len(raw) + 8
    member = (struct.pack("<BBBBIBBH", 31, 139, 8, 4, 0, 0, 255, xlen) + before + b"BC" + struct.pack("<HH", 2, total - 1)
              + after + raw + struct.pack("<II", zlib.crc32(payload), len(payload)))
    assert gzip.decompress(member) == payload  # a gzip member like any other
    plain = C.bgzf_member(raw, payload)
    rows, stopped, reason = scan_rows(plain + member + C.BGZF_EOF)
    assert reason is None and stopped == len(plain) + len(member) + len(C.BGZF_EOF)
    assert rows[1] == (len(plain) + 12 + xlen, len(payload), len(raw), len(payload), zlib.crc32(payload))
    assert rows[2][1:] == (2 * len(payload), 2, 0, 0)


def test_scan_of_empty_members_and_empty_files():
    parts = members_of([b"abc\n", b"", b"def"])
    rows, stopped, reason = scan_rows(b"".join(m for m, _ in parts))
    assert reason is None and [r[3] for r in rows] == [4, 0, 3] and [r[1] for r in rows] == [0, 4, 4]
    assert rows == expected_table(parts)[0]
    rows, stopped, reason = scan_rows(C.BGZF_EOF)  # only the EOF member
    assert reason is None and stopped == 28 and rows == [(18, 0, 2, 0, 0)]
    rows, stopped, reason = scan_rows(b"")
    assert reason is None and stopped == 0 and rows == []


def test_scan_says_where_a_file_stops_being_bgzf():
    parts = members_of([b"ACGT\n" * 300, b"TTTT\n" * 200])
    good = b"".join(m for m, _ in parts)
    first = len(parts[0][0])
    python_gzip = gzip.compress(b"ACGT\n" * 100)
    cases = {
        "python gzip": (python_gzip, 0, 0),
        "plain member appended": (good + python_gzip, len(good), 2),
        "member cut in half": (good[:first + (len(good) - first) // 2], first, 1),
        "bsize past the end": (good + parts[0][0][:16] + struct.pack("<H", 0xFFFF) + parts[0][0][18:], len(good), 2),
        "five trailing bytes": (good + C.BGZF_EOF + b"\0\0\0\0\0", len(good) + 28, 3),
    }
    for name, (data, at, n) in cases.items():
        rows, stopped, reason = scan_rows(data)
        assert reason == "not BGZF at byte %d" % at, name
        assert stopped == at and len(rows) == n, name
        assert rows == expected_table(parts)[0][:n] + ([(len(good) + 18, 500 * 5, 2, 0, 0)] if n == 3 else []), name


def test_scan_refuses_an_isize_no_bgzf_member_can_have():
    payload = b"ACGT\n" * 10
    good = C.bgzf_member(deflate(payload), payload)
    big = C.bgzf_member(deflate(payload), payload, isize=65537)
    assert scan_rows(good + C.bgzf_member(deflate(payload), payload, isize=65536))[2] is None
    assert scan_rows(good + big)[2] == "not BGZF at byte %d" % len(good)


def test_scan_walks_more_members_than_one_call_takes():
    n = (1 << 16) + 3
    rows, stopped, reason = scan_rows(C.BGZF_EOF * n)
    assert reason is None and stopped == 28 * n and len(rows) == n
    assert rows[-1] == (28 * (n - 1) + 18, 0, 2, 0, 0)


# ---------------------------------------------------------------- the CRC routine on the host

@pytest.fixture(scope="module")
def crc_lib():
    lib = ctypes.CDLL(CRC_LIB)  # built by the Makefile's `all`
    lib.fq_crc32_wave.restype = ctypes.c_uint32
    lib.fq_crc32_wave.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    lib.fq_crc32_many.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.fq_gf_mul.restype = lib.fq_gf_xpow.restype = ctypes.c_uint32
    lib.fq_gf_mul.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    lib.fq_gf_xpow.argtypes = [ctypes.c_uint64]
    return lib


EDGE_LENGTHS = list(range(301)) + list(range(1019, 1026)) + [4095, 4096, 4097, 65279, 65280, 65535, 65536]


def test_crc_equals_zlib_at_every_edge_length(crc_lib):
    rng = random.Random(11)
    for n in EDGE_LENGTHS:
        for data in (rng.randbytes(n), bytes(n), b"\xff" * n):
            assert crc_lib.fq_crc32_wave(data, n) == zlib.crc32(data), n


def test_crc_equals_zlib_on_random_lengths_and_seeds(crc_lib):
    rng = np.random.default_rng(12)
    pool = rng.integers(0, 256, size=1 << 20, dtype=np.uint8)  # slices begin at every alignment
    n = 10_000
    length = np.concatenate([rng.integers(0, 65537, size=n // 2), rng.integers(0, 700, size=n // 2)]).astype(np.uint32)
    off = rng.integers(0, len(pool) - 65536, size=n).astype(np.int64)
    got = np.zeros(n, dtype=np.uint32)
    assert crc_lib.fq_crc32_many(pool.ctypes.data, off.ctypes.data, length.ctypes.data, n, got.ctypes.data) == 0
    raw = pool.tobytes()
    want = np.array([zlib.crc32(raw[o:o + k]) for o, k in zip(off.tolist(), length.tolist())], dtype=np.uint32)
    assert np.array_equal(got, want)


def test_crc_pieces_are_polynomial_arithmetic(crc_lib):
    one, x = 0x80000000, 0x40000000
    assert crc_lib.fq_gf_xpow(0) == one and crc_lib.fq_gf_xpow(1) == x
    assert crc_lib.fq_gf_mul(one, 0xDEADBEEF) == 0xDEADBEEF
    assert crc_lib.fq_gf_xpow(32) == 0xEDB88320  # x^32 mod P is P without its top term
    for a, b in ((3, 5), (1000, 24), (65536 * 8, 77)):
        assert crc_lib.fq_gf_mul(crc_lib.fq_gf_xpow(a), crc_lib.fq_gf_xpow(b)) == crc_lib.fq_gf_xpow(a + b)


def test_the_librarys_own_host_crc_is_the_same_routine():
    lib = fastq.load_inflate()
    rng = random.Random(13)
    for n in (0, 1, 63, 64, 65, 1024, 65536):
        data = rng.randbytes(n)
        assert lib.sct_fq_crc32(ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), n) == zlib.crc32(data)


# ---------------------------------------------------------------- arguments

def test_header_declares_the_inflate_functions():
    import re

    text = open(os.path.join(ROOT, "include", "sct_fastq_inflate.h")).read()
    names = sorted(set(re.findall(r"^(?:int|uint32_t)\s+(sct_fq_\w+)\(", text, flags=re.M)))
    assert names == sorted(fastq.INFLATE_PROTOTYPES)
    lib = fastq.load_inflate()
    assert lib is fastq.load()
    for name in names:
        assert hasattr(lib, name), name
    assert int(re.search(r"#define SCT_FQ_INFLATE_SLACK (\d+)", text).group(1)) == fastq.INFLATE_SLACK
    assert int(re.search(r"#define SCT_FQ_ST_CRC (\d+)", text).group(1)) == fastq.ST_CRC
    assert int(re.search(r"#define SCT_FQ_ENOTBGZF (-\d+)", text).group(1)) == fastq.NOT_BGZF
    assert fastq.MEMBER.itemsize == 24


def test_inflate_refuses_a_buffer_without_the_slack_and_members_outside_their_buffers():
    lib = fastq.load_inflate()
    p = ctypes.c_void_p
    members = np.zeros(1, dtype=fastq.MEMBER)
    members[0] = (18, 0, 100, 200)
    crcs = np.zeros(1, dtype=np.uint32)
    need = ctypes.c_size_t(0)
    assert lib.sct_fq_inflate_workspace_size(1, ctypes.byref(need)) == 0 and need.value >= 28
    assert lib.sct_fq_inflate_workspace_size(-1, ctypes.byref(need)) == -1

    def call(comp=4096, comp_bytes=1000, capacity=1000 + 65536, text_capacity=1000, text_off=0, work=1 << 12,
             status=1 << 13, summary=1 << 14):
        return lib.sct_fq_inflate(p(comp), comp_bytes, capacity, members.ctypes.data, crcs.ctypes.data, 1, p(1 << 16),
                                  text_capacity, text_off, p(work), 64, p(status), p(summary), None)

    err = lib.sct_fq_last_error
    assert call(capacity=1000 + 65535) == -2 and b"slack" in err()  # nothing is launched: no GPU is needed to say so
    assert call(capacity=999) == -2
    assert call(comp=4098) == -1 and b"4-byte aligned" in err()
    assert call(comp_bytes=117, capacity=117 + 65536) == -1 and b"deflate data leaves" in err()  # 18 + 100 > 117
    assert call(text_capacity=199) == -1 and b"payload leaves" in err()
    assert call(text_capacity=1000, text_off=801) == -1 and b"payload leaves" in err()
    assert call(text_off=1001) == -1
    assert call(summary=(1 << 14) + 2) == -1 and b"summary" in err()
    members[0]["isize"] = 65537
    assert call(text_capacity=1 << 20) == -1 and b"isize" in err()


def test_inflate_takes_auto_and_host_only(tmp_path):
    for bad in ("device", "gpu", None, ""):
        with pytest.raises(ValueError, match="inflate must be one of"):
            fastq_metrics.FastqMetrics(R1, "16C10M", inflate=bad)
        with pytest.raises(ValueError, match="inflate must be one of"):
            fastq_process.FastqProcess(R1, R1, barcode_length=16, umi_length=10, num_shards=1, inflate=bad)
        with pytest.raises(ValueError, match="inflate must be one of"):
            next(fastq.EmbeddedBarcodeGenerator(R1, [platform.TenXV2.cell_barcode]).columns(inflate=bad))
        if bad is not None:  # (the Tagger's None is the default)
            with pytest.raises(ValueError, match="inflate must be one of"):
                bam.Tagger(R1, inflate=bad)
    for ok in fastq.INFLATE_MODES:
        assert fastq_metrics.FastqMetrics(R1, "16C10M", inflate=ok).inflate == ok
        assert fastq_process.FastqProcess(R1, R1, barcode_length=16, umi_length=10, num_shards=1, inflate=ok).inflate == ok
    assert fastq.DEFAULT_INFLATE in fastq.INFLATE_MODES
    assert fastq_metrics.FastqMetrics(R1, "16C10M").inflated_by == {}


def test_the_four_commands_parse_inflate(monkeypatch, tmp_path):
    seen = []

    class Metrics:
        def __init__(self, *a, **kw):
            seen.append(("FastqMetrics", kw["inflate"]))

        def compute(self, **kw):
            raise StopIteration

    class Process:
        def __init__(self, *a, **kw):
            seen.append(("FastqProcess", kw["inflate"]))

        def run(self, **kw):
            raise StopIteration

    monkeypatch.setattr(fastq_metrics, "FastqMetrics", Metrics)
    monkeypatch.setattr(fastq_process, "FastqProcess", Process)
    for cls in (platform.TenXV2, platform.BarcodePlatform):
        monkeypatch.setattr(cls, "_tag_bamfile", classmethod(
            lambda c, u2, out, gens, device=None, inflate=None: seen.append((c.__name__, inflate))))
        monkeypatch.setattr(cls, "_make_tag_generators", classmethod(lambda c, *a, **kw: []))
    commands = {
        "FastqMetrics": ["--R1", R1, "--read-structure", "16C10M", "--sample-id", "x"],
        "FastqProcess": ["--R1", R1, "--R2", R1, "--barcode-length", "16", "--umi-length", "10"],
        "FastqSlideseq": ["--R1", R1, "--R2", R1, "--read-structure", "8C18X6C9M1X"],
        "Attach10xBarcodes": ["--r1", R1, "--u2", "u.bam", "-o", "o.bam"],
        "AttachBarcodes": ["--r1", R1, "--u2", "u.bam", "-o", "o.bam", "--cell-barcode-start-position", "0",
                           "--cell-barcode-length", "16"],
    }
    for name, args in commands.items():
        for given, want in ((["--inflate", "host"], "host"), (["--inflate", "auto"], "auto"), ([], fastq.DEFAULT_INFLATE)):
            seen.clear()
            try:
                platform.COMMANDS[name](args + given)
            except StopIteration:
                pass
            assert [w for _, w in seen] == [want], (name, given, seen)
        with pytest.raises(SystemExit):
            platform.COMMANDS[name](args + ["--inflate", "device"])
