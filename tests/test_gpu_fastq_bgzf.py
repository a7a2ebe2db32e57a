"""BGZF-compressed FASTQ inflated on the GPU (``sct_fq_inflate``: ``k_inflate`` and ``k_fq_crc32``), from the
kernels up to the tools.  The reference for every byte is the host path: ``reader.open_binary(path).read()``,
zlib and ``zlib.crc32``.  A test that means to exercise the device path asserts that ``inflated_by`` says
``"device"`` and that nothing was declined: passing by falling back would show nothing.

A BGZF member holds at most 64 KiB with its framing, so 65536 incompressible bytes do not fit one
(``deflate_cases``'s docstring): the 65536-byte members here hold bytes of a 16-letter alphabet, or a
compressed part followed by a stored block of random bytes.
"""
import gzip
import os
import random
import re
import struct
import zlib

import numpy as np
import pytest

import deflate_cases as K
import deflate_craft as C
from sctools_amd import bam, fastq, fastq_metrics, fastq_process as fp, platform, reader
from sctools_amd.__main__ import main as cli_main

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R1 = os.path.join(ROOT, "tests", "golden", "fastq", "test_r1.fastq")
I7 = os.path.join(ROOT, "tests", "golden", "fastq", "test_i7.fastq")
R2 = os.path.join(ROOT, "tests", "golden", "fastq_process", "test_r2.fastq")
R2_BAM = os.path.join(ROOT, "tests", "golden", "fastq", "test_r2.bam")
WHITELIST = os.path.join(ROOT, "tests", "golden", "barcode", "1k-august-2016.txt")
SPANS = [(0, 16), (16, 26), (3, 4)]
CRC_BIT = 1 << fastq.ST_CRC


def deflate(data: bytes, level: int = 6) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def bgzf_bytes(data: bytes, block: int, eof: bool = True) -> bytes:
    out = b"".join(C.bgzf_member(deflate(data[i:i + block]), data[i:i + block]) for i in range(0, len(data), block))
    return out + (C.BGZF_EOF if eof else b"")


def write(path, data: bytes) -> str:
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def all_device(obj, *paths):
    assert obj.declined == {}, obj.declined
    for p in paths:
        assert obj.inflated_by[p] == "device", (p, obj.inflated_by)


def n_records_of(stream: bytes) -> int:
    lines = stream.split(b"\n")
    if not lines[-1]:
        lines.pop()
    return len(lines) // 4


def records_end(data: bytes, n: int) -> int:
    """The offset behind the first n records (4 n lines) of data."""
    ends = np.flatnonzero(np.frombuffer(data, dtype=np.uint8) == 10)
    return int(ends[4 * n - 1]) + 1 if 4 * n <= len(ends) else len(data)


def walk_windows(path, text, window_bytes, inflate="auto"):
    """Checks every window of ``path`` against ``text``; returns (the TextWindows, the windows' n_bytes, the
    columns of ``SPANS`` over all windows)."""
    windows = fastq.TextWindows([path], window_bytes=window_bytes, inflate=inflate)
    at, total, sizes, cols = 0, 0, [], [([], []) for _ in SPANS]
    for window in windows:
        got = window.text[:window.n_bytes].cpu().numpy().tobytes()
        assert got == text[at:at + window.n_bytes], ("window at", at)
        assert window.host.tobytes() == got
        assert len(window) == 5
        t, n_bytes, n, work, _ = window  # the unpacking the extractors use
        assert n_bytes == window.n_bytes and n == window.n_records
        columns, first_flagged, _ = fastq.extract_spans(window, SPANS)
        assert first_flagged == -1
        for k, (seq, qual) in enumerate(columns):
            cols[k][0].append(seq.cpu().numpy())
            cols[k][1].append(qual.cpu().numpy())
        sizes.append(window.n_bytes)
        total += window.n_records
        at += records_end(got, window.n_records)
    assert total == n_records_of(text)
    return windows, sizes, [(np.concatenate(s), np.concatenate(q)) for s, q in cols]


# ---------------------------------------------------------------- 1. windows

def test_windows_of_members_that_end_mid_line_and_mid_record(tmp_path):
    text = open(R1, "rb").read() * 30
    assert n_records_of(text) == 3000
    path = write(tmp_path / "r1.fastq.gz", bgzf_bytes(text, 997))
    plain = write(tmp_path / "r1.fastq", text)
    windows, sizes, cols = walk_windows(path, text, 5000)
    all_device(windows, path)
    assert len(sizes) > 50 and max(sizes) <= 5000
    _, _, want = walk_windows(plain, text, 5000, inflate="host")
    for (seq, qual), (wseq, wqual) in zip(cols, want):
        assert np.array_equal(seq, wseq) and np.array_equal(qual, wqual)
    hosted, _, again = walk_windows(path, text, 5000, inflate="host")
    assert hosted.inflated_by == {path: "host"} and hosted.declined == {}
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(again, want))


def test_a_window_smaller_than_one_member_grows(tmp_path):
    text = (open(R1, "rb").read() * 12)[:65536]
    assert len(text) == 65536 and not text.endswith(b"\n")
    path = write(tmp_path / "one.fastq.gz", bgzf_bytes(text, 65536))
    assert len(fastq.bgzf_scan(open(path, "rb").read())[0]) == 2  # the member and the EOF member
    windows, sizes, _ = walk_windows(path, text + b"\n", 2000)  # (a file that ends mid-line gets its newline)
    all_device(windows, path)
    assert sizes[0] >= 65536


# ---------------------------------------------------------------- 2. crafted members

def crafted_file(members):
    data, offs = bytearray(), []
    for m in members:
        offs.append(len(data) + 18)
        data += K.bgzf(m)
    return bytes(data) + C.BGZF_EOF, offs


@pytest.mark.parametrize("name", list(K.VALID))
def test_valid_crafted_members(tmp_path, name):
    members = K.VALID[name]()
    data, offs = crafted_file(members)
    got = fastq.bgzf_inflate(write(tmp_path / "crafted.gz", data))
    assert got is not None, fastq.last_error()
    at = 0
    for i, m in enumerate(members):  # member by member, so a failure names the member
        assert got[at:at + m.isize] == m.payload, (name, i)
        at += m.isize
    assert len(got) == at
    if name == "framing":
        assert {o & 3 for o in offs} == {0, 1, 2, 3}


@pytest.mark.parametrize("name", list(K.INVALID))
def test_invalid_crafted_member_declines_with_its_status(tmp_path, name):
    build, status = K.INVALID[name]
    rng = random.Random(3)
    good = [K.M(deflate(p), p, zlib.crc32(p), len(p)) for p in (rng.randbytes(700), b"ACGT\n" * 999, rng.randbytes(5))]
    data, _ = crafted_file(good[:2] + [build()] + good[2:])
    assert fastq.bgzf_inflate(write(tmp_path / "bad.gz", data)) is None
    found = re.fullmatch(r"status mask 0x([0-9a-f]+), first failed member (\d+)", fastq.last_error())
    assert found, fastq.last_error()
    mask = int(found.group(1), 16)
    assert int(found.group(2)) == 2
    assert mask & (1 << status) if status is not None else mask != 0
    assert not mask & CRC_BIT  # a member that did not inflate is not judged by its CRC


# ---------------------------------------------------------------- 3. the CRC kernel at its edges

EDGE_SIZES = (0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 65279, 65280, 65536)


def stored_member(payload: bytes, rng) -> bytes:
    """A member whose data ends in one stored block: all of it, or for 65536 bytes (too many for a stored
    block in a member) the bytes behind a compressed first part."""
    head = b""
    tail = payload
    if len(payload) > 65280:
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        head = c.compress(payload[:45000]) + c.flush(zlib.Z_FULL_FLUSH)  # ends on a byte boundary
        tail = payload[45000:]
    raw = head + b"\x01" + struct.pack("<HH", len(tail), len(tail) ^ 0xFFFF) + tail
    assert zlib.decompress(raw, -15) == payload
    return C.bgzf_member(raw, payload)


@pytest.fixture(scope="module")
def edge_file():
    rng = random.Random(17)
    payloads = [rng.randbytes(n) if n <= 65280 else bytes(rng.choices(b"ACGTNacgtn#IF:@+", k=45000)) + rng.randbytes(n - 45000)
                for n in EDGE_SIZES]
    members = [stored_member(p, rng) for p in payloads]
    return payloads, members


def test_crc_kernel_accepts_every_edge_size(tmp_path, edge_file):
    payloads, members = edge_file
    path = write(tmp_path / "edges.gz", b"".join(members) + C.BGZF_EOF)
    assert gzip.open(path, "rb").read() == b"".join(payloads)
    got = fastq.bgzf_inflate(path)
    assert got is not None, fastq.last_error()
    assert got == b"".join(payloads)


@pytest.mark.parametrize("k", range(len(EDGE_SIZES)), ids=["isize%d" % n for n in EDGE_SIZES])
def test_crc_kernel_names_the_member_whose_crc_or_data_is_off_by_one_bit(tmp_path, edge_file, k):
    payloads, members = edge_file
    rng = random.Random(100 + k)
    start = sum(len(m) for m in members[:k])
    end = start + len(members[k])
    flips = [end - 8 + rng.randrange(4)]  # a byte of the stored CRC
    if EDGE_SIZES[k]:
        flips.append(end - 9 - rng.randrange(min(EDGE_SIZES[k], 20000)))  # a byte of the last stored block's data
    for at in flips:
        data = bytearray(b"".join(members) + C.BGZF_EOF)
        data[at] ^= 1 << rng.randrange(8)
        path = write(tmp_path / "flip.gz", bytes(data))
        assert fastq.bgzf_scan(bytes(data))[3] is None  # the header still looks right
        assert fastq.bgzf_inflate(path) is None
        assert fastq.last_error() == "status mask 0x%x, first failed member %d" % (CRC_BIT, k), (at - end)
        with pytest.raises(gzip.BadGzipFile, match="CRC check failed"):
            gzip.open(path, "rb").read()


# ---------------------------------------------------------------- 4. errors are the host's

def broken_files(tmp_path):
    text = open(R1, "rb").read()
    members = [C.bgzf_member(deflate(text[i:i + 2000]), text[i:i + 2000]) for i in range(0, len(text), 2000)]
    assert len(members) >= 4
    at = sum(len(m) for m in members[:3])  # the end of member 2

    def patched(offset, value):
        data = bytearray(b"".join(members) + C.BGZF_EOF)
        data[at + offset:at + offset + 4] = struct.pack("<I", value)
        return bytes(data)

    crc, isize = struct.unpack_from("<II", members[2], len(members[2]) - 8)
    yield "crc", write(tmp_path / "crc.fastq.gz", patched(-8, crc ^ 0x10)), True
    yield "isize", write(tmp_path / "isize.fastq.gz", patched(-4, isize - 1)), True
    bad = K.bgzf(K.INVALID["btype-3"][0]())
    yield "deflate", write(tmp_path / "deflate.fastq.gz", b"".join(members[:2]) + bad + b"".join(members[2:]) + C.BGZF_EOF), True
    whole = b"".join(members)
    yield "truncated", write(tmp_path / "cut.fastq.gz", whole[:len(whole) - len(members[-1]) // 2]), False


def test_a_broken_file_raises_what_the_host_reader_raises(tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    for name, path, device_sees_it in broken_files(tmp_path):
        with pytest.raises(Exception) as host:
            reader.open_binary(path).read()
        assert isinstance(host.value, (gzip.BadGzipFile, zlib.error, EOFError)), name
        metrics = fastq_metrics.FastqMetrics(path, "16C10M")
        with pytest.raises(Exception) as device:
            metrics.compute()
        assert type(device.value) is type(host.value), (name, device.value)
        assert str(device.value) == str(host.value), name
        assert (path in metrics.declined) == device_sees_it, (name, metrics.declined)
        if device_sees_it:
            assert metrics.declined[path].startswith("status mask 0x"), name
        with pytest.raises(type(host.value)):
            fp.FastqProcess([path], [R2], [I7], barcode_length=16, umi_length=10, num_shards=2, output_dir=str(out)).run()
        assert [n for n in os.listdir(out) if n.startswith(("subfile_", "fastq_R"))] == [], name


# ---------------------------------------------------------------- 5. the tools agree with themselves

@pytest.fixture(scope="module")
def copies(tmp_path_factory):
    """The golden R1 / I1 / R2 as BGZF files with members of 4,096 bytes."""
    d = tmp_path_factory.mktemp("bgzf")
    return {name: write(d / (name + ".fastq.gz"), bgzf_bytes(open(src, "rb").read(), 4096))
            for name, src in (("r1", R1), ("i1", I7), ("r2", R2))}


def same_result(a, b):
    fields = sorted(vars(a))
    assert fields == sorted(vars(b)) and "barcode_counts" in fields and "umi_pwm" in fields
    for field in fields:
        x, y = getattr(a, field), getattr(b, field)
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, field


def test_fastq_metrics_on_bgzf_equals_plain(tmp_path, copies):
    want = fastq_metrics.FastqMetrics(R1, "16C10M").compute()
    want_files = [open(p, "rb").read() for p in want.write(str(tmp_path / "plain"))]
    for mode in ("auto", "host"):
        metrics = fastq_metrics.FastqMetrics(copies["r1"], "16C10M", inflate=mode)
        got = metrics.compute(window_bytes=3000)
        same_result(got, want)
        assert [open(p, "rb").read() for p in got.write(str(tmp_path / mode))] == want_files
        if mode == "auto":
            all_device(metrics, copies["r1"])
        else:
            assert metrics.inflated_by == {copies["r1"]: "host"} and metrics.declined == {}
    assert want.n_records == 100
    out = tmp_path / "cli"
    assert cli_main(["FastqMetrics", "--R1", copies["r1"], "--read-structure", "16C10M", "--sample-id", str(out),
                     "--inflate", "auto"]) == 0
    assert [open(p, "rb").read() for p in sorted(str(p) for p in tmp_path.glob("cli.*"))] == \
        [open(p, "rb").read() for p in sorted(str(p) for p in tmp_path.glob("plain.*"))]


@pytest.mark.parametrize("fmt", ["BAM", "FASTQ"])
def test_fastq_process_on_bgzf_equals_plain(tmp_path, copies, fmt):
    def run(name, r1, r2, i1, **kw):
        out = tmp_path / name
        out.mkdir()
        job = fp.FastqProcess([r1], [r2], [i1], whitelist=WHITELIST, barcode_length=16, umi_length=10, num_shards=4,
                              output_format=fmt, output_dir=str(out), **kw)
        return job, job.run()

    _, want = run("plain", R1, R2, I7)
    for mode in ("auto", "host"):
        job, got = run(mode, copies["r1"], copies["r2"], copies["i1"], inflate=mode)
        assert got[1:] == want[1:] and got.n_reads == 100
        for a, b in zip(got.paths, want.paths):
            assert gzip.open(a, "rb").read() == gzip.open(b, "rb").read(), (mode, a)
        if mode == "auto":
            all_device(job, copies["r1"], copies["r2"], copies["i1"])
        else:
            assert job.inflated_by == {copies[k]: "host" for k in ("r1", "r2", "i1")} and job.declined == {}


def tagged_payload(path) -> bytes:
    return gzip.open(path, "rb").read()


def test_attach_commands_on_bgzf_equal_plain(tmp_path, copies):
    def tenx(name, r1, i1, mode):
        out = str(tmp_path / (name + ".bam"))
        generators = platform.TenXV2._make_tag_generators(r1, i1, WHITELIST)
        bam.Tagger(R2_BAM, inflate=mode).tag(out, generators)
        return tagged_payload(out), generators

    want, _ = tenx("plain", R1, I7, "auto")
    got, generators = tenx("auto", copies["r1"], copies["i1"], "auto")
    assert got == want
    all_device(generators[0], copies["r1"])
    all_device(generators[1], copies["i1"])
    got, generators = tenx("host", copies["r1"], copies["i1"], "host")
    assert got == want
    assert generators[0].inflated_by == {copies["r1"]: "host"} and generators[1].inflated_by == {copies["i1"]: "host"}

    def cli(command, name, r1, i1, *more):
        out = str(tmp_path / (name + ".bam"))
        try:
            assert cli_main([command, "--r1", r1, "--i1", i1, "--u2", R2_BAM, "-o", out, "-w", WHITELIST] + list(more)) == 0
        finally:
            bp = platform.BarcodePlatform
            bp.cell_barcode = bp.molecule_barcode = bp.sample_barcode = None
        return tagged_payload(out)

    assert cli("Attach10xBarcodes", "c10", copies["r1"], copies["i1"]) == want
    assert cli("Attach10xBarcodes", "c10h", copies["r1"], copies["i1"], "--inflate", "host") == want
    layout = ["--cell-barcode-start-position", "0", "--cell-barcode-length", "16", "--molecule-barcode-start-position", "16",
              "--molecule-barcode-length", "10", "--sample-barcode-start-position", "0", "--sample-barcode-length", "8"]
    plain = cli("AttachBarcodes", "ab", R1, I7, *layout)
    assert cli("AttachBarcodes", "abz", copies["r1"], copies["i1"], *layout) == plain
    assert cli("AttachBarcodes", "abh", copies["r1"], copies["i1"], "--inflate", "host", *layout) == plain
    # the generators AttachBarcodes builds, asked who inflated
    bp = platform.BarcodePlatform
    try:
        bp.cell_barcode, bp.molecule_barcode = platform.TenXV2.cell_barcode, platform.TenXV2.molecule_barcode
        generators = bp._make_tag_generators(copies["r1"], None, WHITELIST)
        bam.Tagger(R2_BAM).tag(str(tmp_path / "abg.bam"), generators)
        all_device(generators[0], copies["r1"])
    finally:
        bp.cell_barcode = bp.molecule_barcode = bp.sample_barcode = None


# ---------------------------------------------------------------- 6. mixed lists

def test_a_list_of_plain_bgzf_and_gzip_files_is_one_stream(tmp_path, copies):
    text = open(R1, "rb").read()
    assert text.endswith(b"\n")
    no_newline = write(tmp_path / "nonl.fastq.gz", bgzf_bytes(text[:-1], 1500))
    python_gzip = write(tmp_path / "py.fastq.gz", gzip.compress(text))
    files = [R1, no_newline, python_gzip, copies["r1"]]
    for window_bytes in (256 << 20, 3000):
        want = fastq_metrics.FastqMetrics(files, "16C10M", inflate="host").compute(window_bytes=window_bytes)
        metrics = fastq_metrics.FastqMetrics(files, "16C10M")
        got = metrics.compute(window_bytes=window_bytes)
        same_result(got, want)
        assert got.n_records == 400  # the missing newline was supplied: no record ran into the next file's
        assert metrics.inflated_by == {R1: "host", no_newline: "device", python_gzip: "host", copies["r1"]: "device"}
        assert metrics.declined == {}
    one = fastq_metrics.FastqMetrics(R1, "16C10M").compute()
    assert np.array_equal(got.barcode_counts, 4 * one.barcode_counts)


def test_a_bgzf_file_with_a_foreign_member_or_trailing_bytes_is_the_hosts(tmp_path):
    text = open(R1, "rb").read()
    foreign = write(tmp_path / "foreign.fastq.gz", bgzf_bytes(text, 4096, eof=False) + gzip.compress(text))
    metrics = fastq_metrics.FastqMetrics(foreign, "16C10M")
    assert metrics.compute().n_records == 200
    assert metrics.inflated_by == {foreign: "host"} and metrics.declined == {}


# ---------------------------------------------------------------- 7. the project's own output

def test_the_fastq_shards_this_project_writes_are_read_back_on_the_device(tmp_path):
    result = fp.FastqProcess([R1], [R2], [I7], barcode_length=16, umi_length=10, num_shards=2, output_format="FASTQ",
                             output_dir=str(tmp_path)).run()
    shards = result.paths[:2]
    assert all(os.path.basename(p).startswith("fastq_R1_") for p in shards) and result.n_reads == 100
    counts = []
    for path in shards:
        metrics = fastq_metrics.FastqMetrics(path, "16C10M")
        counts.append(metrics.compute().n_records)
        all_device(metrics, path)
    assert counts == result.shard_counts and sum(counts) == result.n_reads
    both = fastq_metrics.FastqMetrics(shards, "16C10M")
    want = fastq_metrics.FastqMetrics(R1, "16C10M").compute()
    same_result(both.compute(), want)  # the shards together hold R1's barcodes
    all_device(both, *shards)


# ---------------------------------------------------------------- 8. early stop

def test_a_bgzf_r1_longer_than_the_bam_ends_cleanly(tmp_path):
    text = open(R1, "rb").read() * 3
    plain = write(tmp_path / "r1x3.fastq", text)
    packed = write(tmp_path / "r1x3.fastq.gz", bgzf_bytes(text, 4096))
    outs = []
    for name, r1 in (("plain", plain), ("bgzf", packed)):
        out = str(tmp_path / (name + ".bam"))
        generator = fastq.EmbeddedBarcodeGenerator(r1, [platform.TenXV2.cell_barcode, platform.TenXV2.molecule_barcode])
        tagger = bam.Tagger(R2_BAM)
        tagger.tag(out, [generator])
        outs.append(tagged_payload(out))
        assert generator.declined == {}
    assert outs[0] == outs[1]
    assert len(list(bam.open_alignments(str(tmp_path / "bgzf.bam"), "rb"))) == 100
    sizes = [w["CR"].shape[0] for w in fastq.EmbeddedBarcodeGenerator(packed, [platform.TenXV2.cell_barcode]).columns(
        window_bytes=2000, max_records=33)]
    assert sum(sizes) == 33
