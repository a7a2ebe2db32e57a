"""FastqProcess on the GPU: the ``sct_fqp_*`` calls one at a time on crafted input, and the command end
to end on the bundled triple.

The expectation is tests/fqp_expect.py: plain Python that splits the text, builds the record bytes,
hashes and concatenates per shard in input order.  The reference binary needs libStatGen and
gzstream, which are not at hand; its own output for the bundled triple is
``tests/golden/bam/test_r2_tagged.bam`` (written with an 8-base UMI span, so the run with the 10-base
UMI is compared on the first 8 bases of ``UR``/``UY`` and a run with ``--umi-length 8`` on all of them).
"""
import functools
import gzip
import os
import random
from collections import Counter

import numpy as np
import pytest

import fqp_expect as E
from sctools_amd import bam, barcode, fastq, fastq_process as fp
from sctools_amd.__main__ import main as cli_main

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R1 = os.path.join(ROOT, "tests", "golden", "fastq", "test_r1.fastq")
I7 = os.path.join(ROOT, "tests", "golden", "fastq", "test_i7.fastq")
R2 = os.path.join(ROOT, "tests", "golden", "fastq_process", "test_r2.fastq")
TAGGED = os.path.join(ROOT, "tests", "golden", "bam", "test_r2_tagged.bam")
WHITELIST = os.path.join(ROOT, "tests", "golden", "barcode", "1k-august-2016.txt")
TILE = fastq.TILE_BYTES
BASES = b"ACGT"


def dev_tensor(array):
    import torch

    return torch.from_numpy(np.array(array)).cuda()  # (a copy: the array may be a read-only view of bytes)


# ---- lines ----

def device_lines(text: bytes, is_last: bool = True):
    window = fp.text_window(text, is_last)
    off, length, first_flagged, flags = fp.window_lines(window)
    return window.n_records, off.cpu().numpy(), length.cpu().numpy(), first_flagged, flags.cpu().numpy()


def check_lines(text: bytes, is_last: bool = True):
    want = E.lines_of(text, is_last)
    n, off, length, first_flagged, flags = device_lines(text, is_last)
    assert n == len(want)
    for r, (ident, seq, qual, flag) in enumerate(want):
        got = [(int(off[r, k]), int(length[r, k])) for k in range(3)]
        # a line's offset is compared where the line has bytes; an empty line has no first byte
        for k, (start, size) in enumerate((ident, seq, qual)):
            assert got[k][1] == size, (r, k)
            if size:
                assert got[k][0] == start, (r, k)
        assert int(flags[r]) == flag, r
    flagged = [r for r, w in enumerate(want) if w[3]]
    assert first_flagged == (flagged[0] if flagged else -1)
    return want


def make_record(rng, name_length=None, read_length=None, description=None):
    name_length = rng.randint(1, 200) if name_length is None else name_length
    read_length = rng.randint(1, 151) if read_length is None else read_length
    name = bytes(rng.choice(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789:_-") for _ in range(name_length))
    if description is None:
        description = rng.random() < 0.5
    if description:
        name += b" " + bytes(rng.choice(b"12:NY ") for _ in range(rng.randint(0, 12)))
    seq = bytes(rng.choice(b"ACGTNacgtn") for _ in range(read_length))
    qual = bytes(rng.randint(33, 74) for _ in range(read_length))
    return b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n"


def make_text(n, seed, **kw):
    rng = random.Random(seed)
    return b"".join(make_record(rng, **kw) for _ in range(n))


def test_lines_of_generated_records_over_several_tiles():
    rng = random.Random(1)
    records = [make_record(rng, name_length=1 + i % 200, read_length=1 + i % 151, description=bool(i & 1))
               for i in range(400)]
    text = b"".join(records)
    assert len(text) > 3 * TILE
    want = check_lines(text)
    assert {w[1][1] for w in want} == set(range(1, 152)) and not any(w[3] for w in want)


def shifted_text(kind: int, target: int, n=300, seed=5):
    """A text whose first ``\\n`` of line kind ``kind`` (0 name .. 3 quality) at or after ``target`` is moved
    exactly onto ``target`` by lengthening the first record's name."""
    tail = make_text(n, seed + 1)
    for pad in range(1, 700):
        text = make_text(1, seed, name_length=pad, description=False) + tail
        at, line = -1, -1
        while True:
            at = text.find(b"\n", at + 1)
            line += 1
            if at < 0 or (at >= target and line % 4 == kind):
                break
        if at == target:
            return text
    raise AssertionError("no padding puts a newline of kind %d at %d" % (kind, target))


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("target", [TILE - 1, TILE, 2 * TILE - 1, 2 * TILE])
def test_newline_as_the_last_and_as_the_first_byte_of_a_tile(kind, target):
    check_lines(shifted_text(kind, target))


@pytest.mark.parametrize("cut", [1, 75, 150])
def test_a_sequence_line_straddles_a_tile_boundary(cut):
    tail = make_text(150, 12, read_length=151)
    for pad in range(1, 700):
        text = make_text(1, 11, name_length=pad, description=False) + tail
        if any(i % 4 == 1 and (s, e) == (TILE - cut, TILE - cut + 151) for i, (s, e) in enumerate(E.split_lines(text))):
            break
    else:
        raise AssertionError("no padding puts a sequence line %d bytes before the tile's end" % cut)
    check_lines(text)


def test_a_name_line_of_40_kb_is_flagged_and_its_neighbours_are_not():
    long_name = b"@" + b"N" * 40000 + b"\nACGT\n+\nIIII\n"
    text = make_text(30, 21) + long_name + make_text(30, 22)
    want = check_lines(text)
    assert [r for r, w in enumerate(want) if w[3]] == [30] and want[30][3] == fp.BAD_IDENTIFIER
    # with a description the identifier is short again and nothing is flagged
    text = make_text(30, 21) + b"@id " + b"N" * 40000 + b"\nACGT\n+\nIIII\n" + make_text(30, 22)
    assert not any(w[3] for w in check_lines(text))


def test_crlf_lines_lose_their_carriage_return():
    text = make_text(120, 31).replace(b"\n", b"\r\n")
    want = check_lines(text)
    assert not any(w[3] for w in want)
    assert E.fields_of(text) == E.fields_of(text.replace(b"\r\n", b"\n"))


@pytest.mark.parametrize("is_last", [True, False])
def test_a_last_line_without_a_newline(is_last):
    text = make_text(70, 41)[:-1]
    want = check_lines(text, is_last)
    assert len(want) == (70 if is_last else 69)
    assert len(check_lines(b"@a\nAC\n+\nII", True)) == 1 and len(check_lines(b"@a\nAC\n+\nII", False)) == 0


def test_every_flag_marks_exactly_its_record():
    records = [make_record(random.Random(50 + i)) for i in range(90)]
    records[80] = b"@x\nACGT\n+\nIII\n"           # lengths differ
    records[61] = b"name without at\nAC\n+\nII\n"  # no '@'
    records[47] = b"@empty\n\n+\n\n"               # empty sequence
    records[33] = b"@low\nACGT\n+\nII I\n"         # a quality byte of 32
    records[75] = b"@ description only\nAC\n+\nII\n"  # empty identifier
    text = b"".join(records)
    n, off, length, first_flagged, flags = device_lines(text)
    assert n == 90 and first_flagged == 33
    want = {33: fp.LOW_QUALITY, 47: fp.EMPTY_SEQUENCE, 61: fp.BAD_NAME, 75: fp.BAD_IDENTIFIER, 80: fp.LENGTH_MISMATCH}
    assert {r: int(f) for r, f in enumerate(flags) if f} == want
    check_lines(text)


# ---- shard ----

def random_barcodes(n, length, seed, alphabet=BASES):
    rng = np.random.RandomState(seed)
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.randint(0, len(alphabet), size=(n, length))]


def test_the_device_shard_is_the_hash_modulo_the_shard_count():
    for length in range(1, 32):
        rows = random_barcodes(10000, length, 100 + length, b"ACGTN")
        hashes = E.native_hashes([r.tobytes() for r in rows])  # std::hash<std::string> itself
        raw = dev_tensor(rows)
        for n_shards in (1, 2, 7, 1024):
            shard, counts = fp.shards(raw, None, None, n_shards)
            assert np.array_equal(shard.cpu().numpy().astype(np.uint64), hashes % np.uint64(n_shards)), (length, n_shards)
            assert counts == (0, 0, len(rows))


def test_bucket_barcode_and_counts_with_a_whitelist(tmp_path):
    rng = random.Random(7)
    length = 16
    pool = [bytes(rng.choice(BASES) for _ in range(length)) for _ in range(600)]
    listed = pool[:300]
    path = tmp_path / "whitelist.txt"
    path.write_bytes(b"".join(b + b"\n" for b in listed))
    queries = []
    for i in range(3000):
        b = bytearray(rng.choice(pool))
        kind = i % 4
        if kind == 1:  # a single-base mutant
            at = rng.randrange(length)
            b[at] = rng.choice([x for x in BASES if x != b[at]])
        elif kind == 2:  # a single N
            b[rng.randrange(length)] = ord("N")
        elif kind == 3:  # two mutations
            for at in rng.sample(range(length), 2):
                b[at] = rng.choice([x for x in BASES if x != b[at]])
        queries.append(bytes(b))
    corrector = barcode.ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(str(path))
    raw = dev_tensor(np.frombuffer(b"".join(queries), dtype=np.uint8).reshape(len(queries), length))
    index, corrected = corrector.correct_barcodes(raw, return_corrected=True)
    shard, counts = fp.shards(raw, corrected, index, 1024)
    want_shard, want_counts = [], [0, 0, 0]
    for q in queries:
        try:
            fixed = corrector.get_corrected_barcode(q.decode()).encode()
        except KeyError:
            want_counts[2] += 1
            want_shard.append(E.shard_of(q, 1024))
            continue
        want_counts[0 if fixed == q else 1] += 1
        want_shard.append(E.shard_of(fixed, 1024))
    assert min(want_counts) > 100  # every class is there
    assert shard.cpu().tolist() == want_shard  # (1024 shards: a wrong bucket barcode would show)
    assert counts == tuple(want_counts)


# ---- plan and emit ----

@functools.lru_cache(maxsize=None)
def synthetic(n):
    """n records: the R2 text, an I1 text, random barcode columns, and CB for every third record."""
    rng = random.Random(1000 + n)
    r2 = b"".join(make_record(rng) for _ in range(n))
    i1 = b"".join(make_record(rng, name_length=5, read_length=rng.randint(1, 12)) for _ in range(n))
    cols = {k: random_barcodes(n, length, 2000 + n + i, b"ACGTNFJ#") for i, (k, length) in
            enumerate((("cr", 16), ("cy", 16), ("ur", 10), ("uy", 10), ("cb", 16)))}
    index = np.array([i if i % 3 == 0 else -1 for i in range(n)], dtype=np.int32)
    return r2, i1, cols, index


def expected_shards(n, shard, n_shards, with_i1, with_cb):
    r2, i1, cols, index = synthetic(n)
    reads, indexes = E.fields_of(r2), E.fields_of(i1)
    bams, firsts, seconds = [b""] * n_shards, [b""] * n_shards, [b""] * n_shards
    for i, (name, seq, qual) in enumerate(reads):
        cr, cy, ur, uy, cb = (cols[k][i].tobytes() for k in ("cr", "cy", "ur", "uy", "cb"))
        tags = E.tags_of(cr, cy, ur, uy, indexes[i][1:] if with_i1 else None, cb if with_cb and index[i] >= 0 else None)
        s = int(shard[i])
        bams[s] += E.bam_record(name, seq, qual, tags)
        first, second = E.fastq_records(name, seq, qual, cr, cy, ur, uy)
        firsts[s] += first
        seconds[s] += second
    return bams, firsts, seconds


def device_outputs(n, shard, n_shards, fmt, with_i1, with_cb):
    r2, i1, cols, index = synthetic(n)
    window = fp.text_window(r2)
    off, length, first_flagged, _ = fp.window_lines(window)
    assert window.n_records == n and first_flagged == -1
    index_part = None
    if with_i1:
        w1 = fp.text_window(i1)
        off1, len1, flagged1, _ = fp.window_lines(w1)
        assert w1.n_records == n and flagged1 == -1
        index_part = (w1.text, w1.n_bytes, off1, len1)
    t = {k: dev_tensor(v) for k, v in cols.items()}
    batch = fp.Batch(window.text, window.n_bytes, off, length, t["cr"], t["cy"], t["ur"], t["uy"],
                     dev_tensor(np.asarray(shard, dtype=np.int32)), n_shards, fmt, i1=index_part,
                     cb=t["cb"] if with_cb else None, cb_index=dev_tensor(index) if with_cb else None)
    offsets, shard_counts, shard_bytes = fp.plan(batch)
    out, bounds = fp.emit(batch, offsets, shard_bytes)
    out = out.cpu().numpy().tobytes()
    pieces = [out[bounds[k]:bounds[k + 1]] for k in range(len(bounds) - 1)]
    return pieces, shard_counts.cpu().tolist(), offsets.cpu().numpy()


def shard_patterns(n, n_shards):
    r2, i1, cols, index = synthetic(n)
    hashed = [E.shard_of(row.tobytes(), n_shards) for row in cols["cr"]]
    yield "hash", hashed
    yield "one shard", [n_shards - 1] * n
    yield "own shard", [i % n_shards for i in range(n)]


@pytest.mark.parametrize("n_shards", [1, 2, 7, 1024])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, fp.PLAN_TILE - 1, fp.PLAN_TILE, fp.PLAN_TILE + 1, 3 * fp.PLAN_TILE])
def test_plan_and_emit_give_the_expected_bytes(n, n_shards):
    for what, shard in shard_patterns(n, n_shards):
        for with_i1, with_cb in ((True, True), (False, False)):
            bams, firsts, seconds = expected_shards(n, shard, n_shards, with_i1, with_cb)
            want_counts = [shard.count(s) for s in range(n_shards)]
            got, counts, _ = device_outputs(n, shard, n_shards, fp.BAM, with_i1, with_cb)
            assert counts == want_counts, what
            assert got == bams, what
            if what == "hash":  # the same bytes on a second run
                again, _, _ = device_outputs(n, shard, n_shards, fp.BAM, with_i1, with_cb)
                assert again == got
        got, counts, _ = device_outputs(n, shard, n_shards, fp.FASTQ, False, False)
        assert counts == want_counts, what
        assert got == firsts + seconds, what
        if what == "hash":
            again, _, _ = device_outputs(n, shard, n_shards, fp.FASTQ, False, False)
            assert again == got


def test_plan_carries_over_more_than_256_tiles():
    """More tiles than one round of the per-shard scan takes (256): 257 tiles and a few records."""
    n, n_shards = 257 * fp.PLAN_TILE + 5, 7
    rng = random.Random(77)
    records = [make_record(rng, name_length=rng.randint(1, 3), read_length=rng.randint(1, 4), description=False)
               for _ in range(n)]
    r2 = b"".join(records)
    cols = {k: random_barcodes(n, length, 300 + i) for i, (k, length) in enumerate((("cr", 5), ("cy", 5), ("ur", 3), ("uy", 3)))}
    shard = [E.shard_of(row.tobytes(), n_shards) for row in cols["cr"]]
    window = fp.text_window(r2)
    off, length, first_flagged, _ = fp.window_lines(window)
    assert window.n_records == n and first_flagged == -1
    t = {k: dev_tensor(v) for k, v in cols.items()}
    device_shard, _ = fp.shards(t["cr"], None, None, n_shards)
    assert device_shard.cpu().tolist() == shard
    batch = fp.Batch(window.text, window.n_bytes, off, length, t["cr"], t["cy"], t["ur"], t["uy"], device_shard, n_shards, fp.BAM)
    offsets, shard_counts, shard_bytes = fp.plan(batch)
    want = [b""] * n_shards
    want_offsets = []
    for i, (name, seq, qual) in enumerate(E.fields_of(r2)):
        want_offsets.append(len(want[shard[i]]))
        want[shard[i]] += E.bam_record(name, seq, qual, E.tags_of(*(cols[k][i].tobytes() for k in ("cr", "cy", "ur", "uy"))))
    assert offsets[0].cpu().tolist() == want_offsets
    assert shard_counts.cpu().tolist() == [shard.count(s) for s in range(n_shards)]
    assert shard_bytes[0].cpu().tolist() == [len(w) for w in want]
    out, bounds = fp.emit(batch, offsets, shard_bytes)
    out = out.cpu().numpy().tobytes()
    assert [out[bounds[k]:bounds[k + 1]] for k in range(n_shards)] == want


def test_the_hashed_pattern_is_what_the_device_shard_call_gives():
    r2, i1, cols, index = synthetic(3 * fp.PLAN_TILE)
    shard, _ = fp.shards(dev_tensor(cols["cr"]), None, None, 7)
    assert shard.cpu().tolist() == dict(shard_patterns(3 * fp.PLAN_TILE, 7))["hash"]


# ---- end to end ----

def run_cli(tmp_path, name, *args):
    out = tmp_path / name
    out.mkdir()
    assert cli_main(["FastqProcess", "--R1", R1, "--R2", R2, "--I1", I7, "--sample-id", "test",
                     "--output-dir", str(out)] + list(args)) == 0
    return out


def r1_fields():
    return [(seq[:16], qual[:16], seq[16:26], qual[16:26]) for _, seq, qual in E.fields_of(open(R1, "rb").read())]


@pytest.mark.parametrize("umi", [10, 8])
def test_one_shard_equals_the_references_tagged_bam(tmp_path, umi):
    out = run_cli(tmp_path, "one", "--barcode-length", "16", "--umi-length", str(umi), "--num-shards", "1")
    assert sorted(os.listdir(out)) == ["subfile_0.bam"]
    header, records = E.read_bam(str(out / "subfile_0.bam"))
    assert header == "@HD\tVN:1.6\tSO:unsorted\n@RG\tID:A\tSM:test\n"
    _, reference = E.read_bam(TAGGED)
    assert len(records) == len(reference) == 100
    for raw, ref, (cr, cy, ur, uy) in zip(records, reference, r1_fields()):
        got, want = E.parse_record(raw), E.parse_record(ref)
        assert [t for t, _ in got["tags"]] == [b"RG", b"CR", b"CY", b"UR", b"UY", b"SR", b"SY"]
        assert (got["name"], got["flag"], got["seq"], got["qual"]) == (want["name"], want["flag"], want["seq"], want["qual"])
        ours, theirs = dict(got["tags"]), dict(want["tags"])
        assert sorted(ours) == sorted(theirs)
        assert (ours[b"UR"], ours[b"UY"]) == (ur[:umi], uy[:umi])
        for tag in theirs:  # the reference's file was written with an 8-base UMI
            assert ours[tag][:8] == theirs[tag] if tag in (b"UR", b"UY") else ours[tag] == theirs[tag], tag
        if umi == 8:
            assert got["tags"] == want["tags"]
        assert got["core"] == (-1, -1, 0, fp.BAM_BIN, 0, len(got["seq"]), -1, -1, 0)
    # the file opens with the package's own reader as well
    assert [r.query_name for r in bam.open_alignments(str(out / "subfile_0.bam"), "rb")] == \
        [E.parse_record(r)["name"].decode() for r in reference]


def own_whitelist(tmp_path):
    """A whitelist made from the file's own barcodes, so that most reads are correctable."""
    barcodes = sorted({cr for cr, _, _, _ in r1_fields() if set(cr) <= set(BASES)})
    path = tmp_path / "own_whitelist.txt"
    path.write_bytes(b"".join(b + b"\n" for b in barcodes[::2]))
    return str(path)


@pytest.mark.parametrize("which", ["1k", "own"])
def test_cb_is_present_exactly_where_the_host_map_corrects(tmp_path, which):
    whitelist = WHITELIST if which == "1k" else own_whitelist(tmp_path)
    out = run_cli(tmp_path, "wl", "--barcode-length", "16", "--umi-length", "10", "--num-shards", "1",
                  "--white-list", whitelist)
    corrector = barcode.ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(whitelist)
    _, records = E.read_bam(str(out / "subfile_0.bam"))
    with_cb = 0
    for raw, (cr, cy, ur, uy) in zip(records, r1_fields()):
        tags = E.parse_record(raw)["tags"]
        try:
            want = corrector.get_corrected_barcode(cr.decode()).encode()
        except KeyError:
            want = None
        assert tags == E.tags_of(cr, cy, ur, uy, tuple(t for k, t in tags if k in (b"SR", b"SY")), want)
        with_cb += want is not None
    if which == "own":
        assert 30 <= with_cb < 100


def bucket_barcodes(whitelist):
    corrector = barcode.ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(whitelist)
    out = []
    for cr, _, _, _ in r1_fields():
        try:
            out.append(corrector.get_corrected_barcode(cr.decode()).encode())
        except KeyError:
            out.append(cr)
    return out


def test_seven_shards_hold_the_one_shard_output_partitioned_by_barcode(tmp_path):
    whitelist = own_whitelist(tmp_path)
    common = ["--barcode-length", "16", "--umi-length", "10", "--white-list", whitelist]
    one = run_cli(tmp_path, "one", "--num-shards", "1", *common)
    _, single = E.read_bam(str(one / "subfile_0.bam"))
    result = fp.FastqProcess([R1], [R2], [I7], whitelist=whitelist, barcode_length=16, umi_length=10, sample_id="test",
                             num_shards=7, output_dir=str(tmp_path)).run()
    assert result.paths == [str(tmp_path / ("subfile_%d.bam" % s)) for s in range(7)]
    assert result.n_reads == 100 == sum(result.shard_counts)
    assert result.n_correct + result.n_corrected + result.n_uncorrectable == 100
    buckets = bucket_barcodes(whitelist)
    position = {raw: i for i, raw in enumerate(single)}
    assert len(position) == 100
    seen, where = [], {}
    for s, path in enumerate(result.paths):
        header, records = E.read_bam(path)
        assert header == "@HD\tVN:1.6\tSO:unsorted\n@RG\tID:A\tSM:test\n"
        assert len(records) == result.shard_counts[s]
        order = [position[raw] for raw in records]
        assert order == sorted(order)  # input order inside the shard
        for i in order:
            assert where.setdefault(buckets[i], s) == s  # a bucket barcode lives in one shard
            assert E.shard_of(buckets[i], 7) == s
        seen += records
        assert len(list(bam.open_alignments(path, "rb"))) == len(records)
        assert gzip.open(path, "rb").read()[:4] == b"BAM\1"
    assert Counter(seen) == Counter(single)
    assert len({s for s in where.values()}) > 1


def test_fastq_mode_writes_the_expected_texts(tmp_path):
    out = run_cli(tmp_path, "fq", "--barcode-length", "16", "--umi-length", "10", "--num-shards", "3",
                  "--output-format", "FASTQ")
    assert sorted(os.listdir(out)) == sorted(["fastq_R%d_%d.fastq.gz" % (k, s) for k in (1, 2) for s in range(3)])
    firsts, seconds = [b""] * 3, [b""] * 3
    for (name, seq, qual), (cr, cy, ur, uy) in zip(E.fields_of(open(R2, "rb").read()), r1_fields()):
        s = E.shard_of(cr, 3)
        first, second = E.fastq_records(name, seq, qual, cr, cy, ur, uy)
        assert first.split(b"\n")[1] == cr + ur
        firsts[s] += first
        seconds[s] += second
    for s in range(3):
        assert gzip.open(out / ("fastq_R1_%d.fastq.gz" % s), "rb").read() == firsts[s]
        assert gzip.open(out / ("fastq_R2_%d.fastq.gz" % s), "rb").read() == seconds[s]
    assert all(firsts)


def write_triple(tmp_path, stem, n, seed, r1_length=42, i1=True):
    rng = random.Random(seed)
    names = [b"read%d_%d" % (seed, i) for i in range(n)]
    files = {}
    for kind, length in (("r1", r1_length), ("r2", None), ("i1", 8)):
        text = b""
        for name in names:
            size = rng.randint(20, 120) if length is None else length
            text += (b"@" + name + b" " + kind.encode() + b"\n" + bytes(rng.choice(BASES) for _ in range(size)) + b"\n+\n" +
                     bytes(rng.randint(35, 73) for _ in range(size)) + b"\n")
        files[kind] = tmp_path / ("%s_%s.fastq" % (stem, kind))
        files[kind].write_bytes(text)
    return files


def test_a_read_structure_with_two_cell_spans(tmp_path):
    files = write_triple(tmp_path, "rs", 300, 3)
    result = fp.FastqProcess([str(files["r1"])], [str(files["r2"])], None, read_structure="8C18X6C9M1X", sample_id="s",
                             num_shards=2, output_dir=str(tmp_path)).run()
    reads = E.fields_of(files["r1"].read_bytes())
    got = {}
    for path in result.paths:
        for raw in E.read_bam(path)[1]:
            rec = E.parse_record(raw)
            got[rec["name"]] = dict(rec["tags"])
            assert [t for t, _ in rec["tags"]] == [b"RG", b"CR", b"CY", b"UR", b"UY"]
    assert len(got) == 300
    for name, seq, qual in reads:
        tags = got[name]
        assert tags[b"CR"] == seq[:8] + seq[26:32] and len(tags[b"CR"]) == 14
        assert tags[b"CY"] == qual[:8] + qual[26:32]
        assert tags[b"UR"] == seq[32:41] and len(tags[b"UR"]) == 9 and tags[b"UY"] == qual[32:41]


def test_small_windows_and_two_triples_give_the_files_of_the_default_window(tmp_path):
    a, b = write_triple(tmp_path, "a", 700, 21, r1_length=26), write_triple(tmp_path, "b", 450, 22, r1_length=26)
    outs = []
    for name, window_bytes in (("default", 256 << 20), ("small", 20000)):
        out = tmp_path / name
        out.mkdir()
        job = fp.FastqProcess([str(a["r1"]), str(b["r1"])], [str(a["r2"]), str(b["r2"])], [str(a["i1"]), str(b["i1"])],
                              barcode_length=16, umi_length=10, sample_id="w", num_shards=3, output_dir=str(out))
        result = job.run(window_bytes=window_bytes)
        assert result.n_reads == 1150
        outs.append([open(p, "rb").read() for p in result.paths])
    # R1 (~80 bytes a record), I1 (~45) and R2 (~170) are cut at different records by a 20,000-byte window
    assert a["r2"].stat().st_size > 4 * 20000 and a["i1"].stat().st_size > 20000
    assert outs[0] == outs[1]
    records = [r for p in result.paths for r in E.read_bam(p)[1]]
    assert len(records) == 1150
    names = [E.parse_record(r)["name"] for r in E.read_bam(result.paths[0])[1]]
    firsts = [n for n in names if n.startswith(b"read21_")]
    assert names[:len(firsts)] == firsts  # the first triple's records come first in every shard


@pytest.mark.parametrize("with_whitelist", [False, True])
def test_small_windows_with_a_barcode_that_is_no_multiple_of_16_bytes(tmp_path, with_whitelist):
    """A 12-base cell barcode: from the second R2 window on, the rows an R2 window takes from an R1 window
    begin at a byte that is no multiple of 16, and the shard call wants its columns 16-byte aligned."""
    files = write_triple(tmp_path, "t", 900, 41, r1_length=26)
    reads = E.fields_of(files["r1"].read_bytes())
    whitelist = None
    if with_whitelist:
        whitelist = str(tmp_path / "wl12.txt")
        open(whitelist, "wb").write(b"".join(b + b"\n" for b in sorted({seq[:12] for _, seq, _ in reads})[::2]))
    outs = []
    for name, window_bytes in (("default", 256 << 20), ("small", 20000)):
        out = tmp_path / name
        out.mkdir()
        result = fp.FastqProcess([str(files["r1"])], [str(files["r2"])], [str(files["i1"])], whitelist=whitelist,
                                 barcode_length=12, umi_length=8, sample_id="w", num_shards=3,
                                 output_dir=str(out)).run(window_bytes=window_bytes)
        assert result.n_reads == 900 == sum(result.shard_counts)
        outs.append([open(p, "rb").read() for p in result.paths])
    assert files["r2"].stat().st_size > 3 * 20000
    assert outs[0] == outs[1]
    corrector = barcode.ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(whitelist) if whitelist else None
    by_name = {name: (seq, qual) for name, seq, qual in reads}
    seen = 0
    for s, path in enumerate(result.paths):
        for raw in E.read_bam(path)[1]:
            rec = E.parse_record(raw)
            seq, qual = by_name[rec["name"]]
            tags = dict(rec["tags"])
            assert (tags[b"CR"], tags[b"CY"], tags[b"UR"], tags[b"UY"]) == (seq[:12], qual[:12], seq[12:20], qual[12:20])
            bucket = seq[:12]
            if corrector is not None:
                try:
                    bucket = corrector.get_corrected_barcode(seq[:12].decode()).encode()
                    assert tags[b"CB"] == bucket
                except KeyError:
                    assert b"CB" not in tags
            assert E.shard_of(bucket, 3) == s
            seen += 1
    assert seen == 900


def no_outputs(path):
    return [n for n in os.listdir(path) if n.startswith("subfile_") or n.startswith("fastq_R")] == []


def test_errors_raise_value_error_and_leave_no_output(tmp_path):
    good = write_triple(tmp_path, "good", 400, 31, r1_length=26)
    out = tmp_path / "out"
    out.mkdir()

    def run(r1, r2, i1, **kw):
        return fp.FastqProcess([str(r1)], [str(r2)], [str(i1)], barcode_length=16, umi_length=10, num_shards=2,
                               output_dir=str(out)).run(**kw)

    r2_text = good["r2"].read_bytes()
    short = tmp_path / "short_r2.fastq"
    short.write_bytes(b"\n".join(r2_text.split(b"\n")[:4 * 399]) + b"\n")
    with pytest.raises(ValueError, match="same number"):
        run(good["r1"], short, good["i1"], window_bytes=20000)
    assert no_outputs(out)
    with pytest.raises(ValueError, match="same number"):  # and the other way round: R1 one record short
        r1_short = tmp_path / "short_r1.fastq"
        r1_short.write_bytes(b"\n".join(good["r1"].read_bytes().split(b"\n")[:4 * 399]) + b"\n")
        run(r1_short, good["r2"], good["i1"])
    assert no_outputs(out)

    lines = good["r1"].read_bytes().split(b"\n")
    lines[4 * 200 + 1] = lines[4 * 200 + 1][:20]
    lines[4 * 200 + 3] = lines[4 * 200 + 3][:20]
    bad_r1 = tmp_path / "bad_r1.fastq"
    bad_r1.write_bytes(b"\n".join(lines))
    with pytest.raises(ValueError, match="record 200"):
        run(bad_r1, good["r2"], good["i1"], window_bytes=20000)
    assert no_outputs(out)

    lines = r2_text.split(b"\n")
    lines[4 * 310 + 3] = lines[4 * 310 + 3][:-1]
    bad_r2 = tmp_path / "bad_r2.fastq"
    bad_r2.write_bytes(b"\n".join(lines))
    with pytest.raises(ValueError, match=r"bad_r2\.fastq: FASTQ record 310: sequence and quality differ"):
        run(good["r1"], bad_r2, good["i1"], window_bytes=20000)
    assert no_outputs(out)
    run(good["r1"], good["r2"], good["i1"])  # the good triple does write
    assert not no_outputs(out)
