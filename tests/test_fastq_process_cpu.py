"""FastqProcess without a GPU: the restated ``std::hash<std::string>``, the read structure, the
shard-count formula, the argument errors, and the native shard writer (host code)."""
import gzip
import os
import random

import numpy as np
import pytest

import fqp_expect as E
from sctools_amd import bam, bamnative, fastq_process as fp

PINNED = [(b"", 6142509188972423790), (b"A", 6919333181322027406), (b"NTAAGAGTCTGCAAGT", 3691365170403569384),
          (b"ACGTACGT", 8082405133221442893), (b"ACGTACGTACG", 12775255082311150925),
          (b"AAACCCGGGTTTAAACCCGGGTTTAAACCCG", 8697300111780995106)]


def test_the_python_hash_gives_the_six_pinned_values():
    for data, want in PINNED:
        assert fp.std_hash(data) == want, data


def test_the_python_hash_is_std_hash_itself():
    rng = random.Random(3)
    strings = [bytes(rng.randrange(256) for _ in range(i % 32)) for i in range(3200)]
    strings += [bytes(rng.choice(b"ACGTN") for _ in range(i % 32)) for i in range(3200)]
    native = E.native_hashes(strings)
    assert [fp.std_hash(x) for x in strings] == native.tolist()
    assert E.native_hashes([d for d, _ in PINNED]).tolist() == [w for _, w in PINNED]


def test_read_structure_to_spans_and_joined_lengths():
    assert fp.structure_spans(16, 10, None) == ([(0, 16)], [(16, 26)])
    assert fp.structure_spans(None, None, "16C10M") == ([(0, 16)], [(16, 26)])
    cell, umi = fp.structure_spans(None, None, "8C18X6C9M1X")
    assert (cell, umi) == ([(0, 8), (26, 32)], [(32, 41)])
    job = fp.FastqProcess(["a"], ["b"], read_structure="8C18X6C9M1X", num_shards=1)
    assert (job.cell_length, job.umi_length) == (14, 9)
    assert fp.structure_spans(None, None, "3M4C2M")[1] == [(0, 3), (7, 9)]
    assert fp.structure_spans(12, 0, None) == ([(0, 12)], [])


def test_the_shard_count_formula(tmp_path):
    gib = 1 << 30
    assert fp.default_num_shards(0, 1.0) == 1
    assert fp.default_num_shards(1, 1.0) == 1
    assert fp.default_num_shards(gib, 1.0) == 1
    assert fp.default_num_shards(gib + 1, 1.0) == 2
    assert fp.default_num_shards(3 * gib, 0.5) == 6
    assert fp.default_num_shards(10 * gib, 3.0) == 4
    with pytest.raises(ValueError):
        fp.default_num_shards(gib, 0)
    files = []
    for name, size in (("r1", 1000), ("r2", 3000), ("i1", 500)):
        files.append(tmp_path / name)
        files[-1].write_bytes(b"x" * size)
    r1, r2, i1 = (str(f) for f in files)
    per_byte = 1.0 / gib  # one shard per byte of input
    assert fp.FastqProcess([r1], [r2], barcode_length=16, umi_length=10, bam_size=100 * per_byte).num_shards == 40
    assert fp.FastqProcess([r1], [r2], [i1], barcode_length=16, umi_length=10, bam_size=100 * per_byte).num_shards == 45
    assert fp.FastqProcess([r1], [r2], [i1], barcode_length=16, umi_length=10).num_shards == 1
    assert fp.FastqProcess([r1], [r2], barcode_length=16, umi_length=10, num_shards=9).num_shards == 9
    with pytest.raises(ValueError, match="outside 1..1024"):
        fp.FastqProcess([r1], [r2], barcode_length=16, umi_length=10, bam_size=per_byte)


def test_the_output_names():
    job = fp.FastqProcess("a", "b", barcode_length=16, umi_length=10, num_shards=2, output_dir="out")
    assert job.paths() == [os.path.join("out", "subfile_0.bam"), os.path.join("out", "subfile_1.bam")]
    job = fp.FastqProcess("a", "b", barcode_length=16, umi_length=10, num_shards=2, output_format="FASTQ")
    assert [os.path.basename(p) for p in job.paths()] == ["fastq_R1_0.fastq.gz", "fastq_R1_1.fastq.gz",
                                                          "fastq_R2_0.fastq.gz", "fastq_R2_1.fastq.gz"]
    assert fp.sam_header("s1") == "@HD\tVN:1.6\tSO:unsorted\n@RG\tID:A\tSM:s1\n"


@pytest.mark.parametrize("kwargs", [
    dict(),                                                          # neither lengths nor a read structure
    dict(barcode_length=16, umi_length=10, read_structure="16C10M"),  # both
    dict(barcode_length=16),                                         # one length alone
    dict(barcode_length=32, umi_length=10),                          # a cell barcode of more than 31 bases
    dict(read_structure="20C12X12C8M"),
    dict(read_structure="10M"),                                      # no cell barcode
    dict(read_structure="C10M"),                                     # a type without a length
    dict(barcode_length=16, umi_length=10, output_format="SAM"),
    dict(barcode_length=16, umi_length=10, num_shards=0),
    dict(barcode_length=16, umi_length=10, num_shards=1025),
    dict(barcode_length=16, umi_length=10, r2_files=["b", "c"]),
    dict(barcode_length=16, umi_length=10, i1_files=["b", "c"]),
    dict(barcode_length=-1, umi_length=10),
])
def test_argument_errors(kwargs):
    kwargs = dict(dict(r1_files=["a"], r2_files=["b"], num_shards=1), **kwargs)
    with pytest.raises(ValueError):
        fp.FastqProcess(**kwargs)


def test_the_expectation_builds_the_references_records():
    """tests/fqp_expect.py against the reference's own file: every byte but the bin, which the file's writer left 0."""
    _, records = E.read_bam(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bam", "test_r2_tagged.bam"))
    for raw in records:
        rec = E.parse_record(raw)
        built = E.bam_record(rec["name"], rec["seq"], rec["qual"], rec["tags"])
        assert built[:14] == raw[:14] and built[16:] == raw[16:]
        assert built[14:16] == (4680).to_bytes(2, "little") and raw[14:16] == b"\0\0"


# ---- the shard writer ----

def test_shard_writer_writes_bams_and_plain_gzip(tmp_path):
    paths = [str(tmp_path / ("s%d.bam" % i)) for i in range(3)] + [str(tmp_path / "t.fastq.gz")]
    headers = [fp.sam_header("x")] * 3 + [None]
    records = [[E.bam_record(b"r%d_%d" % (s, i), b"ACGT" * 30, b"I" * 120, E.tags_of(b"AC", b"II", b"G", b"I"))
                for i in range(700 * s)] for s in range(3)]
    text = b"".join(b"@r%d\nACGT\n+\nIIII\n" % i for i in range(9000))  # more than one 0xff00-byte member
    with bamnative.ShardWriter(paths, headers, level=1, threads=2) as writer:
        for step in range(4):  # four appends of a quarter each, cut anywhere
            parts = [b"".join(r)[len(b"".join(r)) * step // 4:len(b"".join(r)) * (step + 1) // 4] for r in records]
            parts.append(text[len(text) * step // 4:len(text) * (step + 1) // 4])
            bounds = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
            writer.append(np.frombuffer(b"".join(parts), dtype=np.uint8), bounds)
        writer.append(np.zeros(0, dtype=np.uint8), np.zeros(5, dtype=np.int64))
    for s in range(3):
        header, got = E.read_bam(paths[s])
        assert header == fp.sam_header("x") and got == records[s]
        assert len(list(bam.open_alignments(paths[s], "rb"))) == len(records[s])
        assert bam.read_header(paths[s])[1] == []
    assert gzip.open(paths[3], "rb").read() == text
    assert open(paths[3], "rb").read()[-28:] == open(paths[0], "rb").read()[-28:]  # the BGZF EOF member


def test_shard_writer_removes_every_file_on_failure(tmp_path):
    paths = [str(tmp_path / "a.bam"), str(tmp_path / "b.bam")]
    with pytest.raises(RuntimeError, match="boom"):
        with bamnative.ShardWriter(paths, [fp.sam_header("x")] * 2) as writer:
            writer.append(np.frombuffer(b"abcdef", dtype=np.uint8), [0, 3, 6])
            raise RuntimeError("boom")
    assert os.listdir(tmp_path) == []
    with pytest.raises(OSError):  # the second file cannot be created: the first is removed again
        bamnative.ShardWriter([paths[0], str(tmp_path / "missing" / "b.bam")], None)
    assert os.listdir(tmp_path) == []
    with pytest.raises(ValueError):
        with bamnative.ShardWriter(paths) as writer:
            writer.append(np.zeros(4, dtype=np.uint8), [0, 3, 2])  # bounds that run backwards
    assert os.listdir(tmp_path) == []
    with pytest.raises(ValueError):
        bamnative.ShardWriter(paths, [None])
    writer = bamnative.ShardWriter(paths)
    writer.close()
    writer.close()
    assert sorted(os.listdir(tmp_path)) == ["a.bam", "b.bam"]
    assert gzip.open(paths[0], "rb").read() == b""
