"""sctools_amd.reader / sctools_amd.fastq / bam.Tagger on the host (no GPU).

``tests/golden/fastq/expected_tags.json.gz`` holds what the reference's own generators yield for the
fixture files (tools/make_fastq_golden.py); the host iterators must yield the same.  The native tag
writer (``sct_bam_attach_*``) is driven with numpy columns and read back with
``sctools_amd.bam.open_alignments``; ``tests/golden/bam/test_r2_tagged.bam`` is the reference's own
output for ``test_r2.bam`` with an 8-base molecule barcode.
"""
import argparse
import gzip
import hashlib
import json
import os
import re

import numpy as np
import pytest

from sctools_amd import bam, bamnative, consts, fastq, platform, reader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "fastq")
R1 = os.path.join(GOLD, "test_r1.fastq")
I7 = os.path.join(GOLD, "test_i7.fastq")
R2_BAM = os.path.join(GOLD, "test_r2.bam")
TAGGED = os.path.join(ROOT, "tests", "golden", "bam", "test_r2_tagged.bam")
WHITELIST = os.path.join(ROOT, "tests", "golden", "barcode", "1k-august-2016.txt")
EXPECTED = json.load(gzip.open(os.path.join(GOLD, "expected_tags.json.gz"), "rt"))

CELL, MOLECULE, SAMPLE = platform.TenXV2.cell_barcode, platform.TenXV2.molecule_barcode, platform.TenXV2.sample_barcode
MOLECULE7 = MOLECULE._replace(end=23)
MOLECULE8 = MOLECULE._replace(end=24)


def generators(case):
    if case == "10x":
        return [fastq.EmbeddedBarcodeGenerator(R1, [CELL, MOLECULE]), fastq.EmbeddedBarcodeGenerator(I7, [SAMPLE])]
    if case == "10x_whitelist":
        return [fastq.BarcodeGeneratorWithCorrectedCellBarcodes(R1, CELL, WHITELIST, [MOLECULE]),
                fastq.EmbeddedBarcodeGenerator(I7, [SAMPLE])]
    if case == "10x_gz":
        return [fastq.EmbeddedBarcodeGenerator(R1 + ".gz", [CELL, MOLECULE])]
    if case == "10x_bz2":
        return [fastq.EmbeddedBarcodeGenerator(R1 + ".bz2", [CELL, MOLECULE])]
    if case == "attach_barcodes":
        return [fastq.EmbeddedBarcodeGenerator(R1, [SAMPLE]),
                fastq.BarcodeGeneratorWithCorrectedCellBarcodes(R1, CELL, WHITELIST, [MOLECULE7])]
    raise KeyError(case)


def test_manifest():
    manifest = json.load(open(os.path.join(GOLD, "MANIFEST.json")))["sha256"]
    assert sorted(manifest) == sorted(n for n in os.listdir(GOLD) if n != "MANIFEST.json")
    for name, digest in manifest.items():
        assert hashlib.sha256(open(os.path.join(GOLD, name), "rb").read()).hexdigest() == digest, name


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_host_generators_yield_what_the_reference_yields(case):
    for generator, expected in zip(generators(case), EXPECTED[case]):
        got = [[[tag, value] for tag, value, kind in tags] for tags in generator]
        assert all(kind == "Z" for tags in generator for _, _, kind in tags)
        assert len(got) == 100
        assert got == expected


def test_fixture_has_a_record_with_and_without_cb():
    with_cb = [any(tag == "CB" for tag, _ in tags) for tags in EXPECTED["10x_whitelist"][0]]
    assert any(with_cb) and not all(with_cb)


def test_bytes_mode_yields_bytes():
    got = list(fastq.EmbeddedBarcodeGenerator(R1, [CELL], mode="rb"))
    assert [[t, v.decode()] for t, v, _ in got[3]] == EXPECTED["10x"][0][3][:2]


@pytest.mark.parametrize("suffix", ["", ".gz", ".bz2"])
def test_reader_detects_the_compression(suffix, tmp_path):
    plain = open(R1).read().splitlines(keepends=True)
    assert list(reader.Reader(R1 + suffix)) == plain
    assert list(reader.Reader(R1 + suffix, mode="rb")) == [ln.encode() for ln in plain]
    # by magic number, not by name
    disguised = str(tmp_path / "reads.txt")
    with open(R1 + suffix, "rb") as src, open(disguised, "wb") as dst:
        dst.write(src.read())
    assert list(reader.Reader(disguised)) == plain
    opener = reader.infer_open(R1 + suffix, "r")
    assert opener.func is {"": open, ".gz": gzip.open, ".bz2": __import__("bz2").open}[suffix]


def test_reader_arguments_and_several_files(tmp_path):
    assert len(reader.Reader([R1, R1])) == 800
    assert reader.Reader(R1).filenames == [R1]
    assert reader.Reader([R1, I7]).size == os.stat(R1).st_size + os.stat(I7).st_size
    with pytest.raises(ValueError):
        reader.Reader(R1, mode="w")
    with pytest.raises(TypeError):
        reader.Reader([R1, 3])
    with pytest.raises(TypeError):
        reader.Reader(3)
    commented = tmp_path / "c.txt"
    commented.write_text("#a\n#b\nx\n#kept\ny\n")
    assert list(reader.Reader(str(commented), header_comment_char="#")) == ["x\n", "#kept\n", "y\n"]
    assert list(reader.Reader(str(commented), mode="rb", header_comment_char="#")) == [b"x\n", b"#kept\n", b"y\n"]
    assert list(reader.zip_readers(reader.Reader(R1), reader.Reader(R1), indices={1, 5})) == \
        [(ln, ln) for i, ln in enumerate(open(R1)) if i in (1, 5)]


def test_len_and_select_record_indices():
    rd = fastq.Reader(R1)
    assert len(rd) == 100
    wanted = {0, 7, 99}
    picked = list(rd.select_record_indices(wanted))
    assert wanted == {0, 7, 99}  # the caller's set is left alone
    everything = list(rd)
    assert [str(r) for r in picked] == [str(everything[i]) for i in (0, 7, 99)]
    assert isinstance(everything[0], fastq.StrRecord) and isinstance(next(iter(fastq.Reader(R1, mode="rb"))), fastq.Record)


def test_trailing_lines_and_missing_final_newline(tmp_path):
    lines = open(R1).read().splitlines(keepends=True)
    p = tmp_path / "t.fastq"
    p.write_text("".join(lines[:10]))  # two records and two lines
    assert len(fastq.Reader(str(p))) == 2
    p.write_text("".join(lines[:8])[:-1])  # the last line unterminated
    got = list(fastq.EmbeddedBarcodeGenerator(str(p), [CELL, MOLECULE]))
    assert [[t, v] for t, v, _ in got[1]] == EXPECTED["10x"][0][1]


def test_records_raise_as_the_references_do():
    good = [b"@name\n", b"ACGT\n", b"+\n", b"FFFF\n"]
    rec = fastq.Record(good)
    assert bytes(rec) == b"".join(good) and str(rec) == b"".join(good).decode() and len(rec) == 5
    assert "Name: " in repr(rec)
    with pytest.raises(ValueError):
        fastq.Record([b"name\n"] + good[1:])
    for k in range(4):
        bad = list(good)
        bad[k] = 7
        with pytest.raises(TypeError):
            fastq.Record(bad)
    with pytest.raises(TypeError):
        fastq.Record(["@name\n"] + good[1:])  # str.startswith(bytes), as in the reference
    sgood = [g.decode() for g in good]
    srec = fastq.StrRecord(sgood)
    assert str(srec) == "".join(sgood) and bytes(srec) == b"".join(good)
    with pytest.raises(ValueError):
        fastq.StrRecord(["name\n"] + sgood[1:])
    for k in range(4):
        bad = list(sgood)
        bad[k] = 7
        with pytest.raises(TypeError):
            fastq.StrRecord(bad)
    with pytest.raises(ValueError):
        fastq.Record(good[:3])  # not four lines


def test_average_quality():
    # the quality line's last byte (the newline) is left out; Phred offset 33
    assert fastq.Record([b"@n\n", b"ACGT\n", b"+\n", b"I5+!\n"]).average_quality() == (40 + 20 + 10 + 0) / 4
    assert fastq.StrRecord(["@n\n", "ACGT\n", "+\n", "I5+!\n"]).average_quality() == (40 + 20 + 10 + 0) / 4


def test_extract_barcode():
    rec = fastq.StrRecord(["@n\n", "ACGTACGT\n", "+\n", "ABCDEFGH\n"])
    eb = fastq.EmbeddedBarcode(start=2, end=5, sequence_tag="XS", quality_tag="XQ")
    assert fastq.extract_barcode(rec, eb) == (("XS", "GTA", "Z"), ("XQ", "CDE", "Z"))


def test_generator_errors_name_the_record(tmp_path):
    lines = open(R1).read().splitlines(keepends=True)
    bad_name = list(lines)
    bad_name[4 * 17] = "ST-K00126\n"
    p = tmp_path / "n.fastq"
    p.write_text("".join(bad_name))
    with pytest.raises(ValueError, match=r"must start with @.*record 17"):
        list(fastq.EmbeddedBarcodeGenerator(str(p), [CELL, MOLECULE]))
    short = list(lines)
    short[4 * 23 + 1] = short[4 * 23 + 1][:20] + "\n"
    p.write_text("".join(short))
    with pytest.raises(ValueError, match=r"record 23\b.*sequence line has 20 bytes.*26"):
        list(fastq.BarcodeGeneratorWithCorrectedCellBarcodes(str(p), CELL, WHITELIST, [MOLECULE]))
    short = list(lines)
    short[4 * 5 + 3] = short[4 * 5 + 3][:9] + "\n"
    p.write_text("".join(short))
    with pytest.raises(ValueError, match=r"record 5\b.*quality line has 9 bytes.*26"):
        list(fastq.EmbeddedBarcodeGenerator(str(p), [CELL, MOLECULE]))
    with pytest.raises(TypeError):
        fastq.BarcodeGeneratorWithCorrectedCellBarcodes(R1, CELL, WHITELIST, iter([MOLECULE]))


def test_columns_are_offered_only_where_the_cell_span_has_the_whitelists_length():
    assert fastq.BarcodeGeneratorWithCorrectedCellBarcodes(R1, CELL, WHITELIST, [MOLECULE]).supports_columns
    assert not fastq.BarcodeGeneratorWithCorrectedCellBarcodes(R1, CELL._replace(end=15), WHITELIST).supports_columns
    assert fastq.EmbeddedBarcodeGenerator(R1, [CELL]).supports_columns


def test_generator_without_a_barcode_yields_empty_tag_sets_and_is_left_to_the_host(tmp_path):
    # AttachBarcodes without a cell or molecule barcode builds this generator (platform.py:992-999)
    gen = fastq.EmbeddedBarcodeGenerator(R1, [])
    assert list(gen) == [[]] * 100
    assert not gen.supports_columns
    with pytest.raises(ValueError, match="no embedded barcode"):
        next(gen.columns())
    assert not fastq.EmbeddedBarcodeGenerator(R1, iter([CELL])).supports_columns  # an iterator is not consumed to find out
    out = str(tmp_path / "o.bam")
    bam.Tagger(R2_BAM).tag(out, [gen])
    same_records(records(out), records(R2_BAM))
    sample = [tags for tags in fastq.EmbeddedBarcodeGenerator(R1, [SAMPLE])]
    bam.Tagger(R2_BAM).tag(out, [sample, gen])
    for i, (a, b) in enumerate(zip(records(R2_BAM), records(out))):
        assert [(t, v) for t, v, *_ in b.get_tags()] == \
            [(t, v) for t, v, *_ in a.get_tags()] + [(t, v) for t, v, _ in sample[i]]


def test_header_declares_exactly_the_exported_functions():
    text = open(os.path.join(ROOT, "include", "sct_fastq.h")).read()
    names = sorted(set(re.findall(r"^\s*(?:int|const char\*)\s+(sct_fq_\w+)\(", text, flags=re.M)))
    assert names == sorted(fastq.EXPORTED)
    lib = fastq.load()
    for name in names:
        assert hasattr(lib, name), name
    assert "Lone-CR" in text


def test_argument_checks_need_no_gpu():
    import ctypes

    lib = fastq.load()
    nbytes = ctypes.c_size_t(0)
    assert lib.sct_fq_workspace_size(256 << 20, ctypes.byref(nbytes)) == 0
    assert nbytes.value >= (256 << 20) // fastq.TILE_BYTES * 12
    assert lib.sct_fq_workspace_size(-1, ctypes.byref(nbytes)) < 0
    assert b"n_bytes" in lib.sct_fq_last_error()
    p = ctypes.c_void_p
    assert lib.sct_fq_count(p(8), 100, 1, p(64), 1 << 20, p(64), None) == -1  # misaligned text
    assert lib.sct_fq_count(p(16), 1 << 20, 1, p(64), 16, p(64), None) == -2  # short workspace
    assert b"needed" in lib.sct_fq_last_error()
    spans = (fastq.Span * 1)(fastq.Span(4, 4))
    cols = (ctypes.c_void_p * 1)(64)
    assert lib.sct_fq_extract(p(16), 100, 1, p(64), 1 << 20, spans, 1, cols, cols, p(64), p(64), None) == -1
    assert b"span" in lib.sct_fq_last_error()
    assert lib.sct_fq_extract(p(16), 100, 1, p(64), 1 << 20, spans, 5, cols, cols, p(64), p(64), None) == -1


# ---- the native writer alone ----

def records(path):
    return list(bam.open_alignments(path, "rb"))


def raw_records(path):
    """The records' bytes as they are in the file: the whole inflated stream cut at the block sizes."""
    import struct

    data = gzip.open(path, "rb").read()  # BGZF is a series of gzip members
    off = 8 + struct.unpack_from("<i", data, 4)[0]
    n_ref = struct.unpack_from("<i", data, off)[0]
    off += 4
    for _ in range(n_ref):
        off += 8 + struct.unpack_from("<i", data, off)[0]
    out = []
    while off < len(data):
        size = struct.unpack_from("<i", data, off)[0]
        out.append(data[off:off + 4 + size])
        off += 4 + size
    return out


def same_records(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        for field in ("query_name", "flag", "reference_id", "pos", "mapq", "cigar", "l_seq", "_qual"):
            assert getattr(a, field) == getattr(b, field), field
        assert list(a.get_tags()) == list(b.get_tags())  # tag for tag, in order


def column(values):
    width = max(len(v) for v in values)
    out = np.zeros((len(values), width), dtype=np.uint8)
    for i, v in enumerate(values):
        out[i, :len(v)] = np.frombuffer(v.encode(), dtype=np.uint8)
    return out


def ten_x_columns(molecule=MOLECULE8):
    """The six columns of the 10x order from the fixture files, sliced here."""
    r1 = open(R1).read().splitlines()
    i7 = open(I7).read().splitlines()
    out = []
    for tag, lines, which, eb in (("CR", r1, 1, CELL), ("CY", r1, 3, CELL), ("UR", r1, 1, molecule),
                                  ("UY", r1, 3, molecule), ("SR", i7, 1, SAMPLE), ("SY", i7, 3, SAMPLE)):
        out.append((tag, column([lines[4 * r + which][eb.start:eb.end] for r in range(100)]), None))
    return out


def test_tagged_fixture_is_r2_with_the_six_tags_of_the_fastq_files():
    # every tag of every record of the reference's output, confirmed against slices made here
    cols = ten_x_columns()
    plain, tagged = records(R2_BAM), records(TAGGED)
    assert len(plain) == len(tagged) == 100
    for i, (a, b) in enumerate(zip(plain, tagged)):
        want = list(a.get_tags()) + [(tag, bytes(values[i]).decode()) for tag, values, _ in cols]
        assert [(t, v) for t, v, *_ in b.get_tags()] == [(t, v) for t, v, *_ in want]


def test_native_writer_reproduces_the_references_tagged_bam(tmp_path):
    out = str(tmp_path / "o.bam")
    with bamnative.TagAttacher(R2_BAM, out) as w:
        assert w.n == 100
        assert w.write([], 0) == 0  # an empty window
        cols = ten_x_columns()
        assert w.write([(t, v[:37], ln) for t, v, ln in cols]) == 37  # two windows: the members do not depend on the cut
        assert w.write([(t, v[37:], ln) for t, v, ln in cols]) == 63
    same_records(records(out), records(TAGGED))
    assert raw_records(out) == raw_records(TAGGED)  # every byte of every record, the sequence included
    whole = str(tmp_path / "w.bam")
    with bamnative.TagAttacher(R2_BAM, whole) as w:
        w.write(ten_x_columns())
    assert open(whole, "rb").read() == open(out, "rb").read()
    assert bam.read_header(out) == bam.read_header(R2_BAM)


def test_existing_tag_moves_to_the_end_with_the_new_value(tmp_path):
    out = str(tmp_path / "o.bam")
    with bamnative.TagAttacher(TAGGED, out) as w:
        w.write([("CR", column(["ACGT"] * 100), None)])
    for a, b in zip(records(TAGGED), records(out)):
        before = [(t, v) for t, v, *_ in a.get_tags()]
        assert [(t, v) for t, v, *_ in b.get_tags()] == [tv for tv in before if tv[0] != "CR"] + [("CR", "ACGT")]
        assert (a.query_name, a.flag, a._qual) == (b.query_name, b.flag, b._qual)


def test_length_minus_one_leaves_the_tag_off_and_shorter_lengths_cut_the_value(tmp_path):
    out = str(tmp_path / "o.bam")
    lengths = np.full(100, 4, dtype=np.int32)
    lengths[::3] = -1
    lengths[1::3] = 2
    with bamnative.TagAttacher(R2_BAM, out) as w:
        w.write([("CB", column(["ACGT"] * 100), lengths), ("XY", column(["Q"] * 100), None)])
    plain = records(R2_BAM)
    for i, b in enumerate(records(out)):
        want = [(t, v) for t, v, *_ in plain[i].get_tags()]
        if lengths[i] >= 0:
            want.append(("CB", "ACGT"[:lengths[i]]))
        want.append(("XY", "Q"))
        assert [(t, v) for t, v, *_ in b.get_tags()] == want


def test_a_tag_listed_twice_keeps_the_later_value(tmp_path):
    out = str(tmp_path / "o.bam")
    with bamnative.TagAttacher(R2_BAM, out) as w:
        w.write([("CB", column(["AAAA"] * 100), None), ("UR", column(["GG"] * 100), None),
                 ("CB", column(["TTTT"] * 100), None)])
    for a, b in zip(records(R2_BAM), records(out)):
        assert [(t, v) for t, v, *_ in b.get_tags()] == \
            [(t, v) for t, v, *_ in a.get_tags()] + [("UR", "GG"), ("CB", "TTTT")]


def test_bam_longer_than_the_columns_is_truncated(tmp_path):
    out = str(tmp_path / "o.bam")
    with bamnative.TagAttacher(R2_BAM, out) as w:
        assert w.write([(t, v[:40], ln) for t, v, ln in ten_x_columns()]) == 40
    same_records(records(out), records(TAGGED)[:40])


def test_columns_longer_than_the_bam_stop_at_its_end(tmp_path):
    out = str(tmp_path / "o.bam")
    cols = [(t, np.concatenate([v, v]), ln) for t, v, ln in ten_x_columns()]
    with bamnative.TagAttacher(R2_BAM, out) as w:
        assert w.write(cols) == 100
        assert w.remaining == 0
        assert w.write(cols) == 0
    same_records(records(out), records(TAGGED))


def test_writer_rejects_bad_values_and_removes_the_output_on_an_exception(tmp_path):
    out = str(tmp_path / "o.bam")
    with pytest.raises(ValueError):
        with bamnative.TagAttacher(R2_BAM, out) as w:
            w.write([("CB", np.zeros((100, 4), dtype=np.uint8), None)])  # NUL bytes
    assert not os.path.exists(out)
    with pytest.raises(ValueError):
        with bamnative.TagAttacher(R2_BAM, out) as w:
            w.write([("CB", column(["ACGT"] * 100), np.full(100, 5, dtype=np.int32))])  # longer than the stride
    assert not os.path.exists(out)
    with pytest.raises(ValueError):
        with bamnative.TagAttacher(R2_BAM, out) as w:
            w.write([("CBX", column(["ACGT"] * 100), None)])
    with pytest.raises((OSError, ValueError)):
        bamnative.TagAttacher(R1, out)  # not a BAM
    assert not os.path.exists(out)  # nothing is created for an input that cannot be read
    with pytest.raises(OSError):
        bamnative.TagAttacher(R2_BAM, str(tmp_path / "no-such-directory" / "o.bam"))


# ---- Tagger on host iterables ----

def test_tagger_needs_a_file_name():
    with pytest.raises(TypeError, match='The argument "bam_file" must be of type str'):
        bam.Tagger(1)


def test_tagger_with_plain_iterables_reproduces_the_tagged_bam(tmp_path):
    out = str(tmp_path / "o.bam")
    r1 = [tags for tags in fastq.EmbeddedBarcodeGenerator(R1, [CELL, MOLECULE8])]
    i7 = (tags for tags in fastq.EmbeddedBarcodeGenerator(I7, [SAMPLE]))
    bam.Tagger(R2_BAM).tag(out, [r1, i7])
    same_records(records(out), records(TAGGED))


def test_tagger_keeps_each_records_own_tag_order_and_ends_with_the_shortest_input(tmp_path):
    out = str(tmp_path / "o.bam")
    expected = EXPECTED["10x_whitelist"][0]
    assert any(len(tags) == 5 for tags in expected) and len(expected[0]) == 4  # CB appears after records without it
    sets = [[(t, v, "Z") for t, v in tags] for tags in expected][:60]
    sets[10] = list(reversed(sets[10]))  # an order that contradicts the window's
    sets[11] = sets[11] + [("CR", "twice", "Z")]
    bam.Tagger(R2_BAM).tag(out, [sets])
    got, plain = records(out), records(R2_BAM)
    assert len(got) == 60
    for i, rec in enumerate(got):
        want = {}
        for t, v, _ in sets[i]:  # set_tag in order: a repeated tag moves to the end
            want.pop(t, None)
            want[t] = v
        assert [(t, v) for t, v, *_ in rec.get_tags()] == \
            [(t, v) for t, v, *_ in plain[i].get_tags()] + list(want.items())
    bam.Tagger(R2_BAM).tag(out, [])
    same_records(records(out), plain)


def test_tagger_reads_a_host_iterable_one_record_past_the_bams_end_and_no_further(tmp_path):
    # the reference's zip: a bad record the BAM's end keeps it from reaching is never read
    u2, out, r1 = str(tmp_path / "forty.bam"), str(tmp_path / "o.bam"), str(tmp_path / "bad.fastq")
    with bamnative.TagAttacher(R2_BAM, u2) as w:
        assert w.write([], 40) == 40
    lines = open(R1).read().splitlines(keepends=True)
    edited = list(lines)
    edited[4 * 41] = edited[4 * 41][1:]
    open(r1, "w").write("".join(edited))
    consumed = []
    counted = (consumed.append(1) or tags for tags in fastq.EmbeddedBarcodeGenerator(r1, [CELL, MOLECULE8]))
    bam.Tagger(u2).tag(out, [counted, iter(fastq.EmbeddedBarcodeGenerator(I7, [SAMPLE]))])
    assert len(consumed) == 41
    same_records(records(out), records(TAGGED)[:40])
    edited = list(lines)
    edited[4 * 40] = edited[4 * 40][1:]
    open(r1, "w").write("".join(edited))
    with pytest.raises(ValueError, match=r"record 40\b"):
        bam.Tagger(u2).tag(out, [iter(fastq.EmbeddedBarcodeGenerator(r1, [CELL]))])
    assert not os.path.exists(out)


# ---- the command line's validation ----

BASE = ["--r1", R1, "--u2", R2_BAM, "-o", "unused.bam"]


@pytest.mark.parametrize("extra, error", [
    (["--cell-barcode-start-position", "0"], argparse.ArgumentError),  # a position without a length
    (["--molecule-barcode-length", "10"], argparse.ArgumentError),  # a length without a position
    (["--cell-barcode-start-position", "0", "--cell-barcode-length", "16", "--molecule-barcode-start-position", "15",
      "--molecule-barcode-length", "10"], argparse.ArgumentTypeError),  # the molecule barcode overlaps the cell barcode
    (["--sample-barcode-start-position", "0", "--sample-barcode-length", "8"], argparse.ArgumentError),  # no --i1
    (["--cell-barcode-start-position", "-1", "--cell-barcode-length", "16"], SystemExit),  # argparse rejects the type
    (["--cell-barcode-start-position", "0", "--cell-barcode-length", "0"], SystemExit),
])
def test_barcode_platform_validation(extra, error, capsys):
    with pytest.raises(error):
        platform.BarcodePlatform.attach_barcodes(BASE + extra)
    assert not os.path.exists("unused.bam")


def test_validators_and_commands():
    bp = platform.BarcodePlatform
    assert bp._validate_barcode_start_pos("0") == 0 and bp._validate_barcode_length("1") == 1
    with pytest.raises(argparse.ArgumentTypeError):
        bp._validate_barcode_start_pos("-1")
    with pytest.raises(argparse.ArgumentTypeError):
        bp._validate_barcode_length("0")
    assert bp._validate_barcode_input(5, 5) == 5
    bp._validate_barcode_length_and_position(0, 16)
    bp._validate_barcode_length_and_position(None, None)
    assert platform.COMMANDS["Attach10xBarcodes"] == platform.TenXV2.attach_barcodes
    assert platform.COMMANDS["AttachBarcodes"] == platform.BarcodePlatform.attach_barcodes
    assert (CELL.start, CELL.end, CELL.sequence_tag, CELL.quality_tag) == (0, 16, "CR", "CY")
    assert (MOLECULE.start, MOLECULE.end, MOLECULE.sequence_tag, MOLECULE.quality_tag) == (16, 26, "UR", "UY")
    assert (SAMPLE.start, SAMPLE.end, SAMPLE.sequence_tag, SAMPLE.quality_tag) == (0, 8, "SR", "SY")
    assert consts.CELL_BARCODE_TAG_KEY == "CB"
