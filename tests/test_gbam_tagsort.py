"""The device decoder's TagSort mode (sct_gbam_parse_tagsort, csrc/gbam.hip k_parse_tagsort) against the host
decoder's (bamnative.decode(path, "tagsort"), itself pinned to the restatement of the reference's per-read
rule by test_tagsort_native_cpu.py): all fourteen columns and the three name lists equal, or, where the host
raises, ``gbam.decode`` returns None.  Then TagSort end to end: the device-decoded run writes the bytes the
host-decoded run writes."""
import os
import re
import struct

import numpy as np
import pytest

import bamwriter
import tagsort_ref as R
import test_gbam as TG
import test_tagsort_native_cpu as TC
from sctools_amd import _native as N
from sctools_amd import bamnative, columnar, gbam, tagsort

pytestmark = pytest.mark.gpu

CUG = ("CB", "UB", "GE")
GTF = os.path.join(R.FIXTURES, "genes.gtf")
NAMES = os.path.join(R.FIXTURES, "mito_names.txt")
UNSORTED = os.path.join(TG.GOLD, "unsorted.bam")
NUMBERS = ("cy_gt30", "cy_len", "uy_gt30", "uy_len", "gq_sum", "gq_len", "gq_gt30")


def host(path, tags):
    try:
        return bamnative.decode(path, "tagsort", tags=tags)
    except Exception as e:  # noqa: BLE001 -- the host decoder's error for this file
        return e


def same_as_host(path, tags=CUG, timings=None):
    """Device == host for this file; returns the host's (arrays, names), or its exception."""
    want = host(path, tags)
    got = gbam.decode(path, "tagsort", tags=tags, timings=timings)
    if isinstance(want, Exception):
        assert got is None, (path, tags, want)
        return want
    assert got is not None, (path, tags, gbam.last_error())
    cols, names = got
    arrays, want_names = want
    assert [list(x) for x in names] == [list(x) for x in want_names], (path, tags)
    assert set(N.RECORD_COLUMNS) <= set(arrays) and len(N.RECORD_COLUMNS) == 14
    for c in N.RECORD_COLUMNS:
        g = cols[c].cpu().numpy().view(arrays[c].dtype)
        assert g.shape == arrays[c].shape, (path, tags, c)
        bad = np.nonzero(g != arrays[c])[0][:5]
        assert bad.size == 0, (path, tags, c, bad, g[bad], arrays[c][bad])
    return want


def host_arrays(cols):
    """The device columns on the host, in the host decoder's dtypes (torch holds the uint16 ones as int16)."""
    return {c: cols[c].cpu().numpy().view(dt) for c, dt in columnar.COLUMNS}


def raw_record(rec, front=b"", back=b"") -> bytes:
    """bamwriter's record with raw tag bytes spliced before and after its tag area."""
    b = bamwriter.record_bytes(rec)[4:]
    tags = b"".join(bamwriter._tag(k, v) for k, v in rec._tags.items())
    assert b.endswith(tags)
    body = b[:len(b) - len(tags)] + front + tags + back
    return struct.pack("<i", len(body)) + body


def write_raw(path, blobs, n_ref=32):
    """bamwriter.write_bam's header, then the record bytes as given."""
    hdr = b"BAM\x01" + struct.pack("<i", 0) + struct.pack("<i", n_ref)
    for i in range(n_ref):
        nm = ("chr%d" % i).encode() + b"\x00"
        hdr += struct.pack("<i", len(nm)) + nm + struct.pack("<i", 1 << 30)
    TG.rebgzf(hdr + b"".join(blobs), path)


def fields(arrays, names, k):
    return {"barcode": names[0][arrays["cell"][k]], "umi": names[1][arrays["umi"][k]],
            "gene": names[2][arrays["gene"][k]], "bits": int(arrays["bits"][k]), "xf": int(arrays["xf"][k]),
            "numbers": [int(arrays[f][k]) for f in NUMBERS]}


# ---- 1: the crafted records of the host decoder's test ----
def test_crafted_records(tmp_path):
    path = str(tmp_path / "crafted.bam")
    bamwriter.write_bam(path, TC.DECODE_RECORDS)
    got = gbam.decode(path, "tagsort", tags=CUG)
    assert got is not None, gbam.last_error()
    same_as_host(path)
    cols, names = got
    arrays = host_arrays(cols)
    assert len(TC.DECODE_RECORDS) == 28 and len(arrays["cell"]) == 28
    for k, rec in enumerate(TC.DECODE_RECORDS):
        want, who = R.read_fields(rec), rec.query_name
        f = fields(arrays, names, k)
        assert (f["barcode"], f["umi"], f["gene"]) == (want["barcode"], want["umi"], want["gene"]), who
        bits = f["bits"]
        seen = {"mapped": int(not bits & 0x01), "strand": (bits >> 1) & 1, "dup": (bits >> 2) & 1,
                "spliced": (bits >> 3) & 1, "nh1": (bits >> 4) & 1, "perfect_umi": (bits >> 5) & 1,
                "perfect_cb": (bits >> 7) & 1, "ref": int(arrays["ref"][k]), "pos": int(arrays["pos"][k])}
        seen.update(zip(NUMBERS, f["numbers"]))
        assert seen == {key: want[key] for key in seen}, who
        assert f["xf"] == R.XF_CODE.get(want["xf"], 5), who


# ---- 2: tag areas bamwriter cannot express ----
FULL_FIELDS = {"barcode": "ACGT", "umi": "TTT", "gene": "G1", "bits": 0xd0, "xf": 1,
               "numbers": [4, 4, 2, 3, 2550, 10, 10]}
F32_ONE = struct.pack("<f", 1.0)
RAW_CASES = [  # (name, record, front, back, what differs from FULL_FIELDS)
    ("second_cb", TC._rec("a", TC.FULL), b"", b"CBZZZZZ\x00", {}),
    ("cb_in_front", TC._rec("b", TC.FULL), b"CBZQQQQ\x00", b"", {"barcode": "QQQQ", "bits": 0x50}),
    ("second_nh", TC._rec("c", TC.FULL), b"", b"NHi" + struct.pack("<i", 5), {}),
    ("nh_in_front", TC._rec("d", TC.FULL), b"NHC\x02", b"", {"bits": 0xc0}),
    ("cr_char", TC._rec("e", TC._without("CR")), b"", b"CRAA", {"bits": 0x50}),
    ("xf_char", TC._rec("f", TC._without("XF")), b"", b"XFAC", {"xf": 0}),
    ("cb_hex", TC._rec("g", TC._without("CB")), b"", b"CBHACGT\x00", {}),
    ("nh_int8", TC._rec("h", TC._without("NH")), b"", b"NHc\x01", {}),
    ("nh_float", TC._rec("i", TC._without("NH")), b"", b"NHf" + F32_ONE, {"bits": 0xc0}),
    ("filler_257", TC._rec("j", TC.FULL, l_seq=257, cigar=((0, 257),)), b"", b"",
     {"numbers": [4, 4, 2, 3, 65535, 257, 257]}),
    ("cy_255", TC._rec("k", TC._without(CY="I" * 255)), b"", b"", {"numbers": [255, 255, 2, 3, 2550, 10, 10]}),
    ("uy_low_bytes", TC._rec("l", TC._without(UY=" \x1fI")), b"", b"", {"numbers": [4, 4, 1, 3, 2550, 10, 10]}),
    ("ub_dash", TC._rec("m", TC._without(UB="-")), b"", b"", {"umi": None}),
    ("ub_missing_ur_none", TC._rec("n", TC._without("UB", UR="None")), b"", b"", {"umi": None, "bits": 0xf0}),
]


def test_raw_tag_records(tmp_path):
    path = str(tmp_path / "raw.bam")
    write_raw(path, [raw_record(rec, front, back) for _, rec, front, back, _ in RAW_CASES])
    want = same_as_host(path)
    assert not isinstance(want, Exception), want
    got = gbam.decode(path, "tagsort", tags=CUG)
    cols, names = got
    arrays = host_arrays(cols)
    for k, (name, _, _, _, differs) in enumerate(RAW_CASES):
        expect = dict(FULL_FIELDS)
        expect.update(differs)
        assert fields(arrays, names, k) == expect, name
        assert fields(want[0], want[1], k) == expect, name  # the table is the host decoder's


# ---- 3: files the device declines ----
def nonascii_file(tmp_path) -> str:
    path = str(tmp_path / "latin1.bam")
    recs = [TC._rec("r%d" % k, TC.FULL) for k in range(64)] + [TC._rec("odd", TC._without(CB="AC\xe9T"))]
    write_raw(path, [raw_record(r) for r in recs])
    return path


DECLINES = {
    "cb_char": (raw_record(TC._rec("x", TC._without("CB")), back=b"CBAA"), bamnative.TypedTagValue, None),
    "cb_int": (raw_record(TC._rec("x", TC._without(CB=7))), bamnative.TypedTagValue, None),
    "filler_258": (raw_record(TC._rec("x", TC.FULL, l_seq=258, cigar=((0, 258),))), ValueError, "columnar limits"),
    "cy_256": (raw_record(TC._rec("x", TC._without(CY="I" * 256))), ValueError, "columnar limits"),
}


@pytest.mark.parametrize("case", sorted(DECLINES))
def test_declined_files(case, tmp_path):
    blob, error, match = DECLINES[case]
    path = str(tmp_path / (case + ".bam"))
    write_raw(path, [raw_record(TC._rec("r%d" % k, TC.FULL)) for k in range(64)] + [blob])  # a second wavefront
    assert gbam.decode(path, "tagsort", tags=CUG) is None
    with pytest.raises(error, match=match):
        bamnative.decode(path, "tagsort", tags=CUG)


def test_declined_non_ascii_barcode(tmp_path):
    path = nonascii_file(tmp_path)
    assert gbam.decode(path, "tagsort", tags=CUG) is None
    arrays, names = bamnative.decode(path, "tagsort", tags=CUG)  # decodes, no error
    assert len(arrays["cell"]) == 65 and len(names[0]) == 2


# ---- 4: quality lengths and alignments ----
L_SEQ = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 300)


def quality_records(last_l_seq):
    """Every l_seq with query names of 1..8 characters (the quality bytes start at every address modulo 8);
    the record of ``last_l_seq`` with the 8-character name goes last."""
    rng = np.random.default_rng(1234)
    recs = []
    for ln in L_SEQ:
        for name_len in range(1, 9):
            q = rng.integers(0, 94, ln, dtype=np.uint8)
            if ln >= 1:
                q[0] = 31
            if ln >= 2:
                q[-1] = 30
            recs.append(TC._rec("q" * name_len, TC.FULL, l_seq=ln, cigar=((0, ln),) if ln else (), qual=q.tobytes()))
    k = next(i for i, r in enumerate(recs) if r.l_seq == last_l_seq and len(r.query_name) == 8)
    recs.append(recs.pop(k))
    return recs


@pytest.mark.parametrize("last_l_seq", [300, 1])
def test_quality_lengths_and_alignments(last_l_seq, tmp_path):
    recs = quality_records(last_l_seq)
    assert len(recs) == 112 and recs[-1].l_seq == last_l_seq
    path = str(tmp_path / "qual.bam")
    write_raw(path, [raw_record(r) for r in recs])
    arrays, _ = same_as_host(path)
    assert arrays["gq_len"].tolist() == [r.l_seq for r in recs]
    assert arrays["gq_sum"].tolist() == [sum(r._qual) for r in recs]
    assert arrays["gq_gt30"].tolist() == [sum(b > 30 for b in r._qual) for r in recs]


@pytest.mark.parametrize("name_len", range(1, 9))
def test_qualities_that_end_the_payload(name_len, tmp_path):
    """The file's last record carries no tag, so its quality bytes are the payload's last bytes: the aligned
    word that holds the last of them reaches past the payload for most alignments and is read byte by byte."""
    rng = np.random.default_rng(name_len)
    recs = [TC._rec("r%d" % k, TC.FULL) for k in range(64)]
    for ln in (300, 13):  # (the first of the two is followed by a record, the second by nothing)
        q = rng.integers(0, 94, ln, dtype=np.uint8)
        q[0], q[-1] = 31, 30
        name = "long" if ln == 300 else "e" * name_len  # (so the payload's length takes every value modulo 8)
        recs.append(TC._rec(name, {}, l_seq=ln, cigar=((0, ln),), qual=q.tobytes()))
    path = str(tmp_path / "end.bam")
    write_raw(path, [raw_record(r) for r in recs])
    assert len(TG.payload(path)) % 8 == (name_len + 4) % 8
    arrays, names = same_as_host(path)
    assert arrays["gq_sum"][-2:].tolist() == [sum(r._qual) for r in recs[-2:]]
    assert arrays["gq_gt30"][-2:].tolist() == [sum(b > 30 for b in r._qual) for r in recs[-2:]]
    assert names[0][arrays["cell"][-1]] is None and int(arrays["bits"][-1]) == 0


# ---- 5: the bundled BAMs, several tag choices ----
@pytest.mark.parametrize("tags", [CUG, ("CR", "UR", "GE"), ("GE", "CB", "UB"), ("CB", "UB", "XX")], ids="-".join)
@pytest.mark.parametrize("bam", TG.BAMS)
def test_bundled_bams(bam, tags):
    same_as_host(os.path.join(TG.GOLD, bam + ".bam"), tags)


# ---- 6: members that cut records anywhere, and windows ----
@pytest.mark.parametrize("setting", [dict(level=6, block=997), dict(level=0)], ids=["block997", "stored"])
def test_members_and_windows(setting, tmp_path, monkeypatch):
    raw = TG.payload(os.path.join(TG.GOLD, "cell-sorted-missing-cb.bam"))
    path = str(tmp_path / "re.bam")
    TG.rebgzf(raw, path, **setting)
    same_as_host(path)
    monkeypatch.setenv("SCT_GBAM_WINDOW_BYTES", "40000")
    tm = {}
    same_as_host(path, timings=tm)
    assert tm["windows"] >= 3, tm


# ---- 7: ~59k records over ~300 members ----
def test_replicated_records(tmp_path):
    raw = TG.payload(os.path.join(TG.GOLD, "small-cell-sorted.bam"))
    hdr_end = TG._header_end(raw)
    body = raw[hdr_end:]
    reps = [re.sub(rb"CBZ.", b"CBZ" + bytes([65 + r % 26]), body) for r in range(90)]
    path = str(tmp_path / "big.bam")
    TG.rebgzf(raw[:hdr_end] + b"".join(reps), path, level=6, block=65280)
    arrays, _ = same_as_host(path)
    assert len(arrays["cell"]) > 50000


# ---- 8: TagSort end to end ----
def _run(bam, metric_type, roles, out, **kw):
    ts = tagsort.TagSort(bam, metric_type, "CB", "UB", "GE", tag_order=roles, gtf_file=GTF,
                         mitochondrial_gene_names_filename=NAMES, **kw)
    tm = {}
    ts.run(str(out), timings=tm)
    with open(str(out), newline="") as f:
        return ts, f.read(), tm


@pytest.mark.parametrize("roles", [("barcode", "umi", "gene"), ("gene", "barcode", "umi"), ("umi", "gene", "barcode")],
                         ids="-".join)
@pytest.mark.parametrize("metric_type", ["cell", "gene"])
def test_end_to_end_device_equals_host(metric_type, roles, tmp_path):
    dev, dev_text, tm = _run(UNSORTED, metric_type, roles, tmp_path / "dev.csv")
    assert dev.decoded_by == "device"
    assert set(gbam.STAGES) <= set(tm)
    hst, host_text, _ = _run(UNSORTED, metric_type, roles, tmp_path / "host.csv", decoder="host")
    assert hst.decoded_by == "host"
    assert dev_text == host_text and dev_text.count("\n") > 2


def test_end_to_end_falls_back_to_the_host(tmp_path):
    path = nonascii_file(tmp_path)
    auto, auto_text, tm = _run(path, "gene", tagsort.ROLES, tmp_path / "auto.csv")
    assert auto.decoded_by == "host" and tm == {}
    assert auto_text == _run(path, "gene", tagsort.ROLES, tmp_path / "host.csv", decoder="host")[1]


def test_cli_decoder_option(tmp_path):
    from sctools_amd.__main__ import main

    argv = ["TagSort", "--bam-input", UNSORTED, "--metric-type", "cell", "--compute-metric", "--gtf-file", GTF,
            "--mitochondrial-gene-names-filename", NAMES, "--barcode-tag", "CB", "--umi-tag", "UB", "--gene-tag", "GE"]
    a, b = tmp_path / "default.csv", tmp_path / "host.csv"
    assert main(argv + ["--metric-output", str(a)]) == 0
    assert main(argv + ["--metric-output", str(b), "--decoder", "host"]) == 0
    assert a.read_bytes() == b.read_bytes() and a.read_bytes().startswith(b",n_reads,")
