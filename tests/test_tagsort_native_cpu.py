"""TagSort (the reference's native tag sort with metrics) -- everything that needs no GPU: the six-digit
text round trip against glibc, the gatherer restatement against the CSVs recorded from the reference's
gatherer, the mitochondrial selector, the option checks, the re-ranking and the host decoder's mode."""
import os
import types

import numpy as np
import pytest

import bamwriter
import tagsort_ref as R
from sctools_amd import bamnative, tagsort


# ---- the round trip: ts_roundtrip(a, b) == strtof(snprintf("%g", (float)a / (float)b)) bit for bit ----
def _assert_roundtrip(a, b):
    got, want = R.roundtrip(a, b)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "first mismatch %d/%d: got %08x want %08x (%d in all)" % (
        a[bad[0]], b[bad[0]], got[bad[0]], want[bad[0]], bad.size)


def test_roundtrip_every_8bit_fraction():
    ln = np.repeat(np.arange(256, dtype=np.uint32), np.arange(1, 257))
    num = np.concatenate([np.arange(k + 1, dtype=np.uint32) for k in range(256)])
    assert ln.size == num.size == 257 * 128
    _assert_roundtrip(num, ln)


def test_roundtrip_every_quality_mean_up_to_160_bases():
    ln = np.concatenate([np.full(255 * k + 1, k, dtype=np.uint32) for k in range(1, 161)])
    num = np.concatenate([np.arange(255 * k + 1, dtype=np.uint32) for k in range(1, 161)])
    _assert_roundtrip(num, ln)


def test_roundtrip_random_16bit_pairs_and_zero_length():
    rng = np.random.default_rng(20)
    _assert_roundtrip(rng.integers(0, 1 << 16, 1_000_000, dtype=np.uint32),
                      rng.integers(1, 1 << 16, 1_000_000, dtype=np.uint32))
    got, want = R.roundtrip(np.array([0], dtype=np.uint32), np.array([0], dtype=np.uint32))
    assert np.isnan(got.view(np.float32)[0]) and np.isnan(want.view(np.float32)[0])
    assert got[0] >> 31 == 1  # the sign the reference's x86 build gives 0 / 0: it prints "-nan"
    _assert_roundtrip(np.array([7, 65535], dtype=np.uint32), np.array([0, 0], dtype=np.uint32))  # x / 0 = inf


# ---- the restatement of the gatherer against the reference's own output ----
MITO = None


def fixture_mito():
    global MITO
    if MITO is None:
        MITO = tagsort.mitochondrial_gene_ids(os.path.join(R.FIXTURES, "genes.gtf"),
                                              os.path.join(R.FIXTURES, "mito_names.txt"))
    return MITO


def test_fixture_cases_are_all_there():
    assert set(R.case_names()) == {
        "leading_unmapped", "unmapped_starts", "no_mapped_between", "last_unmapped", "none_tags", "multi_gene",
        "all_dropped", "fragments", "long_run", "mitochondrial", "constant_streams", "zero_lengths", "single_reads"}
    for name in R.case_names():
        assert R.recorded(name, "cell") is not None and R.recorded(name, "gene") is not None


@pytest.mark.parametrize("metric_type", ["cell", "gene"])
@pytest.mark.parametrize("name", R.case_names())
def test_restatement_reproduces_the_recorded_csv(name, metric_type):
    c = R.load_case(name)
    assert R.gather(c, metric_type, fixture_mito()) == R.recorded(name, metric_type)
    # the committed lines are the lines of the committed columns
    with open(os.path.join(R.FIXTURES, name + ".lines.txt")) as f:
        assert f.read() == "".join(ln + "\n" for ln in R.lines_of(c))


def test_recorded_csvs_show_the_native_rules():
    rows = R.recorded("constant_streams", "cell").split("\n")
    assert rows[1].split(",")[13] == "1.110223025e-16"  # four equal 0.7f: the order of the additions shows
    assert R.recorded("all_dropped", "gene").split("\n")[1].startswith(",0,0,")  # the lone final row, no name
    assert "-nan" in R.recorded("zero_lengths", "cell") and ",nan," in R.recorded("single_reads", "cell")
    assert R.recorded("mitochondrial", "cell").split("\n")[2].endswith(",100")


# ---- the mitochondrial selector ----
def test_mitochondrial_ids_with_and_without_a_names_file():
    gtf = os.path.join(R.FIXTURES, "genes.gtf")
    assert tagsort.mitochondrial_gene_ids(gtf, os.path.join(R.FIXTURES, "mito_names.txt")) == {"ENSG_MT1", "GX"}
    assert tagsort.mitochondrial_gene_ids(gtf) == {"ENSG_MT1", "G2"}  # ^mt- in any letter case


@pytest.mark.parametrize("line,message", [
    ("chr1\tfix\tgene\t1\t2\t.\t+\t.", "Expected at least 9 tabbed fields, got 8"),
    ('chr1\tfix\tgene\t1\t2\t.\t+\t.\tgene_id "a"; gene_name "b c";', "Expected 2 fields, found 3 fields"),
    ('chr1\tfix\tgene\t1\t2\t.\t+\t.\tgene_id "a"; ', "Expected 2 fields, found 0 fields"),
    ('chr1\tfix\tgene\t1\t2\t.\t+\t.\tgene_id "a";', "does not have a gene_name"),
])
def test_mitochondrial_selector_errors(tmp_path, line, message):
    p = tmp_path / "bad.gtf"
    p.write_text("# c\n" + line + "\n")
    with pytest.raises(tagsort.TagSortError, match=message):
        tagsort.mitochondrial_gene_ids(str(p))


def test_mitochondrial_selector_missing_files(tmp_path):
    with pytest.raises(tagsort.TagSortError, match="failed to open the GTF file"):
        tagsort.mitochondrial_gene_ids(str(tmp_path / "none.gtf"))
    with pytest.raises(tagsort.TagSortError, match="failed to open the mitochondrial gene names file"):
        tagsort.mitochondrial_gene_ids(os.path.join(R.FIXTURES, "genes.gtf"), str(tmp_path / "none.txt"))


# ---- options ----
def _cli(tmp_path, **over):
    bam = tmp_path / "in.bam"
    bam.write_bytes(b"x")
    opts = {"--bam-input": str(bam), "--metric-type": "gene", "--metric-output": str(tmp_path / "m.csv"),
            "--compute-metric": None, "--barcode-tag": "CB", "--umi-tag": "UB", "--gene-tag": "GE"}
    opts.update(over)
    argv = []
    for k, v in opts.items():
        if v is False:
            continue
        argv += [k] if v is None else [k, v]
    return argv


@pytest.mark.parametrize("over,message", [
    ({"--compute-metric": False}, "either the sorted alignment info or metric computation"),
    ({"--metric-output": False}, "Must specify --metric-output"),
    ({"--metric-type": "molecule"}, "--metric-type must be"),
    ({"--metric-type": "cell"}, "gtf file name must be provided"),
    ({"--metric-type": "cell", "--gtf-file": "genes.gtf.GZ"}, "must not be gzipped"),
    ({"--bam-input": False}, "Must specify a input file name"),
    ({"--bam-input": "/nonexistent/in.bam"}, "is missing!"),
    ({"--temp-folder": "/nonexistent/tmp"}, "temp folder /nonexistent/tmp is missing!"),
    ({"--gene-tag": False}, "Must have three distinct tags"),
    ({"--gene-tag": "CB"}, "Must have three distinct tags"),
    ({"--alignments-per-thread": "999"}, "at least 1000"),
    ({"--nthreads": "31"}, "between 1 and 30"),
    ({"--nthreads": "0"}, "between 1 and 30"),
    ({"--metric-type": "umi"}, "umi is not supported"),
    ({"--output-sorted-info": None}, "--output-sorted-info is not supported"),
])
def test_cli_option_checks(tmp_path, over, message):
    with pytest.raises(tagsort.TagSortError, match=message):
        tagsort.main(_cli(tmp_path, **over))


def test_tag_order_follows_the_command_line():
    def order(*seq):
        return tagsort.resolve_tag_order("CB", "UB", "GE", [(r, {"barcode": "CB", "umi": "UB", "gene": "GE"}[r])
                                                            for r in seq])
    for roles in [("barcode", "umi", "gene"), ("barcode", "gene", "umi"), ("umi", "barcode", "gene"),
                  ("umi", "gene", "barcode"), ("gene", "umi", "barcode"), ("gene", "barcode", "umi")]:
        assert order(*roles) == roles
    from sctools_amd import platform
    assert platform.COMMANDS["TagSort"] == platform.GenericPlatform.tag_sort


def test_api_checks(tmp_path):
    bam = tmp_path / "in.bam"
    bam.write_bytes(b"x")
    with pytest.raises(tagsort.TagSortError, match="gtf file name must be provided"):
        tagsort.TagSort(str(bam), "cell", "CB", "UB", "GE")
    with pytest.raises(tagsort.TagSortError, match="three distinct tags"):
        tagsort.TagSort(str(bam), "gene", "CB", "CB", "GE")
    with pytest.raises(NotImplementedError):
        tagsort.TagSort(str(bam), "gene", "CB", "UB", "GE", decoder="device")


# ---- ranks ----
def test_rank_dictionary_puts_none_in_its_place():
    remap, names = tagsort.rank_dictionary([None, "AAA", "None", "Zeta", "alpha", "B,C"])
    assert names == ["AAA", "B,C", "None", "Zeta", "alpha"]  # byte order; the missing tag IS the word None
    assert remap.tolist() == [2, 0, 2, 3, 4, 1]
    arrays = {"cell": np.array([0, 1, 2], dtype=np.int32), "umi": np.array([0, 0, 1], dtype=np.int32),
              "gene": np.array([1, 2, 0], dtype=np.int32)}
    names3 = [[None, "AAA", "B"], [None, "u"], [None, "G1,G2", "mt"]]
    r = tagsort.Ranked(arrays, names3, ("gene", "barcode", "umi"), "gene", {"u"})
    assert r.names[0] == ["G1,G2", "None", "mt"] and r.first_drop.tolist() == [1, 1, 0]
    assert r.columns["cell"].tolist() == [0, 2, 1] and r.columns["umi"].tolist() == [2, 0, 1]
    assert r.names[2] == ["None", "u"] and r.third_is_mito.tolist() == [0, 1]
    assert tagsort.Ranked(arrays, names3, ("gene", "barcode", "umi"), "cell").first_drop.tolist() == [0, 1, 0]


# ---- the host decoder's mode against the per-read restatement ----
def _rec(name, tags, flag=0, ref=3, pos=100, cigar=((0, 10),), l_seq=10, qual=None):
    return types.SimpleNamespace(query_name=name, flag=flag, reference_id=ref, pos=pos, mapq=30, cigar=list(cigar),
                                 l_seq=l_seq, _qual=qual, _tags=dict(tags))


FULL = {"CB": "ACGT", "CR": "ACGT", "CY": "IIII", "UB": "TTT", "UR": "TTA", "UY": "I5@", "GE": "G1", "XF": "CODING",
        "NH": 1}


def _without(*keys, **set_):
    t = {k: v for k, v in FULL.items() if k not in keys}
    t.update(set_)
    return t


DECODE_RECORDS = [
    _rec("full", FULL, qual=bytes([40, 31, 30, 2, 0, 41, 12, 35, 33, 30])),
    _rec("no_cb", _without("CB")), _rec("no_ub", _without("UB")), _rec("no_ge", _without("GE")),
    _rec("dash_cb", _without(CB="-")), _rec("dash_ge", _without(GE="-")), _rec("dash_cr", _without(CR="-")),
    _rec("cb_missing_cr_none", _without("CB", CR="None")),  # strcmp("None", "None"): perfect
    _rec("no_nh", _without("NH")), _rec("nh2", _without(NH=2)),
    _rec("no_cy", _without("CY")), _rec("empty_cy", _without(CY="")), _rec("no_uy", _without("UY")),
    _rec("empty_uy", _without(UY="")), _rec("low_cy", _without(CY="I \x1f?@")),
    _rec("ref_none_flag_clear", FULL, flag=0, ref=-1, pos=-1),
    _rec("flag_unmapped_ref_set", FULL, flag=0x4, ref=2),
    _rec("soft_clips", FULL, cigar=((4, 3), (0, 5), (4, 2)), qual=bytes([40, 40, 40, 10, 10, 10, 10, 10, 35, 35])),
    _rec("n_zero", FULL, cigar=((0, 5), (3, 0), (0, 5))), _rec("n_real", FULL, cigar=((0, 5), (3, 700), (0, 5))),
    _rec("rev_dup", FULL, flag=0x10 | 0x400), _rec("no_qual", FULL, qual=None), _rec("no_seq", FULL, l_seq=0, cigar=()),
    _rec("xf_other", _without(XF="SOMETHING")), _rec("xf_empty", _without(XF="")), _rec("no_xf", _without("XF")),
    _rec("xf_intergenic", _without(XF="INTERGENIC")), _rec("multi", _without(GE="G1,G2")),
]


def test_host_decoder_tagsort_mode(tmp_path):
    path = str(tmp_path / "t.bam")
    bamwriter.write_bam(path, DECODE_RECORDS)
    arrays, names = bamnative.decode(path, "tagsort", tags=("CB", "UB", "GE"))
    assert len(arrays["cell"]) == len(DECODE_RECORDS)
    for k, rec in enumerate(DECODE_RECORDS):
        want = R.read_fields(rec)
        who = rec.query_name
        assert names[0][arrays["cell"][k]] == want["barcode"], who
        assert names[1][arrays["umi"][k]] == want["umi"], who
        assert names[2][arrays["gene"][k]] == want["gene"], who
        bits = int(arrays["bits"][k])
        got = {"mapped": int(not bits & 0x01), "strand": (bits >> 1) & 1, "dup": (bits >> 2) & 1,
               "spliced": (bits >> 3) & 1, "nh1": (bits >> 4) & 1, "perfect_umi": (bits >> 5) & 1,
               "perfect_cb": (bits >> 7) & 1, "xf": int(arrays["xf"][k]), "ref": int(arrays["ref"][k]),
               "pos": int(arrays["pos"][k])}
        for f in ("cy_gt30", "cy_len", "uy_gt30", "uy_len", "gq_sum", "gq_len", "gq_gt30"):
            got[f] = int(arrays[f][k])
        exp = {f: want[f] for f in got if f != "xf"}
        exp["xf"] = R.XF_CODE.get(want["xf"], 5)
        assert got == exp, who
    by = {r.query_name: k for k, r in enumerate(DECODE_RECORDS)}
    assert arrays["gq_len"][by["soft_clips"]] == 10 and arrays["gq_sum"][by["soft_clips"]] == 240  # whole read
    assert not arrays["bits"][by["flag_unmapped_ref_set"]] & 0x01 and arrays["bits"][by["ref_none_flag_clear"]] & 0x01
    assert arrays["bits"][by["cb_missing_cr_none"]] & 0x80 and not arrays["bits"][by["n_zero"]] & 0x08


def test_host_decoder_tagsort_mode_errors(tmp_path):
    path = str(tmp_path / "wide.bam")
    bamwriter.write_bam(path, [_rec("ok", FULL), _rec("wide", _without(CY="I" * 256))])
    with pytest.raises(ValueError, match="columnar limits"):
        bamnative.decode(path, "tagsort", tags=("CB", "UB", "GE"))
    bamwriter.write_bam(path, [_rec("typed", _without(CB=7))])
    with pytest.raises(bamnative.TypedTagValue):
        bamnative.decode(path, "tagsort", tags=("CB", "UB", "GE"))
    bamwriter.write_bam(path, [])
    arrays, _ = bamnative.decode(path, "tagsort", tags=("CB", "UB", "GE"))
    assert len(arrays["cell"]) == 0
