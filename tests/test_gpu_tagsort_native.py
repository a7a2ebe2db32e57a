"""TagSort on the GPU: sct_tagsort_metrics (csrc/tsmetrics.h) behind sctools_amd.tagsort, byte for byte
against the CSVs recorded from the reference's gatherer and, on generated input, against the Python
restatement of it (tests/tagsort_ref.py, itself pinned to those CSVs by the CPU tests)."""
import os

import numpy as np
import pytest

import tagsort_ref as R
from sctools_amd import tagsort

pytestmark = pytest.mark.gpu

GTF = os.path.join(R.FIXTURES, "genes.gtf")
NAMES = os.path.join(R.FIXTURES, "mito_names.txt")
UNSORTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bam", "unsorted.bam")


def _first_difference(got, want):
    g, w = got.split("\n"), want.split("\n")
    for k in range(max(len(g), len(w))):
        a, b = (g[k] if k < len(g) else None), (w[k] if k < len(w) else None)
        if a != b:
            return "line %d:\n got  %s\n want %s" % (k, a, b)
    return "equal"


def _csv_of(arrays, names, roles, metric_type, mito, tmp_path, presorted=False):
    ranked = tagsort.Ranked(arrays, names, roles, metric_type, mito)
    rows = tagsort.gather(ranked, metric_type, presorted=presorted)
    path = tagsort.write_metrics(rows, str(tmp_path / "metrics.csv"))
    with open(path, newline="") as f:
        return f.read()


# ---- every fixture case: the bytes the reference's gatherer wrote ----
@pytest.mark.parametrize("metric_type", ["cell", "gene"])
@pytest.mark.parametrize("name", R.case_names())
def test_fixture_case_bytes(name, metric_type, tmp_path):
    arrays, names = R.engine_arrays(R.load_case(name))
    mito = tagsort.mitochondrial_gene_ids(GTF, NAMES)
    got = _csv_of(arrays, names, tagsort.ROLES, metric_type, mito, tmp_path, presorted=True)
    want = R.recorded(name, metric_type)
    assert got == want, _first_difference(got, want)


# ---- generated reads ----
def _dictionary(prefix, k, with_none):
    strings = sorted("%s%04d" % (prefix, i) for i in range(k))
    return ([None] if with_none else []) + strings


def _reads(rng, cell_ids, names, n_umi, n_gene, p_unmapped, p_none):
    """Decoder-style arrays for reads whose barcode ids are given; umi / gene ids random over small
    dictionaries (id 0 = a missing tag, with probability p_none); qualities over every length class."""
    n = len(cell_ids)
    a = {"cell": np.asarray(cell_ids, dtype=np.int32)}
    for col, k in (("umi", n_umi), ("gene", n_gene)):
        ids = rng.integers(1, k + 1, n)
        ids[rng.random(n) < p_none] = 0
        a[col] = ids.astype(np.int32)
    unmapped = rng.random(n) < p_unmapped
    a["ref"] = np.where(unmapped, -1, rng.integers(0, 3, n)).astype(np.int32)
    a["pos"] = np.where(unmapped, 0, rng.integers(0, 12, n) * 50).astype(np.int32)
    bits = unmapped.astype(np.uint8)
    for bit, p in ((0x02, 0.5), (0x04, 0.1), (0x08, 0.2), (0x10, 0.8), (0x20, 0.9), (0x80, 0.9)):
        bits |= (rng.random(n) < p).astype(np.uint8) * np.uint8(bit)
    a["bits"] = bits
    a["xf"] = np.where(unmapped & (rng.random(n) < 0.7), 0, rng.integers(0, 6, n)).astype(np.uint8)
    gl = np.where(rng.random(n) < 0.01, 0, rng.integers(20, 151, n))
    a["gq_len"] = gl.astype(np.uint16)
    a["gq_gt30"] = (rng.random(n) * (gl + 1)).astype(np.uint16)
    a["gq_sum"] = (rng.random(n) * (41 * gl + 1)).astype(np.uint16)
    for q, full in (("cy", 16), ("uy", 10)):
        ln = np.where(rng.random(n) < 0.01, 0, full)
        a[q + "_len"] = ln.astype(np.uint8)
        a[q + "_gt30"] = (rng.random(n) * (ln + 1)).astype(np.uint8)
    return a, [names, _dictionary("U", n_umi, True), _dictionary("G", n_gene, True)]


def _check(arrays, names, roles, metric_type, mito, tmp_path):
    got = _csv_of(arrays, names, roles, metric_type, mito, tmp_path)
    want = R.gather(R.stable_sorted(R.columns_from_arrays(arrays, names, roles)), metric_type, mito)
    assert got == want, _first_difference(got, want)
    return got


# entity sizes around what the kernels tile by: ts_chains walks 64 records at a time, ts_records runs
# 256-record blocks of 64-lane waves, triplet runs up to 32 records are scanned and longer ones hashed
SIZES = {
    "around_the_tiles": ([1, 63, 64, 65, 2047, 2048, 2049, 5000], 0.1, 12, 6),
    # entities start at 0, 64, 128, 255, 256, 512, 767, 768, 1024, 1025: rows that begin on the first and on
    # the last record of a block and of a wave; every read mapped, so each entity closes exactly one row
    "boundaries_on_tile_edges": ([64, 64, 127, 1, 256, 255, 1, 256, 1, 300], 0.0, 3, 2),
    # two umis and one gene: triplet runs of hundreds of records that straddle waves and blocks
    "long_runs": ([700, 33, 32, 31, 1500], 0.05, 2, 1),
    "one_record": ([1], 0.0, 1, 1),
}


@pytest.mark.parametrize("metric_type", ["cell", "gene"])
@pytest.mark.parametrize("case", sorted(SIZES))
def test_row_lengths_around_the_tiles(case, metric_type, tmp_path):
    sizes, p_unmapped, n_umi, n_gene = SIZES[case]
    rng = np.random.default_rng(len(case))
    cells = _dictionary("C", len(sizes), False)
    ids = np.repeat(np.arange(len(sizes)), sizes)
    arrays, names = _reads(rng, rng.permutation(ids), cells, n_umi, n_gene, p_unmapped, 0.02)
    got = _check(arrays, names, tagsort.ROLES, metric_type, {"G0001"}, tmp_path)
    if p_unmapped == 0.0:
        assert got.count("\n") == 1 + len(sizes)


RANDOM = {"cell_barcode_umi_gene": ("cell", ("barcode", "umi", "gene")),
          "gene_gene_barcode_umi": ("gene", ("gene", "barcode", "umi")),
          "cell_umi_gene_barcode": ("cell", ("umi", "gene", "barcode"))}


@pytest.mark.parametrize("case", sorted(RANDOM))
def test_200k_random_records(case, tmp_path):
    metric_type, roles = RANDOM[case]
    rng = np.random.default_rng(7)
    n, n_cell = 200_000, 150
    cells = [None] + _dictionary("C", n_cell, False) + ["C0001,C0002"]
    cell_ids = rng.integers(1, len(cells), n)
    cell_ids[rng.random(n) < 0.05] = 0
    arrays, names = _reads(rng, cell_ids, cells, 40, 25, 0.10, 0.05)
    names[2] = names[2] + ["G0001,G0002"]
    arrays["gene"][rng.random(n) < 0.01] = len(names[2]) - 1
    _check(arrays, names, roles, metric_type, {"G0002", "G0007", "U0003", "C0005"}, tmp_path)


# ---- end to end on the bundled unsorted BAM ----
@pytest.mark.parametrize("metric_type", ["cell", "gene"])
def test_end_to_end_unsorted_bam(metric_type, tmp_path):
    from sctools_amd import bamnative

    roles = ("barcode", "umi", "gene") if metric_type == "cell" else ("gene", "barcode", "umi")
    ts = tagsort.TagSort(UNSORTED, metric_type, "CB", "UB", "GE", tag_order=roles, gtf_file=GTF,
                         mitochondrial_gene_names_filename=NAMES, decoder="host")
    rows, path = ts.run(str(tmp_path / "e2e.csv"))
    with open(path, newline="") as f:
        got = f.read()
    arrays, names = bamnative.decode(UNSORTED, "tagsort", tags=("CB", "UB", "GE"))
    mito = tagsort.mitochondrial_gene_ids(GTF, NAMES)
    want = R.gather(R.stable_sorted(R.columns_from_arrays(arrays, names, roles)), metric_type, mito)
    assert got == want, _first_difference(got, want)
    assert len(rows) == got.count("\n") - 1 and len(rows) > 1
    auto = tagsort.TagSort(UNSORTED, metric_type, "CB", "UB", "GE", tag_order=roles, gtf_file=GTF,
                           mitochondrial_gene_names_filename=NAMES).run(str(tmp_path / "auto.csv"))[0]
    assert auto.text() == got  # "auto" picks a decoder that was built: the same bytes


def test_cli_writes_the_file(tmp_path):
    from sctools_amd.__main__ import main

    out = tmp_path / "cli.csv"
    rc = main(["TagSort", "--bam-input", UNSORTED, "--metric-type", "gene", "--compute-metric", "--metric-output",
               str(out), "--gene-tag", "GE", "--barcode-tag", "CB", "--umi-tag", "UB", "--nthreads", "2"])
    assert rc == 0
    api = tagsort.TagSort(UNSORTED, "gene", "CB", "UB", "GE", tag_order=("gene", "barcode", "umi"))
    assert out.read_text() == api.run(str(tmp_path / "api.csv"))[0].text()
    assert out.read_text().startswith(",n_reads,noise_reads,")


def test_unsorted_records_are_rejected():
    import torch

    from sctools_amd import _native as N
    from sctools_amd import engine as E

    arrays, names = R.engine_arrays(R.load_case("unmapped_starts"))
    for col in ("cell", "umi", "gene", "bits"):
        arrays[col] = arrays[col][::-1].copy()
    ranked = tagsort.Ranked(arrays, names, tagsort.ROLES, "gene")
    with pytest.raises(N.EngineError, match="not sorted"):
        tagsort.gather(ranked, "gene", presorted=True)
    eng = E.get_engine()
    cols = E.to_device(ranked.columns, eng.device)
    cols["gene"] = cols["gene"] + 1000
    with pytest.raises(N.EngineError, match="outside its dictionary"):
        eng.tagsort_metrics(cols, E.Dims(len(ranked.names[0]), len(ranked.names[2]), len(ranked.names[1])), "gene",
                            torch.from_numpy(ranked.first_drop).to(eng.device))
