"""The exact quality-stream lanes as a kernel of their own (segment.h k_stream_lanes, round 8).

On the planned bucket path with exact floats the lanes leave the key pass and run on the side pool's
second stream.  Every shard here is small and built on the host so that one branch of stream_tile
decides the rows: partial and exact tiles, run boundaries at tile, thread and half edges and inside a
thread's items, records that miss the per-tile increment table, tiles without a table, zero operands,
and the wide gene payload flag that k_gene_emit reads after the lanes kernel set it.  Each shard's
rows are held to the oracle and, bit for bit, to the fused launch (SCT_STREAM_LANES=fused).
"""
import threading

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_buckets import REL, _same_rows, kernels_run

pytestmark = pytest.mark.gpu

N_GENE_IDS = 30_000  # 15 bits of k1: the first partition level is planned
N_UMI_IDS = 1 << 20
N_CELL_IDS_MIN = 300  # the gene view's k1 is the cell: >= 8 bits for the planned path
T = 8192  # the key pass's tile (segment.h kKTile)
SPLIT = ("pre",)  # the split placement the engine has (the default)


@pytest.fixture(scope="module")
def eng():
    from sctools_amd import engine as E

    return E.get_engine("cuda:0")


def shard(n, heads, seed, view="cell"):
    """n records whose entity column (cell, or gene for view="gene") starts a run at every position in
    `heads` (and at 0), other columns random with fixed barcode lengths (uy 10, cy 16)."""
    rng = np.random.default_rng(seed)
    start = np.zeros(n, np.int64)
    start[[h for h in heads if 0 < h < n]] = 1
    ent = np.cumsum(start).astype(np.int32)
    n_ent = int(ent[-1]) + 1
    assert n_ent <= N_GENE_IDS
    n_cell_ids = max(n_ent, N_CELL_IDS_MIN)
    other = rng.integers(0, N_GENE_IDS if view == "cell" else N_CELL_IDS_MIN, n).astype(np.int32)
    unm = rng.random(n) < 0.05
    bits = np.where(unm, 1, 0) | np.where(rng.random(n) < 0.5, 2, 0) | 64
    bits |= np.where(~unm & (rng.random(n) < 0.3), 4, 0) | np.where(rng.random(n) < 0.9, 32, 0)
    bits |= np.where(~unm & (rng.random(n) < 0.8), 16, 0) | np.where(rng.random(n) < 0.95, 128, 0)
    glen = rng.integers(30, 99, n)
    arrays = {
        "cell": ent if view == "cell" else other, "gene": other if view == "cell" else ent,
        "umi": rng.integers(0, N_UMI_IDS, n).astype(np.int32),
        "ref": np.where(unm, -1, rng.integers(0, 25, n)).astype(np.int32),
        "pos": np.where(unm, -1, rng.integers(0, 1 << 20, n)).astype(np.int32),
        "gq_len": glen.astype(np.uint16), "gq_sum": (glen * rng.integers(20, 40, n)).astype(np.uint16),
        "gq_gt30": rng.integers(0, glen + 1).astype(np.uint16), "bits": bits.astype(np.uint8),
        "xf": np.where(unm, 0, rng.integers(1, 5, n)).astype(np.uint8),
        "cy_len": np.full(n, 16, np.uint8), "cy_gt30": rng.integers(0, 17, n).astype(np.uint8),
        "uy_len": np.full(n, 10, np.uint8), "uy_gt30": rng.integers(0, 11, n).astype(np.uint8),
    }
    mito = np.zeros(N_GENE_IDS, np.uint8)
    mito[::97] = 1
    return arrays, mito, n_cell_ids


def rows_of(eng, arrays, mito, n_cell_ids, view):
    """view "cell": the cell rows, the combined call's cell rows and its grouped gene rows; "gene": the gene rows"""
    from sctools_amd import engine as E

    dims = E.Dims(n_cell_ids, N_GENE_IDS, N_UMI_IDS)
    cols = E.to_device(arrays, eng.device)
    gm = torch.from_numpy(mito).to(eng.device)
    out = {}
    gi, gf = eng.compute(cols, view, dims, gm, gm, float_mode="exact")
    out[view] = (gi.cpu().numpy(), gf.cpu().numpy())
    if view == "cell":
        ci, cf, part = eng.cell_and_gene(cols, dims, gm)
        gi, gf = eng.finalize_partials(part)
        out["combined_cell"] = (ci.cpu().numpy(), cf.cpu().numpy())
        out["grouped"] = (gi.cpu().numpy(), gf.cpu().numpy())
    return out


def near(gi, gf, oi, of, skip_rows=()):
    """integers and NaN positions exactly, floats within REL (the exact-mode comparison of test_gpu_buckets.py);
    skip_rows: rows whose floats the oracle does not define (below)"""
    assert gi.shape == oi.shape
    assert np.array_equal(gi, oi), np.argwhere(gi != oi)[:10]
    keep = np.ones(len(gf), bool)
    keep[list(skip_rows)] = False
    gf, of = gf[keep], of[keep]
    ng, no = np.isnan(gf), np.isnan(of)
    assert np.array_equal(ng, no)
    x, y = gf[~ng], of[~no]
    rel = np.abs(x - y) / np.maximum(np.maximum(np.abs(x), np.abs(y)), 1e-300)
    assert (rel <= REL).all(), rel.max()


def check(eng, monkeypatch, arrays, mito, n_cell_ids, view, skip_rows=()):
    monkeypatch.setenv("SCT_STREAM_LANES", "fused")
    fused = rows_of(eng, arrays, mito, n_cell_ids, view)
    oi, of = O.run(arrays, view, mito, N_GENE_IDS, threads=8)
    near(*fused[view], oi, of, skip_rows)
    if view == "cell":
        near(*fused["combined_cell"], oi, of, skip_rows)
        if not len(skip_rows):
            oi, of = O.run(arrays, "gene_grouped", mito, N_GENE_IDS, threads=8)
            gi, gf = fused["grouped"]
            live = oi[:, 0] > 0
            assert np.array_equal(gi[:, 0] > 0, live)
            near(gi[live], gf[live], oi[live], of[live])
    for at in SPLIT:
        monkeypatch.setenv("SCT_STREAM_LANES", at)
        _same_rows(fused, rows_of(eng, arrays, mito, n_cell_ids, view))
    monkeypatch.delenv("SCT_STREAM_LANES")
    _same_rows(fused, rows_of(eng, arrays, mito, n_cell_ids, view))


# run boundaries: every branch of stream_tile's flush logic
BOUNDARIES = {
    "every_record": (T + 5, list(range(1, T + 5))),  # the per-thread flush at every item
    "tile_edges": (3 * T + 17, [T, 2 * T, 3 * T]),
    "thread_edges": (2 * T + 40, [32, 64, 96, 32 * 100, T - 32, T + 32, 2 * T + 32]),
    "half_edges": (2 * T + 40, [16, 48, 32 * 100 + 16, T - 16, T + 16, 2 * T + 16]),
    "odd_inside_a_thread": (2 * T + 40, [32 * 129 + 3]),
}


@pytest.mark.parametrize("view", ["cell", "gene"])
@pytest.mark.parametrize("n", [1, 255, T - 1, T, T + 1, 3 * T + 17])
def test_single_run_sizes(eng, monkeypatch, n, view):
    """a lone thread, the partial-tile load path, an exact tile, a tail tile of one record"""
    arrays, mito, nc = shard(n, [], 100 + n, view)
    check(eng, monkeypatch, arrays, mito, nc, view)


@pytest.mark.parametrize("view", ["cell", "gene"])
@pytest.mark.parametrize("name", list(BOUNDARIES))
def test_run_boundaries(eng, monkeypatch, name, view):
    n, heads = BOUNDARIES[name]
    arrays, mito, nc = shard(n, heads, 7, view)
    check(eng, monkeypatch, arrays, mito, nc, view)


@pytest.mark.parametrize("view", ["cell", "gene"])
def test_records_that_miss_the_tile_table_and_zero_numerators(eng, monkeypatch, view):
    """Tile 0's first record has uy_len 10 and cy_len 16, so both tables exist; records with other
    lengths (and numerators above their own length's table range) compute their increments in place.
    Tile 1's first record has uy_len 40: no uy table.  Whole stretches of zero numerators."""
    n = 2 * T + 100
    arrays, mito, nc = shard(n, [5000, T + 77], 21, view)
    rng = np.random.default_rng(22)
    odd = rng.choice(np.arange(1, n), 900, replace=False)
    odd = odd[odd != T]
    arrays["uy_len"][odd] = rng.integers(1, 60, odd.size)
    arrays["uy_gt30"][odd] = rng.integers(0, arrays["uy_len"][odd] + 1)
    arrays["cy_len"][odd] = rng.integers(1, 40, odd.size)
    arrays["cy_gt30"][odd] = rng.integers(0, arrays["cy_len"][odd] + 1)
    arrays["uy_len"][T], arrays["uy_gt30"][T] = 40, 33
    for c in ("uy_gt30", "cy_gt30", "gq_gt30", "gq_sum"):
        arrays[c][300:900] = 0
        arrays[c][T + 4000:T + 4100] = 0
    check(eng, monkeypatch, arrays, mito, nc, view)


@pytest.mark.parametrize("view", ["cell", "gene"])
def test_zero_denominators(eng, monkeypatch, view):
    """A record with a zero length adds nothing to the lanes (util.h: a / 0 = 0), where the oracle's
    0 / 0 makes its run's means NaN: those records sit in run 1 alone, whose floats are not held to
    the oracle; its integers, every other run, and bit-identity between the launches are."""
    n = T + 900
    arrays, mito, nc = shard(n, [2000, 4000, T + 10], 31, view)
    z = np.arange(2100, 3900, 7)
    for num, den in (("uy_gt30", "uy_len"), ("cy_gt30", "cy_len"), ("gq_gt30", "gq_len")):
        arrays[den][z] = 0
        arrays[num][z] = 0
    arrays["gq_sum"][z] = 0
    check(eng, monkeypatch, arrays, mito, nc, view, skip_rows=(1,))


@pytest.mark.parametrize("wide", [False, True])
def test_gene_emit_waits_for_the_wide_payload_flag(eng, monkeypatch, wide):
    """One record with gq_len 600 does not fit the narrow gene payload: the lanes kernel raises the
    flag k_gene_emit reads.  The grouped gene rows match the oracle with and without that record."""
    arrays, mito, nc = shard(3 * T + 17, [T + 5, 2 * T + 900], 41, "cell")
    if wide:
        arrays["gq_len"][2 * T + 1234] = 600
        arrays["gq_gt30"][2 * T + 1234] = 555
        arrays["gq_sum"][2 * T + 1234] = 600 * 35
    check(eng, monkeypatch, arrays, mito, nc, "cell")


def test_which_launches_run_the_lanes_kernel(eng, monkeypatch):
    from sctools_amd import engine as E

    arrays, mito, nc = shard(2 * T + 40, [T + 3], 51, "cell")
    garrays, _, gnc = shard(2 * T + 40, [T + 3], 51, "gene")
    gm = torch.from_numpy(mito).to(eng.device)
    cols, gcols = E.to_device(arrays, eng.device), E.to_device(garrays, eng.device)
    dims, gdims = E.Dims(nc, N_GENE_IDS, N_UMI_IDS), E.Dims(gnc, N_GENE_IDS, N_UMI_IDS)
    calls = {
        "cell": lambda fm="exact": eng.compute(cols, "cell", dims, gm, gm, float_mode=fm),
        "gene": lambda fm="exact": eng.compute(gcols, "gene", gdims, gm, gm, float_mode=fm),
        "combined": lambda fm="exact": eng.cell_and_gene(cols, dims, gm),
    }
    monkeypatch.delenv("SCT_STREAM_LANES", raising=False)
    for name, call in calls.items():
        assert "stream_lanes" in kernels_run(eng, call), name
    for at in SPLIT:
        monkeypatch.setenv("SCT_STREAM_LANES", at)
        for name, call in calls.items():
            ran = kernels_run(eng, call)
            assert "stream_lanes" in ran and "build_keys" in ran, (at, name)
    monkeypatch.setenv("SCT_STREAM_LANES", "fused")
    for name, call in calls.items():
        assert "stream_lanes" not in kernels_run(eng, call), name
    monkeypatch.delenv("SCT_STREAM_LANES")
    for name in ("cell", "gene"):
        assert "stream_lanes" not in kernels_run(eng, lambda: calls[name]("welford")), name
    monkeypatch.setenv("SCT_NO_SIDE", "1")
    for name, call in calls.items():
        assert "stream_lanes" not in kernels_run(eng, call), name


def test_two_calls_at_once_on_two_streams(eng):
    """The second call finds the side pool's pair taken and keeps the fused launch; both calls' rows
    equal the single call's."""
    from sctools_amd import engine as E
    from sctools_amd import synth

    d = synth.generate(synth.SynthConfig(n_reads=200_000, n_cells=40, n_genes=N_GENE_IDS, seed=11), device=eng.device)
    dims = E.Dims(d.n_cell_ids, d.n_gene_ids, d.n_umi_ids)
    mito = torch.from_numpy(d.gene_is_mito).to(eng.device)

    def rows(e):
        ci, cf, part = e.cell_and_gene(d.cols, dims, mito)
        gi, gf = e.finalize_partials(part)
        torch.cuda.current_stream(eng.device).synchronize()
        return {"cell": (ci.cpu().numpy(), cf.cpu().numpy()), "gene": (gi.cpu().numpy(), gf.cpu().numpy())}

    assert "stream_lanes" in kernels_run(eng, lambda: eng.cell_and_gene(d.cols, dims, mito))
    single = rows(eng)
    torch.cuda.synchronize()
    got, errors = {}, []
    gate = threading.Barrier(2)

    def worker(k):
        try:
            e = E.Engine(eng.device)  # a workspace of its own
            with torch.cuda.stream(torch.cuda.Stream(eng.device)):
                gate.wait(timeout=30)
                got[k] = [rows(e) for _ in range(4)]
        except Exception as ex:  # noqa: BLE001 (reported by the assertion below)
            errors.append(ex)

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        for r in got[k]:
            _same_rows(single, r)
