"""bench.py's command line: a plain run is lean and can show its work (--dump-outputs), --full adds the rest.

One small config-2-shaped shard (200k records, 40 cells, 500 genes), each mode started once:
* the result line carries the headline fields and the number of timed steps asked for;
* a plain run carries none of what --full measures (kernel table, roofline, side measurements,
  CPU baseline), a --full run carries all of it;
* the dumped arrays are float64 and finite, hold every record once, and are the rows the engine
  gives in this process for the same generated shard, its NaN entries written as 0 and marked in
  <name>_nonfinite.npy.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDS, CELLS, GENES, STEPS = 200_000, 40, 500, 3
FULL_ONLY = ("roofline", "sort_model_yardstick", "kernel_ms_per_step", "kernel_items_per_step", "cpu_baseline",
             "speedup_vs_cpu_baseline", "reference_python", "allreduce_ms", "h2d", "count_entities_ms",
             "dropin_cell_welford_ms", "records_per_s_incl_h2d_and_count")


@pytest.fixture(scope="module")
def rows():
    """The engine's rows for the bench's shard of these sizes (seed 0), computed once in this process."""
    from sctools_amd import engine as E
    from sctools_amd import synth

    dev = torch.device("cuda", 0)
    eng = E.get_engine(dev)
    d = synth.generate(synth.SynthConfig(n_reads=RECORDS, n_cells=CELLS, n_genes=GENES, sigma=1.0, seed=0,
                                         umi_bits=20), device=dev, chunk=16_000_000)
    dims = E.Dims(d.n_cell_ids, d.n_gene_ids, d.n_umi_ids)
    mito = torch.from_numpy(d.gene_is_mito).to(dev)
    partials = torch.empty((d.n_gene_ids, 64), dtype=torch.int64, device=dev)
    ci, cf, _ = eng.cell_and_gene(d.cols, dims, mito, partials=partials)
    gi, gf = eng.finalize_partials(partials)
    return {"cell_int": ci.cpu().numpy(), "cell_float": cf.cpu().numpy(), "gene_int": gi.cpu().numpy(),
            "gene_float": gf.cpu().numpy()}


@pytest.mark.parametrize("mode", ["plain", "full"])
def test_bench_line_and_dumped_outputs(tmp_path, rows, mode):
    out = str(tmp_path / "dump")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
           "--records", str(RECORDS), "--cells", str(CELLS), "--genes", str(GENES), "--dump-outputs", out]
    if mode == "full":
        cmd += ["--full", "--cpu-sample-s", "0.2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout  # ONE result line
    d = json.loads(lines[0])
    assert d["metric"] == "aligned records/sec for cell+gene metrics" and d["unit"] == "records/s"
    assert d["higher_is_better"] is True and d["dtype"] == "int64"
    assert d["steps"] == STEPS and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(RECORDS / (d["ms_per_step"] / 1e3), rel=1e-9)
    if mode == "plain":
        assert d["full"] is False and not [k for k in FULL_ONLY if k in d]
    else:
        assert d["full"] is True and not [k for k in FULL_ONLY if k not in d]
        assert d["cpu_baseline"]["value"] > 0 and d["kernel_ms_per_step"] and d["roofline"]["kernel"]
    floats = [k for k in rows if k.endswith("float")]
    assert sorted(os.listdir(out)) == sorted([k + ".npy" for k in rows] + [k + "_nonfinite.npy" for k in floats])
    assert np.isnan(rows["gene_float"]).any()  # (gene ids without records: the case the marks are for)
    for k, want in rows.items():
        got = np.load(os.path.join(out, k + ".npy"))
        assert got.dtype == np.float64 and got.shape == want.shape, k
        assert np.isfinite(got).all(), k
        if k in floats:  # NaN is written as 0 and marked; the engine gives no infinities here
            mark = np.load(os.path.join(out, k + "_nonfinite.npy"))
            assert mark.dtype == np.float32 and np.array_equal(mark, np.isnan(want).astype(np.float32)), k
            assert not np.isinf(want).any(), k
            want = np.where(np.isnan(want), 0.0, want)
        assert np.array_equal(got, want.astype(np.float64)), k
    assert np.load(os.path.join(out, "cell_int.npy"))[:, 0].sum() == RECORDS
    assert np.load(os.path.join(out, "gene_int.npy"))[:, 0].sum() == RECORDS
