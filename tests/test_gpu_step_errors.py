"""A rejected call of the metric step leaves nothing behind (beside
test_gpu_buckets.py::test_ids_outside_the_dictionaries_are_rejected, on its data).

A UMI id past the dictionary makes the step return early (SCT_EINVAL, not a fault: the key pass clamps
ids), with side streams forked and, on the planned path, the level-1 readback queued.  StepStreams'
destructor (csrc/streams.h) drains the streams and waits for the copy, so the same engine on the same
workspace gives the right rows straight afterwards.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_buckets import _same_rows, compare, craft

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from sctools_amd import engine as E

    return E.get_engine("cuda:0")


@pytest.mark.parametrize("call", ["compute_exact", "compute_welford", "cell_and_gene"])
def test_a_rejected_call_leaves_nothing_behind(eng, call):
    """The rejected call, then at once the clean records on the same engine: the rows equal the oracle's
    and, bit for bit, a fresh engine's."""
    from sctools_amd import _native as N
    from sctools_amd import engine as E

    arrays, mito, n_cells = craft(300, 4096, 4)
    bad = {k: v.copy() for k, v in arrays.items()}
    bad["umi"][len(bad["umi"]) // 2] = 4096 + 5
    dims = E.Dims(n_cells, 300, 4096)
    cols, bad_cols = E.to_device(arrays, eng.device), E.to_device(bad, eng.device)
    gm = torch.from_numpy(mito).to(eng.device)
    float_mode = "welford" if call == "compute_welford" else "exact"

    def run(e, c):
        if call == "cell_and_gene":
            ci, cf, part = e.cell_and_gene(c, dims, gm)
            gi, gf = e.finalize_partials(part)
            return {"cell": (ci.cpu().numpy(), cf.cpu().numpy()), "grouped": (gi.cpu().numpy(), gf.cpu().numpy())}
        gi, gf = e.compute(c, "cell", dims, gm, gm, float_mode=float_mode)
        return {"cell": (gi.cpu().numpy(), gf.cpu().numpy())}

    with pytest.raises(N.EngineError, match="outside"):
        run(eng, bad_cols)
    got = run(eng, cols)
    oi, of = O.run(arrays, "cell", mito, 300, threads=8)
    compare(*got["cell"], oi, of, exact=float_mode == "welford")
    if call == "cell_and_gene":
        oi, of = O.run(arrays, "gene_grouped", mito, 300, threads=8)
        gi, gf = got["grouped"]
        live = oi[:, 0] > 0
        assert np.array_equal(gi[:, 0] > 0, live)
        compare(gi[live], gf[live], oi[live], of[live], exact=False)
    _same_rows(run(E.Engine(eng.device), cols), got)
