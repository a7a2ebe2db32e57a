"""The metric step's launches, held to a table recorded from the commit before the step driver was
reorganised (StepStreams, StepSwitches, the stage functions of sct_engine.hip).

Two small shards -- the crafted bucket edge cases of test_gpu_buckets.py and the two-tile pair of
test_gpu_stream_lanes.py -- run through every entry point of the step (cell / gene rows with exact
and Welford floats, the combined cell + gene call, grouped gene partials) under each switch that
changes which kernels the driver launches.  {kernel: launches}, counted by the engine's own profile
scopes, must equal tests/golden/engine/step_launches.json, and the rows must be bit-identical to the
rows without a switch.

The table is regenerated only on purpose, against the library that is the reference for the change:
collect_table() below is what recorded it.
"""
import json
import os

import pytest
import torch

from test_gpu_buckets import _same_rows, craft
from test_gpu_stream_lanes import N_GENE_IDS, N_UMI_IDS, T, shard

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine", "step_launches.json")

SWITCHES = [
    {},
    {"SCT_NO_SIDE": "1"},
    {"SCT_NO_L1_PLAN": "1"},
    {"SCT_FORCE_GLOBAL_SORT": "1"},
    {"SCT_STREAM_LANES": "fused"},
    {"SCT_NO_EARLY_BIG": "1"},
    {"SCT_NO_WF_GATE": "1"},
]
CASES = ["craft", "lanes_pair"]


def switch_id(sw):
    return ",".join(f"{k}={v}" for k, v in sw.items()) or "none"


@pytest.fixture(scope="module")
def eng():
    from sctools_amd import engine as E

    return E.get_engine("cuda:0")


def load_case(eng, name):
    """{"cell": (cols, dims), "gene": (cols, dims), "mito": tensor}: the records each view runs on"""
    from sctools_amd import engine as E

    if name == "craft":
        arrays, mito, n_cells = craft(300, 4096, 6)
        cell = gene = (E.to_device(arrays, eng.device), E.Dims(n_cells, 300, 4096))
    else:
        arrays, mito, nc = shard(2 * T + 40, [T + 3], 51, "cell")
        garrays, _, gnc = shard(2 * T + 40, [T + 3], 51, "gene")
        cell = (E.to_device(arrays, eng.device), E.Dims(nc, N_GENE_IDS, N_UMI_IDS))
        gene = (E.to_device(garrays, eng.device), E.Dims(gnc, N_GENE_IDS, N_UMI_IDS))
    return {"cell": cell, "gene": gene, "mito": torch.from_numpy(mito).to(eng.device)}


def step_runs(eng, case):
    """{run name: call returning {key: (ints, floats)}}"""
    gm = case["mito"]

    def compute(view, fm):
        cols, dims = case[view]
        gi, gf = eng.compute(cols, view, dims, gm, gm, float_mode=fm)
        return {"rows": (gi.cpu().numpy(), gf.cpu().numpy())}

    def cell_and_gene():
        cols, dims = case["cell"]
        ci, cf, part = eng.cell_and_gene(cols, dims, gm)
        gi, gf = eng.finalize_partials(part)
        return {"cell": (ci.cpu().numpy(), cf.cpu().numpy()), "grouped": (gi.cpu().numpy(), gf.cpu().numpy())}

    def gene_partials():
        cols, dims = case["cell"]
        gi, gf = eng.finalize_partials(eng.gene_partials(cols, dims))
        return {"grouped": (gi.cpu().numpy(), gf.cpu().numpy())}

    runs = {f"{view}_{fm}": (lambda view=view, fm=fm: compute(view, fm))
            for view in ("cell", "gene") for fm in ("exact", "welford")}
    runs["cell_and_gene"] = cell_and_gene
    runs["gene_partials"] = gene_partials
    return runs


def collect(eng, case, switches):
    """({run: {kernel: launches}}, {run: rows}) of one case under one switch setting"""
    saved = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)
    launches, rows = {}, {}
    try:
        for name, call in step_runs(eng, case).items():
            eng.profile_only("")
            eng.profile_read()  # (resets the counters)
            eng.profile_enable(True)
            try:
                rows[name] = call()
                torch.cuda.synchronize()
            finally:
                eng.profile_enable(False)
            launches[name] = {k: int(v[1]) for k, v in sorted(eng.profile_read().items())}
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return launches, rows


def collect_table(eng):
    """{case: {switch setting: {run: {kernel: launches}}}}: what the golden file holds"""
    return {name: {switch_id(sw): collect(eng, load_case(eng, name), sw)[0] for sw in SWITCHES} for name in CASES}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cases(eng):
    """each case's records on the device and its rows without a switch, computed once"""
    out = {}
    for name in CASES:
        case = load_case(eng, name)
        out[name] = (case, collect(eng, case, {}))
    return out


@pytest.mark.parametrize("switches", SWITCHES, ids=switch_id)
@pytest.mark.parametrize("name", CASES)
def test_step_launches_match_the_recorded_table(eng, golden, cases, name, switches):
    case, (base_launches, base_rows) = cases[name]
    launches, rows = (base_launches, base_rows) if not switches else collect(eng, case, switches)
    want = golden[name][switch_id(switches)]
    assert sorted(launches) == sorted(want)
    for run in want:
        print(name, switch_id(switches), run, launches[run])
        assert launches[run] == want[run], (run, launches[run], want[run])
        _same_rows(base_rows[run], rows[run])
