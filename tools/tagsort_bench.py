#!/usr/bin/env python
"""
Times the native TagSort device stage -- sct_tag_sort by (cell, umi, gene) then sct_tagsort_metrics --
on synth.py's config-5-shaped records (globally shuffled, 30 % NH > 1, 40 % duplicates, secondary
alignments) resident in HBM, and beside it, in the same process, the existing config-5 step in Welford
mode (the same sort with the query-name tiebreak, then cell rows with sequential Welford chains and
the grouped gene partials): the nearest thing the engine had before.  Steps alternate A, B, A, B ...

Prints one JSON line: per step kind the whole-step times (host clock around steps that end in a
device synchronise), their median and spread, and the per-kernel times of one profiled step (HIP events
inside the library, a pass of its own).  Needs a GPU; there is no CPU fallback.

    python tools/tagsort_bench.py [--records 100000000] [--cells 10000] [--steps 5] [--warmup 1]
                                  [--metric-type cell|gene] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--genes", type=int, default=30_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--metric-type", default="cell", choices=["cell", "gene"])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args(argv)

    import torch

    from sctools_amd import engine as E
    from sctools_amd import synth

    dev = E._device(None)
    torch.cuda.set_device(dev)
    eng = E.get_engine(dev)
    cfg = synth.SynthConfig(n_reads=a.records, n_cells=a.cells, n_genes=a.genes, seed=a.seed)
    cfg.p_nh1, cfg.p_dup, cfg.p_secondary = 0.70, 0.40, 0.10
    data = synth.generate(cfg, device=dev, chunk=16_000_000)
    g = torch.Generator(device=dev)
    g.manual_seed(a.seed + 1)
    perm = torch.randperm(a.records, generator=g, device=dev)
    cols = {c: t[perm].contiguous() for c, t in data.cols.items()}
    qname, n_qnames = data.extra["qname"][perm].contiguous(), data.extra["n_qnames"]
    del perm, data.cols
    dims = E.Dims(data.n_cell_ids, data.n_gene_ids, data.n_umi_ids)
    mito = torch.from_numpy(data.gene_is_mito).to(dev)
    multi = torch.from_numpy(data.gene_is_multi).to(dev)

    # TagSort: the roles in (first, second, third) position; the synthetic ids stand for the ranks
    if a.metric_type == "cell":
        ts_cols, ts_dims = cols, dims
        drop = torch.zeros(dims.n_cell_ids, dtype=torch.uint8, device=dev)
        if data.cell_has_none:
            drop[0] = 1
        third_mito = mito
    else:  # gene, barcode, umi
        ts_cols = dict(cols, cell=cols["gene"], umi=cols["cell"], gene=cols["umi"])
        ts_dims = E.Dims(dims.n_gene_ids, dims.n_umi_ids, dims.n_cell_ids)
        drop = multi.clone()
        drop[0] = 1  # gene id 0 is the missing tag
        third_mito = None
    state = {"cap": None, "rows": 0}

    def step_tagsort():
        s = eng.tag_sort(ts_cols, ts_dims, "cell_umi_gene")
        ints, sums = eng.tagsort_metrics(s, ts_dims, a.metric_type, drop, third_mito, capacity=state["cap"])
        state["cap"] = state["rows"] = int(ints.shape[0])
        return ints, sums

    n_ent = eng.count_entities(eng.tag_sort(cols, dims, "cell_umi_gene", qname, n_qnames), "cell", dims)
    partials = torch.empty((data.n_gene_ids, 64), dtype=torch.int64, device=dev)

    def step_welford():
        s = eng.tag_sort(cols, dims, "cell_umi_gene", qname, n_qnames)
        ci, cf = eng.compute(s, "cell", dims, mito, multi, float_mode="welford", n_entities=n_ent)
        eng.gene_partials(s, dims, out=partials)
        return eng.finalize_partials(partials)

    steps = {"tagsort": step_tagsort, "config5_welford": step_welford}
    for _ in range(max(1, a.warmup)):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    kernels = {}
    for name, fn in steps.items():  # per-kernel times: a pass of its own, events around every launch
        eng.profile_only("")
        eng.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        eng.profile_enable(False)
        kernels[name] = {k: {"ms": round(v[0], 4), "launches": v[1]} for k, v in
                         sorted(eng.profile_read_items().items(), key=lambda kv: -kv[1][0])}
    times = {name: [] for name in steps}
    for _ in range(a.steps):
        for name, fn in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    result = {
        "tool": "tools/tagsort_bench.py", "device": torch.cuda.get_device_name(dev), "records": a.records,
        "cells": a.cells, "genes": a.genes, "metric_type": a.metric_type, "steps": a.steps,
        "tagsort_rows": state["rows"], "config5_entities": int(n_ent),
        "step_ms": {k: [round(t, 3) for t in v] for k, v in times.items()},
        "median_ms": {k: round(statistics.median(v), 3) for k, v in times.items()},
        "spread_ms": {k: round(max(v) - min(v), 3) for k, v in times.items()},
        "records_per_s": {k: round(a.records / (statistics.median(v) * 1e-3)) for k, v in times.items()},
        "kernels_ms": kernels,
    }
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
