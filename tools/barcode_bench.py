"""
Barcode correction and pair statistics on the GPU, timed (include/sct_barcode.h through ctypes).

    python tools/barcode_bench.py [--whitelist 737280] [--queries 100000000] [--calls 20] [--out FILE]

A random 16-base whitelist and the queries are generated on the device from a seed and stay resident
in HBM.  Two query mixes:

  realistic    92 % on the list, 6 % one substitution away, 2 % random 16-mers (no correction)
  adversarial  100 % one substitution away: every lane takes the neighbour search

One JSON line per mix: milliseconds per sct_bc_correct call from device events (after a warm-up,
over --calls calls, index only and with the corrected bytes), queries per second, the fraction of
the 8 TB/s HBM peak by algorithmic bytes (16 B read + 4 B index, + 16 B corrected, per query),
the table build time and the all-pairs histogram time over the whole whitelist.

The last line times, on the host, a plain Python dict holding the reference's error map of a
10,000-entry whitelist over 1,000,000 lookups: the per-lookup cost the reference's per-record
loop (barcode.py:371-378) cannot go below.  It is a floor for that loop, not a measurement of it.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sctools_amd import barcode  # noqa: E402
from sctools_amd._ffi import ptr, stream as current_stream  # noqa: E402

L = 16
HBM_PEAK = 8.0e12


def decode(codes):
    """[n] int64 codes -> [n, 16] uint8 ASCII"""
    shifts = torch.arange(2 * (L - 1), -1, -2, device=codes.device, dtype=torch.int64)
    lut = torch.tensor(list(b"ACTG"), dtype=torch.uint8, device=codes.device)
    return lut[(codes[:, None] >> shifts[None, :]) & 3]


def make_queries(wl_codes, n, p_error, p_random, gen, chunk=10_000_000):
    out = torch.empty((n, L), dtype=torch.uint8, device=wl_codes.device)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        codes = wl_codes[torch.randint(0, wl_codes.numel(), (m,), device=wl_codes.device, generator=gen)]
        u = torch.rand(m, device=wl_codes.device, generator=gen)
        pos = torch.randint(0, L, (m,), device=wl_codes.device, generator=gen)
        flip = torch.randint(1, 4, (m,), device=wl_codes.device, generator=gen)
        codes = torch.where(u < p_error, codes ^ (flip << (2 * pos)), codes)
        rnd = torch.randint(0, 1 << (2 * L), (m,), device=wl_codes.device, generator=gen)
        codes = torch.where(u >= 1.0 - p_random, rnd, codes)
        out[lo:lo + m] = decode(codes)
    return out


def timed(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in events:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in events]
    return float(np.mean(ms)), float(np.min(ms)), float(np.max(ms))


def host_dict_floor(n_whitelist=10_000, n_lookups=1_000_000):
    rng = np.random.default_rng(1)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    lines = [bytes(r).decode() for r in bases[rng.integers(0, 4, size=(n_whitelist, L))]]
    t0 = time.perf_counter()
    error_map = {}
    for w in lines:
        error_map[w] = w
        for pos in range(L):
            for e in "ACGTN":
                if e != w[pos]:
                    error_map[w[:pos] + e + w[pos + 1:]] = w
    build_s = time.perf_counter() - t0
    keys = list(error_map)
    queries = [keys[k] for k in rng.integers(0, len(keys), size=n_lookups)]
    t0 = time.perf_counter()
    hits = 0
    for q in queries:
        try:
            error_map[q]
            hits += 1
        except KeyError:
            pass
    lookup_s = time.perf_counter() - t0
    return {"what": "host Python dict of the same map: a floor for the reference's per-record loop, not a run of it",
            "whitelist": n_whitelist, "dict_entries": len(error_map), "dict_build_s": round(build_s, 3),
            "lookups": n_lookups, "ns_per_lookup": round(lookup_s / n_lookups * 1e9, 1),
            "lookups_per_s": round(n_lookups / lookup_s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--whitelist", type=int, default=737_280)
    ap.add_argument("--queries", type=int, default=100_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--pair-calls", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("barcode_bench needs a ROCm GPU; a CPU run gives no timing")
    lib = barcode.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    stream = current_stream(dev)

    wl = torch.unique(torch.randint(0, 1 << (2 * L), (args.whitelist * 2,), device=dev, generator=gen))
    wl = wl[torch.randperm(wl.numel(), device=dev, generator=gen)[:args.whitelist]].contiguous()
    n_wl = int(wl.numel())
    nbytes = ctypes.c_size_t(0)
    barcode.check(lib.sct_bc_table_size(n_wl, ctypes.byref(nbytes)))
    table = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    build_ms = timed(lambda: barcode.check(lib.sct_bc_table_build(ptr(wl), n_wl, L, ptr(table), nbytes.value, stream)),
                     calls=5, warmup=1)
    hist = torch.empty(barcode.HIST_BINS, dtype=torch.int64, device=dev)
    pair_ms = timed(lambda: barcode.check(lib.sct_bc_pair_hist(ptr(wl), n_wl, L, ptr(hist), stream)),
                    calls=args.pair_calls, warmup=1)
    pairs = n_wl * (n_wl - 1) // 2
    assert int(hist.sum()) == pairs

    n = args.queries
    index = torch.empty(n, dtype=torch.int32, device=dev)
    corrected = torch.empty((n, L), dtype=torch.uint8, device=dev)
    lines = []
    for mix, p_error, p_random in (("realistic", 0.06, 0.02), ("adversarial", 1.0, 0.0)):
        raw = make_queries(wl, n, p_error, p_random, gen)
        idx_ms = timed(lambda: barcode.check(lib.sct_bc_correct(ptr(table), n_wl, ptr(raw), n, L, ptr(index), None, stream)),
                       calls=args.calls)
        cor_ms = timed(lambda: barcode.check(lib.sct_bc_correct(ptr(table), n_wl, ptr(raw), n, L, ptr(index), ptr(corrected),
                                                                stream)), calls=args.calls)
        lines.append({
            "mix": mix, "whitelist": n_wl, "queries": n, "barcode_length": L, "table_bytes": nbytes.value,
            "fraction_uncorrected": round(float((index < 0).float().mean()), 5),
            "ms_per_call_index_only": {"mean": round(idx_ms[0], 4), "min": round(idx_ms[1], 4), "max": round(idx_ms[2], 4)},
            "ms_per_call_with_corrected": {"mean": round(cor_ms[0], 4), "min": round(cor_ms[1], 4),
                                           "max": round(cor_ms[2], 4)},
            "calls": args.calls,
            "queries_per_s": round(n / (idx_ms[0] * 1e-3)),
            "queries_per_s_with_corrected": round(n / (cor_ms[0] * 1e-3)),
            "hbm_fraction_index_only": round(20.0 * n / (idx_ms[0] * 1e-3) / HBM_PEAK, 4),
            "hbm_fraction_with_corrected": round(36.0 * n / (cor_ms[0] * 1e-3) / HBM_PEAK, 4),
            "table_build_ms": round(build_ms[0], 4),
            "pair_hist_ms": round(pair_ms[0], 3), "pair_hist_pairs": pairs,
            "pair_hist_pairs_per_s": round(pairs / (pair_ms[0] * 1e-3)),
        })
        del raw
    lines.append(host_dict_floor())
    for line in lines:
        text = json.dumps(line, sort_keys=True)
        print(text, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
