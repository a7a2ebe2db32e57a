"""
FastqMetrics on the GPU, timed: ``sct_fqm_accumulate`` (include/sct_fastq_metrics.h through ctypes) on
barcode columns resident in HBM, and ``FastqMetrics.compute`` end to end on a plain file.

    python tools/fastq_metrics_bench.py [--records 20000000] [--calls 10] [--e2e-records 2000000]
                                        [--host-yardstick] [--out FILE]

Kernel lines: synthetic ``16C10M`` columns of ``--records`` rows, drawn on the device.
  uniform   the cell barcode column, rows drawn evenly from 2^20 random 16-base barcodes
  hot       the same with 5 % of the rows replaced by one key, poly-G (what a NovaSeq writes for a
            read without signal)
  umi       the UMI column, 10 random bases (at most 4^10 = 2^20 keys)
Each is timed with device events in two states that a run goes through: ``first``, into a freshly
initialised table, where every key is claimed by a compare-and-swap, and ``again``, into the table
that holds the keys already, where a row costs one load and one atomic add.  The table has the size
the growth rule asks for.  One JSON line per column: milliseconds, rows/s, and the fraction of the
8 TB/s HBM peak by algorithmic bytes, which is the column read once (n * L); the table traffic is
the cost of the method, not of the problem, and is not counted.

``--host-yardstick``: ``np.unique(rows, return_counts=True)`` over the same columns on the host, the
counting a user without this package would do in numpy (one thread; it does not build the matrix).

End-to-end line (``--e2e-records`` > 0): a plain-text R1 file of 26-base reads with sequencer-style
names is written to a temporary directory and ``FastqMetrics(file, "16C10M").compute()`` is timed
with the host clock (it ends in device-to-host copies), twice; the file's reads repeat a block of
8192, so the tables stay small: the figure is the reading, copying and extraction, not the table.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sctools_amd import fastq_metrics  # noqa: E402
from sctools_amd._ffi import ptr, stream as current_stream  # noqa: E402

HBM_PEAK = 8.0e12
POOL = 1 << 20
HOT_FRACTION = 0.05


def columns(n, dev):
    """The three columns, uint8 [n, L] on the device, from a fixed seed."""
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    bases = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    pool = bases[torch.randint(0, 4, (POOL, 16), device=dev, generator=g)]
    uniform = pool[torch.randint(0, POOL, (n,), device=dev, generator=g)].contiguous()
    hot = uniform.clone()
    hot[torch.rand(n, device=dev, generator=g) < HOT_FRACTION] = ord("G")
    umi = bases[torch.randint(0, 4, (n, 10), device=dev, generator=g)].contiguous()
    return {"uniform": uniform, "hot": hot, "umi": umi}


def kernel_line(name, col, calls):
    lib = fastq_metrics.load()
    dev = col.device
    n, length = col.shape
    n_slots = fastq_metrics.next_slots(fastq_metrics.MIN_SLOTS, 0, n)
    table = torch.empty(16 * n_slots, dtype=torch.uint8, device=dev)
    pwm = torch.zeros((length, 6), dtype=torch.int64, device=dev)
    exceptions = torch.empty(n, dtype=torch.int64, device=dev)
    result = torch.zeros(4, dtype=torch.int64, device=dev)
    stream = current_stream(dev)

    def init():
        fastq_metrics.check(lib.sct_fqm_table_init(ptr(table), n_slots, table.numel(), stream))
        result.zero_()

    def accumulate():
        fastq_metrics.check(lib.sct_fqm_accumulate(ptr(col), n, length, ptr(table), n_slots, table.numel(), ptr(pwm),
                                                   ptr(exceptions), ptr(result), stream))

    def timed(before):
        ms = []
        for i in range(calls + 2):  # two warm-up calls
            before()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            accumulate()
            b.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms.append(a.elapsed_time(b))
        return {"mean": round(float(np.mean(ms)), 4), "min": round(float(np.min(ms)), 4), "max": round(float(np.max(ms)), 4)}

    first = timed(init)
    distinct, n_exceptions, _, error = (int(x) for x in result.cpu())
    again = timed(lambda: None)
    assert error == 0 and n_exceptions == 0 and int(result[0].cpu()) == distinct
    assert int(pwm.sum().cpu()) == 2 * (calls + 2) * n * length
    line = {"what": "sct_fqm_accumulate, column resident in HBM", "column": name, "rows": n, "L": length,
            "n_slots": n_slots, "table_bytes": 16 * n_slots, "distinct": distinct, "calls": calls,
            "ms_first": first, "ms_again": again,
            "rows_per_s_first": round(n / (first["mean"] * 1e-3)), "rows_per_s_again": round(n / (again["mean"] * 1e-3)),
            "algorithmic_bytes": n * length, "ms_at_hbm_peak": round(n * length / HBM_PEAK * 1e3, 4),
            "hbm_fraction_first": round(n * length / (first["mean"] * 1e-3) / HBM_PEAK, 5),
            "hbm_fraction_again": round(n * length / (again["mean"] * 1e-3) / HBM_PEAK, 5)}
    return line, distinct


def host_line(name, col, distinct):
    rows = col.cpu().numpy()
    t0 = time.perf_counter()
    keys, counts = np.unique(rows.view("S%d" % rows.shape[1]).ravel(), return_counts=True)
    seconds = time.perf_counter() - t0
    assert len(keys) == distinct and int(counts.sum()) == len(rows)
    return {"what": "host yardstick: np.unique(rows, return_counts=True), one thread, counts only", "column": name,
            "rows": len(rows), "distinct": len(keys), "seconds": round(seconds, 3), "rows_per_s": round(len(rows) / seconds)}


def r1_block(n, rng):
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for _ in range(n):
        name = b"@A00123:45:HXXXXXXXX:1:%d:%d:%d 1:N:0:ACGTACGT" % (rng.integers(1101, 2679), rng.integers(1000, 33000),
                                                                  rng.integers(1000, 37000))
        out.append(name + b"\n" + bytes(bases[rng.integers(0, 4, 26)]) + b"\n+\n" + bytes(rng.integers(35, 75, 26).astype(np.uint8))
                   + b"\n")
    return b"".join(out)


def e2e_line(n_records):
    rng = np.random.default_rng(5)
    block = r1_block(8192, rng)
    reps = max(1, n_records // 8192)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "R1.fastq")
        with open(path, "wb") as f:
            for _ in range(reps):
                f.write(block)
        seconds = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = fastq_metrics.FastqMetrics(path, "16C10M").compute()
            seconds.append(round(time.perf_counter() - t0, 3))
        assert result.n_records == reps * 8192 and result.n_host_rows == 0
        assert int(result.barcode_counts.sum()) == result.n_records and result.barcode_counts.min() >= reps
        return {"what": "FastqMetrics(plain R1 file, 16C10M).compute(), host clock, two runs; reads repeat a block of 8192",
                "records": result.n_records, "text_bytes": reps * len(block), "seconds": seconds,
                "records_per_s": round(result.n_records / seconds[1]), "distinct_barcodes": len(result.barcode_counts),
                "distinct_umis": len(result.umi_counts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20_000_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--e2e-records", type=int, default=2_000_000)
    ap.add_argument("--host-yardstick", action="store_true", help="also time np.unique on the same columns on the host")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("fastq_metrics_bench needs a ROCm GPU; a CPU run gives no timing")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    def emit(line):
        text = json.dumps(line, sort_keys=True)
        print(text, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")

    for name, col in columns(args.records, dev).items():
        line, distinct = kernel_line(name, col, args.calls)
        emit(line)
        if args.host_yardstick:
            emit(host_line(name, col, distinct))
    if args.e2e_records > 0:
        emit(e2e_line(args.e2e_records))


if __name__ == "__main__":
    main()
