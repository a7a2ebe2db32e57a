"""
FastqProcess on the GPU, timed: the sct_fqp_* kernels one at a time on a synthetic 10x triple
resident in HBM (include/sct_fastq_process.h through ctypes), and a FastqProcess run end to end
split into phases, beside Attach10xBarcodes on input of the same size.

    python tools/fastq_process_bench.py [--records 2000000] [--calls 10] [--e2e-records 500000] [--out FILE]

Kernel lines: R1 as tools/fastq_bench.py makes it (26 bases), R2 with the same names and 98 bases,
I1 with 8.  Every call is timed with device events after a warm-up.  One JSON line per call:
milliseconds, records/s, the algorithmic bytes (what the call must read and write once) and their
fraction of the 8 TB/s HBM peak.

End-to-end line (``--e2e-records`` > 0): the triple as .fastq.gz in a temporary directory, then
``FastqProcess --white-list`` to ``--shards`` BAM shards with the phases timed on the host from
outside the library (its functions are wrapped here for the run): read (gunzip into the pinned
windows), H2D + kernels (count, extract, lines, shard, plan, emit, synchronized), correction, D2H
of the records, deflate (the native shard writer).  Then tools/fastq_bench.py's Attach10xBarcodes
line on the same number of records, in the same process.
"""
import argparse
import ctypes
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fastq_bench  # noqa: E402
from sctools_amd import bamnative, barcode, fastq, fastq_process as fp  # noqa: E402
from sctools_amd._ffi import ptr, stream as current_stream  # noqa: E402

HBM_PEAK = 8.0e12
READ = 98


def triple_blocks(n, rng, whitelist=None):
    """n records of R1, R2 and I1 as lists of bytes, the three with the same names."""
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    r1 = fastq_bench.r1_block(n, rng, whitelist)
    r2, i1 = [], []
    for rec in r1:
        name = rec.split(b" ")[0]
        seq = bytes(bases[rng.integers(0, 4, READ)])
        qual = bytes(rng.integers(35, 75, READ).astype(np.uint8))
        r2.append(name + b" 2:N:0:ACGTACGT\n" + seq + b"\n+\n" + qual + b"\n")
        i1.append(name + b" 1:N:0:ACGTACGT\n" + bytes(bases[rng.integers(0, 4, 8)]) + b"\n+\nFFFFFFFF\n")
    return r1, r2, i1


def resident(block, reps, dev):
    text = torch.from_numpy(np.frombuffer(b"".join(block), dtype=np.uint8).copy()).to(dev).repeat(reps)
    lib = fastq.load()
    nbytes = ctypes.c_size_t(0)
    fastq.check(lib.sct_fq_workspace_size(int(text.numel()), ctypes.byref(nbytes)))
    work = torch.empty(nbytes.value + 8, dtype=torch.uint8, device=dev)
    result = torch.empty(4, dtype=torch.int64, device=dev)
    fastq.check(lib.sct_fq_count(ptr(text), int(text.numel()), 1, ptr(work), work.numel(), ptr(result), current_stream(dev)))
    n = int(result[0].cpu())
    return fastq.Window(text, int(text.numel()), n, work, None)


def line(what, n, ms, algorithmic, **more):
    mean, lo, hi = ms
    out = {"what": what, "records": n, "ms": {"mean": round(mean, 4), "min": round(lo, 4), "max": round(hi, 4)},
           "records_per_s": round(n / (mean * 1e-3)), "algorithmic_bytes": int(algorithmic),
           "ms_at_hbm_peak": round(algorithmic / HBM_PEAK * 1e3, 4),
           "hbm_fraction": round(algorithmic / (mean * 1e-3) / HBM_PEAK, 4)}
    out.update(more)
    return out


def kernel_lines(n_records, calls, n_shards, whitelist_file):
    lib = fp.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    whitelist = [ln[:-1].encode() for ln in open(whitelist_file) if set(ln[:-1]) <= set("ACGT")]
    r1, r2, i1 = triple_blocks(4096, rng, whitelist)
    reps = max(1, n_records // 4096)
    w1, w2, wi = (resident(b, reps, dev) for b in (r1, r2, i1))
    n = w2.n_records
    assert w1.n_records == n == wi.n_records == reps * 4096
    stream = current_stream(dev)
    cols, flagged, _ = fastq.extract_spans(w1, [(0, 16), (16, 26)])
    assert flagged == -1
    (cr, cy), (ur, uy) = cols
    corrector = barcode.ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(whitelist_file, device=dev)
    index, cb = corrector.correct_barcodes(cr, return_corrected=True)
    out = []

    off = torch.empty((n, 3), dtype=torch.int64, device=dev)
    length = torch.empty((n, 3), dtype=torch.int32, device=dev)
    flags = torch.empty((n + 3) // 4 * 4, dtype=torch.uint8, device=dev)
    result = torch.empty(4, dtype=torch.int64, device=dev)

    def lines():
        fp.check(lib.sct_fqp_lines(ptr(w2.text), w2.n_bytes, n, ptr(w2.workspace), w2.workspace.numel(), ptr(off),
                                   ptr(length), ptr(flags), ptr(result), stream))

    ms = fastq_bench.timed(lines, calls)
    assert int(result[3].cpu()) == -1
    out.append(line("sct_fqp_lines on the R2 text (after sct_fq_count)", n, ms, w2.n_bytes + 37 * n,
                    text_bytes=w2.n_bytes, bytes_per_record=round(w2.n_bytes / n, 2)))
    off1, len1, flagged1, _ = fp.window_lines(wi)
    assert flagged1 == -1

    shard = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)

    def shard_call():
        fp.check(lib.sct_fqp_shard(ptr(cr), ptr(cb), ptr(index), n, 16, n_shards, ptr(shard), ptr(counts), stream))

    ms = fastq_bench.timed(shard_call, calls)
    out.append(line("sct_fqp_shard, L 16, %d shards" % n_shards, n, ms, n * (16 + 16 + 4 + 4),
                    counts=[int(x) for x in counts.cpu()]))

    for fmt, name in ((fp.BAM, "BAM"), (fp.FASTQ, "FASTQ")):
        batch = fp.Batch(w2.text, w2.n_bytes, off, length, cr, cy, ur, uy, shard, n_shards, fmt,
                         i1=(wi.text, wi.n_bytes, off1, len1) if fmt == fp.BAM else None,
                         cb=cb if fmt == fp.BAM else None, cb_index=index if fmt == fp.BAM else None)
        k = batch.outputs
        nbytes = ctypes.c_size_t(0)
        fp.check(lib.sct_fqp_plan_workspace_size(n, n_shards, fmt, ctypes.byref(nbytes)))
        work = torch.empty(nbytes.value + 8, dtype=torch.uint8, device=dev)
        offsets = torch.empty((k, n), dtype=torch.int64, device=dev)
        shard_counts = torch.empty(n_shards, dtype=torch.int64, device=dev)
        shard_bytes = torch.empty((k, n_shards), dtype=torch.int64, device=dev)

        def plan():
            fp.check(lib.sct_fqp_plan(ctypes.byref(batch.c), ptr(work), work.numel(), ptr(offsets), ptr(shard_counts),
                                      ptr(shard_bytes), stream))

        ms = fastq_bench.timed(plan, calls)
        per_record = 2 * (12 + 4 + (4 + 12 if fmt == fp.BAM else 0)) + 8 * k
        out.append(line("sct_fqp_plan, %s, %d shards" % (name, n_shards), n, ms,
                        n * per_record + 2 * int(nbytes.value), workspace_bytes=int(nbytes.value)))
        sizes = shard_bytes.reshape(-1).cpu().numpy()
        bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        total, total1 = int(bounds[-1]), int(bounds[n_shards])
        base = torch.from_numpy(bounds[:-1].copy())
        if k == 2:
            base[n_shards:] -= total1
        base = base.to(dev)
        buf = torch.empty(total, dtype=torch.uint8, device=dev)
        error = torch.empty(1, dtype=torch.int64, device=dev)
        if fmt == fp.BAM:
            def emit():
                fp.check(lib.sct_fqp_emit_bam(ctypes.byref(batch.c), ptr(offsets), ptr(base), ptr(buf), total, ptr(error), stream))
        else:
            def emit():
                fp.check(lib.sct_fqp_emit_fastq(ctypes.byref(batch.c), ptr(offsets), ptr(base), ptr(buf), total1,
                                                ctypes.c_void_p(buf.data_ptr() + total1), total - total1, ptr(error), stream))
        ms = fastq_bench.timed(emit, calls)
        assert int(error.cpu()) == 0
        lens = length.sum(dim=0).cpu().tolist()
        read = sum(lens) + n * (2 * 16 + 2 * 10) + n * (36 + 4 + 8)  # the lines, the columns, offsets/lengths/shard/offset
        if fmt == fp.BAM:
            read += int(len1[:, 1:].sum().cpu()) + n * (16 + 4 + 36)
        out.append(line("sct_fqp_emit_%s, %d shards" % (name.lower(), n_shards), n, ms, read + total,
                        output_bytes=total, output_bytes_per_record=round(total / n, 2)))
    return out


class Phases(fastq_bench.Phases):
    def __enter__(self):
        lib = fastq.load()
        self.wrap(fastq._ByteStream, "readinto", "read")
        self.wrap(fastq._Inflater, "run", "stage_h2d_inflate_crc", sync=True)
        for name in ("sct_fq_count", "sct_fq_extract", "sct_fqp_lines", "sct_fqp_shard", "sct_fqp_plan", "sct_fqp_emit_bam",
                     "sct_fqp_emit_fastq"):
            self.wrap(lib, name, "h2d_kernels", sync=True)
        self.wrap(barcode.ErrorsToCorrectBarcodesMap, "correct_barcodes", "correct", sync=True)
        self.wrap(fp, "to_host", "d2h")
        self.wrap(bamnative.ShardWriter, "append", "deflate")
        self.wrap(bamnative.ShardWriter, "close", "deflate")
        return self


def e2e_line(n_records, n_shards, whitelist_file):
    rng = np.random.default_rng(5)
    whitelist = [ln[:-1].encode() for ln in open(whitelist_file) if set(ln[:-1]) <= set("ACGT")]
    with tempfile.TemporaryDirectory() as tmp:
        blocks = triple_blocks(8192, rng, whitelist)
        reps = max(1, n_records // 8192)
        n = reps * 8192
        paths, sizes = [], {}
        for kind, block in zip(("R1", "R2", "I1"), blocks):
            paths.append(os.path.join(tmp, kind + ".fastq.gz"))
            with gzip.open(paths[-1], "wb", compresslevel=4) as f:
                for _ in range(reps):
                    f.write(b"".join(block))
            sizes[kind.lower() + "_gz_bytes"] = os.path.getsize(paths[-1])
            sizes[kind.lower() + "_text_bytes"] = reps * len(b"".join(block))
        out = os.path.join(tmp, "out")
        os.mkdir(out)
        job = fp.FastqProcess([paths[0]], [paths[1]], [paths[2]], whitelist=whitelist_file, barcode_length=16, umi_length=10,
                              sample_id="bench", num_shards=n_shards, output_dir=out)
        torch.cuda.synchronize()
        with Phases() as phases:
            t0 = time.perf_counter()
            result = job.run()
            total = time.perf_counter() - t0
        timings = {k: round(v, 3) for k, v in phases.seconds.items()}
        assert result.n_reads == n
        return {"what": "FastqProcess --white-list end to end, BAM shards", "records": n, "shards": n_shards, **sizes,
                "total_s": round(total, 3), "records_per_s": round(n / total), "phases_s": timings,
                "other_s": round(total - sum(timings.values()), 3),
                "output_bytes": sum(os.path.getsize(p) for p in result.paths),
                "counts": [result.n_correct, result.n_corrected, result.n_uncorrectable],
                "phase_key": {"read": "gunzip into the pinned windows of R1, R2 and I1",
                              "h2d_kernels": "copy to the GPU + count, extract, lines, shard, plan, emit; synchronized",
                              "correct": "sct_bc_correct", "d2h": "the emitted records to the host",
                              "deflate": "native shard writer: BGZF deflate and file writes",
                              "other_s": "Python glue, allocation, the small reads of counts and sizes"}}


def bgzf_line(n_records, n_shards, whitelist_file, runs, modes=("host", "auto")):
    """FastqProcess on BGZF-compressed copies of the triple, ``inflate="host"`` and ``"auto"`` in turn in one process."""
    rng = np.random.default_rng(5)
    whitelist = [ln[:-1].encode() for ln in open(whitelist_file) if set(ln[:-1]) <= set("ACGT")]
    with tempfile.TemporaryDirectory() as tmp:
        blocks = triple_blocks(8192, rng, whitelist)
        reps = max(1, n_records // 8192)
        n = reps * 8192
        paths, sizes = [], {}
        for kind, block in zip(("R1", "R2", "I1"), blocks):
            paths.append(os.path.join(tmp, kind + ".fastq.gz"))
            fastq_bench.write_fastq(paths[-1], b"".join(block), reps, bgzf=True)
            sizes[kind.lower() + "_gz_bytes"] = os.path.getsize(paths[-1])
            sizes[kind.lower() + "_text_bytes"] = reps * len(b"".join(block))
        who, counts = {}, {}

        def run(mode):
            out = os.path.join(tmp, "out_" + mode)
            os.makedirs(out, exist_ok=True)
            job = fp.FastqProcess([paths[0]], [paths[1]], [paths[2]], whitelist=whitelist_file, barcode_length=16,
                                  umi_length=10, sample_id="bench", num_shards=n_shards, output_dir=out, inflate=mode)
            torch.cuda.synchronize()
            with Phases() as phases:
                t0 = time.perf_counter()
                result = job.run()
                total = time.perf_counter() - t0
            assert result.n_reads == n and not job.declined
            who[mode] = sorted(set(job.inflated_by.values()))
            counts[mode] = [result.n_correct, result.n_corrected, result.n_uncorrectable, result.shard_counts]
            return total, {k: round(v, 3) for k, v in phases.seconds.items()}

        out = fastq_bench.alternate(run, modes, runs)
        assert all(counts[m] == counts[modes[0]] for m in modes)
        return {"what": "FastqProcess --white-list end to end on BGZF FASTQ, BAM shards, --inflate host and auto in turn",
                "records": n, "shards": n_shards, "runs": runs, **sizes, "inflated_by": who, **out,
                "phase_key": {"read": "host gunzip into the pinned windows (inflate=host)",
                              "stage_h2d_inflate_crc": "mapped file -> pinned buffer -> GPU, k_inflate, k_fq_crc32; synchronized",
                              "h2d_kernels": "copy to the GPU (host path) + count, extract, lines, shard, plan, emit; synchronized",
                              "correct": "sct_bc_correct", "d2h": "the emitted records to the host",
                              "deflate": "native shard writer: BGZF deflate and file writes"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2_000_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--shards", type=int, default=16)
    ap.add_argument("--e2e-records", type=int, default=500_000)
    ap.add_argument("--whitelist", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                        "tests", "golden", "barcode", "1k-august-2016.txt"))
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--bgzf", action="store_true", help="instead: FastqProcess on BGZF-compressed copies of the triple, "
                    "the --inflate modes in turn (DESIGN.md section 19)")
    ap.add_argument("--inflate", default="both", choices=["both", "auto", "host"], help="with --bgzf: the mode(s) to run")
    ap.add_argument("--runs", type=int, default=5, help="with --bgzf: timed runs per mode, after one warm-up of each")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("fastq_process_bench needs a ROCm GPU; a CPU run gives no timing")
    torch.cuda.set_device(0)
    if args.bgzf:
        modes = ("host", "auto") if args.inflate == "both" else (args.inflate,)
        lines = [bgzf_line(args.e2e_records, args.shards, args.whitelist, args.runs, modes)]
    else:
        lines = kernel_lines(args.records, args.calls, args.shards, args.whitelist)
    if args.e2e_records > 0 and not args.bgzf:
        lines.append(e2e_line(args.e2e_records, args.shards, args.whitelist))
        lines.append(fastq_bench.e2e_line(args.e2e_records, args.whitelist))
    for entry in lines:
        text = json.dumps(entry, sort_keys=True)
        print(text, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
