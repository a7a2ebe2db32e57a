"""
FASTQ text -> barcode columns on the GPU, timed (include/sct_fastq.h through ctypes), and an
Attach10xBarcodes run end to end split into phases.

    python tools/fastq_bench.py [--records 20000000] [--calls 20] [--e2e-records 1000000] [--out FILE]

Kernel line: synthetic 10x R1 text (26-base reads, Illumina-style names of 41..50 bytes) resident in
HBM.  ``sct_fq_count`` + ``sct_fq_extract`` with the 10x spans (0,16) and (16,26) are timed with
device events after a warm-up.  One JSON line: milliseconds per window, records/s, and the
fraction of the 8 TB/s HBM peak by algorithmic bytes: the text read twice (the two passes) plus the
four columns (2 x 26 bytes per record) and one flag byte written.

End-to-end line (``--e2e-records`` > 0): a synthetic R1.fastq.gz, I1.fastq.gz and unaligned BAM are
written to a temporary directory, then ``Attach10xBarcodes --whitelist`` runs on them with the
phases timed on the host from outside the library (its functions are wrapped here for the run):
read (gunzip into the pinned window), H2D + kernels (the kernels wait on the stream for the copy in
front of them, so the two are one figure), correction, BAM write (record rebuild, BGZF deflate).
The same files then go through the host-iterator path of this package -- OUR PORT of the
reference's per-record loop feeding the same native writer, not the reference itself (pysam is not
installed) -- for the loop the device path replaces.
"""
import argparse
import ctypes
import gzip
import json
import os
import struct
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sctools_amd import bam, bamnative, barcode, fastq, platform  # noqa: E402
from sctools_amd._ffi import ptr, stream as current_stream  # noqa: E402

HBM_PEAK = 8.0e12
SPANS = [(0, 16), (16, 26)]


def r1_block(n, rng, whitelist=None):
    """n 10x R1 records as bytes: names as a sequencer writes them, 26 bases, 26 qualities."""
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for r in range(n):
        name = b"@A00123:45:HXXXXXXXX:1:%d:%d:%d 1:N:0:ACGTACGT" % (rng.integers(1101, 2679), rng.integers(1000, 33000),
                                                                  rng.integers(1000, 37000))
        if whitelist is not None and rng.random() < 0.9:
            cell = whitelist[rng.integers(0, len(whitelist))]
        else:
            cell = bytes(bases[rng.integers(0, 4, 16)])
        seq = cell + bytes(bases[rng.integers(0, 4, 10)])
        qual = bytes(rng.integers(35, 75, 26).astype(np.uint8))
        out.append(name + b"\n" + seq + b"\n+\n" + qual + b"\n")
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


def kernel_line(n_records, calls):
    lib = fastq.load()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(11)
    block = r1_block(4096, rng)
    block_text = torch.from_numpy(np.frombuffer(b"".join(block), dtype=np.uint8).copy()).to(dev)
    reps = max(1, n_records // len(block))
    text = block_text.repeat(reps)
    n, n_bytes = reps * len(block), int(text.numel())
    nbytes = ctypes.c_size_t(0)
    fastq.check(lib.sct_fq_workspace_size(n_bytes, ctypes.byref(nbytes)))
    work = torch.empty(nbytes.value + 8, dtype=torch.uint8, device=dev)
    result = torch.empty(4, dtype=torch.int64, device=dev)
    seq = [torch.empty((n, e - s), dtype=torch.uint8, device=dev) for s, e in SPANS]
    qual = [torch.empty((n, e - s), dtype=torch.uint8, device=dev) for s, e in SPANS]
    flags = torch.empty((n + 3) // 4 * 4, dtype=torch.uint8, device=dev)
    c_spans = (fastq.Span * 2)(*[fastq.Span(s, e) for s, e in SPANS])
    c_seq = (ctypes.c_void_p * 2)(*[t.data_ptr() for t in seq])
    c_qual = (ctypes.c_void_p * 2)(*[t.data_ptr() for t in qual])
    stream = current_stream(dev)

    def count():
        fastq.check(lib.sct_fq_count(ptr(text), n_bytes, 1, ptr(work), work.numel(), ptr(result), stream))

    def extract():
        fastq.check(lib.sct_fq_extract(ptr(text), n_bytes, n, ptr(work), work.numel(), c_spans, 2, c_seq, c_qual,
                                       ptr(flags), ptr(result), stream))

    def both():
        count()
        extract()

    count_ms, extract_ms, both_ms = timed(count, calls), timed(extract, calls), timed(both, calls)
    got = [int(x) for x in result.cpu()]
    assert got == [n, n_bytes, 4 * n, -1], got
    assert bytes(seq[0][n - 1].cpu().numpy()) == block[-1].split(b"\n")[1][:16]
    algorithmic = 2 * n_bytes + n * (2 * 26 + 1)
    return {"what": "sct_fq_count + sct_fq_extract, 10x spans, text resident in HBM", "records": n, "text_bytes": n_bytes,
            "bytes_per_record": round(n_bytes / n, 2), "tiles": -(-n_bytes // fastq.TILE_BYTES), "calls": calls,
            "ms_count": {"mean": round(count_ms[0], 4), "min": round(count_ms[1], 4), "max": round(count_ms[2], 4)},
            "ms_extract": {"mean": round(extract_ms[0], 4), "min": round(extract_ms[1], 4), "max": round(extract_ms[2], 4)},
            "ms_count_and_extract": {"mean": round(both_ms[0], 4), "min": round(both_ms[1], 4), "max": round(both_ms[2], 4)},
            "records_per_s": round(n / (both_ms[0] * 1e-3)), "text_bytes_per_s": round(n_bytes / (both_ms[0] * 1e-3)),
            "algorithmic_bytes": algorithmic, "hbm_fraction": round(algorithmic / (both_ms[0] * 1e-3) / HBM_PEAK, 4)}


class Phases:
    """Wraps library functions for one run and adds up the seconds spent in each, by phase."""

    def __init__(self):
        self.seconds = {}
        self._undo = []

    def wrap(self, owner, name, phase, sync=False):
        inner = getattr(owner, name)

        def timed_call(*args, **kwargs):
            t0 = time.perf_counter()
            try:
                return inner(*args, **kwargs)
            finally:
                if sync:
                    torch.cuda.synchronize()
                self.seconds[phase] = self.seconds.get(phase, 0.0) + time.perf_counter() - t0

        had = name in vars(owner)
        self._undo.append((owner, name, inner, had))
        setattr(owner, name, timed_call)

    def __enter__(self):
        lib = fastq.load()
        self.wrap(fastq._ByteStream, "readinto", "read")
        self.wrap(fastq._Inflater, "run", "stage_h2d_inflate_crc", sync=True)
        self.wrap(lib, "sct_fq_count", "h2d_kernels", sync=True)
        self.wrap(lib, "sct_fq_extract", "h2d_kernels", sync=True)
        self.wrap(barcode.ErrorsToCorrectBarcodesMap, "correct_barcodes", "correct", sync=True)
        self.wrap(bamnative.TagAttacher, "write", "write")
        return self

    def __exit__(self, *exc):
        for owner, name, inner, had in reversed(self._undo):
            if had:
                setattr(owner, name, inner)
            else:
                delattr(owner, name)


def write_fastq(path, block: bytes, reps: int, bgzf: bool, level: int = 4):
    """``block`` ``reps`` times as a FASTQ file: Python gzip (one stream), or with ``bgzf`` members of 0xff00 bytes
    and the EOF member, as bgzip and this project's shard writer lay them out."""
    if not bgzf:
        with gzip.open(path, "wb", compresslevel=level) as f:
            for _ in range(reps):
                f.write(block)
        return
    with open(path, "wb") as f:
        buf = bytearray()

        def flush(final=False):
            while len(buf) >= 0xff00 or (final and buf):
                chunk = bytes(buf[:0xff00])
                del buf[:0xff00]
                z = zlib.compressobj(level, zlib.DEFLATED, -15)
                data = z.compress(chunk) + z.flush()
                f.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(data) + 25) + data
                        + struct.pack("<II", zlib.crc32(chunk), len(chunk)))

        for _ in range(reps):
            buf += block
            flush()
        flush(final=True)
        f.write(bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]))


def alternate(run, modes, runs):
    """``run(mode)`` -> (seconds, phases): one warm-up of every mode, then ``runs`` of each in turn.  Per mode the
    totals, their median and spread (max - min), and the phases of the median run."""
    for mode in modes:
        run(mode)
    seen = {mode: [] for mode in modes}
    for _ in range(runs):
        for mode in modes:
            seen[mode].append(run(mode))
    out = {}
    for mode, results in seen.items():
        totals = sorted(t for t, _ in results)
        median = totals[len(totals) // 2]
        phases = next(ph for t, ph in results if t == median)
        out[mode] = {"total_s": [round(t, 3) for t, _ in results], "median_s": round(median, 3),
                     "spread_s": round(totals[-1] - totals[0], 3), "phases_of_median_s": phases}
    return out


def write_unaligned_bam(path, n, rng):
    """n unaligned 98-base records (flag 77 pattern of FastqToSam: unpaired, unmapped) as BGZF, level 1."""
    header = b"BAM\1" + struct.pack("<i", 0) + struct.pack("<i", 0)
    seq = bytes(rng.integers(0, 256, 49).astype(np.uint8) & 0x77 | 0x11)  # packed bases, 98 of them
    qual = bytes(rng.integers(2, 41, 98).astype(np.uint8))
    tail = struct.pack("<HHiiii", 0, 4, 98, -1, -1, 0)  # n_cigar_op, flag, l_seq, next_refID, next_pos, tlen
    with open(path, "wb") as f:
        buf = bytearray(header)

        def flush(final=False):
            while len(buf) >= 0xff00 or (final and buf):
                chunk = bytes(buf[:0xff00])
                del buf[:0xff00]
                z = zlib.compressobj(1, zlib.DEFLATED, -15)
                data = z.compress(chunk) + z.flush()
                f.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(data) + 25) + data
                        + struct.pack("<II", zlib.crc32(chunk), len(chunk)))

        for r in range(n):
            name = b"read%09d\0" % r
            core = struct.pack("<iiBBH", -1, -1, len(name), 0, 4680) + tail + name + seq + qual + b"RGZA\0"
            buf += struct.pack("<i", len(core)) + core
            if len(buf) >= 1 << 20:
                flush()
        flush(final=True)
        f.write(bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]))


def bgzf_line(n_records, whitelist_file, runs, modes=("host", "auto")):
    """Attach10xBarcodes on BGZF-compressed R1 / I1, ``inflate="host"`` and ``"auto"`` in turn in one process."""
    rng = np.random.default_rng(5)
    whitelist = [ln[:-1].encode() for ln in open(whitelist_file) if set(ln[:-1]) <= set("ACGT")]
    with tempfile.TemporaryDirectory() as tmp:
        r1, i1, u2 = os.path.join(tmp, "R1.fastq.gz"), os.path.join(tmp, "I1.fastq.gz"), os.path.join(tmp, "u2.bam")
        block = r1_block(8192, rng, whitelist)
        reps = max(1, n_records // len(block))
        n = reps * len(block)
        write_fastq(r1, b"".join(block), reps, bgzf=True)
        write_fastq(i1, b"".join(rec.split(b"\n")[0] + b"\nACGTACGT\n+\nFFFFFFFF\n" for rec in block), reps, bgzf=True)
        write_unaligned_bam(u2, n, rng)
        sizes = {"r1_gz_bytes": os.path.getsize(r1), "i1_gz_bytes": os.path.getsize(i1), "u2_bam_bytes": os.path.getsize(u2),
                 "r1_text_bytes": reps * len(b"".join(block))}
        who = {}

        def run(mode):
            dst = os.path.join(tmp, "tagged_%s.bam" % mode)
            generators = platform.TenXV2._make_tag_generators(r1, i1, whitelist_file)
            tagger = bam.Tagger(u2, inflate=mode)
            torch.cuda.synchronize()
            with Phases() as phases:
                t0 = time.perf_counter()
                tagger.tag(dst, generators)
                total = time.perf_counter() - t0
            who[mode] = sorted(set(generators[0].inflated_by.values()) | set(generators[1].inflated_by.values()))
            assert not generators[0].declined and not generators[1].declined
            return total, {k: round(v, 3) for k, v in phases.seconds.items()}

        out = alternate(run, modes, runs)
        files = [open(os.path.join(tmp, "tagged_%s.bam" % mode), "rb").read() for mode in modes]
        assert all(f == files[0] for f in files)
        return {"what": "Attach10xBarcodes --whitelist end to end on BGZF FASTQ, --inflate host and auto in turn",
                "records": n, "runs": runs, **sizes, "inflated_by": who, **out,
                "phase_key": {"read": "host gunzip into the pinned window (inflate=host)",
                              "stage_h2d_inflate_crc": "mapped file -> pinned buffer -> GPU, k_inflate, k_fq_crc32; synchronized",
                              "h2d_kernels": "copy to the GPU (host path) + sct_fq_count + sct_fq_extract, synchronized",
                              "correct": "sct_bc_correct", "write": "native BAM writer: record rebuild + BGZF deflate"}}


def e2e_line(n_records, whitelist_file):
    rng = np.random.default_rng(5)
    whitelist = [ln[:-1].encode() for ln in open(whitelist_file) if set(ln[:-1]) <= set("ACGT")]
    with tempfile.TemporaryDirectory() as tmp:
        r1, i1, u2 = os.path.join(tmp, "R1.fastq.gz"), os.path.join(tmp, "I1.fastq.gz"), os.path.join(tmp, "u2.bam")
        block = r1_block(8192, rng, whitelist)
        reps = max(1, n_records // len(block))
        n = reps * len(block)
        with gzip.open(r1, "wb", compresslevel=4) as f:
            for _ in range(reps):
                f.write(b"".join(block))
        iblock = b"".join(rec.split(b"\n")[0] + b"\nACGTACGT\n+\nFFFFFFFF\n" for rec in block)
        with gzip.open(i1, "wb", compresslevel=4) as f:
            for _ in range(reps):
                f.write(iblock)
        write_unaligned_bam(u2, n, rng)
        sizes = {"r1_gz_bytes": os.path.getsize(r1), "i1_gz_bytes": os.path.getsize(i1), "u2_bam_bytes": os.path.getsize(u2),
                 "r1_text_bytes": reps * len(b"".join(block))}
        out = {}
        for path in ("device", "host"):
            dst = os.path.join(tmp, "tagged_%s.bam" % path)
            generators = platform.TenXV2._make_tag_generators(r1, i1, whitelist_file)
            if path == "host":
                generators = [iter(g) for g in generators]  # plain iterables: consumed record by record on the host
            tagger = bam.Tagger(u2)
            torch.cuda.synchronize()
            with Phases() as phases:
                t0 = time.perf_counter()
                tagger.tag(dst, generators)
                total = time.perf_counter() - t0
            timings = {k: round(v, 3) for k, v in phases.seconds.items()}
            known = sum(timings.values())
            out[path] = {"total_s": round(total, 3), "records_per_s": round(n / total), "phases_s": timings,
                         "other_s": round(total - known, 3), "output_bytes": os.path.getsize(dst)}
        a = [r.get_tags() for _, r in zip(range(2000), bam.open_alignments(os.path.join(tmp, "tagged_device.bam"), "rb"))]
        b = [r.get_tags() for _, r in zip(range(2000), bam.open_alignments(os.path.join(tmp, "tagged_host.bam"), "rb"))]
        assert a == b and any("CB" in dict(t) for t in a)
        return {"what": "Attach10xBarcodes --whitelist end to end; 'host' is this package's port of the reference's "
                        "per-record loop into the same native writer, not the reference itself",
                "records": n, **sizes, "device_path": out["device"], "host_iterator_path": out["host"],
                "phase_key": {"read": "gunzip into the pinned window",
                              "h2d_kernels": "copy to the GPU + sct_fq_count + sct_fq_extract, synchronized",
                              "correct": "sct_bc_correct", "write": "native BAM writer: record rebuild + BGZF deflate",
                              "other_s": "D2H of the columns, input BAM inflate, Python glue; on the host path, the "
                                         "per-record loop itself"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--e2e-records", type=int, default=1_000_000)
    ap.add_argument("--whitelist", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                        "tests", "golden", "barcode", "1k-august-2016.txt"))
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--bgzf", action="store_true", help="instead: Attach10xBarcodes on BGZF-compressed copies of the "
                    "FASTQ inputs, the --inflate modes in turn (DESIGN.md section 19)")
    ap.add_argument("--inflate", default="both", choices=["both", "auto", "host"], help="with --bgzf: the mode(s) to run")
    ap.add_argument("--runs", type=int, default=5, help="with --bgzf: timed runs per mode, after one warm-up of each")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("fastq_bench needs a ROCm GPU; a CPU run gives no timing")
    torch.cuda.set_device(0)
    if args.bgzf:
        modes = ("host", "auto") if args.inflate == "both" else (args.inflate,)
        lines = [bgzf_line(args.e2e_records, args.whitelist, args.runs, modes)]
    else:
        lines = [kernel_line(args.records, args.calls)]
        if args.e2e_records > 0:
            lines.append(e2e_line(args.e2e_records, args.whitelist))
    for line in lines:
        text = json.dumps(line, sort_keys=True)
        print(text, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
