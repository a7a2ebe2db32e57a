"""
FastqProcess -- the reference's ``fastqprocess`` and its read-structure sibling ``fastq_slideseq``
(``fastqpreprocessing/src/fastqprocess.cpp``, ``fastq_slideseq.cpp``, ``fastq_common.cpp``): I1/R1/R2
FASTQ triples to N output shards, unaligned BAMs (``subfile_<i>.bam``) or R1/R2 FASTQ pairs
(``fastq_R1_<i>.fastq.gz``, ``fastq_R2_<i>.fastq.gz``).  The cell barcode and the UMI are cut out of
R1, the cell barcode is corrected against the whitelist, and every read goes to the shard that the
hash of its corrected barcode picks, so a cell never spans two shards.

The records are built on the GPU (``sct_fqp_*`` in ``libsct_fastq.so``,
``include/sct_fastq_process.h``): whole lines of R2 and I1, the shard of every record, a stable
partition by shard, and the record bytes written where the partition puts them.  The host reads
and decompresses the inputs and deflates the outputs (``sct_bam_shards_*`` in ``libsct_bam.so``).

``std_hash``             ``std::hash<std::string>`` of libstdc++ on x86-64, restated
``default_num_shards``   the reference's ``get_num_blocks``
``FastqProcess``         ``FastqProcess(r1_files, r2_files, ...).run()`` -> ``FastqProcessResult``
``text_window``, ``window_lines``, ``shards``, ``Batch``, ``plan``, ``emit``
                         the device calls one at a time, on tensors

ORDER: the triples are processed in the order given, and inside a shard the records stand in input
order.  The reference's order depends on its threads.

Deliberate departures, each a ``ValueError`` that leaves no output file:
  - the files of a triple hold different numbers of records (the reference stops at the shortest);
  - an R1 line is shorter than a barcode span (as in section 14);
  - an R2 or I1 record is flagged by ``sct_fqp_lines`` (name without ``@``, identifier empty or
    longer than 254 bytes, empty sequence, sequence and quality of different lengths, a quality
    byte below 33); the message names the file and the record;
  - the cell barcode is longer than 31 bases.
Without a whitelist no read gets ``CB`` and the raw barcode picks the shard (an addition: the
reference requires a whitelist).
"""
import ctypes
import math
import os
from collections import namedtuple
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from sctools_amd import _ffi, bamnative, fastq
from sctools_amd.fastq_metrics import kind_spans

BAD_NAME, BAD_IDENTIFIER, EMPTY_SEQUENCE, LENGTH_MISMATCH, LOW_QUALITY = 1, 2, 4, 8, 16
MAX_IDENTIFIER = 254
MAX_SHARDS = 1024
MAX_BARCODE = 31       # SCT_FQP_MAX_BARCODE, barcode.MAX_CORRECT_LENGTH
PLAN_TILE = 256        # SCT_FQP_PLAN_TILE
BAM, FASTQ = 0, 1
BAM_BIN = 4680         # reg2bin(-1, 0)
FORMATS = {"BAM": BAM, "FASTQ": FASTQ}

_FLAG_WORDS = ((BAD_NAME, "the name does not begin with @"),
               (BAD_IDENTIFIER, "the identifier is empty or longer than %d bytes" % MAX_IDENTIFIER),
               (EMPTY_SEQUENCE, "the sequence is empty"),
               (LENGTH_MISMATCH, "sequence and quality differ in length"),
               (LOW_QUALITY, "a quality byte is below 33"))


class FastqProcessError(RuntimeError):
    """A sct_fqp_* call returned an error code (message from sct_fq_last_error), or the device
    refused a record it had planned."""


class Records(ctypes.Structure):
    """``sct_fqp_records_t``."""
    _fields_ = [("n", ctypes.c_int64),
                ("r2_text", ctypes.c_void_p), ("r2_bytes", ctypes.c_int64),
                ("r2_off", ctypes.c_void_p), ("r2_len", ctypes.c_void_p),
                ("i1_text", ctypes.c_void_p), ("i1_bytes", ctypes.c_int64),
                ("i1_off", ctypes.c_void_p), ("i1_len", ctypes.c_void_p),
                ("cr", ctypes.c_void_p), ("cy", ctypes.c_void_p), ("ur", ctypes.c_void_p), ("uy", ctypes.c_void_p),
                ("cb", ctypes.c_void_p), ("cb_index", ctypes.c_void_p), ("shard", ctypes.c_void_p),
                ("cell_length", ctypes.c_int32), ("umi_length", ctypes.c_int32),
                ("n_shards", ctypes.c_int32), ("format", ctypes.c_int32)]


_P = ctypes.POINTER
_vp, _i64, _i32, _int, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_size_t

PROTOTYPES = {
    "sct_fqp_lines": (_int, [_vp, _i64, _i64, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "sct_fqp_shard": (_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    "sct_fqp_plan_workspace_size": (_int, [_i64, _i32, _i32, _P(_sz)]),
    "sct_fqp_plan": (_int, [_P(Records), _vp, _sz, _vp, _vp, _vp, _vp]),
    "sct_fqp_emit_bam": (_int, [_P(Records), _vp, _vp, _vp, _i64, _vp, _vp]),
    "sct_fqp_emit_fastq": (_int, [_P(Records), _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp]),
}
EXPORTED = tuple(PROTOTYPES)

# the sct_fqp_* calls live in libsct_fastq.so and report through sct_fq_last_error: fastq's handle, opened once
LIBRARY = _ffi.Library("libsct_fastq.so", "sct_fastq_process", "sct_fq_last_error", FastqProcessError, PROTOTYPES,
                       shares=fastq.LIBRARY)
load = LIBRARY.load
check = LIBRARY.check


# ---- host arithmetic ----

_MASK = (1 << 64) - 1
_MUL = 0xc6a4a7935bd1e995
_SEED = 0xc70f6907


def _mix(v: int) -> int:
    return v ^ (v >> 47)


def std_hash(data: bytes) -> int:
    """``std::hash<std::string>`` of libstdc++ on x86-64: ``_Hash_bytes(data, len, 0xc70f6907)``."""
    data = bytes(data)
    n = len(data)
    h = _SEED ^ ((n * _MUL) & _MASK)
    full = n & ~7
    for at in range(0, full, 8):
        d = int.from_bytes(data[at:at + 8], "little")
        h ^= (_mix((d * _MUL) & _MASK) * _MUL) & _MASK
        h = (h * _MUL) & _MASK
    if n & 7:
        h ^= int.from_bytes(data[full:], "little")
        h = (h * _MUL) & _MASK
    h = (_mix(h) * _MUL) & _MASK
    return _mix(h)


def default_num_shards(total_bytes: int, bam_size: float) -> int:
    """The reference's ``get_num_blocks``: ``ceil(total on-disk bytes / 2^30 / bam_size)``, and 1 for no bytes."""
    if not bam_size > 0:
        raise ValueError("bam_size must be positive, got %r" % (bam_size,))
    return max(1, int(math.ceil(total_bytes / float(1 << 30) / bam_size)))


def sam_header(sample_id: str) -> str:
    return "@HD\tVN:1.6\tSO:unsorted\n@RG\tID:A\tSM:%s\n" % sample_id


def structure_spans(barcode_length: Optional[int], umi_length: Optional[int], read_structure: Optional[str]):
    """``(cell spans, umi spans)`` as ``[start, end)`` lists, from the two lengths (cell barcode first,
    the UMI behind it) or from a read structure (``C`` cell, ``M`` UMI, anything else skipped)."""
    lengths = barcode_length is not None or umi_length is not None
    if lengths == (read_structure is not None):
        raise ValueError("give either barcode_length and umi_length, or read_structure")
    if read_structure is not None:
        cell, umi = kind_spans(read_structure, "C"), kind_spans(read_structure, "M")
    else:
        if barcode_length is None or umi_length is None:
            raise ValueError("barcode_length and umi_length are given together")
        if barcode_length < 0 or umi_length < 0:
            raise ValueError("barcode_length and umi_length must not be negative")
        cell = [(0, int(barcode_length))] if barcode_length else []
        umi = [(int(barcode_length), int(barcode_length) + int(umi_length))] if umi_length else []
    cell_length, umi_total = sum(e - s for s, e in cell), sum(e - s for s, e in umi)
    if cell_length < 1:
        raise ValueError("there is no cell barcode: nothing to pick the shard by")
    if cell_length > MAX_BARCODE:
        raise ValueError("the cell barcode has %d bases, the limit is %d" % (cell_length, MAX_BARCODE))
    if umi_total > 255:
        raise ValueError("the UMI has %d bases, the limit is 255" % umi_total)
    return cell, umi


# ---- the device calls, one at a time ----

def text_window(data: bytes, is_last: bool = True, device=None) -> fastq.Window:
    """``data`` on the device as a counted window (``sct_fq_count``), as ``TextWindows`` yields them."""
    import torch

    lib, dev = fastq.load(), _ffi.device(device)
    with torch.cuda.device(dev):
        host = np.frombuffer(bytes(data), dtype=np.uint8)
        text = torch.empty(max(len(host), 1), dtype=torch.uint8, device=dev)
        if len(host):
            text[:len(host)].copy_(torch.from_numpy(host.copy()))
        nbytes = ctypes.c_size_t(0)
        fastq.check(lib.sct_fq_workspace_size(len(host), ctypes.byref(nbytes)))
        work = torch.empty(int(nbytes.value) + 8, dtype=torch.uint8, device=dev)
        result = torch.empty(4, dtype=torch.int64, device=dev)
        fastq.check(lib.sct_fq_count(_ffi.ptr(text) if len(host) else None, len(host), 1 if is_last else 0,
                                     _ffi.ptr(work), work.numel(), _ffi.ptr(result), _ffi.stream(dev)))
        n = int(result[0].cpu())
    return fastq.Window(text, len(host), n, work, host)


def window_lines(window: fastq.Window, n_records: Optional[int] = None):
    """``sct_fqp_lines`` on a counted window: ``(off int64 [n, 3], len int32 [n, 3], first_flagged, flags)``;
    column 0 the identifier, 1 the sequence line, 2 the quality line."""
    import torch

    lib = load()
    text, n_bytes, n, work, _ = window
    n = n if n_records is None else int(n_records)
    dev = text.device
    with torch.cuda.device(dev):
        off = torch.empty((n, 3), dtype=torch.int64, device=dev)
        length = torch.empty((n, 3), dtype=torch.int32, device=dev)
        flags = torch.empty((n + 3) // 4 * 4, dtype=torch.uint8, device=dev)
        result = torch.empty(4, dtype=torch.int64, device=dev)
        check(lib.sct_fqp_lines(_ffi.ptr(text) if n_bytes else None, n_bytes, n, _ffi.ptr(work), work.numel(),
                                _ffi.ptr(off), _ffi.ptr(length), _ffi.ptr(flags), _ffi.ptr(result), _ffi.stream(dev)))
        first_flagged = int(result[3].cpu())
    return off, length, first_flagged, flags[:n]


def aligned16(t):
    """``t`` contiguous and 16-byte aligned, as ``sct_fqp_shard`` reads its columns: a copy where it is not (a
    row slice of a column begins wherever its first row does)."""
    if t is None:
        return None
    t = t.contiguous()
    return t.clone() if t.data_ptr() & 15 else t


def shards(raw, corrected, index, n_shards: int):
    """``sct_fqp_shard``: ``(shard int32 [n], (n_correct, n_corrected, n_uncorrectable))`` of the raw cell
    barcode column and, with a whitelist, the outputs of ``correct_barcodes``."""
    import torch

    lib = load()
    dev = raw.device
    n, length = int(raw.shape[0]), int(raw.shape[1])
    with torch.cuda.device(dev):
        raw, corrected = aligned16(raw), aligned16(corrected)
        index = None if index is None else index.contiguous()
        shard = torch.empty(n, dtype=torch.int32, device=dev)
        counts = torch.empty(3, dtype=torch.int64, device=dev)
        check(lib.sct_fqp_shard(_ffi.ptr(raw), _ffi.ptr(corrected) if n else None, _ffi.ptr(index) if n else None,
                                n, length, int(n_shards), _ffi.ptr(shard), _ffi.ptr(counts), _ffi.stream(dev)))
        counts = tuple(int(x) for x in counts.cpu())
    return shard, counts


class Batch:
    """The records of one R2 window as plan and emit read them: the tensors, kept alive, and the
    ``sct_fqp_records_t`` that points at them."""

    def __init__(self, r2_text, r2_bytes: int, r2_off, r2_len, cr, cy, ur, uy, shard, n_shards: int, fmt: int,
                 i1=None, cb=None, cb_index=None):
        self.n = int(r2_off.shape[0])
        self.device = r2_text.device
        self.n_shards, self.format = int(n_shards), int(fmt)
        c = (lambda t: None if t is None else t.contiguous())
        i1_text, i1_bytes, i1_off, i1_len = i1 if i1 is not None else (None, 0, None, None)
        self._keep = [c(t) for t in (r2_text, r2_off, r2_len, i1_text, i1_off, i1_len, cr, cy, ur, uy, cb, cb_index, shard)]
        p = [None if t is None else ctypes.c_void_p(t.data_ptr()) for t in self._keep]
        self.cell_length = int(cr.shape[1])
        self.umi_length = 0 if ur is None else int(ur.shape[1])
        self.shard = self._keep[12]
        self.c = Records(self.n, p[0], int(r2_bytes), p[1], p[2], p[3], int(i1_bytes), p[4], p[5], p[6], p[7],
                         p[8] if self.umi_length else None, p[9] if self.umi_length else None, p[10], p[11], p[12],
                         self.cell_length, self.umi_length, self.n_shards, self.format)

    @property
    def outputs(self) -> int:
        return 2 if self.format == FASTQ else 1


def plan(batch: Batch):
    """``sct_fqp_plan``: ``(offsets int64 [K, n], shard_counts int64 [S], shard_bytes int64 [K, S])`` on the device."""
    import torch

    lib, dev, k = load(), batch.device, batch.outputs
    with torch.cuda.device(dev):
        nbytes = ctypes.c_size_t(0)
        check(lib.sct_fqp_plan_workspace_size(batch.n, batch.n_shards, batch.format, ctypes.byref(nbytes)))
        work = torch.empty(int(nbytes.value) + 8, dtype=torch.uint8, device=dev)
        offsets = torch.empty((k, batch.n), dtype=torch.int64, device=dev)
        shard_counts = torch.empty(batch.n_shards, dtype=torch.int64, device=dev)
        shard_bytes = torch.empty((k, batch.n_shards), dtype=torch.int64, device=dev)
        check(lib.sct_fqp_plan(ctypes.byref(batch.c), _ffi.ptr(work), work.numel(), _ffi.ptr(offsets),
                               _ffi.ptr(shard_counts), _ffi.ptr(shard_bytes), _ffi.stream(dev)))
        torch.cuda.current_stream(dev).synchronize()  # `work` may be freed
    return offsets, shard_counts, shard_bytes


def emit(batch: Batch, offsets, shard_bytes):
    """``sct_fqp_emit_bam`` / ``sct_fqp_emit_fastq``: ``(out uint8 tensor, bounds int64 numpy [K * S + 1])``.  The
    buffer holds shard 0, shard 1, ... of output 0, then of output 1; ``bounds`` cuts it."""
    import torch

    lib, dev, k, s = load(), batch.device, batch.outputs, batch.n_shards
    with torch.cuda.device(dev):
        sizes = shard_bytes.reshape(-1).cpu().numpy()
        bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        total1 = int(bounds[s])
        total = int(bounds[-1])
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        base = torch.from_numpy(bounds[:-1].copy())
        if k == 2:
            base[s:] -= total1  # the second output's shards are counted from its own first byte
        base = base.to(dev)
        error = torch.empty(1, dtype=torch.int64, device=dev)
        if batch.format == BAM:
            check(lib.sct_fqp_emit_bam(ctypes.byref(batch.c), _ffi.ptr(offsets), _ffi.ptr(base), _ffi.ptr(out), total,
                                       _ffi.ptr(error), _ffi.stream(dev)))
        else:
            out2 = ctypes.c_void_p(out.data_ptr() + total1)
            check(lib.sct_fqp_emit_fastq(ctypes.byref(batch.c), _ffi.ptr(offsets), _ffi.ptr(base), _ffi.ptr(out), total1,
                                         out2, total - total1, _ffi.ptr(error), _ffi.stream(dev)))
        refused = int(error.cpu())
        if refused:
            raise FastqProcessError("the device refused %d of %d records: a line or a planned offset lies outside "
                                    "its buffer" % (refused, batch.n))
    return out[:total], bounds


def to_host(out) -> np.ndarray:
    """The emitted bytes on the host, for the shard writer."""
    return out.cpu().numpy()


# ---- the streams of a triple ----

class _Taker:
    """The records of a stream of windows, handed out ``m`` at a time.  ``source`` yields ``(n, payload)``;
    ``take`` returns ``[(payload, a, b)]`` whose row ranges add up to ``m``, or to less at the stream's end."""

    def __init__(self, source):
        self._source = iter(source)
        self._payload, self._at, self._n = None, 0, 0

    def _refill(self) -> bool:
        while self._at >= self._n:
            nxt = next(self._source, None)
            if nxt is None:
                return False
            self._n, self._payload = nxt
            self._at = 0
        return True

    def take(self, m: int):
        pieces = []
        while m > 0 and self._refill():
            k = min(m, self._n - self._at)
            pieces.append((self._payload, self._at, self._at + k))
            self._at += k
            m -= k
        return pieces

    def more(self) -> bool:
        return self._refill()


def _flag_error(path: str, record: int, flag: int) -> ValueError:
    words = "; ".join(w for bit, w in _FLAG_WORDS if flag & bit)
    return ValueError("%s: FASTQ record %d: %s" % (path, record, words))


def _line_windows(windows, keep_text: bool):
    """Per window of the one file of the ``TextWindows`` ``windows``: ``(n, (window, text, off, len))`` after
    ``sct_fqp_lines``; a flagged record raises.  With ``keep_text`` the text is a copy that outlives the window."""
    base, path = 0, windows.files[0]
    for window in windows:
        off, length, first_flagged, flags = window_lines(window)
        if first_flagged >= 0:
            raise _flag_error(path, base + first_flagged, int(flags[first_flagged].cpu()))
        text = window.text[:window.n_bytes].clone() if keep_text else window.text
        yield window.n_records, (window, text, off, length)
        base += window.n_records


def _column_windows(windows, spans):
    """Per window of the R1 file of ``windows``: ``(n, [(seq, qual) per span])``; a short line raises."""
    base, max_end = 0, max(end for _, end in spans)
    for window in windows:
        columns, first_flagged, flags = fastq.extract_spans(window, spans)
        if first_flagged >= 0:
            raise fastq.flag_error(window, base, first_flagged, flags, max_end)
        yield window.n_records, columns
        base += window.n_records


FastqProcessResult = namedtuple("FastqProcessResult", ["paths", "n_reads", "n_correct", "n_corrected",
                                                       "n_uncorrectable", "shard_counts"])


class FastqProcess:
    """I1/R1/R2 FASTQ triples to sharded unaligned BAM or FASTQ.

    Parameters
    ----------
    r1_files, r2_files : str or list of str
        the barcode reads and the cDNA reads, plain or gzip/bz2 compressed, file k of one with file k of the other
    i1_files : str or list of str, optional
        the index reads; their sequence and quality lines become ``SR`` and ``SY``
    whitelist : str, optional
        one barcode per line; without it no read gets ``CB``
    barcode_length, umi_length : int
        the cell barcode is the first ``barcode_length`` bases of R1, the UMI the ``umi_length`` behind it
    read_structure : str
        instead of the two lengths, e.g. ``8C18X6C9M1X``
    sample_id : str
        the ``SM`` of the BAM header's read group
    output_format : {"BAM", "FASTQ"}
    bam_size : float
        GiB of input per shard where ``num_shards`` is not given
    num_shards : int, optional
    output_dir : str
    inflate : {"auto", "host"}
        ``"auto"`` inflates BGZF-compressed inputs on the GPU (``fastq.TextWindows``), ``"host"`` none; after
        ``run()``, ``inflated_by`` maps every input file to ``"device"`` or ``"host"`` and ``declined`` a file the
        device gave back to the reason
    """

    def __init__(self, r1_files, r2_files, i1_files=None, whitelist: Optional[str] = None,
                 barcode_length: Optional[int] = None, umi_length: Optional[int] = None,
                 read_structure: Optional[str] = None, sample_id: str = "", output_format: str = "BAM",
                 bam_size: float = 1.0, num_shards: Optional[int] = None, output_dir: str = ".",
                 inflate: str = fastq.DEFAULT_INFLATE):
        self.inflate = fastq.check_inflate(inflate)
        self.inflated_by, self.declined = {}, {}
        as_list = (lambda f: [f] if isinstance(f, (str, os.PathLike)) else list(f))
        self.r1_files, self.r2_files = as_list(r1_files), as_list(r2_files)
        self.i1_files = as_list(i1_files) if i1_files else []
        if not self.r1_files:
            raise ValueError("no R1 file")
        if len(self.r1_files) != len(self.r2_files):
            raise ValueError("%d R1 files and %d R2 files" % (len(self.r1_files), len(self.r2_files)))
        if self.i1_files and len(self.i1_files) != len(self.r1_files):
            raise ValueError("%d I1 files and %d R1 files" % (len(self.i1_files), len(self.r1_files)))
        if output_format not in FORMATS:
            raise ValueError("output_format must be BAM or FASTQ, got %r" % (output_format,))
        self.cell_spans, self.umi_spans = structure_spans(barcode_length, umi_length, read_structure)
        self.cell_length = sum(e - s for s, e in self.cell_spans)
        self.umi_length = sum(e - s for s, e in self.umi_spans)
        self.whitelist, self.sample_id = whitelist, sample_id
        self.output_format, self.output_dir = output_format, os.fspath(output_dir)
        if num_shards is None:
            total = sum(os.stat(f).st_size for f in self.r1_files + self.r2_files + self.i1_files)
            num_shards = default_num_shards(total, bam_size)
        self.num_shards = int(num_shards)
        if not 1 <= self.num_shards <= MAX_SHARDS:
            raise ValueError("%d shards: outside 1..%d" % (self.num_shards, MAX_SHARDS))

    def paths(self) -> List[str]:
        """The output files: the BAM shards, or the R1 shards followed by the R2 shards."""
        shards_ = range(self.num_shards)
        if self.output_format == "BAM":
            names = ["subfile_%d.bam" % i for i in shards_]
        else:
            names = ["fastq_R1_%d.fastq.gz" % i for i in shards_] + ["fastq_R2_%d.fastq.gz" % i for i in shards_]
        return [os.path.join(self.output_dir, name) for name in names]

    def run(self, device=None, window_bytes: int = 256 << 20, level: int = 6, threads: int = 0) -> FastqProcessResult:
        """Reads the triples in order, a window of at most ``window_bytes`` of text at a time per stream, and
        writes the shards.  Never more than one window of R2 is on the device."""
        import torch

        from sctools_amd.barcode import ErrorsToCorrectBarcodesMap

        dev = _ffi.device(device)
        corrector = None
        if self.whitelist is not None:
            corrector = ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(self.whitelist, device=dev)
            if corrector.barcode_length != self.cell_length:
                raise ValueError("the whitelist's barcodes have %d bases, the cell barcode has %d"
                                 % (corrector.barcode_length, self.cell_length))
        for f in self.r1_files + self.r2_files + self.i1_files:
            if not os.path.exists(f):
                raise FileNotFoundError(f)
        fmt = FORMATS[self.output_format]
        paths = self.paths()
        headers = [sam_header(self.sample_id)] * len(paths) if fmt == BAM else None
        totals = np.zeros(3, dtype=np.int64)
        shard_totals = np.zeros(self.num_shards, dtype=np.int64)
        n_reads = 0
        with bamnative.ShardWriter(paths, headers, level=level, threads=threads) as writer, torch.cuda.device(dev):
            for k, (r1, r2) in enumerate(zip(self.r1_files, self.r2_files)):
                i1 = self.i1_files[k] if self.i1_files else None
                for batch, counts in self._batches(r1, r2, i1, corrector, fmt, dev, window_bytes):
                    offsets, shard_counts, shard_bytes = plan(batch)
                    out, bounds = emit(batch, offsets, shard_bytes)
                    writer.append(to_host(out), bounds)
                    totals += np.asarray(counts, dtype=np.int64)
                    shard_totals += shard_counts.cpu().numpy()
                    n_reads += batch.n
        return FastqProcessResult(paths, n_reads, int(totals[0]), int(totals[1]), int(totals[2]), shard_totals.tolist())

    def _batches(self, r1: str, r2: str, i1: Optional[str], corrector, fmt: int, dev, window_bytes: int):
        """Per R2 window of one triple: ``(Batch, (n_correct, n_corrected, n_uncorrectable))``."""
        streams = [fastq.TextWindows([f], dev, window_bytes, inflate=self.inflate) if f else None for f in (r1, i1, r2)]
        try:
            yield from self._triple(streams, r1, r2, i1, corrector, fmt)
        finally:  # who inflated the three files, as far as they were read
            for stream in streams:
                if stream is not None:
                    self.inflated_by.update(stream.inflated_by)
                    self.declined.update(stream.declined)

    def _triple(self, streams, r1: str, r2: str, i1: Optional[str], corrector, fmt: int):
        import torch

        spans = self.cell_spans + self.umi_spans
        n_cell = len(self.cell_spans)
        columns = _Taker(_column_windows(streams[0], spans))
        index_lines = _Taker(_line_windows(streams[1], keep_text=True)) if i1 else None
        done = 0

        def short(path, have):
            return ValueError("%s holds %d records, %s holds more: the files of a triple must hold the same number"
                              % (path, have, r2))

        for n, (window, text, off, length) in _line_windows(streams[2], keep_text=False):
            pieces = columns.take(n)
            if sum(b - a for _, a, b in pieces) < n:
                raise short(r1, done + sum(b - a for _, a, b in pieces))
            joined = []  # per span (seq, qual) of the n records
            for s in range(len(spans)):
                joined.append(tuple(torch.cat([cols[s][q][a:b] for cols, a, b in pieces]) if len(pieces) > 1
                                    else pieces[0][0][s][q][pieces[0][1]:pieces[0][2]] for q in (0, 1)))
            side = (lambda group, q: group[0][q] if len(group) == 1 else torch.cat([g[q] for g in group], dim=1))
            cr, cy = (side(joined[:n_cell], q).contiguous() for q in (0, 1))
            ur, uy = ((side(joined[n_cell:], q).contiguous() for q in (0, 1)) if self.umi_spans else (None, None))
            index_part = None
            if index_lines is not None:
                got = index_lines.take(n)
                if sum(b - a for _, a, b in got) < n:
                    raise short(i1, done + sum(b - a for _, a, b in got))
                if len(got) == 1:
                    (_, i1_text, i1_off, i1_len), a, b = got[0]
                    index_part = (i1_text, int(i1_text.numel()), i1_off[a:b], i1_len[a:b])
                else:  # the R2 window spans several I1 windows: their texts back to back, the offsets moved along
                    bases = np.concatenate([[0], np.cumsum([int(p[1].numel()) for p, _, _ in got])])
                    i1_text = torch.cat([p[1] for p, _, _ in got])
                    i1_off = torch.cat([p[2][a:b] + int(base) for (p, a, b), base in zip(got, bases)])
                    i1_len = torch.cat([p[3][a:b] for p, a, b in got])
                    index_part = (i1_text, int(i1_text.numel()), i1_off, i1_len)
            cb_index = cb = None
            if corrector is not None:
                cb_index, cb = corrector.correct_barcodes(cr, return_corrected=True)
                cb_index = cb_index.to(torch.int32)
            shard, counts = shards(cr, cb, cb_index, self.num_shards)
            yield Batch(text, window.n_bytes, off, length, cr, cy, ur, uy, shard, self.num_shards, fmt,
                        i1=index_part, cb=cb, cb_index=cb_index), counts
            done += n
        if columns.more():
            raise ValueError("%s holds more than the %d records of %s: the files of a triple must hold the same number"
                             % (r1, done, r2))
        if index_lines is not None and index_lines.more():
            raise ValueError("%s holds more than the %d records of %s: the files of a triple must hold the same number"
                             % (i1, done, r2))
