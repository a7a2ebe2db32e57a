"""
FastqMetrics -- the reference's ``fastq_metrics`` tool (``fastqpreprocessing/src/fastq_metrics.cpp``):
for a read structure such as ``16C10M`` or ``8C18X6C9M1X``, the number of reads per distinct cell
barcode (``C``) and per distinct UMI (``M``) of the R1 file(s), and a position weight matrix of each,
in the reference's four text files.  The counting runs on the GPU (``sct_fqm_*`` in
``libsct_fastq.so``, ``include/sct_fastq_metrics.h``) over the columns that ``sct_fq_extract`` cuts
from the FASTQ text.

``parse_read_structure``   ``"8C18X6C9M1X"`` -> ``[("C", 8), ("X", 18), ("C", 6), ("M", 9), ("X", 1)]``
``FastqMetrics``           ``FastqMetrics(r1_files, read_structure).compute()`` -> ``FastqMetricsResult``
``FastqMetricsResult``     the arrays, and ``write(prefix)`` for the four files

A count key is the raw bytes of the barcode: ``acgt`` and ``ACGT`` are two keys, as in the
reference; only the matrices fold case.  Rows with a byte outside upper-case ``ACGTN`` do not fit
the device key; the device lists them and they are counted here in a ``Counter``
(``FastqMetricsResult.n_host_rows`` says how many).

ORDER OF THE COUNT FILES: by count descending, then by barcode bytes ascending.  This is a
definition of ours.  The reference sorts an ``unordered_map``'s entries by count alone with an
unstable ``std::sort``: its order among equal counts is whatever the hash and the sort give.

Deliberate departures:
  - the reference lets a short read yield a truncated barcode (``string_view::substr`` clamps), and
    libStatGen silently stops at the first malformed record.  Here a record the extractor flags
    (sequence or quality line shorter than the last ``C``/``M`` base, name without ``@``) raises the
    ``ValueError`` that ``EmbeddedBarcodeGenerator.columns()`` raises, naming the record;
  - barcodes and UMIs of more than 21 bases (each kind's spans together) are refused;
  - the whitelist is accepted and unused, which is what the reference does with it as well
    (``white_list_data`` is handed down and never read).
"""
import ctypes
import sys
from collections import Counter
from typing import Iterable, List, Optional, Tuple, Union

import numpy as np

from sctools_amd import _ffi, fastq

MAX_LENGTH = 21        # SCT_FQM_MAX_LENGTH
MIN_SLOTS = 64         # SCT_FQM_MIN_SLOTS
TILE_ROWS = 512        # SCT_FQM_TILE_ROWS
R = TILE_ROWS
PWM_CLASSES = 6        # A C G T N other
KEY_ALPHABET = b"ACGNT"  # code 0..4 of the device key: byte order


class FastqMetricsError(RuntimeError):
    """A sct_fqm_* call returned an error code (message from sct_fqm_last_error)."""


_vp, _i64, _i32, _int, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_size_t

PROTOTYPES = {
    "sct_fqm_last_error": (ctypes.c_char_p, []),
    "sct_fqm_table_size": (_int, [_i64, ctypes.POINTER(_sz)]),
    "sct_fqm_table_init": (_int, [_vp, _i64, _sz, _vp]),
    "sct_fqm_accumulate": (_int, [_vp, _i64, _i32, _vp, _i64, _sz, _vp, _vp, _vp, _vp]),
    "sct_fqm_rehash": (_int, [_vp, _i64, _sz, _vp, _i64, _sz, _vp, _vp]),
    "sct_fqm_compact": (_int, [_vp, _i64, _sz, _vp, _vp, _i64, _vp, _vp]),
}
EXPORTED = tuple(PROTOTYPES)

# the sct_fqm_* calls live in libsct_fastq.so: fastq's handle, opened once
LIBRARY = _ffi.Library("libsct_fastq.so", "sct_fastq_metrics", "sct_fqm_last_error", FastqMetricsError, PROTOTYPES,
                       shares=fastq.LIBRARY)
load = LIBRARY.load
check = LIBRARY.check


def parse_read_structure(read_structure: str) -> List[Tuple[str, int]]:
    """``[(type letter, length)]`` of a read structure: digits, then one character of any kind that is
    no digit.  ``ValueError`` for a type with no digits before it (the reference's ``stoi`` throws
    there) and for trailing digits with no type (the reference asserts there)."""
    out, digits = [], ""
    for ch in read_structure:
        if ch in "0123456789":
            digits += ch
            continue
        if not digits:
            raise ValueError("read structure %r: type %r has no length before it" % (read_structure, ch))
        out.append((ch, int(digits)))
        digits = ""
    if digits:
        raise ValueError("read structure %r: the trailing length %s has no type" % (read_structure, digits))
    return out


def kind_spans(read_structure: str, kind: str) -> List[Tuple[int, int]]:
    """The ``[start, end)`` of every non-empty segment of type ``kind``, left to right."""
    spans, at = [], 0
    for type_, length in parse_read_structure(read_structure):
        if type_ == kind and length > 0:
            spans.append((at, at + length))
        at += length
    return spans


def decode_keys(keys: np.ndarray, length: int) -> np.ndarray:
    """``uint8 [D, length]`` barcodes of device keys (3 bits per base, first base highest)."""
    keys = np.asarray(keys, dtype=np.uint64)
    alphabet = np.frombuffer(KEY_ALPHABET + b"???", dtype=np.uint8)
    out = np.empty((len(keys), length), dtype=np.uint8)
    for j in range(length):
        out[:, j] = alphabet[((keys >> np.uint64(3 * (length - 1 - j))) & np.uint64(7)).astype(np.intp)]
    return out


def sort_counts(barcodes: np.ndarray, counts: np.ndarray):
    """Rows ordered by count descending, then barcode bytes ascending."""
    length = barcodes.shape[1]
    order = np.lexsort([barcodes[:, j] for j in range(length - 1, -1, -1)] + [-counts])
    return barcodes[order], counts[order]


def next_slots(n_slots: int, distinct: int, rows: int) -> int:
    """The growth rule: the smallest power-of-two multiple of ``n_slots`` with ``2 * (distinct + rows)`` slots."""
    while n_slots < 2 * (distinct + rows):
        n_slots *= 2
    return n_slots


class FastqMetricsResult:
    """What ``FastqMetrics.compute`` returns.

    ``barcodes`` (uint8 [D, L]) and ``barcode_counts`` (int64 [D]), ``umis`` and ``umi_counts``: the
    distinct keys and their reads, by count descending, then bytes ascending.
    ``barcode_pwm``, ``umi_pwm`` (int64 [L, 5]): per position the reads with A, C, G, T, N (either case).
    ``barcode_other``, ``umi_other`` (int64 [L]): per position the reads with any other byte.
    ``n_records``: the records read.  ``n_host_rows``: the rows, of both kinds together, that the
    device handed to the host to count.
    """

    def __init__(self, barcodes, barcode_counts, umis, umi_counts, barcode_pwm, umi_pwm, barcode_other, umi_other,
                 n_records: int, n_host_rows: int = 0):
        self.barcodes = np.asarray(barcodes, dtype=np.uint8)
        self.barcode_counts = np.asarray(barcode_counts, dtype=np.int64)
        self.umis = np.asarray(umis, dtype=np.uint8)
        self.umi_counts = np.asarray(umi_counts, dtype=np.int64)
        self.barcode_pwm = np.asarray(barcode_pwm, dtype=np.int64)
        self.umi_pwm = np.asarray(umi_pwm, dtype=np.int64)
        self.barcode_other = np.asarray(barcode_other, dtype=np.int64)
        self.umi_other = np.asarray(umi_other, dtype=np.int64)
        self.n_records = int(n_records)
        self.n_host_rows = int(n_host_rows)

    @staticmethod
    def _write_counts(path: str, rows: np.ndarray, counts: np.ndarray) -> None:
        with open(path, "wb") as f:
            for at in range(0, len(counts), 1 << 16):
                f.write(b"".join(b"%d\t%s\n" % (c, r.tobytes())
                                 for c, r in zip(counts[at:at + (1 << 16)].tolist(), rows[at:at + (1 << 16)])))

    @staticmethod
    def _write_pwm(path: str, pwm: np.ndarray) -> None:
        with open(path, "wb") as f:
            f.write(b"position\tA\tC\tG\tT\tN\n")
            for i, row in enumerate(pwm.tolist()):
                f.write(b"%d\t%d\t%d\t%d\t%d\t%d\n" % (i + 1, *row))

    def write(self, prefix: str) -> List[str]:
        """Writes ``PREFIX.numReads_perCell_X{C,M}.txt`` (``count\\tbarcode`` lines) and
        ``PREFIX.barcode_distribution_X{C,M}.txt`` (header, then ``position\\tA\\tC\\tG\\tT\\tN`` lines,
        positions from 1); returns the four names."""
        names = [prefix + ".numReads_perCell_XM.txt", prefix + ".numReads_perCell_XC.txt",
                 prefix + ".barcode_distribution_XC.txt", prefix + ".barcode_distribution_XM.txt"]
        self._write_counts(names[0], self.umis, self.umi_counts)
        self._write_counts(names[1], self.barcodes, self.barcode_counts)
        self._write_pwm(names[2], self.barcode_pwm)
        self._write_pwm(names[3], self.umi_pwm)
        return names


class _KindAccumulator:
    """One kind's (``C`` or ``M``) device state: table, matrix, result block; and its host counter."""

    def __init__(self, length: int, initial_slots: int, dev):
        import torch

        self.length, self.dev = length, dev
        self.lib = load()
        self.result = torch.zeros(4, dtype=torch.int64, device=dev)
        self.pwm = torch.zeros((length, PWM_CLASSES), dtype=torch.int64, device=dev)
        self.host = Counter()
        self.host_rows = 0
        self.distinct = 0
        self.n_slots, self.table = 0, None
        self._new_table(initial_slots)

    def _new_table(self, n_slots: int):
        import torch

        nbytes = ctypes.c_size_t(0)
        check(self.lib.sct_fqm_table_size(n_slots, ctypes.byref(nbytes)))
        table = torch.empty(int(nbytes.value), dtype=torch.uint8, device=self.dev)
        check(self.lib.sct_fqm_table_init(_ffi.ptr(table), n_slots, table.numel(), _ffi.stream(self.dev)))
        old = (self.table, self.n_slots)
        self.table, self.n_slots = table, n_slots
        return old

    def _read_result(self):
        distinct, exceptions, compacted, error = (int(x) for x in self.result.cpu())
        if error:
            raise FastqMetricsError("the count table dropped %d rows: the growth rule was not kept" % error)
        self.distinct = distinct
        return exceptions, compacted

    def add(self, col) -> None:
        """Accumulates one window's column (uint8 [n, length] on the device, contiguous)."""
        import torch

        n = int(col.shape[0])
        if n == 0:
            return
        col = col.contiguous()
        want = next_slots(self.n_slots, self.distinct, n)
        if want != self.n_slots:
            old, old_slots = self._new_table(want)
            check(self.lib.sct_fqm_rehash(_ffi.ptr(old), old_slots, old.numel(), _ffi.ptr(self.table), self.n_slots,
                                          self.table.numel(), _ffi.ptr(self.result), _ffi.stream(self.dev)))
        exceptions = torch.empty(n, dtype=torch.int64, device=self.dev)
        check(self.lib.sct_fqm_accumulate(_ffi.ptr(col), n, self.length, _ffi.ptr(self.table), self.n_slots,
                                          self.table.numel(), _ffi.ptr(self.pwm), _ffi.ptr(exceptions),
                                          _ffi.ptr(self.result), _ffi.stream(self.dev)))
        n_exceptions, _ = self._read_result()  # (waits for the kernels: `old` and `col` are free from here)
        if n_exceptions:
            rows = col[exceptions[:n_exceptions]].cpu().numpy()
            self.host.update(r.tobytes() for r in rows)
            self.host_rows += n_exceptions

    def finish(self):
        """(barcodes, counts) sorted, pwm [L, 5], other [L]."""
        import torch

        keys = torch.empty(max(self.distinct, 1), dtype=torch.int64, device=self.dev)
        counts = torch.empty(max(self.distinct, 1), dtype=torch.int64, device=self.dev)
        check(self.lib.sct_fqm_compact(_ffi.ptr(self.table), self.n_slots, self.table.numel(), _ffi.ptr(keys),
                                       _ffi.ptr(counts), self.distinct, _ffi.ptr(self.result), _ffi.stream(self.dev)))
        _, compacted = self._read_result()
        if compacted != self.distinct:
            raise FastqMetricsError("%d occupied slots, %d distinct keys counted" % (compacted, self.distinct))
        rows = decode_keys(keys[:compacted].cpu().numpy().view(np.uint64), self.length)
        counts = counts[:compacted].cpu().numpy()
        if self.host:
            extra = np.frombuffer(b"".join(self.host), dtype=np.uint8).reshape(len(self.host), self.length)
            rows = np.concatenate([rows, extra])
            counts = np.concatenate([counts, np.fromiter(self.host.values(), dtype=np.int64, count=len(self.host))])
        rows, counts = sort_counts(rows, counts)
        pwm = self.pwm.cpu().numpy()
        return rows, counts, pwm[:, :5].copy(), pwm[:, 5].copy()


class FastqMetrics:
    """Reads per distinct cell barcode and UMI, and their position weight matrices, of R1 FASTQ file(s).

    Parameters
    ----------
    r1_files : str or list of str
        plain or gzip/bz2 compressed; several files are read as one stream, as the reference's
        ``--R1`` shards are summed
    read_structure : str
        e.g. ``16C10M``: ``C`` segments together are the cell barcode, ``M`` segments the UMI
    whitelist : str, optional
        accepted and unused, as in the reference
    inflate : {"auto", "host"}
        ``"auto"`` inflates BGZF-compressed files on the GPU (``fastq.TextWindows``), ``"host"`` none; after
        ``compute()``, ``inflated_by`` maps each file to ``"device"`` or ``"host"`` and ``declined`` a file the
        device gave back to the reason
    """

    def __init__(self, r1_files: Union[str, Iterable[str]], read_structure: str, whitelist: Optional[str] = None,
                 inflate: str = fastq.DEFAULT_INFLATE):
        self.r1_files = [r1_files] if isinstance(r1_files, str) else list(r1_files)
        self.inflate = fastq.check_inflate(inflate)
        self.inflated_by, self.declined = {}, {}
        self.read_structure = read_structure
        self.whitelist = whitelist
        self.barcode_spans = kind_spans(read_structure, "C")
        self.umi_spans = kind_spans(read_structure, "M")
        self.barcode_length = sum(e - s for s, e in self.barcode_spans)
        self.umi_length = sum(e - s for s, e in self.umi_spans)
        if not self.barcode_spans and not self.umi_spans:
            raise ValueError("read structure %r has neither a C nor an M segment: nothing to count" % read_structure)
        for what, length in (("cell barcode", self.barcode_length), ("UMI", self.umi_length)):
            if length > MAX_LENGTH:
                raise ValueError("read structure %r: the %s has %d bases, the limit is %d"
                                 % (read_structure, what, length, MAX_LENGTH))

    def compute(self, device=None, window_bytes: int = 256 << 20, initial_slots: int = 1 << 20) -> FastqMetricsResult:
        """Reads the files a window of ``window_bytes`` of text at a time and counts on the GPU.  The count
        tables start at ``initial_slots`` slots (rounded up to a power of two of at least 64) and double
        by the growth rule of ``include/sct_fastq_metrics.h``."""
        import torch

        spans = self.barcode_spans + self.umi_spans
        max_end = max(end for _, end in spans)
        slots = MIN_SLOTS
        while slots < int(initial_slots):
            slots *= 2
        windows = fastq.TextWindows(self.r1_files, device, window_bytes, inflate=self.inflate)
        self.inflated_by, self.declined = windows.inflated_by, windows.declined
        dev = windows.device
        n_records = 0
        with torch.cuda.device(dev):
            kinds = [_KindAccumulator(length, slots, dev) if length else None
                     for length in (self.barcode_length, self.umi_length)]
            for window in windows:
                cols, first_flagged, flags = fastq.extract_spans(window, spans)
                if first_flagged >= 0:
                    raise fastq.flag_error(window, n_records, first_flagged, flags, max_end)
                n_records += window.n_records
                seqs = [seq for seq, _ in cols]
                groups = (seqs[:len(self.barcode_spans)], seqs[len(self.barcode_spans):])
                for kind, group in zip(kinds, groups):
                    if kind is not None:
                        kind.add(group[0] if len(group) == 1 else torch.cat(group, dim=1))
            out, n_host_rows = [], 0
            for kind in kinds:
                if kind is None:  # the reference's map then holds one key, the empty string, once per record
                    out.append((np.zeros((1 if n_records else 0, 0), dtype=np.uint8),
                                np.full(1 if n_records else 0, n_records, dtype=np.int64),
                                np.zeros((0, 5), dtype=np.int64), np.zeros(0, dtype=np.int64)))
                else:
                    out.append(kind.finish())
                    n_host_rows += kind.host_rows
        (barcodes, barcode_counts, barcode_pwm, barcode_other), (umis, umi_counts, umi_pwm, umi_other) = out
        other = int(barcode_other.sum() + umi_other.sum())
        if other:
            sys.stderr.write("FastqMetrics: %d bytes that are none of ACGTN (either case) are in no matrix column\n" % other)
        return FastqMetricsResult(barcodes, barcode_counts, umis, umi_counts, barcode_pwm, umi_pwm, barcode_other,
                                  umi_other, n_records, n_host_rows)
