"""
FASTQ records, readers and barcode generators -- the reference's ``sctools.fastq`` (``fastq.py``)
with the same class names and constructors, and the barcode extraction on the GPU
(``libsct_fastq.so``, ``include/sct_fastq.h``).

``Record`` / ``StrRecord``                      one FASTQ record (bytes / str lines)
``Reader``                                      iterates the records of FASTQ file(s)
``EmbeddedBarcode``, ``extract_barcode``        a barcode's position and tags; its slices of a record
``EmbeddedBarcodeGenerator``                    per record, the tags of every embedded barcode
``BarcodeGeneratorWithCorrectedCellBarcodes``   the same, with ``CB`` where the whitelist corrects ``CR``

Iterated on the host, the generators yield what the reference's yield: one list of
``(tag, value, "Z")`` per record.  Their device method ``columns()`` yields the same values a
window of text at a time as ``uint8 [n, L]`` tensors: the decompressed text is copied to the GPU,
``sct_fq_count`` / ``sct_fq_extract`` cut it into barcode columns, and the cell barcode column goes
to ``ErrorsToCorrectBarcodesMap.correct_barcodes`` without leaving the device.

One deliberate departure: a sequence or quality line shorter than a
barcode's ``end`` raises ``ValueError`` on both paths, where the reference slices the line with
its newline and hands on a tag value that holds a newline.
"""
import ctypes
import os
from collections import namedtuple
from typing import Iterable, Iterator, Optional, Union

import numpy as np

from sctools_amd import consts, reader
from sctools_amd.barcode import ErrorsToCorrectBarcodesMap

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsct_fastq.so")

MAX_SPANS = 4
TILE_BYTES = 16384
SHORT_SEQUENCE, SHORT_QUALITY, BAD_NAME = 1, 2, 4
INDEX_SUFFIX = "_index"  # columns()["CB_index"]: whitelist file index of CB, -1 = no correction

EXPORTED = ("sct_fq_last_error", "sct_fq_workspace_size", "sct_fq_count", "sct_fq_extract")

_lib: Optional[ctypes.CDLL] = None


class FastqError(RuntimeError):
    """A libsct_fastq.so call returned an error code (message from sct_fq_last_error)."""


class Span(ctypes.Structure):
    _fields_ = [("start", ctypes.c_int32), ("end", ctypes.c_int32)]


def load() -> ctypes.CDLL:
    """Load the HIP FASTQ library; raise loudly if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("sctools_amd fastq library not built (%s missing); run `python -c "
                          "'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    L.sct_fq_last_error.restype = ctypes.c_char_p
    L.sct_fq_last_error.argtypes = []
    L.sct_fq_workspace_size.restype = ctypes.c_int
    L.sct_fq_workspace_size.argtypes = [i64, ctypes.POINTER(ctypes.c_size_t)]
    L.sct_fq_count.restype = ctypes.c_int
    L.sct_fq_count.argtypes = [vp, i64, i32, vp, ctypes.c_size_t, vp, vp]
    L.sct_fq_extract.restype = ctypes.c_int
    L.sct_fq_extract.argtypes = [vp, i64, i64, vp, ctypes.c_size_t, ctypes.POINTER(Span), i32, ctypes.POINTER(vp),
                                 ctypes.POINTER(vp), vp, vp, vp]
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != 0:
        raise FastqError("sct_fastq error %d: %s" % (rc, load().sct_fq_last_error().decode("utf-8", "replace")))


class Record:
    """A FASTQ record of four bytes lines: name, sequence, name2, quality."""

    __slots__ = ["_name", "_sequence", "_name2", "_quality"]
    _at = b"@"

    def __init__(self, record: Iterable):
        self.name, self.sequence, self.name2, self.quality = record

    @staticmethod
    def _line(value, what: str):
        if not isinstance(value, (bytes, str)):
            raise TypeError("FASTQ %s must be str or bytes" % what)
        return value

    @property
    def name(self):
        return self._name

    @name.setter
    def name(self, value):
        if not isinstance(value, (bytes, str)):
            raise TypeError("FASTQ name must be bytes")
        if not value.startswith(self._at):  # (a str name of a bytes Record is a TypeError here, as in the reference)
            raise ValueError("FASTQ name must start with @")
        self._name = value

    @property
    def sequence(self):
        return self._sequence

    @sequence.setter
    def sequence(self, value):
        self._sequence = self._line(value, "sequence")

    @property
    def name2(self):
        return self._name2

    @name2.setter
    def name2(self, value):
        self._name2 = self._line(value, "name2")

    @property
    def quality(self):
        return self._quality

    @quality.setter
    def quality(self, value):
        self._quality = self._line(value, "quality")

    def _lines(self):
        return (self.name, self.sequence, self.name2, self.quality)

    def __bytes__(self):
        return b"".join(self._lines())

    def __str__(self):
        return bytes(self).decode()

    def __repr__(self):
        return "Name: %s\nSequence: %s\nName2: %s\nQuality: %s\n" % self._lines()

    def __len__(self):
        return len(self.sequence)

    def average_quality(self) -> float:
        """Mean Phred quality (offset 33) of the quality line without its last byte, the newline."""
        return sum(self.quality[:-1]) / (len(self.quality) - 1) - 33


class StrRecord(Record):
    """A FASTQ record of four str lines."""

    _at = "@"

    def __bytes__(self):
        return "".join(self._lines()).encode()

    def __str__(self):
        return "".join(self._lines())

    def average_quality(self) -> float:
        scores = self.quality[:-1].encode()
        return sum(scores) / len(scores) - 33


class Reader(reader.Reader):
    """Iterates FASTQ file(s) four lines at a time: ``StrRecord`` in mode ``'r'``, ``Record`` in ``'rb'``.
    A trailing group of fewer than four lines is dropped."""

    @staticmethod
    def _record_grouper(iterable):
        return zip(*([iter(iterable)] * 4))

    def __iter__(self) -> Iterator[Record]:
        record_type = StrRecord if self._mode == "r" else Record
        for lines in self._record_grouper(super().__iter__()):
            yield record_type(lines)

    def _checked_records(self):
        """The records with their index; a bad name line names its record."""
        record_type = StrRecord if self._mode == "r" else Record
        for i, lines in enumerate(self._record_grouper(reader.Reader.__iter__(self))):
            try:
                yield i, record_type(lines)
            except ValueError as e:
                raise ValueError("%s (record %d)" % (e, i)) from None


EmbeddedBarcode = namedtuple("Tag", ["start", "end", "sequence_tag", "quality_tag"])


def extract_barcode(record, embedded_barcode):
    """``((sequence_tag, bases, 'Z'), (quality_tag, qualities, 'Z'))`` of one embedded barcode."""
    cut = slice(embedded_barcode.start, embedded_barcode.end)
    return ((embedded_barcode.sequence_tag, record.sequence[cut], "Z"),
            (embedded_barcode.quality_tag, record.quality[cut], "Z"))


def _line_length(line) -> int:
    newline = "\n" if isinstance(line, str) else b"\n"
    return len(line) - (1 if line.endswith(newline) else 0)


def _short_line_error(index: int, which: str, length: int, end: int) -> ValueError:
    return ValueError("FASTQ record %d: the %s line has %d bytes, shorter than the barcode end %d"
                      % (index, which, length, end))


def _check_lengths(index: int, record, max_end: int) -> None:
    for which, line in (("sequence", record.sequence), ("quality", record.quality)):
        if _line_length(line) < max_end:
            raise _short_line_error(index, which, _line_length(line), max_end)


class _ByteStream:
    """The decompressed bytes of several files as one stream.  A file that does not end in a newline
    gets one, so its last line does not run into the next file's first."""

    def __init__(self, files):
        self._names = list(files)
        self._file = None
        self._last = 10
        self._newline_due = False
        self.ended = False

    def readinto(self, view) -> int:
        """Reads up to ``len(view)`` bytes into the uint8 array ``view``; 0 only at the stream's end."""
        while len(view):
            if self._newline_due:
                view[0] = 10
                self._newline_due = False
                return 1
            if self._file is None:
                if not self._names:
                    self.ended = True
                    return 0
                self._file = reader.open_binary(self._names.pop(0))
                self._last = 10
            k = self._file.readinto(memoryview(view))
            if k:
                self._last = int(view[k - 1])
                return k
            self._file.close()
            self._file = None
            self._newline_due = self._last != 10
        return 0


class _DeviceColumns:
    """The device side shared by the two generators: text windows -> barcode columns."""

    def _spans(self):
        raise NotImplementedError

    def _fill(self, view, stream) -> int:
        """Reads into ``view`` until it is full or the stream ends; returns the bytes read."""
        got = 0
        while got < len(view):
            k = stream.readinto(view[got:])
            if not k:
                break
            got += k
        return got

    def _extract_windows(self, device=None, window_bytes: int = 256 << 20, max_records: Optional[int] = None):
        """Yields ``(first record index, n, [(seq tensor, qual tensor) per span])`` per window.  With
        ``max_records`` the stream ends after that many records and a bad record from there on is
        never seen, as an iterator that is not advanced past its consumer's last record never sees it."""
        import torch

        from sctools_amd import barcode as _barcode

        if self._header_comment_char is not None:
            raise ValueError("columns() reads whole files; header_comment_char needs the host iterator")
        spans = list(self._spans())
        if not spans:
            raise ValueError("no embedded barcode: there is no column to extract; iterate on the host")
        for b in spans:
            if not (0 <= b.start < b.end):
                raise ValueError("barcode [%d, %d) is empty or negative" % (b.start, b.end))
        max_end = max(b.end for b in spans)
        lib = load()
        dev = _barcode._device(device)
        stored = sum(os.stat(f).st_size for f in self._files)
        cap = max(16, min(int(window_bytes), max(8 * stored + 64, 1 << 16)))

        stream = _ByteStream(self._files)
        with torch.cuda.device(dev):
            host = torch.empty(cap, dtype=torch.uint8).pin_memory()
            text = torch.empty(cap, dtype=torch.uint8, device=dev)
            result = torch.empty(4, dtype=torch.int64, device=dev)
            fill, base, eof = 0, 0, False
            while True:
                view = host.numpy()
                got = self._fill(view[fill:cap], stream)
                n_bytes = fill + got
                eof = stream.ended
                nbytes = ctypes.c_size_t(0)
                check(lib.sct_fq_workspace_size(n_bytes, ctypes.byref(nbytes)))
                work = torch.empty(int(nbytes.value) + 8, dtype=torch.uint8, device=dev)
                text[:n_bytes].copy_(host[:n_bytes], non_blocking=True)
                s = _barcode._stream(dev)
                check(lib.sct_fq_count(_barcode._ptr(text), n_bytes, 1 if eof else 0, ctypes.c_void_p(work.data_ptr()),
                                       work.numel(), ctypes.c_void_p(result.data_ptr()), s))
                n, consumed = (int(x) for x in result[:2].cpu())
                if n == 0:
                    if eof:
                        break
                    if n_bytes == cap:  # not one whole record in a full window: a larger window, not a loop
                        cap *= 2
                        bigger = torch.empty(cap, dtype=torch.uint8).pin_memory()
                        bigger[:n_bytes].copy_(host[:n_bytes])
                        host = bigger
                        text = torch.empty(cap, dtype=torch.uint8, device=dev)
                    fill = n_bytes
                    continue
                columns = []
                flags = torch.empty((n + 3) // 4 * 4, dtype=torch.uint8, device=dev)
                all_flags, first_flagged = None, -1  # over the groups of MAX_SPANS: every call writes `flags` anew
                for g in range(0, len(spans), MAX_SPANS):
                    group = spans[g:g + MAX_SPANS]
                    c_spans = (Span * len(group))(*[Span(b.start, b.end) for b in group])
                    seq = [torch.empty((n, b.end - b.start), dtype=torch.uint8, device=dev) for b in group]
                    qual = [torch.empty((n, b.end - b.start), dtype=torch.uint8, device=dev) for b in group]
                    c_seq = (ctypes.c_void_p * len(group))(*[t.data_ptr() for t in seq])
                    c_qual = (ctypes.c_void_p * len(group))(*[t.data_ptr() for t in qual])
                    check(lib.sct_fq_extract(_barcode._ptr(text), n_bytes, n, ctypes.c_void_p(work.data_ptr()),
                                             work.numel(), c_spans, len(group), c_seq, c_qual,
                                             ctypes.c_void_p(flags.data_ptr()), ctypes.c_void_p(result.data_ptr()), s))
                    columns.extend(zip(seq, qual))
                    flagged = int(result[3].cpu())
                    if flagged >= 0 and (first_flagged < 0 or flagged < first_flagged):
                        first_flagged = flagged
                    if len(spans) > MAX_SPANS:
                        all_flags = flags.clone() if all_flags is None else all_flags | flags
                if max_records is not None and base + n >= max_records:
                    n, eof = max_records - base, True  # the rest of the text is nobody's business
                    columns = [(seq[:n], qual[:n]) for seq, qual in columns]
                    if first_flagged >= n:
                        first_flagged = -1
                    if n == 0:
                        break
                if first_flagged >= 0:
                    # a line shorter than one group's largest end is shorter than the largest end of all
                    flag = int((flags if all_flags is None else all_flags)[first_flagged].cpu())
                    raise self._flag_error(view[:n_bytes], base, first_flagged, flag, max_end)
                yield base, n, columns
                base += n
                torch.cuda.current_stream(dev).synchronize()  # the copy out of `host` is done before it is refilled
                fill = n_bytes - consumed
                if fill:
                    view[:fill] = view[consumed:n_bytes].copy()
                if eof:
                    break

    @staticmethod
    def _flag_error(window: np.ndarray, base: int, r: int, flag: int, max_end: int) -> ValueError:
        """The ValueError of window record ``r`` (stream record ``base + r``) whose flags are ``flag``."""
        ends = np.flatnonzero(window == 10)
        starts = np.concatenate([[0], ends + 1])
        stops = np.concatenate([ends, [len(window)]])
        if flag & BAD_NAME:
            return ValueError("FASTQ name must start with @ (record %d)" % (base + r))
        line, which = (4 * r + 1, "sequence") if flag & SHORT_SEQUENCE else (4 * r + 3, "quality")
        return _short_line_error(base + r, which, int(stops[line] - starts[line]), max_end)


class EmbeddedBarcodeGenerator(Reader, _DeviceColumns):
    """Per FASTQ record, the sequence and quality tags of every barcode in ``embedded_barcodes``.

    Parameters
    ----------
    fastq_files : str or list of str
    embedded_barcodes : Iterable[EmbeddedBarcode]
    mode : {'r', 'rb'}, optional
    """

    def __init__(self, fastq_files, embedded_barcodes, *args, **kwargs):
        super().__init__(files=fastq_files, *args, **kwargs)
        self.embedded_barcodes = embedded_barcodes

    @property
    def supports_columns(self) -> bool:
        """False with a ``header_comment_char`` (skipping header lines is the host iterator's) and with no
        embedded barcode at all (the host iterator then yields an empty tag list per record, as the
        reference's does for ``AttachBarcodes`` without a cell or molecule barcode)."""
        try:
            n_barcodes = len(self.embedded_barcodes)
        except TypeError:  # an iterable without a length is left to the host iterator, untouched
            return False
        return self._header_comment_char is None and n_barcodes > 0

    def __iter__(self):
        max_end = max((b.end for b in self.embedded_barcodes), default=0)
        for i, record in self._checked_records():
            _check_lengths(i, record, max_end)
            tags = []
            for barcode in self.embedded_barcodes:
                tags.extend(extract_barcode(record, barcode))
            yield tags

    def _spans(self):
        return list(self.embedded_barcodes)

    def columns(self, device=None, window_bytes: int = 256 << 20, max_records: Optional[int] = None):
        """Per window of at most ``window_bytes`` of decompressed text, a dict ``tag -> uint8 [n, L]``
        tensor on the device, in the order the host iterator lists the tags.  ``max_records`` ends the
        stream after that many records; what follows them is neither extracted nor checked."""
        for _, _, cols in self._extract_windows(device, window_bytes, max_records):
            out = {}
            for b, (seq, qual) in zip(self._spans(), cols):
                out[b.sequence_tag] = seq
                out[b.quality_tag] = qual
            yield out


class BarcodeGeneratorWithCorrectedCellBarcodes(Reader, _DeviceColumns):
    """Per FASTQ record, the tags of the cell barcode, ``CB`` where the whitelist holds the raw barcode
    or one within Hamming distance 1 of it, and the tags of the other barcodes.

    Parameters
    ----------
    fastq_files : str or list of str
    embedded_cell_barcode : EmbeddedBarcode
    whitelist : str
        text file, one barcode per line
    other_embedded_barcodes : list or tuple of EmbeddedBarcode, optional
    mode : {'r', 'rb'}, optional
    """

    def __init__(self, fastq_files: Union[str, Iterable[str]], embedded_cell_barcode: EmbeddedBarcode, whitelist: str,
                 other_embedded_barcodes: Iterable[EmbeddedBarcode] = tuple(), *args, **kwargs):
        super().__init__(files=fastq_files, *args, **kwargs)
        if not isinstance(other_embedded_barcodes, (list, tuple)):
            raise TypeError("if passed, other_embedded_barcodes must be a list or tuple")
        self.embedded_barcodes = other_embedded_barcodes
        self._error_mapping = ErrorsToCorrectBarcodesMap.single_hamming_errors_from_whitelist(whitelist)
        self.embedded_cell_barcode = embedded_cell_barcode

    def __iter__(self):
        max_end = max(b.end for b in self._spans())
        for i, record in self._checked_records():
            _check_lengths(i, record, max_end)
            tags = list(self.extract_cell_barcode(record, self.embedded_cell_barcode))
            for barcode in self.embedded_barcodes:
                tags.extend(extract_barcode(record, barcode))
            yield tags

    def extract_cell_barcode(self, record, cb: EmbeddedBarcode):
        """The cell barcode's sequence and quality tags, followed by the ``CB`` tag where
        ``get_corrected_barcode`` has an answer for the raw sequence."""
        seq_tag, qual_tag = extract_barcode(record, cb)
        try:
            corrected = self._error_mapping.get_corrected_barcode(seq_tag[1])
        except KeyError:
            return seq_tag, qual_tag
        return seq_tag, qual_tag, (consts.CELL_BARCODE_TAG_KEY, corrected, "Z")

    def _spans(self):
        return [self.embedded_cell_barcode] + list(self.embedded_barcodes)

    @property
    def supports_columns(self) -> bool:
        """False where the cell barcode's length is not the whitelist's: the answer is then whatever the
        reference's dict of odd whitelist lines gives, of any length, and the host iterator gives it."""
        cb = self.embedded_cell_barcode
        return cb.end - cb.start == self._error_mapping.barcode_length and self._header_comment_char is None

    def columns(self, device=None, window_bytes: int = 256 << 20, max_records: Optional[int] = None):
        """As :meth:`EmbeddedBarcodeGenerator.columns`, with ``CB`` after the cell barcode's two tags: the
        corrected bytes (the raw bytes where there is no correction) and, under ``"CB_index"``, the
        int32 whitelist file index, -1 where the record gets no ``CB``."""
        if not self.supports_columns:
            raise ValueError("the cell barcode's length differs from the whitelist's, or there is a "
                             "header_comment_char: iterate on the host")
        key = consts.CELL_BARCODE_TAG_KEY
        for _, _, cols in self._extract_windows(device, window_bytes, max_records):
            out = {}
            for k, (b, (seq, qual)) in enumerate(zip(self._spans(), cols)):
                out[b.sequence_tag] = seq
                out[b.quality_tag] = qual
                if k == 0:
                    out[key + INDEX_SUFFIX], out[key] = self._error_mapping.correct_barcodes(seq, return_corrected=True)
            index = out.pop(key + INDEX_SUFFIX)
            out[key + INDEX_SUFFIX] = index  # listed last: it is no tag
            yield out
