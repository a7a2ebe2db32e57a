"""
FASTQ records, readers and barcode generators -- the reference's ``sctools.fastq`` (``fastq.py``)
with the same class names and constructors, and the barcode extraction on the GPU
(``libsct_fastq.so``, ``include/sct_fastq.h``).

``Record`` / ``StrRecord``                      one FASTQ record (bytes / str lines)
``Reader``                                      iterates the records of FASTQ file(s)
``EmbeddedBarcode``, ``extract_barcode``        a barcode's position and tags; its slices of a record
``EmbeddedBarcodeGenerator``                    per record, the tags of every embedded barcode
``BarcodeGeneratorWithCorrectedCellBarcodes``   the same, with ``CB`` where the whitelist corrects ``CR``
``TextWindows``, ``extract_spans``              the files' text a window at a time on the GPU; its barcode columns
``bgzf_scan``, ``bgzf_inflate``                 a BGZF file's members; its bytes inflated on the GPU

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
import mmap
import os
import zlib
from collections import namedtuple
from typing import Iterable, Iterator, Optional, Union

import numpy as np

from sctools_amd import _ffi, consts, reader
from sctools_amd.barcode import ErrorsToCorrectBarcodesMap

MAX_SPANS = 4
TILE_BYTES = 16384
SHORT_SEQUENCE, SHORT_QUALITY, BAD_NAME = 1, 2, 4
INDEX_SUFFIX = "_index"  # columns()["CB_index"]: whitelist file index of CB, -1 = no correction


class FastqError(RuntimeError):
    """A libsct_fastq.so call returned an error code (message from sct_fq_last_error)."""


class Span(ctypes.Structure):
    _fields_ = [("start", ctypes.c_int32), ("end", ctypes.c_int32)]


_P = ctypes.POINTER
_vp, _i64, _i32, _int, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_size_t

PROTOTYPES = {
    "sct_fq_last_error": (ctypes.c_char_p, []),
    "sct_fq_workspace_size": (_int, [_i64, _P(_sz)]),
    "sct_fq_count": (_int, [_vp, _i64, _i32, _vp, _sz, _vp, _vp]),
    "sct_fq_extract": (_int, [_vp, _i64, _i64, _vp, _sz, _P(Span), _i32, _P(_vp), _P(_vp), _vp, _vp, _vp]),
}
EXPORTED = tuple(PROTOTYPES)

LIBRARY = _ffi.Library("libsct_fastq.so", "sct_fastq", "sct_fq_last_error", FastqError, PROTOTYPES)
LIB_PATH = LIBRARY.path
load = LIBRARY.load
check = LIBRARY.check

# include/sct_fastq_inflate.h: the same library, a table of its own (PROTOTYPES is what sct_fastq.h declares)
NOT_BGZF = -4
INFLATE_SLACK = 65536
ST_CRC = 10
MEMBER = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("clen", "<u4"), ("isize", "<u4")])
INFLATE_PROTOTYPES = {
    "sct_fq_bgzf_scan": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _P(_i64), _P(_i64)]),
    "sct_fq_crc32": (ctypes.c_uint32, [_vp, _i64]),
    "sct_fq_inflate_workspace_size": (_int, [_i64, _P(_sz)]),
    "sct_fq_inflate": (_int, [_vp, _i64, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _sz, _vp, _vp, _vp]),
}
INFLATE_LIBRARY = _ffi.Library("libsct_fastq.so", "sct_fastq", "sct_fq_last_error", FastqError, INFLATE_PROTOTYPES,
                               shares=LIBRARY)
load_inflate = INFLATE_LIBRARY.load

INFLATE_MODES = ("auto", "host")
DEFAULT_INFLATE = "auto"  # who inflates a BGZF FASTQ: the device, or ("host") Python's gzip as for every other file
_last_error = ""


def last_error() -> str:
    """Why the last :func:`bgzf_inflate` returned None."""
    return _last_error


def check_inflate(inflate: str) -> str:
    if inflate not in INFLATE_MODES:
        raise ValueError("inflate must be one of %s, got %r: there is no device-only mode" % (INFLATE_MODES, inflate))
    return inflate


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


Window = namedtuple("Window", ["text", "n_bytes", "n_records", "workspace", "host"])


class _DeviceWindow(Window):
    """A window with bytes the device inflated: ``host`` is fetched from the device on first use (before the
    next window is asked for), and the fifth item of the tuple is None."""

    def __new__(cls, text, n_bytes, n_records, workspace):
        return super().__new__(cls, text, n_bytes, n_records, workspace, None)

    @property
    def host(self):
        if "_host" not in self.__dict__:
            self.__dict__["_host"] = self.text[:self.n_bytes].cpu().numpy()
        return self.__dict__["_host"]


def bgzf_scan(data):
    """The BGZF members of the file image ``data`` (bytes, mmap or uint8 array), by ``sct_fq_bgzf_scan``:
    ``(members, crcs, stopped_at, reason)`` -- a ``MEMBER`` array (``in_off`` the file offset of the deflate
    data, ``out_off`` the payload bytes before the member), the stored CRC-32 of each, the offset behind the
    last member and None, or ``"not BGZF at byte N"`` where the scan stopped at something else."""
    lib = load_inflate()
    arr = data if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
    size, step = int(arr.size), 1 << 16
    parts, crc_parts, at, out, reason = [], [], 0, 0, None
    while True:
        members, crcs = np.zeros(step, dtype=MEMBER), np.zeros(step, dtype=np.uint32)
        n, stop = ctypes.c_int64(0), ctypes.c_int64(0)
        rc = lib.sct_fq_bgzf_scan(arr.ctypes.data if size else None, size, at, step, members.ctypes.data,
                                  crcs.ctypes.data, ctypes.byref(n), ctypes.byref(stop))
        if rc not in (0, NOT_BGZF):
            INFLATE_LIBRARY.check(rc)
        k = int(n.value)
        members = members[:k]
        members["out_off"] += np.uint64(out)
        parts.append(members)
        crc_parts.append(crcs[:k])
        if k:
            out = int(members["out_off"][-1]) + int(members["isize"][-1])
        at = int(stop.value)
        if rc == NOT_BGZF:
            reason = INFLATE_LIBRARY.last_error()
        if rc == NOT_BGZF or at >= size:
            return np.concatenate(parts), np.concatenate(crc_parts), at, reason


class _HostFile:
    """One file through ``reader.open_binary``; a last line without a newline gets one."""

    kind = "host"

    def __init__(self, path: str, skip: int = 0):
        self.path = path
        self._stream = _ByteStream([path])
        scratch = np.empty(min(max(skip, 1), 1 << 20), dtype=np.uint8)
        while skip > 0:  # (after the device declined the file: on to where its text was good)
            k = self._stream.readinto(scratch[:min(skip, len(scratch))])
            if not k:
                break
            skip -= k

    def readinto(self, view) -> int:
        return self._stream.readinto(view)

    def close(self):
        if self._stream._file is not None:
            self._stream._file.close()


class _BgzfFile:
    """A file that is BGZF from its first byte to its last, mapped: its member table and the next member."""

    kind = "device"

    def __init__(self, path: str, handle, mapped, image, members, crcs):
        self.path, self._handle, self._mapped, self.image = path, handle, mapped, image
        self.members, self.crcs = members, crcs
        self.n, self.at = len(members), 0
        self.starts = members["out_off"].astype(np.int64)  # of the payload, in the file's text
        self.ends = self.starts + members["isize"].astype(np.int64)
        self.newline_due = False

    @classmethod
    def open(cls, path: str):
        """``(file, None)``, or ``(None, reason)`` for a file the host path reads."""
        handle = open(path, "rb")
        try:
            mapped = mmap.mmap(handle.fileno(), 0, access=mmap.ACCESS_READ)
        except (ValueError, OSError):  # an empty file, or one that cannot be mapped
            handle.close()
            return None, "not mapped"
        image = np.frombuffer(mapped, dtype=np.uint8)
        members, crcs, _, reason = bgzf_scan(image)
        self = cls(path, handle, mapped, image, members, crcs)
        full = np.flatnonzero(members["isize"])
        if reason is None and len(full):  # the file's last byte decides whether a newline follows it
            m = members[full[-1]]
            try:
                tail = zlib.decompress(image[int(m["in_off"]):int(m["in_off"]) + int(m["clen"])].tobytes(), -15)
                self.newline_due = tail[-1:] != b"\n"
            except zlib.error as e:
                reason = "the last member does not inflate: %s" % e
        if reason is not None:
            self.close()
            return None, reason
        return self, None

    def take(self, room: int):
        """``(m1, n_bytes)``: members ``[at, m1)`` are the longest run whose ``n_bytes`` of payload fit ``room``."""
        if self.at >= self.n:
            return self.at, 0
        base = int(self.starts[self.at])
        m1 = max(self.at, int(np.searchsorted(self.ends, base + room, side="right")))
        return m1, (int(self.ends[m1 - 1]) - base if m1 > self.at else 0)

    def compressed(self, m0: int, m1: int):
        """File offsets ``[c0, c1)`` that hold the deflate data of members ``[m0, m1)``."""
        last = self.members[m1 - 1]
        return int(self.members[m0]["in_off"]), int(last["in_off"]) + int(last["clen"])

    def close(self):
        self.image = None
        try:
            self._mapped.close()
        except BufferError:  # a view of the map is still alive somewhere: the collector closes it
            pass
        self._handle.close()


class _Inflater:
    """The device buffers of ``sct_fq_inflate``, grown as runs need them and reused from run to run."""

    def __init__(self, dev):
        self.dev, self.lib = dev, load_inflate()
        self.staged = self.comp = self.table = self.work = None

    @staticmethod
    def _room(t, n: int, make):
        return t if t is not None and t.numel() >= n else make(max(n, 1) * 5 // 4 + 64)

    def run(self, source: _BgzfFile, m0: int, m1: int, text, text_off: int, summary):
        """Queues the inflate of members ``[m0, m1)`` into ``text[text_off:]`` on the current stream; returns the
        members' status tensor.  The pinned buffers are free again once the stream has passed the call."""
        import torch

        k = m1 - m0
        c0, c1 = source.compressed(m0, m1)
        c0 -= c0 & 3  # (the run's first word as the file has it, so members keep their alignment)
        n_comp = c1 - c0
        pin = (lambda n: torch.empty(n, dtype=torch.uint8).pin_memory())
        gpu = (lambda n: torch.empty(n, dtype=torch.uint8, device=self.dev))
        self.staged = self._room(self.staged, n_comp, pin)
        self.comp = self._room(self.comp, n_comp + INFLATE_SLACK, gpu)
        self.table = self._room(self.table, 28 * k, pin)
        need = ctypes.c_size_t(0)
        INFLATE_LIBRARY.check(self.lib.sct_fq_inflate_workspace_size(k, ctypes.byref(need)))
        self.work = self._room(self.work, int(need.value) + 8, gpu)
        self.staged.numpy()[:n_comp] = source.image[c0:c1]
        self.comp[:n_comp].copy_(self.staged[:n_comp], non_blocking=True)
        table = self.table.numpy()
        members = table[:24 * k].view(MEMBER)
        members[:] = source.members[m0:m1]
        members["in_off"] -= np.uint64(c0)
        members["out_off"] -= np.uint64(int(source.starts[m0]))
        table[24 * k:28 * k].view(np.uint32)[:] = source.crcs[m0:m1]
        status = torch.empty(max(k, 1), dtype=torch.int32, device=self.dev)
        INFLATE_LIBRARY.check(self.lib.sct_fq_inflate(
            _ffi.ptr(self.comp), n_comp, self.comp.numel(), self.table.data_ptr(), self.table.data_ptr() + 24 * k, k,
            _ffi.ptr(text), text.numel(), text_off, _ffi.ptr(self.work), self.work.numel(), _ffi.ptr(status),
            _ffi.ptr(summary), _ffi.stream(self.dev)))
        return status[:k]


def _status_words(status, first: int) -> str:
    mask = 0
    for st in np.unique(status[status != 0]):
        mask |= 1 << int(st)
    return "status mask 0x%x, first failed member %d" % (mask, first)


def bgzf_inflate(path: str, device=None) -> Optional[bytes]:
    """The inflated bytes of the BGZF file ``path`` from the device path (``sct_fq_inflate``: ``k_inflate`` and
    the CRC kernel), or None with :func:`last_error` saying why: ``not BGZF at byte N``, or the mask of the
    members' status codes (bit ``s`` for status ``s``; bit 10 is a CRC mismatch) and the first failed member."""
    import torch

    global _last_error
    _last_error = ""
    dev = _ffi.device(device)
    source, reason = _BgzfFile.open(path)
    if source is None:
        _last_error = reason
        return None
    try:
        with torch.cuda.device(dev):
            total = int(source.ends[-1]) if source.n else 0
            text = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
            summary = torch.empty(2, dtype=torch.int32, device=dev)
            if source.n:
                status = _Inflater(dev).run(source, 0, source.n, text, 0, summary).cpu().numpy()
                n_bad, first = (int(x) & 0xFFFFFFFF for x in summary.cpu())
                if n_bad or status.any():
                    _last_error = _status_words(status, first)
                    return None
            return text[:total].cpu().numpy().tobytes()
    finally:
        source.close()


class TextWindows:
    """The decompressed text of ``files`` as one stream, a window of whole records at a time on the device.

    Iterating yields ``Window(text, n_bytes, n_records, workspace, host)``: the device tensor whose first
    ``n_bytes`` bytes are the window, the complete records ``sct_fq_count`` found in them, the workspace
    it filled for ``sct_fq_extract`` (:func:`extract_spans`), and the same bytes on the host as a uint8
    array.  What follows a window's last complete record opens the next window; a full window without
    one whole record is doubled.  A window's tensors are overwritten when the next one is asked for.

    ``inflate="auto"``: a file that is BGZF from its first byte to its last is inflated on the device
    (``sct_fq_inflate``): whole members are copied compressed and inflated behind the carry, which moves
    device to device; such a window's ``host`` is fetched from the device when it is first asked for.
    Every other file, and every file with ``inflate="host"``, is read through ``reader.open_binary``.  A
    member the device declines sends its file back to the host reader from its first byte: what that
    raises is the error, and where it raises nothing the stream goes on from the same place on the host.
    ``inflated_by[path]`` is ``"device"`` or ``"host"`` once the file is finished, ``declined[path]`` the
    reason where the device had a file and gave it back.
    """

    def __init__(self, files, device=None, window_bytes: int = 256 << 20, inflate: str = DEFAULT_INFLATE):
        self.files = list(files)
        self.inflate = check_inflate(inflate)
        self.device = _ffi.device(device)
        stored = sum(os.stat(f).st_size for f in self.files)
        self.cap = max(16, min(int(window_bytes), max(8 * stored + 64, 1 << 16)))
        self.inflated_by, self.declined = {}, {}

    def _open(self, path: str):
        if self.inflate == "auto":
            source, _ = _BgzfFile.open(path)
            if source is not None:
                return source
        return _HostFile(path)

    def __iter__(self):
        import torch

        lib, dev, cap = load(), self.device, self.cap
        pending, cur, eof = list(self.files), None, False
        with torch.cuda.device(dev):
            host = torch.empty(cap, dtype=torch.uint8).pin_memory()
            text = torch.empty(cap, dtype=torch.uint8, device=dev)
            result = torch.empty(5, dtype=torch.int64, device=dev)  # sct_fq_result_t, then the inflate's two words
            summary = result[4:].view(torch.int32)
            inflater = None
            fill = 0
            # the carry text[:fill] is on the host (view[:fill]), on the device, or both
            host_valid = dev_valid = True
            try:
                while True:
                    view = host.numpy()
                    pos, was_valid, chunk, progressed = fill, host_valid, None, False
                    ranges = [] if dev_valid or not fill else [(0, fill)]  # of `view`, to be copied to `text`
                    while not eof and chunk is None:
                        if cur is None:
                            if not pending:
                                eof = True
                                break
                            cur = self._open(pending.pop(0))
                        if cur.kind == "host":
                            k = cur.readinto(view[pos:cap]) if pos < cap else -1
                            if k < 0:
                                break  # the window is full
                            if k:
                                if ranges and ranges[-1][1] == pos:
                                    ranges[-1] = (ranges[-1][0], pos + k)
                                else:
                                    ranges.append((pos, pos + k))
                                pos += k
                            else:
                                self.inflated_by[cur.path] = "host"
                                cur.close()
                                cur = None
                            progressed = True
                        elif cur.at < cur.n:
                            m1, k = cur.take(cap - pos)
                            if m1 == cur.at:
                                break  # the next member does not fit behind what the window holds
                            inflater = inflater or _Inflater(dev)
                            status = inflater.run(cur, cur.at, m1, text, pos, summary)
                            chunk = (cur.at, pos, int(cur.starts[cur.at]), status)
                            cur.at = m1
                            pos += k
                            host_valid = False
                            progressed = True  # (a run of empty members is progress too)
                        elif cur.newline_due:
                            if pos == cap:
                                break
                            view[pos] = 10
                            ranges.append((pos, pos + 1))
                            pos += 1
                            cur.newline_due = False
                            progressed = True
                        else:
                            self.inflated_by[cur.path] = "device"
                            cur.close()
                            cur = None
                            progressed = True
                    n_bytes = pos
                    nbytes = ctypes.c_size_t(0)
                    check(lib.sct_fq_workspace_size(n_bytes, ctypes.byref(nbytes)))
                    work = torch.empty(int(nbytes.value) + 8, dtype=torch.uint8, device=dev)
                    if host_valid:
                        text[:n_bytes].copy_(host[:n_bytes], non_blocking=True)
                    else:
                        for a, b in ranges:
                            text[a:b].copy_(host[a:b], non_blocking=True)
                    dev_valid = True
                    check(lib.sct_fq_count(_ffi.ptr(text), n_bytes, 1 if eof else 0, _ffi.ptr(work), work.numel(),
                                           _ffi.ptr(result), _ffi.stream(dev)))
                    fetched = [int(x) for x in result.cpu()]  # the one wait of the window: count and summary
                    n, consumed = fetched[:2]
                    if chunk is not None and fetched[4] & 0xFFFFFFFF:
                        # the device declined a member: the count is void, the window ends where the run began and
                        # the file is the host reader's from its first byte (its exception is the error)
                        m0, pos0, skip, status = chunk
                        reason = _status_words(status.cpu().numpy(), m0 + ((fetched[4] >> 32) & 0xFFFFFFFF))
                        path = cur.path
                        cur.close()
                        cur = None
                        cur = _HostFile(path, skip)
                        self.declined[path] = reason
                        fill, host_valid = pos0, was_valid
                        continue
                    if chunk is not None and cur.at >= cur.n:
                        self.inflated_by[cur.path] = "device"  # its last member passed (a newline may still follow)
                    if n == 0:
                        if eof:
                            break
                        if n_bytes == cap or not progressed:
                            # not one whole record in a full window, or no room for one more member: a larger
                            # window, not a loop
                            cap *= 2
                            bigger = torch.empty(cap, dtype=torch.uint8).pin_memory()
                            if host_valid:
                                bigger[:n_bytes].copy_(host[:n_bytes])
                            host = bigger
                            grown = torch.empty(cap, dtype=torch.uint8, device=dev)
                            grown[:n_bytes].copy_(text[:n_bytes])
                            text = grown
                        fill = n_bytes
                        continue
                    if host_valid:
                        yield Window(text, n_bytes, n, work, view[:n_bytes])
                    else:
                        yield _DeviceWindow(text, n_bytes, n, work)
                    torch.cuda.current_stream(dev).synchronize()  # the copy out of `host` is done before it is refilled
                    fill = n_bytes - consumed
                    if fill and host_valid:
                        view[:fill] = view[consumed:n_bytes].copy()
                        dev_valid = False  # (the next window copies all of `view`, as it always has)
                    elif fill:
                        text[:fill].copy_(text[consumed:n_bytes].clone())  # device to device
                    else:
                        host_valid = True  # no carry: the next window starts clean on either side
                    if eof:
                        break
            finally:
                if cur is not None:
                    cur.close()


def extract_spans(window: Window, spans):
    """The bases and qualities ``[start, end)`` of every record of ``window``, for each ``(start, end)`` of
    ``spans``: ``([(seq, qual) per span], first_flagged, flags)`` -- uint8 ``[n_records, end - start]``
    device tensors, the first record with a flag (-1: none) and the records' flags (``SHORT_SEQUENCE``,
    ``SHORT_QUALITY``, ``BAD_NAME``) as a device tensor; :func:`flag_error` words them."""
    import torch

    lib = load()
    text, n_bytes, n, work, _ = window
    dev = text.device
    columns = []
    with torch.cuda.device(dev):
        result = torch.empty(4, dtype=torch.int64, device=dev)
        flags = torch.empty((n + 3) // 4 * 4, dtype=torch.uint8, device=dev)
        all_flags, first_flagged = None, -1  # over the groups of MAX_SPANS: every call writes `flags` anew
        for g in range(0, len(spans), MAX_SPANS):
            group = spans[g:g + MAX_SPANS]
            c_spans = (Span * len(group))(*[Span(start, end) for start, end in group])
            seq = [torch.empty((n, end - start), dtype=torch.uint8, device=dev) for start, end in group]
            qual = [torch.empty((n, end - start), dtype=torch.uint8, device=dev) for start, end in group]
            c_seq = (ctypes.c_void_p * len(group))(*[t.data_ptr() for t in seq])
            c_qual = (ctypes.c_void_p * len(group))(*[t.data_ptr() for t in qual])
            check(lib.sct_fq_extract(_ffi.ptr(text), n_bytes, n, _ffi.ptr(work), work.numel(), c_spans, len(group),
                                     c_seq, c_qual, _ffi.ptr(flags), _ffi.ptr(result), _ffi.stream(dev)))
            columns.extend(zip(seq, qual))
            flagged = int(result[3].cpu())
            if flagged >= 0 and (first_flagged < 0 or flagged < first_flagged):
                first_flagged = flagged
            if len(spans) > MAX_SPANS:
                all_flags = flags.clone() if all_flags is None else all_flags | flags
    return columns, first_flagged, flags if all_flags is None else all_flags


def flag_error(window: Window, base: int, r: int, flags, max_end: int) -> ValueError:
    """The ValueError of window record ``r`` (stream record ``base + r``) that ``flags`` flags, where
    ``max_end`` is the largest end of the spans extracted."""
    # a line shorter than one group's largest end is shorter than the largest end of all
    flag = int(flags[r].cpu())
    if flag & BAD_NAME:
        return ValueError("FASTQ name must start with @ (record %d)" % (base + r))
    ends = np.flatnonzero(window.host == 10)
    starts = np.concatenate([[0], ends + 1])
    stops = np.concatenate([ends, [len(window.host)]])
    line, which = (4 * r + 1, "sequence") if flag & SHORT_SEQUENCE else (4 * r + 3, "quality")
    return _short_line_error(base + r, which, int(stops[line] - starts[line]), max_end)


class _DeviceColumns:
    """The device side shared by the two generators: text windows -> barcode columns."""

    def _spans(self):
        raise NotImplementedError

    inflated_by: dict = {}  # after columns(): path -> "device" / "host", as TextWindows.inflated_by
    declined: dict = {}

    def _extract_windows(self, device=None, window_bytes: int = 256 << 20, max_records: Optional[int] = None,
                         inflate: str = DEFAULT_INFLATE):
        """Yields ``(first record index, n, [(seq tensor, qual tensor) per span])`` per window.  With
        ``max_records`` the stream ends after that many records and a bad record from there on is
        never seen, as an iterator that is not advanced past its consumer's last record never sees it."""
        if self._header_comment_char is not None:
            raise ValueError("columns() reads whole files; header_comment_char needs the host iterator")
        spans = [(b.start, b.end) for b in self._spans()]
        if not spans:
            raise ValueError("no embedded barcode: there is no column to extract; iterate on the host")
        for start, end in spans:
            if not (0 <= start < end):
                raise ValueError("barcode [%d, %d) is empty or negative" % (start, end))
        base = 0
        windows = TextWindows(self._files, device, window_bytes, inflate=inflate)
        self.inflated_by, self.declined = windows.inflated_by, windows.declined
        for window in windows:
            columns, first_flagged, flags = extract_spans(window, spans)
            n = window.n_records
            if max_records is not None and base + n >= max_records:
                n = max_records - base  # the rest of the text is nobody's business
                columns = [(seq[:n], qual[:n]) for seq, qual in columns]
                if first_flagged >= n:
                    first_flagged = -1
                if n == 0:
                    break
            if first_flagged >= 0:
                raise flag_error(window, base, first_flagged, flags, max(end for _, end in spans))
            yield base, n, columns
            base += n
            if max_records is not None and base >= max_records:
                break


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

    def columns(self, device=None, window_bytes: int = 256 << 20, max_records: Optional[int] = None,
                inflate: str = DEFAULT_INFLATE):
        """Per window of at most ``window_bytes`` of decompressed text, a dict ``tag -> uint8 [n, L]``
        tensor on the device, in the order the host iterator lists the tags.  ``max_records`` ends the
        stream after that many records; what follows them is neither extracted nor checked.  ``inflate``
        is ``TextWindows``'s: ``"auto"`` inflates BGZF files on the device, ``"host"`` none; ``inflated_by``
        then says per file which it was."""
        check_inflate(inflate)
        for _, _, cols in self._extract_windows(device, window_bytes, max_records, inflate):
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

    def columns(self, device=None, window_bytes: int = 256 << 20, max_records: Optional[int] = None,
                inflate: str = DEFAULT_INFLATE):
        """As :meth:`EmbeddedBarcodeGenerator.columns`, with ``CB`` after the cell barcode's two tags: the
        corrected bytes (the raw bytes where there is no correction) and, under ``"CB_index"``, the
        int32 whitelist file index, -1 where the record gets no ``CB``."""
        if not self.supports_columns:
            raise ValueError("the cell barcode's length differs from the whitelist's, or there is a "
                             "header_comment_char: iterate on the host")
        check_inflate(inflate)
        key = consts.CELL_BARCODE_TAG_KEY
        for _, _, cols in self._extract_windows(device, window_bytes, max_records, inflate):
            out = {}
            for k, (b, (seq, qual)) in enumerate(zip(self._spans(), cols)):
                out[b.sequence_tag] = seq
                out[b.quality_tag] = qual
                if k == 0:
                    out[key + INDEX_SUFFIX], out[key] = self._error_mapping.correct_barcodes(seq, return_corrected=True)
            index = out.pop(key + INDEX_SUFFIX)
            out[key + INDEX_SUFFIX] = index  # listed last: it is no tag
            yield out
