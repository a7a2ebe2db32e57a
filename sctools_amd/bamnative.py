"""
ctypes binding of ``libsct_bam.so`` (``include/sct_bam.h``): the native BAM -> columns decoder.

It replaces the per-record pysam reads of the reference's aggregation loop
(``aggregator.py:251-334, 507-530``) for ``GatherCellMetrics`` /
``GatherGeneMetrics`` on BAM input: BGZF blocks inflate and records parse on all
cores, and CB / UB / GE are dictionary-encoded natively.  Validation and the
exception classes are those of :func:`sctools_amd.columnar.columnarize` (the
first offending record in file order decides), which the tests check against
the pure-Python decoder on every fixture.
"""
import ctypes
import os
from typing import Optional

import numpy as np

from sctools_amd import _ffi

OK, EIO, EFORMAT = 0, -1, -2
KEYERROR, TYPEERROR, ZERODIV, VALUEERROR, EMPTY, MISSING_TAG, ETYPED = -10, -11, -12, -13, -14, -15, -16


class TypedTagValue(Exception):
    """A dictionary tag holds a float or array value (or, for the sort keys, an integer): the native
    decoder cannot key it as the Python reader does, so the caller decodes with the Python reader
    (include/sct_bam.h SCT_BAM_ETYPED)."""
CELL_METRICS, GENE_METRICS, COUNT_MATRIX, SORT_KEYS, TAGSORT = 0, 1, 2, 3, 4
_MODES = {"cell": CELL_METRICS, "gene": GENE_METRICS, "count": COUNT_MATRIX, "sortkeys": SORT_KEYS,
          "tagsort": TAGSORT}

_P = ctypes.POINTER
_vp, _i32, _i64, _int, _str = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int, ctypes.c_char_p

PROTOTYPES = {
    "sct_bam_decode": (_int, [_str, _i32, _i32, _P(_vp), _P(_i64)]),
    "sct_bam_decode_tags": (_int, [_str, _i32, _str, _i32, _P(_vp), _P(_i64)]),
    "sct_bam_last_error": (_str, []),
    "sct_bam_n": (_i64, [_vp]),
    "sct_bam_column": (_vp, [_vp, _str]),
    "sct_bam_dictionary": (_int, [_vp, _i32, _P(_i64), _P(_vp), _P(_vp), _P(_i32)]),
    "sct_bam_close": (None, [_vp]),
    "sct_bam_split": (_int, [_P(_str), _i32, _str, _str, _i32, _i32, _i32, _i32, _i32, _P(_i32), _P(_i64)]),
    "sct_bam_write_order": (_int, [_str, _str, _vp, _i64, _i32, _i32]),
    "sct_bam_tag_collect": (_int, [_str, _str, _str, _i32, _i32, _P(_vp), _P(_i64)]),
    "sct_bam_tag_n": (_i64, [_vp]),
    "sct_bam_tag_values": (_vp, [_vp]),
    "sct_bam_tag_others": (_int, [_vp, _P(_i64), _P(_vp), _P(_vp), _P(_vp)]),
    "sct_bam_tag_write": (_int, [_vp, _str, _str, _vp, _str, _vp, _i32, _i32]),
    "sct_bam_tag_close": (None, [_vp]),
    "sct_bam_attach_open": (_int, [_str, _str, _i32, _i32, _P(_vp)]),
    "sct_bam_attach_n": (_i64, [_vp]),
    "sct_bam_attach_write": (_int, [_vp, _i64, _i32, _str, _P(_vp), _P(_i64), _P(_vp), _P(_i64)]),
    "sct_bam_attach_close": (_int, [_vp]),
    "sct_bam_shards_open": (_int, [_P(_str), _P(_str), _i32, _i32, _i32, _P(_vp)]),
    "sct_bam_shards_append": (_int, [_vp, _vp, _P(_i64)]),
    "sct_bam_shards_close": (_int, [_vp]),
    "sct_bam_shards_abort": (None, [_vp]),
}
EXPORTED = tuple(PROTOTYPES)

# a return code is the reference's exception class for the first offending record; the message stands alone
_EXC = {KEYERROR: KeyError, TYPEERROR: TypeError, ZERODIV: ZeroDivisionError, VALUEERROR: ValueError,
        EMPTY: RuntimeError, EFORMAT: ValueError, EIO: OSError, MISSING_TAG: RuntimeError, ETYPED: TypedTagValue}

LIBRARY = _ffi.Library("libsct_bam.so", "sct_bam", "sct_bam_last_error", RuntimeError, PROTOTYPES, exceptions=_EXC)
LIB_PATH = LIBRARY.path
load = LIBRARY.load
check = LIBRARY.check
available = LIBRARY.available


def decode(path: str, metric_mode: str = "cell", threads: int = 0, tags=("CB", "UB", "GE")):
    """(arrays, [cell names, umi names, gene names]) -- names in id order, None first if present.

    metric_mode "count" (CountMatrix): only cell / umi / gene / xf are meaningful, the three
    dictionary tags are ``tags``, nothing is validated, and ``arrays["qhead"]`` marks the first
    record of each run of equal query names.

    metric_mode "sortkeys" (TagSortBam / VerifyBamSort): cell / umi / gene are the ranks of the
    three ``tags`` (a missing tag and an empty value both rank first, as "" does),
    ``arrays["qname"]`` the rank of the query name, and a fourth name list holds the query
    names in rank order.

    metric_mode "tagsort" (the native TagSort's per-read rule, :mod:`sctools_amd.tagsort`): ``tags``
    are the barcode, umi and gene tag; a missing tag and the value ``-`` are the None id; nothing
    is validated."""
    from sctools_amd.columnar import COLUMNS, PackedDictionary

    L = load()
    h = ctypes.c_void_p()
    bad = ctypes.c_int64(-1)
    tag_bytes = "".join(tags).encode()
    if len(tag_bytes) != 6 or any(len(t) != 2 for t in tags):
        raise ValueError("tags must be three two-character BAM tag names: %r" % (tags,))
    rc = L.sct_bam_decode_tags(os.fsencode(path), _MODES[metric_mode], tag_bytes, int(threads), ctypes.byref(h),
                               ctypes.byref(bad))
    check(rc)
    try:
        n = int(L.sct_bam_n(h))
        arrays = {}
        extra = {"count": [("qhead", np.uint8)], "sortkeys": [("qname", np.int32)]}
        cols = list(COLUMNS) + extra.get(metric_mode, [])
        for name, dt in cols:
            ptr = L.sct_bam_column(h, name.encode())
            buf = (ctypes.c_char * (n * np.dtype(dt).itemsize)).from_address(ptr) if n else b""
            arrays[name] = np.frombuffer(buf, dtype=dt, count=n).copy()
        names = []
        for which in range(4 if metric_mode == "sortkeys" else 3):
            names.append(PackedDictionary(*_ffi.read_dictionary(L.sct_bam_dictionary, h, which)).names)
        return arrays, names
    finally:
        L.sct_bam_close(h)


def split(in_paths, out_prefix: str, tags, n_subfiles: int, raise_missing: bool = True, level: int = 6,
          threads: int = 0) -> int:
    """sct_bam_split: chunk files ``<out_prefix>_<k>.bam``; returns the number written."""
    L = load()
    for t in tags:
        if len(t) != 2:
            raise ValueError("tags must be two-character BAM tag names: %r" % (tags,))
    arr = (ctypes.c_char_p * len(in_paths))(*[os.fsencode(p) for p in in_paths])
    n_out = ctypes.c_int32(0)
    bad = ctypes.c_int64(-1)
    rc = L.sct_bam_split(arr, len(in_paths), os.fsencode(out_prefix), "".join(tags).encode(), len(tags),
                         int(n_subfiles), 1 if raise_missing else 0, int(level), int(threads), ctypes.byref(n_out),
                         ctypes.byref(bad))
    check(rc)
    return int(n_out.value)


def write_order(in_path: str, out_path: str, perm, level: int = 6, threads: int = 0) -> None:
    """sct_bam_write_order: the records of ``in_path`` in the order ``perm`` (output record k is
    input record perm[k]) under the input's header."""
    L = load()
    p = np.ascontiguousarray(perm, dtype=np.int64)
    rc = L.sct_bam_write_order(os.fsencode(in_path), os.fsencode(out_path), p.ctypes.data if p.size else None,
                               int(p.size), int(level), int(threads))
    check(rc)


class TagColumn:
    """sct_bam_tag_*: the string tag ``src_tag`` of every record of ``path`` as an ``[n, length]`` byte
    column, and the file written back with ``dst_tag`` set from such a column.  A context manager:
    the inflated records are held until it exits."""

    def __init__(self, path: str, src_tag: str, dst_tag: str, length: int, threads: int = 0):
        self._lib = load()
        self._h = ctypes.c_void_p()
        self.length = int(length)
        self.dst_tag = dst_tag
        bad = ctypes.c_int64(-1)
        rc = self._lib.sct_bam_tag_collect(os.fsencode(path), src_tag.encode(), dst_tag.encode(), self.length,
                                           int(threads), ctypes.byref(self._h), ctypes.byref(bad))
        check(rc)
        self.n = int(self._lib.sct_bam_tag_n(self._h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self) -> None:
        if self._h:
            self._lib.sct_bam_tag_close(self._h)
            self._h = ctypes.c_void_p()

    def _bytes(self, ptr, count: int) -> np.ndarray:
        if not count:
            return np.zeros(0, dtype=np.uint8)
        return np.frombuffer((ctypes.c_char * count).from_address(ptr), dtype=np.uint8, count=count).copy()

    def values(self) -> np.ndarray:
        """uint8 [n, length]: the values of exactly ``length`` bytes, zeros for the others."""
        return self._bytes(self._lib.sct_bam_tag_values(self._h), self.n * self.length).reshape(self.n, self.length)

    def others(self):
        """The values of another length, in record order."""
        cnt, rec, by, off = ctypes.c_int64(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        self._lib.sct_bam_tag_others(self._h, ctypes.byref(cnt), ctypes.byref(rec), ctypes.byref(by), ctypes.byref(off))
        k = int(cnt.value)
        offs = np.frombuffer((ctypes.c_int64 * (k + 1)).from_address(off.value), dtype=np.int64)
        raw = ctypes.string_at(by.value, int(offs[-1])) if int(offs[-1]) else b""
        return [raw[offs[i]:offs[i + 1]].decode("utf-8") for i in range(k)]

    def write(self, out_path: str, values: np.ndarray, others=None, level: int = 6, threads: int = 0) -> None:
        """The records to ``out_path`` with ``dst_tag`` set: row i of ``values`` where the record's
        source value fits, else the matching entry of ``others`` (None: its own source value)."""
        v = np.ascontiguousarray(values, dtype=np.uint8)
        if v.shape != (self.n, self.length):
            raise ValueError("values must be [%d, %d], got %s" % (self.n, self.length, v.shape))
        ob, oo = None, None
        if others is not None:
            enc = [s.encode("utf-8") for s in others]
            ob = b"".join(enc)
            oo = np.concatenate([[0], np.cumsum([len(e) for e in enc], dtype=np.int64)]).astype(np.int64)
        rc = self._lib.sct_bam_tag_write(self._h, os.fsencode(out_path), self.dst_tag.encode(),
                                         v.ctypes.data if v.size else None, ob,
                                         oo.ctypes.data if oo is not None else None, int(level), int(threads))
        check(rc)


class TagAttacher:
    """sct_bam_attach_*: the records of ``in_path`` written to ``out_path`` with string tags set from
    byte columns, a window of records at a time (``bam.Tagger.tag``).  A context manager; leaving it
    on an exception removes the partly written output."""

    def __init__(self, in_path: str, out_path: str, level: int = 6, threads: int = 0):
        self._lib = load()
        self._h = ctypes.c_void_p()
        self.out_path = out_path
        rc = self._lib.sct_bam_attach_open(os.fsencode(in_path), os.fsencode(out_path), int(level), int(threads),
                                           ctypes.byref(self._h))
        check(rc)
        self.n = int(self._lib.sct_bam_attach_n(self._h))
        self.written = 0

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self.abort()

    @property
    def remaining(self) -> int:
        return self.n - self.written

    def write(self, columns, n: Optional[int] = None) -> int:
        """``columns`` is a list of ``(tag, values, lengths)``: ``values`` a uint8 ``[n, stride]`` array,
        ``lengths`` an int32 ``[n]`` array (-1: the record does not get the tag) or None for "every
        row is ``stride`` bytes".  Every column has the same n (given as ``n`` when there is no
        column).  Returns the number of records written (fewer than n at the input's end)."""
        keep = []
        for tag, values, lengths in columns:
            if len(tag) != 2:
                raise ValueError("tags are two-character names: %r" % (tag,))
            v = np.ascontiguousarray(values, dtype=np.uint8)
            if v.ndim != 2 or (n is not None and v.shape[0] != n):
                raise ValueError("the values of %s must be [%s, stride], got %s" % (tag, n, v.shape))
            n = v.shape[0]
            ln = None
            if lengths is not None:
                ln = np.ascontiguousarray(lengths, dtype=np.int32)
                if ln.shape != (n,):
                    raise ValueError("the lengths of %s must be [%d], got %s" % (tag, n, ln.shape))
            keep.append((tag, v, ln))
        k = len(keep)
        n = n or 0
        names = "".join(t for t, _, _ in keep).encode("ascii")
        vals = (ctypes.c_void_p * max(k, 1))(*[v.ctypes.data if v.size else None for _, v, _ in keep])
        strides = (ctypes.c_int64 * max(k, 1))(*[v.shape[1] for _, v, _ in keep])
        lens = (ctypes.c_void_p * max(k, 1))(*[ln.ctypes.data if ln is not None and ln.size else None
                                              for _, _, ln in keep])
        done = ctypes.c_int64(0)
        rc = self._lib.sct_bam_attach_write(self._h, n, k, names, vals, strides, lens, ctypes.byref(done))
        check(rc)
        self.written += int(done.value)
        return int(done.value)

    def close(self) -> None:
        if self._h:
            h, self._h = self._h, ctypes.c_void_p()
            rc = self._lib.sct_bam_attach_close(h)
            check(rc)

    def abort(self) -> None:
        """Close and remove the output."""
        if self._h:
            h, self._h = self._h, ctypes.c_void_p()
            self._lib.sct_bam_attach_close(h)
        if os.path.exists(self.out_path):
            os.remove(self.out_path)


class ShardWriter:
    """sct_bam_shards_*: ``paths`` created together and appended to together.  ``headers`` is None or one
    SAM header text (or None) per path: a file with one is a BAM with no references, a file without
    one holds the appended bytes alone (a ``.fastq.gz`` shard).  A context manager; leaving it on an
    exception removes every file."""

    def __init__(self, paths, headers=None, level: int = 6, threads: int = 0):
        self._lib = load()
        self._h = ctypes.c_void_p()
        self.paths = [os.fspath(p) for p in paths]
        n = len(self.paths)
        if headers is not None and len(headers) != n:
            raise ValueError("%d headers for %d paths" % (len(headers), n))
        c_paths = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(p) for p in self.paths])
        c_headers = None
        if headers is not None:
            c_headers = (ctypes.c_char_p * max(n, 1))(*[None if h is None else h.encode("utf-8") for h in headers])
        check(self._lib.sct_bam_shards_open(c_paths, c_headers, n, int(level), int(threads), ctypes.byref(self._h)))

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:
            self.abort()

    def append(self, data, bounds) -> None:
        """``data`` is a contiguous uint8 numpy array; file i gets ``data[bounds[i]:bounds[i + 1]]``."""
        b = np.ascontiguousarray(bounds, dtype=np.int64)
        if b.shape != (len(self.paths) + 1,):
            raise ValueError("bounds must have %d entries, got %s" % (len(self.paths) + 1, b.shape))
        d = np.ascontiguousarray(data, dtype=np.uint8)
        if b[-1] > d.size:
            raise ValueError("the bounds end at %d, the data has %d bytes" % (int(b[-1]), d.size))
        check(self._lib.sct_bam_shards_append(self._h, d.ctypes.data if d.size else None,
                                              b.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))

    def close(self) -> None:
        if self._h:
            h, self._h = self._h, ctypes.c_void_p()
            check(self._lib.sct_bam_shards_close(h))

    def abort(self) -> None:
        """Close and remove every file."""
        if self._h:
            h, self._h = self._h, ctypes.c_void_p()
            self._lib.sct_bam_shards_abort(h)
