"""
ctypes binding of ``libsct_gbam.so`` (``include/sct_gbam.h``): BAM -> columns decoded on the GPU.

The compressed file goes to HBM once; BGZF members inflate one wavefront each, record starts are
found and proven on the device, every record is parsed by one lane and CB / UB / GE are interned
in device hash tables.  The columns stay in HBM as the engine's input tensors; only the distinct
dictionary strings visit the host (to be ranked in Python's ``sorted()`` order).

It stands in for the same reference reads as ``bamnative`` (the per-record pysam loop of
``MetricAggregator.parse_molecule``, ``aggregator.py:251-334``, and
``CellMetrics.parse_extra_fields``, ``aggregator.py:507-530``; in "tagsort" mode the per-read stage of the native TagSort,
``htslib_tagsort.cpp:106-218``).  A file the device path does not
reproduce exactly (a record the reference rejects, typed dictionary tags, non-ASCII dictionary
bytes, a malformed deflate stream, an empty file) returns ``None``: the caller decodes it with
``bamnative``, whose error is the reference's exception for the first offending record.
"""
import ctypes
import os
from typing import Optional

import numpy as np

from sctools_amd import _ffi

OK, HOST = 0, 1
_MODES = {"cell": 0, "gene": 1}
STAGES = ("map_scan", "h2d", "inflate", "record_starts", "parse_intern", "dictionaries", "members",
          "start_rounds")

_P = ctypes.POINTER
_vp, _i32, _i64, _u64, _int = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int

PROTOTYPES = {
    "sct_gbam_open": (_int, [ctypes.c_char_p, _i32, _vp, _P(_vp), _P(_i64)]),
    "sct_gbam_open_part": (_int, [ctypes.c_char_p, _i32, _i32, _i64, _i32, _vp, _P(_vp), _P(_i64)]),
    "sct_gbam_part_bounds": (_int, [_vp, _P(_i64), _P(_i64)]),
    "sct_gbam_merge_dictionaries": (_int, [_P(_vp), _i32, _i32, _P(_P(_i32))]),
    "sct_gbam_remap": (_int, [_vp, _P(_i32), _i64, _vp, _i64]),
    "sct_gbam_parse": (_int, [_vp, _i32, _P(_vp)]),
    "sct_gbam_parse_count": (_int, [_vp, ctypes.c_char_p, _P(_vp)]),
    "sct_gbam_parse_tagsort": (_int, [_vp, ctypes.c_char_p, _P(_vp)]),
    "sct_gbam_dictionary": (_int, [_vp, _i32, _P(_i64), _P(_vp), _P(_vp), _P(_i32)]),
    "sct_gbam_read_inflated": (_int, [_vp, _u64, _u64, _vp, _P(_u64)]),
    "sct_gbam_timing": (_int, [_vp, _P(ctypes.c_double)]),
    "sct_gbam_windows": (_i64, [_vp]),
    "sct_gbam_close": (None, [_vp]),
    "sct_gbam_last_error": (ctypes.c_char_p, []),
}
EXPORTED = tuple(PROTOTYPES)

# HOST is no error: the file goes to the host decoder
LIBRARY = _ffi.Library("libsct_gbam.so", "device BAM decode failed", "sct_gbam_last_error", OSError, PROTOTYPES,
                       env_override="SCT_GBAM_LIB_PATH", accept=(OK, HOST), error_format="%s (%d): %s")
LIB_PATH = LIBRARY.path  # SCT_GBAM_LIB_PATH overrides it: experiments only
load = LIBRARY.load
available = LIBRARY.available
last_error = LIBRARY.last_error
_check = LIBRARY.check
_device = _ffi.device


class _Handle:
    def __init__(self, path: str, device, part: int = 0, n_parts: int = 1, first_start: int = -1):
        self.L = load()
        self.dev = _device(device)
        self.h = ctypes.c_void_p()
        n = ctypes.c_int64(0)
        self.rc = self.L.sct_gbam_open_part(os.fsencode(path), int(part), int(n_parts), int(first_start),
                                            int(self.dev.index), _ffi.stream(self.dev),
                                            ctypes.byref(self.h), ctypes.byref(n))
        self.err = last_error()  # (thread-local in the library: read on the calling thread)
        self.n = int(n.value)

    def check_open(self):
        """Raises what the open returned, with the message read on the thread that opened."""
        _check(self.rc, self.err)

    def bounds(self):
        a, b = ctypes.c_int64(), ctypes.c_int64()
        _check(self.L.sct_gbam_part_bounds(self.h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def dictionary_size(self, which: int) -> int:
        """Entries of dictionary ``which`` (the count alone: no copy of its strings)."""
        return len(_ffi.read_dictionary(self.L.sct_gbam_dictionary, self.h, which, strings=False)[1]) - 1

    def dictionary(self, which: int, lazy: bool = True):
        from sctools_amd.columnar import PackedDictionary

        packed = PackedDictionary(*_ffi.read_dictionary(self.L.sct_gbam_dictionary, self.h, which))
        return packed if lazy else packed.names

    def close(self):
        if self.h:
            self.L.sct_gbam_close(self.h)
            self.h = ctypes.c_void_p()

    def timing(self):
        t = (ctypes.c_double * 8)()
        self.L.sct_gbam_timing(self.h, t)
        out = dict(zip(STAGES, list(t)))
        out["windows"] = int(self.L.sct_gbam_windows(self.h))
        return out


COUNT_COLUMNS = ("cell", "umi", "gene", "xf", "qhead")


def decode(path: str, metric_mode: str = "cell", device=None, timings: Optional[dict] = None,
           lazy: bool = False, tags=None):
    """(device column tensors, [cell names, umi names, gene names]) -- or None when the file needs
    the host decoder.  Names in id order, None first when a record lacks the tag; with ``lazy``
    each dictionary is a ``columnar.PackedDictionary`` (strings decoded only when asked for).

    ``metric_mode`` "count": the count-matrix columns ``COUNT_COLUMNS`` of the three tags named by
    ``tags`` (cell, molecule, gene), as ``bamnative.decode(path, "count", tags=tags)``.

    ``metric_mode`` "tagsort": the record columns under the native TagSort's per-read rule for the
    three tags named by ``tags`` (barcode, umi, gene), as ``bamnative.decode(path, "tagsort",
    tags=tags)``."""
    import torch

    from sctools_amd import _native as N
    from sctools_amd.engine import TORCH_DTYPES

    H = _Handle(path, device)
    try:
        H.check_open()
        if H.rc == HOST:
            return None
        if metric_mode in ("count", "tagsort") and (tags is None or len(tags) != 3 or any(len(t) != 2 for t in tags)):
            raise ValueError("%s mode needs three 2-character tag names" % metric_mode)
        names_ = COUNT_COLUMNS if metric_mode == "count" else N.RECORD_COLUMNS
        try:  # columns that do not fit the device: the host decoder takes the file
            if metric_mode == "count":
                cols = {c: torch.empty(H.n, dtype=torch.int32 if c in ("cell", "umi", "gene") else torch.uint8,
                                       device=H.dev) for c in COUNT_COLUMNS}
            else:
                cols = {c: torch.empty(H.n, dtype=TORCH_DTYPES[c], device=H.dev) for c in N.RECORD_COLUMNS}
        except torch.cuda.OutOfMemoryError:
            return None
        ptrs = (ctypes.c_void_p * len(names_))(*[cols[c].data_ptr() for c in names_])
        if metric_mode == "count":
            rc = H.L.sct_gbam_parse_count(H.h, "".join(tags).encode("ascii"), ptrs)
        elif metric_mode == "tagsort":
            rc = H.L.sct_gbam_parse_tagsort(H.h, "".join(tags).encode("ascii"), ptrs)
        else:
            rc = H.L.sct_gbam_parse(H.h, _MODES[metric_mode], ptrs)
        _check(rc)
        if rc == HOST:
            return None
        names = [H.dictionary(which, lazy) for which in range(3)]
        if timings is not None:
            timings.update(H.timing())
        return cols, names
    finally:
        H.close()


def inflate(path: str, device=None) -> Optional[bytes]:
    """The concatenated BGZF payload as the device inflated it (tests compare it with zlib), or
    None when the device path declines the file."""
    H = _Handle(path, device)
    try:
        H.check_open()
        if H.rc == HOST:
            return None
        total = ctypes.c_uint64(0)
        H.L.sct_gbam_read_inflated(H.h, 0, 0, None, ctypes.byref(total))
        buf = ctypes.create_string_buffer(int(total.value))
        rc = H.L.sct_gbam_read_inflated(H.h, 0, int(total.value), buf, None)
        _check(rc)
        return buf.raw
    finally:
        H.close()


def decode_parts(path: str, metric_mode: str, devices, timings: Optional[dict] = None):
    """One file decoded by several devices together (``GatherCellMetrics(devices=N)``): part p of
    len(devices) -- a byte-balanced range of BGZF members and the records starting in them -- is
    inflated, parsed and interned on devices[p] (``sct_gbam_open_part``), so no device holds the
    whole file.  The parts' record starts are checked against each other (part p's first record is
    the landing of part p-1's walk; a part that guessed wrong is reopened there), their dictionaries
    merged into the global ranked ones and every part's ids renumbered on its device.

    Returns (per-part column dicts on their devices, [cells, umis, genes] ``PackedDictionary``) --
    records in file order, part after part -- or None when the file needs the host decoder."""
    import threading

    import torch

    from sctools_amd import _native as N
    from sctools_amd.engine import TORCH_DTYPES

    if metric_mode not in _MODES:
        raise ValueError("decode_parts reads the cell and gene metric modes")
    devs = [_device(d) for d in devices]
    P = len(devs)
    hs: list = [None] * P
    errs: list = [None] * P

    def each(fn):
        def work(p):
            try:
                with torch.cuda.device(devs[p]):
                    fn(p)
            except BaseException as e:  # noqa: BLE001 -- re-raised below
                errs[p] = e

        th = [threading.Thread(target=work, args=(p,)) for p in range(P)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for e in errs:
            if e is not None:
                raise e

    def close_all():
        for h in hs:
            if h is not None:
                h.close()

    try:
        def open_one(p):
            hs[p] = _Handle(path, devs[p], p, P)

        each(open_one)
        for h in hs:
            h.check_open()
        if hs[0].rc == HOST:
            return None
        # part p starts where part p-1's walk lands: a part whose own guess disagrees (or failed
        # from a wrong guess) is reopened there
        for p in range(1, P):
            land = hs[p - 1].bounds()[1]
            if hs[p].rc == HOST or hs[p].bounds()[0] != land:
                hs[p].close()
                with torch.cuda.device(devs[p]):
                    hs[p] = _Handle(path, devs[p], p, P, first_start=land)
                hs[p].check_open()
                if hs[p].rc == HOST:
                    return None
        cols: list = [None] * P
        rcs = [OK] * P
        msgs = [""] * P

        def parse_one(p):
            h = hs[p]
            try:
                cols[p] = {c: torch.empty(h.n, dtype=TORCH_DTYPES[c], device=h.dev) for c in N.RECORD_COLUMNS}
            except torch.cuda.OutOfMemoryError:
                rcs[p] = HOST
                return
            if h.n:
                ptrs = (ctypes.c_void_p * len(N.RECORD_COLUMNS))(*[cols[p][c].data_ptr() for c in N.RECORD_COLUMNS])
                rcs[p] = h.L.sct_gbam_parse(h.h, _MODES[metric_mode], ptrs)
                msgs[p] = last_error()

        each(parse_one)
        for rc, msg in zip(rcs, msgs):
            _check(rc, msg)
        if any(rc == HOST for rc in rcs):
            return None
        L = load()
        remaps = []
        for which in range(3):
            sizes = [hs[p].dictionary_size(which) for p in range(P)]
            arrs = [np.zeros(max(1, k), dtype=np.int32) for k in sizes]
            ptrs = (ctypes.POINTER(ctypes.c_int32) * P)(
                *[a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) for a in arrs])
            handles = (ctypes.c_void_p * P)(*[h.h.value for h in hs])
            _check(L.sct_gbam_merge_dictionaries(handles, P, which, ptrs))
            remaps.append((arrs, sizes))

        def remap_one(p):
            h = hs[p]
            if not h.n:
                return
            for which, col in enumerate(("cell", "umi", "gene")):
                arrs, sizes = remaps[which]
                a = arrs[p]
                _check(h.L.sct_gbam_remap(h.h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), sizes[p],
                                          ctypes.c_void_p(cols[p][col].data_ptr()), h.n))

        each(remap_one)
        names = [hs[0].dictionary(which) for which in range(3)]
        if timings is not None:
            timings.update(hs[0].timing())
            timings["parts"] = [h.n for h in hs]
        return cols, names
    finally:
        close_all()
