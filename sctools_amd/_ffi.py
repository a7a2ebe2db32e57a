"""
The ctypes plumbing shared by every binding of a native library of this package.

``Library``          one shared library: where it is, its prototype table, how a return code becomes
                     an exception.  ``load()`` opens it once and applies the table.
``ptr``, ``stream``  a tensor's address and torch's current stream as ctypes arguments.
``device``           the torch device of an optional ``device`` argument; raises without a GPU.
``read_dictionary``  the packed strings of a ``sct_*_dictionary`` call.

A binding module declares ``PROTOTYPES = {name: (restype, [argtypes])}``, builds one ``Library``
from it and publishes ``load = LIBRARY.load``, ``check = LIBRARY.check`` and
``EXPORTED = tuple(PROTOTYPES)``: the table is the only list of the library's functions.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


class Library:
    """``filename`` is relative to the package (an absolute path is taken as it is); the environment
    variable ``env_override``, when set, names another file.  ``shares`` is a ``Library`` whose open
    handle this one uses (two prototype tables, one ``.so``, opened once).

    ``check(rc)`` passes the codes in ``accept`` and raises for every other one with the text of
    ``last_error_name()``: ``exceptions[rc]`` (default ``error_class``) with the message alone where
    an ``exceptions`` map is given, else ``error_class(error_format % (error_prefix, rc, message))``.

    Names in ``optional`` may be absent from the file (an older build given by ``env_override``);
    ``verify(lib)`` runs once after the table is applied and may raise.
    """

    def __init__(self, filename, error_prefix, last_error_name, error_class, prototypes, env_override=None,
                 mode=ctypes.DEFAULT_MODE, optional=(), exceptions=None, accept=(0,), error_format="%s error %d: %s",
                 shares=None, verify=None):
        self.path = (os.environ.get(env_override) if env_override else None) or os.path.join(HERE, filename)
        self.error_prefix, self.last_error_name, self.error_class = error_prefix, last_error_name, error_class
        self.prototypes, self.mode, self.optional = prototypes, mode, frozenset(optional)
        self.exceptions, self.accept, self.error_format = exceptions, frozenset(accept), error_format
        self.shares, self.verify = shares, verify
        self._lib = None

    def available(self) -> bool:
        return os.path.exists(self.path)

    def load(self) -> ctypes.CDLL:
        """The open library with every prototype set; ``ImportError`` if it was not built."""
        if self._lib is not None:
            return self._lib
        if self.shares is not None:
            lib = self.shares.load()
        else:
            if not self.available():
                raise ImportError("sctools_amd native library not built (%s missing); run `python -c "
                                  "'import __graft_entry__ as g; g.build()'`" % self.path)
            lib = ctypes.CDLL(self.path, mode=self.mode)
        for name, (restype, argtypes) in self.prototypes.items():
            if name in self.optional and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)
            fn.restype = restype
            fn.argtypes = argtypes
        if self.verify is not None:
            self.verify(lib)
        self._lib = lib
        return lib

    def last_error(self) -> str:
        """The library's message for the calling thread's last failed call."""
        return getattr(self.load(), self.last_error_name)().decode("utf-8", "replace")

    def check(self, rc: int, message=None) -> None:
        """Raises for a return code outside ``accept``.  ``message`` is for a caller that read
        ``last_error()`` earlier, on the thread that made the call (the text is thread-local)."""
        if rc in self.accept:
            return
        if message is None:
            message = self.last_error()
        if self.exceptions is not None:
            raise self.exceptions.get(rc, self.error_class)(message)
        raise self.error_class(self.error_format % (self.error_prefix, rc, message))


def ptr(t):
    """``c_void_p`` of a tensor's data; None (a NULL argument) for None and for an empty tensor."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def stream(dev):
    """torch's current stream on ``dev`` as a ``hipStream_t`` argument."""
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def device(device=None):
    """The torch device to run on, always with an index: of None (the current device), an int, a
    digit string, ``"cuda"``, ``"cuda:N"`` or a ``torch.device``.  Raises when there is no GPU."""
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("sctools_amd needs a ROCm GPU (torch.cuda.is_available() is False); "
                           "there is no CPU fallback")
    if isinstance(device, int) or (isinstance(device, str) and device.isdigit()):
        return torch.device("cuda", int(device))
    dev = torch.device("cuda" if device is None else device)
    if dev.type == "cuda" and dev.index is None:  # "cuda": the current device, for the library and the stream alike
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def read_dictionary(lib_fn, handle, which: int, strings: bool = True):
    """``(raw bytes, int64 offsets [k + 1], has_none)`` of dictionary ``which`` behind ``handle``:
    the k names back to back in id order, as ``columnar.PackedDictionary`` takes them.  ``lib_fn``
    is the library's ``sct_*_dictionary``; without ``strings`` the bytes are not copied."""
    cnt, by, off, hn = ctypes.c_int64(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int32()
    lib_fn(handle, which, ctypes.byref(cnt), ctypes.byref(by), ctypes.byref(off), ctypes.byref(hn))
    k = int(cnt.value)
    if k == 0 or not off.value:
        offs = np.zeros(1, dtype=np.int64)
    else:
        offs = np.frombuffer((ctypes.c_int64 * (k + 1)).from_address(off.value), dtype=np.int64).copy()
    total = int(offs[-1])
    raw = ctypes.string_at(by.value, total) if total and strings else b""
    return raw, offs, bool(hn.value)
