"""
Line readers over one or more plain, gzip or bz2 files -- the reference's ``sctools.reader``
(``reader.py``) with the same names and signatures.

``infer_open``   picks ``open`` / ``gzip.open`` / ``bz2.open`` from the file's first bytes.
``Reader``       iterates the lines of several files as one stream.
``zip_readers``  iterates several readers in step.

:func:`open_binary` is what the device path of :mod:`sctools_amd.fastq` reads through: the same
detection, always bytes.
"""
import bz2
import gzip
import os
from functools import partial
from typing import Callable, Generator, Iterable, List, Set

GZIP_MAGIC = b"\x1f\x8b"
BZ2_MAGIC = b"BZh"


def _compression(file_: str) -> Callable:
    with open(file_, "rb") as f:
        head = f.read(3)
    if head[:2] == GZIP_MAGIC:
        return gzip.open
    if head == BZ2_MAGIC:
        return bz2.open
    return open


def infer_open(file_: str, mode: str) -> Callable:
    """The open function for ``file_``, chosen by magic number and not by extension, with the mode
    bound: ``'r'`` yields str (``'rt'`` for the compressed openers), ``'rb'`` bytes."""
    opener = _compression(file_)
    if opener is not open and mode == "r":
        mode = "rt"
    return partial(opener, mode=mode)


def open_binary(file_: str):
    """``file_`` opened for reading decompressed bytes."""
    return _compression(file_)(file_, "rb")


class Reader:
    """Loops over the lines of one or more files.

    Parameters
    ----------
    files : str or list of str
        the file(s) to read (default ``'-'``, as in the reference)
    mode : {'r', 'rb'}
        ``'r'`` yields str lines, ``'rb'`` bytes lines
    header_comment_char : str, optional
        when given, the leading lines of every file that begin with it are skipped
    """

    def __init__(self, files="-", mode="r", header_comment_char=None):
        if isinstance(files, str):
            self._files = [files]
        elif isinstance(files, Iterable):
            files = list(files)
            if not all(isinstance(f, str) for f in files):
                raise TypeError("All passed files must be type str")
            self._files = files
        else:
            raise TypeError("Files must be a string filename or a list of such names.")
        if mode not in {"r", "rb"}:
            raise ValueError("Mode must be one of 'r', 'rb'")
        self._mode = mode
        if isinstance(header_comment_char, str) and mode == "rb":
            header_comment_char = header_comment_char.encode()
        self._header_comment_char = header_comment_char

    @property
    def filenames(self) -> List[str]:
        return self._files

    def __len__(self) -> int:
        """Number of records; reads everything."""
        return sum(1 for _ in self)

    def __iter__(self):
        for name in self._files:
            with infer_open(name, self._mode)(name) as f:
                lines = iter(f)
                if self._header_comment_char is not None:
                    for line in lines:
                        if not line.startswith(self._header_comment_char):
                            yield line  # the first line that is no header
                            break
                yield from lines

    @property
    def size(self) -> int:
        """Bytes of all the files together, as stored."""
        return sum(os.stat(f).st_size for f in self._files)

    def select_record_indices(self, indices: Set) -> Generator:
        """The records whose index is in ``indices``, in file order; stops after the last of them."""
        wanted = set(indices)
        for i, record in enumerate(self):
            if i in wanted:
                yield record
                wanted.discard(i)
                if not wanted:
                    return


def zip_readers(*readers, indices=None) -> Generator:
    """One record of every reader at a time; with ``indices`` only the records at those indices."""
    if indices:
        yield from zip(*(r.select_record_indices(indices) for r in readers))
    else:
        yield from zip(*readers)
