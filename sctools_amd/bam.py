"""
Minimal BAM / SAM record reader (host side).

The reference reads alignments through ``pysam`` (``pysam==0.16.0.1``,
``/root/reference/requirements.txt:3``), which is not installed in this image.
This module is a self-contained reader for the subset of the SAM/BAM spec the
metric path touches: the fixed BAM core fields, the CIGAR, the base qualities
and the optional tags.  It reproduces the pysam 0.16 semantics that the
reference's ``MetricAggregator.parse_molecule`` depends on
(``/root/reference/src/sctools/metrics/aggregator.py:251-334``):

* ``query_alignment_qualities``: qualities between the leading and trailing
  soft clips (pysam ``getQueryStart`` / ``getQueryEnd``; hard clips skipped,
  the trailing walk stops at CIGAR index 1), ``None`` when the read has no
  sequence or its first quality byte is 0xff;
* ``get_cigar_stats()[0][3]``: the summed length of ``N`` operations;
* ``get_tag``: ``KeyError`` for an absent tag.

BGZF is a concatenation of gzip members, so it is inflated with ``zlib`` in
streaming fashion.  It decodes SAM input and is the decoder the tests compare the
native one against; BAM input of the metric path goes through the native
multi-threaded decoder (``sctools_amd/csrc/bamdec.cpp``).

``split`` is SplitBam (``bam.py:361-488``) on the native splitter
(``sctools_amd/csrc/bamsplit.cpp``).  ``TagSortableRecord`` / ``verify_sort`` /
``sort_by_tags_and_queryname`` mirror the reference's sort order on record objects
(``bam.py:602-728``); ``verify_bam_sort`` checks a whole BAM on the GPU (VerifyBamSort) and
``tag_sort_bam`` writes one in that order (TagSortBam).  ``Tagger`` attaches tags from generators to
the records of a BAM (``bam.py:185-233``): barcode generators that have ``columns()`` extract on the
GPU, any other iterable is consumed on the host, and one native writer rewrites the records
(``sct_bam_attach_*``).
"""

import math
import os
import struct
import sys
import warnings
import zlib
from typing import Dict, Iterator, List, Optional, Set, Tuple

from sctools_amd import consts

__all__ = ["BamRecord", "open_alignments", "read_header", "split", "get_barcodes_from_bam",
           "get_barcode_for_alignment", "SortError", "TagSortableRecord", "get_tag_or_default",
           "sort_by_tags_and_queryname", "verify_sort", "verify_bam_sort", "tag_sort_bam", "Tagger"]

_CIGAR_OPS = "MIDNSHP=X"
_SEQ_NT16 = "=ACMGRSVTWYHKDBN"

BAM_CMATCH, BAM_CINS, BAM_CDEL, BAM_CREF_SKIP, BAM_CSOFT_CLIP, BAM_CHARD_CLIP = range(6)
BAM_CEQUAL, BAM_CDIFF = 7, 8

_TAG_INT_FMT = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
_ARRAY_FMT = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}


class BamRecord:
    """One alignment with the attributes the metric path reads.

    Attribute names follow ``pysam.AlignedSegment`` so the host code reads
    like the reference.
    """

    __slots__ = (
        "query_name", "flag", "reference_id", "pos", "mapq", "cigar",
        "l_seq", "_qual", "_tags",
    )

    def __init__(self, query_name, flag, reference_id, pos, mapq, cigar, l_seq, qual, tags):
        self.query_name = query_name
        self.flag = flag
        self.reference_id = reference_id
        self.pos = pos
        self.mapq = mapq
        self.cigar = cigar  # list of (op, length)
        self.l_seq = l_seq
        self._qual = qual  # bytes (raw phred, 0xff.. if absent) or None
        self._tags = tags  # dict tag -> python value

    # --- flag helpers (pysam names) ---
    @property
    def is_unmapped(self) -> bool:
        return bool(self.flag & 0x4)

    @property
    def is_reverse(self) -> bool:
        return bool(self.flag & 0x10)

    @property
    def is_duplicate(self) -> bool:
        return bool(self.flag & 0x400)

    @property
    def is_secondary(self) -> bool:
        return bool(self.flag & 0x100)

    # --- tags ---
    def get_tag(self, tag: str):
        return self._tags[tag]

    def has_tag(self, tag: str) -> bool:
        return tag in self._tags

    def get_tags(self):
        return list(self._tags.items())

    # --- CIGAR derived ---
    def n_skip_length(self) -> int:
        """Summed length of N (reference skip) operations: pysam ``get_cigar_stats()[0][3]``."""
        return sum(length for op, length in self.cigar if op == BAM_CREF_SKIP)

    def query_start(self) -> int:
        """pysam 0.16 ``getQueryStart``: leading soft clips, hard clips skipped."""
        start = 0
        for op, length in self.cigar:
            if op == BAM_CHARD_CLIP:
                if start != 0 and start != self.l_seq:
                    raise ValueError("Invalid clipping in CIGAR string")
            elif op == BAM_CSOFT_CLIP:
                start += length
            else:
                break
        return start

    def query_end(self) -> int:
        """pysam 0.16 ``getQueryEnd``: l_seq minus trailing soft clips (walk stops at index 1)."""
        end = self.l_seq
        if end == 0:
            for op, length in self.cigar:
                if op in (BAM_CMATCH, BAM_CINS, BAM_CEQUAL, BAM_CDIFF) or (
                    op == BAM_CSOFT_CLIP and end == 0
                ):
                    end += length
            return end
        for k in range(len(self.cigar) - 1, 0, -1):
            op, length = self.cigar[k]
            if op == BAM_CHARD_CLIP:
                if end != self.l_seq:
                    raise ValueError("Invalid clipping in CIGAR string")
            elif op == BAM_CSOFT_CLIP:
                end -= length
            else:
                break
        return end

    @property
    def query_alignment_qualities(self) -> Optional[bytes]:
        if self.l_seq == 0 or self._qual is None:
            return None
        if len(self._qual) == 0 or self._qual[0] == 0xFF:
            return None
        start, end = self.query_start(), self.query_end()
        if end < start:
            return b""
        return self._qual[start:end]


def _parse_tags(buf: bytes, off: int, end: int) -> Dict[str, object]:
    tags = {}
    unpack_from = struct.unpack_from
    while off < end:
        tag = buf[off:off + 2].decode("ascii")
        typ = chr(buf[off + 2])
        off += 3
        if typ == "Z" or typ == "H":
            nul = buf.index(b"\x00", off)
            tags[tag] = buf[off:nul].decode("ascii", "replace")
            off = nul + 1
        elif typ in _TAG_INT_FMT:
            fmt = _TAG_INT_FMT[typ]
            tags[tag] = unpack_from(fmt, buf, off)[0]
            off += struct.calcsize(fmt)
        elif typ == "A":
            tags[tag] = chr(buf[off])
            off += 1
        elif typ == "f":
            tags[tag] = unpack_from("<f", buf, off)[0]
            off += 4
        elif typ == "d":
            tags[tag] = unpack_from("<d", buf, off)[0]
            off += 8
        elif typ == "B":
            sub = chr(buf[off])
            count = unpack_from("<i", buf, off + 1)[0]
            off += 5
            code = _ARRAY_FMT[sub]
            size = struct.calcsize(code)
            tags[tag] = list(struct.unpack_from("<%d%s" % (count, code), buf, off))
            off += count * size
        else:
            raise ValueError("unsupported BAM tag type %r" % typ)
    return tags


class _BgzfStream:
    """Streaming inflater over concatenated gzip members (BGZF)."""

    def __init__(self, path: str, chunk: int = 1 << 20):
        self._fh = open(path, "rb")
        self._chunk = chunk
        self._buf = bytearray()
        self._pos = 0
        self._d = zlib.decompressobj(16 + zlib.MAX_WBITS)
        self._eof = False

    def close(self):
        self._fh.close()

    def _fill(self, need: int) -> None:
        while len(self._buf) - self._pos < need and not self._eof:
            raw = self._fh.read(self._chunk)
            if not raw:
                self._eof = True
                break
            while raw:
                out = self._d.decompress(raw)
                self._buf += out
                if self._d.eof:
                    raw = self._d.unused_data
                    self._d = zlib.decompressobj(16 + zlib.MAX_WBITS)
                else:
                    raw = b""
        if self._pos > (1 << 22):
            del self._buf[: self._pos]
            self._pos = 0

    def read(self, n: int) -> bytes:
        self._fill(n)
        out = bytes(self._buf[self._pos:self._pos + n])
        self._pos += len(out)
        return out


def _iter_bam(path: str) -> Iterator[BamRecord]:
    stream = _BgzfStream(path)
    try:
        magic = stream.read(4)
        if magic != b"BAM\x01":
            raise ValueError("%s is not a BAM file" % path)
        (l_text,) = struct.unpack("<i", stream.read(4))
        stream.read(l_text)
        (n_ref,) = struct.unpack("<i", stream.read(4))
        for _ in range(n_ref):
            (l_name,) = struct.unpack("<i", stream.read(4))
            stream.read(l_name + 4)
        core = struct.Struct("<iiBBHHHiiii")
        while True:
            head = stream.read(4)
            if len(head) < 4:
                return
            (block_size,) = struct.unpack("<i", head)
            data = stream.read(block_size)
            (ref_id, pos, l_read_name, mapq, _bin, n_cigar, flag, l_seq,
             _nref, _npos, _tlen) = core.unpack_from(data, 0)
            off = 32
            qname = data[off:off + l_read_name - 1].decode("ascii", "replace")
            off += l_read_name
            cigar = []
            for k in range(n_cigar):
                (c,) = struct.unpack_from("<I", data, off + 4 * k)
                cigar.append((c & 0xF, c >> 4))
            off += 4 * n_cigar
            off += (l_seq + 1) // 2
            qual = data[off:off + l_seq]
            off += l_seq
            tags = _parse_tags(data, off, len(data))
            yield BamRecord(qname, flag, ref_id, pos, mapq, cigar, l_seq, qual, tags)
    finally:
        stream.close()


def _parse_sam_tag(field: str):
    tag, typ, val = field.split(":", 2)
    if typ == "i":
        return tag, int(val)
    if typ == "f":
        return tag, float(val)
    if typ == "B":
        parts = val.split(",")
        conv = float if parts[0] == "f" else int
        return tag, [conv(p) for p in parts[1:]]
    return tag, val


def _iter_sam(path: str) -> Iterator[BamRecord]:
    import re

    refs: Dict[str, int] = {}
    cig_re = re.compile(r"(\d+)([MIDNSHP=X])")
    opener = open
    if path.endswith(".gz"):
        import gzip

        opener = gzip.open
    with opener(path, "rt") as fh:
        for line in fh:
            if line.startswith("@"):
                if line.startswith("@SQ"):
                    for f in line.rstrip("\n").split("\t"):
                        if f.startswith("SN:"):
                            refs[f[3:]] = len(refs)
                continue
            f = line.rstrip("\n").split("\t")
            if len(f) < 11:
                continue
            flag = int(f[1])
            ref_id = refs.get(f[2], -1) if f[2] != "*" else -1
            pos = int(f[3]) - 1
            cigar: List[Tuple[int, int]] = []
            if f[5] != "*":
                cigar = [(_CIGAR_OPS.index(o), int(n)) for n, o in cig_re.findall(f[5])]
            seq = f[9]
            l_seq = 0 if seq == "*" else len(seq)
            if f[10] == "*":
                qual = b"\xff" * l_seq if l_seq else b""
            else:
                qual = bytes(ord(c) - 33 for c in f[10])
            tags = dict(_parse_sam_tag(t) for t in f[11:])
            yield BamRecord(f[0], flag, ref_id, pos, int(f[4]), cigar, l_seq, qual, tags)


def open_alignments(path: str, mode: str = "rb") -> Iterator[BamRecord]:
    """Iterate alignments of a BAM (``mode='rb'``) or SAM (``mode='r'``) file in file order."""
    if "b" in mode:
        return _iter_bam(path)
    return _iter_sam(path)


def read_header(path: str) -> Tuple[str, List[Tuple[str, int]]]:
    """Return (header text, [(reference name, length)]) of a BAM file."""
    stream = _BgzfStream(path)
    try:
        if stream.read(4) != b"BAM\x01":
            raise ValueError("%s is not a BAM file" % path)
        (l_text,) = struct.unpack("<i", stream.read(4))
        text = stream.read(l_text).decode("ascii", "replace").rstrip("\x00")
        (n_ref,) = struct.unpack("<i", stream.read(4))
        refs = []
        for _ in range(n_ref):
            (l_name,) = struct.unpack("<i", stream.read(4))
            name = stream.read(l_name).rstrip(b"\x00").decode("ascii")
            (l_ref,) = struct.unpack("<i", stream.read(4))
            refs.append((name, l_ref))
        return text, refs
    finally:
        stream.close()


# ---------------- SplitBam (bam.py:236-488) ----------------
def get_barcode_for_alignment(alignment, tags: List[str], raise_missing: bool):
    """The value of the first of ``tags`` the alignment carries (bam.py:263-290)."""
    barcode = None
    for tag in tags:
        if alignment.has_tag(tag):
            barcode = alignment.get_tag(tag)
            break
    if raise_missing and barcode is None:
        raise RuntimeError("Alignment encountered that is missing {} tag(s).".format(tags))
    return barcode


def get_barcodes_from_bam(in_bam: str, tags: List[str], raise_missing: bool) -> Set:
    """Distinct barcodes of a BAM, None excluded (bam.py:236-260)."""
    out = set()
    for alignment in open_alignments(in_bam, "rb"):
        b = get_barcode_for_alignment(alignment, tags, raise_missing)
        if b is not None:
            out.add(b)
    return out


def split(in_bams: List[str], out_prefix: str, tags: List[str], approx_mb_per_split: float = 1000,
          raise_missing: bool = True, num_processes: Optional[int] = None) -> List[str]:
    """SplitBam (bam.py:361-488): split ``in_bams`` by barcode into chunks of about
    ``approx_mb_per_split`` MB, every barcode in exactly one chunk.

    Same arguments, limits, errors and return value as the reference: ``ValueError`` for no
    tags or too many chunks, ``RuntimeError`` for a record without any of ``tags`` when
    ``raise_missing``, chunk paths ``realpath(f"{out_prefix}_{k}.bam")`` in chunk order.  The
    work is one native call (sctools_amd/csrc/bamsplit.cpp) on ``num_processes`` threads.
    Barcodes are assigned to chunks in string order (the reference uses Python set order, which
    varies from run to run); records keep their file order; several inputs are concatenated.
    """
    from sctools_amd import bamnative

    if len(tags) == 0:
        raise ValueError("At least one tag must be passed")
    if num_processes is None:
        num_processes = os.cpu_count() or 1
    bam_mb = sum(os.path.getsize(b) * 1e-6 for b in in_bams)
    n_subfiles = int(math.ceil(bam_mb / approx_mb_per_split))
    if n_subfiles > consts.MAX_BAM_SPLIT_SUBFILES_TO_WARN:
        warnings.warn("Number of requested subfiles (%d) exceeds %d; this may cause OS errors by exceeding fid "
                      "limits" % (n_subfiles, consts.MAX_BAM_SPLIT_SUBFILES_TO_WARN))
    if n_subfiles > consts.MAX_BAM_SPLIT_SUBFILES_TO_RAISE:
        raise ValueError("Number of requested subfiles (%d) exceeds %d; this will usually cause OS errors, think "
                         "about increasing max_mb_per_split." % (n_subfiles, consts.MAX_BAM_SPLIT_SUBFILES_TO_RAISE))
    sys.stderr.write("Splitting the bams by barcode\n")
    n = bamnative.split(list(in_bams), out_prefix, list(tags), max(1, n_subfiles), raise_missing,
                        threads=num_processes)
    return [os.path.realpath("%s_%d.bam" % (out_prefix, k)) for k in range(n)]


# ---------------- TagSortBam / VerifyBamSort order (bam.py:602-728) ----------------
class SortError(Exception):
    """Records out of (tags, query name) order (bam.py:727-728)."""


def get_tag_or_default(alignment, tag_key: str, default: Optional[str] = None):
    """The tag's value, or ``default`` when the alignment lacks it (bam.py:602-610)."""
    try:
        return alignment.get_tag(tag_key)
    except KeyError:
        return default


class TagSortableRecord:
    """A record keyed by its tag values, then its query name (bam.py:638-695): the order of
    ``sort_by_tags_and_queryname`` and ``verify_sort``; comparing records keyed by different tag
    lists raises ValueError."""

    def __init__(self, tag_keys, tag_values, query_name: str, record=None) -> None:
        self.tag_keys = tag_keys
        self.tag_values = tag_values
        self.query_name = query_name
        self.record = record

    @classmethod
    def from_aligned_segment(cls, record, tag_keys) -> "TagSortableRecord":
        assert record is not None
        return cls(tag_keys, [get_tag_or_default(record, key, "") for key in tag_keys], record.query_name, record)

    def _check(self, other) -> None:
        if self.tag_keys != other.tag_keys:
            raise ValueError("Cannot compare records using different tag lists: {0}, {1}".format(
                self.tag_keys, other.tag_keys))

    def _key(self):
        return (list(self.tag_values), self.query_name)

    def __lt__(self, other) -> bool:
        if not isinstance(other, TagSortableRecord):
            return NotImplemented
        self._check(other)
        return self._key() < other._key()

    def __eq__(self, other) -> bool:
        if not isinstance(other, TagSortableRecord):
            return NotImplemented
        self._check(other)
        return self._key() == other._key()

    def __le__(self, other) -> bool:
        return self < other or self == other

    def __gt__(self, other) -> bool:
        if not isinstance(other, TagSortableRecord):
            return NotImplemented
        return other < self

    def __ge__(self, other) -> bool:
        if not isinstance(other, TagSortableRecord):
            return NotImplemented
        return other < self or self == other

    __hash__ = None

    def __repr__(self) -> str:
        return "TagSortableRecord(tags: {0}, tag_values: {1}, query_name: {2}".format(
            self.tag_keys, self.tag_values, self.query_name)

    __str__ = __repr__


def sort_by_tags_and_queryname(records, tag_keys):
    """The records in (tag values, query name) order, stable (bam.py:698-709)."""
    return (r.record for r in sorted(TagSortableRecord.from_aligned_segment(r, tag_keys) for r in records))


def _order_error(i: int, record, old_record) -> SortError:
    msg = "Records {0} and {1} are not in correct order:\n{1}:{2} \nis less than \n{0}:{3}"
    return SortError(msg.format(i - 1, i, record, old_record))


def verify_sort(records, tag_keys) -> None:
    """Raise SortError at the first record smaller than its predecessor (bam.py:712-724)."""
    old = TagSortableRecord(tag_keys=tag_keys, tag_values=["" for _ in tag_keys], query_name="", record=None)
    i = 0
    for record in records:
        i += 1
        if not record >= old:
            raise _order_error(i, record, old)
        old = record


def _sort_keys(path: str, tag_keys):
    """(keys, key names, query-name ranks, query names) of a BAM: up to three string-valued tags as
    ranks of their sorted values (native decode, "" for a missing tag); query names as ranks of the
    sorted names.  More tags, or a tag holding integer / float / array values, go through
    _typed_sort_keys: Python's own comparisons of the values (ints numerically; an int against a
    str raises TypeError, as the reference's sorted() does)."""
    from sctools_amd import bamnative

    if len(tag_keys) <= 3:
        pad = [t for t in ("~0", "~1", "~2") if t not in tag_keys][: 3 - len(tag_keys)]
        try:
            arrays, names = bamnative.decode(path, "sortkeys", tags=tuple(list(tag_keys) + pad))
        except bamnative.TypedTagValue:
            return _typed_sort_keys(path, tag_keys)
        keys = [arrays["cell"], arrays["umi"], arrays["gene"]][: len(tag_keys)]
        key_names = [["" if v is None else v for v in nm] for nm in names[: len(tag_keys)]]
        return keys, key_names, arrays["qname"], names[3], False
    return _typed_sort_keys(path, tag_keys)


def _ranks(values):
    """(rank of each value, distinct values in order) under Python's comparisons -- unhashable
    values (arrays) included; mixed incomparable types raise TypeError as sorted() does."""
    order = sorted(range(len(values)), key=lambda i: values[i])
    rank = [0] * len(values)
    distinct = []
    for i in order:
        if not distinct or values[i] != distinct[-1]:
            distinct.append(values[i])
        rank[i] = len(distinct) - 1
    return rank, distinct


def _typed_sort_keys(path: str, tag_keys):
    """_sort_keys on the host with the tags' Python values (get_tag_or_default(r, k, ""),
    bam.py:655-656): the value tuples are ranked with Python's comparisons (one key column; the
    last element True says so)."""
    import numpy as np

    recs = [(tuple(get_tag_or_default(r, k, "") for k in tag_keys), r.query_name) for r in open_alignments(path, "rb")]
    trank, tuples = _ranks([t for t, _ in recs])
    qs = sorted(set(q for _, q in recs))
    qr = {q: i for i, q in enumerate(qs)}
    return ([np.array(trank, dtype=np.int32)], [[list(t) for t in tuples]],
            np.array([qr[q] for _, q in recs], dtype=np.int32), qs, True)


def _key_columns(eng, keys, key_names, n):
    """Record columns carrying the sort keys (cell, umi, gene slots), Dims and the order name."""
    import numpy as np
    import torch

    from sctools_amd import engine as E
    from sctools_amd import _native as N

    cols = {c: torch.zeros(n, dtype=E.TORCH_DTYPES[c], device=eng.device) for c in N.RECORD_COLUMNS}
    for slot, k in zip(("cell", "umi", "gene"), keys):
        cols[slot] = torch.from_numpy(np.ascontiguousarray(k, dtype=np.int32)).to(eng.device)
    size = [max(1, len(nm)) for nm in key_names] + [1] * (3 - len(key_names))
    dims = E.Dims(size[0], size[2], size[1])  # (cell, gene, umi) id counts
    return cols, dims, ("cell" if len(keys) <= 1 else "cell_umi_gene")


def verify_bam_sort(path: str, tag_keys, device=None) -> None:
    """VerifyBamSort on a BAM file (platform.py:100-143): the records decoded natively (the
    tags' values and the query names as ranks of their sorted strings, bamdec.cpp sort-key
    mode) and checked on the GPU (sct_verify_sort); raises SortError as verify_sort does."""
    import numpy as np
    import torch

    from sctools_amd import engine as E

    tag_keys = list(tag_keys)
    keys, key_names, qrank, qnames, typed = _sort_keys(path, tag_keys)
    n = int(qrank.shape[0])
    if n < 2:
        return
    if typed:  # integer / float / array values: the reference's comparisons themselves (TypeError included)
        verify_sort((TagSortableRecord.from_aligned_segment(r, tag_keys) for r in open_alignments(path, "rb")),
                    tag_keys)
        return
    eng = E.get_engine(device)
    cols, dims, order = _key_columns(eng, keys, key_names, n)
    tie = torch.from_numpy(np.ascontiguousarray(qrank, dtype=np.int32)).to(eng.device)
    p = eng.verify_sort(cols, dims, order, tie)
    if p < 0:
        return

    def record(j):
        vals = [key_names[k][int(keys[k][j])] for k in range(len(tag_keys))]
        return TagSortableRecord(tag_keys, vals, qnames[int(qrank[j])])

    raise _order_error(p + 1, record(p), record(p - 1))


def tag_sort_bam(in_bam: str, out_bam: str, tag_keys, device=None, level: int = 6) -> None:
    """TagSortBam (platform.py:60-97): the records of ``in_bam`` written to ``out_bam`` in
    (tags, query name) order, ties in input order (sort_by_tags_and_queryname's stable
    sorted()): keys decoded natively, the order computed on the GPU (sct_tag_sort: one radix
    round on the packed tag ranks, the query-name rank as the tiebreak), the records written
    byte for byte under the input's header (sct_bam_write_order)."""
    import numpy as np
    import torch

    from sctools_amd import bamnative
    from sctools_amd import engine as E

    tag_keys = list(tag_keys)
    keys, key_names, qrank, qnames, _ = _sort_keys(in_bam, tag_keys)
    n = int(qrank.shape[0])
    if n == 0:
        bamnative.write_order(in_bam, out_bam, np.zeros(0, np.int64), level=level)
        return
    eng = E.get_engine(device)
    cols, dims, order = _key_columns(eng, keys, key_names, n)
    cols["pos"] = torch.arange(n, dtype=torch.int32, device=eng.device)  # rides along: the permutation
    tie = torch.from_numpy(np.ascontiguousarray(qrank, dtype=np.int32)).to(eng.device)
    out = eng.tag_sort(cols, dims, order, tie, len(qnames))
    bamnative.write_order(in_bam, out_bam, out["pos"].to(torch.int64).cpu().numpy(), level=level)


# ---- Tagger (bam.py:185-233) ----

_HOST_BATCH = 1 << 16  # records per window of a host iterable


def _host_windows(tag_sets, batch: int = _HOST_BATCH):
    """Windows of a host iterable of tag sets (lists of ``(tag, value, "Z")``) in column form: ``(n, columns)``,
    ``columns`` a list of ``(tag, uint8 [n, stride], int32 [n] lengths)`` with -1 where a record does not
    carry the tag.  The
    columns keep every record's tag order; a record whose order contradicts the window's starts a
    new window."""
    import numpy as np

    order, rows = [], []

    def flush():
        n = len(rows)
        out = []
        for key in order:
            values = [row.get(key) for row in rows]
            stride = max((len(v) for v in values if v is not None), default=0)
            col = np.zeros((n, stride), dtype=np.uint8)
            lengths = np.full(n, -1, dtype=np.int32)
            for i, v in enumerate(values):
                if v is not None:
                    lengths[i] = len(v)
                    col[i, :len(v)] = np.frombuffer(v, dtype=np.uint8)
            out.append((key[0], col, lengths))
        del order[:], rows[:]
        return n, out

    for tag_set in tag_sets:
        row, seen = {}, {}
        for tag, value, *kind in tag_set:
            if kind and kind[0] != "Z":
                raise ValueError("Tagger attaches string (Z) tags only, got %r for %s" % (kind[0], tag))
            if isinstance(tag, bytes):
                tag = tag.decode()
            seen[tag] = seen.get(tag, 0) + 1
            row[(tag, seen[tag])] = value.encode() if isinstance(value, str) else bytes(value)
        for attempt in range(2):
            pos, trial = -1, list(order)
            for key in row:
                if key in trial:
                    at = trial.index(key)
                    if at <= pos:
                        break
                    pos = at
                else:
                    pos += 1
                    trial.insert(pos, key)
            else:
                order[:] = trial
                break
            yield flush()  # this record lists its tags in another order than the window's
        rows.append(row)
        if len(rows) >= batch:
            yield flush()
    if rows:
        yield flush()


def _device_windows(generator, device, max_records, inflate):
    """The windows of ``generator.columns()`` in the column form of :func:`_host_windows`."""
    import numpy as np

    for window in generator.columns(device=device, max_records=max_records, inflate=inflate):
        out = []
        for key, values in window.items():
            if len(key) != 2:
                continue  # "CB_index"
            values = values.cpu().numpy()
            lengths = None
            index = window.get(key + "_index")
            if index is not None:  # the tag goes only to the records that have a correction
                lengths = np.where(index.cpu().numpy() < 0, -1, values.shape[1]).astype(np.int32)
            out.append((key, values, lengths))
        yield (out[0][1].shape[0] if out else 0), out


class Tagger:
    """Attaches the tags that generators yield to the records of a BAM, in step.

    Parameters
    ----------
    bam_file : str
        the BAM whose records receive the tags
    device : optional
        GPU index or torch device for the generators that extract on the GPU (default: current GPU)
    inflate : {"auto", "host"}, optional
        who inflates those generators' BGZF-compressed FASTQ files (``fastq.TextWindows``)
    """

    def __init__(self, bam_file: str, device=None, inflate: Optional[str] = None) -> None:
        if not isinstance(bam_file, str):
            raise TypeError(f'The argument "bam_file" must be of type str, not {type(bam_file)}')
        self.bam_file = bam_file
        self.device = device
        from sctools_amd import fastq

        self.inflate = fastq.check_inflate(fastq.DEFAULT_INFLATE if inflate is None else inflate)

    def tag(self, output_bam_name: str, tag_generators) -> None:
        """Writes the records of ``bam_file`` to ``output_bam_name`` with the tags of every generator
        set, record k getting the k-th tag set of each; the output ends with the shortest of the
        inputs.  A generator with ``columns()`` runs on the GPU, any other iterable on the host."""
        import itertools

        from sctools_amd import bamnative

        with bamnative.TagAttacher(self.bam_file, output_bam_name) as out:
            # the reference's zip advances every generator once more than the BAM has records before it
            # ends; a bad FASTQ record beyond that one is never read there, and is not looked at here
            sources = []
            for g in tag_generators:
                if hasattr(g, "columns") and getattr(g, "supports_columns", True):
                    sources.append(_device_windows(g, self.device, out.n + 1, self.inflate))
                else:
                    sources.append(_host_windows(itertools.islice(g, out.n + 1)))
            held = [(0, [], 0)] * len(sources)  # per source: (rows, columns, rows already written)
            while out.remaining > 0:
                n = out.remaining
                for k, source in enumerate(sources):
                    while held[k][2] >= held[k][0]:  # used up: the next window that has rows
                        window = next(source, None)
                        if window is None:
                            n = 0  # the zip ends with its shortest input
                            break
                        held[k] = (window[0], window[1], 0)
                    n = min(n, held[k][0] - held[k][2])
                    if n == 0:
                        break
                if n == 0:
                    break
                columns = []
                for k, (rows, window, at) in enumerate(held):
                    for tag, values, lengths in window:
                        columns.append((tag, values[at:at + n], None if lengths is None else lengths[at:at + n]))
                    held[k] = (rows, window, at + n)
                out.write(columns, n)
