"""What FastqProcess must produce, restated in plain Python for tests/test_gpu_fastq_process.py:
split the text, build the record bytes, hash, concatenate per shard in input order.  Nothing here
calls the code under test except ``std_hash``, which tests/test_fastq_process_cpu.py pins to
``std::hash<std::string>`` itself."""
import ctypes
import gzip
import os
import struct

import numpy as np

from sctools_amd.fastq_process import (BAD_IDENTIFIER, BAD_NAME, EMPTY_SEQUENCE, LENGTH_MISMATCH, LOW_QUALITY,
                                       MAX_IDENTIFIER, std_hash)

CODES = {c: i for i, c in enumerate(b"=ACMGRSVTWYHKDBN")}


def code(b: int) -> int:
    return CODES.get(b - 32 if 97 <= b <= 122 else b, 15)


def split_lines(text: bytes, is_last: bool = True):
    """``[(start, end)]`` of the lines: a line ends at ``\\n``; an unterminated last line counts only with
    ``is_last``; one ``\\r`` directly before the ``\\n`` is not part of the line."""
    out, at = [], 0
    while at < len(text):
        nl = text.find(b"\n", at)
        if nl < 0:
            if is_last:
                out.append((at, len(text)))
            break
        out.append((at, nl - 1 if nl > at and text[nl - 1] == 13 else nl))
        at = nl + 1
    return out


def lines_of(text: bytes, is_last: bool = True):
    """Per complete record ``((identifier start, length), (sequence ...), (quality ...), flags)``."""
    lines = split_lines(text, is_last)
    out = []
    for r in range(len(lines) // 4):
        (ns, ne), (ss, se), _, (qs, qe) = lines[4 * r:4 * r + 4]
        flags = 0
        at_sign = ne > ns and text[ns] == 64
        if not at_sign:
            flags |= BAD_NAME
        i0 = ns + (1 if at_sign else 0)
        space = text.find(b" ", i0, min(ne, i0 + MAX_IDENTIFIER + 1))
        i1 = space if space >= 0 else ne
        if not 1 <= i1 - i0 <= MAX_IDENTIFIER:
            flags |= BAD_IDENTIFIER
        if se == ss:
            flags |= EMPTY_SEQUENCE
        if se - ss != qe - qs:
            flags |= LENGTH_MISMATCH
        if any(b < 33 for b in text[qs:qe]):
            flags |= LOW_QUALITY
        out.append(((i0, i1 - i0), (ss, se - ss), (qs, qe - qs), flags))
    return out


def fields_of(text: bytes):
    """``[(identifier, sequence, quality)]`` of a well-formed text."""
    return [(text[a:a + la], text[b:b + lb], text[c:c + lc]) for (a, la), (b, lb), (c, lc), _ in lines_of(text)]


def bam_record(name: bytes, seq: bytes, qual: bytes, tags) -> bytes:
    core = struct.pack("<iiBBHHHIiii", -1, -1, len(name) + 1, 0, 4680, 0, 4, len(seq), -1, -1, 0)
    packed = bytes((code(seq[i]) << 4) | (code(seq[i + 1]) if i + 1 < len(seq) else 0) for i in range(0, len(seq), 2))
    body = core + name + b"\0" + packed + bytes(q - 33 for q in qual) + b"".join(t + b"Z" + v + b"\0" for t, v in tags)
    return struct.pack("<I", len(body)) + body


def tags_of(cr, cy, ur, uy, index=None, cb=None):
    """The reference's tag order: RG CR CY UR UY [SR SY] [CB]."""
    tags = [(b"RG", b"A"), (b"CR", cr), (b"CY", cy), (b"UR", ur), (b"UY", uy)]
    if index is not None:
        tags += [(b"SR", index[0]), (b"SY", index[1])]
    if cb is not None:
        tags.append((b"CB", cb))
    return tags


def fastq_records(name, seq, qual, cr, cy, ur, uy):
    return (b"@" + name + b"\n" + cr + ur + b"\n+\n" + cy + uy + b"\n",
            b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n")


def shard_of(bucket: bytes, n_shards: int) -> int:
    return std_hash(bucket) % n_shards


def read_bam(path):
    """``(header text, [raw record bytes])`` of a BAM file, through gzip alone."""
    data = gzip.open(path, "rb").read()
    assert data[:4] == b"BAM\1"
    l_text = int.from_bytes(data[4:8], "little")
    header = data[8:8 + l_text].decode()
    off = 8 + l_text
    n_ref = int.from_bytes(data[off:off + 4], "little")
    off += 4
    for _ in range(n_ref):
        off += 8 + int.from_bytes(data[off:off + 4], "little")
    out = []
    while off < len(data):
        size = int.from_bytes(data[off:off + 4], "little")
        out.append(data[off:off + 4 + size])
        off += 4 + size
    assert off == len(data)
    return header, out


def parse_record(raw: bytes):
    """``dict(name, flag, seq, qual, tags=[(tag, value)], core=...)`` of a raw record whose tags are all ``Z``."""
    size, = struct.unpack_from("<I", raw, 0)
    assert size + 4 == len(raw)
    ref, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, next_ref, next_pos, tlen = struct.unpack_from("<iiBBHHHIiii", raw, 4)
    at = 36
    name = raw[at:at + l_name - 1]
    assert raw[at + l_name - 1] == 0
    at += l_name + 4 * n_cigar
    packed = raw[at:at + (l_seq + 1) // 2]
    at += (l_seq + 1) // 2
    seq = "".join("=ACMGRSVTWYHKDBN"[(packed[i // 2] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
    qual = bytes(q + 33 for q in raw[at:at + l_seq])
    at += l_seq
    tags = []
    while at < len(raw):
        assert raw[at + 2] == ord("Z"), raw[at:at + 3]
        end = raw.index(b"\0", at + 3)
        tags.append((raw[at:at + 2], raw[at + 3:end]))
        at = end + 1
    return dict(name=name, flag=flag, seq=seq.encode(), qual=qual, tags=tags,
                core=(ref, pos, mapq, bin_, n_cigar, l_seq, next_ref, next_pos, tlen))


def native_hashes(strings) -> np.ndarray:
    """``std::hash<std::string>`` of every byte string, from tests/native/libstdhash.so (built by the Makefile)."""
    lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "libstdhash.so"))
    lib.sct_test_std_hash.restype = None
    lib.sct_test_std_hash.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    offsets = np.zeros(len(strings) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in strings], out=offsets[1:])
    out = np.zeros(len(strings), dtype=np.uint64)
    lib.sct_test_std_hash(b"".join(strings), offsets.ctypes.data, len(strings), out.ctypes.data)
    return out
