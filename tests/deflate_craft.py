"""A small raw-deflate writer (RFC 1951) for tests: every bit of a stream is the caller's choice.

A deflate compressor leaves most of the format unused; this writer reaches the rest -- chosen code
lengths, chosen run-length coding of the lengths, chosen distances, stored blocks anywhere, and raw
bits for streams that must be rejected.  ``Deflate.payload`` follows along as the plain-Python
meaning of what was written (``apply``), the expected output of any inflater.

ops: an int is a literal byte, ``(length, distance)`` a match; for broken streams also
``("sym", s)`` (the code of literal/length symbol s, no extra bits), ``("dsym", s)`` (the code of
distance symbol s) and ``("bits", value, n)``.
"""
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def length_symbol(length):
    """(symbol, extra value, extra bits) of a match length 3..258; 258 as symbol 285."""
    assert 3 <= length <= 258, length
    if length == 258:
        return 285, 0, 0
    k = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + k, length - LEN_BASE[k], LEN_EXTRA[k]


def distance_symbol(dist):
    assert 1 <= dist <= 32768, dist
    k = max(i for i in range(30) if DIST_BASE[i] <= dist)
    return k, dist - DIST_BASE[k], DIST_EXTRA[k]


def canonical(lens):
    """{symbol: (code, length)} of the canonical Huffman code with these lengths (RFC 1951 3.2.2)."""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for s, n in enumerate(lens):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def kraft(lens):
    """Sum of 2^-len over the coded symbols, in units of 2^-15: 32768 for a complete code."""
    return sum(1 << (15 - n) for n in lens if n)


def balanced(n):
    """n >= 2 code lengths of a complete code, as even as can be."""
    p = n.bit_length() - 1
    short = (2 << p) - n
    return [p] * short + [p + 1] * (n - short)


def rle_verbatim(lens):
    return list(lens)


def rle_greedy(lens):
    """Lengths -> code-length symbols with the longest repeats: ints, or (16 | 17 | 18, repeat)."""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r))
                run -= r
            if run >= 3:
                out.append((17, run))
                run = 0
        else:
            out.append(v)
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r))
                run -= r
        out.extend([v] * run)
        i = j
    return out


def rle_expand(rle):
    out = []
    for c in rle:
        if isinstance(c, tuple):
            sym, rep = c
            out.extend([out[-1] if sym == 16 else 0] * rep)
        else:
            out.append(c)
    return out


def apply(ops, out=None):
    """The bytes ``ops`` mean, appended to ``out`` (the member's earlier output, a bytearray)."""
    out = bytearray() if out is None else out
    for op in ops:
        if isinstance(op, tuple):
            length, dist = op
            assert 1 <= dist <= len(out), (dist, len(out))
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:  # overlapping: the last `dist` bytes repeat
                for _ in range(length):
                    out.append(out[-dist])
        else:
            out.append(op)
    return out


class Deflate:
    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0
        self.payload = bytearray()
        self.hclens = []  # the code-length code count of every dynamic block written

    # ---- bits
    def bits(self, value, n):
        """n bits of value, least significant first."""
        assert 0 <= value < (1 << n), (value, n)
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """A Huffman code: its bits go out most significant first."""
        self.bits(int(format(code, "0%db" % n)[::-1], 2), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    @property
    def nbits(self):
        return 8 * len(self.buf) + self.n

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")

    # ---- blocks
    def stored(self, data, final=False, nlen=None, length=None):
        """``length`` / ``nlen`` override the LEN / NLEN fields (broken streams)."""
        self.bits(1 if final else 0, 1)
        self.bits(0, 2)
        self.align()
        length = len(data) if length is None else length
        self.bits(length, 16)
        self.bits(length ^ 0xFFFF if nlen is None else nlen, 16)
        self.buf += data
        self.payload += data
        return self

    def symbols(self, ops, lit, dist, eob=True):
        for op in ops:
            if not isinstance(op, tuple):
                self.code(*lit[op])
                self.payload.append(op)
            elif op[0] == "bits":
                self.bits(op[1], op[2])
            elif op[0] == "sym":
                self.code(*lit[op[1]])
            elif op[0] == "dsym":
                self.code(*dist[op[1]])
            else:
                length, d = op
                s, xv, xb = length_symbol(length)
                self.code(*lit[s])
                self.bits(xv, xb)
                s, xv, xb = distance_symbol(d)
                self.code(*dist[s])
                self.bits(xv, xb)
                if d <= len(self.payload):
                    apply([op], self.payload)
        if eob:
            self.code(*lit[256])

    def fixed(self, ops, final=False, eob=True):
        self.bits(1 if final else 0, 1)
        self.bits(1, 2)
        self.symbols(ops, canonical(FIXED_LIT), canonical(FIXED_DIST), eob)
        return self

    def dynamic(self, ops, lit_lens, dist_lens, final=False, hclen=None, cl_lens=None, rle=rle_greedy, eob=True,
                hlit=None, hdist=None):
        """A dynamic block.  ``rle``: the code-length symbols of lit_lens + dist_lens, or a function
        making them; ``cl_lens``: the 19 lengths of the code-length code (default: a near-even
        complete code over the symbols ``rle`` uses); ``hclen``: how many of them are sent (default:
        up to the last nonzero one in the header's order); ``hlit`` / ``hdist`` override the header
        fields' values (broken streams)."""
        rle = rle(list(lit_lens) + list(dist_lens)) if callable(rle) else list(rle)
        used = sorted({c[0] if isinstance(c, tuple) else c for c in rle})
        if cl_lens is None:
            if len(used) == 1:  # a code-length code of one code would be incomplete
                used = sorted(set(used) | {0 if used[0] else 8})
            cl_lens = [0] * 19
            for s, n in zip(used, balanced(len(used))):
                cl_lens[s] = n
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
        self.hclens.append(hclen)
        self.bits(1 if final else 0, 1)
        self.bits(2, 2)
        self.bits(len(lit_lens) - 257 if hlit is None else hlit, 5)
        self.bits(len(dist_lens) - 1 if hdist is None else hdist, 5)
        self.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            self.bits(cl_lens[s], 3)
        cl = canonical(cl_lens)
        for c in rle:
            if isinstance(c, tuple):
                sym, rep = c
                self.code(*cl[sym])
                self.bits(rep - (11 if sym == 18 else 3), 7 if sym == 18 else 3 if sym == 17 else 2)
            else:
                self.code(*cl[c])
        if ops is not None:
            self.symbols(ops, canonical(lit_lens), canonical(dist_lens), eob)
        return self


def bgzf_member(deflate_bytes, payload=None, crc=None, isize=None):
    """One BGZF member around raw deflate data; crc / isize default to the payload's."""
    crc = zlib.crc32(payload) & 0xFFFFFFFF if crc is None else crc
    isize = len(payload) if isize is None else isize
    head = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(deflate_bytes) + 25)
    assert len(deflate_bytes) + 26 <= 65536, "a BGZF member holds at most 64 KB"
    return head + deflate_bytes + struct.pack("<II", crc, isize)


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
