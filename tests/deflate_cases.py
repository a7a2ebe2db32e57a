"""Crafted deflate members for the inflaters (tests/deflate_craft.py writes them).

VALID: name -> builder of a list of members whose payload is known from ``apply``; INVALID: name ->
builder of one member a conforming inflater rejects, with the device status it must report
(sctools_amd/csrc/inflate.h ST_*; None: any nonzero status).  test_deflate_craft_cpu.py proves
every label against zlib; test_gpu_inflate_crafted.py runs the device inflate on the same members.

Two of the format's corners cannot be framed as BGZF and are left to the writer's own CPU test: a
stored block of 65535 bytes (a member holds 65536 bytes with its 26 of framing: the largest stored
block that fits has 65505), and a header that sends only 4 code-length code lengths and is valid
(those four are the lengths of 16, 17, 18 and 0: every literal length would be 0, so the block has
no end-of-block code; it is in INVALID, and 5 is the smallest count among the valid ones).
"""
import collections
import functools
import random
import struct
import zlib

import deflate_craft as C

WINDOWS = (2048, 4096, 8192, 16384, 32768)  # every window size the kernel can be built with

M = collections.namedtuple("M", "deflate payload crc isize")


def member(d, payload=None, crc=None, isize=None):
    """A finished Deflate as a member; payload None: the stream is invalid (isize is then given)."""
    p = bytes(d.payload) if payload is None and isize is None else payload
    if p is not None:
        assert len(p) <= 65536
        return M(d.getvalue(), p, zlib.crc32(p) & 0xFFFFFFFF if crc is None else crc, len(p) if isize is None else isize)
    return M(d.getvalue(), None, 0 if crc is None else crc, isize)


def bgzf(m):
    return C.bgzf_member(m.deflate, crc=m.crc, isize=m.isize)


def lens_over(n, symbols, lengths=None):
    """n code lengths: `lengths` (default: a near-even complete code) on `symbols`, 0 elsewhere."""
    lengths = C.balanced(len(symbols)) if lengths is None else lengths
    out = [0] * n
    for s, l in zip(symbols, lengths):
        out[s] = l
    return out


def distinct(rng, n):
    """n bytes, no two equal within any 256 in a row: a copy from the wrong phase shows."""
    perm = rng.sample(range(256), 256)
    return [perm[i % 256] ^ (0x80 if i >= 256 else 0) for i in range(n)]


# ---------------------------------------------------------------- valid members

def overlap_all_dists():
    """For every dist in 1..257: dist literals, then (258, dist)."""
    rng = random.Random(101)
    out = []
    for lo, hi in ((1, 128), (129, 257)):
        ops = []
        for dist in range(lo, hi + 1):
            ops += distinct(rng, dist) + [(258, dist)]
        out.append(member(C.Deflate().fixed(ops, final=True)))
    return out


OVERLAP_DISTS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 257)


def overlap_lengths(dists):
    """Per dist one member: dist literals, then a copy of every length 3..258 at that distance."""
    rng = random.Random(102)
    out = []
    for dist in dists:
        ops = distinct(rng, dist) + [(n, dist) for n in range(3, 259)]
        out.append(member(C.Deflate().fixed(ops, final=True)))
    return out


def window_dists(W):
    ds = {W + k for k in (-258, -257, -65, -64, -1, 0, 1, 63, 64, 65, 257, 258, 259)}
    return sorted({min(d, 32768) for d in ds})


WINDOW_LENS = (3, 63, 64, 65, 128, 129, 257, 258)


@functools.lru_cache(maxsize=None)
def window_members(W):
    """Every (dist, len) around a window of W bytes, each issued at pos mod W/4 in {0, 1, W/4 - 1}
    (right after the kernel's flush and as far from it as can be): random bytes (a stored block,
    then three literals), then the match.  Returns (members, the (dist, len, pos) of every match)."""
    rng = random.Random(W)
    q = W // 4
    tasks = [(ph, d, n) for ph in (0, 1, q - 1) for d in window_dists(W) for n in WINDOW_LENS]
    out, issued = [], []
    d = C.Deflate()
    for ph, dist, n in tasks:
        while True:
            pos = len(d.payload)
            t = max(pos + 4, dist)
            t += (ph - t) % q
            if t + n <= 63000:
                break
            assert pos, (W, dist, n)
            out.append(member(d.stored(b"", final=True)))
            d = C.Deflate()
        d.stored(rng.randbytes(t - pos - 3))
        d.fixed(list(rng.randbytes(3)) + [(n, dist)])
        issued.append((dist, n, t))
    out.append(member(d.stored(b"", final=True)))
    return out, issued


def format_limits():
    rng = random.Random(103)
    # exactly 65536 bytes, ending with the longest match at the largest distance
    a = C.Deflate().stored(rng.randbytes(65536 - 258)).fixed([(258, 32768)], final=True)
    assert len(a.payload) == 65536
    # dist == pos: the source is the member's very first byte
    b = C.Deflate()
    for target in (1, 4, 7, 63, 129, 257, 2047, 2305, 4096, 32768):
        fill = target - len(b.payload)
        if fill > 300:
            b.stored(rng.randbytes(fill))
            fill = 0
        b.fixed(list(rng.randbytes(fill)) + [(3, target)])
    b.fixed([(258, 32768)], final=True)
    return [member(a), member(b)]


LONG_COUNTS = {2: 2, 3: 2, 4: 2, 5: 1, 6: 1, 7: 1, 8: 3, 9: 16, 10: 16, 11: 8, 12: 16, 13: 16, 14: 16, 15: 32}
LONG_DIST = list(range(1, 15)) + [15, 15]


def long_code_sets(seed):
    """(lit_lens, dist_lens): literal/length lengths 2..15 over 102 literals, end-of-block and the
    29 length symbols, distance lengths 1..14, 15, 15 over 16 of the 30 symbols; literals, length
    symbols and distance symbols each own codes of 9, 10, 12 and 15 bits."""
    lengths = [l for l, k in sorted(LONG_COUNTS.items()) for _ in range(k)]
    assert C.kraft(lengths) == 32768 and C.kraft(LONG_DIST) == 32768
    while True:
        rng = random.Random(seed)
        syms = rng.sample(range(256), 102) + list(range(256, 286))
        rng.shuffle(syms)
        lit = lens_over(286, syms, lengths)
        have_lit = {lit[s] for s in range(256)}
        have_len = {lit[s] for s in range(257, 286)}
        if {9, 10, 12, 15} <= have_lit and {9, 10, 12, 15} <= have_len:
            break
        seed += 1000
    dsyms = rng.sample(range(30), 16)
    return lit, lens_over(30, dsyms, LONG_DIST)


def long_codes():
    """Every coded symbol used: each literal, each length symbol with each distance symbol.  The same
    ops under two assignments of the lengths (the second drawn from the first's symbols)."""
    rng = random.Random(104)
    lit, dist = long_code_sets(7)
    ops = [s for s in range(256) if lit[s]]
    for ls in range(257, 286):
        for ds in (s for s in range(30) if dist[s]):
            k = ls - 257
            n = 258 if ls == 285 else C.LEN_BASE[k] + rng.randrange(1 << C.LEN_EXTRA[k])
            ops.append((n, C.DIST_BASE[ds] + rng.randrange(1 << C.DIST_EXTRA[ds])))
    rng.shuffle(ops)
    # the second assignment: the same symbols, their lengths dealt again
    r2 = random.Random(8)
    while True:
        lsyms = [s for s in range(286) if lit[s]]
        lit2 = lens_over(286, lsyms, r2.sample([lit[s] for s in lsyms], len(lsyms)))
        if ({9, 10, 12, 15} <= {lit2[s] for s in range(256)} and {9, 10, 12, 15} <= {lit2[s] for s in range(257, 286)}
                and lit2 != lit):
            break
    dsyms = [s for s in range(30) if dist[s]]
    dist2 = lens_over(30, dsyms, r2.sample(LONG_DIST, 16))
    head = rng.randbytes(32768)
    out = []
    for ll, dl in ((lit, dist), (lit2, dist2)):
        assert max(ll) == 15 and max(dl) == 15
        out.append(member(C.Deflate().stored(head).dynamic(ops, ll, dl, final=True)))
    return out


def _chain_lits(L):
    """A complete literal/length set that has length L, built from 8-bit codes with the code-length
    symbols that come no later than L in the header's order (CL_ORDER): L < 8 joins 2^(8-L) of the
    8-bit codes into one; L > 8 splits one into 9, 10, ..., L, L."""
    syms = list(range(250)) + [256, 257, 258, 259, 260, 261]  # 256 codes of 8 bits
    lens = lens_over(286, syms, [8] * 256)
    if L < 8:
        for s in range(250 - (1 << (8 - L)), 250):
            lens[s] = 0
        lens[249] = L
    elif L > 8:
        lens[249] = 0
        extra = [250, 251, 252, 253, 254, 255, 262, 263]
        for s, l in zip(extra, list(range(9, L + 1)) + [L]):
            lens[s] = l
    assert C.kraft(lens) == 32768, L
    return lens


def hclen_member(k):
    """A dynamic block whose header sends k >= 5 code-length code lengths, the k-th nonzero."""
    L = C.CL_ORDER[k - 1]
    lit = _chain_lits(L)
    avail = set(C.CL_ORDER[3:k])
    dist = [4] * 16 if 4 in avail else [0]
    rng = random.Random(k)
    ops = [s for s in range(256) if lit[s]]
    if dist != [0]:
        ops += [(n, 1 + rng.randrange(32)) for n in (3, 4, 5, 6, 7)]
    d = C.Deflate().dynamic(ops, lit, dist, final=True, rle=C.rle_verbatim if k % 2 else C.rle_greedy)
    assert d.hclens == [k]
    return d


def header_shapes():
    out = [member(hclen_member(k)) for k in range(5, 20)]
    rng = random.Random(105)
    # HLIT 257 and HDIST 1: literals only, the single distance length 0
    lit = lens_over(257, [65, 66, 67, 256])
    out.append(member(C.Deflate().dynamic([65, 66, 67, 67, 66], lit, [0], final=True)))
    # HLIT 286 and HDIST 30, symbols 285 and 29 used
    lit = lens_over(286, [65, 66, 67, 256, 257, 270, 285])
    dist = lens_over(30, [0, 5, 29])
    d = C.Deflate().stored(rng.randbytes(25000))
    d.dynamic([65, 66, (3, 1), (258, 24577), (25, 8), 67, (258, 25000), (3, 7)], lit, dist, final=True)
    out.append(member(d))
    # the longest and the shortest repeat of each kind, written out by hand
    lens = [0] * 162 + [4] * 15 + [0] * 79 + [4] + [0]
    rle = [(18, 138), (18, 11), (17, 10), (17, 3), 4, (16, 6), 4, (16, 3), 4, 4, 4, 4, (18, 79), 4, 0]
    assert C.rle_expand(rle) == lens and C.kraft(lens) == 32768
    ops = [rng.randrange(162, 177) for _ in range(200)]
    out.append(member(C.Deflate().dynamic(ops, lens[:257], lens[257:], final=True, rle=rle)))
    # a 16 repeat from the last literal/length length into the distance lengths
    lit = lens_over(259, [65, 256, 257, 258], [1, 2, 3, 3])
    dist = [3, 3, 3, 3, 1]
    rle = [(18, 65), 1, (18, 138), (18, 52), 2, 3, (16, 5), 1]
    assert C.rle_expand(rle) == lit + dist
    ops = [65] * 9 + [(4, 1), (3, 2), (4, 3), (3, 4), (4, 5), (3, 6), 65, (4, 2)]
    out.append(member(C.Deflate().dynamic(ops, lit, dist, final=True, rle=rle)))
    # an 18 repeat from the literal/length lengths into the distance lengths
    lit = lens_over(270, [65, 66, 256, 257], [1, 3, 3, 2])
    dist = [0, 0, 0, 1, 1]
    rle = [(18, 65), 1, 3, (18, 138), (18, 51), 3, 2, (18, 15), 1, 1]
    assert C.rle_expand(rle) == lit + dist
    ops = [65, 66, 66, 65, 66, 65, 65, (3, 4), (3, 5), (3, 6), 66]
    out.append(member(C.Deflate().dynamic(ops, lit, dist, final=True, rle=rle)))
    # a single one-bit distance code, used by matches
    lit = lens_over(258, [97, 256, 257])
    out.append(member(C.Deflate().dynamic([97, (3, 1), 97, (3, 1)], lit, [1], final=True)))
    # a block whose only code is a one-bit end-of-block, then more data
    d = C.Deflate().dynamic([], [0] * 256 + [1], [0]).fixed(list(b"after the empty block"), final=True)
    out.append(member(d))
    d = C.Deflate().fixed(list(b"before, ")).dynamic([], [0] * 256 + [1], [0]).stored(b"and after", final=True)
    out.append(member(d))
    return out


SMALL_LIT = lens_over(260, [97, 98, 99, 256, 257, 258, 259])
SMALL_DIST = lens_over(4, [0, 1, 2, 3])


def stored_blocks():
    rng = random.Random(106)
    out = []
    # empty stored blocks: first, in the middle, last
    d = C.Deflate().stored(b"").fixed(list(b"one")).stored(b"").stored(b"").fixed(list(b"two")).stored(b"", final=True)
    out.append(member(d))
    # the largest stored block a BGZF member holds
    out.append(member(C.Deflate().stored(rng.randbytes(65505), final=True)))
    # stored blocks of 1..8 bytes: the data ends at every alignment; then a fixed / a dynamic block
    d = C.Deflate()
    ends = set()
    for n in range(1, 9):
        for target in range(4):
            for follower in ("fixed", "dynamic"):
                while ((d.nbits + 3 + 7) // 8 + 4 + n) & 3 != target:
                    d.fixed([])  # ten bits
                d.stored(rng.randbytes(n))
                ends.add((follower, len(d.buf) & 3))
                if follower == "fixed":
                    d.fixed(list(rng.randbytes(5)) + [(4, 3)])
                else:
                    d.dynamic([97, 98, (5, 2), 99, (3, 4)], SMALL_LIT, SMALL_DIST)
    assert len(ends) == 8, ends
    out.append(member(d.fixed([], final=True)))
    # a stored block after a fixed block that ends at each of the 8 bit phases
    d = C.Deflate().stored(b"x")
    phases = set()
    for k in range(8):  # k nine-bit literals move the end by k bits
        d.fixed([65, 66] + [200 + k] * k)
        phases.add(d.nbits & 7)
        d.stored(rng.randbytes(3 + k))
    assert phases == set(range(8))
    out.append(member(d.fixed([], final=True)))
    # three stored blocks in a row
    d = C.Deflate().stored(rng.randbytes(700)).stored(rng.randbytes(3)).stored(rng.randbytes(1500), final=True)
    out.append(member(d))
    # matches that reach back into stored data, near and far
    d = C.Deflate().stored(rng.randbytes(5000)).fixed(list(rng.randbytes(100)) + [(258, 4900), (100, 5100), (3, 101)])
    d.stored(rng.randbytes(1000)).fixed([(258, 6000), (258, 1000), (17, 2300)], final=True)
    out.append(member(d))
    return out


def many_blocks():
    rng = random.Random(107)
    d = C.Deflate()
    for _ in range(2000):
        d.fixed([])
    d.fixed(list(rng.randbytes(300)) + [(200, 299)], final=True)
    out = [member(d)]
    d = C.Deflate()
    for i in range(300):
        d.stored(rng.randbytes(1 + i % 7))
        d.fixed(list(rng.randbytes(1 + i % 5)) + [(3 + i % 9, 1 + i % 6)])
        d.dynamic([97, 98, 99, (3 + i % 3, 1 + i % 4)], SMALL_LIT, SMALL_DIST)
    out.append(member(d.stored(b"", final=True)))
    return out


def framing():
    """isize 1, an empty member between others, and members whose compressed length varies mod 4 so
    that the members after them start at every alignment."""
    rng = random.Random(108)
    out = [member(C.Deflate().fixed([120], final=True))]
    for pad in (0, 1, 2, 3, 0, 2, 1, 3):
        d = C.Deflate()
        for _ in range(pad):
            d.stored(b"")
        d.stored(rng.randbytes(40)).fixed(list(rng.randbytes(9)) + [(30, 45)], final=True)
        out.append(member(d))
        if pad == 3:
            out.append(member(C.Deflate().fixed([], final=True)))  # isize 0
    return out


def _window_slice(W, i):
    return window_members(W)[0][i:i + 5]


def _window_builders():
    """window-W-k: five members of window_members(W) per file."""
    out = {}
    for W in WINDOWS:
        n = len(window_members(W)[0])
        for i in range(0, n, 5):
            out["window-%d-%d" % (W, i // 5)] = functools.partial(_window_slice, W, i)
    return out


VALID = {
    "overlap-all-dists": overlap_all_dists,
    "overlap-lengths-a": functools.partial(overlap_lengths, OVERLAP_DISTS[:5]),
    "overlap-lengths-b": functools.partial(overlap_lengths, OVERLAP_DISTS[5:]),
    **_window_builders(),
    "format-limits": format_limits,
    "long-codes": long_codes,
    "header-shapes": header_shapes,
    "stored-blocks": stored_blocks,
    "many-blocks": many_blocks,
    "framing": framing,
}


# ---------------------------------------------------------------- invalid members

def _bad(d, isize, pad=True):
    if pad:
        d.align()
        d.buf += bytes(8)  # whatever the decoder reads on after the fault is zeros, not the trailer
    return member(d, isize=isize)


def _header(hlit, hdist):
    d = C.Deflate().fixed([65, 66])
    d.bits(1, 1)
    d.bits(2, 2)
    d.bits(hlit, 5)
    d.bits(hdist, 5)
    d.bits(15, 4)
    return _bad(d, 100)


def _dyn(isize=100, ops=(), **kw):
    kw.setdefault("lit_lens", lens_over(257, [65, 66, 256], [1, 2, 2]))
    kw.setdefault("dist_lens", [0])
    if "cl_lens" in kw:  # a given code-length code has no repeat symbols unless the case brings its own
        kw.setdefault("rle", C.rle_verbatim)
    return _bad(C.Deflate().fixed([65, 66]).dynamic(None if ops is None else list(ops), final=True, **kw), isize)


def _btype3():
    d = C.Deflate().fixed([65, 66]).stored(b"")
    d.bits(1, 1)
    d.bits(3, 2)
    return _bad(d, 100)


def _truncated():
    rng = random.Random(109)
    d = C.Deflate().fixed(list(rng.randbytes(1000)), final=True)
    data = d.getvalue()
    return M(data[:len(data) // 2], None, zlib.crc32(bytes(d.payload)), 1000)


ST_BTYPE, ST_STORED, ST_COUNTS, ST_CODES, ST_LENS, ST_SYMBOL, ST_DIST, ST_SIZE = 1, 2, 3, 4, 5, 6, 7, 8

CL3 = lens_over(19, [0, 1, 2], [1, 2, 2])  # a complete code-length code for lengths 0, 1, 2

INVALID = {
    "btype-3": (_btype3, ST_BTYPE),
    "stored-nlen": (lambda: _bad(C.Deflate().fixed([65]).stored(b"abc", nlen=0x1234, final=True), 4), ST_STORED),
    "hlit-30": (lambda: _header(30, 0), ST_COUNTS),
    "hlit-31": (lambda: _header(31, 0), ST_COUNTS),
    "hdist-30": (lambda: _header(0, 30), ST_COUNTS),
    "hdist-31": (lambda: _header(0, 31), ST_COUNTS),
    "cl-oversubscribed": (lambda: _dyn(cl_lens=lens_over(19, [0, 1, 2], [1, 1, 1])), ST_CODES),
    "cl-incomplete": (lambda: _dyn(cl_lens=lens_over(19, [0, 1, 2], [1, 2, 3])), ST_CODES),
    "lit-oversubscribed": (lambda: _dyn(lit_lens=lens_over(257, [65, 66, 256], [1, 1, 1]), cl_lens=CL3), ST_CODES),
    "lit-incomplete-2bit": (lambda: _dyn(lit_lens=lens_over(257, [65, 256], [1, 2]), cl_lens=CL3), ST_CODES),
    "dist-incomplete-two": (lambda: _dyn(dist_lens=[2, 2], cl_lens=CL3), ST_CODES),
    "hclen-4": (lambda: _dyn(lit_lens=[0] * 257, rle=[(18, 138), (18, 120)], cl_lens=lens_over(19, [18, 0], [1, 1]),
                             ops=None), ST_LENS),
    "first-length-16": (lambda: _dyn(rle=[(16, 3), (18, 62), 1, 2, (18, 138), (18, 51), 2, 0],
                                     cl_lens=lens_over(19, [0, 1, 2, 16, 18], [2, 2, 2, 3, 3]), ops=None), ST_LENS),
    "repeat-past-end": (lambda: _dyn(rle=[(18, 65), 1, 2, (18, 138), (18, 51), 2, (18, 11)],
                                     cl_lens=lens_over(19, [1, 2, 18], [2, 2, 1]), ops=None), ST_LENS),
    "no-end-of-block": (lambda: _dyn(lit_lens=lens_over(257, [65, 66], [1, 1]), cl_lens=CL3, ops=None), ST_LENS),
    "fixed-symbol-286": (lambda: _bad(C.Deflate().fixed([65, ("sym", 286)], final=True), 100), ST_SYMBOL),
    "one-bit-unused-code": (lambda: _dyn(lit_lens=[0] * 256 + [1], ops=[("bits", 1, 1)], eob=False), ST_SYMBOL),
    "dist-pos-plus-1": (lambda: _bad(C.Deflate().fixed([65, 66, (3, 3)], final=True), 100), ST_DIST),
    "fixed-dist-30": (lambda: _bad(C.Deflate().fixed([65, ("sym", 257), ("dsym", 30)], final=True), 100), ST_DIST),
    "length-no-dist-set": (lambda: _dyn(lit_lens=lens_over(258, [97, 256, 257]), ops=[97, ("sym", 257)]), ST_DIST),
    "isize-literal-more": (lambda: _bad(C.Deflate().fixed([65, 66, 67], final=True), 2, pad=False), ST_SIZE),
    "isize-match-more": (lambda: _bad(C.Deflate().fixed([65, (3, 1)], final=True), 1, pad=False), ST_SIZE),
    "isize-stored-more": (lambda: _bad(C.Deflate().stored(b"abcd").stored(b"efgh", final=True), 4, pad=False), ST_SIZE),
    "isize-byte-fewer": (lambda: _bad(C.Deflate().fixed([65, 66, 67], final=True), 4, pad=False), ST_SIZE),
    "stored-past-end": (lambda: _bad(C.Deflate().stored(b"abc", length=200, final=True), 200, pad=False), ST_SIZE),
    "truncated": (_truncated, None),
}


def zlib_verdict(m):
    """How zlib and the BGZF trailer judge a member: None if it inflates, whole, to isize bytes;
    else the reason it is rejected."""
    z = zlib.decompressobj(-15)
    try:
        out = z.decompress(m.deflate)
    except zlib.error as e:
        return str(e)
    if not z.eof:
        return "truncated"
    if len(out) != m.isize:
        return "%d bytes, ISIZE %d" % (len(out), m.isize)
    return None


# ---------------------------------------------------------------- a BAM around the members

def carrier(raw, header_end, text_members, bad=None, level=6, block=65280):
    """A BAM whose header text is the payload of `text_members`; after it n_ref, the references and
    the records of the BAM payload `raw` (its header ending at `header_end`), deflated by zlib.
    `bad`: one more member, put before the last member of records (past the header's end, so the
    file reaches the device inflate).  Returns (file bytes, payload or None with `bad`, the file
    offsets of the members' deflate data)."""
    l_text = struct.unpack_from("<i", raw, 4)[0]
    text = b"".join(m.payload for m in text_members)
    head = b"BAM\1" + struct.pack("<i", len(text))
    rest = raw[8 + l_text:]
    mems = [M(_z(head, level), head, zlib.crc32(head), len(head))] + list(text_members)
    chunks = [rest[i:i + block] for i in range(0, len(rest), block)]
    assert len(rest) - len(chunks[-1]) > header_end - 8 - l_text, "the last member holds records only"
    for k, chunk in enumerate(chunks):
        if k == len(chunks) - 1 and bad is not None:
            mems.append(bad)
        mems.append(M(_z(chunk, level), chunk, zlib.crc32(chunk), len(chunk)))
    out, offs = bytearray(), []
    for m in mems:
        offs.append(len(out) + 18)
        out += bgzf(m)
    out += C.BGZF_EOF
    return bytes(out), None if bad is not None else head + text + rest, offs


def _z(chunk, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(chunk) + c.flush()
