"""The reference side of the crafted deflate cases (deflate_craft.py, deflate_cases.py), no GPU.

Every valid member must inflate with zlib to exactly the bytes its ops mean; every invalid member
must be rejected by zlib (or by its ISIZE); test_gpu_inflate_crafted.py then holds the device
inflate to the same verdicts.  Also here: the arithmetic of the kernel's overlapping copy, on numpy.
"""
import os
import zlib

import numpy as np
import pytest

import deflate_cases as K
import deflate_craft as C
import helpers as H
from test_gbam import _header_end, payload

# what zlib says for a member the device reports with this status
ZLIB_SAYS = {
    K.ST_BTYPE: ("invalid block type",),
    K.ST_STORED: ("invalid stored block lengths",),
    K.ST_COUNTS: ("too many length or distance symbols",),
    K.ST_CODES: ("invalid code lengths set", "invalid literal/lengths set", "invalid distances set"),
    K.ST_LENS: ("invalid bit length repeat", "missing end-of-block"),
    K.ST_SYMBOL: ("invalid literal/length code",),
    K.ST_DIST: ("invalid distance too far back", "invalid distance code"),
    K.ST_SIZE: ("ISIZE", "truncated"),
    None: ("truncated",),
}


def test_writer_against_zlib_on_plain_blocks():
    data = bytes(range(256)) * 3
    ops = list(data) + [(258, 1), (3, 768), (100, 256)]
    want = bytes(C.apply(ops))
    assert want[:768] == data and want[768:1026] == data[-1:] * 258
    lit, dist = [8] * 148 + [9] * 108 + [7] * 24 + [8] * 6, [4] * 2 + [5] * 28  # complete without 286, 287, 30, 31
    assert C.kraft(lit) == C.kraft(dist) == C.kraft(C.FIXED_LIT) == C.kraft(C.FIXED_DIST) == 32768
    for d in (C.Deflate().fixed(ops, final=True),
              C.Deflate().dynamic(ops, lit, dist, final=True),
              C.Deflate().dynamic(ops, lit, dist, final=True, rle=C.rle_verbatim),
              C.Deflate().stored(data).fixed(ops[768:], final=True)):
        assert zlib.decompress(d.getvalue(), -15) == want == bytes(d.payload)
    assert C.rle_expand(C.rle_greedy(C.FIXED_LIT + C.FIXED_DIST)) == C.FIXED_LIT + C.FIXED_DIST
    assert C.canonical([2, 1, 3, 3]) == {0: (2, 2), 1: (0, 1), 2: (6, 3), 3: (7, 3)}  # RFC 1951 3.2.2's method


def test_largest_stored_block():
    """65535 bytes: more than a BGZF member holds, so only zlib sees this one."""
    data = os.urandom(65535)
    d = C.Deflate().fixed([1, 2, 3]).stored(data, final=True)
    assert zlib.decompress(d.getvalue(), -15) == b"\1\2\3" + data


@pytest.mark.parametrize("name", list(K.VALID))
def test_valid_members_inflate_to_their_ops(name):
    members = K.VALID[name]()
    assert members
    for i, m in enumerate(members):
        assert len(m.deflate) + 26 <= 65536 and m.isize == len(m.payload) <= 65536
        assert K.zlib_verdict(m) is None, (name, i, K.zlib_verdict(m))
        assert zlib.decompress(m.deflate, -15) == m.payload, (name, i)
        assert zlib.crc32(m.payload) == m.crc


@pytest.mark.parametrize("name", list(K.INVALID))
def test_invalid_members_are_rejected(name):
    build, status = K.INVALID[name]
    m = build()
    assert m.payload is None and m.isize > 0  # (a member of ISIZE 0 is never inflated)
    verdict = K.zlib_verdict(m)
    assert verdict is not None, name
    assert any(s in verdict for s in ZLIB_SAYS[status]), (name, status, verdict)


def test_invalid_table_covers_every_status_but_overrun():
    assert {st for _, st in K.INVALID.values()} == {1, 2, 3, 4, 5, 6, 7, 8, None}


@pytest.mark.parametrize("W", K.WINDOWS)
def test_window_cases_are_complete(W):
    """Every (dist, len) of the list at every flush phase, and each where it was meant to be."""
    members, issued = K.window_members(W)
    q = W // 4
    want = {(d, n, ph) for d in K.window_dists(W) for n in K.WINDOW_LENS for ph in (0, 1, q - 1)}
    assert {(d, n, pos % q) for d, n, pos in issued} == want
    assert all(d <= pos for d, n, pos in issued)
    assert sum(len(K.VALID[k]()) for k in K.VALID if k.startswith("window-%d-" % W)) == len(members)


def test_long_code_sets_have_every_class_at_9_10_12_15():
    a, b = K.long_codes()
    assert a.payload == b.payload and a.deflate != b.deflate
    lit, dist = K.long_code_sets(7)
    for cls in (range(256), range(257, 286)):
        assert {9, 10, 12, 15} <= {lit[s] for s in cls}
    assert sorted(n for n in dist if n) == K.LONG_DIST


def test_carrier_is_the_same_bam_to_the_host_decoder(tmp_path):
    """Crafted members as the header text: the host decoder reads the same records as from the
    original file, and the members' payloads concatenate to the expected bytes."""
    from sctools_amd import bamnative

    src = os.path.join(H.GOLDEN, "bam", "small-cell-sorted.bam")
    raw = payload(src)
    data, whole, offs = K.carrier(raw, _header_end(raw), K.framing())
    path = str(tmp_path / "c.bam")
    open(path, "wb").write(data)
    assert payload(path) == whole
    assert {o & 3 for o in offs} == {0, 1, 2, 3}
    want, want_names = bamnative.decode(src, "cell")
    got, names = bamnative.decode(path, "cell")
    assert names == want_names
    for c, a in want.items():
        assert np.array_equal(got[c], a), c


def _overlap_index(j, dist, rcp):
    """inflate.h's source index of byte j of an overlapping copy, in its own number formats:
    (quotient-only result, result after the two corrections), as uint32."""
    q = (j.astype(np.float32) * rcp).astype(np.uint32)  # float -> unsigned truncates
    r0 = (j - q * dist).astype(np.uint32)
    r = np.where(r0.view(np.int32) < 0, r0 + dist, r0).astype(np.uint32)
    r = np.where(r >= dist, r - dist, r).astype(np.uint32)
    return r0, r


def test_overlap_index_arithmetic():
    """j mod dist from a float reciprocal: right for every j < 258 and dist in 1..257 with the
    reciprocal off by up to 2 ulp either way, and only thanks to the corrections: the bare quotient
    is wrong for some pairs even with the correctly rounded reciprocal."""
    j, dist = np.meshgrid(np.arange(258, dtype=np.uint32), np.arange(1, 258, dtype=np.uint32))
    exact = np.float32(1) / dist.astype(np.float32)  # correctly rounded
    want = j % dist
    bare_wrong = 0
    for ulp in range(-2, 3):
        rcp = exact.copy()
        for _ in range(abs(ulp)):
            rcp = np.nextafter(rcp, np.float32(np.inf if ulp > 0 else 0))
        r0, r = _overlap_index(j, dist, rcp)
        assert np.array_equal(r, want), ulp
        if ulp == 0:
            bare_wrong = int((r0 != want).sum())
    assert bare_wrong > 0
