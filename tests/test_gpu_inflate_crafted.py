"""The device inflate (sctools_amd/csrc/inflate.h k_inflate) on crafted deflate streams.

A compressor leaves most of the deflate format unused; deflate_cases.py reaches the rest -- long
codes, every overlapping copy, copies around every window size, the format's limits, odd headers,
stored blocks at every alignment -- and streams that must be rejected.  The reference is zlib plus
the plain-Python meaning of each member's ops (test_deflate_craft_cpu.py proves the two agree).

The members ride in a BAM as its header text (the device skips the text, the kernel still inflates
every member); after it come the references and records of small-cell-sorted.bam, so the stages
after the inflate see a file they know.  A member that must be rejected sits among the records'
members: a bad member in the header would be declined by the host's zlib before the kernel runs.
"""
import functools
import os
import re

import pytest

import deflate_cases as K
import helpers as H
from sctools_amd import gbam
from test_gbam import _header_end, payload, same_as_host

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _records():
    raw = payload(os.path.join(H.GOLDEN, "bam", "small-cell-sorted.bam"))
    return raw, _header_end(raw)


def _write(tmp_path, text_members, bad=None):
    raw, end = _records()
    data, whole, offs = K.carrier(raw, end, text_members, bad)
    path = str(tmp_path / "crafted.bam")
    with open(path, "wb") as f:
        f.write(data)
    return path, whole, offs


@pytest.mark.parametrize("name", list(K.VALID))
def test_valid_members(tmp_path, name):
    members = K.VALID[name]()
    path, whole, offs = _write(tmp_path, members)
    got = gbam.inflate(path)
    assert got is not None, gbam.last_error()
    at = 8
    for i, m in enumerate(members):  # member by member, so a failure names the member
        assert got[at:at + m.isize] == m.payload, (name, i)
        at += m.isize
    assert got == whole
    same_as_host(path, "cell")
    if name == "framing":  # members began at every alignment of the compressed words
        assert {o & 3 for o in offs[1:1 + len(members)]} == {0, 1, 2, 3}
        assert 0 in [m.isize for m in members[1:-1]] and members[0].isize == 1


@pytest.mark.parametrize("name", list(K.INVALID))
def test_invalid_member_declines_with_its_status(tmp_path, name):
    build, status = K.INVALID[name]
    path, _, _ = _write(tmp_path, [], build())
    assert gbam.inflate(path) is None
    found = re.search(r"status mask 0x([0-9a-f]+)", gbam.last_error())
    assert found, gbam.last_error()  # declined by the kernel, not before it
    mask = int(found.group(1), 16)
    if status is None:
        assert mask != 0
    else:
        assert mask == 1 << status, (name, "0x%x" % mask)
    assert gbam.decode(path, "cell") is None
    assert "status mask 0x%x" % mask in gbam.last_error()
