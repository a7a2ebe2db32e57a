"""The C ABI of include/sct_fastq_process.h: the exports, the prototype table, and the argument errors.
A call that returns an error launches nothing, so the argument checks run without a GPU on made-up
addresses; the GPU test repeats them on real buffers and looks at the buffers afterwards."""
import ctypes
import os
import re

import pytest

from sctools_amd import fastq, fastq_process as fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESIZE = -1, -2
A = 0x7f0000001000  # a made-up address, 4096-byte aligned; no call that fails reads it


def test_the_prototype_table_is_the_header_and_the_library():
    text = open(os.path.join(ROOT, "include", "sct_fastq_process.h")).read()
    names = sorted(set(re.findall(r"^(?:const\s+)?\w+[\s*]+(sct_fqp_\w+)\(", text, flags=re.M)))
    assert names == sorted(fp.PROTOTYPES) and len(names) == 6
    assert fp.EXPORTED == tuple(fp.PROTOTYPES)
    lib = fp.load()
    assert lib is fastq.load()  # one library, opened once
    for name, (restype, argtypes) in fp.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_the_struct_is_the_headers():
    # int64 n; (pointer, int64, pointer, pointer) twice; 7 pointers; 4 x int32
    assert ctypes.sizeof(fp.Records) == 8 + 2 * 32 + 7 * 8 + 16
    assert fp.Records.n_shards.offset == 8 + 2 * 32 + 7 * 8 + 8


def shard_call(lib, raw=A, corrected=None, index=None, n=10, length=16, n_shards=4, shard=A + 4096, counts=A + 8192):
    return lib.sct_fqp_shard(raw, corrected, index, n, length, n_shards, shard, counts, None)


def records(**kw):
    base = dict(n=10, r2_text=A, r2_bytes=1000, r2_off=A + 4096, r2_len=A + 8192, i1_text=None, i1_bytes=0, i1_off=None,
                i1_len=None, cr=A, cy=A, ur=A, uy=A, cb=None, cb_index=None, shard=A + 12288, cell_length=16,
                umi_length=10, n_shards=4, format=fp.BAM)
    base.update(kw)
    return fp.Records(**base)


def failing_calls(lib):
    """(what, call) pairs that must all return EINVAL."""
    size = ctypes.c_size_t(0)
    yield "shard n_shards 0", lambda: shard_call(lib, n_shards=0)
    yield "shard n_shards 1025", lambda: shard_call(lib, n_shards=1025)
    yield "shard L 32", lambda: shard_call(lib, length=32)
    yield "shard L 0", lambda: shard_call(lib, length=0)
    yield "shard raw misaligned", lambda: shard_call(lib, raw=A + 8)
    yield "shard corrected misaligned", lambda: shard_call(lib, corrected=A + 4, index=A)
    yield "shard corrected without index", lambda: shard_call(lib, corrected=A)
    yield "shard index misaligned", lambda: shard_call(lib, corrected=A, index=A + 2)
    yield "shard shard misaligned", lambda: shard_call(lib, shard=A + 2)
    yield "shard counts misaligned", lambda: shard_call(lib, counts=A + 4)
    yield "shard negative n", lambda: shard_call(lib, n=-1)
    yield "plan size n_shards 0", lambda: lib.sct_fqp_plan_workspace_size(10, 0, fp.BAM, ctypes.byref(size))
    yield "plan size n_shards 1025", lambda: lib.sct_fqp_plan_workspace_size(10, 1025, fp.BAM, ctypes.byref(size))
    yield "plan size format", lambda: lib.sct_fqp_plan_workspace_size(10, 4, 2, ctypes.byref(size))
    plan = (lambda rec, work=A, nbytes=1 << 20, offsets=A, counts=A, sizes=A:
            lib.sct_fqp_plan(ctypes.byref(rec), work, nbytes, offsets, counts, sizes, None))
    yield "plan n_shards 0", lambda: plan(records(n_shards=0))
    yield "plan n_shards 1025", lambda: plan(records(n_shards=1025))
    yield "plan cell_length 32", lambda: plan(records(cell_length=32))
    yield "plan lines misaligned", lambda: plan(records(r2_off=A + 4))
    yield "plan lengths misaligned", lambda: plan(records(r2_len=A + 2))
    yield "plan shard misaligned", lambda: plan(records(shard=A + 1))
    yield "plan half an I1", lambda: plan(records(i1_text=A))
    yield "plan cb without index", lambda: plan(records(cb=A))
    yield "plan workspace misaligned", lambda: plan(records(), work=A + 4)
    yield "plan offsets misaligned", lambda: plan(records(), offsets=A + 4)
    emit = (lambda rec, offsets=A, base=A, out=A, error=A:
            lib.sct_fqp_emit_bam(ctypes.byref(rec), offsets, base, out, 1 << 20, error, None))
    yield "emit n_shards 1025", lambda: emit(records(n_shards=1025))
    yield "emit fastq records", lambda: emit(records(format=fp.FASTQ))
    yield "emit offsets misaligned", lambda: emit(records(), offsets=A + 4)
    yield "emit error misaligned", lambda: emit(records(), error=A + 4)
    yield "emit_fastq bam records", lambda: lib.sct_fqp_emit_fastq(ctypes.byref(records()), A, A, A, 10, A, 10, A, None)
    yield "lines text misaligned", lambda: lib.sct_fqp_lines(A + 8, 100, 1, A, 1 << 20, A, A, A, A, None)
    yield "lines offsets misaligned", lambda: lib.sct_fqp_lines(A, 100, 1, A, 1 << 20, A + 4, A, A, A, None)
    yield "lines lengths misaligned", lambda: lib.sct_fqp_lines(A, 100, 1, A, 1 << 20, A, A + 2, A, A, None)
    yield "lines too many records", lambda: lib.sct_fqp_lines(A, 100, 100, A, 1 << 20, A, A, A, A, None)


def test_argument_errors_return_einval_with_a_message():
    lib = fp.load()
    seen = 0
    for what, call in failing_calls(lib):
        assert call() == EINVAL, what
        assert fp.LIBRARY.last_error(), what
        seen += 1
    assert seen > 30
    with pytest.raises(fp.FastqProcessError, match="sct_fastq_process error -1: n_shards 1025 outside 1..1024"):
        fp.check(shard_call(lib, n_shards=1025))
    assert lib.sct_fqp_plan(ctypes.byref(records()), A, 16, A, A, A, None) == ESIZE  # a workspace too small
    size = ctypes.c_size_t(0)
    assert lib.sct_fqp_plan_workspace_size(1000, 7, fp.BAM, ctypes.byref(size)) == 0
    assert size.value == 4 * 7 * 12  # four tiles of 256 records: a count and a byte total per shard
    assert lib.sct_fqp_plan_workspace_size(1000, 7, fp.FASTQ, ctypes.byref(size)) == 0 and size.value == 4 * 7 * 20


@pytest.mark.gpu
def test_a_failing_call_leaves_its_buffers_alone():
    import torch

    lib = fp.load()
    n = 64
    raw = torch.full((n, 16), 65, dtype=torch.uint8, device="cuda")
    shard = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for kw in (dict(n_shards=0), dict(n_shards=1025), dict(length=32), dict(raw=raw.data_ptr() + 8),
               dict(shard=shard.data_ptr() + 2), dict(counts=counts.data_ptr() + 4)):
        args = dict(raw=raw.data_ptr(), n=n, shard=shard.data_ptr(), counts=counts.data_ptr())
        args.update(kw)
        length = args.pop("length", 16)
        assert lib.sct_fqp_shard(args["raw"], None, None, args["n"], length, args.get("n_shards", 4), args["shard"],
                                 args["counts"], stream) == EINVAL, kw
    torch.cuda.synchronize()
    assert shard.cpu().tolist() == [-7] * n and counts.cpu().tolist() == [-7] * 3
    assert lib.sct_fqp_shard(raw.data_ptr(), None, None, n, 16, 4, shard.data_ptr(), counts.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [0, 0, n] and set(shard.cpu().tolist()) == {fp.std_hash(b"A" * 16) % 4}
