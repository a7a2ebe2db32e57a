"""sctools_amd._ffi: the one loader, error path and set of torch helpers of the seven bindings (no GPU).

Every binding's prototype table must name exactly what its header declares and what its library
exports; ``check`` must raise the module's error class with the library's message; a missing file
must raise the one documented ImportError; ``device`` must refuse to run without a GPU for every
spelling it accepts; ``read_dictionary`` must give the names of the pure-Python decoder.
"""
import ctypes
import os
import re

import pytest

import helpers as H
from sctools_amd import (_ffi, _native, bamnative, barcode, columnar, csvnative, engine, fastq, fastq_metrics,
                         gbam)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BINDINGS = [(_native, "sctools_gpu.h", "sct_"), (bamnative, "sct_bam.h", "sct_bam_"), (csvnative, "sct_csv.h", "sct_csv_"),
            (gbam, "sct_gbam.h", "sct_gbam_"), (barcode, "sct_barcode.h", "sct_bc_"), (fastq, "sct_fastq.h", "sct_fq_"),
            (fastq_metrics, "sct_fastq_metrics.h", "sct_fqm_")]


def declared_functions(header: str, prefix: str):
    """The functions a header declares: a return type at the start of a line, then the name."""
    text = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"^(?:const\s+)?\w+[\s*]+(%s\w+)\(" % prefix, text, flags=re.M)))


@pytest.mark.parametrize("module,header,prefix", BINDINGS, ids=[m.__name__.split(".")[-1] for m, _, _ in BINDINGS])
def test_prototype_table_is_the_header_and_the_library(module, header, prefix):
    names = declared_functions(header, prefix)
    assert len(names) >= 4
    assert names == sorted(module.PROTOTYPES)  # a missing or an extra name fails
    assert module.EXPORTED == tuple(module.PROTOTYPES)
    lib = module.load()
    assert lib is module.load()  # cached
    for name, (restype, argtypes) in module.PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError: the library does not export it
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_the_helper_sees_a_missing_and_an_extra_name():
    names = declared_functions("sct_fastq.h", "sct_fq_")
    assert names != sorted(list(fastq.PROTOTYPES) + ["sct_fq_more"])
    assert names != sorted(list(fastq.PROTOTYPES)[1:])


def test_fastq_metrics_shares_the_open_fastq_library():
    assert fastq_metrics.load() is fastq.load()
    assert fastq_metrics.LIBRARY.path == fastq.LIB_PATH


def _bad_engine_plan(lib):
    plan = _native.Plan(n_records=10, mode=7, float_mode=0, n_cell_ids=1, n_gene_ids=1, n_umi_ids=1)
    return lib.sct_workspace_size(ctypes.byref(plan), ctypes.byref(ctypes.c_size_t(0)))


def _bad_bam_path(lib):
    h, bad = ctypes.c_void_p(), ctypes.c_int64(-1)
    return lib.sct_bam_decode_tags(b"/nonexistent/none.bam", 0, b"CBUBGE", 1, ctypes.byref(h), ctypes.byref(bad))


CHECKS = [
    (_native, _native.EngineError, "sctools_gpu error %d: %s", _bad_engine_plan),
    (bamnative, OSError, None, _bad_bam_path),  # the rc -> exception map: the message alone
    (gbam, OSError, "device BAM decode failed (%d): %s",
     lambda lib: lib.sct_gbam_part_bounds(None, ctypes.byref(ctypes.c_int64()), ctypes.byref(ctypes.c_int64()))),
    (barcode, barcode.BarcodeError, "sct_barcode error %d: %s",
     lambda lib: lib.sct_bc_table_size(-1, ctypes.byref(ctypes.c_size_t(0)))),
    (fastq, fastq.FastqError, "sct_fastq error %d: %s",
     lambda lib: lib.sct_fq_workspace_size(-1, ctypes.byref(ctypes.c_size_t(0)))),
    (fastq_metrics, fastq_metrics.FastqMetricsError, "sct_fastq_metrics error %d: %s",
     lambda lib: lib.sct_fqm_table_size(3, ctypes.byref(ctypes.c_size_t(0)))),
]


@pytest.mark.parametrize("module,error_class,form,provoke", CHECKS, ids=[c[0].__name__.split(".")[-1] for c in CHECKS])
def test_check_raises_the_modules_error_with_the_librarys_message(module, error_class, form, provoke):
    library = module.LIBRARY
    lib = module.load()
    library.check(0)
    rc = provoke(lib)
    assert rc not in library.accept
    message = library.last_error()
    assert message  # the library said why
    with pytest.raises(error_class) as e:
        library.check(rc)
    assert type(e.value) is error_class
    assert str(e.value) == (message if form is None else form % (rc, message))
    with pytest.raises(error_class, match="read earlier"):  # a message the caller read on the calling thread
        library.check(rc, "read earlier")


def test_gbam_host_code_is_no_error():
    gbam.LIBRARY.check(gbam.HOST)
    assert bamnative.LIBRARY.exceptions[bamnative.KEYERROR] is KeyError


def test_missing_library_raises_one_import_error(tmp_path):
    path = str(tmp_path / "libsct_nowhere.so")
    library = _ffi.Library(path, "sct_nowhere", "sct_nowhere_last_error", RuntimeError, {"f": (ctypes.c_int, [])})
    assert library.path == path and not library.available()
    with pytest.raises(ImportError) as e:
        library.load()
    assert path in str(e.value) and "__graft_entry__" in str(e.value) and "build()" in str(e.value)


def test_library_path_overrides(monkeypatch, tmp_path):
    monkeypatch.setenv("SCT_FFI_TEST_PATH", str(tmp_path / "other.so"))
    assert _ffi.Library("libx.so", "x", None, RuntimeError, {}, env_override="SCT_FFI_TEST_PATH").path == \
        str(tmp_path / "other.so")
    monkeypatch.delenv("SCT_FFI_TEST_PATH")
    assert _ffi.Library("libx.so", "x", None, RuntimeError, {}, env_override="SCT_FFI_TEST_PATH").path == \
        os.path.join(os.path.dirname(_ffi.__file__), "libx.so")
    assert _native.LIBRARY.mode == ctypes.RTLD_GLOBAL and "sct_bin_records" in _native.LIBRARY.optional


def test_an_optional_name_may_be_absent(tmp_path):
    table = dict(csvnative.PROTOTYPES, sct_csv_not_yet=(ctypes.c_int, []))
    with pytest.raises(AttributeError):
        _ffi.Library(csvnative.LIB_PATH, "sct_csv", None, RuntimeError, table).load()
    lib = _ffi.Library(csvnative.LIB_PATH, "sct_csv", None, RuntimeError, table, optional=("sct_csv_not_yet",)).load()
    assert lib.sct_csv_free.argtypes == [ctypes.c_void_p]


def test_device_without_a_gpu_has_no_cpu_fallback(monkeypatch):
    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for spelling in (None, 0, "0", "cuda", "cuda:0", torch.device("cuda", 0)):
        with pytest.raises(RuntimeError, match="needs a ROCm GPU .* no CPU fallback"):
            _ffi.device(spelling)
    assert engine._device is _ffi.device and gbam._device is _ffi.device and barcode._device is _ffi.device


def test_ptr_is_null_for_none_and_for_an_empty_tensor():
    import torch

    t = torch.zeros(4, dtype=torch.uint8)
    assert _ffi.ptr(None) is None and _ffi.ptr(t[:0]) is None
    assert _ffi.ptr(t).value == t.data_ptr()


@pytest.mark.parametrize("name", ["small-cell-sorted", "cell-sorted-missing-cb"])
def test_read_dictionary_gives_the_python_decoders_names(name):
    want = H.bam_columns(name, "cell")
    path = os.path.join(H.GOLDEN, "bam", name + ".bam")
    lib = bamnative.load()
    h, bad = ctypes.c_void_p(), ctypes.c_int64(-1)
    bamnative.check(lib.sct_bam_decode_tags(os.fsencode(path), bamnative.CELL_METRICS, b"CBUBGE", 1, ctypes.byref(h),
                                            ctypes.byref(bad)))
    try:
        got = []
        for which, ref in enumerate((want.cells, want.umis, want.genes)):
            raw, offsets, has_none = _ffi.read_dictionary(lib.sct_bam_dictionary, h, which)
            assert offsets.dtype.kind == "i" and offsets.itemsize == 8 and len(offsets) == len(ref.names) + 1
            assert offsets[0] == 0 and offsets[-1] == len(raw) and has_none == (ref.names[0] is None)
            got.append(columnar.PackedDictionary(raw, offsets, has_none).names)
            count_only = _ffi.read_dictionary(lib.sct_bam_dictionary, h, which, strings=False)
            assert count_only[0] == b"" and list(count_only[1]) == list(offsets)
    finally:
        lib.sct_bam_close(h)
    assert got == [want.cells.names, want.umis.names, want.genes.names]
    assert got == bamnative.decode(path, "cell")[1]
