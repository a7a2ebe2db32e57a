"""TagSort's decoder choice, the parts that need no GPU: the binding of sct_gbam_parse_tagsort, the
``decoder`` argument and option, and ``Ranked`` on host columns."""
import ctypes

import numpy as np
import pytest

from sctools_amd import gbam, tagsort


def test_parse_tagsort_is_bound():
    assert "sct_gbam_parse_tagsort" in gbam.EXPORTED
    restype, argtypes = gbam.PROTOTYPES["sct_gbam_parse_tagsort"]
    assert restype is ctypes.c_int
    assert argtypes == [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
    assert argtypes == gbam.PROTOTYPES["sct_gbam_parse_count"][1]  # the same shape of call


def test_decoder_argument(tmp_path):
    bam = tmp_path / "in.bam"
    bam.write_bytes(b"x")
    with pytest.raises(ValueError, match="decoder must be"):
        tagsort.TagSort(str(bam), "gene", "CB", "UB", "GE", decoder="bogus")
    with pytest.raises(NotImplementedError, match="no device-only mode"):
        tagsort.TagSort(str(bam), "gene", "CB", "UB", "GE", decoder="device")
    for decoder in ("auto", "host"):
        ts = tagsort.TagSort(str(bam), "gene", "CB", "UB", "GE", decoder=decoder)
        assert ts.decoder == decoder and ts.decoded_by is None


def _argv(tmp_path, *more):
    bam = tmp_path / "in.bam"
    bam.write_bytes(b"x")
    # --temp-folder is missing: the option checks stop the run after the arguments were parsed
    return ["--bam-input", str(bam), "--metric-type", "gene", "--metric-output", str(tmp_path / "m.csv"),
            "--compute-metric", "--barcode-tag", "CB", "--umi-tag", "UB", "--gene-tag", "GE",
            "--temp-folder", str(tmp_path / "none")] + list(more)


def test_cli_decoder_option(tmp_path, capsys):
    with pytest.raises(tagsort.TagSortError, match="temp folder .* is missing"):
        tagsort.main(_argv(tmp_path, "--decoder", "host"))
    with pytest.raises(tagsort.TagSortError, match="temp folder .* is missing"):
        tagsort.main(_argv(tmp_path))
    with pytest.raises(SystemExit):
        tagsort.main(_argv(tmp_path, "--decoder", "device"))
    assert "--decoder" in capsys.readouterr().err


def test_ranked_on_host_columns_is_unchanged():
    arrays = {"cell": np.array([0, 1, 2], dtype=np.int32), "umi": np.array([0, 0, 1], dtype=np.int32),
              "gene": np.array([1, 2, 0], dtype=np.int32)}
    names3 = [[None, "AAA", "B"], [None, "u"], [None, "G1,G2", "mt"]]
    r = tagsort.Ranked(arrays, names3, ("gene", "barcode", "umi"), "gene", {"u"})
    assert r.names[0] == ["G1,G2", "None", "mt"] and r.first_drop.tolist() == [1, 1, 0]
    assert r.columns["cell"].tolist() == [0, 2, 1] and r.columns["umi"].tolist() == [2, 0, 1]
    assert r.names[2] == ["None", "u"] and r.third_is_mito.tolist() == [0, 1]
    for c in ("cell", "umi", "gene"):
        assert isinstance(r.columns[c], np.ndarray) and r.columns[c].dtype == np.int32
    assert tagsort.Ranked(arrays, names3, ("gene", "barcode", "umi"), "cell").first_drop.tolist() == [0, 1, 0]
    empty = {c: np.zeros(0, dtype=np.int32) for c in arrays}
    assert tagsort.Ranked(empty, [[], [], []], tagsort.ROLES, "gene").columns["cell"].shape == (0,)


def test_ranked_renumbers_tensors_where_they_lie():
    import torch

    arrays = {"cell": np.array([0, 1, 2, 2], dtype=np.int32), "umi": np.array([0, 0, 1, 1], dtype=np.int32),
              "gene": np.array([1, 2, 0, 2], dtype=np.int32)}
    names3 = [[None, "AAA", "B"], [None, "u"], [None, "G1,G2", "mt"]]
    for roles in (tagsort.ROLES, ("gene", "barcode", "umi"), ("umi", "gene", "barcode")):
        want = tagsort.Ranked(arrays, names3, roles, "gene")
        got = tagsort.Ranked({c: torch.from_numpy(a) for c, a in arrays.items()}, names3, roles, "gene")
        assert got.names == want.names
        for c in arrays:
            assert torch.is_tensor(got.columns[c]) and got.columns[c].dtype == torch.int32
            assert got.columns[c].tolist() == want.columns[c].tolist()
    none = tagsort.Ranked({c: torch.zeros(0, dtype=torch.int32) for c in arrays}, [[], [], []], tagsort.ROLES, "gene")
    assert none.columns["umi"].shape == (0,)
