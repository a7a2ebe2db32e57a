"""
ctypes binding of ``libsctools_gpu.so`` (declared in ``include/sctools_gpu.h``).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc,
``--offload-arch=gfx950``).  There is no CPU fallback: if the shared library
is missing, importing the engine raises immediately.
"""

import ctypes

from sctools_amd import _ffi

SCT_ABI_VERSION = 2
SCT_NI, SCT_NF, SCT_NP = 24, 12, 64
SCT_P_FLOAT_BASE, SCT_P_STREAM_LANES = 24, 8
SCT_ENOMEM = -3

MODE_CELL, MODE_GENE, MODE_GENE_GROUPED = 0, 1, 2
FLOAT_EXACT_SUM, FLOAT_WELFORD = 0, 1

# output int columns
I_N_READS, I_NOISE_READS, I_PERFECT_UMI, I_EXONIC, I_INTRONIC, I_UTR = 0, 1, 2, 3, 4, 5
I_UNIQUE, I_MULTIPLE, I_DUP, I_SPLICED, I_ANTISENSE = 6, 7, 8, 9, 10
I_N_MOL, I_N_FRAG, I_FRAG_SINGLE, I_MOL_SINGLE = 11, 12, 13, 14
I_PERFECT_CB, I_INTERGENIC, I_UNMAPPED, I_TOO_MANY_LOCI = 15, 16, 17, 18
I_N_K1, I_K1_MULTI, I_MITO_GENES, I_MITO_READS, I_ENTITY = 19, 20, 21, 22, 23
# output float columns
F_UY_MEAN, F_UY_VAR, F_GQF_MEAN, F_GQF_VAR, F_GQ_MEAN, F_GQ_VAR = 0, 1, 2, 3, 4, 5
F_RPM, F_RPF, F_FPM, F_CY_VAR, F_CY_MEAN, F_PCT_MITO = 6, 7, 8, 9, 10, 11

# native TagSort rows (sct_tagsort_metrics): int columns, then [stream][count, sum, sum2]
SCT_TS_NI, SCT_TS_NF = 21, 12
(TS_N_READS, TS_PERFECT_UMI, TS_EXONIC, TS_INTRONIC, TS_UTR, TS_UNIQUE, TS_MULTIPLE, TS_DUP, TS_SPLICED, TS_N_MOL,
 TS_N_FRAG, TS_FRAG_SINGLE, TS_MOL_SINGLE, TS_PERFECT_CB, TS_INTERGENIC, TS_UNMAPPED, TS_MITO_READS, TS_N_K1,
 TS_K1_MULTI, TS_MITO_GENES, TS_NAME) = range(21)
TS_S_UY, TS_S_GQF, TS_S_GQ, TS_S_CY = 0, 1, 2, 3

RECORD_COLUMNS = ("cell", "umi", "gene", "ref", "pos", "gq_sum", "gq_len", "gq_gt30", "bits", "xf",
                  "cy_gt30", "cy_len", "uy_gt30", "uy_len")

SCT_MAX_BINS = 256
ORDER_CELL, ORDER_CELL_UMI_GENE, ORDER_GENE_CELL_UMI = 0, 1, 2
PLAN_GENE_PARTIALS = 0x1


class Records(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int64)] + [(c, ctypes.c_void_p) for c in RECORD_COLUMNS]


class Plan(ctypes.Structure):
    _fields_ = [
        ("n_records", ctypes.c_int64),
        ("max_entities", ctypes.c_int64),
        ("mode", ctypes.c_int32),
        ("float_mode", ctypes.c_int32),
        ("n_cell_ids", ctypes.c_int32),
        ("n_gene_ids", ctypes.c_int32),
        ("n_umi_ids", ctypes.c_int32),
        ("flags", ctypes.c_int32),
    ]


COUNT_SKIP, COUNT_UNKNOWN = -1, -2


class CountInput(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_int64),
        ("cell", ctypes.c_void_p),
        ("umi", ctypes.c_void_p),
        ("gene", ctypes.c_void_p),
        ("xf", ctypes.c_void_p),
        ("qhead", ctypes.c_void_p),
        ("n_cell_ids", ctypes.c_int32),
        ("n_umi_ids", ctypes.c_int32),
        ("n_gene_ids", ctypes.c_int32),
        ("cell_none", ctypes.c_int32),
        ("umi_none", ctypes.c_int32),
        ("gene_col", ctypes.c_void_p),
        ("n_cols", ctypes.c_int32),
    ]


class CountOutput(ctypes.Structure):
    _fields_ = [
        ("row_cell", ctypes.c_void_p),
        ("indptr", ctypes.c_void_p),
        ("indices", ctypes.c_void_p),
        ("data", ctypes.c_void_p),
        ("n_rows", ctypes.c_int64),
        ("nnz", ctypes.c_int64),
        ("unknown_record", ctypes.c_int64),
        ("n_sorted", ctypes.c_int64),
    ]


class EngineError(RuntimeError):
    """A C-ABI call returned an error code (message from sct_last_error)."""


_P = ctypes.POINTER
_vp, _i64, _i32, _int, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_size_t
_plan, _rec = _P(Plan), _P(Records)

PROTOTYPES = {
    "sct_abi_version": (_int, []),
    "sct_last_error": (ctypes.c_char_p, []),
    "sct_workspace_size": (_int, [_plan, _P(_sz)]),
    "sct_count_entities": (_int, [_plan, _rec, _vp, _sz, _P(_i64), _vp]),
    "sct_compute_metrics": (_int, [_plan, _rec, _vp, _vp, _vp, _sz, _vp, _vp, _i64, _P(_i64), _vp]),
    "sct_gene_partials": (_int, [_plan, _rec, _vp, _sz, _vp, _vp]),
    "sct_cell_metrics_gene_partials": (_int, [_plan, _rec, _vp, _vp, _sz, _vp, _vp, _i64, _P(_i64), _vp, _vp]),
    "sct_finalize_partials": (_int, [_i32, _vp, _i64, _vp, _vp, _vp]),
    "sct_profile_enable": (_int, [_int]),
    "sct_profile_only": (_int, [ctypes.c_char_p]),
    "sct_profile_read": (_int, [_P(ctypes.c_char_p), _P(ctypes.c_double), _P(_i64), _int]),
    "sct_profile_read_items": (_int, [_P(ctypes.c_char_p), _P(ctypes.c_double), _P(_i64), _P(_i64), _int]),
    "sct_tag_sort_workspace_size": (_int, [_plan, _P(_sz)]),
    "sct_tag_sort": (_int, [_plan, _rec, _vp, _i32, _i32, _rec, _vp, _sz, _vp]),
    "sct_verify_sort": (_int, [_plan, _rec, _vp, _i32, _vp, _sz, _P(_i64), _vp]),
    "sct_count_matrix_workspace_size": (_int, [_P(CountInput), _P(_sz)]),
    "sct_count_matrix": (_int, [_P(CountInput), _P(CountOutput), _vp, _sz, _vp]),
    "sct_allreduce_gene_partials": (_int, [_vp, _i64, _vp, _vp]),
    "sct_comm_unique_id": (_int, [_vp, _sz]),
    "sct_comm_init_rank": (_int, [_P(_vp), _int, _vp, _sz, _int, _int]),
    "sct_comm_init_all": (_int, [_P(_vp), _int, _P(_int)]),
    "sct_comm_destroy": (_int, [_vp]),
    "sct_comm_abort": (_int, [_vp]),
    "sct_bin_workspace_size": (_int, [_plan, _i32, _P(_sz)]),
    "sct_bin_records": (_int, [_plan, _rec, _vp, _vp, _i32, _rec, _vp, _vp, _vp, _sz, _vp]),
    "sct_exchange_counts": (_int, [_vp, _vp, _i32, _vp, _vp]),
    "sct_exchange_records": (_int, [_rec, _vp, _P(_i64), _P(_i64), _i32, _rec, _vp, _vp, _vp]),
    "sct_tagsort_metrics_workspace_size": (_int, [_plan, _P(_sz)]),
    "sct_tagsort_metrics": (_int, [_plan, _rec, _vp, _vp, _vp, _sz, _vp, _vp, _P(_i64), _vp]),
}
EXPORTED = tuple(PROTOTYPES)


def _verify_abi(lib) -> None:
    if lib.sct_abi_version() != SCT_ABI_VERSION:
        raise ImportError("libsctools_gpu.so ABI %d != %d" % (lib.sct_abi_version(), SCT_ABI_VERSION))


# RTLD_GLOBAL: as before this table existed.  The optional names are those an older engine given by
# SCT_LIB_PATH for an A/B lacks.
LIBRARY = _ffi.Library("libsctools_gpu.so", "sctools_gpu", "sct_last_error", EngineError, PROTOTYPES,
                       env_override="SCT_LIB_PATH", mode=ctypes.RTLD_GLOBAL, verify=_verify_abi,
                       optional=("sct_comm_abort", "sct_bin_workspace_size", "sct_bin_records", "sct_exchange_counts",
                                 "sct_exchange_records", "sct_profile_read_items"))
LIB_PATH = LIBRARY.path  # SCT_LIB_PATH overrides it: experiments only
load = LIBRARY.load
check = LIBRARY.check
