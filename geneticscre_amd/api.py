"""Host-side mirror of the reference's join interface on top of libgcre_hip.so (ctypes).

``JoinExec`` / ``PathSet`` follow the reference classes of the same name (src/gcre.h:103-180,
src/gcre_paths.h:10-98); ``process_paths`` follows ``ProcessPaths`` (src/wrapper.cpp:177-281).  All
compute happens in the HIP library; there is no CPU path here -- if the library or a gfx950 device is
missing, construction raises.
"""
from __future__ import annotations

import ctypes
import functools
import os
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np

from . import build as _build

_LIB = None

GCRE_OK, GCRE_ERR_ASSERT, GCRE_ERR_RANGE, GCRE_ERR_DEVICE, GCRE_ERR_ARG = 0, -1, -2, -3, -4
EXPECTED_ABI = 4   # GCRE_ABI_VERSION of include/gcre_hip.h this mirror was written against


class GcreError(RuntimeError):
    pass


class gcre_result(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("scores", ctypes.POINTER(ctypes.c_double)),
                ("src", ctypes.POINTER(ctypes.c_int32)), ("trg", ctypes.POINTER(ctypes.c_int32)),
                ("cases", ctypes.POINTER(ctypes.c_int32)), ("ctrls", ctypes.POINTER(ctypes.c_int32)),
                ("n_perm", ctypes.c_int32), ("null_max", ctypes.POINTER(ctypes.c_float))]


class gcre_join_opts(ctypes.Structure):
    _fields_ = [("sharded", ctypes.c_int32), ("keep_ranged", ctypes.c_int32), ("shard_begin", ctypes.c_int64),
                ("shard_end", ctypes.c_int64), ("d_null_out", ctypes.c_void_p), ("keep_begin", ctypes.c_int64),
                ("keep_end", ctypes.c_int64), ("exchanges", ctypes.c_int32), ("exchange", ctypes.c_void_p),
                ("exchange_user", ctypes.c_void_p)]


EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32)


class gcre_profile(ctypes.Structure):
    _fields_ = [("null_kernel_ms", ctypes.c_double), ("null_kernel_launches", ctypes.c_int64),
                ("stats_kernel_ms", ctypes.c_double), ("select_ms", ctypes.c_double), ("total_ms", ctypes.c_double),
                ("paths", ctypes.c_int64), ("scores", ctypes.c_int64), ("null_alg_bytes", ctypes.c_double),
                ("null_row_loads", ctypes.c_double), ("ie_launches", ctypes.c_int64),
                ("ie_overlap_lists", ctypes.c_int64), ("ie_hinted_joins", ctypes.c_int64),
                ("ie_plane_joins", ctypes.c_int64), ("ie_lookup_tiles", ctypes.c_int64), ("prepare_ms", ctypes.c_double), ("inspect_ms", ctypes.c_double),
                ("ie_quad_launches", ctypes.c_int64), ("inspect_replays", ctypes.c_int64)]


class gcre_level(ctypes.Structure):
    _fields_ = [("uid_count", ctypes.c_void_p), ("uid_location", ctypes.c_void_p), ("n_uids", ctypes.c_int64),
                ("signs", ctypes.c_void_p), ("n_signs", ctypes.c_int64)]


class gcre_level_table(ctypes.Structure):
    _fields_ = [("path_length", ctypes.c_int32), ("n_uids", ctypes.c_int64),
                ("src", ctypes.POINTER(ctypes.c_int32)), ("trg", ctypes.POINTER(ctypes.c_int32)),
                ("count", ctypes.POINTER(ctypes.c_int32)), ("location", ctypes.POINTER(ctypes.c_int64)),
                ("n_signs", ctypes.c_int64), ("signs", ctypes.POINTER(ctypes.c_int32)), ("total_paths", ctypes.c_int64)]


class gcre_levels(ctypes.Structure):
    _fields_ = [("level", gcre_level_table * 6), ("n_data_inds", ctypes.c_int64 * 4),
                ("data_inds", ctypes.POINTER(ctypes.c_int32) * 4), ("n_rels3", ctypes.c_int64),
                ("r3_src", ctypes.POINTER(ctypes.c_int32)), ("r3_trg", ctypes.POINTER(ctypes.c_int32)),
                ("r3_sign", ctypes.POINTER(ctypes.c_int32)), ("r3_trg2", ctypes.POINTER(ctypes.c_int32)),
                ("r3_sign2", ctypes.POINTER(ctypes.c_int32))]


class gcre_pp_input(ctypes.Structure):
    _fields_ = [("level", gcre_level * 6), ("data_inds", ctypes.c_void_p * 4), ("n_data_inds", ctypes.c_int64 * 4),
                ("data1", ctypes.c_void_p), ("data1_rows", ctypes.c_int64),
                ("data2", ctypes.c_void_p), ("data2_rows", ctypes.c_int64), ("data_col_major", ctypes.c_int),
                ("value_table", ctypes.c_void_p), ("vt_rows", ctypes.c_int), ("vt_cols", ctypes.c_int),
                ("vt_col_major", ctypes.c_int),
                ("perm_cases", ctypes.c_void_p), ("perm_rows", ctypes.c_int), ("perm_col_major", ctypes.c_int),
                ("path_length", ctypes.c_int), ("shard_rank", ctypes.c_int), ("shard_world", ctypes.c_int),
                ("window_perms", ctypes.c_int)]


class gcre_dp_input(ctypes.Structure):
    _fields_ = [("method", ctypes.c_int32), ("n_cases", ctypes.c_int32), ("n_ctrls", ctypes.c_int32),
                ("n_paths", ctypes.c_int32), ("path_len", ctypes.c_void_p), ("path_rows", ctypes.c_void_p),
                ("path_sign", ctypes.c_void_p), ("rows", ctypes.c_void_p), ("n_rows", ctypes.c_int32),
                ("stratum", ctypes.c_void_p), ("n_strata", ctypes.c_int32), ("iterations", ctypes.c_int32),
                ("seed", ctypes.c_uint64), ("strata_out", ctypes.c_void_p)]


# gcre_dp_split / gcre_dp_stratum as numpy records (C layout): the library writes straight into these arrays
DP_SPLIT = np.dtype([("path", "<i4"), ("direction", "<i4"), ("j", "<i4"), ("valid", "<i4"),
                     ("cases1", "<i4"), ("ctrls1", "<i4"), ("cases2", "<i4"), ("ctrls2", "<i4"),
                     ("case_pos1", "<i4"), ("ctrl_pos1", "<i4"), ("case_neg1", "<i4"), ("ctrl_neg1", "<i4"),
                     ("case_pos2", "<i4"), ("ctrl_pos2", "<i4"), ("case_neg2", "<i4"), ("ctrl_neg2", "<i4"),
                     ("score", "<f8"), ("k_pos", "<i4"), ("pop_pos", "<i4"), ("succ_pos", "<i4"),
                     ("k_neg", "<i4"), ("pop_neg", "<i4"), ("succ_neg", "<i4"),
                     ("strata_off", "<i8"), ("n_ge", "<i8"), ("pvalue", "<f8")], align=True)
DP_STRATUM = np.dtype([("pop", "<i4"), ("cases", "<i4"), ("k_pos", "<i4"), ("k_neg", "<i4")])


class gcre_set_input(ctypes.Structure):
    _fields_ = [("n_sets", ctypes.c_int64), ("set_off", ctypes.c_void_p), ("members", ctypes.c_void_p),
                ("signs", ctypes.c_void_p), ("rows", ctypes.c_void_p), ("n_rows", ctypes.c_int64),
                ("n_cols", ctypes.c_int32)]


# gcre_set_score as a numpy record (C layout)
SET_SCORE = np.dtype([("set", "<i8"), ("valid", "<i4"), ("cases", "<i4"), ("ctrls", "<i4"), ("cases_pos", "<i4"),
                      ("ctrls_pos", "<i4"), ("cases_neg", "<i4"), ("ctrls_neg", "<i4"), ("score", "<f8"),
                      ("n_ge", "<i8"), ("pvalue", "<f8")], align=True)
# gcre_family_score
FAMILY_SCORE = np.dtype([("n_ge_stepdown", "<i8"), ("exceed", "<u8"), ("observed", "<i8")], align=True)
FAMILY_KMAX = 10   # GCRE_FAMILY_KMAX
# gcre_minp_score
MINP_SCORE = np.dtype([("n_le_minp", "<i8"), ("n_le_stepdown", "<i8")], align=True)
# gcre_prefix_score
PREFIX_SCORE = np.dtype([("score", "<f8"), ("n_ge", "<i8"), ("best_step", "<i4"), ("best_members", "<i4"), ("steps", "<i4"),
                         ("cases_pos", "<i4"), ("ctrls_pos", "<i4"), ("cases_neg", "<i4"), ("ctrls_neg", "<i4")], align=True)
# gcre_dose_score
DOSE_SCORE = np.dtype([("score", "<f8"), ("n_ge", "<i8"), ("best_index", "<i4"), ("best_level", "<i4"), ("levels", "<i4"),
                       ("cases_pos", "<i4"), ("ctrls_pos", "<i4"), ("cases_neg", "<i4"), ("ctrls_neg", "<i4"), ("pad", "<i4")],
                      align=True)
DOSE_MAX_LEVEL = 15   # GCRE_DOSE_MAX_LEVEL
# gcre_seq_score
SEQ_SCORE = np.dtype([("n_hit", "<i8"), ("n_perm", "<i8"), ("stopped", "<i4"), ("pad", "<i4")], align=True)
# gcre_strata_score
STRATA_SCORE = np.dtype([("score", "<f8"), ("n_ge", "<i8")], align=True)
STRATA_MAX = 16   # GCRE_STRATA_MAX
# gcre_burden
BURDEN = np.dtype([("total", "<i8"), ("observed", "<i8"), ("n_ge", "<i8"), ("n_le", "<i8"), ("planes", "<i4"),
                   ("p_upper", "<f8"), ("p_lower", "<f8")], align=True)


# every symbol include/gcre_hip.h declares; tests check that the library exports all of them
EXPORTS = [
    "gcre_create", "gcre_destroy", "gcre_last_error", "gcre_abi_version", "gcre_set_top_k", "gcre_width_ul",
    "gcre_vlen", "gcre_set_value_table", "gcre_set_perm_cases", "gcre_set_perm_masks", "gcre_pathset_zeros",
    "gcre_pathset_from_dense", "gcre_pathset_from_words", "gcre_pathset_select", "gcre_pathset_size",
    "gcre_pathset_read", "gcre_pathset_free", "gcre_join", "gcre_result_free", "gcre_uids_create",
    "gcre_uids_total_paths", "gcre_uids_free", "gcre_join_uids", "gcre_get_profile",
    "gcre_process_paths", "gcre_resolve_count_locs", "gcre_build_levels", "gcre_levels_free", "gcre_values_table", "gcre_values_table_exact_order",
    "gcre_generate_perm_masks", "gcre_mix64", "gcre_get_perm_mask", "gcre_uids_set_reduced",
    "gcre_set_perm_window", "gcre_plan_perm_window", "gcre_process_paths_devices",
    "gcre_set_inspect_cache", "gcre_drop_inspections", "gcre_build_flags", "gcre_device_count",
    "gcre_rccl_selftest", "gcre_rccl_collectives", "gcre_join_ahead",
    "gcre_decorated_splits", "gcre_decorated_pvalues", "gcre_score_sets",
    "gcre_score_sets_given", "gcre_given_launches",
    "gcre_score_sets_family", "gcre_family_launches",
    "gcre_score_sets_minp", "gcre_minp_launches",
    "gcre_score_sets_compete", "gcre_compete_launches",
    "gcre_score_sets_prefix", "gcre_prefix_launches",
    "gcre_score_sets_subsample", "gcre_subsample_launches",
    "gcre_score_sets_dose", "gcre_dose_launches",
    "gcre_score_sets_sequential", "gcre_sequential_launches",
    "gcre_score_sets_strata", "gcre_strata_launches",
    "gcre_generate_weighted_masks", "gcre_weighted_thresholds", "gcre_weighted_launches",
    "gcre_score_sets_sequential_weighted",
    "gcre_score_sets_prefix_sequential", "gcre_score_sets_dose_sequential", "gcre_seq_prefix_launches",
    "gcre_set_overlap", "gcre_overlap_launches",
    "gcre_clump_sets", "gcre_clump_launches",
    "gcre_set_patient_counts", "gcre_patient_launches",
    "gcre_patient_burden", "gcre_burden_launches",
    "gcre_gene_tally_create", "gcre_join_set_tally", "gcre_process_paths_set_tally", "gcre_gene_tally_read",
    "gcre_gene_tally_free",
    "gcre_exceed_create", "gcre_join_set_exceed", "gcre_process_paths_set_exceed", "gcre_exceed_read",
    "gcre_exceed_reset", "gcre_exceed_free",
    "gcre_exceed_keep_perm_counts", "gcre_exceed_read_perm_counts",
    "gcre_exceed_stepdown", "gcre_stepdown_launches",
    "gcre_hits_create", "gcre_join_set_hits", "gcre_process_paths_set_hits", "gcre_hits_count", "gcre_hits_read",
    "gcre_hits_reset", "gcre_hits_free", "gcre_hits_launches",
    "gcre_test_range_union", "gcre_test_expand", "gcre_test_inspect",
]


def lib_path() -> str:
    return _build.LIB


def load_library():
    """dlopen libgcre_hip.so (building it first if the tree is newer).  Fails loudly when it cannot."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # GCRE_LIB: a variant library built by tools/build_variant.py for an A/B measurement (never set by the product)
    path = os.environ.get("GCRE_LIB") or _build.build()
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:   # no silent fallback: the product IS this library
        raise GcreError(f"cannot load {path}: {e}") from e
    if os.environ.get("GCRE_LIB"):
        # a variant library skips build()'s staleness check: make up for it here, before any other symbol is touched
        abi = lib.gcre_abi_version() if hasattr(lib, "gcre_abi_version") else "?"
        if abi != EXPECTED_ABI:
            raise GcreError(f"GCRE_LIB={path}: ABI {abi}, this tree expects {EXPECTED_ABI} (rebuild the variant: tools/build_variant.py)")
    V, I, I64, P = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    lib.gcre_create.restype = V
    lib.gcre_create.argtypes = [I, I, I, I, I]
    lib.gcre_destroy.argtypes = [V]
    lib.gcre_destroy.restype = None
    lib.gcre_last_error.restype = ctypes.c_char_p
    lib.gcre_last_error.argtypes = [V]
    lib.gcre_abi_version.restype = I
    lib.gcre_build_flags.restype = ctypes.c_char_p
    if os.environ.get("GCRE_LIB"):
        # ... and for build()'s diagnostics check
        flags = lib.gcre_build_flags().decode()
        diag = [f for f in flags.split() if f.startswith("-D") and (f[2:].split("=")[0] in _build.DIAG_DEFINES or "ZHACK" in f or
                                                                      (f[2:].startswith("GCRE_") and "_NO" in f[2:]))]
        if diag and os.environ.get("GCRE_ALLOW_DIAG_BUILD") != "1":
            raise GcreError(f"GCRE_LIB={path} is a diagnostics build ({' '.join(diag)}): its results are wrong by design; "
                            "set GCRE_ALLOW_DIAG_BUILD=1 for a timing experiment")
        import sys
        print(f"[gcre] GCRE_LIB: using variant library {path} (build flags: {flags or 'none'})", file=sys.stderr)
    lib.gcre_set_top_k.argtypes = [V, I]
    lib.gcre_width_ul.argtypes = [V]
    lib.gcre_vlen.argtypes = [V]
    lib.gcre_set_value_table.argtypes = [V, P, I, I, I]
    lib.gcre_set_perm_cases.argtypes = [V, P, I, I, I]
    lib.gcre_set_perm_masks.argtypes = [V, P, I]
    lib.gcre_pathset_zeros.restype = V
    lib.gcre_pathset_zeros.argtypes = [V, I64]
    lib.gcre_pathset_from_dense.restype = V
    lib.gcre_pathset_from_dense.argtypes = [V, P, I64, I, I]
    lib.gcre_pathset_from_words.restype = V
    lib.gcre_pathset_from_words.argtypes = [V, P, I64]
    lib.gcre_pathset_select.restype = V
    lib.gcre_pathset_select.argtypes = [V, V, P, I64]
    lib.gcre_pathset_size.restype = I64
    lib.gcre_pathset_size.argtypes = [V]
    lib.gcre_pathset_read.argtypes = [V, V, P]
    lib.gcre_pathset_free.argtypes = [V]
    lib.gcre_pathset_free.restype = None
    lib.gcre_join.argtypes = [V, I, P, P, I64, P, I64, V, V, V, ctypes.POINTER(gcre_join_opts),
                              ctypes.POINTER(gcre_result)]
    lib.gcre_result_free.argtypes = [ctypes.POINTER(gcre_result)]
    lib.gcre_result_free.restype = None
    lib.gcre_uids_create.restype = V
    lib.gcre_uids_create.argtypes = [V, I, P, P, I64, P, I64]
    lib.gcre_uids_total_paths.restype = I64
    lib.gcre_uids_total_paths.argtypes = [V]
    lib.gcre_uids_free.argtypes = [V]
    lib.gcre_uids_free.restype = None
    lib.gcre_join_uids.argtypes = [V, V, V, V, V, ctypes.POINTER(gcre_join_opts), ctypes.POINTER(gcre_result)]
    lib.gcre_join_ahead.argtypes = [V, V, V, V, V, ctypes.POINTER(gcre_join_opts)]
    lib.gcre_get_profile.argtypes = [V, ctypes.POINTER(gcre_profile)]
    lib.gcre_process_paths.argtypes = [V, ctypes.POINTER(gcre_pp_input), ctypes.POINTER(gcre_result)]
    lib.gcre_resolve_count_locs.argtypes = [P, I64, P, P, P, I64, P, P]
    lib.gcre_build_levels.argtypes = [ctypes.c_int32, P, P, P, I64, ctypes.POINTER(gcre_levels)]
    lib.gcre_levels_free.argtypes = [ctypes.POINTER(gcre_levels)]
    lib.gcre_levels_free.restype = None
    lib.gcre_values_table.argtypes = [I, I, P]
    lib.gcre_values_table_exact_order.argtypes = [I, I]
    lib.gcre_rccl_selftest.argtypes = [I, ctypes.c_char_p, ctypes.c_size_t]
    lib.gcre_rccl_collectives.restype = ctypes.c_int64
    lib.gcre_generate_perm_masks.argtypes = [V, ctypes.c_uint64, P, I]
    lib.gcre_mix64.restype = ctypes.c_uint64
    lib.gcre_mix64.argtypes = [ctypes.c_uint64]
    lib.gcre_get_perm_mask.argtypes = [V, I, P]
    if hasattr(lib, "gcre_test_expand"):   # (a GCRE_LIB variant built from an older commit has neither)
        lib.gcre_test_range_union.argtypes = [V, P, I64, P, I64, P, P, P, I64, I, I, I, P, P, P]
        lib.gcre_test_expand.argtypes = [V, P, P, I64, P, I64, I, I, I64, I64, P, P]
    if hasattr(lib, "gcre_test_inspect"):
        lib.gcre_test_inspect.argtypes = [V, V, V, P, P, I64, P, I64, P, P, I64, I64, P, P, P, P, P, P, P, I64, P, P]
    lib.gcre_uids_set_reduced.argtypes = [V, V, P, I64]
    lib.gcre_set_perm_window.argtypes = [V, I, I]
    lib.gcre_plan_perm_window.argtypes = [V, P, I]
    lib.gcre_set_inspect_cache.argtypes = [V, I]
    lib.gcre_drop_inspections.argtypes = [V, I]
    _LIB = lib
    return lib


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


# The entry points that came after the first release: bound on first use, so that a GCRE_LIB variant built before one of
# them existed still loads for everything else.  Per feature: the feature it builds on, the symbols that must exist, what
# the library lacks without them, and (restype, argtypes) of every symbol it binds.
_V = _P = ctypes.c_void_p
_I, _I32, _I64 = ctypes.c_int, ctypes.c_int32, ctypes.c_int64
_FEATURES = {
    "decorated": (None, ["gcre_decorated_pvalues"], "decorated p-values (gcre_decorated_splits)", {
        "gcre_decorated_splits": (_I, [ctypes.POINTER(gcre_dp_input), _P, _I, _I, _I, _P, _I64, ctypes.POINTER(_I64)]),
        "gcre_decorated_pvalues": (_I, [_P, ctypes.POINTER(gcre_dp_input), _P, _I64, ctypes.POINTER(_I64), _P])}),
    "sets": (None, ["gcre_score_sets"], "set scoring (gcre_score_sets)", {
        "gcre_score_sets": (_I, [_V, ctypes.POINTER(gcre_set_input), _P, _I64, ctypes.POINTER(_I64), _P])}),
    "given": ("sets", ["gcre_score_sets_given", "gcre_given_launches"], "conditional set scores (gcre_score_sets_given)", {
        "gcre_score_sets_given": (_I, [_V, ctypes.POINTER(gcre_set_input), _P, _P, _I64, _P, _I64, ctypes.POINTER(_I64), _P]),
        "gcre_given_launches": (_I64, [_V])}),
    "family": ("sets", ["gcre_score_sets_family", "gcre_family_launches"], "family-wise set inference (gcre_score_sets_family)", {
        "gcre_score_sets_family": (_I, [_V, ctypes.POINTER(gcre_set_input), _P, _I64, ctypes.POINTER(_I64), _P, _P, _P]),
        "gcre_family_launches": (_I64, [_V])}),
    "minp": ("sets", ["gcre_score_sets_minp", "gcre_minp_launches"], "min-P set inference (gcre_score_sets_minp)", {
        "gcre_score_sets_minp": (_I, [_V, ctypes.POINTER(gcre_set_input), _P, _I64, ctypes.POINTER(_I64), _P, _P, _P]),
        "gcre_minp_launches": (_I64, [_V])}),
    "compete": ("sets", ["gcre_score_sets_compete", "gcre_compete_launches"], "competitive set tests (gcre_score_sets_compete)", {
        "gcre_score_sets_compete": (_I, [_V, ctypes.POINTER(gcre_set_input), _P, _I32, _I64, ctypes.c_uint64, _P, _I64,
                                         ctypes.POINTER(_I64), _P, _P, _P]),
        "gcre_compete_launches": (_I64, [_V])}),
    "prefix": ("sets", ["gcre_score_sets_prefix", "gcre_prefix_launches"], "variable-threshold set tests (gcre_score_sets_prefix)", {
        "gcre_score_sets_prefix": (_I, [_V, ctypes.POINTER(gcre_set_input), _P, _P, _I64, ctypes.POINTER(_I64), _P, _P, _P, _P]),
        "gcre_prefix_launches": (_I64, [_V])}),
    "subsample": ("sets", ["gcre_score_sets_subsample", "gcre_subsample_launches"], "split-half stability counts (gcre_score_sets_subsample)", {
        "gcre_score_sets_subsample": (_I, [_V, ctypes.POINTER(gcre_set_input), _I32, _I32, _I64, ctypes.c_uint64, _P, _I, _I, _P, _I, _I,
                                           _P, _I32, _P, _I64, ctypes.POINTER(_I64), _P, _P, _P, _P, _P]),
        "gcre_subsample_launches": (_I64, [_V])}),
    "dose": ("sets", ["gcre_score_sets_dose", "gcre_dose_launches"], "multi-hit set tests (gcre_score_sets_dose)", {
        "gcre_score_sets_dose": (_I, [_V, ctypes.POINTER(gcre_set_input), _P, _I32, _P, _I64, ctypes.POINTER(_I64), _P, _P, _P, _P]),
        "gcre_dose_launches": (_I64, [_V])}),
    "sequential": ("sets", ["gcre_score_sets_sequential", "gcre_sequential_launches"], "sequential permutation p-values (gcre_score_sets_sequential)", {
        "gcre_score_sets_sequential": (_I, [_V, ctypes.POINTER(gcre_set_input), ctypes.c_uint64, _P, _I, _I64, _I64, _P, _I64,
                                            ctypes.POINTER(_I64), _P]),
        "gcre_sequential_launches": (_I64, [_V])}),
    "strata": ("sets", ["gcre_score_sets_strata", "gcre_strata_launches"], "stratified set scores (gcre_score_sets_strata)", {
        "gcre_score_sets_strata": (_I, [_V, ctypes.POINTER(gcre_set_input), _P, _I32, _P, _P, _P, _P, _P, _I64, ctypes.POINTER(_I64),
                                        _P, _P, _P, _P, _P]),
        "gcre_strata_launches": (_I64, [_V])}),
    "weighted": (None, ["gcre_generate_weighted_masks", "gcre_weighted_thresholds", "gcre_weighted_launches"],
                 "covariate-adjusted permutation masks (gcre_generate_weighted_masks)", {
        "gcre_generate_weighted_masks": (_I, [_V, ctypes.c_uint64, _P, _P, _I32, _I64, _P]),
        "gcre_weighted_thresholds": (_I, [_I32, _I32, _P, _P, _I32, _P, _P]),
        "gcre_weighted_launches": (_I64, [_V])}),
    "sequential_weighted": ("sequential", ["gcre_score_sets_sequential_weighted"],
                            "weighted sequential p-values (gcre_score_sets_sequential_weighted)", {
        "gcre_score_sets_sequential_weighted": (_I, [_V, ctypes.POINTER(gcre_set_input), ctypes.c_uint64, _P, _P, _I, _I64, _I64, _I64,
                                                     _P, _I64, ctypes.POINTER(_I64), _P])}),
    "seq_prefix": ("sequential", ["gcre_score_sets_prefix_sequential", "gcre_score_sets_dose_sequential", "gcre_seq_prefix_launches"],
                   "sequential p-values of the adaptive set tests (gcre_score_sets_prefix_sequential)", {
        "gcre_score_sets_prefix_sequential": (_I, [_V, ctypes.POINTER(gcre_set_input), _P, ctypes.c_uint64, _P, _P, _I, _I64, _I64, _I64,
                                                   _P, _I64, ctypes.POINTER(_I64), _P, _P, _P]),
        "gcre_score_sets_dose_sequential": (_I, [_V, ctypes.POINTER(gcre_set_input), _P, _I32, ctypes.c_uint64, _P, _P, _I, _I64, _I64,
                                                 _I64, _P, _I64, ctypes.POINTER(_I64), _P, _P, _P]),
        "gcre_seq_prefix_launches": (_I64, [_V])}),
    "overlap": (None, ["gcre_set_overlap"], "carrier overlaps (gcre_set_overlap)", {
        "gcre_set_overlap": (_I, [_V, ctypes.POINTER(gcre_set_input), _P, _I64, _P, _I64, _P, _P]),
        "gcre_overlap_launches": (_I64, [_V])}),
    "clump": ("overlap", ["gcre_clump_sets", "gcre_clump_launches"], "device-side clumping (gcre_clump_sets)", {
        "gcre_clump_sets": (_I, [_V, ctypes.POINTER(gcre_set_input), _P, _I64, ctypes.c_double, _I, _I, _P, _P, _P, _P, _P]),
        "gcre_clump_launches": (_I64, [_V])}),
    "patients": (None, ["gcre_set_patient_counts", "gcre_patient_launches"], "carrier tallies per patient (gcre_set_patient_counts)", {
        "gcre_set_patient_counts": (_I, [_V, ctypes.POINTER(gcre_set_input), _P, _I64, _P, _I32, _I, _P, _P, ctypes.POINTER(_I64)]),
        "gcre_patient_launches": (_I64, [_V])}),
    "burden": (None, ["gcre_patient_burden", "gcre_burden_launches"], "burden tests of per-patient weights (gcre_patient_burden)", {
        "gcre_patient_burden": (_I, [_V, _P, _I64, _I32, _P, _P]),
        "gcre_burden_launches": (_I64, [_V])}),
    "genes": (None, ["gcre_gene_tally_create"], "per-gene best-path tally (gcre_gene_tally_create)", {
        "gcre_gene_tally_create": (_V, [_V, _I32, _P, _I64, _I32, _P, _I64, _I32]),
        "gcre_join_set_tally": (_I, [_V, _V]),
        "gcre_process_paths_set_tally": (_I, [_V, _I, _V]),
        "gcre_gene_tally_read": (_I, [_V, _P, _P, _P, _P, _P, _P]),
        "gcre_gene_tally_free": (None, [_V])}),
    "exceed": (None, ["gcre_exceed_create"], "null exceedance counts (gcre_exceed_create)", {
        "gcre_exceed_create": (_V, [_V, _P, _I32]),
        "gcre_join_set_exceed": (_I, [_V, _V]),
        "gcre_process_paths_set_exceed": (_I, [_V, _I, _V]),
        "gcre_exceed_read": (_I, [_V, _P, _P, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
        "gcre_exceed_reset": (_I, [_V]),
        "gcre_exceed_free": (None, [_V])}),
    "perm_counts": ("exceed", ["gcre_exceed_keep_perm_counts", "gcre_exceed_read_perm_counts"],
                    "per-permutation exceedance counts (gcre_exceed_keep_perm_counts)", {
        "gcre_exceed_keep_perm_counts": (_I, [_V, _I]),
        "gcre_exceed_read_perm_counts": (_I, [_V, _P])}),
    "stepdown": ("perm_counts", ["gcre_exceed_stepdown", "gcre_stepdown_launches"],
                 "step-down counts (gcre_exceed_stepdown)", {
        "gcre_exceed_stepdown": (_I, [_V, ctypes.POINTER(gcre_set_input), _P]),
        "gcre_stepdown_launches": (_I64, [_V])}),
    "hits": (None, ["gcre_hits_create"], "hit lists (gcre_hits_create)", {
        "gcre_hits_create": (_V, [_V, ctypes.c_double, _I64]),
        "gcre_join_set_hits": (_I, [_V, _V]),
        "gcre_process_paths_set_hits": (_I, [_V, _I, _V]),
        "gcre_hits_count": (_I, [_V, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
        "gcre_hits_read": (_I, [_V, _I64, _P, _P, _P, _P, _P, _P]),
        "gcre_hits_reset": (_I, [_V]),
        "gcre_hits_free": (None, [_V]),
        "gcre_hits_launches": (_I64, [_V])}),
}
del _V, _P, _I, _I32, _I64


def _feature_lib(feature: str):
    """The library with the entries of ``feature`` (and of what it builds on) bound."""
    parent, needs, what, binds = _FEATURES[feature]
    lib = _feature_lib(parent) if parent else load_library()
    if not all(hasattr(lib, sym) for sym in needs):
        raise GcreError(f"{lib._name} has no {what}: rebuild it")
    for sym, (restype, argtypes) in binds.items():
        fn = getattr(lib, sym)
        if fn.argtypes is None:
            fn.restype, fn.argtypes = restype, argtypes
    return lib


_decorated_lib = functools.partial(_feature_lib, "decorated")
_sets_lib = functools.partial(_feature_lib, "sets")
_given_lib = functools.partial(_feature_lib, "given")
_family_lib = functools.partial(_feature_lib, "family")
_minp_lib = functools.partial(_feature_lib, "minp")
_compete_lib = functools.partial(_feature_lib, "compete")
_prefix_lib = functools.partial(_feature_lib, "prefix")
_subsample_lib = functools.partial(_feature_lib, "subsample")
_dose_lib = functools.partial(_feature_lib, "dose")
_sequential_lib = functools.partial(_feature_lib, "sequential")
_strata_lib = functools.partial(_feature_lib, "strata")
_weighted_lib = functools.partial(_feature_lib, "weighted")
_overlap_lib = functools.partial(_feature_lib, "overlap")
_clump_lib = functools.partial(_feature_lib, "clump")
_patients_lib = functools.partial(_feature_lib, "patients")
_burden_lib = functools.partial(_feature_lib, "burden")
_genes_lib = functools.partial(_feature_lib, "genes")
_exceed_lib = functools.partial(_feature_lib, "exceed")
_perm_counts_lib = functools.partial(_feature_lib, "perm_counts")
_stepdown_lib = functools.partial(_feature_lib, "stepdown")
_hits_lib = functools.partial(_feature_lib, "hits")


OVERLAP_TILE = 64   # kOverlapTile: pairs per edge of a k_set_overlap block's tile
GENE_WIDTH_MAX = 3   # kGeneWidthMax: gene slots a joined path inherits from one operand row, at most
LEVEL_INDEX = {"1a": 0, "1b": 1, "2": 2, "3": 3, "4": 4, "5": 5}   # gcre_pp_input.level


def check_gene_tables(n_slots: int, genes0, genes1, n_uids: Optional[int] = None, max_loc: Optional[int] = None):
    """The checks gcre_gene_tally_create and the armed join make, on the host, before the library is called: each table
    None (that operand contributes no gene) or int32 [rows][1..3] with values -1..n_slots-1; with ``n_uids`` / ``max_loc``
    (the join's uid rows and the largest paths1 row it reads) also the row counts.  Returns the two tables as contiguous
    int32 arrays (or None); raises GcreError."""
    if int(n_slots) < 1:
        raise GcreError("gene tally: n_slots must be >= 1")
    out = []
    for name, g in (("genes0", genes0), ("genes1", genes1)):
        if g is None:
            out.append(None)
            continue
        a = np.asarray(g)
        if a.ndim != 2 or not 1 <= a.shape[1] <= GENE_WIDTH_MAX:
            raise GcreError(f"gene tally: {name} must be [rows][1..{GENE_WIDTH_MAX}], got shape {a.shape}")
        if not np.issubdtype(a.dtype, np.integer):
            raise GcreError(f"gene tally: {name} must hold integer slots")
        if a.size and (a.min() < -1 or a.max() >= int(n_slots)):
            bad = a[(a < -1) | (a >= int(n_slots))].ravel()[0]
            raise GcreError(f"gene tally: {name} holds slot {int(bad)} outside -1..{int(n_slots) - 1}")
        out.append(np.ascontiguousarray(a, dtype=np.int32))
    if n_uids is not None and out[0] is not None and out[0].shape[0] != int(n_uids):
        raise GcreError(f"gene tally: genes0 has {out[0].shape[0]} rows, the join index has {int(n_uids)} uid rows")
    if max_loc is not None and out[1] is not None and out[1].shape[0] <= int(max_loc):
        raise GcreError(f"gene tally: genes1 has {out[1].shape[0]} rows, the join reads paths1 row {int(max_loc)}")
    return out[0], out[1]


@dataclass
class GeneBest:
    """One entry per gene slot (gcre_gene_tally_read): -inf / -1 / 0 where no scored path touches the slot."""

    score: np.ndarray      # float64
    ordinal: np.ndarray    # int64 joined-path ordinal
    src: np.ndarray        # int32 row of paths0 (Score.src)
    trg: np.ndarray        # int32 row of paths1 (Score.trg)
    cases: np.ndarray
    ctrls: np.ndarray


class _Observer:
    """What GeneTally, ExceedCounts and HitList share: an object of the library that lives on a context (``_owner``), is
    armed for one join or for one level of process_paths, and is freed once -- by ``free()``, or by its context's close()."""

    _FREE = _JOIN_SET = _LEVEL_SET = ""   # gcre_*_free, gcre_join_set_*, gcre_process_paths_set_*
    _SET_LIB = ""                         # the module-level accessor of the library with the two setters bound
    _REFUSAL = ""                         # "<what> does not", in front of " belong to this context"

    def _check_armable(self, ex: "JoinExec", uids) -> None:
        """Raises unless the object can be armed on ``ex``.  ``uids``: the join's index where the host holds it (None: it is
        resident, and the library checks what depends on it before any launch)."""
        if self._owner is not ex or not self._h:
            raise GcreError(self._REFUSAL + " belong to this context")

    def _set(self, level: Optional[int], h) -> int:
        """Arm (``h`` = the handle) or disarm (None) for the owner's next join, or for ``level`` of its next process_paths."""
        lib = globals()[self._SET_LIB]()       # (looked up per call: the accessors can be replaced)
        if level is None:
            return getattr(lib, self._JOIN_SET)(self._owner._h, h)
        return getattr(lib, self._LEVEL_SET)(self._owner._h, level, h)

    def free(self) -> None:
        h, self._h = self._h, None
        if h and self._owner._h:       # (a closed context has freed it already)
            getattr(self._lib, self._FREE)(h)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _arm_observers(ex: "JoinExec", observers) -> None:
    """Arm ``observers`` -- [(observer, level index of process_paths or None for a single join, the join's host-side uids or
    None)], tallies first, then exceedance counts, then hit lists -- for the next call on ``ex``.  Every one is checked before
    any is armed, and a refusal by the library disarms what was armed before it: a refused call leaves nothing armed for
    the next one to consume."""
    for o, _, uids in observers:
        o._check_armable(ex, uids)
    for i, (o, level, _) in enumerate(observers):
        rc = o._set(level, o._h)
        if rc != GCRE_OK:
            for armed, at, _ in observers[:i]:
                armed._set(at, None)
            ex._check(rc)


class GeneTally(_Observer):
    """gcre_gene_tally: the per-gene best-path table of a join.  ``genes0`` / ``genes1``: the slots a
    joined path inherits from its paths0 row / its paths1 row (``report.gene_tables`` builds them per level).  Pass it as
    ``JoinExec.join(..., tally=t)`` or ``process_paths(..., tallies={"4": t})``, then ``read()``."""

    _FREE, _JOIN_SET, _LEVEL_SET = "gcre_gene_tally_free", "gcre_join_set_tally", "gcre_process_paths_set_tally"
    _SET_LIB, _REFUSAL = "_genes_lib", "gene tally does not"

    def __init__(self, owner: "JoinExec", n_slots: int, genes0, genes1):
        self.genes0, self.genes1 = check_gene_tables(n_slots, genes0, genes1)
        self.n_slots = int(n_slots)
        self._owner, self._lib, self._h = owner, _genes_lib(), None
        g0, g1 = self.genes0, self.genes1
        self._h = self._lib.gcre_gene_tally_create(owner._h, self.n_slots,
                                                   _ptr(g0), 0 if g0 is None else g0.shape[0], 0 if g0 is None else g0.shape[1],
                                                   _ptr(g1), 0 if g1 is None else g1.shape[0], 0 if g1 is None else g1.shape[1])
        if not self._h:
            owner._raise(GCRE_ERR_ARG)

    def read(self) -> GeneBest:
        n = self.n_slots
        score, ordinal = np.zeros(n, np.float64), np.zeros(n, np.int64)
        src, trg, cases, ctrls = (np.zeros(n, np.int32) for _ in range(4))
        self._owner._check(self._lib.gcre_gene_tally_read(self._h, _ptr(score), _ptr(ordinal), _ptr(src), _ptr(trg),
                                                          _ptr(cases), _ptr(ctrls)))
        return GeneBest(score, ordinal, src, trg, cases, ctrls)

    def _check_armable(self, ex, uids) -> None:
        super()._check_armable(ex, uids)
        if uids is not None:
            cnt = np.asarray(uids.count)
            ends = (np.asarray(uids.location, dtype=np.int64) + cnt)[cnt > 0]
            check_gene_tables(self.n_slots, self.genes0, self.genes1, len(cnt), int(ends.max()) - 1 if len(ends) else -1)


EXCEED_MAX = 10000   # kExceedMax: thresholds of one ExceedCounts (the top_k limit)
EXCEED_PERM_CELLS = 1 << 26   # thresholds x iterations of an ExceedCounts that keeps per-permutation counts (256 MB of u32 cells)


@dataclass
class Exceedances:
    """gcre_exceed_read, in the order of the thresholds given."""

    exceed: np.ndarray     # uint64: (joined path, permutation) pairs with a null score >= the threshold
    observed: np.ndarray   # uint64: joined paths with an observed score >= the threshold
    perms: int             # permutations counted (the window lengths of the joins counted, added)
    paths: int             # joined paths whose observed scores were counted
    # uint64 [m][iterations]: joined paths with a null score >= the threshold, per permutation (absolute index); every row
    # sums to ``exceed``.  None when the object keeps none (``ExceedCounts(perm_counts=False)``)
    perm_counts: Optional[np.ndarray] = None


class ExceedCounts(_Observer):
    """gcre_exceed: null exceedance counts of a join for a list of thresholds.  Pass it as
    ``JoinExec.join(..., exceed=x)`` or ``process_paths(..., exceeds={"4": x})``, then ``read()``.  Counts ADD: a join counted
    twice is counted twice (``reset()`` starts over); ``report.fdr_columns`` turns them into PFER, FDR and q-values.

    ``perm_counts=True`` also keeps the counts per permutation (gcre_exceed_keep_perm_counts, DESIGN.md §3.8a: thresholds x
    iterations <= ``EXCEED_PERM_CELLS``), read as ``Exceedances.perm_counts``; ``report.false_count_columns`` turns them into
    k-FWER, the median and the (1 - alpha) bound of the number of false positives.  False, the default: nothing new is called."""

    _FREE, _JOIN_SET, _LEVEL_SET = "gcre_exceed_free", "gcre_join_set_exceed", "gcre_process_paths_set_exceed"
    _SET_LIB, _REFUSAL = "_exceed_lib", "exceedance counts do not"

    def __init__(self, owner: "JoinExec", thresholds, perm_counts: bool = False):
        t = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).ravel())
        self.thresholds = t
        self.keeps_perm_counts = bool(perm_counts)
        self._owner, self._lib, self._h = owner, (_perm_counts_lib() if perm_counts else _exceed_lib()), None
        self._h = self._lib.gcre_exceed_create(owner._h, _ptr(t), len(t))
        if not self._h:
            owner._raise(GCRE_ERR_ARG)
        if perm_counts:
            rc = self._lib.gcre_exceed_keep_perm_counts(self._h, 1)
            if rc != 0:
                self.free()
                owner._raise(rc)

    def read(self) -> Exceedances:
        m = len(self.thresholds)
        exceed, observed = np.zeros(m, np.uint64), np.zeros(m, np.uint64)
        perms, paths = ctypes.c_int64(0), ctypes.c_int64(0)
        self._owner._check(self._lib.gcre_exceed_read(self._h, _ptr(exceed), _ptr(observed), ctypes.byref(perms),
                                                      ctypes.byref(paths)))
        pc = None
        if self.keeps_perm_counts:
            pc = np.zeros((m, int(self._owner.iters)), np.uint64)
            self._owner._check(self._lib.gcre_exceed_read_perm_counts(self._h, _ptr(pc)))
        return Exceedances(exceed, observed, int(perms.value), int(paths.value), pc)

    def stepdown(self, sets, rows, signs=None) -> np.ndarray:
        """Step-down max-T counts (gcre_exceed_stepdown) of an object that keeps per-permutation counts and
        holds exactly one full pass of one join.  ``sets`` / ``rows`` / ``signs`` as ``JoinExec.score_sets`` takes them (lists
        per set, or an ``(off, members)`` pair with flat signs), one set per threshold, in the thresholds' order: set j is
        the joined path whose observed score is threshold j (the library refuses a set whose score is not its threshold,
        bit for bit).  Returns int64 [m]: n_ge[j] = the permutations whose maximum null value over the join's paths, the
        rows with a strictly larger threshold left out, reaches threshold j.  ``report.stepdown_columns`` turns them into
        ``PvaluesStepDown``.  The object is not changed."""
        lib = _stepdown_lib()
        inp, keep = _set_input(sets, rows, signs, self._owner.num_cases + self._owner.num_ctrls)
        n_ge = np.zeros(len(self.thresholds), dtype=np.int64)
        rc = lib.gcre_exceed_stepdown(self._h, ctypes.byref(inp), _ptr(n_ge))
        self._owner._check_gcre(rc)        # (as score_sets: every refusal is a GcreError with the library's message)
        return n_ge

    def reset(self) -> None:
        self._owner._check(self._lib.gcre_exceed_reset(self._h))


HITS_CAP_MAX = 1 << 26   # kHitsCapMax: records of one HitList (32 B each on the device)


@dataclass
class Hits:
    """gcre_hits_count / gcre_hits_read: the joined paths at or above a HitList's cut-off, best first (score descending as
    doubles, then ordinal ascending).  The six arrays are empty when the list overflowed (``complete`` False): ``found`` is
    exact all the same."""

    found: int             # joined paths at or above the cut-off (may exceed the list's cap)
    paths: int             # joined paths looked at
    complete: bool         # found <= cap: the arrays hold every hit
    score: np.ndarray      # float64
    ordinal: np.ndarray    # int64 joined-path ordinal
    src: np.ndarray        # int32 row of paths0 (Score.src)
    trg: np.ndarray        # int32 row of paths1 (Score.trg)
    cases: np.ndarray
    ctrls: np.ndarray

    def as_join_result(self, null) -> "JoinResult":
        """The hits as ``report.results_table`` takes a level: a JoinResult (scores ascending, as a top-k list has them)
        whose ``pvalues()`` compare with ``null``, the level's null maxima."""
        r = slice(None, None, -1)
        return JoinResult(self.score[r].copy(), self.src[r].copy(), self.trg[r].copy(), self.cases[r].copy(),
                          self.ctrls[r].copy(), np.asarray(null, dtype=np.float32))


class HitList(_Observer):
    """gcre_hits: every joined path of a join whose observed score is >= ``cutoff``, up to ``cap``
    records (32 x cap bytes of device memory).  Pass it as ``JoinExec.join(..., hits=h)``, ``process_paths(..., hits={"4":
    h})`` or ``ResidentPlan.run(..., hits={"4": h})``, then ``read()``.  The list ADDS: shards of one join append into one
    list, a join collected twice is listed twice (``reset()`` starts over)."""

    _FREE, _JOIN_SET, _LEVEL_SET = "gcre_hits_free", "gcre_join_set_hits", "gcre_process_paths_set_hits"
    _SET_LIB, _REFUSAL = "_hits_lib", "hit list does not"

    def __init__(self, owner: "JoinExec", cutoff: float, cap: int = 1 << 20):
        self.cutoff, self.cap = float(cutoff), int(cap)
        self._owner, self._lib, self._h = owner, _hits_lib(), None
        if not owner._h:
            raise GcreError("hit list: the context is closed")
        if not -(1 << 63) <= self.cap < (1 << 63):
            raise GcreError(f"hit list: cap must be 1..{HITS_CAP_MAX} (2^26), not {self.cap}")
        self._h = self._lib.gcre_hits_create(owner._h, self.cutoff, self.cap)
        if not self._h:
            owner._raise(GCRE_ERR_ARG)

    def _alive(self):
        if not self._h or not self._owner._h:     # (a closed context has freed it already)
            raise GcreError("hit list does not belong to this context (freed, or its context is closed)")
        return self._h

    def count(self) -> Tuple[int, int]:
        """(found, paths): joined paths at or above the cut-off, and joined paths looked at."""
        found, paths = ctypes.c_int64(0), ctypes.c_int64(0)
        self._owner._check(self._lib.gcre_hits_count(self._alive(), ctypes.byref(found), ctypes.byref(paths)))
        return int(found.value), int(paths.value)

    def read(self) -> Hits:
        found, paths = self.count()
        n = found if found <= self.cap else 0
        score, ordinal = np.zeros(n, np.float64), np.zeros(n, np.int64)
        src, trg, cases, ctrls = (np.zeros(n, np.int32) for _ in range(4))
        if found <= self.cap:
            self._owner._check(self._lib.gcre_hits_read(self._alive(), found, _ptr(score), _ptr(ordinal), _ptr(src), _ptr(trg),
                                                        _ptr(cases), _ptr(ctrls)))
        return Hits(found, paths, found <= self.cap, score, ordinal, src, trg, cases, ctrls)

    def reset(self) -> None:
        self._owner._check(self._lib.gcre_hits_reset(self._alive()))


def _set_input(sets, rows, signs, n: int):
    """gcre_set_input of the ``sets`` / ``rows`` / ``signs`` every set entry takes (``n``: the context's patients), and the
    arrays it points into (keep them alive for the call): ``(inp, (off, members, signs, packed rows))``.  An entry that has
    index lists to check before it reads its context parses with ``_set_lists`` first and passes ``(off, members)`` and the
    flat signs on to here -- they are a set list like any other."""
    S, off, members, sg = _set_lists(sets, signs)
    packed, n_cols = _carrier_rows(rows, n)
    inp = gcre_set_input(S, _ptr(off), _ptr(members), _ptr(sg), _ptr(packed), packed.shape[0], n_cols)
    return inp, (off, members, sg, packed)


def _set_lists(sets, signs):
    """(S, off, members, signs) as the set entries take them -- int64 [S + 1] offsets into int32 members, int32 signs or None
    -- from one sequence of rows per set with one sequence of signs per set, or from an ``(off, members)`` pair (what
    ``report.hit_sets`` returns) with one flat signs array.  ValueError where the signs do not match the members."""
    def flat(lists):
        return np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in lists])
                                    if len(lists) else np.zeros(0), dtype=np.int32)

    if isinstance(sets, tuple) and len(sets) == 2 and isinstance(sets[0], np.ndarray):
        off = np.ascontiguousarray(sets[0], dtype=np.int64)
        members = np.ascontiguousarray(sets[1], dtype=np.int32)
        sg = None if signs is None else flat([signs])
        matching = sg is None or len(sg) == len(members)
    else:
        lens = [len(s) for s in sets]
        off = np.zeros(len(sets) + 1, dtype=np.int64)
        off[1:] = np.cumsum(lens)
        members = flat(sets)
        matching = signs is None or (len(signs) == len(sets) and all(len(x) == L for x, L in zip(signs, lens)))
        sg = flat(signs) if matching and signs is not None else None
    if not matching:
        raise ValueError("signs: one sign per member of every set")
    return len(off) - 1, off, members, sg


def _prefix_cuts(sets, cuts, S, off, members):
    """``cuts`` of ``prefix_tests`` as uint8 flags [members], or None for None: it follows the signs of ``_set_lists`` -- one
    sequence per set, or one flat array beside an ``(off, members)`` pair.  ValueError where it does not match the members."""
    if cuts is None:
        return None
    if isinstance(sets, tuple) and len(sets) == 2 and isinstance(sets[0], np.ndarray):
        ct = np.asarray(cuts).reshape(-1)
        matching = len(ct) == len(members)
    else:
        matching = len(cuts) == S and all(len(x) == L for x, L in zip(cuts, np.diff(off)))
        ct = np.concatenate([np.asarray(x).reshape(-1) for x in cuts]) if matching and S else np.zeros(0)
    if not matching:
        raise ValueError("cuts: one flag per member of every set")
    return np.ascontiguousarray(ct != 0, dtype=np.uint8)


def _dose_levels(levels) -> np.ndarray:
    """``levels`` of ``dose_tests`` as int32: 1 to 15 strictly ascending integers in 1 .. 15, or ValueError."""
    a = np.asarray(levels)
    if a.ndim != 1 or not 1 <= a.size <= DOSE_MAX_LEVEL:
        raise ValueError(f"levels: 1 to {DOSE_MAX_LEVEL} levels, one list")
    lv = a.astype(np.int64)
    if not np.array_equal(lv, a):
        raise ValueError("levels: whole numbers")
    if lv.min() < 1 or lv.max() > DOSE_MAX_LEVEL:
        raise ValueError(f"levels: every level in 1 .. {DOSE_MAX_LEVEL}")
    if (np.diff(lv) <= 0).any():
        raise ValueError("levels: strictly ascending")
    return np.ascontiguousarray(lv, dtype=np.int32)


def pack_carriers(rows, n_cols: int) -> np.ndarray:
    """A 0/1 carrier matrix [rows][n_cols] as gcre's packed rows: uint64 [rows][ceil(n_cols/64)], bit c = patient c."""
    d = np.asarray(rows).reshape(-1, n_cols) != 0
    bits = np.zeros((d.shape[0], -(-n_cols // 64) * 64), dtype=bool)
    bits[:, :n_cols] = d
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little").view("<u8"))


def _carrier_rows(rows, n: int):
    """(packed rows, columns) of the carrier matrix a set entry is given: a 2-D ``rows`` keeps its width (the library
    compares it with the context's), anything else is read as rows of ``n`` patients."""
    d = np.asarray(rows)
    if d.ndim != 2:
        d = d.reshape(-1, n)
    return pack_carriers(d, d.shape[1]), d.shape[1]


class _DpInput:
    """gcre_dp_input over numpy arrays it keeps alive.  ``paths``: one sequence of data-row indices per path (-1 = NA gene);
    ``rows``: the 0/1 carrier matrix [rows][patients]; ``signs``: per path, +1 / -1 per gene (None = all +1); ``strata``:
    one id per patient, any integers (mapped to 0..n_strata-1 in ascending order of id)."""

    def __init__(self, method, n_cases, n_ctrls, paths, rows, signs, strata, iterations, seed):
        if isinstance(method, str):
            method = 1 if method == "method1" else 2
        n = int(n_cases) + int(n_ctrls)
        P = len(paths)
        self.path_len = np.array([len(p) for p in paths], dtype=np.int32)
        if P and (self.path_len.min() < 1 or self.path_len.max() > 5):
            raise ValueError("a path has 1 to 5 genes")
        self.path_rows = np.full((max(P, 1), 5), -1, dtype=np.int32)
        self.path_sign = np.ones((max(P, 1), 5), dtype=np.int32)
        for i, p in enumerate(paths):
            self.path_rows[i, :len(p)] = p
            if signs is not None:
                self.path_sign[i, :len(p)] = signs[i]
        # always n columns, whatever shape ``rows`` has: gcre_dp_input states no width of its own
        self.rows = pack_carriers(rows, n)
        self.n_strata = 0
        self.stratum = None
        if strata is not None:
            ids, inv = np.unique(np.asarray(strata).reshape(-1), return_inverse=True)
            if len(inv) != n:
                raise ValueError("strata: one stratum id per patient")
            self.stratum = np.ascontiguousarray(inv, dtype=np.int32)
            self.n_strata = len(ids)
        self.S = int(sum(2 * (L - 1) for L in self.path_len.tolist()))
        self.st_out = np.zeros(max(self.S, 1) * max(self.n_strata, 1), dtype=DP_STRATUM) if strata is not None else None
        self.c = gcre_dp_input(int(method), int(n_cases), int(n_ctrls), P, _ptr(self.path_len), _ptr(self.path_rows),
                               _ptr(self.path_sign), _ptr(self.rows), self.rows.shape[0], _ptr(self.stratum),
                               self.n_strata, int(iterations), int(seed) & (2**64 - 1), _ptr(self.st_out))

    def out(self) -> np.ndarray:
        return np.zeros(max(self.S, 1), dtype=DP_SPLIT)

    def strata_records(self) -> Optional[np.ndarray]:
        return None if self.st_out is None else self.st_out[:self.S * self.n_strata].reshape(self.S, self.n_strata)


def decorated_splits(method, n_cases: int, n_ctrls: int, paths, rows, signs=None, table=None, strata=None,
                     iterations: int = 0, seed: int = 0):
    """Host stage of the decorated p-values (gcre_decorated_splits, no device needed): one DP_SPLIT record per split --
    counts, observed score (NaN without ``table``), urns -- and, with ``strata``, the [splits][n_strata] DP_STRATUM urns.
    p-values stay NaN: the permutations run on the device (JoinExec.decorated_pvalues)."""
    lib = _decorated_lib()
    d = _DpInput(method, n_cases, n_ctrls, paths, rows, signs, strata, iterations, seed)
    out = d.out()
    t = None if table is None else np.ascontiguousarray(table, dtype=np.float64)
    n_out = ctypes.c_int64(0)
    rc = lib.gcre_decorated_splits(ctypes.byref(d.c), _ptr(t), 0 if t is None else t.shape[0],
                                   0 if t is None else t.shape[1], 0, _ptr(out), len(out), ctypes.byref(n_out))
    if rc == GCRE_ERR_RANGE:
        raise IndexError("gcre_decorated_splits: a row index or stratum id is out of range")
    if rc != GCRE_OK:
        raise ValueError(f"gcre_decorated_splits: bad input ({rc})")
    return out[:n_out.value], d.strata_records()


@dataclass
class JoinResult:
    """joined_res (src/gcre_types.h:45-48) as arrays; what make_score_list turns into an R list (wrapper.cpp:142-174)."""

    scores: np.ndarray     # float64 ascending
    src: np.ndarray        # idx; R sees ids[,1] = src + 1
    trg: np.ndarray        # loc; R sees ids[,2] = trg + 1
    cases: np.ndarray
    ctrls: np.ndarray
    null: np.ndarray       # float32 [iterations] -- "TestScores"

    def pvalues(self) -> np.ndarray:
        """#(TestScores >= score) / length(TestScores), R/ProcessPaths.R:316 (f64 score vs f32 maxima)."""
        t = self.null.astype(np.float64)
        if len(t) == 0:
            return np.full(len(self.scores), np.nan)
        return np.array([(t >= s).sum() / len(t) for s in self.scores])

    def as_r_list(self) -> Dict[str, object]:
        """The named list make_score_list builds (wrapper.cpp:167-173)."""
        return {
            "scores": self.scores,
            "ids": np.stack([self.src + 1, self.trg + 1], axis=1) if len(self.src) else np.zeros((0, 2), np.int32),
            "TestScores": self.null.astype(np.float64),
            "cases": self.cases.astype(np.float64),
            "controls": self.ctrls.astype(np.float64),
            "debug": [f"[debug] {s}:{t} {c}/{d}" for s, t, c, d in
                      zip(self.src.tolist(), self.trg.tolist(), self.cases.tolist(), self.ctrls.tolist())],
        }


def _take_result(lib, r: gcre_result) -> JoinResult:
    n, k = r.n, r.n_perm
    out = JoinResult(
        np.ctypeslib.as_array(r.scores, (n,)).copy() if n > 0 else np.zeros(0),
        np.ctypeslib.as_array(r.src, (n,)).copy() if n > 0 else np.zeros(0, np.int32),
        np.ctypeslib.as_array(r.trg, (n,)).copy() if n > 0 else np.zeros(0, np.int32),
        np.ctypeslib.as_array(r.cases, (n,)).copy() if n > 0 else np.zeros(0, np.int32),
        np.ctypeslib.as_array(r.ctrls, (n,)).copy() if n > 0 else np.zeros(0, np.int32),
        np.ctypeslib.as_array(r.null_max, (k,)).copy() if k > 0 else np.zeros(0, np.float32),
    )
    lib.gcre_result_free(ctypes.byref(r))
    return out


class PathSet:
    """Device-resident PathSet (src/gcre_paths.h:10-98)."""

    def __init__(self, owner: "JoinExec", handle: int):
        if not handle:
            owner._raise()
        self._owner, self._h = owner, handle
        self.size = int(owner._lib.gcre_pathset_size(handle))
        self.vlen = owner.vlen

    def select(self, indices) -> "PathSet":
        idx = np.ascontiguousarray(indices, dtype=np.int32)
        return PathSet(self._owner, self._owner._lib.gcre_pathset_select(self._owner._h, self._h, _ptr(idx), len(idx)))

    def to_numpy(self) -> np.ndarray:
        out = np.zeros((self.size, self.vlen), dtype=np.uint64)
        self._owner._check(self._owner._lib.gcre_pathset_read(self._owner._h, self._h, _ptr(out)))
        return out

    def free(self) -> None:
        h, self._h = self._h, None
        if h and self._owner._h:
            self._owner._lib.gcre_pathset_free(h)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceUids:
    """UidRelSet (src/gcre.h:49-90) resident on the device."""

    def __init__(self, owner: "JoinExec", uids):
        count = np.ascontiguousarray(uids.count, dtype=np.int32)
        location = np.ascontiguousarray(uids.location, dtype=np.int64)
        signs = np.ascontiguousarray(uids.signs, dtype=np.int32)
        self._owner = owner
        self.path_length = int(uids.path_length)
        self._h = owner._lib.gcre_uids_create(owner._h, self.path_length, _ptr(count), _ptr(location), len(count),
                                              _ptr(signs), len(signs))
        if not self._h:
            owner._raise()
        self.total_paths = int(owner._lib.gcre_uids_total_paths(self._h))
        self._reduced = None

    def set_reduced(self, reduced: Optional["PathSet"], index=None) -> None:
        """gcre_uids_set_reduced: paths0[idx] | paths1[loc] == paths0[idx] | reduced[index[loc]] (checked per join)."""
        if reduced is None:
            self._owner._check(self._owner._lib.gcre_uids_set_reduced(self._h, None, None, 0))
            self._reduced = None
            return
        idx = np.ascontiguousarray(np.asarray(index).astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32)   # bit 31 = swap halves
        self._owner._check(self._owner._lib.gcre_uids_set_reduced(self._h, reduced._h, _ptr(idx), len(idx)))
        self._reduced = reduced     # keeps the operand alive

    def free(self) -> None:
        h, self._h = self._h, None
        if h and self._owner._h:
            self._owner._lib.gcre_uids_free(h)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class JoinExec:
    """JoinExec (src/gcre.h:103-180) on one MI355X.  ``method`` is "method1" | "method2" or 1 | 2."""

    def __init__(self, method, num_cases: int, num_ctrls: int, iters: int, device: int = 0):
        self._lib = load_library()
        if isinstance(method, str):
            method = 1 if method == "method1" else 2   # JoinExec::to_method, gcre.h:125-133
        self.method, self.num_cases, self.num_ctrls, self.iters = int(method), int(num_cases), int(num_ctrls), int(iters)
        self._h = self._lib.gcre_create(self.method, self.num_cases, self.num_ctrls, self.iters, int(device))
        if not self._h:
            msg = self._lib.gcre_last_error(None).decode()
            if msg.startswith("assertion"):
                raise ValueError(msg)
            raise GcreError(msg)
        self.width_ul = self._lib.gcre_width_ul(self._h)
        self.vlen = self._lib.gcre_vlen(self._h)
        self._top_k = 12
        self.nthreads = 0   # accepted for interface parity; the device schedules the work

    # -- plumbing --
    def _raise(self, rc: int = GCRE_ERR_DEVICE):
        msg = self._lib.gcre_last_error(self._h).decode()
        if rc == GCRE_ERR_RANGE or "out of range" in msg:
            raise IndexError(msg)          # std::out_of_range
        if rc == GCRE_ERR_ASSERT or msg.startswith("assertion"):
            raise ValueError(msg)          # std::logic_error
        raise GcreError(msg)

    def _check(self, rc: int):
        if rc != GCRE_OK:
            self._raise(rc)

    def _check_gcre(self, rc: int):
        """``_check`` of the set entries: every refusal is a GcreError with the library's message."""
        if rc != GCRE_OK:
            raise GcreError(self._lib.gcre_last_error(self._h).decode())

    def close(self):
        h, self._h = self._h, None
        if h:
            self._lib.gcre_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def top_k(self) -> int:
        return self._top_k

    @top_k.setter
    def top_k(self, k: int):
        self._check(self._lib.gcre_set_top_k(self._h, int(k)))
        self._top_k = int(k)

    # -- JoinExec interface --
    def set_value_table(self, table) -> None:
        t = np.ascontiguousarray(table, dtype=np.float64)
        self._check(self._lib.gcre_set_value_table(self._h, _ptr(t), t.shape[0], t.shape[1], 0))

    def set_permuted_cases(self, perms) -> None:
        p = np.ascontiguousarray(perms, dtype=np.int32)
        if p.ndim != 2:
            p = p.reshape(0, 0)
        self._check(self._lib.gcre_set_perm_cases(self._h, _ptr(p), p.shape[0], p.shape[1], 0))

    def set_permuted_masks(self, masks) -> None:
        m = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1, self.width_ul)
        self._check(self._lib.gcre_set_perm_masks(self._h, _ptr(m), m.shape[0]))

    def generate_permutations(self, seed: int, strata=None) -> None:
        """Device-side getRandIndicesMat + getCaseORControl + setPermutedCases (R/Utils.R:22-46, 246-262)."""
        if strata is None:
            self._check(self._lib.gcre_generate_perm_masks(self._h, int(seed) & (2**64 - 1), None, 0))
        else:
            st = np.ascontiguousarray(strata, dtype=np.int32)
            self._check(self._lib.gcre_generate_perm_masks(self._h, int(seed) & (2**64 - 1), _ptr(st), int(st.max()) + 1))

    def generate_weighted_permutations(self, seed: int, odds, strata=None, max_attempts: int = 1 << 20, attempts: bool = False):
        """Covariate-adjusted permutations (gcre_generate_weighted_masks; Epstein et al. 2012): the case
        labels of every permutation are redrawn with per-patient ``odds`` -- one finite value >= 0 per patient, e.g.
        ``report.case_odds(covariates, ...)`` -- conditional on the number of cases, inside every stratum when ``strata`` is
        given (one id per patient, any integers, mapped to 0 .. S-1 in ascending order; at most 16 distinct).  Equal odds
        give the uniform law of ``generate_permutations`` (not its bits).  The masks replace the context's, so every join and
        every set statistic that follows is tested against the adjusted null; the adjustment is on the null, not on the
        statistic, and the p-values are only as good as the model behind ``odds``.  ``max_attempts``: the cap of the exact
        rejection sampler per (permutation, stratum), not a tuning knob; a call that meets it is refused and the context
        keeps the masks it had.  ``attempts=True`` returns the accepted attempts, uint32 [iters][S].
        ``report.weighted_masks`` restates the draw in numpy on ``weighted_thresholds``.  Refusals raise GcreError."""
        w, st, S, _ = _weighted_args(odds, strata, self.num_cases + self.num_ctrls)
        lib = _weighted_lib()
        att = np.zeros((self.iters, S), dtype=np.uint32) if attempts else None
        self._check_gcre(lib.gcre_generate_weighted_masks(self._h, int(seed) & (2**64 - 1), _ptr(w), _ptr(st), S if st is not None else 0,
                                                          int(max_attempts), _ptr(att) if attempts and att.size else None))
        return att

    def weighted_launches(self) -> int:
        """k_weighted_search / k_weighted_write launches of ``generate_weighted_permutations`` on this context so far: two
        per successful call, one for a call that met the cap, none for one refused up front."""
        return int(_weighted_lib().gcre_weighted_launches(self._h))

    def set_perm_window(self, k0: int, k1: int) -> None:
        """Joins that follow score permutations [k0, k1) only (tile aligned); see gcre_set_perm_window."""
        self._check(self._lib.gcre_set_perm_window(self._h, int(k0), int(k1)))

    def set_inspect_cache(self, on: bool) -> None:
        """Keep every join's mask-independent (inspector) output with its join index; see gcre_set_inspect_cache."""
        self._check(self._lib.gcre_set_inspect_cache(self._h, 1 if on else 0))

    def drop_inspections(self, release_memory: bool = False) -> None:
        """Forget the cached inspector outputs (the next join on every index recomputes them)."""
        self._check(self._lib.gcre_drop_inspections(self._h, 1 if release_memory else 0))

    def plan_perm_window(self, set_rows) -> int:
        """Permutations per window so that the count planes of path sets with ``set_rows`` rows fit in device memory."""
        rows = np.ascontiguousarray(np.atleast_1d(set_rows), dtype=np.int64)
        w = self._lib.gcre_plan_perm_window(self._h, _ptr(rows), len(rows))
        if w < 0:
            self._check(w)
        return max(int(w), 1)

    def decorated_pvalues(self, paths, rows, signs=None, strata=None, seed: int = 0, return_counts: bool = False):
        """Decorated p-values (R/DecoratedPvalue.R) of ``paths`` on this context's device and value table, ``iters``
        permutations per split: a DP_SPLIT record per split (paths in order, each Forward then Backward).  ``paths`` are
        rows of ``rows`` (-1 = NA gene), ``signs`` +1 / -1 per gene (read by method 2).  With ``return_counts`` also the
        [splits][iters][2] urn successes of every permutation (cases of the pos draw, controls of the neg draw)."""
        lib = _decorated_lib()
        d = _DpInput(self.method, self.num_cases, self.num_ctrls, paths, rows, signs, strata, self.iters, seed)
        out = d.out()
        counts = np.zeros((max(d.S, 1), self.iters, 2), dtype=np.int32) if return_counts else None
        n_out = ctypes.c_int64(0)
        self._check(lib.gcre_decorated_pvalues(self._h, ctypes.byref(d.c), _ptr(out), len(out), ctypes.byref(n_out),
                                               _ptr(counts)))
        rec = out[:n_out.value]
        return (rec, counts[:n_out.value]) if return_counts else rec

    def score_sets(self, sets, rows, signs=None, family: bool = False, given=None, which=None):
        """Permutation tests of caller-given sets (gcre_score_sets): one SET_SCORE record per set, against this context's
        value table and all ``iters`` permutation masks.  ``sets``: one sequence of row indices of ``rows`` per set
        (-1 = NA gene), or a pair ``(off, members)`` -- int64 [S + 1] offsets into int32 members, what ``report.hit_sets``
        returns; ``rows``: the 0/1 carrier matrix [rows][patients]; ``signs``: per set +1 / -1 per member, with a pair one
        flat array (None = all +1; read by method 2).  With ``family`` also the per-permutation maximum of the sets' null
        scores (float32 [iters]).  Errors raise GcreError with the library's message.

        ``given`` / ``which``: conditional scores (gcre_score_sets_given), one record per ENTRY: entry i is
        set ``which[i]`` (None: every set in order; repeats allowed) scored without the carriers of set ``given[i]`` -- the
        patients with a variant in any member of that set, whatever the signs; -1 or ``given=None``: nothing set aside.
        The removed patients count as non-carriers.  An index out of range, ``given`` and ``which`` of different lengths,
        or a given set with an NA member raise ValueError before the library is touched.
        With both None nothing changes: the same call, the same records."""
        S, off, members, sg = _set_lists(sets, signs)
        iw = None if which is None else np.ascontiguousarray(np.asarray(which, dtype=np.int64).reshape(-1))
        ig = None if given is None else np.ascontiguousarray(np.asarray(given, dtype=np.int64).reshape(-1))
        E = S if iw is None else len(iw)
        if ig is not None and len(ig) != E:
            raise ValueError(f"given: {len(ig)} entries for {E} scored sets (one per entry of which, or per set)")
        if iw is not None and len(iw) and (iw.min() < 0 or iw.max() >= S):
            raise ValueError(f"which: a set index outside 0..{S - 1}")
        if ig is not None and len(ig):
            if ig.min() < -1 or ig.max() >= S:
                raise ValueError(f"given: a set index outside -1..{S - 1}")
            na = np.zeros(S, bool)
            np.logical_or.at(na, np.repeat(np.arange(S), np.diff(off)), members < 0)
            if na[ig[ig >= 0]].any():
                raise ValueError("given: a given set has an NA member (-1): its carriers are not known")
        conditional = iw is not None or ig is not None
        lib = _given_lib() if conditional else _sets_lib()
        inp, keep = _set_input((off, members), rows, sg, self.num_cases + self.num_ctrls)
        out = np.zeros(max(E, 1), dtype=SET_SCORE)
        fam = np.zeros(self.iters, dtype=np.float32) if family else None
        n_out = ctypes.c_int64(0)
        tail = (_ptr(out), len(out), ctypes.byref(n_out), _ptr(fam) if family and self.iters > 0 else None)
        if conditional:
            self._check_gcre(lib.gcre_score_sets_given(self._h, ctypes.byref(inp), _ptr(iw), _ptr(ig), E, *tail))
        else:
            self._check_gcre(lib.gcre_score_sets(self._h, ctypes.byref(inp), *tail))
        rec = out[:n_out.value]
        return (rec, fam) if family else rec

    @property
    def given_launches(self) -> int:
        """Kernels gcre_score_sets_given launched on this context so far."""
        return int(_given_lib().gcre_given_launches(self._h))

    def family_tests(self, sets, rows, signs=None, kmax: bool = False, null: bool = False):
        """Step-down, k-FWER and FDR over the family of the given sets (gcre_score_sets_family).  ``sets`` /
        ``rows`` / ``signs`` as ``score_sets`` takes them (lists per set, or an ``(off, members)`` pair with flat signs).
        Returns ``(records, family)``: the SET_SCORE records of ``score_sets``, and one FAMILY_SCORE record per set --
        ``n_ge_stepdown`` (permutations whose maximum over the sets that do not score strictly higher reaches the set's
        score), ``exceed`` (null scores of ALL sets and permutations that reach it) and ``observed`` (sets that reach
        it); a NaN score gives 0 / 0 / 0, an NA member -1 / 0 / -1.
        With ``kmax`` also float32 [FAMILY_KMAX][iters], row k the (k+1)-th largest null score of every permutation (row 0
        = ``score_sets(family=True)``'s maxima); with ``null`` also the null matrix, float32 [sets][iters] (NaN rows for
        sets with an NA member).  ``report.family_columns`` turns these into p-values.  Errors raise GcreError."""
        lib = _family_lib()
        inp, keep = _set_input(sets, rows, signs, self.num_cases + self.num_ctrls)
        S = inp.n_sets
        out = np.zeros(max(S, 1), dtype=SET_SCORE)
        fam = np.zeros(max(S, 1), dtype=FAMILY_SCORE)
        km = np.zeros((FAMILY_KMAX, self.iters), dtype=np.float32) if kmax else None
        nul = np.zeros((S, self.iters), dtype=np.float32) if null else None
        n_out = ctypes.c_int64(0)
        self._check_gcre(lib.gcre_score_sets_family(self._h, ctypes.byref(inp), _ptr(out), len(out), ctypes.byref(n_out), _ptr(fam),
                                                    _ptr(km) if kmax and km.size else None,
                                                    _ptr(nul) if null and nul.size else None))
        res = (out[:n_out.value], fam[:n_out.value])
        return res + ((km,) if kmax else ()) + ((nul,) if null else ())

    def family_launches(self) -> int:
        """k_family_null / k_family_scan / k_family_hist launches of this context so far."""
        return int(_family_lib().gcre_family_launches(self._h))

    def minp_tests(self, sets, rows, signs=None, min_count: bool = False, counts: bool = False):
        """Westfall-Young min-P over the family of the given sets (gcre_score_sets_minp).  ``sets`` / ``rows``
        / ``signs`` as ``score_sets`` takes them (lists per set, or an ``(off, members)`` pair with flat signs).  Returns
        ``(records, minp)``: the SET_SCORE records of ``score_sets``, and one MINP_SCORE record per set -- ``n_le_minp``
        (permutations whose smallest within-set count over ALL valid sets is at most the set's own ``n_ge``) and
        ``n_le_stepdown`` (the same with the sets of a smaller ``n_ge`` left out); a NaN score gives 0 / 0, an NA member
        -1 / -1.  With ``min_count`` also uint32 [iters], per permutation the smallest count
        over the valid sets (0xFFFFFFFF without one); with ``counts`` also uint32 [sets][iters], the count R of every null
        score within its own row -- the permutations of that set whose null score is at least as large (rows of 0xFFFFFFFF
        for sets with an NA member).  ``report.minp_columns`` turns the records into p-values.  Errors raise GcreError."""
        lib = _minp_lib()
        inp, keep = _set_input(sets, rows, signs, self.num_cases + self.num_ctrls)
        S = inp.n_sets
        out = np.zeros(max(S, 1), dtype=SET_SCORE)
        mp = np.zeros(max(S, 1), dtype=MINP_SCORE)
        mc = np.full(self.iters, 0xFFFFFFFF, dtype=np.uint32) if min_count else None
        cn = np.full((S, self.iters), 0xFFFFFFFF, dtype=np.uint32) if counts else None
        n_out = ctypes.c_int64(0)
        self._check_gcre(lib.gcre_score_sets_minp(self._h, ctypes.byref(inp), _ptr(out), len(out), ctypes.byref(n_out), _ptr(mp),
                                                  _ptr(mc) if min_count and mc.size else None,
                                                  _ptr(cn) if counts and cn.size else None))
        res = (out[:n_out.value], mp[:n_out.value])
        return res + ((mc,) if min_count else ()) + ((cn,) if counts else ())

    def minp_launches(self) -> int:
        """k_minp_gather / k_family_null / k_minp_rank / k_minp_scan launches of ``minp_tests`` on this context so far."""
        return int(_minp_lib().gcre_minp_launches(self._h))

    def competitive_tests(self, sets, rows, signs=None, bins=None, draws: int = 1000, seed: int = 0, null: bool = False,
                          picks: bool = False):
        """Competitive tests of the given sets (gcre_score_sets_compete): every set against ``draws`` random
        sets of the same size, drawn from ``rows`` -- here the whole gene POOL, not only the members -- and scored on the
        observed labels.  ``sets`` / ``signs`` as ``score_sets`` takes them (lists per set, or an ``(off, members)`` pair with
        flat signs).  ``bins``: per row of ``rows`` its bin 0 .. max, or -1 for a row that is never drawn (a member on
        such a row is fixed: it stays itself in every draw); None = one bin.  A member is replaced by a row of its own bin.
        No permutation mask is read: a context with ``iters`` = 0 will do.  Returns ``(records, n_ge)``: the SET_SCORE
        records of ``score_sets``, and int64 per set the draws whose score reaches the set's (-1 for an NA member).  With
        ``null`` also float64 [sets][draws], the score of every draw (NaN rows for sets with an NA member); with ``picks``
        also int32 [draws][members of all sets], the row every member received.  ``report.competitive_columns`` turns n_ge
        into p-values, ``report.competitive_reference`` restates the call in numpy.  Errors raise GcreError."""
        inp, keep = _set_input(sets, rows, signs, self.num_cases + self.num_ctrls)
        S = inp.n_sets
        B = int(draws)
        nb = 1
        bn = None
        if bins is not None:
            bn = np.ascontiguousarray(np.asarray(bins, dtype=np.int64).reshape(-1), dtype=np.int32)
            if len(bn) != keep[3].shape[0]:
                raise ValueError(f"bins: {len(bn)} entries for {keep[3].shape[0]} rows")
            nb = max(int(bn.max()) + 1, 1) if len(bn) else 1
        lib = _compete_lib()
        out = np.zeros(max(S, 1), dtype=SET_SCORE)
        ge = np.zeros(max(S, 1), dtype=np.int64)
        nul = np.full((S, max(B, 0)), np.nan, dtype=np.float64) if null else None
        pk = np.full((max(B, 0), len(keep[1])), -1, dtype=np.int32) if picks else None
        n_out = ctypes.c_int64(0)
        self._check_gcre(lib.gcre_score_sets_compete(self._h, ctypes.byref(inp), _ptr(bn), nb, B, int(seed) & (2**64 - 1), _ptr(out),
                                                     len(out), ctypes.byref(n_out), _ptr(ge),
                                                     _ptr(nul) if null and nul.size else None,
                                                     _ptr(pk) if picks and pk.size else None))
        res = (out[:n_out.value], ge[:n_out.value])
        return res + ((nul,) if null else ()) + ((pk,) if picks else ())

    def compete_launches(self) -> int:
        """k_compete_null launches of ``competitive_tests`` on this context so far."""
        return int(_compete_lib().gcre_compete_launches(self._h))

    def prefix_tests(self, sets, rows, signs=None, cuts=None, family: bool = False, null: bool = False, steps: bool = False):
        """Variable-threshold tests of the given sets (gcre_score_sets_prefix): the best score over nested
        prefixes of every set's member list, with the same maximum taken under every permutation.  ``sets`` / ``rows`` /
        ``signs`` as ``score_sets`` takes them (lists per set, or an ``(off, members)`` pair with flat signs); the ORDER of a
        set's members is the order its prefixes grow in (``report.threshold_order``).  ``cuts`` follows ``signs``: per member
        non-zero where a prefix may end (the last member of a set always ends one); None = every member.  Returns
        ``(records, prefix)``: the SET_SCORE records of ``score_sets`` for the full sets, and one PREFIX_SCORE record per set
        -- ``score`` the best step's observed score, ``best_step`` / ``best_members`` which prefix that is, ``steps``, its
        four counts, and ``n_ge`` the permutations whose maximum over the steps reaches ``score`` (-1 for an NA member).
        With ``family`` also float32 [iters], per permutation the maximum over the sets; with ``null`` also float32
        [sets][iters], the maximum over every set's steps (NaN rows for sets with an NA member); with ``steps`` also float64
        [members], the observed score of the step ending at every member (NaN where none does).  The order and the cuts must
        not be chosen from the labels.  Errors raise GcreError."""
        S, off, members, sg = _set_lists(sets, signs)
        ct = _prefix_cuts(sets, cuts, S, off, members)
        lib = _prefix_lib()
        inp, keep = _set_input((off, members), rows, sg, self.num_cases + self.num_ctrls)
        out = np.zeros(max(S, 1), dtype=SET_SCORE)
        px = np.zeros(max(S, 1), dtype=PREFIX_SCORE)
        fam = np.zeros(self.iters, dtype=np.float32) if family else None
        nul = np.full((S, self.iters), np.nan, dtype=np.float32) if null else None
        stp = np.full(len(members), np.nan, dtype=np.float64) if steps else None
        n_out = ctypes.c_int64(0)
        self._check_gcre(lib.gcre_score_sets_prefix(self._h, ctypes.byref(inp), _ptr(ct) if ct is not None and ct.size else None,
                                                    _ptr(out), len(out), ctypes.byref(n_out), _ptr(px),
                                                    _ptr(fam) if family and fam.size else None,
                                                    _ptr(nul) if null and nul.size else None,
                                                    _ptr(stp) if steps and stp.size else None))
        res = (out[:n_out.value], px[:n_out.value])
        return res + ((fam,) if family else ()) + ((nul,) if null else ()) + ((stp,) if steps else ())

    def subsample_tests(self, sets, rows, signs=None, m_cases=None, m_ctrls=None, draws: int = 100, seed: int = 0, table_a=None,
                        table_b=None, cuts=None, scores: bool = False):
        """Split-half stability of the given sets (gcre_score_sets_subsample): every set scored on ``draws``
        random halves of the cohort -- ``m_cases`` of the cases and ``m_ctrls`` of the controls (None: ``n // 2`` of each
        label), half A -- and on the complementary halves, half B.  ``sets`` / ``rows`` / ``signs`` as ``score_sets`` takes
        them.  ``table_a`` / ``table_b``: the value tables of the two half cohorts (None: ``values_table(m_cases, m_ctrls)``
        and that of the patients left); ``table_b=False`` scores half A only.  ``cuts``: the cut-offs in score units, one
        list for every set or one list per set (at most 8 each); None = no counts.  No permutation mask is read: a context
        with ``iters`` = 0 will do.  Returns ``(records, counts)``: the SET_SCORE records of ``score_sets`` on the full
        cohort, and ``counts`` with ``n_a`` / ``n_b`` / ``n_both``, int64 [sets][cuts] -- the draws in which half A, half B
        and both reach the cut (-1 for a set with an NA member; ``n_b`` and ``n_both`` None without half B).  With ``scores``
        also float64 [sets][draws] twice, the A and the B score of every draw (NaN rows for sets with an NA member; None
        for B without half B).  ``report.stability_columns`` turns the counts into frequencies, ``report.subsample_reference``
        restates the call in numpy.  Errors raise GcreError."""
        inp, keep = _set_input(sets, rows, signs, self.num_cases + self.num_ctrls)
        S = inp.n_sets
        B = int(draws)
        ma = self.num_cases // 2 if m_cases is None else int(m_cases)
        mt = self.num_ctrls // 2 if m_ctrls is None else int(m_ctrls)
        ct = None
        n_cut = 0
        if cuts is not None:
            ct = np.asarray(cuts, dtype=np.float64)
            if ct.ndim == 1:
                ct = np.broadcast_to(ct, (S, len(ct)))
            if ct.ndim != 2 or ct.shape[0] != S:
                raise ValueError(f"cuts: one list, or one list per set ({S} sets), not shape {ct.shape}")
            n_cut = ct.shape[1]
            ct = np.ascontiguousarray(ct) if ct.size else np.zeros(max(n_cut, 1))     # (no set: still an array to point to)
        half_b = table_b is not False
        in_range = 0 <= ma <= self.num_cases and 0 <= mt <= self.num_ctrls     # (otherwise the library refuses)
        if table_a is None and in_range:
            table_a = values_table(ma, mt)
        if table_b is None and in_range:
            table_b = values_table(self.num_cases - ma, self.num_ctrls - mt)
        ta = None if table_a is None else np.ascontiguousarray(table_a, dtype=np.float64)
        tb = np.ascontiguousarray(table_b, dtype=np.float64) if half_b and table_b is not None else None
        if any(t is not None and t.ndim != 2 for t in (ta, tb)):
            raise ValueError("table_a / table_b: a value table has rows and columns")
        lib = _subsample_lib()
        out = np.zeros(max(S, 1), dtype=SET_SCORE)
        cnt = [np.zeros((max(S, 1), n_cut), dtype=np.int64) if h == 0 or half_b else None for h in range(3)]
        sc = [np.full((S, max(B, 0)), np.nan, dtype=np.float64) if scores and (h == 0 or half_b) else None for h in range(2)]
        n_out = ctypes.c_int64(0)
        given = lambda a: _ptr(a) if a is not None and a.size else None
        self._check_gcre(lib.gcre_score_sets_subsample(
            self._h, ctypes.byref(inp), ma, mt, B, int(seed) & (2**64 - 1),
            _ptr(ta), 0 if ta is None else ta.shape[0], 0 if ta is None else ta.shape[1],
            _ptr(tb), 0 if tb is None else tb.shape[0], 0 if tb is None else tb.shape[1],
            given(ct), n_cut, _ptr(out), len(out), ctypes.byref(n_out), given(cnt[0]), given(cnt[1]), given(cnt[2]),
            given(sc[0]), given(sc[1])))
        n = n_out.value
        counts = {k: None if c is None else c[:n] for k, c in zip(("n_a", "n_b", "n_both"), cnt)}
        return (out[:n], counts) + ((sc[0], sc[1]) if scores else ())

    def dose_tests(self, sets, rows, signs=None, levels=(1, 2), family: bool = False, null: bool = False,
                   level_scores: bool = False):
        """Multi-hit tests of the given sets (gcre_score_sets_dose): per set and per level m of ``levels`` the
        row "patients who carry at least m of the set's members" is scored, the best level is the statistic, and the same
        maximum is taken under every permutation.  ``sets`` / ``rows`` / ``signs`` as ``score_sets`` takes them (lists per set,
        or an ``(off, members)`` pair with flat signs); ``levels``: 1 to 15 strictly ascending integers in 1 .. 15, the same
        for every set.  Method 1 counts all members whatever their signs (a member listed twice counts twice); method 2
        counts the (+) and the (-) members apart, into the two halves of the row.  Level 1 is the set's union.  Returns
        ``(records, dose)``: the SET_SCORE records of ``score_sets`` for the full sets, and one DOSE_SCORE record per set --
        ``score`` the best level's observed score, ``best_index`` / ``best_level`` which level that is (the smallest that
        attains the maximum), ``levels``, its four counts, and ``n_ge`` the permutations whose maximum over the levels
        reaches ``score`` (-1 for an NA member).  With ``family`` also float32 [iters], per permutation the maximum over the
        sets; with ``null`` also float32 [sets][iters], the maximum over every set's levels (NaN rows for sets with an NA
        member); with ``level_scores`` also float64 [sets][levels], the observed score of every level row (NaN rows
        likewise).  ``report.dose_sets`` restates the level rows in numpy; ``report.pair_sets`` with ``levels=[2]`` screens
        gene pairs.  The levels must not be chosen from the labels.  Bad ``levels`` raise ValueError, errors of the library
        GcreError."""
        S, off, members, sg = _set_lists(sets, signs)
        lv = _dose_levels(levels)
        lib = _dose_lib()
        inp, keep = _set_input((off, members), rows, sg, self.num_cases + self.num_ctrls)
        L = len(lv)
        out = np.zeros(max(S, 1), dtype=SET_SCORE)
        ds = np.zeros(max(S, 1), dtype=DOSE_SCORE)
        fam = np.zeros(self.iters, dtype=np.float32) if family else None
        nul = np.full((S, self.iters), np.nan, dtype=np.float32) if null else None
        lsc = np.full((S, L), np.nan, dtype=np.float64) if level_scores else None
        n_out = ctypes.c_int64(0)
        self._check_gcre(lib.gcre_score_sets_dose(self._h, ctypes.byref(inp), _ptr(lv), L, _ptr(out), len(out), ctypes.byref(n_out),
                                                  _ptr(ds), _ptr(fam) if family and fam.size else None,
                                                  _ptr(nul) if null and nul.size else None,
                                                  _ptr(lsc) if level_scores and lsc.size else None))
        res = (out[:n_out.value], ds[:n_out.value])
        return res + ((fam,) if family else ()) + ((nul,) if null else ()) + ((lsc,) if level_scores else ())

    def sequential_tests(self, sets, rows, signs=None, hits: int = 20, max_perms: int = 10**6, seed: int = 0, strata=None):
        """Sequential permutation p-values of the given sets (gcre_score_sets_sequential): every set is
        permuted until its null score has reached its observed score ``hits`` times, or ``max_perms`` permutations are used.
        ``sets`` / ``rows`` / ``signs`` as ``score_sets`` takes them.  The permutations are those ``generate_permutations(seed,
        strata)`` draws -- permutation r is the same mask here and there -- but they are made in batches as they are needed
        and never kept, so ``max_perms`` may be far above what a context can hold, and a context with ``iters`` = 0 will do.
        Returns ``(records, seq)``: the SET_SCORE records of ``score_sets`` on this context, and one SEQ_SCORE record per
        set -- ``n_hit`` the exceedances counted, ``n_perm`` the permutations used (the position of the ``hits``-th
        exceedance, or ``max_perms``), ``stopped`` whether it was reached; ``n_hit`` = ``n_perm`` = -1 for a set with an NA
        member.  ``n_hit / n_perm`` is the set's nominal p-value (``report.sequential_columns``); no value depends on the
        batches.  ``report.sequential_reference`` states the rule in numpy.  Errors raise GcreError."""
        inp, keep = _set_input(sets, rows, signs, self.num_cases + self.num_ctrls)
        S = inp.n_sets
        lib = _feature_lib("sequential")
        _, st, n_strata = self._sequential_draw(strata, None)
        out = np.zeros(max(S, 1), dtype=SET_SCORE)
        seq = np.zeros(max(S, 1), dtype=SEQ_SCORE)
        n_out = ctypes.c_int64(0)
        self._check_gcre(lib.gcre_score_sets_sequential(self._h, ctypes.byref(inp), int(seed) & (2**64 - 1), _ptr(st), n_strata,
                                                        int(hits), int(max_perms), _ptr(out), len(out), ctypes.byref(n_out),
                                                        _ptr(seq)))
        return out[:n_out.value], seq[:n_out.value]

    def weighted_sequential_tests(self, sets, rows, signs=None, odds=None, hits: int = 20, max_perms: int = 10**6, seed: int = 0,
                                  strata=None, max_attempts: int = 1 << 20):
        """Sequential permutation p-values under covariate-adjusted permutations (gcre_score_sets_sequential_weighted;
        DESIGN.md §3.24): ``sequential_tests`` with the masks ``generate_weighted_permutations(seed, odds, strata,
        max_attempts)`` draws -- permutation r is the same mask here and there -- made in batches as they are needed and never
        kept.  ``odds`` (required) and ``strata`` as ``generate_weighted_permutations`` reads them (any integer ids, mapped to
        0 .. S-1 in ascending order).  Returns ``(records, seq)`` as ``sequential_tests`` does.  Each weighted permutation
        costs about sqrt(2 pi V) attempts over the whole stratum, where a uniform one costs one hash per patient.

        Let R be the first permutation below ``max_perms`` with a stratum that has no accepted attempt below ``max_attempts``.
        The sets are scored on the permutations in front of R; if every set has stopped there, the answer is complete and
        returned, otherwise the call raises GcreError (GCRE_ERR_RANGE) naming R, the stratum, the cap and the sets still
        active.  ``report.weighted_sequential_reference`` states the rule in numpy.  ``sequential_launches`` counts the
        kernels: four per batch.  A missing or misshapen ``odds`` / ``strata`` is a ValueError; other errors raise
        GcreError."""
        if odds is None:
            raise ValueError("odds: one value per patient is required (sequential_tests draws uniform permutations)")
        w, st, S, _ = _weighted_args(odds, strata, self.num_cases + self.num_ctrls)
        inp, keep = _set_input(sets, rows, signs, self.num_cases + self.num_ctrls)
        n_sets = inp.n_sets
        lib = _feature_lib("sequential_weighted")
        out = np.zeros(max(n_sets, 1), dtype=SET_SCORE)
        seq = np.zeros(max(n_sets, 1), dtype=SEQ_SCORE)
        n_out = ctypes.c_int64(0)
        self._check_gcre(lib.gcre_score_sets_sequential_weighted(self._h, ctypes.byref(inp), int(seed) & (2**64 - 1), _ptr(w), _ptr(st),
                                                                 S if st is not None else 0, int(max_attempts), int(hits),
                                                                 int(max_perms), _ptr(out), len(out), ctypes.byref(n_out), _ptr(seq)))
        return out[:n_out.value], seq[:n_out.value]

    def _sequential_draw(self, strata, odds):
        """(odds or None, strata ids or None, n_strata) of the two adaptive sequential entries: uniform permutations read
        ``strata`` as ``sequential_tests`` does, weighted ones ``odds`` / ``strata`` as ``weighted_sequential_tests``."""
        n = self.num_cases + self.num_ctrls
        if odds is not None:
            w, st, S, _ = _weighted_args(odds, strata, n)
            return w, st, S if st is not None else 0
        st = None if strata is None else np.ascontiguousarray(strata, dtype=np.int32).reshape(-1)
        if st is not None and len(st) != n:
            raise ValueError(f"strata: one id per patient ({n}), not {len(st)}")
        return None, st, 0 if st is None else int(st.max()) + 1

    def prefix_sequential_tests(self, sets, rows, signs=None, cuts=None, hits: int = 20, max_perms: int = 10**6, seed: int = 0,
                                strata=None, odds=None, max_attempts: int = 1 << 20, steps: bool = False):
        """Sequential p-values of the variable-threshold test (gcre_score_sets_prefix_sequential): the
        statistic of ``prefix_tests`` -- the best score over nested prefixes of every set's member list -- with the
        permutations of ``sequential_tests`` drawn in batches as they are needed: every set is permuted until the maximum
        over its steps has reached its best observed score ``hits`` times, or ``max_perms`` permutations are used.  No
        resident mask is read: a context with ``iters`` = 0 will do.  ``sets`` / ``rows`` / ``signs`` / ``cuts`` / ``steps``
        as ``prefix_tests`` takes them; ``seed`` / ``strata`` as ``sequential_tests``; with ``odds`` the masks, ``strata``,
        ``max_attempts`` and the refusal (GcreError, GCRE_ERR_RANGE) are ``weighted_sequential_tests``'.  Returns ``(records,
        prefix, seq)``: the SET_SCORE records of ``score_sets``, the PREFIX_SCORE records of ``prefix_tests`` with ``n_ge`` 0
        (-1 for an NA member), and one SEQ_SCORE record per set as ``sequential_tests`` gives them.  ``n_hit / n_perm`` is a
        nominal p-value of the maximum, one set at a time.  With ``steps`` also float64 [members].
        ``report.adaptive_sequential_reference`` states the rule in numpy.  A misshapen ``cuts`` / ``odds`` / ``strata`` is a
        ValueError; other errors raise GcreError."""
        S, off, members, sg = _set_lists(sets, signs)
        ct = _prefix_cuts(sets, cuts, S, off, members)
        w, st, n_strata = self._sequential_draw(strata, odds)
        lib = _feature_lib("seq_prefix")
        inp, keep = _set_input((off, members), rows, sg, self.num_cases + self.num_ctrls)
        out = np.zeros(max(S, 1), dtype=SET_SCORE)
        px = np.zeros(max(S, 1), dtype=PREFIX_SCORE)
        seq = np.zeros(max(S, 1), dtype=SEQ_SCORE)
        stp = np.full(len(members), np.nan, dtype=np.float64) if steps else None
        n_out = ctypes.c_int64(0)
        self._check_gcre(lib.gcre_score_sets_prefix_sequential(
            self._h, ctypes.byref(inp), _ptr(ct) if ct is not None and ct.size else None, int(seed) & (2**64 - 1), _ptr(w), _ptr(st),
            n_strata, int(max_attempts), int(hits), int(max_perms), _ptr(out), len(out), ctypes.byref(n_out), _ptr(px), _ptr(seq),
            _ptr(stp) if steps and stp.size else None))
        n = n_out.value
        return (out[:n], px[:n], seq[:n]) + ((stp,) if steps else ())

    def dose_sequential_tests(self, sets, rows, signs=None, levels=(1, 2), hits: int = 20, max_perms: int = 10**6, seed: int = 0,
                              strata=None, odds=None, max_attempts: int = 1 << 20, level_scores: bool = False):
        """Sequential p-values of the multi-hit test (gcre_score_sets_dose_sequential): the statistic of
        ``dose_tests`` -- the best score over the level rows "carries at least m of the set's members" -- with the
        permutations of ``sequential_tests`` drawn in batches as they are needed, every set until the maximum over its
        levels has reached its best observed score ``hits`` times.  ``sets`` / ``rows`` / ``signs`` / ``levels`` /
        ``level_scores`` as ``dose_tests`` takes them; everything else as ``prefix_sequential_tests``.  Returns ``(records,
        dose, seq)``: the DOSE_SCORE records with ``n_ge`` 0 (-1 for an NA member).  ``n_hit / n_perm`` is a nominal p-value
        of the maximum, one set at a time.  With ``level_scores`` also float64 [sets][levels].  Bad ``levels`` / ``odds`` /
        ``strata`` raise ValueError, errors of the library GcreError."""
        S, off, members, sg = _set_lists(sets, signs)
        lv = _dose_levels(levels)
        w, st, n_strata = self._sequential_draw(strata, odds)
        lib = _feature_lib("seq_prefix")
        inp, keep = _set_input((off, members), rows, sg, self.num_cases + self.num_ctrls)
        L = len(lv)
        out = np.zeros(max(S, 1), dtype=SET_SCORE)
        ds = np.zeros(max(S, 1), dtype=DOSE_SCORE)
        seq = np.zeros(max(S, 1), dtype=SEQ_SCORE)
        lsc = np.full((S, L), np.nan, dtype=np.float64) if level_scores else None
        n_out = ctypes.c_int64(0)
        self._check_gcre(lib.gcre_score_sets_dose_sequential(
            self._h, ctypes.byref(inp), _ptr(lv), L, int(seed) & (2**64 - 1), _ptr(w), _ptr(st), n_strata, int(max_attempts), int(hits),
            int(max_perms), _ptr(out), len(out), ctypes.byref(n_out), _ptr(ds), _ptr(seq),
            _ptr(lsc) if level_scores and lsc.size else None))
        n = n_out.value
        return (out[:n], ds[:n], seq[:n]) + ((lsc,) if level_scores else ())

    def seq_prefix_launches(self) -> int:
        """Kernels ``prefix_sequential_tests`` and ``dose_sequential_tests`` launched for their own stage on this context so
        far: three per slab, then three per batch (four weighted)."""
        return int(_feature_lib("seq_prefix").gcre_seq_prefix_launches(self._h))

    def strata_tests(self, sets, rows, signs=None, strata=None, tables=None, family: bool = False, null: bool = False,
                     terms: bool = False):
        """Stratified scores of the given sets (gcre_score_sets_strata): every stratum of the cohort scored on
        its own counts against the value table of its own cases and controls, the terms summed in ascending order of the
        stratum, and the same sum taken under every permutation of the context.  ``sets`` / ``rows`` / ``signs`` as
        ``score_sets`` takes them.  ``strata``: one id per patient, any integers (mapped to 0 .. S-1 in ascending order of id;
        at most 16 distinct); required.  The context's masks must keep these strata: ``generate_permutations(seed, strata)``
        with the same ``strata`` -- anything else is refused.  ``tables``: one value table per stratum in ascending order of
        id (cells a table lacks read as -1); None = ``values_table(cases_s, ctrls_s)`` of every stratum.  Returns ``(records,
        strata_records)``: the SET_SCORE records of ``score_sets`` (the pooled score), and one STRATA_SCORE record per set --
        ``score`` the summed observed score and ``n_ge`` the permutations whose sum reaches it (-1 for an NA member; 0
        without permutations).  With ``family`` also float64 [iters], per permutation the maximum over the sets (NaN and
        negatives as +0); with ``null`` also float64 [sets][iters], the summed null score (NaN rows for sets with an NA
        member); with ``terms`` also float64 [sets][S], the observed terms, and int32 [sets][S][4], cases_pos, ctrls_pos,
        cases_neg, ctrls_neg inside every stratum.  ``n_ge / iters`` is a nominal p-value of the sum; the terms and counts
        are descriptive.  ``report.strata_reference`` restates the call in numpy.  Errors raise GcreError."""
        n = self.num_cases + self.num_ctrls
        inp, keep = _set_input(sets, rows, signs, n)
        S = inp.n_sets
        if strata is None:
            raise ValueError("strata: one id per patient is required (score_sets gives the pooled score)")
        ids, inv = np.unique(np.asarray(strata).reshape(-1), return_inverse=True)
        if len(inv) != n:
            raise ValueError(f"strata: one id per patient ({n}), not {len(inv)}")
        st = np.ascontiguousarray(inv, dtype=np.int32)
        NS = len(ids)
        if tables is None:
            tables = [values_table(int((st[:self.num_cases] == s).sum()), int((st[self.num_cases:] == s).sum())) for s in range(NS)]
        tabs = [np.ascontiguousarray(t, dtype=np.float64) for t in tables]
        if len(tabs) != NS or any(t.ndim != 2 for t in tabs):
            raise ValueError(f"tables: one value table (rows and columns) per stratum ({NS}), in ascending order of id")
        nrow = np.array([t.shape[0] for t in tabs], dtype=np.int32)
        ncol = np.array([t.shape[1] for t in tabs], dtype=np.int32)
        toff = np.concatenate([[0], np.cumsum([t.size for t in tabs])[:-1]]).astype(np.int64) if NS else np.zeros(0, np.int64)
        flat = np.ascontiguousarray(np.concatenate([t.reshape(-1) for t in tabs] + [np.zeros(1)]))   # (never empty)
        lib = _strata_lib()
        out = np.zeros(max(S, 1), dtype=SET_SCORE)
        sr = np.zeros(max(S, 1), dtype=STRATA_SCORE)
        fam = np.zeros(self.iters, dtype=np.float64) if family else None
        nul = np.full((S, self.iters), np.nan, dtype=np.float64) if null else None
        trm = np.full((S, NS), np.nan, dtype=np.float64) if terms else None
        cnt = np.zeros((S, NS, 4), dtype=np.int32) if terms else None
        n_out = ctypes.c_int64(0)
        given = lambda a: _ptr(a) if a is not None and a.size else None
        self._check_gcre(lib.gcre_score_sets_strata(self._h, ctypes.byref(inp), _ptr(st), NS, _ptr(flat), _ptr(nrow), _ptr(ncol),
                                                    _ptr(toff), _ptr(out), len(out), ctypes.byref(n_out), _ptr(sr), given(trm),
                                                    given(cnt), given(nul), given(fam)))
        res = (out[:n_out.value], sr[:n_out.value])
        return res + ((fam,) if family else ()) + ((nul,) if null else ()) + ((trm, cnt) if terms else ())

    def strata_launches(self) -> int:
        """Kernels ``strata_tests`` launched for its own stage on this context so far: the indicator rows, the check of the
        masks, one per table, then three per slab (two without permutations)."""
        return int(_strata_lib().gcre_strata_launches(self._h))

    def sequential_launches(self) -> int:
        """Kernels ``sequential_tests`` launched for its own stage on this context so far: three per batch; and those of
        ``weighted_sequential_tests``: four per batch, the search alone for a batch whose first permutation is left over."""
        return int(_feature_lib("sequential").gcre_sequential_launches(self._h))

    def dose_launches(self) -> int:
        """Kernels ``dose_tests`` launched for its own stage on this context so far."""
        return int(_dose_lib().gcre_dose_launches(self._h))

    def subsample_launches(self) -> int:
        """Kernels ``subsample_tests`` launched for its own stage on this context so far: one per table, two per slab."""
        return int(_subsample_lib().gcre_subsample_launches(self._h))

    def prefix_launches(self) -> int:
        """Kernels ``prefix_tests`` launched for its own stage on this context so far."""
        return int(_prefix_lib().gcre_prefix_launches(self._h))

    def set_overlap(self, sets, rows, a=None, b=None):
        """Carrier overlaps of caller-given sets (gcre_set_overlap).  A set's carrier row is the OR of all
        its members (row indices of the 0/1 matrix ``rows``; -1 = NA gene), whatever the method; ``sets``: one sequence of
        members per set, or an ``(off, members)`` pair as ``clump_sets`` takes it.  Returns ``(size, both)``:
        ``size`` int32 [S][2] = the carriers of every set among the cases and among the controls ((-1, -1) with an NA
        member), ``both`` int32 [na][nb][2] = the patients sets ``a[i]`` and ``b[j]`` share, cases and controls (zeros
        where either has an NA member).  ``a`` / ``b``: set indices, repeats allowed; None = every set in order.  Needs
        neither a value table nor permutation masks.  Errors raise GcreError with the library's message."""
        lib = _overlap_lib()
        inp, keep = _set_input(sets, rows, None, self.num_cases + self.num_ctrls)
        S = inp.n_sets
        ia = None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.int64).reshape(-1))
        ib = None if b is None else np.ascontiguousarray(np.asarray(b, dtype=np.int64).reshape(-1))
        na = S if ia is None else len(ia)
        nb = S if ib is None else len(ib)
        size = np.zeros((S, 2), dtype=np.int32)
        both = np.zeros((na, nb, 2), dtype=np.int32)
        self._check_gcre(lib.gcre_set_overlap(self._h, ctypes.byref(inp), _ptr(ia), na, _ptr(ib), nb, _ptr(size), _ptr(both)))
        return size, both

    def clump_sets(self, sets, rows, order, r: float = 0.5, measure: str = "jaccard", patients: str = "all"):
        """Greedy clumping of caller-given sets by shared carriers, on the device (gcre_clump_sets):
        ``report.clump_rows(order, size, both_of, r, measure, patients)`` with ``size`` / ``both`` as ``set_overlap``
        defines them, bit for bit, without a pair count leaving the GPU.  ``sets``: one sequence of row indices of the
        0/1 matrix ``rows`` per set, or a pair ``(off, members)`` -- int64 [S + 1] offsets into int32 members, what
        ``report.hit_sets`` returns; ``order``: the sets to clump, best first, each at most once, none with an NA member
        (-1).  Returns ``(clump, lead, value, shared, size)``: int64 [S] clump ids, int64 [S] the lead's set (a lead names
        itself), float64 [S] the measure against the lead (NaN on leads), int64 [S][2] the carriers shared with it (-1 on
        leads) -- all -1 / NaN for a set outside ``order`` -- and int32 [S][2] the sets' carriers.  Raises the
        ValueErrors of ``clump_rows`` before the library is touched; the library's refusals raise GcreError."""
        if not 0 < r <= 1:
            raise ValueError("r must be > 0 and <= 1")
        if measure not in ("jaccard", "containment"):
            raise ValueError("measure must be 'jaccard' or 'containment'")
        if patients not in ("all", "cases"):
            raise ValueError("patients must be 'all' or 'cases'")
        lib = _clump_lib()
        inp, keep = _set_input(sets, rows, None, self.num_cases + self.num_ctrls)
        S = inp.n_sets
        io = np.ascontiguousarray(np.asarray(order, dtype=np.int64).reshape(-1))
        size = np.zeros((S, 2), dtype=np.int32)
        clump = np.zeros(S, dtype=np.int64)
        lead = np.zeros(S, dtype=np.int64)
        value = np.zeros(S, dtype=np.float64)
        shared = np.zeros((S, 2), dtype=np.int32)
        self._check_gcre(lib.gcre_clump_sets(self._h, ctypes.byref(inp), _ptr(io), len(io), float(r),
                                             0 if measure == "jaccard" else 1, 0 if patients == "all" else 1,
                                             _ptr(size), _ptr(clump), _ptr(lead), _ptr(value), _ptr(shared)))
        return clump, lead, value, shared.astype(np.int64), size

    @property
    def clump_launches(self) -> int:
        """Kernels gcre_clump_sets launched on this context so far."""
        return int(_clump_lib().gcre_clump_launches(self._h))

    def patient_counts(self, sets, rows, which=None, group=None, n_groups=None, by_sign: bool = False, signs=None):
        """How many of the listed sets each patient carries (gcre_set_patient_counts): exact counts,
        descriptive only -- no test statistic, and the carriers of sets selected on the case / control labels are enriched
        in cases by construction.  ``sets``: one sequence of row indices of the 0/1 matrix ``rows`` per set (-1 = NA
        gene), or a pair ``(off, members)`` as ``clump_sets`` takes it (``signs`` then one flat array); ``which``: the sets
        to count, repeats allowed and counted as often (None: every set once); ``group``: per entry 0 .. n_groups - 1, or
        -1 = not counted (None: all in group 0); ``n_groups``: None = 1 without ``group``, max(group) + 1 (at least 1) with
        it.  ``by_sign`` False: one plane, the carrier row of ``set_overlap`` (the OR of all members); True: two planes,
        the OR of the +1 members and the OR of the -1 members of ``signs`` (as ``score_sets`` takes them; None: all +1),
        whatever the context's method.  Returns ``(counts, group_sets, skipped)``: int32 [n_groups][1 + by_sign][n],
        int64 [n_groups] the entries counted into every group, and the number of entries with a group whose set has an NA
        member (counted nowhere).  An index out of range, ``group`` of another length than the entries, or a wrong signs
        shape raise ValueError before the library is touched; the library's refusals raise GcreError."""
        S, off, members, sg = _set_lists(sets, signs)
        iw = None if which is None else np.ascontiguousarray(np.asarray(which, dtype=np.int64).reshape(-1))
        ig = None if group is None else np.ascontiguousarray(np.asarray(group, dtype=np.int64).reshape(-1))
        E = S if iw is None else len(iw)
        if iw is not None and len(iw) and (iw.min() < 0 or iw.max() >= S):
            raise ValueError(f"which: a set index outside 0..{S - 1}")
        if ig is not None and len(ig) != E:
            raise ValueError(f"group: {len(ig)} entries for {E} counted sets (one per entry of which, or per set)")
        if n_groups is None:
            n_groups = 1 if ig is None or not len(ig) else max(int(ig.max()) + 1, 1)
        G = int(n_groups)
        if G < 1:
            raise ValueError(f"n_groups must be at least 1, not {n_groups!r}")
        if ig is None and G != 1:
            raise ValueError(f"group: None puts every entry in group 0, so n_groups must be 1, not {G}")
        if ig is not None and len(ig) and (ig.min() < -1 or ig.max() >= G):
            raise ValueError(f"group: a group outside -1..{G - 1}")
        lib = _patients_lib()
        inp, keep = _set_input((off, members), rows, sg, self.num_cases + self.num_ctrls)
        ig32 = None if ig is None else np.ascontiguousarray(ig, dtype=np.int32)
        H = 2 if by_sign else 1
        counts = np.zeros((G, H, inp.n_cols), dtype=np.int32)
        group_sets = np.zeros(G, dtype=np.int64)
        skipped = ctypes.c_int64(0)
        self._check_gcre(lib.gcre_set_patient_counts(self._h, ctypes.byref(inp), _ptr(iw), E, _ptr(ig32), G, 1 if by_sign else 0,
                                                     _ptr(counts), _ptr(group_sets), ctypes.byref(skipped)))
        return counts, group_sets, int(skipped.value)

    @property
    def patient_launches(self) -> int:
        """Kernels gcre_set_patient_counts launched on this context so far."""
        return int(_patients_lib().gcre_patient_launches(self._h))

    def patient_burden(self, weights, null: bool = False):
        """Burden tests of per-patient weights (gcre_patient_burden): for every row of non-negative
        integer ``weights`` -- [rows][n], or the [G][H][n] counts ``patient_counts`` returns, flattened to G * H rows --
        the weighted sum over the cases, ``observed``, against the same sum over the cases of every one of the context's
        permutation masks (all of them, whatever the permutation window; strata come in through the masks).  Returns a
        dict of arrays with one entry per row: ``total``, ``observed``, ``n_ge``, ``n_le`` (int64: the permutations whose
        sum is >= / <= the observed one; a tie counts in both), ``planes`` (int32, the bit length of the row's largest
        weight), ``p_upper`` = n_ge / iterations, ``p_lower`` = n_le / iterations (NaN at 0 iterations) and, with
        ``null``, ``null``: int64 [rows][iterations], every null sum.  All sums are exact integers.  A p-value on weights
        selected on these very labels (the tallies of a run's own significant paths) is meaningless.  A wrong shape, a
        negative weight or one above 2^31 - 1 raise ValueError before the library is touched; the library's refusals
        raise GcreError (ValueError: no permutation masks set)."""
        n = self.num_cases + self.num_ctrls
        w = np.asarray(weights)
        if w.dtype == object or not (np.issubdtype(w.dtype, np.integer) or np.issubdtype(w.dtype, np.bool_)):
            raise ValueError(f"weights: integers, not {w.dtype}")
        if w.ndim not in (2, 3) or w.shape[-1] != n:
            raise ValueError(f"weights: [rows][{n}] or [groups][planes][{n}] (n_cases + n_ctrls columns), not {list(w.shape)}")
        w = w.reshape(-1, n)
        if w.size and (int(w.min()) < 0 or int(w.max()) > 2**31 - 1):
            raise ValueError("weights: every weight must lie in 0 .. 2^31 - 1")
        w32 = np.ascontiguousarray(w, dtype=np.int32)
        lib = _burden_lib()
        R = w32.shape[0]
        rec = np.zeros(R, dtype=BURDEN)
        sums = np.zeros((R, self.iters), dtype=np.int64) if null else None
        rc = lib.gcre_patient_burden(self._h, _ptr(w32), R, n, _ptr(rec), _ptr(sums))
        if rc != GCRE_OK:
            self._raise(rc)
        out = {k: np.ascontiguousarray(rec[k]) for k in ("total", "observed", "n_ge", "n_le", "planes", "p_upper", "p_lower")}
        if null:
            out["null"] = sums
        return out

    @property
    def burden_launches(self) -> int:
        """Kernels gcre_patient_burden launched on this context so far."""
        return int(_burden_lib().gcre_burden_launches(self._h))

    def stepdown_launches(self) -> int:
        """k_stepdown_null / k_stepdown_finish launches of this context so far."""
        return int(_stepdown_lib().gcre_stepdown_launches(self._h))

    def overlap_launches(self) -> int:
        """k_set_overlap launches of this context so far."""
        return int(_overlap_lib().gcre_overlap_launches(self._h))

    def perm_mask(self, r: int) -> np.ndarray:
        out = np.zeros(self.width_ul, dtype=np.uint64)
        self._check(self._lib.gcre_get_perm_mask(self._h, int(r), _ptr(out)))
        return out

    def test_range_union(self, p1, pz, zindex, loc, cnt, wp: int, method: int):
        """Tests: the range check of a hinted join (k_range_union) on given rows.  p1[n1][S], pz[nz][S] uint64 with
        S = method * wp; zindex[n1] (bit 31 = halves swapped); ranges loc[r] .. loc[r] + cnt[r] - 1.
        Returns (U[n_ranges][S], bad, rows per piece)."""
        p1 = np.ascontiguousarray(p1, dtype=np.uint64)
        pz = np.ascontiguousarray(pz, dtype=np.uint64)
        zindex = np.ascontiguousarray(zindex, dtype=np.int32)
        loc = np.ascontiguousarray(loc, dtype=np.int64)
        cnt = np.ascontiguousarray(cnt, dtype=np.int32)
        S = method * wp
        assert p1.shape[1:] == (S,) and pz.shape[1:] == (S,) and len(zindex) == len(p1) and len(loc) == len(cnt)
        u = np.zeros((len(loc), S), dtype=np.uint64)
        bad = np.zeros(1, dtype=np.uint32)
        piece = np.zeros(1, dtype=np.int32)
        self._check(self._lib.gcre_test_range_union(self._h, _ptr(p1), len(p1), _ptr(pz), len(pz), _ptr(zindex), _ptr(loc), _ptr(cnt),
                                                    len(loc), S, wp, method, _ptr(u), _ptr(bad), _ptr(piece)))
        return u, int(bad[0]), int(piece[0])

    def test_expand(self, path_idx, location, signs, path_length: int, method: int, first: int, count: int):
        """Tests: the expansion of a join index (k_expand) for ordinals [first, first + count).  Returns (row0, row1)."""
        path_idx = np.ascontiguousarray(path_idx, dtype=np.int64)
        location = np.ascontiguousarray(location, dtype=np.int64)
        signs = np.ascontiguousarray(signs, dtype=np.int32)
        row0 = np.full(max(count, 1), 0xffffffff, dtype=np.uint32)
        row1 = np.full(max(count, 1), 0xffffffff, dtype=np.uint32)
        self._check(self._lib.gcre_test_expand(self._h, _ptr(path_idx), _ptr(location), len(location), _ptr(signs), len(signs),
                                               int(path_length), int(method), int(first), int(count), _ptr(row0), _ptr(row1)))
        return row0[:count], row1[:count]

    def test_inspect(self, p0: PathSet, red: PathSet, row0, row1, zindex=None, excess=None, range_of=None,
                     over_entries: Optional[int] = None, ent_stride: Optional[int] = None, keep_rows: bool = False) -> dict:
        """Tests: the method-1 inspector (k_stats_ie2) on given row numbers, on the road GCRE_STATS_IE_COUNTS selects.  Path i
        joins row row0[i] of p0 to row row1[i] of red, or to row zindex[row1[i]] of it; excess[ranges][vlen] and
        range_of[rows of p0] make it a hinted join.  Returns tot, cases, ctrls, rowz, linfo, key, lists (per path: the
        entries without padding, as the inspector ordered them), padding (per path: the padding entries), flags and, with
        keep_rows, rows."""
        row0 = np.ascontiguousarray(row0, dtype=np.uint32)
        row1 = np.ascontiguousarray(row1, dtype=np.uint32)
        n = len(row0)
        assert len(row1) == n
        if zindex is not None:
            zindex = np.ascontiguousarray(zindex, dtype=np.int32)
        if excess is not None:
            excess = np.ascontiguousarray(excess, dtype=np.uint64).reshape(-1, self.vlen)
            range_of = np.ascontiguousarray(range_of, dtype=np.int32)
            assert len(range_of) == p0.size
        stride = int(ent_stride) if ent_stride is not None else 64 * self.vlen + 8
        over = int(over_entries) if over_entries is not None else n * stride
        out = {k: np.zeros(max(n, 1), dtype=np.uint32) for k in ("tot", "cases", "ctrls", "rowz", "linfo")}
        out["key"] = np.zeros(max(n, 1), dtype=np.uint64)
        entries = np.zeros((max(n, 1), stride), dtype=np.uint32)
        rows = np.zeros((max(n, 1), self.vlen), dtype=np.uint64) if keep_rows else None
        flags = np.zeros(8, dtype=np.uint32)
        self._check(self._lib.gcre_test_inspect(
            self._h, p0._h, red._h, _ptr(row0), _ptr(row1), n, _ptr(zindex) if zindex is not None else None,
            len(zindex) if zindex is not None else 0, _ptr(excess) if excess is not None else None,
            _ptr(range_of) if excess is not None else None, len(excess) if excess is not None else 0, over,
            _ptr(out["tot"]), _ptr(out["cases"]), _ptr(out["ctrls"]), _ptr(out["rowz"]), _ptr(out["linfo"]), _ptr(out["key"]),
            _ptr(entries), stride, _ptr(rows) if keep_rows else None, _ptr(flags)))
        out = {k: v[:n] for k, v in out.items()}
        len8 = (out["linfo"] & 0x0ffffff8).astype(np.int64)
        pad = (out["linfo"] >> 28).astype(np.int64)
        out["lists"] = [entries[i, :len8[i] - pad[i]] for i in range(n)]
        out["padding"] = [entries[i, len8[i] - pad[i]:len8[i]] for i in range(n)]
        out["flags"] = flags
        if keep_rows:
            out["rows"] = rows[:n]
        return out

    def create_path_set(self, size: int) -> PathSet:
        return PathSet(self, self._lib.gcre_pathset_zeros(self._h, int(size)))

    def load(self, data) -> PathSet:
        d = np.ascontiguousarray(data, dtype=np.int32)
        ncol = d.shape[1] if d.ndim == 2 else 0
        return PathSet(self, self._lib.gcre_pathset_from_dense(self._h, _ptr(d), d.shape[0], ncol, 0))

    def from_words(self, rows) -> PathSet:
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, self.vlen)
        return PathSet(self, self._lib.gcre_pathset_from_words(self._h, _ptr(r), r.shape[0]))

    def join(self, uids, paths0: PathSet, paths1: PathSet, paths_res: Optional[PathSet] = None,
             shard: Optional[Tuple[int, int]] = None, d_null_out: int = 0,
             keep: Optional[Tuple[int, int]] = None, keep_mode: int = 1, exchange=None, exchanges: int = 0,
             tally: Optional["GeneTally"] = None, exceed: Optional["ExceedCounts"] = None,
             hits: Optional["HitList"] = None) -> JoinResult:
        """JoinExec::join (src/join_base.cpp:189-264).  ``paths_res`` receives the joined rows when given.
        ``uids`` is a UidRelSet (uploaded for this call) or a DeviceUids (already resident).  ``shard`` restricts
        scoring to a range of joined paths; ``keep`` restricts the rows written to ``paths_res`` to a range (plus
        the scored shard) -- the rows this device's shards of the later joins will read -- or, with ``keep_mode`` 2,
        only the rows that get count planes (all rows are still written).  ``exchange(k0, k1)`` is called ``exchanges``
        times during the join (gcre_join_opts.exchange): it MAX-all-reduces d_null_out[k0:k1] across the ranks in place.
        ``tally``: a GeneTally this join's scored paths are folded into (gcre_join_set_tally).  ``exceed``: an ExceedCounts
        this join's null values and observed scores are counted into (gcre_join_set_exceed).  ``hits``: a HitList this
        join's scored paths at or above its cut-off are appended to (gcre_join_set_hits)."""
        opts = gcre_join_opts(0, 0, 0, 0, None, 0, 0, 0, None, None)
        cb = None
        if exchange is not None and exchanges > 0:
            if not d_null_out:
                raise GcreError("exchange needs d_null_out")

            def _cb(_user, _d_null, k0, k1):
                try:
                    exchange(int(k0), int(k1))
                    return 0
                except Exception:      # an exception must not unwind through the C frame
                    import traceback
                    traceback.print_exc()
                    return 1
            cb = EXCHANGE_FN(_cb)      # kept alive until the join returns
            opts.exchanges = int(exchanges)
            opts.exchange = ctypes.cast(cb, ctypes.c_void_p)
        if shard is not None:
            opts.sharded, opts.shard_begin, opts.shard_end = 1, int(shard[0]), int(shard[1])
        if keep is not None:
            opts.keep_ranged, opts.keep_begin, opts.keep_end = int(keep_mode), int(keep[0]), int(keep[1])
        if d_null_out:
            opts.d_null_out = ctypes.c_void_p(int(d_null_out))
        res = gcre_result()
        res_h = paths_res._h if paths_res is not None else None
        host_uids = None if isinstance(uids, DeviceUids) else uids
        _arm_observers(self, [(o, None, host_uids) for o in (tally, exceed, hits) if o is not None])
        if isinstance(uids, DeviceUids):
            rc = self._lib.gcre_join_uids(self._h, uids._h, paths0._h, paths1._h, res_h, ctypes.byref(opts),
                                          ctypes.byref(res))
        else:
            count = np.ascontiguousarray(uids.count, dtype=np.int32)
            location = np.ascontiguousarray(uids.location, dtype=np.int64)
            signs = np.ascontiguousarray(uids.signs, dtype=np.int32)
            rc = self._lib.gcre_join(self._h, int(uids.path_length), _ptr(count), _ptr(location), len(count),
                                     _ptr(signs), len(signs), paths0._h, paths1._h, res_h, ctypes.byref(opts),
                                     ctypes.byref(res))
        self._check(rc)
        return _take_result(self._lib, res)

    def join_ahead(self, uids: Optional["DeviceUids"], paths0: Optional[PathSet] = None, paths1: Optional[PathSet] = None,
                   paths_res: Optional[PathSet] = None, shard: Optional[Tuple[int, int]] = None,
                   keep: Optional[Tuple[int, int]] = None, keep_mode: int = 1) -> None:
        """gcre_join_ahead: register a LATER join of a sequence (call it once per later join, in order; ``None`` cancels).
        The join call that follows inspects and launches every registered join in turn once its own work is queued -- the
        inspectors on a stream of their own, beside the permutation kernels of the joins before them -- and the registered
        joins, called afterwards with the same arguments, only collect their results.  Needs the inspection cache
        (``set_inspect_cache(True)``) and GCRE_AHEAD=1."""
        if uids is None:
            self._check(self._lib.gcre_join_ahead(self._h, None, None, None, None, None))
            return
        opts = gcre_join_opts(0, 0, 0, 0, None, 0, 0, 0, None, None)
        if shard is not None:
            opts.sharded, opts.shard_begin, opts.shard_end = 1, int(shard[0]), int(shard[1])
        if keep is not None:
            opts.keep_ranged, opts.keep_begin, opts.keep_end = int(keep_mode), int(keep[0]), int(keep[1])
        res_h = paths_res._h if paths_res is not None else None
        self._check(self._lib.gcre_join_ahead(self._h, uids._h, paths0._h, paths1._h, res_h, ctypes.byref(opts)))

    def profile(self) -> Dict[str, float]:
        p = gcre_profile()
        self._check(self._lib.gcre_get_profile(self._h, ctypes.byref(p)))
        return {f: getattr(p, f) for f, _ in gcre_profile._fields_}


def resolve_count_locs(trg_uids, keys, counts, locations):
    """assemble_uids' lookup (src/wrapper.cpp:106-132) through the C ABI."""
    lib = load_library()
    trg = np.ascontiguousarray(trg_uids, dtype=np.int32)
    keys = np.ascontiguousarray(keys, dtype=np.int32)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    locations = np.ascontiguousarray(locations, dtype=np.int32)
    oc = np.zeros(len(trg), dtype=np.int32)
    ol = np.zeros(len(trg), dtype=np.int64)
    rc = lib.gcre_resolve_count_locs(_ptr(trg), len(trg), _ptr(keys), _ptr(counts), _ptr(locations), len(keys),
                                     _ptr(oc), _ptr(ol))
    if rc != GCRE_OK:
        raise GcreError(f"gcre_resolve_count_locs failed: {rc}")
    return oc, ol


def build_levels(n_genes: int, src, trg, sign):
    """Native build of the per-level join tables (R/ProcessPaths.R:206-256) -> geneticscre_amd.uids.LevelTables."""
    from .uids import LevelTables, UidRelSet
    lib = load_library()
    s = np.ascontiguousarray(src, dtype=np.int32)
    t = np.ascontiguousarray(trg, dtype=np.int32)
    g = np.ascontiguousarray(sign, dtype=np.int32)
    out = gcre_levels()
    rc = lib.gcre_build_levels(int(n_genes), _ptr(s), _ptr(t), _ptr(g), len(s), ctypes.byref(out))
    if rc == GCRE_ERR_RANGE:
        raise IndexError("relation endpoint outside 0..n_genes-1")
    if rc != GCRE_OK:
        raise ValueError("relations must be sorted by (src, trg), unique, without self loops")

    def arr(ptr, n, dt):
        return np.ctypeslib.as_array(ptr, (n,)).astype(dt, copy=True) if n > 0 else np.zeros(0, dt)

    names = ["1a", "1b", "2", "3", "4", "5"]
    uids, n_paths = {}, {}
    for i, name in enumerate(names):
        lt = out.level[i]
        uids[name] = UidRelSet(lt.path_length, arr(lt.src, lt.n_uids, np.int32), arr(lt.trg, lt.n_uids, np.int32),
                               arr(lt.count, lt.n_uids, np.int32), arr(lt.location, lt.n_uids, np.int64),
                               arr(lt.signs, lt.n_signs, np.int32))
        n_paths[name] = int(lt.total_paths)
    data_inds = {name: arr(out.data_inds[i], out.n_data_inds[i], np.int32) for i, name in enumerate(names[:4])}
    n3 = out.n_rels3
    rels3 = {"srcuid": arr(out.r3_src, n3, np.int32), "trguid": arr(out.r3_trg, n3, np.int32),
             "sign": arr(out.r3_sign, n3, np.int32), "trguid2": arr(out.r3_trg2, n3, np.int32),
             "sign2": arr(out.r3_sign2, n3, np.int32)}
    lib.gcre_levels_free(ctypes.byref(out))
    return LevelTables(uids, data_inds, rels3, n_paths)


def values_table(n_cases: int, n_ctrls: int) -> np.ndarray:
    """Native getValuesTable (R/Utils.R:137-159)."""
    out = np.zeros((n_cases + 1, n_ctrls + 1), dtype=np.float64)
    rc = load_library().gcre_values_table(int(n_cases), int(n_ctrls), _ptr(out))
    if rc != GCRE_OK:
        raise ValueError("bad table dimensions")
    return out


def _weighted_args(odds, strata, n: int):
    """odds as float64 [n] and ``strata`` mapped to ids 0 .. S-1 in ascending order (None: one stratum): (odds, ids or None,
    S, the distinct strata)."""
    w = np.ascontiguousarray(np.asarray(odds, dtype=np.float64).reshape(-1))
    if len(w) != n:
        raise ValueError(f"odds: one value per patient ({n}), not {len(w)}")
    if strata is None:
        return w, None, 1, np.zeros(1, np.int64)
    ids, inv = np.unique(np.asarray(strata).reshape(-1), return_inverse=True)
    if len(inv) != n:
        raise ValueError(f"strata: one id per patient ({n}), not {len(inv)}")
    return w, np.ascontiguousarray(inv, dtype=np.int32), len(ids), ids


def weighted_thresholds(odds, n_cases: int, n_ctrls: int, strata=None):
    """The 32-bit thresholds of ``JoinExec.generate_weighted_permutations`` (gcre_weighted_thresholds) and
    the expected attempts per stratum, sqrt(2 pi V): ``(uint32 [n], float64 [S])``.  Host only, no GPU.  The thresholds are
    the definition of the law that is sampled -- conditional Bernoulli with p = thr / 2^32 -- and what
    ``report.weighted_masks`` takes.  ``strata`` as ``generate_weighted_permutations`` reads them.  Refusals raise GcreError
    with the library's message."""
    n = int(n_cases) + int(n_ctrls)
    w, st, S, _ = _weighted_args(odds, strata, n)
    lib = _weighted_lib()
    thr = np.zeros(max(n, 1), dtype=np.uint32)
    exp = np.zeros(max(S, 1), dtype=np.float64)
    rc = lib.gcre_weighted_thresholds(n, int(n_cases), _ptr(w) if n else _ptr(np.zeros(1)), _ptr(st), S if st is not None else 0,
                                      _ptr(thr), _ptr(exp))
    if rc != GCRE_OK:
        raise GcreError(lib.gcre_last_error(None).decode())
    return thr[:n], exp[:S]


def rccl_selftest(device: int = 0) -> None:
    """One-rank RCCL communicator + MAX all-reduce through the library's own (dlopen'ed) RCCL binding; raises on failure."""
    buf = ctypes.create_string_buffer(512)
    if load_library().gcre_rccl_selftest(int(device), buf, 512) != GCRE_OK:
        raise GcreError("gcre_rccl_selftest: " + buf.value.decode())


def rccl_collectives() -> int:
    return int(load_library().gcre_rccl_collectives())


def values_table_exact_order(n_cases: int, n_ctrls: int) -> bool:
    """True: ``values_table`` sums every cell in R's index order at this size; False: the sorted prefix sum of very large
    cohorts (the last bit of a cell in a hundred can differ).  Recorded with fixtures and bench lines."""
    return bool(load_library().gcre_values_table_exact_order(int(n_cases), int(n_ctrls)))


def _pp_input(problem, keep):
    """gcre_pp_input for a synth.Problem; numpy buffers are appended to ``keep`` (they must outlive the call)."""
    def arr(a, dt):
        b = np.ascontiguousarray(a, dtype=dt)
        keep.append(b)
        return b

    inp = gcre_pp_input()
    for i, name in enumerate(["1a", "1b", "2", "3", "4", "5"]):
        u = problem.levels.uids[name]
        c, l, s = arr(u.count, np.int32), arr(u.location, np.int64), arr(u.signs, np.int32)
        inp.level[i] = gcre_level(_ptr(c), _ptr(l), len(c), _ptr(s), len(s))
    for i, name in enumerate(["1a", "1b", "2", "3"]):
        d = arr(problem.levels.data_inds[name], np.int32)
        inp.data_inds[i], inp.n_data_inds[i] = _ptr(d), len(d)
    d1, d2 = arr(problem.data1, np.int32), arr(problem.data2, np.int32)
    inp.data1, inp.data1_rows, inp.data2, inp.data2_rows, inp.data_col_major = _ptr(d1), d1.shape[0], _ptr(d2), d2.shape[0], 0
    vt = arr(problem.value_table, np.float64)
    inp.value_table, inp.vt_rows, inp.vt_cols, inp.vt_col_major = _ptr(vt), vt.shape[0], vt.shape[1], 0
    pc = arr(problem.perm_cases, np.int32)
    inp.perm_cases = _ptr(pc) if pc.size else None
    inp.perm_rows, inp.perm_col_major = (pc.shape[0] if pc.ndim == 2 else 0), 0
    inp.path_length = int(problem.path_length)
    return inp


def process_paths_devices(problem, devices=None, tallies=None) -> Dict[str, object]:
    """ProcessPaths on several GPUs of the node from this one process (gcre_process_paths_devices): one context and host
    thread per entry of ``devices`` (None: every visible device; an id may repeat), joined paths sharded, maxima and top-k
    tables merged.  Bit-identical to ``process_paths`` for any device list.  It takes no gene tallies (merging them across
    devices is out of scope: shard the joins yourself, ``JoinExec.join(shard=, tally=)``): ``tallies`` raises GcreError."""
    if tallies:
        raise GcreError("process_paths_devices takes no gene tallies: merging tallies across devices is not supported")
    lib = load_library()
    lib.gcre_process_paths_devices.restype = ctypes.c_int
    lib.gcre_process_paths_devices.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_char_p, ctypes.c_size_t]
    keep = []
    inp = _pp_input(problem, keep)
    outs = (gcre_result * 5)()
    err = ctypes.create_string_buffer(512)
    dev = None if devices is None else np.ascontiguousarray(devices, dtype=np.int32)
    rc = lib.gcre_process_paths_devices(1 if problem.method == "method1" else 2, int(problem.n_cases), int(problem.n_ctrls),
                                        int(problem.iterations), int(problem.top_k), _ptr(dev) if dev is not None else None,
                                        0 if dev is None else len(dev), ctypes.byref(inp), outs, err, len(err))
    if rc != GCRE_OK:
        msg = err.value.decode() or f"gcre error {rc}"
        if rc == GCRE_ERR_RANGE or "out of range" in msg:
            raise IndexError(msg)
        if rc == GCRE_ERR_ASSERT or "assertion" in msg:
            raise ValueError(msg)
        raise GcreError(msg)
    return {f"lst{i + 1}": (None if outs[i].n < 0 else _take_result(lib, outs[i])) for i in range(5)}


def process_paths(problem, device: int = 0, exec_: Optional[JoinExec] = None, tallies=None, exceeds=None,
                  hits=None) -> Dict[str, object]:
    """ProcessPaths (src/wrapper.cpp:177-281) in one native call.  Returns {"lst1": JoinResult | None, ...}.

    ``problem`` carries the 39 arguments as arrays (geneticscre_amd.synth.Problem).  ``tallies``: level name ("1b", "2",
    .., "5"; "1a" too) -> GeneTally of ``exec_``: that level's join folds its scored paths into it.  ``exceeds``: level name
    -> ExceedCounts of ``exec_``: that level's join counts into it (all permutations, the observed scores once).
    ``hits``: level name -> HitList of ``exec_``: that level's join appends its scored paths at or above the list's cut-off
    (once, however many permutation windows the call walks).
    """
    for given, what in ((tallies, "gene tallies"), (exceeds, "exceedance counts"), (hits, "hit lists")):
        if given and exec_ is None:
            raise GcreError(f"process_paths: {what} live on a context; pass the JoinExec they were made on as exec_")
    ex = exec_ or JoinExec(problem.method, problem.n_cases, problem.n_ctrls, problem.iterations, device)
    ex.top_k = problem.top_k
    lib = ex._lib
    keep = []   # keep numpy buffers alive across the call
    inp = _pp_input(problem, keep)
    outs = (gcre_result * 5)()
    observers = [(name, o) for given in (tallies, exceeds, hits) for name, o in (given or {}).items()]
    for name, _ in observers:
        if name not in LEVEL_INDEX:
            raise GcreError(f"process_paths: no level {name!r} (levels are {', '.join(LEVEL_INDEX)})")
    _arm_observers(ex, [(o, LEVEL_INDEX[name], problem.levels.uids[name]) for name, o in observers])
    rc = lib.gcre_process_paths(ex._h, ctypes.byref(inp), outs)
    ex._check(rc)
    result: Dict[str, object] = {}
    for i in range(5):
        result[f"lst{i + 1}"] = None if outs[i].n < 0 else _take_result(lib, outs[i])
    result["profile"] = ex.profile()
    if exec_ is None:
        ex.close()
    return result


class ResidentPlan:
    """The ProcessPaths join sequence (src/wrapper.cpp:216-276) with every input already in HBM.

    ``prepare`` uploads data, table, masks and the per-level join indices once; ``run`` then performs the
    joins of one pass: levels 1a, 1b, 2 .. path_length.  With ``world > 1`` each rank scores a contiguous
    slice of every level's joined paths (kept rows are materialised in full on every rank) and the caller
    merges null maxima (MAX) and top-k tables across ranks -- see bench.py.
    """

    LEVELS = ["1a", "1b", "2", "3", "4", "5"]

    def __init__(self, problem, device: int = 0, packed_masks: Optional[np.ndarray] = None,
                 mask_seed: Optional[int] = None):
        self.problem = problem
        self._needed: Dict[tuple, Optional[Tuple[int, int]]] = {}
        self._first: Dict[str, np.ndarray] = {}
        self._window: Optional[int] = None
        self._cache_on = False
        ex = self.ex = JoinExec(problem.method, problem.n_cases, problem.n_ctrls, problem.iterations, device)
        ex.top_k = problem.top_k
        ex.set_value_table(problem.value_table)
        if mask_seed is not None:
            ex.generate_permutations(mask_seed)      # drawn on the device: every rank with the same seed gets the same masks
        elif packed_masks is not None:
            ex.set_permuted_masks(packed_masks)
        else:
            ex.set_permuted_cases(problem.perm_cases)
        lv, L = problem.levels, problem.path_length
        self.names = ["1a", "1b"] + [str(l) for l in range(2, L + 1)]
        self.uids = {k: DeviceUids(ex, lv.uids[k]) for k in self.names}
        parsed1 = ex.load(problem.data1)
        parsed2 = ex.load(problem.data2)
        self.inputs = {"1a": parsed1.select(lv.data_inds["1a"]), "1b": parsed2.select(lv.data_inds["1b"])}
        self.zeros = {"1a": ex.create_path_set(len(lv.data_inds["1a"])), "1b": ex.create_path_set(len(lv.data_inds["1b"]))}
        if L >= 2:
            self.inputs["2"] = parsed1.select(lv.data_inds["3"])   # wrapper.cpp:207 reads data_idx2 from r_data_inds3
        if L >= 3:
            self.inputs["3"] = parsed1.select(lv.data_inds["3"])
        self.parsed = (parsed1, parsed2)
        self.kept = {"1": ex.create_path_set(self.uids["1a"].total_paths)}
        if L >= 2:
            self.kept["2"] = ex.create_path_set(self.uids["2"].total_paths)
        if L >= 3:
            self.kept["3"] = ex.create_path_set(self.uids["3"].total_paths)
        # what every join really adds to paths0 (gcre_uids_set_reduced; the same hints gcre_process_paths attaches)
        self.uids["1a"].set_reduced(parsed1, lv.data_inds["1a"])
        self.uids["1b"].set_reduced(parsed2, lv.data_inds["1b"])
        signed = problem.method == "method2"
        rel_neg = (np.asarray(lv.uids["2"].signs) != 1) if signed else np.zeros(len(lv.uids["2"].signs), bool)
        for name in ("2", "3"):
            if name in self.uids:
                self.uids[name].set_reduced(parsed1, lv.data_inds["3"])
        self._reduced_args: Dict[str, tuple] = {}
        self._pivot: Dict[tuple, DeviceUids] = {}
        # off by default: measured -- the level-4 shard gains 3 %, keeping all of level 2's planes costs more
        self.pivot_shards = os.environ.get("GCRE_PIVOT_SHARDS", "0") == "1"
        # Inspect- and launch-ahead (gcre_join_ahead): the later joins of a pass are inspected and launched while the first one's
        # results are collected.  Worth 5-8 % on BASELINE configs[1] (per-join host gaps), 0.5 % on configs[2], nothing or less on
        # configs[3] (long joins: inspector and permutation kernel each fill the GPU); it keeps every chunk's inspection for the
        # length of the pass (~130 B per joined path).  Default: plans of up to 64 M joined paths and 10^12 scores per pass.
        # GCRE_AHEAD=1 / 0: always / never (the library honours the same variable).
        env_ahead = os.environ.get("GCRE_AHEAD", "")
        total_paths = sum(int(self.uids[k].total_paths) for k in self.names)
        self.ahead = env_ahead == "1" or (env_ahead == "" and total_paths <= 64_000_000 and
                                          total_paths * max(int(problem.iterations), 1) <= 10 ** 12)
        if "4" in self.uids:    # level 2 put the added gene into the (-) half of paths2[loc] when the relation is negative
            self._reduced_args["4"] = (parsed1, np.asarray(lv.data_inds["3"], np.int64) | (rel_neg.astype(np.int64) << 31))
            self.uids["4"].set_reduced(*self._reduced_args["4"])
        if "5" in self.uids:    # paths3[loc] = (c, d, e): the join adds paths2[(d, e)], swapped when (c, d) is negative
            u3 = lv.uids["3"]
            cnt = np.maximum(np.asarray(u3.count, dtype=np.int64), 0)
            start = np.repeat(np.asarray(u3.location, dtype=np.int64), cnt)
            within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            first_neg = np.repeat((np.asarray(u3.signs)[:len(cnt)] != 1) if signed else np.zeros(len(cnt), bool), cnt)
            self._reduced_args["5"] = (self.kept["2"], (start + within) | (first_neg.astype(np.int64) << 31))
            self.uids["5"].set_reduced(*self._reduced_args["5"])

    def operands(self, name: str):
        """(paths0, paths1, paths_res) of one level, as in wrapper.cpp:227-276."""
        k = self.kept
        return {
            "1a": (self.zeros["1a"], self.inputs["1a"], k["1"]),
            "1b": (self.zeros["1b"], self.inputs["1b"], None),
            "2": (k["1"], self.inputs.get("2"), k.get("2")),
            "3": (k.get("2"), self.inputs.get("3"), k.get("3")),
            "4": (k.get("3"), k.get("2"), None),
            "5": (k.get("3"), k.get("3"), None),
        }[name]

    def _uids_of(self, name: str, b: int, e: int) -> Tuple[int, int]:
        """Rows of paths0 (uids) that own the joined paths [b, e) of level ``name``."""
        if e <= b:
            return (0, 0)
        if name not in self._first:
            u = self.problem.levels.uids[name]
            self._first[name] = np.concatenate([[0], np.cumsum(np.maximum(np.asarray(u.count, dtype=np.int64), 0))])
        first = self._first[name]
        return (int(np.searchsorted(first, b, side="right")) - 1, int(np.searchsorted(first, e - 1, side="right")))

    def pivot_sharded(self, name: str, world: int) -> bool:
        """``GCRE_PIVOT_SHARDS=1``: levels that keep nothing (4 and 5) are sharded by PIVOT GROUP when there are several ranks:
        all uids that join the same paths1 rows (same ``location``: the 3-paths ending in one gene) go to one rank, so the
        planes of those rows are fetched on one GPU only.  The other levels keep an ordinal range (their kept rows must be
        ranges).  Exact like any sharding; not the default because it does not pay."""
        return self.pivot_shards and world > 1 and name in ("4", "5") and name in self.uids

    def pivot_uids(self, name: str, rank: int, world: int) -> DeviceUids:
        """The join index of level ``name`` with ``count = 0`` outside this rank's pivot groups (the reference skips such
        uids, src/join_base.cpp:236): a shard by uid subset that needs nothing below the C ABI.  Groups are cut at equal
        cumulative path counts; a rank's joined paths stay in the level's order, so ties are cut as on one GPU."""
        key = (name, rank, world)
        if key not in self._pivot:
            u = self.problem.levels.uids[name]
            cnt = np.maximum(np.asarray(u.count, dtype=np.int64), 0)
            loc = np.asarray(u.location, dtype=np.int64)
            groups, inv = np.unique(np.where(cnt > 0, loc, -1), return_inverse=True)
            weight = np.bincount(inv, weights=cnt.astype(np.float64), minlength=len(groups))
            cum = np.concatenate([[0.0], np.cumsum(weight)])
            total = cum[-1]
            g_lo = int(np.searchsorted(cum, total * rank / world, side="left"))
            g_hi = int(np.searchsorted(cum, total * (rank + 1) / world, side="left")) if rank + 1 < world else len(groups)
            mine = (inv >= g_lo) & (inv < g_hi)
            from .uids import UidRelSet
            sub = UidRelSet(u.path_length, u.src, u.trg, np.where(mine, cnt, 0).astype(np.int32), u.location, u.signs)
            du = DeviceUids(self.ex, sub)
            du.set_reduced(*self._reduced_args[name])
            self._pivot[key] = du
        return self._pivot[key]

    def needed_rows(self, name: str, rank: int, world: int) -> Optional[Tuple[int, int]]:
        """What THIS rank needs of the set level ``name`` keeps, as a range of its rows (None: everything).
        Level 3's rows are only read as paths0 of the level-4 shard: the others are not produced at all
        (gcre_join_opts.keep_ranged = 1).  Levels 1 and 2 are also read as paths1 / reduced operands, so all their
        rows are written, but count planes are only needed for the rows this rank's work on the next level reads
        as paths0 (keep_ranged = 2, see ``keep_mode``).  With level 5 in the run every rank needs all of levels 2
        and 3 (level 5 joins level 3 with itself through level 2's planes)."""
        if world == 1 or "5" in self.uids or name not in ("1a", "2", "3"):
            return None
        if self.pivot_sharded("4", world) and name in ("2", "3"):
            # a rank's pivot groups read level-3 rows from everywhere, and their recipes start at arbitrary rows of level 2:
            # every rank keeps all of both (level 3 as recipes, level 2 with its planes)
            return None
        key = (name, rank, world)
        if key in self._needed:
            return self._needed[key]
        nxt = {"1a": "2", "2": "3", "3": "4"}[name]
        if nxt not in self.uids:
            self._needed[key] = None if name != "3" else (0, 0)
            return self._needed[key]
        # joined paths of the next level this rank works on: its shard, and whatever the level after needs of it
        b, e = self.shard(nxt, rank, world)
        more = self.needed_rows(nxt, rank, world) if nxt in ("2", "3") else (0, 0)
        if more is None:
            more = (0, self.uids[nxt].total_paths)
        if more[1] > more[0]:
            b, e = (min(b, more[0]), max(e, more[1])) if e > b else more
        self._needed[key] = self._uids_of(nxt, b, e)
        return self._needed[key]

    def keep_mode(self, name: str) -> int:
        return 1 if name == "3" else 2

    def shard(self, name: str, rank: int, world: int) -> Tuple[int, int]:
        total = self.uids[name].total_paths
        return (total * rank) // world, (total * (rank + 1)) // world

    def exchange_count(self, name: str, world: int) -> int:
        """How often a rank shares its running maxima with the others during the join of level ``name`` (the same on
        every rank: it only depends on the level's size): one exchange per doubling of the work beyond
        GCRE_EXCHANGE_UNIT joined-path x 2048-permutation tiles per rank (default 2 M, about 0.3 ms of the pruned kernel),
        at most 8.  Small joins do not exchange at all."""
        if world <= 1 or self.problem.iterations <= 0:
            return 0
        unit = float(os.environ.get("GCRE_EXCHANGE_UNIT", 2e6))
        window = self._window if self._window else self.problem.iterations
        tiles = -(-min(window, self.problem.iterations) // 2048)
        work = self.uids[name].total_paths / world * tiles
        if unit <= 0 or work < 2 * unit:
            return 0
        most = min(max(float(os.environ.get("GCRE_EXCHANGE_MAX", 8)), 1.0), 32.0)
        return int(min(most, np.floor(np.log2(work / unit))))

    def run(self, rank: int = 0, world: int = 1, d_null_out: int = 0, on_level=None,
            keep_inspections: bool = False, exchange=None, tallies=None, exceeds=None, hits=None) -> Dict[str, JoinResult]:
        """One pass over all levels.  Large permutation counts run in windows of whole 2048-permutation tiles (the count
        planes of the kept sets are per tile and have to fit in device memory): all levels for window 0, then all levels
        for window 1, ...  ``on_level(name, result, shard, window)`` sees every (level, window) result -- its null
        maxima are those of the window's permutations; ``d_null_out`` (device pointer to K floats) receives them at
        the window's offset.  The returned results carry the first window's top-k (they do not depend on the window)
        and the concatenated null maxima.

        A pass of several windows runs every join's inspector (expansion, observed scores, top-k, kept rows, lists) for the
        first window only: the library's inspection cache is on for the pass, and forgotten when the next pass starts --
        unless ``keep_inspections``: then a later pass over the same resident inputs starts every join at its null
        kernel (steady state of a service that re-scores the same network against new permutations).

        ``exchange(name, k0, k1)`` (multi-GPU): MAX-all-reduce ``d_null_out[k0:k1]`` across the ranks in place; called
        ``exchange_count(name, world)`` times during a level's join so that every rank prunes against the whole level's
        running maxima, not only its shard's (gcre_join_opts.exchange).  The null maxima a rank then returns include what
        it learned from the others; their MAX over the ranks is unchanged.

        ``tallies``: level name -> GeneTally of ``self.ex``; that level's join folds its scored paths into it (every window
        folds the same observed scores again, which changes nothing).  One rank only.

        ``exceeds``: level name -> ExceedCounts of ``self.ex``; that level's join counts into it.  Every (level, window) is a
        join call of its own: the null values of the windows add up to all permutations, and the observed scores are
        counted once per window (``Exceedances.paths`` says how often: it grows by the level's joined paths each time).

        ``hits``: level name -> HitList of ``self.ex``; that level's join appends its scored paths at or above the list's
        cut-off -- in the first window only (the observed scores do not depend on the window): a pass lists a level once.
        One rank only."""
        if tallies and world > 1:
            raise GcreError("ResidentPlan.run: gene tallies need world == 1 (merging tallies across ranks is not supported)")
        if exceeds and world > 1:
            raise GcreError("ResidentPlan.run: exceedance counts need world == 1 (add the counts of sharded joins yourself)")
        if hits and world > 1:
            raise GcreError("ResidentPlan.run: hit lists need world == 1 (merging lists across ranks is not supported)")
        K = self.problem.iterations
        if self._window is None:
            self._window = self.planned_window()
        n_windows = len(range(0, max(K, 1), self._window))
        # inspect-ahead (gcre_join_ahead): every join's inspector runs beside the permutation kernel of the join before it,
        # into the inspection cache -- which therefore is on for the pass and, unless the caller keeps inspections, forgotten
        # when the pass ends (nothing of one pass serves the next)
        ahead = self.ahead and K > 0
        if keep_inspections or n_windows > 1 or ahead:
            self.ex.set_inspect_cache(True)
            if not keep_inspections:
                self.ex.drop_inspections()
        elif self._cache_on:
            self.ex.set_inspect_cache(False)
        self._cache_on = keep_inspections or n_windows > 1 or ahead
        out: Dict[str, JoinResult] = {}
        nulls: Dict[str, list] = {}
        prof: Dict[str, float] = {}
        for k0 in range(0, max(K, 1), self._window):
            k1 = min(K, k0 + self._window)
            if K > 0:
                self.ex.set_perm_window(k0, k1)
            def spec(name):
                p0, p1, res = self.operands(name)
                b, e = self.shard(name, rank, world)
                by_pivot = self.pivot_sharded(name, world)
                return (self.pivot_uids(name, rank, world) if by_pivot else self.uids[name], p0, p1, res,
                        (b, e) if (world > 1 and not by_pivot) else None, self.needed_rows(name, rank, world), self.keep_mode(name))

            for pos, name in enumerate(self.names):
                p0, p1, res = self.operands(name)
                b, e = self.shard(name, rank, world)
                n_ex = self.exchange_count(name, world) if (exchange is not None and d_null_out) else 0
                by_pivot = self.pivot_sharded(name, world)
                if ahead and pos == 0:
                    # the chain: every later level of this window, in order, up to the first one that exchanges thresholds
                    # with other ranks inside its join (that one, and what reads its rows, runs in its own call)
                    self.ex.join_ahead(None)
                    for later in self.names[1:]:
                        if exchange is not None and d_null_out and self.exchange_count(later, world) > 0:
                            break
                        u_n, p0_n, p1_n, res_n, shard_n, keep_n, mode_n = spec(later)
                        self.ex.join_ahead(u_n, p0_n, p1_n, res_n, shard=shard_n, keep=keep_n, keep_mode=mode_n)
                r = self.ex.join(self.pivot_uids(name, rank, world) if by_pivot else self.uids[name], p0, p1, res,
                                 shard=(b, e) if (world > 1 and not by_pivot) else None,
                                 d_null_out=(d_null_out + 4 * k0) if d_null_out else 0,
                                 keep=self.needed_rows(name, rank, world), keep_mode=self.keep_mode(name),
                                 exchange=(lambda a, b_, name=name: exchange(name, a, b_)) if n_ex else None, exchanges=n_ex,
                                 tally=(tallies or {}).get(name), exceed=(exceeds or {}).get(name),
                                 hits=(hits or {}).get(name) if k0 == 0 else None)
                for k, v in self.ex.profile().items():
                    prof[k] = prof.get(k, 0) + v
                if on_level is not None:
                    r = on_level(name, r, (b, e), (k0, k1))
                nulls.setdefault(name, []).append(r.null)
                if name not in out:
                    out[name] = r
        if K > 0:
            self.ex.set_perm_window(0, K)
        if self._cache_on and not keep_inspections:
            self.ex.drop_inspections()     # this pass's inspections end with it (the buffers stay for the next pass)
        for name, r in out.items():
            r.null = np.concatenate(nulls[name]) if len(nulls[name]) > 1 else nulls[name][0]
        self.last_profile = prof
        return out

    def planned_window(self) -> int:
        """Permutations per window THIS device would choose (from its free memory, gcre_plan_perm_window).  Ranks of a
        multi-GPU job must agree on one value before the first pass -- every (level, window) is one round of collectives --
        see ``geneticscre_amd.dist.agree_window`` and ``set_window``."""
        if self.problem.iterations <= 0:
            return 1
        sets = [ps.size for ps in self.kept.values()] + [ps.size for ps in self.parsed]
        return self.ex.plan_perm_window(sets)

    def set_window(self, perms: int) -> None:
        """Fix the permutation window (a multiple of the 2048-permutation tile unless it covers everything)."""
        K = max(self.problem.iterations, 1)
        perms = int(perms)
        self._window = K if perms >= K else max(2048, perms // 2048 * 2048)

    def windows(self):
        """[(k0, k1), ...] the passes of ``run`` will walk."""
        K = self.problem.iterations
        w = self._window if self._window is not None else self.planned_window()
        return [(k0, min(K, k0 + w)) for k0 in range(0, max(K, 1), w)]

    def total_scores(self) -> int:
        return self.problem.iterations * sum(self.uids[k].total_paths for k in self.names)

    def close(self):
        self.ex.close()
