"""Checks of the dense-matrix input roads of the library (gcre_pathset_from_dense, gcre_set_perm_cases) in both storage
layouts, against plain numpy.  The functions here are run twice: by tests/test_gpu_inputs.py in the pytest process (the host
packs the bits: pack_bits_host) and by tests/device_pack_child.py in a process started with GCRE_DEVICE_PACK=1 (the ints go
up and k_pack_dense / k_masks_from_ints pack them) -- that knob is read once per process."""
from __future__ import annotations

import ctypes

import numpy as np

import oracle
from geneticscre_amd import api
from geneticscre_amd.synth import make_problem
from helpers import assert_same_result, small_table

INT32_MIN = -2 ** 31                                   # NA_integer_
GENOTYPES = np.array([0, 0, 0, 1, 2, -1, INT32_MIN], dtype=np.int32)   # "data != 0" is a carrier
LABELS = np.array([0, 1, 1, 2, -1], dtype=np.int32)                    # "label != 1" is flipped
DENSE_N = (2, 63, 64, 65, 128, 129, 2049)              # below, at and past a word; one bit past a 2048-bit chunk
DENSE_ROWS = (1, 5, 300)
LABEL_K = (1, 33, 2049)
LABEL_N = (65, 129)


def label_rows(K: int):
    """every row reused, cyclic reuse, exact fit, truncation"""
    return sorted({1, K // 2 + 1, K, K + 7})


# ---- the references: plain numpy ----------------------------------------------------------------------------------------
def pack_bits(bits: np.ndarray, W: int) -> np.ndarray:
    """bool [rows][n] -> uint64 [rows][W], bit c of word c // 64 = column c"""
    padded = np.zeros((bits.shape[0], W * 64), dtype=bool)
    padded[:, :bits.shape[1]] = bits
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(bits.shape[0], W)


def expected_rows(data: np.ndarray, W: int, method: int) -> np.ndarray:
    """PathSet::load: the carriers in the (+) half, the (-) half of the signed method zero"""
    rows = pack_bits(data != 0, W)
    return rows if method == 1 else np.hstack([rows, np.zeros_like(rows)])


def expected_masks(labels: np.ndarray, n_cases: int, K: int, W: int) -> np.ndarray:
    """setPermutedCases: mask = (q < n_cases) XOR (label != 1); row r of K comes from input row r % min(rows_in, K)"""
    used = min(labels.shape[0], K)
    is_case = np.arange(labels.shape[1]) < n_cases
    packed = pack_bits(is_case[None, :] ^ (labels[:used] != 1), W)
    return packed[np.arange(K) % used]


# ---- the calls, through ctypes, in either layout ---------------------------------------------------------------------
def storage(m: np.ndarray, col_major: int) -> np.ndarray:
    """The same logical matrix as C-ordered (row-major) or F-ordered (column-major: what R holds) storage."""
    m = np.asarray(m, dtype=np.int32)
    return np.ascontiguousarray(m.T if col_major else m).reshape(-1)


def from_dense(ex, m: np.ndarray, col_major: int, ncol=None):
    s = storage(m, col_major)
    return ex._lib.gcre_pathset_from_dense(ex._h, s.ctypes.data_as(ctypes.c_void_p), m.shape[0],
                                           m.shape[1] if ncol is None else ncol, col_major)


def set_labels(ex, m: np.ndarray, col_major: int) -> None:
    s = storage(m, col_major)
    ex._check(ex._lib.gcre_set_perm_cases(ex._h, s.ctypes.data_as(ctypes.c_void_p), m.shape[0], m.shape[1], col_major))


def all_masks(ex) -> np.ndarray:
    return np.stack([ex.perm_mask(r) for r in range(ex.iters)]) if ex.iters else np.zeros((0, ex.width_ul), np.uint64)


def draw(values: np.ndarray, shape, seed) -> np.ndarray:
    return values[np.random.default_rng(seed).integers(0, len(values), size=shape)]


# ---- the checks ---------------------------------------------------------------------------------------------------------
def check_dense_rows(method: int, n: int) -> int:
    """Every row count of DENSE_ROWS in both layouts: all words equal numpy's, the (-) half zero, select with repeats; one
    column too many is refused.  Returns the number of path sets compared."""
    n_cases = max(1, n // 2)
    ex = api.JoinExec(method, n_cases, n - n_cases, 0)
    ox = oracle.OracleJoinExec(method, n_cases, n - n_cases, 0)
    W = ex.width_ul
    assert W == (n + 63) // 64 and ex.vlen == W * method
    done = 0
    for nrow in DENSE_ROWS:
        data = draw(GENOTYPES, (nrow, n), [method, n, nrow])
        data[0, n - 1] = INT32_MIN                       # the last patient of the first row: NA counts as a carrier
        want = expected_rows(data, W, method)
        np.testing.assert_array_equal(ox.load(data), want)          # the oracle agrees with numpy on the row-major form
        idx = np.random.default_rng(nrow).integers(0, nrow, size=2 * nrow + 3).astype(np.int32)
        for col_major in (0, 1):
            ps = api.PathSet(ex, from_dense(ex, data, col_major))
            got = ps.to_numpy()
            np.testing.assert_array_equal(got, want, err_msg=f"n={n} nrow={nrow} col_major={col_major}")
            if method == 2:
                assert not got[:, W:].any()
            np.testing.assert_array_equal(ps.select(idx).to_numpy(), want[idx])
            ps.free()
            done += 1
    # check_index(data[r].size(), width_ul * 64), gcre_paths.h:63: GCRE_ERR_RANGE, no path set
    wide = np.ones((3, 64 * W + 1), dtype=np.int32)
    for col_major in (0, 1):
        assert not from_dense(ex, wide, col_major)
        assert "more data columns than mask bits" in ex._lib.gcre_last_error(ex._h).decode()
        with np.testing.assert_raises(IndexError):
            ox.load(wide)
    ex.close()
    return done


def check_labels(K: int, n: int) -> int:
    """Every input row count of label_rows(K) in both layouts: perm_mask(r) equals numpy's for every r, words past n zero."""
    n_cases = n // 2 - 3
    ex = api.JoinExec(1, n_cases, n - n_cases, K)
    ox = oracle.OracleJoinExec(1, n_cases, n - n_cases, K)
    W = ex.width_ul
    tail = np.uint64((1 << (n - 64 * (W - 1))) - 1)
    done = 0
    for rows_in in label_rows(K):
        labels = draw(LABELS, (rows_in, n), [K, n, rows_in])
        want = expected_masks(labels, n_cases, K, W)
        assert not (want[:, W - 1] & ~tail).any()
        ox.set_permuted_cases(labels)
        np.testing.assert_array_equal(np.stack([ox.perm_mask(r) for r in range(K)]), want)
        for col_major in (0, 1):
            ex.set_permuted_masks(np.zeros((1, W), np.uint64))      # so that a call that writes nothing cannot pass
            set_labels(ex, labels, col_major)
            got = all_masks(ex)
            np.testing.assert_array_equal(got, want, err_msg=f"K={K} n={n} rows_in={rows_in} col_major={col_major}")
            assert not (got[:, W - 1] & ~tail).any()
            done += 1
    ex.close()
    return done


def check_join_behind_column_major_inputs(method: str) -> None:
    """One join sequence on data and labels that went in column-major: levels 2 and 3 equal the oracle's."""
    p = make_problem(35, 80, 70, 61, 130, 3, method=method, top_k=6, seed=21, table=small_table(70, 61, 5))
    want = oracle.process_paths(p, order="canonical")
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    ex.top_k = p.top_k
    ex.set_value_table(p.value_table)
    set_labels(ex, p.perm_cases, 1)
    d = api.PathSet(ex, from_dense(ex, p.data1, 1))
    lv = p.levels
    k1 = ex.create_path_set(lv.n_paths["1a"])
    ex.join(lv.uids["1a"], ex.create_path_set(len(lv.data_inds["1a"])), d.select(lv.data_inds["1a"]), k1)
    k2 = ex.create_path_set(lv.n_paths["2"])
    assert_same_result(ex.join(lv.uids["2"], k1, d.select(lv.data_inds["2"]), k2), want["lst2"])
    k3 = ex.create_path_set(lv.n_paths["3"])
    assert_same_result(ex.join(lv.uids["3"], k2, d.select(lv.data_inds["3"]), k3), want["lst3"])
    np.testing.assert_array_equal(k3.to_numpy(), want["paths3"])
    ex.close()
