"""Burden tests of per-patient weights on the device (gcre_patient_burden: k_burden_planes, k_burden_null, k_burden_finish;
DESIGN.md §3.14) against ``report.burden_reference`` on the masks read back through ``JoinExec.perm_mask``: totals,
observed sums, every null sum, both tail counts, planes and p-values, every comparison exact (pytest -m gpu).  The
hand-worked cases of the definition itself are in tests/test_burden_host.py.

A context needs at least one case and one control (gcre_create), so the smallest cohort has 2 patients.

GCRE_BURDEN_FUZZ_CASES=300 [GCRE_BURDEN_FUZZ_BASE=...] for a long run of the seeded loop at the end
(GCRE_BURDEN_FUZZ_OUT: a file for its summary); a handful by default."""
from __future__ import annotations

import os

import numpy as np
import pytest

from geneticscre_amd import api, report, synth

pytestmark = pytest.mark.gpu

BIG = 2**31 - 1
INT_KEYS = ("total", "observed", "n_ge", "n_le", "planes")
# row maxima: none, the small ones, around an item's four planes (2^4 - 1 .. 2^4 + 1), the largest weight
MAXIMA = [0, 1, 2, 3, 15, 16, 17, BIG]


def masks_of(ex):
    """every permutation mask of the context as the device holds it, packed: uint64 [iterations][width_ul]"""
    if ex.iters == 0:
        return np.zeros((0, ex.width_ul), np.uint64)
    return np.stack([ex.perm_mask(r) for r in range(ex.iters)])


def same(got, want, what="", null=True):
    for k in INT_KEYS:
        assert got[k].dtype == (np.int32 if k == "planes" else np.int64), (k, got[k].dtype)
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} {what}")
    for k in ("p_upper", "p_lower"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} {what}")      # (NaN equals NaN here)
    if null:
        assert got["null"].dtype == np.int64 and got["null"].shape == want["null"].shape, (what, got["null"].shape)
        np.testing.assert_array_equal(got["null"], want["null"], err_msg=f"null {what}")
    else:
        assert "null" not in got


def check(ex, w, masks=None, null=True, what=""):
    masks = masks_of(ex) if masks is None else masks
    got = ex.patient_burden(w, null=null)
    same(got, report.burden_reference(w, masks, ex.num_cases), what, null)
    return got


def weights_with_maxima(rng, maxima, n):
    """one row per maximum: values below it, the maximum itself at least once (a zero maximum: a row of zeros)"""
    w = np.zeros((len(maxima), n), np.int64)
    for g, top in enumerate(maxima):
        if top:
            w[g] = rng.integers(0, top + 1, n) * (rng.random(n) < 0.7)
            w[g, int(rng.integers(0, n))] = top
    return w


def context(n, nc, K, seed=1, strata=None, method=1):
    ex = api.JoinExec(method, nc, n - nc, K)
    if K:
        ex.generate_permutations(seed, strata)
    return ex


def raw_burden(ex, w, n_rows=None, n_cols=None, want_out=True, want_null=False):
    """gcre_patient_burden through the C entry: (rc, records, null sums); the outputs start as -7."""
    lib = api._burden_lib()
    w32 = None if w is None else np.ascontiguousarray(w, np.int32)
    R = (0 if w32 is None else w32.shape[0]) if n_rows is None else n_rows
    C = (ex.num_cases + ex.num_ctrls) if n_cols is None else n_cols
    rec = np.zeros(max(R, 1), api.BURDEN) if want_out else None
    if rec is not None:
        rec.view(np.uint8)[:] = 0xF9
    null = np.full((max(R, 1), ex.iters), -7, np.int64) if want_null else None
    rc = lib.gcre_patient_burden(ex._h, api._ptr(w32), R, C, api._ptr(rec), api._ptr(null))
    return rc, rec, null


# ---- 1. patients: the partial last dword, the second plane word, stray mask bits --------------------------------------------------

# n_cases off a dword boundary, and once at each end a context admits
@pytest.mark.parametrize("n,nc", [(2, 1), (31, 13), (32, 1), (33, 32), (64, 32), (65, 33), (77, 45), (2048, 1000), (2085, 1037)])
def test_patients(n, nc):
    rng = np.random.default_rng(200 + n)
    K = 70
    w = weights_with_maxima(rng, [5, 0, BIG, 1, 200], n)
    w[0, n - 1] = 5                                        # the last patient carries weight
    ex = context(n, nc, K, seed=n)
    try:
        m = masks_of(ex)
        bits = report.unpack_masks(m, n)
        assert (bits.sum(axis=1) == nc).all()
        got = check(ex, w, m, what=f"n {n} generated")
        assert got["planes"].tolist() == [3, 0, 31, 1, 8] and got["n_ge"][1] == got["n_le"][1] == K
        # caller-given masks with stray bits beyond the patients in the last word: they select nobody
        W = -(-n // 64)
        given = rng.integers(0, 2**63, (K, W), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (K, W)).astype(np.uint64)
        ex.set_permuted_masks(given)
        m = masks_of(ex)
        np.testing.assert_array_equal(m, given)
        assert n % 64 == 0 or (m[:, -1] >> np.uint64(n % 64)).any()
        check(ex, w, m, what=f"n {n} given")
    finally:
        ex.close()


# ---- 2. permutations: the lane, wave and tile edges; the padding is never counted ---------------------------------------------------

@pytest.mark.parametrize("K", [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1025])
def test_permutations(K):
    n, nc = 77, 30
    rng = np.random.default_rng(300 + K)
    w = weights_with_maxima(rng, [9, 1, 70000], n)
    w[1, :nc] = 0                                          # observed = 0 with a non-zero row: every sum is >= 0 = observed
    w[1, nc] = 1
    ex = context(n, nc, K, seed=K)
    try:
        got = check(ex, w, what=f"K {K}")
        assert got["observed"][1] == 0 and got["planes"][1] == 1
        assert got["n_ge"][1] == K                         # every permutation, and not one of the padding
        lo = np.zeros((1, n), np.int64)
        lo[0, :nc] = 3                                     # observed = the largest sum there is: every sum is <= observed
        got = check(ex, lo, what=f"K {K} top")
        assert got["n_le"][0] == K and got["observed"][0] == 3 * nc
        # observed = 0 and a row that is launched: n_le counts the permutations with sum 0, exactly, never the padded ones
        z = np.zeros((2, n), np.int64)
        z[0, nc:] = 1                                      # all controls carry 1: the sum is 0 only for the identity split
        z[1, n - 1] = 4
        got = check(ex, z, what=f"K {K} zero observed")
        assert got["observed"].tolist() == [0, 0] and (got["n_le"] <= K).all() and (got["n_ge"] == K).all()
        zero = check(ex, np.zeros((1, n), np.int64), what=f"K {K} zero row")
        assert zero["n_le"][0] == K and zero["n_ge"][0] == K
        # masks that never pick the last patient, a control, and a row that weighs nobody else: the row is launched, every
        # sum is 0 = observed, and n_le is exactly K -- a padded permutation (sum 0 <= 0) would make it more
        m = masks_of(ex)
        m[:, -1] &= ~np.uint64(1 << ((n - 1) % 64))
        ex.set_permuted_masks(m)
        before = ex.burden_launches
        got = check(ex, z[1:], m, what=f"K {K} nobody picked")
        assert ex.burden_launches - before == 3 and got["planes"][0] == 3 and got["observed"][0] == 0 and not got["null"].any()
        assert got["n_le"][0] == K and got["n_ge"][0] == K
    finally:
        ex.close()


# ---- 3. planes: rows with different maxima in one call ---------------------------------------------------------------------------

@pytest.mark.parametrize("rows", [1, 3, 4, 5, 9])
def test_planes(rows):
    n, nc, K = 100, 41, 130
    rng = np.random.default_rng(400 + rows)
    ex = context(n, nc, K, seed=rows)
    try:
        m = masks_of(ex)
        # every maximum appears, `rows` rows at a time, rotated so that every call mixes widths
        for start in range(len(MAXIMA)):
            maxima = [MAXIMA[(start + 3 * k) % len(MAXIMA)] for k in range(rows)]
            before = ex.burden_launches
            got = check(ex, weights_with_maxima(rng, maxima, n), m, what=f"maxima {maxima}")
            assert got["planes"].tolist() == [int(x).bit_length() for x in maxima]
            assert ex.burden_launches - before == (3 if any(maxima) else 0)
    finally:
        ex.close()


def test_sums_beyond_32_bits():
    ex = context(5, 3, 64, seed=5)
    try:
        got = check(ex, np.full((2, 5), BIG, np.int64), what="all 2^31 - 1")
        assert got["total"].tolist() == [5 * BIG] * 2 and got["observed"].tolist() == [3 * BIG] * 2
        assert (got["null"] == 3 * BIG).all() and 3 * BIG > 2**32
    finally:
        ex.close()
    # the most a sum can be: 65,535 cases of the largest weight (the 65,536-patient limit), below 2^47
    n = 65536
    ex = context(n, n - 1, 3, seed=6)
    try:
        got = check(ex, np.full((1, n), BIG, np.int64), what="65,535 x (2^31 - 1)")
        assert (got["null"] == (n - 1) * BIG).all() and got["observed"][0] == (n - 1) * BIG < 2**47
    finally:
        ex.close()


def test_ties():
    n, nc, K = 8, 4, 512
    w = np.array([[1, 1, 0, 0, 1, 1, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0]], np.int64)
    ex = context(n, nc, K, seed=12)
    try:
        m = masks_of(ex)
        want = report.burden_reference(w, m, nc)
        # the case is what it is meant to be: permutations tie the observed value, and a tie counts in both tails
        assert ((want["null"] == want["observed"][:, None]).sum(axis=1) >= 1).all()
        assert (want["n_ge"] + want["n_le"] > K).all()
        assert ((want["null"] > want["observed"][:, None]).any(axis=1) | (want["null"] < want["observed"][:, None]).any(axis=1)).all()
        same(ex.patient_burden(w, null=True), want, "ties")
    finally:
        ex.close()


# ---- 4. invariants that need no reference ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("stratified", [False, True])
def test_invariants(stratified):
    n, nc, K = 150, 61, 700
    rng = np.random.default_rng(50)
    strata = (np.arange(n) * 7 % 4).astype(np.int32) if stratified else None
    ex = context(n, nc, K, seed=77, strata=strata)
    try:
        for c in (1, 6, 1000, BIG):
            got = ex.patient_burden(np.full((1, n), c, np.int64), null=True)
            assert (got["null"] == c * nc).all() and got["observed"][0] == c * nc and got["total"][0] == c * n
            assert got["n_ge"][0] == K and got["n_le"][0] == K and got["p_upper"][0] == 1.0 and got["p_lower"][0] == 1.0
        # the complement c - w mirrors every sum about c * n_cases: the tails swap
        c = 37
        w = rng.integers(0, c + 1, (4, n))
        a, b = ex.patient_burden(w, null=True), ex.patient_burden(c - w, null=True)
        np.testing.assert_array_equal(a["null"] + b["null"], np.full((4, K), c * nc))
        np.testing.assert_array_equal(a["n_ge"], b["n_le"])
        np.testing.assert_array_equal(a["n_le"], b["n_ge"])
        assert 0 < a["n_ge"].min() and a["n_ge"].max() < K          # not degenerate
    finally:
        ex.close()


# ---- 5. mask roads ------------------------------------------------------------------------------------------------------------

def test_mask_roads():
    n, nc = 90, 40
    rng = np.random.default_rng(60)
    w = weights_with_maxima(rng, [7, 300, 1], n)
    # caller-given permutation rows: fewer rows than iterations are reused, more are truncated; a row need not hold n_cases ones
    for K, rows_in in ((50, 50), (50, 7), (50, 80)):
        perms = (rng.random((rows_in, n)) < 0.5).astype(np.int32)
        perms[0] = 1                                          # nobody flipped: the cases themselves
        ex = api.JoinExec(1, nc, n - nc, K)
        try:
            ex.set_permuted_cases(perms)
            m = masks_of(ex)
            bits = report.unpack_masks(m, n)
            assert (bits.sum(axis=1) != nc).any() and bits[0].tolist() == [1] * nc + [0] * (n - nc)
            if rows_in < K:
                np.testing.assert_array_equal(m[rows_in:2 * rows_in], m[:rows_in])
            got = check(ex, w, m, what=f"{rows_in} rows for {K} iterations")
            np.testing.assert_array_equal(got["null"][:, 0], got["observed"])
        finally:
            ex.close()
    # a permutation window is the joins' business: every permutation counts
    K = 2100
    ex = context(n, nc, K, seed=9)
    try:
        m = masks_of(ex)
        full = check(ex, w, m, what="no window")
        ex.set_perm_window(0, 2048)
        same(ex.patient_burden(w, null=True), full, "window 0..2048")
        ex.set_perm_window(2048, K)
        same(ex.patient_burden(w, null=True), full, "window 2048..K")
    finally:
        ex.close()


# ---- 6. knobs ---------------------------------------------------------------------------------------------------------------------

def test_slabs_and_null_change_nothing(monkeypatch):
    n, nc, K = 130, 55, 600
    rng = np.random.default_rng(70)
    w = weights_with_maxima(rng, [3, 0, BIG, 17, 0, 1, 90], n)
    monkeypatch.delenv("GCRE_BURDEN_SLAB_ROWS", raising=False)
    monkeypatch.delenv("GCRE_BURDEN_MAX_MB", raising=False)
    ex = context(n, nc, K, seed=4)
    try:
        m = masks_of(ex)
        full = check(ex, w, m, what="default")
        launches = {}
        for slab in ("1", "2", "3", "100"):
            monkeypatch.setenv("GCRE_BURDEN_SLAB_ROWS", slab)
            before = ex.burden_launches
            same(ex.patient_burden(w, null=True), full, f"slab rows {slab}")
            launches[slab] = ex.burden_launches - before
            check(ex, w, m, null=False, what=f"slab rows {slab}, no null")
        # three kernels per slab with a non-zero row: rows 1 and 4 are zeros
        assert launches == {"1": 15, "2": 12, "3": 9, "100": 3}
        monkeypatch.delenv("GCRE_BURDEN_SLAB_ROWS")
        # the byte bound cuts slabs too: one row of 31 planes and 2,048 sums fits, two do not
        monkeypatch.setenv("GCRE_BURDEN_MAX_MB", str((31 * 8 * 4 + 2048 * 8 + 100) / 1048576))
        before = ex.burden_launches
        same(ex.patient_burden(w, null=True), full, "one row per slab by bytes")
        assert ex.burden_launches - before == 15
    finally:
        ex.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(monkeypatch):
    n, nc, K = 45, 20, 30
    rng = np.random.default_rng(3)
    w = rng.integers(0, 9, (3, n))
    w[:, 0] = 8                                              # four planes in every row
    monkeypatch.delenv("GCRE_BURDEN_MAX_MB", raising=False)
    monkeypatch.delenv("GCRE_BURDEN_SLAB_ROWS", raising=False)
    ex = api.JoinExec(1, nc, n - nc, K)
    lib = api._burden_lib()
    ARG, ASSERT = api.GCRE_ERR_ARG, api.GCRE_ERR_ASSERT
    W = b"patient_burden: "

    def failed(res, code, text):
        msg = ex._lib.gcre_last_error(ex._h)
        assert res[0] == code and text in msg, (res[0], msg)
        assert ex.burden_launches == 0

    # no masks yet
    failed(raw_burden(ex, w), ASSERT, b"assertion: patient_burden needs the permutation masks")
    with pytest.raises(ValueError, match="needs the permutation masks"):
        ex.patient_burden(w)
    ex.generate_permutations(8)
    neg = w.copy()
    neg[2, 44] = -1
    failed(raw_burden(ex, neg), ARG, W + b"weights[2][44] = -1 is negative")
    failed(raw_burden(ex, None, n_rows=2), ARG, W + b"NULL weights with 2 rows")
    failed(raw_burden(ex, w, want_out=False), ARG, W + b"NULL out")
    failed(raw_burden(ex, w, n_rows=-1), ARG, W + b"n_rows must not be negative")
    failed(raw_burden(ex, w[:, :44], n_cols=44), ARG, W + b"44 columns for 45 patients")
    failed(raw_burden(ex, np.zeros((1, 46), np.int32), n_cols=46), ARG, W + b"46 columns for 45 patients")
    monkeypatch.setenv("GCRE_BURDEN_MAX_MB", "0.015")            # 15,728 bytes: the 2,048 sums of a row alone are 16,384
    failed(raw_burden(ex, w), ARG, W + b"one row of 4 planes and 2048 sums takes 16512 bytes: above GCRE_BURDEN_MAX_MB")
    # a refused call leaves the outputs alone
    rc, rec, null = raw_burden(ex, neg, want_null=True)
    assert rc == ARG and (rec.view(np.uint8) == 0xF9).all() and (null == -7).all()
    monkeypatch.delenv("GCRE_BURDEN_MAX_MB")
    assert lib.gcre_patient_burden(None, None, 0, 0, None, None) == ARG
    # not refusals, and nothing launched: no rows, a row of zeros
    rc, rec, _ = raw_burden(ex, None, n_rows=0)
    assert rc == api.GCRE_OK and (rec.view(np.uint8) == 0xF9).all()
    got = ex.patient_burden(np.zeros((0, n), np.int32), null=True)
    assert got["total"].shape == (0,) and got["null"].shape == (0, K)
    got = ex.patient_burden(np.zeros((2, n), np.int32), null=True)
    assert got["planes"].tolist() == [0, 0] and got["n_ge"].tolist() == [K, K] and got["n_le"].tolist() == [K, K]
    assert got["p_upper"].tolist() == [1.0, 1.0] and not got["null"].any()
    assert ex.burden_launches == 0
    # the Python method: its own ValueErrors, and the library's message
    with pytest.raises(ValueError, match="every weight must lie in"):
        ex.patient_burden(neg)
    with pytest.raises(ValueError, match=r"weights: \[rows\]\[45\]"):
        ex.patient_burden(w[:, :44])
    assert ex.burden_launches == 0
    # the context still works
    check(ex, w, what="after the refusals")
    assert ex.burden_launches == 3
    ex.close()
    # no iterations: totals and observed sums, zero counts, NaN, nothing launched, no masks needed
    ex = api.JoinExec(2, nc, n - nc, 0)
    try:
        got = check(ex, w, what="0 iterations")
        assert got["n_ge"].tolist() == [0, 0, 0] and got["n_le"].tolist() == [0, 0, 0] and got["null"].shape == (3, 0)
        assert np.isnan(got["p_upper"]).all() and np.isnan(got["p_lower"]).all()
        assert got["observed"].tolist() == w[:, :nc].sum(axis=1).tolist() and got["planes"].tolist() == [4, 4, 4]
        assert ex.burden_launches == 0
    finally:
        ex.close()


# ---- 8. round trips -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", [1, 2])
def test_patient_counts_into_patient_burden(method):
    n, nc, K = 140, 66, 300
    rng = np.random.default_rng(80 + method)
    R, S = 12, 90
    rows = (rng.random((R, n)) < 0.2).astype(np.int8)
    sets = [rng.integers(0, R, int(rng.integers(1, 5))).tolist() for _ in range(S)]
    sets[3][0] = -1
    signs = [rng.choice([1, -1], len(s)).tolist() for s in sets]
    group = rng.integers(-1, 4, S)
    ex = context(n, nc, K, seed=31, method=method)
    try:
        m = masks_of(ex)
        for by_sign in (False, True):
            counts, group_sets, skipped = ex.patient_counts(sets, rows, group=group, n_groups=4, by_sign=by_sign, signs=signs)
            ref_counts = report.patient_counts_reference(sets, rows, signs, None, group, 4, n, by_sign)[0]
            np.testing.assert_array_equal(counts, ref_counts)
            got = ex.patient_burden(counts, null=True)                      # [G][H][n], flattened to G * H rows
            same(got, report.burden_reference(ref_counts, m, nc), f"method {method} by_sign {by_sign}")
            assert len(got["total"]) == 4 * (2 if by_sign else 1) and got["total"].sum() == ref_counts.sum() > 0
    finally:
        ex.close()


def test_burden_test_as_a_gene_set_burden():
    import pandas as pd
    nc, nt, K = 60, 70, 400
    n = nc + nt
    rng = np.random.default_rng(90)
    genes = [f"G{i}" for i in range(25)]
    data = (rng.random((25, n)) < 0.08).astype(np.int32)
    data[3, :nc] |= (rng.random(nc) < 0.3).astype(np.int32)             # one gene the cases carry more often
    pathways = {"A": ["G3", "G4", "G5"], "B": ["G6", "G7", "missing", "G8"], "C": ["G20"]}
    sets = [[g] for p in pathways.values() for g in p]
    group = [i for i, p in enumerate(pathways.values()) for _ in p]
    strata = (np.arange(n) % 2).astype(np.int32)
    kw = dict(group=group, names=list(pathways), threshold=0.5, n_permutations=K, strata=strata, seed=5)
    table = report.burden_test(sets, genes, data, nc, nt, **kw)
    # numpy: per patient the number of the pathway's genes with a variant, on the masks the same seed draws
    ex = context(n, nc, K, seed=5, strata=strata)
    try:
        m = masks_of(ex)
    finally:
        ex.close()
    load = np.stack([data[[genes.index(g) for g in p if g in genes]].sum(axis=0) for p in pathways.values()])
    want = report.burden_table(report.burden_reference(load, m, nc), nc, nt, names=list(pathways), group_sets=[3, 3, 1])
    pd.testing.assert_frame_equal(table, want, check_exact=True)
    assert table.attrs["skipped"] == 1 and table["Load"].tolist() == load.sum(axis=1).tolist()
    assert table["PvalueUpper"][0] < 0.05                                  # the planted gene's pathway
    # signed: a (+) and a (-) row per group
    ssets = ["G3 (+) -> G4 (-)", "G5 (-)", "G6 (+) -> G7 (+)"]
    st = report.burden_test(ssets, genes, data, nc, nt, signed=True, group=[0, 0, 1], names=["x", "y"], threshold=0.5,
                            n_permutations=K, strata=strata, seed=5)
    assert st["Group"].tolist() == ["x (+)", "x (-)", "y (+)", "y (-)"] and st["Sets"].tolist() == [2, 2, 1, 1]
    sload = np.stack([data[3], data[4] + data[5], data[6] | data[7], np.zeros(n, np.int32)])
    swant = report.burden_table(report.burden_reference(sload, m, nc), nc, nt, names=st["Group"].tolist(), group_sets=[2, 2, 1, 1])
    pd.testing.assert_frame_equal(st, swant, check_exact=True)


def _network_case(seed, nc=48, nt=52):      # the small problem of test_gpu_patients.py
    rng = np.random.default_rng(seed)
    g, src, trg, sign = synth.signed_network(30, 70, rng)
    uid = np.arange(g) * 5 + 100
    symbols = [f"G{u}" for u in uid]
    data = (rng.random((g, nc + nt)) < 0.06).astype(np.int32)
    return symbols, data, (uid, symbols, uid[src], uid[trg], sign)


@pytest.mark.parametrize("signed", [False, True])
def test_replicate(signed):
    import pandas as pd
    nc, nt, K = 48, 52, 500
    genes, data, network = _network_case(17)
    # discovery: the top rows of every length, clumped
    found = report.gwaspa(genes, data, nc, nt, network, signed=signed, threshold=0.2, n_permutations=200, seed=909, path_length=5,
                          top_k=6, clump=0.5)["GWASPA.Results"]
    assert len(found) > 10 and len(set(found["Lengths"])) == 5 and "ClumpLead" in found
    # replication: another cohort of the same genes from another seed, without two of them
    genes2, data2, _ = _network_case(18, 40, 45)
    n2c, n2t = 40, 45
    used = sorted({g for p in found["Paths"] for g in str(p).split(" -> ")})
    gone = set(used[:2])
    keep = [i for i, g in enumerate(genes2) if g not in gone]
    genes2, data2 = [genes2[i] for i in keep], data2[keep]
    ex = context(n2c + n2t, n2c, K, seed=33)
    try:
        m = masks_of(ex)
    finally:
        ex.close()
    pgenes, pdata = report.preprocess_table(genes2, data2, 0.2, n2c, n2t)
    col = "SignedPaths" if signed else "Paths"
    names, rows, _ = report.parse_sets([str(p) for p in found[col]], pgenes)
    na = np.array([any(r < 0 for r in rs) for rs in rows])
    assert 0 < na.sum() < len(found)
    lengths = np.array([len(x) for x in names])
    np.testing.assert_array_equal(lengths, found["Lengths"].to_numpy())
    for leads_only in (False, True):
        got = report.replicate(found, genes2, data2, n2c, n2t, signed=signed, threshold=0.2, n_permutations=K, seed=33,
                               leads_only=leads_only)
        assert set(got) == {"Replication.Paths", "Replication.Burden", "skipped"}
        sp = report.score_paths([str(p) for p in found[col]], genes2, data2, n2c, n2t, signed, 0.2, K, None, 33)
        pd.testing.assert_frame_equal(got["Replication.Paths"], sp, check_exact=True)
        assert list(sp.columns) == report.SCORE_PATHS_COLUMNS and np.isnan(sp["Scores"].to_numpy()[na]).all()
        keep_rows = (found["ClumpLead"] == found["Paths"]).to_numpy() if leads_only else np.ones(len(found), bool)
        assert 0 < keep_rows.sum()
        load = np.zeros((6, n2c + n2t), np.int64)
        sets_in = np.zeros(6, np.int64)
        skipped_in = np.zeros(6, np.int64)
        for i in np.flatnonzero(keep_rows):
            for g in (lengths[i] - 1, 5):
                if na[i]:
                    skipped_in[g] += 1
                else:
                    load[g] += pdata[rows[i]].any(axis=0)
                    sets_in[g] += 1
        want = report.burden_table(report.burden_reference(load, m, n2c), n2c, n2t, names=["L1", "L2", "L3", "L4", "L5", "All"],
                                   group_sets=sets_in)
        want["Skipped"] = skipped_in
        table = got["Replication.Burden"]
        assert list(table.columns) == report.BURDEN_COLUMNS + report.BURDEN_NULL_COLUMNS + ["Skipped"]
        pd.testing.assert_frame_equal(table, want, check_exact=True)
        assert got["skipped"] == int(na[keep_rows].sum()) == table["Skipped"][5] and table["Load"][5] == table["Load"][:5].sum() > 0
    with pytest.raises(ValueError, match="leads_only: the table has no ClumpLead column"):
        report.replicate(found.drop(columns="ClumpLead"), genes2, data2, n2c, n2t, signed=signed, threshold=0.2, leads_only=True)


# ---- 9. seeded loop -----------------------------------------------------------------------------------------------------------------
N_FUZZ = int(os.environ.get("GCRE_BURDEN_FUZZ_CASES", "6"))
FUZZ_BASE = int(os.environ.get("GCRE_BURDEN_FUZZ_BASE", "0"))


def test_seeded_loop(monkeypatch):
    lines = []
    for k in range(FUZZ_BASE, FUZZ_BASE + N_FUZZ):
        rng = np.random.default_rng(9_000_000 + k)
        n = int(rng.choice([int(rng.integers(2, 70)), int(rng.integers(70, 600)), int(rng.integers(2049, 4300))]))
        nc = int(rng.integers(1, n))
        K = int(rng.choice([int(rng.integers(1, 70)), int(rng.integers(400, 700)), int(rng.integers(2040, 2060))]))
        R = int(rng.integers(1, 12))
        maxima = [int(rng.choice([0, 1, int(rng.integers(1, 40)), int(rng.integers(40, 70000)), BIG])) for _ in range(R)]
        w = weights_with_maxima(rng, maxima, n)
        n_strata = int(rng.choice([0, 2, 5]))
        strata = rng.integers(0, n_strata, n).astype(np.int32) if n_strata and n >= 10 else None
        slab = rng.choice(["", "1", "2", "5"])
        if slab:
            monkeypatch.setenv("GCRE_BURDEN_SLAB_ROWS", str(slab))
        else:
            monkeypatch.delenv("GCRE_BURDEN_SLAB_ROWS", raising=False)
        null = bool(rng.integers(0, 2))
        ex = context(n, nc, K, seed=k, strata=strata, method=1 + k % 2)
        try:
            got = check(ex, w, null=null, what=f"case {k}")
        finally:
            ex.close()
        lines.append(f"case {k}: patients {n} cases {nc} permutations {K} rows {R} planes {got['planes'].tolist()} "
                     f"strata {n_strata if strata is not None else 0} slab {slab or 'default'} null {int(null)} "
                     f"n_ge {got['n_ge'].tolist()} n_le {got['n_le'].tolist()} ok")
    out = os.environ.get("GCRE_BURDEN_FUZZ_OUT")
    if out:
        with open(out, "w") as f:
            f.write(f"test_gpu_burden.py::test_seeded_loop: cases {FUZZ_BASE}..{FUZZ_BASE + N_FUZZ - 1}, every one exact\n")
            f.write("\n".join(lines) + "\n")
