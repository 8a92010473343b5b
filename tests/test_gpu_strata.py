"""Stratified set scores on the device (gcre_score_sets_strata: k_strata_masks, k_strata_check, k_strata_rows,
k_strata_observed, k_strata_null).  Everything ``JoinExec.strata_tests(family=True, null=True, terms=True)``
returns is compared exactly against ``report.strata_reference`` on the same tables and on the masks ``report.permutation_masks``
gives for the context's seed and strata -- the counts as integers, the scores as bit patterns -- and the records against
``score_sets``.  The shapes are the smallest at which each part can go wrong: the dword that straddles n_cases, a stratum
boundary inside a dword, one stratum more than a step tile, sixteen strata, permutations around the 512-permutation tile, sets
around a block of four, slabs by count and by bytes."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from geneticscre_amd import api, report
from helpers import small_table, special_table

pytestmark = pytest.mark.gpu

N_ROWS = 90
ENV = ("GCRE_STRATA_MAX_MB", "GCRE_STRATA_SLAB_SETS")
COUNTERS = [("given", "gcre_given_launches"), ("family", "gcre_family_launches"), ("minp", "gcre_minp_launches"),
            ("compete", "gcre_compete_launches"), ("prefix", "gcre_prefix_launches"), ("subsample", "gcre_subsample_launches"),
            ("dose", "gcre_dose_launches"), ("sequential", "gcre_sequential_launches"), ("overlap", "gcre_overlap_launches"),
            ("clump", "gcre_clump_launches"), ("patients", "gcre_patient_launches"), ("burden", "gcre_burden_launches"),
            ("stepdown", "gcre_stepdown_launches"), ("hits", "gcre_hits_launches")]


def other_counters(ex):
    """Every launch counter of the context but the stage's own."""
    return [int(getattr(api._feature_lib(f), sym)(ex._h)) for f, sym in COUNTERS]


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)


def make_rows(rng, n, n_rows=N_ROWS):
    rows = (rng.random((n_rows, n)) < rng.uniform(0.02, 0.5, size=(n_rows, 1))).astype(np.int8)
    rows[0], rows[1] = 1, 0            # everybody, nobody
    return rows


def make_family(rng, n_rows=N_ROWS):
    """Sets of 1, 2 and 65 members, a repeated member row, an NA member, everybody and nobody, and sets of one sign only."""
    sets = [[int(rng.integers(2, n_rows))], rng.integers(2, n_rows, 2).tolist(), rng.permutation(n_rows)[:65].tolist(),
            [5, 5, 7], [4, -1, 9], [0], [1], rng.integers(2, n_rows, 3).tolist(), rng.integers(2, n_rows, 4).tolist()]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    signs[-2] = [1] * 3                # (+) only: the (-) union is empty
    signs[-1] = [-1] * 4               # (-) only
    return sets, signs


def stratum_tables(nc, strata, seed=0, negatives=0.1):
    """One table per stratum (ids ascending), of the stratum's own size, a share of the cells negative."""
    st = np.asarray(strata)
    rng = np.random.default_rng([77, seed])
    tables = []
    for i in np.unique(st):
        t = small_table(int((st[:nc] == i).sum()), int((st[nc:] == i).sum()), seed + len(tables))
        t[rng.random(t.shape) < negatives] *= -1
        tables.append(t)
    return tables


def open_context(method, nc, nt, K, seed=1, strata=None, VT=None):
    ex = api.JoinExec(method, nc, nt, K)
    ex.set_value_table(small_table(nc, nt, 3) if VT is None else VT)
    if K > 0:
        ex.generate_permutations(seed, None if strata is None else np.unique(strata, return_inverse=True)[1])
    return ex


def bits(a):
    """The bit patterns of doubles, every NaN as one pattern: the sign of the NaN that inf - inf gives is the adder's own."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.float64(np.nan), a).view(np.uint64)


def assert_equal_reference(got, ref, what=""):
    rec, sr, fam, nul, trm, cnt = got
    assert sr.dtype == api.STRATA_SCORE and fam.dtype == nul.dtype == trm.dtype == np.float64 and cnt.dtype == np.int32
    np.testing.assert_array_equal(bits(sr["score"]), bits(ref["score"]), err_msg=f"{what} score")
    np.testing.assert_array_equal(sr["n_ge"], ref["n_ge"], err_msg=f"{what} n_ge")
    np.testing.assert_array_equal(bits(trm), bits(ref["terms"]), err_msg=f"{what} terms")
    np.testing.assert_array_equal(cnt, ref["counts"], err_msg=f"{what} counts")
    np.testing.assert_array_equal(bits(nul), bits(ref["null_scores"]), err_msg=f"{what} null_scores")
    np.testing.assert_array_equal(fam.view(np.uint64), ref["family_max"].view(np.uint64), err_msg=f"{what} family_max")
    assert (rec["valid"] != 0).tolist() == (sr["n_ge"] >= 0).tolist()
    # the per-stratum counts add up to the record's
    ok = rec["valid"] != 0
    for j, k in enumerate(("cases_pos", "ctrls_pos", "cases_neg", "ctrls_neg")):
        np.testing.assert_array_equal(cnt[ok][:, :, j].sum(axis=1), rec[k][ok], err_msg=f"{what} {k}")


def run_and_compare(ex, method, nc, nt, sets, rows, signs, strata, tables, K, seed, what=""):
    """One call with every output against the reference of the same arguments: (what the call returned, the reference)."""
    masks = report.permutation_masks(nc, nt, K, seed, np.unique(strata, return_inverse=True)[1]) if K > 0 else None
    ref = report.strata_reference(sets, rows, signs, nc, strata, tables, masks, method)
    got = ex.strata_tests(sets, rows, signs, strata=strata, tables=tables, family=True, null=True, terms=True)
    assert_equal_reference(got, ref, what)
    return got, ref


def layouts(nc, nt):
    """The strata of the cohort tests, by name."""
    n = nc + nt
    q = np.arange(n)
    three = np.concatenate([np.arange(nc) % 2, np.arange(nt) % 3])            # stratum 2 holds controls only
    inside = (q >= 13).astype(int) + (q >= 45)                                 # boundaries at patients 13 and 45: inside dwords 0 and 1
    return [("one", np.zeros(n, int)), ("two interleaved", q % 2), ("three, one without a case", three), ("five", q % 5),
            ("sixteen", (q * 7) % 16), ("a boundary inside a dword", inside)]


# ---- cohort shapes x strata ---------------------------------------------------------------------------------------------


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("cohort", [(1, 1), (31, 2), (32, 32), (33, 31), (65, 135)])
def test_cohort_shapes_and_strata(method, cohort):
    nc, nt = cohort
    n = nc + nt
    rng = np.random.default_rng([7100, method, nc, nt])
    rows = make_rows(rng, n)
    sets, signs = make_family(rng)
    K = 70
    ex = open_context(method, nc, nt, K)
    try:
        plain = ex.score_sets(sets, rows, signs)
        others = other_counters(ex)
        launches = 0
        for i, (name, strata) in enumerate(layouts(nc, nt)):
            strata = strata * 3 + 5                                           # any integers
            ex.generate_permutations(20 + i, np.unique(strata, return_inverse=True)[1])
            tables = stratum_tables(nc, strata, 10 * i)
            got, ref = run_and_compare(ex, method, nc, nt, sets, rows, signs, strata, tables, K, 20 + i, f"{cohort} {name}")
            rec, sr = got[0], got[1]
            ex2 = ex.score_sets(sets, rows, signs)
            assert rec.tobytes() == ex2.tobytes()                             # the records of score_sets under these masks
            assert rec["score"].tobytes() == plain["score"].tobytes()
            launches += 2 + len(np.unique(strata)) + 3                        # indicator rows, check, tables, one slab
            assert ex.strata_launches() == launches
            assert sr["n_ge"][4] == -1 and np.isnan(sr["score"][4]) and np.isnan(got[3][4]).all() and (got[5][4] == 0).all()
        assert other_counters(ex) == others
        # the default tables: the library's builder at every stratum's own size
        strata = layouts(nc, nt)[1][1]
        ex.generate_permutations(3, strata)
        tables = [api.values_table(int((strata[:nc] == s).sum()), int((strata[nc:] == s).sum())) for s in np.unique(strata)]
        masks = report.permutation_masks(nc, nt, K, 3, np.unique(strata, return_inverse=True)[1])
        ref = report.strata_reference(sets, rows, signs, nc, strata, tables, masks, method)
        rec, sr = ex.strata_tests(sets, rows, signs, strata=strata)
        assert np.array_equal(bits(sr["score"]), bits(ref["score"])) and np.array_equal(sr["n_ge"], ref["n_ge"])
    finally:
        ex.close()


# ---- a larger cohort: many chunks, two strata split off the chunk grid ----------------------------------------------------


@pytest.mark.parametrize("method", [1, 2])
def test_a_larger_cohort(method):
    nc, nt = 4100, 4157
    n = nc + nt
    q = np.arange(n)
    strata = ((q >= 3001) & (q < nc)) | (q >= nc + 2222)                     # 3,001 is no multiple of 128 (nor of 32)
    strata = strata.astype(int)
    rng = np.random.default_rng([7200, method])
    rows = make_rows(rng, n, 40)
    sets = [[2], [3, 4], rng.permutation(40)[:30].tolist(), [0], [1], [5, -1], [6, 7, 8], [9, 10], [11]]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    # tables smaller than their strata beyond 700 carriers a side: the cells they lack read as -1
    tables = [small_table(700, 700, 1), small_table(1099, 600, 2)]
    K = 40
    ex = open_context(method, nc, nt, K, seed=9, strata=strata)
    try:
        assert 8 * ((ex.width_ul + 3) // 4) // 4 == 66                        # 66 chunks of four dwords
        got, ref = run_and_compare(ex, method, nc, nt, sets, rows, signs, strata, tables, K, 9, "8,257 patients")
        if method == 1:
            assert (ref["terms"][3] == -1.0).all()                            # everybody: beyond both tables
    finally:
        ex.close()


# ---- permutation counts around the tile ----------------------------------------------------------------------------------


@pytest.mark.parametrize("method", [1, 2])
def test_permutation_counts(method):
    nc, nt = 33, 31
    strata = np.arange(nc + nt) % 3
    rng = np.random.default_rng([7300, method])
    rows = make_rows(rng, nc + nt)
    sets, signs = make_family(rng)
    tables = stratum_tables(nc, strata, 4)
    low = [np.full_like(t, -np.inf) for t in tables]                          # every sum is -inf: >= holds for every live permutation
    for K in (1, 511, 512, 513, 1025):
        ex = open_context(method, nc, nt, K, seed=K, strata=strata)
        try:
            got, ref = run_and_compare(ex, method, nc, nt, sets, rows, signs, strata, tables, K, K, f"K = {K}")
            assert got[3].shape == (len(sets), K) and got[2].shape == (K,)
            rec, sr, fam = ex.strata_tests(sets, rows, signs, strata=strata, tables=low, family=True)
            ok = rec["valid"] != 0
            assert (sr["score"][ok] == -np.inf).all() and (sr["n_ge"][ok] == K).all() and (sr["n_ge"][~ok] == -1).all()
            assert (fam.view(np.uint64) == 0).all()
        finally:
            ex.close()


# ---- set counts around a block --------------------------------------------------------------------------------------------


@pytest.mark.parametrize("method", [1, 2])
def test_set_counts(method):
    nc, nt = 40, 50
    strata = np.arange(nc + nt) % 4
    rng = np.random.default_rng([7400, method])
    rows = make_rows(rng, nc + nt)
    K = 100
    ex = open_context(method, nc, nt, K, seed=2, strata=strata)
    try:
        tables = stratum_tables(nc, strata, 6)
        for S in (1, 4, 5, 9):                                                # one wave, one block, one more, three blocks
            sets = [rng.integers(2, N_ROWS, int(rng.integers(1, 6))).tolist() for _ in range(S)]
            signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
            run_and_compare(ex, method, nc, nt, sets, rows, signs, strata, tables, K, 2, f"{S} sets")
        # an NA set between valid ones: the slots are the valid sets, the outputs the caller's
        sets = [[2], [3, -1], [4], [-1], [5], [6], [7]]
        run_and_compare(ex, method, nc, nt, sets, rows, None, strata, tables, K, 2, "NA sets between")
        # no valid set: defaults, and only the checks' launches? no: nothing of the stage runs without a valid set
        before = ex.strata_launches()
        rec, sr, fam, nul, trm, cnt = ex.strata_tests([[3, -1], [-1]], rows, None, strata=strata, tables=tables, family=True, null=True, terms=True)
        assert ex.strata_launches() == before
        assert (sr["n_ge"] == -1).all() and np.isnan(sr["score"]).all() and (fam == 0).all() and np.isnan(nul).all()
        assert np.isnan(trm).all() and (cnt == 0).all()
    finally:
        ex.close()


# ---- S = 1 identities ----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("method", [1, 2])
def test_one_stratum_identities(method):
    nc, nt = 65, 135
    rng = np.random.default_rng([7500, method])
    rows = make_rows(rng, nc + nt)
    sets, signs = make_family(rng)
    VT = small_table(nc, nt, 8)
    VT[rng.random(VT.shape) < 0.1] *= -1
    K = 600
    ex = open_context(method, nc, nt, K, seed=4, VT=VT)
    try:
        rec, sr, nul = ex.strata_tests(sets, rows, signs, strata=np.full(nc + nt, 9), tables=[VT], null=True)
        plain = ex.score_sets(sets, rows, signs)
        assert rec.tobytes() == plain.tobytes()
        assert sr["score"].tobytes() == plain["score"].tobytes()              # +0.0 + the observed expression, bit for bit
        if method == 1:
            f32 = nul.astype(np.float32)
            folded = np.where(f32 > 0, f32, np.float32(0)).astype(np.float32)
            fam_null = ex.family_tests(sets, rows, signs, null=True)[2]
            ok = rec["valid"] != 0
            assert fam_null[ok].tobytes() == folded[ok].tobytes()
            assert np.isnan(fam_null[~ok]).all() and np.isnan(nul[~ok]).all()
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_swapped_strata(method):
    """Two strata with ids and tables swapped: the two terms are added the other way round, and a + b = b + a."""
    nc, nt = 33, 31
    strata = (np.arange(nc + nt) % 3 == 0).astype(int)
    rng = np.random.default_rng([7600, method])
    rows = make_rows(rng, nc + nt)
    sets, signs = make_family(rng)
    tables = stratum_tables(nc, strata, 12)
    K = 200
    ex = open_context(method, nc, nt, K, seed=6, strata=strata)
    try:
        a = ex.strata_tests(sets, rows, signs, strata=strata, tables=tables, family=True, null=True, terms=True)
        b = ex.strata_tests(sets, rows, signs, strata=1 - strata, tables=tables[::-1], family=True, null=True, terms=True)
        assert a[1].tobytes() == b[1].tobytes()                               # score and n_ge
        assert np.array_equal(bits(a[3]), bits(b[3])) and np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))
        assert np.array_equal(bits(a[4]), bits(b[4][:, ::-1])) and np.array_equal(a[5], b[5][:, ::-1])
    finally:
        ex.close()


# ---- slabs ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("method", [1, 2])
def test_slabs_change_nothing(monkeypatch, method):
    nc, nt = 33, 31
    strata = np.arange(nc + nt) % 3
    rng = np.random.default_rng([7700, method])
    rows = make_rows(rng, nc + nt)
    sets, signs = make_family(rng)                                            # 8 valid sets
    tables = stratum_tables(nc, strata, 14)
    K = 520
    ex = open_context(method, nc, nt, K, seed=8, strata=strata)
    try:
        whole, ref = run_and_compare(ex, method, nc, nt, sets, rows, signs, strata, tables, K, 8, "one slab")
        assert ex.strata_launches() == 2 + 3 + 3
        W32p, Kpad = 8 * ((ex.width_ul + 3) // 4), 2048                       # device rows are padded to four words, the masks to 2,048 permutations
        set_bytes = 3 * method * W32p * 4 + Kpad * 8
        for env, value, slabs in [("GCRE_STRATA_SLAB_SETS", "1", 8), ("GCRE_STRATA_SLAB_SETS", "3", 3), ("GCRE_STRATA_SLAB_SETS", "8", 1),
                                  ("GCRE_STRATA_MAX_MB", repr(3 * set_bytes / 1048576.0), 3),
                                  # the smallest bound a 512-permutation tile of null_scores over the 9 sets admits: two sets fit
                                  ("GCRE_STRATA_MAX_MB", repr(9 * 512 * 8 / 1048576.0), 4)]:
            monkeypatch.setenv(env, value)
            before = ex.strata_launches()
            got = ex.strata_tests(sets, rows, signs, strata=strata, tables=tables, family=True, null=True, terms=True)
            monkeypatch.delenv(env)
            assert ex.strata_launches() - before == 2 + 3 + 3 * slabs, (env, value)
            assert_equal_reference(got, ref, f"{env}={value}")
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:2], whole[:2]))
    finally:
        ex.close()


# ---- tables with special values, and tables smaller than their stratum ----------------------------------------------------


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("kind,variant", [("nonfinite", 0), ("nonfinite", 2), ("zeros", 0), ("huge", 0), ("huge", 1), ("tiny", 0)])
def test_special_tables(method, kind, variant):
    nc, nt = 33, 31
    strata = np.arange(nc + nt) % 2
    rng = np.random.default_rng([7800, method, variant])
    rows = make_rows(rng, nc + nt)
    sets, signs = make_family(rng)
    tables = [special_table(kind, int((strata[:nc] == s).sum()), int((strata[nc:] == s).sum()), 30 + s, variant) for s in (0, 1)]
    K = 300
    ex = open_context(method, nc, nt, K, seed=10, strata=strata)
    try:
        got, ref = run_and_compare(ex, method, nc, nt, sets, rows, signs, strata, tables, K, 10, f"{kind} {variant}")
        if kind == "nonfinite":
            assert np.isnan(ref["null_scores"][0]).any() or np.isnan(ref["null_scores"][2]).any() or np.isinf(ref["null_scores"]).any()
        # smaller than the stratum: one row and one column, a quarter, one row short
        small = [tables[0][:1, :1], tables[1][:5, :9]]
        got, ref = run_and_compare(ex, method, nc, nt, sets, rows, signs, strata, small, K, 10, f"{kind} {variant} small")
        if method == 1:
            assert (ref["terms"] == -1.0).any()
        short = [tables[0][:-1], tables[1][:, :-1]]
        run_and_compare(ex, method, nc, nt, sets, rows, signs, strata, short, K, 10, f"{kind} {variant} short")
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_family_max_folds_nan_and_negatives(method):
    nc, nt = 31, 2
    strata = np.arange(nc + nt) % 2
    rng = np.random.default_rng([7900, method])
    rows = make_rows(rng, nc + nt)
    sets = [[2], [3], [4, 5]]
    signs = [[1], [-1], [1, -1]]
    K = 513
    ex = open_context(method, nc, nt, K, seed=12, strata=strata)
    try:
        neg = [-np.abs(t) - 1.0 for t in stratum_tables(nc, strata, 16, 0.0)]    # every sum negative: the maxima stay +0
        got, ref = run_and_compare(ex, method, nc, nt, sets, rows, signs, strata, neg, K, 12, "negative")
        assert (got[2].view(np.uint64) == 0).all() and (ref["null_scores"] < 0).all()
        mixed = stratum_tables(nc, strata, 18, 0.3)
        mixed[0][::4, :] = np.nan                                             # every fourth count of case carriers in stratum 0
        mixed[1][0, 0] = -0.0
        got, ref = run_and_compare(ex, method, nc, nt, sets, rows, signs, strata, mixed, K, 12, "mixed")
        assert np.isnan(ref["null_scores"]).any() and (ref["null_scores"] < 0).any() and (ref["family_max"] > 0).any() and not np.isnan(got[2]).any()
        assert (np.signbit(got[2]) == False).all()                            # noqa: E712  (+0, never -0)
    finally:
        ex.close()


# ---- the masks must keep the strata ---------------------------------------------------------------------------------------


def _raw_call(ex, sets, rows, signs, n, strata="default", n_strata=None, tables="default", K=0, cap=None, null=()):
    """gcre_score_sets_strata through ctypes on arrays filled with a pattern: (return code, the arrays, *n_out)."""
    lib = api._strata_lib()
    inp, keep = api._set_input(sets, rows, signs, n)
    S = len(sets)
    st = np.ascontiguousarray((np.arange(n) % 2) if isinstance(strata, str) else strata, dtype=np.int32) if strata is not None else None
    NS = (int(st.max()) + 1 if st is not None else 2) if n_strata is None else n_strata
    tabs = [np.ones((3, 3)) for _ in range(max(NS, 0))] if isinstance(tables, str) else tables
    m = max(len(tabs), 1) if tabs is not None else 1
    nrow = np.array([t.shape[0] for t in tabs] + [0] * (m - len(tabs)), np.int32) if tabs is not None else np.ones(1, np.int32)
    ncol = np.array([t.shape[1] for t in tabs] + [0] * (m - len(tabs)), np.int32) if tabs is not None else np.ones(1, np.int32)
    toff = np.concatenate([[0], np.cumsum(nrow.astype(np.int64) * ncol)[:-1]]).astype(np.int64)
    flat = np.ascontiguousarray(np.concatenate([t.reshape(-1) for t in tabs] + [np.zeros(1)])) if tabs is not None else None
    P64 = 0x5a5a5a5a5a5a5a5a
    out = np.full(max(S, 1), 0x5a, dtype=np.uint8).repeat(api.SET_SCORE.itemsize).view(api.SET_SCORE)
    px = np.full(max(S, 1), 0x5a, dtype=np.uint8).repeat(api.STRATA_SCORE.itemsize).view(api.STRATA_SCORE)
    trm = np.full((max(S, 1), max(NS, 1)), P64, np.uint64)
    cnt = np.full((max(S, 1), max(NS, 1), 4), 0x5a5a5a5a, np.int32)
    nul = np.full((max(S, 1), max(K, 1)), P64, np.uint64)
    fam = np.full(max(K, 1), P64, np.uint64)
    n_out = ctypes.c_int64(-7)
    p = lambda name, a: None if name in null or a is None else api._ptr(a)
    rc = lib.gcre_score_sets_strata(ex._h, ctypes.byref(inp), p("stratum", st), NS, p("tables", flat), p("nrow", nrow), p("ncol", ncol),
                                    p("tab_off", toff), api._ptr(out), len(out) if cap is None else cap, ctypes.byref(n_out),
                                    p("px_out", px), p("terms", trm), p("counts", cnt), p("null_scores", nul), p("family_max", fam))
    del keep
    return rc, (out, px, trm, cnt, nul, fam), n_out.value


def _untouched(arrays, skip=()):
    names = ("out", "px", "terms", "counts", "null_scores", "family_max")
    return all((a.view(np.uint8) == 0x5a).all() for k, a in zip(names, arrays) if k not in skip)


@pytest.mark.parametrize("method", [1, 2])
def test_masks_that_do_not_keep_the_strata_are_refused(method):
    nc, nt = 20, 25
    n = nc + nt
    strata = np.arange(n) % 2
    K = 64
    rng = np.random.default_rng([8000, method])
    rows = make_rows(rng, n)[:40]
    sets, signs = [[2, 3], [4, -1], [5, 6, 7]], [[1, -1], [1, 1], [-1, 1, 1]]
    tables = stratum_tables(nc, strata, 20)
    want = [int((strata[:nc] == s).sum()) for s in (0, 1)]
    for how, drawn in (("without strata", None), ("with other strata", np.arange(n) % 3)):
        seed = 31
        masks = report.permutation_masks(nc, nt, K, seed, drawn)
        broken = sum(int((masks[:, strata == s].sum(axis=1) != want[s]).sum()) for s in (0, 1))
        assert broken > 0, how                                                # the CPU says so before the device is asked
        ex = open_context(method, nc, nt, K)
        try:
            ex.generate_permutations(seed, drawn)
            plain = ex.score_sets(sets, rows, signs)
            others = other_counters(ex)
            rc, arrays, n_out = _raw_call(ex, sets, rows, signs, n, strata=strata, tables=tables, K=K)
            msg = ex._lib.gcre_last_error(ex._h)
            assert rc == api.GCRE_ERR_ARG and b"generate_permutations(seed, strata)" in msg and f"{broken} (stratum, permutation)".encode() in msg
            out, px, trm, cnt, nul, fam = arrays
            assert n_out == 3 and out.tobytes() == plain.tobytes()            # gcre_score_sets' records
            assert np.isnan(px["score"]).all() and px["n_ge"].tolist() == [0, -1, 0]
            assert np.isnan(trm.view(np.float64)).all() and (cnt == 0).all() and np.isnan(nul.view(np.float64)).all()
            assert (fam == 0).all()
            assert ex.strata_launches() == 2 and other_counters(ex) == others  # the indicator rows and the check, nothing behind them
            with pytest.raises(api.GcreError, match="do not keep the cases of the stratum"):
                ex.strata_tests(sets, rows, signs, strata=strata, tables=tables)
            # the same context with masks that keep them: accepted
            ex.generate_permutations(seed, strata)
            run_and_compare(ex, method, nc, nt, sets, rows, signs, strata, tables, K, seed, how)
        finally:
            ex.close()


def test_refusals_launch_nothing_and_write_nothing(monkeypatch):
    nc, nt = 20, 25
    n = nc + nt
    rng = np.random.default_rng(8100)
    rows = make_rows(rng, n)[:40]
    VT = small_table(nc, nt, 1)
    sets, signs = [[2, 3], [4], [5, 6, 7]], [[1, -1], [1], [-1, 1, 1]]
    fresh = api.JoinExec(2, nc, nt, 0)
    try:
        rc, arrays, _ = _raw_call(fresh, sets, rows, signs, n)
        assert rc == api.GCRE_ERR_ASSERT and b"value table" in fresh._lib.gcre_last_error(fresh._h) and _untouched(arrays)
        assert fresh.strata_launches() == 0
    finally:
        fresh.close()
    masked = api.JoinExec(2, nc, nt, 100)                       # permutations asked for, none set: what score_sets refuses
    try:
        masked.set_value_table(VT)
        rc, arrays, _ = _raw_call(masked, sets, rows, signs, n, K=100)
        assert rc == api.GCRE_ERR_ASSERT and b"permutation masks" in masked._lib.gcre_last_error(masked._h) and _untouched(arrays)
        assert masked.strata_launches() == 0
    finally:
        masked.close()
    K = 30
    ex = open_context(2, nc, nt, K, seed=1, strata=np.arange(n) % 2, VT=VT)
    try:
        others = other_counters(ex)
        two = [np.ones((3, 3)), np.ones((2, 4))]
        refused = [
            (dict(sets=[[2], []]), api.GCRE_ERR_ARG, b"has no members", 0),
            (dict(sets=[[2, 3]], signs=[[1, 0]]), api.GCRE_ERR_ARG, b"neither", 0),
            (dict(sets=[[2], [3, 40]]), api.GCRE_ERR_RANGE, b"out of range", 0),
            (dict(cap=2), api.GCRE_ERR_RANGE, b"room for 2", 3),
            (dict(null=("px_out",)), api.GCRE_ERR_ARG, b"NULL argument (px_out)", 3),
            (dict(strata=None), api.GCRE_ERR_ARG, b"NULL argument (stratum)", 3),
            (dict(n_strata=0, tables=two), api.GCRE_ERR_ARG, b"n_strata = 0 outside 1 .. GCRE_STRATA_MAX = 16", 3),
            (dict(n_strata=17, tables=[np.ones((1, 1))] * 17), api.GCRE_ERR_ARG, b"n_strata = 17 outside 1 .. GCRE_STRATA_MAX = 16", 3),
            (dict(null=("tables",)), api.GCRE_ERR_ARG, b"NULL argument (tables, nrow, ncol or tab_off)", 3),
            (dict(null=("nrow",)), api.GCRE_ERR_ARG, b"NULL argument (tables, nrow, ncol or tab_off)", 3),
            (dict(null=("ncol",)), api.GCRE_ERR_ARG, b"NULL argument (tables, nrow, ncol or tab_off)", 3),
            (dict(null=("tab_off",)), api.GCRE_ERR_ARG, b"NULL argument (tables, nrow, ncol or tab_off)", 3),
            (dict(tables=[np.ones((3, 3)), np.ones((0, 4))]), api.GCRE_ERR_ARG, b"the table of stratum 1 must have at least one row and one column, not 0 x 4", 3),
            (dict(tables=[np.ones((3, 0)), np.ones((2, 4))]), api.GCRE_ERR_ARG, b"the table of stratum 0 must have at least one row and one column, not 3 x 0", 3),
            (dict(strata=np.arange(n) % 3, n_strata=2, tables=two), api.GCRE_ERR_RANGE, b"stratum id out of range", 3),
            (dict(strata=(np.arange(n) % 2) - 1, n_strata=2, tables=two), api.GCRE_ERR_RANGE, b"stratum id out of range", 3),
        ]
        for kw, code, msg, n_out in refused:
            kw = dict(kw)
            own = "sets" in kw
            rc, arrays, got_n = _raw_call(ex, kw.pop("sets", sets), rows, kw.pop("signs", None if own else signs), n, K=K, **kw)
            assert rc == code and msg in ex._lib.gcre_last_error(ex._h), (kw, rc, ex._lib.gcre_last_error(ex._h))
            assert _untouched(arrays) and got_n == n_out, kw
        rc, arrays, _ = _raw_call(ex, sets, np.zeros((40, n + 1), np.int8), signs, n + 1, K=K)
        assert rc == api.GCRE_ERR_ARG and _untouched(arrays)
        # one 512-permutation tile of null_scores: 3 sets x 512 x 8 bytes = 12,288 bytes
        monkeypatch.setenv("GCRE_STRATA_MAX_MB", repr(12287 / 1048576.0))
        rc, arrays, _ = _raw_call(ex, sets, rows, signs, n, K=K)
        assert rc == api.GCRE_ERR_ARG and b"GCRE_STRATA_MAX_MB" in ex._lib.gcre_last_error(ex._h) and _untouched(arrays)
        assert ex.strata_launches() == 0 and other_counters(ex) == others
        assert _raw_call(ex, sets, rows, signs, n, K=K, null=("null_scores",))[0] == api.GCRE_OK     # not asked without the matrix
        monkeypatch.setenv("GCRE_STRATA_MAX_MB", repr(12288 / 1048576.0))      # exactly one tile: accepted, a set per slab
        tables = stratum_tables(nc, np.arange(n) % 2, 22)
        before = ex.strata_launches()
        rc, arrays, got_n = _raw_call(ex, sets, rows, signs, n, tables=tables, K=K)
        assert rc == api.GCRE_OK and got_n == 3 and ex.strata_launches() - before == 2 + 2 + 3 * 3 and not _untouched(arrays)
        monkeypatch.delenv("GCRE_STRATA_MAX_MB")
        ref = report.strata_reference(sets, rows, signs, nc, np.arange(n) % 2, tables, report.permutation_masks(nc, nt, K, 1, np.arange(n) % 2), 2)
        out, px, trm, cnt, nul, fam = arrays
        assert np.array_equal(bits(px["score"]), bits(ref["score"])) and np.array_equal(px["n_ge"], ref["n_ge"])
        assert np.array_equal(bits(trm.view(np.float64)), bits(ref["terms"])) and np.array_equal(cnt, ref["counts"])
        assert np.array_equal(bits(nul.view(np.float64)), bits(ref["null_scores"])) and np.array_equal(fam, ref["family_max"].view(np.uint64))
        # every optional output may be left out; the limits themselves pass
        assert _raw_call(ex, sets, rows, signs, n, K=K, null=("terms", "counts", "null_scores", "family_max"))[0] == api.GCRE_OK
        sixteen = (np.arange(n) * 7) % 16
        ex.generate_permutations(1, sixteen)
        assert _raw_call(ex, sets, rows, signs, n, K=K, strata=sixteen, tables=[np.ones((1, 1))] * 16)[0] == api.GCRE_OK
        assert other_counters(ex) == others
    finally:
        ex.close()


# ---- contexts ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("method", [1, 2])
def test_a_context_without_permutations(method):
    """iterations = 0: the observed side is still made -- score, terms, counts -- and n_ge is 0 (-1 for an NA member)."""
    nc, nt = 33, 31
    strata = np.arange(nc + nt) % 5
    rng = np.random.default_rng([8200, method])
    rows = make_rows(rng, nc + nt)
    sets, signs = make_family(rng)
    tables = stratum_tables(nc, strata, 24)
    ex = open_context(method, nc, nt, 0)
    try:
        others = other_counters(ex)
        got, ref = run_and_compare(ex, method, nc, nt, sets, rows, signs, strata, tables, 0, 0, "no permutations")
        rec, sr, fam, nul, trm, cnt = got
        assert fam.shape == (0,) and nul.shape == (len(sets), 0)
        assert sr["n_ge"].tolist() == [0, 0, 0, 0, -1, 0, 0, 0, 0] and not np.isnan(sr["score"][rec["valid"] != 0]).any()
        assert ex.strata_launches() == 1 + 5 + 2                              # indicator rows, tables, rows + observed: no check, no null
        assert rec.tobytes() == ex.score_sets(sets, rows, signs).tobytes() and other_counters(ex) == others
    finally:
        ex.close()


# ---- the report ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("signed", [False, True])
def test_score_paths_stratified(signed):
    method = 2 if signed else 1
    nc, nt = 40, 50
    n = nc + nt
    rng = np.random.default_rng([8300, method])
    genes = [f"G{i}" for i in range(30)]
    data = (rng.random((30, n)) < rng.uniform(0.1, 0.5, size=(30, 1))).astype(np.int32)
    strata = np.where(np.arange(n) % 3 == 0, 12, 4)
    paths = ["G1 (+) -> G2 (-) -> G3 (+)", "G4 (+)", "G5 (-) -> NA (+)", ["G6", "G7", "G8", "G9"], "G10 (-) -> G11 (-)"]
    K = 150
    kw = dict(signed=signed, threshold=1.0, n_permutations=K, strata=strata, seed=5)
    base = report.score_paths(paths, genes, data, nc, nt, **kw)
    again = report.score_paths(paths, genes, data, nc, nt, stratified=False, **kw)
    assert list(base.columns) == report.SCORE_PATHS_COLUMNS and base.equals(again)
    df = report.score_paths(paths, genes, data, nc, nt, stratified=True, **kw)
    extra = report.STRATIFIED_COLUMNS + [f"{c}.{i}" for i in (4, 12) for c in report.STRATUM_COLUMNS]
    assert list(df.columns) == report.SCORE_PATHS_COLUMNS + extra and df[report.SCORE_PATHS_COLUMNS].equals(base)
    # the same numbers from the reference alone
    g2, d2 = report.preprocess_table(genes, data, 1.0, nc, nt)
    names, rows, signs = report.parse_sets(paths, g2)
    ids, inv = np.unique(strata, return_inverse=True)
    tables = [api.values_table(int((inv[:nc] == s).sum()), int((inv[nc:] == s).sum())) for s in range(len(ids))]
    ref = report.strata_reference(rows, d2, signs, nc, strata, tables, report.permutation_masks(nc, nt, K, 5, inv), method)
    valid = ref["n_ge"] >= 0
    want = report.stratified_columns(ref, valid, ref["family_max"], ref["terms"], ref["counts"], ids, K)
    for c in extra:
        np.testing.assert_array_equal(bits(df[c].to_numpy()), bits(want[c]), err_msg=c)
    assert np.isnan(df["StratifiedScores"][2]) and np.isnan(df["Score.12"][2]) and not np.isnan(df["StratifiedPvalues"][0])
    assert (df["Cases.4"] + df["Cases.12"])[valid].tolist() == df["Cases"][valid].tolist()
    with pytest.raises(ValueError, match="stratified=True needs strata"):
        report.score_paths(paths, genes, data, nc, nt, signed=signed, threshold=1.0, n_permutations=K, stratified=True)


# ---- a seeded loop -------------------------------------------------------------------------------------------------------------


def test_seeded_fuzz(monkeypatch):
    """GCRE_STRATA_FUZZ_CASES random calls (default 3; a longer run is summarised in profiles/strata_fuzz.txt): cohort, strata,
    tables, sets, permutations and slab knobs drawn from the case's seed, every output against the reference."""
    cases = int(os.environ.get("GCRE_STRATA_FUZZ_CASES", "3"))
    base = int(os.environ.get("GCRE_STRATA_FUZZ_SEED", "0"))
    failures = []
    for case in range(base, base + cases):
        rng = np.random.default_rng([8400, case])
        method = int(rng.integers(1, 3))
        nc, nt = int(rng.integers(1, 200)), int(rng.integers(1, 200))
        n = nc + nt
        NS = int(rng.integers(1, 17))
        strata = rng.integers(0, NS, n) if rng.random() < 0.7 else np.sort(rng.integers(0, NS, n))
        K = int(rng.choice([0, 1, 37, 512, 700]))
        n_rows = int(rng.integers(3, 40))
        rows = make_rows(rng, n, n_rows)
        sets = [rng.integers(-1 if rng.random() < 0.1 else 0, n_rows, int(rng.integers(1, 8))).tolist() for _ in range(int(rng.integers(1, 12)))]
        signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets] if rng.random() < 0.8 else None
        tables = stratum_tables(nc, strata, case, float(rng.choice([0.0, 0.2])))
        if rng.random() < 0.3:
            tables[0] = tables[0][:max(1, tables[0].shape[0] // 2)]
        if rng.random() < 0.3:
            tables[-1][rng.random(tables[-1].shape) < 0.1] = rng.choice([np.nan, np.inf, -np.inf])
        if rng.random() < 0.5:
            monkeypatch.setenv("GCRE_STRATA_SLAB_SETS", str(int(rng.integers(1, 6))))
        ex = open_context(method, nc, nt, K, seed=case, strata=strata)
        try:
            run_and_compare(ex, method, nc, nt, sets, rows, signs, strata, tables, K, case, f"case {case}")
        except AssertionError as e:
            failures.append((case, str(e)[:300]))
        finally:
            ex.close()
            monkeypatch.delenv("GCRE_STRATA_SLAB_SETS", raising=False)
    print(f"strata fuzz: {cases} cases from {base}, {len(failures)} failures")
    assert not failures, failures
