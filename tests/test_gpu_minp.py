"""Westfall-Young min-P over a family of given sets on the device (gcre_score_sets_minp: k_minp_gather, k_family_null,
k_minp_rank, k_minp_scan).  Everything ``JoinExec.minp_tests(min_count=True, counts=True)`` returns is
compared as integers against ``report.minp_reference`` fed the null matrix that ``family_tests(null=True)`` reads back on the
same context (tests/test_gpu_family.py holds that matrix against a restatement of its own), and the records against
``score_sets``.  The shapes are the smallest at which each part can go wrong: partial tiles, more values than the rank
kernel sorts at a time, slabs that cut tie groups, rows that are one value throughout."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from geneticscre_amd import api, report
from helpers import small_table, special_table
from test_gpu_family import N_ROWS, make_rows, make_sets, open_context

pytestmark = pytest.mark.gpu

CHUNK = 16384   # kMinpChunk of csrc/gcre_kernels.h: the values of a row k_minp_rank sorts at a time
ONES = 0xFFFFFFFF


def reference(ex, sets, rows, signs):
    """(score_sets' records, minp_reference of the null matrix the family entry reads back, that matrix)."""
    rec, _, null = ex.family_tests(sets, rows, signs, null=True)
    return rec, report.minp_reference(rec["score"], rec["valid"], null), null


def assert_minp(got, ref, what=""):
    rec, mp, mc, cn = got
    assert mp.dtype == api.MINP_SCORE and mc.dtype == np.uint32 and cn.dtype == np.uint32
    np.testing.assert_array_equal(rec["n_ge"], ref["n_ge"], err_msg=f"{what} n_ge")
    np.testing.assert_array_equal(cn, ref["counts"], err_msg=f"{what} counts")
    np.testing.assert_array_equal(mc, ref["min_count"], err_msg=f"{what} min_count")
    for f in ("n_le_minp", "n_le_stepdown"):
        np.testing.assert_array_equal(mp[f], ref[f], err_msg=f"{what} {f}")


def check_context(ex, sets, rows, signs, what=""):
    """One family on one context: against the reference, against score_sets, and the consequences of the definitions."""
    rec0, ref, null = reference(ex, sets, rows, signs)
    got = ex.minp_tests(sets, rows, signs, min_count=True, counts=True)
    assert_minp(got, ref, what)
    assert got[0].tobytes() == rec0.tobytes() == ex.score_sets(sets, rows, signs).tobytes(), what    # identical records
    bare = ex.minp_tests(sets, rows, signs)                     # without the optional arrays: the same records
    assert len(bare) == 2 and bare[0].tobytes() == got[0].tobytes() and bare[1].tobytes() == got[1].tobytes(), what
    rec, mp, mc, cn = got
    ok = (rec["valid"] != 0) & ~np.isnan(rec["score"])
    c = rec["n_ge"]
    assert ((cn <= c[:, None]).sum(axis=1)[ok] == c[ok]).all(), what
    assert (c[ok] <= mp["n_le_stepdown"][ok]).all() and (mp["n_le_stepdown"][ok] <= mp["n_le_minp"][ok]).all(), what
    if ok.any():
        low = ok & (c == c[ok].min())
        assert (mp["n_le_stepdown"][low] == mp["n_le_minp"][low]).all(), what
    return got, ref, null


# permutations x patients, the family sizes dealt over them so that every size meets every cohort once per method
KS, NS, VS = (1, 100, 512, 513, 700, 1300), (2, 33, 70, 200), (1, 9, 17, 37)
SHAPES = [(K, n, VS[(i + j) % 4]) for i, K in enumerate(KS) for j, n in enumerate(NS)]


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("K,n,V", SHAPES)
def test_minp_against_the_reference(method, K, n, V):
    i = SHAPES.index((K, n, V))
    rng = np.random.default_rng(3100 + 100 * method + i)
    nc = max(1, n // 2 - 1)
    nt = n - nc
    rows = make_rows(rng, n)
    sets, signs = make_sets(rng, V)                              # V valid sets and one with an NA member
    VT = small_table(n, n, i)
    VT[rng.random(VT.shape) < 0.05] *= -1                        # negatives fold as 0 in the null
    ex = open_context(method, nc, nt, K, VT, 140 + i)
    try:
        before, fam_before = ex.minp_launches(), ex.family_launches()
        (rec, mp, mc, cn), ref, null = check_context(ex, sets, rows, signs, f"K={K} n={n} V={V}")
        assert ex.minp_launches() == before + 2 * 4              # two calls of one slab: gather, null, rank, scan
        assert ex.family_launches() == fam_before + 3            # the reference's one call, nothing of ours
        assert (cn[0] == K).all()                                # the set of non-carriers: one value throughout
        na = min(2, V)
        assert rec["valid"][na] == 0 and tuple(mp[na]) == (-1, -1) and (cn[na] == ONES).all()
        if V >= 9:
            tie = [5, 6, 9]                                      # the duplicates, behind the inserted NA set
            assert len({int(c) for c in rec["n_ge"][tie]}) == 1
            assert len({tuple(mp[s]) for s in tie}) == 1
        if V == 1:
            assert mp["n_le_minp"][0] == mp["n_le_stepdown"][0] == rec["n_ge"][0]
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_rows_longer_than_the_rank_kernel_sorts_at_a_time(method):
    """Two full chunks and 77 values.  At 33 patients a row holds at most 34 distinct values, so every chunk boundary falls
    inside runs of ties, and the null score 0 occurs: a chunk's padding counted as a value would show."""
    K, n, nc = 2 * CHUNK + 77, 33, 15
    nt = n - nc
    rng = np.random.default_rng(3300 + method)
    rows = make_rows(rng, n)
    sets, signs = make_sets(rng, 5)
    sets[4], signs[4] = list(sets[3]), list(signs[3])            # a tie (the NA set sits at 2)
    VT = small_table(n, n, 5)
    VT[rng.random(VT.shape) < 0.3] *= -1
    VT[0, 0] = 0.0                                               # the set of non-carriers: a row of zeros
    ex = open_context(method, nc, nt, K, VT, 151)
    try:
        (rec, mp, mc, cn), ref, null = check_context(ex, sets, rows, signs, f"K={K}")
        live = null[rec["valid"] != 0]
        assert (live == 0).any() and max(len(np.unique(r)) for r in live) <= n + 1
        assert cn[rec["valid"] != 0].max() <= K
    finally:
        ex.close()


def walk_order(rec):
    """The valid sets as the stage walks them: NaN scores first, then c descending, stable."""
    v = np.flatnonzero(rec["valid"] != 0)
    isnan = np.isnan(rec["score"][v])
    scored = v[~isnan]
    return np.concatenate([v[isnan], scored[np.argsort(-rec["n_ge"][scored], kind="stable")]])


@pytest.mark.parametrize("method", [1, 2])
def test_slabs_do_not_change_the_results(method, monkeypatch):
    """37 valid sets in slabs of 5 rows, by count and by bytes, and in one slab: equal, and equal to the reference.  Seven
    of the sets are one set: wherever that tie group stands in the walk, a slab boundary cuts it."""
    K, n, V = 1300, 70, 37
    nc, nt = 33, 37
    rng = np.random.default_rng(3400 + method)
    rows = make_rows(rng, n)
    sets, signs = make_sets(rng, V)
    for s in (12, 17, 21, 26, 30, 35):
        sets[s], signs[s] = list(sets[11]), list(signs[11])
    VT = small_table(n, n, 7)
    ex = open_context(method, nc, nt, K, VT, 161)
    try:
        monkeypatch.delenv("GCRE_MINP_SLAB_SETS", raising=False)
        monkeypatch.delenv("GCRE_MINP_MAX_MB", raising=False)
        whole, ref, null = check_context(ex, sets, rows, signs, "one slab")
        order = walk_order(whole[0])
        c = whole[0]["n_ge"][order]
        scored = ~np.isnan(whole[0]["score"][order])
        cuts = [b for b in range(5, len(order), 5) if scored[b - 1] and scored[b] and c[b - 1] == c[b]]
        assert cuts, "no tie group across a slab boundary"
        l0 = ex.minp_launches()
        monkeypatch.setenv("GCRE_MINP_SLAB_SETS", "5")
        slabs = ex.minp_tests(sets, rows, signs, min_count=True, counts=True)
        l1 = ex.minp_launches()
        assert l1 - l0 == 1 + 3 * 8                              # the gather, then eight slabs of null, rank, scan
        for a, b in zip(whole, slabs):
            assert a.tobytes() == b.tobytes()
        # the memory bound cuts the same slabs: a row is 3 tiles x 512 permutations x 8 bytes, and 5.5 fit
        monkeypatch.delenv("GCRE_MINP_SLAB_SETS")
        monkeypatch.setenv("GCRE_MINP_MAX_MB", repr(3 * 512 * 8 * 5.5 / 1048576.0))
        bound = ex.minp_tests(sets, rows, signs, min_count=True, counts=True)
        assert ex.minp_launches() - l1 == 1 + 3 * 8
        for a, b in zip(whole, bound):
            assert a.tobytes() == b.tobytes()
        monkeypatch.setenv("GCRE_MINP_SLAB_SETS", "1")           # both bounds: the smaller one holds
        single = ex.minp_tests(sets, rows, signs, min_count=True, counts=True)
        for a, b in zip(whole, single):
            assert a.tobytes() == b.tobytes()
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("kind,variant", [("zeros", 0), ("nonfinite", 0), ("nonfinite", 2)])
def test_special_scores(kind, variant, method):
    """Tables of signed zeros and of NaN and infinities, as tests/test_gpu_family.py builds them (a NaN observed score: first
    in the walk, in no D, 0 / 0)."""
    K, n, nc = 100, 70, 33
    nt = n - nc
    rng = np.random.default_rng(1800 + method)
    rows = make_rows(rng, n)
    sets, signs = make_sets(rng, 17)
    sets += [[r] for r in range(2, N_ROWS)]                 # every row alone: more cells of the table among the scores
    signs += [[1 if r % 2 else -1] for r in range(2, N_ROWS)]
    VT = special_table(kind, n, n, 3, variant)
    if kind == "zeros":
        VT[0, 0] = -0.0
    ex = open_context(method, nc, nt, K, VT, 71)
    try:
        (rec, mp, mc, cn), ref, null = check_context(ex, sets, rows, signs, f"{kind}{variant}")
        score = rec["score"][rec["valid"] != 0]
        if kind == "zeros":
            assert len({bool(np.signbit(z)) for z in score[score == 0.0]}) == 2, "no -0.0 / +0.0 among the observed scores"
        elif variant == 0:
            assert np.isnan(score).any(), "no NaN observed score"
            s = int(np.flatnonzero((rec["valid"] != 0) & np.isnan(rec["score"]))[0])
            assert tuple(mp[s]) == (0, 0) and (cn[s] != ONES).all()     # counted nowhere, but its row is in every minimum
    finally:
        ex.close()


def _raw_call(ex, sets, rows, signs, n, mp_null=False, cap=None):
    """gcre_score_sets_minp through ctypes on arrays filled with a pattern: (return code, the arrays)."""
    lib = api._minp_lib()
    inp, keep = api._set_input(sets, rows, signs, n)
    S = len(sets)
    out = np.full(max(S, 1), 0x5a, dtype=np.uint8).repeat(api.SET_SCORE.itemsize).view(api.SET_SCORE)
    mp = np.full(max(S, 1) * 2, 0x5a5a5a5a, dtype=np.int64).view(api.MINP_SCORE)
    mc = np.full(ex.iters, 0x5a5a5a5a, np.uint32)
    cn = np.full((S, ex.iters), 0x5a5a5a5a, np.uint32)
    n_out = ctypes.c_int64(0)
    rc = lib.gcre_score_sets_minp(ex._h, ctypes.byref(inp), api._ptr(out), len(out) if cap is None else cap, ctypes.byref(n_out),
                                  None if mp_null else api._ptr(mp), api._ptr(mc), api._ptr(cn))
    del keep
    return rc, (out, mp, mc, cn)


def _untouched(arrays):
    out, mp, mc, cn = arrays
    return (out.view(np.uint8) == 0x5a).all() and (mp.view(np.int64) == 0x5a5a5a5a).all() and (mc == 0x5a5a5a5a).all() and \
        (cn == 0x5a5a5a5a).all()


def test_refusals_launch_nothing_and_write_nothing(monkeypatch):
    nc, nt, K = 20, 25, 600
    n = nc + nt
    rng = np.random.default_rng(3600)
    rows = make_rows(rng, n)
    VT = small_table(n, n, 1)
    sets, signs = [[2, 3], [4], [5, 6, 7]], [[1, -1], [1], [-1, 1, 1]]
    monkeypatch.delenv("GCRE_MINP_SLAB_SETS", raising=False)
    monkeypatch.delenv("GCRE_MINP_MAX_MB", raising=False)
    fresh = api.JoinExec(2, nc, nt, K)
    try:
        assert fresh.minp_launches() == 0
        rc, arrays = _raw_call(fresh, sets, rows, signs, n)
        assert rc == api.GCRE_ERR_ASSERT and b"value table" in fresh._lib.gcre_last_error(fresh._h) and _untouched(arrays)
        fresh.set_value_table(VT)
        rc, arrays = _raw_call(fresh, sets, rows, signs, n)
        assert rc == api.GCRE_ERR_ASSERT and b"permutation masks" in fresh._lib.gcre_last_error(fresh._h) and _untouched(arrays)
        with pytest.raises(api.GcreError, match="permutation masks"):
            fresh.minp_tests(sets, rows, signs)
        assert fresh.minp_launches() == 0
    finally:
        fresh.close()
    ex = open_context(2, nc, nt, K, VT, 5)
    try:
        refused = [
            (dict(sets=[[2], []], signs=None), api.GCRE_ERR_ARG, b"has no members"),
            (dict(sets=[[2, 3]], signs=[[1, 0]]), api.GCRE_ERR_ARG, b"neither"),
            (dict(sets=[[2], [3, N_ROWS]], signs=None), api.GCRE_ERR_RANGE, b"out of range"),
            (dict(sets=sets, signs=signs, cap=2), api.GCRE_ERR_RANGE, b"room for 2"),
            (dict(sets=sets, signs=signs, mp_null=True), api.GCRE_ERR_ARG, b"mp_out"),
        ]
        for kw, code, msg in refused:
            rc, arrays = _raw_call(ex, kw["sets"], rows, kw["signs"], n, mp_null=kw.get("mp_null", False), cap=kw.get("cap"))
            assert rc == code and msg in ex._lib.gcre_last_error(ex._h), (kw, rc, ex._lib.gcre_last_error(ex._h))
            assert _untouched(arrays), kw
        rc, arrays = _raw_call(ex, sets, np.zeros((N_ROWS, n + 1), np.int8), signs, n + 1)
        assert rc == api.GCRE_ERR_ARG and _untouched(arrays)
        # one row above the limit: 2 tiles x 512 permutations x 8 bytes = 8,192 bytes
        monkeypatch.setenv("GCRE_MINP_MAX_MB", repr(8191 / 1048576.0))
        rc, arrays = _raw_call(ex, sets, rows, signs, n)
        assert rc == api.GCRE_ERR_ARG and b"GCRE_MINP_MAX_MB" in ex._lib.gcre_last_error(ex._h) and _untouched(arrays)
        with pytest.raises(api.GcreError, match="GCRE_MINP_MAX_MB"):
            ex.minp_tests(sets, rows, signs)
        assert ex.minp_launches() == 0 and ex.family_launches() == 0
        monkeypatch.setenv("GCRE_MINP_MAX_MB", repr(8192 / 1048576.0))            # exactly one row: three slabs
        rc, arrays = _raw_call(ex, sets, rows, signs, n)
        assert rc == api.GCRE_OK and ex.minp_launches() == 1 + 3 * 3 and not _untouched(arrays)
        monkeypatch.delenv("GCRE_MINP_MAX_MB")
        check_context(ex, sets, rows, signs, "after the refusals")
        # an empty family, and one without a valid set: nothing is launched
        before = ex.minp_launches()
        rec, mp, mc = ex.minp_tests([], rows, min_count=True)
        assert len(rec) == 0 and len(mp) == 0 and mc.shape == (K,) and (mc == ONES).all()
        rec, mp, mc, cn = ex.minp_tests([[2, -1]], rows, min_count=True, counts=True)
        assert rec["valid"].tolist() == [0] and mp.tolist() == [(-1, -1)] and (mc == ONES).all() and (cn == ONES).all()
        assert ex.minp_launches() == before
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_no_permutations(method):
    """iterations == 0: the records of score_sets, zeros for the valid sets, nothing of the stage launched."""
    nc, nt = 20, 25
    n = nc + nt
    rng = np.random.default_rng(3700)
    rows = make_rows(rng, n)
    sets, signs = make_sets(rng, 9)
    ex = open_context(method, nc, nt, 0, small_table(n, n, 2), 0)
    try:
        rec, mp, mc, cn = ex.minp_tests(sets, rows, signs, min_count=True, counts=True)
        assert rec.tobytes() == ex.score_sets(sets, rows, signs).tobytes()
        assert mc.shape == (0,) and cn.shape == (len(sets), 0)
        valid = rec["valid"] != 0
        assert mp[valid].tolist() == [(0, 0)] * int(valid.sum()) and mp[~valid].tolist() == [(-1, -1)]
        assert ex.minp_launches() == 0 and ex.family_launches() == 0
    finally:
        ex.close()


def test_the_launch_counters_are_apart():
    """A min-P call leaves family_launches where it was, and a family call minp_launches."""
    nc, nt, K = 20, 25, 300
    n = nc + nt
    rng = np.random.default_rng(3800)
    rows = make_rows(rng, n)
    sets, signs = make_sets(rng, 9)
    ex = open_context(1, nc, nt, K, small_table(n, n, 3), 7)
    try:
        ex.minp_tests(sets, rows, signs)
        assert (ex.minp_launches(), ex.family_launches()) == (4, 0)
        ex.family_tests(sets, rows, signs)
        assert (ex.minp_launches(), ex.family_launches()) == (4, 3)
        ex.minp_tests(sets, rows, signs, counts=True)
        assert (ex.minp_launches(), ex.family_launches()) == (8, 3)
    finally:
        ex.close()


@pytest.mark.parametrize("signed", [False, True])
def test_score_paths_minp(signed):
    """The columns score_paths appends are minp_columns of the reference; without ``minp`` the frame is the one it was."""
    nc, nt, K, G = 33, 37, 700, 40
    n = nc + nt
    rng = np.random.default_rng(3900 + signed)
    genes = [f"G{i}" for i in range(G)]
    data = (rng.random((G, n)) < 0.15).astype(np.int32)
    tags = ["(+)", "(-)"]
    paths = [" -> ".join(f"{genes[g]} {tags[int(rng.integers(0, 2))]}" for g in rng.choice(G, size=int(rng.integers(1, 5)), replace=False))
             for _ in range(28)]
    paths += [paths[3], "NOSUCHGENE (+) -> G1 (-)"]                  # a tie and an NA row: 30 paths
    kw = dict(signed=signed, threshold=0.9, n_permutations=K, seed=77)
    plain = report.score_paths(paths, genes, data, nc, nt, **kw)
    full = report.score_paths(paths, genes, data, nc, nt, minp=True, **kw)
    both = report.score_paths(paths, genes, data, nc, nt, family_inference=True, minp=True, **kw)
    assert list(plain.columns) == report.SCORE_PATHS_COLUMNS
    assert list(full.columns) == report.SCORE_PATHS_COLUMNS + report.MINP_COLUMNS
    assert list(both.columns) == report.SCORE_PATHS_COLUMNS + report.FAMILY_COLUMNS + report.MINP_COLUMNS
    assert plain.equals(report.score_paths(paths, genes, data, nc, nt, minp=False, **kw))
    for col in report.SCORE_PATHS_COLUMNS:
        assert plain[col].equals(full[col]) and plain[col].equals(both[col]), col
    fam = report.score_paths(paths, genes, data, nc, nt, family_inference=True, **kw)
    assert fam.equals(both[report.SCORE_PATHS_COLUMNS + report.FAMILY_COLUMNS])
    assert full[report.MINP_COLUMNS].equals(both[report.MINP_COLUMNS])
    # the reference: the same rows, table and masks on a context of our own
    method = 2 if signed else 1
    g2, d2 = report.preprocess_table(genes, data, 0.9, nc, nt)
    _, prow, psign = report.parse_sets(paths, g2)
    ex = api.JoinExec(method, nc, nt, K)
    try:
        ex.set_value_table(api.values_table(nc, nt))
        ex.generate_permutations(77, None)
        rec, ref, null = reference(ex, prow, np.asarray(d2), psign)
    finally:
        ex.close()
    cols = report.minp_columns(ref["n_ge"], rec["valid"], rec["score"], ref, K)
    for c in report.MINP_COLUMNS:
        np.testing.assert_array_equal(full[c].to_numpy(), cols[c], err_msg=c)
    assert np.isnan(full[report.MINP_COLUMNS].to_numpy()[-1]).all()                        # the NA row
    ok = rec["valid"] != 0
    assert (full["FamilyPvaluesMinPStepDown"][ok] <= full["FamilyPvaluesMinP"][ok]).all()
    assert (full["FamilyPvaluesMinPStepDown"][ok] >= full["NominalPvalues"][ok]).all()
    assert full["FamilyPvaluesMinPStepDown"].iat[3] == full["FamilyPvaluesMinPStepDown"].iat[28]     # the tie


# ---- seeded fuzz: a handful of cases by default, GCRE_MINP_FUZZ_CASES asks for a long run -------------------------------


def fuzz_case(case):
    rng = np.random.default_rng([3950, case])
    method = int(rng.integers(1, 3))
    n = int(rng.choice([2, 3, 31, 32, 33, 64, 65, 70, 129, 200, 260]))
    nc = int(rng.integers(1, n))
    nt = n - nc
    K = int(rng.choice([1, 2, 63, 64, 100, 511, 512, 513, 700, 1024, 1300, CHUNK - 1, CHUNK, CHUNK + 1]))
    V = int(rng.choice([1, 2, 7, 8, 9, 10, 11, 15, 16, 17, 33, 37, 64, 65, 90]))
    if K >= CHUNK - 1:
        V = min(V, 17)
    rows = make_rows(rng, n)
    sets, signs = make_sets(rng, V)
    kind = str(rng.choice(["small", "small", "zeros", "nonfinite", "ladder"]))
    VT = small_table(n, n, case) if kind == "small" else special_table(kind, n, n, case, int(rng.integers(0, 3)) if kind == "nonfinite" else 0)
    slab = int(rng.choice([0, 0, 1, 3, 64]))
    return method, nc, nt, K, sets, rows, signs, VT, slab, f"case {case}: method {method} n={n} K={K} V={V} {kind} slab={slab}"


def test_seeded_fuzz(monkeypatch):
    cases = int(os.environ.get("GCRE_MINP_FUZZ_CASES", "6"))
    monkeypatch.delenv("GCRE_MINP_MAX_MB", raising=False)
    for case in range(cases):
        method, nc, nt, K, sets, rows, signs, VT, slab, what = fuzz_case(case)
        if slab:
            monkeypatch.setenv("GCRE_MINP_SLAB_SETS", str(slab))
        else:
            monkeypatch.delenv("GCRE_MINP_SLAB_SETS", raising=False)
        ex = open_context(method, nc, nt, K, VT, 500 + case)
        try:
            check_context(ex, sets, rows, signs, what)
        finally:
            ex.close()
    print(f"minp fuzz: {cases} cases equal the reference")
