"""Split-half stability on the device (gcre_score_sets_subsample: k_subsample_masks, k_subsample_null).
Everything ``JoinExec.subsample_tests(scores=True)`` returns is compared exactly against ``report.subsample_reference`` on the
same tables -- the counts as integers, the scores as bit patterns -- and the records against ``score_sets``.  The shapes are
the smallest at which each part can go wrong: the dword that straddles n_cases at every position, more than one staged mask
chunk, draws around the 512-draw tile, sets around a block's tile, slabs by count and by bytes."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from geneticscre_amd import api, report
from helpers import small_table, special_table

pytestmark = pytest.mark.gpu

N_ROWS = 90
TILE = {1: 16, 2: 8}        # subsample_tile_sets(method): sets per block of k_subsample_null (k_set_null's)
PT = 512                    # draws per tile
ENV = ("GCRE_SUBSAMPLE_MAX_MB", "GCRE_SUBSAMPLE_SLAB_DRAWS")
COUNTERS = [("given", "gcre_given_launches"), ("family", "gcre_family_launches"), ("minp", "gcre_minp_launches"),
            ("compete", "gcre_compete_launches"), ("prefix", "gcre_prefix_launches"), ("overlap", "gcre_overlap_launches"),
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


def make_cuts(rng, S, J=3, top=20.0):
    cuts = np.sort(rng.random((S, J)) * top, axis=1)
    cuts[:, 0] = -np.inf
    return cuts


def open_context(method, nc, nt, VT, K=0, seed=1):
    ex = api.JoinExec(method, nc, nt, K)
    ex.set_value_table(VT)
    if K > 0:
        ex.generate_permutations(seed, None)
    return ex


def bits(a):
    """The bit patterns of doubles, every NaN as one pattern: the sign of the NaN that inf - inf gives is the adder's own."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.float64(np.nan), a).view(np.uint64)


def counts_of(scores_a, scores_b, cuts, valid):
    """n_a, n_b, n_both of score matrices [sets][draws] against cuts [sets][cuts]."""
    with np.errstate(invalid="ignore"):
        ga = scores_a[:, None, :] >= cuts[:, :, None]
        gb = scores_b[:, None, :] >= cuts[:, :, None] if scores_b is not None else None
    na = np.where(valid[:, None], ga.sum(axis=2), -1)
    if gb is None:
        return na, None, None
    return na, np.where(valid[:, None], gb.sum(axis=2), -1), np.where(valid[:, None], (ga & gb).sum(axis=2), -1)


def assert_equal_reference(got, ref, B, cuts, what=""):
    """(records, counts, scores_a, scores_b) of a call with B draws against a reference of B draws or more."""
    rec, counts, sa, sb = got
    valid = rec["valid"] != 0
    assert sa.dtype == np.float64 and sa.shape == (len(rec), B)
    np.testing.assert_array_equal(bits(sa), bits(ref["scores_a"][:, :B]), err_msg=f"{what} scores_a")
    half_b = ref["scores_b"] is not None
    if half_b:
        np.testing.assert_array_equal(bits(sb), bits(ref["scores_b"][:, :B]), err_msg=f"{what} scores_b")
    else:
        assert sb is None and counts["n_b"] is None and counts["n_both"] is None
    if cuts is not None:
        ct = np.asarray(cuts, np.float64)
        ct = np.broadcast_to(ct, (len(rec), len(ct))) if ct.ndim == 1 else ct
        want = counts_of(ref["scores_a"][:, :B], ref["scores_b"][:, :B] if half_b else None, ct, valid)
        for k, w in zip(("n_a", "n_b", "n_both"), want):
            if w is not None:
                assert counts[k].dtype == np.int64
                np.testing.assert_array_equal(counts[k], w, err_msg=f"{what} {k}")


def run_and_compare(ex, method, nc, sets, rows, signs, ma, mt, B, seed, TA, TB, cuts, what=""):
    """One call with the matrices against the reference of the same arguments: (what the call returned, the reference)."""
    ref =report.subsample_reference(sets, rows, signs, nc, ma, mt, B, seed, TA, TB, cuts, method)
    got = ex.subsample_tests(sets, rows, signs, m_cases=ma, m_ctrls=mt, draws=B, seed=seed, table_a=TA, table_b=TB, cuts=cuts, scores=True)
    assert_equal_reference(got, ref, B, cuts, what)
    if cuts is not None and TB is not False:
        for k in ("n_a", "n_b", "n_both"):
            np.testing.assert_array_equal(got[1][k], ref[k], err_msg=f"{what} {k} (reference)")
    return got, ref


# ---- the dword that straddles n_cases ---------------------------------------------------------------------------------


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("cohort", [(1, 1), (31, 2), (32, 32), (33, 31), (64, 1), (65, 135)])
def test_boundary_dword(method, cohort):
    nc, nt = cohort
    n = nc + nt
    rng = np.random.default_rng([5100, method, nc, nt])
    rows = make_rows(rng, n)
    sets, signs = make_family(rng)
    cuts = make_cuts(rng, len(sets))
    VT = small_table(nc, nt, 3)
    ex = open_context(method, nc, nt, VT)
    try:
        plain = ex.score_sets(sets, rows, signs)
        others = other_counters(ex)
        for i, (ma, mt) in enumerate([(nc // 2, nt // 2), (0, 0), (nc, nt), (1, nt)]):
            TA, TB = small_table(ma, mt, 10 + i), small_table(nc - ma, nt - mt, 20 + i)
            TA[rng.random(TA.shape) < 0.1] *= -1
            got, ref = run_and_compare(ex, method, nc, sets, rows, signs, ma, mt, 100, 7 + i, TA, TB, cuts, f"{cohort} m=({ma}, {mt})")
            rec, counts, sa, sb = got
            assert rec.tobytes() == plain.tobytes()                              # the records of score_sets
            assert ex.subsample_launches() == 4 * (i + 1)                        # two tables, one slab
            assert rec["valid"][4] == 0 and (counts["n_a"][4] == -1).all() and (counts["n_both"][4] == -1).all()
            assert np.isnan(sa[4]).all() and np.isnan(sb[4]).all()
            assert (counts["n_a"][rec["valid"] != 0, 0] == 100).all()            # a cut of -inf: every draw, no padded one
        # the default halves and their default tables
        rec, counts = ex.subsample_tests(sets, rows, signs, draws=20, seed=3, cuts=[0.5])
        ref = report.subsample_reference(sets, rows, signs, nc, nc // 2, nt // 2, 20, 3, api.values_table(nc // 2, nt // 2),
                                         api.values_table(nc - nc // 2, nt - nt // 2), [0.5], method)
        for k in ("n_a", "n_b", "n_both"):
            np.testing.assert_array_equal(counts[k], ref[k])
        assert other_counters(ex) == others
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_many_chunks_and_a_far_boundary(method):
    """4,100 cases and 4,157 controls: 66 staged mask chunks, the last one padding only, and the straddling dword is word
    128, the first of chunk 32."""
    nc, nt = 4100, 4157
    n = nc + nt
    rng = np.random.default_rng(5200 + method)
    rows = (rng.random((40, n)) < rng.uniform(0.01, 0.3, size=(40, 1))).astype(np.int8)
    rows[:, nc - 40:nc + 40] |= (rng.random((40, 80)) < 0.5).astype(np.int8)
    sets = [[3], [4, 5, 6], rng.integers(0, 40, 9).tolist(), [7, -1]] + [rng.integers(0, 40, 2).tolist() for _ in range(15)]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    ma, mt = 2050, 2078
    TA, TB = small_table(ma, mt, 1), small_table(nc - ma, nt - mt, 2)
    cuts = make_cuts(rng, len(sets))
    ex = open_context(method, nc, nt, small_table(60, 60, 3))        # (the records are not what this test is about)
    try:
        got, _ = run_and_compare(ex, method, nc, sets, rows, signs, ma, mt, 40, 2, TA, TB, cuts, f"n={n}")
        assert len(np.unique(got[2][2])) > 20                    # the scores move with the draw
    finally:
        ex.close()


# ---- draws around the tile, sets around a block -------------------------------------------------------------------------


@pytest.mark.parametrize("method", [1, 2])
def test_draws_around_the_tile(method):
    nc, nt = 33, 40
    rng = np.random.default_rng(5300 + method)
    rows = make_rows(rng, nc + nt)
    sets, signs = make_family(rng)
    ma, mt = 16, 20
    TA, TB = small_table(ma, mt, 1), small_table(nc - ma, nt - mt, 2)
    cuts = make_cuts(rng, len(sets))
    ref = report.subsample_reference(sets, rows, signs, nc, ma, mt, 1025, 11, TA, TB, cuts, method)
    ex = open_context(method, nc, nt, small_table(nc, nt, 3))
    try:
        for B in (1, 511, 512, 513, 1025):
            got = ex.subsample_tests(sets, rows, signs, m_cases=ma, m_ctrls=mt, draws=B, seed=11, table_a=TA, table_b=TB, cuts=cuts, scores=True)
            assert_equal_reference(got, ref, B, cuts, f"B={B}")
            valid = got[0]["valid"] != 0
            assert (got[1]["n_a"][valid, 0] == B).all() and (got[1]["n_b"][valid, 0] == B).all() and (got[1]["n_both"][valid, 0] == B).all()
        bare = ex.subsample_tests(sets, rows, signs, m_cases=ma, m_ctrls=mt, draws=1025, seed=11, table_a=TA, table_b=TB, cuts=cuts)
        assert len(bare) == 2 and all(np.array_equal(bare[1][k], got[1][k]) for k in ("n_a", "n_b", "n_both"))
        other = ex.subsample_tests(sets, rows, signs, m_cases=ma, m_ctrls=mt, draws=513, seed=12, table_a=TA, table_b=TB, scores=True)
        assert not np.array_equal(bits(other[2]), bits(ref["scores_a"][:, :513]))       # another seed gives other draws
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_sets_around_a_block(method):
    nc, nt = 20, 45
    rng = np.random.default_rng(5400 + method)
    rows = make_rows(rng, nc + nt)
    ma, mt = 10, 22
    TA, TB = small_table(ma, mt, 1), small_table(nc - ma, nt - mt, 2)
    ex = open_context(method, nc, nt, small_table(nc, nt, 3))
    try:
        for S in (1, TILE[method], TILE[method] + 1, 3 * TILE[method] + 2):
            sets = [rng.integers(0, N_ROWS, int(rng.integers(1, 4))).tolist() for _ in range(S)]
            if S > 2:
                sets[1] = [3, -1]                               # an NA set inside the tile: the launched sets are one fewer
            signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
            run_and_compare(ex, method, nc, sets, rows, signs, ma, mt, 70, 5, TA, TB, make_cuts(rng, S), f"S={S}")
    finally:
        ex.close()


# ---- the two identities, complementarity -----------------------------------------------------------------------------------


@pytest.mark.parametrize("method", [1, 2])
def test_the_whole_cohort_reproduces_the_observed_score(method):
    nc, nt = 33, 31
    rng = np.random.default_rng(5500 + method)
    rows = make_rows(rng, nc + nt)
    sets, signs = make_family(rng)
    VT = small_table(nc, nt, 4)
    VT[2, 3] = np.nan
    empty = np.full((1, 1), 123.0)
    ex = open_context(method, nc, nt, VT)
    try:
        plain = ex.score_sets(sets, rows, signs)
        valid = plain["valid"] != 0
        obs = plain["score"]
        cut = np.where(np.isnan(obs), 0.0, obs)[:, None]
        # everybody in half A, scored on the context's table: A is the observed score, B the empty cohort's one cell
        rec, counts, sa, sb = ex.subsample_tests(sets, rows, signs, m_cases=nc, m_ctrls=nt, draws=40, seed=1, table_a=VT, table_b=empty,
                                                 cuts=cut, scores=True)
        assert (bits(sa[valid]) == bits(obs[valid])[:, None]).all()
        assert (counts["n_a"][valid, 0] == np.where(np.isnan(obs[valid]), 0, 40)).all()
        assert (sb[valid] == (123.0 if method == 1 else 246.0)).all()
        # nobody in half A: the complement is the cohort
        rec, counts, sa, sb = ex.subsample_tests(sets, rows, signs, m_cases=0, m_ctrls=0, draws=40, seed=1, table_a=empty, table_b=VT,
                                                 cuts=cut, scores=True)
        assert (bits(sb[valid]) == bits(obs[valid])[:, None]).all()
        assert (counts["n_b"][valid, 0] == np.where(np.isnan(obs[valid]), 0, 40)).all()
        assert (sa[valid] == (123.0 if method == 1 else 246.0)).all()
        assert rec.tobytes() == plain.tobytes()
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_half_b_is_half_a_of_the_complement(method):
    """scores_b equals what the definition gives half A on the complement masks with table_b -- stated here on the masks of
    ``report.subsample_masks``, not through the entry."""
    nc, nt = 37, 64
    n = nc + nt
    rng = np.random.default_rng(5600 + method)
    rows = make_rows(rng, n)
    sets, signs = make_family(rng)
    ma, mt = 11, 40
    TA, TB = small_table(ma, mt, 1), small_table(nc - ma, nt - mt, 2)
    comp = ~report.subsample_masks(nc, nt, ma, mt, 60, 9)
    assert (comp[:, :nc].sum(axis=1) == nc - ma).all() and (comp[:, nc:].sum(axis=1) == nt - mt).all()
    d = rows != 0
    case = np.arange(n) < nc
    ex = open_context(method, nc, nt, small_table(nc, nt, 3))
    try:
        rec, counts, sa, sb = ex.subsample_tests(sets, rows, signs, m_cases=ma, m_ctrls=mt, draws=60, seed=9, table_a=TA, table_b=TB, scores=True)
        for s, (m, sg) in enumerate(zip(sets, signs)):
            if min(m) < 0:
                continue
            neg = np.array([method == 2 and g == -1 for g in sg])
            P = d[np.asarray(m)[~neg]].any(axis=0) if (~neg).any() else np.zeros(n, bool)
            N = d[np.asarray(m)[neg]].any(axis=0) if neg.any() else np.zeros(n, bool)
            nb = n - ma - mt
            want = report._vt_cell(TB, nb, (comp & P & case).sum(axis=1), (comp & P & ~case).sum(axis=1))
            if method == 2:
                want = want + report._vt_cell(TB, nb, (comp & N & ~case).sum(axis=1), (comp & N & case).sum(axis=1))
            np.testing.assert_array_equal(bits(sb[s]), bits(want), err_msg=f"set {s}")
    finally:
        ex.close()


# ---- slabs ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("method", [1, 2])
def test_slabs_change_nothing(monkeypatch, method):
    nc, nt = 60, 69
    rng = np.random.default_rng(5700 + method)
    rows = make_rows(rng, nc + nt)
    sets, signs = make_family(rng)
    ma, mt = 30, 34
    TA, TB = small_table(ma, mt, 1), small_table(nc - ma, nt - mt, 2)
    cuts = make_cuts(rng, len(sets))
    B = 1300
    kw = dict(m_cases=ma, m_ctrls=mt, draws=B, seed=12, table_a=TA, table_b=TB, cuts=cuts)
    ex = open_context(method, nc, nt, small_table(nc, nt, 3))
    try:
        whole, _ = run_and_compare(ex, method, nc, sets, rows, signs, ma, mt, B, 12, TA, TB, cuts, "one slab")
        assert ex.subsample_launches() == 2 + 2

        def same(got):
            assert got[0].tobytes() == whole[0].tobytes()
            for k in ("n_a", "n_b", "n_both"):
                assert np.array_equal(got[1][k], whole[1][k]), k
            for x, y in zip(got[2:], whole[2:]):
                assert x.tobytes() == y.tobytes()

        for slab, n_slabs in ((1, 3), (512, 3), (1024, 2), (1535, 2), (4096, 1)):
            monkeypatch.setenv("GCRE_SUBSAMPLE_SLAB_DRAWS", str(slab))
            before = ex.subsample_launches()
            same(ex.subsample_tests(sets, rows, signs, scores=True, **kw))
            assert ex.subsample_launches() == before + 2 + 2 * n_slabs, slab
        monkeypatch.delenv("GCRE_SUBSAMPLE_SLAB_DRAWS")
        # by bytes: a tile of draws holds its masks (W32p dwords a draw) and two matrices of 8 bytes a set
        w32p = 2 * (((nc + nt + 63) // 64 + 3) // 4 * 4)          # 64-bit words of a row, padded to four: 8 dwords here
        assert w32p == 8
        tile = PT * (w32p * 4 + 2 * 8 * len(sets))
        monkeypatch.setenv("GCRE_SUBSAMPLE_MAX_MB", repr((2 * tile + 1) / 1048576.0))
        before = ex.subsample_launches()
        same(ex.subsample_tests(sets, rows, signs, scores=True, **kw))
        assert ex.subsample_launches() == before + 2 + 2 * 2      # two tiles a slab: three tiles are two slabs
        before = ex.subsample_launches()                          # without the matrices the same bound holds all three
        bare = ex.subsample_tests(sets, rows, signs, **kw)
        assert all(np.array_equal(bare[1][k], whole[1][k]) for k in ("n_a", "n_b", "n_both"))
        assert ex.subsample_launches() == before + 2 + 2
        monkeypatch.setenv("GCRE_SUBSAMPLE_MAX_MB", "0.000001")  # one tile at the least, without matrices
        before = ex.subsample_launches()
        bare = ex.subsample_tests(sets, rows, signs, **kw)
        assert all(np.array_equal(bare[1][k], whole[1][k]) for k in ("n_a", "n_b", "n_both"))
        assert ex.subsample_launches() == before + 2 + 2 * 3
    finally:
        ex.close()


# ---- cuts ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("method", [1, 2])
def test_cuts(method):
    nc, nt = 40, 33
    rng = np.random.default_rng(5800 + method)
    rows = make_rows(rng, nc + nt)
    sets, signs = make_family(rng)
    S = len(sets)
    ma, mt = 20, 16
    TA, TB = small_table(ma, mt, 1), small_table(nc - ma, nt - mt, 2)
    TA[rng.random(TA.shape) < 0.2] = np.nan                      # NaN scores against finite cuts never count
    TB[rng.random(TB.shape) < 0.2] = np.nan
    ex = open_context(method, nc, nt, small_table(nc, nt, 3))
    try:
        # no cuts: the matrices only
        got, ref = run_and_compare(ex, method, nc, sets, rows, signs, ma, mt, 90, 4, TA, TB, None, "no cuts")
        assert got[1]["n_a"].shape == (S, 0) and got[1]["n_both"].shape == (S, 0)
        assert np.isnan(got[2]).any() and np.isnan(got[3]).any()
        # eight cuts, every set its own, unsorted, with both infinities
        cuts = rng.random((S, 8)) * 20
        cuts[:, 2], cuts[:, 5] = np.inf, -np.inf
        got8, _ = run_and_compare(ex, method, nc, sets, rows, signs, ma, mt, 90, 4, TA, TB, cuts, "eight cuts")
        valid = got8[0]["valid"] != 0
        finite_a = (~np.isnan(ref["scores_a"])).sum(axis=1)
        assert (got8[1]["n_a"][valid, 5] == finite_a[valid]).all() and (got8[1]["n_a"][valid, 5] < 90).any()
        assert (got8[1]["n_a"][valid, 2] == (ref["scores_a"][valid] == np.inf).sum(axis=1)).all()
        # one list for every set
        one, _ = run_and_compare(ex, method, nc, sets, rows, signs, ma, mt, 90, 4, TA, TB, [3.0, 12.0], "one list")
        assert one[1]["n_a"].shape == (S, 2)
        # half A only: the same A side, no B outputs
        half, _ = run_and_compare(ex, method, nc, sets, rows, signs, ma, mt, 90, 4, TA, False, cuts, "half A only")
        assert np.array_equal(half[1]["n_a"], got8[1]["n_a"]) and half[2].tobytes() == got8[2].tobytes()
        assert ex.subsample_launches() == 3 * 4 + 3                                 # one table less
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("kind,variant", [("zeros", 0), ("nonfinite", 0), ("nonfinite", 1), ("nonfinite", 2), ("huge", 0), ("tiny", 0),
                                          ("undersized", 0)])
def test_special_tables(method, kind, variant):
    """NaN, infinities, signed zeros, huge and tiny values: a score is the table's own f64 value; a table smaller than the half
    cohort reads -1 where it has no cell."""
    nc, nt = 33, 37
    rng = np.random.default_rng(5900 + 10 * method + variant)
    rows = make_rows(rng, nc + nt)
    sets = [rng.integers(0, N_ROWS, size=int(k)).tolist() for k in rng.integers(1, 5, size=30)] + [[1], [0]]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    ma, mt = 16, 18
    if kind == "undersized":
        TA, TB = small_table(5, 7, 1), small_table(9, 4, 2)
    else:
        TA, TB = special_table(kind, ma, mt, 3, variant), special_table(kind, nc - ma, nt - mt, 4, variant)
    cuts = np.array([-np.inf, 0.0, 1.0])
    ex = open_context(method, nc, nt, small_table(nc, nt, 3))
    try:
        got, ref = run_and_compare(ex, method, nc, sets, rows, signs, ma, mt, 256, 3, TA, TB, cuts, f"{kind}{variant}")
        sa = got[2]
        if kind == "nonfinite":
            assert np.isnan(sa).any() or np.isnan(got[3]).any(), "no NaN score"
        if kind == "zeros":
            z = np.concatenate([sa[sa == 0.0], got[3][got[3] == 0.0]])
            assert len({bool(x) for x in np.signbit(z)}) == 2, "no -0.0 / +0.0 among the scores"
        if kind == "undersized":
            assert (sa < 0).any() and (got[3] < 0).any(), "no cell outside the table"      # (the tables' own cells are positive)
    finally:
        ex.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------


def _raw_call(ex, sets, rows, signs, n, m=(10, 12), draws=10, TA="default", TB="default", cuts="default", n_cut=None, cap=None,
              null=()):
    """gcre_score_sets_subsample through ctypes on arrays filled with a pattern: (return code, the arrays)."""
    lib = api._subsample_lib()
    inp, keep = api._set_input(sets, rows, signs, n)
    S = len(sets)
    B = max(int(draws), 0)
    ta = np.ones((max(m[0], 0) + 1, max(m[1], 0) + 1)) if isinstance(TA, str) else TA
    tb = np.ones((4, 4)) if isinstance(TB, str) else TB
    ct = np.tile([1.0, 2.0], (max(S, 1), 1)) if isinstance(cuts, str) else cuts
    J = (0 if ct is None else ct.shape[1]) if n_cut is None else n_cut
    out = np.full(max(S, 1), 0x5a, dtype=np.uint8).repeat(api.SET_SCORE.itemsize).view(api.SET_SCORE)
    cnt = [np.full((max(S, 1), max(J, 1)), 0x5a5a5a5a, np.int64) for _ in range(3)]
    sc = [np.full((max(S, 1), max(B, 1)), 0x5a5a5a5a5a5a5a5a, np.uint64) for _ in range(2)]
    n_out = ctypes.c_int64(0)
    p = lambda name, a: None if name in null else api._ptr(a)
    shape = lambda t, i: 0 if t is None else t.shape[i]
    rc = lib.gcre_score_sets_subsample(ex._h, ctypes.byref(inp), m[0], m[1], draws, 7, api._ptr(ta), shape(ta, 0), shape(ta, 1),
                                       api._ptr(tb), shape(tb, 0), shape(tb, 1), api._ptr(ct), J, api._ptr(out),
                                       len(out) if cap is None else cap, ctypes.byref(n_out), p("n_a", cnt[0]), p("n_b", cnt[1]),
                                       p("n_both", cnt[2]), p("scores_a", sc[0]), p("scores_b", sc[1]))
    del keep
    return rc, (out, cnt, sc), n_out.value


def _untouched(arrays):
    out, cnt, sc = arrays
    return (out.view(np.uint8) == 0x5a).all() and all((c == 0x5a5a5a5a).all() for c in cnt) and \
        all((s == 0x5a5a5a5a5a5a5a5a).all() for s in sc)


def test_refusals_launch_nothing_and_write_nothing(monkeypatch):
    nc, nt = 20, 25
    n = nc + nt
    rng = np.random.default_rng(6000)
    rows = make_rows(rng, n)[:40]
    VT = small_table(nc, nt, 1)
    sets, signs = [[2, 3], [4], [5, 6, 7]], [[1, -1], [1], [-1, 1, 1]]
    fresh = api.JoinExec(2, nc, nt, 0)
    try:
        rc, arrays, _ = _raw_call(fresh, sets, rows, signs, n)
        assert rc == api.GCRE_ERR_ASSERT and b"value table" in fresh._lib.gcre_last_error(fresh._h) and _untouched(arrays)
        assert fresh.subsample_launches() == 0
    finally:
        fresh.close()
    masked = api.JoinExec(2, nc, nt, 100)                       # permutations asked for, none set: what score_sets refuses
    try:
        masked.set_value_table(VT)
        rc, arrays, _ = _raw_call(masked, sets, rows, signs, n)
        assert rc == api.GCRE_ERR_ASSERT and b"permutation masks" in masked._lib.gcre_last_error(masked._h) and _untouched(arrays)
        assert masked.subsample_launches() == 0
    finally:
        masked.close()
    ex = open_context(2, nc, nt, VT)
    try:
        others = other_counters(ex)
        nan_cut = np.tile([1.0, 2.0], (3, 1))
        nan_cut[2, 0] = np.nan
        refused = [
            (dict(sets=[[2], []]), api.GCRE_ERR_ARG, b"has no members", 0),
            (dict(sets=[[2, 3]], signs=[[1, 0]]), api.GCRE_ERR_ARG, b"neither", 0),
            (dict(sets=[[2], [3, 40]]), api.GCRE_ERR_RANGE, b"out of range", 0),
            (dict(cap=2), api.GCRE_ERR_RANGE, b"room for 2", 3),
            (dict(draws=-1), api.GCRE_ERR_ARG, b"draws must not be negative, not -1", 3),
            (dict(m=(21, 12)), api.GCRE_ERR_ARG, b"m_cases = 21 outside 0 .. n_cases = 20", 3),
            (dict(m=(-1, 12)), api.GCRE_ERR_ARG, b"m_cases = -1 outside 0 .. n_cases = 20", 3),
            (dict(m=(10, 26)), api.GCRE_ERR_ARG, b"m_ctrls = 26 outside 0 .. n_ctrls = 25", 3),
            (dict(m=(10, -3)), api.GCRE_ERR_ARG, b"m_ctrls = -3 outside 0 .. n_ctrls = 25", 3),
            (dict(TA=None), api.GCRE_ERR_ARG, b"NULL argument (table_a)", 3),
            (dict(TA=np.ones((0, 5))), api.GCRE_ERR_ARG, b"table_a must have at least one row and one column, not 0 x 5", 3),
            (dict(TB=np.ones((3, 0))), api.GCRE_ERR_ARG, b"table_b must have at least one row and one column, not 3 x 0", 3),
            (dict(n_cut=-1), api.GCRE_ERR_ARG, b"n_cut = -1 outside 0 .. GCRE_SUBSAMPLE_MAX_CUTS = 8", 3),
            (dict(cuts=np.ones((3, 9))), api.GCRE_ERR_ARG, b"n_cut = 9 outside 0 .. GCRE_SUBSAMPLE_MAX_CUTS = 8", 3),
            (dict(cuts=None, n_cut=2), api.GCRE_ERR_ARG, b"NULL argument (cut) with n_cut = 2", 3),
            (dict(null=("n_a",)), api.GCRE_ERR_ARG, b"NULL argument (n_a) with n_cut = 2", 3),
            (dict(TB=None, null=("n_both", "scores_b")), api.GCRE_ERR_ARG, b"n_b without table_b", 3),
            (dict(TB=None, null=("n_b", "scores_b")), api.GCRE_ERR_ARG, b"n_both without table_b", 3),
            (dict(TB=None, null=("n_b", "n_both")), api.GCRE_ERR_ARG, b"scores_b without table_b", 3),
            (dict(cuts=nan_cut), api.GCRE_ERR_ARG, b"cut[2][0] is NaN", 3),
        ]
        for kw, code, msg, n_out in refused:
            kw = dict(kw)
            own = "sets" in kw
            rc, arrays, got_n = _raw_call(ex, kw.pop("sets", sets), rows, kw.pop("signs", None if own else signs), n, **kw)
            assert rc == code and msg in ex._lib.gcre_last_error(ex._h), (kw, rc, ex._lib.gcre_last_error(ex._h))
            assert _untouched(arrays) and got_n == n_out, kw
        rc, arrays, _ = _raw_call(ex, sets, np.zeros((40, n + 1), np.int8), signs, n + 1)
        assert rc == api.GCRE_ERR_ARG and _untouched(arrays)
        # the optional outputs of one tile: 512 draws x 3 sets x 8 bytes x 2 matrices = 24,576 bytes
        monkeypatch.setenv("GCRE_SUBSAMPLE_MAX_MB", repr(24575 / 1048576.0))
        rc, arrays, _ = _raw_call(ex, sets, rows, signs, n)
        assert rc == api.GCRE_ERR_ARG and b"GCRE_SUBSAMPLE_MAX_MB" in ex._lib.gcre_last_error(ex._h) and _untouched(arrays)
        with pytest.raises(api.GcreError, match="GCRE_SUBSAMPLE_MAX_MB"):
            ex.subsample_tests(sets, rows, signs, m_cases=10, m_ctrls=12, draws=10, scores=True)
        assert ex.subsample_launches() == 0 and other_counters(ex) == others
        monkeypatch.setenv("GCRE_SUBSAMPLE_MAX_MB", repr(24576 / 1048576.0))      # exactly the matrices of one tile: accepted, one slab
        TA, TB = small_table(10, 12, 5), small_table(10, 13, 6)
        rc, arrays, got_n = _raw_call(ex, sets, rows, signs, n, TA=TA, TB=TB)
        assert rc == api.GCRE_OK and got_n == 3 and ex.subsample_launches() == 4 and not _untouched(arrays)
        monkeypatch.delenv("GCRE_SUBSAMPLE_MAX_MB")
        ref = report.subsample_reference(sets, rows, signs, nc, 10, 12, 10, 7, TA, TB, np.tile([1.0, 2.0], (3, 1)), 2)
        out, cnt, sc = arrays
        assert all(np.array_equal(c, ref[k]) for c, k in zip(cnt, ("n_a", "n_b", "n_both")))
        assert np.array_equal(sc[0], bits(ref["scores_a"])) and np.array_equal(sc[1], bits(ref["scores_b"]))
        # with table_b, n_b and n_both may still be left out; the limits themselves pass
        assert _raw_call(ex, sets, rows, signs, n, null=("n_b", "n_both", "scores_a", "scores_b"))[0] == api.GCRE_OK
        assert _raw_call(ex, sets, rows, signs, n, m=(20, 25), cuts=np.ones((3, 8)))[0] == api.GCRE_OK
        assert _raw_call(ex, sets, rows, signs, n, m=(0, 0), cuts=None, null=("n_a", "n_b", "n_both"))[0] == api.GCRE_OK
        assert other_counters(ex) == others
    finally:
        ex.close()


# ---- contexts ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("method", [1, 2])
def test_no_draws_and_the_context(method):
    """draws = 0 launches nothing of the stage; a context without permutations is enough, one with masks gives the records of
    score_sets with their permutation p-values and the same counts, and only the stage's own counter moves."""
    nc, nt = 20, 25
    rng = np.random.default_rng(6100 + method)
    rows = make_rows(rng, nc + nt)
    sets, signs = make_family(rng)
    VT = small_table(nc, nt, 2)
    ma, mt = 10, 12
    TA, TB = small_table(ma, mt, 1), small_table(nc - ma, nt - mt, 2)
    cuts = make_cuts(rng, len(sets))
    kw = dict(m_cases=ma, m_ctrls=mt, seed=31, table_a=TA, table_b=TB, cuts=cuts, scores=True)
    ex = open_context(method, nc, nt, VT)
    try:
        others = other_counters(ex)
        rec, counts, sa, sb = ex.subsample_tests(sets, rows, signs, draws=0, **kw)
        assert ex.subsample_launches() == 0
        assert rec.tobytes() == ex.score_sets(sets, rows, signs).tobytes() and np.isnan(rec["pvalue"]).all()
        assert sa.shape == (len(sets), 0) and sb.shape == (len(sets), 0)
        for k in ("n_a", "n_b", "n_both"):
            assert counts[k].tolist() == [[0 if v else -1] * 3 for v in rec["valid"]]
        whole, _ = run_and_compare(ex, method, nc, sets, rows, signs, ma, mt, 100, 31, TA, TB, cuts)
        assert ex.subsample_launches() == 4 and other_counters(ex) == others
        rec0, counts0 = ex.subsample_tests([], rows, draws=50, cuts=[1.0])
        assert len(rec0) == 0 and len(counts0["n_a"]) == 0
        rec1, c1, a1, b1 = ex.subsample_tests([[2, -1]], rows, draws=50, cuts=[1.0], scores=True)
        assert rec1["valid"].tolist() == [0] and c1["n_a"].tolist() == [[-1]] and np.isnan(a1).all() and np.isnan(b1).all()
        assert ex.subsample_launches() == 4                          # no valid set: nothing launched
    finally:
        ex.close()
    masked = open_context(method, nc, nt, VT, K=300, seed=5)
    try:
        got = masked.subsample_tests(sets, rows, signs, draws=100, **kw)
        plain = masked.score_sets(sets, rows, signs)
        assert got[0].tobytes() == plain.tobytes() and (plain["pvalue"][plain["valid"] != 0] >= 0).all()
        for k in ("n_a", "n_b", "n_both"):
            assert np.array_equal(got[1][k], whole[1][k])
        assert got[2].tobytes() == whole[2].tobytes() and got[3].tobytes() == whole[3].tobytes()
        assert masked.subsample_launches() == 4
        # the draws are not the context's permutation masks: other masks, the same draws
        masked.generate_permutations(6, None)
        again = masked.subsample_tests(sets, rows, signs, draws=100, **kw)
        assert again[2].tobytes() == whole[2].tobytes()
    finally:
        masked.close()


@pytest.mark.parametrize("signed", [False, True])
def test_score_paths_stability(signed):
    """The columns score_paths appends are stability_columns of the reference on the default halves and their tables; without
    ``stability`` the frame is the one it was."""
    nc, nt, G, B = 33, 37, 60, 64
    rng = np.random.default_rng(6200 + signed)
    genes = [f"G{i}" for i in range(G)]
    data = (rng.random((G, nc + nt)) < rng.uniform(0.05, 0.4, size=(G, 1))).astype(np.int32)
    tags = ["(+)", "(-)"]
    paths = [" -> ".join(f"{genes[g]} {tags[int(rng.integers(0, 2))]}" for g in rng.choice(G, size=int(rng.integers(1, 5)), replace=False))
             for _ in range(18)]
    paths += [paths[3], "NOSUCHGENE (+) -> G1 (-)"]                  # a repeat and an NA row: 20 paths
    kw = dict(signed=signed, threshold=0.9, n_permutations=100, seed=77)
    plain = report.score_paths(paths, genes, data, nc, nt, **kw)
    assert list(plain.columns) == report.SCORE_PATHS_COLUMNS and "PerHalfSelected" not in plain.attrs
    assert plain.equals(report.score_paths(paths, genes, data, nc, nt, stability=0, **kw))
    assert plain.equals(report.score_paths(paths, genes, data, nc, nt, stability=0, stability_cuts=[1.0], **kw))
    method = 2 if signed else 1
    g2, d2 = report.preprocess_table(genes, data, 0.9, nc, nt)
    _, prow, psign = report.parse_sets(paths, g2)
    ma, mt = nc // 2, nt // 2
    TA, TB = api.values_table(ma, mt), api.values_table(nc - ma, nt - mt)
    for cuts in ([0.7], [0.3, 1.2], (rng.random((20, 2)) * 2).tolist()):
        full = report.score_paths(paths, genes, data, nc, nt, stability=B, stability_cuts=cuts, **kw)
        ref = report.subsample_reference(prow, np.asarray(d2), psign, nc, ma, mt, B, 77, TA, TB, cuts, method)
        valid = np.array([min(r) >= 0 for r in prow])
        want, per_half = report.stability_columns(ref, valid, B)
        assert list(full.columns) == report.SCORE_PATHS_COLUMNS + list(want)
        for col in report.SCORE_PATHS_COLUMNS:
            assert plain[col].equals(full[col]), col
        for col, w in want.items():
            np.testing.assert_array_equal(full[col].to_numpy(), w, err_msg=col)
            assert np.isnan(w[-1]) and (col.startswith("HalfReplication") or not np.isnan(w[:-1]).any())
        np.testing.assert_array_equal(full.attrs["PerHalfSelected"], per_half)
        assert 0 < per_half.max() <= 19
    both = report.score_paths(paths, genes, data, nc, nt, stability=B, stability_cuts=[0.7], competitive=20, minp=True, **kw)
    assert list(both.columns) == report.SCORE_PATHS_COLUMNS + report.MINP_COLUMNS + report.COMPETITIVE_COLUMNS + report.STABILITY_COLUMNS


# ---- seeded fuzz: a handful of cases by default, GCRE_SUBSAMPLE_FUZZ_CASES asks for a long run -------------------------------


def fuzz_case(case):
    rng = np.random.default_rng([6350, case])
    method = int(rng.integers(1, 3))
    n = int(rng.choice([2, 3, 31, 32, 33, 63, 64, 65, 70, 127, 128, 129, 200, 260, 700]))
    nc = int(rng.integers(1, n))
    nt = n - nc
    ma = int(rng.choice([0, nc // 2, nc, int(rng.integers(0, nc + 1))]))
    mt = int(rng.choice([0, nt // 2, nt, int(rng.integers(0, nt + 1))]))
    n_rows = int(rng.choice([4, 9, 40, 130]))
    sets = []
    for _ in range(int(rng.choice([1, 2, 7, 8, 9, 16, 17, 40]))):
        m = rng.integers(0, n_rows, int(rng.choice([1, 2, 3, 5, 30, 70]))).tolist()
        if rng.random() < 0.05:
            m[int(rng.integers(0, len(m)))] = -1
        sets.append(m)
    signs = None if rng.random() < 0.2 else [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    rows = (rng.random((n_rows, n)) < rng.uniform(0.0, 0.6, size=(n_rows, 1))).astype(np.int8)
    kind = str(rng.choice(["small", "small", "zeros", "nonfinite", "short"]))

    def table(a, b, seed):
        if kind == "small" or min(a, b) < 2:
            return small_table(a, b, seed)
        if kind == "short":
            return small_table(max(a // 2, 0), max(b - 1, 0), seed)
        return special_table(kind, a, b, seed, int(rng.integers(0, 3)) if kind == "nonfinite" else 0)

    TA = table(ma, mt, case)
    TB = False if rng.random() < 0.15 else table(nc - ma, nt - mt, case + 1)
    J = int(rng.choice([0, 1, 2, 8]))
    cuts = None if J == 0 else np.where(rng.random((len(sets), J)) < 0.1, -np.inf, rng.random((len(sets), J)) * 20)
    B = int(rng.choice([1, 2, 63, 64, 65, 257, 511, 512, 513, 1100]))
    slab = int(rng.choice([0, 0, 1, 512, 1024]))
    what = f"case {case}: method {method} n=({nc}, {nt}) m=({ma}, {mt}) rows={n_rows} sets={len(sets)} B={B} {kind} cuts={J} slab={slab} B-half={TB is not False}"
    return method, nc, nt, ma, mt, sets, rows, signs, TA, TB, cuts, B, slab, what


def test_seeded_fuzz(monkeypatch):
    cases = int(os.environ.get("GCRE_SUBSAMPLE_FUZZ_CASES", "8"))
    for case in range(cases):
        method, nc, nt, ma, mt, sets, rows, signs, TA, TB, cuts, B, slab, what = fuzz_case(case)
        if slab:
            monkeypatch.setenv("GCRE_SUBSAMPLE_SLAB_DRAWS", str(slab))
        else:
            monkeypatch.delenv("GCRE_SUBSAMPLE_SLAB_DRAWS", raising=False)
        ex = open_context(method, nc, nt, small_table(nc, nt, case))
        try:
            got, _ = run_and_compare(ex, method, nc, sets, rows, signs, ma, mt, B, 1000 + case, TA, TB, cuts, what)
            assert got[0].tobytes() == ex.score_sets(sets, rows, signs).tobytes(), what
        finally:
            ex.close()
    print(f"subsample fuzz: {cases} cases equal the reference")
