"""Competitive set tests on the device (gcre_score_sets_compete: k_compete_null).  Everything
``JoinExec.competitive_tests(null=True, picks=True)`` returns is compared exactly against ``report.competitive_reference`` on
the same table -- ``n_ge`` and ``picks`` as integers, ``null_scores`` as bit patterns -- and the records against ``score_sets``.
The shapes are the smallest at which each part can go wrong: dword and word edges of the patient columns, sets of more than
one pick per lane, draws around a wave's run and a slab's edge, the fallback of the draw rule, bins with fixed members."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from geneticscre_amd import api, report
from helpers import small_table, special_table

pytestmark = pytest.mark.gpu

N_POOL = 330
SIZES = (1, 2, 64, 65, 130)
DRAWS = (1, 63, 64, 65, 1000)
COUNTERS = [("given", "gcre_given_launches"), ("family", "gcre_family_launches"), ("minp", "gcre_minp_launches"),
            ("overlap", "gcre_overlap_launches"), ("clump", "gcre_clump_launches"), ("patients", "gcre_patient_launches"),
            ("burden", "gcre_burden_launches"), ("stepdown", "gcre_stepdown_launches")]


def other_counters(ex):
    """Every launch counter of the context but the stage's own."""
    return [int(getattr(api._feature_lib(f), sym)(ex._h)) for f, sym in COUNTERS]


def make_bins(kind):
    if kind == "one":
        return None
    bins = (np.arange(N_POOL) * 7 % 3).astype(np.int32)
    if kind == "fixed":
        bins[::11] = -1
    return bins


def fit(rng, k, bins):
    """k member rows in random order such that every bin keeps 2 (members drawn from it) <= its size; repeats allowed."""
    bn = np.zeros(N_POOL, int) if bins is None else bins
    size = np.bincount(bn[bn >= 0], minlength=3)
    need = np.zeros(3, int)
    out = []
    for r in rng.integers(0, N_POOL, 6 * k + 20).tolist():
        if len(out) == k:
            break
        if bn[r] < 0 or 2 * (need[bn[r]] + 1) <= size[bn[r]]:
            out.append(r)
            need[bn[r]] += bn[r] >= 0
    assert len(out) == k
    return out


def make_family(rng, bins):
    """Sets of every size of SIZES under both signs, a repeated member row, an NA member and, where the pool has rows that are
    never drawn, a set made only of those."""
    sets = [fit(rng, k, bins) for k in SIZES]
    sets.append([1, 1, 2])                                       # one row twice: two members, two distinct picks (rows that are drawn)
    sets.insert(2, [5, -1, 9])                                   # an NA member
    if bins is not None and (bins < 0).any():
        held = np.flatnonzero(bins < 0)
        sets.append(held[:3].tolist())                           # only fixed members
        sets[0] = [int(held[4])]                                 # ... and of one
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    signs[-1][0] = -1
    return sets, signs


def make_rows(rng, n):
    rows = (rng.random((N_POOL, n)) < rng.uniform(0.02, 0.5, size=(N_POOL, 1))).astype(np.int8)
    rows[0], rows[1] = 1, 0            # everybody, nobody
    return rows


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


def assert_equal_reference(got, ref, B, what=""):
    """(records, n_ge, null, picks) of a call with B draws against a reference of B draws or more."""
    rec, n_ge, null, picks = got
    assert n_ge.dtype == np.int64 and null.dtype == np.float64 and picks.dtype == np.int32
    assert null.shape == (len(rec), B) and picks.shape == (B, ref["picks"].shape[1])
    np.testing.assert_array_equal(picks, ref["picks"][:B], err_msg=f"{what} picks")
    np.testing.assert_array_equal(bits(null), bits(ref["null"][:, :B]), err_msg=f"{what} null scores")
    with np.errstate(invalid="ignore"):
        want = np.where(ref["n_ge"] < 0, -1, (ref["null"][:, :B] >= ref["obs"][:, None]).sum(axis=1))
    np.testing.assert_array_equal(n_ge, want, err_msg=f"{what} n_ge")
    np.testing.assert_array_equal(bits(rec["score"]), bits(ref["obs"]), err_msg=f"{what} observed")


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("pool", ["one", "three", "fixed"])
@pytest.mark.parametrize("n", [2, 33, 64, 65, 200])
def test_compete_against_the_reference(monkeypatch, method, pool, n):
    for var in ("GCRE_COMPETE_ATTEMPTS", "GCRE_COMPETE_SLAB_DRAWS", "GCRE_COMPETE_MAX_MB"):
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng([4100, method, ("one", "three", "fixed").index(pool), n])
    nc = max(1, n // 2 - 1)
    nt = n - nc
    bins = make_bins(pool)
    rows = make_rows(rng, n)
    sets, signs = make_family(rng, bins)
    VT = small_table(n, n, n)
    VT[rng.random(VT.shape) < 0.05] *= -1
    seed = int(rng.integers(0, 2**63))
    ref = report.competitive_reference(sets, rows, signs, bins, max(DRAWS), seed, nc, VT, method)
    ex = open_context(method, nc, nt, VT)
    try:
        plain = ex.score_sets(sets, rows, signs)
        others = other_counters(ex)
        for i, B in enumerate(DRAWS):
            got = ex.competitive_tests(sets, rows, signs, bins=bins, draws=B, seed=seed, null=True, picks=True)
            assert_equal_reference(got, ref, B, f"n={n} {pool} B={B}")
            assert got[0].tobytes() == plain.tobytes()                           # the records of score_sets
            assert ex.compete_launches() == i + 1                                # one slab
        rec, n_ge, null, picks = got
        bare = ex.competitive_tests(sets, rows, signs, bins=bins, draws=max(DRAWS), seed=seed)
        assert len(bare) == 2 and bare[0].tobytes() == rec.tobytes() and np.array_equal(bare[1], n_ge)
        assert other_counters(ex) == others
        # the NA set; distinct picks for the row listed twice; the sets of fixed members reproduce their observed score
        assert rec["valid"][2] == 0 and n_ge[2] == -1 and np.isnan(null[2]).all()
        off = np.concatenate([[0], np.cumsum([len(s) for s in sets])])
        assert (picks[:, off[2]:off[3]] == -1).all()
        dup = picks[:, off[6]:off[7]]
        assert ((dup[:, 0] != dup[:, 1]) & (dup[:, 1] != dup[:, 2]) & (dup[:, 0] != dup[:, 2])).all()
        if pool == "fixed":
            for s in (0, len(sets) - 1):
                assert (picks[:, off[s]:off[s + 1]] == np.asarray(sets[s])).all()
                assert (bits(null[s]) == bits(rec["score"][s])).all() and n_ge[s] == max(DRAWS)
        # another seed gives other draws
        assert not np.array_equal(ex.competitive_tests(sets, rows, signs, bins=bins, draws=65, seed=seed + 1, picks=True)[2], picks[:65])
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_a_pool_of_equal_rows(method):
    """Every row of the pool is the same row: whatever is drawn, the unions are the observed ones."""
    n, nc = 70, 30
    rng = np.random.default_rng(4200)
    rows = np.tile((rng.random(n) < 0.3).astype(np.int8), (N_POOL, 1))
    sets, signs = make_family(rng, None)
    if method == 2:
        signs = [[1] * len(s) for s in sets]
        signs[3] = [-1] * len(sets[3])                    # a draw keeps every sign: all (+) and all (-) sets stay what they are
    VT = small_table(n, n, 3)
    ex = open_context(method, nc, n - nc, VT)
    try:
        rec, n_ge, null = ex.competitive_tests(sets, rows, signs, draws=200, seed=9, null=True)
        valid = rec["valid"] != 0
        assert (n_ge[valid] == 200).all() and (bits(null[valid]) == bits(rec["score"][valid])[:, None]).all()
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_the_fallback(monkeypatch, method):
    """Sets exactly at 2k = N with one attempt per member: most draws take the fallback."""
    n, nc = 65, 31
    rng = np.random.default_rng(4300 + method)
    bins = (np.arange(N_POOL) % 2).astype(np.int32)             # two bins of 165
    bins[164:] = -1                                             # ... cut to 82 each; the rest is never drawn
    rows = make_rows(rng, n)
    even, odd = np.flatnonzero(bins == 0), np.flatnonzero(bins == 1)
    sets = [rng.permutation(even)[:41].tolist() + rng.permutation(odd)[:41].tolist(), [0, 2, 4, 6, 8, 10] + [200],
            rng.permutation(even)[:41].tolist()]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    VT = small_table(n, n, 4)
    ex = open_context(method, nc, n - nc, VT)
    try:
        for attempts in (1, 2, 64):
            monkeypatch.setenv("GCRE_COMPETE_ATTEMPTS", str(attempts))
            ref = report.competitive_reference(sets, rows, signs, bins, 300, 5, nc, VT, method, attempts=attempts)
            got = ex.competitive_tests(sets, rows, signs, bins=bins, draws=300, seed=5, null=True, picks=True)
            assert_equal_reference(got, ref, 300, f"attempts={attempts}")
            if attempts == 1:
                one = got[3]
        assert (one != got[3]).any(axis=1).mean() > 0.9         # the fallback was taken
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_slabs_change_nothing(monkeypatch, method):
    n, nc = 129, 60
    rng = np.random.default_rng(4400 + method)
    bins = make_bins("fixed")
    rows = make_rows(rng, n)
    sets, signs = make_family(rng, bins)
    VT = small_table(n, n, 5)
    ex = open_context(method, nc, n - nc, VT)
    try:
        monkeypatch.delenv("GCRE_COMPETE_SLAB_DRAWS", raising=False)
        monkeypatch.delenv("GCRE_COMPETE_MAX_MB", raising=False)
        B = 150
        ref = report.competitive_reference(sets, rows, signs, bins, B, 12, nc, VT, method)
        whole = ex.competitive_tests(sets, rows, signs, bins=bins, draws=B, seed=12, null=True, picks=True)
        assert_equal_reference(whole, ref, B, "one slab")
        assert ex.compete_launches() == 1
        for slab in (1, 7, 64):
            monkeypatch.setenv("GCRE_COMPETE_SLAB_DRAWS", str(slab))
            before = ex.compete_launches()
            got = ex.competitive_tests(sets, rows, signs, bins=bins, draws=B, seed=12, null=True, picks=True)
            assert ex.compete_launches() == before + (B + slab - 1) // slab
            for x, y in zip(got, whole):
                assert x.tobytes() == y.tobytes(), slab
            bare = ex.competitive_tests(sets, rows, signs, bins=bins, draws=B, seed=12)
            assert np.array_equal(bare[1], whole[1])
        monkeypatch.delenv("GCRE_COMPETE_SLAB_DRAWS")
        # a bound that leaves room for 10 draws of both optional outputs
        per_draw = len(sets) * 8 + sum(len(s) for s in sets) * 4
        monkeypatch.setenv("GCRE_COMPETE_MAX_MB", repr((10 * per_draw + 1) / 1048576.0))
        before = ex.compete_launches()
        got = ex.competitive_tests(sets, rows, signs, bins=bins, draws=B, seed=12, null=True, picks=True)
        assert ex.compete_launches() == before + 15
        for x, y in zip(got, whole):
            assert x.tobytes() == y.tobytes()
        before = ex.compete_launches()                          # without optional outputs the bound does not bind
        assert np.array_equal(ex.competitive_tests(sets, rows, signs, bins=bins, draws=B, seed=12)[1], whole[1])
        assert ex.compete_launches() == before + 1
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("kind,variant", [("zeros", 0), ("nonfinite", 0), ("nonfinite", 1), ("nonfinite", 2), ("huge", 0), ("tiny", 0)])
def test_special_tables(method, kind, variant):
    """NaN, infinities, signed zeros: the null score is the table's own f64 value, and a NaN on either side never counts."""
    nc, nt = 33, 37
    n = nc + nt
    rng = np.random.default_rng(4500 + 10 * method + variant)
    bins = make_bins("three")
    rows = make_rows(rng, n)
    sets = [rng.integers(0, N_POOL, size=int(k)).tolist() for k in rng.integers(1, 5, size=40)] + [[1]]      # nobody: table[0][0]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    VT = special_table(kind, nc, nt, 3, variant)
    ref = report.competitive_reference(sets, rows, signs, bins, 256, 3, nc, VT, method)
    ex = open_context(method, nc, nt, VT)
    try:
        got = ex.competitive_tests(sets, rows, signs, bins=bins, draws=256, seed=3, null=True, picks=True)
        assert_equal_reference(got, ref, 256, f"{kind}{variant}")
        rec, n_ge, null, _ = got
        if kind == "nonfinite":
            assert np.isnan(null).any(), "no NaN null score"
            nan_obs = np.isnan(rec["score"])
            assert (n_ge[nan_obs] == 0).all()
            if variant == 0:
                assert nan_obs.any(), "no NaN observed score"
        if kind == "zeros":
            z = null[null == 0.0]
            assert len({bool(x) for x in np.signbit(z)}) == 2, "no -0.0 / +0.0 among the null scores"
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_more_patients_than_one_column_chunk(method):
    """A wave covers 8,192 patients at a time: 8,192 + 65 patients are one whole chunk of columns and a partial one, with
    carriers and controls on both sides of the edge.  Sets of 9 and 70 members are more than the rows a lane keeps in flight."""
    n, nc = 8192 + 65, 120
    rng = np.random.default_rng(4250 + method)
    rows = (rng.random((160, n)) < rng.uniform(0.001, 0.02, size=(160, 1))).astype(np.int8)
    rows[:, 8180:] |= (rng.random((160, n - 8180)) < 0.2).astype(np.int8)
    rows[:, :nc] |= (rng.random((160, nc)) < 0.1).astype(np.int8)
    bins = (np.arange(160) % 2).astype(np.int32)
    sets = [[3], [4, 5, 6], rng.integers(0, 160, 9).tolist(), rng.permutation(160)[:70].tolist()]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    VT = small_table(nc, n - nc, 6)
    ref = report.competitive_reference(sets, rows, signs, bins, 40, 2, nc, VT, method)
    ex = open_context(method, nc, n - nc, VT)
    try:
        got = ex.competitive_tests(sets, rows, signs, bins=bins, draws=40, seed=2, null=True, picks=True)
        assert_equal_reference(got, ref, 40, f"n={n}")
        assert len(np.unique(got[2][3])) > 20                    # the scores move with the draw
    finally:
        ex.close()


def _raw_call(ex, sets, rows, signs, n, bins=None, n_bins=1, draws=10, cap=None, ge_null=False):
    """gcre_score_sets_compete through ctypes on arrays filled with a pattern: (return code, the arrays)."""
    lib = api._compete_lib()
    inp, keep = api._set_input(sets, rows, signs, n)
    S = len(sets)
    B = max(int(draws), 0)
    out = np.full(max(S, 1), 0x5a, dtype=np.uint8).repeat(api.SET_SCORE.itemsize).view(api.SET_SCORE)
    ge = np.full(max(S, 1), 0x5a5a5a5a, np.int64)
    nul = np.full((S, B), 0x5a5a5a5a5a5a5a5a, np.uint64)
    pk = np.full((B, len(keep[1])), 0x5a5a5a5a, np.int32)
    bn = None if bins is None else np.ascontiguousarray(bins, dtype=np.int32)
    n_out = ctypes.c_int64(0)
    rc = lib.gcre_score_sets_compete(ex._h, ctypes.byref(inp), api._ptr(bn), n_bins, draws, 7, api._ptr(out), len(out) if cap is None else cap,
                                     ctypes.byref(n_out), None if ge_null else api._ptr(ge), api._ptr(nul), api._ptr(pk))
    del keep
    return rc, (out, ge, nul, pk)


def _untouched(arrays):
    out, ge, nul, pk = arrays
    return (out.view(np.uint8) == 0x5a).all() and (ge == 0x5a5a5a5a).all() and (nul == 0x5a5a5a5a5a5a5a5a).all() and \
        (pk == 0x5a5a5a5a).all()


def test_refusals_launch_nothing_and_write_nothing(monkeypatch):
    nc, nt = 20, 25
    n = nc + nt
    rng = np.random.default_rng(4600)
    rows = make_rows(rng, n)[:40]
    VT = small_table(n, n, 1)
    sets, signs = [[2, 3], [4], [5, 6, 7]], [[1, -1], [1], [-1, 1, 1]]
    bins = (np.arange(40) % 2).astype(np.int32)
    for var in ("GCRE_COMPETE_ATTEMPTS", "GCRE_COMPETE_SLAB_DRAWS", "GCRE_COMPETE_MAX_MB"):
        monkeypatch.delenv(var, raising=False)
    fresh = api.JoinExec(2, nc, nt, 0)
    try:
        rc, arrays = _raw_call(fresh, sets, rows, signs, n)
        assert rc == api.GCRE_ERR_ASSERT and b"value table" in fresh._lib.gcre_last_error(fresh._h) and _untouched(arrays)
        assert fresh.compete_launches() == 0
    finally:
        fresh.close()
    masked = api.JoinExec(2, nc, nt, 100)                       # permutations asked for, none set: what score_sets refuses
    try:
        masked.set_value_table(VT)
        rc, arrays = _raw_call(masked, sets, rows, signs, n)
        assert rc == api.GCRE_ERR_ASSERT and b"permutation masks" in masked._lib.gcre_last_error(masked._h) and _untouched(arrays)
    finally:
        masked.close()
    ex = open_context(2, nc, nt, VT)
    try:
        others = other_counters(ex)
        big = [list(range(40)) * 26]                            # 1,040 members
        tight = [[0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20]]       # 11 of the 20 even rows
        refused = [
            (dict(sets=[[2], []]), api.GCRE_ERR_ARG, b"has no members"),
            (dict(sets=[[2, 3]], signs=[[1, 0]]), api.GCRE_ERR_ARG, b"neither"),
            (dict(sets=[[2], [3, 40]]), api.GCRE_ERR_RANGE, b"out of range"),
            (dict(sets=sets, signs=signs, cap=2), api.GCRE_ERR_RANGE, b"room for 2"),
            (dict(sets=sets, signs=signs, ge_null=True), api.GCRE_ERR_ARG, b"NULL argument (n_ge)"),
            (dict(sets=sets, signs=signs, draws=-1), api.GCRE_ERR_ARG, b"draws must not be negative"),
            (dict(sets=sets, signs=signs, n_bins=0), api.GCRE_ERR_ARG, b"n_bins must be at least 1"),
            (dict(sets=sets, signs=signs, bins=bins, n_bins=1), api.GCRE_ERR_ARG, b"bin[1] = 1 out of range (1 bins"),
            (dict(sets=sets, signs=signs, bins=np.where(np.arange(40) == 7, -2, bins), n_bins=2), api.GCRE_ERR_ARG, b"bin[7] = -2 out of range"),
            (dict(sets=tight, bins=bins, n_bins=2), api.GCRE_ERR_ARG, b"set 0 draws 11 members from bin 0 of 20 rows"),
            (dict(sets=[list(range(21))]), api.GCRE_ERR_ARG, b"set 0 draws 21 members from bin 0 of 40 rows"),
            (dict(sets=big), api.GCRE_ERR_ARG, b"1040 members, more than GCRE_COMPETE_MAX_MEMBERS = 1024"),
        ]
        for kw, code, msg in refused:
            rc, arrays = _raw_call(ex, kw["sets"], rows, kw.get("signs"), n, bins=kw.get("bins"), n_bins=kw.get("n_bins", 1),
                                   draws=kw.get("draws", 10), cap=kw.get("cap"), ge_null=kw.get("ge_null", False))
            assert rc == code and msg in ex._lib.gcre_last_error(ex._h), (kw, rc, ex._lib.gcre_last_error(ex._h))
            assert _untouched(arrays), kw
        rc, arrays = _raw_call(ex, sets, np.zeros((40, n + 1), np.int8), signs, n + 1)
        assert rc == api.GCRE_ERR_ARG and _untouched(arrays)
        # the optional outputs of one draw: 3 sets x 8 + 6 members x 4 = 48 bytes
        monkeypatch.setenv("GCRE_COMPETE_MAX_MB", repr(47 / 1048576.0))
        rc, arrays = _raw_call(ex, sets, rows, signs, n, bins=bins, n_bins=2)
        assert rc == api.GCRE_ERR_ARG and b"GCRE_COMPETE_MAX_MB" in ex._lib.gcre_last_error(ex._h) and _untouched(arrays)
        with pytest.raises(api.GcreError, match="GCRE_COMPETE_MAX_MB"):
            ex.competitive_tests(sets, rows, signs, bins=bins, draws=10, null=True, picks=True)
        assert ex.compete_launches() == 0 and other_counters(ex) == others
        monkeypatch.setenv("GCRE_COMPETE_MAX_MB", repr(48 / 1048576.0))             # exactly one draw: ten slabs
        rc, arrays = _raw_call(ex, sets, rows, signs, n, bins=bins, n_bins=2)
        assert rc == api.GCRE_OK and ex.compete_launches() == 10 and not _untouched(arrays)
        monkeypatch.delenv("GCRE_COMPETE_MAX_MB")
        ref = report.competitive_reference(sets, rows, signs, bins, 10, 7, nc, VT, 2)
        out, ge, nul, pk = arrays
        assert np.array_equal(ge, ref["n_ge"]) and np.array_equal(pk, ref["picks"]) and np.array_equal(nul, bits(ref["null"]))
        # the limits themselves pass: 20 of 40 rows, 1,024 members (in a pool that holds twice as many)
        assert _raw_call(ex, [list(range(20))], rows, None, n)[0] == api.GCRE_OK
        wide = np.zeros((2048, n), np.int8)
        assert _raw_call(ex, [list(range(1024))], wide, None, n, draws=2)[0] == api.GCRE_OK
        assert other_counters(ex) == others
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_no_draws_and_the_context(method):
    """draws = 0 launches nothing of the stage; a context without permutations is enough, one with masks gives the records of
    score_sets with their permutation p-values, and only the stage's own counter moves."""
    nc, nt = 20, 25
    n = nc + nt
    rng = np.random.default_rng(4700 + method)
    bins = make_bins("three")
    rows = make_rows(rng, n)
    sets, signs = make_family(rng, bins)
    VT = small_table(n, n, 2)
    ref = report.competitive_reference(sets, rows, signs, bins, 100, 31, nc, VT, method)
    ex = open_context(method, nc, nt, VT)
    try:
        others = other_counters(ex)
        rec, n_ge, null, picks = ex.competitive_tests(sets, rows, signs, bins=bins, draws=0, seed=31, null=True, picks=True)
        assert ex.compete_launches() == 0
        assert rec.tobytes() == ex.score_sets(sets, rows, signs).tobytes() and np.isnan(rec["pvalue"]).all()
        assert null.shape == (len(sets), 0) and picks.shape == (0, sum(len(s) for s in sets))
        assert n_ge.tolist() == [0 if v else -1 for v in rec["valid"]]
        assert_equal_reference(ex.competitive_tests(sets, rows, signs, bins=bins, draws=100, seed=31, null=True, picks=True), ref, 100)
        assert ex.compete_launches() == 1 and other_counters(ex) == others
        rec0, ge0 = ex.competitive_tests([], rows, draws=50)
        assert len(rec0) == 0 and len(ge0) == 0
        rec1, ge1, nul1 = ex.competitive_tests([[2, -1]], rows, draws=50, null=True)
        assert rec1["valid"].tolist() == [0] and ge1.tolist() == [-1] and np.isnan(nul1).all()
        assert ex.compete_launches() == 1
    finally:
        ex.close()
    masked = open_context(method, nc, nt, VT, K=300, seed=5)
    try:
        got = masked.competitive_tests(sets, rows, signs, bins=bins, draws=100, seed=31, null=True, picks=True)
        assert_equal_reference(got, ref, 100, "with masks")
        plain = masked.score_sets(sets, rows, signs)
        assert got[0].tobytes() == plain.tobytes() and (plain["pvalue"][plain["valid"] != 0] >= 0).all()
        assert masked.compete_launches() == 1
    finally:
        masked.close()


@pytest.mark.parametrize("signed", [False, True])
def test_score_paths_competitive(signed):
    """The column score_paths appends is competitive_columns of the reference on the whole preprocessed table; without
    ``competitive`` the frame is the one it was; a fixed gene changes only the sets that contain it."""
    nc, nt, G, B = 33, 37, 120, 200
    n = nc + nt
    rng = np.random.default_rng(4800 + signed)
    genes = [f"G{i}" for i in range(G)]
    data = (rng.random((G, n)) < rng.uniform(0.05, 0.4, size=(G, 1))).astype(np.int32)
    tags = ["(+)", "(-)"]
    paths = [" -> ".join(f"{genes[g]} {tags[int(rng.integers(0, 2))]}" for g in rng.choice(G, size=int(rng.integers(1, 5)), replace=False))
             for _ in range(28)]
    paths += [paths[3], "NOSUCHGENE (+) -> G1 (-)"]                  # a repeat and an NA row: 30 paths
    kw = dict(signed=signed, threshold=0.9, n_permutations=100, seed=77)
    plain = report.score_paths(paths, genes, data, nc, nt, **kw)
    full = report.score_paths(paths, genes, data, nc, nt, competitive=B, **kw)
    assert list(plain.columns) == report.SCORE_PATHS_COLUMNS
    assert list(full.columns) == report.SCORE_PATHS_COLUMNS + report.COMPETITIVE_COLUMNS
    assert plain.equals(report.score_paths(paths, genes, data, nc, nt, competitive=0, **kw))
    for col in report.SCORE_PATHS_COLUMNS:
        assert plain[col].equals(full[col]), col
    both = report.score_paths(paths, genes, data, nc, nt, competitive=B, minp=True, family_inference=True, **kw)
    assert list(both.columns) == report.SCORE_PATHS_COLUMNS + report.FAMILY_COLUMNS + report.MINP_COLUMNS + report.COMPETITIVE_COLUMNS
    assert both["CompetitivePvalues"].equals(full["CompetitivePvalues"])
    # the reference: the whole preprocessed table as the pool, ten bins of carrier totals
    method = 2 if signed else 1
    g2, d2 = report.preprocess_table(genes, data, 0.9, nc, nt)
    _, prow, psign = report.parse_sets(paths, g2)
    VT = api.values_table(nc, nt)
    b10 = report.carrier_bins(d2, 10)
    ref = report.competitive_reference(prow, np.asarray(d2), psign, b10, B, 77, nc, VT, method)
    want = report.competitive_columns(ref["n_ge"], ~np.isnan(ref["obs"]), B)["CompetitivePvalues"]
    np.testing.assert_array_equal(full["CompetitivePvalues"].to_numpy(), want)
    assert np.isnan(want[-1]) and not np.isnan(want[:-1]).any()
    assert np.array_equal(full["Scores"].to_numpy()[:-1], ref["obs"][:-1])
    # other bins, other draws
    b4 = report.score_paths(paths, genes, data, nc, nt, competitive=B, competitive_bins=4, **kw)
    ref4 = report.competitive_reference(prow, np.asarray(d2), psign, report.carrier_bins(d2, 4), B, 77, nc, VT, method)
    np.testing.assert_array_equal(b4["CompetitivePvalues"].to_numpy(), report.competitive_columns(ref4["n_ge"], ~np.isnan(ref4["obs"]), B)["CompetitivePvalues"])
    # a fixed gene: the sets that contain it are drawn with it held, the others as before
    gene = g2[prow[0][0]]
    held = report.score_paths(paths, genes, data, nc, nt, competitive=B, fixed=[gene], **kw)
    touched = np.array([prow[0][0] in rs for rs in prow])
    assert touched.any() and not touched.all()
    fb = b10.copy()
    fb[prow[0][0]] = -1
    reff = report.competitive_reference(prow, np.asarray(d2), psign, fb, B, 77, nc, VT, method)
    wantf = np.where(touched, report.competitive_columns(reff["n_ge"], ~np.isnan(reff["obs"]), B)["CompetitivePvalues"], want)
    np.testing.assert_array_equal(held["CompetitivePvalues"].to_numpy(), wantf)
    assert held["CompetitivePvalues"][~touched].equals(full["CompetitivePvalues"][~touched])
    for col in report.SCORE_PATHS_COLUMNS:
        assert held[col].equals(plain[col]), col


# ---- seeded fuzz: a handful of cases by default, GCRE_COMPETE_FUZZ_CASES asks for a long run ----------------------------


def fuzz_case(case):
    rng = np.random.default_rng([4950, case])
    method = int(rng.integers(1, 3))
    n = int(rng.choice([2, 3, 31, 32, 33, 63, 64, 65, 70, 127, 128, 129, 200, 260]))
    nc = int(rng.integers(1, n))
    n_rows = int(rng.choice([4, 9, 40, 130, 300, 700]))
    n_bins = int(rng.choice([1, 1, 2, 3, 7]))
    bins = rng.integers(0, n_bins, n_rows).astype(np.int32)
    bins[rng.random(n_rows) < float(rng.choice([0.0, 0.0, 0.1, 0.5]))] = -1
    size = np.bincount(bins[bins >= 0], minlength=n_bins)
    sets = []
    for _ in range(int(rng.choice([1, 2, 5, 17, 40]))):
        want = int(rng.choice([1, 2, 3, 5, 30, 63, 64, 65, 128, 129, 257, 300]))
        need, m = np.zeros(n_bins, int), []
        for r in rng.integers(0, n_rows, 3 * want).tolist():
            if len(m) < want and (bins[r] < 0 or 2 * (need[bins[r]] + 1) <= size[bins[r]]):
                m.append(r)
                need[bins[r]] += bins[r] >= 0
        if not m:
            m = [-1]
        if rng.random() < 0.05:
            m[int(rng.integers(0, len(m)))] = -1
        sets.append(m)
    signs = None if rng.random() < 0.2 else [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    rows = (rng.random((n_rows, n)) < rng.uniform(0.0, 0.5, size=(n_rows, 1))).astype(np.int8)
    kind = str(rng.choice(["small", "small", "zeros", "nonfinite"]))
    VT = small_table(nc, n - nc, case) if kind == "small" else special_table(kind, nc, n - nc, case, int(rng.integers(0, 3)) if kind == "nonfinite" else 0)
    B = int(rng.choice([1, 2, 7, 8, 9, 63, 64, 65, 100, 257]))
    slab = int(rng.choice([0, 0, 1, 5, 64]))
    attempts = int(rng.choice([64, 64, 1, 2]))
    use_bins = None if n_bins == 1 and not (bins < 0).any() and rng.random() < 0.5 else bins
    what = f"case {case}: method {method} n={n} rows={n_rows} bins={n_bins} sets={len(sets)} B={B} {kind} slab={slab} attempts={attempts}"
    return method, nc, n - nc, sets, rows, signs, use_bins, VT, B, slab, attempts, what


def test_seeded_fuzz(monkeypatch):
    cases = int(os.environ.get("GCRE_COMPETE_FUZZ_CASES", "8"))
    monkeypatch.delenv("GCRE_COMPETE_MAX_MB", raising=False)
    for case in range(cases):
        method, nc, nt, sets, rows, signs, bins, VT, B, slab, attempts, what = fuzz_case(case)
        if slab:
            monkeypatch.setenv("GCRE_COMPETE_SLAB_DRAWS", str(slab))
        else:
            monkeypatch.delenv("GCRE_COMPETE_SLAB_DRAWS", raising=False)
        monkeypatch.setenv("GCRE_COMPETE_ATTEMPTS", str(attempts))
        seed = 1000 + case
        ref = report.competitive_reference(sets, rows, signs, bins, B, seed, nc, VT, method, attempts=attempts)
        ex = open_context(method, nc, nt, VT)
        try:
            got = ex.competitive_tests(sets, rows, signs, bins=bins, draws=B, seed=seed, null=True, picks=True)
            assert_equal_reference(got, ref, B, what)
            assert got[0].tobytes() == ex.score_sets(sets, rows, signs).tobytes(), what
        finally:
            ex.close()
    print(f"compete fuzz: {cases} cases equal the reference")
