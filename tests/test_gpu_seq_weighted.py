"""Weighted sequential p-values on the device (gcre_score_sets_sequential_weighted: k_seq_weighted_search,
k_seq_weighted_write, then k_seq_null and k_seq_retire as they were).  Every count
``JoinExec.weighted_sequential_tests`` returns is compared as an integer, for every set, with the definition in numpy alone:
``api.weighted_thresholds`` (host code) -> ``report.weighted_masks`` -> the null scores through the value table ->
``report.weighted_sequential_reference``.  The inputs, cohorts and helpers are those of tests/test_gpu_sequential.py; the odds
are log-normal and confounded with the strata.  The permutation index is 64-bit in the kernels, but no test here can reach an
index beyond 2^32: tests/test_seq_weighted_host.py holds the hash chain there, on the header the kernels compile."""
from __future__ import annotations

import os

import numpy as np
import pytest

from geneticscre_amd import api, report
import test_gpu_sequential as t
from test_seq_weighted_host import implied_launches

pytestmark = pytest.mark.gpu

PERM_SEED = t.PERM_SEED
HITS, CAP, P_MAX = t.HITS, t.CAP, t.P_MAX
ERR_RANGE, ERR_ARG = -2, -4
WHO = "score_sets_sequential_weighted: "
SIX = [1 / 3, 1, 3, 1, 1, 1]

# (method, cases, controls, strata) -> (the trial of make_input, max_perms): found on the CPU by tools/seq_weighted_seeds.py so
# that the reference alone puts a set into every class of `classes_of` at HITS hits and CAP permutations a batch, and the
# accepted attempts hold even ones, odd ones and one >= 8 (a second pass of the search)
CLASS_CASES = {
    (1, 70, 61, 1): (24, 18761),
    (1, 70, 61, 3): (37, 2941),
    (1, 33, 31, 1): (84, 2645),
    (1, 33, 31, 3): (37, 16178),
    (2, 70, 61, 1): (13, 17546),
    (2, 70, 61, 3): (193, 10035),
    (2, 33, 31, 1): (93, 14728),
    (2, 33, 31, 3): (209, 16527),
}
# the six-patient cohort with odds SIX: (seed, max_attempts, max_perms, hits) with 512 < R < max_perms, and (seed,
# max_attempts) whose permutation 0 is left over; by the same tool
LEFT_OVER = (0, 14, 3000, 200)                # R = 935
LEFT_AT_ZERO = (6, 3)
# ... and a cohort whose estimate fits under max_attempts = 1 (odds LEFT_ONE_ODDS): a seed whose permutation 0 is left over
LEFT_ONE_ODDS = [1e4, 1e4, 200.0, 1.0, 1e-4, 1e-4]
LEFT_AT_ZERO_ONE = 1


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for var in t.ENV:
        monkeypatch.delenv(var, raising=False)


def make_odds(method, nc, nt, ns, strata, trial=0):
    """Log-normal odds that lean on the stratum: the covariate the strata only bin."""
    rng = np.random.default_rng([7350, method, nc, nt, ns, trial])
    st = np.zeros(nc + nt) if strata is None else np.asarray(strata, float)
    return np.exp(rng.normal(0.0, 0.8, nc + nt) + 0.6 * st)


def reference(method, sets, signs, rows, nc, nt, VT, odds, strata, perms, seed, max_attempts=1 << 20):
    """(obs, null, valid, attempts) of the definition over ``perms`` permutations."""
    thr, _ = api.weighted_thresholds(odds, nc, nt, strata)
    masks, att = report.weighted_masks(thr, nc, nt, perms, seed, strata, max_attempts=max_attempts)
    obs, null, valid = t.reference_null(method, sets, signs, rows, nc, VT, masks)
    return obs, null, valid, att


_NULLS = {}


def problem(method, nc, nt, ns, trial=0):
    """The input of a configuration, its odds and its reference null matrix over P_MAX permutations: computed once, never
    changed."""
    key = (method, nc, nt, ns, trial)
    if key not in _NULLS:
        rows, sets, signs, strata = t.make_input(method, nc, nt, ns, trial)
        odds = make_odds(method, nc, nt, ns, strata, trial)
        VT = api.values_table(nc, nt)
        obs, null, valid, att = reference(method, sets, signs, rows, nc, nt, VT, odds, strata, P_MAX, PERM_SEED)
        for a in (obs, null, valid, att, odds):
            a.setflags(write=False)
        _NULLS[key] = (rows, sets, signs, strata, odds, VT, obs, null, valid, att)
    return _NULLS[key]


def dwords_of(nc, nt, ns):
    """W32p + S: the mask rows of a context (64-bit words, rounded up to four of them, as dwords) and one accepted attempt per
    stratum."""
    return 2 * 4 * (((nc + nt + 63) // 64 + 3) // 4) + ns


def open_context(method, nc, nt, VT, K=0):
    ex = api.JoinExec(method, nc, nt, K)
    ex.set_value_table(VT)
    return ex


# ---- every class of set, every set as integers -----------------------------------------------------------------------------


@pytest.mark.parametrize("method,nc,nt,ns", t.CONFIGS)
def test_every_class_of_set(monkeypatch, method, nc, nt, ns):
    trial, max_perms = CLASS_CASES[(method, nc, nt, ns)]
    rows, sets, signs, strata, odds, VT, obs, null, valid, att = problem(method, nc, nt, ns, trial)
    ref = report.weighted_sequential_reference(null, obs, valid, HITS, max_perms, att)
    found = t.classes_of(ref, valid, max_perms, CAP)
    print(found, "attempts: mean", att[:max_perms].mean(axis=0), "max", att[:max_perms].max(axis=0))
    # from the reference alone: the input covers every class, nothing is left over, and the search takes a second pass
    assert all(v > 0 for v in found.values()), found
    assert ref["first_left_over"] is None and not ref["refused"]
    a = att[:max_perms]
    assert (a % 2 == 0).any() and (a % 2 == 1).any() and (a >= 8).any() and (a != report.WEIGHTED_NONE).all()
    assert ref["n_perm"][34] == HITS and ref["stopped"][34] == 1     # no carriers: every permutation ties the score
    assert ref["n_hit"][35] == 0 and ref["stopped"][35] == 0         # planted on the cases: never reached
    assert ref["n_hit"][33] == -1 and ref["n_perm"][33] == -1        # an NA member
    monkeypatch.setenv("GCRE_SEQ_BATCH_PERMS", str(CAP))
    ex = open_context(method, nc, nt, VT)
    try:
        plain = ex.score_sets(sets, rows, signs)
        others = t.other_counters(ex)
        assert ex.sequential_launches() == 0 and ex.weighted_launches() == 0
        rec, seq = ex.weighted_sequential_tests(sets, rows, signs, odds=odds, hits=HITS, max_perms=max_perms, seed=PERM_SEED, strata=strata)
        assert rec.tobytes() == plain.tobytes()                       # the records of score_sets
        assert seq.dtype == api.SEQ_SCORE and len(seq) == len(sets)
        t.assert_equal(seq, ref, f"{(method, nc, nt, ns)}")
        # four kernels a batch, and batches until the last active set has stopped or max_perms is reached
        want = implied_launches(ref, valid, max_perms, dwords_of(nc, nt, ns), cap_perms=CAP)
        assert want == 4 * ((max_perms + CAP - 1) // CAP)             # (a set runs to the end)
        assert ex.sequential_launches() == want
        assert t.other_counters(ex) == others and ex.weighted_launches() == 0
    finally:
        ex.close()


@pytest.mark.parametrize("method,nc,nt,ns", [(1, 70, 61, 1), (2, 70, 61, 3), (2, 33, 31, 1), (1, 33, 31, 3)])
def test_no_value_depends_on_the_batches(monkeypatch, method, nc, nt, ns):
    """hits x max_perms x batch cap, and a byte bound that leaves one tile: against the reference, so equal to each other."""
    rows, sets, signs, strata, odds, VT, obs, null, valid, att = problem(method, nc, nt, ns, CLASS_CASES[(method, nc, nt, ns)][0])
    ex = open_context(method, nc, nt, VT)
    try:
        for h in (1, 5, 20):
            for max_perms in (0, 700, 3000, P_MAX):
                ref = report.weighted_sequential_reference(null, obs, valid, h, max_perms, att)
                assert not ref["refused"]
                for cap, mb in (("512", None), ("1024", None), (None, None), (None, "0.01")):
                    for var, val in (("GCRE_SEQ_BATCH_PERMS", cap), ("GCRE_SEQ_MAX_MB", mb)):
                        if val is None:
                            monkeypatch.delenv(var, raising=False)
                        else:
                            monkeypatch.setenv(var, val)
                    before = ex.sequential_launches()
                    rec, seq = ex.weighted_sequential_tests(sets, rows, signs, odds=odds, hits=h, max_perms=max_perms, seed=PERM_SEED,
                                                            strata=strata)
                    t.assert_equal(seq, ref, f"h={h} max_perms={max_perms} cap={cap} mb={mb}")
                    want = implied_launches(ref, valid, max_perms, dwords_of(nc, nt, ns), float(mb) if mb else 1024.0, int(cap) if cap else 0)
                    assert ex.sequential_launches() == before + want, f"h={h} max_perms={max_perms} cap={cap} mb={mb}"
        # the schedule without a cap: 4,096, then 16,384 -- two batches when a set runs to the end
        monkeypatch.delenv("GCRE_SEQ_MAX_MB")
        before = ex.sequential_launches()
        ex.weighted_sequential_tests(sets, rows, signs, odds=odds, hits=20, max_perms=P_MAX, seed=PERM_SEED, strata=strata)
        assert ex.sequential_launches() == before + 4 * 2
    finally:
        ex.close()


# ---- odd strata and odds ------------------------------------------------------------------------------------------------------


def odd_cases():
    nc, nt = 70, 61
    n = nc + nt
    rng = np.random.default_rng(7360)
    st16 = (np.arange(n) * 7) % 16
    yield "sixteen strata", st16, np.exp(rng.normal(0, 0.7, n) + 0.1 * st16)
    z = rng.uniform(0.5, 2.0, n)
    z[nc + rng.permutation(nt)[:25]] = 0.0
    yield "odds with zeros", None, z
    heavy = np.ones(n)
    heavy[90] = 1e9
    yield "one patient at 1e9", rng.integers(0, 2, n), heavy
    none = rng.integers(0, 3, n)
    none[:nc][none[:nc] == 2] = 0                                   # stratum 2: controls only
    yield "a stratum without cases", none, np.exp(rng.normal(0, 1, n))
    full = rng.integers(0, 2, n) * 5                                # ids 0 and 5; a third stratum, id 9:
    full[[3, 8, 20, 100, 101, 120]] = 9                             # three cases, three controls ...
    o = np.exp(rng.normal(0, 1, n))
    o[[100, 101, 120]] = 0.0                                        # ... whose controls have odds 0: its cases are all it can draw
    yield "a stratum whose cases are its positive odds", full, o


@pytest.mark.parametrize("name,strata,odds", list(odd_cases()), ids=[c[0] for c in odd_cases()])
@pytest.mark.parametrize("method", [1, 2])
def test_odd_strata_and_odds(monkeypatch, method, name, strata, odds):
    nc, nt, max_perms = 70, 61, 3000
    rows, sets, signs, _ = t.make_input(method, nc, nt, 1)
    VT = api.values_table(nc, nt)
    obs, null, valid, att = reference(method, sets, signs, rows, nc, nt, VT, odds, strata, max_perms, PERM_SEED)
    assert (att != report.WEIGHTED_NONE).all()
    ex = open_context(method, nc, nt, VT)
    try:
        for h, cap in ((5, "512"), (20, None)):
            if cap:
                monkeypatch.setenv("GCRE_SEQ_BATCH_PERMS", cap)
            else:
                monkeypatch.delenv("GCRE_SEQ_BATCH_PERMS", raising=False)
            ref = report.weighted_sequential_reference(null, obs, valid, h, max_perms, att)
            rec, seq = ex.weighted_sequential_tests(sets, rows, signs, odds=odds, hits=h, max_perms=max_perms, seed=PERM_SEED, strata=strata)
            t.assert_equal(seq, ref, f"{name} h={h}")
        assert ref["stopped"].sum() > 5 and (ref["stopped"] == 0).sum() > 1
    finally:
        ex.close()


# ---- against the kernels that were there before ------------------------------------------------------------------------------


@pytest.mark.parametrize("method,nc,nt,ns", [(1, 70, 61, 3), (2, 33, 31, 1)])
def test_counts_equal_score_sets_when_nothing_stops(method, nc, nt, ns):
    """hits above max_perms: nothing stops, and n_hit is the n_ge of score_sets on a context whose masks came from
    generate_weighted_permutations with the same seed, odds and strata.  The call runs on that context too, and on one
    without masks.  One stratum's odds times 4 -- a power of two, the thresholds do not move -- gives the same bytes."""
    rows, sets, signs, strata = t.make_input(method, nc, nt, ns)
    odds = make_odds(method, nc, nt, ns, strata)
    VT = api.values_table(nc, nt)
    max_perms = 3000
    full = open_context(method, nc, nt, VT, K=max_perms)
    bare = open_context(method, nc, nt, VT)
    try:
        full.generate_weighted_permutations(PERM_SEED, odds, strata)
        drawn = full.weighted_launches()
        want = full.score_sets(sets, rows, signs)
        valid = want["valid"] != 0
        kw = dict(odds=odds, hits=max_perms + 1, max_perms=max_perms, seed=PERM_SEED, strata=strata)
        for ex in (full, bare):
            rec, seq = ex.weighted_sequential_tests(sets, rows, signs, **kw)
            assert not seq["stopped"].any()
            np.testing.assert_array_equal(seq["n_hit"][valid], want["n_ge"][valid])
            assert (seq["n_perm"][valid] == max_perms).all() and (seq["n_hit"][~valid] == -1).all() and (seq["n_perm"][~valid] == -1).all()
            if ex is full:
                assert rec.tobytes() == want.tobytes()               # the records keep the context's own n_ge / pvalue
            else:
                assert np.isnan(rec["pvalue"]).all()
        assert full.weighted_launches() == drawn and bare.weighted_launches() == 0
        scaled = odds.copy()
        scaled[(np.zeros(nc + nt, int) if strata is None else strata) == 0] *= 4.0
        first = bare.weighted_sequential_tests(sets, rows, signs, odds=odds, hits=5, max_perms=max_perms, seed=PERM_SEED, strata=strata)[1]
        again = bare.weighted_sequential_tests(sets, rows, signs, odds=scaled, hits=5, max_perms=max_perms, seed=PERM_SEED, strata=strata)[1]
        assert first.tobytes() == again.tobytes() and first["stopped"].any()
    finally:
        full.close()
        bare.close()


# ---- left-over permutations ------------------------------------------------------------------------------------------------------


def six_patients():
    """3 + 3 patients: nobody, the cases, everybody, and rows in between; the sets that stop early -- every permutation ties
    the score of rows 0, 2 and 3, about 0.4 of them reach that of rows 4, 5 and 6 -- and the set planted on the cases, which
    only the permutation that redraws the cases themselves reaches (about one in sixteen)."""
    rows = np.array([[0, 0, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0], [1, 1, 1, 1, 1, 1], [1, 0, 0, 1, 1, 0], [1, 1, 0, 0, 0, 0], [1, 1, 1, 1, 0, 0],
                     [0, 0, 0, 1, 1, 0]], np.int8)
    early = [[0], [2], [3], [4], [5], [6]]
    return rows, early, [[1] * len(s) for s in early], [1]


def six_reference(method, sets, signs, rows, odds, seed, max_attempts, hits, max_perms):
    VT = api.values_table(3, 3)
    obs, null, valid, att = reference(method, sets, signs, rows, 3, 3, VT, odds, None, max_perms, seed, max_attempts)
    return VT, report.weighted_sequential_reference(null, obs, valid, hits, max_perms, att), valid


@pytest.mark.parametrize("method", [1, 2])
def test_left_over_permutations(monkeypatch, method):
    """None of these provokes a fault: a left-over permutation is an ordinary refusal, or no refusal at all."""
    seed, cap, max_perms, hits = LEFT_OVER
    rows, early, esigns, planted = six_patients()
    lib = api._feature_lib("sequential_weighted")
    # (a) every set stops in front of R: the call returns the truncated reference, whatever the batches
    VT, ref, valid = six_reference(method, early, esigns, rows, SIX, seed, cap, hits, max_perms)
    R = ref["first_left_over"]
    assert R is not None and 512 < R < max_perms and not ref["refused"]
    assert (ref["stopped"] == 1).all() and (ref["n_perm"] <= R).all() and ref["n_perm"][0] == hits
    assert (ref["n_perm"] > 512).any()                               # with 512 a batch, the cut batch itself retires a set
    # (b) the same plus the set planted on the cases, still active at R
    both, bsigns = early + [planted], esigns + [[1]]
    _, bref, bvalid = six_reference(method, both, bsigns, rows, SIX, seed, cap, hits, max_perms)
    assert bref["first_left_over"] == R and bref["refused"] and bref["n_active"] == 1 and bref["stopped"][-1] == 0
    ex = open_context(method, 3, 3, VT)
    try:
        for batch in ("512", None):
            if batch:
                monkeypatch.setenv("GCRE_SEQ_BATCH_PERMS", batch)
            else:
                monkeypatch.delenv("GCRE_SEQ_BATCH_PERMS", raising=False)
            before = ex.sequential_launches()
            rec, seq = ex.weighted_sequential_tests(early, rows, esigns, odds=SIX, hits=hits, max_perms=max_perms, seed=seed, max_attempts=cap)
            t.assert_equal(seq, ref, f"(a) batch={batch}")
            assert ex.sequential_launches() == before + implied_launches(ref, valid, max_perms, dwords_of(3, 3, 1), cap_perms=int(batch or 0))
            before = ex.sequential_launches()
            with pytest.raises(api.GcreError, match=rf"{WHO}permutation {R} has no accepted attempt below max_attempts = {cap} in stratum 0, "
                                                    r"and 1 sets were still active there") as err:
                ex.weighted_sequential_tests(both, rows, bsigns, odds=SIX, hits=hits, max_perms=max_perms, seed=seed, max_attempts=cap)
            assert lib.gcre_last_error(ex._h).decode() in str(err.value)
            # nothing ran past the cut batch: whole batches in front of it, then four kernels (R is not a batch's first permutation)
            want = implied_launches(bref, bvalid, max_perms, dwords_of(3, 3, 1), cap_perms=int(batch or 0))
            assert ex.sequential_launches() == before + want
            if batch:
                assert R % 512 != 0 and want == 4 * (R // 512 + 1)
            else:
                assert want == 4
        # (c) permutation 0 left over: refused behind one launch
        monkeypatch.delenv("GCRE_SEQ_BATCH_PERMS", raising=False)
        zseed, zcap = LEFT_AT_ZERO
        _, zref, _ = six_reference(method, early, esigns, rows, SIX, zseed, zcap, 5, 100)
        assert zref["first_left_over"] == 0 and zref["refused"] and zref["n_active"] == len(early)
        before = ex.sequential_launches()
        with pytest.raises(api.GcreError, match=rf"{WHO}permutation 0 has no accepted attempt below max_attempts = {zcap} in stratum 0, and "
                                                rf"{len(early)} sets were still active"):
            ex.weighted_sequential_tests(early, rows, esigns, odds=SIX, hits=5, max_perms=100, seed=zseed, max_attempts=zcap)
        assert ex.sequential_launches() == before + 1
        # with these odds max_attempts = 1 is below the estimate, about 3 attempts: refused up front, nothing launched ...
        with pytest.raises(api.GcreError, match=WHO + "stratum 0 needs about 3 attempts per permutation, above max_attempts = 1"):
            ex.weighted_sequential_tests(early, rows, esigns, odds=SIX, hits=5, max_perms=100, seed=zseed, max_attempts=1)
        assert ex.sequential_launches() == before + 1
        # ... so max_attempts = 1 meets a left-over permutation only where the estimate is 1: two patients decide the third case
        _, oref, _ = six_reference(method, early, esigns, rows, LEFT_ONE_ODDS, LEFT_AT_ZERO_ONE, 1, 5, 100)
        assert oref["first_left_over"] == 0 and oref["refused"]
        with pytest.raises(api.GcreError, match=WHO + "permutation 0 has no accepted attempt below max_attempts = 1 in stratum 0"):
            ex.weighted_sequential_tests(early, rows, esigns, odds=LEFT_ONE_ODDS, hits=5, max_perms=100, seed=LEFT_AT_ZERO_ONE, max_attempts=1)
        assert ex.sequential_launches() == before + 2
        assert ex.weighted_launches() == 0
    finally:
        ex.close()


def test_a_nan_score_forces_the_refusal(monkeypatch):
    """A set whose observed cell is NaN never stops: with a left-over permutation below max_perms the call is refused, although
    every other set has stopped; without one the set runs to max_perms with no hit."""
    seed, cap, max_perms, hits = LEFT_OVER
    rows, early, esigns, _ = six_patients()
    VT = api.values_table(3, 3).copy()
    VT[1, 2] = np.nan                                               # the observed cell of row 3: one case, two controls
    obs, null, valid, att = reference(1, early, esigns, rows, 3, 3, VT, SIX, None, max_perms, seed, cap)
    assert np.isnan(obs[2]) and np.isnan(obs).sum() == 1
    ref = report.weighted_sequential_reference(null, obs, valid, hits, max_perms, att)
    R = ref["first_left_over"]
    assert ref["refused"] and ref["n_active"] == 1 and ref["stopped"].sum() == len(early) - 1
    ex = open_context(1, 3, 3, VT)
    try:
        with pytest.raises(api.GcreError, match=rf"permutation {R} has no accepted attempt .* and 1 sets were still active"):
            ex.weighted_sequential_tests(early, rows, esigns, odds=SIX, hits=hits, max_perms=max_perms, seed=seed, max_attempts=cap)
        short = R - 1                                               # nothing is left over below this limit
        ref = report.weighted_sequential_reference(null, obs, valid, hits, short, att)
        assert ref["first_left_over"] is None
        rec, seq = ex.weighted_sequential_tests(early, rows, esigns, odds=SIX, hits=hits, max_perms=short, seed=seed, max_attempts=cap)
        t.assert_equal(seq, ref, "NaN")
        assert seq["n_hit"][2] == 0 and seq["n_perm"][2] == short and seq["stopped"][2] == 0
    finally:
        ex.close()


# ---- refusals that launch nothing ------------------------------------------------------------------------------------------


def test_up_front_refusals_launch_nothing():
    nc, nt = 33, 31
    n = nc + nt
    rows, sets, signs, strata = t.make_input(1, nc, nt, 3)
    odds = make_odds(1, nc, nt, 3, strata)
    ex = open_context(1, nc, nt, api.values_table(nc, nt))
    try:
        others = t.other_counters(ex)

        def bad(i, v):
            o = odds.copy()
            o[i] = v
            return o

        few = np.where(np.asarray(strata) == 1, 0.0, odds)            # stratum 1 without a positive odd
        refusals = [
            (dict(odds=bad(4, -1.0)), f"the odds of patient 4 \\(stratum {strata[4]}\\) must be finite and >= 0, not -1.000000"),
            (dict(odds=bad(7, np.nan)), f"the odds of patient 7 \\(stratum {strata[7]}\\) must be finite and >= 0, not nan"),
            (dict(odds=bad(9, np.inf)), f"the odds of patient 9 \\(stratum {strata[9]}\\) must be finite and >= 0, not inf"),
            (dict(odds=few), "stratum 1 has 0 patients with positive odds, fewer than its"),
            (dict(max_attempts=0), "max_attempts = 0 must be at least 1"),
            (dict(max_attempts=2), "stratum [0-2] needs about [0-9]+ attempts per permutation, above max_attempts = 2"),
            (dict(hits=0), "hits = 0 outside 1 .. 2147483647"),
            (dict(max_perms=-1), "max_perms = -1 outside 0 .. 1099511627776"),
        ]
        assert (np.asarray(strata)[:nc] == 1).any()
        for kw, msg in refusals:
            with pytest.raises(api.GcreError, match=WHO + msg):
                ex.weighted_sequential_tests(sets, rows, signs, **{**dict(odds=odds, hits=5, max_perms=100, strata=strata), **kw})
        with pytest.raises(api.GcreError, match="member row"):
            ex.weighted_sequential_tests([[t.N_ROWS]], rows, None, odds=odds, hits=5, max_perms=100)
        # the codes, and a NULL output, as C sees them
        lib = api._feature_lib("sequential_weighted")
        inp, keep = api._set_input(sets, rows, signs, n)
        out = np.zeros(len(sets), api.SET_SCORE)
        seq = np.zeros(len(sets), api.SEQ_SCORE)
        n_out = api.ctypes.c_int64(0)
        ptr = api._ptr
        st = np.ascontiguousarray(strata, np.int32)

        def call(o, max_attempts, seq_out, h=5):
            return lib.gcre_score_sets_sequential_weighted(ex._h, api.ctypes.byref(inp), 1, ptr(o), ptr(st), 3, max_attempts, h, 100, ptr(out),
                                                           len(out), api.ctypes.byref(n_out), ptr(seq_out) if seq_out is not None else None)

        assert call(odds, 1 << 20, None) == ERR_ARG and b"NULL argument (seq_out)" in lib.gcre_last_error(ex._h)
        assert call(None, 1 << 20, seq) == ERR_ARG and b"NULL argument (odds)" in lib.gcre_last_error(ex._h)
        assert call(bad(4, -1.0), 1 << 20, seq) == ERR_ARG and call(odds, 0, seq) == ERR_ARG and call(odds, 2, seq) == ERR_RANGE
        assert call(odds, 1 << 20, seq, h=0) == ERR_ARG
        assert ex.sequential_launches() == 0 and ex.weighted_launches() == 0 and t.other_counters(ex) == others
        # max_perms = 0: nothing of the stage is launched, every valid set gets zeros
        rec, sq = ex.weighted_sequential_tests(sets, rows, signs, odds=odds, hits=5, max_perms=0, strata=strata)
        valid = rec["valid"] != 0
        assert ex.sequential_launches() == 0 and (sq["n_perm"][valid] == 0).all() and (sq["n_perm"][~valid] == -1).all()
        assert call(odds, 1 << 20, seq) == 0 and ex.sequential_launches() == 4
    finally:
        ex.close()


# ---- score_paths -----------------------------------------------------------------------------------------------------------


def test_score_paths_columns():
    """``sequential_weighted=True``: the four columns are ``sequential_columns`` of the reference; every other column is the
    frame without the sequential stage; and the default frame is what it was."""
    nc, nt = 70, 61
    rng = np.random.default_rng(7500)
    genes = [f"G{i}" for i in range(30)]
    data = (rng.random((30, nc + nt)) < rng.uniform(0.1, 0.4, size=(30, 1))).astype(np.int32)
    data[:, :nc] |= (rng.random((30, nc)) < 0.1).astype(np.int32)
    strata = (np.arange(nc + nt) % 2).astype(np.int32) * 4 + 3       # ids 3 and 7
    odds = np.exp(rng.normal(0, 0.8, nc + nt) + 0.3 * (strata == 7))
    paths = ["G1 (+) -> G2 (-) -> G3 (+)", "G4 (+) -> G5 (+)", "G6 (-)", ["G7", "G8", "G9", "G10"], "G1 (+) -> NA (+)", "G11 (+)"]
    for signed in (False, True):
        method = 2 if signed else 1
        kw = dict(signed=signed, threshold=1.0, n_permutations=64, strata=strata, seed=5)
        plain = report.score_paths(paths, genes, data, nc, nt, **kw)
        assert plain.equals(report.score_paths(paths, genes, data, nc, nt, sequential_weighted=False, **kw))
        base = report.score_paths(paths, genes, data, nc, nt, case_odds=odds, **kw)
        got = report.score_paths(paths, genes, data, nc, nt, case_odds=odds, sequential=2000, sequential_hits=4, sequential_weighted=True, **kw)
        assert list(got.columns) == report.SCORE_PATHS_COLUMNS + report.SEQUENTIAL_COLUMNS
        assert got[report.SCORE_PATHS_COLUMNS].equals(base)
        g2, d2 = report.preprocess_table(genes, data, 1.0, nc, nt)
        _, rows, signs = report.parse_sets(paths, g2)
        obs, null, valid, att = reference(method, rows, signs, d2, nc, nt, api.values_table(nc, nt), odds, strata, 2000, 5)
        ref = report.weighted_sequential_reference(null, obs, valid, 4, 2000, att)
        assert not ref["refused"]
        want = report.sequential_columns(ref, valid)
        for k in report.SEQUENTIAL_COLUMNS:
            np.testing.assert_array_equal(got[k].to_numpy(), want[k], err_msg=k)
        assert np.isnan(got["SequentialPvalues"][4]) and (got["SequentialPerms"][[0, 1, 2, 3, 5]] > 0).all()
        with pytest.raises(ValueError, match="case_odds: sequential p-values draw their own uniform masks"):
            report.score_paths(paths, genes, data, nc, nt, case_odds=odds, sequential=2000, **kw)


# ---- a seeded fuzz -----------------------------------------------------------------------------------------------------


def fuzz_case(i):
    """Case i of the fuzz: the input, the call and what the definition gives -- (what, mismatch or None, reference)."""
    from test_gpu_weighted import PATTERNS, odds_pattern
    rng = np.random.default_rng([7800, i])
    method = int(rng.integers(1, 3))
    nc, nt = int(rng.integers(1, 91)), int(rng.integers(1, 91))
    n = nc + nt
    ns = int(rng.integers(1, 17))
    strata = None if ns == 1 else rng.integers(0, ns, n) * 3 - 7
    odds = odds_pattern(PATTERNS[i % 4], rng, nc, nt)
    if strata is not None:
        odds[:nc] = np.where(odds[:nc] > 0, odds[:nc], 1.0)             # every stratum keeps enough positive odds
    n_rows = int(rng.integers(1, 40))
    rows = (rng.random((n_rows, n)) < rng.uniform(0.0, 0.6, size=(n_rows, 1))).astype(np.int8)
    rows[:, :nc] |= (rng.random((n_rows, nc)) < rng.uniform(0.0, 0.3)).astype(np.int8)
    S = int(rng.integers(1, 41))
    sets = [rng.integers(0, n_rows, int(rng.integers(1, 6))).tolist() for _ in range(S)]
    if rng.random() < 0.3:
        sets[int(rng.integers(0, S))][0] = -1
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    h = int(rng.integers(1, 31))
    max_perms = int(rng.integers(0, 3001))
    cap = int(rng.choice([0, 1, 512, 700, 1024, 2048]))
    seed = int(rng.integers(0, 2**63))
    VT = api.values_table(nc, nt)
    obs, null, valid, att = reference(method, sets, signs, rows, nc, nt, VT, odds, strata, max_perms, seed)
    ref = report.weighted_sequential_reference(null, obs, valid, h, max_perms, att)
    what = f"case {i}: method {method}, {nc}+{nt} patients, {ns} strata, {PATTERNS[i % 4]} odds, {S} sets, h={h}, max_perms={max_perms}, cap={cap}"
    if ref["refused"]:                                                # (the cap is 2^20: not met at these sizes)
        return what, "the reference is refused", ref
    if cap:
        os.environ["GCRE_SEQ_BATCH_PERMS"] = str(cap)
    else:
        os.environ.pop("GCRE_SEQ_BATCH_PERMS", None)
    ex = open_context(method, nc, nt, VT)
    try:
        rec, seq = ex.weighted_sequential_tests(sets, rows, signs, odds=odds, hits=h, max_perms=max_perms, seed=seed, strata=strata)
    finally:
        ex.close()
        os.environ.pop("GCRE_SEQ_BATCH_PERMS", None)
    for k in ("n_hit", "n_perm", "stopped"):
        if not np.array_equal(seq[k], ref[k]):
            return what, f"{k}: sets {np.flatnonzero(seq[k] != ref[k]).tolist()[:8]}", ref
    return what, None, ref


def test_fuzz_against_the_definition():
    """GCRE_SEQ_WEIGHTED_FUZZ_CASES seeded cases (default 12, a few seconds): cohorts of 1-90 + 1-90 patients, 1-16 strata, the
    odds patterns of tests/test_gpu_weighted.py, 1-40 sets, 1-30 hits, 0-3,000 permutations, a random batch cap, both methods."""
    cases = int(os.environ.get("GCRE_SEQ_WEIGHTED_FUZZ_CASES", "12"))
    stopped = total = 0
    for i in range(cases):
        what, bad, ref = fuzz_case(i)
        print(what)
        assert bad is None, f"{what}: {bad}"
        stopped += int(ref["stopped"].sum())
        total += int((ref["n_hit"] >= 0).sum())
    print(f"weighted sequential fuzz: {cases} cases, {total} valid sets, {stopped} stopped, every count equal")
    assert cases == 0 or 0 < stopped
