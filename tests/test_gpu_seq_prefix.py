"""Sequential p-values of the variable-threshold and the multi-hit tests on the device (gcre_score_sets_prefix_sequential,
gcre_score_sets_dose_sequential: k_seq_prefix_null between the step rows and the batches).  Every count
``JoinExec.prefix_sequential_tests`` and ``dose_sequential_tests`` return is compared as an integer, for every set, with the
definition in numpy alone: ``report.permutation_masks`` / ``report.weighted_masks``, the null scores of every step row through
the value table, ``report.adaptive_sequential_reference``.  The cohorts are 70 + 61 patients (five dwords: neither a dword nor
a qword multiple) and 33 + 31, without strata, with 3 and with 7; the sets put one-step sets, 3-5-step sets and two 60-step
sets into the same groups of four; the batches are cut at 512 and 1,024 permutations, by bytes and not at all, the sets walked
in one slab and in many, and no value may move."""
from __future__ import annotations

import os

import numpy as np
import pytest

from geneticscre_amd import api, report
import test_gpu_sequential as t
import test_gpu_seq_weighted as tw

pytestmark = pytest.mark.gpu

PERM_SEED = t.PERM_SEED
HITS, CAP, P_MAX = t.HITS, t.CAP, t.P_MAX
ENV = ("GCRE_SEQ_MAX_MB", "GCRE_SEQ_BATCH_PERMS", "GCRE_PREFIX_SLAB_SETS", "GCRE_PREFIX_MAX_MB")
DOSE_LEVELS = (1, 2, 3)
COUNTERS = t.COUNTERS + [("sequential", "gcre_sequential_launches"), ("strata", "gcre_strata_launches")]

# (kind, method, cases, controls, strata) -> (the trial of make_input, max_perms): found on the CPU by tools/seq_prefix_seeds.py
# so that the reference alone puts a set into every class of test_gpu_sequential.classes_of at HITS hits and CAP permutations a
# batch; no max_perms is a multiple of 512, so the last tile is partly live
CLASS_CASES = {
    ("prefix", 1, 70, 61, 1): (264, 13405),
    ("prefix", 1, 70, 61, 3): (52, 1486),
    ("prefix", 1, 33, 31, 1): (113, 16818),
    ("prefix", 1, 33, 31, 3): (25, 14638),
    ("prefix", 2, 70, 61, 1): (57, 9562),
    ("prefix", 2, 70, 61, 3): (40, 14896),
    ("prefix", 2, 33, 31, 1): (17, 17082),
    ("prefix", 2, 33, 31, 3): (0, 9642),
    ("dose", 1, 70, 61, 1): (80, 18819),
    ("dose", 1, 70, 61, 3): (64, 11444),
    ("dose", 1, 33, 31, 1): (66, 5966),
    ("dose", 1, 33, 31, 3): (143, 13877),
    ("dose", 2, 70, 61, 1): (6, 7723),
    ("dose", 2, 70, 61, 3): (19, 17339),
    ("dose", 2, 33, 31, 1): (17, 19289),
    ("dose", 2, 33, 31, 3): (0, 8024),
}


def other_counters(ex):
    """Every launch counter of the context but the stage's own."""
    return [int(getattr(api._feature_lib(f), sym)(ex._h)) for f, sym in COUNTERS]


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)


def make_cuts(sets, trial=0):
    """One flag per member: every member a cut, but for set 13 (3-5 members), whose cuts are all zero but one -- and its last
    member, which always ends a step."""
    cuts = [[1] * len(s) for s in sets]
    cuts[13] = [0] * len(sets[13])
    cuts[13][0] = 1
    return cuts


def make_input(kind, method, nc, nt, ns, trial=0):
    """test_gpu_sequential.make_input -- 37 sets (no multiple of 4) on 90 gene rows: twelve one-gene sets, eighteen of 3 to 5,
    two of 60 members, a duplicate, an NA member, a set without carriers, a set planted on the cases -- with the cuts of
    ``make_cuts`` (prefix: the 60-member sets are 15 step tiles in method 1 and 30 in method 2) or DOSE_LEVELS (dose)."""
    rows, sets, signs, strata = t.make_input(method, nc, nt, ns, trial)
    return rows, sets, signs, strata, (make_cuts(sets, trial) if kind == "prefix" else DOSE_LEVELS)


def step_lists(kind, method, sets, signs, rows, extra):
    """(step_rows, step_sets, step_signs, step_set): the steps or levels of every set as sets of their own."""
    if kind == "prefix":
        step_sets, step_signs, owner = report.prefix_sets(sets, signs, extra)
        return rows, step_sets, step_signs, owner
    level_rows, level_sets, level_signs, owner = report.dose_sets(sets, rows, signs, extra, method == 2)
    return level_rows, level_sets, level_signs, owner


def step_null(kind, method, sets, signs, rows, extra, nc, VT, masks):
    """(step_obs, step_null float32 [steps][perms], step_set, valid [sets]) under the given masks, in numpy."""
    srows, ssets, ssigns, owner = step_lists(kind, method, sets, signs, rows, extra)
    obs, null, _ = t.reference_null(method, ssets, ssigns, srows, nc, VT, masks)
    valid = np.array([int(all(m >= 0 for m in s)) for s in sets])
    return obs, null, owner, valid


def call(ex, kind, sets, rows, signs, extra, **kw):
    if kind == "prefix":
        return ex.prefix_sequential_tests(sets, rows, signs, cuts=extra, **kw)
    return ex.dose_sequential_tests(sets, rows, signs, levels=extra, **kw)


def n_steps(kind, sets, extra):
    if kind == "dose":
        return [len(extra)] * len(sets)
    return [sum(1 for i in range(len(s)) if extra[k][i] or i + 1 == len(s)) for k, s in enumerate(sets)]


def slab_walk(valid, steps, slab_sets):
    """The slabs of gcre_prefix.h where only GCRE_PREFIX_SLAB_SETS bounds them: lists of set indices."""
    vs = [s for s in range(len(valid)) if valid[s]]
    if not slab_sets:
        return [vs] if vs else []
    return [vs[i:i + slab_sets] for i in range(0, len(vs), slab_sets)]


def implied_launches(ref, valid, slabs, max_perms, cap, weighted=False):
    """Sum over the slabs of 3 + 3 batches (4 weighted): a slab's loop runs until its last set with a score has stopped, or to
    max_perms; whole batches of ``cap`` permutations."""
    total = 0
    for slab in slabs:
        total += 3
        if max_perms == 0:
            total -= 3
            continue
        live = [s for s in slab if ref["score"][s] == ref["score"][s] or weighted]
        if not live:
            continue
        last = max_perms if any(ref["stopped"][s] == 0 for s in live) else max(int(ref["n_perm"][s]) for s in live)
        total += (4 if weighted else 3) * ((last + cap - 1) // cap)
    return total


_NULLS = {}


def problem(kind, method, nc, nt, ns, trial=0):
    """The input of a configuration and its reference step null over P_MAX permutations: computed once, never changed."""
    key = (kind, method, nc, nt, ns, trial)
    if key not in _NULLS:
        rows, sets, signs, strata, extra = make_input(kind, method, nc, nt, ns, trial)
        VT = api.values_table(nc, nt)
        masks = report.permutation_masks(nc, nt, P_MAX, PERM_SEED, strata)
        obs, null, owner, valid = step_null(kind, method, sets, signs, rows, extra, nc, VT, masks)
        for a in (obs, null, owner, valid):
            a.setflags(write=False)
        _NULLS[key] = (rows, sets, signs, strata, extra, VT, obs, null, owner, valid)
    return _NULLS[key]


def reference(p, hits, max_perms, attempts=None):
    rows, sets, signs, strata, extra, VT, obs, null, owner, valid = p
    return report.adaptive_sequential_reference(obs, null, owner, len(sets), valid, hits, max_perms, attempts)


CONFIGS = [(k, m, nc, nt, ns) for k in ("prefix", "dose") for m in (1, 2) for nc, nt in ((70, 61), (33, 31)) for ns in (1, 3)]


# ---- every class of set, every set as integers -----------------------------------------------------------------------------


@pytest.mark.parametrize("kind,method,nc,nt,ns", CONFIGS)
def test_every_class_of_set(monkeypatch, kind, method, nc, nt, ns):
    trial, max_perms = CLASS_CASES[(kind, method, nc, nt, ns)]
    assert max_perms % 512 != 0
    p = problem(kind, method, nc, nt, ns, trial)
    rows, sets, signs, strata, extra, VT, obs, null, owner, valid = p
    ref = reference(p, HITS, max_perms)
    found = t.classes_of(ref, valid, max_perms, CAP)
    print(found)
    assert all(v > 0 for v in found.values()), found                 # from the reference alone: the input covers every class
    assert ref["n_perm"][34] == HITS and ref["stopped"][34] == 1     # no carriers: every permutation ties the score
    assert ref["n_hit"][35] == 0 and ref["stopped"][35] == 0         # planted on the cases: never reached
    assert ref["n_hit"][33] == -1 and ref["n_perm"][33] == -1        # an NA member
    assert ref["n_perm"][32] == ref["n_perm"][14]                    # the duplicate
    steps = n_steps(kind, sets, extra)
    if kind == "prefix":
        assert steps[30] == 60 and steps[31] == 60 and steps[0] == 1 and steps[13] == 2 and len(sets) % 4 != 0
    monkeypatch.setenv("GCRE_SEQ_BATCH_PERMS", str(CAP))
    ex = t.open_context(method, nc, nt, VT)
    try:
        plain = ex.score_sets(sets, rows, signs)
        others = other_counters(ex)
        assert ex.seq_prefix_launches() == 0
        rec, px, seq = call(ex, kind, sets, rows, signs, extra, hits=HITS, max_perms=max_perms, seed=PERM_SEED, strata=strata)
        assert rec.tobytes() == plain.tobytes()                       # the records of score_sets
        assert seq.dtype == api.SEQ_SCORE and len(seq) == len(sets)
        ok = valid != 0
        np.testing.assert_array_equal(px["score"][ok], ref["score"][ok])
        np.testing.assert_array_equal(px["best_step" if kind == "prefix" else "best_index"][ok], ref["best_step"][ok])
        np.testing.assert_array_equal(px["n_ge"], np.where(ok, 0, -1))
        t.assert_equal(seq, ref, f"{(kind, method, nc, nt, ns)}")
        assert ex.seq_prefix_launches() == implied_launches(ref, valid, slab_walk(valid, steps, 0), max_perms, CAP)
        assert other_counters(ex) == others
    finally:
        ex.close()


# ---- nothing depends on the schedule or the slabs --------------------------------------------------------------------------------


@pytest.mark.parametrize("kind,method,nc,nt,ns", [("prefix", 1, 70, 61, 1), ("prefix", 2, 33, 31, 3), ("dose", 2, 70, 61, 3),
                                                   ("dose", 1, 33, 31, 1)])
def test_no_value_depends_on_the_batches_or_the_slabs(monkeypatch, kind, method, nc, nt, ns):
    """hits x max_perms x batch cap x slabs: against the reference, so equal to each other; the launches are three per slab and
    three per batch of every slab."""
    p = problem(kind, method, nc, nt, ns, CLASS_CASES[(kind, method, nc, nt, ns)][0])
    rows, sets, signs, strata, extra, VT, obs, null, owner, valid = p
    steps = n_steps(kind, sets, extra)
    W32p = tw.dwords_of(nc, nt, 0)
    # GCRE_PREFIX_MAX_MB small enough for several slabs: room for 70 step rows
    small_mb = 70 * method * W32p * 4 / 1048576.0
    ex = t.open_context(method, nc, nt, VT)
    try:
        others = other_counters(ex)
        for h in (1, 5, 20):
            for max_perms in (0, 700, 3000, P_MAX):
                ref = reference(p, h, max_perms)
                for cap, mb in (("512", None), ("1024", None), (None, None), (None, "0.01")):
                    for slab_sets, slab_mb in ((None, None), ("1", None), ("3", None), (None, repr(small_mb))):
                        if (cap, mb) != ("512", None) and slab_sets == "1":
                            continue                                   # (37 slabs: once per hits and max_perms is enough)
                        for var, val in (("GCRE_SEQ_BATCH_PERMS", cap), ("GCRE_SEQ_MAX_MB", mb), ("GCRE_PREFIX_SLAB_SETS", slab_sets),
                                         ("GCRE_PREFIX_MAX_MB", slab_mb)):
                            if val is None:
                                monkeypatch.delenv(var, raising=False)
                            else:
                                monkeypatch.setenv(var, val)
                        before = ex.seq_prefix_launches()
                        rec, px, seq = call(ex, kind, sets, rows, signs, extra, hits=h, max_perms=max_perms, seed=PERM_SEED, strata=strata)
                        what = f"h={h} max_perms={max_perms} cap={cap} mb={mb} slab_sets={slab_sets} slab_mb={slab_mb}"
                        t.assert_equal(seq, ref, what)
                        if max_perms == 0:
                            assert ex.seq_prefix_launches() == before, what
                        elif cap is not None and slab_mb is None:
                            want = implied_launches(ref, valid, slab_walk(valid, steps, int(slab_sets or 0)), max_perms, int(cap))
                            assert ex.seq_prefix_launches() == before + want, what
        assert other_counters(ex) == others
    finally:
        ex.close()


@pytest.mark.parametrize("kind,method", [("prefix", 1), ("prefix", 2), ("dose", 1), ("dose", 2)])
def test_seven_strata_and_nan_steps(monkeypatch, kind, method):
    """More strata than k_seq_masks keeps in registers, and a table with NaN cells: a one-step set whose only step is NaN (a
    NaN score: never counts, never stops), and a set with one NaN step among others (skipped for the pick, inside the null
    maximum)."""
    nc, nt, ns = 70, 61, 7
    rows, sets, signs, strata, extra = make_input(kind, method, nc, nt, ns)
    VT = api.values_table(nc, nt).copy()
    d = rows != 0
    signs[3] = [1]
    signs[13] = [1] * len(sets[13])
    g, g2 = sets[3][0], sets[13][0]
    VT[int(d[g, :nc].sum()), int(d[g, nc:].sum())] = np.nan          # set 3: its one gene
    VT[int(d[g2, :nc].sum()), int(d[g2, nc:].sum())] = np.nan        # set 13: its first step / level 1 of its first gene alone
    if kind == "dose":
        extra = (1,)                                                  # one level: set 3 is all NaN
    masks = report.permutation_masks(nc, nt, 3000, PERM_SEED, strata)
    obs, null, owner, valid = step_null(kind, method, sets, signs, rows, extra, nc, VT, masks)
    ex = t.open_context(method, nc, nt, VT)
    try:
        for h, max_perms, cap, slab in ((5, 3000, "512", None), (1, 1500, None, "5"), (20, 2999, "1024", None)):
            for var, val in (("GCRE_SEQ_BATCH_PERMS", cap), ("GCRE_PREFIX_SLAB_SETS", slab)):
                if val is None:
                    monkeypatch.delenv(var, raising=False)
                else:
                    monkeypatch.setenv(var, val)
            ref = report.adaptive_sequential_reference(obs, null, owner, len(sets), valid, h, max_perms)
            assert np.isnan(ref["score"][3]) and np.isnan(ref["score"]).sum() < 8
            rec, px, seq = call(ex, kind, sets, rows, signs, extra, hits=h, max_perms=max_perms, seed=PERM_SEED, strata=strata)
            t.assert_equal(seq, ref, f"h={h} max_perms={max_perms}")
            assert np.isnan(px["score"][3]) and px["best_step" if kind == "prefix" else "best_index"][3] == -1
            assert seq["n_hit"][3] == 0 and seq["n_perm"][3] == max_perms and seq["stopped"][3] == 0
            if kind == "prefix":
                assert np.isnan(obs[np.flatnonzero(owner == 13)[0]]) and px["best_step"][13] == 1
    finally:
        ex.close()


@pytest.mark.parametrize("method,levels", [(1, (2,)), (2, (2,)), (1, tuple(range(1, 16))), (2, tuple(range(1, 16)))])
def test_one_level_and_fifteen(monkeypatch, method, levels):
    nc, nt, ns = 33, 31, 3
    rows, sets, signs, strata, _ = make_input("dose", method, nc, nt, ns)
    VT = api.values_table(nc, nt)
    max_perms = 2500
    masks = report.permutation_masks(nc, nt, max_perms, PERM_SEED, strata)
    obs, null, owner, valid = step_null("dose", method, sets, signs, rows, levels, nc, VT, masks)
    ref = report.adaptive_sequential_reference(obs, null, owner, len(sets), valid, HITS, max_perms)
    monkeypatch.setenv("GCRE_SEQ_BATCH_PERMS", "1024")
    ex = t.open_context(method, nc, nt, VT)
    try:
        rec, ds, seq, lsc = ex.dose_sequential_tests(sets, rows, signs, levels=levels, hits=HITS, max_perms=max_perms, seed=PERM_SEED,
                                                     strata=strata, level_scores=True)
        t.assert_equal(seq, ref, f"levels={levels}")
        ok = valid != 0
        np.testing.assert_array_equal(lsc[ok].reshape(-1), obs[np.isin(owner, np.flatnonzero(ok))])
        assert (ds["levels"] == len(levels)).all()
    finally:
        ex.close()


# ---- against the kernels that were there before ------------------------------------------------------------------------------


@pytest.mark.parametrize("method,nc,nt,ns", [(1, 70, 61, 3), (2, 70, 61, 1), (2, 33, 31, 3), (1, 70, 61, 7)])
def test_counts_equal_the_resident_road_when_nothing_stops(method, nc, nt, ns):
    """hits above max_perms: nothing stops, and n_hit is the n_ge of prefix_tests / dose_tests on a context that holds
    permutations 0 .. max_perms-1 of generate_permutations(seed, strata); every other field of the records is equal."""
    rows, sets, signs, strata, cuts = make_input("prefix", method, nc, nt, ns)
    VT = api.values_table(nc, nt)
    max_perms = 3000
    full = t.open_context(method, nc, nt, VT, K=max_perms, seed=PERM_SEED, strata=strata)
    bare = t.open_context(method, nc, nt, VT)
    try:
        plain = full.score_sets(sets, rows, signs)
        valid = plain["valid"] != 0
        want_px = full.prefix_tests(sets, rows, signs, cuts=cuts, steps=True)
        want_ds = full.dose_tests(sets, rows, signs, levels=DOSE_LEVELS, level_scores=True)
        for ex in (full, bare):
            for want, got in ((want_px, ex.prefix_sequential_tests(sets, rows, signs, cuts=cuts, hits=max_perms + 1, max_perms=max_perms,
                                                                   seed=PERM_SEED, strata=strata, steps=True)),
                              (want_ds, ex.dose_sequential_tests(sets, rows, signs, levels=DOSE_LEVELS, hits=max_perms + 1,
                                                                 max_perms=max_perms, seed=PERM_SEED, strata=strata, level_scores=True))):
                rec, px, seq, sc = got
                assert not seq["stopped"].any()
                np.testing.assert_array_equal(seq["n_hit"][valid], want[1]["n_ge"][valid])
                assert (seq["n_perm"][valid] == max_perms).all() and (seq["n_hit"][~valid] == -1).all() and (seq["n_perm"][~valid] == -1).all()
                for name in px.dtype.names:
                    if name != "n_ge":
                        np.testing.assert_array_equal(px[name], want[1][name], err_msg=name)
                np.testing.assert_array_equal(px["n_ge"], np.where(valid, 0, -1))
                np.testing.assert_array_equal(sc, want[2])
                if ex is full:
                    assert rec.tobytes() == plain.tobytes()
                else:
                    for name in rec.dtype.names:
                        if name not in ("n_ge", "pvalue"):
                            np.testing.assert_array_equal(rec[name], plain[name], err_msg=name)
    finally:
        full.close()
        bare.close()


@pytest.mark.parametrize("method,nc,nt,ns", [(1, 70, 61, 1), (2, 33, 31, 3)])
def test_level_one_and_a_single_step_are_sequential_tests(monkeypatch, method, nc, nt, ns):
    """Level 1 is the set's union and so is the one step of a set whose cuts are all zero."""
    rows, sets, signs, strata, _ = make_input("prefix", method, nc, nt, ns)
    VT = api.values_table(nc, nt)
    monkeypatch.setenv("GCRE_SEQ_BATCH_PERMS", "1024")
    ex = t.open_context(method, nc, nt, VT)
    try:
        rec, want = ex.sequential_tests(sets, rows, signs, hits=HITS, max_perms=5000, seed=PERM_SEED, strata=strata)
        assert want["stopped"].any() and not want["stopped"].all()
        _, ds, seq = ex.dose_sequential_tests(sets, rows, signs, levels=(1,), hits=HITS, max_perms=5000, seed=PERM_SEED, strata=strata)
        assert seq.tobytes() == want.tobytes()
        np.testing.assert_array_equal(ds["score"], rec["score"])
        _, px, seq = ex.prefix_sequential_tests(sets, rows, signs, cuts=[[0] * len(s) for s in sets], hits=HITS, max_perms=5000,
                                                seed=PERM_SEED, strata=strata)
        assert seq.tobytes() == want.tobytes()
        np.testing.assert_array_equal(px["score"], rec["score"])
        assert (px["steps"] == 1).all()
    finally:
        ex.close()


# ---- weighted permutations ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind,method,nc,nt,ns", [("prefix", 1, 70, 61, 1), ("dose", 2, 33, 31, 3), ("prefix", 2, 33, 31, 3),
                                                   ("dose", 1, 70, 61, 1)])
def test_weighted_masks(monkeypatch, kind, method, nc, nt, ns):
    """The cohorts and odds of test_gpu_seq_weighted.py, one and three strata: the null under report.weighted_masks."""
    rows, sets, signs, strata, extra = make_input(kind, method, nc, nt, ns)
    odds = tw.make_odds(method, nc, nt, ns, strata)
    VT = api.values_table(nc, nt)
    max_perms = 3000
    thr, _ = api.weighted_thresholds(odds, nc, nt, strata)
    masks, att = report.weighted_masks(thr, nc, nt, max_perms, PERM_SEED, strata)
    obs, null, owner, valid = step_null(kind, method, sets, signs, rows, extra, nc, VT, masks)
    steps = n_steps(kind, sets, extra)
    ex = t.open_context(method, nc, nt, VT)
    try:
        others = other_counters(ex)
        for h, cap, slab in ((HITS, "512", None), (20, "1024", "3"), (max_perms + 1, None, None)):
            for var, val in (("GCRE_SEQ_BATCH_PERMS", cap), ("GCRE_PREFIX_SLAB_SETS", slab)):
                if val is None:
                    monkeypatch.delenv(var, raising=False)
                else:
                    monkeypatch.setenv(var, val)
            ref = report.adaptive_sequential_reference(obs, null, owner, len(sets), valid, h, max_perms, attempts=att)
            assert ref["first_left_over"] is None and not ref["refused"]
            before = ex.seq_prefix_launches()
            rec, px, seq = call(ex, kind, sets, rows, signs, extra, hits=h, max_perms=max_perms, seed=PERM_SEED, strata=strata, odds=odds)
            t.assert_equal(seq, ref, f"h={h} cap={cap} slab={slab}")
            if cap:
                want = implied_launches(ref, valid, slab_walk(valid, steps, int(slab or 0)), max_perms, int(cap), weighted=True)
                assert ex.seq_prefix_launches() == before + want
        assert other_counters(ex) == others and ex.weighted_launches() == 0
    finally:
        ex.close()


@pytest.mark.parametrize("kind,method", [("prefix", 1), ("prefix", 2), ("dose", 1), ("dose", 2)])
def test_left_over_permutations_across_slabs(monkeypatch, kind, method):
    """The six patients of test_gpu_seq_weighted.py: a left-over permutation R with every set stopped in front of it
    (returned), and with the planted set in each of two slabs still active (refused: the message sums them)."""
    seed, cap, max_perms, hits = tw.LEFT_OVER
    rows, early, esigns, planted = tw.six_patients()
    extra = [[1] * len(s) for s in early] if kind == "prefix" else (1,)
    who = f"score_sets_{kind}_sequential: "
    VT = api.values_table(3, 3)
    thr, _ = api.weighted_thresholds(tw.SIX, 3, 3, None)
    masks, att = report.weighted_masks(thr, 3, 3, max_perms, seed, None, max_attempts=cap)

    def ref_of(sets, signs, ext):
        obs, null, owner, valid = step_null(kind, method, sets, signs, rows, ext, 3, VT, masks)
        return report.adaptive_sequential_reference(obs, null, owner, len(sets), valid, hits, max_perms, attempts=att)

    ref = ref_of(early, esigns, extra)
    R = ref["first_left_over"]
    assert R is not None and 512 < R < max_perms and not ref["refused"] and (ref["stopped"] == 1).all()
    # the planted set first and last: with two sets a slab, one is still active in the first slab and one in the last
    both, bsigns = [planted] + early + [planted], [[1]] + esigns + [[1]]
    bextra = [[1]] + extra + [[1]] if kind == "prefix" else extra
    bref = ref_of(both, bsigns, bextra)
    assert bref["first_left_over"] == R and bref["refused"] and bref["n_active"] == 2
    lib = api._feature_lib("seq_prefix")
    ex = t.open_context(method, 3, 3, VT)
    try:
        for batch, slab in (("512", None), (None, "4"), ("512", "4")):
            for var, val in (("GCRE_SEQ_BATCH_PERMS", batch), ("GCRE_PREFIX_SLAB_SETS", slab)):
                if val is None:
                    monkeypatch.delenv(var, raising=False)
                else:
                    monkeypatch.setenv(var, val)
            rec, px, seq = call(ex, kind, early, rows, esigns, extra, odds=tw.SIX, hits=hits, max_perms=max_perms, seed=seed, max_attempts=cap)
            t.assert_equal(seq, ref, f"(a) batch={batch} slab={slab}")
            with pytest.raises(api.GcreError, match=rf"{who}permutation {R} has no accepted attempt below max_attempts = {cap} in stratum 0, "
                                                    r"and 2 sets were still active there") as err:
                call(ex, kind, both, rows, bsigns, bextra, odds=tw.SIX, hits=hits, max_perms=max_perms, seed=seed, max_attempts=cap)
            assert lib.gcre_last_error(ex._h).decode() in str(err.value)
        # seq stays untouched by the refused call: straight through the C entry
        inp, keep = api._set_input(both, rows, bsigns, 6)
        n = len(both)
        out, px, seq = np.zeros(n, api.SET_SCORE), np.zeros(n, api.PREFIX_SCORE if kind == "prefix" else api.DOSE_SCORE), np.zeros(n, api.SEQ_SCORE)
        seq["n_hit"] = 77
        w = np.ascontiguousarray(tw.SIX, np.float64)
        n_out = api.ctypes.c_int64(0)
        if kind == "prefix":
            rc = lib.gcre_score_sets_prefix_sequential(ex._h, api.ctypes.byref(inp), None, seed, api._ptr(w), None, 0, cap, hits, max_perms,
                                                       api._ptr(out), n, api.ctypes.byref(n_out), api._ptr(px), api._ptr(seq), None)
        else:
            lv = np.array([1], np.int32)
            rc = lib.gcre_score_sets_dose_sequential(ex._h, api.ctypes.byref(inp), api._ptr(lv), 1, seed, api._ptr(w), None, 0, cap, hits,
                                                     max_perms, api._ptr(out), n, api.ctypes.byref(n_out), api._ptr(px), api._ptr(seq), None)
        assert rc == api.GCRE_ERR_RANGE
        assert (seq["n_hit"] == 0).all() and (seq["n_perm"] == 0).all() and (seq["stopped"] == 0).all()   # its defaults
        # the context stays usable
        rec, px, seq = call(ex, kind, early, rows, esigns, extra, odds=tw.SIX, hits=hits, max_perms=max_perms, seed=seed, max_attempts=cap)
        t.assert_equal(seq, ref, "after the refusal")
    finally:
        ex.close()


# ---- the report functions ---------------------------------------------------------------------------------------------------------


def test_report_columns():
    """``sequential=0`` is the frame as it was; with a limit the four columns are ``sequential_columns`` of the reference."""
    nc, nt = 70, 61
    rng = np.random.default_rng(7600)
    genes = [f"G{i}" for i in range(30)]
    data = (rng.random((30, nc + nt)) < rng.uniform(0.1, 0.4, size=(30, 1))).astype(np.int32)
    data[:, :nc] |= (rng.random((30, nc)) < 0.1).astype(np.int32)
    strata = (np.arange(nc + nt) % 2).astype(np.int32)
    paths = ["G1 (+) -> G2 (-) -> G3 (+)", "G4 (+) -> G5 (+)", "G6 (-)", ["G7", "G8", "G9", "G10"], "G1 (+) -> NA (+)", "G11 (+)"]
    VT = api.values_table(nc, nt)
    masks = report.permutation_masks(nc, nt, 3000, 5, strata)
    for signed in (False, True):
        method = 2 if signed else 1
        kw = dict(signed=signed, threshold=1.0, n_permutations=64, strata=strata, seed=5)
        g2, d2 = report.preprocess_table(genes, data, 1.0, nc, nt)
        names_of, rows, signs = report.parse_sets(paths, g2)
        # the variable-threshold test
        base = report.variable_threshold_test(paths, genes, data, nc, nt, **kw)
        same = report.variable_threshold_sequential_test(paths, genes, data, nc, nt, sequential=0, **kw)
        assert list(base.columns) == report.VARIABLE_THRESHOLD_COLUMNS and base.equals(same)
        got = report.variable_threshold_sequential_test(paths, genes, data, nc, nt, sequential=3000, sequential_hits=4, **kw)
        assert list(got.columns) == report.VARIABLE_THRESHOLD_COLUMNS + report.SEQUENTIAL_COLUMNS
        assert got[report.VARIABLE_THRESHOLD_COLUMNS].equals(base)
        osets, osigns, cuts = [], [], []
        for rs, sg in zip(rows, signs):
            order, ct = report.threshold_order(rs, np.asarray(d2))
            osets.append(np.asarray(rs, np.int64)[order].tolist())
            osigns.append(np.asarray(sg, np.int64)[order].tolist())
            cuts.append(ct.tolist())
        obs, null, owner, valid = step_null("prefix", method, osets, osigns, np.asarray(d2), cuts, nc, VT, masks)
        want = report.sequential_columns(report.adaptive_sequential_reference(obs, null, owner, len(osets), valid, 4, 3000), valid)
        for k in report.SEQUENTIAL_COLUMNS:
            np.testing.assert_array_equal(got[k].to_numpy(), want[k], err_msg=k)
        # the multi-hit test
        base = report.multi_hit_test(paths, genes, data, nc, nt, levels=(1, 2), **kw)
        same = report.multi_hit_sequential_test(paths, genes, data, nc, nt, levels=(1, 2), sequential=0, **kw)
        assert list(base.columns) == report.MULTI_HIT_COLUMNS and base.equals(same)
        got = report.multi_hit_sequential_test(paths, genes, data, nc, nt, levels=(1, 2), sequential=3000, sequential_hits=4, **kw)
        assert list(got.columns) == report.MULTI_HIT_COLUMNS + report.SEQUENTIAL_COLUMNS
        assert got[report.MULTI_HIT_COLUMNS].equals(base)
        obs, null, owner, valid = step_null("dose", method, rows, signs, np.asarray(d2), (1, 2), nc, VT, masks)
        want = report.sequential_columns(report.adaptive_sequential_reference(obs, null, owner, len(rows), valid, 4, 3000), valid)
        for k in report.SEQUENTIAL_COLUMNS:
            np.testing.assert_array_equal(got[k].to_numpy(), want[k], err_msg=k)
        assert np.isnan(got["SequentialPvalues"][4]) and (got["SequentialPerms"][[0, 1, 2, 3, 5]] > 0).all()


# ---- seeded fuzz against the definition ------------------------------------------------------------------------------------------------


def fuzz_case(i):
    rng = np.random.default_rng([7700, i])
    kind = ("prefix", "dose")[int(rng.integers(2))]
    method = int(rng.integers(1, 3))
    nc, nt = int(rng.integers(5, 90)), int(rng.integers(5, 90))
    n = nc + nt
    ns = int(rng.choice([1, 1, 2, 3, 5, 7]))
    strata = t.make_strata(rng, n, ns) if n >= 2 * ns else None
    n_rows = int(rng.integers(3, 40))
    rows = (rng.random((n_rows, n)) < rng.uniform(0.05, 0.5, size=(n_rows, 1))).astype(np.int8)
    rows[:, :nc] |= (rng.random((n_rows, nc)) < rng.uniform(0, 0.3)).astype(np.int8)
    S = int(rng.integers(1, 30))
    sets = [rng.integers(0, n_rows, int(rng.integers(1, 12))).tolist() for _ in range(S)]
    if rng.random() < 0.3:
        sets[int(rng.integers(S))][0] = -1
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    if kind == "prefix":
        extra = None if rng.random() < 0.3 else [(rng.random(len(s)) < 0.6).astype(int).tolist() for s in sets]
    else:
        extra = tuple(sorted(rng.choice(np.arange(1, 16), int(rng.integers(1, 5)), replace=False).tolist()))
    hits = int(rng.choice([1, 2, 5, 20, 5000]))
    max_perms = int(rng.choice([1, 511, 512, 513, 1500, 2600]))
    env = {"GCRE_SEQ_BATCH_PERMS": rng.choice([None, "512", "1024"]), "GCRE_SEQ_MAX_MB": rng.choice([None, "0.01"]),
           "GCRE_PREFIX_SLAB_SETS": rng.choice([None, "1", "2", "5"])}
    weighted = bool(rng.random() < 0.4) and min(nc, nt) >= 20 and ns <= 3     # (every stratum then has cases and controls to draw)
    odds = np.exp(rng.normal(0, 0.7, n)) if weighted else None
    return kind, method, nc, nt, strata, rows, sets, signs, extra, hits, max_perms, env, odds, int(rng.integers(1 << 30))


def test_fuzz_against_the_definition(monkeypatch):
    for i in range(int(os.environ.get("GCRE_SEQ_PREFIX_FUZZ_CASES", "6"))):
        kind, method, nc, nt, strata, rows, sets, signs, extra, hits, max_perms, env, odds, seed = fuzz_case(i)
        VT = api.values_table(nc, nt)
        att = None
        if odds is None:
            masks = report.permutation_masks(nc, nt, max_perms, seed, strata)
        else:
            thr, _ = api.weighted_thresholds(odds, nc, nt, strata)
            masks, att = report.weighted_masks(thr, nc, nt, max_perms, seed, strata)
        cuts = [[1] * len(s) for s in sets] if kind == "prefix" and extra is None else extra
        obs, null, owner, valid = step_null(kind, method, sets, signs, rows, cuts, nc, VT, masks)
        ref = report.adaptive_sequential_reference(obs, null, owner, len(sets), valid, hits, max_perms, attempts=att)
        for var, val in env.items():
            if val is None:
                monkeypatch.delenv(var, raising=False)
            else:
                monkeypatch.setenv(var, str(val))
        ex = t.open_context(method, nc, nt, VT)
        try:
            rec, px, seq = call(ex, kind, sets, rows, signs, extra, hits=hits, max_perms=max_perms, seed=seed, strata=strata, odds=odds)
            t.assert_equal(seq, ref, f"case {i}")
            ok = valid != 0
            np.testing.assert_array_equal(px["score"][ok], ref["score"][ok], err_msg=f"case {i}")
        finally:
            ex.close()
