"""Multi-hit set tests on the device (gcre_score_sets_dose: k_dose_rows, then k_set_observed, k_prefix_pick, k_prefix_null;
DESIGN.md §3.20).  The yardstick is the code that already exists and is itself held to the oracle: the level rows of every set
are written out in numpy as synthetic genes by ``report.dose_sets``, scored by ``score_sets`` and ``family_tests(null=True)``
on the same context, and folded by ``report.prefix_reference``.  Every comparison is exact: integers, and scores as bit
patterns.  The shapes are the smallest at which each part can go wrong: the word and dword edges of the patient columns and a
case boundary inside a dword; a row of more than 64 dwords (a second wave per slot); set sizes around the eight loads a lane
keeps in flight; counts that pass 15; levels whose constants differ in every plane; a partial last block of four slots."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from geneticscre_amd import api, report
from helpers import small_table, special_table

pytestmark = pytest.mark.gpu

N_ROWS = 42
PERMS = (1, 100, 512, 513, 1300)
COHORTS = ((1, 1), (16, 17), (32, 32), (33, 32), (90, 110))
SIZES = (1, 2, 3, 5, 9, 16, 17, 40)
LEVELS = ([1], [2], [15], [1, 2, 3], [1, 15], list(range(1, 16)), [3, 4, 7, 8])
COUNTERS = [("given", "gcre_given_launches"), ("family", "gcre_family_launches"), ("minp", "gcre_minp_launches"),
            ("compete", "gcre_compete_launches"), ("prefix", "gcre_prefix_launches"), ("subsample", "gcre_subsample_launches"),
            ("overlap", "gcre_overlap_launches"), ("clump", "gcre_clump_launches"), ("patients", "gcre_patient_launches"),
            ("burden", "gcre_burden_launches"), ("stepdown", "gcre_stepdown_launches")]
ENV = ("GCRE_PREFIX_MAX_MB", "GCRE_PREFIX_SLAB_SETS", "GCRE_FAMILY_MAX_MB", "GCRE_FAMILY_SLAB_PERMS")
COUNTS = ("cases_pos", "ctrls_pos", "cases_neg", "ctrls_neg")


def other_counters(ex):
    """Every launch counter of the context but the stage's own."""
    return [int(getattr(api._feature_lib(f), sym)(ex._h)) for f, sym in COUNTERS]


def make_rows(rng, n, n_rows=N_ROWS):
    """Gene rows at carrier rates 0.02 .. 0.4; row 0 everybody, row 1 nobody."""
    rows = (rng.random((n_rows, n)) < rng.uniform(0.02, 0.4, size=(n_rows, 1))).astype(np.int8)
    rows[0], rows[1] = 1, 0
    return rows


def make_family(rng):
    """Sets of every size of SIZES in a shuffled order, the all-ones row listed 17 and 40 times (the counter passes 15: the
    sticky plane decides), a set with a member listed twice, a set of non-carriers, a row under both signs, an NA set in the
    middle: 14 sets, 13 valid, so the last block of four slots has one."""
    sets = [rng.integers(2, N_ROWS, k).tolist() for k in SIZES]
    order = rng.permutation(len(sets)).tolist()
    sets = [sets[i] for i in order]
    sets.append([0] * 17)
    sets.append([0] * 40)
    sets.append([9, 4, 9])                                       # a duplicated member
    sets.append([1, 1, 1])                                       # non-carriers
    sets.append([7, 3, 7, 0])                                    # a row under both signs (below), then everybody
    sets.insert(6, [-1, 5, 9])                                   # an NA member
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    signs[-1] = [1, -1, -1, 1]
    signs[-4] = [1] * 20 + [-1] * 20                             # (method 2: 20 in either half, both past 15)
    return sets, signs


def open_context(method, nc, nt, VT, K, seed=1):
    ex = api.JoinExec(method, nc, nt, K)
    ex.set_value_table(VT)
    if K > 0:
        ex.generate_permutations(seed, None)
    return ex


def bits(a):
    """The bit patterns of doubles, every NaN as one pattern."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.float64(np.nan), a).view(np.uint64)


def bits32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return np.where(np.isnan(a), np.float32(np.nan), a).view(np.uint32)


def reference(ex, sets, rows, signs, levels):
    """The call restated through the entries that exist: the level sets scored by score_sets and family_tests(null=True) and
    folded by prefix_reference.  Returns the reference, the level records, the level sets' owner, the family maxima over the
    level sets of the valid sets and the level rows."""
    lrows, lsets, lsigns, owner = report.dose_sets(sets, rows, signs, levels, ex.method == 2)
    if not len(lrows):                                           # (no valid set: still a row to point to)
        lrows = np.zeros((1, np.asarray(rows).shape[1]), np.int8)
    rec, fam = ex.score_sets(lsets, lrows, lsigns, family=True)
    rec2, _, null = ex.family_tests(lsets, lrows, lsigns, null=True)
    assert rec2.tobytes() == rec.tobytes()
    lists = report._set_lists(sets, signs)[0]
    valid = np.array([all(r >= 0 for r in m) for m in lists])
    assert np.array_equal(rec["valid"] != 0, valid[owner])       # the level sets of an NA set are dropped by the entries themselves
    ref = report.prefix_reference(rec["score"], null, owner, len(lists), valid)
    return ref, rec, owner, fam, lrows


def assert_equal_reference(ex, sets, rows, signs, levels, what=""):
    """dose_tests with every optional output against ``reference``; returns what it returned and the reference."""
    plain = ex.score_sets(sets, rows, signs)
    ref, lrec, owner, fam_want, lrows = reference(ex, sets, rows, signs, levels)
    others = other_counters(ex)
    before = ex.dose_launches()
    rec, ds, fam, null, lsc = ex.dose_tests(sets, rows, signs, levels=levels, family=True, null=True, level_scores=True)
    K, S, L = ex.iters, len(rec), len(levels)
    assert other_counters(ex) == others
    assert ex.dose_launches() > before if K > 0 and (rec["valid"] != 0).any() else ex.dose_launches() == before
    assert rec.tobytes() == plain.tobytes(), f"{what} the records of score_sets"
    assert ds.dtype == api.DOSE_SCORE and fam.dtype == np.float32 and null.shape == (S, K) and lsc.shape == (S, L)
    assert (ds["levels"] == L).all() and (ds["pad"] == 0).all()
    if K == 0:                                                   # nothing of the stage runs
        assert (ds["best_index"] == -1).all() and (ds["best_level"] == 0).all() and np.isnan(ds["score"]).all()
        assert np.isnan(lsc).all() and fam.shape == (0,) and all((ds[f] == 0).all() for f in COUNTS)
        np.testing.assert_array_equal(ds["n_ge"], np.where(rec["valid"] != 0, 0, -1))
        return (rec, ds, fam, null, lsc), ref, lrec
    np.testing.assert_array_equal(ds["best_index"], ref["best_step"], err_msg=f"{what} best_index")
    np.testing.assert_array_equal(bits(ds["score"]), bits(ref["score"]), err_msg=f"{what} score")
    np.testing.assert_array_equal(ds["n_ge"], ref["n_ge"], err_msg=f"{what} n_ge")
    np.testing.assert_array_equal(bits32(null), bits32(ref["null_max"]), err_msg=f"{what} null_max")
    np.testing.assert_array_equal(fam.view(np.uint32), fam_want.view(np.uint32), err_msg=f"{what} family_max")
    lv = np.asarray(levels)
    np.testing.assert_array_equal(ds["best_level"], np.where(ds["best_index"] >= 0, lv[np.maximum(ds["best_index"], 0)], 0))
    for s in range(S):
        b = ds["best_index"][s]
        if b < 0:
            assert all(ds[f][s] == 0 for f in COUNTS), (what, s)
            continue
        r = lrec[s * L + b]
        assert all(ds[f][s] == r[f] for f in COUNTS), (what, s)
        # a consequence: the maximum over the levels reaches the score at least as often as the best level alone
        assert ds["n_ge"][s] >= r["n_ge"], (what, s)
    # level_scores: the observed score of every level row, NaN rows for invalid sets
    want = np.where((rec["valid"] != 0)[:, None], lrec["score"].reshape(S, L), np.nan)
    np.testing.assert_array_equal(bits(lsc), bits(want), err_msg=f"{what} level_scores")
    invalid = rec["valid"] == 0
    assert np.isnan(null[invalid]).all() and (ds["n_ge"][invalid] == -1).all() and np.isnan(ds["score"][invalid]).all()
    assert (ds["best_index"][invalid] == -1).all() and (ds["best_level"][invalid] == 0).all()
    return (rec, ds, fam, null, lsc), ref, lrec


def noisy_table(rng, n, seed):
    VT = small_table(n, n, seed)
    VT[rng.random(VT.shape) < 0.05] *= -1
    VT[rng.random(VT.shape) < 0.03] = np.nan
    return VT


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("cohort", COHORTS, ids=[f"{a}+{b}" for a, b in COHORTS])
def test_dose_against_the_existing_entries(monkeypatch, method, cohort):
    """The set family at levels 1, 2, 3 under every permutation count, and at every level list under 513 permutations."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    nc, nt = cohort
    n = nc + nt
    rng = np.random.default_rng([2000, n])                      # the seed of the guard below: see the assertion
    rows = make_rows(rng, n)
    sets, signs = make_family(rng)
    VT = noisy_table(rng, n, n)
    for K, levels in [(K, [1, 2, 3]) for K in PERMS] + [(513, lv) for lv in LEVELS if lv != [1, 2, 3]]:
        ex = open_context(method, nc, nt, VT, K, seed=n + K)
        try:
            (rec, ds, fam, null, lsc), ref, lrec = assert_equal_reference(ex, sets, rows, signs, levels, f"n={n} K={K} levels={levels}")
            L = len(levels)
            ok = rec["valid"] != 0
            if levels == [1, 2, 3] and n >= 33:
                # no vacuous pass, and by the reference alone: a best level beyond the first, and carriers at a level >= 2
                assert (ref["best_step"][ok] > 0).any()
                assert (lrec["cases_pos"] + lrec["ctrls_pos"]).reshape(-1, L)[:, 1:].sum() > 0
            # the all-ones row 17 and 40 times: every patient is at or above every level (method 2: 20 + 20 at 40)
            for s in (len(sets) - 5, len(sets) - 4):
                assert set(sets[s]) == {0} and len(sets[s]) in (17, 40)
                if ds["best_index"][s] < 0:                      # (a NaN cell of the table)
                    continue
                if method == 1:
                    assert ds["cases_pos"][s] + ds["ctrls_pos"][s] == n
                elif len(sets[s]) == 40:
                    assert (ds["cases_pos"][s] + ds["ctrls_pos"][s], ds["cases_neg"][s] + ds["ctrls_neg"][s]) == (n, n)
            # non-carriers: every level reads table[0][0]; the first one is the best
            s = len(sets) - 2
            assert ds["best_index"][s] == (0 if not np.isnan(VT[0][0]) else -1) and all(ds[f][s] == 0 for f in COUNTS)
        finally:
            ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_second_stretch_wave_and_a_case_boundary_inside_a_dword(monkeypatch, method):
    """2,100 patients: 66 dwords, so a second wave per slot with two live lanes; 1,037 cases end inside dword 32."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    nc, nt, K = 1037, 1063, 100
    n = nc + nt
    rng = np.random.default_rng(2010 + method)
    rows = make_rows(rng, n)
    rows[2:6, 2048:] = 1                                         # carriers in the second wave's dwords, four genes deep
    rows[2:4, 1030:1045] = 1                                     # and on either side of the case boundary
    sets, signs = make_family(rng)
    sets.append([2, 3, 4, 5])
    signs.append([1, 1, -1, -1])
    ex = open_context(method, nc, nt, small_table(n, n, 7), K)
    try:
        (rec, ds, fam, null, lsc), ref, lrec = assert_equal_reference(ex, sets, rows, signs, [1, 2, 4], "2100 patients")
        # the planted block, by hand: the last 52 patients (controls) carry all four genes
        tail = report.dose_sets([sets[-1]], rows, [signs[-1]], [4 if method == 1 else 2], method == 2)[0]
        assert tail[0, 2048:].all() and tail[-1, 2048:].all()
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_level_1_is_score_sets(monkeypatch, method):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(2020 + method)
    nc, nt, K = 90, 110, 513
    n = nc + nt
    rows = make_rows(rng, n)
    sets, signs = make_family(rng)
    ex = open_context(method, nc, nt, noisy_table(rng, n, 3), K)
    try:
        rec, fam0 = ex.score_sets(sets, rows, signs, family=True)
        got, ds, fam, null, lsc = ex.dose_tests(sets, rows, signs, levels=[1], family=True, null=True, level_scores=True)
        assert got.tobytes() == rec.tobytes()
        ok = rec["valid"] != 0
        np.testing.assert_array_equal(bits(ds["score"]), bits(rec["score"]))
        np.testing.assert_array_equal(ds["n_ge"], np.where(ok, rec["n_ge"], -1))
        for f in COUNTS:
            np.testing.assert_array_equal(ds[f], np.where(np.isnan(rec["score"]), 0, rec[f]))
        np.testing.assert_array_equal(ds["best_index"], np.where(np.isnan(rec["score"]), -1, 0))
        np.testing.assert_array_equal(bits(lsc[:, 0]), bits(rec["score"]))
        np.testing.assert_array_equal(fam.view(np.uint32), fam0.view(np.uint32))
        np.testing.assert_array_equal(bits32(null), bits32(ex.family_tests(sets, rows, signs, null=True)[2]))
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_optional_outputs_change_nothing(monkeypatch, method):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(2030 + method)
    nc, nt, K = 33, 32, 513
    n = nc + nt
    rows = make_rows(rng, n)
    sets, signs = make_family(rng)
    ex = open_context(method, nc, nt, small_table(n, n, 4), K)
    try:
        plain = ex.score_sets(sets, rows, signs)
        full = ex.dose_tests(sets, rows, signs, levels=[1, 2, 3], family=True, null=True, level_scores=True)
        assert full[0].tobytes() == plain.tobytes()
        for family in (False, True):
            for null in (False, True):
                for lsc in (False, True):
                    got = ex.dose_tests(sets, rows, signs, levels=[1, 2, 3], family=family, null=null, level_scores=lsc)
                    assert len(got) == 2 + family + null + lsc
                    assert got[0].tobytes() == full[0].tobytes() and got[1].tobytes() == full[1].tobytes()
                    rest = list(got[2:])
                    for on, want in ((family, full[2]), (null, full[3]), (lsc, full[4])):
                        if on:
                            assert rest.pop(0).tobytes() == want.tobytes()
        # the flat form gives the same
        off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
        flat = (off, np.concatenate(sets).astype(np.int32))
        again = ex.dose_tests(flat, rows, np.concatenate(signs), levels=np.array([1, 2, 3]))
        assert again[0].tobytes() == full[0].tobytes() and again[1].tobytes() == full[1].tobytes()
    finally:
        ex.close()


@pytest.mark.parametrize("null", [False, True])
@pytest.mark.parametrize("method", [1, 2])
def test_slabs_change_nothing(monkeypatch, method, null):
    """Thirty-seven sets in slabs of 1, 3 and 5 by count and of 5 by bytes against one slab."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(2040 + method)
    nc, nt, K = 31, 34, 600
    n = nc + nt
    rows = make_rows(rng, n)
    sets = [rng.integers(0, N_ROWS, int(rng.integers(1, 12))).tolist() for _ in range(37)]
    sets[11] = [4, -1, 6, 1, 1]
    signs = [rng.choice([-1, 1], len(s)).tolist() for s in sets]
    levels = [1, 2, 3]
    ex = open_context(method, nc, nt, small_table(n, n, 5), K)
    try:
        one = ex.dose_tests(sets, rows, signs, levels=levels, family=True, null=null, level_scores=True)
        count = ex.dose_launches()
        assert count == 4                                        # rows, observed, pick, null: one slab
        for slab_sets in (1, 3, 5):
            monkeypatch.setenv("GCRE_PREFIX_SLAB_SETS", str(slab_sets))
            got = ex.dose_tests(sets, rows, signs, levels=levels, family=True, null=null, level_scores=True)
            count += 4 * -(-36 // slab_sets)                     # 36 valid sets
            assert ex.dose_launches() == count
            assert len(got) == len(one) and all(x.tobytes() == y.tobytes() for x, y in zip(got, one))
        monkeypatch.delenv("GCRE_PREFIX_SLAB_SETS")
        # a set's working rows: 3 levels x M halves x 8 dwords (65 patients: 2 words, padded to 4) x 4 bytes, and with null a
        # row of 2,048 floats; five and a half of them
        per = 3 * method * 8 * 4 + (2048 * 4 if null else 0)
        monkeypatch.setenv("GCRE_PREFIX_MAX_MB", repr((5 * per + per // 2) / 1048576.0))
        got = ex.dose_tests(sets, rows, signs, levels=levels, family=True, null=null, level_scores=True)
        assert ex.dose_launches() == count + 4 * 8               # seven slabs of 5 and one of 1
        assert len(got) == len(one) and all(x.tobytes() == y.tobytes() for x, y in zip(got, one))
        monkeypatch.delenv("GCRE_PREFIX_MAX_MB")
        if null:
            assert_equal_reference(ex, sets, rows, signs, levels, "37 sets")
    finally:
        ex.close()


def set_tables(kind, n, seed):
    return [(f"variant{v}", special_table(kind, n, n, seed, v)) for v in range({"nonfinite": 3, "huge": 2}.get(kind, 1))]


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("kind", ["zeros", "nonfinite", "tiny", "huge", "ladder"])
def test_special_tables(monkeypatch, kind, method):
    """Signed zeros, NaN, infinities, denormals and overflowing sums in the table: the maximum over the levels, the tie rule
    and the f32 threshold on such values."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    n, K, nc = 200, 300, 93
    rng = np.random.default_rng(2050 + method)
    rows = make_rows(rng, n, 16)
    sets = [rng.integers(0, 16, size=int(rng.integers(1, 9))).tolist() for _ in range(14)]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    sets[0], signs[0] = [1, 0], [1, 1]                        # the empty row, then the full row
    sets[1], signs[1] = [6], [-1]                             # a lone (-) gene: the (+) half reads table[0][0]
    for name, VT in set_tables(kind, n, 3):
        ex = open_context(method, nc, n - nc, VT, K, seed=91)
        try:
            with np.errstate(over="ignore", invalid="ignore"):
                assert_equal_reference(ex, sets, rows, signs, [1, 2, 3], f"{kind} {name}")
        finally:
            ex.close()


def test_no_permutations(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(2060)
    nc, nt = 16, 17
    rows = make_rows(rng, nc + nt)
    sets, signs = make_family(rng)
    ex = open_context(2, nc, nt, small_table(nc + nt, nc + nt, 1), 0)
    try:
        (rec, ds, fam, null, lsc), _, _ = assert_equal_reference(ex, sets, rows, signs, [1, 2], "K=0")
        assert ex.dose_launches() == 0 and null.shape == (len(sets), 0) and lsc.shape == (len(sets), 2)
    finally:
        ex.close()


def test_refusals_leave_everything_untouched(monkeypatch):
    """Every refusal through the C entry: the code, the message, the outputs and all launch counters untouched."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(2070)
    n, nc, K = 65, 30, 100
    rows = make_rows(rng, n)
    packed = api.pack_carriers(rows, n)
    lib = api._dose_lib()
    ex = open_context(1, nc, n - nc, small_table(n, n, 2), K)
    bare = api.JoinExec(1, nc, n - nc, K)                      # no table, no masks
    try:
        def call(off, members, sg=None, n_cols=n, cap=None, ds=True, env=None, on=ex, null=False, levels=(1, 2, 3), n_levels=None):
            off = np.asarray(off, np.int64)
            members = np.asarray(members, np.int32)
            sg = None if sg is None else np.asarray(sg, np.int32)
            lv = None if levels is None else np.asarray(levels, np.int32)
            L = (0 if lv is None else len(lv)) if n_levels is None else n_levels
            S = len(off) - 1
            inp = api.gcre_set_input(S, api._ptr(off), api._ptr(members), api._ptr(sg), api._ptr(packed), packed.shape[0], n_cols)
            out = np.full(max(S, 1), 7, dtype=np.uint8).repeat(api.SET_SCORE.itemsize).view(api.SET_SCORE)
            dso = np.full(max(S, 1) * api.DOSE_SCORE.itemsize, 7, np.uint8).view(api.DOSE_SCORE)
            fam = np.full(K, -5.0, np.float32)
            nul = np.full((max(S, 1), K), -5.0, np.float32)
            lsc = np.full((max(S, 1), 16), -5.0)
            n_out = ctypes.c_int64(0)
            counters = (other_counters(on), on.dose_launches())
            for k, v in (env or {}).items():
                monkeypatch.setenv(k, v)
            rc = lib.gcre_score_sets_dose(on._h, ctypes.byref(inp), api._ptr(lv), L, api._ptr(out), S if cap is None else cap,
                                          ctypes.byref(n_out), api._ptr(dso) if ds else None, api._ptr(fam),
                                          api._ptr(nul) if null else None, api._ptr(lsc))
            for k in (env or {}):
                monkeypatch.delenv(k)
            msg = api.load_library().gcre_last_error(on._h).decode()
            assert (other_counters(on), on.dose_launches()) == counters
            assert (dso.view(np.uint8) == 7).all() and (fam == -5).all() and (nul == -5).all() and (lsc == -5).all()
            assert (out.view(np.uint8) == 7).all()
            return rc, msg

        ARG = -4                                                 # GCRE_ERR_ARG
        W = "score_sets_dose: "
        assert lib.gcre_score_sets_dose(None, None, None, 0, None, 0, None, None, None, None, None) == ARG
        rc, msg = call([0, 2, 5], [1, 2, 3, 4, 5], ds=False)
        assert rc == ARG and msg == W + "NULL argument (dose_out)"
        rc, msg = call([0, 2, 5], [1, 2, 3, 4, 5], levels=[], n_levels=0)
        assert rc == ARG and msg == W + "n_levels = 0: 1 .. 15 levels"
        rc, msg = call([0, 2, 5], [1, 2, 3, 4, 5], levels=list(range(1, 16)), n_levels=16)
        assert rc == ARG and msg == W + "n_levels = 16: 1 .. 15 levels"
        rc, msg = call([0, 2, 5], [1, 2, 3, 4, 5], levels=None, n_levels=2)
        assert rc == ARG and msg == W + "NULL argument (levels)"
        rc, msg = call([0, 2, 5], [1, 2, 3, 4, 5], levels=[0, 1])
        assert rc == ARG and msg == W + "level 0 (index 0) is outside 1 .. 15"
        rc, msg = call([0, 2, 5], [1, 2, 3, 4, 5], levels=[1, 16])
        assert rc == ARG and msg == W + "level 16 (index 1) is outside 1 .. 15"
        rc, msg = call([0, 2, 5], [1, 2, 3, 4, 5], levels=[2, 2])
        assert rc == ARG and msg == W + "the levels are not strictly ascending (2 after 2)"
        rc, msg = call([0, 2, 2], [1, 2])
        assert rc == ARG and msg == W + "set 1 has no members"
        rc, msg = call([0, 2], [1, N_ROWS])
        assert rc != 0 and msg == W + f"set 0: member row {N_ROWS} out of range ({N_ROWS} rows)"
        rc, msg = call([0, 2], [1, 2], sg=[1, 0])
        assert rc == ARG and msg == W + "set 0: sign 0 is neither +1 nor -1"
        rc, msg = call([0, 2], [1, 2], n_cols=n - 1)
        assert rc == ARG and msg == W + f"the rows have {n - 1} columns, not n_cases + n_ctrls = {n}"
        rc, msg = call([0, 1, 2], [1, 2], cap=1)
        assert rc != 0 and msg == W + "2 sets, room for 1 records (out of range)"
        rc, msg = call([0, 2], [1, 2], on=bare)
        assert rc != 0 and msg == "assertion: score_sets_dose needs a value table"
        # 3 levels x 1 half x 8 dwords (65 patients: two words, padded to four) x 4 bytes = 96 bytes
        rc, msg = call([0, 1, 4], [-1, 2, 3, 4], env={"GCRE_PREFIX_MAX_MB": "0.00005"})
        assert rc == ARG and msg == W + "the 3 level rows of set 1 take 96 bytes: above GCRE_PREFIX_MAX_MB = 0.000050"
        rc, msg = call([0, 1, 4], [1, 2, 3, 4], env={"GCRE_PREFIX_MAX_MB": "0.001"}, null=True, levels=[2])
        assert rc == ARG and msg == W + "the 1 level rows of set 0 take 8224 bytes: above GCRE_PREFIX_MAX_MB = 0.001000"
        # and the same list is accepted without the bound
        rec, ds = ex.dose_tests([[1], [2, 3, 4]], rows, levels=[1, 2, 3])
        assert ds["levels"].tolist() == [3, 3] and ex.dose_launches() == 4
    finally:
        ex.close()
        bare.close()


def test_launch_counters_are_apart(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(2080)
    n, nc, K = 33, 15, 100
    rows = make_rows(rng, n)
    sets = [[2, 3], [4, 5, 6]]
    ex = open_context(1, nc, n - nc, small_table(n, n, 2), K)
    try:
        assert ex.dose_launches() == 0
        ex.score_sets(sets, rows)
        ex.family_tests(sets, rows)
        ex.prefix_tests(sets, rows)
        ex.score_sets(sets, rows, which=[0, 1], given=[1, 0])
        assert ex.dose_launches() == 0                           # nobody else's launches count here
        others = other_counters(ex)
        assert ex.prefix_launches() == 4 and ex.family_launches() > 0
        ex.dose_tests(sets, rows)
        assert ex.dose_launches() == 4
        assert other_counters(ex) == others and ex.prefix_launches() == 4      # the prefix stage's kernels, not its counter
        ex.dose_tests([[-1, 2]], rows)                           # no valid set: nothing to launch
        assert ex.dose_launches() == 4
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_pairs_at_level_2_are_the_anded_rows(monkeypatch, method):
    """Digenic screening: ``pair_sets`` at level 2 is score_sets on the genes' rows ANDed in numpy."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(2090 + method)
    nc, nt, K = 90, 110, 513
    n = nc + nt
    rows = (rng.random((9, n)) < rng.uniform(0.2, 0.6, size=(9, 1))).astype(np.int8)
    pairs = report.pair_sets(range(9))
    assert len(pairs) == 36
    anded = np.array([rows[a] & rows[b] for a, b in pairs], np.int8)
    ex = open_context(method, nc, nt, noisy_table(rng, n, 6), K)
    try:
        want, fam_want = ex.score_sets([[i] for i in range(36)], anded, family=True)
        rec, ds, fam = ex.dose_tests(pairs, rows, levels=[2], family=True)
        assert anded.any(axis=1).all()
        np.testing.assert_array_equal(bits(ds["score"]), bits(want["score"]))
        np.testing.assert_array_equal(ds["n_ge"], want["n_ge"])
        for f in COUNTS:
            np.testing.assert_array_equal(ds[f], np.where(np.isnan(want["score"]), 0, want[f]))
        np.testing.assert_array_equal(fam.view(np.uint32), fam_want.view(np.uint32))
        assert rec.tobytes() == ex.score_sets(pairs, rows).tobytes()
    finally:
        ex.close()


@pytest.mark.parametrize("signed", [False, True])
def test_multi_hit_test_columns(monkeypatch, signed):
    """Twelve sets, one with planted double hits among the cases: every column recomputed from the records of a context of
    the same seed."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(2100 + signed)
    nc, nt, K, G = 60, 70, 200, 30
    n = nc + nt
    genes = [f"G{i}" for i in range(G)]
    data = (rng.random((G, n)) < rng.uniform(0.01, 0.3, size=(G, 1))).astype(np.int32)
    data[10:13] = 0
    data[10:13, :20] = 1                                         # planted: twenty cases carry G10, G11 and G12
    data[10, 60:100] = 1                                         # ... and forty controls G10 alone
    names = [f"P{i}" for i in range(12)]
    sets = [[genes[j] for j in rng.choice(G, int(rng.integers(1, 9)), replace=False)] for _ in range(12)]
    sets[3] = ["G10", "G11", "G12", "G11"]                       # a gene named twice: kept once
    sets[7] = ["G2", "nowhere"]                                  # a gene that is not in the table
    levels = (1, 2, 3)
    if signed:
        sets = [" -> ".join(f"{g} (+)" if i == 3 or rng.random() < 0.5 else f"{g} (-)" for g in s) for i, s in enumerate(sets)]
    df = report.multi_hit_test(sets, genes, data, nc, nt, signed=signed, names=names, levels=levels, threshold=1.0,
                               n_permutations=K, seed=5)
    assert list(df.columns) == report.MULTI_HIT_COLUMNS and df["Sets"].tolist() == names and len(df) == 12
    g2, d2 = report.preprocess_table(genes, data, 1.0, nc, nt)
    d2 = np.asarray(d2)
    nms, rws, sgs = report.parse_sets(sets, g2)
    keep = [[i for i, x in enumerate(nm) if x not in nm[:i]] for nm in nms]
    rws = [[r[i] for i in k] for r, k in zip(rws, keep)]
    sgs = [[s[i] for i in k] for s, k in zip(sgs, keep)]
    assert len(rws[3]) == 3
    ex = api.JoinExec(2 if signed else 1, nc, nt, K)
    try:
        ex.set_value_table(api.values_table(nc, nt))
        ex.generate_permutations(5, None)
        rec, ds, fam = ex.dose_tests(rws, d2, sgs, levels=levels, family=True)
    finally:
        ex.close()
    ok = (rec["valid"] != 0) & (ds["best_index"] >= 0)
    assert not ok[7] and ok.sum() >= 10
    assert df["Genes"].tolist() == [len(r) for r in rws]
    np.testing.assert_array_equal(bits(df["Scores"]), bits(rec["score"]))
    np.testing.assert_array_equal(bits(df["NominalPvalues"]), bits(rec["pvalue"]))
    np.testing.assert_array_equal(bits(df["MultiHitScores"]), bits(np.where(ok, ds["score"], np.nan)))
    np.testing.assert_array_equal(bits(df["MultiHitPvalues"]), bits(np.where(ok, ds["n_ge"] / K, np.nan)))
    np.testing.assert_array_equal(bits(df["BestLevel"]), bits(np.where(ok, ds["best_level"], np.nan)))
    np.testing.assert_array_equal(bits(df["BestCases"]), bits(np.where(ok, ds["cases_pos"], np.nan)))
    np.testing.assert_array_equal(bits(df["BestControls"]), bits(np.where(ok, ds["ctrls_pos"], np.nan)))
    famp = np.array([(fam.astype(np.float64) >= ds["score"][s]).sum() / K if ok[s] else np.nan for s in range(12)])
    np.testing.assert_array_equal(bits(df["MultiHitFamilyPvalues"]), bits(famp))
    # the planted set: the union is diluted by the forty controls, the double hits are not
    assert df["BestLevel"][3] >= 2 and df["BestCases"][3] == 20 and df["BestControls"][3] == 0
    assert df["MultiHitScores"][3] > df["Scores"][3]
    # the statistic is at least the union's score (level 1 is among the levels), its family p-value at least its own
    assert (df["MultiHitScores"][ok] >= df["Scores"][ok]).all() and (df["MultiHitFamilyPvalues"][ok] >= df["MultiHitPvalues"][ok]).all()
    none = report.multi_hit_test(sets, genes, data, nc, nt, signed=signed, levels=levels, threshold=1.0, n_permutations=0)
    assert none["Sets"].tolist() == [f"Set{i}" for i in range(12)]
    assert none[["BestLevel", "BestCases", "BestControls", "MultiHitScores", "MultiHitPvalues", "MultiHitFamilyPvalues"]].isna().all().all()


def test_seeded_fuzz(monkeypatch):
    """GCRE_DOSE_FUZZ_CASES random calls (default 6; a long run is recorded in profiles/dose_fuzz.txt)."""
    cases = int(os.environ.get("GCRE_DOSE_FUZZ_CASES", "6"))
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    for case in range(cases):
        rng = np.random.default_rng([2110, case])
        method = int(rng.integers(1, 3))
        n = int(rng.integers(2, 300))
        nc = int(rng.integers(1, n))
        K = int(rng.choice([1, 37, 511, 512, 513, 1025, 2049]))
        n_rows = int(rng.integers(2, 30))
        rows = make_rows(rng, n, n_rows)
        rows[2:] |= (rng.random((n_rows - 2, n)) < rng.uniform(0, 0.5)).astype(np.int8)     # denser: deeper counts
        S = int(rng.integers(1, 14))
        sets = [rng.integers(0, n_rows, int(rng.choice([1, 2, 3, 4, 5, 8, 9, 16, 17, 40]))).tolist() for _ in range(S)]
        if case % 3 == 0:
            sets[int(rng.integers(0, S))][0] = -1
        signs = None if case % 4 == 1 else [rng.choice([-1, 1], len(s)).tolist() for s in sets]
        levels = sorted(rng.choice(np.arange(1, 16), int(rng.integers(1, 16)), replace=False).tolist())
        VT = noisy_table(rng, n, case)
        if case % 2:
            monkeypatch.setenv("GCRE_PREFIX_SLAB_SETS", str(int(rng.integers(1, 6))))
        if case % 5 == 4:                                        # and a byte bound of two and a half sets
            per = len(levels) * method * 8 * -(-n // 256) * 4 + 4 * 2048 * -(-K // 2048)     # level rows and the null_max row
            monkeypatch.setenv("GCRE_PREFIX_MAX_MB", repr(2.5 * per / 1048576.0))
        ex = open_context(method, nc, n - nc, VT, K, seed=case)
        try:
            assert_equal_reference(ex, sets, rows, signs, levels, f"fuzz case {case}")
        finally:
            ex.close()
            monkeypatch.delenv("GCRE_PREFIX_SLAB_SETS", raising=False)
            monkeypatch.delenv("GCRE_PREFIX_MAX_MB", raising=False)
