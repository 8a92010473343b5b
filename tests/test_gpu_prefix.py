"""Variable-threshold set tests on the device (gcre_score_sets_prefix: k_prefix_rows, k_prefix_pick, k_prefix_null; DESIGN.md
§3.18).  The yardstick is the code that already exists and is itself held to the oracle: the steps of every set are expanded
into sets of their own by ``report.prefix_sets``, scored by ``score_sets`` and ``family_tests(null=True)`` on the same
context, and folded by ``report.prefix_reference``.  Every comparison is exact: integers, and scores as bit patterns.  The
shapes are the smallest at which each part can go wrong: one permutation tile, its edge and the dead padding lanes; the word
and dword edges of the patient columns; step counts around a wave's step tile; blocks whose waves have unequal lengths."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from geneticscre_amd import api, report
from helpers import small_table, special_table

pytestmark = pytest.mark.gpu

N_ROWS = 40
PERMS = (1, 100, 512, 513, 1300)
PATIENTS = (2, 33, 64, 65, 200)
STEPS = (1, 2, 3, 4, 5, 9, 17, 70)
COUNTERS = [("given", "gcre_given_launches"), ("family", "gcre_family_launches"), ("minp", "gcre_minp_launches"),
            ("compete", "gcre_compete_launches"), ("overlap", "gcre_overlap_launches"), ("clump", "gcre_clump_launches"),
            ("patients", "gcre_patient_launches"), ("burden", "gcre_burden_launches"), ("stepdown", "gcre_stepdown_launches")]
ENV = ("GCRE_PREFIX_MAX_MB", "GCRE_PREFIX_SLAB_SETS", "GCRE_FAMILY_MAX_MB", "GCRE_FAMILY_SLAB_PERMS")


def other_counters(ex):
    """Every launch counter of the context but the stage's own."""
    return [int(getattr(api._feature_lib(f), sym)(ex._h)) for f, sym in COUNTERS]


def make_rows(rng, n, n_rows=N_ROWS):
    rows = (rng.random((n_rows, n)) < rng.uniform(0.02, 0.4, size=(n_rows, 1))).astype(np.int8)
    rows[0], rows[1] = 1, 0            # everybody, nobody
    return rows


def make_family(rng):
    """Sets of every step count of STEPS in a shuffled order (the waves of a block then have unequal lengths), a set with its
    last member appended again, a set of non-carriers, a row under both signs, an NA set: 12 sets, 11 valid, so the last
    block has three."""
    sets = [rng.integers(2, N_ROWS, k).tolist() for k in STEPS]
    order = rng.permutation(len(sets)).tolist()
    sets = [sets[i] for i in order]
    sets.append(sets[2] + sets[2][-1:])                          # a duplicated member appended
    sets.append([1, 1, 1])                                       # non-carriers
    sets.append([7, 3, 7, 0])                                    # a row under both signs (below), then everybody
    sets.insert(5, [-1, 5, 9])                                   # an NA member: no step of it is valid
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    signs[-1] = [1, -1, -1, 1]
    signs[-3] = signs[2] + signs[2][-1:]                         # ... under the sign it already has
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


def reference(ex, sets, rows, signs, cuts):
    """The call restated through the entries that exist: the step sets scored by score_sets and family_tests(null=True) and
    folded by prefix_reference.  Returns the reference, the step records, the steps' set index and score_sets' family maxima."""
    st, sg, owner = report.prefix_sets(sets, signs, cuts)
    rec, fam = ex.score_sets(st, rows, sg, family=True)
    rec2, _, null = ex.family_tests(st, rows, sg, null=True)
    assert rec2.tobytes() == rec.tobytes()
    lists = report._set_lists(sets, signs)[0]
    valid = np.array([all(r >= 0 for r in m) for m in lists])
    # a step of an invalid set may be a valid set of its own: it is in no result of the call
    dead = ~valid[owner]
    null[dead] = np.nan
    ref = report.prefix_reference(rec["score"], null, owner, len(lists), valid)
    live = [i for i in range(len(st)) if not dead[i]]
    fam_live = ex.score_sets([st[i] for i in live], rows, None if sg is None else [sg[i] for i in live], family=True)[1] \
        if dead.any() and live else fam
    return ref, rec, owner, (fam_live if live else np.zeros(ex.iters, np.float32)), st


def assert_equal_reference(ex, sets, rows, signs, cuts, what=""):
    """prefix_tests with every optional output against ``reference``; returns what it returned."""
    plain = ex.score_sets(sets, rows, signs)
    ref, srec, owner, fam_want, st = reference(ex, sets, rows, signs, cuts)
    others, fl, gl = other_counters(ex), ex.family_launches(), ex.given_launches
    before = ex.prefix_launches()
    rec, px, fam, null, steps = ex.prefix_tests(sets, rows, signs, cuts=cuts, family=True, null=True, steps=True)
    K, S = ex.iters, len(rec)
    assert other_counters(ex) == others and ex.family_launches() == fl and ex.given_launches == gl
    assert ex.prefix_launches() > before if K > 0 and (rec["valid"] != 0).any() else ex.prefix_launches() == before
    assert rec.tobytes() == plain.tobytes(), f"{what} the records of score_sets"
    assert px.dtype == api.PREFIX_SCORE and fam.dtype == np.float32 and null.shape == (S, K) and steps.dtype == np.float64
    first = np.searchsorted(owner, np.arange(S))
    nsteps = np.bincount(owner, minlength=S)
    np.testing.assert_array_equal(px["steps"], nsteps, err_msg=f"{what} steps")
    if K == 0:                                                   # nothing of the stage runs
        assert (px["best_step"] == -1).all() and np.isnan(px["score"]).all() and np.isnan(steps).all() and fam.shape == (0,)
        np.testing.assert_array_equal(px["n_ge"], np.where(rec["valid"] != 0, 0, -1))
        return rec, px, fam, null, steps
    np.testing.assert_array_equal(px["best_step"], ref["best_step"], err_msg=f"{what} best_step")
    np.testing.assert_array_equal(bits(px["score"]), bits(ref["score"]), err_msg=f"{what} score")
    np.testing.assert_array_equal(px["n_ge"], ref["n_ge"], err_msg=f"{what} n_ge")
    np.testing.assert_array_equal(bits32(null), bits32(ref["null_max"]), err_msg=f"{what} null_max")
    np.testing.assert_array_equal(fam.view(np.uint32), fam_want.view(np.uint32), err_msg=f"{what} family_max")
    for s in range(S):
        b = px["best_step"][s]
        if b < 0:
            assert px["best_members"][s] == 0 and all(px[f][s] == 0 for f in ("cases_pos", "ctrls_pos", "cases_neg", "ctrls_neg"))
            continue
        r = srec[first[s] + b]
        assert px["best_members"][s] == len(st[first[s] + b]), (what, s)
        assert all(px[f][s] == r[f] for f in ("cases_pos", "ctrls_pos", "cases_neg", "ctrls_neg")), (what, s)
        # a consequence: the maximum over the steps reaches the score at least as often as the best prefix alone
        assert px["n_ge"][s] >= r["n_ge"], (what, s)
    # step_scores: the observed score of the step that ends at every member, NaN elsewhere and for invalid sets
    lists = report._set_lists(sets, signs)[0]
    want = np.full(sum(len(m) for m in lists), np.nan)
    pos = np.concatenate([[0], np.cumsum([len(m) for m in lists])])
    for i, m in enumerate(st):
        if rec["valid"][owner[i]]:
            want[pos[owner[i]] + len(m) - 1] = srec["score"][i]
    np.testing.assert_array_equal(bits(steps), bits(want), err_msg=f"{what} step_scores")
    invalid = rec["valid"] == 0
    assert np.isnan(null[invalid]).all() and (px["n_ge"][invalid] == -1).all() and np.isnan(px["score"][invalid]).all()
    # the optional outputs change nothing
    bare = ex.prefix_tests(sets, rows, signs, cuts=cuts)
    assert len(bare) == 2 and bare[0].tobytes() == rec.tobytes() and bare[1].tobytes() == px.tobytes()
    return rec, px, fam, null, steps


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("n", PATIENTS)
def test_prefix_against_the_existing_entries(monkeypatch, method, n):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng([1800, method, n])
    nc = max(1, n // 2 - 1)
    nt = n - nc
    rows = make_rows(rng, n)
    sets, signs = make_family(rng)
    VT = small_table(n, n, n)
    VT[rng.random(VT.shape) < 0.05] *= -1
    VT[rng.random(VT.shape) < 0.03] = np.nan
    for K in PERMS:
        ex = open_context(method, nc, nt, VT, K, seed=n + K)
        try:
            rec, px, fam, null, steps = assert_equal_reference(ex, sets, rows, signs, None, f"n={n} K={K}")
            assert px["steps"].tolist() == [len(s) for s in sets]
            assert (px["best_step"] > 0).any() or n == 2         # (the best prefix is not always the first)
            # the set with its last member listed again: the same score, the same n_ge, the smaller index
            a, b = 2, len(sets) - 3
            assert sets[b][:-1] == sets[a] and signs[b][:-1] == signs[a]
            assert bits(px["score"][a:a + 1]) == bits(px["score"][b:b + 1]) and px["n_ge"][a] == px["n_ge"][b]
            assert px["best_step"][a] == px["best_step"][b] and np.array_equal(bits32(null[a]), bits32(null[b]))
        finally:
            ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_duplicated_member_and_non_carriers(monkeypatch, method):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(1810 + method)
    n, nc, K = 65, 30, 513
    rows = make_rows(rng, n)
    base = rng.integers(2, N_ROWS, 6).tolist()
    sg = rng.choice([-1, 1], 6).tolist()
    sets = [base, base + base[-1:], [1], [1, 1, 1, 1, 1], [0], [3, 3]]
    signs = [sg, sg + sg[-1:], [1], [1, -1, 1, -1, 1], [-1], [1, -1]]
    ex = open_context(method, nc, n - nc, small_table(n, n, 4), K)
    try:
        rec, px, fam, null, steps = assert_equal_reference(ex, sets, rows, signs, None, "duplicates")
        assert bits(px["score"][:1]) == bits(px["score"][1:2]) and px["n_ge"][0] == px["n_ge"][1]
        assert px["best_step"][0] == px["best_step"][1] < 6 and np.array_equal(null[0], null[1])
        # non-carriers: every step reads table[0][0]; the first one is the best
        assert px["best_step"][2] == 0 and px["best_step"][3] == 0 and px["cases_pos"][3] == 0 and px["ctrls_pos"][3] == 0
        assert bits(px["score"][2:3]) == bits(px["score"][3:4]) and px["n_ge"][2] == px["n_ge"][3]
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("kind", ["zeros", "random", "ties"])
def test_cuts(monkeypatch, method, kind):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng([1820, method, ["zeros", "random", "ties"].index(kind)])
    n, nc, K = 200, 93, 513
    rows = make_rows(rng, n)
    rows[10:20] = rows[10]                                       # rows of equal carrier total: tie groups
    sets, signs = make_family(rng)
    if kind == "zeros":
        cuts = [[0] * len(s) for s in sets]
    elif kind == "random":
        cuts = [(rng.random(len(s)) < 0.4).astype(int).tolist() for s in sets]
    else:
        cuts = []
        for i, s in enumerate(sets):
            order, ct = report.threshold_order(s, rows)
            sets[i] = np.asarray(s)[order].tolist()
            signs[i] = np.asarray(signs[i])[order].tolist()
            cuts.append(ct.tolist())
        sets[5] = [-1] + [r for r in sets[5] if r >= 0]          # (keep the NA member first: no valid step)
        cuts[5] = [1] * len(sets[5])
        assert any(0 in c[:-1] for c in cuts)                    # some genes do enter together
    ex = open_context(method, nc, n - nc, small_table(n, n, 9), K)
    try:
        rec, px, fam, null, steps = assert_equal_reference(ex, sets, rows, signs, cuts, kind)
        if kind == "zeros":                                      # one step, the full set: score_sets itself
            ok = rec["valid"] != 0
            assert (px["steps"] == 1).all() and (px["best_step"][ok & ~np.isnan(rec["score"])] == 0).all()
            np.testing.assert_array_equal(px["n_ge"], np.where(ok, rec["n_ge"], -1))
            np.testing.assert_array_equal(bits(px["score"]), bits(rec["score"]))
            for f in ("cases_pos", "ctrls_pos", "cases_neg", "ctrls_neg"):
                np.testing.assert_array_equal(px[f], rec[f])
            np.testing.assert_array_equal(fam.view(np.uint32), ex.score_sets(sets, rows, signs, family=True)[1].view(np.uint32))
        # the flat form gives the same
        off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
        flat = (off, np.concatenate(sets).astype(np.int32))
        again = ex.prefix_tests(flat, rows, np.concatenate(signs), cuts=np.concatenate(cuts))
        assert again[0].tobytes() == rec.tobytes() and again[1].tobytes() == px.tobytes()
    finally:
        ex.close()


@pytest.mark.parametrize("null", [False, True])
@pytest.mark.parametrize("method", [1, 2])
def test_slabs_change_nothing(monkeypatch, method, null):
    """Thirty-seven sets in slabs of 5 by count and by bytes against one slab."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(1830 + method)
    n, nc, K = 65, 31, 600
    rows = make_rows(rng, n)
    sets = [rng.integers(0, N_ROWS, 5).tolist() for _ in range(37)]
    sets[11] = [4, -1, 6, 1, 1]
    signs = [rng.choice([-1, 1], 5).tolist() for _ in sets]
    ex = open_context(method, nc, n - nc, small_table(n, n, 5), K)
    try:
        one = ex.prefix_tests(sets, rows, signs, family=True, null=null, steps=True)
        l0 = ex.prefix_launches()
        assert l0 == 4                                           # rows, observed, pick, null: one slab
        monkeypatch.setenv("GCRE_PREFIX_SLAB_SETS", "5")
        by_count = ex.prefix_tests(sets, rows, signs, family=True, null=null, steps=True)
        assert ex.prefix_launches() == l0 + 4 * 8                # 36 valid sets: seven slabs of 5 and one of 1
        monkeypatch.delenv("GCRE_PREFIX_SLAB_SETS")
        # a set's working rows: 5 steps x M halves x 4 dwords (65 patients: 2 words, padded to 4) x 4 bytes, and with null
        # a row of 2,048 floats
        per = 5 * method * 8 * 4 + (2048 * 4 if null else 0)
        monkeypatch.setenv("GCRE_PREFIX_MAX_MB", repr((5 * per + per // 2) / 1048576.0))
        by_bytes = ex.prefix_tests(sets, rows, signs, family=True, null=null, steps=True)
        assert ex.prefix_launches() == l0 + 4 * 8 + 4 * 8
        for got in (by_count, by_bytes):
            assert len(got) == len(one)
            for x, y in zip(got, one):
                assert x.tobytes() == y.tobytes()
        if null:
            monkeypatch.delenv("GCRE_PREFIX_MAX_MB")
            assert_equal_reference(ex, sets, rows, signs, None, "37 sets")
    finally:
        ex.close()


def set_tables(kind, n, seed):
    return [(f"variant{v}", special_table(kind, n, n, seed, v)) for v in range({"nonfinite": 3, "huge": 2}.get(kind, 1))]


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("kind", ["zeros", "nonfinite", "tiny", "huge", "ladder"])
def test_special_tables(monkeypatch, kind, method):
    """Signed zeros, NaN, infinities, denormals and overflowing sums in the table: the maximum over the steps, the tie rule
    and the f32 threshold on such values."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    n, K, nc = 200, 300, 93
    rng = np.random.default_rng(1840 + method)
    rows = make_rows(rng, n, 16)
    sets = [rng.integers(0, 16, size=int(rng.integers(1, 9))).tolist() for _ in range(14)]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    sets[0], signs[0] = [1, 0], [1, 1]                        # the empty row, then the full row
    sets[1], signs[1] = [6], [-1]                             # a lone (-) gene: the (+) half reads table[0][0]
    for name, VT in set_tables(kind, n, 3):
        ex = open_context(method, nc, n - nc, VT, K, seed=91)
        try:
            with np.errstate(over="ignore", invalid="ignore"):
                assert_equal_reference(ex, sets, rows, signs, None, f"{kind} {name}")
        finally:
            ex.close()


def test_no_permutations(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(1850)
    n, nc = 33, 15
    rows = make_rows(rng, n)
    sets, signs = make_family(rng)
    ex = open_context(2, nc, n - nc, small_table(n, n, 1), 0)
    try:
        rec, px, fam, null, steps = assert_equal_reference(ex, sets, rows, signs, None, "K=0")
        assert ex.prefix_launches() == 0 and null.shape == (len(sets), 0)
        assert px["steps"].tolist() == [len(s) for s in sets]
    finally:
        ex.close()


def test_refusals_leave_everything_untouched(monkeypatch):
    """Every refusal through the C entry: the code, the message, the outputs and all launch counters untouched."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(1860)
    n, nc, K = 65, 30, 100
    rows = make_rows(rng, n)
    packed = api.pack_carriers(rows, n)
    lib = api._prefix_lib()
    ex = open_context(1, nc, n - nc, small_table(n, n, 2), K)
    bare = api.JoinExec(1, nc, n - nc, K)                      # no table, no masks
    try:
        def call(off, members, sg=None, n_cols=n, cap=None, px=True, env=None, on=ex, null=False):
            off = np.asarray(off, np.int64)
            members = np.asarray(members, np.int32)
            sg = None if sg is None else np.asarray(sg, np.int32)
            S = len(off) - 1
            inp = api.gcre_set_input(S, api._ptr(off), api._ptr(members), api._ptr(sg), api._ptr(packed), packed.shape[0], n_cols)
            out = np.full(max(S, 1), 7, dtype=np.uint8).repeat(api.SET_SCORE.itemsize).view(api.SET_SCORE)
            pxo = np.full(max(S, 1) * api.PREFIX_SCORE.itemsize, 7, np.uint8).view(api.PREFIX_SCORE)
            fam = np.full(K, -5.0, np.float32)
            nul = np.full((max(S, 1), K), -5.0, np.float32)
            stp = np.full(max(len(members), 1), -5.0)
            n_out = ctypes.c_int64(0)
            counters = (other_counters(on), on.prefix_launches(), on.family_launches())
            for k, v in (env or {}).items():
                monkeypatch.setenv(k, v)
            rc = lib.gcre_score_sets_prefix(on._h, ctypes.byref(inp), None, api._ptr(out), S if cap is None else cap, ctypes.byref(n_out),
                                            api._ptr(pxo) if px else None, api._ptr(fam), api._ptr(nul) if null else None, api._ptr(stp))
            for k in (env or {}):
                monkeypatch.delenv(k)
            msg = api.load_library().gcre_last_error(on._h).decode()
            assert (other_counters(on), on.prefix_launches(), on.family_launches()) == counters
            assert (pxo.view(np.uint8) == 7).all() and (fam == -5).all() and (nul == -5).all() and (stp == -5).all()
            assert (out.view(np.uint8) == 7).all()
            return rc, msg

        ARG = -4                                                 # GCRE_ERR_ARG
        assert lib.gcre_score_sets_prefix(None, None, None, None, 0, None, None, None, None, None) == ARG
        rc, msg = call([0, 2, 5], [1, 2, 3, 4, 5], px=False)
        assert rc == ARG and msg == "score_sets_prefix: NULL argument (px_out)"
        rc, msg = call([0, 2, 2], [1, 2])
        assert rc == ARG and msg == "score_sets_prefix: set 1 has no members"
        rc, msg = call([0, 2], [1, N_ROWS])
        assert rc != 0 and msg == f"score_sets_prefix: set 0: member row {N_ROWS} out of range ({N_ROWS} rows)"
        rc, msg = call([0, 2], [1, 2], sg=[1, 0])
        assert rc == ARG and msg == "score_sets_prefix: set 0: sign 0 is neither +1 nor -1"
        rc, msg = call([0, 2], [1, 2], n_cols=n - 1)
        assert rc == ARG and msg == f"score_sets_prefix: the rows have {n - 1} columns, not n_cases + n_ctrls = {n}"
        rc, msg = call([0, 1, 2], [1, 2], cap=1)
        assert rc != 0 and msg == "score_sets_prefix: 2 sets, room for 1 records (out of range)"
        rc, msg = call([0, 2], [1, 2], on=bare)
        assert rc != 0 and msg == "assertion: score_sets_prefix needs a value table"
        # 3 steps x 1 half x 4 dwords x 4 bytes = 48 bytes (65 patients: two words, padded to four: 8 dwords -> 96)
        rc, msg = call([0, 1, 4], [1, 2, 3, 4], env={"GCRE_PREFIX_MAX_MB": "0.00005"})
        assert rc == ARG and msg == "score_sets_prefix: the 3 step rows of set 1 take 96 bytes: above GCRE_PREFIX_MAX_MB = 0.000050"
        rc, msg = call([0, 1, 4], [1, 2, 3, 4], env={"GCRE_PREFIX_MAX_MB": "0.001"}, null=True)
        assert rc == ARG and msg == "score_sets_prefix: the 1 step rows of set 0 take 8224 bytes: above GCRE_PREFIX_MAX_MB = 0.001000"
        # and the same list is accepted without the bound
        rec, px = ex.prefix_tests([[1], [2, 3, 4]], rows)
        assert px["steps"].tolist() == [1, 3] and ex.prefix_launches() == 4
    finally:
        ex.close()
        bare.close()


def test_launch_counters_are_apart(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(1870)
    n, nc, K = 33, 15, 100
    rows = make_rows(rng, n)
    sets = [[2, 3], [4, 5, 6]]
    ex = open_context(1, nc, n - nc, small_table(n, n, 2), K)
    try:
        assert ex.prefix_launches() == 0
        ex.score_sets(sets, rows)
        ex.family_tests(sets, rows)
        ex.score_sets(sets, rows, which=[0, 1], given=[1, 0])
        assert ex.prefix_launches() == 0                         # nobody else's launches count here
        fl, gl, others = ex.family_launches(), ex.given_launches, other_counters(ex)
        assert fl > 0 and gl > 0
        ex.prefix_tests(sets, rows)
        assert ex.prefix_launches() == 4
        assert (ex.family_launches(), ex.given_launches, other_counters(ex)) == (fl, gl, others)
        ex.prefix_tests([[-1, 2]], rows)                         # no valid set: nothing to launch
        assert ex.prefix_launches() == 4
    finally:
        ex.close()


@pytest.mark.parametrize("signed", [False, True])
def test_variable_threshold_test_columns(monkeypatch, signed):
    """Twelve sets: every column recomputed from the records of a context of the same seed."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rng = np.random.default_rng(1880 + signed)
    nc, nt, K, G = 60, 70, 200, 30
    n = nc + nt
    genes = [f"G{i}" for i in range(G)]
    data = (rng.random((G, n)) < rng.uniform(0.01, 0.3, size=(G, 1))).astype(np.int32)
    data[4] = data[5]                                            # a tie in the carrier totals
    names = [f"P{i}" for i in range(12)]
    sets = [[genes[j] for j in rng.choice(G, int(rng.integers(1, 9)), replace=False)] for _ in range(12)]
    sets[3] = ["G4", "G5", "G1"]
    sets[7] = ["G2", "nowhere"]                                  # a gene that is not in the table
    if signed:
        sets = [" -> ".join(f"{g} {'(+)' if rng.random() < 0.5 else '(-)'}" for g in s) for s in sets]
    df = report.variable_threshold_test(sets, genes, data, nc, nt, signed=signed, names=names, threshold=1.0, n_permutations=K, seed=5)
    assert list(df.columns) == report.VARIABLE_THRESHOLD_COLUMNS and df["Sets"].tolist() == names and len(df) == 12
    g2, d2 = report.preprocess_table(genes, data, 1.0, nc, nt)
    d2 = np.asarray(d2)
    _, rws, sgs = report.parse_sets(sets, g2)
    tot = (d2 != 0).sum(axis=1)
    osets, osigns, cuts = [], [], []
    for r, s in zip(rws, sgs):
        order, ct = report.threshold_order(r, d2)
        osets.append(np.asarray(r)[order].tolist())
        osigns.append(np.asarray(s)[order].tolist())
        cuts.append(ct.tolist())
    ex = api.JoinExec(2 if signed else 1, nc, nt, K)
    try:
        ex.set_value_table(api.values_table(nc, nt))
        ex.generate_permutations(5, None)
        rec, px, fam = ex.prefix_tests(osets, d2, osigns, cuts=cuts, family=True)
    finally:
        ex.close()
    ok = (rec["valid"] != 0) & (px["best_step"] >= 0)
    assert not ok[7] and ok.sum() >= 10
    assert df["Genes"].tolist() == [len(r) for r in rws]
    np.testing.assert_array_equal(bits(df["Scores"]), bits(rec["score"]))
    np.testing.assert_array_equal(bits(df["NominalPvalues"]), bits(rec["pvalue"]))
    np.testing.assert_array_equal(bits(df["AdaptiveScores"]), bits(np.where(ok, px["score"], np.nan)))
    np.testing.assert_array_equal(bits(df["AdaptivePvalues"]), bits(np.where(ok, px["n_ge"] / K, np.nan)))
    np.testing.assert_array_equal(bits(df["BestGenes"]), bits(np.where(ok, px["best_members"], np.nan)))
    thr = np.array([tot[osets[s][px["best_members"][s] - 1]] if ok[s] else np.nan for s in range(12)])
    np.testing.assert_array_equal(bits(df["BestThreshold"]), bits(thr))
    famp = np.array([(fam.astype(np.float64) >= px["score"][s]).sum() / K if ok[s] else np.nan for s in range(12)])
    np.testing.assert_array_equal(bits(df["AdaptiveFamilyPvalues"]), bits(famp))
    # the adaptive statistic is at least the full set's score, and its family p-value at least its own p-value
    assert (df["AdaptiveScores"][ok] >= df["Scores"][ok]).all() and (df["AdaptiveFamilyPvalues"][ok] >= df["AdaptivePvalues"][ok]).all()
    none = report.variable_threshold_test(sets, genes, data, nc, nt, signed=signed, threshold=1.0, n_permutations=0)
    assert none["Sets"].tolist() == [f"Set{i}" for i in range(12)]
    assert none[["BestGenes", "BestThreshold", "AdaptiveScores", "AdaptivePvalues", "AdaptiveFamilyPvalues"]].isna().all().all()


def test_seeded_fuzz(monkeypatch):
    """GCRE_PREFIX_FUZZ_CASES random calls (default 6; a long run is recorded in profiles/prefix_fuzz.txt)."""
    cases = int(os.environ.get("GCRE_PREFIX_FUZZ_CASES", "6"))
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    for case in range(cases):
        rng = np.random.default_rng([1890, case])
        method = int(rng.integers(1, 3))
        n = int(rng.integers(2, 300))
        nc = int(rng.integers(1, n))
        K = int(rng.choice([1, 37, 511, 512, 513, 1025, 2049]))
        n_rows = int(rng.integers(2, 30))
        rows = make_rows(rng, n, n_rows)
        S = int(rng.integers(1, 14))
        sets = [rng.integers(0, n_rows, int(rng.choice([1, 2, 3, 4, 5, 8, 9, 16, 17, 40]))).tolist() for _ in range(S)]
        if case % 3 == 0:
            sets[int(rng.integers(0, S))][0] = -1
        signs = None if case % 4 == 1 else [rng.choice([-1, 1], len(s)).tolist() for s in sets]
        cuts = None if case % 3 == 1 else [(rng.random(len(s)) < rng.uniform(0.1, 0.9)).astype(int).tolist() for s in sets]
        VT = small_table(n, n, case)
        VT[rng.random(VT.shape) < 0.05] *= -1
        VT[rng.random(VT.shape) < 0.02] = np.nan
        if case % 2:
            monkeypatch.setenv("GCRE_PREFIX_SLAB_SETS", str(int(rng.integers(1, 6))))
        ex = open_context(method, nc, n - nc, VT, K, seed=case)
        try:
            assert_equal_reference(ex, sets, rows, signs, cuts, f"fuzz case {case}")
        finally:
            ex.close()
            monkeypatch.delenv("GCRE_PREFIX_SLAB_SETS", raising=False)
