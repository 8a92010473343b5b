"""Step-down, k-FWER and FDR over a family of given sets on the device (gcre_score_sets_family: k_family_null, k_family_scan,
k_family_hist).  Everything ``JoinExec.family_tests(kmax=True, null=True)`` returns is compared, integers as
they are and floats as bits, against ``report.family_reference`` fed the null matrix that tests/test_sets_host.restate
recomputes from the context's masks and the value table, and against ``score_sets(family=True)``.  The shapes are the
smallest at which each part can go wrong: partial tiles, several slabs, padded mask words, families smaller than KMAX and
no multiple of a block's sets, more thresholds than the LDS histogram holds."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from geneticscre_amd import api, report
from helpers import small_table, special_table
from test_sets_host import restate

pytestmark = pytest.mark.gpu

HIST_BINS = 4096   # kFamilyHistBins, the capacity DESIGN.md §3.15 states
N_ROWS = 16


def device_masks(ex, K, n):
    if K == 0:
        return np.zeros((0, n), bool)
    w = np.stack([ex.perm_mask(r) for r in range(K)])
    return np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def make_rows(rng, n):
    rows = (rng.random((N_ROWS, n)) < rng.uniform(0.05, 0.6, size=(N_ROWS, 1))).astype(np.int8)
    rows[0], rows[1] = 1, 0            # everybody, nobody
    return rows


def make_sets(rng, V):
    """V valid sets and one with an NA member: duplicates (which tie), a set of non-carriers, members under both signs."""
    sets, signs = [], []
    for _ in range(V):
        L = int(rng.integers(1, 6))
        sets.append(rng.integers(2, N_ROWS, size=L).tolist())
        signs.append(rng.choice([-1, 1], size=L).tolist())
    sets[0], signs[0] = [1], [1]                                   # non-carriers
    if V >= 9:
        sets[3], signs[3] = [4, 4, 7], [1, -1, -1]                 # one gene under both signs
        sets[5], signs[5] = list(sets[4]), list(signs[4])          # a duplicate: a tie
        sets[8], signs[8] = list(sets[4]), list(signs[4])          # and a third of the group
        sets[6], signs[6] = [0, 1], [1, -1]                        # everybody (+), nobody (-)
    at = min(2, V)
    sets.insert(at, [3, -1, 5])                                    # an NA member
    signs.insert(at, [1, 1, -1])
    return sets, signs


def reference(method, nc, nt, sets, rows, signs, VT, masks):
    """(records of restate, family_reference of the recomputed null matrix, that matrix with NaN rows for invalid sets)."""
    with np.errstate(over="ignore", invalid="ignore"):
        want, wnull, wfam = restate(method, nc, nt, sets, rows, signs, VT, masks)
    K = len(masks)
    null = np.full((len(sets), K), np.nan, np.float32)
    for s, v in enumerate(wnull):
        if v is not None:
            null[s] = v
    obs = np.array([w["score"] for w in want], np.float64)
    valid = np.array([w["valid"] for w in want])
    return want, report.family_reference(obs, valid, null), null, wfam


def assert_family(got, ref, null, what=""):
    rec, fam, km, nul = got
    assert fam.dtype == api.FAMILY_SCORE and km.dtype == np.float32 and nul.dtype == np.float32
    for f in ("n_ge_stepdown", "exceed", "observed"):
        np.testing.assert_array_equal(fam[f], ref[f], err_msg=f"{what} {f}")
    np.testing.assert_array_equal(km.view(np.uint32), ref["kmax"].view(np.uint32), err_msg=f"{what} kmax")
    assert np.isnan(nul).tolist() == np.isnan(null).tolist(), what
    ok = ~np.isnan(null)
    np.testing.assert_array_equal(nul[ok].view(np.uint32), null[ok].view(np.uint32), err_msg=f"{what} null")


def assert_records(rec, want):
    for s, w in enumerate(want):
        for f in ("valid", "cases", "ctrls", "cases_pos", "ctrls_pos", "cases_neg", "ctrls_neg", "n_ge"):
            assert rec[f][s] == w[f], (s, f)
        assert np.float64(rec["score"][s]).view(np.uint64) == np.float64(w["score"]).view(np.uint64) or \
            (np.isnan(w["score"]) and np.isnan(rec["score"][s])), s


def check_context(ex, method, nc, nt, K, sets, rows, signs, VT, what=""):
    """One family on one context, against the reference and against score_sets(family=True)."""
    n = nc + nt
    masks = device_masks(ex, K, n)
    want, ref, null, wfam = reference(method, nc, nt, sets, rows, signs, VT, masks)
    got = ex.family_tests(sets, rows, signs, kmax=True, null=True)
    assert_records(got[0], want)
    assert_family(got, ref, null, what)
    rec2, fmax = ex.score_sets(sets, rows, signs, family=True)
    assert got[0].tobytes() == rec2.tobytes(), what                            # identical records
    np.testing.assert_array_equal(got[2][0].view(np.uint32), fmax.view(np.uint32), err_msg=what)
    np.testing.assert_array_equal(fmax.view(np.uint32), wfam.view(np.uint32), err_msg=what)
    V = int(sum(w["valid"] for w in want))
    assert not got[2][min(V, api.FAMILY_KMAX):].any()                          # fewer valid sets than KMAX: zero rows
    return got, ref


def open_context(method, nc, nt, K, VT, seed):
    ex = api.JoinExec(method, nc, nt, K)
    ex.set_value_table(VT)
    if K > 0:
        ex.generate_permutations(seed, None if seed % 2 else (np.arange(nc + nt) * 7 % 3).astype(np.int32))
    return ex


# permutations x patients, the family sizes dealt over them so that every size meets every K and every cohort once per method
KS, NS, VS = (1, 100, 512, 700), (2, 33, 70, 200), (1, 9, 17, 37)
SHAPES = [(K, n, VS[(i + j) % 4]) for i, K in enumerate(KS) for j, n in enumerate(NS)]


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("K,n,V", SHAPES)
def test_family_against_the_reference(method, K, n, V):
    i = SHAPES.index((K, n, V))
    rng = np.random.default_rng(1500 + 100 * method + i)
    nc = max(1, n // 2 - 1)
    nt = n - nc
    rows = make_rows(rng, n)
    sets, signs = make_sets(rng, V)
    VT = small_table(n, n, i)
    VT[rng.random(VT.shape) < 0.05] *= -1          # negatives fold as 0 in the null, and count when the score is one
    ex = open_context(method, nc, nt, K, VT, 40 + i)
    try:
        before = ex.family_launches()
        got, ref = check_context(ex, method, nc, nt, K, sets, rows, signs, VT, f"K={K} n={n} V={V}")
        assert ex.family_launches() == before + 3                               # one slab: null, scan, hist
        if V >= 9:
            tie = [5, 6, 9]                                                     # the duplicates, behind the inserted NA set
            assert len({int(got[1]["n_ge_stepdown"][s]) for s in tie}) == 1 and got[1]["observed"][tie[0]] >= 3
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_slabs_do_not_change_the_results(method, monkeypatch):
    """1,300 permutations in slabs of 512 -- three, the last one partial -- and in one: equal, and equal to the reference."""
    K, n, V = 1300, 70, 37
    nc, nt = 33, 37
    rng = np.random.default_rng(1700 + method)
    rows = make_rows(rng, n)
    sets, signs = make_sets(rng, V)
    VT = small_table(n, n, 7)
    ex = open_context(method, nc, nt, K, VT, 61)
    try:
        monkeypatch.delenv("GCRE_FAMILY_SLAB_PERMS", raising=False)
        monkeypatch.delenv("GCRE_FAMILY_MAX_MB", raising=False)
        l0 = ex.family_launches()
        whole, ref = check_context(ex, method, nc, nt, K, sets, rows, signs, VT, "one slab")
        bare = ex.family_tests(sets, rows, signs)                               # without the optional arrays: the same records
        assert len(bare) == 2 and bare[0].tobytes() == whole[0].tobytes() and bare[1].tobytes() == whole[1].tobytes()
        l1 = ex.family_launches()
        monkeypatch.setenv("GCRE_FAMILY_SLAB_PERMS", "512")
        slabs = ex.family_tests(sets, rows, signs, kmax=True, null=True)
        l2 = ex.family_launches()
        assert (l1 - l0, l2 - l1) == (6, 9)                                     # two calls of one slab, one of three
        for a, b in zip(whole, slabs):
            assert a.tobytes() == b.tobytes()
        # the memory bound cuts the same slabs: 37 valid rows x 512 permutations x 4 bytes is one tile, and 1.5 fit
        monkeypatch.delenv("GCRE_FAMILY_SLAB_PERMS")
        monkeypatch.setenv("GCRE_FAMILY_MAX_MB", repr(V * 512 * 4 * 1.5 / 1048576.0))
        bound = ex.family_tests(sets, rows, signs, kmax=True, null=True)
        assert ex.family_launches() - l2 == 9
        for a, b in zip(whole, bound):
            assert a.tobytes() == b.tobytes()
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("kind,variant", [("zeros", 0), ("nonfinite", 0), ("nonfinite", 2)])
def test_special_scores(kind, variant, method):
    """Tables of signed zeros (observed scores of -0.0 and +0.0 tie) and of NaN and infinities (a NaN observed score: first in
    the walk, in no D, counted nowhere)."""
    K, n, nc = 100, 70, 33
    nt = n - nc
    rng = np.random.default_rng(1800 + method)
    rows = make_rows(rng, n)
    sets, signs = make_sets(rng, 17)
    sets += [[r] for r in range(2, N_ROWS)]                 # every row alone: more cells of the table among the scores
    signs += [[1 if r % 2 else -1] for r in range(2, N_ROWS)]
    VT = special_table(kind, n, n, 3, variant)
    if kind == "zeros":
        VT[0, 0] = -0.0                                     # the empty half of the signed method: -0.0 + -0.0 stays -0.0
    ex = open_context(method, nc, nt, K, VT, 71)
    try:
        got, ref = check_context(ex, method, nc, nt, K, sets, rows, signs, VT, f"{kind}{variant}")
        score = got[0]["score"][got[0]["valid"] != 0]
        if kind == "zeros":
            zeros = score[score == 0.0]
            assert len({bool(np.signbit(z)) for z in zeros}) == 2, "no -0.0 / +0.0 tie among the observed scores"
        elif variant == 0:
            assert np.isnan(score).any(), "no NaN observed score"
            s = int(np.flatnonzero((got[0]["valid"] != 0) & np.isnan(got[0]["score"]))[0])
            assert (got[1]["n_ge_stepdown"][s], got[1]["exceed"][s], got[1]["observed"][s]) == (0, 0, 0)
    finally:
        ex.close()


def test_more_thresholds_than_the_histogram_holds():
    """A family whose distinct observed scores exceed the LDS histogram's capacity: k_family_hist walks the bins in passes.
    Sets of one (+) and one (-) row under the signed method: the scores are sums of two cells."""
    K, n, nc = 512, 70, 33
    nt = n - nc
    rng = np.random.default_rng(1900)
    R = 100
    rows = (rng.random((R, n)) < rng.uniform(0.0, 1.0, size=(R, 1))).astype(np.int8)
    sets = [[a, b] for a in range(R) for b in range(R) if a != b][:7000]
    signs = [[1, -1]] * len(sets)
    VT = small_table(n, n, 11)
    ex = open_context(2, nc, nt, K, VT, 81)
    try:
        before = ex.family_launches()
        got, ref = check_context(ex, 2, nc, nt, K, sets, rows, signs, VT, "passes")
        assert ex.family_launches() == before + 3
        assert len(np.unique(got[0]["score"])) > HIST_BINS
    finally:
        ex.close()


def _raw_call(ex, sets, rows, signs, n, fam_null=False, cap=None):
    """gcre_score_sets_family through ctypes on arrays filled with a pattern: (return code, the arrays)."""
    lib = api._family_lib()
    inp, keep = api._set_input(sets, rows, signs, n)
    S = len(sets)
    out = np.full(max(S, 1), 0x5a, dtype=np.uint8).repeat(api.SET_SCORE.itemsize).view(api.SET_SCORE)
    fam = np.full(max(S, 1) * 3, 0x5a5a5a5a, dtype=np.int64).view(api.FAMILY_SCORE)
    km = np.full((api.FAMILY_KMAX, ex.iters), 7.5, np.float32)
    nul = np.full((S, ex.iters), 7.5, np.float32)
    n_out = ctypes.c_int64(0)
    rc = lib.gcre_score_sets_family(ex._h, ctypes.byref(inp), api._ptr(out), len(out) if cap is None else cap, ctypes.byref(n_out),
                                    None if fam_null else api._ptr(fam), api._ptr(km), api._ptr(nul))
    del keep
    return rc, (out, fam, km, nul)


def _untouched(arrays):
    out, fam, km, nul = arrays
    return (out.view(np.uint8) == 0x5a).all() and (fam.view(np.int64) == 0x5a5a5a5a).all() and (km == 7.5).all() and (nul == 7.5).all()


def test_refusals_launch_nothing_and_write_nothing(monkeypatch):
    nc, nt, K = 20, 25, 600
    n = nc + nt
    rng = np.random.default_rng(2000)
    rows = make_rows(rng, n)
    VT = small_table(n, n, 1)
    sets, signs = [[2, 3], [4], [5, 6, 7]], [[1, -1], [1], [-1, 1, 1]]
    monkeypatch.delenv("GCRE_FAMILY_SLAB_PERMS", raising=False)
    monkeypatch.delenv("GCRE_FAMILY_MAX_MB", raising=False)
    fresh = api.JoinExec(2, nc, nt, K)
    try:
        assert fresh.family_launches() == 0
        rc, arrays = _raw_call(fresh, sets, rows, signs, n)
        assert rc == api.GCRE_ERR_ASSERT and b"value table" in fresh._lib.gcre_last_error(fresh._h) and _untouched(arrays)
        fresh.set_value_table(VT)
        rc, arrays = _raw_call(fresh, sets, rows, signs, n)
        assert rc == api.GCRE_ERR_ASSERT and b"permutation masks" in fresh._lib.gcre_last_error(fresh._h) and _untouched(arrays)
        with pytest.raises(api.GcreError, match="permutation masks"):
            fresh.family_tests(sets, rows, signs)
        assert fresh.family_launches() == 0
    finally:
        fresh.close()
    ex = open_context(2, nc, nt, K, VT, 5)
    try:
        refused = [
            (dict(sets=[[2], []], signs=None), api.GCRE_ERR_ARG, b"has no members"),
            (dict(sets=[[2, 3]], signs=[[1, 0]]), api.GCRE_ERR_ARG, b"neither"),
            (dict(sets=[[2], [3, N_ROWS]], signs=None), api.GCRE_ERR_RANGE, b"out of range"),
            (dict(sets=sets, signs=signs, cap=2), api.GCRE_ERR_RANGE, b"room for 2"),
            (dict(sets=sets, signs=signs, fam_null=True), api.GCRE_ERR_ARG, b"fam_out"),
        ]
        for kw, code, msg in refused:
            rc, arrays = _raw_call(ex, kw["sets"], rows, kw["signs"], n, fam_null=kw.get("fam_null", False), cap=kw.get("cap"))
            assert rc == code and msg in ex._lib.gcre_last_error(ex._h), (kw, rc, ex._lib.gcre_last_error(ex._h))
            assert _untouched(arrays), kw
        rc, arrays = _raw_call(ex, sets, np.zeros((N_ROWS, n + 1), np.int8), signs, n + 1)
        assert rc == api.GCRE_ERR_ARG and _untouched(arrays)
        # one row of one tile above the limit: three valid sets x 512 permutations x 4 bytes = 6,144 bytes
        monkeypatch.setenv("GCRE_FAMILY_MAX_MB", repr(6143 / 1048576.0))
        rc, arrays = _raw_call(ex, sets, rows, signs, n)
        assert rc == api.GCRE_ERR_ARG and b"GCRE_FAMILY_MAX_MB" in ex._lib.gcre_last_error(ex._h) and _untouched(arrays)
        with pytest.raises(api.GcreError, match="GCRE_FAMILY_MAX_MB"):
            ex.family_tests(sets, rows, signs)
        assert ex.family_launches() == 0
        monkeypatch.setenv("GCRE_FAMILY_MAX_MB", repr(6144 / 1048576.0))          # exactly one tile: two slabs
        rc, arrays = _raw_call(ex, sets, rows, signs, n)
        assert rc == api.GCRE_OK and ex.family_launches() == 6 and not _untouched(arrays)
        monkeypatch.delenv("GCRE_FAMILY_MAX_MB")
        check_context(ex, 2, nc, nt, K, sets, rows, signs, VT, "after the refusals")
        # an empty family, and one without a valid set: nothing is launched
        before = ex.family_launches()
        rec, fam, km = ex.family_tests([], rows, kmax=True)
        assert len(rec) == 0 and len(fam) == 0 and km.shape == (api.FAMILY_KMAX, K) and not km.any()
        rec, fam, km, nul = ex.family_tests([[2, -1]], rows, kmax=True, null=True)
        assert rec["valid"].tolist() == [0] and fam.tolist() == [(-1, 0, -1)] and not km.any() and np.isnan(nul).all()
        assert ex.family_launches() == before
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_no_permutations(method):
    """iterations == 0: the records of score_sets, zeros for the valid sets, nothing of the family launched."""
    nc, nt = 20, 25
    n = nc + nt
    rng = np.random.default_rng(2100)
    rows = make_rows(rng, n)
    sets, signs = make_sets(rng, 9)
    ex = open_context(method, nc, nt, 0, small_table(n, n, 2), 0)
    try:
        rec, fam, km, nul = ex.family_tests(sets, rows, signs, kmax=True, null=True)
        assert rec.tobytes() == ex.score_sets(sets, rows, signs).tobytes()
        assert km.shape == (api.FAMILY_KMAX, 0) and nul.shape == (len(sets), 0)
        valid = rec["valid"] != 0
        assert fam[valid].tolist() == [(0, 0, 0)] * int(valid.sum()) and fam[~valid].tolist() == [(-1, 0, -1)]
        assert ex.family_launches() == 0
    finally:
        ex.close()


@pytest.mark.parametrize("signed", [False, True])
def test_score_paths_family_inference(signed):
    """The columns score_paths appends are family_columns of the reference; the default call is the frame it was."""
    nc, nt, K, G = 33, 37, 700, 40
    n = nc + nt
    rng = np.random.default_rng(2200 + signed)
    genes = [f"G{i}" for i in range(G)]
    data = (rng.random((G, n)) < 0.15).astype(np.int32)
    tags = ["(+)", "(-)"]
    paths = [" -> ".join(f"{genes[g]} {tags[int(rng.integers(0, 2))]}" for g in rng.choice(G, size=int(rng.integers(1, 5)), replace=False))
             for _ in range(28)]
    paths += [paths[3], "NOSUCHGENE (+) -> G1 (-)"]                  # a tie and an NA row: 30 paths
    kw = dict(signed=signed, threshold=0.9, n_permutations=K, seed=77)
    plain = report.score_paths(paths, genes, data, nc, nt, **kw)
    full = report.score_paths(paths, genes, data, nc, nt, family_inference=True, **kw)
    assert list(plain.columns) == report.SCORE_PATHS_COLUMNS
    assert list(full.columns) == report.SCORE_PATHS_COLUMNS + report.FAMILY_COLUMNS
    assert plain.equals(report.score_paths(paths, genes, data, nc, nt, family_inference=False, **kw))
    assert plain.equals(full[report.SCORE_PATHS_COLUMNS])
    # the reference: the same rows, table and masks on a context of our own
    method = 2 if signed else 1
    g2, d2 = report.preprocess_table(genes, data, 0.9, nc, nt)
    _, prow, psign = report.parse_sets(paths, g2)
    ex = api.JoinExec(method, nc, nt, K)
    try:
        VT = api.values_table(nc, nt)
        ex.set_value_table(VT)
        ex.generate_permutations(77, None)
        masks = device_masks(ex, K, n)
    finally:
        ex.close()
    want, ref, null, _ = reference(method, nc, nt, prow, np.asarray(d2), psign, VT, masks)
    score = np.array([w["score"] for w in want])
    valid = np.array([w["valid"] for w in want])
    np.testing.assert_array_equal(full["Scores"].to_numpy().view(np.uint64)[valid != 0], score.view(np.uint64)[valid != 0])
    cols = report.family_columns(score, valid, ref, ref["kmax"], K)
    for c in report.FAMILY_COLUMNS:
        np.testing.assert_array_equal(full[c].to_numpy(), cols[c], err_msg=c)
    assert np.isnan(full[report.FAMILY_COLUMNS].to_numpy()[-1]).all()                      # the NA row
    ok = valid != 0
    assert (full["FamilyPvaluesStepDown"][ok] <= full["FamilyPvalues"][ok]).all()
    assert (full["FamilyPvaluesStepDown"][ok] >= full["NominalPvalues"][ok]).all()
    assert full["FamilyPvaluesStepDown"].iat[3] == full["FamilyPvaluesStepDown"].iat[28]     # the tie


# ---- seeded fuzz: a handful of cases by default, GCRE_FAMILY_FUZZ_CASES asks for a long run ------------------------------


def fuzz_case(case):
    rng = np.random.default_rng([2300, case])
    method = int(rng.integers(1, 3))
    n = int(rng.choice([2, 3, 31, 32, 33, 64, 65, 70, 129, 200, 260]))
    nc = int(rng.integers(1, n))
    nt = n - nc
    K = int(rng.choice([1, 2, 63, 64, 100, 511, 512, 513, 700, 1024, 1300]))
    V = int(rng.choice([1, 2, 7, 8, 9, 10, 11, 15, 16, 17, 33, 37, 64, 90]))
    rows = make_rows(rng, n)
    sets, signs = make_sets(rng, V)
    kind = str(rng.choice(["small", "small", "zeros", "nonfinite", "ladder"]))
    VT = small_table(n, n, case) if kind == "small" else special_table(kind, n, n, case, int(rng.integers(0, 3)) if kind == "nonfinite" else 0)
    slab = int(rng.choice([0, 0, 512, 1024]))
    return method, nc, nt, K, sets, rows, signs, VT, slab, f"case {case}: method {method} n={n} K={K} V={V} {kind} slab={slab}"


def test_seeded_fuzz(monkeypatch):
    cases = int(os.environ.get("GCRE_FAMILY_FUZZ_CASES", "6"))
    monkeypatch.delenv("GCRE_FAMILY_MAX_MB", raising=False)
    for case in range(cases):
        method, nc, nt, K, sets, rows, signs, VT, slab, what = fuzz_case(case)
        if slab:
            monkeypatch.setenv("GCRE_FAMILY_SLAB_PERMS", str(slab))
        else:
            monkeypatch.delenv("GCRE_FAMILY_SLAB_PERMS", raising=False)
        ex = open_context(method, nc, nt, K, VT, 300 + case)
        try:
            check_context(ex, method, nc, nt, K, sets, rows, signs, VT, what)
        finally:
            ex.close()
    print(f"family fuzz: {cases} cases equal the reference")
