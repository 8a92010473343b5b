"""Sequential permutation p-values on the device (gcre_score_sets_sequential: k_seq_masks, k_seq_null, k_seq_retire; DESIGN.md
§3.21).  Every count ``JoinExec.sequential_tests`` returns is compared as an integer, for every set, with the definition in
numpy alone: ``report.permutation_masks``, the null scores through the value table, ``report.sequential_reference``.  The
cohorts are 70 + 61 patients (five dwords: neither a dword nor a qword multiple) and 33 + 31, without strata, with 3 (need /
rem in registers) and with 7 (in memory); the batches are cut at 512 and 1,024 permutations, by bytes and not at all, and no
value may move."""
from __future__ import annotations

import os

import numpy as np
import pytest

from geneticscre_amd import api, report

pytestmark = pytest.mark.gpu

N_ROWS = 90
PERM_SEED = 11
HITS = 5                    # of the class tests
CAP = 512                   # ... and their batch cap: one tile
P_MAX = 20001               # the most permutations any test here asks for
ENV = ("GCRE_SEQ_MAX_MB", "GCRE_SEQ_BATCH_PERMS")
COUNTERS = [("given", "gcre_given_launches"), ("family", "gcre_family_launches"), ("minp", "gcre_minp_launches"),
            ("compete", "gcre_compete_launches"), ("prefix", "gcre_prefix_launches"), ("subsample", "gcre_subsample_launches"),
            ("dose", "gcre_dose_launches"), ("overlap", "gcre_overlap_launches"), ("clump", "gcre_clump_launches"),
            ("patients", "gcre_patient_launches"), ("burden", "gcre_burden_launches"), ("stepdown", "gcre_stepdown_launches"),
            ("hits", "gcre_hits_launches")]

# (method, cases, controls, strata) -> (the trial of make_input, max_perms): found on the CPU by tools/sequential_seeds.py so
# that the reference alone puts a set into every class of `classes_of` at HITS hits and CAP permutations a batch
CLASS_CASES = {
    (1, 70, 61, 1): (233, 7771),
    (1, 70, 61, 3): (64, 16646),
    (1, 33, 31, 1): (173, 14015),
    (1, 33, 31, 3): (52, 16338),
    (2, 70, 61, 1): (6, 7723),
    (2, 70, 61, 3): (23, 17086),
    (2, 33, 31, 1): (17, 19289),
    (2, 33, 31, 3): (0, 8024),
}


def other_counters(ex):
    """Every launch counter of the context but the stage's own."""
    return [int(getattr(api._feature_lib(f), sym)(ex._h)) for f, sym in COUNTERS]


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)


def make_strata(rng, n, ns):
    if ns == 1:
        return None
    st = rng.integers(0, ns, n)
    st[:ns] = np.arange(ns)            # every stratum is there
    return st.astype(np.int32)


def make_input(method, nc, nt, ns, trial=0):
    """(rows, sets, signs, strata): about 40 sets on 90 gene rows whose carriers lean towards the cases by various amounts --
    one-gene sets, 3-5-gene signed paths, two 60-gene sets, a duplicate, a set with an NA member, a set without carriers
    (every permutation ties its score) and a set planted on the cases (no permutation reaches it)."""
    n = nc + nt
    rng = np.random.default_rng([7300, method, nc, nt, ns, trial])
    freq = rng.uniform(0.05, 0.4, size=(N_ROWS, 1))
    lean = rng.uniform(0.0, 0.7, size=(N_ROWS, 1))
    p = np.where(np.arange(n)[None, :] < nc, freq * (1 + lean), freq * (1 - lean))
    rows = (rng.random((N_ROWS, n)) < p).astype(np.int8)
    rows[0] = 0                                                     # nobody
    rows[1] = (np.arange(n) < nc).astype(np.int8)                   # the cases and nobody else
    sets = [[int(g)] for g in rng.integers(2, N_ROWS, 12)]
    sets += [rng.integers(2, N_ROWS, int(k)).tolist() for k in rng.integers(3, 6, 18)]
    sets += [rng.permutation(np.arange(2, N_ROWS))[:60].tolist() for _ in range(2)]
    sets += [list(sets[14]), [4, -1, 9], [0], [1], [1, 0]]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    signs[32] = list(signs[14])                                     # the duplicate, signs and all
    signs[34], signs[35], signs[36] = [1], [1], [1, 1]              # (in method 2 a (-) planted row would score the controls)
    return rows, sets, signs, make_strata(rng, n, ns)


def reference_null(method, sets, signs, rows, nc, VT, masks):
    """(obs [S], null [S][perms] float32, valid [S]) of ``score_sets`` under the given masks, bool [perms][n], in numpy."""
    d = np.asarray(rows) != 0
    n = d.shape[1]
    case = np.arange(n) < nc
    mk = np.asarray(masks).astype(np.int32)
    S = len(sets)
    obs, valid = np.full(S, np.nan), np.zeros(S, int)
    null = np.zeros((S, len(mk)), np.float32)
    for s, m in enumerate(sets):
        m = np.asarray(m, np.int64)
        if (m < 0).any():
            continue
        valid[s] = 1
        sg = np.ones(len(m), np.int64) if signs is None else np.asarray(signs[s], np.int64)
        neg = (sg == -1) if method == 2 else np.zeros(len(m), bool)
        P = d[m[~neg]].any(axis=0) if (~neg).any() else np.zeros(n, bool)
        N = d[m[neg]].any(axis=0) if neg.any() else np.zeros(n, bool)
        a, tp = mk @ P.astype(np.int32), int(P.sum())
        o = report._vt_cell(VT, n, (P & case).sum(), (P & ~case).sum())
        with np.errstate(invalid="ignore"):
            if method == 1:
                null[s] = report._fold_f32(report._vt_cell(VT, n, a, tp - a))
            else:
                b, tn = mk @ N.astype(np.int32), int(N.sum())
                o = o + report._vt_cell(VT, n, (N & ~case).sum(), (N & case).sum())
                null[s] = report._fold_f32(report._vt_max(VT, n, a, tp - a) + report._vt_max(VT, n, tn - b, b))
        obs[s] = float(o)
    return obs, null, valid


def classes_of(ref, valid, max_perms, cap, first=None):
    """How many valid sets the reference puts into every class the batches can treat differently: cap = permutations a batch."""
    first = cap if first is None else first
    ok = valid != 0
    n_hit, n_perm, stopped = ref["n_hit"], ref["n_perm"], ref["stopped"] != 0
    later = ok & stopped & (n_perm > first)
    return {"stopped inside the first batch": int((ok & stopped & (n_perm <= first)).sum()),
            "stopped in a later batch": int(later.sum()),
            "stopped on the last permutation of a batch": int((ok & stopped & (n_perm % cap == 0)).sum()),
            "stopped at max_perms": int((ok & stopped & (n_perm == max_perms)).sum()),
            "never stopped, hits": int((ok & ~stopped & (n_hit > 0)).sum()),
            "never stopped, no hit": int((ok & ~stopped & (n_hit == 0)).sum())}


def open_context(method, nc, nt, VT, K=0, seed=PERM_SEED, strata=None):
    ex = api.JoinExec(method, nc, nt, K)
    ex.set_value_table(VT)
    if K > 0:
        ex.generate_permutations(seed, strata)
    return ex


def assert_equal(seq, ref, what=""):
    for k in ("n_hit", "n_perm", "stopped"):
        assert seq[k].dtype == ref[k].dtype
        np.testing.assert_array_equal(seq[k], ref[k], err_msg=f"{what} {k}")


_NULLS = {}


def problem(method, nc, nt, ns, trial=0):
    """The input of a configuration and its reference null matrix over P_MAX permutations: computed once, never changed."""
    key = (method, nc, nt, ns, trial)
    if key not in _NULLS:
        rows, sets, signs, strata = make_input(method, nc, nt, ns, trial)
        VT = api.values_table(nc, nt)
        masks = report.permutation_masks(nc, nt, P_MAX, PERM_SEED, strata)
        obs, null, valid = reference_null(method, sets, signs, rows, nc, VT, masks)
        for a in (obs, null, valid, masks):
            a.setflags(write=False)
        _NULLS[key] = (rows, sets, signs, strata, VT, obs, null, valid)
    return _NULLS[key]


CONFIGS = [(m, nc, nt, ns) for m in (1, 2) for nc, nt in ((70, 61), (33, 31)) for ns in (1, 3)]


# ---- every class of set, every set as integers -----------------------------------------------------------------------------


@pytest.mark.parametrize("method,nc,nt,ns", CONFIGS)
def test_every_class_of_set(monkeypatch, method, nc, nt, ns):
    trial, max_perms = CLASS_CASES[(method, nc, nt, ns)]
    rows, sets, signs, strata, VT, obs, null, valid = problem(method, nc, nt, ns, trial)
    ref = report.sequential_reference(null, obs, valid, HITS, max_perms)
    found = classes_of(ref, valid, max_perms, CAP)
    print(found)
    assert all(v > 0 for v in found.values()), found                 # from the reference alone: the input covers every class
    assert ref["n_perm"][34] == HITS and ref["stopped"][34] == 1     # no carriers: every permutation ties the score
    assert ref["n_hit"][35] == 0 and ref["stopped"][35] == 0         # planted on the cases: never reached
    assert ref["n_hit"][33] == -1 and ref["n_perm"][33] == -1        # an NA member
    assert ref["n_perm"][32] == ref["n_perm"][14]                    # the duplicate
    monkeypatch.setenv("GCRE_SEQ_BATCH_PERMS", str(CAP))
    ex = open_context(method, nc, nt, VT)
    try:
        plain = ex.score_sets(sets, rows, signs)
        others = other_counters(ex)
        assert ex.sequential_launches() == 0
        rec, seq = ex.sequential_tests(sets, rows, signs, hits=HITS, max_perms=max_perms, seed=PERM_SEED, strata=strata)
        assert rec.tobytes() == plain.tobytes()                       # the records of score_sets
        assert seq.dtype == api.SEQ_SCORE and len(seq) == len(sets)
        np.testing.assert_array_equal(rec["score"][valid != 0], obs[valid != 0])
        assert_equal(seq, ref, f"{(method, nc, nt, ns)}")
        # three kernels a batch, and batches until the last active set has stopped or max_perms is reached
        last = max_perms if found["never stopped, hits"] + found["never stopped, no hit"] else int(ref["n_perm"].max())
        assert ex.sequential_launches() == 3 * ((last + CAP - 1) // CAP)
        assert other_counters(ex) == others
    finally:
        ex.close()


@pytest.mark.parametrize("method,nc,nt,ns", [(1, 70, 61, 1), (2, 70, 61, 3), (2, 33, 31, 1), (1, 33, 31, 3)])
def test_no_value_depends_on_the_batches(monkeypatch, method, nc, nt, ns):
    """hits x max_perms x batch cap, and a byte bound that leaves one tile: against the reference, so equal to each other."""
    rows, sets, signs, strata, VT, obs, null, valid = problem(method, nc, nt, ns, CLASS_CASES[(method, nc, nt, ns)][0])
    ex = open_context(method, nc, nt, VT)
    try:
        for h in (1, 5, 20):
            for max_perms in (0, 700, 3000, P_MAX):
                ref = report.sequential_reference(null, obs, valid, h, max_perms)
                for cap, mb in (("512", None), ("1024", None), (None, None), (None, "0.01")):
                    for var, val in (("GCRE_SEQ_BATCH_PERMS", cap), ("GCRE_SEQ_MAX_MB", mb)):
                        if val is None:
                            monkeypatch.delenv(var, raising=False)
                        else:
                            monkeypatch.setenv(var, val)
                    before = ex.sequential_launches()
                    rec, seq = ex.sequential_tests(sets, rows, signs, hits=h, max_perms=max_perms, seed=PERM_SEED, strata=strata)
                    assert_equal(seq, ref, f"h={h} max_perms={max_perms} cap={cap} mb={mb}")
                    if max_perms == 0:
                        assert ex.sequential_launches() == before
        # the schedule without a cap: 4,096, then 16,384 -- two batches when a set runs to the end
        assert report.sequential_reference(null, obs, valid, 20, P_MAX)["stopped"][35] == 0
        monkeypatch.delenv("GCRE_SEQ_MAX_MB")
        before = ex.sequential_launches()
        ex.sequential_tests(sets, rows, signs, hits=20, max_perms=P_MAX, seed=PERM_SEED, strata=strata)
        assert ex.sequential_launches() == before + 3 * 2
    finally:
        ex.close()


@pytest.mark.parametrize("method", [1, 2])
def test_seven_strata_and_a_nan_score(monkeypatch, method):
    """More strata than k_seq_masks keeps in registers, and a table whose cell under one set's observed counts is NaN: that
    set's score is NaN, it never counts, never stops, and the NaN cell folds to 0 wherever a permutation of another set reads
    it."""
    nc, nt, ns = 70, 61, 7
    rows, sets, signs, strata = make_input(method, nc, nt, ns)
    VT = api.values_table(nc, nt).copy()
    d = rows != 0
    g = sets[3][0]
    signs[3] = [1]
    VT[int(d[g, :nc].sum()), int(d[g, nc:].sum())] = np.nan
    masks = report.permutation_masks(nc, nt, 3000, PERM_SEED, strata)
    obs, null, valid = reference_null(method, sets, signs, rows, nc, VT, masks)
    assert np.isnan(obs[3]) and np.isnan(obs).sum() < 6
    ex = open_context(method, nc, nt, VT)
    try:
        for h, max_perms, cap in ((5, 3000, "512"), (1, 1500, None), (20, 2999, "1024")):
            if cap is None:
                monkeypatch.delenv("GCRE_SEQ_BATCH_PERMS", raising=False)
            else:
                monkeypatch.setenv("GCRE_SEQ_BATCH_PERMS", cap)
            ref = report.sequential_reference(null, obs, valid, h, max_perms)
            rec, seq = ex.sequential_tests(sets, rows, signs, hits=h, max_perms=max_perms, seed=PERM_SEED, strata=strata)
            assert_equal(seq, ref, f"h={h} max_perms={max_perms}")
            assert np.isnan(rec["score"][3])
            assert seq["n_hit"][3] == 0 and seq["n_perm"][3] == max_perms and seq["stopped"][3] == 0
    finally:
        ex.close()


# ---- against the kernels that were there before ------------------------------------------------------------------------------


@pytest.mark.parametrize("method,nc,nt,ns", [(1, 70, 61, 3), (2, 70, 61, 1), (2, 33, 31, 3), (1, 70, 61, 7)])
def test_counts_equal_score_sets_when_nothing_stops(method, nc, nt, ns):
    """hits above max_perms: nothing stops, and n_hit is the n_ge of score_sets on a context that holds permutations
    0 .. max_perms-1 of generate_permutations(seed, strata).  The sequential call runs on that context too, and on one without
    masks."""
    rows, sets, signs, strata = make_input(method, nc, nt, ns)
    VT = api.values_table(nc, nt)
    max_perms = 3000
    full = open_context(method, nc, nt, VT, K=max_perms, seed=PERM_SEED, strata=strata)
    bare = open_context(method, nc, nt, VT)
    try:
        want = full.score_sets(sets, rows, signs)
        valid = want["valid"] != 0
        for ex in (full, bare):
            rec, seq = ex.sequential_tests(sets, rows, signs, hits=max_perms + 1, max_perms=max_perms, seed=PERM_SEED, strata=strata)
            assert not seq["stopped"].any()
            np.testing.assert_array_equal(seq["n_hit"][valid], want["n_ge"][valid])
            assert (seq["n_perm"][valid] == max_perms).all() and (seq["n_hit"][~valid] == -1).all() and (seq["n_perm"][~valid] == -1).all()
        rec, _ = full.sequential_tests(sets, rows, signs, hits=3, max_perms=500, seed=PERM_SEED + 1, strata=strata)
        assert rec.tobytes() == want.tobytes()               # the records keep the context's own n_ge / pvalue
        assert np.isnan(bare.sequential_tests(sets, rows, signs, hits=3, max_perms=500)[0]["pvalue"]).all()
    finally:
        full.close()
        bare.close()


def test_score_paths_columns():
    """``sequential=0`` is the frame as it was; with a limit the four columns are ``sequential_columns`` of the reference."""
    nc, nt = 70, 61
    rng = np.random.default_rng(7500)
    genes = [f"G{i}" for i in range(30)]
    data = (rng.random((30, nc + nt)) < rng.uniform(0.1, 0.4, size=(30, 1))).astype(np.int32)
    data[:, :nc] |= (rng.random((30, nc)) < 0.1).astype(np.int32)
    strata = (np.arange(nc + nt) % 2).astype(np.int32)
    paths = ["G1 (+) -> G2 (-) -> G3 (+)", "G4 (+) -> G5 (+)", "G6 (-)", ["G7", "G8", "G9", "G10"], "G1 (+) -> NA (+)", "G11 (+)"]
    for signed in (False, True):
        method = 2 if signed else 1
        base = report.score_paths(paths, genes, data, nc, nt, signed=signed, threshold=1.0, n_permutations=64, strata=strata, seed=5)
        same = report.score_paths(paths, genes, data, nc, nt, signed=signed, threshold=1.0, n_permutations=64, strata=strata, seed=5, sequential=0)
        assert list(base.columns) == report.SCORE_PATHS_COLUMNS and base.equals(same)
        got = report.score_paths(paths, genes, data, nc, nt, signed=signed, threshold=1.0, n_permutations=64, strata=strata, seed=5, sequential=2000,
                                 sequential_hits=4)
        assert list(got.columns) == report.SCORE_PATHS_COLUMNS + report.SEQUENTIAL_COLUMNS
        assert got[report.SCORE_PATHS_COLUMNS].equals(base)
        g2, d2 = report.preprocess_table(genes, data, 1.0, nc, nt)
        _, rows, signs = report.parse_sets(paths, g2)
        masks = report.permutation_masks(nc, nt, 2000, 5, strata)
        obs, null, valid = reference_null(method, rows, signs, d2, nc, api.values_table(nc, nt), masks)
        want = report.sequential_columns(report.sequential_reference(null, obs, valid, 4, 2000), valid)
        for k in report.SEQUENTIAL_COLUMNS:
            np.testing.assert_array_equal(got[k].to_numpy(), want[k], err_msg=k)
        assert np.isnan(got["SequentialPvalues"][4]) and (got["SequentialPerms"][[0, 1, 2, 3, 5]] > 0).all()


def test_launch_counter_and_refusals():
    nc, nt = 33, 31
    rows, sets, signs, strata = make_input(1, nc, nt, 3)
    ex = open_context(1, nc, nt, api.values_table(nc, nt))
    try:
        assert ex.sequential_launches() == 0
        rec, seq = ex.sequential_tests(sets, rows, signs, hits=5, max_perms=0, seed=1, strata=strata)
        assert ex.sequential_launches() == 0
        valid = rec["valid"] != 0
        assert (seq["n_hit"][valid] == 0).all() and (seq["n_perm"][valid] == 0).all() and not seq["stopped"].any()
        assert (seq["n_hit"][~valid] == -1).all() and (seq["n_perm"][~valid] == -1).all()
        others = other_counters(ex)
        bad = strata.copy()
        bad[5] = 3
        refusals = [(dict(hits=0), "hits = 0 outside 1 .. 2147483647"), (dict(hits=2**31), "hits = 2147483648 outside"),
                    (dict(max_perms=-1), "max_perms = -1 outside 0 .. 1099511627776"),
                    (dict(max_perms=2**40 + 1), "max_perms = 1099511627777 outside")]
        for kw, msg in refusals:
            with pytest.raises(api.GcreError, match="score_sets_sequential: " + msg):
                ex.sequential_tests(sets, rows, signs, **{**dict(hits=5, max_perms=100, strata=strata), **kw})
        lib = api._feature_lib("sequential")
        inp, keep = api._set_input(sets, rows, signs, nc + nt)
        out = np.zeros(len(sets), api.SET_SCORE)
        seq = np.zeros(len(sets), api.SEQ_SCORE)
        n_out = api.ctypes.c_int64(0)
        ptr = api._ptr

        def call(st, n_strata, seq_out):
            return lib.gcre_score_sets_sequential(ex._h, api.ctypes.byref(inp), 1, ptr(st), n_strata, 5, 100, ptr(out), len(out),
                                                  api.ctypes.byref(n_out), ptr(seq_out) if seq_out is not None else None)

        assert call(strata, 3, None) == -4 and b"NULL argument (seq_out)" in lib.gcre_last_error(ex._h)
        assert call(strata, 0, seq) == -4 and b"score_sets_sequential: bad strata" in lib.gcre_last_error(ex._h)
        assert call(bad, 3, seq) == -2 and b"score_sets_sequential: stratum id out of range" in lib.gcre_last_error(ex._h)
        assert call(strata, 2, seq) == -2
        with pytest.raises(api.GcreError, match="member row"):
            ex.sequential_tests([[N_ROWS]], rows, None, hits=5, max_perms=100)
        assert ex.sequential_launches() == 0 and other_counters(ex) == others
        assert call(strata, 3, seq) == 0 and ex.sequential_launches() == 3
    finally:
        ex.close()


# ---- a seeded fuzz -----------------------------------------------------------------------------------------------------


def fuzz_case(i):
    """Case i of the fuzz: the input, the call and what the definition gives -- or the mismatch, as a string."""
    rng = np.random.default_rng([7700, i])
    method = int(rng.integers(1, 3))
    n = int(rng.integers(2, 301))
    nc = int(rng.integers(1, n))
    nt = n - nc
    ns = int(rng.integers(1, 5))
    strata = None if ns == 1 else rng.integers(0, ns, n).astype(np.int32)
    n_rows = int(rng.integers(1, 40))
    rows = (rng.random((n_rows, n)) < rng.uniform(0.0, 0.6, size=(n_rows, 1))).astype(np.int8)
    rows[:, :nc] |= (rng.random((n_rows, nc)) < rng.uniform(0.0, 0.3)).astype(np.int8)
    S = int(rng.integers(1, 61))
    sets = [rng.integers(0, n_rows, int(rng.integers(1, 6))).tolist() for _ in range(S)]
    if rng.random() < 0.3:
        sets[int(rng.integers(0, S))][0] = -1
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    h = int(rng.integers(1, 31))
    max_perms = int(rng.integers(0, 5001))
    cap = int(rng.choice([0, 1, 512, 700, 1024, 2048, 4096]))
    seed = int(rng.integers(0, 2**63))
    VT = api.values_table(nc, nt)
    if rng.random() < 0.3:
        VT = VT[:int(rng.integers(1, nc + 2)), :int(rng.integers(1, nt + 2))].copy()      # cells the table lacks read as -1
    masks = report.permutation_masks(nc, nt, max_perms, seed, strata)
    obs, null, valid = reference_null(method, sets, signs, rows, nc, VT, masks)
    ref = report.sequential_reference(null, obs, valid, h, max_perms)
    if cap:
        os.environ["GCRE_SEQ_BATCH_PERMS"] = str(cap)
    else:
        os.environ.pop("GCRE_SEQ_BATCH_PERMS", None)
    ex = open_context(method, nc, nt, VT)
    try:
        rec, seq = ex.sequential_tests(sets, rows, signs, hits=h, max_perms=max_perms, seed=seed, strata=strata)
    finally:
        ex.close()
        os.environ.pop("GCRE_SEQ_BATCH_PERMS", None)
    what = f"case {i}: method {method}, {nc}+{nt} patients, {ns} strata, {S} sets, h={h}, max_perms={max_perms}, cap={cap}"
    for k in ("n_hit", "n_perm", "stopped"):
        if not np.array_equal(seq[k], ref[k]):
            return what, f"{k}: sets {np.flatnonzero(seq[k] != ref[k]).tolist()[:8]}", ref
    return what, None, ref


def test_fuzz_against_the_definition():
    """GCRE_SEQ_FUZZ_CASES seeded cases (default 16, a few seconds): random cohorts of 2-300 patients, 1-4 strata, 1-60 sets,
    1-30 hits, 0-5,000 permutations, a random batch cap, both methods."""
    cases = int(os.environ.get("GCRE_SEQ_FUZZ_CASES", "16"))
    stopped = total = 0
    for i in range(cases):
        what, bad, ref = fuzz_case(i)
        assert bad is None, f"{what}: {bad}"
        stopped += int(ref["stopped"].sum())
        total += int((ref["n_hit"] >= 0).sum())
    print(f"sequential fuzz: {cases} cases, {total} valid sets, {stopped} stopped, every count equal")
    assert cases == 0 or 0 < stopped
