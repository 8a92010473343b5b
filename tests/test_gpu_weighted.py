"""Covariate-adjusted permutation masks on the device (gcre_generate_weighted_masks: k_weighted_search, k_weighted_write;
DESIGN.md §3.23).  Every mask, read back with gcre_get_perm_mask, and every accepted attempt is compared bit for bit against
``report.weighted_masks`` on the library's own thresholds.  The shapes are the smallest at which each part can go wrong: one
patient per group, the dword that straddles n_cases, a stratum boundary inside a dword, sixteen strata, a stratum without a
case and one that is all cases, permutation counts around a wave of k_weighted_write and around a block of k_weighted_search,
patients at odds 0 and one patient with almost all the weight.  Then the cap, the refusals, and what reads the masks
afterwards: set scores, stratified set scores, the joins of ``gwaspa`` and ``score_paths``."""
from __future__ import annotations

import os

import numpy as np
import pytest

from geneticscre_amd import api, report, synth
from helpers import small_table
from test_sets_host import restate

pytestmark = pytest.mark.gpu

OK, ERR_RANGE, ERR_ARG = 0, -2, -4   # include/gcre_hip.h
G = "generate_weighted_masks: "


def device_words(ex, K):
    return np.stack([ex.perm_mask(r) for r in range(K)]) if K else np.zeros((0, ex.width_ul), np.uint64)


def unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little").astype(bool)


def draw_and_compare(ex, nc, nt, K, seed, odds, strata=None, what=""):
    """One call against the numpy definition: (masks bool [K][n], attempts)."""
    n = nc + nt
    thr, exp = api.weighted_thresholds(odds, nc, nt, strata)
    want, watt = report.weighted_masks(thr, nc, nt, K, seed, strata)
    before = ex.weighted_launches()
    att = ex.generate_weighted_permutations(seed, odds, strata, attempts=True)
    assert ex.weighted_launches() == before + 2
    bits = unpack(device_words(ex, K), n)
    assert att.dtype == np.uint32 and att.shape == watt.shape
    np.testing.assert_array_equal(att, watt, err_msg=f"{what} attempts")
    np.testing.assert_array_equal(bits[:, :n], want, err_msg=f"{what} masks")
    assert not bits[:, n:].any(), f"{what}: bits beyond the patients"
    # the law's support: every stratum keeps its cases; odds 0 is never a case
    st = np.zeros(n, int) if strata is None else np.asarray(strata)
    for s in np.unique(st):
        assert (want[:, st == s].sum(axis=1) == (st[:nc] == s).sum()).all()
    assert not want[:, np.asarray(odds) == 0].any()
    print(what, "mean attempt", att.mean(axis=0), "max", att.max(axis=0), "sqrt(2 pi V)", exp)
    return want, att


def odds_pattern(kind, rng, nc, nt):
    n = nc + nt
    if kind == "equal":
        return np.ones(n)
    if kind == "log-uniform":
        return 10.0 ** rng.uniform(-6, 6, n)
    if kind == "zeros":                        # as many as the controls allow, a fifth of the cohort at the most
        o = rng.uniform(0.5, 2.0, n)
        o[rng.permutation(n)[:min(nt, max(1, n // 5))]] = 0.0
        return o
    if kind == "heavy":                        # one patient carries almost all the weight
        o = np.ones(n)
        o[int(rng.integers(0, n))] = 1e9
        return o
    raise ValueError(kind)


COHORTS = [(1, 1), (31, 2), (32, 32), (33, 31), (65, 135)]
PATTERNS = ["equal", "log-uniform", "zeros", "heavy"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nc,nt", COHORTS)
def test_cohorts_and_odds(nc, nt, pattern):
    rng = np.random.default_rng([nc, nt, PATTERNS.index(pattern)])
    ex = api.JoinExec(1, nc, nt, 130)
    draw_and_compare(ex, nc, nt, 130, 40 + nc, odds_pattern(pattern, rng, nc, nt), None, f"{nc}+{nt} {pattern}")
    ex.close()


def layouts(nc, nt):
    n = nc + nt
    q = np.arange(n)
    three = np.concatenate([np.arange(nc) % 2, np.arange(nt) % 3])            # stratum 2 holds controls only
    all_cases = np.where(q < 5, 4, q % 2 * 9)                                  # stratum 4: five patients, all of them cases
    inside = (q >= 13).astype(int) + (q >= 45)                                 # boundaries at patients 13 and 45: inside dwords 0 and 1
    return [("one", None), ("two interleaved", q % 2), ("three, one without a case", three), ("one that is all cases", all_cases),
            ("a boundary inside a dword", inside), ("sixteen", (q * 7) % 16 - 5)]


@pytest.mark.parametrize("name", [x[0] for x in layouts(2, 2)])
def test_strata(name):
    nc, nt, K = 65, 135, 130
    strata = dict(layouts(nc, nt))[name]
    rng = np.random.default_rng(len(name))
    ex = api.JoinExec(2, nc, nt, K)
    for pattern in ("log-uniform", "equal"):
        odds = odds_pattern(pattern, rng, nc, nt)
        if pattern == "log-uniform":
            odds[::17] = 0.0
            odds[:nc] = np.maximum(odds[:nc], 1e-6)       # (every case keeps a positive odds: enough of them in every stratum)
        draw_and_compare(ex, nc, nt, K, 9, odds, strata, f"{name} {pattern}")
    ex.close()


@pytest.mark.parametrize("K", [1, 63, 64, 65, 513, 1025])
def test_permutation_counts(K):
    nc, nt = 33, 31
    rng = np.random.default_rng(K)
    ex = api.JoinExec(1, nc, nt, K)
    draw_and_compare(ex, nc, nt, K, 1000 + K, np.exp(rng.normal(0, 1.5, nc + nt)), np.arange(nc + nt) % 3, f"K = {K}")
    ex.close()


def test_seeds_and_repeats():
    nc, nt, K = 20, 30, 100
    odds = np.exp(np.random.default_rng(3).normal(0, 1, nc + nt))
    ex = api.JoinExec(1, nc, nt, K)
    assert ex.generate_weighted_permutations(5, odds) is None
    a = device_words(ex, K)
    ex.generate_weighted_permutations(6, odds)
    b = device_words(ex, K)
    ex.generate_weighted_permutations(5, odds)
    c = device_words(ex, K)
    assert np.array_equal(a, c) and not np.array_equal(a, b)
    assert (a != b).any(axis=1).mean() > 0.9            # nearly every permutation differs
    # another context, another order of calls: the same masks
    ex2 = api.JoinExec(2, nc, nt, K)
    ex2.generate_permutations(1)
    ex2.generate_weighted_permutations(5, odds)
    assert np.array_equal(device_words(ex2, K), a)
    # not the bits of the uniform generator, even with equal odds
    ex2.generate_permutations(5)
    u = device_words(ex2, K)
    ex2.generate_weighted_permutations(5, np.ones(nc + nt))
    assert not np.array_equal(device_words(ex2, K), u)
    ex.close()
    ex2.close()


def test_no_permutations():
    ex = api.JoinExec(1, 4, 5, 0)
    att = ex.generate_weighted_permutations(1, np.ones(9), attempts=True)
    assert att.shape == (0, 1) and ex.weighted_launches() == 0
    with pytest.raises(api.GcreError, match="must be finite and >= 0"):      # the arguments are still checked
        ex.generate_weighted_permutations(1, -np.ones(9))
    ex.close()


# ---- the cap ----------------------------------------------------------------------------------------------------------------


def c_call(ex, seed, odds, stratum, n_strata, max_attempts, att=None):
    lib = api._weighted_lib()
    w = None if odds is None else np.ascontiguousarray(odds, dtype=np.float64)
    st = None if stratum is None else np.ascontiguousarray(stratum, dtype=np.int32)
    rc = lib.gcre_generate_weighted_masks(ex._h, seed, api._ptr(w), api._ptr(st), n_strata, max_attempts, api._ptr(att))
    return rc, (lib.gcre_last_error(ex._h).decode() if rc else "")


def test_max_attempts():
    nc, nt, K, seed = 3, 3, 40, 12
    odds = np.array([1 / 3, 1, 3, 1, 1, 1])
    thr, exp = api.weighted_thresholds(odds, nc, nt)
    want, watt = report.weighted_masks(thr, nc, nt, K, seed)
    assert watt.max() >= 3 and exp[0] <= 3                         # chosen on the CPU: some permutation needs a fourth attempt
    left = int((watt[:, 0] >= 3).sum())
    ex = api.JoinExec(1, nc, nt, K)
    ex.generate_permutations(5)
    before = device_words(ex, K)
    att = np.full((K, 1), 77, np.uint32)
    rc, msg = c_call(ex, seed, odds, None, 0, 3, att)
    assert rc == ERR_RANGE
    assert msg == G + f"{left} of {K} permutations were left over without an accepted attempt below max_attempts = 3: the context's masks are unchanged"
    assert ex.weighted_launches() == 1                             # the search alone: no mask bit was written
    assert np.array_equal(device_words(ex, K), before) and (att == 77).all()
    with pytest.raises(api.GcreError, match=f"{left} of {K} permutations were left over"):
        ex.generate_weighted_permutations(seed, odds, max_attempts=3)
    assert np.array_equal(device_words(ex, K), before)
    # the reference under the same cap names the same permutations
    _, capped = report.weighted_masks(thr, nc, nt, K, seed, max_attempts=3)
    assert ((capped[:, 0] == report.WEIGHTED_NONE) == (watt[:, 0] >= 3)).all()
    # one more than the largest accepted attempt is enough
    got = ex.generate_weighted_permutations(seed, odds, max_attempts=int(watt.max()) + 1, attempts=True)
    assert np.array_equal(got, watt) and np.array_equal(unpack(device_words(ex, K), 6)[:, :6], want)
    rc, msg = c_call(ex, seed, odds, None, 0, int(watt.max()))
    assert rc == ERR_RANGE and msg.startswith(G + f"{int((watt == watt.max()).sum())} of {K} permutations were left over")
    ex.close()


REFUSALS = [
    ("NULL odds", None, None, 0, 1 << 20, ERR_ARG, "NULL argument (odds)"),
    ("negative odds", [1, 1, -2, 1, 1, 1], None, 0, 1 << 20, ERR_ARG, "the odds of patient 2 (stratum 0) must be finite and >= 0, not -2.000000"),
    ("NaN odds", [1, 1, 1, 1, np.nan, 1], [0, 0, 1, 1, 1, 0], 2, 1 << 20, ERR_ARG, "the odds of patient 4 (stratum 1) must be finite and >= 0, not nan"),
    ("infinite odds", [np.inf, 1, 1, 1, 1, 1], None, 0, 1 << 20, ERR_ARG, "the odds of patient 0 (stratum 0) must be finite and >= 0, not inf"),
    ("too few positive odds", [1, 0, 0, 1, 1, 1], [1, 1, 1, 0, 0, 1], 2, 1 << 20, ERR_ARG,
     "stratum 1 has 2 patients with positive odds, fewer than its 3 cases"),
    ("a stratum id out of range", [1] * 6, [0, 1, 2, 0, 1, 0], 2, 1 << 20, ERR_ARG, "stratum id 2 of patient 2 outside 0 .. 1"),
    ("seventeen strata", [1] * 6, [0] * 6, 17, 1 << 20, ERR_ARG, "n_strata = 17 outside 1 .. GCRE_STRATA_MAX = 16"),
    ("max_attempts 0", [1] * 6, None, 0, 0, ERR_ARG, "max_attempts = 0 must be at least 1"),
    ("the estimate alone above the cap", [1] * 6, None, 0, 2, ERR_RANGE, "stratum 0 needs about 4 attempts per permutation, above max_attempts = 2"),
]


@pytest.mark.parametrize("name,odds,stratum,ns,cap,code,message", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_up_front_refusals_launch_nothing(name, odds, stratum, ns, cap, code, message):
    K = 10
    ex = api.JoinExec(1, 3, 3, K)
    ex.generate_permutations(2)
    before = device_words(ex, K)
    rc, msg = c_call(ex, 1, odds, stratum, ns, cap)
    assert (rc, msg) == (code, G + message)
    assert ex.weighted_launches() == 0 and np.array_equal(device_words(ex, K), before)
    ex.close()
    assert api._weighted_lib().gcre_generate_weighted_masks(None, 1, None, None, 0, 1, None) == ERR_ARG


# ---- what reads the masks ---------------------------------------------------------------------------------------------------


def confounded(rng, nc, nt):
    """A covariate that shifts the case fraction, the fitted odds, and two strata."""
    n = nc + nt
    cov = np.r_[rng.normal(0.6, 1, nc), rng.normal(-0.3, 1, nt)]
    return report.case_odds(cov, nc, nt), (np.arange(n) * 3 % 2) * 5


@pytest.mark.parametrize("method", [1, 2])
def test_set_scores_count_over_the_weighted_masks(method):
    nc, nt, K = 37, 45, 700
    rng = np.random.default_rng(method)
    odds, strata = confounded(rng, nc, nt)
    rows = (rng.random((12, nc + nt)) < rng.uniform(0.05, 0.5, size=(12, 1))).astype(np.int8)
    sets = [rng.integers(0, 12, int(rng.integers(1, 5))).tolist() for _ in range(9)]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    VT = small_table(nc + nt, nc + nt, 5)
    ex = api.JoinExec(method, nc, nt, K)
    ex.set_value_table(VT)
    masks, _ = draw_and_compare(ex, nc, nt, K, 21, odds, strata)
    rec, fam = ex.score_sets(sets, rows, signs, family=True)
    want, _, wfam = restate(method, nc, nt, sets, rows, signs, VT, masks)
    assert rec["n_ge"].tolist() == [w["n_ge"] for w in want]
    np.testing.assert_array_equal(fam.view(np.uint32), wfam.view(np.uint32))
    # the stratified scores accept the context: its masks keep these strata (the mask check of the stratified stage) ...
    tables = [small_table(int((strata[:nc] == i).sum()), int((strata[nc:] == i).sum()), 3) for i in np.unique(strata)]
    _, sr = ex.strata_tests(sets, rows, signs, strata=strata, tables=tables)
    ref = report.strata_reference(sets, rows, signs, nc, strata, tables, masks, method)
    assert sr["n_ge"].tolist() == ref["n_ge"].tolist()
    # ... and refuse it once the masks were drawn without them
    ex.generate_weighted_permutations(21, odds)
    with pytest.raises(api.GcreError, match="do not keep the cases of the stratum"):
        ex.strata_tests(sets, rows, signs, strata=strata, tables=tables)
    ex.close()


def _network_case(seed, nc=48, nt=52):      # the small problem of test_gpu_genes.py
    rng = np.random.default_rng(seed)
    g, src, trg, sign = synth.signed_network(60, 200, rng)
    uid = np.arange(g) * 5 + 100
    symbols = [f"G{u}" for u in uid]
    data = (rng.random((g, nc + nt)) < 0.06).astype(np.int32)
    return symbols, data, (uid, symbols, uid[src], uid[trg], sign)


def upload_reference(monkeypatch, nc, nt, K):
    """``gwaspa`` / ``score_paths`` with the masks of the numpy definitions uploaded instead of drawn on the device."""
    def draw(ex, seed, strata, case_odds):
        if case_odds is None:
            m = report.permutation_masks(nc, nt, K, seed, strata)
        else:
            thr, _ = api.weighted_thresholds(case_odds, nc, nt, strata)
            m, _ = report.weighted_masks(thr, nc, nt, K, seed, strata)
        ex.set_permuted_masks(api.pack_carriers(m, nc + nt))
    monkeypatch.setattr(report, "_draw_permutations", draw)


def same_levels(a, b, L):
    for i in range(1, L + 1):
        x, y = a["levels"][f"lst{i}"], b["levels"][f"lst{i}"]
        np.testing.assert_array_equal(x.null.view(np.uint32), y.null.view(np.uint32), err_msg=f"null maxima of level {i}")
        np.testing.assert_array_equal(x.scores.view(np.uint64), y.scores.view(np.uint64))


@pytest.mark.parametrize("signed", [False, True])
def test_gwaspa_and_score_paths(signed, monkeypatch):
    nc, nt, K, L = 48, 52, 600, 3
    genes, data, network = _network_case(17)
    rng = np.random.default_rng(2)
    odds, strata = confounded(rng, nc, nt)
    kw = dict(signed=signed, threshold=0.2, n_permutations=K, strata=strata, seed=909, top_k=6, path_length=L)
    plain = report.gwaspa(genes, data, nc, nt, network, **kw)
    plain_none = report.gwaspa(genes, data, nc, nt, network, case_odds=None, **kw)
    adjusted = report.gwaspa(genes, data, nc, nt, network, case_odds=odds, **kw)
    assert set(plain) == set(plain_none) == {"GWASPA.Results", "levels", "prepared"}       # the default output is what it was
    assert set(adjusted) == set(plain) | {"case_odds_digest"}
    assert plain_none["GWASPA.Results"].equals(plain["GWASPA.Results"])
    # the joins' null maxima moved, the observed scores did not: the adjustment is on the null
    for i in range(1, L + 1):          # (the table's rows are ordered by p-value: compare the levels)
        np.testing.assert_array_equal(adjusted["levels"][f"lst{i}"].scores.view(np.uint64), plain["levels"][f"lst{i}"].scores.view(np.uint64))
    assert any(not np.array_equal(adjusted["levels"][f"lst{i}"].null, plain["levels"][f"lst{i}"].null) for i in range(1, L + 1))
    res = plain["GWASPA.Results"]
    res = res[[all(h.split(" ")[0] != "NA" for h in p.split(" -> ")) for p in res["SignedPaths"]]]
    prep = plain["prepared"]
    paths = list(res["SignedPaths"]) + [prep.ents_symbol[0], [prep.ents_symbol[1], prep.ents_symbol[2]]]
    skw = dict(signed=signed, threshold=0.2, n_permutations=K, strata=strata, seed=909)
    sp_plain = report.score_paths(paths, genes, data, nc, nt, gwaspa_out=plain, stratified=True, **skw)
    sp_none = report.score_paths(paths, genes, data, nc, nt, gwaspa_out=plain, stratified=True, case_odds=None, **skw)
    sp_adj = report.score_paths(paths, genes, data, nc, nt, gwaspa_out=adjusted, stratified=True, case_odds=odds, **skw)
    assert sp_none.equals(sp_plain)
    with pytest.raises(ValueError, match="gwaspa_out was drawn under different case_odds"):
        report.score_paths(paths, genes, data, nc, nt, gwaspa_out=adjusted, **skw)
    with pytest.raises(ValueError, match="gwaspa_out was drawn under different case_odds"):
        report.score_paths(paths, genes, data, nc, nt, gwaspa_out=plain, case_odds=odds, **skw)
    # the same calls on the uploaded masks of the numpy definitions
    upload_reference(monkeypatch, nc, nt, K)
    ref_plain = report.gwaspa(genes, data, nc, nt, network, **kw)
    ref_adjusted = report.gwaspa(genes, data, nc, nt, network, case_odds=odds, **kw)
    assert ref_plain["GWASPA.Results"].equals(plain["GWASPA.Results"])
    assert ref_adjusted["GWASPA.Results"].equals(adjusted["GWASPA.Results"])
    same_levels(ref_plain, plain, L)
    same_levels(ref_adjusted, adjusted, L)
    assert report.score_paths(paths, genes, data, nc, nt, gwaspa_out=ref_plain, stratified=True, **skw).equals(sp_plain)
    assert report.score_paths(paths, genes, data, nc, nt, gwaspa_out=ref_adjusted, stratified=True, case_odds=odds, **skw).equals(sp_adj)


# ---- fuzz -------------------------------------------------------------------------------------------------------------------


def test_fuzz():
    cases = int(os.environ.get("GCRE_WEIGHTED_FUZZ_CASES", "12"))
    for case in range(cases):
        rng = np.random.default_rng([2300, case])
        nc, nt = int(rng.integers(1, 90)), int(rng.integers(1, 90))
        n = nc + nt
        K = int(rng.choice([1, 7, 64, 200, 513]))
        ns = int(rng.choice([0, 1, 2, 5, 16]))
        strata = None if ns == 0 else rng.integers(0, ns, n) * 3 - 7
        odds = odds_pattern(PATTERNS[case % 4], rng, nc, nt)
        if strata is not None:
            odds[:nc] = np.where(odds[:nc] > 0, odds[:nc], 1.0)             # every stratum keeps enough positive odds
        ex = api.JoinExec(1 + case % 2, nc, nt, K)
        draw_and_compare(ex, nc, nt, K, int(rng.integers(0, 2**63)), odds, strata, f"case {case}")
        ex.close()
