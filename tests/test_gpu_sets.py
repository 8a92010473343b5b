"""Set scoring on the device (gcre_score_sets / k_set_null): bit for bit against the numpy restatement of
tests/test_sets_host.py, every level of a join passed as one family against that level's null maxima, the report front
end against gwaspa's own table, and the argument errors."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import oracle
from geneticscre_amd import api, report, synth
from helpers import small_table
from test_sets_host import restate

pytestmark = pytest.mark.gpu

FIELDS = ["valid", "cases", "ctrls", "cases_pos", "ctrls_pos", "cases_neg", "ctrls_neg", "n_ge"]


def device_masks(ex, K, n):
    """bool [K][n]: the context's permutation masks read back."""
    if K == 0:
        return np.zeros((0, n), bool)
    w = np.stack([ex.perm_mask(r) for r in range(K)])
    return np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def random_sets(rng, n_rows, S):
    """Sets of 1-12 members with mixed signs, and the special cases: duplicates, a gene under both signs, NA members."""
    sets, signs = [], []
    for _ in range(S):
        L = int(rng.integers(1, 13))
        sets.append(rng.integers(0, n_rows, size=L).tolist())
        signs.append(rng.choice([-1, 1], size=L).tolist())
    sets[0], signs[0] = [3, 3, 5, 3], [1, 1, -1, 1]          # duplicates
    sets[1], signs[1] = [4, 4], [1, -1]                       # one gene under both signs
    sets[2], signs[2] = [2, -1, 7], [1, 1, -1]                # an NA member
    sets[3], signs[3] = [6], [-1]                             # a lone (-) gene
    sets[4], signs[4] = [0, 1], [1, 1]                        # the full row and the empty row
    return sets, signs


def check_against_restatement(rec, fam, want, wnull, wfam):
    for s, w in enumerate(want):
        for f in FIELDS:
            assert rec[f][s] == w[f], (s, f, rec[s], w)
        if w["valid"]:
            assert np.float64(rec["score"][s]).view(np.uint64) == np.float64(w["score"]).view(np.uint64), s
            assert rec["pvalue"][s] == w["pvalue"] or (np.isnan(w["pvalue"]) and np.isnan(rec["pvalue"][s])), s
        else:
            assert np.isnan(rec["score"][s]) and np.isnan(rec["pvalue"][s])
    np.testing.assert_array_equal(fam.view(np.uint32), wfam.view(np.uint32))


CASES = [(n, K) for n in (5, 63, 64, 65, 200, 4999) for K in (1, 63, 64, 100, 2048, 2049, 5000)]


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("n,K", CASES)
def test_restatement_bit_for_bit(method, n, K):
    """Scores, every count, n_ge, p-values and family_max equal the restatement's; each set's own null vector, read as
    family_max of a one-set family, equals its restated one.  Masks from the host, or drawn on the device with or without
    strata (the three alternate over the cases)."""
    i = CASES.index((n, K))
    source = ("host", "device", "strata")[(i + method) % 3]
    rng = np.random.default_rng(1000 * method + i)
    nc = max(1, n // 2 - 1)
    nt = n - nc
    rows = (rng.random((16, n)) < rng.uniform(0.02, 0.6, size=(16, 1))).astype(np.int8)
    rows[0], rows[1] = 1, 0
    VT = small_table(n, n, i)                      # square: the signed method's (-) half reads rows by control counts
    VT[rng.random(VT.shape) < 0.05] *= -1          # negatives fold as 0 in the null, and count when the score is one
    ex = api.JoinExec(method, nc, nt, K)
    ex.set_value_table(VT)
    if source == "host":
        m = rng.random((K, n)) < 0.5
        ex.set_permuted_masks(api.pack_carriers(m, n))
    else:
        ex.generate_permutations(77 + i, (np.arange(n) * 7 % 3).astype(np.int32) if source == "strata" else None)
    masks = device_masks(ex, K, n)
    sets, signs = random_sets(rng, 16, 24)
    rec, fam = ex.score_sets(sets, rows, signs, family=True)
    want, wnull, wfam = restate(method, nc, nt, sets, rows, signs, VT, masks)
    check_against_restatement(rec, fam, want, wnull, wfam)
    for s in (0, 1, 3, 4, 5):
        _, own = ex.score_sets([sets[s]], rows, [signs[s]], family=True)
        np.testing.assert_array_equal(own.view(np.uint32), wnull[s].view(np.uint32), err_msg=f"set {s}")
    ex.close()


# ---- a level's joined paths as one family == the level's null maxima ---------------------------------------------------


def oracle_levels_kept(p):
    """oracle.process_paths with every level's joined rows kept: {L: OracleResult}."""
    ex = oracle.OracleJoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    ex.top_k = p.top_k
    ex.set_value_table(p.value_table)
    ex.set_permuted_cases(p.perm_cases)
    lv = p.levels
    parsed1, parsed2 = ex.load(p.data1), ex.load(p.data2)
    i1a, i1b = lv.data_inds["1a"], lv.data_inds["1b"]
    p1 = ex.join(lv.uids["1a"], ex.create_path_set(len(i1a)), parsed1[i1a], keep=True, order="canonical").paths_res
    out = {1: ex.join(lv.uids["1b"], ex.create_path_set(len(i1b)), parsed2[i1b], keep=True, order="canonical")}
    out[2] = ex.join(lv.uids["2"], p1, parsed1[lv.data_inds["2"]], keep=True, order="canonical")
    out[3] = ex.join(lv.uids["3"], out[2].paths_res, parsed1[lv.data_inds["3"]], keep=True, order="canonical")
    out[4] = ex.join(lv.uids["4"], out[3].paths_res, out[2].paths_res, keep=True, order="canonical")
    out[5] = ex.join(lv.uids["5"], out[3].paths_res, out[3].paths_res, keep=True, order="canonical")
    return out, ex.width


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_level_family_equals_join_null_max(method):
    """Every kept row of a level (method 2: its (+) half as a (+) member, its (-) half as a (-) member) as one family:
    family_max == the level's null_max from api.process_paths and from the oracle, bit for bit; every joined path's score,
    cases and controls == the oracle's, and the top-k entries are among them."""
    p = synth.make_problem(34, 80, 61, 70, 700, 5, method=method, top_k=9, seed=4242, table=small_table(131, 131, 8))
    got = api.process_paths(p)
    want, W = oracle_levels_kept(p)
    n = p.n_cases + p.n_ctrls
    ex = api.JoinExec(method, p.n_cases, p.n_ctrls, p.iterations)
    ex.set_value_table(p.value_table)
    ex.set_permuted_cases(p.perm_cases)
    for L in range(1, 6):
        r = want[L]
        np.testing.assert_array_equal(got[f"lst{L}"].null.view(np.uint32), r.null.view(np.uint32))
        rows = np.ascontiguousarray(r.paths_res)
        T = len(rows)
        assert T > 0, L
        bits = np.unpackbits(rows.view(np.uint8).reshape(T, -1), axis=1, bitorder="little")
        pos, neg = bits[:, :n], bits[:, 64 * W:64 * W + n]
        if method == "method1":
            rec, fam = ex.score_sets([[i] for i in range(T)], pos, family=True)
        else:
            rec, fam = ex.score_sets([[i, T + i] for i in range(T)], np.vstack([pos, neg]), [[1, -1]] * T, family=True)
        np.testing.assert_array_equal(fam.view(np.uint32), r.null.view(np.uint32), err_msg=f"level {L}")
        np.testing.assert_array_equal(rec["score"].view(np.uint64), r.all_scores.view(np.uint64), err_msg=f"level {L}")
        np.testing.assert_array_equal(rec["cases"], r.all_cases)
        np.testing.assert_array_equal(rec["ctrls"], r.all_ctrls)
        top = got[f"lst{L}"]
        have = set(zip(rec["score"].view(np.uint64).tolist(), rec["cases"].tolist(), rec["ctrls"].tolist()))
        for s, c, t in zip(top.scores.view(np.uint64).tolist(), top.cases.tolist(), top.ctrls.tolist()):
            assert (s, c, t) in have
    ex.close()


# ---- front end ---------------------------------------------------------------------------------------------------------


def _network_case(seed, nc=48, nt=52):
    rng = np.random.default_rng(seed)
    g, src, trg, sign = synth.signed_network(60, 200, rng)
    uid = np.arange(g) * 5 + 100
    symbols = [f"G{u}" for u in uid]
    data = (rng.random((g, nc + nt)) < 0.06).astype(np.int32)
    return symbols, data, (uid, symbols, uid[src], uid[trg], sign)


@pytest.mark.parametrize("signed", [False, True])
def test_score_paths_reproduces_gwaspa(signed):
    nc, nt, K = 48, 52, 3000
    genes, data, network = _network_case(17)
    strata = (np.arange(nc + nt) * 5 % 3).astype(np.int32)
    kw = dict(signed=signed, threshold=0.2, n_permutations=K, strata=strata, seed=909)
    out = report.gwaspa(genes, data, nc, nt, network, top_k=6, path_length=4, **kw)
    res = out["GWASPA.Results"]
    res = res[[all(h.split(" ")[0] != "NA" for h in p.split(" -> ")) for p in res["SignedPaths"]]]
    assert len(res) == 24
    sp = report.score_paths(list(res["SignedPaths"]), genes, data, nc, nt, gwaspa_out=out, **kw)
    assert list(sp.columns) == report.SCORE_PATHS_COLUMNS
    np.testing.assert_array_equal(sp["Scores"].to_numpy().view(np.uint64), res["Scores"].to_numpy().view(np.uint64))
    np.testing.assert_array_equal(sp["Cases"].to_numpy(), res["Cases"].to_numpy())
    np.testing.assert_array_equal(sp["Controls"].to_numpy(), res["Controls"].to_numpy())
    np.testing.assert_array_equal(sp["Pvalues"].to_numpy(), res["Pvalues"].to_numpy())
    np.testing.assert_array_equal(sp["Lengths"].to_numpy(), res["Lengths"].to_numpy())
    assert (sp["FamilyPvalues"] >= sp["NominalPvalues"]).all()
    # a length-2 network path that is not in the table: its score cannot exceed the lowest listed one of its length
    prep = out["prepared"]
    listed = set(res.loc[res["Lengths"] == 2, "Paths"])
    extra = None
    for a, b, s in zip(prep.src.tolist(), prep.trg.tolist(), prep.sign.tolist()):
        path = f"{prep.ents_symbol[a]} -> {prep.ents_symbol[b]}"
        if path not in listed:
            extra = f"{prep.ents_symbol[a]} (+) -> {prep.ents_symbol[b]} {'(-)' if s == -1 else '(+)'}"
            break
    assert extra is not None
    one = report.score_paths([extra], genes, data, nc, nt, gwaspa_out=out, **kw)
    assert one["Pvalues"].iat[0] >= res.loc[res["Lengths"] == 2, "Pvalues"].max()
    # a gene set, a Paths string and an unknown symbol go through the same call
    mixed = report.score_paths([[prep.ents_symbol[0], prep.ents_symbol[1]], res["Paths"].iat[0], "NOSUCHGENE -> G100"],
                               genes, data, nc, nt, **kw)
    assert mixed["Lengths"].tolist() == [2, len(res["Paths"].iat[0].split(" -> ")), 2]
    assert np.isnan(mixed["Scores"].iat[2]) and np.isnan(mixed["Pvalues"]).all()
    # checkBestPaths: passes on the table, fails on a copy with one score one ulp up, naming that row
    ok, bad = report.check_best_paths(res, genes, data, nc, nt, signed)
    assert ok and len(bad) == 0
    moved = res.copy()
    i = moved.index[3]
    moved.loc[i, "Scores"] = np.nextafter(moved.loc[i, "Scores"], np.inf)
    ok, bad = report.check_best_paths(moved, genes, data, nc, nt, signed)
    assert not ok and bad.index.tolist() == [i]
    assert bad["CheckScores"].iat[0] == res.loc[i, "Scores"] and bad["CheckCases"].iat[0] == res.loc[i, "Cases"]


# ---- errors and edges --------------------------------------------------------------------------------------------------


def test_errors_and_edges():
    rng = np.random.default_rng(3)
    nc, nt, K = 20, 25, 5000
    n = nc + nt
    rows = (rng.random((6, n)) < 0.3).astype(np.int32)
    VT = small_table(n, n, 1)
    fresh = api.JoinExec(1, nc, nt, K)
    with pytest.raises(api.GcreError, match="value table"):
        fresh.score_sets([[0]], rows)
    fresh.set_value_table(VT)
    with pytest.raises(api.GcreError, match="permutation masks"):
        fresh.score_sets([[0]], rows)
    fresh.close()
    ex = api.JoinExec(2, nc, nt, K)
    ex.set_value_table(VT)
    ex.generate_permutations(5)
    with pytest.raises(api.GcreError, match="set 1 has no members"):
        ex.score_sets([[0], []], rows)
    with pytest.raises(api.GcreError, match="set 0: sign 0 is neither"):
        ex.score_sets([[0, 1]], rows, [[1, 0]])
    with pytest.raises(api.GcreError, match="46 columns"):
        ex.score_sets([[0]], np.zeros((3, n + 1), np.int32))
    with pytest.raises(api.GcreError, match="set 2: member row 6 out of range"):
        ex.score_sets([[0], [1], [2, 6]], rows)
    # more records than cap, through the C entry
    lib = api._sets_lib()
    off = np.array([0, 1, 2], np.int64)
    mem = np.array([0, 1], np.int32)
    packed = api.pack_carriers(rows, n)
    inp = api.gcre_set_input(2, api._ptr(off), api._ptr(mem), None, api._ptr(packed), len(packed), n)
    out = np.zeros(2, dtype=api.SET_SCORE)
    n_out = ctypes.c_int64(0)
    assert lib.gcre_score_sets(ex._h, ctypes.byref(inp), api._ptr(out), 1, ctypes.byref(n_out), None) == api.GCRE_ERR_RANGE
    assert n_out.value == 2 and b"room for 1" in ex._lib.gcre_last_error(ex._h)
    # an empty family: no records, family_max all zeros
    rec, fam = ex.score_sets([], rows, family=True)
    assert len(rec) == 0 and fam.shape == (K,) and not fam.any()
    # a permutation window on the context changes nothing
    sets = [[0, 1], [2], [3, 4, 5]]
    signs = [[1, -1], [-1], [1, 1, -1]]
    a, fa = ex.score_sets(sets, rows, signs, family=True)
    ex.set_perm_window(2048, 4096)
    b, fb = ex.score_sets(sets, rows, signs, family=True)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(fa.view(np.uint32), fb.view(np.uint32))
    ex.close()
    # K = 0: NaN p-values, no family
    ex0 = api.JoinExec(1, nc, nt, 0)
    ex0.set_value_table(VT)
    rec, fam = ex0.score_sets(sets, rows, family=True)
    assert np.isnan(rec["pvalue"]).all() and (rec["n_ge"] == 0).all() and len(fam) == 0
    assert (rec["valid"] == 1).all() and not np.isnan(rec["score"]).any()
    ex0.close()
