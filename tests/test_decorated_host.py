"""Decorated p-values, host side: gcre_decorated_splits against a literal transcription of R/DecoratedPvalue.R, a
hand-worked example, and the shape of report.decorated_table.  No GPU needed."""
from __future__ import annotations

import warnings

import numpy as np
import pandas as pd
import pytest

from geneticscre_amd import api, report
from helpers import small_table

FIELDS = ["cases1", "ctrls1", "cases2", "ctrls2", "case_pos1", "ctrl_pos1", "case_neg1", "ctrl_neg1",
          "case_pos2", "ctrl_pos2", "case_neg2", "ctrl_neg2", "k_pos", "pop_pos", "succ_pos", "k_neg", "pop_neg",
          "succ_neg"]


# ---- R/DecoratedPvalue.R, transcribed -------------------------------------------------------------------------------
# 0-based patient indices where R has 1-based ones; which() / setdiff() / intersect() as numpy set operations.  The value
# table is read as the device reads it (-1 past its edge: INTEGRATION.md deviation 4).


def r_compute_decorated(sp1, sn1, sp2, sn2, n_cases, n_ctrls, method, VT, strata):
    """computeDecoratedPvalue (:198-304) up to the permutation loop: counts, observed score and what the loop samples."""
    def vt(a, b):
        return float(VT[a, b]) if a < VT.shape[0] and b < VT.shape[1] else -1.0
    n = n_cases + n_ctrls
    inds_pos1, inds_neg1 = np.flatnonzero(sp1 != 0), np.flatnonzero(sn1 != 0)
    inds_pos2, inds_neg2 = np.flatnonzero(sp2 != 0), np.flatnonzero(sn2 != 0)
    sp2, sn2 = sp2.copy(), sn2.copy()
    sp2[np.intersect1d(inds_pos1, inds_pos2)] = 0
    sn2[np.intersect1d(inds_neg1, inds_neg2)] = 0
    inds_pos2 = np.setdiff1d(inds_pos2, inds_pos1)
    inds_neg2 = np.setdiff1d(inds_neg2, inds_neg1)
    C, T = slice(0, n_cases), slice(n_cases, n)
    o = dict(case_pos1=int(sp1[C].sum()), case_neg1=int(sn1[T].sum()), ctrl_pos1=int(sp1[T].sum()),
             ctrl_neg1=int(sn1[C].sum()), case_pos2=int(sp2[C].sum()), case_neg2=int(sn2[T].sum()),
             ctrl_pos2=int(sp2[T].sum()), ctrl_neg2=int(sn2[C].sum()))
    if method == 1:
        o["score"] = vt(o["case_pos1"] + o["case_pos2"] + o["case_neg1"] + o["case_neg2"],
                        o["ctrl_pos1"] + o["ctrl_pos2"] + o["ctrl_neg1"] + o["ctrl_neg2"])
    else:
        o["score"] = (vt(o["case_pos1"] + o["case_pos2"], o["ctrl_pos1"] + o["ctrl_pos2"]) +
                      vt(o["case_neg1"] + o["case_neg2"], o["ctrl_neg1"] + o["ctrl_neg2"]))
    o["cases1"], o["ctrls1"] = o["case_pos1"] + o["case_neg1"], o["ctrl_pos1"] + o["ctrl_neg1"]
    o["cases2"], o["ctrls2"] = o["case_pos2"] + o["case_neg2"], o["ctrl_pos2"] + o["ctrl_neg2"]
    to_sample_pos = np.setdiff1d(np.arange(n), inds_pos1)
    to_sample_neg = np.setdiff1d(np.arange(n), inds_neg1)
    if strata is None:
        # sample(toSample_pos, length(inds_pos2)): cases are successes; the neg draw counts controls
        o.update(k_pos=len(inds_pos2), pop_pos=len(to_sample_pos), succ_pos=int((to_sample_pos < n_cases).sum()),
                 k_neg=len(inds_neg2), pop_neg=len(to_sample_neg), succ_neg=int((to_sample_neg >= n_cases).sum()))
        o["strata"] = None
    else:
        inds_1 = np.union1d(inds_pos1, inds_neg1)
        st = []
        for s in range(int(strata.max()) + 1):
            group = np.setdiff1d(np.flatnonzero(strata == s), inds_1)
            st.append((len(group), int((group < n_cases).sum()), int(np.isin(inds_pos2, group).sum()),
                       int(np.isin(inds_neg2, group).sum())))
        o["strata"] = st
        o.update(k_pos=sum(x[2] for x in st), pop_pos=0, succ_pos=0, k_neg=sum(x[3] for x in st), pop_neg=0, succ_neg=0)
    return o


def r_decorated_splits(data, paths, signs, n_cases, n_ctrls, method, VT, strata=None):
    """getDecoratedPvalues (:48-193): the splits of every path, Forward j = 1..L-1 then Backward j = L..2."""
    out = []
    for p, (rows, sg) in enumerate(zip(paths, signs)):
        L = len(rows)
        if L < 2:
            continue
        if any(r < 0 for r in rows):
            for d, js in ((0, range(1, L)), (1, range(L, 1, -1))):
                out += [dict(path=p, direction=d, j=j, valid=0) for j in js]
            continue
        pos = data[rows].astype(np.int64)
        neg = np.zeros_like(pos)
        if method == 2:
            m = np.asarray(sg) == -1
            neg[m] = pos[m]
            pos[m] = 0
        for j in range(1, L):
            sp1, sn1 = (pos[:j].sum(0) != 0).astype(np.int64), (neg[:j].sum(0) != 0).astype(np.int64)
            o = r_compute_decorated(sp1, sn1, pos[j], neg[j], n_cases, n_ctrls, method, VT, strata)
            out.append(dict(o, path=p, direction=0, j=j, valid=1))
        for j in range(L, 1, -1):
            sp1 = (pos[j - 1:L].sum(0) != 0).astype(np.int64)
            sn1 = (neg[j - 1:L].sum(0) != 0).astype(np.int64)
            o = r_compute_decorated(sp1, sn1, pos[j - 2], neg[j - 2], n_cases, n_ctrls, method, VT, strata)
            out.append(dict(o, path=p, direction=1, j=j, valid=1))
    return out


def random_case(seed, method):
    rng = np.random.default_rng(seed)
    nc, nt = int(rng.integers(20, 90)), int(rng.integers(20, 90))
    n = nc + nt
    G = 14
    data = (rng.random((G, n)) < rng.uniform(0.03, 0.3, size=(G, 1))).astype(np.int32)
    data[3] = data[2] & (rng.random(n) < 0.5)                  # gene 3 inside gene 2: k = 0 after gene 2
    data[5] = data[4] | data[6]                                # gene 5 covers 4 and 6
    paths, signs = [[2, 3], [4, 5, 6], [3, 2, 7, 8]], [[1, 1], [1, -1, 1], [-1, 1, 1, -1]]
    for _ in range(10):
        L = int(rng.integers(2, 6))
        paths.append(rng.choice(G, size=L, replace=False).tolist())
        signs.append(rng.choice([-1, 1], size=L).tolist())
    paths.append([0])                                          # length 1: no split
    signs.append([1])
    return nc, nt, data, paths, signs, small_table(nc, nt, seed)


# ---- the special-value tables (tests/helpers.py) under the splits of random_case ----------------------------------------------
TABLE_KINDS = ("zeros", "nonfinite", "tiny", "huge", "ladder", "few_both")
TABLE_PERMS = 300
# (kind, method) -> (seed of random_case, seed and variant of the table): found on the CPU so that the observed values of the
# transcription alone hold what test_special_tables_hold_every_kind_of_observed_value asks
TABLE_CASES = {
    ("zeros", 1): (0, 0, 0), ("nonfinite", 1): (39, 3, 2), ("tiny", 1): (0, 0, 0), ("huge", 1): (0, 0, 0), ("ladder", 1): (0, 0, 0),
    ("few_both", 1): (0, 0, 0),
    ("zeros", 2): (0, 0, 0), ("nonfinite", 2): (0, 1, 2), ("tiny", 2): (0, 0, 0), ("huge", 2): (0, 0, 0), ("ladder", 2): (0, 0, 0),
    ("few_both", 2): (0, 0, 0),
}


def table_case(kind, method):
    """(nc, nt, data, paths, signs, VT): the splits of ``random_case`` on a table of the family ``kind``."""
    from helpers import shape_tables, special_table
    seed, tseed, variant = TABLE_CASES[(kind, method)]
    nc, nt, data, paths, signs, _ = random_case(seed, method)
    if kind == "few_both":
        VT = dict((name, tb) for name, tb, _ in shape_tables(nc, nt, tseed))["few_both"]
    else:
        VT = special_table(kind, nc, nt, tseed, variant)
    return nc, nt, data, paths, signs, VT


def table_strata(nc, nt):
    return (np.arange(nc + nt) * 7 % 3).astype(np.int32)


def observed_kinds(scores):
    """Which special values the observed scores of a list of splits hold."""
    s = np.asarray(scores, np.float64)
    tiny = float(np.finfo(np.float32).tiny)
    return {"NaN": bool(np.isnan(s).any()), "+0": bool(((s == 0) & ~np.signbit(s)).any()), "-0": bool(((s == 0) & np.signbit(s)).any()),
            "+inf": bool(np.isposinf(s).any()), "-inf": bool(np.isneginf(s).any()), "denormal": bool(((s > 0) & (s < tiny)).any()),
            "negative": bool(((s < 0) & np.isfinite(s)).any())}


def table_expectation(kind, method, stratified, seed=99):
    """What the device must return for a table case, from the transcription, the host stage and the restated sampler:
    (host records, their strata, urn counts [splits][K][2], n_ge [splits], exact ties [splits])."""
    from test_gpu_decorated import perm_scores, restated_counts
    nc, nt, data, paths, signs, VT = table_case(kind, method)
    strata = table_strata(nc, nt) if stratified else None
    host, st = api.decorated_splits(method, nc, nt, paths, data, signs, VT, strata)
    counts = restated_counts(host, st, seed, TABLE_PERMS)
    n_ge, ties = np.zeros(len(host), np.int64), np.zeros(len(host), np.int64)
    with np.errstate(invalid="ignore"):
        for s, r in enumerate(host):
            if r["valid"]:
                ps = perm_scores(r, counts[s, :, 0], counts[s, :, 1], method, VT)
                n_ge[s], ties[s] = int((ps >= r["score"]).sum()), int((ps == r["score"]).sum())
    return host, st, counts, n_ge, ties


def assert_same(got, want, strata_got=None):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (int(g["path"]), int(g["direction"]), int(g["j"]), int(g["valid"])) == \
            (w["path"], w["direction"], w["j"], w["valid"]), i
        if not w["valid"]:
            assert np.isnan(g["score"]) and np.isnan(g["pvalue"])
            assert all(int(g[f]) == 0 for f in FIELDS)
            continue
        for f in FIELDS:
            assert int(g[f]) == w[f], (i, f, int(g[f]), w[f])
        assert np.float64(g["score"]).view(np.uint64) == np.float64(w["score"]).view(np.uint64), (i, g["score"], w["score"])
        if w["strata"] is None:
            assert int(g["strata_off"]) == -1
        else:
            assert [tuple(int(v) for v in x) for x in strata_got[i]] == w["strata"], i
        assert np.isnan(g["pvalue"]) and int(g["n_ge"]) == 0       # permutations are the device's


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("stratified", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_stage_matches_r_transcription(method, stratified, seed):
    nc, nt, data, paths, signs, VT = random_case(100 * seed + method, method)
    strata = (np.random.default_rng(seed).integers(0, 4, nc + nt)).astype(np.int32) if stratified else None
    got, st = api.decorated_splits(method, nc, nt, paths, data, signs, VT, strata, iterations=10, seed=seed)
    want = r_decorated_splits(data, paths, signs, nc, nt, method, VT, strata)
    assert_same(got, want, st)
    # the planted k = 0 split: gene 3 after gene 2 (path 0, Forward j = 1) draws nothing
    assert int(got[0]["k_pos"]) == 0 and int(got[0]["k_neg"]) == 0
    if method == 2:
        # mixed signs reach the neg half, and overlap is removed only within a half
        assert (got["k_neg"] > 0).any() and (got["case_neg1"] + got["ctrl_neg1"] > 0).any()


@pytest.mark.parametrize("method", [1, 2])
def test_host_stage_at_the_cohort_limit(method):
    """n = 65,536 (R's limit): dense rows, a gene every patient carries, 64 strata (one of a single patient, one without
    cases) and a table smaller than the cohort (-1 cells), with and without strata."""
    nc, nt = 60000, 5536
    n = nc + nt
    rng = np.random.default_rng(65536 + method)
    data = (rng.random((8, n)) < rng.uniform(0.02, 0.7, (8, 1))).astype(np.int32)
    data[3] = 1
    data[6:] = rng.random((2, n)) < 0.01                        # sparse genes: splits inside the table
    paths = [[0, 1, 2], [3, 4], [5, 3, 6], [7, 0, 1, 2, 4], [6, 7]]
    signs = [[1, -1, 1], [-1, 1], [1, 1, -1], [1, -1, -1, 1, 1], [1, 1]]
    strata = rng.integers(0, 62, n).astype(np.int32)
    strata[nc + 5] = 62
    strata[nc + 100:nc + 400] = 63
    VT = small_table(6000, 3000, method)
    for st_in in (None, strata):
        got, st = api.decorated_splits(method, nc, nt, paths, data, signs, VT, st_in)
        want = r_decorated_splits(data, paths, signs, nc, nt, method, VT, st_in)
        assert_same(got, want, st)
        assert max(w["k_pos"] + w["k_neg"] for w in want) >= 10000
        assert any(w["score"] < 0 for w in want) and any(w["score"] > 0 for w in want)      # -1 cells and table cells
    assert [w["cases1"] + w["ctrls1"] for w in want if w["path"] == 1 and w["direction"] == 0] == [n]


def test_host_stage_column_major_table_and_na_genes():
    nc, nt, data, paths, signs, VT = random_case(77, 2)
    paths = paths[:4] + [[1, -1, 2]]
    signs = signs[:4] + [[1, 1, -1]]
    a, _ = api.decorated_splits(2, nc, nt, paths, data, signs, VT)
    lib = api._decorated_lib()
    d = api._DpInput(2, nc, nt, paths, data, signs, None, 0, 0)
    out = d.out()
    F = np.asfortranarray(VT)
    n_out = api.ctypes.c_int64(0)
    assert lib.gcre_decorated_splits(api.ctypes.byref(d.c), F.ctypes.data_as(api.ctypes.c_void_p), VT.shape[0],
                                     VT.shape[1], 1, api._ptr(out), len(out), api.ctypes.byref(n_out)) == 0
    np.testing.assert_array_equal(a["score"].view(np.uint64), out[:n_out.value]["score"].view(np.uint64))
    assert_same(a, r_decorated_splits(data, paths, signs, nc, nt, 2, VT))
    na = a[a["path"] == 4]
    assert len(na) == 4 and (na["valid"] == 0).all() and np.isnan(na["score"]).all()


def test_host_stage_errors():
    data = np.eye(4, 10, dtype=np.int32)
    with pytest.raises(IndexError):
        api.decorated_splits(1, 4, 6, [[0, 9]], data)           # row out of range
    with pytest.raises(ValueError):
        api.decorated_splits(1, 4, 6, [[0, 1, 2, 3, 0, 1]], data)
    lib = api._decorated_lib()
    d = api._DpInput(1, 4, 6, [[0, 1, 2]], data, None, None, 0, 0)
    out = d.out()
    n_out = api.ctypes.c_int64(0)
    assert lib.gcre_decorated_splits(api.ctypes.byref(d.c), None, 0, 0, 0, api._ptr(out), 3, api.ctypes.byref(n_out)) \
        == api.GCRE_ERR_RANGE and n_out.value == 4                # capacity below the split count
    d = api._DpInput(1, 4, 6, [[0, 1]], data, None, np.arange(10) % 3, 0, 0)
    d.stratum[4] = 7                                            # stratum id past n_strata
    out = d.out()
    assert lib.gcre_decorated_splits(api.ctypes.byref(d.c), None, 0, 0, 0, api._ptr(out), 2, api.ctypes.byref(n_out)) \
        == api.GCRE_ERR_RANGE


# ---- worked by hand ---------------------------------------------------------------------------------------------------
# 4 cases (patients 0-3), 6 controls (4-9).  A = {0,1,4}, B = {1,2,5,6}, C = {2,3,7}; the path A -> B -> C.
HAND = np.zeros((3, 10), np.int32)
for _g, _c in enumerate(([0, 1, 4], [1, 2, 5, 6], [2, 3, 7])):
    HAND[_g, _c] = 1


def test_hand_worked_unsigned():
    VT = api.values_table(4, 6)
    got, _ = api.decorated_splits(1, 4, 6, [[0, 1, 2]], HAND, None, VT)
    # Forward 1: {A} = {0,1,4} (2 cases, 1 control); B \ A = {2,5,6}: 1 case, 2 controls drawn from the 7 others (2 cases)
    # Forward 2: {A,B} = {0,1,2,4,5,6} (3, 3); C \ {A,B} = {3,7}: (1, 1) from the 4 others (1 case)
    # Backward 3: {C} = {2,3,7} (2, 1); B \ C = {1,5,6}: (1, 2) from 7 (2 cases)
    # Backward 2: {C,B} = {1,2,3,5,6,7} (3, 3); A \ {C,B} = {0,4}: (1, 1) from 4 (1 case)
    want = [(0, 1, 2, 1, 1, 2, 3, 7, 2, (3, 3)), (0, 2, 3, 3, 1, 1, 2, 4, 1, (4, 4)),
            (1, 3, 2, 1, 1, 2, 3, 7, 2, (3, 3)), (1, 2, 3, 3, 1, 1, 2, 4, 1, (4, 4))]
    for s, (d, j, c1, t1, c2, t2, k, pop, succ, cell) in zip(got, want):
        assert (s["direction"], s["j"], s["cases1"], s["ctrls1"], s["cases2"], s["ctrls2"]) == (d, j, c1, t1, c2, t2)
        assert (s["k_pos"], s["pop_pos"], s["succ_pos"], s["k_neg"]) == (k, pop, succ, 0)
        assert s["score"] == VT[cell]


def test_hand_worked_signed_with_strata():
    """A (+) -> B (-) -> C (+), Forward j = 1: B goes to the neg half, where sub-path 1 has nothing, so its overlap with A
    (patient 1) stays.  Without strata all 4 carriers are drawn from the 10 patients (6 controls); with strata
    {0,1,4,5,8} / {2,3,6,7,9} only G_s = stratum minus A's {0,1,4} is drawn from: patient 1 is not drawn."""
    VT = api.values_table(4, 6)
    got, _ = api.decorated_splits(2, 4, 6, [[0, 1, 2]], HAND, [[1, -1, 1]], VT)
    s = got[0]
    assert (s["case_pos1"], s["ctrl_pos1"], s["case_neg2"], s["ctrl_neg2"]) == (2, 1, 2, 2)  # neg: {5,6} controls, {1,2} cases
    assert (s["cases1"], s["ctrls1"], s["cases2"], s["ctrls2"]) == (2, 1, 2, 2)
    assert s["score"] == VT[2, 1] + VT[2, 2]
    assert (s["k_pos"], s["k_neg"], s["pop_neg"], s["succ_neg"]) == (0, 4, 10, 6)
    strata = np.array([0, 0, 1, 1, 0, 0, 1, 1, 0, 1])
    got, st = api.decorated_splits(2, 4, 6, [[0, 1, 2]], HAND, [[1, -1, 1]], VT, strata)
    assert (got[0]["k_pos"], got[0]["k_neg"]) == (0, 3)
    assert [tuple(int(v) for v in x) for x in st[0]] == [(2, 0, 0, 1), (5, 2, 0, 2)]   # (pop, cases, k_pos, k_neg)
    # stratum ids are any integers, taken in ascending order
    _, st2 = api.decorated_splits(2, 4, 6, [[0, 1, 2]], HAND, [[1, -1, 1]], VT, strata * 10 + 3)
    np.testing.assert_array_equal(st, st2)


# ---- report.decorated_table -------------------------------------------------------------------------------------------


def _results(rows):
    return pd.DataFrame(rows, columns=report.COLUMNS)


def test_decorated_table_shape_without_permutations():
    """Columns, row order (lengths ascending, GWASPA.Results order inside a length, Forward j = 1..L-1 then Backward
    j = L..2), the Subpaths strings, the copied columns, NaN for NA genes and for n_permutations = 0."""
    genes = ["A", "B", "C", "D"]
    data = np.vstack([HAND, (np.arange(10) % 4 == 0).astype(np.int32)])
    res = _results([
        ["A (+) -> B (-) -> C (+)", "A -> B -> C", 3, 5.5, 0.01, 4, 3],
        ["D (+)", "D", 1, 1.0, 0.5, 1, 2],
        ["C (+) -> D (+)", "C -> D", 2, 2.5, 0.2, 3, 2],
        ["B (+) -> NA (+)", "B -> NA", 2, -np.inf, np.nan, 0, 0],
    ])
    out = report.decorated_table(res, genes, data, 4, 6, True, 0)
    assert list(out.columns) == report.DECORATED_COLUMNS
    assert out["SignedPaths"].tolist() == ["C (+) -> D (+)"] * 2 + ["B (+) -> NA (+)"] * 2 + ["A (+) -> B (-) -> C (+)"] * 4
    assert out["Direction"].tolist() == ["Forward", "Backward"] * 2 + ["Forward", "Forward", "Backward", "Backward"]
    assert out["Subpaths1"].tolist() == ["C", "D", "B", "NA", "A", "A -> B", "C", "C -> B"]
    assert out["Subpaths2"].tolist() == ["D", "C", "NA", "B", "B", "C", "B", "A"]
    assert out["Lengths"].tolist() == [2, 2, 2, 2, 3, 3, 3, 3]
    assert out["Scores"].tolist()[4:] == [5.5] * 4 and out["Cases"].tolist()[4:] == [4] * 4
    assert out["Controls"].tolist()[:2] == [2, 2] and out["Pvalues"].tolist()[:2] == [0.2, 0.2]
    assert out["DecoratedPvalues"].isna().all()
    # A (+) -> B (-) -> C (+), Forward 1 (see test_hand_worked_signed_with_strata)
    assert out.iloc[4][["Subpaths1_Cases", "Subpaths1_Controls", "Subpaths2_Cases", "Subpaths2_Controls"]].tolist() == [2, 1, 2, 2]
    assert out.iloc[2:4][["Subpaths1_Cases", "Subpaths2_Controls"]].to_numpy().tolist() == [[0, 0], [0, 0]]
    # unsigned: every gene in the pos half, the hand-worked numbers of test_hand_worked_unsigned
    out1 = report.decorated_table(res, genes, data, 4, 6, False, 0)
    assert out1.iloc[4:][["Subpaths1_Cases", "Subpaths1_Controls", "Subpaths2_Cases", "Subpaths2_Controls"]] \
        .to_numpy().tolist() == [[2, 1, 1, 2], [3, 3, 1, 1], [2, 1, 1, 2], [3, 3, 1, 1]]


def test_decorated_table_edge_cases():
    genes, data = ["A", "B", "C"], HAND
    only1 = _results([["A (+)", "A", 1, 1.0, 0.5, 2, 1]])
    empty = report.decorated_table(only1, genes, data, 4, 6, False, 0)
    assert list(empty.columns) == report.DECORATED_COLUMNS and len(empty) == 0
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert report.decorated_table(only1, genes, data, 4, 6, False, 100, path_length=1) is None
    assert [str(x.message) for x in w] == ["Can only compute the Decorated P-values for pathLength > 1!"]


TABLE_ASKS = {"zeros": ("+0", "-0", "negative"), "nonfinite": ("NaN", "-inf", "+inf"), "tiny": ("denormal",), "huge": (),
              "ladder": (), "few_both": ("negative",)}


def table_case_holds(kind, method):
    """(the kinds of observed value the case's splits hold, per stratification whether a drawing split has a permutation that
    ties its observed value exactly while others do not); the host stage equals the transcription on the way."""
    nc, nt, data, paths, signs, VT = table_case(kind, method)
    kinds, tie = None, {}
    for stratified in (False, True):
        strata = table_strata(nc, nt) if stratified else None
        want = r_decorated_splits(data, paths, signs, nc, nt, method, VT, strata)
        host, st, counts, n_ge, ties = table_expectation(kind, method, stratified)
        assert_same(host, want, st)
        kinds = observed_kinds([w["score"] for w in want if w["valid"]])
        draws = (host["k_pos"] + host["k_neg"] > 0) & (host["valid"] != 0)
        tie[stratified] = bool((draws & (ties > 0) & (ties < TABLE_PERMS)).any())
        nan = (host["valid"] != 0) & np.isnan(host["score"])
        assert (n_ge[nan] == 0).all()               # R/DecoratedPvalue.R:290: which(scores >= NaN) is empty
    return kinds, tie


@pytest.mark.parametrize("method", [1, 2])
def test_special_tables_hold_every_kind_of_observed_value(method):
    """What tests/test_gpu_decorated.py::test_special_tables needs of its inputs, on the transcription and the restated
    sampler alone: observed values of NaN, both zeros, both infinities and an f32 denormal, the -1 padding of a short
    table, and with and without strata a split with a permutation that ties its observed value exactly."""
    union, tie = {}, {False: False, True: False}
    for kind in TABLE_KINDS:
        kinds, t = table_case_holds(kind, method)
        missing = [k for k in TABLE_ASKS[kind] if not kinds[k]]
        assert not missing, (kind, method, missing)
        for k, v in kinds.items():
            union[k] = union.get(k, False) or v
        for k in tie:
            tie[k] |= t[k]
    assert all(union.values()), union
    assert all(tie.values()), tie
