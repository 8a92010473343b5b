"""Set scoring, host side: a numpy restatement of gcre_score_sets' semantics checked on a hand-worked example of each
method, a literal transcription of checkBestPaths' score formulas (R/CheckResults.R) checked against the restatement, and
the parsing of score_paths' three path forms.  No GPU needed."""
from __future__ import annotations

import numpy as np

from geneticscre_amd import report
from helpers import small_table


# ---- the semantics, restated (include/gcre_hip.h gcre_score_sets) ---------------------------------------------------


def vt_cell(VT, n, a, b):
    """VT[a][b] as the device reads its copy: -1 outside the caller's table and beyond n patients (k_table_to_diag)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    ok = (a <= n) & (b <= n) & (a < VT.shape[0]) & (b < VT.shape[1])
    return np.where(ok, VT[np.minimum(a, VT.shape[0] - 1), np.minimum(b, VT.shape[1] - 1)], -1.0)


def vt_max(VT, n, a, b):
    """compute_value_table_max (methods.h:110-118) with std::max semantics."""
    x, y = vt_cell(VT, n, a, b), vt_cell(VT, n, b, a)
    return np.where(x < y, y, x)


def fold_f32(x):
    """The f32 value the join's null kernels fold into their maxima: rounded to f32, NaN and negatives as +0."""
    f = np.asarray(x, np.float64).astype(np.float32)
    return np.where(f > 0, f, np.float32(0)).astype(np.float32)


def restate(method, n_cases, n_ctrls, sets, rows, signs, VT, masks):
    """Every set's record fields and its null vector, and the family maximum.  ``rows`` 0/1 [rows][n]; ``masks`` bool
    [K][n] (True = a case under that permutation)."""
    n = n_cases + n_ctrls
    rows = np.asarray(rows) != 0
    K = len(masks)
    mf = np.asarray(masks, dtype=np.float32).reshape(K, n)
    case = np.arange(n) < n_cases
    recs, nulls = [], []
    family = np.zeros(K, np.float32)
    for s, members in enumerate(sets):
        sg = signs[s] if signs is not None else [1] * len(members)
        r = dict(set=s, valid=int(all(m >= 0 for m in members)), cases=0, ctrls=0, cases_pos=0, ctrls_pos=0,
                 cases_neg=0, ctrls_neg=0, score=np.nan, n_ge=0, pvalue=np.nan)
        if not r["valid"]:
            recs.append(r)
            nulls.append(None)
            continue
        P, N = np.zeros(n, bool), np.zeros(n, bool)
        for m, x in zip(members, sg):
            if method == 2 and x == -1:
                N |= rows[m]
            else:
                P |= rows[m]
        r.update(cases_pos=int((P & case).sum()), ctrls_pos=int((P & ~case).sum()),
                 cases_neg=int((N & ~case).sum()), ctrls_neg=int((N & case).sum()))
        r["cases"], r["ctrls"] = r["cases_pos"] + r["cases_neg"], r["ctrls_pos"] + r["ctrls_neg"]
        pp = (mf @ P.astype(np.float32)).astype(np.int64)          # exact: counts < 2^24
        if method == 1:
            r["score"] = float(vt_cell(VT, n, r["cases_pos"], r["ctrls_pos"]))
            null = fold_f32(vt_cell(VT, n, pp, int(P.sum()) - pp))
        else:
            r["score"] = float(vt_cell(VT, n, r["cases_pos"], r["ctrls_pos"]) + vt_cell(VT, n, r["cases_neg"], r["ctrls_neg"]))
            pn = (mf @ N.astype(np.float32)).astype(np.int64)
            null = fold_f32(vt_max(VT, n, pp, int(P.sum()) - pp) + vt_max(VT, n, int(N.sum()) - pn, pn))
        r["n_ge"] = int((null.astype(np.float64) >= r["score"]).sum())
        r["pvalue"] = r["n_ge"] / K if K else np.nan
        family = np.maximum(family, null)
        recs.append(r)
        nulls.append(null)
    return recs, nulls, family


def restate_slabs(method, n_cases, n_ctrls, pos, neg, VT, masks, slab=512):
    """``restate`` for many sets, each given by its union rows (``pos`` bool [V][n], and for method 2 ``neg``): the same
    definition a slab of sets at a time.  Every cell the sets can read is looked up once through vt_cell / vt_max ([a][b] for
    a, b <= n); a slab's null values are then one gather per cell.  Returns arrays over the sets (the record fields, "score",
    "n_ge") and "family" (f32 [K])."""
    n = n_cases + n_ctrls
    pos = np.asarray(pos) != 0
    neg = np.asarray(neg) != 0 if method == 2 else np.zeros_like(pos)
    V, K = len(pos), len(masks)
    mft = np.ascontiguousarray(np.asarray(masks, dtype=np.float32).reshape(K, n).T)
    case = np.arange(n) < n_cases
    a, b = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    cell = vt_cell(VT, n, a, b)
    out = {"cases_pos": (pos & case).sum(axis=1), "ctrls_pos": (pos & ~case).sum(axis=1),
           "cases_neg": (neg & ~case).sum(axis=1), "ctrls_neg": (neg & case).sum(axis=1)}
    out["cases"], out["ctrls"] = out["cases_pos"] + out["cases_neg"], out["ctrls_pos"] + out["ctrls_neg"]
    out["score"] = cell[out["cases_pos"], out["ctrls_pos"]]
    if method == 2:
        out["score"] = out["score"] + cell[out["cases_neg"], out["ctrls_neg"]]
        big = vt_max(VT, n, a, b).ravel()
    else:
        folded = fold_f32(cell).ravel()
    tp, tn = pos.sum(axis=1), neg.sum(axis=1)
    out["n_ge"] = np.zeros(V, np.int64)
    family = np.zeros(K, np.float32)
    for lo in range(0, V, slab):
        s = slice(lo, lo + slab)
        pp = (pos[s].astype(np.float32) @ mft).astype(np.intp)          # exact: counts < 2^24
        if method == 1:
            null = folded[pp * n + tp[s, None]]                          # [pp][tot - pp] of an (n + 1)-wide table
        else:
            pn = (neg[s].astype(np.float32) @ mft).astype(np.intp)
            null = fold_f32(big[pp * n + tp[s, None]] + big[(tn[s, None] - pn) * (n + 1) + pn])
        out["n_ge"][s] = (null.astype(np.float64) >= out["score"][s, None]).sum(axis=1)
        if null.size:
            family = np.maximum(family, null.max(axis=0))
    out["family"] = family
    return out


def test_slabs_equal_the_restatement():
    """restate_slabs == restate on sets of one (+) and one (-) member, several slabs with a ragged last one."""
    rng = np.random.default_rng(5)
    nc, nt, K, V = 33, 37, 45, 53
    n = nc + nt
    VT = small_table(n, n, 2)
    VT[rng.random(VT.shape) < 0.05] *= -1
    masks = rng.random((K, n)) < 0.5
    pos = rng.random((V, n)) < rng.uniform(0.0, 0.6, size=(V, 1))
    neg = rng.random((V, n)) < rng.uniform(0.0, 0.6, size=(V, 1))
    pos[0], neg[1] = False, True
    for method in (1, 2):
        recs, _, family = restate(method, nc, nt, [[i, V + i] for i in range(V)], np.vstack([pos, neg]), [[1, -1]] * V, VT, masks)
        if method == 1:      # method 1 ignores the signs: both members join the one union
            got = restate_slabs(1, nc, nt, pos | neg, None, VT, masks, slab=16)
        else:
            got = restate_slabs(2, nc, nt, pos, neg, VT, masks, slab=16)
        for f in ("cases", "ctrls", "cases_pos", "ctrls_pos", "cases_neg", "ctrls_neg", "n_ge"):
            assert got[f].tolist() == [r[f] for r in recs], (method, f)
        assert got["score"].view(np.uint64).tolist() == [np.float64(r["score"]).view(np.uint64) for r in recs]
        assert family.view(np.uint32).tolist() == got["family"].view(np.uint32).tolist()


# ---- hand-worked examples -------------------------------------------------------------------------------------------
# patients 0-2 are cases, 3-5 controls; VT[a][b] = 4a + b + 0.25 (so vtmax[a][b] = 4 max + min + 0.25)
ROWS = np.array([[1, 0, 0, 1, 0, 0],     # g0
                 [0, 1, 0, 0, 0, 0],     # g1
                 [0, 0, 0, 0, 1, 1]])    # g2
VT4 = (4 * np.arange(4)[:, None] + np.arange(4)[None, :] + 0.25).astype(np.float64)
MASKS = np.array([[1, 1, 1, 0, 0, 0],    # r0: the real labels
                  [0, 0, 0, 1, 1, 1],    # r1: swapped
                  [1, 0, 0, 1, 1, 0]], bool)


def test_hand_worked_method1():
    recs, nulls, family = restate(1, 3, 3, [[0, 1], [2], [0, -1]], ROWS, None, VT4, MASKS)
    a, b, na = recs
    # {g0, g1}: U = {0, 1, 3}: 2 cases, 1 control -> VT[2][1] = 9.25; r0 p=2 -> 9.25, r1 p=1 -> VT[1][2] = 6.25,
    # r2 p=2 (0, 3) -> 9.25
    assert (a["cases"], a["ctrls"], a["score"]) == (2, 1, 9.25)
    assert nulls[0].tolist() == [9.25, 6.25, 9.25] and a["n_ge"] == 2 and a["pvalue"] == 2 / 3
    # {g2}: U = {4, 5}: 0 cases, 2 controls -> VT[0][2] = 2.25; r0 p=0 -> 2.25, r1 p=2 -> 8.25, r2 p=1 -> 5.25
    assert (b["cases"], b["ctrls"], b["score"], b["n_ge"]) == (0, 2, 2.25, 3)
    assert nulls[1].tolist() == [2.25, 8.25, 5.25]
    # an NA member: no score, out of the family
    assert na["valid"] == 0 and np.isnan(na["score"]) and np.isnan(na["pvalue"])
    assert family.tolist() == [9.25, 8.25, 9.25]


def test_hand_worked_method2():
    recs, nulls, family = restate(2, 3, 3, [[0, 1]], ROWS, [[1, -1]], VT4, MASKS)
    (r,) = recs
    # P = g0 = {0, 3}, N = g1 = {1}: cases_pos 1, ctrls_pos 1, cases_neg |N & ctrls| 0, ctrls_neg |N & cases| 1
    assert (r["cases_pos"], r["ctrls_pos"], r["cases_neg"], r["ctrls_neg"]) == (1, 1, 0, 1)
    assert (r["cases"], r["ctrls"]) == (1, 2)
    assert r["score"] == VT4[1, 1] + VT4[0, 1] == 6.5
    # r0: pp=1 -> vtmax[1][1] 5.25, pn=1 -> vtmax[0][1] 4.25; r1: pp=1, pn=0 -> vtmax[1][0] 4.25; r2: pp=2 -> vtmax[2][0] 8.25
    assert nulls[0].tolist() == [9.5, 9.5, 12.5] and r["n_ge"] == 3 and r["pvalue"] == 1.0
    assert family.tolist() == [9.5, 9.5, 12.5]
    # one gene under both signs lands in both halves (no conflict removal)
    (both,), _, _ = restate(2, 3, 3, [[0, 0]], ROWS, [[1, -1]], VT4, MASKS)
    assert (both["cases_pos"], both["ctrls_pos"], both["cases_neg"], both["ctrls_neg"]) == (1, 1, 1, 1)
    # method 1 ignores the signs
    (m1,), _, _ = restate(1, 3, 3, [[0, 1]], ROWS, [[1, -1]], VT4, MASKS)
    assert (m1["cases"], m1["ctrls"], m1["score"]) == (2, 1, 9.25)


# ---- checkBestPaths (R/CheckResults.R:29-73), transcribed -----------------------------------------------------------


def r_check_best_paths_score(genes, data, signed_path, n_cases, method, VT):
    """The per-row score of checkBestPaths; 0-based patient indices where R has 1-based ones (inds <= nCases <-> < n_cases)."""
    split_path = signed_path.split(" -> ")
    sign = [x.split(" ")[1] for x in split_path]
    sign = np.array([1 if s == "(+)" else -1 for s in sign])
    g = [x.split(" ")[0] for x in split_path]
    path_data_pos = np.array([data[genes.index(x)] for x in g])
    path_data_neg = np.zeros_like(path_data_pos)
    if method == 2:
        path_data_neg[sign == -1, :] = path_data_pos[sign == -1, :]
        path_data_pos[sign == -1, :] = 0
    subpath_pos1 = path_data_pos.sum(axis=0)
    subpath_pos1[subpath_pos1 != 0] = 1
    subpath_neg1 = path_data_neg.sum(axis=0)
    subpath_neg1[subpath_neg1 != 0] = 1
    inds_pos1 = np.flatnonzero(subpath_pos1 != 0)
    inds_neg1 = np.flatnonzero(subpath_neg1 != 0)
    cases_pos = len(np.flatnonzero(inds_pos1 < n_cases))
    controls_pos = len(inds_pos1) - cases_pos
    cases_neg = len(np.flatnonzero(inds_neg1 >= n_cases))
    controls_neg = len(inds_neg1) - cases_neg
    cases = cases_pos + cases_neg
    controls = controls_pos + controls_neg
    if method == 1:
        score = VT[cases, controls]
    else:
        score = VT[cases_pos, controls_pos] + VT[cases_neg, controls_neg]
    return score, cases, controls, (cases_pos, controls_pos, cases_neg, controls_neg)


def test_check_best_paths_transcription_matches_restatement():
    rng = np.random.default_rng(11)
    nc, nt = 37, 45
    n = nc + nt
    data = (rng.random((14, n)) < rng.uniform(0.03, 0.4, size=(14, 1))).astype(np.int32)
    genes = [f"S{i}" for i in range(14)]
    VT = small_table(n, n, 3)   # square: the signed method indexes rows by control counts too
    for method in (1, 2):
        for _ in range(60):
            L = int(rng.integers(1, 6))
            rows = rng.choice(14, size=L, replace=False).tolist()
            sg = rng.choice([-1, 1], size=L).tolist()
            path = " -> ".join(f"{genes[r]} {'(+)' if s == 1 else '(-)'}" for r, s in zip(rows, sg))
            score, cases, ctrls, halves = r_check_best_paths_score(genes, data, path, nc, method, VT)
            _, prow, psg = report.parse_sets([path], genes)
            (r,), _, _ = restate(method, nc, nt, prow, data, psg, VT, np.zeros((0, n), bool))
            assert r["score"] == score and (r["cases"], r["ctrls"]) == (cases, ctrls), path
            assert (r["cases_pos"], r["ctrls_pos"], r["cases_neg"], r["ctrls_neg"]) == halves, path


# ---- parsing --------------------------------------------------------------------------------------------------------


def test_parse_sets_forms_and_na():
    genes = ["A", "B", "C", "A"]
    names, rows, signs = report.parse_sets(["A (+) -> B (-) -> C (+)", "C -> A", ["B", "C", "Z"], "A (+) -> NA (-)",
                                            ("C",)], genes)
    assert names == [["A", "B", "C"], ["C", "A"], ["B", "C", "Z"], ["A", "NA"], ["C"]]
    assert rows == [[0, 1, 2], [2, 0], [1, 2, -1], [0, -1], [2]]        # first row of a symbol; unknown / NA -> -1
    assert signs == [[1, -1, 1], [1, 1], [1, 1, 1], [1, -1], [1]]
    assert callable(report.score_paths) and callable(report.check_best_paths)
    assert report.SCORE_PATHS_COLUMNS == ["SignedPaths", "Paths", "Lengths", "Scores", "Cases", "Controls",
                                          "NominalPvalues", "FamilyPvalues", "Pvalues"]
