"""Null exceedance counts, host side: report.fdr_columns on a hand-worked example, report.exceed_reference against a brute
force triple loop on a three-gene problem and against the null vectors of test_sets_host.restate on a random one, and the
declarations of the C interface.  No GPU needed."""
from __future__ import annotations

import os
from types import SimpleNamespace

import numpy as np
import pytest

from geneticscre_amd import api, report
from helpers import small_table
from test_sets_host import fold_f32, restate, vt_cell, vt_max


def uids_of(count, location, signs, path_length):
    return SimpleNamespace(count=np.asarray(count, np.int32), location=np.asarray(location, np.int64),
                           signs=np.asarray(signs, np.int32), path_length=path_length)


def packed(rows_pos, rows_neg=None):
    """Path rows as the library keeps them: the (+) half, then (signed method) the (-) half."""
    n = np.asarray(rows_pos).shape[1]
    a = api.pack_carriers(rows_pos, n)
    return a if rows_neg is None else np.concatenate([a, api.pack_carriers(rows_neg, n)], axis=1)


# ---- fdr_columns ----------------------------------------------------------------------------------------------------


def test_fdr_columns_hand_worked():
    # ten permutations; thresholds in no order, one tie (3.0 twice), one threshold nothing is observed at
    thr = [5.0, 3.0, 3.0, 1.0, 9.0, 2.0]
    exceed = [2, 10, 10, 100, 0, 12]
    observed = [1, 4, 4, 20, 0, 16]
    c = report.fdr_columns(thr, exceed, observed, 10)
    assert c["ExpectedFalse"].tolist() == [0.2, 1.0, 1.0, 10.0, 0.0, 1.2]
    # FDR = min(1, PFER / observed): 0.2, 0.25, 0.25, 0.5, nothing observed, 0.075
    np.testing.assert_array_equal(c["FDR"][[0, 1, 2, 3, 5]], [0.2, 0.25, 0.25, 0.5, 1.2 / 16])
    assert np.isnan(c["FDR"][4])
    # q = the smallest FDR among the thresholds that are not larger: 1.0 -> 0.5; 2.0 -> 0.075; 3.0 (both) -> 0.075, the
    # monotone step (their own FDR is 0.25); 5.0 -> 0.075; 9.0 stays NaN
    np.testing.assert_array_equal(c["Qvalues"][[3, 5, 1, 2, 0]], [0.5, 0.075, 0.075, 0.075, 0.075])
    assert np.isnan(c["Qvalues"][4])
    # never above 1, and non-increasing as the threshold rises
    c = report.fdr_columns([1.0, 2.0, 3.0], [500, 30, 1], [3, 2, 1], 10)
    assert c["FDR"].tolist() == [1.0, 1.0, 0.1] and c["Qvalues"].tolist() == [1.0, 1.0, 0.1]
    # no permutations: everything NaN, nothing raised
    c = report.fdr_columns(thr, [0] * 6, observed, 0)
    assert all(np.isnan(c[k]).all() for k in report.FDR_COLUMNS)
    assert report.FDR_COLUMNS == ["ExpectedFalse", "FDR", "Qvalues"]


# ---- exceed_reference -----------------------------------------------------------------------------------------------
# patients 0-2 are cases, 3-5 controls; VT[a][b] = 4a + b + 0.25
ROWS = np.array([[1, 0, 0, 1, 0, 0],     # g0
                 [0, 1, 0, 0, 0, 0],     # g1
                 [0, 0, 0, 0, 1, 1]])    # g2
VT4 = (4 * np.arange(4)[:, None] + np.arange(4)[None, :] + 0.25).astype(np.float64)
MASKS = np.array([[1, 1, 1, 0, 0, 0],
                  [0, 0, 0, 1, 1, 1],
                  [1, 0, 0, 1, 1, 0]], bool)


def brute(method, n_cases, uids, pos0, neg0, pos1, neg1, VT, masks, thr, shard=None):
    """Three nested loops, integers and Python floats only."""
    n = pos0.shape[1]
    exceed, observed, p = [0] * len(thr), [0] * len(thr), 0
    for i, cnt in enumerate(uids.count.tolist()):
        for j in range(max(cnt, 0)):
            loc = int(uids.location[i]) + j
            here, p = p, p + 1
            if shard is not None and not shard[0] <= here < shard[1]:
                continue
            if method == 1:
                P, N = pos0[i] | pos1[loc], np.zeros(n, bool)
            else:
                L = uids.path_length
                sign = uids.signs[i] if L > 3 else uids.signs[loc] if L < 3 else (-1 if uids.signs[i] + uids.signs[loc] == 0 else 1)
                a, b = (pos1[loc], neg1[loc]) if sign == 1 else (neg1[loc], pos1[loc])
                P, N = pos0[i] | a, neg0[i] | b
            case = np.arange(n) < n_cases
            if method == 1:
                score = float(vt_cell(VT, n, int((P & case).sum()), int((P & ~case).sum())))
            else:
                score = float(vt_cell(VT, n, int((P & case).sum()), int((P & ~case).sum())) +
                              vt_cell(VT, n, int((N & ~case).sum()), int((N & case).sum())))
            for k, t in enumerate(thr):
                observed[k] += score > -np.inf and score >= t
            for m in masks:
                pp, pn = int((P & m).sum()), int((N & m).sum())
                if method == 1:
                    v = fold_f32(vt_cell(VT, n, pp, int(P.sum()) - pp))
                else:
                    v = fold_f32(vt_max(VT, n, pp, int(P.sum()) - pp) + vt_max(VT, n, int(N.sum()) - pn, pn))
                for k, t in enumerate(thr):
                    exceed[k] += float(v) >= t
    return exceed, observed


@pytest.mark.parametrize("method", [1, 2])
def test_reference_equals_the_triple_loop_on_three_genes(method):
    rows = ROWS.astype(bool)
    zero = np.zeros_like(rows)
    # paths0 = the three genes, paths1 = the three genes; uid 0 joins rows 1..2, uid 1 row 2, uid 2 rows 0..1
    u = uids_of([2, 1, 2], [1, 2, 0], [1, -1, 1], 2)
    thr = [9.25, 6.25, -1.0, 100.0, 6.25, 2.25, 0.0, 12.5]
    want_e, want_o = brute(method, 3, u, rows, zero, rows, zero, VT4, MASKS, thr)
    r0 = packed(ROWS) if method == 1 else packed(ROWS, zero)
    got = report.exceed_reference(method, 3, 3, u, r0, r0, VT4, MASKS, thr)
    assert got["exceed"].dtype == np.uint64 and got["observed"].dtype == np.uint64
    assert got["exceed"].tolist() == want_e and got["observed"].tolist() == want_o
    assert (got["perms"], got["paths"]) == (3, 5)
    assert got["exceed"][2] == 15 and got["exceed"][3] == 0 and any(0 < e < 15 for e in want_e)   # all, none, some
    assert got["exceed"][1] == got["exceed"][4]                                                # equal thresholds, equal counts
    # a shard and a window of the permutations: sums over the parts give the whole
    a = report.exceed_reference(method, 3, 3, u, r0, r0, VT4, MASKS, thr, shard=(0, 2))
    b = report.exceed_reference(method, 3, 3, u, r0, r0, VT4, MASKS, thr, shard=(2, 5))
    assert (a["exceed"] + b["exceed"]).tolist() == want_e and (a["observed"] + b["observed"]).tolist() == want_o
    assert a["exceed"].tolist() == brute(method, 3, u, rows, zero, rows, zero, VT4, MASKS, thr, shard=(0, 2))[0]
    w0 = report.exceed_reference(method, 3, 3, u, r0, r0, VT4, MASKS, thr, window=(0, 1))
    w1 = report.exceed_reference(method, 3, 3, u, r0, r0, VT4, MASKS, thr, window=(1, 3))
    assert (w0["exceed"] + w1["exceed"]).tolist() == want_e and (w0["perms"], w1["perms"]) == (1, 2)
    # packed masks are read like bool ones
    pm = api.pack_carriers(MASKS, 6)
    assert report.exceed_reference(method, 3, 3, u, r0, r0, VT4, pm, thr)["exceed"].tolist() == want_e
    with pytest.raises(ValueError):
        report.exceed_reference(method, 3, 3, u, r0, r0, VT4, MASKS, [1.0, np.nan])


@pytest.mark.parametrize("method", [1, 2])
def test_reference_equals_the_set_restatement_on_a_random_problem(method):
    """A level-2 join read as sets of two rows: restate (tests/test_sets_host.py) gives every set's f32 null vector and
    score; the counts follow from them by comparison."""
    rng = np.random.default_rng(23 + method)
    nc, nt, G, K = 37, 45, 16, 70
    n = nc + nt
    data = rng.random((G, n)) < rng.uniform(0.03, 0.3, size=(G, 1))
    VT = small_table(n, n, 5)
    masks = np.stack([rng.permutation(n) < nc for _ in range(K)])
    count = rng.integers(0, 4, size=G)
    location = np.array([rng.integers(0, G - c + 1) for c in count])
    signs = rng.choice([-1, 1], size=G)
    u = uids_of(count, location, signs, 2)
    sets, sg = [], []
    for i in range(G):
        for j in range(count[i]):
            sets.append([i, int(location[i]) + j])
            sg.append([1, int(signs[location[i] + j])])      # path_length < 3: the sign of the paths1 row decides the half
    recs, nulls, family = restate(method, nc, nt, sets, data, sg, VT, masks)
    scores = np.array([r["score"] for r in recs])
    allv = np.concatenate(nulls).astype(np.float64)
    thr = np.concatenate([np.quantile(allv, [0.5, 0.9, 0.99]), np.sort(scores)[-5:], [-3.0, 0.0, 1e9, float(family.max())]])
    zero = np.zeros_like(data)
    rows = packed(data) if method == 1 else packed(data, zero)
    got = report.exceed_reference(method, nc, nt, u, rows, rows, VT, masks, thr)
    assert got["exceed"].tolist() == [int((allv >= t).sum()) for t in thr]
    assert got["observed"].tolist() == [int((scores >= t).sum()) for t in thr]
    np.testing.assert_array_equal(got["scores"], scores)
    assert 0 < got["exceed"][0] < len(sets) * K and got["exceed"][-2] == 0 and got["exceed"][-1] >= 1
    assert got["exceed"][-4] == len(sets) * K == got["exceed"][-3]


# ---- the interface --------------------------------------------------------------------------------------------------


def test_interface_is_declared():
    names = ["gcre_exceed_create", "gcre_join_set_exceed", "gcre_process_paths_set_exceed", "gcre_exceed_read",
             "gcre_exceed_reset", "gcre_exceed_free"]
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "gcre_hip.h")).read()
    for nm in names:
        assert nm in api.EXPORTS and nm + "(" in header
    assert "#define GCRE_ABI_VERSION 4" in header           # additions only
    assert api.EXCEED_MAX == 10000
    assert callable(api.ExceedCounts) and callable(report.exceed_reference) and callable(report.fdr_columns)
    # counters live on a context: the one-call driver says so before it makes one
    with pytest.raises(api.GcreError, match="exec_"):
        api.process_paths(None, exceeds={"2": object()})
