"""Per-permutation exceedance counts, host side: report.false_count_columns on hand-worked arrays,
report.exceed_reference(per_permutation=True) against the null vectors of test_sets_host.restate on a 20-gene problem, and
the declarations of the C interface.  No GPU needed."""
from __future__ import annotations

import os

import numpy as np
import pytest

from geneticscre_amd import api, report
from helpers import small_table
from test_exceed_host import packed, uids_of
from test_sets_host import restate

nan = float("nan")


def same(got, want):
    np.testing.assert_array_equal(np.asarray(got, np.float64), np.asarray(want, np.float64))


# ---- false_count_columns --------------------------------------------------------------------------------------------


def test_false_count_columns_hand_worked():
    # B = 10 permutations; thresholds in no order, one tie (3.0 twice: equal rows), one threshold nothing is observed at
    thr = [5.0, 3.0, 3.0, 1.0, 9.0]
    V = np.array([[0, 0, 5, 1, 0, 2, 0, 0, 9, 0],         # sorted: 0 0 0 0 0 0 1 2 5 9
                  [1, 1, 7, 2, 1, 2, 1, 1, 9, 1],         # sorted: 1 1 1 1 1 1 2 2 7 9
                  [1, 1, 7, 2, 1, 2, 1, 1, 9, 1],
                  [4, 3, 9, 4, 3, 4, 3, 3, 9, 5],         # sorted: 3 3 3 3 4 4 4 5 9 9
                  [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]], np.uint64)
    observed = [4, 8, 8, 20, 0]
    c = report.false_count_columns(thr, V, observed, 10, ks=(1, 2, 5, 10), alpha=0.05)
    assert list(c) == ["MedianFalse", "FDRmedian", "FalseBound", "FDPbound", "kFWER.1", "kFWER.2", "kFWER.5", "kFWER.10"]
    assert list(c) == report.false_count_names((1, 2, 5, 10))
    # the ceil(10 / 2) = 5th smallest; the ceil(0.95 * 10) = 10th smallest
    same(c["MedianFalse"], [0, 1, 1, 4, 0])
    same(c["FalseBound"], [9, 9, 9, 9, 0])
    same(c["FDRmedian"], [0.0, 1 / 8, 1 / 8, 4 / 20, nan])
    same(c["FDPbound"], [1.0, 1.0, 1.0, 9 / 20, nan])                     # min(1, .): 9/4 and 9/8 are cut
    same(c["kFWER.1"], [0.4, 1.0, 1.0, 1.0, 0.0])
    same(c["kFWER.2"], [0.3, 0.4, 0.4, 1.0, 0.0])
    same(c["kFWER.5"], [0.2, 0.2, 0.2, 0.3, 0.0])
    same(c["kFWER.10"], [0.0] * 5)                                          # k larger than every count
    for v in c.values():
        assert v.dtype == np.float64 and v[1] == v[2]                      # equal thresholds, equal rows
    # alpha = 0: the largest count; 0.2: the ceil(8) = 8th; 0.25: ceil(7.5) = 8th; 0.3: the 7th -- ranks taken exactly,
    # (1 - 0.3) * 10 is 7.000000000000001 in binary floating point and must not become the 8th
    for alpha, want in ((0.0, [9, 9, 9, 9, 0]), (0.2, [2, 2, 2, 5, 0]), (0.25, [2, 2, 2, 5, 0]), (0.3, [1, 2, 2, 4, 0]),
                        (0.5, [0, 1, 1, 4, 0]), (0.9, [0, 1, 1, 3, 0]), (0.999, [0, 1, 1, 3, 0]), (1.0, [0, 1, 1, 3, 0])):
        same(report.false_count_columns(thr, V, observed, 10, alpha=alpha)["FalseBound"], want)
    # the default ks
    assert list(report.false_count_columns(thr, V, observed, 10)) == report.false_count_names() == [
        "MedianFalse", "FDRmedian", "FalseBound", "FDPbound", "kFWER.2", "kFWER.5", "kFWER.10"]
    # counts beyond 2^53 keep their order (uint64 all the way to the order statistic)
    big = np.array([[2**63 + 2, 2**63, 2**63 + 1]], np.uint64)
    c = report.false_count_columns([1.0], big, [1], 3, ks=(2**62,), alpha=0.0)
    assert c["MedianFalse"][0] == float(2**63 + 1) and c[f"kFWER.{2**62}"][0] == 1.0


def test_false_count_columns_edges():
    thr, observed = [2.0, 1.0], [3, 0]
    # B = 0: every column NaN, whatever is passed for the counts (an object that kept none reads None)
    for V in (None, np.zeros((2, 0), np.uint64)):
        c = report.false_count_columns(thr, V, observed, 0, ks=(1, 3))
        assert list(c) == report.false_count_names((1, 3)) and all(np.isnan(v).all() and len(v) == 2 for v in c.values())
    # B = 1: the one permutation is the median and every bound
    V = np.array([[2], [7]], np.uint64)
    for alpha in (0.0, 0.05, 0.999):
        c = report.false_count_columns(thr, V, observed, 1, ks=(1, 3), alpha=alpha)
        same(c["MedianFalse"], [2, 7])
        same(c["FalseBound"], [2, 7])
        same(c["FDRmedian"], [2 / 3, nan])                                  # observed == 0: the ratios are NaN, the counts not
        same(c["FDPbound"], [2 / 3, nan])
        same(c["kFWER.1"], [1.0, 1.0])
        same(c["kFWER.3"], [0.0, 1.0])
    # B = 2: the median is the ceil(2 / 2) = 1st smallest
    c = report.false_count_columns([1.0], np.array([[5, 1]], np.uint64), [10], 2)
    assert c["MedianFalse"][0] == 1 and c["FalseBound"][0] == 5
    with pytest.raises(ValueError):
        report.false_count_columns(thr, V, observed, 2)                     # one column, two permutations
    with pytest.raises(ValueError):
        report.false_count_columns(thr, V, observed, 1, alpha=1.5)


def test_kfwer_1_is_the_family_wise_p_value():
    """V[j][r] >= 1 iff permutation r's maximum reaches threshold j: kFWER.1 is #{r : max_r >= t} / B."""
    rng = np.random.default_rng(8)
    null = rng.gamma(2.0, size=(40, 25)).astype(np.float32)                 # [path][permutation]
    thr = np.quantile(null, [0.5, 0.9, 0.99, 1.0])
    V = (null.astype(np.float64)[None, :, :] >= thr[:, None, None]).sum(axis=1).astype(np.uint64)
    c = report.false_count_columns(thr, V, [1] * 4, 25, ks=(1,))
    same(c["kFWER.1"], [(null.max(axis=0).astype(np.float64) >= t).mean() for t in thr])


# ---- exceed_reference(per_permutation=True) -------------------------------------------------------------------------


@pytest.mark.parametrize("method", [1, 2])
def test_reference_per_permutation_on_a_twenty_gene_problem(method):
    """A level-2 join of 20 genes read as sets of two rows (as tests/test_exceed_host.py does): restate gives every set's f32
    null vector; V[j][r] follows by comparison."""
    rng = np.random.default_rng(61 + method)
    nc, nt, G, K = 33, 41, 20, 90
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
            sg.append([1, int(signs[location[i] + j])])
    _, nulls, _ = restate(method, nc, nt, sets, data, sg, VT, masks)
    null = np.stack(nulls).astype(np.float64)                                # [path][permutation]
    P = len(sets)
    thr = np.concatenate([np.quantile(null, [0.5, 0.9, 0.99]), [-3.0, 0.0, 1e9], np.quantile(null, [0.9])])
    rows = packed(data) if method == 1 else packed(data, np.zeros_like(data))
    args = (method, nc, nt, u, rows, rows, VT, masks, thr)
    got = report.exceed_reference(*args, per_permutation=True)
    V = got["perm_counts"]
    assert V.dtype == np.uint64 and V.shape == (len(thr), K)
    np.testing.assert_array_equal(V, (null[None, :, :] >= thr[:, None, None]).sum(axis=1))
    np.testing.assert_array_equal(V.sum(axis=1), got["exceed"])
    np.testing.assert_array_equal(V[1], V[-1])                               # equal thresholds, equal rows
    assert (V[3] == P).all() and (V[4] == P).all() and not V[5].any()        # every path, every path, none
    assert ((V[0] > 0) & (V[0] < P)).any() and len(set(V[0].tolist())) > 1   # it can tell right from wrong
    # without the flag the result is what it was
    plain = report.exceed_reference(*args)
    assert "perm_counts" not in plain and plain["exceed"].tolist() == got["exceed"].tolist()
    # windows are column ranges, shards add cell by cell
    cuts = (0, 17, 64, K)
    for a, b in zip(cuts[:-1], cuts[1:]):
        w = report.exceed_reference(*args, window=(a, b), per_permutation=True)
        assert w["perms"] == b - a
        np.testing.assert_array_equal(w["perm_counts"], V[:, a:b])
        np.testing.assert_array_equal(w["perm_counts"].sum(axis=1), w["exceed"])
    parts = [report.exceed_reference(*args, shard=s, per_permutation=True) for s in ((0, P // 3), (P // 3, P))]
    np.testing.assert_array_equal(parts[0]["perm_counts"] + parts[1]["perm_counts"], V)
    for part in parts:
        np.testing.assert_array_equal(part["perm_counts"].sum(axis=1), part["exceed"])
    both = report.exceed_reference(*args, shard=(P // 3, P), window=(17, 64), per_permutation=True)
    np.testing.assert_array_equal(both["perm_counts"], parts[1]["perm_counts"][:, 17:64])
    # no permutations, no paths
    none = report.exceed_reference(*args, window=(5, 5), per_permutation=True)
    assert none["perm_counts"].shape == (len(thr), 0)
    empty = report.exceed_reference(*args, shard=(2, 2), per_permutation=True)
    assert empty["perm_counts"].shape == (len(thr), K) and not empty["perm_counts"].any()


# ---- the interface --------------------------------------------------------------------------------------------------


def test_interface_is_declared():
    import inspect
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "gcre_hip.h")).read()
    for nm in ("gcre_exceed_keep_perm_counts", "gcre_exceed_read_perm_counts"):
        assert nm in api.EXPORTS and nm + "(" in header
    assert "#define GCRE_ABI_VERSION 4" in header           # additions only
    assert api.EXCEED_PERM_CELLS == report.EXCEED_PERM_CELLS == 1 << 26
    assert inspect.signature(api.ExceedCounts.__init__).parameters["perm_counts"].default is False
    assert inspect.signature(report.exceed_reference).parameters["per_permutation"].default is False
    sig = inspect.signature(report.gwaspa).parameters
    assert sig["false_counts"].default is False and tuple(sig["false_count_ks"].default) == (2, 5, 10)
    assert sig["false_count_alpha"].default == 0.05
    assert api.Exceedances(np.zeros(1, np.uint64), np.zeros(1, np.uint64), 0, 0).perm_counts is None
    # the limit is checked before anything is built or run (no GPU is touched here)
    with pytest.raises(ValueError, match="2\\^26"):
        report.gwaspa(["G1"], np.zeros((1, 4), np.int32), 2, 2, ([], [], [], [], []), top_k=10000, n_permutations=6711,
                      false_counts=True)
