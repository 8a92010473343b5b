"""Hit lists (gcre_hits), the parts that need no device: the numpy definition against hand-worked
examples, the significance cut-off against the p-value rule it inverts, the per-gene counts, and the declared interface."""
from __future__ import annotations

import os
import types

import numpy as np
import pytest

from geneticscre_amd import api, report

NINF = float("-inf")


def _uids():
    # three uid rows: counts 3, 0, 4 at paths1 locations 10, 99, 20 -> ordinals 0..6
    return types.SimpleNamespace(count=np.array([3, 0, 4], np.int32), location=np.array([10, 99, 20], np.int64))


#          ordinal   0     1     2     3     4        5     6
SCORES = np.array([2.5, -0.0, 7.0, 0.0, NINF, np.nan, 2.5])
CASES = np.array([1, 2, 3, 4, 5, 6, 7], np.int32)
CTRLS = np.array([10, 20, 30, 40, 50, 60, 70], np.int32)
SRC = [0, 0, 0, 2, 2, 2, 2]
TRG = [10, 11, 12, 20, 21, 22, 23]


def _check(got, ordinals):
    assert got["found"] == len(ordinals)
    assert got["ordinal"].tolist() == ordinals and got["ordinal"].dtype == np.int64
    np.testing.assert_array_equal(got["score"].view(np.uint64), SCORES[ordinals].view(np.uint64))   # -0.0 keeps its sign
    assert got["src"].tolist() == [SRC[o] for o in ordinals] and got["src"].dtype == np.int32
    assert got["trg"].tolist() == [TRG[o] for o in ordinals] and got["trg"].dtype == np.int32
    assert got["cases"].tolist() == CASES[ordinals].tolist()
    assert got["ctrls"].tolist() == CTRLS[ordinals].tolist()


def test_hits_reference_hand_worked():
    ref = lambda cutoff, shard=None: report.hits_reference(SCORES, CASES, CTRLS, _uids(), cutoff, shard=shard)
    _check(ref(2.5), [2, 0, 6])                   # a tie AT the cut-off: both listed, in ordinal order
    _check(ref(np.nextafter(2.5, 3.0)), [2])
    _check(ref(0.0), [2, 0, 6, 1, 3])             # -0.0 and +0.0 tie and both reach a cut-off of 0.0: ordinal order
    _check(ref(-0.0), [2, 0, 6, 1, 3])            # ... and of -0.0
    _check(ref(NINF), [2, 0, 6, 1, 3])            # every score above -inf; the -inf score and the NaN never
    _check(ref(7.5), [])
    _check(ref(float("inf")), [])
    _check(ref(0.0, shard=(1, 6)), [2, 1, 3])     # a shard: ordinals 1..5 only
    _check(ref(NINF, shard=(3, 7)), [6, 3])
    with pytest.raises(ValueError):
        ref(float("nan"))


def _pvalues(null_max, scores):
    return api.JoinResult(np.asarray(scores, np.float64), *(np.zeros(len(scores), np.int32) for _ in range(4)),
                          np.asarray(null_max, np.float32)).pvalues()


def _probe_scores(null_max):
    nm = np.unique(np.asarray(null_max, np.float32).astype(np.float64))
    return np.concatenate([nm, np.nextafter(nm, np.inf), np.nextafter(nm, -np.inf), [-1.0, 0.0, -0.0, 1e9, NINF, np.inf]])


@pytest.mark.parametrize("what, null_max, alpha, m, cutoff", [
    # ten maxima, tied at 3.0 (three times): descending 9 7 5 3 3 3 2 2 1 0.5
    ("m = 0: nothing below 1/K", [3, 9, 3, 2, 7, 3, 1, 5, 2, 0.5], 0.05, 0, np.nextafter(9.0, np.inf)),
    ("m = 2", [3, 9, 3, 2, 7, 3, 1, 5, 2, 0.5], 0.2, 2, np.nextafter(5.0, np.inf)),
    ("m = 3: nm[3] is the first of the tie", [3, 9, 3, 2, 7, 3, 1, 5, 2, 0.5], 0.3, 3, np.nextafter(3.0, np.inf)),
    ("m = 4: inside the tie, the same cut-off", [3, 9, 3, 2, 7, 3, 1, 5, 2, 0.5], 0.4, 4, np.nextafter(3.0, np.inf)),
    ("m = 5: the last of the tie", [3, 9, 3, 2, 7, 3, 1, 5, 2, 0.5], 0.5, 5, np.nextafter(3.0, np.inf)),
    ("m = 6: past the tie", [3, 9, 3, 2, 7, 3, 1, 5, 2, 0.5], 0.6, 6, np.nextafter(2.0, np.inf)),
    ("m = K", [3, 9, 3, 2, 7, 3, 1, 5, 2, 0.5], 1.0, 10, NINF),
    ("alpha above 1", [3, 9, 3, 2, 7, 3, 1, 5, 2, 0.5], 1.5, 10, NINF),
    # a hundred maxima 1..100: 29 / 100 <= 0.29 holds, floor(0.29 * 100) is 28
    ("n / K against floor(alpha K)", np.arange(1, 101), 0.29, 29, np.nextafter(71.0, np.inf)),
    # f32 maxima: the cut-off is a double just above the f32 value
    ("f32 rounding", [np.float32(0.1), np.float32(0.3)], 0.5, 1, np.nextafter(float(np.float32(0.1)), np.inf)),
])
def test_significance_cutoff_hand_worked(what, null_max, alpha, m, cutoff):
    K = len(null_max)
    assert m == max(n for n in range(K + 1) if n / K <= alpha), what
    if what.startswith("n / K"):
        assert int(np.floor(alpha * K)) != m                   # the case bites
    got = report.significance_cutoff(null_max, alpha)
    assert got == cutoff, what
    s = _probe_scores(null_max)
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(s >= got, _pvalues(null_max, s) <= alpha, err_msg=what)
    # the smallest such double: one step below it the two filters part
    if np.isfinite(got):
        below = np.nextafter(got, -np.inf)
        assert _pvalues(null_max, [below])[0] > alpha, what


def test_significance_cutoff_refuses_what_has_no_answer():
    with pytest.raises(ValueError, match="0 permutations"):
        report.significance_cutoff(np.zeros(0, np.float32), 0.05)
    with pytest.raises(ValueError, match="NaN"):
        report.significance_cutoff([1.0, 2.0], float("nan"))


def test_hit_gene_counts_hand_worked():
    genes0 = np.array([[0, 1, 2], [2, 2, 3], [4, -1, -1]], np.int32)      # by src
    genes1 = np.array([[1], [5], [2], [-1]], np.int32)                    # by trg
    hits = {"src": np.array([0, 0, 1, 1, 2, 2], np.int32), "trg": np.array([0, 1, 2, 3, 3, 1], np.int32)}
    # paths: {0,1,2} (slot 1 twice: once) | {0,1,2,5} | {2,3} (slot 2 three times) | {2,3} | {4} | {4,5}
    want = [2, 2, 4, 2, 2, 2, 0]
    assert report.hit_gene_counts(hits, genes0, genes1, 7).tolist() == want
    h = api.Hits(6, 6, True, np.zeros(6), np.arange(6), hits["src"], hits["trg"], np.zeros(6, np.int32), np.zeros(6, np.int32))
    assert report.hit_gene_counts(h, genes0, genes1, 7).tolist() == want
    assert report.hit_gene_counts(h, None, genes1, 7).tolist() == [0, 1, 1, 0, 0, 2, 0]
    assert report.hit_gene_counts(h, None, None, 3).tolist() == [0, 0, 0]
    empty = {"src": np.zeros(0, np.int32), "trg": np.zeros(0, np.int32)}
    assert report.hit_gene_counts(empty, genes0, genes1, 7).tolist() == [0] * 7
    with pytest.raises(ValueError, match="outside"):
        report.hit_gene_counts(hits, genes0, genes1, 5)


def test_hits_as_join_result_is_a_top_k_list():
    h = api.Hits(3, 9, True, np.array([7.0, 2.5, 2.5]), np.array([2, 0, 6]), np.array([0, 0, 2], np.int32),
                 np.array([12, 10, 23], np.int32), np.array([3, 1, 7], np.int32), np.array([30, 10, 70], np.int32))
    r = h.as_join_result(np.array([1.0, 3.0, 8.0, 2.5], np.float32))
    assert r.scores.tolist() == [2.5, 2.5, 7.0]               # ascending, as a top-k list
    assert r.src.tolist() == [2, 0, 0] and r.trg.tolist() == [23, 10, 12]
    assert r.pvalues().tolist() == [0.75, 0.75, 0.25]
    assert r.as_r_list()["ids"].tolist() == [[3, 24], [1, 11], [1, 13]]


def test_interface_is_declared():
    names = ["gcre_hits_create", "gcre_join_set_hits", "gcre_process_paths_set_hits", "gcre_hits_count", "gcre_hits_read",
             "gcre_hits_reset", "gcre_hits_free", "gcre_hits_launches"]
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "gcre_hip.h")).read()
    for nm in names:
        assert nm in api.EXPORTS and nm + "(" in header
        assert nm in api._FEATURES["hits"][3]
    assert "#define GCRE_ABI_VERSION 4" in header           # additions only
    assert api.HITS_CAP_MAX == 1 << 26
    assert callable(api.HitList) and callable(report.hits_reference) and callable(report.significance_cutoff)
    assert callable(report.hit_gene_counts)
    lib = api.load_library()                                 # dlopen needs no device
    for nm in names:
        assert hasattr(lib, nm), nm


def test_process_paths_refuses_hits_without_a_context():
    with pytest.raises(api.GcreError, match="exec_"):
        api.process_paths(None, hits={"4": object()})


@pytest.mark.parametrize("kw, match", [
    (dict(significant=0.0), "significant"), (dict(significant=1.0), "significant"), (dict(significant=-0.1), "significant"),
    (dict(significant=1.5), "significant"), (dict(significant=float("nan")), "significant"),
    (dict(significant=0.05, n_permutations=0), "n_permutations"),
    (dict(significant=0.05, significant_cap=0), "significant_cap"),
    (dict(significant=0.05, significant_cap=(1 << 26) + 1), "significant_cap"),
])
def test_gwaspa_refuses_before_anything_runs(kw, match):
    args = dict(n_permutations=100)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        # (no gene, no network: the refusal comes before either is looked at, and before a device is asked for)
        report.gwaspa([], np.zeros((0, 20), np.int32), 10, 10, None, **args)
