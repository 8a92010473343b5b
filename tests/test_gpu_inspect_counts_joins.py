"""Whole joins with the method-1 inspector's counts taken from row totals (GCRE_STATS_IE_COUNTS=1, the default) and counted
word by word (=0), against the oracle: path length 4 and 5 (levels 1 to 3 keep their rows), joins cut into chunks, two ranks,
and the inspect-ahead chain.  The trace says which road ran: k_row_counts is launched on the new one only."""
import numpy as np
import pytest

import oracle
from geneticscre_amd import api, dist
from geneticscre_amd.synth import make_problem
from helpers import assert_same_result

pytestmark = pytest.mark.gpu

LEVELS = (("1b", "lst1"), ("2", "lst2"), ("3", "lst3"), ("4", "lst4"), ("5", "lst5"))
_WANT = {}


def problem(L):
    if L not in _WANT:
        p = make_problem(40, 110, 29, 33, 100, L, method="method1", top_k=15, seed=30 + L, threshold=0.2)
        _WANT[L] = (p, oracle.process_paths(p, order="canonical"))
    return _WANT[L]


@pytest.fixture
def road(request, monkeypatch, capfd):
    """The knob, the inclusion-exclusion form and the trace; road(text) checks which inspector road the trace shows."""
    knob = request.param
    monkeypatch.setenv("GCRE_STATS_IE_COUNTS", str(knob))
    monkeypatch.setenv("GCRE_NULL_KERNEL", "ie")
    monkeypatch.setenv("GCRE_LAUNCH_TRACE", "1")
    capfd.readouterr()

    def check():
        err = capfd.readouterr().err
        assert "launch k_stats_ie2 " in err
        assert ("launch k_row_counts" in err) == (knob == 1), err[-2000:]
    return check


@pytest.mark.parametrize("road", [1, 0], indirect=True)
@pytest.mark.parametrize("chunk", ["0", "1024"])
@pytest.mark.parametrize("L", [4, 5])
def test_joins_match_the_oracle(L, chunk, road, monkeypatch):
    if chunk != "0":
        monkeypatch.setenv("GCRE_CHUNK_PATHS", chunk)
    p, want = problem(L)
    plan = api.ResidentPlan(p)
    try:
        for _ in range(2):           # the second pass rewrites the kept sets: their row totals are built again
            got = plan.run()
            for name, lst in LEVELS[:L]:
                assert_same_result(got[name], want[lst])
    finally:
        plan.close()
    road()


@pytest.mark.parametrize("road", [1, 0], indirect=True)
def test_joins_ahead(road, monkeypatch):
    monkeypatch.setenv("GCRE_AHEAD", "1")
    p, want = problem(5)
    plan = api.ResidentPlan(p)
    try:
        got = plan.run()
        for name, lst in LEVELS:
            assert_same_result(got[name], want[lst])
    finally:
        plan.close()
    road()


@pytest.mark.parametrize("road", [1, 0], indirect=True)
def test_two_ranks(road, monkeypatch):
    monkeypatch.setenv("GCRE_CHUNK_PATHS", "1024")
    p, want = problem(5)
    parts = []
    for rank in range(2):
        plan = api.ResidentPlan(p)
        try:
            parts.append(plan.run(rank=rank, world=2))
        finally:
            plan.close()
    road()
    for name, lst in LEVELS:
        null = np.maximum(parts[0][name].null, parts[1][name].null)
        rows = [np.stack([r[name].scores, r[name].src, r[name].trg, r[name].cases, r[name].ctrls], axis=1) for r in parts]
        best = dist.merge_topk(np.vstack(rows), p.top_k)
        w = want[lst]
        np.testing.assert_array_equal(null.view(np.uint32), w.null.view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(best[:, 0], w.scores, err_msg=name)
        np.testing.assert_array_equal(best[:, 3], w.cases, err_msg=name)
        np.testing.assert_array_equal(best[:, 4], w.ctrls, err_msg=name)
