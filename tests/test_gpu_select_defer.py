"""The top-k selection of a join that is inspected ahead (the gcre_join_ahead chain) stays open until the join is launched:
the launch queues the join's null kernels first and closes the selection behind them, and the join's own call unpacks the
winners -- against the CPU oracle, every level, bit for bit, with the chain on and off and with GCRE_SELECT_DEFER=0 (the
ahead inspection closes its selection itself, as it did before).

The selection's scratch is one per context, its stream is one per context: what is open at any time is the selections of
ONE join, a state and a winners' buffer per chunk.  So the cases are the ones where more than one selection is in flight or
where somebody else comes for the chunk: several chunks per chained join, another chained join behind it (path length 5),
two permutation tiles, two ranks' shards, later permutation windows and kept inspections (the winners are then the
cached ones), a broken hint (the chunk is inspected twice), and the observers that read a chunk's keys after the join.

The network is that of test_gpu_warm_sizes.py: about 120 genes, 420 signed relations, 300 + 330 patients; level 4 has
5,535 joined paths, level 5 more.  test_inputs_are_chained_and_chunked checks on the CPU what the GPU tests rely on."""
import re

import numpy as np
import pytest

import oracle
from geneticscre_amd import api, dist, report
from geneticscre_amd.synth import make_problem
from helpers import assert_same_result

NC, NT = 300, 330
LEVELS4 = (("1b", "lst1"), ("2", "lst2"), ("3", "lst3"), ("4", "lst4"))
LEVELS5 = LEVELS4 + (("5", "lst5"),)
CHUNK = 1024

INPUTS = {
    "k40": lambda: make_problem(120, 420, NC, NT, 40, 4, method="method1", top_k=12, seed=3),
    "tiles": lambda: make_problem(120, 420, NC, NT, 2049, 4, method="method1", top_k=12, seed=3),
    "len5": lambda: make_problem(120, 420, NC, NT, 40, 5, method="method1", top_k=12, seed=3),
    "m2_k40": lambda: make_problem(120, 420, NC, NT, 40, 4, method="method2", top_k=12, seed=3),
    "m2_tiles": lambda: make_problem(120, 420, NC, NT, 2049, 4, method="method2", top_k=12, seed=3),
    "m2_len5": lambda: make_problem(120, 420, NC, NT, 40, 5, method="method2", top_k=12, seed=3),
}
_CACHE: dict = {}
# chain on / off x selection left open / closed by the inspection
ROADS = ({"GCRE_AHEAD": "1", "GCRE_SELECT_DEFER": "1"}, {"GCRE_AHEAD": "1", "GCRE_SELECT_DEFER": "0"},
         {"GCRE_AHEAD": "0", "GCRE_SELECT_DEFER": "1"}, {"GCRE_AHEAD": "0", "GCRE_SELECT_DEFER": "0"})


def case(name):
    """(problem, the oracle's results): computed once per session and shared."""
    if name not in _CACHE:
        p = INPUTS[name]()
        _CACHE[name] = (p, oracle.process_paths(p, order="canonical", nthreads=8))
    return _CACHE[name]


def levels_of(p):
    return LEVELS5 if p.path_length == 5 else LEVELS4


def run_plan(p, rank=0, world=1, **kw):
    plan = api.ResidentPlan(p, device=0)
    try:
        out = plan.run(rank=rank, world=world, **kw) if world > 1 else plan.run(**kw)
        prof = dict(plan.last_profile)
    finally:
        plan.close()
    return out, prof


def check(p, got, want):
    for name, lst in levels_of(p):
        assert_same_result(got[name], want[lst])


def same_bytes(a, b, names):
    for name, _ in names:
        for f in ("scores", "null", "cases", "ctrls", "src", "trg"):
            assert getattr(a[name], f).tobytes() == getattr(b[name], f).tobytes(), (name, f)


def on_all_roads(monkeypatch, p, want, **env):
    """The plan once per road, the oracle's results on every one; chained joins replay their ahead inspection."""
    runs = []
    for road in ROADS:
        with monkeypatch.context() as m:
            for k, v in {**road, **env}.items():
                m.setenv(k, str(v))
            got, prof = run_plan(p)
        check(p, got, want)
        if road["GCRE_AHEAD"] == "1":
            assert prof["inspect_replays"] >= len(levels_of(p)), (road, prof)   # every later level was launched from its inspection
        else:
            assert prof["inspect_replays"] == 0, (road, prof)
        runs.append(got)
    for other in runs[1:]:
        same_bytes(runs[0], other, levels_of(p))


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_inputs_are_chained_and_chunked(name):
    """CPU only: every level has top_k scored paths with finite scores; levels 4 and 5 have several chunks of 1,024 joined
    paths; the plan is small enough for the chain to be on by default (ResidentPlan: up to 64 M joined paths and 10^12
    scores per pass); 2,049 permutations are two tiles."""
    p, want = case(name)
    for _, lst in levels_of(p):
        assert len(want[lst].scores) == p.top_k and np.isfinite(want[lst].scores).all(), lst
        assert len(want[lst].null) == p.iterations
    paths = {k: int(np.maximum(np.asarray(p.levels.uids[k].count), 0).sum()) for k, _ in levels_of(p)}
    assert paths["4"] > 4 * CHUNK, paths
    if p.path_length == 5:
        assert paths["5"] > 4 * CHUNK, paths
    total = sum(paths.values())
    assert total <= 64_000_000 and total * p.iterations <= 10 ** 12
    assert p.iterations in (40, 2049) and 2049 > 2048


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_chain_on_and_off_selection_open_and_closed(name, monkeypatch):
    """40 and 2,049 permutations, path lengths 4 and 5, both methods: the four roads give the oracle's results, and
    identical bytes."""
    p, want = case(name)
    on_all_roads(monkeypatch, p, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["k40", "tiles", "len5", "m2_k40"])
def test_several_chunks_per_chained_join(name, monkeypatch):
    """Chunks of 1,024 joined paths: a chained join leaves several selections open at once, each with a state of its own, and
    its launch closes them one after the other on the one selection stream, into the one scratch."""
    p, want = case(name)
    on_all_roads(monkeypatch, p, want, GCRE_CHUNK_PATHS=CHUNK)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, CHUNK])
def test_two_ranks(chunk, monkeypatch):
    """Two ranks' shards of every level, merged as bench.py merges them: the oracle's null maxima and top-k."""
    monkeypatch.setenv("GCRE_AHEAD", "1")
    if chunk:
        monkeypatch.setenv("GCRE_CHUNK_PATHS", str(chunk))
    p, want = case("k40")
    parts = [run_plan(p, rank, 2)[0] for rank in range(2)]
    for name, lst in LEVELS4[1:]:
        null = np.maximum.reduce([r[name].null for r in parts])
        rows = [np.stack([r[name].scores, r[name].src, r[name].trg, r[name].cases, r[name].ctrls], axis=1) for r in parts]
        best = dist.merge_topk(np.vstack(rows), p.top_k)
        np.testing.assert_array_equal(null.view(np.uint32), want[lst].null.view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(best[:, 0], want[lst].scores, err_msg=name)


_SELECT = re.compile(r"^launch k_hist_st ", re.M)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, CHUNK])
def test_kept_inspections_replay_the_cached_winners(chunk, monkeypatch, capfd):
    """Two one-tile windows over 2,049 permutations, inspections kept: the first pass selects once per chunk (in the first
    window; its chained joins' selections are closed by their launches, the winners reach the cache in the joins' own
    calls); the second window and the whole second pass replay -- the oracle's results, and not one selection is launched."""
    monkeypatch.setenv("GCRE_AHEAD", "1")
    monkeypatch.setenv("GCRE_WINDOW_TILES", "1")
    monkeypatch.setenv("GCRE_LAUNCH_TRACE", "1")
    if chunk:
        monkeypatch.setenv("GCRE_CHUNK_PATHS", str(chunk))
    p, want = case("tiles")
    plan = api.ResidentPlan(p, device=0)
    try:
        plan.set_window(2048)
        assert len(plan.windows()) == 2
        capfd.readouterr()
        first = plan.run(keep_inspections=True)
        selections = len(_SELECT.findall(capfd.readouterr().err))
        check(p, first, want)
        chunks = sum(-(-int(plan.uids[k].total_paths) // (chunk or 1 << 25)) for k in plan.names)
        # one per chunk (and one more for a chunk that is inspected twice): a second window that selected again would double it
        assert chunks <= selections < 2 * chunks, (selections, chunks)
        second = plan.run(keep_inspections=True)
        assert len(_SELECT.findall(capfd.readouterr().err)) == 0
        check(p, second, want)
        assert plan.last_profile["inspect_replays"] >= 2 * chunks, plan.last_profile
        assert plan.last_profile["stats_kernel_ms"] == 0
        same_bytes(first, second, LEVELS4)
    finally:
        plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, 256])
@pytest.mark.parametrize("name", ["k40", "m2_k40"])
def test_broken_hint_on_a_chained_join(name, chunk, monkeypatch):
    """A reduced operand that does not describe level 4 (the road of test_wrong_hint_is_detected_and_ignored) on a join of
    the chain: its ahead inspection finds the hint broken and inspects the chunk again on paths1 itself -- the first
    attempt's digit passes are abandoned --, and whichever call scores the join then returns the oracle's top-k."""
    monkeypatch.setenv("GCRE_AHEAD", "1")
    monkeypatch.setenv("GCRE_NULL_KERNEL", "ie")
    if chunk:
        monkeypatch.setenv("GCRE_CHUNK_PATHS", str(chunk))
    p, want = case(name)
    plan = api.ResidentPlan(p, device=0)
    try:
        genes = plan.parsed[0]
        rng = np.random.default_rng(1)
        plan.uids["4"].set_reduced(genes, rng.integers(0, genes.size, plan.kept["2"].size))     # garbage
        seen = {}
        got = plan.run(on_level=lambda name, r, shard, window: (seen.__setitem__(name, plan.ex.profile()), r)[1])
        check(p, got, want)
        assert seen["4"]["ie_hinted_joins"] == 0 and seen["4"]["ie_launches"] > 0, seen["4"]
    finally:
        plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("observer", ["hits", "exceed", "tally"])
def test_observers_on_a_chained_join(observer, monkeypatch):
    """A hit list, exceedance counts or a gene tally armed on level 4, a join of the chain: they read the chunk's keys in the
    join's own call, after the launch has closed the selection -- their CPU references, the oracle's joins, and the same
    with the selection closed by the inspection."""
    from test_gpu_exceed import Cpu, assert_counts
    from test_gpu_genes import assert_tally
    from test_gpu_hits import assert_hits
    p, want = case("k40")
    r4 = want["lst4"]
    tables = report.gene_tables(p.levels, len(p.data1), len(p.data2))
    slots = report.gene_slots("4", len(p.data1), len(p.data2))
    cut = float(r4.scores.min())
    if observer == "exceed":
        if "cpu" not in _CACHE:
            _CACHE["cpu"] = Cpu(p, nthreads=8)
        thr = _CACHE["cpu"].thresholds("4")
    for defer in ("1", "0"):
        monkeypatch.setenv("GCRE_AHEAD", "1")
        monkeypatch.setenv("GCRE_SELECT_DEFER", defer)
        plan = api.ResidentPlan(p, device=0)
        try:
            if observer == "hits":
                obs = api.HitList(plan.ex, cut, cap=1 << 16)
                got = plan.run(hits={"4": obs})
                assert_hits(obs.read(), report.hits_reference(r4.all_scores, r4.all_cases, r4.all_ctrls, p.levels.uids["4"], cut))
            elif observer == "exceed":
                obs = api.ExceedCounts(plan.ex, thr)
                got = plan.run(exceeds={"4": obs})
                assert_counts(obs.read(), _CACHE["cpu"].reference("4", thr))
            else:
                obs = api.GeneTally(plan.ex, slots, *tables["4"])
                got = plan.run(tallies={"4": obs})
                assert_tally(obs.read(), report.gene_best_reference(r4.all_scores, r4.all_cases, r4.all_ctrls, p.levels.uids["4"],
                                                                    *tables["4"], slots))
            assert plan.last_profile["inspect_replays"] >= len(LEVELS4), plan.last_profile
        finally:
            plan.close()
        check(p, got, want)
