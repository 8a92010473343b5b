"""The pruned null kernels read their launch arguments from the kernarg segment where they use them, through a pointer
the compiler cannot see through (ie_args, gcre_ie_common.h), instead of keeping every field in a scalar register from
kernel entry.  A field that is stale after a loop renewed the pointer, or read at a wrong offset, shows only on the road
that uses it -- so every road that reads an argument late is driven here, each against the CPU oracle, every level, bit
for bit (pytest -m gpu):

  the tile change, the flush and the last partial tile (2,049 and 4,100 permutations: two and three tiles);
  the last level from a recipe (GCRE_PLANES_OUT_MAX_MB=0) and from stored planes (a large limit);
  the wide road of the added rows' planes (GCRE_IE_ZWIDE=1);
  the flag queue and the second look it replaced (GCRE_IE_FLAGQ=1 / 0);
  thresholds that do not come from the maxima (GCRE_IE_PRUNE=0: ladder mode 2, everything is looked up);
  overlap lists of more than 8 entries at 5 % carriers on 160 patients (the recipe's overflow words, the second look of
  a long list, the exact pass);
  a two-shard run (a table with segments this rank does not score);
  the default knobs: levels 1-2 on k_null_ie_m1 and the warm-up slices on k_null_ie<1,L>, the kernels that got the
  same treatment;
  method 2 at path length 5 (k_null_ie_m2, same treatment), with stored planes and from recipes.

The network has 300 genes and 1,000 relations, path length 4.  test_inputs_reach_every_level checks on the CPU that every
input has top_k scorable paths and non-zero null maxima at each level, and that the dense input has the long lists."""
import numpy as np
import pytest

import oracle
from geneticscre_amd import api, dist
from geneticscre_amd.synth import make_problem
from helpers import assert_same_result

LEVELS = (("1b", "lst1"), ("2", "lst2"), ("3", "lst3"), ("4", "lst4"))
GENES, EDGES, NC, NT, TOP_K = 300, 1000, 450, 550, 25
DENSE_N = 160
_CACHE: dict = {}


def dense_problem():
    """160 patients, every gene carried by about 5 % of them (drawn, not capped).  A level-4 join adds the 2-paths c->d->e
    to the walks a->b->c: both operands hold gene c, so the overlap list has c's carriers and more."""
    p = make_problem(GENES, EDGES, DENSE_N // 2 - 6, DENSE_N // 2 + 6, 2049, 4, method="method1", top_k=TOP_K, seed=3)
    rng = np.random.default_rng(4)
    p.data1 = (rng.random(p.data1.shape) < 0.05).astype(np.int32)
    for g in np.flatnonzero(p.data1.sum(axis=1) == 0):
        p.data1[g, rng.integers(DENSE_N)] = 1
    p.data2 = p.data1[p.levels.uids["1b"].src]
    return p


INPUTS = {
    "k2049": lambda: make_problem(GENES, EDGES, NC, NT, 2049, 4, method="method1", top_k=TOP_K, seed=2049),
    "k4100": lambda: make_problem(GENES, EDGES, NC, NT, 4100, 4, method="method1", top_k=TOP_K, seed=4100),
    "dense": dense_problem,
    "m2len5": lambda: make_problem(GENES, EDGES, NC, NT, 2049, 5, method="method2", top_k=TOP_K, seed=2049),
}


def case(name):
    """(problem, the oracle's results): computed once per session, shared by every knob of the input, never changed."""
    if name not in _CACHE:
        p = INPUTS[name]()
        _CACHE[name] = (p, oracle.process_paths(p, order="canonical", nthreads=8))
    return _CACHE[name]


def force_quad(monkeypatch, **env):
    """The quad form on every join that can take it, no warm-up slice: the whole join goes through k_null_ie_q."""
    monkeypatch.setenv("GCRE_NULL_KERNEL", "ie")
    monkeypatch.setenv("GCRE_IE_QUAD", "2")
    monkeypatch.setenv("GCRE_IE_WARM", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def run_plan(p, rank=0, world=1):
    plan = api.ResidentPlan(p, device=0)
    try:
        out = plan.run(rank=rank, world=world) if world > 1 else plan.run()
        prof = dict(plan.last_profile)
    finally:
        plan.close()
    return out, prof


def check(got, prof, want, quad_launches=1):
    for name, lst in LEVELS:
        assert_same_result(got[name], want[lst])
    assert prof["ie_quad_launches"] >= quad_launches, prof
    assert prof["ie_lookup_tiles"] > 0, prof


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_inputs_reach_every_level(name):
    """CPU only: top_k scored paths and non-zero null maxima at every level of every input."""
    p, want = case(name)
    for lst in [f"lst{l}" for l in range(1, p.path_length + 1)]:
        assert len(want[lst].scores) == p.top_k, (lst, len(want[lst].scores))
        assert np.isfinite(want[lst].scores).all() and (want[lst].all_scores > 0).sum() >= p.top_k, lst
        assert len(want[lst].null) == p.iterations and (want[lst].null > 0).all(), lst
    if name == "dense":
        d, r3, u4 = p.data1.astype(bool), p.levels.rels3, p.levels.uids["4"]
        # the join that produces the level-3 row a->b->c lists what c shares with a|b: the recipe's overflow
        shared3 = ((d[r3["srcuid"]] | d[r3["trguid"]]) & d[r3["trguid2"]]).sum(axis=1)
        assert int(shared3.max()) > 8, int(shared3.max())
        # level 4: walk a->b->c with a 2-path from c; the pivot's own carriers are shared by construction
        rows3 = d[r3["srcuid"]] | d[r3["trguid"]] | d[r3["trguid2"]]
        pivot = d[r3["trguid2"]].sum(axis=1)
        live = np.asarray(u4.count) > 0
        assert int(pivot[live].max()) > 8 and int(rows3.sum(axis=1).max()) < 128, (int(pivot[live].max()), int(rows3.sum(axis=1).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("planes_mb", ["0", "4096"])
@pytest.mark.parametrize("name", ["k2049", "k4100"])
def test_tiles_with_and_without_a_recipe(name, planes_mb, monkeypatch):
    """Two tiles with one live permutation in the second, three with four in the third.  No stored planes: level 3 runs the
    quad kernel on level 2's planes and level 4 from level 3's recipe; stored planes: level 4 reads level 3's."""
    force_quad(monkeypatch, GCRE_PLANES_OUT_MAX_MB=planes_mb)
    p, want = case(name)
    check(*run_plan(p), want, quad_launches=2 if planes_mb == "0" else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("planes_mb", ["0", "4096"])
def test_wide_road(planes_mb, monkeypatch):
    force_quad(monkeypatch, GCRE_PLANES_OUT_MAX_MB=planes_mb, GCRE_IE_ZWIDE="1")
    p, want = case("k2049")
    check(*run_plan(p), want)


@pytest.mark.gpu
@pytest.mark.parametrize("warm", ["0", "64"])
@pytest.mark.parametrize("road", ["1", "0"])
def test_flag_queue_and_second_look(road, warm, monkeypatch):
    force_quad(monkeypatch, GCRE_PLANES_OUT_MAX_MB="0", GCRE_IE_FLAGQ=road, GCRE_IE_WARM=warm)
    p, want = case("k4100")
    check(*run_plan(p), want)


@pytest.mark.gpu
@pytest.mark.parametrize("planes_mb", ["0", "4096"])
def test_ladder_mode_2(planes_mb, monkeypatch):
    force_quad(monkeypatch, GCRE_PLANES_OUT_MAX_MB=planes_mb, GCRE_IE_PRUNE="0")
    p, want = case("k2049")
    check(*run_plan(p), want)


@pytest.mark.gpu
@pytest.mark.parametrize("road", ["1", "0"])
@pytest.mark.parametrize("planes_mb", ["0", "4096"])
def test_long_lists(planes_mb, road, monkeypatch):
    force_quad(monkeypatch, GCRE_PLANES_OUT_MAX_MB=planes_mb, GCRE_IE_FLAGQ=road)
    p, want = case("dense")
    check(*run_plan(p), want)


@pytest.mark.gpu
def test_two_shards(monkeypatch):
    """Each rank scores its half of levels 3 and 4; maxima and top-k tables merged are the oracle's."""
    force_quad(monkeypatch, GCRE_PLANES_OUT_MAX_MB="0")
    p, want = case("k2049")
    parts = []
    for rank in range(2):
        got, prof = run_plan(p, rank, 2)
        assert prof["ie_quad_launches"] >= 2 and prof["ie_lookup_tiles"] > 0, prof
        parts.append(got)
    for name, lst in (("3", "lst3"), ("4", "lst4")):
        null = np.maximum.reduce([r[name].null for r in parts])
        rows = [np.stack([r[name].scores, r[name].src, r[name].trg, r[name].cases, r[name].ctrls], axis=1) for r in parts]
        best = dist.merge_topk(np.vstack(rows), p.top_k)
        np.testing.assert_array_equal(null.view(np.uint32), want[lst].null.view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(best[:, 0], want[lst].scores, err_msg=name)


@pytest.mark.gpu
@pytest.mark.parametrize("planes_mb", ["", "0"])
@pytest.mark.parametrize("name", ["k4100", "dense"])
def test_default_knobs(name, planes_mb, monkeypatch):
    """What a caller gets: k_null_ie_m1 on the levels that keep rows, warm-up slices on k_null_ie<1,L>, the quad form on
    the last level."""
    monkeypatch.setenv("GCRE_NULL_KERNEL", "ie")
    if planes_mb:
        monkeypatch.setenv("GCRE_PLANES_OUT_MAX_MB", planes_mb)
    p, want = case(name)
    got, prof = run_plan(p)
    for lvl, lst in LEVELS:
        assert_same_result(got[lvl], want[lst])
    assert prof["ie_lookup_tiles"] > 0, prof


@pytest.mark.gpu
@pytest.mark.parametrize("warm", ["0", ""])
@pytest.mark.parametrize("planes_mb", ["0", "4096"])
def test_method2_length5(planes_mb, warm, monkeypatch):
    """The signed method's pruned kernel on every level of a length-5 pass; warm = 0: no slice of a join is left to the
    general kernel."""
    monkeypatch.setenv("GCRE_NULL_KERNEL", "ie")
    monkeypatch.setenv("GCRE_PLANES_OUT_MAX_MB", planes_mb)
    if warm:
        monkeypatch.setenv("GCRE_IE_WARM", warm)
    p, want = case("m2len5")
    got, prof = run_plan(p)
    for lvl, lst in LEVELS + (("5", "lst5"),):
        assert_same_result(got[lvl], want[lst])
    assert prof["ie_lookup_tiles"] > 0, prof
