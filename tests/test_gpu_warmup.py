"""The general inclusion-exclusion kernel k_null_ie<M,L> (gcre_ie.hip) in its four uses: the warm-up slice of a pruned
launch, whole small joins, the plane output of kept joins and shards.  The four waves of a block share a tile, and their
running maxima leave LDS in ONE merged flush per (block, tile): a barrier, the four arrays combined, the global value
read first, atomicMax only where the block's value is larger.  Every case is compared with the CPU oracle,
level by level, bit for bit (pytest -m gpu).

What can go wrong, case by case: a block's walk over several tiles and its flush per tile; waves with no segment that
must still reach the barrier; a slot the merged flush or the mapping skips (poisoned buffers show it as 0x5A); the
recipe base; long and delta lists inside the slice; shard borders inside segments; the slice-size and items knobs."""
import numpy as np
import pytest

import oracle
from geneticscre_amd import api, dist
from geneticscre_amd.synth import make_problem
from helpers import assert_same_result

pytestmark = pytest.mark.gpu

LEVELS = {"1b": "lst1", "2": "lst2", "3": "lst3", "4": "lst4", "5": "lst5"}
_CACHE: dict = {}


def cached(name, make):
    """(problem, the oracle's results): computed once per session, shared by the cases that use the problem."""
    if name not in _CACHE:
        p = make()
        _CACHE[name] = (p, oracle.process_paths(p, order="canonical", nthreads=8))
    return _CACHE[name]


def run_plan(p, rank=0, world=1):
    plan = api.ResidentPlan(p, device=0)
    try:
        out = plan.run(rank, world)
        prof = dict(plan.last_profile)
    finally:
        plan.close()
    return out, prof


def set_env(monkeypatch, warm="64", **env):
    monkeypatch.setenv("GCRE_NULL_KERNEL", "ie")
    monkeypatch.setenv("GCRE_IE_WARM", warm)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def check_levels(got, want):
    for name, lst in LEVELS.items():
        if name in got:
            assert_same_result(got[name], want[lst])


def tiles_problem(n_perm, method="method1"):
    return cached(("tiles", n_perm, method),
                  lambda: make_problem(120, 700, 450, 550, n_perm, 4, method=method, top_k=25, seed=400 + n_perm))


@pytest.mark.parametrize("n_perm", [2049, 4096, 6200, 10300])
def test_tiles(n_perm, monkeypatch):
    """One live permutation in the last tile; two full tiles; four and six tiles (6200 and 10300 permutations), more than
    the smallest launches have blocks per XCD: a block walks several tiles and flushes once for each."""
    set_env(monkeypatch)
    p, want = tiles_problem(n_perm)
    got, prof = run_plan(p)
    check_levels(got, want)
    assert prof["ie_launches"] > 0, prof


def test_idle_waves_reach_the_barrier(monkeypatch):
    """Joins with fewer scored segments than the launch has waves, and with fewer than four: waves without a segment in a
    tile still take part in the block's flush.  The run must end, and must be right."""
    set_env(monkeypatch)
    p, want = cached("idle", lambda: make_problem(40, 90, 70, 80, 4100, 3, method="method1", top_k=10, seed=11))
    got, _ = run_plan(p)
    check_levels(got, want)


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_whole_joins_in_the_general_kernel(method, monkeypatch):
    """GCRE_IE_PRUNE=0: every join runs whole in k_null_ie<M,L>; method 2 is k_null_ie<2,L>."""
    set_env(monkeypatch, GCRE_IE_PRUNE="0")
    p, want = tiles_problem(2500, method)
    got, _ = run_plan(p)
    check_levels(got, want)


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_plane_output_of_a_kept_joins_slice(method, monkeypatch):
    """Poisoned buffers: levels 3 and 4 read the count planes that the warm-up slices (and the pruned kernels) of levels 1
    to 2 wrote; a plane slot that no wave wrote reads 0x5A5A5A5A and changes the maxima."""
    set_env(monkeypatch, GCRE_POISON="1")
    p, want = tiles_problem(2500, method)
    got, _ = run_plan(p)
    check_levels(got, want)


@pytest.mark.parametrize("ahead", ["1", "0"])
@pytest.mark.parametrize("length", [4, 5])
def test_recipe_base(length, ahead, monkeypatch):
    """No stored planes of kept joins: the base counters of a segment are rebuilt from the recipe of the join that made
    its row, in the slice as in the pruned kernel (which reads the gathered recipe entries of its segments)."""
    set_env(monkeypatch, GCRE_PLANES_OUT_MAX_MB="0", GCRE_AHEAD=ahead)
    if length == 4:
        p, want = tiles_problem(2500)
    else:
        p, want = cached("len5", lambda: make_problem(60, 260, 150, 170, 2300, 5, method="method1", top_k=12, seed=21))
    got, _ = run_plan(p)
    check_levels(got, want)


def dense_problem(top_rate):
    rng = np.random.default_rng(3)
    p = make_problem(70, 420, 260, 250, 2100, 4, method="method1", top_k=15, seed=9)
    dense = (rng.random(p.data1.shape) < rng.uniform(0.02, top_rate, size=(p.data1.shape[0], 1))).astype(np.int32)
    p.data1[:] = dense
    p.data2[:] = dense[p.levels.uids["1b"].src]
    return p


def test_long_and_delta_lists_in_the_slice(monkeypatch):
    """Carrier rates up to 25 %: lists longer than 8 entries and delta lists among the slice's paths."""
    set_env(monkeypatch)
    p, want = cached("dense", lambda: dense_problem(0.25))
    got, _ = run_plan(p)
    check_levels(got, want)


def test_shards(monkeypatch):
    """Three shards on one device: borders fall inside segments, paths of another shard only give planes.  The
    element-wise maximum of the three null vectors and the merged top-k are the oracle's."""
    set_env(monkeypatch)
    p, want = tiles_problem(2500)
    plan = api.ResidentPlan(p, device=0)
    try:
        parts = [plan.run(rank, 3) for rank in range(3)]
    finally:
        plan.close()
    for name, lst in LEVELS.items():
        if name not in parts[0]:
            continue
        null = np.maximum.reduce([r[name].null for r in parts])
        rows = [np.stack([r[name].scores, r[name].src, r[name].trg, r[name].cases, r[name].ctrls], axis=1) for r in parts]
        best = dist.merge_topk(np.vstack(rows), p.top_k)
        w = want[lst]
        np.testing.assert_array_equal(null.view(np.uint32), w.null.view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(np.ascontiguousarray(best[:, 0]).view(np.uint64), w.scores.view(np.uint64), err_msg=name)
        np.testing.assert_array_equal(best[:, 1].astype(np.int64), w.src, err_msg=name)
        np.testing.assert_array_equal(best[:, 2].astype(np.int64), w.trg, err_msg=name)


@pytest.mark.parametrize("items", ["1", "4"])
@pytest.mark.parametrize("div", ["1", "1024", "1000000"])
def test_knobs(div, items, monkeypatch):
    """GCRE_IE_WARM_DIV = 1: the slice is as long as its cap lets it be; 1,000,000: the least slice.  GCRE_IE_WARM_ITEMS:
    more and shorter waves, or fewer and longer ones.  Any slice and any split give the same maxima."""
    set_env(monkeypatch, GCRE_IE_WARM_DIV=div, GCRE_IE_WARM_ITEMS=items)
    p, want = tiles_problem(4096)
    got, _ = run_plan(p)
    check_levels(got, want)


def test_seeded_loop(monkeypatch):
    """60 tiny problems: lengths 3-5, 60-400 patients, 100-2,300 permutations, slices of 64 and 1,024 segments, both
    methods.  The sizes bound the time: the largest draw takes the oracle and the GPU together well under 0.2 s."""
    for case in range(60):
        rng = np.random.default_rng(7000 + case)
        genes, edges = int(rng.integers(40, 81)), int(rng.integers(200, 401))
        n = int(rng.integers(60, 401))
        nc = int(rng.integers(n // 3, 2 * n // 3 + 1))
        perms = int(rng.choice([100, 300, 700, 2048, 2049, 2300]))
        length = int(rng.integers(3, 6))
        if length == 5:     # the last level of a length-5 problem is the largest by far
            genes, edges, perms = min(genes, 50), min(edges, 240), min(perms, 700)
        set_env(monkeypatch, warm=("64", "1024")[case % 2])
        p = make_problem(genes, edges, nc, n - nc, perms, length, method=("method1", "method2")[(case // 2) % 2], top_k=8,
                         seed=7000 + case, threshold=float(rng.choice([0.05, 0.1, 0.3])))
        want = oracle.process_paths(p, order="canonical", nthreads=8)
        got, _ = run_plan(p)
        try:
            check_levels(got, want)
        except AssertionError as e:
            raise AssertionError(f"case {case}: {genes} genes, {edges} relations, {nc}+{n - nc} patients, {perms} permutations, "
                                 f"length {length}, {p.method}") from e
