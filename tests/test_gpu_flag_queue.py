"""The flag queue of the quad kernel (gcre_ieq.hip): a permutation the bound filter flags is queued with its
count W and scored on its own -- eight mask dwords, one table cell, one maximum -- 64 at a time, instead of sending the
whole path-tile through the exact pass.  Every case runs the queue road (GCRE_IE_FLAGQ=1, the default) and the old road
(0: second look + exact pass) against the CPU oracle, every level, bit for bit (pytest -m gpu).

What must fall back to the exact pass: thresholds still at zero (GCRE_IE_WARM=0: the first quads flag every permutation),
delta lists, lists longer than 8 entries, lanes with more than GCRE_REFINE_MAX flagged permutations (dense genotypes)."""
import numpy as np
import pytest

import oracle
from geneticscre_amd import api
from geneticscre_amd.synth import make_problem
from helpers import assert_same_result, small_table

pytestmark = pytest.mark.gpu

LEVELS = {"1b": "lst1", "2": "lst2", "3": "lst3", "4": "lst4", "5": "lst5"}
ROADS = ("1", "0")
_CACHE: dict = {}


def cached(name, make):
    """(problem, the oracle's results): computed once per session, shared by the roads and knobs of a case."""
    if name not in _CACHE:
        p = make()
        _CACHE[name] = (p, oracle.process_paths(p, order="canonical", nthreads=8))
    return _CACHE[name]


def run_plan(p):
    plan = api.ResidentPlan(p, device=0)
    try:
        out = plan.run()
        prof = dict(plan.last_profile)
    finally:
        plan.close()
    return out, prof


def force_quad(monkeypatch, road, warm="0", **env):
    monkeypatch.setenv("GCRE_NULL_KERNEL", "ie")
    monkeypatch.setenv("GCRE_IE_QUAD", "2")
    monkeypatch.setenv("GCRE_IE_WARM", warm)
    monkeypatch.setenv("GCRE_IE_FLAGQ", road)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def check_levels(got, want):
    for name, lst in LEVELS.items():
        if name in got:
            assert_same_result(got[name], want[lst])


@pytest.mark.parametrize("road", ROADS)
@pytest.mark.parametrize("warm", ["0", "64"])
@pytest.mark.parametrize("n_perm", [2500, 2049, 4096])
def test_two_tiles(n_perm, warm, road, monkeypatch):
    """Two tiles: a short second one (452 live permutations), one with a single live permutation, and two full ones.  The
    queue is emptied before the tile changes: its items address the tile's masks.  warm = 0: the first quads see
    threshold 0, every permutation is flagged and the paths take the exact pass; later ones queue."""
    force_quad(monkeypatch, road, warm)
    p, want = cached(("tiles", n_perm), lambda: make_problem(120, 700, 450, 550, n_perm, 4, method="method1", top_k=25, seed=400 + n_perm))
    got, prof = run_plan(p)
    check_levels(got, want)
    assert prof["ie_quad_launches"] > 0, prof
    assert prof["ie_lookup_tiles"] > 0, prof


def test_the_queue_road_is_taken(monkeypatch):
    """ie_lookup_tiles tells the roads apart.  On the old road it counts the path-tiles whose exact pass looked something
    up; each of those has a permutation outside its interval, which the bound filter flags first.  On the queue road
    every flagged path-tile counts -- when it queues its first item, or in the exact pass as before -- so the count
    is larger: by 5 % on this small problem (33,133 against 31,508 where the test was written; most of its flagged
    path-tiles are looked up on either road), six times at the benchmark's size.  The threshold exchange between waves
    is not deterministic, hence no exact figure.  A library whose
    host glue left the knob at 0 would report the old road's count twice."""
    p, want = cached(("tiles", 2500), lambda: make_problem(120, 700, 450, 550, 2500, 4, method="method1", top_k=25, seed=400 + 2500))
    counts = {}
    for road in ROADS:
        force_quad(monkeypatch, road, "64")
        got, prof = run_plan(p)
        check_levels(got, want)
        counts[road] = prof["ie_lookup_tiles"]
    monkeypatch.delenv("GCRE_IE_FLAGQ")      # the default is the queue road
    _, prof = run_plan(p)
    print("ie_lookup_tiles by road:", counts, "default:", prof["ie_lookup_tiles"])
    assert counts["1"] > counts["0"] > 0, counts
    assert prof["ie_lookup_tiles"] > counts["0"], (prof["ie_lookup_tiles"], counts)


@pytest.mark.parametrize("road", ROADS)
@pytest.mark.parametrize("prune", ["1", "0"])
def test_arbitrary_table(prune, road, monkeypatch):
    """Random cells instead of a valley: narrow intervals flag many permutations, the queue fills and is drained inside a
    quad.  Pruned and unpruned (lad_mode != 0: nothing is queued) give the oracle's maxima."""
    nc, nt = 300, 340
    force_quad(monkeypatch, road, GCRE_IE_PRUNE=prune)
    p, want = cached("table", lambda: make_problem(100, 600, nc, nt, 2300, 4, method="method1", top_k=10, seed=5, table=small_table(nc, nt, 1)))
    got, prof = run_plan(p)
    check_levels(got, want)
    assert prof["ie_quad_launches"] > 0, prof


def dense_problem(top_rate):
    rng = np.random.default_rng(3)
    p = make_problem(70, 420, 260, 250, 2100, 4, method="method1", top_k=15, seed=9)
    dense = (rng.random(p.data1.shape) < rng.uniform(0.02, top_rate, size=(p.data1.shape[0], 1))).astype(np.int32)
    p.data1[:] = dense
    p.data2[:] = dense[p.levels.uids["1b"].src]
    return p


@pytest.mark.parametrize("road", ROADS)
@pytest.mark.parametrize("top_rate", [0.08, 0.25])
def test_dense_rows_fall_back(top_rate, road, monkeypatch):
    """Carrier rates up to 8 % / 25 %: lists longer than 8 entries, delta lists and lanes with many flagged permutations
    all leave the queue road for the exact pass."""
    force_quad(monkeypatch, road)
    p, want = cached(("dense", top_rate), lambda: dense_problem(top_rate))
    got, prof = run_plan(p)
    check_levels(got, want)
    assert prof["ie_quad_launches"] > 0, prof


def carry_problem():
    """5,000 patients, 99 % of them cases; every gene is carried by the same 5 patients and by 83 others drawn at
    random: 88 carriers.  A level-3 row a|b|c then carries at most 5 + 3 * 83 = 254 -- 8 counter planes -- while the two
    operands of its join carry 2 * 88 - 5 - |a & b others| + 88 = 259 minus a Poisson(1.4) number: W = N0 + Nz passes 255
    in the permutations that leave at most three of those carriers controls (a permutation in two, at 1 % controls)."""
    nc, nt = 4950, 50
    p = make_problem(60, 260, nc, nt, 2100, 4, method="method1", top_k=10, seed=31)
    rng = np.random.default_rng(32)
    n = nc + nt
    core = rng.choice(n, size=5, replace=False)
    rest = np.setdiff1d(np.arange(n), core)
    d = np.zeros(p.data1.shape, dtype=np.int32)
    for g in range(d.shape[0]):
        d[g, core] = 1
        d[g, rng.choice(rest, size=83, replace=False)] = 1
    p.data1[:] = d
    p.data2[:] = d[p.levels.uids["1b"].src]
    return p


@pytest.mark.parametrize("road", ROADS)
def test_carry_out_of_the_top_plane(road, monkeypatch):
    """The 8-plane variant with a carry out of plane 7 in W: the carry is part of the queued count (9 bits here).  The
    variant follows from the join's largest carrier total (counter_planes, gcre_host.hip): below 256 at level 3, asserted
    here on the oracle's kept rows; with no stored planes both level 3 and level 4 run the quad kernel."""
    force_quad(monkeypatch, road, GCRE_PLANES_OUT_MAX_MB="0")   # level 3 on the quad kernel too (stored planes of level 2)
    p, want = cached("carry", carry_problem)
    # the totals of level 3's joins, from the oracle's kept rows: walk a -> b -> c joins the level-2 row a|b with gene c
    r3, d = p.levels.rels3, p.data1.astype(bool)
    rows0 = d[r3["srcuid"]] | d[r3["trguid"]]
    rowz = d[r3["trguid2"]]
    tot0, totz, joined = rows0.sum(axis=1), rowz.sum(axis=1), (rows0 | rowz).sum(axis=1)
    kept = np.unpackbits(want["paths3"].view(np.uint8), axis=1).sum(axis=1)
    assert sorted(kept.tolist()) == sorted(joined.tolist())
    assert int(kept.max()) < 256, int(kept.max())
    carry = (tot0 + totz >= 256) & (joined < 256) & (tot0 + totz - joined <= 8)
    assert int(carry.sum()) > 0, (int((tot0 + totz).max()), int(joined.max()))
    got, prof = run_plan(p)
    check_levels(got, want)
    assert prof["ie_quad_launches"] >= 2, prof


def test_seeded_loop(monkeypatch):
    """100 tiny problems on the queue road: lengths 3-5, 60-400 patients, 100-2,300 permutations, with and without a
    warm-up slice.  The sizes are what bounds the time: the largest draw (80 genes, 400 relations, length 4; length 5 is
    cut to 50 genes, 240 relations, 700 permutations) takes the oracle and the GPU together well under 0.2 s, the whole
    loop 3 s where it was written."""
    for case in range(100):
        rng = np.random.default_rng(7000 + case)
        genes, edges = int(rng.integers(40, 81)), int(rng.integers(200, 401))
        n = int(rng.integers(60, 401))
        nc = int(rng.integers(n // 3, 2 * n // 3 + 1))
        perms = int(rng.choice([100, 300, 700, 2048, 2049, 2300]))
        length = int(rng.integers(3, 6))
        if length == 5:     # the last level of a length-5 problem is the largest by far
            genes, edges, perms = min(genes, 50), min(edges, 240), min(perms, 700)
        force_quad(monkeypatch, "1", warm=("0", "64")[case % 2])
        p = make_problem(genes, edges, nc, n - nc, perms, length, method="method1", top_k=8, seed=7000 + case,
                         threshold=float(rng.choice([0.05, 0.1, 0.3])))
        want = oracle.process_paths(p, order="canonical", nthreads=8)
        got, _ = run_plan(p)
        try:
            check_levels(got, want)
        except AssertionError as e:
            raise AssertionError(f"case {case}: {genes} genes, {edges} relations, {nc}+{n - nc} patients, {perms} permutations, length {length}") from e
