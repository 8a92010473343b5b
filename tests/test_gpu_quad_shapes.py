"""The shapes at which the quad kernel's per-quad decisions can go wrong (gcre_ieq.hip): the loop instance a quad takes
(keep-only, one segment, two segments), the peeled last positions of the filter pass, the two ways an added row's planes
are addressed, the prologue's long-recipe loop and the plane counts -- against the CPU oracle, every level, bit for bit.

A level-3 uid is an edge a->b joined with the targets of b, a level-4 uid a walk a->b->c joined with the 2-paths from c:
the uids that end in one pivot gene form its quads, as many segments as walks end in it, as many positions as it has
out-edges.  The networks below plant pivots with chosen in- and out-degrees into a small random network.

Every GPU case forces the quad form, switches the warm-up slice off, so that all of a join goes through the pruned
quad kernel, and lets no kept join store count planes (GCRE_PLANES_OUT_MAX_MB=0).  A join that writes planes stays on
k_null_ie_m1, so only then does level 3 run the quad kernel (on the stored planes of level 2's operand: REC = false), and
level 4 finds its paths0 rows as level 3's recipe alone: REC = true, the instance the benchmark spends its time in.  Every
case asserts that at least two joins ran the quad form -- levels 3 and 4; level 2's uids are the genes themselves, one per
pivot -- and that something was looked up.  What keeps a case meaningful is the oracle:
test_inputs_score_at_every_level checks on the CPU that every input yields top_k scored paths at each level."""
import numpy as np
import pytest

import oracle
from geneticscre_amd import api, dist
from geneticscre_amd.synth import Problem, case_or_control, make_problem, signed_network, values_table, variant_matrix
from geneticscre_amd.uids import build_level_tables
from helpers import assert_same_result, small_table

NC, NT = 300, 330
LEVELS = (("1b", "lst1"), ("2", "lst2"), ("3", "lst3"), ("4", "lst4"))
OUT_EDGES = (1, 2, 3, 64, 65)


def pivot_problem(n_out, n_perm, seed, dense_genes=0):
    """~70 genes, 630 patients, path length 4.  The last three genes become pivots with 1, 2 and 3 in-edges and ``n_out``
    out-edges each: level-3 quads of one segment, of two, and a two plus a one, all of length n_out (a segment holds at
    most 64 paths: 65 out-edges cut it at 64).  ``dense_genes``: that many genes are carried by 30 % of the patients."""
    rng = np.random.default_rng(seed)
    g, src, trg, _ = signed_network(70, 230, rng)
    assert g >= 68, g           # 65 out-edges go to 65 genes that are not pivots
    pivots = [g - 1, g - 2, g - 3]
    pairs = {(int(s), int(t)) for s, t in zip(src, trg) if s not in pivots and t not in pivots}
    others = np.arange(g - 3)
    for n_in, p in zip((1, 2, 3), pivots):
        for s in rng.choice(others, size=n_in, replace=False):
            pairs.add((int(s), p))
        for t in rng.permutation(others)[:n_out]:
            pairs.add((p, int(t)))
    used = {x for e in pairs for x in e}
    for x in range(g):             # every gene occurs in a relation (no new edge touches a pivot)
        if x not in used:
            pairs.add((x, int(others[(x + 1) % len(others)])))
    pairs = np.array(sorted(pairs), dtype=np.int32)
    in_deg = np.bincount(pairs[:, 1], minlength=g)
    out_deg = np.bincount(pairs[:, 0], minlength=g)
    for n_in, p in zip((1, 2, 3), pivots):
        assert in_deg[p] == n_in and out_deg[p] == n_out, (p, in_deg[p], out_deg[p])
    sign = np.where(rng.random(len(pairs)) < 0.7, 1, -1).astype(np.int32)
    levels = build_level_tables(g, pairs[:, 0], pairs[:, 1], sign)
    data1 = variant_matrix(g, NC + NT, rng, 0.05)
    if dense_genes:
        rows = rng.choice(g, size=dense_genes, replace=False)
        data1[rows] = (rng.random((dense_genes, NC + NT)) < 0.30).astype(np.int32)
    data2 = data1[levels.uids["1b"].src]
    perms = case_or_control(NC, NT, n_perm, rng)
    return Problem("method1", NC, NT, 4, 12, n_perm, levels, data1, data2, values_table(NC, NT), perms, seed)


def dense_problem():
    """2,600 patients, every gene carried by 45 % of them: the rows of level 3 carry more than 2,048 -- 12 counter
    planes (the geometry of test_wide_counters_and_dense_rows at a cohort that reaches them)."""
    n = 2600
    nc = n // 2 - 37
    p = make_problem(24, 55, nc, n - nc, 130, 4, method="method1", top_k=9, seed=21, threshold=0.9, table=small_table(nc, n - nc, 4))
    rng = np.random.default_rng(6)
    p.data1 = (rng.random(p.data1.shape) < 0.45).astype(np.int32)
    p.data2 = p.data1[p.levels.uids["1b"].src]
    return p


INPUTS = {f"out{n}": (lambda n=n: pivot_problem(n, 40, 100 + n)) for n in OUT_EDGES}
INPUTS["tiles"] = lambda: pivot_problem(3, 2049, 7)
INPUTS["long_recipe"] = lambda: pivot_problem(3, 40, 9, dense_genes=6)
INPUTS["planes12"] = dense_problem
_CACHE: dict = {}


def case(name):
    """(problem, the oracle's results): computed once per session and shared."""
    if name not in _CACHE:
        p = INPUTS[name]()
        _CACHE[name] = (p, oracle.process_paths(p, order="canonical", nthreads=8))
    return _CACHE[name]


def force_quad(monkeypatch):
    monkeypatch.setenv("GCRE_NULL_KERNEL", "ie")
    monkeypatch.setenv("GCRE_IE_QUAD", "2")
    monkeypatch.setenv("GCRE_IE_WARM", "0")
    monkeypatch.setenv("GCRE_PLANES_OUT_MAX_MB", "0")


def run_plan(p, rank=0, world=1):
    plan = api.ResidentPlan(p, device=0)
    try:
        out = plan.run(rank=rank, world=world) if world > 1 else plan.run()
        prof = dict(plan.last_profile)
    finally:
        plan.close()
    return out, prof


def check(got, prof, want):
    for name, lst in LEVELS:
        assert_same_result(got[name], want[lst])
    assert prof["ie_quad_launches"] >= 2, prof      # level 3 (stored planes) and level 4 (recipe)
    assert prof["ie_lookup_tiles"] > 0, prof


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_inputs_score_at_every_level(name):
    """CPU only: every constructed input runs through the oracle and every level has top_k scored paths."""
    p, want = case(name)
    for _, lst in LEVELS:
        assert len(want[lst].scores) == p.top_k, (lst, len(want[lst].scores))
        assert np.isfinite(want[lst].scores).all() and (want[lst].all_scores > 0).sum() >= p.top_k, lst
        assert len(want[lst].null) == p.iterations
    if name == "planes12":
        most = int(np.unpackbits(want["paths3"].view(np.uint8), axis=1).sum(axis=1).max())
        assert 2048 <= most < 4096, most
    if name == "long_recipe":
        # the join that produces a level-3 row a->b->c lists the carriers that c shares with the row of a->b: some walk
        # shares several blocks of 8
        r3, d = p.levels.rels3, p.data1.astype(bool)
        shared = ((d[r3["srcuid"]] | d[r3["trguid"]]) & d[r3["trguid2"]]).sum(axis=1)
        assert int(shared.max()) > 24, int(shared.max())


@pytest.mark.gpu
@pytest.mark.parametrize("n_out", OUT_EDGES)
def test_quad_sizes_and_peeled_positions(n_out, monkeypatch):
    """Quads of one and of two segments with 1, 2, 3, 64 and 65 positions: the peeled-only case, the peeled pair, one
    round of the loop plus the odd last position, full lanes, and the cut at 64.  K = 40: one tile, partly live."""
    force_quad(monkeypatch)
    p, want = case(f"out{n_out}")
    check(*run_plan(p), want)


@pytest.mark.gpu
def test_two_tiles_one_live_permutation(monkeypatch):
    """K = 2049: two tiles, the second with one live permutation; the per-tile descriptors change under the waves."""
    force_quad(monkeypatch)
    p, want = case("tiles")
    check(*run_plan(p), want)


@pytest.mark.gpu
def test_sharded_plan_of_three_ranks(monkeypatch):
    """Three ranks: every rank scores its shard of levels 3 and 4 on the quad kernel, from a range of level 3's recipe;
    the merged results are the oracle's.  (The kernel's branch for quads of another shard's rows is not reached here,
    nor by any launch the host makes today: segments outside the scored range exist only for rows that get count planes,
    and a join that writes planes does not take the quad form.)"""
    force_quad(monkeypatch)
    p, want = case("out3")
    parts = []
    for rank in range(3):
        got, prof = run_plan(p, rank, 3)
        assert prof["ie_quad_launches"] >= 2 and prof["ie_lookup_tiles"] > 0, prof
        parts.append(got)
    for name, lst in (("3", "lst3"), ("4", "lst4")):
        null = np.maximum.reduce([r[name].null for r in parts])
        rows = [np.stack([r[name].scores, r[name].src, r[name].trg, r[name].cases, r[name].ctrls], axis=1) for r in parts]
        best = dist.merge_topk(np.vstack(rows), p.top_k)
        np.testing.assert_array_equal(null.view(np.uint32), want[lst].null.view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(best[:, 0], want[lst].scores, err_msg=name)


@pytest.mark.gpu
def test_wide_offsets_match_narrow_bit_for_bit(monkeypatch):
    """GCRE_IE_ZWIDE=1 forces the road of a tile of added rows' planes past 4 GiB (a descriptor per row) on a small
    problem: the oracle's results, and the narrow road's bit for bit."""
    force_quad(monkeypatch)
    p, want = case("tiles")
    narrow, prof_n = run_plan(p)
    monkeypatch.setenv("GCRE_IE_ZWIDE", "1")
    wide, prof_w = run_plan(p)
    check(narrow, prof_n, want)
    check(wide, prof_w, want)
    for name, _ in LEVELS:
        for f in ("scores", "null", "cases", "ctrls", "src", "trg"):
            a, b = getattr(narrow[name], f), getattr(wide[name], f)
            assert a.tobytes() == b.tobytes(), (name, f)


@pytest.mark.gpu
def test_long_recipe_lists(monkeypatch):
    """Six genes at 30 % carriers: producing joins whose overlap list has more than 8 entries (the prologue's loop over
    the rest of a recipe's list) and delta lists."""
    force_quad(monkeypatch)
    p, want = case("long_recipe")
    check(*run_plan(p), want)


@pytest.mark.gpu
def test_twelve_counter_planes(monkeypatch):
    force_quad(monkeypatch)
    p, want = case("planes12")
    check(*run_plan(p), want)
