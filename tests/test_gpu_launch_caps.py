"""Every launcher's grid cap, crossed against the oracle.

Nearly every launcher clamps its grid and lets the kernel walk the rest in a grid-stride loop; some of those loops carry
state from one round to the next (the inspectors' LDS staging and overflow reservations, k_scan_top's carry, k_set_null's
double-buffered mask stream).  The joins here have millions of paths on a narrow cohort (640 patients), which the CPU
oracle runs in about a second, and GCRE_LAUNCH_TRACE=1 makes every launcher say on stderr what it was asked for and what
it launched: every test asserts through that trace that the cap it is named for was crossed, so a changed constant fails
the test instead of silently shrinking it.  What the inputs must be like for that (path counts past each cap, long lists,
null maxima that tell paths apart) is asserted on the oracle's results alone."""
from __future__ import annotations

import contextlib
import dataclasses
import re

import numpy as np
import pytest
import torch

import oracle
from geneticscre_amd import api, report
from geneticscre_amd.synth import make_problem
from helpers import assert_same_result
from test_gpu_configs import LST, MODES, bench, set_mode
from test_gpu_exceed import Cpu
from test_gpu_sets import FIELDS, device_masks, oracle_levels_kept
from test_gpu_stepdown import sets_of, top_rows
from test_sets_host import restate_slabs
from test_stepdown_host import reference_sorted

pytestmark = pytest.mark.gpu

_LAUNCH = re.compile(r"^launch (\S+) want=(\d+) got=(\d+)$", re.M)
_TILES = re.compile(r"^launch (\S+) npt=(\d+) pgroups=(\d+) per=(\d+)$", re.M)


def launches(err):
    """The trace on stderr: kernel -> [(want, got)] of the launchers that clamp a grid."""
    out = {}
    for k, w, g in _LAUNCH.findall(err):
        out.setdefault(k, []).append((int(w), int(g)))
    return out


def set_tiles(err, kernel):
    """[(npt, pgroups, per)] of the launches of k_set_null / k_stepdown_null."""
    return [(int(a), int(b), int(c)) for k, a, b, c in _TILES.findall(err) if k == kernel]


def crossed(tr, kernel):
    """Some launch of the kernel was asked for more blocks (rounds) than it got."""
    return any(w > g for w, g in tr.get(kernel, ()))


def assert_crossed(tr, kernels, what=""):
    for k in kernels:
        assert crossed(tr, k), f"{what}: no launch of {k} went past its cap: {tr.get(k)}"


@pytest.fixture
def trace(monkeypatch, capfd):
    """Switch the trace on for the contexts the test creates; trace() returns the stderr text since the last call."""
    monkeypatch.setenv("GCRE_LAUNCH_TRACE", "1")
    capfd.readouterr()
    return lambda: capfd.readouterr().err


# ---- the two million-path joins ---------------------------------------------------------------------------------------
# (genes, relations) of make_problem(.., 300, 340, 130, 5, top_k=40, seed=1, threshold=0.05, table=fast_table(300, 340)):
# 689,683 / 5,305,862 level-4 / level-5 paths for method 1 and 344,407 / 2,331,263 for method 2; level 3 (the operand set
# of level 5) has 91,237 and 50,198 rows
BIG = {"method1": (1500, 12000), "method2": (1100, 7500)}
LONG_LIST_THRESHOLD = 0.05     # carrier threshold at which >= 1,000 level-5 joins have |p0 & z| > 8 (asserted below)


@pytest.fixture(scope="module")
def table():
    return bench.fast_table(300, 340)


def big_problem(method, table, perms=130, top_k=40):
    g, e = BIG[method]
    return make_problem(g, e, 300, 340, perms, 5, method=method, top_k=top_k, seed=1, threshold=LONG_LIST_THRESHOLD,
                        table=table)


def joined_pairs(uids):
    """(src, trg) of every joined path in ordinal order: uid row i joins paths0 row i to paths1 rows location[i] + j."""
    count = np.maximum(np.asarray(uids.count, dtype=np.int64), 0)
    src = np.repeat(np.arange(len(count), dtype=np.int64), count)
    first = np.cumsum(count) - count
    trg = np.repeat(np.asarray(uids.location, dtype=np.int64), count) + (np.arange(int(count.sum())) - np.repeat(first, count))
    return src, trg


def long_lists(p, rows3, W):
    """Level-5 joins whose paths0 row shares more than 8 carriers with the row joined to it (method 2: half by half, the
    joined row's halves swapped where the relation is not positive): the inspectors' lists of more than one 8-entry block."""
    u = p.levels.uids["5"]
    src, trg = joined_pairs(u)
    flip = np.zeros(len(src), bool)
    if p.method == "method2":
        flip = np.asarray(u.signs, np.int64)[src] != 1            # path length > 3: the sign of the uid row
    n = 0
    for lo in range(0, len(src), 1 << 20):
        s, t, f = src[lo:lo + (1 << 20)], trg[lo:lo + (1 << 20)], flip[lo:lo + (1 << 20)]
        z = rows3[t]
        if p.method == "method2":
            z = np.where(f[:, None], np.concatenate([z[:, W:], z[:, :W]], axis=1), z)
        n += int((np.bitwise_count(rows3[s] & z).sum(axis=1) > 8).sum())
    return n


@dataclasses.dataclass
class Big:
    p: object
    want: dict       # level 1..5 -> OracleResult (all_scores / all_cases / all_ctrls per joined path; rows of levels 1-3 kept)
    W: int


def _big(method, table):
    p = big_problem(method, table)
    want, W = oracle_levels_kept(p)
    want[4].paths_res = want[5].paths_res = None              # (hundreds of MB nobody reads)
    n = p.levels.n_paths
    # what the caps need of the input, on the oracle alone
    assert n["3"] > 32_768 and n["5"] > 1_048_576 and n["5"] * (2 if method == "method2" else 1) > 4_194_304, n
    assert method == "method2" or n["5"] > 4_194_304, n
    assert long_lists(p, want[3].paths_res, W) >= 1000
    assert len(set(want[5].null.tolist())) * 2 >= p.iterations      # maxima that can tell a dropped stripe of paths
    return Big(p, want, W)


@pytest.fixture(scope="module")
def big_m1(table):
    return _big("method1", table)


@pytest.fixture(scope="module")
def big_m2(table):
    return _big("method2", table)


@contextlib.contextmanager
def plan_of(p):
    """A ResidentPlan with default chunking whose passes are one permutation window."""
    plan = api.ResidentPlan(p, device=0)
    try:
        assert len(plan.windows()) == 1
        yield plan
    finally:
        plan.close()


def run_plan(p):
    with plan_of(p) as plan:
        return plan.run()


def assert_levels(got, want):
    for name, lst in LST.items():
        assert_same_result(got[name], want[int(lst[3:])])


# the caps a join form crosses on the method-1 problem (5.3 M joined paths in one chunk) ...
SELECT = ("k_expand", "k_hist_st", "k_collect_gt")
IE_M1 = SELECT + ("k_stats_ie2", "k_range_union")
CAPS_M1 = {"auto": IE_M1, "ie-quad": IE_M1, "ie-m1": IE_M1, "ie-noprune": IE_M1,
           "sparse": SELECT + ("k_stats", "k_row_bits", "k_row_fill", "k_delta_fill", "k_scan_top"),
           "dense": SELECT + ("k_stats",)}
# ... and on the method-2 problem (2.3 M joined paths, 4.7 M lists): level 5 joins rows of level 3, which have carriers in
# both halves, so its inspector is k_stats_ie2s (k_stats_ie2h: test_one_sided_inspector_past_its_grid)
CAPS_M2 = {"auto": ("k_stats_ie2s",), "ie-quad": ("k_stats_ie2s",), "ie-m1": ("k_stats_ie2s",), "ie-noprune": ("k_stats_ie2s",),
           "sparse": ("k_stats", "k_row_bits", "k_row_fill", "k_delta_fill", "k_scan_top"), "dense": ("k_stats",)}


@pytest.mark.parametrize("kernel", MODES)
def test_method1_join_past_the_caps(big_m1, kernel, monkeypatch, trace):
    """5.3 M level-5 paths: k_expand and the select kernels past 4,194,304 entries, the block-staged inspector k_stats_ie2 past
    its 1,048,576 paths (a wave owns 64 paths per round), k_range_union past 65,536 pairs; on the sparse and dense roads
    k_stats past 16,384 paths, and the sparse road's list kernels (k_row_bits, k_row_fill, k_delta_fill) past their grids."""
    set_mode(monkeypatch, kernel)
    got = run_plan(big_m1.p)
    tr = launches(trace())
    assert_levels(got, big_m1.want)
    assert_crossed(tr, CAPS_M1[kernel], f"method1 {kernel}")


@pytest.mark.parametrize("kernel", MODES)
def test_method2_join_past_the_caps(big_m2, kernel, monkeypatch, trace):
    """2.3 M level-5 paths of the signed method: k_stats_ie2s (one round per half, a wave owns 32 paths) past its 524,288
    paths; on the sparse road 4.7 M delta lists, which k_scan_top's one block scans in >= 4 carried rounds."""
    set_mode(monkeypatch, kernel)
    got = run_plan(big_m2.p)
    tr = launches(trace())
    assert_levels(got, big_m2.want)
    assert_crossed(tr, CAPS_M2[kernel], f"method2 {kernel}")
    if kernel == "sparse":
        assert max(w for w, _ in tr["k_scan_top"]) >= 4, tr["k_scan_top"]


# ---- the one-sided inspector -------------------------------------------------------------------------------------------
# k_stats_ie2h runs where every row of the join's reduced operand has an empty half (gene rows: levels up to 4), and the
# stated method-2 problem has 344,407 level-4 paths.  A length-4 network of its own: 1,112,198 level-4 paths
ONE_SIDED_NETWORK = (2000, 17000)


@pytest.fixture(scope="module")
def one_sided(table):
    p = make_problem(*ONE_SIDED_NETWORK, 300, 340, 130, 4, method="method2", top_k=40, seed=1, threshold=LONG_LIST_THRESHOLD,
                     table=table)
    assert p.levels.n_paths["4"] > 1_048_576, p.levels.n_paths
    want = oracle.process_paths(p, order="canonical", nthreads=8)
    assert len(set(want["lst4"].null.tolist())) * 2 >= p.iterations
    return p, want


@pytest.mark.parametrize("kernel", ["auto", "ie-noprune"])
def test_one_sided_inspector_past_its_grid(one_sided, kernel, monkeypatch, trace):
    """1.1 M level-4 paths of the signed method (rows of level 3 joined to gene rows): k_stats_ie2h, one round per path, past
    its 4,096 blocks x 4 waves x 64 paths."""
    p, want = one_sided
    set_mode(monkeypatch, kernel)
    got = run_plan(p)
    tr = launches(trace())
    for name, lst in LST.items():
        if name in got:
            assert_same_result(got[name], want[lst])
    assert_crossed(tr, ("k_stats_ie2h",), f"one-sided {kernel}")


# ---- the cut among equal keys -----------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def flat(table):
    """The method-1 problem on a flat table: every joined path of every level scores 3.25."""
    t = table.copy()
    t[:] = 3.25
    p = big_problem("method1", t, perms=3, top_k=3000)
    return p, oracle.process_paths(p, order="canonical", nthreads=8)


@pytest.mark.parametrize("kernel", ["auto", "dense"])
def test_cut_among_five_million_equal_keys(flat, kernel, monkeypatch, trace):
    """top_k = 3,000 of 5.3 M equal keys: the radix select finds one bucket per digit over every round of k_hist_st, and the
    tie cut keeps the smallest ordinals, which are the oracle's."""
    p, want = flat
    w5 = want["lst5"]
    assert len(w5.scores) == 3000 and (w5.all_scores == 3.25).all() and len(w5.all_scores) > 4_194_304
    src, trg = joined_pairs(p.levels.uids["5"])
    np.testing.assert_array_equal(np.sort(w5.src.astype(np.int64) * (1 << 32) + w5.trg),
                                  src[:3000] * (1 << 32) + trg[:3000])             # the 3,000 smallest ordinals
    set_mode(monkeypatch, kernel)
    got = run_plan(p)
    tr = launches(trace())
    for name, lst in LST.items():
        assert_same_result(got[name], want[lst])
    assert_crossed(tr, ("k_hist_st",), f"ties {kernel}")


# ---- the wide-row inspector -------------------------------------------------------------------------------------------
WIDE_NETWORK = (350, 2150)      # 74,343 level-4 paths: more than 4,096 blocks x 16 paths, fewer than two rounds of them


@pytest.fixture(scope="module")
def wide_table():
    return bench.fast_table(5150, 5154)


@pytest.fixture(scope="module", params=["method1", "method2"])
def wide(request, wide_table):
    p = make_problem(*WIDE_NETWORK, 5150, 5154, 130, 4, method=request.param, top_k=40, seed=1, table=wide_table)
    assert (p.n_cases + p.n_ctrls + 63) // 64 == 161 and 65_536 < p.levels.n_paths["4"] < 131_072, p.levels.n_paths
    return p, oracle.process_paths(p, order="canonical", nthreads=8)


@pytest.mark.parametrize("kernel", ["auto", "ie-noprune"])
def test_wide_row_inspector_past_its_grid(wide, kernel, monkeypatch, trace):
    """161 mask words (rows too wide for the block-staged inspectors) and 74,343 level-4 paths: the blocks of k_stats_ie<M>
    take a second batch of 16 paths, and the last round is ragged."""
    p, want = wide
    set_mode(monkeypatch, kernel)
    got = run_plan(p)
    tr = launches(trace())
    for name, lst in LST.items():
        if name in got:
            assert_same_result(got[name], want[lst])
    assert_crossed(tr, ("k_stats_ie<M>",), f"wide {p.method} {kernel}")


# ---- per-path outputs on the big joins --------------------------------------------------------------------------------
NAMES = {"4": 4, "5": 5}


def test_hit_lists_of_every_path(big_m1, trace):
    """A HitList with cut-off -inf on levels 4 and 5, sized to the join: every record equals the definition's
    (report.hits_reference).  k_hits_collect walks 5.3 M paths with cus x 8 blocks of 256."""
    p, want = big_m1.p, big_m1.want
    with plan_of(p) as plan:
        hits = {k: api.HitList(plan.ex, float("-inf"), cap=p.levels.n_paths[k]) for k in NAMES}
        got = plan.run(hits=hits)
        tr = launches(trace())
        assert_levels(got, want)
        for name, L in NAMES.items():
            r = want[L]
            ref = report.hits_reference(r.all_scores, r.all_cases, r.all_ctrls, p.levels.uids[name], float("-inf"))
            h = hits[name].read()
            assert h.complete and h.found == ref["found"] == p.levels.n_paths[name] and h.paths == p.levels.n_paths[name]
            np.testing.assert_array_equal(h.score.view(np.uint64), ref["score"].view(np.uint64), err_msg=name)
            for f in ("ordinal", "src", "trg", "cases", "ctrls"):
                np.testing.assert_array_equal(getattr(h, f), ref[f], err_msg=f"{name} {f}")
        assert_crossed(tr, ("k_hits_collect",), "hits")


def test_gene_tally_of_every_path(big_m1, trace):
    """A GeneTally on levels 4 and 5 against report.gene_best_reference: k_gene_fold / k_gene_index past cus x 8 x 256 paths."""
    p, want = big_m1.p, big_m1.want
    ng, ng2 = len(p.data1), len(p.data2)
    tables = report.gene_tables(p.levels, ng, ng2)
    with plan_of(p) as plan:
        tallies = {k: api.GeneTally(plan.ex, report.gene_slots(k, ng, ng2), *tables[k]) for k in NAMES}
        got = plan.run(tallies=tallies)
        tr = launches(trace())
        assert_levels(got, want)
        for name, L in NAMES.items():
            r = want[L]
            ref = report.gene_best_reference(r.all_scores, r.all_cases, r.all_ctrls, p.levels.uids[name], *tables[name],
                                             report.gene_slots(name, ng, ng2))
            g = tallies[name].read()
            assert np.isfinite(ref["score"]).sum() > ng // 2, name
            np.testing.assert_array_equal(g.score.view(np.uint64), ref["score"].view(np.uint64), err_msg=name)
            for f in ("ordinal", "src", "trg", "cases", "ctrls"):
                np.testing.assert_array_equal(getattr(g, f), ref[f], err_msg=f"{name} {f}")
        assert_crossed(tr, ("k_gene_fold",), "gene tally")


def perm_counts_reference(p, want, name, thr, shard=None):
    """(V[threshold][permutation], observed[threshold], scores) of the method-1 problem's level ``name`` for ascending
    thresholds: report.exceed_reference(per_permutation=True) restated for 6.9e8 (path, permutation) pairs.  A null value is
    the folded f32 table cell [a][tot - a] (a = the path's carriers among the permutation's cases, tot = its carriers), so how
    many thresholds a pair reaches is looked up per (a, tot) -- through the reference's own _vt_cell and _fold_f32 -- and the
    pairs are counted per permutation.  Checked against exceed_reference itself on a shard of each level (perm_counts_m1)."""
    assert p.method == "method1" and (np.diff(thr) > 0).all()
    n, K = p.n_cases + p.n_ctrls, p.iterations
    masks = (np.arange(n) < p.n_cases)[None, :] ^ (np.asarray(p.perm_cases) != 1)
    rows = {"4": (want[3].paths_res, want[2].paths_res), "5": (want[3].paths_res, want[3].paths_res)}[name]
    VT = np.asarray(p.value_table, np.float64)
    a, tot = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    null = report._fold_f32(report._vt_cell(VT, n, a, tot - a))
    reached = np.searchsorted(thr, null.astype(np.float64), side="right").astype(np.uint8).ravel()     # [a * (n + 1) + tot]
    wide = np.ascontiguousarray(masks.astype(np.float32).T) * np.float32(n + 1)     # a row times it: a * (n + 1) per permutation
    W = rows[0].shape[1]
    case = np.packbits(np.arange(64 * W) < p.n_cases, bitorder="little").view("<u8")
    src, trg = joined_pairs(p.levels.uids[name])
    if shard is not None:
        src, trg = src[shard[0]:shard[1]], trg[shard[0]:shard[1]]
    h = np.zeros((len(thr) + 1, K), np.int64)
    scores = np.zeros(len(src))
    for lo in range(0, len(src), 1 << 15):
        bp = rows[0][src[lo:lo + (1 << 15)]] | rows[1][trg[lo:lo + (1 << 15)]]                      # packed, [block][W]
        t = np.bitwise_count(bp).sum(axis=1)
        cases = np.bitwise_count(bp & case).sum(axis=1)
        scores[lo:lo + (1 << 15)] = report._vt_cell(VT, n, cases, t - cases)
        bits = np.unpackbits(bp.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(np.float32)
        cell = (bits @ wide + t[:, None].astype(np.float32)).astype(np.intp)       # exact: a * (n + 1) + tot < 2^24
        got = reached[cell]
        i, r = np.nonzero(got)                                                     # few pairs reach the lowest threshold
        np.add.at(h, (got[i, r], r), 1)
    h[0] = len(src) - h[1:].sum(axis=0)
    V = np.cumsum(h[::-1], axis=0)[::-1][1:].astype(np.uint64)             # row j: the pairs that reach more than j thresholds
    observed = (scores[None, :] >= thr[:, None]).sum(axis=1).astype(np.uint64)
    return V, observed, scores, masks, rows


@pytest.fixture(scope="module")
def perm_counts_m1(big_m1):
    """Ten thresholds at the 10th .. 99.9th percentiles of the level-5 null maxima, and per level the definition's counts."""
    p, want = big_m1.p, big_m1.want
    thr = np.unique(np.percentile(want[5].null.astype(np.float64), [10, 20, 30, 40, 50, 60, 70, 80, 90, 99.9]))
    assert len(thr) == 10
    # the restated counts are the project's definition: equal to report.exceed_reference on a shard of either level
    for name, shard in (("4", (0, 20_000)), ("5", (2_600_000, 2_620_000))):
        V, observed, _, masks, rows = perm_counts_reference(p, want, name, thr, shard)
        full = report.exceed_reference(p.method, p.n_cases, p.n_ctrls, p.levels.uids[name], *rows, p.value_table, masks, thr,
                                       shard=shard, per_permutation=True)
        np.testing.assert_array_equal(V, full["perm_counts"])
        np.testing.assert_array_equal(observed, full["observed"])
        assert V.any()
    ref = {}
    for name, L in NAMES.items():
        V, observed, sc, _, _ = perm_counts_reference(p, want, name, thr)
        np.testing.assert_array_equal(sc.view(np.uint64), want[L].all_scores.view(np.uint64))
        # the counts can tell: the permutations' counts differ (level 5: at every threshold; level 4's maxima are lower)
        assert sum(len(set(row.tolist())) > 1 for row in V) >= (10 if name == "5" else 5), name
        ref[name] = (V, observed)
    return thr, ref


@pytest.mark.parametrize("form", ["ie", "dense"])
def test_perm_counts_of_every_pair(big_m1, perm_counts_m1, form, monkeypatch, trace):
    """ExceedCounts(perm_counts=True) on levels 4 and 5 under both counting forms: V[threshold][permutation] sees every (path,
    permutation) pair of the join, and k_exceed_observed walks 5.3 M scores with cus x 8 blocks."""
    p, want = big_m1.p, big_m1.want
    thr, ref = perm_counts_m1
    monkeypatch.setenv("GCRE_EXCEED_KERNEL", form)
    with plan_of(p) as plan:
        xs = {k: api.ExceedCounts(plan.ex, thr, perm_counts=True) for k in NAMES}
        got = plan.run(exceeds=xs)
        tr = launches(trace())
        assert_levels(got, want)
        for name in NAMES:
            V, observed = ref[name]
            e = xs[name].read()
            assert e.paths == p.levels.n_paths[name] and e.perms == p.iterations
            np.testing.assert_array_equal(e.perm_counts, V, err_msg=f"{form} level {name}")
            np.testing.assert_array_equal(e.exceed, V.sum(axis=1), err_msg=f"{form} level {name}")
            np.testing.assert_array_equal(e.observed, observed, err_msg=f"{form} level {name}")
        assert_crossed(tr, ("k_exceed_observed",), f"perm counts {form}")


# ---- k_select ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("method", [1, 2])
def test_select_past_its_grid(big_m1, method, trace):
    """430,000 indices with repetition into the 1,500 loaded rows: 430,000 x 12 (24) padded words > 16,384 blocks x 256."""
    p = big_m1.p
    rng = np.random.default_rng(11)
    idx = rng.integers(0, len(p.data1), size=430_000).astype(np.int32)
    idx[:3] = (len(p.data1) - 1, 0, len(p.data1) - 1)
    ox = oracle.OracleJoinExec(method, p.n_cases, p.n_ctrls, 0)
    rows = ox.load(p.data1)
    assert rows.shape == (1500, 10 * method) and rows.any(axis=1).sum() > 1000
    ex = api.JoinExec(method, p.n_cases, p.n_ctrls, 0)
    try:
        loaded = ex.load(p.data1)
        np.testing.assert_array_equal(loaded.to_numpy(), rows)
        picked = loaded.select(idx)
        assert picked.size == len(idx)
        np.testing.assert_array_equal(picked.to_numpy(), rows[idx])
        assert_crossed(launches(trace()), ("k_select",), f"select method {method}")
    finally:
        ex.close()


# ---- set tiles per block ----------------------------------------------------------------------------------------------
SET_K = 16 * 512 + 1       # 17 permutation tiles, the last of one permutation


def tiles_for(per, cus):
    """The fewest set tiles npt for which a block of k_set_null walks ``per`` of them at SET_K permutations (fill_set_launch:
    per = npt * nkt / (cus * 32), rounded down), not a multiple of ``per``: the last blocks get one tile fewer."""
    nkt, slots = (SET_K + 511) // 512, cus * 32
    npt = -(-per * slots // nkt)
    while npt % per == 0:
        npt += 1
    assert npt * nkt // slots == per
    return npt


@pytest.mark.parametrize("method,per", [(1, 3), (2, 3)])
def test_set_tiles_per_block(method, per, trace):
    """Enough sets that a block of k_set_null walks three set tiles (its double-buffered mask stream wraps to chunk 0 between
    them), a ragged share for the last blocks and a ragged last tile: records, n_ge and family_max equal the restatement's
    (test_sets_host.restate_slabs, checked against restate there) as bits."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tile = 16 if method == 1 else 8
    npt = tiles_for(per, cus)
    V = (npt - 1) * tile + 3
    nc, nt = 33, 37
    n = nc + nt
    rng = np.random.default_rng(100 + method)
    pos = rng.random((V, n)) < rng.uniform(0.02, 0.6, size=(V, 1))
    neg = rng.random((V, n)) < rng.uniform(0.02, 0.6, size=(V, 1))
    pos[0], pos[1], neg[1] = True, False, False
    # a chi-square-like table (square: the signed method's (-) half reads rows by control counts) with f64 tails and some
    # negative cells: on uniform cells the maximum over 20,000 sets is the same few cells for every permutation
    VT = bench.fast_table(n, n) + rng.random((n + 1, n + 1)) * 1e-7
    VT[rng.random(VT.shape) < 0.05] *= -1
    ex = api.JoinExec(method, nc, nt, SET_K)
    try:
        ex.set_value_table(VT)
        ex.generate_permutations(4711)
        masks = device_masks(ex, SET_K, n)
        if method == 1:
            rec, fam = ex.score_sets(np.arange(V).reshape(V, 1), pos.astype(np.int8), family=True)
        else:
            rec, fam = ex.score_sets(np.stack([np.arange(V), V + np.arange(V)], axis=1), np.vstack([pos, neg]).astype(np.int8),
                                     np.tile(np.array([1, -1]), (V, 1)), family=True)
        geo = set_tiles(trace(), "k_set_null")
    finally:
        ex.close()
    assert geo and all(g[0] == npt and g[2] >= per and g[0] % g[1] != 0 for g in geo), geo
    want = restate_slabs(method, nc, nt, pos, neg if method == 2 else None, VT, masks)
    assert len(rec) == V and (rec["valid"] == 1).all()
    for f in FIELDS[1:]:
        np.testing.assert_array_equal(rec[f], want[f], err_msg=f)
    np.testing.assert_array_equal(rec["score"].view(np.uint64), want["score"].view(np.uint64))
    np.testing.assert_array_equal(fam.view(np.uint32), want["family"].view(np.uint32))
    # what was compared can tell: thousands of different per-set counts (70 patients leave the family maximum, the largest of
    # 20,000 sets' values, a few dozen cells to be)
    assert len(set(want["n_ge"].tolist())) >= 1000 and len(set(want["family"].tolist())) >= 30


STEPDOWN_TOP = 7953        # of the 7,961 level-3 paths below: 995 set tiles of 8, the last of one row


def test_stepdown_tiles_per_block(trace):
    """k_stepdown_null with two set tiles per block.  Its sets are a join's top rows, at most 10,000 of them with at most 2^26
    (row, permutation) cells, so only the signed method (8 sets per tile) reaches per = 2 at 256 CUs, with 7,705 to 8,190 rows
    at SET_K permutations: the top 7,953 of a level-3 join of 7,961 paths (995 tiles over 498 blocks per permutation tile: the
    last block walks one), through gcre_process_paths and ExceedCounts.stepdown, against report.stepdown_reference in its sorted
    form (test_stepdown_host.reference_sorted, checked against the reference there).  The table is the carrier total plus a
    little noise, so that a row's null values rank as its score does: hundreds of rows' counts lie below the single-step ones
    (on a table of unrelated cells the maximum over thousands of paths reaches every threshold but the best few)."""
    a, b = np.meshgrid(np.arange(71), np.arange(71), indexing="ij")
    VT = a + b + np.random.default_rng(8).random((71, 71)) * 0.05
    p = make_problem(100, 850, 33, 37, SET_K, 3, method="method2", top_k=STEPDOWN_TOP, seed=3, threshold=0.3, table=VT)
    assert p.levels.n_paths["3"] == 7961
    assert STEPDOWN_TOP <= api.EXCEED_MAX and STEPDOWN_TOP * SET_K <= api.EXCEED_PERM_CELLS
    cpu = Cpu(p, nthreads=8)
    top = top_rows(cpu, "3")
    assert len(top[2]) == STEPDOWN_TOP
    want = reference_sorted(p.method, p.n_cases, p.n_ctrls, p.levels.uids["3"], *cpu.ops["3"], p.value_table, cpu.masks, top)
    np.testing.assert_array_equal(want["scores"].view(np.uint64), top[2].view(np.uint64))
    assert (want["n_ge"] < want["single"]).sum() >= 400 and len(set(want["n_ge"].tolist())) >= 100
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    try:
        x = api.ExceedCounts(ex, top[2], perm_counts=True)
        res = api.process_paths(p, exec_=ex, exceeds={"3": x})
        trace()
        got = x.stepdown(*sets_of(cpu, "3", top[0], top[1]))
        geo = set_tiles(trace(), "k_stepdown_null")
    finally:
        ex.close()
    assert geo and all(g[0] == 995 and g[2] >= 2 and g[0] % g[1] != 0 for g in geo), geo
    np.testing.assert_array_equal(res["lst3"].null.view(np.uint32), want["null_max"].view(np.uint32))
    np.testing.assert_array_equal(got, want["n_ge"])
