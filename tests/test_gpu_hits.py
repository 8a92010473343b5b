"""Hit lists on the device (gcre_hits, k_hits_collect) against their numpy definition, report.hits_reference, fed with every
joined path's score, cases and controls from the CPU oracle.  Every comparison is exact: scores as f64 bit patterns,
integers as integers (pytest -m gpu).

GCRE_HITS_FUZZ_CASES=200 [GCRE_HITS_FUZZ_BASE=...] for a long run of the seeded loop at the end; a handful by default."""
from __future__ import annotations

import ctypes
import dataclasses
import os

import numpy as np
import pytest

import oracle
from geneticscre_amd import api, report, synth
from helpers import small_table

pytestmark = pytest.mark.gpu

LEVELS = report.GENE_LEVELS                      # "1b", "2", "3", "4", "5": the joins behind lst1 .. lst5
FIELDS = ("ordinal", "src", "trg", "cases", "ctrls")
COUNTERS = ("null_kernel_launches", "ie_launches", "ie_quad_launches", "ie_hinted_joins", "ie_plane_joins",
            "ie_overlap_lists", "inspect_replays", "paths", "scores")   # (not ie_lookup_tiles: it depends on when thresholds land)
NINF = float("-inf")
KINDS = ("worst_top", "median", "ninf", "above", "zero")

SIZES = {"sets": (34, 80, 61, 70, 700, 5, 9, 4242), "cache": (40, 110, 310, 335, 300, 5, 15, 21)}


def sized(method, size, K=None, table=True):
    g, e, nc, nt, perms, L, top_k, seed = SIZES[size]
    return synth.make_problem(g, e, nc, nt, perms if K is None else K, L, method=method, top_k=top_k, seed=seed,
                              table=small_table(nc + nt, nc + nt, 8) if table else None)


_ORACLE = {}


def oracle_levels(p, key):
    """lst1 .. lst5 of the oracle, computed once per problem: observed scores do not depend on the permutations, the
    oracle runs with one."""
    if key not in _ORACLE:
        few = dataclasses.replace(p, iterations=min(p.iterations, 1), perm_cases=p.perm_cases[:1] if p.iterations else p.perm_cases)
        _ORACLE[key] = oracle.process_paths(few, order="canonical")
    return _ORACLE[key]


def cutoffs(want, kind, levels=LEVELS):
    """Level name -> the cut-off of that kind."""
    out = {}
    for name in levels:
        r = want[f"lst{LEVELS.index(name) + 1}"]
        finite = r.all_scores[np.isfinite(r.all_scores)]
        top = r.scores[np.isfinite(r.scores)]
        out[name] = {"worst_top": float(top.min()), "median": float(np.median(finite)), "ninf": NINF,
                     "above": float(np.nextafter(finite.max(), np.inf)), "zero": 0.0}[kind]
    return out


def reference(p, want, cuts, shard=None):
    out = {}
    for name, c in cuts.items():
        r = want[f"lst{LEVELS.index(name) + 1}"]
        out[name] = report.hits_reference(r.all_scores, r.all_cases, r.all_ctrls, p.levels.uids[name], c, shard=shard)
    return out


def assert_hits(got, want, what=""):
    assert got.found == want["found"], f"{what} found"
    assert got.complete
    assert got.score.dtype == np.float64 and got.ordinal.dtype == np.int64
    np.testing.assert_array_equal(got.score.view(np.uint64), want["score"].view(np.uint64), err_msg=f"{what} score")
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(got, f), want[f], err_msg=f"{what} {f}")


def make_lists(ex, cuts, cap=1 << 16):
    return {name: api.HitList(ex, c, cap=cap) for name, c in cuts.items()}


def bites(got):
    return any(0 < h.found < h.paths for h in got.values())


@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_list_equals_the_reference_on_every_level(method, size):
    p = sized(method, size, table=size == "sets")
    if size == "cache":
        assert all(p.levels.n_paths[k] >= 192 for k in ("3", "4", "5")), p.levels.n_paths
    want = oracle_levels(p, (method, size))
    lib = api._hits_lib()
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    try:
        bit = False
        for kind in KINDS:
            cuts = cutoffs(want, kind)
            ref = reference(p, want, cuts)
            lists = make_lists(ex, cuts)
            before = lib.gcre_hits_launches(ex._h)
            res = api.process_paths(p, exec_=ex, hits=lists)
            assert lib.gcre_hits_launches(ex._h) >= before + len(LEVELS), kind   # (also when nothing reaches the cut-off)
            got = {name: h.read() for name, h in lists.items()}
            for L, name in enumerate(LEVELS, start=1):
                what = f"{method} {size} {kind} level {name}"
                assert_hits(got[name], ref[name], what)
                assert got[name].paths == p.levels.n_paths[name], what
                n_scorable = int((want[f"lst{L}"].all_scores > NINF).sum())
                if kind == "ninf":
                    assert got[name].found == n_scorable, what
                if kind == "above":
                    assert got[name].found == 0 and len(got[name].score) == 0, what
                if kind == "worst_top":
                    # the list begins with the top-k list, best first
                    top = res[f"lst{L}"]
                    keep = np.isfinite(top.scores)
                    n = int(keep.sum())
                    assert n > 0 and got[name].found >= n, what
                    np.testing.assert_array_equal(got[name].score[:n].view(np.uint64), top.scores[keep][::-1].view(np.uint64))
                    for f in ("src", "trg", "cases", "ctrls"):
                        np.testing.assert_array_equal(getattr(got[name], f)[:n], getattr(top, f)[keep][::-1], err_msg=f"{what} {f}")
            bit = bit or bites(got)
            for h in lists.values():
                h.free()
        assert bit
    finally:
        ex.close()


def tied_problem(method):
    """Duplicate genotype rows for groups of genes, and a table of thirteen distinct values: many paths share a score."""
    p = synth.make_problem(36, 100, 50, 55, 200, 5, method=method, top_k=9, seed=77)
    rng = np.random.default_rng(5)
    data1 = p.data1.copy()
    for group in (range(0, 8), range(8, 14), range(14, 18)):
        for g in group:
            if g < len(data1):
                data1[g] = data1[group[0]]
    table = np.round(rng.random((p.n_cases + p.n_ctrls + 1,) * 2) * 12.0)
    return dataclasses.replace(p, data1=data1, data2=data1[p.levels.uids["1b"].src], value_table=table)


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_ties_at_the_cutoff_are_all_listed_in_ordinal_order(method):
    p = tied_problem(method)
    want = oracle_levels(p, (method, "tied"))
    cuts = {}
    for L, name in enumerate(LEVELS, start=1):
        s = want[f"lst{L}"].all_scores
        vals, n = np.unique(s[np.isfinite(s)], return_counts=True)
        many = vals[n >= 3]
        cuts[name] = float(many[len(many) // 2]) if len(many) else float(vals[0])     # a score several paths share
    ref = reference(p, want, cuts)
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    try:
        lists = make_lists(ex, cuts)
        api.process_paths(p, exec_=ex, hits=lists)
        got = {name: h.read() for name, h in lists.items()}
    finally:
        ex.close()
    tied_levels = 0
    for L, name in enumerate(LEVELS, start=1):
        assert_hits(got[name], ref[name], f"{method} level {name}")
        at = np.flatnonzero(want[f"lst{L}"].all_scores == cuts[name])
        tail = got[name].ordinal[got[name].score == cuts[name]]
        assert tail.tolist() == at.tolist(), name                      # every one of them, in ordinal order, ...
        assert len(at) == 0 or got[name].ordinal[-len(at):].tolist() == at.tolist(), name    # ... at the end of the list
        tied_levels += len(at) >= 3
    assert tied_levels >= 3 and bites(got)


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_overflow_counts_everything_and_refuses_the_read(method):
    p = sized(method, "cache", table=False)
    want = oracle_levels(p, (method, "cache"))
    cuts = cutoffs(want, "median")
    ref = reference(p, want, cuts)
    lib = api._hits_lib()
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    try:
        small = make_lists(ex, cuts, cap=7)
        api.process_paths(p, exec_=ex, hits=small)
        for name in LEVELS:
            h = small[name].read()
            assert h.found == ref[name]["found"] and h.paths == p.levels.n_paths[name], name
            if name in ("3", "4", "5"):
                assert h.found > 7, name
            assert h.complete == (h.found <= 7) and (h.complete or len(h.score) == 0), name
        h5 = small["5"]
        n = ref["5"]["found"]
        score, ordinal = np.full(n, 123.0), np.full(n, -5, np.int64)
        rc = lib.gcre_hits_read(h5._h, n, api._ptr(score), api._ptr(ordinal), None, None, None, None)
        assert rc == api.GCRE_ERR_RANGE and b"cut-off" in ex._lib.gcre_last_error(ex._h)
        assert (score == 123.0).all() and (ordinal == -5).all()           # the outputs are untouched
        assert lib.gcre_hits_read(h5._h, 7, api._ptr(score), api._ptr(ordinal), None, None, None, None) == api.GCRE_ERR_ARG
        # reset empties the small lists; a large enough list on the same context is right
        for name in LEVELS:
            small[name].reset()
            assert small[name].count() == (0, 0)
        big = make_lists(ex, cuts)
        api.process_paths(p, exec_=ex, hits=big)
        for name in LEVELS:
            assert_hits(big[name].read(), ref[name], f"{method} level {name} after the overflow")
            assert small[name].count() == (0, 0)                          # (not armed: not touched)
    finally:
        ex.close()


VARIANTS = {
    "chunks": ({"GCRE_CHUNK_PATHS": "64"}, {}),
    "chunks_dense": ({"GCRE_CHUNK_PATHS": "64", "GCRE_NULL_KERNEL": "dense"}, {}),
    "cache_replay": ({}, {"passes": 2, "keep": True}),
    "ahead_off": ({"GCRE_AHEAD": "0"}, {}),
    "ahead_on": ({"GCRE_AHEAD": "1"}, {}),
    "ahead_on_chunks": ({"GCRE_AHEAD": "1", "GCRE_CHUNK_PATHS": "64"}, {}),
    "no_perms": ({}, {"K": 0}),
    "windows": ({"GCRE_WINDOW_TILES": "1"}, {"K": 5000, "window": 2048}),
    "windows_ahead_off": ({"GCRE_WINDOW_TILES": "1", "GCRE_AHEAD": "0"}, {"K": 5000, "window": 2048}),
    "sparse": ({"GCRE_NULL_KERNEL": "sparse"}, {}),
    "dense": ({"GCRE_NULL_KERNEL": "dense"}, {}),
    "ie": ({"GCRE_NULL_KERNEL": "ie"}, {}),
    "ie_no_quad": ({"GCRE_NULL_KERNEL": "ie", "GCRE_IE_QUAD": "0"}, {}),
}


def plan_pass(p, cuts, passes=1, keep=False, window=None):
    """ResidentPlan passes (the launch-ahead chain, the inspection cache, permutation windows), fresh lists per pass:
    (hits of the last pass, its profile)."""
    plan = api.ResidentPlan(p)
    try:
        if window:
            plan.set_window(window)
        for _ in range(passes):
            lists = make_lists(plan.ex, cuts)
            plan.run(keep_inspections=keep, hits=lists)
            got = {k: h.read() for k, h in lists.items()}
        return got, dict(plan.last_profile)
    finally:
        plan.close()


def one_call(p, cuts=None):
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    try:
        lists = make_lists(ex, cuts) if cuts else {}
        res = api.process_paths(p, exec_=ex, hits=lists or None)
        return res, {k: h.read() for k, h in lists.items()}
    finally:
        ex.close()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_list_does_not_depend_on_how_the_join_ran(method, variant, monkeypatch):
    """Chunk size (>= 3 chunks per join from level 3 up, a ragged last wave), a pass replayed from the inspection cache, the
    launch-ahead chain on and off, no permutations, several permutation windows, every null kernel form: the same list, the
    reference's, every path listed ONCE -- a list appends, so a chunk collected per window or per replay would show."""
    env, how = VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)                 # before the context is created: gcre_create reads them
    p = sized(method, "cache", K=how.get("K"), table=False)
    if "GCRE_CHUNK_PATHS" in env:
        assert all(p.levels.n_paths[k] >= 3 * 64 for k in ("3", "4", "5")), p.levels.n_paths
        assert any(p.levels.n_paths[k] % 64 for k in ("3", "4", "5")), p.levels.n_paths
    want = oracle_levels(sized(method, "cache", table=False), (method, "cache"))
    cuts = cutoffs(want, "median")
    ref = reference(p, want, cuts)
    got, prof = plan_pass(p, cuts, passes=how.get("passes", 1), keep=how.get("keep", False), window=how.get("window"))
    if variant.startswith("ahead_on"):
        assert prof["inspect_replays"] > 0, prof     # the chain ran: the later joins were collected in their counting replay
    if variant == "ahead_off":
        assert prof["inspect_replays"] == 0, prof
    if variant == "cache_replay":
        assert prof["inspect_replays"] >= len(LEVELS), prof
    if variant.startswith("windows"):
        assert prof["inspect_replays"] >= 2 * len(LEVELS), prof    # three windows: the joins ran three times
    assert bites(got)
    for name in LEVELS:
        assert_hits(got[name], ref[name], f"{method} {variant} level {name}")
        assert got[name].paths == p.levels.n_paths[name], name
    # and through the one-call driver (no chain; it turns the cache on by itself for several windows)
    _, got2 = one_call(p, cuts)
    for name in LEVELS:
        assert_hits(got2[name], ref[name], f"{method} {variant} one call, level {name}")
        assert got2[name].paths == p.levels.n_paths[name], name


@pytest.mark.parametrize("chunk", ["", "64"])
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_two_shards_append_to_the_whole(method, chunk, monkeypatch):
    """Levels 3, 4 and 5 joined in two sharded calls over [0, P/2) and [P/2, P): each list equals the reference restricted
    to its shard, and both shards into ONE list equal the unsharded reference."""
    monkeypatch.setenv("GCRE_AHEAD", "0")
    if chunk:
        monkeypatch.setenv("GCRE_CHUNK_PATHS", chunk)
    p = sized(method, "cache", table=False)
    want = oracle_levels(p, (method, "cache"))
    cuts = cutoffs(want, "median", levels=("3", "4", "5"))
    whole = reference(p, want, cuts)
    plan = api.ResidentPlan(p)
    try:
        plan.run()                                # the kept sets of levels 1..3 are the operands below
        for name in ("3", "4", "5"):
            P = p.levels.n_paths[name]
            p0, p1, _ = plan.operands(name)
            both = api.HitList(plan.ex, cuts[name], cap=1 << 16)
            for half in [(0, P // 2), (P // 2, P)]:
                h = api.HitList(plan.ex, cuts[name], cap=1 << 16)
                plan.ex.join(plan.uids[name], p0, p1, None, shard=half, hits=h)
                plan.ex.join(plan.uids[name], p0, p1, None, shard=half, hits=both)
                part = reference(p, want, {name: cuts[name]}, shard=half)[name]
                got = h.read()
                assert_hits(got, part, f"{method} level {name} shard {half}")
                assert got.paths == half[1] - half[0] and 0 < got.found < got.paths
            got = both.read()
            assert_hits(got, whole[name], f"{method} level {name} one list")
            assert got.paths == P
    finally:
        plan.close()


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_found_is_the_observed_count_and_nothing_else_changes(method):
    """With an ExceedCounts on the same joins whose one threshold is the cut-off, found == observed (and a tally may be
    armed too).  The joins' results are byte-identical with and without lists and the launch counters of gcre_profile are
    the same: the list costs its own kernel and nothing else."""
    p = sized(method, "cache", table=False)
    want = oracle_levels(p, (method, "cache"))
    plain, _ = one_call(p)
    tables = report.gene_tables(p.levels, len(p.data1), len(p.data2))
    for kind in ("median", "zero", "ninf"):
        cuts = cutoffs(want, kind)
        ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
        try:
            lists = make_lists(ex, cuts)
            counts = {name: api.ExceedCounts(ex, [c]) for name, c in cuts.items()}
            tallies = {"4": api.GeneTally(ex, report.gene_slots("4", len(p.data1), len(p.data2)), *tables["4"])}
            res = api.process_paths(p, exec_=ex, hits=lists, exceeds=counts, tallies=tallies)
            for L, name in enumerate(LEVELS, start=1):
                h, x = lists[name].read(), counts[name].read()
                assert h.found == int(x.observed[0]) and h.paths == x.paths, (kind, name)
                assert h.found == reference(p, want, {name: cuts[name]})[name]["found"]
            assert tallies["4"].read().score.max() == res["lst4"].scores[-1]
        finally:
            ex.close()
    armed, got = one_call(p, cutoffs(want, "median"))
    assert bites(got)
    for L in range(1, 6):
        a, b = plain[f"lst{L}"], armed[f"lst{L}"]
        for f in ("scores", "src", "trg", "cases", "ctrls", "null"):
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (L, f)
    for f in COUNTERS:
        assert plain["profile"][f] == armed["profile"][f], f


def _network_case(seed, nc=48, nt=52):
    rng = np.random.default_rng(seed)
    g, src, trg, sign = synth.signed_network(30, 70, rng)
    uid = np.arange(g) * 5 + 100
    symbols = [f"G{u}" for u in uid]
    data = (rng.random((g, nc + nt)) < 0.06).astype(np.int32)
    return symbols, data, (uid, symbols, uid[src], uid[trg], sign)


def _rows(df):
    return sorted(zip(df["Lengths"].tolist(), df["SignedPaths"].tolist(), df["Scores"].to_numpy(np.float64).view(np.uint64).tolist(),
                      df["Pvalues"].tolist(), df["Cases"].tolist(), df["Controls"].tolist()))


@pytest.mark.parametrize("signed", [False, True])
def test_gwaspa_significant(signed):
    nc, nt, K, L, top_all, small = 48, 52, 1000, 5, 2000, 3
    genes, data, network = _network_case(17)
    strata = (np.arange(nc + nt) * 5 % 3).astype(np.int32)
    kw = dict(signed=signed, threshold=0.2, n_permutations=K, strata=strata, seed=909, path_length=L)
    # every path of the small problem, as a top-k table
    full = report.gwaspa(genes, data, nc, nt, network, top_k=top_all, **kw)
    prep = full["prepared"]
    levels = api.build_levels(len(prep.ents_uid), prep.src, prep.trg, prep.sign)
    assert max(len(prep.ents2_uid), *(levels.n_paths[k] for k in ("2", "3", "4", "5"))) <= top_all, levels.n_paths
    table = full["GWASPA.Results"]
    table = table[np.isfinite(table["Scores"].to_numpy(np.float64))]
    pv = np.unique(table["Pvalues"].to_numpy(np.float64))
    inner = pv[(pv > 0) & (pv < 1)]
    assert len(inner) >= 2, pv
    # the smallest level at which some length has more significant rows than the small top_k below can hold
    alpha = next(float(a) for a in inner if (table.loc[table["Pvalues"] <= a, "Lengths"].value_counts() > small).any())
    expect = table[table["Pvalues"] <= alpha]
    assert 0 < len(expect) < len(table)                                   # alpha bites
    base = report.gwaspa(genes, data, nc, nt, network, top_k=small, **kw)
    assert set(base) == {"GWASPA.Results", "levels", "prepared"}          # the default output is what it was
    out = report.gwaspa(genes, data, nc, nt, network, top_k=small, significant=alpha, **kw)
    assert set(out) == set(base) | {"Significant.Results", "significant", "significant_cutoffs"}
    assert out["GWASPA.Results"].equals(base["GWASPA.Results"])
    sig = out["Significant.Results"]
    assert list(sig.columns) == report.COLUMNS
    assert _rows(sig) == _rows(expect)
    p_, s_ = sig["Pvalues"].to_numpy(), sig["Scores"].to_numpy()
    assert all((p_[i], -s_[i]) <= (p_[i + 1], -s_[i + 1]) for i in range(len(sig) - 1))     # ordered like GWASPA.Results
    for Lx in range(1, L + 1):
        h = out["significant"][Lx]
        assert h.complete and h.found == int((expect["Lengths"] == Lx).sum()), Lx
        assert out["significant_cutoffs"][Lx] == report.significance_cutoff(out["levels"][f"lst{Lx}"].null, alpha)
    # together with the counting pass of fdr: the same rows, and fdr's columns are what they are without the lists
    both = report.gwaspa(genes, data, nc, nt, network, top_k=small, significant=alpha, fdr=True, **kw)
    fdr = report.gwaspa(genes, data, nc, nt, network, top_k=small, fdr=True, **kw)
    assert both["GWASPA.Results"].equals(fdr["GWASPA.Results"]) and _rows(both["Significant.Results"]) == _rows(expect)
    # a tiny cap: the lengths that overflow warn and contribute no rows
    over = [Lx for Lx in range(1, L + 1) if out["significant"][Lx].found > 1]
    assert over
    with pytest.warns(UserWarning, match="significant_cap") as rec:
        tiny = report.gwaspa(genes, data, nc, nt, network, top_k=small, significant=alpha, significant_cap=1, **kw)
    msgs = [str(w.message) for w in rec if "significant_cap" in str(w.message)]
    assert len(msgs) == len(over)
    for Lx in over:
        assert any(f"length {Lx}:" in m and f"{out['significant'][Lx].found} paths" in m for m in msgs), (Lx, msgs)
        assert not tiny["significant"][Lx].complete and tiny["significant"][Lx].found == out["significant"][Lx].found
    assert _rows(tiny["Significant.Results"]) == _rows(expect[~expect["Lengths"].isin(over)])
    assert tiny["GWASPA.Results"].equals(base["GWASPA.Results"])


def test_refusals():
    p = sized("method1", "sets")
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    lib = api._hits_lib()
    launches = lambda: lib.gcre_hits_launches(ex._h)
    try:
        before, nulls = launches(), ex.profile()["null_kernel_launches"]
        # what gcre_hits_create refuses: in Python and by the library itself
        with pytest.raises(api.GcreError, match="NaN"):
            api.HitList(ex, float("nan"))
        for cap in (0, -1, (1 << 26) + 1):
            with pytest.raises(api.GcreError, match="cap"):
                api.HitList(ex, 1.0, cap=cap)
            assert not lib.gcre_hits_create(ex._h, 1.0, cap) and b"cap" in ex._lib.gcre_last_error(ex._h)
        assert not lib.gcre_hits_create(ex._h, float("nan"), 10) and b"NaN" in ex._lib.gcre_last_error(ex._h)
        for c in (float("inf"), NINF):           # the infinities are cut-offs like any other
            api.HitList(ex, c, cap=1).free()
        good = api.HitList(ex, 0.0, cap=1 << 12)
        # a level outside 0..5
        assert lib.gcre_process_paths_set_hits(ex._h, 6, good._h) == api.GCRE_ERR_ARG
        assert lib.gcre_process_paths_set_hits(ex._h, -1, good._h) == api.GCRE_ERR_ARG
        with pytest.raises(api.GcreError, match="no level"):
            api.process_paths(p, exec_=ex, hits={"6": good})
        # one device of several: refused by the library, and by the resident plan in Python
        keep = []
        inp = api._pp_input(p, keep)
        outs = (api.gcre_result * 5)()
        assert lib.gcre_process_paths_set_hits(ex._h, 4, good._h) == 0
        inp.shard_rank, inp.shard_world = 0, 2
        assert ex._lib.gcre_process_paths(ex._h, ctypes.byref(inp), outs) == api.GCRE_ERR_ARG
        assert b"several" in ex._lib.gcre_last_error(ex._h)
        # a list of another context, and of a destroyed one
        other = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
        try:
            theirs = api.HitList(other, 0.0, cap=16)
            assert lib.gcre_join_set_hits(ex._h, theirs._h) == api.GCRE_ERR_ARG
            assert lib.gcre_process_paths_set_hits(ex._h, 4, theirs._h) == api.GCRE_ERR_ARG
            assert lib.gcre_join_set_hits(other._h, good._h) == api.GCRE_ERR_ARG
            with pytest.raises(api.GcreError, match="context"):
                api.process_paths(p, exec_=ex, hits={"4": theirs})
            dead = theirs._h
        finally:
            other.close()
        assert lib.gcre_join_set_hits(ex._h, dead) == api.GCRE_ERR_ARG        # (looked up among the live lists, never followed)
        with pytest.raises(api.GcreError, match="context"):
            theirs.read()
        with pytest.raises(api.GcreError, match="context"):
            theirs.reset()
        with pytest.raises(api.GcreError, match="context"):
            api.process_paths(p, exec_=ex, hits={"4": theirs})
        with pytest.raises(api.GcreError, match="closed"):
            api.HitList(other, 0.0)
        # nothing was launched by any of it, and the untouched list reads as empty
        assert launches() == before and ex.profile()["null_kernel_launches"] == nulls
        empty = good.read()
        assert (empty.found, empty.paths, empty.complete, len(empty.score)) == (0, 0, True, 0)
        # the context still works
        res = api.process_paths(p, exec_=ex, hits={"4": good})
        got = good.read()
        assert launches() > before and got.paths == p.levels.n_paths["4"]
        assert got.found > 0 and got.score[0] == res["lst4"].scores[-1]
    finally:
        ex.close()


def test_resident_plan_refuses_lists_for_one_rank_of_several():
    p = sized("method1", "sets")
    plan = api.ResidentPlan(p)
    try:
        h = api.HitList(plan.ex, 0.0, cap=16)
        before = api._hits_lib().gcre_hits_launches(plan.ex._h)
        with pytest.raises(api.GcreError, match="world == 1"):
            plan.run(rank=0, world=2, hits={"4": h})
        assert api._hits_lib().gcre_hits_launches(plan.ex._h) == before and h.count() == (0, 0)
    finally:
        plan.close()


# ---- seeded loop ----------------------------------------------------------------------------------------------------
N_FUZZ = int(os.environ.get("GCRE_HITS_FUZZ_CASES", "6"))
FUZZ_BASE = int(os.environ.get("GCRE_HITS_FUZZ_BASE", "0"))
KNOBS = {"GCRE_CHUNK_PATHS": ["", "", "64", "200", "1000"], "GCRE_NULL_KERNEL": ["", "", "dense", "sparse", "ie"],
         "GCRE_AHEAD": ["", "0", "1"], "GCRE_WINDOW_TILES": ["", "", "1"]}


def draw(case):
    rng = np.random.default_rng(770000 + case)
    genes = int(rng.integers(25, 70))
    length = int(rng.choice([3, 4, 5]))
    edges = int(rng.integers(genes * 2, genes * (3 if length == 5 else 4)))
    cfg = dict(genes=genes, edges=edges, n_cases=int(rng.integers(20, 300)), n_ctrls=int(rng.integers(20, 300)), length=length,
               perms=int(rng.choice([0, 1, 100, 257, 2300, 4500])), method=str(rng.choice(["method1", "method2"])),
               top_k=int(rng.choice([1, 7, 40])), seed=3000 + case, threshold=float(rng.choice([0.05, 0.15, 0.4])),
               table=str(rng.choice(["hyper", "random", "ties"])), kind=str(rng.choice(KINDS + ("quantile",))),
               cap=int(rng.choice([5, 1 << 16])), passes=int(rng.integers(1, 4)), keep=bool(rng.integers(0, 2)))
    return cfg, {k: str(rng.choice(v)) for k, v in KNOBS.items()}


@pytest.mark.parametrize("case", range(N_FUZZ))
def test_random_problem_list_equals_the_reference(case, monkeypatch):
    """Random small problems (sizes, methods, path lengths, tables with ties), cut-offs of every kind, caps that overflow,
    and the knobs that change how a join runs: even cases through gcre_process_paths, odd ones through ResidentPlan."""
    number = FUZZ_BASE + case
    cfg, env = draw(number)
    import sys
    print(f"[fuzz] hits case {number}: {cfg} {env}", file=sys.stderr, flush=True)
    for k, v in env.items():
        if v:
            monkeypatch.setenv(k, v)
    rng = np.random.default_rng(cfg["seed"])
    table = None
    if cfg["table"] != "hyper":
        table = rng.random((cfg["n_cases"] + 1, cfg["n_ctrls"] + 1)) * 12.0 - 2.0
        if cfg["table"] == "ties":
            table = np.round(table)
    p = synth.make_problem(cfg["genes"], cfg["edges"], cfg["n_cases"], cfg["n_ctrls"], cfg["perms"], cfg["length"],
                           method=cfg["method"], top_k=cfg["top_k"], seed=cfg["seed"], threshold=cfg["threshold"], table=table)
    levels = LEVELS[:p.path_length]
    want = oracle_levels(p, ("fuzz", number))
    _ORACLE.pop(("fuzz", number))
    if cfg["kind"] == "quantile":
        cuts = {}
        for L, name in enumerate(levels, start=1):
            s = want[f"lst{L}"].all_scores
            s = s[np.isfinite(s)]
            cuts[name] = float(np.quantile(s, rng.random())) if len(s) else 0.0
    else:
        cuts = {}
        for L, name in enumerate(levels, start=1):
            s = want[f"lst{L}"].all_scores
            cuts[name] = cutoffs(want, cfg["kind"], levels=(name,))[name] if np.isfinite(s).any() else 0.0
    ref = reference(p, want, cuts)
    if case % 2 == 0:
        ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
        try:
            lists = make_lists(ex, cuts, cap=cfg["cap"])
            api.process_paths(p, exec_=ex, hits=lists)
            got = {k: h.read() for k, h in lists.items()}
        finally:
            ex.close()
    else:
        plan = api.ResidentPlan(p)
        try:
            for _ in range(cfg["passes"]):
                lists = make_lists(plan.ex, cuts, cap=cfg["cap"])
                plan.run(keep_inspections=cfg["keep"], hits=lists)
                got = {k: h.read() for k, h in lists.items()}
        finally:
            plan.close()
    for name in levels:
        what = f"case {number} level {name}"
        assert got[name].found == ref[name]["found"] and got[name].paths == p.levels.n_paths[name], what
        assert got[name].complete == (got[name].found <= cfg["cap"]), what
        if got[name].complete:
            assert_hits(got[name], ref[name], what)
        else:
            assert len(got[name].score) == 0, what
