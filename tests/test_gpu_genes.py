"""The per-gene best-path tally on the device (gcre_gene_tally, k_gene_fold / k_gene_index / k_gene_merge) against its numpy
definition, report.gene_best_reference, fed with every joined path's score, cases and controls from the CPU oracle.  Every
comparison is exact: scores as f64 bit patterns, integers as integers (pytest -m gpu).

GCRE_GENE_FUZZ_CASES=1000 [GCRE_GENE_FUZZ_BASE=...] for a long run of the seeded loop at the end; a handful by default."""
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


def reference(p, shard=None):
    """Level name -> gene_best_reference over the oracle's per-path scores.  Observed scores do not depend on the
    permutations: the oracle runs with one."""
    few = dataclasses.replace(p, iterations=min(p.iterations, 1), perm_cases=p.perm_cases[:1] if p.iterations else p.perm_cases)
    want = oracle.process_paths(few, order="canonical")
    tables = report.gene_tables(p.levels, len(p.data1), len(p.data2))
    out = {}
    for L, name in enumerate(LEVELS[:p.path_length], start=1):
        r = want[f"lst{L}"]
        out[name] = report.gene_best_reference(r.all_scores, r.all_cases, r.all_ctrls, p.levels.uids[name], *tables[name],
                                               report.gene_slots(name, len(p.data1), len(p.data2)),
                                               shard=None if shard is None else shard(name))
    return out


def make_tallies(ex, p):
    tables = report.gene_tables(p.levels, len(p.data1), len(p.data2))
    return {name: api.GeneTally(ex, report.gene_slots(name, len(p.data1), len(p.data2)), *tables[name])
            for name in LEVELS[:p.path_length]}


def assert_tally(got, want, what=""):
    g = got if isinstance(got, dict) else {k: getattr(got, k) for k in ("score",) + FIELDS}
    assert np.asarray(g["score"]).dtype == np.float64
    np.testing.assert_array_equal(np.asarray(g["score"]).view(np.uint64), want["score"].view(np.uint64), err_msg=f"{what} score")
    for f in FIELDS:
        np.testing.assert_array_equal(g[f], want[f], err_msg=f"{what} {f}")


def one_call(p, tallied=True):
    """gcre_process_paths with a tally on every level: (results, level name -> GeneBest)."""
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    try:
        tallies = make_tallies(ex, p) if tallied else {}
        res = api.process_paths(p, exec_=ex, tallies=tallies or None)
        return res, {k: t.read() for k, t in tallies.items()}
    finally:
        ex.close()


def plan_pass(p, passes=1, keep=False, window=None):
    """ResidentPlan passes (the launch-ahead chain, the inspection cache, permutation windows), fresh tallies per pass:
    (tallies of the last pass, its profile)."""
    plan = api.ResidentPlan(p)
    try:
        if window:
            plan.set_window(window)
        for _ in range(passes):
            tallies = make_tallies(plan.ex, p)
            plan.run(keep_inspections=keep, tallies=tallies)
            got = {k: t.read() for k, t in tallies.items()}
        return got, dict(plan.last_profile)
    finally:
        plan.close()


SIZES = {"sets": (34, 80, 61, 70, 700, 5, 9, 4242), "cache": (40, 110, 310, 335, 300, 5, 15, 21)}


def sized(method, size, K=None, table=True):
    g, e, nc, nt, perms, L, top_k, seed = SIZES[size]
    return synth.make_problem(g, e, nc, nt, perms if K is None else K, L, method=method, top_k=top_k, seed=seed,
                              table=small_table(nc + nt, nc + nt, 8) if table else None)


@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_tally_equals_the_reference_on_every_level(method, size):
    p = sized(method, size, table=size == "sets")
    want = reference(p)
    _, got = one_call(p)
    for name in LEVELS:
        assert np.isfinite(want[name]["score"]).any(), name
        assert_tally(got[name], want[name], f"{method} {size} level {name}")


def tied_problem(method):
    """Duplicate genotype rows for groups of genes, and a table of thirteen distinct values: many paths share the best score
    of a gene, so the ordinal is decided by the tie rule alone."""
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
def test_ties_go_to_the_smallest_ordinal(method):
    p = tied_problem(method)
    few = dataclasses.replace(p, iterations=1, perm_cases=p.perm_cases[:1])
    scores = oracle.process_paths(few, order="canonical")
    want = reference(p)
    _, got = one_call(p)
    tables = report.gene_tables(p.levels, len(p.data1), len(p.data2))
    for L, name in enumerate(LEVELS, start=1):
        assert_tally(got[name], want[name], f"{method} level {name}")
        if L >= 3:
            # the test bites: some gene's best score is reached by several paths through it, the winner is not the last
            all_scores = scores[f"lst{L}"].all_scores
            g0, g1 = tables[name]
            u = p.levels.uids[name]
            count = np.maximum(np.asarray(u.count, np.int64), 0)
            src = np.repeat(np.arange(len(count)), count)
            trg = np.repeat(np.asarray(u.location, np.int64), count) + np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count)
            tied = 0
            for g in np.flatnonzero(np.isfinite(want[name]["score"])).tolist():
                through = (g1[trg] == g).any(axis=1) | (g0[src] == g).any(axis=1)
                n_best = int((all_scores[through] == want[name]["score"][g]).sum())
                tied += n_best > 1
            assert tied >= 3, (name, tied)


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
_WANT = {}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_tally_does_not_depend_on_how_the_join_ran(method, variant, monkeypatch):
    """Chunk size (>= 3 chunks per join from level 3 up), a pass replayed from the inspection cache, the launch-ahead chain on
    and off, no permutations, several permutation windows, every null kernel form: the same table, the reference's."""
    env, how = VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)                 # before the context is created: gcre_create reads them
    p = sized(method, "cache", K=how.get("K"), table=False)
    if "GCRE_CHUNK_PATHS" in env:
        # a chunk is at most 64 joined paths (the path tile of the dense kernel is 64 at most): levels 3, 4, 5 run in 4, 8, 16
        assert all(p.levels.n_paths[k] >= 3 * 64 for k in ("3", "4", "5")), p.levels.n_paths
    if method not in _WANT:
        _WANT[method] = reference(p)
    want = _WANT[method]
    got, prof = plan_pass(p, passes=how.get("passes", 1), keep=how.get("keep", False), window=how.get("window"))
    if variant.startswith("ahead_on"):
        assert prof["inspect_replays"] > 0, prof     # the chain ran: later joins were inspected and launched ahead,
    if variant == "ahead_off":                       # their tallies folded from the inspection cache when they were collected
        assert prof["inspect_replays"] == 0, prof
    if variant == "cache_replay":
        assert prof["inspect_replays"] >= len(LEVELS), prof
    if variant.startswith("windows"):
        assert prof["inspect_replays"] >= 2 * len(LEVELS), prof    # three windows: the joins ran three times
    for name in LEVELS:
        assert_tally(got[name], want[name], f"{method} {variant} level {name}")
    # and through the one-call driver (no chain; it turns the cache on by itself for several windows)
    _, got2 = one_call(p)
    for name in LEVELS:
        assert_tally(got2[name], want[name], f"{method} {variant} one call, level {name}")


@pytest.mark.parametrize("chunk", ["", "64"])
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_two_shards_merge_to_the_whole(method, chunk, monkeypatch):
    """Levels 3, 4 and 5 joined in two sharded calls over [0, P/2) and [P/2, P), each into a tally of its own: each equals the
    reference restricted to its shard, and merged on the host by the rule they equal the unsharded table.  Both shards
    into ONE tally give the same."""
    monkeypatch.setenv("GCRE_AHEAD", "0")
    if chunk:
        monkeypatch.setenv("GCRE_CHUNK_PATHS", chunk)
    p = sized(method, "cache", table=False)
    whole = reference(p)
    tables = report.gene_tables(p.levels, len(p.data1), len(p.data2))
    plan = api.ResidentPlan(p)
    try:
        plan.run()                                # the kept sets of levels 1..3 are the operands below
        for name in ("3", "4", "5"):
            P = p.levels.n_paths[name]
            halves = [(0, P // 2), (P // 2, P)]
            n_slots = report.gene_slots(name, len(p.data1), len(p.data2))
            p0, p1, _ = plan.operands(name)
            parts, both = [], api.GeneTally(plan.ex, n_slots, *tables[name])
            for h in halves:
                t = api.GeneTally(plan.ex, n_slots, *tables[name])
                plan.ex.join(plan.uids[name], p0, p1, None, shard=h, tally=t)
                plan.ex.join(plan.uids[name], p0, p1, None, shard=h, tally=both)
                parts.append(t.read())
                assert_tally(parts[-1], reference_shard(p, name, h), f"{method} level {name} shard {h}")
            a, b = parts
            take_b = (b.score > a.score) | ((b.score == a.score) & (b.ordinal >= 0) & ((a.ordinal < 0) | (b.ordinal < a.ordinal)))
            merged = {k: np.where(take_b, getattr(b, k), getattr(a, k)) for k in ("score",) + FIELDS}
            assert_tally(merged, whole[name], f"{method} level {name} merged")
            assert_tally(both.read(), whole[name], f"{method} level {name} one tally")
    finally:
        plan.close()


_SHARD_SCORES = {}


def reference_shard(p, name, shard):
    key = (p.method, p.seed)
    if key not in _SHARD_SCORES:
        few = dataclasses.replace(p, iterations=1, perm_cases=p.perm_cases[:1])
        _SHARD_SCORES[key] = oracle.process_paths(few, order="canonical")
    r = _SHARD_SCORES[key][f"lst{LEVELS.index(name) + 1}"]
    tables = report.gene_tables(p.levels, len(p.data1), len(p.data2))
    return report.gene_best_reference(r.all_scores, r.all_cases, r.all_ctrls, p.levels.uids[name], *tables[name],
                                      report.gene_slots(name, len(p.data1), len(p.data2)), shard=shard)


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_a_tally_changes_nothing_else(method):
    """The joins' results -- top-k scores, ids, counts, null maxima -- are byte-identical with and without tallies, and the
    launch counters of gcre_profile are the same: the unarmed road launches what it launched before."""
    p = sized(method, "cache", table=False)
    plain, _ = one_call(p, tallied=False)
    armed, _ = one_call(p)
    for L in range(1, 6):
        a, b = plain[f"lst{L}"], armed[f"lst{L}"]
        for f in ("scores", "src", "trg", "cases", "ctrls", "null"):
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (L, f)
    for f in COUNTERS:
        assert plain["profile"][f] == armed["profile"][f], f
    again, _ = one_call(p, tallied=False)
    for f in COUNTERS:
        assert plain["profile"][f] == again["profile"][f], f


def _network_case(seed, nc=48, nt=52):
    rng = np.random.default_rng(seed)
    g, src, trg, sign = synth.signed_network(60, 200, rng)
    uid = np.arange(g) * 5 + 100
    symbols = [f"G{u}" for u in uid]
    data = (rng.random((g, nc + nt)) < 0.06).astype(np.int32)
    return symbols, data, (uid, symbols, uid[src], uid[trg], sign)


@pytest.mark.parametrize("signed", [False, True])
def test_gwaspa_gene_table(signed):
    from geneticscre_amd.uids import UidRelSet
    nc, nt, K, L = 48, 52, 3000, 5
    genes, data, network = _network_case(17)
    strata = (np.arange(nc + nt) * 5 % 3).astype(np.int32)
    kw = dict(signed=signed, threshold=0.2, n_permutations=K, strata=strata, seed=909, top_k=6, path_length=L)
    base = report.gwaspa(genes, data, nc, nt, network, **kw)
    assert set(base) == {"GWASPA.Results", "levels", "prepared"}            # the default output is what it was
    out = report.gwaspa(genes, data, nc, nt, network, gene_table=True, **kw)
    assert set(out) == set(base) | {"Gene.Results", "gene_best"}
    assert out["GWASPA.Results"].equals(base["GWASPA.Results"])
    df = out["Gene.Results"]
    assert list(df.columns) == report.GENE_COLUMNS

    # the reference: the same problem, rebuilt from the prepared inputs, through the oracle
    prep = out["prepared"]
    g, n2 = len(prep.ents_uid), len(prep.ents2_uid)
    levels = api.build_levels(g, prep.src, prep.trg, prep.sign)
    ids2 = np.arange(n2, dtype=np.int32)
    levels.uids["1b"] = UidRelSet(1, ids2, ids2, np.ones(n2, np.int32), np.arange(n2, dtype=np.int64), np.ones(n2, np.int32))
    levels.data_inds["1b"] = ids2.copy()
    levels.n_paths["1b"] = n2
    p = synth.Problem("method2" if signed else "method1", nc, nt, L, 6, 0, levels, prep.data1, prep.data2,
                      api.values_table(nc, nt), np.zeros((0, 0), np.int32), 0)
    want = reference(p)
    for i, name in enumerate(LEVELS, start=1):
        assert_tally(out["gene_best"][i], want[name], f"level {name}")
    frames = report.frames_of(prep, levels)
    ents, ents2 = (prep.ents_uid, prep.ents_symbol), (prep.ents2_uid, prep.ents2_symbol)
    expect = report.gene_results({i: want[name] for i, name in enumerate(LEVELS, start=1)}, out["levels"], frames, ents, ents2)
    assert len(df) == len(expect) == sum(int(np.isfinite(want[name]["score"]).sum()) for name in LEVELS)
    for c in report.GENE_COLUMNS:
        if c in ("Scores", "Pvalues"):
            np.testing.assert_array_equal(df[c].to_numpy(np.float64).view(np.uint64), expect[c].to_numpy(np.float64).view(np.uint64))
        else:
            assert df[c].tolist() == expect[c].tolist(), c
    # p-values: the length's null maxima, f64 score against f32 maxima; ordered like GWASPA.Results
    for Lx in range(1, L + 1):
        rows = df[df["Lengths"] == Lx]
        pv = report._tail_pvalues(out["levels"][f"lst{Lx}"].null, rows["Scores"].to_numpy(np.float64))
        np.testing.assert_array_equal(rows["Pvalues"].to_numpy(np.float64), pv)
    pcol, scol = df["Pvalues"].to_numpy(), df["Scores"].to_numpy()
    assert all((pcol[i], -scol[i]) <= (pcol[i + 1], -scol[i + 1]) for i in range(len(df) - 1))
    # every GWASPA.Results row: each of its genes has a row of that length that scores at least as high
    best_of = {(gene, int(Lx)): s for gene, Lx, s in zip(df["Gene"], df["Lengths"], df["Scores"])}
    checked = 0
    for path, Lx, s in zip(out["GWASPA.Results"]["Paths"], out["GWASPA.Results"]["Lengths"], out["GWASPA.Results"]["Scores"]):
        if "NA" in path.split(" -> ") or not np.isfinite(s):
            continue
        for gene in path.split(" -> "):
            assert best_of[(gene, int(Lx))] >= s, (gene, Lx)
            checked += 1
    assert checked > 20
    summary = report.gene_summary(df)
    assert summary["Gene"].is_unique and set(summary["Gene"]) == set(df["Gene"])
    for gene, pmin in df.groupby("Gene")["Pvalues"].min().items():
        assert summary.loc[summary["Gene"] == gene, "Pvalues"].iat[0] == pmin


def test_refusals():
    p = sized("method1", "sets")
    n_genes, n_genes2 = len(p.data1), len(p.data2)
    tables = report.gene_tables(p.levels, n_genes, n_genes2)
    g0, g1 = tables["4"]
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    lib = api._genes_lib()
    try:
        # malformed tables: in Python, and by the library itself
        with pytest.raises(api.GcreError, match="outside"):
            api.GeneTally(ex, n_genes - 1, g0, g1)
        with pytest.raises(api.GcreError):
            api.GeneTally(ex, n_genes, np.zeros((len(g0), 4), np.int32), g1)
        bad = np.ascontiguousarray(g1.copy())
        bad[0, 0] = n_genes
        h = lib.gcre_gene_tally_create(ex._h, n_genes, api._ptr(g0), len(g0), g0.shape[1], api._ptr(bad), len(bad), bad.shape[1])
        assert not h and b"outside" in lib.gcre_last_error(ex._h)
        h = lib.gcre_gene_tally_create(ex._h, n_genes, api._ptr(g0), len(g0), 4, api._ptr(g1), len(g1), g1.shape[1])
        assert not h and b"width" in lib.gcre_last_error(ex._h)
        assert not lib.gcre_gene_tally_create(ex._h, 0, None, 0, 0, api._ptr(g1), len(g1), g1.shape[1])
        # a tally whose rows do not fit the join: the one-call driver (Python check), a resident index (the library's)
        wrong = api.GeneTally(ex, n_genes, *tables["3"])
        with pytest.raises(api.GcreError, match="uid rows|paths1 row"):
            api.process_paths(p, exec_=ex, tallies={"4": wrong})
        keep = []
        inp = api._pp_input(p, keep)
        assert lib.gcre_process_paths_set_tally(ex._h, 4, wrong._h) == 0
        outs = (api.gcre_result * 5)()
        assert ex._lib.gcre_process_paths(ex._h, ctypes.byref(inp), outs) == api.GCRE_ERR_ARG
        assert b"gene tally" in lib.gcre_last_error(ex._h)
        assert lib.gcre_process_paths_set_tally(ex._h, 6, wrong._h) == api.GCRE_ERR_ARG
        # one device of several: refused by the library; the several-device driver: refused in Python
        good = api.GeneTally(ex, n_genes, g0, g1)
        assert lib.gcre_process_paths_set_tally(ex._h, 4, good._h) == 0
        inp.shard_rank, inp.shard_world = 0, 2
        assert ex._lib.gcre_process_paths(ex._h, ctypes.byref(inp), outs) == api.GCRE_ERR_ARG
        assert b"several" in lib.gcre_last_error(ex._h)
        with pytest.raises(api.GcreError, match="tallies"):
            api.process_paths_devices(p, devices=[0, 0], tallies={"4": good})
        # a tally of another context
        other = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
        try:
            assert lib.gcre_join_set_tally(other._h, good._h) == api.GCRE_ERR_ARG
        finally:
            other.close()
        # the context still works, and an untouched tally reads as empty
        res = api.process_paths(p, exec_=ex, tallies={"4": good})
        assert res["lst4"].scores[-1] == good.read().score.max()
        empty = wrong.read()
        assert np.isneginf(empty.score).all() and (empty.ordinal == -1).all() and (empty.src == -1).all() and not empty.cases.any()
    finally:
        ex.close()


# ---- seeded loop ----------------------------------------------------------------------------------------------------
N_FUZZ = int(os.environ.get("GCRE_GENE_FUZZ_CASES", "6"))
FUZZ_BASE = int(os.environ.get("GCRE_GENE_FUZZ_BASE", "0"))


@pytest.mark.parametrize("case", range(N_FUZZ))
def test_random_problem_tally_equals_the_reference(case, monkeypatch):
    """tests/test_gpu_fuzz.py's draw (sizes, methods, path lengths, tables with ties, kernel forms, chunk sizes, windows,
    the chain) under case numbers of its own: even cases through gcre_process_paths, odd ones through ResidentPlan."""
    from test_gpu_fuzz import draw, entered, value_table
    number = 500000 + FUZZ_BASE + case
    entered("gene_tally", number)
    cfg, env = draw(number)
    for k, v in env.items():
        if v:
            monkeypatch.setenv(k, v)
    p = synth.make_problem(cfg["genes"], cfg["edges"], cfg["n_cases"], cfg["n_ctrls"], cfg["perms"], cfg["length"],
                           method=cfg["method"], top_k=cfg["top_k"], seed=cfg["seed"], threshold=cfg["threshold"],
                           table=value_table(cfg["table"], cfg["n_cases"], cfg["n_ctrls"], cfg["seed"]))
    want = reference(p)
    if case % 2 == 0:
        _, got = one_call(p)
    else:
        got, _ = plan_pass(p, passes=1 + case % 3, keep=case % 4 == 1)
    for name in LEVELS[:p.path_length]:
        assert_tally(got[name], want[name], f"case {number} level {name}")
