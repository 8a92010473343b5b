"""Null exceedance counts on the device (gcre_exceed: k_exceed_ie, k_exceed_dense, k_exceed_observed) against their numpy
definition, report.exceed_reference, fed with operand rows, scores and null maxima from the CPU oracle.  Every comparison
of counts is exact (pytest -m gpu).

GCRE_EXCEED_FUZZ_CASES=1000 [GCRE_EXCEED_FUZZ_BASE=...] for a long run of the seeded loop at the end; a handful by default."""
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


class Cpu:
    """What the definition needs, from the CPU oracle: every level's results, operand rows and the permutation masks."""

    def __init__(self, p, nthreads=0):
        self.p = p
        self.want = oracle.process_paths(p, order="canonical", nthreads=nthreads)
        ox = oracle.OracleJoinExec(p.method, p.n_cases, p.n_ctrls, 0)
        lv, w = p.levels, self.want
        parsed1, parsed2 = ox.load(p.data1), ox.load(p.data2)
        self.ops = {"1b": (ox.create_path_set(len(lv.data_inds["1b"])), parsed2[lv.data_inds["1b"]])}
        if p.path_length >= 2:
            self.ops["2"] = (w["paths1"], parsed1[lv.data_inds["2"]])
        if p.path_length >= 3:
            self.ops["3"] = (w["paths2"], parsed1[lv.data_inds["3"]])
        if p.path_length >= 4:
            self.ops["4"] = (w["paths3"], w["paths2"])
        if p.path_length >= 5:
            self.ops["5"] = (w["paths3"], w["paths3"])
        n = p.n_cases + p.n_ctrls
        if p.iterations > 0:      # setPermutedCases: anything but 1 flips the patient's label (rows reused when there are fewer)
            pc = np.asarray(p.perm_cases)
            pc = pc[np.arange(p.iterations) % len(pc)]
            self.masks = (np.arange(n) < p.n_cases)[None, :] ^ (pc != 1)
        else:
            self.masks = np.zeros((0, n), bool)

    def thresholds(self, name, extra=()):
        """The level's finite top-K scores, three quantiles of its null maxima, one value <= 0, one above every null value."""
        r = self.want[f"lst{LEVELS.index(name) + 1}"]
        s = r.scores[np.isfinite(r.scores)]
        q = np.quantile(r.null.astype(np.float64), [0.1, 0.5, 0.9]) if len(r.null) else np.zeros(0)
        return np.concatenate([s, q, [-1.0, 1e30], np.asarray(extra, np.float64)])

    def reference(self, name, thr, shard=None, window=None):
        p = self.p
        return report.exceed_reference(p.method, p.n_cases, p.n_ctrls, p.levels.uids[name], *self.ops[name], p.value_table,
                                       self.masks, thr, shard=shard, window=window)


def assert_counts(got, want, what="", observed_calls=1, perms=None):
    np.testing.assert_array_equal(got.exceed, want["exceed"], err_msg=f"{what} exceed")
    np.testing.assert_array_equal(got.observed, want["observed"] * np.uint64(observed_calls), err_msg=f"{what} observed")
    assert got.paths == want["paths"] * observed_calls, what
    assert got.perms == (want["perms"] if perms is None else perms), what


def bites(want):
    """Some threshold is neither never nor always exceeded: the expected values can tell a wrong count from a right one."""
    full = want["paths"] * want["perms"]
    return any(0 < int(e) < full for e in want["exceed"])


SIZES = {"sets": (34, 80, 61, 70, 700, 5, 9, 4242), "cache": (40, 110, 310, 335, 300, 5, 15, 21)}
_CPU = {}


def sized(method, size, K=None, table=True):
    g, e, nc, nt, perms, L, top_k, seed = SIZES[size]
    return synth.make_problem(g, e, nc, nt, perms if K is None else K, L, method=method, top_k=top_k, seed=seed,
                              table=small_table(nc + nt, nc + nt, 8) if table else None)


def cpu_of(method, size, K=None, table=True):
    key = (method, size, K, table)
    if key not in _CPU:
        _CPU[key] = Cpu(sized(method, size, K, table))
    return _CPU[key]


def make_counters(ex, cpu, names=None, extra=()):
    return {name: api.ExceedCounts(ex, cpu.thresholds(name, extra)) for name in (names or LEVELS[:cpu.p.path_length])}


def one_call(p, cpu=None, names=None):
    """gcre_process_paths, counters on the levels named (all of them by default): (results, level name -> Exceedances)."""
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    try:
        xs = make_counters(ex, cpu, names) if cpu is not None else {}
        res = api.process_paths(p, exec_=ex, exceeds=xs or None)
        return res, {k: x.read() for k, x in xs.items()}
    finally:
        ex.close()


def plan_pass(p, cpu=None, passes=1, keep=False, window=None):
    """ResidentPlan passes (the launch-ahead chain, the inspection cache, permutation windows), fresh counters per pass:
    (results and counters of the last pass, its profile)."""
    plan = api.ResidentPlan(p)
    try:
        if window:
            plan.set_window(window)
        got = {}
        for _ in range(passes):
            xs = make_counters(plan.ex, cpu) if cpu is not None else {}
            res = plan.run(keep_inspections=keep, exceeds=xs or None)
            got = {k: x.read() for k, x in xs.items()}
        return res, got, dict(plan.last_profile)
    finally:
        plan.close()


def same_results(a, b, names):
    for name in names:
        for f in ("scores", "src", "trg", "cases", "ctrls", "null"):
            assert getattr(a[name], f).tobytes() == getattr(b[name], f).tobytes(), (name, f)


# ---- 1. the definition, bit for bit ---------------------------------------------------------------------------------


@pytest.mark.parametrize("size", sorted(SIZES))
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_counts_equal_the_definition_on_every_level(method, size):
    cpu = cpu_of(method, size, table=size == "sets")
    p = cpu.p
    res, got = one_call(p, cpu)
    for L, name in enumerate(LEVELS, start=1):
        thr = cpu.thresholds(name)
        want = cpu.reference(name, thr)
        np.testing.assert_array_equal(want["scores"].view(np.uint64), cpu.want[f"lst{L}"].all_scores.view(np.uint64))
        assert bites(want), (method, size, name, want["exceed"])
        assert want["exceed"][-2] == want["paths"] * p.iterations and want["exceed"][-1] == 0     # the value <= 0, the one above all
        assert_counts(got[name], want, f"{method} {size} level {name}")
    # the masks the definition was fed are the context's
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    try:
        ex.set_permuted_cases(p.perm_cases)
        for r in (0, 1, p.iterations - 1):
            np.testing.assert_array_equal(ex.perm_mask(r), api.pack_carriers(cpu.masks[r:r + 1], p.n_cases + p.n_ctrls)[0])
    finally:
        ex.close()


@pytest.mark.parametrize("form", ["ie", "dense"])
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_ten_thousand_thresholds(method, form, monkeypatch):
    """m = 10,000 (more than a block's histogram holds: the bins are global), in no order, with repeats."""
    monkeypatch.setenv("GCRE_NULL_KERNEL", "ie")
    monkeypatch.setenv("GCRE_EXCEED_KERNEL", form)
    cpu = cpu_of(method, "sets")
    p = cpu.p
    rng = np.random.default_rng(3)
    null = cpu.want["lst4"].null.astype(np.float64)
    thr = rng.uniform(null.min() * 0.5, null.max() * 1.01, size=api.EXCEED_MAX)
    thr[::7] = thr[3]
    thr[5] = -np.inf
    thr[6] = np.inf
    want = cpu.reference("4", thr)
    assert bites(want) and len(set(want["exceed"].tolist())) > 50
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    try:
        x = api.ExceedCounts(ex, thr)
        api.process_paths(p, exec_=ex, exceeds={"4": x})
        assert_counts(x.read(), want, f"{method} {form}")
    finally:
        ex.close()


# ---- 2. invariance --------------------------------------------------------------------------------------------------

VARIANTS = {
    "plain": ({}, {}),
    "chunks": ({"GCRE_CHUNK_PATHS": "64"}, {}),
    "chunks_dense": ({"GCRE_CHUNK_PATHS": "64", "GCRE_NULL_KERNEL": "dense"}, {}),
    "chunks_ie": ({"GCRE_CHUNK_PATHS": "64", "GCRE_NULL_KERNEL": "ie"}, {}),
    "cache_replay": ({}, {"passes": 2, "keep": True}),
    "ahead_off": ({"GCRE_AHEAD": "0"}, {}),
    "ahead_on": ({"GCRE_AHEAD": "1"}, {}),
    "ahead_on_chunks": ({"GCRE_AHEAD": "1", "GCRE_CHUNK_PATHS": "64"}, {}),
    "ahead_on_ie": ({"GCRE_AHEAD": "1", "GCRE_NULL_KERNEL": "ie"}, {"form": "ie"}),
    "ahead_on_ie_chunks": ({"GCRE_AHEAD": "1", "GCRE_NULL_KERNEL": "ie", "GCRE_CHUNK_PATHS": "64"}, {"form": "ie"}),
    "sparse": ({"GCRE_NULL_KERNEL": "sparse"}, {}),
    "dense": ({"GCRE_NULL_KERNEL": "dense"}, {}),
    "ie": ({"GCRE_NULL_KERNEL": "ie", "GCRE_AHEAD": "0"}, {"form": "ie"}),
    "ie_no_prune": ({"GCRE_NULL_KERNEL": "ie", "GCRE_IE_PRUNE": "0", "GCRE_AHEAD": "0"}, {"form": "ie"}),
    "ie_counted_dense": ({"GCRE_NULL_KERNEL": "ie", "GCRE_EXCEED_KERNEL": "dense", "GCRE_AHEAD": "0"}, {"form": "dense"}),
    "ie_counted_ie": ({"GCRE_NULL_KERNEL": "ie", "GCRE_EXCEED_KERNEL": "ie", "GCRE_AHEAD": "0"}, {"form": "ie"}),
    "windows": ({"GCRE_WINDOW_TILES": "1"}, {"K": 5000, "window": 2048}),
    "windows_ie": ({"GCRE_WINDOW_TILES": "1", "GCRE_NULL_KERNEL": "ie", "GCRE_AHEAD": "0"}, {"K": 5000, "window": 2048, "form": "ie"}),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_counts_do_not_depend_on_how_the_join_ran(method, variant, monkeypatch, capfd):
    """Chunk size (>= 3 chunks per join from level 3 up), a pass replayed from the inspection cache, the launch-ahead chain on
    and off, every null kernel form, pruning off, either counting form, several permutation windows: the definition's
    counts, and the joins' own results byte for byte those of a pass without counters."""
    env, how = VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)                 # before the context is created: gcre_create reads them
    monkeypatch.setenv("GCRE_EXCEED_TRACE", "1")
    cpu = cpu_of(method, "cache", K=how.get("K"), table=False)
    p = cpu.p
    if "GCRE_CHUNK_PATHS" in env:
        assert all(p.levels.n_paths[k] >= 3 * 64 for k in ("3", "4", "5")), p.levels.n_paths
    capfd.readouterr()
    res, got, prof = plan_pass(p, cpu, passes=how.get("passes", 1), keep=how.get("keep", False), window=how.get("window"))
    err = capfd.readouterr().err
    plain, _, _ = plan_pass(p, None, passes=how.get("passes", 1), keep=how.get("keep", False), window=how.get("window"))
    same_results(res, plain, LEVELS)
    if variant.startswith("ahead_on"):
        assert prof["inspect_replays"] > 0, prof     # the chain ran: later joins were counted by a pass over the inspection cache
    if variant == "cache_replay":
        assert prof["inspect_replays"] >= len(LEVELS), prof
    if how.get("form") == "ie":
        assert "[exceed] ie form" in err, err[-400:]
    if how.get("form") == "dense" or env.get("GCRE_NULL_KERNEL") in ("dense", "sparse"):
        assert "[exceed] dense form" in err and "[exceed] ie form" not in err, err[-400:]
    windows = len(range(0, p.iterations, how["window"])) if how.get("window") else 1
    for name in LEVELS:
        want = cpu.reference(name, cpu.thresholds(name))
        assert bites(want), (method, variant, name)
        assert_counts(got[name], want, f"{method} {variant} level {name}", observed_calls=windows)
    # and through the one-call driver (no chain; it walks the windows itself and counts the observed scores once)
    res2, got2 = one_call(p, cpu)
    for name in LEVELS:
        assert_counts(got2[name], cpu.reference(name, cpu.thresholds(name)), f"{method} {variant} one call, level {name}")
    same_results({n: res2[f"lst{i}"] for i, n in enumerate(LEVELS, start=1)}, plain, LEVELS)


# ---- 3. additivity --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("chunk", ["", "64"])
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_shards_windows_and_repeats_add(method, chunk, monkeypatch):
    monkeypatch.setenv("GCRE_AHEAD", "0")
    monkeypatch.setenv("GCRE_WINDOW_TILES", "2")
    if chunk:
        monkeypatch.setenv("GCRE_CHUNK_PATHS", chunk)
    cpu = cpu_of(method, "cache", K=4096, table=False)
    p = cpu.p
    K = p.iterations
    plan = api.ResidentPlan(p)
    try:
        plan.set_window(K)
        plan.run()                                # the kept sets of levels 1..3 are the operands below
        ex = plan.ex
        for name in ("3", "4", "5"):
            P = p.levels.n_paths[name]
            thr = cpu.thresholds(name)
            whole = cpu.reference(name, thr)
            assert bites(whole)
            p0, p1, _ = plan.operands(name)
            # two shards: each the definition restricted to it, their sum the whole; both into one object the same
            halves = [(0, P // 3), (P // 3, P)]
            both, parts = api.ExceedCounts(ex, thr), []
            for h in halves:
                x = api.ExceedCounts(ex, thr)
                ex.join(plan.uids[name], p0, p1, None, shard=h, exceed=x)
                ex.join(plan.uids[name], p0, p1, None, shard=h, exceed=both)
                parts.append(x.read())
                assert_counts(parts[-1], cpu.reference(name, thr, shard=h), f"{method} level {name} shard {h}")
            np.testing.assert_array_equal(parts[0].exceed + parts[1].exceed, whole["exceed"])
            np.testing.assert_array_equal(parts[0].observed + parts[1].observed, whole["observed"])
            assert_counts(both.read(), whole, f"{method} level {name} one object", perms=2 * K)   # (two joins: perms says so)
            # two permutation windows of 2048: each the definition on its window, their sum the 4096-permutation run
            x = api.ExceedCounts(ex, thr)
            for w in ((0, 2048), (2048, 4096)):
                ex.set_perm_window(*w)
                y = api.ExceedCounts(ex, thr)
                ex.join(plan.uids[name], p0, p1, None, exceed=y)
                ex.join(plan.uids[name], p0, p1, None, exceed=x)
                assert_counts(y.read(), cpu.reference(name, thr, window=w), f"{method} level {name} window {w}")
            ex.set_perm_window(0, K)
            got = x.read()
            np.testing.assert_array_equal(got.exceed, whole["exceed"])
            assert got.perms == 4096 and got.paths == 2 * P
            # an armed join repeated without reset doubles, and says so; reset starts over; an unarmed join adds nothing
            ex.join(plan.uids[name], p0, p1, None, exceed=both)
            again = both.read()
            np.testing.assert_array_equal(again.exceed, 2 * whole["exceed"])
            np.testing.assert_array_equal(again.observed, 2 * whole["observed"])
            assert (again.perms, again.paths) == (3 * K, 2 * P)
            ex.join(plan.uids[name], p0, p1, None)
            assert both.read().perms == 3 * K
            both.reset()
            z = both.read()
            assert not z.exceed.any() and not z.observed.any() and (z.perms, z.paths) == (0, 0)
            ex.join(plan.uids[name], p0, p1, None, exceed=both)
            assert_counts(both.read(), whole, f"{method} level {name} after reset")
    finally:
        plan.close()


# ---- 4. ties to what exists -----------------------------------------------------------------------------------------


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_counts_against_the_null_maxima_and_the_top_k(method):
    cpu = cpu_of(method, "cache", table=False)
    p = cpu.p
    res, got = one_call(p, cpu)
    for L, name in enumerate(LEVELS, start=1):
        thr = cpu.thresholds(name)
        r = res[f"lst{L}"]
        null = r.null.astype(np.float64)
        for j, t in enumerate(thr):
            n_max = int((null >= t).sum())        # permutations whose maximum reaches t: each holds at least one such path
            assert n_max <= got[name].exceed[j], (name, t)
            assert (n_max == 0) == (got[name].exceed[j] == 0), (name, t)
        s = r.scores[np.isfinite(r.scores)]
        k = len(s)
        assert got[name].observed[0] >= k        # thr[0] = the smallest kept score: at least the kept rows reach it
        np.testing.assert_array_equal(got[name].observed[:k] >= (k - np.arange(k)), True)


def test_observed_counts_past_the_cut_when_scores_tie():
    """The shape of the golden m1_all_ties (tests/golden/make_ref_goldens.py): a flat table, every path scores 1.5, top_k = 11:
    the K-th top score is reached by every scored path, not by K."""
    p = synth.make_problem(20, 50, 16, 16, 6, 4, method="method1", top_k=11, seed=107, table=np.full((17, 17), 1.5))
    cpu = Cpu(p)
    res, got = one_call(p, cpu)
    for L, name in enumerate(LEVELS[:4], start=1):
        P = p.levels.n_paths[name]
        want = cpu.reference(name, cpu.thresholds(name))
        assert_counts(got[name], want, name)
        if P > p.top_k:
            assert got[name].observed[0] == P > p.top_k
            assert got[name].exceed[0] == P * p.iterations      # every null value is 1.5 too


# ---- 5. mid size, two forms -----------------------------------------------------------------------------------------


def two_forms(p, thr_of, monkeypatch, names):
    out = {}
    for form in ("ie", "dense"):
        monkeypatch.setenv("GCRE_EXCEED_KERNEL", form)
        ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
        try:
            xs = {name: api.ExceedCounts(ex, thr_of[name]) for name in names}
            api.process_paths(p, exec_=ex, exceeds=xs)
            out[form] = {k: x.read() for k, x in xs.items()}
        finally:
            ex.close()
    return out


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_mid_size_both_forms_and_the_definition(method, monkeypatch, capfd):
    """configs[2] geometry (5,000 patients, 79 mask words, K not a multiple of the tile) on the 220-gene / 800-edge network of
    tests/test_gpu_parity.py: the two counting forms agree on every level, and with the definition where numpy affords it
    (levels up to 3)."""
    monkeypatch.setenv("GCRE_EXCEED_TRACE", "1")
    p = synth.make_problem(220, 800, 2500, 2500, 1100, 4, method=method, top_k=50, seed=77)
    plain = api.process_paths(p)
    names = LEVELS[:4]
    thr_of = {}
    for L, name in enumerate(names, start=1):
        r = plain[f"lst{L}"]
        thr_of[name] = np.concatenate([r.scores[np.isfinite(r.scores)], np.quantile(r.null.astype(np.float64), [0.1, 0.5, 0.9]),
                                       [0.0, 1e30]])
    capfd.readouterr()
    out = two_forms(p, thr_of, monkeypatch, names)
    err = capfd.readouterr().err
    assert "[exceed] ie form" in err and "[exceed] dense form" in err
    for name in names:
        a, b = out["ie"][name], out["dense"][name]
        np.testing.assert_array_equal(a.exceed, b.exceed, err_msg=name)
        np.testing.assert_array_equal(a.observed, b.observed, err_msg=name)
        assert (a.perms, a.paths) == (b.perms, b.paths) == (p.iterations, p.levels.n_paths[name])
        assert a.exceed[-2] == a.paths * a.perms and a.exceed[-1] == 0
        assert any(0 < int(e) < a.paths * a.perms for e in a.exceed), name
    cpu = Cpu(dataclasses.replace(p, path_length=3), nthreads=8)
    for name in names[:3]:
        assert_counts(out["ie"][name], cpu.reference(name, thr_of[name]), f"{method} level {name}")


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_large_network_both_forms(method, monkeypatch):
    """3,000 genes / 30,000 edges at 5,000 patients (the run of test_full_size_properties_without_oracle), no oracle: the two
    forms agree, the counts are consistent with the null maxima and with each other (monotone in the threshold)."""
    p = synth.make_problem(3000, 30000, 2500, 2500, 2000, 4, method=method, top_k=64, seed=99)
    plain = api.process_paths(p)
    names = LEVELS[:4]
    thr_of = {}
    for L, name in enumerate(names, start=1):
        r = plain[f"lst{L}"]
        # (-1, not 0: the hypergeometric table's -log of a p-value that rounds to 1 is a few ulps below zero here and there)
        thr_of[name] = np.concatenate([np.sort(r.scores[np.isfinite(r.scores)]), np.quantile(r.null.astype(np.float64), [0.5, 0.99]),
                                       [-1.0, 1e30]])
    out = two_forms(p, thr_of, monkeypatch, names)
    for L, name in enumerate(names, start=1):
        a, b = out["ie"][name], out["dense"][name]
        np.testing.assert_array_equal(a.exceed, b.exceed, err_msg=name)
        np.testing.assert_array_equal(a.observed, b.observed, err_msg=name)
        P = p.levels.n_paths[name]
        assert (a.perms, a.paths) == (p.iterations, P)
        assert a.exceed[-2] == P * p.iterations and a.exceed[-1] == 0 and a.observed[-2] == P
        null = plain[f"lst{L}"].null.astype(np.float64)
        order = np.argsort(thr_of[name])
        assert (np.diff(a.exceed[order].astype(np.int64)) <= 0).all() and (np.diff(a.observed[order].astype(np.int64)) <= 0).all()
        for j, t in enumerate(thr_of[name]):
            assert int((null >= t).sum()) <= a.exceed[j] and ((null >= t).any() == (a.exceed[j] > 0))
        k = int(np.isfinite(plain[f"lst{L}"].scores).sum())
        assert a.observed[0] >= k


# ---- 6. the front end -----------------------------------------------------------------------------------------------


def _network_case(seed, nc=48, nt=52):
    rng = np.random.default_rng(seed)
    g, src, trg, sign = synth.signed_network(60, 200, rng)
    uid = np.arange(g) * 5 + 100
    symbols = [f"G{u}" for u in uid]
    data = (rng.random((g, nc + nt)) < 0.06).astype(np.int32)
    return symbols, data, (uid, symbols, uid[src], uid[trg], sign)


@pytest.mark.parametrize("signed", [False, True])
def test_gwaspa_fdr_columns(signed):
    from geneticscre_amd.uids import UidRelSet
    nc, nt, K, L = 48, 52, 3000, 5
    genes, data, network = _network_case(17)
    strata = (np.arange(nc + nt) * 5 % 3).astype(np.int32)
    kw = dict(signed=signed, threshold=0.2, n_permutations=K, strata=strata, seed=909, top_k=6, path_length=L)
    base = report.gwaspa(genes, data, nc, nt, network, **kw)
    assert set(base) == {"GWASPA.Results", "levels", "prepared"}            # the default output is what it was
    out = report.gwaspa(genes, data, nc, nt, network, fdr=True, **kw)
    assert set(out) == set(base) | {"exceed"}
    df = out["GWASPA.Results"]
    assert list(df.columns) == report.COLUMNS + report.FDR_COLUMNS
    assert df[report.COLUMNS].equals(base["GWASPA.Results"])               # the seven columns and the row order
    # the definition: the same problem rebuilt from the prepared inputs, the masks read back from a context
    prep = out["prepared"]
    g, n2 = len(prep.ents_uid), len(prep.ents2_uid)
    levels = api.build_levels(g, prep.src, prep.trg, prep.sign)
    ids2 = np.arange(n2, dtype=np.int32)
    levels.uids["1b"] = UidRelSet(1, ids2, ids2, np.ones(n2, np.int32), np.arange(n2, dtype=np.int64), np.ones(n2, np.int32))
    levels.data_inds["1b"] = ids2.copy()
    levels.n_paths["1b"] = n2
    method = "method2" if signed else "method1"
    ex = api.JoinExec(method, nc, nt, K)
    try:
        ex.generate_permutations(909, strata)
        words = np.stack([ex.perm_mask(r) for r in range(K)])
    finally:
        ex.close()
    masks = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :nc + nt].astype(bool)
    p = synth.Problem(method, nc, nt, L, 6, K, levels, prep.data1, prep.data2, api.values_table(nc, nt),
                      np.ones((1, nc + nt), np.int32), 0)
    cpu = Cpu(p)
    cpu.masks = masks
    some = False
    for Lx, name in enumerate(LEVELS, start=1):
        s = out["levels"][f"lst{Lx}"].scores
        thr = s[np.isfinite(s)]
        want = cpu.reference(name, thr)
        got = out["exceed"][Lx]
        np.testing.assert_array_equal(got.exceed, want["exceed"])
        np.testing.assert_array_equal(got.observed, want["observed"])
        assert (got.perms, got.paths) == (K, want["paths"])
        cols = report.fdr_columns(thr, want["exceed"], want["observed"], K)
        rows = df[df["Lengths"] == Lx]
        by_score = {t: i for i, t in enumerate(thr.tolist())}
        for c in report.FDR_COLUMNS:
            exp = np.array([cols[c][by_score[sc]] if np.isfinite(sc) else np.nan for sc in rows["Scores"]])
            np.testing.assert_array_equal(rows[c].to_numpy(np.float64), exp)
        q = rows.sort_values("Scores", ascending=False, kind="stable")["Qvalues"].to_numpy(np.float64)
        q = q[~np.isnan(q)]
        assert (q <= 1).all() and (np.diff(q) >= 0).all()
        some = some or bool(((q > 0) & (q < 1)).any())
    assert some     # not all zeros and ones: the columns say something on this case


# ---- 7. errors ------------------------------------------------------------------------------------------------------


def test_refusals():
    cpu = cpu_of("method1", "sets")
    p = cpu.p
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    lib = api._exceed_lib()
    try:
        before = ex.profile()["null_kernel_launches"]
        one = np.array([1.0, np.nan, 2.0])
        assert not lib.gcre_exceed_create(ex._h, api._ptr(one), 3) and b"NaN" in lib.gcre_last_error(ex._h)
        assert not lib.gcre_exceed_create(ex._h, api._ptr(one), 0) and b"1..10000" in lib.gcre_last_error(ex._h)
        big = np.zeros(api.EXCEED_MAX + 1)
        assert not lib.gcre_exceed_create(ex._h, api._ptr(big), len(big)) and b"1..10000" in lib.gcre_last_error(ex._h)
        assert not lib.gcre_exceed_create(ex._h, None, 3)
        with pytest.raises(api.GcreError, match="NaN"):
            api.ExceedCounts(ex, [1.0, float("nan")])
        with pytest.raises(api.GcreError, match="1..10000"):
            api.ExceedCounts(ex, [])
        good = api.ExceedCounts(ex, cpu.thresholds("4"))
        assert lib.gcre_process_paths_set_exceed(ex._h, 6, good._h) == api.GCRE_ERR_ARG
        # one device of several: refused by the library before anything runs
        keep = []
        inp = api._pp_input(p, keep)
        outs = (api.gcre_result * 5)()
        assert lib.gcre_process_paths_set_exceed(ex._h, 4, good._h) == 0
        inp.shard_rank, inp.shard_world = 0, 2
        assert ex._lib.gcre_process_paths(ex._h, ctypes.byref(inp), outs) == api.GCRE_ERR_ARG
        assert b"several" in lib.gcre_last_error(ex._h)
        assert ex.profile()["null_kernel_launches"] == before
        z = good.read()
        assert not z.exceed.any() and not z.observed.any() and (z.perms, z.paths) == (0, 0)
        # counters of another context
        other = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
        try:
            assert lib.gcre_join_set_exceed(other._h, good._h) == api.GCRE_ERR_ARG
            with pytest.raises(api.GcreError, match="context"):
                api.process_paths(p, exec_=other, exceeds={"4": good})
        finally:
            other.close()
        with pytest.raises(api.GcreError, match="no level"):
            api.process_paths(p, exec_=ex, exceeds={"7": good})
        # the context still works; a tally and counters on the same join
        tables = report.gene_tables(p.levels, len(p.data1), len(p.data2))
        tally = api.GeneTally(ex, len(p.data1), *tables["4"])
        res = api.process_paths(p, exec_=ex, exceeds={"4": good}, tallies={"4": tally})
        assert_counts(good.read(), cpu.reference("4", cpu.thresholds("4")), "after the refusals")
        assert res["lst4"].scores[-1] == tally.read().score.max()
        # objects alive when the context closes are released by it: free() afterwards is a no-op
        alive = api.ExceedCounts(ex, [1.0, 2.0])
    finally:
        ex.close()
    alive.free()
    good.free()


# ---- 8. seeded loop -------------------------------------------------------------------------------------------------
N_FUZZ = int(os.environ.get("GCRE_EXCEED_FUZZ_CASES", "6"))
FUZZ_BASE = int(os.environ.get("GCRE_EXCEED_FUZZ_BASE", "0"))


@pytest.mark.parametrize("case", range(N_FUZZ))
def test_random_problem_counts_equal_the_definition(case, monkeypatch):
    """helpers.fuzz_problem's draws (sizes, methods, path lengths, tables with ties) under the knob draws of
    tests/test_gpu_fuzz.py, plus the counting form: even cases through gcre_process_paths, odd ones through ResidentPlan."""
    from helpers import fuzz_problem
    from test_gpu_fuzz import draw, entered
    number = FUZZ_BASE + case
    entered("exceed", number)
    _, env = draw(600000 + number)
    env["GCRE_EXCEED_KERNEL"] = ["", "ie", "dense"][number % 3]
    for k, v in env.items():
        if v:
            monkeypatch.setenv(k, v)
    _, p = fuzz_problem(number)
    cpu = Cpu(p)
    if case % 2 == 0:
        _, got = one_call(p, cpu)
        calls = 1
    else:
        plan = api.ResidentPlan(p)
        try:
            calls = len(plan.windows())
        finally:
            plan.close()
        _, got, _ = plan_pass(p, cpu, passes=1 + case % 3, keep=case % 4 == 1)
    for name in LEVELS[:p.path_length]:
        assert_counts(got[name], cpu.reference(name, cpu.thresholds(name)), f"case {number} level {name}", observed_calls=calls)
