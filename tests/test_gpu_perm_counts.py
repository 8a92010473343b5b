"""Per-permutation exceedance counts on the device (gcre_exceed_keep_perm_counts: the PC instantiations of k_exceed_ie and
k_exceed_dense) against their numpy definition, report.exceed_reference(per_permutation=True), fed with
operand rows and null maxima from the CPU oracle.  Every comparison of counts is exact equality of integers (pytest -m gpu).

GCRE_PERM_COUNTS_FUZZ_CASES=1000 [GCRE_PERM_COUNTS_FUZZ_BASE=...] for a long run of the seeded loop at the end; eight by
default."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from geneticscre_amd import api, report, synth
from test_gpu_exceed import LEVELS, Cpu, _network_case, cpu_of, same_results

pytestmark = pytest.mark.gpu

def reference(cpu, name, thr, shard=None, window=None):
    """The definition, once per (problem, level, thresholds, shard, window); shared and never written to.  (Kept on the
    Cpu object: it lives as long as the problem does.)"""
    _REF = cpu.__dict__.setdefault("_perm_refs", {})
    key = (name, np.asarray(thr, np.float64).tobytes(), shard, window)
    if key not in _REF:
        p = cpu.p
        want = report.exceed_reference(p.method, p.n_cases, p.n_ctrls, p.levels.uids[name], *cpu.ops[name], p.value_table,
                                       cpu.masks, thr, shard=shard, window=window, per_permutation=True)
        for v in want.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = want
    return _REF[key]


def tells(want):
    """The expected array can tell right from wrong: for some threshold some permutation's count is neither 0 nor the number
    of paths, and the counts differ between permutations."""
    V, P = want["perm_counts"], want["paths"]
    return any(((row > 0) & (row < P)).any() and len(set(row.tolist())) > 1 for row in V)


def assert_perm(got, want, what="", times=1):
    """Exceedances against the definition: the per-permutation array, its row sums, the totals."""
    assert got.perm_counts is not None and got.perm_counts.dtype == np.uint64, what
    np.testing.assert_array_equal(got.perm_counts, want["perm_counts"] * np.uint64(times), err_msg=f"{what} perm_counts")
    np.testing.assert_array_equal(got.exceed, want["exceed"] * np.uint64(times), err_msg=f"{what} exceed")
    np.testing.assert_array_equal(got.perm_counts.sum(axis=1), got.exceed, err_msg=f"{what} row sums")


def assert_ties_to_maxima(got, thr, null_max, what=""):
    """For an unsharded join over all permutations: at least one path of permutation r reaches the threshold exactly when
    the join's own maximum of r does (the pruned kernels' null_max, f32)."""
    np.testing.assert_array_equal(got.perm_counts.sum(axis=1), got.exceed, err_msg=f"{what} row sums")
    reach = null_max.astype(np.float64)[None, :] >= np.asarray(thr, np.float64)[:, None]
    np.testing.assert_array_equal(got.perm_counts >= 1, reach, err_msg=f"{what} counts >= 1 against the null maxima")


def make_counters(ex, cpu, names=None, extra=()):
    return {name: api.ExceedCounts(ex, cpu.thresholds(name, extra), perm_counts=True)
            for name in (names or LEVELS[:cpu.p.path_length])}


def one_call(p, cpu, names=None):
    """gcre_process_paths with per-permutation counters on the levels named: (results, level name -> Exceedances)."""
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    try:
        xs = make_counters(ex, cpu, names)
        res = api.process_paths(p, exec_=ex, exceeds=xs)
        return res, {k: x.read() for k, x in xs.items()}
    finally:
        ex.close()


def plan_pass(p, cpu, passes=1, keep=False, window=None):
    """ResidentPlan passes with fresh per-permutation counters per pass: results and counters of the last pass, its profile."""
    plan = api.ResidentPlan(p)
    try:
        if window:
            plan.set_window(window)
        for _ in range(passes):
            xs = make_counters(plan.ex, cpu)
            res = plan.run(keep_inspections=keep, exceeds=xs)
            got = {k: x.read() for k, x in xs.items()}
        return res, got, dict(plan.last_profile)
    finally:
        plan.close()


def check_every_level(p, cpu, res, got, what, need_tells=True):
    """The definition and the two invariants on every level of an unsharded run over all permutations.  ``res``: level
    name -> JoinResult, or the one-call driver's lst1 .."""
    some = False
    for L, name in enumerate(LEVELS[:p.path_length], start=1):
        thr = cpu.thresholds(name)
        want = reference(cpu, name, thr)
        P = want["paths"]
        assert got[name].perm_counts.shape == (len(thr), p.iterations)
        assert (want["perm_counts"][-2] == P).all() and not want["perm_counts"][-1].any()     # the value <= 0, the one above all
        some = some or tells(want)
        assert_perm(got[name], want, f"{what} level {name}")
        r = res[name] if name in res else res[f"lst{L}"]
        assert_ties_to_maxima(got[name], thr, r.null, f"{what} level {name}")
    assert some or not need_tells, what


# ---- 1, 2. the definition on every level, and the invariants that do not pass through numpy -------------------------


@pytest.mark.parametrize("size", ["sets", "cache"])
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_perm_counts_equal_the_definition_on_every_level(method, size):
    cpu = cpu_of(method, size, table=size == "sets")
    p = cpu.p
    res, got = one_call(p, cpu)
    for name in LEVELS:
        assert tells(reference(cpu, name, cpu.thresholds(name))), (method, size, name)
    check_every_level(p, cpu, res, got, f"{method} {size}")
    # an object without them reads None and counts what it counted
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    try:
        x = api.ExceedCounts(ex, cpu.thresholds("4"))
        api.process_paths(p, exec_=ex, exceeds={"4": x})
        plain = x.read()
        assert plain.perm_counts is None
        np.testing.assert_array_equal(plain.exceed, got["4"].exceed)
        np.testing.assert_array_equal(plain.observed, got["4"].observed)
        assert (plain.perms, plain.paths) == (got["4"].perms, got["4"].paths)
    finally:
        ex.close()


# ---- 3. tile and window edges ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("K", [6, 40, 2100])
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_tile_edges(method, K, monkeypatch, capfd):
    """K = 2,100: two 2048-permutation tiles, the second almost empty; K = 6 and 40: the small-K dense instantiations."""
    monkeypatch.setenv("GCRE_EXCEED_TRACE", "1")
    if K < 64:
        monkeypatch.setenv("GCRE_EXCEED_KERNEL", "dense")
    cpu = cpu_of(method, "sets", K=K)
    p = cpu.p
    capfd.readouterr()
    res, got = one_call(p, cpu)
    err = capfd.readouterr().err
    if K < 64:
        assert "[exceed] dense form" in err and "[exceed] ie form" not in err, err[-400:]
    check_every_level(p, cpu, res, got, f"{method} K={K}")
    for name in LEVELS:                                  # the last permutation's column is the last column
        want = reference(cpu, name, cpu.thresholds(name))
        np.testing.assert_array_equal(got[name].perm_counts[:, K - 1], want["perm_counts"][:, K - 1])
        assert got[name].perm_counts[-2, K - 1] == want["paths"] > 0


@pytest.mark.parametrize("form", ["", "ie"])
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_three_windows(method, form, monkeypatch):
    """K = 4,200 under GCRE_WINDOW_TILES=1: three windows, the permutation index is absolute -- permutation 4,199 lands in
    column 4,199 -- through ResidentPlan.run(exceeds=) and through api.process_paths."""
    monkeypatch.setenv("GCRE_WINDOW_TILES", "1")
    if form:
        monkeypatch.setenv("GCRE_NULL_KERNEL", form)
        monkeypatch.setenv("GCRE_AHEAD", "0")
    K = 4200
    cpu = cpu_of(method, "sets", K=K)
    p = cpu.p
    plan = api.ResidentPlan(p)
    try:
        plan.set_window(2048)
        assert len(plan.windows()) == 3
    finally:
        plan.close()
    res, got, _ = plan_pass(p, cpu, window=2048)
    check_every_level(p, cpu, res, got, f"{method} plan")
    res2, got2 = one_call(p, cpu)
    check_every_level(p, cpu, res2, got2, f"{method} one call")
    for g in (got, got2):
        for name in LEVELS:
            want = reference(cpu, name, cpu.thresholds(name))
            assert g[name].perm_counts.shape[1] == K
            np.testing.assert_array_equal(g[name].perm_counts[:, 4199], want["perm_counts"][:, 4199])
            assert g[name].perm_counts[-2, 4199] == want["paths"] and g[name].perm_counts[-2, 2048] == want["paths"]
    # one window alone fills its own columns and no others
    plan = api.ResidentPlan(p)
    try:
        plan.set_window(2048)
        plan.run()                                # the kept sets of levels 1..3 are the operands below
        p0, p1, _ = plan.operands("4")
        thr = cpu.thresholds("4")
        x = api.ExceedCounts(plan.ex, thr, perm_counts=True)
        plan.ex.set_perm_window(2048, 4096)
        plan.ex.join(plan.uids["4"], p0, p1, None, exceed=x)
        g = x.read()
        want = reference(cpu, "4", thr, window=(2048, 4096))
        np.testing.assert_array_equal(g.perm_counts[:, 2048:4096], want["perm_counts"])
        assert not g.perm_counts[:, :2048].any() and not g.perm_counts[:, 4096:].any()     # not covered: 0
        assert g.perms == 2048 and g.perm_counts[-2, 2048:4096].min() == want["paths"]
    finally:
        plan.close()


# ---- 4. both forms, both bin roads ----------------------------------------------------------------------------------


@pytest.mark.parametrize("m", [20, 5000])
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_both_forms_and_both_bin_roads(method, m, monkeypatch, capfd):
    """m = 5,000 thresholds at K = 700 is above both LDS-histogram limits (4,096 / 2,048): the bins are global; m = 20 takes
    the block's LDS histogram.  k_exceed_ie and k_exceed_dense give the same array, the definition's.  Equal thresholds,
    thresholds in no order, -inf and +inf."""
    monkeypatch.setenv("GCRE_NULL_KERNEL", "ie")
    monkeypatch.setenv("GCRE_EXCEED_TRACE", "1")
    cpu = cpu_of(method, "sets")
    p = cpu.p
    rng = np.random.default_rng(5 + m)
    null = cpu.want["lst4"].null.astype(np.float64)
    thr = rng.uniform(null.min() * 0.5, null.max() * 1.01, size=m)
    thr[::7] = thr[3]
    thr[5], thr[6] = -np.inf, np.inf
    want = reference(cpu, "4", thr)
    assert tells(want) and len({row.tobytes() for row in want["perm_counts"]}) > min(m, 50) // 2
    np.testing.assert_array_equal(want["perm_counts"][0], want["perm_counts"][7])
    out = {}
    for form in ("ie", "dense"):
        monkeypatch.setenv("GCRE_EXCEED_KERNEL", form)
        capfd.readouterr()
        ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
        try:
            x = api.ExceedCounts(ex, thr, perm_counts=True)
            res = api.process_paths(p, exec_=ex, exceeds={"4": x})
            out[form] = x.read()
        finally:
            ex.close()
        err = capfd.readouterr().err
        assert f"[exceed] {form} form" in err and f"[exceed] {'dense' if form == 'ie' else 'ie'} form" not in err, err[-400:]
        assert_perm(out[form], want, f"{method} m={m} {form}")
        assert_ties_to_maxima(out[form], thr, res["lst4"].null, f"{method} m={m} {form}")
    np.testing.assert_array_equal(out["ie"].perm_counts, out["dense"].perm_counts)


# ---- 5. how the join ran does not matter; counts add ----------------------------------------------------------------

VARIANTS = {
    "chunks": ({"GCRE_CHUNK_PATHS": "64"}, {}),
    "ahead_off": ({"GCRE_AHEAD": "0"}, {}),
    "ahead_on": ({"GCRE_AHEAD": "1"}, {}),
    "ahead_on_ie_chunks": ({"GCRE_AHEAD": "1", "GCRE_NULL_KERNEL": "ie", "GCRE_CHUNK_PATHS": "64"}, {}),
    "cache_replay": ({}, {"passes": 2, "keep": True}),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_perm_counts_do_not_depend_on_how_the_join_ran(method, variant, monkeypatch):
    env, how = VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cpu = cpu_of(method, "cache", table=False)
    p = cpu.p
    res, got, prof = plan_pass(p, cpu, passes=how.get("passes", 1), keep=how.get("keep", False))
    if variant.startswith("ahead_on"):
        assert prof["inspect_replays"] > 0, prof     # the chain ran: later joins were counted by a pass over the inspection cache
    if variant == "cache_replay":
        assert prof["inspect_replays"] >= len(LEVELS), prof
    check_every_level(p, cpu, res, got, f"{method} {variant}")
    # and the joins' own results are those of a pass without counters
    plan = api.ResidentPlan(p)
    try:
        for _ in range(how.get("passes", 1)):
            plain = plan.run(keep_inspections=how.get("keep", False))
    finally:
        plan.close()
    same_results(res, plain, LEVELS)


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_shards_and_repeats_add_and_reset_zeroes(method, monkeypatch):
    monkeypatch.setenv("GCRE_AHEAD", "0")
    cpu = cpu_of(method, "cache", table=False)
    p = cpu.p
    K = p.iterations
    plan = api.ResidentPlan(p)
    try:
        plan.run()                                # the kept sets of levels 1..3 are the operands below
        ex = plan.ex
        for name in ("3", "5"):
            P = p.levels.n_paths[name]
            thr = cpu.thresholds(name)
            whole = reference(cpu, name, thr)
            assert tells(whole)
            p0, p1, _ = plan.operands(name)
            halves = [(0, P // 3), (P // 3, P)]
            both, parts = api.ExceedCounts(ex, thr, perm_counts=True), []
            for h in halves:
                x = api.ExceedCounts(ex, thr, perm_counts=True)
                ex.join(plan.uids[name], p0, p1, None, shard=h, exceed=x)
                ex.join(plan.uids[name], p0, p1, None, shard=h, exceed=both)
                parts.append(x.read())
                assert_perm(parts[-1], reference(cpu, name, thr, shard=h), f"{method} level {name} shard {h}")
            np.testing.assert_array_equal(parts[0].perm_counts + parts[1].perm_counts, whole["perm_counts"])
            assert_perm(both.read(), whole, f"{method} level {name} two shards into one object")
            # a join counted twice doubles every cell; reset zeroes; then it counts afresh
            ex.join(plan.uids[name], p0, p1, None, exceed=both)
            assert_perm(both.read(), whole, f"{method} level {name} counted twice", times=2)
            ex.join(plan.uids[name], p0, p1, None)                        # an unarmed join adds nothing
            assert_perm(both.read(), whole, f"{method} level {name} after an unarmed join", times=2)
            both.reset()
            z = both.read()
            assert not z.perm_counts.any() and not z.exceed.any() and (z.perms, z.paths) == (0, 0)
            assert z.perm_counts.shape == (len(thr), K)
            ex.join(plan.uids[name], p0, p1, None, exceed=both)
            assert_perm(both.read(), whole, f"{method} level {name} after reset")
    finally:
        plan.close()


# ---- 6. the wide-count instantiations -------------------------------------------------------------------------------


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_mid_size_wide_counts(method, monkeypatch, capfd):
    """The shape of test_mid_size_both_forms_and_the_definition (5,000 patients: counts need 12 or 16 planes, K = 1,100 is not
    a multiple of the tile): the definition on the top level, the invariants on every level."""
    monkeypatch.setenv("GCRE_EXCEED_TRACE", "1")
    p = synth.make_problem(220, 800, 2500, 2500, 1100, 4, method=method, top_k=50, seed=77)
    cpu = Cpu(p, nthreads=8)
    names = LEVELS[:4]
    capfd.readouterr()
    res, got = one_call(p, cpu)
    assert "[exceed] ie form" in capfd.readouterr().err
    for L, name in enumerate(names, start=1):
        assert_ties_to_maxima(got[name], cpu.thresholds(name), res[f"lst{L}"].null, f"{method} level {name}")
        assert (got[name].perm_counts[-2] == p.levels.n_paths[name]).all() and not got[name].perm_counts[-1].any()
    want = reference(cpu, "4", cpu.thresholds("4"))
    assert tells(want)
    assert_perm(got["4"], want, f"{method} level 4")


# ---- 7. refusals ----------------------------------------------------------------------------------------------------


def test_refusals():
    cpu = cpu_of("method1", "sets")
    p = cpu.p
    lib = api._perm_counts_lib()
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    try:
        thr = cpu.thresholds("4")
        # arming after a count; reset lifts it
        late = api.ExceedCounts(ex, thr)
        api.process_paths(p, exec_=ex, exceeds={"4": late})
        assert late.read().perms == p.iterations
        assert lib.gcre_exceed_keep_perm_counts(late._h, 1) == api.GCRE_ERR_ARG
        assert b"after something was counted" in lib.gcre_last_error(ex._h)
        late.reset()
        assert lib.gcre_exceed_keep_perm_counts(late._h, 1) == 0
        assert lib.gcre_exceed_keep_perm_counts(late._h, 1) == 0            # already on: nothing to do
        late.keeps_perm_counts = True
        api.process_paths(p, exec_=ex, exceeds={"4": late})
        assert_perm(late.read(), reference(cpu, "4", thr), "armed after a reset")
        # off again: the array is freed, reading it is refused, the totals stay
        assert lib.gcre_exceed_keep_perm_counts(late._h, 0) == 0
        late.keeps_perm_counts = False
        buf = np.zeros((len(thr), p.iterations), np.uint64)
        assert lib.gcre_exceed_read_perm_counts(late._h, api._ptr(buf)) == api.GCRE_ERR_ARG
        assert b"keeps no per-permutation counts" in lib.gcre_last_error(ex._h)
        np.testing.assert_array_equal(late.read().exceed, reference(cpu, "4", thr)["exceed"])
        # reading an object that never kept any
        plain = api.ExceedCounts(ex, thr)
        assert lib.gcre_exceed_read_perm_counts(plain._h, api._ptr(buf)) == api.GCRE_ERR_ARG
        assert b"keeps no per-permutation counts" in lib.gcre_last_error(ex._h)
        assert plain.read().perm_counts is None
        assert lib.gcre_exceed_keep_perm_counts(None, 1) == api.GCRE_ERR_ARG
        # the several-device driver refuses an armed object, before anything runs
        before = ex.profile()["null_kernel_launches"]
        good = api.ExceedCounts(ex, thr, perm_counts=True)
        keep = []
        inp = api._pp_input(p, keep)
        outs = (api.gcre_result * 5)()
        assert lib.gcre_process_paths_set_exceed(ex._h, 4, good._h) == 0
        inp.shard_rank, inp.shard_world = 0, 2
        assert ex._lib.gcre_process_paths(ex._h, ctypes.byref(inp), outs) == api.GCRE_ERR_ARG
        assert b"several" in lib.gcre_last_error(ex._h)
        assert ex.profile()["null_kernel_launches"] == before
        z = good.read()
        assert not z.perm_counts.any() and not z.exceed.any() and (z.perms, z.paths) == (0, 0)
        # the context still works
        api.process_paths(p, exec_=ex, exceeds={"4": good})
        assert_perm(good.read(), reference(cpu, "4", thr), "after the refusals")
        alive = api.ExceedCounts(ex, [1.0, 2.0], perm_counts=True)         # released by the context
    finally:
        ex.close()
    alive.free()
    # m x iterations over the limit: 10,000 x 6,711 = 2^26 + 1,136; 10,000 x 6,710 is allowed
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, 6711)
    try:
        big = np.linspace(1.0, 2.0, api.EXCEED_MAX)
        with pytest.raises(api.GcreError, match="2\\^26"):
            api.ExceedCounts(ex, big, perm_counts=True)
        x = api.ExceedCounts(ex, big)
        assert lib.gcre_exceed_keep_perm_counts(x._h, 1) == api.GCRE_ERR_ARG and b"67108864" in lib.gcre_last_error(ex._h)
        assert api.ExceedCounts(ex, big[:-2], perm_counts=True).read().perm_counts.shape == (api.EXCEED_MAX - 2, 6711)
    finally:
        ex.close()
    # a context with 0 iterations
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, 0)
    try:
        with pytest.raises(api.GcreError, match="0 iterations"):
            api.ExceedCounts(ex, [1.0], perm_counts=True)
        x = api.ExceedCounts(ex, [1.0])
        assert lib.gcre_exceed_keep_perm_counts(x._h, 1) == api.GCRE_ERR_ARG
    finally:
        ex.close()
    with pytest.raises(ValueError, match="2\\^26"):
        report.gwaspa(*_network_case(17)[:2], 48, 52, _network_case(17)[2], top_k=10000, n_permutations=6711, false_counts=True)


# ---- 8. the front end -----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("signed", [False, True])
def test_gwaspa_false_counts(signed):
    nc, nt, K, L = 48, 52, 700, 5
    genes, data, network = _network_case(17)
    strata = (np.arange(nc + nt) * 5 % 3).astype(np.int32)
    kw = dict(signed=signed, threshold=0.2, n_permutations=K, strata=strata, seed=909, top_k=6, path_length=L)
    ks = (1, 2, 5)
    base = report.gwaspa(genes, data, nc, nt, network, **kw)
    out = report.gwaspa(genes, data, nc, nt, network, false_counts=True, false_count_ks=ks, false_count_alpha=0.1, **kw)
    assert set(out) == set(base) | {"exceed"}
    df = out["GWASPA.Results"]
    names = report.false_count_names(ks)
    assert list(df.columns) == report.COLUMNS + names                        # fdr's own columns only with fdr=True
    assert df[report.COLUMNS].equals(base["GWASPA.Results"])                 # every earlier column, and the row order
    for c in report.COLUMNS:
        a, b = df[c].to_numpy(), base["GWASPA.Results"][c].to_numpy()
        assert a.dtype == b.dtype and (a.tobytes() == b.tobytes() if a.dtype != object else list(a) == list(b)), c
    some = False
    for Lx in range(1, L + 1):
        got = out["exceed"][Lx]
        s = out["levels"][f"lst{Lx}"].scores
        thr = s[np.isfinite(s)]
        assert got.perm_counts.shape == (len(thr), K) and got.perms == K
        np.testing.assert_array_equal(got.perm_counts.sum(axis=1), got.exceed)
        assert_ties_to_maxima(got, thr, out["levels"][f"lst{Lx}"].null, f"length {Lx}")
        cols = report.false_count_columns(thr, got.perm_counts, got.observed, got.perms, ks=ks, alpha=0.1)
        rows = df[df["Lengths"] == Lx]
        by_score = {t: i for i, t in enumerate(thr.tolist())}
        for c in names:
            exp = np.array([cols[c][by_score[sc]] if np.isfinite(sc) else np.nan for sc in rows["Scores"]])
            np.testing.assert_array_equal(rows[c].to_numpy(np.float64), exp)
        fin = np.isfinite(rows["Scores"].to_numpy(np.float64))
        np.testing.assert_array_equal(rows["kFWER.1"].to_numpy(np.float64)[fin], rows["Pvalues"].to_numpy(np.float64)[fin])
        assert np.isnan(rows[names].to_numpy(np.float64)[~fin]).all()         # sentinel rows
        v = rows["kFWER.2"].to_numpy(np.float64)[fin]
        some = some or bool(((v > 0) & (v < 1)).any())
    assert some      # not all zeros and ones: the columns say something on this case
    # with fdr too: its three columns first, the same numbers
    both = report.gwaspa(genes, data, nc, nt, network, fdr=True, false_counts=True, false_count_ks=ks, false_count_alpha=0.1, **kw)
    assert list(both["GWASPA.Results"].columns) == report.COLUMNS + report.FDR_COLUMNS + names
    assert both["GWASPA.Results"][report.COLUMNS + names].equals(df)
    # no permutations: NaN columns
    none = report.gwaspa(genes, data, nc, nt, network, false_counts=True, **dict(kw, n_permutations=0, strata=None))
    dn = none["GWASPA.Results"]
    assert list(dn.columns) == report.COLUMNS + report.false_count_names() and np.isnan(dn[report.false_count_names()].to_numpy()).all()


# ---- 9. seeded loop -------------------------------------------------------------------------------------------------
N_FUZZ = int(os.environ.get("GCRE_PERM_COUNTS_FUZZ_CASES", "8"))
FUZZ_BASE = int(os.environ.get("GCRE_PERM_COUNTS_FUZZ_BASE", "0"))


@pytest.mark.parametrize("case", range(N_FUZZ))
def test_random_problem_perm_counts_equal_the_definition(case, monkeypatch):
    """helpers.fuzz_problem's draws (sizes, methods, path lengths, tables with ties) under the knob draws of
    tests/test_gpu_fuzz.py, plus the counting form: even cases through gcre_process_paths, odd ones through ResidentPlan."""
    from helpers import fuzz_problem
    from test_gpu_fuzz import draw, entered
    number = FUZZ_BASE + case
    entered("perm_counts", number)
    _, env = draw(700000 + number)
    env["GCRE_EXCEED_KERNEL"] = ["", "ie", "dense"][number % 3]
    for k, v in env.items():
        if v:
            monkeypatch.setenv(k, v)
    _, p = fuzz_problem(number)
    cpu = Cpu(p)
    if case % 2 == 0:
        res, got = one_call(p, cpu)
    else:
        res, got, _ = plan_pass(p, cpu, passes=1 + case % 3, keep=case % 4 == 1)
    check_every_level(p, cpu, res, got, f"case {number}", need_tells=False)
