"""A GeneTally, an ExceedCounts (with and without per-permutation counts, which step-down reads) and a HitList armed on the
SAME joins: every route of the four single-observer matrices (tests/test_gpu_genes.py, test_gpu_exceed.py,
test_gpu_perm_counts.py, test_gpu_hits.py), observers spread over the levels of a chain, shards into shared objects, repeats,
resets and lifetimes on one plan, and calls that are refused half way through arming.  The definitions, problems and
comparers are those files' own; every comparison is exact -- integers as integers, scores as f64 bit patterns.

GCRE_OBS_FUZZ_CASES=300 [GCRE_OBS_FUZZ_BASE=...] [GCRE_FUZZ_LIGHT=1] for a long run of the seeded loop at the end; four by
default."""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np
import pytest

import test_gpu_exceed as X
import test_gpu_genes as G
import test_gpu_hits as H
import test_gpu_perm_counts as PC
import test_gpu_stepdown as SD
from geneticscre_amd import api, report

gpu = pytest.mark.gpu          # every test but the one that looks at the references alone

LEVELS = report.GENE_LEVELS                      # "1b", "2", "3", "4", "5": the joins behind lst1 .. lst5
METHODS = ["method1", "method2"]
SUBSETS = [("tally", "exceed"), ("tally", "hits"), ("exceed", "hits"), ("tally", "exceed", "hits"), ("tally", "perm", "hits")]
# the union of the four matrices; where a name occurs in several, the exceedance file's entry (it pins the chain as well)
ROUTES = {**G.VARIANTS, **H.VARIANTS, **PC.VARIANTS, **X.VARIANTS}
NAMED = ("chunks", "chunks_dense", "cache_replay", "ahead_off", "ahead_on", "ahead_on_chunks", "ahead_on_ie",
         "ahead_on_ie_chunks", "no_perms", "windows", "windows_ahead_off", "windows_ie", "sparse", "dense", "ie", "ie_no_quad",
         "ie_no_prune", "ie_counted_dense", "ie_counted_ie")
assert not set(NAMED) - set(ROUTES), set(NAMED) - set(ROUTES)
assert G.SIZES["cache"] == X.SIZES["cache"] == H.SIZES["cache"] == (40, 110, 310, 335, 300, 5, 15, 21)


class Refs:
    """The problem at the "cache" size and every definition on it, computed once per (method, K) and never written to."""

    def __init__(self, method, K=None):
        self.cpu = cpu = X.cpu_of(method, "cache", K=K, table=False)
        self.p = p = cpu.p
        self.K = p.iterations
        if method not in G._WANT:
            G._WANT[method] = G.reference(p)                 # (observed scores: they do not depend on K)
        self.tally = G._WANT[method]
        self.cuts = H.cutoffs(cpu.want, "median")
        self.hits = H.reference(p, cpu.want, self.cuts)
        self.thr = {name: cpu.thresholds(name) for name in LEVELS}
        self.top = {name: SD.top_rows(cpu, name) for name in LEVELS}
        for h in self.hits.values():
            for v in h.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)

    def counts(self, name, shard=None):
        """exceed_reference(per_permutation=True) for the single tests' thresholds: totals and the array."""
        return PC.reference(self.cpu, name, self.thr[name], shard=shard)

    def top_counts(self, name):
        """The same for the oracle's top scores alone: the thresholds step-down takes."""
        return PC.reference(self.cpu, name, self.top[name][2])

    def stepdown(self, name):
        return SD.reference(self.cpu, name, self.top[name])

    def bite(self):
        """The inputs can tell right from wrong -- on the references alone."""
        p = self.p
        assert all(p.levels.n_paths[k] >= 3 * 64 for k in ("3", "4", "5")), p.levels.n_paths      # three 64-path chunks ...
        assert any(p.levels.n_paths[k] % 64 for k in ("3", "4", "5")), p.levels.n_paths            # ... and a ragged last one
        assert any(0 < self.hits[k]["found"] < p.levels.n_paths[k] for k in LEVELS)
        assert all(np.isfinite(self.tally[k]["score"]).any() for k in LEVELS)
        if self.K > 0:
            for name in LEVELS:
                assert X.bites(self.counts(name)), name                                            # non-zero null exceedances
            assert any((self.counts(k)["perm_counts"] > 1).any() for k in LEVELS)                  # a V[threshold][permutation] > 1
            assert any((self.top_counts(k)["perm_counts"] > 1).any() for k in LEVELS)
            assert any(PC.tells(self.top_counts(k)) for k in LEVELS)


_REFS = {}


def refs_of(method, K=None):
    if (method, K) not in _REFS:
        _REFS[(method, K)] = Refs(method, K)
        _REFS[(method, K)].bite()
    return _REFS[(method, K)]


@pytest.mark.parametrize("method", METHODS)
def test_the_references_bite(method):
    """No GPU: a generator that drifts away from inputs that tell right from wrong fails here."""
    refs_of(method)


def arm(ex, R, subset):
    """Fresh observers of ``subset`` on every level: {"tally" | "exceed" | "hits": level name -> object} ("perm": an
    ExceedCounts that keeps per-permutation counts, its thresholds the oracle's top scores)."""
    obs = {}
    if "tally" in subset:
        obs["tally"] = G.make_tallies(ex, R.p)
    if "exceed" in subset:
        obs["exceed"] = {k: api.ExceedCounts(ex, R.thr[k]) for k in LEVELS}
    if "perm" in subset:
        obs["exceed"] = {k: api.ExceedCounts(ex, R.top[k][2], perm_counts=True) for k in LEVELS}
    if "hits" in subset:
        obs["hits"] = {k: api.HitList(ex, R.cuts[k], cap=1 << 16) for k in LEVELS}
    return obs


def kw(obs):
    return dict(tallies=obs.get("tally"), exceeds=obs.get("exceed"), hits=obs.get("hits"))


def check(obs, R, subset, what, calls=1):
    """Every armed observer against its definition.  ``calls``: how many join calls counted each level (the permutation
    windows of a ResidentPlan pass: the observed scores are counted once per call, the null values add up to K)."""
    p = R.p
    for name, t in obs.get("tally", {}).items():
        G.assert_tally(t.read(), R.tally[name], f"{what} tally level {name}")
    for name, x in obs.get("exceed", {}).items():
        got = x.read()
        assert got.perms == R.K, f"{what} level {name}"
        if "perm" in subset:
            want = R.top_counts(name)
            PC.assert_perm(got, want, f"{what} level {name}")
            n_ge = x.stepdown(*SD.sets_of(R.cpu, name, R.top[name][0], R.top[name][1]))   # (the counts in the form step-down reads)
            np.testing.assert_array_equal(n_ge, R.stepdown(name)["n_ge"], err_msg=f"{what} step-down level {name}")
        else:
            want = R.counts(name)
            assert got.perm_counts is None
        X.assert_counts(got, want, f"{what} level {name}", observed_calls=calls)
    for name, h in obs.get("hits", {}).items():
        got = h.read()
        H.assert_hits(got, R.hits[name], f"{what} hits level {name}")
        assert got.paths == p.levels.n_paths[name], f"{what} level {name}: listed once"


def assert_untouched(obs, what):
    for name, t in obs.get("tally", {}).items():
        e = t.read()
        assert np.isneginf(e.score).all() and (e.ordinal == -1).all() and not e.cases.any(), f"{what} tally level {name}"
    for name, x in obs.get("exceed", {}).items():
        z = x.read()
        assert not z.exceed.any() and not z.observed.any() and (z.perms, z.paths) == (0, 0), f"{what} counts level {name}"
        assert z.perm_counts is None or not z.perm_counts.any(), f"{what} counts level {name}"
    for name, h in obs.get("hits", {}).items():
        assert h.count() == (0, 0), f"{what} hits level {name}"


@contextlib.contextmanager
def plan_pass(R, subset, how):
    """One fresh ResidentPlan, ``how``'s passes with fresh observers each: (results, observers, profile, windows) of the
    last pass, the plan open while the caller reads the observers."""
    plan = api.ResidentPlan(R.p)
    try:
        if how.get("window"):
            plan.set_window(how["window"])
        for _ in range(how.get("passes", 1)):
            obs = arm(plan.ex, R, subset)
            res = plan.run(keep_inspections=how.get("keep", False), **kw(obs))
        yield res, obs, dict(plan.last_profile), len(plan.windows())
    finally:
        plan.close()


# ---- 1. armed together equals the definition, on every route ---------------------------------------------------------


@gpu
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("method", METHODS)
def test_armed_together_equals_the_definitions(method, route, monkeypatch):
    """Every subset of two or three observers, all levels armed, one ResidentPlan pass each: each observer is its numpy
    definition, the joins' own results are those of an unarmed pass, the counts cover K permutations, a list holds a level
    once, and step-down reads the combined pass's per-permutation counts as it reads a pass of its own."""
    env, how = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)                 # before the context is created: gcre_create reads them
    R = refs_of(method, how.get("K"))
    with plan_pass(R, (), how) as (plain, _, _, windows):
        pass
    assert windows == (3 if route.startswith("windows") else 1)
    for subset in SUBSETS:
        what = f"{method} {route} {'+'.join(subset)}"
        if "perm" in subset and R.K == 0:
            ex = api.JoinExec(R.p.method, R.p.n_cases, R.p.n_ctrls, 0)
            try:
                with pytest.raises(api.GcreError, match="0 iterations"):     # nothing to keep per permutation: refused when made
                    api.ExceedCounts(ex, R.top["4"][2], perm_counts=True)
            finally:
                ex.close()
            continue
        with plan_pass(R, subset, how) as (res, obs, prof, _):
            if route.startswith("ahead_on"):
                assert prof["inspect_replays"] > 0, (what, prof)     # the chain ran: later joins were counted and collected in a replay
            if route == "ahead_off":
                assert prof["inspect_replays"] == 0, (what, prof)
            if route == "cache_replay":
                assert prof["inspect_replays"] >= len(LEVELS), (what, prof)
            if route.startswith("windows"):
                assert prof["inspect_replays"] >= 2 * len(LEVELS), (what, prof)    # three windows: the joins ran three times
            X.same_results(res, plain, LEVELS)
            check(obs, R, subset, what, calls=windows)


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_armed_together_through_the_one_call_driver(method):
    """The same subsets through gcre_process_paths (no chain; the observed scores are counted once)."""
    R = refs_of(method)
    p = R.p
    plain = api.process_paths(p)
    for subset in SUBSETS:
        ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
        try:
            obs = arm(ex, R, subset)
            res = api.process_paths(p, exec_=ex, **kw(obs))
            for L in range(1, 6):
                for f in ("scores", "src", "trg", "cases", "ctrls", "null"):
                    assert getattr(res[f"lst{L}"], f).tobytes() == getattr(plain[f"lst{L}"], f).tobytes(), (subset, L, f)
            check(obs, R, subset, f"{method} one call {'+'.join(subset)}")
        finally:
            ex.close()


# ---- 2. different observers on different levels ----------------------------------------------------------------------

SPREAD = {"tally": ("2", "4"), "exceed": ("3", "4"), "hits": ("4", "5")}           # nothing on "1b", all three on "4"
MIRROR = {kind: tuple(k for k in LEVELS if k not in on) for kind, on in SPREAD.items()}   # nothing on "4", all three on "1b"


@gpu
@pytest.mark.parametrize("chunk", ["", "64"])
@pytest.mark.parametrize("method", METHODS)
def test_observers_spread_over_the_levels_of_a_chain(method, chunk, monkeypatch):
    """Some joins launched ahead need a counting replay, their neighbours do not; level 5 (then level 3) is replayed for a
    list alone.  Objects of every level are made, only some are passed: the others stay empty."""
    monkeypatch.setenv("GCRE_AHEAD", "1")
    if chunk:
        monkeypatch.setenv("GCRE_CHUNK_PATHS", chunk)
    R = refs_of(method)
    plan = api.ResidentPlan(R.p)
    try:
        plain = plan.run()
        for spread, subset in ((SPREAD, ("tally", "exceed", "hits")), (MIRROR, ("tally", "perm", "hits"))):
            made = arm(plan.ex, R, subset)
            passed = {kind: {k: o for k, o in made[kind].items() if k in spread[kind]} for kind in made}
            left = {kind: {k: o for k, o in made[kind].items() if k not in spread[kind]} for kind in made}
            assert all(len(passed[kind]) == len(spread[kind]) and left[kind] for kind in made)
            res = plan.run(**kw(passed))
            assert plan.last_profile["inspect_replays"] > 0
            what = f"{method} chunk={chunk!r} {'mirror' if spread is MIRROR else 'spread'}"
            X.same_results(res, plain, LEVELS)
            check(passed, R, subset, what)
            assert_untouched(left, what)
    finally:
        plan.close()


# ---- 3. shards into shared objects, all three at once ----------------------------------------------------------------


@gpu
@pytest.mark.parametrize("chunk", ["", "64"])
@pytest.mark.parametrize("method", METHODS)
def test_two_shards_into_shared_objects_all_three_at_once(method, chunk, monkeypatch):
    """Levels 3, 4 and 5 in two sharded calls over [0, P/2) and [P/2, P), each call with a tally, counters and a list:
    per-half objects equal the definitions restricted to the shard, both halves into shared objects equal the whole."""
    monkeypatch.setenv("GCRE_AHEAD", "0")
    if chunk:
        monkeypatch.setenv("GCRE_CHUNK_PATHS", chunk)
    R = refs_of(method)
    p, K = R.p, R.K
    tables = report.gene_tables(p.levels, len(p.data1), len(p.data2))
    plan = api.ResidentPlan(p)
    try:
        plan.run()                                # the kept sets of levels 1..3 are the operands below
        ex = plan.ex
        for name in ("3", "4", "5"):
            P = p.levels.n_paths[name]
            p0, p1, _ = plan.operands(name)
            slots = report.gene_slots(name, len(p.data1), len(p.data2))
            t_all = api.GeneTally(ex, slots, *tables[name])
            x_all = api.ExceedCounts(ex, R.thr[name], perm_counts=True)
            h_all = api.HitList(ex, R.cuts[name], cap=1 << 16)
            for half in [(0, P // 2), (P // 2, P)]:
                what = f"{method} level {name} shard {half}"
                t, x, h = api.GeneTally(ex, slots, *tables[name]), api.ExceedCounts(ex, R.thr[name]), api.HitList(ex, R.cuts[name], cap=1 << 16)
                ex.join(plan.uids[name], p0, p1, None, shard=half, tally=t, exceed=x, hits=h)
                ex.join(plan.uids[name], p0, p1, None, shard=half, tally=t_all, exceed=x_all, hits=h_all)
                G.assert_tally(t.read(), G.reference_shard(p, name, half), what)
                X.assert_counts(x.read(), R.counts(name, shard=half), what)
                got = h.read()
                H.assert_hits(got, H.reference(p, R.cpu.want, {name: R.cuts[name]}, shard=half)[name], what)
                assert got.paths == half[1] - half[0] and 0 < got.found < got.paths, what
            what = f"{method} level {name} both halves"
            G.assert_tally(t_all.read(), R.tally[name], what)
            got = x_all.read()
            PC.assert_perm(got, R.counts(name), what)
            X.assert_counts(got, R.counts(name), what, perms=2 * K)          # (two joins: perms says so)
            got = h_all.read()
            H.assert_hits(got, R.hits[name], what)
            assert got.paths == P, what
    finally:
        plan.close()


# ---- 4. repeats, resets and lifetimes on one plan --------------------------------------------------------------------


def snapshot(obs):
    out = {}
    for kind, per in obs.items():
        for name, o in per.items():
            r = o.read()
            out[kind, name] = {k: (v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in vars(r).items()}
    return out


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_repeats_resets_and_lifetimes_on_one_plan(method, monkeypatch):
    monkeypatch.setenv("GCRE_AHEAD", "1")
    R = refs_of(method)
    lib = api._hits_lib()
    subset = ("tally", "perm", "hits")
    plan = api.ResidentPlan(R.p)
    try:
        run = lambda **k: plan.run(keep_inspections=True, **k)
        # pass 1: everything armed
        obs = arm(plan.ex, R, subset)
        first = run(**kw(obs))
        check(obs, R, subset, f"{method} pass 1")
        before = snapshot(obs)
        # pass 2: fresh lists alone; what pass 1 filled is not touched
        fresh = arm(plan.ex, R, ("hits",))
        X.same_results(run(**kw(fresh)), first, LEVELS)
        assert plan.last_profile["inspect_replays"] >= len(LEVELS)
        check(fresh, R, ("hits",), f"{method} pass 2")
        assert snapshot(obs) == before
        assert snapshot(fresh) == {k: v for k, v in before.items() if k[0] == "hits"}
        # reset, pass 3: all armed again
        for o in list(obs["exceed"].values()) + list(obs["hits"].values()) + list(fresh["hits"].values()):
            o.reset()
        assert_untouched({"exceed": obs["exceed"], "hits": {**obs["hits"], **{k + "'": h for k, h in fresh["hits"].items()}}},
                         f"{method} after reset")
        X.same_results(run(**kw(obs)), first, LEVELS)
        check(obs, R, subset, f"{method} pass 3")
        assert snapshot(obs) == before
        assert_untouched(fresh, f"{method} pass 3, the lists not passed")
        # close every list, pass 4: the other two armed; the counts of two passes, the same table
        for h in list(obs["hits"].values()) + list(fresh["hits"].values()):
            h.free()
        X.same_results(run(tallies=obs["tally"], exceeds=obs["exceed"]), first, LEVELS)
        for name in LEVELS:
            G.assert_tally(obs["tally"][name].read(), R.tally[name], f"{method} pass 4 level {name}")
            got, want = obs["exceed"][name].read(), R.top_counts(name)
            PC.assert_perm(got, want, f"{method} pass 4 level {name}", times=2)
            np.testing.assert_array_equal(got.observed, 2 * want["observed"])
            assert (got.perms, got.paths) == (2 * R.K, 2 * want["paths"])
        # a closed list passed again: refused, nothing launched, nothing else counted; the plan still works
        launches, after4 = lib.gcre_hits_launches(plan.ex._h), snapshot({"tally": obs["tally"], "exceed": obs["exceed"]})
        with pytest.raises(api.GcreError, match="context"):
            run(tallies={"4": obs["tally"]["4"]}, exceeds={"4": obs["exceed"]["4"]}, hits={"4": obs["hits"]["4"]})
        with pytest.raises(api.GcreError, match="context"):
            obs["hits"]["4"].read()
        assert lib.gcre_hits_launches(plan.ex._h) == launches
        X.same_results(run(), first, LEVELS)
        assert lib.gcre_hits_launches(plan.ex._h) == launches
        assert snapshot({"tally": obs["tally"], "exceed": obs["exceed"]}) == after4
    finally:
        plan.close()


# ---- 5. a refused call arms nothing ----------------------------------------------------------------------------------


@gpu
def test_a_refused_join_arms_nothing(monkeypatch):
    """JoinExec.join validates every observer of the call before it arms any: after a call refused for its second or third
    observer, the next plain join -- of another level -- runs as on an untouched context and the good objects stay empty."""
    monkeypatch.setenv("GCRE_AHEAD", "0")        # (single joins below, as in the shard tests)
    R = refs_of("method1")
    p = R.p
    tables = report.gene_tables(p.levels, len(p.data1), len(p.data2))
    plan = api.ResidentPlan(p)
    other = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    try:
        untouched = plan.run()
        ex = plan.ex
        p0, p1, _ = plan.operands("4")
        good = api.GeneTally(ex, len(p.data1), *tables["4"])
        good_x = api.ExceedCounts(ex, R.thr["4"], perm_counts=True)
        closed = api.HitList(ex, R.cuts["4"], cap=1 << 16)
        closed.free()
        foreign = {"counters of another context": dict(tally=good, exceed=api.ExceedCounts(other, R.thr["4"])),
                   "closed counters": dict(tally=good, exceed=api.ExceedCounts(ex, R.thr["4"])),
                   "a list of another context": dict(tally=good, exceed=good_x, hits=api.HitList(other, R.cuts["4"], cap=16)),
                   "a closed list": dict(tally=good, exceed=good_x, hits=closed),
                   "counters armed, a closed list": dict(exceed=good_x, hits=closed)}
        foreign["closed counters"]["exceed"].free()
        launches = api._hits_lib().gcre_hits_launches(ex._h)
        for next_level, (what, armed) in zip(("5", "1b", "5", "1b", "5"), foreign.items()):
            with pytest.raises(api.GcreError, match="context"):
                ex.join(plan.uids["4"], p0, p1, None, **armed)
            q0, q1, _ = plan.operands(next_level)
            r = ex.join(plan.uids[next_level], q0, q1, None)
            X.same_results({next_level: r}, untouched, [next_level])
            assert_untouched({"tally": {"4": good}, "exceed": {"4": good_x}}, what)
        assert api._hits_lib().gcre_hits_launches(ex._h) == launches
        # and the objects work afterwards
        ex.join(plan.uids["4"], p0, p1, None, tally=good, exceed=good_x)
        G.assert_tally(good.read(), R.tally["4"], "after the refusals")
        PC.assert_perm(good_x.read(), R.counts("4"), "after the refusals")
    finally:
        plan.close()
        other.close()


@gpu
def test_a_refused_process_paths_arms_nothing():
    """api.process_paths validates every observer of every level before it sets any: after a refused call a plain call on
    the same context returns what an untouched context returns and the good objects stay empty."""
    R = refs_of("method1")
    p = R.p
    tables = report.gene_tables(p.levels, len(p.data1), len(p.data2))
    untouched = api.process_paths(p)
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    other = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    try:
        good = {"tally": {k: api.GeneTally(ex, report.gene_slots(k, len(p.data1), len(p.data2)), *tables[k]) for k in ("3", "4")},
                "exceed": {k: api.ExceedCounts(ex, R.thr[k], perm_counts=k == "4") for k in ("3", "4")},
                "hits": {k: api.HitList(ex, R.cuts[k], cap=1 << 16) for k in ("3", "4")}}
        t, x, h = good["tally"], good["exceed"], good["hits"]
        wrong = api.GeneTally(ex, len(p.data1), *tables["3"])                 # level 3's rows on level 4
        closed = api.HitList(ex, R.cuts["4"], cap=16)
        closed.free()
        refused = [
            ("no level", dict(tallies={"4": t["4"]}, exceeds={"7": x["4"]})),
            ("context", dict(tallies={"4": t["4"]}, exceeds={"4": api.ExceedCounts(other, R.thr["4"])})),
            ("context", dict(tallies={"4": t["4"]}, exceeds={"3": x["3"], "4": api.ExceedCounts(other, R.thr["4"])})),
            ("context", dict(tallies=dict(t), exceeds=dict(x), hits={"3": h["3"], "4": api.HitList(other, R.cuts["4"], cap=16)})),
            ("context", dict(tallies=dict(t), exceeds=dict(x), hits={"3": h["3"], "4": closed})),
            ("no level", dict(exceeds=dict(x), hits={"4": h["4"], "6": h["3"]})),
            ("uid rows|paths1 row", dict(tallies={"3": t["3"], "4": wrong})),
            ("uid rows|paths1 row", dict(tallies={"3": t["3"], "4": wrong}, exceeds=dict(x), hits=dict(h))),
        ]
        launches = api._hits_lib().gcre_hits_launches(ex._h)
        for i, (msg, armed) in enumerate(refused):
            with pytest.raises(api.GcreError, match=msg):
                api.process_paths(p, exec_=ex, **armed)
            res = api.process_paths(p, exec_=ex)
            for L in range(1, 6):
                for f in ("scores", "src", "trg", "cases", "ctrls", "null"):
                    assert getattr(res[f"lst{L}"], f).tobytes() == getattr(untouched[f"lst{L}"], f).tobytes(), (i, L, f)
            assert_untouched(good, f"refused call {i}")
            assert_untouched({"tally": {"4": wrong}}, f"refused call {i}")
        assert api._hits_lib().gcre_hits_launches(ex._h) == launches
        # and the objects work afterwards
        api.process_paths(p, exec_=ex, tallies=t, exceeds=x, hits=h)
        for k in ("3", "4"):
            G.assert_tally(t[k].read(), R.tally[k], f"after the refusals, level {k}")
            X.assert_counts(x[k].read(), R.counts(k), f"after the refusals, level {k}")
            H.assert_hits(h[k].read(), R.hits[k], f"after the refusals, level {k}")
        PC.assert_perm(x["4"].read(), R.counts("4"), "after the refusals")
    finally:
        ex.close()
        other.close()


# ---- 7. seeded loop --------------------------------------------------------------------------------------------------
N_FUZZ = int(os.environ.get("GCRE_OBS_FUZZ_CASES", "4"))
FUZZ_BASE = int(os.environ.get("GCRE_OBS_FUZZ_BASE", "0"))
KINDS = ("tally", "exceed", "hits")


def draw_observers(number):
    """Case ``number``: (cfg, Problem, knobs, what is armed where and how it runs).  The problem is helpers.fuzz_problem's
    (tests/test_gpu_fuzz.py's draw of sizes, methods, path lengths and tables, its permutations cut to 600, to 100 for wide
    cohorts) -- with the permutations as drawn (0 .. 4,500: no permutations, several windows) where the numpy definitions
    still take about a second: at most 10^7 (joined path, permutation) pairs of up to 850 patients, the "cache" size at
    K = 5,000.  The knobs are that file's draw under a case number of their own, plus the counting form; for half the cases
    a chunk size that cuts small joins, and for half of those with more than one tile of permutations one tile per window."""
    from helpers import fuzz_problem
    from geneticscre_amd.synth import make_problem
    from test_gpu_fuzz import draw, value_table
    cfg, p = fuzz_problem(number)
    drawn = draw(400000 + number)[0]["perms"]
    paths = sum(p.levels.n_paths[k] for k in LEVELS[:p.path_length])
    if drawn != cfg["perms"] and cfg["n_cases"] + cfg["n_ctrls"] <= 850 and paths * drawn <= 10 ** 7:
        cfg["perms"] = drawn
        p = make_problem(cfg["genes"], cfg["edges"], cfg["n_cases"], cfg["n_ctrls"], drawn, cfg["length"], method=cfg["method"],
                         top_k=cfg["top_k"], seed=cfg["seed"], threshold=cfg["threshold"],
                         table=value_table(cfg["table"], cfg["n_cases"], cfg["n_ctrls"], cfg["seed"]))
    _, env = draw(800000 + number)
    rng = np.random.default_rng(8800000 + number)
    env["GCRE_EXCEED_KERNEL"] = str(rng.choice(["", "ie", "dense"]))
    if rng.random() < 0.5:                           # these problems are small: chunks that cut their joins, as test_gpu_hits draws them
        env["GCRE_CHUNK_PATHS"] = str(rng.choice(["64", "200"]))
    if p.iterations > 2048 and rng.random() < 0.5:   # several windows: a list is armed in the first one only
        env["GCRE_WINDOW_TILES"] = "1"
    levels = LEVELS[:p.path_length]
    on = {name: [kind for kind in KINDS if rng.random() < 0.6] for name in levels}
    if not any(len(v) >= 2 for v in on.values()):
        on[levels[-1]] = list(KINDS)                 # every case arms at least two observers on some join
    how = dict(on=on, perm_counts=bool(rng.integers(0, 2)) and p.iterations > 0, one_call=bool(rng.integers(0, 2)),
               keep=bool(rng.integers(0, 2)), passes=int(rng.integers(1, 4)), cutoff=["median", "worst_top", "zero"][number % 3])
    return cfg, p, env, how


@gpu
@pytest.mark.parametrize("case", range(N_FUZZ))
def test_random_problem_all_observers(case, monkeypatch):
    """Random small problems under the knobs that change how a join runs (draw_observers), per level a drawn subset of the
    three observers, per-permutation counts or not, the driver -- gcre_process_paths or ResidentPlan -- the number of
    passes and whether they keep their inspections: every armed observer is its numpy definition."""
    from test_gpu_fuzz import entered
    number = FUZZ_BASE + case
    entered("observers", number)
    cfg, p, env, how = draw_observers(number)
    print(f"[fuzz] observers case {number}: {cfg} {env} {how}", file=sys.stderr, flush=True)
    for k, v in env.items():
        if v:
            monkeypatch.setenv(k, v)
    levels = LEVELS[:p.path_length]
    on, perm, one_call, keep, passes = how["on"], how["perm_counts"], how["one_call"], how["keep"], how["passes"]
    cpu = X.Cpu(p)
    tally_ref = G.reference(p)
    cuts = {}
    for name in levels:
        s = cpu.want[f"lst{LEVELS.index(name) + 1}"].all_scores
        cuts[name] = H.cutoffs(cpu.want, how["cutoff"], levels=(name,))[name] if np.isfinite(s).any() else 0.0
    hits_ref = H.reference(p, cpu.want, cuts)
    thr = {name: cpu.thresholds(name) for name in levels}

    def arm_drawn(ex):
        tables = report.gene_tables(p.levels, len(p.data1), len(p.data2))
        return {"tally": {k: api.GeneTally(ex, report.gene_slots(k, len(p.data1), len(p.data2)), *tables[k]) for k in levels if "tally" in on[k]},
                "exceed": {k: api.ExceedCounts(ex, thr[k], perm_counts=perm) for k in levels if "exceed" in on[k]},
                "hits": {k: api.HitList(ex, cuts[k], cap=1 << 18) for k in levels if "hits" in on[k]}}

    calls = 1
    if one_call:
        ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
        try:
            obs = arm_drawn(ex)
            api.process_paths(p, exec_=ex, **{k: (v or None) for k, v in kw(obs).items()})
            got = {kind: {k: o.read() for k, o in per.items()} for kind, per in obs.items()}
        finally:
            ex.close()
    else:
        plan = api.ResidentPlan(p)
        try:
            calls = len(plan.windows())
            for _ in range(passes):
                obs = arm_drawn(plan.ex)
                plan.run(keep_inspections=keep, **{k: (v or None) for k, v in kw(obs).items()})
                got = {kind: {k: o.read() for k, o in per.items()} for kind, per in obs.items()}
        finally:
            plan.close()
    for name in levels:
        what = f"case {number} level {name}"
        if "tally" in on[name]:
            G.assert_tally(got["tally"][name], tally_ref[name], what)
        if "exceed" in on[name]:
            want = PC.reference(cpu, name, thr[name]) if perm else cpu.reference(name, thr[name])
            X.assert_counts(got["exceed"][name], want, what, observed_calls=calls)
            if perm:
                PC.assert_perm(got["exceed"][name], want, what)
        if "hits" in on[name]:
            g = got["hits"][name]
            assert g.found == hits_ref[name]["found"] and g.paths == p.levels.n_paths[name], what
            assert g.complete == (g.found <= 1 << 18), what
            if g.complete:
                H.assert_hits(g, hits_ref[name], what)
