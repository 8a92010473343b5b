"""Step-down max-T counts on the device (gcre_exceed_stepdown: k_stepdown_null, k_stepdown_finish) against
their numpy definition, report.stepdown_reference, fed with operand rows and top lists from the CPU oracle.  Every comparison
of counts is exact equality of integers (pytest -m gpu).

GCRE_STEPDOWN_FUZZ_CASES=1000 [GCRE_STEPDOWN_FUZZ_BASE=...] for a long run of the seeded loop at the end; four by default."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from geneticscre_amd import api, report, synth
from helpers import small_table
from test_gpu_exceed import LEVELS, Cpu, _network_case, cpu_of

pytestmark = pytest.mark.gpu

TOP_K = 45      # every level of the problem below has more paths: m = 45, not a multiple of the 16 (8) sets of a set tile
_BIG = {}


def big(method):
    """The problem of tests/test_gpu_sets.py::test_level_family_equals_join_null_max with a longer top list."""
    if method not in _BIG:
        _BIG[method] = Cpu(synth.make_problem(34, 80, 61, 70, 700, 5, method=method, top_k=TOP_K, seed=4242,
                                              table=small_table(131, 131, 8)))
    return _BIG[method]


def top_rows(cpu, name):
    """(src, trg, scores) of the level's finite top rows, in the list's order."""
    r = cpu.want[f"lst{LEVELS.index(name) + 1}"]
    fin = np.isfinite(r.scores)
    return r.src[fin].astype(np.int64), r.trg[fin].astype(np.int64), r.scores[fin].astype(np.float64)


def sets_of(cpu, name, src, trg):
    """The joined paths (src, trg) of a level as score_sets' arguments: their union rows from the oracle's operand rows
    (method 2: the (+) half as a (+) member, the (-) half as a (-) member; the added row's halves swapped where the relation
    is not positive, UidRelSet::need_flip)."""
    p = cpu.p
    M = 1 if p.method in (1, "method1") else 2
    n = p.n_cases + p.n_ctrls
    u = p.levels.uids[name]
    r0, r1 = report._unpack_rows(cpu.ops[name][0], M, n), report._unpack_rows(cpu.ops[name][1], M, n)
    m = len(src)
    if M == 1:
        return [[i] for i in range(m)], (r0[0][src] | r1[0][trg]).astype(np.int8), None
    signs, L = np.asarray(u.signs, np.int64), int(u.path_length)
    sg = signs[src] if L > 3 else signs[trg] if L < 3 else np.where(signs[src] + signs[trg] == 0, -1, 1)
    keep = (sg == 1)[:, None]
    pos = r0[0][src] | np.where(keep, r1[0][trg], r1[1][trg])
    neg = r0[1][src] | np.where(keep, r1[1][trg], r1[0][trg])
    return [[i, m + i] for i in range(m)], np.vstack([pos, neg]).astype(np.int8), [[1, -1]] * m


def reference(cpu, name, top):
    """The definition, once per (problem, level, top list); shared and never written to."""
    refs = cpu.__dict__.setdefault("_stepdown_refs", {})
    key = (name, top[0].tobytes(), top[1].tobytes(), top[2].tobytes())
    if key not in refs:
        p = cpu.p
        want = report.stepdown_reference(p.method, p.n_cases, p.n_ctrls, p.levels.uids[name], *cpu.ops[name], p.value_table,
                                         cpu.masks, top)
        for v in want.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        refs[key] = want
    return refs[key]


def stepdown_of(ex, cpu, name, x, top):
    sets, rows, signs = sets_of(cpu, name, top[0], top[1])
    return x.stepdown(sets, rows, signs)


def check_level(ex, cpu, name, x, top, res, what):
    """One counted level against the definition and its consequences; returns (n_ge, the definition)."""
    want = reference(cpu, name, top)
    np.testing.assert_array_equal(want["scores"].view(np.uint64), top[2].view(np.uint64), err_msg=what)
    got = stepdown_of(ex, cpu, name, x, top)
    assert got.dtype == np.int64 and got.shape == (len(top[2]),)
    np.testing.assert_array_equal(got, want["n_ge"], err_msg=what)
    null = res.null.astype(np.float64)                                  # the join's own maxima, from the pruned kernels
    single = (null[None, :] >= top[2][:, None]).sum(axis=1)
    np.testing.assert_array_equal(want["single"], single, err_msg=what)
    best = top[2] == top[2].max()
    np.testing.assert_array_equal(got[best], single[best], err_msg=f"{what}: the best row")
    assert (got <= single).all(), what
    col = report.stepdown_columns(top[2], got, len(null))["PvaluesStepDown"]
    assert (col <= single / len(null)).all() and (col[best] == single[best] / len(null)).all(), what
    return got, want


def one_call(p, cpu, tops, check=True, what=""):
    """gcre_process_paths with per-permutation counters on the levels of ``tops`` (level name -> top list), then the
    step-down counts of each: level name -> n_ge."""
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    try:
        xs = {name: api.ExceedCounts(ex, top[2], perm_counts=True) for name, top in tops.items()}
        res = api.process_paths(p, exec_=ex, exceeds=xs)
        out = {}
        for name, top in tops.items():
            r = res[f"lst{LEVELS.index(name) + 1}"]
            out[name] = check_level(ex, cpu, name, xs[name], top, r, f"{what} level {name}")[0] if check else \
                stepdown_of(ex, cpu, name, xs[name], top)
        return out
    finally:
        ex.close()


# ---- 1. every level, both methods ------------------------------------------------------------------------------------


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_stepdown_equals_the_definition_on_every_level(method):
    cpu = big(method)
    p = cpu.p
    tops = {name: top_rows(cpu, name) for name in LEVELS}
    tile = 16 if method == "method1" else 8
    assert any(len(t[2]) % tile for t in tops.values()) and max(len(t[2]) for t in tops.values()) == TOP_K
    # the test can tell the feature from Pvalues: somewhere a row's count is strictly below its single-step count; and
    # tied scores occur among the top rows (the tie rule is exercised)
    gain = sum(int((reference(cpu, name, t)["n_ge"] < reference(cpu, name, t)["single"]).sum()) for name, t in tops.items())
    assert gain > 0, method
    assert any(len(set(t[2].tolist())) < len(t[2]) for t in tops.values())
    one_call(p, cpu, tops, what=method)
    # m = 1: a tile's tail is empty; m = 17: a second tile holds one set (method 2: a third)
    for m in (1, 17):
        one_call(p, cpu, {name: tuple(a[:m] for a in tops[name]) for name in ("3", "5")}, what=f"{method} m={m}")


# ---- 2. tile edges ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("K", [6, 513, 2100])
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_tile_edges(method, K):
    """K = 6: inside one 512-permutation tile; 513: one past it; 2,100: past the 2,048 unit of the counts' stride."""
    cpu = cpu_of(method, "sets", K=K)
    one_call(cpu.p, cpu, {name: top_rows(cpu, name) for name in LEVELS}, what=f"{method} K={K}")


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_three_windows(method, monkeypatch):
    """K = 4,200 under GCRE_WINDOW_TILES=1: the counts were filled by three permutation windows of one pass."""
    monkeypatch.setenv("GCRE_WINDOW_TILES", "1")
    cpu = cpu_of(method, "sets", K=4200)
    plan = api.ResidentPlan(cpu.p)
    try:
        plan.set_window(2048)
        assert len(plan.windows()) == 3
    finally:
        plan.close()
    one_call(cpu.p, cpu, {name: top_rows(cpu, name) for name in ("2", "4", "5")}, what=f"{method} three windows")


# ---- 3. wide rows ----------------------------------------------------------------------------------------------------


def test_wide_rows():
    """5,000 patients: 157 mask dwords, not a multiple of the 4-dword chunk; a handful of rows, the signed method."""
    p = synth.make_problem(30, 60, 2500, 2500, 300, 2, method="method2", top_k=7, seed=5, table=small_table(5000, 5000, 3))
    cpu = Cpu(p)
    top = top_rows(cpu, "2")
    assert 2 <= len(top[2]) <= 7
    one_call(p, cpu, {"2": top}, what="wide")


# ---- 4. how the counting pass ran does not matter ---------------------------------------------------------------------

VARIANTS = {
    "chunks": ({"GCRE_CHUNK_PATHS": "64"}, 1, False),
    "ahead_off": ({"GCRE_AHEAD": "0"}, 1, False),
    "cache_replay": ({}, 2, True),
    "counted_dense": ({"GCRE_EXCEED_KERNEL": "dense"}, 1, False),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("method", ["method1", "method2"])
def test_stepdown_does_not_depend_on_how_the_pass_ran(method, variant, monkeypatch):
    env, passes, keep = VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cpu = big(method)
    p = cpu.p
    tops = {name: top_rows(cpu, name) for name in LEVELS}
    plan = api.ResidentPlan(p)
    try:
        for _ in range(passes):
            xs = {name: api.ExceedCounts(plan.ex, top[2], perm_counts=True) for name, top in tops.items()}
            res = plan.run(keep_inspections=keep, exceeds=xs)
        if variant == "cache_replay":
            assert plan.last_profile["inspect_replays"] >= len(LEVELS), plan.last_profile
        for name, top in tops.items():
            check_level(plan.ex, cpu, name, xs[name], top, res[name], f"{method} {variant} level {name}")
    finally:
        plan.close()


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_thresholds_in_any_order(method):
    cpu = big(method)
    p = cpu.p
    rng = np.random.default_rng(8)
    tops, perms = {}, {}
    for name in ("2", "4"):
        top = top_rows(cpu, name)
        perms[name] = rng.permutation(len(top[2]))
        tops[name] = tuple(a[perms[name]] for a in top)
    got = one_call(p, cpu, tops, what=f"{method} shuffled")
    for name in tops:
        np.testing.assert_array_equal(got[name], reference(cpu, name, top_rows(cpu, name))["n_ge"][perms[name]])


# ---- 4b. the special-value tables ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("method", ["method1", "method2"])
@pytest.mark.parametrize("kind", ["zeros", "nonfinite", "tiny", "huge", "ladder"])
def test_stepdown_on_special_tables(kind, method):
    """The table families of tests/helpers.py at 70 patients (what the problems must hold -- tied scores, both zeros among the
    top rows, a row below its single-step count, non-finite top scores left out -- is asserted on the CPU in
    tests/test_seq_tables_host.py).  gcre_exceed_stepdown refuses a set whose score is not its threshold bit for bit: under
    signed zeros, denormals and sums that overflow f32 the join's score and the set's must still be one pattern, so no call
    may be refused."""
    from test_seq_tables_host import STEPDOWN_FAMILIES, stepdown_problem
    assert kind in STEPDOWN_FAMILIES
    cpu = stepdown_problem(kind, method)
    tops = {name: top_rows(cpu, name) for name in LEVELS}
    tops = {name: top for name, top in tops.items() if len(top[2])}
    assert tops
    try:
        one_call(cpu.p, cpu, tops, what=f"{kind} {method}")
    except api.GcreError as e:
        pytest.fail(f"{kind} {method}: a call was refused: {e}")


# ---- 5. refusals -----------------------------------------------------------------------------------------------------


def test_refusals():
    cpu = big("method1")
    p = cpu.p
    # the level the `bad` refusal needs: a better row `a` and a row `b` below it such that under some permutation a's own
    # null value reaches b's score and a is the ONLY joined path that does (V = 1): given twice, a counts twice (E = 2)
    pair = None
    for name in LEVELS:
        top = top_rows(cpu, name)
        m = len(top[2])
        V = report.exceed_reference(p.method, p.n_cases, p.n_ctrls, p.levels.uids[name], *cpu.ops[name], p.value_table,
                                    cpu.masks, top[2], per_permutation=True)["perm_counts"]
        own = reference(cpu, name, top)["top_null"].astype(np.float64)
        pair = next(((a, b) for b in range(m) for a in range(m)
                     if top[2][a] > top[2][b] and ((V[b] == 1) & (own[a] >= top[2][b])).any()), None)
        if pair is not None:
            break
    assert pair is not None
    want = reference(cpu, name, top)["n_ge"]
    sets, rows, signs = sets_of(cpu, name, top[0], top[1])
    ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
    lib = api._stepdown_lib()
    try:
        x = api.ExceedCounts(ex, top[2], perm_counts=True)
        api.process_paths(p, exec_=ex, exceeds={name: x})
        before = ex.stepdown_launches()
        assert before == 0

        def still_right():
            n0 = ex.stepdown_launches()
            np.testing.assert_array_equal(x.stepdown(sets, rows, signs), want)
            assert ex.stepdown_launches() == n0 + 2
            np.testing.assert_array_equal(x.stepdown(sets, rows, signs), want)     # twice: the same answer, x unchanged

        still_right()
        # a set whose score is not its threshold: rows 0 and the first with another score exchanged
        j = int(np.flatnonzero(top[2] != top[2][0])[0])
        swapped = list(sets)
        swapped[0], swapped[j] = sets[j], sets[0]
        n0 = ex.stepdown_launches()
        with pytest.raises(api.GcreError, match="stepdown: set 0: its observed score"):
            x.stepdown(swapped, rows, signs)
        assert ex.stepdown_launches() == n0
        still_right()
        # n_sets != m
        with pytest.raises(api.GcreError, match=f"{m - 1} sets for {m} thresholds"):
            x.stepdown(sets[:-1], rows, signs)
        # what gcre_score_sets refuses, and an NA member
        with pytest.raises(api.GcreError, match="stepdown: set 1 has no members"):
            x.stepdown([sets[0], []] + sets[2:], rows, signs)
        with pytest.raises(api.GcreError, match="out of range"):
            x.stepdown([[len(rows)]] + sets[1:], rows, signs)
        with pytest.raises(api.GcreError, match="stepdown: set 2 has an NA member"):
            x.stepdown(sets[:2] + [[-1]] + sets[3:], rows, signs)
        with pytest.raises(api.GcreError, match="columns"):
            x.stepdown(sets, np.zeros((len(rows), p.n_cases + p.n_ctrls + 1), np.int8), signs)
        assert ex.stepdown_launches() == n0 + 4
        # no per-permutation counts
        plain = api.ExceedCounts(ex, top[2])
        api.process_paths(p, exec_=ex, exceeds={name: plain})
        with pytest.raises(api.GcreError, match="keeps no per-permutation counts"):
            plain.stepdown(sets, rows, signs)
        # nothing counted; two passes counted
        fresh = api.ExceedCounts(ex, top[2], perm_counts=True)
        with pytest.raises(api.GcreError, match="exactly one full pass"):
            fresh.stepdown(sets, rows, signs)
        api.process_paths(p, exec_=ex, exceeds={name: fresh})
        api.process_paths(p, exec_=ex, exceeds={name: fresh})
        assert fresh.read().perms == 2 * p.iterations
        with pytest.raises(api.GcreError, match="exactly one full pass"):
            fresh.stepdown(sets, rows, signs)
        # a threshold that is not finite
        inf = api.ExceedCounts(ex, np.append(top[2][:-1], np.inf), perm_counts=True)
        api.process_paths(p, exec_=ex, exceeds={name: inf})
        with pytest.raises(api.GcreError, match="not finite"):
            inf.stepdown(sets, rows, signs)
        assert ex.stepdown_launches() == n0 + 4
        n_ge = np.zeros(m, np.int64)
        assert lib.gcre_exceed_stepdown(None, None, api._ptr(n_ge)) == api.GCRE_ERR_ARG
        assert lib.gcre_exceed_stepdown(x._h, None, api._ptr(n_ge)) == api.GCRE_ERR_ARG
        still_right()
        # the same row given twice: the kernels run (only they can tell), the call fails, nothing is returned
        a, b = pair
        twice = api.ExceedCounts(ex, top[2][[a, a, b]], perm_counts=True)
        api.process_paths(p, exec_=ex, exceeds={name: twice})
        s3, r3, g3 = sets_of(cpu, name, top[0][[a, a, b]], top[1][[a, a, b]])
        n0 = ex.stepdown_launches()
        with pytest.raises(api.GcreError, match="the sets are not distinct joined paths of the counted join"):
            twice.stepdown(s3, r3, g3)
        assert ex.stepdown_launches() == n0 + 2
        inp, keep = api._set_input(s3, r3, g3, p.n_cases + p.n_ctrls)
        out = np.full(3, -7, np.int64)
        assert lib.gcre_exceed_stepdown(twice._h, ctypes.byref(inp), api._ptr(out)) == api.GCRE_ERR_ASSERT
        assert (out == -7).all()
        del keep
        still_right()
    finally:
        ex.close()
    # the front end's limit on cells is the counters' own, checked before anything runs
    with pytest.raises(ValueError, match="2\\^26"):
        report.gwaspa(*_network_case(17)[:2], 48, 52, _network_case(17)[2], top_k=10000, n_permutations=6711, stepdown=True)


# ---- 6. the front end ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("signed", [False, True])
def test_gwaspa_stepdown(signed):
    from geneticscre_amd.uids import UidRelSet
    nc, nt, K, L = 48, 52, 700, 5
    genes, data, network = _network_case(17)
    strata = (np.arange(nc + nt) * 5 % 3).astype(np.int32)
    kw = dict(signed=signed, threshold=0.2, n_permutations=K, strata=strata, seed=909, top_k=6, path_length=L)
    base = report.gwaspa(genes, data, nc, nt, network, **kw)
    out = report.gwaspa(genes, data, nc, nt, network, stepdown=True, **kw)
    assert set(out) == set(base) | {"stepdown"}
    df = out["GWASPA.Results"]
    assert list(df.columns) == report.COLUMNS + report.STEPDOWN_COLUMNS
    assert df[report.COLUMNS].equals(base["GWASPA.Results"])                 # every other column, and the row order
    for c in report.COLUMNS:
        a, b = df[c].to_numpy(), base["GWASPA.Results"][c].to_numpy()
        assert a.dtype == b.dtype and (a.tobytes() == b.tobytes() if a.dtype != object else list(a) == list(b)), c
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
    p = synth.Problem(method, nc, nt, L, 6, K, levels, prep.data1, prep.data2, api.values_table(nc, nt),
                      np.ones((1, nc + nt), np.int32), 0)
    cpu = Cpu(p)
    cpu.masks = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :nc + nt].astype(bool)
    for Lx, name in enumerate(LEVELS, start=1):
        lst = out["levels"][f"lst{Lx}"]
        fin = np.isfinite(lst.scores)
        top = (lst.src[fin].astype(np.int64), lst.trg[fin].astype(np.int64), lst.scores[fin].astype(np.float64))
        want = report.stepdown_reference(method, nc, nt, levels.uids[name], *cpu.ops[name], p.value_table, cpu.masks, top)
        np.testing.assert_array_equal(out["stepdown"][Lx], want["n_ge"], err_msg=f"length {Lx}")
        cols = report.stepdown_columns(top[2], want["n_ge"], K)
        rows = df[df["Lengths"] == Lx]
        by_score = {t: i for i, t in enumerate(top[2].tolist())}
        exp = np.array([cols["PvaluesStepDown"][by_score[sc]] if np.isfinite(sc) else np.nan for sc in rows["Scores"]])
        np.testing.assert_array_equal(rows["PvaluesStepDown"].to_numpy(np.float64), exp)
        sc = rows["Scores"].to_numpy(np.float64)
        ok = np.isfinite(sc)
        sd, pv = rows["PvaluesStepDown"].to_numpy(np.float64), rows["Pvalues"].to_numpy(np.float64)
        assert np.isnan(sd[~ok]).all() and (sd[ok] <= pv[ok]).all()
        assert (sd[ok][sc[ok] == sc[ok].max()] == pv[ok][sc[ok] == sc[ok].max()]).all()
    # with false_counts too: one pass, one set of counters, the same numbers
    both = report.gwaspa(genes, data, nc, nt, network, stepdown=True, false_counts=True, **kw)
    assert set(both) == set(base) | {"stepdown", "exceed"}
    assert list(both["GWASPA.Results"].columns) == report.COLUMNS + report.false_count_names() + report.STEPDOWN_COLUMNS
    assert both["GWASPA.Results"][report.COLUMNS + report.STEPDOWN_COLUMNS].equals(df)
    # no permutations: a NaN column
    none = report.gwaspa(genes, data, nc, nt, network, stepdown=True, **dict(kw, n_permutations=0, strata=None))
    assert np.isnan(none["GWASPA.Results"]["PvaluesStepDown"].to_numpy()).all()


# ---- 7. seeded loop --------------------------------------------------------------------------------------------------
N_FUZZ = int(os.environ.get("GCRE_STEPDOWN_FUZZ_CASES", "4"))
FUZZ_BASE = int(os.environ.get("GCRE_STEPDOWN_FUZZ_BASE", "0"))


@pytest.mark.parametrize("case", range(N_FUZZ))
def test_random_problem_stepdown_equals_the_definition(case, monkeypatch):
    """helpers.fuzz_problem's draws (sizes, methods, path lengths, tables with ties) under the knob draws of
    tests/test_gpu_fuzz.py, plus the counting form; every level's finite top rows."""
    from helpers import fuzz_problem
    from test_gpu_fuzz import draw, entered
    number = FUZZ_BASE + case
    entered("stepdown", number)
    _, env = draw(700000 + number)
    env["GCRE_EXCEED_KERNEL"] = ["", "ie", "dense"][number % 3]
    for k, v in env.items():
        if v:
            monkeypatch.setenv(k, v)
    _, p = fuzz_problem(number)
    cpu = Cpu(p)
    tops = {name: top_rows(cpu, name) for name in LEVELS[:p.path_length]}
    tops = {name: t for name, t in tops.items() if len(t[2])}
    got = one_call(p, cpu, tops, what=f"case {number}")
    gain = sum(int((got[name] < reference(cpu, name, t)["single"]).sum()) for name, t in tops.items())
    rows = sum(len(t[2]) for t in tops.values())
    path = os.environ.get("GCRE_STEPDOWN_FUZZ_SUMMARY")
    if path:
        with open(path, "a") as f:
            f.write(f"case {number} method {p.method} patients {p.n_cases + p.n_ctrls} perms {p.iterations} "
                    f"levels {len(tops)} rows {rows} below_single_step {gain}\n")
