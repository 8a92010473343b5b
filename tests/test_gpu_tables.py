"""Every kernel that reads the value table, on tables that hold special values or have the wrong shape (the families of
tests/helpers.py: zeros, nonfinite, tiny, huge, ladder, shapes), bit for bit against the CPU oracle in canonical order or
against the reader's own numpy definition.  What each family provokes in the oracle's results -- both zeros in one top-k
list, +inf and NaN among the scores, denormal maxima, maxima on either side of the ladders' tops -- is asserted without a
GPU in tests/test_tables_host.py (pytest -m gpu)."""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import pytest

import oracle
from geneticscre_amd import api, dist, report
from helpers import (BAND_TABLE_CASES, FLT_DENORM, FLT_MAX, MIRRORED_TABLE_CASES, TABLE_CASES, TABLE_GOLDEN_CASES, TABLE_SIZES, WIDE_TABLE_CASES, assert_same_result,
                     load_table_case, shape_tables, special_table, table_problem, zeros_cut_top_k)
from test_gpu_exchange import check_merged, run_ranks
from test_gpu_parity import set_kernel
from test_sets_host import restate

pytestmark = pytest.mark.gpu

KERNELS = ["auto", "ie", "ie-quad", "ie-m1", "ie-noprune", "sparse", "dense"]
METHODS = ["method1", "method2"]
FAMILIES = ["zeros", "nonfinite", "tiny", "huge", "ladder"]
_WANT: dict = {}


def want_of(kind, size, method, top_k, nthreads=4):
    """(problem, the oracle's canonical results), once per session."""
    key = (kind, size, method, top_k)
    if key not in _WANT:
        p = table_problem(kind, size, method, top_k=top_k)
        _WANT[key] = (p, oracle.process_paths(p, order="canonical", nthreads=nthreads))
    return _WANT[key]


def top_ks(kind, size, method):
    """7, 3000, and for the zeros the values that put a level's cut among its zero-scored paths."""
    ks = [7, 3000]
    if kind == "zeros":
        _, full = want_of(kind, size, method, 3000)
        L = TABLE_SIZES[size][5]
        cuts = [zeros_cut_top_k(full[f"lst{l}"].all_scores) for l in range(2, L + 1)]
        cuts = [k for k in cuts if k]
        assert cuts, "no level with two zero-scored paths"
        ks += sorted({cuts[0], cuts[-1]})
    return ks


def assert_levels(got, want, L, names=None, what=""):
    for lvl in range(1, L + 1):
        g = got[f"lst{lvl}"] if names is None else got[names[lvl - 1]]
        try:
            assert_same_result(g, want[f"lst{lvl}"])
        except AssertionError as e:
            raise AssertionError(f"{what} level {lvl}: {e}") from None


PLAN_NAMES = ("1b", "2", "3", "4", "5")


# ---- a. every family x both methods x the seven kernel forms, two sizes -------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("size", ["p70", "p1000"])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", FAMILIES)
def test_family_matches_oracle_in_every_kernel_form(kind, method, size, kernel, monkeypatch):
    assert (kind, size, method) in TABLE_CASES       # (its conditions are asserted in tests/test_tables_host.py)
    set_kernel(monkeypatch, kernel)
    for top_k in top_ks(kind, size, method):
        p, want = want_of(kind, size, method, top_k)
        got = api.process_paths(p)
        assert_levels(got, want, p.path_length, what=f"{kind} {method} {size} {kernel} top_k={top_k}")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("kind,size,method", list(BAND_TABLE_CASES), ids=lambda v: str(v))
def test_ladder_band_matches_oracle_in_every_kernel_form(kind, size, method, kernel, monkeypatch):
    """The ladder family's band variant: all maxima of a level within a few ladder steps of one another, below the ladders'
    tops -- what a ladder row admits one step too early is some permutation's maximum."""
    set_kernel(monkeypatch, kernel)
    key = ("band", size, method)
    if key not in _WANT:
        p = table_problem(kind, size, method, top_k=50, case=BAND_TABLE_CASES[(kind, size, method)])
        _WANT[key] = (p, oracle.process_paths(p, order="canonical", nthreads=8))
    p, want = _WANT[key]
    assert_levels(api.process_paths(p), want, p.path_length, what=f"ladder band {method} {size} {kernel}")


# The nonfinite cases above hold a NaN on one side of the diagonal only: for the signed method the library then scores
# permutations by the dense kernel whatever form is asked for.  With mirrored NaN cells vtmax stays symmetric and the pruned
# kernels themselves read NaN, -inf and +inf: their ladders, and the staircase of an empty half for each kind of table[0][0].
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("size,g00", list(MIRRORED_TABLE_CASES), ids=lambda v: str(v))
def test_mirrored_nonfinite_matches_oracle_in_the_pruned_kernels(size, g00, kernel, monkeypatch):
    if size == "p5000" and kernel not in ("auto", "ie-quad", "ie", "sparse"):
        return                                   # (the forms of section b at that width)
    set_kernel(monkeypatch, kernel)
    key = ("mirrored", size, g00)
    if key not in _WANT:
        p = table_problem("nonfinite", size, "method2", top_k=50, case=MIRRORED_TABLE_CASES[(size, g00)])
        _WANT[key] = (p, oracle.process_paths(p, order="canonical", nthreads=8))
    p, want = _WANT[key]
    assert_levels(api.process_paths(p), want, p.path_length, what=f"mirrored nonfinite g00={g00} {size} {kernel}")


@pytest.mark.parametrize("ahead", ["0", "1"])
@pytest.mark.parametrize("kernel", ["auto", "ie", "sparse"])
def test_one_context_from_a_symmetric_table_to_a_one_sided_one_and_back(kernel, ahead, monkeypatch):
    """One context: a symmetric table with masks M1 (pruned kernels), a table with one-sided NaN (dense kernel), new masks
    M2 under it, a symmetric table again.  The last stage runs the pruned kernels on M2: neither the transposed masks nor
    count planes or a launch-ahead record made for M1 may survive.  Every stage twice, inspections kept."""
    set_kernel(monkeypatch, kernel)
    monkeypatch.setenv("GCRE_AHEAD", ahead)
    seed, variant = MIRRORED_TABLE_CASES[("p1000", 1)]
    p = table_problem("nonfinite", "p1000", "method2", top_k=50, case=(seed, variant))
    one_sided = special_table("nonfinite", p.n_cases, p.n_ctrls, seed, variant - 3)
    m2 = table_problem("nonfinite", "p1000", "method2", case=(seed + 1, variant)).perm_cases
    assert m2.shape == p.perm_cases.shape and not np.array_equal(m2, p.perm_cases)
    stages = [("symmetric, M1", None, None), ("one-sided NaN, M1", one_sided, None), ("one-sided NaN, M2", None, m2),
              ("symmetric, M2", p.value_table, None)]
    plan = api.ResidentPlan(p)
    try:
        q = p
        for what, table, perms in stages:
            if table is not None:
                q = dataclasses.replace(q, value_table=table)
                plan.ex.set_value_table(table)
            if perms is not None:
                q = dataclasses.replace(q, perm_cases=perms)
                plan.ex.set_permuted_cases(perms)
            want = oracle.process_paths(q, order="canonical", nthreads=8)
            for again in (0, 1):
                got = plan.run(keep_inspections=True)
                assert_levels(got, want, p.path_length, PLAN_NAMES, f"{what} {kernel} ahead={ahead} run {again}")
    finally:
        plan.close()


# ---- b. the mask width of BASELINE configs[2]: the quad kernel and the signed staircase in their production shapes --------
@pytest.mark.parametrize("kernel", ["auto", "ie-quad", "ie", "sparse"])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", ["nonfinite", "ladder", "huge"])
def test_family_matches_oracle_at_the_baseline_mask_width(kind, method, kernel, monkeypatch):
    assert (kind, "p5000", method) in WIDE_TABLE_CASES
    set_kernel(monkeypatch, kernel)
    p, want = want_of(kind, "p5000", method, 50, nthreads=8)
    assert 79 <= (p.n_cases + p.n_ctrls + 63) // 64 <= 82
    got = api.process_paths(p)
    assert_levels(got, want, p.path_length, what=f"{kind} {method} p5000 {kernel}")


# ---- c. the same tables through the other routes: the host-side merges meet signed zeros and infinities -----------------
def route_problem(kind, method):
    """The 1,000-patient case; for the zeros with the top_k that cuts level 4 among its zeros."""
    top_k = top_ks(kind, "p1000", method)[-1] if kind == "zeros" else 15
    return want_of(kind, "p1000", method, top_k)


@pytest.mark.parametrize("env", [{"GCRE_WINDOW_TILES": "1"}, {"GCRE_CHUNK_PATHS": "64"},
                                 {"GCRE_WINDOW_TILES": "1", "GCRE_CHUNK_PATHS": "64", "GCRE_NULL_KERNEL": "ie"}],
                         ids=["window1", "chunk64", "window1-chunk64-ie"])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", ["zeros", "nonfinite"])
def test_family_through_windows_and_small_chunks(kind, method, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p, want = route_problem(kind, method)
    assert_levels(api.process_paths(p), want, p.path_length, what=f"{kind} {method} {env}")


@pytest.mark.parametrize("ahead", ["0", "1"])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", ["zeros", "nonfinite"])
def test_family_through_the_resident_plan_with_kept_inspections(kind, method, ahead, monkeypatch):
    monkeypatch.setenv("GCRE_AHEAD", ahead)
    p, want = route_problem(kind, method)
    plan = api.ResidentPlan(p)
    try:
        for keep, window in ((False, None), (True, None), (True, 2048), (False, 2048)):
            if window is not None:
                plan.set_window(window)
            got = plan.run(keep_inspections=keep)
            assert_levels(got, want, p.path_length, PLAN_NAMES, f"{kind} {method} ahead={ahead} keep={keep} window={window}")
    finally:
        plan.close()


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", ["zeros", "nonfinite"])
def test_family_on_several_device_threads(kind, method, monkeypatch):
    monkeypatch.setenv("GCRE_EXCHANGE_UNIT", "5")
    p, want = route_problem(kind, method)
    got = api.process_paths_devices(p, devices=[0, 0, 0])
    assert_levels(got, want, p.path_length, what=f"{kind} {method} three device threads")


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", ["zeros", "nonfinite"])
def test_family_in_two_shards_with_shared_thresholds(kind, method, monkeypatch):
    monkeypatch.setenv("GCRE_EXCHANGE_UNIT", "5")
    p, want = route_problem(kind, method)
    parts, _, _ = run_ranks(p, 2, p.iterations)
    check_merged(parts, want, p, p.path_length)
    for name, lvl in zip(PLAN_NAMES, range(1, p.path_length + 1)):      # ... and the zeros' signs, which == does not see
        rows = [np.stack([r[name].scores, r[name].src, r[name].trg, r[name].cases, r[name].ctrls], axis=1) for r in parts]
        best = dist.merge_topk(np.vstack(rows), p.top_k)
        w = want[f"lst{lvl}"]
        np.testing.assert_array_equal(np.ascontiguousarray(best[:, 0]).view(np.uint64), w.scores.view(np.uint64), err_msg=name)
        np.testing.assert_array_equal(best[:, 1].astype(np.int64), w.src, err_msg=name)
        np.testing.assert_array_equal(best[:, 2].astype(np.int64), w.trg, err_msg=name)


# ---- d. the other readers of the table ------------------------------------------------------------------------------------
def device_masks(ex, K, n):
    w = np.stack([ex.perm_mask(r) for r in range(K)])
    return np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def set_tables(kind, nc, nt, seed):
    """The tables score_sets reads for a family: square ones (the signed method's (-) half reads rows by control counts),
    for the shapes every wrong size."""
    n = nc + nt
    if kind == "shapes":
        return [(name, t) for name, t, _ in shape_tables(nc, nt, seed)]
    return [(f"variant{v}", special_table(kind, n, n, seed, v)) for v in range({"nonfinite": 3, "huge": 2}.get(kind, 1))]


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("kind", FAMILIES + ["shapes"])
def test_score_sets_on_every_family(kind, method):
    """gcre_score_sets (k_set_null) against tests/test_sets_host.restate: scores, counts, n_ge, p-values, the family
    maximum, and a one-set family read as that set's own null vector."""
    n, K, nc = 200, 300, 93
    nt = n - nc
    rng = np.random.default_rng(500 + method)
    rows = (rng.random((16, n)) < rng.uniform(0.02, 0.4, size=(16, 1))).astype(np.int8)
    rows[0], rows[1] = 1, 0
    sets = [rng.integers(0, 16, size=int(rng.integers(1, 9))).tolist() for _ in range(24)]
    signs = [rng.choice([-1, 1], size=len(s)).tolist() for s in sets]
    sets[0], signs[0] = [0, 1], [1, 1]                        # the full row and the empty row
    sets[1], signs[1] = [6], [-1]                             # a lone (-) gene: the (+) half reads table[0][0]
    for name, VT in set_tables(kind, nc, nt, 3):
        ex = api.JoinExec(method, nc, nt, K)
        try:
            ex.set_value_table(VT)
            ex.generate_permutations(91)
            masks = device_masks(ex, K, n)
            rec, fam = ex.score_sets(sets, rows, signs, family=True)
            with np.errstate(over="ignore", invalid="ignore"):
                want, wnull, wfam = restate(method, nc, nt, sets, rows, signs, VT if VT.size else np.full((1, 1), -1.0), masks)
            for s, w in enumerate(want):
                for f in ("valid", "cases", "ctrls", "cases_pos", "ctrls_pos", "cases_neg", "ctrls_neg", "n_ge"):
                    assert rec[f][s] == w[f], (kind, name, s, f)
                assert np.float64(rec["score"][s]).view(np.uint64) == np.float64(w["score"]).view(np.uint64) or \
                    (np.isnan(w["score"]) and np.isnan(rec["score"][s])), (kind, name, s, rec["score"][s], w["score"])
                assert rec["pvalue"][s] == w["pvalue"], (kind, name, s)
            np.testing.assert_array_equal(fam.view(np.uint32), wfam.view(np.uint32), err_msg=f"{kind} {name}")
            for s in (0, 1, 2, 5, 11):
                _, own = ex.score_sets([sets[s]], rows, [signs[s]], family=True)
                np.testing.assert_array_equal(own.view(np.uint32), wnull[s].view(np.uint32), err_msg=f"{kind} {name} set {s}")
        finally:
            ex.close()


SPECIAL_THRESHOLDS = [0.0, -0.0, np.inf, -np.inf, FLT_MAX, FLT_DENORM, 22.0]


@pytest.mark.parametrize("form", ["ie", "dense"])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", ["zeros", "huge", "tiny", "ladder", "nonfinite"])
def test_exceed_counts_on_special_tables(kind, method, form, monkeypatch):
    """gcre_exceed against report.exceed_reference: ``(double)null >= threshold`` and ``observed >= threshold`` are double
    comparisons, so a score of -0.0 reaches a threshold of 0.0 and either zero reaches -0.0.  The nonfinite case of the
    signed method has a NaN on one side of the diagonal only: the (-) half's null value is read from vtmax's mirror image."""
    from test_gpu_exceed import Cpu, LEVELS, assert_counts
    monkeypatch.setenv("GCRE_EXCEED_KERNEL", form)
    p, _ = want_of(kind, "p70", method, 15)
    cpu = Cpu(p)
    names = LEVELS[:p.path_length]
    zeros_counted = 0
    for which in ("special", "observed"):
        thr = {}
        for L, name in enumerate(names, start=1):
            r = cpu.want[f"lst{L}"]
            thr[name] = np.asarray(SPECIAL_THRESHOLDS) if which == "special" else r.scores[r.scores > -np.inf]
        ex = api.JoinExec(p.method, p.n_cases, p.n_ctrls, p.iterations)
        try:
            xs = {name: api.ExceedCounts(ex, thr[name]) for name in names}
            api.process_paths(p, exec_=ex, exceeds=xs)
            got = {k: x.read() for k, x in xs.items()}
        finally:
            ex.close()
        for name in names:
            with np.errstate(over="ignore", invalid="ignore"):
                want = cpu.reference(name, thr[name])
            assert_counts(got[name], want, f"{kind} {method} {form} {which} level {name}")
            if which == "special":     # both zero thresholds count alike: the positive paths and the zeros of either sign
                assert want["observed"][0] == want["observed"][1] == (want["scores"] >= 0).sum()
                zeros_counted += int((want["scores"] == 0).sum())
    if kind == "zeros":
        assert zeros_counted > 0, "no zero-scored path on any level"


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", ["zeros", "nonfinite"])
def test_gene_tally_on_special_tables(kind, method):
    """gcre_gene_tally against report.gene_best_reference: a gene whose best score is a zero takes the smallest ordinal
    among the zeros of either sign (and reports that path's own zero); NaN and -inf scores never enter."""
    from test_gpu_genes import LEVELS, assert_tally, one_call, reference
    zero_best = 0
    for size in ("p70", "p1000"):
        p, _ = want_of(kind, size, method, 15)
        want = reference(p)
        _, got = one_call(p)
        for name in LEVELS[:p.path_length]:
            assert_tally(got[name], want[name], f"{kind} {method} {size} level {name}")
            zero_best += int((want[name]["score"] == 0).sum())
    if kind == "zeros":
        assert zero_best > 0, "no gene whose best score is a zero"


# ---- e. tables of the wrong shape -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["auto", "dense"])
@pytest.mark.parametrize("method", METHODS)
def test_tables_of_the_wrong_shape(method, kernel, monkeypatch):
    """Cells the table does not have read as -1, through gcre_process_paths and through gcre_set_value_table with the table
    row-major and column-major; with the signed method the transposed reads fall outside a non-square table."""
    set_kernel(monkeypatch, kernel)
    for name, table, _ in shape_tables(37, 33):
        p = table_problem("shapes", "p70", method, top_k=40, table=table)
        want = oracle.process_paths(p, order="canonical")
        assert_levels(api.process_paths(p), want, p.path_length, what=f"shape {name} {method} {kernel} one call")
        for col_major in (0, 1):
            plan = api.ResidentPlan(dataclasses.replace(p, value_table=np.zeros((p.n_cases + 1, p.n_ctrls + 1))))
            try:
                raw = np.ascontiguousarray(table.T if col_major else table, dtype=np.float64)
                ptr = raw.ctypes.data_as(ctypes.c_void_p) if raw.size else None
                plan.ex._check(plan.ex._lib.gcre_set_value_table(plan.ex._h, ptr, table.shape[0], table.shape[1], col_major))
                got = plan.run()
                assert_levels(got, want, p.path_length, PLAN_NAMES, f"shape {name} {method} {kernel} col_major={col_major}")
            finally:
                plan.close()


# ---- the reference's own scoring code on the families (tests/golden/ref_cases/table_*.json) ---------------------------------
@pytest.mark.parametrize("kernel", ["auto", "ie", "sparse", "dense"])
@pytest.mark.parametrize("name", TABLE_GOLDEN_CASES)
def test_hip_matches_reference_scoring_code_on_special_tables(name, kernel, monkeypatch):
    """The HIP path against what the reference's scoring code printed for one case per family and method: score values and
    f32 null maxima bit-exact at every level, counts and ids wherever the score is not tied among all paths of the level
    (the reference's choice among ties is heap-order dependent; both zeros are one score there)."""
    set_kernel(monkeypatch, kernel)
    p, exp = load_table_case(name)
    got = api.process_paths(p)
    every = oracle.process_paths(p, order="canonical")       # only for "is this score tied among ALL paths?"
    hexes = lambda a: [f"{int(b):016x}" for b in a.view(np.uint64)]
    canon = lambda h: "0000000000000000" if h == "8000000000000000" else h      # -0.0 ties with +0.0
    for lvl in range(1, p.path_length + 1):
        e, r = exp[f"lst{lvl}"], got[f"lst{lvl}"]
        all_bits = [canon(h) for h in hexes(every[f"lst{lvl}"].all_scores)]
        # the values: bit-exact up to which of two tied zeros a slot holds (heap order there, ordinal here)
        assert [canon(h) for h in hexes(r.scores)] == [canon(h) for h in e["scores"]], (name, lvl)
        assert [f"{int(b):08x}" for b in r.null.view(np.uint32)] == e["null"], (name, lvl)
        untied = {s for s in e["scores"] if all_bits.count(canon(s)) == 1}
        assert hexes(r.scores) == e["scores"] or not set(e["scores"]) <= untied, (name, lvl)
        assert sorted((s, c, t) for s, c, t in zip(e["scores"], e["cases"], e["ctrls"]) if s in untied) == \
               sorted((s, c, t) for s, c, t in zip(hexes(r.scores), r.cases.tolist(), r.ctrls.tolist()) if s in untied), (name, lvl)
        for k, s in enumerate(e["scores"]):
            if s in untied:
                assert (r.src[k], r.trg[k]) == (e["src"][k], e["trg"][k]), (name, lvl, k)
        assert_same_result(r, every[f"lst{lvl}"])
