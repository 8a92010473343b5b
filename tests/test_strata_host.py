"""Stratified set scores, host side: the confounded cohort that motivates them, worked out with the oracle's
value tables; ``report.strata_reference`` on a hand-worked six-patient example with every cell written out and against the
definition taken literally; one stratum with the cohort's own table against the observed expression of ``score_sets``;
``stratified_columns`` written out; the host plan in C++ (csrc/gcre_strata.h) -- stratum counts, table offsets, slab sizing
and every refusal with its code and message -- driven by tests/native/strata_main.cpp under the address and
undefined-behaviour sanitizers as a child process; the interface.  No GPU needed."""
from __future__ import annotations

import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from geneticscre_amd import api, report
from helpers import small_table
from oracle.values_table import values_table as oracle_values_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "strata_main.cpp")
OK, ERR_RANGE, ERR_ARG = 0, -2, -4   # include/gcre_hip.h


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


# ---- why: a gene that is merely commoner in the case-rich stratum ---------------------------------------------------------


def confounded_cohort():
    """Stratum A: 16 cases and 4 controls, the gene in 8 cases and 2 controls -- the null expectation; stratum B: 4 cases and
    16 controls, no carrier.  Columns: the 20 cases first (A's 16, then B's 4), then the 20 controls (A's 4, then B's 16)."""
    strata = np.array([0] * 16 + [1] * 4 + [0] * 4 + [1] * 16)
    gene = np.zeros(40, np.int8)
    gene[:8] = 1          # 8 of A's cases
    gene[20:22] = 1       # 2 of A's controls
    return strata, gene[None, :]


def test_confounded_cohort_pooled_against_stratified():
    strata, rows = confounded_cohort()
    tables = [oracle_values_table(16, 4), oracle_values_table(4, 16)]
    pooled = oracle_values_table(20, 20)[8, 2]
    K = 300
    masks = report.permutation_masks(20, 20, K, 7, strata)
    ref = report.strata_reference([[0]], rows, None, 20, strata, tables, masks, 1)
    print("pooled", pooled, "stratified", ref["score"][0], "terms", ref["terms"][0], "smallest null sum", ref["null_scores"][0].min())
    assert pooled > 2.7
    assert abs(ref["score"][0]) < 1e-9
    assert bits(ref["score"][0]) == bits((0.0 + tables[0][8, 2]) + tables[1][0, 0])
    assert ref["counts"][0].tolist() == [[8, 2, 0, 0], [0, 0, 0, 0]]
    # the observed counts sit at the null expectation of both strata: no stratified permutation scores lower
    assert (ref["null_scores"][0] >= ref["score"][0]).all()
    assert ref["n_ge"][0] == K
    # ... while under the same masks the pooled score is as large as observed every time: the gene's 10 carriers are all in
    # stratum A, and a mask that keeps the strata labels 16 of A's 20 patients as cases whichever they are
    pooled_null = np.array([oracle_values_table(20, 20)[(m & (rows[0] != 0)).sum(), (~m & (rows[0] != 0)).sum()] for m in masks])
    assert pooled_null.max() > 2.7 and (pooled_null >= pooled).mean() > 0.3


# ---- the definition ------------------------------------------------------------------------------------------------------

T0 = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])                    # stratum 0: 2 cases, 1 control
T1 = np.array([[10.0, 20.0, 30.0], [40.0, 50.0, 60.0]])                # stratum 1: 1 case, 2 controls
HAND_STRATA = [7, 7, 9, 7, 9, 9]                                       # Z_0 = {0, 1, 3}, Z_1 = {2, 4, 5}; cases: patients 0, 1, 2
HAND_ROWS = np.array([[1, 0, 1, 1, 0, 0],
                      [0, 1, 0, 0, 0, 1],
                      [0, 0, 0, 0, 1, 1]])
HAND_MASKS = np.array([[1, 0, 0, 1, 1, 0],                             # cases {0, 3, 4}: two of Z_0, one of Z_1
                       [0, 1, 0, 1, 0, 1],                             # cases {1, 3, 5}
                       [1, 1, 1, 0, 0, 0]], bool)                      # the observed labels


def test_reference_hand_worked_method_1():
    """The set {gene 0, gene 1}: U = {0, 1, 2, 3, 5}.
    observed    Z_0: cases {0, 1}, control {3} -> T0[2][1] = 6;   Z_1: case {2}, control {5} -> T1[1][1] = 50;   56
    mask 0      Z_0: cases {0, 3}, control {1} -> T0[2][1] = 6;   Z_1: no case, controls {2, 5} -> T1[0][2] = 30;   36
    mask 1      Z_0: cases {1, 3}, control {0} -> T0[2][1] = 6;   Z_1: case {5}, control {2} -> T1[1][1] = 50;   56
    mask 2      the observed labels: 56"""
    ref = report.strata_reference([[0, 1]], HAND_ROWS, None, 3, HAND_STRATA, [T0, T1], HAND_MASKS, 1)
    assert ref["score"].tolist() == [56.0] and ref["terms"].tolist() == [[6.0, 50.0]]
    assert ref["counts"].tolist() == [[[2, 1, 0, 0], [1, 1, 0, 0]]]
    assert ref["null_scores"].tolist() == [[36.0, 56.0, 56.0]] and ref["n_ge"].tolist() == [2]
    assert ref["family_max"].tolist() == [36.0, 56.0, 56.0]


def test_reference_hand_worked_method_2():
    """The set {+gene 0, -gene 2}: P = {0, 2, 3}, N = {4, 5}; the (-) half reads T[controls][cases].
    observed    Z_0: P case {0}, control {3} -> T0[1][1] = 4, N empty -> T0[0][0] = 1: 5
                Z_1: P case {2} -> T1[1][0] = 40, N controls {4, 5} -> T1[2][0], a row T1 does not have: -1: 39;   44
    mask 0      Z_0: P cases {0, 3} -> T0[2][0] = 5, + 1: 6;   Z_1: P control {2} -> T1[0][1] = 20, N case {4}, control {5} ->
                T1[1][1] = 50: 70;   76
    mask 1      Z_0: P case {3}, control {0} -> 4, + 1: 5;   Z_1: P control {2} -> 20, N case {5}, control {4} -> 50: 70;   75"""
    ref = report.strata_reference([[0, 2], [1, -1]], HAND_ROWS, [[1, -1], [1, 1]], 3, HAND_STRATA, [T0, T1], HAND_MASKS, 2)
    assert ref["score"][0] == 44.0 and ref["terms"][0].tolist() == [5.0, 39.0]
    assert ref["counts"][0].tolist() == [[1, 1, 0, 0], [1, 0, 2, 0]]
    assert ref["null_scores"][0].tolist() == [76.0, 75.0, 44.0] and ref["n_ge"][0] == 3
    # the set with an NA member: NaN everywhere, -1, and no part in the maxima
    assert np.isnan(ref["score"][1]) and ref["n_ge"][1] == -1 and np.isnan(ref["terms"][1]).all() and np.isnan(ref["null_scores"][1]).all()
    assert ref["counts"][1].tolist() == [[0, 0, 0, 0]] * 2
    assert ref["family_max"].tolist() == [76.0, 75.0, 44.0]
    # method 1 ignores the signs: one union
    one = report.strata_reference([[0, 2]], HAND_ROWS, [[1, -1]], 3, HAND_STRATA, [T0, T1], None, 1)
    assert one["score"].tolist() == [T0[1][1] + T1[1][2]] and one["null_scores"].shape == (1, 0) and one["n_ge"].tolist() == [0]


def literal(sets, rows, signs, n_cases, strata, tables, masks, method):
    """gcre_score_sets_strata taken literally on unpacked 0/1 arrays: one mask and one patient at a time, Python sets."""
    rows = np.asarray(rows) != 0
    n = rows.shape[1]
    ids = sorted(set(strata))
    Z = [{q for q in range(n) if strata[q] == i} for i in ids]

    def cell(VT, a, b):
        return float(VT[a][b]) if a < VT.shape[0] and b < VT.shape[1] else -1.0       # (the device's padding)

    def score(P, N, m):
        total = 0.0
        for s, z in enumerate(Z):
            term = cell(tables[s], len(P & z & m), len((P & z) - m))
            if method == 2:
                term = term + cell(tables[s], len((N & z) - m), len(N & z & m))
            total = total + term
        return total

    observed = set(range(n_cases))
    out = {"score": [], "n_ge": [], "null_scores": []}
    for s, mem in enumerate(sets):
        if any(r < 0 for r in mem):
            out["score"].append(float("nan"))
            out["n_ge"].append(-1)
            out["null_scores"].append([float("nan")] * len(masks))
            continue
        sg = [1] * len(mem) if signs is None else signs[s]
        P, N = set(), set()
        for r, g in zip(mem, sg):
            (N if method == 2 and g == -1 else P).update(np.flatnonzero(rows[r]).tolist())
        sc = score(P, N, observed)
        null = [score(P, N, set(np.flatnonzero(m).tolist())) for m in masks]
        out["score"].append(sc)
        out["null_scores"].append(null)
        out["n_ge"].append(sum(v >= sc for v in null))
    return out


@pytest.mark.parametrize("method", [1, 2])
def test_reference_equals_the_definition(method):
    rng = np.random.default_rng(220 + method)
    n_cases, n_ctrls = 11, 14
    n = n_cases + n_ctrls
    for trial in range(4):
        NS = [1, 2, 3, 5][trial]
        strata = (rng.integers(0, NS, n) * 3 + 2).tolist()               # any integers
        strata[:NS] = [3 * s + 2 for s in range(NS)]                     # every stratum has a patient
        ids = sorted(set(strata))
        tables = []
        for i in ids:
            cs = sum(strata[q] == i for q in range(n_cases))
            ts = sum(strata[q] == i for q in range(n_cases, n))
            tables.append(small_table(cs, ts, 10 * trial + len(tables)))
        if trial == 1:
            tables[0][0, 0] = np.nan
            tables[1] = tables[1][:2, :2]                                 # smaller than its stratum: cells read as -1
        if trial == 2:
            tables[2][:] = -np.inf
        rows = rng.random((9, n)) < 0.3
        sets = [rng.integers(0, 9, int(rng.integers(1, 5))).tolist() for _ in range(5)] + [[0, -1]]
        signs = [rng.choice([1, -1], len(x)).tolist() for x in sets] if trial != 3 else None
        masks = report.permutation_masks(n_cases, n_ctrls, 25, 5 + trial, strata)
        got = report.strata_reference(sets, rows, signs, n_cases, strata, tables, masks, method)
        want = literal(sets, rows, signs, n_cases, strata, tables, masks, method)
        assert np.array_equal(bits(got["score"]), bits(want["score"])), trial
        assert np.array_equal(bits(got["null_scores"]), bits(want["null_scores"])), trial
        assert got["n_ge"].tolist() == want["n_ge"], trial
        null = np.asarray(want["null_scores"][:-1])
        assert np.array_equal(bits(got["family_max"]), bits(np.where(null > 0, null, 0.0).max(axis=0))), trial
        # the masks keep every stratum's cases: what the entry verifies on the device
        for i in ids:
            z = np.array(strata) == i
            assert (masks[:, z].sum(axis=1) == z[:n_cases].sum()).all()


@pytest.mark.parametrize("method", [1, 2])
def test_one_stratum_with_the_cohorts_table_is_the_observed_score(method):
    """S = 1: the sum is +0.0 + the one term, and the term is k_set_observed's expression -- VT[cases_pos][ctrls_pos] (+
    VT[cases_neg][ctrls_neg], the (-) half counted the other way round)."""
    rng = np.random.default_rng(5)
    n_cases, n_ctrls = 13, 9
    VT = small_table(n_cases, n_ctrls, 3)
    rows = rng.random((6, n_cases + n_ctrls)) < 0.4
    sets = [[0], [1, 2], [3, 4, 5], [2, 2]]
    signs = [[1], [1, -1], [-1, 1, -1], [-1, -1]]
    ref = report.strata_reference(sets, rows, signs, n_cases, np.full(n_cases + n_ctrls, 42), [VT], None, method)
    case = np.arange(n_cases + n_ctrls) < n_cases
    for i, (m, sg) in enumerate(zip(sets, signs)):
        neg = np.array(sg) == -1 if method == 2 else np.zeros(len(m), bool)
        P = rows[np.array(m)[~neg]].any(axis=0) if (~neg).any() else np.zeros(len(case), bool)
        N = rows[np.array(m)[neg]].any(axis=0) if neg.any() else np.zeros(len(case), bool)
        want = VT[(P & case).sum(), (P & ~case).sum()]
        if method == 2:
            want = want + VT[(N & ~case).sum(), (N & case).sum()]
        assert bits(ref["score"][i]) == bits(want) and bits(ref["terms"][i, 0]) == bits(want)
        assert ref["counts"][i, 0].tolist() == [(P & case).sum(), (P & ~case).sum(), (N & ~case).sum(), (N & case).sum()]


def test_stratified_columns_written_out():
    rec = np.zeros(4, api.STRATA_SCORE)
    rec["score"] = [3.0, 0.5, np.nan, np.nan]
    rec["n_ge"] = [1, 4, -1, 0]
    fam = [1.0, 3.0, 0.0, 2.5]
    terms = [[1.0, 2.0], [0.5, 0.0], [np.nan, np.nan], [np.nan, 1.0]]
    counts = np.arange(32).reshape(4, 2, 4)
    cols = report.stratified_columns(rec, [1, 1, 0, 1], fam, terms, counts, [-3, 8], 4)
    assert list(cols) == ["StratifiedScores", "StratifiedPvalues", "StratifiedFamilyPvalues", "Score.-3", "Cases.-3", "Controls.-3",
                          "Score.8", "Cases.8", "Controls.8"]
    assert list(cols)[:3] == report.STRATIFIED_COLUMNS
    assert cols["StratifiedScores"][:2].tolist() == [3.0, 0.5] and np.isnan(cols["StratifiedScores"][2:]).all()
    assert cols["StratifiedPvalues"][[0, 1, 3]].tolist() == [0.25, 1.0, 0.0] and np.isnan(cols["StratifiedPvalues"][2])
    # max-T: 3.0 is reached by one maximum of four, 0.5 by three; a NaN score by none; the NA set has no p-value
    assert cols["StratifiedFamilyPvalues"][[0, 1, 3]].tolist() == [0.25, 0.75, 0.0] and np.isnan(cols["StratifiedFamilyPvalues"][2])
    assert cols["Score.-3"][:2].tolist() == [1.0, 0.5] and cols["Score.8"][[0, 1, 3]].tolist() == [2.0, 0.0, 1.0]
    assert cols["Cases.-3"][[0, 1, 3]].tolist() == [0 + 2, 8 + 10, 24 + 26] and cols["Controls.8"][[0, 1, 3]].tolist() == [5 + 7, 13 + 15, 29 + 31]
    assert all(np.isnan(v[2]) for v in cols.values())
    # no permutations: scores and per-stratum columns stand, the p-values do not
    cols = report.stratified_columns(rec, [1, 1, 0, 1], np.zeros(0), terms, counts, ["a", "b"], 0)
    assert cols["StratifiedScores"][0] == 3.0 and np.isnan(cols["StratifiedPvalues"]).all() and np.isnan(cols["StratifiedFamilyPvalues"]).all()
    assert "Score.a" in cols and "Controls.b" in cols
    doc = " ".join(report.stratified_columns.__doc__.split())
    assert "nominal permutation p-value" in doc and "descriptive" in doc and "no test of heterogeneity" in doc


# ---- the C++ itself --------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("strata") / "strata_main")
    # the sanitizers' runtimes are linked statically: the program then runs whatever the environment it inherits preloads
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", SRC, "-o", out], check=True)
    return out


def run_case(prog, tmp_path, case):
    lines = []
    for k, v in case:
        lines.append(" ".join([k] + [str(x) for x in (v if isinstance(v, (list, tuple)) else [v])]))
    path = tmp_path / "case.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout}\n{r.stderr}"
    return r.stdout.splitlines()


COHORT = [("n_cases", 3), ("n_ctrls", 4), ("n_sets", 2), ("iterations", 10), ("kpad", 512)]
STRATA = [("n_strata", 3), ("strata", [0, 2, 2, 1, 2, 0, 2])]          # cases: one of stratum 0, two of stratum 2
TABLES = [("nrow", [2, 1, 3]), ("ncol", [2, 2, 3]), ("tab_off", [0, 4, 6])]
W = "score_sets_strata: "


def without(case, *keys):
    return [kv for kv in case if kv[0] not in keys]


def test_native_counts_and_offsets(prog, tmp_path):
    out = run_case(prog, tmp_path, COHORT + STRATA + TABLES)
    # stratum sizes 2, 1, 4: tables of 3, 2 and 5 diagonals hold 6, 3 and 15 cells
    assert out == ["check 0 ", "cases 1 0 2", "sizes 2 1 4", "offsets 0 6 9 24"]
    out = run_case(prog, tmp_path, [("n_cases", 40), ("n_ctrls", 60), ("n_sets", 1), ("n_strata", 1), ("strata", [0] * 100),
                                    ("nrow", [1]), ("ncol", [1]), ("tab_off", [0])])
    assert out == ["check 0 ", "cases 40", "sizes 100", f"offsets 0 {101 * 102 // 2}"]
    # sixteen strata, some without a patient
    st = [15] * 5 + [0] * 2
    out = run_case(prog, tmp_path, [("n_cases", 3), ("n_ctrls", 4), ("n_sets", 1), ("n_strata", 16), ("strata", st),
                                    ("nrow", [1] * 16), ("ncol", [1] * 16), ("tab_off", list(range(16)))])
    assert out[1] == "cases 0" + " 0" * 14 + " 3" and out[2] == "sizes 2" + " 0" * 14 + " 5"
    assert out[3].split()[1:] == [str(v) for v in [0, 6] + list(range(7, 21)) + [20 + 21]]


def test_native_slab_sizing(prog, tmp_path, monkeypatch):
    monkeypatch.delenv("GCRE_STRATA_SLAB_SETS", raising=False)
    # valid sets, strata, method, dwords per row, Kpad, null_scores or not, the bound in MB -> sets per slab
    asks = [((100, 2, 1, 1564, 100352, 0, 1024), 100),             # 12,512 bytes a set: all of them
            ((100000, 4, 2, 1564, 100352, 0, 1024), 21454),        # 50,048 bytes a set: floor(2^30 / 50,048)
            ((100, 2, 1, 1564, 100352, 1, 1024), 100),
            ((5000, 2, 1, 1564, 100352, 1, 1024), 1316),           # + 802,816 bytes of doubles a set: floor(2^30 / 815,328)
            ((7, 16, 2, 4, 512, 0, 0), 1),                         # one set at the least
            ((7, 3, 1, 4, 512, 0, 3 * 48 / 2**20), 3),             # 48 bytes a set: exactly three
            ((7, 3, 1, 4, 512, 1, 2 * (48 + 4096) / 2**20), 2),
            ((0, 3, 1, 4, 512, 0, 1024), 1)]
    out = run_case(prog, tmp_path, COHORT + STRATA + TABLES + [("slab", a) for a, _ in asks])
    assert out[4:] == [f"slab {w}" for _, w in asks]
    monkeypatch.setenv("GCRE_STRATA_SLAB_SETS", "3")
    out = run_case(prog, tmp_path, COHORT + STRATA + TABLES + [("slab", (100, 2, 1, 1564, 100352, 0, 1024)), ("slab", (2, 2, 1, 4, 512, 0, 1024))])
    assert out[4:] == ["slab 3", "slab 2"]
    monkeypatch.setenv("GCRE_STRATA_SLAB_SETS", "0")               # at least one
    assert run_case(prog, tmp_path, COHORT + STRATA + TABLES + [("slab", (100, 2, 1, 1564, 100352, 0, 1024))])[4:] == ["slab 1"]


def test_native_max_mb_from_the_environment(prog, tmp_path, monkeypatch):
    big = without(COHORT, "n_sets") + [("n_sets", 1000)] + STRATA + TABLES + [("want_null", 1)]      # 4,096,000 bytes a tile
    monkeypatch.delenv("GCRE_STRATA_MAX_MB", raising=False)
    assert run_case(prog, tmp_path, big)[0] == "check 0 "
    monkeypatch.setenv("GCRE_STRATA_MAX_MB", "3.5")
    assert run_case(prog, tmp_path, big)[0] == (f"check {ERR_ARG} {W}one tile of 512 permutations of null_scores takes 4096000 bytes: "
                                                 "above GCRE_STRATA_MAX_MB = 3.500000")
    monkeypatch.setenv("GCRE_STRATA_MAX_MB", "4")
    assert run_case(prog, tmp_path, big)[0] == "check 0 "


def test_native_mask_message(prog, tmp_path):
    out = run_case(prog, tmp_path, COHORT + STRATA + TABLES + [("message", 17)])
    assert out[-1] == ("message " + W + "17 (stratum, permutation) pairs of the context's masks do not keep the cases of the stratum: the masks "
                       "must come from generate_permutations(seed, strata) with these strata")


BAD_TABLE = "the table of stratum {} must have at least one row and one column, not {} x {} at offset {}"
CHECK_CASES = [
    ("accepted", COHORT + STRATA + TABLES, OK, ""),
    ("no permutations", without(COHORT, "iterations") + STRATA + TABLES + [("want_null", 1), ("max_mb", 0)], OK, ""),
    ("no sets", without(COHORT, "n_sets") + [("n_sets", 0)] + STRATA + TABLES + [("want_null", 1), ("max_mb", 0)], OK, ""),
    ("NULL px_out", COHORT + STRATA + TABLES + [("have_px", 0)], ERR_ARG, W + "NULL argument (px_out)"),
    ("NULL stratum", COHORT + [("n_strata", 3)] + TABLES, ERR_ARG, W + "NULL argument (stratum)"),
    ("no strata", COHORT + [("n_strata", 0), ("strata", [0] * 7), ("nrow", []), ("ncol", []), ("tab_off", [])], ERR_ARG,
     W + "n_strata = 0 outside 1 .. GCRE_STRATA_MAX = 16"),
    ("negative n_strata", COHORT + [("n_strata", -1), ("strata", [0] * 7), ("nrow", []), ("ncol", []), ("tab_off", [])], ERR_ARG,
     W + "n_strata = -1 outside 1 .. GCRE_STRATA_MAX = 16"),
    ("seventeen strata", COHORT + [("n_strata", 17), ("strata", [0] * 7), ("nrow", [1] * 17), ("ncol", [1] * 17), ("tab_off", [0] * 17)],
     ERR_ARG, W + "n_strata = 17 outside 1 .. GCRE_STRATA_MAX = 16"),
    ("NULL tables", COHORT + STRATA + TABLES + [("tables", 0)], ERR_ARG, W + "NULL argument (tables, nrow, ncol or tab_off)"),
    ("NULL nrow", COHORT + STRATA + without(TABLES, "nrow"), ERR_ARG, W + "NULL argument (tables, nrow, ncol or tab_off)"),
    ("NULL ncol", COHORT + STRATA + without(TABLES, "ncol"), ERR_ARG, W + "NULL argument (tables, nrow, ncol or tab_off)"),
    ("NULL tab_off", COHORT + STRATA + without(TABLES, "tab_off"), ERR_ARG, W + "NULL argument (tables, nrow, ncol or tab_off)"),
    ("a table without rows", COHORT + STRATA + without(TABLES, "nrow") + [("nrow", [2, 0, 3])], ERR_ARG, W + BAD_TABLE.format(1, 0, 2, 4)),
    ("a table without columns", COHORT + STRATA + without(TABLES, "ncol") + [("ncol", [2, 2, -1])], ERR_ARG, W + BAD_TABLE.format(2, 3, -1, 6)),
    ("a negative offset", COHORT + STRATA + without(TABLES, "tab_off") + [("tab_off", [-4, 4, 6])], ERR_ARG, W + BAD_TABLE.format(0, 2, 2, -4)),
    ("an id above the range", COHORT + [("n_strata", 3), ("strata", [0, 2, 2, 1, 3, 0, 2])] + TABLES, ERR_RANGE, W + "stratum id out of range"),
    ("a negative id", COHORT + [("n_strata", 3), ("strata", [0, 2, 2, 1, 2, 0, -1])] + TABLES, ERR_RANGE, W + "stratum id out of range"),
    ("too many sets", without(COHORT, "n_sets") + [("n_sets", 2**31 // 16)] + STRATA + TABLES, ERR_ARG, W + "too many sets"),
    ("null_scores above the bound", COHORT + STRATA + TABLES + [("want_null", 1), ("max_mb", 0.0078)], ERR_ARG,
     W + "one tile of 512 permutations of null_scores takes 8192 bytes: above GCRE_STRATA_MAX_MB = 0.007800"),
    ("null_scores at the bound", COHORT + STRATA + TABLES + [("want_null", 1), ("max_mb", 8192 / 2**20)], OK, ""),
    ("the bound is not asked without null_scores", COHORT + STRATA + TABLES + [("max_mb", 0)], OK, ""),
]


@pytest.mark.parametrize("name,case,code,message", CHECK_CASES, ids=[c[0] for c in CHECK_CASES])
def test_argument_checks_under_sanitizers(prog, tmp_path, name, case, code, message):
    assert run_case(prog, tmp_path, case)[0] == f"check {code} {message}"


# ---- the interface ---------------------------------------------------------------------------------------------------


def test_interface_is_declared():
    header = open(os.path.join(ROOT, "include", "gcre_hip.h")).read()
    assert re.search(r"#define GCRE_ABI_VERSION 4\b", header)      # additions only
    flat = " ".join(re.sub(r"/\*.*?\*/", " ", header, flags=re.S).split())
    assert ("int gcre_score_sets_strata(gcre_ctx* ctx, const gcre_set_input* in, const int32_t* stratum, int32_t n_strata, "
            "const double* tables, const int32_t* nrow, const int32_t* ncol, const int64_t* tab_off, gcre_set_score* out, int64_t cap, "
            "int64_t* n_out, gcre_strata_score* px_out , double* terms , int32_t* counts , double* null_scores , double* family_max );") in flat
    assert "int64_t gcre_strata_launches(const gcre_ctx* ctx);" in flat
    assert "typedef struct { double score; int64_t n_ge; } gcre_strata_score;" in flat
    assert re.search(r"#define GCRE_STRATA_MAX 16\b", header) and api.STRATA_MAX == 16
    assert api.STRATA_SCORE.itemsize == 16 and api.STRATA_SCORE.names == ("score", "n_ge")
    assert [api.STRATA_SCORE.fields[k][1] for k in api.STRATA_SCORE.names] == [0, 8]
    assert {"gcre_score_sets_strata", "gcre_strata_launches"} <= set(api.EXPORTS)
    declared = set(re.findall(r"\b(gcre_[a-z0-9_]+)\s*\(", header))
    assert declared == set(api.EXPORTS)
    parent, needs, _, binds = api._FEATURES["strata"]
    assert parent == "sets" and set(needs) == set(binds) == {"gcre_score_sets_strata", "gcre_strata_launches"}
    assert len(binds["gcre_score_sets_strata"][1]) == 16
    from geneticscre_amd import build
    assert {"gcre_strata.hip", "gcre_host_strata.hip"} <= set(build.SOURCES) and "gcre_strata.h" in build.HEADERS
    kernels = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_kernels.h")).read()
    assert "struct StrataArgs" in kernels and all(f"launch_strata_{k}(" in kernels for k in ("masks", "check", "rows", "observed", "null"))
    lib = api._strata_lib()                                   # loads without a GPU
    assert lib.gcre_abi_version() == 4 and lib.gcre_strata_launches(None) == -1
    # the block table is the prefix stage's, not a copy of it
    host = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_host_strata.hip")).read()
    assert "gcre_prefix::prefix_blocks(" in host and "stable_sort" not in host
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.22" in design and "k_strata_null" in design and "Not built" in design


def test_signatures():
    st = inspect.signature(api.JoinExec.strata_tests).parameters
    assert list(st) == ["self", "sets", "rows", "signs", "strata", "tables", "family", "null", "terms"]
    assert [st[k].default for k in list(st)[3:]] == [None, None, None, False, False, False]
    assert list(inspect.signature(api.JoinExec.strata_launches).parameters) == ["self"]
    assert list(inspect.signature(report.strata_reference).parameters) == ["sets", "rows", "signs", "n_cases", "strata", "tables", "masks",
                                                                          "method"]
    sp = inspect.signature(report.score_paths).parameters
    assert "stratified" in sp and sp["stratified"].default is False and list(sp)[-1] == "family_inference"
    assert "stratified" not in inspect.signature(report.gwaspa).parameters
    doc = " ".join(report.score_paths.__doc__.split())
    assert "POOLED" in doc and "no test of heterogeneity" in doc


def test_value_errors_come_before_the_library(monkeypatch):
    ex = api.JoinExec.__new__(api.JoinExec)
    ex.num_cases, ex.num_ctrls, ex.iters = 3, 2, 0
    monkeypatch.setattr(api, "_strata_lib", lambda: None)
    rows = np.zeros((4, 5), np.int8)
    with pytest.raises(ValueError, match="strata: one id per patient is required"):
        api.JoinExec.strata_tests(ex, [[0]], rows)
    with pytest.raises(ValueError, match=r"strata: one id per patient \(5\), not 4"):
        api.JoinExec.strata_tests(ex, [[0]], rows, strata=[0, 1, 0, 1])
    with pytest.raises(ValueError, match=r"tables: one value table \(rows and columns\) per stratum \(2\)"):
        api.JoinExec.strata_tests(ex, [[0]], rows, strata=[0, 1, 0, 1, 0], tables=[np.zeros((2, 2))])
    with pytest.raises(ValueError, match="signs: one sign per member of every set"):
        api.JoinExec.strata_tests(ex, [[0, 1]], rows, signs=[[1]], strata=[0] * 5)
    with pytest.raises(ValueError, match="stratified=True needs strata"):
        report.score_paths(["A"], ["A"], np.zeros((1, 5), np.int8), 3, 2, stratified=True)
    with pytest.raises(ValueError, match="tables: one per stratum"):
        report.strata_reference([[0]], rows, None, 3, [0, 1, 0, 1, 0], [np.zeros((2, 2))], None, 1)
