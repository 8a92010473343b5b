"""Westfall-Young min-P over a family of given sets (gcre_score_sets_minp), the parts that need no device:
``report.minp_reference`` -- the contract every device test compares against -- on a hand-worked example and against the
definitions taken literally, the consequences the definitions have, ``report.minp_columns``, the host plan in C++
(csrc/gcre_minp.h: slab sizing, walk order, finish), driven by tests/native/family_main.cpp under the address and
undefined-behaviour sanitizers as a child process, and the interface (header, ctypes mirror, ``score_paths``)."""
from __future__ import annotations

import inspect
import os
import re

import numpy as np
import pytest

import family_native
from geneticscre_amd import api, report

NAN = float("nan")
ONES = 0xFFFFFFFF

# four valid sets x six permutations and a set with an NA member.  Sets 0 and 1 tie in c; set 3 has a NaN score and a row
# whose values are all equal; set 2 is the most significant one.
EX_NULL = np.array([[1, 2, 3, 4, 5, 6],
                    [3, 3, 1, 1, 2, 2],
                    [0, 0, 7, 0, 0, 0],
                    [2, 2, 2, 2, 2, 2],
                    [NAN] * 6], np.float32)
EX_OBS = np.array([5.0, 3.0, 7.0, NAN, NAN])
EX_VALID = np.array([1, 1, 1, 1, 0])
EX_COUNTS = np.array([[6, 5, 4, 3, 2, 1],
                      [2, 2, 6, 6, 4, 4],
                      [6, 6, 1, 6, 6, 6],
                      [6, 6, 6, 6, 6, 6],
                      [ONES] * 6], np.uint32)


def test_the_worked_example():
    ref = report.minp_reference(EX_OBS, EX_VALID, EX_NULL)
    assert ref["n_ge"].tolist() == [2, 2, 1, 0, 0]
    np.testing.assert_array_equal(ref["counts"], EX_COUNTS)
    assert ref["counts"].dtype == np.uint32 and ref["min_count"].dtype == np.uint32
    # per permutation the smallest count of the four valid rows
    assert ref["min_count"].tolist() == [2, 2, 1, 3, 2, 1]
    # c = 2: five minima are <= 2; c = 1: two are; the NaN score 0, the NA set -1
    assert ref["n_le_minp"].tolist() == [5, 5, 2, 0, -1]
    # sets 0 and 1 without set 2 (c = 1 < 2), with the NaN-score set: minima 2 2 4 3 2 1 -> four <= 2; set 2 against all
    assert ref["n_le_stepdown"].tolist() == [4, 4, 2, 0, -1]


def test_the_example_columns():
    ref = report.minp_reference(EX_OBS, EX_VALID, EX_NULL)
    cols = report.minp_columns(ref["n_ge"], EX_VALID, EX_OBS, ref, 6)
    assert list(cols) == report.MINP_COLUMNS == ["FamilyPvaluesMinP", "FamilyPvaluesMinPStepDown"]
    np.testing.assert_array_equal(cols["FamilyPvaluesMinP"], np.array([5 / 6, 5 / 6, 2 / 6, NAN, NAN]))
    np.testing.assert_array_equal(cols["FamilyPvaluesMinPStepDown"], np.array([4 / 6, 4 / 6, 2 / 6, NAN, NAN]))
    none = report.minp_columns(ref["n_ge"], EX_VALID, EX_OBS, ref, 0)
    assert all(np.isnan(none[c]).all() for c in report.MINP_COLUMNS)
    # the monotone step: a less significant set whose own count is smaller takes the larger one
    mp = {"n_le_minp": np.array([9, 7, 8]), "n_le_stepdown": np.array([3, 6, 2])}
    cols = report.minp_columns(np.array([4, 2, 1]), np.ones(3), np.array([1.0, 2.0, 3.0]), mp, 10)
    assert cols["FamilyPvaluesMinPStepDown"].tolist() == [0.6, 0.6, 0.2]
    assert cols["FamilyPvaluesMinP"].tolist() == [0.9, 0.7, 0.8]


def literal(obs, valid, null):
    """The definitions of DESIGN.md §3.16, one set and one permutation at a time."""
    S, K = null.shape
    vs = [i for i in range(S) if valid[i]]
    c = [0] * S
    R = [[ONES] * K for _ in range(S)]
    for i in vs:
        c[i] = sum(1 for r in range(K) if float(null[i][r]) >= obs[i])           # (False for a NaN score)
        for r in range(K):
            R[i][r] = sum(1 for q in range(K) if null[i][q] >= null[i][r])
    mc = [min([R[i][r] for i in vs], default=ONES) for r in range(K)]
    mp, sd = [-1] * S, [-1] * S
    for j in vs:
        if np.isnan(obs[j]):
            mp[j] = sd[j] = 0
            continue
        mp[j] = sum(1 for r in range(K) if mc[r] <= c[j])
        keep = [i for i in vs if np.isnan(obs[i]) or not c[i] < c[j]]
        sd[j] = sum(1 for r in range(K) if min(R[i][r] for i in keep) <= c[j])
    return c, mp, sd, mc, R


def random_family(rng):
    S = int(rng.integers(1, 9))
    K = int(rng.integers(1, 13))
    levels = np.array([0.0, 0.5, 1.0, 2.5, np.inf], np.float32)[:int(rng.integers(1, 6))]
    null = rng.choice(levels, size=(S, K)).astype(np.float32)
    obs = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 2.5, 3.0, np.inf, NAN]), size=S)
    valid = (rng.random(S) < 0.85).astype(np.int32)
    null[valid == 0] = NAN
    return obs, valid, null


def test_the_reference_is_the_definitions_taken_literally():
    rng = np.random.default_rng(316)
    ties_c = ties_row = 0
    for _ in range(300):
        obs, valid, null = random_family(rng)
        ref = report.minp_reference(obs, valid, null)
        c, mp, sd, mc, R = literal(obs, valid, null)
        assert ref["n_ge"].tolist() == c
        assert ref["n_le_minp"].tolist() == mp
        assert ref["n_le_stepdown"].tolist() == sd
        assert ref["min_count"].tolist() == mc
        assert ref["counts"].tolist() == R
        scored = [c[i] for i in range(len(c)) if valid[i] and not np.isnan(obs[i])]
        ties_c += len(scored) != len(set(scored))
        ties_row += any(len(set(null[i].tolist())) < null.shape[1] for i in range(len(c)) if valid[i])
    assert ties_c > 100 and ties_row > 100      # ties in c and inside rows are common


def test_the_consequences_of_the_definitions():
    rng = np.random.default_rng(317)
    for _ in range(300):
        obs, valid, null = random_family(rng)
        ref = report.minp_reference(obs, valid, null)
        c, mp, sd, R = ref["n_ge"], ref["n_le_minp"], ref["n_le_stepdown"], ref["counts"]
        scored = np.flatnonzero((valid != 0) & ~np.isnan(obs))
        for j in scored:
            assert int((R[j] <= c[j]).sum()) == c[j]          # a set alone: its own nominal count
            assert c[j] <= sd[j] <= mp[j]
        if len(scored):
            low = scored[c[scored] == c[scored].min()]
            assert (sd[low] == mp[low]).all()                 # nothing is left out for the smallest c
        # a family of one valid set gives c for both
        for j in scored:
            one = np.zeros_like(valid)
            one[j] = 1
            alone = report.minp_reference(obs, one, null)
            assert alone["n_le_minp"][j] == alone["n_le_stepdown"][j] == c[j]
        # the step-down column is monotone in c, tied sets are equal, and it lies between the nominal and the single step
        K = null.shape[1]
        cols = report.minp_columns(c, valid, obs, ref, K)
        a = cols["FamilyPvaluesMinPStepDown"]
        for x in scored:
            assert c[x] / K <= a[x] <= cols["FamilyPvaluesMinP"][x]
            for y in scored:
                if c[x] <= c[y]:
                    assert a[x] <= a[y]
        rest = np.setdiff1d(np.arange(len(obs)), scored)
        assert np.isnan(a[rest]).all() and np.isnan(cols["FamilyPvaluesMinP"][rest]).all()


def test_no_valid_set_and_no_permutation():
    ref = report.minp_reference([1.0, 2.0], [0, 0], np.full((2, 3), NAN, np.float32))
    assert ref["n_le_minp"].tolist() == ref["n_le_stepdown"].tolist() == [-1, -1]
    assert ref["min_count"].tolist() == [ONES] * 3 and (ref["counts"] == ONES).all()
    ref = report.minp_reference([1.0, NAN, 2.0], [1, 1, 0], np.zeros((3, 0), np.float32))
    assert ref["n_le_minp"].tolist() == ref["n_le_stepdown"].tolist() == [0, 0, -1]
    assert ref["min_count"].shape == (0,) and ref["counts"].shape == (3, 0) and ref["n_ge"].tolist() == [0, 0, 0]


# ---- the host plan in C++ (csrc/gcre_minp.h), driven by tests/native/family_main.cpp under the sanitizers -------------
TOP = 0x80000000
SLAB_REFUSAL = "score_sets_minp: the null scores and counts of one set under 2 tiles of 512 permutations exceed GCRE_MINP_MAX_MB"


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return family_native.build_prog(tmp_path_factory.mktemp("minp"))


def test_native_worked_example(prog, tmp_path):
    vset = np.flatnonzero(EX_VALID).tolist()
    obs = EX_OBS[vset].tolist()
    order, ge, le, q = family_native.minp_device_part(obs, EX_NULL[vset])
    assert (order, ge, le, q) == ([3, 0, 1, 2], [2, 2, 1, 0], [0, 0, 4, 2], [2, 2, 1, 3, 2, 1])
    out = family_native.run_case(prog, tmp_path, [("n_sets", 5), ("vset", vset), ("obs", obs), ("ge", ge), ("le", le), ("q", q), ("minp", [])])
    assert out[0] == "minp" and family_native.ints(out[1], "order") == order
    # the NaN score first and never the end of a group; sets 0 and 1 tie in c: their group ends at the second
    assert family_native.ints(out[2], "meta") == [0, 2, TOP | 2, TOP | 1]
    rec = np.array(family_native.ints(out[3], "records")).reshape(5, 2)
    assert rec[:, 0].tolist() == [5, 5, 2, 0, -1] and rec[:, 1].tolist() == [4, 4, 2, 0, -1]


def test_native_walk_and_finish_edges(prog, tmp_path):
    # NaN-scored sets first, in input order, none ending a group -- not even as the last row of the walk
    out = family_native.run_case(prog, tmp_path, [("n_sets", 2), ("vset", [0, 1]), ("obs", [NAN, NAN]), ("ge", [0, 0]), ("le", [0, 0]),
                                                  ("q", [1, 1]), ("minp", [])])
    assert family_native.ints(out[1], "order") == [0, 1] and family_native.ints(out[2], "meta") == [0, 0]
    assert family_native.ints(out[3], "records") == [0, 0, 0, 0]
    # ties in c among scored sets, stable; the last row of the walk inside a tie group: its count goes to the whole group
    obs, ge = [1.0, NAN, 2.0, 3.0, 4.0], [3, 0, 7, 3, 3]
    out = family_native.run_case(prog, tmp_path, [("n_sets", 6), ("vset", [0, 1, 2, 4, 5]), ("obs", obs), ("ge", ge), ("le", [0, 2, 0, 0, 5]),
                                                  ("q", [9, 2, 4, 4]), ("minp", [])])
    assert family_native.ints(out[1], "order") == [1, 2, 0, 3, 4] == family_native.minp_walk(obs, ge)[0]
    assert family_native.ints(out[2], "meta") == [0, TOP | 7, 3, 3, TOP | 3]
    # n_le_minp against the sorted minima 2 4 4 9: c = 3 between them, c = 7 too; the invalid set 3 keeps -1 / -1
    assert family_native.ints(out[3], "records") == [1, 5, 0, 0, 3, 2, -1, -1, 1, 5, 1, 5]
    # c equal to, below and above every minimum
    out = family_native.run_case(prog, tmp_path, [("n_sets", 4), ("vset", [0, 1, 2, 3]), ("obs", [1.0, 1.0, 1.0, 1.0]), ("ge", [4, 1, 9, 2]),
                                                  ("le", [3, 2, 1, 0]), ("q", [4, 2, 4]), ("minp", [])])
    assert family_native.ints(out[1], "order") == [2, 0, 3, 1]
    assert family_native.ints(out[3], "records") == [3, 2, 0, 0, 3, 3, 1, 1]
    # one set
    out = family_native.run_case(prog, tmp_path, [("n_sets", 1), ("vset", [0]), ("obs", [0.5]), ("ge", [0]), ("le", [0]), ("q", [1]), ("minp", [])])
    assert family_native.ints(out[2], "meta") == [TOP] and family_native.ints(out[3], "records") == [0, 0]


def test_native_slab_sizing(prog, tmp_path):
    one_row = 2 * family_native.TILE * 8 / 1048576.0           # 1000 permutations: two tiles, 8 bytes a column, in MB: exact in binary
    below = float(np.nextafter(one_row, 0.0))
    asks = [((5, 1000, 512, one_row, 0), "minp_slab 0 1 "), ((5, 1000, 512, below, 0), f"minp_slab -4 0 {SLAB_REFUSAL}"),
            ((5, 1000, 512, 1024.0, 0), "minp_slab 0 5 "), ((5, 1000, 512, 1024.0, 1), "minp_slab 0 1 "),
            ((5, 1000, 512, 1024.0, 7), "minp_slab 0 5 "), ((5, 1000, 512, 3 * one_row, 0), "minp_slab 0 3 "),
            ((0, 1000, 512, below, 0), "minp_slab 0 0 "), ((5, 0, 512, below, 0), "minp_slab 0 0 ")]
    assert family_native.run_case(prog, tmp_path, [("minp_slab", a) for a, _ in asks]) == [w for _, w in asks]
    env = {k: v for k, v in os.environ.items() if not k.startswith("GCRE_")}
    for sets, want in (("0", 1), ("-2", 1), ("3", 3)):            # the test-only bound: one row at the least
        out = family_native.run_case(prog, tmp_path, [("env", [])], env={**env, "GCRE_MINP_SLAB_SETS": sets, "GCRE_MINP_MAX_MB": "0.5"})
        assert out == [f"env 1024 0 0.5 {want}"]
    assert family_native.run_case(prog, tmp_path, [("env", [])], env={**env, "GCRE_MINP_MAX_MB": "-1"}) == ["env 1024 0 0 0"]
    assert family_native.run_case(prog, tmp_path, [("env", [])], env={**env, "GCRE_MINP_MAX_MB": "2e6"}) == ["env 1024 0 1048576 0"]


def test_native_finish_on_random_families(prog, tmp_path):
    """The device's part taken literally from a null matrix, the native walk and finish, every field against the reference."""
    rng = np.random.default_rng(319)
    levels = np.array([0.0, 0.5, 1.0, 2.5, np.inf], np.float32)
    case, want = [], []
    for _ in range(200):
        S, K = int(rng.integers(1, 41)), int(rng.integers(1, 51))
        null = rng.choice(levels[:int(rng.integers(1, 6))], size=(S, K)).astype(np.float32)
        obs = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 2.5, 3.0, np.inf, NAN]), size=S)
        valid = (rng.random(S) < 0.85).astype(np.int32)
        null[valid == 0] = NAN
        vset = np.flatnonzero(valid).tolist()
        order, ge, le, q = family_native.minp_device_part(obs[vset].tolist(), null[vset])
        ref = report.minp_reference(obs, valid, null)
        assert ref["n_ge"][vset].tolist() == ge and (not vset or ref["min_count"].tolist() == q)
        case += [("n_sets", S), ("vset", vset), ("obs", obs[vset].tolist()), ("ge", ge), ("le", le), ("q", q), ("minp", [])]
        want.append((order, ref))
    out = family_native.run_case(prog, tmp_path, case)
    assert len(out) == 4 * len(want)
    for i, (order, ref) in enumerate(want):
        assert family_native.ints(out[4 * i + 1], "order") == order, i
        rec = np.array(family_native.ints(out[4 * i + 3], "records")).reshape(-1, 2)
        assert rec[:, 0].tolist() == ref["n_le_minp"].tolist(), i
        assert rec[:, 1].tolist() == ref["n_le_stepdown"].tolist(), i


def test_the_interface():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "gcre_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+GCRE_ABI_VERSION\s+4\b", header)
    assert api.EXPECTED_ABI == 4
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*gcre_minp_score\s*;", header)
    assert m and re.findall(r"int64_t\s+(\w+)\s*;", m.group(1)) == ["n_le_minp", "n_le_stepdown"]
    assert re.search(r"\bint\s+gcre_score_sets_minp\s*\(\s*gcre_ctx\s*\*", header)
    assert re.search(r"\bint64_t\s+gcre_minp_launches\s*\(\s*const\s+gcre_ctx\s*\*", header)
    assert api.MINP_SCORE.itemsize == 16 and list(api.MINP_SCORE.names) == ["n_le_minp", "n_le_stepdown"]
    assert api.MINP_SCORE.fields["n_le_stepdown"][1] == 8
    assert {"gcre_score_sets_minp", "gcre_minp_launches"} <= set(api.EXPORTS)
    parent, needs, _, binds = api._FEATURES["minp"]
    assert parent == "sets" and set(needs) == set(binds) == {"gcre_score_sets_minp", "gcre_minp_launches"}
    assert len(binds["gcre_score_sets_minp"][1]) == 8
    p = inspect.signature(report.score_paths).parameters["minp"]
    assert p.default is False
    sig = inspect.signature(api.JoinExec.minp_tests).parameters
    assert [k for k in sig][1:] == ["sets", "rows", "signs", "min_count", "counts"]
    assert sig["min_count"].default is False and sig["counts"].default is False
    assert callable(api.JoinExec.minp_launches)
