"""The sequential p-values of the two adaptive set tests off the device: ``report.adaptive_sequential_reference``
on hand-worked matrices; the host plan of csrc/gcre_seq_prefix.h -- argument checks, the slab walk, the first active list of
every slab, the sum of the sets still active at a left-over permutation, the launches -- driven by
tests/native/seq_prefix_main.cpp under the address and undefined-behaviour sanitizers and compared with a restatement in
Python; the row variants of csrc/gcre_steps.h and the budget readers of csrc/gcre_env.h, driven by tests/native/steps_main.cpp
under the same sanitizers against values written down by hand; and what ``JoinExec.prefix_sequential_tests`` /
``dose_sequential_tests`` refuse before they reach the library.  No GPU."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from geneticscre_amd import api, report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "seq_prefix_main.cpp")
ERR_ARG, ERR_RANGE = api.GCRE_ERR_ARG, api.GCRE_ERR_RANGE
WHO_P, WHO_D = "score_sets_prefix_sequential: ", "score_sets_dose_sequential: "
NONE = report.WEIGHTED_NONE


# ---- the reference on hand-worked matrices -------------------------------------------------------------------------------------


def hand_case():
    """Four sets: set 0 of three steps whose null maximum moves between the steps from one permutation to the next; set 1 of
    two steps, the first NaN; set 2 of one step, NaN; set 3 invalid.  Ten permutations."""
    step_set = [0, 0, 0, 1, 1, 2, 3]
    step_obs = [1.0, 3.0, 2.0, np.nan, 2.0, np.nan, 5.0]
    null = np.zeros((7, 10), np.float32)
    #                 r: 0  1  2  3  4  5  6  7  8  9
    null[0] = [3, 0, 0, 0, 1, 0, 0, 3, 0, 0]        # set 0: the maximum is at step 0 in r = 0 and 7,
    null[1] = [0, 4, 0, 0, 2, 0, 0, 0, 2, 0]        # at step 1 in r = 1, 4 and 8,
    null[2] = [1, 0, 2, 0, 0, 0, 3, 0, 0, 0]        # at step 2 in r = 2 and 6: T = 3 4 2 0 2 0 3 3 2 0, score 3
    null[3] = [0, 0, 9, 0, 0, 0, 0, 0, 0, 2]        # set 1: the NaN step still counts under the permutations (folded values)
    null[4] = [0, 1, 0, 0, 2, 0, 0, 0, 0, 0]        # T = 0 1 9 0 2 0 0 0 0 2, score 2
    null[5] = [7, 7, 7, 7, 7, 7, 7, 7, 7, 7]        # set 2: a NaN score never counts
    null[6] = 9
    return step_obs, null, step_set, 4, [1, 1, 1, 0]


def test_reference_maximum_moves_between_the_steps():
    obs, null, owner, S, valid = hand_case()
    ref = report.adaptive_sequential_reference(obs, null, owner, S, valid, 3, 10)
    np.testing.assert_array_equal(ref["score"], [3.0, 2.0, np.nan, np.nan])
    np.testing.assert_array_equal(ref["best_step"], [1, 1, -1, -1])
    # set 0: T >= 3 at r = 0, 1, 6, 7: the third at position 7.  set 1: T >= 2 at r = 2, 4, 9: the third at position 10 =
    # max_perms exactly -- hits reached on the last permutation.  set 2: NaN, nothing.  set 3: invalid
    np.testing.assert_array_equal(ref["n_hit"], [3, 3, 0, -1])
    np.testing.assert_array_equal(ref["n_perm"], [7, 10, 10, -1])
    np.testing.assert_array_equal(ref["stopped"], [1, 1, 0, 0])
    assert ref["n_hit"].dtype == np.int64 and ref["stopped"].dtype == np.int32
    # one permutation fewer: set 1 no longer stops
    ref = report.adaptive_sequential_reference(obs, null, owner, S, valid, 3, 9)
    np.testing.assert_array_equal(ref["n_hit"], [3, 2, 0, -1])
    np.testing.assert_array_equal(ref["n_perm"], [7, 9, 9, -1])
    np.testing.assert_array_equal(ref["stopped"], [1, 0, 0, 0])
    # the NaN step is inside the null maximum: without it set 1 would have two exceedances, not three
    assert (np.maximum(null[3], null[4]) >= 2).sum() == 3 and (null[4] >= 2).sum() == 1
    # it is prefix_reference's score and null_max fed to sequential_reference
    pr = report.prefix_reference(obs, null, owner, S, valid)
    sr = report.sequential_reference(pr["null_max"], pr["score"], valid, 3, 10)
    again = report.adaptive_sequential_reference(obs, null, owner, S, valid, 3, 10)
    for k in ("n_hit", "n_perm", "stopped"):
        np.testing.assert_array_equal(sr[k], again[k])


def test_reference_without_permutations():
    obs, null, owner, S, valid = hand_case()
    for nul in (null, null[:, :0]):
        ref = report.adaptive_sequential_reference(obs, nul, owner, S, valid, 3, 0)
        np.testing.assert_array_equal(ref["n_hit"], [0, 0, 0, -1])
        np.testing.assert_array_equal(ref["n_perm"], [0, 0, 0, -1])
        np.testing.assert_array_equal(ref["stopped"], [0, 0, 0, 0])
        np.testing.assert_array_equal(ref["score"], [3.0, 2.0, np.nan, np.nan])
    with pytest.raises(ValueError):
        report.adaptive_sequential_reference(obs, null, owner, S, valid, 0, 10)
    with pytest.raises(ValueError):
        report.adaptive_sequential_reference(obs, null, owner, S, valid, 3, 11)      # more permutations than null scores


def test_reference_weighted_rule():
    """R in front of, at and behind the last stop.  Without the NaN set (always active) sets 0 and 1 stop at 7 and 10."""
    obs, null, owner, S, valid = hand_case()
    keep = [0, 1, 2, 3, 4, 6]                                     # set 2 left out: its one step
    obs2, null2, owner2 = [obs[i] for i in keep], null[keep], [0, 0, 0, 1, 1, 2]
    valid2 = [1, 1, 0]

    def att(R):
        a = np.ones((10, 2), np.uint32)
        if R is not None:
            a[R, 1] = NONE
        return a

    ref = report.adaptive_sequential_reference(obs2, null2, owner2, 3, valid2, 3, 10, attempts=att(None))
    assert ref["first_left_over"] is None and not ref["refused"] and ref["n_active"] == 0
    np.testing.assert_array_equal(ref["n_perm"], [7, 10, -1])
    # R = 8: in front of the last stop (position 10): set 1 is still active there -- refused
    ref = report.adaptive_sequential_reference(obs2, null2, owner2, 3, valid2, 3, 10, attempts=att(8))
    assert ref["first_left_over"] == 8 and ref["refused"] and ref["n_active"] == 1
    np.testing.assert_array_equal(ref["stopped"], [1, 0, 0])
    # R = 9: permutation 9 itself is set 1's third exceedance and is never drawn -- still refused
    ref = report.adaptive_sequential_reference(obs2, null2, owner2, 3, valid2, 3, 10, attempts=att(9))
    assert ref["first_left_over"] == 9 and ref["refused"] and ref["n_active"] == 1
    # two hits: set 1 stops at position 5, set 0 at 2; R = 5 is AT the last stop (n_perm <= R): complete
    ref = report.adaptive_sequential_reference(obs2, null2, owner2, 3, valid2, 2, 10, attempts=att(5))
    assert ref["first_left_over"] == 5 and not ref["refused"] and ref["n_active"] == 0
    np.testing.assert_array_equal(ref["n_perm"], [2, 5, -1])
    # R = 4: one in front of it -- refused; R = 7: behind it -- complete
    assert report.adaptive_sequential_reference(obs2, null2, owner2, 3, valid2, 2, 10, attempts=att(4))["refused"]
    ref = report.adaptive_sequential_reference(obs2, null2, owner2, 3, valid2, 2, 10, attempts=att(7))
    assert not ref["refused"] and ref["first_left_over"] == 7
    # with the all-NaN set on the list any R refuses
    ref = report.adaptive_sequential_reference(obs, null, owner, S, valid, 2, 10, attempts=att(7))
    assert ref["refused"] and ref["n_active"] == 1


# ---- the C++ itself ---------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("seq_prefix") / "seq_prefix_main")
    # a program with a main of its own; the sanitizers' runtimes are linked statically, nothing is preloaded
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", SRC, "-o", out], check=True)
    return out


def run_case(prog, tmp_path, case):
    lines = [" ".join([k] + [str(x) for x in (v if isinstance(v, (list, tuple)) else [v])]) for k, v in case]
    path = tmp_path / "case.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout}\n{r.stderr}"
    return r.stdout.splitlines()


def set_lines(sets):
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(int).tolist()
    return [("n_sets", len(sets)), ("set_off", off), ("members", [m for s in sets for m in s])]


def plan(sets, cuts, levels, nan, weighted, method, w32p, max_mb, slab_sets, loops):
    """The restatement: the slabs of whole valid sets, every slab's first active list -- step count descending, ties by slot;
    a NaN score off the list unless weighted -- its launches, and the totals."""
    valid = [s for s in range(len(sets)) if all(m >= 0 for m in sets[s])]
    if levels is not None:
        steps = [len(levels)] * len(valid)
    else:
        steps = [sum(1 for i in range(len(sets[s])) if cuts is None or cuts[s][i] or i + 1 == len(sets[s])) for s in valid]
    slabs, cur, size = [], [], 0.0
    for v, n in enumerate(steps):
        b = n * method * w32p * 4.0
        if cur and (size + b > max_mb * 1048576.0 or (slab_sets and len(cur) >= slab_sets)):
            slabs.append(cur)
            cur, size = [], 0.0
        cur.append(v)
        size += b
    if cur:
        slabs.append(cur)
    out = []
    left, stratum, active = -1, -1, 0
    for i, slab in enumerate(slabs):
        out.append(f"slab {slab[0]} {len(slab)} {sum(steps[v] for v in slab)}")
        order = sorted(range(len(slab)), key=lambda e: (-steps[slab[e]], e))
        out.append(" ".join(["active"] + [str(e) for e in order if weighted or not nan[slab[e]]]))
        if loops:
            lo, st, ac, batches = loops[i]
            if lo >= 0:
                left, stratum, active = lo, st, active + ac
            out.append(f"launches {3 + (4 if weighted else 3) * batches}")
    out.append(f"total {int(left >= 0 and active > 0)} {left} {stratum} {active}")
    return out


def random_case(rng):
    S = int(rng.integers(1, 25))
    sets = [rng.integers(0, 50, int(rng.integers(1, 15))).tolist() for _ in range(S)]
    for s in rng.integers(0, S, int(rng.integers(0, 3))).tolist():
        sets[s][int(rng.integers(len(sets[s])))] = -1
    dose = rng.random() < 0.4
    levels = sorted(rng.choice(np.arange(1, 16), int(rng.integers(1, 6)), replace=False).tolist()) if dose else None
    cuts = None if dose or rng.random() < 0.3 else [(rng.random(len(s)) < 0.5).astype(int).tolist() for s in sets]
    n_valid = sum(all(m >= 0 for m in s) for s in sets)
    nan = (rng.random(n_valid) < 0.25).astype(int).tolist()
    weighted = int(rng.random() < 0.5)
    method, w32p = int(rng.integers(1, 3)), int(rng.choice([8, 16, 40]))
    slab_sets = int(rng.choice([0, 0, 1, 3, 4]))
    max_mb = float(rng.choice([1024.0, 15 * method * w32p * 4 / 1048576.0, 40 * method * w32p * 4 / 1048576.0]))
    return sets, cuts, levels, nan, weighted, method, w32p, max_mb, slab_sets


@pytest.mark.parametrize("case", range(12))
def test_native_plan_equals_the_restatement(prog, tmp_path, case):
    rng = np.random.default_rng([7800, case])
    sets, cuts, levels, nan, weighted, method, w32p, max_mb, slab_sets = random_case(rng)
    base = set_lines(sets) + [("method", method), ("w32p", w32p), ("max_mb", repr(max_mb)), ("slab_sets", slab_sets), ("nan", nan),
                              ("weighted", weighted), ("hits", 5), ("max_perms", 1000)]
    base += [("levels", levels)] if levels is not None else ([("cut", [c for x in cuts for c in x])] if cuts is not None else [])
    first = run_case(prog, tmp_path, base)
    assert first[0] == "check 0 "
    want = plan(sets, cuts, levels, nan, weighted, method, w32p, max_mb, slab_sets, None)
    assert first[1:] == want
    # every slab behind its loop: some meet R (weighted only) with sets still active, some with none
    n_slabs = sum(1 for ln in want if ln.startswith("slab"))
    R = int(rng.integers(0, 1000))
    loops = [(R if weighted and rng.random() < 0.6 else -1, 2, int(rng.integers(0, 3)), int(rng.integers(0, 9))) for _ in range(n_slabs)]
    got = run_case(prog, tmp_path, base + [("loop", list(lo)) for lo in loops])
    assert got[1:] == plan(sets, cuts, levels, nan, weighted, method, w32p, max_mb, slab_sets, loops)


def test_native_first_list_by_hand(prog, tmp_path):
    """Steps 1, 3, 3, 5, 1 (the second set's middle cut is off: 2 steps ... ), a NaN set, ties by slot."""
    sets = [[1], [2, 3, 4], [5, 6, 7], [1, 2, 3, 4, 5], [9, -1], [8]]
    cuts = [[1], [1, 0, 1], [1, 1, 1], [1, 1, 1, 1, 1], [1, 1], [0]]
    base = set_lines(sets) + [("cut", [c for x in cuts for c in x]), ("hits", 5), ("max_perms", 100)]
    # valid sets 0, 1, 2, 3, 5 with 1, 2, 3, 5, 1 steps; slot 2 (3 steps) has a NaN score
    out = run_case(prog, tmp_path, base + [("nan", [0, 0, 1, 0, 0])])
    assert out == ["check 0 ", "slab 0 5 12", "active 3 1 0 4", "total 0 -1 -1 0"]
    out = run_case(prog, tmp_path, base + [("nan", [0, 0, 1, 0, 0]), ("weighted", 1)])
    assert out == ["check 0 ", "slab 0 5 12", "active 3 2 1 0 4", "total 0 -1 -1 0"]
    # two sets a slab; the active sets at R = 40 are summed over the slabs that reached it: 1 + 0 + 2
    out = run_case(prog, tmp_path, base + [("nan", [0, 0, 1, 0, 0]), ("weighted", 1), ("slab_sets", 2), ("loop", [40, 1, 1, 2]),
                                           ("loop", [40, 1, 0, 1]), ("loop", [40, 1, 2, 0])])
    assert out == ["check 0 ", "slab 0 2 3", "active 1 0", "launches 11", "slab 2 2 8", "active 1 0", "launches 7", "slab 4 1 1", "active 0",
                   "launches 3", "total 1 40 1 3"]
    # every set stopped in front of R in every slab: complete
    out = run_case(prog, tmp_path, base + [("nan", [0, 0, 0, 0, 0]), ("weighted", 1), ("slab_sets", 4), ("loop", [40, 0, 0, 2]),
                                           ("loop", [-1, -1, 0, 1])])
    assert out[-1] == "total 0 40 0 0"


def test_native_refusals(prog, tmp_path):
    sets = [[1, 2, 3], [4, -1], [5, 6]]
    base = set_lines(sets) + [("nan", [0, 0])]
    hits0 = "hits = 0 outside 1 .. 2147483647"
    for who, extra in ((WHO_P, []), (WHO_D, [("levels", [1, 2])])):
        b = base + extra
        assert run_case(prog, tmp_path, b + [("hits", 0)]) == [f"check {ERR_ARG} {who}{hits0}"]
        assert run_case(prog, tmp_path, b + [("max_perms", -1)]) == [f"check {ERR_ARG} {who}max_perms = -1 outside 0 .. 1099511627776"]
        assert run_case(prog, tmp_path, b + [("have_seq", 0)]) == [f"check {ERR_ARG} {who}NULL argument (seq_out)"]
        what = "px_out" if who == WHO_P else "dose_out"
        # the statistic's own arguments are read first
        assert run_case(prog, tmp_path, b + [("have_out", 0), ("hits", 0)]) == [f"check {ERR_ARG} {who}NULL argument ({what})"]
    # a set whose step rows do not fit GCRE_PREFIX_MAX_MB: refused where permutations are drawn, not without them
    tiny = repr(2 * 8 * 4 / 1048576.0)                              # two rows of 8 dwords
    out = run_case(prog, tmp_path, base + [("max_mb", tiny), ("w32p", 8)])
    assert out == [f"check {ERR_ARG} {WHO_P}the 3 step rows of set 0 take 96 bytes: above GCRE_PREFIX_MAX_MB = {float(tiny):.6f}"]
    assert run_case(prog, tmp_path, base + [("max_mb", tiny), ("w32p", 8), ("max_perms", 0)])[0] == "check 0 "
    out = run_case(prog, tmp_path, base + [("max_mb", tiny), ("w32p", 8), ("levels", [1, 2, 3])])
    assert out == [f"check {ERR_ARG} {WHO_D}the 3 level rows of set 0 take 96 bytes: above GCRE_PREFIX_MAX_MB = {float(tiny):.6f}"]
    # the levels
    assert run_case(prog, tmp_path, base + [("levels", [2, 2])]) == [f"check {ERR_ARG} {WHO_D}the levels are not strictly ascending (2 after 2)"]
    assert run_case(prog, tmp_path, base + [("levels", [16])]) == [f"check {ERR_ARG} {WHO_D}level 16 (index 0) is outside 1 .. 15"]


# ---- the two row variants the resident and the sequential stages share (csrc/gcre_steps.h), the budget readers (csrc/gcre_env.h) ----


@pytest.fixture(scope="module")
def steps_prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("steps") / "steps_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tests", "native", "steps_main.cpp"), "-o", out], check=True)
    return out


def run_steps(steps_prog, what, env=None):
    keep = {k: v for k, v in os.environ.items() if k not in ("GCRE_TEST_MB", "GCRE_TEST_COUNT")}
    r = subprocess.run([steps_prog, what], capture_output=True, text=True, timeout=300, env={**keep, **(env or {})})
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout}\n{r.stderr}"
    return r.stdout.splitlines()


def test_native_records_of_both_variants_by_hand(steps_prog):
    """Sets [3, NA, 5], [1, 2, 9] and [4, 6, 7, 8] with cuts 1 1 1 | 0 0 0 | 0 1 0 1: three, one and two steps.  Set 1's pick is NaN,
    set 2's is step 1 (members 4, level 3).  Every record starts as 0x5a bytes and every score as 7."""
    nan10 = " ".join(["nan"] * 10)
    assert run_steps(steps_prog, "records") == [
        f"check {ERR_ARG} who: too many sets or members",                 # in front of the steps, resident and sequential
        f"check_seq {ERR_ARG} who: too many sets or members",
        "check 0 ",
        # score n_ge best_step best_members steps, four counts
        "px nan -1 -1 0 3 0 0 0 0",                                       # the defaults: -1 for the NA set, the steps of every set
        "px nan 0 -1 0 1 0 0 0 0",
        "px nan 0 -1 0 2 0 0 0 0",
        f"step_scores {nan10}",
        "px nan -1 -1 0 3 0 0 0 0",                                       # never written
        "px nan 0 -1 0 1 0 0 0 0",                                        # a NaN pick: no step, no members, zeros; n_ge stands
        "px 2.5 0 1 4 2 5 6 7 8",                                         # step 1 ends at the set's fourth member
        "step_scores nan nan nan nan nan nan nan 1.5 nan 2.5",            # at the members that end a step
        "vsteps 1 2",
        "row0 0 1 3",                                                     # the running sum over the slab's sets
        "row0 0 2",
        "check_seq 0 ",
        "bare 1 2 4",                                                     # without cuts every member ends a step
        # score n_ge best_index best_level levels, four counts, pad
        "ds nan -1 -1 0 2 0 0 0 0 0",
        "ds nan 0 -1 0 2 0 0 0 0 0",
        "ds nan 0 -1 0 2 0 0 0 0 0",
        "level_scores nan nan nan nan nan nan",
        "ds nan -1 -1 0 2 0 0 0 0 0",
        "ds nan 0 -1 0 2 0 0 0 0 0",
        "ds 4 0 1 3 2 1 2 3 4 0",                                         # index 1 of the levels 1, 3
        "level_scores nan nan nan nan 3 4",                               # [set][level]
        "vsteps 2 2",
        "row0 0 2 4",
        "row0 0 2",
    ]


ENV_CASES = [(None, None, "1024", "0"), ("-3", "-5", "0", "1"), ("1e9", "7", "65536", "7"), ("0.25", "7.9", "0.25", "7"),
             ("65536.5", "0", "65536", "1"), ("abc", "", "0", "1"), ("12", str(2**40), "12", str(2**40))]


@pytest.mark.parametrize("mb,count,want_mb,want_count", ENV_CASES, ids=[f"{c[0]}-{c[1]}" for c in ENV_CASES])
def test_native_budget_readers_clamp(steps_prog, mb, count, want_mb, want_count):
    """Unset: the default and 0 = no bound; else the MB clamped to [0, cap], fractions kept, and the count at least 1."""
    env = {k: v for k, v in (("GCRE_TEST_MB", mb), ("GCRE_TEST_COUNT", count)) if v is not None}
    assert run_steps(steps_prog, "env", env) == [f"mb {want_mb}", f"count {want_count}"]


# ---- what the binding refuses before it reaches the library ------------------------------------------------------------------------


def bare_context(nc=4, nt=3):
    ex = api.JoinExec.__new__(api.JoinExec)
    ex.method, ex.num_cases, ex.num_ctrls, ex.iters, ex._h, ex._lib = 1, nc, nt, 0, None, None
    return ex


def test_marshalling_refusals(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(api, "_feature_lib", no_library)
    monkeypatch.setattr(api, "load_library", no_library)
    ex = bare_context()
    sets, rows = [[0, 1], [1]], np.zeros((2, 7), np.int8)
    try:
        for cuts in ([[1, 1]], [[1], [1]], [[1, 1], [1, 0]]):
            with pytest.raises(ValueError, match="cuts: one flag per member of every set"):
                ex.prefix_sequential_tests(sets, rows, cuts=cuts)
        flat = (np.array([0, 2, 3]), np.array([0, 1, 1]))
        with pytest.raises(ValueError, match="cuts: one flag per member of every set"):
            ex.prefix_sequential_tests(flat, rows, cuts=[1, 1])
        for levels, text in (((), "1 to 15 levels"), ((1, 1), "strictly ascending"), ((0,), "every level in 1 .. 15"), ((1.5,), "whole numbers"),
                             ([[1, 2]], "one list"), (tuple(range(1, 17)), "1 to 15 levels")):
            with pytest.raises(ValueError, match=text):
                ex.dose_sequential_tests(sets, rows, levels=levels)
        for call, kw in ((ex.prefix_sequential_tests, {}), (ex.dose_sequential_tests, {})):
            with pytest.raises(ValueError, match=r"odds: one value per patient \(7\), not 6"):
                call(sets, rows, odds=np.ones(6), **kw)
            with pytest.raises(ValueError, match=r"strata: one id per patient \(7\), not 3"):
                call(sets, rows, strata=[0, 1, 0], **kw)
            with pytest.raises(ValueError, match=r"strata: one id per patient \(7\), not 8"):
                call(sets, rows, odds=np.ones(7), strata=np.zeros(8), **kw)
            with pytest.raises(ValueError, match="signs: one sign per member of every set"):
                call(sets, rows, signs=[[1], [1]], **kw)
    finally:
        ex._h = None


def test_exports_and_bindings():
    assert {"gcre_score_sets_prefix_sequential", "gcre_score_sets_dose_sequential", "gcre_seq_prefix_launches"} <= set(api.EXPORTS)
    parent, needs, what, binds = api._FEATURES["seq_prefix"]
    assert parent == "sequential" and set(needs) == set(binds)
    assert len(binds["gcre_score_sets_prefix_sequential"][1]) == 16 and len(binds["gcre_score_sets_dose_sequential"][1]) == 17
    header = open(os.path.join(ROOT, "include", "gcre_hip.h")).read()
    for sym in binds:
        assert sym + "(" in header
