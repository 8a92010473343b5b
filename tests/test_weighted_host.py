"""Covariate-adjusted permutation masks, host side: the thresholds of gcre_weighted_thresholds -- their sum
against the bound derived in csrc/gcre_weighted.h, monotone in the odds, unchanged by a power-of-two rescaling, the degenerate
strata, every refusal with its code and message; the header itself driven by tests/native/weighted_main.cpp under the address
and undefined-behaviour sanitizers as a child process, against ``report.weighted_masks``; the draw rule on a six-patient cohort
with the attempts written out by hand; the sampled law against the uniform law and against
``report.conditional_bernoulli_reference`` by chi-square; ``report.case_odds``; the interface.  No GPU needed."""
from __future__ import annotations

import ctypes
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from geneticscre_amd import api, report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "weighted_main.cpp")
OK, ERR_RANGE, ERR_ARG = 0, -2, -4   # include/gcre_hip.h
W = "weighted_thresholds: "
G = "generate_weighted_masks: "


def sum_bound(size: int) -> float:
    """weighted_sum_bound of csrc/gcre_weighted.h: |Z| (2^-32 + 2^-44) + |Z|^2 2^-52 -- the floor of every threshold, the
    last double of the bisection on log2 of the tilt, and the rounding of a plain sum of |Z| terms."""
    return size * (2.0**-32 + 2.0**-44) + size * size * 2.0**-52


def thresholds_call(n, n_cases, odds, stratum, n_strata, want_expected=True):
    """gcre_weighted_thresholds as C sees it: (code, message, thr, expected)."""
    lib = api._weighted_lib()
    w = None if odds is None else np.ascontiguousarray(odds, dtype=np.float64)
    st = None if stratum is None else np.ascontiguousarray(stratum, dtype=np.int32)
    thr = np.full(max(n, 1), 0xDEADBEEF, dtype=np.uint32)
    exp = np.full(max(n_strata, 1), -1.0)
    rc = lib.gcre_weighted_thresholds(n, n_cases, api._ptr(w), api._ptr(st), n_strata, api._ptr(thr), api._ptr(exp) if want_expected else None)
    return rc, (lib.gcre_last_error(None).decode() if rc else ""), thr[:n], exp


# ---- the thresholds ---------------------------------------------------------------------------------------------------------


def cohorts():
    rng = np.random.default_rng(23)
    yield "equal", np.ones(40), 15, None
    yield "log-uniform", 10.0 ** rng.uniform(-6, 6, 200), 80, None
    yield "three strata", np.exp(rng.normal(0, 2, 333)), 100, rng.integers(0, 3, 333)
    yield "one heavy patient", np.r_[1e12, np.ones(63)], 20, None
    yield "large", np.exp(rng.normal(0, 1, 5000)), 2500, rng.integers(0, 4, 5000)
    yield "sixteen strata", rng.uniform(0.5, 2, 400), 190, np.arange(400) % 16


@pytest.mark.parametrize("name,odds,n_cases,strata", list(cohorts()), ids=[c[0] for c in cohorts()])
def test_threshold_sums_stay_inside_the_bound(name, odds, n_cases, strata):
    n = len(odds)
    thr, exp = api.weighted_thresholds(odds, n_cases, n - n_cases, strata)
    st = np.zeros(n, int) if strata is None else np.asarray(strata)
    assert thr.dtype == np.uint32 and len(exp) == len(np.unique(st))
    for s in np.unique(st):
        z = st == s
        cases = int(z[:n_cases].sum())
        total = float((thr[z].astype(np.float64) / 2.0**32).sum())
        print(name, "stratum", s, "size", z.sum(), "cases", cases, "sum", total, "bound", sum_bound(int(z.sum())))
        assert abs(total - cases) < sum_bound(int(z.sum()))
        # the expected attempts are sqrt(2 pi V) of the thresholds as they are
        p = thr[z] / 2.0**32
        assert exp[list(np.unique(st)).index(s)] == pytest.approx(max(1.0, np.sqrt(2 * np.pi * (p * (1 - p)).sum())), rel=1e-12)
        # monotone in the odds
        order = np.argsort(odds[z], kind="stable")
        assert (np.diff(thr[z][order].astype(np.int64)) >= 0).all()
        assert (thr[z][odds[z] == odds[z].max()] == thr[z].max()).all()


def test_balanced_cohorts_expect_what_the_design_says():
    _, e = api.weighted_thresholds(np.ones(200), 100, 100)
    assert e[0] == pytest.approx(np.sqrt(2 * np.pi * 50), rel=1e-6) and 17 < e[0] < 18
    _, e = api.weighted_thresholds(np.ones(50000), 25000, 25000)
    assert 279 < e[0] < 281


def test_rescaling_a_stratums_odds_changes_nothing():
    """The odds of a stratum are divided by their maximum before the bisection, so a power of two -- exact in binary -- leaves
    every threshold as it was: well inside the bisection's stated tolerance."""
    rng = np.random.default_rng(4)
    odds = np.exp(rng.normal(0, 1.5, 120))
    strata = rng.integers(0, 3, 120)
    want, _ = api.weighted_thresholds(odds, 50, 70, strata)
    for scale in (2.0**20, 2.0**-20):
        for s in range(3):
            o = odds.copy()
            o[strata == s] *= scale
            got, _ = api.weighted_thresholds(o, 50, 70, strata)
            assert np.array_equal(got, want), (scale, s)
    # any other constant: the law is the same, the thresholds move by the rounding of one division at the most
    got, _ = api.weighted_thresholds(odds * 3.7, 50, 70, strata)
    assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 4


def test_degenerate_strata():
    # stratum 0: no case; stratum 1: all cases; stratum 2: as many cases as patients with positive odds; stratum 3: ordinary
    strata = np.array([1, 1, 2, 2, 3, 3, 0, 0, 0, 2, 3, 3])
    odds = np.array([5.0, 0.25, 1.0, 2.0, 1.0, 1.0, 3.0, 1.0, 0.0, 0.0, 1.0, 0.0])
    thr, exp = api.weighted_thresholds(odds, 6, 6, strata)
    assert thr[strata == 0].tolist() == [0, 0, 0]
    assert thr[strata == 1].tolist() == [2**32 - 1] * 2
    assert thr[strata == 2].tolist() == [2**32 - 1, 2**32 - 1, 0]
    assert thr[11] == 0 and abs(int(thr[4]) - (2**32 * 2) // 3) <= 2 and thr[4] == thr[5] == thr[10]
    assert exp[0] == 1.0 and exp[1] == 1.0 and exp[2] == 1.0 and exp[3] == pytest.approx(np.sqrt(2 * np.pi * 3 * 2 / 9), rel=1e-6)
    # a cohort without cases, and one without controls
    assert api.weighted_thresholds(np.ones(5), 0, 5)[0].tolist() == [0] * 5
    assert api.weighted_thresholds(np.ones(5), 5, 0)[0].tolist() == [2**32 - 1] * 5


BAD_ODDS = "the odds of patient {} (stratum {}) must be finite and >= 0, not {}"
REFUSALS = [
    ("NULL odds", (4, 2, None, None, 0), W + "NULL argument (odds)"),
    ("negative odds", (4, 2, [1, 1, -0.5, 1], None, 0), W + BAD_ODDS.format(2, 0, "-0.500000")),
    ("NaN odds", (4, 2, [1, np.nan, 1, 1], [0, 1, 0, 1], 2), W + BAD_ODDS.format(1, 1, "nan")),
    ("infinite odds", (4, 2, [1, 1, 1, np.inf], [0, 1, 0, 1], 2), W + BAD_ODDS.format(3, 1, "inf")),
    ("too few positive odds", (5, 3, [1, 0, 1, 0, 1], [0, 1, 1, 1, 0], 2),
     W + "stratum 1 has 1 patients with positive odds, fewer than its 2 cases"),
    ("an id above the range", (4, 2, [1, 1, 1, 1], [0, 1, 2, 1], 2), W + "stratum id 2 of patient 2 outside 0 .. 1"),
    ("a negative id", (4, 2, [1, 1, 1, 1], [0, -1, 0, 1], 2), W + "stratum id -1 of patient 1 outside 0 .. 1"),
    ("no strata", (4, 2, [1, 1, 1, 1], [0, 0, 0, 0], 0), W + "n_strata = 0 outside 1 .. GCRE_STRATA_MAX = 16"),
    ("seventeen strata", (4, 2, [1, 1, 1, 1], [0, 0, 0, 0], 17), W + "n_strata = 17 outside 1 .. GCRE_STRATA_MAX = 16"),
]


@pytest.mark.parametrize("name,args,message", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusals_of_the_library(name, args, message):
    rc, msg, thr, _ = thresholds_call(*args)
    assert rc == ERR_ARG and msg == message
    assert (thr == 0xDEADBEEF).all()                      # nothing written
    if "odds" in name and args[2] is not None:            # (the Python layer maps the ids itself: it cannot pass a bad one)
        with pytest.raises(api.GcreError, match=re.escape(message)):
            api.weighted_thresholds(args[2], args[1], args[0] - args[1], args[3])


def test_thresholds_without_the_optional_output():
    rc, _, thr, _ = thresholds_call(4, 2, [1, 1, 1, 1], None, 0, want_expected=False)
    assert rc == OK and len(set(thr.tolist())) == 1 and 2**31 - 2 <= thr[0] <= 2**31          # (the bisection ends below the root)
    lib = api._weighted_lib()
    assert lib.gcre_weighted_thresholds(4, 2, api._ptr(np.ones(4)), None, 0, None, None) == ERR_ARG
    assert lib.gcre_last_error(None).decode() == W + "NULL argument (thr_out)"


# ---- the C++ itself ---------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("weighted") / "weighted_main")
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


def hexes(odds):
    return [float(x).hex() if np.isfinite(x) else repr(float(x)) for x in odds]


def mask_words(masks):
    n = masks.shape[1]
    out = []
    for row in masks:
        out.append([int(sum(1 << (c - 32 * k) for c in np.flatnonzero(row) if c // 32 == k)) for k in range((n + 31) // 32)])
    return out


NATIVE = [
    ("one stratum", 7, 12, None, 3),
    ("three strata", 20, 51, 3, 9),
    ("sixteen strata", 60, 70, 16, 1),
    ("a stratum without a patient", 5, 6, 4, 2),
]


@pytest.mark.parametrize("name,n_cases,n_ctrls,ns,seed", NATIVE, ids=[c[0] for c in NATIVE])
def test_native_header_equals_the_library_and_numpy(prog, tmp_path, name, n_cases, n_ctrls, ns, seed):
    rng = np.random.default_rng(seed)
    n = n_cases + n_ctrls
    odds = np.exp(rng.uniform(-3, 3, n))
    odds[rng.integers(0, n)] = 0.0 if ns is None else odds[0]
    strata = None if ns is None else rng.integers(0, ns, n)
    if name == "a stratum without a patient":
        strata[strata == 2] = 3
    if ns == 16:
        strata[:16] = np.arange(16)
    perms = 12
    case = [("n_cases", n_cases), ("n_ctrls", n_ctrls), ("seed", seed), ("perms", perms), ("odds", hexes(odds))]
    if ns is not None:
        case += [("n_strata", ns), ("strata", strata.tolist())]
    out = run_case(prog, tmp_path, case)
    assert out[0] == "check 0 "
    rc, _, thr, exp = thresholds_call(n, n_cases, odds, strata, ns or 0)
    assert rc == OK
    assert out[1].split()[1:] == [str(v) for v in thr]
    assert [float(v) for v in out[2].split()[1:]] == exp[:ns or 1].tolist()
    sizes = [n] if ns is None else [int((strata == s).sum()) for s in range(ns)]
    assert [float(v) for v in out[3].split()[1:]] == [sum_bound(z) for z in sizes]
    # the draw: ids 0 .. ns-1 as they are (an absent id keeps its column of attempts, always 0)
    present = np.arange(1) if ns is None else np.unique(strata)
    masks, att = report.weighted_masks(thr, n_cases, n_ctrls, perms, seed, strata)
    full = np.zeros((perms, ns or 1), np.int64)
    full[:, present] = att
    words = mask_words(masks)
    gap = name == "a stratum without a patient"      # numpy numbers the strata it sees 0 .. S-1: ids behind the gap hash otherwise
    for r in range(perms):
        tok = out[4 + r].split()
        i = tok.index("mask")
        got = [int(v) for v in tok[3:i]]
        assert tok[:3] == ["perm", str(r), "att"] and len(got) == (ns or 1)
        if gap:
            assert got[:2] == full[r, :2].tolist() and got[2] == 0
            w = int(tok[i + 1])
            assert all(bin(w & sum(1 << int(c) for c in np.flatnonzero(strata == s))).count("1") == (strata[:n_cases] == s).sum() for s in range(ns))
        else:
            assert got == full[r].tolist() and [int(v) for v in tok[i + 1:]] == words[r]
    for s in present:
        z = np.ones(n, bool) if ns is None else strata == s
        assert (masks[:, z].sum(axis=1) == z[:n_cases].sum()).all()


def test_native_cap_and_messages(prog, tmp_path):
    base = [("n_cases", 3), ("n_ctrls", 3), ("seed", 12), ("perms", 2), ("odds", hexes([1 / 3, 1, 3, 1, 1, 1]))]
    out = run_case(prog, tmp_path, base + [("max_attempts", 0)])
    assert out == [f"check {ERR_ARG} {G}max_attempts = 0 must be at least 1"]
    out = run_case(prog, tmp_path, base + [("max_attempts", -7)])
    assert out == [f"check {ERR_ARG} {G}max_attempts = -7 must be at least 1"]
    # sqrt(2 pi V) of six patients is about 2.9: refused before anything is drawn
    out = run_case(prog, tmp_path, base + [("max_attempts", 2)])
    assert out == [f"check {ERR_RANGE} {G}stratum 0 needs about 3 attempts per permutation, above max_attempts = 2"]
    # the cap cuts the search: an odd cap ends on an even attempt
    full = run_case(prog, tmp_path, base)
    a0, a1 = int(full[4].split()[3]), int(full[5].split()[3])
    assert (a0, a1) == (5, 1)
    out = run_case(prog, tmp_path, base + [("max_attempts", 5), ("left", 1)])
    assert out[4] == f"perm 0 att {2**32 - 1} mask" and out[5] == full[5]
    assert out[6] == ("left " + G + "1 of 2 permutations were left over without an accepted attempt below max_attempts = 5: "
                      "the context's masks are unchanged")
    assert run_case(prog, tmp_path, base + [("max_attempts", 6)])[4:6] == full[4:6]
    out = run_case(prog, tmp_path, [("n_cases", 3), ("n_ctrls", 3), ("odds", hexes([1, -1, 1, 1, 1, 1]))])
    assert out == [f"check {ERR_ARG} {G}" + BAD_ODDS.format(1, 0, "-1.000000")]
    assert run_case(prog, tmp_path, [("n_cases", 3), ("n_ctrls", 3)]) == [f"check {ERR_ARG} {G}NULL argument (odds)"]


# ---- the draw rule by hand --------------------------------------------------------------------------------------------------

HAND_THR = [0x40000000, 0x80000000, 0xC0000000, 0x80000000, 0x80000000, 0x80000000]   # p = 1/4, 1/2, 3/4, 1/2, 1/2, 1/2
# seed 12, one stratum, three cases.  Per permutation: the hash key of every attempt pair, and per attempt the six 32-bit
# uniforms in column order -- the high halves of mix64(pair + c) for the even attempt, the low halves for the odd one.
HAND = {
    0: [(0xFF45454D64B09FE7, [0xF1E3B917, 0xA1A7A291, 0x2B7B431C, 0x7F9D50B6, 0x037ECCFC, 0x161B5748],    # a = 0: cases 2 3 4 5: four
                             [0x6F3C8BE2, 0x12962403, 0xDB805C3B, 0xD9751458, 0xDA37D827, 0x61200584]),   # a = 1: cases 1 5: two
        (0x01697F1E60F925E8, [0x1078784F, 0xCACE7DC9, 0x490AC358, 0x5AE635D8, 0x085BE8F5, 0x96FFB286],    # a = 2: cases 0 2 3 4: four
                             [0x5D7052B0, 0xE9AC46DF, 0x820EF90B, 0xDA1AF95F, 0xFEFD8413, 0x83D0FDD2]),   # a = 3: case 2: one
        (0x8DEEF38461DACB78, [0xA5963253, 0x76E27C28, 0xF9819719, 0x4F44A9F2, 0x6A600A4F, 0x50637630],    # a = 4: cases 1 3 4 5: four
                             [0x2D03A545, 0xAF9B0ACC, 0x45F0B1E2, 0x49D30A3C, 0x8282510C, 0x87954300])],  # a = 5: cases 0 2 3: ACCEPTED
    1: [(0xD6263ADD9FE2CC16, [0x17125F53, 0x2BD259AC, 0x51F358DF, 0x44235246, 0x871B6C6E, 0xFBA19DB4],    # a = 0: cases 0 1 2 3: four
                             [0x660D971F, 0xB22BCF60, 0x8009370C, 0x4B9DC50D, 0xD44249C0, 0x66AA4380])],  # a = 1: cases 2 3 5: ACCEPTED
}


def test_six_patients_by_hand():
    lib = api.load_library()
    mix = lambda z: int(lib.gcre_mix64(ctypes.c_uint64(z & (2**64 - 1))))
    seed1 = mix(12 ^ report.WEIGHTED_TAG)
    counts = {}
    for r, pairs in HAND.items():
        key = mix(seed1 ^ (0x51ED270B7F3C9A1D * (r + 1)))
        base = mix(key ^ 0xD1B54A32D192ED03)                  # stratum 0: the multiplier times 0 + 1
        for j, (pair, even, odd) in enumerate(pairs):
            assert mix(base + j) == pair
            for c in range(6):
                u = mix(pair + c)
                assert (u >> 32, u & 0xFFFFFFFF) == (even[c], odd[c])
            counts[r, 2 * j] = [c for c in range(6) if even[c] < HAND_THR[c]]
            counts[r, 2 * j + 1] = [c for c in range(6) if odd[c] < HAND_THR[c]]
    assert [counts[0, a] for a in range(6)] == [[2, 3, 4, 5], [1, 5], [0, 2, 3, 4], [2], [1, 3, 4, 5], [0, 2, 3]]
    assert [counts[1, a] for a in range(2)] == [[0, 1, 2, 3], [2, 3, 5]]
    masks, att = report.weighted_masks(HAND_THR, 3, 3, 2, 12)
    assert att.tolist() == [[5], [1]] and att.dtype == np.uint32
    assert [np.flatnonzero(m).tolist() for m in masks] == [[0, 2, 3], [2, 3, 5]]
    # the cap: attempt 5 is not below 5
    masks, att = report.weighted_masks(HAND_THR, 3, 3, 2, 12, max_attempts=5)
    assert att.tolist() == [[report.WEIGHTED_NONE], [1]] and not masks[0].any() and np.flatnonzero(masks[1]).tolist() == [2, 3, 5]
    # two strata {0, 2, 4} and {1, 3, 5} with ids 7 and 3: stratum 0 is id 3, every patient hashed under its own column
    masks, att = report.weighted_masks(HAND_THR, 3, 3, 50, 12, strata=[7, 3, 7, 3, 7, 3])
    assert (masks[:, [1, 3, 5]].sum(axis=1) == 1).all() and (masks[:, [0, 2, 4]].sum(axis=1) == 2).all()
    with pytest.raises(ValueError, match="thresholds: one per patient"):
        report.weighted_masks(HAND_THR[:5], 3, 3, 2, 12)


# ---- the law ---------------------------------------------------------------------------------------------------------------


def subset_counts(masks, subsets):
    code = (masks * (1 << np.arange(masks.shape[1]))).sum(axis=1)
    return np.array([(code == sum(1 << c for c in a)).sum() for a in subsets])


def test_equal_odds_give_the_uniform_law():
    """Seed 1, 20,000 masks of three cases among six patients: the 20 subsets against 1,000 each.  Chi-square with 19 degrees
    of freedom; the bound is its 99.9 % point, 43.82.  The numpy definition gives 20.378."""
    thr, _ = api.weighted_thresholds(np.ones(6), 3, 3)
    assert len(set(thr.tolist())) == 1 and 2**31 - 2 <= thr[0] <= 2**31
    masks, _ = report.weighted_masks(thr, 3, 3, 20000, 1)
    subsets = list(itertools.combinations(range(6), 3))
    obs = subset_counts(masks, subsets)
    chi = float(((obs - 1000.0) ** 2 / 1000.0).sum())
    print("chi-square", chi)
    assert obs.sum() == 20000 and chi < 43.82
    assert chi == pytest.approx(20.378, abs=1e-9)


def test_unequal_odds_give_the_conditional_bernoulli_law():
    """Seed 1, 20,000 masks of three cases among eight patients with odds 1, 2, 3, 4, 1.5, 2.5, 0.5, 6: the 56 subsets against
    ``conditional_bernoulli_reference`` on p = thr / 2^32 (the smallest expectation is 19.2).  Chi-square with 55 degrees of
    freedom; the bound is its 99.9 % point, 93.17.  The numpy definition gives 58.087."""
    odds = np.array([1, 2, 3, 4, 1.5, 2.5, 0.5, 6.0])
    thr, _ = api.weighted_thresholds(odds, 3, 5)
    incl, subsets, pr = report.conditional_bernoulli_reference(thr / 2.0**32, 3, subsets=True)
    assert len(subsets) == 56 and pr.sum() == pytest.approx(1.0, abs=1e-12) and incl.sum() == pytest.approx(3.0, abs=1e-12)
    # the thresholds keep the law of the odds: subset probabilities proportional to the product of the odds
    want = np.array([np.prod(odds[list(a)]) for a in subsets])
    assert np.allclose(pr, want / want.sum(), rtol=0, atol=1e-8)
    masks, _ = report.weighted_masks(thr, 3, 5, 20000, 1)
    obs = subset_counts(masks, subsets)
    ex = pr * 20000
    chi = float(((obs - ex) ** 2 / ex).sum())
    print("chi-square", chi, "smallest expectation", ex.min())
    assert obs.sum() == 20000 and ex.min() > 5 and chi < 93.17
    assert chi == pytest.approx(58.087, abs=1e-3)
    # inclusion frequencies: 20,000 draws, standard error below 0.0036
    assert np.abs(masks.mean(axis=0) - incl).max() < 4 * 0.0036


def test_conditional_bernoulli_reference_by_enumeration():
    p = np.array([0.1, 0.5, 0.7, 0.25, 0.0])
    incl, subsets, pr = report.conditional_bernoulli_reference(p, 2, subsets=True)
    w = p / (1 - p)
    want = np.array([w[a] * w[b] for a, b in subsets])
    want /= want.sum()
    assert np.allclose(pr, want, rtol=1e-14, atol=0)
    assert np.allclose(incl, [sum(q for s, q in zip(subsets, want) if c in s) for c in range(5)], rtol=1e-13, atol=0)
    assert incl[4] == 0.0
    assert report.conditional_bernoulli_reference(p, 0).tolist() == [0.0] * 5
    with pytest.raises(ValueError):
        report.conditional_bernoulli_reference([0.5, 1.0], 1)
    with pytest.raises(ValueError):
        report.conditional_bernoulli_reference([0.5, 0.0], 2)


# ---- case_odds -------------------------------------------------------------------------------------------------------------


def test_case_odds():
    # one binary covariate: the saturated model reproduces the cell frequencies -- 3 cases : 2 controls with x = 1, 2 : 5 with x = 0
    x = np.array([1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    o = report.case_odds(x, 5, 7)
    assert np.abs(o - np.where(x == 1, 3 / 2, 2 / 5)).max() < 1e-10
    assert np.abs(report.case_odds(x[:, None] * 40.0 - 3, 5, 7) - o).max() < 1e-10        # (any scale and shift of it)
    # nothing to fit: equal odds, cases : controls
    assert np.abs(report.case_odds(np.zeros(12), 5, 7) - 5 / 7).max() < 1e-12
    assert np.abs(report.case_odds(np.zeros((12, 3)), 5, 7) - 5 / 7).max() < 1e-12
    # separation raises; so does a wrong shape
    with pytest.raises(ValueError, match="separate cases from controls"):
        report.case_odds(np.r_[np.ones(5), np.zeros(7)], 5, 7)
    with pytest.raises(ValueError, match="separate cases from controls"):
        report.case_odds(np.arange(12.0), 5, 7)
    with pytest.raises(ValueError, match="one row per patient"):
        report.case_odds(np.zeros(11), 5, 7)
    # a ridge penalty shrinks the slope: the odds move towards cases : controls
    r = report.case_odds(x, 5, 7, ridge=5.0)
    assert (np.abs(r - 5 / 7) < np.abs(o - 5 / 7)).all()
    # the fitted odds are what the thresholds take: their tilted probabilities sum to the cases
    rng = np.random.default_rng(8)
    cov = rng.normal(size=(300, 2))
    lab = np.argsort(-(cov[:, 0] * 0.8 + rng.logistic(size=300)))                          # cases first
    o = report.case_odds(cov[lab], 120, 180)
    assert o.shape == (300,) and (o > 0).all() and np.isfinite(o).all()
    assert (o / (1 + o)).sum() == pytest.approx(120, abs=1e-6)                             # the score equation of the intercept
    thr, _ = api.weighted_thresholds(o, 120, 180)
    assert np.abs(thr / 2.0**32 - o / (1 + o)).max() < 1e-6                                # so the tilt is 1


# ---- the interface ---------------------------------------------------------------------------------------------------------


def test_interface_is_declared():
    header = open(os.path.join(ROOT, "include", "gcre_hip.h")).read()
    assert re.search(r"#define GCRE_ABI_VERSION 4\b", header)      # additions only
    flat = " ".join(re.sub(r"/\*.*?\*/", " ", header, flags=re.S).split())
    assert ("int gcre_generate_weighted_masks(gcre_ctx* ctx, uint64_t seed, const double* odds, const int32_t* stratum, int32_t n_strata, "
            "int64_t max_attempts, uint32_t* attempts_out );") in flat
    assert ("int gcre_weighted_thresholds(int32_t n, int32_t n_cases, const double* odds, const int32_t* stratum, int32_t n_strata, "
            "uint32_t* thr_out, double* expected_attempts_out );") in flat
    assert "int64_t gcre_weighted_launches(const gcre_ctx* ctx);" in flat
    names = {"gcre_generate_weighted_masks", "gcre_weighted_thresholds", "gcre_weighted_launches"}
    assert names <= set(api.EXPORTS)
    assert set(re.findall(r"\b(gcre_[a-z0-9_]+)\s*\(", header)) == set(api.EXPORTS)
    parent, needs, _, binds = api._FEATURES["weighted"]
    assert parent is None and set(needs) == set(binds) == names
    from geneticscre_amd import build
    assert {"gcre_weighted.hip", "gcre_host_weighted.hip"} <= set(build.SOURCES) and "gcre_weighted.h" in build.HEADERS
    kernels = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_kernels.h")).read()
    assert "struct WeightedArgs" in kernels and "launch_weighted_search(" in kernels and "launch_weighted_write(" in kernels
    lib = api._weighted_lib()                                 # loads without a GPU
    assert lib.gcre_abi_version() == 4 and lib.gcre_weighted_launches(None) == -1
    # the tag of the stream is its own, and Python's is the header's
    wh = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_weighted.h")).read()
    assert f"kWeightedTag = {report.WEIGHTED_TAG:#018x}ull" in wh and report.WEIGHTED_TAG == int.from_bytes(b"weighted", "big")
    assert f"{report.WEIGHTED_TAG:#018x}" not in kernels
    # gcre_host_stats.hip did not grow by it
    assert "weighted" not in open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_host_stats.hip")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.23" in design and "k_weighted_search" in design and "k_weighted_write" in design and "Not built" in design


def test_signatures():
    g = inspect.signature(api.JoinExec.generate_weighted_permutations).parameters
    assert list(g) == ["self", "seed", "odds", "strata", "max_attempts", "attempts"]
    assert [g[k].default for k in list(g)[3:]] == [None, 1 << 20, False]
    assert list(inspect.signature(api.weighted_thresholds).parameters) == ["odds", "n_cases", "n_ctrls", "strata"]
    w = inspect.signature(report.weighted_masks).parameters
    assert list(w) == ["thresholds", "n_cases", "n_ctrls", "perms", "seed", "strata", "max_attempts"]
    assert list(inspect.signature(report.conditional_bernoulli_reference).parameters)[:2] == ["p", "m"]
    c = inspect.signature(report.case_odds).parameters
    assert list(c)[:4] == ["covariates", "n_cases", "n_ctrls", "ridge"] and c["ridge"].default == 0.0
    for fn in (report.gwaspa, report.score_paths):
        assert inspect.signature(fn).parameters["case_odds"].default is None
        doc = " ".join(fn.__doc__.split())
        assert "only as good as the fitted model" in doc and "on the null, not on" in doc


def test_value_errors_come_before_the_library(monkeypatch):
    ex = api.JoinExec.__new__(api.JoinExec)
    ex.num_cases, ex.num_ctrls, ex.iters = 3, 2, 4
    monkeypatch.setattr(api, "_weighted_lib", lambda: None)
    with pytest.raises(ValueError, match=r"odds: one value per patient \(5\), not 4"):
        api.JoinExec.generate_weighted_permutations(ex, 1, np.ones(4))
    with pytest.raises(ValueError, match=r"strata: one id per patient \(5\), not 3"):
        api.JoinExec.generate_weighted_permutations(ex, 1, np.ones(5), strata=[0, 1, 0])
    rows = np.zeros((1, 5), np.int8)
    with pytest.raises(ValueError, match="case_odds: sequential p-values draw their own uniform masks"):
        report.score_paths(["A"], ["A"], rows, 3, 2, case_odds=np.ones(5), sequential=100)
    with pytest.raises(ValueError, match="gwaspa_out was drawn under different case_odds"):
        report.score_paths(["A"], ["A"], rows, 3, 2, case_odds=np.ones(5), gwaspa_out={"levels": {}})
    with pytest.raises(ValueError, match="gwaspa_out was drawn under different case_odds"):
        report.score_paths(["A"], ["A"], rows, 3, 2, gwaspa_out={"levels": {}, "case_odds_digest": report._odds_digest(np.ones(5))})
    with pytest.raises(ValueError, match="gwaspa_out was drawn under different case_odds"):
        report.score_paths(["A"], ["A"], rows, 3, 2, case_odds=np.ones(5) * 2,
                           gwaspa_out={"levels": {}, "case_odds_digest": report._odds_digest(np.ones(5))})
    with pytest.raises(ValueError, match="case_odds: decorated_pvalues and clump_conditional draw uniform nulls"):
        report.gwaspa(["A"], rows, 3, 2, None, case_odds=np.ones(5), decorated_pvalues=True)
