"""Split-half stability, host side: the draw rule ``report.subsample_masks`` on a hand-worked mask, its bit
counts per label, its dependence on (seed, b, c) only and its uniformity; the same rule, the argument checks and the slab
sizing in C++ (csrc/gcre_subsample.h), driven by tests/native/subsample_main.cpp under the address and undefined-behaviour
sanitizers as a child process; ``subsample_reference`` against the definition taken literally; ``stability_columns`` and
``stability_bound`` on written-out examples; the interface.  No GPU needed."""
from __future__ import annotations

import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from geneticscre_amd import api, report
from helpers import small_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "subsample_main.cpp")
OK, ERR_ARG = 0, -4   # include/gcre_hip.h
M64 = (1 << 64) - 1


def mix(z):
    """splitmix64's finaliser on Python integers."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


# ---- the draw rule ---------------------------------------------------------------------------------------------------


def test_mask_hand_worked():
    """Three cases, three controls, two cases and one control to take; seed 5, draw 1.  Cases 0 and 1 are taken, which leaves
    case 2 nothing; controls 3 and 4 miss their one chance in three and one in two, so control 5 must be taken."""
    seed, b = 5, 1
    seed1 = mix(seed ^ 0x73756273616D706C)
    base = mix(seed1 ^ ((0x51ED270B7F3C9A1D * (b + 1)) & M64))
    assert (seed1, base) == (0x08D66FFF1EE976FE, 0x96352486FFF05F4A)
    # patient c -> u = mix(base + c), the patients left in its stratum, those still to take, floor(u rem / 2^64), taken
    steps = [(0, 0x940AD8B9A4D31D32, 3, 2, 1, True),      # 0.578 * 3 -> 1 < 2
             (1, 0x6249EF5E14F591E4, 2, 1, 0, True),      # 0.384 * 2 -> 0 < 1
             (2, 0xBA452B2FBC2C06C7, 1, 0, 0, False),     # nothing left to take
             (3, 0x82759E9D46C8583E, 3, 1, 1, False),     # 0.510 * 3 -> 1
             (4, 0xDD0A9F45B0664504, 2, 1, 1, False),     # 0.863 * 2 -> 1
             (5, 0x0C6420D859CC11AF, 1, 1, 0, True)]      # the last of its stratum with one to take
    for c, u, rem, need, pick, take in steps:
        assert mix((base + c) & M64) == u
        assert (u * rem) >> 64 == pick and (pick < need) == take
        assert int(report._mix64(np.uint64((base + c) & M64))) == u and int(report._mulhi(np.uint64(u), rem)) == pick
    assert report.subsample_masks(3, 3, 2, 1, [1], seed).astype(int).tolist() == [[1, 1, 0, 0, 0, 1]]
    assert report.subsample_masks(3, 3, 2, 1, 2, seed).astype(int).tolist() == [[1, 0, 1, 0, 0, 1], [1, 1, 0, 0, 0, 1]]
    assert report.SUBSAMPLE_SEED_TAG == 0x73756273616D706C == int.from_bytes(b"subsampl", "big")


@pytest.mark.parametrize("shape", [(1, 1, 0, 1), (7, 5, 3, 2), (31, 2, 15, 1), (33, 31, 33, 0), (64, 1, 0, 0), (65, 135, 32, 67),
                                   (40, 60, 40, 60)])
def test_exact_bit_counts_per_label(shape):
    nc, nt, ma, mt = shape
    mk = report.subsample_masks(nc, nt, ma, mt, 300, 11)
    assert mk.shape == (300, nc + nt) and mk.dtype == bool
    assert (mk[:, :nc].sum(axis=1) == ma).all() and (mk[:, nc:].sum(axis=1) == mt).all()
    if 0 < ma < nc or 0 < mt < nt:
        assert len({r.tobytes() for r in mk}) > 1


def test_draws_depend_on_seed_draw_and_patient_only():
    full = report.subsample_masks(20, 30, 10, 15, 50, 3)
    assert np.array_equal(report.subsample_masks(20, 30, 10, 15, [49, 7, 7], 3), full[[49, 7, 7]])
    assert not np.array_equal(report.subsample_masks(20, 30, 10, 15, 50, 4), full)
    assert not np.array_equal(full[0], full[1])
    # the stream of a patient does not depend on the needs: with everything to take in neither stratum the first patient
    # whose number falls under need / rem is the same whatever the other stratum asks for
    a = report.subsample_masks(20, 30, 10, 15, 50, 3)[:, :20]
    b = report.subsample_masks(20, 30, 10, 0, 50, 3)[:, :20]
    assert np.array_equal(a, b)                               # the cases do not see the controls' needs
    # ... and the draws share nothing with the permutation masks of the same seed: another tag
    assert report.SUBSAMPLE_SEED_TAG != report.DECORATED_SEED_TAG
    with pytest.raises(ValueError, match="outside"):
        report.subsample_masks(3, 3, 4, 0, 1, 0)


CHI2_999_DF11 = 31.264      # the 0.999 quantile of the chi-square distribution with 11 degrees of freedom (12 cells)
CHI2_999_DF9 = 27.877       # ... with 9 (10 cells)


def test_which_patient_is_taken_is_uniform():
    """One case of 12 and one control of 10 per draw: every case, and every control, is the one taken equally often."""
    B = 24000
    mk = report.subsample_masks(12, 10, 1, 1, B, 2024)

    def chi_square(counts):
        e = counts.sum() / len(counts)
        return float(((counts - e) ** 2 / e).sum())

    cases, ctrls = mk[:, :12].sum(axis=0), mk[:, 12:].sum(axis=0)
    assert cases.sum() == B and ctrls.sum() == B
    x_cases, x_ctrls = chi_square(cases), chi_square(ctrls)
    print("chi-square over the 12 cases:", round(x_cases, 2), "over the 10 controls:", round(x_ctrls, 2))
    assert x_cases < CHI2_999_DF11, x_cases
    assert x_ctrls < CHI2_999_DF9, x_ctrls


# ---- the C++ itself --------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("subsample") / "subsample_main")
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


def test_native_masks_equal_the_python_rule(prog, tmp_path):
    rng = np.random.default_rng(23)
    shapes = [(3, 3, 2, 1), (1, 1, 0, 1), (31, 2, 15, 1), (32, 32, 16, 16), (33, 31, 33, 31), (64, 1, 0, 0), (65, 135, 32, 67)]
    for _ in range(4):
        nc, nt = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        shapes.append((nc, nt, int(rng.integers(0, nc + 1)), int(rng.integers(0, nt + 1))))
    for nc, nt, ma, mt in shapes:
        seed = int(rng.integers(0, 2**64, dtype=np.uint64))
        ask = [0, 1, 5, 511, 512, 1000003]
        out = run_case(prog, tmp_path, [("n_cases", nc), ("n_ctrls", nt), ("m_cases", ma), ("m_ctrls", mt), ("draws", 10), ("seed", seed),
                                        ("n_sets", 0)] + [("mask", b) for b in ask])
        assert out[0] == "check 0 ", out[0]
        want = report.subsample_masks(nc, nt, ma, mt, ask, seed)
        assert out[1:] == [f"mask {b} " + "".join("1" if x else "0" for x in row) for b, row in zip(ask, want)], (nc, nt, ma, mt)


def test_native_mix64_is_the_library_s(prog, tmp_path):
    zs = [0, 1, 2**63, M64, 0x9E3779B97F4A7C15, 123456789]
    out = run_case(prog, tmp_path, [("n_sets", 0)] + [("mix", z) for z in zs])
    lib = api.load_library()
    assert out[1:] == [f"mix {z} {mix(z)}" for z in zs]
    assert [int(lib.gcre_mix64(z)) for z in zs] == [mix(z) for z in zs]


def test_native_slab_sizing(prog, tmp_path, monkeypatch):
    monkeypatch.delenv("GCRE_SUBSAMPLE_SLAB_DRAWS", raising=False)
    # draws, mask dwords per draw, optional-output bytes per draw, the bound in MB -> draws per slab (whole 512-draw tiles)
    asks = [((1, 4, 0, 1024), 512), ((512, 4, 0, 1024), 512), ((513, 4, 0, 1024), 1024), ((100000, 1564, 0, 1024), 100352),
            ((100000, 1564, 2 * 8 * 1100, 1024), 44544),        # 512 x (6,256 + 17,600) bytes a tile: 87 tiles
            ((5000, 4, 0, 0), 512),                             # one tile at the least
            ((5000, 4, 16, 512 * 32 * 3 / 2**20), 1536)]        # 32 bytes a draw: exactly three tiles
    out = run_case(prog, tmp_path, [("n_sets", 0)] + [("slab", a) for a, _ in asks])
    assert out[1:] == [f"slab {w}" for _, w in asks]
    monkeypatch.setenv("GCRE_SUBSAMPLE_SLAB_DRAWS", "1300")      # rounded down to whole tiles, one at the least
    out = run_case(prog, tmp_path, [("n_sets", 0), ("slab", (5000, 4, 0, 1024)), ("slab", (600, 4, 0, 1024))])
    assert out[1:] == ["slab 1024", "slab 1024"]
    monkeypatch.setenv("GCRE_SUBSAMPLE_SLAB_DRAWS", "1")
    assert run_case(prog, tmp_path, [("n_sets", 0), ("slab", (5000, 4, 0, 1024))])[1:] == ["slab 512"]


COHORT = [("n_cases", 5), ("n_ctrls", 7), ("m_cases", 2), ("m_ctrls", 3), ("n_sets", 2)]
TABLES = [("table_a", (1, 3, 4)), ("table_b", (1, 4, 5))]
CUTS = [("n_cut", 2), ("cut", [1.5, 2.5, "-inf", "inf"]), ("have_n_b", 1), ("have_n_both", 1)]
W = "score_sets_subsample: "


def without(case, *keys):
    return [kv for kv in case if kv[0] not in keys]


CHECK_CASES = [
    ("accepted", COHORT + TABLES + CUTS + [("draws", 5)], OK, ""),
    ("no draws", COHORT + TABLES + CUTS + [("draws", 0)], OK, ""),
    ("half A only", COHORT + TABLES[:1] + [("n_cut", 1), ("cut", [0.0, 1.0]), ("draws", 5)], OK, ""),
    ("no cuts, matrices only", COHORT + TABLES + [("draws", 5), ("want_a", 1), ("want_b", 1), ("have_n_a", 0)], OK, ""),
    ("nothing taken", without(COHORT, "m_cases", "m_ctrls") + [("m_cases", 0), ("m_ctrls", 0)] + TABLES + CUTS + [("draws", 5)], OK, ""),
    ("everything taken", without(COHORT, "m_cases", "m_ctrls") + [("m_cases", 5), ("m_ctrls", 7)] + TABLES + CUTS + [("draws", 5)], OK, ""),
    ("eight cuts", COHORT + TABLES + [("n_cut", 8), ("cut", list(range(16))), ("draws", 5)], OK, ""),
    ("negative draws", COHORT + TABLES + CUTS + [("draws", -1)], ERR_ARG, W + "draws must not be negative, not -1"),
    ("m_cases above", without(COHORT, "m_cases") + [("m_cases", 6)] + TABLES + [("draws", 5)], ERR_ARG, W + "m_cases = 6 outside 0 .. n_cases = 5"),
    ("m_cases below", without(COHORT, "m_cases") + [("m_cases", -1)] + TABLES + [("draws", 5)], ERR_ARG, W + "m_cases = -1 outside 0 .. n_cases = 5"),
    ("m_ctrls above", without(COHORT, "m_ctrls") + [("m_ctrls", 8)] + TABLES + [("draws", 5)], ERR_ARG, W + "m_ctrls = 8 outside 0 .. n_ctrls = 7"),
    ("m_ctrls below", without(COHORT, "m_ctrls") + [("m_ctrls", -2)] + TABLES + [("draws", 5)], ERR_ARG, W + "m_ctrls = -2 outside 0 .. n_ctrls = 7"),
    ("NULL table_a", COHORT + [("table_a", (0, 3, 4))] + [("draws", 5)], ERR_ARG, W + "NULL argument (table_a)"),
    ("table_a without rows", COHORT + [("table_a", (1, 0, 4))] + [("draws", 5)], ERR_ARG,
     W + "table_a must have at least one row and one column, not 0 x 4"),
    ("table_a without columns", COHORT + [("table_a", (1, 3, 0))] + [("draws", 5)], ERR_ARG,
     W + "table_a must have at least one row and one column, not 3 x 0"),
    ("table_b without rows", COHORT + [("table_a", (1, 3, 4)), ("table_b", (1, -1, 5))] + [("draws", 5)], ERR_ARG,
     W + "table_b must have at least one row and one column, not -1 x 5"),
    ("negative n_cut", COHORT + TABLES + [("n_cut", -1), ("draws", 5)], ERR_ARG, W + "n_cut = -1 outside 0 .. GCRE_SUBSAMPLE_MAX_CUTS = 8"),
    ("nine cuts", COHORT + TABLES + [("n_cut", 9), ("cut", list(range(18))), ("draws", 5)], ERR_ARG,
     W + "n_cut = 9 outside 0 .. GCRE_SUBSAMPLE_MAX_CUTS = 8"),
    ("NULL cut", COHORT + TABLES + [("n_cut", 2), ("draws", 5)], ERR_ARG, W + "NULL argument (cut) with n_cut = 2"),
    ("NULL n_a", COHORT + TABLES + CUTS + [("have_n_a", 0), ("draws", 5)], ERR_ARG, W + "NULL argument (n_a) with n_cut = 2"),
    ("n_b without table_b", COHORT + TABLES[:1] + [("n_cut", 1), ("cut", [0.0, 1.0]), ("have_n_b", 1), ("draws", 5)], ERR_ARG,
     W + "n_b without table_b: half B is not scored"),
    ("n_both without table_b", COHORT + TABLES[:1] + [("n_cut", 1), ("cut", [0.0, 1.0]), ("have_n_both", 1), ("draws", 5)], ERR_ARG,
     W + "n_both without table_b: half B is not scored"),
    ("scores_b without table_b", COHORT + TABLES[:1] + [("want_b", 1), ("draws", 5)], ERR_ARG, W + "scores_b without table_b: half B is not scored"),
    ("NaN cut", COHORT + TABLES + [("n_cut", 2), ("cut", [1.5, 2.5, 0.5, "nan"]), ("draws", 5)], ERR_ARG, W + "cut[1][1] is NaN"),
    ("matrices above the bound", COHORT + TABLES + [("draws", 5), ("want_a", 1), ("want_b", 1), ("max_mb", 0.015)], ERR_ARG,
     W + "the optional outputs of one tile of 512 draws take 16384 bytes: above GCRE_SUBSAMPLE_MAX_MB = 0.015000"),
    ("one matrix fits it", COHORT + TABLES + [("draws", 5), ("want_a", 1), ("max_mb", 0.015)], OK, ""),
    ("the bound is not asked without matrices", COHORT + TABLES + CUTS + [("draws", 5), ("max_mb", 0)], OK, ""),
    ("nor without draws", COHORT + TABLES + [("draws", 0), ("want_a", 1), ("want_b", 1), ("max_mb", 0)], OK, ""),
]


@pytest.mark.parametrize("name,case,code,message", CHECK_CASES, ids=[c[0] for c in CHECK_CASES])
def test_argument_checks_under_sanitizers(prog, tmp_path, name, case, code, message):
    assert run_case(prog, tmp_path, case) == [f"check {code} {message}"]


# ---- the definition --------------------------------------------------------------------------------------------------


def literal(sets, rows, signs, n_cases, m_cases, m_ctrls, draws, seed, TA, TB, cuts, method):
    """gcre_score_sets_subsample taken literally on unpacked 0/1 arrays: one draw and one patient at a time, Python sets."""
    rows = np.asarray(rows) != 0
    n = rows.shape[1]
    n_ctrls = n - n_cases
    masks = []
    seed1 = mix(seed ^ 0x73756273616D706C)
    for b in range(draws):
        base = mix(seed1 ^ ((0x51ED270B7F3C9A1D * (b + 1)) & M64))
        rem, need, S = [n_cases, n_ctrls], [m_cases, m_ctrls], set()
        for c in range(n):
            k = 0 if c < n_cases else 1
            if (mix((base + c) & M64) * rem[k]) >> 64 < need[k]:
                S.add(c)
                need[k] -= 1
            rem[k] -= 1
        masks.append(S)

    def cell(VT, a, b):
        return float(VT[a][b]) if a < VT.shape[0] and b < VT.shape[1] else -1.0       # (the device's padding)

    def score(P, N, keep, VT):
        P, N = P & keep, N & keep
        v = cell(VT, sum(q < n_cases for q in P), sum(q >= n_cases for q in P))
        if method == 2:
            v = v + cell(VT, sum(q >= n_cases for q in N), sum(q < n_cases for q in N))
        return v

    everyone = set(range(n))
    out = {"n_a": [], "n_b": [], "n_both": [], "scores_a": [], "scores_b": []}
    for s, m in enumerate(sets):
        J = len(cuts[s])
        if any(r < 0 for r in m):
            for k in ("n_a", "n_b", "n_both"):
                out[k].append([-1] * J)
            out["scores_a"].append([float("nan")] * draws)
            out["scores_b"].append([float("nan")] * draws)
            continue
        sg = [1] * len(m) if signs is None else signs[s]
        P, N = set(), set()
        for r, g in zip(m, sg):
            (N if method == 2 and g == -1 else P).update(np.flatnonzero(rows[r]).tolist())
        A = [score(P, N, S, TA) for S in masks]
        Bs = [score(P, N, everyone - S, TB) for S in masks]
        out["scores_a"].append(A)
        out["scores_b"].append(Bs)
        out["n_a"].append([sum(a >= c for a in A) for c in cuts[s]])
        out["n_b"].append([sum(b >= c for b in Bs) for c in cuts[s]])
        out["n_both"].append([sum(a >= c and b >= c for a, b in zip(A, Bs)) for c in cuts[s]])
    return out


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("method", [1, 2])
def test_reference_equals_the_definition(method):
    rng = np.random.default_rng(60 + method)
    n_cases, n_ctrls = 9, 12
    for trial in range(4):
        ma, mt = [(4, 6), (0, 0), (9, 12), (1, 12)][trial]
        TA, TB = small_table(ma, mt, 1 + trial), small_table(n_cases - ma, n_ctrls - mt, 7 + trial)
        if trial == 0:
            TA[1, 2] = np.nan
            TB = TB[:3, :4]                                   # smaller than the half cohort: cells read as -1
        n_rows = int(rng.integers(6, 20))
        rows = rng.random((n_rows, n_cases + n_ctrls)) < 0.2
        sets = [rng.integers(0, n_rows, int(rng.integers(1, 5))).tolist() for _ in range(5)] + [[0, -1]]
        signs = [rng.choice([1, -1], len(x)).tolist() for x in sets] if trial != 1 else None
        cuts = np.sort(rng.random((len(sets), 3)) * 20, axis=1)
        cuts[0] = [-np.inf, 5.0, np.inf]
        got = report.subsample_reference(sets, rows, signs, n_cases, ma, mt, 30, 99, TA, TB, cuts, method)
        want = literal(sets, rows, signs, n_cases, ma, mt, 30, 99, TA, TB, cuts.tolist(), method)
        for k in ("n_a", "n_b", "n_both"):
            assert got[k].tolist() == want[k], (trial, k)
        for k in ("scores_a", "scores_b"):
            assert np.array_equal(bits(got[k]), bits(want[k])), (trial, k)
        assert got["n_a"][0, 0] == 30 or np.isnan(got["scores_a"][0]).any()
        half = report.subsample_reference(sets, rows, signs, n_cases, ma, mt, 30, 99, TA, False, cuts, method)
        assert half["n_b"] is None and half["n_both"] is None and half["scores_b"] is None
        assert np.array_equal(half["n_a"], got["n_a"]) and np.array_equal(bits(half["scores_a"]), bits(got["scores_a"]))
    one = report.subsample_reference([[0, 1]], rows, None, n_cases, 4, 6, 0, 1, TA, TB, [1.0], method)
    assert one["n_a"].tolist() == [[0]] and one["scores_a"].shape == (1, 0)
    none = report.subsample_reference([[0, 1]], rows, None, n_cases, 4, 6, 3, 1, TA, TB, None, method)
    assert none["n_a"].shape == (1, 0) and none["scores_b"].shape == (1, 3)


def test_stability_columns_written_out():
    counts = {"n_a": [[10], [0], [-1], [4]], "n_b": [[8], [2], [-1], [4]], "n_both": [[5], [0], [-1], [1]]}
    cols, per_half = report.stability_columns(counts, [1, 1, 0, 1], 20)
    assert list(cols) == report.STABILITY_COLUMNS == ["StabilityA", "StabilityB", "StabilityBoth", "HalfReplication"]
    assert cols["StabilityA"][[0, 1, 3]].tolist() == [0.5, 0.0, 0.2] and np.isnan(cols["StabilityA"][2])
    assert cols["StabilityB"][[0, 1, 3]].tolist() == [0.4, 0.1, 0.2]
    assert cols["StabilityBoth"][[0, 1, 3]].tolist() == [0.25, 0.0, 0.05]
    assert cols["HalfReplication"][[0, 3]].tolist() == [0.5, 0.25] and np.isnan(cols["HalfReplication"][[1, 2]]).all()   # 0 / 0; NA
    assert per_half.tolist() == [(10 + 0 + 4) / 20]
    # two cuts: suffixed, cut-major; a valid flag that is off hides a row whatever its counts
    two = {"n_a": [[6, 2], [3, 0]], "n_b": [[6, 1], [3, 3]], "n_both": [[3, 1], [3, 0]]}
    cols, per_half = report.stability_columns(two, [1, 0], 6)
    assert list(cols) == [f"{n}.{j}" for j in (0, 1) for n in report.STABILITY_COLUMNS]
    assert cols["StabilityA.0"][0] == 1.0 and cols["StabilityA.1"][0] == 2 / 6 and cols["HalfReplication.1"][0] == 0.5
    assert all(np.isnan(v[1]) for v in cols.values())
    assert per_half.tolist() == [1.0, 2 / 6]
    # half A only; no draws
    cols, per_half = report.stability_columns({"n_a": [[3]], "n_b": None, "n_both": None}, [1], 4)
    assert cols["StabilityA"].tolist() == [0.75] and all(np.isnan(cols[k]).all() for k in report.STABILITY_COLUMNS[1:])
    cols, per_half = report.stability_columns({"n_a": [[0]], "n_b": [[0]], "n_both": [[0]]}, [1], 0)
    assert all(np.isnan(v).all() for v in cols.values()) and np.isnan(per_half).all()


def test_stability_bound_written_out():
    assert report.stability_bound(3, 100, 0.9) == 9 / (0.8 * 100)
    assert report.stability_bound(2.5, 10, 0.75) == 6.25 / (0.5 * 10)
    assert report.stability_bound(0, 10, 0.6) == 0.0
    for tau in (0.5, 0.2):
        with pytest.raises(ValueError, match="above 1/2"):
            report.stability_bound(3, 100, tau)
    with pytest.raises(ValueError, match="n_sets"):
        report.stability_bound(3, 0, 0.9)
    doc = " ".join(report.stability_bound.__doc__.split())
    assert "exchangeable" in doc and "Overlapping paths through one gene do not meet this" in doc and "indicative" in doc


# ---- the interface ---------------------------------------------------------------------------------------------------


def test_interface_is_declared():
    header = open(os.path.join(ROOT, "include", "gcre_hip.h")).read()
    assert re.search(r"#define GCRE_ABI_VERSION 4\b", header)      # additions only
    flat = " ".join(header.split())
    assert ("int gcre_score_sets_subsample(gcre_ctx* ctx, const gcre_set_input* in, int32_t m_cases, int32_t m_ctrls, int64_t draws, "
            "uint64_t seed, const double* table_a, int nrow_a, int ncol_a, const double* table_b, int nrow_b, int ncol_b, "
            "const double* cut, int32_t n_cut, gcre_set_score* out, int64_t cap, int64_t* n_out, int64_t* n_a, int64_t* n_b, "
            "int64_t* n_both, double* scores_a, double* scores_b);") in flat
    assert "int64_t gcre_subsample_launches(const gcre_ctx* ctx);" in flat
    assert re.search(r"#define GCRE_SUBSAMPLE_MAX_CUTS 8\b", header)
    assert {"gcre_score_sets_subsample", "gcre_subsample_launches"} <= set(api.EXPORTS)
    declared = set(re.findall(r"\b(gcre_[a-z0-9_]+)\s*\(", header))
    assert declared == set(api.EXPORTS)
    parent, needs, _, binds = api._FEATURES["subsample"]
    assert parent == "sets" and set(needs) == set(binds) == {"gcre_score_sets_subsample", "gcre_subsample_launches"}
    assert len(binds["gcre_score_sets_subsample"][1]) == 22
    from geneticscre_amd import build
    assert "gcre_subsample.hip" in build.SOURCES and "gcre_subsample.h" in build.HEADERS
    kernels = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_kernels.h")).read()
    assert "launch_subsample_null(" in kernels and "launch_subsample_masks(" in kernels and "struct SubsampleArgs" in kernels
    lib = api._subsample_lib()                               # loads without a GPU
    assert lib.gcre_abi_version() == 4 and lib.gcre_subsample_launches(None) == -1
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.19" in design and "k_subsample_null" in design and "Not built" in design
    # the mask generator of the permutations is untouched: the new kernel is a kernel of its own
    frontend = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_frontend.hip")).read()
    assert "subsample" not in frontend


def test_signatures():
    st = inspect.signature(api.JoinExec.subsample_tests).parameters
    assert list(st) == ["self", "sets", "rows", "signs", "m_cases", "m_ctrls", "draws", "seed", "table_a", "table_b", "cuts", "scores"]
    assert [st[k].default for k in list(st)[3:]] == [None, None, None, 100, 0, None, None, None, False]
    assert list(inspect.signature(api.JoinExec.subsample_launches).parameters) == ["self"]
    assert list(inspect.signature(report.subsample_masks).parameters) == ["n_cases", "n_ctrls", "m_cases", "m_ctrls", "draws", "seed"]
    assert list(inspect.signature(report.stability_columns).parameters) == ["counts", "valid", "draws"]
    assert list(inspect.signature(report.stability_bound).parameters) == ["q", "n_sets", "tau"]
    sp = inspect.signature(report.score_paths).parameters
    names = list(sp)
    assert names[-1] == "family_inference"                    # (tests/test_family_host.py requires it to stay last)
    i = names.index("stability")
    assert names[i:i + 2] == ["stability", "stability_cuts"] and names[i - 1] == "fixed"
    assert [sp[k].default for k in ("stability", "stability_cuts")] == [0, None]
    assert "stability" not in inspect.signature(report.gwaspa).parameters
    assert list(inspect.signature(report.gwaspa).parameters)[-1] == "patient_table"
    doc = " ".join(report.score_paths.__doc__.split())
    assert "no default" in doc and "the labels must not make it" in doc and "optimistic" in doc


def test_value_errors_come_before_the_library(monkeypatch):
    ex = api.JoinExec.__new__(api.JoinExec)
    ex.num_cases, ex.num_ctrls = 3, 2
    monkeypatch.setattr(api, "_feature_lib", lambda f: None)
    monkeypatch.setattr(api, "_subsample_lib", lambda: None)
    with pytest.raises(ValueError, match="cuts: one list, or one list per set"):
        api.JoinExec.subsample_tests(ex, [[0], [1]], np.zeros((4, 5), np.int8), cuts=[[1.0], [2.0], [3.0]])
    with pytest.raises(ValueError, match="signs: one sign per member of every set"):
        api.JoinExec.subsample_tests(ex, [[0, 1]], np.zeros((4, 5), np.int8), signs=[[1]])
    with pytest.raises(ValueError, match="stability > 0 needs stability_cuts"):
        report.score_paths(["A"], ["A"], np.zeros((1, 5), np.int8), 3, 2, stability=8)
    with pytest.raises(ValueError, match="must not be negative"):
        report.score_paths(["A"], ["A"], np.zeros((1, 5), np.int8), 3, 2, stability=-1)
