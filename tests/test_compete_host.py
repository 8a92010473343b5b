"""Competitive set tests, host side: the draw rule ``report.competitive_picks`` on a hand-worked example, its
properties on random inputs, its fallback and its uniformity; the same rule and the argument checks in C++ (csrc/gcre_compete.h),
driven by tests/native/compete_main.cpp under the address and undefined-behaviour sanitizers as a child process;
``competitive_reference`` against the definition taken literally; ``carrier_bins`` and ``competitive_columns`` on written-out
examples; the interface.  No GPU needed."""
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
SRC = os.path.join(ROOT, "tests", "native", "compete_main.cpp")
OK, ERR_ARG = 0, -4   # include/gcre_hip.h
M64 = (1 << 64) - 1


def mix(z):
    """splitmix64's finaliser on Python integers: the third statement of gcre_mix64 in this tree, next to C++ and numpy."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


# ---- the draw rule, hand-worked --------------------------------------------------------------------------------------


def test_picks_hand_worked():
    """Six rows, bin 0 = rows {0, 1, 3, 4}, bin 1 = rows {2, 5}; set 2 = rows (1, 5, 3); seed 5, draw 0.  Member 2 proposes row
    3 twice, which member 0 holds, and takes row 1 at its third attempt."""
    bins, members, seed, s, b = [0, 0, 1, 0, 0, 1], [1, 5, 3], 5, 2, 0
    key = mix(seed ^ ((0xD1B54A32D192ED03 * (s + 1)) & M64))
    base = mix(key ^ ((0x51ED270B7F3C9A1D * (b + 1)) & M64))
    assert (key, base) == (0xE9B7B8175C25D135, 0xF95E6D0349F8A9A4)
    # (member j, attempt t) -> u = mix(base + 64 j + t), the pool entry floor(u N / 2^64) and the row there
    steps = [(0, 0, 0xAE0156689D4E01A7, 4, 2, 3),     # 0.680 * 4 -> entry 2 of (0, 1, 3, 4)
             (1, 0, 0x6EBD5355E4F14F3D, 2, 0, 2),     # 0.433 * 2 -> entry 0 of (2, 5)
             (2, 0, 0x80FF45EC5E53E196, 4, 2, 3),     # 0.504 * 4 -> entry 2: taken
             (2, 1, 0xA5633F87E56AB833, 4, 2, 3),     # 0.646 * 4 -> entry 2: taken
             (2, 2, 0x721B2B2C6218206C, 4, 1, 1)]     # 0.446 * 4 -> entry 1
    pools = {4: (0, 1, 3, 4), 2: (2, 5)}
    for j, t, u, N, entry, row in steps:
        assert mix((base + 64 * j + t) & M64) == u
        assert (u * N) >> 64 == entry and pools[N][entry] == row
        assert int(report._mix64(np.uint64((base + 64 * j + t) & M64))) == u and int(report._mulhi(np.uint64(u), N)) == entry
    assert report.competitive_picks(members, bins, 6, s, b, seed).tolist() == [3, 2, 1]
    assert int(report._compete_base(seed, s, [b])[0]) == base
    # a fixed member stays itself and uses up no row of a pool; its position still counts in 64 j
    assert report.competitive_picks([1, 5, 3], [0, 0, 1, 0, 0, -1], 6, s, b, seed).tolist() == [3, 5, 1]
    # one attempt only: member 2 falls back to the lowest row of its bin not handed out
    assert report.competitive_picks(members, bins, 6, s, b, seed, attempts=1).tolist() == [3, 2, 0]
    assert report.competitive_picks(members, bins, 6, s, b, seed, attempts=2).tolist() == [3, 2, 0]
    assert report.competitive_picks(members, bins, 6, s, b, seed, attempts=3).tolist() == [3, 2, 1]


# ---- properties ------------------------------------------------------------------------------------------------------


def random_family(rng, n_rows, n_bins, n_sets, fixed_share=0.0):
    bins = rng.integers(0, n_bins, n_rows)
    bins[rng.random(n_rows) < fixed_share] = -1
    size = np.bincount(bins[bins >= 0], minlength=n_bins)
    sets = []
    for _ in range(n_sets):
        m = []
        for beta in range(n_bins):
            m += rng.integers(0, n_rows, rng.integers(0, size[beta] // 2 + 1)).tolist()      # any rows: replaced by rows of bin beta
        m = [int(r) for r in m]
        # a member draws from the bin of ITS row: keep k <= N / 2 in every bin by construction
        keep, need = [], np.zeros(n_bins, int)
        for r in m + np.flatnonzero(bins < 0)[:2].tolist():
            if bins[r] < 0 or 2 * (need[bins[r]] + 1) <= size[bins[r]]:
                keep.append(r)
                if bins[r] >= 0:
                    need[bins[r]] += 1
        if keep:
            rng.shuffle(keep)
            sets.append(keep)
    return bins, sets


def test_picks_properties():
    rng = np.random.default_rng(3)
    for trial in range(12):
        n_rows, n_bins = int(rng.integers(8, 80)), int(rng.integers(1, 5))
        bins, sets = random_family(rng, n_rows, n_bins, 5, fixed_share=0.1 * (trial % 3))
        seed = int(rng.integers(0, 2**63))
        bn, pools = report._compete_pools(bins, n_rows)
        for s, m in enumerate(sets):
            pk = report._compete_draws(m, bn, pools, s, np.arange(40), seed, 64)
            m = np.asarray(m)
            drawn = bins[m] >= 0
            for b in range(40):
                row = pk[b]
                assert len(set(row[drawn].tolist())) == int(drawn.sum())           # distinct within the draw
                assert np.array_equal(bins[row[drawn]], bins[m[drawn]])            # every pick in its member's bin
                assert np.array_equal(row[~drawn], m[~drawn])                      # fixed members are themselves
            # a function of (seed, s, b) only: one draw at a time, in any order, with other draws around it or not
            for b in (0, 7, 39):
                assert np.array_equal(report.competitive_picks(m, bins, n_rows, s, b, seed), pk[b])
            assert np.array_equal(report._compete_draws(m, bn, pools, s, [39, 3], seed, 64), pk[[39, 3]])
            if s > 0:
                assert not np.array_equal(report._compete_draws(m, bn, pools, s - 1, np.arange(40), seed, 64), pk)
    # the reference: a set's draws do not depend on the other sets of the list nor on the number of draws
    bins, sets = random_family(np.random.default_rng(8), 40, 2, 4)
    rows = np.random.default_rng(9).random((40, 30)) < 0.2
    VT = small_table(14, 16)
    full = report.competitive_reference(sets, rows, None, bins, 30, 21, 14, VT, 1)
    off = np.concatenate([[0], np.cumsum([len(x) for x in sets])])
    short = report.competitive_reference(sets, rows, None, bins, 11, 21, 14, VT, 1)
    assert np.array_equal(short["picks"], full["picks"][:11]) and np.array_equal(short["null"], full["null"][:, :11])
    # the same set at the same index in another list
    other = report.competitive_reference([sets[3], sets[1], sets[0]], rows, None, bins, 30, 21, 14, VT, 1)
    o2 = len(sets[3])
    assert np.array_equal(other["picks"][:, o2:o2 + len(sets[1])], full["picks"][:, off[1]:off[2]])
    assert np.array_equal(other["null"][1], full["null"][1]) and other["n_ge"][1] == full["n_ge"][1]
    with pytest.raises(ValueError, match="2k <= N"):
        report.competitive_picks([0, 1, 2], None, 5, 0, 0, 0)
    with pytest.raises(ValueError, match="bins: 3 entries for 5 rows"):
        report.competitive_picks([0], [0, 0, 0], 5, 0, 0, 0)


def test_fallback_keeps_the_picks_distinct():
    """attempts = 1 at the 2k = N limit: 6 members in a bin of 12.  The fallback is taken about 1.2 times a draw (the sum over
    j of j / 12 = 1.25 expected) and the picks stay distinct."""
    bn, pools = report._compete_pools(None, 12)
    one = report._compete_draws(np.arange(6), bn, pools, 0, np.arange(2000), 5, 1)
    full = report._compete_draws(np.arange(6), bn, pools, 0, np.arange(2000), 5, 64)
    assert all(len(set(r)) == 6 for r in one.tolist()) and one.min() >= 0 and one.max() < 12
    # a draw without a collision is the same under both; where the first attempt collided the fallback took the lowest free row
    fell = (one != full).any(axis=1)
    assert 0.5 < fell.mean() < 0.8                                                  # 1 - prod(1 - j / 12) = 0.777 collide at all
    j = np.argmax(one != full, axis=1)[fell]
    first = one[fell, j]
    for row, jj, f in zip(one[fell].tolist(), j.tolist(), first.tolist()):
        assert f == min(set(range(12)) - set(row[:jj]))
    # per draw: members whose first proposal was taken
    u = report._mix64(report._compete_base(5, 0, np.arange(2000))[:, None] + np.uint64(64) * np.arange(6, dtype=np.uint64)[None, :])
    prop = report._mulhi(u, 12)
    falls = sum(int(prop[b, jj] in one[b, :jj]) for b in range(2000) for jj in range(6))
    assert 1.1 < falls / 2000 < 1.4


def chi_square(counts):
    e = counts.sum() / counts.size
    return float(((counts - e) ** 2 / e).sum())


def test_uniformity_of_positions():
    """Seed 7, set 3, one bin of 12 rows, 6 members, 20,000 draws: every member position is uniform over the 12 rows.  The bound
    is the 99.9 % point of chi-square at 11 degrees of freedom."""
    bn, pools = report._compete_pools(None, 12)
    pk = report._compete_draws(np.arange(6), bn, pools, 3, np.arange(20000), 7, 64)
    stats = [chi_square(np.bincount(pk[:, j], minlength=12).astype(float)) for j in range(6)]
    print("chi-square per position:", [round(x, 1) for x in stats])
    assert all(x < 31.3 for x in stats), stats


def test_uniformity_of_ordered_pairs():
    """Seed 11, set 0, 2 members of one bin of 12 rows, 20,000 draws: the 132 ordered pairs of distinct rows are equally likely.
    The bound is the 99.9 % point of chi-square at 131 degrees of freedom."""
    bn, pools = report._compete_pools(None, 12)
    pk = report._compete_draws([4, 9], bn, pools, 0, np.arange(20000), 11, 64)
    assert (pk[:, 0] != pk[:, 1]).all()
    counts = np.zeros((12, 12))
    np.add.at(counts, (pk[:, 0], pk[:, 1]), 1)
    x = chi_square(counts[~np.eye(12, dtype=bool)])
    print("chi-square over the ordered pairs:", round(x, 1))
    assert x < 185, x


# ---- the C++ itself --------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("compete") / "compete_main")
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


def test_native_picks_equal_the_python_rule(prog, tmp_path):
    rng = np.random.default_rng(17)
    families = [(np.array([0, 0, 1, 0, 0, 1]), [[1, 5, 3], [0], [2, 4]], 6),       # the hand-worked pool
                (None, [list(range(6)), [11, 11, 3]], 12)]                           # no bin list; 2k = N; a repeated member
    for trial in range(4):
        n_rows, n_bins = int(rng.integers(20, 120)), int(rng.integers(1, 6))
        bins, sets = random_family(rng, n_rows, n_bins, 4, fixed_share=0.1 * (trial % 2))
        families.append((bins, sets, n_rows))
    big = np.zeros(2100, int)
    families.append((big, [rng.integers(0, 2100, 1024).tolist()], 2100))             # the member limit: j up to 1,023
    for fi, (bins, sets, n_rows) in enumerate(families):
        for attempts in (64, 1, 3):
            seed = int(rng.integers(0, 2**64, dtype=np.uint64))
            off = np.concatenate([[0], np.cumsum([len(x) for x in sets])]).tolist()
            ask = [(s, b) for s in range(len(sets)) for b in (0, 1, 5, 1000003)]
            case = [("n_rows", n_rows), ("n_sets", len(sets)), ("set_off", off), ("members", [r for x in sets for r in x]),
                    ("n_bins", 1 if bins is None else int(max(bins.max() + 1, 1))), ("draws", 10), ("seed", seed), ("attempts", attempts)]
            if bins is not None:
                case.append(("bin", bins.tolist()))
            case += [("pick", sb) for sb in ask]
            out = run_case(prog, tmp_path, case)
            assert out[0] == "check 0 ", out[0]
            assert len(out) == 1 + len(ask)
            for (s, b), ln in zip(ask, out[1:]):
                want = report.competitive_picks(sets[s], bins, n_rows, s, b, seed, attempts).tolist()
                assert ln.split() == ["picks", str(s), str(b)] + [str(x) for x in want], (fi, attempts, s, b)


def test_native_mix64_is_the_library_s(prog, tmp_path):
    zs = [0, 1, 2**63, M64, 0x9E3779B97F4A7C15, 123456789]
    out = run_case(prog, tmp_path, [("n_rows", 0), ("n_sets", 0), ("set_off", [0])] + [("mix", z) for z in zs])
    lib = api.load_library()
    assert out[1:] == [f"mix {z} {mix(z)}" for z in zs]
    assert [int(lib.gcre_mix64(z)) for z in zs] == [mix(z) for z in zs]


# four rows in bin 0, two in bin 1, row 6 never drawn; sets: two of bin 0 and the fixed row; one NA member with too many members
POOL = [("n_rows", 7), ("bin", [0, 0, 1, 0, 0, 1, -1]), ("n_bins", 2)]
LIST = [("n_sets", 2), ("set_off", [0, 3, 7]), ("members", [0, 6, 3, 0, 1, 3, -1])]
W = "score_sets_compete: "
CHECK_CASES = [
    ("accepted", POOL + LIST + [("draws", 5)], OK, ""),
    ("no draws", POOL + LIST + [("draws", 0)], OK, ""),
    ("NULL bin", [("n_rows", 7), ("n_bins", 1)] + LIST + [("draws", 5)], OK, ""),
    ("more bins than used", [("n_rows", 7), ("n_bins", 3)] + LIST + [("draws", 5)], OK, ""),
    ("no sets", POOL + [("n_sets", 0), ("set_off", [0]), ("draws", 5)], OK, ""),
    ("NULL n_ge", POOL + LIST + [("draws", 5), ("have_n_ge", 0)], ERR_ARG, W + "NULL argument (n_ge)"),
    ("negative draws", POOL + LIST + [("draws", -1)], ERR_ARG, W + "draws must not be negative, not -1"),
    ("no bins", [("n_rows", 7), ("n_bins", 0)] + LIST + [("draws", 5)], ERR_ARG, W + "n_bins must be at least 1, not 0"),
    ("bin above", [("n_rows", 7), ("bin", [0, 0, 1, 0, 2, 1, -1]), ("n_bins", 2)] + LIST + [("draws", 5)], ERR_ARG,
     W + "bin[4] = 2 out of range (2 bins, -1 = never drawn)"),
    ("bin below", [("n_rows", 7), ("bin", [0, -2, 1, 0, 0, 1, -1]), ("n_bins", 2)] + LIST + [("draws", 5)], ERR_ARG,
     W + "bin[1] = -2 out of range (2 bins, -1 = never drawn)"),
    ("2k > N", POOL + [("n_sets", 2), ("set_off", [0, 1, 4]), ("members", [2, 0, 1, 1]), ("draws", 5)], ERR_ARG,
     W + "set 1 draws 3 members from bin 0 of 4 rows: a bin must hold twice as many rows as a set draws from it"),
    ("2k > N in the second bin", POOL + [("n_sets", 1), ("set_off", [0, 3]), ("members", [2, 0, 5]), ("draws", 5)], ERR_ARG,
     W + "set 0 draws 2 members from bin 1 of 2 rows: a bin must hold twice as many rows as a set draws from it"),
    ("2k > N is not asked of an NA set", POOL + [("n_sets", 1), ("set_off", [0, 4]), ("members", [0, 1, 3, -1]), ("draws", 5)], OK, ""),
    ("too many members", [("n_rows", 3000), ("n_bins", 1), ("n_sets", 1), ("set_off", [0, 1025]), ("members", list(range(1025))),
                          ("draws", 5)], ERR_ARG, W + "set 0 has 1025 members, more than GCRE_COMPETE_MAX_MEMBERS = 1024"),
    ("the member limit itself", [("n_rows", 3000), ("n_bins", 1), ("n_sets", 1), ("set_off", [0, 1024]), ("members", list(range(1024))),
                                 ("draws", 5)], OK, ""),
    ("null scores above the bound", POOL + LIST + [("draws", 5), ("want_null", 1), ("max_mb", 0.00001)], ERR_ARG,
     W + "the optional outputs of one draw take 16 bytes: above GCRE_COMPETE_MAX_MB = 0.000010"),
    ("picks above the bound", POOL + LIST + [("draws", 5), ("want_picks", 1), ("max_mb", 0.00002)], ERR_ARG,
     W + "the optional outputs of one draw take 28 bytes: above GCRE_COMPETE_MAX_MB = 0.000020"),
    ("the bound is not asked without optional outputs", POOL + LIST + [("draws", 5), ("max_mb", 0)], OK, ""),
    ("nor without draws", POOL + LIST + [("draws", 0), ("want_null", 1), ("want_picks", 1), ("max_mb", 0)], OK, ""),
]


@pytest.mark.parametrize("name,case,code,message", CHECK_CASES, ids=[c[0] for c in CHECK_CASES])
def test_argument_checks_under_sanitizers(prog, tmp_path, name, case, code, message):
    assert run_case(prog, tmp_path, case) == [f"check {code} {message}"]


# ---- the definition --------------------------------------------------------------------------------------------------


def literal(sets, rows, signs, bins, draws, seed, n_cases, VT, method, attempts=64):
    """gcre_score_sets_compete taken literally: one draw at a time, Python integers and sets."""
    rows = np.asarray(rows) != 0
    n_rows, n = rows.shape
    bins = [0] * n_rows if bins is None else [int(x) for x in bins]
    pool = {beta: [r for r in range(n_rows) if bins[r] == beta] for beta in set(bins) if beta >= 0}
    n_ge, null, picks = [], [], [[] for _ in range(draws)]

    def score(rs, sg):
        P, N = set(), set()
        for r, g in zip(rs, sg):
            (N if method == 2 and g == -1 else P).update(np.flatnonzero(rows[r]).tolist())
        cell = lambda a, b: float(VT[a][b]) if a < VT.shape[0] and b < VT.shape[1] else -1.0     # (the device's padding)
        v = cell(sum(q < n_cases for q in P), sum(q >= n_cases for q in P))
        if method == 2:
            v = v + cell(sum(q >= n_cases for q in N), sum(q < n_cases for q in N))
        return v

    for s, m in enumerate(sets):
        sg = [1] * len(m) if signs is None else signs[s]
        if any(r < 0 for r in m):
            n_ge.append(-1)
            null.append([float("nan")] * draws)
            for b in range(draws):
                picks[b] += [-1] * len(m)
            continue
        obs = score(m, sg)
        key = mix(seed ^ ((0xD1B54A32D192ED03 * (s + 1)) & M64))
        row_null = []
        for b in range(draws):
            base = mix(key ^ ((0x51ED270B7F3C9A1D * (b + 1)) & M64))
            got, out = set(), []
            for j, r in enumerate(m):
                if bins[r] < 0:
                    out.append(r)
                    continue
                p = pool[bins[r]]
                for t in range(attempts):
                    c = p[(mix((base + 64 * j + t) & M64) * len(p)) >> 64]
                    if c not in got:
                        break
                else:
                    c = min(set(p) - got)
                got.add(c)
                out.append(c)
            picks[b] += out
            row_null.append(score(out, sg))
        null.append(row_null)
        n_ge.append(sum(x >= obs for x in row_null))
    return n_ge, null, picks


@pytest.mark.parametrize("method", [1, 2])
def test_reference_equals_the_definition(method):
    rng = np.random.default_rng(40 + method)
    n_cases, n_ctrls = 9, 12
    VT = small_table(n_cases, n_ctrls, method)
    VT[2, 3] = np.nan
    for trial in range(4):
        n_rows = int(rng.integers(12, 40))
        bins, sets = random_family(rng, n_rows, int(rng.integers(1, 4)), 5, fixed_share=0.1 * (trial % 2))
        sets.append([int(sets[0][0]), -1])
        signs = [rng.choice([1, -1], len(x)).tolist() for x in sets] if trial != 1 else None
        rows = rng.random((n_rows, n_cases + n_ctrls)) < 0.15
        for attempts in (64, 1):
            got = report.competitive_reference(sets, rows, signs, None if trial == 3 and len(set(bins.tolist())) == 1 else bins, 25, 77,
                                               n_cases, VT, method, attempts)
            n_ge, null, picks = literal(sets, rows, signs, bins, 25, 77, n_cases, VT, method, attempts)
            assert got["n_ge"].tolist() == n_ge
            assert got["picks"].tolist() == picks
            assert np.array_equal(got["null"].view(np.uint64), np.array(null, np.float64).view(np.uint64))
    none = report.competitive_reference([[0, 1]], rows, None, None, 0, 1, n_cases, VT, method)
    assert none["n_ge"].tolist() == [0] and none["null"].shape == (1, 0) and none["picks"].shape == (0, 2)


def test_carrier_bins_written_out():
    data = np.zeros((7, 6), int)
    for r, c in enumerate([3, 0, 5, 3, 1, 0, 2]):        # carrier totals by row
        data[r, :c] = 1
    # ascending, ties by row: rows 1, 5, 4, 6, 0, 3, 2
    assert report.carrier_bins(data, 1).tolist() == [0] * 7
    assert report.carrier_bins(data, 2).tolist() == [1, 0, 1, 1, 0, 0, 0]     # positions 0..3 -> bin 0 (7 = 4 + 3)
    assert report.carrier_bins(data, 3).tolist() == [1, 0, 2, 2, 0, 0, 1]     # 3 + 2 + 2: rows (1, 5, 4), (6, 0), (3, 2)
    assert report.carrier_bins(data, 7).tolist() == [4, 0, 6, 5, 2, 1, 3]
    assert report.carrier_bins(data, 10).max() < 10 and len(set(report.carrier_bins(data, 10).tolist())) == 7
    assert report.carrier_bins(data, 3).dtype == np.int32
    assert report.carrier_bins(np.zeros((0, 4)), 3).tolist() == []
    sizes = np.bincount(report.carrier_bins(np.random.default_rng(0).random((103, 50)) < 0.3, 10))
    assert sizes.max() - sizes.min() <= 1 and sizes.sum() == 103


def test_competitive_columns_written_out():
    col = report.competitive_columns([0, 5, 20, -1, 7], [1, 1, 1, 0, 0], 20)
    assert list(col) == report.COMPETITIVE_COLUMNS == ["CompetitivePvalues"]
    got = col["CompetitivePvalues"]
    assert got[:3].tolist() == [0.0, 0.25, 1.0] and np.isnan(got[3:]).all()       # n / K; an NA member; a NaN score (valid 0)
    assert np.isnan(report.competitive_columns([0, 0], [1, 1], 0)["CompetitivePvalues"]).all()
    assert np.isnan(report.competitive_columns([-1], [1], 5)["CompetitivePvalues"]).all()


# ---- the interface ---------------------------------------------------------------------------------------------------


def test_interface_is_declared():
    header = open(os.path.join(ROOT, "include", "gcre_hip.h")).read()
    assert re.search(r"#define GCRE_ABI_VERSION 4\b", header)      # additions only
    flat = " ".join(header.split())
    assert ("int gcre_score_sets_compete(gcre_ctx* ctx, const gcre_set_input* in, const int32_t* bin, int32_t n_bins, int64_t draws, "
            "uint64_t seed, gcre_set_score* out, int64_t cap, int64_t* n_out, int64_t* n_ge, double* null_scores, int32_t* picks);") in flat
    assert "int64_t gcre_compete_launches(const gcre_ctx* ctx);" in flat
    assert int(re.search(r"#define GCRE_COMPETE_MAX_MEMBERS (\d+)", header).group(1)) >= 1024
    assert {"gcre_score_sets_compete", "gcre_compete_launches"} <= set(api.EXPORTS)
    declared = set(re.findall(r"\b(gcre_[a-z0-9_]+)\s*\(", header))
    assert declared == set(api.EXPORTS)
    parent, needs, _, binds = api._FEATURES["compete"]
    assert parent == "sets" and set(needs) == set(binds) == {"gcre_score_sets_compete", "gcre_compete_launches"}
    assert len(binds["gcre_score_sets_compete"][1]) == 12
    from geneticscre_amd import build
    assert "gcre_compete.hip" in build.SOURCES and "gcre_compete.h" in build.HEADERS
    kernels = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_kernels.h")).read()
    assert "launch_compete_null(" in kernels and "struct CompeteArgs" in kernels
    lib = api._compete_lib()                                 # loads without a GPU
    assert lib.gcre_abi_version() == 4 and lib.gcre_compete_launches(None) == -1
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.17" in design and "competitive" in design.lower()


def test_signatures():
    ct = inspect.signature(api.JoinExec.competitive_tests).parameters
    assert list(ct) == ["self", "sets", "rows", "signs", "bins", "draws", "seed", "null", "picks"]
    assert [ct[k].default for k in ("signs", "bins", "draws", "seed", "null", "picks")] == [None, None, 1000, 0, False, False]
    assert list(inspect.signature(api.JoinExec.compete_launches).parameters) == ["self"]
    assert list(inspect.signature(report.competitive_picks).parameters) == ["set_members", "bins", "n_rows", "s", "b", "seed", "attempts"]
    assert inspect.signature(report.competitive_picks).parameters["attempts"].default == 64
    assert list(inspect.signature(report.competitive_reference).parameters) == [
        "sets", "rows", "signs", "bins", "draws", "seed", "n_cases", "table", "method", "attempts"]
    assert list(inspect.signature(report.carrier_bins).parameters) == ["data", "n_bins"]
    assert list(inspect.signature(report.competitive_columns).parameters) == ["n_ge", "valid", "draws"]
    sp = inspect.signature(report.score_paths).parameters
    names = list(sp)
    assert names[-1] == "family_inference"                    # (tests/test_family_host.py requires it to stay last)
    i = names.index("competitive")
    assert names[i:i + 3] == ["competitive", "competitive_bins", "fixed"] and i < names.index("family_inference")
    assert names[i - 1] == "minp"
    assert [sp[k].default for k in ("competitive", "competitive_bins", "fixed")] == [0, 10, None]
    assert list(inspect.signature(report.gwaspa).parameters)[-1] == "patient_table"
    assert "competitive" not in inspect.signature(report.gwaspa).parameters


def test_value_errors_come_before_the_library(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched")
    ex = api.JoinExec.__new__(api.JoinExec)
    ex.num_cases, ex.num_ctrls = 3, 2
    monkeypatch.setattr(api, "_feature_lib", lambda f: None)
    monkeypatch.setattr(api, "_compete_lib", lambda: None)
    with pytest.raises(ValueError, match="bins: 2 entries for 4 rows"):
        api.JoinExec.competitive_tests(ex, [[0]], np.zeros((4, 5), np.int8), bins=[0, 0])
    with pytest.raises(ValueError, match="signs: one sign per member of every set"):
        api.JoinExec.competitive_tests(ex, [[0, 1]], np.zeros((4, 5), np.int8), signs=[[1]])
