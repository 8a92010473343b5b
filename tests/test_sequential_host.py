"""Sequential permutation p-values, host side: the mask rule ``report.permutation_masks`` on a hand-worked
mask with two strata, its case counts per stratum and its dependence on (seed, r, patient) only; ``sequential_reference`` on
written-out bit rows; ``sequential_columns`` on written-out counts; the same rule, the search in a bit row, the argument checks
and the batch schedule in C++ (csrc/gcre_sequential.h), driven by tests/native/sequential_main.cpp under the address and
undefined-behaviour sanitizers as a child process; the interface.  No GPU needed."""
from __future__ import annotations

import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from geneticscre_amd import api, report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sequential_main.cpp")
OK, ERR_RANGE, ERR_ARG = 0, -2, -4   # include/gcre_hip.h
M64 = (1 << 64) - 1
TILE = 512


def mix(z):
    """splitmix64's finaliser on Python integers."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def literal_mask(n_cases, n_ctrls, r, seed, strata=None):
    """Permutation r on Python integers, one patient at a time."""
    n = n_cases + n_ctrls
    st = [0] * n if strata is None else [int(s) for s in strata]
    need = {s: sum(1 for c in range(n_cases) if st[c] == s) for s in set(st)}
    rem = {s: st.count(s) for s in set(st)}
    base = mix(seed ^ ((0x51ED270B7F3C9A1D * (r + 1)) & M64))
    out = []
    for c in range(n):
        s = st[c]
        take = (mix((base + c) & M64) * rem[s]) >> 64 < need[s]
        need[s] -= take
        rem[s] -= 1
        out.append(int(take))
    return out


# ---- the mask rule ---------------------------------------------------------------------------------------------------


def test_mask_hand_worked_with_two_strata():
    """Three cases, three controls; stratum 0 holds patients 0, 2, 5 (two cases), stratum 1 patients 1, 3, 4 (one case); seed
    7, permutation 2.  Patient 0 misses two chances in three, so patients 2 and 5 must both become cases; patient 1 takes the
    one case of its stratum at once."""
    seed, r, strata = 7, 2, [0, 1, 0, 1, 1, 0]
    base = mix(seed ^ ((0x51ED270B7F3C9A1D * (r + 1)) & M64))
    assert base == 0x2AB5EFB23B3292E3
    # patient c -> u = mix(base + c), its stratum, the patients left in it, the cases still to place, floor(u rem / 2^64), taken
    steps = [(0, 0xDB2F8DD8549FDEF5, 0, 3, 2, 2, False),     # 0.856 * 3 -> 2
             (1, 0x3008FFA910D217FF, 1, 3, 1, 0, True),      # 0.188 * 3 -> 0 < 1
             (2, 0xEB64A2580CD6CEC0, 0, 2, 2, 1, True),      # two left, two to place
             (3, 0x8D44AFB60D0E0511, 1, 2, 0, 1, False),     # nothing left to place
             (4, 0x89BD09C99315D11D, 1, 1, 0, 0, False),
             (5, 0x212359238B7219E1, 0, 1, 1, 0, True)]      # the last of its stratum with one to place
    for c, u, s, rem, need, pick, take in steps:
        assert mix((base + c) & M64) == u and strata[c] == s
        assert (u * rem) >> 64 == pick and (pick < need) == take
        assert int(report._mix64(np.uint64((base + c) & M64))) == u and int(report._mulhi(np.uint64(u), rem)) == pick
    want = [0, 1, 1, 0, 0, 1]
    assert literal_mask(3, 3, r, seed, strata) == want
    assert report.permutation_masks(3, 3, [2], seed, strata).astype(int).tolist() == [want]
    assert report.permutation_masks(3, 3, 3, seed, strata).astype(int)[2].tolist() == want
    # one stratum: the same stream, other needs
    assert report.permutation_masks(3, 3, [2], seed).astype(int).tolist() == [literal_mask(3, 3, 2, seed)]


@pytest.mark.parametrize("n_strata", [1, 3])
@pytest.mark.parametrize("shape", [(1, 1), (31, 2), (33, 31), (64, 1), (65, 135)])
def test_exact_case_counts_per_stratum(shape, n_strata):
    nc, nt = shape
    n = nc + nt
    rng = np.random.default_rng([7100, nc, nt, n_strata])
    strata = None if n_strata == 1 else rng.integers(0, n_strata, n)
    mk = report.permutation_masks(nc, nt, 200, 11, strata)
    assert mk.shape == (200, n) and mk.dtype == bool
    st = np.zeros(n, int) if strata is None else strata
    for s in range(n_strata):
        assert (mk[:, st == s].sum(axis=1) == (st[:nc] == s).sum()).all()
    assert (mk.sum(axis=1) == nc).all()
    if n > 2:
        assert len({row.tobytes() for row in mk}) > 1
    for r in (0, 199):
        assert mk[r].astype(int).tolist() == literal_mask(nc, nt, r, 11, strata)


def test_masks_depend_on_seed_permutation_and_patient_only():
    strata = np.arange(50) % 3
    full = report.permutation_masks(20, 30, 50, 3, strata)
    assert np.array_equal(report.permutation_masks(20, 30, [49, 7, 7], 3, strata), full[[49, 7, 7]])
    assert not np.array_equal(report.permutation_masks(20, 30, 50, 4, strata), full)
    assert not np.array_equal(full[0], full[1])
    # a permutation index far beyond any context: 64-bit, and still the literal rule
    big = [2**40 - 1, 2**33 + 5]
    got = report.permutation_masks(20, 30, big, 3, strata).astype(int).tolist()
    assert got == [literal_mask(20, 30, r, 3, strata) for r in big]
    # no tag between the seed and the base: permutation r of any context is mask r here
    assert int(report._mix64(np.uint64(3 ^ 0x51ED270B7F3C9A1D))) == mix(3 ^ 0x51ED270B7F3C9A1D)
    with pytest.raises(ValueError, match="strata: one id >= 0 per patient"):
        report.permutation_masks(3, 3, 1, 0, [0, 1])
    with pytest.raises(ValueError, match="strata: one id >= 0 per patient"):
        report.permutation_masks(2, 1, 1, 0, [0, -1, 0])


# ---- the definition on written-out bit rows ----------------------------------------------------------------------------


def rows_to_null(rows):
    """Bit rows (strings of 0 / 1) -> a null matrix whose score 1.0 is reached exactly where a row says 1."""
    return np.array([[2.0 if ch == "1" else 0.5 for ch in row] for row in rows], np.float32)


def test_reference_on_written_out_rows():
    rows = ["1100000000",      # h = 2: the h-th hit at position 2; h = 1: at position 1
            "0000010001",      # h = 2: at the last position = max_perms exactly
            "0000010000",      # h = 2: never, one hit
            "0000000000",      # never, no hit
            "1111111111"]
    null = rows_to_null(rows)
    obs = np.ones(5)
    valid = np.ones(5, int)
    ref = report.sequential_reference(null, obs, valid, 2, 10)
    assert ref["n_hit"].tolist() == [2, 2, 1, 0, 2] and ref["n_perm"].tolist() == [2, 10, 10, 10, 2]
    assert ref["stopped"].tolist() == [1, 1, 0, 0, 1]
    assert ref["n_hit"].dtype == np.int64 and ref["n_perm"].dtype == np.int64 and ref["stopped"].dtype == np.int32
    one = report.sequential_reference(null, obs, valid, 1, 10)
    assert one["n_perm"].tolist() == [1, 6, 6, 10, 1] and one["n_hit"].tolist() == [1, 1, 1, 0, 1] and one["stopped"].tolist() == [1, 1, 1, 0, 1]
    # a shorter limit cuts the row: the hit at position 10 is not seen
    cut = report.sequential_reference(null, obs, valid, 2, 9)
    assert cut["n_perm"].tolist() == [2, 9, 9, 9, 2] and cut["n_hit"].tolist() == [2, 1, 1, 0, 2] and cut["stopped"].tolist() == [1, 0, 0, 0, 1]
    # a NaN score never counts; a NaN null score neither; an invalid set gets -1; the compare is >= in float64
    odd = report.sequential_reference(null, [np.nan, 1.0, 2.0, 0.5, 0.0], [1, 0, 1, 1, 1], 1, 10)
    assert odd["n_hit"].tolist() == [0, -1, 1, 1, 1] and odd["n_perm"].tolist() == [10, -1, 6, 1, 1] and odd["stopped"].tolist() == [0, 0, 1, 1, 1]
    nn = null.copy()
    nn[0, 0] = np.nan
    assert report.sequential_reference(nn, obs, valid, 1, 10)["n_perm"][0] == 2
    tie = np.float32(0.1)                                       # (float64)(float32)0.1 > 0.1: counts
    assert report.sequential_reference([[tie]], [0.1], [1], 1, 1)["stopped"].tolist() == [1]
    assert report.sequential_reference([[tie]], [float(np.nextafter(np.float64(tie), 1.0))], [1], 1, 1)["stopped"].tolist() == [0]
    # no permutation at all: zeros for a valid set
    zero = report.sequential_reference(null, obs, [1, 1, 0, 1, 1], 3, 0)
    assert zero["n_hit"].tolist() == [0, 0, -1, 0, 0] and zero["n_perm"].tolist() == [0, 0, -1, 0, 0] and not zero["stopped"].any()
    assert report.sequential_reference(np.zeros((0, 4)), [], [], 1, 4)["n_hit"].shape == (0,)
    with pytest.raises(ValueError, match="hits = 0 must be at least 1"):
        report.sequential_reference(null, obs, valid, 0, 10)
    with pytest.raises(ValueError, match="10 null scores per set for max_perms = 11"):
        report.sequential_reference(null, obs, valid, 1, 11)


def test_sequential_columns_written_out():
    seq = {"n_hit": [20, 3, 0, -1, 0, 20], "n_perm": [40, 1000, 1000, -1, 0, 1000], "stopped": [1, 0, 0, 0, 0, 1]}
    cols = report.sequential_columns(seq, [1, 1, 1, 0, 1, 1])
    assert list(cols) == report.SEQUENTIAL_COLUMNS == ["SequentialPvalues", "SequentialPerms", "SequentialHits", "SequentialStopped"]
    assert cols["SequentialPvalues"][[0, 1, 2, 5]].tolist() == [0.5, 0.003, 0.0, 0.02]
    assert np.isnan(cols["SequentialPvalues"][[3, 4]]).all()                      # an NA member; no permutation used
    assert cols["SequentialPerms"][[0, 1, 2, 4, 5]].tolist() == [40, 1000, 1000, 0, 1000] and np.isnan(cols["SequentialPerms"][3])
    assert cols["SequentialHits"][[0, 1, 2, 4, 5]].tolist() == [20, 3, 0, 0, 20] and np.isnan(cols["SequentialHits"][3])
    assert cols["SequentialStopped"][[0, 1, 2, 4, 5]].tolist() == [1, 0, 0, 0, 1] and np.isnan(cols["SequentialStopped"][3])
    # the records of the binding are read the same way; a valid flag that is off hides a row whatever its counts
    rec = np.zeros(2, api.SEQ_SCORE)
    rec["n_hit"], rec["n_perm"], rec["stopped"] = [5, 5], [10, 10], [1, 1]
    cols = report.sequential_columns(rec, [1, 0])
    assert cols["SequentialPvalues"][0] == 0.5 and all(np.isnan(v[1]) for v in cols.values())


# ---- the C++ itself --------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sequential") / "sequential_main")
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
    rng = np.random.default_rng(29)
    shapes = [(3, 3, 2), (1, 1, 1), (31, 2, 1), (32, 32, 3), (33, 31, 3), (64, 1, 1), (65, 135, 3), (70, 61, 7)]
    for _ in range(4):
        shapes.append((int(rng.integers(1, 300)), int(rng.integers(1, 300)), int(rng.integers(1, 5))))
    for nc, nt, ns in shapes:
        n = nc + nt
        seed = int(rng.integers(0, 2**64, dtype=np.uint64))
        strata = None if ns == 1 else rng.integers(0, ns, n).tolist()
        ask = [0, 1, 5, 511, 512, 1000003, 2**40 - 1]
        case = [("n_cases", nc), ("n_ctrls", nt), ("seed", seed)] + ([("n_strata", ns), ("strata", strata)] if strata else [])
        out = run_case(prog, tmp_path, case + [("mask", r) for r in ask])
        assert out[0] == "check 0 ", out[0]
        want = report.permutation_masks(nc, nt, ask, seed, strata)
        assert out[1:] == [f"mask {r} " + "".join("1" if x else "0" for x in row) for r, row in zip(ask, want)], (nc, nt, ns)


def test_native_mix64_is_the_library_s(prog, tmp_path):
    zs = [0, 1, 2**63, M64, 0x9E3779B97F4A7C15, 123456789]
    out = run_case(prog, tmp_path, [("mix", z) for z in zs])
    lib = api.load_library()
    assert out[1:] == [f"mix {z} {mix(z)}" for z in zs]
    assert [int(lib.gcre_mix64(z)) for z in zs] == [mix(z) for z in zs]


def words_of(bits):
    """A list of 0 / 1 -> hexadecimal 64-bit words, bit i & 63 of word i >> 6."""
    out = []
    for w in range((len(bits) + 63) // 64):
        out.append(format(sum(b << i for i, b in enumerate(bits[64 * w:64 * w + 64])), "x"))
    return out


def find_literal(bits, prior, h):
    seen = prior
    for i, b in enumerate(bits):
        seen += b
        if b and seen == h:
            return i
    return -1


def test_native_find_in_bit_rows(prog, tmp_path):
    rng = np.random.default_rng(31)
    cases = []

    def ask(bits, prior, h):
        cases.append((("find", [prior, h, len(bits)] + words_of(bits)), find_literal(bits, prior, h)))

    row = [0] * 320
    row[0] = 1
    ask(row, 0, 1)                                   # the crossing bit is bit 0
    ask(row, 4, 5)
    row = [0] * 64
    row[63] = 1
    ask(row, 0, 1)                                   # bit 63
    row = [0] * 300
    row[299] = row[10] = 1
    ask(row, 0, 2)                                   # in the last word, at the last bit of a partial word
    ask(row, 0, 3)                                   # not in this batch
    row = [0] * 512
    row[5] = row[64 * 5 + 17] = 1
    ask(row, 0, 2)                                   # in a word after several empty ones
    ask(row, 1, 2)
    ask([1] * 512, 0, 512)                           # every bit: the last one
    ask([1] * 512, 0, 65)                            # the first bit of the second word
    ask([1] * 512, 30, 94)                           # bit 63 of the first word
    ask([0] * 512, 0, 1)
    for _ in range(40):
        nb = int(rng.integers(1, 1400))
        bits = (rng.random(nb) < rng.choice([0.01, 0.2, 0.9])).astype(int).tolist()
        prior = int(rng.integers(0, 50))
        ask(bits, prior, prior + int(rng.integers(1, 40)))
    out = run_case(prog, tmp_path, [c for c, _ in cases])
    assert out[1:] == [f"find {w}" for _, w in cases]
    assert {w for _, w in cases} >= {-1, 0, 63, 299, 511}


W = "score_sets_sequential: "
COHORT = [("n_cases", 3), ("n_ctrls", 4)]
CHECK_CASES = [
    ("accepted", COHORT + [("hits", 20), ("max_perms", 1000)], OK, ""),
    ("no permutations", COHORT + [("hits", 1), ("max_perms", 0)], OK, ""),
    ("the largest hits", COHORT + [("hits", 2**31 - 1), ("max_perms", 1)], OK, ""),
    ("the largest limit", COHORT + [("hits", 1), ("max_perms", 2**40)], OK, ""),
    ("with strata", COHORT + [("hits", 1), ("max_perms", 5), ("n_strata", 2), ("strata", [0, 1, 0, 1, 0, 1, 1])], OK, ""),
    ("n_strata without strata is ignored", COHORT + [("hits", 1), ("max_perms", 5), ("n_strata", -3)], OK, ""),
    ("NULL seq_out", COHORT + [("hits", 1), ("max_perms", 5), ("have_seq_out", 0)], ERR_ARG, W + "NULL argument (seq_out)"),
    ("hits zero", COHORT + [("hits", 0), ("max_perms", 5)], ERR_ARG, W + "hits = 0 outside 1 .. 2147483647"),
    ("hits negative", COHORT + [("hits", -4), ("max_perms", 5)], ERR_ARG, W + "hits = -4 outside 1 .. 2147483647"),
    ("hits above", COHORT + [("hits", 2**31), ("max_perms", 5)], ERR_ARG, W + "hits = 2147483648 outside 1 .. 2147483647"),
    ("max_perms negative", COHORT + [("hits", 1), ("max_perms", -1)], ERR_ARG, W + "max_perms = -1 outside 0 .. 1099511627776"),
    ("max_perms above", COHORT + [("hits", 1), ("max_perms", 2**40 + 1)], ERR_ARG,
     W + "max_perms = 1099511627777 outside 0 .. 1099511627776"),
    ("strata without a count", COHORT + [("hits", 1), ("max_perms", 5), ("n_strata", 0), ("strata", [0] * 7)], ERR_ARG, W + "bad strata"),
    ("stratum id above", COHORT + [("hits", 1), ("max_perms", 5), ("n_strata", 2), ("strata", [0, 1, 2, 0, 0, 0, 0])], ERR_RANGE,
     W + "stratum id out of range"),
    ("stratum id negative", COHORT + [("hits", 1), ("max_perms", 5), ("n_strata", 2), ("strata", [0, 1, 0, 0, 0, 0, -1])], ERR_RANGE,
     W + "stratum id out of range"),
]


@pytest.mark.parametrize("name,case,code,message", CHECK_CASES, ids=[c[0] for c in CHECK_CASES])
def test_argument_checks_under_sanitizers(prog, tmp_path, name, case, code, message):
    assert run_case(prog, tmp_path, case) == [f"check {code} {message}"]


def test_native_batch_schedule(prog, tmp_path):
    # the batch before, mask dwords per permutation, active sets, the bound in MB, the cap in permutations (0: none) -> batch
    asks = [((0, 8, 40, 1024, 0), 4096),                               # the first batch
            ((4096, 8, 40, 1024, 0), 16384), ((16384, 8, 40, 1024, 0), 65536),   # four times the one before
            ((0, 8, 40, 1024, 512), 512), ((512, 8, 40, 1024, 512), 512),        # capped
            ((0, 8, 40, 1024, 1300), 1024),                            # the cap is rounded down to whole tiles
            ((0, 8, 40, 1024, 1), 512),                                # ... one tile at the least
            ((65536, 1564, 1100, 1024, 0), 167936),                    # 512 x (6,256 + 137.5) bytes a tile of masks and bit rows: 328 tiles
            ((4096, 1564, 1100, 0, 0), 512),                           # no room at all: one tile
            ((4096, 8, 8 * 10**6, 8000, 0), 512 * 16),                 # 1,000,032 bytes a permutation, most of it bit rows: 16 tiles in 8000 MB
            ((0, 8, 40, 512 * 37 * 3 / 2**20, 0), 1536),               # 37 bytes a permutation: exactly three tiles
            ((2**29, 8, 1, 1048576, 0), 2**27),                        # the masks of a batch stay below 2^30 dwords
            ((2**28, 2, 1, 1048576, 0), 2**29)]
    out = run_case(prog, tmp_path, [("batch", a) for a, _ in asks])
    assert out[1:] == [f"batch {w}" for _, w in asks]
    # whole calls: always whole tiles but the last, always advancing, never above the bound, the sum is max_perms
    sched = [((8, 40, 1024, 0, 20001), [4096, 15905]),
             ((8, 40, 1024, 512, 3000), [512] * 5 + [440]),
             ((8, 40, 1024, 1024, 3000), [1024, 1024, 952]),
             ((8, 40, 1024, 0, 700), [700]),
             ((8, 40, 1024, 0, 0), []),
             ((8, 40, 0.001, 0, 2000), [512, 512, 512, 464]),
             ((1564, 1100, 1024, 0, 10**6), [4096, 16384, 65536] + [167936] * 5 + [74304])]
    out = run_case(prog, tmp_path, [("schedule", a) for a, _ in sched])
    assert out[1:] == [" ".join(["schedule"] + [str(x) for x in w]) for _, w in sched]
    for (dwords, active, mb, cap, total), w in sched:
        assert sum(w) == total and all(x > 0 for x in w) and all(x % TILE == 0 for x in w[:-1])
        if mb >= 1:
            assert all(x * (4 * dwords + active / 8) <= mb * 2**20 for x in w)


# ---- the interface ---------------------------------------------------------------------------------------------------


def test_interface_is_declared():
    header = open(os.path.join(ROOT, "include", "gcre_hip.h")).read()
    assert re.search(r"#define GCRE_ABI_VERSION 4\b", header)      # additions only
    flat = " ".join(header.split())
    assert ("int gcre_score_sets_sequential(gcre_ctx* ctx, const gcre_set_input* in, uint64_t seed, const int32_t* stratum, "
            "int n_strata, int64_t h, int64_t max_perms, gcre_set_score* out, int64_t cap, int64_t* n_out, "
            "gcre_seq_score* seq_out /* [n_sets] */);") in flat
    assert "int64_t gcre_sequential_launches(const gcre_ctx* ctx);" in flat
    prose = flat.replace(" * ", " ")
    assert "Not built: family-wise versions" in prose and "an early stop for sets that are clearly significant" in prose
    assert {"gcre_score_sets_sequential", "gcre_sequential_launches"} <= set(api.EXPORTS)
    declared = set(re.findall(r"\b(gcre_[a-z0-9_]+)\s*\(", header))
    assert declared == set(api.EXPORTS)
    parent, needs, _, binds = api._FEATURES["sequential"]
    assert parent == "sets" and set(needs) == set(binds) == {"gcre_score_sets_sequential", "gcre_sequential_launches"}
    assert len(binds["gcre_score_sets_sequential"][1]) == 11
    assert api.SEQ_SCORE.itemsize == 24 and api.SEQ_SCORE.names == ("n_hit", "n_perm", "stopped", "pad")
    from geneticscre_amd import build
    assert {"gcre_sequential.hip", "gcre_host_sequential.hip"} <= set(build.SOURCES) and "gcre_sequential.h" in build.HEADERS
    kernels = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_kernels.h")).read()
    assert all(x in kernels for x in ("launch_seq_masks(", "launch_seq_null(", "launch_seq_retire(", "struct SeqNullArgs"))
    lib = api._feature_lib("sequential")                     # loads without a GPU
    assert lib.gcre_abi_version() == 4 and lib.gcre_sequential_launches(None) == -1
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.21" in design and all(k in design for k in ("k_seq_masks", "k_seq_null", "k_seq_retire", "Not built"))
    # the existing kernels are untouched: the new ones are kernels of their own
    for name in ("gcre_frontend.hip", "gcre_sets.hip", "gcre_subsample.hip"):
        assert "k_seq_" not in open(os.path.join(ROOT, "geneticscre_amd", "csrc", name)).read()


def test_signatures():
    st = inspect.signature(api.JoinExec.sequential_tests).parameters
    assert list(st) == ["self", "sets", "rows", "signs", "hits", "max_perms", "seed", "strata"]
    assert [st[k].default for k in list(st)[3:]] == [None, 20, 10**6, 0, None]
    assert list(inspect.signature(api.JoinExec.sequential_launches).parameters) == ["self"]
    assert list(inspect.signature(report.permutation_masks).parameters) == ["n_cases", "n_ctrls", "perms", "seed", "strata"]
    assert list(inspect.signature(report.sequential_reference).parameters) == ["null", "obs", "valid", "hits", "max_perms"]
    assert list(inspect.signature(report.sequential_columns).parameters) == ["seq", "valid"]
    sp = inspect.signature(report.score_paths).parameters
    names = list(sp)
    assert names[-1] == "family_inference"                    # (tests/test_family_host.py requires it to stay last)
    i = names.index("sequential")
    assert names[i:i + 2] == ["sequential", "sequential_hits"] and names[i - 1] == "stability_cuts"
    assert [sp[k].default for k in ("sequential", "sequential_hits")] == [0, 20]
    assert "sequential" not in inspect.signature(report.gwaspa).parameters
    doc = " ".join(report.score_paths.__doc__.split())
    assert "SEQUENTIAL_COLUMNS" in doc and "no family-wise version" in doc


def test_value_errors_come_before_the_library(monkeypatch):
    ex = api.JoinExec.__new__(api.JoinExec)
    ex.num_cases, ex.num_ctrls = 3, 2
    monkeypatch.setattr(api, "_feature_lib", lambda f: None)
    with pytest.raises(ValueError, match="signs: one sign per member of every set"):
        api.JoinExec.sequential_tests(ex, [[0, 1]], np.zeros((4, 5), np.int8), signs=[[1]])
    with pytest.raises(ValueError, match="strata: one id per patient"):
        api.JoinExec.sequential_tests(ex, [[0, 1]], np.zeros((4, 5), np.int8), strata=[0, 1])
    with pytest.raises(ValueError, match="sequential: the limit of permutations must not be negative"):
        report.score_paths(["A"], ["A"], np.zeros((1, 5), np.int8), 3, 2, sequential=-1)
