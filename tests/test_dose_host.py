"""Multi-hit set tests, host side: ``report.dose_sets`` and ``report.pair_sets`` on hand-worked examples;
``dose_sets`` folded by ``report.prefix_reference`` against a per-patient count taken literally; the argument checks in C++
(csrc/gcre_dose.h) and the slabs they hand to csrc/gcre_prefix.h, driven by tests/native/dose_main.cpp under the address and
undefined-behaviour sanitizers as a child process and compared with their restatement in Python here; the interface.  No GPU
needed."""
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
SRC = os.path.join(ROOT, "tests", "native", "dose_main.cpp")
OK, ERR_ARG = 0, -4   # include/gcre_hip.h
NAN = float("nan")


# ---- dose_sets, pair_sets: hand-worked -------------------------------------------------------------------------------

#            patient  0  1  2  3  4  5
ROWS = np.array([[1, 1, 0, 0, 1, 0],      # gene 0
                 [1, 0, 1, 0, 1, 0],      # gene 1
                 [1, 1, 1, 0, 0, 0],      # gene 2
                 [0, 0, 0, 0, 1, 1]])     # gene 3
SETS = [[0, 1, 2], [3, 3], [1, -1], [0, 3]]
SIGNS = [[1, -1, 1], [1, 1], [1, 1], [1, -1]]


def test_dose_sets_method_1_hand_worked():
    """Set 0: counts 3 2 2 0 2 0.  Set 1 lists gene 3 twice: counts 0 0 0 0 2 2.  Set 2 has an NA member.  Set 3: patient 4
    carries both members: counts 1 1 0 0 2 1.  Level 3 is above the size of sets 1 and 3: an empty row."""
    rows, sets, signs, owner = report.dose_sets(SETS, ROWS, SIGNS, [1, 2, 3], False)
    assert rows.dtype == np.int8 and owner.dtype == np.int64
    assert owner.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]
    assert sets == [[0], [1], [2], [3], [4], [5], [-1], [-1], [-1], [6], [7], [8]]
    assert signs == [[1]] * 12
    assert rows.tolist() == [[1, 1, 1, 0, 1, 0], [1, 1, 1, 0, 1, 0], [1, 0, 0, 0, 0, 0],     # set 0: >= 1, 2, 3 (signs ignored)
                             [0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0],     # set 1: the duplicate counts twice
                             [1, 1, 0, 0, 1, 1], [0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0]]     # set 3
    # level 1 is the union
    assert rows[0].tolist() == (ROWS[[0, 1, 2]].sum(axis=0) > 0).astype(int).tolist()


def test_dose_sets_method_2_hand_worked():
    """The two halves count apart.  Set 0: (+) genes 0, 2: counts 2 2 1 0 1 0; (-) gene 1: 1 0 1 0 1 0.  Set 3: patient 4
    carries the (+) member and the (-) member: one hit in either half, no level-2 row has it."""
    rows, sets, signs, owner = report.dose_sets(SETS, ROWS, SIGNS, [1, 2], True)
    assert owner.tolist() == [0, 0, 1, 1, 2, 2, 3, 3]
    assert sets == [[0, 1], [2, 3], [4, 5], [6, 7], [-1, -1], [-1, -1], [8, 9], [10, 11]]
    assert signs == [[1, -1]] * 8
    assert rows.tolist() == [[1, 1, 1, 0, 1, 0], [1, 0, 1, 0, 1, 0],      # set 0, level 1: (+), (-)
                             [1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0],      # set 0, level 2
                             [0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0],      # set 1, level 1: both members (+)
                             [0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0],      # set 1, level 2
                             [1, 1, 0, 0, 1, 0], [0, 0, 0, 0, 1, 1],      # set 3, level 1
                             [0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]]      # set 3, level 2
    # without signs everything is (+): the (-) rows are empty and the (+) rows are method 1's
    r2, s2, _, _ = report.dose_sets(SETS, ROWS, None, [1, 2], True)
    r1, _, _, _ = report.dose_sets(SETS, ROWS, None, [1, 2], False)
    assert np.array_equal(r2[0::2], r1) and not r2[1::2].any() and s2 == sets
    # the (off, members) form with flat signs
    off, mem = np.array([0, 3, 5, 7, 9]), np.array([0, 1, 2, 3, 3, 1, -1, 0, 3], np.int32)
    r3, s3, g3, o3 = report.dose_sets((off, mem), ROWS, np.concatenate(SIGNS), [1, 2], True)
    assert np.array_equal(r3, rows) and s3 == sets and g3 == signs and o3.tolist() == owner.tolist()
    with pytest.raises(ValueError, match="signs: one sign per member of every set"):
        report.dose_sets(SETS, ROWS, [[1]], [1], True)
    empty = report.dose_sets([], ROWS, None, [1, 2], False)
    assert empty[0].shape == (0, 6) and empty[1] == [] and empty[3].tolist() == []


def test_pair_sets():
    assert report.pair_sets([4, 2, 9]) == [[4, 2], [4, 9], [2, 9]]
    assert report.pair_sets([5]) == [] and report.pair_sets([]) == []
    assert len(report.pair_sets(range(12))) == 66


# ---- dose_sets + prefix_reference against the definition -------------------------------------------------------------


def literal(method, nc, sets, signs, levels, rows, VT, masks):
    """gcre_score_sets_dose taken literally: one set, one patient, one level and one permutation at a time."""
    n = rows.shape[1]
    cell = lambda a, b: float(VT[a][b]) if a < VT.shape[0] and b < VT.shape[1] else -1.0       # (the device's padding)
    vmax = lambda a, b: cell(b, a) if cell(a, b) < cell(b, a) else cell(a, b)                  # std::max(VT[a][b], VT[b][a])

    def observed(P, N):
        v = cell(sum(q < nc for q in P), sum(q >= nc for q in P))
        return v + cell(sum(q >= nc for q in N), sum(q < nc for q in N)) if method == 2 else v

    def null(P, N, case):
        pp = sum(q in case for q in P)
        with np.errstate(over="ignore", invalid="ignore"):
            if method == 1:
                f = np.float32(cell(pp, len(P) - pp))
            else:
                pn = sum(q in case for q in N)
                f = np.float32(vmax(pp, len(P) - pp) + vmax(len(N) - pn, pn))
        return f if f > 0 else np.float32(0)           # NaN and negatives fold to 0

    out = []
    for s, m in enumerate(sets):
        sg = [1] * len(m) if signs is None else signs[s]
        if any(r < 0 for r in m):
            out.append((NAN, -1, -1, None))
            continue
        hits_pos, hits_neg = [0] * n, [0] * n
        for q in range(n):
            for r, g in zip(m, sg):
                if rows[r][q]:
                    if method == 2 and g == -1:
                        hits_neg[q] += 1
                    else:
                        hits_pos[q] += 1
        score, best = NAN, -1
        T = [np.float32(0)] * len(masks)
        for k, level in enumerate(levels):
            P = {q for q in range(n) if hits_pos[q] >= level}
            N = {q for q in range(n) if hits_neg[q] >= level}
            v = observed(P, N)
            if v == v and (best < 0 or v > score):
                score, best = v, k
            for r, mk in enumerate(masks):
                x = null(P, N, set(np.flatnonzero(mk).tolist()))
                if x > T[r]:
                    T[r] = x
        n_ge = sum(float(t) >= score for t in T) if best >= 0 else 0
        out.append((score, best, n_ge, T))
    return out


@pytest.mark.parametrize("method", [1, 2])
def test_dose_sets_folded_equal_the_definition(method):
    """A few hundred random small problems: the level sets scored by the restatement the set tests are held to
    (tests/test_sets_host.restate) and folded by ``prefix_reference``, against the loops above."""
    from test_sets_host import restate
    rng = np.random.default_rng(200 + method)
    seen_multi = 0
    for trial in range(150):
        nc, nt = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        n, K = nc + nt, int(rng.integers(1, 6))
        n_rows = int(rng.integers(2, 8))
        rows = (rng.random((n_rows, n)) < 0.45).astype(np.int8)
        VT = small_table(n, n, trial)
        VT[rng.random(VT.shape) < 0.15] = np.nan
        VT[rng.random(VT.shape) < 0.1] *= -1
        sets = [rng.integers(0, n_rows, int(rng.integers(1, 7))).tolist() for _ in range(3)]     # with repeats
        if trial % 5 == 0:
            sets[1][0] = -1
        signs = None if trial % 4 == 1 else [rng.choice([1, -1], len(x)).tolist() for x in sets]
        levels = sorted(rng.choice(np.arange(1, 8), int(rng.integers(1, 5)), replace=False).tolist())
        masks = np.zeros((K, n), bool)
        for r in range(K):
            masks[r, rng.permutation(n)[:nc]] = True
        lrows, lsets, lsigns, owner = report.dose_sets(sets, rows, signs, levels, method == 2)
        with np.errstate(over="ignore", invalid="ignore"):
            want, wnull, _ = restate(method, nc, nt, lsets, lrows, lsigns, VT, masks)
        valid = [all(r >= 0 for r in m) for m in sets]
        lnull = np.array([w if w is not None else np.full(K, np.nan, np.float32) for w in wnull], np.float32).reshape(len(lsets), K)
        ref = report.prefix_reference([w["score"] for w in want], lnull, owner, len(sets), valid)
        lit = literal(method, nc, sets, signs, levels, rows != 0, VT, masks)
        for s, (score, best, n_ge, T) in enumerate(lit):
            assert ref["best_step"][s] == best and ref["n_ge"][s] == n_ge, (trial, s)
            assert (np.isnan(score) and np.isnan(ref["score"][s])) or np.float64(score).view(np.uint64) == ref["score"][s].view(np.uint64)
            if T is None:
                assert np.isnan(ref["null_max"][s]).all()
            else:
                assert np.array_equal(np.array(T, np.float32).view(np.uint32), ref["null_max"][s].view(np.uint32)), (trial, s)
            seen_multi += best > 0
    assert seen_multi > 10                            # (the best level is not always the first)


# ---- the C++ itself --------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dose") / "dose_main")
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


def set_bytes(rows, method, w32p, kpad, want_null):
    return rows * method * w32p * 4.0 + (kpad * 4.0 if want_null else 0.0)


def plan(sets, levels, method, w32p, kpad, want_null, max_mb, slab_sets):
    """The slabs and block tables of a call restated: csrc/gcre_prefix.h's rule with len(levels) rows for every valid set --
    the lines tests/native/dose_main.cpp prints after its check."""
    L = len(levels)
    lines = ["packed %x" % sum(m << (4 * i) for i, m in enumerate(levels))]
    V = sum(all(r >= 0 for r in m) for m in sets)
    slabs, cur, size = [], [0, 0, 0], 0.0
    b = set_bytes(L, method, w32p, kpad, want_null)
    for v in range(V):
        if cur[1] > 0 and (size + b > max_mb * 1048576.0 or (slab_sets > 0 and cur[1] >= slab_sets)):
            slabs.append(cur)
            cur, size = [v, 0, 0], 0.0
        cur[1] += 1
        cur[2] += L
        size += b
    if cur[1]:
        slabs.append(cur)
    for v0, nv, rows in slabs:
        waves = [(e, L, e * L) for e in range(nv)] + [(-1, 0, 0)] * (-nv % 4)      # equal lengths: the stable sort keeps the order
        lines += [f"slab {v0} {nv} {rows}", "order " + " ".join(map(str, range(nv))),
                  "waves " + " ".join(f"{a} {b} {c}" for a, b, c in waves)]
    return lines


def case_of(sets, levels, **more):
    off = np.concatenate([[0], np.cumsum([len(x) for x in sets])]).astype(int).tolist()
    case = [("n_sets", len(sets)), ("set_off", off), ("members", [r for x in sets for r in x])]
    if levels is not None:
        case.append(("levels", list(levels)))
    return case + list(more.items())


def test_native_slabs_equal_the_python_restatement(prog, tmp_path):
    rng = np.random.default_rng(61)
    for trial in range(6):
        sizes = rng.permutation([1, 2, 3, 5, 9, 16, 17, 40, 1, 33, 7])[:int(rng.integers(1, 12))].tolist()
        sets = [rng.integers(0, 50, k).tolist() for k in sizes]
        if trial % 2 == 1:
            sets[len(sets) // 2][0] = -1                                         # an NA set takes no slot
        levels = [[1], [2], [15], [1, 2, 3], [1, 15], list(range(1, 16))][trial]
        method, w32p, kpad = 1 + trial % 2, 4 * int(rng.integers(1, 5)), 2048
        per = set_bytes(len(levels), method, w32p, kpad, 1)
        for want_null, max_mb, slab_sets in [(0, 1024, 0), (1, 1024, 0), (0, 1024, 1), (1, 1024, 5), (0, 1024, 3),
                                            (1, 5.5 * per / 1048576.0, 0), (1, 2 * per / 1048576.0, 3)]:
            out = run_case(prog, tmp_path, case_of(sets, levels, method=method, w32p=w32p, kpad=kpad, want_null=want_null,
                                                   max_mb=max_mb, slab_sets=slab_sets, iterations=100))
            assert out[0] == "check 0 "
            assert out[1:] == plan(sets, levels, method, w32p, kpad, want_null, max_mb, slab_sets), (trial, want_null, max_mb, slab_sets)
            valid = sum(all(r >= 0 for r in m) for m in sets)
            if slab_sets == 1:
                assert sum(ln.startswith("slab ") for ln in out) == valid
            if max_mb == 5.5 * per / 1048576.0:                                  # five and a half sets fit: five to a slab
                assert sum(ln.startswith("slab ") for ln in out) == -(-valid // 5)


def test_native_plan_written_out(prog, tmp_path):
    """Five valid sets and an NA set at levels 1, 2, 4: three rows each, the last block of four waves partial."""
    sets = [[0, 1, 2], [3], [1, 1, 1], [-1, 2], [4, 5, 6], [0, 1, 2, 3, 4]]
    out = run_case(prog, tmp_path, case_of(sets, [1, 2, 4]))
    assert out == ["check 0 ", "packed 421", "slab 0 5 15", "order 0 1 2 3 4",
                   "waves 0 3 0 1 3 3 2 3 6 3 3 9 4 3 12 -1 0 0 -1 0 0 -1 0 0"]
    out = run_case(prog, tmp_path, case_of(sets, [3, 4, 7, 8], slab_sets=2))
    assert out[1:] == ["packed 8743", "slab 0 2 8", "order 0 1", "waves 0 4 0 1 4 4 -1 0 0 -1 0 0",
                       "slab 2 2 8", "order 0 1", "waves 0 4 0 1 4 4 -1 0 0 -1 0 0",
                       "slab 4 1 4", "order 0", "waves 0 4 0 -1 0 0 -1 0 0 -1 0 0"]
    assert run_case(prog, tmp_path, case_of(sets, list(range(1, 16))))[1] == "packed fedcba987654321"


LIST = [("n_sets", 3), ("set_off", [0, 3, 4, 9]), ("members", [0, 1, 2, 5, 3, 3, 1, 0, 2])]
LV = [("levels", [1, 2, 3])]
W = "score_sets_dose: "
CHECK_CASES = [
    ("accepted", LIST + LV, OK, ""),
    ("one level", LIST + [("levels", [15])], OK, ""),
    ("fifteen levels", LIST + [("levels", list(range(1, 16)))], OK, ""),
    ("no sets", [("n_sets", 0), ("set_off", [0])] + LV, OK, ""),
    ("NULL dose_out", LIST + LV + [("have_out", 0)], ERR_ARG, W + "NULL argument (dose_out)"),
    ("NULL dose_out comes first", LIST + [("have_out", 0), ("n_levels", 0)], ERR_ARG, W + "NULL argument (dose_out)"),
    ("no level", LIST + [("levels", []), ("n_levels", 0)], ERR_ARG, W + "n_levels = 0: 1 .. 15 levels"),
    ("a negative number of levels", LIST + LV + [("n_levels", -2)], ERR_ARG, W + "n_levels = -2: 1 .. 15 levels"),
    ("sixteen levels", LIST + [("levels", list(range(1, 16))), ("n_levels", 16)], ERR_ARG, W + "n_levels = 16: 1 .. 15 levels"),
    ("NULL levels", LIST + [("n_levels", 2)], ERR_ARG, W + "NULL argument (levels)"),
    ("level 0", LIST + [("levels", [0, 1])], ERR_ARG, W + "level 0 (index 0) is outside 1 .. 15"),
    ("level 16", LIST + [("levels", [1, 2, 16])], ERR_ARG, W + "level 16 (index 2) is outside 1 .. 15"),
    ("a negative level", LIST + [("levels", [-3])], ERR_ARG, W + "level -3 (index 0) is outside 1 .. 15"),
    ("a level twice", LIST + [("levels", [1, 2, 2])], ERR_ARG, W + "the levels are not strictly ascending (2 after 2)"),
    ("descending levels", LIST + [("levels", [3, 1])], ERR_ARG, W + "the levels are not strictly ascending (1 after 3)"),
    ("the first fault in list order", LIST + [("levels", [5, 4, 16])], ERR_ARG, W + "the levels are not strictly ascending (4 after 5)"),
    # 3 levels x 1 half x 8 dwords x 4 bytes = 96 bytes
    ("one set above the bound", LIST + LV + [("max_mb", 0.00009)], ERR_ARG,
     W + "the 3 level rows of set 0 take 96 bytes: above GCRE_PREFIX_MAX_MB = 0.000090"),
    ("the bound itself", LIST + LV + [("max_mb", 96 / 1048576.0)], OK, ""),
    ("both halves count", LIST + LV + [("max_mb", 96 / 1048576.0), ("method", 2)], ERR_ARG,
     W + "the 3 level rows of set 0 take 192 bytes: above GCRE_PREFIX_MAX_MB = 0.000092"),
    ("the null_max row counts", LIST + LV + [("max_mb", 0.005), ("want_null", 1)], ERR_ARG,
     W + "the 3 level rows of set 0 take 8288 bytes: above GCRE_PREFIX_MAX_MB = 0.005000"),
    ("fewer levels fit", LIST + [("levels", [2]), ("max_mb", 0.00009)], OK, ""),
    ("the first valid set names the refusal", [("n_sets", 2), ("set_off", [0, 1, 3]), ("members", [-1, 3, 4]), ("max_mb", 0.00001)] + LV,
     ERR_ARG, W + "the 3 level rows of set 1 take 96 bytes: above GCRE_PREFIX_MAX_MB = 0.000010"),
    ("the bound is not asked of an NA set", [("n_sets", 1), ("set_off", [0, 2]), ("members", [0, -1]), ("max_mb", 0.00001)] + LV, OK, ""),
    ("nor without permutations", LIST + LV + [("max_mb", 0), ("iterations", 0)], OK, ""),
]


@pytest.mark.parametrize("name,case,code,message", CHECK_CASES, ids=[c[0] for c in CHECK_CASES])
def test_argument_checks_under_sanitizers(prog, tmp_path, name, case, code, message):
    assert run_case(prog, tmp_path, case)[0] == f"check {code} {message}"


# ---- the interface ---------------------------------------------------------------------------------------------------


def test_interface_is_declared():
    header = open(os.path.join(ROOT, "include", "gcre_hip.h")).read()
    assert re.search(r"#define GCRE_ABI_VERSION 4\b", header)      # additions only
    assert re.search(r"#define GCRE_DOSE_MAX_LEVEL 15\b", header) and api.DOSE_MAX_LEVEL == 15
    flat = " ".join(re.sub(r"/\*.*?\*/", " ", header, flags=re.S).split())
    assert ("int gcre_score_sets_dose(gcre_ctx* ctx, const gcre_set_input* in, const int32_t* levels, int32_t n_levels, "
            "gcre_set_score* out, int64_t cap, int64_t* n_out, gcre_dose_score* dose_out , float* family_max , float* null_max , "
            "double* level_scores );") in flat
    assert "int64_t gcre_dose_launches(const gcre_ctx* ctx);" in flat
    assert ("typedef struct { double score; int64_t n_ge; int32_t best_index, best_level, levels; int32_t cases_pos, ctrls_pos, "
            "cases_neg, ctrls_neg; int32_t pad; } gcre_dose_score;") in flat
    assert {"gcre_score_sets_dose", "gcre_dose_launches"} <= set(api.EXPORTS)
    declared = set(re.findall(r"\b(gcre_[a-z0-9_]+)\s*\(", header))
    assert declared == set(api.EXPORTS)
    parent, needs, _, binds = api._FEATURES["dose"]
    assert parent == "sets" and set(needs) == set(binds) == {"gcre_score_sets_dose", "gcre_dose_launches"}
    assert len(binds["gcre_score_sets_dose"][1]) == 11
    assert api.DOSE_SCORE.itemsize == 48 and api.DOSE_SCORE.names == (       # sizeof(gcre_dose_score), static_assert'ed in the host stage
        "score", "n_ge", "best_index", "best_level", "levels", "cases_pos", "ctrls_pos", "cases_neg", "ctrls_neg", "pad")
    assert [api.DOSE_SCORE.fields[k][1] for k in api.DOSE_SCORE.names] == [0, 8, 16, 20, 24, 28, 32, 36, 40, 44]
    from geneticscre_amd import build
    assert {"gcre_dose.hip", "gcre_host_steps.hip"} <= set(build.SOURCES) and "gcre_dose.h" in build.HEADERS
    kernels = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_kernels.h")).read()
    assert "struct DoseArgs" in kernels and "launch_dose_rows(" in kernels
    # one host file for this entry and gcre_score_sets_prefix: each hands the stage its own counter and nobody else's, and the
    # stage counts through what it was handed alone
    host = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_host_steps.hip")).read()
    assert "static_assert(sizeof(gcre_dose_score) == 48" in host
    entry = {m.group(1): m.group(2) for m in re.finditer(r"\nint (gcre_score_sets_\w+)\(.*?\) \{\n(.*?)\n\}\n", host, flags=re.S)}
    assert set(entry) == {"gcre_score_sets_prefix", "gcre_score_sets_dose"}
    assert "&gcre_ctx::dose_launches" in entry["gcre_score_sets_dose"] and "prefix_launches" not in entry["gcre_score_sets_dose"]
    assert "&gcre_ctx::prefix_launches" in entry["gcre_score_sets_prefix"] and "dose_launches" not in entry["gcre_score_sets_prefix"]
    stage = host[:host.index('extern "C"')]
    assert "int64_t& launches = c->*counter;" in stage and "_launches" not in stage
    rows = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_step_rows.h")).read()
    assert "if (d.ok()) counter++;" in rows and "_launches" not in rows
    lib = api._dose_lib()                                    # loads without a GPU
    assert lib.gcre_abi_version() == 4 and lib.gcre_dose_launches(None) == -1
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.20" in design and "k_dose_rows" in design


def test_signatures():
    dt = inspect.signature(api.JoinExec.dose_tests).parameters
    assert list(dt) == ["self", "sets", "rows", "signs", "levels", "family", "null", "level_scores"]
    assert [dt[k].default for k in ("signs", "levels", "family", "null", "level_scores")] == [None, (1, 2), False, False, False]
    assert list(inspect.signature(api.JoinExec.dose_launches).parameters) == ["self"]
    assert list(inspect.signature(report.dose_sets).parameters) == ["sets", "rows", "signs", "levels", "signed"]
    assert list(inspect.signature(report.pair_sets).parameters) == ["rows"]
    mh = inspect.signature(report.multi_hit_test).parameters
    assert list(mh) == ["sets", "genes", "data", "n_cases", "n_ctrls", "signed", "names", "levels", "threshold", "n_permutations",
                        "strata", "seed", "device"]
    assert mh["levels"].default == (1, 2, 3) and mh["signed"].default is False and mh["n_permutations"].default == 100
    vt = list(inspect.signature(report.variable_threshold_test).parameters)
    assert [p for p in mh if p != "levels"] == vt             # the order variable_threshold_test takes the ones they share
    assert report.MULTI_HIT_COLUMNS == ["Sets", "Genes", "Scores", "NominalPvalues", "BestLevel", "BestCases", "BestControls",
                                        "MultiHitScores", "MultiHitPvalues", "MultiHitFamilyPvalues"]


BAD_LEVELS = [([], "levels: 1 to 15 levels"), (list(range(1, 17)), "levels: 1 to 15 levels"), ([[1, 2]], "levels: 1 to 15 levels"),
              (3, "levels: 1 to 15 levels"), ([0, 1], "levels: every level in 1 .. 15"), ([1, 16], "levels: every level in 1 .. 15"),
              ([-1], "levels: every level in 1 .. 15"), ([1, 1], "levels: strictly ascending"), ([2, 1], "levels: strictly ascending"),
              ([1.5, 2], "levels: whole numbers")]


@pytest.mark.parametrize("levels,message", BAD_LEVELS, ids=[str(b[0]) for b in BAD_LEVELS])
def test_value_errors_come_before_the_library(monkeypatch, levels, message):
    ex = api.JoinExec.__new__(api.JoinExec)
    ex.num_cases, ex.num_ctrls, ex.iters = 3, 2, 4
    ex._h = None

    def no_library(*a):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(api, "_feature_lib", no_library)
    monkeypatch.setattr(api, "_dose_lib", no_library)
    monkeypatch.setattr(api, "load_library", no_library)
    rows = np.zeros((4, 5), np.int8)
    with pytest.raises(ValueError, match=re.escape(message)):
        api.JoinExec.dose_tests(ex, [[0, 1]], rows, levels=levels)
    with pytest.raises(ValueError, match="signs: one sign per member of every set"):
        api.JoinExec.dose_tests(ex, [[0, 1]], rows, signs=[[1]], levels=levels)        # the marshaller's own refusal comes first


def test_good_levels_are_marshalled():
    assert api._dose_levels((1, 2)).tolist() == [1, 2] and api._dose_levels((1, 2)).dtype == np.int32
    assert api._dose_levels(np.arange(1, 16)).tolist() == list(range(1, 16))
    assert api._dose_levels([3.0, 4.0, 7.0, 8.0]).tolist() == [3, 4, 7, 8]
    assert api._dose_levels([15]).flags["C_CONTIGUOUS"]
