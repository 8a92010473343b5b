"""Variable-threshold set tests, host side: ``report.prefix_sets`` and ``report.threshold_order`` on
hand-written examples; ``report.prefix_reference`` on a hand-worked case and against the definition taken literally; the host
plan in C++ (csrc/gcre_prefix.h: steps, argument checks, slabs, sorted order, block table), driven by
tests/native/prefix_main.cpp under the address and undefined-behaviour sanitizers as a child process and compared with its
restatement in Python here; the interface.  No GPU needed."""
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
SRC = os.path.join(ROOT, "tests", "native", "prefix_main.cpp")
OK, ERR_ARG = 0, -4   # include/gcre_hip.h
NAN = float("nan")


# ---- prefix_sets, threshold_order ------------------------------------------------------------------------------------


def test_prefix_sets_written_out():
    sets, signs = [[4, 2, 7], [5], [3, 3, -1, 0]], [[1, -1, 1], [-1], [1, 1, -1, -1]]
    st, sg, owner = report.prefix_sets(sets, signs, None)
    assert st == [[4], [4, 2], [4, 2, 7], [5], [3], [3, 3], [3, 3, -1], [3, 3, -1, 0]]
    assert sg == [[1], [1, -1], [1, -1, 1], [-1], [1], [1, 1], [1, 1, -1], [1, 1, -1, -1]]
    assert owner.tolist() == [0, 0, 0, 1, 2, 2, 2, 2] and owner.dtype == np.int64
    # cuts: the last member always ends a step, whatever its flag
    st, sg, owner = report.prefix_sets(sets, None, [[0, 1, 0], [0], [1, 0, 0, 0]])
    assert st == [[4, 2], [4, 2, 7], [5], [3], [3, 3, -1, 0]] and sg is None and owner.tolist() == [0, 0, 1, 2, 2]
    # all zeros: one step per set, the full set
    st, _, owner = report.prefix_sets(sets, None, [[0, 0, 0], [0], [0, 0, 0, 0]])
    assert st == sets and owner.tolist() == [0, 1, 2]
    # the (off, members) form with flat signs and flat cuts
    off, mem = np.array([0, 3, 4, 8]), np.array([4, 2, 7, 5, 3, 3, -1, 0], np.int32)
    st, sg, owner = report.prefix_sets((off, mem), np.concatenate(signs), [0, 1, 0, 0, 1, 0, 0, 0])
    assert st == [[4, 2], [4, 2, 7], [5], [3], [3, 3, -1, 0]] and sg[1] == [1, -1, 1] and owner.tolist() == [0, 0, 1, 2, 2]
    with pytest.raises(ValueError, match="cuts: one flag per member of every set"):
        report.prefix_sets(sets, None, [[1, 1], [1], [1, 1, 1, 1]])
    with pytest.raises(ValueError, match="cuts: one flag per member of every set"):
        report.prefix_sets((off, mem), None, [1, 1, 1])
    assert report.prefix_sets([], None, None)[0] == []


def test_threshold_order_written_out():
    data = np.zeros((7, 6), int)
    for r, c in enumerate([3, 0, 5, 3, 1, 0, 2]):        # carrier totals by row
        data[r, :c] = 1
    order, cuts = report.threshold_order([2, 0, 5, 3, 1, 6], data)
    # totals 5 3 0 3 0 2 -> rows by (total, row): 1 5 | 6 | 0 3 | 2
    assert np.asarray([2, 0, 5, 3, 1, 6])[order].tolist() == [1, 5, 6, 0, 3, 2]
    assert cuts.tolist() == [0, 1, 1, 0, 1, 1] and cuts.dtype == np.uint8 and order.dtype == np.int64
    # genes of equal carrier total enter together: every step is "all genes with at most t carriers"
    st, _, _ = report.prefix_sets([np.asarray([2, 0, 5, 3, 1, 6])[order].tolist()], None, [cuts.tolist()])
    assert st == [[1, 5], [1, 5, 6], [1, 5, 6, 0, 3], [1, 5, 6, 0, 3, 2]]
    # a row listed twice keeps both positions next to one another; an NA gene goes last, a step of its own
    order, cuts = report.threshold_order([3, -1, 4, 3], data)
    assert order.tolist() == [2, 0, 3, 1] and cuts.tolist() == [1, 0, 1, 1]
    order, cuts = report.threshold_order([4], data)
    assert order.tolist() == [0] and cuts.tolist() == [1]
    order, cuts = report.threshold_order([], data)
    assert order.tolist() == [] and cuts.tolist() == []


# ---- prefix_reference: hand-worked -----------------------------------------------------------------------------------


def test_reference_hand_worked():
    """Three sets x six permutations, plus an NA set.  Set 0: steps (2.5, 4.0, 4.0): a tie, the smaller index wins.  Set 1: steps
    (NaN, 1.5): the NaN step is skipped but its null row still counts in the maximum.  Set 2: every step NaN.  Set 3: NA."""
    step_obs = [2.5, 4.0, 4.0, NAN, 1.5, NAN, NAN, NAN]
    step_set = [0, 0, 0, 1, 1, 2, 2, 3]
    step_null = np.array([[1.0, 4.5, 0.0, 3.0, 2.0, 0.5],      # set 0
                          [0.5, 1.0, 4.0, 3.5, 2.0, 0.0],
                          [0.0, 2.0, 1.0, 3.9, 5.0, 0.0],
                          [9.0, 0.0, 0.0, 1.0, 0.0, 1.5],      # set 1
                          [0.0, 1.5, 1.0, 2.0, 0.0, 1.4],
                          [1.0, 0.0, 2.0, 0.0, 0.0, 0.0],      # set 2
                          [0.0, 3.0, 1.0, 0.0, 0.0, 0.0],
                          [NAN] * 6], np.float32)              # set 3: what family_tests returns for an NA set
    ref = report.prefix_reference(step_obs, step_null, step_set, 4, [1, 1, 1, 0])
    assert ref["best_step"].tolist() == [1, 1, -1, -1]
    assert ref["score"][:2].tolist() == [4.0, 1.5] and np.isnan(ref["score"][2:]).all()
    want = np.array([[1.0, 4.5, 4.0, 3.9, 5.0, 0.5], [9.0, 1.5, 1.0, 2.0, 0.0, 1.5], [1.0, 3.0, 2.0, 0.0, 0.0, 0.0]], np.float32)
    assert np.array_equal(ref["null_max"][:3], want) and np.isnan(ref["null_max"][3]).all()
    assert ref["null_max"].dtype == np.float32 and ref["null_max"].shape == (4, 6)
    # set 0: 4.5, 4.0, 5.0 reach 4.0; set 1: 9.0, 1.5, 2.0, 1.5 reach 1.5; a NaN score counts nothing; NA: -1
    assert ref["n_ge"].tolist() == [3, 4, 0, -1] and ref["n_ge"].dtype == np.int64
    # no permutations
    none = report.prefix_reference(step_obs, np.zeros((8, 0), np.float32), step_set, 4, [1, 1, 1, 0])
    assert none["n_ge"].tolist() == [0, 0, 0, -1] and none["null_max"].shape == (4, 0) and none["best_step"].tolist() == [1, 1, -1, -1]


# ---- prefix_reference against the definition -------------------------------------------------------------------------


def literal(method, nc, sets, signs, cuts, rows, VT, masks):
    """gcre_score_sets_prefix taken literally: one set, one step and one permutation at a time, Python sets and loops."""
    n = rows.shape[1]
    cell = lambda a, b: float(VT[a][b]) if a < VT.shape[0] and b < VT.shape[1] else -1.0       # (the device's padding)
    vmax = lambda a, b: cell(b, a) if cell(a, b) < cell(b, a) else cell(a, b)                  # std::max(VT[a][b], VT[b][a])

    def unions(members, sg):
        P, N = set(), set()
        for r, g in zip(members, sg):
            (N if method == 2 and g == -1 else P).update(np.flatnonzero(rows[r]).tolist())
        return P, N

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
        ct = [1] * len(m) if cuts is None else cuts[s]
        if any(r < 0 for r in m):
            out.append((NAN, -1, -1, None))
            continue
        ends = [i for i in range(len(m)) if ct[i] or i + 1 == len(m)]
        score, best = NAN, -1
        T = [np.float32(0)] * len(masks)
        for k, i in enumerate(ends):
            P, N = unions(m[:i + 1], sg[:i + 1])
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
def test_reference_equals_the_definition(method):
    """A few hundred random small problems: the expanded step sets scored by the restatement the set tests are held to
    (tests/test_sets_host.restate) and folded by ``prefix_reference``, against the loops above."""
    from test_sets_host import restate
    rng = np.random.default_rng(180 + method)
    for trial in range(200):
        nc, nt = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        n, K = nc + nt, int(rng.integers(1, 6))
        n_rows = int(rng.integers(2, 8))
        rows = (rng.random((n_rows, n)) < 0.3).astype(np.int8)
        VT = small_table(n, n, trial)
        VT[rng.random(VT.shape) < 0.15] = np.nan
        VT[rng.random(VT.shape) < 0.1] *= -1
        sets = [rng.integers(0, n_rows, int(rng.integers(1, 6))).tolist() for _ in range(3)]
        if trial % 5 == 0:
            sets[1][0] = -1
        signs = None if trial % 4 == 1 else [rng.choice([1, -1], len(x)).tolist() for x in sets]
        cuts = None if trial % 3 == 0 else [(rng.random(len(x)) < 0.5).astype(int).tolist() for x in sets]
        masks = np.zeros((K, n), bool)
        for r in range(K):
            masks[r, rng.permutation(n)[:nc]] = True
        st, sg, owner = report.prefix_sets(sets, signs, cuts)
        with np.errstate(over="ignore", invalid="ignore"):
            want, wnull, _ = restate(method, nc, nt, st, rows, sg if sg is not None else [[1] * len(x) for x in st], VT, masks)
        valid = [all(r >= 0 for r in m) for m in sets]
        step_null = np.array([w if w is not None else np.full(K, np.nan, np.float32) for w in wnull], np.float32).reshape(len(st), K)
        ref = report.prefix_reference([w["score"] for w in want], step_null, owner, len(sets), valid)
        lit = literal(method, nc, sets, signs, cuts, rows != 0, VT, masks)
        for s, (score, best, n_ge, T) in enumerate(lit):
            assert ref["best_step"][s] == best and ref["n_ge"][s] == n_ge, (trial, s)
            assert (np.isnan(score) and np.isnan(ref["score"][s])) or np.float64(score).view(np.uint64) == ref["score"][s].view(np.uint64)
            if T is None:
                assert np.isnan(ref["null_max"][s]).all()
            else:
                assert np.array_equal(np.array(T, np.float32).view(np.uint32), ref["null_max"][s].view(np.uint32)), (trial, s)


# ---- the C++ itself --------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("prefix") / "prefix_main")
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


def set_bytes(steps, method, w32p, kpad, want_null):
    return steps * method * w32p * 4.0 + (kpad * 4.0 if want_null else 0.0)


def plan(sets, cuts, method, w32p, kpad, want_null, max_mb, slab_sets):
    """The host plan of csrc/gcre_prefix.h restated: the lines tests/native/prefix_main.cpp prints after its check."""
    off, end, members, pos = [0], [], [], 0
    for s, m in enumerate(sets):
        for i in range(len(m)):
            if cuts is None or cuts[s][i] or i + 1 == len(m):
                end.append(pos + i)
                members.append(i + 1)
        pos += len(m)
        off.append(len(end))
    lines = ["off " + " ".join(map(str, off)), ("end " + " ".join(map(str, end))).rstrip(),
             ("members " + " ".join(map(str, members))).rstrip()]
    vsteps = [off[s + 1] - off[s] for s, m in enumerate(sets) if all(r >= 0 for r in m)]
    slabs, cur, size = [], [0, 0, 0], 0.0
    for v, k in enumerate(vsteps):
        b = set_bytes(k, method, w32p, kpad, want_null)
        if cur[1] > 0 and (size + b > max_mb * 1048576.0 or (slab_sets > 0 and cur[1] >= slab_sets)):
            slabs.append(cur)
            cur, size = [v, 0, 0], 0.0
        cur[1] += 1
        cur[2] += k
        size += b
    if cur[1]:
        slabs.append(cur)
    for v0, nv, steps in slabs:
        mine = vsteps[v0:v0 + nv]
        row0 = np.concatenate([[0], np.cumsum(mine)]).tolist()
        order = sorted(range(nv), key=lambda e: (-mine[e], e))
        waves = [(e, mine[e], row0[e]) for e in order] + [(-1, 0, 0)] * (-nv % 4)
        lines += [f"slab {v0} {nv} {steps}", "order " + " ".join(map(str, order)),
                  "waves " + " ".join(f"{a} {b} {c}" for a, b, c in waves)]
    return lines


def case_of(sets, cuts, **more):
    off = np.concatenate([[0], np.cumsum([len(x) for x in sets])]).astype(int).tolist()
    case = [("n_sets", len(sets)), ("set_off", off), ("members", [r for x in sets for r in x])]
    if cuts is not None:
        case.append(("cut", [c for x in cuts for c in x]))
    return case + list(more.items())


@pytest.mark.parametrize("cut_kind", ["null", "zeros", "random"])
def test_native_plan_equals_the_python_restatement(prog, tmp_path, cut_kind):
    rng = np.random.default_rng(["null", "zeros", "random"].index(cut_kind) + 60)
    sizes = [1, 2, 3, 4, 5, 9, 17, 70, 1024, 1, 33, 1023, 7, 2]
    for trial in range(6):
        ks = sizes if trial == 0 else rng.permutation(sizes)[:int(rng.integers(1, 12))].tolist()
        sets = [rng.integers(0, 50, k).tolist() for k in ks]
        if trial % 2 == 1:
            sets[len(sets) // 2][0] = -1                                         # an NA set takes no slot
        cuts = None if cut_kind == "null" else [[0] * k for k in ks] if cut_kind == "zeros" else \
            [(rng.random(k) < 0.4).astype(int).tolist() for k in ks]
        method, w32p, kpad = 1 + trial % 2, 4 * int(rng.integers(1, 5)), 2048
        for want_null, max_mb, slab_sets in [(0, 1024, 0), (1, 1024, 0), (0, 1024, 1), (1, 1024, 5), (0, 1024, 3),
                                            (0, 0.07, 0), (1, 0.1, 0), (1, 0.1, 2)]:
            out = run_case(prog, tmp_path, case_of(sets, cuts, method=method, w32p=w32p, kpad=kpad, want_null=want_null,
                                                   max_mb=max_mb, slab_sets=slab_sets, iterations=100))
            if out[0] != "check 0 ":                                             # the largest set does not fit this bound
                steps = max(len(report.prefix_sets([m], None, None if cuts is None else [cuts[s]])[0]) for s, m in enumerate(sets)
                            if all(r >= 0 for r in m))
                assert set_bytes(steps, method, w32p, kpad, want_null) > max_mb * 1048576.0 and out[0].startswith("check -4 ")
                continue
            assert out[1:] == plan(sets, cuts, method, w32p, kpad, want_null, max_mb, slab_sets), (trial, want_null, max_mb, slab_sets)
            if slab_sets == 1:                                                   # a slab bound that cuts between every pair of sets
                assert sum(ln.startswith("slab ") for ln in out) == sum(all(r >= 0 for r in m) for m in sets)


def test_native_plan_written_out(prog, tmp_path):
    """Five valid sets of 3, 1, 3, 2 and 5 steps and an NA set: the blocks take them longest first, ties in input order."""
    sets = [[0, 1, 2], [3], [1, 1, 1], [-1, 2], [4, 5, 6], [0, 1, 2, 3, 4]]
    cuts = [[1, 1, 1], [0], [1, 1, 0], [1, 1], [0, 1, 0], [1, 1, 1, 1, 1]]
    out = run_case(prog, tmp_path, case_of(sets, cuts))
    assert out == ["check 0 ", "off 0 3 4 7 9 11 16", "end 0 1 2 3 4 5 6 7 8 10 11 12 13 14 15 16", "members 1 2 3 1 1 2 3 1 2 2 3 1 2 3 4 5",
                   "slab 0 5 14", "order 4 0 2 3 1", "waves 4 5 9 0 3 0 2 3 4 3 2 7 1 1 3 -1 0 0 -1 0 0 -1 0 0"]
    out = run_case(prog, tmp_path, case_of(sets, cuts, slab_sets=2))
    assert out[4:] == ["slab 0 2 4", "order 0 1", "waves 0 3 0 1 1 3 -1 0 0 -1 0 0",
                       "slab 2 2 5", "order 0 1", "waves 0 3 0 1 2 3 -1 0 0 -1 0 0",
                       "slab 4 1 5", "order 0", "waves 0 5 0 -1 0 0 -1 0 0 -1 0 0"]


LIST = [("n_sets", 3), ("set_off", [0, 3, 4, 9]), ("members", [0, 1, 2, 5, 3, 3, 1, 0, 2])]
W = "score_sets_prefix: "
CHECK_CASES = [
    ("accepted", LIST, OK, ""),
    ("no sets", [("n_sets", 0), ("set_off", [0])], OK, ""),
    ("NULL px_out", LIST + [("have_px", 0)], ERR_ARG, W + "NULL argument (px_out)"),
    ("NULL px_out without sets", [("n_sets", 0), ("set_off", [0]), ("have_px", 0)], ERR_ARG, W + "NULL argument (px_out)"),
    # 5 steps x 1 half x 8 dwords x 4 bytes = 160 bytes
    ("one set above the bound", LIST + [("max_mb", 0.00015)], ERR_ARG,
     W + "the 5 step rows of set 2 take 160 bytes: above GCRE_PREFIX_MAX_MB = 0.000150"),
    ("the bound itself", LIST + [("max_mb", 160 / 1048576.0)], OK, ""),
    ("both halves count", LIST + [("max_mb", 160 / 1048576.0), ("method", 2)], ERR_ARG,
     W + "the 3 step rows of set 0 take 192 bytes: above GCRE_PREFIX_MAX_MB = 0.000153"),      # the first set that does not fit
    ("the null_max row counts", LIST + [("max_mb", 0.005), ("want_null", 1)], ERR_ARG,
     W + "the 3 step rows of set 0 take 8288 bytes: above GCRE_PREFIX_MAX_MB = 0.005000"),
    ("fewer steps fit", LIST + [("max_mb", 0.0001), ("cut", [0] * 9)], OK, ""),
    ("the bound is not asked of an NA set", [("n_sets", 2), ("set_off", [0, 1, 6]), ("members", [0, 1, 2, -1, 3, 4]), ("max_mb", 0.0001)], OK, ""),
    ("nor without permutations", LIST + [("max_mb", 0), ("iterations", 0)], OK, ""),
]


@pytest.mark.parametrize("name,case,code,message", CHECK_CASES, ids=[c[0] for c in CHECK_CASES])
def test_argument_checks_under_sanitizers(prog, tmp_path, name, case, code, message):
    assert run_case(prog, tmp_path, case)[0] == f"check {code} {message}"


# ---- the interface ---------------------------------------------------------------------------------------------------


def test_interface_is_declared():
    header = open(os.path.join(ROOT, "include", "gcre_hip.h")).read()
    assert re.search(r"#define GCRE_ABI_VERSION 4\b", header)      # additions only
    flat = " ".join(re.sub(r"/\*.*?\*/", " ", header, flags=re.S).split())
    assert ("int gcre_score_sets_prefix(gcre_ctx* ctx, const gcre_set_input* in, const uint8_t* cut , gcre_set_score* out, int64_t cap, "
            "int64_t* n_out, gcre_prefix_score* px_out , float* family_max , float* null_max , double* step_scores );") in flat
    assert "int64_t gcre_prefix_launches(const gcre_ctx* ctx);" in flat
    assert "} gcre_prefix_score;" in flat
    assert {"gcre_score_sets_prefix", "gcre_prefix_launches"} <= set(api.EXPORTS)
    declared = set(re.findall(r"\b(gcre_[a-z0-9_]+)\s*\(", header))
    assert declared == set(api.EXPORTS)
    parent, needs, _, binds = api._FEATURES["prefix"]
    assert parent == "sets" and set(needs) == set(binds) == {"gcre_score_sets_prefix", "gcre_prefix_launches"}
    assert len(binds["gcre_score_sets_prefix"][1]) == 10
    assert api.PREFIX_SCORE.itemsize == 48 and api.PREFIX_SCORE.names == (
        "score", "n_ge", "best_step", "best_members", "steps", "cases_pos", "ctrls_pos", "cases_neg", "ctrls_neg")
    from geneticscre_amd import build
    assert "gcre_prefix.hip" in build.SOURCES and "gcre_prefix.h" in build.HEADERS
    kernels = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_kernels.h")).read()
    assert "struct PrefixArgs" in kernels and all(f"launch_prefix_{k}(" in kernels for k in ("rows", "pick", "null"))
    lib = api._prefix_lib()                                  # loads without a GPU
    assert lib.gcre_abi_version() == 4 and lib.gcre_prefix_launches(None) == -1
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.18" in design and "variable-threshold" in design.lower()


def test_signatures():
    pt = inspect.signature(api.JoinExec.prefix_tests).parameters
    assert list(pt) == ["self", "sets", "rows", "signs", "cuts", "family", "null", "steps"]
    assert [pt[k].default for k in ("signs", "cuts", "family", "null", "steps")] == [None, None, False, False, False]
    assert list(inspect.signature(api.JoinExec.prefix_launches).parameters) == ["self"]
    assert list(inspect.signature(report.prefix_sets).parameters) == ["sets", "signs", "cuts"]
    assert list(inspect.signature(report.prefix_reference).parameters) == ["step_obs", "step_null", "step_set", "n_sets", "valid"]
    assert list(inspect.signature(report.threshold_order).parameters) == ["set_genes", "data"]
    vt = list(inspect.signature(report.variable_threshold_test).parameters)
    bt = list(inspect.signature(report.burden_test).parameters)
    assert vt == [p for p in bt if p != "group"]               # the order burden_test takes the ones they share
    assert report.VARIABLE_THRESHOLD_COLUMNS == ["Sets", "Genes", "Scores", "NominalPvalues", "BestGenes", "BestThreshold",
                                                 "AdaptiveScores", "AdaptivePvalues", "AdaptiveFamilyPvalues"]
    assert list(inspect.signature(report.score_paths).parameters)[-1] == "family_inference"
    assert list(inspect.signature(report.gwaspa).parameters)[-1] == "patient_table"


def test_value_errors_come_before_the_library(monkeypatch):
    ex = api.JoinExec.__new__(api.JoinExec)
    ex.num_cases, ex.num_ctrls, ex.iters = 3, 2, 4
    monkeypatch.setattr(api, "_feature_lib", lambda f: None)
    monkeypatch.setattr(api, "_prefix_lib", lambda: None)
    rows = np.zeros((4, 5), np.int8)
    with pytest.raises(ValueError, match="cuts: one flag per member of every set"):
        api.JoinExec.prefix_tests(ex, [[0, 1]], rows, cuts=[[1]])
    with pytest.raises(ValueError, match="cuts: one flag per member of every set"):
        api.JoinExec.prefix_tests(ex, [[0, 1], [2]], rows, cuts=[[1, 0]])
    with pytest.raises(ValueError, match="cuts: one flag per member of every set"):
        api.JoinExec.prefix_tests(ex, (np.array([0, 2]), np.array([0, 1], np.int32)), rows, cuts=[1, 0, 1])
    with pytest.raises(ValueError, match="signs: one sign per member of every set"):
        api.JoinExec.prefix_tests(ex, [[0, 1]], rows, signs=[[1]])
