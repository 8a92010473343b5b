"""Device-side clumping (gcre_clump_sets), the part that needs no GPU: the C++ order checks themselves
(tests/native/clump_main.cpp under the address and undefined-behaviour sanitizers, one case per run), ``report.hit_sets`` on
a hand-worked example against ``results_table``, the declared interface, the defaults, the ValueErrors that come before
the library is touched -- and the generator of the GPU tests' cases with what those tests need of it, asserted on
``report.clump_rows`` alone."""
from __future__ import annotations

import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from geneticscre_amd import api, report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "clump_main.cpp")
OK, ERR_RANGE, ERR_ARG = 0, -2, -4   # include/gcre_hip.h


# ---- the cases of tests/test_gpu_clump.py ---------------------------------------------------------------------------------

SHAPES = [(1, 145, 70, 40, 300),    # seed, patients, cases, gene rows, sets: the split dword inside the only chunk
          (2, 67, 37, 24, 200),
          (3, 1100, 517, 60, 400)]  # two chunks, the split in the first


def make_case(seed, patients, cases, R, S):
    """R gene rows at carrier probability 0.08, the first 3 at 0.4; S sets of 1-5 members drawn from rows 3..R-1, with
    probability 0.6 one member replaced by a strong row; the walk order a permutation from the same seed."""
    rng = np.random.default_rng(seed)
    rows = (rng.random((R, patients)) < 0.08).astype(np.int8)
    rows[:3] = rng.random((3, patients)) < 0.4
    sets = []
    for _ in range(S):
        m = rng.integers(3, R, int(rng.integers(1, 6)))
        if rng.random() < 0.6:
            m[int(rng.integers(0, len(m)))] = int(rng.integers(0, 3))
        sets.append(m.tolist())
    order = np.random.default_rng(seed).permutation(S)
    return dict(n=patients, nc=cases, rows=rows, sets=sets, order=order)


_CACHE = {}


def counts_of(case):
    """(size, both) of a case by report.overlap_reference, computed once."""
    key = id(case["rows"])
    if key not in _CACHE:
        _CACHE[key] = (case, report.overlap_reference(case["sets"], case["rows"], case["nc"], case["n"] - case["nc"]))
    return _CACHE[key][1]


def reference(case, r, measure="jaccard", patients="all", order=None):
    """report.clump_rows fed from report.overlap_reference: (clump, lead, value, shared, size)."""
    size, both = counts_of(case)
    order = case["order"] if order is None else np.asarray(order, np.int64)
    c, l, v, sh = report.clump_rows(order, size, lambda a, b: both[np.asarray(a)][:, np.asarray(b)], r, measure, patients)
    return c, l, v, sh, size


def pair_value(case, j, k, measure="jaccard", patients="all"):
    size, both = counts_of(case)
    tot = size[:, 0].astype(np.int64) + (size[:, 1] if patients == "all" else 0)
    bo = int(both[j, k, 0]) + (int(both[j, k, 1]) if patients == "all" else 0)
    den = tot[j] + tot[k] - bo if measure == "jaccard" else min(tot[j], tot[k])
    return bo / den if den > 0 else 0.0


def chains(case, r):
    """Pairs (j, k) at jaccard / all: j is no lead, k comes later and lies in another clump, value(j, k) >= r, and k's lead
    comes after j -- a kernel that lets an absorbed candidate lead gets k wrong."""
    c, l, _, _, _ = reference(case, r)
    order = case["order"]
    pos = np.empty(len(order), np.int64)
    pos[order] = np.arange(len(order))
    out = 0
    for a, j in enumerate(order.tolist()):
        if l[j] == j:
            continue
        for k in order[a + 1:].tolist():
            if c[k] != c[j] and pos[l[k]] > a and pair_value(case, j, k) >= r:
                out += 1
    return out


def check_generator(case):
    """What the GPU tests need of a case, on the reference's result alone: a changed generator fails here instead of
    shrinking those tests."""
    lead_count = lambda res: int((res[1] == np.arange(len(res[1]))).sum())
    assert lead_count(reference(case, 0.8)) > 64                    # several rounds
    assert lead_count(reference(case, 0.5, "containment")) < 64     # one round of leads
    v = reference(case, 0.5)[2]
    assert (v == 0.5).sum() >= 1                                    # a member exactly at r
    assert chains(case, 0.8) >= 1


@pytest.mark.parametrize("shape", SHAPES, ids=[f"seed{s[0]}" for s in SHAPES])
def test_generated_cases_hold_what_the_gpu_tests_need(shape):
    check_generator(make_case(*shape))


# ---- the C++ checks -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("clump") / "clump_main")
    # the sanitizers' runtimes are linked statically: the program then runs whatever the environment it inherits preloads
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", SRC, "-o", out], check=True)
    return out


def run_case(prog, path, env=None, **case):
    base = dict(n_sets=4, set_off=[0, 1, 3, 5, 6], members=[0, 1, 2, 0, -1, 3])   # set 2 has an NA member
    base.update(case)
    lines = [(k, *v) if isinstance(v, (list, tuple)) else (k, v) for k, v in base.items() if v is not None]
    with open(path, "w") as f:
        f.write("\n".join(" ".join(str(x) for x in ln) for ln in lines) + "\n")
    e = dict(os.environ)
    e.pop("GCRE_CLUMP_MAX_MB", None)
    e.update(env or {})
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=60, env=e)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout}\n{r.stderr}"
    out = dict(ln.split(" ", 1) for ln in r.stdout.splitlines())
    assert set(out) == {"rule", "order", "bytes"}
    return out


def test_a_good_case_passes_every_check(prog, tmp_path):
    out = run_case(prog, tmp_path / "c.txt", order=[3, 0, 1], r=1.0, measure=1, patients=1)
    assert out == {"rule": "0 ", "order": "0 ", "bytes": "0  32768"}
    out = run_case(prog, tmp_path / "c.txt", order=[], r=1e-300)      # nothing to walk; the smallest r
    assert out["rule"] == "0 " and out["order"] == "0 "
    out = run_case(prog, tmp_path / "c.txt", order=[1, 0, 3], n_order=2)   # only the declared length is read
    assert out["order"] == "0 "


RULES = [(dict(r=0.0), "r must be > 0 and <= 1, not 0.000000"), (dict(r=-0.5), "r must be > 0 and <= 1"),
         (dict(r=1.0000001), "r must be > 0 and <= 1"), (dict(r="nan"), "r must be > 0 and <= 1, not nan"),
         (dict(r="inf"), "r must be > 0 and <= 1"),
         (dict(measure=2), "measure must be 0 (jaccard) or 1 (containment), not 2"), (dict(measure=-1), "measure must be"),
         (dict(patients=2), "patients must be 0 (all) or 1 (cases), not 2"), (dict(patients=-1), "patients must be")]


@pytest.mark.parametrize("change,text", RULES, ids=[str(c) for c, _ in RULES])
def test_rules_refused(prog, tmp_path, change, text):
    out = run_case(prog, tmp_path / "c.txt", order=[0], **change)
    assert out["rule"].startswith(f"{ERR_ARG} clump_sets: ") and text in out["rule"], out
    assert out["order"] == "0 "


ORDERS = [(dict(order=[0, 4]), ERR_RANGE, "clump_sets: order[1] = 4 out of range (4 sets)"),
          (dict(order=[-1]), ERR_RANGE, "clump_sets: order[0] = -1 out of range (4 sets)"),
          (dict(order=[3, 1, 3]), ERR_ARG, "clump_sets: order[2] = 3 is listed twice"),
          (dict(order=[0, 2]), ERR_ARG, "clump_sets: order[1] = 2 names a set with an NA member"),
          (dict(order=None, n_order=2), ERR_ARG, "clump_sets: bad order (a negative length or a NULL array)"),
          (dict(order=[0], n_order=-1), ERR_ARG, "clump_sets: bad order (a negative length or a NULL array)"),
          (dict(order=[2, 2, 9]), ERR_ARG, "clump_sets: order[0] = 2 names a set with an NA member")]   # the first fault


@pytest.mark.parametrize("change,code,message", ORDERS, ids=[str(c) for c, _, _ in ORDERS])
def test_orders_refused(prog, tmp_path, change, code, message):
    out = run_case(prog, tmp_path / "c.txt", **change)
    assert out["order"] == f"{code} {message}" and out["rule"] == "0 "


def test_the_size_bound_is_read_per_call(prog, tmp_path):
    big = 1 << 26
    assert run_case(prog, tmp_path / "c.txt", order=None, n_order=big, row_bytes=512)["bytes"] == "0  32768"
    out = run_case(prog, tmp_path / "c.txt", order=None, n_order=big + 1, row_bytes=512)["bytes"]
    assert out.startswith(f"{ERR_ARG} clump_sets: {big + 1} rows of 512 bytes exceed GCRE_CLUMP_MAX_MB")
    env = {"GCRE_CLUMP_MAX_MB": "0.001"}     # 1048 bytes: 8 rows of 128 bytes, not 9
    assert run_case(prog, tmp_path / "c.txt", env, order=None, n_order=8)["bytes"] == "0  0.001"
    assert run_case(prog, tmp_path / "c.txt", env, order=None, n_order=9)["bytes"].startswith(f"{ERR_ARG} clump_sets: 9 rows of 128")
    assert run_case(prog, tmp_path / "c.txt", {"GCRE_CLUMP_MAX_MB": "-5"}, order=[0])["bytes"].startswith(f"{ERR_ARG} ")
    assert run_case(prog, tmp_path / "c.txt", {"GCRE_CLUMP_MAX_MB": "1e9"}, order=[0])["bytes"] == "0  65536"


# ---- hit_sets ---------------------------------------------------------------------------------------------------------------

def test_hit_sets_by_hand():
    """Ents A B C D (data1 rows 0-3), Ents2 B C D (data2 rows 0-2, stacked rows 4-6), relations A->B, B->C, C->D.  Five hits
    over three lengths; one names slot 1 twice.  The sets come in the order of results_table's rows."""
    ents = (np.array([10, 11, 12, 13]), ["A", "B", "C", "D"])
    ents2 = (np.array([11, 12, 13]), ["B", "C", "D"])
    rs, rt = np.array([0, 1, 2], np.int32), np.array([1, 2, 3], np.int32)
    tables = {"1b": (None, np.arange(3, dtype=np.int32).reshape(3, 1)), "2": (None, np.stack([rs, rt], axis=1)),
              "3": (np.stack([rs, rt], axis=1), rt.reshape(-1, 1))}
    frames = {"rels_data": {"srcuid": ents[0]}, "rels_data2": {"srcuid": ents2[0]},
              "rels": {"srcuid": ents[0][rs], "trguid": ents[0][rt], "sign": np.ones(3, np.int32)}}
    i32 = lambda *x: np.array(x, np.int32)
    hits = lambda score, src, trg: api.Hits(len(score), 10, True, np.array(score, np.float64), np.arange(len(score)),
                                            i32(*src), i32(*trg), i32(*[1] * len(score)), i32(*[1] * len(score)))
    found = {1: hits([5.0, 1.0], [0, 0], [0, 2]),      # B, D: ranks 0 and 2 in Ents2
             2: hits([4.0], [2], [2]),                 # C -> D
             3: hits([6.0, 3.0], [1, 0], [0, 1])}      # B -> C -> B (slot 1 twice), A -> B -> C
    nulls = {1: np.array([2.0, 4.5], np.float32), 2: np.array([3.0, 5.0], np.float32), 3: np.array([1.0, 7.0], np.float32)}
    off, members = report.hit_sets(found, tables, 4, 3, nulls=nulls)
    assert off.dtype == np.int64 and members.dtype == np.int32
    got = [members[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
    # p = 0: 5.0; p = 0.5: 6.0, 4.0, 3.0 by score; p = 1: 1.0
    assert got == [[4], [1, 2], [2, 3], [0, 1, 2], [6]]
    table = report.results_table({f"lst{L}": found[L].as_join_result(nulls[L]) for L in found}, 3, frames, ents, ents2)
    assert table["Scores"].tolist() == [5.0, 6.0, 4.0, 3.0, 1.0] and table["Pvalues"].tolist() == [0.0, 0.5, 0.5, 0.5, 1.0]
    names = ents[1] + ents2[1]                                  # the rows of vstack(data1, data2)
    assert list(table["Paths"]) == ["B", "B -> C -> B", "C -> D", "A -> B -> C", "D"]
    for path, m in zip(table["Paths"], got):
        assert set(path.split(" -> ")) == {names[x] for x in m}
    # without nulls: no p-values, the order results_table gives the same lists without permutations
    off0, members0 = report.hit_sets(found, tables, 4, 3)
    got0 = [members0[off0[i]:off0[i + 1]].tolist() for i in range(len(off0) - 1)]
    none = report.results_table({f"lst{L}": found[L].as_join_result(np.zeros(0, np.float32)) for L in found}, 3, frames,
                                ents, ents2)
    assert none["Scores"].tolist() == [6.0, 5.0, 4.0, 3.0, 1.0]
    assert got0 == [[1, 2], [4], [2, 3], [0, 1, 2], [6]]
    # a list that overflowed has no records: no sets; nothing at all: one offset
    over = dict(found)
    over[3] = api.Hits(7, 10, False, *[np.zeros(0, t) for t in (np.float64, np.int64, np.int32, np.int32, np.int32, np.int32)])
    off1, members1 = report.hit_sets(over, tables, 4, 3, nulls=nulls)
    assert [members1[off1[i]:off1[i + 1]].tolist() for i in range(len(off1) - 1)] == [[4], [2, 3], [6]]
    off2, members2 = report.hit_sets({3: over[3]}, tables, 4, 3)
    assert off2.tolist() == [0] and len(members2) == 0
    with pytest.raises(ValueError, match="slot 3 lies outside the 3 slots"):
        report.hit_sets(found, tables, 3, 3)


# ---- the interface ------------------------------------------------------------------------------------------------------

def test_interface_is_declared():
    header = open(os.path.join(ROOT, "include", "gcre_hip.h")).read()
    assert re.search(r"#define GCRE_ABI_VERSION 4\b", header)
    flat = " ".join(header.split())
    assert ("int gcre_clump_sets(gcre_ctx* ctx, const gcre_set_input* in, const int64_t* order, int64_t n_order, double r, "
            "int measure, int patients, int32_t* size, int64_t* clump, int64_t* lead, double* value, int32_t* shared);") in flat
    assert "int64_t gcre_clump_launches(const gcre_ctx* ctx);" in flat
    assert {"gcre_clump_sets", "gcre_clump_launches"} <= set(api.EXPORTS)
    parent, needs, _, binds = api._FEATURES["clump"]
    assert parent == "overlap" and set(needs) == set(binds) == {"gcre_clump_sets", "gcre_clump_launches"}
    assert len(binds["gcre_clump_sets"][1]) == 12
    from geneticscre_amd import build
    assert "gcre_clump.hip" in build.SOURCES and "gcre_clumporder.h" in build.HEADERS
    lib = api._clump_lib()                                   # loads without a GPU
    assert lib.gcre_abi_version() == 4 and lib.gcre_clump_launches(None) == -1
    assert isinstance(api.JoinExec.clump_launches, property)


def test_defaults_change_nothing():
    sig = inspect.signature(report.gwaspa).parameters
    assert sig["clump_significant"].default is False
    assert inspect.signature(report.clump_paths).parameters["on_device"].default is False
    cs = inspect.signature(api.JoinExec.clump_sets).parameters
    assert [cs[k].default for k in ("r", "measure", "patients")] == [0.5, "jaccard", "all"]
    assert list(cs)[:4] == ["self", "sets", "rows", "order"]
    assert list(inspect.signature(report.hit_sets).parameters)[:4] == ["found", "tables", "n_genes", "n_genes2"]


def test_value_errors_come_before_the_library(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(api, "load_library", touched)
    monkeypatch.setattr(api, "_feature_lib", touched)
    monkeypatch.setattr(api, "_clump_lib", touched)
    rows = np.zeros((2, 5), np.int8)
    for kw, text in ((dict(r=0.0), "r must be > 0 and <= 1"), (dict(r=1.5), "r must be"), (dict(r=float("nan")), "r must be"),
                     (dict(measure="dice"), "measure must be 'jaccard' or 'containment'"),
                     (dict(patients="controls"), "patients must be 'all' or 'cases'")):
        with pytest.raises(ValueError, match=text):
            api.JoinExec.clump_sets(None, [[0], [1]], rows, [0, 1], **kw)
        with pytest.raises(ValueError, match=text):      # the same ones as clump_rows
            report.clump_rows([0, 1], np.ones((2, 2)), None, **{"r": 0.5, **kw})
    data = np.zeros((3, 6), np.int32)
    net = (np.arange(3), ["a", "b", "c"], np.array([0]), np.array([1]), np.array([1]))
    for kw in (dict(clump_significant=True), dict(clump_significant=True, clump=0.5),
               dict(clump_significant=True, significant=0.05)):
        with pytest.raises(ValueError, match="clump_significant: needs both clump"):
            report.gwaspa(["a", "b", "c"], data, 3, 3, net, **kw)
    with pytest.raises(ValueError, match="r must be > 0 and <= 1"):
        report.gwaspa(["a", "b", "c"], data, 3, 3, net, clump_significant=True, clump=0.0, significant=0.05)
