"""The plain-C++ parts of the one-call pipeline (csrc/gcre_pipeline.h; gcre_host_pipeline.hip is built on them): the top-k merge,
the hints of levels 4 and 5, the sets a permutation window is planned for, the window rounding, a device's shard, the hub's
round tag and the hub itself -- the C++ itself, driven by tests/native/pipeline_main.cpp under the address and
undefined-behaviour sanitizers as a child process.  No GPU needed."""
from __future__ import annotations

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pipeline_main.cpp")
CSRC = os.path.join(ROOT, "geneticscre_amd", "csrc")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pipeline") / "pipeline_main")
    # the sanitizers' runtimes are linked statically: the program then runs whatever the environment it inherits preloads
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-pthread", SRC, "-o", out], check=True)
    return out


def run(prog, tmp_path, lines):
    path = tmp_path / "case.txt"
    path.write_text("\n".join(" ".join(str(x) for x in ln) for ln in lines) + "\n")
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout}\n{r.stderr}"
    return r.stdout.splitlines()


# ---- merge_candidates ---------------------------------------------------------------------------------------------------
SENTINEL = "row -inf -1 -1 0 0"
#        score path src trg cases ctrls
FIVE = [(9.0, 40, 1, 2, 3, 4), (8.0, 30, 5, 6, 7, 8), (5.0, 20, 9, 10, 11, 12), (5.0, 10, 13, 14, 15, 16), (1.0, 50, 17, 18, 19, 20)]
MERGE_CASES = [
    ("no candidates", [], [SENTINEL]),
    ("fewer than top_k", [(1.5, 7, 1, 2, 3, 4), (2.5, 3, 5, 6, 7, 8)], [SENTINEL, "row 1.5 1 2 3 4", "row 2.5 5 6 7 8"]),
    # two candidates tied at the cut: the smaller joined-path ordinal stays
    ("tie at the cut", FIVE, ["row 5 13 14 15 16", "row 8 5 6 7 8", "row 9 1 2 3 4"]),
]


@pytest.mark.parametrize("name,cands,want", MERGE_CASES, ids=[c[0] for c in MERGE_CASES])
def test_merge_candidates(prog, tmp_path, name, cands, want):
    assert run(prog, tmp_path, [("case", "merge"), ("top_k", 3)] + [("cand", *c) for c in cands]) == want


def test_merge_does_not_depend_on_how_the_candidates_arrive(prog, tmp_path):
    """Three devices' tables, handed over in any order, give the bytes of one table."""
    one = run(prog, tmp_path, [("case", "merge"), ("top_k", 3)] + [("cand", *c) for c in FIVE])
    for tables in ([[3, 0], [4], [1, 2]], [[2], [4, 1, 3], [0]], [[4, 3], [2, 1], [0]]):
        order = [i for t in tables for i in t]
        assert run(prog, tmp_path, [("case", "merge"), ("top_k", 3)] + [("cand", *FIVE[i]) for i in order]) == one


# ---- the hints of levels 4 and 5 ----------------------------------------------------------------------------------------
# a level of 3 uids with counts {2, 0, 1} at locations {5, 9, 7}; level 4 adds data rows {4, 2, 6}
HINT_CASES = [
    # method, signs, want added, want second
    (1, [1, -1, 0], "00000004 00000002 00000006", "00000005 00000006 00000007"),
    (2, [1, -1, 0], "00000004 80000002 80000006", "00000005 00000006 80000007"),     # a sign other than 1 sets bit 31
    (2, [1, -1], "00000004 80000002 00000006", "00000005 00000006 00000007"),        # a sign index at or past n_signs does not
    (1, [1, -1], "00000004 00000002 00000006", "00000005 00000006 00000007"),
    (2, [], "00000004 00000002 00000006", "00000005 00000006 00000007"),
]


@pytest.mark.parametrize("method,signs,added,second", HINT_CASES, ids=[f"m{c[0]}-{len(c[1])}signs" for c in HINT_CASES])
def test_hint_builders(prog, tmp_path, method, signs, added, second):
    got = run(prog, tmp_path, [("case", "hints"), ("method", method), ("counts", 2, 0, 1), ("locations", 5, 9, 7), ("signs", *signs),
                               ("data_inds", 4, 2, 6), ("l2_signs", *signs)])
    assert got == ["added " + added, "second " + second]


# ---- set_rows, the window, the shard, the tag ---------------------------------------------------------------------------
@pytest.mark.parametrize("path_length,want", [(1, "11 13 5"), (2, "11 13 5 8"), (3, "11 13 5 8 7"), (4, "11 13 5 8 7"), (5, "11 13 5 8 7")])
def test_set_rows(prog, tmp_path, path_length, want):
    """The two data matrices, then the joined paths of levels 1a, 2 and 3 as far as the path length goes (a negative count
    joins nothing; level 1b keeps no set)."""
    got = run(prog, tmp_path, [("case", "set_rows"), ("path_length", path_length), ("data1_rows", 11), ("data2_rows", 13),
                               ("level", 0, 2, -1, 3), ("level", 1, 100), ("level", 2, 4, 0, 4), ("level", 3, 7)])
    assert got == ["set_rows " + want]


def test_window_perms_rounding(prog, tmp_path):
    got = run(prog, tmp_path, [("case", "window"), ("kall", 2300), ("perms", 1, 2047, 2048, 2049, 2300, 2301)])
    assert got == ["window 2048 2048 2048 2048 2300 2300"]


def test_shard_bounds(prog, tmp_path):
    assert run(prog, tmp_path, [("case", "shard"), ("total", 7), ("world", 3)]) == ["shard 0 2", "shard 2 4", "shard 4 7"]


def test_hub_tag_is_distinct(prog, tmp_path):
    got = run(prog, tmp_path, [("case", "tags"), ("levels", 6), ("k0", 0, 2048), ("rounds", 3)])
    assert len(got) == 36 and len({ln.split()[-1] for ln in got}) == 36
    assert {tuple(ln.split()[1:4]) for ln in got} == {(str(lv), str(k0), str(r)) for lv in range(6) for k0 in (0, 2048) for r in range(3)}


# ---- ExchangeHub, three threads -----------------------------------------------------------------------------------------
def test_hub_reduce_returns_the_max_to_all(prog, tmp_path):
    got = run(prog, tmp_path, [("case", "hub"), ("mode", "reduce")])
    want = ["2 -0.5 2", "4 1.5 2", "6 3.5 0"]
    assert got == [f"t{t} round {r} rc 0 {want[r]}" for t in range(3) for r in range(3)] + ["failed 0 timed_out 0"]


def test_hub_another_tag_fails_the_round_for_all(prog, tmp_path):
    got = run(prog, tmp_path, [("case", "hub"), ("mode", "tag")])
    assert got == [f"t{t} round 0 rc 1" for t in range(3)] + ["failed 1 timed_out 0"]


def test_hub_times_out_when_a_thread_is_absent(prog, tmp_path):
    got = run(prog, tmp_path, [("case", "hub"), ("mode", "timeout")])      # timeout_s = 0.05
    assert got == ["t0 round 0 rc 1", "t1 round 0 rc 1", "failed 1 timed_out 1"]


def test_hub_fail_releases_the_waiters(prog, tmp_path):
    got = run(prog, tmp_path, [("case", "hub"), ("mode", "fail")])         # the default deadline: 300 s
    assert got == ["t0 round 0 rc 1", "t1 round 0 rc 1", "failed 1 timed_out 0"]


# ---- where the pipeline lives -------------------------------------------------------------------------------------------
def test_the_pipeline_has_a_translation_unit_of_its_own():
    from geneticscre_amd import build
    assert "gcre_host_pipeline.hip" in build.SOURCES and "gcre_pipeline.h" in build.HEADERS
    host = open(os.path.join(CSRC, "gcre_host.hip")).read()
    pipeline = open(os.path.join(CSRC, "gcre_host_pipeline.hip")).read()
    for entry in ("int gcre_process_paths(", "int gcre_process_paths_devices(", "gcre_rccl_selftest(", "gcre_rccl_collectives("):
        assert entry not in host and entry in pipeline
    header = open(os.path.join(CSRC, "gcre_host.h")).read()
    assert "#include <rccl" not in header and "#include <dlfcn.h>" not in header and "struct RcclApi" not in header
    plain = open(os.path.join(CSRC, "gcre_pipeline.h")).read()
    includes = [ln.split()[1] for ln in plain.splitlines() if ln.startswith("#include")]
    assert '"../../include/gcre_hip.h"' in includes and not [i for i in includes if "hip/" in i or "gcre_kernels" in i or "gcre_host" in i]
