"""Conditional set scores, host side: ``report.residual_rows`` -- the definition of gcre_score_sets_given's
union rows -- on a hand-worked example per method; the index check of the entry (check_given_index, csrc/gcre_setlists.h), the
C++ itself, driven by tests/native/given_main.cpp under the address and undefined-behaviour sanitizers as a child process; the
interface, the keyword defaults and the ValueErrors that come before the library.  No GPU needed."""
from __future__ import annotations

import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from geneticscre_amd import api, report
from test_sets_host import restate_slabs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "given_main.cpp")
OK, ERR_RANGE, ERR_ARG = 0, -2, -4   # include/gcre_hip.h

# ---- the definition, hand-worked -------------------------------------------------------------------------------------
# patients 0-3 are cases, 4-7 controls
ROWS = np.array([[1, 1, 0, 0, 1, 0, 0, 0],     # g0
                 [0, 1, 1, 0, 0, 1, 0, 0],     # g1
                 [0, 0, 0, 1, 0, 0, 1, 0],     # g2
                 [1, 1, 1, 1, 1, 1, 1, 1],     # g3: everybody
                 [0, 0, 0, 0, 0, 0, 0, 1]])    # g4
SETS = [[0, 1], [1, 2], [3], [4], [0, -1], [0, 0, 1]]
SIGNS = [[1, -1], [1, -1], [1], [-1], [1, 1], [1, 1, -1]]
# (which, given): nothing given; a given set with a (+) and a (-) member; given == which; a superset; a disjoint set; an NA
# member; repeated members; and set 1 given set 0 next to set 0 given set 1 -- no chaining: C_0 is g0 | g1 in full
WHICH = [0, 0, 0, 0, 0, 4, 5, 1]
GIVEN = [-1, 1, 0, 2, 3, -1, 1, 0]


def bits(s):
    return np.array([c == "1" for c in s.replace(" ", "")], bool)


def test_residual_rows_method2_hand_worked():
    pos, neg, valid = report.residual_rows(SETS, ROWS, SIGNS, WHICH, GIVEN, 8, 2)
    assert valid.tolist() == [True, True, True, True, True, False, True, True]
    want_pos = ["1100 1000", "1000 1000", "0000 0000", "0000 0000", "1100 1000", "0000 0000", "1000 1000", "0000 0000"]
    want_neg = ["0110 0100", "0000 0000", "0000 0000", "0000 0000", "0110 0100", "0000 0000", "0000 0000", "0001 0010"]
    for i in range(len(WHICH)):
        assert np.array_equal(pos[i], bits(want_pos[i])), i
        assert np.array_equal(neg[i], bits(want_neg[i])), i
    # chained, entry 7 would have kept g1 & ~(1000 1000) = 0110 0100 in its (+) half
    assert not pos[7].any()
    # the counts as restate_slabs takes them: the (-) half counts the other way round
    got = restate_slabs(2, 4, 4, pos, neg, np.zeros((9, 9)), np.zeros((0, 8), bool))
    assert got["cases_pos"].tolist() == [2, 1, 0, 0, 2, 0, 1, 0] and got["ctrls_pos"].tolist() == [1, 1, 0, 0, 1, 0, 1, 0]
    assert got["cases_neg"].tolist() == [1, 0, 0, 0, 1, 0, 0, 1] and got["ctrls_neg"].tolist() == [2, 0, 0, 0, 2, 0, 0, 1]


def test_residual_rows_method1_hand_worked():
    for signs in (SIGNS, None):      # method 1 does not read them
        pos, neg, valid = report.residual_rows(SETS, ROWS, signs, WHICH, GIVEN, 8, 1)
        assert valid.tolist() == [True, True, True, True, True, False, True, True]
        want = ["1110 1100", "1000 1000", "0000 0000", "0000 0000", "1110 1100", "0000 0000", "1000 1000", "0001 0010"]
        for i in range(len(WHICH)):
            assert np.array_equal(pos[i], bits(want[i])), i
        assert not neg.any()


def test_residual_rows_defaults_and_refusals():
    pos, neg, valid = report.residual_rows(SETS, ROWS, SIGNS, None, None, 8, 2)      # every set, nothing given
    assert len(pos) == len(SETS) and valid.tolist() == [True, True, True, True, False, True]
    assert np.array_equal(pos[5], bits("1100 1000")) and np.array_equal(neg[3], bits("0000 0001"))
    p2, n2, _ = report.residual_rows(SETS, ROWS, SIGNS, None, [-1] * 6, 8, 2)
    assert np.array_equal(pos, p2) and np.array_equal(neg, n2)
    # columns beyond n are not patients
    wide = np.hstack([ROWS, np.ones((5, 3), int)])
    p3, n3, _ = report.residual_rows(SETS, wide, SIGNS, WHICH, GIVEN, 8, 2)
    p4, n4, _ = report.residual_rows(SETS, ROWS, SIGNS, WHICH, GIVEN, 8, 2)
    assert np.array_equal(p3, p4) and np.array_equal(n3, n4)
    with pytest.raises(ValueError, match="given set 4 has an NA member"):
        report.residual_rows(SETS, ROWS, SIGNS, [0], [4], 8, 2)
    with pytest.raises(ValueError, match="out of range"):
        report.residual_rows(SETS, ROWS, SIGNS, [6], [0], 8, 2)
    with pytest.raises(ValueError, match="out of range"):
        report.residual_rows(SETS, ROWS, SIGNS, [0], [-2], 8, 2)
    with pytest.raises(ValueError, match="2 entries for 1 scored sets"):
        report.residual_rows(SETS, ROWS, SIGNS, [0], [1, 1], 8, 2)


# ---- the index check, the C++ itself ------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("given") / "given_main")
    # the sanitizers' runtimes are linked statically: the program then runs whatever the environment it inherits preloads
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", SRC, "-o", out], check=True)
    return out


# three sets over four rows; set 2 has an NA member
LIST = dict(n_rows=4, n_sets=3, set_off=[0, 2, 3, 5], members=[0, 1, 2, 3, -1])
W = "score_sets_given: "
INDEX_CASES = [
    ("both lists", dict(n_which=4, cap=4, which=[0, 2, 1, 1], given=[-1, 0, 1, 0]), OK, ""),
    ("an NA set may be scored", dict(n_which=1, cap=1, which=[2], given=[1]), OK, ""),
    ("NULL which", dict(n_which=3, cap=3, given=[1, 0, -1]), OK, ""),
    ("NULL given", dict(n_which=2, cap=5, which=[1, 1]), OK, ""),
    ("both NULL", dict(n_which=3, cap=3), OK, ""),
    ("no entries", dict(n_which=0, cap=0, which=[], given=[]), OK, ""),
    ("negative length", dict(n_which=-1, cap=3, which=[0], given=[0]), ERR_ARG,
     W + "bad index list (a negative length, or NULL `which` with a length other than n_sets)"),
    ("NULL which, another length", dict(n_which=2, cap=3, given=[0, 0]), ERR_ARG,
     W + "bad index list (a negative length, or NULL `which` with a length other than n_sets)"),
    ("which below", dict(n_which=2, cap=2, which=[0, -1], given=[0, 0]), ERR_RANGE, W + "which[1] = -1 out of range (3 sets)"),
    ("which above", dict(n_which=2, cap=2, which=[3, 0]), ERR_RANGE, W + "which[0] = 3 out of range (3 sets)"),
    ("given below", dict(n_which=2, cap=2, which=[0, 0], given=[-1, -2]), ERR_RANGE,
     W + "given[1] = -2 out of range (3 sets, -1 = none)"),
    ("given above", dict(n_which=3, cap=3, given=[0, 3, 0]), ERR_RANGE, W + "given[1] = 3 out of range (3 sets, -1 = none)"),
    ("given NA set", dict(n_which=2, cap=2, which=[0, 1], given=[1, 2]), ERR_ARG,
     W + "given[1] = set 2 has an NA member: its carriers are not known"),
    ("no room", dict(n_which=3, cap=2, which=[0, 1, 0]), ERR_RANGE, W + "3 entries, room for 2 records (out of range)"),
    ("range before room", dict(n_which=3, cap=2, which=[0, 9, 0]), ERR_RANGE, W + "which[1] = 9 out of range (3 sets)"),
]


@pytest.mark.parametrize("name,case,code,message", INDEX_CASES, ids=[c[0] for c in INDEX_CASES])
def test_index_check_under_sanitizers(prog, tmp_path, name, case, code, message):
    lines = [(k, *v) if isinstance(v, list) else (k, v) for k, v in {**LIST, **case}.items()]
    path = tmp_path / "case.txt"
    path.write_text("\n".join(" ".join(str(x) for x in ln) for ln in lines) + "\n")
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout}\n{r.stderr}"
    assert r.stdout.splitlines() == [f"check {code} {message}"]


# ---- the interface ---------------------------------------------------------------------------------------------------


def test_interface_is_declared():
    header = open(os.path.join(ROOT, "include", "gcre_hip.h")).read()
    assert re.search(r"#define GCRE_ABI_VERSION 4\b", header)      # additions only
    flat = " ".join(header.split())
    assert ("int gcre_score_sets_given(gcre_ctx* ctx, const gcre_set_input* in, const int64_t* which, const int64_t* given, "
            "int64_t n_which, gcre_set_score* out, int64_t cap, int64_t* n_out, float* family_max);") in flat
    assert "int64_t gcre_given_launches(const gcre_ctx* ctx);" in flat
    assert {"gcre_score_sets_given", "gcre_given_launches"} <= set(api.EXPORTS)
    parent, needs, _, binds = api._FEATURES["given"]
    assert parent == "sets" and set(needs) == set(binds) == {"gcre_score_sets_given", "gcre_given_launches"}
    assert len(binds["gcre_score_sets_given"][1]) == 9
    from geneticscre_amd import build
    assert "gcre_given.hip" in build.SOURCES
    kernels = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_kernels.h")).read()
    assert "launch_set_residual(" in kernels and "struct SetResidualArgs" in kernels
    lib = api._given_lib()                                   # loads without a GPU
    assert lib.gcre_abi_version() == 4 and lib.gcre_given_launches(None) == -1
    assert isinstance(api.JoinExec.given_launches, property)


def test_defaults_change_nothing():
    ss = inspect.signature(api.JoinExec.score_sets).parameters
    assert list(ss) == ["self", "sets", "rows", "signs", "family", "given", "which"]
    assert ss["given"].default is None and ss["which"].default is None and ss["family"].default is False
    cp = inspect.signature(report.clump_paths).parameters
    assert cp["exec_"].default is None and cp["table"].default is None
    assert cp["exec_"].kind is inspect.Parameter.KEYWORD_ONLY and cp["table"].kind is inspect.Parameter.KEYWORD_ONLY
    assert cp["conditional"].default is False and cp["on_device"].default is False
    gw = inspect.signature(report.gwaspa).parameters
    assert [gw[k].default for k in ("clump", "clump_conditional", "significant", "clump_significant")] == [None, False, None, False]
    assert list(inspect.signature(report.residual_rows).parameters) == ["sets", "rows", "signs", "which", "given", "n", "method"]
    assert "residual columns for hits are not built" not in report.gwaspa.__doc__
    assert report.RESIDUAL_COLUMNS == ["ResidualScores", "ResidualCases", "ResidualControls", "ResidualPvalues"]


def test_value_errors_come_before_the_library(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched")
    for name in ("load_library", "_feature_lib", "_sets_lib", "_given_lib"):
        monkeypatch.setattr(api, name, touched)
    rows = np.zeros((4, 5), np.int8)
    sets = [[0, 1], [2], [3, -1]]
    off, members = np.array([0, 2, 3, 5], np.int64), np.array([0, 1, 2, 3, -1], np.int32)
    for form in (sets, (off, members)):
        for kw, text in ((dict(which=[0, 3]), r"which: a set index outside 0\.\.2"),
                         (dict(which=[-1]), "which: a set index outside"),
                         (dict(given=[0, 0, 3]), r"given: a set index outside -1\.\.2"),
                         (dict(given=[-2, 0, 0]), "given: a set index outside"),
                         (dict(given=[0, 1]), "given: 2 entries for 3 scored sets"),
                         (dict(which=[0], given=[0, 1]), "given: 2 entries for 1 scored sets"),
                         (dict(which=[0, 1], given=[1, 2]), "given: a given set has an NA member")):
            with pytest.raises(ValueError, match=text):
                api.JoinExec.score_sets(None, form, rows, **kw)
    with pytest.raises(ValueError, match="signs: one sign per member of every set"):
        api.JoinExec.score_sets(None, sets, rows, [[1, 1], [1], [1]], given=[0, 0, 0])
    with pytest.raises(ValueError, match="signs: one sign per member of every set"):
        api.JoinExec.score_sets(None, (off, members), rows, [1, 1, 1], which=[0])
