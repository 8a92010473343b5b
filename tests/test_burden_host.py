"""Burden tests of per-patient weights, host side: ``report.burden_reference`` -- the definition of
gcre_patient_burden -- on a hand-worked example; ``report.burden_table``; the argument check of the entry
(check_burden_args, csrc/gcre_setlists.h), the C++ itself, driven by tests/native/burden_main.cpp under the address and
undefined-behaviour sanitizers as a child process; the interface and the ValueErrors that come before the library.  No GPU
needed."""
from __future__ import annotations

import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

from geneticscre_amd import api, report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "burden_main.cpp")
OK, ERR_ASSERT, ERR_ARG = 0, -1, -4   # include/gcre_hip.h
BIG = 2**31 - 1

# ---- the definition, hand-worked -------------------------------------------------------------------------------------
# patients 0-3 are cases, 4-7 controls
WEIGHTS = np.array([[1, 0, 2, 3, 0, 1, 0, 0],          # observed 6 of 7
                    [0, 0, 0, 0, 0, 0, 0, 0],          # a row of zeros
                    [BIG, 0, 0, 0, BIG, 0, 0, 1],      # the largest weight there is: sums beyond 32 bits
                    [1, 1, 0, 0, 1, 1, 0, 0]])         # 0/1: ties
# bit q = patient q: the cases themselves; the controls; patients 0, 2, 5, 7; patients 0, 1, 4, 5 (and a stray bit 20)
MASKS = np.array([[0b00001111], [0b11110000], [0b10100101], [0b00110011 | (1 << 20)]], dtype=np.uint64)


def test_reference_hand_worked():
    r = report.burden_reference(WEIGHTS, MASKS, 4)
    assert r["total"].tolist() == [7, 0, 2 * BIG + 1, 4] and r["observed"].tolist() == [6, 0, BIG, 2]
    assert r["null"].dtype == np.int64
    assert r["null"].tolist() == [[6, 1, 4, 2], [0, 0, 0, 0], [BIG, BIG + 1, BIG + 1, 2 * BIG], [2, 2, 2, 4]]
    assert r["n_ge"].tolist() == [1, 4, 4, 4] and r["n_le"].tolist() == [4, 4, 1, 3]
    assert r["n_ge"][3] + r["n_le"][3] > 4                         # a tie counts in both tails
    assert r["planes"].tolist() == [2, 0, 31, 1] and r["planes"].dtype == np.int32
    assert r["p_upper"].tolist() == [0.25, 1.0, 1.0, 1.0] and r["p_lower"].tolist() == [1.0, 1.0, 0.25, 0.75]
    # [G][H][n] is flattened; no permutations: NaN
    r3 = report.burden_reference(WEIGHTS.reshape(2, 2, 8), MASKS, 4)
    assert all(np.array_equal(r3[k], r[k]) for k in r)
    r0 = report.burden_reference(WEIGHTS, np.zeros((0, 1), np.uint64), 4)
    assert r0["null"].shape == (4, 0) and r0["n_ge"].tolist() == [0] * 4 and np.isnan(r0["p_upper"]).all() and np.isnan(r0["p_lower"]).all()
    assert r0["observed"].tolist() == [6, 0, BIG, 2]
    # more than one word per mask
    wide = np.zeros((1, 70), np.int64)
    wide[0, [0, 63, 64, 69]] = [1, 2, 4, 8]
    m = np.array([[1 << 63, 1 << 5], [1, 1 | (1 << 6)]], dtype=np.uint64)     # patients 63 and 69; 0 and 64 (bit 70: nobody)
    assert report.burden_reference(wide, m, 1)["null"].tolist() == [[10, 5]]
    for bad in (np.array([[1, -1]]), np.array([[2**31, 0]])):
        with pytest.raises(ValueError, match="every weight must lie in"):
            report.burden_reference(bad, np.array([[1]], np.uint64), 1)
    with pytest.raises(ValueError, match="n_cases = 9"):
        report.burden_reference(WEIGHTS, MASKS, 9)


def test_burden_table_columns_and_order():
    r = report.burden_reference(WEIGHTS, MASKS, 4)
    t = report.burden_table(r, 4, 4)
    assert list(t.columns) == ["Group", "Sets", "Load", "CaseLoad", "ControlLoad", "CaseMean", "ControlMean", "PvalueUpper",
                               "PvalueLower", "NullMean", "NullSD", "Z"]
    assert t["Group"].tolist() == [0, 1, 2, 3] and np.isnan(t["Sets"]).all()
    assert t["Load"].tolist() == [7, 0, 2 * BIG + 1, 4] and t["CaseLoad"].tolist() == [6, 0, BIG, 2]
    assert t["ControlLoad"].tolist() == [1, 0, BIG + 1, 2]
    assert t["CaseMean"].tolist() == [1.5, 0.0, BIG / 4, 0.5] and t["ControlMean"].tolist() == [0.25, 0.0, (BIG + 1) / 4, 0.5]
    assert t["PvalueUpper"].tolist() == [0.25, 1.0, 1.0, 1.0] and t["PvalueLower"].tolist() == [1.0, 1.0, 0.25, 0.75]
    null = r["null"]
    assert np.array_equal(t["NullMean"].to_numpy(), null.mean(axis=1)) and np.array_equal(t["NullSD"].to_numpy(), null.std(axis=1))
    assert t["NullMean"].tolist()[0] == 3.25 and t["NullMean"].tolist()[3] == 2.5
    z = t["Z"].to_numpy()
    assert np.isnan(z[1]) and z[0] == (6 - 3.25) / null[0].std() and z[3] == (2 - 2.5) / null[3].std()
    # without the null: the nine columns; names and set counts
    plain = {k: v for k, v in r.items() if k != "null"}
    t2 = report.burden_table(plain, 4, 4, names=["a", "b", "c", "d"], group_sets=[3, 0, 2, 9])
    assert list(t2.columns) == report.BURDEN_COLUMNS and t2["Group"].tolist() == ["a", "b", "c", "d"] and t2["Sets"].tolist() == [3, 0, 2, 9]
    assert t2[report.BURDEN_COLUMNS[2:]].equals(t[report.BURDEN_COLUMNS[2:]])
    # unbalanced cohorts: the means divide by their own side
    t3 = report.burden_table(report.burden_reference(WEIGHTS, MASKS, 2), 2, 6)
    assert t3["CaseLoad"].tolist() == [1, 0, BIG, 2] and t3["CaseMean"].tolist() == [0.5, 0.0, BIG / 2, 1.0]
    assert t3["ControlMean"].tolist() == [1.0, 0.0, (BIG + 1) / 6, 2 / 6]
    # no permutations: NaN p-values, NaN null columns
    t0 = report.burden_table(report.burden_reference(WEIGHTS, np.zeros((0, 1), np.uint64), 4), 4, 4)
    assert np.isnan(t0[["PvalueUpper", "PvalueLower", "NullMean", "NullSD", "Z"]].to_numpy()).all()
    with pytest.raises(ValueError, match="3 names for 4 rows"):
        report.burden_table(r, 4, 4, names=["a", "b", "c"])
    with pytest.raises(ValueError, match="2 set counts for 4 rows"):
        report.burden_table(r, 4, 4, group_sets=[1, 2])


# ---- the argument check, the C++ itself ---------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("burden") / "burden_main")
    # the sanitizers' runtimes are linked statically: the program then runs whatever the environment it inherits preloads
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", SRC, "-o", out], check=True)
    return out


# a context of 5 patients, 100 permutations (padded to 2,048), 8 dwords per plane
CTX = dict(n_patients=5, n_cols=5, iterations=100, masks=1, W32p=8, Kpad=2048)
W = "patient_burden: "
ARG_CASES = [
    ("rows of every width", dict(n_rows=4, weights=[0, 1, 0, 0, 0, 2, 3, 0, 0, 0, 0, 0, 0, 0, 0, BIG, 0, 16, 15, 0]), OK, "[1 2 0 31]", ""),
    ("no rows, NULL weights", dict(n_rows=0), OK, "[]", ""),
    ("no rows, an empty array", dict(n_rows=0, weights=[]), OK, "[]", ""),
    ("no rows, no patients at all", dict(n_rows=0, n_cols=0, n_patients=0), OK, "[]", ""),
    ("no permutations need no masks", dict(n_rows=1, weights=[1, 2, 3, 4, 5], iterations=0, masks=0, Kpad=0), OK, "[3]", ""),
    ("under the bound", dict(n_rows=1, weights=[1, 0, 0, 0, 7], max_mb=(3 * 32 + 2048 * 8) / 1048576), OK, "[3]", ""),
    ("a row of zeros is never too large", dict(n_rows=1, weights=[0] * 5, max_mb=0), OK, "[0]", ""),
    ("NULL out", dict(n_rows=1, weights=[0] * 5, out=0), ERR_ARG, "[]", W + "NULL out"),
    ("negative rows", dict(n_rows=-1, weights=[]), ERR_ARG, "[]", W + "n_rows must not be negative, not -1"),
    ("NULL weights", dict(n_rows=2), ERR_ARG, "[]", W + "NULL weights with 2 rows"),
    ("too few columns", dict(n_rows=1, n_cols=4, weights=[0] * 4), ERR_ARG, "[]", W + "4 columns for 5 patients (n_cases + n_ctrls)"),
    ("too many columns", dict(n_rows=1, n_cols=6, weights=[0] * 6), ERR_ARG, "[]", W + "6 columns for 5 patients (n_cases + n_ctrls)"),
    ("no masks", dict(n_rows=1, weights=[1] * 5, masks=0), ERR_ASSERT, "[]",
     "assertion: patient_burden needs the permutation masks (iterations > 0, none set)"),
    ("a negative weight", dict(n_rows=2, weights=[1, 2, 3, 4, 5, 0, 0, -1, 0, 0]), ERR_ARG, "[]", W + "weights[1][2] = -1 is negative"),
    ("the most negative weight", dict(n_rows=1, weights=[0, 0, 0, 0, -2**31]), ERR_ARG, "[]", W + "weights[0][4] = -2147483648 is negative"),
    ("over the bound", dict(n_rows=2, weights=[1] * 5 + [4] * 5, max_mb=(3 * 32 + 2048 * 8 - 1) / 1048576), ERR_ARG, "[]",
     W + "one row of 3 planes and 2048 sums takes 16480 bytes: above GCRE_BURDEN_MAX_MB = 0.015716"),
    ("arguments before weights", dict(n_rows=1, n_cols=4, weights=[-1] * 4), ERR_ARG, "[]", W + "4 columns for 5 patients (n_cases + n_ctrls)"),
]


@pytest.mark.parametrize("name,case,code,planes,message", ARG_CASES, ids=[c[0] for c in ARG_CASES])
def test_argument_check_under_sanitizers(prog, tmp_path, name, case, code, planes, message):
    lines = [(k, *v) if isinstance(v, list) else (k, v) for k, v in {**CTX, **case}.items()]
    path = tmp_path / "case.txt"
    path.write_text("\n".join(" ".join(str(x) for x in ln) for ln in lines) + "\n")
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout}\n{r.stderr}"
    assert r.stdout.splitlines() == [f"check {code} {planes} {message}"]


# ---- the interface ---------------------------------------------------------------------------------------------------


def test_interface_is_declared():
    header = open(os.path.join(ROOT, "include", "gcre_hip.h")).read()
    assert re.search(r"#define GCRE_ABI_VERSION 4\b", header)      # additions only
    flat = " ".join(header.split())
    assert "typedef struct { int64_t total, observed, n_ge, n_le; int32_t planes; double p_upper, p_lower; } gcre_burden;" in flat
    assert ("int gcre_patient_burden(gcre_ctx* ctx, const int32_t* weights, int64_t n_rows, int32_t n_cols, gcre_burden* out, "
            "int64_t* null_sums);") in flat
    assert "int64_t gcre_burden_launches(const gcre_ctx* ctx);" in flat
    assert {"gcre_patient_burden", "gcre_burden_launches"} <= set(api.EXPORTS)
    parent, needs, _, binds = api._FEATURES["burden"]
    assert parent is None and set(needs) == set(binds) == {"gcre_patient_burden", "gcre_burden_launches"}
    assert len(binds["gcre_patient_burden"][1]) == 6
    assert api.BURDEN.itemsize == 56 and api.BURDEN.names == ("total", "observed", "n_ge", "n_le", "planes", "p_upper", "p_lower")
    assert [api.BURDEN.fields[k][1] for k in api.BURDEN.names] == [0, 8, 16, 24, 32, 40, 48]
    from geneticscre_amd import build
    assert "gcre_burden.hip" in build.SOURCES
    kernels = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_kernels.h")).read()
    for name in ("launch_burden_planes(", "launch_burden_null(", "launch_burden_finish(", "struct BurdenItem", "struct BurdenNullArgs"):
        assert name in kernels, name
    src = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_burden.hip")).read()
    assert all(k in src for k in ("k_burden_planes", "k_burden_null", "k_burden_finish")) and "asm" not in src
    assert "check_burden_args(" in open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_setlists.h")).read()
    lib = api._burden_lib()                                  # loads without a GPU
    assert lib.gcre_abi_version() == 4 and lib.gcre_burden_launches(None) == -1
    assert lib.gcre_patient_burden(None, None, 0, 0, None, None) == ERR_ARG      # no context: nothing to touch
    assert isinstance(api.JoinExec.burden_launches, property)


def test_signatures_and_the_caveat():
    pb = inspect.signature(api.JoinExec.patient_burden).parameters
    assert list(pb) == ["self", "weights", "null"] and pb["null"].default is False
    assert list(inspect.signature(report.burden_reference).parameters) == ["weights", "masks", "n_cases"]
    bt = inspect.signature(report.burden_table).parameters
    assert list(bt) == ["res", "n_cases", "n_ctrls", "names", "group_sets"] and bt["names"].default is None and bt["group_sets"].default is None
    bs = inspect.signature(report.burden_test).parameters
    assert list(bs) == ["sets", "genes", "data", "n_cases", "n_ctrls", "signed", "group", "names", "threshold", "n_permutations",
                        "strata", "seed", "device"]
    assert [bs[k].default for k in list(bs)[5:]] == [False, None, None, 0.05, 100, None, 0, 0]
    rp = inspect.signature(report.replicate).parameters
    assert list(rp)[:5] == ["results_df", "genes", "data", "n_cases", "n_ctrls"] and rp["leads_only"].default is False
    for fn in (report.replicate, report.burden_test):
        doc = " ".join(fn.__doc__.split())
        assert "A burden p-value on sets selected on the same labels" in doc and "is meaningless" in doc
    doc = " ".join(report.burden_test.__doc__.split())
    assert "one-gene sets" in doc and "group=group" in doc
    # gwaspa gets no new option: patient_table is still the last one
    assert list(inspect.signature(report.gwaspa).parameters)[-1] == "patient_table"


def test_value_errors_come_before_the_library(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched")
    for name in ("load_library", "_feature_lib", "_burden_lib"):
        monkeypatch.setattr(api, name, touched)
    ex = types.SimpleNamespace(num_cases=3, num_ctrls=2, iters=4, _h=None)
    for bad, text in ((np.zeros((2, 4), np.int32), r"weights: \[rows\]\[5\]"),
                      (np.zeros(5, np.int32), r"weights: \[rows\]\[5\]"),
                      (np.zeros((2, 2, 2, 5), np.int32), r"weights: \[rows\]\[5\]"),
                      (np.zeros((2, 5)), "weights: integers, not float64"),
                      (np.array([[0, 0, 0, 0, -1]]), "every weight must lie in"),
                      (np.array([[0, 0, 2**31, 0, 0]]), "every weight must lie in")):
        with pytest.raises(ValueError, match=text):
            api.JoinExec.patient_burden(ex, bad)
    # a well-formed call gets as far as the library: [rows][n], [G][H][n], no rows at all
    for good in (np.zeros((2, 5), np.int64), np.ones((2, 2, 5), np.int32), np.zeros((0, 5), np.int32), np.ones((1, 5), bool)):
        with pytest.raises(AssertionError, match="the library was touched"):
            api.JoinExec.patient_burden(ex, good, null=True)
