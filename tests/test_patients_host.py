"""Carrier tallies per patient, host side: ``report.patient_counts_reference`` -- the definition of
gcre_set_patient_counts -- on a hand-worked example; ``report.patient_table``; the argument check of the entry
(check_patient_index, csrc/gcre_setlists.h), the C++ itself, driven by tests/native/patients_main.cpp under the address and
undefined-behaviour sanitizers as a child process; the interface, the keyword defaults and the ValueErrors that come before the
library.  No GPU needed."""
from __future__ import annotations

import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from geneticscre_amd import api, report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "patients_main.cpp")
OK, ERR_RANGE, ERR_ARG = 0, -2, -4   # include/gcre_hip.h

# ---- the definition, hand-worked -------------------------------------------------------------------------------------
# patients 0-3 are cases, 4-7 controls
ROWS = np.array([[1, 1, 0, 0, 1, 0, 0, 0],     # g0
                 [0, 1, 1, 0, 0, 1, 0, 0],     # g1
                 [0, 0, 0, 1, 0, 0, 1, 0],     # g2
                 [1, 1, 1, 1, 1, 1, 1, 1],     # g3: everybody
                 [0, 0, 0, 0, 0, 0, 0, 1]])    # g4
# set 4 has an NA member, set 5 a repeated member, set 6 one member under both signs
SETS = [[0, 1], [1, 2], [3], [4], [0, -1], [0, 0, 1], [1, 1]]
SIGNS = [[1, -1], [1, -1], [1], [-1], [1, 1], [1, 1, -1], [1, -1]]
# set 0 twice (a repeated which); the NA set in a group (skipped); set 3 once outside every group (-1) and once inside;
# group 2 stays empty
WHICH = [0, 0, 1, 2, 4, 5, 3, 6, 3]
GROUP = [0, 0, 0, 1, 1, 3, -1, 3, 3]
ZERO = [0] * 8
ONES = [1] * 8


def test_reference_hand_worked_carrier_rows():
    counts, group_sets, skipped = report.patient_counts_reference(SETS, ROWS, SIGNS, WHICH, GROUP, 4, 8, False)
    assert counts.shape == (4, 1, 8) and counts.dtype == np.int32
    # group 0: 2 x (g0 | g1) + (g1 | g2); group 1: g3; group 3: (g0 | g1) + g1 + g4
    assert counts[:, 0].tolist() == [[2, 3, 3, 1, 2, 3, 1, 0], ONES, ZERO, [1, 2, 2, 0, 1, 2, 0, 1]]
    assert group_sets.tolist() == [3, 1, 0, 3] and skipped == 1
    # the signs are not read without by_sign
    again = report.patient_counts_reference(SETS, ROWS, None, WHICH, GROUP, 4, 8, False)
    assert np.array_equal(again[0], counts) and again[1].tolist() == [3, 1, 0, 3] and again[2] == 1


def test_reference_hand_worked_by_sign():
    counts, group_sets, skipped = report.patient_counts_reference(SETS, ROWS, SIGNS, WHICH, GROUP, 4, 8, True)
    assert counts.shape == (4, 2, 8)
    # group 0: P = 2 x g0 + g1, N = 2 x g1 + g2; group 3: P = g0 (listed twice, ORed once) + g1 + nothing, N = g1 + g1 + g4:
    # set 6's member counts in both planes, no conflict removal
    assert counts[0].tolist() == [[2, 3, 1, 0, 2, 1, 0, 0], [0, 2, 2, 1, 0, 2, 1, 0]]
    assert counts[1].tolist() == [ONES, ZERO] and counts[2].tolist() == [ZERO, ZERO]
    assert counts[3].tolist() == [[1, 2, 1, 0, 1, 1, 0, 0], [0, 2, 2, 0, 0, 2, 0, 1]]
    assert group_sets.tolist() == [3, 1, 0, 3] and skipped == 1
    # signs None: everything is in P
    plain = report.patient_counts_reference(SETS, ROWS, None, WHICH, GROUP, 4, 8, False)[0]
    nos = report.patient_counts_reference(SETS, ROWS, None, WHICH, GROUP, 4, 8, True)[0]
    assert np.array_equal(nos[:, 0], plain[:, 0]) and not nos[:, 1].any()


def test_reference_defaults_forms_and_refusals():
    counts, group_sets, skipped = report.patient_counts_reference(SETS, ROWS, None, None, None, None, 8, False)
    assert counts.shape == (1, 1, 8) and group_sets.tolist() == [6] and skipped == 1      # every set once, the NA set skipped
    assert counts[0, 0].tolist() == [3, 5, 5, 2, 3, 5, 2, 2]
    # n_groups None with a group list: max + 1
    assert report.patient_counts_reference(SETS, ROWS, None, WHICH, GROUP, None, 8, False)[0].shape == (4, 1, 8)
    # (off, members) with flat signs is the same list
    off = np.cumsum([0] + [len(s) for s in SETS]).astype(np.int64)
    members = np.concatenate(SETS).astype(np.int32)
    flat = np.concatenate(SIGNS)
    for by_sign in (False, True):
        a = report.patient_counts_reference(SETS, ROWS, SIGNS, WHICH, GROUP, 4, 8, by_sign)
        b = report.patient_counts_reference((off, members), ROWS, flat, WHICH, GROUP, 4, 8, by_sign)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    # columns beyond n are not patients
    wide = np.hstack([ROWS, np.ones((5, 3), int)])
    assert np.array_equal(report.patient_counts_reference(SETS, wide, SIGNS, WHICH, GROUP, 4, 8, True)[0],
                          report.patient_counts_reference(SETS, ROWS, SIGNS, WHICH, GROUP, 4, 8, True)[0])
    # no entries, and every entry outside the groups
    assert not report.patient_counts_reference(SETS, ROWS, None, [], [], 2, 8, False)[0].any()
    none = report.patient_counts_reference(SETS, ROWS, None, [0, 4], [-1, -1], 2, 8, False)
    assert not none[0].any() and none[1].tolist() == [0, 0] and none[2] == 0
    for kw, text in ((dict(which=[7], group=[0]), "out of range"), (dict(which=[-1], group=[0]), "out of range"),
                     (dict(which=[0], group=[4]), "out of range"), (dict(which=[0], group=[-2]), "out of range"),
                     (dict(which=[0], group=[0, 0]), "2 entries for 1 counted sets")):
        with pytest.raises(ValueError, match=text):
            report.patient_counts_reference(SETS, ROWS, None, kw["which"], kw["group"], 4, 8, False)
    with pytest.raises(ValueError, match="n_groups"):
        report.patient_counts_reference(SETS, ROWS, None, None, None, 2, 8, False)
    with pytest.raises(ValueError, match="signs: one sign per member"):
        report.patient_counts_reference(SETS, ROWS, SIGNS[:-1], None, None, 1, 8, True)


def test_patient_table_columns_and_order():
    counts, group_sets, _ = report.patient_counts_reference(SETS, ROWS, None, WHICH, GROUP, 4, 8, False)
    t = report.patient_table(counts, 4, group_sets=group_sets)
    assert list(t.columns) == ["Patient", "Label", "Group0", "Group1", "Group2", "Group3", "Hits", "HitShare"]
    assert t["Patient"].tolist() == list(range(8))                        # patient order, not sorted by anything
    assert t["Label"].tolist() == ["case"] * 4 + ["control"] * 4
    assert t["Group0"].tolist() == [2, 3, 3, 1, 2, 3, 1, 0] and t["Group2"].tolist() == ZERO
    assert t["Hits"].tolist() == [4, 6, 6, 2, 4, 6, 2, 2]
    assert np.array_equal(t["HitShare"].to_numpy(), np.array([4, 6, 6, 2, 4, 6, 2, 2]) / 7)
    # names, column names, a last group that is not part of Hits (gwaspa's "Leads")
    names = [f"p{q}" for q in range(8)]
    t2 = report.patient_table(counts[:, 0], 3, names=names, columns=["Hits.L1", "Hits.L2", "Hits.L3", "Leads"],
                              group_sets=group_sets, summed=3)
    assert list(t2.columns) == ["Patient", "Label", "Hits.L1", "Hits.L2", "Hits.L3", "Leads", "Hits", "HitShare"]
    assert t2["Patient"].tolist() == names and t2["Label"].tolist() == ["case"] * 3 + ["control"] * 5
    assert t2["Leads"].tolist() == [1, 2, 2, 0, 1, 2, 0, 1] and t2["Hits"].tolist() == [3, 4, 4, 2, 3, 4, 2, 1]
    assert np.array_equal(t2["HitShare"].to_numpy(), np.array([3, 4, 4, 2, 3, 4, 2, 1]) / 4)
    # without the numbers of sets there is no share; all cases, all controls
    assert np.isnan(report.patient_table(counts, 4)["HitShare"]).all()
    assert report.patient_table(counts, 0)["Label"].tolist() == ["control"] * 8
    assert report.patient_table(counts, 8)["Label"].tolist() == ["case"] * 8
    both = report.patient_counts_reference(SETS, ROWS, SIGNS, WHICH, GROUP, 4, 8, True)[0]
    with pytest.raises(ValueError, match="2 planes"):
        report.patient_table(both, 4)
    with pytest.raises(ValueError, match="4 distinct column names"):
        report.patient_table(counts, 4, columns=["a", "b", "c"])
    with pytest.raises(ValueError, match="4 distinct column names"):
        report.patient_table(counts, 4, columns=["a", "b", "c", "Hits"])
    with pytest.raises(ValueError, match="7 names for 8 patients"):
        report.patient_table(counts, 4, names=names[:7])
    with pytest.raises(ValueError, match="n_cases = 9"):
        report.patient_table(counts, 9)
    assert "Descriptive" in report.patient_table.__doc__


# ---- the argument check, the C++ itself ---------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("patients") / "patients_main")
    # the sanitizers' runtimes are linked statically: the program then runs whatever the environment it inherits preloads
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", SRC, "-o", out], check=True)
    return out


# three sets over four rows; set 2 has an NA member
LIST = dict(n_rows=4, n_sets=3, set_off=[0, 2, 3, 5], members=[0, 1, 2, 3, -1])
W = "set_patient_counts: "
BAD_LIST = W + "bad index list (a negative length, or NULL `which` with a length other than n_sets)"
INDEX_CASES = [
    ("both lists", dict(n_which=4, n_groups=2, which=[0, 2, 1, 1], group=[0, -1, 1, 0]), OK, ""),
    ("an NA set may be listed", dict(n_which=1, which=[2], group=[0]), OK, ""),
    ("NULL which", dict(n_which=3, n_groups=2, group=[1, 0, -1]), OK, ""),
    ("NULL group", dict(n_which=2, which=[1, 1]), OK, ""),
    ("both NULL", dict(n_which=3, by_sign=1), OK, ""),
    ("no entries", dict(n_which=0, which=[], group=[]), OK, ""),
    ("under the size bound", dict(n_which=3, n_cols=1000, max_mb=0.004), OK, ""),
    ("by_sign 2", dict(n_which=3, by_sign=2), ERR_ARG, W + "by_sign must be 0 or 1, not 2"),
    ("by_sign negative", dict(n_which=3, by_sign=-1), ERR_ARG, W + "by_sign must be 0 or 1, not -1"),
    ("no groups", dict(n_which=3, n_groups=0, group=[0, 0, 0]), ERR_ARG, W + "n_groups must be at least 1, not 0"),
    ("negative length", dict(n_which=-1, which=[0], group=[0]), ERR_ARG, BAD_LIST),
    ("NULL which, another length", dict(n_which=2, group=[0, 0]), ERR_ARG, BAD_LIST),
    ("NULL group, two groups", dict(n_which=3, n_groups=2), ERR_ARG,
     W + "NULL `group` puts every entry in group 0: n_groups must be 1, not 2"),
    ("NULL counts", dict(n_which=3, counts=0), ERR_ARG, W + "NULL counts"),
    ("a cell could overflow", dict(n_which=2**31 - 17, which=[0], group=[0]), ERR_ARG,
     W + "2147483631 entries: a 32-bit count could overflow (fewer than 2^31 - 16)"),
    ("over the size bound", dict(n_which=3, n_groups=3, by_sign=1, n_cols=1000, max_mb=0.01, group=[0, 1, 2]), ERR_ARG,
     W + "3 groups x 2 planes x 1000 patients x 4 bytes exceed GCRE_PATIENT_MAX_MB = 0.010000"),
    ("which below", dict(n_which=2, which=[0, -1], group=[0, 0]), ERR_RANGE, W + "which[1] = -1 out of range (3 sets)"),
    ("which above", dict(n_which=2, which=[3, 0]), ERR_RANGE, W + "which[0] = 3 out of range (3 sets)"),
    ("group below", dict(n_which=2, n_groups=2, which=[0, 0], group=[-1, -2]), ERR_RANGE,
     W + "group[1] = -2 out of range (2 groups, -1 = not counted)"),
    ("group above", dict(n_which=3, n_groups=2, group=[0, 2, 0]), ERR_RANGE,
     W + "group[1] = 2 out of range (2 groups, -1 = not counted)"),
    ("arguments before ranges", dict(n_which=2, by_sign=2, which=[9, 0]), ERR_ARG, W + "by_sign must be 0 or 1, not 2"),
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
    assert ("int gcre_set_patient_counts(gcre_ctx* ctx, const gcre_set_input* in, const int64_t* which, int64_t n_which, "
            "const int32_t* group, int32_t n_groups, int by_sign, int32_t* counts, int64_t* group_sets, int64_t* skipped);") in flat
    assert "int64_t gcre_patient_launches(const gcre_ctx* ctx);" in flat
    assert {"gcre_set_patient_counts", "gcre_patient_launches"} <= set(api.EXPORTS)
    parent, needs, _, binds = api._FEATURES["patients"]
    assert parent is None and set(needs) == set(binds) == {"gcre_set_patient_counts", "gcre_patient_launches"}
    assert len(binds["gcre_set_patient_counts"][1]) == 10
    from geneticscre_amd import build
    assert "gcre_patients.hip" in build.SOURCES
    kernels = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_kernels.h")).read()
    assert "launch_set_patient_counts(" in kernels and "struct PatientCountArgs" in kernels
    assert 5 <= int(re.search(r"constexpr int kPatientPlanes = (\d+);", kernels).group(1)) <= 30
    assert "k_set_patient_counts" in open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_patients.hip")).read()
    assert "check_patient_index(" in open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_setlists.h")).read()
    lib = api._patients_lib()                                # loads without a GPU
    assert lib.gcre_abi_version() == 4 and lib.gcre_patient_launches(None) == -1
    assert isinstance(api.JoinExec.patient_launches, property)


def test_defaults_change_nothing():
    pc = inspect.signature(api.JoinExec.patient_counts).parameters
    assert list(pc) == ["self", "sets", "rows", "which", "group", "n_groups", "by_sign", "signs"]
    assert [pc[k].default for k in ("which", "group", "n_groups", "by_sign", "signs")] == [None, None, None, False, None]
    assert list(inspect.signature(report.patient_counts_reference).parameters) == \
        ["sets", "rows", "signs", "which", "group", "n_groups", "n", "by_sign"]
    pt = inspect.signature(report.patient_table).parameters
    assert list(pt)[:4] == ["counts", "n_cases", "names", "columns"] and pt["names"].default is None
    gw = inspect.signature(report.gwaspa).parameters
    assert gw["patient_table"].default is False
    # every keyword gwaspa had keeps its place and its default: the new one is the last
    assert list(gw)[-1] == "patient_table" and list(gw)[-2] == "clump_significant"
    assert "descriptive" in report.gwaspa.__doc__ and "Patient.Results" in report.gwaspa.__doc__


def test_gwaspa_needs_significant_before_anything_runs(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("something ran")
    for name in ("load_library", "_feature_lib", "_patients_lib", "JoinExec", "build_levels", "values_table"):
        monkeypatch.setattr(api, name, touched)
    monkeypatch.setattr(report, "preprocess_table", touched)
    with pytest.raises(ValueError, match="patient_table: needs significant"):
        report.gwaspa(["a", "b"], np.zeros((2, 8)), 4, 4, None, patient_table=True)
    # the default does not reach the new check: the next thing the call does is the old one
    with pytest.raises(AssertionError, match="something ran"):
        report.gwaspa(["a", "b"], np.zeros((2, 8)), 4, 4, None)


def test_value_errors_come_before_the_library(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the library was touched")
    for name in ("load_library", "_feature_lib", "_patients_lib"):
        monkeypatch.setattr(api, name, touched)
    rows = np.zeros((4, 5), np.int8)
    sets = [[0, 1], [2], [3, -1]]
    off, members = np.array([0, 2, 3, 5], np.int64), np.array([0, 1, 2, 3, -1], np.int32)
    for form in (sets, (off, members)):
        for kw, text in ((dict(which=[0, 3]), r"which: a set index outside 0\.\.2"),
                         (dict(which=[-1]), "which: a set index outside"),
                         (dict(group=[0, 0, 2], n_groups=2), r"group: a group outside -1\.\.1"),
                         (dict(group=[-2, 0, 0]), "group: a group outside"),
                         (dict(group=[0, 1]), "group: 2 entries for 3 counted sets"),
                         (dict(which=[0], group=[0, 1]), "group: 2 entries for 1 counted sets"),
                         (dict(n_groups=2), "group: None puts every entry in group 0"),
                         (dict(group=[0, 0, 0], n_groups=0), "n_groups must be at least 1")):
            with pytest.raises(ValueError, match=text):
                api.JoinExec.patient_counts(None, form, rows, **kw)
    with pytest.raises(ValueError, match="signs: one sign per member of every set"):
        api.JoinExec.patient_counts(None, sets, rows, by_sign=True, signs=[[1, 1], [1], [1]])
    with pytest.raises(ValueError, match="signs: one sign per member of every set"):
        api.JoinExec.patient_counts(None, (off, members), rows, by_sign=True, signs=[1, 1, 1])
    # a well-formed call gets as far as the library
    with pytest.raises(AssertionError, match="the library was touched"):
        api.JoinExec.patient_counts(None, sets, rows, which=[0, 0, 2], group=[1, -1, 0])
