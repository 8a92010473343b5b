"""Step-down, k-FWER and FDR over a family of given sets, host side: ``report.family_reference`` -- the
definition of gcre_score_sets_family -- on a hand-worked example and against the definitions taken literally on random
matrices; the consequences the header states; ``report.family_columns``; the host plan in C++ (csrc/gcre_family.h), driven
by tests/native/family_main.cpp under the address and undefined-behaviour sanitizers as a child process; the interface.  No
GPU needed."""
from __future__ import annotations

import inspect
import os
import re

import numpy as np
import pytest

import family_native
from geneticscre_amd import api, report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -4   # include/gcre_hip.h
NAN = float("nan")

# ---- the definition, hand-worked: four valid sets x six permutations, and a set with an NA member -------------------
OBS = np.array([3.0, 1.0, NAN, 1.0, NAN])      # set 2 is invalid (its score is never read); sets 1 and 3 tie; set 4 scores NaN
VALID = np.array([1, 1, 0, 1, 1])
NULL = np.array([[0.5, 3.0, 1.0, 0.0, 4.0, 0.5],
                 [1.0, 0.5, 0.5, 0.0, 0.5, 2.0],
                 [NAN] * 6,
                 [0.5, 0.5, 0.0, 0.5, 3.5, 0.5],
                 [0.0, 0.5, 0.5, 1.5, 0.0, 0.0]], dtype=np.float32)
# set 0 (3.0): nothing scores higher: the maxima over all four rows are 1, 3, 1, 1.5, 4, 2 -- two reach 3; the values >= 3
#   are 3.0, 4.0 and 3.5; one set scores >= 3
# sets 1 and 3 (1.0, tied): set 0 is set aside, the tied partner and the NaN-scored set are not: maxima 1, .5, .5, 1.5, 3.5, 2
#   -- four reach 1; the values >= 1: three of set 0, two of set 1, one of set 3, one of set 4; three sets score >= 1
SD = [2, 4, -1, 4, 0]
EXCEED = [3, 7, 0, 7, 0]
OBSERVED = [1, 3, -1, 3, 0]
KMAX0 = [1.0, 3.0, 1.0, 1.5, 4.0, 2.0]
KMAX1 = [0.5, 0.5, 0.5, 0.5, 3.5, 0.5]
KMAX3 = [0.0, 0.5, 0.0, 0.0, 0.0, 0.0]


def test_reference_hand_worked():
    ref = report.family_reference(OBS, VALID, NULL)
    assert ref["n_ge_stepdown"].dtype == np.int64 and ref["n_ge_stepdown"].tolist() == SD
    assert ref["exceed"].dtype == np.uint64 and ref["exceed"].tolist() == EXCEED
    assert ref["observed"].dtype == np.int64 and ref["observed"].tolist() == OBSERVED
    km = ref["kmax"]
    assert km.dtype == np.float32 and km.shape == (report.FAMILY_KMAX, 6)
    assert km[0].tolist() == KMAX0 and km[1].tolist() == KMAX1 and km[3].tolist() == KMAX3
    assert not km[4:].any()                     # four valid sets: nothing beyond the fourth largest


def test_reference_signed_zeros_tie_and_empty_family():
    ref = report.family_reference([0.0, -0.0], [1, 1], np.zeros((2, 3), np.float32))
    assert ref["n_ge_stepdown"].tolist() == [3, 3] and ref["exceed"].tolist() == [6, 6] and ref["observed"].tolist() == [2, 2]
    ref = report.family_reference([1.0, 2.0], [0, 0], np.full((2, 4), NAN, np.float32))
    assert ref["n_ge_stepdown"].tolist() == [-1, -1] and ref["exceed"].tolist() == [0, 0] and not ref["kmax"].any()
    ref = report.family_reference([1.0], [1], np.zeros((1, 0), np.float32))
    assert ref["n_ge_stepdown"].tolist() == [0] and ref["observed"].tolist() == [1] and ref["kmax"].shape == (report.FAMILY_KMAX, 0)


def _literal(obs, valid, null):
    """The definitions of the header, one set at a time."""
    S = len(obs)
    N = null.astype(np.float64)
    sd, ex, ob = np.zeros(S, np.int64), np.zeros(S, np.uint64), np.zeros(S, np.int64)
    v = np.flatnonzero(valid)
    for j in range(S):
        if not valid[j]:
            sd[j] = ob[j] = -1
            continue
        if np.isnan(obs[j]):
            continue
        keep = [i for i in v if not obs[i] > obs[j]]
        sd[j] = int((N[keep].max(axis=0) >= obs[j]).sum())
        ex[j] = int((N[v] >= obs[j]).sum())
        ob[j] = int((obs[v] >= obs[j]).sum())
    return sd, ex, ob


def _random_family(rng, S, K):
    """Scores and null values from a small grid, so that ties and exact hits are common; some sets invalid or NaN-scored."""
    grid = np.array([0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0, np.inf], np.float32)
    null = rng.choice(grid[:-1], size=(S, K)).astype(np.float32)
    obs = rng.choice(np.concatenate([grid[:-1].astype(np.float64), [0.3, 1.0 + 1e-12, -0.0, NAN]]), size=S)
    valid = rng.random(S) > 0.15
    null[~valid] = NAN
    return obs, valid, null


def test_reference_against_the_literal_definitions_and_the_consequences():
    rng = np.random.default_rng(315)
    for case in range(40):
        S, K = int(rng.integers(1, 24)), int(rng.integers(1, 40))
        obs, valid, null = _random_family(rng, S, K)
        ref = report.family_reference(obs, valid, null)
        sd, ex, ob = _literal(obs, valid, null)
        assert ref["n_ge_stepdown"].tolist() == sd.tolist(), case
        assert ref["exceed"].tolist() == ex.tolist(), case
        assert ref["observed"].tolist() == ob.tolist(), case
        v = np.flatnonzero(valid)
        km = ref["kmax"].astype(np.float64)
        if len(v):
            srt = -np.sort(-null[v], axis=0)
            for k in range(report.FAMILY_KMAX):
                assert km[k].tolist() == (srt[k].tolist() if k < len(v) else [0.0] * K)
        scored = [j for j in v if not np.isnan(obs[j])]
        for j in scored:
            nominal = int((null[j].astype(np.float64) >= obs[j]).sum())
            single = int((km[0] >= obs[j]).sum())
            assert nominal <= ref["n_ge_stepdown"][j] <= single                     # between the set's own count and max-T
            assert int(ref["exceed"][j]) == sum(int((null[i].astype(np.float64) >= obs[j]).sum()) for i in v)
        if scored:
            best = max(scored, key=lambda j: obs[j])
            assert ref["n_ge_stepdown"][best] == int((km[0] >= obs[best]).sum())     # nothing is set aside for the best set


def test_family_columns_hand_worked():
    ref = report.family_reference(OBS, VALID, NULL)
    cols = report.family_columns(OBS, VALID, ref, ref["kmax"], 6)
    assert list(cols) == report.FAMILY_COLUMNS == ["FamilyPvaluesStepDown", "FamilyExpectedFalse", "FamilyFDR", "FamilyQvalues",
                                                   "FamilykFWER.2", "FamilykFWER.5", "FamilykFWER.10"]
    ok = np.array([True, True, False, True, False])
    for c in cols.values():
        assert np.isnan(c[~ok]).all() and not np.isnan(c[ok]).any()
    single = report._tail_pvalues(ref["kmax"][0], OBS[ok])                      # 2/6, 6/6, 6/6
    sdp = cols["FamilyPvaluesStepDown"]
    assert sdp[ok].tolist() == [2 / 6, 4 / 6, 4 / 6]
    assert (sdp[ok] <= single).all() and sdp[0] == single[0]                    # never above max-T, equal on the best row
    assert cols["FamilyExpectedFalse"][ok].tolist() == [3 / 6, 7 / 6, 7 / 6]
    assert cols["FamilyFDR"][ok].tolist() == [0.5, 7 / 6 / 3, 7 / 6 / 3]
    assert cols["FamilyQvalues"][ok].tolist() == [7 / 6 / 3, 7 / 6 / 3, 7 / 6 / 3]
    assert cols["FamilykFWER.2"][ok].tolist() == [1 / 6, 1 / 6, 1 / 6]          # second largest values: only 3.5 reaches 1
    assert cols["FamilykFWER.5"][ok].tolist() == [0.0, 0.0, 0.0] and cols["FamilykFWER.10"][ok].tolist() == [0.0, 0.0, 0.0]
    none = report.family_columns(OBS, VALID, ref, np.zeros((report.FAMILY_KMAX, 0), np.float32), 0)
    assert all(np.isnan(c).all() for c in none.values())


def test_family_columns_monotone_on_random_families():
    rng = np.random.default_rng(316)
    for case in range(20):
        S, K = int(rng.integers(2, 30)), int(rng.integers(1, 50))
        obs, valid, null = _random_family(rng, S, K)
        ref = report.family_reference(obs, valid, null)
        cols = report.family_columns(obs, valid, ref, ref["kmax"], K)
        ok = valid & ~np.isnan(obs)
        if not ok.any():
            continue
        order = np.flatnonzero(ok)[np.argsort(-obs[ok], kind="stable")]           # best score first
        sdp, q = cols["FamilyPvaluesStepDown"][order], cols["FamilyQvalues"][order]
        single = report._tail_pvalues(ref["kmax"][0], obs[order])
        assert (sdp <= single).all() and sdp[0] == single[0], case
        assert (np.diff(sdp) >= 0).all(), case                                   # a p-value never falls as the score does
        qq = q[~np.isnan(q)]
        assert (np.diff(qq) >= 0).all(), case
        same = np.flatnonzero(np.diff(obs[order]) == 0)
        assert (sdp[same] == sdp[same + 1]).all()                                # tied scores, equal values


# ---- the host plan in C++ (csrc/gcre_family.h), under the sanitizers ---------------------------------------------------
TOP = 0x80000000
SLAB_REFUSAL = "score_sets_family: the null scores of 3 sets under one tile of 512 permutations exceed GCRE_FAMILY_MAX_MB"


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return family_native.build_prog(tmp_path_factory.mktemp("family"))


def _walk(out):
    """The seven lines a `family` command prints first."""
    assert out[0].split()[0] == "family"
    return {"m": int(out[0].split()[1]), **{k: family_native.ints(out[1 + i], k)
                                            for i, k in enumerate(("order", "rank", "meta", "gstart", "bin", "pat"))}}


def test_native_hand_worked_walk_and_finish(prog, tmp_path):
    vset = np.flatnonzero(VALID).tolist()
    obs = OBS[vset].tolist()                                   # 3.0, 1.0, 1.0, NaN
    order, sd, pat, hist = family_native.family_device_part(obs, NULL[vset])
    assert (order, sd, pat, hist) == ([3, 1, 2, 0], [0, 0, 4, 2], [0x3F800000, 0x40400000], [4, 3])
    out = family_native.run_case(prog, tmp_path, [("n_sets", 5), ("vset", vset), ("obs", obs), ("sd", [0, 0, 4, 2]), ("hist", [4, 3]),
                                                  ("family", [])])
    w = _walk(out)
    assert w["m"] == 2 and w["order"] == [3, 1, 2, 0] and w["rank"] == [3, 1, 2, 0]
    assert len(w["meta"]) == 64 and not any(w["meta"][4:])
    assert [x >> 31 for x in w["meta"][:4]] == [1, 0, 1, 1]                        # tie groups end at rows 0, 2, 3
    assert [x & ~TOP for x in w["meta"][:4]] == [0x7F800001, 0x3F800000, 0x3F800000, 0x40400000]
    assert w["gstart"] == [0, 1, 1, 3] and w["bin"] == [-1, 0, 0, 1] and w["pat"] == [0x3F800000, 0x40400000]
    rec = np.array(family_native.ints(out[7], "records")).reshape(5, 3)
    assert rec[:, 0].tolist() == SD and rec[:, 1].tolist() == EXCEED and rec[:, 2].tolist() == OBSERVED


def test_native_walk_edges(prog, tmp_path):
    w = _walk(family_native.run_case(prog, tmp_path, [("n_sets", 1), ("vset", [0]), ("obs", [2.5]), ("family", [])]))
    assert w["order"] == [0] and w["rank"] == [0] and w["gstart"] == [0] and w["bin"] == [0] and w["m"] == 1
    assert len(w["meta"]) == 64 and w["meta"][0] == TOP | 0x40200000 and w["pat"] == [0x40200000]
    # every score NaN: no bin, no pattern but the one placeholder, every row ends a group that counts nothing
    out = family_native.run_case(prog, tmp_path, [("n_sets", 3), ("vset", [0, 1, 2]), ("obs", [NAN, NAN, NAN]), ("sd", [0, 0, 0]),
                                                  ("hist", [0]), ("family", [])])
    w = _walk(out)
    assert w["m"] == 0 and w["pat"] == [0] and w["bin"] == [-1, -1, -1] and w["order"] == [0, 1, 2]
    assert w["meta"][:3] == [TOP | 0x7F800001] * 3
    assert family_native.ints(out[7], "records") == [0, 0, 0] * 3
    # +0.0 against -0.0: one tie group, one pattern
    w = _walk(family_native.run_case(prog, tmp_path, [("n_sets", 2), ("vset", [0, 1]), ("obs", [0.0, -0.0]), ("family", [])]))
    assert w["order"] == [0, 1] and w["meta"][:2] == [0, TOP] and w["gstart"] == [0, 0] and w["bin"] == [0, 0] and w["pat"] == [0]
    # the padding of meta: whole 64 rows
    for V, padded in ((64, 64), (65, 128)):
        obs = [float(v % 7) for v in range(V)]
        w = _walk(family_native.run_case(prog, tmp_path, [("n_sets", V), ("vset", list(range(V))), ("obs", obs), ("family", [])]))
        assert len(w["meta"]) == padded and not any(w["meta"][V:]) and w["meta"][V - 1] >> 31 == 1
        assert sorted(w["order"]) == list(range(V)) and [w["rank"][v] for v in w["order"]] == list(range(V))
        assert w["order"] == family_native.family_walk(obs)[0] and w["m"] == 7
    assert [family_native.ints(line, "thr")[0] for line in family_native.run_case(
        prog, tmp_path, [("thr", 1.0), ("thr", 1.0 + 1e-12), ("thr", -0.0), ("thr", NAN), ("thr", float("inf"))])] == [
            0x3F800000, 0x3F800001, 0, 0x7F800001, 0x7F800000] == [family_native.f32_threshold(x) for x in (1.0, 1.0 + 1e-12, -0.0, NAN,
                                                                                                             float("inf"))]


def test_native_slab_sizing(prog, tmp_path):
    one_tile = 3 * family_native.TILE * 4 / 1048576.0          # three rows of one tile, in MB: exact in binary
    below = float(np.nextafter(one_tile, 0.0))
    asks = [((3, 2000, 512, one_tile, 0), "family_slab 0 1 "),((3, 2000, 512, below, 0), f"family_slab -4 0 {SLAB_REFUSAL}"),
            ((3, 2000, 512, 1024.0, 0), "family_slab 0 4 "), ((3, 2000, 512, 1024.0, 1), "family_slab 0 1 "),
            ((3, 2000, 512, 1024.0, 1023), "family_slab 0 1 "), ((3, 2000, 512, 1024.0, 1024), "family_slab 0 2 "),
            ((3, 2000, 512, 2 * one_tile, 0), "family_slab 0 2 "), ((0, 2000, 512, below, 0), "family_slab 0 0 "),
            ((3, 0, 512, below, 0), "family_slab 0 0 ")]
    assert family_native.run_case(prog, tmp_path, [("family_slab", a) for a, _ in asks]) == [w for _, w in asks]
    env = {k: v for k, v in os.environ.items() if not k.startswith("GCRE_")}
    assert family_native.run_case(prog, tmp_path, [("env", [])], env=env) == ["env 1024 0 1024 0"]
    for perms, want in (("0", 1), ("-5", 1), ("700", 700)):       # the test-only bound: one permutation at the least, so one tile
        out = family_native.run_case(prog, tmp_path, [("env", [])], env={**env, "GCRE_FAMILY_SLAB_PERMS": perms, "GCRE_FAMILY_MAX_MB": "0.25"})
        assert out == [f"env 0.25 {want} 1024 0"]
    assert family_native.run_case(prog, tmp_path, [("env", [])], env={**env, "GCRE_FAMILY_MAX_MB": "-3"}) == ["env 0 0 1024 0"]
    assert family_native.run_case(prog, tmp_path, [("env", [])], env={**env, "GCRE_FAMILY_MAX_MB": "1e9"}) == ["env 1048576 0 1024 0"]


def test_native_finish_on_random_families(prog, tmp_path):
    """The device's part taken literally from a null matrix, the native walk and finish, every field against the reference."""
    rng = np.random.default_rng(318)
    case, want = [], []
    for _ in range(200):
        S, K = int(rng.integers(1, 41)), int(rng.integers(1, 51))
        obs, valid, null = _random_family(rng, S, K)
        vset = np.flatnonzero(valid).tolist()
        order, sd, pat, hist = family_native.family_device_part(obs[vset].tolist(), null[vset])
        case += [("n_sets", S), ("vset", vset), ("obs", obs[vset].tolist()), ("sd", sd), ("hist", hist), ("family", [])]
        want.append((order, pat, report.family_reference(obs, valid, null)))
    out = family_native.run_case(prog, tmp_path, case)
    assert len(out) == 8 * len(want)
    for i, (order, pat, ref) in enumerate(want):
        w = _walk(out[8 * i:8 * i + 7])
        assert w["order"] == order and w["m"] == len(pat) and w["pat"] == (pat or [0]), i
        rec = np.array(family_native.ints(out[8 * i + 7], "records"), dtype=object).reshape(-1, 3)
        assert rec[:, 0].tolist() == ref["n_ge_stepdown"].tolist(), i
        assert rec[:, 1].tolist() == ref["exceed"].tolist(), i
        assert rec[:, 2].tolist() == ref["observed"].tolist(), i


# ---- the interface ---------------------------------------------------------------------------------------------------


def test_interface_is_declared():
    header = open(os.path.join(ROOT, "include", "gcre_hip.h")).read()
    assert re.search(r"#define GCRE_ABI_VERSION 4\b", header)      # additions only
    flat = " ".join(header.split())
    assert "#define GCRE_FAMILY_KMAX 10" in header
    assert "typedef struct { int64_t n_ge_stepdown; uint64_t exceed; int64_t observed; } gcre_family_score;" in flat
    assert ("int gcre_score_sets_family(gcre_ctx* ctx, const gcre_set_input* in, gcre_set_score* out, int64_t cap, int64_t* n_out, "
            "gcre_family_score* fam_out, float* kmax, float* null_scores);") in flat
    assert "int64_t gcre_family_launches(const gcre_ctx* ctx);" in flat
    assert {"gcre_score_sets_family", "gcre_family_launches"} <= set(api.EXPORTS)
    parent, needs, _, binds = api._FEATURES["family"]
    assert parent == "sets" and set(needs) == set(binds) == {"gcre_score_sets_family", "gcre_family_launches"}
    assert len(binds["gcre_score_sets_family"][1]) == 8
    assert api.FAMILY_KMAX == report.FAMILY_KMAX == 10
    assert api.FAMILY_SCORE.itemsize == 24 and api.FAMILY_SCORE.names == ("n_ge_stepdown", "exceed", "observed")
    assert [api.FAMILY_SCORE.fields[k][1] for k in api.FAMILY_SCORE.names] == [0, 8, 16]
    from geneticscre_amd import build
    assert "gcre_family.hip" in build.SOURCES
    kernels = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_kernels.h")).read()
    for name in ("launch_family_null(", "launch_family_scan(", "launch_family_hist(", "struct FamilyNullArgs", "struct FamilyScanArgs",
                 "struct FamilyHistArgs", "kFamilyKmax = 10", "kFamilyHistBins = 4096"):
        assert name in kernels, name
    src = open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_family.hip")).read()
    assert all(k in src for k in ("k_family_null", "k_family_scan", "k_family_hist")) and "asm" not in src
    lib = api._family_lib()                                  # loads without a GPU
    assert lib.gcre_abi_version() == 4 and lib.gcre_family_launches(None) == -1
    assert lib.gcre_score_sets_family(None, None, None, 0, None, None, None, None) == ERR_ARG   # no context: nothing to touch


def test_signatures():
    ft = inspect.signature(api.JoinExec.family_tests).parameters
    assert list(ft) == ["self", "sets", "rows", "signs", "kmax", "null"]
    assert ft["signs"].default is None and ft["kmax"].default is False and ft["null"].default is False
    assert callable(api.JoinExec.family_launches) and not isinstance(api.JoinExec.family_launches, property)
    assert list(inspect.signature(report.family_reference).parameters) == ["obs", "valid", "null"]
    assert list(inspect.signature(report.family_columns).parameters) == ["scores", "valid", "family", "kmax", "perms"]
    sp = inspect.signature(report.score_paths).parameters
    assert list(sp)[-1] == "family_inference" and sp["family_inference"].default is False
    assert report.SCORE_PATHS_COLUMNS == ["SignedPaths", "Paths", "Lengths", "Scores", "Cases", "Controls", "NominalPvalues",
                                          "FamilyPvalues", "Pvalues"]
