"""Bit-exact checks at the limits the product claims: cohorts between 2^15 and 2^16 patients, permutation counts past
2^16, and decorated p-values at both (pytest -m gpu).

Near these limits the code packs counts into 16-bit fields: the inspectors hold two counts per u32, ladder entries are
hi << 16 | lo, the sparse kernel packs two diagonal indices per u32, the bound filter clamps at 0xffff, and up to 16
counter planes hold a count.  IE, sparse and the pruning ladder run while 64 * Wp < 65535 (n <= 65,280); from 65,281 to
65,536 patients (R's limit, report.check_input) only the dense kernel runs.  Every check here compares with the CPU oracle
or with a CPU restatement of a sampler, bit for bit, at every level; each oracle runs once per geometry (module fixtures).

Memory: the cohort-limit geometries hold one (nc+1) x (nt+1) bench.fast_table at a time on the host (2.5 GB; the oracle
copies it once more in its lazy mode, so about 6 GB at peak).  On the device, 65,536 patients with method 2 hold about
37 GB of value tables (the f64 diagonal table and dmax, 2^31 cells each); method 1 holds the f64 table and its f32 copy."""
from __future__ import annotations

import dataclasses
import importlib.util
import os
import sys

import numpy as np
import pytest

import oracle
from geneticscre_amd import api, synth
from geneticscre_amd.synth import make_problem
from helpers import assert_same_result
from test_decorated_host import random_case
from test_gpu_api import _masks_restated
from test_gpu_configs import LST, MODES, run_plan, set_mode
from test_gpu_decorated import perm_scores, restated_counts
from test_gpu_exchange import check_merged, run_ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu


def assert_levels(got, want, L):
    for name, lst in LST.items():
        if name in got:
            assert_same_result(got[name], want[lst])
    assert sum(name in got for name in LST) == L


# ---------------------------------------------------------------------------------------------------------------------
# 1. the cohort limit: carrier counts between 2^15 and 2^16
# ---------------------------------------------------------------------------------------------------------------------
COHORTS = {
    # name: cases, controls, method, path length.  65,280 = 1,020 words (TD 65,281): the largest cohort on the IE, sparse
    # and ladder path; 65,281 = the first dense-only cohort (Wp 1,024, TD 65,537); 65,536 = R's limit (a count of 2^16)
    "n65280_m1": (60000, 5280, "method1", 4),
    "n65280_m2": (5280, 60000, "method2", 5),
    "n65281_m1": (60000, 5281, "method1", 4),
    "n65536_m2": (60000, 5536, "method2", 5),
    "n65536_m1": (60000, 5536, "method1", 4),
}
ALL_GENE = 11          # the gene every patient carries (count = n)


def cohort_problem(nc, nt, method, L, K, seed):
    """A 28-gene / 65-relation network whose genes carry 30-70 % of the larger class and 1-3 % of the smaller one (path
    unions of 40,000-60,000 carriers), one gene carried by every patient, and for method 2 every third relation negative
    (dense genes in both halves).  The full (nc+1) x (nt+1) chi-square stand-in table; host-drawn masks."""
    rng = np.random.default_rng(seed)
    g, src, trg, sign = synth.signed_network(28, 65, rng)
    if method == "method2":
        sign = np.where(np.arange(len(sign)) % 3 == 0, -1, 1).astype(np.int32)
    levels = synth.build_level_tables(g, src, trg, sign)
    n = nc + nt
    big = (np.arange(n) < nc) == (nc > nt)
    rate = np.where(big[None, :], rng.uniform(0.3, 0.7, (g, 1)), rng.uniform(0.01, 0.03, (g, 1)))
    data1 = (rng.random((g, n)) < rate).astype(np.int32)
    data1[ALL_GENE] = 1
    masks = synth.packed_case_masks(nc, nt, K, rng)
    p = synth.Problem(method, nc, nt, L, 20, K, levels, data1, data1[levels.uids["1b"].src], bench.fast_table(nc, nt),
                      np.zeros((0, 0), np.int32), seed)
    return p, masks


@pytest.fixture(scope="module")
def cohort(request):
    nc, nt, method, L = COHORTS[request.param]
    p, masks = cohort_problem(nc, nt, method, L, 257, 60 + list(COHORTS).index(request.param))
    assert (nc + nt + 63) // 64 == {65280: 1020, 65281: 1021, 65536: 1024}[nc + nt]
    return request.param, p, masks, oracle.process_paths(p, order="canonical", nthreads=8, packed_masks=masks)


def biggest_path(got):
    return max(int((r.cases + r.ctrls).max()) for r in got.values())


@pytest.mark.parametrize("kernel", MODES)
@pytest.mark.parametrize("cohort", ["n65280_m1", "n65280_m2"], indirect=True)
def test_largest_ie_cohort_in_every_form(cohort, kernel, monkeypatch):
    """65,280 patients, K = 257: every kernel form, counts with bits 14 and 15 set in 16 counter planes."""
    name, p, masks, want = cohort
    set_mode(monkeypatch, kernel)
    got, prof, windows = run_plan(p, masks)
    assert_levels(got, want, p.path_length)
    assert biggest_path(got) >= 40000 and len(got["1b"].null) == 257
    if kernel not in ("sparse", "dense"):
        assert prof["ie_launches"] > 0


@pytest.mark.parametrize("kernel", MODES)
@pytest.mark.parametrize("cohort", ["n65281_m1", "n65536_m2", "n65536_m1"], indirect=True)
def test_past_the_ie_limit_every_form_is_dense(cohort, kernel, monkeypatch):
    """65,281 and 65,536 patients (TD 65,537: no ladder, no IE, no sparse kernel): whatever form is asked for, the dense
    kernel runs, and its results stay exact up to a count of 2^16 (the all-carrier gene)."""
    name, p, masks, want = cohort
    set_mode(monkeypatch, kernel)
    got, prof, windows = run_plan(p, masks)
    assert_levels(got, want, p.path_length)
    assert prof["ie_launches"] == 0
    assert biggest_path(got) >= 40000
    if p.method == "method1":     # paths through the all-carrier gene: a count of n (2^16 at R's limit)
        assert any((w.all_cases + w.all_ctrls == p.n_cases + p.n_ctrls).any() for k, w in want.items() if k.startswith("lst"))


@pytest.mark.parametrize("cohort", ["n65280_m1"], indirect=True)
def test_largest_ie_cohort_in_two_windows(cohort, monkeypatch):
    """The same cohort, K = 2,300 with one-tile windows: two windows, the second 252 permutations long."""
    name, p0, _, _ = cohort
    K = 2300
    p = dataclasses.replace(p0, iterations=K)
    masks = synth.packed_case_masks(p.n_cases, p.n_ctrls, K, np.random.default_rng(9))
    want = oracle.process_paths(p, order="canonical", nthreads=8, packed_masks=masks)
    monkeypatch.setenv("GCRE_WINDOW_TILES", "1")
    got, prof, windows = run_plan(p, masks)
    assert windows == 2 and len(got["4"].null) == K
    assert prof["ie_launches"] > 0
    assert_levels(got, want, p.path_length)


# ---------------------------------------------------------------------------------------------------------------------
# 2. permutation counts past 2^16
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def topk_limit():
    """configs[2]'s cohort (2,500 + 2,500, 79 words), K = 10,000 host-drawn, top_k = 10,000 (R's limit) on a network with
    14,000 level-4 paths: the top-k selection cuts at the limit."""
    nc = nt = 2500
    p = make_problem(100, 500, nc, nt, 10000, 4, method="method1", top_k=10000, seed=71, table=bench.fast_table(nc, nt))
    assert p.levels.n_paths["4"] > 10000
    return p, oracle.process_paths(p, order="canonical", nthreads=8)


@pytest.mark.parametrize("tiles", [None, 2])
def test_top_k_at_the_limit_with_10000_permutations(topk_limit, tiles, monkeypatch):
    p, want = topk_limit
    if tiles:
        monkeypatch.setenv("GCRE_WINDOW_TILES", str(tiles))
    got, prof, windows = run_plan(p)
    assert windows == (3 if tiles else 1)
    assert len(got["4"].scores) == 10000 and len(got["4"].null) == 10000
    assert_levels(got, want, 4)


PERM_CASES = {
    # name: genes, edges, cases, controls, permutations, length, method, mask seed
    "k65537_m1": (20, 40, 5000, 5000, 65537, 4, "method1", 7001),
    "k100000_m1": (20, 40, 5000, 5000, 100000, 4, "method1", 7002),
    "k100000_m2": (20, 40, 5000, 5000, 100000, 4, "method2", 7002),
    "k100000_w782_m2": (12, 22, 25000, 25000, 100000, 5, "method2", 7003),
}
_MASKS: dict = {}


def device_masks(nc, nt, K, seed):
    """The masks gcre_generate_perm_masks draws for (seed, cohort), read back one permutation at a time: uint64 [K][W]."""
    key = (nc, nt, K, seed)
    if key not in _MASKS:
        _MASKS.clear()
        ex = api.JoinExec("method1", nc, nt, K)
        try:
            ex.generate_permutations(seed)
            _MASKS[key] = np.stack([ex.perm_mask(r) for r in range(K)])
        finally:
            ex.close()
    return _MASKS[key]


def corner_table(nc, nt, m):
    spec = importlib.util.spec_from_file_location("decorated_time", os.path.join(ROOT, "tools", "decorated_time.py"))
    dt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dt)
    return dt.corner_table(nc, nt, m)


@pytest.fixture(scope="module")
def perms(request):
    """Built with no permutations and given K afterwards, as bench.build_inputs does (no K x n label matrix); masks drawn
    on the device and read back for the oracle.  The 50,000-patient table is the 8,001 x 8,001 corner (-1 beyond)."""
    genes, edges, nc, nt, K, L, method, seed = PERM_CASES[request.param]
    table = bench.fast_table(nc, nt) if nc + nt <= 10000 else corner_table(nc, nt, 8000)
    p = make_problem(genes, edges, nc, nt, 0, L, method=method, top_k=20, seed=seed, table=table)
    p.iterations = K
    masks = device_masks(nc, nt, K, seed)
    return p, masks, seed, oracle.process_paths(p, order="canonical", nthreads=8, packed_masks=masks)


@pytest.mark.parametrize("kernel", ["auto", "sparse"])
@pytest.mark.parametrize("perms", list(PERM_CASES), indirect=True)
def test_device_masks_past_2_16(perms, kernel, monkeypatch):
    """Device-drawn masks at r >= 65,536 against the oracle; the same masks uploaded (k_masks_from_words) give the same
    results."""
    p, masks, seed, want = perms
    set_mode(monkeypatch, kernel)
    got, prof, windows = run_plan(p, seed=seed)
    assert windows == 1 and len(got["1b"].null) == p.iterations
    assert_levels(got, want, p.path_length)
    up, _, _ = run_plan(p, masks)
    for name in got:
        assert_same_result(up[name], got[name])


@pytest.mark.parametrize("tiles,n_windows", [(7, 7), (1, 49)])
@pytest.mark.parametrize("perms", ["k100000_m1", "k100000_m2"], indirect=True)
def test_windows_past_2_16(perms, tiles, n_windows, monkeypatch):
    """K = 100,000 (49 tiles) in windows of 7 tiles and of one tile: windows that start past 65,536."""
    p, masks, seed, want = perms
    monkeypatch.setenv("GCRE_WINDOW_TILES", str(tiles))
    got, prof, windows = run_plan(p, seed=seed)
    assert windows == n_windows and len(got["4"].null) == p.iterations
    assert_levels(got, want, p.path_length)


@pytest.fixture(scope="module")
def label_matrix():
    """K = 100,000 permutations as a K x n label matrix (R's getCaseORControl form, 256 MB) on 300 + 340 patients."""
    p = make_problem(40, 110, 300, 340, 100000, 4, method="method1", top_k=15, seed=73, table=bench.fast_table(300, 340))
    return p, oracle.process_paths(p, order="canonical", nthreads=8)


def test_label_matrix_past_2_16_single_call(label_matrix):
    p, want = label_matrix
    got = api.process_paths(p)
    for lvl in range(1, 5):
        assert_same_result(got[f"lst{lvl}"], want[f"lst{lvl}"])
    assert len(got["lst4"].null) == 100000


def test_label_matrix_past_2_16_two_contexts(label_matrix):
    p, want = label_matrix
    got = api.process_paths_devices(p, devices=[0, 0])
    for lvl in range(1, 5):
        assert_same_result(got[f"lst{lvl}"], want[f"lst{lvl}"])


def test_label_matrix_past_2_16_two_ranks(label_matrix):
    p, want = label_matrix
    parts, calls, counts = run_ranks(p, 2, p.iterations)
    check_merged(parts, want, p, 4)
    assert all(len(r["4"].null) == p.iterations for r in parts)


@pytest.mark.parametrize("stratified", [False, True])
def test_mask_restatement_past_2_16(stratified):
    """k_generate_masks bit for bit at the tile edges, at 2^16 - 1 .. 2^16 + 1, at K - 1 and at 16 random permutations."""
    nc, nt, K, seed = 400, 600, 100000, 20261016
    n = nc + nt
    strata = (np.arange(n) * 7 % 5).astype(np.int32) if stratified else None
    rows = [0, 2047, 2048, 65535, 65536, 65537, K - 1] + np.random.default_rng(3).integers(0, K, 16).tolist()
    ex = api.JoinExec("method1", nc, nt, K)
    try:
        ex.generate_permutations(seed, strata)
        got = [sum(int(w) << (64 * k) for k, w in enumerate(ex.perm_mask(r))) for r in rows]
    finally:
        ex.close()
    assert got == _masks_restated(seed, K, n, nc, strata, rows=rows)
    assert all(bin(b).count("1") == nc for b in got)


# ---------------------------------------------------------------------------------------------------------------------
# 3. decorated p-values at the same limits
# ---------------------------------------------------------------------------------------------------------------------
def check_decorated(method, nc, nt, K, paths, data, signs, VT, strata, seed):
    """k_decorated_null's perm_counts, n_ge and p-values against the restatement; observed values against the host stage."""
    ex = api.JoinExec(method, nc, nt, K)
    try:
        ex.set_value_table(VT)
        rec, counts = ex.decorated_pvalues(paths, data, signs, strata=strata, seed=seed, return_counts=True)
    finally:
        ex.close()
    host, st = api.decorated_splits(method, nc, nt, paths, data, signs, VT, strata)
    for f in ("path", "direction", "j", "valid", "cases1", "ctrls1", "cases2", "ctrls2", "k_pos", "k_neg"):
        np.testing.assert_array_equal(rec[f], host[f])
    np.testing.assert_array_equal(rec["score"].view(np.uint64), host["score"].view(np.uint64))
    want = restated_counts(host, st, seed, K)
    np.testing.assert_array_equal(counts, want)
    for s, r in enumerate(host):
        n_ge = int((perm_scores(r, want[s, :, 0], want[s, :, 1], method, VT) >= r["score"]).sum())
        assert int(rec[s]["n_ge"]) == n_ge, s
        assert rec[s]["pvalue"] == n_ge / K
    return host, st


def limit_strata(nc, n):
    """64 strata: 62 random ones, a one-patient stratum (62) and a stratum of controls only (63)."""
    strata = np.random.default_rng(17).integers(0, 62, n).astype(np.int32)
    strata[nc + 5] = 62
    strata[nc + 100:nc + 400] = 63
    return strata


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("cohort", ["n65536_m2"], indirect=True)
def test_decorated_at_the_cohort_limit(cohort, method):
    """65,536 patients, K = 2,000: draws of tens of thousands of carriers, the all-carrier gene, 64 strata of which a
    sparse gene's draws reach only a few."""
    name, p, _, _ = cohort
    nc, nt = p.n_cases, p.n_ctrls
    n = nc + nt
    sparse = np.zeros((1, n), np.int32)
    sparse[0, np.random.default_rng(4).choice(n, 12, replace=False)] = 1
    data = np.vstack([p.data1, sparse])
    S = len(data) - 1
    paths = [[0, 1, 2], [ALL_GENE, 3], [4, ALL_GENE, 5], [6, 7], [8, S]]
    signs = [[1, -1, 1], [-1, 1], [1, 1, -1], [1, -1], [1, 1]]
    host, st = check_decorated(method, nc, nt, 2000, paths, data, signs, p.value_table, limit_strata(nc, n), 5)
    assert int((host["k_pos"] + host["k_neg"]).max()) >= 10000
    drawing = [int(((x["k_pos"] + x["k_neg"]) > 0).sum()) for x in st]      # strata that draw, per split
    assert len(st[0]) == 64 and min(d for d in drawing if d) <= 12 and max(drawing) >= 60


@pytest.mark.parametrize("K,method,stratified", [(65537, 1, False), (100000, 2, True), (100000, 1, False)])
def test_decorated_past_2_16_permutations(K, method, stratified):
    nc, nt, data, paths, signs, VT = random_case(600 + method, method)
    strata = (np.arange(nc + nt) * 7 % 3).astype(np.int32) if stratified else None
    host, _ = check_decorated(method, nc, nt, K, paths, data, signs, VT, strata, 77)
    assert host["valid"].sum() > 10
