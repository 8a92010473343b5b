"""Greedy clumping on the device (gcre_clump_sets: k_clump_union, k_clump_leads, k_clump_assign) against
``report.clump_rows`` fed from ``report.overlap_reference``: clump, lead, value (as bits), shared and size, every one exact
(pytest -m gpu).  The cases and what they must hold come from tests/test_clump_host.py.

GCRE_CLUMP_FUZZ_CASES=500 [GCRE_CLUMP_FUZZ_BASE=...] for a long run of the seeded loop at the end (GCRE_CLUMP_FUZZ_OUT: a
file for its summary); a handful by default."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from geneticscre_amd import api, report
from test_clump_host import _CACHE, SHAPES, check_generator, make_case, reference

pytestmark = pytest.mark.gpu

MEASURES = [(m, p) for m in ("jaccard", "containment") for p in ("all", "cases")]


def same(got, want, what=""):
    """(clump, lead, value, shared, size) against the reference's: integers as integers, value by its bits."""
    for name, g, w in zip(("clump", "lead", "value", "shared", "size"), got, want):
        if name == "value":
            np.testing.assert_array_equal(np.asarray(g, np.float64).view(np.uint64), np.asarray(w, np.float64).view(np.uint64),
                                          err_msg=f"value {what}")
        else:
            np.testing.assert_array_equal(np.asarray(g, np.int64), np.asarray(w, np.int64), err_msg=f"{name} {what}")


def case_of(rows, sets, nc, order=None):
    rows = np.asarray(rows)
    return dict(n=rows.shape[1], nc=nc, rows=rows, sets=sets, order=np.arange(len(sets)) if order is None else np.asarray(order))


def run(case, r, measure="jaccard", patients="all", order=None, method=1):
    ex = api.JoinExec(method, case["nc"], case["n"] - case["nc"], 0)
    try:
        return ex.clump_sets(case["sets"], case["rows"], case["order"] if order is None else order, r, measure, patients)
    finally:
        ex.close()


def raw_clump(ex, sets, packed, n_cols, order, r=0.5, measure=0, patients=0, signs=None, n_order=None, want_size=True):
    """gcre_clump_sets through the C entry: (rc, clump, lead, value, shared, size)."""
    lib = api._clump_lib()
    S = len(sets)
    off = np.zeros(S + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in sets])
    mem = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int64) for s in sets]) if S else np.zeros(0), np.int32)
    sg = None if signs is None else np.ascontiguousarray(np.concatenate([np.asarray(s, np.int64) for s in signs]), np.int32)
    io = None if order is None else np.ascontiguousarray(order, np.int64)
    n_order = (0 if io is None else len(io)) if n_order is None else n_order
    inp = api.gcre_set_input(S, api._ptr(off), api._ptr(mem), api._ptr(sg), api._ptr(packed), len(packed), n_cols)
    size = np.full((S, 2), -7, np.int32) if want_size else None
    clump, lead = np.full(S, -7, np.int64), np.full(S, -7, np.int64)
    value, shared = np.full(S, -7.0), np.full((S, 2), -7, np.int32)
    rc = lib.gcre_clump_sets(ex._h, ctypes.byref(inp), api._ptr(io), n_order, r, measure, patients, api._ptr(size),
                             api._ptr(clump), api._ptr(lead), api._ptr(value), api._ptr(shared))
    return rc, clump, lead, value, shared, size


# ---- 1. the three shapes, every measure, r = 0.5 / 0.8 / 1.0 ------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=[f"seed{s[0]}" for s in SHAPES])
def test_shapes_against_the_reference(shape):
    case = make_case(*shape)
    check_generator(case)
    ex = api.JoinExec(1, case["nc"], case["n"] - case["nc"], 0)
    launches = 0
    try:
        for measure, patients in MEASURES:
            for r in (0.5, 0.8, 1.0):
                got = ex.clump_sets(case["sets"], case["rows"], case["order"], r, measure, patients)
                assert [a.dtype for a in got] == [np.int64, np.int64, np.float64, np.int64, np.int32]
                want = reference(case, r, measure, patients)
                same(got, want, f"{measure} {patients} r={r}")
                leads = int((want[1] == np.arange(len(want[1]))).sum())
                # the union, then whole batches of rounds, two kernels each: at least ceil(leads / 64) rounds
                now = ex.clump_launches
                assert (now - launches - 1) % 2 == 0 and (now - launches - 1) // 2 >= -(-leads // 64)
                launches = now
    finally:
        ex.close()


# ---- 2. edges -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_order", [1, 63, 64, 65, 129])
def test_walks_around_the_candidate_count(n_order):
    case = make_case(*SHAPES[1])
    order = case["order"][:n_order]
    for r in (0.5, 0.8):
        same(run(case, r, order=order), reference(case, r, order=order), f"n_order {n_order} r={r}")


def rounds_of(capfd):
    return [int(x) for x in re.findall(r"clump rows=\d+ rounds=(\d+) ", capfd.readouterr().err)]


def test_identical_rows_make_one_clump(monkeypatch, capfd):
    monkeypatch.setenv("GCRE_CLUMP_STATS", "1")
    rng = np.random.default_rng(5)
    rows = (rng.random((3, 90)) < 0.3).astype(np.int8)
    case = case_of(rows, [[1]] * 150, 40)
    got = run(case, 1.0)
    same(got, reference(case, 1.0))
    assert (got[0] == 0).all() and (got[1] == 0).all() and np.isnan(got[2][0]) and (got[2][1:] == 1.0).all()
    assert rounds_of(capfd) == [1]


def test_disjoint_rows_are_all_leads(monkeypatch, capfd):
    monkeypatch.setenv("GCRE_CLUMP_STATS", "1")
    n = 130
    case = case_of(np.eye(n, dtype=np.int8), [[i] for i in range(n)], 50, order=np.random.default_rng(1).permutation(n))
    got = run(case, 1.0)
    same(got, reference(case, 1.0))
    assert sorted(got[0].tolist()) == list(range(n)) and (got[1] == np.arange(n)).all() and np.isnan(got[2]).all()
    assert rounds_of(capfd) == [-(-n // 64)]


def test_a_set_without_carriers_stays_alone():
    rng = np.random.default_rng(6)
    rows = (rng.random((5, 70)) < 0.3).astype(np.int8)
    rows[0] = 0
    case = case_of(rows, [[1], [0], [1, 2], [0, 0], [1]], 30)
    for measure, patients in MEASURES:
        got = run(case, 0.01, measure, patients)
        same(got, reference(case, 0.01, measure, patients), f"{measure} {patients}")
        assert got[1][1] == 1 and got[1][3] == 3 and got[0][1] != got[0][3]     # two empty sets: two clumps of one
        assert got[4][1].tolist() == [0, 0]


def test_order_a_shuffled_strict_subset():
    case = make_case(*SHAPES[0])
    order = np.random.default_rng(9).permutation(300)[:171]
    got = run(case, 0.5, order=order)
    same(got, reference(case, 0.5, order=order))
    out = np.setdiff1d(np.arange(300), order)
    assert (got[0][out] == -1).all() and (got[1][out] == -1).all() and np.isnan(got[2][out]).all() and (got[3][out] == -1).all()
    assert (got[4][out] >= 0).all()                      # the sizes come for every set
    empty = run(case, 0.5, order=[])                     # nothing to walk: the outputs are filled, the sizes come
    assert (empty[0] == -1).all() and np.isnan(empty[2]).all()
    np.testing.assert_array_equal(empty[4], got[4])


def test_six_members_with_a_repeat_and_an_na_set_outside_the_order():
    rng = np.random.default_rng(11)
    rows = (rng.random((12, 200)) < 0.06).astype(np.int8)
    sets = []
    for _ in range(100):
        m = rng.integers(0, 12, 6)
        m[5] = m[0]
        sets.append(m.tolist())
    sets.append([3, -1, 4])                              # an NA member: not in the order, size (-1, -1)
    case = case_of(rows, sets, 90, order=rng.permutation(100))
    got = run(case, 0.5)
    same(got, reference(case, 0.5))
    assert got[4][100].tolist() == [-1, -1] and got[0][100] == -1


def test_signs_and_the_method_change_nothing():
    case = make_case(*SHAPES[1])
    want = reference(case, 0.8)
    packed = api.pack_carriers(case["rows"], case["n"])
    rng = np.random.default_rng(12)
    signs = [rng.choice([-1, 1], len(s)).tolist() for s in case["sets"]]
    ex = api.JoinExec(2, case["nc"], case["n"] - case["nc"], 0)
    rc, *got = raw_clump(ex, case["sets"], packed, case["n"], case["order"], r=0.8, signs=signs)
    rc0, *got0 = raw_clump(ex, case["sets"], packed, case["n"], case["order"], r=0.8)
    ex.close()
    assert rc == api.GCRE_OK and rc0 == api.GCRE_OK
    same(got, want, "signs")
    same(got0, want, "no signs")


def test_stray_bits_beyond_the_patients_are_not_counted():
    n, nc = 33, 11
    rng = np.random.default_rng(33)
    rows = (rng.random((10, n)) < 0.25).astype(np.int8)
    sets = [rng.integers(0, 10, int(rng.integers(1, 4))).tolist() for _ in range(90)]
    case = case_of(rows, sets, nc, order=rng.permutation(90))
    packed = api.pack_carriers(rows, n)
    packed[:, -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)
    ex = api.JoinExec(1, nc, n - nc, 0)
    for measure, patients in ((0, 0), (1, 1)):
        rc, *got = raw_clump(ex, sets, packed, n, case["order"], r=0.5, measure=measure, patients=patients)
        assert rc == api.GCRE_OK
        same(got, reference(case, 0.5, ("jaccard", "containment")[measure], ("all", "cases")[patients]))
    rc, *got = raw_clump(ex, sets, packed, n, case["order"], want_size=False)      # size may be NULL
    assert rc == api.GCRE_OK and got[4] is None
    same(got[:4], reference(case, 0.5)[:4])
    ex.close()


def test_width_limit():
    """65,536 patients, 256 sets."""
    n, nc = 65536, 30001
    rng = np.random.default_rng(65536)
    rows = (rng.random((32, n)) < np.linspace(0.02, 0.6, 32)[:, None]).astype(np.int8)
    rows[0], rows[1] = 1, 0
    sets = [rng.integers(0, 32, int(rng.integers(1, 6))).tolist() for _ in range(256)]
    sets[0], sets[1] = [0], [1]
    case = case_of(rows, sets, nc, order=rng.permutation(256))
    same(run(case, 0.8), reference(case, 0.8))


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(monkeypatch):
    n, nc = 45, 20
    rng = np.random.default_rng(3)
    rows = (rng.random((6, n)) < 0.3).astype(np.int8)
    packed = api.pack_carriers(rows, n)
    ex = api.JoinExec(2, nc, n - nc, 0)
    good = [[0], [2, 3], [4, -1], [5]]
    lib = api._clump_lib()
    monkeypatch.delenv("GCRE_CLUMP_MAX_MB", raising=False)

    def failed(res, code, text):
        msg = ex._lib.gcre_last_error(ex._h)
        assert res[0] == code and text in msg, (res[0], msg)
        assert ex.clump_launches == 0

    ARG, RANGE = api.GCRE_ERR_ARG, api.GCRE_ERR_RANGE
    failed(raw_clump(ex, good, packed, n + 1, [0]), ARG, b"clump_sets: the rows have 46 columns")
    failed(raw_clump(ex, [[0], []], packed, n, [0]), ARG, b"clump_sets: set 1 has no members")
    failed(raw_clump(ex, [[0], [6]], packed, n, [0]), RANGE, b"clump_sets: set 1: member row 6 out of range")
    for r in (0.0, -1.0, 1.5, float("nan"), float("inf")):
        failed(raw_clump(ex, good, packed, n, [0, 1], r=r), ARG, b"clump_sets: r must be > 0 and <= 1")
    for m in (-1, 2):
        failed(raw_clump(ex, good, packed, n, [0, 1], measure=m), ARG, b"clump_sets: measure must be 0")
        failed(raw_clump(ex, good, packed, n, [0, 1], patients=m), ARG, b"clump_sets: patients must be 0")
    failed(raw_clump(ex, good, packed, n, [0, 4]), RANGE, b"clump_sets: order[1] = 4 out of range (4 sets)")
    failed(raw_clump(ex, good, packed, n, [-1]), RANGE, b"clump_sets: order[0] = -1 out of range")
    failed(raw_clump(ex, good, packed, n, [1, 3, 1]), ARG, b"clump_sets: order[2] = 1 is listed twice")
    failed(raw_clump(ex, good, packed, n, [0, 2]), ARG, b"clump_sets: order[1] = 2 names a set with an NA member")
    failed(raw_clump(ex, good, packed, n, None, n_order=2), ARG, b"clump_sets: bad order")
    failed((lib.gcre_clump_sets(ex._h, None, None, 0, 0.5, 0, 0, None, None, None, None, None),), ARG, b"NULL argument")
    monkeypatch.setenv("GCRE_CLUMP_MAX_MB", "0.001")           # 1048 bytes: 8 rows of 128 bytes
    many = [[i % 6] for i in range(9)]
    failed(raw_clump(ex, many, packed, n, np.arange(9)), ARG, b"clump_sets: 9 rows of 128 bytes exceed GCRE_CLUMP_MAX_MB")
    assert raw_clump(ex, many, packed, n, np.arange(8))[0] == api.GCRE_OK and ex.clump_launches > 0
    monkeypatch.delenv("GCRE_CLUMP_MAX_MB")
    # the Python method: its own ValueErrors, and the library's message
    before = ex.clump_launches
    with pytest.raises(ValueError, match="r must be"):
        ex.clump_sets(good, rows, [0], r=0.0)
    with pytest.raises(api.GcreError, match="is listed twice"):
        ex.clump_sets(good, rows, [0, 0])
    with pytest.raises(api.GcreError, match=r"order\[0\] = 7 out of range"):
        ex.clump_sets(good, rows, [7])
    assert ex.clump_launches == before
    # the context still works
    case = case_of(rows, good, nc, order=[3, 0, 1])
    same(ex.clump_sets(good, rows, [3, 0, 1], 0.2), reference(case, 0.2))
    size, both = ex.set_overlap(good, rows)
    np.testing.assert_array_equal(size, report.overlap_reference(good, rows, nc, n - nc)[0])
    ex.close()


# ---- 4. the front end -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("signed", [False, True])
def test_clump_paths_on_device_equals_the_old_road(signed):
    import pandas as pd
    from test_gpu_overlap import NC, NT, K_PERM, THRESHOLD, SEED, _problem
    symbols, data, network, strata = _problem()
    table = report.gwaspa(symbols, data, NC, NT, network, signed=signed, threshold=THRESHOLD, top_k=200, path_length=5,
                          n_permutations=K_PERM, strata=strata, seed=SEED)["GWASPA.Results"]
    assert 900 < len(table) <= 1000           # 200 per length; level 1 has fewer genes than that
    ckw = dict(signed=signed, threshold=THRESHOLD)
    for kw in (dict(r=0.5), dict(r=0.8, measure="containment"), dict(r=0.5, patients="cases", by_length=True)):
        old = report.clump_paths(table, symbols, data, NC, NT, **ckw, **kw)
        new = report.clump_paths(table, symbols, data, NC, NT, on_device=True, **ckw, **kw)
        assert list(new.columns) == list(table.columns) + report.CLUMP_COLUMNS
        pd.testing.assert_frame_equal(new, old, check_exact=True)
        np.testing.assert_array_equal(new["LeadOverlap"].to_numpy().view(np.uint64), old["LeadOverlap"].to_numpy().view(np.uint64))
        assert new["Clump"].max() >= 1 and (new["ClumpSize"] > 1).any()
        print(f"clump_paths {kw}: {int(new['Clump'].max()) + 1} clumps of {len(new)} rows")


@pytest.mark.parametrize("signed", [False, True])
def test_gwaspa_clump_significant(signed):
    import pandas as pd
    from test_gpu_hits import _network_case
    nc, nt = 48, 52
    genes, data, network = _network_case(17)
    strata = (np.arange(nc + nt) * 5 % 3).astype(np.int32)
    kw = dict(signed=signed, threshold=0.2, n_permutations=1000, strata=strata, seed=909, path_length=5)
    # the problem has no planted signal: the level is the largest p-value below 1 that any path has
    full = report.gwaspa(genes, data, nc, nt, network, top_k=2000, **kw)["GWASPA.Results"]
    pv = full["Pvalues"].to_numpy(np.float64)[np.isfinite(full["Scores"].to_numpy(np.float64))]
    alpha = float(pv[pv < 1].max())
    kw.update(top_k=3, significant=alpha, clump=0.5)
    base = report.gwaspa(genes, data, nc, nt, network, **kw)
    got = report.gwaspa(genes, data, nc, nt, network, clump_significant=True, **kw)
    sig = got["Significant.Results"]
    print(f"Significant.Results at {alpha}: {len(sig)} rows, lengths {sorted(set(sig['Lengths']))}, {sig['Clump'].max() + 1} clumps")
    assert list(sig.columns) == report.COLUMNS + report.CLUMP_COLUMNS and len(sig) > 3
    assert len(set(sig["Lengths"])) > 1
    # the clump columns: clump_paths by the old road, over the printed paths
    want = report.clump_paths(base["Significant.Results"], genes, data, nc, nt, signed=signed, r=0.5, threshold=0.2)
    pd.testing.assert_frame_equal(sig, want, check_exact=True)
    np.testing.assert_array_equal(sig["LeadOverlap"].to_numpy().view(np.uint64), want["LeadOverlap"].to_numpy().view(np.uint64))
    assert (sig["ClumpSize"] > 1).any()
    # every other key is what it is without
    assert set(got) == set(base)
    for key in base:
        if key == "Significant.Results":
            pd.testing.assert_frame_equal(sig[report.COLUMNS], base[key], check_exact=True)
        elif isinstance(base[key], pd.DataFrame):
            pd.testing.assert_frame_equal(got[key], base[key], check_exact=True)
    for L in base["significant"]:
        for f in ("score", "ordinal", "src", "trg", "cases", "ctrls"):
            assert getattr(got["significant"][L], f).tobytes() == getattr(base["significant"][L], f).tobytes(), (L, f)
        for f in ("scores", "src", "trg", "cases", "ctrls", "null"):
            assert getattr(got["levels"][f"lst{L}"], f).tobytes() == getattr(base["levels"][f"lst{L}"], f).tobytes(), (L, f)
    assert got["significant_cutoffs"] == base["significant_cutoffs"]


# ---- 5. seeded loop -----------------------------------------------------------------------------------------------------------
N_FUZZ = int(os.environ.get("GCRE_CLUMP_FUZZ_CASES", "6"))
FUZZ_BASE = int(os.environ.get("GCRE_CLUMP_FUZZ_BASE", "0"))


def test_seeded_loop():
    lines = []
    for k in range(FUZZ_BASE, FUZZ_BASE + N_FUZZ):
        rng = np.random.default_rng(7_000_000 + k)
        n = int(rng.choice([int(rng.integers(2, 70)), int(rng.integers(70, 1100)), int(rng.integers(1100, 2300))]))
        nc = int(rng.integers(1, n))
        R, S = int(rng.integers(4, 50)), int(rng.integers(1, 500))
        rows = (rng.random((R, n)) < rng.choice([0.02, 0.08, 0.3])).astype(np.int8)
        rows[:3] = rng.random((3, n)) < 0.4
        sets = []
        for _ in range(S):
            m = rng.integers(3, R, int(rng.integers(1, 7)))
            if rng.random() < 0.6:
                m[int(rng.integers(0, len(m)))] = int(rng.integers(0, 3))
            sets.append(m.tolist())
        order = rng.permutation(S)[:int(rng.integers(0, S + 1))]
        measure, patients = MEASURES[int(rng.integers(0, 4))]
        r = float(rng.choice([0.25, 1 / 3, 0.5, 0.8, 1.0, rng.uniform(0.05, 1.0)]))
        case = case_of(rows, sets, nc, order=order)
        want = reference(case, r, measure, patients)
        same(run(case, r, measure, patients, method=1 + k % 2), want, f"case {k}")
        leads = int((want[1] == np.arange(S)).sum())
        _CACHE.clear()
        lines.append(f"case {k}: patients {n} cases {nc} rows {R} sets {S} walked {len(order)} {measure} {patients} "
                     f"r {r:.6g} leads {leads} ok")
    out = os.environ.get("GCRE_CLUMP_FUZZ_OUT")
    if out:
        with open(out, "w") as f:
            f.write(f"test_gpu_clump.py::test_seeded_loop: cases {FUZZ_BASE}..{FUZZ_BASE + N_FUZZ - 1}, every one exact\n")
            f.write("\n".join(lines) + "\n")
