"""Carrier overlaps on the device (gcre_set_overlap / k_set_overlap): exact against report.overlap_reference over patient
counts, case / control splits, index lists around the kernel's tile edge, contexts, stray bits, slabs and the width limit;
the argument errors; and the front end -- gwaspa(clump=...) / clump_paths against a brute-force clumping and against
score_paths on datasets whose lead-carrier columns the test zeroed by hand."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from geneticscre_amd import api, report, synth
from helpers import small_table
from test_gpu_sets import random_sets
from test_overlap_host import brute_clumps

pytestmark = pytest.mark.gpu

T = api.OVERLAP_TILE


def carrier_matrix(rng, n, R=16):
    """R rows at densities 0.02 .. 0.6; row 0 all ones, row 1 all zeros."""
    rows = (rng.random((R, n)) < np.linspace(0.02, 0.6, R)[:, None]).astype(np.int8)
    rows[0], rows[1] = 1, 0
    return rows


def case_counts(n):
    """n_cases with n_cases % 32 in {0, 1, 31} (the smallest, a middle one and the largest of each), 1 and n - 1, and
    around the first chunk edge of the kernel (32 dwords: the split dword last in its chunk, first in the next one)."""
    out = {1, n - 1}
    for res in (0, 1, 31):
        cs = [c for c in range(1, n) if c % 32 == res]
        if cs:
            out |= {cs[0], cs[len(cs) // 2], cs[-1]}
    out |= {c for c in (992, 1023, 1024, 1025) if c < n}
    return sorted(c for c in out if 1 <= c <= n - 1)


def raw_overlap(ex, sets, packed, n_cols, a=None, b=None, na=None, nb=None, want_size=True, want_both=True, signs=None):
    """gcre_set_overlap through the C entry: (rc, size, both)."""
    lib = api._overlap_lib()
    S = len(sets)
    off = np.zeros(S + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in sets])
    mem = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int64) for s in sets]) if S else np.zeros(0), np.int32)
    ia = None if a is None else np.ascontiguousarray(a, np.int64)
    ib = None if b is None else np.ascontiguousarray(b, np.int64)
    na = (S if ia is None else len(ia)) if na is None else na
    nb = (S if ib is None else len(ib)) if nb is None else nb
    sg = None if signs is None else np.ascontiguousarray(np.concatenate([np.asarray(s, np.int64) for s in signs]), np.int32)
    inp = api.gcre_set_input(S, api._ptr(off), api._ptr(mem), api._ptr(sg), api._ptr(packed), len(packed), n_cols)
    size = np.full((S, 2), -7, np.int32) if want_size else None
    both = np.full((max(na, 0), max(nb, 0), 2), -7, np.int32) if want_both else None
    rc = lib.gcre_set_overlap(ex._h, ctypes.byref(inp), api._ptr(ia), na, api._ptr(ib), nb, api._ptr(size), api._ptr(both))
    return rc, size, both


@pytest.mark.parametrize("n", [5, 31, 32, 33, 63, 64, 65, 200, 4999])
def test_every_shape_against_the_reference(n):
    """130 random sets of 1-12 members and the special sets (duplicates, a gene twice, an NA member, the full and the empty
    row), every set against every set, for every split of the n patients into cases and controls listed above; method 1
    and method 2 contexts alternate."""
    rng = np.random.default_rng(500 + n)
    rows = carrier_matrix(rng, n)
    sets, _ = random_sets(rng, 16, 135)
    for i, nc in enumerate(case_counts(n)):
        want_size, want_both = report.overlap_reference(sets, rows, nc, n - nc)
        ex = api.JoinExec(1 + i % 2, nc, n - nc, 0)
        size, both = ex.set_overlap(sets, rows)
        assert size.dtype == np.int32 and both.dtype == np.int32 and both.shape == (135, 135, 2)
        np.testing.assert_array_equal(size, want_size, err_msg=f"n_cases {nc}")
        np.testing.assert_array_equal(both, want_both, err_msg=f"n_cases {nc}")
        assert size[2].tolist() == [-1, -1] and not both[2].any() and not both[:, 2].any()   # the set with an NA member
        assert ex.overlap_launches() == 1
        ex.close()


def test_index_lists_around_the_tile_edge():
    n, nc = 200, 97
    rng = np.random.default_rng(77)
    rows = carrier_matrix(rng, n)
    sets, _ = random_sets(rng, 16, 135)
    _, full = report.overlap_reference(sets, rows, nc, n - nc)
    ex = api.JoinExec(1, nc, n - nc, 0)
    lens = [1, T - 1, T, T + 1, 2 * T + 2]
    for na in lens:
        for nb in lens:
            a, b = rng.integers(0, 135, na), rng.integers(0, 135, nb)   # a != b, with repeats
            if na > 1:
                a[-1] = a[0]
            size, both = ex.set_overlap(sets, rows, a=a, b=b)
            np.testing.assert_array_equal(both, full[a][:, b], err_msg=f"{na} x {nb}")
    a = rng.integers(0, 135, 70)
    np.testing.assert_array_equal(ex.set_overlap(sets, rows, a=a)[1], full[a])
    np.testing.assert_array_equal(ex.set_overlap(sets, rows, b=a)[1], full[:, a])
    np.testing.assert_array_equal(ex.set_overlap(sets, rows)[1], full)
    # nothing to pair: the sizes still come, nothing is launched
    before = ex.overlap_launches()
    size, both = ex.set_overlap(sets, rows, a=[])
    assert both.shape == (0, 135, 2)
    np.testing.assert_array_equal(size, report.overlap_reference(sets, rows, nc, n - nc)[0])
    assert ex.set_overlap(sets, rows, a=[3, 4], b=[])[1].shape == (2, 0, 2)
    assert ex.set_overlap([], rows)[1].shape == (0, 0, 2)
    assert ex.overlap_launches() == before
    ex.close()


def test_contexts_give_the_same_arrays():
    """The carrier row is the OR of all members whatever the method; neither a value table nor masks are needed."""
    n, nc, K = 200, 64, 100
    rng = np.random.default_rng(8)
    rows = carrier_matrix(rng, n)
    sets, _ = random_sets(rng, 16, 135)
    want = report.overlap_reference(sets, rows, nc, n - nc)
    for method in (1, 2):
        bare = api.JoinExec(method, nc, n - nc, K)                 # no value table, no masks
        got = bare.set_overlap(sets, rows)
        bare.close()
        full = api.JoinExec(method, nc, n - nc, K)
        full.set_value_table(small_table(n, n, 2))
        full.generate_permutations(5)
        got2 = full.set_overlap(sets, rows)
        full.close()
        for g, g2, w in zip(got, got2, want):
            np.testing.assert_array_equal(g, w)
            np.testing.assert_array_equal(g2, w)


def test_signs_do_not_split_the_carrier_row():
    """A signed context, signs given: the carrier row is still the OR of ALL members -- the host stage that gcre_score_sets
    splits by sign is the one that builds it.  The same arrays as without signs, and as the numpy OR."""
    n, nc = 70, 31
    rng = np.random.default_rng(70)
    rows = carrier_matrix(rng, n, R=6)
    sets = [[2, 3], [3, 4, 5], [0, -1, 2], [1], [2, 2, 5]]
    signs = [[-1, -1], [1, -1, 1], [1, -1, -1], [-1], [-1, 1, -1]]   # every member (-), mixed, an NA member, the empty row
    carriers = np.array([np.any([rows[m] for m in s], axis=0) for s in sets])
    case = np.arange(n) < nc
    want_size = np.array([[(c & case).sum(), (c & ~case).sum()] for c in carriers], np.int32)
    want_both = np.array([[[(x & y & case).sum(), (x & y & ~case).sum()] for y in carriers] for x in carriers], np.int32)
    want_size[2] = -1
    want_both[2], want_both[:, 2] = 0, 0
    packed = api.pack_carriers(rows, n)
    ex = api.JoinExec(2, nc, n - nc, 0)
    rc, size, both = raw_overlap(ex, sets, packed, n, signs=signs)
    rc0, size0, both0 = raw_overlap(ex, sets, packed, n)
    ex.close()
    assert rc == api.GCRE_OK and rc0 == api.GCRE_OK
    for got, plain, want in ((size, size0, want_size), (both, both0, want_both)):
        np.testing.assert_array_equal(got, plain)
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("n", [33, 200])
def test_stray_bits_beyond_the_patients_are_not_counted(n):
    nc = n // 3
    rng = np.random.default_rng(n)
    rows = carrier_matrix(rng, n)
    sets, _ = random_sets(rng, 16, 135)
    want_size, want_both = report.overlap_reference(sets, rows, nc, n - nc)
    packed = api.pack_carriers(rows, n)
    packed[:, -1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)   # every bit >= n_cols of every row
    ex = api.JoinExec(1, nc, n - nc, 0)
    rc, size, both = raw_overlap(ex, sets, packed, n)
    assert rc == api.GCRE_OK
    np.testing.assert_array_equal(size, want_size)
    np.testing.assert_array_equal(both, want_both)
    # either output may be NULL
    rc, size, _ = raw_overlap(ex, sets, packed, n, want_both=False)
    assert rc == api.GCRE_OK
    np.testing.assert_array_equal(size, want_size)
    rc, _, both = raw_overlap(ex, sets, packed, n, want_size=False)
    assert rc == api.GCRE_OK
    np.testing.assert_array_equal(both, want_both)
    ex.close()


def test_slabs_do_not_change_the_result(monkeypatch):
    n, nc = 300, 130
    rng = np.random.default_rng(21)
    rows = carrier_matrix(rng, n)
    sets = [rng.integers(0, 16, int(rng.integers(1, 6))).tolist() for _ in range(200)]
    want = report.overlap_reference(sets, rows, nc, n - nc)[1]
    ex = api.JoinExec(1, nc, n - nc, 0)
    monkeypatch.delenv("GCRE_OVERLAP_SLAB_MB", raising=False)
    whole = ex.set_overlap(sets, rows)[1]
    assert ex.overlap_launches() == 1
    monkeypatch.setenv("GCRE_OVERLAP_SLAB_MB", "0.1")      # 200 x 200 x 8 bytes = 0.31 MB: slabs of 64 rows of `a`
    slabbed = ex.set_overlap(sets, rows)[1]
    assert ex.overlap_launches() == 1 + 4
    monkeypatch.setenv("GCRE_OVERLAP_SLAB_MB", "0")        # never less than one row of tiles
    least = ex.set_overlap(sets, rows)[1]
    assert ex.overlap_launches() == 1 + 4 + 4
    ex.close()
    np.testing.assert_array_equal(whole, want)
    np.testing.assert_array_equal(slabbed, want)
    np.testing.assert_array_equal(least, want)


def test_width_limit():
    """65,536 patients, 256 x 256 sets."""
    n, nc = 65536, 30001
    rng = np.random.default_rng(65536)
    rows = carrier_matrix(rng, n, R=32)
    sets = [rng.integers(0, 32, int(rng.integers(1, 6))).tolist() for _ in range(256)]
    sets[0], sets[1], sets[2] = [0], [1], [5, -1]
    want_size, want_both = report.overlap_reference(sets, rows, nc, n - nc)
    assert want_both[0][0].tolist() == [nc, n - nc]
    ex = api.JoinExec(1, nc, n - nc, 0)
    size, both = ex.set_overlap(sets, rows)
    ex.close()
    np.testing.assert_array_equal(size, want_size)
    np.testing.assert_array_equal(both, want_both)


def test_errors_launch_nothing():
    n, nc = 45, 20
    rng = np.random.default_rng(3)
    rows = carrier_matrix(rng, n, R=6)
    packed = api.pack_carriers(rows, n)
    ex = api.JoinExec(2, nc, n - nc, 0)
    good = [[0], [2, 3], [4, -1]]

    def failed(rc, code, text):
        msg = ex._lib.gcre_last_error(ex._h)
        assert rc == code and text in msg, (rc, msg)
        assert ex.overlap_launches() == 0

    failed(raw_overlap(ex, good, packed, n, a=[0, 3])[0], api.GCRE_ERR_RANGE, b"a[1] = 3 out of range")
    failed(raw_overlap(ex, good, packed, n, b=[-1])[0], api.GCRE_ERR_RANGE, b"b[0] = -1 out of range")
    failed(raw_overlap(ex, [[0], [6]], packed, n)[0], api.GCRE_ERR_RANGE, b"set 1: member row 6 out of range")
    failed(raw_overlap(ex, good, packed, n + 1)[0], api.GCRE_ERR_ARG, b"46 columns")
    failed(raw_overlap(ex, [[0], []], packed, n)[0], api.GCRE_ERR_ARG, b"set 1 has no members")
    failed(raw_overlap(ex, good, packed, n, a=None, na=2)[0], api.GCRE_ERR_ARG, b"bad index list")
    lib = api._overlap_lib()
    out = np.zeros((3, 3, 2), np.int32)
    failed(lib.gcre_set_overlap(ex._h, None, None, 3, None, 3, None, api._ptr(out)), api.GCRE_ERR_ARG, b"NULL argument")
    # a bad sign, through the C entry with a signs array
    off, mem, sg = np.array([0, 2], np.int64), np.array([0, 1], np.int32), np.array([1, 0], np.int32)
    inp = api.gcre_set_input(1, api._ptr(off), api._ptr(mem), api._ptr(sg), api._ptr(packed), len(packed), n)
    failed(lib.gcre_set_overlap(ex._h, ctypes.byref(inp), None, 1, None, 1, None, api._ptr(out)), api.GCRE_ERR_ARG,
           b"sign 0 is neither")
    # the Python method raises with the library's message
    with pytest.raises(api.GcreError, match="set 1 has no members"):
        ex.set_overlap([[0], []], rows)
    with pytest.raises(api.GcreError, match=r"a\[0\] = 9 out of range"):
        ex.set_overlap(good, rows, a=[9])
    assert ex.overlap_launches() == 0
    # a set with an NA member is no error: size (-1, -1), overlaps 0
    size, both = ex.set_overlap(good, rows)
    assert size[2].tolist() == [-1, -1] and not both[2].any() and not both[:, 2].any()
    assert both[0][0].tolist() == [nc, n - nc] and ex.overlap_launches() == 1
    # only sets with NA members: zeros, and still nothing more to launch
    size, both = ex.set_overlap([[-1], [0, -1]], rows)
    assert (size == -1).all() and not both.any() and ex.overlap_launches() == 1
    ex.close()


# ---- front end ---------------------------------------------------------------------------------------------------------

NC, NT, K_PERM, TOP_K, THRESHOLD, SEED = 140, 160, 256, 40, 0.2, 4711


def _problem():
    """About 200 genes, 800 relations, 300 patients.  A few strong genes carried by many cases: they drive most of the top
    paths of every length, the situation clumping is for."""
    rng = np.random.default_rng(2024)
    g, src, trg, sign = synth.signed_network(200, 800, rng)
    uid = np.arange(g) * 3 + 10
    symbols = [f"G{u}" for u in uid]
    data = (rng.random((g, NC + NT)) < 0.03).astype(np.int32)
    hubs = np.argsort(-np.bincount(np.concatenate([src, trg]), minlength=g))[:3]
    for h, dens in zip(hubs, (0.18, 0.14, 0.10)):
        data[h, :NC] |= (rng.random(NC) < dens).astype(np.int32)
    strata = (np.arange(NC + NT) * 5 % 3).astype(np.int32)
    return symbols, data, (uid, symbols, uid[src], uid[trg], sign), strata


def _brute_table(df, genes, data, r, measure, patients, by_length):
    """The clump columns by the numpy definitions: carrier_rows of the printed paths, counts by overlap_reference, the
    brute-force loop of test_overlap_host."""
    _, rows, _ = report.parse_sets(list(df["Paths"]), genes)
    size, both = report.overlap_reference(rows, data, NC, NT)
    scores, lengths = df["Scores"].to_numpy(), df["Lengths"].to_numpy()
    ok = np.isfinite(scores) & (size[:, 0] >= 0)
    S = len(df)
    clump, lead, value = np.full(S, -1), np.full(S, -1), np.full(S, np.nan)
    shared = np.full((S, 2), np.nan)
    groups = [np.flatnonzero(ok & (lengths == L)) for L in sorted(set(lengths[ok].tolist()))] if by_length \
        else [np.flatnonzero(ok)]
    base = 0
    for idx in groups:
        order = idx[np.argsort(-scores[idx], kind="stable")]
        c, l, v, sh = brute_clumps(order.tolist(), size, both, r, measure, patients)
        clump[order], lead[order], value[order] = c[order] + base, l[order], v[order]
        member = order[l[order] != order]
        shared[member] = sh[member]
        base += c[order].max() + 1
    return clump, lead, value, shared


def _check_clump_columns(got, base, genes, data, r, measure, patients, by_length):
    clump, lead, value, shared = _brute_table(base, genes, data, r, measure, patients, by_length)
    np.testing.assert_array_equal(got["Clump"].to_numpy(), clump)
    paths = list(base["Paths"])
    assert list(got["ClumpLead"]) == [paths[l] if l >= 0 else None for l in lead]
    sizes = np.bincount(clump[clump >= 0])
    np.testing.assert_array_equal(got["ClumpSize"].to_numpy(), np.where(clump >= 0, sizes[np.maximum(clump, 0)], 0))
    np.testing.assert_array_equal(got["LeadOverlap"].to_numpy().view(np.uint64), value.view(np.uint64))
    np.testing.assert_array_equal(got["SharedCases"].to_numpy(), shared[:, 0])
    np.testing.assert_array_equal(got["SharedControls"].to_numpy(), shared[:, 1])
    return clump, lead


def _check_residuals(got, lead, signed, genes, data, strata):
    """Every Residual* value == score_paths on the dataset with the lead's carrier columns zeroed by hand."""
    _, rows, _ = report.parse_sets(list(got["Paths"]), genes)
    C, _ = report.carrier_rows(rows, data, NC + NT)
    S = len(got)
    member = (lead >= 0) & (lead != np.arange(S))
    res = {c: got[c].to_numpy() for c in report.RESIDUAL_COLUMNS}
    for c in report.RESIDUAL_COLUMNS:
        assert np.isnan(res[c][~member]).all(), c
    assert member.any()
    for ld in np.unique(lead[member]).tolist():
        js = np.flatnonzero(member & (lead == ld))
        zeroed = np.array(data, copy=True)
        zeroed[:, C[ld]] = 0
        sp = report.score_paths(list(got["SignedPaths"].iloc[js]), genes, zeroed, NC, NT, signed=signed,
                                threshold=THRESHOLD, n_permutations=K_PERM, strata=strata, seed=SEED)
        np.testing.assert_array_equal(res["ResidualScores"][js].view(np.uint64), sp["Scores"].to_numpy().view(np.uint64))
        np.testing.assert_array_equal(res["ResidualCases"][js], sp["Cases"].to_numpy())
        np.testing.assert_array_equal(res["ResidualControls"][js], sp["Controls"].to_numpy())
        np.testing.assert_array_equal(res["ResidualPvalues"][js], sp["NominalPvalues"].to_numpy())


@pytest.mark.parametrize("signed", [False, True])
def test_gwaspa_clump_and_conditional(signed):
    import pandas as pd
    symbols, data, network, strata = _problem()
    kw = dict(signed=signed, threshold=THRESHOLD, top_k=TOP_K, path_length=5, n_permutations=K_PERM, strata=strata,
              seed=SEED)
    base = report.gwaspa(symbols, data, NC, NT, network, **kw)["GWASPA.Results"]
    got = report.gwaspa(symbols, data, NC, NT, network, clump=0.5, clump_conditional=True, **kw)["GWASPA.Results"]
    # the original columns bit for bit, in the same row order
    assert list(got.columns) == list(base.columns) + report.CLUMP_COLUMNS + report.RESIDUAL_COLUMNS
    pd.testing.assert_frame_equal(got[list(base.columns)], base, check_exact=True)
    np.testing.assert_array_equal(got["Scores"].to_numpy().view(np.uint64), base["Scores"].to_numpy().view(np.uint64))
    plain = report.gwaspa(symbols, data, NC, NT, network, clump=0.5, **kw)["GWASPA.Results"]
    assert list(plain.columns) == list(base.columns) + report.CLUMP_COLUMNS
    pd.testing.assert_frame_equal(plain, got[list(plain.columns)], check_exact=True)

    genes, pdata = report.preprocess_table(symbols, data, THRESHOLD, NC, NT)
    clump, lead = _check_clump_columns(got, base, genes, pdata, 0.5, "jaccard", "all", False)
    # not vacuous: a clump of three rows or more, and a lead on its own
    sizes = np.bincount(clump[clump >= 0])
    assert sizes.max() >= 3 and (sizes == 1).any(), sizes
    _check_residuals(got, lead, signed, genes, pdata, strata)

    # the other measure, the cases alone, every length on its own: clump_paths on the same table
    ckw = dict(signed=signed, threshold=THRESHOLD, n_permutations=K_PERM, strata=strata, seed=SEED)
    for measure, patients, by_length, r, conditional in (("containment", "all", False, 0.8, False),
                                                          ("jaccard", "cases", True, 0.5, True),
                                                          ("containment", "cases", True, 1.0, False)):
        other = report.clump_paths(base, symbols, data, NC, NT, r=r, measure=measure, patients=patients,
                                   by_length=by_length, conditional=conditional, **ckw)
        pd.testing.assert_frame_equal(other[list(base.columns)], base, check_exact=True)
        clump, lead = _check_clump_columns(other, base, genes, pdata, r, measure, patients, by_length)
        if by_length:   # no clump spans two lengths
            ln = base["Lengths"].to_numpy()
            assert all(len(set(ln[clump == k].tolist())) == 1 for k in range(clump.max() + 1))
        if conditional:
            _check_residuals(other, lead, signed, genes, pdata, strata)
