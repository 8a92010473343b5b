"""Conditional set scores on the device (gcre_score_sets_given: k_set_residual, then gcre_score_sets' kernels; DESIGN.md
§3.12): everything exact -- against ``report.residual_rows`` fed to ``restate_slabs`` of tests/test_sets_host.py, against
gcre_score_sets itself, against the old road of column-zeroed matrices, across slab sizes; the refusals; and the two front
ends, ``clump_paths(conditional=True)`` against the per-lead loop it replaces and ``gwaspa``'s residual columns for hits
(pytest -m gpu).

GCRE_GIVEN_FUZZ_CASES=300 [GCRE_GIVEN_FUZZ_BASE=...] for a long run of the seeded loop at the end (GCRE_GIVEN_FUZZ_OUT: a
file for its summary); a handful by default."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from geneticscre_amd import api, report
from helpers import small_table
from test_gpu_sets import device_masks
from test_sets_host import restate_slabs

pytestmark = pytest.mark.gpu

COUNTS = ["valid", "cases", "ctrls", "cases_pos", "ctrls_pos", "cases_neg", "ctrls_neg"]
TILE = {1: 16, 2: 8}      # set_null_tile_sets(method): sets per block of k_set_null


def raw_given(ex, sets, packed, n_cols, which, given, signs=None, n_which=None, cap=None, family=True, null_in=False,
              null_out=False):
    """gcre_score_sets_given through the C entry: (rc, records, n_out, family_max).  The records start as 0xAB bytes and
    family_max as -7, so that what a call leaves untouched shows."""
    lib = api._given_lib()
    S = len(sets)
    off = np.zeros(S + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in sets])
    mem = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int64) for s in sets]) if S else np.zeros(0), np.int32)
    sg = None if signs is None else np.ascontiguousarray(np.concatenate([np.asarray(s, np.int64) for s in signs]), np.int32)
    iw = None if which is None else np.ascontiguousarray(which, np.int64)
    ig = None if given is None else np.ascontiguousarray(given, np.int64)
    if n_which is None:
        n_which = S if iw is None else len(iw)
    cap = max(n_which, 0) if cap is None else cap
    inp = api.gcre_set_input(S, api._ptr(off), api._ptr(mem), api._ptr(sg), api._ptr(packed), len(packed), n_cols)
    out = np.frombuffer(bytearray(b"\xab" * (api.SET_SCORE.itemsize * max(cap, 1))), dtype=api.SET_SCORE)
    fam = np.full(ex.iters, -7, np.float32) if family else None
    n_out = ctypes.c_int64(-7)
    rc = lib.gcre_score_sets_given(ex._h, None if null_in else ctypes.byref(inp), api._ptr(iw), api._ptr(ig), n_which,
                                   None if null_out else api._ptr(out), cap, ctypes.byref(n_out), api._ptr(fam))
    return rc, out, n_out.value, fam


def make_inputs(rng, n, R=16, S=24):
    """Gene rows (a full one, an empty one), sets of 1-12 members with mixed signs and the special ones: repeats, a gene
    under both signs, an NA member, a lone (-) gene, the full and the empty row."""
    rows = (rng.random((R, n)) < rng.uniform(0.02, 0.6, size=(R, 1))).astype(np.int8)
    rows[0], rows[1] = 1, 0
    sets, signs = [], []
    for _ in range(S):
        L = int(rng.integers(1, 13))
        sets.append(rng.integers(0, R, size=L).tolist())
        signs.append(rng.choice([-1, 1], size=L).tolist())
    sets[0], signs[0] = [3, 3, 5, 3], [1, 1, -1, 1]
    sets[1], signs[1] = [4, 4], [1, -1]
    sets[2], signs[2] = [2, -1, 7], [1, 1, -1]
    sets[3], signs[3] = [6], [-1]
    sets[4], signs[4] = [0, 1], [1, 1]
    return rows, sets, signs


def make_entries(rng, sets, E):
    """``which`` with repeats (the NA set among them from 5 entries on) and ``given``: -1, the set itself, or an NA-free set."""
    S = len(sets)
    free = np.array([s for s in range(S) if min(sets[s]) >= 0])
    which = rng.integers(0, S, E)
    given = np.where(rng.random(E) < 0.25, -1, free[rng.integers(0, len(free), E)])
    own = (rng.random(E) < 0.15) & np.isin(which, free)
    given[own] = which[own]
    if E >= 5:
        which[1], given[1] = 2, free[0]          # an NA set may be scored, given anything
        which[2], given[2] = which[0], given[0]  # the same entry twice
        which[3], given[3] = 4, 4                # the full row without itself
        which[4], given[4] = 5, 4                # ... and another set without everybody
    return which.astype(np.int64), given.astype(np.int64)


def check_against_definition(rec, fam, method, nc, nt, sets, rows, signs, which, given, VT, masks, what=""):
    """Every record field, n_ge and family_max against restate_slabs(residual_rows(...)): integers as integers, scores and
    maxima by their bits."""
    n, K = nc + nt, len(masks)
    pos, neg, valid = report.residual_rows(sets, rows, signs, which, given, n, method)
    want = restate_slabs(method, nc, nt, pos[valid], neg[valid] if method == 2 else None, VT, masks)
    assert len(rec) == len(which), what
    np.testing.assert_array_equal(rec["set"], which, err_msg=what)
    np.testing.assert_array_equal(rec["valid"], valid.astype(np.int32), err_msg=what)
    v = np.flatnonzero(valid)
    for f in COUNTS[1:] + ["n_ge"]:
        np.testing.assert_array_equal(rec[f][v], want[f], err_msg=f"{f} {what}")
        assert not rec[f][~valid].any(), (f, what)
    np.testing.assert_array_equal(rec["score"][v].view(np.uint64), want["score"].view(np.uint64), err_msg=what)
    assert np.isnan(rec["score"][~valid]).all() and np.isnan(rec["pvalue"][~valid]).all(), what
    if K:
        np.testing.assert_array_equal(rec["pvalue"][v], want["n_ge"] / K, err_msg=what)
    else:      # no permutations: the scores are there, the p-values are NaN
        assert np.isnan(rec["pvalue"]).all() and np.isfinite(rec["score"][v]).all(), what
    np.testing.assert_array_equal(fam.view(np.uint32), want["family"].view(np.uint32), err_msg=what)


def context(method, nc, nt, K, seed, VT):
    ex = api.JoinExec(method, nc, nt, K)
    ex.set_value_table(VT)
    if K:
        ex.generate_permutations(seed, (np.arange(nc + nt) * 7 % 3).astype(np.int32) if seed % 2 else None)
    return ex


# ---- 1-3, 8: the definition, gcre_score_sets itself, the old road ------------------------------------------------------
# padding words; whole words; a split inside a dword, 3 dwords; one bit in the second word; more than 64 dwords
SHAPES = [(nc, nt, K) for nc, nt in ((48, 52), (64, 64), (37, 30), (33, 32)) for K in (0, 1, 513)] + [(1000, 1100, 64)]


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("nc,nt,K", SHAPES, ids=[f"{a}+{b}-K{k}" for a, b, k in SHAPES])
def test_definition_score_sets_and_old_road(method, nc, nt, K):
    i = SHAPES.index((nc, nt, K))
    rng = np.random.default_rng(5000 + 10 * i + method)
    n = nc + nt
    rows, sets, signs = make_inputs(rng, n)
    VT = small_table(n, n, i)
    VT[rng.random(VT.shape) < 0.05] *= -1
    ex = context(method, nc, nt, K, 300 + i, VT)
    masks = device_masks(ex, K, n)
    tile = TILE[method]
    for E in (1, tile - 1, tile, tile + 1, 70):
        which, given = make_entries(rng, sets, E)
        before = ex.given_launches
        rec, fam = ex.score_sets(sets, rows, signs, family=True, given=given, which=which)
        has_valid = any(min(sets[s]) >= 0 for s in which)
        assert ex.given_launches - before == ((3 if K else 2) if has_valid else 0), E      # one slab
        check_against_definition(rec, fam, method, nc, nt, sets, rows, signs, which, given, VT, masks, f"E={E}")
    # 3. the old road: per distinct given set, gcre_score_sets on the matrix with that set's carrier columns zeroed
    C, _ = report.carrier_rows(sets, rows, n)
    for g in np.unique(given).tolist():
        js = np.flatnonzero(given == g)
        zeroed = rows if g < 0 else np.where(C[g][None, :], 0, rows)
        old = ex.score_sets([sets[s] for s in which[js]], zeroed, [signs[s] for s in which[js]])
        for f in COUNTS + ["n_ge"]:
            np.testing.assert_array_equal(rec[f][js], old[f], err_msg=f"{f} given {g}")
        np.testing.assert_array_equal(rec["score"][js].view(np.uint64), old["score"].view(np.uint64))
        np.testing.assert_array_equal(rec["pvalue"][js].view(np.uint64), old["pvalue"].view(np.uint64))
    # 2. nothing given, every set: the device-built rows against SetUnion's, byte for byte
    old, ofam = ex.score_sets(sets, rows, signs, family=True)
    packed = api.pack_carriers(rows, n)
    for kw in (dict(which=None, given=None), dict(which=np.arange(len(sets)), given=np.full(len(sets), -1))):
        rc, new, n_out, nfam = raw_given(ex, sets, packed, n, signs=signs, **kw)
        assert rc == api.GCRE_OK and n_out == len(sets)
        assert new.tobytes() == old.tobytes()
        if K:
            assert nfam.tobytes() == ofam.tobytes()
    # only which, through the Python method: a selection of gcre_score_sets' records
    pick = rng.integers(0, len(sets), 9)
    sel = ex.score_sets(sets, rows, signs, which=pick)
    for f in api.SET_SCORE.names:      # (field by field: a fancy index does not copy a record's padding)
        assert sel[f].tobytes() == old[f][pick].tobytes(), f
    ex.close()


# ---- 4. slabs -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", [1, 2])
def test_slabs_do_not_change_the_result(method, monkeypatch, capfd):
    nc, nt, K = 37, 30, 513
    rng = np.random.default_rng(81 + method)
    rows, sets, signs = make_inputs(rng, nc + nt)
    ex = context(method, nc, nt, K, 12, small_table(nc + nt, nc + nt, 3))
    which, given = make_entries(rng, sets, 70)
    launched = sum(min(sets[s]) >= 0 for s in which)
    monkeypatch.delenv("GCRE_GIVEN_SLAB_SETS", raising=False)
    monkeypatch.setenv("GCRE_GIVEN_STATS", "1")
    want, wfam = ex.score_sets(sets, rows, signs, family=True, given=given, which=which)
    assert f"launched={launched} slab={launched} slabs=1" in capfd.readouterr().err
    tile = TILE[method]
    for slab in (1, tile, tile + 1):
        monkeypatch.setenv("GCRE_GIVEN_SLAB_SETS", str(slab))
        before = ex.given_launches
        got, gfam = ex.score_sets(sets, rows, signs, family=True, given=given, which=which)
        slabs = -(-launched // slab)
        assert ex.given_launches - before == 3 * slabs
        assert f"slab={slab} slabs={slabs}" in capfd.readouterr().err
        assert got.tobytes() == want.tobytes() and gfam.tobytes() == wfam.tobytes(), slab
    ex.close()


# ---- 5. stray bits --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nc,nt", [(48, 52), (37, 30), (33, 32)])
def test_stray_bits_beyond_the_patients_change_nothing(nc, nt):
    n = nc + nt
    rng = np.random.default_rng(n)
    rows, sets, signs = make_inputs(rng, n)
    which, given = make_entries(rng, sets, 40)
    packed = api.pack_carriers(rows, n)
    dirty = packed.copy()
    dirty[::2, -1] |= ~np.uint64(0) << np.uint64(n % 64)      # rows 0, 2, ..: every bit from n on
    assert (dirty != packed).any()
    for method in (1, 2):
        ex = context(method, nc, nt, 65, 5, small_table(n, n, 1))
        rc0, a, _, fa = raw_given(ex, sets, packed, n, which, given, signs)
        rc1, b, _, fb = raw_given(ex, sets, dirty, n, which, given, signs)
        assert rc0 == rc1 == api.GCRE_OK and a.tobytes() == b.tobytes() and fa.tobytes() == fb.tobytes()
        assert a["cases"].max() <= nc + nt and (a["valid"] == 1).any()
        ex.close()


# ---- 6, 7. refusals, no entries ------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing_and_write_nothing():
    nc, nt, K = 20, 25, 10
    n = nc + nt
    rng = np.random.default_rng(3)
    rows = (rng.random((6, n)) < 0.3).astype(np.int8)
    packed = api.pack_carriers(rows, n)
    good = [[0], [2, 3], [4, -1], [5]]
    ARG, RANGE, ASSERT = api.GCRE_ERR_ARG, api.GCRE_ERR_RANGE, api.GCRE_ERR_ASSERT
    ex = api.JoinExec(2, nc, nt, K)

    def failed(res, code, text):
        rc, out, _, fam = res
        msg = ex._lib.gcre_last_error(ex._h)
        assert rc == code and text in msg, (rc, msg)
        assert ex.given_launches == 0
        assert out.tobytes() == b"\xab" * out.nbytes and (fam == -7).all()

    # what check_sets refuses
    failed(raw_given(ex, good, packed, n, [0], [1]), ASSERT, b"score_sets_given needs a value table")
    ex.set_value_table(small_table(n, n, 0))
    failed(raw_given(ex, good, packed, n, [0], [1]), ASSERT, b"score_sets_given needs the permutation masks")
    ex.generate_permutations(1)
    failed(raw_given(ex, good, packed, n + 1, [0], [1]), ARG, b"score_sets_given: the rows have 46 columns")
    failed(raw_given(ex, [[0], []], packed, n, [0], [0]), ARG, b"score_sets_given: set 1 has no members")
    failed(raw_given(ex, [[0], [6]], packed, n, [0], [0]), RANGE, b"score_sets_given: set 1: member row 6 out of range")
    failed(raw_given(ex, good, packed, n, [0], [1], signs=[[1], [1, 0], [1, 1], [1]]), ARG, b"sign 0 is neither +1 nor -1")
    # the index lists
    failed(raw_given(ex, good, packed, n, [0, 4], [1, 1]), RANGE, b"score_sets_given: which[1] = 4 out of range (4 sets)")
    failed(raw_given(ex, good, packed, n, [-1], [1]), RANGE, b"score_sets_given: which[0] = -1 out of range")
    failed(raw_given(ex, good, packed, n, [0, 1], [-1, 4]), RANGE, b"score_sets_given: given[1] = 4 out of range (4 sets, -1 = none)")
    failed(raw_given(ex, good, packed, n, [0], [-2]), RANGE, b"score_sets_given: given[0] = -2 out of range")
    failed(raw_given(ex, good, packed, n, [0, 1, 3], [1, 1, 1], cap=2), RANGE, b"score_sets_given: 3 entries, room for 2 records")
    failed(raw_given(ex, good, packed, n, [0, 1], [1, 2]), ARG, b"score_sets_given: given[1] = set 2 has an NA member")
    failed(raw_given(ex, good, packed, n, [0], [1], n_which=-1, cap=1), ARG, b"score_sets_given: bad index list")
    failed(raw_given(ex, good, packed, n, None, [1, 1, 1], n_which=3, cap=3), ARG, b"score_sets_given: bad index list")
    failed(raw_given(ex, good, packed, n, [0], [1], null_in=True), ARG, b"score_sets_given: NULL argument")
    failed(raw_given(ex, good, packed, n, [0], [1], null_out=True), ARG, b"score_sets_given: NULL argument")
    failed(raw_given(ex, good, packed, n, [0], [1], cap=-1), ARG, b"score_sets_given: NULL argument")
    # 7. no entries: nothing launched, nothing written but zeros into family_max
    rc, out, n_out, fam = raw_given(ex, good, packed, n, [], [], cap=0)
    assert rc == api.GCRE_OK and n_out == 0 and ex.given_launches == 0
    assert out.tobytes() == b"\xab" * out.nbytes and not fam.any()
    # only entries with an NA member: records, and still nothing to launch
    rc, out, n_out, fam = raw_given(ex, good, packed, n, [2, 2], [-1, 0])
    assert rc == api.GCRE_OK and n_out == 2 and ex.given_launches == 0
    assert out["set"].tolist() == [2, 2] and not out["valid"].any() and np.isnan(out["score"]).all() and not fam.any()
    # the Python method: its own ValueErrors, and the library's message
    with pytest.raises(ValueError, match="which: a set index outside"):
        ex.score_sets(good, rows, which=[4])
    with pytest.raises(ValueError, match="given: a given set has an NA member"):
        ex.score_sets(good, rows, which=[0], given=[2])
    with pytest.raises(api.GcreError, match="set 1: member row 6 out of range"):
        ex.score_sets([[0], [6]], rows, given=[0, 0])
    assert ex.given_launches == 0
    # the context still works
    rec = ex.score_sets(good, rows, which=[1, 0, 2], given=[0, 0, -1])
    assert rec["valid"].tolist() == [1, 1, 0] and ex.given_launches == 3
    assert rec["cases"][1] == 0 and rec["ctrls"][1] == 0           # a set without its own carriers
    ex.close()


# ---- 9. clump_paths(conditional=True): one call, the table of the loop it replaces ------------------------------------------

def loop_conditional(out, ex, sets, sub, signs, n):
    """The residual columns as clump_paths computed them before: per lead that has members a zeroed copy of the carrier
    matrix and one score_sets call."""
    S = len(out)
    clump = out["Clump"].to_numpy()
    is_lead = (clump >= 0) & np.isnan(out["LeadOverlap"].to_numpy())          # the one row of a clump without a measure
    lead_of = np.full(int(clump.max()) + 1, -1)
    lead_of[clump[is_lead]] = np.flatnonzero(is_lead)
    lead = np.where(clump >= 0, lead_of[np.maximum(clump, 0)], -1)
    res = {c: np.full(S, np.nan) for c in report.RESIDUAL_COLUMNS}
    C, _ = report.carrier_rows(sets, sub, n)
    members = (clump >= 0) & (lead != np.arange(S))
    calls = 0
    for ld in np.unique(lead[members]).tolist():
        js = np.flatnonzero(members & (lead == ld))
        need = {}
        msets = [[need.setdefault(x, len(need)) for x in sets[j]] for j in js]
        rec = ex.score_sets(msets, np.where(C[ld][None, :], 0, sub[list(need.keys())]), [signs[j] for j in js])
        calls += 1
        res["ResidualScores"][js] = rec["score"]
        res["ResidualCases"][js] = rec["cases"]
        res["ResidualControls"][js] = rec["ctrls"]
        res["ResidualPvalues"][js] = rec["pvalue"]
    return res, calls, int(members.sum())


@pytest.mark.parametrize("signed", [False, True])
def test_clump_paths_conditional_is_one_call(signed):
    import pandas as pd
    from test_gpu_overlap import NC, NT, K_PERM, THRESHOLD, SEED, _problem
    symbols, data, network, strata = _problem()
    table = report.gwaspa(symbols, data, NC, NT, network, signed=signed, threshold=THRESHOLD, top_k=200, path_length=5,
                          n_permutations=K_PERM, strata=strata, seed=SEED)["GWASPA.Results"]
    assert 900 < len(table) <= 1000
    ckw = dict(signed=signed, threshold=THRESHOLD, n_permutations=K_PERM, strata=strata, seed=SEED, conditional=True)
    # a context of the caller's: the launches of the one call show on it
    vt = api.values_table(NC, NT)
    ex = api.JoinExec(2 if signed else 1, NC, NT, K_PERM)
    ex.set_value_table(vt)
    ex.generate_permutations(SEED, strata)
    got = {}
    for on_device in (False, True):
        before = ex.given_launches
        got[on_device] = report.clump_paths(table, symbols, data, NC, NT, on_device=on_device, exec_=ex, **ckw)
        assert ex.given_launches - before == 3       # k_set_residual, k_set_observed, k_set_null: one slab, one call
    own = report.clump_paths(table, symbols, data, NC, NT, **ckw)                 # its own context
    with_table = report.clump_paths(table, symbols, data, NC, NT, table=vt, **ckw)
    for other in (got[True], own, with_table):
        pd.testing.assert_frame_equal(other, got[False], check_exact=True)
    new = got[False]
    assert list(new.columns) == list(table.columns) + report.CLUMP_COLUMNS + report.RESIDUAL_COLUMNS
    # the loop this replaces, on the same context
    genes, pdata = report.preprocess_table(symbols, data, THRESHOLD, NC, NT)
    _, prow, psigns = report.parse_sets([str(p) for p in table["SignedPaths"]], genes)
    used = {}
    sets = [[-1 if x < 0 else used.setdefault(x, len(used)) for x in rs] for rs in prow]
    sub = np.asarray(pdata)[list(used.keys())]
    want, calls, members = loop_conditional(new, ex, sets, sub, psigns, NC + NT)
    assert calls > 10 and members > calls
    for c in report.RESIDUAL_COLUMNS:
        np.testing.assert_array_equal(new[c].to_numpy().view(np.uint64), want[c].view(np.uint64), err_msg=c)
    print(f"clump_paths(conditional) signed={signed}: {members} member rows, 1 call instead of {calls}")
    with pytest.raises(ValueError, match="exec_: a context of 256 permutations, n_permutations = 100"):
        report.clump_paths(table, symbols, data, NC, NT, signed=signed, threshold=THRESHOLD, conditional=True, exec_=ex)
    ex.close()


# ---- 10. gwaspa: residual columns for the hits ---------------------------------------------------------------------------------

@pytest.mark.parametrize("signed", [False, True])
def test_gwaspa_residual_columns_for_hits(signed):
    import pandas as pd
    from test_gpu_hits import _network_case
    nc, nt = 48, 52
    genes, data, network = _network_case(17)
    strata = (np.arange(nc + nt) * 5 % 3).astype(np.int32)
    kw = dict(signed=signed, threshold=0.2, n_permutations=1000, strata=strata, seed=909, path_length=5)
    full = report.gwaspa(genes, data, nc, nt, network, top_k=2000, **kw)["GWASPA.Results"]
    pv = full["Pvalues"].to_numpy(np.float64)[np.isfinite(full["Scores"].to_numpy(np.float64))]
    alpha = float(pv[pv < 1].max())
    kw.update(top_k=3, significant=alpha, clump=0.5, clump_significant=True)
    base = report.gwaspa(genes, data, nc, nt, network, **kw)
    got = report.gwaspa(genes, data, nc, nt, network, clump_conditional=True, **kw)
    sig = got["Significant.Results"]
    assert list(sig.columns) == report.COLUMNS + report.CLUMP_COLUMNS + report.RESIDUAL_COLUMNS and len(sig) > 3
    pd.testing.assert_frame_equal(sig[report.COLUMNS + report.CLUMP_COLUMNS], base["Significant.Results"], check_exact=True)
    want = report.clump_paths(sig[report.COLUMNS], genes, data, nc, nt, signed=signed, r=0.5, threshold=0.2, conditional=True,
                              on_device=True, n_permutations=1000, strata=strata, seed=909)
    pd.testing.assert_frame_equal(sig, want, check_exact=True)
    for c in report.RESIDUAL_COLUMNS:
        np.testing.assert_array_equal(sig[c].to_numpy().view(np.uint64), want[c].to_numpy().view(np.uint64), err_msg=c)
    member = (sig["ClumpSize"] > 1) & sig["LeadOverlap"].notna()
    assert member.any() and np.isfinite(sig["ResidualScores"][member]).all() and sig["ResidualScores"][~member].isna().all()
    # GWASPA.Results is what clump_conditional alone gives it
    assert list(got["GWASPA.Results"].columns) == list(base["GWASPA.Results"].columns) + report.RESIDUAL_COLUMNS
    pd.testing.assert_frame_equal(got["GWASPA.Results"][list(base["GWASPA.Results"].columns)], base["GWASPA.Results"],
                                  check_exact=True)


# ---- 11. seeded loop ----------------------------------------------------------------------------------------------------------
N_FUZZ = int(os.environ.get("GCRE_GIVEN_FUZZ_CASES", "4"))
FUZZ_BASE = int(os.environ.get("GCRE_GIVEN_FUZZ_BASE", "0"))


def test_seeded_loop(monkeypatch):
    lines = []
    for k in range(FUZZ_BASE, FUZZ_BASE + N_FUZZ):
        rng = np.random.default_rng(9_000_000 + k)
        n = int(rng.choice([int(rng.integers(2, 70)), int(rng.integers(70, 700)), int(rng.integers(700, 2300))]))
        nc = int(rng.integers(1, n))
        method = 1 + k % 2
        K = int(rng.choice([0, 1, 100, 512, 513, 1100]))
        R, S, E = int(rng.integers(8, 40)), int(rng.integers(6, 60)), int(rng.integers(1, 200))     # (sets 0-5 are named)
        rows, sets, signs = make_inputs(rng, n, R, S)
        which, given = make_entries(rng, sets, E)
        VT = small_table(n, n, k)
        VT[rng.random(VT.shape) < 0.05] *= -1
        slab = int(rng.choice([0, 1, 7, 33]))
        if slab:
            monkeypatch.setenv("GCRE_GIVEN_SLAB_SETS", str(slab))
        else:
            monkeypatch.delenv("GCRE_GIVEN_SLAB_SETS", raising=False)
        ex = context(method, nc, n - nc, K, k, VT)
        rec, fam = ex.score_sets(sets, rows, signs if k % 3 else None, family=True, given=given, which=which)
        check_against_definition(rec, fam, method, nc, n - nc, sets, rows, signs if k % 3 else None, which, given, VT,
                                 device_masks(ex, K, n), f"case {k}")
        ex.close()
        lines.append(f"case {k}: method {method} patients {n} cases {nc} perms {K} rows {R} sets {S} entries {E} "
                     f"slab {slab or 'default'} valid {int(rec['valid'].sum())} ok")
    out = os.environ.get("GCRE_GIVEN_FUZZ_OUT")
    if out:
        with open(out, "w") as f:
            f.write(f"test_gpu_given.py::test_seeded_loop: cases {FUZZ_BASE}..{FUZZ_BASE + N_FUZZ - 1}, every one exact\n")
            f.write("\n".join(lines) + "\n")
