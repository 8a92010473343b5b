"""The sequential entries on the special-value tables (gcre_score_sets_sequential, _sequential_weighted, _prefix_sequential,
_dose_sequential: k_seq_null, k_seq_prefix_null, k_seq_retire).  Every case of helpers.SEQ_TABLE_CASES --
what each must provoke is asserted on the definitions alone in tests/test_seq_tables_host.py -- is run with the table at the
cohort's shape row- and column-major and drawn as an (n + 1)^2 square, with 512 permutations a batch and uncut, and compared
record for record with the numpy definition: counts as integers, scores bit for bit.  The definition's own null matrix is
held to the resident road (family_tests / prefix_tests / dose_tests with ``null=True``), which the table tests already hold
to the oracle.  There is no tolerance in this file."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from geneticscre_amd import api, report
from helpers import SEQ_ENTRIES, SEQ_TABLE_CASES
import test_gpu_sequential as t
import test_gpu_seq_prefix as tp
import test_seq_tables_host as h

pytestmark = pytest.mark.gpu

HITS, PERM_SEED = h.HITS, h.PERM_SEED
CASES = [(entry, family, method, spec) for entry in SEQ_ENTRIES for method in h.METHODS for family, spec in h.cases_of(entry, method)]
SMALL_FAMILIES = ("zeros", "nonfinite", "tiny", "huge", "ladder", "shapes")      # of the 33 + 31 leg


def case_id(case):
    entry, family, method, spec = case
    return f"{entry}-{family}-m{method}-v{spec[1]}"


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for var in tp.ENV:
        monkeypatch.delenv(var, raising=False)


def open_context(c, K=0, col_major=0):
    """A context with the case's table, handed over row- or column-major."""
    ex = api.JoinExec(c.method, c.nc, c.nt, K)
    raw = np.ascontiguousarray(c.VT.T if col_major else c.VT, dtype=np.float64)
    ptr = raw.ctypes.data_as(ctypes.c_void_p) if raw.size else None
    try:
        ex._check(ex._lib.gcre_set_value_table(ex._h, ptr, c.VT.shape[0], c.VT.shape[1], col_major))
    except BaseException:
        ex.close()
        raise
    return ex


def same_bits(got, want, what):
    """Doubles bit for bit; a NaN equals a NaN."""
    g, w = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    nan = np.isnan(w)
    np.testing.assert_array_equal(np.isnan(g), nan, err_msg=what)
    np.testing.assert_array_equal(g[~nan].view(np.uint64), w[~nan].view(np.uint64), err_msg=what)


def run(ex, c):
    """The case's entry: (records, per-set records or None, seq, the steps' or levels' scores or None)."""
    kw = dict(hits=HITS, max_perms=c.max_perms, seed=PERM_SEED)
    if c.entry == "sequential":
        rec, seq = ex.sequential_tests(c.sets, c.rows, c.signs, **kw)
        return rec, None, seq, None
    if c.entry == "weighted":
        rec, seq = ex.weighted_sequential_tests(c.sets, c.rows, c.signs, odds=c.odds, **kw)
        return rec, None, seq, None
    if c.entry == "prefix":
        return ex.prefix_sequential_tests(c.sets, c.rows, c.signs, cuts=c.extra, steps=True, **kw)
    return ex.dose_sequential_tests(c.sets, c.rows, c.signs, levels=c.extra, level_scores=True, **kw)


def check(c, out, what):
    """Record for record against the definition."""
    rec, px, seq, sc = out
    ok = c.valid != 0
    assert seq.dtype == api.SEQ_SCORE and len(seq) == len(c.sets) == len(rec)
    t.assert_equal(seq, c.ref, what)
    np.testing.assert_array_equal(rec["valid"] != 0, ok, err_msg=what)
    same_bits(rec["score"][ok], c.full_obs[ok], f"{what}: the records' scores")
    if px is None:
        return
    same_bits(px["score"][ok], c.ref["score"][ok], f"{what}: the best score")
    np.testing.assert_array_equal(px["best_step" if c.entry == "prefix" else "best_index"][ok], c.ref["best_step"][ok], err_msg=what)
    np.testing.assert_array_equal(px["n_ge"], np.where(ok, 0, -1), err_msg=what)
    of_valid = np.isin(c.owner, np.flatnonzero(ok))
    if c.entry == "dose":
        same_bits(sc[ok], c.step_obs[of_valid], f"{what}: the levels' scores")
        return
    # the step that ends at a member, in the order of report.prefix_sets; NaN where none does
    want, member, step = [], 0, 0
    for s, m in enumerate(c.sets):
        for i in range(len(m)):
            ends = bool(c.extra[s][i]) or i + 1 == len(m)
            if ok[s]:
                want.append((member, c.step_obs[step] if ends else np.nan))
            member, step = member + 1, step + int(ends)
    at = np.array([w[0] for w in want])
    same_bits(sc[at], np.array([w[1] for w in want]), f"{what}: the steps' scores")


def anchor(c, what):
    """The definition's null matrix is the resident road's, bit for bit, under K = max_perms masks of the same seed; a set
    that never stops has counted what that road counts."""
    full = open_context(c, K=c.max_perms)
    try:
        if c.entry == "weighted":
            full.generate_weighted_permutations(PERM_SEED, c.odds, None)
        else:
            full.generate_permutations(PERM_SEED, None)
        if c.entry in ("sequential", "weighted"):
            rec, _, nul = full.family_tests(c.sets, c.rows, c.signs, null=True)
            n_ge = rec["n_ge"]
        elif c.entry == "prefix":
            _, px, nul = full.prefix_tests(c.sets, c.rows, c.signs, cuts=c.extra, null=True)
            n_ge = px["n_ge"]
        else:
            _, ds, nul = full.dose_tests(c.sets, c.rows, c.signs, levels=c.extra, null=True)
            n_ge = ds["n_ge"]
    finally:
        full.close()
    ok = c.valid != 0
    assert nul.dtype == np.float32 and nul.shape == (len(c.sets), c.max_perms)
    np.testing.assert_array_equal(nul[ok].view(np.uint32), np.ascontiguousarray(c.null[ok, :c.max_perms]).view(np.uint32),
                                  err_msg=f"{what}: the null matrix")
    never = ok & (c.ref["stopped"] == 0)
    np.testing.assert_array_equal(c.ref["n_hit"][never], n_ge[never], err_msg=f"{what}: the sets that never stop")


def both_batches(monkeypatch, ex, c, what):
    """512 permutations a batch, then uncut: each against the definition, and the same bytes."""
    outs = []
    for cap in ("512", None):
        if cap is None:
            monkeypatch.delenv("GCRE_SEQ_BATCH_PERMS", raising=False)
        else:
            monkeypatch.setenv("GCRE_SEQ_BATCH_PERMS", cap)
        out = run(ex, c)
        check(c, out, f"{what} cap={cap}")
        outs.append(out)
    for a, b in zip(*outs):
        assert (a is None and b is None) or a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_entry_on_a_special_table(monkeypatch, case):
    entry, family, method, spec = case
    legs = [(0, False), (1, False)] + ([(0, True)] if family != "shapes" else [])
    for col_major, square in legs:
        c = h.build(entry, family, method, spec, square=square)
        what = f"{case_id(case)} col_major={col_major} square={square}"
        ex = open_context(c, col_major=col_major)
        try:
            both_batches(monkeypatch, ex, c, what)
        finally:
            ex.close()
        if col_major == 0:
            anchor(c, what)


@pytest.mark.parametrize("method", h.METHODS)
@pytest.mark.parametrize("entry", SEQ_ENTRIES)
def test_two_full_dwords(monkeypatch, entry, method):
    """33 + 31 patients: 64, two full mask dwords.  The first case of every family the entry runs, on that cohort."""
    for family in SMALL_FAMILIES:
        specs = SEQ_TABLE_CASES.get((entry, family, method), [])
        if not specs:
            continue
        spec = next(s for s in specs if s[1] == h.WEIGHTED_FAMILIES["shapes"][0]) if family == "shapes" else specs[0]     # few_both
        c = h.build(entry, family, method, spec, nc=33, nt=31)
        if entry == "weighted":
            assert c.ref["first_left_over"] is None
        ex = open_context(c)
        try:
            both_batches(monkeypatch, ex, c, f"{entry} {family} method {method} 33 + 31")
        finally:
            ex.close()


@pytest.mark.parametrize("method", h.METHODS)
def test_a_nan_score_and_a_left_over_permutation_refuse(method):
    """The weighted entry on the nonfinite table: a set whose score is NaN never stops, so a permutation without an accepted
    attempt below max_attempts refuses the call (GCRE_ERR_RANGE; an ordinary return, nothing faults)."""
    c, cap, att, ref = h.refusal_case(method)
    R, active = ref["first_left_over"], ref["n_active"]
    assert ref["refused"] and R is not None
    ex = open_context(c)
    try:
        with pytest.raises(api.GcreError, match=rf"score_sets_sequential_weighted: permutation {R} has no accepted attempt below "
                                                rf"max_attempts = {cap} in stratum 0, and {active} sets were still active there"):
            ex.weighted_sequential_tests(c.sets, c.rows, c.signs, odds=c.odds, hits=HITS, max_perms=c.max_perms, seed=PERM_SEED,
                                         max_attempts=cap)
        lib = api._feature_lib("sequential_weighted")
        inp, keep = api._set_input(c.sets, c.rows, c.signs, c.nc + c.nt)
        n = len(c.sets)
        out, seq = np.zeros(n, api.SET_SCORE), np.zeros(n, api.SEQ_SCORE)
        w = np.ascontiguousarray(c.odds, np.float64)
        n_out = ctypes.c_int64(0)
        rc = lib.gcre_score_sets_sequential_weighted(ex._h, ctypes.byref(inp), PERM_SEED, api._ptr(w), None, 0, cap, HITS, c.max_perms,
                                                     api._ptr(out), n, ctypes.byref(n_out), api._ptr(seq))
        assert rc == api.GCRE_ERR_RANGE
        # below R nothing is left over: the call returns, and the NaN-scored sets have run to the limit without a hit
        short = report.weighted_sequential_reference(c.null, c.obs, c.valid, HITS, R, att)
        assert short["first_left_over"] is None
        rec, seq = ex.weighted_sequential_tests(c.sets, c.rows, c.signs, odds=c.odds, hits=HITS, max_perms=R, seed=PERM_SEED,
                                                max_attempts=cap)
        t.assert_equal(seq, short, "below the left-over permutation")
        nan = (c.valid != 0) & np.isnan(c.obs)
        assert (seq["n_hit"][nan] == 0).all() and (seq["n_perm"][nan] == R).all() and not seq["stopped"][nan].any()
    finally:
        ex.close()
