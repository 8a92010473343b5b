"""What the special-value tables must provoke in the sequential entries, asserted on the numpy definitions alone (no GPU):
``report.permutation_masks`` / ``weighted_masks``, ``_vt_cell``, ``_vt_max``, ``_fold_f32``, ``sequential_reference``,
``weighted_sequential_reference``, ``adaptive_sequential_reference`` -- and, for the step-down counts of a join,
``stepdown_reference`` on the oracle's rows.  A sequential p-value is a stop position: one wrong tie moves it, so every case
of helpers.SEQ_TABLE_CASES has to hold, in the reference's own results, the scores and null values at which the device's
f32 threshold, its fold and its mirror table can go wrong.  tests/test_gpu_seq_tables.py runs the same cases on the device;
a drifting generator or seed fails here first.  ``build`` and ``provoked`` are shared with that file and with
tools/seq_table_seeds.py, which found the cases."""
from __future__ import annotations

import types

import numpy as np
import pytest

from geneticscre_amd import api, report
from helpers import (FLT_MAX, FLT_MIN, FLT_OVERFLOW, SEQ_ENTRIES, SEQ_PLANTED, SEQ_SHAPE_NAMES, SEQ_TABLE_CASES, shape_tables,
                     special_table, table_problem, zeros_cut_top_k)
import test_gpu_sequential as t
import test_gpu_seq_prefix as tp
import test_gpu_seq_weighted as tw

HITS, P_MAX, CAP, PERM_SEED = t.HITS, 3000, t.CAP, t.PERM_SEED
PLANTED_SET = 3                      # a one-gene set of make_input
FAMILIES = ("zeros", "nonfinite", "tiny", "huge", "huge+hi", "huge+mid", "ladder", "shapes")
WEIGHTED_FAMILIES = {"zeros": (0,), "nonfinite": (2,), "huge": (1,), "shapes": (SEQ_SHAPE_NAMES.index("few_both"),)}
METHODS = (1, 2)


def variants_of(entry, family, method):
    """The variants of a family an entry runs."""
    if entry == "weighted":
        return WEIGHTED_FAMILIES.get(family, ())
    return {"zeros": (0,), "nonfinite": (0, 1, 2) + ((3, 4, 5) if method == 2 else ()), "tiny": (0,), "huge": (0, 1),
            "huge+hi": (0,), "huge+mid": (1,), "ladder": (0, 1), "shapes": tuple(range(len(SEQ_SHAPE_NAMES)))}[family]


def case_table(family, nc, nt, seed, variant, square=False):
    """The value table of a case: at the cohort's shape, or drawn as an (n + 1)^2 square."""
    if family == "shapes":
        return dict((name, tb) for name, tb, _ in shape_tables(nc, nt, seed))[SEQ_SHAPE_NAMES[variant]]
    kind, n = family.split("+")[0], nc + nt
    return special_table(kind, n, n, seed, variant) if square else special_table(kind, nc, nt, seed, variant)


def plant(VT, method, rows, sets, signs, nc, value):
    """The cell under the observed counts of set PLANTED_SET (one gene, made a (+) member) set so that the set scores
    ``value``: in method 2 its empty (-) half adds table[0][0], and the transposed cell is set too, so that vtmax there is the
    planted value.  Returns the table and the cell."""
    d = np.asarray(rows) != 0
    g = sets[PLANTED_SET][0]
    assert len(sets[PLANTED_SET]) == 1
    signs[PLANTED_SET] = [1]
    a, b = int(d[g, :nc].sum()), int(d[g, nc:].sum())
    VT = VT.copy()
    assert (a, b) != (0, 0) and a < VT.shape[0] and b < VT.shape[1]
    if method == 2:
        value = value - VT[0, 0]
        if b < VT.shape[0] and a < VT.shape[1]:
            VT[b, a] = value
    VT[a, b] = value
    return VT, (a, b)


def step_counts(method, ssets, ssigns, srows, nc, masks):
    """Per scored row (a set, a step or a level): observed (cases, controls) of the (+) and of the (-) union, the unions'
    sizes, and per permutation the cases among them -- the counts ``test_gpu_sequential.reference_null`` reads the table at."""
    d = np.asarray(srows) != 0
    n = d.shape[1]
    case = np.arange(n) < nc
    mk = np.asarray(masks).astype(np.int32)
    S, K = len(ssets), len(mk)
    out = types.SimpleNamespace(tp=np.zeros(S, np.int64), tn=np.zeros(S, np.int64), a=np.zeros((S, K), np.int64),
                                b=np.zeros((S, K), np.int64), oa=np.zeros(S, np.int64), ob=np.zeros(S, np.int64),
                                scored=np.zeros(S, bool))
    for s, m in enumerate(ssets):
        m = np.asarray(m, np.int64)
        if (m < 0).any():
            continue
        out.scored[s] = True
        sg = np.ones(len(m), np.int64) if ssigns is None else np.asarray(ssigns[s], np.int64)
        neg = (sg == -1) if method == 2 else np.zeros(len(m), bool)
        pos_u = d[m[~neg]].any(axis=0) if (~neg).any() else np.zeros(n, bool)
        neg_u = d[m[neg]].any(axis=0) if neg.any() else np.zeros(n, bool)
        out.tp[s], out.tn[s] = pos_u.sum(), neg_u.sum()
        out.a[s], out.b[s] = mk @ pos_u.astype(np.int32), mk @ neg_u.astype(np.int32)
        out.oa[s], out.ob[s] = (pos_u & case).sum(), (pos_u & ~case).sum()
    return out


def null_terms(method, VT, n, c):
    """(x, y, y transposed) float64 [rows][perms]: the two terms of every null score before the fold (method 1: y = 0), and
    the (-) term read at the transposed cell, vtmax[b][tn - b] where the definition reads vtmax[tn - b][b]."""
    a, b, tp_, tn = c.a, c.b, c.tp[:, None], c.tn[:, None]
    if method == 1:
        x = report._vt_cell(VT, n, a, tp_ - a)
        return x, np.zeros_like(x), np.zeros_like(x)
    return report._vt_max(VT, n, a, tp_ - a), report._vt_max(VT, n, tn - b, b), report._vt_max(VT, n, b, tn - b)


_BUILT: dict = {}


def build(entry, family, method, spec, nc=70, nt=61, square=False):
    """One case, computed once and never changed: the input, the table, the masks, the definition's null matrix and its
    answer.  ``spec`` = (table seed, variant, trial of make_input, max_perms)."""
    key = (entry, family, method, tuple(spec), nc, nt, square)
    if key in _BUILT:
        return _BUILT[key]
    seed, variant, trial, max_perms = spec
    c = types.SimpleNamespace(entry=entry, family=family, method=method, spec=tuple(spec), nc=nc, nt=nt, max_perms=max_perms,
                              extra=None, odds=None, att=None, cell=None)
    if entry in ("prefix", "dose"):
        c.rows, c.sets, c.signs, _, c.extra = tp.make_input(entry, method, nc, nt, 1, trial)
    else:
        c.rows, c.sets, c.signs, _ = t.make_input(method, nc, nt, 1, trial)
    c.VT = case_table(family, nc, nt, seed, variant, square)
    if family in SEQ_PLANTED:
        c.VT, c.cell = plant(c.VT, method, c.rows, c.sets, c.signs, nc, SEQ_PLANTED[family])
    if entry == "weighted":
        c.odds = tw.make_odds(method, nc, nt, 1, None, trial)
        thr, _ = api.weighted_thresholds(c.odds, nc, nt, None)
        c.masks, c.att = report.weighted_masks(thr, nc, nt, P_MAX, PERM_SEED, None)
    else:
        c.masks = report.permutation_masks(nc, nt, P_MAX, PERM_SEED, None)
    S = len(c.sets)
    if entry in ("prefix", "dose"):
        c.srows, c.ssets, c.ssigns, c.owner = tp.step_lists(entry, method, c.sets, c.signs, c.rows, c.extra)
    else:
        c.srows, c.ssets, c.ssigns, c.owner = c.rows, c.sets, c.signs, np.arange(S)
    c.valid = np.array([int(all(m >= 0 for m in s)) for s in c.sets])
    with np.errstate(all="ignore"):
        c.step_obs, c.step_null, _ = t.reference_null(method, c.ssets, c.ssigns, c.srows, nc, c.VT, c.masks)
        c.full_obs = t.reference_null(method, c.sets, c.signs, c.rows, nc, c.VT, c.masks[:0])[0]     # of the sets' unions
        if entry in ("prefix", "dose"):
            c.ref = report.adaptive_sequential_reference(c.step_obs, c.step_null, c.owner, S, c.valid, HITS, max_perms)
            c.obs, c.null = c.ref["score"], report.prefix_reference(c.step_obs, c.step_null, c.owner, S, c.valid)["null_max"]
        elif entry == "weighted":
            c.ref = report.weighted_sequential_reference(c.step_null, c.step_obs, c.valid, HITS, max_perms, c.att)
            c.obs, c.null = c.step_obs, c.step_null
        else:
            c.ref = report.sequential_reference(c.step_null, c.step_obs, c.valid, HITS, max_perms)
            c.obs, c.null = c.step_obs, c.step_null
    for v in vars(c).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _BUILT[key] = c
    return c


def stops(e, hits):
    """(n_hit, n_perm) of ``sequential_reference`` for rows of flags e [sets][max_perms], vectorised."""
    cs = np.cumsum(e, axis=1)
    P = e.shape[1]
    total = cs[:, -1] if P else np.zeros(len(e), np.int64)
    reached = total >= hits
    first = (cs >= hits).argmax(axis=1) + 1 if P else np.zeros(len(e), np.int64)
    return np.where(reached, hits, total), np.where(reached, first, P)


def set_null(c, step_null):
    """A step null matrix as the entry's own: the maximum over every set's rows (the rows themselves where a set is one)."""
    if c.entry not in ("prefix", "dose"):
        return step_null
    return report.prefix_reference(c.step_obs, step_null, c.owner, len(c.sets), c.valid)["null_max"]


def provoked(c):
    """name -> bool: which of the conditions of this file the definition's results of case ``c`` hold."""
    mp, S = c.max_perms, len(c.sets)
    n = c.nc + c.nt
    ok = c.valid != 0
    obs = np.asarray(c.obs, np.float64)
    n_hit, n_perm, stopped = c.ref["n_hit"], c.ref["n_perm"], c.ref["stopped"] != 0
    with np.errstate(all="ignore"):
        null = np.where(ok[:, None], c.null[:, :mp], np.float32(0)).astype(np.float32)
        null64 = null.astype(np.float64)
        o32 = obs.astype(np.float32)
        base = stops(null64 >= obs[:, None], HITS)
        assert (base[0][ok] == n_hit[ok]).all() and (base[1][ok] == n_perm[ok]).all()      # `stops` is the definition
        differs = lambda e: bool((ok & ((e[0] != base[0]) | (e[1] != base[1]))).any())
        used = ok[:, None] & (np.arange(mp)[None, :] < n_perm[:, None])                    # the permutations a set reads
        at_hits = ok & stopped & (n_perm == HITS)
        zero = obs == 0
        eq32 = used & (null == o32[:, None]) & (obs > 0)[:, None]
        up = obs == np.nextafter(o32.astype(np.float64), np.inf)
        dn = obs == np.nextafter(o32.astype(np.float64), -np.inf)
        got = {
            "score -0 stops at hits": (at_hits & zero & np.signbit(obs)).any(),
            "score +0 stops at hits": (at_hits & zero & ~np.signbit(obs)).any(),
            "negative score stops at hits": (at_hits & (obs < 0) & np.isfinite(obs)).any(),
            "f64 tie decides": bool((ok & (obs > 0) & ((stops(null64 > obs[:, None], HITS)[1] != base[1]))).any()),
            "NaN score never counts": (ok & np.isnan(obs) & (n_hit == 0) & (n_perm == mp) & ~stopped).any(),
            "-inf score stops at hits": (at_hits & np.isneginf(obs)).any(),
            "+inf score counts at +inf nulls": (ok & np.isposinf(obs) & (n_hit > 0)).any(),
            "denormal score": (ok & (obs > 0) & (obs < FLT_MIN)).any(),
            "denormal null": (used & (null > 0) & (null < FLT_MIN)).any(),
            "f32-equal null above counts": (eq32 & (null64 > obs[:, None])).any(),
            "f32-equal null below does not count": (eq32 & (null64 < obs[:, None])).any(),
            "rounding decides": differs(stops(null >= o32[:, None], HITS)),
            "null +inf under a finite score": (used & np.isposinf(null) & np.isfinite(obs)[:, None]).any(),
            "ulp above: the f32 value never counts": (eq32 & up[:, None]).any(),
            "ulp below: the f32 value counts": (eq32 & dn[:, None]).any(),
        }
        # ---- on the table cells themselves ----
        k = step_counts(c.method, c.ssets, c.ssigns, c.srows, c.nc, c.masks[:mp])
        x, y, yt = null_terms(c.method, c.VT, n, k)
        snull = c.step_null[:, :mp]
        folded = report._fold_f32(x + y)
        assert (folded.view(np.uint32)[k.scored] == snull.view(np.uint32)[k.scored]).all()   # the terms are the definition's
        live = k.scored[:, None] & used[c.owner]
        got["null rounds to +0"] = (live & (x + y > 0) & (snull == 0)).any()
        got["padding folds to 0 in the null"] = (live & ((x == -1) | (y == -1)) & (snull == 0)).any()
        got["padding in the score"] = (at_hits & np.isin(obs, (-1.0, -2.0))).any() and c.family == "shapes"
        if c.method == 2:
            got["a sum of two finite halves overflows"] = (live & (x < FLT_MAX) & (y < FLT_MAX) & np.isposinf(snull)).any()
            alt = report._fold_f32(x + yt)
            got["mirror: the transposed (-) half reads another value"] = (live & (alt.view(np.uint32) != snull.view(np.uint32))).any()
            alt_set = np.where(ok[:, None], set_null(c, alt), np.float32(0)).astype(np.float64)
            got["mirror decides"] = differs(stops(alt_set >= obs[:, None], HITS))
            R, C = c.VT.shape
            inside = lambda r, q: (r < R) & (q < C)
            tp_, tn = k.tp[:, None], k.tn[:, None]
            got["transposed read outside the table"] = bool(
                (live & ((inside(k.a, tp_ - k.a) != inside(tp_ - k.a, k.a)) | (inside(tn - k.b, k.b) != inside(k.b, tn - k.b)))).any())
        if c.cell is not None:
            s = PLANTED_SET
            row = int(np.flatnonzero(c.owner == s)[0])
            same = used[s] & (k.a[row] == c.cell[0]) & (k.tp[row] - k.a[row] == c.cell[1])
            finite_above = bool(np.isfinite(obs[s]) and obs[s] > FLT_MAX)
            got["planted beyond FLT_OVERFLOW: its own cell counts"] = bool(
                finite_above and obs[s] >= FLT_OVERFLOW and (same & np.isposinf(null[s])).any() and n_hit[s] >= 1)
            got["planted below FLT_OVERFLOW: its own cell does not count"] = bool(
                finite_above and obs[s] < FLT_OVERFLOW and (same & (null[s] == np.float32(FLT_MAX))).any())
        if c.entry in ("prefix", "dose"):
            so = c.step_obs
            kinds = {"NaN": np.isnan(so), "-0": (so == 0) & np.signbit(so), "+inf": np.isposinf(so)}
            among = dict.fromkeys(kinds, False)
            not_last = varies = False
            for s in np.flatnonzero(ok).tolist():
                rws = np.flatnonzero(c.owner == s)
                if len(rws) < 2:
                    continue
                fin = np.isfinite(so[rws]) & (so[rws] != 0)
                for name, m in kinds.items():
                    among[name] |= bool(m[rws].any() and fin.any())
                not_last |= bool(0 <= c.ref["best_step"][s] < len(rws) - 1)
                top = snull[rws][:, :int(n_perm[s])]
                if top.shape[1]:
                    alone = (top == top.max(axis=0)).sum(axis=0) == 1
                    varies |= len(set(top.argmax(axis=0)[alone].tolist())) >= 2
            got["the best step is not the last"] = not_last
            got["the null maximum moves between the steps"] = varies
            for name in kinds:
                got[f"a {name} step among finite ones"] = among[name]
    return {name: bool(v) for name, v in got.items()}


def asked(entry, family, variant, method):
    """What one case must hold by construction of its family and variant."""
    if family == "zeros":
        return ["score -0 stops at hits", "score +0 stops at hits", "negative score stops at hits", "f64 tie decides"]
    if family == "nonfinite":
        mirror = ["mirror: the transposed (-) half reads another value", "mirror decides"] if method == 2 and variant < 3 else []
        if entry == "dose" and variant % 3:
            # a set's upper levels are carried by nobody or by few: they read table[0][0] and its neighbours, which are
            # finite or +inf in these variants, and a NaN or -inf level is skipped or beaten
            return (["negative score stops at hits", "a NaN step among finite ones"] if variant % 3 == 1 else
                    ["+inf score counts at +inf nulls", "a +inf step among finite ones"]) + mirror
        if entry == "prefix" and variant % 3 == 2:
            # one cell in a thousand is +inf: a table that puts one under a step of a longer set seldom holds a NaN and a
            # -inf score besides; variants 0 and 1 hold those
            return ["+inf score counts at +inf nulls", "a +inf step among finite ones"] + mirror
        return (["NaN score never counts", "-inf score stops at hits"] +
                (["+inf score counts at +inf nulls"] if variant % 3 == 2 else []) + mirror)
    if family == "tiny":
        return ["denormal score", "denormal null", "f32-equal null above counts", "f32-equal null below does not count",
                "rounding decides", "null rounds to +0"]
    if family == "huge":
        return ["null +inf under a finite score"]
    if family == "huge+hi":
        return ["planted beyond FLT_OVERFLOW: its own cell counts"]
    if family == "huge+mid":
        return ["planted below FLT_OVERFLOW: its own cell does not count", "rounding decides"]
    if family == "ladder":
        if variant == 1 and method == 2:
            # the band: a score is the sum of two cells of [8, 10.5), each a level or an ulp off it -- seldom one f64 ulp
            # off an f32 value itself; variant 0 holds those
            return ["f32-equal null below does not count", "rounding decides"]
        return ["ulp above: the f32 value never counts", "ulp below: the f32 value counts", "rounding decides"]
    return []


def asked_of_all(entry, method):
    """... and what the union of an entry's cases must hold besides, per method."""
    out = ["padding in the score", "padding folds to 0 in the null"]
    if method == 2:
        out += ["transposed read outside the table"]
        if entry != "weighted":
            out += ["a sum of two finite halves overflows"]
    if entry in ("prefix", "dose"):
        out += ["the best step is not the last", "the null maximum moves between the steps", "a NaN step among finite ones",
                "a -0 step among finite ones", "a +inf step among finite ones"]
    return out


def cases_of(entry, method):
    """[(family, spec)] of an entry and method, in the order of FAMILIES."""
    return [(family, spec) for family in FAMILIES for spec in SEQ_TABLE_CASES.get((entry, family, method), [])]


# ---- the cases are all there ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("entry", SEQ_ENTRIES)
def test_every_family_and_variant_has_its_case(entry):
    for method in METHODS:
        for family in FAMILIES:
            want = list(variants_of(entry, family, method))
            have = [spec[1] for spec in SEQ_TABLE_CASES.get((entry, family, method), [])]
            assert have == want, (entry, family, method, have, want)
            assert all(0 < spec[3] <= P_MAX for spec in SEQ_TABLE_CASES.get((entry, family, method), []))


# ---- every case holds what its family is there for -----------------------------------------------------------------------


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("entry", SEQ_ENTRIES)
def test_what_the_cases_provoke(entry, method):
    union: dict = {}
    for family, spec in cases_of(entry, method):
        c = build(entry, family, method, spec)
        if entry == "weighted":
            assert c.ref["first_left_over"] is None and not c.ref["refused"]
        got = provoked(c)
        missing = [name for name in asked(entry, family, spec[1], method) if not got[name]]
        assert not missing, (entry, family, method, spec, missing)
        for name, v in got.items():
            union[name] = union.get(name, False) or v
    missing = [name for name in asked_of_all(entry, method) if not union.get(name)]
    assert not missing, (entry, method, missing)


@pytest.mark.parametrize("entry", SEQ_ENTRIES)
def test_every_class_of_the_batches(entry):
    """Over all cases of an entry, at one 512-permutation tile a batch: a set in every class of
    test_gpu_sequential.classes_of, so that the retirement is inside the comparison."""
    total: dict = {}
    for method in METHODS:
        for family, spec in cases_of(entry, method):
            c = build(entry, family, method, spec)
            for name, v in t.classes_of(c.ref, c.valid, c.max_perms, CAP).items():
                total[name] = total.get(name, 0) + v
    assert total and all(v > 0 for v in total.values()), (entry, total)


def test_the_tiny_table_is_positive_and_the_shapes_are_padded():
    """What two conditions above lean on: a null of +0 under the tiny table is a rounding (no cell is 0 or negative), and
    the tables of the family `shapes` are positive, so a score of -1 or -2 there is the padding."""
    for m in METHODS:
        for seed, variant, _, _ in SEQ_TABLE_CASES[("sequential", "tiny", m)]:
            assert (special_table("tiny", 70, 61, seed, variant) > 0).all()
        for seed, variant, _, _ in SEQ_TABLE_CASES[("sequential", "shapes", m)]:
            assert (case_table("shapes", 70, 61, seed, variant) > 0).all()


# ---- step-down max-T of a join on the table families -----------------------------------------------------------------------

STEPDOWN_FAMILIES = ("zeros", "nonfinite", "tiny", "huge", "ladder")
STEPDOWN_TOP_K = 45
# (seed, variant) where the case TABLE_CASES names does not do: its nonfinite problems have no non-finite score among the
# 45 best of any level.  These have a -inf one (method 2 on a table with one-sided NaN cells: the mirror table is read)
STEPDOWN_CASES = {("nonfinite", "method1"): (1, 0), ("nonfinite", "method2"): (2, 0)}
_STEPDOWN: dict = {}


def stepdown_problem(kind, method):
    """Cpu(table_problem(kind, "p70", method, top_k=45)); for zeros the top_k that cuts some level among its zeros."""
    from test_gpu_exceed import LEVELS, Cpu
    key = (kind, method)
    if key not in _STEPDOWN:
        top_k, case = STEPDOWN_TOP_K, STEPDOWN_CASES.get(key)
        if kind == "zeros":
            full = Cpu(table_problem(kind, "p70", method))
            cuts = [zeros_cut_top_k(full.want[f"lst{l + 1}"].all_scores) for l in range(len(LEVELS))]
            top_k = min(k for k in cuts if k)
        _STEPDOWN[key] = Cpu(table_problem(kind, "p70", method, top_k=top_k, case=case))
    return _STEPDOWN[key]


@pytest.mark.parametrize("method", ["method1", "method2"])
@pytest.mark.parametrize("kind", STEPDOWN_FAMILIES)
def test_stepdown_problems_on_special_tables(kind, method):
    from test_gpu_exceed import LEVELS
    from test_gpu_stepdown import reference, top_rows
    cpu = stepdown_problem(kind, method)
    tops = {name: top_rows(cpu, name) for name in LEVELS}
    refs = {name: reference(cpu, name, top) for name, top in tops.items() if len(top[2])}
    assert refs
    for name, want in refs.items():
        np.testing.assert_array_equal(want["scores"].view(np.uint64), tops[name][2].view(np.uint64))    # join score = set score
    assert any(len(set(top[2].tolist())) < len(top[2]) for top in tops.values()), "no tied scores among the top rows"
    assert any((want["n_ge"] < want["single"]).any() for want in refs.values()), "no row gains from stepping down"
    if kind == "zeros":
        assert any(((top[2] == 0) & np.signbit(top[2])).any() and ((top[2] == 0) & ~np.signbit(top[2])).any() for top in tops.values())
    if kind == "nonfinite":
        lists = [cpu.want[f"lst{l + 1}"].scores for l in range(len(LEVELS))]
        assert any((~np.isfinite(s)).any() and np.isfinite(s).any() for s in lists), "no level with non-finite top scores"


# ---- the refusal of the weighted entry on a NaN score ----------------------------------------------------------------------


def refusal_case(method):
    """The weighted nonfinite case under a max_attempts that leaves a permutation over: (case, max_attempts, the masks' accepted
    attempts under it, the definition's answer).  max_attempts is the largest accepted attempt of the case's own 3,000
    permutations, so the first permutation that needed it has none below it."""
    c = build("weighted", "nonfinite", method, SEQ_TABLE_CASES[("weighted", "nonfinite", method)][0])
    cap = int(c.att[:c.max_perms].max())
    thr, _ = api.weighted_thresholds(c.odds, c.nc, c.nt, None)
    masks, att = report.weighted_masks(thr, c.nc, c.nt, c.max_perms, PERM_SEED, None, max_attempts=cap)
    with np.errstate(all="ignore"):
        obs, null, valid = t.reference_null(method, c.sets, c.signs, c.rows, c.nc, c.VT, masks)
        ref = report.weighted_sequential_reference(null, obs, valid, HITS, c.max_perms, att)
    return c, cap, att, ref


@pytest.mark.parametrize("method", METHODS)
def test_a_nan_score_and_a_left_over_permutation_refuse(method):
    c, cap, att, ref = refusal_case(method)
    R = ref["first_left_over"]
    assert R is not None and 0 < R < c.max_perms and ref["refused"]
    nan = (c.valid != 0) & np.isnan(c.obs)
    assert nan.any() and (ref["stopped"][nan] == 0).all() and ref["n_active"] >= int(nan.sum())
    assert (att[:R] != report.WEIGHTED_NONE).all()
