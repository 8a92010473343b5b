"""Decorated p-values on the device: k_decorated_null against a CPU restatement of its urn sampler (every draw count),
the sampler's distribution against the exact hypergeometric, the front end on a planted pathway, and one call at
configs[4] geometry."""
from __future__ import annotations

import importlib.util
import math
import os
import time

import numpy as np
import pandas as pd
import pytest

from geneticscre_amd import api, report, synth
from test_decorated_host import r_decorated_splits, random_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the sampler, restated (gcre_kernels.h dp_split_key / dp_perm_base, gcre_decorated.hip dp_urn) -------------------


def mix64(z):
    with np.errstate(over="ignore"):                            # arithmetic mod 2^64, as on the device
        z = np.asarray(z, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def split_key(seed, s):
    with np.errstate(over="ignore"):
        return mix64(np.uint64(seed) ^ (np.uint64(0xD1B54A32D192ED03) * np.uint64(s + 1)))


def perm_base(key, K):
    with np.errstate(over="ignore"):
        return mix64(np.uint64(key) ^ (np.uint64(0x51ED270B7F3C9A1D) * (np.arange(K, dtype=np.uint64) + np.uint64(1))))


def urn(base, t0, k, rem, need):
    """dp_urn for every permutation at once: successes among k draws, draw t reading mix64(base + t0 + t)."""
    K = len(base)
    rem = np.full(K, rem, np.uint64)
    need = np.full(K, need, np.uint64)
    got = np.zeros(K, np.int64)
    done = np.zeros(K, bool)
    for t in range(k):
        stop0 = ~done & (need == 0)
        rest = ~done & ~stop0 & (need == rem)
        got[rest] += k - t
        done |= stop0 | rest
        live = ~done
        u = mix64(base + np.uint64(t0 + t))
        # floor(u * rem / 2^64) from 32-bit halves (rem < 2^32: no overflow)
        pick = ((u >> np.uint64(32)) * rem + (((u & np.uint64(0xFFFFFFFF)) * rem) >> np.uint64(32))) >> np.uint64(32)
        hit = live & (pick < need)
        got += hit
        need -= hit.astype(np.uint64)
        rem -= live.astype(np.uint64)
    return got


def restated_counts(rec, strata_rec, seed, K):
    """[splits][K][2]: what k_decorated_null draws for every split."""
    out = np.zeros((len(rec), K, 2), np.int64)
    for s, r in enumerate(rec):
        if not r["valid"]:
            continue
        base = perm_base(split_key(seed, s), K)
        if strata_rec is None:
            out[s, :, 0] = urn(base, 0, int(r["k_pos"]), int(r["pop_pos"]), int(r["succ_pos"]))
            out[s, :, 1] = urn(base, int(r["k_pos"]), int(r["k_neg"]), int(r["pop_neg"]), int(r["succ_neg"]))
            continue
        t0 = 0
        for pop, cases, kp, kn in strata_rec[s].tolist():      # strata ascending, pos then neg
            x = urn(base, t0, kp, pop, cases)
            t0 += kp
            out[s, :, 1] += urn(base, t0, kn, np.full(K, pop - kp), (pop - cases) - (kp - x))
            t0 += kn
            out[s, :, 0] += x
    return out


def vt_lookup(VT, a, b):
    a, b = np.asarray(a), np.asarray(b)
    ok = (a < VT.shape[0]) & (b < VT.shape[1])
    return np.where(ok, VT[np.minimum(a, VT.shape[0] - 1), np.minimum(b, VT.shape[1] - 1)], -1.0)


def perm_scores(r, xp, xn, method, VT):
    """The permutation score of split r when the pos draw holds xp cases and the neg draw xn controls."""
    yp, yn = int(r["k_pos"]) - xp, int(r["k_neg"]) - xn
    if method == 1:
        return vt_lookup(VT, r["case_pos1"] + xp + r["case_neg1"] + xn, r["ctrl_pos1"] + yp + r["ctrl_neg1"] + yn)
    return vt_lookup(VT, r["case_pos1"] + xp, r["ctrl_pos1"] + yp) + vt_lookup(VT, r["case_neg1"] + xn, r["ctrl_neg1"] + yn)


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("stratified", [False, True])
def test_device_draws_match_restatement(method, stratified):
    """perm_counts, n_ge and the p-values of k_decorated_null equal the CPU restatement's; the observed scores equal the
    host stage's bit for bit; a split whose gene adds nothing has p = 1."""
    nc, nt, data, paths, signs, VT = random_case(500 + method, method)
    K = 300
    strata = (np.arange(nc + nt) * 7 % 3).astype(np.int32) if stratified else None
    ex = api.JoinExec(method, nc, nt, K)
    ex.set_value_table(VT)
    rec, counts = ex.decorated_pvalues(paths, data, signs, strata=strata, seed=99, return_counts=True)
    host, st = api.decorated_splits(method, nc, nt, paths, data, signs, VT, strata)
    for f in ("path", "direction", "j", "valid", "cases1", "ctrls1", "cases2", "ctrls2", "k_pos", "k_neg"):
        np.testing.assert_array_equal(rec[f], host[f])
    np.testing.assert_array_equal(rec["score"].view(np.uint64), host["score"].view(np.uint64))
    want = restated_counts(host, st, 99, K)
    np.testing.assert_array_equal(counts, want)
    for s, r in enumerate(host):
        if not r["valid"]:
            assert np.isnan(rec[s]["pvalue"])
            continue
        n_ge = int((perm_scores(r, want[s, :, 0], want[s, :, 1], method, VT) >= r["score"]).sum())
        assert int(rec[s]["n_ge"]) == n_ge, s
        assert rec[s]["pvalue"] == n_ge / K
    assert rec[0]["k_pos"] + rec[0]["k_neg"] == 0 and rec[0]["pvalue"] == 1.0
    assert (counts[:, :, 0] <= rec["k_pos"][:, None]).all() and (counts[:, :, 1] <= rec["k_neg"][:, None]).all()
    # the same call again: the same draws; another seed: other draws
    rec2, counts2 = ex.decorated_pvalues(paths, data, signs, strata=strata, seed=99, return_counts=True)
    np.testing.assert_array_equal(counts2, counts)
    np.testing.assert_array_equal(rec2["n_ge"], rec["n_ge"])
    _, counts3 = ex.decorated_pvalues(paths, data, signs, strata=strata, seed=100, return_counts=True)
    assert not np.array_equal(counts3, counts)
    ex.close()


@pytest.mark.parametrize("stratified", [False, True])
@pytest.mark.parametrize("method", [1, 2])
def test_special_tables(method, stratified):
    """The table families of tests/helpers.py and a table shorter than the cohort both ways: k_decorated_observed and
    k_decorated_null read the raw table in f64 and count ``ps >= o``.  On the transcription alone the splits hold observed
    values of NaN, both zeros, both infinities and an f32 denormal, and a split with a permutation that ties its observed
    value exactly (asserted again here; tests/test_decorated_host.py holds it without a GPU).  The observed scores equal
    r_decorated_splits' bit for bit, the urn counts and n_ge the restatement's.  A NaN observed value is reached by no
    permutation, as in R (DecoratedPvalue.R:290, ``which(scores >= score)`` is empty): n_ge = 0, and the p-value is n_ge / K
    like every other."""
    from test_decorated_host import TABLE_KINDS, TABLE_PERMS, observed_kinds, table_case, table_expectation, table_strata
    union, tie = {}, False
    for kind in TABLE_KINDS:
        nc, nt, data, paths, signs, VT = table_case(kind, method)
        strata = table_strata(nc, nt) if stratified else None
        want = r_decorated_splits(data, paths, signs, nc, nt, method, VT, strata)
        host, st, counts_want, n_ge, ties = table_expectation(kind, method, stratified)
        valid = host["valid"] != 0
        assert [w["valid"] for w in want] == valid.astype(int).tolist()
        for k, v in observed_kinds([w["score"] for w in want if w["valid"]]).items():
            union[k] = union.get(k, False) or v
        tie |= bool((valid & (host["k_pos"] + host["k_neg"] > 0) & (ties > 0) & (ties < TABLE_PERMS)).any())
        ex = api.JoinExec(method, nc, nt, TABLE_PERMS)
        try:
            ex.set_value_table(VT)
            rec, counts = ex.decorated_pvalues(paths, data, signs, strata=strata, seed=99, return_counts=True)
        finally:
            ex.close()
        assert len(rec) == len(want)
        for s, w in enumerate(want):
            if not w["valid"]:
                assert np.isnan(rec[s]["score"]) and np.isnan(rec[s]["pvalue"])
                continue
            ws, gs = np.float64(w["score"]), np.float64(rec[s]["score"])
            assert (np.isnan(ws) and np.isnan(gs)) or ws.view(np.uint64) == gs.view(np.uint64), (kind, s, gs, ws)
            assert int(rec[s]["n_ge"]) == n_ge[s], (kind, s)
            assert rec[s]["pvalue"] == n_ge[s] / TABLE_PERMS, (kind, s)
            if np.isnan(ws):
                assert int(rec[s]["n_ge"]) == 0
        np.testing.assert_array_equal(counts, counts_want, err_msg=kind)
        for f in ("path", "direction", "j", "cases1", "ctrls1", "cases2", "ctrls2", "k_pos", "k_neg"):
            np.testing.assert_array_equal(rec[f], host[f], err_msg=f"{kind} {f}")
    assert all(union.values()), union
    assert tie


def test_device_errors():
    nc, nt, data, paths, signs, VT = random_case(9, 1)
    ex = api.JoinExec(1, nc, nt, 10)
    with pytest.raises(ValueError):
        ex.decorated_pvalues(paths, data, signs)               # no value table yet
    ex.set_value_table(VT)
    with pytest.raises(IndexError):
        ex.decorated_pvalues([[0, len(data)]], data)           # row out of range
    ex.close()
    ex2 = api.JoinExec(2, nc, nt, 10)
    ex2.set_value_table(VT)
    d = api._DpInput(1, nc, nt, paths, data, signs, None, 10, 0)   # method 1 input on a method 2 context
    out = d.out()
    n_out = api.ctypes.c_int64(0)
    assert api._decorated_lib().gcre_decorated_pvalues(ex2._h, api.ctypes.byref(d.c), api._ptr(out), len(out),
                                                       api.ctypes.byref(n_out), None) == api.GCRE_ERR_ASSERT
    ex2.close()


# ---- distribution ------------------------------------------------------------------------------------------------------


def hyper_pmf(pop, succ, k):
    tot = math.comb(pop, k)
    return np.array([math.comb(succ, x) * math.comb(pop - succ, k - x) / tot for x in range(k + 1)])


def chi_square_ok(hist, pmf, K):
    exp = pmf * K
    keep = exp >= 5
    obs_k, exp_k = hist[:len(pmf)][keep], exp[keep]
    rest_o, rest_e = hist.sum() - obs_k.sum(), K - exp_k.sum()
    chi = float(((obs_k - exp_k) ** 2 / exp_k).sum())
    dof = int(keep.sum()) - 1
    if rest_e >= 5:
        chi += (rest_o - rest_e) ** 2 / rest_e
        dof += 1
    assert dof >= 1
    return chi, dof, abs(chi - dof) < 5 * math.sqrt(2 * dof)


@pytest.mark.parametrize("stratified", [False, True])
def test_device_draws_are_hypergeometric(stratified):
    """2e5 permutations of a few splits: the histogram of each split's draw count against the exact hypergeometric pmf
    (with strata: the convolution of the per-stratum ones, the neg urn conditioned on nothing since only one half
    draws), chi-square; every p-value within 5 sigma of the exact tail P(score(X) >= score)."""
    nc, nt, K, method = 150, 190, 200000, 2
    n = nc + nt
    rng = np.random.default_rng(7)
    data = (rng.random((6, n)) < np.array([0.15, 0.1, 0.2, 0.08, 0.12, 0.1])[:, None]).astype(np.int32)
    data[1, :20] = 1                                            # gene 1: more cases than chance
    paths, signs = [[0, 1, 2], [3, 4, 5]], [[1, 1, -1], [1, -1, 1]]
    VT = api.values_table(nc, nt)
    strata = (np.arange(n) * 5 % 4).astype(np.int32) if stratified else None
    ex = api.JoinExec(method, nc, nt, K)
    ex.set_value_table(VT)
    rec, counts = ex.decorated_pvalues(paths, data, signs, strata=strata, seed=2026, return_counts=True)
    _, st = api.decorated_splits(method, nc, nt, paths, data, signs, VT, strata)
    ex.close()
    checked = 0
    for s, r in enumerate(rec):
        half = 0 if r["k_pos"] > 0 else 1
        k = int(r["k_pos"] if half == 0 else r["k_neg"])
        if k == 0:
            continue
        if st is None:
            pmf = hyper_pmf(int(r["pop_pos"]), int(r["succ_pos"]), k) if half == 0 else \
                hyper_pmf(int(r["pop_neg"]), int(r["succ_neg"]), k)
        else:
            pmf = np.ones(1)
            for pop, cases, kp, kn in st[s].tolist():
                kk = kp if half == 0 else kn
                if kk:
                    pmf = np.convolve(pmf, hyper_pmf(pop, cases if half == 0 else pop - cases, kk))
        x = counts[s, :, half]
        hist = np.bincount(x, minlength=len(pmf)).astype(np.float64)
        assert len(hist) == len(pmf)
        chi, dof, ok = chi_square_ok(hist, pmf, K)
        assert ok, (s, chi, dof)
        # the exact tail of the permutation score
        xs = np.arange(len(pmf))
        xp, xn = (xs, np.zeros_like(xs)) if half == 0 else (np.zeros_like(xs), xs)
        p_exact = float(pmf[perm_scores(r, xp, xn, method, VT) >= r["score"]].sum())
        sigma = math.sqrt(max(p_exact * (1 - p_exact), 1e-12) / K)
        assert abs(r["pvalue"] - p_exact) <= 5 * sigma + 1.0 / K, (s, r["pvalue"], p_exact)
        checked += 1
    assert checked >= 6


# ---- front end -------------------------------------------------------------------------------------------------------


def _planted_case(seed, nc=48, nt=52):
    """test_gpu_api's planted-pathway dataset with 8 cases per planted gene: a -> b -> c carry cases 0-7, 8-15, 16-23."""
    rng = np.random.default_rng(seed)
    g, src, trg, sign = synth.signed_network(60, 200, rng)
    uid = np.arange(g) * 5 + 100
    symbols = [f"G{u}" for u in uid]
    n = nc + nt
    data = (rng.random((g, n)) < 0.02).astype(np.int32)
    a, b = int(src[0]), int(trg[0])
    c = int(trg[np.flatnonzero(src == b)[0]])
    for k, gene in enumerate((a, b, c)):
        data[gene] = 0
        data[gene, 8 * k:8 * k + 8] = 1
    return symbols, data, (uid, symbols, uid[src], uid[trg], sign), (f"G{uid[a]}", f"G{uid[b]}", f"G{uid[c]}")


@pytest.mark.parametrize("signed", [False, True])
def test_gwaspa_decorated_table(signed):
    nc, nt, K = 48, 52, 4000
    genes, data, network, (a, b, c) = _planted_case(5)
    kw = dict(signed=signed, threshold=0.2, top_k=6, path_length=4, n_permutations=K, seed=31)
    plain = report.gwaspa(genes, data, nc, nt, network, **kw)
    out = report.gwaspa(genes, data, nc, nt, network, decorated_pvalues=True, **kw)
    assert "Decorated.Pvalues.Results" not in plain
    pd.testing.assert_frame_equal(out["GWASPA.Results"], plain["GWASPA.Results"])
    res, dec = out["GWASPA.Results"], out["Decorated.Pvalues.Results"]
    assert list(dec.columns) == report.DECORATED_COLUMNS
    multi = res[res["Lengths"] >= 2]
    assert len(dec) == int((2 * (multi["Lengths"] - 1)).sum())
    assert (dec["Lengths"] >= 2).all() and dec["Lengths"].is_monotonic_increasing
    # counts: the host transcription on the preprocessed dataset
    g2, d2 = report.preprocess_table(genes, data, 0.2, nc, nt)
    row_of = {s: i for i, s in enumerate(g2)}
    order = [i for L in range(2, 5) for i in np.flatnonzero(res["Lengths"].to_numpy() == L)]
    paths, signs = [], []
    for i in order:
        hops = [h.split(" ") for h in res["SignedPaths"].iat[i].split(" -> ")]
        paths.append([row_of.get(h[0], -1) for h in hops])
        signs.append([1 if h[1] == "(+)" else -1 for h in hops])
    want = r_decorated_splits(d2, paths, signs, nc, nt, 2 if signed else 1, api.values_table(nc, nt))
    got = dec[["Subpaths1_Cases", "Subpaths1_Controls", "Subpaths2_Cases", "Subpaths2_Controls"]].to_numpy().tolist()
    assert got == [[w.get("cases1", 0), w.get("ctrls1", 0), w.get("cases2", 0), w.get("ctrls2", 0)] for w in want]
    assert dec["DecoratedPvalues"].between(0, 1).all()
    # the planted path: gene b adds 8 cases and no control to a
    row = dec[(dec["Paths"] == f"{a} -> {b} -> {c}") & (dec["Direction"] == "Forward") & (dec["Subpaths1"] == a)]
    assert len(row) == 1, dec[["Paths", "Direction", "Subpaths1"]]
    assert row["Subpaths2"].iat[0] == b and row["Subpaths2_Cases"].iat[0] + row["Subpaths2_Controls"].iat[0] == 8
    assert row["DecoratedPvalues"].iat[0] < 0.05, row


def test_configs4_geometry_time():
    """One call at configs[4] geometry (25,000 + 25,000 patients, 100,000 permutations, 200 splits): tools/decorated_time."""
    spec = importlib.util.spec_from_file_location("decorated_time", os.path.join(ROOT, "tools", "decorated_time.py"))
    dt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dt)
    data, paths, signs = dt.make_case()
    ex = api.JoinExec(2, dt.N_CASES, dt.N_CTRLS, dt.PERMS)
    ex.set_value_table(dt.corner_table(dt.N_CASES, dt.N_CTRLS, 4000))
    t0 = time.perf_counter()
    rec = ex.decorated_pvalues(paths, data, signs, seed=5)
    ms = (time.perf_counter() - t0) * 1e3
    ex.close()
    print(f"decorated p-values at configs[4] geometry: {len(rec)} splits x {dt.PERMS} permutations in {ms:.1f} ms "
          "(first call)")
    assert len(rec) == 200 and rec["valid"].all()
    assert ((rec["pvalue"] >= 0) & (rec["pvalue"] <= 1)).all()
    assert ms < 60000
