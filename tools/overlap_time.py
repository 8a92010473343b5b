"""Wall time of gcre_set_overlap (k_set_overlap) and of report.clump_paths.

    python tools/overlap_time.py [--shapes big,small] [--reps R] [--host-rows H] [--no-clump]

Shapes, every set against every set:
  big    10,000 sets of 5 genes, 25,000 + 25,000 patients (configs[4] width), genes carried by 0.5-5 % of the patients
  small   1,000 sets of 5 genes,  2,500 +  2,500 patients (configs[2] width)
Per shape one JSON line:
  call_ms       host clock around the C entry on rows packed beforehand and a `both` array touched beforehand: the host OR
                stage, the upload, every slab's launch and the read-back of `both` (the call ends synchronised)
  method_ms     JoinExec.set_overlap: the same plus packing the carrier matrix and allocating `both` in numpy
  estimate_valu_ms  2 VALU (v_and_b32, v_bcnt_u32_b32) per pair and dword, 2 cycles per wave64 instruction on each of
                1,024 SIMDs at 2.4 GHz: the instruction-issue bound of the dense form.  The kernel's own time comes from a
                separate run under rocprofv3 --kernel-trace --stats.
  host_ms_scaled  the same counts by a packed-word numpy loop (AND, np.bitwise_count, sum) over the first H `a` rows
                against all `b` rows, checked against the device, and SCALED to all rows: host_ms_rows * sets / H
Then report.clump_paths on a 1,000-row table over the small shape (paths through three strong genes and their
neighbours), with and without `conditional` (1,000 permutations): wall time, leads, leads with members, and the share of
the conditional call spent inside JoinExec.score_sets (one call over all member rows) and
inside api.values_table (the value table of the call's one context).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GCRE_QUIET", "1")
import numpy as np  # noqa: E402

SHAPES = {"big": (10000, 25000, 25000), "small": (1000, 2500, 2500)}
POOL, PATH_LEN = 2000, 5


def make_case(n_sets: int, n: int, seed: int = 20261017):
    rng = np.random.default_rng(seed)
    rows = rng.random((POOL, n), dtype=np.float32) < rng.uniform(0.005, 0.05, size=(POOL, 1)).astype(np.float32)
    sets = [rng.choice(POOL, size=PATH_LEN, replace=False).tolist() for _ in range(n_sets)]
    return rows, sets


def estimate_ms(na: int, nb: int, n: int) -> float:
    wd = 2 * ((n + 63) // 64)
    return na * nb * wd * 2 / 64 * 2 / (1024 * 2.4e9) * 1e3


def time_shape(name: str, reps: int, host_rows: int) -> None:
    from geneticscre_amd import api
    S, nc, nt = SHAPES[name]
    n = nc + nt
    rows, sets = make_case(S, n)
    ex = api.JoinExec(1, nc, nt, 0)
    lib = api._overlap_lib()
    packed = api.pack_carriers(rows, n)
    off = np.arange(0, (S + 1) * PATH_LEN, PATH_LEN, dtype=np.int64)
    mem = np.ascontiguousarray(np.concatenate(sets), np.int32)
    inp = api.gcre_set_input(S, api._ptr(off), api._ptr(mem), None, api._ptr(packed), len(packed), n)
    size = np.zeros((S, 2), np.int32)
    both = np.ones((S, S, 2), np.int32)   # touched: the page faults of a fresh array are not the library's
    call = []
    for i in range(reps + 1):             # the first call is the warm-up: code object, allocations
        t0 = time.perf_counter()
        rc = lib.gcre_set_overlap(ex._h, ctypes.byref(inp), None, S, None, S, api._ptr(size), api._ptr(both))
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, ex._lib.gcre_last_error(ex._h)
        if i:
            call.append(dt)
    launches = ex.overlap_launches() // (reps + 1)
    t0 = time.perf_counter()
    size2, both2 = ex.set_overlap(sets, rows)
    method_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(size2, size) and np.array_equal(both2, both)
    del both2
    ex.close()
    # the host: OR of the members as packed words, then AND + popcount of H rows against all of them
    U = np.bitwise_or.reduce(packed[np.asarray(sets)], axis=1)                       # [S][W]
    W = U.shape[1]
    cmask = np.zeros(W, np.uint64)
    for w in range(W):
        lo = min(max(nc - 64 * w, 0), 64)
        cmask[w] = np.uint64((1 << lo) - 1) if lo < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    H = min(host_rows, S)
    t0 = time.perf_counter()
    host = np.empty((H, S, 2), np.int32)
    for i in range(H):
        x = U[i][None, :] & U
        host[i, :, 0] = np.bitwise_count(x & cmask).sum(axis=1)
        host[i, :, 1] = np.bitwise_count(x & ~cmask).sum(axis=1)
    host_ms = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(host, both[:H])
    print(json.dumps({"tool": "overlap_time", "shape": name, "sets": S, "n_cases": nc, "n_ctrls": nt,
                      "pairs": S * S, "dwords_per_row": 2 * W, "launches_per_call": launches,
                      "both_mb": round(S * S * 8 / 2**20, 1),
                      "call_ms": [round(t, 2) for t in call], "best_call_ms": round(min(call), 2),
                      "method_ms": round(method_ms, 2), "estimate_valu_ms": round(estimate_ms(S, S, n), 3),
                      "host_rows": H, "host_ms_rows": round(host_ms, 1), "host_ms_scaled": round(host_ms * S / H, 0),
                      "carrier_frac_mean": round(float(size.sum(axis=1).mean()) / n, 4)}), flush=True)


def time_clump() -> None:
    import pandas as pd
    from geneticscre_amd import api, report
    S, nc, nt = SHAPES["small"]
    n = nc + nt
    rng = np.random.default_rng(7)
    rows = (rng.random((POOL, n)) < rng.uniform(0.002, 0.01, size=(POOL, 1))).astype(np.int32)
    genes = [f"G{i}" for i in range(POOL)]
    strong = [0, 1, 2]
    for g, dens in zip(strong, (0.15, 0.12, 0.09)):
        rows[g, :nc] |= (rng.random(nc) < dens).astype(np.int32)
    sets = []
    for i in range(S):   # two thirds of the paths run through a strong gene
        s = rng.choice(np.arange(3, POOL), size=PATH_LEN, replace=False).tolist()
        if i % 3:
            s[int(rng.integers(PATH_LEN))] = strong[int(rng.integers(3))]
        sets.append(s)
    C, _ = report.carrier_rows(sets, rows, n)
    ca, ct = C[:, :nc].sum(axis=1), C[:, nc:].sum(axis=1)
    df = pd.DataFrame({"SignedPaths": [" -> ".join(f"{genes[g]} (+)" for g in s) for s in sets],
                       "Paths": [" -> ".join(genes[g] for g in s) for s in sets],
                       "Lengths": np.full(S, PATH_LEN), "Scores": (ca - ct).astype(np.float64) ** 2 / (ca + ct + 1.0),
                       "Pvalues": np.zeros(S), "Cases": ca, "Controls": ct})
    spent = [0.0, 0]
    setup = [0.0]
    inner, inner_vt = api.JoinExec.score_sets, api.values_table

    def timed_vt(*a, **k):
        t0 = time.perf_counter()
        try:
            return inner_vt(*a, **k)
        finally:
            setup[0] += time.perf_counter() - t0

    api.values_table = timed_vt

    def timed(self, *a, **k):
        t0 = time.perf_counter()
        try:
            return inner(self, *a, **k)
        finally:
            spent[0] += time.perf_counter() - t0
            spent[1] += 1

    api.JoinExec.score_sets = timed
    kw = dict(r=0.5, threshold=1.0, n_permutations=1000, seed=3)
    report.clump_paths(df.iloc[:50], genes, rows, nc, nt, conditional=True, **kw)   # warm-up
    out = {}
    for cond in (False, True):
        spent[0], spent[1], setup[0] = 0.0, 0, 0.0
        t0 = time.perf_counter()
        got = report.clump_paths(df, genes, rows, nc, nt, conditional=cond, **kw)
        out[cond] = ((time.perf_counter() - t0) * 1e3, spent[0] * 1e3, spent[1], setup[0] * 1e3)
    api.JoinExec.score_sets, api.values_table = inner, inner_vt
    sizes = np.bincount(got["Clump"].to_numpy())
    print(json.dumps({"tool": "overlap_time", "what": "clump_paths", "rows": S, "n_cases": nc, "n_ctrls": nt, "r": 0.5,
                      "measure": "jaccard", "permutations": 1000, "leads": int(len(sizes)),
                      "leads_with_members": int((sizes > 1).sum()), "largest_clump": int(sizes.max()),
                      "clump_ms": round(out[False][0], 1), "conditional_ms": round(out[True][0], 1),
                      "score_sets_calls": out[True][2], "score_sets_ms": round(out[True][1], 1),
                      "score_sets_share": round(out[True][1] / out[True][0], 3),
                      "values_table_ms": round(out[True][3], 1)}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="big,small")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=64)
    ap.add_argument("--no-clump", action="store_true")
    a = ap.parse_args()
    for name in [s for s in a.shapes.split(",") if s]:
        time_shape(name, a.reps, a.host_rows)
    if not a.no_clump:
        time_clump()


if __name__ == "__main__":
    main()
