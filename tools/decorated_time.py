"""Wall time of one gcre_decorated_pvalues call at configs[4] geometry (bench.py "signed": 25,000 cases, 25,000 controls,
100,000 permutations, method 2): 10 paths of each length 2..5 = 200 splits, genes carried by 0.5-5 % of the patients
(a few hundred to 2,500 draws per split).  The call ends in a stream synchronise, so a host clock around it times the
device work; rocprofv3 --kernel-trace --stats gives k_decorated_null on its own.

    python tools/decorated_time.py [--perms K] [--reps R]

The value table is a cheap stand-in (half the 2 x 2 chi-square statistic) over the corner the splits reach; cells past it
read -1 as everywhere outside a caller's table.  Its values do not change the work: every permutation draws the same
number of patients whatever it scores.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GCRE_QUIET", "1")
import numpy as np  # noqa: E402

N_CASES, N_CTRLS, PERMS = 25000, 25000, 100000


def make_case(seed: int = 20261016, n_cases: int = N_CASES, n_ctrls: int = N_CTRLS, per_length: int = 10):
    """(data, paths, signs): per_length random paths of each length 2..5 over their own genes, mixed signs."""
    rng = np.random.default_rng(seed)
    n = n_cases + n_ctrls
    paths, signs, rows = [], [], []
    for L in range(2, 6):
        for _ in range(per_length):
            paths.append(list(range(len(rows), len(rows) + L)))
            signs.append(rng.choice([-1, 1], size=L).tolist())
            for _g in range(L):
                rows.append(rng.random(n) < rng.uniform(0.005, 0.05))
    return np.array(rows, dtype=np.uint8), paths, signs


def corner_table(n_cases: int, n_ctrls: int, m: int) -> np.ndarray:
    """table[i][j], i, j <= m: half the chi-square statistic of the 2 x 2 split (i cases, j controls carry)."""
    n = float(n_cases + n_ctrls)
    i = np.arange(m + 1, dtype=np.float64)[:, None]
    j = np.arange(m + 1, dtype=np.float64)[None, :]
    tot = i + j
    den = np.maximum(tot * (n - tot), 1.0) * (2.0 * n_cases * n_ctrls / n)
    return (i * n_ctrls - j * n_cases) ** 2 * n / den


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--perms", type=int, default=PERMS)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--corner", type=int, default=6000)
    a = ap.parse_args()
    from geneticscre_amd import api

    data, paths, signs = make_case()
    t0 = time.perf_counter()
    ex = api.JoinExec(2, N_CASES, N_CTRLS, a.perms)
    ex.set_value_table(corner_table(N_CASES, N_CTRLS, a.corner))
    print(f"context + table: {(time.perf_counter() - t0) * 1e3:.0f} ms", flush=True)
    rec = ex.decorated_pvalues(paths, data, signs, seed=1)            # warm-up: code objects, allocations
    draws = int((rec["k_pos"] + rec["k_neg"]).sum())
    times = []
    for r in range(a.reps):
        t0 = time.perf_counter()
        rec2 = ex.decorated_pvalues(paths, data, signs, seed=1)
        times.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(rec2["n_ge"], rec["n_ge"])
    ex.close()
    ms = min(times)
    print(json.dumps({"tool": "decorated_time", "n_cases": N_CASES, "n_ctrls": N_CTRLS, "perms": a.perms,
                      "splits": len(rec), "draws_per_perm": draws, "k_min": int((rec["k_pos"] + rec["k_neg"]).min()),
                      "k_max": int((rec["k_pos"] + rec["k_neg"]).max()), "call_ms": [round(t, 2) for t in times],
                      "best_ms": round(ms, 2), "urn_draws_per_s_upper": draws * a.perms / (ms * 1e-3),
                      "pvalue_min": float(np.nanmin(rec["pvalue"])), "pvalue_max": float(np.nanmax(rec["pvalue"]))}),
          flush=True)


if __name__ == "__main__":
    main()
