"""Wall time of gcre_score_sets at configs[4] geometry (bench.py "signed": 25,000 cases, 25,000 controls, 100,000
permutations), both methods: 1,000 random length-5 paths over genes carried by 0.5-5 % of the patients and 100 gene sets
of 200 such genes, in one call with the family maximum.  The call ends in a stream synchronise, so a host clock around it
times the device work and the host stage (packing the union rows); rocprofv3 --kernel-trace --stats gives k_set_null on
its own.

    python tools/sets_time.py [--perms K] [--reps R] [--methods 1,2]

The estimate it prints is the issue count of the dense form: 2 VALU (AND, popcount-add) per (set, 64 permutations, mask
dword, half), at 2 cycles per wave64 instruction on each of 1,024 SIMDs at 2.4 GHz.  The value table is
tools/decorated_time.py's cheap stand-in over the corner the paths reach; the work does not depend on its values.
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
N_PATHS, PATH_LEN, N_GENESETS, GENESET_SIZE, POOL = 1000, 5, 100, 200, 2000


def make_case(seed: int = 20261016):
    """(rows, sets, signs): a pool of genes at 0.5-5 % carriers, 1,000 paths of 5 of them, 100 gene sets of 200."""
    rng = np.random.default_rng(seed)
    n = N_CASES + N_CTRLS
    rows = rng.random((POOL, n), dtype=np.float32) < rng.uniform(0.005, 0.05, size=(POOL, 1)).astype(np.float32)
    sets, signs = [], []
    for _ in range(N_PATHS):
        sets.append(rng.choice(POOL, size=PATH_LEN, replace=False).tolist())
        signs.append(rng.choice([-1, 1], size=PATH_LEN).tolist())
    for _ in range(N_GENESETS):
        sets.append(rng.choice(POOL, size=GENESET_SIZE, replace=False).tolist())
        signs.append(rng.choice([-1, 1], size=GENESET_SIZE).tolist())
    return rows, sets, signs


def estimate_ms(n_sets: int, perms: int, method: int) -> float:
    w32p = 2 * (((N_CASES + N_CTRLS + 63) // 64 + 3) // 4 * 4)
    instr = n_sets * -(-perms // 64) * w32p * 2 * method
    return instr * 2 / (1024 * 2.4e9) * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--perms", type=int, default=PERMS)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--corner", type=int, default=6000)
    ap.add_argument("--methods", default="1,2")
    a = ap.parse_args()
    from geneticscre_amd import api
    from decorated_time import corner_table

    rows, sets, signs = make_case()
    table = corner_table(N_CASES, N_CTRLS, a.corner)
    for method in [int(m) for m in a.methods.split(",")]:
        t0 = time.perf_counter()
        ex = api.JoinExec(method, N_CASES, N_CTRLS, a.perms)
        ex.set_value_table(table)
        ex.generate_permutations(1)
        print(f"method {method}: context + table + masks: {(time.perf_counter() - t0) * 1e3:.0f} ms", flush=True)
        rec, fam = ex.score_sets(sets, rows, signs, family=True)            # warm-up: code objects, allocations
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            rec2, fam2 = ex.score_sets(sets, rows, signs, family=True)
            times.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(rec2["n_ge"], rec["n_ge"]) and np.array_equal(fam2, fam)
        ex.close()
        carriers = (rec["cases"] + rec["ctrls"]) / float(N_CASES + N_CTRLS)
        print(json.dumps({"tool": "sets_time", "method": method, "n_cases": N_CASES, "n_ctrls": N_CTRLS,
                          "perms": a.perms, "sets": len(rec), "paths": N_PATHS, "gene_sets": N_GENESETS,
                          "path_carrier_frac_max": round(float(carriers[:N_PATHS].max()), 4),
                          "geneset_carrier_frac_mean": round(float(carriers[N_PATHS:].mean()), 4),
                          "call_ms": [round(t, 2) for t in times], "best_ms": round(min(times), 2),
                          "estimate_valu_ms": round(estimate_ms(len(rec), a.perms, method), 2),
                          "pvalue_min": float(np.nanmin(rec["pvalue"])), "family_max_mean": float(fam.mean())}),
              flush=True)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
