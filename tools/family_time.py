"""Time of the family-wise inference over caller-given sets (gcre_score_sets_family: k_family_null, k_family_scan,
k_family_hist) beside gcre_score_sets (k_set_null) on the same sets and beside the bytes bound of the two
streaming kernels.

    python tools/family_time.py [--what call,paths] [--sets 1000,10000] [--runs N]

One-gene sets on random rows (0.5 % to 5 % carriers) at 25,000 + 25,000 patients and 100,000 generated permutations, method 1;
the value table is tools/decorated_time.py's stand-in, the work does not depend on its values.
  call     N calls after a warm-up: wall time of JoinExec.score_sets(family=True) and of JoinExec.family_tests(kmax=True),
           the launches of the latter, and the bytes bound of one pass over the null matrix (sets x permutations x 4 bytes
           at 6.3 TB/s)
  kernel   one warm-up and one call of each, for a run of its own under rocprofv3 --kernel-trace --stats
  paths    report.score_paths with and without family_inference on 1,000 gene sets at 2,500 + 2,500 patients (its value table
           is the full one, which a 50,000-patient cohort does not hold in memory)
  fuzz     tests/test_gpu_family.fuzz_case for --cases cases against the reference: one summary line
One JSON line per item."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GCRE_QUIET", "1")
import numpy as np  # noqa: E402

PERMS = 100_000
N_CASES = N_CTRLS = 25_000
HBM_BYTES_PER_S = 6.3e12      # what a float4 copy reaches on one MI355X


def problem(n_sets: int, perms: int):
    from geneticscre_amd import api
    from decorated_time import corner_table
    rng = np.random.default_rng(15)
    n = N_CASES + N_CTRLS
    genes = np.empty((n_sets, n), dtype=np.int8)
    for lo in range(0, n_sets, 500):
        hi = min(lo + 500, n_sets)
        genes[lo:hi] = rng.random((hi - lo, n), dtype=np.float32) < rng.uniform(0.005, 0.05, size=(hi - lo, 1)).astype(np.float32)
    ex = api.JoinExec(1, N_CASES, N_CTRLS, perms)
    ex.set_value_table(corner_table(N_CASES, N_CTRLS, 6000))
    ex.generate_permutations(1)
    return ex, [[s] for s in range(n_sets)], genes


def shape(n_sets: int, perms: int) -> dict:
    nbytes = n_sets * perms * 4
    slab = max(1, min(-(-perms // 512), (1024 << 20) // (n_sets * 512 * 4)))
    return {"tool": "family_time", "sets": n_sets, "n_cases": N_CASES, "n_ctrls": N_CTRLS, "perms": perms, "null_matrix_bytes": nbytes,
            "slabs": -(-(-(-perms // 512)) // slab), "one_pass_bound_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 1)}


def call(n_sets: int, runs: int, perms: int) -> None:
    ex, sets, genes = problem(n_sets, perms)
    ex.family_tests(sets[:16], genes, kmax=True)                 # warm-up: code objects
    ex.score_sets(sets[:16], genes, family=True)
    plain, fam = [], []
    before = ex.family_launches()
    for _ in range(runs):
        t0 = time.perf_counter()
        rec, fmax = ex.score_sets(sets, genes, family=True)
        plain.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        rec2, f, km = ex.family_tests(sets, genes, kmax=True)
        fam.append((time.perf_counter() - t0) * 1e3)
    launches = (ex.family_launches() - before) // runs
    ex.close()
    assert rec.tobytes() == rec2.tobytes() and np.array_equal(km[0].view(np.uint32), fmax.view(np.uint32))
    best = int(np.argmax(rec["score"]))
    assert f["n_ge_stepdown"][best] == int((km[0].astype(np.float64) >= rec["score"][best]).sum())
    assert (f["n_ge_stepdown"] >= rec["n_ge"]).all()
    line = shape(n_sets, perms)
    line.update({"what": "call", "score_sets_ms": [round(t, 2) for t in plain], "score_sets_median_ms": round(float(np.median(plain)), 2),
                 "family_tests_ms": [round(t, 2) for t in fam], "family_tests_median_ms": round(float(np.median(fam)), 2),
                 "family_launches_per_call": launches, "exceed_max": int(f["exceed"].max()),
                 "stepdown_over_nominal_max": int((f["n_ge_stepdown"] - rec["n_ge"]).max())})
    print(json.dumps(line), flush=True)


def kernel(n_sets: int, perms: int) -> None:
    ex, sets, genes = problem(n_sets, perms)
    ex.family_tests(sets[:16], genes, kmax=True)
    ex.score_sets(sets[:16], genes, family=True)
    ex.score_sets(sets, genes, family=True)
    ex.family_tests(sets, genes, kmax=True)
    ex.close()
    line = shape(n_sets, perms)
    line["what"] = "kernel"
    print(json.dumps(line), flush=True)


def paths(runs: int, perms: int, n_paths: int = 1000, nc: int = 2500, nt: int = 2500) -> None:
    from geneticscre_amd import report
    rng = np.random.default_rng(16)
    G = 2000
    genes = [f"G{i}" for i in range(G)]
    data = (rng.random((G, nc + nt)) < 0.02).astype(np.int32)
    named = [[genes[g] for g in rng.choice(G, size=int(rng.integers(2, 30)), replace=False)] for _ in range(n_paths)]
    kw = dict(threshold=0.05, n_permutations=perms, seed=3)
    report.score_paths(named[:8], genes, data, nc, nt, family_inference=True, **kw)      # warm-up
    plain, fam = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        a = report.score_paths(named, genes, data, nc, nt, **kw)
        plain.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        b = report.score_paths(named, genes, data, nc, nt, family_inference=True, **kw)
        fam.append((time.perf_counter() - t0) * 1e3)
    assert a.equals(b[report.SCORE_PATHS_COLUMNS])
    print(json.dumps({"tool": "family_time", "what": "paths", "paths": n_paths, "n_cases": nc, "n_ctrls": nt, "perms": perms,
                      "score_paths_ms": [round(t, 1) for t in plain], "score_paths_median_ms": round(float(np.median(plain)), 1),
                      "family_inference_ms": [round(t, 1) for t in fam], "family_inference_median_ms": round(float(np.median(fam)), 1),
                      "q_below_0.05": int((b["FamilyQvalues"] < 0.05).sum()),
                      "stepdown_below_0.05": int((b["FamilyPvaluesStepDown"] < 0.05).sum())}), flush=True)


def fuzz(cases: int) -> None:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_family as T
    t0 = time.perf_counter()
    seen = {"method": set(), "slab": set(), "K": set(), "V": set(), "n": set()}
    for case in range(cases):
        method, nc, nt, K, sets, rows, signs, VT, slab, what = T.fuzz_case(case)
        os.environ.pop("GCRE_FAMILY_SLAB_PERMS", None)
        if slab:
            os.environ["GCRE_FAMILY_SLAB_PERMS"] = str(slab)
        ex = T.open_context(method, nc, nt, K, VT, 300 + case)
        try:
            T.check_context(ex, method, nc, nt, K, sets, rows, signs, VT, what)
        finally:
            ex.close()
        for k, v in (("method", method), ("slab", slab), ("K", K), ("V", len(sets) - 1), ("n", nc + nt)):
            seen[k].add(v)
    os.environ.pop("GCRE_FAMILY_SLAB_PERMS", None)
    print(json.dumps({"tool": "family_time", "what": "fuzz", "cases": cases, "failures": 0, "seconds": round(time.perf_counter() - t0, 1),
                      **{k: sorted(v) for k, v in seen.items()}}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="call,paths")
    ap.add_argument("--sets", default="1000,10000")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--perms", type=int, default=PERMS)
    ap.add_argument("--cases", type=int, default=300)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sets.split(",") if s]
    for what in [w for w in a.what.split(",") if w]:
        if what == "call":
            for s in sizes:
                call(s, a.runs, a.perms)
        elif what == "kernel":
            for s in sizes:
                kernel(s, a.perms)
        elif what == "paths":
            paths(a.runs, a.perms)
        elif what == "fuzz":
            fuzz(a.cases)
        else:
            raise SystemExit(f"unknown item {what!r}")


if __name__ == "__main__":
    main()
