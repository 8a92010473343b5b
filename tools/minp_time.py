"""Time of min-P over caller-given sets (gcre_score_sets_minp: k_minp_gather, k_family_null, k_minp_rank, k_minp_scan;
DESIGN.md §3.16) beside gcre_score_sets_family on the same sets and beside the bytes bound of one read and one write of the
null matrix.

    python tools/minp_time.py [--what call] [--sets 1000,10000] [--runs N]

The geometry is tools/family_time.py's: one-gene sets on random rows (0.5 % to 5 % carriers) at 25,000 + 25,000 patients and
100,000 generated permutations, method 1.
  call     N calls after a warm-up: wall time of JoinExec.family_tests() and of JoinExec.minp_tests(), the launches of the
           latter, and the bytes bound of one read and one write of N (sets x permutations x 8 bytes at 6.3 TB/s)
  kernel   a 16-set warm-up and one call of minp_tests, for a run of its own under rocprofv3 --kernel-trace --stats
  fuzz     tests/test_gpu_minp.fuzz_case for --cases cases against the reference: one summary line
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

from family_time import HBM_BYTES_PER_S, N_CASES, N_CTRLS, PERMS, problem  # noqa: E402


def shape(n_sets: int, perms: int) -> dict:
    stride = -(-perms // 512) * 512
    mb = float(os.environ.get("GCRE_MINP_MAX_MB", "1024"))
    slab = max(1, min(n_sets, int(mb * 1048576 / (stride * 8))))
    nbytes = n_sets * perms * 8
    return {"tool": "minp_time", "sets": n_sets, "n_cases": N_CASES, "n_ctrls": N_CTRLS, "perms": perms, "read_write_bytes": nbytes,
            "slab_rows": slab, "slabs": -(-n_sets // slab), "read_write_bound_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 1)}


def call(n_sets: int, runs: int, perms: int) -> None:
    ex, sets, genes = problem(n_sets, perms)
    ex.family_tests(sets[:16], genes)                            # warm-up: code objects
    ex.minp_tests(sets[:16], genes)
    fam, mnp = [], []
    before = ex.minp_launches()
    for _ in range(runs):
        t0 = time.perf_counter()
        rec, f = ex.family_tests(sets, genes)
        fam.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        rec2, mp, mc = ex.minp_tests(sets, genes, min_count=True)
        mnp.append((time.perf_counter() - t0) * 1e3)
    launches = (ex.minp_launches() - before) // runs
    ex.close()
    assert rec.tobytes() == rec2.tobytes()
    c = rec["n_ge"]
    assert (c <= mp["n_le_stepdown"]).all() and (mp["n_le_stepdown"] <= mp["n_le_minp"]).all()
    assert (mp["n_le_minp"] == np.searchsorted(np.sort(mc), c.astype(np.uint32), side="right")).all()
    low = c == c.min()
    assert (mp["n_le_stepdown"][low] == mp["n_le_minp"][low]).all()
    line = shape(n_sets, perms)
    line.update({"what": "call", "family_tests_ms": [round(t, 2) for t in fam], "family_tests_median_ms": round(float(np.median(fam)), 2),
                 "minp_tests_ms": [round(t, 2) for t in mnp], "minp_tests_median_ms": round(float(np.median(mnp)), 2),
                 "minp_launches_per_call": launches, "min_count_min": int(mc.min()), "min_count_median": int(np.median(mc)),
                 "minp_over_nominal_max": int((mp["n_le_minp"] - c).max()),
                 "minp_minus_stepdown_max": int((mp["n_le_minp"] - mp["n_le_stepdown"]).max())})
    print(json.dumps(line), flush=True)


def kernel(n_sets: int, perms: int) -> None:
    ex, sets, genes = problem(n_sets, perms)
    ex.minp_tests(sets[:16], genes)
    ex.minp_tests(sets, genes)       # (k_family_null below is this stage's own: the family entry is not called)
    ex.close()
    line = shape(n_sets, perms)
    line["what"] = "kernel"
    print(json.dumps(line), flush=True)


def fuzz(cases: int) -> None:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_minp as T
    t0 = time.perf_counter()
    seen = {"method": set(), "slab": set(), "K": set(), "V": set(), "n": set()}
    os.environ.pop("GCRE_MINP_MAX_MB", None)
    for case in range(cases):
        method, nc, nt, K, sets, rows, signs, VT, slab, what = T.fuzz_case(case)
        os.environ.pop("GCRE_MINP_SLAB_SETS", None)
        if slab:
            os.environ["GCRE_MINP_SLAB_SETS"] = str(slab)
        ex = T.open_context(method, nc, nt, K, VT, 500 + case)
        try:
            T.check_context(ex, sets, rows, signs, what)
        finally:
            ex.close()
        for k, v in (("method", method), ("slab", slab), ("K", K), ("V", len(sets) - 1), ("n", nc + nt)):
            seen[k].add(v)
    os.environ.pop("GCRE_MINP_SLAB_SETS", None)
    print(json.dumps({"tool": "minp_time", "what": "fuzz", "cases": cases, "failures": 0, "seconds": round(time.perf_counter() - t0, 1),
                      **{k: sorted(v) for k, v in seen.items()}}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="call")
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
        elif what == "fuzz":
            fuzz(a.cases)
        else:
            raise SystemExit(f"unknown item {what!r}")


if __name__ == "__main__":
    main()
