"""Time of the burden tests of per-patient weights (gcre_patient_burden: k_burden_planes, k_burden_null, k_burden_finish;
DESIGN.md §3.14) beside its instruction-issue estimate and beside k_set_null on as many plain sets as there are planes.

    python tools/burden_time.py [--what call,reference] [--geometry large,table] [--runs N]

Weights are uniform below 2^planes (the time does not depend on their values), at two geometries, 100,000 permutations each:
  large   100 rows of 20 planes at 25,000 + 25,000 patients (the tallies of 10^6 sets in 100 groups)
  table   10 rows of 10 planes at 2,500 + 2,500 patients
  call       N calls after a warm-up: wall time of JoinExec.patient_burden without and with the null sums, and of the C
             entry from the library's own line (GCRE_BURDEN_STATS), beside the estimate the tool computes from the shape
  kernel     one warm-up and one call, for a run of its own under rocprofv3 --kernel-trace --stats (the trace gives the times)
  sets       JoinExec.score_sets (k_set_null) on rows x planes one-gene sets at the same shape, method 1, likewise for a
             traced run; the value table is tools/decorated_time.py's stand-in, the work does not depend on its values
  reference  report.burden_reference on a slice of the permutations, scaled to all of them (and said so)
One JSON line per item."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["GCRE_BURDEN_STATS"] = "1"
os.environ.setdefault("GCRE_QUIET", "1")
from clump_time import Stderr  # noqa: E402
import numpy as np  # noqa: E402

PERMS = 100_000
GEOMETRY = {"large": (100, 20, 25_000, 25_000), "table": (10, 10, 2_500, 2_500)}   # rows, planes, cases, controls
# MI355X: 256 CUs x 4 SIMDs, one wave64 vector instruction per 2 cycles per SIMD, 2.4 GHz (DESIGN.md §3.6's rate)
SIMDS, CYC_PER_VALU, CLOCK_HZ = 1024, 2, 2.4e9


def estimate(rows: int, planes: int, n: int, perms: int) -> dict:
    """What k_burden_null has to issue, from the shape alone: 2 vector instructions (AND, popcount-add) per (plane, 64
    permutations, mask dword); the atomics it ends an item with: one per (item of four planes, permutation)."""
    w32p = 2 * (((n + 63) // 64 + 3) // 4 * 4)
    instr = rows * planes * -(-perms // 64) * w32p * 2
    return {"mask_dwords": w32p, "valu_instructions": instr,
            "issue_estimate_us": round(instr * CYC_PER_VALU / (SIMDS * CLOCK_HZ) * 1e6, 1),
            "sum_atomics": rows * -(-planes // 4) * perms, "mask_bytes": w32p * 4 * (-(-perms // 2048) * 2048)}


def problem(name: str, perms: int):
    from geneticscre_amd import api
    rows, planes, nc, nt = GEOMETRY[name]
    rng = np.random.default_rng(11)
    w = rng.integers(0, 2**planes, (rows, nc + nt), dtype=np.int64).astype(np.int32)
    w[:, 0] = 2**planes - 1
    ex = api.JoinExec(1, nc, nt, perms)
    ex.generate_permutations(1)
    return ex, w, rows, planes, nc, nt


def stats_of(text: str):
    return [{k: float(v) if "." in v else int(v) for k, v in (kv.split("=") for kv in ln.split()[1:])}
            for ln in text.splitlines() if ln.startswith("burden rows=")]


def call(name: str, runs: int, perms: int) -> None:
    ex, w, rows, planes, nc, nt = problem(name, perms)
    ex.patient_burden(w[:1])                                    # warm-up: code objects
    wall, wall_null, lib = [], [], []
    for _ in range(runs):
        with Stderr() as err:
            t0 = time.perf_counter()
            res = ex.patient_burden(w)
            wall.append((time.perf_counter() - t0) * 1e3)
        lib.append(stats_of(err.text)[-1])
        t0 = time.perf_counter()
        full = ex.patient_burden(w, null=True)
        wall_null.append((time.perf_counter() - t0) * 1e3)
    launches = ex.burden_launches
    ex.close()
    assert res["planes"].tolist() == [planes] * rows and np.array_equal(res["n_ge"], full["n_ge"])
    assert np.array_equal((full["null"] >= full["observed"][:, None]).sum(axis=1), res["n_ge"])
    line = {"tool": "burden_time", "what": "call", "geometry": name, "rows": rows, "planes": planes, "n_cases": nc, "n_ctrls": nt,
            "perms": perms, "python_call_ms": [round(t, 2) for t in wall], "python_call_median_ms": round(float(np.median(wall)), 2),
            "python_call_with_null_median_ms": round(float(np.median(wall_null)), 2),
            "entry_median_ms": round(float(np.median([x["entry_ms"] for x in lib])), 3), "items": lib[-1]["items"],
            "slabs": lib[-1]["slabs"], "launches": launches, "p_upper_min": float(res["p_upper"].min()),
            "p_upper_max": float(res["p_upper"].max())}
    line.update(estimate(rows, planes, nc + nt, perms))
    print(json.dumps(line), flush=True)


def kernel(name: str, perms: int) -> None:
    ex, w, rows, planes, nc, nt = problem(name, perms)
    ex.patient_burden(w[:1])
    ex.patient_burden(w)
    ex.close()
    line = {"tool": "burden_time", "what": "kernel", "geometry": name, "rows": rows, "planes": planes, "n_cases": nc, "n_ctrls": nt,
            "perms": perms}
    line.update(estimate(rows, planes, nc + nt, perms))
    print(json.dumps(line), flush=True)


def sets(name: str, perms: int, corner: int = 6000) -> None:
    from geneticscre_amd import api
    from decorated_time import corner_table
    rows, planes, nc, nt = GEOMETRY[name]
    S = rows * planes
    rng = np.random.default_rng(12)
    genes = rng.random((S, nc + nt), dtype=np.float32) < rng.uniform(0.005, 0.05, size=(S, 1)).astype(np.float32)
    one_gene = [[s] for s in range(S)]
    ex = api.JoinExec(1, nc, nt, perms)
    ex.set_value_table(corner_table(nc, nt, min(corner, nc, nt)))
    ex.generate_permutations(1)
    ex.score_sets(one_gene[:16], genes)                          # warm-up
    t0 = time.perf_counter()
    rec = ex.score_sets(one_gene, genes)
    ms = (time.perf_counter() - t0) * 1e3
    ex.close()
    line = {"tool": "burden_time", "what": "sets", "geometry": name, "sets": len(rec), "n_cases": nc, "n_ctrls": nt, "perms": perms,
            "score_sets_call_ms": round(ms, 2)}
    line.update(estimate(rows, planes, nc + nt, perms))
    print(json.dumps(line), flush=True)


def reference(name: str, perms: int, slice_perms: int = 200) -> None:
    from geneticscre_amd import report
    ex, w, rows, planes, nc, nt = problem(name, slice_perms)
    masks = np.stack([ex.perm_mask(r) for r in range(slice_perms)])
    ex.close()
    t0 = time.perf_counter()
    report.burden_reference(w, masks, nc)
    ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"tool": "burden_time", "what": "reference", "geometry": name, "rows": rows, "slice_perms": slice_perms,
                      "slice_ms": round(ms, 1), "perms": perms, "scaled_to_all_perms_ms": round(ms * perms / slice_perms, 1),
                      "scaled": "linear in the permutations, from the slice; the masks are already unpacked words read back"}),
          flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="call,reference")
    ap.add_argument("--geometry", default="large,table")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--perms", type=int, default=PERMS)
    a = ap.parse_args()
    for what in [w for w in a.what.split(",") if w]:
        for name in [g for g in a.geometry.split(",") if g]:
            if what == "call":
                call(name, a.runs, a.perms)
            elif what == "kernel":
                kernel(name, a.perms)
            elif what == "sets":
                sets(name, a.perms)
            elif what == "reference":
                reference(name, a.perms)
            else:
                raise SystemExit(f"unknown item {what!r}")


if __name__ == "__main__":
    main()
