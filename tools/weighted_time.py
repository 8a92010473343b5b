"""Time of the covariate-adjusted permutation masks (gcre_generate_weighted_masks: k_weighted_search, k_weighted_write;
DESIGN.md §3.23) beside k_generate_masks and k_subsample_masks in the same run.

    python tools/weighted_time.py                      every geometry: writes profiles/weighted_time.txt and
                                                       profiles/weighted_kernel_stats.csv
    python tools/weighted_time.py --what call ...      one item in this process (what the driver starts as children)

Geometries: configs[2] of the benchmark (2,500 + 2,500 patients, 10,000 permutations) and 25,000 + 25,000 patients with
100,000 permutations; one stratum and four (patient q is of stratum q mod 4); equal odds and the odds ``report.case_odds`` fits
on two synthetic Gaussian covariates.  Per geometry the driver starts two children, each under a time limit of its own, and
stops at the first that fails:
  call     a warm-up and N calls of generate_weighted_permutations(attempts=True): the wall time of the whole call, the mean and
           the maximum accepted attempt against sqrt(2 pi V), and the hashes k_weighted_search evaluated -- per (r, s) the
           batches of eight attempts it ran, four hashes a patient each
  kernel   one call of each of generate_weighted_permutations, generate_permutations and subsample_tests (as many draws as
           permutations: one hash per patient and draw in k_subsample_masks) under rocprofv3 --kernel-trace --stats
One JSON line per item; the driver adds a "summary" line per geometry: k_weighted_write against k_generate_masks, and
k_weighted_search against its hashes at k_subsample_masks' hash rate of the same run."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GCRE_QUIET", "1")
import numpy as np  # noqa: E402

from geneticscre_amd import api, report  # noqa: E402

SEED = 5
GEOMETRIES = [(2500, 2500, 10000), (25000, 25000, 100000)]
BATCH = 8          # kWeightedBatch
KERNELS = ("k_weighted_search", "k_weighted_write", "k_generate_masks", "k_subsample_masks")


def inputs(nc: int, nt: int, S: int, odds_kind: str):
    n = nc + nt
    rng = np.random.default_rng(41)
    strata = None if S == 1 else (np.arange(n) % S).astype(np.int32)
    if odds_kind == "equal":
        return np.ones(n), strata
    cov = rng.normal(size=(n, 2)) + np.where(np.arange(n) < nc, 0.4, 0.0)[:, None] * np.array([1.0, -0.5])
    return report.case_odds(cov, nc, nt), strata


def shape(nc, nt, K, S, odds_kind) -> dict:
    return {"tool": "weighted_time", "n_cases": nc, "n_ctrls": nt, "perms": K, "strata": S, "odds": odds_kind}


def call(nc, nt, K, S, odds_kind, runs) -> None:
    odds, strata = inputs(nc, nt, S, odds_kind)
    t0 = time.perf_counter()
    thr, exp = api.weighted_thresholds(odds, nc, nt, strata)
    host_ms = (time.perf_counter() - t0) * 1e3
    ex = api.JoinExec(1, nc, nt, K)
    ex.generate_weighted_permutations(SEED, odds, strata)                  # warm-up: code objects
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        att = ex.generate_weighted_permutations(SEED, odds, strata, attempts=True)
        ms.append((time.perf_counter() - t0) * 1e3)
    launches = ex.weighted_launches()
    ex.close()
    sizes = np.array([nc + nt]) if strata is None else np.bincount(strata, minlength=S)
    batches = att.astype(np.int64) // BATCH + 1
    line = shape(nc, nt, K, S, odds_kind)
    line.update({"what": "call", "thresholds_host_ms": round(host_ms, 2), "call_ms": [round(t, 2) for t in ms],
                 "call_median_ms": round(float(np.median(ms)), 2), "launches": launches,
                 "expected_attempts": [round(float(e), 1) for e in exp],
                 "mean_accepted_attempt": [round(float(a), 1) for a in att.mean(axis=0)],
                 "max_accepted_attempt": [int(a) for a in att.max(axis=0)],
                 "search_hashes": int((batches * sizes[None, :]).sum() * (BATCH // 2)),
                 "odds_range": [float(odds.min()), float(odds.max())]})
    print(json.dumps(line), flush=True)


def kernel(nc, nt, K, S, odds_kind) -> None:
    odds, strata = inputs(nc, nt, S, odds_kind)
    ex = api.JoinExec(1, nc, nt, K)
    ex.set_value_table(np.ones((2, 2)))
    ex.generate_weighted_permutations(SEED, odds, strata)
    ex.generate_permutations(SEED, strata)
    rows = np.zeros((1, nc + nt), np.int8)
    rows[0, ::3] = 1
    ex.subsample_tests([[0]], rows, draws=K, seed=SEED, table_a=np.ones((2, 2)), table_b=np.ones((2, 2)))
    ex.close()
    line = shape(nc, nt, K, S, odds_kind)
    line.update({"what": "kernel", "subsample_hashes": K * (nc + nt)})
    print(json.dumps(line), flush=True)


def child(args, limit, log):
    """One step under its own time limit; its JSON lines, or None when it failed (the driver then stops)."""
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + args, capture_output=True, text=True, cwd=ROOT)
    log.write(r.stdout)
    log.flush()
    if r.returncode != 0:
        log.write(f"# step failed with exit status {r.returncode}: {' '.join(args)}\n{r.stderr[-2000:]}\n")
        return None
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def stats_of(d):
    """{kernel: (calls, total ns)} from the kernel stats of a rocprofv3 run, and the csv's path."""
    f = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
    out = {}
    for row in csv.DictReader(open(f)):
        for k in KERNELS:
            if k in row["Name"]:
                out[k] = (int(row["Calls"]), int(float(row["TotalDurationNs"])))
    return out, f


def drive(runs: int, only_small: bool) -> int:
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    csv_out = os.path.join(ROOT, "profiles", "weighted_kernel_stats.csv")
    first = True
    with open(os.path.join(ROOT, "profiles", "weighted_time.txt"), "w") as log:
        for nc, nt, K in GEOMETRIES[:1] if only_small else GEOMETRIES:
            for S in (1, 4):
                for kind in ("equal", "fitted"):
                    geo = ["--n-cases", str(nc), "--n-ctrls", str(nt), "--perms", str(K), "--strata", str(S), "--odds", kind]
                    limit = 120 if K <= 10000 else 240
                    c = child(me + ["--what", "call", "--runs", str(runs)] + geo, limit, log)
                    if c is None:
                        return 1
                    d = tempfile.mkdtemp(prefix="weighted_kt_")
                    k = child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"] + me +
                              ["--what", "kernel"] + geo, limit, log)
                    if k is None:
                        return 1
                    st, f = stats_of(d)
                    with open(csv_out, "w" if first else "a") as out:
                        out.write(f"# {nc}+{nt} patients, {K} permutations, {S} strata, {kind} odds\n" + open(f).read())
                    first = False
                    shutil.rmtree(d, ignore_errors=True)
                    ms = {name: st[name][1] / 1e6 for name in st}
                    rate = k[0]["subsample_hashes"] / (ms["k_subsample_masks"] / 1e3)
                    line = shape(nc, nt, K, S, kind)
                    line.update({"what": "summary", "kernel_ms": {n: round(v, 3) for n, v in ms.items()},
                                 "write_over_generate": round(ms["k_weighted_write"] / ms["k_generate_masks"], 2),
                                 "subsample_hashes_per_s": float(f"{rate:.4g}"),
                                 "search_ms_at_that_rate": round(c[0]["search_hashes"] / rate * 1e3, 3),
                                 "search_over_that": round(ms["k_weighted_search"] / (c[0]["search_hashes"] / rate * 1e3), 2)})
                    log.write(json.dumps(line) + "\n")
                    log.flush()
                    print(json.dumps(line), flush=True)
    return 0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="all")
    ap.add_argument("--n-cases", type=int, default=2500)
    ap.add_argument("--n-ctrls", type=int, default=2500)
    ap.add_argument("--perms", type=int, default=10000)
    ap.add_argument("--strata", type=int, default=1)
    ap.add_argument("--odds", default="equal")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="all: the first geometry alone")
    a = ap.parse_args()
    if a.what == "all":
        raise SystemExit(drive(a.runs, a.small))
    if a.what == "call":
        call(a.n_cases, a.n_ctrls, a.perms, a.strata, a.odds, a.runs)
    elif a.what == "kernel":
        kernel(a.n_cases, a.n_ctrls, a.perms, a.strata, a.odds)
    else:
        raise SystemExit(f"unknown item {a.what!r}")


if __name__ == "__main__":
    main()
