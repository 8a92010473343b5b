"""What the per-gene best-path tally (gcre_gene_tally) costs a pass at BASELINE configs[2] geometry
(bench.py "roofline": 17,000 genes, 200,000 relations, 5,000 patients, 10,000 permutations, path length 4): resident
passes of ResidentPlan with a tally armed on every level and without, interleaved, after warm-up; median and spread of
both.  A pass ends in a stream synchronise (the tallies' reads included), so a host clock around it times the device work.

    python tools/gene_best_time.py [--passes N] [--warmup W] [--config roofline] [--only armed|unarmed]

The byte bound it prints is 16 B per joined path (key 8, row0 4, row1 4): the compulsory traffic of k_gene_fold.  The
kernels' own time comes from a run of its own under rocprofv3 --kernel-trace --stats (`--only armed`), summed over
k_gene_fold, k_gene_index and k_gene_merge; the level's null kernel time is gcre_profile.null_kernel_ms.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GCRE_QUIET", "1")
import numpy as np  # noqa: E402


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "iqr_ms": round(float(np.subtract(*np.percentile(ms, [75, 25]))), 3), "n": len(ms)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="roofline")
    ap.add_argument("--only", default="", choices=["", "armed", "unarmed"])
    a = ap.parse_args()
    import bench
    from geneticscre_amd import api, report

    cfg = dict(bench.CONFIGS[a.config])
    prob, masks = bench.build_inputs(cfg, 20261003, 100)
    plan = api.ResidentPlan(prob, packed_masks=masks, mask_seed=None if masks is not None else 1)
    n_genes, n_genes2 = len(prob.data1), len(prob.data2)
    tables = report.gene_tables(prob.levels, n_genes, n_genes2)
    names = report.GENE_LEVELS[:prob.path_length]
    paths = {k: int(prob.levels.n_paths[k]) for k in names}

    def one(armed: bool):
        # (tallies are made outside the timed region: their tables are uploaded once per network in a real run)
        tallies = {k: api.GeneTally(plan.ex, report.gene_slots(k, n_genes, n_genes2), *tables[k]) for k in names} if armed else None
        t0 = time.perf_counter()
        plan.run(tallies=tallies)
        best = {k: t.read() for k, t in tallies.items()} if armed else None
        ms = (time.perf_counter() - t0) * 1e3
        prof = dict(plan.last_profile)
        for t in (tallies or {}).values():
            t.free()
        return ms, prof, best

    kinds = [a.only == "armed"] if a.only else [False, True]
    for _ in range(a.warmup):
        for armed in kinds:
            one(armed)
    times = {True: [], False: []}
    null_ms = {True: [], False: []}
    best = None
    for _ in range(a.passes):
        for armed in kinds:                     # interleaved: both see the same machine
            ms, prof, b = one(armed)
            times[armed].append(ms)
            null_ms[armed].append(prof["null_kernel_ms"])
            best = b or best
    total_paths = sum(paths.values())
    out = {"config": a.config, "joined_paths": paths, "byte_bound_bytes": 16 * total_paths,
           "byte_bound_ms_at_4.5TBs": round(16 * total_paths / 4.5e12 * 1e3, 4)}
    for armed in kinds:
        key = "armed" if armed else "unarmed"
        out[key] = spread(times[armed])
        out[key]["null_kernel_ms_median"] = round(statistics.median(null_ms[armed]), 3)
    if len(kinds) == 2:
        out["armed_minus_unarmed_median_ms"] = round(out["armed"]["median_ms"] - out["unarmed"]["median_ms"], 3)
    if best is not None:
        out["genes_with_a_best_path"] = {k: int(np.isfinite(best[k].score).sum()) for k in names}
    print(json.dumps(out))
    plan.close()


if __name__ == "__main__":
    main()
