"""What hit lists (gcre_hits) cost and buy, at BASELINE configs[2] geometry (bench.py "roofline": 17,000
genes, 200,000 relations, 5,000 patients, 10,000 permutations, path length 4).  One JSON line per measurement, on stdout and
appended to --out when given (profiles/hits_time.txt is put together from them).

    python tools/hits_time.py ab --parent geneticscre_amd/variants/libgcre_hip_parent.so [--runs 12]
        the unarmed headline: `python bench.py --gpus 1 --steps 20 --warmup 5` on this build and on the parent commit's
        library (tools/build_variant.py in a checkout of the parent, GCRE_LIB=), alternating, a fresh process each; this
        build's median per-pass time against the parent's own min-max range, and every result_sha256
    python tools/hits_time.py armed [--passes 5] [--warmup 2] [--alpha 0.05] [--cutoff ninf]
        resident passes with a list on every level and without, interleaved.  The cut-off of a level is
        report.significance_cutoff of its own null maxima at --alpha, or -inf with --cutoff ninf (every scorable path is a
        hit: the other end of k_hits_collect's bytes bound).  Also: how many paths each length has at that level against
        the top_k it had.  The kernel's own time comes from a run of this mode under rocprofv3 --kernel-trace --stats
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GCRE_QUIET", "1")


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "n": len(ms)}


def emit(out_path, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write(line + "\n")


def bench_once(lib):
    env = dict(os.environ)
    env.pop("GCRE_LIB", None)
    if lib:
        env["GCRE_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                       env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py failed ({r.returncode}): {r.stderr[-2000:]}")
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return float(line["ms_per_step"]), str(line["result_sha256"])


def mode_ab(a):
    series = {"parent": [], "this": []}
    shas = set()
    for i in range(a.runs):
        order = ("parent", "this") if i % 2 == 0 else ("this", "parent")
        for who in order:
            ms, sha = bench_once(os.path.abspath(a.parent) if who == "parent" else None)
            series[who].append(round(ms, 3))
            shas.add(sha)
    p, t = series["parent"], series["this"]
    med = statistics.median(t)
    emit(a.out, {"mode": "ab", "command": "python bench.py --gpus 1 --steps 20 --warmup 5", "parent_ms_per_step": p,
                 "this_ms_per_step": t, "parent": spread(p), "this": spread(t),
                 "this_median_inside_parent_range": bool(min(p) <= med <= max(p)), "result_sha256": sorted(shas)})


def mode_armed(a):
    import bench
    from geneticscre_amd import api, report
    prob, masks = bench.build_inputs(dict(bench.CONFIGS["roofline"]), 20261003, 100)
    plan = api.ResidentPlan(prob, packed_masks=masks, mask_seed=None if masks is not None else 1)
    names = report.GENE_LEVELS[:prob.path_length]
    first = plan.run()
    ninf = a.cutoff == "ninf"
    cut = {k: float("-inf") if ninf else report.significance_cutoff(first[k].null, a.alpha) for k in names}
    cap = {k: min(api.HITS_CAP_MAX, max(1, int(prob.levels.n_paths[k]))) if ninf else a.cap for k in names}
    lists = {k: api.HitList(plan.ex, cut[k], cap=cap[k]) for k in names}     # (allocated once: a pass resets and re-arms)

    def one(armed):
        if armed:
            for h in lists.values():
                h.reset()
        t0 = time.perf_counter()
        plan.run(hits=lists if armed else None)
        got = {k: h.count() for k, h in lists.items()} if armed else None
        return (time.perf_counter() - t0) * 1e3, got

    for _ in range(a.warmup):
        for armed in (False, True):
            one(armed)
    times, got = {True: [], False: []}, None
    for _ in range(a.passes):
        for armed in (False, True):
            ms, g = one(armed)
            times[armed].append(ms)
            got = g or got
    t0 = time.perf_counter()
    read = {k: h.read() for k, h in lists.items()}
    read_ms = (time.perf_counter() - t0) * 1e3
    rec = {"mode": "armed", "cutoff": "-inf" if ninf else f"significance_cutoff(alpha={a.alpha})",
           "cutoffs": {k: cut[k] for k in names}, "cap": cap, "top_k": prob.top_k, "permutations": prob.iterations,
           "joined_paths": {k: int(prob.levels.n_paths[k]) for k in names}, "found": {k: got[k][0] for k in names},
           "paths_looked_at": {k: got[k][1] for k in names}, "complete": {k: bool(read[k].complete) for k in names},
           "read_and_sort_ms": round(read_ms, 3),
           "top_k_rows_at_or_above_cutoff": {k: int((first[k].scores >= cut[k]).sum()) for k in names},
           "unarmed": spread(times[False]), "armed": spread(times[True])}
    rec["armed_minus_unarmed_median_ms"] = round(rec["armed"]["median_ms"] - rec["unarmed"]["median_ms"], 3)
    # bytes k_hits_collect has to move at the very least: the key of every path, the operand fields and the record of a hit
    paths, found = sum(got[k][1] for k in names), sum(min(got[k][0], cap[k]) for k in names)
    rec["bytes_bound"] = {"key_bytes": 8 * paths, "hit_bytes": (24 + 32) * found, "total": 8 * paths + 56 * found}
    emit(a.out, rec)
    plan.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["ab", "armed"])
    ap.add_argument("--parent", default=os.path.join(ROOT, "geneticscre_amd", "variants", "libgcre_hip_parent.so"))
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--alpha", type=float, default=0.05)
    ap.add_argument("--cutoff", default="alpha", choices=["alpha", "ninf"])
    ap.add_argument("--cap", type=int, default=1 << 24)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    {"ab": mode_ab, "armed": mode_armed}[a.mode](a)


if __name__ == "__main__":
    main()
