"""What null exceedance counts (gcre_exceed) cost, at BASELINE configs[2] geometry (bench.py "roofline": 17,000
genes, 200,000 relations, 5,000 patients, 10,000 permutations, path length 4).  One JSON line per measurement, on stdout and
appended to --out when given (profiles/exceed_time.txt is put together from them).

    python tools/exceed_time.py ab --parent geneticscre_amd/variants/libgcre_hip_parent.so [--runs 12]
        the unarmed headline: `python bench.py --gpus 1 --steps 20 --warmup 5` on this build and on the parent commit's
        library (tools/build_variant.py in a checkout of the parent, GCRE_LIB=), alternating, a fresh process each; this
        build's median per-pass time against the parent's own min-max range, and every result_sha256
    python tools/exceed_time.py armed [--passes 5] [--warmup 2] [--form ie|dense] [--thresholds 10]
        resident passes with counters on every level (thresholds: the level's top scores) and without, interleaved; the
        kernels' own time comes from a run of this mode under rocprofv3 --kernel-trace --stats
    python tools/exceed_time.py unpruned [--passes 5] [--warmup 2]
        gcre_profile.null_kernel_ms of passes under GCRE_IE_PRUNE=0 (set GCRE_LIB= for the parent's library): the yardstick
        of k_exceed_ie, which does the count work of an unpruned pass
    python tools/exceed_time.py gwaspa
        report.gwaspa(fdr=True) against fdr=False on a 2,000-gene network, whole calls
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
import numpy as np  # noqa: E402


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


def roofline_plan():
    import bench
    from geneticscre_amd import api
    cfg = dict(bench.CONFIGS["roofline"])
    prob, masks = bench.build_inputs(cfg, 20261003, 100)
    return prob, api.ResidentPlan(prob, packed_masks=masks, mask_seed=None if masks is not None else 1)


def mode_armed(a):
    from geneticscre_amd import api, report
    if a.form:
        os.environ["GCRE_EXCEED_KERNEL"] = a.form
    prob, plan = roofline_plan()
    names = report.GENE_LEVELS[:prob.path_length]
    first = plan.run()
    thr = {}
    for k in names:
        s = first[k].scores[np.isfinite(first[k].scores)]
        thr[k] = np.sort(s)[-a.thresholds:]

    def one(armed):
        xs = {k: api.ExceedCounts(plan.ex, thr[k]) for k in names} if armed else None
        t0 = time.perf_counter()
        plan.run(exceeds=xs)
        got = {k: x.read() for k, x in xs.items()} if armed else None
        ms = (time.perf_counter() - t0) * 1e3
        prof = dict(plan.last_profile)
        for x in (xs or {}).values():
            x.free()
        return ms, prof, got

    kinds = [True] if a.only_armed else [False, True]
    for _ in range(a.warmup):
        for armed in kinds:
            one(armed)
    times, null_ms, got = {True: [], False: []}, {True: [], False: []}, None
    for _ in range(a.passes):
        for armed in kinds:
            ms, prof, g = one(armed)
            times[armed].append(ms)
            null_ms[armed].append(prof["null_kernel_ms"])
            got = g or got
    rec = {"mode": "armed", "form": a.form or "ie (default)", "thresholds_per_level": a.thresholds,
           "joined_paths": {k: int(prob.levels.n_paths[k]) for k in names}, "permutations": prob.iterations,
           "windows": len(plan.windows())}
    for armed in kinds:
        key = "armed" if armed else "unarmed"
        rec[key] = spread(times[armed])
        rec[key]["null_kernel_ms_median"] = round(statistics.median(null_ms[armed]), 3)
    if len(kinds) == 2:
        rec["armed_minus_unarmed_median_ms"] = round(rec["armed"]["median_ms"] - rec["unarmed"]["median_ms"], 3)
    rec["counts"] = {k: {"exceed": got[k].exceed.tolist(), "observed": got[k].observed.tolist(), "perms": got[k].perms} for k in names}
    emit(a.out, rec)
    plan.close()


def mode_unpruned(a):
    os.environ["GCRE_IE_PRUNE"] = "0"
    prob, plan = roofline_plan()
    for _ in range(a.warmup):
        plan.run()
    null_ms, pass_ms = [], []
    for _ in range(a.passes):
        t0 = time.perf_counter()
        plan.run()
        pass_ms.append((time.perf_counter() - t0) * 1e3)
        null_ms.append(plan.last_profile["null_kernel_ms"])
    emit(a.out, {"mode": "unpruned", "GCRE_IE_PRUNE": "0", "library": os.environ.get("GCRE_LIB", "this build"),
                 "null_kernel_ms": spread(null_ms), "pass": spread(pass_ms)})
    plan.close()


def mode_gwaspa(a):
    from geneticscre_amd import report, synth
    rng = np.random.default_rng(4)
    nc, nt, K = 500, 500, 4096
    g, src, trg, sign = synth.signed_network(2000, 12000, rng)
    uid = np.arange(g) * 3 + 10
    symbols = [f"G{u}" for u in uid]
    data = (rng.random((g, nc + nt)) < 0.03).astype(np.int32)
    network = (uid, symbols, uid[src], uid[trg], sign)
    kw = dict(threshold=0.2, n_permutations=K, seed=5, top_k=100, path_length=4)
    times = {False: [], True: []}
    for i in range(a.warmup + a.passes):
        for fdr in (False, True):
            t0 = time.perf_counter()
            out = report.gwaspa(symbols, data, nc, nt, network, fdr=fdr, **kw)
            if i >= a.warmup:
                times[fdr].append((time.perf_counter() - t0) * 1e3)
    q = out["GWASPA.Results"]["Qvalues"].to_numpy()
    emit(a.out, {"mode": "gwaspa", "genes": g, "relations": len(src), "patients": nc + nt, "permutations": K, "top_k": 100,
                 "joined_paths": {k: int(v.paths) for k, v in out["exceed"].items()},
                 "fdr_false": spread(times[False]), "fdr_true": spread(times[True]),
                 "qvalues_min_median_max": [float(np.nanmin(q)), float(np.nanmedian(q)), float(np.nanmax(q))]})


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["ab", "armed", "unpruned", "gwaspa"])
    ap.add_argument("--parent", default=os.path.join(ROOT, "geneticscre_amd", "variants", "libgcre_hip_parent.so"))
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--form", default="", choices=["", "ie", "dense"])
    ap.add_argument("--thresholds", type=int, default=10)
    ap.add_argument("--only-armed", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    {"ab": mode_ab, "armed": mode_armed, "unpruned": mode_unpruned, "gwaspa": mode_gwaspa}[a.mode](a)


if __name__ == "__main__":
    main()
