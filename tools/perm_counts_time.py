"""What per-permutation exceedance counts (gcre_exceed_keep_perm_counts) cost, at BASELINE configs[2] geometry
(bench.py "roofline": 17,000 genes, 200,000 relations, 5,000 patients, 10,000 permutations, path length 4), ten thresholds per
level = the level's ten best scores, counters on all four levels.  One JSON line per measurement, on stdout and appended to
--out when given (profiles/perm_counts_time.txt is put together from them).

    python tools/perm_counts_time.py armed --parent geneticscre_amd/variants/libgcre_hip_parent.so [--rounds 3] [--passes 4]
        (a) resident passes with perm_counts=True, with perm_counts=False, and the parent commit's library armed
        (tools/build_variant.py in a checkout of the parent, GCRE_LIB=).  A library is fixed when a process loads it, so the
        parent runs in processes of its own: every round starts one worker on the parent's library and one on this build
        (which interleaves perm_counts False / True pass by pass), the order of the two swapped from round to round;
        rounds x passes timed passes of each kind
    python tools/perm_counts_time.py worker --kinds plain,perm [--passes 4] [--warmup 1]
        one such process (GCRE_LIB= for the parent, --kinds plain).  (b): this mode with --kinds perm under
        rocprofv3 --kernel-trace --stats, in a run of its own, gives k_exceed_ie per pass
    python tools/perm_counts_time.py ab --parent ... [--runs 12]
        (c) the unarmed headline: `python bench.py --gpus 1 --steps 20 --warmup 5`, this build against the parent,
        alternating, a fresh process each (tools/exceed_time.py ab), and every result_sha256
    python tools/perm_counts_time.py slow [--level 1b] [--passes 5]
        the slow case, not a target: one threshold <= 0 on a small level -- every value passes, every one is an atomic on
        its cell --, perm_counts False against True
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("GCRE_QUIET", "1")
import numpy as np  # noqa: E402
from exceed_time import emit, mode_ab, roofline_plan, spread  # noqa: E402

KINDS = {"plain": False, "perm": True}


def timed_passes(plan, names, thr, kinds, passes, warmup):
    """Interleaved resident passes: kind -> ms per pass (the run plus the reads of the counters), and the last counts."""
    from geneticscre_amd import api

    def one(kind):
        kw = {"perm_counts": True} if KINDS[kind] else {}
        xs = {k: api.ExceedCounts(plan.ex, thr[k], **kw) for k in names}
        t0 = time.perf_counter()
        plan.run(exceeds=xs)
        got = {k: x.read() for k, x in xs.items()}
        ms = (time.perf_counter() - t0) * 1e3
        for x in xs.values():
            x.free()
        return ms, got

    for _ in range(warmup):
        for kind in kinds:
            one(kind)
    times, last = {k: [] for k in kinds}, {}
    for _ in range(passes):
        for kind in kinds:
            ms, last[kind] = one(kind)
            times[kind].append(round(ms, 3))
    return times, last


def check(got_perm, got_plain):
    """The per-permutation array is consistent with the totals it was counted next to."""
    for k, g in got_perm.items():
        assert (g.perm_counts.sum(axis=1) == g.exceed).all(), k
        if got_plain is not None:
            assert (g.exceed == got_plain[k].exceed).all() and (g.observed == got_plain[k].observed).all(), k


def mode_worker(a):
    from geneticscre_amd import report
    prob, plan = roofline_plan()
    names = report.GENE_LEVELS[:prob.path_length]
    first = plan.run()
    thr = {k: np.sort(first[k].scores[np.isfinite(first[k].scores)])[-a.thresholds:] for k in names}
    kinds = a.kinds.split(",")
    times, last = timed_passes(plan, names, thr, kinds, a.passes, a.warmup)
    rec = {"mode": "worker", "library": os.environ.get("GCRE_LIB", "this build"), "thresholds_per_level": a.thresholds,
           "permutations": prob.iterations, "ms": times}
    if "perm" in last:
        check(last["perm"], last.get("plain"))
        g = last["perm"]
        # what the distribution looks like at each level's best score: mean, median, 95th percentile, maximum over permutations
        rec["false_counts_at_best_score"] = {
            k: {"mean": float(v.perm_counts[-1].mean()), "median": float(np.median(v.perm_counts[-1])),
                "p95": float(np.sort(v.perm_counts[-1])[int(np.ceil(0.95 * v.perm_counts.shape[1])) - 1]),
                "max": int(v.perm_counts[-1].max()), "permutations_with_any": int((v.perm_counts[-1] > 0).sum())}
            for k, v in g.items()}
    emit(a.out, rec)
    plan.close()


def run_worker(a, lib, kinds):
    env = dict(os.environ)
    env.pop("GCRE_LIB", None)
    if lib:
        env["GCRE_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", "--kinds", kinds, "--passes", str(a.passes),
                        "--warmup", str(a.warmup), "--thresholds", str(a.thresholds)], env=env, capture_output=True, text=True,
                       timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"worker failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def mode_armed(a):
    series = {"parent_plain": [], "plain": [], "perm": []}
    dist = None
    for i in range(a.rounds):
        for who in (("parent", "this") if i % 2 == 0 else ("this", "parent")):
            if who == "parent":
                series["parent_plain"] += run_worker(a, os.path.abspath(a.parent), "plain")["ms"]["plain"]
            else:
                rec = run_worker(a, None, "plain,perm")
                series["plain"] += rec["ms"]["plain"]
                series["perm"] += rec["ms"]["perm"]
                dist = rec.get("false_counts_at_best_score")
    pp, pl, pe = (spread(series[k]) for k in ("parent_plain", "plain", "perm"))
    emit(a.out, {"mode": "armed", "rounds": a.rounds, "passes_per_round": a.passes, "thresholds_per_level": a.thresholds,
                 "ms": series, "parent_armed": pp, "perm_counts_false": pl, "perm_counts_true": pe,
                 "false_median_inside_parent_range": bool(pp["min_ms"] <= pl["median_ms"] <= pp["max_ms"]),
                 "true_minus_false_median_ms": round(pe["median_ms"] - pl["median_ms"], 3),
                 "parent_range_ms": round(pp["max_ms"] - pp["min_ms"], 3), "false_counts_at_best_score": dist})


def mode_slow(a):
    prob, plan = roofline_plan()
    plan.run()
    thr = {a.level: np.array([-1.0])}
    times, last = timed_passes(plan, [a.level], thr, ["plain", "perm"], a.passes, a.warmup)
    check(last["perm"], last["plain"])
    P = int(prob.levels.n_paths[a.level])
    assert (last["perm"][a.level].perm_counts == P).all()      # every value of every permutation passes
    emit(a.out, {"mode": "slow", "level": a.level, "joined_paths": P, "permutations": prob.iterations,
                 "values_that_pass": P * prob.iterations, "perm_counts_false": spread(times["plain"]),
                 "perm_counts_true": spread(times["perm"]),
                 "true_minus_false_median_ms": round(statistics.median(times["perm"]) - statistics.median(times["plain"]), 3)})
    plan.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["armed", "worker", "ab", "slow"])
    ap.add_argument("--parent", default=os.path.join(ROOT, "geneticscre_amd", "variants", "libgcre_hip_parent.so"))
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kinds", default="plain,perm")
    ap.add_argument("--thresholds", type=int, default=10)
    ap.add_argument("--level", default="1b")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    {"armed": mode_armed, "worker": mode_worker, "ab": mode_ab, "slow": mode_slow}[a.mode](a)


if __name__ == "__main__":
    main()
