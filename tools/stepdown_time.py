"""What step-down max-T counts (gcre_exceed_stepdown) cost.  One JSON line per measurement, on stdout and
appended to --out when given (profiles/stepdown_time.txt is put together from them).

    python tools/stepdown_time.py kernels [--perms 65536] [--reps 3] [--methods 1,2]
        k_stepdown_null against k_set_null on the same rows in one session, at the geometry of tools/sets_time.py (configs[4]:
        25,000 cases, 25,000 controls; its 1,000 random length-5 paths), and k_stepdown_finish.  1,000 thresholds x 100,000
        permutations is above the 2^26 cells an ExceedCounts may keep per permutation, so both kernels run at 65,536
        permutations.  The rows are not the top rows of a join: the counters are filled by a small stand-in join on the same
        context, the call passes the score check (the thresholds are the rows' own scores), launches both kernels and then
        ends in the "not distinct joined paths" refusal, which is caught -- the kernels have done all their work by then.
        Host wall time per call here; the kernels' own time from a run of this mode under rocprofv3 --kernel-trace --stats
    python tools/stepdown_time.py gwaspa [--passes 3] [--warmup 1]
        report.gwaspa(stepdown=True) against false_counts=True alone and against neither, whole calls, on the 2,000-gene
        network of tools/exceed_time.py gwaspa
    python tools/stepdown_time.py column [--rows 10]
        what the column shows at BASELINE configs[2] (bench.py "roofline"): per level, how many of the ten best rows have
        PvaluesStepDown < Pvalues
    python tools/stepdown_time.py ab --parent geneticscre_amd/variants/libgcre_hip_parent.so [--runs 6]
        the unarmed headline: `python bench.py --gpus 1 --steps 20 --warmup 5`, this build against the parent commit's library,
        alternating, a fresh process each (tools/exceed_time.py ab), and every result_sha256
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("GCRE_QUIET", "1")
import numpy as np  # noqa: E402
from exceed_time import emit, mode_ab, roofline_plan, spread  # noqa: E402


def mode_kernels(a):
    import sets_time
    from decorated_time import corner_table
    from geneticscre_amd import api
    from geneticscre_amd.uids import UidRelSet
    rows, sets, signs = sets_time.make_case()
    sets, signs = sets[:sets_time.N_PATHS], signs[:sets_time.N_PATHS]
    nc, nt = sets_time.N_CASES, sets_time.N_CTRLS
    table = corner_table(nc, nt, a.corner)
    m = len(sets)
    for method in [int(x) for x in a.methods.split(",")]:
        ex = api.JoinExec(method, nc, nt, a.perms)
        ex.set_value_table(table)
        ex.generate_permutations(1)
        rec = ex.score_sets(sets, rows, signs)                       # warm-up, and the rows' own scores
        t_set = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ex.score_sets(sets, rows, signs)
            t_set.append((time.perf_counter() - t0) * 1e3)
        x = api.ExceedCounts(ex, rec["score"], perm_counts=True)
        ids = np.arange(8, dtype=np.int32)
        u = UidRelSet(1, ids, ids, np.ones(8, np.int32), np.arange(8, dtype=np.int64), np.ones(8, np.int32))
        ex.join(u, ex.create_path_set(8), ex.load(rows[:8].astype(np.int32)), None, exceed=x)   # one full pass of some join
        t_sd, ended = [], set()
        for _ in range(a.reps + 1):
            before = ex.stepdown_launches()
            t0 = time.perf_counter()
            try:
                x.stepdown(sets, rows, signs)
                ended.add("ok")
            except api.GcreError as e:
                assert "not distinct joined paths" in str(e), e
                ended.add("refused after the kernels: not joined paths of the stand-in join")
            t_sd.append((time.perf_counter() - t0) * 1e3)
            assert ex.stepdown_launches() == before + 2
        kpad = -(-a.perms // 2048) * 2048
        emit(a.out, {"mode": "kernels", "method": method, "n_cases": nc, "n_ctrls": nt, "perms": a.perms, "rows": m,
                     "score_sets_call_ms": spread(t_set), "stepdown_call_ms": spread(t_sd[1:]), "stepdown_call_ended": sorted(ended),
                     "estimate_valu_ms": round(sets_time.estimate_ms(m, a.perms, method), 2),
                     "finish_bytes": 2 * m * kpad * 4, "finish_ms_at_4_TB_s": round(2 * m * kpad * 4 / 4e12 * 1e3, 4)})
        ex.close()


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
    kinds = {"neither": {}, "false_counts": {"false_counts": True}, "stepdown": {"stepdown": True},
             "both": {"false_counts": True, "stepdown": True}}
    times = {k: [] for k in kinds}
    for i in range(a.warmup + a.passes):
        for k, flags in kinds.items():
            t0 = time.perf_counter()
            out = report.gwaspa(symbols, data, nc, nt, network, **flags, **kw)
            if i >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
            if k == "stepdown":
                df = out["GWASPA.Results"]
    sd, pv = df["PvaluesStepDown"].to_numpy(np.float64), df["Pvalues"].to_numpy(np.float64)
    ok = np.isfinite(sd)
    assert (sd[ok] <= pv[ok]).all()
    emit(a.out, {"mode": "gwaspa", "genes": g, "relations": len(src), "patients": nc + nt, "permutations": K, "top_k": 100,
                 **{k: spread(v) for k, v in times.items()},
                 "stepdown_minus_false_counts_median_ms": round(spread(times["stepdown"])["median_ms"] -
                                                                 spread(times["false_counts"])["median_ms"], 3),
                 "rows": int(ok.sum()), "rows_below_Pvalues": int((sd[ok] < pv[ok]).sum())})


def mode_column(a):
    """The ten best rows of every level of the roofline problem: their union rows are read back from the resident operands
    (PathSet.select), so that the sets are the joined paths themselves."""
    from geneticscre_amd import api, report
    prob, plan = roofline_plan()
    names = report.GENE_LEVELS[:prob.path_length]
    first = plan.run()
    M = 1 if prob.method in (1, "method1") else 2
    n = prob.n_cases + prob.n_ctrls
    tops = {}
    for k in names:
        r = first[k]
        idx = np.flatnonzero(np.isfinite(r.scores))
        idx = idx[np.argsort(-r.scores[idx], kind="stable")][:a.rows]
        tops[k] = (r.src[idx].astype(np.int64), r.trg[idx].astype(np.int64), r.scores[idx].astype(np.float64))
    xs = {k: api.ExceedCounts(plan.ex, tops[k][2], perm_counts=True) for k in names}
    t0 = time.perf_counter()
    res = plan.run(exceeds=xs)
    pass_ms = (time.perf_counter() - t0) * 1e3
    rec = {"mode": "column", "rows_per_level": a.rows, "permutations": prob.iterations, "counting_pass_ms": round(pass_ms, 2),
           "levels": {}}
    for k in names:
        src, trg, tau = tops[k]
        p0, p1, _ = plan.operands(k)
        u = prob.levels.uids[k]
        r1 = report._unpack_rows(p1.select(trg.astype(np.int32)).to_numpy(), M, n)
        r0 = report._unpack_rows(p0.select(src.astype(np.int32)).to_numpy(), M, n)
        m = len(tau)
        if M == 1:
            sets, rows, signs = [[i] for i in range(m)], (r0[0] | r1[0]).astype(np.int8), None
        else:
            sg_all, L = np.asarray(u.signs, np.int64), int(u.path_length)
            sg = sg_all[src] if L > 3 else sg_all[trg] if L < 3 else np.where(sg_all[src] + sg_all[trg] == 0, -1, 1)
            keep = (sg == 1)[:, None]
            pos, neg = r0[0] | np.where(keep, r1[0], r1[1]), r0[1] | np.where(keep, r1[1], r1[0])
            sets, rows, signs = [[i, m + i] for i in range(m)], np.vstack([pos, neg]).astype(np.int8), [[1, -1]] * m
        t0 = time.perf_counter()
        n_ge = xs[k].stepdown(sets, rows, signs)
        call_ms = (time.perf_counter() - t0) * 1e3
        K = prob.iterations
        single = (res[k].null.astype(np.float64)[None, :] >= tau[:, None]).sum(axis=1)
        col = report.stepdown_columns(tau, n_ge, K)["PvaluesStepDown"]
        assert (n_ge <= single).all() and n_ge[0] == single[0]
        rec["levels"][k] = {"joined_paths": int(prob.levels.n_paths[k]), "stepdown_call_ms": round(call_ms, 2),
                            "Pvalues": (single / K).tolist(), "PvaluesStepDown": col.tolist(),
                            "rows_below_Pvalues": int((col < single / K).sum())}
    emit(a.out, rec)
    plan.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernels", "gwaspa", "column", "ab"])
    ap.add_argument("--parent", default=os.path.join(ROOT, "geneticscre_amd", "variants", "libgcre_hip_parent.so"))
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--perms", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--corner", type=int, default=6000)
    ap.add_argument("--methods", default="1,2")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    {"kernels": mode_kernels, "gwaspa": mode_gwaspa, "column": mode_column, "ab": mode_ab}[a.mode](a)


if __name__ == "__main__":
    main()
