"""Wall time of conditional set scores (gcre_score_sets_given, k_set_residual) against the loop they replace.

    python tools/given_time.py [--what road,kernel,large] [--runs N] [--rows ROWS[,ROWS..]] [--large-sets S] [--perms K]

The cohort, the genes and the 5-gene paths are those of tools/clump_time.py (2,500 + 2,500 patients, two thirds of the
paths through one of three strong genes); K permutations (1,000).
  road    report.clump_paths(conditional=True, on_device=True) on a ROWS-row table (1,000 and 10,000), r = 0.5, Jaccard,
          three ways, alternating, N runs each after one warm-up of each: `loop` -- the residual columns by the loop this
          replaces (per lead that has members a zeroed copy of the carrier matrix and one score_sets call; kept here as
          loop_columns), `one_call` -- this build, and `held` -- this build on a context the caller holds (exec_=: no
          api.values_table, no masks drawn again).  Medians, ranges, and that the tables are equal.
  kernel  one score_sets(which=, given=) call over the member rows of the largest ROWS table, for a run of its own under
          rocprofv3 --kernel-trace --stats: prints the bytes k_set_residual has to move, the trace gives the times
  large   S sets (1,000,000) clumped on the device in a random walk order, then ONE call over every member row given its
          lead: entries, wall time, slabs
One JSON line per item.  The library's own line (GCRE_GIVEN_STATS) is read from its stderr."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ["GCRE_GIVEN_STATS"] = "1"
from clump_time import NC, NT, PATH_LEN, POOL, Stderr, make_rows, make_sets, scores_of  # noqa: E402
import numpy as np  # noqa: E402


def given_stats(text: str):
    return [{k: int(v) for k, v in (kv.split("=") for kv in ln.split()[1:])}
            for ln in text.splitlines() if ln.startswith("given entries=")]


def loop_columns(out, ex, sets, sub, signs, n):
    """RESIDUAL_COLUMNS as clump_paths filled them before gcre_score_sets_given: one score_sets call per lead with members."""
    from geneticscre_amd import report
    S = len(out)
    clump = out["Clump"].to_numpy()
    is_lead = (clump >= 0) & np.isnan(out["LeadOverlap"].to_numpy())
    lead_of = np.full(int(clump.max()) + 1, -1)
    lead_of[clump[is_lead]] = np.flatnonzero(is_lead)
    lead = np.where(clump >= 0, lead_of[np.maximum(clump, 0)], -1)
    res = {c: np.full(S, np.nan) for c in report.RESIDUAL_COLUMNS}
    C, _ = report.carrier_rows(sets, sub, n)
    members = (clump >= 0) & (lead != np.arange(S))
    calls = 0
    for ld in np.unique(lead[members]).tolist():
        js = np.flatnonzero(members & (lead == ld))
        need = {}
        msets = [[need.setdefault(x, len(need)) for x in sets[j]] for j in js]
        rec = ex.score_sets(msets, np.where(C[ld][None, :], 0, sub[list(need.keys())]), [signs[j] for j in js])
        calls += 1
        for c, f in zip(report.RESIDUAL_COLUMNS, ("score", "cases", "ctrls", "pvalue")):
            res[c][js] = rec[f]
    return res, calls, int(members.sum())


def table_of(rows, sets):
    import pandas as pd
    genes = [f"G{i}" for i in range(POOL)]
    sc, ca, ct = scores_of(rows, sets)
    n = len(sets)
    return genes, pd.DataFrame({"SignedPaths": [" -> ".join(f"{genes[g]} (+)" for g in s) for s in sets.tolist()],
                                "Paths": [" -> ".join(genes[g] for g in s) for s in sets.tolist()],
                                "Lengths": np.full(n, PATH_LEN), "Scores": sc, "Pvalues": np.zeros(n), "Cases": ca, "Controls": ct})


def road(rows_n: int, runs: int, K: int) -> None:
    import pandas as pd
    from geneticscre_amd import api, report
    rng, rows = make_rows()
    sets = make_sets(rng, rows_n)
    genes, df = table_of(rows, sets)
    kw = dict(r=0.5, threshold=1.0, on_device=True, n_permutations=K, seed=11)
    vt = api.values_table(NC, NT)
    held = api.JoinExec(1, NC, NT, K)
    held.set_value_table(vt)
    held.generate_permutations(11, None)
    # what the loop needs beside the clump columns: the sets of the printed paths over the rows they use
    _, prow, psigns = report.parse_sets([str(p) for p in df["SignedPaths"]], genes)
    used = {}
    lsets = [[used.setdefault(x, len(used)) for x in rs] for rs in prow]
    sub = rows[list(used.keys())]

    def loop():
        out = report.clump_paths(df, genes, rows, NC, NT, r=0.5, threshold=1.0, on_device=True)
        ex = api.JoinExec(1, NC, NT, K)
        try:
            ex.set_value_table(api.values_table(NC, NT))
            ex.generate_permutations(11, None)
            res, calls, members = loop_columns(out, ex, lsets, sub, psigns, NC + NT)
        finally:
            ex.close()
        for c in report.RESIDUAL_COLUMNS:
            out[c] = res[c]
        return out, calls, members

    ways = {"loop": lambda: loop()[0],
            "one_call": lambda: report.clump_paths(df, genes, rows, NC, NT, conditional=True, **kw),
            "held": lambda: report.clump_paths(df, genes, rows, NC, NT, conditional=True, exec_=held, **kw)}
    ms = {w: [] for w in ways}
    got = {}
    with Stderr() as err:
        for i in range(runs + 1):           # run 0 of each way is the warm-up
            for w, fn in ways.items():
                t0 = time.perf_counter()
                got[w] = fn()
                if i:
                    ms[w].append((time.perf_counter() - t0) * 1e3)
    for w in ("one_call", "held"):
        pd.testing.assert_frame_equal(got[w], got["loop"], check_exact=True)
        for c in report.RESIDUAL_COLUMNS:
            assert got[w][c].to_numpy().tobytes() == got["loop"][c].to_numpy().tobytes(), (w, c)
    _, calls, members = loop()
    held.close()
    line = {"tool": "given_time", "what": "road", "rows": rows_n, "n_cases": NC, "n_ctrls": NT, "perms": K, "r": 0.5,
            "member_rows": members, "loop_score_sets_calls": calls, "equal": True}
    for w in ways:
        line[w + "_ms"] = [round(t, 1) for t in ms[w]]
        line[w + "_median_ms"] = round(float(np.median(ms[w])), 1)
    line["library"] = given_stats(err.text)[-1]
    print(json.dumps(line), flush=True)


def clumped(S: int, K: int, random_order: bool):
    """S sets of the generator clumped on the device: (context with table and masks, rows, (off, members), member rows, leads)."""
    from geneticscre_amd import api
    rng, rows = make_rows()
    sets = make_sets(rng, S)
    if random_order:
        order = rng.permutation(S).astype(np.int64)
    else:
        order = np.argsort(-scores_of(rows, sets)[0], kind="stable")
    off = np.arange(0, (S + 1) * PATH_LEN, PATH_LEN, dtype=np.int64)
    hsets = (off, np.ascontiguousarray(sets.reshape(-1)))
    ex = api.JoinExec(1, NC, NT, K)
    ex.set_value_table(api.values_table(NC, NT))
    ex.generate_permutations(11, None)
    c, l, v, sh, size = ex.clump_sets(hsets, rows, order, 0.5)
    js = np.flatnonzero((c >= 0) & (l != np.arange(S)))
    return ex, rows, hsets, js, l[js]


def kernel(rows_n: int, K: int) -> None:
    ex, rows, hsets, js, leads = clumped(rows_n, K, False)
    ex.score_sets(hsets, rows, which=js[:64], given=leads[:64])     # warm-up: code objects
    with Stderr() as err:
        t0 = time.perf_counter()
        rec = ex.score_sets(hsets, rows, which=js, given=leads)
        ms = (time.perf_counter() - t0) * 1e3
    full = ex.score_sets(hsets, rows, which=js)                      # the same rows with nothing set aside
    ex.close()
    w2 = 2 * -(-(NC + NT) // 64)
    wp = -(-(w2 // 2) // 4) * 4
    E = len(js)
    print(json.dumps({"tool": "given_time", "what": "kernel", "sets": rows_n, "entries": E, "perms": K, "call_ms": round(ms, 1),
                      "row_dwords": w2, "residual_read_bytes": E * 2 * PATH_LEN * w2 * 4, "residual_written_bytes": E * wp * 8,
                      "mean_union_carriers": round(float((full["cases"] + full["ctrls"]).mean()), 1),
                      "mean_residual_carriers": round(float((rec["cases"] + rec["ctrls"]).mean()), 1),
                      "valid": int(rec["valid"].sum()), "library": given_stats(err.text)[-1]}), flush=True)


def large(S: int, K: int) -> None:
    t0 = time.perf_counter()
    ex, rows, hsets, js, leads = clumped(S, K, True)
    clump_ms = (time.perf_counter() - t0) * 1e3
    ex.score_sets(hsets, rows, which=js[:64], given=leads[:64])     # warm-up
    with Stderr() as err:
        t0 = time.perf_counter()
        rec = ex.score_sets(hsets, rows, which=js, given=leads)
        ms = (time.perf_counter() - t0) * 1e3
    ex.close()
    st = given_stats(err.text)[-1]
    print(json.dumps({"tool": "given_time", "what": "large", "sets": S, "entries": len(js), "leads": S - len(js), "perms": K,
                      "n_cases": NC, "n_ctrls": NT, "setup_and_clump_ms": round(clump_ms, 1), "one_call_ms": round(ms, 1),
                      "slabs": st["slabs"], "slab_sets": st["slab"], "empty_residuals": int((rec["cases"] + rec["ctrls"] == 0).sum()),
                      "residual_p_below_0.05": int((rec["pvalue"] < 0.05).sum())}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="road,kernel,large")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--rows", default="1000,10000")
    ap.add_argument("--large-sets", type=int, default=1000000)
    ap.add_argument("--perms", type=int, default=1000)
    a = ap.parse_args()
    sizes = [int(x) for x in a.rows.split(",") if x]
    for what in [w for w in a.what.split(",") if w]:
        if what == "road":
            for n in sizes:
                road(n, a.runs, a.perms)
        elif what == "kernel":
            kernel(max(sizes), a.perms)
        elif what == "large":
            large(a.large_sets, a.perms)
        else:
            raise SystemExit(f"unknown item {what!r}")


if __name__ == "__main__":
    main()
