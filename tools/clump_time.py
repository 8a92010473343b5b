"""Wall time of device-side clumping (gcre_clump_sets) against the old road.

    python tools/clump_time.py [--what road,kernel,large] [--runs N] [--rows ROWS] [--large-sets S]

The cohort is 2,500 + 2,500 patients; genes are carried by 0.2-1 % of the patients, three strong genes by 9-15 % of the
cases more; two thirds of the 5-gene paths run through a strong gene (the mix of tools/overlap_time.py's clump line).
  road    report.clump_paths on a ROWS-row table (10,000), r = 0.5, Jaccard: on_device=False against True, alternating, N
          runs each after one warm-up of each; medians, ranges, and that the two tables are equal
  kernel  one clump_sets call and one set_overlap call over the same ROWS sets, for a run of its own under
          rocprofv3 --kernel-trace --stats: prints the pair-dwords each kernel covers, the trace gives the times
  large   S sets (1,000,000), one clump_sets call: total time, rounds, leads, the share of tiles that ended at the vote
One JSON line per item.  The library's own line (GCRE_CLUMP_STATS) is read from its stderr."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("GCRE_QUIET", "1")
os.environ["GCRE_CLUMP_STATS"] = "1"
import numpy as np  # noqa: E402

NC = NT = 2500
POOL, PATH_LEN, STRONG = 2000, 5, (0.15, 0.12, 0.09)


def make_rows(seed: int = 7):
    rng = np.random.default_rng(seed)
    rows = (rng.random((POOL, NC + NT)) < rng.uniform(0.002, 0.01, size=(POOL, 1))).astype(np.int8)
    for g, dens in enumerate(STRONG):
        rows[g, :NC] |= (rng.random(NC) < dens).astype(np.int8)
    return rng, rows


def make_sets(rng, S: int) -> np.ndarray:
    """int32 [S][5]: distinct genes 3..POOL-1; in two thirds of the sets one of them replaced by a strong gene"""
    sets = np.argsort(rng.random((S, POOL - 3), dtype=np.float32), axis=1)[:, :PATH_LEN].astype(np.int32) + 3 if S <= 20000 \
        else rng.integers(3, POOL, (S, PATH_LEN), dtype=np.int32)
    hit = np.arange(S) % 3 != 0
    sets[hit, rng.integers(0, PATH_LEN, S)[hit]] = rng.integers(0, 3, S)[hit]
    return sets


class Stderr:
    """The process's stderr (the library writes there) into a file for the length of a block."""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()

    def stats(self):
        out = []
        for ln in self.text.splitlines():
            if ln.startswith("clump rows="):
                out.append({k: int(v) for k, v in (kv.split("=") for kv in ln.split()[1:])})
        return out


def scores_of(rows, sets):
    U = np.zeros((len(sets), rows.shape[1]), bool)
    for k in range(sets.shape[1]):
        U |= rows[sets[:, k]] != 0
    ca, ct = U[:, :NC].sum(axis=1), U[:, NC:].sum(axis=1)
    return (ca - ct).astype(np.float64) ** 2 / (ca + ct + 1.0), ca, ct


def road(rows_n: int, runs: int) -> None:
    import pandas as pd
    from geneticscre_amd import report
    rng, rows = make_rows()
    sets = make_sets(rng, rows_n)
    genes = [f"G{i}" for i in range(POOL)]
    sc, ca, ct = scores_of(rows, sets)
    df = pd.DataFrame({"SignedPaths": [" -> ".join(f"{genes[g]} (+)" for g in s) for s in sets.tolist()],
                       "Paths": [" -> ".join(genes[g] for g in s) for s in sets.tolist()],
                       "Lengths": np.full(rows_n, PATH_LEN), "Scores": sc, "Pvalues": np.zeros(rows_n), "Cases": ca, "Controls": ct})
    kw = dict(r=0.5, threshold=1.0)
    ms = {False: [], True: []}
    got = {}
    with Stderr() as err:
        for i in range(runs + 1):           # run 0 of each road is the warm-up
            for dev in (False, True):
                t0 = time.perf_counter()
                got[dev] = report.clump_paths(df, genes, rows, NC, NT, on_device=dev, **kw)
                if i:
                    ms[dev].append((time.perf_counter() - t0) * 1e3)
    pd.testing.assert_frame_equal(got[True], got[False], check_exact=True)
    sizes = np.bincount(got[True]["Clump"].to_numpy())
    line = {"tool": "clump_time", "what": "road", "rows": rows_n, "n_cases": NC, "n_ctrls": NT, "r": 0.5, "measure": "jaccard",
            "leads": int(len(sizes)), "largest_clump": int(sizes.max()), "equal": True}
    for dev, name in ((False, "host_road"), (True, "device_road")):
        line[name + "_ms"] = [round(t, 1) for t in ms[dev]]
        line[name + "_median_ms"] = round(float(np.median(ms[dev])), 1)
    line["library"] = err.stats()[-1]
    print(json.dumps(line), flush=True)


def kernel(rows_n: int) -> None:
    from geneticscre_amd import api
    rng, rows = make_rows()
    sets = make_sets(rng, rows_n)
    sc, _, _ = scores_of(rows, sets)
    order = np.argsort(-sc, kind="stable")
    off = np.arange(0, (rows_n + 1) * PATH_LEN, PATH_LEN, dtype=np.int64)
    ex = api.JoinExec(1, NC, NT, 0)
    with Stderr() as err:
        t0 = time.perf_counter()
        c, l, v, sh, size = ex.clump_sets((off, sets.reshape(-1)), rows, order, 0.5)
        clump_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ex.set_overlap(sets.tolist(), rows)
    overlap_ms = (time.perf_counter() - t0) * 1e3
    ex.close()
    wd = -(-2 * -(-(NC + NT) // 64) // 32) * 32
    st = err.stats()[-1]
    print(json.dumps({"tool": "clump_time", "what": "kernel", "sets": rows_n, "dwords_per_row": wd, "clump_sets_ms": round(clump_ms, 1),
                      "set_overlap_ms": round(overlap_ms, 1), "leads": int((l == np.arange(rows_n)).sum()), "library": st,
                      "assign_pair_dwords_upper": st["tiles_run"] * 64 * 64 * wd,
                      "overlap_pair_dwords": (-(-rows_n // 64) * 64) ** 2 * wd}), flush=True)


def large(S: int) -> None:
    from geneticscre_amd import api
    rng, rows = make_rows()
    sets = make_sets(rng, S)
    order = rng.permutation(S).astype(np.int64)   # (any order: the sets are drawn independently of their position)
    off = np.arange(0, (S + 1) * PATH_LEN, PATH_LEN, dtype=np.int64)
    ex = api.JoinExec(1, NC, NT, 0)
    ex.clump_sets((off[:1001], sets[:1000].reshape(-1)), rows, np.arange(1000), 0.5)   # warm-up: code objects
    with Stderr() as err:
        t0 = time.perf_counter()
        c, l, v, sh, size = ex.clump_sets((off, sets.reshape(-1)), rows, order, 0.5)
        ms = (time.perf_counter() - t0) * 1e3
    ex.close()
    st = err.stats()[-1]
    tiles = st["tiles_run"] + st["tiles_skipped"]
    print(json.dumps({"tool": "clump_time", "what": "large", "sets": S, "n_cases": NC, "n_ctrls": NT, "r": 0.5, "measure": "jaccard",
                      "total_ms": round(ms, 1), "rounds": st["rounds"], "leads": st["leads"], "batches": st["batches"],
                      "tiles_run": st["tiles_run"], "tiles_skipped": st["tiles_skipped"],
                      "tiles_skipped_share": round(st["tiles_skipped"] / max(tiles, 1), 4),
                      "largest_clump": int(np.bincount(c).max()), "bytes_back_per_row": 32}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="road,kernel,large")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--large-sets", type=int, default=1000000)
    a = ap.parse_args()
    for what in [w for w in a.what.split(",") if w]:
        if what == "road":
            road(a.rows, a.runs)
        elif what == "kernel":
            kernel(a.rows)
        elif what == "large":
            large(a.large_sets)
        else:
            raise SystemExit(f"unknown item {what!r}")


if __name__ == "__main__":
    main()
