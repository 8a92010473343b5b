"""Time of the carrier tallies per patient (gcre_set_patient_counts, k_set_patient_counts) beside two bounds.

    python tools/patients_time.py [--what call,kernel,reference] [--geometry large,table] [--runs N]

Genes and 5-gene paths are those of tools/clump_time.py (2,000 genes carried by 0.2-1 % of the patients, three strong genes by
9-15 % of the cases more, two thirds of the paths through a strong gene), at two geometries:
  large   1,000,000 sets at 25,000 + 25,000 patients
  table   10,000 sets at 2,500 + 2,500 patients
  call       N calls after a warm-up: wall time of JoinExec.patient_counts and, from the library's own line
             (GCRE_PATIENT_STATS), of the C entry's stages -- host stage, upload, kernel + download -- beside the two bounds
             the tool computes from the shape: the instruction-issue estimate of the inner loop and the member-row bytes read
  kernel     one warm-up and one call, for a run of its own under rocprofv3 --kernel-trace --stats (the trace gives the time)
  reference  report.patient_counts_reference on a slice of the entries it can finish, scaled to all of them (and said so)
One JSON line per item."""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ["GCRE_PATIENT_STATS"] = "1"
from clump_time import PATH_LEN, POOL, STRONG, Stderr, make_sets  # noqa: E402
import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRY = {"large": (1_000_000, 25_000, 25_000), "table": (10_000, 2_500, 2_500)}
PLANES = int(re.search(r"constexpr int kPatientPlanes = (\d+);",
                       open(os.path.join(ROOT, "geneticscre_amd", "csrc", "gcre_kernels.h")).read()).group(1))
# MI355X: 256 CUs x 4 SIMDs, one wave64 vector instruction per 2 cycles per SIMD, 2.4 GHz; aggregate L2 and achievable HBM
SIMDS, CYC_PER_VALU, CLOCK_HZ, L2_BPS, HBM_BPS = 1024, 2, 2.4e9, 34.5e12, 6.3e12


def make_rows(nc: int, nt: int, seed: int = 7):
    """clump_time.make_rows at any cohort size, drawn in blocks of genes (0/1 int8 [POOL][nc + nt])"""
    rng = np.random.default_rng(seed)
    dens = rng.uniform(0.002, 0.01, size=(POOL, 1))
    rows = np.zeros((POOL, nc + nt), np.int8)
    for g0 in range(0, POOL, 100):
        rows[g0:g0 + 100] = rng.random((100, nc + nt), dtype=np.float32) < dens[g0:g0 + 100]
    for g, d in enumerate(STRONG):
        rows[g, :nc] |= (rng.random(nc) < d).astype(np.int8)
    return rng, rows


def bounds(entries: int, members: int, n: int) -> dict:
    """What the kernel has to issue and to read, from the shape alone.  Per (entry, dword column) a lane executes, per member,
    the row address, the select and the OR (3 vector instructions beside the load itself), one AND with the patients' mask,
    and 1/16 of add16: 15 carry-save adders of 2 instructions and a ripple of 2 per plane above the fourth."""
    tiles = -(-n // 2048)
    dwords = -(-n // 32)
    valu = 3 * members + 1 + (30 + 2 * (PLANES - 4)) / 16
    issue_s = entries * tiles * valu * CYC_PER_VALU / (SIMDS * CLOCK_HZ)
    read = entries * members * dwords * 4
    return {"tiles": tiles, "row_dwords": dwords, "valu_per_entry_dword": round(valu, 2), "issue_bound_us": round(issue_s * 1e6, 1),
            "member_row_bytes": read, "bytes_at_l2_us": round(read / L2_BPS * 1e6, 1), "bytes_at_hbm_us": round(read / HBM_BPS * 1e6, 1),
            "gene_rows_bytes": POOL * dwords * 4}


def problem(name: str):
    from geneticscre_amd import api
    S, nc, nt = GEOMETRY[name]
    rng, rows = make_rows(nc, nt)
    sets = make_sets(rng, S)
    off = np.arange(0, (S + 1) * PATH_LEN, PATH_LEN, dtype=np.int64)
    return api.JoinExec(1, nc, nt, 0), rows, (off, np.ascontiguousarray(sets.reshape(-1))), S, nc, nt


def stats_of(text: str):
    return [{k: float(v) if "." in v else int(v) for k, v in (kv.split("=") for kv in ln.split()[1:])}
            for ln in text.splitlines() if ln.startswith("patients entries=")]


def call(name: str, runs: int) -> None:
    ex, rows, hsets, S, nc, nt = problem(name)
    ex.patient_counts(hsets, rows, which=np.arange(64))            # warm-up: code objects
    wall, lib = [], []
    for _ in range(runs):
        with Stderr() as err:
            t0 = time.perf_counter()
            counts, group_sets, skipped = ex.patient_counts(hsets, rows)
            wall.append((time.perf_counter() - t0) * 1e3)
        lib.append(stats_of(err.text)[-1])
    ex.close()
    assert group_sets.tolist() == [S] and skipped == 0
    med = lambda key: round(float(np.median([x[key] for x in lib])), 3)  # noqa: E731
    line = {"tool": "patients_time", "what": "call", "geometry": name, "sets": S, "n_cases": nc, "n_ctrls": nt, "planes": PLANES,
            "python_call_ms": [round(t, 1) for t in wall], "python_call_median_ms": round(float(np.median(wall)), 1),
            "entry_host_stage_median_ms": med("host_ms"), "entry_upload_median_ms": med("upload_ms"),
            "entry_kernel_download_median_ms": med("kernel_download_ms"), "upload_bytes": lib[-1]["upload_bytes"],
            "segments": lib[-1]["segments"], "most_hits_on_one_patient": int(counts.max()),
            "patients_on_a_tenth_of_the_sets": int((counts[0, 0] >= S / 10).sum())}
    entry = line["entry_host_stage_median_ms"] + line["entry_upload_median_ms"] + line["entry_kernel_download_median_ms"]
    line["entry_median_ms"] = round(entry, 3)
    line["upload_share_of_entry"] = round(line["entry_upload_median_ms"] / entry, 3)
    line.update(bounds(S, PATH_LEN, nc + nt))
    print(json.dumps(line), flush=True)


def kernel(name: str) -> None:
    ex, rows, hsets, S, nc, nt = problem(name)
    ex.patient_counts(hsets, rows, which=np.arange(64))
    ex.patient_counts(hsets, rows)
    ex.close()
    line = {"tool": "patients_time", "what": "kernel", "geometry": name, "sets": S, "n_cases": nc, "n_ctrls": nt}
    line.update(bounds(S, PATH_LEN, nc + nt))
    print(json.dumps(line), flush=True)


def reference(name: str, slice_entries: int = 2000) -> None:
    from geneticscre_amd import report
    S, nc, nt = GEOMETRY[name]
    rng, rows = make_rows(nc, nt)
    sets = make_sets(rng, S)[:slice_entries]
    t0 = time.perf_counter()
    report.patient_counts_reference(sets.tolist(), rows, None, None, None, 1, nc + nt, False)
    ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"tool": "patients_time", "what": "reference", "geometry": name, "slice_entries": len(sets),
                      "slice_ms": round(ms, 1), "sets": S, "scaled_to_all_sets_ms": round(ms * S / len(sets), 1),
                      "scaled": "linear in the entries, from the slice"}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="call,reference")
    ap.add_argument("--geometry", default="large,table")
    ap.add_argument("--runs", type=int, default=6)
    a = ap.parse_args()
    for what in [w for w in a.what.split(",") if w]:
        for name in [g for g in a.geometry.split(",") if g]:
            if what == "call":
                call(name, a.runs)
            elif what == "kernel":
                kernel(name)
            elif what == "reference":
                reference(name)
            else:
                raise SystemExit(f"unknown item {what!r}")


if __name__ == "__main__":
    main()
