#!/usr/bin/env python3
"""A/B of several libraries under the protocol of DESIGN.md 5.1: one bench.py process per run, the libraries alternating
round by round in one session.

    tools/ab_libs.py --rounds 6 parent -            ("-": the product library; NAME: geneticscre_amd/variants/libgcre_hip_NAME.so)
    tools/ab_libs.py --rounds 4 --bench "--config subgraph --steps 40 --warmup 5" parent -

Prints one line per run (ms per step, result digest), then per library median and range, whether every run of a library
was faster than the first library's fastest, and the digests seen.  Stops at the first run that fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs="+")
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--bench", default="--gpus 1 --steps 20 --warmup 5")
ap.add_argument("--timeout", type=int, default=240)
a = ap.parse_args()

ms = {v: [] for v in a.libs}
sha = set()
for r in range(1, a.rounds + 1):
    for v in a.libs:
        env = dict(os.environ)
        env.pop("GCRE_LIB", None)
        if v != "-":
            env["GCRE_LIB"] = os.path.join(ROOT, "geneticscre_amd", "variants", f"libgcre_hip_{v}.so")
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *a.bench.split()], env=env, cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.timeout)
        if p.returncode != 0:
            print(f"{v} r{r} FAILED rc={p.returncode}\n{p.stderr[-2000:]}", flush=True)
            sys.exit(p.returncode if p.returncode > 0 else 1)
        d = json.loads(p.stdout.strip().splitlines()[-1])
        ms[v].append(d["ms_per_step"])
        sha.add(d.get("result_sha256", "")[:16])
        print(f"{v:10s} r{r}  {d['ms_per_step']:8.3f} ms/step  {d['value']:.4e} scores/s  sha {d.get('result_sha256', '')[:16]}", flush=True)
base = a.libs[0]
for v in a.libs:
    x = ms[v]
    line = f"{v:10s} median {statistics.median(x):8.3f}  range {min(x):.3f}-{max(x):.3f} ({max(x) - min(x):.3f})"
    if v != base:
        line += f"  median gain {statistics.median(ms[base]) - statistics.median(x):+.3f} ms; every run below {base}'s fastest: {max(x) < min(ms[base])}"
    print(line)
print("digests:", sorted(sha))
