"""What tests/test_family_host.py and tests/test_minp_host.py share: tests/native/family_main.cpp built under the address
and undefined-behaviour sanitizers and run on a case file, and the device's part of gcre_score_sets_family and
gcre_score_sets_minp taken literally from a null matrix, so that the native finish can be fed
what the kernels would leave.  No GPU needed."""
from __future__ import annotations

import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "family_main.cpp")
TILE = 512          # kSetPermTile
ONES = 0xFFFFFFFF


def build_prog(directory) -> str:
    out = str(directory / "family_main")
    # the sanitizers' runtimes are linked statically: the program then runs whatever the environment it inherits preloads
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", SRC, "-o", out], check=True)
    return out


def run_case(prog, tmp_path, case, env=None):
    """``case``: (key, value or list of values) pairs, one line each; returns the program's output lines."""
    lines = []
    for k, v in case:
        lines.append(" ".join([k] + [repr(float(x)) if isinstance(x, float) else str(x) for x in (v if isinstance(v, (list, tuple)) else [v])]))
    path = tmp_path / "case.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout}\n{r.stderr}"
    return r.stdout.splitlines()


def ints(line: str, name: str):
    words = line.split()
    assert words[0] == name, line
    return [int(w) for w in words[1:]]


def f32_threshold(score: float) -> int:
    """The bit pattern of the smallest float32 x with (double)x >= score among the non-negative floats."""
    if np.isnan(score):
        return 0x7F800001
    if score <= 0:
        return 0
    f = np.float32(score)
    if float(f) < score:
        f = np.nextafter(f, np.float32(np.inf))
    return int(np.array([f], np.float32).view(np.uint32)[0])


def family_walk(obs):
    """Rows of the walk -> valid set: NaN scores first, then ascending as doubles (+-0 tie), stable; and which rows end a tie
    group (a NaN score equals nothing: every NaN row does)."""
    order = sorted(range(len(obs)), key=lambda v: (0, 0.0) if np.isnan(obs[v]) else (1, obs[v]))
    ends = [i + 1 == len(order) or not obs[order[i + 1]] == obs[order[i]] for i in range(len(order))]
    return order, ends


def family_device_part(obs, null):
    """What k_family_scan and k_family_hist leave for the valid sets' scores ``obs`` [V] and their float32 null matrix [V][K]:
    sd[i] at the last row i of every tie group = the columns whose maximum over rows 0 .. i of the walk reaches the group's
    threshold (0 elsewhere), and hist[b] = the cells whose largest threshold reached among the distinct ones is pat[b]."""
    order, ends = family_walk(obs)
    bits = np.ascontiguousarray(null, np.float32).view(np.uint32)[order]       # [V][K], rows in the walk's order
    thr = [f32_threshold(obs[v]) for v in order]
    sd = [0] * len(order)
    run = np.zeros(bits.shape[1], np.uint32)
    for i in range(len(order)):
        run = np.maximum(run, bits[i])
        if ends[i]:
            sd[i] = int((run >= thr[i]).sum())
    pat = sorted({thr[i] for i in range(len(order)) if not np.isnan(obs[order[i]])})
    hist = [0] * max(len(pat), 1)
    for b in bits.ravel().tolist():
        below = [j for j, p in enumerate(pat) if p <= b]
        if below:
            hist[below[-1]] += 1
    return order, sd, pat, hist


def minp_walk(obs, ge):
    """Rows of the walk -> valid set: NaN scores first, then the counts descending, stable; and which rows end a counted tie
    group (a run of equal counts among the scored sets)."""
    order = sorted(range(len(obs)), key=lambda v: (0, 0) if np.isnan(obs[v]) else (1, -int(ge[v])))
    ends = [not np.isnan(obs[order[i]]) and (i + 1 == len(order) or ge[order[i + 1]] != ge[order[i]]) for i in range(len(order))]
    return order, ends


def minp_device_part(obs, null):
    """What k_set_null, k_minp_rank and k_minp_scan leave for the valid sets' scores ``obs`` [V] and their float32 null
    matrix [V][K]: ge[v] = the row's values that reach the score, le[i] at the last row i of every counted tie group = the
    columns whose minimum rank count over rows 0 .. i of the walk is at most the group's count, q = the minimum of every column."""
    N = np.asarray(null, np.float32)
    K = N.shape[1]
    ge = [0 if np.isnan(obs[v]) else int((N[v].astype(np.float64) >= obs[v]).sum()) for v in range(len(obs))]
    R = np.array([[int((N[v] >= N[v][r]).sum()) for r in range(K)] for v in range(len(obs))], np.uint32).reshape(len(obs), K)
    order, ends = minp_walk(obs, ge)
    le = [0] * len(order)
    q = np.full(K, ONES, np.uint32)
    for i, v in enumerate(order):
        q = np.minimum(q, R[v])
        if ends[i]:
            le[i] = int((q <= ge[v]).sum())
    return order, ge, le, q.tolist()
