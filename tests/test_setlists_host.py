"""The set-list host stage of gcre_score_sets, gcre_set_overlap and gcre_exceed_stepdown (csrc/gcre_setlists.h): the C++
itself, not a restatement.  tests/native/setlists_main.cpp is built with the address and undefined-behaviour sanitizers and
run as a child process on one case per run; what it prints is compared with numpy, the counts also with ``restate`` of
test_sets_host.py.  A sanitizer report ends the child with a non-zero status.  No GPU needed."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

from test_sets_host import restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "setlists_main.cpp")
OK, ERR_RANGE, ERR_ARG = 0, -2, -4   # include/gcre_hip.h


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("setlists") / "setlists_main")
    # the sanitizers' runtimes are linked statically: the program then runs whatever the environment it inherits preloads
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", SRC, "-o", out], check=True)
    return out


def run_case(prog, path, lines):
    """Write the case, run the program on it (the test preloads nothing), return its output lines."""
    with open(path, "w") as f:
        f.write("\n".join(" ".join(str(x) for x in ln) for ln in lines) + "\n")
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout}\n{r.stderr}"
    return r.stdout.splitlines()


def pack(bits):
    """0/1 [rows][n] -> uint64 [rows][ceil(n/64)], bit c of word c/64 = column c."""
    bits = np.asarray(bits, np.uint8)
    W = (bits.shape[1] + 63) // 64
    padded = np.zeros((bits.shape[0], 64 * W), np.uint8)
    padded[:, :bits.shape[1]] = bits
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(bits.shape[0], W)


# six rows; the sets: one member, a repeated member, mixed signs, every member (-), an NA member, all rows
SETS = [[3], [1, 1, 4], [0, 2, 5], [2, 4], [0, -1, 3], [0, 1, 2, 3, 4, 5]]
SIGNS = [[1], [1, -1, 1], [1, -1, -1], [-1, -1], [1, 1, -1], [-1, 1, -1, 1, 1, -1]]


def layouts(W):
    """(method, split, signs given, row stride in words): the unsigned method on bare rows, the signed method on rows padded
    to 4 words with and without signs, and the overlap's layout -- nothing split, rows padded to whole 32-dword chunks."""
    Wp = (W + 3) // 4 * 4
    return [(1, 0, True, W), (2, 1, True, Wp), (2, 1, False, Wp + 1), (2, 0, True, (2 * W + 31) // 32 * 32 // 2)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 70])
def test_union_rows_and_counts(prog, tmp_path, n):
    rng = np.random.default_rng(100 + n)
    W = (n + 63) // 64
    bits = (rng.random((6, n)) < 0.4).astype(np.uint8)
    bits[3] = 1   # a full row: every patient of the last word counts, nothing beyond
    words = pack(bits)
    stray = ~np.uint64(0) << np.uint64(n % 64) if n % 64 else np.uint64(0)
    words[::2, W - 1] |= stray   # bits beyond n in the last word of rows 0, 2, 4: to be ignored
    flat_members = [m for s in SETS for m in s]
    off = np.concatenate([[0], np.cumsum([len(s) for s in SETS])])
    for n_cases in sorted({0, 1, n - 1, n}):
        case = np.arange(n) < n_cases
        for method, split, with_signs, stride in layouts(W):
            lines = [("method", method), ("n", n), ("n_cases", n_cases), ("stride", stride), ("split", split),
                     ("n_cols", n), ("n_rows", 6), ("n_sets", len(SETS)), ("rows", *[f"{w:x}" for w in words.ravel()]),
                     ("set_off", *off), ("members", *flat_members)]
            if with_signs:
                lines.append(("signs", *[x for s in SIGNS for x in s]))
            out = run_case(prog, tmp_path / "case.txt", lines)
            assert out[0] == "check 0 "
            recs, _, _ = restate(method if split else 1, n_cases, n - n_cases, SETS, bits, SIGNS if with_signs else None,
                                 np.zeros((n + 1, n + 1)), np.zeros((0, n), bool))
            per = 1 + method
            assert len(out) == 1 + per * len(SETS)
            for s, members in enumerate(SETS):
                head, halves = out[1 + per * s], out[2 + per * s:1 + per * (s + 1)]
                got = np.array([[int(x, 16) for x in h.split()[1:]] for h in halves], np.uint64)
                assert [h.split()[0] for h in halves] == ["P", "N"][:method] and got.shape == (method, stride)
                what = (n, n_cases, method, split, with_signs, stride, s)
                if -1 in members:   # an NA member: invalid, nothing written
                    assert head == f"set {s} valid 0 k 0 0 0 0", what
                    assert not got.any(), what
                    continue
                P, N = np.zeros(n, bool), np.zeros(n, bool)
                for m, sg in zip(members, SIGNS[s]):
                    if split and with_signs and sg == -1:
                        N |= bits[m] != 0
                    else:
                        P |= bits[m] != 0
                want = np.zeros((method, stride), np.uint64)
                want[0, :W] = pack(P[None])[0]
                if method == 2:
                    want[1, :W] = pack(N[None])[0]
                assert np.array_equal(got, want), what
                k = [int((P & case).sum()), int((P & ~case).sum()), int((N & ~case).sum()), int((N & case).sum())]
                assert head == f"set {s} valid 1 k {k[0]} {k[1]} {k[2]} {k[3]}", what
                r = recs[s]
                assert k == [r["cases_pos"], r["ctrls_pos"], r["cases_neg"], r["ctrls_neg"]], what


BASE = dict(method=2, n=70, n_cases=30, stride=4, split=1, n_cols=70, n_rows=3, n_sets=2,
            rows=["0"] * 6, set_off=[0, 2, 3], members=[0, 1, 2], signs=[1, -1, 1])

FAULTS = [
    ("columns", "score_sets", dict(n_cols=69), ERR_ARG, "score_sets: the rows have 69 columns, not n_cases + n_ctrls = 70"),
    ("negative count", "stepdown", dict(n_rows=-1), ERR_ARG, "stepdown: bad input (a negative count or a NULL array)"),
    ("NULL array", "set_overlap", dict(members=None), ERR_ARG, "set_overlap: bad input (a negative count or a NULL array)"),
    ("empty set", "score_sets", dict(set_off=[0, 2, 2]), ERR_ARG, "score_sets: set 1 has no members"),
    ("row range", "set_overlap", dict(members=[0, 3, 2]), ERR_RANGE, "set_overlap: set 0: member row 3 out of range (3 rows)"),
    ("sign 0", "stepdown", dict(signs=[1, -1, 0]), ERR_ARG, "stepdown: set 1: sign 0 is neither +1 nor -1"),
]


@pytest.mark.parametrize("name,who,change,code,message", FAULTS, ids=[f[0] for f in FAULTS])
def test_faults_keep_their_code_and_message(prog, tmp_path, name, who, change, code, message):
    case = dict(BASE, who=who, **change)
    lines = [(k, *v) if isinstance(v, list) else (k, v) for k, v in case.items() if v is not None]
    assert run_case(prog, tmp_path / "case.txt", lines) == [f"check {code} {message}"]


def test_checks_pass_in_order(prog, tmp_path):
    """The shape is looked at before the members: with both wrong the shape is what is reported."""
    case = dict(BASE, n_cols=71, signs=[0, 0, 0])
    lines = [(k, *v) if isinstance(v, list) else (k, v) for k, v in case.items()]
    assert run_case(prog, tmp_path / "case.txt", lines) == [
        f"check {ERR_ARG} score_sets: the rows have 71 columns, not n_cases + n_ctrls = 70"]
