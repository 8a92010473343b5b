"""Weighted sequential p-values, host side (gcre_score_sets_sequential_weighted): the rule of
csrc/gcre_seq_weighted.h -- the cut of a batch at the first left-over permutation, when the call is refused, the launches
that implies, the W32p + S dwords a permutation of a batch takes -- driven by tests/native/seq_weighted_main.cpp under the
address and undefined-behaviour sanitizers as a child process with a ``main`` of its own, against
``report.weighted_masks`` and ``report.weighted_sequential_reference``; the hash chain at permutation indices 2^32 + 5 and
2^40 - 1 against ``report._mix64`` -- the GPU tests cannot reach such r (a batch's first permutation only gets there behind
2^32 scored permutations), so the 64-bit index is held here, on the header both the kernels and this program compile; the
interface, the signatures and the ValueErrors that come before the library.  No GPU needed."""
from __future__ import annotations

import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from geneticscre_amd import api, report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "seq_weighted_main.cpp")
OK, ERR_RANGE, ERR_ARG = 0, -2, -4   # include/gcre_hip.h
WHO = "score_sets_sequential_weighted: "
TILE, FIRST_BATCH, GROWTH, BATCH_LIMIT = 512, 4096, 4, 1 << 30   # csrc/gcre_sequential.h
SIX = [1 / 3, 1, 3, 1, 1, 1]         # the odds of the six-patient cohort of tests/test_weighted_host.py


# ---- the schedule and the launches a reference implies (shared with tests/test_gpu_seq_weighted.py) ------------------------


def sequential_batch(prev, dwords, n_active, max_mb=1024.0, cap_perms=0):
    """sequential_batch of csrc/gcre_sequential.h, restated."""
    want = FIRST_BATCH if prev <= 0 else (BATCH_LIMIT if prev >= BATCH_LIMIT // GROWTH else prev * GROWTH)
    fit = max_mb * 1048576.0 / (TILE * (dwords * 4.0 + n_active / 8.0))
    tiles_fit = BATCH_LIMIT // TILE if fit >= BATCH_LIMIT // TILE else max(int(fit), 1)
    want = min(want, tiles_fit * TILE, max(BATCH_LIMIT // max(dwords, 1) // TILE, 1) * TILE)
    if cap_perms > 0:
        want = min(want, max(cap_perms // TILE, 1) * TILE)
    return max(want // TILE, 1) * TILE


def implied_batches(ref, valid, max_perms, dwords, max_mb=1024.0, cap_perms=0):
    """The batches of a weighted call whose answer is ``ref`` (``report.weighted_sequential_reference``), from the rule alone:
    [(r0, asked, scored, launches)].  Every valid set is on the active list (a NaN score never stops) until it has stopped;
    a batch that holds R is cut there and is the last: the search alone when R is its first permutation, else all four."""
    ok = np.asarray(valid) != 0
    stop_at = np.where(ok & (ref["stopped"] != 0), ref["n_perm"], np.iinfo(np.int64).max)[ok]
    R = ref["first_left_over"]
    out, r0, batch = [], 0, 0
    while r0 < max_perms and (stop_at > r0).any():
        batch = sequential_batch(batch, dwords, int((stop_at > r0).sum()), max_mb, cap_perms)
        nb = min(batch, max_perms - r0)
        if R is not None and R < r0 + nb:
            out.append((r0, nb, R - r0, 1 if R == r0 else 4))
            break
        out.append((r0, nb, nb, 4))
        r0 += nb
    return out


def implied_launches(ref, valid, max_perms, dwords, max_mb=1024.0, cap_perms=0):
    return sum(b[3] for b in implied_batches(ref, valid, max_perms, dwords, max_mb, cap_perms))


# ---- the C++ itself ---------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("seq_weighted") / "seq_weighted_main")
    # a program with a main of its own; the sanitizers' runtimes are linked statically, nothing is preloaded
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", SRC, "-o", out], check=True)
    return out


def run_case(prog, tmp_path, case):
    lines = [" ".join([k] + [str(x) for x in (v if isinstance(v, (list, tuple)) else [v])]) for k, v in case]
    path = tmp_path / "case.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout}\n{r.stderr}"
    return r.stdout.splitlines()


def hexes(odds):
    return [float(x).hex() if np.isfinite(x) else repr(float(x)) for x in odds]


def exceedance_sets(rng, perms, densities):
    """One bool row per set: e[r], with the given density of ones; None = a set that never counts (a NaN score)."""
    return [None if p is None else rng.random(perms) < p for p in densities]


def reference_of(e_rows, hits, max_perms, att):
    """``weighted_sequential_reference`` on null scores that are the exceedance bits themselves (observed score 1; NaN for a
    set that never counts)."""
    null = np.array([np.zeros(max_perms) if e is None else e[:max_perms].astype(np.float64) for e in e_rows], np.float32).reshape(len(e_rows), -1)
    obs = np.array([np.nan if e is None else 1.0 for e in e_rows])
    return report.weighted_sequential_reference(null, obs, np.ones(len(e_rows), int), hits, max_perms, att)


# name, cases, controls, odds or None (random), strata, seed, max_attempts, hits, max_perms, densities, W32p, max_mb, cap
RULE = [
    ("no left-over, one tile a batch", 7, 12, None, None, 3, 1 << 20, 5, 1800, [0.3, 0.01, 0.002, 0.0, 1.0], 4, 1024.0, 512),
    ("no left-over, three strata, the schedule", 20, 31, None, 3, 9, 1 << 20, 3, 5000, [0.2, 0.001, 0.0005, 0.0], 4, 1024.0, 0),
    ("a never-counting set runs to the end", 7, 12, None, None, 4, 1 << 20, 2, 1500, [0.5, None], 4, 1024.0, 1024),
    ("bytes bound the batch", 20, 31, None, 3, 9, 1 << 20, 3, 3000, [0.2, 0.0005, 0.0], 8, 0.01, 0),
    ("left-over behind every stop", 3, 3, SIX, None, 12, 6, 2, 3000, [0.9, 1.0, 0.7], 4, 1024.0, 512),
    ("left-over with a set still active", 3, 3, SIX, None, 12, 6, 2, 3000, [0.9, 0.0], 4, 1024.0, 512),
    ("left-over in the first batch of the schedule", 3, 3, SIX, None, 12, 8, 4, 9000, [0.001, 0.5], 4, 1024.0, 0),
    ("two strata, the second one left over", 4, 4, [1, 2, 1, 2, 1, 3, 1, 1 / 3], [0, 0, 1, 1, 1, 1, 1, 1], 5, 5, 3, 2500, [0.02, 0.0], 4, 1024.0, 512),
    ("permutation 0 left over", 3, 3, SIX, None, 12, 5, 2, 100, [1.0], 4, 1024.0, 512),
]


@pytest.mark.parametrize("case", RULE, ids=[c[0] for c in RULE])
def test_native_rule_equals_the_reference(prog, tmp_path, case):
    name, nc, nt, odds, ns, seed, cap, hits, max_perms, dens, W32p, max_mb, cap_perms = case
    rng = np.random.default_rng([41, seed, max_perms])
    n = nc + nt
    odds = np.exp(rng.uniform(-2, 2, n)) if odds is None else np.asarray(odds, float)
    strata = None if ns is None else (rng.integers(0, ns, n) if isinstance(ns, int) else np.asarray(ns))
    S = 1 if strata is None else int(strata.max()) + 1
    e_rows = exceedance_sets(rng, max_perms, dens)
    lines = [("n_cases", nc), ("n_ctrls", nt), ("seed", seed), ("max_attempts", cap), ("odds", hexes(odds)), ("hits", hits),
             ("max_perms", max_perms), ("w32p", W32p), ("max_mb", max_mb), ("cap_perms", cap_perms)]
    if strata is not None:
        lines += [("n_strata", S), ("strata", strata.tolist())]
    lines += [("set", "" if e is None else "".join("1" if b else "0" for b in e)) for e in e_rows]
    out = run_case(prog, tmp_path, lines)
    assert out[0] == "check 0 "
    assert out[1] == f"dwords {W32p + S}"                    # the mask and the accepted attempts
    thr, _ = api.weighted_thresholds(odds, nc, nt, strata)
    _, att = report.weighted_masks(thr, nc, nt, max_perms, seed, strata, max_attempts=cap)
    ref = reference_of(e_rows, hits, max_perms, att)
    R = ref["first_left_over"]
    batches = implied_batches(ref, np.ones(len(e_rows), int), max_perms, W32p + S, max_mb, cap_perms)
    got = [[int(x) for x in ln.split()[1:]] for ln in out if ln.startswith("batch ")]
    assert [(b[0], b[1], b[3]) for b in got] == [(b[0], b[1], b[2]) for b in batches], name
    assert all(b[1] % TILE == 0 or b[0] + b[1] == max_perms for b in got)
    for b in got:                                            # FIRST: the left-over column of the batch that holds R, else none
        assert b[2] == (R - b[0] if R is not None and b[0] <= R < b[0] + b[1] else -1)
    tail = out[2 + len(got):]
    assert tail[0] == f"launches {sum(b[3] for b in batches)}"
    left_s = -1 if R is None else int(np.flatnonzero(att[R] == report.WEIGHTED_NONE)[0])
    assert tail[1] == f"left_over {-1 if R is None else R} {left_s}"
    if ref["refused"]:
        assert tail[2] == (f"refused 1 {WHO}permutation {R} has no accepted attempt below max_attempts = {cap} in stratum {left_s}, and "
                           f"{ref['n_active']} sets were still active there (max_perms = {max_perms}): raise max_attempts or lower max_perms")
    else:
        assert tail[2] == "refused 0 "
    seq = [[int(x) for x in ln.split()[1:]] for ln in tail[3:]]
    assert [s[0] for s in seq] == ref["n_hit"].tolist() and [s[1] for s in seq] == ref["n_perm"].tolist()
    assert [s[2] for s in seq] == ref["stopped"].tolist()
    # what the case is there for
    if "no left-over" in name or "never-counting" in name or "bytes" in name:
        assert R is None and not ref["refused"]
    if name == "bytes bound the batch":
        assert all(b[1] == TILE for b in got[:-1]) and len(got) > 3        # 0.01 MB: one tile of (8 + 3) dwords a permutation
    if name == "no left-over, three strata, the schedule":
        assert [b[1] for b in got] == [4096, 904]
    if name == "left-over behind every stop":
        assert R is not None and R > 0 and not ref["refused"] and (ref["n_perm"] <= R).all()
    if name in ("left-over with a set still active", "two strata, the second one left over", "left-over in the first batch of the schedule"):
        assert R is not None and R > 0 and ref["refused"] and got[-1][3] == R - got[-1][0]
    if name == "two strata, the second one left over":
        assert left_s == 1
    if name == "permutation 0 left over":
        assert R == 0 and ref["refused"] and tail[0] == "launches 1" and got == [[0, 100, 0, 0, 1]]


def test_native_refusals_come_in_order(prog, tmp_path):
    base = [("n_cases", 3), ("n_ctrls", 3), ("seed", 12), ("hits", 2), ("max_perms", 10)]
    good = base + [("odds", hexes(SIX))]
    bad_odds = "the odds of patient {} (stratum 0) must be finite and >= 0, not {}"
    for extra, code, msg in [
            ([("odds", hexes([1, -1, 1, 1, 1, 1]))], ERR_ARG, bad_odds.format(1, "-1.000000")),
            ([("odds", hexes([1, 1, float("nan"), 1, 1, 1]))], ERR_ARG, bad_odds.format(2, "nan")),
            ([("odds", hexes([1, 1, 1, float("inf"), 1, 1]))], ERR_ARG, bad_odds.format(3, "inf")),
            ([("odds", hexes([1, 1, 0, 0, 0, 0]))], ERR_ARG, "stratum 0 has 2 patients with positive odds, fewer than its 3 cases"),
            ([], ERR_ARG, "NULL argument (odds)"),
            ([("odds", hexes(SIX)), ("max_attempts", 0)], ERR_ARG, "max_attempts = 0 must be at least 1"),
            ([("odds", hexes(SIX)), ("max_attempts", 2)], ERR_RANGE, "stratum 0 needs about 3 attempts per permutation, above max_attempts = 2"),
            ([("odds", hexes(SIX)), ("n_strata", 17), ("strata", [0] * 6)], ERR_ARG, "n_strata = 17 outside 1 .. GCRE_STRATA_MAX = 16")]:
        assert run_case(prog, tmp_path, base + extra) == [f"check {code} {WHO}{msg}"]
    assert run_case(prog, tmp_path, good + [("hits", 0)]) == [f"check {ERR_ARG} {WHO}hits = 0 outside 1 .. 2147483647"]
    assert run_case(prog, tmp_path, good + [("max_perms", -1)]) == [f"check {ERR_ARG} {WHO}max_perms = -1 outside 0 .. 1099511627776"]
    assert run_case(prog, tmp_path, good + [("no_seq_out", 1)]) == [f"check {ERR_ARG} {WHO}NULL argument (seq_out)"]
    # the sequential arguments are read first
    assert run_case(prog, tmp_path, base + [("hits", 0)]) == [f"check {ERR_ARG} {WHO}hits = 0 outside 1 .. 2147483647"]
    # max_perms = 0: nothing is searched
    out = run_case(prog, tmp_path, base + [("odds", hexes(SIX)), ("max_perms", 0), ("set", "")])
    assert out == ["check 0 ", "dwords 5", "launches 0", "left_over -1 -1", "refused 0 ", "seq 0 0 0"]


def test_hash_chain_at_64_bit_permutation_indices(prog, tmp_path):
    """wt_key / wt_base / wt_pair / wt_draw at r = 2^32 + 5 and 2^40 - 1 (max_perms ends at 2^40) against ``report._mix64``: the
    permutation index enters the key as 64 bits.  A key made from the low 32 bits of r would be the key of permutation 5 and
    of 2^32 - 1; the test holds them apart.  The GPU tests cannot reach such r; the kernels compile these same functions."""
    U = np.uint64
    seed = 0x1234567890ABCDEF
    asks = [(2**32 + 5, 0, 0, 0), (2**32 + 5, 3, 7, 130), (2**40 - 1, 15, 2**19, 65535), (5, 0, 0, 0), (2**32 - 1, 15, 2**19, 65535)]
    out = run_case(prog, tmp_path, [("seed", seed)] + [("chain", list(a)) for a in asks])
    assert out[0].startswith(f"check {ERR_ARG} ")            # (no odds: only the chains are printed)
    got = [[int(x, 16) for x in ln.split()[1:]] for ln in out[1:]]
    assert len(got) == len(asks)
    with np.errstate(over="ignore"):
        seed1 = report._mix64(U(seed) ^ U(report.WEIGHTED_TAG))
        for (r, s, j, c), g in zip(asks, got):
            key = report._mix64(seed1 ^ (U(0x51ED270B7F3C9A1D) * U(r + 1)))
            base = report._mix64(key ^ (U(0xD1B54A32D192ED03) * U(s + 1)))
            pair = report._mix64(base + U(j))
            u = report._mix64(pair + U(c))
            assert g == [int(key), int(base), int(pair), int(u)], (r, s, j, c)
    assert got[0][0] != got[3][0] and got[2][0] != got[4][0]
    # and the same chain is what weighted_masks walks: permutation 1 of the six patients, by its own numbers
    masks, att = report.weighted_masks([0x40000000, 0x80000000, 0xC0000000, 0x80000000, 0x80000000, 0x80000000], 3, 3, 2, 12)
    out = run_case(prog, tmp_path, [("seed", 12)] + [("chain", [1, 0, int(att[1, 0]) >> 1, c]) for c in range(6)])
    low = [int(ln.split()[4], 16) & 0xFFFFFFFF for ln in out[1:]]
    assert att[1, 0] == 1 and [c for c in range(6) if low[c] < [0x40000000, 0x80000000, 0xC0000000, 0x80000000, 0x80000000, 0x80000000][c]] \
        == np.flatnonzero(masks[1]).tolist()


# ---- the reference -----------------------------------------------------------------------------------------------------------


def test_weighted_sequential_reference():
    none = report.WEIGHTED_NONE
    e = np.zeros((4, 10), np.float32)
    e[0, [1, 3, 4]] = 1         # two hits at position 4
    e[1, [0, 6, 8]] = 1         # two hits at position 7
    e[2, [2]] = 1               # never two
    obs = np.array([1.0, 1.0, 1.0, 1.0])
    valid = np.array([1, 1, 1, 0])
    att = np.zeros((10, 2), np.uint32)
    ref = report.weighted_sequential_reference(e, obs, valid, 2, 10, att)
    plain = report.sequential_reference(e, obs, valid, 2, 10)
    assert ref["first_left_over"] is None and ref["refused"] is False and ref["n_active"] == 0
    assert all(np.array_equal(ref[k], plain[k]) and ref[k].dtype == plain[k].dtype for k in plain)
    att[8, 1] = none            # R = 8: set 2 is still active
    ref = report.weighted_sequential_reference(e, obs, valid, 2, 10, att)
    assert ref["first_left_over"] == 8 and ref["refused"] is True and ref["n_active"] == 1
    assert ref["n_perm"].tolist() == [4, 7, 8, -1] and ref["n_hit"].tolist() == [2, 2, 1, -1]
    # the sets that stopped in front of R alone: complete
    ref = report.weighted_sequential_reference(e[:2], obs[:2], valid[:2], 2, 10, att)
    assert ref["first_left_over"] == 8 and ref["refused"] is False and ref["n_perm"].tolist() == [4, 7]
    att[5, 0] = none            # R = 5: set 1 stops behind it
    ref = report.weighted_sequential_reference(e[:2], obs[:2], valid[:2], 2, 10, att)
    assert ref["first_left_over"] == 5 and ref["refused"] is True and ref["n_active"] == 1 and ref["n_perm"].tolist() == [4, 5]
    # n_perm == R is in front of R: the h-th hit is permutation R - 1
    att[:] = 0
    att[4, 0] = none
    ref = report.weighted_sequential_reference(e[:1], obs[:1], valid[:1], 2, 10, att)
    assert ref["first_left_over"] == 4 and ref["refused"] is False and ref["n_perm"].tolist() == [4]
    # a left-over permutation at or beyond max_perms is none; a NaN score never stops
    assert report.weighted_sequential_reference(e[:1], obs[:1], valid[:1], 2, 4, att)["first_left_over"] is None
    ref = report.weighted_sequential_reference(e[:1], [np.nan], valid[:1], 2, 10, att)
    assert ref["refused"] is True and ref["n_hit"].tolist() == [0] and ref["n_perm"].tolist() == [4]
    att[0, 0] = none
    ref = report.weighted_sequential_reference(e[:1], obs[:1], valid[:1], 2, 10, att)
    assert ref["first_left_over"] == 0 and ref["refused"] is True and ref["n_perm"].tolist() == [0]
    assert report.weighted_sequential_reference(e[3:], obs[3:], valid[3:], 2, 10, att)["refused"] is False     # no valid set
    with pytest.raises(ValueError, match="rows of attempts"):
        report.weighted_sequential_reference(e, obs, valid, 2, 10, att[:9])


# ---- the interface ---------------------------------------------------------------------------------------------------------


def test_interface_is_declared():
    header = open(os.path.join(ROOT, "include", "gcre_hip.h")).read()
    assert re.search(r"#define GCRE_ABI_VERSION 4\b", header)      # additions only
    flat = " ".join(re.sub(r"/\*.*?\*/", " ", header, flags=re.S).split())
    assert ("int gcre_score_sets_sequential_weighted(gcre_ctx* ctx, const gcre_set_input* in, uint64_t seed, const double* odds, "
            "const int32_t* stratum, int n_strata, int64_t max_attempts, int64_t h, int64_t max_perms, gcre_set_score* out, "
            "int64_t cap, int64_t* n_out, gcre_seq_score* seq_out );") in flat
    prose = " ".join(header.split()).replace(" * ", " ")
    assert "Not built: weighted draws in the subsample set scores" in prose
    assert "weighted draws in the sequential and subsample" not in prose
    assert "gcre_score_sets_sequential_weighted" in api.EXPORTS
    assert set(re.findall(r"\b(gcre_[a-z0-9_]+)\s*\(", header)) == set(api.EXPORTS)
    parent, needs, _, binds = api._FEATURES["sequential_weighted"]
    assert parent == "sequential" and set(needs) == set(binds) == {"gcre_score_sets_sequential_weighted"}
    assert len(binds["gcre_score_sets_sequential_weighted"][1]) == 13
    from geneticscre_amd import build
    assert "gcre_seq_weighted.hip" in build.SOURCES and "gcre_seq_weighted.h" in build.HEADERS
    csrc = os.path.join(ROOT, "geneticscre_amd", "csrc")
    kernels = open(os.path.join(csrc, "gcre_kernels.h")).read()
    assert all(x in kernels for x in ("struct SeqWeightedArgs", "launch_seq_weighted_search(", "launch_seq_weighted_write("))
    lib = api._feature_lib("sequential_weighted")           # loads without a GPU
    assert lib.gcre_abi_version() == 4 and hasattr(lib, "gcre_score_sets_sequential_weighted")
    # the draw is gcre_weighted.h's: no hash constant is restated, and the kernels that were there are untouched
    for name in ("gcre_seq_weighted.h", "gcre_seq_weighted.hip"):
        text = open(os.path.join(csrc, name)).read().lower()
        assert not any(k in text for k in ("9e3779b9", "bf58476d", "94d049bb", "51ed270b", "d1b54a32", "77656967")), name
    new = open(os.path.join(csrc, "gcre_seq_weighted.hip")).read()
    assert "k_seq_weighted_search" in new and "k_seq_weighted_write" in new and "atomicMin" in new
    for name in ("gcre_weighted.hip", "gcre_sequential.hip", "gcre_frontend.hip"):
        assert "k_seq_weighted" not in open(os.path.join(csrc, name)).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.24" in design and "k_seq_weighted_search" in design and "k_seq_weighted_write" in design
    for doc in ("README.md", "INTEGRATION.md"):
        assert "weighted_sequential_tests" in open(os.path.join(ROOT, doc)).read()


def test_signatures():
    w = inspect.signature(api.JoinExec.weighted_sequential_tests).parameters
    assert list(w) == ["self", "sets", "rows", "signs", "odds", "hits", "max_perms", "seed", "strata", "max_attempts"]
    assert [w[k].default for k in list(w)[3:]] == [None, None, 20, 10**6, 0, None, 1 << 20]
    r = inspect.signature(report.weighted_sequential_reference).parameters
    assert list(r) == ["null", "obs", "valid", "hits", "max_perms", "attempts"]
    sp = inspect.signature(report.score_paths).parameters
    names = list(sp)
    assert names[-1] == "family_inference" and names[-3:-1] == ["case_odds", "sequential_weighted"]
    assert sp["sequential_weighted"].default is False
    doc = " ".join(report.score_paths.__doc__.split())
    assert "The switch is explicit because of what it costs" in doc and "sqrt(2 pi V) attempts over the whole stratum" in doc
    # what was pinned before stays
    st = inspect.signature(api.JoinExec.sequential_tests).parameters
    assert list(st) == ["self", "sets", "rows", "signs", "hits", "max_perms", "seed", "strata"]
    assert list(inspect.signature(report.sequential_reference).parameters) == ["null", "obs", "valid", "hits", "max_perms"]


def test_value_errors_come_before_the_library(monkeypatch):
    ex = api.JoinExec.__new__(api.JoinExec)
    ex.num_cases, ex.num_ctrls, ex.iters = 3, 2, 0
    monkeypatch.setattr(api, "_feature_lib", lambda name: None)
    rows = np.zeros((1, 5), np.int8)
    with pytest.raises(ValueError, match="odds: one value per patient is required"):
        api.JoinExec.weighted_sequential_tests(ex, [[0]], rows)
    with pytest.raises(ValueError, match=r"odds: one value per patient \(5\), not 4"):
        api.JoinExec.weighted_sequential_tests(ex, [[0]], rows, odds=np.ones(4))
    with pytest.raises(ValueError, match=r"strata: one id per patient \(5\), not 3"):
        api.JoinExec.weighted_sequential_tests(ex, [[0]], rows, odds=np.ones(5), strata=[0, 1, 0])
    # score_paths: the three refusals, before anything is opened
    with pytest.raises(ValueError, match=r"^case_odds: sequential p-values draw their own uniform masks; sequential_weighted=True"):
        report.score_paths(["A"], ["A"], rows, 3, 2, case_odds=np.ones(5), sequential=100)
    with pytest.raises(ValueError, match="sequential_weighted=True needs case_odds and sequential > 0"):
        report.score_paths(["A"], ["A"], rows, 3, 2, sequential=100, sequential_weighted=True)
    with pytest.raises(ValueError, match="sequential_weighted=True needs case_odds and sequential > 0"):
        report.score_paths(["A"], ["A"], rows, 3, 2, case_odds=np.ones(5), sequential_weighted=True)
