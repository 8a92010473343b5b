"""The warm-up slice left ON in front of the pruned quad kernel, and the recipe gather (k_fill_rec_segs) that runs beside
it on a stream of its own -- against the CPU oracle, every level, bit for bit.

A pruned method-1 launch whose paths0 rows come as a recipe is three things: the slice (general kernel, reads the recipe
itself), the gather (the recipe entries of every segment, next to the segment table) and the pruned launches that read
what the gather wrote.  The gather and the slice run side by side; the one gather buffer of a context is shared by
everything that follows one another on it: the chunks of a join, level 5 behind level 4, two ranks' shards, a join
launched ahead while the one before it still runs.  The quad tests (test_gpu_quad_shapes.py) switch the slice off; here
it stays on, and its length is varied: a slice's length changes which counts are looked up, never a maximum.

The network: about 120 genes and 420 signed relations, 300 + 330 patients.  Level 4 has about 1,400 uids -- one segment
each -- so the smallest slice (256 segments) leaves most of the join to the pruned launch, and a level cut into chunks of
1,024 joined paths has a slice, a gather and a short pruned launch per chunk.  A network of 40 genes has fewer level-4
uids than the smallest slice: the join fits whole into it, nothing is gathered and no pruned kernel runs.
test_inputs_score_at_every_level checks those sizes, and that every level has top_k scored paths, on the CPU."""
import numpy as np
import pytest

import oracle
from geneticscre_amd import api, dist
from geneticscre_amd.synth import make_problem
from helpers import assert_same_result

NC, NT = 300, 330
SMALLEST_SLICE = 256      # warm_segments() never gives a join less (gcre_host.hip)
LEVELS4 = (("1b", "lst1"), ("2", "lst2"), ("3", "lst3"), ("4", "lst4"))
LEVELS5 = LEVELS4 + (("5", "lst5"),)

INPUTS = {
    "k40": lambda: make_problem(120, 420, NC, NT, 40, 4, method="method1", top_k=12, seed=3),
    "tiles": lambda: make_problem(120, 420, NC, NT, 2049, 4, method="method1", top_k=12, seed=3),
    "len5": lambda: make_problem(120, 420, NC, NT, 40, 5, method="method1", top_k=12, seed=3),
    "small": lambda: make_problem(40, 110, NC, NT, 40, 4, method="method1", top_k=12, seed=1),
}
_CACHE: dict = {}


def case(name):
    """(problem, the oracle's results): computed once per session and shared."""
    if name not in _CACHE:
        p = INPUTS[name]()
        _CACHE[name] = (p, oracle.process_paths(p, order="canonical", nthreads=8))
    return _CACHE[name]


def levels_of(p):
    return LEVELS5 if p.path_length == 5 else LEVELS4


def scored_uids(p, level):
    return int((np.asarray(p.levels.uids[level].count) > 0).sum())


def quad_with_slice(monkeypatch, **env):
    """The quad form wherever it can run, recipes instead of stored planes, the slice as the library ships it."""
    monkeypatch.setenv("GCRE_NULL_KERNEL", "ie")
    monkeypatch.setenv("GCRE_IE_QUAD", "2")
    monkeypatch.setenv("GCRE_PLANES_OUT_MAX_MB", "0")
    monkeypatch.delenv("GCRE_IE_WARM", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def run_plan(p, rank=0, world=1):
    plan = api.ResidentPlan(p, device=0)
    try:
        out = plan.run(rank=rank, world=world) if world > 1 else plan.run()
        prof = dict(plan.last_profile)
    finally:
        plan.close()
    return out, prof


def check(p, got, prof, want, quad_joins=2):
    for name, lst in levels_of(p):
        assert_same_result(got[name], want[lst])
    assert prof["ie_quad_launches"] >= quad_joins, prof      # level 3 (stored planes) and level 4 (recipe), behind their slices
    assert prof["ie_lookup_tiles"] > 0, prof


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_inputs_score_at_every_level(name):
    """CPU only: every level of every input has top_k scored paths; level 4 (and 5) has more scored uids than the
    smallest slice has segments, the small network's level 4 has fewer."""
    p, want = case(name)
    for _, lst in levels_of(p):
        assert len(want[lst].scores) == p.top_k, (lst, len(want[lst].scores))
        assert np.isfinite(want[lst].scores).all() and (want[lst].all_scores > 0).sum() >= p.top_k, lst
        assert len(want[lst].null) == p.iterations
    if name == "small":
        assert 0 < scored_uids(p, "4") <= SMALLEST_SLICE, scored_uids(p, "4")
    else:
        assert scored_uids(p, "4") > 4 * SMALLEST_SLICE, scored_uids(p, "4")     # (a rank's half stays well above it)
        # chunks of 1,024 joined paths: several per level, so several gathers into the one buffer
        assert int(np.maximum(np.asarray(p.levels.uids["4"].count), 0).sum()) > 4 * 1024
    if name == "len5":
        assert scored_uids(p, "5") > SMALLEST_SLICE, scored_uids(p, "5")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["k40", "tiles"])
def test_slice_gather_and_pruned_launch(name, monkeypatch):
    """K = 40 (one tile, partly live) and K = 2,049 (two tiles): slice, gather beside it, quad kernel behind both."""
    quad_with_slice(monkeypatch)
    p, want = case(name)
    got, prof = run_plan(p)
    check(p, got, prof, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["k40", "tiles"])
def test_chunks_share_the_gather_buffer(name, monkeypatch):
    """Level 4 in chunks of 1,024 joined paths: every chunk has its own slice, gather and pruned launch, and every
    gather writes the buffer the pruned launch of the chunk before it has just read."""
    quad_with_slice(monkeypatch, GCRE_CHUNK_PATHS=1024)
    p, want = case(name)
    got, prof = run_plan(p)
    check(p, got, prof, want)


@pytest.mark.gpu
@pytest.mark.parametrize("ahead", ["default", "0"])
def test_level_5_gathers_behind_level_4(ahead, monkeypatch):
    """Path length 5: levels 4 and 5 both read level 3's recipe through the gather buffer; with the launch-ahead chain
    (the default for a plan of this size) level 5 is queued while level 4 still runs, with GCRE_AHEAD=0 it is not."""
    quad_with_slice(monkeypatch)
    if ahead == "default":
        monkeypatch.delenv("GCRE_AHEAD", raising=False)
    else:
        monkeypatch.setenv("GCRE_AHEAD", ahead)
    p, want = case("len5")
    got, prof = run_plan(p)
    check(p, got, prof, want)
    assert prof["ie_quad_launches"] >= 3, prof      # levels 3, 4 and 5


@pytest.mark.gpu
def test_two_ranks(monkeypatch):
    """Two ranks, each with its shard of every level (and its share of the slice); merged, the oracle's results.
    Half of level 3 (371 uids) fits into the smallest slice, half of level 4 (1,416 uids) does not: every rank's level 4
    has its gather and its quad launch (test_inputs_score_at_every_level checks that size)."""
    quad_with_slice(monkeypatch)
    p, want = case("k40")
    parts = []
    for rank in range(2):
        got, prof = run_plan(p, rank, 2)
        assert prof["ie_quad_launches"] >= 1 and prof["ie_lookup_tiles"] > 0, prof
        parts.append(got)
    for name, lst in (("3", "lst3"), ("4", "lst4")):
        null = np.maximum.reduce([r[name].null for r in parts])
        rows = [np.stack([r[name].scores, r[name].src, r[name].trg, r[name].cases, r[name].ctrls], axis=1) for r in parts]
        best = dist.merge_topk(np.vstack(rows), p.top_k)
        np.testing.assert_array_equal(null.view(np.uint32), want[lst].null.view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(best[:, 0], want[lst].scores, err_msg=name)


@pytest.mark.gpu
def test_no_slice_gather_on_its_own(monkeypatch):
    """GCRE_IE_WARM=0: no slice to run beside -- the gather stays on the join's stream, in front of the pruned launch."""
    quad_with_slice(monkeypatch, GCRE_IE_WARM=0)
    p, want = case("k40")
    got, prof = run_plan(p)
    check(p, got, prof, want)


@pytest.mark.gpu
def test_gather_on_the_join_stream(monkeypatch):
    """GCRE_REC_STREAM=0: the slice on, the gather in front of it on the join's stream (the A/B switch)."""
    quad_with_slice(monkeypatch, GCRE_REC_STREAM=0)
    p, want = case("k40")
    got, prof = run_plan(p)
    check(p, got, prof, want)


@pytest.mark.gpu
def test_slice_lengths_give_identical_results(monkeypatch):
    """GCRE_IE_WARM_CAP_DIV at 8, 64 and 1,000,000, GCRE_IE_WARM=256 with the cap at 64, and the cap at 1 (the slice
    then has its full 1,024 segments instead of 256: all of level 3's 371, so only level 4 has a pruned launch): the
    oracle's results in all, and identical bytes."""
    p, want = case("tiles")
    runs = []
    for env in ({"GCRE_IE_WARM_CAP_DIV": 8}, {"GCRE_IE_WARM_CAP_DIV": 64}, {"GCRE_IE_WARM_CAP_DIV": 1000000},
                {"GCRE_IE_WARM": 256, "GCRE_IE_WARM_CAP_DIV": 64}, {"GCRE_IE_WARM_CAP_DIV": 1}):
        with monkeypatch.context() as m:
            quad_with_slice(m, **env)
            got, prof = run_plan(p)
        check(p, got, prof, want, quad_joins=1 if env.get("GCRE_IE_WARM_CAP_DIV") == 1 else 2)
        runs.append(got)
    for other in runs[1:]:
        for name, _ in LEVELS4:
            for f in ("scores", "null", "cases", "ctrls", "src", "trg"):
                assert getattr(runs[0][name], f).tobytes() == getattr(other[name], f).tobytes(), (name, f)


@pytest.mark.gpu
def test_join_that_fits_into_its_slice(monkeypatch):
    """40 genes: level 4 has fewer segments than the smallest slice -- the general kernel scores it whole, no gather,
    no pruned launch (so no quad launch at any level), and the oracle's results all the same."""
    quad_with_slice(monkeypatch)
    p, want = case("small")
    got, prof = run_plan(p)
    for name, lst in LEVELS4:
        assert_same_result(got[name], want[lst])
    assert prof["ie_quad_launches"] == 0, prof
