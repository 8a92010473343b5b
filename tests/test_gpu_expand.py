"""The expansion of a join index (k_expand: joined-path ordinal -> rows of paths0 and paths1), word for word against a numpy
restatement of JoinExec::join's two nested loops, through the test-only export gcre_test_expand; and through whole joins,
chunked and sharded, against the oracle."""
import numpy as np
import pytest

import oracle
from geneticscre_amd import api
from geneticscre_amd.synth import make_problem
from helpers import assert_same_result

pytestmark = pytest.mark.gpu

TILE = 1024     # ordinals per wave and round (kExpandTile); a wave holds 64 uids at a time


@pytest.fixture(scope="module")
def ex():
    e = api.JoinExec("method2", 30, 34, 0)
    yield e
    e.close()


def index_of(counts, rng, n_rows1=None):
    """path_idx, location and signs of a join index with these paths per uid: locations anywhere in paths1 (-1 where a uid
    has no paths, as the reference leaves them), signs of both kinds for every uid row and every paths1 row."""
    counts = np.asarray(counts, np.int64)
    path_idx = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n_rows1 = n_rows1 or int(counts.max()) + 1000
    location = np.where(counts > 0, rng.integers(0, n_rows1 - counts + 1), -1).astype(np.int64)
    signs = rng.choice(np.array([-1, 1], np.int32), size=max(len(counts), n_rows1))
    return path_idx, location, signs


def expand_numpy(path_idx, location, signs, path_length, method, first, count):
    p = first + np.arange(count, dtype=np.int64)
    idx = np.searchsorted(path_idx, p, side="right") - 1     # the last uid whose first ordinal is <= p: never an empty one
    loc = location[idx] + (p - path_idx[idx])
    swap = np.zeros(count, np.uint32)
    if method == 2:
        if path_length > 3:
            sign = signs[idx]
        elif path_length < 3:
            sign = signs[loc]
        else:
            sign = np.where(signs[idx] + signs[loc] == 0, -1, 1)
        swap = (sign != 1).astype(np.uint32)
    return idx.astype(np.uint32), loc.astype(np.uint32) | (swap << np.uint32(31))


def check(ex, index, path_length, method, first, count):
    path_idx, location, signs = index
    r0, r1 = ex.test_expand(path_idx, location, signs, path_length, method, first, count)
    w0, w1 = expand_numpy(path_idx, location, signs, path_length, method, first, count)
    np.testing.assert_array_equal(r0, w0)
    np.testing.assert_array_equal(r1, w1)


EMPTY = [0] * 65
COUNTS = {
    "one_uid": [700],
    "one_uid_three_tiles": [2 * TILE + 77],
    "empty_runs": EMPTY + [1, 3, 2] * 40 + EMPTY + [5, 1] * 30 + EMPTY,
    "hub_beside_singles": [1] * 300 + [64 * 8 + 1] + [1] * 300 + [3 * TILE + 5] + [1] * 10,
    "more_uids_than_a_round": [1, 0, 2, 1] * 900,            # 3,600 uids in four tiles: sixteen rounds of 64 a tile
    "empty_run_longer_than_a_round": [2] * 10 + [0] * 600 + [3] * 10,
}


@pytest.mark.parametrize("name", sorted(COUNTS))
@pytest.mark.parametrize("method,path_length", [(1, 4), (2, 2), (2, 3), (2, 4)])
def test_expand_matches_numpy(ex, name, method, path_length):
    """Every shape of index, unsigned and at the three sign rules of the signed method (path length <, =, > 3), whole and
    from an ordinal inside a uid to one inside another."""
    rng = np.random.default_rng(len(name) * 10 + path_length)
    index = index_of(COUNTS[name], rng)
    total = int(index[0][-1])
    check(ex, index, path_length, method, 0, total)            # (the totals are no multiples of 64)
    assert total % 64
    if total > 3:
        check(ex, index, path_length, method, total // 3, total - total // 3 - 1)


def test_expand_past_the_grid(ex):
    """More tiles than the launch has waves (1,024 blocks of four): 4,097 full tiles and a partial one; hubs, singles and
    empty uids mixed."""
    rng = np.random.default_rng(5)
    counts = rng.choice(np.array([0, 1, 2, 11, 700, 5000]), p=[.3, .3, .2, .17, .02, .01], size=40_000)
    counts[-1] += max(0, 4097 * TILE + 100 - int(counts.sum()))
    index = index_of(counts, rng, n_rows1=int(counts.max()) + 50_000)
    total = int(index[0][-1])
    assert total > 4097 * TILE
    check(ex, index, 3, 2, 0, total)


@pytest.mark.parametrize("first,count", [(0, 1), (0, 64), (1, 63), (TILE - 1, 2), (TILE, TILE), (1024, 1024), (3072, 1000)])
def test_expand_windows(ex, first, count):
    """Chunks as GCRE_CHUNK_PATHS=1024 cuts them, and windows that begin and end inside a uid, on and off a tile's edge."""
    rng = np.random.default_rng(9)
    index = index_of([700, 0, 0, 1500, 1, 1, 900, 0, 2000], rng)
    check(ex, index, 3, 2, first, count)


@pytest.mark.parametrize("method", ["method1", "method2"])
def test_chunked_and_sharded_joins_match_the_oracle(method, monkeypatch):
    """Whole pipelines whose joins are expanded in chunks of 1,024 paths, and the two shards of a two-rank split (first != 0),
    against the oracle."""
    p = make_problem(70, 260, 310, 335, 130, 4, method=method, top_k=15, seed=3, threshold=0.05)
    want = oracle.process_paths(p, order="canonical")
    monkeypatch.setenv("GCRE_CHUNK_PATHS", "1024")
    got = api.process_paths(p)
    for lvl in range(1, 5):
        assert_same_result(got[f"lst{lvl}"], want[f"lst{lvl}"])
    monkeypatch.delenv("GCRE_CHUNK_PATHS")
    u = p.levels.uids["4"]
    path_idx = np.concatenate([[0], np.cumsum(np.maximum(u.count, 0))]).astype(np.int64)
    total = int(path_idx[-1])
    e = api.JoinExec(method, p.n_cases, p.n_ctrls, 0)
    try:
        for first, count in ((0, total // 2), (total // 2, total - total // 2)):
            check(e, (path_idx, np.asarray(u.location, np.int64), np.asarray(u.signs, np.int32)), 4, int(method[-1]), first, count)
    finally:
        e.close()
