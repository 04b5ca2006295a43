"""The wave tiles of the point back-substitution (k_backsub_points_tiles), built on the host at session set-up and exported as
mavba_debug_backsub_tiles: runs of consecutive points with at most 64 observations and at most 64 points; a point with more
than 64 observations is a tile of its own. No GPU needed."""
import numpy as np
import pytest

TILE_OBS = 64
TILE_PTS = 64


def _pt_start(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int32)


def _check(mavba, counts):
    from mavmap_amd import api
    mavba.load()
    counts = np.asarray(counts, np.int64)
    start = _pt_start(counts)
    tiles = api.backsub_tiles(start)
    again = api.backsub_tiles(start)
    assert np.array_equal(tiles, again)
    num_points = len(counts)
    if num_points == 0:
        assert len(tiles) == 0
        return tiles
    p0, npts, o0, nobs = tiles.T
    # every point exactly once, in order; the observation ranges follow pt_start and are contiguous
    assert p0[0] == 0 and np.array_equal(p0[1:], (p0 + npts)[:-1]) and p0[-1] + npts[-1] == num_points
    assert (npts >= 1).all() and (npts <= TILE_PTS).all()
    assert np.array_equal(o0, start[p0]) and np.array_equal(o0 + nobs, start[p0 + npts])
    assert ((nobs <= TILE_OBS) | (npts == 1)).all()
    # a long point stands alone
    for q in np.nonzero(counts > TILE_OBS)[0]:
        t = np.searchsorted(p0, q, side="right") - 1
        assert p0[t] == q and npts[t] == 1 and nobs[t] == counts[q]
    # greedy: a tile ends only where the next point would not fit (or is long), or at 64 points
    for t in range(len(tiles) - 1):
        nxt = counts[p0[t + 1]]
        assert npts[t] == TILE_PTS or nobs[t] + nxt > TILE_OBS or counts[p0[t]] > TILE_OBS, t
    return tiles


def test_header_declares_the_export(mavba):
    import os
    import re
    from mavmap_amd import api
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mavba_backsub_tiles.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mavba_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(api.BACKSUB_TILES_SYMBOLS) and all(hasattr(mavba.load(), n) for n in declared)
    assert not set(declared) & set(api.EXPORTED_SYMBOLS)


def test_no_points(mavba):
    assert len(_check(mavba, [])) == 0


def test_empty_points_split_by_the_point_rule(mavba):
    tiles = _check(mavba, np.zeros(1000, int))
    assert len(tiles) == 16 and (tiles[:15, 1] == 64).all() and tiles[15, 1] == 1000 - 15 * 64 and (tiles[:, 3] == 0).all()
    assert len(_check(mavba, np.zeros(1, int))) == 1


@pytest.mark.parametrize("length", [1, 63, 64, 65, 128, 129])
def test_one_track_between_six_view_points(mavba, length):
    counts = [6] * 25 + [length] + [6] * 25
    tiles = _check(mavba, counts)
    t = [i for i in range(len(tiles)) if tiles[i, 0] <= 25 < tiles[i, 0] + tiles[i, 1]][0]
    if length > 64:
        assert tuple(tiles[t, [0, 1, 3]]) == (25, 1, length)
    elif length == 64:
        assert tuple(tiles[t, [0, 1, 3]]) == (25, 1, 64)  # (fits alone, shares with nobody)
    else:
        assert tiles[t, 3] <= 64


def test_long_point_first_and_last(mavba):
    tiles = _check(mavba, [300] + [6] * 40 + [129])
    assert tuple(tiles[0]) == (0, 1, 0, 300) and tuple(tiles[-1, [1, 3]]) == (1, 129)
    tiles = _check(mavba, [65])
    assert tuple(tiles[0]) == (0, 1, 0, 65)


def test_random_arrays(mavba):
    rng = np.random.default_rng(20260)
    for k in range(40):
        n = int(rng.integers(1, 700))
        kind = k % 4
        if kind == 0:
            counts = rng.integers(0, 12, n)
        elif kind == 1:
            counts = rng.integers(0, 3, n)  # many empty points: the point rule
        elif kind == 2:
            counts = np.where(rng.random(n) < 0.05, rng.integers(60, 400, n), rng.integers(1, 20, n))
        else:
            counts = rng.integers(30, 70, n)
        _check(mavba, counts)
