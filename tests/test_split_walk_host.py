"""CPU: the tile walk of the split GEMM's 256 x 256 form (csrc/split_gemm.hip: split_walk on the host, split_walk_next on the device).

A launch of that form has at most one workgroup per compute unit; a workgroup keeps its XCD lane (blockIdx.x % 8) and strides statically
through the lane's sequence of tile positions, all z batches in one list.  The kernel has no counter in memory and no wait between
workgroups, so everything rests on the host's numbers (df_split_walk: grid, positions, loop trips per workgroup) agreeing with the
device's decode of a position.  ``_decode`` below is a copy of that decode (split_walk_next / split_tile_at); the walk is replayed from
the host's numbers and must
  * visit every tile (z, row tile, column tile) exactly once, and every position, padding included, exactly once;
  * keep each workgroup on the row tiles of its own XCD lane (row tile % 8 == workgroup % 8);
  * make, per workgroup, exactly the loop trips the host computed: no trip past the last position, no position left over.
Covered: tiles_m 1 .. 70, tiles_n 1 .. 9, z 1 .. 36, workgroup limits 8 .. 256 in steps of 8: every (tiles_m, tiles_n) pair with 16 of
the 1 152 (z, limit) pairs, dealt round-robin so that each (z, limit) pair meets 8 or 9 tile shapes; and the corner limits (0: one workgroup
per position; below 8; not a multiple of 8; above the position count) on a handful of shapes, those of tests/test_split_gemm_walk_gpu.py
among them."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from densefusion_amd import _lib
    return _lib.lib()


def _plan(L, tiles_m, tiles_n, z, workgroups):
    grid, total = ctypes.c_int(), ctypes.c_int()
    trips = (ctypes.c_int * 4096)()
    assert L.df_split_walk(tiles_m, tiles_n, z, workgroups, ctypes.byref(grid), ctypes.byref(total), trips, 4096) == 0
    assert grid.value <= 4096
    return grid.value, total.value, np.frombuffer(trips, dtype=np.int32, count=grid.value).astype(np.int64)


def _decode(seq, lane, tiles_m, tiles_n):
    """(z, row tile, column tile, real) of sequence number ``seq`` of XCD lane ``lane``: the device's decode."""
    seq_z = ((tiles_m + 7) >> 3) * tiles_n
    z, s = seq // seq_z, seq % seq_z
    tm, tn = (s // tiles_n) * 8 + lane, s % tiles_n
    return z, tm, tn, tm < tiles_m


def _replay(L, tiles_m, tiles_n, z, workgroups, explicit=False):
    grid, total, trips = _plan(L, tiles_m, tiles_n, z, workgroups)
    what = (tiles_m, tiles_n, z, workgroups, grid, total)
    assert total == ((tiles_m + 7) // 8) * 8 * tiles_n * z, what
    assert grid % 8 == 0 and 8 <= grid <= total, what
    if workgroups <= 0 or workgroups >= total:
        assert grid == total, what                                    # one workgroup per position
    else:
        assert grid == max(8, workgroups // 8 * 8), what              # the limit, rounded down to whole groups of 8
    b = np.arange(grid)
    lane, first, step, seqs = b % 8, b // 8, grid // 8, total // 8
    if explicit:          # the loop counts, workgroup by workgroup (the coverage below pins them as well: one trip short leaves a position out)
        assert np.array_equal(trips, [len(range(f, seqs, step)) for f in first]), what
    i = np.arange(trips.max())
    live = i[None, :] < trips[:, None]
    seq = (first[:, None] + i[None, :] * step)[live]
    wlane = np.broadcast_to(lane[:, None], live.shape)[live]
    assert seq.max() < seqs, what
    assert np.array_equal(np.bincount(seq * 8 + wlane, minlength=total), np.ones(total, dtype=np.int64)), what          # every position once
    zz, tm, tn, real = _decode(seq, wlane, tiles_m, tiles_n)
    assert zz.max() < z and tn.max() < tiles_n, what
    assert np.array_equal(tm % 8, wlane), what                                                       # a workgroup stays in its XCD lane
    tiles = ((zz * tiles_m + tm) * tiles_n + tn)[real]
    assert np.array_equal(np.bincount(tiles, minlength=z * tiles_m * tiles_n), np.ones(z * tiles_m * tiles_n, dtype=np.int64)), what   # every tile once
    return grid, trips


def test_every_tile_is_visited_once_by_a_workgroup_of_its_lane(L):
    pairs = [(z, w) for z in range(1, 37) for w in range(8, 257, 8)]
    seen, k = set(), 0
    for tiles_m in range(1, 71):
        for tiles_n in range(1, 10):
            for _ in range(16):
                z, w = pairs[k % len(pairs)]
                k += 1
                _replay(L, tiles_m, tiles_n, z, w)
                seen.add((z, w))
    assert len(seen) == len(pairs)


def test_corner_limits(L):
    for tiles_m, tiles_n, z in [(1, 1, 1), (7, 1, 1), (8, 1, 1), (9, 2, 1), (70, 9, 36), (33, 3, 16), (86, 1, 3), (129, 2, 1), (256, 1, 1)]:
        total = ((tiles_m + 7) // 8) * 8 * tiles_n * z
        for w in (0, -1, 1, 7, 8, 9, 15, 23, 250, 255, 256, 257, total - 1, total, total + 1, 4 * total):
            if min(w, total) > 4096 or (w <= 0 and total > 4096):
                continue
            grid, trips = _replay(L, tiles_m, tiles_n, z, w, explicit=True)
            if w <= 0:
                assert grid == total and (trips == 1).all()


def test_bad_arguments_are_errors(L):
    for args in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (1 << 20, 1 << 10, 1)]:
        assert L.df_split_walk(*args, 256, None, None, None, 0) != 0
        assert b"split_walk" in L.df_last_error()
