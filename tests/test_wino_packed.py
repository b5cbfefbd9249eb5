"""CPU: the packed axis layout of the F(4x4,3x3) transforms (csrc/wino.h) against a brute-force layout in Python.

A dilated 3x3 convolution is the dense 3x3 convolution of a rearranged map: along an axis the sub-lattices (residues mod d) stand one after
another in residue order with ONE zero position between neighbours.  Everything here is host arithmetic (df_wino_tiles, df_wino_axis_map,
df_wino_route): no GPU."""
import ctypes

import pytest

from densefusion_amd import _lib

MAPS = [(10, 10), (15, 15), (15, 20), (20, 20), (20, 25), (25, 30), (30, 40)]          # the benchmark's seven crop sizes at 1/8 resolution
# (Cin, Cout, dilation) of the trunk's stride-1 3x3 convolutions that can leave the direct route (layer2, layer3, layer4)
LAYERS = [(128, 128, 1), (128, 256, 1), (256, 256, 1), (256, 256, 2), (256, 512, 1), (512, 512, 1), (512, 512, 4)]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    return _lib.lib()


def cdiv(a, b):
    return -(-a // b)


def brute_layout(Lx, d, m):
    """(positions, packed): the axis as a list of map coordinates / -1, strips one after another, m * tiles-per-strip positions each"""
    lattices = [list(range(r, Lx, d)) for r in range(d)]
    padded_tiles = d * cdiv(cdiv(Lx, d), m)
    strip = []
    for lat in (l for l in lattices if l):
        strip += ([-1] if strip else []) + lat
    if m == 4 and d > 1 and cdiv(len(strip), m) < padded_tiles:
        return strip + [-1] * (m * cdiv(len(strip), m) - len(strip)), True
    per = m * cdiv(cdiv(Lx, d), m)
    out = []
    for lat in lattices:
        out += lat + [-1] * (per - len(lat))
    return out, False


def tiles_py(H, W, d, m, packed=True):
    t = 1
    for Lx in (H, W):
        pos, pk = brute_layout(Lx, d, m)
        t *= len(pos) // m if packed else d * cdiv(cdiv(Lx, d), m)
    return t


@pytest.mark.parametrize("d", [1, 2, 4])
def test_axis_map_matches_the_brute_force_layout(L, d):
    n_packed = 0
    for Lx in range(1, 81):
        for m in (2, 4):
            want, packed = brute_layout(Lx, d, m)
            got = [L.df_wino_axis_map(Lx, d, m, v) for v in range(-2, len(want) + 6)]
            assert got[:2] == [-1, -1] and got[2 + len(want):] == [-1] * 6, (Lx, d, m)
            got = got[2:2 + len(want)]
            assert got == want, (Lx, d, m, got, want)
            assert sorted(y for y in got if y >= 0) == list(range(Lx))                   # a bijection with the map's points
            if not packed:
                continue
            n_packed += 1
            assert m == 4 and d > 1
            at = {y: v for v, y in enumerate(got) if y >= 0}
            val = lambda v: got[v] if 0 <= v < len(got) else -1
            for y, v in at.items():                                                      # the neighbours +-d sit at +-1; else a zero is there
                assert val(v + 1) == (y + d if y + d < Lx else -1), (Lx, d, y)
                assert val(v - 1) == (y - d if y - d >= 0 else -1), (Lx, d, y)
    assert (n_packed > 0) == (d > 1)


def test_tile_counts_and_modes(L):
    py, px = ctypes.c_int(-1), ctypes.c_int(-1)
    for d in (1, 2, 4):
        for m in (2, 4):
            for H in range(1, 81):
                for W in (1, 2, 3, 5, 9, 10, 15, 20, 25, 30, 40, 41, 80):
                    got = L.df_wino_tiles(3, H, W, d, m, ctypes.byref(py), ctypes.byref(px))
                    assert got == 3 * tiles_py(H, W, d, m), (H, W, d, m)
                    assert (py.value, px.value) == (int(brute_layout(H, d, m)[1]), int(brute_layout(W, d, m)[1]))
                    assert got <= 3 * tiles_py(H, W, d, m, packed=False)
                    if m == 2 or d == 1:
                        assert (py.value, px.value) == (0, 0)
    assert L.df_wino_tiles(1, 0, 4, 1, 4, None, None) == -1 and L.df_wino_tiles(1, 4, 4, 1, 3, None, None) == -1


def test_tiles_per_object_over_the_benchmarks_maps(L):
    """Tiles of one object of every crop size whose bucket is on the F(4x4) route: what the packed layout saves on the trunk."""
    for (ci, co, d), before, after in (((512, 512, 4), 288, 242), ((256, 256, 2), 268, 254), ((256, 256, 1), 241, 241)):
        on4 = [(H, W) for H, W in MAPS if L.df_wino_route(H, W, d, ci, co) == 4]
        assert sum(tiles_py(H, W, d, 4, packed=False) for H, W in on4) == before
        assert sum(L.df_wino_tiles(1, H, W, d, 4, None, None) for H, W in on4) == after
    assert L.df_wino_route(20, 20, 4, 512, 512) == 2            # costed on the padded count: stays on F(2x2)


def route_py(H, W, dil, Cin, Cout):
    """wino_route's cost estimate as it stood before the packed layout: tiles counted on the padded layout"""
    if Cin < 128 or Cin % 4 or Cout % 4:
        return 0
    px, cc = float(H) * W, float(Cin) * Cout
    rate = 144e12 if Cin >= 512 else 128e12 if Cin >= 256 else 100e12
    best, route = 18.0 * cc / 145e12, 0
    for m in (2, 4):
        n2 = float((m + 2) * (m + 2))
        per_px = n2 * float(dil * dil * cdiv(cdiv(H, dil), m) * cdiv(cdiv(W, dil), m)) / px
        t = 2.0 * per_px * cc / rate + 4.0 * ((1.0 + per_px) * Cin + (per_px + 2.0) * Cout) / 4.0e12
        if t < 0.9 * best:
            best, route = t / 0.9, m
    return route


def test_route_decisions_did_not_move(L):
    seen = set()
    for ci, co, d in LAYERS:
        for H in range(1, 81):
            for W in range(1, 81):
                r = L.df_wino_route(H, W, d, ci, co)
                assert r == route_py(H, W, d, ci, co), (H, W, d, ci, co)
                seen.add(r)
    assert seen == {0, 2, 4}
    assert L.df_wino_route(20, 20, 1, 64, 64) == 0
