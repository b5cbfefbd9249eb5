"""GPU: the customCAD triangle rasteriser -- ``df_cad_render_mesh`` against its numpy restatement (tests/cad_raster_np.py) bit for bit,
its argument errors, then tools/render_cad_dataset.py --raster mesh: the tree it writes goes through the unchanged loader, whose clouds
must lie on the rendered icosphere where the records say it is, and through tools/train.py --dataset cad and tools/eval_cad.py."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import cad_raster_np as mnp
import cad_render_np as rnp
import fabricate_cad as fab
from densefusion_amd import synth

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROJ = np.array(fab.PROJ[1])
IH, IW = 37, 53                     # no multiple of a wave; an odd pixel count

# The camera of the small scene.  With the identity pose at t_z = -4096, a vertex with m_z = 0 has c_3 = 4096 and lands on the node
# (r, q) when m_x = 8 (2 q - IW) and m_y = 8 (IH - 2 r): ndc_x = fl(P00 * 80 (2 q - IW)) / 4096 is (2 q - IW) / IW to one rounding, and
# the two roundings of V4 bring sx back to q exactly for the nodes the scene uses (test_the_fixture_has_its_cases checks each).
NODE_PROJ = np.array([[4096.0 / (80 * IW), 0, 0, 0], [0, 4096.0 / (80 * IH), 0, 0], [0, 0, 0.5, 3000.0], [0, 0, -1.0, 0]])


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _pose(R, t):
    return np.concatenate([np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)[:, None]], axis=1)


def _on(q, r, z=0.0):
    """model coordinates that frame 0 of the small scene puts at column q, row r (exactly, for integers and z = 0) and depth -4096 + 10 z"""
    s = (4096.0 - 10.0 * z) / 4096.0
    return [8.0 * (2 * q - IW) * s, 8.0 * (IH - 2 * r) * s, z]


def small_scene():
    """About 300 triangles, four poses, K = 3 holes; code limits at |z| = 2000 and 6000.  Returns (vertices, colours, triangles, poses,
    holes, parts): parts names the triangle indices of each crafted case.
    frame 0: no rotation at z = -4096, where the crafted vertices sit on their nodes; frame 1: turned, shifted, reaching past the far
    code limit; frame 2: around the camera: vertices behind it and before the near code limit; frame 3: all behind."""
    rng = np.random.default_rng(41)
    verts, tris, parts = [], [], {}

    def add(name, vs, ts):
        base = len(verts)
        verts.extend(vs)
        parts[name] = list(range(len(tris), len(tris) + len(ts)))
        tris.extend([[base + i if i >= 0 else -i - 1 for i in t] for t in ts])      # a negative entry -k-1 names the absolute vertex k
        return base

    # a 4 x 4 lattice of vertices on nodes, 18 triangles: shared edges (horizontal, vertical, diagonal) and corners lie on nodes
    lat_q, lat_r = (20, 24, 28, 32), (4, 8, 12, 16)
    grid = lambda i, j: i * 4 + j
    quads = [(grid(i, j), grid(i + 1, j), grid(i + 1, j + 1), grid(i, j + 1)) for i in range(3) for j in range(3)]
    add("lattice", [_on(q, r) for r in lat_r for q in lat_q], [[a, b, c] for a, b, c, d in quads] + [[a, c, d] for a, b, c, d in quads])
    # a fan of seven triangles around the node (18, 40), the rim off the nodes and at its own depths
    ang = np.linspace(0, 2 * np.pi, 8)[:-1] + 0.3
    add("fan", [_on(40, 18)] + [_on(40 + 6.3 * np.cos(a), 18 + 5.1 * np.sin(a), 4.0 * k - 10.0) for k, a in enumerate(ang)],
        [[0, 1 + k, 1 + (k + 1) % 7] for k in range(7)])
    # zero area: three lattice vertices of one row; a repeated index, twice
    add("zero_area", [], [[-1, -2, -3], [-2, -4, -3]])
    add("repeated", [], [[-1, -1, -6], [-6, -11, -6]])
    # slivers that cover no node: between two columns, between two rows
    add("slivers", [_on(36.2, 3.0), _on(36.8, 9.0), _on(36.6, 14.5), _on(28.0, 30.3), _on(36.0, 30.6), _on(45.0, 30.4)], [[0, 1, 2], [3, 4, 5]])
    # two copies of one triangle with different colours, nearest to the camera of frame 0
    tw = [_on(25.5, 22.3, 150.0), _on(34.2, 24.1, 150.0), _on(29.7, 33.6, 150.0)]
    add("twins", tw + tw, [[0, 2, 1], [3, 5, 4]])
    # one triangle larger than the frame on all four sides, behind the rest
    add("huge", [_on(-400.0, -300.0, -185.0), _on(500.0, -280.0, -185.0), _on(30.0, 700.0, -185.0)], [[0, 2, 1]])
    # one corner behind the camera of frame 0
    add("behind", [_on(5.0, 30.0, 20.0), _on(12.0, 33.0, 20.0), [10.0, -100.0, 500.0]], [[0, 1, 2]])
    # reaching past the far code limit (|z| > 6000) and before the near one (|z| < 2000): cut per node
    add("far", [_on(44.0, 2.0, -150.0), _on(51.0, 4.0, -150.0), _on(47.0, 12.0, -250.0)], [[0, 2, 1]])
    add("near", [_on(2.0, 24.0, 180.0), _on(9.0, 26.0, 180.0), _on(4.0, 35.0, 240.0)], [[0, 2, 1]])
    # a soup of both windings and all sizes over shared vertices
    # (220 between near neighbours: a few nodes each; 30 over random triples: tens to hundreds of nodes)
    n_soup = 150
    soup = np.stack([rng.uniform(-420, 420, n_soup), rng.uniform(-300, 300, n_soup), rng.uniform(-150, 150, n_soup)], axis=1)
    near = np.argsort(((soup[:, None, :2] - soup[None, :, :2]) ** 2).sum(axis=2), axis=1)[:, 1:9]
    first = rng.integers(0, n_soup, 220)
    pick = rng.integers(0, 8, (220, 2))
    local = np.stack([first, near[first, pick[:, 0]], near[first, pick[:, 1]]], axis=1)
    add("soup", soup.tolist(), local.tolist() + rng.integers(0, n_soup, (30, 3)).tolist())
    verts = np.array(verts, dtype=np.float32)
    tris = np.array(tris, dtype=np.int32)
    col = rng.integers(0, 256, (len(verts), 3), dtype=np.uint8)
    rot = Rotation.from_quat(rng.normal(size=(2, 4))).as_matrix()
    poses = np.stack([_pose(np.eye(3), [0, 0, -4096.0]), _pose(rot[0], [500.0, -300.0, -5000.0]), _pose(rot[1], [100.0, 50.0, -1500.0]),
                      _pose(rot[0], [0, 0, 9000.0])])
    s0 = int(tris[parts["soup"][0], 0])
    hole_idx = np.array([[15, s0 + 7, -1], [-1, 3, s0 + 20], [-1, -1, -1], [0, -1, -1]], dtype=np.int32)      # 15: a lattice corner
    hole_r = np.array([[0.0, 80.0, 7.0], [9.0, 0.0, 150.0], [1.0, 2.0, 3.0], [50.0, 0.0, 0.0]])
    return verts, col, tris, poses, (hole_idx, hole_r), parts


def _gpu(verts, col, tris, poses, holes, dims, cull, mask_mode, proj=NODE_PROJ):
    from densefusion_amd.lib import preprocess as pp
    up = lambda a: torch.from_numpy(a).cuda()
    out = pp.cad_render_mesh(up(verts), up(col), up(tris), poses, 10.0, proj, dims, holes=holes, cull=cull, mask_mode=mask_mode)
    return tuple(o.cpu().numpy() for o in out)


def _same(got, want):
    for name, g, w in zip(("rgb", "depth", "mask", "stats"), got, want[:4]):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


def _nodes(v, tri, neg):
    """T4..T6 of one triangle whatever its winding: (covered [IH,IW] bool, code [IH,IW] before the limits)"""
    py, px = np.arange(IH, dtype=np.float64)[:, None], np.arange(IW, dtype=np.float64)[None, :]
    w = mnp.weights(tri[0], tri[1], tri[2], neg, v["sx"], v["sy"], px, py)
    W = (w[0] + w[1]) + w[2]
    cov = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0) & (W > 0)
    with np.errstate(all="ignore"):
        code = np.rint(65534.0 * (((w[0] * v["d"][tri[0]] + w[1] * v["d"][tri[1]]) + w[2] * v["d"][tri[2]]) / W))
    return cov, code, w


def test_the_fixture_has_its_cases():
    """What the bit-equality test below is meant to cover is really in the scene (restatement only; no device work)."""
    verts, col, tris, poses, holes, parts = small_scene()
    assert 280 <= len(tris) <= 320
    v = mnp.project_vertices(verts, poses[0], 10.0, None, None, NODE_PROJ, IH, IW)
    area = lambda t: float(mnp.edge(tris[t, 0], tris[t, 1], v["sx"], v["sy"], v["sx"][tris[t, 2]], v["sy"][tris[t, 2]]))
    # vertices exactly on nodes: the lattice and the fan's centre
    lat = np.unique(tris[parts["lattice"]])
    assert len(lat) == 16 and (v["sx"][lat] == np.tile([20, 24, 28, 32], 4)).all() and (v["sy"][lat] == np.repeat([4, 8, 12, 16], 4)).all()
    c = tris[parts["fan"][0], 0]
    assert v["sx"][c] == 40 and v["sy"][c] == 18 and all(tris[t, 0] == c for t in parts["fan"]) and len(parts["fan"]) == 7
    # w == 0 on shared edges and corners: nodes of the lattice where one weight, and where two weights, vanish exactly
    one, two = 0, 0
    for t in parts["lattice"]:
        cov, code, w = _nodes(v, tris[t], area(t) < 0)
        zeros = (w[0] == 0).astype(int) + (w[1] == 0) + (w[2] == 0)
        one, two = one + int((cov & (zeros == 1)).sum()), two + int((cov & (zeros == 2)).sum())
    assert one >= 50 and two >= 30, (one, two)
    # zero area and repeated indices
    assert all(area(t) == 0 for t in parts["zero_area"]) and all(len(set(tris[t])) == 3 for t in parts["zero_area"])
    assert all(len(set(tris[t])) == 2 for t in parts["repeated"])
    # slivers: a non-empty bounding range on one axis, no covered node
    for t in parts["slivers"]:
        assert area(t) != 0 and not _nodes(v, tris[t], area(t) < 0)[0].any()
    # both windings
    signs = np.array([area(t) for t in parts["soup"] if len(set(tris[t])) == 3])
    assert (signs < 0).sum() >= 50 and (signs > 0).sum() >= 50
    # larger than the frame on all four sides: every node is covered (the cooperative path: far more nodes than a lane walks)
    h = parts["huge"][0]
    assert area(h) < 0 and _nodes(v, tris[h], True)[0].all()
    # a corner behind the camera
    assert v["behind"][tris[parts["behind"][0]]].sum() == 1
    # the code limits cut the far and the near triangle per node: some covered nodes within the limits, some past them
    for name in ("far", "near"):
        t = parts[name][0]
        cov, code, _ = _nodes(v, tris[t], area(t) < 0)
        inside = (code >= 0) & (code <= 65534)
        assert area(t) < 0 and (cov & inside).sum() >= 5 and (cov & ~inside).sum() >= 5, name
    assert (_nodes(v, tris[parts["far"][0]], True)[1] > 65534).any() and (_nodes(v, tris[parts["near"][0]], True)[1] < 0).any()
    hidx, hr = holes
    assert (hr[hidx >= 0] == 0).any() and (hr[hidx >= 0] > 0).any()
    for cull in (0, 1):
        rgb, depth, mask, stats, winner = mnp.render(verts, col, tris, poses, 10.0, holes, NODE_PROJ, IH, IW, cull, 0)
        assert (stats[3] == 0).all() and (depth[3] == 65535).all() and (mask[3] == 0).all() and (rgb[3] == 130).all()
        assert (stats[:3, 0] > 0).all()
        # the twins: the lower index wins pixels, its copy none; nothing dropped wins anything
        assert (winner[0] == parts["twins"][0]).sum() >= 20 and not (winner[0] == parts["twins"][1]).any()
        for name in ("zero_area", "repeated", "slivers", "behind"):
            assert not np.isin(winner[0], parts[name]).any(), name
        # the far and near triangles show where nothing is in front of them, and the huge one fills the rest of frame 0
        assert np.isin(winner[0], parts["far"]).any() and np.isin(winner[0], parts["near"]).any()
        assert (winner[0] == h).any() and stats[0, 0] == IH * IW
        # hole 15 (radius 0) removed the lattice's last corner and with it the two triangles of the last quad
        assert not np.isin(winner[0], [t for t in parts["lattice"] if 15 in tris[t]]).any()
        assert np.isin(winner[0], [t for t in parts["lattice"] if 15 not in tris[t]]).any()
    a = mnp.render(verts, col, tris, poses[:1], 10.0, None, NODE_PROJ, IH, IW, 0, 0)
    b = mnp.render(verts, col, tris, poses[:1], 10.0, None, NODE_PROJ, IH, IW, 1, 0)
    assert a[3][0, 1] > b[3][0, 1] and not np.array_equal(a[1], b[1]), "culling matters in an open soup"


@gpu
@pytest.mark.parametrize("mask_mode", [0, 1])
@pytest.mark.parametrize("cull", [0, 1])
def test_raster_equals_the_restatement_bit_for_bit(cull, mask_mode):
    _dev()
    verts, col, tris, poses, holes, _ = small_scene()
    _same(_gpu(verts, col, tris, poses, holes, (IH, IW), cull, mask_mode), mnp.render(verts, col, tris, poses, 10.0, holes, NODE_PROJ, IH, IW, cull, mask_mode))


@gpu
def test_raster_without_holes_and_frame_independence():
    """K = 0 (NULL hole arrays); two identical calls give identical bytes; frame 2 of the F = 4 call equals the F = 1 call of its pose."""
    _dev()
    verts, col, tris, poses, holes, _ = small_scene()
    a = _gpu(verts, col, tris, poses, None, (IH, IW), 0, 0)
    _same(a, mnp.render(verts, col, tris, poses, 10.0, None, NODE_PROJ, IH, IW, 0, 0))
    b = _gpu(verts, col, tris, poses, holes, (IH, IW), 0, 0)
    c = _gpu(verts, col, tris, poses, holes, (IH, IW), 0, 0)
    for x, y in zip(b, c):
        assert x.tobytes() == y.tobytes()
    one = _gpu(verts, col, tris, poses[2:3], (holes[0][2:3], holes[1][2:3]), (IH, IW), 0, 0)
    for x, y in zip(b, one):
        assert np.array_equal(x[2], y[0])


@gpu
def test_many_holes_take_several_raster_launches():
    """K = 50: the hole records travel as launch arguments, 128 a launch, so the four frames take two raster launches (frames 0-1, 2-3)."""
    _dev()
    verts, col, tris, poses, _, _ = small_scene()
    rng = np.random.default_rng(3)
    hole_idx = rng.integers(-1, len(verts), (4, 50)).astype(np.int32)
    hole_idx[rng.random((4, 50)) < 0.5] = -1
    holes = (hole_idx, rng.uniform(0.0, 30.0, (4, 50)))
    want = mnp.render(verts, col, tris, poses[[0, 1, 0, 2]], 10.0, holes, NODE_PROJ, IH, IW, 0, 1)
    assert (want[3][:3, 0] > 0).all() and not np.array_equal(want[1][0], want[1][2])          # frames 0 and 2: one pose, different holes
    _same(_gpu(verts, col, tris, poses[[0, 1, 0, 2]], holes, (IH, IW), 0, 1), want)


def _box(lo, hi):
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    v = np.array([[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0], [x0, y0, z1], [x1, y0, z1], [x1, y1, z1], [x0, y1, z1]], dtype=np.float64)
    f = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5], [2, 3, 7], [2, 7, 6], [3, 0, 4], [3, 4, 7]])
    return v, f                                               # counter-clockwise seen from outside


@gpu
def test_full_size_frames_with_large_and_small_triangles():
    """520 x 1109, F = 2: an icosphere of subdivision 5 (20 480 triangles of a few nodes each, walked by their lanes; the second frame's
    sphere is cut by the right edge) and behind it a 12-triangle box over more than a quarter of the frame (the cooperative path, and
    more pixels than threads in the resolve and mask passes); one hole each."""
    _dev()
    sv, sf = mnp.icosphere(5, 60.0)
    bv, bf = _box([-240.0, -110.0, -160.0], [240.0, 110.0, -120.0])
    verts = np.concatenate([sv, bv]).astype(np.float32)
    tris = np.concatenate([sf, bf + len(sv)]).astype(np.int32)
    col = np.random.default_rng(8).integers(0, 256, (len(verts), 3), dtype=np.uint8)
    poses = np.stack([_pose(np.eye(3), [300.0, -200.0, -3000.0]), _pose(np.eye(3), [2150.0, 100.0, -2700.0])])
    holes = (np.array([[11], [700]], dtype=np.int32), np.array([[25.0], [12.0]]))
    want = mnp.render(verts, col, tris, poses, 10.0, holes, PROJ, 520, 1109, 1, 0)
    box_pixels = np.isin(want[4][0], np.arange(len(sf), len(tris))).sum()
    assert box_pixels >= 520 * 1109 // 4 and want[3][1, 5] == 1108 and (want[3][:, 1] > 5000).all()
    assert np.isin(want[4][1], np.arange(len(sf))).sum() > 10000
    _same(_gpu(verts, col, tris, poses, holes, (520, 1109), 1, 0, proj=PROJ), want)


@gpu
def test_argument_errors_write_nothing():
    _dev()
    from densefusion_amd import _lib
    L = _lib.lib()
    V, T, F, K = 64, 40, 2, 2
    dev = torch.device("cuda")
    vts = torch.rand(V, 3, device=dev)
    col = torch.zeros(V, 3, dtype=torch.uint8, device=dev)
    tri = torch.randint(0, V, (T, 3), dtype=torch.int32, device=dev)
    pose = torch.from_numpy(np.stack([_pose(np.eye(3), [0, 0, -4000.0])] * F)).to(dev)
    outs = dict(rgb=torch.full((F, IH, IW, 3), 7, dtype=torch.uint8, device=dev), depth=torch.full((F, IH, IW), 7, dtype=torch.int16, device=dev),
                mask=torch.full((F, IH, IW), 7, dtype=torch.int16, device=dev), stats=torch.full((F, 6), 7, dtype=torch.int32, device=dev))
    need = L.df_cad_render_mesh_scratch_bytes(F, IH, IW, V, T)
    assert need == F * IH * IW * 8
    for bad in ((0, IH, IW, V, T), (F, 0, IW, V, T), (F, IH, -1, V, T), (F, IH, IW, 0, T), (F, IH, IW, V, 0)):
        assert L.df_cad_render_mesh_scratch_bytes(*bad) == 0
    scratch = torch.full((need + 8,), 7, dtype=torch.uint8, device=dev)
    hole_idx, hole_r = np.full((F, K), -1, dtype=np.int32), np.zeros((F, K))
    good = dict(vertices=vts.data_ptr(), colors=col.data_ptr(), V=V, triangles=tri.data_ptr(), T=T, pose=pose.data_ptr(), model_scale=10.0,
                hole_idx=hole_idx.ctypes.data, hole_r=hole_r.ctypes.data, K=K, proj=None, F=F, IH=IH, IW=IW, cull=1, mask_mode=0,
                rgb=outs["rgb"].data_ptr(), depth=outs["depth"].data_ptr(), mask=outs["mask"].data_ptr(), stats=outs["stats"].data_ptr(),
                scratch=scratch.data_ptr(), scratch_bytes=need, stream=_lib.current_stream())

    def call(**kw):
        proj = kw.pop("proj", PROJ)
        pm = None if proj is None else np.ascontiguousarray(proj, dtype=np.float64)
        a = dict(good, **kw)
        a["proj"] = None if pm is None else pm.ctypes.data
        return L.df_cad_render_mesh(*[a[k] for k in good])

    bad_holes = hole_idx.copy()
    bad_holes[1, 1] = V
    row2, row3, row3b = PROJ.copy(), PROJ.copy(), PROJ.copy()
    row2[2, 0], row3[3, 2], row3b[3, 3] = 0.1, -2.0, 1.0
    cases = [dict(vertices=None), dict(colors=None), dict(triangles=None), dict(pose=None), dict(proj=None), dict(rgb=None), dict(depth=None),
             dict(mask=None), dict(stats=None), dict(scratch=None), dict(hole_idx=None), dict(hole_r=None), dict(cull=-1), dict(cull=2),
             dict(mask_mode=2), dict(mask_mode=-1), dict(hole_idx=bad_holes.ctypes.data), dict(scratch_bytes=need - 1),
             dict(scratch=scratch.data_ptr() + 4, scratch_bytes=need + 4), dict(V=0), dict(T=0), dict(V=-5), dict(T=-1), dict(F=0),
             dict(F=65536), dict(IH=0), dict(IW=0), dict(K=-1), dict(K=129)]
    for kw in cases:
        assert call(**kw) == -1, kw                                       # DF_ERR_ARG
        assert len(L.df_last_error()) > 10, kw
    for pm in (row2, row3, row3b):
        assert call(proj=pm) == -1 and b"projection" in L.df_last_error()
    torch.cuda.synchronize()
    for name, t in list(outs.items()) + [("scratch", scratch)]:
        assert bool((t == 7).all()), name
    assert call() == 0 and call(cull=0, mask_mode=1) == 0 and call(K=0, hole_idx=None, hole_r=None) == 0
    torch.cuda.synchronize()
    assert not bool((outs["stats"] == 7).any())


# ---- the tool, the loader, the trainer ---------------------------------------------------------------------------------------------
TREE_DIMS = (96, 144)


@pytest.fixture(scope="module")
def mesh_model(tmp_path_factory):
    """The icosphere of subdivision 4, radius 60 file units, as a coloured binary PLY."""
    root = tmp_path_factory.mktemp("mesh_model")
    v, f = mnp.icosphere(4, 60.0)
    v = v.astype(np.float32)
    col = np.random.default_rng(12).integers(0, 256, (len(v), 3), dtype=np.uint8)
    return mnp.write_mesh_ply(root / "icosphere.ply", v, f, col), v, f, root


@pytest.fixture(scope="module")
def rendered_tree(mesh_model):
    """tools/render_cad_dataset.py --raster mesh on the icosphere: one object, 24 frames of 96 x 144."""
    _dev()
    from densefusion_amd.datasets.customCAD.dataset import read_ply
    path, v, f, root = mesh_model
    pm = rnp.write_proj(root / "proj_in.txt", fab.PROJ[1])
    tree = str(root / "tree")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render_cad_dataset.py"), "--model", path, "--output_root", tree, "--object", "1",
                        "--frames", "24", "--proj_mat", pm, "--height", "96", "--width", "144", "--min_pixels", "200", "--raster", "mesh",
                        "--chunk", "16"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "frames written: 24" in r.stdout and "device time per rendered view" in r.stdout and "%d triangles" % len(f) in r.stdout
    mv, mf = read_ply(os.path.join(tree, "models", "obj_01.ply"))
    assert np.array_equal(mv.astype(np.float32), v) and np.array_equal(mf, f)
    return tree


@gpu
def test_mesh_tree_through_the_loader(rendered_tree, mesh_model):
    """The cloud of every training frame lies on the rendered icosphere where the record says it is.  The surface is the mesh, not the
    sphere: a facet lies inside the sphere of radius 600 by up to its sagitta, 600 minus the smallest distance of a triangle's plane from
    the centre.  So every cloud point lies within the bound of test_rendered_tree_through_the_loader (half a grid step and half a depth
    code at its own depth, + 1e-3 for the loader's float32) of the shell between radius 600 - sagitta and 600."""
    from densefusion_amd.datasets.customCAD import render as cr
    from densefusion_amd.datasets.customCAD.dataset import PoseDataset
    tree = rendered_tree
    _, v, f, _ = mesh_model
    a, b, c = (v[f[:, k]].astype(np.float64) * 10.0 for k in range(3))
    nrm = np.cross(b - a, c - a)
    plane = np.abs((nrm * a).sum(axis=1)) / np.linalg.norm(nrm, axis=1)
    sagitta = 600.0 - plane.min()
    assert 0.5 < sagitta < 5.0, sagitta
    sub = os.path.join(tree, "data", "01")
    train = [int(x) for x in open(os.path.join(sub, "train.txt")).read().split()]
    test = [int(x) for x in open(os.path.join(sub, "test.txt")).read().split()]
    assert len(train) == 19 and len(test) == 5 and sorted(train + test) == list(range(24))
    np.random.seed(1)
    ds = PoseDataset("train", 500, False, tree, 0.0, False)
    assert len(ds) == 19 and ds.udp[1].image_dims == TREE_DIMS
    worst = [0.0, 0.0]
    for i, item in enumerate(ds.batch(list(range(len(ds))))):
        cloud, choose, img, target, model_points, idx = item
        assert cloud.dim() == 2 and tuple(cloud.shape) == (500, 3), "the sentinel"
        R, t_cam = cr.transform_to_pose(*ds.meta[1][ds.list_meta[i] + 1])
        p = cloud.double().cpu().numpy() * 10000
        bx, by, bz = rnp.grid_bounds(p[:, 2], fab.PROJ[1], *TREE_DIMS)
        dist = np.linalg.norm(p - t_cam, axis=1)
        off = np.maximum(np.maximum(dist - 600.0, (600.0 - sagitta) - dist), 0.0)
        bound = np.sqrt(bx * bx + by * by + bz * bz) * (1 + 1e-6) + 1e-3
        worst[0] = max(worst[0], float((off / bound).max()))
        assert (off <= bound).all(), (i, float((off / bound).max()))
        # the model points are drawn from the mesh by area: on the facets, hence in the same shell around the record's t_cam
        tg = np.linalg.norm(target.double().cpu().numpy() * 10000 - t_cam, axis=1)
        worst[1] = max(worst[1], float(np.maximum(tg - 600.0, (600.0 - sagitta) - tg).max()))
        assert (tg <= 600.0 + 1e-2).all() and (tg >= 600.0 - sagitta - 1e-2).all(), (i, float(tg.min()), float(tg.max()))
    print("sagitta", sagitta, "worst cloud offset / bound", worst[0], "worst target offset", worst[1])


@gpu
def test_train_and_eval_tools_on_a_mesh_tree(rendered_tree, tmp_path):
    """tools/train.py --dataset cad for two optimizer steps (19 // 8), then tools/eval_cad.py, on the mesh-rendered tree: both exit 0."""
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--dataset", "cad", "--dataset_root", rendered_tree, "--nepoch", "2", "--batch_size", "8",
           "--workers", "2", "--feed", "threads", "--jitter", "host", "--outf", str(out / "models"), "--log_dir", str(out / "logs"), "--decay_margin", "0",
           "--refine_margin", "0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = r.stdout + r.stderr
    dists = [float(x) for x in re.findall(r"Batch \d+ Frame \d+ Avg_dis:(\S+)", log)]
    assert len(dists) == 2 and all(math.isfinite(d) and d > 0 for d in dists), log[-3000:]
    assert "length of the training set: 19" in log
    ckpt = [f for f in os.listdir(out / "models") if f.startswith("pose_model_")]
    assert ckpt, os.listdir(out / "models")
    sdr = synth.make_state_dict(synth.refiner_spec(5), 1031)
    torch.save({k: torch.from_numpy(x) for k, x in sdr.items()}, tmp_path / "r.pth")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_cad.py"), "--dataset_root", rendered_tree, "--model", str(out / "models" / sorted(ckpt)[0]),
                        "--refine_model", str(tmp_path / "r.pth"), "--output_result_dir", str(tmp_path / "eval"), "--workers", "0"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL success rate" in open(tmp_path / "eval" / "eval_result_logs.txt").read()
