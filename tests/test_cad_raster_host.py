"""CPU: the host side of the customCAD triangle rasteriser -- the numpy restatement of ``df_cad_render_mesh`` (tests/cad_raster_np.py)
held to what a rasteriser must give (no cracks between triangles, culling that changes nothing on a closed convex mesh, depth that the
loader's projector puts back on the facet, flat colour), then the mesh reader, the index check of ``CadMeshRenderer`` and the tool's flags."""
import importlib
import os
import sys

import numpy as np
import pytest
from scipy import ndimage
from scipy.spatial.transform import Rotation

import cad_raster_np as mnp
import fabricate_cad as fab
from cad_render_np import grid_bounds, write_proj
from densefusion_amd.datasets.customCAD import render as cr
from densefusion_amd.datasets.customCAD.project_unity_depth import UnityDepthProjector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROJ = np.array(fab.PROJ[1])
IH, IW = 120, 160


def _pose(R, t):
    return np.concatenate([np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)[:, None]], axis=1)


@pytest.fixture(scope="module")
def sphere_frames():
    """The icosphere of subdivision 4 (radius 60 file units, x 10) at four poses inside a 120 x 160 frame, with cull 0 and cull 1."""
    v, tri = mnp.icosphere(4, 60.0)
    v = v.astype(np.float32)
    col = np.random.default_rng(2).integers(0, 256, (len(v), 3), dtype=np.uint8)
    rot = Rotation.from_quat(np.random.default_rng(1).normal(size=(4, 4))).as_matrix()
    poses = np.stack([_pose(rot[k], [150.0 * k - 200.0, 60.0 * k - 100.0, -3500.0]) for k in range(4)])
    return {cull: mnp.render(v, col, tri, poses, 10.0, None, PROJ, IH, IW, cull, 1) for cull in (0, 1)}


def test_no_cracks_between_triangles(sphere_frames):
    """Every uncovered pixel is 4-connected to the frame's border: no node was lost between two triangles of the closed surface."""
    rgb, depth, mask, stats, winner = sphere_frames[1]
    for f in range(4):
        covered = winner[f] >= 0
        assert covered.sum() >= 1000 and stats[f, 0] == covered.sum()
        assert stats[f, 2] > 0 and stats[f, 3] < IH - 1 and stats[f, 4] > 0 and stats[f, 5] < IW - 1, "the sphere lies inside the frame"
        lab, n = ndimage.label(~covered)                              # 4-connectivity is scipy's default structure
        border = np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))
        enclosed = np.setdiff1d(np.arange(1, n + 1), border)
        assert len(enclosed) == 0, (f, [np.argwhere(lab == k)[:3].tolist() for k in enclosed[:3]])
        assert (depth[f][covered] <= 65534).all() and (depth[f][~covered] == 65535).all() and (rgb[f][~covered] == 130).all()


def test_culling_changes_nothing_on_a_closed_convex_mesh(sphere_frames):
    a, b = sphere_frames[0], sphere_frames[1]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert (a[3][:, 1] > b[3][:, 1]).all(), "cull 0 also sends the back faces through the key test"


def test_depth_round_trip_through_the_loaders_projector(tmp_path):
    """A rectangle of 2 x 8 x 8 triangles in the model's plane z = 0 (exactly planar in float32), tilted by the pose: for every covered
    pixel the point ``UnityDepthProjector.project_depth`` recovers lies on the rectangle's plane to within half a depth code, measured
    along the pixel's view ray.  V5 is linear over the screen on a plane, so the surface is exact on the grid ray and only the code's
    rounding enters: 1/z' - 1/z = delta / p23 with |delta| <= 0.5 / 65534, i.e. |z' - z| <= 0.5 |z z'| / (p23 65534), which is ``bz`` of
    ``grid_bounds`` at the geometric mean of the two depths; 1e-6 relative for fp64 rounding."""
    g = np.arange(9, dtype=np.float64) * 15.0 - 60.0
    v = np.stack([np.repeat(g, 9), np.tile(g, 9), np.zeros(81)], axis=1).astype(np.float32)
    quad = np.array([[i * 9 + j, (i + 1) * 9 + j, (i + 1) * 9 + j + 1, i * 9 + j + 1] for i in range(8) for j in range(8)])
    tri = np.concatenate([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]]).astype(np.int32)
    assert len(tri) == 2 * 8 * 8
    col = np.full((81, 3), 200, dtype=np.uint8)
    R = Rotation.from_euler("xyz", [35.0, -40.0, 20.0], degrees=True).as_matrix()
    t = np.array([120.0, -80.0, -3600.0])
    rgb, depth, mask, stats, winner = mnp.render_frame(v, col, tri, _pose(R, t), 10.0, None, None, PROJ, IH, IW, 0, 0)
    covered = winner >= 0
    assert covered.sum() >= 500
    udp = UnityDepthProjector(write_proj(tmp_path / "proj_mat.txt", PROJ), (IH, IW))
    p = udp.project_depth(depth)[covered]
    n = R[:, 2]                                                          # the plane n . (x - t) = 0 in camera space
    on_plane = p * ((n @ t) / (p @ n))[:, None]                          # where the pixel's view ray meets it
    bz = grid_bounds(np.sqrt(on_plane[:, 2] * p[:, 2]), PROJ, IH, IW)[2]
    err = np.abs(on_plane[:, 2] - p[:, 2])
    print("covered", covered.sum(), "codes", depth[covered].min(), depth[covered].max(), "worst error / bound", (err / bz).max())
    assert (err <= bz * (1 + 1e-6)).all(), (err / bz).max()
    assert len(np.unique(depth[covered])) > 100, "the rectangle is tilted: it spans many codes"


def test_equal_corner_colours_render_exactly():
    v = np.array([[-50, -40, 3], [60, -30, -20], [5, 55, 30], [-50, -40, -80], [60, -30, -90], [5, 55, -70]], dtype=np.float32)
    tri = np.array([[0, 1, 2], [3, 5, 4]], dtype=np.int32)
    col = np.array([[37, 201, 9]] * 3 + [[255, 0, 128]] * 3, dtype=np.uint8)
    R = Rotation.from_euler("xyz", [10.0, 25.0, -15.0], degrees=True).as_matrix()
    rgb, depth, mask, stats, winner = mnp.render_frame(v, col, tri, _pose(R, [0.0, 0.0, -3000.0]), 10.0, None, None, PROJ, IH, IW, 0, 0)
    assert (winner == 0).sum() >= 200 and stats[1] == 2
    assert (rgb[winner == 0] == [37, 201, 9]).all() and (rgb[winner == 1] == [255, 0, 128]).all() and (rgb[winner < 0] == 130).all()


def test_read_colored_mesh(tmp_path):
    """A quad and a pentagon are cut into fans; ASCII equals binary; missing colours come back mid-grey."""
    rng = np.random.default_rng(6)
    pts = rng.uniform(-60, 60, (7, 3)).astype(np.float32)
    col = rng.integers(0, 256, (7, 3), dtype=np.uint8)
    faces = [[0, 1, 2, 3], [2, 4, 5], [6, 5, 4, 3, 1]]
    want = np.array([[0, 1, 2], [0, 2, 3], [2, 4, 5], [6, 5, 4], [6, 4, 3], [6, 3, 1]], dtype=np.int32)
    head = ("ply\nformat %s 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n%s"
            "element face 3\nproperty list uchar int vertex_indices\nend_header\n")
    cprops = "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    rows = "".join("%s %s\n" % (" ".join("%.9g" % x for x in pts[i]), " ".join(str(int(x)) for x in col[i])) for i in range(7))
    (tmp_path / "a.ply").write_text(head % ("ascii", cprops) + rows + "".join("%d %s\n" % (len(f), " ".join(map(str, f))) for f in faces))
    rec = np.zeros(7, dtype=[(a, "<f4") for a in "xyz"] + [(a, "u1") for a in "rgb"])
    for k, a in enumerate("xyz"):
        rec[a] = pts[:, k]
    for k, a in enumerate("rgb"):
        rec[a] = col[:, k]
    fbytes = b"".join(np.uint8(len(f)).tobytes() + np.asarray(f, dtype="<i4").tobytes() for f in faces)
    (tmp_path / "b.ply").write_bytes((head % ("binary_little_endian", cprops)).encode("ascii") + rec.tobytes() + fbytes)
    (tmp_path / "g.ply").write_bytes((head % ("binary_little_endian", "")).encode("ascii") + pts.astype("<f4").tobytes() + fbytes)
    for name in ("a.ply", "b.ply"):
        v, tri, c = cr.read_colored_mesh(str(tmp_path / name))
        assert v.dtype == np.float32 and tri.dtype == np.int32 and c.dtype == np.uint8
        assert np.array_equal(v, pts) and np.array_equal(tri, want) and np.array_equal(c, col), name
    v, tri, c = cr.read_colored_mesh(str(tmp_path / "g.ply"))
    assert np.array_equal(v, pts) and np.array_equal(tri, want) and c.shape == (7, 3) and (c == 128).all()
    # the fixture writer of the rasteriser tests reads back as it was written
    path = mnp.write_mesh_ply(tmp_path / "w.ply", pts, want, col)
    v, tri, c = cr.read_colored_mesh(path)
    assert np.array_equal(v, pts) and np.array_equal(tri, want) and np.array_equal(c, col)


def test_triangle_indices_are_checked_before_anything_is_uploaded():
    tri = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int64)
    got = cr.check_triangles(tri, 4)
    assert got.dtype == np.int32 and got.flags.c_contiguous and np.array_equal(got, tri)
    for bad in (np.array([[0, 1, 4]]), np.array([[0, -1, 2]]), np.array([[0, 1, 2], [2, 1, 2 ** 31]], dtype=np.int64)):
        with pytest.raises(ValueError, match="outside 0..3"):
            cr.check_triangles(bad, 4)
    for bad in (np.zeros((0, 3), dtype=np.int32), np.zeros((2, 4), dtype=np.int32), np.zeros((2, 3))):
        with pytest.raises(ValueError):
            cr.check_triangles(bad, 4)
    # the constructor raises from that check, before it touches a device: this holds on a machine without one
    with pytest.raises(ValueError, match="outside 0..3"):
        cr.CadMeshRenderer(np.zeros((4, 3), dtype=np.float32), np.array([[0, 1, 4]]), np.zeros((4, 3), dtype=np.uint8), PROJ, (IH, IW))


def test_tool_knows_raster_and_cull(capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        tool = importlib.import_module("render_cad_dataset")
    finally:
        sys.path.pop(0)
    ap = tool.build_parser()
    opt = ap.parse_args(["--model", "m.ply", "--output_root", "out"])
    assert opt.raster == "points" and opt.cull == 1 and opt.splat == 1 and opt.points == 0, "the defaults of every existing command line"
    opt = ap.parse_args(["--model", "m.ply", "--output_root", "out", "--raster", "mesh", "--cull", "0"])
    assert opt.raster == "mesh" and opt.cull == 0
    for extra in (["--raster", "voxels"], ["--cull", "2"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["--model", "m.ply", "--output_root", "out"] + extra)
    # --splat and --points belong to the point path: rejected with --raster mesh before anything else happens
    for extra in (["--splat", "2"], ["--points", "5000"]):
        with pytest.raises(SystemExit) as e:
            tool.main(["--model", "m.ply", "--output_root", "out", "--raster", "mesh"] + extra)
        assert e.value.code == 2 and "--raster points" in capsys.readouterr().err
