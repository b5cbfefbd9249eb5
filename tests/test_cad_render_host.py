"""CPU: the host side of the customCAD renderer -- the pose <-> ``transforms.txt`` maps against the loader's own arithmetic, the numpy
restatement of the renderer (tests/cad_render_np.py) against the loader's depth projector (the first check that a depth image and a pose
describe the same object in the same place), the view draws, and the coloured-PLY reader."""
import random

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import cad_render_np as rnp
import fabricate_cad as fab
from densefusion_amd.datasets.customCAD import render as cr
from densefusion_amd.datasets.customCAD.dataset import PoseDataset, parse_transforms
from densefusion_amd.datasets.customCAD.project_unity_depth import UnityDepthProjector

from cad_render_np import RADIUS, SPHERE_POS, camera_points, grid_bounds, sphere, write_proj  # noqa: F401


def test_pose_round_trip_and_the_loaders_targets(tmp_path):
    rng = np.random.default_rng(0)
    for k in range(20):
        R = Rotation.from_quat(rng.normal(size=4)).as_matrix()
        t = rng.uniform(-3000, 3000, 3)
        pos, quat = cr.pose_to_transform(R, t)
        R2, t2 = cr.transform_to_pose(pos, quat)
        assert np.abs(R2 - R).max() <= 1e-12 and np.abs(t2 - t).max() <= 1e-12
        # the same text record through the loader's parser and its target arithmetic (500 model points: its subset keeps all of them)
        path = tmp_path / "transforms.txt"
        path.write_text("7\n(%s)\n(%s)\n" % (", ".join(repr(float(v)) for v in pos), ", ".join(repr(float(v)) for v in quat)))
        rec = parse_transforms(str(path))[7]
        ds = PoseDataset.__new__(PoseDataset)
        ds.pt, ds.num_pt_mesh_small, ds.add_noise = {1: rng.uniform(-30, 30, (500, 3))}, 500, False
        random.seed(k)
        target, model_points = ds._targets(1, [rec[0].copy(), rec[1].copy()], np.zeros(3))
        Rr, tr = cr.transform_to_pose(rec[0], rec[1])
        want = (np.dot(ds.pt[1] * 10, Rr.T) + tr).astype(np.float32) / 10000.
        assert np.array_equal(target.numpy(), want)
        assert np.abs(Rr - R).max() <= 1e-12


def _sphere_frame(tmp_path, quat_seed):
    IH, IW = 96, 144
    proj = fab.PROJ[1]
    pts, nrm, col = sphere()
    quat = np.random.default_rng(quat_seed).normal(size=4)
    quat /= np.linalg.norm(quat)
    R, t = cr.transform_to_pose(SPHERE_POS, quat)
    pose = np.concatenate([R, t[:, None]], axis=1)
    rgb, depth, mask, stats, winner = rnp.render_frame(pts, nrm, col, pose, 10.0, None, None, proj, IH, IW, 0, 0)
    covered = winner >= 0
    udp = UnityDepthProjector(write_proj(tmp_path / "proj_mat.txt", proj), (IH, IW))
    got = udp.project_depth(depth)[covered]
    want = camera_points(pts[winner[covered]], pose)
    return (rgb, depth, mask, stats, winner, covered, col), got, want, grid_bounds(got[:, 2], proj, IH, IW)


def test_restated_render_agrees_with_the_loaders_projector(tmp_path):
    """A 20 000-point sphere through the restatement, then back through ``UnityDepthProjector.project_depth``: every covered pixel's
    recovered point lies within half a grid step (|z| / (IW P00), |z| / (IH P11)) and half a depth code (0.5 z^2 / (p23 65534)) of the
    point that won the pixel, with a relative slack of 1e-6 for fp64 rounding.

    Measured: 789 covered pixels, worst errors 22.94 / 16.24 / 0.0380 against bounds 22.95 / 16.27 / 0.0380 at those pixels (ratios
    0.99985 / 0.99833 / 0.99972).  The x and y bounds are half a grid step at the RECOVERED depth; the recovered depth itself is off by
    up to half a code, which moves x by up to bz |x / z| more (y alike): 1e-3 of the bound here, so a winner within 1e-3 of a cell's edge
    can pass the stated bound by that much with the renderer exactly on its contract -- of the quaternion seeds 0 .. 15, seeds 5, 10,
    11 and 12 do, by at most 9.5e-5 of the bound.  Seed 0 is the fixture for the stated bound; the next test holds eight seeds to the
    bound with that term added."""
    (rgb, depth, mask, stats, winner, covered, col), got, want, bounds = _sphere_frame(tmp_path, 0)
    assert covered.sum() >= 700 and stats[0] == covered.sum()
    assert (depth[~covered] == 65535).all() and (depth[covered] <= 65534).all() and (rgb[~covered] == 130).all()
    assert np.array_equal(rgb[covered], col[winner[covered]])
    err = np.abs(got - want)
    print("covered", covered.sum(), "worst errors", err.max(axis=0), "worst error / bound", [(err[:, k] / bounds[k]).max() for k in range(3)])
    for k, b in enumerate(bounds):
        assert (err[:, k] <= b * (1 + 1e-6)).all(), (k, (err[:, k] / b).max())
    # the box mask is the half-open slice of the inclusive box
    assert mask[stats[2]:stats[3], stats[4]:stats[5]].all() and mask.sum() == 65535 * (stats[3] - stats[2]) * (stats[5] - stats[4])


@pytest.mark.parametrize("quat_seed", range(8))
def test_restated_render_within_the_complete_bound(tmp_path, quat_seed):
    """The same round trip for eight orientations against the bound that holds in real arithmetic for every input:
    |x' - x| <= |z'| / (IW P00) + bz |x / z| (y alike), |z' - z| <= bz = 0.5 z'^2 / (p23 65534); 1e-6 relative for fp64 rounding."""
    (_, _, _, _, _, covered, _), got, want, (bx, by, bz) = _sphere_frame(tmp_path, quat_seed)
    assert covered.sum() >= 700
    err = np.abs(got - want)
    assert (err[:, 2] <= bz * (1 + 1e-6)).all()
    assert (err[:, 0] <= (bx + bz * np.abs(want[:, 0] / want[:, 2])) * (1 + 1e-6)).all()
    assert (err[:, 1] <= (by + bz * np.abs(want[:, 1] / want[:, 2])) * (1 + 1e-6)).all()


def test_sample_view_is_seeded_and_in_range():
    kw = dict(n_points=1000, center=(0.0, 0.0, 4.0), scene_scale=2.0, max_holes=3, hole_mean=30.0, hole_std=10.0)
    counts = set()
    for seed in range(200):
        axis, angle, xyz, holes = cr.sample_view(seed, **kw)
        a2, g2, x2, h2 = cr.sample_view(seed, **kw)
        assert np.array_equal(axis, a2) and angle == g2 and np.array_equal(xyz, x2) and holes == h2
        assert abs(np.linalg.norm(axis) - 1) < 1e-12 and 0 <= angle < 2 * np.pi
        assert abs(xyz[0]) <= 1.0 and abs(xyz[1]) <= 1.0 and abs(xyz[2] - 4.0) <= 0.6
        assert len(holes) < 3 and all(0 <= h < 1000 and r >= 0 for h, r in holes)
        counts.add(len(holes))
    assert counts == {0, 1, 2}
    assert not np.array_equal(cr.sample_view(0, **kw)[0], cr.sample_view(1, **kw)[0])
    # the stream itself: the draws in the stated order
    np.random.seed(5)
    axis = np.random.uniform(-1, 1, size=3)
    axis /= np.linalg.norm(axis)
    angle = np.random.uniform(0, np.pi * 2)
    xyz = np.array([0.0, 0.0, 4.0])
    for k, span in enumerate((0.5, 0.5, 0.3)):
        u = np.random.uniform(0, span)
        xyz[k] += u * (-1 if np.random.rand() < 0.5 else 1) * 2.0
    n = np.random.randint(3)
    holes = []
    for _ in range(n):
        h = np.random.randint(1000)
        holes.append((h, max(0, np.random.normal(30.0, 10.0))))
    got = cr.sample_view(5, **kw)
    assert np.array_equal(got[0], axis) and got[1] == angle and np.array_equal(got[2], xyz) and got[3] == holes


def test_view_pose_turns_about_the_centroid():
    rng = np.random.default_rng(2)
    pts = rng.uniform(-50, 50, (100, 3)) + np.array([20.0, -10.0, 5.0])
    centroid = pts.mean(axis=0)
    axis, angle, xyz, _ = cr.sample_view(9, 100, (0, 0, 4.0), 1.0, hole_mean=30.0, hole_std=10.0)
    R, t = cr.view_pose(axis, angle, xyz, centroid, 10.0)
    placed = (10.0 * pts) @ R.T + t
    assert np.allclose(placed.mean(axis=0), [xyz[0] * 1000, xyz[1] * 1000, -xyz[2] * 1000], atol=1e-9)
    assert np.allclose(R, Rotation.from_rotvec(axis * angle).as_matrix()) and abs(np.linalg.det(R) - 1) < 1e-12


@pytest.mark.parametrize("with_normals", [True, False])
def test_read_colored_ply_ascii_equals_binary(tmp_path, with_normals):
    rng = np.random.default_rng(4)
    n = 257
    pts = rng.uniform(-60, 60, (n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    col = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    props = "property float x\nproperty float y\nproperty float z\n" + ("property float nx\nproperty float ny\nproperty float nz\n" if with_normals else "") + \
        "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    head = "ply\nformat %s 1.0\ncomment fabricated\nelement vertex %d\n" + props + "end_header\n"
    dt = np.dtype([(a, "<f4") for a in (("x", "y", "z", "nx", "ny", "nz") if with_normals else ("x", "y", "z"))] + [(a, "u1") for a in ("r", "g", "b")])
    rec = np.zeros(n, dtype=dt)
    for k, a in enumerate("xyz"):
        rec[a] = pts[:, k]
        if with_normals:
            rec["n" + a] = nrm[:, k]
    for k, a in enumerate("rgb"):
        rec[a] = col[:, k]
    (tmp_path / "b.ply").write_bytes((head % ("binary_little_endian", n)).encode("ascii") + rec.tobytes())
    rows = ["%s %s\n" % (" ".join("%.9g" % v for v in (list(pts[i]) + (list(nrm[i]) if with_normals else []))), " ".join(str(int(v)) for v in col[i]))
            for i in range(n)]
    (tmp_path / "a.ply").write_text(head % ("ascii", n) + "".join(rows))
    a, b = cr.read_colored_ply(str(tmp_path / "a.ply")), cr.read_colored_ply(str(tmp_path / "b.ply"))
    assert np.array_equal(b[0], pts) and np.array_equal(b[2], col) and b[0].dtype == np.float32 and b[2].dtype == np.uint8
    assert (b[1] is None) == (not with_normals) and (b[1] is None or np.array_equal(b[1], nrm))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and (a[1] is None) == (b[1] is None)
    assert a[1] is None or np.array_equal(a[1], b[1])


def test_read_colored_ply_samples_a_mesh(tmp_path):
    """A two-triangle square in the plane z = 2 with coloured corners: sampled points lie on it, carry its normal and mixed colours."""
    text = ("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
            "property uchar blue\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n"
            "0 0 2 255 0 0\n1 0 2 255 0 0\n1 1 2 255 0 0\n0 1 2 255 0 0\n4 0 1 2 3\n")
    (tmp_path / "m.ply").write_text(text)
    with pytest.raises(ValueError):
        cr.read_colored_ply(str(tmp_path / "m.ply"))
    np.random.seed(1)
    pts, nrm, col = cr.read_colored_ply(str(tmp_path / "m.ply"), n_points=300)
    assert pts.shape == (300, 3) and (pts[:, 2] == 2).all() and pts[:, :2].min() >= 0 and pts[:, :2].max() <= 1
    assert np.allclose(nrm, [0, 0, 1]) and (col == [255, 0, 0]).all()
