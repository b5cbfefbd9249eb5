"""CPU: the rule of ``df_mesh_icp`` as restated in tests/mesh_icp_np.py, alone, on ``mesh_closest_np.bracket()`` (24 triangles, no
symmetry, bounding-box diagonal D): it converges to the true pose from a perturbed one, and its statuses, counts and options do what the
contract says.  The GPU test holds the device to this restatement bit for bit."""
import math

import numpy as np
import pytest

import mesh_closest_np as m
import mesh_icp_np as icp

V, T = m.bracket()
D = icp.diameter(V)
INF = float("inf")
FACING = (0.3, -0.5, 0.8)


@pytest.mark.parametrize("n,deg,tau,facing", [(64, 5, 0.05, None), (256, 10, 0.1, None), (64, 5, 0.05, FACING), (256, 10, 0.1, FACING)])
def test_converges_to_the_true_pose(n, deg, tau, facing):
    """12 steps, no trimming: the mean point error to the true pose must be <= 1e-9 D.  The points are float64 here (exact samples of
    the surface under the true pose up to rounding), so the fit is limited by fp64 alone."""
    rng = np.random.default_rng(1000 + n + (7 if facing else 0))
    pts, _ = icp.surface_samples(V, T, n, rng, facing)
    assert len(pts) >= 6 and (facing is None or len(pts) < n)
    truth = icp.random_pose(rng)
    start = icp.perturb(truth, rng, math.radians(deg), tau * D)
    cloud = icp.apply_pose(truth, pts)
    pose, stats = icp.icp_item(V, T, cloud, start, INF, 12)
    err0, err = icp.mean_point_error(start, truth, V) / D, icp.mean_point_error(pose, truth, V) / D
    print(f"N {len(pts)}: start {err0:.3e} D -> {err:.3e} D, rms {stats[2]:.3e} -> {stats[4]:.3e}, steps {stats[5]:.0f}")
    assert stats[0] == icp.OK and stats[5] == 12 and stats[1] == stats[3] == len(pts)
    assert err <= 1e-9
    assert abs(math.sqrt(sum(e * e for e in pose[:4])) - 1) < 1e-15 and pose[0] >= 0


def _top_face_points(rng, n):
    """points 0.01 above the box's +z face (z = 1.5), well inside it"""
    return np.stack([rng.uniform(-.4, .4, n), rng.uniform(-.9, .9, n), np.full(n, 1.51)], axis=1)


def test_one_flat_face_is_degenerate_and_keeps_the_pose():
    rng = np.random.default_rng(3)
    pose = icp.random_pose(rng)
    pose[:4] *= 2.5                                                   # not normalised: the output is
    cloud = icp.apply_pose(pose, _top_face_points(rng, 40)).astype(np.float32)
    out, stats = icp.icp_np(V, T, [0, len(T)], [INF], [0], cloud[None], pose[None], 5)
    assert stats[0].tolist() == [icp.DEGENERATE, 40, stats[0, 2], 40, stats[0, 2], 0] and 0.009 < stats[0, 2] < 0.011
    assert m.same_bits(out[0], icp.normalised(pose))


def test_five_inliers_are_too_few():
    rng = np.random.default_rng(4)
    pts, _ = icp.surface_samples(V, T, 5, rng)
    pose = icp.random_pose(rng)
    cloud = icp.apply_pose(pose, pts).astype(np.float32)
    out, stats = icp.icp_np(V, T, [0, len(T)], [INF], [0], cloud[None], pose[None], 3)
    assert stats[0, 0] == icp.FEW and stats[0, 1] == stats[0, 3] == 5 and stats[0, 5] == 0 and m.same_bits(out[0], icp.normalised(pose))
    six, _ = icp.surface_samples(V, T, 6, rng)
    _, stats = icp.icp_np(V, T, [0, len(T)], [INF], [0], icp.apply_pose(pose, six).astype(np.float32)[None], pose[None], 1)
    assert stats[0, 0] != icp.FEW


def test_no_iterations_score_the_given_pose():
    rng = np.random.default_rng(5)
    pts, _ = icp.surface_samples(V, T, 100, rng)
    truth = icp.random_pose(rng)
    start = icp.perturb(truth, rng, math.radians(5), 0.05 * D)
    cloud = icp.apply_pose(truth, pts).astype(np.float32)
    out, stats = icp.icp_np(V, T, [0, len(T)], [INF], [0], cloud[None], start[None], 0)
    assert m.same_bits(out[0, 4:], start[4:]) and np.allclose(out[0, :4], start[:4], rtol=0, atol=1e-15)
    assert stats[0, 0] == icp.OK and stats[0, 1] == stats[0, 3] == 100 and stats[0, 2] == stats[0, 4] > 0.001 * D and stats[0, 5] == 0
    _, at_truth = icp.icp_np(V, T, [0, len(T)], [INF], [0], cloud[None], truth[None], 0)
    assert at_truth[0, 2] < 1e-6 * D                                  # fp32 points: 6e-8 of their size


def test_max_dist_drops_exactly_the_planted_outlier():
    rng = np.random.default_rng(6)
    pts, _ = icp.surface_samples(V, T, 50, rng)
    pts = np.concatenate([pts, [[0.0, 0.0, 2.0]]])                     # 0.5 above the +z face
    pose = icp.random_pose(rng)
    cloud = icp.apply_pose(pose, pts).astype(np.float32)
    _, wide = icp.icp_np(V, T, [0, len(T)], [INF], [0], cloud[None], pose[None], 0)
    _, tight = icp.icp_np(V, T, [0, len(T)], [0.1], [0], cloud[None], pose[None], 0)
    assert wide[0, 1] == 51 and tight[0, 1] == 50 and tight[0, 2] < 1e-6 < wide[0, 2]


def test_cull_rejects_the_back_faces():
    """The camera looks along +z at the box 10 units away: the -z face looks at it, the +z face away."""
    rng = np.random.default_rng(7)
    pts, pick = icp.surface_samples(V, T, 200, rng)
    pose = np.array([1.0, 0, 0, 0, 0, 0, 10.0])
    vv = V.astype(np.float64)
    nrm = np.cross(vv[T[:, 1]] - vv[T[:, 0]], vv[T[:, 2]] - vv[T[:, 0]])[pick]
    front = (nrm * (np.array([0, 0, -10.0]) - pts)).sum(axis=1) > 0
    back_z = (nrm[:, 2] > 0) & (np.abs(nrm[:, 0]) + np.abs(nrm[:, 1]) == 0)
    assert 0 < front.sum() < 200 and back_z.any() and not front[back_z].any()
    cloud = icp.apply_pose(pose, pts).astype(np.float32)
    _, off = icp.icp_np(V, T, [0, len(T)], [INF], [0], cloud[None], pose[None], 0, cull=0)
    _, on = icp.icp_np(V, T, [0, len(T)], [INF], [0], cloud[None], pose[None], 0, cull=1)
    assert off[0, 1] == 200 and on[0, 1] == front.sum()


def test_bad_objects_and_ranges():
    rng = np.random.default_rng(8)
    pts, _ = icp.surface_samples(V, T, 20, rng)
    pose = icp.random_pose(rng)
    cloud = np.repeat(icp.apply_pose(pose, pts).astype(np.float32)[None], 4, axis=0)
    out, stats = icp.icp_np(V, T, [0, len(T), len(T)], [INF, INF], [0, 1, 2, -1], cloud, np.repeat(pose[None], 4, axis=0), 2)
    assert stats[:, 0].tolist() == [icp.OK, icp.BAD_OBJECT, icp.BAD_OBJECT, icp.BAD_OBJECT] and not stats[1:, 1:].any()
    assert all(m.same_bits(out[b], icp.normalised(pose)) for b in (1, 2, 3))
