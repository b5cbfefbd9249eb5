"""CPU: the restatement of ``df_pose_refine_contour`` (tests/pose_contour_np.py) on hand-made frames: that the outline term holds the views
the plane term alone leaves free (two faces of a box, one flat wall), leaves the held views where they were, keeps the truth a fixed point,
equals the dense rule when it adds nothing, and the unit rules of E1..E4.  The GPU test holds the kernels to this restatement bit for bit."""
import math

import numpy as np
import pytest

import mesh_closest_np as m
import mesh_icp_np as icp
import pose_contour_np as cn
import pose_dense_np as dn
import pose_error_np as pe
import pose_verify_np as pv

IH, IW = 48, 64
PROJ = np.array(pv.PROJ, dtype=np.float64)
CLOUD_DIV = 10000.0
SCALE = 600.0
GATE, STEPS, REACH, EDGE = 3000, 10, 6, 65535
WHOLE = np.array([[0, 0, 0, 0, 0, 1]])
SEEDS = (1, 2, 3, 4, 5)
# the box(1, 2, 3) turned about the camera's y axis only: two of its faces show
TWO_FACES = np.concatenate([icp.quat_from_axis_angle([0.0, 1.0, 0.0], math.radians(30.0)), [0.005, -0.003, -0.40]])
WALL = icp.normalised(np.array([0.98, 0.1, -0.15, 0.05, 0.0, 0.0, -0.4]))     # test_flat_wall_is_degenerate_and_frozen's
# test_pose_dense_host.py's three-face views and starts
TRUE = {"box": icp.normalised(np.array([0.85, 0.25, -0.35, 0.3, 0.01, -0.005, -0.40])),
        "bracket": icp.normalised(np.array([0.8, 0.35, -0.3, 0.4, -0.015, 0.01, -0.41]))}
MESH = {"box": m.box(1, 2, 3), "bracket": m.bracket()}
STARTS = {"box": ([1.0, 2.0, -1.0], math.radians(3.0), [0.0015, -0.001, 0.002]),
          "bracket": ([-1.0, 0.5, 2.0], math.radians(2.5), [-0.001, 0.0015, -0.0015])}
# the restatement's own worst final MSSD of the two-face box over SEEDS, in diameters (printed by the test), times 2 for the
# rounding of sums taken in another order
TWO_FACE_WORST = 2.2e-4
TWO_FACE_BOUND = 2.0 * TWO_FACE_WORST


def _scene(mesh, scale, truth, noise=0, seed=4):
    v, t = mesh
    v, t, begin = icp.concat_meshes([(v, t)])
    codes, keys = dn.render_codes(v, t, 0, len(t), scale, PROJ, truth, CLOUD_DIV, IH, IW)
    drawn = codes != 65535
    obs = codes.copy()
    if noise:
        obs = np.where(drawn, np.clip(codes + np.random.default_rng(seed).integers(-noise, noise + 1, codes.shape), 0, 65534), 65535)
    x = v.astype(np.float64) * (scale / CLOUD_DIV)
    return dict(vertices=v, triangles=t, tri_begin=begin, model_scale=np.array([scale]), proj=PROJ, rays=dn.ray_map(PROJ, IH, IW),
                depth=obs[None].astype(np.uint16), mask=drawn[None].astype(np.uint16), codes=codes, keys=keys, x=x, truth=truth)


def _dense(sc, items, pose, gate, iters, mask=False, WH=IH, WW=IW):
    return dn.dense_np(sc["vertices"], sc["triangles"], sc["tri_begin"], sc["model_scale"], sc["proj"], sc["depth"], sc["rays"],
                       sc["mask"] if mask else None, items, pose, CLOUD_DIV, WH, WW, gate, iters)


def _contour(sc, items, pose, gate, iters, scale, reach=REACH, edge_step=EDGE, mask=False, WH=IH, WW=IW, trace=None):
    return cn.contour_np(sc["vertices"], sc["triangles"], sc["tri_begin"], sc["model_scale"], sc["proj"], sc["depth"], sc["rays"],
                         sc["mask"] if mask else None, items, pose, CLOUD_DIV, WH, WW, gate, iters, edge_step, reach, scale, trace=trace)


def _mssd(sc, pose):
    ident = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)[None]
    return math.sqrt(pe.item_maxima(sc["x"], pose, sc["truth"], ident, PROJ, IH, IW)[0][0])


def _starts(truth):
    return np.stack([icp.perturb(truth, np.random.default_rng(s), math.radians(2.0), 0.002) for s in SEEDS])


def test_two_faces_of_a_box_are_held_by_the_outline():
    """Frames with +-2 codes of noise, five starts 2 degrees and 0.002 off.  The dense rule freezes on every one (status 2, no step); with
    the outline term at scale 0.1 every one takes its ten steps and ends nearer the truth, below the recorded bound."""
    sc = _scene(MESH["box"], SCALE, TWO_FACES, noise=2)
    start = _starts(TWO_FACES)
    items = np.repeat(WHOLE, len(SEEDS), axis=0)
    _, ds = _dense(sc, items, start, GATE, STEPS)
    assert (ds[:, 0] == dn.DEGENERATE).all() and (ds[:, 5] == 0).all()
    pose, st = _contour(sc, items, start, GATE, STEPS, 0.1)
    diam = icp.diameter(sc["x"])
    before, after = [_mssd(sc, p) / diam for p in start], [_mssd(sc, p) / diam for p in pose]
    print("two faces: nodes", int((sc["codes"] != 65535).sum()), "pairs", st[:, 6].tolist(), "->", st[:, 7].tolist(),
          "MSSD / diameter", ["%.3e" % e for e in before], "->", ["%.3e" % e for e in after], "worst", "%.3e" % max(after))
    assert (st[:, 0] == cn.OK).all() and (st[:, 5] == STEPS).all() and (st[:, 6] > 0).all()
    assert all(a < b for a, b in zip(after, before))
    assert max(after) < TWO_FACE_BOUND
    assert max(after) > TWO_FACE_WORST / 2, "the recorded worst case is out of date: measure again"


def test_flat_wall_is_held_at_scale_one():
    v, t = pv.quad(2500.0, 1800.0)
    sc = _scene((v, t), 1.0, WALL, noise=2)
    start = _starts(WALL)
    items = np.repeat(WHOLE, len(SEEDS), axis=0)
    _, ds = _dense(sc, items, start, GATE, STEPS)
    assert (ds[:, 0] == dn.DEGENERATE).all()
    pose, st = _contour(sc, items, start, GATE, STEPS, 1.0)
    diam = icp.diameter(sc["x"])
    before, after = [_mssd(sc, p) / diam for p in start], [_mssd(sc, p) / diam for p in pose]
    print("wall: inliers", st[:, 1].tolist(), "pairs", st[:, 6].tolist(), "rms", st[:, 2].tolist(), "->", st[:, 4].tolist(),
          "MSSD / diameter", ["%.3e" % e for e in before], "->", ["%.3e" % e for e in after])
    assert (st[:, 0] == cn.OK).all() and (st[:, 5] == STEPS).all()
    assert (st[:, 4] < st[:, 2]).all(), "the plane rms falls"
    assert all(a < b for a, b in zip(after, before)), "MSSD falls on all five seeds"


@pytest.mark.parametrize("name", ("box", "bracket"))
def test_views_that_were_held_stay_where_they_were(name):
    """test_pose_dense_host.py's three-face views and starts at scale 0.1: MSSD ends within 2 x of the dense rule's."""
    sc = _scene(MESH[name], SCALE, TRUE[name], noise=2)
    axis, angle, shift = STARTS[name]
    start = np.concatenate([icp.quat_mul(icp.quat_from_axis_angle(axis, angle), TRUE[name][:4]), TRUE[name][4:] + np.array(shift)])
    dp, ds = _dense(sc, WHOLE, start[None], GATE, STEPS)
    cp, cs = _contour(sc, WHOLE, start[None], GATE, STEPS, 0.1)
    d, c, diam = _mssd(sc, dp[0]), _mssd(sc, cp[0]), icp.diameter(sc["x"])
    print(f"{name}: MSSD / diameter dense {d / diam:.3e} contour {c / diam:.3e}, pairs {cs[0, 6]:.0f} -> {cs[0, 7]:.0f}")
    assert ds[0, 0] == cs[0, 0] == cn.OK and cs[0, 5] == STEPS and cs[0, 6] > 0
    assert c <= 2.0 * d


def test_the_truth_is_a_fixed_point_on_a_clean_frame():
    """From the true pose on the frame it draws, the drawn outline is the observed outline node for node and code for code: every pair
    has w = 0 and adds nothing to G.  The plane residuals are the code's quantisation, each at most q = 0.5 z_max^2 / (p23 65534)
    rho_max / cloud_div (test_true_pose_scores_every_rendered_node's bound), and three faces that stand at right angles hold a model point
    to the residual along each normal: it moves by at most sqrt(3) q."""
    sc = _scene(MESH["box"], SCALE, TRUE["box"])
    trace = []
    pose, st = _contour(sc, WHOLE, TRUE["box"][None], GATE, 4, 1.0, trace=trace)
    drawn = sc["codes"] != 65535
    z = dn.code_depth(sc["codes"][drawn], PROJ[2, 2], PROJ[2, 3])
    rho = np.sqrt((sc["rays"][drawn] ** 2).sum(axis=1))
    q = 0.5 * (z * z).max() / (PROJ[2, 3] * 65534.0) * rho.max() / CLOUD_DIV
    keys, _, pair, feat = trace[0][0]
    edge = cn.drawn_outline(keys, 0, 0, IH, IW, EDGE)
    assert pair.sum() == edge.sum() > 20 and (feat.reshape(-1)[pair] == np.nonzero(pair)[0]).all(), "every outline node pairs with itself"
    moved = _mssd(sc, pose[0])
    print("truth: pairs", st[0, 6], "rms", st[0, 2], "->", st[0, 4], "MSSD", moved, "bound", math.sqrt(3.0) * q)
    assert st[0, 0] == cn.OK and st[0, 5] == 4 and st[0, 4] <= q and moved <= math.sqrt(3.0) * q


def test_scale_zero_and_no_pair_equal_the_dense_rule():
    sc = _scene(MESH["box"], SCALE, TRUE["box"], noise=2)
    start = icp.perturb(TRUE["box"], np.random.default_rng(3), math.radians(2.0), 0.002)
    dp, ds = _dense(sc, WHOLE, start[None], GATE, 4)
    cp, cs = _contour(sc, WHOLE, start[None], GATE, 4, 0.0)
    assert m.same_bits(cp, dp) and m.same_bits(cs[:, :6], ds) and cs[0, 6] > 0, "scale 0: pairs form and add zeros"
    # reach 0 with disjoint outlines: a far background behind the object, so that the object has no observed outline of its own, and one
    # hole in a corner of the frame, whose four neighbours are the observed outline
    shifted = dict(sc)
    depth = np.where(sc["depth"] == 65535, 60000, sc["depth"]).astype(np.uint16)
    depth[0, 1, 1] = 65535
    shifted["depth"] = depth
    trace = []
    dp, ds = _dense(shifted, WHOLE, start[None], GATE, 3)
    cp, cs = _contour(shifted, WHOLE, start[None], GATE, 3, 1.0, reach=0, trace=trace)
    obs_edge = cn.observed_outline(depth[0], None, 0, 0, 0, IH, IW, EDGE)
    assert obs_edge.sum() == 4 and all(not (cn.drawn_outline(tr[0], 0, 0, IH, IW, EDGE) & obs_edge).any() for tr in trace[0])
    assert ds[0, 5] == 3 and m.same_bits(cp, dp) and m.same_bits(cs[:, :6], ds) and cs[0, 6] == cs[0, 7] == 0


# ---- unit rules --------------------------------------------------------------------------------------------------------------------------
def test_edge_step_at_the_difference_and_one_below():
    """A frame that is on everywhere: columns 0..4 at code 1000, columns 5.. at 1300.  The step makes outline nodes of column 4 (the
    nearer side: its neighbour lies behind it) when edge_step < 300 and none when edge_step = 300; never of column 5."""
    depth = np.full((8, 10), 1300, dtype=np.uint16)
    depth[:, :5] = 1000
    at = cn.observed_outline(depth, None, 0, 0, 0, 8, 10, 300)
    below = cn.observed_outline(depth, None, 0, 0, 0, 8, 10, 299)
    assert not at.any()
    assert below[:, 4].all() and below.sum() == 8


def test_frame_and_window_borders_make_no_outline():
    depth = np.full((8, 10), 500, dtype=np.uint16)
    assert not cn.observed_outline(depth, None, 0, 0, 0, 8, 10, EDGE).any(), "an object cut by the frame on every side"
    assert not cn.observed_outline(depth, None, 0, 2, 3, 4, 5, EDGE).any(), "cut by the window"
    assert not cn.observed_outline(depth, None, 0, -3, -3, 14, 16, EDGE).any(), "a window larger than the frame: nodes outside do not exist"
    depth[3, 4] = 65535
    e = cn.observed_outline(depth, None, 0, 0, 0, 8, 10, EDGE)
    assert e.sum() == 4 and e[2, 4] and e[4, 4] and e[3, 3] and e[3, 5], "a hole inside has an outline"
    mask = np.ones((8, 10), dtype=np.uint16)
    mask[:, 7:] = 0
    e = cn.observed_outline(depth, mask, 1, 0, 0, 8, 10, EDGE)
    assert e[:, 6].all() and not e[:, 7:].any(), "the mask's border is an outline"
    assert not cn.observed_outline(depth, mask, 1, 0, 0, 8, 7, EDGE)[:, 6].any(), "unless the window ends there"


def test_tie_rule_against_a_double_loop():
    """Outline nodes at the four corners of a square: its centre is equidistant from all four, the middles of its sides from two."""
    edge = np.zeros((9, 9), dtype=bool)
    edge[2, 2] = edge[2, 6] = edge[6, 2] = edge[6, 6] = True
    exists = np.ones((9, 9), dtype=bool)
    for reach in (2, 3, 4, 6, 64):
        f = cn.feature_map(exists, edge, reach)
        assert np.array_equal(f, cn.feature_map_loops(exists, edge, reach)), reach
    f = cn.feature_map(exists, edge, 6)
    assert f[4, 4] == 2 * 9 + 2 and f[2, 4] == 2 * 9 + 2 and f[4, 2] == 2 * 9 + 2 and f[6, 4] == 6 * 9 + 2 and f[4, 6] == 2 * 9 + 6
    rng = np.random.default_rng(0)
    edge = rng.random((11, 13)) < 0.08
    exists = rng.random((11, 13)) < 0.9
    for reach in (0, 1, 2, 5):
        assert np.array_equal(cn.feature_map(exists, edge, reach), cn.feature_map_loops(exists, edge, reach)), reach


def test_reach_at_the_distance_and_one_above():
    edge = np.zeros((12, 12), dtype=bool)
    edge[1, 1] = True
    exists = np.ones((12, 12), dtype=bool)
    f5, f4 = cn.feature_map(exists, edge, 5), cn.feature_map(exists, edge, 4)
    assert f5[4, 5] == 13 and f5[5, 4] == 13 and f5[1, 6] == 13, "d2 = 25 = reach^2"
    assert f5[2, 6] == cn.NONE and f5[6, 2] == cn.NONE, "d2 = 26"
    assert f4[4, 5] == cn.NONE and f4[1, 5] == 13
    assert (cn.feature_map(exists, edge, 0) != cn.NONE).sum() == 1


def test_a_nan_ray_drops_its_pair():
    sc = _scene(MESH["box"], SCALE, TWO_FACES)
    trace = []
    _, st = _contour(sc, WHOLE, TWO_FACES[None], GATE, 0, 1.0, trace=trace)
    pair = trace[0][0][2]
    s = int(np.nonzero(pair)[0][3])
    rays = sc["rays"].copy()
    rays[s // IW, s % IW, 1] = np.nan
    sc["rays"] = rays
    trace = []
    _, st2 = _contour(sc, WHOLE, TWO_FACES[None], GATE, 0, 1.0, trace=trace)
    assert not trace[0][0][2][s] and st2[0, 6] == st[0, 6] - 1 and st2[0, 1] == st[0, 1] - 1, "the node is its own feature: one pair, one inlier"


def test_the_few_inlier_rule_ignores_pairs():
    sc = _scene(MESH["box"], SCALE, TWO_FACES)
    drawn = np.argwhere(sc["codes"] != 65535)
    obs = np.where(sc["codes"] != 65535, sc["codes"] + 1, 65535)
    for r, q in drawn[::len(drawn) // 5][:5]:
        obs[r, q] -= 1
    sc["depth"] = obs[None].astype(np.uint16)
    pose, st = _contour(sc, WHOLE, TWO_FACES[None], 0, 3, 1.0)
    assert st[0, 0] == cn.FEW and st[0, 1] == 5 and st[0, 6] > 20 and st[0, 5] == 0
    assert m.same_bits(pose[0], icp.normalised(TWO_FACES))
