"""CPU: the restatement of ``df_pose_refine_dense`` (tests/pose_dense_np.py) on hand-made frames: what the contract promises of a frame
drawn from the true pose, of a flat wall, of windows with too few nodes, of the gate, the mask, bad poses and bad items, and that it
converges on a box and on the bracket from starts inside the gate.  The GPU test holds the kernels to this restatement bit for bit."""
import math

import numpy as np
import pytest

import mesh_closest_np as m
import mesh_icp_np as icp
import pose_dense_np as dn
import pose_error_np as pe
import pose_verify_np as pv

IH, IW = 48, 64
PROJ = np.array(pv.PROJ, dtype=np.float64)
CLOUD_DIV = 10000.0
SCALE = 600.0                                                    # file units -> camera units: the box(1, 2, 3) is 600 x 1200 x 1800
TRUE = {"box": icp.normalised(np.array([0.85, 0.25, -0.35, 0.3, 0.01, -0.005, -0.40])),
        "bracket": icp.normalised(np.array([0.8, 0.35, -0.3, 0.4, -0.015, 0.01, -0.41]))}
MESH = {"box": m.box(1, 2, 3), "bracket": m.bracket()}
# start offsets (rotation about this axis by this angle, shift in cloud units), chosen on the CPU: the restatement converges from them
STARTS = {"box": ([1.0, 2.0, -1.0], math.radians(3.0), [0.0015, -0.001, 0.002]),
          "bracket": ([-1.0, 0.5, 2.0], math.radians(2.5), [-0.001, 0.0015, -0.0015])}
GATE = 3000


def _scene(name, noise=0, seed=0):
    """One object, one frame drawn from its true pose by the raster restatement (no noise unless asked), a mask frame that is 1 where
    it was drawn."""
    v, t = MESH[name]
    v, t, begin = icp.concat_meshes([(v, t)])
    codes, keys = dn.render_codes(v, t, 0, len(t), SCALE, PROJ, TRUE[name], CLOUD_DIV, IH, IW)
    drawn = codes != 65535
    obs = codes.copy()
    if noise:
        obs = np.where(drawn, np.clip(codes + np.random.default_rng(seed).integers(-noise, noise + 1, codes.shape), 0, 65534), 65535)
    return dict(vertices=v, triangles=t, tri_begin=begin, model_scale=np.array([SCALE]), proj=PROJ, rays=dn.ray_map(PROJ, IH, IW),
                depth=obs[None].astype(np.uint16), mask=drawn[None].astype(np.uint16), codes=codes, keys=keys)


def _run(sc, items, pose, WH, WW, gate, iters, mask=False, cull=0, trace=None):
    return dn.dense_np(sc["vertices"], sc["triangles"], sc["tri_begin"], sc["model_scale"], sc["proj"], sc["depth"], sc["rays"],
                       sc["mask"] if mask else None, items, pose, CLOUD_DIV, WH, WW, gate, iters, cull, trace)


WHOLE = np.array([[0, 0, 0, 0, 0, 1]])


@pytest.mark.parametrize("name", ("box", "bracket"))
def test_true_pose_scores_every_rendered_node(name):
    """iters = 0 on the frame the true pose draws: every rendered node is observed with its own code and is an inlier; the residual is
    what the code's quantisation leaves.  A code is off by at most half a step, a step of the code is z^2 / (p23 65534) of depth (the
    derivative of D3's formula), the point moves along its ray of length rho, and the plane distance is at most the point's: rms <=
    0.5 z_max^2 / (p23 65534) rho_max / cloud_div."""
    sc = _scene(name)
    trace = []
    pose, stats = _run(sc, WHOLE, TRUE[name][None], IH, IW, 0, 0, trace=trace)
    drawn = sc["codes"] != 65535
    assert stats[0, 0] == dn.OK and stats[0, 1] == stats[0, 3] == drawn.sum() > 200 and stats[0, 5] == 0
    assert np.array_equal(trace[0][0][1].reshape(IH, IW), drawn)
    z = dn.code_depth(sc["codes"][drawn], PROJ[2, 2], PROJ[2, 3])
    rho = np.sqrt((sc["rays"][drawn] ** 2).sum(axis=1))
    bound = 0.5 * (z * z).max() / (PROJ[2, 3] * 65534.0) * rho.max() / CLOUD_DIV
    print(name, "inliers", int(stats[0, 1]), "rms", stats[0, 2], "bound", bound)
    assert 0 < stats[0, 2] <= bound and stats[0, 2] == stats[0, 4]
    assert m.same_bits(pose[0], icp.normalised(TRUE[name])), "iters = 0 leaves the pose untouched: pose_out is S0's (q, t)"


def test_flat_wall_is_degenerate_and_frozen():
    v, t = pv.quad(2500.0, 1800.0)
    v, t, begin = icp.concat_meshes([(v, t)])
    truth = icp.normalised(np.array([0.98, 0.1, -0.15, 0.05, 0.0, 0.0, -0.4]))
    codes, _ = dn.render_codes(v, t, 0, 2, 1.0, PROJ, truth, CLOUD_DIV, IH, IW)
    sc = dict(vertices=v, triangles=t, tri_begin=begin, model_scale=np.array([1.0]), proj=PROJ, rays=dn.ray_map(PROJ, IH, IW),
              depth=codes[None].astype(np.uint16), mask=None)
    start = icp.perturb(truth, np.random.default_rng(1), math.radians(1.0), 0.001)
    (p4, s4), (p0, s0) = _run(sc, WHOLE, start[None], IH, IW, GATE, 4), _run(sc, WHOLE, start[None], IH, IW, GATE, 0)
    assert s4[0, 0] == dn.DEGENERATE and s4[0, 5] == 0 and s4[0, 1] > 500
    assert m.same_bits(p4[0], icp.normalised(start)) and m.same_bits(s4[0, 1:5], s0[0, 1:5]), "the pose is kept and no later pass touches the item"
    assert m.same_bits(s4[0, 1:3], s4[0, 3:5])


def test_too_few_nodes():
    sc = _scene("box")
    drawn = np.argwhere(sc["codes"] != 65535)
    r, q = drawn[len(drawn) // 2]
    row = int((sc["codes"][r] != 65535).sum())
    assert row >= 6
    items = np.array([[0, 0, IH, 3, 0, 1], [0, 0, -5, 0, 0, 1], [0, 0, r, q, 0, 1], [0, 0, r, q, 0, 1]])
    pose = np.repeat(TRUE["box"][None], 4, axis=0)
    _, stats = _run(sc, items[:2], pose[:2], 5, 7, GATE, 3)
    assert (stats[:, 0] == dn.FEW).all() and not stats[:, 1:].any(), "a window wholly outside the frame"
    _, stats = _run(sc, items, pose, 1, 5, GATE, 3)
    assert (stats[:, 0] == dn.FEW).all() and not stats[:2, 1:].any() and (stats[:, 5] == 0).all()
    assert stats[2, 1] == stats[2, 3] == 5, "five candidate nodes: one short of a step"
    _, stats = _run(sc, items[2:3], pose[:1], 1, 6, GATE, 0)
    assert stats[0, 0] == dn.OK and stats[0, 1] == 6, "iters = 0 scores and does not ask for six"


def test_gate_at_and_below_the_difference():
    sc = _scene("bracket")
    g = 25
    r, q = np.mgrid[0:IH, 0:IW]
    drawn = sc["codes"] != 65535
    obs = np.where(drawn, sc["codes"] + np.where((r + q) % 2 == 0, g, -g), 65535)
    sc["depth"] = obs[None].astype(np.uint16)
    for gate, want in ((g, int(drawn.sum())), (g - 1, 0)):
        trace = []
        _, stats = _run(sc, WHOLE, TRUE["bracket"][None], IH, IW, gate, 0, trace=trace)
        assert int(trace[0][0][2].sum()) == want == stats[0, 1], f"gate {gate}"


def test_mask_that_leaves_one_face():
    """The mask keeps the nodes of the two triangles of the box's largest visible face: the inliers lie on one plane, so the item is
    degenerate; without the mask the same call takes its steps."""
    sc = _scene("box")
    tri = (sc["keys"] & np.uint64(0xffffffff)).astype(np.int64)
    drawn = sc["codes"] != 65535
    face = np.bincount(tri[drawn] // 2).argmax()                 # m.box lays the two triangles of a face next to each other
    sc["mask"] = (drawn & (tri // 2 == face))[None].astype(np.uint16)
    start = icp.perturb(TRUE["box"], np.random.default_rng(2), math.radians(0.5), 0.0005)
    trace = []
    _, masked = _run(sc, WHOLE, start[None], IH, IW, GATE, 2, mask=True, trace=trace)
    inl = trace[0][0][1].reshape(IH, IW)
    assert inl.sum() > 50 and not (inl & (sc["mask"][0] == 0)).any(), "no inlier outside the mask"
    assert masked[0, 0] == dn.DEGENERATE and masked[0, 5] == 0
    _, free = _run(sc, WHOLE, start[None], IH, IW, GATE, 2)
    assert free[0, 0] == dn.OK and free[0, 5] == 2 and free[0, 1] > masked[0, 1]


def test_bad_poses_and_bad_items():
    sc = _scene("box")
    pose = np.repeat(TRUE["box"][None], 6, axis=0)
    pose[0, :4] = 0.0
    pose[1, 1] = np.nan
    pose[2, 6] = np.nan
    items = np.array([[0, 0, 0, 0, 0, 1]] * 3 + [[1, 0, 0, 0, 0, 1], [-1, 0, 0, 0, 0, 1], [0, 1, 0, 0, 0, 1]])
    out, stats = _run(sc, items, pose, IH, IW, GATE, 2)
    assert stats[:, 0].tolist() == [dn.FEW] * 3 + [dn.BAD_ITEM] * 3 and not stats[:, 1:].any()
    assert np.isnan(out[0, :4]).all() and np.isnan(out[1, :4]).all() and np.isnan(out[2, 6]) and m.same_bits(out[2, :4], TRUE["box"][:4])
    assert m.same_bits(out[3:], pose[3:]), "a bad item's pose is the normalised input"
    out, stats = _run(sc, np.array([[0, 0, 0, 0, 3, 1]]), pose[3:4], IH, IW, GATE, 2, mask=True)
    assert stats[0, 0] == dn.BAD_ITEM, "with a mask the mask frame is checked as well"


@pytest.mark.parametrize("name", ("box", "bracket"))
def test_convergence_from_inside_the_gate(name):
    """Frames with +-2 codes of noise; starts a few degrees and millimetres off (``STARTS``).  The last rms is below the first and the
    MSSD to the true pose falls; the measured values are printed (DESIGN 12n records them)."""
    sc = _scene(name, noise=2, seed=4)
    axis, angle, shift = STARTS[name]
    start = np.concatenate([icp.quat_mul(icp.quat_from_axis_angle(axis, angle), TRUE[name][:4]), TRUE[name][4:] + np.array(shift)])
    x = (sc["vertices"].astype(np.float64) * (SCALE / CLOUD_DIV))
    ident = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)[None]
    mssd = lambda p: math.sqrt(pe.item_maxima(x, p, TRUE[name], ident, PROJ, IH, IW)[0][0])
    pose, stats = _run(sc, WHOLE, start[None], IH, IW, GATE, 10)
    before, after = mssd(start), mssd(pose[0])
    print(f"{name}: inliers {int(stats[0, 1])} -> {int(stats[0, 3])}, rms {stats[0, 2]:.3e} -> {stats[0, 4]:.3e}, MSSD {before:.3e} -> {after:.3e} "
          f"(diameter {icp.diameter(x):.3f}), steps {int(stats[0, 5])}")
    assert stats[0, 0] == dn.OK and stats[0, 5] == 10
    assert stats[0, 4] < stats[0, 2] and after < before
    q = pose[0, :4]
    assert abs(math.sqrt(float(q @ q)) - 1.0) < 1e-15 and q[0] >= 0
