"""CPU: the symmetry sets made from a symmetry report (datasets/customCAD/symmetry.py ``symmetry_set``) and the numpy restatement of
df_pose_sym_error (tests/pose_error_np.py) on cases whose answers are known by hand.  The reports are hand-made, or ``detect_symmetry``'s
own through its CPU seam (``closest=``)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_closest_np as m  # noqa: E402
import pose_error_np as pn  # noqa: E402

from densefusion_amd.datasets.customCAD.symmetry import SymmetryReport, detect_symmetry, is_revolution, symmetry_set  # noqa: E402

IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)


def _report(axes, passed, centroid=(0.0, 0.0, 0.0)):
    """a hand-made report: ``passed`` rows are (axis index, order; 0 = the 1-radian probe)"""
    return SymmetryReport(symmetric=bool(passed), axes=np.array(axes, dtype=np.float64), passed=[(a, n, 0.0, float("nan")) for a, n in passed],
                          D=1.0, centroid=np.array(centroid, dtype=np.float64))


def _detect(mesh, **kw):
    return detect_symmetry(mesh[0], mesh[1], None, closest=m.closest_np, samples=256, **kw)


def _is_group(S):
    """closed under composition, holds the inverse of each element, every element a proper rotation, the identity first"""
    R = S[:, :, :3]
    assert np.array_equal(S[0], IDENTITY)
    assert np.allclose(np.einsum("sij,skj->sik", R, R), np.eye(3), atol=1e-9) and np.allclose(np.linalg.det(R), 1.0, atol=1e-9)

    def member(X):
        return bool((np.abs(R - X).reshape(len(R), 9).max(axis=1) <= 5e-6).any())
    for A in R:
        assert member(A.T)
    step = max(1, len(R) // 24)                                     # every element against a spread of the others: the large sets stay quick
    for A in R:
        for B in R[::step]:
            assert member(A @ B)
    return True


HAND = {
    "box": (_report(np.eye(3), [(0, 2), (1, 2), (2, 2)]), 4),
    "square prism": (_report(np.eye(3), [(0, 2), (1, 2), (2, 2), (2, 4)]), 8),
    "cube": (_report(np.eye(3), [(0, 2), (0, 4), (1, 2), (1, 4), (2, 2), (2, 4)]), 24),
    "revolution": (_report(np.eye(3), [(2, n) for n in range(2, 13)] + [(2, 0)]), 315),
    "revolution with flip": (_report(np.eye(3), [(0, 2), (1, 2)] + [(2, n) for n in range(2, 13)] + [(2, 0)]), 630),
    "nothing": (_report(np.eye(3), []), 1),
}
for _n in (3, 5, 6):
    _side = [[math.cos(math.pi * (2 * k + 1) / _n), math.sin(math.pi * (2 * k + 1) / _n), 0.0] for k in range(_n)]
    HAND["prism %d" % _n] = (_report([[0, 0, 1.0]] + _side, [(0, _n)] + [(1 + k, 2) for k in range(_n)]), 2 * _n)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_made_reports_give_the_known_groups(name):
    report, order = HAND[name]
    S = symmetry_set(report)
    assert S.shape == (order, 3, 4) and S.dtype == np.float64 and np.array_equal(S[0], IDENTITY) and _is_group(S)
    assert symmetry_set(report).tobytes() == S.tobytes()            # a pure function of the report
    if order > 1:
        with pytest.raises(ValueError, match="widget"):
            symmetry_set(report, cap=order - 1, name="widget")
    assert len(symmetry_set(report, cap=order)) == order            # a cap at the order itself is enough


def test_the_revolution_step_is_the_bop_discretisation():
    report = HAND["revolution"][0]
    assert len(symmetry_set(report, step=0.01)) == 315 and len(symmetry_set(report, step=0.1)) == 32 == math.ceil(math.pi / 0.1)
    S = symmetry_set(report)
    assert np.allclose(S[1, :, :3], pn.rotation((0, 0, 1), 2 * math.pi / 315), atol=1e-12)
    with pytest.raises(ValueError):
        symmetry_set(report, step=0.0)


def test_which_reports_are_taken_as_surfaces_of_revolution():
    assert is_revolution(HAND["revolution"][0]) and is_revolution(HAND["revolution with flip"][0])
    assert not is_revolution(HAND["cube"][0]) and not is_revolution(HAND["nothing"][0])
    # the hexagon at the default tolerance: 1 radian is 2.7 degrees short of its sixth turn and the probe passes; at 0.2 % it does not
    hexagon = m.prism(6, 1, 1.5)
    assert is_revolution(_detect(hexagon)) and not is_revolution(_detect(hexagon, tol=0.002))


def test_two_revolution_axes_do_not_close():
    with pytest.raises(ValueError, match="ball"):
        symmetry_set(_report(np.eye(3), [(0, 0), (2, 0)]), name="ball")


def test_the_perpendicular_rule_on_each_side_of_its_bound():
    """A half turn about an axis b beside a revolution axis a: with |a . b| <= 0.05 it is the flip of the revolution set, taken about
    the part of b that is exactly perpendicular to a (630 rotations); past 0.05 it stays a generator as it is, and a half turn about an
    axis 87 degrees from a, composed with the rotations about a, does not close."""
    a = np.array([0.0, 0.0, 1.0])
    for dot, closes in ((0.0, True), (0.049, True), (0.05, True), (0.051, False)):
        b = np.array([math.sqrt(1.0 - dot * dot), 0.0, dot])
        report = _report([a, b], [(1, 2), (0, 0)])
        if closes:
            S = symmetry_set(report)
            assert len(S) == 630 and _is_group(S)
            flips = S[np.abs(S[:, 2, 2] + 1.0) < 1e-9]               # the elements that turn a over: half turns about axes in the xy plane
            assert len(flips) == 315 and np.abs(flips[:, 2, :2]).max() < 1e-9
        else:
            with pytest.raises(ValueError, match="tilted"):
                symmetry_set(report, name="tilted")


def test_the_centre_of_rotation_is_the_reports_centroid():
    c = np.array([1.0, -2.0, 3.0])
    S = symmetry_set(_report(np.eye(3), [(2, 4)], centroid=c))
    assert len(S) == 4
    for X in S:
        assert np.array_equal(X[:, :3] @ c + X[:, 3], c)            # quarter turns are exact: the centroid stays where it is


DETECTED = [("box", lambda: m.box(2, 4, 6), 4), ("square prism", lambda: m.box(2, 2, 6), 8), ("cube", lambda: m.box(2, 2, 2), 24),
            ("prism 3", lambda: m.prism(3, 1, 1.5), 6), ("prism 5", lambda: m.prism(5, 1, 1.5), 10), ("prism 6", lambda: m.prism(6, 1, 1.5), 12),
            ("bracket", m.bracket, 1)]


@pytest.mark.parametrize("name,make,order", DETECTED, ids=[d[0] for d in DETECTED])
def test_detected_reports_give_the_known_groups_and_move_the_mesh_onto_itself(name, make, order):
    v, t = make()
    # 1 radian is 2.7 degrees short of a hexagon's sixth turn: at the default tolerance of 1 % of the diagonal the probe passes and the
    # hexagon counts as a surface of revolution (630 rotations); its own twelve are what a tolerance of 0.2 % finds
    S = symmetry_set(_detect((v, t), **({"tol": 0.002} if name == "prism 6" else {})), name=name)
    assert len(S) == order and _is_group(S)
    d2, tri, _ = m.closest_np(v, t, v.astype(np.float64), S, want_closest=False)
    assert (tri >= 0).all()
    worst = float(np.sqrt(d2.max()))
    print(name, "set of", len(S), "largest distance of a moved vertex", worst)
    if name in ("box", "square prism", "cube"):
        # integer coordinates, signed permutations and a centroid that is zero to rounding: every moved vertex is within rounding of
        # the surface; the hand-made report below, whose centroid is exactly zero, gives exactly 0
        assert worst < 1e-14
    else:
        # the ring is stored in fp32 and the half-turn axes come from its normals: angles good to about 1e-7
        assert worst < 1e-6


def test_a_moved_vertex_of_an_integer_box_lies_exactly_on_the_surface():
    v, t = m.box(2, 4, 6)
    S = symmetry_set(HAND["box"][0])
    assert np.array_equal(np.abs(S[:, :, :3]), np.tile(np.eye(3), (4, 1, 1))) and not S[:, :, 3].any()
    d2, _, _ = m.closest_np(v, t, v.astype(np.float64), S, want_closest=False)
    assert (d2 == 0.0).all()
    v, t = m.box(2, 2, 2)
    d2, _, _ = m.closest_np(v, t, v.astype(np.float64), symmetry_set(HAND["cube"][0]), want_closest=False)
    assert d2.shape == (24, 24) and (d2 == 0.0).all()


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------------
FLIP = np.array([[-1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, 1.0, 0]])


def _box_call(sets, pose_est, pose_gt):
    v, _ = m.box(6, 8, 2)                                           # half extents 3, 4, 1: the xy diagonal is 2 * 5
    vv, vb, s, sb = pn.pack([v], [sets])
    return pn.sym_error_np(vv, vb, s, sb, [0], np.array([pose_est], dtype=np.float64), np.array([pose_gt], dtype=np.float64), pn.PROJ, pn.IH, pn.IW)[0]


def test_equal_poses_give_zero():
    pose = pn.random_poses(1, np.random.default_rng(0))[0]
    row = _box_call(pn.cyclic_set(4), pose, pose)
    assert row.tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 24.0]


def test_a_flipped_box_costs_nothing_with_its_set_and_its_extent_without():
    """q = (1, 0, 0, +-1) are the exact quarter turns about z (n = 2, s = 1: every entry of R is 0 or +-1), so est = gt o FLIP holds
    to the bit."""
    gt, est = [1.0, 0, 0, -1.0, 0.0, 0.0, -20.0], [1.0, 0, 0, 1.0, 0.0, 0.0, -20.0]
    with_set = _box_call(np.stack([IDENTITY, FLIP]), est, gt)
    assert with_set.tolist() == [0.0, 0.0, 1.0, 0.0, 1.0, 24.0]
    alone = _box_call(IDENTITY[None], est, gt)
    assert alone[1] == 10.0 and alone[2] == 0.0 and alone[3] > 0.0
    # the pixel distance of the same corner: u and v differ by 2 * (x, y) * p / depth * size / 2 with depth 19 or 21
    print("flipped box without its set: mssd", alone[1], "mspd", alone[3])


def test_a_vertex_behind_the_camera_has_no_pixel():
    gt = [1.0, 0, 0, 0, 0.0, 0.0, -20.0]
    est = [1.0, 0, 0, 0, 0.0, 0.0, 0.5]                             # the box straddles the camera plane: z in -0.5 .. 1.5
    row = _box_call(IDENTITY[None], est, gt)
    assert row[0] == 0 and row[1] == 20.5 and np.isposinf(row[3]) and row[4] == 0
    row = _box_call(IDENTITY[None], gt, est)                        # the true pose behind the camera: the same
    assert np.isposinf(row[3])


def test_bad_items_and_poses():
    v, _ = m.box(2, 4, 6)
    vv, vb, s, sb = pn.pack([v, np.zeros((0, 3)), v], [IDENTITY[None], IDENTITY[None], np.zeros((0, 3, 4))])
    pose = pn.random_poses(6, np.random.default_rng(1))
    est = pose.copy()
    est[4, 0] = np.nan
    est[5, :4] = 0.0                                                # a zero quaternion is the identity rotation
    out = pn.sym_error_np(vv, vb, s, sb, [0, 1, 2, 3, 0, 0], est, pose, pn.PROJ, pn.IH, pn.IW)
    assert out[:, 0].tolist() == [0, 1, 1, 1, 0, 0] and not out[1:4, 1:].any()
    assert np.isposinf(out[4, 1]) and np.isposinf(out[4, 3]) and out[4, 2] == 0 and out[4, 4] == 0
    ident = pose[5].copy()
    ident[:4] = [1, 0, 0, 0]
    want = pn.sym_error_np(vv, vb, s, sb, [0], ident[None], pose[5:6], pn.PROJ, pn.IH, pn.IW)
    assert pn.same_bits(out[5], want[0]) and out[5, 1] > 0


# ---- the restatement of df_pose_vsd on the wall-and-occluder frames of tests/test_pose_verify_host.py ---------------------------------------
import fabricate_cad as fab  # noqa: E402
import mesh_icp_np as icp  # noqa: E402
import pose_verify_np as pv  # noqa: E402

VH, VW, WALL = 64, 96, 60000
DELTA, SHIFT = 15.0, 0.002                                         # camera units; cloud units (20 camera units along the view axis)


@pytest.fixture(scope="module")
def part():
    """The bracket of the verification tests at its true pose in front of a wall: scene arguments, pose, rendered codes, ray map."""
    from densefusion_amd.datasets.customCAD.project_unity_depth import UnityDepthProjector
    v, t = m.bracket()
    q = icp.quat_mul(icp.quat_from_axis_angle([0, 1, 0], 0.6), icp.quat_from_axis_angle([1, 0, 0], 0.5))
    sc = dict(vertices=v * np.float32(30.0), triangles=t, tri_begin=np.array([0, len(t)], np.int32), model_scale=np.array([10.0]),
              proj=np.array(fab.PROJ[1]), pose=np.concatenate([q, [0.004, -0.003, -0.28]]))
    sc["rays"] = UnityDepthProjector.from_matrix(sc["proj"], (VH, VW)).ray_map
    keys = []
    pv.verify_np(sc["vertices"], t, sc["tri_begin"], sc["model_scale"], sc["proj"], np.full((1, VH, VW), WALL, np.uint16), None,
                 [[0, 0, 0, 0, 0, 65535]], [sc["pose"]], pv.CLOUD_DIV, VH, VW, 1, 1, keys)
    sc["codes"] = pv.rendered_codes(keys[0], 0, 0, VH, VW)
    return sc


def vsd_run(sc, depth, est, gt, tau, delta=DELTA, gaps=None):
    return pn.vsd_np(sc["vertices"], sc["triangles"], sc["tri_begin"], sc["model_scale"], sc["proj"], np.asarray(depth, np.uint16)[None], sc["rays"],
                     [[0, 0, 0, 0, 0, 0]], [est], [gt], pv.CLOUD_DIV, [delta], [tau], VH, VW, 1, gaps)[0]


def test_vsd_of_the_true_pose_is_zero(part):
    on = part["codes"] != 65535
    n = int(on.sum())
    row = vsd_run(part, np.where(on, part["codes"], WALL), part["pose"], part["pose"], [0.0, 5.0])
    assert n > 300 and row.tolist() == [0, n, n, n, n, 0]           # tau = 0: every inter node has a gap >= 0; tau = 5: none
    assert pn.vsd_values(row[None]).tolist() == [[1.0, 0.0]]


def test_vsd_under_an_occluder_and_with_nothing_observed(part):
    on = part["codes"] != 65535
    n = int(on.sum())
    # 3 000 codes nearer over the whole part: about 120 camera units at this range, far past delta = 15: nothing is visible
    hidden = vsd_run(part, np.where(on, part["codes"] - 3000, WALL), part["pose"], part["pose"], [5.0])
    assert hidden.tolist() == [0, 0, 0, n, 0] and pn.vsd_values(hidden[None]).tolist() == [[1.0]]
    # no observation anywhere: everything rendered is visible, for both poses
    moved = part["pose"].copy()
    moved[4] += 0.01                                                # 100 camera units sideways: the two renders overlap in part
    keys = []
    for p in (moved, part["pose"]):
        pv.verify_np(part["vertices"], part["triangles"], part["tri_begin"], part["model_scale"], part["proj"], np.zeros((1, VH, VW), np.uint16),
                     None, [[0, 0, 0, 0, 0, 0]], [p], pv.CLOUD_DIV, VH, VW, 0, 1, keys)
    re, rg = keys[0] != pv.NO_KEY, keys[1] != pv.NO_KEY
    blind = vsd_run(part, np.full((VH, VW), 65535), moved, part["pose"], [1e9])
    assert blind.tolist() == [0, int((re | rg).sum()), int((re & rg).sum()), int(re.sum()), 0] and 0 < blind[2] < blind[1]
    want = (blind[1] - blind[2]) / blind[1]
    assert pn.vsd_values(blind[None])[0, 0] == want


def test_vsd_of_a_pose_pushed_along_the_view_axis(part):
    """est 20 camera units farther than the truth, which the depth shows: every node of both renders is visible through vis_g, the nodes
    of est alone see the wall behind them; the gaps are about 20 (more where the shifted render shows another face at a step of the
    part), so tau = 10 counts all of inter and tau = 10 000, past the part's size, none."""
    on = part["codes"] != 65535
    depth = np.where(on, part["codes"], WALL)
    far = part["pose"].copy()
    far[6] -= SHIFT
    keys = []
    pv.verify_np(part["vertices"], part["triangles"], part["tri_begin"], part["model_scale"], part["proj"], np.zeros((1, VH, VW), np.uint16),
                 None, [[0, 0, 0, 0, 0, 0]], [far], pv.CLOUD_DIV, VH, VW, 0, 1, keys)
    re = keys[0] != pv.NO_KEY
    gaps = []
    row = vsd_run(part, depth, far, part["pose"], [10.0, 1e4], gaps=gaps)
    assert row.tolist() == [0, int((re | on).sum()), int((re & on).sum()), int(re.sum()), int((re & on).sum()), 0]
    assert len(gaps[0]) == row[2] and 15.0 < gaps[0].min() and 15.0 < float(np.median(gaps[0])) < 30.0 and gaps[0].max() < 1e4
    # a tau that sits exactly on a computed gap counts it (>=); the next double above does not
    g = float(np.sort(gaps[0])[len(gaps[0]) // 2])
    edge = vsd_run(part, depth, far, part["pose"], [g, float(np.nextafter(g, np.inf))])
    assert edge[4] - edge[5] == int((gaps[0] == g).sum()) >= 1 and edge[4] == int((gaps[0] >= g).sum())
    # the same pose without the truth's help: against a depth that shows nothing of the part (the wall alone) est is visible on its own
    alone = vsd_run(part, np.full((VH, VW), WALL), far, part["pose"], [10.0])
    assert alone[1] == int((re | on).sum()) and alone[2] == int((re & on).sum())
