"""GPU: ``df_pose_sym_error`` against its restatement (tests/pose_error_np.py) bit for bit in all six columns, its argument errors, the
wrapper ``lib.pose_error.PoseErrors`` and ``RenderedPoseDataset.symmetry_sets()`` / ``pose_errors()``.

The shapes are the smallest at which the kernels can go wrong: V = 1, on each side of a wave (63, 64, 65), of a workgroup's lanes (255,
256, 257) and of a workgroup's sweep of two vertices per lane (511, 512, 513); a V past what an item's capped grid takes in one sweep, for
B = 1 and for B = 64, so that the stride loop runs twice; S = 1, 2, 3 and 630, once cut into symmetry slices (few workgroups) and once
in one slice of more than the 512 maxima a workgroup holds at a time (B = 64 next to a large mesh); B = 1 and 5 with three objects of
different V and S; a bad object, an empty vertex range and an empty symmetry range; a tie between two symmetries; a NaN pose and a
zero quaternion; a vertex behind the camera."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fabricate_cad as fab  # noqa: E402
import mesh_closest_np as m  # noqa: E402
import pose_error_np as pn  # noqa: E402

pytestmark = pytest.mark.gpu
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
FLIP = np.array([[-1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, 1.0, 0]])
FILL = 7.0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _up(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _call(v, vb, s, sb, obj, est, gt, proj=pn.PROJ, IH=pn.IH, IW=pn.IW, over=None):
    """``df_pose_sym_error`` itself: (return code, out as numpy); ``over`` replaces arguments of the C call by name, for the refusals"""
    from densefusion_amd import _lib
    L = _lib.lib()
    B = len(obj)
    vb, sb = np.ascontiguousarray(vb, dtype=np.int32), np.ascontiguousarray(sb, dtype=np.int32)
    proj = np.ascontiguousarray(proj, dtype=np.float64).reshape(-1)
    keep = [_up(v, np.float32), _up(np.asarray(s).reshape(-1, 12), np.float64), _up(obj, np.int32), _up(est, np.float64), _up(gt, np.float64)]
    S_max = max(1, int(np.diff(sb).max()))
    need = L.df_pose_sym_error_scratch_bytes(B, S_max)
    scratch = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")
    out = torch.full((B, 6), FILL, dtype=torch.float64, device="cuda")
    a = dict(vertices=keep[0].data_ptr(), V=len(v), vertex_begin=vb.ctypes.data, sym=keep[1].data_ptr(), NS=len(keep[1]), sym_begin=sb.ctypes.data,
             O=len(vb) - 1, obj=keep[2].data_ptr(), pose_est=keep[3].data_ptr(), pose_gt=keep[4].data_ptr(), B=B, proj=proj.ctypes.data, IH=IH, IW=IW,
             out=out.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=need, stream=_lib.current_stream())
    a.update(over or {})
    rc = L.df_pose_sym_error(*a.values())
    return rc, out.cpu().numpy()


def _check(name, v, vb, s, sb, obj, est, gt, **kw):
    rc, got = _call(v, vb, s, sb, obj, est, gt, **kw)
    assert rc == 0
    want = pn.sym_error_np(v, vb, s, sb, obj, est, gt, kw.get("proj", pn.PROJ), kw.get("IH", pn.IH), kw.get("IW", pn.IW))
    assert pn.same_bits(got, want), f"{name}: out differs\n{got}\n{want}"
    return got


def _cloud(n, rng, size=0.4):
    return (rng.uniform(-size, size, (n, 3))).astype(np.float32)


SETS = {1: IDENTITY[None], 2: pn.cyclic_set(2, (0, 0, 1), center=(0.01, -0.02, 0.03)), 3: pn.cyclic_set(3, (1, 2, 3)),
        630: pn.cyclic_set(315, (0.2, -0.1, 1.0), flip=True, center=(0.05, 0.0, -0.02))}


def _off(pose, rng, angle=0.2, shift=0.05):
    """poses a small rotation and shift away (unit quaternions are not needed)"""
    out = pose.copy()
    out[:, :4] += rng.normal(scale=angle, size=(len(pose), 4))
    out[:, 4:] += rng.normal(scale=shift, size=(len(pose), 3))
    return out


@pytest.mark.parametrize("V", [1, 63, 64, 65, 255, 256, 257, 511, 512, 513])
def test_bit_exact_on_every_small_vertex_count(V):
    _dev()
    rng = np.random.default_rng(V)
    for S in (1, 2, 3):
        v, vb, s, sb = pn.pack([_cloud(V, rng)], [SETS[S]])
        gt = pn.random_poses(1, rng)
        got = _check(f"V {V} S {S}", v, vb, s, sb, [0], _off(gt, rng), gt)
        assert got[0, 0] == 0 and got[0, 5] == V and got[0, 1] > 0 and np.isfinite(got[0, 3])


def test_the_whole_symmetry_set_in_slices():
    _dev()
    rng = np.random.default_rng(630)
    v, vb, s, sb = pn.pack([_cloud(257, rng)], [SETS[630]])
    gt = pn.random_poses(1, rng)
    got = _check("S 630 in slices", v, vb, s, sb, [0], _off(gt, rng, 0.8), gt)
    assert got[0, 2] != 0 or got[0, 4] != 0                          # a large turn: some other element than the identity is nearest


def test_a_mesh_past_one_sweep():
    """B = 1: the grid is capped at 256 vertex blocks; B = 64: at 32, and the symmetry set of the small object next to the large mesh
    then runs in one slice, past the 512 maxima a workgroup holds at a time"""
    _dev()
    from densefusion_amd import _lib
    L = _lib.lib()
    assert L.df_pose_sym_error_sweep_vertices(1) == 256 * 512 and L.df_pose_sym_error_sweep_vertices(64) == 32 * 512
    assert L.df_pose_sym_error_sweep_vertices(0) == 0 and L.df_pose_sym_error_sweep_vertices(65535) == 512
    rng = np.random.default_rng(3)
    V = L.df_pose_sym_error_sweep_vertices(1) + 3
    cloud = _cloud(V, rng)
    cloud[-1] = [3.0, -2.0, 1.0]                                      # the farthest vertex is the last: only the second sweep meets it
    v, vb, s, sb = pn.pack([cloud], [SETS[2]])
    gt = pn.random_poses(1, rng)
    _check("B 1 past a sweep", v, vb, s, sb, [0], _off(gt, rng), gt)
    V = L.df_pose_sym_error_sweep_vertices(64) + 3
    cloud = _cloud(V, rng)
    cloud[-1] = [3.0, -2.0, 1.0]
    v, vb, s, sb = pn.pack([cloud, _cloud(5, rng)], [SETS[1], SETS[630]])
    obj = [0] + [1] * 63
    gt = pn.random_poses(64, rng)
    got = _check("B 64 past a sweep", v, vb, s, sb, obj, _off(gt, rng, 0.8), gt)
    assert (got[1:, 2] >= 512).any(), "no item found its symmetry in the second tile: the case does not test it"


def _mixed(rng):
    clouds = [_cloud(300, rng), _cloud(70, rng), _cloud(5, rng), np.zeros((0, 3), np.float32), _cloud(9, rng)]
    sets = [SETS[3], SETS[630], SETS[1], SETS[2], np.zeros((0, 3, 4))]
    return pn.pack(clouds, sets)


def test_five_items_of_three_objects_and_every_bad_item():
    _dev()
    rng = np.random.default_rng(5)
    v, vb, s, sb = _mixed(rng)
    gt = pn.random_poses(5, rng)
    got = _check("B 5", v, vb, s, sb, [1, 0, 2, 0, 1], _off(gt, rng, 0.5), gt)
    assert got[:, 0].tolist() == [0] * 5 and got[:, 5].tolist() == [70, 300, 5, 300, 70]
    obj = [0, 5, -1, 3, 4, 2, 2 ** 31 - 1]                            # out of range twice and at INT_MAX, no vertex, no symmetry
    gt = pn.random_poses(len(obj), rng)
    got = _check("bad items", v, vb, s, sb, obj, _off(gt, rng), gt)
    assert got[:, 0].tolist() == [0, 1, 1, 1, 1, 0, 1] and not got[[1, 2, 3, 4, 6], 1:].any()


def test_rows_do_not_depend_on_their_neighbours():
    """the same items in another order, and each alone: equal bytes row by row"""
    _dev()
    rng = np.random.default_rng(8)
    v, vb, s, sb = _mixed(rng)
    obj = np.array([1, 0, 2, 3, 0, 1])
    gt = pn.random_poses(len(obj), rng)
    est = _off(gt, rng, 0.5)
    _, base = _call(v, vb, s, sb, obj, est, gt)
    order = np.array([4, 2, 5, 0, 3, 1])
    _, moved = _call(v, vb, s, sb, obj[order], est[order], gt[order])
    assert pn.same_bits(moved, base[order])
    for b in range(len(obj)):
        _, alone = _call(v, vb, s, sb, obj[b:b + 1], est[b:b + 1], gt[b:b + 1])
        assert pn.same_bits(alone[0], base[b]), b
    _, again = _call(v, vb, s, sb, obj, est, gt)
    assert pn.same_bits(again, base)


def test_ties_flips_nan_and_zero_quaternions():
    _dev()
    box, _ = m.box(6, 8, 2)
    v, vb, s, sb = pn.pack([box, box, box], [np.stack([FLIP, FLIP, IDENTITY]), np.stack([IDENTITY, FLIP]), IDENTITY[None]])
    quarter, back = [1.0, 0, 0, 1.0, 0.0, 0.0, -20.0], [1.0, 0, 0, -1.0, 0.0, 0.0, -20.0]   # exact quarter turns: est = gt o FLIP to the bit
    rng = np.random.default_rng(2)
    ordinary = pn.random_poses(1, rng)[0]
    nan = ordinary.copy()
    nan[5] = np.nan
    zero = ordinary.copy()
    zero[:4] = 0.0
    behind = [1.0, 0, 0, 0, 0.0, 0.0, 0.5]
    est = np.array([quarter, back, quarter, quarter, nan, ordinary, zero, behind, ordinary])
    gt = np.array([back, back, back, back, ordinary, nan, ordinary, back, behind])
    obj = [0, 0, 1, 2, 1, 1, 1, 2, 2]
    got = _check("ties", v, vb, s, sb, obj, est, gt)
    assert got[0].tolist() == [0, 0, 0, 0, 0, 24]                    # both flips give exactly 0: the lower s
    assert got[1].tolist() == [0, 0, 2, 0, 2, 24]                    # est = gt: only the identity, the last element
    assert got[2].tolist() == [0, 0, 1, 0, 1, 24]
    assert got[3, 1] == 10.0 and got[3, 2] == 0                      # without the flip: the xy diagonal of half extents 3 and 4, twice
    for b in (4, 5):
        assert np.isposinf(got[b, 1]) and np.isposinf(got[b, 3]) and got[b, 2] == 0 and got[b, 4] == 0
    assert np.isfinite(got[6, 1]) and got[6, 1] > 0                  # a zero quaternion is the identity rotation
    for b in (7, 8):
        assert np.isfinite(got[b, 1]) and np.isposinf(got[b, 3])     # a vertex at or behind the camera plane has no pixel


def test_every_refusal_leaves_out_untouched():
    _dev()
    from densefusion_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(4)
    v, vb, s, sb = pn.pack([_cloud(10, rng), _cloud(4, rng)], [SETS[2], SETS[3]])
    gt = pn.random_poses(2, rng)
    base = (v, vb, s, sb, [0, 1], _off(gt, rng), gt)
    assert _call(*base)[0] == 0
    assert L.df_pose_sym_error_scratch_bytes(2, 3) == 2 * 3 * 16 + (2 * 3 + 2) * 96
    assert L.df_pose_sym_error_scratch_bytes(0, 3) == 0 and L.df_pose_sym_error_scratch_bytes(65536, 3) == 0 and L.df_pose_sym_error_scratch_bytes(2, 0) == 0
    bad_proj = pn.PROJ.copy().reshape(-1)
    bad_proj[14] = 1.0
    down, past = np.array([0, 11, 10], dtype=np.int32), np.array([0, 10, 15], dtype=np.int32)
    sdown, spast = np.array([0, 3, 2], dtype=np.int32), np.array([0, 2, 6], dtype=np.int32)
    some = torch.zeros(64, dtype=torch.float64, device="cuda")
    refusals = [dict(vertices=None), dict(vertex_begin=None), dict(sym=None), dict(sym_begin=None), dict(obj=None), dict(pose_est=None),
                dict(pose_gt=None), dict(proj=None), dict(out=None), dict(scratch=None), dict(V=0), dict(NS=0), dict(V=2 ** 31 // 3 + 1),
                dict(NS=2 ** 31 // 12 + 1), dict(B=0), dict(B=65536), dict(O=0), dict(O=65), dict(IH=0), dict(IW=0), dict(IH=2 ** 16, IW=2 ** 15),
                dict(proj=bad_proj.ctypes.data), dict(vertex_begin=down.ctypes.data), dict(vertex_begin=past.ctypes.data),
                dict(sym_begin=sdown.ctypes.data), dict(sym_begin=spast.ctypes.data), dict(scratch_bytes=L.df_pose_sym_error_scratch_bytes(2, 3) - 1),
                dict(pose_est=some.data_ptr() + 4), dict(sym=some.data_ptr() + 4), dict(vertices=some.data_ptr() + 2)]
    for over in refusals:
        rc, out = _call(*base, over=over)
        if "out" not in over:
            assert rc == -1 and (out == FILL).all(), over
        else:
            assert rc == -1, over
        assert L.df_last_error()
    # misaligned scratch and an out that overlaps an input
    est = _up(base[5], np.float64)
    rc, _ = _call(*base, over=dict(pose_est=est.data_ptr(), out=est.data_ptr()))
    assert rc == -1 and pn.same_bits(est.cpu().numpy(), base[5])
    scratch = torch.empty(4096, dtype=torch.uint8, device="cuda")
    rc, out = _call(*base, over=dict(scratch=scratch.data_ptr() + 4, scratch_bytes=4000))
    assert rc == -1 and (out == FILL).all() and L.df_last_error()


def test_the_wrapper_and_its_argument_errors():
    _dev()
    from densefusion_amd.lib.mesh_set import MeshSet
    from densefusion_amd.lib.pose_error import STATS, PoseErrors
    assert STATS == pn.STATS
    bv, bt = m.box(6, 8, 2)
    pv_, pt = m.prism(5, 3, 2)
    ms = MeshSet([(bv, bt), (pv_, pt)])
    scale, div = 10.0, 10000.0
    sets = [np.stack([IDENTITY, FLIP]), pn.cyclic_set(5)]
    pe = PoseErrors(ms, scale, sets, pn.PROJ, (pn.IH, pn.IW), cloud_div=div)
    assert np.array_equal(pe.vertices.cpu().numpy(), ms.scaled(scale / div)) and pe.sym_begin.tolist() == [0, 2, 7] and pe.sym_max == 5
    rng = np.random.default_rng(6)
    gt = pn.random_poses(4, rng, depth=(-0.08, -0.04), lateral=0.005)
    est = _off(gt, rng, 0.3, 0.002)
    obj = np.array([0, 1, 1, 0])
    got = pe.sym_error(_up(est, np.float64), _up(gt, np.float64), _up(obj, np.int64)).cpu().numpy()
    want = pn.sym_error_np(ms.scaled(scale / div), ms.vertex_begin, np.concatenate(sets), pe.sym_begin, obj, est, gt, pn.PROJ, pn.IH, pn.IW)
    assert pn.same_bits(got, want) and (got[:, 0] == 0).all()
    with pytest.raises(RuntimeError, match="pose_est"):
        pe.sym_error(_up(est, np.float32), _up(gt, np.float64), _up(obj, np.int64))
    with pytest.raises(RuntimeError, match="pose_gt"):
        pe.sym_error(_up(est, np.float64), _up(gt[:3], np.float64), _up(obj, np.int64))
    with pytest.raises(RuntimeError, match="obj"):
        pe.sym_error(_up(est, np.float64), _up(gt, np.float64), torch.from_numpy(obj))
    with pytest.raises(ValueError):
        pe.sym_error(_up(est[:0], np.float64), _up(gt[:0], np.float64), _up(obj[:0], np.int64))
    with pytest.raises(ValueError):
        PoseErrors(ms, scale, sets[:1], pn.PROJ, (pn.IH, pn.IW))
    with pytest.raises(ValueError):
        PoseErrors(ms, scale, [sets[0], np.zeros((0, 3, 4))], pn.PROJ, (pn.IH, pn.IW))
    with pytest.raises(RuntimeError):
        PoseErrors(ms, scale, sets, pn.PROJ, (pn.IH, pn.IW), device="cpu")


def test_the_datasets_sets_and_errors():
    """``symmetry="auto"`` on a box: its four rotations in cloud units from the report the ADD-S list was made from; the true pose of a
    served view turned by a symmetry costs nothing, and the same pose scored without the set costs the box's diagonal."""
    _dev()
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    bv, bt = m.box(1, 2, 3)
    model = (bv * np.float32(30.0), bt, np.full((len(bv), 3), 130, dtype=np.uint8))
    frame = dict(image_dims=(64, 96), min_pixels=60)
    ds = RenderedPoseDataset(model, 500, False, 0.0, False, raster="mesh", proj_mat=fab.PROJ[1], chunk=8, first_seed=0, frames=8, max_holes=1,
                             symmetry="auto", **frame)
    assert ds.get_sym_list() == [0]
    sets = ds.symmetry_sets()
    assert len(sets) == 1 and sets[0].shape == (4, 3, 4) and np.array_equal(sets[0][0], IDENTITY)
    assert np.allclose(sets[0][:, :, 3], 0, atol=1e-12)              # the box is centred: c - R c is zero to rounding, in any units
    plain = RenderedPoseDataset(model, 500, False, 0.0, False, raster="mesh", proj_mat=fab.PROJ[1], chunk=8, first_seed=0, frames=8, max_holes=1, **frame)
    assert [x.tolist() for x in plain.symmetry_sets()] == [IDENTITY[None].tolist()]
    listed = RenderedPoseDataset(model, 500, False, 0.0, False, raster="mesh", proj_mat=fab.PROJ[1], chunk=8, first_seed=0, frames=8, max_holes=1,
                                 symmetry=[0], **frame)
    with pytest.raises(ValueError, match="auto"):
        listed.symmetry_sets()
    pe, alone = ds.pose_errors(), plain.pose_errors()
    assert pe.sym_max == 4 and alone.sym_max == 1 and pe.image_dims == (64, 96)
    pose = np.array([0.3, -0.2, 0.5, 0.7, 0.001, -0.002, -0.4])        # the box is 0.03 x 0.06 x 0.09 in these units: all of it in front
    R = np.array(pn.icp.quat_to_mat(pose[:4]))
    turned = np.concatenate([pn.quat_of(R @ sets[0][2, :, :3]), pose[4:]])
    est, gt, obj = _up([turned], np.float64), _up([pose], np.float64), _up([0], np.int64)
    with_set, without = pe.sym_error(est, gt, obj).cpu().numpy()[0], alone.sym_error(est, gt, obj).cpu().numpy()[0]
    assert with_set[0] == 0 and with_set[1] < 1e-12 and with_set[2] == 2 and with_set[3] < 1e-6 and with_set[5] == 24
    assert without[1] > 0.005 and without[2] == 0                    # a half turn of a 30 x 60 x 90 box, in units of 1 / 1000: centimetres
    cloud_ds = RenderedPoseDataset((np.random.default_rng(0).normal(size=(2000, 3)).astype(np.float32) * 30, None, np.full((2000, 3), 130, dtype=np.uint8)),
                                   500, False, 0.0, False, proj_mat=fab.PROJ[1], frames=4, **frame)
    with pytest.raises(ValueError, match="mesh"):
        cloud_ds.pose_errors()


def test_the_symmetry_tool_prints_the_set_sizes(tmp_path, capsys):
    _dev()
    import importlib

    import cad_raster_np as mnp
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [str(mnp.write_mesh_ply(tmp_path / name, *mesh)) for name, mesh in (("box.ply", m.box(1, 2, 3)), ("bracket.ply", m.bracket()))]
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        tool = importlib.import_module("cad_symmetry")
    finally:
        sys.path.pop(0)
    reports = tool.main(["--model", *paths, "--no_color", "--write", str(tmp_path / "tree")])
    text = capsys.readouterr().out
    assert [r.symmetric for r in reports] == [True, False]
    assert text.count("symmetry set: 4 rotations") == 1 and text.count("symmetry set: 1 rotations") == 1
    assert "symmetry set: 4 rotations" in open(tmp_path / "tree" / "data" / "01" / "meta" / "symmetry.txt").read()


# ---- df_pose_vsd ----------------------------------------------------------------------------------------------------------------------------
import mesh_icp_np as icp  # noqa: E402
import pose_verify_np as pv  # noqa: E402


def _rays(proj, IH, IW):
    from densefusion_amd.datasets.customCAD.project_unity_depth import UnityDepthProjector
    return UnityDepthProjector.from_matrix(np.asarray(proj, dtype=np.float64).reshape(4, 4), (IH, IW)).ray_map


def _vsd_call(sc, rays, items, est, gt, delta, tau, WH, WW, cull=0, over=None):
    """``df_pose_vsd`` itself on a scene of tests/pose_verify_np.py: (return code, stats as numpy)"""
    from densefusion_amd import _lib
    L = _lib.lib()
    B, O = len(items), len(sc["tri_begin"]) - 1
    tau = np.ascontiguousarray(np.broadcast_to(np.asarray(tau, dtype=np.float64).reshape(-1, np.asarray(tau).shape[-1]), (O, np.asarray(tau).shape[-1])))
    delta = np.ascontiguousarray(np.broadcast_to(np.asarray(delta, dtype=np.float64).reshape(-1), (O,)))
    NT = tau.shape[1]
    F, IH, IW = sc["depth"].shape
    keep = [_up(sc["vertices"], np.float32), _up(sc["triangles"], np.int32), _up(sc["depth"], np.uint16), _up(rays, np.float64), _up(items, np.int32),
            _up(est, np.float64), _up(gt, np.float64)]
    begin, scale = np.ascontiguousarray(sc["tri_begin"], dtype=np.int32), np.ascontiguousarray(sc["model_scale"], dtype=np.float64)
    proj = np.ascontiguousarray(sc["proj"], dtype=np.float64).reshape(-1)
    need = L.df_pose_vsd_scratch_bytes(B, WH, WW)
    scratch = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")
    stats = torch.full((B, 4 + NT), 7, dtype=torch.int64, device="cuda")
    a = dict(vertices=keep[0].data_ptr(), V=len(sc["vertices"]), triangles=keep[1].data_ptr(), T=len(sc["triangles"]), tri_begin=begin.ctypes.data,
             model_scale=scale.ctypes.data, O=O, proj=proj.ctypes.data, depth=keep[2].data_ptr(), F=F, IH=IH, IW=IW, rays=keep[3].data_ptr(),
             items=keep[4].data_ptr(), pose_est=keep[5].data_ptr(), pose_gt=keep[6].data_ptr(), cloud_div=pv.CLOUD_DIV, delta=delta.ctypes.data,
             tau=tau.ctypes.data, NT=NT, B=B, WH=WH, WW=WW, cull=cull, stats=stats.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=need,
             stream=_lib.current_stream())
    a.update(over or {})
    rc = L.df_pose_vsd(*a.values())
    return rc, stats.cpu().numpy()


def _vsd_check(name, sc, rays, items, est, gt, delta, tau, WH, WW, cull=0, gaps=None):
    rc, got = _vsd_call(sc, rays, items, est, gt, delta, tau, WH, WW, cull)
    assert rc == 0
    O = len(sc["tri_begin"]) - 1
    tau2 = np.broadcast_to(np.asarray(tau, dtype=np.float64).reshape(-1, np.asarray(tau).shape[-1]), (O, np.asarray(tau).shape[-1]))
    want = pn.vsd_np(sc["vertices"], sc["triangles"], sc["tri_begin"], sc["model_scale"], sc["proj"], sc["depth"], rays, items, est, gt, pv.CLOUD_DIV,
                     np.broadcast_to(np.asarray(delta, dtype=np.float64).reshape(-1), (O,)), tau2, WH, WW, cull, gaps)
    assert np.array_equal(got, want), f"{name}: stats differ\n{got}\n{want}"
    return got


def _verify_device(sc, items, pose, WH, WW, tol, cull):
    from densefusion_amd import _lib
    L = _lib.lib()
    B = len(items)
    F, IH, IW = sc["depth"].shape
    keep = [_up(sc["vertices"], np.float32), _up(sc["triangles"], np.int32), _up(sc["depth"], np.uint16), _up(sc["mask"], np.uint16), _up(items, np.int32),
            _up(pose, np.float64)]
    begin, scale = np.ascontiguousarray(sc["tri_begin"], dtype=np.int32), np.ascontiguousarray(sc["model_scale"], dtype=np.float64)
    proj = np.ascontiguousarray(sc["proj"], dtype=np.float64).reshape(-1)
    need = L.df_pose_verify_scratch_bytes(B, WH, WW)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    stats = torch.full((B, 12), 7, dtype=torch.int64, device="cuda")
    rc = L.df_pose_verify(keep[0].data_ptr(), len(sc["vertices"]), keep[1].data_ptr(), len(sc["triangles"]), begin.ctypes.data, scale.ctypes.data,
                          len(begin) - 1, proj.ctypes.data, keep[2].data_ptr(), F, IH, IW, keep[3].data_ptr(), len(sc["mask"]), keep[4].data_ptr(),
                          keep[5].data_ptr(), pv.CLOUD_DIV, B, WH, WW, tol, cull, stats.data_ptr(), scratch.data_ptr(), need, _lib.current_stream())
    assert rc == 0
    return stats.cpu().numpy()


@pytest.mark.parametrize("config,WH,WW,NT", [("a", 20, 28, 1), ("b", 33, 17, 16)])
def test_vsd_on_windows_over_every_edge_and_verify_unchanged_around_it(config, WH, WW, NT):
    """The scenes and calls of the verification tests: windows at the origin, inside, over each edge and corner and wholly outside, four
    objects (one range empty), bad frames and objects; NT = 1 and 16.  ``df_pose_verify`` on the same items before and after gives the
    restatement's bytes both times."""
    _dev()
    sc = pv.make_scene(config)
    rays = _rays(sc["proj"], pv.IH, pv.IW)
    items, est = pv.make_call(24, WH, WW, seed=11)
    gt = est + np.concatenate([np.random.default_rng(12).normal(scale=0.05, size=(24, 4)), np.random.default_rng(13).normal(scale=0.002, size=(24, 3))], axis=1)
    gt[0] = est[0]                                                   # item 0: est = gt on the frame that shows it
    items[5, 0], items[6, 1] = pv.F, pv.O                            # a bad frame, a bad object
    want_verify = pv.verify_np(sc["vertices"], sc["triangles"], sc["tri_begin"], sc["model_scale"], sc["proj"], sc["depth"], sc["mask"], items, est,
                               pv.CLOUD_DIV, WH, WW, 4, 1)
    items_v = items.copy()
    before = _verify_device(sc, items_v, est, WH, WW, 4, 1)
    tau = np.linspace(5.0, 400.0, NT) if NT > 1 else np.array([40.0])
    got = _vsd_check(f"{config} {WH}x{WW}", sc, rays, items, est, gt, [30.0, 20.0, 25.0, 15.0], tau, WH, WW, cull=1)
    after = _verify_device(sc, items_v, est, WH, WW, 4, 1)
    assert np.array_equal(before, want_verify) and np.array_equal(after, want_verify)
    assert got[5, 0] == 1 and got[6, 0] == 1 and not got[5, 1:].any() and not got[6, 1:].any()
    outside = [k for k in range(24) if k % 12 >= 8 and k not in (5, 6)]
    assert not got[outside].any()                                    # a window wholly outside the frame: a row of zeros
    assert got[0, 1] == got[0, 2] > 0 or config == "b"               # est = gt on its own noisy frame: what is visible is visible for both
    assert (got[:, 4:] >= 0).all() and (np.diff(got[:, 4:], axis=1) <= 0).all() and (got[:, 2] <= got[:, 1]).all()


@pytest.fixture(scope="module")
def wall_part():
    """the bracket in front of a wall, as tests/test_pose_verify_host.py and the host VSD tests have it"""
    _dev()
    IH, IW, WALL = 64, 96, 60000
    v, t = m.bracket()
    q = icp.quat_mul(icp.quat_from_axis_angle([0, 1, 0], 0.6), icp.quat_from_axis_angle([1, 0, 0], 0.5))
    sc = dict(vertices=v * np.float32(30.0), triangles=t, tri_begin=np.array([0, len(t)], np.int32), model_scale=np.array([10.0]),
              proj=np.array(fab.PROJ[1]), pose=np.concatenate([q, [0.004, -0.003, -0.28]]))
    sc["rays"] = _rays(sc["proj"], IH, IW)
    keys = []
    pv.verify_np(sc["vertices"], t, sc["tri_begin"], sc["model_scale"], sc["proj"], np.full((1, IH, IW), WALL, np.uint16), None,
                 [[0, 0, 0, 0, 0, 65535]], [sc["pose"]], pv.CLOUD_DIV, IH, IW, 1, 1, keys)
    codes = pv.rendered_codes(keys[0], 0, 0, IH, IW)
    on = codes != 65535
    far = sc["pose"].copy()
    far[6] -= 0.002
    # frames: the part before the wall; an occluder 3 000 codes nearer over the whole part; nothing observed; the wall alone
    sc["depth"] = np.stack([np.where(on, codes, WALL), np.where(on, codes - 3000, WALL), np.full((IH, IW), 65535), np.full((IH, IW), WALL)]).astype(np.uint16)
    sc["on"], sc["far"], sc["dims"] = on, far, (IH, IW)
    return sc


def test_vsd_on_the_wall_and_occluder_frames(wall_part):
    sc = wall_part
    IH, IW = sc["dims"]
    n = int(sc["on"].sum())
    items = np.array([[f, 0, 0, 0, 0, 0] for f in (0, 1, 2, 3, 0)], dtype=np.int32)
    est = np.stack([sc["pose"], sc["pose"], sc["far"], sc["far"], sc["far"]])
    gt = np.stack([sc["pose"]] * 5)
    gaps = []
    got = _vsd_check("wall", sc, sc["rays"], items, est, gt, [15.0], [0.0, 10.0, 1e4], IH, IW, cull=1, gaps=gaps)
    assert got[0].tolist() == [0, n, n, n, n, 0, 0]                  # est = gt: union = inter > 0 and no gap reaches a positive tau
    assert got[1].tolist() == [0, 0, 0, n, 0, 0, 0]                  # the occluder is nearer than both renders by more than delta
    assert got[2, 1] > got[2, 2] > 0 and got[2, 5] == got[2, 2]      # nothing observed: everything rendered is visible
    assert got[4, 5] == got[4, 2] > 0 and got[4, 6] == 0
    from densefusion_amd.lib.pose_error import vsd_values
    vals = vsd_values(got)
    assert np.array_equal(vals, pn.vsd_values(got)) and vals[0].tolist() == [1.0, 0.0, 0.0] and vals[1].tolist() == [1.0, 1.0, 1.0]
    assert np.array_equal(vsd_values(torch.from_numpy(got)).numpy(), vals)
    # tau exactly on a computed |D_g - D_e| (the restatement supplies it): >= counts it, the next double above does not
    g = float(np.sort(gaps[4])[len(gaps[4]) // 2])
    edge = _vsd_check("edge", sc, sc["rays"], items[4:], est[4:], gt[4:], [15.0], [g, float(np.nextafter(g, np.inf))], IH, IW, cull=1)
    assert edge[0, 4] - edge[0, 5] == int((gaps[4] == g).sum()) >= 1


def test_vsd_refusals_leave_stats_untouched(wall_part):
    sc = wall_part
    IH, IW = sc["dims"]
    items, pose = np.array([[0, 0, 0, 0, 0, 0]], dtype=np.int32), sc["pose"][None]
    base = (sc, sc["rays"], items, pose, pose, [15.0], [1.0, 2.0], IH, IW)
    assert _vsd_call(*base)[0] == 0
    from densefusion_amd import _lib
    L = _lib.lib()
    assert L.df_pose_vsd_scratch_bytes(2, 3, 5) == 2 * 2 * 15 * 8 + 2 * 12 * 8 + 64 * 17 * 8 and L.df_pose_vsd_scratch_bytes(0, 3, 5) == 0
    bad_tau, neg_tau, nan_delta = np.array([2.0, 1.0]), np.array([-1.0, 2.0]), np.array([np.nan])
    for over in [dict(rays=None), dict(pose_est=None), dict(pose_gt=None), dict(delta=None), dict(tau=None), dict(depth=None), dict(scratch=None),
                 dict(NT=0), dict(NT=17), dict(B=0), dict(WH=0), dict(O=0), dict(O=65), dict(cull=2), dict(cloud_div=0.0), dict(V=0), dict(F=0),
                 dict(tau=bad_tau.ctypes.data), dict(tau=neg_tau.ctypes.data), dict(delta=nan_delta.ctypes.data), dict(scratch_bytes=8)]:
        rc, stats = _vsd_call(*base, over=over)
        assert rc == -1 and (stats == 7).all() and L.df_last_error(), over


def test_the_vsd_wrapper_on_rendered_views():
    """Eight rendered views of the bracket (the dataset keeps its frames): est = gt gives union = inter > 0 and every bad_k = 0; start
    poses a few degrees and millimetres off give the restatement's tallies on the downloaded frames; argument errors come before any
    launch; without ``keep_frames`` ``.vsd`` raises."""
    _dev()
    tool_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tool_dir)
    try:
        import importlib
        tool = importlib.import_module("eval_cad_render")
    finally:
        sys.path.pop(0)
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    v, t = m.bracket()
    model = (v * np.float32(30.0), t, np.random.default_rng(5).integers(0, 256, (len(v), 3), dtype=np.uint8))
    kw = dict(raster="mesh", proj_mat=fab.PROJ[1], chunk=16, first_seed=0, frames=64, max_holes=1, image_dims=(64, 96), min_pixels=60)
    np.random.seed(1)
    ds = RenderedPoseDataset(model, 500, False, 0.0, False, keep_frames=True, **kw)
    live = [i for i in range(64) if ds.view_info(i)["live"]][:8]
    assert len(live) == 8
    pe = ds.pose_errors()
    infos = [ds.view_info(i) for i in live]
    depth = torch.stack([f["depth"] for f in infos])
    gt = np.stack([tool.true_pose(ds, i) for i in live])
    rng = np.random.default_rng(9)
    start = gt + np.concatenate([rng.normal(scale=0.03, size=(8, 4)), rng.normal(scale=0.0005, size=(8, 3))], axis=1)
    margin = 8
    window = (max(f["box"][1] - f["box"][0] for f in infos) + 2 * margin, max(f["box"][3] - f["box"][2] for f in infos) + 2 * margin)
    corner = np.array([[f["box"][0] - margin, f["box"][2] - margin] for f in infos])
    frame, obj = np.arange(8), np.zeros(8, dtype=np.int64)
    D = tool.mesh_diameter(pe.vertices.cpu().numpy(), pe.device) * 10000.0      # camera units
    delta, tau = [0.075 * D], np.array([0.05 * k * D for k in range(1, 11)])
    sc = dict(vertices=ds.meshes.vertices, triangles=ds.meshes.triangles, tri_begin=ds.meshes.tri_begin, model_scale=np.array([ds.model_scale]),
              proj=ds.proj_mat, depth=depth.cpu().numpy())
    items = np.concatenate([frame[:, None], obj[:, None], corner, np.zeros((8, 2), dtype=np.int64)], axis=1)
    for name, est in (("true", gt), ("start", start)):
        got = pe.vsd(depth, _up(est, np.float64), _up(gt, np.float64), _up(frame, np.int64), _up(obj, np.int64), _up(corner, np.int64), window, delta, tau,
                     cull=bool(ds.cull)).cpu().numpy()
        want = pn.vsd_np(sc["vertices"], sc["triangles"], sc["tri_begin"], sc["model_scale"], sc["proj"], sc["depth"], ds.udp.ray_map, items, est, gt,
                         10000.0, delta, tau[None], window[0], window[1], int(bool(ds.cull)))
        assert np.array_equal(got, want), name
        if name == "true":
            assert (got[:, 0] == 0).all() and (got[:, 1] == got[:, 2]).all() and (got[:, 1] > 0).all() and not got[:, 4:].any()
    args = (depth, _up(gt, np.float64), _up(gt, np.float64), _up(frame, np.int64), _up(obj, np.int64), _up(corner, np.int64), window)
    with pytest.raises(ValueError):
        pe.vsd(*args, delta, tau[::-1].copy())
    with pytest.raises(ValueError):
        pe.vsd(*args, delta, np.arange(17.0))
    with pytest.raises(RuntimeError, match="pose_gt"):
        pe.vsd(depth, _up(gt, np.float64), _up(gt, np.float32), *args[3:], delta, tau)
    np.random.seed(1)
    plain = RenderedPoseDataset(model, 500, False, 0.0, False, **kw).pose_errors()
    with pytest.raises(ValueError, match="keep_frames"):
        plain.vsd(*args, delta, tau)
