"""GPU: ``df_mesh_icp`` against its restatement (tests/mesh_icp_np.py) bit for bit in pose_out and stats, its argument errors, the wrapper
``lib.mesh_icp.MeshIcp``, then what is built on it: ``RenderedPoseDataset.mesh_icp()`` on rendered views and
``tools/eval_cad_render.py --icp``.

The shapes are the smallest at which the kernels can go wrong (``mesh_icp_np.make_icp_cases``): a triangle range of 1 and on each side of
the 128-record LDS tile with the winner in its last triangle; N = 1, 5, 6 (below and at the six inliers), 63, 64, 65 (a wave's slots),
129 (a second scan workgroup), 513 (a third round of the 256 summing lanes); B = 1 and 3; 0, 1 and 4 steps; items of one call on
different ranges, one starting mid-tile, one empty; a call that mixes a normal item, too few inliers, one flat face, bad objects and a NaN
point."""
import importlib
import math
import os
import sys

import numpy as np
import pytest
import torch

import cad_raster_np as mnp
import cad_render_np as rnp
import fabricate_cad as fab
import mesh_closest_np as m
import mesh_icp_np as icp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# test_icp_on_rendered_views: the largest ADD to the true pose after 10 steps, over the diameter, that the restatement gave on those items
# (set by the 16-bit depth code of the rendered frames), times 2 for view-to-view spread
RENDERED_ADD_MEASURED = 1.82e-5
RENDERED_ADD_BOUND = 2 * RENDERED_ADD_MEASURED


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _up(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _device(case, iters=None, rows=None):
    """``df_mesh_icp`` itself on a case (or on the items ``rows`` of it): (pose_out, stats) as numpy."""
    from densefusion_amd import _lib
    L = _lib.lib()
    v, t, begin = icp.concat_meshes(case["meshes"])
    rows = list(range(len(case["obj"]))) if rows is None else list(rows)
    obj, pts, pose = np.asarray(case["obj"], np.int32)[rows], np.asarray(case["points"], np.float32)[rows], np.asarray(case["pose"], np.float64)[rows]
    B, N = pts.shape[:2]
    dv, dt, dobj, dpts, dpose = _up(v, np.float32), _up(t, np.int32), _up(obj, np.int32), _up(pts, np.float32), _up(pose, np.float64)
    md = np.ascontiguousarray(case["max_dist"], dtype=np.float64)
    need = L.df_mesh_icp_scratch_bytes(len(t), B, N)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    out, stats = torch.full((B, 7), 7.0, dtype=torch.float64, device="cuda"), torch.full((B, 6), 7.0, dtype=torch.float64, device="cuda")
    rc = L.df_mesh_icp(dv.data_ptr(), len(v), dt.data_ptr(), len(t), begin.ctypes.data, md.ctypes.data, len(begin) - 1, dobj.data_ptr(),
                       dpts.data_ptr(), dpose.data_ptr(), B, N, case["iters"] if iters is None else iters, case["cull"], out.data_ptr(),
                       stats.data_ptr(), scratch.data_ptr(), need, _lib.current_stream())
    assert rc == 0, L.df_last_error()
    return out.cpu().numpy(), stats.cpu().numpy()


def _same(got, want, name):
    for g, w, what in zip(got, want, ("pose_out", "stats")):
        assert m.same_bits(g, w), f"{name}: {what} differs\n{g}\n{w}"


@pytest.fixture(scope="module")
def cases():
    _dev()
    from densefusion_amd import _lib
    L = _lib.lib()
    assert L.df_mesh_icp_scratch_bytes(3, 2, 5) == 3 * 256 + 2 * 5 * 64 + 48 and L.df_mesh_icp_scratch_bytes(0, 2, 5) == 0
    assert L.df_mesh_icp_scratch_bytes(3, 0, 5) == 0 and L.df_mesh_icp_scratch_bytes(3, 2, -1) == 0
    made = icp.make_icp_cases(L.df_mesh_closest_tile_triangles())
    return made, {k: icp.run_case(c) for k, c in made.items()}                 # the restatement, once for every test


def test_bit_exact_on_every_small_shape(cases):
    made, want = cases
    for name in made:
        _same(_device(made[name]), want[name], name)
    assert all(want["T%d" % T][1][0, 0] == icp.DEGENERATE and want["T%d" % T][1][0, 1] == 65 for T in (1, 127, 128, 129))
    assert want["N5_B1_it4"][1][0, 0] == icp.FEW and want["N513_B1_it4"][1][0].tolist()[::5] == [icp.OK, 4]
    assert want["N65_B1_it0"][1][0, 5] == 0 and 0 < want["N65_B1_it0"][1][0, 1] < 65            # cull and max_dist took points away
    r = want["ranges"][1]
    assert r[:, 0].tolist() == [icp.OK, icp.DEGENERATE, icp.OK, icp.BAD_OBJECT, icp.DEGENERATE] and r[0, 4] < 1e-6 and r[2, 4] < 1e-6


def test_a_mixed_call_and_frozen_items(cases):
    made, want = cases
    case, (pose, stats) = made["mixed"], _device(made["mixed"])
    _same((pose, stats), want["mixed"], "mixed")
    assert stats[:, 0].tolist() == [icp.OK, icp.FEW, icp.DEGENERATE, icp.BAD_OBJECT, icp.BAD_OBJECT, icp.OK, icp.OK]
    assert stats[:, 1].tolist() == [70, 5, 70, 0, 0, 69, 70] and stats[:, 5].tolist() == [4, 0, 0, 0, 0, 4, 4]
    for b in (1, 2, 3, 4):                                                       # frozen at the first step: four more change nothing
        assert m.same_bits(pose[b], icp.normalised(case["pose"][b])), icp.MIXED[b]
    assert m.same_bits(pose[6], pose[0]) and m.same_bits(stats[6], stats[0]), "the same item in another position"
    assert not np.isnan(pose[5]).any() and stats[5, 4] < 1e-6
    # more steps on six points each: whichever step freezes an item, it is the restatement's
    one = _device(made["N6_B3_it1"], iters=3)
    _same(one, icp.run_case(made["N6_B3_it1"], iters=3), "N6 at 3 steps")


def test_an_item_does_not_depend_on_the_call_around_it(cases):
    made, want = cases
    case = made["mixed"]
    whole = _device(case)
    for rows in ([0], [5], [2, 0], [6, 5, 4, 3, 2, 1, 0]):
        part = _device(case, rows=rows)
        for k, b in enumerate(rows):
            assert m.same_bits(part[0][k], whole[0][b]) and m.same_bits(part[1][k], whole[1][b]), (rows, b)
    again = _device(case)
    assert m.same_bits(again[0], whole[0]) and m.same_bits(again[1], whole[1]), "two calls, the same bytes"
    r = made["ranges"]
    alone = _device(r, rows=[2])
    assert m.same_bits(alone[0][0], want["ranges"][0][2]) and m.same_bits(alone[1][0], want["ranges"][1][2])


def test_argument_errors_write_nothing(cases):
    from densefusion_amd import _lib
    L = _lib.lib()
    v, t = m.bracket()
    V, T, B, N = len(v), len(t), 2, 9
    dv, dt = _up(v, np.float32), _up(t, np.int32)
    obj, pts = _up([0, 0], np.int32), torch.rand(B, N, 3, device="cuda")
    pose = _up([[1, 0, 0, 0, 0, 0, 0]] * B, np.float64)
    begin, md = np.array([0, T], dtype=np.int32), np.array([1.0])
    out, stats = torch.full((B, 7), 7.0, dtype=torch.float64, device="cuda"), torch.full((B, 6), 7.0, dtype=torch.float64, device="cuda")
    need = L.df_mesh_icp_scratch_bytes(T, B, N)
    scratch = torch.full((need + 16,), 7, dtype=torch.uint8, device="cuda")
    good = dict(vertices=dv.data_ptr(), V=V, triangles=dt.data_ptr(), T=T, begin=begin.ctypes.data, md=md.ctypes.data, O=1, obj=obj.data_ptr(),
                points=pts.data_ptr(), pose=pose.data_ptr(), B=B, N=N, iters=2, cull=0, out=out.data_ptr(), stats=stats.data_ptr(),
                scratch=scratch.data_ptr(), scratch_bytes=need, stream=_lib.current_stream())
    big = 2 ** 31 - 1
    bad_begin = [np.array(a, dtype=np.int32) for a in ([0, T + 1], [-1, T], [5, 4])]
    bad_md = [np.array([a]) for a in (0.0, -1.0, float("nan"))]
    errors = [dict(vertices=None), dict(triangles=None), dict(begin=None), dict(md=None), dict(obj=None), dict(points=None), dict(pose=None),
              dict(out=None), dict(stats=None), dict(scratch=None), dict(V=0), dict(T=0), dict(B=0), dict(N=0), dict(V=-1), dict(N=-2),
              dict(V=big // 3 + 1), dict(T=big // 3 + 1), dict(N=big // (8 * B) + 1), dict(O=0), dict(O=65), dict(iters=-1), dict(iters=65),
              dict(cull=2), dict(cull=-1), dict(scratch_bytes=need - 1), dict(scratch_bytes=0), dict(scratch=scratch.data_ptr() + 8),
              dict(points=pts.data_ptr() + 2), dict(pose=pose.data_ptr() + 4), dict(out=out.data_ptr() + 4), dict(stats=stats.data_ptr() + 4),
              dict(out=pose.data_ptr()), dict(stats=pose.data_ptr()), dict(out=scratch.data_ptr()), dict(stats=out.data_ptr() + 8)]
    errors += [dict(begin=a.ctypes.data) for a in bad_begin] + [dict(md=a.ctypes.data) for a in bad_md]
    for kw in errors:
        a = dict(good, **kw)
        assert L.df_mesh_icp(*[a[k] for k in good]) == -1, kw                    # DF_ERR_ARG
        assert len(L.df_last_error()) > 10, kw
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((stats == 7).all()) and bool((scratch == 7).all()), "nothing was written"
    inf = np.array([float("inf")])
    assert L.df_mesh_icp(*[dict(good, md=inf.ctypes.data)[k] for k in good]) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7).any()) and bool((scratch[need:] == 7).all())


def test_the_wrapper(cases):
    from densefusion_amd.lib.mesh_icp import MeshIcp
    made, want = cases
    case = made["mixed"]
    fit = MeshIcp(case["meshes"])
    assert fit.n_objects == 1 and fit.tri_begin.tolist() == [0, 24] and fit.vertices.dtype == torch.float32 and fit.triangles.dtype == torch.int32
    keep = [0, 1, 2, 5, 6]
    pts, pose, obj = _up(case["points"][keep], np.float32), _up(case["pose"][keep], np.float64), _up(np.zeros(5), np.int64)
    got, stats = fit.refine(pts, pose, obj, iters=4)
    assert m.same_bits(got.cpu().numpy(), want["mixed"][0][keep]) and m.same_bits(stats.cpu().numpy(), want["mixed"][1][keep])
    # scales take the vertices into the clouds' units: half the mesh against half the cloud gives half the translation and the rms
    half = MeshIcp(case["meshes"], 0.5)
    hp = pose.clone()
    hp[:, 4:] *= 0.5
    got2, stats2 = half.refine((pts.double() * 0.5).float(), hp, obj.int(), iters=4, max_dist=[10.0])
    assert torch.allclose(got2[[0, 3, 4], :4], got[[0, 3, 4], :4], atol=1e-6) and torch.allclose(got2[[0, 3, 4], 4:], got[[0, 3, 4], 4:] * 0.5, atol=1e-6)
    assert stats2[:, 0].tolist() == stats[:, 0].tolist()
    two = MeshIcp([case["meshes"][0], m.scalene_tetrahedron()], [1.0, 2.0])
    assert two.tri_begin.tolist() == [0, 24, 28] and int(two.triangles[24:].min()) == len(case["meshes"][0][0])
    for bad in (dict(points=pts.cpu()), dict(points=pts.double()), dict(points=pts[:, :, :2]), dict(pose=pose.float()), dict(pose=pose[:4]),
                dict(pose=pose[:, :6]), dict(obj=obj[:3]), dict(obj=obj.float()), dict(obj=obj.cpu())):
        with pytest.raises(RuntimeError):
            fit.refine(**dict(dict(points=pts, pose=pose, obj=obj), **bad))
    for bad in (dict(iters=-1), dict(iters=65), dict(max_dist=0.0), dict(max_dist=[1.0, 2.0]), dict(max_dist=float("nan"))):
        with pytest.raises(ValueError):
            fit.refine(pts, pose, obj, **bad)
    with pytest.raises(ValueError):
        fit.refine(pts[:, :0], pose, obj)
    with pytest.raises(ValueError):
        MeshIcp([])
    with pytest.raises(ValueError):
        MeshIcp([(case["meshes"][0][0], np.array([[0, 1, len(case["meshes"][0][0])]]))])     # an index outside the vertices
    with pytest.raises(ValueError):
        MeshIcp(case["meshes"], [1.0, 2.0])
    with pytest.raises(ValueError):
        MeshIcp(case["meshes"], -1.0)


# ---- what is built on it ---------------------------------------------------------------------------------------------------------------------
VIEWS = 8
FRAME = dict(image_dims=(64, 96), min_pixels=60)


def _bracket_model():
    """the bracket in file units, sized like the fixtures of the rendered-scene tests (their spheres have radius 60)"""
    v, t = m.bracket()
    return (v * np.float32(30.0), t, np.random.default_rng(5).integers(0, 256, (len(v), 3), dtype=np.uint8))


def _third_face_cosine(pose):
    """Of the box's six faces seen from the camera of the true pose [R|t] (t in the units of ``transforms.txt`` x model_scale 10), the
    third largest cosine between a face's outward normal and the direction from its centre to the camera: > 0 when three faces show."""
    normals = np.array([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]], dtype=np.float64)
    centres = normals * np.array([15.0, 30.0, 45.0])
    o = -pose[:, :3].T @ pose[:, 3] / 10.0
    return sorted(float(n @ (o - c)) / float(np.linalg.norm(o - c)) for n, c in zip(normals, centres))[-3]


def test_icp_on_rendered_views():
    """Items of a rendered mesh dataset, started 5 degrees and 0.05 D from their true poses: the device equals the restatement on the
    downloaded points, and every item ends nearer the truth than it started and within ``RENDERED_ADD_BOUND`` of it.
    The eight views are the first of 128 that are served and show three faces of the box, the third at a cosine of 0.15 or more: a view
    of one or two flat faces does not hold six degrees of freedom, which the contract answers with `degenerate` and the pose kept
    (seen on the first run of this test: views of two faces).  The views are drawn without holes (``max_holes`` 1 draws none) for the same reason."""
    _dev()
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    np.random.seed(1)
    ds = RenderedPoseDataset(_bracket_model(), 500, False, 0.0, False, raster="mesh", proj_mat=fab.PROJ[1], chunk=16, first_seed=0, frames=128,
                             max_holes=1, **FRAME)
    fit = ds.mesh_icp()
    assert fit.n_objects == 1 and fit.tri_begin.tolist() == [0, 24]
    scale = ds.model_scale / 10000.0
    assert np.allclose(fit.vertices.cpu().numpy(), _bracket_model()[0] * scale, rtol=1e-6, atol=0)
    D = icp.diameter(fit.vertices.cpu().numpy())
    rng = np.random.default_rng(9)
    live = [i for i in range(128) if ds.view_info(i)["live"] and _third_face_cosine(ds.view_info(i)["pose"]) >= 0.15][:VIEWS]
    print("views:", live, "of", sum(bool(ds.view_info(i)["live"]) for i in range(128)), "served")
    assert len(live) == VIEWS
    clouds, truths, starts, models = [], [], [], []
    for i in live:
        cloud, _, _, target, model_points, idx = ds[i]
        info = ds.view_info(i)
        truth = np.concatenate([icp.quat_from_matrix(info["pose"][:, :3]), info["pose"][:, 3] / 10000.0])
        mp = model_points.reshape(-1, 3).double().cpu().numpy()
        assert np.abs(icp.apply_pose(truth, mp) - target.reshape(-1, 3).double().cpu().numpy()).max() < 1e-5 * D, "the true pose maps the model to the target"
        assert int(idx.reshape(-1)[0]) == 0
        clouds.append(cloud.reshape(-1, 3)); truths.append(truth); models.append(mp)
        starts.append(icp.perturb(truth, rng, math.radians(5), 0.05 * D))
    points, start = torch.stack(clouds).float().contiguous(), _up(np.stack(starts), np.float64)
    obj = torch.zeros(len(live), dtype=torch.int32, device="cuda")
    pose, stats = fit.refine(points, start, obj, iters=10)
    pose, stats = pose.cpu().numpy(), stats.cpu().numpy()
    want = icp.icp_np(fit.vertices.cpu().numpy(), fit.triangles.cpu().numpy(), fit.tri_begin, [icp.INF], [0] * len(live), points.cpu().numpy(),
                      np.stack(starts), 10)
    add0 = [icp.mean_point_error(starts[k], truths[k], models[k]) / D for k in range(len(live))]
    add = [icp.mean_point_error(pose[k], truths[k], models[k]) / D for k in range(len(live))]
    for k, i in enumerate(live):
        print(f"view {i}: status {stats[k, 0]:.0f} inliers {stats[k, 1]:.0f} -> {stats[k, 3]:.0f} rms/D {stats[k, 2] / D:.3e} -> {stats[k, 4] / D:.3e} "
              f"steps {stats[k, 5]:.0f} ADD/D {add0[k]:.3e} -> {add[k]:.3e}")
    print("largest ADD / D after ICP:", max(add), "bound:", RENDERED_ADD_BOUND)
    _same((pose, stats), want, "rendered views")
    assert all(a < b for a, b in zip(add, add0)), "every item ends nearer the truth than it started"
    assert max(add) <= RENDERED_ADD_BOUND
    cloud_ds = RenderedPoseDataset((np.random.default_rng(0).normal(size=(2000, 3)).astype(np.float32) * 30, None, np.full((2000, 3), 130, dtype=np.uint8)),
                                   500, False, 0.0, False, proj_mat=fab.PROJ[1], frames=4, **FRAME)
    with pytest.raises(ValueError, match="triangles"):
        cloud_ds.mesh_icp()


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return importlib.import_module(name)
    finally:
        sys.path.pop(0)


def test_the_tool_scores_each_source_with_and_without_icp(tmp_path):
    _dev()
    from densefusion_amd.lib.network import PoseNet, PoseRefineNet
    import cad_scene_np as snp
    paths = [str(mnp.write_mesh_ply(tmp_path / name, *mesh)) for name, mesh in zip(("big.ply", "small.ply", "box.ply"), snp.tool_meshes())]
    pm = rnp.write_proj(tmp_path / "proj_in.txt", fab.PROJ[1])
    torch.manual_seed(3)
    torch.save(PoseNet(num_points=500, num_obj=5).state_dict(), tmp_path / "pose.pth")
    torch.save(PoseRefineNet(num_points=500, num_obj=5).state_dict(), tmp_path / "refine.pth")
    tool = _tool("eval_cad_render")

    def run(out, *extra):
        return tool.main(["--cad_model", paths[0], paths[1], "--cad_distractor", paths[2], "--model", str(tmp_path / "pose.pth"), "--refine_model",
                          str(tmp_path / "refine.pth"), "--masks", "truth", "--cad_seed", "0", "--cad_frames", str(VIEWS), "--proj_mat", pm,
                          "--height", "64", "--width", "96", "--min_pixels", "60", "--mask", "pixels", "--chunk", "4", "--workers", "0",
                          "--iteration", "2", "--output_result_dir", str(tmp_path / out), *extra])

    plain, both = run("plain"), run("icp", "--icp", "3", "--icp_max_dist", "0.5")
    assert sorted(plain) == ["truth"] and sorted(both) == ["truth", "truth_icp"]
    assert both["truth"] == plain["truth"], "the plain entry does not change"
    log = open(tmp_path / "icp" / "eval_result_logs_truth.txt").read()
    assert log == open(tmp_path / "plain" / "eval_result_logs_truth.txt").read() and sorted(os.listdir(tmp_path / "plain")) == ["eval_result_logs_truth.txt"]
    t, r = both["truth"], both["truth_icp"]
    assert r["served"] == t["served"] and r["kept"] == t["kept"] and r["views"] == t["views"] and sum(r["served"]) >= 3
    c = r["icp"]
    assert c["items"] == sum(r["served"]) and 0 <= c["few"] + c["degenerate"] <= c["items"] and c["bad_object"] == 0
    assert math.isfinite(c["mean_first_rms"]) and math.isfinite(c["mean_last_rms"]) and c["mean_first_rms"] > 0 and "icp" not in t
    log = open(tmp_path / "icp" / "eval_result_logs_truth_icp.txt").read()
    assert "[truth_icp masks] ICP 3 steps: %d items, %d few inliers, %d degenerate" % (c["items"], c["few"], c["degenerate"]) in log
    assert "[truth_icp masks] ALL success rate:" in log and log.count("Distance: ") == sum(r["served"])
    with pytest.raises(SystemExit):
        run("bad", "--icp", "65")
