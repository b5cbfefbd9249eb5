"""GPU: what is built on ``df_pose_verify``: ``RenderedPoseDataset(keep_frames=True)`` and ``pose_verifier()``, ``evaluate(select_pose=)``,
``tools/eval_cad_render.py --verify`` and the choice between the refiner's pose and the ICP pose on rendered views."""
import argparse
import importlib
import io
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
import pose_verify_np as pv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS = 8
FRAME = dict(image_dims=(64, 96), min_pixels=60)
TOL, MARGIN = 4, 8                                               # the tool's defaults


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bracket_model():
    v, t = m.bracket()
    return (v * np.float32(30.0), t, np.random.default_rng(5).integers(0, 256, (len(v), 3), dtype=np.uint8))


def _third_face_cosine(pose):
    """the selection rule of test_mesh_icp_gpu.test_icp_on_rendered_views: > 0 when three faces of the box show"""
    normals = np.array([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]], dtype=np.float64)
    centres = normals * np.array([15.0, 30.0, 45.0])
    o = -pose[:, :3].T @ pose[:, 3] / 10.0
    return sorted(float(n @ (o - c)) / float(np.linalg.norm(o - c)) for n, c in zip(normals, centres))[-3]


def _dataset(frames=128, chunk=16, **kw):
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    np.random.seed(1)
    return RenderedPoseDataset(_bracket_model(), 500, False, 0.0, False, raster="mesh", proj_mat=fab.PROJ[1], chunk=chunk, first_seed=0,
                               frames=frames, max_holes=1, **FRAME, **kw)


def test_keep_frames_changes_no_item():
    _dev()
    plain, kept = _dataset(16, 8), _dataset(16, 8, keep_frames=True)
    served = 0
    for i in range(16):
        a, b = plain[i], kept[i]
        assert len(a) == len(b) == 6
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), f"item {i} differs with keep_frames"
        info, base = kept.view_info(i), plain.view_info(i)
        assert "depth" not in base and "mask" not in base and "box" not in base
        assert info["depth"].shape == info["mask"].shape == (64, 96) and info["depth"].dtype == info["mask"].dtype == torch.uint16 and info["depth"].is_cuda
        assert tuple(info["box"]) == tuple(int(x) for x in info["table"][2:6])
        served += bool(info["live"])
    assert served >= 4
    ver = kept.pose_verifier()
    assert ver.n_objects == 1 and ver.tri_begin.tolist() == [0, 24] and ver.cloud_div == 10000.0 and ver.model_scales.tolist() == [kept.model_scale]
    assert np.array_equal(ver.vertices.cpu().numpy(), _bracket_model()[0]), "vertices stay in file units"
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    cloud_ds = RenderedPoseDataset((np.random.default_rng(0).normal(size=(2000, 3)).astype(np.float32) * 30, None, np.full((2000, 3), 130, dtype=np.uint8)),
                                   500, False, 0.0, False, proj_mat=fab.PROJ[1], frames=4, **FRAME)
    with pytest.raises(ValueError, match="triangles"):
        cloud_ds.pose_verifier()


def test_icp_pose_is_chosen_on_rendered_views():
    """The eight views of test_icp_on_rendered_views, started 5 degrees and 0.05 D off and refined by 10 ICP steps: the device tallies
    equal the restatement's on the downloaded frames, vsiou rises on every view, ``better`` takes the ICP pose on all eight, and with
    the candidates swapped the same poses are chosen."""
    _dev()
    from densefusion_amd.lib.pose_verify import better, vsiou
    ds = _dataset(keep_frames=True)
    fit, ver = ds.mesh_icp(), ds.pose_verifier()
    D = icp.diameter(fit.vertices.cpu().numpy())
    rng = np.random.default_rng(9)
    live = [i for i in range(128) if ds.view_info(i)["live"] and _third_face_cosine(ds.view_info(i)["pose"]) >= 0.15][:VIEWS]
    assert len(live) == VIEWS
    clouds, starts = [], []
    for i in live:
        info = ds.view_info(i)
        truth = np.concatenate([icp.quat_from_matrix(info["pose"][:, :3]), info["pose"][:, 3] / 10000.0])
        clouds.append(ds[i][0].reshape(-1, 3))
        starts.append(icp.perturb(truth, rng, math.radians(5), 0.05 * D))
    before = torch.from_numpy(np.stack(starts)).cuda()
    obj = torch.zeros(VIEWS, dtype=torch.int32, device="cuda")
    after, _ = fit.refine(torch.stack(clouds).float().contiguous(), before, obj, iters=10)
    infos = [ds.view_info(i) for i in live]
    depth, mask = torch.stack([f["depth"] for f in infos]), torch.stack([f["mask"] for f in infos])
    window = (max(f["box"][1] - f["box"][0] for f in infos) + 2 * MARGIN, max(f["box"][3] - f["box"][2] for f in infos) + 2 * MARGIN)
    corner = torch.tensor([[f["box"][0] - MARGIN, f["box"][2] - MARGIN] for f in infos], dtype=torch.int32, device="cuda")
    frame = torch.arange(VIEWS, dtype=torch.int32, device="cuda")
    score = lambda pose: ver.score(depth, pose, frame, obj, corner, window, TOL, mask=mask, cull=bool(ds.cull))
    sa, sb = score(before), score(after)
    items = np.concatenate([np.arange(VIEWS)[:, None], np.zeros((VIEWS, 1), int), corner.cpu().numpy(), np.arange(VIEWS)[:, None],
                            np.full((VIEWS, 1), 65535)], axis=1)
    for got, pose in ((sa, before), (sb, after)):
        want = pv.verify_np(ver.vertices.cpu().numpy(), ver.triangles.cpu().numpy(), ver.tri_begin, ver.model_scales, ver.proj.reshape(4, 4),
                            depth.cpu().numpy(), mask.cpu().numpy(), items, pose.cpu().numpy(), 10000.0, window[0], window[1], TOL, int(bool(ds.cull)))
        assert m.same_bits(got.cpu().numpy(), want), "the device equals the restatement on the rendered frames"
    va, vb = vsiou(sa).cpu().numpy(), vsiou(sb).cpu().numpy()
    for k, i in enumerate(live):
        print(f"view {i}: window {window} vsiou {va[k]:.6f} -> {vb[k]:.6f}  before {dict(zip(pv.STATS[1:10], sa[k, 1:10].tolist()))} after {dict(zip(pv.STATS[1:10], sb[k, 1:10].tolist()))}")
    assert (vb > va).all(), "ICP raises the visible-surface IoU on every view"
    take = better(sa, sb)
    assert take.cpu().numpy().all(), "the ICP pose is taken on all eight"
    chosen = torch.where(take[:, None], after, before)
    swapped = torch.where(better(sb, sa)[:, None], before, after)
    assert torch.equal(chosen, swapped) and torch.equal(chosen, after), "the order of the candidates does not matter"


def _nets(tmp_path=None):
    from densefusion_amd.lib.network import PoseNet, PoseRefineNet
    torch.manual_seed(3)
    est, ref = PoseNet(num_points=500, num_obj=5), PoseRefineNet(num_points=500, num_obj=5)
    if tmp_path is not None:
        torch.save(est.state_dict(), tmp_path / "pose.pth")
        torch.save(ref.state_dict(), tmp_path / "refine.pth")
    return est.cuda().eval(), ref.cuda().eval()


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return importlib.import_module(name)
    finally:
        sys.path.pop(0)


def test_evaluate_hands_candidates_to_select_pose():
    _dev()
    evaluate = _tool("eval_linemod").evaluate
    est, ref = _nets()
    ds = _dataset(16, 8)
    live = [i for i in range(16) if ds.view_info(i)["live"]]
    opt = argparse.Namespace(max_frames=0, window=4, workers=0, iteration=2, feed="threads")
    diameter = [0.01] * 5

    def run(**steps):
        fw = io.StringIO()
        counts = evaluate(ds, est, ref, diameter, opt, fw, **steps)
        return fw.getvalue(), counts

    plain, icp_like = run(), run(refine_pose=lambda pose, points, objs: pose + 0.25)
    seen = []

    def stub(take):
        def select(indices, candidates, objs):
            seen.append((list(indices), [c.clone() for c in candidates], list(objs)))
            return candidates[take]
        return select

    assert run(select_pose=stub(0)) == plain and run(select_pose=stub(-1)) == plain, "one candidate: the refiner's pose, the log bytes unchanged"
    assert sorted(i for call in seen for i in call[0]) == sorted(live + live) and all(len(c[1]) == 1 and c[1][0].shape == (len(c[0]), 7) for c in seen)
    assert all(c[2] == [0] * len(c[0]) for c in seen)
    del seen[:]
    shift = lambda pose, points, objs: pose + 0.25
    assert run(refine_pose=shift, select_pose=stub(1)) == icp_like and run(refine_pose=shift, select_pose=stub(0)) == plain
    assert all(len(c[1]) == 2 and torch.equal(c[1][1], c[1][0] + 0.25) for c in seen) and icp_like != plain
    assert run(select_pose=lambda indices, candidates, objs: candidates[0] + 0.25) == icp_like, "what select_pose returns is what is scored"


def test_the_tool_verifies_and_chooses(tmp_path):
    _dev()
    import cad_scene_np as snp
    paths = [str(mnp.write_mesh_ply(tmp_path / name, *mesh)) for name, mesh in zip(("big.ply", "small.ply", "box.ply"), snp.tool_meshes())]
    pm = rnp.write_proj(tmp_path / "proj_in.txt", fab.PROJ[1])
    _nets(tmp_path)
    tool = _tool("eval_cad_render")

    def run(out, *extra):
        return tool.main(["--cad_model", paths[0], paths[1], "--cad_distractor", paths[2], "--model", str(tmp_path / "pose.pth"), "--refine_model",
                          str(tmp_path / "refine.pth"), "--masks", "truth", "--cad_seed", "0", "--cad_frames", str(VIEWS), "--proj_mat", pm,
                          "--height", "64", "--width", "96", "--min_pixels", "60", "--mask", "pixels", "--chunk", "4", "--workers", "0",
                          "--iteration", "2", "--output_result_dir", str(tmp_path / out), *extra])

    read = lambda out, name: open(tmp_path / out / ("eval_result_logs_%s.txt" % name)).read()
    icp_args = ("--icp", "3", "--icp_max_dist", "0.5")
    plain, both, ver = run("plain", *icp_args), run("icp", *icp_args), run("ver", *icp_args, "--verify", "--verify_tol", "6", "--verify_margin", "5")
    assert plain == both and sorted(os.listdir(tmp_path / "plain")) == ["eval_result_logs_truth.txt", "eval_result_logs_truth_icp.txt"]
    assert sorted(ver) == ["truth", "truth_icp", "truth_icp_best"]
    for name in ("truth", "truth_icp"):
        assert read("plain", name) == read("icp", name), "without --verify two runs give the same bytes"
        lines = read("ver", name).splitlines(keepends=True)
        assert "".join(x for x in lines if "verify" not in x) == read("plain", name), "--verify only adds its own lines"
        assert {k: v for k, v in ver[name].items() if k != "verify"} == plain[name] and "verify" not in plain[name]
        v = ver[name]["verify"]
        assert v["items"] == sum(ver[name]["served"]) >= 3 and v["passes"] == sum(ver[name]["success"]) and (v["tol"], v["margin"]) == (6, 5)
        assert 0.0 <= v["mean_vsiou_pass"] <= 1.0 and 0.0 <= v["mean_vsiou_miss"] <= 1.0 and v["took_first"] == 0
        assert sum("verify tol 6 margin 5: mean vsiou" in x for x in lines) == 1
    best = ver["truth_icp_best"]
    v = best["verify"]
    assert best["served"] == ver["truth"]["served"] and v["took_last"] + v["took_first"] == v["items"] == sum(best["served"])
    log = read("ver", "truth_icp_best")
    assert "[truth_icp_best masks] verify: %d items took the ICP pose, %d kept the refiner's" % (v["took_last"], v["took_first"]) in log
    assert log.count("Distance: ") == sum(best["served"])
    # every item's distance under `best` is the one it has under one of the two candidates
    dist = lambda text: {x.split(" ")[0]: x.split("Distance: ")[1] for x in text.splitlines() if "Distance: " in x}
    a, b, c = dist(read("ver", "truth")), dist(read("ver", "truth_icp")), dist(log)
    assert sorted(a) == sorted(b) == sorted(c) and all(c[k] in (a[k], b[k]) for k in c)
    assert sum(c[k] == b[k] for k in c) >= v["took_last"] and sum(c[k] == a[k] for k in c) >= v["took_first"]
    with pytest.raises(SystemExit):
        run("bad", "--verify", "--verify_tol", "-1")
