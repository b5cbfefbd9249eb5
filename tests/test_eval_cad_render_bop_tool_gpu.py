"""GPU: ``tools/eval_cad_render.py --bop``: the tiny run of tests/test_cad_eval_render_gpu.py with and without the flag.  Without its own
lines the log of the run with ``--bop`` is the log of the run without, the ``bop`` dict holds recalls in [0, 1] and the symmetry set sizes,
and an entry that is fed the true poses through the ``select_pose`` seam has every recall exactly 1."""
import argparse
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cad_raster_np as mnp  # noqa: E402
import cad_render_np as rnp  # noqa: E402
import cad_scene_np as snp  # noqa: E402
import fabricate_cad as fab  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS = 8


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return importlib.import_module(name)
    finally:
        sys.path.pop(0)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the meshes as PLY files, the camera as a proj_mat.txt, and pose checkpoints of plain initial weights"""
    _dev()
    from densefusion_amd.lib.network import PoseNet, PoseRefineNet
    root = tmp_path_factory.mktemp("cad_eval_render_bop")
    paths = [mnp.write_mesh_ply(root / name, *m) for name, m in zip(("big.ply", "small.ply", "box.ply"), snp.tool_meshes())]
    pm = rnp.write_proj(root / "proj_in.txt", fab.PROJ[1])
    torch.manual_seed(3)
    torch.save(PoseNet(num_points=500, num_obj=5).state_dict(), root / "pose.pth")
    torch.save(PoseRefineNet(num_points=500, num_obj=5).state_dict(), root / "refine.pth")
    return dict(root=root, paths=[str(p) for p in paths], pm=pm, pose=str(root / "pose.pth"), refine=str(root / "refine.pth"))


def _eval_args(files, out):
    return ["--cad_model", files["paths"][0], files["paths"][1], "--cad_distractor", files["paths"][2], "--model", files["pose"], "--refine_model",
            files["refine"], "--masks", "truth", "--cad_seed", "0", "--cad_frames", str(VIEWS), "--seg_blur", "0", "--proj_mat", files["pm"],
            "--height", "64", "--width", "96", "--min_pixels", "60", "--mask", "pixels", "--chunk", "4", "--workers", "0", "--iteration", "2",
            "--cad_sym", "auto", "--output_result_dir", str(out)]


def test_the_flag_adds_its_lines_and_changes_no_other(files):
    tool = _tool("eval_cad_render")
    plain = tool.main(_eval_args(files, files["root"] / "plain"))
    with_bop = tool.main(_eval_args(files, files["root"] / "bop") + ["--bop"])
    assert sorted(plain) == sorted(with_bop) == ["truth"] and "bop" not in plain["truth"]
    bop = with_bop["truth"].pop("bop")
    assert with_bop == plain
    base = open(files["root"] / "plain" / "eval_result_logs_truth.txt").read().splitlines()
    more = open(files["root"] / "bop" / "eval_result_logs_truth.txt").read().splitlines()
    own = [line for line in more if line.startswith("[truth masks] bop: ")]
    assert [line for line in more if not line.startswith("[truth masks] bop: ")] == base and len(own) == 2 + 4 * 3 and not any("bop" in line for line in base)
    served = sum(plain["truth"]["served"])
    assert served >= 3 and bop["items"] == served == bop["all"]["items"] == sum(o["items"] for o in bop["objects"]) and bop["bad_items"] == 0
    assert len(bop["set_sizes"]) == len(bop["diameter"]) == len(bop["objects"]) == 2 and all(n >= 1 for n in bop["set_sizes"])
    assert bop["pixel"] == 96 / 640.0 and all(d > 0 for d in bop["diameter"])
    for r in bop["objects"] + [bop["all"]]:
        for key in ("mssd_recall", "mspd_recall", "vsd_recall"):
            assert len(r[key]) == 10 and all(0.0 <= x <= 1.0 for x in r[key]) and r[key] == sorted(r[key])       # a recall grows with its threshold
        assert 0.0 <= r["ar"] <= 1.0 and r["ar"] == (r["ar_vsd"] + r["ar_mssd"] + r["ar_mspd"]) / 3.0
    assert "symmetry set sizes %s" % bop["set_sizes"] in own[0]
    assert bop["revolution"] == [] and "models taken as surfaces of revolution" in own[1] and own[1].endswith(": []")


def test_true_poses_through_the_seam_score_one_everywhere(files):
    """the diameter is the exact largest vertex-to-vertex distance of the scaled mesh, and est = gt gives MSSD = MSPD = 0 below every
    threshold: recall exactly 1, whatever the symmetry set"""
    tool = _tool("eval_cad_render")
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    np.random.seed(0)
    ds = RenderedPoseDataset(files["paths"][:2], 500, False, 0.0, False, distractors=files["paths"][2:], proj_mat=files["pm"], mask="pixels",
                             min_visible=0.3, chunk=4, first_seed=0, frames=VIEWS, image_dims=(64, 96), min_pixels=60, symmetry="auto", keep_frames=True)
    scorer = tool.BopScorer(ds, argparse.Namespace(bop_step=0.01, bop_delta=0.075, verify_margin=8))
    step = tool.BopStep(ds, scorer)
    for k in range(2):
        v = ds.meshes.scaled(ds.model_scale / 10000.0)[ds.meshes.vertex_begin[k]:ds.meshes.vertex_begin[k + 1]].astype(np.float64)
        want = max(float(np.sqrt(((v[a] - v) ** 2).sum(axis=1).max())) for a in range(len(v)))
        assert abs(step.diameter[k] - want) <= 1e-12 * want
    live = [i for i in range(VIEWS) if ds.view_info(i)["live"]]
    assert len(live) >= 3
    gt = torch.from_numpy(np.stack([tool.true_pose(ds, i) for i in live])).cuda()
    objs = [ds.view_info(i)["object"] - 1 for i in live]
    # the true pose is the one the target was built from: the model points under it are the item's target
    for n, i in enumerate(live):
        item = ds[i]
        R = np.asarray(ds.view_info(i)["pose"], dtype=np.float64)[:, :3]
        got = item[4].double().cpu().numpy().reshape(-1, 3) @ R.T + gt[n, 4:].cpu().numpy()
        assert np.abs(got - item[3].double().cpu().numpy().reshape(-1, 3)).max() < 1e-5
    assert step(live, [gt + 1.0, gt], objs) is not None              # the last candidate goes on
    m = step.summary()
    assert m["items"] == len(live) and m["bad_items"] == 0
    assert m["all"]["items"] == len(live) and sum(r["items"] > 0 for r in m["objects"]) >= 1
    for r in m["objects"] + [m["all"]]:
        if r["items"]:
            assert r["mssd_recall"] == [1.0] * 10 and r["mspd_recall"] == [1.0] * 10 and r["vsd_recall"] == [1.0] * 10 and r["ar"] == 1.0
    # a pose a whole diameter off scores nothing on the tightest threshold
    off = gt.clone()
    off[:, 4] += max(m["diameter"])
    miss = tool.BopStep(ds, scorer)                                  # the same scorer: nothing is uploaded or measured again
    miss(live, [off], objs)
    assert miss.summary()["all"]["mssd_recall"][0] == 0.0


def test_the_true_pose_carries_the_translation_noise(files):
    """with ``add_noise`` the target is built from T + add_t: so is the true pose"""
    tool = _tool("eval_cad_render")
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    np.random.seed(0)
    ds = RenderedPoseDataset(files["paths"][:2], 500, True, 0.03, False, distractors=files["paths"][2:], proj_mat=files["pm"], mask="pixels",
                             min_visible=0.3, chunk=4, first_seed=0, frames=VIEWS, image_dims=(64, 96), min_pixels=60)
    live = [i for i in range(VIEWS) if ds.view_info(i)["live"]]
    assert len(live) >= 3 and any(np.abs(ds.view_info(i)["add_t"]).max() > 1e-3 for i in live)
    for i in live:
        item, info = ds[i], ds.view_info(i)
        pose = tool.true_pose(ds, i)
        assert np.allclose(pose[4:], np.asarray(info["pose"])[:, 3] / 10000.0 + info["add_t"], atol=0, rtol=1e-15)
        got = item[4].double().cpu().numpy().reshape(-1, 3) @ np.asarray(info["pose"], dtype=np.float64)[:, :3].T + pose[4:]
        assert np.abs(got - item[3].double().cpu().numpy().reshape(-1, 3)).max() < 1e-5
