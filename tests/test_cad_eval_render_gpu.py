"""GPU: the closed loop on rendered customCAD scenes -- ``RenderedPoseDataset`` with SegNet's masks in place of the renderer's
(``segnet=``), tools/eval_cad_render.py and ``tools/train_segnet.py --seg_score``.  The seam ``_seg_logits`` is overridden to put known
logits in: the one-hot of the rendered truth must reproduce the truth-mask dataset bit for bit."""
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

import cad_raster_np as mnp
import cad_render_np as rnp
import cad_scene_np as snp
import fabricate_cad as fab

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS = 8
# tool_meshes() are sized for 96 x 144 frames under fab.PROJ[1] with min_pixels 200; the smaller frames here scale the rule with their area
FULL, SMALL = dict(image_dims=(64, 96), min_pixels=60), dict(image_dims=(40, 72), min_pixels=30)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return importlib.import_module(name)
    finally:
        sys.path.pop(0)


def _segnet():
    from densefusion_amd.vanilla_segmentation.segnet import SegNet
    torch.manual_seed(5)
    return SegNet(label_nbr=3).cuda().eval()


def _one_hot(self, x, target):
    return torch.nn.functional.one_hot(target, 4).float()


def _background(self, x, target):
    logits = torch.zeros(tuple(target.shape) + (4,), device=target.device)
    logits[..., 0] = 1.0
    return logits


def _dataset(cls=None, **kw):
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    m = snp.tool_meshes()
    np.random.seed(1)                                                          # ``pt`` is drawn with np.random
    args = dict(distractors=m[2:], proj_mat=fab.PROJ[1], mask="pixels", min_visible=0.3, chunk=4, first_seed=0, frames=VIEWS)
    args.update(kw)
    return (cls or RenderedPoseDataset)(m[:2], 500, False, 0.0, False, **args)


def _subclass(seg_logits):
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    return type("Seamed", (RenderedPoseDataset,), dict(_seg_logits=seg_logits))


def test_one_hot_of_the_truth_reproduces_the_truth_mask_dataset():
    _dev()
    truth = _dataset(**FULL)
    seg = _dataset(_subclass(_one_hot), segnet=_segnet(), seg_blur=0, **FULL)
    assert seg.seg_window == (64, 96) and seg.seg_corner == (0, 0) and truth.mask_source == "truth" and seg.mask_source == "segnet"
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    live = 0
    for i in range(VIEWS):
        a, b = truth.view_info(i), seg.view_info(i)
        assert a["table"] == b["table"] and a["live"] == b["live"] and a["kept"] == b["kept"] and a["seed"] == b["seed"], i
        assert a["mask_source"] == "truth" and a["conf"] is None and b["mask_source"] == "segnet"
        assert b["conf"].is_cuda and tuple(b["conf"].shape) == (3, 3) and torch.equal(torch.diagonal(b["conf"]), b["seg_counts"]), i
        counts += b["seg_counts"]
        x, y = truth[i], seg[i]
        assert len(x) == len(y) == 6 and all(p.shape == q.shape and torch.equal(p, q) for p, q in zip(x, y)), i
        live += a["live"]
    print("live views:", live, "of", VIEWS)
    assert live >= 3, "the comparison has something to compare"
    m = seg.seg_score.summary()
    assert np.array_equal(m["conf"], np.diag(counts.cpu().numpy())) and m["skipped"] == 0 and m["pixels"] == VIEWS * 64 * 96
    assert m["miou"] == 1.0 and m["pixel_accuracy"] == 1.0
    seg.view_info(0)                                                           # a chunk the cache prepares again is not scored twice
    seg._cache.clear()
    seg.view_info(0)
    assert seg.seg_score.summary()["pixels"] == VIEWS * 64 * 96
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    from densefusion_amd.vanilla_segmentation.segnet import SegNet
    for bad in (dict(segnet=SegNet(label_nbr=3).cuda()), dict(segnet=SegNet(label_nbr=4).cuda().eval()),
                dict(segnet=_segnet(), seg_window=(32, 50)), dict(segnet=_segnet(), seg_blur=2)):
        with pytest.raises(ValueError):
            _dataset(**dict(FULL, **bad))
    with pytest.raises(ValueError):                                            # one model, no scene: no label plane to score against
        RenderedPoseDataset(snp.tool_meshes()[0], 500, False, 0.0, False, raster="mesh", proj_mat=fab.PROJ[1], segnet=_segnet(), **FULL)


def test_an_empty_prediction_serves_nothing():
    _dev()
    truth = _dataset(**FULL)
    seg = _dataset(_subclass(_background), segnet=_segnet(), seg_blur=0, **FULL)
    kept = [i for i in range(VIEWS) if seg.view_info(i)["kept"]]
    assert kept == [i for i in range(VIEWS) if truth.view_info(i)["kept"]] and len(kept) >= 3
    assert not any(seg.view_info(i)["live"] for i in range(VIEWS))
    assert all(seg[i][0].dim() == 1 for i in range(VIEWS))
    m = seg.seg_score.summary()
    assert m["conf"][:, 1:].sum() == 0 and m["recall"][0] == 1.0 and m["iou"][1] == 0.0 and m["iou"][2] == 0.0


def test_untrained_segnet_on_a_window_inside_the_frame(monkeypatch):
    _dev()
    from densefusion_amd.datasets.customCAD import online
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    seen = dict(logits=[], label=[], win=[], pairs=[])

    class Recording(RenderedPoseDataset):
        def _seg_logits(self, x, target):
            assert tuple(x.shape[1:]) == (32, 64, 4) and tuple(target.shape[1:]) == (32, 64)
            logits = super()._seg_logits(x, target)
            seen["logits"].append(logits)
            return logits

    real = online.ss.seg_masks

    def recording_masks(label, win, pairs, image_dims):
        seen["label"].append(label)
        seen["win"] += [list(w) for w in win]
        seen["pairs"] += [list(p) for p in pairs]
        assert tuple(image_dims) == (40, 72)
        return real(label, win, pairs, image_dims)

    monkeypatch.setattr(online.ss, "seg_masks", recording_masks)
    ds = _dataset(Recording, segnet=_segnet(), seg_window=(32, 64), **SMALL)
    infos = [ds.view_info(i) for i in range(VIEWS)]
    m = ds.seg_score.summary()
    assert m["pixels"] + m["skipped"] == VIEWS * 2048 and m["skipped"] == 0
    assert len(seen["logits"]) == 2 and seen["win"] == [[4, 4]] * VIEWS
    assert seen["pairs"] == [[j % 4, infos[j]["object"]] for j in range(VIEWS)]
    for logits, label in zip(seen["logits"], seen["label"]):
        assert label.dtype == torch.int32 and torch.equal(label.long(), torch.argmax(logits[..., :3], dim=-1))
    total = sum(int(info["conf"].sum()) for info in infos)
    assert total == VIEWS * 2048


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the meshes as PLY files, the camera as a proj_mat.txt, and pose checkpoints of plain initial weights"""
    _dev()
    from densefusion_amd.lib.network import PoseNet, PoseRefineNet
    root = tmp_path_factory.mktemp("cad_eval_render")
    paths = [mnp.write_mesh_ply(root / name, *m) for name, m in zip(("big.ply", "small.ply", "box.ply"), snp.tool_meshes())]
    pm = rnp.write_proj(root / "proj_in.txt", fab.PROJ[1])
    torch.manual_seed(3)
    torch.save(PoseNet(num_points=500, num_obj=5).state_dict(), root / "pose.pth")
    torch.save(PoseRefineNet(num_points=500, num_obj=5).state_dict(), root / "refine.pth")
    return dict(root=root, paths=[str(p) for p in paths], pm=pm, pose=str(root / "pose.pth"), refine=str(root / "refine.pth"))


def _eval_args(files, out, masks):
    return ["--cad_model", files["paths"][0], files["paths"][1], "--cad_distractor", files["paths"][2], "--model", files["pose"], "--refine_model",
            files["refine"], "--masks", masks, "--cad_seed", "0", "--cad_frames", str(VIEWS), "--seg_blur", "0", "--proj_mat", files["pm"],
            "--height", "64", "--width", "96", "--min_pixels", "60", "--mask", "pixels", "--chunk", "4", "--workers", "0", "--iteration", "2",
            "--output_result_dir", str(out)]


def test_the_tool_on_both_mask_sources(files, monkeypatch):
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    tool, eval_cad = _tool("eval_cad_render"), _tool("eval_cad")
    monkeypatch.setattr(RenderedPoseDataset, "_seg_logits", _one_hot)
    out = files["root"] / "both"
    got = tool.main(_eval_args(files, out, "both"))
    assert sorted(got) == ["segnet", "truth"]
    t, s = got["truth"], got["segnet"]
    # the truth run is tools/eval_cad.py over the same views
    np.random.seed(0)
    ds = RenderedPoseDataset(files["paths"][:2], 500, False, 0.0, False, distractors=files["paths"][2:], proj_mat=files["pm"], mask="pixels",
                             min_visible=0.3, chunk=4, first_seed=0, frames=VIEWS, **FULL)
    success, served = eval_cad.main(["--model", files["pose"], "--refine_model", files["refine"], "--iteration", "2", "--workers", "0",
                                     "--output_result_dir", str(files["root"] / "plain")], testdataset=ds)
    assert t["success"] == success[:2] and t["served"] == served[:2] and sum(served[2:]) == 0
    assert t["kept"] == [sum(ds.view_info(i)["kept"] and ds.view_info(i)["object"] == o for i in range(VIEWS)) for o in (1, 2)]
    assert sum(t["served"]) >= 3 and all(a <= b for a, b in zip(t["served"], t["kept"]))
    # with the truth's one-hot behind the seam, SegNet's masks are the truth's: the same counts
    for k in ("views", "success", "served", "kept", "success_served", "success_kept", "all_served", "all_kept"):
        assert s[k] == t[k], k
    assert s["seg"]["miou"] == 1.0 and s["seg"]["pixels"] == VIEWS * 64 * 96 and "seg" not in t
    log = open(out / "eval_result_logs_segnet.txt").read()
    assert re.search(r"No\.\d+ (NOT )?Pass! Distance: ", log) and "[segnet masks] mIoU 1.0000 pixel accuracy 1.0000" in log
    assert "[segnet masks] ALL success rate:" in log and "object 2: IoU 1.0000 precision 1.0000 recall 1.0000" in log
    assert "[truth masks] ALL success rate:" in open(out / "eval_result_logs_truth.txt").read()


def test_the_tool_on_an_empty_prediction(files, monkeypatch):
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    tool = _tool("eval_cad_render")
    monkeypatch.setattr(RenderedPoseDataset, "_seg_logits", _background)
    got = tool.main(_eval_args(files, files["root"] / "empty", "segnet"))
    s = got["segnet"]
    assert sorted(got) == ["segnet"] and sum(s["served"]) == 0 and sum(s["kept"]) >= 3 and sum(s["success"]) == 0
    assert s["all_kept"] == 0.0 and s["all_served"] == 0.0 and s["seg"]["iou"][1] == 0.0
    assert open(files["root"] / "empty" / "eval_result_logs_segnet.txt").read().count("Lost detection") == VIEWS


def test_the_trainer_logs_miou_only_when_asked(files, tmp_path):
    tool = _tool("train_segnet")

    def run(name, n_epochs, *extra):
        out, logs = str(tmp_path / name / "models"), str(tmp_path / name / "logs")
        history = tool.main(["--dataset", "cad_render", "--cad_model", files["paths"][0], files["paths"][1], "--cad_distractor", files["paths"][2],
                             "--proj_mat", files["pm"], "--height", "40", "--width", "72", "--seg_height", "32", "--seg_width", "64",
                             "--cad_frames", "8", "--cad_test_frames", "8", "--n_epochs", str(n_epochs), "--batch_size", "4", "--chunk", "4",
                             "--workers", "2", "--lr", "0.001", "--seed", "7", "--model_save_path", out, "--log_dir", logs, *extra])
        return history, logs

    history, logs = run("scored", 3, "--seg_score")                           # the loop runs epochs 1 .. n_epochs - 1
    assert len(history["miou"]) == 2 and all(0.0 <= v <= 1.0 for v in history["miou"]), history["miou"]
    for epoch in (1, 2):
        found = re.findall(r"Test Finish mIoU: (\S+) IoU: (.+)", open(os.path.join(logs, "epoch_%d_test_log.txt" % epoch)).read())
        assert len(found) == 1 and abs(float(found[0][0]) - history["miou"][epoch - 1]) <= 5e-5 and len(found[0][1].split()) == 3
    plain, logs = run("plain", 2)
    assert "miou" not in plain and "mIoU" not in open(os.path.join(logs, "epoch_1_test_log.txt")).read()
