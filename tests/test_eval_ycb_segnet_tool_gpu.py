"""GPU: tools/eval_ycb.py --segnet_model on a fabricated YCB-Video tree without any PoseCNN file: the result files hold `poses`
and `rois` of equal length, do not depend on --window or --depth, and tools/eval_ycb_auc.py --rois_from_results reads them."""
import os
import sys

import numpy as np
import pytest
import scipy.io as scio
import torch
from PIL import Image

import fabricate
from densefusion_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_ycb_with_segnet_detections(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eval_ycb
    import eval_ycb_auc
    rng = np.random.default_rng(4)
    root, cfg, tool = tmp_path / "YCB", tmp_path / "cfg", tmp_path / "toolbox"
    names = fabricate.make_ycb_tree(str(root), str(cfg), rng)
    os.makedirs(tool)
    for i, name in enumerate(names):          # colour frames the block SegNet turns into known masks (synth.make_segnet_block_state_dict)
        blocks = [(1, 1 + i, 2, 3, 4), (3, 9, 10 + i, 4, 2)] + ([(4 % 3 + 1, 6, 16, 2, 3)] if i % 2 else [])
        rgb, _ = synth.block_frame(rng, blocks)
        Image.fromarray(rgb).save(f"{root}/{name}-color.png")
    (tool / "keyframe.txt").write_text("\n".join(n[len("data/"):] for n in names) + "\n")
    (tool / "classes.txt").write_text((cfg / "classes.txt").read_text())
    K = 21
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_segnet_block_state_dict(K + 1).items()}, tmp_path / "segnet.pth")
    torch.save({k: torch.from_numpy(v) for k, v in synth.make_state_dict(synth.posenet_spec(K), 41).items()}, tmp_path / "pose.pth")
    torch.save({k: torch.from_numpy(v) for k, v in synth.make_state_dict(synth.refiner_spec(K), 1041).items()}, tmp_path / "refine.pth")
    empty = tmp_path / "no_toolbox"
    os.makedirs(empty)
    outs = {}
    for window, depth in ((1, 1), (3, 1), (3, 2)):
        wo, ref = tmp_path / f"wo{window}{depth}", tmp_path / f"ref{window}{depth}"
        eval_ycb.main(["--dataset_root", str(root), "--model", str(tmp_path / "pose.pth"), "--refine_model", str(tmp_path / "refine.pth"),
                       "--dataset_config_dir", str(cfg), "--ycb_toolbox_dir", str(empty), "--result_wo_refine_dir", str(wo),
                       "--result_refine_dir", str(ref), "--segnet_model", str(tmp_path / "segnet.pth"), "--min_pixels", "2",
                       "--num_points", "500", "--seed", "5", "--window", str(window), "--depth", str(depth), "--workers", "2"])
        outs[(window, depth)] = [(scio.loadmat(wo / f"{i:04d}.mat"), scio.loadmat(ref / f"{i:04d}.mat")) for i in range(len(names))]
    n_live = 0
    for i in range(len(names)):
        a_wo, a_ref = outs[(1, 1)][i]
        n = a_ref["rois"].shape[0]
        assert a_ref["poses"].shape[0] == n and a_wo["poses"].shape[0] == n and n >= 2, i
        assert np.array_equal(a_ref["rois"], a_wo["rois"])
        assert np.all(np.diff(a_ref["rois"][:, 1]) > 0)                      # one detection per class, ascending
        n_live += int(a_ref["poses"].any(axis=1).sum())
        for key in ((3, 1), (3, 2)):
            b_wo, b_ref = outs[key][i]
            for k in ("poses", "rois"):
                assert np.array_equal(a_ref[k], b_ref[k]) and np.array_equal(a_wo[k], b_wo[k]), (i, key, k)
    assert n_live >= len(names)
    capsys.readouterr()
    table = eval_ycb_auc.main(["--dataset_root", str(root), "--ycb_toolbox_dir", str(tool), "--result_refine_dir", str(tmp_path / "ref11"),
                               "--result_wo_refine_dir", str(tmp_path / "wo11"), "--output_dir", str(tmp_path / "auc"), "--rois_from_results"])
    assert table["All %d objects" % len(fabricate.CLASSES)]["instances"] > 0
