"""GPU: tools/train_segnet.py end to end in a child process on a fabricated YCB tree (one epoch of 4 frames at batch 2): exit code 0,
the reference's CEloss log lines, and a checkpoint that loads strictly into SegNet."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fabricate import make_ycb_tree

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_segnet_one_epoch(tmp_path):
    root, cfg = str(tmp_path / "ycb"), str(tmp_path / "cfg")
    make_ycb_tree(root, cfg, np.random.Generator(np.random.PCG64(4)))
    models, logs = tmp_path / "models", tmp_path / "logs"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_segnet.py"), "--dataset_root", root, "--dataset_config_dir", cfg,
           "--batch_size", "2", "--n_epochs", "2", "--workers", "0", "--train_length", "4", "--test_length", "2", "--seed", "1",
           "--model_save_path", str(models), "--log_dir", str(logs)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    train_log = open(logs / "epoch_1_log.txt").read()
    batches = [ln for ln in train_log.splitlines() if "Batch" in ln and "CEloss" in ln]
    assert len(batches) == 2
    assert all(np.isfinite(float(ln.split("CEloss ")[1])) for ln in batches)
    assert "Train Finish Avg CEloss" in train_log
    assert "Test Finish Avg CEloss" in open(logs / "epoch_1_test_log.txt").read()
    ckpts = glob.glob(str(models / "model_1_*.pth"))
    assert len(ckpts) == 1
    from densefusion_amd.vanilla_segmentation.segnet import SegNet
    sd = torch.load(ckpts[0], weights_only=True)
    SegNet().load_state_dict(sd, strict=True)
    assert int(sd["bn11.num_batches_tracked"]) == 2                              # two training batches went through BatchNorm
