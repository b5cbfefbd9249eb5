"""GPU: tools/train_segnet.py --dataset cad_render -- a mask network for two small meshes and a distractor, trained on scenes rendered on
the fly: the run finishes, writes its checkpoints in the reference's key layout, logs finite losses that go down over a fixed set of
views, and is reproducible from its seed."""
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

import cad_raster_np as mnp
import cad_scene_np as snp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return importlib.import_module("train_segnet")
    finally:
        sys.path.pop(0)


def _logged(log_dir, name):
    with open(os.path.join(log_dir, name)) as f:
        return [float(m.group(1)) for m in re.finditer(r"Batch \d+ CEloss (\S+)", f.read())]


def test_train_segnet_on_rendered_scenes(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from densefusion_amd.vanilla_segmentation.segnet import SegNet
    rng = np.random.default_rng(31)
    paths = []
    for k, (v, f) in enumerate((mnp.icosphere(1, 160.0), mnp.icosphere(1, 120.0), snp.box([-90.0] * 3, [90.0] * 3))):
        v = v.astype(np.float32)
        paths.append(str(mnp.write_mesh_ply(tmp_path / ("mesh%d.ply" % k), v, np.asarray(f), rng.integers(0, 256, (len(v), 3), dtype=np.uint8))))
    tool = _tool()

    def run(name, n_epochs):
        out, logs = str(tmp_path / name / "models"), str(tmp_path / name / "logs")
        history = tool.main(["--dataset", "cad_render", "--cad_model", paths[0], paths[1], "--cad_distractor", paths[2], "--height", "40",
                             "--width", "72", "--seg_height", "32", "--seg_width", "64", "--cad_frames", "8", "--cad_test_frames", "4",
                             "--n_epochs", str(n_epochs), "--batch_size", "4", "--light", "random", "--chunk", "4", "--workers", "2",
                             "--lr", "0.001", "--seed", "7", "--model_save_path", out, "--log_dir", logs])
        return history, out, logs

    history, out, logs = run("a", 4)
    saved = sorted(os.listdir(out))
    best = [n for n in saved if re.fullmatch(r"model_\d+_\S+\.pth", n) and n != "model_current.pth"]
    assert "model_current.pth" in saved and best, saved
    for name in ("model_current.pth", best[-1]):
        sd = torch.load(os.path.join(out, name), map_location="cpu")
        SegNet(label_nbr=3).load_state_dict(sd, strict=True)
        assert tuple(sd["conv11d.weight"].shape) == (3, 64, 3, 3)
    train = [_logged(logs, "epoch_%d_log.txt" % e) for e in (1, 2, 3)]
    test = [_logged(logs, "epoch_%d_test_log.txt" % e) for e in (1, 2, 3)]
    assert [len(t) for t in train] == [2, 2, 2] and [len(t) for t in test] == [4, 4, 4]
    assert train == history["train"] and test == history["test"]
    assert all(np.isfinite(v) for t in train + test for v in t)
    first, last = float(np.mean(train[0])), float(np.mean(train[-1]))
    print("mean training loss: first epoch", first, "last epoch", last)
    assert last < first, "the 8 views are a fixed set: the loss goes down"
    with open(os.path.join(logs, "epoch_1_log.txt")) as f:
        shares = re.search(r"Class pixel shares: (\S+) (\S+) (\S+)", f.read())
    assert shares and abs(sum(float(s) for s in shares.groups()) - 1.0) < 1e-3
    again, _, logs2 = run("b", 2)                                              # the same seed: the same first epoch
    assert again["train"][0] == history["train"][0] and _logged(logs2, "epoch_1_log.txt") == train[0]
    assert again["shares"][0] == history["shares"][0]
