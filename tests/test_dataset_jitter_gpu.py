"""GPU: ``jitter="device"`` of the two disk datasets against ``jitter="host"`` on the fabricated trees of tests/fabricate.py.  Same
``random`` / ``np.random`` / torch state in, the same tensors and the same ``random`` state out: the host half draws every jitter the
host path draws (rejected occluder candidates included), the device applies them to the same bytes."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fabricate import make_linemod_tree, make_ycb_tree  # noqa: E402


def _seed(s):
    import torch
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


def _same(a, b):
    import torch
    assert len(a) == len(b) == 6
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y.cpu())


@pytest.fixture(scope="module")
def linemod_tree(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return make_linemod_tree(str(tmp_path_factory.mktemp("linemod_jitter")), frames_per_obj=12)


def _both(make):
    return make("host"), make("device")


def test_linemod_device_jitter_equals_host_jitter(linemod_tree):
    import torch
    from densefusion_amd.datasets.linemod.dataset import PoseDataset
    host, dev = _both(lambda j: PoseDataset("train", 500, True, linemod_tree, 0.03, False, seed=3, jitter=j))
    clean = PoseDataset("train", 500, False, linemod_tree, 0.0, False, seed=3, jitter="device")
    idxs = [0, 1, 2, 14, 40, 155]                       # several crop sizes; frame 1 of an object touches two frame edges, frame 2 wrap-pads
    for i in idxs:
        _seed(300 + i); a = host[i]; sa = random.getstate()
        _seed(300 + i); b = dev[i]; sb = random.getstate()
        _same(a, b)
        assert sa == sb
        _seed(300 + i); c = clean[i]
        assert torch.equal(a[1], c[1]) and not torch.equal(a[2], c[2])          # the jitter did change the crop
        # the fetch cut in two, the pixel subset handed in so that sampling cannot differ
        _seed(400 + i); hh = host.host_item(i); c = host.device_item(i, hh, choose=a[1]); sa = random.getstate()
        _seed(400 + i); hd = dev.host_item(i); d = dev.device_item(i, hd, choose=a[1]); sb = random.getstate()
        _same(c, d)
        assert sa == sb and torch.equal(c[1], a[1])
        assert len(hh) == 7 and len(hd) == 8 and hd[7].shape == (1, 8) and hd[7].dtype == torch.float32
        raw = torch.from_numpy(np.array(Image.open(dev.list_rgb[i]))[:, :, :3])
        assert torch.equal(hd[0], raw) and not torch.equal(hh[0], raw)         # host half of "device": the decoded frame, untouched
        for x, y in zip(hh[1:], hd[1:7]):
            assert torch.equal(x, y)
    _seed(77); a = host.batch(idxs); sa = random.getstate()
    _seed(77); b = dev.batch(idxs); sb = random.getstate()
    assert sa == sb and len(a) == len(b) == len(idxs)
    for x, y in zip(a, b):
        _same(x, y)
    # without add_noise the keyword changes nothing: no plan, no launch
    assert len(clean.host_item(0)) == 7
    with pytest.raises(ValueError):
        PoseDataset("train", 500, True, linemod_tree, 0.03, False, jitter="gpu")


def _ycb_tree(root, cfg):
    """fabricate.make_ycb_tree, then real frame data/0001/000001 relabelled: one 1200-pixel patch of object 1 inside the rectangle of
    data_syn/000000's object 1 -- an occluder candidate that draws that object leaves fewer than 1000 labelled pixels and is rejected
    (datasets/ycb/dataset.py:130), one that draws the other two objects of either synthetic frame may be accepted."""
    make_ycb_tree(root, cfg, np.random.default_rng(4))
    syn = np.array(Image.open(f"{root}/data_syn/000000-label.png"))
    rows, cols = np.nonzero(syn == 1)
    r0, c0 = int(rows.min()), int(cols.min())
    lab = np.zeros((480, 640), dtype=np.uint8)
    lab[r0 + 10:r0 + 40, c0 + 10:c0 + 50] = 1
    Image.fromarray(lab).save(f"{root}/data/0001/000001-label.png")


# (index, seed): picked on the CPU from the host path; what each must show is asserted below from the host half's own outputs
YCB_CASES = [(4, 0), (5, 1), (1, 2), (3, 3), (0, 7), (0, 1)]         # (0, 7): three candidates rejected, the fourth accepted


def test_ycb_device_jitter_equals_host_jitter(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from densefusion_amd.datasets.ycb.dataset import PoseDataset
    root, cfg = str(tmp_path / "YCB"), str(tmp_path / "cfg")
    _ycb_tree(root, cfg)
    host, dev = _both(lambda j: PoseDataset("train", 1000, True, root, 0.03, False, dataset_config_dir=cfg, seed=5, jitter=j))
    assert len(dev.syn) == 2 and len(dev.real) == 4
    draws, draw = [0], dev.trancolor.draw

    def counted():
        draws[0] += 1
        return draw()
    dev.trancolor.draw = counted
    seen = set()
    for i, s in YCB_CASES:
        syn = dev.list[i][:8] == "data_syn"
        _seed(500 + s); a = host[i]; sa = random.getstate(); na = np.random.get_state()[1].copy()
        _seed(500 + s); b = dev[i]; sb = random.getstate(); nb = np.random.get_state()[1].copy()
        _same(a, b)                                     # the N(0, 7) pixel noise of a synthetic frame included: torch seeded alike
        assert sa == sb and np.array_equal(na, nb)
        _seed(600 + s); hh = host.host_item(i); c = host.device_item(i, hh, choose=a[1]); sa = random.getstate()
        _seed(600 + s); draws[0] = 0; hd = dev.host_item(i); n = draws[0]; d = dev.device_item(i, hd, choose=a[1]); sb = random.getstate()
        _same(c, d)
        assert sa == sb and len(hh) == 7 and len(hd) == 12 and hd[7].shape == (3, 8)
        for x, y in zip(hh[1:], hd[1:7]):
            assert torch.equal(x, y)
        back, front = hd[8].numel() > 0, hd[10].numel() > 0
        assert back == syn and int(hd[3][5]) == int(syn)
        raw = np.array(Image.open(f"{root}/{dev.list[i]}-color.png"))[:, :, :3]
        assert torch.equal(hd[0], torch.from_numpy(raw))                        # the decoded frame, neither jittered nor composed
        if back:
            assert hd[8].shape == (480, 640, 3) and hd[9].shape == (480, 640) and 0 < int(hd[9].count_nonzero()) < 480 * 640
        if front:
            assert hd[10].shape == (480, 640, 3) and 0 < int(hd[11].count_nonzero()) < 480 * 640
            assert not torch.equal(hh[0], torch.from_numpy(raw))
        candidates = n - 1 - int(back)                   # one draw per occluder candidate, one for the frame, one for the background
        assert 1 <= candidates <= 5 and (front or candidates == 5)
        seen.add(("syn" if syn else "real", "front" if front else "no front", "first rejected" if candidates > 1 else "first accepted"))
    assert ("syn", "front", "first accepted") in seen                           # occluder accepted and background pasted
    assert any(k[0] == "real" for k in seen)
    assert any(k[2] == "first rejected" and k[1] == "front" for k in seen), seen   # plans drawn for rejected candidates, never applied


def test_train_tool_with_device_jitter(linemod_tree, tmp_path):
    """tools/train.py --jitter device on the fabricated LineMOD tree, fed by worker processes: one epoch, a checkpoint."""
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--dataset", "linemod", "--dataset_root", linemod_tree, "--nepoch", "2", "--repeat_epoch", "1",
           "--batch_size", "4", "--workers", "3", "--feed", "processes", "--jitter", "device", "--lanes", "2", "--outf", str(out / "models"),
           "--log_dir", str(out / "logs"), "--decay_margin", "0", "--refine_margin", "0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = r.stdout + r.stderr
    assert log.count("train finish") == 1 and "colour jitter on the device" in log, log[-3000:]
    assert any(f.startswith("pose_model_") for f in os.listdir(out / "models")), os.listdir(out / "models")
