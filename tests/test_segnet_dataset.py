"""CPU: vanilla_segmentation/data_controller.py's SegDataset over a fabricated YCB tree (tests/fabricate.py) plus a data_syn/ frame
written here.

The reference loader (vanilla_segmentation/data_controller.py) imports torchvision, which is not part of this build, so its parity is
unpinned: these tests check the behaviour the reference's code prescribes -- shapes and dtypes, normalisation on the 0..255 scale,
flips that move image and label together, and the synthetic composite taking the background frame's pixels and labels where the
synthetic label is 0."""
import random

import numpy as np
import pytest
from PIL import Image

from densefusion_amd.vanilla_segmentation.data_controller import MEAN, STD, SegDataset
from fabricate import make_ycb_tree


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("ycb")
    cfg = root / "cfg"
    make_ycb_tree(str(root / "data_root"), str(cfg), np.random.Generator(np.random.PCG64(3)))
    return str(root / "data_root"), str(cfg)


def _write_list(path, names):
    with open(path, "w") as f:
        f.write("\n".join(names) + "\n")
    return str(path)


def _unnormalise(rgb):
    return rgb.numpy() * STD[:, None, None] + MEAN[:, None, None]


def test_shapes_dtypes_and_scale(tree):
    root, cfg = tree
    ds = SegDataset(root, f"{cfg}/test_data_list.txt", False, 7)
    assert len(ds) == 7
    random.seed(0)
    rgb, target = ds[0]
    assert rgb.shape == (3, 480, 640) and str(rgb.dtype) == "torch.float32"
    assert target.shape == (480, 640) and str(target.dtype) == "torch.int64"
    # the list has fewer than 10 frames: the draw is the first frame; normalised on the 0..255 scale, not 0..1
    name = open(f"{cfg}/test_data_list.txt").read().split()[0]
    img = np.array(Image.open(f"{root}/{name}-color.png").convert("RGB")).astype(np.float32).transpose(2, 0, 1)
    np.testing.assert_allclose(_unnormalise(rgb), img, atol=1e-3)
    assert float(rgb.max()) > 100.0
    np.testing.assert_array_equal(target.numpy(), np.array(Image.open(f"{root}/{name}-label.png")))


def test_flips_move_image_and_label_together(tree, tmp_path):
    root, cfg = tree
    name = open(f"{cfg}/test_data_list.txt").read().split()[0]
    lst = _write_list(tmp_path / "one.txt", [name])
    img = np.array(Image.open(f"{root}/{name}-color.png").convert("RGB")).astype(np.float32).transpose(2, 0, 1)
    lab = np.array(Image.open(f"{root}/{name}-label.png")).astype(np.int64)
    ds = SegDataset(root, lst, True, 1)
    seen = set()
    for s in range(40):
        random.seed(s)
        rgb, target = ds[0]
        t = target.numpy()
        for k, (fi, fl) in enumerate(((lambda a: a[..., ::-1], lambda a: a[:, ::-1]), (lambda a: a[..., ::-1, :], lambda a: a[::-1]),
                                      (lambda a: a[..., ::-1, ::-1], lambda a: a[::-1, ::-1]), (lambda a: a, lambda a: a))):
            if np.array_equal(t, fl(lab)):
                seen.add(k)
                # colour jitter changes values, not geometry: the jittered image correlates with the flipped original
                back = _unnormalise(rgb)
                c = np.corrcoef(back.reshape(-1), np.ascontiguousarray(fi(img)).reshape(-1))[0, 1]
                assert c > 0.8
                break
        else:
            raise AssertionError("label is not a flip of the source label")
    assert seen == {0, 1, 2, 3}


def test_synthetic_composite(tree, tmp_path):
    root, cfg = tree
    syn = "data_syn/000000"
    real = open(f"{cfg}/test_data_list.txt").read().split()[0]
    lst = _write_list(tmp_path / "syn.txt", [syn, real])
    ds = SegDataset(root, lst, False, 1)
    syn_lab = np.array(Image.open(f"{root}/{syn}-label.png")).astype(np.int64)
    back_lab = np.array(Image.open(f"{root}/{real}-label.png")).astype(np.int64)
    back_img = np.array(Image.open(f"{root}/{real}-color.png").convert("RGB")).astype(np.float32).transpose(2, 0, 1)
    for s in range(20):
        random.seed(s)
        np.random.seed(s)
        rgb, target = ds[0]
        if np.array_equal(target.numpy()[syn_lab > 0], syn_lab[syn_lab > 0]):
            break
    t = target.numpy()
    assert np.array_equal(t[syn_lab == 0], back_lab[syn_lab == 0])      # labels: the background frame's where the render is empty
    assert np.array_equal(t[syn_lab > 0], syn_lab[syn_lab > 0])
    # pixels: the (jittered) background plus the blurred render's dark surround and N(0, 5) noise where the label is 0
    back = _unnormalise(rgb)
    m = syn_lab == 0
    c = np.corrcoef(back[:, m].reshape(-1), back_img[:, m].reshape(-1))[0, 1]
    assert c > 0.8
    assert np.abs(back[:, m] - back_img[:, m]).mean() < 60.0
