"""Dev-only: the golden of one SegNet training step, tests/golden/segnet_train_step.npz (read by tests/test_segnet_train_gpu.py).

Runs on the build machine, where the reference tree exists (DF_REFERENCE, default the sibling checkout); the GPU machine only sees the
.npz.  The reference's vanilla_segmentation/segnet.py and loss.py are imported as they stand (nothing is copied): seeded synthetic
weights (synth.make_segnet_state_dict), a seeded 1 x 3 x 480 x 640 frame (flat colour blobs, ImageNet-normalised on the 0..255
scale as data_controller.py does) and its 22-class blob label map; train() forward, the reference Loss, backward, one
optim.Adam(lr=1e-4) step -- once in fp32 and once in fp64 (module and input .double()).  Stored: the fp64 values, and per tensor the
fp32 run's relative L2 error against them (the envelope the GPU has to meet; for the parameters after the step, the error of the
update after - before).  Gradients are stored in full for conv11, conv11d and every BatchNorm weight and bias, at SAMPLES evenly
spaced entries (sample_positions, recomputed by the test) for the other convolution weights; the parameters after the step at those
entries, or at SAMPLES of them where there are more; the L2 norm of every gradient; the BatchNorm running statistics after the step.
The biases of the 25 convolutions followed by BatchNorm are left out: their gradient is analytically zero.

    python tools/dev/make_segnet_train_golden.py
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from densefusion_amd import synth  # noqa: E402

REF = os.environ.get("DF_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
OUT = os.path.join(ROOT, "tests", "golden", "segnet_train_step.npz")
SEED, H, W, SAMPLES = 41, 480, 640, 512
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def _import(name):
    spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, "vanilla_segmentation", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_frame(seed, h=H, w=W):
    """-> (uint8 [3,h,w], int64 [h,w]): 22-class rectangles and ellipses over class 0, each class its own flat colour (flat
    regions keep the stored frame small; their equal pixels give tied pool windows, which both sides resolve by the first maximum)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    label = np.zeros((h, w), dtype=np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(40):
        c = int(rng.integers(1, 22))
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        ry, rx = rng.uniform(h / 24, h / 5), rng.uniform(w / 24, w / 5)
        m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1 if rng.random() < 0.5 else (abs(yy - cy) < ry) & (abs(xx - cx) < rx)
        label[m] = c
    colours = rng.integers(0, 256, (22, 3))
    return colours[label].astype(np.uint8).transpose(2, 0, 1).copy(), label


def sample_positions(size, n=SAMPLES):
    """The entries stored of a large tensor: n evenly spaced flat indices (recomputed by the test, not stored)."""
    return np.linspace(0, size - 1, n).round().astype(np.int64)


def normalise(u8):
    """data_controller.py's Normalize on the 0..255 values (the reference does not divide by 255)."""
    return ((u8.astype(np.float32) - MEAN[:, None, None]) / STD[:, None, None]).astype(np.float32)


def one_step(segnet, loss, sd, x, target, dtype):
    torch.manual_seed(0)
    net = segnet.SegNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    net = net.to(dtype).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    sem = net(torch.from_numpy(x)[None].to(dtype))
    ls = loss.Loss()(sem, torch.from_numpy(target)[None])
    opt.zero_grad()
    ls.backward()
    grads = {k: p.grad.detach().double().numpy().copy() for k, p in net.named_parameters()}
    opt.step()
    state = {k: v.detach().double().numpy().copy() for k, v in net.state_dict().items()}
    return float(ls.item()), grads, state


def rel(a, b):
    n = float(np.linalg.norm(b))
    return float(np.linalg.norm(a - b)) / n if n > 0 else float(np.linalg.norm(a - b))


def main():
    torch.set_num_threads(os.cpu_count() or 1)
    segnet, loss = _import("segnet"), _import("loss")
    sd = synth.make_segnet_state_dict(SEED)
    u8, target = make_frame(SEED + 1)
    x = normalise(u8)
    l32, g32, s32 = one_step(segnet, loss, sd, x, target, torch.float32)
    l64, g64, s64 = one_step(segnet, loss, sd, x, target, torch.float64)
    out = {"x_u8": u8, "target": target.astype(np.uint8), "meta": np.array([SEED, H, W, SAMPLES]), "loss": np.array([l64, l32])}
    names = []
    for k, shape in synth.segnet_spec():
        if k.endswith("num_batches_tracked"):
            continue
        if k.startswith("bn") and k.split(".")[1] in ("running_mean", "running_var"):
            out["after/" + k] = s64[k].astype(np.float32)
            out["env/after/" + k] = np.array(rel(s32[k], s64[k]))
            continue
        if k.startswith("conv") and k.endswith(".bias") and not k.startswith("conv11d."):
            continue             # a conv followed by BatchNorm: analytically zero gradient, its value is rounding noise
        names.append(k)
        full = k.startswith("bn") or k.startswith("conv11.") or k.startswith("conv11d.")
        g, g_32 = g64[k].reshape(-1), g32[k].reshape(-1)
        a, a_32 = s64[k].reshape(-1), s32[k].reshape(-1)
        pos = np.arange(g.size) if full or g.size <= SAMPLES else sample_positions(g.size)
        out["grad/" + k] = g[pos].astype(np.float32)
        out["gnorm/" + k] = np.array(np.linalg.norm(g))
        out["env/grad/" + k] = np.array(rel(g_32[pos], g[pos]))
        if pos.size > SAMPLES:   # the parameters after the step: sampled for every tensor
            pos = sample_positions(g.size)
        out["after/" + k] = a[pos].astype(np.float32)
        w0 = np.asarray(sd[k], dtype=np.float64).reshape(-1)[pos]
        out["env/step/" + k] = np.array(rel(a_32[pos] - w0, a[pos] - w0))          # envelope of the Adam update itself
    np.savez_compressed(OUT, **out)
    print(f"loss fp64 {l64:.9f} fp32 {l32:.9f}; {os.path.getsize(OUT) / 1e6:.2f} MB -> {OUT}")
    worst = sorted(((float(out['env/grad/' + k]), k) for k in names), reverse=True)[:6]
    print("largest fp32-vs-fp64 gradient errors:", ", ".join(f"{k} {e:.2e}" for e, k in worst))


if __name__ == "__main__":
    main()
