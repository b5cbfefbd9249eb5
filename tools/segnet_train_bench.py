"""SegNet training step on the GPU: ms per step and frames/s (default 480 x 640, batch 3 -- the reference's train.py), the executed
TFLOP/s of the convolution launches against the 157.3 TFLOP/s fp32-MFMA peak, and ms per step of each kernel class (conv forward /
data gradient / weight gradient, BatchNorm forward / backward, pool, un-pool, cross-entropy, Adam).  One JSON line at the end.

    python tools/segnet_train_bench.py [--batch 3 --height 480 --width 640 --steps 10 --warmup 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from densefusion_amd import segtrain_ops, synth, train_ops  # noqa: E402
from densefusion_amd.train_utils import FlatAdam, FlatParams  # noqa: E402
from densefusion_amd.vanilla_segmentation.loss import Loss  # noqa: E402
from densefusion_amd.vanilla_segmentation.segnet import SegNet  # noqa: E402

PEAK_TFLOPS = 157.3          # fp32 MFMA, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    B, H, W = opt.batch, opt.height, opt.width
    net = SegNet(trainable=True)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_segnet_state_dict(1).items()})
    net = net.to(dev).train()
    flat = FlatParams(net)
    adam = FlatAdam(flat, lr=1e-4)
    crit = Loss()
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(B, 3, H, W, generator=g) * 255 - 120).div(58).to(dev)
    target = torch.randint(0, 22, (B, H, W), generator=g).to(dev)

    def step():
        flat.zero_grad()
        loss = crit(net(x), target)
        loss.backward()
        adam.step()
        return loss

    for _ in range(opt.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(opt.steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / opt.steps

    # one more step with per-launch events (measurement only: the events add launch gaps, the step time above has none)
    train_ops.profile_begin()
    segtrain_ops.profile_begin()
    a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    flat.zero_grad()
    crit(net(x), target).backward()
    a0.record()
    adam.step()
    a1.record()
    conv = train_ops.profile_end()
    other = segtrain_ops.profile_end()
    classes = {f"conv_{k}": round(v[0], 3) for k, v in conv.items()}
    classes.update({k: round(v[0], 3) for k, v in other.items()})
    classes["adam"] = round(a0.elapsed_time(a1), 3)
    conv_ms = sum(v[0] for v in conv.values())
    conv_flops = sum(v[1] for v in conv.values())
    res = {"workload": "segnet_train_step", "batch": B, "height": H, "width": W, "ms_per_step": round(ms, 3),
           "frames_per_s": round(B * 1e3 / ms, 2), "loss": round(float(loss.detach()), 6),
           "conv_tflops_executed": round(conv_flops / 1e12, 3),
           "conv_tflops_per_s_in_conv_launches": round(conv_flops / conv_ms / 1e9, 2),
           "conv_fraction_of_peak": round(conv_flops / conv_ms / 1e9 / PEAK_TFLOPS, 3),
           "step_tflops_per_s": round(conv_flops / ms / 1e9, 2),
           "ms_per_step_by_class": classes,
           "per_kind_fraction_of_peak": {k: round(v[1] / v[0] / 1e9 / PEAK_TFLOPS, 3) for k, v in conv.items() if v[0] > 0}}
    for k, v in classes.items():
        print(f"{k:>14s} {v:9.3f} ms")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
