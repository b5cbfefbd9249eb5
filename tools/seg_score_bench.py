#!/usr/bin/env python
"""What scoring SegNet on the device costs: the device time of ``df_seg_score`` for one chunk of ``--chunk`` windows (default 32 of
512 x 1088), at C = 3 with ld 4 and at C = 22 with ld 24, on two inputs each -- next to a plain device-to-device copy of as many
bytes as the call READS (4 ld + 8 per pixel), in the same run.  One JSON line.

    python tools/seg_score_bench.py [--chunk 32] [--seg_height 512] [--seg_width 1088] [--passes 5] [--reps 20]

``rendered``: the target is a rendered scene's (two icospheres of ``--subdiv`` subdivisions through ``RenderedSegDataset``, no noise:
mostly background) and the logits are the one-hot of that target with about 1 % of the labels moved to a class drawn at random, so
nearly every pixel of a wave lands in cell (0, 0).  ``uniform``: N(0, 1) logits against a target drawn uniformly from the classes, which
hits every cell and makes a wave walk up to 64 distinct cells per tile.  A pass is ``--reps`` calls between two device events; every
figure is the median per call over ``--passes`` passes after one warm-up pass, with the smallest and largest pass next to it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from densefusion_amd import _lib  # noqa: E402
from densefusion_amd.datasets.customCAD import render as cr  # noqa: E402

CASES = ((3, 4), (22, 24))


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdiv", type=int, default=4, help="subdivisions of the generated icospheres")
    ap.add_argument("--seg_height", type=int, default=None)
    ap.add_argument("--seg_width", type=int, default=None)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed pass")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--flip", type=float, default=0.01, help="share of the rendered labels the logits get wrong")
    cr.add_view_arguments(ap)
    return ap


def spread(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def device_ms(fn, passes, reps):
    """device milliseconds per call of ``fn()``: ``passes`` timed passes of ``reps`` calls after one warm-up pass"""
    out = []
    for k in range(passes + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        if k:
            out.append(a.elapsed_time(b) / reps)
    return out


def rendered_target(opt, window, dev):
    """[chunk,H,W] int64: the targets of one chunk of rendered scenes, classes 0..2"""
    from densefusion_amd.datasets.customCAD.online_seg import RenderedSegDataset
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cad_raster_np as mnp
    rng = np.random.default_rng(12)
    models = []
    for radius in (60.0, 45.0):
        v, f = mnp.icosphere(opt.subdiv, radius)
        models.append((v.astype(np.float32), np.asarray(f, dtype=np.int32), rng.integers(0, 256, (len(v), 3), dtype=np.uint8)))
    ds = RenderedSegDataset.from_options(opt, models, first_seed=opt.seed, frames=opt.chunk, use_noise=False, window=window, device=dev)
    return ds.batch(range(opt.chunk))[1].contiguous()


def main(argv=None):
    opt = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("seg_score_bench needs a GPU (no CPU path)")
    from densefusion_amd.datasets.customCAD.online_seg import default_window
    dev = torch.device("cuda", torch.cuda.current_device())
    h, w = default_window((opt.height, opt.width))
    H, W = opt.seg_height or h, opt.seg_width or w
    F = opt.chunk
    gen = torch.Generator(device=dev).manual_seed(opt.seed)
    scene = rendered_target(opt, (H, W), dev)
    L = _lib.lib()
    out = {"chunk": F, "window": [H, W], "passes": opt.passes, "reps": opt.reps, "flip": opt.flip,
           "background_share": float((scene == 0).double().mean()), "cases": []}
    for C, ld in CASES:
        conf = torch.empty(F, C, C, dtype=torch.int32, device=dev)
        skipped = torch.empty(F, dtype=torch.int32, device=dev)
        label = torch.empty(F, H, W, dtype=torch.int32, device=dev)
        read = F * H * W * (4 * ld + 8)
        src = torch.empty(read, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        for name in ("rendered", "uniform"):
            if name == "rendered":
                target = scene
                wrong = torch.rand(scene.shape, device=dev, generator=gen) < opt.flip
                said = torch.where(wrong, torch.randint(0, C, scene.shape, device=dev, generator=gen), scene)
                logits = torch.zeros(F, H, W, ld, device=dev)
                logits.scatter_(3, said[..., None], 1.0)
                del wrong, said
            else:
                target = torch.randint(0, C, (F, H, W), device=dev, generator=gen)
                logits = torch.randn(F, H, W, ld, device=dev, generator=gen)

            def call():
                st = L.df_seg_score(logits.data_ptr(), target.data_ptr(), F, H, W, ld, C, label.data_ptr(), conf.data_ptr(), skipped.data_ptr(),
                                    _lib.current_stream())
                _lib.check(st, "seg_score")
            with _lib.device_guard(dev):
                score = spread(device_ms(call, opt.passes, opt.reps))
            copy = spread(device_ms(lambda: dst.copy_(src), opt.passes, opt.reps))
            cells = int((conf.sum(dim=0) > 0).sum())
            assert int(conf.sum()) + int(skipped.sum()) == F * H * W
            out["cases"].append({"C": C, "ld": ld, "input": name, "bytes_read": read, "cells_hit": cells, "seg_score_ms": score,
                                 "copy_ms_same_bytes": copy, "seg_score_over_copy": score["median"] / copy["median"],
                                 "read_GBps": read / score["median"] / 1e6})
            del logits
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
