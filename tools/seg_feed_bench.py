#!/usr/bin/env python
"""What feeding SegNet from rendered customCAD scenes costs (``RenderedSegDataset``, datasets/customCAD/online_seg.py): batches per
second out of ``train_utils.Prefetcher``, the device time of ``df_seg_batch`` for one chunk, and next to it the device time of a
plain device-to-device copy of as many bytes as that call writes -- same machine, same run.  One JSON line.

    python tools/seg_feed_bench.py [--model A.ply B.ply] [--frames 256] [--batch_size 4] [--workers 4] [the render tool's view options]

Without ``--model`` two icospheres of ``--subdiv`` subdivisions (radii 60 and 45 file units, tests/cad_raster_np.py builds them) are
drawn.  Backgrounds are ``--backgrounds DIR`` or, without it, ``--pool`` random images of the frame's size.  A pass hands every batch
of the set over in the order a training epoch takes it and ends with a device synchronise (host clock); the kernel and the copy are
timed with device events around one call each.  Every figure is the median over ``--passes`` passes (default 5) after one warm-up
pass, with the smallest and largest pass next to it.
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
sys.path.insert(0, ROOT)
from densefusion_amd import train_utils  # noqa: E402
from densefusion_amd.datasets.customCAD import render as cr  # noqa: E402
from densefusion_amd.lib import preprocess as pp  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", type=str, nargs="+", default=None, help="PLY meshes; default: two generated icospheres")
    ap.add_argument("--subdiv", type=int, default=4, help="subdivisions of the generated icospheres")
    ap.add_argument("--frames", type=int, default=256, help="views per pass")
    ap.add_argument("--batch_size", type=int, default=4)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--seg_height", type=int, default=None)
    ap.add_argument("--seg_width", type=int, default=None)
    ap.add_argument("--backgrounds", type=str, default=None)
    ap.add_argument("--pool", type=int, default=8, help="random backgrounds when --backgrounds is not given (0: none)")
    cr.add_view_arguments(ap)
    return ap


def spread(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def device_ms(fn, passes):
    """device milliseconds of ``fn()``: ``passes`` timed calls after one warm-up call"""
    out = []
    for k in range(passes + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k:
            out.append(a.elapsed_time(b))
    return out


def main(argv=None):
    opt = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("seg_feed_bench needs a GPU (no CPU path)")
    from densefusion_amd.datasets.customCAD.online_seg import RenderedSegDataset, default_window
    dev = torch.device("cuda", torch.cuda.current_device())
    if opt.model is None:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import cad_raster_np as mnp
        rng = np.random.default_rng(12)
        models = []
        for radius in (60.0, 45.0):
            v, f = mnp.icosphere(opt.subdiv, radius)
            models.append((v.astype(np.float32), np.asarray(f, dtype=np.int32), rng.integers(0, 256, (len(v), 3), dtype=np.uint8)))
    else:
        models = list(opt.model)
    h, w = default_window((opt.height, opt.width))
    window = (opt.seg_height or h, opt.seg_width or w)
    back = opt.backgrounds
    if back is None and opt.pool > 0:
        back = np.random.default_rng(3).integers(0, 256, (opt.pool, opt.height, opt.width, 3), dtype=np.uint8)
    ds = RenderedSegDataset.from_options(opt, models, first_seed=opt.seed, frames=opt.frames, use_noise=True, window=window, backgrounds=back)
    out = {"frames": opt.frames, "image": [opt.height, opt.width], "window": list(window), "chunk": ds.chunk, "batch_size": opt.batch_size,
           "workers": opt.workers, "passes": opt.passes, "classes": ds.n_classes, "light": opt.light,
           "backgrounds": 0 if ds.pool is None else ds.pool[0]}

    # 1. batches per second out of the Prefetcher, in a training epoch's order
    batches = ds.batches(ds.permutation(np.random.RandomState(opt.seed)), opt.batch_size)
    pf = train_utils.Prefetcher(batches, range(len(batches)), dev, workers=opt.workers)
    rates = []
    try:
        for k in range(opt.passes + 1):
            ds._cache.clear()                                      # every pass renders every chunk again
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = sum(1 for _ in pf)
            torch.cuda.synchronize()
            if k:
                rates.append(n / (time.perf_counter() - t0))
    finally:
        pf.close()
    out["batches_per_s"] = spread(rates)
    out["frames_per_s"] = spread([r * opt.batch_size for r in rates])

    # 2. df_seg_batch alone on one chunk's frames, and a plain copy of the bytes it writes
    F = min(ds.chunk, opt.frames)
    seeds = [opt.seed + j for j in range(F)]
    _, poses, present = cr.draw_scene_records(seeds, ds._n_points, ds._centroids, ds.n_models, ds.center, ds.scene_scale, ds.model_scale,
                                              ds.max_holes, p_present=ds.p_present, lateral=ds.lateral, depth=ds.depth, hole_mean=ds.hole_mean,
                                              hole_std=ds.hole_std, private=True)
    light = np.stack([cr.draw_light(ds.light, s, ds.light_angle)[1] for s in seeds]) if ds.light != "none" else None
    rgb, _, label, _ = ds.renderer.render(poses, present=present, cull=ds.cull, light=light)
    desc = torch.from_numpy(np.array([[j] + ds._draws(j)[1] for j in range(F)], dtype=np.int64).astype(np.int32)).to(dev)
    call = lambda: pp.seg_batch(rgb, label, ds.class_map, ds.n_classes, desc, window, back=ds.back, blur=ds.blur, noise_mul=ds.noise_mul)
    out["seg_batch_ms_per_chunk"] = spread(device_ms(call, opt.passes))
    written = F * window[0] * window[1] * (16 + 8) + F * ds.n_classes * 4
    src = torch.empty(written, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    out["copy_ms_same_bytes"] = spread(device_ms(lambda: dst.copy_(src), opt.passes))
    out["bytes_written_per_chunk"] = written
    out["seg_batch_over_copy"] = out["seg_batch_ms_per_chunk"]["median"] / out["copy_ms_same_bytes"]["median"]
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
