#!/usr/bin/env python
"""Items per second out of ``train_utils.Prefetcher`` for the two ways to feed customCAD training: ``RenderedPoseDataset`` (views
rendered on the fly, datasets/customCAD/online.py) and ``PoseDataset`` over a tree tools/render_cad_dataset.py wrote from the same
seeds with the same options -- same machine, same ``--workers``, training augmentation on for both, the jitter on the device.  One
JSON line.

    python tools/cad_feed_bench.py [--model M.ply] [--frames 512] [--workers 4] [--feed processes] [the render tool's view options]

Without ``--model`` an icosphere of ``--subdiv`` subdivisions (radius 60 file units, tests/cad_raster_np.py builds it) is written to the
work directory and drawn with ``--raster mesh``.  A pass hands every item of the set over in the order a training epoch takes it and
ends with a device synchronise; the rate is the median over ``--passes`` passes (default 5) after one warm-up pass, by the host clock.
The disk loader is fed the way ``tools/train.py --feed`` feeds it (``processes``: its worker processes decode; ``threads``); the
rendering set has no CPU half and is always fed from ``--workers`` threads.  The tree holds the first ``--frames`` kept views; the
rendering set serves the views of as many seeds, its skipped views as sentinels (reported: they cost their render and yield no item).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from densefusion_amd import train_utils  # noqa: E402
from densefusion_amd.datasets.customCAD import render as cr  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", type=str, default=None, help="PLY model; default: a generated icosphere, drawn with --raster mesh")
    ap.add_argument("--subdiv", type=int, default=5, help="subdivisions of the generated icosphere")
    ap.add_argument("--frames", type=int, default=512, help="frames of the tree = view seeds of the rendering set")
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--feed", type=str, default="processes", choices=["processes", "threads"], help="how the disk loader is fed")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise_trans", type=float, default=0.005)
    ap.add_argument("--work_dir", type=str, default=None, help="where the model and the tree go; default: a temporary directory")
    cr.add_view_arguments(ap)
    return ap


def view_argv(opt):
    """the view options of ``opt`` as the render tool's command line"""
    argv = []
    for action in cr.add_view_arguments(argparse.ArgumentParser())._actions:
        value = getattr(opt, action.dest, None)
        if action.dest == "help" or value is None:
            continue
        argv += [action.option_strings[0]] + [str(v) for v in (value if isinstance(value, list) else [value])]
    return argv


def rate(dataset, order, dev, workers, processes, passes):
    """(items per second: the median over ``passes`` passes after one warm-up, every pass's rate, sentinels per pass)"""
    pf = train_utils.Prefetcher(dataset, order, dev, workers=workers, processes=processes)
    rates, sentinels = [], 0
    try:
        for k in range(passes + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sentinels = sum(1 for item in pf if item[0].dim() == 1)
            torch.cuda.synchronize()
            if k:
                rates.append(len(order) / (time.perf_counter() - t0))
    finally:
        pf.close()
    return float(np.median(rates)), rates, sentinels


def main(argv=None):
    ap = build_parser()
    ap.set_defaults(raster=None)
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("cad_feed_bench needs a GPU (no CPU path)")
    import render_cad_dataset as tool
    from densefusion_amd.datasets.customCAD.dataset import PoseDataset
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    dev = torch.device("cuda", torch.cuda.current_device())
    with tempfile.TemporaryDirectory() as tmp:
        work = opt.work_dir or tmp
        os.makedirs(work, exist_ok=True)
        if opt.model is None:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import cad_raster_np as mnp
            v, f = mnp.icosphere(opt.subdiv, 60.0)
            opt.model = mnp.write_mesh_ply(os.path.join(work, "icosphere.ply"), v.astype(np.float32), f,
                                           np.random.default_rng(12).integers(0, 256, (len(v), 3), dtype=np.uint8))
            opt.raster = opt.raster or "mesh"
        opt.raster = opt.raster or "points"
        tree = os.path.join(work, "tree")
        t0 = time.perf_counter()
        written = tool.main(["--model", opt.model, "--output_root", tree, "--frames", str(opt.frames), "--seed", str(opt.seed)] + view_argv(opt))
        write_s = time.perf_counter() - t0
        np.random.seed(opt.seed)
        disk = PoseDataset("train", 500, True, tree, opt.noise_trans, False, jitter="device")
        online = RenderedPoseDataset.from_options(opt, [opt.model], first_seed=opt.seed, frames=opt.frames, num=500, add_noise=True,
                                                  noise_trans=opt.noise_trans)
        rs = np.random.RandomState(opt.seed)
        out = {"frames": opt.frames, "image": [opt.height, opt.width], "raster": opt.raster, "workers": opt.workers, "passes": opt.passes,
               "tree_written": written["written"], "tree_skipped": written["skipped"], "tree_write_s": write_s}
        r, every, sent = rate(online, online.permutation(rs), dev, opt.workers, 0, opt.passes)
        out.update(online_items_per_s=r, online_passes=every, online_items=len(online), online_sentinels=sent, online_chunk=online.chunk)
        r, every, sent = rate(disk, rs.permutation(len(disk)), dev, opt.workers, opt.workers if opt.feed == "processes" else 0, opt.passes)
        out.update(disk_items_per_s=r, disk_passes=every, disk_items=len(disk), disk_sentinels=sent, disk_feed=opt.feed)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
