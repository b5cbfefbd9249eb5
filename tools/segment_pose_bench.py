#!/usr/bin/env python
"""Dev tool: the SegNet -> detections -> poses pipeline (densefusion_amd.lib.segment_pose) on windows of 480 x 640 frames.

Seeded synthetic weights: the colour-block SegNet (synth.make_segnet_block_state_dict; its forward costs what any SegNet's does),
seeded PoseNet / refiner weights, frames of five coloured blocks of 32 x 32 cells (3 detections per frame: one per colour).
Reports, per frame:
  * SegNet eval forward ms;
  * the input kernel and the label / statistics / detection call in us, with their fraction of 6.3 TB/s on algorithmic bytes
    (input: rgb read once, fp32 NHWC4 written once; label call: logits read once at ld channels, depth once, label written once);
    the label call on the block SegNet's logits (1 - 2 classes per wave) and on N(0, 1) logits (every class in every wave);
  * the pose stage ms: WindowEstimator.run over the window's detections, timed between events on the slot stream it runs on,
    and by the host clock to a full sync;
  * the segmentation half alone, window by window with its upload and table sync;
  * end-to-end frames/s through SegmentPoseEstimator at depth 1 and 2, and its ratio to SegNet alone + pose stage alone.

    python tools/segment_pose_bench.py [--frames 8] [--windows 12] [--reps 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from densefusion_amd import synth  # noqa: E402
from densefusion_amd.lib import segment  # noqa: E402
from densefusion_amd.lib.eval_window import WindowEstimator  # noqa: E402
from densefusion_amd.lib.network import PoseNet, PoseRefineNet  # noqa: E402
from densefusion_amd.lib.segment_pose import SegmentPoseEstimator  # noqa: E402
from densefusion_amd.vanilla_segmentation.segnet import SegNet  # noqa: E402

HBM = 6.3e12
H, W, K = 480, 640, 21


def timed(fn, reps, stream=None):
    """ms per call of fn, between events on `stream` (default: the current one): the stream fn's work runs on."""
    fn()
    torch.cuda.synchronize()
    stream = stream if stream is not None else torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def frames(rng, n):
    out = []
    for i in range(n):
        blocks = [(1 + (i + j) % 3, int(rng.integers(0, 12)), int(rng.integers(0, 16)), int(rng.integers(2, 4)), int(rng.integers(2, 5)))
                  for j in range(5)]
        out.append(synth.block_frame(rng, blocks, H, W))
    return np.stack([f[0] for f in out]), np.stack([f[1] for f in out])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--num_points", type=int, default=1000)
    ap.add_argument("--iteration", type=int, default=2)
    ap.add_argument("--min_pixels", type=int, default=2, help="the block SegNet labels one pixel per 32 x 32 cell")
    opt = ap.parse_args(argv)
    Fn, dev = opt.frames, torch.device("cuda")
    segnet = SegNet(label_nbr=K + 1)
    segnet.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_segnet_block_state_dict(K + 1).items()})
    segnet = segnet.to(dev).eval()
    est, rfn = PoseNet(opt.num_points, K), PoseRefineNet(opt.num_points, K)
    est.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(synth.posenet_spec(K), 21).items()})
    rfn.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(synth.refiner_spec(K), 1021).items()})
    est, rfn = est.to(dev).eval(), rfn.to(dev).eval()
    rng = np.random.default_rng(0)
    rgb_np, depth_np = frames(rng, Fn * opt.windows)
    rgb_h, depth_h = torch.from_numpy(rgb_np).pin_memory(), torch.from_numpy(depth_np.view(np.int16)).pin_memory()
    rgb, depth = rgb_h[:Fn].to(dev), depth_h[:Fn].to(dev)
    res = {"frames_per_window": Fn, "H": H, "W": W}

    x4 = segment.segment_input(rgb)
    ms = timed(lambda: segment.segment_input(rgb, x4), opt.reps)
    nb = Fn * H * W * (3 + 16)
    res["input_us"], res["input_hbm_frac"] = ms * 1e3, nb / (ms * 1e-3) / HBM
    ms = timed(lambda: segnet.forward_nhwc(x4), max(2, opt.reps // 4))
    res["segnet_ms_per_frame"] = ms / Fn
    logits = segnet.forward_nhwc(x4)
    ld = logits.shape[-1]
    nb = Fn * H * W * (ld * 4 + 2 + 4)
    label = torch.empty(Fn, H, W, dtype=torch.int32, device=dev)
    for name, lg in (("segnet", logits), ("randn", torch.randn_like(logits))):
        ms = timed(lambda: segment.detect(lg, K + 1, depth, K, opt.min_pixels, label), opt.reps)
        res[f"detect_{name}_us"], res[f"detect_{name}_hbm_frac"] = ms * 1e3, nb / (ms * 1e-3) / HBM
    seg = segment.detect(logits, K + 1, depth, K, opt.min_pixels, label)
    res["detections_per_frame"] = float(seg.ndet.float().mean())

    # pose stage alone: the window's detections on frames already resident
    we = WindowEstimator(est, rfn, opt.num_points, opt.iteration, Fn, (H, W), depth=1)
    det, ndet = seg.det.cpu().numpy(), seg.ndet.cpu().numpy()
    dets = [(f, int(r[0]), segment.det_row_to_roi(r), f * 64 + i) for f in range(Fn) for i, r in enumerate(det[f, :ndet[f]])]
    slot = we.upload(rgb_h[:Fn], depth_h[:Fn], torch.from_numpy(seg.label.cpu().numpy()))
    torch.cuda.synchronize()
    reps = max(2, opt.reps // 4)
    ms = timed(lambda: we.run(slot, Fn, dets), reps, slot["stream"])        # WindowEstimator.run enqueues on the slot's stream
    res["pose_ms_per_frame"] = ms / Fn
    t0 = time.perf_counter()                                                # the same, host wall clock to a full sync
    for _ in range(reps):
        we.run(slot, Fn, dets)
    torch.cuda.synchronize()
    res["pose_wall_ms_per_frame"] = (time.perf_counter() - t0) * 1e3 / (reps * Fn)

    # segmentation alone, window by window as the pipeline runs it: upload, segment_frames, the table to the host, wait
    def seg_only(nwin):
        for w in range(nwin):
            rgb_d = rgb_h[w * Fn:(w + 1) * Fn].to(dev, non_blocking=True)
            depth_d = depth_h[w * Fn:(w + 1) * Fn].to(dev, non_blocking=True)
            segment.segment_frames(segnet, rgb_d, depth_d, K, opt.min_pixels).ndet.cpu()
    seg_only(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seg_only(opt.windows)
    res["seg_only_ms_per_frame"] = (time.perf_counter() - t0) * 1e3 / (opt.windows * Fn)

    # end to end: host frames in, poses out
    for depth_in_flight in (1, 2):
        spe = SegmentPoseEstimator(segnet, est, rfn, opt.num_points, opt.iteration, Fn, depth_in_flight, opt.min_pixels, (H, W))

        def run_all(nwin):
            pending = []
            for w in range(nwin):
                while len(pending) >= depth_in_flight:
                    spe.collect(pending.pop(0))
                pending.append(spe.submit(rgb_h[w * Fn:(w + 1) * Fn], depth_h[w * Fn:(w + 1) * Fn]))
            while pending:
                spe.collect(pending.pop(0))
        run_all(depth_in_flight + 1)                   # every slot once: its stream's allocations and workspaces exist
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_all(opt.windows)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[f"e2e_fps_depth{depth_in_flight}"] = opt.windows * Fn / dt
        res[f"e2e_ms_per_frame_depth{depth_in_flight}"] = dt * 1e3 / (opt.windows * Fn)
    for d in (1, 2):
        res[f"e2e_over_parts_depth{d}"] = res[f"e2e_ms_per_frame_depth{d}"] / (res["segnet_ms_per_frame"] + res["pose_ms_per_frame"])
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
