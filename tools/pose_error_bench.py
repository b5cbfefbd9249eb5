#!/usr/bin/env python
"""What the symmetry-aware BOP pose errors cost on the device: one ``df_pose_sym_error`` call (``lib.pose_error.PoseErrors.sym_error``)
for B = 64 items on the squashed icospheres of tools/pose_verify_bench.py (``icosphere(4)``: 2 562 vertices, ``icosphere(6)``: 40 962)
with symmetry sets of 1, 8 and 630 rotations; in the same run the fp64 vector rate of the part (``df_fp64_rate_probe``, a register-only
multiply / add loop), one ``df_pose_verify`` call and one ``df_pose_vsd`` call (ten tau) on the same meshes and poses (160 x 160 windows
on 480 x 640 frames, as pose_verify_bench.py sets them up).  Device events around one call, the median of ``--calls`` calls after one warm-up, with the range.
``fp64_ops`` is the contract's own count per (vertex, symmetry) pair (include/dfusion.h: 58, one of them a division); compares and
selects are not counted and the probe's rate counts multiplies and adds the same way.  The numpy restatement (tests/pose_error_np.py)
is timed once on a slice of the largest case (one item, eight symmetries, every vertex) and extrapolated to the whole of it by the
pair count; the JSON says so.  One JSON line.

    python tools/pose_error_bench.py [--levels 4 6] [--sets 1 8 630] [--calls 5]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_verify_bench as pvb  # noqa: E402
from densefusion_amd import _lib  # noqa: E402
from densefusion_amd.datasets.customCAD import render as cad_render  # noqa: E402
from densefusion_amd.lib.pose_error import PoseErrors  # noqa: E402
from densefusion_amd.lib.pose_verify import PoseVerifier  # noqa: E402

OPS_PER_PAIR = 58
PROBE_OPS_PER_ROUND = 16
IH, IW, B, WIN, RADIUS, SCALE = pvb.IH, pvb.IW, pvb.B, pvb.WIN, pvb.RADIUS, pvb.SCALE


def rotation_z(angle):
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def symmetry_set(n):
    """[n,3,4] about the origin: the identity alone, or n / 2 turns about z each also followed by a half turn about x (n even)"""
    if n == 1:
        return np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)[None]
    turns = [rotation_z(2 * math.pi * k / (n // 2)) for k in range(n // 2)]
    flip = np.diag([1.0, -1.0, -1.0])
    return np.stack([np.concatenate([R, np.zeros((3, 1))], axis=1) for R in turns + [flip @ R for R in turns]])


def bench_mesh(level, sets, calls, rng, peak, numpy_slice):
    v, t = pvb.icosphere(level)
    v = (v * np.array([1.0, 0.7, 0.5]) * RADIUS).astype(np.float32)
    proj = np.array(cad_render.DEFAULT_PROJ, dtype=np.float64)
    quat = rng.normal(size=(B, 4))
    trans = np.stack([rng.uniform(-800, 800, B), rng.uniform(-300, 300, B), rng.uniform(-4400, -3800, B)], axis=1)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    gt = np.concatenate([quat, trans], axis=1)
    est = gt + np.concatenate([rng.normal(scale=0.05, size=(B, 4)), rng.normal(scale=5.0, size=(B, 3))], axis=1)
    pose_gt, pose_est, obj = up(gt, np.float64), up(est, np.float64), torch.zeros(B, dtype=torch.int32, device="cuda")
    out = dict(vertices=len(v), triangles=len(t), sets=[])
    for n in sets:
        pe = PoseErrors([(v, t)], SCALE, [symmetry_set(n)], proj, (IH, IW), cloud_div=1.0)
        ms = pvb.summary(pvb.timed(lambda: pe.sym_error(pose_est, pose_gt, obj), calls))
        pairs = B * len(v) * n
        row = pe.sym_error(pose_est, pose_gt, obj).cpu().numpy()
        tops = pairs * OPS_PER_PAIR / ms["median_ms"] / 1e9
        out["sets"].append(dict(symmetries=n, sym_error_call=ms, pairs=pairs, Gpairs_per_s=pairs / ms["median_ms"] / 1e6, fp64_Tops=tops,
                                share_of_probe_rate=tops / peak, mean_mssd=float(row[:, 1].mean()), mean_mspd=float(row[:, 3].mean())))
        if numpy_slice and n == max(sets):
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import pose_error_np as pn
            x = (v.astype(np.float64) * SCALE).astype(np.float32).astype(np.float64)
            t0 = time.perf_counter()
            pn.item_maxima(x, est[0], gt[0], symmetry_set(n)[:8], proj, IH, IW)
            dt = time.perf_counter() - t0
            out["numpy_restatement"] = dict(slice_pairs=len(v) * 8, slice_s=dt, extrapolated_to_pairs=pairs, extrapolated_s=dt * pairs / (len(v) * 8),
                                            note="one item x 8 symmetries x every vertex timed on the host; the whole case is extrapolated by the pair count")
    # one df_pose_verify call on the same mesh and true poses, against frames rendered at those poses
    poses = np.stack([np.concatenate([pvb.quat_to_matrix(q), tr[:, None]], axis=1) for q, tr in zip(quat, trans)])
    renderer = cad_render.CadMeshRenderer(v, t, np.full((len(v), 3), 128, dtype=np.uint8), proj, (IH, IW), model_scale=SCALE)
    _, depth, mask, _ = renderer.render(poses, cull=1, mask="pixels")
    ver = PoseVerifier([(v, t)], SCALE, proj, (IH, IW), cloud_div=1.0)
    frame = torch.arange(B, dtype=torch.int32, device="cuda")
    cx = ((proj[0, 0] * trans[:, 0] + proj[0, 2] * trans[:, 2]) / -trans[:, 2] + 1.0) * IW * 0.5
    cy = (1.0 - (proj[1, 1] * trans[:, 1] + proj[1, 2] * trans[:, 2]) / -trans[:, 2]) * IH * 0.5
    corner = up(np.stack([np.rint(cy) - WIN // 2, np.rint(cx) - WIN // 2], axis=1), np.int32)
    items = torch.cat([frame[:, None], obj[:, None], corner, frame[:, None], torch.full_like(frame, 65535)[:, None]], dim=1).contiguous()
    out["verify_call"] = pvb.summary(pvb.timed(lambda: ver.score_items(depth, pose_gt, items, (WIN, WIN), 0, mask=mask, cull=True), calls))
    # one df_pose_vsd call on the same items: both poses drawn, ten tau, the BOP delta
    from densefusion_amd.datasets.customCAD.project_unity_depth import UnityDepthProjector
    scorer = PoseErrors([(v, t)], SCALE, [symmetry_set(1)], proj, (IH, IW), cloud_div=1.0).set_rays(
        UnityDepthProjector.from_matrix(proj, (IH, IW)).ray_map_on(obj.device))
    diameter = 2.0 * RADIUS * SCALE
    tau = np.array([0.05 * k * diameter for k in range(1, 11)])
    out["vsd_call"] = pvb.summary(pvb.timed(lambda: scorer.vsd(depth, pose_est, pose_gt, frame, obj, corner, (WIN, WIN), [0.075 * diameter], tau, cull=True), calls))
    out["vsd_over_verify_call"] = out["vsd_call"]["median_ms"] / out["verify_call"]["median_ms"]
    st = scorer.vsd(depth, pose_est, pose_gt, frame, obj, corner, (WIN, WIN), [0.075 * diameter], tau, cull=True).cpu().numpy()
    out["vsd_mean_union"], out["vsd_mean_inter"] = float(st[:, 1].mean()), float(st[:, 2].mean())
    for s in out["sets"]:
        s["over_verify_call"] = s["sym_error_call"]["median_ms"] / out["verify_call"]["median_ms"]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--levels", type=int, nargs="+", default=[4, 6], help="icosphere subdivisions: 4 = 2 562 vertices, 6 = 40 962")
    ap.add_argument("--sets", type=int, nargs="+", default=[1, 8, 630], help="symmetry set sizes (1 or even)")
    ap.add_argument("--probe_blocks", type=int, default=2048, help="workgroups of the fp64 rate loop (256 lanes each)")
    ap.add_argument("--probe_iters", type=int, default=200000, help="rounds of 16 fp64 operations a lane runs")
    ap.add_argument("--no_numpy", action="store_true", help="skip the host timing of the restatement")
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("pose_error_bench.py needs a GPU (no CPU path)")
    if any(n != 1 and n % 2 for n in opt.sets):
        raise SystemExit("--sets: 1 or an even size")
    L = _lib.lib()
    sink = torch.empty(opt.probe_blocks * 256, dtype=torch.float64, device="cuda")

    def probe():
        _lib.check(L.df_fp64_rate_probe(opt.probe_blocks, opt.probe_iters, sink.data_ptr(), _lib.current_stream()), "fp64_rate_probe")
    probe_ms = pvb.summary(pvb.timed(probe, opt.calls))
    peak = opt.probe_blocks * 256 * opt.probe_iters * PROBE_OPS_PER_ROUND / probe_ms["median_ms"] / 1e9      # Tops/s
    rng = np.random.default_rng(0)
    out = dict(bench="pose_error", items=B, frame=[IH, IW], calls=opt.calls, ops_per_pair=OPS_PER_PAIR,
               fp64_probe=dict(blocks=opt.probe_blocks, iters=opt.probe_iters, call=probe_ms, fp64_Tops=peak),
               meshes=[bench_mesh(level, opt.sets, opt.calls, rng, peak, not opt.no_numpy and level == max(opt.levels)) for level in opt.levels])
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
