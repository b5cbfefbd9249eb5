"""Time ``df_pose_refine_dense`` (lib.pose_refine_dense.DensePoseRefiner.refine) against what it is built beside, in
tools/pose_verify_bench.py's setup: B = 64 items with 160 x 160 windows on 480 x 640 frames rendered by ``df_cad_render_mesh``, ellipsoid
icospheres of 5 120 and 81 920 triangles, start poses a little off the rendered ones, device events around one call, the median of 5
calls after one warm-up with the range.  Per mesh: one dense call at iters = 0 and one at iters = 10; next to them iters + 1 = 11
``df_pose_verify`` calls on the same items, ``df_mesh_icp_tree`` with 10 steps on 500 observed points per item, and a plain device copy of
the bytes one accumulation pass reads (8-byte key, 2-byte depth code and three 8-byte ray components per window node: 34 bytes).
One JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from densefusion_amd.datasets.customCAD import render as cad_render  # noqa: E402
from densefusion_amd.datasets.customCAD.project_unity_depth import UnityDepthProjector  # noqa: E402
from densefusion_amd.lib.mesh_icp import MeshIcp  # noqa: E402
from densefusion_amd.lib.pose_refine_dense import DensePoseRefiner  # noqa: E402
from densefusion_amd.lib.pose_verify import PoseVerifier  # noqa: E402
from pose_verify_bench import B, IH, IW, RADIUS, SCALE, WIN, icosphere, quat_to_matrix, summary, timed  # noqa: E402

ITERS, GATE, POINTS = 10, 200, 500


def bench_mesh(level, calls, rng):
    v, t = icosphere(level)
    v = (v * np.array([1.0, 0.7, 0.5]) * RADIUS).astype(np.float32)
    proj = np.array(cad_render.DEFAULT_PROJ, dtype=np.float64)
    quat = rng.normal(size=(B, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    trans = np.stack([rng.uniform(-800, 800, B), rng.uniform(-300, 300, B), rng.uniform(-4400, -3800, B)], axis=1)
    poses = np.stack([np.concatenate([quat_to_matrix(q), tr[:, None]], axis=1) for q, tr in zip(quat, trans)])
    renderer = cad_render.CadMeshRenderer(v, t, np.full((len(v), 3), 128, dtype=np.uint8), proj, (IH, IW), model_scale=SCALE)
    _, depth, mask, _ = renderer.render(poses, cull=1, mask="pixels")
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    # starts a little off the rendered poses: a turn of about a degree and a few units of shift (the ellipsoid's radius is 750 units)
    start = up(np.concatenate([quat + rng.normal(scale=0.01, size=(B, 4)), trans + rng.normal(scale=3.0, size=(B, 3))], axis=1), np.float64)
    frame = torch.arange(B, dtype=torch.int32, device="cuda")
    obj = torch.zeros(B, dtype=torch.int32, device="cuda")
    cx = ((proj[0, 0] * trans[:, 0] + proj[0, 2] * trans[:, 2]) / -trans[:, 2] + 1.0) * IW * 0.5
    cy = (1.0 - (proj[1, 1] * trans[:, 1] + proj[1, 2] * trans[:, 2]) / -trans[:, 2]) * IH * 0.5
    corner = up(np.stack([np.rint(cy) - WIN // 2, np.rint(cx) - WIN // 2], axis=1), np.int32)
    udp = UnityDepthProjector.from_matrix(proj, (IH, IW))
    ref = DensePoseRefiner([(v, t)], SCALE, proj, (IH, IW), cloud_div=1.0).set_rays(udp.ray_map_on("cuda"))
    ver = PoseVerifier([(v, t)], SCALE, proj, (IH, IW), cloud_div=1.0)
    items = torch.cat([frame[:, None], obj[:, None], corner, frame[:, None], torch.full_like(frame, 65535)[:, None]], dim=1).contiguous()
    dense = lambda iters: ref.refine(depth, start, frame, obj, corner, (WIN, WIN), iters=iters, gate=GATE, cull=True)
    pose10, stats10 = dense(ITERS)
    stats10 = stats10.cpu().numpy()

    def verify_calls():
        for _ in range(ITERS + 1):
            ver.score_items(depth, start, items, (WIN, WIN), 4, mask=mask, cull=True)
    # 500 observed points per item, from the mask's own nodes (the loader's cloud: ray x depth)
    dh, mh = depth.cpu().numpy(), mask.cpu().numpy()
    cloud = np.zeros((B, POINTS, 3), dtype=np.float32)
    for b in range(B):
        r, q = np.nonzero((mh[b] != 0) & (dh[b] != 65535))
        pick = rng.choice(len(r), POINTS, replace=len(r) < POINTS)
        cloud[b] = udp.project_depth(dh[b])[r[pick], q[pick]]
    icp = MeshIcp([(v, t)], SCALE, accel=True)
    points = up(cloud, np.float32)
    sparse = lambda: icp.refine(points, start, obj, iters=ITERS, max_dist=[0.1 * 2 * RADIUS * SCALE], cull=True)
    _, sstats = sparse()
    sstats = sstats.cpu().numpy()
    nbytes = B * WIN * WIN * 34
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    d0, d10, vcalls, tree, copy = (summary(timed(f, calls)) for f in (lambda: dense(0), lambda: dense(ITERS), verify_calls, sparse,
                                                                      lambda: dst.copy_(src)))
    ok = stats10[:, 0] == 0
    return dict(triangles=len(t), dense_iters0_call=d0, dense_iters10_call=d10, verify_11_calls=vcalls, mesh_icp_tree_10_steps_500_points=tree,
                copy_of_accumulation_bytes=copy, accumulation_bytes=nbytes, dense_per_pass_ms=(d10["median_ms"] - d0["median_ms"]) / ITERS,
                dense10_over_verify11=d10["median_ms"] / vcalls["median_ms"], dense10_over_mesh_icp_tree=d10["median_ms"] / tree["median_ms"],
                status_ok=int(ok.sum()), few=int((stats10[:, 0] == 1).sum()), degenerate=int((stats10[:, 0] == 2).sum()),
                mean_inliers_first=float(stats10[:, 1].mean()), mean_inliers_last=float(stats10[:, 3].mean()),
                mean_rms_first=float(stats10[ok, 2].mean()) if ok.any() else 0.0, mean_rms_last=float(stats10[ok, 4].mean()) if ok.any() else 0.0,
                mesh_icp_mean_rms_first=float(sstats[:, 2].mean()), mesh_icp_mean_rms_last=float(sstats[:, 4].mean()))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--levels", type=int, nargs="+", default=[4, 6], help="icosphere subdivisions: 4 = 5 120 triangles, 6 = 81 920")
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("pose_dense_bench.py needs a GPU")
    rng = np.random.default_rng(0)
    out = dict(bench="pose_refine_dense", items=B, window=[WIN, WIN], frame=[IH, IW], calls=opt.calls, iters=ITERS, gate=GATE, points=POINTS,
               meshes=[bench_mesh(level, opt.calls, rng) for level in opt.levels])
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
