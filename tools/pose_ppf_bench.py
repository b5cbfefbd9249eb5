"""Time ``df_pose_ppf`` (lib.pose_ppf.PpfEstimator.estimate) in tools/pose_dense_bench.py's setup: B = 64 items with 160 x 160 windows on
480 x 640 frames rendered by ``df_cad_render_mesh``, ellipsoid icospheres of 5 120 and 81 920 triangles and the bracket, device events
around one call, the median of 5 calls after one warm-up with the range.  Per mesh: the host time of the model build
(``df_ppf_model_build``, 400 samples), one ``df_pose_ppf`` call (every second node a scene point: 6 400 grid nodes a window, every fifth
of those per row and column a reference: 256 workgroups an item, top 4), the table entries the call visited (counted by the vote kernel
itself) and their rate, and in the same run one ``df_pose_refine_dense`` call of 10 steps on the same items from the best cluster's poses.
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
from densefusion_amd.lib.pose_ppf import PpfEstimator, PpfModels  # noqa: E402
from densefusion_amd.lib.pose_refine_dense import DensePoseRefiner  # noqa: E402
from pose_verify_bench import B, IH, IW, RADIUS, SCALE, WIN, icosphere, quat_to_matrix, summary, timed  # noqa: E402

ITERS, GATE, POINTS, STEP, REF_STEP, K = 10, 200, 400, 2, 5, 4


def bracket():
    """An L-shaped bracket (two boxes sharing a face, outward faces), sized like the ellipsoids: flat faces put long buckets in the table."""
    def box(lo, hi):
        c = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], dtype=np.float64)
        t = [[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]]
        return c, np.array(t, dtype=np.int32)
    (a, ta), (b, tb) = box((-1.0, -0.5, -0.6), (1.0, -0.1, 0.6)), box((-1.0, -0.1, -0.6), (-0.6, 0.9, 0.6))
    return (np.concatenate([a, b]) * RADIUS).astype(np.float32), np.concatenate([ta, tb + 8]).astype(np.int32)


def bench_mesh(name, v, t, calls, rng):
    proj = np.array(cad_render.DEFAULT_PROJ, dtype=np.float64)
    quat = rng.normal(size=(B, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    trans = np.stack([rng.uniform(-800, 800, B), rng.uniform(-300, 300, B), rng.uniform(-4400, -3800, B)], axis=1)
    poses = np.stack([np.concatenate([quat_to_matrix(q), tr[:, None]], axis=1) for q, tr in zip(quat, trans)])
    renderer = cad_render.CadMeshRenderer(v, t, np.full((len(v), 3), 128, dtype=np.uint8), proj, (IH, IW), model_scale=SCALE)
    _, depth, mask, _ = renderer.render(poses, cull=0, mask="pixels")
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    frame = torch.arange(B, dtype=torch.int32, device="cuda")
    obj = torch.zeros(B, dtype=torch.int32, device="cuda")
    cx = ((proj[0, 0] * trans[:, 0] + proj[0, 2] * trans[:, 2]) / -trans[:, 2] + 1.0) * IW * 0.5
    cy = (1.0 - (proj[1, 1] * trans[:, 1] + proj[1, 2] * trans[:, 2]) / -trans[:, 2]) * IH * 0.5
    corner = up(np.stack([np.rint(cy) - WIN // 2, np.rint(cx) - WIN // 2], axis=1), np.int32)
    udp = UnityDepthProjector.from_matrix(proj, (IH, IW))
    models = PpfModels([(v, t)], SCALE, 1.0, points=POINTS, seed=0)
    est = PpfEstimator(models, proj, (IH, IW), cloud_div=1.0).set_rays(udp.ray_map_on("cuda"))
    ref = DensePoseRefiner([(v, t)], SCALE, proj, (IH, IW), cloud_div=1.0).set_rays(udp.ray_map_on("cuda"))
    ppf = lambda: est.estimate(depth, frame, obj, corner, (WIN, WIN), step=STEP, gate=GATE, ref_step=REF_STEP, k=K, mask=mask)
    pose, votes, stats = ppf()
    torch.cuda.synchronize()
    need = est.scratch_bytes(B, (WIN, WIN), STEP, REF_STEP)
    visited = int(est._scratch[need - 8 * B:need].cpu().numpy().view(np.uint64).sum())
    start = pose[:, 0].contiguous()
    dense = lambda: ref.refine(depth, start, frame, obj, corner, (WIN, WIN), iters=ITERS, gate=GATE, cull=False)
    _, dstats = dense()
    st, dstats = stats.cpu().numpy(), dstats.cpu().numpy()
    p, d = summary(timed(ppf, calls)), summary(timed(dense, calls))
    lens = np.diff(models.bucket_begin, axis=1)
    return dict(mesh=name, triangles=len(t), model_points=POINTS, model_build_host_ms=1e3 * models.build_seconds, entries=models.n_entries,
                longest_bucket=int(lens.max()), buckets_in_use=int((lens > 0).sum()), ppf_call=p, entries_visited=visited,
                entries_per_second=visited / (p["median_ms"] * 1e-3), dense_iters10_call=d, ppf_over_dense10=p["median_ms"] / d["median_ms"],
                status_ok=int((st[:, 0] == 0).sum()), no_hypothesis=int((st[:, 0] == 1).sum()), mean_usable=float(st[:, 1].mean()),
                mean_hypotheses=float(st[:, 2].mean()), mean_clusters=float(st[:, 3].mean()), mean_best_score=float(votes[:, 0, 0].double().mean()),
                dense_status_ok=int((dstats[:, 0] == 0).sum()), dense_mean_rms_last=float(dstats[:, 4].mean()))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--levels", type=int, nargs="*", default=[4, 6], help="icosphere subdivisions: 4 = 5 120 triangles, 6 = 81 920")
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("pose_ppf_bench.py needs a GPU")
    rng = np.random.default_rng(0)
    meshes = []
    for level in opt.levels:
        v, t = icosphere(level)
        meshes.append(("icosphere(%d)" % level, (v * np.array([1.0, 0.7, 0.5]) * RADIUS).astype(np.float32), t))
    meshes.append(("bracket",) + bracket())
    out = dict(bench="pose_ppf", items=B, window=[WIN, WIN], frame=[IH, IW], calls=opt.calls, step=STEP, ref_step=REF_STEP, k=K, gate=GATE,
               grid_nodes=((WIN + STEP - 1) // STEP) ** 2, references=((((WIN + STEP - 1) // STEP) + REF_STEP - 1) // REF_STEP) ** 2,
               meshes=[bench_mesh(name, v, t, opt.calls, rng) for name, v, t in meshes])
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
