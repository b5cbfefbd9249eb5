#!/usr/bin/env python
"""What point-to-mesh ICP costs on the device: one ``df_mesh_icp`` call (``lib.mesh_icp.MeshIcp.refine``) of B = 64 items x N = 500
points x 10 steps against ``icosphere(4)`` (5 120 triangles) and ``icosphere(6)`` (81 920), and in the same run ``df_mesh_closest`` on the
same number of point-triangle pairs (B N T (steps + 1), as K = B (steps + 1) transforms of N points).  One JSON line.

    python tools/mesh_icp_bench.py [--subdiv 4 6] [--items 64] [--points 500] [--iters 10] [--passes 5] [--accel [--tree_only 7] [--leaf 2 4 8]]

The icospheres are squashed to ellipsoids with axes 1 : 0.7 : 0.5: a sphere does not hold a rotation, its items would be `degenerate`
at the first step and the call would time one scan instead of eleven.  Each item's points are surface samples of the half that faces its
camera under a pose of its own; the start is 5 degrees and 0.05 diameters off.  A time is the median of ``--passes`` calls between two
device events after one warm-up call, with the smallest and largest next to it.  ``ok`` and ``mean_steps`` show that the items did run
their steps; ``scan_share`` is the time of the eleven scans alone (a call with 0 steps, times steps + 1) over the whole call.
``--accel`` times ``df_mesh_icp_tree`` (``MeshIcp(accel=True)``) on the same inputs right after the scan, the same way: ``tree`` holds its
times, the host time of the tree build (reported apart: it is paid once per mesh set), the speed-up over the scan of this run, and whether
poses and stats equal the scan's byte for byte.  ``--tree_only`` lists subdivisions where only the tree route runs (default 7: 327 680
triangles, where one scan call takes most of a second); ``--leaf`` also times trees of other leaf sizes than the library's.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from densefusion_amd.lib import mesh_distance as md  # noqa: E402
from densefusion_amd.lib.mesh_icp import MeshIcp  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdiv", type=int, nargs="+", default=[4, 6], help="subdivisions of the icospheres")
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--points", type=int, default=500)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--accel", action="store_true", help="also time the bounding-box tree route on the same inputs")
    ap.add_argument("--tree_only", type=int, nargs="*", default=[7], help="with --accel: subdivisions timed on the tree route alone")
    ap.add_argument("--leaf", type=int, nargs="*", default=[], help="with --accel: leaf sizes timed besides the library's")
    return ap


def spread(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def device_ms(fn, passes):
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


def time_scan(opt, v, f, points, start, obj, starts, D):
    """the scan route on one mesh: df_mesh_icp, and df_mesh_closest on the same pairs"""
    import mesh_icp_np as icp
    dev, (B, N), iters, T = points.device, points.shape[:2], opt.iters, len(f)
    fit = MeshIcp([(v, f)], 1.0, device=dev)
    icp_ms = spread(device_ms(lambda: fit.refine(points, start, obj, iters=iters), opt.passes))
    scan_ms = spread(device_ms(lambda: fit.refine(points, start, obj, iters=0), opt.passes))
    pose, stats = fit.refine(points, start, obj, iters=iters)
    stats = stats.cpu().numpy()
    # df_mesh_closest on the same pairs: K = B (iters + 1) transforms of one item's N points
    K = B * (iters + 1)
    xf = torch.from_numpy(np.stack([icp.model_frame([float(e) for e in starts[k % B]]).reshape(12) for k in range(K)])).to(dev)
    p64 = points[0].double().contiguous()
    scratch = torch.empty(md.scratch_bytes(T), dtype=torch.uint8, device=dev)
    closest_ms = spread(device_ms(lambda: md.mesh_closest(fit.vertices, fit.triangles, p64, xf, want_closest=True, scratch=scratch), opt.passes))
    pairs = B * N * T * (iters + 1)
    return {"_out": [pose.cpu().numpy(), stats], "mesh_icp_ms": icp_ms, "mesh_icp_0_steps_ms": scan_ms, "mesh_closest_ms": closest_ms,
            "icp_Gpairs_per_s": pairs / icp_ms["median"] / 1e6, "closest_Gpairs_per_s": pairs / closest_ms["median"] / 1e6,
            "icp_over_closest_rate": closest_ms["median"] / icp_ms["median"],
            "scan_share": scan_ms["median"] * (iters + 1) / icp_ms["median"],
            "ok": int((stats[:, 0] == 0).sum()), "mean_steps": float(stats[:, 5].mean()),
            "rms_over_D_first": float(stats[:, 2].mean() / D), "rms_over_D_last": float(stats[:, 4].mean() / D)}


def main(argv=None):
    opt = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_icp_bench needs a GPU (no CPU path)")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cad_raster_np as mnp
    import mesh_icp_np as icp
    dev = torch.device("cuda", torch.cuda.current_device())
    B, N, iters = opt.items, opt.points, opt.iters
    out = {"items": B, "points": N, "iters": iters, "passes": opt.passes, "cases": []}
    from densefusion_amd.lib.mesh_set import MeshTree
    for n in list(opt.subdiv) + ([k for k in opt.tree_only if k not in opt.subdiv] if opt.accel else []):
        scan = n in opt.subdiv
        v, f = mnp.icosphere(n, 0.06)
        v, f = (v * np.array([1.0, 0.7, 0.5])).astype(np.float32), np.asarray(f, dtype=np.int32)
        D, T = icp.diameter(v), len(f)
        rng = np.random.default_rng(n)
        clouds, starts = [], []
        for _ in range(B):
            truth = icp.random_pose(rng, 0.05) + np.array([0, 0, 0, 0, 0, 0, 0.6])
            centre = -np.array(icp.quat_to_mat([float(e) for e in truth[:4]])).T @ truth[4:]     # the camera in the model frame
            pts, _ = icp.surface_samples(v, f, 4 * N, rng, facing=centre)
            clouds.append(icp.apply_pose(truth, pts[:N]).astype(np.float32))
            starts.append(icp.perturb(truth, rng, math.radians(5), 0.05 * D))
        assert all(len(c) == N for c in clouds)
        points = torch.from_numpy(np.stack(clouds)).to(dev)
        start = torch.from_numpy(np.stack(starts)).to(dev)
        obj = torch.zeros(B, dtype=torch.int32, device=dev)
        case = {"subdiv": n, "triangles": T, "pairs": B * N * T * (iters + 1)}
        if scan:
            case.update(time_scan(opt, v, f, points, start, obj, starts, D))
        if opt.accel:
            tree = {}
            for leaf in [None] + list(opt.leaf):
                fast = MeshIcp([(v, f)], 1.0, device=dev, accel=True)
                if leaf is not None:
                    fast.tree = MeshTree(v, f, fast.tri_begin, leaf)
                ms = spread(device_ms(lambda: fast.refine(points, start, obj, iters=iters), opt.passes))
                ms0 = spread(device_ms(lambda: fast.refine(points, start, obj, iters=0), opt.passes))
                got = [x.cpu().numpy() for x in fast.refine(points, start, obj, iters=iters)]
                entry = {"leaf": fast.tree.leaf, "nodes": fast.tree.n_nodes, "loose": fast.tree.n_loose, "build_host_s": fast.tree.build_seconds,
                         "mesh_icp_tree_ms": ms, "mesh_icp_tree_0_steps_ms": ms0, "ok": int((got[1][:, 0] == 0).sum())}
                if scan:
                    entry["speedup"] = case["mesh_icp_ms"]["median"] / ms["median"]
                    entry["same_bytes"] = all(a.tobytes() == b.tobytes() for a, b in zip(got, case["_out"]))
                tree["default" if leaf is None else "leaf%d" % leaf] = entry
                del fast
            case["tree"] = tree
        case.pop("_out", None)
        out["cases"].append(case)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
