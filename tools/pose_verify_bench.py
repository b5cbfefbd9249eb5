"""Time ``df_pose_verify`` (lib.pose_verify.PoseVerifier.score_items: the bare call) against what it is built beside: B = 64 items with 160 x 160 windows on
480 x 640 frames, ellipsoid icospheres of 5 120 and 81 920 triangles, device events around one call, the median of 5 calls after one
warm-up with the range.  In the same run: ``df_cad_render_mesh`` on the same meshes and poses at F = 64 whole frames, and a plain device
copy of the bytes the score pass reads (8-byte key, 2-byte depth code and 2-byte mask value per window node).

The passes of a call are told apart by calls, not by a profiler: a second verifier whose object 1 is an empty triangle range runs the
clears and the score pass and a raster launch whose workgroups return at once, so ``raster_ms`` = whole call - that call.  The renderer's
figure is its whole call (clear, raster, resolve, finish), so its triangles/s is a lower bound of its raster pass's.
``fill_of_keys_and_stats`` is torch's fill of as many key and tally bytes as the call clears, for scale.  One JSON line."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from densefusion_amd.datasets.customCAD import render as cad_render  # noqa: E402
from densefusion_amd.lib.pose_verify import PoseVerifier, STATS  # noqa: E402

IH, IW, B, WIN = 480, 640, 64, 160
RADIUS, SCALE = 75.0, 10.0


def icosphere(n):
    """(vertices float64 [V,3] on the unit sphere, triangles int32 [20 * 4^n, 3]), counter-clockwise seen from outside"""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    v = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g], [g, 0, -1], [g, 0, 1],
                  [-g, 0, -1], [-g, 0, 1]], dtype=np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], dtype=np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(n):
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        uniq, inv = np.unique(e, axis=0, return_inverse=True)
        mid = v[uniq[:, 0]] + v[uniq[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        k = len(v) + inv.reshape(3, -1)
        v = np.concatenate([v, mid])
        f = np.concatenate([np.stack([f[:, 0], k[0], k[2]], axis=1), np.stack([f[:, 1], k[1], k[0]], axis=1),
                            np.stack([f[:, 2], k[2], k[1]], axis=1), np.stack([k[0], k[1], k[2]], axis=1)])
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    flip = (np.cross(b - a, c - a) * a).sum(axis=1) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return v, f.astype(np.int32)


def quat_to_matrix(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def timed(fn, calls):
    """ms of each of ``calls`` calls of fn after one warm-up, device events around the call"""
    fn()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def summary(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def bench_mesh(level, calls, rng):
    v, t = icosphere(level)
    v = (v * np.array([1.0, 0.7, 0.5]) * RADIUS).astype(np.float32)
    proj = np.array(cad_render.DEFAULT_PROJ, dtype=np.float64)
    quat = rng.normal(size=(B, 4))
    trans = np.stack([rng.uniform(-800, 800, B), rng.uniform(-300, 300, B), rng.uniform(-4400, -3800, B)], axis=1)
    poses = np.stack([np.concatenate([quat_to_matrix(q), tr[:, None]], axis=1) for q, tr in zip(quat, trans)])
    renderer = cad_render.CadMeshRenderer(v, t, np.full((len(v), 3), 128, dtype=np.uint8), proj, (IH, IW), model_scale=SCALE)
    render = lambda: renderer.render(poses, cull=1, mask="pixels")
    _, depth, mask, rstats = render()
    ver = PoseVerifier([(v, t)], SCALE, proj, (IH, IW), cloud_div=1.0)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    pose = up(np.concatenate([quat, trans], axis=1), np.float64)
    frame = torch.arange(B, dtype=torch.int32, device="cuda")
    # the window is centred on the projection of the object's origin
    cx = ((proj[0, 0] * trans[:, 0] + proj[0, 2] * trans[:, 2]) / -trans[:, 2] + 1.0) * IW * 0.5
    cy = (1.0 - (proj[1, 1] * trans[:, 1] + proj[1, 2] * trans[:, 2]) / -trans[:, 2]) * IH * 0.5
    corner = up(np.stack([np.rint(cy) - WIN // 2, np.rint(cx) - WIN // 2], axis=1), np.int32)
    obj0, obj1 = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.ones(B, dtype=torch.int32, device="cuda")
    record = lambda obj: torch.cat([frame[:, None], obj[:, None], corner, frame[:, None], torch.full_like(frame, 65535)[:, None]], dim=1).contiguous()
    items0, items1 = record(obj0), record(obj1)
    score = lambda: ver.score_items(depth, pose, items0, (WIN, WIN), 0, mask=mask, cull=True)
    stats = score().cpu().numpy()
    assert np.array_equal(stats, ver.score(depth, pose, frame, obj0, corner, (WIN, WIN), 0, mask=mask, cull=True).cpu().numpy())
    # the same call on an empty triangle range: the clears and the score pass, no triangle
    ver2 = _with_empty_range(ver)
    score_only = lambda: ver2.score_items(depth, pose, items1, (WIN, WIN), 0, mask=mask, cull=True)
    nbytes = B * WIN * WIN * 12
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    keys, tallies = torch.empty(B * WIN * WIN, dtype=torch.int64, device="cuda"), torch.empty(B, len(STATS), dtype=torch.int64, device="cuda")
    whole, only, rend, copy, clears = (summary(timed(f, calls)) for f in (score, score_only, render, lambda: dst.copy_(src),
                                                                          lambda: (keys.fill_(-1), tallies.zero_())))
    raster_ms = max(whole["median_ms"] - only["median_ms"], 1e-6)
    T = len(t)
    tot = dict(zip(STATS, stats.sum(axis=0).tolist()))
    return dict(triangles=T, verify_call=whole, verify_empty_range_call=only, render_mesh_call=rend, copy_of_score_bytes=copy,
                fill_of_keys_and_stats=clears, score_bytes=nbytes, raster_ms=raster_ms, verify_raster_mtri_per_s=B * T / raster_ms / 1e3,
                render_mesh_call_mtri_per_s=B * T / rend["median_ms"] / 1e3, score_over_copy=only["median_ms"] / copy["median_ms"],
                rendered=tot["rendered"], agree=tot["agree"], renderer_pixels=int(rstats[:, 0].sum().item()), cut_triangles=tot["cut_triangles"])


def _with_empty_range(ver):
    """``ver`` with a second object that owns no triangle"""
    import copy
    other = copy.copy(ver)
    other.tri_begin = np.array([ver.tri_begin[0], ver.tri_begin[1], ver.tri_begin[1]], dtype=np.int32)
    other.model_scales = np.array([ver.model_scales[0], ver.model_scales[0]], dtype=np.float64)
    other.n_objects, other._scratch = 2, None
    return other


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--levels", type=int, nargs="+", default=[4, 6], help="icosphere subdivisions: 4 = 5 120 triangles, 6 = 81 920")
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("pose_verify_bench.py needs a GPU")
    rng = np.random.default_rng(0)
    out = dict(bench="pose_verify", items=B, window=[WIN, WIN], frame=[IH, IW], calls=opt.calls,
               meshes=[bench_mesh(level, opt.calls, rng) for level in opt.levels])
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
