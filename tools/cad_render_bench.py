#!/usr/bin/env python
"""Device time per frame of ``df_cad_render`` (HIP events, the median of ``--calls`` calls after one warm-up) on a fabricated sphere
cloud, and with ``--cpu`` the time per frame of the numpy restatement (tests/cad_render_np.py) on this machine's CPU.  One JSON line.

    python tools/cad_render_bench.py --points 1000000 --height 520 --width 1109 --splat 1 --chunk 32 [--cpu]

``--mesh`` times ``df_cad_render_mesh`` instead, in one run and on the same poses (no holes): an icosphere of ``--subdiv`` subdivisions
(tests/cad_raster_np.py builds it; radius 60 file units), a 12-triangle box of the sphere's size, and for comparison the point path on
``--points`` points drawn from that icosphere by area with their faces' normals.

    python tools/cad_render_bench.py --mesh --subdiv 7 --points 1000000 --splat 1 --chunk 32

``--scene`` times ``df_cad_render_scene`` on one icosphere of ``--subdiv`` subdivisions (the target of ``render.sample_scene``), four
icospheres of subdivision 5 and the 12-triangle box, all present, next to the sum of the six ``df_cad_render_mesh`` calls that draw each
mesh alone at the same poses (without occlusion: what the single-object path costs for the same work).

    python tools/cad_render_bench.py --scene --subdiv 7 --chunk 32

``--light`` (with ``--mesh`` or ``--scene``) times the lit calls instead (``df_cad_render_mesh_lit`` / ``df_cad_render_scene_lit``) with
the light ``render.sample_light`` draws for each frame's seed and ``--shading flat|smooth`` normals; the point path stays unlit.

    python tools/cad_render_bench.py --scene --subdiv 7 --chunk 32 --light

``--sensor`` times ``df_cad_depth_sensor`` (record: sigma 4 codes, R 2, edge_step 64, edge_drop 0.5, drop 0.01, quant 1) on the depth of
``--chunk`` frames that ``df_cad_render_mesh`` renders from the icosphere of ``--subdiv`` subdivisions, next to that render call and to
a plain device copy of the same depth buffer (4 bytes of traffic per pixel: the floor), all in one run.

    python tools/cad_render_bench.py --sensor --subdiv 7 --chunk 32

``--visibility N`` draws the scenes of seeds 0..N-1 as tools/render_cad_dataset.py --scene does for the meshes of its test
(tests/cad_scene_np.py: two spheres as models, a box as distractor, 96 x 144 frames) and prints the histogram of the visible fractions
of the models that are present, in ten bins.

    python tools/cad_render_bench.py --visibility 256
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
from densefusion_amd.datasets.customCAD import render as cr  # noqa: E402

PROJ = [[1.16667, 0.0, 0.0, 0.0], [0.0, 2.48814, 0.0, 0.0], [0.0, 0.0, 0.5, 3000.0], [0.0, 0.0, -1.0, 0.0]]


def timed(render, calls):
    """(device ms of each call after one warm-up, the last call's outputs)"""
    times = []
    for k in range(calls + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = render()
        e1.record()
        torch.cuda.synchronize()
        if k:
            times.append(e0.elapsed_time(e1))
    return times, out


def lights_of(opt):
    """(normals argument of the renderers, light [chunk,8] or None)"""
    if not opt.light:
        return None, None
    return opt.shading, np.stack([cr.sample_light(s) for s in range(opt.chunk)])


def mesh_bench(opt):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cad_raster_np as mnp
    rng = np.random.default_rng(0)
    sv, sf = mnp.icosphere(opt.subdiv, 60.0)
    e = 60.0 / np.sqrt(3.0)                                   # the cube inscribed in the sphere
    bv = np.array([[x, y, z] for z in (-e, e) for y in (-e, e) for x in (-e, e)])
    bf = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]])
    poses = []
    for s in range(opt.chunk):
        axis, angle, xyz, _ = cr.sample_view(s, len(sv), (0.0, 0.0, 4.0), 1.0, hole_mean=30.0, hole_std=10.0)
        R, t = cr.view_pose(axis, angle, xyz, np.zeros(3), 10.0)
        poses.append(np.concatenate([R, t[:, None]], axis=1))
    poses = np.stack(poses)
    dims = (opt.height, opt.width)
    normals, light = lights_of(opt)
    res = {"frame": list(dims), "chunk": opt.chunk, "holes": 0, "light": bool(opt.light), "shading": opt.shading if opt.light else None}
    for name, v, f in (("icosphere", sv, sf), ("box", bv, bf)):
        r = cr.CadMeshRenderer(v, f, rng.integers(0, 256, (len(v), 3), dtype=np.uint8), PROJ, dims, normals=normals)
        times, out = timed(lambda: r.render(poses, cull=1, mask="box", light=light), opt.calls)
        stats = out[3].cpu().numpy()
        res[name] = {"triangles": int(len(f)), "device_ms_per_frame_median": float(np.median(times)) / opt.chunk,
                     "device_ms_per_call": [round(t, 3) for t in times], "covered_mean": float(stats[:, 0].mean()),
                     "triangles_reaching_mean": float(stats[:, 1].mean())}
    a, b, c = sv[sf[:, 0]], sv[sf[:, 1]], sv[sf[:, 2]]      # the point path on the same poses: points by area, each with its face's normal
    cross = np.cross(b - a, c - a)
    area = 0.5 * np.linalg.norm(cross, axis=1)
    t = rng.choice(len(sf), opt.points, p=area / area.sum())
    r1, r2 = np.sqrt(rng.random(opt.points))[:, None], rng.random(opt.points)[:, None]
    pts = (1.0 - r1) * a[t] + r1 * (1.0 - r2) * b[t] + r1 * r2 * c[t]
    nrm = cross[t] / (2.0 * area[t])[:, None]
    r = cr.CadRenderer(pts, nrm, rng.integers(0, 256, (opt.points, 3), dtype=np.uint8), PROJ, dims)
    times, out = timed(lambda: r.render(poses, splat=opt.splat, mask="box"), opt.calls)
    stats = out[3].cpu().numpy()
    res["points_of_icosphere"] = {"points": opt.points, "splat": opt.splat, "device_ms_per_frame_median": float(np.median(times)) / opt.chunk,
                                  "device_ms_per_call": [round(t, 3) for t in times], "covered_mean": float(stats[:, 0].mean()),
                                  "points_reaching_mean": float(stats[:, 1].mean())}
    print(json.dumps(res))
    return res


def sensor_bench(opt):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cad_raster_np as mnp
    rng = np.random.default_rng(0)
    sv, sf = mnp.icosphere(opt.subdiv, 60.0)
    poses = []
    for s in range(opt.chunk):
        axis, angle, xyz, _ = cr.sample_view(s, len(sv), (0.0, 0.0, 4.0), 1.0, hole_mean=30.0, hole_std=10.0)
        R, t = cr.view_pose(axis, angle, xyz, np.zeros(3), 10.0)
        poses.append(np.concatenate([R, t[:, None]], axis=1))
    poses = np.stack(poses)
    dims = (opt.height, opt.width)
    r = cr.CadMeshRenderer(sv, sf, rng.integers(0, 256, (len(sv), 3), dtype=np.uint8), PROJ, dims)
    render_ms, out = timed(lambda: r.render(poses, cull=1, mask="box"), opt.calls)
    depth = out[1]
    sensor = cr.DepthSensor(sigma_code=4.0, edge_radius=2, edge_step=64, edge_drop=0.5, drop=0.01, quant=1)
    from densefusion_amd.lib import preprocess as pp
    dst = torch.empty_like(depth)
    sensor_ms, (_, stats) = timed(lambda: pp.cad_depth_sensor(depth, sensor.record(), 0, 0, out=dst), opt.calls)
    copy_ms, _ = timed(lambda: dst.copy_(depth), opt.calls)
    med = lambda t: float(np.median(t))
    res = {"frame": list(dims), "chunk": opt.chunk, "triangles": int(len(sf)), "record": list(sensor.record()),
           "covered_mean": float(out[3].cpu().numpy()[:, 0].mean()), "sensor_counts_mean": [float(x) for x in stats.cpu().numpy().mean(axis=0)],
           "render_ms_per_call_median": med(render_ms), "sensor_ms_per_call_median": med(sensor_ms), "copy_ms_per_call_median": med(copy_ms),
           "render_ms_per_call": [round(t, 4) for t in render_ms], "sensor_ms_per_call": [round(t, 4) for t in sensor_ms],
           "copy_ms_per_call": [round(t, 4) for t in copy_ms], "sensor_over_render": med(sensor_ms) / med(render_ms),
           "sensor_over_copy": med(sensor_ms) / med(copy_ms)}
    print(json.dumps(res))
    return res


def scene_bench(opt):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cad_raster_np as mnp
    rng = np.random.default_rng(0)
    e = 60.0 / np.sqrt(3.0)                                   # the cube inscribed in the target's sphere
    bv = np.array([[x, y, z] for z in (-e, e) for y in (-e, e) for x in (-e, e)])
    bf = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]])
    shapes = [mnp.icosphere(opt.subdiv, 60.0)] + [mnp.icosphere(5, 40.0) for _ in range(4)] + [(bv, bf)]
    meshes = [(v, f, rng.integers(0, 256, (len(v), 3), dtype=np.uint8)) for v, f in shapes]
    O = len(meshes)
    poses = np.zeros((opt.chunk, O, 3, 4))
    for s in range(opt.chunk):
        views, _ = cr.sample_scene(s, len(meshes[0][0]), (0.0, 0.0, 4.0), 1.0, O, 0, hole_mean=30.0, hole_std=10.0, p_present=1.0)
        for o, (_, axis, angle, xyz) in enumerate(views):
            R, t = cr.view_pose(axis, angle, xyz, np.zeros(3), 10.0)
            poses[s, o] = np.concatenate([R, t[:, None]], axis=1)
    dims = (opt.height, opt.width)
    normals, light = lights_of(opt)
    scene = cr.CadSceneRenderer(meshes, PROJ, dims, [10.0] * O, normals=normals)
    times, out = timed(lambda: scene.render(poses, cull=1, light=light), opt.calls)
    stats = out[3].cpu().numpy()
    res = {"frame": list(dims), "chunk": opt.chunk, "objects": O, "triangles": [int(len(m[1])) for m in meshes],
           "light": bool(opt.light), "shading": opt.shading if opt.light else None,
           "scene": {"device_ms_per_frame_median": float(np.median(times)) / opt.chunk, "device_ms_per_call": [round(t, 3) for t in times],
                     "pixels_won_mean": [float(x) for x in stats[:, :, 0].mean(axis=0)],
                     "triangles_tested_mean": [float(x) for x in stats[:, :, 1].mean(axis=0)]},
           "solo": []}
    for o, (v, f, c) in enumerate(meshes):
        r = cr.CadMeshRenderer(v, f, c, PROJ, dims, normals=normals)
        times, out = timed(lambda: r.render(poses[:, o], cull=1, mask="box", light=light), opt.calls)
        res["solo"].append({"triangles": int(len(f)), "device_ms_per_frame_median": float(np.median(times)) / opt.chunk,
                            "covered_mean": float(out[3].cpu().numpy()[:, 0].mean())})
    res["solo_sum_device_ms_per_frame"] = float(sum(x["device_ms_per_frame_median"] for x in res["solo"]))
    print(json.dumps(res))
    return res


def visibility(opt):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cad_scene_np as snp
    meshes = snp.tool_meshes()
    O, n_targets, dims = len(meshes), 2, (96, 144)
    centroids = [m[0].astype(np.float64).mean(axis=0) for m in meshes]
    scene = cr.CadSceneRenderer(meshes, PROJ, dims, [10.0] * O)
    poses, present = np.zeros((opt.visibility, O, 3, 4)), np.zeros((opt.visibility, O), dtype=np.uint8)
    for s in range(opt.visibility):
        views, _ = cr.sample_scene(s, len(meshes[s % n_targets][0]), (0.0, 0.0, 4.0), 1.0, O, s % n_targets, hole_mean=30.0, hole_std=10.0)
        for o, (here, axis, angle, xyz) in enumerate(views):
            R, t = cr.view_pose(axis, angle, xyz, centroids[o], 10.0)
            poses[s, o], present[s, o] = np.concatenate([R, t[:, None]], axis=1), here
    won = scene.render(poses, present=present)[3].cpu().numpy()[:, :, 0]
    frac = []
    for k in range(n_targets):
        alone = np.zeros_like(present)
        alone[:, k] = present[:, k]
        solo = scene.render(poses, present=alone)[3].cpu().numpy()[:, k, 0]
        frac.extend((won[:, k][solo > 0] / solo[solo > 0]).tolist())
    hist = np.histogram(frac, bins=10, range=(0.0, 1.0))[0]
    res = {"seeds": opt.visibility, "frame": list(dims), "views": len(frac), "visible_fraction_histogram_10_bins": hist.tolist(),
           "wholly_visible": int(sum(1 for x in frac if x == 1.0)), "mean": float(np.mean(frac))}
    print(json.dumps(res))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", action="store_true", help="time df_cad_render_scene (six objects) next to the sum of the solo df_cad_render_mesh calls")
    ap.add_argument("--visibility", type=int, default=0, help="histogram of the visible fractions sample_scene gives over this many seeds")
    ap.add_argument("--mesh", action="store_true", help="time df_cad_render_mesh (icosphere, box) and the point path on points of that icosphere")
    ap.add_argument("--sensor", action="store_true", help="time df_cad_depth_sensor next to the mesh render it follows and to a device copy")
    ap.add_argument("--light", action="store_true", help="--mesh / --scene: time the lit calls, one sample_light record per frame")
    ap.add_argument("--shading", type=str, default="flat", choices=("flat", "smooth"), help="--light: one normal per triangle, or per vertex")
    ap.add_argument("--subdiv", type=int, default=7, help="--mesh: icosphere subdivisions (20 * 4^n triangles)")
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--height", type=int, default=520)
    ap.add_argument("--width", type=int, default=1109)
    ap.add_argument("--splat", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--cpu", action="store_true", help="also time the numpy restatement on one frame")
    opt = ap.parse_args(argv)
    if opt.light and not (opt.mesh or opt.scene):
        ap.error("--light needs --mesh or --scene: the point renderer is unlit")
    if opt.visibility:
        return visibility(opt)
    if opt.sensor:
        return sensor_bench(opt)
    if opt.scene:
        return scene_bench(opt)
    if opt.mesh:
        return mesh_bench(opt)
    rng = np.random.default_rng(0)
    d = rng.normal(size=(opt.points, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts, nrm, col = (d * 60.0).astype(np.float32), d.astype(np.float32), rng.integers(0, 256, (opt.points, 3), dtype=np.uint8)
    poses, holes = [], []
    for s in range(opt.chunk):
        axis, angle, xyz, hs = cr.sample_view(s, opt.points, (0.0, 0.0, 4.0), 1.0, hole_mean=30.0, hole_std=10.0)
        R, t = cr.view_pose(axis, angle, xyz, np.zeros(3), 10.0)
        poses.append(np.concatenate([R, t[:, None]], axis=1)); holes.append(hs)
    poses = np.stack(poses)
    renderer = cr.CadRenderer(pts, nrm, col, PROJ, (opt.height, opt.width))
    times = []
    for k in range(opt.calls + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = renderer.render(poses, holes=holes, splat=opt.splat, mask="box")
        e1.record()
        torch.cuda.synchronize()
        if k:
            times.append(e0.elapsed_time(e1))
    stats = out[3].cpu().numpy()
    res = {"points": opt.points, "frame": [opt.height, opt.width], "splat": opt.splat, "chunk": opt.chunk,
           "device_ms_per_frame_median": float(np.median(times)) / opt.chunk, "device_ms_per_call": [round(t, 3) for t in times],
           "covered_mean": float(stats[:, 0].mean()), "points_reaching_mean": float(stats[:, 1].mean())}
    if opt.cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import cad_render_np as rnp
        idx, rad = cr.CadRenderer.pack_holes(holes, opt.chunk) or (None, None)
        t0 = time.time()
        want = rnp.render_frame(pts, nrm, col, poses[0], 10.0, None if idx is None else idx[0], None if rad is None else rad[0], PROJ,
                                opt.height, opt.width, opt.splat, 0)
        res["numpy_ms_per_frame"] = (time.time() - t0) * 1e3
        res["frame0_equal"] = bool(all(np.array_equal(o[0].cpu().numpy(), w) for o, w in zip(out, want[:4])))
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
