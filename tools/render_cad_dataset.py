#!/usr/bin/env python
"""Render a customCAD training set from a coloured CAD cloud or mesh on the device -- no Unity, open3d or OpenCV.

    python tools/render_cad_dataset.py --model M.ply --output_root ROOT [--object 1 --frames 2000] [--raster mesh]

writes the tree ``tools/train.py --dataset cad`` and ``tools/eval_cad.py`` read (datasets/customCAD/dataset.py of the reference):
``ROOT/data/XX/{train,test}.txt``, ``rgb/FrameBuffer_NNNN.png``, ``depth/Depth_NNNN.png``, ``mask/NNNN.png``, ``meta/transforms.txt``,
``meta/proj_mat.txt`` and ``ROOT/models/obj_XX.ply``.  It does the jobs of the reference's cad_to_dataset.py (views drawn per seed, :264-276;
holes, :145-160; views with too few pixels skipped, :219-221), mask_generator.py (:21-28) and train_test_generator.py (:17-28).

Views are drawn seed by seed from ``--seed`` on (``render.sample_view``) and rendered ``--chunk`` at a time by ``df_cad_render``; a view
with fewer than ``--min_pixels`` covered pixels is skipped and the next seed is tried, accepted frames are numbered consecutively.  Every
pose is first written as its ``transforms.txt`` record (``repr`` precision) and parsed back, and the frame is rendered from the parsed
values: images and records agree exactly.  Record k + 1 holds frame k (the loader looks up ``index + 1``); record 0 repeats record 1.
Hole radii are in model file units (the reference's 0.03 / 0.01 apply to a model scaled by 0.001).

``--raster points`` (the default) samples a mesh into a cloud and splats it (``--points``, ``--splat``).  ``--raster mesh`` draws the
model's triangles themselves (``df_cad_render_mesh``: watertight, the depth exact on each facet, no splat radius): the model must have
faces, the hole indices of ``sample_view`` name vertices, ``--cull 1`` drops the triangles that face away, and ``models/obj_XX.ply``
receives the mesh (vertices and faces), which the loader samples by area.

    python tools/render_cad_dataset.py --scene --model A.ply B.ply ... [--distractor D.ply ...] --output_root ROOT [--min_visible 0.3]

renders frames that hold several meshes at once (``df_cad_render_scene``: one z-buffer, so objects cover each other) and writes one tree
per ``--model``: model k is object k + 1, ``data/%02d`` and ``models/obj_%02d.ply``.  Distractors are drawn and can occlude; they are
never targets and get no tree.  The view of seed s is ``render.sample_scene``: object s mod (number of models) is shown exactly where the
single-object tool shows it for that seed, the others are present with ``--p_present`` at a drawn offset from it (``--lateral``,
``--depth``).  Each chunk takes one scene call plus one call per model with only that model present, which gives its unoccluded pixel
count at the same poses: visible fraction = pixels won in the scene / pixels won alone.  A frame goes into a model's tree when the model
is present, won at least ``--min_pixels`` pixels and is visible to at least ``--min_visible``; its rgb and depth files are the shared
scene's, its mask, record and numbering its own.  No holes are cut in scenes.  ``--mask box`` marks the occluder's pixels inside the box
as the object -- the reference's own rule (mask_generator.py:21-28) -- so the loader's cloud then holds points of the occluder;
``--mask pixels`` marks only the pixels the object won and is the mode that keeps them out.

``--light head|random`` (with ``--raster mesh`` or ``--scene``) lights the frames (``df_cad_render_mesh_lit`` /
``df_cad_render_scene_lit``): ``head`` is ``render.HEAD_LIGHT`` in every frame, ``random`` draws ``render.sample_light(seed)`` within
``--light_angle`` degrees of the viewing direction; ``--shading flat|smooth`` takes one normal per triangle or per vertex.  A scene has
one light per shared frame for all its objects.  ``data/XX/meta/lights.txt`` then holds one line per written frame: the frame number and
the eight values of its record with ``repr``; as with the poses the frame is rendered from the parsed text.  The loader ignores the
file.  With ``--light none`` (the default) no such file is written and the trees are what they were without the flag.

``--sensor_sigma CODES`` (or ``--sensor_sigma_z S --sensor_z Z``: the code sigma that means range noise S at range Z, in the units of
``UnityDepthProjector.project_depth``), ``--sensor_edge R --sensor_edge_step STEP --sensor_edge_drop P``, ``--sensor_drop P`` and
``--sensor_quant Q`` put a depth-sensor model (``df_cad_depth_sensor``, ``render.DepthSensor``) over each chunk's depth after the render
and before the read-back, with any renderer and with ``--scene`` (once on the shared depth): disparity noise, pixels missing along depth
discontinuities and at random, quantisation.  Only the depth files change: colour, masks, records, ``--min_pixels`` and
``--min_visible`` are those of the clean render.  Frame j of a chunk draws from (``--sensor_seed``, the view's seed), so a frame's
noise does not depend on ``--chunk``.  ``data/XX/meta/sensor.txt`` holds the record (the sensor seed and the six integers of the call)
and one line per written frame: the frame number, its view's seed and the four counts {edge pixels, dropped at random, dropped at an
edge, kept with another code}.  The loader ignores the file; it paints the dropped pixels grey and leaves them out of ``choose``, as it
does with Unity's own horizon.  Without any of these flags nothing of this runs and no such file is written.
"""
from __future__ import annotations

import argparse
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from densefusion_amd.datasets.customCAD import render as cr  # noqa: E402
from densefusion_amd.datasets.customCAD.project_unity_depth import read_proj_mat  # noqa: E402

DEFAULT_PROJ = cr.DEFAULT_PROJ


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", type=str, nargs="+", required=True,
                    help="PLY with red / green / blue (and optionally nx / ny / nz) vertex properties; cloud or mesh.  Several only with --scene")
    ap.add_argument("--scene", action="store_true", help="render the models together, with occlusion: one tree per model from shared frames")
    ap.add_argument("--distractor", type=str, nargs="*", default=[], help="--scene: meshes that are drawn and can occlude, never targets")
    ap.add_argument("--output_root", type=str, required=True)
    ap.add_argument("--object", type=int, default=1, help="object directory data/XX and models/obj_XX.ply")
    ap.add_argument("--frames", type=int, default=2000)
    cr.add_view_arguments(ap)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--max_skipped", type=int, default=100000, help="give up after this many skipped views")
    return ap


record_text, parse_record, light_text, parse_light = cr.record_text, cr.parse_record, cr.light_text, cr.parse_light


def draw_light(opt, seed):
    """The light of seed ``seed`` as (text, record parsed back from it): rendered from the file's own values."""
    return cr.draw_light(opt.light, seed, opt.light_angle)


def write_lights(sub, texts):
    with open(os.path.join(sub, "meta", "lights.txt"), "w") as f:
        f.write("".join("%d %s\n" % (n, t) for n, t in enumerate(texts)))


def make_sensor(opt, ap, proj):
    """The ``DepthSensor`` of the --sensor_* flags, or None when none of them is given."""
    try:
        return cr.sensor_from_flags(proj, opt.sensor_sigma, opt.sensor_sigma_z, opt.sensor_z, opt.sensor_edge, opt.sensor_edge_step,
                                    opt.sensor_edge_drop, opt.sensor_drop, opt.sensor_quant)
    except ValueError as e:
        ap.error(str(e))


def write_sensor(sub, opt, sensor, rows):
    """meta/sensor.txt: the record, then per written frame its number, its view's seed and its four counts"""
    with open(os.path.join(sub, "meta", "sensor.txt"), "w") as f:
        f.write("sensor %d %s\n" % (opt.sensor_seed & 0xFFFFFFFF, " ".join("%d" % v for v in sensor.record())))
        f.write("".join("%d %d %s\n" % (n, view, " ".join("%d" % c for c in counts)) for n, (view, counts) in enumerate(rows)))


def write_vertex_ply(path, pts):
    pts = np.ascontiguousarray(pts, dtype="<f4").reshape(-1, 3)
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\ncomment rendered by densefusion_amd\nelement vertex %d\nproperty float x\n"
                 "property float y\nproperty float z\nend_header\n" % len(pts)).encode("ascii"))
        f.write(pts.tobytes())


def write_mesh_ply(path, vertices, triangles):
    vertices = np.ascontiguousarray(vertices, dtype="<f4").reshape(-1, 3)
    face = np.zeros(len(triangles), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    face["n"], face["v"] = 3, triangles
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\ncomment rendered by densefusion_amd\nelement vertex %d\nproperty float x\n"
                 "property float y\nproperty float z\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n"
                 % (len(vertices), len(face))).encode("ascii"))
        f.write(vertices.tobytes() + face.tobytes())


load_model = cr.load_cloud


def write_split(sub, written, seed):
    """train_test_generator.py:17-28: the shuffled frame numbers, 80 / 20"""
    nums = list(range(written))
    random.seed(seed)
    random.shuffle(nums)
    cut = int(len(nums) / 100. * 80)
    for name, part in (("train.txt", nums[:cut]), ("test.txt", nums[cut:])):
        with open(os.path.join(sub, name), "w") as f:
            f.write("".join("%d\n" % n for n in part))


def main_scene(opt, ap):
    """--scene: one tree per model from shared frames of all models and distractors."""
    if opt.splat != ap.get_default("splat") or opt.points != ap.get_default("points") or opt.raster != ap.get_default("raster"):
        ap.error("--scene draws the triangles of every model: --raster, --splat and --points do not apply")
    if not torch.cuda.is_available():
        raise SystemExit("render_cad_dataset needs a GPU (no CPU path)")
    n_targets = len(opt.model)
    meshes = []
    for path in list(opt.model) + list(opt.distractor):
        pts, tris, col = cr.read_colored_mesh(path)
        if len(tris) == 0:
            raise SystemExit(f"{path}: --scene needs models with faces")
        meshes.append((pts, tris, col))
    O = len(meshes)
    proj = read_proj_mat(opt.proj_mat) if opt.proj_mat else np.array(DEFAULT_PROJ)
    os.makedirs(os.path.join(opt.output_root, "models"), exist_ok=True)
    subs = [os.path.join(opt.output_root, "data", "%02d" % (k + 1)) for k in range(n_targets)]
    for k, sub in enumerate(subs):
        for d in ("rgb", "depth", "mask", "meta"):
            os.makedirs(os.path.join(sub, d), exist_ok=True)
        write_mesh_ply(os.path.join(opt.output_root, "models", "obj_%02d.ply" % (k + 1)), meshes[k][0], meshes[k][1])
        with open(os.path.join(sub, "meta", "proj_mat.txt"), "w") as f:
            f.write("".join("\t".join(repr(float(v)) for v in row) + "\n" for row in proj) + "\n")
    proj = read_proj_mat(os.path.join(subs[0], "meta", "proj_mat.txt"))      # what the loader will read
    lit = opt.light != "none"
    sensor = make_sensor(opt, ap, proj)
    renderer = cr.CadSceneRenderer(meshes, proj, (opt.height, opt.width), [opt.model_scale] * O, normals=opt.shading if lit else None)
    centroids = [m[0].astype(np.float64).mean(axis=0) for m in meshes]

    def save(sub, n, rgb, depth, mask):
        Image.fromarray(rgb).save(os.path.join(sub, "rgb", "FrameBuffer_%04d.png" % n))
        Image.fromarray(depth).save(os.path.join(sub, "depth", "Depth_%04d.png" % n))
        Image.fromarray(mask).save(os.path.join(sub, "mask", "%04d.png" % n))

    records = [[] for _ in range(n_targets)]
    visible = [[] for _ in range(n_targets)]
    seeds = [[] for _ in range(n_targets)]
    light_texts = [[] for _ in range(n_targets)]
    sensor_rows = [[] for _ in range(n_targets)]
    skipped, seed, device_ms = 0, opt.seed, []
    t_start = time.time()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        while any(len(r) < opt.frames for r in records):
            if skipped > opt.max_skipped:
                raise SystemExit(f"{skipped} views skipped for fewer than {opt.min_pixels} pixels or less than {opt.min_visible} visible: "
                                 "check --center, --scene_scale, --lateral, --depth and the camera")
            texts, poses, present = cr.draw_scene_records(range(seed, seed + opt.chunk), [len(m[0]) for m in meshes], centroids, n_targets,
                                                          opt.center, opt.scene_scale, opt.model_scale, opt.max_holes,
                                                          hole_mean=opt.hole_mean, hole_std=opt.hole_std, p_present=opt.p_present,
                                                          lateral=opt.lateral, depth=opt.depth)      # rendered from the records' own values
            lights = [draw_light(opt, s) for s in range(seed, seed + opt.chunk)] if lit else None
            seed += opt.chunk
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            rgb, depth, label, stats = renderer.render(poses, present=present, cull=opt.cull,
                                                       light=np.stack([l for _, l in lights]) if lit else None)
            ev1.record()
            if sensor is not None:                                            # once on the shared depth; masks and counts stay the clean render's
                depth, counts = cr.apply_sensor(depth, sensor, opt.sensor_seed, seed - opt.chunk)
                counts = counts.cpu().numpy()
            rows = stats.cpu().numpy()                                        # the chunk's read-backs before its frames
            device_ms.append(ev0.elapsed_time(ev1))
            solo = np.zeros((opt.chunk, n_targets), dtype=np.int64)
            for k in range(n_targets):                                        # the same poses with model k alone: its unoccluded pixels
                alone = np.zeros_like(present)
                alone[:, k] = present[:, k]
                solo[:, k] = renderer.render(poses, present=alone, cull=opt.cull)[3][:, k, 0].cpu().numpy()
            pairs = []
            for j in range(opt.chunk):
                for k in range(n_targets):
                    if len(records[k]) + sum(1 for p in pairs if p[1] == k) >= opt.frames or not present[j, k]:
                        continue
                    kept, frac = cr.scene_view_kept(rows[j, k, 0], solo[j, k], opt.min_pixels, opt.min_visible)
                    if not kept:
                        skipped += 1
                        continue
                    pairs.append((j, k, frac))
            if not pairs:
                continue
            mask = renderer.masks(label, stats, np.array([[j, k] for j, k, _ in pairs], dtype=np.int32), mask=opt.mask).cpu().numpy()
            rgb, depth = rgb.cpu().numpy(), depth.cpu().numpy()
            pending = []
            for n, (j, k, frac) in enumerate(pairs):
                pending.append(pool.submit(save, subs[k], len(records[k]), rgb[j], depth[j], mask[n]))
                records[k].append(parse_record(texts[j][k]))
                visible[k].append(float(frac)); seeds[k].append(seed - opt.chunk + j)
                if lit:
                    light_texts[k].append(lights[j][0])
                if sensor is not None:
                    sensor_rows[k].append((seed - opt.chunk + j, counts[j]))
            for p in pending:
                p.result()
    for k, sub in enumerate(subs):
        with open(os.path.join(sub, "meta", "transforms.txt"), "w") as f:
            for idx, (pos, quat) in enumerate([records[k][0]] + records[k]):
                f.write(record_text(idx, pos, quat))
        write_split(sub, len(records[k]), opt.seed)
        if lit:
            write_lights(sub, light_texts[k])
        if sensor is not None:
            write_sensor(sub, opt, sensor, sensor_rows[k])
    wall = time.time() - t_start
    per_view = float(np.median(device_ms)) / opt.chunk
    summary = {"objects": {}, "skipped": skipped, "device_ms_per_view": per_view}
    for k in range(n_targets):
        summary["objects"][k + 1] = {"written": len(records[k]), "mean_visible": float(np.mean(visible[k])), "visible": visible[k],
                                     "seeds": seeds[k]}
        print(f"object {k + 1}: frames written: {len(records[k])}, mean visible fraction: {np.mean(visible[k]):.3f}")
    print(f"views skipped: {skipped}, device time per rendered scene: {per_view:.3f} ms (HIP events, the median of {len(device_ms)} calls; "
          f"{O} objects, {int(renderer.tri_begin[-1])} triangles, {opt.height} x {opt.width}, cull {opt.cull}, chunk {opt.chunk}); "
          f"wall {wall / max(sum(len(r) for r in records), 1) * 1e3:.1f} ms per frame written")
    return summary


def main(argv=None):
    ap = build_parser()
    opt = ap.parse_args(argv)
    if opt.scene:
        return main_scene(opt, ap)
    if len(opt.model) != 1 or opt.distractor:
        ap.error("several --model paths and --distractor need --scene; without it exactly one model is rendered")
    opt.model = opt.model[0]
    mesh = opt.raster == "mesh"
    if mesh and (opt.splat != ap.get_default("splat") or opt.points != ap.get_default("points")):
        ap.error("--splat and --points belong to --raster points; --raster mesh draws the triangles themselves")
    lit = opt.light != "none"
    if lit and not mesh:
        ap.error("--light needs --raster mesh or --scene: the point renderer is unlit")
    if not torch.cuda.is_available():
        raise SystemExit("render_cad_dataset needs a GPU (no CPU path)")
    np.random.seed(opt.seed)
    if mesh:
        pts, tris, col = cr.read_colored_mesh(opt.model)
        if len(tris) == 0:
            raise SystemExit(f"{opt.model}: --raster mesh needs a model with faces")
    else:
        pts, nrm, col = load_model(opt.model, opt.points)
    proj = read_proj_mat(opt.proj_mat) if opt.proj_mat else np.array(DEFAULT_PROJ)
    sub = os.path.join(opt.output_root, "data", "%02d" % opt.object)
    for d in ("rgb", "depth", "mask", "meta"):
        os.makedirs(os.path.join(sub, d), exist_ok=True)
    os.makedirs(os.path.join(opt.output_root, "models"), exist_ok=True)
    if mesh:
        write_mesh_ply(os.path.join(opt.output_root, "models", "obj_%02d.ply" % opt.object), pts, tris)
    else:
        write_vertex_ply(os.path.join(opt.output_root, "models", "obj_%02d.ply" % opt.object), pts)
    with open(os.path.join(sub, "meta", "proj_mat.txt"), "w") as f:
        f.write("".join("\t".join(repr(float(v)) for v in row) + "\n" for row in proj) + "\n")
    proj = read_proj_mat(os.path.join(sub, "meta", "proj_mat.txt"))          # what the loader will read
    sensor = make_sensor(opt, ap, proj)
    if mesh:
        renderer = cr.CadMeshRenderer(pts, tris, col, proj, (opt.height, opt.width), model_scale=opt.model_scale,
                                      normals=opt.shading if lit else None)
    else:
        renderer = cr.CadRenderer(pts, nrm, col, proj, (opt.height, opt.width), model_scale=opt.model_scale)
    centroid = pts.astype(np.float64).mean(axis=0)

    def save(n, rgb, depth, mask):
        Image.fromarray(rgb).save(os.path.join(sub, "rgb", "FrameBuffer_%04d.png" % n))
        Image.fromarray(depth).save(os.path.join(sub, "depth", "Depth_%04d.png" % n))
        Image.fromarray(mask).save(os.path.join(sub, "mask", "%04d.png" % n))

    records, light_texts, sensor_rows, written, skipped, seed, device_ms = [], [], [], 0, 0, opt.seed, []
    t_start = time.time()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        pending = []
        while written < opt.frames:
            if skipped > opt.max_skipped:
                raise SystemExit(f"{skipped} views skipped for fewer than {opt.min_pixels} pixels: check --center, --scene_scale and the camera")
            texts, poses, holes = cr.draw_view_records(range(seed, seed + opt.chunk), len(pts), centroid, opt.center, opt.scene_scale,
                                                       opt.model_scale, opt.max_holes, hole_mean=opt.hole_mean,
                                                       hole_std=opt.hole_std)          # rendered from the records' own values
            lights = [draw_light(opt, s) for s in range(seed, seed + opt.chunk)] if lit else None
            seed += opt.chunk
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            if mesh:
                rgb, depth, mask, stats = renderer.render(poses, holes=holes, cull=opt.cull, mask=opt.mask,
                                                          light=np.stack([l for _, l in lights]) if lit else None)
            else:
                rgb, depth, mask, stats = renderer.render(poses, holes=holes, splat=opt.splat, mask=opt.mask)
            ev1.record()
            if sensor is not None:                                            # the mask and the counts stay the clean render's
                depth, counts = cr.apply_sensor(depth, sensor, opt.sensor_seed, seed - opt.chunk)
                counts = counts.cpu().numpy()
            rows = stats.cpu().numpy()                                        # the chunk's one read-back before its frames
            device_ms.append(ev0.elapsed_time(ev1))
            rgb, depth, mask = rgb.cpu().numpy(), depth.cpu().numpy(), mask.cpu().numpy()
            for k in range(opt.chunk):
                if written == opt.frames:
                    break
                if not cr.view_kept(rows[k, 0], opt.min_pixels):
                    skipped += 1
                    continue
                pos, quat = parse_record(texts[k])
                records.append((pos, quat))
                if lit:
                    light_texts.append(lights[k][0])
                if sensor is not None:
                    sensor_rows.append((seed - opt.chunk + k, counts[k]))
                pending.append(pool.submit(save, written, rgb[k], depth[k], mask[k]))
                written += 1
            for p in pending:
                p.result()
            pending = []
    with open(os.path.join(sub, "meta", "transforms.txt"), "w") as f:
        for idx, (pos, quat) in enumerate([records[0]] + records):
            f.write(record_text(idx, pos, quat))
    write_split(sub, written, opt.seed)
    if lit:
        write_lights(sub, light_texts)
    if sensor is not None:
        write_sensor(sub, opt, sensor, sensor_rows)
    wall = time.time() - t_start
    per_view = float(np.median(device_ms)) / opt.chunk            # the median call: the first one also loads the kernels
    what = (f"{len(tris)} triangles", f"cull {opt.cull}") if mesh else (f"{len(pts)} points", f"splat {opt.splat}")
    print(f"frames written: {written}, views skipped: {skipped}, device time per rendered view: {per_view:.3f} ms "
          f"(HIP events, the median of {len(device_ms)} calls; {what[0]}, {opt.height} x {opt.width}, {what[1]}, chunk {opt.chunk}); "
          f"wall {wall / max(written, 1) * 1e3:.1f} ms per frame written")
    return {"written": written, "skipped": skipped, "device_ms_per_view": per_view}


if __name__ == "__main__":
    main()
