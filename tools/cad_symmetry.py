#!/usr/bin/env python
"""Report which proper rotations map each CAD model onto itself (datasets/customCAD/symmetry.py).

    python tools/cad_symmetry.py --model washer.ply bracket.ply [--tol 0.01] [--no_color] [--accel] [--write TREE]

Per model: whether it is symmetric (its views are then trained and scored with ADD-S: ``--cad_sym auto`` of tools/train.py and
tools/eval_cad_render.py runs the same detection), the axes and orders that passed and their residuals as fractions of the bounding-box
diagonal, and the size of its symmetry set (``symmetry_set``: the closure of what passed, a surface of revolution discretised to
ceil(pi / ``--step``) rotations, which the line then says; the BOP pose errors of lib/pose_error.py take their minimum over it).
``--write TREE`` also puts model k's report into ``TREE/data/<k + 1>/meta/symmetry.txt`` of a tree tools/render_cad_dataset.py wrote;
the disk loader does not read it.  ``main`` returns the reports.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from densefusion_amd.datasets.customCAD import render as cad_render  # noqa: E402
from densefusion_amd.datasets.customCAD.symmetry import detect_symmetry, is_revolution, symmetry_set  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", type=str, nargs="+", required=True, help="PLY mesh(es)")
    ap.add_argument("--tol", type=float, default=0.01, help="largest residual of a symmetry, as a fraction of the bounding-box diagonal")
    ap.add_argument("--color_tol", type=float, default=8.0, help="largest mean colour difference of a symmetry, in 8-bit levels")
    ap.add_argument("--no_color", action="store_true", help="geometry only")
    ap.add_argument("--max_order", type=int, default=12)
    ap.add_argument("--axes", type=int, default=10, help="face-normal directions tried besides the three principal axes")
    ap.add_argument("--samples", type=int, default=2048, help="surface samples")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--accel", action="store_true", help="find the distances through the model's bounding-box tree (the same report, faster on large meshes)")
    ap.add_argument("--step", type=float, default=0.01, help="a surface of revolution is discretised to ceil(pi / step) rotations in the symmetry set (BOP: 0.01)")
    ap.add_argument("--write", type=str, default="", metavar="TREE", help="also write data/XX/meta/symmetry.txt of this tree")
    return ap


def main(argv=None):
    opt = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("cad_symmetry.py needs a GPU (densefusion_amd has no CPU path)")
    reports = []
    for k, path in enumerate(opt.model):
        vertices, triangles, colors = cad_render.read_colored_mesh(path)
        if len(triangles) == 0:
            raise SystemExit(f"{path}: no faces; symmetry is decided from the triangles")
        try:
            report = detect_symmetry(vertices, triangles, None if opt.no_color else colors, tol=opt.tol, color_tol=opt.color_tol,
                                     max_order=opt.max_order, axes=opt.axes, samples=opt.samples, seed=opt.seed, accel=opt.accel)
        except ValueError as e:
            raise SystemExit(f"{path}: {e}")
        text = "model %d (object %d): %s\n%s" % (k, k + 1, path, report)
        try:                                                         # the rotations the BOP pose errors take their minimum over
            text += "\nsymmetry set: %d rotations%s" % (len(symmetry_set(report, step=opt.step, name=path)),
                                                       " (taken as a surface of revolution)" if is_revolution(report) else "")
        except ValueError as e:
            text += "\nsymmetry set: none (%s)" % e
        print(text)
        if opt.write:
            meta = os.path.join(opt.write, "data", "%02d" % (k + 1), "meta")
            os.makedirs(meta, exist_ok=True)
            with open(os.path.join(meta, "symmetry.txt"), "w") as f:
                f.write(text + "\n")
        reports.append(report)
    return reports


if __name__ == "__main__":
    main()
