"""A small customCAD dataset tree for the loader tests (the layout of datasets/customCAD/dataset.py:37-76,99 of the reference): two object
directories of 20 frames of 48 x 72 each, 16-bit depth and mask PNGs written through PIL, a perspective matrix with off-centre terms per
directory, vertex-only PLYs of 3200 points (ASCII for object 1, binary little-endian for object 2), 20 lines in every ``test.txt`` --
'test' mode keeps lines 10 and 20, i.e. frames 9 and 19.

Cases fixed by construction, CASES[(object, frame)]:
  edge     the mask touches row 0 and the last column (and holds fewer than 500 valid pixels)
  big      more than 500 valid mask pixels; the depth maximum also occurs inside the box, off the mask (grey fill in the crop)
  thin     a mask of 5 rows: a 4-row crop, the sentinel
  allmax   every masked pixel sits at the frame's depth maximum: count 0, the sentinel
  small    fewer than 500 valid mask pixels
  partmax  some masked pixels at the depth maximum (dropped from the mask), in a frame whose maximum fills the whole upper half
Every frame's maximum depth ("the horizon") occurs in many pixels and differs from frame to frame.
"""
import os

import numpy as np
from PIL import Image

IH, IW = 48, 72
FRAMES = 20
OBJECTS = (1, 2)
CASES = {(1, 0): "edge", (1, 9): "big", (1, 19): "thin", (1, 3): "allmax", (1, 5): "partmax", (1, 7): "small",
         (2, 9): "small", (2, 19): "allmax", (2, 2): "edge", (2, 4): "big"}
PROJ = {1: [[1.16667, 0.0, 0.07500, 0.0], [0.0, 2.48814, -0.04000, 0.0], [0.0, 0.0, 0.50000, 3000.0], [0.0, 0.0, -1.0, 0.0]],
        2: [[1.30000, 0.0, -0.05000, 0.0], [0.0, 2.10000, 0.06250, 0.0], [0.0, 0.0, 0.25000, 2000.0], [0.0, 0.0, -1.0, 0.0]]}


def _box(kind, rng):
    """inclusive (r0, r1, c0, c1) of the mask rectangle"""
    if kind == "edge":
        return 0, 20, 50, IW - 1
    if kind == "big":
        return 4, 44, 8, 66
    if kind == "thin":
        return 10, 14, 20, 50
    if kind == "small":
        return 15, 26, 30, 44
    r0, c0 = int(rng.integers(0, 20)), int(rng.integers(0, 30))
    return r0, r0 + int(rng.integers(10, 25)), c0, c0 + int(rng.integers(10, 40))


def make_frame(kind, rng, far):
    """(rgba uint8 [IH,IW,4], depth uint16, mask uint16) of one frame; `far`: the frame's depth maximum."""
    rgba = rng.integers(0, 256, (IH, IW, 4), dtype=np.uint8)
    depth = np.empty((IH, IW), dtype=np.uint16)
    depth[:IH // 2] = far                                                  # the horizon: the maximum, in many pixels
    depth[IH // 2:] = rng.integers(30000, 50000, (IH - IH // 2, IW))       # the ground
    r0, r1, c0, c1 = _box(kind, rng)
    mask = np.zeros((IH, IW), dtype=np.uint16)
    rr, cc = np.mgrid[0:IH, 0:IW]
    inside = (rr >= r0) & (rr <= r1) & (cc >= c0) & (cc <= c1)
    if kind not in ("edge", "thin", "small"):                              # an ellipse inside the box, touching its four sides
        cr, cq, ar, ac = (r0 + r1) / 2, (c0 + c1) / 2, (r1 - r0) / 2 + 1e-9, (c1 - c0) / 2 + 1e-9
        inside &= ((rr - cr) / ar) ** 2 + ((cc - cq) / ac) ** 2 <= 1.0
    mask[inside] = 65535
    mask[rng.random((IH, IW)) < 0.01] = 1000                               # stray labels of another value: not the object
    mask[inside] = 65535
    depth[inside] = rng.integers(8000, 25000, int(inside.sum()))
    if kind == "allmax":
        depth[inside] = far
    elif kind == "partmax":
        depth[inside & (rng.random((IH, IW)) < 0.3)] = far
    return rgba, depth, mask


def _write_ply(path, pts, binary):
    with open(path, "wb") as f:
        f.write(("ply\nformat %s 1.0\ncomment fabricated\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
                 % ("binary_little_endian" if binary else "ascii", len(pts))).encode("ascii"))
        if binary:
            f.write(pts.astype("<f4").tobytes())
        else:
            f.write("".join("%.6f %.6f %.6f\n" % tuple(p) for p in pts).encode("ascii"))


def make_cad_tree(root, seed=0):
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "models"), exist_ok=True)
    for obj in OBJECTS:
        sub = os.path.join(root, "data", "%02d" % obj)
        for d in ("rgb", "depth", "mask", "meta"):
            os.makedirs(os.path.join(sub, d), exist_ok=True)
        for n in range(FRAMES):
            rgba, depth, mask = make_frame(CASES.get((obj, n), "random"), rng, far=65535 - 100 * n - obj)
            Image.fromarray(rgba if obj == 1 else rgba[:, :, :3]).save(os.path.join(sub, "rgb", "FrameBuffer_%04d.png" % n))
            Image.fromarray(depth).save(os.path.join(sub, "depth", "Depth_%04d.png" % n))
            Image.fromarray(mask).save(os.path.join(sub, "mask", "%04d.png" % n))
        for name in ("train.txt", "test.txt"):
            with open(os.path.join(sub, name), "w") as f:
                f.write("".join("%d\n" % n for n in range(FRAMES)))
        with open(os.path.join(sub, "meta", "transforms.txt"), "w") as f:        # the generator's format: index, (pos), (quaternion)
            for idx in range(FRAMES + 1):
                pos = rng.uniform(-1.0, 1.0, 3) + np.array([0.0, 0.0, 4.0])
                q = rng.normal(size=4)
                q /= np.linalg.norm(q)
                f.write("%d\n(%.1f, %.1f, %.1f)\n(%.1f, %.1f, %.1f, %.1f)\n" % ((idx,) + tuple(pos) + tuple(q + 0.05)))
        with open(os.path.join(sub, "meta", "proj_mat.txt"), "w") as f:
            f.write("".join("\t".join("%.5f" % v for v in row) + "\n" for row in PROJ[obj]) + "\n")
        _write_ply(os.path.join(root, "models", "obj_%02d.ply" % obj), rng.uniform(-30.0, 30.0, (3200, 3)), binary=obj == 2)
    return root
