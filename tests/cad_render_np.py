"""The point-cloud renderer restated in numpy: the contract of ``df_cad_render`` (include/dfusion.h), i.e. the job of
datasets/customCAD/cad_to_dataset.py:137-243 (``augment_pointcloud``, ``project_pointcloud``) and mask_generator.py:20-28 of the reference
for the Unity-format frames datasets/customCAD/dataset.py reads.  TEST INFRASTRUCTURE: the specification
densefusion_amd/csrc/cad_render.hip is held to, bit for bit.

The reference's generator cannot be imported here (open3d and cv2 are absent, and it uses ``np.float`` / ``np.int``), so the renderer is
pinned by this restatement only.  Every sum is spelled out element-wise in the contract's order (no ``@``, no ``np.dot``: BLAS may fuse
or reorder).  Deliberate differences from the reference, as the contract states them: the facing test uses the point's own view ray
(:175-176 uses the direction to the centroid), depth and colour share one winner (:223-236 gives the colour to the farthest point), the
hole rule is a plain radius test (:153-162 asks open3d's KD-tree), the camera is the loader's projection matrix (:181-188 is a pinhole).
"""
import numpy as np

HORIZON = 65535
GRAY = 130


def render_frame(points, normals, colors, pose, model_scale, hole_idx, hole_r, proj, IH, IW, splat, mask_mode):
    """One frame: (rgb [IH,IW,3] u8, depth [IH,IW] u16, mask [IH,IW] u16, stats [6] int32, winner [IH,IW] int64 with -1 = uncovered)."""
    P_ = np.asarray(proj, dtype=np.float64)
    T = np.asarray(pose, dtype=np.float64).reshape(3, 4)
    m = points.astype(np.float64)                                                     # 1.
    idx = np.arange(len(m))
    keep = np.ones(len(m), dtype=bool)
    for h, r in zip(([] if hole_idx is None else hole_idx), ([] if hole_r is None else hole_r)):
        if h < 0:
            continue
        c = m[h]
        d2 = ((m[:, 0] - c[0]) * (m[:, 0] - c[0]) + (m[:, 1] - c[1]) * (m[:, 1] - c[1])) + (m[:, 2] - c[2]) * (m[:, 2] - c[2])
        keep &= ~(d2 <= np.float64(r) * np.float64(r))
    s = m * np.float64(model_scale)                                                   # 2.
    X = [((T[j, 0] * s[:, 0] + T[j, 1] * s[:, 1]) + T[j, 2] * s[:, 2]) + T[j, 3] for j in range(3)]
    if normals is not None:                                                           # 3.
        n = normals.astype(np.float64)
        nr = [(T[j, 0] * n[:, 0] + T[j, 1] * n[:, 1]) + T[j, 2] * n[:, 2] for j in range(3)]
        keep &= ((nr[0] * (-X[0]) + nr[1] * (-X[1])) + nr[2] * (-X[2])) > 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c = {j: ((P_[j, 0] * X[0] + P_[j, 1] * X[1]) + P_[j, 2] * X[2]) + P_[j, 3] for j in (0, 1, 3)}      # 4.
        keep &= c[3] > 0
        ndc_x, ndc_y = c[0] / c[3], c[1] / c[3]
        code = np.rint(65534.0 * ((1.0 + P_[2, 2]) + P_[2, 3] / X[2]))                # 5.
        keep &= (code >= 0) & (code <= 65534)
        colf = np.floor(((ndc_x + 1.0) * np.float64(IW)) * 0.5 + 0.5)                 # 6.
        rowf = np.floor(((1.0 - ndc_y) * np.float64(IH)) * 0.5 + 0.5)
        keep &= (colf >= -splat) & (colf <= IW - 1 + splat) & (rowf >= -splat) & (rowf <= IH - 1 + splat)
    idx, code = idx[keep], code[keep].astype(np.int64)
    col, row = colf[keep].astype(np.int64), rowf[keep].astype(np.int64)
    keys = np.full((IH, IW), np.iinfo(np.uint64).max, dtype=np.uint64)                # 7.
    key = (code.astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    for dr in range(-splat, splat + 1):
        for dc in range(-splat, splat + 1):
            r, q = row + dr, col + dc
            ok = (r >= 0) & (r < IH) & (q >= 0) & (q < IW)
            np.minimum.at(keys, (r[ok], q[ok]), key[ok])
    covered = keys != np.iinfo(np.uint64).max
    winner = np.where(covered, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    depth = np.where(covered, (keys >> np.uint64(32)).astype(np.int64), HORIZON).astype(np.uint16)
    rgb = np.full((IH, IW, 3), GRAY, dtype=np.uint8)
    rgb[covered] = colors[winner[covered]]
    stats = np.zeros(6, dtype=np.int32)
    mask = np.zeros((IH, IW), dtype=np.uint16)
    if covered.any():
        a = np.where(covered)
        stats[:] = [covered.sum(), len(idx), a[0].min(), a[0].max(), a[1].min(), a[1].max()]
        if mask_mode == 0:
            mask[stats[2]:stats[3], stats[4]:stats[5]] = 65535                        # mask_generator.py:28: half-open, as it is
    if mask_mode == 1:
        mask[covered] = 65535
    return rgb, depth, mask, stats, winner


def render(points, normals, colors, poses, model_scale, holes, proj, IH, IW, splat, mask_mode):
    """F frames, each on its own: rgb [F,IH,IW,3], depth, mask [F,IH,IW], stats [F,6], winner [F,IH,IW]."""
    out = [render_frame(points, normals, colors, poses[f], model_scale, None if holes is None else holes[0][f],
                        None if holes is None else holes[1][f], proj, IH, IW, splat, mask_mode) for f in range(len(poses))]
    return tuple(np.stack([o[k] for o in out]) for k in range(5))


# ---- fixtures the renderer tests share ---------------------------------------------------------------------------------------------
RADIUS = 60.0                       # file units; the loader's `model * 10` makes it 600
SPHERE_POS = np.array([0.3, -0.2, 4.0])


def sphere(n=20000, seed=3):
    """n points on a sphere of RADIUS with outward normals and random colours."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * RADIUS).astype(np.float32), d.astype(np.float32), rng.integers(0, 256, (n, 3), dtype=np.uint8)


def write_proj(path, proj):
    with open(path, "w") as f:
        f.write("".join("\t".join(repr(float(v)) for v in row) + "\n" for row in proj) + "\n")
    return str(path)


def camera_points(points, pose, model_scale=10.0):
    """Step 2 of the contract for chosen points, in its order."""
    s = points.astype(np.float64) * model_scale
    return np.stack([((pose[j, 0] * s[:, 0] + pose[j, 1] * s[:, 1]) + pose[j, 2] * s[:, 2]) + pose[j, 3] for j in range(3)], axis=1)


def grid_bounds(z, proj, IH, IW):
    """Half a step of the loader's ray grid in x and y and half a depth code in z, at depth z: exact in real arithmetic."""
    z = np.abs(z)
    return z / (IW * proj[0][0]), z / (IH * proj[1][1]), 0.5 * z * z / (proj[2][3] * 65534)
