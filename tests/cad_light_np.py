"""The lit resolve restated in numpy: steps L1..L6 of ``df_cad_render_mesh_lit`` / ``df_cad_render_scene_lit`` (include/dfusion.h) over
the restatements of the unlit calls (tests/cad_raster_np.py, tests/cad_scene_np.py), which are imported and not edited: they give
geometry, depth, masks, labels, stats and the ``winner`` maps; this module recomputes the winners' weights from those maps by T5 and
writes the lit colour of every covered pixel.  TEST INFRASTRUCTURE: the specification the LIT instantiations of the resolve kernels are
held to, bit for bit.  Every sum is spelled out element-wise in the contract's order (no ``@``, no ``np.dot``)."""
import numpy as np

import cad_raster_np as mnp
import cad_scene_np as snp

IDENTITY = np.array([0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0])          # ambient 1, diffuse 0, white: multiplies by exactly 1.0


def rotate(R, n):
    """L2: n'_j = (R[j][0]*n_x + R[j][1]*n_y) + R[j][2]*n_z for n [..., 3] -> list of three arrays"""
    return [(R[j, 0] * n[..., 0] + R[j, 1] * n[..., 1]) + R[j, 2] * n[..., 2] for j in range(3)]


def lit_pixels(v, tri, colors, R, r, q, wt_idx, normals, normal_mode, rec):
    """The lit colour [n,3] uint8 of the covered pixels (r, q) [n] whose winners are the triangles ``wt_idx`` [n] of ``tri``; ``v`` is
    ``project_vertices`` under the winners' pose, whose rotation is ``R``; ``rec`` the frame's light record (8,)."""
    sx, sy = v["sx"], v["sy"]
    wt = tri[wt_idx]
    py, px = r.astype(np.float64), q.astype(np.float64)
    A = mnp.edge(wt[:, 0], wt[:, 1], sx, sy, sx[wt[:, 2]], sy[wt[:, 2]])
    w = [mnp.edge(wt[:, 1], wt[:, 2], sx, sy, px, py), mnp.edge(wt[:, 2], wt[:, 0], sx, sy, px, py), mnp.edge(wt[:, 0], wt[:, 1], sx, sy, px, py)]
    w = [np.where(A < 0, -x, x) for x in w]
    col = colors.astype(np.float64)
    rec = np.asarray(rec, dtype=np.float64)
    nrm = np.asarray(normals, dtype=np.float32).astype(np.float64)                          # L1
    out = np.zeros((len(r), 3), dtype=np.uint8)
    with np.errstate(all="ignore"):
        u = [w[k] / v["c3"][wt[:, k]] for k in range(3)]
        U = (u[0] + u[1]) + u[2]
        if normal_mode == 0:                                                                # L2
            N = rotate(R, nrm[wt_idx])
        else:
            n = [rotate(R, nrm[wt[:, k]]) for k in range(3)]
            N = [((u[0] * n[0][j] + u[1] * n[1][j]) + u[2] * n[2][j]) / U for j in range(3)]
        N = [np.where(A > 0, -x, x) for x in N]                                             # L3
        c = (N[0] * rec[0] + N[1] * rec[1]) + N[2] * rec[2]                                 # L4
        c = np.where(c > 0, c, 0.0)
        s = rec[3] + rec[4] * c                                                             # L5
        for ch in range(3):                                                                 # L6
            a = ((u[0] * col[wt[:, 0], ch] + u[1] * col[wt[:, 1], ch]) + u[2] * col[wt[:, 2], ch]) / U
            val = np.rint(a * (s * rec[5 + ch]))
            out[:, ch] = np.where(val >= 0, np.minimum(val, 255.0), 0.0).astype(np.uint8)   # a NaN gives 0
    return out


def render_mesh(vertices, colors, triangles, poses, model_scale, holes, proj, IH, IW, cull, mask_mode, normals, normal_mode, light):
    """``df_cad_render_mesh_lit``: (rgb, depth, mask, stats, winner) as ``cad_raster_np.render``; light [F,8] or None = unlit."""
    rgb, depth, mask, stats, winner = mnp.render(vertices, colors, triangles, poses, model_scale, holes, proj, IH, IW, cull, mask_mode)
    if light is None:
        return rgb, depth, mask, stats, winner
    rgb = rgb.copy()
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    for f in range(len(poses)):
        r, q = np.where(winner[f] >= 0)
        if len(r) == 0:
            continue
        T = np.asarray(poses[f], dtype=np.float64).reshape(3, 4)
        v = mnp.project_vertices(vertices, T, model_scale, None, None, proj, IH, IW)
        rgb[f, r, q] = lit_pixels(v, tri, colors, T[:, :3], r, q, winner[f, r, q], normals, normal_mode, light[f])
    return rgb, depth, mask, stats, winner


def render_scene(vertices, colors, triangles, tri_begin, model_scales, poses, present, proj, IH, IW, cull, normals, normal_mode, light):
    """``df_cad_render_scene_lit``: (rgb, depth, label, stats, winner, cover) as ``cad_scene_np.render``; light [F,8] or None = unlit."""
    out = snp.render(vertices, colors, triangles, tri_begin, model_scales, poses, present, proj, IH, IW, cull)
    if light is None:
        return out
    rgb, depth, label, stats, winner, cover = out
    rgb = rgb.copy()
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    for f in range(len(poses)):
        for o in range(len(tri_begin) - 1):
            r, q = np.where(label[f] == o + 1)
            if len(r) == 0:
                continue
            T = np.asarray(poses[f][o], dtype=np.float64).reshape(3, 4)
            v = mnp.project_vertices(vertices, T, model_scales[o], None, None, proj, IH, IW)
            rgb[f, r, q] = lit_pixels(v, tri, colors, T[:, :3], r, q, winner[f, r, q], normals, normal_mode, light[f])
    return rgb, depth, label, stats, winner, cover
