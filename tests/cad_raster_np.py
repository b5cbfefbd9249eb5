"""The triangle rasteriser restated in numpy: the contract of ``df_cad_render_mesh`` (include/dfusion.h), steps V1..V5, T1..T7 and the
resolve, vectorised over each triangle's node range.  TEST INFRASTRUCTURE: the specification densefusion_amd/csrc/cad_raster.hip is held
to, bit for bit.  Every sum is spelled out element-wise in the contract's order (no ``@``, no ``np.dot``: BLAS may fuse or reorder).
Also the fixtures the rasteriser tests share: an icosphere and a PLY writer for coloured meshes."""
import numpy as np

HORIZON = 65535
GRAY = 130
NO_KEY = np.iinfo(np.uint64).max


def project_vertices(vertices, pose, model_scale, hole_idx, hole_r, proj, IH, IW):
    """V1..V5 for every vertex: dict of removed, behind (bool [V]) and sx, sy, d, c3 (float64 [V])."""
    P_ = np.asarray(proj, dtype=np.float64)
    T = np.asarray(pose, dtype=np.float64).reshape(3, 4)
    m = vertices.astype(np.float64)                                                   # V1
    removed = np.zeros(len(m), dtype=bool)
    for h, r in zip(([] if hole_idx is None else hole_idx), ([] if hole_r is None else hole_r)):
        if h < 0:
            continue
        c = m[h]
        d2 = ((m[:, 0] - c[0]) * (m[:, 0] - c[0]) + (m[:, 1] - c[1]) * (m[:, 1] - c[1])) + (m[:, 2] - c[2]) * (m[:, 2] - c[2])
        removed |= d2 <= np.float64(r) * np.float64(r)
    s = m * np.float64(model_scale)                                                   # V2
    X = [((T[j, 0] * s[:, 0] + T[j, 1] * s[:, 1]) + T[j, 2] * s[:, 2]) + T[j, 3] for j in range(3)]
    with np.errstate(all="ignore"):
        c = {j: ((P_[j, 0] * X[0] + P_[j, 1] * X[1]) + P_[j, 2] * X[2]) + P_[j, 3] for j in (0, 1, 3)}      # V3
        behind = ~(c[3] > 0)
        ndc_x, ndc_y = c[0] / c[3], c[1] / c[3]
        sx = ((ndc_x + 1.0) * np.float64(IW)) * 0.5                                   # V4
        sy = ((1.0 - ndc_y) * np.float64(IH)) * 0.5
        d = (1.0 + P_[2, 2]) + P_[2, 3] / X[2]                                        # V5
    return dict(removed=removed, behind=behind, sx=sx, sy=sy, d=d, c3=c[3])


def edge(a, b, sx, sy, px, py):
    """T2: E(a, b; p) for vertex indices a != b (scalars or arrays); px and py broadcast against them."""
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    with np.errstate(all="ignore"):
        e = (sx[hi] - sx[lo]) * (py - sy[lo]) - (sy[hi] - sy[lo]) * (px - sx[lo])
    return np.where(a < b, e, -e)


def weights(i0, i1, i2, neg, sx, sy, px, py):
    """T5 for one triangle: w0, w1, w2 at the nodes (py rows, px columns)."""
    w = [edge(i1, i2, sx, sy, px, py), edge(i2, i0, sx, sy, px, py), edge(i0, i1, sx, sy, px, py)]
    return [-x for x in w] if neg else w


def setup_triangles(v, triangles, IH, IW, cull):
    """T1, T3, T4 for all triangles: (indices of the live ones, neg [n] bool, ranges [n,4] int64 = r0, r1, q0, q1)."""
    V = len(v["sx"])
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    live = ((tri >= 0) & (tri < V)).all(axis=1)                                        # T1
    live &= (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    idx = np.where(live)[0]
    t = tri[idx]
    ok = ~(v["removed"][t].any(axis=1) | v["behind"][t].any(axis=1))
    idx, t = idx[ok], t[ok]
    A = edge(t[:, 0], t[:, 1], v["sx"], v["sy"], v["sx"][t[:, 2]], v["sy"][t[:, 2]])  # T3
    ok = (A != 0) & np.isfinite(A)
    if cull == 1:
        ok &= A < 0
    idx, t, A = idx[ok], t[ok], A[ok]
    sx, sy = v["sx"][t], v["sy"][t]                                                   # T4: doubles first
    q0 = np.maximum(np.ceil(sx.min(axis=1)), 0.0)
    q1 = np.minimum(np.floor(sx.max(axis=1)), np.float64(IW - 1))
    r0 = np.maximum(np.ceil(sy.min(axis=1)), 0.0)
    r1 = np.minimum(np.floor(sy.max(axis=1)), np.float64(IH - 1))
    ok = (q0 <= q1) & (r0 <= r1)
    rng = np.stack([r0[ok], r1[ok], q0[ok], q1[ok]], axis=1).astype(np.int64)
    return idx[ok], A[ok] < 0, rng


def render_frame(vertices, colors, triangles, pose, model_scale, hole_idx, hole_r, proj, IH, IW, cull, mask_mode):
    """One frame: (rgb [IH,IW,3] u8, depth [IH,IW] u16, mask [IH,IW] u16, stats [6] int32, winner [IH,IW] int64: the triangle index,
    -1 = uncovered)."""
    v = project_vertices(vertices, pose, model_scale, hole_idx, hole_r, proj, IH, IW)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    idx, negs, rng = setup_triangles(v, tri, IH, IW, cull)
    sx, sy, d = v["sx"], v["sy"], v["d"]
    keys = np.full((IH, IW), NO_KEY, dtype=np.uint64)
    tested = 0
    for t, neg, (r0, r1, q0, q1) in zip(idx.tolist(), negs.tolist(), rng.tolist()):
        i0, i1, i2 = tri[t]
        py = np.arange(r0, r1 + 1, dtype=np.float64)[:, None]
        px = np.arange(q0, q1 + 1, dtype=np.float64)[None, :]
        w0, w1, w2 = weights(i0, i1, i2, neg, sx, sy, px, py)                        # T5
        W = (w0 + w1) + w2
        cov = (w0 >= 0) & (w1 >= 0) & (w2 >= 0) & (W > 0)
        if not cov.any():
            continue
        with np.errstate(all="ignore"):
            code = np.rint(65534.0 * (((w0 * d[i0] + w1 * d[i1]) + w2 * d[i2]) / W))  # T6
        cov &= (code >= 0) & (code <= 65534)
        if not cov.any():
            continue
        tested += 1
        key = (np.where(cov, code, 0).astype(np.uint64) << np.uint64(32)) | np.uint64(t)      # T7
        sl = keys[r0:r1 + 1, q0:q1 + 1]
        sl[...] = np.where(cov, np.minimum(sl, key), sl)
    covered = keys != NO_KEY
    winner = np.where(covered, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    depth = np.where(covered, (keys >> np.uint64(32)).astype(np.int64), HORIZON).astype(np.uint16)
    rgb = np.full((IH, IW, 3), GRAY, dtype=np.uint8)
    if covered.any():                                                                 # resolve: the winners' weights again, by T5
        r, q = np.where(covered)
        wt = tri[winner[r, q]]
        py, px = r.astype(np.float64), q.astype(np.float64)
        A = edge(wt[:, 0], wt[:, 1], sx, sy, sx[wt[:, 2]], sy[wt[:, 2]])
        w = [edge(wt[:, 1], wt[:, 2], sx, sy, px, py), edge(wt[:, 2], wt[:, 0], sx, sy, px, py), edge(wt[:, 0], wt[:, 1], sx, sy, px, py)]
        w = [np.where(A < 0, -x, x) for x in w]
        col = colors.astype(np.float64)
        with np.errstate(all="ignore"):
            u = [w[k] / v["c3"][wt[:, k]] for k in range(3)]
            U = (u[0] + u[1]) + u[2]
            for ch in range(3):
                val = np.rint(((u[0] * col[wt[:, 0], ch] + u[1] * col[wt[:, 1], ch]) + u[2] * col[wt[:, 2], ch]) / U)
                rgb[r, q, ch] = np.where(val >= 0, np.minimum(val, 255.0), 0.0).astype(np.uint8)      # a NaN gives 0
    stats = np.zeros(6, dtype=np.int32)
    mask = np.zeros((IH, IW), dtype=np.uint16)
    if covered.any():
        a = np.where(covered)
        stats[:] = [covered.sum(), tested, a[0].min(), a[0].max(), a[1].min(), a[1].max()]
        if mask_mode == 0:
            mask[stats[2]:stats[3], stats[4]:stats[5]] = 65535                        # mask_generator.py:28: half-open, as it is
    if mask_mode == 1:
        mask[covered] = 65535
    return rgb, depth, mask, stats, winner


def render(vertices, colors, triangles, poses, model_scale, holes, proj, IH, IW, cull, mask_mode):
    """F frames, each on its own: rgb [F,IH,IW,3], depth, mask [F,IH,IW], stats [F,6], winner [F,IH,IW]."""
    out = [render_frame(vertices, colors, triangles, poses[f], model_scale, None if holes is None else holes[0][f],
                        None if holes is None else holes[1][f], proj, IH, IW, cull, mask_mode) for f in range(len(poses))]
    return tuple(np.stack([o[k] for o in out]) for k in range(5))


# ---- fixtures the rasteriser tests share -------------------------------------------------------------------------------------------
def icosphere(n, radius=1.0):
    """(vertices float64 [V,3] on the sphere of ``radius``, triangles int32 [20 * 4^n, 3]) of an icosahedron subdivided n times, every
    triangle wound counter-clockwise seen from outside."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g], [g, 0, -1], [g, 0, 1],
                  [-g, 0, -1], [-g, 0, 1]], dtype=np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], dtype=np.int64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for _ in range(n):
        e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        uniq, inv = np.unique(e, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        mid = v[uniq[:, 0]] + v[uniq[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = len(v) + inv.reshape(3, -1)                      # midpoints of the edges 01, 12, 20 of every face
        v = np.concatenate([v, mid])
        f = np.concatenate([np.stack([f[:, 0], m[0], m[2]], axis=1), np.stack([f[:, 1], m[1], m[0]], axis=1),
                            np.stack([f[:, 2], m[2], m[1]], axis=1), np.stack([m[0], m[1], m[2]], axis=1)])
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    flip = (np.cross(b - a, c - a) * a).sum(axis=1) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return v * radius, f.astype(np.int32)


def write_mesh_ply(path, vertices, triangles, colors=None):
    """A binary little-endian PLY of a triangle mesh with float vertices and optional uchar colours."""
    n = len(vertices)
    fields = [(a, "<f4") for a in "xyz"] + ([(a, "u1") for a in ("red", "green", "blue")] if colors is not None else [])
    rec = np.zeros(n, dtype=fields)
    for k, a in enumerate("xyz"):
        rec[a] = np.asarray(vertices)[:, k]
    if colors is not None:
        for k, a in enumerate(("red", "green", "blue")):
            rec[a] = np.asarray(colors)[:, k]
    face = np.zeros(len(triangles), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    face["n"], face["v"] = 3, triangles
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % n + \
        ("property uchar red\nproperty uchar green\nproperty uchar blue\n" if colors is not None else "") + \
        "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(triangles)
    with open(path, "wb") as f:
        f.write(head.encode("ascii") + rec.tobytes() + face.tobytes())
    return str(path)
