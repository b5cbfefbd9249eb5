"""The rule of df_pose_sym_error (include/dfusion.h, steps E0..E7) restated in numpy, and the cases its tests share.  E1 is
``mesh_icp_np.quat_to_mat``; every product, sum, difference, quotient and square root below is one IEEE fp64 operation in the order the
header writes; nothing is fused.  The maxima and minima are exact, so the order they are taken in does not show."""
import math

import numpy as np

import mesh_icp_np as icp

OK, BAD_ITEM = 0, 1
STATS = ("status", "mssd", "mssd_sym", "mspd", "mspd_sym", "vertices")
INF = float("inf")


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------
def pose_matrix(pose):
    """E1: [R | t] as nested lists of Python floats."""
    R = icp.quat_to_mat([float(e) for e in pose[:4]])
    return [[R[j][0], R[j][1], R[j][2], float(pose[4 + j])] for j in range(3)]


def compose(M, S):
    """E2: G = M o S, [3,4] float64."""
    G = np.zeros((3, 4))
    for j in range(3):
        for k in range(4):
            G[j, k] = (M[j][0] * float(S[0][k]) + M[j][1] * float(S[1][k])) + M[j][2] * float(S[2][k])
        G[j, 3] = G[j, 3] + M[j][3]
    return G


def transform(X, x):
    """E3 (Q1): X [..,3,4] applied to x [V,3] -> [..,V,3]."""
    X = np.asarray(X, dtype=np.float64)
    return np.stack([((X[..., j, 0, None] * x[:, 0] + X[..., j, 1, None] * x[:, 1]) + X[..., j, 2, None] * x[:, 2]) + X[..., j, 3, None]
                     for j in range(3)], axis=-1)


def project(proj, p, IH, IW):
    """E5: (u, v, has a pixel) of the points p [..,3]."""
    P = np.asarray(proj, dtype=np.float64).reshape(4, 4)
    with np.errstate(all="ignore"):
        c = [((P[k, 0] * p[..., 0] + P[k, 1] * p[..., 1]) + P[k, 2] * p[..., 2]) + P[k, 3] for k in (0, 1, 3)]
        i = 1.0 / c[2]
        u = (((c[0] * i) + 1.0) * float(IW)) * 0.5
        v = ((1.0 - (c[1] * i)) * float(IH)) * 0.5
    return u, v, c[2] > 0.0


def item_maxima(x, pose_est, pose_gt, sym, proj, IH, IW, sym_step=64):
    """E1..E6 and the maxima of E7 for one item: x [V,3] float64 (widened vertices), sym [S,3,4] -> (D [S], P [S])."""
    E, M = pose_matrix(pose_est), pose_matrix(pose_gt)
    with np.errstate(all="ignore"):
        pe = transform(np.array(E), x)
        ue, ve, oke = project(proj, pe, IH, IW)
        D, P = [], []
        for s0 in range(0, len(sym), sym_step):
            G = np.stack([compose(M, S) for S in sym[s0:s0 + sym_step]])
            pg = transform(G, x)                                    # [s,V,3]
            d = pe[None] - pg
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            d2 = np.where(d2 < INF, d2, INF)                        # E4
            ug, vg, okg = project(proj, pg, IH, IW)
            du, dv = ue[None] - ug, ve[None] - vg
            e2 = du * du + dv * dv
            e2 = np.where((e2 < INF) & oke[None] & okg, e2, INF)    # E6
            D.append(d2.max(axis=1))
            P.append(e2.max(axis=1))
    return np.concatenate(D), np.concatenate(P)


def sym_error_np(vertices, vertex_begin, sym, sym_begin, obj, pose_est, pose_gt, proj, IH, IW):
    """out [B,6] float64 of the whole call; ``sym`` [NS,3,4] or [NS,12]."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    sym = np.asarray(sym, dtype=np.float64).reshape(-1, 3, 4)
    O = len(vertex_begin) - 1
    out = np.zeros((len(obj), 6))
    for b, o in enumerate(np.asarray(obj).tolist()):
        if not 0 <= o < O or vertex_begin[o + 1] <= vertex_begin[o] or sym_begin[o + 1] <= sym_begin[o]:
            out[b, 0] = BAD_ITEM                                    # E0
            continue
        x = v[vertex_begin[o]:vertex_begin[o + 1]]
        D, P = item_maxima(x, pose_est[b], pose_gt[b], sym[sym_begin[o]:sym_begin[o + 1]], proj, IH, IW)
        ds, es = int(np.argmin(D)), int(np.argmin(P))               # the first of equal minima: the lowest s
        out[b] = [OK, math.sqrt(D[ds]) if D[ds] < INF else INF, ds, math.sqrt(P[es]) if P[es] < INF else INF, es, len(x)]
    return out


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------
IH, IW = 120, 160
PROJ = np.array([[1.6, 0, 0, 0], [0, 2.1, 0, 0], [0, 0, -1.002, -0.2], [0, 0, -1, 0]], dtype=np.float64)


def rotation(axis, angle):
    """[3,3] by Rodrigues; exact for the half and quarter turns about a coordinate axis once rounded."""
    x, y, z = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def cyclic_set(n, axis=(0, 0, 1), flip=False, center=(0.0, 0.0, 0.0)):
    """[n or 2n,3,4]: the rotations by 2 pi k / n about ``axis`` through ``center``, with ``flip`` each followed by a half turn about a
    perpendicular axis; the identity first."""
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    perp = np.cross(a, [1.0, 0, 0] if abs(a[0]) < 0.9 else [0, 1.0, 0])
    c = np.asarray(center, dtype=np.float64)
    Rs = [rotation(a, 2 * math.pi * k / n) if k else np.eye(3) for k in range(n)]
    if flip:
        Rs += [rotation(perp, math.pi) @ R for R in Rs]
    return np.stack([np.concatenate([R, (c - R @ c)[:, None]], axis=1) for R in Rs])


def quat_of(R):
    """A unit quaternion (w, x, y, z) of the rotation R, w >= 0 (host maths for fixtures only)."""
    t = np.trace(R)
    w = math.sqrt(max(0.0, 1 + t)) / 2
    if w > 1e-6:
        q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    else:
        k = int(np.argmax(np.diag(R)))
        e = np.zeros(3)
        e[k] = math.sqrt(max(0.0, (1 + R[k, k]) / 2))
        for j in range(3):
            if j != k:
                e[j] = (R[j, k] + R[k, j]) / (4 * e[k])
        q = np.array([0.0, e[0], e[1], e[2]])
    return q / np.linalg.norm(q)


def random_poses(n, rng, depth=(-6.0, -3.0), lateral=0.5):
    """[n,7] poses in front of the renderers' camera (it looks along -z)."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = np.stack([rng.uniform(-lateral, lateral, n), rng.uniform(-lateral, lateral, n), rng.uniform(depth[0], depth[1], n)], axis=1)
    return np.concatenate([q, t], axis=1)


def pack(clouds, sets):
    """(vertices float32 [V,3], vertex_begin, sym [NS,3,4], sym_begin) of per-object vertex arrays and symmetry sets (either may be empty)."""
    vb = np.cumsum([0] + [len(c) for c in clouds]).astype(np.int32)
    sb = np.cumsum([0] + [len(s) for s in sets]).astype(np.int32)
    v = np.concatenate([np.asarray(c, dtype=np.float32).reshape(-1, 3) for c in clouds])
    s = np.concatenate([np.asarray(s, dtype=np.float64).reshape(-1, 3, 4) for s in sets])
    return v, vb, s, sb


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


# ---- df_pose_vsd (include/dfusion.h, P0..P2 of df_pose_verify twice, then S1..S4) ------------------------------------------------------------
VSD_STATS = ("status", "union", "inter", "rendered_e")             # then bad_0 .. bad_{NT-1}


def code_distance(c, p22, p23, rho):
    """S2: D(c) = |z(c)| rho, elementwise."""
    with np.errstate(all="ignore"):
        z = -np.float64(p23) / (np.float64(p22) + (1.0 - np.asarray(c, dtype=np.float64) / 65534.0))
    return np.where(z < 0.0, -z, z) * rho


def vsd_nodes(keys_e, keys_g, depth_f, rays, r0, c0, p22, p23, delta):
    """S1..S3 over the nodes of window and frame together: (vis_e, vis_g, rendered_e, gap) arrays, or None when there is no node."""
    import pose_verify_np as pv
    WH, WW = keys_e.shape
    IH, IW = depth_f.shape
    rlo, rhi, qlo, qhi = pv.window_nodes(r0, c0, WH, WW, IH, IW)
    if rlo > rhi or qlo > qhi:
        return None
    ke, kg = (k[rlo - r0:rhi + 1 - r0, qlo - c0:qhi + 1 - c0] for k in (keys_e, keys_g))
    re, rg = ke != pv.NO_KEY, kg != pv.NO_KEY
    ce, cg = (np.where(r, (k >> np.uint64(32)).astype(np.int64), 0) for k, r in ((ke, re), (kg, rg)))
    co = depth_f[rlo:rhi + 1, qlo:qhi + 1].astype(np.int64)
    seen = co != pv.NO_OBSERVATION
    ray = np.asarray(rays, dtype=np.float64)[rlo:rhi + 1, qlo:qhi + 1]
    rho = np.sqrt((ray[..., 0] * ray[..., 0] + ray[..., 1] * ray[..., 1]) + ray[..., 2] * ray[..., 2])      # S1
    De, Dg, Do = (code_distance(c, p22, p23, rho) for c in (ce, cg, np.where(seen, co, 0)))
    with np.errstate(all="ignore"):
        vis_g = rg & (~seen | (Dg - Do <= delta))
        vis_e = re & (~seen | (De - Do <= delta) | vis_g)
        d = Dg - De
    return vis_e, vis_g, re, np.where(d < 0.0, -d, d)


def vsd_np(vertices, triangles, tri_begin, model_scale, proj, depth, rays, items, pose_est, pose_gt, cloud_div, delta, tau, WH, WW, cull=0,
           gaps_out=None):
    """stats int64 [B, 4 + NT].  ``gaps_out``: a list that receives, per item, the |D_g - D_e| of its inter nodes (None for a bad item)."""
    import pose_verify_np as pv
    depth = np.asarray(depth)
    F, IH, IW = depth.shape
    O = len(tri_begin) - 1
    P = np.asarray(proj, dtype=np.float64).reshape(4, 4)
    tau = np.asarray(tau, dtype=np.float64).reshape(O, -1)
    NT = tau.shape[1]
    items = np.asarray(items, dtype=np.int64).reshape(-1, 6)
    vertices = np.asarray(vertices, dtype=np.float32)
    stats = np.zeros((len(items), 4 + NT), dtype=np.int64)
    for b, it in enumerate(items.tolist()):
        if pv.item_bad(it, F, O, None):
            stats[b, 0] = 1
            if gaps_out is not None:
                gaps_out.append(None)
            continue
        f, o, r0, c0 = it[:4]
        keys = [pv.raster_item(vertices, triangles, int(tri_begin[o]), int(tri_begin[o + 1]), float(model_scale[o]), P,
                               pv.pose_matrix(np.asarray(p, dtype=np.float64)[b], cloud_div), IH, IW, r0, c0, WH, WW, cull)[0] for p in (pose_est, pose_gt)]
        nodes = vsd_nodes(keys[0], keys[1], depth[f], rays, r0, c0, P[2, 2], P[2, 3], float(delta[o]))
        if nodes is None:
            if gaps_out is not None:
                gaps_out.append(np.zeros(0))
            continue
        vis_e, vis_g, re, gap = nodes
        inter = vis_e & vis_g
        stats[b, 1:4] = [int((vis_e | vis_g).sum()), int(inter.sum()), int(re.sum())]
        stats[b, 4:] = [int((inter & (gap >= t)).sum()) for t in tau[o]]
        if gaps_out is not None:
            gaps_out.append(gap[inter])
    return stats


def vsd_values(stats):
    """vsd_k = (bad_k + union - inter) / union in fp64, 1 where union = 0: float64 [B, NT]."""
    stats = np.asarray(stats, dtype=np.int64)
    union, inter = stats[:, 1:2].astype(np.float64), stats[:, 2:3].astype(np.float64)
    return np.where(union > 0, (stats[:, 4:].astype(np.float64) + union - inter) / np.where(union > 0, union, 1.0), 1.0)
