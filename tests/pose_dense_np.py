"""The rule of df_pose_refine_dense (include/dfusion.h, steps S0, D1..D6) restated in numpy.  TEST INFRASTRUCTURE: the specification the
kernels of densefusion_amd/csrc/pose_verify.hip are held to, bit for bit in pose_out and all six stats columns.  D1 is
``pose_verify_np.raster_item`` (the verifier's own draw), D2 plain integer numpy, D3 and D4 one IEEE fp64 operation per numpy operation in
the contract's order, D5 the tile, lane and tree order written out, D6 ``mesh_icp_np.solve6`` / ``update_pose`` unchanged."""
import math

import numpy as np

import mesh_closest_np as m
import mesh_icp_np as icp
import pose_verify_np as pv

OK, FEW, DEGENERATE, BAD_ITEM = 0, 1, 2, 3
TILE, LANES, WAVE = 2048, 256, 64
NPART = 29                                                                  # the 28 sums of I6 and the count
MAX_TILE_BLOCKS = 64                                                        # the tile blocks of one item at most: a window of more tiles makes them stride


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------
def code_depth(c, p22, p23):
    """D3: z of a code (array), negative in front of the camera."""
    with np.errstate(all="ignore"):
        return -np.float64(p23) / (np.float64(p22) + (1.0 - np.asarray(c, dtype=np.float64) / 65534.0))


def observed_points(co, ray, p22, p23, cloud_div):
    """D3: p [n,3] in the units of the poses, camera frame."""
    z = code_depth(co, p22, p23)
    with np.errstate(all="ignore"):
        return (ray * z[:, None]) / np.float64(cloud_div)


def node_terms(keys, depth_f, mask_f, mask_value, rays, r0, c0, IH, IW, gate, p22, p23, cloud_div, pose, vertices, triangles, factor):
    """D2..D4 over the WH*WW slots of one item: (inlier [S] bool, term [S,8] = J, r, d2; zeros where no inlier, candidate [S] bool)."""
    WH, WW = keys.shape
    S = WH * WW
    inl, cand, term = np.zeros(S, dtype=bool), np.zeros(S, dtype=bool), np.zeros((S, 8))
    rlo, rhi, qlo, qhi = pv.window_nodes(r0, c0, WH, WW, IH, IW)
    if rlo > rhi or qlo > qhi:
        return inl, term, cand
    rr, qq = np.meshgrid(np.arange(rlo, rhi + 1), np.arange(qlo, qhi + 1), indexing="ij")
    rr, qq = rr.reshape(-1), qq.reshape(-1)
    slot = (rr - r0) * WW + (qq - c0)
    k = keys[rr - r0, qq - c0]
    cr = (k >> np.uint64(32)).astype(np.int64)
    co = depth_f[rr, qq].astype(np.int64)
    c = (k != pv.NO_KEY) & (co != pv.NO_OBSERVATION) & (np.abs(co - cr) <= int(gate))                    # D2
    if mask_f is not None:
        c &= mask_f[rr, qq].astype(np.int64) == int(mask_value)
    cand[slot] = c
    if not c.any():
        return inl, term, cand
    rr, qq, slot, k, co = rr[c], qq[c], slot[c], k[c], co[c]
    X = icp.model_frame(pose)
    x = m.transform_np(observed_points(co, np.asarray(rays, dtype=np.float64)[rr, qq], p22, p23, cloud_div), X[None])[0]     # D3
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)[(k & np.uint64(0xffffffff)).astype(np.int64)]
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):                                                                     # D4
        a = v[tri[:, 0]] * factor
        e1, e2 = v[tri[:, 1]] * factor - a, v[tri[:, 2]] * factor - a
        n = m._cross(e1, e2)
        nn = m._dot(n, n)
        nh = n / np.sqrt(nn)[:, None]
        r = m._dot(nh, x - a)
        t = np.concatenate([m._cross(x, nh), nh, r[:, None], (r * r)[:, None]], axis=1)
        good = (nn > 0) & np.isfinite(t).all(axis=1)
    inl[slot] = good
    term[slot] = np.where(good[:, None], t, 0.0)
    return inl, term, cand


def reduce_tiles(inl, term):
    """D5: (sums [28], count) in the order of the contract: tiles of 2048 slots, in a tile the lanes and the tree of I6, the tile totals
    in ascending order onto zero."""
    S = len(inl)
    nt = -(-S // TILE)
    cols = [term[:, a] * term[:, b] for a in range(6) for b in range(a, 6)] + [term[:, 6] * term[:, a] for a in range(6)] + [term[:, 7]]
    v = np.zeros((nt * TILE, NPART))
    v[:S] = np.where(inl[:, None], np.stack(cols + [np.ones(S)], axis=1), 0.0)
    v = v.reshape(nt, TILE // LANES, LANES, NPART)
    acc = np.zeros((nt, LANES, NPART))
    for j in range(TILE // LANES):
        acc = acc + v[:, j]
    acc = acc.reshape(nt, LANES // WAVE, WAVE, NPART)
    s = WAVE // 2
    while s >= 1:
        acc[:, :, :s] = acc[:, :, :s] + acc[:, :, s:2 * s]
        s //= 2
    tiles = (acc[:, 0, 0] + acc[:, 1, 0]) + (acc[:, 2, 0] + acc[:, 3, 0])
    tot = np.zeros(NPART)
    for t in range(nt):
        tot = tot + tiles[t]
    return [float(e) for e in tot[:28]], int(tot[28])


def dense_item(vertices, triangles, t0, t1, model_scale, proj, depth_f, mask_f, mask_value, rays, r0, c0, WH, WW, pose_in, cloud_div, gate,
               iters, cull=0, trace=None):
    """One good item: (pose [7], stats [6]) as lists of floats.  ``trace``: a list that receives (keys, inlier, candidate) of every pass."""
    IH, IW = depth_f.shape
    P = np.asarray(proj, dtype=np.float64).reshape(4, 4)
    pose = icp.normalise_quat([float(e) for e in pose_in[:4]]) + [float(e) for e in pose_in[4:7]]
    with np.errstate(all="ignore"):
        factor = np.float64(model_scale) / np.float64(cloud_div)
    stats = [0.0] * 6
    for k in range(iters + 1):
        keys, _, _ = pv.raster_item(vertices, triangles, t0, t1, float(model_scale), P, pv.pose_matrix(pose, cloud_div), IH, IW, r0, c0, WH,
                                    WW, cull)                                                            # D1
        inl, term, cand = node_terms(keys, depth_f, mask_f, mask_value, rays, r0, c0, IH, IW, gate, P[2, 2], P[2, 3], cloud_div, pose,
                                     vertices, triangles, factor)
        if trace is not None:
            trace.append((keys, inl, cand))
        sums, count = reduce_tiles(inl, term)
        rms = math.sqrt(sums[27] / count) if count > 0 else 0.0
        if k == 0:
            stats[1], stats[2] = float(count), rms
        stats[3], stats[4] = float(count), rms
        if k == iters:
            break
        if count < icp.MIN_INLIERS:
            stats[0] = float(FEW)
            break
        z = icp.solve6(sums)
        if z is None:
            stats[0] = float(DEGENERATE)
            break
        pose = icp.update_pose(pose, z)
        stats[5] += 1.0
    return pose, stats


def dense_np(vertices, triangles, tri_begin, model_scale, proj, depth, rays, mask, items, pose_in, cloud_div, WH, WW, gate, iters, cull=0,
             trace=None):
    """(pose_out [B,7], stats [B,6]) float64.  depth [F,IH,IW] uint16; rays [IH,IW,3]; mask [NM,IH,IW] uint16 or None; items int [B,6]."""
    depth = np.asarray(depth)
    F, O = depth.shape[0], len(tri_begin) - 1
    items = np.asarray(items, dtype=np.int64).reshape(-1, 6)
    pose_in = np.asarray(pose_in, dtype=np.float64).reshape(-1, 7)
    vertices = np.asarray(vertices, dtype=np.float32)
    B = len(items)
    pose_out, stats = np.zeros((B, 7)), np.zeros((B, 6))
    for b, it in enumerate(items.tolist()):
        if pv.item_bad(it, F, O, None if mask is None else len(mask)):
            pose_out[b], stats[b, 0] = icp.normalised(pose_in[b]), BAD_ITEM
            if trace is not None:
                trace.append(None)
            continue
        f, o, r0, c0, mf, mv = it
        tr = None if trace is None else []
        pose_out[b], stats[b] = dense_item(vertices, triangles, int(tri_begin[o]), int(tri_begin[o + 1]), float(model_scale[o]), proj, depth[f],
                                           None if mask is None else mask[mf], mv, rays, r0, c0, WH, WW, pose_in[b], cloud_div, gate, iters,
                                           cull, tr)
        if trace is not None:
            trace.append(tr)
    return pose_out, stats


# ---- fixtures the tests share ------------------------------------------------------------------------------------------------------------
def ray_map(proj, IH, IW):
    """The loader's ray map [IH,IW,3] of a projection matrix (``UnityDepthProjector``: the back-projection of node (r, q) at z = 1)."""
    inv = np.linalg.inv(np.asarray(proj, dtype=np.float64).reshape(4, 4))
    px = np.empty((IH, IW, 4))
    px[:, :, 0] = np.arange(-1, 1, 2.0 / IW)[:IW][None, :]
    px[:, :, 1] = -np.arange(-1, 1, 2.0 / IH)[:IH][:, None]
    px[:, :, 2], px[:, :, 3] = -1.0, 1.0
    ray = np.matmul(inv, px[..., None]).squeeze(-1)
    ray /= ray[:, :, 3, None]
    ray /= ray[:, :, 2, None]
    return np.ascontiguousarray(ray[:, :, :3])


def render_codes(vertices, triangles, t0, t1, model_scale, proj, pose, cloud_div, IH, IW, cull=0):
    """The whole-frame codes [IH,IW] int64 of one object at a pose (65535: nothing drawn) and its key plane."""
    keys, _, _ = pv.raster_item(np.asarray(vertices, dtype=np.float32), triangles, t0, t1, float(model_scale), np.asarray(proj, dtype=np.float64),
                                pv.pose_matrix(pose, cloud_div), IH, IW, 0, 0, IH, IW, cull)
    return pv.rendered_codes(keys, 0, 0, IH, IW), keys


IH, IW = 24, 32
COUNTS = (1, 63, 64, 65, 257)                                               # triangles per object; the one-triangle object is a flat wall
CLOUD_DIV = pv.CLOUD_DIV
SCALES = np.array([1.0, 1.0, 0.5, 2.0, 1.0])                                   # object 3 fills most of the frame
TRUE_POSES = np.array([[1.0, 0, 0, 0, 0.0, 0.0, -0.40], [0.9, 0.1, -0.3, 0.2, 0.01, -0.005, -0.40], [0.7, -0.4, 0.2, 0.5, -0.02, 0.01, -0.38],
                       [0.5, 0.5, -0.5, 0.4, 0.015, 0.0, -0.42], [0.8, 0.3, 0.4, -0.2, -0.01, -0.01, -0.41]])
GATE = 1500


def make_meshes():
    out = []
    for n in COUNTS:
        out.append(pv.big_triangle() if n == 1 else pv.ellipsoid(1 if n <= 80 else 2, n))
    return out


def make_scene(seed=0):
    """dict: vertices, triangles, tri_begin, model_scale, proj, rays, depth [6,IH,IW] u16, mask [6,IH,IW] u16, true [5,7].  Frame f < 5
    shows object f at ``TRUE_POSES[f]`` with noise of a few codes, holes and a far background; frame 5 holds random codes.  Mask frame f
    is 7 on most nodes of the object and on a few others."""
    rng = np.random.default_rng(seed)
    v, t, begin = icp.concat_meshes(make_meshes())
    proj = np.array(pv.PROJ, dtype=np.float64)
    sc = dict(vertices=v, triangles=t, tri_begin=begin, model_scale=SCALES, proj=proj, rays=ray_map(proj, IH, IW), true=TRUE_POSES.copy())
    depth, mask = [], []
    for f in range(len(COUNTS)):
        codes, _ = render_codes(v, t, int(begin[f]), int(begin[f + 1]), SCALES[f], proj, TRUE_POSES[f], CLOUD_DIV, IH, IW)
        drawn = codes != pv.NO_OBSERVATION
        d = np.where(drawn, np.clip(codes + rng.integers(-3, 4, codes.shape), 0, 65534), rng.integers(60000, 65536, codes.shape))
        d[rng.random(codes.shape) < 0.05] = pv.NO_OBSERVATION
        depth.append(d)
        mask.append(np.where(drawn ^ (rng.random(codes.shape) < 0.1), 7, 0))
    depth.append(rng.integers(0, 65536, (IH, IW)))
    mask.append(rng.choice(np.array([0, 7]), size=(IH, IW)))
    sc["depth"], sc["mask"] = np.stack(depth).astype(np.uint16), np.stack(mask).astype(np.uint16)
    return sc


def start_poses(objs, rng, angle=math.radians(2.0), shift=0.002):
    """The true poses of the objects turned by ``angle`` and moved by ``shift`` (cloud units), with quaternions that are not unit length."""
    out = []
    for o in objs:
        p = icp.perturb(icp.normalised(TRUE_POSES[o]), rng, angle, shift)
        p[:4] *= rng.uniform(0.5, 2.0)
        out.append(p)
    return np.array(out)


def make_call(objs, WH, WW, seed, corner=None):
    """(items [B,6], pose [B,7]): item b is object objs[b] on its own frame, mask frame and mask value 7, the window at ``corner`` (default:
    centred on the frame), from a perturbed start."""
    rng = np.random.default_rng(seed)
    r0, c0 = ((IH - WH) // 2, (IW - WW) // 2) if corner is None else corner
    items = np.array([[o, o, r0, c0, o, 7] for o in objs], dtype=np.int32)
    return items, start_poses(objs, rng)


def corners(WH, WW):
    """Window corners: at the frame's origin, inside, hanging over each of the four edges, over each of its four vertices, and wholly
    outside on each side."""
    return [(0, 0), ((IH - WH) // 2, (IW - WW) // 2), (-(WH // 2), 9), (7, -(WW // 2)), (IH - (WH + 1) // 2, 11), (8, IW - (WW + 1) // 2),
            (-(WH // 2), -(WW // 2)), (-(WH // 2), IW - (WW + 1) // 2), (IH - (WH + 1) // 2, -(WW // 2)),
            (IH - (WH + 1) // 2, IW - (WW + 1) // 2), (IH, 2), (-WH, 5), (4, IW), (6, -WW)]
