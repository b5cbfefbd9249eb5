"""The rule of df_pose_refine_contour (include/dfusion.h, steps S0, D1..D6 with E1..E6) restated in numpy.  TEST INFRASTRUCTURE: the
specification the kernels of densefusion_amd/csrc/pose_verify.hip are held to, bit for bit in pose_out and all eight stats columns.  E1..E3
are integer numpy (E2 by brute force over the outline nodes: the definition, not the two separable passes of the kernels), E4 one IEEE fp64
operation per numpy operation in the contract's order, E5 ``pose_dense_np.reduce_tiles``'s tiles, lanes and tree with two terms per slot,
E6 ``mesh_icp_np.solve6`` / ``update_pose`` unchanged.  The plane sums are ``pose_dense_np.node_terms`` and ``reduce_tiles`` themselves."""
import math

import numpy as np

import mesh_closest_np as m
import mesh_icp_np as icp
import pose_dense_np as dn
import pose_verify_np as pv

OK, FEW, DEGENERATE, BAD_ITEM = dn.OK, dn.FEW, dn.DEGENERATE, dn.BAD_ITEM
NONE = -1
MAX_REACH, MAX_EDGE_STEP = 64, 65535
TILE, LANES, WAVE, NPART = dn.TILE, dn.LANES, dn.WAVE, dn.NPART


# ---- E1..E3, integer ---------------------------------------------------------------------------------------------------------------------
def window_exists(r0, c0, WH, WW, IH, IW):
    """[WH,WW] bool: the slots whose node lies inside the frame."""
    r, q = r0 + np.arange(WH), c0 + np.arange(WW)
    return ((r >= 0) & (r < IH))[:, None] & ((q >= 0) & (q < IW))[None, :]


def window_of(frame, r0, c0, WH, WW, fill):
    """[WH,WW] int64: ``frame`` [IH,IW] read through the window, ``fill`` where the node does not exist."""
    IH, IW = frame.shape
    out = np.full((WH, WW), fill, dtype=np.int64)
    rlo, rhi, qlo, qhi = pv.window_nodes(r0, c0, WH, WW, IH, IW)
    if rlo <= rhi and qlo <= qhi:
        out[rlo - r0:rhi + 1 - r0, qlo - c0:qhi + 1 - c0] = frame[rlo:rhi + 1, qlo:qhi + 1]
    return out


def _shift(a, dr, dq, fill):
    """b[r, q] = a[r + dr, q + dq], ``fill`` outside the window."""
    out = np.full_like(a, fill)
    H, W = a.shape
    src = a[max(dr, 0):H + min(dr, 0), max(dq, 0):W + min(dq, 0)]
    out[max(-dr, 0):H + min(-dr, 0), max(-dq, 0):W + min(-dq, 0)] = src
    return out


def outline(exists, on, code, edge_step):
    """E1 / E3 on window arrays [WH,WW]: bool, the outline nodes.  ``on`` is read only where ``exists``."""
    on = on & exists
    code = code.astype(np.int64)
    out = np.zeros_like(on)
    for dr, dq in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        nb_exists, nb_on, nb_code = _shift(exists, dr, dq, False), _shift(on, dr, dq, False), _shift(code, dr, dq, 0)
        out |= nb_exists & (~nb_on | (nb_code - code > int(edge_step)))
    return on & out


def observed_outline(depth_f, mask_f, mask_value, r0, c0, WH, WW, edge_step):
    IH, IW = depth_f.shape
    exists = window_exists(r0, c0, WH, WW, IH, IW)
    co = window_of(np.asarray(depth_f).astype(np.int64), r0, c0, WH, WW, pv.NO_OBSERVATION)
    on = co != pv.NO_OBSERVATION
    if mask_f is not None:
        on &= window_of(np.asarray(mask_f).astype(np.int64), r0, c0, WH, WW, -1) == int(mask_value)
    return outline(exists, on, co, edge_step)


def feature_map(exists, edge, reach):
    """E2: [WH,WW] int64, the slot of the nearest outline node (ties: the lowest slot) or NONE; NONE where the node does not exist."""
    WH, WW = edge.shape
    feat = np.full((WH, WW), NONE, dtype=np.int64)
    er, eq = np.nonzero(edge)                                                 # in ascending slot order
    nr, nq = np.nonzero(exists)
    if len(er) == 0 or len(nr) == 0:
        return feat
    d2 = (nr[:, None] - er[None, :]) ** 2 + (nq[:, None] - eq[None, :]) ** 2
    j = d2.argmin(axis=1)                                                     # the first of the smallest: the lowest slot
    near = d2[np.arange(len(nr)), j] <= int(reach) ** 2
    feat[nr[near], nq[near]] = er[j[near]] * WW + eq[j[near]]
    return feat


def feature_map_loops(exists, edge, reach):
    """E2 as a plain double loop over every slot and every outline node in ascending slot order (the tests' check of ``feature_map``)."""
    WH, WW = edge.shape
    feat = np.full((WH, WW), NONE, dtype=np.int64)
    nodes = [(int(r), int(q)) for r, q in zip(*np.nonzero(edge))]
    for r in range(WH):
        for q in range(WW):
            if not exists[r, q]:
                continue
            best = None
            for er, eq in nodes:
                d = (r - er) ** 2 + (q - eq) ** 2
                if d <= reach * reach and (best is None or d < best[0]):
                    best = (d, er * WW + eq)
            if best is not None:
                feat[r, q] = best[1]
    return feat


def drawn_outline(keys, r0, c0, IH, IW, edge_step):
    WH, WW = keys.shape
    cr = (keys >> np.uint64(32)).astype(np.int64)
    return outline(window_exists(r0, c0, WH, WW, IH, IW), keys != pv.NO_KEY, cr, edge_step)


# ---- E4, fp64 ----------------------------------------------------------------------------------------------------------------------------
def pair_terms(keys, feat, depth_f, rays, r0, c0, edge_step, p22, p23, cloud_div, pose, contour_scale):
    """E3, E4 over the WH*WW slots of one item: (pair [S] bool, terms [2][S,8]; zeros where no pair)."""
    IH, IW = depth_f.shape
    WH, WW = keys.shape
    S = WH * WW
    pair, terms = np.zeros(S, dtype=bool), [np.zeros((S, 8)), np.zeros((S, 8))]
    sel = drawn_outline(keys, r0, c0, IH, IW, edge_step) & (feat != NONE)
    wr, wc = np.nonzero(sel)
    if len(wr) == 0:
        return pair, terms
    slot = wr * WW + wc
    e = feat[wr, wc]
    er, eq = e // WW, e % WW
    rays = np.asarray(rays, dtype=np.float64)
    cr = (keys[wr, wc] >> np.uint64(32)).astype(np.int64)
    co = np.asarray(depth_f).astype(np.int64)[r0 + er, c0 + eq]
    X = icp.model_frame(pose)
    a = m.transform_np(dn.observed_points(cr, rays[r0 + wr, c0 + wc], p22, p23, cloud_div), X[None])[0]
    x = m.transform_np(dn.observed_points(co, rays[r0 + er, c0 + eq], p22, p23, cloud_div), X[None])[0]
    s = np.float64(contour_scale)
    good = np.ones(len(wr), dtype=bool)
    ts = []
    with np.errstate(all="ignore"):
        w = x - a
        for k in range(2):
            n = np.broadcast_to(np.asarray(X, dtype=np.float64)[:, k], x.shape)
            t = np.concatenate([m._cross(x, n) * s, n * s, (m._dot(n, w) * s)[:, None], np.zeros((len(wr), 1))], axis=1)
            good &= np.isfinite(t).all(axis=1)
            ts.append(t)
    pair[slot] = good
    for k in range(2):
        terms[k][slot] = np.where(good[:, None], ts[k], 0.0)
    return pair, terms


# ---- E5 ----------------------------------------------------------------------------------------------------------------------------------
def _products(term, ones):
    cols = [term[:, a] * term[:, b] for a in range(6) for b in range(a, 6)] + [term[:, 6] * term[:, a] for a in range(6)] + [term[:, 7]]
    return np.stack(cols + [ones], axis=1)


def reduce_pair_tiles(pair, terms):
    """``pose_dense_np.reduce_tiles`` with two terms per slot: a lane adds a slot's k = 0 products, then its k = 1 products, before it
    goes to its next slot; the count takes one per pair."""
    S = len(pair)
    nt = -(-S // TILE)
    vs = []
    for k in range(2):
        v = np.zeros((nt * TILE, NPART))
        v[:S] = np.where(pair[:, None], _products(terms[k], np.ones(S) if k == 0 else np.zeros(S)), 0.0)
        vs.append(v.reshape(nt, TILE // LANES, LANES, NPART))
    acc = np.zeros((nt, LANES, NPART))
    for j in range(TILE // LANES):
        acc = acc + vs[0][:, j]
        acc = acc + vs[1][:, j]
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


# ---- the call ----------------------------------------------------------------------------------------------------------------------------
def contour_item(vertices, triangles, t0, t1, model_scale, proj, depth_f, mask_f, mask_value, rays, r0, c0, WH, WW, pose_in, cloud_div, gate,
                 iters, edge_step, reach, contour_scale, cull=0, trace=None):
    """One good item: (pose [7], stats [8]) as lists of floats.  ``trace``: a list that receives (keys, inlier, pair, feat) of every pass."""
    IH, IW = depth_f.shape
    P = np.asarray(proj, dtype=np.float64).reshape(4, 4)
    pose = icp.normalise_quat([float(e) for e in pose_in[:4]]) + [float(e) for e in pose_in[4:7]]
    with np.errstate(all="ignore"):
        factor = np.float64(model_scale) / np.float64(cloud_div)
    exists = window_exists(r0, c0, WH, WW, IH, IW)
    feat = feature_map(exists, observed_outline(depth_f, mask_f, mask_value, r0, c0, WH, WW, edge_step), reach)         # E1, E2
    stats = [0.0] * 8
    for k in range(iters + 1):
        keys, _, _ = pv.raster_item(vertices, triangles, t0, t1, float(model_scale), P, pv.pose_matrix(pose, cloud_div), IH, IW, r0, c0, WH,
                                    WW, cull)                                                            # D1
        inl, term, _ = dn.node_terms(keys, depth_f, mask_f, mask_value, rays, r0, c0, IH, IW, gate, P[2, 2], P[2, 3], cloud_div, pose,
                                     vertices, triangles, factor)
        pair, terms = pair_terms(keys, feat, depth_f, rays, r0, c0, edge_step, P[2, 2], P[2, 3], cloud_div, pose, contour_scale)
        if trace is not None:
            trace.append((keys, inl, pair, feat))
        psum, count = dn.reduce_tiles(inl, term)
        csum, pairs = reduce_pair_tiles(pair, terms)
        sums = [float(np.float64(psum[i]) + np.float64(csum[i])) for i in range(27)] + [psum[27]]        # E5
        rms = math.sqrt(psum[27] / count) if count > 0 else 0.0
        if k == 0:
            stats[1], stats[2], stats[6] = float(count), rms, float(pairs)
        stats[3], stats[4], stats[7] = float(count), rms, float(pairs)
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


def contour_np(vertices, triangles, tri_begin, model_scale, proj, depth, rays, mask, items, pose_in, cloud_div, WH, WW, gate, iters,
               edge_step, reach, contour_scale, cull=0, trace=None):
    """(pose_out [B,7], stats [B,8]) float64: ``pose_dense_np.dense_np``'s arguments with the three of the outline term."""
    depth = np.asarray(depth)
    F, O = depth.shape[0], len(tri_begin) - 1
    items = np.asarray(items, dtype=np.int64).reshape(-1, 6)
    pose_in = np.asarray(pose_in, dtype=np.float64).reshape(-1, 7)
    vertices = np.asarray(vertices, dtype=np.float32)
    B = len(items)
    pose_out, stats = np.zeros((B, 7)), np.zeros((B, 8))
    for b, it in enumerate(items.tolist()):
        if pv.item_bad(it, F, O, None if mask is None else len(mask)):
            pose_out[b], stats[b, 0] = icp.normalised(pose_in[b]), BAD_ITEM
            if trace is not None:
                trace.append(None)
            continue
        f, o, r0, c0, mf, mv = it
        tr = None if trace is None else []
        pose_out[b], stats[b] = contour_item(vertices, triangles, int(tri_begin[o]), int(tri_begin[o + 1]), float(model_scale[o]), proj,
                                             depth[f], None if mask is None else mask[mf], mv, rays, r0, c0, WH, WW, pose_in[b], cloud_div,
                                             gate, iters, edge_step, reach, contour_scale, cull, tr)
        if trace is not None:
            trace.append(tr)
    return pose_out, stats
