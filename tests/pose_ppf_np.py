"""The rule of df_ppf_model_build and df_pose_ppf (include/dfusion.h, steps F1..F3, L1..L2, M1..M2, N1..N2, V1..V3, H1..H3, C1..C3) restated
in numpy.  TEST INFRASTRUCTURE: the specification densefusion_amd/csrc/pose_ppf.hip is held to, bit for bit in the model table, in every
reference's hypothesis (the votes as exact integers), in pose_out, votes_out and stats.  One IEEE fp64 operation per numpy operation in
the contract's order; no angle is computed anywhere: only the tables, which are inputs of the call, come from cos and sin."""
import math

import numpy as np

import mesh_icp_np as icp
import pose_dense_np as dn
import pose_verify_np as pv

OK, NO_HYPOTHESIS, BAD_ITEM = 0, 1, 3
FLIP_EPS = 2.0 ** -20
MAX_ACC_BYTES = 150 * 1024
INT_MAX = 2 ** 31 - 1


def tables(NANG, NA):
    """(ang_cos [NANG-1], alpha_cos [NA/2-1], alpha_cs [NA,2]): what the host passes.  The centre of the sector k is (k + 1/2) 2 pi / NA."""
    ang_cos = np.cos(np.arange(1, NANG, dtype=np.float64) * (math.pi / NANG))
    alpha_cos = np.cos(np.arange(1, NA // 2, dtype=np.float64) * (2.0 * math.pi / NA))
    centre = (np.arange(NA, dtype=np.float64) + 0.5) * (2.0 * math.pi / NA)
    return ang_cos, alpha_cos, np.ascontiguousarray(np.stack([np.cos(centre), np.sin(centre)], axis=1))


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def bins(bound, v):
    """The number of the boundaries that v is <=, per element."""
    v = np.asarray(v, dtype=np.float64)
    return (v[..., None] <= np.asarray(bound, dtype=np.float64)).sum(axis=-1).astype(np.int64)


def pair_keys(p1, n1, p2, n2, dist_step, ND, NANG, ang_cos):
    """F1..F3 over broadcast arrays [..,3]: the keys (int64), -1 where the pair is dropped."""
    with np.errstate(all="ignore"):
        d = p2 - p1
        L = np.sqrt(_dot(d, d))
        fd = L / np.float64(dist_step)
        c1, c2, c3 = _dot(d, n1) / L, _dot(d, n2) / L, np.broadcast_to(_dot(n1, n2), L.shape)
        ok = (L > 0.0) & np.isfinite(L) & (fd < float(ND)) & ~np.isnan(c1) & ~np.isnan(c2) & ~np.isnan(c3)
        bd = np.where(ok, fd, 0.0).astype(np.int64)
        key = ((bd * NANG + bins(ang_cos, c1)) * NANG + bins(ang_cos, c2)) * NANG + bins(ang_cos, c3)
    return np.where(ok, key, -1)


def frame_rot(n):
    """L1 for normals [..,3] -> R [..,3,3]."""
    n = np.asarray(n, dtype=np.float64)
    with np.errstate(all="ignore"):
        k = 1.0 + n[..., 0]
        yz = -((n[..., 1] * n[..., 2]) / k)
        one, zero = np.ones_like(k), np.zeros_like(k)
        R = np.stack([np.stack([1.0 - (n[..., 1] * n[..., 1] + n[..., 2] * n[..., 2]) / k, n[..., 1], n[..., 2]], axis=-1),
                      np.stack([-n[..., 1], 1.0 - (n[..., 1] * n[..., 1]) / k, yz], axis=-1),
                      np.stack([-n[..., 2], yz, 1.0 - (n[..., 2] * n[..., 2]) / k], axis=-1)], axis=-2)
        flip = np.stack([np.stack([-one, zero, zero], axis=-1), np.stack([zero, -one, zero], axis=-1), np.stack([zero, zero, one], axis=-1)], axis=-2)
    return np.where((k < FLIP_EPS)[..., None, None], flip, R)


def frame_angle(R, p, q):
    """L2: (ok, c, s) of the points q [..,3] in the frame (R [..,3,3], p [..,3])."""
    with np.errstate(all="ignore"):
        d = q - p
        y, z = _dot(R[..., 1, :], d), _dot(R[..., 2, :], d)
        mm = np.sqrt(y * y + z * z)
        ok = (mm > 0.0) & np.isfinite(mm)
        return ok, y / mm, -z / mm


def sector(cm, sm, cs, ss, alpha_cos, NA):
    """V2: the sector of the model angle less the scene angle."""
    c, s = cm * cs + sm * ss, sm * cs - cm * ss
    j = bins(alpha_cos, c)
    return np.where(s >= 0.0, j, NA - 1 - j)


def model_build(points, normals, point_begin, dist_step, ND, NANG, NA, ang_cos):
    """M1, M2: (bucket_begin [O,NKEY+1] int32, entry_point [E] int32, entry_cs [E,2] float32)."""
    points, normals = np.asarray(points, dtype=np.float64).reshape(-1, 3), np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    O, NKEY = len(point_begin) - 1, ND * NANG ** 3
    begin, ep, ec, base = np.zeros((O, NKEY + 1), dtype=np.int64), [], [], 0
    for o in range(O):
        m0, m1 = int(point_begin[o]), int(point_begin[o + 1])
        n = m1 - m0
        assert 2 <= n <= 1024 and n * NA * 4 <= MAX_ACC_BYTES
        P, N = points[m0:m1], normals[m0:m1]
        key = pair_keys(P[:, None], N[:, None], P[None, :], N[None, :], dist_step[o], ND, NANG, ang_cos)
        ok, c, s = frame_angle(frame_rot(N)[:, None], P[:, None], P[None, :])
        keep = (key >= 0) & ok & ~np.eye(n, dtype=bool)
        i, j = np.nonzero(keep)                                               # ascending (i, j)
        k = key[i, j]
        order = np.argsort(k, kind="stable")
        ep.append(i[order].astype(np.int32))
        ec.append(np.stack([c[i, j][order], s[i, j][order]], axis=1).astype(np.float32))
        begin[o] = base + np.concatenate([[0], np.cumsum(np.bincount(k, minlength=NKEY))])
        base += len(k)
    return begin.astype(np.int32), np.concatenate(ep), np.concatenate(ec).reshape(-1, 2)


def grid_side(w, step):
    return (w + step - 1) // step


def scene_np(depth_f, mask_f, mask_value, rays, r0, c0, WH, WW, step, reach, gate, p22, p23, cloud_div):
    """N1, N2 for one item: (P [G,3], N [G,3], usable [G] bool); unusable slots hold zeros."""
    IH, IW = depth_f.shape
    GH, GW = grid_side(WH, step), grid_side(WW, step)
    gr, gc = np.meshgrid(np.arange(GH, dtype=np.int64), np.arange(GW, dtype=np.int64), indexing="ij")
    r, q = (int(r0) + gr * step).reshape(-1), (int(c0) + gc * step).reshape(-1)
    rays = np.asarray(rays, dtype=np.float64)

    def code(rr, qq):
        inside = (rr >= 0) & (rr < IH) & (qq >= 0) & (qq < IW)
        ri, qi = np.where(inside, rr, 0), np.where(inside, qq, 0)
        c = np.where(inside, depth_f[ri, qi].astype(np.int64), pv.NO_OBSERVATION)
        if mask_f is not None:
            c = np.where(inside & (mask_f[ri, qi].astype(np.int64) == int(mask_value)), c, pv.NO_OBSERVATION)
        return c, ri, qi

    def point(c, ri, qi):
        return dn.observed_points(np.where(c == pv.NO_OBSERVATION, 0, c), rays[ri, qi], p22, p23, cloud_div)

    co, ri, qi = code(r, q)
    counts = co != pv.NO_OBSERVATION
    p = point(co, ri, qi)
    nb, has = [], []
    for dr, dq in ((0, -reach), (0, reach), (-reach, 0), (reach, 0)):
        cn, rn, qn = code(r + dr, q + dq)
        has.append((cn != pv.NO_OBSERVATION) & (np.abs(cn - co) <= int(gate)))
        nb.append(point(cn, rn, qn))
    with np.errstate(all="ignore"):
        dx = np.where(has[1][:, None], nb[1], p) - np.where(has[0][:, None], nb[0], p)
        dy = np.where(has[3][:, None], nb[3], p) - np.where(has[2][:, None], nb[2], p)
        n = _cross(dx, dy)
        nn = _dot(n, n)
        nh = n / np.sqrt(nn)[:, None]
        nh = np.where((_dot(nh, p) > 0.0)[:, None], -nh, nh)
    usable = counts & (has[0] | has[1]) & (has[2] | has[3]) & (nn > 0.0) & np.isfinite(nn)
    return np.where(usable[:, None], p, 0.0), np.where(usable[:, None], nh, 0.0), usable


def mat_to_quat(R):
    """H2 on a nested list of Python floats."""
    tr = (R[0][0] + R[1][1]) + R[2][2]
    if tr >= R[0][0] and tr >= R[1][1] and tr >= R[2][2]:
        s = math.sqrt(1.0 + tr)
        f = 0.5 / s
        return [0.5 * s, (R[2][1] - R[1][2]) * f, (R[0][2] - R[2][0]) * f, (R[1][0] - R[0][1]) * f]
    if R[0][0] >= R[1][1] and R[0][0] >= R[2][2]:
        s = math.sqrt(((1.0 + R[0][0]) - R[1][1]) - R[2][2])
        f = 0.5 / s
        return [(R[2][1] - R[1][2]) * f, 0.5 * s, (R[0][1] + R[1][0]) * f, (R[0][2] + R[2][0]) * f]
    if R[1][1] >= R[2][2]:
        s = math.sqrt(((1.0 + R[1][1]) - R[0][0]) - R[2][2])
        f = 0.5 / s
        return [(R[0][2] - R[2][0]) * f, (R[0][1] + R[1][0]) * f, 0.5 * s, (R[1][2] + R[2][1]) * f]
    s = math.sqrt(((1.0 + R[2][2]) - R[0][0]) - R[1][1])
    f = 0.5 / s
    return [(R[1][0] - R[0][1]) * f, (R[0][2] + R[2][0]) * f, (R[1][2] + R[2][1]) * f, 0.5 * s]


def hypothesis_pose(ps, ns, pm, nm, ca, sa):
    """H1..H3: the pose [7] as a list of Python floats."""
    Rs, Rm = frame_rot(np.asarray(ns)).tolist(), frame_rot(np.asarray(nm)).tolist()
    ca, sa, pm, ps = float(ca), float(sa), [float(e) for e in pm], [float(e) for e in ps]
    A = [Rm[0], [ca * Rm[1][k] - sa * Rm[2][k] for k in range(3)], [sa * Rm[1][k] + ca * Rm[2][k] for k in range(3)]]
    R = [[(Rs[0][j] * A[0][k] + Rs[1][j] * A[1][k]) + Rs[2][j] * A[2][k] for k in range(3)] for j in range(3)]
    q = icp.normalise_quat(mat_to_quat(R))
    return q + [ps[j] - ((R[j][0] * pm[0] + R[j][1] * pm[1]) + R[j][2] * pm[2]) for j in range(3)]


def vote_reference(P, N, usable, gref, m0, nm, bucket_begin_o, entry_point, entry_cs, dist_step, ND, NANG, NA, ang_cos, alpha_cos,
                   chunk=1 << 22):
    """V1..V3 for one usable reference: (count, i, sector) of the winner, (0, 0, 0) with no vote; and the entries visited."""
    other = usable.copy()
    other[gref] = False
    idx = np.nonzero(other)[0]
    acc = np.zeros(nm * NA, dtype=np.int64)
    if len(idx) == 0:
        return (0, 0, 0), 0
    key = pair_keys(P[gref], N[gref], P[idx], N[idx], dist_step, ND, NANG, ang_cos)
    ok, cs, ss = frame_angle(frame_rot(N[gref]), P[gref], P[idx])
    v = (key >= 0) & ok
    key, cs, ss = key[v], cs[v], ss[v]
    e0, e1 = bucket_begin_o[key].astype(np.int64), bucket_begin_o[key + 1].astype(np.int64)
    lens = e1 - e0
    visited = int(lens.sum())
    start = 0
    while start < len(lens):                                                  # whole scene points, about `chunk` entries at a time
        stop = start + max(1, int(np.searchsorted(np.cumsum(lens[start:]), chunk, side="right")))
        ln = lens[start:stop]
        tot = int(ln.sum())
        if tot:
            e = np.repeat(e0[start:stop] - (np.cumsum(ln) - ln), ln) + np.arange(tot)
            i = entry_point[e].astype(np.int64)
            m = entry_cs[e].astype(np.float64)
            sec = sector(m[:, 0], m[:, 1], np.repeat(cs[start:stop], ln), np.repeat(ss[start:stop], ln), alpha_cos, NA)
            acc += np.bincount(i * NA + sec, minlength=nm * NA)
        start = stop
    cell = int(np.argmax(acc))                                                # the first of the largest: lowest i, then lowest sector
    return ((int(acc[cell]), cell // NA, cell % NA) if acc[cell] > 0 else (0, 0, 0)), visited


def cluster_np(hyp, cluster_trace, cluster_dist, K):
    """C1..C3 on hyp [NR,8]: (pose_out [K,7], votes_out [K,2] int32, hypotheses, clusters)."""
    hyp = np.asarray(hyp, dtype=np.float64)
    votes = hyp[:, 7].astype(np.int64)
    order = [i for i in np.lexsort((np.arange(len(hyp)), -votes)).tolist() if votes[i] > 0]
    dist2 = float(cluster_dist) * float(cluster_dist)
    founders, Rc, score, members = [], [], [], []
    for i in order:
        R = np.array(icp.quat_to_mat([float(e) for e in hyp[i, :4]]))
        t = hyp[i, 4:7]
        for c, f in enumerate(founders):
            d = t - hyp[f, 4:7]
            tr = (_dot(R[0], Rc[c][0]) + _dot(R[1], Rc[c][1])) + _dot(R[2], Rc[c][2])
            if tr >= cluster_trace and (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= dist2:
                score[c] += int(votes[i])
                members[c] += 1
                break
        else:
            founders.append(i); Rc.append(R); score.append(int(votes[i])); members.append(1)
    pose_out, votes_out = np.zeros((K, 7)), np.zeros((K, 2), dtype=np.int32)
    best = sorted(range(len(founders)), key=lambda c: (-score[c], c))[:K]
    for k, c in enumerate(best):
        pose_out[k] = hyp[founders[c], :7]
        votes_out[k] = (min(score[c], INT_MAX), members[c])
    return pose_out, votes_out, len(order), len(founders)


def grid_refs(GH, GW, ref_step):
    """The grid indices of the references, in reference order."""
    rr, rc = np.meshgrid(np.arange(0, GH, ref_step), np.arange(0, GW, ref_step), indexing="ij")
    return (rr * GW + rc).reshape(-1)


def ppf_np(model, proj, depth, rays, mask, items, cloud_div, WH, WW, step, reach, gate, ref_step, K, cluster_trace, cluster_dist, tabs,
           counts=None):
    """The whole call.  ``model``: dict of points, normals [NM,3], point_begin, dist_step, ND, NANG, NA, bucket_begin [O,NKEY+1],
    entry_point, entry_cs.  ``tabs`` = (ang_cos, alpha_cos, alpha_cs).  -> (pose_out [B,K,7], votes_out [B,K,2] int32, stats [B,4], hyp
    [B,NR,8]).  ``counts``: a list that receives the entries visited per item."""
    depth = np.asarray(depth)
    P44 = np.asarray(proj, dtype=np.float64).reshape(4, 4)
    items = np.asarray(items, dtype=np.int64).reshape(-1, 6)
    ang_cos, alpha_cos, alpha_cs = tabs
    ND, NANG, NA = model["ND"], model["NANG"], model["NA"]
    F, O, B = depth.shape[0], len(model["point_begin"]) - 1, len(items)
    GH, GW = grid_side(WH, step), grid_side(WW, step)
    refs = grid_refs(GH, GW, ref_step)
    NR = len(refs)
    pose_out, votes_out, stats, hyp = np.zeros((B, K, 7)), np.zeros((B, K, 2), dtype=np.int32), np.zeros((B, 4)), np.zeros((B, NR, 8))
    for b, it in enumerate(items.tolist()):
        if pv.item_bad(it, F, O, None if mask is None else len(mask)):
            stats[b, 0] = BAD_ITEM
            continue
        f, o, r0, c0, mf, mv = it
        Pp, Nn, usable = scene_np(depth[f], None if mask is None else mask[mf], mv, rays, r0, c0, WH, WW, step, reach, gate, P44[2, 2],
                                  P44[2, 3], cloud_div)
        m0, m1 = int(model["point_begin"][o]), int(model["point_begin"][o + 1])
        visited = 0
        for ri, g in enumerate(refs.tolist()):
            if not usable[g]:
                continue
            (cnt, i, sec), n = vote_reference(Pp, Nn, usable, g, m0, m1 - m0, model["bucket_begin"][o], model["entry_point"], model["entry_cs"],
                                              model["dist_step"][o], ND, NANG, NA, ang_cos, alpha_cos)
            visited += n
            if cnt > 0:
                hyp[b, ri, :7] = hypothesis_pose(Pp[g], Nn[g], model["points"][m0 + i], model["normals"][m0 + i], alpha_cs[sec, 0], alpha_cs[sec, 1])
                hyp[b, ri, 7] = cnt
        if counts is not None:
            counts.append(visited)
        pose_out[b], votes_out[b], nh, nc = cluster_np(hyp[b], cluster_trace, cluster_dist[o], K)
        stats[b] = (OK if nh else NO_HYPOTHESIS, int(usable.sum()), nh, nc)
    return pose_out, votes_out, stats, hyp


# ---- what the wrapper does on the host, for the tests ----------------------------------------------------------------------------------------
def sample_mesh(vertices, triangles, n, seed, scale=1.0):
    """n area-weighted surface samples with their face normals, seeded: (points [n,3], normals [n,3]) float64, points x ``scale``."""
    v = np.asarray(vertices, dtype=np.float64) * float(scale)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    a, e1, e2 = v[t[:, 0]], v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
    nrm = np.cross(e1, e2)
    area = np.linalg.norm(nrm, axis=1)
    live = area > 0
    rng = np.random.default_rng(seed)
    tri = rng.choice(np.nonzero(live)[0], size=n, p=area[live] / area[live].sum())
    u, w = rng.random(n), rng.random(n)
    over = u + w > 1.0
    u, w = np.where(over, 1.0 - u, u), np.where(over, 1.0 - w, w)
    return a[tri] + u[:, None] * e1[tri] + w[:, None] * e2[tri], nrm[tri] / area[tri][:, None]


def make_model(clouds, dist_frac=0.05, NANG=15, NA=30, ND=None):
    """A model dict from [(points, normals)] per object: dist_step = dist_frac x the diagonal of the samples' bounding box; the table by
    ``model_build``.  Also ``diameter`` [O]: that diagonal."""
    pts, nrm = np.concatenate([c[0] for c in clouds]), np.concatenate([c[1] for c in clouds])
    begin = np.concatenate([[0], np.cumsum([len(c[0]) for c in clouds])]).astype(np.int32)
    diag = np.array([float(np.linalg.norm(c[0].max(axis=0) - c[0].min(axis=0))) for c in clouds])
    ND = int(math.floor(1.0 / dist_frac)) + 1 if ND is None else ND
    ang_cos = tables(NANG, NA)[0]
    bb, ep, ec = model_build(pts, nrm, begin, diag * dist_frac, ND, NANG, NA, ang_cos)
    return dict(points=np.ascontiguousarray(pts), normals=np.ascontiguousarray(nrm), point_begin=begin, dist_step=diag * dist_frac, ND=ND,
                NANG=NANG, NA=NA, bucket_begin=bb, entry_point=ep, entry_cs=ec, diameter=diag)


def cluster_trace(deg):
    """What the host passes for an angle in degrees: 1 + 2 cos."""
    return 1.0 + 2.0 * math.cos(math.radians(deg))


def chain_np(sc, model, items, WH, WW, K=4, step=1, reach=1, gate=3000, ref_step=5, dense_iters=10, dense_gate=3000, tol=8, cloud_div=10000.0,
             mask=None):
    """Top K clusters, each refined by ``dense_iters`` steps of ``pose_dense_np.dense_np``, each scored by ``pose_verify_np.verify_np``; per
    item the candidate with the highest visible-surface IoU, ties to the lower rank.  ``mask`` [NM,IH,IW] (or None) picks the scene points
    and counts the verifier's unexplained nodes; the dense steps take the whole window.  ``sc``: a scene dict with vertices, triangles,
    tri_begin, model_scale, proj, depth, rays.  -> (clusters [B,K,7], refined [B,K,7], iou [B,K], kept rank [B], ppf stats [B,4])."""
    B = len(items)
    po, vo, st, _ = ppf_np(model, sc["proj"], sc["depth"], sc["rays"], mask, items, cloud_div, WH, WW, step, reach, gate, ref_step, K,
                           cluster_trace(15.0), model["diameter"] * 0.1, tables(model["NANG"], model["NA"]))
    rep = np.repeat(np.asarray(items), K, axis=0)
    refined, _ = dn.dense_np(sc["vertices"], sc["triangles"], sc["tri_begin"], sc["model_scale"], sc["proj"], sc["depth"], sc["rays"], None, rep,
                             po.reshape(B * K, 7), cloud_div, WH, WW, dense_gate, dense_iters)
    stats = pv.verify_np(sc["vertices"], sc["triangles"], sc["tri_begin"], sc["model_scale"], sc["proj"], sc["depth"], mask, rep, refined, cloud_div,
                         WH, WW, tol)
    iou = np.where(vo[:, :, 0] > 0, pv.vsiou(stats).reshape(B, K), -1.0)       # a missing rank never wins
    return po, refined.reshape(B, K, 7), iou, np.argmax(iou, axis=1), st


# ---- fixtures the tests share ------------------------------------------------------------------------------------------------------------
MODEL_POINTS = (2, 63, 64, 65, 256)                                            # per object of ``pose_dense_np.make_scene``
GATE = 6000                                                                    # neighbouring nodes of these coarse 24 x 32 frames lie thousands of codes apart


def scene_clouds(counts=MODEL_POINTS, seed=3):
    """The meshes of ``pose_dense_np.make_scene`` sampled in the units of the poses: [(points, normals)] with ``counts`` samples."""
    return [sample_mesh(v, t, n, [seed, o], dn.SCALES[o] / dn.CLOUD_DIV) for o, ((v, t), n) in enumerate(zip(dn.make_meshes(), counts))]


def wall_model(n=64, seed=5, NA=30):
    """The flat wall (object 0 of the scene, one triangle) with one distance bin wider than the model: every pair of the model has the
    same key, so one bucket holds the whole table."""
    v, t = pv.big_triangle()
    return make_model([sample_mesh(v, t, n, seed, 1.0 / dn.CLOUD_DIV)], dist_frac=2.0, ND=1, NA=NA)


def facing_model():
    """Two points whose normals look at each other: the table's two keys hold an angle of 180 degrees between the normals, which two
    scene normals that both look at the camera do not make, so every bucket a scene pair names is empty."""
    pts = np.array([[0.0, 0.0, 0.0], [0.05, 0.005, 0.0]])
    return make_model([(pts, np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]]))])


def flat_frames(code=30000, g=40):
    """depth [2,IH,IW] uint16: frame 0 holds ``code`` everywhere (a wall seen head-on: every symmetric pair of nodes ties), frame 1
    ``code`` + g on the nodes with odd r + q, so that every neighbour at one node differs by exactly g codes and at two nodes by 0."""
    r, q = np.mgrid[0:dn.IH, 0:dn.IW]
    return np.stack([np.full((dn.IH, dn.IW), code), code + g * ((r + q) % 2)]).astype(np.uint16)


def make_items(objs, r0, c0):
    """items [B,6]: item b is object objs[b] on its own frame and mask frame, mask value 7, the window's corner at (r0, c0)."""
    return np.array([[o, o, r0, c0, o, 7] for o in objs], dtype=np.int32)


def run_np(sc, model, items, WH, WW, step=1, reach=1, gate=GATE, ref_step=1, K=4, mask=True, deg=15.0, frac=0.1, counts=None):
    """``ppf_np`` on a scene of ``pose_dense_np.make_scene`` with the test defaults."""
    return ppf_np(model, sc["proj"], sc["depth"], sc["rays"], sc["mask"] if mask else None, items, dn.CLOUD_DIV, WH, WW, step, reach, gate, ref_step,
                  K, cluster_trace(deg), model["diameter"] * frac, tables(model["NANG"], model["NA"]), counts)
