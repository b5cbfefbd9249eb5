"""The rule of df_pose_verify (include/dfusion.h, steps P0..P3) restated in numpy.  TEST INFRASTRUCTURE: the specification
densefusion_amd/csrc/pose_verify.hip is held to, bit for bit in all twelve columns.  P1 is ``mesh_icp_np.quat_to_mat`` (plain Python
floats, one IEEE operation each), P2 the rasteriser's restatement (``cad_raster_np``: ``project_vertices``, ``setup_triangles``,
``weights``) with the node range cut to the window, P3 plain integer numpy."""
import numpy as np

import cad_raster_np as mnp
import mesh_icp_np as icp

STATS = ("status", "rendered", "agree", "front", "behind", "missing", "mask", "mask_observed", "unexplained", "sum_abs", "triangles",
         "cut_triangles")
NO_OBSERVATION = 65535
NO_KEY = mnp.NO_KEY


def pose_matrix(pose, cloud_div):
    """P1: [R | t] float64 [3,4] of pose = (q wxyz, t)."""
    R = icp.quat_to_mat([float(e) for e in pose[:4]])
    with np.errstate(all="ignore"):
        t = [float(np.float64(pose[4 + j]) * np.float64(cloud_div)) for j in range(3)]
    return np.array([R[j] + [t[j]] for j in range(3)], dtype=np.float64)


def item_bad(item, F, O, NM):
    """P0; NM is None without a mask."""
    return not 0 <= item[0] < F or not 0 <= item[1] < O or (NM is not None and not 0 <= item[4] < NM)


def window_nodes(r0, c0, WH, WW, IH, IW):
    """(rlo, rhi, qlo, qhi) inclusive of window and frame together; empty when a hi is below its lo."""
    return max(r0, 0), min(r0 + WH - 1, IH - 1), max(c0, 0), min(c0 + WW - 1, IW - 1)


def raster_item(vertices, triangles, t0, t1, model_scale, proj, T34, IH, IW, r0, c0, WH, WW, cull):
    """P2: (keys uint64 [WH,WW] by window slot, triangles that took a key test, drawn triangles whose range the window cut short)."""
    keys = np.full((WH, WW), NO_KEY, dtype=np.uint64)
    rlo, rhi, qlo, qhi = window_nodes(r0, c0, WH, WW, IH, IW)
    if t1 <= t0:
        return keys, 0, 0
    v = mnp.project_vertices(vertices, T34, model_scale, None, None, proj, IH, IW)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    idx, negs, rng = mnp.setup_triangles(v, tri[t0:t1], IH, IW, cull)
    sx, sy, d = v["sx"], v["sy"], v["d"]
    tested = cut = 0
    for k, neg, (a0, a1, b0, b1) in zip(idx.tolist(), negs.tolist(), rng.tolist()):
        t = t0 + k                                                                    # the index in the call's array
        w0_, w1_, x0_, x1_ = max(a0, rlo), min(a1, rhi), max(b0, qlo), min(b1, qhi)
        if w0_ > w1_ or x0_ > x1_:
            continue
        cut += (w0_, w1_, x0_, x1_) != (a0, a1, b0, b1)
        i0, i1, i2 = tri[t]
        py = np.arange(w0_, w1_ + 1, dtype=np.float64)[:, None]
        px = np.arange(x0_, x1_ + 1, dtype=np.float64)[None, :]
        w0, w1, w2 = mnp.weights(i0, i1, i2, neg, sx, sy, px, py)                    # T5
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
        sl = keys[w0_ - r0:w1_ + 1 - r0, x0_ - c0:x1_ + 1 - c0]
        sl[...] = np.where(cov, np.minimum(sl, key), sl)
    return keys, tested, cut


def score_item(keys, depth_f, mask_f, mask_value, r0, c0, IH, IW, tol):
    """P3: the entries 1..9 of the row, Python ints."""
    WH, WW = keys.shape
    rlo, rhi, qlo, qhi = window_nodes(r0, c0, WH, WW, IH, IW)
    if rlo > rhi or qlo > qhi:
        return [0] * 9
    k = keys[rlo - r0:rhi + 1 - r0, qlo - c0:qhi + 1 - c0]
    rendered = k != NO_KEY
    cr = (k >> np.uint64(32)).astype(np.int64)
    co = depth_f[rlo:rhi + 1, qlo:qhi + 1].astype(np.int64)
    observed = co != NO_OBSERVATION
    m = np.zeros(k.shape, dtype=bool) if mask_f is None else (mask_f[rlo:rhi + 1, qlo:qhi + 1].astype(np.int64) == int(mask_value))
    missing = rendered & ~observed
    agree = rendered & observed & (np.abs(co - cr) <= tol)
    front = rendered & observed & (co < cr - tol)
    behind = rendered & observed & (co > cr + tol)
    unexplained = m & observed & (~rendered | front)
    return [int(x.sum()) for x in (rendered, agree, front, behind, missing, m, m & observed, unexplained)] + \
        [int(np.abs(co - cr)[agree].sum())]


def verify_np(vertices, triangles, tri_begin, model_scale, proj, depth, mask, items, pose, cloud_div, WH, WW, tol, cull=0, keys_out=None):
    """stats int64 [B,12].  depth [F,IH,IW] uint16; mask [NM,IH,IW] uint16 or None; items int [B,6]; pose float64 [B,7].  ``keys_out``: a
    list that receives each item's key plane [WH,WW] (None for a bad item)."""
    depth = np.asarray(depth)
    F, IH, IW = depth.shape
    O = len(tri_begin) - 1
    items = np.asarray(items, dtype=np.int64).reshape(-1, 6)
    pose = np.asarray(pose, dtype=np.float64).reshape(-1, 7)
    vertices = np.asarray(vertices, dtype=np.float32)
    stats = np.zeros((len(items), 12), dtype=np.int64)
    for b, it in enumerate(items.tolist()):
        if item_bad(it, F, O, None if mask is None else len(mask)):
            stats[b, 0] = 1
            if keys_out is not None:
                keys_out.append(None)
            continue
        f, o, r0, c0, mf, mv = it
        keys, tested, cut = raster_item(vertices, triangles, int(tri_begin[o]), int(tri_begin[o + 1]), float(model_scale[o]), proj,
                                        pose_matrix(pose[b], cloud_div), IH, IW, r0, c0, WH, WW, cull)
        stats[b, 1:10] = score_item(keys, depth[f], None if mask is None else mask[mf], mv, r0, c0, IH, IW, tol)
        stats[b, 10], stats[b, 11] = tested, cut
        if keys_out is not None:
            keys_out.append(keys)
    return stats


def vsiou(stats):
    """agree / (agree + behind + unexplained) in fp64, 0 where the denominator is 0."""
    stats = np.asarray(stats, dtype=np.int64)
    den = (stats[..., 2] + stats[..., 4] + stats[..., 8]).astype(np.float64)
    return np.where(den > 0, stats[..., 2].astype(np.float64) / np.where(den > 0, den, 1.0), 0.0)


def rendered_codes(keys, r0, c0, IH, IW):
    """The frame [IH,IW] int64 of the codes of a key plane, 65535 where nothing was rendered or outside the window."""
    WH, WW = keys.shape
    out = np.full((IH, IW), NO_OBSERVATION, dtype=np.int64)
    rlo, rhi, qlo, qhi = window_nodes(r0, c0, WH, WW, IH, IW)
    if rlo <= rhi and qlo <= qhi:
        k = keys[rlo - r0:rhi + 1 - r0, qlo - c0:qhi + 1 - c0]
        out[rlo:rhi + 1, qlo:qhi + 1] = np.where(k != NO_KEY, (k >> np.uint64(32)).astype(np.int64), NO_OBSERVATION)
    return out


# ---- fixtures the verification tests share -----------------------------------------------------------------------------------------
IH, IW, F, O, NM = 48, 64, 3, 4, 2
PROJ = [[1.16667, 0.0, 0.07500, 0.0], [0.0, 2.48814, -0.04000, 0.0], [0.0, 0.0, 0.50000, 3000.0], [0.0, 0.0, -1.0, 0.0]]
CLOUD_DIV = 10000.0
FRAME0_POSE = [1.0, 0.0, 0.0, 0.0, 0.01, -0.005, -0.4]          # frame 0 of ``make_scene`` shows object 1 at this pose
RANGES = {"a": (1, 63, 0, 64), "b": (65, 130, 2, 80)}           # triangles per object: 63 / 64 / 65 is the wave set-up boundary


def ellipsoid(n, count=None, radius=1500.0):
    """The first ``count`` triangles of an icosphere(n) squashed to an ellipsoid, radius in camera units at model scale 1."""
    v, t = mnp.icosphere(n, radius)
    return (v * np.array([1.0, 0.7, 0.5])).astype(np.float32), (t if count is None else t[:count])


def big_triangle():
    """One triangle of some 40 x 50 nodes at the test poses: far above SMALL_NODES nodes, so the whole wave walks it."""
    return np.array([[-2000, -1500, 0], [2000, -1500, 300], [0, 2000, -200]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32)


def quad(half_x=8000.0, half_y=4000.0):
    v = np.array([[-half_x, -half_y, 0], [half_x, -half_y, 0], [half_x, half_y, 0], [-half_x, half_y, 0]], dtype=np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


def make_meshes(config):
    """The four meshes of a configuration of ``RANGES`` (an empty range is a mesh of one unused vertex and no triangle)."""
    out = []
    for count in RANGES[config]:
        if count == 0:
            out.append((np.zeros((1, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32)))
        elif count == 1:
            out.append(big_triangle())
        elif count == 2:
            out.append(quad(900.0, 700.0))
        else:
            out.append(ellipsoid(1 if count <= 80 else 2, count))
    return out


def make_scene(config, seed=0):
    """dict: vertices, triangles, tri_begin, model_scale, proj, depth [F,IH,IW] u16, mask [NM,IH,IW] u16.  Frame 0 holds the codes of
    object 1 drawn whole-frame with a little noise and holes, frame 1 random codes, frame 2 a flat wall in mid-range."""
    rng = np.random.default_rng(seed)
    v, t, begin = icp.concat_meshes(make_meshes(config))
    sc = dict(vertices=v, triangles=t, tri_begin=begin, model_scale=np.array([1.0, 1.0, 0.5, 1.25]), proj=np.array(PROJ, dtype=np.float64))
    keys = []
    verify_np(v, t, begin, sc["model_scale"], sc["proj"], np.zeros((1, IH, IW), np.uint16), None, [[0, 1, 0, 0, 0, 0]],
              [FRAME0_POSE], CLOUD_DIV, IH, IW, 0, 0, keys_out=keys)
    f0 = rendered_codes(keys[0], 0, 0, IH, IW)
    f0 = np.where(f0 != NO_OBSERVATION, np.clip(f0 + rng.integers(-6, 7, f0.shape), 0, 65534), rng.integers(20000, 65536, f0.shape))
    f0[rng.random(f0.shape) < 0.1] = NO_OBSERVATION
    f1 = rng.integers(0, 65536, (IH, IW))
    f2 = 30000 + rng.integers(-40, 41, (IH, IW))
    sc["depth"] = np.stack([f0, f1, f2]).astype(np.uint16)
    sc["mask"] = rng.choice(np.array([0, 7, 65535], dtype=np.uint16), size=(NM, IH, IW))
    return sc


def random_poses(n, rng):
    """[n,7]: quaternions that are not unit length, translations (cloud units) that keep the meshes in view and in the depth range."""
    q = rng.normal(size=(n, 4)) * rng.uniform(0.5, 3.0, size=(n, 1))
    t = np.stack([rng.uniform(-0.08, 0.08, n), rng.uniform(-0.05, 0.05, n), rng.uniform(-0.45, -0.36, n)], axis=1)
    return np.concatenate([q, t], axis=1)


def corners(WH, WW):
    """Window corners: at the frame's origin, inside, hanging over each of the four edges (two with negative corners), over a vertex of
    the frame, and wholly outside on each side."""
    return [(0, 0), ((IH - WH) // 2, (IW - WW) // 2), (min(11, IH - 1), min(19, IW - 1)), (-(WH // 2), 7), (5, -(WW // 2)),
            (IH - (WH + 1) // 2, 3), (9, IW - (WW + 1) // 2), (-(WH // 2), -(WW // 2)), (IH, 2), (-WH, 5), (4, IW), (6, -WW)]


def make_items(n, WH, WW, rng):
    """[n,6] item records that cycle through ``corners`` and the objects and draw frame, mask frame and mask value; with
    ``FRAME0_POSE`` item 0 (object 1 on frame 0, corner (0, 0)) sees its own, slightly noisy depth."""
    cs = corners(WH, WW)
    items = np.array([[rng.integers(F), (k // len(cs) + k) % O, cs[k % len(cs)][0], cs[k % len(cs)][1], rng.integers(NM), (0, 7, 65535)[rng.integers(3)]]
                      for k in range(n)], dtype=np.int32)
    return items


def make_call(n, WH, WW, seed):
    """(items [n,6], pose [n,7]) of ``make_items`` and ``random_poses``, item 0 at ``FRAME0_POSE`` on frame 0."""
    rng = np.random.default_rng(seed)
    items, pose = make_items(n, WH, WW, rng), random_poses(n, rng)
    items[0, :2], pose[0] = (0, 1), FRAME0_POSE
    return items, pose
