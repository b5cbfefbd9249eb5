"""The rule of df_mesh_icp (include/dfusion.h, steps S0, I1..I10) restated in numpy and plain Python floats, and the scenes its tests
share.  Steps I2, I3 are ``mesh_closest_np.transform_np`` / ``closest_np``; the sums run in the kernels' order (lane l of 256 takes the
points l, l + 256, ...; a binary tree over each 64 lanes; the four totals pairwise); the Cholesky solve and the update are written out
operation by operation.  Every product, sum, difference, quotient and square root is one IEEE fp64 operation; nothing is fused."""
import math

import numpy as np

import mesh_closest_np as m

OK, FEW, DEGENERATE, BAD_OBJECT = 0, 1, 2, 3
MIN_INLIERS, LANES, WAVE = 6, 256, 64
PIVOT_REL = 2.0 ** -40
EPS4 = 2.220446049250313e-16 * 4.0


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------
def quat_to_mat(q):
    """I1: 3 x 3 nested list."""
    w, x, y, z = q
    n = ((w * w + x * x) + y * y) + z * z
    if n < EPS4:
        return [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    s = math.sqrt(2.0 / n)                                          # a NaN stays a NaN
    w, x, y, z = w * s, x * s, y * s, z * s
    return [[(1.0 - y * y) - z * z, x * y - z * w, x * z + y * w],
            [x * y + z * w, (1.0 - x * x) - z * z, y * z - x * w],
            [x * z - y * w, y * z + x * w, (1.0 - x * x) - y * y]]


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def normalise_quat(q):
    """S0: q / |q|, negated when w < 0."""
    w, x, y, z = q
    n2 = ((w * w + x * x) + y * y) + z * z
    n = float(np.sqrt(np.float64(n2)))
    q = [_div(w, n), _div(x, n), _div(y, n), _div(z, n)]
    return [-e for e in q] if q[0] < 0.0 else q


def normalised(pose):
    """S0 of a whole pose: float64 [7]."""
    return np.array(normalise_quat([float(e) for e in pose[:4]]) + [float(e) for e in pose[4:7]], dtype=np.float64)


def model_frame(pose):
    """I2: X = [R^T | o] as a [3,4] array."""
    R = quat_to_mat(pose[:4])
    t = pose[4:7]
    return np.array([[R[0][j], R[1][j], R[2][j], -((R[0][j] * t[0] + R[1][j] * t[1]) + R[2][j] * t[2])] for j in range(3)], dtype=np.float64)


def point_terms(vertices, triangles, points, pose, max_dist, cull):
    """I2..I5 for one item on its own triangle range: (inlier [N] bool, term [N,8] = J, r, d2; zeros where no inlier)."""
    X = model_frame(pose)
    p = np.asarray(points)
    if p.dtype != np.float64:                                       # the contract's points are fp32 and widen exactly; float64 points are
        p = p.astype(np.float32).astype(np.float64)                 # taken as they are (the host convergence test: fp32 limits a fit at 6e-8)
    d2, tri, c = m.closest_np(vertices, triangles, p, X[None])
    d2, tri, c = d2[0], tri[0].astype(np.int64), c[0]
    x = m.transform_np(p, X[None])[0]
    rec = m.prepare_np(vertices, triangles)
    tc = np.where(tri >= 0, tri, 0)
    n, nn = rec["n"][tc], rec["nn"][tc]
    with np.errstate(all="ignore"):
        md2 = np.float64(max_dist) * np.float64(max_dist)
        inl = (tri >= 0) & (d2 <= md2) & (d2 < m.INF) & (nn > 0)
        if cull:
            inl &= m._dot(n, X[None, :, 3] - c) > 0
        sn = np.sqrt(nn)
        nh = n / sn[:, None]
        term = np.concatenate([m._cross(x, nh), nh, m._dot(nh, x - c)[:, None], d2[:, None]], axis=1)
    return inl, np.where(inl[:, None], term, 0.0)


def reduce_terms(inl, term):
    """I6: (sums [28] = A's 21 upper entries a-major, G's 6, D; count)."""
    N = len(inl)
    cols = [term[:, a] * term[:, b] for a in range(6) for b in range(a, 6)] + [term[:, 6] * term[:, a] for a in range(6)] + [term[:, 7]]
    v = np.where(inl[:, None], np.stack(cols, axis=1), 0.0)
    acc = np.zeros((LANES, 28))
    for i0 in range(0, N, LANES):
        k = min(LANES, N - i0)
        acc[:k] = acc[:k] + v[i0:i0 + k]
    acc = acc.reshape(LANES // WAVE, WAVE, 28)
    s = WAVE // 2
    while s >= 1:
        acc[:, :s] = acc[:, :s] + acc[:, s:2 * s]
        s //= 2
    tot = (acc[0, 0] + acc[1, 0]) + (acc[2, 0] + acc[3, 0])
    return [float(e) for e in tot], int(inl.sum())


def solve6(sums):
    """I8: z (6 floats), or None when a pivot is too small."""
    A = [[0.0] * 6 for _ in range(6)]
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[a][b] = A[b][a] = sums[k]
            k += 1
    dmax = A[0][0]
    for a in range(1, 6):
        dmax = A[a][a] if A[a][a] > dmax else dmax
    thr = PIVOT_REL * dmax
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not s > thr:
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            v = A[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    y, z = [0.0] * 6, [0.0] * 6
    for i in range(6):
        v = -sums[21 + i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v / L[i][i]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * z[k]
        z[i] = v / L[i][i]
    return z


def update_pose(pose, z):
    """I9: the new pose (7 floats)."""
    h = [z[0] * 0.5, z[1] * 0.5, z[2] * 0.5]
    mm = math.sqrt(((1.0 + h[0] * h[0]) + h[1] * h[1]) + h[2] * h[2])
    cw, cx, cy, cz = 1.0 / mm, -(h[0] / mm), -(h[1] / mm), -(h[2] / mm)
    qw, qx, qy, qz = pose[:4]
    q = normalise_quat([((qw * cw - qx * cx) - qy * cy) - qz * cz, ((qw * cx + qx * cw) + qy * cz) - qz * cy,
                        ((qw * cy - qx * cz) + qy * cw) + qz * cx, ((qw * cz + qx * cy) - qy * cx) + qz * cw])
    R = quat_to_mat(q)
    return q + [pose[4 + j] - ((R[j][0] * z[3] + R[j][1] * z[4]) + R[j][2] * z[5]) for j in range(3)]


def icp_item(vertices, triangles, points, pose_in, max_dist, iters, cull=0):
    """One item on its own triangle range ([T,3], T >= 1): (pose [7], stats [6]) as lists of floats."""
    pose = normalise_quat([float(e) for e in pose_in[:4]]) + [float(e) for e in pose_in[4:7]]
    stats = [0.0] * 6
    for k in range(iters + 1):
        inl, term = point_terms(vertices, triangles, points, pose, max_dist, cull)
        sums, count = reduce_terms(inl, term)
        rms = math.sqrt(sums[27] / count) if count > 0 else 0.0
        if k == 0:
            stats[1], stats[2] = float(count), rms
        stats[3], stats[4] = float(count), rms
        if k == iters:
            break
        if count < MIN_INLIERS:
            stats[0] = float(FEW)
            break
        z = solve6(sums)
        if z is None:
            stats[0] = float(DEGENERATE)
            break
        pose = update_pose(pose, z)
        stats[5] += 1.0
    return pose, stats


def icp_np(vertices, triangles, tri_begin, max_dist, obj, points, pose_in, iters, cull=0):
    """(pose_out [B,7], stats [B,6]) float64 by S0, I1..I10."""
    triangles = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    points = np.asarray(points, dtype=np.float32)
    pose_in = np.asarray(pose_in, dtype=np.float64)
    B, O = len(points), len(tri_begin) - 1
    pose_out, stats = np.zeros((B, 7)), np.zeros((B, 6))
    for b in range(B):
        o = int(obj[b])
        if not 0 <= o < O or tri_begin[o + 1] <= tri_begin[o]:
            pose_out[b] = normalise_quat([float(e) for e in pose_in[b, :4]]) + [float(e) for e in pose_in[b, 4:]]
            stats[b, 0] = BAD_OBJECT
            continue
        pose_out[b], stats[b] = icp_item(vertices, triangles[tri_begin[o]:tri_begin[o + 1]], points[b], pose_in[b], max_dist[o], iters, cull)
    return pose_out, stats


# ---- helpers of the tests ------------------------------------------------------------------------------------------------------------------
def quat_from_axis_angle(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / math.sqrt(float(a @ a))
    return np.concatenate([[math.cos(angle / 2)], math.sin(angle / 2) * a])


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw])


def apply_pose(pose, pts):
    """camera = R model + t, float64 [n,3]."""
    return np.asarray(pts, dtype=np.float64) @ np.array(quat_to_mat([float(e) for e in pose[:4]])).T + np.asarray(pose[4:7], dtype=np.float64)


def random_pose(rng, t_scale=1.0):
    q = rng.normal(size=4)
    q = q / math.sqrt(float(q @ q))
    return np.concatenate([q if q[0] >= 0 else -q, rng.normal(size=3) * t_scale])


def perturb(pose, rng, angle, shift):
    """``pose`` followed by a rotation of ``angle`` about a random axis through the object's origin and a shift of norm ``shift``."""
    d = rng.normal(size=3)
    d = d / math.sqrt(float(d @ d)) * shift
    q = quat_mul(quat_from_axis_angle(rng.normal(size=3), angle), pose[:4])
    return np.concatenate([q, np.asarray(pose[4:7]) + d])


def surface_samples(vertices, triangles, n, rng, facing=None):
    """n area-weighted samples of the surface (float64 [n,3]) and their triangles; ``facing``: keep only the samples whose face normal has
    a positive dot with that direction."""
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(triangles, dtype=np.int64)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    nrm = np.cross(b - a, c - a)
    area = np.sqrt((nrm * nrm).sum(axis=1))
    pick = rng.choice(len(t), size=n, p=area / area.sum())
    u, w = rng.random(n), rng.random(n)
    flip = u + w > 1
    u, w = np.where(flip, 1 - u, u), np.where(flip, 1 - w, w)
    pts = a[pick] + u[:, None] * (b - a)[pick] + w[:, None] * (c - a)[pick]
    if facing is not None:
        keep = nrm[pick] @ np.asarray(facing, dtype=np.float64) > 0
        pts, pick = pts[keep], pick[keep]
    return pts, pick


def diameter(vertices):
    v = np.asarray(vertices, dtype=np.float64)
    return float(np.sqrt(((v.max(axis=0) - v.min(axis=0)) ** 2).sum()))


def mean_point_error(pose, truth, model_pts):
    d = apply_pose(pose, model_pts) - apply_pose(truth, model_pts)
    return float(np.sqrt((d * d).sum(axis=1)).mean())


def quat_from_matrix(R):
    """The unit quaternion (w >= 0) of a proper rotation matrix, float64 (a helper of the tests: not part of the rule)."""
    R = np.asarray(R, dtype=np.float64)
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], 0, 0, 0], [R[0, 1] + R[1, 0], R[1, 1] - R[0, 0] - R[2, 2], 0, 0],
                  [R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], R[2, 2] - R[0, 0] - R[1, 1], 0],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, v = np.linalg.eigh(K)
    q = v[[3, 0, 1, 2], np.argmax(w)]
    return q if q[0] >= 0 else -q


# ---- the shapes the GPU test walks (and a host program that runs mesh_icp_core.h over the same) -----------------------------------------
INF = float("inf")
N_SHAPES = (1, 5, 6, 63, 64, 65, 129, 513)      # below, at and above the six inliers; around a wave's 64 slots, a workgroup's 128 queries,
                                                # the 256 lanes of the sums (513: three rounds, the last with one point)


def concat_meshes(meshes):
    """(vertices float32, triangles int32 with global indices, tri_begin int32 [O+1]): what ``MeshIcp`` uploads at scale 1."""
    verts, tris, begin = [], [], [0]
    for v, t in meshes:
        tris.append(np.asarray(t, dtype=np.int32) + np.int32(sum(len(x) for x in verts)))
        verts.append(np.asarray(v, dtype=np.float32))
        begin.append(begin[-1] + len(t))
    return np.concatenate(verts), np.concatenate(tris), np.array(begin, dtype=np.int32)


def fit_item(mesh, n, rng, deg=5.0, tau=0.05):
    """(points float32 [n,3], start pose [7]): n samples of the mesh's surface under a random pose, and that pose perturbed."""
    pts, _ = surface_samples(mesh[0], mesh[1], n, rng)
    truth = random_pose(rng)
    return apply_pose(truth, pts).astype(np.float32), perturb(truth, rng, math.radians(deg), tau * diameter(mesh[0]))


def flat_item(n, rng):
    """n points 0.01 above the +z face of the bracket's box under a random pose, and that pose: geometry that holds three degrees only."""
    pose = random_pose(rng)
    face = np.stack([rng.uniform(-.4, .4, n), rng.uniform(-.9, .9, n), np.full(n, 1.51)], axis=1)
    return apply_pose(pose, face).astype(np.float32), pose


def make_icp_cases(tile=128):
    """name -> dict(meshes, max_dist, obj, points [B,N,3], pose [B,7], iters, cull)."""
    rng = np.random.default_rng(2024)
    br = m.bracket()
    cases = {}
    for T in (1, tile - 1, tile, tile + 1):           # the winner is the range's last triangle: one flat triangle, so `degenerate`
        mesh = m.far_mesh_with_near_last(T, 100 + T)
        pts = rng.uniform(-.5, .5, (1, 65, 3)).astype(np.float32)
        cases["T%d" % T] = dict(meshes=[mesh], max_dist=[INF], obj=[0], points=pts, pose=np.array([[1.0, 0, 0, 0, 0, 0, 0]]), iters=1, cull=0)
    for n in N_SHAPES:
        for B, iters in ((1, 4), (3, 1)):
            items = [fit_item(br, n, rng) for _ in range(B)]
            cases["N%d_B%d_it%d" % (n, B, iters)] = dict(meshes=[br], max_dist=[INF], obj=[0] * B, points=np.stack([i[0] for i in items]),
                                                         pose=np.stack([i[1] for i in items]), iters=iters, cull=0)
    for n in (65, 513):
        pts, start = fit_item(br, n, rng)
        cases["N%d_B1_it0" % n] = dict(meshes=[br], max_dist=[0.2], obj=[0], points=pts[None], pose=start[None], iters=0, cull=1)
    # items of one call on different ranges: the bracket's range starts at 127, mid-tile, the tetrahedron's at 151; object 3 is empty
    meshes = [m.far_mesh_with_near_last(tile - 1, 5), br, m.scalene_tetrahedron(), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),
              m.far_mesh_with_near_last(tile + 1, 6)]
    items = [fit_item(br, 130, rng), (rng.uniform(-.5, .5, (130, 3)).astype(np.float32), np.array([1.0, 0, 0, 0, 0, 0, 0])),
             fit_item(m.scalene_tetrahedron(), 130, rng), fit_item(br, 130, rng), (rng.uniform(-.5, .5, (130, 3)).astype(np.float32), random_pose(rng, .1))]
    cases["ranges"] = dict(meshes=meshes, max_dist=[INF, INF, 0.5, INF, 1.0], obj=[1, 0, 2, 3, 4], points=np.stack([i[0] for i in items]),
                           pose=np.stack([i[1] for i in items]), iters=4, cull=0)
    cases["mixed"] = mixed_case()
    return cases


MIXED = ("normal", "few", "degenerate", "obj too large", "obj negative", "nan point", "normal again")


def mixed_case():
    """One call of the items ``MIXED``, 70 points each, 4 steps: a normal fit; five finite points (the rest NaN); one flat face; two bad
    objects; a normal fit with one NaN point; the first item once more."""
    rng = np.random.default_rng(77)
    br = m.bracket()
    normal, few, flat, nanp = fit_item(br, 70, rng), fit_item(br, 70, rng), flat_item(70, rng), fit_item(br, 70, rng)
    few[0][5:] = np.nan
    nanp[0][33, 1] = np.nan
    items = [normal, few, flat, normal, normal, nanp, normal]
    return dict(meshes=[br], max_dist=[INF], obj=[0, 0, 0, 1, -1, 0, 0], points=np.stack([i[0] for i in items]), pose=np.stack([i[1] for i in items]),
                iters=4, cull=0)


def run_case(case, iters=None):
    """The restatement on a case: (pose_out, stats)."""
    v, t, begin = concat_meshes(case["meshes"])
    return icp_np(v, t, begin, case["max_dist"], case["obj"], case["points"], case["pose"], case["iters"] if iters is None else iters, case["cull"])
