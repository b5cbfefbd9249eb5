"""The rule of df_mesh_closest (include/dfusion.h, steps M1, M2, Q1, D1..D5) restated twice -- ``closest_np`` vectorised in numpy,
``closest_scalar`` pair by pair in plain Python floats -- and the meshes the tests share.  Every product, sum and difference below is
one IEEE fp64 operation in the order the header writes; nothing is fused."""
import math

import numpy as np

from cad_raster_np import icosphere  # noqa: F401  (a fixture of the tests that import this module)

INF, NAN = float("inf"), float("nan")


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------
def box(a, b, c, center=(0.0, 0.0, 0.0)):
    """(vertices float32 [24,3], triangles int32 [12,3]) of the a x b x c box about ``center``: four vertices per face, wound
    counter-clockwise seen from outside."""
    h = np.array([a, b, c], dtype=np.float64) / 2
    verts, tris = [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            quad = []
            for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = np.zeros(3)
                p[axis], p[u], p[v] = sign * h[axis], su * h[u], sv * h[v]
                quad.append(p + np.asarray(center, dtype=np.float64))
            if sign < 0:
                quad = quad[::-1]
            n = len(verts)
            verts += quad
            tris += [[n, n + 1, n + 2], [n, n + 2, n + 3]]
    return np.array(verts, dtype=np.float32), np.array(tris, dtype=np.int32)


def prism(n, r, h):
    """A regular n-gon prism of circumradius r and height h about the z axis through the origin: per-face vertices, the caps as fans
    about their centres.  4 n triangles."""
    ang = 2 * np.pi * np.arange(n) / n
    ring = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1)
    verts, tris = [], []
    for z, flip in ((h / 2, False), (-h / 2, True)):
        base = len(verts)
        verts.append([0.0, 0.0, z])
        verts += [[x, y, z] for x, y in ring]
        for i in range(n):
            j = (i + 1) % n
            tris.append([base, base + 1 + j, base + 1 + i] if flip else [base, base + 1 + i, base + 1 + j])
    for i in range(n):
        j = (i + 1) % n
        base = len(verts)
        verts += [[ring[i][0], ring[i][1], -h / 2], [ring[j][0], ring[j][1], -h / 2], [ring[j][0], ring[j][1], h / 2], [ring[i][0], ring[i][1], h / 2]]
        tris += [[base, base + 1, base + 2], [base, base + 2, base + 3]]
    return np.array(verts, dtype=np.float32), np.array(tris, dtype=np.int32)


def merge(*meshes):
    verts, tris, n = [], [], 0
    for v, t in meshes:
        verts.append(np.asarray(v, dtype=np.float32))
        tris.append(np.asarray(t, dtype=np.int32) + n)
        n += len(v)
    return np.concatenate(verts), np.concatenate(tris)


def bracket():
    """box(1, 2, 3) with a 0.3 cube about (.5, .8, 1.2): it sticks 0.15 out of the +x face, off every axis."""
    return merge(box(1, 2, 3), box(.3, .3, .3, center=(.5, .8, 1.2)))


def scalene_tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [.2, 1.3, 0], [.3, .4, .9]], dtype=np.float32)
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int32)


def regular_tetrahedron():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float32)
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)


# ---- vectorised ----------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def kept_triangles(triangles, V):
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    return ((t >= 0) & (t < V)).all(axis=1) & (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])


def prepare_np(vertices, triangles):
    """M1, M2: dict of U [T,3,3] (A, B, C), e [T,3,3] (AB, BC, CA), iee [T,3], e2, n [T,3], nn, inn [T]; NaN rows for dropped triangles."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    kept = kept_triangles(t, len(v))
    U = v[np.where(kept[:, None], t, 0)].astype(np.float64)
    with np.errstate(all="ignore"):
        e = U[:, [1, 2, 0]] - U
        ee = _dot(e, e)
        iee = np.where(ee > 0, 1.0 / ee, 0.0)
        e2 = U[:, 2] - U[:, 0]
        n = _cross(e[:, 0], e2)
        nn = _dot(n, n)
        inn = np.where(nn > 0, 1.0 / nn, 0.0)
    rec = dict(U=U, e=e, iee=iee, e2=e2, n=n, nn=nn, inn=inn)
    for a in rec.values():
        a[~kept] = NAN
    return rec


def transform_np(points, xf):
    """Q1: q [K,P,3]."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    X = np.asarray(xf, dtype=np.float64).reshape(-1, 3, 4)
    with np.errstate(all="ignore"):
        return np.stack([((X[:, None, j, 0] * p[None, :, 0] + X[:, None, j, 1] * p[None, :, 1]) + X[:, None, j, 2] * p[None, :, 2])
                         + X[:, None, j, 3] for j in range(3)], axis=-1)


def _pair(rec, q, want_c=True):
    """D1..D3 for broadcastable records and queries (q [...,3]): d_t, the candidate that gave it (0..2 edges, 3 face, -1 none), and
    (with ``want_c``) its closest point."""
    d = np.full(np.broadcast_shapes(q.shape[:-1], rec["nn"].shape), INF)
    which = np.full(d.shape, -1, dtype=np.int64)
    c = np.broadcast_to(q, d.shape + (3,)).copy() if want_c else None
    with np.errstate(all="ignore"):
        for k in range(3):
            U, e, iee = rec["U"][..., k, :], rec["e"][..., k, :], rec["iee"][..., k]
            w = q - U
            s = _dot(w, e) * iee
            s = np.where(s < 0, 0.0, np.where(s > 1, 1.0, s))
            r = w - s[..., None] * e
            dk = _dot(r, r)
            take = dk < d
            d, which = np.where(take, dk, d), np.where(take, k, which)
            if want_c:
                c = np.where(take[..., None], U + s[..., None] * e, c)
        w = q - rec["U"][..., 0, :]
        n = rec["n"]
        u, v = _dot(_cross(rec["e"][..., 0, :], w), n), _dot(_cross(w, rec["e2"]), n)
        inside = (rec["nn"] > 0) & (u >= 0) & (v >= 0) & (u + v <= rec["nn"])
        h = _dot(w, n)
        df = np.where(inside, (h * h) * rec["inn"], INF)
        take = df < d
        d, which = np.where(take, df, d), np.where(take, 3, which)
        if want_c:
            c = np.where(take[..., None], q - (h * rec["inn"])[..., None] * n, c)
    return d, which, c


def closest_np(vertices, triangles, points, xf, want_closest=True, pairs_per_step=1 << 18):
    """(dist2 [K,P] float64, tri [K,P] int32, closest [K,P,3] float64 or None) by M1..D5."""
    rec = prepare_np(vertices, triangles)
    T = len(rec["nn"])
    q = transform_np(points, xf)
    K, P = q.shape[:2]
    qf = q.reshape(-1, 3)
    best = np.full(len(qf), INF)
    bt = np.full(len(qf), -1, dtype=np.int64)
    tstep = max(1, min(T, 64))
    qstep = max(1, pairs_per_step // tstep)
    for q0 in range(0, len(qf), qstep):
        qq = qf[q0:q0 + qstep, None, :]
        for t0 in range(0, T, tstep):
            sub = {k: a[None, t0:t0 + tstep] for k, a in rec.items()}
            d = _pair(sub, qq, False)[0]                                  # no NaN in d: a NaN is never taken
            i = np.argmin(d, axis=1)                                # the first smallest
            dm = d[np.arange(len(i)), i]
            win = dm < best[q0:q0 + qstep]                          # ascending t: the lowest index keeps a tie; +inf never wins
            best[q0:q0 + qstep] = np.where(win, dm, best[q0:q0 + qstep])
            bt[q0:q0 + qstep] = np.where(win, t0 + i, bt[q0:q0 + qstep])
    closest = None
    if want_closest:
        closest = qf.copy()
        has = bt >= 0
        if has.any():
            sub = {k: a[bt[has]] for k, a in rec.items()}
            closest[has] = _pair(sub, qf[has])[2]
        closest = closest.reshape(K, P, 3)
    return best.reshape(K, P), bt.astype(np.int32).reshape(K, P), closest


# ---- pair by pair, plain Python floats -----------------------------------------------------------------------------------------------------
def _sdot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _scross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _ssub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def prepare_scalar(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    V, recs = len(v), []
    for i0, i1, i2 in np.asarray(triangles, dtype=np.int64).reshape(-1, 3).tolist():
        if not (0 <= i0 < V and 0 <= i1 < V and 0 <= i2 < V) or i0 == i1 or i1 == i2 or i0 == i2:
            recs.append(None)
            continue
        U = [[float(x) for x in v[i]] for i in (i0, i1, i2)]
        e = [_ssub(U[(k + 1) % 3], U[k]) for k in range(3)]
        iee = []
        for k in range(3):
            ee = _sdot(e[k], e[k])
            iee.append(1.0 / ee if ee > 0 else 0.0)
        e2 = _ssub(U[2], U[0])
        n = _scross(e[0], e2)
        nn = _sdot(n, n)
        recs.append(dict(U=U, e=e, iee=iee, e2=e2, n=n, nn=nn, inn=1.0 / nn if nn > 0 else 0.0))
    return recs


def pair_scalar(r, q):
    """D1..D3 of one pair: (d_t, closest point); d_t = +inf when no candidate is taken."""
    d, c = INF, list(q)
    for k in range(3):
        U, e = r["U"][k], r["e"][k]
        w = _ssub(q, U)
        s = _sdot(w, e) * r["iee"][k]
        s = 0.0 if s < 0 else (1.0 if s > 1 else s)
        rr = [w[j] - s * e[j] for j in range(3)]
        dk = _sdot(rr, rr)
        if dk < d:
            d, c = dk, [U[j] + s * e[j] for j in range(3)]
    if r["nn"] > 0:
        w = _ssub(q, r["U"][0])
        u, v = _sdot(_scross(r["e"][0], w), r["n"]), _sdot(_scross(w, r["e2"]), r["n"])
        if u >= 0 and v >= 0 and u + v <= r["nn"]:
            h = _sdot(w, r["n"])
            df = (h * h) * r["inn"]
            if df < d:
                g = h * r["inn"]
                d, c = df, [q[j] - g * r["n"][j] for j in range(3)]
    return d, c


def closest_scalar(vertices, triangles, points, xf, want_closest=True):
    recs = prepare_scalar(vertices, triangles)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3).tolist()
    X = np.asarray(xf, dtype=np.float64).reshape(-1, 3, 4).tolist()
    K, P = len(X), len(p)
    dist2, tri, closest = np.full((K, P), INF), np.full((K, P), -1, dtype=np.int32), np.zeros((K, P, 3))
    for k in range(K):
        for i in range(P):
            q = [((X[k][j][0] * p[i][0] + X[k][j][1] * p[i][1]) + X[k][j][2] * p[i][2]) + X[k][j][3] for j in range(3)]
            best, bt, bc = INF, -1, q
            for t, r in enumerate(recs):
                if r is None:
                    continue
                d, c = pair_scalar(r, q)
                if d < best:
                    best, bt, bc = d, t, c
            dist2[k, i], tri[k, i], closest[k, i] = best, bt, bc
    return dist2, tri, (closest if want_closest else None)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rotation_xf(axis, angle, center=(0, 0, 0)):
    """[R | c - R c]: the rotation by ``angle`` about ``axis`` through ``center`` as a 3 x 4."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / math.sqrt(float(a @ a))
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)
    c = np.asarray(center, dtype=np.float64)
    return np.concatenate([R, (c - R @ c)[:, None]], axis=1)


# ---- the shapes both test files walk -------------------------------------------------------------------------------------------------------
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
SPLIT_QUERIES = 128            # the queries of a workgroup whose waves share them (64 lanes x 2)
WHOLE_QUERIES = 512            # the queries of a workgroup whose 256 lanes own different ones


def three_xf():
    return np.stack([IDENTITY, rotation_xf((1, 2, 3), 0.7), rotation_xf((0, 0, 1), 2.0, center=(.1, -.2, .3)) + np.array([[0, 0, 0, .05]] * 3)])


def far_mesh_with_near_last(T, seed):
    """T small triangles, all on a shell of radius 5..6 except the last, which lies near the origin: it wins for queries near the origin."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(T, 3))
    centre = d / np.sqrt((d * d).sum(axis=1, keepdims=True)) * rng.uniform(5, 6, (T, 1))
    centre[-1] = (.1, .05, -.1)
    v = (centre[:, None, :] + rng.uniform(-.3, .3, (T, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * T, dtype=np.int32).reshape(T, 3)


def region_case():
    """One triangle and a query for the face and for each of its six outer regions, with the closest point each must get."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    q = np.array([[.25, .25, .5], [.5, -.5, .3], [1, 1, .2], [-.5, .5, -.1], [-1, -1, .2], [2, -.5, 0], [-.5, 2, .1]])
    want = np.array([[.25, .25, 0], [.5, 0, 0], [.5, .5, 0], [0, .5, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0]])
    return v, np.array([[0, 1, 2]], dtype=np.int32), q, want


def shared_edge_case():
    """Two triangles sharing the edge 1-2; queries on a shared vertex, on the shared edge, inside face 0, inside face 1."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.float32)
    q = np.array([[1, 0, 0], [.5, .5, 0], [.25, .25, 0], [.75, .75, 0]])
    return v, np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32), q, np.array([0, 0, 0, 1], dtype=np.int32)


def degenerate_mesh():
    """V = 6.  Triangles: an index of V, a negative index, a repeated index (all dropped); a collinear one (edges only); one whose two
    distinct indices 4, 5 name equal coordinates (iee = 0 on that edge, no face); one good triangle far away."""
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 3, 1], [.5, .5, .5], [.5, .5, .5]], dtype=np.float32)
    t = np.array([[0, 1, 6], [-1, 0, 1], [0, 0, 1], [0, 1, 2], [0, 4, 5], [3, 1, 0]], dtype=np.int32)
    return v, t


def make_cases(tile):
    """name -> (vertices, triangles, points, xf): every shape of the list in the GPU test's docstring."""
    rng = np.random.default_rng(7)
    cases = {}
    for T in (1, tile - 1, tile, tile + 1):
        v, t = far_mesh_with_near_last(T, 100 + T)
        cases["T%d" % T] = (v, t, rng.uniform(-.5, .5, (65, 3)), IDENTITY[None])
    bv, bt = bracket()
    for P in (1, 63, 64, 65, SPLIT_QUERIES + 1, WHOLE_QUERIES + 1):
        pts = rng.uniform(-1, 1, (P, 3)) * np.array([1.0, 1.5, 2.0])
        cases["P%d_K1" % P] = (bv, bt, pts, three_xf()[1:2])
        cases["P%d_K3" % P] = (bv, bt, pts, three_xf())
    v, t, q, _ = region_case()
    cases["regions"] = (v, t, q, IDENTITY[None])
    v, t, q, _ = shared_edge_case()
    cases["shared_edge"] = (v, t, q, IDENTITY[None])
    dv, dt = degenerate_mesh()
    near = np.array([[.5, .5, .5], [1.5, 0, 0], [1.5, .2, 0], [.25, .25, .25], [0, 3, 1]])
    cases["degenerate"] = (dv, dt, np.concatenate([near, rng.uniform(-1, 3, (40, 3))]), three_xf())
    cases["all_dropped"] = (dv, dt[:3], rng.uniform(-1, 1, (5, 3)), three_xf())
    return cases


def whole_path_case(tile):
    """Enough transforms (256 workgroups' worth) that every lane of a workgroup owns its own queries, on T = tile + 1 triangles."""
    rng = np.random.default_rng(11)
    v, t = far_mesh_with_near_last(tile + 1, 55)
    ang = rng.uniform(0, 6.28, 256)
    xf = np.stack([rotation_xf(rng.normal(size=3), a) for a in ang])
    return v, t, rng.uniform(-6, 6, (65, 3)), xf
