"""Which proper rotations map a CAD model onto itself, decided from its triangles.

A symmetric model renders byte-identical views for different poses, so its views must be trained and scored with ADD-S; YCB and LineMOD
ship that list by hand, a user's own PLY has none.  ``detect_symmetry`` tries a few hundred candidate rotations about a few candidate
axes through the surface centroid: every referenced vertex and ``samples`` area-weighted surface points are moved by the candidate and
their EXACT distance to the mesh is taken (``lib.mesh_distance.mesh_closest``: a point moved by a true symmetry lies on the surface
again, distance zero, whatever the sample spacing).  All candidates travel as the K transforms of one device call; everything around it
is deterministic numpy fp64 on the host.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import numpy as np

PROBE_ANGLE = 1.0            # radians: no finite order <= max_order has it, a surface of revolution passes it
MAX_VERTEX_QUERIES = 4096
NORMAL_GRID = 50             # face normals are merged on a grid of 1 / 50 per component
INT_MAX = 2 ** 31 - 1


@dataclass
class SymmetryReport:
    """``symmetric``: any candidate passed.  ``axes`` [A,3]: the candidate axes (unit, through ``centroid``): first the three principal
    axes of the surface, then the merged face normals.  ``passed``: rows (axis index, order (0 = the 1-radian probe), residual / D,
    colour residual or nan) of the candidates that passed.  ``residuals`` [A, orders]: residual / D of every candidate (the larger of its
    two directions), columns ``orders``.  ``D``: the diagonal of the bounding box."""
    symmetric: bool
    axes: np.ndarray
    passed: list
    D: float
    centroid: np.ndarray
    orders: list = field(default_factory=list)
    residuals: np.ndarray = None
    color_residuals: np.ndarray = None

    def __str__(self):
        head = "symmetric: %s   D %.6g   centroid (%.6g, %.6g, %.6g)   smallest residual / D %.3g" % (
            ("yes" if self.symmetric else "no",) + (self.D,) + tuple(self.centroid) + (float(np.nanmin(self.residuals)),))
        rows = []
        for a in sorted({p[0] for p in self.passed}):              # one row per axis: its orders, its largest residuals
            mine = [p for p in self.passed if p[0] == a]
            what = ", ".join(str(n) for _, n, _, _ in mine if n) + (" + revolution" if any(n == 0 for _, n, _, _ in mine) else "")
            cmax = max(c for _, _, _, c in mine)
            rows.append("  axis (%+.4f, %+.4f, %+.4f)  orders %s  residual / D <= %.3g%s" % (
                tuple(self.axes[a]) + (what, max(r for _, _, r, _ in mine), "" if math.isnan(cmax) else "  colour <= %.3g" % cmax)))
        return "\n".join([head] + rows)


def _kept(tri, V):
    return ((tri >= 0) & (tri < V)).all(axis=1) & (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])


def _fold(n):
    """Unit vectors with the sign chosen so that the component of largest magnitude is positive."""
    big = np.argmax(np.abs(n), axis=1)
    return n * np.where(n[np.arange(len(n)), big] < 0, -1.0, 1.0)[:, None]


def candidate_axes(a, b, c, area, centroid, axes):
    """The three eigenvectors of the exact surface covariance, then up to ``axes`` merged face normals (largest summed area first) that
    are not within about a degree of an axis already listed."""
    a0, b0, c0 = a - centroid, b - centroid, c - centroid
    S = a0 + b0 + c0
    cov = sum(np.einsum("t,ti,tj->ij", area / 12.0, x, x) for x in (a0, b0, c0, S))
    out = list(_fold(np.linalg.eigh(cov)[1].T.copy()))
    n = np.cross(b - a, c - a)
    ok = area > 0
    unit = _fold(n[ok] / (2.0 * area[ok])[:, None])
    keys = np.rint(unit * NORMAL_GRID).astype(np.int64)
    merged = {}
    for key, u, w in zip(map(tuple, keys.tolist()), unit, area[ok]):
        s = merged.setdefault(key, [0.0, np.zeros(3)])
        s[0] += w
        s[1] += w * u
    total = float(area.sum())
    taken = 0
    for key, (w, u) in sorted(merged.items(), key=lambda kv: (-round(kv[1][0] / total, 9), kv[0])):
        if taken >= axes:
            break
        norm = math.sqrt(float(u @ u))
        if norm == 0:
            continue
        u = u / norm
        if all(abs(float(u @ o)) < 0.99985 for o in out):
            out.append(u)
            taken += 1
    return np.array(out)


def rotation_about(axis, angle, center):
    """[R | c - R c] (3 x 4): the rotation by ``angle`` about the unit ``axis`` through ``center`` (Rodrigues)."""
    x, y, z = axis
    Kx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    R = np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)
    return np.concatenate([R, (center - R @ center)[:, None]], axis=1)


def _device_closest(vertices, triangles, points, xf, want_closest=True, accel=False):
    import torch
    from ...lib.mesh_distance import mesh_closest
    up = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (vertices, triangles, points, xf)]
    tree = None
    if accel:
        from ...lib.mesh_set import MeshTree
        tree = MeshTree(vertices, triangles)                    # from the host arrays: no download
    d2, tri, closest = mesh_closest(*up, want_closest=want_closest, accel=accel, tree=tree)
    return d2.cpu().numpy(), tri.cpu().numpy(), closest.cpu().numpy() if want_closest else None


def _barycentric(p, A, B, C):
    """Weights of p (on or near triangle ABC) clamped to the triangle; a degenerate triangle gives its nearest corner."""
    v0, v1, v2 = B - A, C - A, p - A
    d00, d01, d11 = (v0 * v0).sum(-1), (v0 * v1).sum(-1), (v1 * v1).sum(-1)
    d20, d21 = (v2 * v0).sum(-1), (v2 * v1).sum(-1)
    den = d00 * d11 - d01 * d01
    good = den > 1e-30 * np.maximum(d00 * d11, 1e-300)
    with np.errstate(all="ignore"):
        w1 = np.where(good, (d11 * d20 - d01 * d21) / den, 0.0)
        w2 = np.where(good, (d00 * d21 - d01 * d20) / den, 0.0)
    w = np.clip(np.stack([1.0 - w1 - w2, w1, w2], axis=-1), 0.0, 1.0)
    near = np.argmin(np.stack([((p - X) ** 2).sum(-1) for X in (A, B, C)], axis=-1), axis=-1)
    w = np.where(good[..., None], w, np.eye(3)[near])
    return w / w.sum(-1, keepdims=True)


def detect_symmetry(vertices, triangles, colors=None, *, tol=0.01, color_tol=8.0, max_order=12, axes=10, samples=2048, seed=0, closest=None,
                    accel=False):
    """vertices [V,3] (read as fp32, like the renderers), triangles [T,3], colors [V,3] 8-bit levels or None -> ``SymmetryReport``.

    Candidates: per axis (``candidate_axes``) the angles 2 pi / n, n = 2..``max_order``, and 1 radian, each in both directions; a
    candidate passes when both directions pass.  Queries: the referenced vertices (every ceil(n / 4096)-th above 4096) and ``samples``
    area-weighted surface points from ``np.random.RandomState(seed)`` (the global ``np.random`` stream is never touched).  Geometry: the
    largest distance of a moved query to the mesh is at most ``tol`` x D.  Colour (with ``colors``): over the surface samples, the mean
    absolute channel difference between the sample's interpolated vertex colour and the colour interpolated at its closest point is at
    most ``color_tol`` on average; vertex queries take no part (a vertex duplicated per face has no single colour at a corner).

    ``tol``, ``color_tol`` and ``max_order`` are the user's choices, not measurements: 1 % of the diameter is the order of a coarse
    tessellator's chord error and below the depth noise of the sensor model; eight 8-bit levels is below the training colour jitter.
    ``closest``: a callable (vertices fp32, triangles int32, points fp64, xf [K,3,4] fp64, want_closest) -> numpy (dist2, tri, closest)
    in place of the device call.  ``accel``: the device call goes through the mesh's bounding-box tree (``df_mesh_closest_tree``): the same
    distances byte for byte, so the same report.  Not found: axes at an unknown angle inside a degenerate principal plane that are no face normal,
    orders above ``max_order`` short of a surface of revolution, improper symmetries (a pose cannot express them)."""
    v32 = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32).reshape(-1, 3))
    v = v32.astype(np.float64)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    if int(max_order) < 2 or int(axes) < 0 or int(samples) < 1 or not tol > 0:
        raise ValueError("detect_symmetry: need max_order >= 2, axes >= 0, samples >= 1, tol > 0")
    if len(tri) and (np.abs(tri) > INT_MAX).any():
        raise ValueError("detect_symmetry: triangle indices must fit an int32")
    tk = tri[_kept(tri, len(v))] if len(tri) else tri
    if len(tk) == 0:
        raise ValueError("detect_symmetry: the model has no valid triangle")
    a, b, c = v[tk[:, 0]], v[tk[:, 1]], v[tk[:, 2]]
    area = 0.5 * np.sqrt((np.cross(b - a, c - a) ** 2).sum(axis=1))
    total = float(area.sum())
    if not (total > 0 and math.isfinite(total)):
        raise ValueError("detect_symmetry: the model has no surface")
    centroid = (area[:, None] * (a + b + c) / 3.0).sum(axis=0) / total
    ref = np.unique(tk)
    D = float(np.sqrt(((v[ref].max(axis=0) - v[ref].min(axis=0)) ** 2).sum()))
    ax = candidate_axes(a, b, c, area, centroid, int(axes))
    orders = list(range(2, int(max_order) + 1)) + [0]
    xf = np.array([rotation_about(u, sgn * (2 * math.pi / n if n else PROBE_ANGLE), centroid) for u in ax for n in orders for sgn in (1.0, -1.0)])
    # queries: vertices first, then the surface samples (their triangle and weights kept for the colour test)
    vq = ref[::max(1, -(-len(ref) // MAX_VERTEX_QUERIES))] if len(ref) > MAX_VERTEX_QUERIES else ref
    rs = np.random.RandomState(seed)
    pick = np.minimum(np.searchsorted(np.cumsum(area) / total, rs.random_sample(int(samples)), side="right"), len(tk) - 1)
    su, r2 = np.sqrt(rs.random_sample(int(samples))), rs.random_sample(int(samples))
    w = np.stack([1.0 - su, su * (1.0 - r2), su * r2], axis=1)
    sp = w[:, 0:1] * a[pick] + w[:, 1:2] * b[pick] + w[:, 2:3] * c[pick]
    points = np.ascontiguousarray(np.concatenate([v[vq], sp]))
    nv, P, K = len(vq), len(vq) + int(samples), len(xf)
    fn = closest if closest is not None else (functools.partial(_device_closest, accel=True) if accel else _device_closest)
    want = colors is not None
    kstep = max(1, min(K, INT_MAX // (3 * P)))
    parts = [fn(v32, np.ascontiguousarray(tri.astype(np.int32)), points, np.ascontiguousarray(xf[k0:k0 + kstep]), want) for k0 in range(0, K, kstep)]
    d2, wt = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    with np.errstate(invalid="ignore"):
        res = np.sqrt(d2.max(axis=1)) / D                                    # inf where a query found no triangle, nan from a nan
    res = np.where(np.isnan(res) | (wt < 0).any(axis=1), np.inf, res)
    cres = np.full(K, np.nan)
    if want:
        col = np.asarray(colors, dtype=np.float64).reshape(len(v), 3)
        cp = np.concatenate([p[2] for p in parts])[:, nv:]
        t = tri[np.maximum(wt[:, nv:], 0)]                                   # [K,S,3] vertex indices of the winning triangles
        own = w[:, 0:1] * col[tk[pick, 0]] + w[:, 1:2] * col[tk[pick, 1]] + w[:, 2:3] * col[tk[pick, 2]]
        for k in np.nonzero(res <= tol)[0]:                                  # colour matters only where the geometry passes
            wb = _barycentric(cp[k], v[t[k, :, 0]], v[t[k, :, 1]], v[t[k, :, 2]])
            there = wb[:, 0:1] * col[t[k, :, 0]] + wb[:, 1:2] * col[t[k, :, 1]] + wb[:, 2:3] * col[t[k, :, 2]]
            cres[k] = float(np.abs(own - there).mean())
    res2, cres2 = res.reshape(len(ax), len(orders), 2).max(axis=2), cres.reshape(len(ax), len(orders), 2)
    cmax = cres2.max(axis=2)                                                 # nan unless both directions passed the geometry
    passed = []
    for i in range(len(ax)):
        for j, n in enumerate(orders):
            if res2[i, j] <= tol and (not want or cmax[i, j] <= color_tol):
                passed.append((i, n, float(res2[i, j]), float(cmax[i, j]) if want else float("nan")))
    return SymmetryReport(symmetric=bool(passed), axes=ax, passed=passed, D=D, centroid=centroid, orders=orders, residuals=res2,
                          color_residuals=cmax if want else None)


# ---- the rotations themselves: the symmetry set the BOP pose errors take their minimum over (lib/pose_error.py) ---------------------------
SET_EQUAL = 1e-6             # two rotations are the same element when every entry of R agrees within this
SET_SNAP = 1e-9
PERPENDICULAR = 0.05        # |a . b| of a half-turn axis b that counts as perpendicular to a revolution axis a


def _matmul(A, B):
    """A B for 3 x 3, every entry (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j]: the same bytes wherever it runs."""
    return (A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :]) + A[:, 2:3] * B[2:3, :]


def is_revolution(report):
    """A 1-radian probe passed: ``symmetry_set`` takes the model as a surface of revolution (a polygon of many sides, or a hexagon at a
    loose tolerance, passes it too: the tools say which models were taken so)."""
    return any(int(n) == 0 for _, n, _, _ in report.passed)


def symmetry_generators(report, step=0.01):
    """The rotations [3,3] that generate a report's symmetry set, in report order.  Without a surface of revolution: the rotation by
    2 pi / n of every passed (axis, n > 0).  With one (a passed 1-radian probe; the first such axis, a): the rotation by 2 pi / N about
    a, N = ceil(pi / ``step``) (the BOP discretisation of a continuous symmetry: 315 at 0.01); the finite orders that passed on a itself
    are rotations of that continuous group and are dropped; of the half turns (n = 2) that passed on axes perpendicular to a
    (|a . b| <= 0.05) only the first is kept, about the part of b perpendicular to a: every other is that one followed by a rotation about
    a, which the discretisation already stands for.  Whatever else passed stays a generator (a second revolution axis, a sphere: such a
    set does not close below the cap)."""
    if not step > 0:
        raise ValueError("symmetry_set: step must be > 0")
    axes = np.asarray(report.axes, dtype=np.float64)
    rev = next((int(i) for i, n, _, _ in report.passed if n == 0), None)
    gens, flipped = [], False
    for i, n, _, _ in report.passed:
        i, n, b = int(i), int(n), axes[int(i)]
        if rev is None:
            if n > 0:
                gens.append(rotation_about(b, 2 * math.pi / n, np.zeros(3))[:, :3])
            continue
        a = axes[rev]
        if i == rev:
            if n == 0:
                gens.append(rotation_about(a, 2 * math.pi / math.ceil(math.pi / step), np.zeros(3))[:, :3])
        elif n == 2 and abs(float(a @ b)) <= PERPENDICULAR:
            if not flipped:
                p = b - float(a @ b) * a
                gens.append(rotation_about(p / math.sqrt(float(p @ p)), math.pi, np.zeros(3))[:, :3])
                flipped = True
        elif n == 0:
            gens.append(rotation_about(b, 2 * math.pi / math.ceil(math.pi / step), np.zeros(3))[:, :3])
        else:
            gens.append(rotation_about(b, 2 * math.pi / n, np.zeros(3))[:, :3])
    return gens


def symmetry_set(report, step=0.01, cap=4096, name="the model"):
    """float64 [S,3,4]: the proper rotations [R | c - R c] about ``report.centroid`` that map the model onto itself, the identity first.

    The set is the closure of ``symmetry_generators(report, step)`` under composition, searched breadth first from the identity: every
    element found, in order of discovery, is multiplied from the left by every generator in report order, and a product is new when no
    element found so far agrees with it within 1e-6 in every entry of R.  The set is listed in order of discovery, so it is a pure
    function of the report: two calls give equal bytes.  A set that reaches ``cap`` elements before it closes raises ``ValueError`` with
    ``name`` in it: a set that is not closed is not a group, and a minimum over it would depend on the order.  A model that is not
    symmetric gives the identity alone."""
    cap = int(cap)
    if cap < 1:
        raise ValueError("symmetry_set: cap must be >= 1")
    gens = symmetry_generators(report, step)
    found = np.zeros((cap, 3, 3))
    found[0] = np.eye(3)
    n, at = 1, 0
    while at < n:
        for g in gens:
            R = _matmul(g, found[at])
            if (np.abs(found[:n] - R).reshape(n, 9).max(axis=1) <= SET_EQUAL).any():
                continue
            if n == cap:
                raise ValueError("symmetry_set: the symmetries of %s do not close within %d rotations (a sphere, two revolution axes or "
                                 "a tolerance that passes rotations the model does not have): not a group, no minimum to take" % (name, cap))
            found[n] = R
            n += 1
        at += 1
    c = np.asarray(report.centroid, dtype=np.float64).reshape(3)
    out = np.zeros((n, 3, 4))
    # an entry within 1e-9 of -1, 0 or 1 is that value (far inside the set's own equality): the half and quarter turns about the
    # coordinate axes come out as the exact signed permutations they are, free of sin(pi)'s 1e-16
    snap = np.rint(found[:n])
    found[:n] = np.where(np.abs(found[:n] - snap) <= SET_SNAP, snap, found[:n])
    out[:, :, :3] = found[:n]
    out[:, :, 3] = c[None, :] - ((found[:n, :, 0] * c[0] + found[:n, :, 1] * c[1]) + found[:n, :, 2] * c[2])
    return out


# ---- the option the tools share -------------------------------------------------------------------------------------------------------------
def add_sym_arguments(ap):
    ap.add_argument("--cad_sym", type=str, nargs="+", default=["none"], metavar="none|auto|ID",
                    help="which models are trained and scored with ADD-S: none, auto (detect_symmetry per model) or model indices (0 = the first --cad_model)")
    ap.add_argument("--cad_sym_tol", type=float, default=0.01, help="auto: the largest residual of a symmetry, as a fraction of the model's bounding-box diagonal")
    ap.add_argument("--cad_sym_accel", action="store_true", help="auto: find the distances through each model's bounding-box tree (the same result, faster on large meshes)")


def parse_sym_option(values):
    """``--cad_sym`` -> "none", "auto" or a list of model indices; ``ValueError`` for anything else."""
    values = [values] if isinstance(values, str) else list(values)
    if values in (["none"], ["auto"]):
        return values[0]
    try:
        return sorted({int(x) for x in values})
    except (TypeError, ValueError):
        raise ValueError("--cad_sym is none, auto or a list of model indices, got %r" % (values,))
