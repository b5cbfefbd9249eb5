"""Views of a coloured CAD cloud (``df_cad_render``), a triangle mesh (``df_cad_render_mesh``) or a scene of several meshes that occlude
each other (``df_cad_render_scene``) as customCAD training frames, rendered on the device -- the job of the reference's
unfinished Unity-free generator datasets/customCAD/cad_to_dataset.py (needs open3d and cv2, uses ``np.float`` / ``np.int``, stops after 50
test images), of mask_generator.py and of train_test_generator.py, for the tree ``dataset.py`` of this directory reads.

Kept from the reference: the draws of one view (``get_perspective_data_from_model_seed``, :264-276, then ``augment_pointcloud``,
:145-160) in their order on ``np.random.seed(seed)``; rotation about the model's centroid followed by moving the centroid to the drawn
position (open3d's ``rotate`` and ``translate(relative=False)``, :71-73); the skip of views with too few pixels (:219-221); the
half-open box mask (mask_generator.py:21-28); the 80 / 20 split of shuffled frame numbers (train_test_generator.py:17-28).

Different by design (DESIGN.md "customCAD renderer"): the camera is the loader's projection matrix and the depth is Unity's 16-bit
non-linear code, not the pinhole / millimetre images of :181-188,236; the facing test uses each point's own view ray; depth and colour
share one winner; a hole is a plain radius test around the drawn point.  Nothing here is checked against open3d or OpenCV, which this
build does not have: ``sample_view`` is pinned by restatement only.
"""
from __future__ import annotations

import numpy as np
import torch
from scipy.spatial.transform import Rotation

from ...lib import preprocess as pp
from .dataset import _PLY_TYPES, Y_180, convert_quat

MASK_MODES = {"box": 0, "pixels": 1}


def _read_ply_elements(path):
    """{element: {property: array}} plus the triangles of an ASCII or binary little-endian PLY (polygons are cut into fans)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a ply file")
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: no end_header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                elements[-1][2].append((tok[-1], tok[2:4]) if tok[1] == "list" else (tok[-1], tok[1]))
            elif tok[0] == "end_header":
                break
        if fmt not in ("ascii", "binary_little_endian"):
            raise ValueError(f"{path}: unsupported ply format {fmt!r}")
        data, faces = {}, []
        for name, count, props in elements:
            has_list = any(isinstance(t, list) for _, t in props)
            if not has_list:
                dt = np.dtype([(p, "<" + _PLY_TYPES[t]) for p, t in props])
                if fmt == "ascii":
                    rows = np.array([[float(x) for x in f.readline().split()] for _ in range(count)], dtype=np.float64).reshape(count, len(props))
                    data[name] = {p: rows[:, k].astype(dt[k]) for k, (p, _) in enumerate(props)}
                else:
                    rec = np.frombuffer(f.read(count * dt.itemsize), dtype=dt, count=count)
                    data[name] = {p: rec[p] for p, _ in props}
                continue
            for _ in range(count):
                if fmt == "ascii":
                    r = f.readline().split()
                    if name == "face":
                        faces.append([int(v) for v in r[1:1 + int(r[0])]])
                    continue
                for p, t in props:
                    if isinstance(t, list):
                        ct, it = np.dtype("<" + _PLY_TYPES[t[0]]), np.dtype("<" + _PLY_TYPES[t[1]])
                        k = int(np.frombuffer(f.read(ct.itemsize), dtype=ct)[0])
                        vals = np.frombuffer(f.read(k * it.itemsize), dtype=it)
                        if name == "face" and p in ("vertex_indices", "vertex_index"):
                            faces.append(vals.astype(np.int64).tolist())
                    else:
                        f.read(np.dtype(_PLY_TYPES[t]).itemsize)
    tris = [[poly[0], poly[j], poly[j + 1]] for poly in faces for j in range(1, len(poly) - 1)]
    return data, np.asarray(tris, dtype=np.int64).reshape(-1, 3)


def read_colored_ply(path, n_points=None):
    """(points float32 [n,3], normals float32 [n,3] or None, colours uint8 [n,3]) of an ASCII or binary little-endian PLY with
    ``red green blue`` (and optionally ``nx ny nz``) vertex properties.  A file without colours comes back mid-grey.  A vertex-only file
    returns its vertices as they are.  A mesh needs ``n_points``: that many points drawn over the surface with ``np.random`` the way
    ``ply_vtx`` draws positions (triangle by area, uniform barycentric coordinates), each with its face's normal and the barycentric mix
    of its corners' colours -- the job of open3d's ``sample_points_uniformly``, not its stream."""
    data, tris = _read_ply_elements(path)
    v = data.get("vertex")
    if v is None or not all(a in v for a in "xyz"):
        raise ValueError(f"{path}: no vertex positions")
    pts = np.stack([v[a].astype(np.float64) for a in "xyz"], axis=1)
    col = (np.stack([v[a].astype(np.float64) for a in ("red", "green", "blue")], axis=1) if all(a in v for a in ("red", "green", "blue"))
           else np.full(pts.shape, 128.0))
    nrm = np.stack([v[a].astype(np.float64) for a in ("nx", "ny", "nz")], axis=1) if all(a in v for a in ("nx", "ny", "nz")) else None
    if len(tris) and n_points is not None:
        a, b, c = pts[tris[:, 0]], pts[tris[:, 1]], pts[tris[:, 2]]
        cross = np.cross(b - a, c - a)
        area = 0.5 * np.linalg.norm(cross, axis=1)
        t = np.random.choice(len(tris), n_points, p=area / area.sum())
        r1, r2 = np.sqrt(np.random.random(n_points))[:, None], np.random.random(n_points)[:, None]
        w = ((1.0 - r1), r1 * (1.0 - r2), r1 * r2)
        pts = w[0] * a[t] + w[1] * b[t] + w[2] * c[t]
        col = w[0] * col[tris[t, 0]] + w[1] * col[tris[t, 1]] + w[2] * col[tris[t, 2]]
        nrm = cross[t] / np.maximum(2.0 * area[t], 1e-300)[:, None]
    elif len(tris):
        raise ValueError(f"{path}: a mesh needs n_points")
    return (np.ascontiguousarray(pts, dtype=np.float32), None if nrm is None else np.ascontiguousarray(nrm, dtype=np.float32),
            np.ascontiguousarray(np.clip(np.rint(col), 0, 255), dtype=np.uint8))


def read_colored_mesh(path):
    """(vertices float32 [V,3], triangles int32 [T,3], colours uint8 [V,3]) of an ASCII or binary little-endian PLY mesh, for
    ``CadMeshRenderer``: polygons are cut into fans as ``read_ply`` does, a file without ``red green blue`` comes back mid-grey.
    A file without faces returns T = 0."""
    data, tris = _read_ply_elements(path)
    v = data.get("vertex")
    if v is None or not all(a in v for a in "xyz"):
        raise ValueError(f"{path}: no vertex positions")
    pts = np.stack([v[a].astype(np.float64) for a in "xyz"], axis=1)
    col = (np.stack([v[a].astype(np.float64) for a in ("red", "green", "blue")], axis=1) if all(a in v for a in ("red", "green", "blue"))
           else np.full(pts.shape, 128.0))
    return (np.ascontiguousarray(pts, dtype=np.float32), np.ascontiguousarray(tris, dtype=np.int32),
            np.ascontiguousarray(np.clip(np.rint(col), 0, 255), dtype=np.uint8))


def check_triangles(triangles, n_vertices):
    """triangles as int32 [T,3] with T >= 1; ``ValueError`` on any other shape or on an index outside 0..n_vertices-1 (host only)."""
    tri = np.asarray(triangles)
    if tri.ndim != 2 or tri.shape[1] != 3 or tri.shape[0] == 0 or not np.issubdtype(tri.dtype, np.integer):
        raise ValueError("triangles must be a non-empty integer array [T,3]")
    lo, hi = int(tri.min()), int(tri.max())
    if lo < 0 or hi >= n_vertices:
        bad = np.argwhere((tri < 0) | (tri >= n_vertices))[0]
        raise ValueError(f"triangle {bad[0]} names vertex {int(tri[bad[0], bad[1]])}, outside 0..{n_vertices - 1}")
    return np.ascontiguousarray(tri, dtype=np.int32)


def sample_view(seed, n_points, center, scene_scale, max_holes=3, *, hole_mean, hole_std):
    """The draws of one view on ``np.random.seed(seed)``, in the reference's order (cad_to_dataset.py:264-276, then :145-160): three
    ``uniform(-1, 1)`` for the axis (normalised), ``uniform(0, 2 pi)`` for the angle, per axis ``uniform(0, 0.5 | 0.5 | 0.3)`` for the
    offset and ``rand() < 0.5`` for its sign, ``randint(max_holes)`` holes of ``randint(n_points)`` and ``max(0, normal(mean, std))``.
    Returns (axis (3,), angle, xyz (3,): the centroid's position in the units of ``transforms.txt``, holes: [(index, radius), ...])."""
    np.random.seed(seed)
    axis = np.random.uniform(-1, 1, size=3)
    axis /= np.linalg.norm(axis)
    angle = np.random.uniform(0, np.pi * 2)
    xyz = np.array(center, dtype=np.float64)
    for k, span in enumerate((0.5, 0.5, 0.3)):
        xyz[k] += np.random.uniform(0, span) * (-1 if np.random.rand() < 0.5 else 1) * scene_scale
    holes = []
    for _ in range(np.random.randint(max_holes)):
        h = int(np.random.randint(n_points))
        holes.append((h, float(max(0, np.random.normal(hole_mean, hole_std)))))
    return axis, float(angle), xyz, holes


def sample_scene(seed, n_points, center, scene_scale, n_objects, target=0, max_holes=3, *, hole_mean, hole_std, p_present=0.7,
                 lateral=0.8, depth=0.8):
    """One scene of ``n_objects`` objects around object ``target``.  The target's view is exactly ``sample_view(seed, n_points, center,
    scene_scale, max_holes, hole_mean=, hole_std=)``: seed s shows the target where the single-object tool shows it (its holes are
    drawn and returned, and not applied: in a scene the occluders play that part).  Everything else comes from
    ``np.random.default_rng((seed, 1))``, which leaves the global stream alone; per other object, in index order: ``random() < p_present``,
    three ``uniform(-1, 1)`` for the axis (normalised), ``uniform(0, 2 pi)`` for the angle, then the centre as an offset from the
    target's: ``uniform(-lateral, lateral)`` for x and for y and ``uniform(-depth, depth)`` for z (nearer or farther), in the units of
    ``transforms.txt``, times ``scene_scale``.  The draws are made whether or not the object is present.
    Returns (views: per object (present, axis (3,), angle, xyz (3,)), holes: the target's)."""
    axis, angle, xyz, holes = sample_view(seed, n_points, center, scene_scale, max_holes, hole_mean=hole_mean, hole_std=hole_std)
    rng = np.random.default_rng((int(seed), 1))
    views = []
    for o in range(n_objects):
        if o == target:
            views.append((True, axis, angle, xyz))
            continue
        here = bool(rng.random() < p_present)
        a = rng.uniform(-1, 1, size=3)
        a /= np.linalg.norm(a)
        ang = float(rng.uniform(0, np.pi * 2))
        off = np.array([rng.uniform(-lateral, lateral), rng.uniform(-lateral, lateral), rng.uniform(-depth, depth)]) * scene_scale
        views.append((here, a, ang, xyz + off))
    return views, holes


def transform_to_pose(pos, quat_xyzw):
    """A ``transforms.txt`` record -> (R_cam [3,3], t_cam (3,)): the loader's own arithmetic (``PoseDataset._targets``: ``convert_quat``,
    ``Rotation.from_quat``, ``@ Y_180``, ``pos * 1000`` with z negated), so that target = R_cam (10 model) + t_cam."""
    R = Rotation.from_quat(convert_quat(np.asarray(quat_xyzw, dtype=np.float64))).as_matrix() @ Y_180
    t = np.asarray(pos, dtype=np.float64) * 1000
    t[2] = -t[2]
    return R, t


def pose_to_transform(R_cam, t_cam):
    """The inverse of ``transform_to_pose`` in closed form (``Y_180`` and ``convert_quat`` are involutions): (pos (3,), quat_xyzw (4,))."""
    quat = convert_quat(Rotation.from_matrix(np.asarray(R_cam, dtype=np.float64) @ Y_180).as_quat())
    t = np.asarray(t_cam, dtype=np.float64)
    return np.array([t[0] / 1000, t[1] / 1000, -t[2] / 1000]), quat


def view_pose(axis, angle, xyz, centroid, model_scale):
    """(R_cam, t_cam) of a drawn view: the model turns about its centroid, then the centroid goes to ``xyz`` (:71-73).  The pose is that
    of the model's origin: t_cam = centre_cam - R (model_scale * centroid), with centre_cam = 1000 (x, y, -z) like the loader's ``pos``."""
    R = Rotation.from_rotvec(np.asarray(axis, dtype=np.float64) * angle).as_matrix()
    centre = np.array([xyz[0] * 1000, xyz[1] * 1000, -xyz[2] * 1000], dtype=np.float64)
    return R, centre - R @ (model_scale * np.asarray(centroid, dtype=np.float64))


class CadRenderer:
    """A coloured cloud on the device and the camera of one object directory.  ``render(poses, holes, splat, mask)``: poses [F,3,4]
    float64 [R|t] (``transform_to_pose``), holes: None or per frame a list of (index, radius) -> device tensors (rgb [F,IH,IW,3] uint8,
    depth, mask [F,IH,IW] uint16, stats [F,6] int32 = {covered, points, rmin, rmax, cmin, cmax}); nothing is read back."""

    def __init__(self, points, normals, colors, proj_mat, image_dims, device="cuda", model_scale=10.0):
        self.device = torch.device(device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        self.points = up(points, np.float32)
        self.normals = None if normals is None else up(normals, np.float32)
        self.colors = up(colors, np.uint8)
        self.proj_mat = np.ascontiguousarray(proj_mat, dtype=np.float64)
        self.image_dims = (int(image_dims[0]), int(image_dims[1]))
        self.model_scale = float(model_scale)
        self._scratch = None

    @staticmethod
    def pack_holes(holes, F):
        """per-frame lists of (index, radius) -> (hole_idx [F,K] int32 padded with -1, hole_r [F,K] float64), or None without any hole"""
        K = max((len(h) for h in holes), default=0) if holes is not None else 0
        if K == 0:
            return None
        if len(holes) != F:
            raise ValueError("holes: one list per frame")
        idx, rad = np.full((F, K), -1, dtype=np.int32), np.zeros((F, K), dtype=np.float64)
        for f, hs in enumerate(holes):
            for k, (h, r) in enumerate(hs):
                idx[f, k], rad[f, k] = h, r
        return idx, rad

    def render(self, poses, holes=None, splat=0, mask="box"):
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3, 4)
        F = poses.shape[0]
        need = F * self.image_dims[0] * self.image_dims[1] * 8
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        return pp.cad_render(self.points, self.normals, self.colors, poses, self.model_scale, self.proj_mat, self.image_dims,
                             holes=self.pack_holes(holes, F), splat=splat, mask_mode=MASK_MODES[mask], scratch=self._scratch)


class CadMeshRenderer:
    """A coloured triangle mesh on the device and the camera of one object directory (``df_cad_render_mesh``).  The triangle indices
    are checked on the host before anything is uploaded (``check_triangles``).  ``render(poses, holes, cull, mask)``: as
    ``CadRenderer.render`` without ``splat``; hole indices name vertices, ``cull`` 1 drops the triangles that face away;
    stats[:, 1] counts the triangles that reached the z-buffer."""

    def __init__(self, vertices, triangles, colors, proj_mat, image_dims, device="cuda", model_scale=10.0):
        vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        triangles = check_triangles(triangles, len(vertices))
        self.device = torch.device(device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        self.vertices = up(vertices, np.float32)
        self.triangles = up(triangles, np.int32)
        self.colors = up(colors, np.uint8)
        self.proj_mat = np.ascontiguousarray(proj_mat, dtype=np.float64)
        self.image_dims = (int(image_dims[0]), int(image_dims[1]))
        self.model_scale = float(model_scale)
        self._scratch = None

    pack_holes = staticmethod(CadRenderer.pack_holes)

    def render(self, poses, holes=None, cull=1, mask="box"):
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3, 4)
        F = poses.shape[0]
        need = F * self.image_dims[0] * self.image_dims[1] * 8
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        return pp.cad_render_mesh(self.vertices, self.colors, self.triangles, poses, self.model_scale, self.proj_mat, self.image_dims,
                                  holes=self.pack_holes(holes, F), cull=cull, mask_mode=MASK_MODES[mask], scratch=self._scratch)


class CadSceneRenderer:
    """Several coloured triangle meshes on the device and one camera (``df_cad_render_scene``): ``meshes`` is a list of (vertices,
    triangles, colours), object o being meshes[o] with ``model_scales[o]``.  Each mesh's indices are checked on the host
    (``check_triangles``); the meshes are concatenated once (indices made global) and uploaded once; the scratch buffer is reused.
    ``render(poses [F,O,3,4], present, cull)`` -> device tensors (rgb [F,IH,IW,3] uint8, depth and label [F,IH,IW] uint16 with label =
    object + 1 on the pixels it won, stats [F,O,6] int32 = {pixels won, triangles tested, rmin, rmax, cmin, cmax});
    ``masks(label, stats, pairs, mask)`` -> the loader's mask [N,IH,IW] uint16 of each (frame, object) pair."""

    def __init__(self, meshes, proj_mat, image_dims, model_scales, device="cuda"):
        if len(meshes) == 0 or len(meshes) != len(np.atleast_1d(model_scales)):
            raise ValueError("one model scale per mesh, at least one mesh")
        verts, tris, cols, begin = [], [], [], [0]
        for v, t, c in meshes:
            v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
            t = check_triangles(t, len(v))
            c = np.ascontiguousarray(c, dtype=np.uint8).reshape(-1, 3)
            if len(c) != len(v):
                raise ValueError("one colour per vertex")
            tris.append(t + np.int32(sum(len(x) for x in verts)))
            verts.append(v); cols.append(c)
            begin.append(begin[-1] + len(t))
        self.device = torch.device(device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(self.device)
        self.vertices = up(np.concatenate(verts), np.float32)
        self.triangles = up(np.concatenate(tris), np.int32)
        self.colors = up(np.concatenate(cols), np.uint8)
        self.tri_begin = np.array(begin, dtype=np.int32)
        self.model_scales = np.ascontiguousarray(model_scales, dtype=np.float64).reshape(-1)
        self.n_objects = len(meshes)
        self.proj_mat = np.ascontiguousarray(proj_mat, dtype=np.float64)
        self.image_dims = (int(image_dims[0]), int(image_dims[1]))
        self._scratch = None

    def render(self, poses, present=None, cull=1):
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, self.n_objects, 3, 4)
        F = poses.shape[0]
        need = F * self.image_dims[0] * self.image_dims[1] * 8
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        return pp.cad_render_scene(self.vertices, self.colors, self.triangles, self.tri_begin, self.model_scales, poses, self.proj_mat,
                                   self.image_dims, present=present, cull=cull, scratch=self._scratch)

    def masks(self, label, stats, pairs, mask="box"):
        return pp.cad_scene_mask(label, stats, pairs, mask_mode=MASK_MODES[mask])
