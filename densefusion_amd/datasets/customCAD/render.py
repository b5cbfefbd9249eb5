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

Lighting (``df_cad_render_mesh_lit`` / ``df_cad_render_scene_lit``): the two triangle renderers take ``normals``
(``"flat"``: ``face_normals``, one per triangle; ``"smooth"``: ``vertex_normals``, one per vertex; or the arrays themselves) and
``render(..., light=)`` one record {Lx, Ly, Lz, ambient, diffuse, cr, cg, cb} per frame, L the unit direction towards the light in
camera space ((0, 0, 1): a head-light).  A covered pixel's colour is multiplied by ambient + diffuse * max(N.L, 0) and the light's
colour; geometry, depth and masks do not change.  ``sample_light`` draws a record per seed from a stream of its own.  The reference
has no counterpart: its frames were lit by Unity.  The point renderer stays unlit.

Depth sensor (``df_cad_depth_sensor``): ``apply_sensor(depth, DepthSensor(...), seed, first_frame)`` turns the exact
depth of any of the three renderers into what a range camera would report -- noise of constant sigma in code units (the code is a
disparity, so the range noise grows with z squared), drop-out along depth discontinuities and at random, quantisation -- in integer
arithmetic on the codes.  Colour, masks, labels and the render's statistics stay those of the clean render.
"""
from __future__ import annotations

import numpy as np
import torch
from scipy.spatial.transform import Rotation

from ... import _lib
from ...lib import preprocess as pp
from ...lib.mesh_set import MeshSet, check_triangles      # noqa: F401 (check_triangles: this module's name for the renderers' host check)
from .dataset import _PLY_TYPES, Y_180, convert_quat

MASK_MODES = {"box": 0, "pixels": 1}
# the reference's shipped dataset_processed/data/01/meta/proj_mat.txt and its 520 x 1109 frames (dataset.py:99)
DEFAULT_PROJ = [[1.16667, 0.0, 0.0, 0.0], [0.0, 2.48814, 0.0, 0.0], [0.0, 0.0, 0.5, 3000.0], [0.0, 0.0, -1.0, 0.0]]


def add_view_arguments(ap):
    """The options that describe the views and the renderer, shared by tools/render_cad_dataset.py and everything that renders the
    same views on the fly (``online.RenderedPoseDataset.from_options``)."""
    ap.add_argument("--min_visible", type=float, default=0.3, help="--scene: smallest visible fraction of a frame that enters a model's tree")
    ap.add_argument("--p_present", type=float, default=0.7, help="--scene: probability that an object other than the view's own is in the frame")
    ap.add_argument("--lateral", type=float, default=0.8, help="--scene: largest sideways offset of the others, units of transforms.txt")
    ap.add_argument("--depth", type=float, default=0.8, help="--scene: largest offset of the others towards or away from the camera")
    ap.add_argument("--proj_mat", type=str, default=None, help="a proj_mat.txt (four tab-separated lines); default: the reference's shipped matrix")
    ap.add_argument("--height", type=int, default=520)
    ap.add_argument("--width", type=int, default=1109)
    ap.add_argument("--center", type=float, nargs=3, default=[0.0, 0.0, 4.0], help="mean position in the units of transforms.txt")
    ap.add_argument("--scene_scale", type=float, default=1.0)
    ap.add_argument("--model_scale", type=float, default=10.0, help="the loader's `model * 10`")
    ap.add_argument("--min_pixels", type=int, default=500)
    ap.add_argument("--splat", type=int, default=1)
    ap.add_argument("--raster", type=str, default="points", choices=("points", "mesh"), help="splat a sampled cloud, or rasterise the triangles")
    ap.add_argument("--cull", type=int, default=1, choices=(0, 1), help="--raster mesh: 1 drops the triangles that face away from the camera")
    ap.add_argument("--mask", type=str, default="box", choices=sorted(MASK_MODES))
    ap.add_argument("--light", type=str, default="none", choices=("none", "head", "random"),
                    help="--raster mesh / --scene: light the frames from the camera, or from a direction drawn per seed")
    ap.add_argument("--shading", type=str, default="flat", choices=("flat", "smooth"), help="--light: one normal per triangle, or per vertex")
    ap.add_argument("--light_angle", type=float, default=60.0, help="--light random: largest angle between light and viewing direction, degrees")
    ap.add_argument("--sensor_sigma", type=float, default=None, help="depth sensor: sigma of the disparity noise in 16-bit codes")
    ap.add_argument("--sensor_sigma_z", type=float, default=None, help="depth sensor: range noise at --sensor_z instead of --sensor_sigma")
    ap.add_argument("--sensor_z", type=float, default=None, help="depth sensor: the range at which --sensor_sigma_z holds")
    ap.add_argument("--sensor_edge", type=int, default=None, help="depth sensor: radius 0..4 of the window that finds depth discontinuities")
    ap.add_argument("--sensor_edge_step", type=int, default=None, help="depth sensor: a neighbour further than this many codes makes an edge")
    ap.add_argument("--sensor_edge_drop", type=float, default=None, help="depth sensor: probability that an edge pixel goes missing")
    ap.add_argument("--sensor_drop", type=float, default=None, help="depth sensor: probability that any pixel goes missing")
    ap.add_argument("--sensor_quant", type=int, default=None, help="depth sensor: codes are rounded to multiples of this, 1..4096")
    ap.add_argument("--sensor_seed", type=int, default=0, help="depth sensor: seed of its draws, next to each view's own seed")
    ap.add_argument("--points", type=int, default=0, help="points to draw from a mesh (default 1 000 000) or to keep of a cloud (default all)")
    ap.add_argument("--max_holes", type=int, default=3)
    ap.add_argument("--hole_mean", type=float, default=30.0, help="model file units")
    ap.add_argument("--hole_std", type=float, default=10.0)
    ap.add_argument("--chunk", type=int, default=32, help="views per device call")
    return ap


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


def load_cloud(path, n_points=0):
    """The cloud the point renderer splats, as the render tool loads it: a mesh is sampled into ``n_points`` points (default
    1 000 000) with ``np.random``; a cloud with more than ``n_points`` > 0 vertices keeps a sorted random subset of that many."""
    pts, nrm, col = read_colored_ply(path, n_points=n_points if n_points > 0 else 1000000)
    if 0 < n_points < len(pts):                      # a cloud with more vertices than asked for
        keep = np.sort(np.random.choice(len(pts), n_points, replace=False))
        pts, col, nrm = pts[keep], col[keep], None if nrm is None else nrm[keep]
    return pts, nrm, col


def _face_crosses(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    return v, t, np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])


def _unit_rows(a):
    """rows / their length as float32; a zero (or non-finite) row gives zeros"""
    n = np.linalg.norm(a, axis=1, keepdims=True)
    ok = np.isfinite(n) & (n > 0)
    return np.ascontiguousarray(np.where(ok, a / np.where(ok, n, 1.0), 0.0), dtype=np.float32)


def face_normals(vertices, triangles):
    """float32 [T,3]: the fp64 cross product (v1 - v0) x (v2 - v0) of every triangle, normalised -- outward for triangles wound
    counter-clockwise seen from outside.  A degenerate triangle gives zeros."""
    return _unit_rows(_face_crosses(vertices, triangles)[2])


def vertex_normals(vertices, triangles):
    """float32 [V,3]: per vertex the sum of the unnormalised crosses of its faces (area weighting), normalised.  A vertex that no
    triangle names gives zeros."""
    v, t, cross = _face_crosses(vertices, triangles)
    acc = np.zeros_like(v)
    for k in range(3):
        np.add.at(acc, t[:, k], cross)
    return _unit_rows(acc)


def sample_light(seed, max_angle=np.radians(60.0), ambient=(0.3, 0.6), diffuse=(0.4, 0.9), tint=0.1):
    """One light record (8,) float64 {Lx, Ly, Lz, ambient, diffuse, cr, cg, cb} from ``np.random.default_rng((seed, 2))``, which leaves
    the global stream and ``sample_scene``'s (seed, 1) stream alone.  The draws, in this order: ``u = random()`` and
    ``phi = uniform(0, 2 pi)`` for a direction uniform on the cap of half angle ``max_angle`` around +z (cos theta = 1 - u (1 - cos
    max_angle)), ``uniform(*ambient)``, ``uniform(*diffuse)``, ``uniform(1 - tint, 1, 3)`` for the colour.  The ranges are design
    defaults, not measurements."""
    rng = np.random.default_rng((int(seed), 2))
    u = rng.random()
    phi = rng.uniform(0, np.pi * 2)
    cos_t = 1.0 - u * (1.0 - np.cos(max_angle))
    sin_t = np.sqrt(max(0.0, 1.0 - cos_t * cos_t))
    L = np.array([sin_t * np.cos(phi), sin_t * np.sin(phi), cos_t])
    L /= np.linalg.norm(L)
    return np.concatenate([L, [rng.uniform(*ambient), rng.uniform(*diffuse)], rng.uniform(1.0 - tint, 1.0, 3)])


HEAD_LIGHT = (0.0, 0.0, 1.0, 0.4, 0.6, 1.0, 1.0, 1.0)      # lit from the camera: a facing surface keeps its colour


def check_light(light, F):
    """light as float64 [F,8]; ``ValueError`` on any other shape, a non-finite entry, a negative ambient, diffuse or colour, or a
    direction whose length differs from 1 by more than 1e-6 (host only)."""
    light = np.ascontiguousarray(light, dtype=np.float64)
    if light.shape != (F, 8):
        raise ValueError(f"light must be [F,8] = [{F},8], one record per frame; got {light.shape}")
    if not np.isfinite(light).all():
        raise ValueError("light holds a non-finite entry")
    if (light[:, 3:] < 0).any():
        raise ValueError("light: ambient, diffuse and colour must not be negative")
    if (np.abs(np.linalg.norm(light[:, :3], axis=1) - 1.0) > 1e-6).any():
        raise ValueError("light: the direction must be of unit length")
    return light


def _make_normals(normals, vertices, triangles):
    """``normals`` of a renderer -> (float32 array, normal_mode): "flat" / "smooth" are computed, an array is [T,3] (mode 0) or [V,3]
    (mode 1; when T == V an array counts as per-triangle)."""
    if isinstance(normals, str):
        if normals not in ("flat", "smooth"):
            raise ValueError('normals must be None, "flat", "smooth" or an array')
        return (face_normals(vertices, triangles), 0) if normals == "flat" else (vertex_normals(vertices, triangles), 1)
    n = np.ascontiguousarray(normals, dtype=np.float32)
    if n.ndim != 2 or n.shape[1] != 3 or n.shape[0] not in (len(triangles), len(vertices)):
        raise ValueError(f"normals must be [T,3] = [{len(triangles)},3] or [V,3] = [{len(vertices)},3]")
    return n, 0 if n.shape[0] == len(triangles) else 1


def sample_view(seed, n_points, center, scene_scale, max_holes=3, *, hole_mean, hole_std, private=False):
    """The draws of one view on ``np.random.seed(seed)``, in the reference's order (cad_to_dataset.py:264-276, then :145-160): three
    ``uniform(-1, 1)`` for the axis (normalised), ``uniform(0, 2 pi)`` for the angle, per axis ``uniform(0, 0.5 | 0.5 | 0.3)`` for the
    offset and ``rand() < 0.5`` for its sign, ``randint(max_holes)`` holes of ``randint(n_points)`` and ``max(0, normal(mean, std))``.
    ``private``: the same draws from ``np.random.RandomState(seed)`` -- the same generator in the same state, so the same values --
    which leaves the global stream alone: for callers on several threads.
    Returns (axis (3,), angle, xyz (3,): the centroid's position in the units of ``transforms.txt``, holes: [(index, radius), ...])."""
    if private:
        rs = np.random.RandomState(seed)
    else:
        rs = np.random
        rs.seed(seed)
    axis = rs.uniform(-1, 1, size=3)
    axis /= np.linalg.norm(axis)
    angle = rs.uniform(0, np.pi * 2)
    xyz = np.array(center, dtype=np.float64)
    for k, span in enumerate((0.5, 0.5, 0.3)):
        xyz[k] += rs.uniform(0, span) * (-1 if rs.rand() < 0.5 else 1) * scene_scale
    holes = []
    for _ in range(rs.randint(max_holes)):
        h = int(rs.randint(n_points))
        holes.append((h, float(max(0, rs.normal(hole_mean, hole_std)))))
    return axis, float(angle), xyz, holes


def sample_scene(seed, n_points, center, scene_scale, n_objects, target=0, max_holes=3, *, hole_mean, hole_std, p_present=0.7,
                 lateral=0.8, depth=0.8, private=False):
    """One scene of ``n_objects`` objects around object ``target``.  The target's view is exactly ``sample_view(seed, n_points, center,
    scene_scale, max_holes, hole_mean=, hole_std=)``: seed s shows the target where the single-object tool shows it (its holes are
    drawn and returned, and not applied: in a scene the occluders play that part).  Everything else comes from
    ``np.random.default_rng((seed, 1))``, which leaves the global stream alone; per other object, in index order: ``random() < p_present``,
    three ``uniform(-1, 1)`` for the axis (normalised), ``uniform(0, 2 pi)`` for the angle, then the centre as an offset from the
    target's: ``uniform(-lateral, lateral)`` for x and for y and ``uniform(-depth, depth)`` for z (nearer or farther), in the units of
    ``transforms.txt``, times ``scene_scale``.  The draws are made whether or not the object is present.
    Returns (views: per object (present, axis (3,), angle, xyz (3,)), holes: the target's)."""
    axis, angle, xyz, holes = sample_view(seed, n_points, center, scene_scale, max_holes, hole_mean=hole_mean, hole_std=hole_std,
                                          private=private)
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


# ---- the view rules the render tool and the online dataset (online.py) share: records, their text round trip, lights, skips -------
def record_text(index, pos, quat):
    """One ``transforms.txt`` record in the generator's format: index / (x, y, z) / (x, y, z, w)."""
    return "%d\n(%s)\n(%s)\n" % (index, ", ".join(repr(float(v)) for v in pos), ", ".join(repr(float(v)) for v in quat))


def parse_record(text):
    """(pos, quat) of one record, token by token like the loader's ``parse_transforms``."""
    lines = text.split("\n")
    return tuple(np.array([float(x.rstrip()) for x in ln.replace("(", "").replace(")", "").replace(",", "").split(" ")]) for ln in lines[1:3])


def light_text(light):
    """The eight values of a light record as they stand in ``lights.txt`` after the frame number."""
    return " ".join(repr(float(v)) for v in light)


def parse_light(text):
    return np.array([float(x) for x in text.split()], dtype=np.float64)


def draw_light(kind, seed, light_angle=60.0):
    """The light of seed ``seed`` as (text, record parsed back from it), rendered from the file's own values: ``kind`` "head" is
    ``HEAD_LIGHT``, "random" is ``sample_light(seed)`` within ``light_angle`` degrees of the viewing direction."""
    if kind not in ("head", "random"):
        raise ValueError(f'light must be "head" or "random", got {kind!r}')
    light = HEAD_LIGHT if kind == "head" else sample_light(seed, max_angle=np.radians(light_angle))
    text = light_text(light)
    return text, parse_light(text)


def record_pose(axis, angle, xyz, centroid, model_scale):
    """A drawn view as (its ``transforms.txt`` record with index 0, the pose [3,4] = [R|t] of the values parsed back from that text):
    the frame is rendered from the record's own values, so images and records agree exactly."""
    text = record_text(0, *pose_to_transform(*view_pose(axis, angle, xyz, centroid, model_scale)))
    R, t = transform_to_pose(*parse_record(text))
    return text, np.concatenate([R, t[:, None]], axis=1)


def draw_view_records(seeds, n_points, centroid, center, scene_scale, model_scale, max_holes=3, *, hole_mean, hole_std, private=False):
    """``sample_view`` and ``record_pose`` per seed: (texts [F], poses [F,3,4], holes: per frame a list of (index, radius))."""
    texts, poses, holes = [], [], []
    for s in seeds:
        axis, angle, xyz, hs = sample_view(s, n_points, center, scene_scale, max_holes, hole_mean=hole_mean, hole_std=hole_std,
                                           private=private)
        text, pose = record_pose(axis, angle, xyz, centroid, model_scale)
        texts.append(text); poses.append(pose); holes.append(hs)
    return texts, np.stack(poses), holes


def draw_scene_records(seeds, n_vertices, centroids, n_targets, center, scene_scale, model_scale, max_holes=3, *, hole_mean, hole_std,
                       p_present=0.7, lateral=0.8, depth=0.8, private=False):
    """``sample_scene`` per seed for O = len(centroids) objects, the first ``n_targets`` of them targets: the scene of seed s is drawn
    around object s mod n_targets (``n_vertices[o]`` its vertex count), every object's view goes through ``record_pose``.
    Returns (texts [F][O], poses [F,O,3,4], present [F,O] uint8)."""
    O = len(centroids)
    texts, poses, present = [], [], np.zeros((len(seeds), O), dtype=np.uint8)
    for j, s in enumerate(seeds):
        primary = s % n_targets
        views, _ = sample_scene(s, n_vertices[primary], center, scene_scale, O, primary, max_holes, hole_mean=hole_mean,
                                hole_std=hole_std, p_present=p_present, lateral=lateral, depth=depth, private=private)
        row_t, row_p = [], []
        for o, (here, axis, angle, xyz) in enumerate(views):
            text, pose = record_pose(axis, angle, xyz, centroids[o], model_scale)
            row_t.append(text); row_p.append(pose)
            present[j, o] = here
        texts.append(row_t); poses.append(np.stack(row_p))
    return texts, np.stack(poses), present


def view_kept(covered, min_pixels):
    """The skip rule of a single-object view (cad_to_dataset.py:219-221): kept with at least ``min_pixels`` covered pixels."""
    return covered >= min_pixels


def scene_view_kept(won, alone, min_pixels, min_visible):
    """The skip rule of one object in a scene frame: (kept, visible fraction = pixels won in the scene / pixels won alone at the same
    poses); kept with at least ``min_pixels`` pixels won and a visible fraction of at least ``min_visible``."""
    frac = won / alone if alone > 0 else 0.0
    return not (won < min_pixels or frac < min_visible), frac


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
        self._scratch = _lib.grow_scratch(self._scratch, F * self.image_dims[0] * self.image_dims[1] * 8, self.device)
        return pp.cad_render(self.points, self.normals, self.colors, poses, self.model_scale, self.proj_mat, self.image_dims,
                             holes=self.pack_holes(holes, F), splat=splat, mask_mode=MASK_MODES[mask], scratch=self._scratch)


class CadMeshRenderer:
    """A coloured triangle mesh on the device and the camera of one object directory (``df_cad_render_mesh``), checked on the host before
    anything is uploaded (``MeshSet``; ``vertices`` may be one, with colours: the other two are unused).  ``render(poses, holes, cull, mask)``: as
    ``CadRenderer.render`` without ``splat``; hole indices name vertices, ``cull`` 1 drops the triangles that face away;
    stats[:, 1] counts the triangles that reached the z-buffer.  ``normals``: None, "flat", "smooth" or an array ([T,3] or [V,3]);
    with them ``render(..., light=[F,8])`` lights the frames (``df_cad_render_mesh_lit``); the light is checked on the host
    (``check_light``) before anything is uploaded, and a light without normals is a ``ValueError``."""

    def __init__(self, vertices, triangles, colors, proj_mat, image_dims, device="cuda", model_scale=10.0, normals=None):
        ms = vertices if isinstance(vertices, MeshSet) else MeshSet([(vertices, triangles, colors)], colors=True)
        made = None if normals is None else _make_normals(normals, ms.vertices, ms.triangles)
        self.device = torch.device(device)
        self.vertices, self.triangles, self.colors = ms.on(self.device)
        self.proj_mat = np.ascontiguousarray(proj_mat, dtype=np.float64)
        self.image_dims = (int(image_dims[0]), int(image_dims[1]))
        self.model_scale = float(model_scale)
        self.normals, self.normal_mode = (None, 0) if made is None else (torch.from_numpy(made[0]).to(self.device), made[1])
        self._scratch = None

    pack_holes = staticmethod(CadRenderer.pack_holes)

    def render(self, poses, holes=None, cull=1, mask="box", light=None):
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3, 4)
        F = poses.shape[0]
        if light is not None:
            if self.normals is None:
                raise ValueError("a light needs normals: build the renderer with normals=")
            light = check_light(light, F)
        self._scratch = _lib.grow_scratch(self._scratch, F * self.image_dims[0] * self.image_dims[1] * 8, self.device)
        return pp.cad_render_mesh(self.vertices, self.colors, self.triangles, poses, self.model_scale, self.proj_mat, self.image_dims,
                                  holes=self.pack_holes(holes, F), cull=cull, mask_mode=MASK_MODES[mask], scratch=self._scratch,
                                  normals=self.normals, normal_mode=self.normal_mode, light=light)


class CadSceneRenderer:
    """Several coloured triangle meshes on the device and one camera (``df_cad_render_scene``): ``meshes`` is a ``MeshSet`` with colours
    or the list of (vertices, triangles, colours) it packs, object o being mesh o with ``model_scales[o]``.  Everything is checked on the
    host before the set is uploaded; the scratch buffer is reused.
    ``render(poses [F,O,3,4], present, cull)`` -> device tensors (rgb [F,IH,IW,3] uint8, depth and label [F,IH,IW] uint16 with label =
    object + 1 on the pixels it won, stats [F,O,6] int32 = {pixels won, triangles tested, rmin, rmax, cmin, cmax});
    ``masks(label, stats, pairs, mask)`` -> the loader's mask [N,IH,IW] uint16 of each (frame, object) pair.
    ``normals``: None, "flat", "smooth" or one array per mesh (all per triangle or all per vertex), concatenated like the vertices and
    triangles; with them ``render(..., light=[F,8])`` lights the frames, one light per frame for all objects
    (``df_cad_render_scene_lit``), checked as in ``CadMeshRenderer``."""

    def __init__(self, meshes, proj_mat, image_dims, model_scales, device="cuda", normals=None):
        ms = meshes if isinstance(meshes, MeshSet) else MeshSet(meshes, colors=True)
        if ms.colors is None or ms.n_objects != len(np.atleast_1d(model_scales)):
            raise ValueError("one model scale per mesh, and meshes with colours")
        if normals is not None and not isinstance(normals, str) and len(normals) != ms.n_objects:
            raise ValueError("normals: one array per mesh")
        vb, tb = ms.vertex_begin, ms.tri_begin
        nrms = [] if normals is None else [_make_normals(normals if isinstance(normals, str) else normals[o], ms.vertices[vb[o]:vb[o + 1]],
                                                         ms.triangles[tb[o]:tb[o + 1]] - vb[o]) for o in range(ms.n_objects)]
        if len({m for _, m in nrms}) > 1:
            raise ValueError("normals: per triangle for all meshes or per vertex for all meshes")
        self.device = torch.device(device)
        self.vertices, self.triangles, self.colors = ms.on(self.device)
        self.tri_begin, self.n_objects = ms.tri_begin, ms.n_objects
        self.model_scales = np.ascontiguousarray(model_scales, dtype=np.float64).reshape(-1)
        self.proj_mat = np.ascontiguousarray(proj_mat, dtype=np.float64)
        self.image_dims = (int(image_dims[0]), int(image_dims[1]))
        self.normals, self.normal_mode, self._scratch = None, 0, None
        if nrms:
            self.normals, self.normal_mode = torch.from_numpy(np.concatenate([n for n, _ in nrms])).to(self.device), nrms[0][1]

    def render(self, poses, present=None, cull=1, light=None):
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, self.n_objects, 3, 4)
        F = poses.shape[0]
        if light is not None:
            if self.normals is None:
                raise ValueError("a light needs normals: build the renderer with normals=")
            light = check_light(light, F)
        self._scratch = _lib.grow_scratch(self._scratch, F * self.image_dims[0] * self.image_dims[1] * 8, self.device)
        return pp.cad_render_scene(self.vertices, self.colors, self.triangles, self.tri_begin, self.model_scales, poses, self.proj_mat,
                                   self.image_dims, present=present, cull=cull, scratch=self._scratch, normals=self.normals,
                                   normal_mode=self.normal_mode, light=light)

    def masks(self, label, stats, pairs, mask="box"):
        return pp.cad_scene_mask(label, stats, pairs, mask_mode=MASK_MODES[mask])


NOISE_VARIANCE = 1431655765          # of the centred sum of four 16-bit uniforms (step D5): 4 (2^32 - 1) / 12


class DepthSensor:
    """The record of the depth-sensor model (steps D0..D6 of ``df_cad_depth_sensor``).  ``sigma_code``: standard deviation of the
    disparity noise in code units (``sigma_code_at`` gives the one that means a range noise at a range); ``edge_radius`` R 0..4: a
    pixel is an edge pixel when its (2R+1)^2 window holds a horizon pixel or a code further than ``edge_step`` from its own;
    ``edge_drop``: probability that an edge pixel goes missing; ``drop``: probability that any pixel does; ``quant`` 1..4096: the codes
    are rounded to multiples of it.  The defaults are the identity.  A bad value is a ``ValueError`` (host only).
    ``record()`` -> (noise_mul, edge_radius, edge_step, edge_drop24, drop24, quant), the six integers of the call."""

    def __init__(self, sigma_code=0.0, edge_radius=0, edge_step=0, edge_drop=0.0, drop=0.0, quant=1):
        sigma_code, edge_drop, drop = float(sigma_code), float(edge_drop), float(drop)
        if not np.isfinite(sigma_code) or sigma_code < 0:
            raise ValueError(f"sigma_code {sigma_code} must be finite and not negative")
        noise_mul = int(np.rint(sigma_code * 2.0 ** 32 / np.sqrt(float(NOISE_VARIANCE))))
        if noise_mul > 2 ** 31 - 1:
            raise ValueError(f"sigma_code {sigma_code} is too large: noise_mul {noise_mul} above 2^31 - 1")
        for name, v, lo, hi in (("edge_radius", edge_radius, 0, 4), ("edge_step", edge_step, 0, 65535), ("quant", quant, 1, 4096)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError(f"{name} {v!r} must be an integer in {lo}..{hi}")
        for name, v in (("edge_drop", edge_drop), ("drop", drop)):
            if not 0.0 <= v <= 1.0:                                             # a NaN fails too
                raise ValueError(f"{name} {v} must be a probability")
        self.sigma_code, self.edge_radius, self.edge_step = sigma_code, int(edge_radius), int(edge_step)
        self.edge_drop, self.drop, self.quant = edge_drop, drop, int(quant)
        self._record = (noise_mul, self.edge_radius, self.edge_step, int(np.rint(edge_drop * 2.0 ** 24)), int(np.rint(drop * 2.0 ** 24)),
                        self.quant)

    def record(self):
        return self._record

    @staticmethod
    def sigma_code_at(proj_mat, sigma_z, z):
        """The code-space sigma that gives range noise ``sigma_z`` at range ``z``, both in the units of
        ``UnityDepthProjector.project_depth``: code = 65534 ((1 + p22) + p23 / z), so |d code / d z| = 65534 |p23| / z^2."""
        return 65534.0 * abs(float(np.asarray(proj_mat, dtype=np.float64)[2, 3])) * float(sigma_z) / (float(z) * float(z))


def sensor_from_flags(proj_mat, sigma=None, sigma_z=None, z=None, edge=None, edge_step=None, edge_drop=None, drop=None, quant=None):
    """The ``DepthSensor`` of the render tool's ``--sensor_*`` flags (None = not given), or None when none of them is given.  The noise
    is ``sigma`` in codes, or the range noise ``sigma_z`` at range ``z`` (``sigma_code_at``).  ``ValueError`` with the tool's message."""
    if all(v is None for v in (sigma, sigma_z, z, edge, edge_step, edge_drop, drop, quant)):
        return None
    if (sigma_z is None) != (z is None) or (sigma is not None and sigma_z is not None):
        raise ValueError("the depth sensor's noise is --sensor_sigma CODES, or --sensor_sigma_z S together with --sensor_z Z")
    sigma = sigma or 0.0
    if sigma_z is not None:
        if z == 0:
            raise ValueError("--sensor_z must not be 0")
        sigma = DepthSensor.sigma_code_at(proj_mat, sigma_z, z)
    try:
        return DepthSensor(sigma_code=sigma, edge_radius=edge or 0, edge_step=edge_step or 0, edge_drop=edge_drop or 0.0, drop=drop or 0.0,
                           quant=1 if quant is None else quant)
    except ValueError as e:
        raise ValueError(f"depth sensor: {e}") from None


def apply_sensor(depth, sensor, seed, first_frame=0):
    """``sensor`` (a ``DepthSensor``) over rendered depth [F,IH,IW] uint16 on the device, after any of the three renderers: frame f draws
    from (seed, first_frame + f), so a frame's result does not depend on how the frames are cut into calls.
    Returns (depth_out, stats [F,4] int32 = {edge pixels, dropped at random, dropped at an edge, kept and changed}); ``depth`` is left
    as it is, nothing is read back."""
    if not isinstance(sensor, DepthSensor):
        raise ValueError("sensor must be a DepthSensor")
    return pp.cad_depth_sensor(depth, sensor.record(), seed, first_frame)
