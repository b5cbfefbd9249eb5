"""CPU: diffuse lighting of the customCAD triangle renderers -- the numpy restatement of steps L1..L6 (tests/cad_light_np.py) against the
unlit restatements and against the analytic sphere, the normals and the light sampler of datasets/customCAD/render.py, the host checks
of the renderers' ``light`` argument and the tool's flags.  No device work."""
import importlib
import os
import sys

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import cad_light_np as lnp
import cad_raster_np as mnp
import cad_scene_np as snp
from densefusion_amd.datasets.customCAD import render as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IH, IW, NODE_PROJ = snp.IH, snp.IW, snp.NODE_PROJ
FAR = [0.0, 0.0, -4096.0]


def scene_normals(s, mode):
    """per-triangle (mode 0) or per-vertex (mode 1) normals of a scene fixture, over its global arrays"""
    v, t = s["vertices"].astype(np.float64), s["triangles"]
    return cr.face_normals(v, t) if mode == 0 else cr.vertex_normals(v, t)


def test_identity_record_gives_the_unlit_bytes():
    """{., ., ., 1, 0, 1, 1, 1} multiplies by exactly 1.0: the mesh fixture with holes and the scene fixture, both modes, cull 0."""
    from test_cad_raster_gpu import small_scene
    verts, col, tris, poses, holes, _ = small_scene()
    want = mnp.render(verts, col, tris, poses, 10.0, holes, NODE_PROJ, IH, IW, 0, 0)
    assert (want[3][:3, 0] > 0).all()
    rec = np.tile(lnp.IDENTITY, (4, 1))
    rec[:, :3] = [[0, 0, 1], [0.6, 0, 0.8], [0, -1, 0], [1, 0, 0]]
    for mode, nrm in ((0, cr.face_normals(verts, tris.clip(0, len(verts) - 1))), (1, cr.vertex_normals(verts, tris.clip(0, len(verts) - 1)))):
        got = lnp.render_mesh(verts, col, tris, poses, 10.0, holes, NODE_PROJ, IH, IW, 0, 0, nrm, mode, rec)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes(), mode
    s = snp.small_scene()
    want = snp.render(s["vertices"], s["colors"], s["triangles"], s["tri_begin"], s["scales"], s["poses"], s["present"], NODE_PROJ, IH, IW, 0)
    for mode in (0, 1):
        got = lnp.render_scene(s["vertices"], s["colors"], s["triangles"], s["tri_begin"], s["scales"], s["poses"], s["present"], NODE_PROJ,
                               IH, IW, 0, scene_normals(s, mode), mode, rec)
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes(), mode


def test_flat_shading_gives_one_colour_per_winning_triangle():
    """A uniformly coloured icosphere in mode 0: every pixel a triangle wins has that triangle's colour, and neighbours differ."""
    v, f = mnp.icosphere(1, 160.0)
    col = np.full((len(v), 3), 200, dtype=np.uint8)
    R = Rotation.from_rotvec([0.3, -0.5, 0.2]).as_matrix()
    poses = snp.pose(R, FAR)[None]
    rec = np.array([[0.48, 0.36, 0.8, 0.2, 0.7, 1.0, 0.9, 0.8]])
    rgb, depth, mask, stats, winner = lnp.render_mesh(v.astype(np.float32), col, f, poses, 10.0, None, NODE_PROJ, IH, IW, 1, 0,
                                                      cr.face_normals(v, f), 0, rec)
    won = np.unique(winner[0][winner[0] >= 0])
    assert len(won) >= 20 and stats[0, 0] > 300
    colours = set()
    for t in won:
        px = rgb[0][winner[0] == t]
        assert (px == px[0]).all(), t
        colours.add(tuple(px[0]))
    assert len(colours) >= len(won) // 2, "facets show"
    assert (rgb[0][winner[0] < 0] == 130).all()


def test_a_back_face_is_lit_as_the_side_the_camera_sees():
    """L3: a quad seen from behind (cull 0, A > 0) gets the colour it gets from the front under the mirrored pose (turned by 180
    degrees about y), not the ambient-only colour an unflipped normal would give."""
    quad = np.array([snp.on(15, 10), snp.on(40, 10), snp.on(40, 28), snp.on(15, 28)], dtype=np.float32)
    tris = np.array([[0, 2, 1], [0, 3, 2]], dtype=np.int32)            # counter-clockwise seen from +z: the camera of `front`
    col = np.full((4, 3), 180, dtype=np.uint8)
    nrm = cr.face_normals(quad, tris)
    assert np.array_equal(nrm, [[0, 0, 1], [0, 0, 1]])
    rec = np.array([[0.0, 0.6, 0.8, 0.25, 0.75, 1.0, 1.0, 1.0]])
    front, back = snp.pose(np.eye(3), FAR)[None], snp.pose(np.diag([-1.0, 1.0, -1.0]), FAR)[None]
    a = lnp.render_mesh(quad, col, tris, front, 10.0, None, NODE_PROJ, IH, IW, 0, 0, nrm, 0, rec)
    b = lnp.render_mesh(quad, col, tris, back, 10.0, None, NODE_PROJ, IH, IW, 0, 0, nrm, 0, rec)
    culled = lnp.render_mesh(quad, col, tris, back, 10.0, None, NODE_PROJ, IH, IW, 1, 0, nrm, 0, rec)
    assert a[3][0, 0] > 300 and b[3][0, 0] > 300 and culled[3][0, 0] == 0
    ca, cb = np.unique(a[0][0][a[4][0] >= 0], axis=0), np.unique(b[0][0][b[4][0] >= 0], axis=0)
    assert len(ca) == 1 and np.array_equal(ca, cb)
    assert ca[0, 0] == round(180 * (0.25 + 0.75 * 0.8)) and ca[0, 0] != round(180 * 0.25)


def test_smooth_shading_follows_the_analytic_sphere():
    """icosphere(3), white, ``vertex_normals``, a head-light: every covered pixel against 255 (ambient + diffuse n.L) of the sphere point
    on that pixel's ray.

    The bound: the largest angle phi between two corner normals of one facet, times 255 * diffuse, plus half an 8-bit step.
    Where it comes from.  The pixel's N is a mix of the winning facet's three corner normals with weights b_k >= 0 of sum 1 (u_k / U
    are the barycentric coordinates of the facet point on the ray), so N lies in their convex hull: it differs from each of them by at
    most the largest chord between two of them, which is below their angle, and what the missing re-normalisation costs
    (|N| >= cos(phi / 2)) is inside that figure.  The sphere's own normal on the ray is not one of the corners', but it is as close: the
    mesh is inscribed, so the ray enters the sphere inside the cap that the facet's plane cuts off, and the corners lie on the rim of
    that cap, whose angular radius is phi / sqrt(3) for a near-equilateral facet; where the ray looks down on the facet the two normals
    differ in second order only, and at the silhouette, where the mesh ends one sagitta inside the sphere, the sphere's n.L is
    sqrt(2 sagitta / radius) = the cap's radius while the mix is near 0.  So the largest difference to expect is phi / sqrt(3) and phi
    holds it with room; the worst geometry one can construct without regard to the ray (the sphere's normal on one side of the rim, the
    mix at the corner opposite) would give two cap radii, 1.16 phi, and does not occur for a ray that meets the sphere before the facet.
    |L| = 1 and max(., 0) is 1-Lipschitz, so the difference reaches the channel times 255 * diffuse; rint adds half a step."""
    radius, scale = 60.0, 10.0
    v, f = mnp.icosphere(3, radius)
    nrm = cr.vertex_normals(v, f).astype(np.float64)
    n = nrm[f]
    cosines = [np.clip((n[:, a] * n[:, b]).sum(axis=1), -1, 1) for a, b in ((0, 1), (1, 2), (2, 0))]
    phi = float(np.arccos(np.min(cosines)))
    assert 0.05 < phi < 0.2, phi
    ambient, diffuse = 0.25, 0.75
    bound = 255.0 * diffuse * phi + 0.5
    H, W = 96, 144
    proj = np.array([[1.16667, 0, 0, 0], [0, 2.48814 * 144 / 96 * 520 / 1109, 0, 0], [0, 0, 0.5, 3000.0], [0, 0, -1.0, 0]])
    R = Rotation.from_rotvec([0.4, 0.7, -0.2]).as_matrix()
    t = np.array([350.0, -150.0, -2600.0])
    rec = np.array([[0.0, 0.0, 1.0, ambient, diffuse, 1.0, 1.0, 1.0]])
    col = np.full((len(v), 3), 255, dtype=np.uint8)
    rgb, depth, mask, stats, winner = lnp.render_mesh(v.astype(np.float32), col, f, snp.pose(R, t)[None], scale, None, proj, H, W, 1, 0,
                                                      nrm.astype(np.float32), 1, rec)
    r, q = np.where(winner[0] >= 0)
    assert len(r) > 1000
    # the ray of node (r, q): ndc (-1 + 2 q / W, 1 - 2 r / H), direction (ndc_x / P00, ndc_y / P11, -1)
    d = np.stack([(-1.0 + 2.0 * q / W) / proj[0, 0], (1.0 - 2.0 * r / H) / proj[1, 1], -np.ones(len(r))], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    b = (d * t).sum(axis=1)
    disc = b * b - ((t * t).sum() - (radius * scale) ** 2)
    assert (disc > 0).all(), "the mesh lies inside the sphere"
    p = (b - np.sqrt(disc))[:, None] * d
    nz = ((p - t) / (radius * scale))[:, 2]
    want = 255.0 * (ambient + diffuse * np.maximum(nz, 0.0))
    err = np.abs(rgb[0, r, q].astype(np.float64) - want[:, None])
    print("phi", phi, "bound", bound, "worst", err.max(), "mean", err.mean(), "pixels", len(r))
    assert err.max() <= bound
    assert rgb[0, r, q, 0].max() - rgb[0, r, q, 0].min() > 100, "the shading spans the sphere"
    assert (rgb[0, r, q, 0] == rgb[0, r, q, 1]).all() and (rgb[0, r, q, 0] == rgb[0, r, q, 2]).all()


def test_normals_of_a_box_and_an_icosphere():
    bv, bf = snp.box([-3.0, -2.0, -1.0], [3.0, 2.0, 1.0])
    fn = cr.face_normals(bv, bf)
    assert fn.dtype == np.float32 and fn.shape == (12, 3)
    centre = bv[bf].mean(axis=1)
    assert (np.abs(fn).max(axis=1) == 1).all() and (np.abs(fn).sum(axis=1) == 1).all(), "axis-aligned, exactly"
    assert ((fn * centre).sum(axis=1) > 0).all(), "outward"
    vn = cr.vertex_normals(bv, bf)
    assert vn.dtype == np.float32 and np.abs(np.linalg.norm(vn, axis=1) - 1).max() < 1e-6 and ((vn * bv) > 0).all()
    v, f = mnp.icosphere(2, 5.0)
    fn, vn = cr.face_normals(v, f), cr.vertex_normals(v, f)
    assert np.abs(np.linalg.norm(fn, axis=1) - 1).max() < 1e-6 and np.abs(np.linalg.norm(vn, axis=1) - 1).max() < 1e-6
    assert ((fn * v[f].mean(axis=1)).sum(axis=1) > 0).all()
    assert ((vn * v / 5.0).sum(axis=1) > 0.999).all(), "close to radial"
    # a degenerate triangle and a vertex no triangle names
    v2 = np.concatenate([v, [[9.0, 9.0, 9.0]]])
    f2 = np.concatenate([f, [[0, 1, 1]], [[2, 2, 2]]])
    fn2, vn2 = cr.face_normals(v2, f2), cr.vertex_normals(v2, f2)
    assert np.array_equal(fn2[:-2], fn) and not fn2[-2:].any()
    assert np.array_equal(vn2[:-1], vn) and not vn2[-1].any()


def test_sample_light_draws():
    np.random.seed(5)
    state = np.random.get_state()
    for seed in range(50):
        a, b = cr.sample_light(seed), cr.sample_light(seed)
        assert a.dtype == np.float64 and a.shape == (8,) and np.array_equal(a, b)
        assert abs(np.linalg.norm(a[:3]) - 1) < 1e-12 and a[2] >= np.cos(np.pi / 3) - 1e-12
        assert 0.3 <= a[3] <= 0.6 and 0.4 <= a[4] <= 0.9 and (a[5:] >= 0.9).all() and (a[5:] <= 1.0).all()
        n = cr.sample_light(seed, max_angle=np.radians(10.0), ambient=(0.1, 0.1), diffuse=(2.0, 3.0), tint=0.0)
        assert n[2] >= np.cos(np.radians(10.0)) - 1e-12 and n[3] == 0.1 and 2.0 <= n[4] <= 3.0 and (n[5:] == 1.0).all()
    assert not np.array_equal(cr.sample_light(1), cr.sample_light(2))
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    # the first draws are those of the documented stream
    rng = np.random.default_rng((7, 2))
    u, phi = rng.random(), rng.uniform(0, 2 * np.pi)
    got = cr.sample_light(7)
    assert abs(got[2] - (1 - u * 0.5)) < 1e-12 and abs(np.arctan2(got[1], got[0]) % (2 * np.pi) - phi) < 1e-9
    assert got[3] == rng.uniform(0.3, 0.6) and got[4] == rng.uniform(0.4, 0.9) and np.array_equal(got[5:], rng.uniform(0.9, 1.0, 3))
    z = np.array([cr.sample_light(s)[2] for s in range(400)])
    assert z.min() < 0.55 and z.max() > 0.97 and abs(z.mean() - 0.75) < 0.03, "uniform on the cap: cos theta uniform in [0.5, 1]"


def test_the_renderers_check_the_light_on_the_host():
    """ValueError before anything is uploaded (the renderers are built on the host here; a good light would need a device)."""
    v, f = mnp.icosphere(0, 10.0)
    col = np.zeros((len(v), 3), dtype=np.uint8)
    proj = NODE_PROJ
    poses = np.stack([snp.pose(np.eye(3), FAR)] * 2)
    good = np.tile([0.0, 0.0, 1.0, 0.4, 0.6, 1.0, 1.0, 1.0], (2, 1))

    def bad_lights():
        yield good[:1]
        yield good[:, :7]
        yield good.reshape(-1)
        for j, val in ((0, np.nan), (3, np.inf), (3, -0.1), (4, -1.0), (5, -0.5), (7, -1e-9), (2, 1.001), (2, 0.999)):
            x = good.copy()
            x[1, j] = val
            yield x

    mesh = cr.CadMeshRenderer(v, f, col, proj, (IH, IW), device="cpu", normals="flat")
    scene = cr.CadSceneRenderer([(v, f, col), (v, f, col)], proj, (IH, IW), [10.0, 10.0], device="cpu", normals="smooth")
    assert mesh.normal_mode == 0 and tuple(mesh.normals.shape) == (len(f), 3)
    assert scene.normal_mode == 1 and tuple(scene.normals.shape) == (2 * len(v), 3)
    for light in bad_lights():
        with pytest.raises(ValueError):
            mesh.render(poses, light=light)
        with pytest.raises(ValueError):
            scene.render(np.stack([poses, poses], axis=1), light=light)
    assert cr.check_light(good, 2).dtype == np.float64
    with pytest.raises(ValueError, match="normals"):
        cr.CadMeshRenderer(v, f, col, proj, (IH, IW), device="cpu").render(poses, light=good)
    with pytest.raises(ValueError, match="normals"):
        cr.CadSceneRenderer([(v, f, col)], proj, (IH, IW), [10.0], device="cpu").render(poses[:, None], light=good)
    # arrays: per triangle or per vertex by their length; one array per mesh, all of one kind
    fn, vn = cr.face_normals(v, f), cr.vertex_normals(v, f)
    assert cr.CadMeshRenderer(v, f, col, proj, (IH, IW), device="cpu", normals=vn).normal_mode == 1
    assert cr.CadSceneRenderer([(v, f, col), (v, f, col)], proj, (IH, IW), [10.0, 10.0], device="cpu", normals=[fn, fn]).normal_mode == 0
    for bad in (dict(normals="phong"), dict(normals=fn[:5]), dict(normals=np.zeros((len(f), 2)))):
        with pytest.raises(ValueError):
            cr.CadMeshRenderer(v, f, col, proj, (IH, IW), device="cpu", **bad)
    with pytest.raises(ValueError):
        cr.CadSceneRenderer([(v, f, col), (v, f, col)], proj, (IH, IW), [10.0, 10.0], device="cpu", normals=[fn, vn])
    with pytest.raises(ValueError):
        cr.CadSceneRenderer([(v, f, col), (v, f, col)], proj, (IH, IW), [10.0, 10.0], device="cpu", normals=[fn])


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return importlib.import_module(name)
    finally:
        sys.path.pop(0)


def test_the_tools_refuse_a_light_for_the_point_renderer(tmp_path, capsys):
    tool = _tool("render_cad_dataset")
    for light in ("head", "random"):
        with pytest.raises(SystemExit) as e:
            tool.main(["--model", str(tmp_path / "m.ply"), "--output_root", str(tmp_path / "out"), "--light", light])
        assert e.value.code == 2 and "--light" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        tool.main(["--model", str(tmp_path / "m.ply"), "--output_root", str(tmp_path / "out"), "--raster", "mesh", "--light", "sun"])
    assert e.value.code == 2
    assert not (tmp_path / "out").exists()
    opt = tool.build_parser().parse_args(["--model", "m.ply", "--output_root", "o"])
    assert opt.light == "none" and opt.shading == "flat" and opt.light_angle == 60.0
    with pytest.raises(SystemExit) as e:
        _tool("cad_render_bench").main(["--light"])
    assert e.value.code == 2
    # a record written with repr parses back to itself
    rec = cr.sample_light(11)
    assert np.array_equal(tool.parse_light(tool.light_text(rec)), rec)
