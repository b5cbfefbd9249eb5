"""GPU: diffuse lighting of the customCAD triangle renderers -- ``df_cad_render_mesh_lit`` and ``df_cad_render_scene_lit`` against the
numpy restatement of steps L1..L6 (tests/cad_light_np.py) bit for bit and against the unlit entry points, their argument errors, then
tools/render_cad_dataset.py --light: the lit trees go through the unchanged loader, which must see the geometry of the unlit trees."""
import filecmp
import importlib
import os
import random
import sys

import numpy as np
import pytest
import torch

import cad_light_np as lnp
import cad_raster_np as mnp
import cad_render_np as rnp
import cad_scene_np as snp
import fabricate_cad as fab
from test_cad_light_host import scene_normals

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROJ = np.array(fab.PROJ[1])
IH, IW, NODE_PROJ = snp.IH, snp.IW, snp.NODE_PROJ

# one record per frame of the four-frame fixtures: an oblique tinted light; one that points away from what the camera sees, so that L4
# clamps; one with ambient + diffuse > 1 and a colour above 1, so that L6 saturates; a dim head-light
LIGHTS = np.array([[0.48, 0.36, 0.8, 0.3, 0.7, 1.0, 0.9, 0.8],
                   [0.6, 0.0, -0.8, 0.35, 0.9, 0.8, 1.0, 0.9],
                   [0.0, 0.6, 0.8, 0.9, 0.8, 1.2, 1.0, 1.0],
                   [0.0, 0.0, 1.0, 0.1, 0.5, 1.0, 1.0, 1.0]])


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _scene_gpu(s, poses, present, cull, normals=None, mode=0, light=None):
    from densefusion_amd.lib import preprocess as pp
    out = pp.cad_render_scene(_up(s["vertices"]), _up(s["colors"]), _up(s["triangles"]), s["tri_begin"], s["scales"], poses, NODE_PROJ,
                              (IH, IW), present=present, cull=cull, normals=None if normals is None else _up(normals), normal_mode=mode,
                              light=light)
    return tuple(o.cpu().numpy() for o in out)


def _mesh_gpu(verts, col, tris, poses, holes, cull, mask_mode, normals=None, mode=0, light=None):
    from densefusion_amd.lib import preprocess as pp
    out = pp.cad_render_mesh(_up(verts), _up(col), _up(tris), poses, 10.0, NODE_PROJ, (IH, IW), holes=holes, cull=cull, mask_mode=mask_mode,
                             normals=None if normals is None else _up(normals), normal_mode=mode, light=light)
    return tuple(o.cpu().numpy() for o in out)


def _same(got, want, names):
    for name, g, w in zip(names, got, want[:4]):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


@pytest.fixture(scope="module")
def scene():
    return snp.small_scene()


@pytest.fixture(scope="module")
def mesh():
    """The fixture of tests/test_cad_raster_gpu.py (about 300 triangles, four poses, K = 3 holes) with its two kinds of normals; the
    triangles with an index outside 0..V-1 win nothing, and their per-triangle normals are taken through clipped indices."""
    from test_cad_raster_gpu import small_scene
    verts, col, tris, poses, holes, _ = small_scene()
    safe = tris.clip(0, len(verts) - 1)
    from densefusion_amd.datasets.customCAD import render as cr
    return dict(verts=verts, col=col, tris=tris, poses=poses, holes=holes, normals=(cr.face_normals(verts, safe), cr.vertex_normals(verts, safe)))


@gpu
@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
def test_lit_scene_equals_the_restatement_bit_for_bit(scene, mode, cull):
    _dev()
    s = scene
    nrm = scene_normals(s, mode)
    want = lnp.render_scene(s["vertices"], s["colors"], s["triangles"], s["tri_begin"], s["scales"], s["poses"], s["present"], NODE_PROJ,
                            IH, IW, cull, nrm, mode, LIGHTS)
    unlit_np = snp.render(s["vertices"], s["colors"], s["triangles"], s["tri_begin"], s["scales"], s["poses"], s["present"], NODE_PROJ,
                          IH, IW, cull)
    covered = want[4] >= 0
    # the cases are in the fixture: frame 1 holds pixels at ambient only (L4 clamped), frame 2 pixels at 255 that the unlit frame has below
    dim = LIGHTS.copy()
    dim[:, 4] = 0.0
    amb = lnp.render_scene(s["vertices"], s["colors"], s["triangles"], s["tri_begin"], s["scales"], s["poses"], s["present"], NODE_PROJ,
                           IH, IW, cull, nrm, mode, dim)[0][1]
    clamped = (want[0][1] == amb).all(axis=2) & covered[1]
    assert clamped.sum() > 300 and (covered[1] & ~clamped).sum() > 200
    assert ((want[0][2] == 255) & (unlit_np[0][2] < 255))[covered[2]].sum() > 100
    assert not np.array_equal(want[0][:3], unlit_np[0][:3]) and np.array_equal(want[0][3], unlit_np[0][3])
    got = _scene_gpu(s, s["poses"], s["present"], cull, nrm, mode, LIGHTS)
    _same(got, want, ("rgb", "depth", "label", "stats"))
    unlit = _scene_gpu(s, s["poses"], s["present"], cull)
    for name, g, u in list(zip(("rgb", "depth", "label", "stats"), got, unlit))[1:]:
        assert np.array_equal(g, u), name
    assert np.array_equal(got[0][~covered], unlit[0][~covered]) and (got[0][~covered] == 130).all()


@gpu
@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("mode", [0, 1])
def test_lit_mesh_with_holes_equals_the_restatement_bit_for_bit(mesh, mode, cull):
    _dev()
    m = mesh
    want = lnp.render_mesh(m["verts"], m["col"], m["tris"], m["poses"], 10.0, m["holes"], NODE_PROJ, IH, IW, cull, 1, m["normals"][mode], mode,
                           LIGHTS)
    assert (want[3][:3, 0] > 0).all()
    got = _mesh_gpu(m["verts"], m["col"], m["tris"], m["poses"], m["holes"], cull, 1, m["normals"][mode], mode, LIGHTS)
    _same(got, want, ("rgb", "depth", "mask", "stats"))
    unlit = _mesh_gpu(m["verts"], m["col"], m["tris"], m["poses"], m["holes"], cull, 1)
    for name, g, u in list(zip(("rgb", "depth", "mask", "stats"), got, unlit))[1:]:
        assert np.array_equal(g, u), name
    assert not np.array_equal(got[0], unlit[0])


@gpu
def test_lit_scene_of_one_object_equals_the_lit_mesh_call(scene):
    _dev()
    from densefusion_amd.lib import preprocess as pp
    s = scene
    v, c, t = _up(s["vertices"]), _up(s["colors"]), _up(s["triangles"])
    poses = s["poses"][:, 0]
    for mode in (0, 1):
        n = _up(scene_normals(s, mode))
        for cull in (0, 1):
            a = pp.cad_render_scene(v, c, t, [0, len(s["triangles"])], [10.0], poses[:, None], NODE_PROJ, (IH, IW), cull=cull, normals=n,
                                    normal_mode=mode, light=LIGHTS)
            b = pp.cad_render_mesh(v, c, t, poses, 10.0, NODE_PROJ, (IH, IW), cull=cull, normals=n, normal_mode=mode, light=LIGHTS)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int16), b[1].view(torch.int16)) and torch.equal(a[3][:, 0], b[3])
            assert int(b[3][:, 0].min()) > 0
            assert not torch.equal(b[0], pp.cad_render_mesh(v, c, t, poses, 10.0, NODE_PROJ, (IH, IW), cull=cull)[0])


def _raw_mesh(L, lit, m, F, normals, mode, light, outs, scratch):
    """``df_cad_render_mesh`` / ``df_cad_render_mesh_lit`` through ctypes; normals and light are device tensors or None (NULL)"""
    from densefusion_amd import _lib
    K = m["holes"][0].shape[1]
    hole_idx, hole_r = np.ascontiguousarray(m["holes"][0][:F], dtype=np.int32), np.ascontiguousarray(m["holes"][1][:F], dtype=np.float64)
    proj = np.ascontiguousarray(NODE_PROJ, dtype=np.float64)
    head = (m["d_verts"].data_ptr(), m["d_col"].data_ptr(), len(m["verts"]), m["d_tris"].data_ptr(), len(m["tris"]), m["d_poses"].data_ptr(), 10.0,
            hole_idx.ctypes.data, hole_r.ctypes.data, K, proj.ctypes.data, F, IH, IW, 0, 1)
    tail = tuple(o.data_ptr() for o in outs) + (scratch.data_ptr(), scratch.numel(), _lib.current_stream())
    if not lit:
        return L.df_cad_render_mesh(*head, *tail)
    return L.df_cad_render_mesh_lit(*head, None if normals is None else normals.data_ptr(), mode, None if light is None else light.data_ptr(), *tail)


def _fresh(F, rows, fill=7):
    dev = torch.device("cuda")
    return [torch.full((F, IH, IW, 3), fill, dtype=torch.uint8, device=dev), torch.full((F, IH, IW), fill, dtype=torch.int16, device=dev),
            torch.full((F, IH, IW), fill, dtype=torch.int16, device=dev), torch.full((F,) + rows, fill, dtype=torch.int32, device=dev)]


@gpu
def test_identity_record_and_null_light_give_the_unlit_call(mesh, scene):
    """The record {., ., ., 1, 0, 1, 1, 1} gives the unlit bytes in both modes; light = NULL through the lit entry points (normals NULL,
    normal_mode out of range: ignored) gives every output of the unlit entry points."""
    _dev()
    from densefusion_amd import _lib
    m, s = mesh, scene
    rec = np.tile(lnp.IDENTITY, (4, 1))
    rec[:, :3] = [[0, 0, 1], [0.6, 0, 0.8], [0, -1, 0], [1, 0, 0]]
    unlit = _mesh_gpu(m["verts"], m["col"], m["tris"], m["poses"], m["holes"], 0, 1)
    unlit_s = _scene_gpu(s, s["poses"], s["present"], 0)
    for mode in (0, 1):
        got = _mesh_gpu(m["verts"], m["col"], m["tris"], m["poses"], m["holes"], 0, 1, m["normals"][mode], mode, rec)
        for g, u in zip(got, unlit):
            assert g.tobytes() == u.tobytes(), mode
        got = _scene_gpu(s, s["poses"], s["present"], 0, scene_normals(s, mode), mode, rec)
        for g, u in zip(got, unlit_s):
            assert g.tobytes() == u.tobytes(), mode
    L = _lib.lib()
    md = dict(m, d_verts=_up(m["verts"]), d_col=_up(m["col"]), d_tris=_up(m["tris"]), d_poses=_up(m["poses"]))
    scratch = torch.empty(4 * IH * IW * 8, dtype=torch.uint8, device="cuda")
    a, b = _fresh(4, (6,)), _fresh(4, (6,), fill=9)
    assert _raw_mesh(L, False, md, 4, None, 0, None, a, scratch) == 0
    assert _raw_mesh(L, True, md, 4, None, 5, None, b, scratch) == 0
    torch.cuda.synchronize()
    for x, y, u in zip(a, b, unlit):
        assert torch.equal(x, y) and x.cpu().numpy().tobytes() == u.tobytes()
    # the scene: the unlit wrapper against the lit entry point with light = NULL
    begin, scales = np.ascontiguousarray(s["tri_begin"], dtype=np.int32), np.ascontiguousarray(s["scales"], dtype=np.float64)
    proj = np.ascontiguousarray(NODE_PROJ, dtype=np.float64)
    v, c, t, p, pr = _up(s["vertices"]), _up(s["colors"]), _up(s["triangles"]), _up(s["poses"]), _up(s["present"])
    outs = _fresh(4, (4, 6))
    st = L.df_cad_render_scene_lit(v.data_ptr(), c.data_ptr(), len(s["vertices"]), t.data_ptr(), len(s["triangles"]), begin.ctypes.data,
                                   scales.ctypes.data, 4, p.data_ptr(), pr.data_ptr(), proj.ctypes.data, 4, IH, IW, 0, None, -3, None,
                                   *[o.data_ptr() for o in outs], scratch.data_ptr(), scratch.numel(), _lib.current_stream())
    assert st == 0
    torch.cuda.synchronize()
    for x, u in zip(outs, unlit_s):
        assert x.cpu().numpy().tobytes() == u.tobytes()


@gpu
def test_a_nan_record_blacks_its_frame_only(scene):
    """Through ``preprocess.cad_render_scene`` (the renderer classes refuse such a light on the host): ambient = NaN in frame 1 makes s
    NaN, every channel of its covered pixels 0 (L6), and leaves the horizon and the other frames as they are."""
    _dev()
    s = scene
    nrm = scene_normals(s, 1)
    good = _scene_gpu(s, s["poses"], s["present"], 0, nrm, 1, LIGHTS)
    bad = LIGHTS.copy()
    bad[1, 3] = np.nan
    got = _scene_gpu(s, s["poses"], s["present"], 0, nrm, 1, bad)
    covered = got[2][1] != 0
    assert covered.sum() > 300 and (got[0][1][covered] == 0).all() and (got[0][1][~covered] == 130).all()
    for f in (0, 2, 3):
        assert np.array_equal(got[0][f], good[0][f]), f
    for g, w in zip(got[1:], good[1:]):
        assert np.array_equal(g, w)
    want = lnp.render_scene(s["vertices"], s["colors"], s["triangles"], s["tri_begin"], s["scales"], s["poses"], s["present"], NODE_PROJ,
                            IH, IW, 0, nrm, 1, bad)
    assert np.array_equal(got[0], want[0])
    # a NaN direction: L4 gives 0, the frame is lit by its ambient term alone
    bad = LIGHTS.copy()
    bad[0, 0] = np.nan
    got = _scene_gpu(s, s["poses"], s["present"], 0, nrm, 1, bad)
    only = LIGHTS.copy()
    only[0, 4] = 0.0
    assert np.array_equal(got[0], _scene_gpu(s, s["poses"], s["present"], 0, nrm, 1, only)[0])


@gpu
def test_determinism_and_frame_independence(scene, mesh):
    """Two identical calls give identical bytes; a frame rendered alone, with its own light record and pose, equals its rows in the
    four-frame call: light[f] and pose[f] are indexed by the frame."""
    _dev()
    s, m = scene, mesh
    nrm = scene_normals(s, 1)
    a = _scene_gpu(s, s["poses"], s["present"], 0, nrm, 1, LIGHTS)
    b = _scene_gpu(s, s["poses"], s["present"], 0, nrm, 1, LIGHTS)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    for f in range(3):
        one = _scene_gpu(s, s["poses"][f:f + 1], s["present"][f:f + 1], 0, nrm, 1, LIGHTS[f:f + 1])
        for x, y in zip(a, one):
            assert np.array_equal(x[f], y[0]), f
    assert not np.array_equal(a[0][2], _scene_gpu(s, s["poses"][2:3], s["present"][2:3], 0, nrm, 1, LIGHTS[:1])[0][0]), "the record matters"
    c = _mesh_gpu(m["verts"], m["col"], m["tris"], m["poses"], m["holes"], 0, 0, m["normals"][0], 0, LIGHTS)
    for f in range(3):
        one = _mesh_gpu(m["verts"], m["col"], m["tris"], m["poses"][f:f + 1], (m["holes"][0][f:f + 1], m["holes"][1][f:f + 1]), 0, 0,
                        m["normals"][0], 0, LIGHTS[f:f + 1])
        for x, y in zip(c, one):
            assert np.array_equal(x[f], y[0]), f


@gpu
def test_argument_errors_write_nothing(mesh, scene):
    """A light without normals and a normal_mode outside 0..1 are DF_ERR_ARG in both calls, as is everything the unlit calls refuse;
    nothing is written: the outputs and the scratch keep the 7s they were filled with."""
    _dev()
    from densefusion_amd import _lib
    L = _lib.lib()
    m, s = mesh, scene
    F = 2
    dev = torch.device("cuda")
    light = _up(LIGHTS[:F])
    need = L.df_cad_render_mesh_scratch_bytes(F, IH, IW, len(m["verts"]), len(m["tris"]))
    assert need == F * IH * IW * 8 == L.df_cad_render_scene_scratch_bytes(F, IH, IW, len(s["vertices"]), len(s["triangles"]), 4)
    scratch = torch.full((need + 8,), 7, dtype=torch.uint8, device=dev)
    hole_idx, hole_r = np.ascontiguousarray(m["holes"][0][:F]), np.ascontiguousarray(m["holes"][1][:F])
    proj = np.ascontiguousarray(NODE_PROJ, dtype=np.float64)
    bad_proj = proj.copy()
    bad_proj[3, 3] = 1.0
    tens = dict(v=_up(m["verts"]), c=_up(m["col"]), t=_up(m["tris"]), p=_up(m["poses"][:F]), n0=_up(m["normals"][0]), n1=_up(m["normals"][1]))
    outs = _fresh(F, (6,))
    good = dict(vertices=tens["v"].data_ptr(), colors=tens["c"].data_ptr(), V=len(m["verts"]), triangles=tens["t"].data_ptr(), T=len(m["tris"]),
                pose=tens["p"].data_ptr(), model_scale=10.0, hole_idx=hole_idx.ctypes.data, hole_r=hole_r.ctypes.data, K=3, proj=proj.ctypes.data,
                F=F, IH=IH, IW=IW, cull=1, mask_mode=0, normals=tens["n0"].data_ptr(), normal_mode=0, light=light.data_ptr(),
                rgb=outs[0].data_ptr(), depth=outs[1].data_ptr(), mask=outs[2].data_ptr(), stats=outs[3].data_ptr(), scratch=scratch.data_ptr(),
                scratch_bytes=need, stream=_lib.current_stream())
    cases = [dict(normals=None), dict(normal_mode=2), dict(normal_mode=-1), dict(normals=None, normal_mode=1), dict(vertices=None), dict(colors=None),
             dict(triangles=None), dict(pose=None), dict(proj=None), dict(rgb=None), dict(depth=None), dict(mask=None), dict(stats=None),
             dict(scratch=None), dict(hole_idx=None), dict(cull=2), dict(mask_mode=-1), dict(scratch_bytes=need - 1),
             dict(scratch=scratch.data_ptr() + 4, scratch_bytes=need + 4), dict(V=0), dict(T=0), dict(F=0), dict(F=65536), dict(IH=0), dict(IW=0),
             dict(K=129), dict(proj=bad_proj.ctypes.data), dict(light=None, cull=2), dict(light=None, F=0)]
    for kw in cases:
        assert L.df_cad_render_mesh_lit(*dict(good, **kw).values()) == -1, kw                  # DF_ERR_ARG
        assert len(L.df_last_error()) > 10 and b"cad_render_mesh_lit" in L.df_last_error(), kw
    # the scene call
    begin, scales = np.ascontiguousarray(s["tri_begin"], dtype=np.int32), np.ascontiguousarray(s["scales"], dtype=np.float64)
    st = dict(v=_up(s["vertices"]), c=_up(s["colors"]), t=_up(s["triangles"]), p=_up(s["poses"][:F]), pr=_up(s["present"][:F]),
              n=_up(scene_normals(s, 1)))
    souts = _fresh(F, (4, 6))
    sgood = dict(vertices=st["v"].data_ptr(), colors=st["c"].data_ptr(), V=len(s["vertices"]), triangles=st["t"].data_ptr(), T=len(s["triangles"]),
                 tri_begin=begin.ctypes.data, model_scale=scales.ctypes.data, O=4, pose=st["p"].data_ptr(), present=st["pr"].data_ptr(),
                 proj=proj.ctypes.data, F=F, IH=IH, IW=IW, cull=1, normals=st["n"].data_ptr(), normal_mode=1, light=light.data_ptr(),
                 rgb=souts[0].data_ptr(), depth=souts[1].data_ptr(), label=souts[2].data_ptr(), stats=souts[3].data_ptr(),
                 scratch=scratch.data_ptr(), scratch_bytes=need, stream=_lib.current_stream())
    wrong = begin.copy()
    wrong[4] -= 1
    scases = [dict(normals=None), dict(normal_mode=2), dict(normal_mode=-1), dict(vertices=None), dict(tri_begin=None), dict(model_scale=None),
              dict(pose=None), dict(proj=None), dict(rgb=None), dict(label=None), dict(stats=None), dict(scratch=None), dict(cull=-1), dict(O=0),
              dict(O=65), dict(scratch_bytes=need - 1), dict(V=0), dict(T=0), dict(F=0), dict(IH=0), dict(tri_begin=wrong.ctypes.data),
              dict(proj=bad_proj.ctypes.data), dict(light=None, cull=2)]
    for kw in scases:
        assert L.df_cad_render_scene_lit(*dict(sgood, **kw).values()) == -1, kw
        assert len(L.df_last_error()) > 10 and b"cad_render_scene_lit" in L.df_last_error(), kw
    torch.cuda.synchronize()
    for name, t in [("mesh %d" % k, o) for k, o in enumerate(outs)] + [("scene %d" % k, o) for k, o in enumerate(souts)] + [("scratch", scratch)]:
        assert bool((t == 7).all()), name
    assert L.df_cad_render_mesh_lit(*good.values()) == 0 and L.df_cad_render_mesh_lit(*dict(good, normals=tens["n1"].data_ptr(), normal_mode=1).values()) == 0
    assert L.df_cad_render_scene_lit(*sgood.values()) == 0 and L.df_cad_render_scene_lit(*dict(sgood, present=None, cull=0).values()) == 0
    torch.cuda.synchronize()
    assert not bool((outs[3] == 7).all(dim=-1).any()) and not bool((souts[3] == 7).all(dim=-1).any()) and not bool((souts[2] == 7).any())


# ---- the tool and the loader -------------------------------------------------------------------------------------------------------
TREE_DIMS = (96, 144)
FRAMES = 6


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return importlib.import_module("render_cad_dataset")
    finally:
        sys.path.pop(0)


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """tools/render_cad_dataset.py --scene on the meshes of the scene tool's test (two models, a box distractor), 6 frames of 96 x 144
    per model from the same seeds: without the flag, with --light none, and with --light random --shading smooth."""
    _dev()
    root = tmp_path_factory.mktemp("light_trees")
    meshes = snp.tool_meshes()
    paths = [mnp.write_mesh_ply(root / name, *[m[k] for k in (0, 1, 2)]) for name, m in zip(("big.ply", "small.ply", "box.ply"), meshes)]
    pm = rnp.write_proj(root / "proj_in.txt", fab.PROJ[1])
    out = {}
    for name, extra in (("plain", []), ("none", ["--light", "none"]), ("lit", ["--light", "random", "--shading", "smooth"])):
        tree = str(root / name)
        summary = _tool().main(["--scene", "--model", paths[0], paths[1], "--distractor", paths[2], "--output_root", tree, "--frames", str(FRAMES),
                                "--proj_mat", pm, "--height", str(TREE_DIMS[0]), "--width", str(TREE_DIMS[1]), "--min_pixels", "200",
                                "--mask", "pixels", "--chunk", "8", "--seed", "0"] + extra)
        out[name] = (tree, summary)
    return out


def _files(tree):
    return sorted(os.path.relpath(os.path.join(d, f), tree) for d, _, fs in os.walk(tree) for f in fs)


@gpu
def test_light_none_writes_the_tree_of_today(trees):
    plain, none = trees["plain"][0], trees["none"][0]
    names = _files(plain)
    assert names == _files(none) and len(names) == 2 * (3 * FRAMES + 4) + 2 and not any("lights" in n for n in names)
    match, mismatch, errors = filecmp.cmpfiles(plain, none, names, shallow=False)
    assert not mismatch and not errors and len(match) == len(names)
    assert trees["plain"][1]["objects"][1]["seeds"] == trees["none"][1]["objects"][1]["seeds"]


@gpu
def test_lights_txt_holds_the_records_of_the_seeds(trees):
    from densefusion_amd.datasets.customCAD import render as cr
    tree, summary = trees["lit"]
    assert _files(tree) == sorted(_files(trees["plain"][0]) + ["data/01/meta/lights.txt", "data/02/meta/lights.txt"])
    for k in (1, 2):
        seeds = summary["objects"][k]["seeds"]
        assert seeds == trees["plain"][1]["objects"][k]["seeds"] and len(seeds) == FRAMES, "lighting changes no geometry: the same views enter"
        lines = open(os.path.join(tree, "data", "%02d" % k, "meta", "lights.txt")).read().splitlines()
        assert len(lines) == FRAMES
        for n, (line, seed) in enumerate(zip(lines, seeds)):
            tok = line.split()
            assert int(tok[0]) == n and len(tok) == 9
            assert np.array_equal(np.array([float(x) for x in tok[1:]]), cr.sample_light(seed)), (k, n)


@gpu
def test_lit_tree_through_the_loader(trees):
    """The unchanged ``PoseDataset`` on the lit and on the unlit tree of the same seeds: cloud, choose, target and model_points are
    equal (depth and masks are), the image is not."""
    from densefusion_amd.datasets.customCAD.dataset import PoseDataset
    for k in (1, 2):
        for name in ("rgb", "depth", "mask"):
            sub = os.path.join("data", "%02d" % k, name)
            files = sorted(os.listdir(os.path.join(trees["plain"][0], sub)))
            same = filecmp.cmpfiles(os.path.join(trees["plain"][0], sub), os.path.join(trees["lit"][0], sub), files, shallow=False)[0]
            assert len(files) == FRAMES and (len(same) == 0 if name == "rgb" else len(same) == FRAMES), (k, name)
        items = {}
        for name in ("plain", "lit"):
            np.random.seed(1)                    # the loader samples the model with np.random and its subset with random
            random.seed(1)
            ds = PoseDataset("train", 500, False, trees[name][0], 0.0, False, objlist=(k,))
            assert len(ds) == 4, "80 % of 6 frames"
            items[name] = ds.batch(list(range(len(ds))))
        for a, b in zip(items["plain"], items["lit"]):
            cloud, choose, img, target, model_points, idx = a
            assert tuple(cloud.shape) == (500, 3), "the sentinel"
            for j in (0, 1, 3, 4, 5):
                assert torch.equal(a[j], b[j]), (k, j)
            assert a[2].shape == b[2].shape and not torch.equal(a[2], b[2])
