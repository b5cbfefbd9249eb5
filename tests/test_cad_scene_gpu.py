"""GPU: multi-object customCAD scenes -- ``df_cad_render_scene`` and ``df_cad_scene_mask`` against their numpy restatement
(tests/cad_scene_np.py) bit for bit and against ``df_cad_render_mesh`` for one object, their argument errors, then
tools/render_cad_dataset.py --scene: the trees it writes go through the unchanged loader, whose clouds must lie on each object's own
sphere although other objects cover parts of it, and through tools/train.py --dataset cad and tools/eval_cad.py."""
import importlib
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import cad_raster_np as mnp
import cad_render_np as rnp
import cad_scene_np as snp
import fabricate_cad as fab
from densefusion_amd import synth

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROJ = np.array(fab.PROJ[1])
IH, IW, NODE_PROJ = snp.IH, snp.IW, snp.NODE_PROJ
NAMES = ("rgb", "depth", "label", "stats")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gpu(s, poses, present, dims, cull, proj=NODE_PROJ):
    from densefusion_amd.lib import preprocess as pp
    out = pp.cad_render_scene(_up(s["vertices"]), _up(s["colors"]), _up(s["triangles"]), s["tri_begin"], s["scales"], poses, proj, dims,
                              present=present, cull=cull)
    return tuple(o.cpu().numpy() for o in out)


def _same(got, want):
    for name, g, w in zip(NAMES, got, want[:4]):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


@pytest.fixture(scope="module")
def scene():
    return snp.small_scene()


@gpu
@pytest.mark.parametrize("cull", [0, 1])
def test_scene_equals_the_restatement_bit_for_bit(scene, cull):
    """The fixture of tests/test_cad_scene_host.py::test_the_fixture_has_its_cases; the masks of every (frame, object) pair in both modes."""
    _dev()
    from densefusion_amd.lib import preprocess as pp
    s = scene
    want = snp.render(s["vertices"], s["colors"], s["triangles"], s["tri_begin"], s["scales"], s["poses"], s["present"], NODE_PROJ, IH, IW, cull)
    got = _gpu(s, s["poses"], s["present"], (IH, IW), cull)
    _same(got, want)
    pairs = np.array([[f, o] for f in range(4) for o in range(4)], dtype=np.int32)
    for mode in (0, 1):
        mask = pp.cad_scene_mask(_up(got[2]), _up(got[3]), pairs, mode).cpu().numpy()
        wm = snp.scene_mask(want[2], want[3], pairs, mode)
        assert mask.dtype == wm.dtype and np.array_equal(mask, wm), mode
    assert wm.any()


@gpu
@pytest.mark.parametrize("cull", [0, 1])
def test_large_triangles_of_three_owners_in_one_wave(cull):
    """The fixture of tests/test_cad_scene_host.py::test_the_large_triangle_fixture_has_its_case: six triangles of three objects, all
    walked by the first wave as a whole; the count each walk leaves with one lane goes to that lane's owner."""
    _dev()
    from densefusion_amd.lib import preprocess as pp
    from test_cad_scene_host import large_triangle_scene
    s = large_triangle_scene()
    want = snp.render(s["vertices"], s["colors"], s["triangles"], s["tri_begin"], s["scales"], s["poses"], s["present"], NODE_PROJ, IH, IW, cull)
    got = _gpu(s, s["poses"], s["present"], (IH, IW), cull)
    _same(got, want)
    pairs = np.array([[f, o] for f in range(2) for o in range(3)], dtype=np.int32)
    for mode in (0, 1):
        mask = pp.cad_scene_mask(_up(got[2]), _up(got[3]), pairs, mode).cpu().numpy()
        wm = snp.scene_mask(want[2], want[3], pairs, mode)
        assert mask.dtype == wm.dtype and np.array_equal(mask, wm), mode
    assert wm.any()


@gpu
def test_one_object_equals_the_mesh_rasteriser(scene):
    """O = 1, all present, against ``df_cad_render_mesh`` with K = 0 on the same mesh and poses, on the device: rgb, depth and stats bit
    for bit, and the two masks through ``df_cad_scene_mask`` with one pair per frame."""
    _dev()
    from densefusion_amd.lib import preprocess as pp
    s = scene
    v, c, t = _up(s["vertices"]), _up(s["colors"]), _up(s["triangles"])
    poses = s["poses"][:, 0]
    pairs = np.array([[f, 0] for f in range(4)], dtype=np.int32)
    for cull in (0, 1):
        rgb, depth, label, stats = pp.cad_render_scene(v, c, t, [0, len(s["triangles"])], [10.0], poses[:, None], NODE_PROJ, (IH, IW), cull=cull)
        for mode in (0, 1):
            want = pp.cad_render_mesh(v, c, t, poses, 10.0, NODE_PROJ, (IH, IW), cull=cull, mask_mode=mode)
            assert torch.equal(rgb, want[0]) and torch.equal(depth.view(torch.int16), want[1].view(torch.int16))
            assert torch.equal(stats[:, 0], want[3]) and int(want[3][:, 0].min()) > 0
            mask = pp.cad_scene_mask(label, stats, pairs, mode)
            assert torch.equal(mask.view(torch.int16), want[2].view(torch.int16)) and bool(mask.view(torch.int16).any()), mode
        assert torch.equal(label.view(torch.int16) != 0, depth.view(torch.int16) != -1)      # 65535: the horizon


@gpu
def test_determinism_and_independence(scene):
    """Two identical calls give identical bytes; frame 2 of the F = 4 call equals the F = 1 call of its poses; present = NULL equals an
    all-ones present."""
    _dev()
    s = scene
    a = _gpu(s, s["poses"], s["present"], (IH, IW), 0)
    b = _gpu(s, s["poses"], s["present"], (IH, IW), 0)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    one = _gpu(s, s["poses"][2:3], s["present"][2:3], (IH, IW), 0)
    for name, x, y in zip(NAMES, a, one):
        assert np.array_equal(x[2], y[0]), name
    ones = _gpu(s, s["poses"], np.ones((4, 4), dtype=np.uint8), (IH, IW), 0)
    null = _gpu(s, s["poses"], None, (IH, IW), 0)
    for name, x, y in zip(NAMES, ones, null):
        assert np.array_equal(x, y), name
    assert (null[3][3, [0, 2, 3], 1] > 0).all() and not np.array_equal(null[2], a[2]), "frame 3 is empty only through `present`"


def full_size_scene():
    """520 x 1109, F = 2: object 0 an icosphere of subdivision 5, object 1 a box nearer to the camera over a part of it, object 2 a
    ground quad behind both over more than a quarter of the frame; in frame 1 the sphere is cut by the right edge."""
    sv, sf = mnp.icosphere(5, 60.0)
    bv, bf = snp.box([-20.0, -20.0, -20.0], [20.0, 20.0, 20.0])
    qv, qf = np.array([[-300.0, -120.0, 0.0], [300.0, -120.0, 0.0], [300.0, 120.0, 0.0], [-300.0, 120.0, 0.0]]), np.array([[0, 1, 2], [0, 2, 3]])
    verts, tris, begin = snp.concat_meshes([(sv, sf), (bv, bf), (qv, qf)])
    col = np.random.default_rng(9).integers(0, 256, (len(verts), 3), dtype=np.uint8)
    eye = np.eye(3)
    poses = np.array([[snp.pose(eye, [300.0, -200.0, -3000.0]), snp.pose(eye, [600.0, -200.0, -2400.0]), snp.pose(eye, [0.0, 0.0, -5000.0])],
                      [snp.pose(eye, [2150.0, 100.0, -2700.0]), snp.pose(eye, [1500.0, 150.0, -2000.0]), snp.pose(eye, [500.0, 100.0, -4500.0])]])
    return dict(vertices=verts, colors=col, triangles=tris, tri_begin=begin, scales=np.array([10.0, 10.0, 10.0]), poses=poses)


@gpu
def test_full_size_scene_with_an_occluded_target():
    """Small triangles walked by their lanes, large ones by whole waves, three owners in the resolve pass, more pixels than threads."""
    _dev()
    s = full_size_scene()
    want = snp.render(s["vertices"], s["colors"], s["triangles"], s["tri_begin"], s["scales"], s["poses"], None, PROJ, 520, 1109, 1)
    rgb, depth, label, stats, winner, cover = want
    for f in range(2):
        lost = (cover[f, 0] & (label[f] == 2)).sum()
        print("frame", f, "target won", stats[f, 0, 0], "of", cover[f, 0].sum(), "alone; lost to the box", lost, "; quad won", stats[f, 2, 0])
        assert stats[f, 0, 0] > 5000 and lost > 1000
    assert stats[0, 2, 0] > 520 * 1109 // 4 and stats[1, 0, 5] == 1108
    _same(_gpu(s, s["poses"], None, (520, 1109), 1, proj=PROJ), want)


@gpu
def test_argument_errors_write_nothing():
    _dev()
    from densefusion_amd import _lib
    L = _lib.lib()
    V, T, F, O = 64, 40, 2, 3
    dev = torch.device("cuda")
    vts = torch.rand(V, 3, device=dev)
    col = torch.zeros(V, 3, dtype=torch.uint8, device=dev)
    tri = torch.randint(0, V, (T, 3), dtype=torch.int32, device=dev)
    pose = torch.from_numpy(np.stack([snp.pose(np.eye(3), [0, 0, -4000.0])] * (F * O))).to(dev)
    present = torch.ones(F, O, dtype=torch.uint8, device=dev)
    outs = dict(rgb=torch.full((F, IH, IW, 3), 7, dtype=torch.uint8, device=dev), depth=torch.full((F, IH, IW), 7, dtype=torch.int16, device=dev),
                label=torch.full((F, IH, IW), 7, dtype=torch.int16, device=dev), stats=torch.full((F, O, 6), 7, dtype=torch.int32, device=dev))
    need = L.df_cad_render_scene_scratch_bytes(F, IH, IW, V, T, O)
    assert need == F * IH * IW * 8
    for bad in ((0, IH, IW, V, T, O), (F, 0, IW, V, T, O), (F, IH, -1, V, T, O), (F, IH, IW, 0, T, O), (F, IH, IW, V, 0, O), (F, IH, IW, V, T, 0),
                (F, IH, IW, V, T, 65), (65536, IH, IW, V, T, O)):
        assert L.df_cad_render_scene_scratch_bytes(*bad) == 0
    assert L.df_cad_render_scene_scratch_bytes(F, IH, IW, V, T, 64) == need
    scratch = torch.full((need + 8,), 7, dtype=torch.uint8, device=dev)
    begin = np.array([0, 10, 10, T], dtype=np.int32)
    scales = np.array([10.0, 5.0, 2.0])
    good = dict(vertices=vts.data_ptr(), colors=col.data_ptr(), V=V, triangles=tri.data_ptr(), T=T, tri_begin=begin.ctypes.data,
                model_scale=scales.ctypes.data, O=O, pose=pose.data_ptr(), present=present.data_ptr(), proj=None, F=F, IH=IH, IW=IW, cull=1,
                rgb=outs["rgb"].data_ptr(), depth=outs["depth"].data_ptr(), label=outs["label"].data_ptr(), stats=outs["stats"].data_ptr(),
                scratch=scratch.data_ptr(), scratch_bytes=need, stream=_lib.current_stream())

    def call(**kw):
        proj = kw.pop("proj", PROJ)
        pm = None if proj is None else np.ascontiguousarray(proj, dtype=np.float64)
        a = dict(good, **kw)
        a["proj"] = None if pm is None else pm.ctypes.data
        return L.df_cad_render_scene(*[a[k] for k in good])

    tables = [np.array(t, dtype=np.int32) for t in ([1, 10, 10, T], [0, 12, 10, T], [0, 10, 41, T], [0, 10, 10, T - 1], [0, 10, 10, T + 1],
                                                    [-1, 10, 10, T])]
    big = np.concatenate([np.zeros(65, dtype=np.int32), [T]]).astype(np.int32)
    row2, row3, row3b = PROJ.copy(), PROJ.copy(), PROJ.copy()
    row2[2, 0], row3[3, 2], row3b[3, 3] = 0.1, -2.0, 1.0
    cases = [dict(vertices=None), dict(colors=None), dict(triangles=None), dict(tri_begin=None), dict(model_scale=None), dict(pose=None),
             dict(proj=None), dict(rgb=None), dict(depth=None), dict(label=None), dict(stats=None), dict(scratch=None), dict(cull=-1),
             dict(cull=2), dict(scratch_bytes=need - 1), dict(scratch=scratch.data_ptr() + 4, scratch_bytes=need + 4), dict(V=0), dict(T=0),
             dict(V=-5), dict(T=-1), dict(F=0), dict(F=65536), dict(IH=0), dict(IW=0), dict(O=0), dict(O=-1),
             dict(O=65, tri_begin=big.ctypes.data)] + [dict(tri_begin=t.ctypes.data) for t in tables]
    for kw in cases:
        assert call(**kw) == -1, kw                                       # DF_ERR_ARG
        assert len(L.df_last_error()) > 10, kw
    for pm in (row2, row3, row3b):
        assert call(proj=pm) == -1 and b"projection" in L.df_last_error()
    # df_cad_scene_mask: its own refusals
    pairs = torch.zeros(2, 2, dtype=torch.int32, device=dev)
    mask = torch.full((2, IH, IW), 7, dtype=torch.int16, device=dev)
    margs = dict(label=outs["label"].data_ptr(), stats=outs["stats"].data_ptr(), F=F, O=O, IH=IH, IW=IW, pairs=pairs.data_ptr(), N=2, mode=0,
                 mask=mask.data_ptr(), stream=_lib.current_stream())
    for kw in (dict(label=None), dict(stats=None), dict(pairs=None), dict(mask=None), dict(F=0), dict(O=0), dict(O=65), dict(IH=0), dict(IW=-3),
               dict(N=0), dict(N=-1), dict(mode=2), dict(mode=-1)):
        assert L.df_cad_scene_mask(*dict(margs, **kw).values()) == -1, kw
        assert len(L.df_last_error()) > 10, kw
    torch.cuda.synchronize()
    for name, t in list(outs.items()) + [("scratch", scratch), ("mask", mask)]:
        assert bool((t == 7).all()), name
    assert call() == 0 and call(cull=0, present=None) == 0
    torch.cuda.synchronize()
    assert not bool((outs["stats"] == 7).any()) and not bool((outs["label"] == 7).any())
    assert L.df_cad_scene_mask(*margs.values()) == 0
    torch.cuda.synchronize()
    assert not bool((mask == 7).any())


@gpu
def test_scene_mask_with_pairs_outside_the_scene(scene):
    _dev()
    from densefusion_amd.lib import preprocess as pp
    s = scene
    rgb, depth, label, stats = _gpu(s, s["poses"], s["present"], (IH, IW), 1)
    pairs = np.array([[0, 0], [4, 0], [-1, 0], [0, 4], [0, -1], [2 ** 31 - 1, 0], [0, 2 ** 31 - 1], [-2 ** 31, -2 ** 31], [0, 3], [65535, 64]],
                     dtype=np.int32)
    for mode in (0, 1):
        mask = pp.cad_scene_mask(_up(label), _up(stats), pairs, mode).cpu().numpy()
        assert np.array_equal(mask, snp.scene_mask(label, stats, pairs, mode))
        assert mask[0].any() and mask[8].any() and not mask[1:8].any() and not mask[9].any(), mode


# ---- the tool, the loader, the trainer ---------------------------------------------------------------------------------------------
TREE_DIMS = (96, 144)
RADII = (600.0, 450.0)              # model_scale 10 x the file's radii
MIN_VISIBLE = 0.3
SEED = 0                            # chosen with the restatement (``_np_fractions`` over seeds 0..31: 11 and 9 frames below 0.9)


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return importlib.import_module("render_cad_dataset")
    finally:
        sys.path.pop(0)


def _np_fractions(seed, meshes, proj, n_targets=2):
    """What the tool does for one seed, by the restatement: (present [O], pixels won [O], pixels alone [O]) at the poses of the records."""
    from densefusion_amd.datasets.customCAD import render as cr
    tool = _tool()
    O = len(meshes)
    primary = seed % n_targets
    views, _ = cr.sample_scene(seed, len(meshes[primary][0]), [0.0, 0.0, 4.0], 1.0, O, primary, 3, hole_mean=30.0, hole_std=10.0)
    poses = []
    for o, (here, axis, angle, xyz) in enumerate(views):
        text = tool.record_text(0, *cr.pose_to_transform(*cr.view_pose(axis, angle, xyz, meshes[o][0].astype(np.float64).mean(axis=0), 10.0)))
        R, t = cr.transform_to_pose(*tool.parse_record(text))
        poses.append(snp.pose(R, t))
    present = np.array([v[0] for v in views], dtype=np.uint8)
    verts, tris, begin = snp.concat_meshes([(m[0], m[1]) for m in meshes])
    out = snp.render_frame(verts, np.concatenate([m[2] for m in meshes]), tris, begin, [10.0] * O, np.stack(poses), present, proj,
                           TREE_DIMS[0], TREE_DIMS[1], 1)
    return present, out[3][:, 0], out[5].sum(axis=(1, 2))


@pytest.fixture(scope="module")
def scene_models(tmp_path_factory):
    root = tmp_path_factory.mktemp("scene_models")
    meshes = snp.tool_meshes()
    paths = [mnp.write_mesh_ply(root / name, *[m[k] for k in (0, 1, 2)]) for name, m in zip(("big.ply", "small.ply", "box.ply"), meshes)]
    return paths, meshes, root, rnp.write_proj(root / "proj_in.txt", fab.PROJ[1])


def _render_trees(scene_models, name, mask):
    _dev()
    paths, meshes, root, pm = scene_models
    tree = str(root / name)
    summary = _tool().main(["--scene", "--model", paths[0], paths[1], "--distractor", paths[2], "--output_root", tree, "--frames", "24",
                            "--proj_mat", pm, "--height", str(TREE_DIMS[0]), "--width", str(TREE_DIMS[1]), "--min_pixels", "200",
                            "--min_visible", str(MIN_VISIBLE), "--mask", mask, "--chunk", "16", "--seed", str(SEED)])
    return tree, summary


@pytest.fixture(scope="module")
def scene_trees(scene_models):
    """tools/render_cad_dataset.py --scene --mask pixels: two models and a box distractor, 24 frames of 96 x 144 per model."""
    return _render_trees(scene_models, "tree_pixels", "pixels")


def _off_sphere(tree, obj, mesh, radius):
    """Per training frame of ``data/obj``: the largest distance of a cloud point from the shell between ``radius`` - sagitta and
    ``radius`` around the record's own t_cam, over the bound of test_mesh_tree_through_the_loader (half a grid step and half a depth
    code at the point's own depth, + 1e-3 for the loader's float32).  Returns (frame numbers, worst offset / bound per frame)."""
    from densefusion_amd.datasets.customCAD import render as cr
    from densefusion_amd.datasets.customCAD.dataset import PoseDataset
    v, f = mesh[0], mesh[1]
    a, b, c = (v[f[:, k]].astype(np.float64) * 10.0 for k in range(3))
    nrm = np.cross(b - a, c - a)
    sagitta = radius - (np.abs((nrm * a).sum(axis=1)) / np.linalg.norm(nrm, axis=1)).min()
    assert 0.5 < sagitta < 0.03 * radius, sagitta
    np.random.seed(1)
    ds = PoseDataset("train", 500, False, tree, 0.0, False, objlist=(obj,))
    rows = list(range(len(ds)))
    assert len(rows) == 19 and ds.udp[obj].image_dims == TREE_DIMS, "80 % of 24 frames"
    frames, worst = [], []
    for i, item in zip(rows, ds.batch(rows)):
        cloud = item[0]
        assert cloud.dim() == 2 and tuple(cloud.shape) == (500, 3), "the sentinel"
        R, t_cam = cr.transform_to_pose(*ds.meta[obj][ds.list_meta[i] + 1])
        p = cloud.double().cpu().numpy() * 10000
        bx, by, bz = rnp.grid_bounds(p[:, 2], fab.PROJ[1], *TREE_DIMS)
        dist = np.linalg.norm(p - t_cam, axis=1)
        off = np.maximum(np.maximum(dist - radius, (radius - sagitta) - dist), 0.0)
        bound = np.sqrt(bx * bx + by * by + bz * bz) * (1 + 1e-6) + 1e-3
        frames.append(ds.list_meta[i]); worst.append(float((off / bound).max()))
    return frames, np.array(worst)


@gpu
def test_scene_trees_hold_occluded_frames(scene_trees, scene_models):
    """From the tool's summary: 24 frames per model, at least three of them less than 0.9 visible and none below --min_visible.  The
    start seed was chosen with the restatement; the first frames written to each tree are recomputed with it here, and the tool's
    visible fractions must be exactly the restatement's."""
    tree, summary = scene_trees
    paths, meshes, root, pm = scene_models
    from densefusion_amd.datasets.customCAD.project_unity_depth import read_proj_mat
    proj = read_proj_mat(os.path.join(tree, "data", "01", "meta", "proj_mat.txt"))
    for k in (1, 2):
        got = summary["objects"][k]
        vis = np.array(got["visible"])
        print("object", k, "visible fractions", np.round(vis, 3).tolist())
        assert got["written"] == 24 and len(vis) == 24
        assert (vis < 0.9).sum() >= 3 and (vis >= MIN_VISIBLE).all() and (vis <= 1.0).all()
        assert abs(got["mean_visible"] - vis.mean()) < 1e-12
        for seed, frac in list(zip(got["seeds"], got["visible"]))[:3]:
            present, won, alone = _np_fractions(seed, meshes, proj)
            assert present[k - 1] and won[k - 1] >= 200 and frac == won[k - 1] / alone[k - 1], (k, seed)
        sub = os.path.join(tree, "data", "%02d" % k)
        train = [int(x) for x in open(os.path.join(sub, "train.txt")).read().split()]
        test = [int(x) for x in open(os.path.join(sub, "test.txt")).read().split()]
        assert len(train) == 19 and len(test) == 5 and sorted(train + test) == list(range(24))
    assert not os.path.exists(os.path.join(tree, "data", "03")) and not os.path.exists(os.path.join(tree, "models", "obj_03.ply"))


@gpu
def test_scene_trees_through_the_loader(scene_trees, scene_models):
    """--mask pixels: every cloud point of every training frame of either tree lies on that object's own sphere around the record's own
    t_cam, within the bound of test_mesh_tree_through_the_loader -- with occluders in view, the check that covered pixels never reach
    the cloud."""
    tree, summary = scene_trees
    meshes = scene_models[1]
    for k in (1, 2):
        frames, worst = _off_sphere(tree, k, meshes[k - 1], RADII[k - 1])
        vis = np.array(summary["objects"][k]["visible"])[frames]
        print("object", k, "worst cloud offset / bound", worst.max(), "over", len(frames), "frames,", (vis < 0.9).sum(), "of them occluded")
        assert (vis < 0.9).any(), "occluded frames are among the training frames"
        assert (worst <= 1.0).all(), (k, worst.max())


@gpu
def test_box_masks_let_occluders_into_the_cloud(scene_models):
    """--mask box on the same seeds marks the occluder's pixels inside the box as the object (the reference's rule): the same check
    finds points off the sphere in at least one occluded frame -- it tells the two modes apart."""
    tree, summary = _render_trees(scene_models, "tree_box", "box")
    meshes = scene_models[1]
    found = 0
    for k in (1, 2):
        frames, worst = _off_sphere(tree, k, meshes[k - 1], RADII[k - 1])
        vis = np.array(summary["objects"][k]["visible"])[frames]
        found += int(((worst > 1.0) & (vis < 0.9)).sum())
        print("object", k, "frames with points off the sphere", int((worst > 1.0).sum()), "occluded", int((vis < 0.9).sum()))
    assert found >= 1


@gpu
def test_train_and_eval_tools_on_scene_trees(scene_trees, tmp_path):
    """tools/train.py --dataset cad for two optimizer steps (19 // 8: it reads object 1, as the reference does), then tools/eval_cad.py
    over both objects, on the two-object tree: both exit 0."""
    tree, _ = scene_trees
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--dataset", "cad", "--dataset_root", tree, "--nepoch", "2", "--batch_size", "8",
           "--workers", "2", "--feed", "threads", "--jitter", "host", "--outf", str(out / "models"), "--log_dir", str(out / "logs"), "--decay_margin", "0",
           "--refine_margin", "0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = r.stdout + r.stderr
    dists = [float(x) for x in re.findall(r"Batch \d+ Frame \d+ Avg_dis:(\S+)", log)]
    assert len(dists) == 2 and all(math.isfinite(d) and d > 0 for d in dists), log[-3000:]
    assert "length of the training set: 19" in log
    ckpt = [f for f in os.listdir(out / "models") if f.startswith("pose_model_")]
    assert ckpt, os.listdir(out / "models")
    sdr = synth.make_state_dict(synth.refiner_spec(5), 1031)
    torch.save({k: torch.from_numpy(x) for k, x in sdr.items()}, tmp_path / "r.pth")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_cad.py"), "--dataset_root", tree, "--model", str(out / "models" / sorted(ckpt)[0]),
                        "--refine_model", str(tmp_path / "r.pth"), "--output_result_dir", str(tmp_path / "eval"), "--workers", "0", "--objlist", "1,2"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL success rate" in open(tmp_path / "eval" / "eval_result_logs.txt").read()
