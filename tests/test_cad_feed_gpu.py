"""GPU: training on customCAD views rendered on the fly.  ``df_cad_item_table`` and ``df_cad_targets`` against their numpy restatement
(tests/cad_feed_np.py) bit for bit; ``RenderedPoseDataset`` against the disk loader over trees tools/render_cad_dataset.py writes from
the same seeds; its purity; tools/train.py --dataset cad_render."""
import importlib
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import cad_feed_np as fnp
import cad_np
import cad_raster_np as mnp
import cad_render_np as rnp
import cad_scene_np as snp
import fabricate_cad as fab

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _up16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


# ---- df_cad_item_table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["9x9", "12x20", "130x257"])
def test_item_table_equals_the_restatement_bit_for_bit(name):
    _dev()
    from densefusion_amd.lib import preprocess as pp
    depth, label = fnp.table_frames()[name]
    want = fnp.item_table(depth, label, 65535, 8)
    got = pp.cad_item_table(_up16(depth), _up16(label)).cpu().numpy()
    assert got.dtype == np.int32 and got.tolist() == want.tolist()
    stats = pp.cad_frame_stats(_up16(depth), _up16(label)).cpu().numpy()
    assert np.array_equal(got[:, :6], stats), "entries 0..5 are the row of df_cad_frame_stats"
    for f in range(3):                                            # a row does not depend on the other rows of its call
        solo = pp.cad_item_table(_up16(depth[f:f + 1]), _up16(label[f:f + 1])).cpu().numpy()
        assert solo.tolist() == want[f:f + 1].tolist(), f
    again = pp.cad_item_table(_up16(depth), _up16(label)).cpu().numpy()
    assert np.array_equal(again, got)
    # another label value and min_side; the call initialises the table itself, on the stream
    for lv, ms in ((7, 0), (65535, 7), (65535, 200)):
        t = torch.full((3, 8), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
        from densefusion_amd import _lib
        d, l = _up16(depth), _up16(label)
        _lib.check(_lib.lib().df_cad_item_table(d.data_ptr(), l.data_ptr(), 3, depth.shape[1], depth.shape[2], lv, ms, t.data_ptr(),
                                                _lib.current_stream()), "cad_item_table")
        assert t.cpu().tolist() == fnp.item_table(depth, label, lv, ms).tolist(), (lv, ms)


def test_item_table_argument_errors_write_nothing():
    _dev()
    from densefusion_amd import _lib
    L = _lib.lib()
    d, l = torch.zeros(2, 9, 9, dtype=torch.int16, device="cuda"), torch.zeros(2, 9, 9, dtype=torch.int16, device="cuda")
    t = torch.full((2, 8), 7, dtype=torch.int32, device="cuda")

    def call(depth=d.data_ptr(), label=l.data_ptr(), F=2, IH=9, IW=9, lv=65535, ms=8, table=t.data_ptr()):
        return L.df_cad_item_table(depth, label, F, IH, IW, lv, ms, table, _lib.current_stream())
    for kw in (dict(depth=None), dict(label=None), dict(table=None)):
        assert call(**kw) == -1 and b"null" in L.df_last_error()
    for kw in (dict(F=0), dict(F=65536), dict(IH=0), dict(IW=-1), dict(IH=1 << 16, IW=1 << 15), dict(lv=-1), dict(lv=65536), dict(ms=-1)):
        assert call(**kw) == -1 and b"bad sizes" in L.df_last_error(), kw
    torch.cuda.synchronize()
    assert bool((t == 7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert t.cpu().tolist() == [[0] * 8] * 2


# ---- df_cad_targets ------------------------------------------------------------------------------------------------------------------
def _poses(rng, B):
    from scipy.spatial.transform import Rotation
    R = Rotation.from_quat(rng.normal(size=(B, 4))).as_matrix()
    t = rng.uniform(-500, 500, (B, 3)) + [0, 0, -4000.0]
    return np.concatenate([R, t[:, :, None]], axis=2)


@pytest.mark.parametrize("P,M", [(500, 500), (501, 500), (3000, 500), (64, 5)])
def test_targets_equal_the_restatement_bit_for_bit(P, M):
    _dev()
    from densefusion_amd.lib import preprocess as pp
    rng = np.random.default_rng(P * 7 + M)
    model = rng.uniform(-80, 80, (P, 3))
    d_model = torch.from_numpy(model).cuda()
    poses = _poses(rng, 3)
    seeds = [0, 0xFFFFFFFF, 123456789]
    want = [fnp.targets(model, 10.0, poses[b], seeds[b], M) for b in range(3)]
    if P == M:
        assert all(np.array_equal(w[2], np.arange(P)) for w in want)
    target, model_points = pp.cad_targets(d_model, poses, seeds, M)
    assert tuple(target.shape) == (3, M, 3) and target.dtype == torch.float32 and tuple(model_points.shape) == (3, M, 3)
    for b in range(3):
        assert np.array_equal(target[b].cpu().numpy().view(np.int32), want[b][0].view(np.int32)), b
        assert np.array_equal(model_points[b].cpu().numpy().view(np.int32), want[b][1].view(np.int32)), b
        t1, m1 = pp.cad_targets(d_model, poses[b:b + 1], seeds[b:b + 1], M)              # B = 1: a row equals its solo call
        assert torch.equal(t1[0], target[b]) and torch.equal(m1[0], model_points[b])
    t2, m2 = pp.cad_targets(d_model, poses, seeds, M)
    assert torch.equal(t2, target) and torch.equal(m2, model_points)
    # another scale and divisor
    t3, m3 = pp.cad_targets(d_model, poses[:1], seeds[:1], M, model_scale=7.5, cloud_div=1000.0)
    w3 = fnp.targets(model, 7.5, poses[0], seeds[0], M, cloud_div=1000.0)
    assert np.array_equal(t3[0].cpu().numpy().view(np.int32), w3[0].view(np.int32))
    assert np.array_equal(m3[0].cpu().numpy().view(np.int32), w3[1].view(np.int32))


def test_targets_argument_errors_write_nothing():
    _dev()
    from densefusion_amd import _lib
    L = _lib.lib()
    P, M, B = 40, 8, 2
    model = torch.zeros(P, 3, dtype=torch.float64, device="cuda")
    pose = torch.zeros(B, 12, dtype=torch.float64, device="cuda")
    seed = torch.zeros(B, dtype=torch.int32, device="cuda")
    need = L.df_cad_targets_scratch_bytes(B, P, M)
    assert need == B * (8 * M + 4 * (P + 1))
    assert L.df_cad_targets_scratch_bytes(B, M - 1, M) == 0 and L.df_cad_targets_scratch_bytes(0, P, M) == 0
    assert L.df_cad_targets_scratch_bytes(B, P, 0) == 0 and L.df_cad_targets_scratch_bytes(65536, P, M) == 0
    scratch = torch.full((need + 8,), 7, dtype=torch.uint8, device="cuda")
    outs = [torch.full((B, M, 3), 7.0, device="cuda") for _ in range(2)]

    def call(model=model.data_ptr(), P=P, pose=pose.data_ptr(), seed=seed.data_ptr(), B=B, M=M, div=10000.0, scratch=scratch.data_ptr(),
             nbytes=need, mp=outs[0].data_ptr(), tg=outs[1].data_ptr()):
        return L.df_cad_targets(model, P, 10.0, pose, seed, B, M, div, scratch, nbytes, mp, tg, _lib.current_stream())
    for kw in (dict(model=None), dict(pose=None), dict(seed=None), dict(scratch=None), dict(mp=None), dict(tg=None)):
        assert call(**kw) == -1 and b"null" in L.df_last_error(), kw
    for kw in (dict(P=M - 1), dict(M=0), dict(B=0), dict(B=65536), dict(P=(1 << 24) + 1), dict(div=0.0)):
        assert call(**kw) == -1 and b"bad sizes" in L.df_last_error(), kw
    assert call(nbytes=need - 1) == -1 and b"scratch" in L.df_last_error()
    assert call(scratch=scratch.data_ptr() + 4) == -1 and b"scratch" in L.df_last_error()
    torch.cuda.synchronize()
    assert bool((scratch == 7).all()) and all(bool((o == 7.0).all()) for o in outs)
    assert call() == 0 and call(P=M) == 0
    torch.cuda.synchronize()
    assert not bool((outs[0] == 7.0).any())
    with pytest.raises(RuntimeError):
        from densefusion_amd.lib import preprocess as pp
        pp.cad_targets(model, pose.cpu().numpy(), [1, 2], P + 1)


# ---- the online items against the disk loader ----------------------------------------------------------------------------------------
TREE_DIMS = (96, 144)
MIN_PIXELS = 600      # single-object trees.  Chosen with the numpy rasteriser (cad_raster_np.render_frame on the icosphere of subdivision
#                       3, seeds 0..39): the views of seeds 1 and 17 cover 592 and 546 pixels and are skipped, every other view up to seed 37
#                       covers 609 or more: 2 sentinels among the 32 views of the test, under the cap of one in six
SENSOR = ["--light", "random", "--sensor_sigma", "3", "--sensor_edge", "1", "--sensor_edge_step", "40", "--sensor_edge_drop", "0.5",
          "--sensor_drop", "0.02", "--sensor_seed", "8"]
# scenes of cad_scene_np.tool_meshes() at --min_pixels 200, --min_visible 0.3: by cad_scene_np.render_frame the own model of seeds 13, 29 and 37 wins
# 88, 122 and 177 pixels (skipped); no other view of seeds 0..39 is skipped: at most 3 sentinels in 40


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return importlib.import_module("render_cad_dataset")
    finally:
        sys.path.pop(0)


def _all_frames_split(tree, obj, written):
    """the loader's train list <- every written frame, in order (the tree is the test's own)"""
    with open(os.path.join(tree, "data", "%02d" % obj, "train.txt"), "w") as f:
        f.write("".join("%d\n" % n for n in range(written)))


@pytest.fixture(scope="module")
def mesh_model(tmp_path_factory):
    """The icosphere of subdivision 3, radius 60 file units, as a coloured binary PLY."""
    root = tmp_path_factory.mktemp("feed_model")
    v, f = mnp.icosphere(3, 60.0)
    v = v.astype(np.float32)
    col = np.random.default_rng(12).integers(0, 256, (len(v), 3), dtype=np.uint8)
    return mnp.write_mesh_ply(root / "icosphere.ply", v, f, col), v, f, root, rnp.write_proj(root / "proj_in.txt", fab.PROJ[1])


def _sagitta(v, f, radius):
    a, b, c = (v[f[:, k]].astype(np.float64) * 10.0 for k in range(3))
    nrm = np.cross(b - a, c - a)
    return radius - (np.abs((nrm * a).sum(axis=1)) / np.linalg.norm(nrm, axis=1)).min()


def _compare(ds, disk, pairs, geometry):
    """Online item i against frame n of the disk loader ``disk`` (one object) for (i, n) in ``pairs``: the record, box, count and
    ``img`` bit for bit, ``choose`` against the key rule, ``cloud`` against the disk loader fed the online ``choose``; with
    ``geometry`` = (radius, sagitta) the target and the cloud on the model's shell around the record's t_cam."""
    from densefusion_amd.datasets.customCAD import render as cr
    obj = disk.objlist[0]
    items = ds.batch([i for i, _ in pairs])
    worst = [0.0, 0.0]
    for (i, n), item in zip(pairs, items):
        info = ds.view_info(i)
        assert info["live"] and info["object"] == obj and item[0].dim() == 2, (i, n)
        pos, quat = cr.parse_record(info["record"])
        assert np.array_equal(disk.meta[obj][n + 1][0], pos) and np.array_equal(disk.meta[obj][n + 1][1], quat), (i, n)
        host = disk.host_item(n)
        assert host[3].tolist()[:7] == info["table"][:7], (i, n, host[3].tolist(), info["table"])
        cloud, choose, img, target, model_points, idx = item
        dmax, _, rmin, rmax, cmin, cmax, count = info["table"][:7]
        depth, label = host[1].numpy().view(np.uint16), host[2].numpy().view(np.uint16)
        mask = (label[rmin:rmax, cmin:cmax] == 65535) & (depth[rmin:rmax, cmin:cmax] != dmax)
        want_choose = cad_np.choose_rule(mask.flatten().nonzero()[0], 500, info["choose_seed"])
        assert count == int(mask.sum()) and np.array_equal(choose.cpu().numpy().reshape(-1), want_choose), (i, n)
        want = disk.device_item(n, host, choose=choose)
        assert torch.equal(want[2], img) and tuple(img.shape) == (3, rmax - rmin, cmax - cmin), (i, n)
        assert torch.equal(want[0], cloud) and torch.equal(want[1], choose), (i, n)
        assert tuple(target.shape) == (500, 3) and tuple(model_points.shape) == (500, 3) and idx._host == [ds.objlist.index(obj)]
        assert idx.cpu().tolist() == idx._host
        keep = fnp.subset(3000, 500, info["subset_seed"])
        want_t, want_m, _ = fnp.targets(ds.pt[obj], 10.0, info["pose"], info["subset_seed"], 500)
        assert np.array_equal(target.cpu().numpy().view(np.int32), want_t.view(np.int32)) and len(keep) == 500
        assert np.array_equal(model_points.cpu().numpy().view(np.int32), want_m.view(np.int32))
        if geometry is not None:
            radius, sagitta = geometry
            t_cam = info["pose"][:, 3]
            tg = np.linalg.norm(target.double().cpu().numpy() * 10000 - t_cam, axis=1)
            assert (tg <= radius + 1e-2).all() and (tg >= radius - sagitta - 1e-2).all(), (i, float(tg.min()), float(tg.max()))
            p = cloud.double().cpu().numpy() * 10000
            bx, by, bz = rnp.grid_bounds(p[:, 2], fab.PROJ[1], *TREE_DIMS)
            dist = np.linalg.norm(p - t_cam, axis=1)
            off = np.maximum(np.maximum(dist - radius, (radius - sagitta) - dist), 0.0)
            bound = np.sqrt(bx * bx + by * by + bz * bz) * (1 + 1e-6) + 1e-3          # the bound of test_rendered_tree_through_the_loader
            worst = [max(worst[0], float((off / bound).max())), max(worst[1], float(np.maximum(tg - radius, radius - sagitta - tg).max()))]
            assert (off <= bound).all(), (i, float((off / bound).max()))
    print("compared", len(pairs), "frames; worst cloud offset / bound", worst[0], "worst target offset", worst[1])


def _sentinel_cap(ds):
    dead = [i for i in range(len(ds)) if not ds.view_info(i)["live"]]
    for i, item in enumerate(ds.batch(range(len(ds)))):
        assert (item[0].dim() == 1) == (i in dead)
        if i in dead:
            assert len(item) == 6 and all(t.dtype == torch.int64 and t.tolist() == [0] for t in item)
    print("sentinels:", dead, "of", len(ds))
    assert 6 * len(dead) <= len(ds), "at most one view in six is a sentinel"
    return dead


@pytest.mark.parametrize("variant", ["clean", "lit_sensor"])
def test_online_items_equal_the_disk_loader_on_a_mesh_tree(mesh_model, variant):
    _dev()
    from densefusion_amd.datasets.customCAD import render as cr
    from densefusion_amd.datasets.customCAD.dataset import PoseDataset
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    path, v, f, root, pm = mesh_model
    tree = str(root / ("tree_" + variant))
    extra = SENSOR if variant == "lit_sensor" else []
    got = _tool().main(["--model", path, "--output_root", tree, "--frames", "24", "--proj_mat", pm, "--height", "96", "--width", "144",
                        "--min_pixels", str(MIN_PIXELS), "--raster", "mesh", "--chunk", "16", "--seed", "0"] + extra)
    assert got["written"] == 24
    _all_frames_split(tree, 1, 24)
    np.random.seed(1)
    disk = PoseDataset("train", 500, False, tree, 0.0, False)
    assert len(disk) == 24
    kw = dict(light="random", sensor=cr.DepthSensor(3.0, 1, 40, 0.5, 0.02, 1), sensor_seed=8) if variant == "lit_sensor" else {}
    ds = RenderedPoseDataset(path, 500, False, 0.0, False, raster="mesh", proj_mat=pm, image_dims=TREE_DIMS, min_pixels=MIN_PIXELS, chunk=16,
                             first_seed=0, frames=32, **kw)
    assert len(ds) == 32 and ds.get_sym_list() == [] and ds.get_num_points_mesh() == 500 and ds.objlist == [1] and ds.pt[1].shape == (3000, 3)
    assert not hasattr(ds, "host_item")
    dead = _sentinel_cap(ds)
    kept = [i for i in range(32) if ds.view_info(i)["kept"]]
    assert dead == [i for i in range(32) if i not in kept] and len(dead) >= 1, "a skipped view is among them"
    assert len(kept) >= 24
    geometry = (600.0, _sagitta(v, f, 600.0)) if variant == "clean" else None
    _compare(ds, disk, list(zip(kept[:24], range(24))), geometry)          # frame n of the tree is the n-th view the tool kept
    if variant == "lit_sensor":                                             # the sensor and the light did change the frames
        clean = RenderedPoseDataset(path, 500, False, 0.0, False, raster="mesh", proj_mat=pm, image_dims=TREE_DIMS, min_pixels=MIN_PIXELS,
                                    chunk=16, first_seed=0, frames=16)
        assert not torch.equal(clean[0][2], ds[0][2]) and clean.view_info(0)["table"][6] != ds.view_info(0)["table"][6]


def test_online_items_equal_the_disk_loader_on_scene_trees(tmp_path_factory):
    _dev()
    from densefusion_amd.datasets.customCAD.dataset import PoseDataset
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    root = tmp_path_factory.mktemp("feed_scene")
    meshes = snp.tool_meshes()
    paths = [mnp.write_mesh_ply(root / name, *[m[k] for k in (0, 1, 2)]) for name, m in zip(("big.ply", "small.ply", "box.ply"), meshes)]
    pm = rnp.write_proj(root / "proj_in.txt", fab.PROJ[1])
    tree = str(root / "tree")
    summary = _tool().main(["--scene", "--model", paths[0], paths[1], "--distractor", paths[2], "--output_root", tree, "--frames", "24",
                            "--proj_mat", pm, "--height", "96", "--width", "144", "--min_pixels", "200", "--min_visible", "0.3", "--mask", "pixels",
                            "--chunk", "16", "--seed", "0"])
    seeds = {k: summary["objects"][k]["seeds"] for k in (1, 2)}
    frames = max(max(s) for s in seeds.values()) + 1
    assert 24 <= frames <= 64
    ds = RenderedPoseDataset(paths[:2], 500, False, 0.0, False, distractors=paths[2:], proj_mat=pm, image_dims=TREE_DIMS, min_pixels=200,
                             min_visible=0.3, mask="pixels", chunk=16, first_seed=0, frames=frames)
    assert ds.scene and ds.objlist == [1, 2] and sorted(ds.pt) == [1, 2]
    dead = _sentinel_cap(ds)
    occluded = 0
    for k in (1, 2):
        _all_frames_split(tree, k, 24)
        np.random.seed(1)
        disk = PoseDataset("train", 500, False, tree, 0.0, False, objlist=(k,))
        own = [i for i in range(frames) if i % 2 == k - 1]
        assert all(ds.view_info(i)["object"] == k for i in own)
        # while its tree was not full, a view's own model was written exactly when the online set keeps it
        filled = seeds[k][-1]
        assert [i for i in own if ds.view_info(i)["kept"] and i <= filled] == [s for s in seeds[k] if s % 2 == k - 1]
        pairs = [(s, n) for n, s in enumerate(seeds[k]) if s % 2 == k - 1]
        assert len(pairs) >= 8
        for s, n in pairs:
            assert ds.view_info(s)["visible"] == summary["objects"][k]["visible"][n]
            occluded += ds.view_info(s)["visible"] < 0.9
        _compare(ds, disk, pairs, ((600.0, 450.0)[k - 1], _sagitta(meshes[k - 1][0], meshes[k - 1][1], (600.0, 450.0)[k - 1])))
    assert occluded >= 3 and len(dead) >= 1, "occluded frames and a skipped view are among them"


# ---- purity ----------------------------------------------------------------------------------------------------------------------------
def _same_item(a, b):
    same = lambda x, y: x.shape == y.shape and torch.equal(x.cpu(), y.cpu()) if x.device != y.device else x.shape == y.shape and torch.equal(x, y)
    return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b)) and \
        (a[0].dim() == 1 or getattr(a[5], "_host", None) == getattr(b[5], "_host", None))          # a sentinel carries no host index


def _noisy(mesh_model, add_noise=True, **kw):
    from densefusion_amd.datasets.customCAD import render as cr
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    path, v, f, root, pm = mesh_model
    np.random.seed(3)                                               # ``pt`` is drawn with np.random, like the loader's
    args = dict(raster="mesh", proj_mat=pm, image_dims=TREE_DIMS, min_pixels=MIN_PIXELS, chunk=16, first_seed=0, frames=20, light="random",
                sensor=cr.DepthSensor(2.0, 1, 40, 0.3, 0.01, 2), sensor_seed=5)
    args.update(kw)
    return RenderedPoseDataset(path, 500, add_noise, 0.03, False, **args)


def test_items_are_a_pure_function_of_the_view_seed(mesh_model):
    _dev()
    a = _noisy(mesh_model)
    whole = a.batch(range(20))
    assert sum(item[0].dim() == 2 for item in whole) >= 17
    for i in (0, 1, 7, 16, 19):
        assert _same_item(a.batch([i])[0], whole[i]) and _same_item(a[i], whole[i]), i
    b = _noisy(mesh_model, chunk=5)
    c = _noisy(mesh_model)
    for i, item in enumerate(whole):
        assert _same_item(b[i], item), ("chunk 5 against chunk 16", i)
        assert _same_item(c[i], item), ("a second construction", i)
    order = a.permutation(np.random.RandomState(4))                 # another cut into chunks: the same items
    assert sorted(order.tolist()) == list(range(20))
    for i in order[:6]:
        assert _same_item(a[int(i)], whole[int(i)]), i
    # add_noise acts: the jitter changes img, and the target moves by add_t * 10000 before the division (the loader's noise, mirrored)
    info = a.view_info(0)
    assert info["plan"] is not None and 0 < np.abs(info["add_t"]).max() <= 0.03
    quiet = _noisy(mesh_model, add_noise=False)
    assert quiet.view_info(0)["record"] == info["record"] and quiet.view_info(0)["table"] == info["table"] and quiet.view_info(0)["plan"] is None
    assert not torch.equal(quiet[0][2], whole[0][2])
    pose = info["pose"].copy()
    pose[:, 3] = pose[:, 3] + info["add_t"] * 10000
    want_t, want_m, _ = fnp.targets(a.pt[1], 10.0, pose, info["subset_seed"], 500)
    assert np.array_equal(whole[0][3].cpu().numpy().view(np.int32), want_t.view(np.int32))
    assert np.array_equal(whole[0][4].cpu().numpy().view(np.int32), want_m.view(np.int32))
    # set_epoch: other views; the view of a seed is the same item in whichever epoch or set it turns up
    a.set_epoch(1)
    fresh = a.batch(range(20))
    assert a.view_info(0)["seed"] == 20 and a.view_info(0)["record"] != info["record"]
    assert not any(_same_item(x, y) for x, y in zip(fresh, whole) if x[0].dim() == 2 and y[0].dim() == 2)
    far = _noisy(mesh_model, frames=40)
    assert far.view_info(20)["record"] == a.view_info(0)["record"] and _same_item(far[20], fresh[0]) and _same_item(far[33], fresh[13])
    a.set_epoch(0)
    for i, item in enumerate(a.batch(range(20))):
        assert _same_item(item, whole[i]), ("epoch 0 again", i)


def test_prefetcher_threads_serve_the_same_items(mesh_model):
    _dev()
    from densefusion_amd import train_utils
    a = _noisy(mesh_model)
    whole = a.batch(range(20))
    b = _noisy(mesh_model, chunk=4, cache_chunks=2)
    order = b.permutation(np.random.RandomState(9)).tolist()
    pf = train_utils.Prefetcher(b, order, torch.device("cuda"), workers=3)
    assert pf.processes == 0
    got = list(pf)
    torch.cuda.synchronize()
    assert len(got) == 20
    for i, item in zip(order, got):
        assert _same_item(item, whole[i]), i


# ---- the trainer -----------------------------------------------------------------------------------------------------------------------
def test_train_tool_on_rendered_views(mesh_model, tmp_path):
    """tools/train.py --dataset cad_render from the fixture's PLY alone: 24 training views in windows of 8, 8 test views."""
    _dev()
    path, v, f, root, pm = mesh_model
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--dataset", "cad_render", "--cad_model", path, "--cad_frames", "24",
           "--cad_test_frames", "8", "--nepoch", "2", "--batch_size", "8", "--workers", "2", "--feed", "threads", "--raster", "mesh",
           "--proj_mat", pm, "--height", "96", "--width", "144", "--min_pixels", str(MIN_PIXELS), "--chunk", "16",
           "--outf", str(out / "models"), "--log_dir", str(out / "logs"), "--decay_margin", "0", "--refine_margin", "0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = r.stdout + r.stderr
    dists = [float(x) for x in re.findall(r"Batch \d+ Frame \d+ Avg_dis:(\S+)", log)]
    assert len(dists) >= 2 and all(math.isfinite(d) and d > 0 for d in dists), log[-3000:]
    assert "length of the training set: 24" in log and "length of the testing set: 8" in log
    test = re.findall(r"TEST FINISH Avg dis: (\S+)", log)
    assert len(test) == 1 and math.isfinite(float(test[0])) and float(test[0]) > 0
    assert [f for f in os.listdir(out / "models") if f.startswith("pose_model_")], os.listdir(out / "models")
