"""GPU: the customCAD renderer -- ``df_cad_render`` against its numpy restatement (tests/cad_render_np.py) bit for bit, its argument errors,
then tools/render_cad_dataset.py: the tree it writes goes through the existing loader, whose clouds and targets must lie on the rendered
sphere where the records say it is, and through tools/train.py --dataset cad and tools/eval_cad.py."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

import cad_render_np as rnp
import fabricate_cad as fab
from densefusion_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROJ = np.array(fab.PROJ[1])
IH, IW = 37, 53                     # no multiple of a wave; an odd pixel count


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _pose(R, t):
    return np.concatenate([np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)[:, None]], axis=1)


def small_scene():
    """About 1 500 points of +-200 file units (x 10 = +-2000 against code limits at |z| = 2000 and 6000), four poses, K = 3 holes.
    frame 0: no rotation at z = -4000: the crafted points below sit where they are meant to; frame 1: turned, shifted, reaching past the
    far code limit (|z| > 6000); frame 2: around the camera: points behind it and before the near code limit; frame 3: all behind."""
    rng = np.random.default_rng(23)
    pts = rng.uniform(-200, 200, (1400, 3))
    nrm = rng.normal(size=(1400, 3))
    # exact duplicates with different colours, nearest to the camera of frame 0 and facing it: the lowest index must win
    dup = np.stack([rng.uniform(-80, 80, 12), rng.uniform(-40, 40, 12), np.full(12, 195.0)], axis=1)
    pts[0:12], pts[100:112] = dup, dup
    nrm[0:12], nrm[100:112] = [0, 0, 1], [0, 0, 1]
    # points on and just past every edge of frame 0 (identity rotation, t_z = -4000): col = floor((ndc_x + 1) IW / 2 + 0.5) is 0 from
    # ndc_x = -1 - 1/IW on and IW from 1 - 1/IW on (rows alike); with splat > 0 their footprints are cut by the border
    edge = []
    for z in (-3000.0, -2500.0):
        for d in (-1e-4, 1e-4):
            for ndc in (-1 - 1 / IW + d, -1.0, 1 - 1 / IW + d, 1.0, -1 - 3 / IW + d, 1 + 1 / IW + d, -1 - 5 / IW + d, 1 + 3 / IW + d):
                edge.append([-z * (ndc + PROJ[0, 2]) / PROJ[0, 0], -z * (0.3 + PROJ[1, 2]) / PROJ[1, 1], z + 4000.0])
            for ndc in (-1 - 1 / IH + d, -1.0, 1 - 1 / IH + d, 1.0, -1 - 3 / IH + d, 1 + 1 / IH + d, -1 - 5 / IH + d, 1 + 3 / IH + d):
                edge.append([-z * (-0.2 + PROJ[0, 2]) / PROJ[0, 0], -z * (-ndc + PROJ[1, 2]) / PROJ[1, 1], z + 4000.0])
    edge = np.array(edge) / 10.0
    pts = np.concatenate([pts, edge])
    nrm = np.concatenate([nrm, np.tile([0.0, 0.0, 1.0], (len(edge), 1))])
    col = rng.integers(0, 256, (len(pts), 3), dtype=np.uint8)
    rot = Rotation.from_quat(rng.normal(size=(2, 4))).as_matrix()
    poses = np.stack([_pose(np.eye(3), [0, 0, -4000.0]), _pose(rot[0], [500.0, -300.0, -5000.0]), _pose(rot[1], [100.0, 50.0, -1500.0]),
                      _pose(rot[0], [0, 0, 9000.0])])
    hole_idx = np.array([[5, 200, -1], [-1, 7, 300], [-1, -1, -1], [0, -1, -1]], dtype=np.int32)       # 5 is a duplicate of 105
    hole_r = np.array([[0.0, 80.0, 7.0], [9.0, 0.0, 150.0], [1.0, 2.0, 3.0], [50.0, 0.0, 0.0]])
    return pts.astype(np.float32), nrm.astype(np.float32), col, poses, (hole_idx, hole_r)


def _gpu(pts, nrm, col, poses, holes, dims, splat, mask_mode, proj=PROJ):
    from densefusion_amd.lib import preprocess as pp
    up = lambda a: None if a is None else torch.from_numpy(a).cuda()
    out = pp.cad_render(up(pts), up(nrm), up(col), poses, 10.0, proj, dims, holes=holes, splat=splat, mask_mode=mask_mode)
    return tuple(o.cpu().numpy() for o in out)


def _same(got, want):
    for name, g, w in zip(("rgb", "depth", "mask", "stats"), got, want[:4]):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5])


def test_the_fixture_has_its_cases():
    """What the bit-equality test below is meant to cover is really in the scene (restatement only; no device work)."""
    pts, nrm, col, poses, holes = small_scene()
    assert 1400 < len(pts) < 1600
    s = pts.astype(np.float64) * 10.0
    z = [poses[f][2, 0] * s[:, 0] + poses[f][2, 1] * s[:, 1] + poses[f][2, 2] * s[:, 2] + poses[f][2, 3] for f in range(4)]
    assert (z[1] < -6000).any() and (z[2] > -2000).any() and (z[2] > 0).any() and (z[3] > 0).all()
    for splat in (0, 1, 2):
        rgb, depth, mask, stats, winner = rnp.render(pts, nrm, col, poses, 10.0, holes, PROJ, IH, IW, splat, 0)
        assert (stats[3] == 0).all() and (depth[3] == 65535).all() and (mask[3] == 0).all()
        assert (stats[:3, 0] > 0).all()
        # duplicates: some pixel of frame 0 is won by one of the first twelve points, none by its copy; hole 5 (radius 0) removed both
        assert np.isin(winner[0], np.arange(0, 12)).any() and not np.isin(winner[0], np.arange(100, 112)).any()
        assert not np.isin(winner[0], [5, 105]).any()
        # the border of frame 0 is reached on all four sides
        assert stats[0, 2] == 0 and stats[0, 3] == IH - 1 and stats[0, 4] == 0 and stats[0, 5] == IW - 1
    stats = rnp.render(pts, None, col, poses, 10.0, None, PROJ, IH, IW, 0, 0)[3]
    assert stats[0, 1] > stats[0, 0]                      # more points than pixels reach the z-buffer: there is contention


@pytest.mark.parametrize("with_normals", [True, False])
@pytest.mark.parametrize("mask_mode", [0, 1])
@pytest.mark.parametrize("splat", [0, 1, 2, 3])
def test_render_equals_the_restatement_bit_for_bit(splat, mask_mode, with_normals):
    _dev()
    pts, nrm, col, poses, holes = small_scene()
    nrm = nrm if with_normals else None
    _same(_gpu(pts, nrm, col, poses, holes, (IH, IW), splat, mask_mode), rnp.render(pts, nrm, col, poses, 10.0, holes, PROJ, IH, IW, splat, mask_mode))


def test_render_without_holes_and_frame_independence():
    """K = 0 (NULL hole arrays); two identical calls give identical bytes; frame 2 of the F = 4 call equals the F = 1 call of its pose."""
    _dev()
    pts, nrm, col, poses, holes = small_scene()
    a = _gpu(pts, nrm, col, poses, None, (IH, IW), 1, 0)
    _same(a, rnp.render(pts, nrm, col, poses, 10.0, None, PROJ, IH, IW, 1, 0))
    b = _gpu(pts, nrm, col, poses, holes, (IH, IW), 1, 0)
    c = _gpu(pts, nrm, col, poses, holes, (IH, IW), 1, 0)
    for x, y in zip(b, c):
        assert x.tobytes() == y.tobytes()
    one = _gpu(pts, nrm, col, poses[2:3], (holes[0][2:3], holes[1][2:3]), (IH, IW), 1, 0)
    for x, y in zip(b, one):
        assert np.array_equal(x[2], y[0])


def test_many_holes_take_several_splat_launches():
    """K = 50: the hole records travel as launch arguments, 128 a launch, so the four frames take two splat launches (frames 0-1, 2-3)."""
    _dev()
    pts, nrm, col, poses, _ = small_scene()
    rng = np.random.default_rng(3)
    hole_idx = rng.integers(-1, len(pts), (4, 50)).astype(np.int32)
    hole_idx[rng.random((4, 50)) < 0.5] = -1
    holes = (hole_idx, rng.uniform(0.0, 30.0, (4, 50)))
    want = rnp.render(pts, nrm, col, poses[[0, 1, 0, 2]], 10.0, holes, PROJ, IH, IW, 1, 1)
    assert (want[3][:3, 0] > 0).all() and not np.array_equal(want[1][0], want[1][2])          # frames 0 and 2: one pose, different holes
    _same(_gpu(pts, nrm, col, poses[[0, 1, 0, 2]], holes, (IH, IW), 1, 1), want)


def test_full_size_frames_where_every_thread_strides():
    """520 x 1109, P = 200 000, F = 2: more points than threads per frame and more pixels than threads in the resolve and mask passes; the
    second sphere is cut by the right edge; splat 1, one hole each."""
    _dev()
    pts, nrm, col = rnp.sphere(200000, seed=8)
    rot = Rotation.from_quat(np.random.default_rng(5).normal(size=(2, 4))).as_matrix()
    poses = np.stack([_pose(rot[0], [300.0, -200.0, -4000.0]), _pose(rot[1], [2200.0, 100.0, -2700.0])])
    holes = (np.array([[11], [70000]], dtype=np.int32), np.array([[25.0], [40.0]]))
    want = rnp.render(pts, nrm, col, poses, 10.0, holes, PROJ, 520, 1109, 1, 0)
    assert want[3][1, 5] == 1108 and (want[3][:, 0] > 10000).all() and (want[3][:, 1] > 50000).all()
    _same(_gpu(pts, nrm, col, poses, holes, (520, 1109), 1, 0), want)


def test_argument_errors_write_nothing():
    _dev()
    from densefusion_amd import _lib
    L = _lib.lib()
    P, F, K = 64, 2, 2
    dev = torch.device("cuda")
    pts = torch.rand(P, 3, device=dev)
    nrm = torch.rand(P, 3, device=dev)
    col = torch.zeros(P, 3, dtype=torch.uint8, device=dev)
    pose = torch.from_numpy(np.stack([_pose(np.eye(3), [0, 0, -4000.0])] * F)).to(dev)
    outs = dict(rgb=torch.full((F, IH, IW, 3), 7, dtype=torch.uint8, device=dev), depth=torch.full((F, IH, IW), 7, dtype=torch.int16, device=dev),
                mask=torch.full((F, IH, IW), 7, dtype=torch.int16, device=dev), stats=torch.full((F, 6), 7, dtype=torch.int32, device=dev))
    need = L.df_cad_render_scratch_bytes(F, IH, IW)
    assert need == F * IH * IW * 8
    assert L.df_cad_render_scratch_bytes(0, IH, IW) == 0 and L.df_cad_render_scratch_bytes(F, 0, IW) == 0 and L.df_cad_render_scratch_bytes(F, IH, -1) == 0
    scratch = torch.full((need,), 7, dtype=torch.uint8, device=dev)
    hole_idx, hole_r = np.full((F, K), -1, dtype=np.int32), np.zeros((F, K))
    good = dict(points=pts.data_ptr(), normals=nrm.data_ptr(), colors=col.data_ptr(), P=P, pose=pose.data_ptr(), model_scale=10.0,
                hole_idx=hole_idx.ctypes.data, hole_r=hole_r.ctypes.data, K=K, proj=None, F=F, IH=IH, IW=IW, splat=1, mask_mode=0,
                rgb=outs["rgb"].data_ptr(), depth=outs["depth"].data_ptr(), mask=outs["mask"].data_ptr(), stats=outs["stats"].data_ptr(),
                scratch=scratch.data_ptr(), scratch_bytes=need, stream=_lib.current_stream())

    def call(**kw):
        proj = kw.pop("proj", PROJ)
        pm = None if proj is None else np.ascontiguousarray(proj, dtype=np.float64)
        a = dict(good, **kw)
        a["proj"] = None if pm is None else pm.ctypes.data
        return L.df_cad_render(*[a[k] for k in good])

    bad_holes = hole_idx.copy()
    bad_holes[1, 1] = P
    row2, row3, row3b = PROJ.copy(), PROJ.copy(), PROJ.copy()
    row2[2, 0], row3[3, 2], row3b[3, 3] = 0.1, -2.0, 1.0
    cases = [dict(points=None), dict(colors=None), dict(pose=None), dict(proj=None), dict(rgb=None), dict(depth=None), dict(mask=None),
             dict(stats=None), dict(scratch=None), dict(hole_idx=None), dict(hole_r=None), dict(splat=-1), dict(splat=4), dict(mask_mode=2),
             dict(hole_idx=bad_holes.ctypes.data), dict(scratch_bytes=need - 1), dict(P=0), dict(F=0), dict(IH=0), dict(K=-1)]
    for kw in cases:
        assert call(**kw) == -1, kw                                       # DF_ERR_ARG
        assert len(L.df_last_error()) > 10, kw
    for pm in (row2, row3, row3b):
        assert call(proj=pm) == -1 and b"projection" in L.df_last_error()
    torch.cuda.synchronize()
    for name, t in list(outs.items()) + [("scratch", scratch)]:
        assert bool((t == 7).all()), name
    assert call() == 0 and call(normals=None) == 0 and call(K=0, hole_idx=None, hole_r=None) == 0
    torch.cuda.synchronize()
    assert not bool((outs["stats"] == 7).any())


# ---- the tool, the loader, the trainer ---------------------------------------------------------------------------------------------
TREE_DIMS = (96, 144)


@pytest.fixture(scope="module")
def rendered_tree(tmp_path_factory):
    """tools/render_cad_dataset.py on the sphere of the host test: one object, 24 frames of 96 x 144."""
    _dev()
    from densefusion_amd.datasets.customCAD.dataset import read_ply
    root = tmp_path_factory.mktemp("rendered")
    pts, nrm, col = rnp.sphere()
    rec = np.zeros(len(pts), dtype=[(a, "<f4") for a in ("x", "y", "z", "nx", "ny", "nz")] + [(a, "u1") for a in ("red", "green", "blue")])
    for k, a in enumerate("xyz"):
        rec[a], rec["n" + a] = pts[:, k], nrm[:, k]
    for k, a in enumerate(("red", "green", "blue")):
        rec[a] = col[:, k]
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(pts) + "".join("property float %s\n" % a for a in ("x", "y", "z", "nx", "ny", "nz")) + \
        "".join("property uchar %s\n" % a for a in ("red", "green", "blue")) + "end_header\n"
    (root / "sphere.ply").write_bytes(head.encode("ascii") + rec.tobytes())
    pm = rnp.write_proj(root / "proj_in.txt", fab.PROJ[1])
    tree = str(root / "tree")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "render_cad_dataset.py"), "--model", str(root / "sphere.ply"), "--output_root", tree,
                        "--object", "1", "--frames", "24", "--proj_mat", pm, "--height", "96", "--width", "144", "--min_pixels", "200", "--splat", "0",
                        "--chunk", "16"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "frames written: 24" in r.stdout and "device time per rendered view" in r.stdout
    assert np.array_equal(read_ply(os.path.join(tree, "models", "obj_01.ply"))[0].astype(np.float32), pts)
    return tree


def test_rendered_tree_through_the_loader(rendered_tree):
    """Cloud and target of every training frame describe the same sphere in the same place: the cloud's points lie on the sphere of
    radius 600 around the record's t_cam to within half a grid step and half a depth code at their own depth (+ 1e-3 for the loader's
    float32), the target's to 1e-2."""
    from densefusion_amd.datasets.customCAD import render as cr
    from densefusion_amd.datasets.customCAD.dataset import PoseDataset
    tree = rendered_tree
    sub = os.path.join(tree, "data", "01")
    train = [int(v) for v in open(os.path.join(sub, "train.txt")).read().split()]
    test = [int(v) for v in open(os.path.join(sub, "test.txt")).read().split()]
    assert len(train) == 19 and len(test) == 5 and sorted(train + test) == list(range(24))
    np.random.seed(1)
    ds = PoseDataset("train", 500, False, tree, 0.0, False)
    assert len(ds) == 19 and ds.udp[1].image_dims == TREE_DIMS
    assert np.array_equal(ds.meta[1][0][0], ds.meta[1][1][0]) and np.array_equal(ds.meta[1][0][1], ds.meta[1][1][1]) and len(ds.meta[1]) == 25
    worst = [0.0, 0.0]
    for i, item in enumerate(ds.batch(list(range(len(ds))))):
        cloud, choose, img, target, model_points, idx = item
        assert cloud.dim() == 2 and tuple(cloud.shape) == (500, 3), "the sentinel"
        R, t_cam = cr.transform_to_pose(*ds.meta[1][ds.list_meta[i] + 1])
        p = cloud.double().cpu().numpy() * 10000
        bx, by, bz = rnp.grid_bounds(p[:, 2], fab.PROJ[1], *TREE_DIMS)
        off = np.abs(np.linalg.norm(p - t_cam, axis=1) - 600)
        bound = np.sqrt(bx * bx + by * by + bz * bz) * (1 + 1e-6) + 1e-3
        worst[0] = max(worst[0], float((off / bound).max()))
        assert (off <= bound).all(), (i, float((off / bound).max()))
        tg = np.abs(np.linalg.norm(target.double().cpu().numpy() * 10000 - t_cam, axis=1) - 600)
        worst[1] = max(worst[1], float(tg.max()))
        assert (tg <= 1e-2).all(), (i, float(tg.max()))
    print("worst cloud offset / bound", worst[0], "worst target offset", worst[1])


def test_train_and_eval_tools_on_a_rendered_tree(rendered_tree, tmp_path):
    """tools/train.py --dataset cad for two optimizer steps (19 // 8), then tools/eval_cad.py, on the rendered tree: both exit 0."""
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--dataset", "cad", "--dataset_root", rendered_tree, "--nepoch", "2", "--batch_size", "8",
           "--workers", "2", "--feed", "threads", "--jitter", "host", "--outf", str(out / "models"), "--log_dir", str(out / "logs"), "--decay_margin", "0",
           "--refine_margin", "0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = r.stdout + r.stderr
    dists = [float(v) for v in re.findall(r"Batch \d+ Frame \d+ Avg_dis:(\S+)", log)]
    assert len(dists) == 2 and all(math.isfinite(d) and d > 0 for d in dists), log[-3000:]
    assert "length of the training set: 19" in log
    ckpt = [f for f in os.listdir(out / "models") if f.startswith("pose_model_")]
    assert ckpt, os.listdir(out / "models")
    sdr = synth.make_state_dict(synth.refiner_spec(5), 1031)
    torch.save({k: torch.from_numpy(v) for k, v in sdr.items()}, tmp_path / "r.pth")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_cad.py"), "--dataset_root", rendered_tree, "--model", str(out / "models" / sorted(ckpt)[0]),
                        "--refine_model", str(tmp_path / "r.pth"), "--output_result_dir", str(tmp_path / "eval"), "--workers", "0"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL success rate" in open(tmp_path / "eval" / "eval_result_logs.txt").read()
