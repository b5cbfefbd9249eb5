"""GPU: the depth-sensor model over rendered customCAD depth (``df_cad_depth_sensor``) against the numpy restatement of steps D0..D6
(tests/cad_sensor_np.py) bit for bit, its chunk independence, determinism, identity, extremes and argument errors, then
tools/render_cad_dataset.py with the --sensor_* flags: only the depth files change, ``meta/sensor.txt`` reproduces them from the clean
tree, and the unchanged loader never chooses a dropped pixel."""
import filecmp
import importlib
import os
import random
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import cad_raster_np as mnp
import cad_render_np as rnp
import cad_scene_np as snp
import cad_sensor_np as dnp
import fabricate_cad as fab

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_NOISE_MUL = 2 ** 31 - 1
ONE24 = 1 << 24


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _up(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16) if a.dtype == np.uint16 else torch.from_numpy(a).cuda()


def _gpu(depth, record, seed, first_frame=0):
    from densefusion_amd.lib import preprocess as pp
    out, stats = pp.cad_depth_sensor(_up(depth), record, seed, first_frame)
    assert out.dtype == torch.uint16 and stats.dtype == torch.int32
    return out.cpu().numpy(), stats.cpu().numpy()


def _same(got, want, what):
    assert got[0].dtype == want[0].dtype and got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    assert np.array_equal(got[0], want[0]), (what, "depth", np.argwhere(got[0] != want[0])[:5])
    assert np.array_equal(got[1], want[1]), (what, "stats", got[1], want[1])


def _scene_depth():
    """the 37 x 53 depth of ``cad_scene_np.small_scene()``'s four frames, rendered by ``df_cad_render_scene`` (which
    tests/test_cad_scene_gpu.py holds to the restatement bit for bit): sphere against sphere, sphere against quad, an empty frame"""
    from densefusion_amd.lib import preprocess as pp
    s = snp.small_scene()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = pp.cad_render_scene(up(s["vertices"]), up(s["colors"]), up(s["triangles"]), s["tri_begin"], s["scales"], s["poses"], snp.NODE_PROJ,
                              (snp.IH, snp.IW), present=s["present"], cull=1)
    return out[1].cpu().numpy()


_INPUTS = {}


def _input(name):
    """(clean depth, edge_step, radii) of a named input, made once"""
    if name not in _INPUTS:
        if name == "scene 37x53":
            _INPUTS[name] = (_scene_depth(), 64, (1, 4))
        elif name == "1x1":
            _INPUTS[name] = (np.array([[[30000]], [[65535]], [[2]]], dtype=np.uint16), 12, (2,))
        else:
            shape, radii = {"5x7": ((5, 7), (0, 1, 2, 4)), "1x64": ((1, 64), (2,)), "64x1": ((64, 1), (2,)), "37x300": ((37, 300), (2,)),
                            "131x301": ((131, 301), (1,))}[name]
            _INPUTS[name] = (dnp.patchy_frames(3, shape[0], shape[1], 11), 12, radii)
    return _INPUTS[name]


def _records(R, edge_step, quant):
    """all three mechanisms at once, then each alone"""
    return {"all": (454047, R, edge_step, ONE24 // 2, ONE24 // 8, quant), "noise": (454047 * 16, R, edge_step, 0, 0, quant),
            "drop": (0, R, edge_step, 0, ONE24 // 4, quant), "edge drop": (0, R, edge_step, ONE24 // 2, 0, quant)}


@gpu
@pytest.mark.parametrize("name", ["5x7", "1x64", "64x1", "1x1", "scene 37x53", "37x300", "131x301"])
def test_sensor_equals_the_restatement_bit_for_bit(name):
    """5 x 7 at every radius (at R = 4 the window is wider than the frame, and every row lies next to another frame's memory); one row,
    one column, one pixel; the scene's 37 x 53 with object-to-object depth steps; 37 x 300 (11 blocks of 4 x 256 pixels per frame, the last one
    with runs that end and runs that lie past the frame) and 131 x 301 (39 such blocks of pixels on the 32 blocks a frame gets: the grid
    stride, and an odd tail)."""
    _dev()
    depth, edge_step, radii = _input(name)
    for R in radii:
        for quant in (1, 7):
            for what, rec in _records(R, edge_step, quant).items():
                want = dnp.sense(depth, rec, 77, 3)
                _same(_gpu(depth, rec, 77, 3), want, (name, R, quant, what))
                if what == "all" and R > 0 and name not in ("1x1",):
                    live = int((depth != 65535).sum())
                    assert want[1][:, 1:].sum(axis=0).min() > 0 and 0 < want[1][:, 0].sum() <= live, "every count counts something"
    if name == "scene 37x53":
        assert 0 < dnp.sense(depth, _records(1, edge_step, 1)["all"], 77, 3)[1][:, 0].sum() < (depth != 65535).sum(), "edge and interior pixels"


@gpu
def test_chunk_independence_and_wrapping_frame_numbers():
    """F = 4 in one call equals two calls of F = 2 with first_frame 0 and 2; first_frame = 2^32 - 1 with F = 2 wraps to frame 0."""
    _dev()
    depth = dnp.patchy_frames(4, 37, 53, 3)
    rec = _records(2, 12, 1)["all"]
    whole = _gpu(depth, rec, 9, 0)
    _same(whole, dnp.sense(depth, rec, 9, 0), "whole")
    for a in (0, 2):
        part = _gpu(depth[a:a + 2], rec, 9, a)
        _same(part, (whole[0][a:a + 2], whole[1][a:a + 2]), a)
    wrap = _gpu(depth[:2], rec, 9, 2 ** 32 - 1)
    _same(wrap, dnp.sense(depth[:2], rec, 9, 2 ** 32 - 1), "wrap")
    assert np.array_equal(wrap[0][1], _gpu(depth[1:2], rec, 9, 0)[0][0]), "the second frame is frame 0"
    assert not np.array_equal(wrap[0][0], whole[0][0])


@gpu
def test_determinism_identity_and_extremes():
    _dev()
    depth, edge_step, _ = _input("37x300")
    rec = _records(2, edge_step, 1)["all"]
    a, b, c = _gpu(depth, rec, 5), _gpu(depth, rec, 5), _gpu(depth, rec, 6)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), "two identical calls"
    assert a[0].tobytes() != c[0].tobytes(), "another seed"
    # the all-zero record with quant 1 is the identity
    ident = _gpu(depth, (0, 0, 0, 0, 0, 1), 5)
    assert np.array_equal(ident[0], depth) and (ident[1] == 0).all()
    ident = _gpu(depth, (0, 2, edge_step, 0, 0, 1), 5)
    assert np.array_equal(ident[0], depth) and (ident[1][:, 1:] == 0).all() and (ident[1][:, 0] > 0).all(), "edges are counted, nothing changes"
    # edge_drop24 = 2^24 drops exactly the restatement's edge set
    live = depth != 65535
    edges = np.stack([dnp.edge_map(d.astype(np.int64), 2, edge_step) for d in depth]) & live
    assert edges.any() and (live & ~edges).any()
    out, stats = _gpu(depth, (0, 2, edge_step, ONE24, 0, 1), 5)
    assert np.array_equal(out == 65535, edges | ~live) and np.array_equal(out[~edges], depth[~edges])
    assert np.array_equal(stats[:, 0], edges.sum(axis=(1, 2))) and np.array_equal(stats[:, 2], stats[:, 0]) and (stats[:, [1, 3]] == 0).all()
    # drop24 = 2^24 leaves only horizon
    out, stats = _gpu(depth, (454047, 2, edge_step, ONE24 // 2, ONE24, 7), 5)
    assert (out == 65535).all() and np.array_equal(stats[:, 1], live.sum(axis=(1, 2))) and (stats[:, 2:] == 0).all()
    # the largest noise_mul: no kept pixel is 65535, on codes next to both ends too
    ends = np.tile(np.array([0, 1, 2, 3, 65531, 65532, 65533, 65534], dtype=np.uint16), (2, 37, 8))
    for d in (depth, ends):
        for quant in (1, 7, 4096):
            got = _gpu(d, (MAX_NOISE_MUL, 0, 0, 0, 0, quant), 5)
            _same(got, dnp.sense(d, (MAX_NOISE_MUL, 0, 0, 0, 0, quant), 5), quant)
            assert np.array_equal(got[0] == 65535, d == 65535) and got[0][d != 65535].max() <= 65534
    assert (got[0] == 0).any() and (got[0] == 65534).any(), "both clamps are reached"


@gpu
def test_argument_errors_write_nothing():
    """Every refusal is DF_ERR_ARG with the call's name in ``df_last_error``; depth_out and stats keep the 7s they were filled with."""
    _dev()
    from densefusion_amd import _lib
    L = _lib.lib()
    F, IH, IW = 2, 37, 53
    n = F * IH * IW
    buf = torch.full((3 * n,), 7, dtype=torch.int16, device="cuda")                    # in | out | a spare frame pair
    src = _up(dnp.patchy_frames(F, IH, IW, 1))
    out = buf[n:2 * n]
    stats = torch.full((F, 4), 7, dtype=torch.int32, device="cuda")
    good = dict(depth_in=src.data_ptr(), depth_out=out.data_ptr(), F=F, IH=IH, IW=IW, seed=1, first_frame=0, noise_mul=454047, edge_radius=2,
                edge_step=64, edge_drop24=ONE24 // 2, drop24=ONE24 // 100, quant=1, stats=stats.data_ptr(), stream=_lib.current_stream())
    inside = buf.data_ptr()
    cases = [dict(depth_in=None), dict(depth_out=None), dict(stats=None),
             dict(depth_in=out.data_ptr()), dict(depth_in=inside + 2, depth_out=inside + 2 * n), dict(depth_in=inside + 2 * n, depth_out=inside + 2),
             dict(depth_in=inside + 2 * n - 2, depth_out=inside), dict(depth_in=inside, depth_out=inside + 2 * n - 2),
             dict(F=0), dict(F=-1), dict(F=65536), dict(IH=0), dict(IW=0), dict(IH=1 << 16, IW=(1 << 14) + 1),
             dict(noise_mul=-1), dict(edge_radius=-1), dict(edge_radius=5), dict(edge_step=-1), dict(edge_step=65536),
             dict(edge_drop24=-1), dict(edge_drop24=ONE24 + 1), dict(drop24=-1), dict(drop24=ONE24 + 1), dict(quant=0), dict(quant=-3), dict(quant=4097)]
    for kw in cases:
        assert L.df_cad_depth_sensor(*dict(good, **kw).values()) == -1, kw                      # DF_ERR_ARG
        assert len(L.df_last_error()) > 20 and b"cad_depth_sensor" in L.df_last_error(), kw
    torch.cuda.synchronize()
    assert bool((buf == 7).all()) and bool((stats == 7).all())
    # ranges that only touch do not overlap; the limits themselves are accepted
    assert L.df_cad_depth_sensor(*dict(good, depth_in=inside, depth_out=inside + 2 * n).values()) == 0
    assert L.df_cad_depth_sensor(*dict(good, noise_mul=MAX_NOISE_MUL, edge_radius=4, edge_step=65535, edge_drop24=ONE24, drop24=ONE24, quant=4096).values()) == 0
    assert L.df_cad_depth_sensor(*good.values()) == 0
    torch.cuda.synchronize()
    assert not bool((stats == 7).all(dim=1).any()) and not bool((out == 7).all())
    from densefusion_amd.lib import preprocess as pp
    with pytest.raises(RuntimeError):
        pp.cad_depth_sensor(src, (0, 0, 0, 0, 0, 0), 0)
    with pytest.raises(RuntimeError):
        pp.cad_depth_sensor(src, (0, 0, 0, 0, 0, 1), 0, out=src)
    with pytest.raises(RuntimeError):
        pp.cad_depth_sensor(src.cpu(), (0, 0, 0, 0, 0, 1), 0)
    with pytest.raises(RuntimeError):
        pp.cad_depth_sensor(src, (2 ** 31, 0, 0, 0, 0, 1), 0)


# ---- the tool and the loader -------------------------------------------------------------------------------------------------------
TREE_DIMS = (96, 144)
FRAMES = 6
SENSOR = ["--sensor_sigma", "4", "--sensor_edge", "2", "--sensor_edge_step", "64", "--sensor_edge_drop", "0.5", "--sensor_drop", "0.01",
          "--sensor_seed", "5"]
SCENE_SENSOR = ["--sensor_sigma_z", "1.5", "--sensor_z", "-4000", "--sensor_edge", "1", "--sensor_edge_step", "200", "--sensor_edge_drop", "0.7",
                "--sensor_quant", "3", "--sensor_seed", "8"]


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return importlib.import_module("render_cad_dataset")
    finally:
        sys.path.pop(0)


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """tools/render_cad_dataset.py on the meshes of the scene tool's test, 6 frames of 96 x 144 per tree: --raster mesh on the big sphere
    without the sensor and with it at --chunk 5 and --chunk 32; --scene of two models and a distractor without and with it."""
    _dev()
    root = tmp_path_factory.mktemp("sensor_trees")
    meshes = snp.tool_meshes()
    paths = [mnp.write_mesh_ply(root / name, *[m[k] for k in (0, 1, 2)]) for name, m in zip(("big.ply", "small.ply", "box.ply"), meshes)]
    pm = rnp.write_proj(root / "proj_in.txt", fab.PROJ[1])
    common = ["--frames", str(FRAMES), "--proj_mat", pm, "--height", str(TREE_DIMS[0]), "--width", str(TREE_DIMS[1]), "--min_pixels", "200",
              "--seed", "0"]
    out = {}
    for name, extra in (("clean", ["--chunk", "8"]), ("chunk5", ["--chunk", "5"] + SENSOR), ("chunk32", ["--chunk", "32"] + SENSOR)):
        tree = str(root / name)
        out[name] = (tree, _tool().main(["--model", paths[0], "--output_root", tree, "--raster", "mesh"] + common + extra))
    for name, extra in (("scene_clean", []), ("scene_sensor", SCENE_SENSOR)):
        tree = str(root / name)
        out[name] = (tree, _tool().main(["--scene", "--model", paths[0], paths[1], "--distractor", paths[2], "--output_root", tree,
                                         "--mask", "pixels", "--chunk", "8"] + common + extra))
    return out


def _files(tree):
    return sorted(os.path.relpath(os.path.join(d, f), tree) for d, _, fs in os.walk(tree) for f in fs)


def _png(path):
    return np.asarray(Image.open(path)).astype(np.uint16)


def _sensor_of(flags, proj):
    from densefusion_amd.datasets.customCAD import render as cr
    kw = {flags[i][2:]: flags[i + 1] for i in range(0, len(flags), 2)}
    sigma = float(kw["sensor_sigma"]) if "sensor_sigma" in kw else cr.DepthSensor.sigma_code_at(proj, float(kw["sensor_sigma_z"]), float(kw["sensor_z"]))
    return cr.DepthSensor(sigma, int(kw.get("sensor_edge", 0)), int(kw.get("sensor_edge_step", 0)), float(kw.get("sensor_edge_drop", 0.0)),
                          float(kw.get("sensor_drop", 0.0)), int(kw.get("sensor_quant", 1))), int(kw["sensor_seed"])


def _check_sensor_txt(clean_sub, sensor_sub, flags, views=None):
    """sensor.txt's record is that of the flags; every frame's depth file and counts are the restatement's on the clean file"""
    from densefusion_amd.datasets.customCAD.project_unity_depth import read_proj_mat
    sensor, seed = _sensor_of(flags, read_proj_mat(os.path.join(sensor_sub, "meta", "proj_mat.txt")))
    lines = open(os.path.join(sensor_sub, "meta", "sensor.txt")).read().splitlines()
    assert lines[0].split() == ["sensor", str(seed)] + [str(v) for v in sensor.record()] and len(lines) == 1 + FRAMES
    changed = 0
    for n, line in enumerate(lines[1:]):
        tok = [int(x) for x in line.split()]
        assert tok[0] == n and len(tok) == 6 and (views is None or tok[1] == views[n])
        clean = _png(os.path.join(clean_sub, "depth", "Depth_%04d.png" % n))
        want, stats = dnp.sense(clean[None], sensor.record(), seed, tok[1])
        assert np.array_equal(_png(os.path.join(sensor_sub, "depth", "Depth_%04d.png" % n)), want[0]), n
        assert tok[2:] == stats[0].tolist(), (n, tok, stats)
        changed += int((want[0] != clean).sum())
    assert changed > FRAMES * 100
    return [int(line.split()[1]) for line in lines[1:]]


@gpu
def test_sensor_flags_change_the_depth_files_only(trees):
    clean, noisy = trees["clean"][0], trees["chunk5"][0]
    names = _files(clean)
    assert _files(noisy) == sorted(names + ["data/01/meta/sensor.txt"]) and len(names) == 3 * FRAMES + 5
    for sub, equal in (("rgb", FRAMES), ("mask", FRAMES), ("depth", 0)):
        files = sorted(os.listdir(os.path.join(clean, "data", "01", sub)))
        same = filecmp.cmpfiles(os.path.join(clean, "data", "01", sub), os.path.join(noisy, "data", "01", sub), files, shallow=False)[0]
        assert len(files) == FRAMES and len(same) == equal, sub
    rest = [n for n in names if not n.startswith(("data/01/rgb", "data/01/mask", "data/01/depth"))]
    assert "data/01/meta/transforms.txt" in rest
    match, mismatch, errors = filecmp.cmpfiles(clean, noisy, rest, shallow=False)
    assert not mismatch and not errors and len(match) == len(rest)
    assert trees["clean"][1]["written"] == trees["chunk5"][1]["written"] == FRAMES and trees["clean"][1]["skipped"] == trees["chunk5"][1]["skipped"]


@gpu
def test_a_frames_noise_does_not_depend_on_the_chunk(trees):
    a, b = trees["chunk5"][0], trees["chunk32"][0]
    names = _files(a)
    assert names == _files(b)
    match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors and len(match) == len(names)


@gpu
def test_sensor_txt_agrees_with_the_restatement_on_the_clean_tree(trees):
    views = _check_sensor_txt(os.path.join(trees["clean"][0], "data", "01"), os.path.join(trees["chunk5"][0], "data", "01"), SENSOR)
    assert views == sorted(set(views)) and views[0] >= 0


def _through_the_loader(tree, clean_tree, objs):
    """The unchanged ``PoseDataset``: no chosen pixel is a dropped one, and every cloud point is ``project_depth`` of the file's own code
    at its chosen pixel -- to fp32 rounding: the loader rounds the fp64 point to float32 and divides by 10000 in float32, two roundings of
    2^-24 relative each per component."""
    from densefusion_amd.datasets.customCAD.dataset import LABEL_VALUE, PoseDataset, get_bbox
    np.random.seed(1)
    random.seed(1)
    ds = PoseDataset("train", 500, False, tree, 0.0, False, objlist=objs)
    assert len(ds) == 4 * len(objs), "80 % of 6 frames"
    worst, dropped_seen = 0.0, 0
    for i, item in enumerate(ds.batch(list(range(len(ds))))):
        cloud, choose = item[0], item[1]
        assert tuple(cloud.shape) == (500, 3), "the sentinel"
        depth, label = _png(ds.list_depth[i]), _png(ds.list_label[i])
        clean = _png(ds.list_depth[i].replace(tree, clean_tree))
        assert depth.max() == 65535, "the loader leaves out the pixels at the frame's depth maximum: the horizon"
        rmin, rmax, cmin, cmax = get_bbox(label == LABEL_VALUE)
        ch = choose.cpu().numpy().reshape(-1)
        rows, cols = rmin + ch // (cmax - cmin), cmin + ch % (cmax - cmin)
        dropped = (depth == 65535) & (clean != 65535)
        dropped_seen += int(dropped[rmin:rmax, cmin:cmax][label[rmin:rmax, cmin:cmax] == LABEL_VALUE].sum())
        assert not dropped[rows, cols].any() and (depth[rows, cols] != 65535).all() and (label[rows, cols] == LABEL_VALUE).all(), i
        want = ds.udp[ds.list_obj[i]].project_depth(depth)[rows, cols]
        err = np.abs(cloud.double().cpu().numpy() * 10000.0 - want) / np.maximum(np.abs(want), 1e-300)
        worst = max(worst, float(err.max()))
        assert (err <= 2.5 * 2.0 ** -24).all(), (i, float(err.max()))
    print("worst relative cloud error", worst, "dropped mask pixels in the crops", dropped_seen)
    assert dropped_seen > 0, "the trees hold dropped pixels inside the masks"


@gpu
def test_sensor_tree_through_the_loader(trees):
    _through_the_loader(trees["chunk5"][0], trees["clean"][0], (1,))


@gpu
def test_scene_with_the_sensor(trees):
    """One --scene run of two models: rgb, mask and records are the clean run's, the depth differs, both trees hold a sensor.txt that
    reproduces the depth files from the clean ones with the views of the summary, and the loader reads both."""
    clean, noisy = trees["scene_clean"], trees["scene_sensor"]
    names = _files(clean[0])
    assert _files(noisy[0]) == sorted(names + ["data/01/meta/sensor.txt", "data/02/meta/sensor.txt"])
    rest = [n for n in names if "/depth/" not in n]
    match, mismatch, errors = filecmp.cmpfiles(clean[0], noisy[0], rest, shallow=False)
    assert not mismatch and not errors and len(match) == len(rest)
    assert not filecmp.cmpfiles(clean[0], noisy[0], [n for n in names if "/depth/" in n], shallow=False)[0], "every depth file differs"
    for k in (1, 2):
        seeds = noisy[1]["objects"][k]["seeds"]
        assert seeds == clean[1]["objects"][k]["seeds"] and noisy[1]["objects"][k]["visible"] == clean[1]["objects"][k]["visible"]
        _check_sensor_txt(os.path.join(clean[0], "data", "%02d" % k), os.path.join(noisy[0], "data", "%02d" % k), SCENE_SENSOR, views=seeds)
    _through_the_loader(noisy[0], clean[0], (1, 2))
