"""GPU: the customCAD data path -- ``df_cad_frame_stats`` and ``df_preprocess_objects_cad`` against numpy (tests/cad_np.py, bit for bit),
the ``PoseDataset`` mirror over a fabricated tree (tests/fabricate_cad.py), then tools/train.py --dataset cad and tools/eval_cad.py on it."""
import math
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import cad_np
import fabricate_cad as fab
from densefusion_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 500


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _up16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return fab.make_cad_tree(str(tmp_path_factory.mktemp("cad")))


def _dataset(tree, mode, add_noise=False, noise_trans=0.0, **kw):
    from densefusion_amd.datasets.customCAD.dataset import PoseDataset
    np.random.seed(5)
    return PoseDataset(mode, N, add_noise, tree, noise_trans, False, objlist=fab.OBJECTS, **kw)


# ---- df_cad_frame_stats ---------------------------------------------------------------------------------------------------------
def _stats_frames():
    """Six frames of 37 x 53 (no multiple of a wave or a vector width; an odd pixel count, so frames 1.. start off an 8-byte boundary)."""
    rng = np.random.default_rng(17)
    IH, IW = 37, 53
    depth = rng.integers(0, 60000, (6, IH, IW)).astype(np.uint16)
    depth[0, 0, 0], depth[1, 7, 5], depth[2, 36, 52] = 60001, 60002, 60003        # different maxima per frame
    label = np.zeros((6, IH, IW), dtype=np.uint16)
    label[rng.random((6, IH, IW)) < 0.05] = 7                    # another label value everywhere: never counted
    label[0, 5:30, 11:40][rng.random((25, 29)) < 0.5] = 65535    # a blob
                                                                 # frame 1: the label absent
    label[2, 36, 0] = 65535                                      # one pixel, in the last row
    for r, c in ((0, 0), (0, IW - 1), (IH - 1, 0), (IH - 1, IW - 1)):
        label[3, r, c] = 65535                                   # all four corners
    depth[3, 20, 31] = 65535                                     # the largest possible value, in one pixel ...
    depth[4] = 1234                                              # ... a constant frame ...
    label[4, 3:9, 50:53] = 65535
    depth[5] = 0                                                 # ... and an all-zero frame with the label on its last column
    label[5, 10:12, IW - 1] = 65535
    return depth, label


def test_frame_stats_match_numpy():
    _dev()
    from densefusion_amd import _lib
    from densefusion_amd.lib import preprocess as pp
    depth, label = _stats_frames()
    want = [cad_np.frame_stats(depth[f], label[f]) for f in range(6)]
    assert want[1][1:] == [0, 0, 0, 0, 0] and want[2][1:] == [1, 36, 36, 0, 0] and want[3][1:] == [4, 0, 36, 0, 52]
    assert want[3][0] == 65535 and want[4][0] == 1234 and want[5][0] == 0 and len({w[0] for w in want}) == 6
    for frames in ([0, 1, 2], [3, 4, 5], [5], [2, 0]):              # F = 3 twice; a frame's row does not depend on its neighbours
        got = pp.cad_frame_stats(_up16(depth[frames]), _up16(label[frames])).cpu().tolist()
        assert got == [want[f] for f in frames], (frames, got)
    # the call initialises `stats` itself, on the stream: garbage in the buffer, another label value
    stats = torch.full((3, 6), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    d, l = _up16(depth[:3]), _up16(label[:3])
    _lib.check(_lib.lib().df_cad_frame_stats(d.data_ptr(), l.data_ptr(), 3, 37, 53, 7, stats.data_ptr(), _lib.current_stream()), "cad_frame_stats")
    assert stats.cpu().tolist() == [cad_np.frame_stats(depth[f], label[f], 7) for f in range(3)]


def test_frame_stats_on_a_full_size_frame():
    """520 x 1109 (the reference's frame): more quads than one pass of the grid, so every thread strides."""
    _dev()
    from densefusion_amd.lib import preprocess as pp
    rng = np.random.default_rng(2)
    depth = rng.integers(0, 65000, (2, 520, 1109)).astype(np.uint16)
    label = np.zeros((2, 520, 1109), dtype=np.uint16)
    label[0, 100:300, 400:900][rng.random((200, 500)) < 0.3] = 65535
    label[1, 519, 1108] = 65535
    got = pp.cad_frame_stats(_up16(depth), _up16(label)).cpu().tolist()
    assert got == [cad_np.frame_stats(depth[f], label[f]) for f in range(2)]


# ---- df_preprocess_objects_cad --------------------------------------------------------------------------------------------------
def _prep_frames():
    """Three frames of 48 x 72 and, per crop size, objects with count > N, count < N and count == 0."""
    rng = np.random.default_rng(23)
    IH, IW = 48, 72
    rgb = rng.integers(0, 256, (3, IH, IW, 3), dtype=np.uint8)
    depth = rng.integers(1000, 50000, (3, IH, IW)).astype(np.uint16)
    label = np.zeros((3, IH, IW), dtype=np.uint16)
    for f, far in enumerate((65535, 61000, 50001)):
        depth[f][rng.random((IH, IW)) < 0.2] = far               # the frame's maximum, scattered: in and off the masks
    label[0, 2:46, 3:70] = 65535                                 # frame 0: nearly everything labelled
    label[1, 10:16, 20:30] = 65535                               # frame 1: a small patch ...
    label[1, 0:45, 0:5] = 65535                                  # ... and a strip
    label[2, 4:44, 5:66] = 65535                                 # frame 2: labelled, every labelled pixel at the maximum
    depth[2][label[2] == 65535] = 50001
    return rgb, depth, label


# (H, W, N, [(frame, rmin, cmin)]): count > N, count < N, count == 0 twice (every labelled pixel at the maximum; for 9 x 13 also a box without a
# label), count > N again; the last 40 x 61 box ends on the frame's last row and column
PREP_CASES = [(9, 13, 64, [(0, 2, 3), (1, 8, 18), (2, 20, 20), (1, 30, 40), (0, 30, 50)]),
              (40, 61, 500, [(0, 0, 0), (1, 3, 0), (2, 4, 5), (2, 8, 11), (0, 8, 11)])]


@pytest.fixture(scope="module")
def prep_setup():
    rgb, depth, label = _prep_frames()
    proj = np.array(fab.PROJ[1])
    rays = cad_np.ray_map(proj, depth.shape[1:])
    return rgb, depth, label, proj, rays


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("case", range(len(PREP_CASES)))
def test_preprocess_cad_bit_equal_to_numpy(prep_setup, case, noise):
    _dev()
    from densefusion_amd.lib import preprocess as pp
    rgb, depth, label, proj, rays = prep_setup
    H, W, n, where = PREP_CASES[case]
    d_rgb, d_depth, d_label = torch.from_numpy(rgb).cuda(), _up16(depth), _up16(label)
    stats = pp.cad_frame_stats(d_depth, d_label)
    objs = [(f, 65535, (r, r + H, c, c + W), 900 + 31 * j) for j, (f, r, c) in enumerate(where)]
    add_t = np.random.default_rng(5).uniform(-300.0, 300.0, (len(objs), 3)) if noise else None
    img, cloud, choose, count = pp.preprocess_objects_cad(d_rgb, d_depth, d_label, objs, n, stats, torch.from_numpy(rays).cuda(), proj[2, 2], proj[2, 3],
                                                          add_t=add_t)
    kinds = []
    for j, (f, _, box, seed) in enumerate(objs):
        w_img, w_cloud, w_choose, w_count = cad_np.prepare(rgb[f], depth[f], label[f], box, n, seed, proj, rays, None if add_t is None else add_t[j])
        assert int(count[j]) == w_count
        kinds.append("zero" if w_count == 0 else "more" if w_count > n else "fewer")
        if w_count == 0:
            assert not choose[j].any()
            continue
        assert torch.equal(choose[j].cpu(), torch.from_numpy(w_choose))
        assert torch.equal(cloud[j].cpu(), torch.from_numpy(w_cloud))               # one rounding per operation, like numpy's -> same bits
        assert torch.equal(img[j].cpu(), torch.from_numpy(w_img))
        assert (w_img[0] == (np.float32(130) - np.float32(0.485)) / np.float32(0.229)).any()          # grey pixels in the crop
    assert kinds == ["more", "fewer", "zero", "zero", "more"]
    # the chosen indices as an INPUT (`given`): the restatement's rows reversed; sampling is skipped, cloud and img follow them
    live = [j for j, k in enumerate(kinds) if k != "zero"]
    given = np.stack([cad_np.prepare(rgb[objs[j][0]], depth[objs[j][0]], label[objs[j][0]], objs[j][2], n, objs[j][3], proj, rays)[2][0][::-1] for j in live])
    sub_t = None if add_t is None else add_t[live]
    img2, cloud2, choose2, count2 = pp.preprocess_objects_cad(d_rgb, d_depth, d_label, [objs[j] for j in live], n, stats, torch.from_numpy(rays).cuda(),
                                                              proj[2, 2], proj[2, 3], add_t=sub_t, choose_in=torch.from_numpy(given.copy()))
    for i, j in enumerate(live):
        f, _, box, seed = objs[j]
        w_img, w_cloud, w_choose, w_count = cad_np.prepare(rgb[f], depth[f], label[f], box, n, seed, proj, rays, None if sub_t is None else sub_t[i],
                                                           given=given[i])
        assert int(count2[i]) == w_count and torch.equal(choose2[i].cpu(), torch.from_numpy(w_choose))
        assert torch.equal(cloud2[i].cpu(), torch.from_numpy(w_cloud)) and torch.equal(img2[i].cpu(), torch.from_numpy(w_img))


def test_wrappers_reject_bad_arguments(prep_setup):
    _dev()
    from densefusion_amd.lib import preprocess as pp
    rgb, depth, label, proj, rays = prep_setup
    d_rgb, d_depth, d_label, d_rays = torch.from_numpy(rgb).cuda(), _up16(depth), _up16(label), torch.from_numpy(rays).cuda()
    stats = pp.cad_frame_stats(d_depth, d_label)
    with pytest.raises(RuntimeError, match="16-bit"):
        pp.cad_frame_stats(d_depth.int(), d_label)
    with pytest.raises(RuntimeError, match="bad sizes"):
        pp.cad_frame_stats(d_depth, d_label, label_value=-1)
    with pytest.raises(RuntimeError, match="outside the frame"):
        pp.preprocess_objects_cad(d_rgb, d_depth, d_label, [(0, 65535, (40, 49, 0, 13), 1)], 64, stats, d_rays, 0.5, 3000.0)
    with pytest.raises(RuntimeError, match="same size"):
        pp.preprocess_objects_cad(d_rgb, d_depth, d_label, [(0, 65535, (0, 9, 0, 13), 1), (0, 65535, (0, 10, 0, 13), 1)], 64, stats, d_rays, 0.5, 3000.0)
    with pytest.raises(RuntimeError, match="ray_map"):
        pp.preprocess_objects_cad(d_rgb, d_depth, d_label, [(0, 65535, (0, 9, 0, 13), 1)], 64, stats, d_rays.float(), 0.5, 3000.0)
    with pytest.raises(RuntimeError, match="bad sizes"):
        pp.preprocess_objects_cad(d_rgb, d_depth, d_label, [(0, 65535, (0, 9, 0, 13), 1)], 64, stats, d_rays, 0.5, 3000.0, cloud_div=0.0)


# ---- PoseDataset ------------------------------------------------------------------------------------------------------------------
def _decoded(ds, i):
    return (np.array(Image.open(ds.list_rgb[i])), np.array(Image.open(ds.list_depth[i])), np.array(Image.open(ds.list_label[i])))


def _same(a, b):
    assert len(a) == len(b) == 6
    for x, y in zip(a, b):
        assert torch.equal(x.cpu(), y.cpu())


def test_batch_matches_restatement(tree):
    _dev()
    ds = _dataset(tree, "train", seed=7)
    idxs = list(range(len(ds)))
    random.seed(99)
    got = ds.batch(idxs)
    random.seed(99)
    lost, sizes = 0, set()
    for i, g in zip(idxs, got):
        obj = ds.list_obj[i]
        rgb, depth, label = _decoded(ds, i)
        gt = ds.meta[obj][ds.list_meta[i] + 1]
        want = cad_np.get_item(rgb, depth, label, [gt[0].copy(), gt[1].copy()], ds.pt[obj], N, (7 * 1000003 + i) & 0xFFFFFFFF, ds.udp[obj].proj_mat,
                               cad_np.ray_map(ds.udp[obj].proj_mat, depth.shape))
        if want is None:
            assert all(t.numel() == 1 and t.dtype == torch.int64 and int(t) == 0 for t in g)
            lost += 1
            continue
        cloud, choose, img, target, model_points, box = want
        assert tuple(g[2].shape[1:]) == (box[1] - box[0], box[3] - box[2])
        sizes.add(tuple(g[2].shape[1:]))
        assert torch.equal(g[1].cpu(), torch.from_numpy(choose))
        assert torch.equal(g[0].cpu(), torch.from_numpy(cloud))
        assert torch.equal(g[2].cpu(), torch.from_numpy(img))
        np.testing.assert_array_equal(g[4].cpu().numpy(), model_points)
        np.testing.assert_allclose(g[3].cpu().numpy(), target, rtol=0, atol=1e-7)
        assert int(g[5][0]) == fab.OBJECTS.index(obj) and g[5]._host == [fab.OBJECTS.index(obj)]
    assert lost == 3 and len(sizes) > 10                                           # the tight boxes: nearly every frame its own crop size


@pytest.mark.parametrize("add_noise,jitter", [(False, "host"), (True, "host"), (True, "device")])
def test_split_fetch_and_getitem_equal_batch(tree, add_noise, jitter):
    """``device_item(i, host_item(i))`` (what the worker-process feed assembles), ``ds[i]`` and ``batch([i])[0]`` are the same tensors."""
    _dev()
    ds = _dataset(tree, "train", add_noise, 0.03, jitter=jitter)
    for i in (0, 3, 5, 9, 19, 29, 39):
        random.seed(100 + i)
        a = ds.batch([i])[0]
        random.seed(100 + i)
        b = ds.device_item(i, ds.host_item(i))
        random.seed(100 + i)
        c = ds[i]
        _same(a, b)
        _same(a, c)


def test_device_jitter_equals_host_jitter(tree):
    """jitter="device" (draws on the host, df_color_jitter after the upload, the grey fill after it) gives the crop of jitter="host" byte for byte;
    and the noise moves the cloud by add_t / 10000 and the target by add_t, like the reference."""
    _dev()
    host, dev, clean = (_dataset(tree, "train", True, 0.03), _dataset(tree, "train", True, 0.03, jitter="device"), _dataset(tree, "train"))
    idxs = [0, 4, 9, 24, 29]
    random.seed(11)
    a = host.batch(idxs)
    random.seed(11)
    b = dev.batch(idxs)
    for x, y in zip(a, b):
        _same(x, y)
    grey, fills = (np.float32(130) - np.float32(0.485)) / np.float32(0.229), 0
    for k, i in enumerate(idxs):
        c = clean[i]
        assert c[2].shape == a[k][2].shape and not torch.equal(c[2], a[k][2])      # jittered colours
        _, depth, label = _decoded(clean, i)
        dmax, _, rmin, rmax, cmin, cmax = cad_np.frame_stats(depth, label)
        far = torch.from_numpy(depth[rmin:rmax, cmin:cmax] == dmax)
        fills += int(far.sum())
        assert (a[k][2][0].cpu()[far] == grey).all() and (c[2][0].cpu()[far] == grey).all()      # the grey fill comes after the jitter
        assert torch.equal(c[1], a[k][1])
        shift = np.abs((a[k][0] - c[0]).double().cpu().numpy()).max()
        assert 0 < shift <= 0.03 / 10000 + 1e-7                  # (1e-7: two float32 roundings of coordinates below 1)
    assert fills > 0


# ---- the tools ------------------------------------------------------------------------------------------------------------------
def _weights(tmp_path):
    sdp, sdr = synth.make_state_dict(synth.posenet_spec(5), 31), synth.make_state_dict(synth.refiner_spec(5), 1031)
    torch.save({k: torch.from_numpy(v) for k, v in sdp.items()}, tmp_path / "p.pth")
    torch.save({k: torch.from_numpy(v) for k, v in sdr.items()}, tmp_path / "r.pth")
    return str(tmp_path / "p.pth"), str(tmp_path / "r.pth")


def test_eval_cad_tool(tree, tmp_path):
    """One log line per test frame, the fabricated lost frames reported as lost, distances that do not depend on the window, PLY dumps.
    (--workers 0: frames fetched in order, so both runs draw the same model points from the seeded streams.)"""
    _dev()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eval_cad
    p, r = _weights(tmp_path)
    logs = {}
    for window in (1, 64):
        out = tmp_path / f"out{window}"
        succ, cnt = eval_cad.main(["--dataset_root", tree, "--model", p, "--refine_model", r, "--output_result_dir", str(out), "--objlist", "1,2",
                                   "--window", str(window), "--workers", "0", "--dump_ply", "2" if window == 64 else "0"])
        logs[window] = open(out / "eval_result_logs.txt").read()
        assert sum(cnt) == 2 and cnt[0] == 1 and cnt[1] == 1
    lines = logs[64].splitlines()
    assert logs[1] == logs[64]                                                       # bit for bit: the distances are printed in full
    assert len(lines) == 4 + 2 + 1                                                   # four test frames, two objects' rates, the overall rate
    assert re.fullmatch(r"No\.0 (NOT )?Pass! Distance: \S+", lines[0]) and math.isfinite(float(lines[0].split("Distance: ")[1]))
    assert lines[1] == "No.1 NOT Pass! Lost detection!"                              # object 1 frame 19: a mask of 5 rows
    assert re.fullmatch(r"No\.2 (NOT )?Pass! Distance: \S+", lines[2])
    assert lines[3] == "No.3 NOT Pass! Lost detection!"                              # object 2 frame 19: every masked pixel at the depth maximum
    assert lines[4].startswith("Object 1 success rate: ") and lines[5].startswith("Object 2 success rate: ") and lines[6].startswith("ALL success rate: ")
    # the dumped clouds: binary little-endian doubles, the target the loader's, the distance between them the logged one
    from densefusion_amd.datasets.customCAD.dataset import read_ply
    out = tmp_path / "out64"
    assert sorted(f for f in os.listdir(out) if f.endswith(".ply")) == ["pred_pcld_0000.ply", "target_pcld_0000.ply"]      # frame 1 is lost
    assert open(out / "pred_pcld_0000.ply", "rb").read(64).startswith(b"ply\nformat binary_little_endian 1.0\n")
    pred, _ = read_ply(str(out / "pred_pcld_0000.ply"))
    target, _ = read_ply(str(out / "target_pcld_0000.ply"))
    assert pred.shape == target.shape == (500, 3)
    assert abs(np.linalg.norm(pred - target, axis=1).mean() - float(lines[0].split("Distance: ")[1])) < 1e-5
    assert eval_cad.cloud_diameter(np.array([[0, 0, 0], [0, 0, 1], [0, 3, 4.0]])) == 5.0


@pytest.mark.parametrize("feed,jitter", [("processes", "device"), ("threads", "host")])
def test_train_tool_on_a_cad_tree(tree, tmp_path, feed, jitter):
    """tools/train.py --dataset cad: two optimizer steps over object 1's 20 training frames, the test pass, a checkpoint tools/eval_cad.py loads."""
    _dev()
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--dataset", "cad", "--dataset_root", tree, "--nepoch", "2", "--batch_size", "8",
           "--workers", "1" if feed == "processes" else "2", "--feed", feed, "--jitter", jitter, "--outf", str(out / "models"), "--log_dir", str(out / "logs"), "--decay_margin", "0",
           "--refine_margin", "0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = r.stdout + r.stderr
    dists = [float(v) for v in re.findall(r"Batch \d+ Frame \d+ Avg_dis:(\S+)", log)]
    assert len(dists) == 2 and all(math.isfinite(d) and d > 0 for d in dists), log[-3000:]          # 20 // 8 optimizer steps
    test_dis = [float(v) for v in re.findall(r"TEST FINISH Avg dis: (\S+)", log)]
    assert len(test_dis) == 1 and math.isfinite(test_dis[0]) and "length of the testing set: 2" in log
    ckpt = [f for f in os.listdir(out / "models") if f.startswith("pose_model_1_")]
    assert len(ckpt) == 1, os.listdir(out / "models")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eval_cad
    _, rpath = _weights(tmp_path)
    succ, cnt = eval_cad.main(["--dataset_root", tree, "--model", str(out / "models" / ckpt[0]), "--refine_model", rpath, "--output_result_dir",
                               str(tmp_path / "eval"), "--workers", "0"])
    assert sum(cnt) == 1 and "No.1 NOT Pass! Lost detection!" in open(tmp_path / "eval" / "eval_result_logs.txt").read()
