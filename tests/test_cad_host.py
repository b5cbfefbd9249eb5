"""CPU: the host half of the customCAD loader (densefusion_amd/datasets/customCAD) on a fabricated tree -- the projector by a property
its own code does not use, the parsers, 'test' mode's line selection, ``host_item`` against the numpy restatement (tests/cad_np.py) and
the consumption of Python's ``random`` stream."""
import ctypes
import os
import random

import numpy as np
import pytest
from PIL import Image

import cad_np
import fabricate_cad as fab

N = 500


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return fab.make_cad_tree(str(tmp_path_factory.mktemp("cad")))


def _dataset(tree, mode, add_noise=False, noise_trans=0.0, **kw):
    from densefusion_amd.datasets.customCAD.dataset import PoseDataset
    np.random.seed(5)                                   # ply_vtx draws its 3000 model points from np.random
    return PoseDataset(mode, N, add_noise, tree, noise_trans, False, device="cpu", objlist=fab.OBJECTS, **kw)


def _decoded(ds, i):
    return (np.array(Image.open(ds.list_rgb[i])), np.array(Image.open(ds.list_depth[i])), np.array(Image.open(ds.list_label[i])))


@pytest.mark.parametrize("obj", fab.OBJECTS)
def test_projector_reprojects_to_the_pixel_grid(tree, obj):
    """For every pixel and two depths, proj_mat @ [ray * z, 1] divided by its w is that pixel's NDC x and y."""
    from densefusion_amd.datasets.customCAD.project_unity_depth import UnityDepthProjector
    udp = UnityDepthProjector(f"{tree}/data/{obj:02d}/meta/proj_mat.txt", (fab.IH, fab.IW))
    np.testing.assert_array_equal(udp.proj_mat, np.array(fab.PROJ[obj]))
    assert udp.ray_map.shape == (fab.IH, fab.IW, 3) and udp.ray_map.dtype == np.float64
    ndc_x = np.arange(-1, 1, 2.0 / fab.IW)[:fab.IW][None, :].repeat(fab.IH, 0)
    ndc_y = -np.arange(-1, 1, 2.0 / fab.IH)[:fab.IH][:, None].repeat(fab.IW, 1)
    for d in (10000, 40000):
        pts = udp.project_depth(np.full((fab.IH, fab.IW), d, dtype=np.uint16))
        z = -udp.proj_mat[2, 3] / (udp.proj_mat[2, 2] + (1 - d / 65534))
        np.testing.assert_allclose(pts[:, :, 2], z, rtol=1e-12)
        clip = np.concatenate([pts, np.ones((fab.IH, fab.IW, 1))], axis=2) @ udp.proj_mat.T
        assert np.abs(clip[:, :, 0] / clip[:, :, 3] - ndc_x).max() < 1e-9
        assert np.abs(clip[:, :, 1] / clip[:, :, 3] - ndc_y).max() < 1e-9
    np.testing.assert_allclose(udp.ray_map, cad_np.ray_map(udp.proj_mat, (fab.IH, fab.IW)), rtol=0, atol=1e-15)
    depth = np.array(Image.open(f"{tree}/data/{obj:02d}/depth/Depth_0004.png"))
    np.testing.assert_allclose(udp.project_depth(depth), cad_np.project_depth(udp.proj_mat, cad_np.ray_map(udp.proj_mat, (fab.IH, fab.IW)), depth),
                               rtol=1e-14)


def test_parsers(tmp_path):
    from densefusion_amd.datasets.customCAD import dataset as cad
    from densefusion_amd.datasets.customCAD.project_unity_depth import read_proj_mat
    p = tmp_path / "transforms.txt"
    p.write_text("0\n(0.5, 0.5, 4.0)\n(-0.5, -0.6, 0.0, 0.7)\n1\n(0.9, 0.3, 4.0)\n(0.1, 0.2, -0.6, 0.8)\n\n7\n(1.0, 0.3, 3.7)\n(0.0, 0.0, 0.0, 1.0)\n")
    meta = cad.parse_transforms(str(p))
    assert sorted(meta) == [0, 1]                              # reading stops at the first record that does not parse (the blank line)
    np.testing.assert_array_equal(meta[1][0], [0.9, 0.3, 4.0])
    np.testing.assert_array_equal(meta[1][1], [0.1, 0.2, -0.6, 0.8])
    np.testing.assert_array_equal(cad.convert_quat(meta[1][1]), [-0.1, -0.2, -0.6, 0.8])
    m = tmp_path / "proj_mat.txt"
    m.write_text("1.16667\t0.00000\t0.00000\t0.00000\n0.00000\t2.48814\t0.00000\t0.00000\n0.00000\t0.00000\t0.50000\t3000.00000\n"
                 "0.00000\t0.00000\t-1.00000\t0.00000\n\n")
    pm = read_proj_mat(str(m))
    assert pm[0, 0] == 1.16667 and pm[1, 1] == 2.48814 and pm[2, 2] == 0.5 and pm[2, 3] == 3000.0 and pm[3, 2] == -1.0 and pm[3, 3] == 0.0
    mask = np.zeros((9, 11), dtype=bool)
    mask[2:5, 3:9] = True
    assert cad.get_bbox(mask) == (2, 4, 3, 8)                # inclusive


def test_ply_readers(tmp_path):
    from densefusion_amd.datasets.customCAD import dataset as cad
    rng = np.random.default_rng(3)
    pts = rng.uniform(-5, 5, (40, 3)).astype(np.float32)
    fab._write_ply(str(tmp_path / "a.ply"), pts, binary=False)
    fab._write_ply(str(tmp_path / "b.ply"), pts, binary=True)
    va, ta = cad.read_ply(str(tmp_path / "a.ply"))
    vb, tb = cad.read_ply(str(tmp_path / "b.ply"))
    assert len(ta) == 0 and len(tb) == 0 and va.dtype == np.float64
    np.testing.assert_array_equal(vb, pts.astype(np.float64))
    np.testing.assert_allclose(va, pts, atol=1e-6)
    np.random.seed(11)
    got = cad.ply_vtx(str(tmp_path / "b.ply"))
    np.random.seed(11)
    np.testing.assert_array_equal(got, pts.astype(np.float64)[np.random.choice(40, 3000)])          # dataset.py:261
    # a mesh: the unit square in the plane z = 2 as a quad (ASCII) and as two triangles plus a normal column (binary)
    quad = "ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n" \
           "property list uchar int vertex_indices\nend_header\n0 0 2\n1 0 2\n1 1 2\n0 1 2\n4 0 1 2 3\n"
    (tmp_path / "q.ply").write_text(quad)
    head = b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty double x\nproperty double y\nproperty double z\nproperty float nx\n" \
           b"element face 2\nproperty list uchar uint vertex_indices\nend_header\n"
    body = b"".join(np.array(v, dtype="<f8").tobytes() + np.array([0.5], dtype="<f4").tobytes() for v in ([0, 0, 2], [1, 0, 2], [1, 1, 2], [0, 1, 2]))
    body += b"".join(bytes([3]) + np.array(t, dtype="<u4").tobytes() for t in ([0, 1, 2], [0, 2, 3]))
    (tmp_path / "t.ply").write_bytes(head + body)
    for name in ("q.ply", "t.ply"):
        v, t = cad.read_ply(str(tmp_path / name))
        assert v.shape == (4, 3) and t.tolist() == [[0, 1, 2], [0, 2, 3]]
        s = cad.ply_vtx(str(tmp_path / name), 2000)
        assert s.shape == (2000, 3) and np.abs(s[:, 2] - 2).max() < 1e-12 and s[:, :2].min() > -1e-12 and s[:, :2].max() < 1 + 1e-12      # (three fp64 products summed)
        assert abs(s[:, 0].mean() - 0.5) < 0.05 and abs((s[:, 0] > s[:, 1]).mean() - 0.5) < 0.06        # both triangles, evenly


def test_mode_selects_lines(tree):
    tr, te = _dataset(tree, "train"), _dataset(tree, "test")
    assert len(tr) == 2 * fab.FRAMES and tr.list_meta == list(range(fab.FRAMES)) * 2
    assert len(te) == 4 and te.list_meta == [9, 19, 9, 19] and te.list_obj == [1, 1, 2, 2]          # every 10th line of each list
    assert te.list_rgb[1].endswith("data/01/rgb/FrameBuffer_0019.png") and te.list_depth[2].endswith("data/02/depth/Depth_0009.png")
    assert te.list_label[3].endswith("data/02/mask/0019.png")
    assert tr.get_sym_list() == [] and tr.get_num_points_mesh() == 500 and te.pt[1].shape == (3000, 3)
    assert te.udp[1].image_dims == (fab.IH, fab.IW) and te.udp[1].proj_mat[2, 3] == 3000.0 and te.udp[2].proj_mat[2, 3] == 2000.0


def test_fabricated_cases(tree):
    """The cases the tree fixes by construction are what they claim to be."""
    ds = _dataset(tree, "train")
    maxima = set()
    for i in range(len(ds)):
        _, depth, label = _decoded(ds, i)
        assert depth.dtype == np.uint16 and label.dtype == np.uint16
        st = cad_np.frame_stats(depth, label)
        maxima.add(st[0])
        assert np.count_nonzero(depth == st[0]) > 100                   # the maximum occurs in many pixels
        kind = fab.CASES.get((ds.list_obj[i], ds.list_meta[i]))
        rmin, rmax, cmin, cmax = st[2:]
        count = np.count_nonzero((label[rmin:rmax, cmin:cmax] == 65535) & (depth[rmin:rmax, cmin:cmax] != st[0]))
        if kind == "edge":
            assert rmin == 0 and cmax == fab.IW - 1 and 0 < count < N
        elif kind == "thin":
            assert rmax - rmin == 4
        elif kind == "allmax":
            assert st[1] > 0 and count == 0
        elif kind == "big":
            assert count > N and np.count_nonzero(depth[rmin:rmax, cmin:cmax] == st[0]) > 0
        elif kind == "small":
            assert 0 < count < N
        elif kind == "partmax":
            assert 0 < count < np.count_nonzero(label[rmin:rmax, cmin:cmax] == 65535)
    assert len(maxima) == len(ds)


@pytest.mark.parametrize("add_noise", [False, True])
def test_host_item_matches_restatement(tree, add_noise):
    ds = _dataset(tree, "train", add_noise, 0.03)
    lost = 0
    for i in range(len(ds)):
        obj = ds.list_obj[i]
        rgb, depth, label = _decoded(ds, i)
        gt = ds.meta[obj][ds.list_meta[i] + 1]                       # :117
        random.seed(40 + i)
        item = ds.host_item(i)
        after = random.random()
        random.seed(40 + i)
        if add_noise:                                               # torchvision's ColorJitter.get_params: four uniforms, one shuffle of four
            for lo, hi in ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.05, 0.05)):
                random.uniform(lo, hi)
            random.shuffle([0, 1, 2, 3])
        want = cad_np.get_item(rgb, depth, label, [gt[0].copy(), gt[1].copy()], ds.pt[obj], N, 0, ds.udp[obj].proj_mat, ds.udp[obj].ray_map,
                               add_noise=add_noise, noise_trans=0.03)
        assert after == random.random()                             # the stream was consumed like the reference consumes it
        dmax, n_label, rmin, rmax, cmin, cmax, count, oi = item[3].tolist()
        assert [dmax, n_label, rmin, rmax, cmin, cmax] == cad_np.frame_stats(depth, label)
        assert oi == fab.OBJECTS.index(obj)
        if want is None:
            assert count == 0
            lost += 1
            continue
        cloud, choose, img, target, model_points, box = want
        assert (rmin, rmax, cmin, cmax) == box
        assert count == np.count_nonzero((label[rmin:rmax, cmin:cmax] == 65535) & (depth[rmin:rmax, cmin:cmax] != dmax)) > 0
        np.testing.assert_array_equal(item[5].numpy(), model_points)
        np.testing.assert_allclose(item[4].numpy(), target, rtol=0, atol=1e-7)
        np.testing.assert_array_equal(item[1].numpy().view(np.uint16), depth)
        np.testing.assert_array_equal(item[2].numpy().view(np.uint16), label)
        if not add_noise:
            np.testing.assert_array_equal(item[0].numpy(), rgb[:, :, :3])
            assert not item[6].numpy().any()
    assert lost == 3                                                # (1, 3) allmax, (1, 19) thin, (2, 19) allmax


def test_device_jitter_consumes_the_same_stream(tree):
    """jitter="device" leaves the pixels alone on the host, hands the plan row over and draws what jitter="host" draws."""
    host, dev = _dataset(tree, "train", True, 0.03), _dataset(tree, "train", True, 0.03, jitter="device")
    for i in (1, 9, 24):
        random.seed(7 + i)
        a = host.host_item(i)
        ra = random.random()
        random.seed(7 + i)
        b = dev.host_item(i)
        assert ra == random.random()
        assert len(a) == 7 and len(b) == 8 and tuple(b[7].shape) == (1, 8)
        np.testing.assert_array_equal(b[0].numpy(), _decoded(host, i)[0][:, :, :3])
        for k in (3, 4, 5, 6):
            np.testing.assert_array_equal(a[k].numpy(), b[k].numpy())


def test_noise_moves_cloud_and_target_differently(tree):
    """The reference's inconsistency, mirrored: the target moves by add_t, the cloud (device side) is handed add_t to add BEFORE the /10000."""
    clean, noisy = _dataset(tree, "train", False, 0.03), _dataset(tree, "train", True, 0.03)
    noisy.trancolor = type("NoJitter", (), {"__call__": lambda self, im: im})()
    random.seed(1)
    a = clean.host_item(9)
    random.seed(1)
    b = noisy.host_item(9)
    add_t = b[6].numpy()
    assert np.abs(add_t).max() > 0 and np.abs(add_t).max() <= 0.03 and not a[6].numpy().any()
    np.testing.assert_allclose(b[4].numpy() - a[4].numpy(), np.broadcast_to(add_t, (500, 3)), atol=1e-6)


def test_bad_arguments_return_an_error_and_a_message():
    import __graft_entry__ as g
    g.build()
    from densefusion_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_int * 64)()
    p = ctypes.addressof(buf)                   # never dereferenced: the arguments are rejected on the host, before any launch
    assert L.df_cad_frame_stats(None, p, 1, 8, 8, 65535, p, None) != 0 and b"cad_frame_stats: null" in L.df_last_error()
    assert L.df_cad_frame_stats(p, p, 0, 8, 8, 65535, p, None) != 0 and b"cad_frame_stats: bad sizes" in L.df_last_error()
    assert L.df_cad_frame_stats(p, p, 1, 8, 8, 70000, p, None) != 0 and b"cad_frame_stats: bad sizes" in L.df_last_error()
    args = [p, p, p, 1, 48, 72, p, p, p, 0.5, 3000.0, None, 1, 9, 13, 500, 10000.0, p, p, p, p, p, None]
    bad = list(args); bad[8] = None             # no ray map
    assert L.df_preprocess_objects_cad(*bad) != 0 and b"preprocess_cad: null" in L.df_last_error()
    bad = list(args); bad[13] = 49              # crop taller than the frame
    assert L.df_preprocess_objects_cad(*bad) != 0 and b"preprocess_cad: bad sizes" in L.df_last_error()
    bad = list(args); bad[16] = 0.0             # cloud_div
    assert L.df_preprocess_objects_cad(*bad) != 0 and b"preprocess_cad: bad sizes" in L.df_last_error()
    with pytest.raises(RuntimeError):
        _lib.check(L.df_cad_frame_stats(None, None, 1, 8, 8, 65535, None, None), "cad_frame_stats")
