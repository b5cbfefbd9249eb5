"""GPU: ``df_mesh_closest`` against its numpy restatement (tests/mesh_closest_np.py) bit for bit in dist2, tri and closest, its argument
errors, then what is built on it: ``detect_symmetry`` on the device against the host run, ``RenderedPoseDataset(symmetry=)``,
``tools/train.py --cad_sym`` and ``tools/eval_cad_render.py --cad_sym``.

The shapes are the smallest at which the kernel can go wrong: T = 1 and T on each side of the LDS tile with the winner in the last
triangle; P = 1, 63, 64, 65, one more than the 128 queries of a workgroup whose waves split the triangles and one more than the 512 of a
workgroup whose lanes all own queries, with K = 1 and 3; 256 transforms, from which on the launch takes the unsplit kernel; queries on a
vertex, on an edge two triangles share and on a face; the seven regions of a triangle; dropped, collinear and zero-edge triangles; all
triangles dropped; a NaN query; no closest_out; the same queries inside a longer call."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import cad_raster_np as mnp
import cad_render_np as rnp
import fabricate_cad as fab
import mesh_closest_np as m

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _device(v, t, p, xf, want_closest=True):
    from densefusion_amd.lib.mesh_distance import mesh_closest
    d2, tri, c = mesh_closest(_up(np.asarray(v, np.float32)), _up(np.asarray(t, np.int32)), _up(np.asarray(p, np.float64)),
                              _up(np.asarray(xf, np.float64)), want_closest=want_closest)
    return d2.cpu().numpy(), tri.cpu().numpy(), None if c is None else c.cpu().numpy()


def _same(got, want, name):
    for g, w, what in zip(got, want, ("dist2", "tri", "closest")):
        assert m.same_bits(g, w), f"{name}: {what} differs in {int((g != w).sum())} of {w.size} elements"


@pytest.fixture(scope="module")
def tile():
    _dev()
    from densefusion_amd.lib.mesh_distance import scratch_bytes, tile_triangles
    assert tile_triangles() >= 2 and scratch_bytes(3) == 3 * 256 and scratch_bytes(0) == 0 and scratch_bytes(-4) == 0
    return tile_triangles()


def test_bit_exact_on_every_small_shape(tile):
    cases = m.make_cases(tile)
    for name in sorted(cases):
        _same(_device(*cases[name]), m.closest_np(*cases[name]), name)
    assert (_device(*cases["T%d" % (tile + 1)])[1] == tile).all(), "the winner sits in the second tile"
    d2, tri, c = _device(*cases["all_dropped"])
    assert (tri == -1).all() and np.isposinf(d2).all()


def test_bit_exact_on_the_unsplit_kernel(tile):
    case = m.whole_path_case(tile)
    assert len(case[3]) * -(-len(case[2]) // m.WHOLE_QUERIES) >= 256
    got, want = _device(*case), m.closest_np(*case)
    _same(got, want, "256 transforms")
    assert (want[1] >= tile).any() and (want[1] < tile).any(), "winners in both tiles"


def test_nan_query_and_no_closest(tile):
    v, t = m.bracket()
    p = np.random.default_rng(3).uniform(-1, 1, (9, 3))
    p[4, 2] = np.nan
    xf = m.three_xf()
    got, want = _device(v, t, p, xf), m.closest_np(v, t, p, xf)
    assert m.same_bits(got[0], want[0]) and m.same_bits(got[1], want[1])
    assert (got[1][:, 4] == -1).all() and np.isposinf(got[0][:, 4]).all() and np.isnan(got[2][:, 4]).any(axis=1).all()
    keep = [0, 1, 2, 3, 5, 6, 7, 8]
    assert m.same_bits(got[2][:, keep], want[2][:, keep]) and np.array_equal(np.isnan(got[2]), np.isnan(want[2]))
    d2, tri, none = _device(v, t, p, xf, want_closest=False)
    assert none is None and m.same_bits(d2, want[0]) and m.same_bits(tri, want[1])


def test_a_query_does_not_depend_on_the_call_around_it(tile):
    v, t = m.far_mesh_with_near_last(tile + 1, 9)
    p = np.random.default_rng(4).uniform(-6, 6, (700, 3))
    xf = m.three_xf()
    short, long_ = _device(v, t, p[:65], xf), _device(v, t, p, xf)
    for a, b in zip(short, long_):
        assert m.same_bits(a, np.ascontiguousarray(b[:, :65]))
    again = _device(v, t, p, xf)
    assert all(m.same_bits(a, b) for a, b in zip(long_, again)), "two calls, the same bytes"
    one = _device(v, t, p, xf[1:2])
    assert all(m.same_bits(a, np.ascontiguousarray(b[1:2])) for a, b in zip(one, long_)), "nor on the other transforms"


def test_argument_errors_write_nothing(tile):
    from densefusion_amd import _lib
    L = _lib.lib()
    V, T, P, K = 6, 5, 7, 2
    v, t = torch.rand(V, 3, device="cuda"), torch.randint(0, V, (T, 3), dtype=torch.int32, device="cuda")
    p, xf = torch.rand(P, 3, dtype=torch.float64, device="cuda"), _up(m.three_xf()[:K])
    outs = dict(d2=torch.full((K, P), 7.0, dtype=torch.float64, device="cuda"), tri=torch.full((K, P), 7, dtype=torch.int32, device="cuda"),
                c=torch.full((K, P, 3), 7.0, dtype=torch.float64, device="cuda"))
    need = L.df_mesh_closest_scratch_bytes(T)
    scratch = torch.full((need + 16,), 7, dtype=torch.uint8, device="cuda")
    good = dict(vertices=v.data_ptr(), V=V, triangles=t.data_ptr(), T=T, points=p.data_ptr(), P=P, xf=xf.data_ptr(), K=K, d2=outs["d2"].data_ptr(),
                tri=outs["tri"].data_ptr(), c=outs["c"].data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=need, stream=_lib.current_stream())
    big = 2 ** 31 - 1
    cases = [dict(vertices=None), dict(triangles=None), dict(points=None), dict(xf=None), dict(d2=None), dict(tri=None), dict(scratch=None),
             dict(V=0), dict(T=0), dict(P=0), dict(K=0), dict(V=-1), dict(T=-3), dict(P=-1), dict(K=-2), dict(V=big // 3 + 1), dict(T=big // 3 + 1),
             dict(K=big // 12 + 1), dict(P=big // (3 * K) + 1), dict(P=big), dict(scratch_bytes=need - 1), dict(scratch_bytes=0),
             dict(scratch=scratch.data_ptr() + 8, scratch_bytes=need), dict(points=p.data_ptr() + 4), dict(d2=outs["d2"].data_ptr() + 4),
             dict(c=outs["c"].data_ptr() + 4), dict(tri=outs["tri"].data_ptr() + 2), dict(vertices=v.data_ptr() + 2)]
    for kw in cases:
        a = dict(good, **kw)
        assert L.df_mesh_closest(*[a[k] for k in good]) == -1, kw            # DF_ERR_ARG
        assert len(L.df_last_error()) > 10, kw
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs.values()) and bool((scratch == 7).all()), "nothing was written"
    assert L.df_mesh_closest(*[dict(good, c=None)[k] for k in good]) == 0
    torch.cuda.synchronize()
    assert bool((outs["c"] == 7).all()) and not bool((outs["tri"] == 7).any()) and bool((scratch[need:] == 7).all())
    from densefusion_amd.lib.mesh_distance import mesh_closest
    with pytest.raises(RuntimeError):
        mesh_closest(v.cpu(), t, p, xf)
    with pytest.raises(RuntimeError):
        mesh_closest(v.double(), t, p, xf)
    with pytest.raises(RuntimeError):
        mesh_closest(v, t.long(), p, xf)
    with pytest.raises(RuntimeError):
        mesh_closest(v, t, p.float(), xf)
    with pytest.raises(RuntimeError):
        mesh_closest(v, t, p, xf[:, :2])
    with pytest.raises(RuntimeError):
        mesh_closest(v, t, p, xf, scratch=torch.empty(need - 1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        mesh_closest(v, t[:0], p, xf)


# ---- what is built on it ---------------------------------------------------------------------------------------------------------------------
def _same_rows(a, b):
    """two ``passed`` lists, the colour residual's nan (no colours) equal to itself"""
    return np.array_equal(np.array(a, dtype=np.float64), np.array(b, dtype=np.float64), equal_nan=True)


def test_detection_on_the_device_equals_the_host_run(tile):
    from densefusion_amd.datasets.customCAD.symmetry import detect_symmetry
    for mesh, symmetric in ((m.box(1, 2, 3), True), (m.bracket(), False)):
        dev, host = detect_symmetry(*mesh), detect_symmetry(*mesh, closest=m.closest_np)
        assert dev.symmetric == host.symmetric == symmetric and _same_rows(dev.passed, host.passed) and dev.D == host.D and dev.orders == host.orders
        assert m.same_bits(dev.axes, host.axes) and m.same_bits(dev.centroid, host.centroid) and m.same_bits(dev.residuals, host.residuals)
    v, t = m.box(1, 2, 3)
    col = np.full((len(v), 3), 130, dtype=np.uint8)
    col[20:24] = (255, 0, 0)
    dev, host = detect_symmetry(v, t, col), detect_symmetry(v, t, col, closest=m.closest_np)
    assert _same_rows(dev.passed, host.passed) and len(dev.passed) == 1 and m.same_bits(dev.color_residuals, host.color_residuals)


SCALE = 30.0                    # the unit fixtures in file units: about the size of the meshes the other scene tests render


def _scene_meshes():
    """model 0: the bracket (no symmetry), model 1: prism(5) (order 5 about its axis, order 2 across it), both plain grey"""
    out = []
    for v, t in (m.bracket(), m.prism(5, 1.3, 1.5)):
        out.append(((v * SCALE).astype(np.float32), t, np.full((len(v), 3), 130, dtype=np.uint8)))
    return out


def _dataset(**kw):
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    np.random.seed(1)                                                          # ``pt`` is drawn with np.random
    return RenderedPoseDataset(_scene_meshes(), 500, False, 0.0, False, proj_mat=fab.PROJ[1], mask="pixels", min_visible=0.3, chunk=4,
                               first_seed=0, frames=8, image_dims=(64, 96), min_pixels=60, **kw)


def test_the_dataset_finds_its_symmetric_model_and_serves_the_same_items(tile):
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    plain, auto = _dataset(), _dataset(symmetry="auto")
    assert plain.get_sym_list() == [] and plain.symmetry == {}
    assert auto.get_sym_list() == [1] and sorted(auto.symmetry) == [0, 1] and not auto.symmetry[0].symmetric and auto.symmetry[1].symmetric
    assert 5 in [n for _, n, _, _ in auto.symmetry[1].passed]
    live = 0
    for i in range(8):
        x, y = plain[i], auto[i]
        assert len(x) == len(y) == 6 and all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(x, y)), i
        live += plain.view_info(i)["live"]
    assert live >= 3, "the comparison has something to compare"
    # the list holds what an item's index holds: model 1's items carry index 1
    own = [int(auto[i][5].reshape(-1)[0]) for i in range(8) if auto.view_info(i)["live"] and auto.view_info(i)["object"] == 2]
    assert own and set(own) == {1}
    assert _dataset(symmetry=[0]).get_sym_list() == [0]
    with pytest.raises(ValueError):
        _dataset(symmetry=[2])
    with pytest.raises(ValueError):
        _dataset(symmetry="yes")
    cloud = (np.random.default_rng(0).normal(size=(2000, 3)).astype(np.float32) * 30, None, np.full((2000, 3), 130, dtype=np.uint8))
    with pytest.raises(ValueError, match="triangles"):
        RenderedPoseDataset(cloud, 500, False, 0.0, False, proj_mat=fab.PROJ[1], image_dims=(64, 96), frames=4, symmetry="auto")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    _dev()
    from densefusion_amd.lib.network import PoseNet, PoseRefineNet
    root = tmp_path_factory.mktemp("cad_symmetry")
    paths = [str(mnp.write_mesh_ply(root / name, *mesh)) for name, mesh in zip(("bracket.ply", "prism.ply"), _scene_meshes())]
    torch.manual_seed(3)
    torch.save(PoseNet(num_points=500, num_obj=5).state_dict(), root / "pose.pth")
    torch.save(PoseRefineNet(num_points=500, num_obj=5).state_dict(), root / "refine.pth")
    return dict(root=root, paths=paths, pm=rnp.write_proj(root / "proj_in.txt", fab.PROJ[1]))


VIEW_FLAGS = ["--height", "64", "--width", "96", "--min_pixels", "60", "--mask", "pixels", "--chunk", "4"]


def test_the_trainer_logs_the_detected_list(files, tmp_path):
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--dataset", "cad_render", "--cad_model", *files["paths"], "--cad_sym", "auto",
           "--cad_frames", "8", "--cad_test_frames", "4", "--nepoch", "2", "--batch_size", "4", "--workers", "2", "--feed", "threads",
           "--proj_mat", files["pm"], *VIEW_FLAGS, "--outf", str(out / "models"), "--log_dir", str(out / "logs"), "--decay_margin", "0",
           "--refine_margin", "0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-3000:]
    assert "symmetry object list: [1]" in log, log[-3000:]
    assert re.findall(r"TEST FINISH Avg dis: (\S+)", log), log[-3000:]


def test_the_evaluation_tool_scores_with_the_detected_list(files):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        tool = importlib.import_module("eval_cad_render")
    finally:
        sys.path.pop(0)
    args = ["--cad_model", *files["paths"], "--model", str(files["root"] / "pose.pth"), "--refine_model", str(files["root"] / "refine.pth"),
            "--masks", "truth", "--cad_seed", "0", "--cad_frames", "8", "--proj_mat", files["pm"], *VIEW_FLAGS, "--workers", "0", "--iteration", "2"]
    got = tool.main(args + ["--cad_sym", "auto", "--output_result_dir", str(files["root"] / "auto")])
    assert got["truth"]["sym_list"] == [1] and sum(got["truth"]["served"]) >= 3
    plain = tool.main(args + ["--output_result_dir", str(files["root"] / "plain")])
    assert plain["truth"]["sym_list"] == [] and plain["truth"]["served"] == got["truth"]["served"]
    # ADD-S is never above ADD: with the list, model 1's views cannot do worse
    assert got["truth"]["success"][1] >= plain["truth"]["success"][1] and got["truth"]["success"][0] == plain["truth"]["success"][0]

    def distances(name):
        text = open(files["root"] / name / "eval_result_logs_truth.txt").read()
        return [float(x) for x in re.findall(r"Pass! Distance: (\S+)", text)]
    a, b = distances("auto"), distances("plain")
    assert len(a) == len(b) >= 3 and all(x <= y for x, y in zip(a, b)) and any(x < y for x, y in zip(a, b))
