"""GPU: the bounding-box tree route -- ``df_mesh_closest_tree`` and ``df_mesh_icp_tree`` -- gives the bytes of the plain scans: against
the restatements ``mesh_closest_np.closest_np`` and ``mesh_icp_np.run_case`` (used by import: the tree adds no numerics), against
``df_mesh_closest`` itself, through the wrappers, and through ``tools/eval_cad_render.py --icp_accel``.

The shapes are those of the scans' own tests (triangle ranges on each side of the 128-record tile, N around a wave, a workgroup of 256
walking lanes and the 256 summing lanes, items of one call on different ranges, one empty, frozen and bad items) plus the adversarial
cases of ``mesh_tree_np`` (exact ties in shuffled order, a repeated triangle, slivers on the loose list, a collinear triangle, far and
large-coordinate queries, NaN and infinite queries, an object with nothing kept)."""
import os

import numpy as np
import pytest
import torch

import cad_raster_np as mnp
import cad_render_np as rnp
import cad_scene_np as snp
import fabricate_cad as fab
import mesh_closest_np as m
import mesh_icp_np as icp
import mesh_tree_np as mt

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _up(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _closest_tree(v, t, p, xf, want_closest=True, tree=None):
    """``df_mesh_closest_tree`` itself: (dist2, tri, closest) as numpy."""
    from densefusion_amd import _lib
    L = _lib.lib()
    tree = mt.tree_of(v, t) if tree is None else tree
    dv, dt, dp, dx = _up(v, np.float32), _up(t, np.int32), _up(p, np.float64), _up(np.asarray(xf).reshape(-1, 12), np.float64)
    K, P, T = len(dx), len(dp), len(dt)
    need = L.df_mesh_closest_scratch_bytes(T)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    d2, tri = torch.full((K, P), 7.0, dtype=torch.float64, device="cuda"), torch.full((K, P), 7, dtype=torch.int32, device="cuda")
    c = torch.full((K, P, 3), 7.0, dtype=torch.float64, device="cuda") if want_closest else None
    rc = L.df_mesh_closest_tree(dv.data_ptr(), len(dv), dt.data_ptr(), T, dp.data_ptr(), P, dx.data_ptr(), K, d2.data_ptr(), tri.data_ptr(),
                                c.data_ptr() if want_closest else None, scratch.data_ptr(), need, _lib.current_stream(), *tree.args("cuda"))
    assert rc == 0, L.df_last_error()
    return d2.cpu().numpy(), tri.cpu().numpy(), c.cpu().numpy() if want_closest else None


def _icp_tree(case, iters=None, leaf=None):
    """``df_mesh_icp_tree`` itself on a case of ``mesh_icp_np``: (pose_out, stats) as numpy."""
    from densefusion_amd import _lib
    L = _lib.lib()
    v, t, begin = icp.concat_meshes(case["meshes"])
    tree = mt.tree_of(v, t, begin, leaf)
    obj, pts, pose = np.asarray(case["obj"], np.int32), np.asarray(case["points"], np.float32), np.asarray(case["pose"], np.float64)
    B, N = pts.shape[:2]
    dv, dt, dobj, dpts, dpose = _up(v, np.float32), _up(t, np.int32), _up(obj, np.int32), _up(pts, np.float32), _up(pose, np.float64)
    md = np.ascontiguousarray(case["max_dist"], dtype=np.float64)
    need = L.df_mesh_icp_scratch_bytes(len(t), B, N)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    out, stats = torch.full((B, 7), 7.0, dtype=torch.float64, device="cuda"), torch.full((B, 6), 7.0, dtype=torch.float64, device="cuda")
    rc = L.df_mesh_icp_tree(dv.data_ptr(), len(v), dt.data_ptr(), len(t), begin.ctypes.data, md.ctypes.data, len(begin) - 1, dobj.data_ptr(),
                            dpts.data_ptr(), dpose.data_ptr(), B, N, case["iters"] if iters is None else iters, case["cull"], out.data_ptr(),
                            stats.data_ptr(), scratch.data_ptr(), need, _lib.current_stream(), *tree.args("cuda"))
    assert rc == 0, L.df_last_error()
    return out.cpu().numpy(), stats.cpu().numpy()


def test_closest_tree_equals_the_scan_bit_for_bit():
    _dev()
    from densefusion_amd import _lib
    from densefusion_amd.lib.mesh_distance import mesh_closest
    tile = _lib.lib().df_mesh_closest_tile_triangles()
    cases = dict(m.make_cases(tile), whole_path=m.whole_path_case(tile), **mt.adversarial_cases())
    for name, (v, t, p, xf) in cases.items():
        want = m.closest_np(v, t, p, xf)
        for g, w, what in zip(_closest_tree(v, t, p, xf), want, ("dist2", "tri", "closest")):
            assert m.same_bits(g, w), f"{name}: {what} differs"
    v, t, p, xf = cases["slivers"]
    got = _closest_tree(v, t, p, xf, want_closest=False, tree=mt.tree_of(v, t, leaf=1))
    assert got[2] is None and m.same_bits(got[0], m.closest_np(v, t, p, xf)[0])
    # against df_mesh_closest itself, where the tree has something to skip
    v, t = m.icosphere(5)
    rng = np.random.default_rng(3)
    d = rng.normal(size=(256, 3))
    q = d / np.sqrt((d * d).sum(axis=1, keepdims=True)) * rng.uniform(0.95, 1.05, (256, 1))
    scan = mesh_closest(_up(v, np.float32), _up(t, np.int32), _up(q, np.float64), _up(m.three_xf(), np.float64))
    for g, w in zip(_closest_tree(v, t, q, m.three_xf()), scan):
        assert m.same_bits(g, w.cpu().numpy())


def _extra_icp_cases():
    """a finite max_dist that leaves some points out over several steps, and cull over several steps"""
    rng = np.random.default_rng(31)
    br = m.bracket()
    pts, start = icp.fit_item(br, 200, rng)
    pts[::7] += np.float32(0.4)                                  # every seventh point lies far off the surface
    a = dict(meshes=[br], max_dist=[0.15], obj=[0], points=pts[None], pose=start[None], iters=3, cull=0)
    items = [icp.fit_item(br, 257, rng) for _ in range(2)]
    b = dict(meshes=[m.scalene_tetrahedron(), br], max_dist=[icp.INF, 0.5], obj=[1, 1], points=np.stack([i[0] for i in items]),
             pose=np.stack([i[1] for i in items]), iters=3, cull=1)
    return {"max_dist": a, "cull": b}


def test_icp_tree_equals_the_restatement_bit_for_bit():
    _dev()
    from densefusion_amd import _lib
    made = dict(icp.make_icp_cases(_lib.lib().df_mesh_closest_tile_triangles()), **_extra_icp_cases())
    assert "mixed" in made and "ranges" in made
    for name, case in made.items():
        want = icp.run_case(case)
        for leaf in (None, 1) if name in ("mixed", "ranges", "max_dist") else (None,):
            for g, w, what in zip(_icp_tree(case, leaf=leaf), want, ("pose_out", "stats")):
                assert m.same_bits(g, w), f"{name}: {what} differs\n{g}\n{w}"
        if name == "max_dist":
            assert 0 < want[1][0, 1] < 200 and want[1][0, 0] == icp.OK, "max_dist took points away"
        if name == "cull":
            assert (want[1][:, 1] < 257).all() and (want[1][:, 1] > 6).all(), "cull took points away"


def test_argument_errors_write_nothing():
    _dev()
    from densefusion_amd import _lib
    L = _lib.lib()
    v, t = m.bracket()
    tree = mt.tree_of(v, t)
    V, T, B, N = len(v), len(t), 2, 9
    dv, dt = _up(v, np.float32), _up(t, np.int32)
    nodes, order, loose = tree.on("cuda")
    big_tree = mt.tree_of(*m.icosphere(2))                       # 320 triangles: more nodes than 24 triangles can have
    bad_nb = [np.array(a, dtype=np.int32) for a in ([1, tree.n_nodes], [0, -1], [0, 2 * T])]
    bad_lb = [np.array(a, dtype=np.int32) for a in ([1, 1], [0, T + 1], [0, -1])]
    tree_errors = [dict(nodes=None), dict(nb=None), dict(order=None), dict(loose=None), dict(lb=None), dict(nodes=nodes.data_ptr() + 8),
                   dict(order=order.data_ptr() + 2), dict(loose=loose.data_ptr() + 2), dict(n_nodes=tree.n_nodes - 1), dict(n_nodes=0),
                   dict(n_order=0), dict(n_order=T + 1), dict(nb=big_tree.node_begin.ctypes.data, n_nodes=big_tree.n_nodes)]
    tree_errors += [dict(nb=a.ctypes.data) for a in bad_nb] + [dict(lb=a.ctypes.data, n_loose=T + 1) for a in bad_lb]
    tree_good = dict(nodes=nodes.data_ptr(), n_nodes=tree.n_nodes, nb=tree.node_begin.ctypes.data, order=order.data_ptr(), n_order=tree.n_order,
                     loose=loose.data_ptr(), n_loose=tree.n_loose, lb=tree.loose_begin.ctypes.data)
    big = 2 ** 31 - 1
    # df_mesh_closest_tree
    P, K = 5, 2
    p, xf = torch.rand(P, 3, dtype=torch.float64, device="cuda"), _up(m.three_xf()[:K].reshape(K, 12), np.float64)
    d2, tri, c = (torch.full((K, P), 7.0, dtype=torch.float64, device="cuda"), torch.full((K, P), 7, dtype=torch.int32, device="cuda"),
                  torch.full((K, P, 3), 7.0, dtype=torch.float64, device="cuda"))
    need = L.df_mesh_closest_scratch_bytes(T)
    scratch = torch.full((need + 16,), 7, dtype=torch.uint8, device="cuda")
    good = dict(vertices=dv.data_ptr(), V=V, triangles=dt.data_ptr(), T=T, points=p.data_ptr(), P=P, xf=xf.data_ptr(), K=K, d2=d2.data_ptr(),
                tri=tri.data_ptr(), c=c.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=need, stream=_lib.current_stream(), **tree_good)
    errors = [dict(vertices=None), dict(triangles=None), dict(points=None), dict(xf=None), dict(d2=None), dict(tri=None), dict(scratch=None),
              dict(V=0), dict(T=0), dict(P=0), dict(K=0), dict(V=big // 3 + 1), dict(T=big // 3 + 1), dict(K=big // 12 + 1), dict(P=big // (3 * K) + 1),
              dict(scratch_bytes=need - 1), dict(scratch=scratch.data_ptr() + 8), dict(points=p.data_ptr() + 4), dict(tri=tri.data_ptr() + 2),
              dict(c=c.data_ptr() + 4)] + tree_errors
    for kw in errors:
        a = dict(good, **kw)
        assert L.df_mesh_closest_tree(*[a[k] for k in good]) == -1, kw
        assert len(L.df_last_error()) > 10, kw
    torch.cuda.synchronize()
    assert bool((d2 == 7).all()) and bool((tri == 7).all()) and bool((c == 7).all()) and bool((scratch == 7).all()), "nothing was written"
    assert L.df_mesh_closest_tree(*good.values()) == 0
    torch.cuda.synchronize()
    assert not bool((d2 == 7).any()) and bool((scratch[need:] == 7).all())
    # df_mesh_icp_tree: df_mesh_icp's refusals and the tree's
    obj, pts = _up([0, 0], np.int32), torch.rand(B, N, 3, device="cuda")
    pose = _up([[1, 0, 0, 0, 0, 0, 0]] * B, np.float64)
    begin, md = np.array([0, T], dtype=np.int32), np.array([1.0])
    out, stats = torch.full((B, 7), 7.0, dtype=torch.float64, device="cuda"), torch.full((B, 6), 7.0, dtype=torch.float64, device="cuda")
    need = L.df_mesh_icp_scratch_bytes(T, B, N)
    scratch = torch.full((need + 16,), 7, dtype=torch.uint8, device="cuda")
    good = dict(vertices=dv.data_ptr(), V=V, triangles=dt.data_ptr(), T=T, begin=begin.ctypes.data, md=md.ctypes.data, O=1, obj=obj.data_ptr(),
                points=pts.data_ptr(), pose=pose.data_ptr(), B=B, N=N, iters=2, cull=0, out=out.data_ptr(), stats=stats.data_ptr(),
                scratch=scratch.data_ptr(), scratch_bytes=need, stream=_lib.current_stream(), **tree_good)
    two = np.array([0, 1, T], dtype=np.int32)                    # the tree was built for one object of 24 triangles, not for 1 + 23
    errors = [dict(vertices=None), dict(begin=None), dict(md=None), dict(obj=None), dict(out=None), dict(stats=None), dict(scratch=None), dict(V=0),
              dict(T=0), dict(B=0), dict(N=0), dict(O=0), dict(O=65), dict(iters=-1), dict(iters=65), dict(cull=2), dict(scratch_bytes=need - 1),
              dict(scratch=scratch.data_ptr() + 8), dict(out=pose.data_ptr()), dict(stats=out.data_ptr() + 8),
              dict(begin=np.array([0, T + 1], dtype=np.int32).ctypes.data), dict(md=np.array([0.0]).ctypes.data)] + tree_errors
    assert tree.n_nodes > 1
    keep = [two, np.array([0, tree.n_nodes, tree.n_nodes], dtype=np.int32), np.array([0, 0, 0], dtype=np.int32), np.array([1.0, 1.0])]
    errors.append(dict(begin=keep[0].ctypes.data, O=2, nb=keep[1].ctypes.data, lb=keep[2].ctypes.data, md=keep[3].ctypes.data))
    for kw in errors:
        a = dict(good, **kw)
        assert L.df_mesh_icp_tree(*[a[k] for k in good]) == -1, kw
        assert len(L.df_last_error()) > 10, kw
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((stats == 7).all()) and bool((scratch == 7).all()), "nothing was written"
    assert L.df_mesh_icp_tree(*good.values()) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7).any()) and bool((scratch[need:] == 7).all())


def test_the_wrappers_give_the_same_bytes_with_accel():
    """``MeshIcp(accel=True).refine`` on the eight rendered views of ``test_icp_on_rendered_views`` and the distance wrapper on the
    queries ``detect_symmetry`` sends for the bracket: the bytes of ``accel=False``; and the two reports of the detection are equal."""
    _dev()
    import test_mesh_icp_gpu as base
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    from densefusion_amd.datasets.customCAD.symmetry import detect_symmetry
    from densefusion_amd.lib.mesh_distance import mesh_closest
    from densefusion_amd.lib.mesh_set import MeshTree
    np.random.seed(1)
    ds = RenderedPoseDataset(base._bracket_model(), 500, False, 0.0, False, raster="mesh", proj_mat=fab.PROJ[1], chunk=16, first_seed=0, frames=128,
                             max_holes=1, **base.FRAME)
    plain, fast = ds.mesh_icp(), ds.mesh_icp(accel=True)
    assert plain.tree is None and fast.tree.n_loose == 0 and fast.tree.n_order == 24 and fast.tree is ds.mesh_icp(accel=True).tree, "built once"
    D = icp.diameter(fast.vertices.cpu().numpy())
    rng = np.random.default_rng(9)
    live = [i for i in range(128) if ds.view_info(i)["live"] and base._third_face_cosine(ds.view_info(i)["pose"]) >= 0.15][:base.VIEWS]
    assert len(live) == base.VIEWS
    clouds, starts = [], []
    for i in live:
        clouds.append(ds[i][0].reshape(-1, 3))
        info = ds.view_info(i)
        truth = np.concatenate([icp.quat_from_matrix(info["pose"][:, :3]), info["pose"][:, 3] / 10000.0])
        starts.append(icp.perturb(truth, rng, np.radians(5), 0.05 * D))
    points, start = torch.stack(clouds).float().contiguous(), _up(np.stack(starts), np.float64)
    obj = torch.zeros(len(live), dtype=torch.int32, device="cuda")
    for kw in (dict(iters=10), dict(iters=3, max_dist=0.02 * D, cull=True)):
        a, b = plain.refine(points, start, obj, **kw), fast.refine(points, start, obj, **kw)
        assert m.same_bits(a[0].cpu().numpy(), b[0].cpu().numpy()) and m.same_bits(a[1].cpu().numpy(), b[1].cpu().numpy()), kw
        assert (a[1][:, 0] == 0).sum() >= 1
    # the distance wrapper on the detection's own queries
    bv, bt = m.bracket()
    seen = {}

    def catch(v, t, p, xf, want):
        seen.update(v=v, t=t, p=p, xf=xf)
        return np.zeros((len(xf), len(p))), np.zeros((len(xf), len(p)), dtype=np.int32), None

    detect_symmetry(bv, bt, closest=catch)
    up = [_up(seen["v"], np.float32), _up(seen["t"], np.int32), _up(seen["p"], np.float64), _up(seen["xf"], np.float64)]
    a = mesh_closest(*up)
    for b in (mesh_closest(*up, accel=True), mesh_closest(*up, accel=True, tree=MeshTree(seen["v"], seen["t"]))):
        assert all(m.same_bits(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        mesh_closest(*up, accel=True, tree=MeshTree(*m.icosphere(1)))
    ra, rb = detect_symmetry(bv, bt), detect_symmetry(bv, bt, accel=True)
    assert m.same_bits(ra.residuals, rb.residuals) and ra.passed == rb.passed and ra.symmetric == rb.symmetric


def test_the_eval_tool_gives_the_same_lines_with_icp_accel(tmp_path):
    _dev()
    import test_mesh_icp_gpu as base
    from densefusion_amd.lib.network import PoseNet, PoseRefineNet
    paths = [str(mnp.write_mesh_ply(tmp_path / name, *mesh)) for name, mesh in zip(("big.ply", "small.ply", "box.ply"), snp.tool_meshes())]
    pm = rnp.write_proj(tmp_path / "proj_in.txt", fab.PROJ[1])
    torch.manual_seed(3)
    torch.save(PoseNet(num_points=500, num_obj=5).state_dict(), tmp_path / "pose.pth")
    torch.save(PoseRefineNet(num_points=500, num_obj=5).state_dict(), tmp_path / "refine.pth")
    tool = base._tool("eval_cad_render")

    def run(out, *extra):
        return tool.main(["--cad_model", paths[0], paths[1], "--cad_distractor", paths[2], "--model", str(tmp_path / "pose.pth"), "--refine_model",
                          str(tmp_path / "refine.pth"), "--masks", "truth", "--cad_seed", "0", "--cad_frames", str(base.VIEWS), "--proj_mat", pm,
                          "--height", "64", "--width", "96", "--min_pixels", "60", "--mask", "pixels", "--chunk", "4", "--workers", "0",
                          "--iteration", "2", "--output_result_dir", str(tmp_path / out), "--icp", "2", *extra])

    scan, tree = run("scan"), run("tree", "--icp_accel")
    assert scan == tree and sorted(tree) == ["truth", "truth_icp"] and tree["truth_icp"]["icp"]["items"] >= 3
    for name in sorted(os.listdir(tmp_path / "scan")):
        assert open(tmp_path / "scan" / name).read() == open(tmp_path / "tree" / name).read(), name
    assert sorted(os.listdir(tmp_path / "tree")) == sorted(os.listdir(tmp_path / "scan"))
