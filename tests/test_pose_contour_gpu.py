"""GPU: ``df_pose_refine_contour`` against its restatement (tests/pose_contour_np.py) bit for bit in ``pose_out`` and all eight stats columns,
its feature map against E2's brute force, its refusals, the wrapper ``lib.pose_refine_contour.ContourPoseRefiner`` and
``RenderedPoseDataset.contour_refiner()``.

Frames are 24 x 32 (``pose_dense_np.make_scene``).  The accumulation has the dense call's shape (tiles of 2048 slots, 8 sweeps of 256 lanes,
4 waves, 64 tile blocks an item at most) and the feature transform's row pass takes strips of 256 columns: the windows stand one slot
below, at and above each of these."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

import fabricate_cad as fab
import mesh_closest_np as m
import mesh_icp_np as icp
import pose_contour_np as cn
import pose_dense_np as dn
import pose_verify_np as pv

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A
REACH, EDGE, SCALE = 6, 65535, 0.5


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _up(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


class Call:
    """One ``df_pose_refine_contour`` call on a scene with every argument open to a test: ``run(**changes)`` -> (rc, pose_out, stats)."""

    def __init__(self, sc, items, pose, WH, WW, gate, iters, edge_step=EDGE, reach=REACH, scale=SCALE, cull=0, mask=True, cloud_div=dn.CLOUD_DIV):
        from densefusion_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.v, self.t = _up(sc["vertices"], np.float32), _up(sc["triangles"], np.int32)
        self.begin = np.ascontiguousarray(sc["tri_begin"], dtype=np.int32)
        self.scale = np.ascontiguousarray(sc["model_scale"], dtype=np.float64)
        self.proj = np.ascontiguousarray(sc["proj"], dtype=np.float64).reshape(-1)
        self.depth, self.mask = _up(sc["depth"], np.uint16), (_up(sc["mask"], np.uint16) if mask else None)
        self.rays = _up(sc["rays"], np.float64)
        self.items, self.pose = _up(items, np.int32), _up(pose, np.float64)
        F, IH, IW = sc["depth"].shape
        self.a = dict(vertices=self.v.data_ptr(), V=len(sc["vertices"]), triangles=self.t.data_ptr(), T=len(sc["triangles"]),
                      tri_begin=self.begin.ctypes.data, model_scale=self.scale.ctypes.data, O=len(self.begin) - 1, proj=self.proj.ctypes.data,
                      depth=self.depth.data_ptr(), F=F, IH=IH, IW=IW, rays=self.rays.data_ptr(), mask=self.mask.data_ptr() if mask else None,
                      NM=len(sc["mask"]) if mask else 0, items=self.items.data_ptr(), pose_in=self.pose.data_ptr(), cloud_div=cloud_div,
                      B=len(items), WH=WH, WW=WW, gate=gate, cull=cull, iters=iters, edge_step=edge_step, reach=reach, contour_scale=scale)

    def run(self, short_scratch=0, misalign=0, null=(), alias=None, out_misalign=(), **changes):
        a = dict(self.a, **changes)
        B = len(self.items)
        need = max(self.L.df_pose_refine_contour_scratch_bytes(B, self.a["WH"], self.a["WW"]), 8)
        pose_out = torch.empty(B * 7 + 1, dtype=torch.float64, device="cuda").view(torch.uint8).fill_(SENTINEL).view(torch.float64)
        stats = torch.empty(B * 8 + 1, dtype=torch.float64, device="cuda").view(torch.uint8).fill_(SENTINEL).view(torch.float64)
        scratch = torch.full((need + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
        ptr = dict(pose_out=pose_out.data_ptr() + (4 if "pose_out" in out_misalign else 0),
                   stats=stats.data_ptr() + (4 if "stats" in out_misalign else 0), scratch=scratch.data_ptr() + misalign)
        if alias == "pose_out=pose_in":
            ptr["pose_out"] = a["pose_in"]
        elif alias == "stats=pose_in":
            ptr["stats"] = a["pose_in"]
        elif alias == "stats=pose_out":
            ptr["stats"] = ptr["pose_out"] + 8
        elif alias == "pose_out=scratch":
            ptr["pose_out"] = ptr["scratch"] + need - 8
        elif alias == "stats=depth":
            ptr["stats"] = a["depth"]
        elif alias == "pose_out=rays":
            ptr["pose_out"] = a["rays"] + 8
        for k in null:
            ptr[k] = None
        rc = self.L.df_pose_refine_contour(a["vertices"], a["V"], a["triangles"], a["T"], a["tri_begin"], a["model_scale"], a["O"], a["proj"],
                                           a["depth"], a["F"], a["IH"], a["IW"], a["rays"], a["mask"], a["NM"], a["items"], a["pose_in"],
                                           ctypes.c_double(a["cloud_div"]), a["B"], a["WH"], a["WW"], a["gate"], a["cull"], a["iters"],
                                           a["edge_step"], a["reach"], ctypes.c_double(a["contour_scale"]), ptr["pose_out"], ptr["stats"],
                                           ptr["scratch"], need - short_scratch, self.lib.current_stream())
        torch.cuda.synchronize()
        self.last_scratch = scratch
        return rc, pose_out.cpu().numpy()[:B * 7].reshape(B, 7), stats.cpu().numpy()[:B * 8].reshape(B, 8)

    def feature(self):
        """The feature map [B,WH,WW] the last call left in its scratch: after the dense call's parts and the six columns an item."""
        B, WH, WW = len(self.items), self.a["WH"], self.a["WW"]
        at = self.L.df_pose_refine_dense_scratch_bytes(B, WH, WW) + B * 6 * 8
        return self.last_scratch[at:at + 4 * B * WH * WW].cpu().numpy().view(np.int32).reshape(B, WH, WW)


def _device(sc, items, pose, WH, WW, gate, iters, **kw):
    call = Call(sc, items, pose, WH, WW, gate, iters, **kw)
    rc, po, st = call.run()
    assert rc == 0, call.L.df_last_error()
    return po, st, call


def _want(sc, items, pose, WH, WW, gate, iters, edge_step=EDGE, reach=REACH, scale=SCALE, cull=0, mask=True, trace=None):
    return cn.contour_np(sc["vertices"], sc["triangles"], sc["tri_begin"], sc["model_scale"], sc["proj"], sc["depth"], sc["rays"],
                         sc["mask"] if mask else None, items, pose, dn.CLOUD_DIV, WH, WW, gate, iters, edge_step, reach, scale, cull, trace)


def _same(got, want, name):
    for what, g, w in (("pose_out", got[0], want[0]), ("stats", got[1], want[1])):
        bad = np.where((g.view(np.uint64) != w.view(np.uint64)).any(axis=1))[0]
        assert g.dtype == np.float64 and len(bad) == 0, f"{name}: {what} differs in rows {bad.tolist()}\n{g[bad][:3]}\n{w[bad][:3]}\nstats\n{want[1][bad][:3]}"


def _same_features(call, trace, name):
    """the device's feature map of every good item against E2 by brute force (the restatement's, from its trace)"""
    got = call.feature()
    for b, tr in enumerate(trace):
        if tr:
            assert np.array_equal(got[b], tr[0][3]), f"{name}: the feature map of item {b} differs at slots {np.nonzero(got[b] != tr[0][3])[0][:5]}"


@pytest.fixture(scope="module")
def scene():
    _dev()
    return dn.make_scene()


# test_pose_dense_gpu.py's windows (sweep, tile and tile-block boundaries), and 1 x 255 / 256 / 257 / 513 columns for the row strips
WINDOWS = ((1, 1, 12, 8), (1, 65, 12, -35), (3, 3, 11, 7), (15, 17, 5, 8), (16, 16, 4, 8), (1, 257, 12, -227), (257, 1, -238, 8),
           (23, 89, 0, -40), (32, 64, -4, -16), (683, 3, -671, 26), (24, 100, 0, 0), (24, 100, 0, -68), (4, 32768, 10, -32740),
           (4, 32769, 10, -32740), (2, 255, 11, -230), (2, 256, 11, -230), (3, 513, 10, -250))


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "%dx%d" % w[:2])
def test_windows_at_every_tile_sweep_and_strip_boundary(scene, window):
    """Object 3 fills most of the frame; its frame has holes and its mask a ragged border, so wherever the window's existing nodes lie
    there is an observed outline.  edge_step 0 makes every drawn node whose neighbour lies behind it an outline node: pairs in every
    tile that holds inliers."""
    WH, WW, r0, c0 = window
    items, pose = dn.make_call([3], WH, WW, 11, corner=(r0, c0))
    trace = []
    want = _want(scene, items, pose, WH, WW, dn.GATE, 2, edge_step=0, trace=trace)
    pairs = np.where(trace[0][0][2])[0]
    tiles = sorted(set((pairs // dn.TILE).tolist()))
    print(window, "stats", want[1][0].tolist(), "pair slots", len(pairs), "tiles", tiles)
    if WH * WW > 1:
        assert len(pairs) > 0
    if (WH, WW) in ((24, 100), (683, 3), (4, 32769), (4, 32768)):
        assert len(tiles) >= 2, "pairs on both sides of a tile boundary"
    if (WH, WW) == (4, 32769):
        assert tiles[-1] == dn.MAX_TILE_BLOCKS, "the 65th tile, which tile block 0 takes in its second round, holds pairs"
    po, st, call = _device(scene, items, pose, WH, WW, dn.GATE, 2, edge_step=0)
    _same_features(call, trace, str(window))
    _same((po, st), want, str(window))


def test_window_positions(scene):
    """9 x 13 windows at the frame's origin, inside, over each edge and each vertex of the frame, and wholly outside: one call."""
    cs = dn.corners(9, 13)
    rng = np.random.default_rng(5)
    items = np.array([[3, 3, r0, c0, 3, 7] for r0, c0 in cs], dtype=np.int32)
    pose = dn.start_poses([3] * len(cs), rng)
    trace = []
    want = _want(scene, items, pose, 9, 13, dn.GATE, 2, trace=trace)
    print(want[1])
    outside = [b for b, (r0, c0) in enumerate(cs) if r0 >= dn.IH or c0 >= dn.IW or r0 + 9 <= 0 or c0 + 13 <= 0]
    assert len(outside) == 4 and (want[1][outside, 0] == cn.FEW).all() and not want[1][outside, 1:].any(), "wholly outside: few inliers"
    assert (want[1][:6, 6] > 0).all(), "at the origin, inside and over each edge there are pairs"
    po, st, call = _device(scene, items, pose, 9, 13, dn.GATE, 2)
    _same_features(call, trace, "positions")
    _same((po, st), want, "positions")


def _boundary_step(scene):
    """an edge_step that is exactly the difference co_nb - co of two neighbouring nodes of frame 3 (inside the mask): at it the pair is no
    outline by this neighbour, one below it is"""
    d = scene["depth"][3].astype(np.int64)
    on = (d != 65535) & (scene["mask"][3] == 7)
    diff = np.where(on[:, 1:] & on[:, :-1], d[:, 1:] - d[:, :-1], 0)
    steps = np.unique(diff[diff > 1])
    return int(steps[len(steps) // 2])


@pytest.mark.parametrize("reach", (0, 1, 6, 64))
@pytest.mark.parametrize("edge", ("zero", "at", "below", "max"))
def test_reach_and_edge_step(scene, reach, edge):
    """B = 5 whole-frame windows; reach 64 is larger than the window."""
    at = _boundary_step(scene)
    edge_step = {"zero": 0, "at": at, "below": at - 1, "max": 65535}[edge]
    items, pose = dn.make_call([0, 1, 2, 3, 4], dn.IH, dn.IW, 3)
    trace = []
    want = _want(scene, items, pose, dn.IH, dn.IW, dn.GATE, 2, edge_step=edge_step, reach=reach, trace=trace)
    if edge in ("at", "below"):
        a, b = (cn.observed_outline(scene["depth"][3], scene["mask"][3], 7, 0, 0, dn.IH, dn.IW, e) for e in (at, at - 1))
        assert b.sum() > a.sum() and not (a & ~b).any(), "one code below the difference there are more outline nodes"
    print(reach, edge_step, want[1][:, [0, 5, 6, 7]].tolist())
    assert (want[1][1:, 6] > 0).all()
    po, st, call = _device(scene, items, pose, dn.IH, dn.IW, dn.GATE, 2, edge_step=edge_step, reach=reach)
    _same_features(call, trace, f"reach {reach} edge_step {edge_step}")
    _same((po, st), want, f"reach {reach} edge_step {edge_step}")


@pytest.mark.parametrize("iters", (0, 1, 4))
@pytest.mark.parametrize("mask", (False, True))
@pytest.mark.parametrize("cull", (0, 1))
def test_meshes_iterations_mask_and_cull(scene, iters, mask, cull):
    """B = 5: the meshes of 1 (the flat wall), 63, 64, 65 and 257 triangles, each on its own frame, whole-frame windows."""
    items, pose = dn.make_call([0, 1, 2, 3, 4], dn.IH, dn.IW, 3)
    want = _want(scene, items, pose, dn.IH, dn.IW, dn.GATE, iters, edge_step=300, cull=cull, mask=mask)
    print(iters, mask, cull, want[1])
    assert (want[1][[1, 4], 6] > 0).all()
    if iters == 0:
        assert not want[1][:, 0].any() and not want[1][:, 5].any() and m.same_bits(want[1][:, 6], want[1][:, 7])
        assert m.same_bits(want[0], np.stack([icp.normalised(p) for p in pose])), "iters = 0 only scores"
    po, st, _ = _device(scene, items, pose, dn.IH, dn.IW, dn.GATE, iters, edge_step=300, cull=cull, mask=mask)
    _same((po, st), want, f"iters {iters} mask {mask} cull {cull}")


def _dense_device(call, iters=None):
    """``df_pose_refine_dense`` on the call's own inputs: (pose_out, stats [B,6])"""
    a, L = call.a, call.L
    B = a["B"]
    po, st = torch.zeros(B, 7, dtype=torch.float64, device="cuda"), torch.zeros(B, 6, dtype=torch.float64, device="cuda")
    scratch = torch.empty(L.df_pose_refine_dense_scratch_bytes(B, a["WH"], a["WW"]), dtype=torch.uint8, device="cuda")
    rc = L.df_pose_refine_dense(a["vertices"], a["V"], a["triangles"], a["T"], a["tri_begin"], a["model_scale"], a["O"], a["proj"], a["depth"],
                                a["F"], a["IH"], a["IW"], a["rays"], a["mask"], a["NM"], a["items"], a["pose_in"], ctypes.c_double(a["cloud_div"]),
                                B, a["WH"], a["WW"], a["gate"], a["cull"], a["iters"] if iters is None else iters, po.data_ptr(), st.data_ptr(),
                                scratch.data_ptr(), scratch.numel(), call.lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0
    return po.cpu().numpy(), st.cpu().numpy()


def test_nothing_to_pair_and_scale_zero_equal_the_dense_call(scene):
    """A frame with no observed outline (every node observed, no mask, edge_step 65535); a drawn model with no outline inside its window
    (a 5 x 5 window inside object 3's drawing, around a hole of the frame); contour_scale 0 with pairs: ``df_pose_refine_dense``'s bytes."""
    sc = dict(scene)
    depth = scene["depth"].copy()
    depth[depth == 65535] = 64000
    sc["depth"] = depth
    items, pose = dn.make_call([1, 3, 4], dn.IH, dn.IW, 13)
    po, st, call = _device(sc, items, pose, dn.IH, dn.IW, dn.GATE, 3, mask=False)
    assert (call.feature() == cn.NONE).all() and not st[:, 6:].any() and (st[:, 5] == 3).all()
    _same((po, st), _want(sc, items, pose, dn.IH, dn.IW, dn.GATE, 3, mask=False), "no observed outline")
    dp, ds = _dense_device(call)
    assert m.same_bits(po, dp) and m.same_bits(st[:, :6], ds)
    # inside the drawing
    found = None
    for r0 in range(2, dn.IH - 7):
        for c0 in range(2, dn.IW - 7):
            it, ps = dn.make_call([3], 5, 5, 2, corner=(r0, c0))
            trace = []
            want = _want(scene, it, ps, 5, 5, dn.GATE, 1, mask=False, trace=trace)
            keys, _, pair, feat = trace[0][0]
            if (keys != pv.NO_KEY).all() and (feat != cn.NONE).any() and want[1][0, 5] == 1:
                found = (it, ps, want)
                break
        if found:
            break
    assert found is not None and found[2][1][0, 6] == 0
    po, st, call = _device(scene, found[0], found[1], 5, 5, dn.GATE, 1, mask=False)
    _same((po, st), found[2], "no drawn outline")
    dp, ds = _dense_device(call)
    assert m.same_bits(po, dp) and m.same_bits(st[:, :6], ds)
    # scale 0
    items, pose = dn.make_call([0, 1, 2, 3, 4], dn.IH, dn.IW, 3)
    po, st, call = _device(scene, items, pose, dn.IH, dn.IW, dn.GATE, 4, scale=0.0)
    dp, ds = _dense_device(call)
    assert (st[1:, 6] > 0).all() and m.same_bits(po, dp) and m.same_bits(st[:, :6], ds), "contour_scale = 0"
    _same((po, st), _want(scene, items, pose, dn.IH, dn.IW, dn.GATE, 4, scale=0.0), "scale 0")


def test_symmetric_tie_frame(scene):
    """Frame 3 with every node observed but a lattice of single holes 4 nodes apart: the outline nodes around them stand at equal
    distances from many nodes (two and eight nearest).  The device's feature map is E2's lowest slot among the nearest."""
    sc = dict(scene)
    depth = scene["depth"].copy()
    d3 = np.where(depth[3] == 65535, 64000, depth[3])
    d3[2::4, 2::4] = 65535
    depth[3] = d3
    sc["depth"] = depth
    for (WH, WW, corner) in ((dn.IH, dn.IW, (0, 0)), (11, 300, (5, -260))):
        items, pose = dn.make_call([3], WH, WW, 4, corner=corner)
        trace = []
        want = _want(sc, items, pose, WH, WW, dn.GATE, 2, reach=4, mask=False, trace=trace)
        feat = trace[0][0][3]
        exists = cn.window_exists(corner[0], corner[1], WH, WW, dn.IH, dn.IW)
        edge = cn.observed_outline(d3, None, 0, corner[0], corner[1], WH, WW, EDGE)
        if WH == dn.IH:
            assert np.array_equal(feat, cn.feature_map_loops(exists, edge, 4)), "the restatement's own check"
            assert feat[4, 4] == 2 * WW + 3 and feat[4, 2] == 3 * WW + 2 and feat[2, 4] == 2 * WW + 3, "eight and two nearest: the lowest slot"
        po, st, call = _device(sc, items, pose, WH, WW, dn.GATE, 2, reach=4, mask=False)
        _same_features(call, trace, "ties")
        _same((po, st), want, "ties")


def test_batches_reordered_alone_and_twice(scene):
    objs = [1, 3, 4, 0, 2, 3, 1, 4, 3, 1, 4, 3]
    items, pose = dn.make_call(objs, 17, 37, 9)
    call = Call(scene, items, pose, 17, 37, dn.GATE, 3, edge_step=300)
    (rc1, p1, s1), (rc2, p2, s2) = call.run(), call.run()
    assert rc1 == rc2 == 0 and p1.tobytes() == p2.tobytes() and s1.tobytes() == s2.tobytes(), "two identical calls give identical bytes"
    _same((p1, s1), _want(scene, items, pose, 17, 37, dn.GATE, 3, edge_step=300), "B = 12")
    order = [4, 2, 0, 3, 1]
    po, so, _ = _device(scene, items[order], pose[order], 17, 37, dn.GATE, 3, edge_step=300)
    assert po.tobytes() == p1[order].tobytes() and so.tobytes() == s1[order].tobytes(), "B = 5: the same items reordered"
    for b in (0, 1, 3, 7):
        pb, sb, _ = _device(scene, items[b:b + 1], pose[b:b + 1], 17, 37, dn.GATE, 3, edge_step=300)
        assert pb.tobytes() == p1[b:b + 1].tobytes() and sb.tobytes() == s1[b:b + 1].tobytes(), f"item {b} alone equals its row of the call"


def test_bad_items_and_bad_poses_leave_their_neighbours_alone(scene):
    rng = np.random.default_rng(6)
    objs = [3, 4, 3, 1, 3, 4, 3, 3, 1, 4, 3, 4]
    items = np.array([[o, o, 2, 3, o, 7] for o in objs], dtype=np.int32)
    pose = dn.start_poses(objs, rng)
    good = items.copy()
    F, O = len(scene["depth"]), len(dn.COUNTS)
    for b, (col, val) in {1: (0, -1), 2: (0, F), 4: (1, -1), 5: (1, O), 7: (4, -1), 8: (4, len(scene["mask"]))}.items():
        items[b, col] = val
    pose[9, :4] = 0.0                                             # a zero quaternion
    pose[10, 2] = np.nan                                          # a NaN in the quaternion
    pose[11, 5] = np.nan                                          # a NaN translation
    want = _want(scene, items, pose, 19, 23, dn.GATE, 3)
    print(want[1])
    assert want[1][:, 0].tolist() == [0, 3, 3, 0, 3, 3, 0, 3, 3, 1, 1, 1] and not want[1][[1, 2, 4, 5, 7, 8, 9, 10, 11], 1:].any()
    po, st, _ = _device(scene, items, pose, 19, 23, dn.GATE, 3)
    _same((po, st), want, "bad items and poses")
    cp, cs, _ = _device(scene, good, pose, 19, 23, dn.GATE, 3)
    for b in (0, 3, 6):
        assert m.same_bits(po[b], cp[b]) and m.same_bits(st[b], cs[b]), "the neighbours of a bad item are unchanged"
    want = _want(scene, items, pose, 19, 23, dn.GATE, 3, mask=False)                  # without a mask the mask frame is not looked at
    assert want[1][:, 0].tolist() == [0, 3, 3, 0, 3, 3, 0, 0, 0, 1, 1, 1]
    _same(_device(scene, items, pose, 19, 23, dn.GATE, 3, mask=False)[:2], want, "bad items, no mask")


def _verify(call):
    a, L = call.a, call.L
    B = a["B"]
    stats = torch.zeros(B, 12, dtype=torch.int64, device="cuda")
    scratch = torch.empty(L.df_pose_verify_scratch_bytes(B, a["WH"], a["WW"]), dtype=torch.uint8, device="cuda")
    rc = L.df_pose_verify(a["vertices"], a["V"], a["triangles"], a["T"], a["tri_begin"], a["model_scale"], a["O"], a["proj"], a["depth"], a["F"],
                          a["IH"], a["IW"], a["mask"], a["NM"], a["items"], a["pose_in"], ctypes.c_double(a["cloud_div"]), B, a["WH"], a["WW"], 8, 0,
                          stats.data_ptr(), scratch.data_ptr(), scratch.numel(), call.lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0
    return stats.cpu().numpy()


def test_the_verifier_and_the_dense_call_are_unchanged(scene):
    items, pose = dn.make_call([1, 3, 4, 0, 2], 17, 37, 9)
    call = Call(scene, items, pose, 17, 37, dn.GATE, 3)
    v0, d0 = _verify(call), _dense_device(call)
    assert m.same_bits(v0, pv.verify_np(scene["vertices"], scene["triangles"], scene["tri_begin"], scene["model_scale"], scene["proj"],
                                        scene["depth"], scene["mask"], items, pose, dn.CLOUD_DIV, 17, 37, 8))
    want = dn.dense_np(scene["vertices"], scene["triangles"], scene["tri_begin"], scene["model_scale"], scene["proj"], scene["depth"],
                       scene["rays"], scene["mask"], items, pose, dn.CLOUD_DIV, 17, 37, dn.GATE, 3)
    assert m.same_bits(d0[0], want[0]) and m.same_bits(d0[1], want[1])
    rc, _, _ = call.run()
    assert rc == 0
    v1, d1 = _verify(call), _dense_device(call)
    assert v1.tobytes() == v0.tobytes() and d1[0].tobytes() == d0[0].tobytes() and d1[1].tobytes() == d0[1].tobytes()


def test_argument_errors_touch_nothing(scene):
    items, pose = dn.make_call([1, 3, 4], 16, 16, 11)
    call = Call(scene, items, pose, 16, 16, dn.GATE, 2)
    L = call.L
    dense = L.df_pose_refine_dense_scratch_bytes
    assert L.df_pose_refine_contour_scratch_bytes(3, 16, 16) == dense(3, 16, 16) + 3 * 6 * 8 + 3 * 256 * 4 + 3 * 32 * 8
    assert L.df_pose_refine_contour_scratch_bytes(1, 1, 2049) == dense(1, 1, 2049) + 6 * 8 + 2050 * 4 + 2 * 32 * 8, "the feature map is rounded up to 8 bytes"
    assert L.df_pose_refine_contour_scratch_bytes(0, 16, 16) == 0 and L.df_pose_refine_contour_scratch_bytes(65536, 1, 1) == 0
    assert L.df_pose_refine_contour_scratch_bytes(1, 0, 5) == 0 and L.df_pose_refine_contour_scratch_bytes(1, 1 << 15, (1 << 15) + 1) == 0
    begin_bad0, begin_dec, begin_end = call.begin.copy(), call.begin.copy(), call.begin.copy()
    begin_bad0[0], begin_dec[2], begin_end[-1] = 1, begin_dec[1] - 1, begin_end[-1] - 1
    proj_bad = call.proj.copy()
    proj_bad[14] = -2.0
    bad = [dict(vertices=None), dict(triangles=None), dict(tri_begin=None), dict(model_scale=None), dict(proj=None), dict(depth=None),
           dict(rays=None), dict(items=None), dict(pose_in=None), dict(null=("pose_out",)), dict(null=("stats",)), dict(null=("scratch",)),
           dict(NM=0), dict(NM=-1), dict(B=0), dict(B=65536), dict(WH=0), dict(WW=0), dict(WH=-1), dict(WH=1 << 15, WW=(1 << 15) + 1),
           dict(F=0), dict(F=65536), dict(IH=0), dict(IW=0), dict(IH=1 << 15, IW=(1 << 15) + 1), dict(V=0), dict(T=0), dict(O=0), dict(O=65),
           dict(tri_begin=begin_bad0.ctypes.data), dict(tri_begin=begin_dec.ctypes.data), dict(tri_begin=begin_end.ctypes.data),
           dict(proj=proj_bad.ctypes.data), dict(gate=-1), dict(gate=65536), dict(iters=-1), dict(iters=65), dict(cull=2), dict(cull=-1),
           dict(cloud_div=0.0), dict(cloud_div=-1.0), dict(cloud_div=float("inf")), dict(cloud_div=float("nan")), dict(short_scratch=1),
           dict(misalign=4), dict(rays=call.rays.data_ptr() + 4), dict(pose_in=call.pose.data_ptr() + 4), dict(out_misalign=("pose_out",)),
           dict(out_misalign=("stats",)), dict(alias="pose_out=pose_in"), dict(alias="stats=pose_in"), dict(alias="stats=pose_out"),
           dict(alias="pose_out=scratch"), dict(alias="stats=depth"), dict(alias="pose_out=rays"),
           dict(edge_step=-1), dict(edge_step=65536), dict(reach=-1), dict(reach=65), dict(contour_scale=-0.5), dict(contour_scale=float("inf")),
           dict(contour_scale=float("nan"))]
    inputs = [t.clone() for t in (call.pose, call.depth, call.rays)]
    for change in bad:
        rc, po, st = call.run(**change)
        assert rc == -1 and L.df_last_error(), f"{change}: DF_ERR_ARG expected, got {rc}"
        assert (po.view(np.uint8) == SENTINEL).all() and (st.view(np.uint8) == SENTINEL).all(), f"{change}: the call wrote before it refused"
        assert (call.last_scratch == SENTINEL).all(), f"{change}: the call wrote to the scratch before it refused"
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(inputs, (call.pose, call.depth, call.rays)))
    rc, po, st = call.run(reach=64, edge_step=0, contour_scale=0.0)
    assert rc == 0, "the ends of the ranges are taken"
    rc, po, st = call.run()
    assert rc == 0
    _same((po, st), _want(scene, items, pose, 16, 16, dn.GATE, 2), "after the refusals")


# Rendered 64 x 96 views (seed 0, 128 frames) of the bracket and of the box(1, 2, 3) that show too few faces to hold a pose: the dense rule
# freezes on them as degenerate without a step.  Chosen from a survey of all live views under both rules (DESIGN 12p says how many were
# tried and what the others gave); the test holds the device to the restatements on them.
TWO_FACE_VIEWS = {"bracket": (15, 28, 36, 46, 67, 75, 86, 114), "box": (10, 20, 23, 40, 47, 48, 55, 124)}


@pytest.mark.parametrize("name", ("bracket", "box"))
def test_wrapper_and_contour_refiner_on_two_face_views(name):
    """From starts a few degrees and millimetres off, ``dense_refiner()`` returns `degenerate` and the start on every view; ``contour_refiner()``
    returns status 0 and a lower MSSD, and its outputs equal the restatement's; then the argument errors and the raises."""
    _dev()
    tool_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tool_dir)
    try:
        import importlib
        tool = importlib.import_module("eval_cad_render")
    finally:
        sys.path.pop(0)
    import pose_error_np as pe
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    from densefusion_amd.lib import pose_refine_contour as prc
    v, t = m.bracket() if name == "bracket" else m.box(1, 2, 3)
    model = (v * np.float32(30.0), t, np.random.default_rng(5).integers(0, 256, (len(v), 3), dtype=np.uint8))
    kw = dict(raster="mesh", proj_mat=fab.PROJ[1], chunk=16, first_seed=0, frames=128, max_holes=1, image_dims=(64, 96), min_pixels=60)
    np.random.seed(1)
    ds = RenderedPoseDataset(model, 500, False, 0.0, False, keep_frames=True, **kw)
    live = [i for i in range(128) if ds.view_info(i)["live"]]
    views = list(TWO_FACE_VIEWS[name])
    n = len(views)
    assert set(views) <= set(live)
    ref = ds.contour_refiner()
    assert isinstance(ref, prc.ContourPoseRefiner) and ref.rays is not None and len(prc.STATS) == 8 and prc.STATS[6:] == ("first_pairs", "last_pairs")
    # the starts of the survey that chose the views: one draw over all live views
    gt_all = np.stack([tool.true_pose(ds, i) for i in live])
    rng = np.random.default_rng(9)
    start_all = gt_all + np.concatenate([rng.normal(scale=0.02, size=(len(live), 4)), rng.normal(scale=0.0003, size=(len(live), 3))], axis=1)
    pick = [live.index(i) for i in views]
    gt, start = gt_all[pick], start_all[pick]
    infos = [ds.view_info(i) for i in views]
    depth = torch.stack([f["depth"] for f in infos])
    margin = 8
    window = (max(f["box"][1] - f["box"][0] for f in infos) + 2 * margin, max(f["box"][3] - f["box"][2] for f in infos) + 2 * margin)
    corner = np.array([[f["box"][0] - margin, f["box"][2] - margin] for f in infos])
    frame, obj = np.arange(n), np.zeros(n, dtype=np.int64)
    items = np.concatenate([frame[:, None], obj[:, None], corner, np.zeros((n, 2), dtype=np.int64)], axis=1)
    dev = (depth, _up(start, np.float64), _up(frame, np.int64), _up(obj, np.int64), _up(corner, np.int64), window)
    gate, cull = 400, bool(ds.cull)
    dp, dst = ds.dense_refiner().refine(*dev, iters=10, gate=gate, cull=cull)
    dp, dst = dp.cpu().numpy(), dst.cpu().numpy()
    assert (dst[:, 0] == cn.DEGENERATE).all() and (dst[:, 5] == 0).all() and m.same_bits(dp, np.stack([icp.normalised(p) for p in start]))
    po, st = ref.refine(*dev, iters=10, gate=gate, cull=cull)
    assert po.is_cuda and st.is_cuda and po.dtype == st.dtype == torch.float64 and tuple(st.shape) == (n, 8)
    po, st = po.cpu().numpy(), st.cpu().numpy()
    want = cn.contour_np(ds.meshes.vertices, ds.meshes.triangles, ds.meshes.tri_begin, np.array([ds.model_scale]), ds.proj_mat, depth.cpu().numpy(),
                         ds.udp.ray_map, None, items, start, 10000.0, window[0], window[1], gate, 10, 65535, 6, 0.1, int(cull))
    _same((po, st), want, name)
    x = ds.meshes.vertices.astype(np.float64) * (ds.model_scale / 10000.0)
    ident = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)[None]
    diam = icp.diameter(x)
    mssd = lambda p, g: math.sqrt(pe.item_maxima(x, p, icp.normalised(g), ident, ds.proj_mat, *ds.image_dims)[0][0]) / diam
    before, after = [mssd(icp.normalised(s), g) for s, g in zip(start, gt)], [mssd(p, g) for p, g in zip(po, gt)]
    print(name, "pairs", st[:, 6].tolist(), "->", st[:, 7].tolist(), "MSSD / diameter", ["%.2e" % e for e in before], "->", ["%.2e" % e for e in after])
    assert (st[:, 0] == cn.OK).all() and (st[:, 5] == 10).all() and all(a < b for a, b in zip(after, before))
    if name == "box":
        return
    # with a mask, and the defaults spelled out
    mask = torch.stack([f["mask"] for f in infos])
    mv = int(mask.cpu().numpy().max())
    items[:, 4], items[:, 5] = frame, mv
    po, st = ref.refine(*dev, iters=2, gate=gate, edge_step=500, reach=3, contour_scale=1.0, mask=mask, mask_value=mv, cull=cull)
    _same((po.cpu().numpy(), st.cpu().numpy()),
          cn.contour_np(ds.meshes.vertices, ds.meshes.triangles, ds.meshes.tri_begin, np.array([ds.model_scale]), ds.proj_mat, depth.cpu().numpy(),
                        ds.udp.ray_map, mask.cpu().numpy(), items, start, 10000.0, window[0], window[1], gate, 2, 500, 3, 1.0, int(cull)), "mask")
    launched = ref._scratch.data_ptr()
    base = dict(depth=depth, pose=dev[1], frame=dev[2], obj=dev[3], corner=dev[4], window=window)
    for change in (dict(depth=depth.cpu()), dict(depth=depth.to(torch.int32)), dict(pose=base["pose"].float()), dict(pose=base["pose"][:, :6]),
                   dict(frame=dev[2][:3]), dict(obj=dev[3].float()), dict(corner=dev[4][:, :1]), dict(mask=mask[:, :-1]), dict(mask=mask.cpu())):
        with pytest.raises(RuntimeError, match="pose_refine_contour"):
            ref.refine(**dict(base, **change))
    for change in (dict(iters=-1), dict(iters=65), dict(gate=-1), dict(gate=65536), dict(window=(0, 4)), dict(window=(1 << 15, (1 << 15) + 1)),
                   dict(mask_frame=dev[2]), dict(edge_step=-1), dict(edge_step=65536), dict(reach=-1), dict(reach=65), dict(contour_scale=-1.0),
                   dict(contour_scale=float("nan")), dict(contour_scale=float("inf"))):
        with pytest.raises(ValueError, match="pose_refine_contour"):
            ref.refine(**dict(base, **change))
    assert ref._scratch.data_ptr() == launched
    assert 0 < ref.scratch_bytes(n, window) <= ref._scratch.numel()
    bare = prc.ContourPoseRefiner(ds.meshes, ds.model_scale, ds.proj_mat, ds.image_dims)
    with pytest.raises(ValueError, match="ray map"):
        bare.refine(**base)
    np.random.seed(1)
    with pytest.raises(ValueError, match="keep_frames"):
        RenderedPoseDataset(model, 500, False, 0.0, False, **kw).contour_refiner()
    cloud_ds = RenderedPoseDataset((np.random.default_rng(0).normal(size=(2000, 3)).astype(np.float32) * 30, None, np.full((2000, 3), 130, dtype=np.uint8)),
                                   500, False, 0.0, False, proj_mat=fab.PROJ[1], image_dims=(64, 96), frames=4)
    with pytest.raises(ValueError, match="triangles"):
        cloud_ds.contour_refiner()
