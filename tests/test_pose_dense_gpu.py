"""GPU: ``df_pose_refine_dense`` against its restatement (tests/pose_dense_np.py) bit for bit in ``pose_out`` and all six stats columns, its
refusals, D3's point against ``df_preprocess_objects_cad``'s cloud, the wrapper ``lib.pose_refine_dense.DensePoseRefiner`` and
``RenderedPoseDataset.dense_refiner()``.

Frames are 24 x 32, six of them, five objects of 1, 63, 64, 65 and 257 triangles (``pose_dense_np.make_scene``); the one-triangle object
is the flat wall.  The accumulation cuts a window's slots into tiles of 2048, a tile into 8 sweeps of 256 lanes and 4 waves of 64, and one
item is given 64 tile blocks at most: the windows stand one slot below, at and above each of these."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import fabricate_cad as fab
import mesh_closest_np as m
import mesh_icp_np as icp
import pose_dense_np as dn
import pose_verify_np as pv

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _up(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


class Call:
    """One ``df_pose_refine_dense`` call on a scene with every argument open to a test: ``run(**changes)`` -> (rc, pose_out, stats)."""

    def __init__(self, sc, items, pose, WH, WW, gate, iters, cull=0, mask=True, cloud_div=dn.CLOUD_DIV):
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
                      B=len(items), WH=WH, WW=WW, gate=gate, cull=cull, iters=iters)

    def run(self, short_scratch=0, misalign=0, null=(), alias=None, out_misalign=(), **changes):
        a = dict(self.a, **changes)
        B = len(self.items)
        need = max(self.L.df_pose_refine_dense_scratch_bytes(B, self.a["WH"], self.a["WW"]), 8)
        pose_out = torch.full((B * 7 + 1,), np.nan, dtype=torch.float64, device="cuda").view(torch.uint8).fill_(SENTINEL).view(torch.float64)
        stats = torch.empty(B * 6 + 1, dtype=torch.float64, device="cuda").view(torch.uint8).fill_(SENTINEL).view(torch.float64)
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
        rc = self.L.df_pose_refine_dense(a["vertices"], a["V"], a["triangles"], a["T"], a["tri_begin"], a["model_scale"], a["O"], a["proj"],
                                         a["depth"], a["F"], a["IH"], a["IW"], a["rays"], a["mask"], a["NM"], a["items"], a["pose_in"],
                                         ctypes.c_double(a["cloud_div"]), a["B"], a["WH"], a["WW"], a["gate"], a["cull"], a["iters"],
                                         ptr["pose_out"], ptr["stats"], ptr["scratch"], need - short_scratch, self.lib.current_stream())
        torch.cuda.synchronize()
        self.last_scratch = scratch
        return rc, pose_out.cpu().numpy()[:B * 7].reshape(B, 7), stats.cpu().numpy()[:B * 6].reshape(B, 6)


def _device(sc, items, pose, WH, WW, gate, iters, cull=0, mask=True):
    call = Call(sc, items, pose, WH, WW, gate, iters, cull, mask)
    rc, po, st = call.run()
    assert rc == 0, call.L.df_last_error()
    return po, st


def _want(sc, items, pose, WH, WW, gate, iters, cull=0, mask=True, trace=None):
    return dn.dense_np(sc["vertices"], sc["triangles"], sc["tri_begin"], sc["model_scale"], sc["proj"], sc["depth"], sc["rays"],
                       sc["mask"] if mask else None, items, pose, dn.CLOUD_DIV, WH, WW, gate, iters, cull, trace)


def _same(got, want, name):
    for what, g, w in (("pose_out", got[0], want[0]), ("stats", got[1], want[1])):
        bad = np.where((g.view(np.uint64) != w.view(np.uint64)).any(axis=1))[0]
        assert g.dtype == np.float64 and len(bad) == 0, f"{name}: {what} differs in rows {bad.tolist()}\n{g[bad][:3]}\n{w[bad][:3]}\nstats\n{want[1][bad][:3]}"


@pytest.fixture(scope="module")
def scene():
    _dev()
    return dn.make_scene()


# (WH, WW, r0, c0): 1 x 1, 1 x 65 over the wave's 64 lanes, 3 x 3; 255 / 256 / 257 slots (a sweep of the 256 lanes); 2047 / 2048 / 2049
# slots (a tile) and two tiles with inliers in both; 131072 / 131076 slots (64 tiles, one per tile block, and 65: block 0 takes two)
WINDOWS = ((1, 1, 12, 8), (1, 65, 12, -35), (3, 3, 11, 7), (15, 17, 5, 8), (16, 16, 4, 8), (1, 257, 12, -227), (257, 1, -238, 8),
           (23, 89, 0, -40), (32, 64, -4, -16), (683, 3, -671, 26), (24, 100, 0, 0), (24, 100, 0, -68), (4, 32768, 10, -32740),
           (4, 32769, 10, -32740))


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "%dx%d" % w[:2])
def test_windows_at_every_tile_and_sweep_boundary(scene, window):
    """Object 3 fills most of the frame, so wherever the window's existing nodes lie there are inliers: the trace of the restatement
    says in which tiles, and the two-tile windows must have them on both sides of the boundary."""
    WH, WW, r0, c0 = window
    items, pose = dn.make_call([3], WH, WW, 11, corner=(r0, c0))
    trace = []
    want = _want(scene, items, pose, WH, WW, dn.GATE, 2, trace=trace)
    slots = np.where(trace[0][0][1])[0]
    tiles = sorted(set((slots // dn.TILE).tolist()))
    print(window, "stats", want[1][0].tolist(), "inlier slots", len(slots), "tiles", tiles)
    if (WH, WW) in ((24, 100), (683, 3), (4, 32769), (4, 32768)):
        assert len(tiles) >= 2, "inliers on both sides of a tile boundary"
    if (WH, WW) == (4, 32769):
        assert tiles[-1] == dn.MAX_TILE_BLOCKS, "the 65th tile, which tile block 0 takes in its second round, holds inliers"
    if (WH, WW) in ((1, 257), (257, 1)):
        assert slots.max() == 256 and slots.min() < 256, "the 257th slot is lane 0's second sweep"
    if (WH, WW) == (1, 65):
        assert slots.max() == 64 and slots.min() < 64, "the 65th slot is the second wave's first lane"
    if (WH, WW) == (1, 1):
        assert len(slots) == 1 and want[1][0, 0] == dn.FEW
    _same(_device(scene, items, pose, WH, WW, dn.GATE, 2), want, str(window))


def test_window_positions(scene):
    """9 x 13 windows at the frame's origin, inside, over each edge and each vertex of the frame, and wholly outside: one call."""
    cs = dn.corners(9, 13)
    rng = np.random.default_rng(5)
    items = np.array([[3, 3, r0, c0, 3, 7] for r0, c0 in cs], dtype=np.int32)
    pose = dn.start_poses([3] * len(cs), rng)
    want = _want(scene, items, pose, 9, 13, dn.GATE, 2)
    print(want[1])
    outside = [b for b, (r0, c0) in enumerate(cs) if r0 >= dn.IH or c0 >= dn.IW or r0 + 9 <= 0 or c0 + 13 <= 0]
    assert len(outside) == 4 and (want[1][outside, 0] == dn.FEW).all() and not want[1][outside, 1:].any(), "wholly outside: few inliers"
    assert (want[1][:3, 0] == dn.OK).all() and (want[1][:6, 1] > 0).all(), "at the origin, inside and over each edge there are inliers"
    _same(_device(scene, items, pose, 9, 13, dn.GATE, 2), want, "positions")


@pytest.mark.parametrize("iters", (0, 1, 4))
@pytest.mark.parametrize("mask", (False, True))
@pytest.mark.parametrize("cull", (0, 1))
def test_meshes_iterations_mask_and_cull(scene, iters, mask, cull):
    """B = 5: the meshes of 1 (the flat wall: degenerate), 63, 64, 65 and 257 triangles, each on its own frame, whole-frame windows."""
    items, pose = dn.make_call([0, 1, 2, 3, 4], dn.IH, dn.IW, 3)
    want = _want(scene, items, pose, dn.IH, dn.IW, dn.GATE, iters, cull, mask)
    print(iters, mask, cull, want[1])
    if iters:
        ok = [1, 4] if cull else [1, 3, 4]                       # culled, the open 65-triangle shell shows too little of itself
        assert want[1][0, 0] == dn.DEGENERATE and want[1][0, 5] == 0 and (want[1][ok, 0] == dn.OK).all()
        assert (want[1][ok, 5] == iters).all() and (want[1][ok, 4] < want[1][ok, 2]).all()
        assert m.same_bits(want[0][0], icp.normalised(pose[0])), "the degenerate item keeps its pose"
    else:
        assert not want[1][:, 0].any() and not want[1][:, 5].any() and m.same_bits(want[1][:, 1:3], want[1][:, 3:5])
        assert m.same_bits(want[0], np.stack([icp.normalised(p) for p in pose])), "iters = 0 only scores"
    _same(_device(scene, items, pose, dn.IH, dn.IW, dn.GATE, iters, cull, mask), want, f"iters {iters} mask {mask} cull {cull}")


def test_one_item_and_five_on_three_objects(scene):
    for objs in ([4], [1, 3, 4, 3, 1]):
        items, pose = dn.make_call(objs, 17, 21, 7)
        _same(_device(scene, items, pose, 17, 21, dn.GATE, 4), _want(scene, items, pose, 17, 21, dn.GATE, 4), str(objs))


def test_mask_changes_the_inliers(scene):
    items, pose = dn.make_call([3, 4], dn.IH, dn.IW, 8)
    with_mask, without = _want(scene, items, pose, dn.IH, dn.IW, dn.GATE, 0), _want(scene, items, pose, dn.IH, dn.IW, dn.GATE, 0, mask=False)
    assert (with_mask[1][:, 1] < without[1][:, 1]).all() and (with_mask[1][:, 1] > 0).all()
    items[1, 4:6] = (5, 0)                                        # another mask frame and value
    _same(_device(scene, items, pose, dn.IH, dn.IW, dn.GATE, 2), _want(scene, items, pose, dn.IH, dn.IW, dn.GATE, 2), "mask frame and value")


@pytest.mark.parametrize("delta", (0, 1))
def test_gate_boundary(scene, delta):
    """The observed frame is the restatement's own rendered codes plus (-g-1, -g, 0, g, g+1) cycling with (r + q) % 5: with gate g the
    nodes of the three middle classes are the candidates, with gate g - 1 only those of offset 0."""
    g = 40
    items, pose = np.array([[3, 3, 0, 0, 0, 0]], dtype=np.int32), dn.TRUE_POSES[3:4]
    codes, _ = dn.render_codes(scene["vertices"], scene["triangles"], int(scene["tri_begin"][3]), int(scene["tri_begin"][4]), dn.SCALES[3],
                               scene["proj"], icp.normalised(dn.TRUE_POSES[3]), dn.CLOUD_DIV, dn.IH, dn.IW)
    r, q = np.mgrid[0:dn.IH, 0:dn.IW]
    obs = np.where(codes != 65535, codes + np.array([-g - 1, -g, 0, g, g + 1])[(r + q) % 5], 65535)
    sc = dict(scene)
    depth = scene["depth"].copy()
    depth[3] = obs
    sc["depth"] = depth
    trace = []
    want = _want(sc, items, pose, dn.IH, dn.IW, g - delta, 1, mask=False, trace=trace)
    drawn = codes != 65535
    n = [int((drawn & ((r + q) % 5 == k)).sum()) for k in range(5)]
    assert min(n) > 0 and int(trace[0][0][2].sum()) == (n[1] + n[2] + n[3] if delta == 0 else n[2])
    _same(_device(sc, items, pose, dn.IH, dn.IW, g - delta, 1, mask=False), want, f"gate {g - delta}")


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
    assert want[1][:, 0].tolist() == [0, 3, 3, 0, 3, 3, 0, 3, 3, 1, 1, 1] and not want[1][[1, 2, 4, 5, 7, 8], 1:].any()
    assert not want[1][[9, 10, 11], 1:].any() and np.isnan(want[0][9, :4]).all() and np.isnan(want[0][10, :4]).all()
    got = _device(scene, items, pose, 19, 23, dn.GATE, 3)
    _same(got, want, "bad items and poses")
    clean = _device(scene, good, pose, 19, 23, dn.GATE, 3)
    for b in (0, 3, 6):
        assert m.same_bits(got[0][b], clean[0][b]) and m.same_bits(got[1][b], clean[1][b]), "the neighbours of a bad item are unchanged"
    want = _want(scene, items, pose, 19, 23, dn.GATE, 3, mask=False)                  # without a mask the mask frame is not looked at
    assert want[1][:, 0].tolist() == [0, 3, 3, 0, 3, 3, 0, 0, 0, 1, 1, 1]
    _same(_device(scene, items, pose, 19, 23, dn.GATE, 3, mask=False), want, "bad items, no mask")


def _verify(call, sc, items, pose, WH, WW):
    B = len(items)
    L = call.L
    stats = torch.zeros(B, 12, dtype=torch.int64, device="cuda")
    scratch = torch.empty(L.df_pose_verify_scratch_bytes(B, WH, WW), dtype=torch.uint8, device="cuda")
    a = call.a
    rc = L.df_pose_verify(a["vertices"], a["V"], a["triangles"], a["T"], a["tri_begin"], a["model_scale"], a["O"], a["proj"], a["depth"], a["F"],
                          a["IH"], a["IW"], a["mask"], a["NM"], a["items"], a["pose_in"], ctypes.c_double(a["cloud_div"]), B, WH, WW, 8, 0,
                          stats.data_ptr(), scratch.data_ptr(), scratch.numel(), call.lib.current_stream())
    assert rc == 0
    return stats.cpu().numpy()


def test_determinism_independence_and_the_verifier_unchanged(scene):
    objs = [1, 3, 4, 0, 2]
    items, pose = dn.make_call(objs, 17, 37, 9)
    call = Call(scene, items, pose, 17, 37, dn.GATE, 3)
    before = _verify(call, scene, items, pose, 17, 37)
    assert m.same_bits(before, pv.verify_np(scene["vertices"], scene["triangles"], scene["tri_begin"], scene["model_scale"], scene["proj"],
                                            scene["depth"], scene["mask"], items, pose, dn.CLOUD_DIV, 17, 37, 8))
    (rc1, p1, s1), (rc2, p2, s2) = call.run(), call.run()
    assert rc1 == rc2 == 0 and p1.tobytes() == p2.tobytes() and s1.tobytes() == s2.tobytes(), "two identical calls give identical bytes"
    assert _verify(call, scene, items, pose, 17, 37).tobytes() == before.tobytes(), "df_pose_verify gives the same bytes before and after"
    order = [4, 2, 0, 3, 1]
    po, so = _device(scene, items[order], pose[order], 17, 37, dn.GATE, 3)
    assert po.tobytes() == p1[order].tobytes() and so.tobytes() == s1[order].tobytes(), "the same items reordered"
    for b in range(5):
        pb, sb = _device(scene, items[b:b + 1], pose[b:b + 1], 17, 37, dn.GATE, 3)
        assert pb.tobytes() == p1[b:b + 1].tobytes() and sb.tobytes() == s1[b:b + 1].tobytes(), f"item {b} alone equals its row of the call"


def test_argument_errors_touch_nothing(scene):
    items, pose = dn.make_call([1, 3, 4], 16, 16, 11)
    call = Call(scene, items, pose, 16, 16, dn.GATE, 2)
    L = call.L
    slots_bytes = 3 * 256 * 8
    assert L.df_pose_refine_dense_scratch_bytes(3, 16, 16) == slots_bytes + 3 * (12 + 7 + 16 + 32) * 8
    assert L.df_pose_refine_dense_scratch_bytes(1, 1, 2049) == 2049 * 8 + (12 + 7 + 16 + 2 * 32) * 8
    assert L.df_pose_refine_dense_scratch_bytes(0, 16, 16) == 0 and L.df_pose_refine_dense_scratch_bytes(65536, 1, 1) == 0
    assert L.df_pose_refine_dense_scratch_bytes(1, 0, 5) == 0 and L.df_pose_refine_dense_scratch_bytes(1, 1 << 15, (1 << 15) + 1) == 0
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
           dict(alias="pose_out=scratch"), dict(alias="stats=depth"), dict(alias="pose_out=rays")]
    inputs = [t.clone() for t in (call.pose, call.depth, call.rays)]
    for change in bad:
        rc, po, st = call.run(**change)
        assert rc == -1 and L.df_last_error(), f"{change}: DF_ERR_ARG expected, got {rc}"
        assert (po.view(np.uint8) == SENTINEL).all() and (st.view(np.uint8) == SENTINEL).all(), f"{change}: the call wrote before it refused"
        assert (call.last_scratch == SENTINEL).all(), f"{change}: the call wrote to the scratch before it refused"
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(inputs, (call.pose, call.depth, call.rays)))
    rc, po, st = call.run()
    assert rc == 0
    _same((po, st), _want(scene, items, pose, 16, 16, dn.GATE, 2), "after the refusals")


def test_observed_point_against_the_loaders_cloud(scene):
    """D3: for every chosen pixel of ``df_preprocess_objects_cad`` on frame 3 (label = the mask frame), the restated point p =
    (ray z(co)) / cloud_div agrees with the fp32 cloud point to fp32 rounding.  The cloud rounds ray z to fp32 and divides in fp32: two
    roundings of relative size 2^-24 each on top of the fp64 value, so |cloud - p| <= 2^-23 |p| (+ the fp64 error, far below)."""
    from densefusion_amd.lib import preprocess as pp
    depth, label = _up(scene["depth"], np.uint16), _up(scene["mask"], np.uint16)
    F = len(scene["depth"])
    rgb = torch.zeros(F, dn.IH, dn.IW, 3, dtype=torch.uint8, device="cuda")
    stats = pp.cad_frame_stats(depth, label, 7)
    P = scene["proj"]
    N = 64
    _, cloud, choose, count = pp.preprocess_objects_cad(rgb, depth, label, [(3, 7, (0, dn.IH, 0, dn.IW), 123)], N, stats, _up(scene["rays"], np.float64),
                                                        P[2, 2], P[2, 3], cloud_div=dn.CLOUD_DIV)
    assert int(count[0]) >= N
    idx = choose.cpu().numpy()[0, 0]
    r, q = idx // dn.IW, idx % dn.IW
    co = scene["depth"][3][r, q].astype(np.int64)
    p = dn.observed_points(co, scene["rays"][r, q], P[2, 2], P[2, 3], dn.CLOUD_DIV)
    got = cloud.cpu().numpy()[0].astype(np.float64)
    err = np.abs(got - p)
    print("largest |cloud - p| / |p|:", float((err / np.abs(p)).max()))
    assert (co != 65535).all() and (p[:, 2] < 0).all() and (err <= 2.0 ** -23 * np.abs(p)).all()


def _third_face_cosine(pose):
    """the selection rule of test_mesh_icp_gpu.test_icp_on_rendered_views: > 0 when three faces of the box show (fewer do not hold six
    degrees of freedom: such a view is `degenerate` by the contract)"""
    normals = np.array([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]], dtype=np.float64)
    centres = normals * np.array([15.0, 30.0, 45.0])
    o = -pose[:, :3].T @ pose[:, 3] / 10.0
    return sorted(float(n @ (o - c)) / float(np.linalg.norm(o - c)) for n, c in zip(normals, centres))[-3]


def test_wrapper_and_dense_refiner_on_rendered_views():
    """Eight rendered views of the bracket that show three faces of its box (the dataset keeps its frames).  From the true poses the status is 0 and the pose moves as
    little as the restatement says; from starts a few degrees and millimetres off the result equals the restatement's; argument errors
    come before any launch; without ``keep_frames`` and in point-cloud mode ``dense_refiner()`` raises, and ``refine`` raises without rays."""
    _dev()
    tool_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tool_dir)
    try:
        import importlib
        tool = importlib.import_module("eval_cad_render")
    finally:
        sys.path.pop(0)
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    from densefusion_amd.lib import pose_refine_dense as prd
    v, t = m.bracket()
    model = (v * np.float32(30.0), t, np.random.default_rng(5).integers(0, 256, (len(v), 3), dtype=np.uint8))
    kw = dict(raster="mesh", proj_mat=fab.PROJ[1], chunk=16, first_seed=0, frames=128, max_holes=1, image_dims=(64, 96), min_pixels=60)
    np.random.seed(1)
    ds = RenderedPoseDataset(model, 500, False, 0.0, False, keep_frames=True, **kw)
    live = [i for i in range(128) if ds.view_info(i)["live"] and _third_face_cosine(ds.view_info(i)["pose"]) >= 0.15][:8]
    assert len(live) == 8
    ref = ds.dense_refiner()
    assert isinstance(ref, prd.DensePoseRefiner) and ref.rays is not None and tuple(prd.STATS) == ("status", "first_inliers", "first_rms",
                                                                                                    "last_inliers", "last_rms", "steps")
    infos = [ds.view_info(i) for i in live]
    depth = torch.stack([f["depth"] for f in infos])
    mask = torch.stack([f["mask"] for f in infos])
    gt = np.stack([tool.true_pose(ds, i) for i in live])
    rng = np.random.default_rng(9)
    start = gt + np.concatenate([rng.normal(scale=0.02, size=(8, 4)), rng.normal(scale=0.0003, size=(8, 3))], axis=1)
    margin = 8
    window = (max(f["box"][1] - f["box"][0] for f in infos) + 2 * margin, max(f["box"][3] - f["box"][2] for f in infos) + 2 * margin)
    corner = np.array([[f["box"][0] - margin, f["box"][2] - margin] for f in infos])
    frame, obj = np.arange(8), np.zeros(8, dtype=np.int64)
    items = np.concatenate([frame[:, None], obj[:, None], corner, np.zeros((8, 2), dtype=np.int64)], axis=1)
    gate = 400
    common = (ds.meshes.vertices, ds.meshes.triangles, ds.meshes.tri_begin, np.array([ds.model_scale]), ds.proj_mat, depth.cpu().numpy(), ds.udp.ray_map)
    dev = (depth, None, _up(frame, np.int64), _up(obj, np.int64), _up(corner, np.int64), window)
    for name, est in (("true", gt), ("start", start)):
        po, st = ref.refine(dev[0], _up(est, np.float64), *dev[2:], iters=3, gate=gate, cull=bool(ds.cull))
        assert po.is_cuda and st.is_cuda and po.dtype == st.dtype == torch.float64
        want = dn.dense_np(*common, None, items, est, 10000.0, window[0], window[1], gate, 3, int(bool(ds.cull)))
        print(name, want[1])
        _same((po.cpu().numpy(), st.cpu().numpy()), want, name)
        if name == "true":
            moved = np.abs(po.cpu().numpy() - np.stack([icp.normalised(p) for p in gt])).max(axis=1)
            assert (st.cpu().numpy()[:, 0] == 0).all() and (moved <= np.abs(want[0] - np.stack([icp.normalised(p) for p in gt])).max(axis=1)).all()
    # with the items' masks: mask frame = frame, the value of the kept masks
    mv = int(mask.cpu().numpy().max())
    items[:, 4], items[:, 5] = frame, mv
    po, st = ref.refine(depth, _up(start, np.float64), *dev[2:], iters=2, gate=gate, mask=mask, mask_value=mv, cull=bool(ds.cull))
    _same((po.cpu().numpy(), st.cpu().numpy()),
          dn.dense_np(*common, mask.cpu().numpy(), items, start, 10000.0, window[0], window[1], gate, 2, int(bool(ds.cull))), "mask")
    launched = ref._scratch.data_ptr()
    base = dict(depth=depth, pose=_up(gt, np.float64), frame=dev[2], obj=dev[3], corner=dev[4], window=window)
    for change in (dict(depth=depth.cpu()), dict(depth=depth.to(torch.int32)), dict(pose=base["pose"].float()), dict(pose=base["pose"][:, :6]),
                   dict(frame=dev[2][:3]), dict(obj=dev[3].float()), dict(corner=dev[4][:, :1]), dict(mask=mask[:, :-1]), dict(mask=mask.cpu())):
        with pytest.raises(RuntimeError, match="pose_refine_dense"):
            ref.refine(**dict(base, **change))
    for change in (dict(iters=-1), dict(iters=65), dict(gate=-1), dict(gate=65536), dict(window=(0, 4)), dict(window=(1 << 15, (1 << 15) + 1)),
                   dict(mask_frame=dev[2])):
        with pytest.raises(ValueError, match="pose_refine_dense"):
            ref.refine(**dict(base, **change))
    assert ref._scratch.data_ptr() == launched
    bare = prd.DensePoseRefiner(ds.meshes, ds.model_scale, ds.proj_mat, ds.image_dims)
    with pytest.raises(ValueError, match="ray map"):
        bare.refine(**base)
    np.random.seed(1)
    with pytest.raises(ValueError, match="keep_frames"):
        RenderedPoseDataset(model, 500, False, 0.0, False, **kw).dense_refiner()
    cloud_ds = RenderedPoseDataset((np.random.default_rng(0).normal(size=(2000, 3)).astype(np.float32) * 30, None, np.full((2000, 3), 130, dtype=np.uint8)),
                                   500, False, 0.0, False, proj_mat=fab.PROJ[1], image_dims=(64, 96), frames=4)
    with pytest.raises(ValueError, match="triangles"):
        cloud_ds.dense_refiner()
