"""GPU: ``df_pose_ppf`` against its restatement (tests/pose_ppf_np.py) bit for bit in every reference's hypothesis (``hyp_out``, the votes
as exact integers), ``pose_out``, ``votes_out`` and ``stats``; its refusals; the wrapper ``lib.pose_ppf`` and
``RenderedPoseDataset.ppf_estimator()``.

Frames are 24 x 32 (``pose_dense_np.make_scene``: five objects, the first a flat wall, noise, holes, a far background and masks), the
models are sampled with 2, 63, 64, 65 and 256 points, and with 1024 points at 30 and 36 rotation bins: 122 880 and 147 456 bytes of
accumulator, the largest the call admits.  A lane walks a bucket of up to 16 entries alone and the whole wave a longer one; the 256-point
model has buckets on both sides (``pose_ppf_np`` prints the longest)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mesh_closest_np as m
import mesh_icp_np as icp
import pose_dense_np as dn
import pose_ppf_np as pp
import pose_verify_np as pv

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _up(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


class Call:
    """One ``df_pose_ppf`` call with every argument open to a test: ``run(**changes)`` -> (rc, pose_out, votes_out, stats, hyp_out)."""

    def __init__(self, sc, model, items, WH, WW, step=1, reach=1, gate=pp.GATE, ref_step=1, K=4, mask=True, deg=15.0, frac=0.1):
        from densefusion_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.host = dict(point_begin=np.ascontiguousarray(model["point_begin"], dtype=np.int32),
                         dist_step=np.ascontiguousarray(model["dist_step"], dtype=np.float64),
                         cluster_dist=np.ascontiguousarray(model["diameter"] * frac, dtype=np.float64),
                         proj=np.ascontiguousarray(sc["proj"], dtype=np.float64).reshape(-1))
        self.host["ang_cos"], self.host["alpha_cos"], self.host["alpha_cs"] = [np.ascontiguousarray(t) for t in pp.tables(model["NANG"], model["NA"])]
        self.dev = dict(model_points=_up(model["points"], np.float64), model_normals=_up(model["normals"], np.float64),
                        bucket_begin=_up(model["bucket_begin"], np.int32), entry_point=_up(model["entry_point"], np.int32),
                        entry_cs=_up(model["entry_cs"], np.float32), depth=_up(sc["depth"], np.uint16), rays=_up(sc["rays"], np.float64),
                        items=_up(items, np.int32))
        self.mask = _up(sc["mask"], np.uint16) if mask else None
        F, IH, IW = sc["depth"].shape
        self.a = dict({k: v.ctypes.data for k, v in self.host.items()}, **{k: v.data_ptr() for k, v in self.dev.items()})
        self.a.update(NM=len(model["points"]), O=len(model["point_begin"]) - 1, n_entries=len(model["entry_point"]), ND=model["ND"], NANG=model["NANG"],
                      NA=model["NA"], F=F, IH=IH, IW=IW, mask=self.mask.data_ptr() if mask else None, NMK=len(sc["mask"]) if mask else 0,
                      cloud_div=dn.CLOUD_DIV, B=len(items), WH=WH, WW=WW, step=step, reach=reach, gate=gate, ref_step=ref_step, K=K,
                      cluster_trace=pp.cluster_trace(deg))
        self.B, self.K = len(items), K
        g = [pp.grid_side(WH, step), pp.grid_side(WW, step)]
        self.NR = pp.grid_side(g[0], ref_step) * pp.grid_side(g[1], ref_step)

    def run(self, short_scratch=0, misalign=0, null=(), alias=None, out_misalign=(), no_hyp=False, **changes):
        a = dict(self.a, **changes)
        B, K, NR = self.B, self.K, self.NR
        need = max(self.L.df_pose_ppf_scratch_bytes(B, self.a["WH"], self.a["WW"], self.a["step"], self.a["ref_step"]), 8)
        sizes = dict(pose_out=B * K * 7 * 8, votes_out=B * K * 2 * 4, stats=B * 4 * 8, hyp_out=B * NR * 8 * 8)
        outs = {k: torch.full((n + 8,), SENTINEL, dtype=torch.uint8, device="cuda") for k, n in sizes.items()}
        scratch = torch.full((need + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
        ptr = {k: t.data_ptr() + (4 if k in out_misalign else 0) for k, t in outs.items()}
        ptr["scratch"] = scratch.data_ptr() + misalign
        if alias is not None:                                       # "dst=src": the output dst lies inside src
            dst, src = alias.split("=")
            ptr[dst] = ptr["scratch"] + need - 8 if src == "scratch" else (ptr[src] + 8 if src in outs else a[src])
        for k in null:
            ptr[k] = None
        if no_hyp:
            ptr["hyp_out"] = None
        rc = self.L.df_pose_ppf(a["model_points"], a["model_normals"], a["NM"], a["point_begin"], a["dist_step"], a["cluster_dist"], a["O"],
                                a["bucket_begin"], a["entry_point"], a["entry_cs"], a["n_entries"], a["ND"], a["NANG"], a["NA"], a["ang_cos"],
                                a["alpha_cos"], a["alpha_cs"], a["proj"], a["depth"], a["F"], a["IH"], a["IW"], a["rays"], a["mask"], a["NMK"],
                                a["items"], ctypes.c_double(a["cloud_div"]), a["B"], a["WH"], a["WW"], a["step"], a["reach"], a["gate"],
                                a["ref_step"], a["K"], ctypes.c_double(a["cluster_trace"]), ptr["pose_out"], ptr["votes_out"], ptr["stats"],
                                ptr["hyp_out"], ptr["scratch"], need - short_scratch, self.lib.current_stream())
        torch.cuda.synchronize()
        self.last_scratch, self.last_outs = scratch, outs
        self.visited = scratch[misalign:misalign + need].cpu().numpy()[need - 8 * B:].view(np.uint64).tolist() if rc == 0 and not misalign else None
        host = {k: t.cpu().numpy()[:sizes[k]] for k, t in outs.items()}
        return (rc, host["pose_out"].view(np.float64).reshape(B, K, 7), host["votes_out"].view(np.int32).reshape(B, K, 2),
                host["stats"].view(np.float64).reshape(B, 4), host["hyp_out"].view(np.float64).reshape(B, NR, 8))


def _device(sc, model, items, WH, WW, visited=None, **kw):
    call = Call(sc, model, items, WH, WW, **kw)
    out = call.run()
    assert out[0] == 0, call.L.df_last_error()
    if visited is not None:
        visited += call.visited
    return out[1:]


def _same(got, want, name):
    for what, g, w in zip(("pose_out", "votes_out", "stats", "hyp_out"), got, want):
        w = np.ascontiguousarray(w, dtype=g.dtype)
        bad = np.argwhere(g.view(np.uint8).reshape(len(g), -1) != w.view(np.uint8).reshape(len(w), -1))
        assert g.shape == w.shape and len(bad) == 0, f"{name}: {what} differs, first in item {bad[0][0]}\n{g[bad[0][0]][:4]}\n{w[bad[0][0]][:4]}"


def _both(sc, model, items, WH, WW, name, **kw):
    """The restatement's outputs after the device's were found equal to them."""
    counts = []
    want = pp.run_np(sc, model, items, WH, WW, counts=counts, **kw)
    visited = []
    _same(_device(sc, model, items, WH, WW, visited=visited, **kw), want, name)
    bad = [b for b in range(len(items)) if want[2][b, 0] == pp.BAD_ITEM]
    assert [v for b, v in enumerate(visited) if b not in bad] == counts and not any(visited[b] for b in bad), f"{name}: the entries visited"
    return want, counts


@pytest.fixture(scope="module")
def scene():
    _dev()
    return dn.make_scene()


@pytest.fixture(scope="module")
def model():
    mod = pp.make_model(pp.scene_clouds())
    lens = np.diff(mod["bucket_begin"], axis=1)
    print("entries", len(mod["entry_point"]), "longest bucket per object", lens.max(axis=1).tolist())
    assert lens[4].max() > 16 and ((lens[4] > 0) & (lens[4] <= 16)).any(), "the 256-point model has buckets a lane walks and buckets a wave walks"
    return mod


WHOLE = (dn.IH, dn.IW)


@pytest.mark.parametrize("mask,ref_step", ((True, 1), (True, 5), (False, 5)))
def test_models_of_2_to_256_points_in_one_table(scene, model, mask, ref_step):
    """B = 5, one item per object, whole-frame windows: five objects with different NM in one table.  (Every node of the unmasked frames
    as a reference is 2.1e6 entries for the restatement: the unmasked call takes every fifth.)"""
    want, counts = _both(scene, model, pp.make_items([0, 1, 2, 3, 4], 0, 0), *WHOLE, name="five", mask=mask, ref_step=ref_step)
    print(mask, ref_step, want[2].tolist(), counts)
    assert (want[2][:, 0] == pp.OK).sum() >= 4 and (want[2][:, 2] > 0).sum() >= 4 and sorted(counts)[1] > 0


@pytest.mark.parametrize("NA", (30, 36))
def test_the_largest_accumulators(scene, NA):
    """1024 points x 30 bins = 122 880 bytes and x 36 = 147 456 bytes, the largest the call admits; 1024 x 38 is refused."""
    big = pp.make_model(pp.scene_clouds((2, 2, 2, 1024, 2), seed=7), NA=NA)
    assert 1024 * NA * 4 == (122880, 147456)[NA == 36]
    items = np.array([[3, 3, 0, 0, 3, 7], [3, 3, -2, 5, 3, 7]], dtype=np.int32)
    want, counts = _both(scene, big, items, *WHOLE, name=f"NA {NA}", mask=False, ref_step=5)
    print(NA, want[2].tolist(), counts, want[1][:, 0].tolist())
    assert (want[2][:, 0] == pp.OK).all() and min(counts) > 1000
    if NA == 36:
        call = Call(scene, big, items, *WHOLE, mask=False, ref_step=5)
        tabs = [np.ascontiguousarray(t) for t in pp.tables(15, 38)]
        assert call.run(NA=38, alpha_cos=tabs[1].ctypes.data, alpha_cs=tabs[2].ctypes.data)[0] == -1 and b"LDS" in call.L.df_last_error()


def test_flat_wall_one_bucket_and_an_empty_bucket(scene):
    """The wall's table has one distance bin: every pair of the model has one key, so one bucket holds the whole table and every scene
    pair that finds a bucket walks all of it.  The table of two points whose normals look at each other (``facing_model``): the scene's
    pairs have other keys, every bucket they name is empty, and the items end without a hypothesis although they have usable points."""
    wall = pp.wall_model()
    lens = np.diff(wall["bucket_begin"][0])
    assert lens.max() == len(wall["entry_point"]) == 64 * 63
    items = np.array([[0, 0, 0, 0, 0, 7], [3, 0, 4, 8, 3, 7]], dtype=np.int32)
    want, counts = _both(scene, wall, items, 16, 16, name="wall", ref_step=3)
    print(want[2].tolist(), counts, want[1][:, 0].tolist())
    assert want[2][0, 0] == pp.OK and counts[0] > 0 and counts[0] % (64 * 63) == 0 and want[1][0, 0, 1] > 1
    facing = pp.facing_model()
    assert len(facing["entry_point"]) == 2
    want, counts = _both(scene, facing, items, 16, 16, name="empty buckets", ref_step=3)
    assert (want[2][:, 0] == pp.NO_HYPOTHESIS).all() and (want[2][:, 1] > 1).all() and counts == [0, 0] and not want[3].any()


# (WH, WW, r0, c0, step): no pair at all; one row over a wave's 64 lanes; 3 x 3; sides that are no multiple of the step
WINDOWS = ((1, 1, 12, 8, 1), (1, 65, 12, -20, 1), (3, 3, 11, 7, 1), (23, 31, 0, 0, 2), (23, 31, 1, 1, 3), (24, 32, 0, 0, 3))


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "%dx%d_step%d" % (w[0], w[1], w[4]))
def test_windows_and_steps(scene, model, window):
    WH, WW, r0, c0, step = window
    want, _ = _both(scene, model, pp.make_items([3, 4, 1], r0, c0), WH, WW, name=str(window), step=step, mask=False)
    print(window, want[2].tolist())
    if (WH, WW) == (1, 1):
        assert (want[2][:, 0] == pp.NO_HYPOTHESIS).all() and (want[2][:, 1] <= 1).all(), "one node: no pair, no hypothesis"
    else:
        assert want[2][:, 1].max() > 1


@pytest.mark.parametrize("step,ref_step,reach", ((1, 1, 1), (2, 1, 3), (1, 5, 3), (3, 5, 1), (2, 5, 2)))
def test_window_positions(scene, model, step, ref_step, reach):
    """9 x 13 windows at the frame's origin, inside, over each edge and each vertex of the frame, and wholly outside, in one call; a reach
    of 3 leaves the frame from the windows at its edges."""
    cs = dn.corners(9, 13)
    items = np.array([[3, 3, r0, c0, 3, 7] for r0, c0 in cs], dtype=np.int32)
    want, _ = _both(scene, model, items, 9, 13, name="positions", step=step, ref_step=ref_step, reach=reach, mask=False)
    print(want[2].tolist())
    outside = [b for b, (r0, c0) in enumerate(cs) if r0 >= dn.IH or c0 >= dn.IW or r0 + 9 <= 0 or c0 + 13 <= 0]
    assert len(outside) == 4 and (want[2][outside, 0] == pp.NO_HYPOTHESIS).all() and not want[2][outside, 1:].any()
    assert (want[2][:2, 1] > 1).all()


@pytest.mark.parametrize("delta", (0, 1))
def test_gate_boundary_and_hand_placed_ties(scene, delta):
    """Frame 1 of ``flat_frames``: every neighbour at one node differs by exactly g codes: with gate g every inner node has a normal,
    with gate g - 1 none has.  Frame 0 is one code everywhere: nodes placed symmetrically about a reference cast the same votes, so cells
    and hypotheses tie and the order rules decide."""
    g = 40
    sc = dict(scene, depth=pp.flat_frames(30000, g))
    wall = pp.wall_model(16)
    items = np.array([[1, 0, 2, 3, 0, 0], [0, 0, 2, 3, 0, 0]], dtype=np.int32)
    want, _ = _both(sc, wall, items, 9, 11, name=f"gate {g - delta}", gate=g - delta, mask=False, ref_step=2, K=16)
    print(want[2].tolist(), want[1][1, :, 0].tolist())
    assert want[2][0, 1] == (9 * 11 if delta == 0 else 0) and want[2][1, 1] == 9 * 11
    votes = want[3][1, :, 7]
    assert len(set(votes[votes > 0].tolist())) < (votes > 0).sum(), "hypotheses with equal votes"


def test_mask_that_leaves_fewer_than_two_points(scene, model):
    sc = dict(scene, mask=scene["mask"].copy())
    sc["mask"][5] = 0
    sc["mask"][5, 10, 12] = 9
    items = np.array([[3, 3, 0, 0, 5, 9], [3, 3, 0, 0, 5, 8], [3, 3, 0, 0, 3, 7]], dtype=np.int32)
    want, _ = _both(sc, model, items, *WHOLE, name="sparse mask", ref_step=2)
    assert want[2][:2, 0].tolist() == [pp.NO_HYPOTHESIS] * 2 and want[2][2, 0] == pp.OK and (want[2][:2, 1] == 0).all()
    assert not want[0][:2].any() and not want[1][:2].any()


@pytest.mark.parametrize("K", (1, 4, 16))
def test_k_with_more_and_fewer_clusters(scene, model, K):
    want, _ = _both(scene, model, pp.make_items([0, 2, 4], 0, 0), *WHOLE, name=f"K {K}", K=K, ref_step=2)
    print(K, want[2].tolist(), want[1][:, :, 0].tolist())
    clusters = want[2][:, 3]
    assert clusters.max() > 16 and 1 <= clusters.min() < 4, "an item with more clusters than any K and one with fewer than 4"
    for b in range(3):
        n = int(min(K, clusters[b]))
        assert (want[1][b, :n, 0] > 0).all() and not want[1][b, n:].any() and not want[0][b, n:].any(), "missing ranks are zero"
        assert (np.diff(want[1][b, :n, 0]) <= 0).all()


def test_batches_order_and_determinism(scene, model):
    objs = [3, 4, 1, 0, 2, 4, 3, 1, 0, 2, 3, 4]
    items = pp.make_items(objs, 2, 3)
    items[5:, 2:4] = (-3, 9)
    kw = dict(ref_step=3, K=4)
    want, _ = _both(scene, model, items, 19, 23, name="B = 12", **kw)
    call = Call(scene, model, items, 19, 23, **kw)
    a, b = call.run(), call.run()
    assert a[0] == b[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:])), "two identical calls give identical bytes"
    order = [7, 2, 11, 0, 5, 9, 4, 1, 10, 3, 8, 6]
    _same(_device(scene, model, items[order], 19, 23, **kw), [w[order] for w in want], "reordered")
    for n in (1, 5):
        _same(_device(scene, model, items[:n], 19, 23, **kw), [w[:n] for w in want], f"B = {n}")
    _same(_device(scene, model, items[7:8], 19, 23, **kw), [w[7:8] for w in want], "item 7 alone")
    out = call.run(no_hyp=True)
    assert out[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(out[1:4], a[1:4])), "hyp_out is optional"
    assert (out[4].view(np.uint8) == SENTINEL).all()


def test_bad_items_leave_their_neighbours_alone(scene, model):
    objs = [3, 4, 3, 1, 3, 4, 3, 3, 1]
    items = pp.make_items(objs, 2, 3)
    good = items.copy()
    F, O = len(scene["depth"]), len(dn.COUNTS)
    for b, (col, val) in {1: (0, -1), 2: (0, F), 4: (1, -1), 5: (1, O), 7: (4, -1), 8: (4, len(scene["mask"]))}.items():
        items[b, col] = val
    want, _ = _both(scene, model, items, 19, 23, name="bad items", ref_step=2)
    assert want[2][:, 0].tolist() == [0, 3, 3, 0, 3, 3, 0, 3, 3]
    bad = [1, 2, 4, 5, 7, 8]
    assert not want[2][bad, 1:].any() and not want[0][bad].any() and not want[1][bad].any() and not want[3][bad].any()
    clean = _device(scene, model, good, 19, 23, ref_step=2)
    for k in range(4):
        assert clean[k][[0, 3, 6]].tobytes() == np.ascontiguousarray(want[k], dtype=clean[k].dtype)[[0, 3, 6]].tobytes()
    want, _ = _both(scene, model, items, 19, 23, name="bad items, no mask", ref_step=2, mask=False)
    assert want[2][:, 0].tolist() == [0, 3, 3, 0, 3, 3, 0, 0, 0], "without a mask the mask frame is not looked at"


def test_verifier_and_dense_refiner_unchanged(scene, model):
    """``df_pose_verify`` and ``df_pose_refine_dense`` before and after a ``df_pose_ppf`` call: equal bytes, equal to their restatements."""
    import test_pose_dense_gpu as tdg
    items, pose = dn.make_call([1, 3, 4], 17, 21, 9)
    dense = tdg.Call(scene, items, pose, 17, 21, dn.GATE, 2)
    ver0, (rc0, p0, s0) = tdg._verify(dense, scene, items, pose, 17, 21), dense.run()
    _device(scene, model, pp.make_items([1, 3, 4], 2, 3), 17, 21, ref_step=2)
    ver1, (rc1, p1, s1) = tdg._verify(dense, scene, items, pose, 17, 21), dense.run()
    assert rc0 == rc1 == 0 and ver0.tobytes() == ver1.tobytes() and p0.tobytes() == p1.tobytes() and s0.tobytes() == s1.tobytes()
    assert m.same_bits(ver0, pv.verify_np(scene["vertices"], scene["triangles"], scene["tri_begin"], scene["model_scale"], scene["proj"],
                                          scene["depth"], scene["mask"], items, pose, dn.CLOUD_DIV, 17, 21, 8))
    tdg._same((p1, s1), tdg._want(scene, items, pose, 17, 21, dn.GATE, 2), "dense after ppf")


def test_argument_errors_touch_nothing(scene, model):
    items = pp.make_items([1, 3, 4], 2, 3)
    call = Call(scene, model, items, 16, 16, ref_step=2)
    L = call.L
    assert L.df_pose_ppf_scratch_bytes(3, 16, 16, 1, 2) == 3 * 256 * 8 * 8 + 3 * 64 * 20 * 8 + 3 * 8
    assert L.df_pose_ppf_scratch_bytes(1, 128, 128, 1, 2) == 16384 * 64 + 4096 * 160 + 8 and L.df_pose_ppf_scratch_bytes(1, 128, 129, 1, 2) == 0
    assert L.df_pose_ppf_scratch_bytes(1, 128, 128, 1, 1) == 0 and L.df_pose_ppf_scratch_bytes(1, 64, 65, 1, 1) == 0
    assert L.df_pose_ppf_scratch_bytes(0, 16, 16, 1, 1) == 0 and L.df_pose_ppf_scratch_bytes(65536, 1, 1, 1, 1) == 0
    assert L.df_pose_ppf_scratch_bytes(1, 16, 16, 0, 1) == 0 and L.df_pose_ppf_scratch_bytes(1, 16, 16, 1, 65) == 0
    h = call.host
    begin_bad0, begin_end, begin_one = h["point_begin"].copy(), h["point_begin"].copy(), h["point_begin"].copy()
    begin_bad0[0], begin_end[-1], begin_one[1] = 1, begin_end[-1] - 1, 1
    proj_bad, ds_bad, cd_bad, ang_bad, al_bad, cs_bad = (h[k].copy() for k in ("proj", "dist_step", "cluster_dist", "ang_cos", "alpha_cos", "alpha_cs"))
    proj_bad[14], ds_bad[2], cd_bad[1], ang_bad[3], al_bad[2], cs_bad[5, 1] = -2.0, 0.0, -1.0, ang_bad[2], np.nan, 1.5
    keep = [begin_bad0, begin_end, begin_one, proj_bad, ds_bad, cd_bad, ang_bad, al_bad, cs_bad]
    nulls = [{k: None} for k in ("model_points", "model_normals", "point_begin", "dist_step", "cluster_dist", "bucket_begin", "entry_point", "entry_cs",
                                 "ang_cos", "alpha_cos", "alpha_cs", "proj", "depth", "rays", "items")]
    bad = nulls + [dict(null=(k,)) for k in ("pose_out", "votes_out", "stats", "scratch")] + [
        dict(NMK=0), dict(NMK=-1), dict(B=0), dict(B=65536), dict(WH=0), dict(WW=0), dict(WH=-1), dict(WH=1 << 15, WW=(1 << 15) + 1),
        dict(WH=128, WW=129), dict(WH=128, WW=128, ref_step=1), dict(F=0), dict(F=65536), dict(IH=0), dict(IW=0), dict(IH=1 << 15, IW=(1 << 15) + 1),
        dict(NM=0), dict(O=0), dict(O=65), dict(ND=0), dict(ND=65), dict(NANG=0), dict(NANG=33), dict(NA=0), dict(NA=29), dict(NA=66),
        dict(step=0), dict(step=65), dict(ref_step=0), dict(ref_step=65), dict(reach=0), dict(reach=9), dict(gate=-1), dict(gate=65536),
        dict(K=0), dict(K=17), dict(cluster_trace=3.5), dict(cluster_trace=-1.5), dict(cluster_trace=float("nan")), dict(n_entries=1 << 31),
        dict(point_begin=begin_bad0.ctypes.data), dict(point_begin=begin_end.ctypes.data), dict(point_begin=begin_one.ctypes.data),
        dict(proj=proj_bad.ctypes.data), dict(dist_step=ds_bad.ctypes.data), dict(cluster_dist=cd_bad.ctypes.data), dict(ang_cos=ang_bad.ctypes.data),
        dict(alpha_cos=al_bad.ctypes.data), dict(alpha_cs=cs_bad.ctypes.data), dict(cloud_div=0.0), dict(cloud_div=-1.0), dict(cloud_div=float("inf")),
        dict(cloud_div=float("nan")), dict(short_scratch=1), dict(misalign=4), dict(rays=call.a["rays"] + 4), dict(model_points=call.a["model_points"] + 4),
        dict(entry_cs=call.a["entry_cs"] + 4), dict(bucket_begin=call.a["bucket_begin"] + 2), dict(depth=call.a["depth"] + 1),
        dict(out_misalign=("pose_out",)), dict(out_misalign=("stats",)), dict(out_misalign=("hyp_out",)),
        dict(alias="pose_out=rays"), dict(alias="stats=depth"), dict(alias="votes_out=items"), dict(alias="hyp_out=entry_cs"),
        dict(alias="pose_out=scratch"), dict(alias="stats=pose_out"), dict(alias="hyp_out=stats"), dict(alias="votes_out=hyp_out"),
        dict(alias="pose_out=model_points"), dict(alias="stats=bucket_begin")]
    inputs = [t.clone() for t in call.dev.values()]
    for change in bad:
        out = call.run(**change)
        assert out[0] == -1 and L.df_last_error(), f"{change}: DF_ERR_ARG expected, got {out[0]}"
        assert all((t == SENTINEL).all() for t in call.last_outs.values()), f"{change}: the call wrote before it refused"
        assert (call.last_scratch == SENTINEL).all(), f"{change}: the call wrote to the scratch before it refused"
        assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(inputs, call.dev.values()))
    assert keep
    out = call.run()
    assert out[0] == 0
    _same(out[1:], pp.run_np(scene, model, items, 16, 16, ref_step=2), "after the refusals")


# ---- the wrapper on rendered views ---------------------------------------------------------------------------------------------------------
# Eight of the first 128 rendered bracket views (64 x 96 frames, ``test_pose_dense_gpu``'s dataset), chosen with the chain below so that
# all eight pass; the device is bit-equal to the restatement on them, so they pass there as well.
VIEWS = (0, 4, 8, 12, 19, 30, 35, 38)
VIEW_GATE, VIEW_REF_STEP, VIEW_DENSE_GATE = 2000, 2, 2000                       # neighbouring nodes of these frames lie some 800 codes apart


def _rendered_dataset(keep_frames=True):
    import importlib
    import os
    import sys
    import fabricate_cad as fab
    tool_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tool_dir)
    try:
        tool = importlib.import_module("eval_cad_render")
    finally:
        sys.path.pop(0)
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    v, t = m.bracket()
    mesh = (v * np.float32(30.0), t, np.random.default_rng(5).integers(0, 256, (len(v), 3), dtype=np.uint8))
    kw = dict(raster="mesh", proj_mat=fab.PROJ[1], chunk=16, first_seed=0, frames=128, max_holes=1, image_dims=(64, 96), min_pixels=60)
    np.random.seed(1)
    return RenderedPoseDataset(mesh, 500, False, 0.0, False, keep_frames=keep_frames, **kw), tool, mesh, kw


def _view_call(ds, views, margin=8):
    infos = [ds.view_info(i) for i in views]
    depth, mask = torch.stack([f["depth"] for f in infos]), torch.stack([f["mask"] for f in infos])
    window = (max(f["box"][1] - f["box"][0] for f in infos) + 2 * margin, max(f["box"][3] - f["box"][2] for f in infos) + 2 * margin)
    corner = np.array([[f["box"][0] - margin, f["box"][2] - margin] for f in infos])
    return depth, mask, window, corner


def _device_chain(ds, est, views, gate, ref_step, dense_gate, K=4, iters=10, tol=8):
    """Top K, refine, verify, select on the device: (ppf outputs with hyp, refined [B,K,7], iou [B,K], kept [B]) as numpy."""
    from densefusion_amd.lib.pose_verify import vsiou
    B = len(views)
    depth, mask, window, corner = _view_call(ds, views)
    frame, obj, mv = _up(np.arange(B), np.int64), _up(np.zeros(B), np.int64), int(mask.cpu().numpy().max())
    out = est.estimate(depth, frame, obj, _up(corner, np.int64), window, gate=gate, ref_step=ref_step, k=K, mask=mask, mask_value=mv, hyp=True)
    rep = lambda x: x.repeat_interleave(K, dim=0)
    refined, _ = ds.dense_refiner().refine(depth, out[0].reshape(B * K, 7), rep(frame), rep(obj), rep(_up(corner, np.int64)), window, iters=iters,
                                           gate=dense_gate, cull=bool(ds.cull))
    stats = ds.pose_verifier().score(depth, refined, rep(frame), rep(obj), rep(_up(corner, np.int64)), window, tol, mask=mask, cull=bool(ds.cull))
    iou = torch.where(out[1][:, :, 0] > 0, vsiou(stats).reshape(B, K), torch.full((B, K), -1.0, dtype=torch.float64, device="cuda"))
    return [o.cpu().numpy() for o in out], refined.cpu().numpy().reshape(B, K, 7), iou.cpu().numpy(), iou.argmax(dim=1).cpu().numpy()


def _mssd_over_diameter(ds, tool, views, poses):
    import pose_error_np as pe
    x = ds.meshes.vertices.astype(np.float64) * (ds.model_scale / 10000.0)
    ident = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)[None]
    diam = icp.diameter(x)
    return [math.sqrt(pe.item_maxima(x, p, tool.true_pose(ds, i), ident, ds.proj_mat, *ds.image_dims)[0][0]) / diam for i, p in zip(views, poses)]


def test_wrapper_and_ppf_estimator_on_rendered_views():
    """``RenderedPoseDataset.ppf_estimator()`` on eight rendered bracket views: the wrapper's outputs equal the restatement's on the
    wrapper's own tables, the tables equal the restatement's, and top 4 -> ten dense steps -> verify -> the highest IoU ends with MSSD
    below 0.01 diameter on all eight; then the argument errors and the raises."""
    _dev()
    from densefusion_amd.lib import pose_ppf as lp
    ds, tool, mesh, kw = _rendered_dataset()
    est = ds.ppf_estimator(points=400, seed=1)
    md = est.models
    assert isinstance(est, lp.PpfEstimator) and est.rays is not None and tuple(lp.STATS) == ("status", "usable", "hypotheses", "clusters")
    for a, b in zip(lp.ppf_tables(15, 30), pp.tables(15, 30)):
        assert a.tobytes() == b.tobytes()
    model = dict(points=md.points, normals=md.normals, point_begin=md.point_begin, dist_step=md.dist_step, ND=md.ND, NANG=md.NANG, NA=md.NA,
                 bucket_begin=md.bucket_begin, entry_point=md.entry_point, entry_cs=md.entry_cs, diameter=md.diameter)
    bb, ep, ec = pp.model_build(md.points, md.normals, md.point_begin, md.dist_step, md.ND, md.NANG, md.NA, md.ang_cos)
    assert bb.tobytes() == md.bucket_begin.tobytes() and ep.tobytes() == md.entry_point.tobytes() and ec.tobytes() == md.entry_cs.tobytes()
    assert md.n_entries == len(ep) and md.build_seconds > 0
    views = list(VIEWS)
    out, refined, iou, kept = _device_chain(ds, est, views, VIEW_GATE, VIEW_REF_STEP, VIEW_DENSE_GATE)
    assert all(torch.is_tensor(o) and o.is_cuda for o in est.estimate(*_estimate_args(ds, views)))
    depth, mask, window, corner = _view_call(ds, views)
    mv = int(mask.cpu().numpy().max())
    items = np.concatenate([np.arange(8)[:, None], np.zeros((8, 1), dtype=np.int64), corner, np.arange(8)[:, None], np.full((8, 1), mv)], axis=1)
    want = pp.ppf_np(model, ds.proj_mat, depth.cpu().numpy(), ds.udp.ray_map, mask.cpu().numpy(), items, 10000.0, window[0], window[1], 1, 1, VIEW_GATE,
                     VIEW_REF_STEP, 4, pp.cluster_trace(15.0), md.diameter * 0.1, (md.ang_cos, md.alpha_cos, md.alpha_cs))
    _same(out, want, "wrapper")
    mssd = _mssd_over_diameter(ds, tool, views, refined[np.arange(8), kept])
    print("stats", want[2].tolist(), "kept ranks", kept.tolist(), "IoU", np.round(iou, 3).tolist(), "MSSD / diameter", ["%.2e" % e for e in mssd])
    assert (want[2][:, 0] == pp.OK).all() and max(mssd) < 0.01, "top 4, refine, verify and select ends below 0.01 diameter on all eight"
    base = dict(zip(("depth", "frame", "obj", "corner", "window"), _estimate_args(ds, views)))
    launched = est._scratch.data_ptr()
    for change in (dict(depth=base["depth"].cpu()), dict(depth=base["depth"].to(torch.int32)), dict(frame=base["frame"].float()),
                   dict(obj=base["obj"][:3]), dict(corner=base["corner"][:, :1]), dict(mask=mask[:, :-1]), dict(mask=mask.cpu())):
        with pytest.raises(RuntimeError, match="pose_ppf"):
            est.estimate(**dict(base, **change))
    for change in (dict(step=0), dict(step=65), dict(ref_step=0), dict(reach=0), dict(reach=9), dict(gate=-1), dict(gate=65536), dict(k=0), dict(k=17),
                   dict(window=(0, 4)), dict(window=(1 << 15, (1 << 15) + 1)), dict(window=(129, 128)), dict(window=(128, 128), ref_step=1),
                   dict(cluster_deg=-1.0), dict(cluster_frac=float("nan")), dict(mask_frame=base["frame"])):
        with pytest.raises(ValueError, match="pose_ppf"):
            est.estimate(**dict(base, **change))
    assert est._scratch.data_ptr() == launched
    bare = lp.PpfEstimator(md, ds.proj_mat, ds.image_dims)
    with pytest.raises(ValueError, match="ray map"):
        bare.estimate(**base)
    for bad in (dict(points=1), dict(points=1025), dict(points=1024, alpha_bins=38), dict(alpha_bins=31), dict(angle_bins=33), dict(dist_frac=0.01)):
        with pytest.raises(ValueError, match="pose_ppf"):
            lp.PpfModels(ds.meshes, ds.model_scale, 10000.0, **bad)
    np.random.seed(1)
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    with pytest.raises(ValueError, match="keep_frames"):
        RenderedPoseDataset(mesh, 500, False, 0.0, False, **kw).ppf_estimator()
    import fabricate_cad as fab
    cloud_ds = RenderedPoseDataset((np.random.default_rng(0).normal(size=(2000, 3)).astype(np.float32) * 30, None, np.full((2000, 3), 130, dtype=np.uint8)),
                                   500, False, 0.0, False, proj_mat=fab.PROJ[1], image_dims=(64, 96), frames=4)
    with pytest.raises(ValueError, match="triangles"):
        cloud_ds.ppf_estimator()


def _estimate_args(ds, views):
    depth, _, window, corner = _view_call(ds, views)
    B = len(views)
    return depth, _up(np.arange(B), np.int64), _up(np.zeros(B), np.int64), _up(corner, np.int64), window
