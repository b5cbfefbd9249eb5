"""GPU: ``df_pose_verify`` against its restatement (tests/pose_verify_np.py) bit for bit in all twelve columns, against the existing mesh
renderer, its argument errors and the wrapper ``lib.pose_verify.PoseVerifier``.

Frames are 48 x 64, F = 3, O = 4 (``pose_verify_np.make_scene``).  Two configurations carry the triangle ranges 1, 63, 64, 65, 130 and an
empty one (63 / 64 / 65 is the wave set-up boundary); the range of 1 is a triangle far above SMALL_NODES nodes, which the whole wave
walks, and one item cuts it with a 16 x 16 window on all four sides.  B = 1, 5 and 67; windows: the whole frame, 16 x 16, 1 x 1, 17 x 37,
each at corners inside the frame, over each of its four edges (negative corners among them) and wholly outside."""
import ctypes

import numpy as np
import pytest
import torch

import mesh_closest_np as m
import pose_verify_np as pv

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _up(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


class Call:
    """One ``df_pose_verify`` call on a scene with every argument open to a test: ``run(**changes)`` -> (rc, stats, scratch bytes)."""

    def __init__(self, sc, items, pose, WH, WW, tol, cull=0, mask=True, cloud_div=pv.CLOUD_DIV):
        from densefusion_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.v, self.t = _up(sc["vertices"], np.float32), _up(sc["triangles"], np.int32)
        self.begin = np.ascontiguousarray(sc["tri_begin"], dtype=np.int32)
        self.scale = np.ascontiguousarray(sc["model_scale"], dtype=np.float64)
        self.proj = np.ascontiguousarray(sc["proj"], dtype=np.float64).reshape(-1)
        self.depth, self.mask = _up(sc["depth"], np.uint16), (_up(sc["mask"], np.uint16) if mask else None)
        self.items, self.pose = _up(items, np.int32), _up(pose, np.float64)
        F, IH, IW = sc["depth"].shape
        self.a = dict(vertices=self.v.data_ptr(), V=len(sc["vertices"]), triangles=self.t.data_ptr(), T=len(sc["triangles"]),
                      tri_begin=self.begin.ctypes.data, model_scale=self.scale.ctypes.data, O=len(self.begin) - 1, proj=self.proj.ctypes.data,
                      depth=self.depth.data_ptr(), F=F, IH=IH, IW=IW, mask=self.mask.data_ptr() if mask else None,
                      NM=len(sc["mask"]) if mask else 0, items=self.items.data_ptr(), pose=self.pose.data_ptr(), cloud_div=cloud_div,
                      B=len(items), WH=WH, WW=WW, tol=tol, cull=cull)

    def run(self, short_scratch=0, misalign=0, null_stats=False, null_scratch=False, **changes):
        a = dict(self.a, **changes)
        B = len(self.items)
        need = max(self.L.df_pose_verify_scratch_bytes(B, self.a["WH"], self.a["WW"]), 8)
        stats = torch.full((B, 12), SENTINEL * 0x0101010101010101, dtype=torch.int64, device="cuda")
        scratch = torch.full((need + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
        rc = self.L.df_pose_verify(a["vertices"], a["V"], a["triangles"], a["T"], a["tri_begin"], a["model_scale"], a["O"], a["proj"],
                                   a["depth"], a["F"], a["IH"], a["IW"], a["mask"], a["NM"], a["items"], a["pose"],
                                   ctypes.c_double(a["cloud_div"]), a["B"], a["WH"], a["WW"], a["tol"], a["cull"],
                                   None if null_stats else stats.data_ptr(), None if null_scratch else scratch.data_ptr() + misalign,
                                   need - short_scratch, self.lib.current_stream())
        return rc, stats.cpu().numpy(), scratch.cpu().numpy()


def _device(sc, items, pose, WH, WW, tol, cull=0, mask=True, cloud_div=pv.CLOUD_DIV):
    call = Call(sc, items, pose, WH, WW, tol, cull, mask, cloud_div)
    rc, stats, _ = call.run()
    assert rc == 0, call.L.df_last_error()
    return stats


def _want(sc, items, pose, WH, WW, tol, cull=0, mask=True, cloud_div=pv.CLOUD_DIV, keys_out=None):
    return pv.verify_np(sc["vertices"], sc["triangles"], sc["tri_begin"], sc["model_scale"], sc["proj"], sc["depth"],
                        sc["mask"] if mask else None, items, pose, cloud_div, WH, WW, tol, cull, keys_out)


def _same(got, want, name):
    assert got.dtype == np.int64 and m.same_bits(got, want), f"{name}: the tallies differ in rows {np.where((got != want).any(axis=1))[0].tolist()}\n" \
        f"{got[(got != want).any(axis=1)][:4]}\n{want[(got != want).any(axis=1)][:4]}"


@pytest.fixture(scope="module")
def scenes():
    _dev()
    return {c: pv.make_scene(c) for c in pv.RANGES}


WINDOWS = ((48, 64), (16, 16), (1, 1), (17, 37))


@pytest.mark.parametrize("config", sorted(pv.RANGES))
def test_ranges_item_counts_and_windows(scenes, config):
    sc = scenes[config]
    assert tuple(np.diff(sc["tri_begin"])) == pv.RANGES[config]
    total = np.zeros(12, dtype=np.int64)
    for w, (WH, WW) in enumerate(WINDOWS):
        for B in ((1, 5, 67) if (WH, WW) == (17, 37) else (1, 67) if (WH, WW) == (16, 16) else (5,)):
            items, pose = pv.make_call(B, WH, WW, 10 * w + B)
            want = _want(sc, items, pose, WH, WW, 4)
            _same(_device(sc, items, pose, WH, WW, 4), want, f"{config} {WH}x{WW} B={B}")
            total += want.sum(axis=0)
            for b, (r0, c0) in enumerate(items[:, 2:4].tolist()):
                if r0 >= pv.IH or c0 >= pv.IW or r0 + WH <= 0 or c0 + WW <= 0:
                    assert not want[b].any(), "a window wholly outside the frame: zeros, status 0"
            if B == 67:
                for o, n in enumerate(pv.RANGES[config]):
                    assert (want[items[:, 1] == o, 1] > 0).any() == (n > 0), f"object {o} is drawn in some item (an empty range in none)"
    print(config, dict(zip(pv.STATS, total.tolist())))
    assert total[0] == 0 and all(total[k] > 0 for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)), "every class and both triangle counts are exercised"


def test_large_triangle_cut_on_all_four_sides(scenes):
    """The one-triangle range at an upright pose spans some 45 rows and 37 columns; a 16 x 16 window in its middle cuts the node range
    on all four sides, and the whole wave walks what is left (256 nodes, above SMALL_NODES)."""
    sc = scenes["a"]
    items = np.array([[2, 0, 20, 24, 0, 0], [2, 0, 0, 0, 0, 0]], dtype=np.int32)
    pose = np.array([[2.0, 0, 0, 0, 0, 0, -0.4]] * 2)
    keys = []
    want = _want(sc, items, pose, 16, 16, 4, keys_out=keys)
    whole = _want(sc, items[1:], pose[1:], pv.IH, pv.IW, 4, keys_out=keys)
    rows, cols = np.where(keys[2] != pv.NO_KEY)
    assert rows.min() < 20 and rows.max() > 35 and cols.min() < 24 and cols.max() > 39, "the triangle passes the window on every side"
    assert want[0, 10] == 1 and want[0, 11] == 1 and want[0, 1] > 16 and whole[0, 11] == 0
    _same(_device(sc, items, pose, 16, 16, 4), want, "cut triangle")


@pytest.mark.parametrize("tol", (0, 1, 7, 65535))
def test_tolerance_boundaries(scenes, tol):
    """The observed frame is the restatement's own rendered codes plus (-tol-1, -tol, 0, +tol, +tol+1) cycling with (r + q) % 5, clamped
    to 0..65534, every 7th node forced to 65535: all four class boundaries are hit exactly."""
    sc = dict(scenes["b"])
    items, pose = np.array([[1, 1, 0, 0, 0, 65535]], dtype=np.int32), np.array([pv.FRAME0_POSE])
    keys = []
    _want(sc, items, pose, pv.IH, pv.IW, 0, keys_out=keys)
    cr = pv.rendered_codes(keys[0], 0, 0, pv.IH, pv.IW)
    r, q = np.mgrid[0:pv.IH, 0:pv.IW]
    off = np.array([-tol - 1, -tol, 0, tol, tol + 1])[(r + q) % 5]
    obs = np.where(cr != pv.NO_OBSERVATION, np.clip(cr + off, 0, 65534), 12345)
    obs[(r * pv.IW + q) % 7 == 0] = 65535
    depth = sc["depth"].copy()
    depth[1] = obs
    sc["depth"] = depth
    want = _want(sc, items, pose, pv.IH, pv.IW, tol)
    rendered, seen = cr != pv.NO_OBSERVATION, obs != 65535
    if tol < 65535:                                               # mid-range codes: nothing was clamped, so the classes follow from the offsets
        assert ((cr[rendered] - tol - 1 >= 0) & (cr[rendered] + tol + 1 <= 65534)).all()
        n = [int((rendered & seen & ((r + q) % 5 == k)).sum()) for k in range(5)]
        assert want[0, 1:6].tolist() == [int(rendered.sum()), n[1] + n[2] + n[3], n[0], n[4], int((rendered & ~seen).sum())]
        assert min(n) > 0 and want[0, 9] == tol * (n[1] + n[3])
    else:                                                         # every observed code is within 65535 of every rendered one
        assert want[0, 2] == int((rendered & seen).sum()) and want[0, 3] == want[0, 4] == 0
    _same(_device(sc, items, pose, pv.IH, pv.IW, tol), want, f"tol {tol}")


def test_mask_given_and_absent(scenes):
    """Items whose ``mask_frame`` differs from ``frame`` and whose ``mask_value`` is 7, 0 or 65535; without a mask the three mask columns
    are zero and the others unchanged."""
    sc = scenes["b"]
    items, pose = pv.make_call(12, 17, 37, 5)
    items[:, 4] = (items[:, 0] + 1) % pv.NM
    assert (items[:, 4] != items[:, 0]).any() and {0, 7, 65535} >= set(items[:, 5].tolist()) and 7 in items[:, 5]
    with_mask, without = _want(sc, items, pose, 17, 37, 3), _want(sc, items, pose, 17, 37, 3, mask=False)
    assert not without[:, 6:9].any() and with_mask[:, 6:9].any(axis=0).all()
    keep = [0, 1, 2, 3, 4, 5, 9, 10, 11]
    assert (with_mask[:, keep] == without[:, keep]).all()
    _same(_device(sc, items, pose, 17, 37, 3), with_mask, "mask")
    _same(_device(sc, items, pose, 17, 37, 3, mask=False), without, "no mask")


def test_bad_items_leave_their_neighbours_alone(scenes):
    sc = scenes["a"]
    items, pose = pv.make_call(9, 16, 16, 6)
    items[:, 2:4] = (14, 22)
    good = items.copy()
    for b, (col, val) in {1: (0, -1), 2: (0, pv.F), 4: (1, -1), 5: (1, pv.O), 7: (4, -1), 8: (4, pv.NM)}.items():
        items[b, col] = val
    bad = [1, 2, 4, 5, 7, 8]
    want = _want(sc, items, pose, 16, 16, 4)
    assert want[bad, 0].tolist() == [1] * 6 and not want[bad, 1:].any() and not want[[0, 3, 6], 0].any()
    got = _device(sc, items, pose, 16, 16, 4)
    _same(got, want, "bad items")
    assert (got[[0, 3, 6]] == _device(sc, good, pose, 16, 16, 4)[[0, 3, 6]]).all(), "the neighbours of a bad item are unchanged"
    # without a mask the mask frame is not looked at
    want = _want(sc, items, pose, 16, 16, 4, mask=False)
    assert want[:, 0].tolist() == [0, 1, 1, 0, 1, 1, 0, 0, 0]
    _same(_device(sc, items, pose, 16, 16, 4, mask=False), want, "bad items, no mask")


def test_nan_pose_draws_nothing(scenes):
    sc = scenes["b"]
    items, pose = pv.make_call(5, 48, 64, 7)
    items[:, 2:4] = 0
    pose[1, 2], pose[3, 5] = np.nan, np.nan                      # a NaN in the quaternion; a NaN translation
    want = _want(sc, items, pose, 48, 64, 4)
    assert not want[[1, 3], 0].any() and not want[[1, 3], 1].any() and not want[[1, 3], 10].any() and want[[0, 2, 4], 1].all()
    _same(_device(sc, items, pose, 48, 64, 4), want, "NaN pose")


def test_cull(scenes):
    sc = scenes["b"]
    items, pose = pv.make_call(8, 48, 64, 8)
    items[:, 2:4] = 0
    both, front = _want(sc, items, pose, 48, 64, 4, cull=0), _want(sc, items, pose, 48, 64, 4, cull=1)
    assert (front[:, 10] <= both[:, 10]).all() and (front[:, 10] < both[:, 10]).any()
    _same(_device(sc, items, pose, 48, 64, 4, cull=0), both, "cull 0")
    _same(_device(sc, items, pose, 48, 64, 4, cull=1), front, "cull 1")


def test_sum_abs_needs_64_bits():
    """256 x 256 frame and window, one far, flat, two-triangle quad over the whole frame, observed depth all 0, tol 65535: every node
    agrees and sum_abs is the sum of the rendered codes.  With 65536 nodes of at most 65534 each the sum stays below 2^32 (65536 x 65534
    = 2^32 - 131072); it is far above 2^31, which is what a 32-bit signed tally would wrap at."""
    _dev()
    v, t = pv.quad(9000.0, 4500.0)
    sc = dict(vertices=v, triangles=t, tri_begin=np.array([0, 2], np.int32), model_scale=np.array([1.0]), proj=np.array(pv.PROJ),
              depth=np.zeros((1, 256, 256), np.uint16), mask=np.zeros((1, 256, 256), np.uint16))
    items, pose = np.array([[0, 0, 0, 0, 0, 0]], dtype=np.int32), np.array([[1.0, 0, 0, 0, 0, 0, -0.595]])
    want = _want(sc, items, pose, 256, 256, 65535)
    print("sum_abs", int(want[0, 9]), "= 2^31 x", want[0, 9] / 2.0 ** 31)
    assert want[0, 1] == want[0, 2] == 256 * 256 and want[0, 9] > 2 ** 31 and want[0, 9] > 65000 * 65536
    _same(_device(sc, items, pose, 256, 256, 65535), want, "sum_abs")


@pytest.mark.parametrize("turn", (0, 1, 2))
def test_against_the_mesh_renderer(turn):
    """The observed depth is ``df_cad_render_mesh``'s own output for [I | t] on an icosphere(2) squashed to an ellipsoid; verifying q =
    (1, 0, 0, 0) (exact under quat_to_mat), the same t with cloud_div 1, the whole frame, tol 0 and the renderer's pixel mask must find
    every rendered node in agreement.  Other orientations are made exact by turning the vertices, not the pose."""
    _dev()
    from densefusion_amd.datasets.customCAD.render import CadMeshRenderer
    from densefusion_amd.lib.pose_verify import PoseVerifier
    v, t = pv.ellipsoid(2, None, 150.0)
    if turn:
        Rm = np.array(m.rotation_xf([1, 2 - turn, 0.5 * turn], 0.7 * turn))[:, :3]
        v = (v.astype(np.float64) @ Rm.T).astype(np.float32)
    colors = np.full((len(v), 3), 99, dtype=np.uint8)
    T34 = np.array([[1, 0, 0, 130.0], [0, 1, 0, -75.0], [0, 0, 1, -4100.0]])
    for cull in (0, 1):
        _, depth, mask, stats = CadMeshRenderer(v, t, colors, pv.PROJ, (pv.IH, pv.IW), model_scale=10.0).render(T34[None], cull=cull, mask="pixels")
        ver = PoseVerifier([(v, t)], 10.0, pv.PROJ, (pv.IH, pv.IW), cloud_div=1.0)
        pose = _up([[1, 0, 0, 0, 130.0, -75.0, -4100.0]], np.float64)
        zero = torch.zeros(1, dtype=torch.int32, device="cuda")
        got = ver.score(depth, pose, zero, zero, torch.zeros(1, 2, dtype=torch.int32, device="cuda"), (pv.IH, pv.IW), 0, mask=mask, cull=bool(cull))
        got, n = got.cpu().numpy()[0], int(stats.cpu().numpy()[0, 0])
        print(dict(zip(pv.STATS, got.tolist())), "renderer:", stats.cpu().numpy()[0].tolist())
        assert n > 400 and got[1] == got[2] == got[6] == got[7] == n and got[10] == int(stats.cpu().numpy()[0, 1])
        assert not got[[0, 3, 4, 5, 8, 9]].any()


def test_determinism_and_independence(scenes):
    sc = scenes["b"]
    items, pose = pv.make_call(5, 17, 37, 9)
    call = Call(sc, items, pose, 17, 37, 2)
    (rc1, s1, k1), (rc2, s2, k2) = call.run(), call.run()
    assert rc1 == rc2 == 0 and s1.tobytes() == s2.tobytes() and k1.tobytes() == k2.tobytes(), "two identical calls give identical bytes"
    for b in range(5):
        assert (_device(sc, items[b:b + 1], pose[b:b + 1], 17, 37, 2)[0] == s1[b]).all(), f"item {b} alone equals its row of the call"


def test_argument_errors_touch_nothing(scenes):
    sc = scenes["a"]
    items, pose = pv.make_call(3, 16, 16, 11)
    call = Call(sc, items, pose, 16, 16, 4)
    L = call.L
    assert L.df_pose_verify_scratch_bytes(3, 16, 16) == 3 * 256 * 8 and L.df_pose_verify_scratch_bytes(0, 16, 16) == 0
    assert L.df_pose_verify_scratch_bytes(65536, 1, 1) == 0 and L.df_pose_verify_scratch_bytes(1, 0, 5) == 0
    assert L.df_pose_verify_scratch_bytes(1, 1 << 15, (1 << 15) + 1) == 0 and L.df_pose_verify_scratch_bytes(1, 1 << 15, 1 << 15) == 8 << 30
    begin_bad0, begin_dec, begin_end = call.begin.copy(), call.begin.copy(), call.begin.copy()
    begin_bad0[0], begin_dec[2], begin_end[-1] = 1, begin_dec[1] - 1, begin_end[-1] - 1
    proj_bad = call.proj.copy()
    proj_bad[14] = -2.0
    bad = [dict(vertices=None), dict(triangles=None), dict(tri_begin=None), dict(model_scale=None), dict(proj=None), dict(depth=None),
           dict(items=None), dict(pose=None), dict(null_stats=True), dict(null_scratch=True), dict(NM=0), dict(NM=-1), dict(B=0), dict(B=65536),
           dict(WH=0), dict(WW=0), dict(WH=-1), dict(WH=1 << 15, WW=(1 << 15) + 1), dict(F=0), dict(F=65536), dict(IH=0), dict(IW=0),
           dict(IH=1 << 15, IW=(1 << 15) + 1), dict(V=0), dict(T=0), dict(O=0), dict(O=65), dict(tri_begin=begin_bad0.ctypes.data),
           dict(tri_begin=begin_dec.ctypes.data), dict(tri_begin=begin_end.ctypes.data), dict(proj=proj_bad.ctypes.data), dict(tol=-1),
           dict(tol=65536), dict(cull=2), dict(cull=-1), dict(cloud_div=0.0), dict(cloud_div=-1.0), dict(cloud_div=float("inf")),
           dict(cloud_div=float("nan")), dict(short_scratch=1), dict(misalign=4)]
    for change in bad:
        rc, stats, scratch = call.run(**change)
        assert rc == -1, f"{change}: DF_ERR_ARG expected, got {rc}"
        assert (stats.view(np.uint8) == SENTINEL).all() and (scratch == SENTINEL).all(), f"{change}: the call wrote before it refused"
    rc, stats, _ = call.run()
    assert rc == 0 and m.same_bits(stats, _want(sc, items, pose, 16, 16, 4))


def test_wrapper(scenes):
    from densefusion_amd.lib import pose_verify as lpv
    sc = scenes["b"]
    assert tuple(lpv.STATS) == tuple(pv.STATS)
    meshes = pv.make_meshes("b")
    ver = lpv.PoseVerifier(meshes, sc["model_scale"], pv.PROJ, (pv.IH, pv.IW))
    assert ver.tri_begin.tolist() == sc["tri_begin"].tolist() and ver.n_objects == 4
    items, pose = pv.make_call(5, 17, 37, 12)
    depth, mask, dpose = _up(sc["depth"], np.uint16), _up(sc["mask"], np.uint16), _up(pose, np.float64)
    it = _up(items, np.int64)
    args = (depth, dpose, it[:, 0], it[:, 1], it[:, 2:4], (17, 37), 3)
    got = ver.score(*args, mask=mask, mask_frame=it[:, 4], mask_value=it[:, 5])
    assert got.dtype == torch.int64 and got.is_cuda
    _same(got.cpu().numpy(), _want(sc, items, pose, 17, 37, 3), "wrapper")
    _same(ver.score(*args).cpu().numpy(), _want(sc, items, pose, 17, 37, 3, mask=False), "wrapper, no mask")
    other = ver.score(depth, _up(pv.random_poses(5, np.random.default_rng(2)), np.float64), *args[2:])
    for a, b in ((got, other), (other, got)):
        va, vb = lpv.vsiou(a).cpu().numpy(), lpv.vsiou(b).cpu().numpy()
        assert va.dtype == np.float64 and m.same_bits(va, pv.vsiou(a.cpu().numpy())) and m.same_bits(lpv.vsiou(a.cpu().numpy()), va)
        assert lpv.better(a, b).cpu().numpy().tolist() == (vb > va).tolist()
    assert lpv.vsiou(torch.zeros(2, 12, dtype=torch.int64)).tolist() == [0.0, 0.0]
    launched = ver._scratch.data_ptr()
    for change in (dict(depth=depth.cpu()), dict(depth=depth.to(torch.int32)), dict(pose=dpose.float()), dict(pose=dpose[:, :6]),
                   dict(frame=it[:3, 0]), dict(obj=it[:, 1].float()), dict(corner=it[:, 2:5]), dict(mask=mask[:, :-1]), dict(mask=mask.cpu())):
        kw = dict(depth=depth, pose=dpose, frame=it[:, 0], obj=it[:, 1], corner=it[:, 2:4], window=(17, 37), tol=3, mask=mask)
        kw.update(change)
        with pytest.raises(RuntimeError, match="pose_verify"):
            ver.score(**kw)
    for change in (dict(tol=-1), dict(tol=65536), dict(window=(0, 4)), dict(window=(1 << 15, (1 << 15) + 1))):
        kw = dict(depth=depth, pose=dpose, frame=it[:, 0], obj=it[:, 1], corner=it[:, 2:4], window=(17, 37), tol=3)
        kw.update(change)
        with pytest.raises(ValueError, match="pose_verify"):
            ver.score(**kw)
    assert ver._scratch.data_ptr() == launched
    with pytest.raises(ValueError):
        lpv.PoseVerifier([(meshes[0][0], np.array([[0, 1, len(meshes[0][0])]]))], 1.0, pv.PROJ, (pv.IH, pv.IW))
