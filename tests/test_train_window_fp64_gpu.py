"""GPU: the training step against the fp64 oracle (tests/oracle_grads.py), at window sizes that cross the chunk limits of the multi-bucket
pass and at the training shapes.

df_posenet_train_step_multi runs a whole accumulation window as one pass, one bucket per crop size.  Past 16 buckets the host code cuts
the bucket tables into chunks (train.hip TAB_MAX: the pooling / bilinear / up-conv / strided-dgrad tables; igemm.hip CONV_MAX_BUCKETS: the
multi-bucket direct kernel; wino.hip WINO_MAXB: the F(4x4,3x3) transforms), past 32 the weight gradient takes a second launch
(igemm.hip WGRAD_MAX_SEGS).  The windows here hold 34 and 18 crop sizes:
  * split-K off, the window equals the sum of its one-frame passes at the bounds of test_native_train_gpu.py (5e-6 of a tensor's scale,
    2e-6 relative L2 over the buffer, 2e-5 on the per-frame outputs).  The chunked paths do not depend on split-K (launch_conv_multi
    launches without it, the Winograd and bucket-table kernels never read it), so this covers their logic at a bound no chunk bug meets;
  * default split-K, every gradient and every frame's outputs against fp64 under the rule of oracle_grads (C x the fp32 CPU reference's
    own error, per tensor and per worst channel, and 2e-3 of the tensor's scale);
  * two identical passes are bit-identical.
The native steps at the YCB and LineMOD training shapes and the refiner at the YCB refine mesh size get the same fp64 anchor beside the
autograd-tape comparisons of test_native_train_gpu.py.  Two windows of the smallest crops the step accepts (tiny11: trunk maps of 1 x 1 .. 5 x 4 and
the 8 x 3200 / 3200 x 8 crops of the maximum side; ones3: 1 x 1 maps only) run the same three checks; they found the pyramid pooling
adjoint's missed bins (pool_bwd_all_kernel).  Each test prints its worst ratio of GPU error to fp32-reference error against
C = 4; measured on the MI355X: tiny11 0.06, small34 1.65, large18 1.63, mixed5 2.60, YCB 2.14, LineMOD 0.76 (its refiner 2.81), YCB refiner 0.05
(a ratio counts the floor as the reference's error where the floor is larger)."""
import numpy as np
import pytest
import torch

import oracle_grads as og
from densefusion_amd import _lib, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# stride-1 3x3 convolutions of the trunk that may take F(4x4,3x3): (name, dilation, channels)
WINO_LAYERS = (("layer2", 1, 128), ("layer3.0.conv2", 1, 256), ("layer3.1", 2, 256), ("layer4.0.conv2", 1, 512), ("layer4.1", 4, 512))


def _trunk(n):
    """Side of the layer2 .. layer4 maps of a crop side n: stem conv (7, stride 2, pad 3), max-pool (3, 2, 1), layer2 (3, 2, 1)."""
    for _ in range(3):
        n = (n - 1) // 2 + 1
    return n


def _f4_buckets(sizes):
    route = _lib.lib().df_wino_route
    return {name: sum(route(_trunk(h), _trunk(w), dil, c, c) == 4 for h, w in sizes) for name, dil, c in WINO_LAYERS}


def _trainer(kind, N, K, sd):
    from densefusion_amd.native_train import NativeTrainer
    tr = NativeTrainer(kind, N, K, DEV)
    tr.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return tr


def _dev_frames(objs):
    keys = ("img", "cloud", "choose", "obj", "target", "model_points")
    return [dict({k: torch.from_numpy(o[k]).to(DEV) for k in keys}, symmetric=o["symmetric"]) for o in objs]


def _close(a, b, rtol, name):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    scale = max(b.abs().max().item(), 1e-12)
    err = (a - b).abs().max().item()
    assert err <= rtol * scale, f"{name}: max err {err:.3e} vs scale {scale:.3e}"


def _window_equals_its_one_frame_passes(tr, frames):
    tr.set_splitk(False)
    tr.zero_grad()
    out, order = tr.step_posenet_window(frames, 0.015, dropout=False)
    g_multi = tr.grad_dict()
    tr.zero_grad()
    for row, j in enumerate(order):
        f = frames[j]
        o1 = tr.step_posenet(f["img"][None], f["cloud"][None], f["choose"].reshape(1, -1), f["obj"].reshape(1), f["target"][None], f["model_points"][None],
                             [f["symmetric"]], 0.015, dropout=False)
        for k in og.OUT_KEYS:
            _close(out[k][row:row + 1], o1[k], 2e-5, f"frame {j} {k}")
    num, den = 0.0, 0.0
    for k, v in tr.grad_dict().items():
        if "classifier" in k:
            assert float(g_multi[k].abs().max()) == 0.0
            continue
        scale = max(float(v.abs().max()), 1e-12)
        err = float((g_multi[k] - v).abs().max()) / scale
        assert err <= 5e-6, f"split-K off: {k}: window vs sum of one-frame passes {err:.2e} of the tensor's scale"
        num += float(((g_multi[k] - v).double() ** 2).sum()); den += float((v.double() ** 2).sum())
    assert (num / den) ** 0.5 <= 2e-6, f"split-K off: relative L2 over the buffer {(num / den) ** 0.5:.2e}"
    tr.set_splitk(True)


def _window_against_fp64(name, tr, frames, r64, r32):
    tr.zero_grad()
    out, order = tr.step_posenet_window(frames, 0.015, dropout=False)
    assert sorted(order) == list(range(len(frames)))
    g_ratio, g_where, n = og.check_grads(tr.grad_dict(), r64, r32)
    o_ratio, o_where = og.check_outputs(out, order, r64, r32)
    assert n >= 70
    print(f"{name}: worst ratio to the fp32 reference's error (C = {og.C}): gradients {g_ratio:.2f} ({g_where}), outputs {o_ratio:.2f} ({o_where})")


@pytest.mark.parametrize("name", ["small34", "large18"])
def test_window_past_the_bucket_chunk_limits(name):
    K, N, M, sd, objs = og.window(name)
    all_sizes = [(o["img"].shape[1], o["img"].shape[2]) for o in objs]
    sizes = list(dict.fromkeys(all_sizes))
    f4 = _f4_buckets(sizes)
    if name == "small34":
        # > 32 buckets: two weight-gradient launches; > 16 on each route of one layer: two chunks of the F(4x4) transforms and of the
        # multi-bucket direct kernel; crops that are not multiples of 8; buckets of 2 and 3 frames
        assert len(sizes) >= 33 and f4["layer3.1"] >= 17 and len(sizes) - f4["layer3.1"] >= 17, f4
        assert sum(h % 8 != 0 and w % 8 != 0 for h, w in sizes) >= 2
        assert sorted(n for n in (all_sizes.count(s) for s in sizes) if n > 1) == [2, 3]
    else:
        assert 17 <= len(sizes) <= 20 and (160, 160) in sizes, sizes
        assert max(f4.values()) >= 17 and f4["layer2"] >= 1, f4
    assert any(o["symmetric"] for o in objs) and not all(o["symmetric"] for o in objs)
    r64, r32 = og.posenet_oracle(sd, objs)
    frames = _dev_frames(objs)
    tr = _trainer("posenet", N, K, sd)
    _window_equals_its_one_frame_passes(tr, frames)
    _window_against_fp64(name, tr, frames, r64, r32)
    _two_dropout_passes_are_bit_identical(tr, frames)


def _two_dropout_passes_are_bit_identical(tr, frames):
    runs = []
    for _ in range(2):
        tr.zero_grad()
        tr.step_posenet_window(frames, 0.015, dropout=True, seed=5)
        runs.append(tr.grad.clone())
    assert torch.equal(runs[0], runs[1]) and float(runs[0].abs().sum()) > 0


def test_window_of_the_smallest_crops_and_the_maximum_side():
    """tiny11: crops of 8 .. 36 pixels (trunk maps of 1 x 1 .. 5 x 4) and the 8 x 3200 / 3200 x 8 crops of the maximum side in one window,
    N = 70 poses of M = 60 mesh points (the last workgroup of the symmetric loss holds 6 of its 8 poses).  On these maps the pyramid's
    pooling bins are wider than the map: a pixel of a 1 x 1 map lies in all 36 bins of the 6-bin stage, one of a 2 x 2 map in 3 per axis.
    pool_bwd_all_kernel searched three candidate bins per axis, complete only for maps of at least 3 pixels per side, and lost the others'
    gradients (0.38 .. 0.43 relative L2 on the trunk weight gradients of this window in the fp64 emulation of tests/test_oracle_grads.py, 177x
    the bound and more).  With the exact bin range it prints, on the MI355X, a worst ratio to the fp32 reference's error (C = 4) of 0.06 on
    the gradients (feat.conv5.weight) and 0.02 on the outputs (new_points)."""
    K, N, M, sd, objs = og.window("tiny11")
    sizes = [(o["img"].shape[1], o["img"].shape[2]) for o in objs]
    maps = {(_trunk(h), _trunk(w)) for h, w in sizes}
    assert maps >= {(1, 1), (2, 2), (1, 3), (3, 1), (2, 3), (4, 4), (5, 4), (2, 5), (1, 400), (400, 1)} and sizes.count((8, 8)) == 2, maps
    assert N % (512 // M) != 0 and 512 // M > 1                 # a ragged last group of poses in the symmetric loss
    assert [i for i, o in enumerate(objs) if o["symmetric"]] == [1, 4, 7, 10]
    r64, r32 = og.posenet_oracle(sd, objs)
    frames = _dev_frames(objs)
    tr = _trainer("posenet", N, K, sd)
    _window_equals_its_one_frame_passes(tr, frames)
    _window_against_fp64("tiny11", tr, frames, r64, r32)
    _two_dropout_passes_are_bit_identical(tr, frames)


def test_window_of_one_pixel_trunk_maps_only():
    """ones3: three 8 x 8 frames, one of them symmetric: every trunk map is 1 x 1, so a defect of the one-pixel map (the pyramid's pooling
    adjoint above all) cannot hide behind larger frames in the summed gradients: the three-candidate rule moves every trunk gradient of this
    window by 415x its bound and more (tests/test_oracle_grads.py).  Three frames do not dilute a single flipped ReLU either: with oseed 3100 a
    conv6 pre-activation lies 1.1e-6 from zero, and the GPU step missed the 1e-4 floor on feat.conv5 / feat.conv6 (3.6e-4 .. 3.9e-4 relative)
    while every other tensor passed; the fixture now keeps og.point_relu_margin above og.RELU_MARGIN, asserted here."""
    K, N, M, sd, objs = og.window("ones3")
    assert all(o["img"].shape[1:] == (8, 8) for o in objs) and [o["symmetric"] for o in objs] == [False, True, False]
    r64, r32 = og.posenet_oracle(sd, objs)
    assert og.point_relu_margin(sd, objs, r64) >= og.RELU_MARGIN, "a point-layer ReLU within fp32 rounding of zero -- ill-conditioned fixture"
    frames = _dev_frames(objs)
    tr = _trainer("posenet", N, K, sd)
    _window_equals_its_one_frame_passes(tr, frames)
    _window_against_fp64("ones3", tr, frames, r64, r32)
    _two_dropout_passes_are_bit_identical(tr, frames)


def test_mixed_window_at_default_splitk_against_fp64():
    """The five-frame window of test_native_train_gpu.py (K = 3, N = 128, crops 40 x 80 .. 160 x 160) at the default split-K: against fp64
    beside the comparison with the library's own one-frame passes at 2e-2."""
    K, N, M, sd, objs = og.window("mixed5")
    r64, r32 = og.posenet_oracle(sd, objs)
    _window_against_fp64("mixed5", _trainer("posenet", N, K, sd), _dev_frames(objs), r64, r32)


def _posenet_step_against_fp64(name, K, N, H, W, M, wseed, oseed, objs_idx, sym):
    sd = synth.make_state_dict(synth.posenet_spec(K), wseed)
    objs = [synth.make_object(oseed + i, H, W, N, K, num_points_mesh=M) for i in range(len(objs_idx))]
    for o, i, s in zip(objs, objs_idx, sym):
        o["obj"][0], o["symmetric"] = i, s
    r64, r32 = og.posenet_oracle(sd, objs)
    f = {k: torch.stack([torch.from_numpy(o[k]) for o in objs]).to(DEV) for k in ("img", "cloud", "choose", "obj", "target", "model_points")}
    tr = _trainer("posenet", N, K, sd)
    out = tr.step_posenet(f["img"], f["cloud"], f["choose"], f["obj"], f["target"], f["model_points"], sym, 0.015, dropout=False, want_pred=True)
    g_ratio, g_where, n = og.check_grads(tr.grad_dict(), r64, r32)
    o_ratio, o_where = og.check_outputs(out, range(len(objs)), r64, r32, og.OUT_KEYS + ("pred_r", "pred_t", "pred_c"))
    assert n >= 70
    print(f"{name}: worst ratio (C = {og.C}): gradients {g_ratio:.2f} ({g_where}), outputs {o_ratio:.2f} ({o_where})")
    return objs, out


def test_native_step_at_the_ycb_training_shape_against_fp64():
    """The fixture of test_native_step_at_the_ycb_training_shape_with_adam_and_a_hipgraph: K = 21, N = 1000, M = 500, 80 x 120, symmetric
    object 15 beside plain object 3."""
    _posenet_step_against_fp64("ycb", 21, 1000, 80, 120, 500, 13, 105, [15, 3], [True, False])


def _refiner_step_against_fp64(name, K, N, rsd, frames):
    r64, r32 = og.refiner_oracle(rsd, frames)
    T = lambda k: torch.stack([torch.as_tensor(f[k]).to(DEV) for f in frames])
    tr = _trainer("refiner", N, K, rsd)
    out = tr.step_refiner(T("points"), T("emb"), torch.tensor([f["obj"] for f in frames], device=DEV), T("target"), T("model_points"),
                          [f["symmetric"] for f in frames])
    g_ratio, g_where, n = og.check_grads(tr.grad_dict(), r64, r32)
    o_ratio, o_where = og.check_outputs(out, range(len(frames)), r64, r32, ("dis", "new_points", "new_target"))
    assert n >= 20
    print(f"{name}: worst ratio (C = {og.C}): gradients {g_ratio:.2f} ({g_where}), outputs {o_ratio:.2f} ({o_where})")


def test_native_steps_at_the_linemod_training_shape_against_fp64():
    """The fixture of test_native_steps_at_the_linemod_training_shape: K = 13, N = 500, M = 500, 120 x 80, eggbox (7, symmetric) beside
    object 2; then the refiner step on the PoseNet step's re-centred points and embeddings."""
    K, N, M = 13, 500, 500
    objs, out = _posenet_step_against_fp64("linemod", K, N, 120, 80, M, 31, 305, [7, 2], [True, False])
    rsd = synth.make_state_dict(synth.refiner_spec(K), 32)
    frames = [dict(points=out["new_points"][b], emb=out["emb"][b], obj=int(o["obj"][0]), target=out["new_target"][b],
                   model_points=o["model_points"], symmetric=o["symmetric"]) for b, o in enumerate(objs)]
    _refiner_step_against_fp64("linemod refiner", K, N, rsd, frames)


def test_refiner_step_at_the_ycb_refine_mesh_size_against_fp64():
    """The fixture of test_refiner_step_at_the_ycb_refine_mesh_size: K = 21, N = 1000, M = 2600 (a 2600 x 2600 nearest-neighbour search for
    the symmetric frame), objects 19 (symmetric) and 4."""
    K, N, M = 21, 1000, 2600
    objs = [synth.make_object(403 + i, 80, 80, N, K, num_points_mesh=M) for i in range(2)]
    emb = np.random.default_rng(2).standard_normal((2, 32, N)).astype(np.float32)
    frames = [dict(points=o["cloud"], emb=emb[b], obj=i, target=o["target"], model_points=o["model_points"], symmetric=s)
              for b, (o, i, s) in enumerate(zip(objs, (19, 4), (True, False)))]
    _refiner_step_against_fp64("ycb refiner", K, N, synth.make_state_dict(synth.refiner_spec(K), 1013), frames)
