"""Power and conditioning of the parameter-update tests (tests/test_trainer_updates_gpu.py), on the CPU oracle alone.

A NativeTrainer handle keeps device copies derived from its parameters: the flipped / transposed weights of every data gradient and the
F(4x4,3x3)-domain copies (forward and data gradient) of the trunk's stride-1 3x3 weights (csrc/train_tape.h, check_flips).  They are
rebuilt when the (version, address) of the parameter buffer changes.  The three ways that protocol can fail are emulated in the fp64
oracle here, on the update window of oracle_grads (upd4), with P0 its first state dict and P1 the one the GPU test reloads in full:
  1. a handle that ignored the update: gradients and outputs are those at P0;
  2. stale data-gradient weights: forward pass and weight gradients at P1, every convolution's / GEMM's gradient with respect to its
     input formed with the P0 weight;
  3. stale forward copies: the trunk convolutions a bucket routes through F(4x4,3x3) run forward with the P0 weight, all else at P1.
Each moves every parameter gradient it can reach by at least 3x that tensor's bound under the rule of oracle_grads, so the fp64
comparison of the GPU test fails on it.  (An Adam-sized update is another matter: it moves the gradients by less than some bounds, and
the GPU test catches a handle that misses one by the bit comparison with a fresh handle.)

The fixture's conditioning -- the same nearest targets and most confident point in fp32 and fp64, point-layer ReLUs clear of zero --
is asserted at every parameter set of the GPU sequences, reached here by emulating the updates (oracle_grads.AdamEmu for FlatAdam)."""
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle_grads as og
from densefusion_amd import _lib, synth
from oracle import dfnet

_ORIG = dict(conv2d=F.conv2d, conv1d=F.conv1d, linear=F.linear)
GRAPH_FRAMES, LANE_JOBS = og.UPDATE_GRAPH_FRAMES, og.UPDATE_LANE_JOBS


def _sd1_and_key(K):
    spec = synth.posenet_spec(K)
    return synth.make_state_dict(spec, og.UPDATE_WSEEDS[0]), synth.make_state_dict(spec, og.UPDATE_WSEEDS[1])[og.UPDATE_KEY]


def _scaled(sd, s):
    return {k: v * np.float32(s) for k, v in sd.items()}


# ---- conditioning at every parameter set of the GPU sequences ----
def test_the_posenet_update_sequence_stays_well_conditioned():
    """The parameter sets of the PoseNet sequence in order: P0, after FlatAdam, the full reload, the one-tensor reload, the in-place
    write, the rebound buffer, FlatAdam after the batch step, FlatAdam after the lanes' window.  og.posenet_oracle asserts the
    nearest-target and arg-max agreement of fp32 and fp64 at each; the point layers' ReLU margin is asserted beside it."""
    K, N, M, sd, objs = og.window("upd4")
    sd1, w2 = _sd1_and_key(K)
    adam = og.AdamEmu()
    margins = []

    def visit(name, p):
        r64, _ = og.posenet_oracle(p, objs)
        margins.append((name, og.point_relu_margin(p, objs, r64)))
        assert margins[-1][1] >= og.RELU_MARGIN, f"{name}: a point-layer ReLU within fp32 rounding of zero ({margins[-1][1]:.1e}) -- ill-conditioned fixture"
        return r64

    r64 = visit("P0", sd)
    p = adam.step(sd, og.summed_grads(r64))
    assert all(not np.array_equal(p[k], sd[k]) for k in sd if "classifier" not in k)
    visit("adam", p)
    visit("reload", sd1)
    p = dict(sd1, **{og.UPDATE_KEY: w2})
    visit("one tensor", p)
    p = _scaled(p, og.INPLACE_SCALE)
    visit("in place", p)
    p = _scaled(p, og.REBIND_SCALE)
    r64 = visit("rebound", p)
    p = adam.step(p, og.summed_grads([r64[j] for j in GRAPH_FRAMES]))
    r64 = visit("adam after the batch step", p)
    p = adam.step(p, og.summed_grads([r64[j] for j in LANE_JOBS]))
    visit("adam after the lanes", p)
    print("point-layer ReLU margins: " + ", ".join(f"{n} {m:.1e}" for n, m in margins))


def test_the_refiner_update_sequence_stays_well_conditioned():
    """Two refine iterations (the second on the first's new_points / new_target) at R0, after FlatAdam on their summed gradient, and
    after the reload: og.refiner_oracle's conditioning checks at each."""
    K, N, M, (sd0, sd1), frames = og.refiner_update_frames()
    assert [f["symmetric"] for f in frames] == [False, True]

    def pair(p):
        a64, _ = og.refiner_oracle(p, frames)
        second = og.second_iteration(frames, {k: [r[k][0] for r in a64] for k in ("new_points", "new_target")})
        b64, _ = og.refiner_oracle(p, second)
        return a64 + b64

    r64 = pair(sd0)
    p = og.AdamEmu().step(sd0, og.summed_grads(r64))
    assert all(not np.array_equal(p[k], sd0[k]) for k in sd0)
    pair(p)
    pair(sd1)


# ---- the three defects ----
class _Stale(torch.autograd.Function):
    """y = op(x, w_fwd, b); the gradient with respect to x is formed with w_bwd, the one with respect to the weight from x and dy as
    the step's weight-gradient kernels form it (they read no weight copy)."""

    @staticmethod
    def forward(ctx, x, w, b, w_fwd, w_bwd, op, kw):
        ctx.save_for_backward(x, w_bwd)
        ctx.op, ctx.kw, ctx.wshape, ctx.has_b = op, kw, w.shape, b is not None
        return _ORIG[op](x, w_fwd, b, **kw)

    @staticmethod
    def backward(ctx, gy):
        x, w_bwd = ctx.saved_tensors
        if ctx.op == "linear":
            gx, gw, gb = gy @ w_bwd, gy.t() @ x, gy.sum(0)
        else:
            inp, wgt = (torch.nn.grad.conv2d_input, torch.nn.grad.conv2d_weight) if ctx.op == "conv2d" else \
                       (torch.nn.grad.conv1d_input, torch.nn.grad.conv1d_weight)
            gx = inp(x.shape, w_bwd, gy, **ctx.kw) if ctx.needs_input_grad[0] else None
            gw = wgt(x, ctx.wshape, gy, **ctx.kw)
            gb = gy.sum(dim=[d for d in range(gy.dim()) if d != 1])
        return gx, gw, gb if ctx.has_b else None, None, None, None, None


def _defective_frames(sd, objs, choose):
    """The fp64 frames at ``sd`` with every convolution / GEMM whose weight leaf ``choose(key, leaf)`` knows replaced by _Stale;
    choose -> None, or a function (x, kw) -> (forward weight, data-gradient weight)."""
    table, met = {}, set()

    def on_params(psd):
        for k, leaf in psd.items():
            if leaf.dim() >= 2 and "classifier" not in k:        # (the forward pass never calls the dead classifier)
                pick = choose(k, leaf)
                if pick is not None:
                    table[id(leaf)] = pick

    def patched(op):
        def call(x, w, b=None, **kw):
            pick = table.get(id(w))
            if pick is None:
                return _ORIG[op](x, w, b, **kw)
            met.add(id(w))
            w_fwd, w_bwd = pick(x, kw)
            return _Stale.apply(x, w, b, w_fwd, w_bwd, op, kw)
        return call

    with mock.patch.object(dfnet.F, "conv2d", patched("conv2d")), mock.patch.object(dfnet.F, "conv1d", patched("conv1d")), \
            mock.patch.object(dfnet.F, "linear", patched("linear")):
        res = og.posenet_frames(sd, objs, torch.float64, on_params=on_params)
    assert table and met == set(table), f"{len(table) - len(met)} registered layers were never called through the patched functions"
    return res, table


def _moved(name, bad, g64, g32, keys):
    """Every tensor of ``keys`` moves by at least 3x its own bound; -> the smallest ratio."""
    worst, where = float("inf"), ""
    for k in keys:
        bound = max(og.C * og.rel_l2(g32[k], g64[k]), og.gpu_floor(k)[0])
        dev = og.rel_l2(bad[k], g64[k])
        assert dev >= 3 * bound, f"{name}: {k}: the defect moves the gradient by {dev:.2e}, bound {bound:.2e}"
        if dev / bound < worst:
            worst, where = dev / bound, k
    print(f"{name}: moves each of {len(keys)} gradients by >= {worst:.1f}x its bound ({where})")
    return worst


@pytest.fixture(scope="module")
def at_p1():
    K, N, M, sd0, objs = og.window("upd4")
    sd1, _ = _sd1_and_key(K)
    r64, r32 = og.posenet_oracle(sd1, objs)
    return sd0, sd1, objs, (r64, r32), og.summed_grads(r64), og.summed_grads(r32)


def test_a_handle_that_ignored_the_update_fails_the_bound(at_p1):
    sd0, sd1, objs, (r64, r32), g64, g32 = at_p1
    old = og.posenet_frames(sd0, objs, torch.float64)
    keys = list(g64)                                  # every tensor with a gradient: the dead classifier weights have none
    assert sum(k.startswith(og.CNN_PREFIXES) for k in keys) >= 35 and not any("classifier" in k for k in keys)
    assert _moved("ignored update", og.summed_grads(old), g64, g32, keys) >= 3
    for k in og.OUT_KEYS:                             # and every output kind
        bound = max(og.C * og.rel_l2(og.stacked(r32, k), og.stacked(r64, k)), og.GPU_FLOOR[0])
        assert og.rel_l2(og.stacked(old, k), og.stacked(r64, k)) >= 3 * bound, k


# what stale data-gradient weights cannot reach: a weight gradient is formed from the layer's input (forward pass: correct) and the
# gradient of its output, which for the last layer of each head tower comes straight from the loss
LAST_LAYERS = tuple(f"conv4_{h}.{p}" for h in "rtc" for p in ("weight", "bias"))


def test_stale_data_gradient_weights_fail_the_bound(at_p1):
    sd0, sd1, objs, _, g64, g32 = at_p1
    old = {k: torch.as_tensor(v).double() for k, v in sd0.items()}
    bad, table = _defective_frames(sd1, objs, lambda k, leaf: (lambda x, kw: (leaf.detach(), old[k])))
    assert len(table) == sum(np.ndim(v) >= 2 and "classifier" not in k for k, v in sd1.items())
    bad = og.summed_grads(bad)
    for k in LAST_LAYERS:
        assert og.rel_l2(bad[k], g64[k]) < 1e-12, k
    keys = [k for k in g64 if k not in LAST_LAYERS]
    assert sum(k.startswith(og.CNN_PREFIXES) for k in keys) >= 35 and len(keys) == len(g64) - 6
    assert _moved("stale data-gradient weights", bad, g64, g32, keys) >= 3


def test_stale_forward_copies_fail_the_bound(at_p1):
    """The defect lives in the buckets and layers that take F(4x4,3x3) (asked of df_wino_route with the rule of the step's conv()):
    layer3.1 on the 44 x 44 frames, layer3.0.conv2 / layer4.0.conv2 on the 24 x 24 one, nothing on the 40 x 40 one.  Their outputs
    feed everything downstream, and the gradient that comes back through them reaches everything upstream: no tensor with a gradient
    is out of reach (the dead classifier weights have none)."""
    sd0, sd1, objs, _, g64, g32 = at_p1
    old = {k: torch.as_tensor(v).double() for k, v in sd0.items()}
    route = _lib.lib().df_wino_route
    routed = set()

    def choose(k, leaf):
        if "feats.layer" not in k or leaf.dim() != 4 or leaf.shape[2] != 3 or leaf.shape[1] < 128:
            return None

        def pick(x, kw):
            f4 = kw.get("stride", 1) == 1 and route(x.shape[2], x.shape[3], kw.get("dilation", 1), leaf.shape[1], leaf.shape[0]) == 4
            if f4:
                routed.add((k, tuple(x.shape[2:])))
            return (old[k] if f4 else leaf.detach()), leaf.detach()
        return pick

    bad, _ = _defective_frames(sd1, objs, choose)
    layers = {k for k, _ in routed}
    assert og.UPDATE_KEY in layers and {hw for _, hw in routed} == {(6, 6), (3, 3)}, routed
    assert any("layer3.0.conv2" in k for k in layers) and any("layer4.0.conv2" in k for k in layers), layers
    keys = list(g64)
    assert sum(k.startswith(og.CNN_PREFIXES) for k in keys) >= 35
    assert _moved("stale forward copies", og.summed_grads(bad), g64, g32, keys) >= 3
