"""Power of the fp64 window tests (tests/test_train_window_fp64_gpu.py), on the CPU oracle alone: for each window fixture, leaving out the
gradient of the bucket with the fewest pixels moves every trunk, PSP and up-conv gradient by at least 3x that tensor's bound under the rule
of tests/oracle_grads.py.  A multi-bucket step that lost a chunk of buckets (a wrong table offset, an overwrite where it should
accumulate) loses at least that much, so the GPU tests would fail on it.  For the windows of the smallest crops: a pyramid pooling adjoint that
misses the bins of a map narrower than they are moves every trunk gradient by at least 3x its bound."""
from unittest import mock

import pytest
import torch
import torch.nn.functional as F

import oracle_grads as og
from oracle import dfnet


@pytest.mark.parametrize("name", sorted(og.WINDOWS))
def test_losing_the_smallest_bucket_fails_the_bound(name):
    K, N, M, sd, objs = og.window(name)
    r64, r32 = og.posenet_oracle(sd, objs)             # also asserts the fixture is well-conditioned (same 1-NN / argmax in fp32 and fp64)
    buckets = {}
    for i, o in enumerate(objs):
        buckets.setdefault(o["img"].shape[1:], []).append(i)
    smallest = min(buckets.values(), key=lambda ix: sum(objs[i]["img"][0].size for i in ix))
    g64, g32 = og.summed_grads(r64), og.summed_grads(r32)
    lost = og.summed_grads(r64, skip=set(smallest))
    keys = [k for k in g64 if k.startswith(og.CNN_PREFIXES)]
    assert len(keys) >= 35
    worst, where = float("inf"), ""
    for k in keys:
        bound = max(og.C * og.rel_l2(g32[k], g64[k]), og.gpu_floor(k)[0])
        dev = og.rel_l2(lost[k], g64[k])
        assert dev >= 3 * bound, f"{name}: {k}: dropping bucket {smallest} moves the gradient by {dev:.2e}, bound {bound:.2e}"
        if dev / bound < worst:
            worst, where = dev / bound, k
    print(f"{name}: dropping the smallest bucket moves every CNN gradient by >= {worst:.1f}x its bound ({where})")


def test_the_bound_rule_accepts_the_fp32_reference_and_rejects_a_lost_frame():
    """The rule itself: the fp32 reference passes against fp64, a gradient missing one frame does not."""
    K, N, M, sd, objs = og.window("mixed5")
    r64, r32 = og.posenet_oracle(sd, objs[:2])
    g64, g32 = og.summed_grads(r64), og.summed_grads(r32)
    for k in g64:
        og.check(k, g32[k], g64[k], g32[k], floor=og.gpu_floor(k))
    k = "cnn.model.module.feats.layer3.1.conv2.weight"
    with pytest.raises(AssertionError, match="relative L2"):
        og.check(k, og.summed_grads(r64, skip={1})[k], g64[k], g32[k], floor=og.gpu_floor(k))


# ---- the pyramid pooling adjoint on maps narrower than its bins ----
class _ThreeCandidatePool(torch.autograd.Function):
    """AdaptiveAvgPool2d whose adjoint looks for the bins of a pixel among yy * s // H - 1 .. + 1 only: the rule pool_bwd_all_kernel
    (csrc/train.hip) had, complete only for maps of at least s / 2 pixels per side."""

    @staticmethod
    def forward(ctx, x, s):
        ctx.s, ctx.hw = s, tuple(x.shape[2:])
        return _POOL(x, (s, s))

    @staticmethod
    def backward(ctx, g):
        s, (H, W) = ctx.s, ctx.hw
        dx = g.new_zeros(g.shape[0], g.shape[1], H, W)

        def bins(p, L):
            for b in range(max(0, p * s // L - 1), min(s - 1, p * s // L + 1) + 1):
                lo, hi = b * L // s, ((b + 1) * L + s - 1) // s
                if lo <= p < hi:
                    yield b, hi - lo

        for yy in range(H):
            for bi, ny in bins(yy, H):
                for xx in range(W):
                    for bj, nx in bins(xx, W):
                        dx[:, :, yy, xx] += g[:, :, bi, bj] / (ny * nx)
        return dx, None


_POOL = F.adaptive_avg_pool2d


@pytest.mark.parametrize("name", ["ones3", "tiny11"])
def test_a_pooling_adjoint_that_misses_bins_fails_the_bound(name):
    """The tiny windows are there for the pyramid's pooling adjoint: with the three-candidate rule in the fp64 oracle, every trunk weight
    gradient of the window moves by at least 3x its bound (the windows of 5 x 5 maps and more are blind to it: the rule is complete there)."""
    K, N, M, sd, objs = og.window(name)
    r64, r32 = og.posenet_oracle(sd, objs)
    if name == "ones3":        # three frames do not dilute a flipped ReLU of the point layers: the fixture keeps its distance from zero
        assert og.point_relu_margin(sd, objs, r64) >= og.RELU_MARGIN
    g64, g32 = og.summed_grads(r64), og.summed_grads(r32)
    with mock.patch.object(dfnet.F, "adaptive_avg_pool2d", lambda x, size: _ThreeCandidatePool.apply(x, size[0])):
        bad = og.summed_grads(og.posenet_frames(sd, objs, torch.float64))
    keys = [k for k in g64 if k.startswith("cnn.model.module.feats.")]
    assert len(keys) >= 17
    worst, where = float("inf"), ""
    for k in keys:
        bound = max(og.C * og.rel_l2(g32[k], g64[k]), og.gpu_floor(k)[0])
        dev = og.rel_l2(bad[k], g64[k])
        assert dev >= 3 * bound, f"{name}: {k}: the missed bins move the gradient by {dev:.2e}, bound {bound:.2e}"
        if dev / bound < worst:
            worst, where = dev / bound, k
    print(f"{name}: the three-candidate pooling adjoint moves every trunk gradient by >= {worst:.1f}x its bound ({where})")
