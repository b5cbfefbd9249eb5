"""Power of the fp64 window tests (tests/test_train_window_fp64_gpu.py), on the CPU oracle alone: for each window fixture, leaving out the
gradient of the bucket with the fewest pixels moves every trunk, PSP and up-conv gradient by at least 3x that tensor's bound under the rule
of tests/oracle_grads.py.  A multi-bucket step that lost a chunk of buckets (a wrong table offset, an overwrite where it should
accumulate) loses at least that much, so the GPU tests would fail on it."""
import pytest

import oracle_grads as og


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
