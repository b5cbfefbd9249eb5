"""GPU: df_color_jitter / df_compose_frame (densefusion_amd/csrc/augment.hip) against the host path itself.  The oracle of the jitter is
``augment.ColorJitter.apply`` -- PIL -- and equality is exact: same plan, same bytes."""
import itertools

import numpy as np
import pytest
from PIL import Image

from densefusion_amd.datasets import augment

pytestmark = pytest.mark.gpu

B, C, S, HUE = augment.OP_BRIGHTNESS, augment.OP_CONTRAST, augment.OP_SATURATION, augment.OP_HUE


@pytest.fixture(scope="module")
def pp():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from densefusion_amd.lib import preprocess
    return preprocess


def _plan(rng, order, b=None, c=None, s=None, shift=None):
    f = lambda v: np.float32(rng.uniform(0.8, 1.2) if v is None else v)
    return augment.JitterPlan(f(b), f(c), f(s), int(rng.choice([*range(0, 13), *range(244, 256)])) if shift is None else shift, tuple(order))


def _host(arr, plan):
    return np.array(augment.ColorJitter.apply(Image.fromarray(arr, "RGB"), plan))


def _device(pp, frames, plans, inplace=False):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    rows = np.stack([augment.plan_row(p) for p in plans])
    out = pp.color_jitter(d, rows, out=d if inplace else None)
    assert (out.data_ptr() == d.data_ptr()) == inplace
    return out.cpu().numpy()


def _report(got, want, what):
    bad = int((got != want).any(axis=-1).sum())
    print(f"{what}: {bad} of {want[..., 0].size} pixels differ")
    return bad


def test_every_order(pp):
    rng = np.random.default_rng(1)
    arr = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)            # 1961 pixels: a one-pixel tail, rows off the dword grid
    orders = list(itertools.permutations((B, C, S, HUE)))
    assert len(orders) == 24
    plans = [_plan(rng, o) for o in orders]
    bad = [o for o, p in zip(orders, plans) if _report(_device(pp, arr[None], [p])[0], _host(arr, p), f"order {o}")]
    assert not bad
    # all of them as ONE call too: 37*53*3 bytes per frame is odd, so three frames in four start off the dword grid (byte-wise walk)
    got = _device(pp, np.stack([arr] * 24), plans)
    assert not [o for k, (o, p) in enumerate(zip(orders, plans)) if _report(got[k], _host(arr, p), f"batched order {o}")]


def test_shorter_orders_and_the_empty_plan(pp):
    rng = np.random.default_rng(2)
    arr = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)              # fewer than one workgroup, two tail pixels
    for order in [(), (C,), (HUE, B), (S, C, B)]:
        p = _plan(rng, order)
        assert np.array_equal(_device(pp, arr[None], [p])[0], _host(arr, p)), order
    assert np.array_equal(_device(pp, arr[None], [augment.IDENTITY_PLAN])[0], arr)


def test_batching_and_in_place(pp):
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (5, 40, 40, 3), dtype=np.uint8)
    orders = [(C, B, S, HUE), (HUE, S, B, C), (B, S, HUE), (S, C, HUE, B), (B, HUE, C, S)]      # one frame without contrast
    plans = [_plan(rng, o) for o in orders]
    solo = np.stack([_device(pp, frames[k][None], [plans[k]])[0] for k in range(5)])
    assert np.array_equal(solo, np.stack([_host(frames[k], plans[k]) for k in range(5)]))
    assert np.array_equal(_device(pp, frames, plans), solo)
    assert np.array_equal(_device(pp, frames, plans, inplace=True), solo)


def test_random_factors_no_contraction(pp):
    """A fused multiply-add in the blend rounds once where PIL rounds twice: it shows on a small share of pixels, at some factors."""
    rng = np.random.default_rng(4)
    arr = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    n = 200
    plans = [_plan(rng, (B, C, S)[k % 3:] + (B, C, S)[:k % 3], shift=0) for k in range(n)]
    got = _device(pp, np.stack([arr] * n), plans)
    bad = sum(1 for k in range(n) if _report(got[k], _host(arr, plans[k]), f"factors {plans[k][:3]}"))
    assert bad == 0
    for op in (B, C, S):                                                      # each enhancer alone, 40 factors
        plans = [_plan(rng, (op,)) for _ in range(40)]
        got = _device(pp, np.stack([arr] * 40), plans)
        assert all(np.array_equal(got[k], _host(arr, plans[k])) for k in range(40)), op


def _frame_with_l_sum(total):
    """A 2x8 grey frame (L of grey v is v) whose 16 values add up to `total`."""
    vals = np.full(16, total // 16, dtype=np.int64)
    vals[:total - int(vals.sum())] += 1
    assert vals.sum() == total and vals.max() <= 255
    g = vals.astype(np.uint8).reshape(2, 8)
    return np.stack([g, g, g], axis=-1)


@pytest.mark.parametrize("order", [(C, B, S, HUE), (B, S, HUE, C)], ids=["contrast_first", "contrast_last"])
def test_contrast_mean_rounding(pp, order):
    rng = np.random.default_rng(5)
    # mean L exactly 100.5 (sum 1608 of 16) rounds up to 101; sum 1607 (100.4375) rounds down to 100
    for total, want_mean in ((1608, 101), (1607, 100)):
        arr = _frame_with_l_sum(total)
        assert int(np.array(Image.fromarray(arr, "RGB").convert("L")).astype(np.int64).sum()) == total
        for _ in range(6):
            # contrast first: brightness / saturation / hue follow.  Contrast last: they come first and move the mean (a grey frame
            # stays grey through saturation and hue, brightness scales it), so the mean that counts is the one after them
            p = _plan(rng, order, c=0.5)
            want = _host(arr, p)
            assert np.array_equal(_device(pp, arr[None], [p])[0], want), (total, p)
        if order[0] == C:                                                    # the rounding is visible: with alpha 0 the frame IS the mean
            p = augment.JitterPlan(np.float32(1), np.float32(0), np.float32(1), 0, (C,))
            got = _device(pp, arr[None], [p])[0]
            assert np.array_equal(got, _host(arr, p)) and (got == want_mean).all()
    if order[-1] == C:
        # contrast last, a mean that falls on k + 0.5 only AFTER brightness: 16 values of 201 at alpha 0.5 -> 100 each; half of them 203 -> 101
        g = np.array([201] * 8 + [203] * 8, dtype=np.uint8).reshape(2, 8)
        arr = np.stack([g, g, g], axis=-1)
        p = augment.JitterPlan(np.float32(0.5), np.float32(0), np.float32(1), 0, (B, C))
        got = _device(pp, arr[None], [p])[0]
        assert np.array_equal(got, _host(arr, p)) and (got == 101).all()       # mean of 8 x 100 and 8 x 101 = 100.5 -> 101


def test_hue_over_the_whole_rgb_cube(pp):
    import torch
    idx = np.arange(1 << 24, dtype=np.uint32)
    cube = np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
    img = Image.fromarray(cube, "RGB")
    d = torch.from_numpy(cube).cuda()[None]
    for factor, shift in ((0.05, 12), (-0.05, 244)):
        assert augment.hue_shift(factor) == shift
        want = np.array(augment.adjust_hue(img, factor))
        got = pp.color_jitter(d, augment.plan_row(augment.JitterPlan(np.float32(1), np.float32(1), np.float32(1), shift, (HUE,)))[None])[0].cpu().numpy()
        assert _report(got, want, f"hue shift {shift} over 2^24 triples") == 0


def test_clamping_and_identity(pp):
    rng = np.random.default_rng(6)
    one = np.float32(1)
    bright = rng.integers(230, 256, (16, 20, 3), dtype=np.uint8)
    p = augment.JitterPlan(np.float32(1.2), one, one, 0, (B,))
    got = _device(pp, bright[None], [p])[0]
    assert np.array_equal(got, _host(bright, p)) and (got == 255).all()
    prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [255, 255, 255], [0, 0, 0]], dtype=np.uint8)
    prim = np.ascontiguousarray(np.broadcast_to(prim[None], (3, 8, 3)))
    p = augment.JitterPlan(one, one, np.float32(1.2), 0, (S,))
    got = _device(pp, prim[None], [p])[0]
    assert np.array_equal(got, _host(prim, p)) and got.min() == 0 and got.max() == 255 and np.array_equal(got, prim)
    p = augment.JitterPlan(one, one, np.float32(0.8), 0, (S,))
    assert np.array_equal(_device(pp, prim[None], [p])[0], _host(prim, p))
    arr = rng.integers(0, 256, (24, 24, 3), dtype=np.uint8)
    for op in (B, C, S):                                                      # factor exactly 1.0: the identity
        p = augment.JitterPlan(one, one, one, 0, (op,))
        got = _device(pp, arr[None], [p])[0]
        assert np.array_equal(got, arr) and np.array_equal(got, _host(arr, p))


def test_argument_errors(pp):
    import torch
    d = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        pp.color_jitter(d.cpu(), np.zeros((1, 8), np.float32))
    with pytest.raises(RuntimeError):
        pp.color_jitter(d, np.zeros((2, 8), np.float32))
    with pytest.raises(RuntimeError):
        pp.compose_frame(d[0], back=d[0])


@pytest.mark.parametrize("shape", [(37, 53), (480, 640)])
@pytest.mark.parametrize("layers", ["both", "back", "front", "none"])
def test_composition(pp, shape, layers):
    import torch
    rng = np.random.default_rng(7)
    H, W = shape
    rgb, back, front = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(3))
    mask_back, mask_front = rng.random((H, W)) < 0.5, rng.random((H, W)) < 0.7
    want = rgb
    if layers in ("both", "back"):
        want = back * mask_back[:, :, None] + want                         # uint8 arithmetic, wrap-around included (datasets/ycb/dataset.py)
        wide = back.astype(np.int32) * mask_back[:, :, None] + rgb
        assert (wide > 255).any() and (wide <= 255).any() and want.dtype == np.uint8
    if layers in ("both", "front"):
        want = want * mask_front[:, :, None] + front * ~mask_front[:, :, None]
    assert mask_back.any() and not mask_back.all() and mask_front.any() and not mask_front.all()
    up = lambda a: torch.from_numpy(a).cuda()
    kw = {}
    if layers in ("both", "back"):
        kw.update(back=up(back), mask_back=up(mask_back.astype(np.uint8) * 255 if H == 37 else mask_back))       # any non-zero byte / bool
    if layers in ("both", "front"):
        kw.update(front=up(front), mask_front=up(mask_front))
    d = up(rgb.copy())
    out = pp.compose_frame(d, **kw)
    assert out.data_ptr() == d.data_ptr()
    assert _report(out.cpu().numpy(), want, f"composition {layers} {shape}") == 0
