"""CPU: the numpy restatement of ``df_seg_batch`` (tests/seg_feed_np.py) against its own per-pixel form and against the properties the
contract states (include/dfusion.h, steps G1..G5), and the draw helpers of ``RenderedSegDataset`` that need no device."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_feed_np as sf  # noqa: E402

SIGMA5 = sf.noise_mul_of(5.0)


def frames(F=2, IH=9, IW=11, O=3, seed=0):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (F, IH, IW, 3), dtype=np.uint8)
    label = rng.integers(0, O + 1, (F, IH, IW)).astype(np.uint16)
    back = rng.integers(0, 256, (2, IH + 1, IW + 2, 3), dtype=np.uint8)
    return rgb, label, back


def equal(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_vectorised_equals_per_pixel():
    rgb, label, back = frames()
    label[1, 2, 3] = 7                                                         # above O
    desc = [[0, 0, 0, 0, 0, 0, 0, 11], [1, 4, 4, 1, 1, 5, 6, 0xFFFFFFFF], [0, 2, 1, 2, -1, 0, 0, 5], [1, 1, 3, 3, 0, 2, 2, 77]]
    cmap = [0, 2, 0, 1]
    for blur in (0, 1):
        for mul in (0, SIGMA5, 2 ** 31 - 1):
            a = sf.seg_batch(rgb, label, cmap, 3, desc, (5, 7), back, blur, mul)
            b = sf.seg_batch_slow(rgb, label, cmap, 3, desc, (5, 7), back, blur, mul)
            assert equal(a, b), (blur, mul)
    a = sf.seg_batch(rgb, label, cmap, 3, [d[:4] + [-1, 0, 0, d[7]] for d in desc], (5, 7), None, 1, SIGMA5)
    b = sf.seg_batch_slow(rgb, label, cmap, 3, [d[:4] + [-1, 0, 0, d[7]] for d in desc], (5, 7), None, 1, SIGMA5)
    assert equal(a, b)


def test_every_flip_is_np_flip_of_flip_0():
    rgb, label, back = frames(seed=1)
    row = [1, 3, 2, 0, 1, 1, 4, 1234]
    x0, t0, c0 = sf.seg_batch(rgb, label, [0, 1, 2, 3], 4, [row], (5, 7), back, 1, SIGMA5)
    for flip, axes in ((1, (2,)), (2, (1,)), (3, (1, 2))):
        x, t, c = sf.seg_batch(rgb, label, [0, 1, 2, 3], 4, [row[:3] + [flip] + row[4:]], (5, 7), back, 1, SIGMA5)
        assert np.array_equal(x, np.flip(x0, axes)) and np.array_equal(t, np.flip(t0, axes)) and np.array_equal(c, c0)
    assert not np.array_equal(x0, np.flip(x0, (2,)))


def test_blur_of_a_constant_window_is_the_identity():
    rgb = np.full((1, 9, 11, 3), 0, dtype=np.uint8)
    rgb[...] = (7, 130, 255)
    label = np.ones((1, 9, 11), dtype=np.uint16)
    a = sf.seg_batch(rgb, label, [0, 1], 2, [[0, 1, 2, 0, -1, 0, 0, 0]], (5, 7), None, 1, 0)
    b = sf.seg_batch(rgb, label, [0, 1], 2, [[0, 1, 2, 0, -1, 0, 0, 0]], (5, 7), None, 0, 0)
    assert equal(a, b)


@pytest.mark.parametrize("at, want", [
    ((2, 3), {(2, 3): 64, (1, 3): 32, (3, 3): 32, (2, 2): 32, (2, 4): 32, (1, 2): 16, (1, 4): 16, (3, 2): 16, (3, 4): 16}),      # interior
    # a corner: the clamped neighbours of (0, 0) are (0, 0) itself four times over (4 + 2 + 2 + 1), of (0, 1) and (1, 0) it twice
    ((0, 0), {(0, 0): 143, (0, 1): 48, (1, 0): 48, (1, 1): 16}),
    # an edge: row 0, column 3: own weight 4 + 2, side neighbours 2 + 1
    ((0, 3), {(0, 3): 96, (0, 2): 48, (0, 4): 48, (1, 3): 32, (1, 2): 16, (1, 4): 16}),
])
def test_blur_of_a_single_pixel(at, want):
    rgb = np.zeros((1, 5, 7, 3), dtype=np.uint8)
    rgb[0, at[0], at[1]] = 255
    label = np.ones((1, 5, 7), dtype=np.uint16)
    expect = np.zeros((5, 7), dtype=np.int64)
    for (i, j), v in want.items():
        expect[i, j] = v                                                       # (255 w + 8) >> 4: 64, 32, 16 for w = 4, 2, 1
    for fn in (sf.seg_batch, sf.seg_batch_slow):
        x, _, _ = fn(rgb, label, [0, 1], 2, [[0, 0, 0, 0, -1, 0, 0, 0]], (5, 7), None, 1, 0)
        assert np.array_equal(x[0], sf.normalise(np.repeat(expect[..., None], 3, axis=2)))
    assert (255 * 9 + 8) >> 4 == 143 and (255 * 6 + 8) >> 4 == 96 and (255 * 3 + 8) >> 4 == 48


def test_plain_item_is_the_loaders_normalisation():
    """no noise, no blur, no background: data_controller.py's own float32 expression on the same bytes, bit for bit"""
    from densefusion_amd.vanilla_segmentation.data_controller import MEAN, STD
    rgb, label, _ = frames(seed=2)
    x, t, _ = sf.seg_batch(rgb, label, [0, 1, 2, 3], 4, [[1, 2, 3, 0, -1, 0, 0, 9]], (5, 7), None, 0, 0)
    win = np.transpose(rgb[1, 2:7, 3:10], (2, 0, 1)).astype(np.float32)
    want = (win - MEAN[:, None, None]) / STD[:, None, None]
    assert want.dtype == np.float32
    assert np.array_equal(np.transpose(x[0, :, :, :3], (2, 0, 1)).view(np.uint32), want.view(np.uint32))
    assert not x[0, :, :, 3].any()
    assert np.array_equal(t[0], label[1, 2:7, 3:10].astype(np.int64))


def test_noise_statistics_at_sigma_5():
    """3 x 64 x 64 = 12288 draws on mid-grey, where no clamp is reached (|n| <= 131070 * noise_mul / 2^32 < 18).  n = floor(t + 1/2), t
    of standard deviation 5: Var n = 25 + 1/12, sd 5.0083.  The draws are hash values, taken as independent.  Standard error of the
    mean: 5.0083 / sqrt(12288) = 0.0452; of the sample sd at most the Gaussian sd / sqrt(2 N) = 0.0320 (the sum of four uniforms has
    less kurtosis than a Gaussian).  Bounds at five standard errors: |mean| < 0.226, |sd - 5| < 0.0083 + 0.160 = 0.168."""
    rgb = np.full((1, 64, 64, 3), 128, dtype=np.uint8)
    label = np.ones((1, 64, 64), dtype=np.uint16)
    x, _, _ = sf.seg_batch(rgb, label, [0, 1], 2, [[0, 0, 0, 0, -1, 0, 0, 20261019]], (64, 64), None, 0, SIGMA5)
    n = np.rint(x[0, :, :, :3].astype(np.float64) * sf.STD + sf.MEAN) - 128
    assert n.size == 12288 and np.abs(n).max() < 18
    print("mean", n.mean(), "sd", n.std())
    assert abs(n.mean()) < 0.226
    assert abs(n.std() - 5.0) < 0.168


def test_label_above_O_is_class_0():
    rgb, label, _ = frames(seed=3)
    label[0, 0, 0], label[0, 1, 1] = 4, 65535
    for fn in (sf.seg_batch, sf.seg_batch_slow):
        _, t, c = fn(rgb, label, [0, 1, 1, 1], 2, [[0, 0, 0, 0, -1, 0, 0, 0]], (5, 7), None, 0, 0)
        assert t[0, 0, 0] == 0 and t[0, 1, 1] == 0 and c[0].sum() == 35 and c[0, 1] == (t[0] == 1).sum()


@pytest.mark.parametrize("row", [[2, 0, 0, 0, -1, 0, 0, 1], [-1, 0, 0, 0, -1, 0, 0, 1], [0, 5, 0, 0, -1, 0, 0, 1], [0, 0, 5, 0, -1, 0, 0, 1],
                                 [0, -1, 0, 0, -1, 0, 0, 1], [0, 0, 0, 4, -1, 0, 0, 1], [0, 0, 0, -1, -1, 0, 0, 1], [0, 0, 0, 0, 2, 0, 0, 1],
                                 [0, 0, 0, 0, -2, 0, 0, 1], [0, 0, 0, 0, 0, 6, 0, 1], [0, 0, 0, 0, 0, 0, 7, 1], [0, 0, 0, 0, 0, 0, -1, 1]])
def test_bad_descriptor_gives_zeros(row):
    rgb, label, back = frames(seed=4)                                          # 2 frames of 9 x 11, 2 backgrounds of 10 x 13, window 5 x 7
    good = [1, 4, 4, 3, 1, 5, 6, 3]
    for fn in (sf.seg_batch, sf.seg_batch_slow):
        x, t, c = fn(rgb, label, [0, 1, 2, 3], 4, [good, row, good], (5, 7), back, 1, SIGMA5)
        assert not x[1].any() and not t[1].any() and not c[1].any()
        assert np.array_equal(x[0], x[2]) and x[0].any() and c[0].sum() == 35


# ---- the dataset's draw helpers (no device) -----------------------------------------------------------------------------------------
def test_draw_order_and_flip_mapping():
    from densefusion_amd.datasets import augment
    from densefusion_amd.datasets.customCAD import online_seg as og
    assert og.FLIP_OF_DRAW == (1, 2, 3, 0)                                     # SegDataset: 0 left-right, 1 up-down, 2 both, 3 none
    dims, win, pool = (40, 72), (32, 64), (3, 44, 80)
    for view in range(12):
        rng = random.Random("seg/%d/%d" % (5, view))
        plan = augment.plan_row(augment.ColorJitter(0.2, 0.2, 0.2, 0.05).draw(rng=rng))
        want = [rng.randint(0, 8), rng.randint(0, 8), og.FLIP_OF_DRAW[rng.randint(0, 3)], rng.randint(0, 2), rng.randint(0, 12), rng.randint(0, 16)]
        want.append(rng.getrandbits(32))
        got_plan, got = og.seg_draws(5, view, True, dims, win, pool)
        assert np.array_equal(got_plan, plan) and got == want
        # without a pool the three background draws are not made
        rng = random.Random("seg/%d/%d" % (5, view))
        augment.ColorJitter(0.2, 0.2, 0.2, 0.05).draw(rng=rng)
        want = [rng.randint(0, 8), rng.randint(0, 8), og.FLIP_OF_DRAW[rng.randint(0, 3)], -1, 0, 0]
        assert og.seg_draws(5, view, True, dims, win, None)[1] == want + [rng.getrandbits(32)]
        # without use_noise: no plan is drawn, the flip is drawn and dropped
        rng = random.Random("seg/%d/%d" % (5, view))
        want = [rng.randint(0, 8), rng.randint(0, 8), 0 * rng.randint(0, 3), rng.randint(0, 2), rng.randint(0, 12), rng.randint(0, 16)]
        got_plan, got = og.seg_draws(5, view, False, dims, win, pool)
        assert got_plan is None and got == want + [rng.getrandbits(32)]
    flips = {og.seg_draws(5, v, True, dims, win, pool)[1][2] for v in range(64)}
    assert flips == {0, 1, 2, 3}
    assert og.seg_draws(5, 3, True, dims, win, pool)[1] != og.seg_draws(6, 3, True, dims, win, pool)[1]


def test_window_validation():
    from densefusion_amd.datasets.customCAD import online_seg as og
    assert og.default_window((520, 1109)) == (512, 1088)
    assert og.check_window(None, (520, 1109)) == (512, 1088)
    assert og.check_window((32, 64), (40, 72)) == (32, 64)
    for bad in ((33, 64), (32, 50), (64, 64), (32, 96), (0, 64), (32, 0)):
        with pytest.raises(ValueError):
            og.check_window(bad, (40, 72))
    with pytest.raises(ValueError):
        og.check_window(None, (31, 72))
    assert og.noise_mul_of(5.0) == SIGMA5 and og.noise_mul_of(0.0) == 0


def test_background_directory_is_scaled_to_cover_and_centre_cropped(tmp_path):
    from PIL import Image
    from densefusion_amd.datasets.customCAD import online_seg as og
    wide = np.zeros((50, 100, 3), dtype=np.uint8)
    wide[:, :50], wide[:, 50:] = (10, 20, 30), (200, 210, 220)                 # scale 0.8 -> 40 x 80, columns 4..75 kept: the seam at 36
    tall = np.full((90, 36, 3), 77, dtype=np.uint8)                            # scale 2 -> 180 x 72, rows 70..109 kept
    Image.fromarray(wide).save(tmp_path / "b_wide.png")
    Image.fromarray(tall).save(tmp_path / "a_tall.png")
    (tmp_path / "notes.txt").write_text("not an image")
    pool = og.load_backgrounds(str(tmp_path), (40, 72))
    assert pool.dtype == np.uint8 and pool.shape == (2, 40, 72, 3)
    assert (pool[0] == 77).all(), "sorted by name: the tall image first"
    assert (pool[1][:, :34] == (10, 20, 30)).all() and (pool[1][:, 38:] == (200, 210, 220)).all()
    os.makedirs(tmp_path / "empty")
    with pytest.raises(ValueError):
        og.load_backgrounds(str(tmp_path / "empty"), (40, 72))
