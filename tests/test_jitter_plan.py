"""CPU: the colour jitter cut into draws and pixel work (densefusion_amd/datasets/augment.py ``ColorJitter.draw`` / ``apply``), and the
numpy restatement of the pixel arithmetic (tests/jitter_np.py, what the device kernel is written from) held against PIL itself."""
import os
import random
import sys

import numpy as np
import pytest
from PIL import Image, ImageEnhance

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jitter_np  # noqa: E402
from densefusion_amd.datasets import augment  # noqa: E402

SETTINGS = [(0.2, 0.2, 0.2, 0.05), (0.0, 0.2, 0.2, 0.05), (0.2, 0.0, 0.2, 0.05), (0.2, 0.2, 0.0, 0.05), (0.2, 0.2, 0.2, 0.0)]


@pytest.mark.parametrize("setting", SETTINGS)
def test_draw_leaves_random_where_get_params_does(setting):
    cj = augment.ColorJitter(*setting)
    for seed in range(20):
        random.seed(seed)
        cj.get_params()
        want = random.getstate()
        random.seed(seed)
        plan = cj.draw()
        assert random.getstate() == want
        assert len(plan.order) == sum(1 for v in setting if v) and len(set(plan.order)) == len(plan.order)
        absent = [op for op, v in enumerate(setting) if not v]
        assert not set(absent) & set(plan.order)
        row = augment.plan_row(plan)
        assert row.dtype == np.float32 and row.shape == (8,) and list(row[4:4 + len(plan.order)]) == list(plan.order)
        assert all(v == augment.OP_NONE for v in row[4 + len(plan.order):])


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("mode", ["RGB", "RGBA"])
def test_apply_of_a_drawn_plan_is_the_call(setting, mode):
    rng = np.random.default_rng(5)
    img = Image.fromarray(rng.integers(0, 256, (31, 45, len(mode)), dtype=np.uint8), mode)
    cj = augment.ColorJitter(*setting)
    for seed in range(12):
        random.seed(seed)
        want = np.array(cj(img))
        random.seed(seed)
        got = np.array(cj.apply(img, cj.draw()))
        assert np.array_equal(got, want)
    assert np.array_equal(np.array(cj.apply(img, augment.IDENTITY_PLAN)), np.array(img))


def test_hue_shift_integer():
    assert augment.hue_shift(0.0) == 0
    assert augment.hue_shift(-0.05) == 244 and augment.hue_shift(0.05) == 12          # int() truncates toward zero: -12.75 -> -12
    assert augment.hue_shift(-0.001) == 0 and augment.hue_shift(0.0039) == 0 and augment.hue_shift(0.004) == 1
    assert augment.hue_shift(-0.5) == 129 and augment.hue_shift(0.5) == 127
    cj = augment.ColorJitter(0.0, 0.0, 0.0, 0.05)
    seen = set()
    for seed in range(200):
        random.seed(seed)
        f = random.uniform(-0.05, 0.05)
        random.seed(seed)
        plan = cj.draw()
        assert plan.hue_shift == int(f * 255) & 0xFF and plan.order == (augment.OP_HUE,)
        seen.add(plan.hue_shift)
    assert seen <= set(range(0, 13)) | set(range(244, 256)) and min(seen) == 0 and max(seen) == 255


def _cube_subset(stride_offset):
    """2^20 triples of the RGB cube: every 16th, from an offset that walks all residues of the three channels."""
    i = np.arange(1 << 20, dtype=np.int64)
    idx = i * 16 + (i + stride_offset * (i >> 4)) % 16
    return np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255], axis=-1).astype(np.uint8)


def test_numpy_hsv_conversions_equal_pil_on_a_strided_cube():
    triples = _cube_subset(7)
    assert len(np.unique(triples[:, 2])) == 256 and len(np.unique(triples[:, 0])) == 256
    for lo in range(0, len(triples), 1 << 17):                       # chunks: the float64 temporaries of the whole set are large
        chunk = triples[lo:lo + (1 << 17)].reshape(256, -1, 3)
        want = np.array(Image.fromarray(chunk, "RGB").convert("HSV"))
        assert np.array_equal(jitter_np.rgb_to_hsv(chunk), want)
        want = np.array(Image.fromarray(chunk, "HSV").convert("RGB"))          # the same triples read as H, S, V
        assert np.array_equal(jitter_np.hsv_to_rgb(chunk), want)


def test_numpy_enhancers_equal_pil_at_random_factors():
    rng = np.random.default_rng(11)
    arr = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    img = Image.fromarray(arr, "RGB")
    assert np.array_equal(jitter_np.luma(arr), np.array(img.convert("L")))
    for f in list(rng.uniform(0.8, 1.2, 50)) + [1.0, 0.8, 1.2]:
        a = np.float32(f)
        assert np.array_equal(jitter_np.brightness(arr, a), np.array(ImageEnhance.Brightness(img).enhance(float(f))))
        assert np.array_equal(jitter_np.contrast(arr, a), np.array(ImageEnhance.Contrast(img).enhance(float(f))))
        assert np.array_equal(jitter_np.saturation(arr, a), np.array(ImageEnhance.Color(img).enhance(float(f))))


def test_numpy_jitter_equals_apply():
    rng = np.random.default_rng(3)
    arr = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    cj = augment.ColorJitter(0.2, 0.2, 0.2, 0.05)
    for seed in range(30):
        random.seed(seed)
        plan = cj.draw()
        want = np.array(cj.apply(Image.fromarray(arr, "RGB"), plan))
        assert np.array_equal(jitter_np.jitter(arr, augment.plan_row(plan)), want), plan


def test_deferred_jitter_hands_over_what_the_host_would_jitter():
    """``defer_jitter`` (the host half of jitter="device"): RGB and RGBA frames go up raw with their plan -- the colour planes of an RGBA
    frame come out of the host jitter exactly like those of the RGB frame without alpha --, other modes are jittered here."""
    rng = np.random.default_rng(8)
    rgba = rng.integers(0, 256, (29, 31, 4), dtype=np.uint8)
    cj = augment.ColorJitter(0.2, 0.2, 0.2, 0.05)
    for seed in range(24):
        for img in (Image.fromarray(rgba, "RGBA"), Image.fromarray(rgba[:, :, :3].copy(), "RGB")):
            random.seed(seed)
            want = np.array(cj(img))[:, :, :3]
            state = random.getstate()
            random.seed(seed)
            up, row = augment.defer_jitter(cj, img)
            assert random.getstate() == state and up.mode == "RGB" and np.array_equal(np.array(up), rgba[:, :, :3])
            assert np.array_equal(jitter_np.jitter(np.array(up), row), want)
    grey = Image.fromarray(rgba[:, :, 0].copy(), "L")
    random.seed(1)
    want = np.array(cj(grey))
    random.seed(1)
    up, row = augment.defer_jitter(cj, grey)
    assert np.array_equal(np.array(up), want) and np.array_equal(row, augment.plan_row(augment.IDENTITY_PLAN))
