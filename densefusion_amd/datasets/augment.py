"""Training-time augmentation of the two disk datasets (datasets/ycb/dataset.py:84,117-136,149-167,196-221;
datasets/linemod/dataset.py:83,114-115,132,159-160,178-180): colour jitter, pose-translation noise and -- YCB only -- synthetic
frames pasted over real backgrounds with occluders from other synthetic frames.

``ColorJitter`` restates ``torchvision.transforms.ColorJitter`` of torchvision 0.2.2.post3 (the reference's pin, Dockerfile:27; the
package is not part of this build): four factors drawn with Python's ``random.uniform`` in the order brightness, contrast,
saturation, hue, the four operations applied in an order given by ``random.shuffle``; brightness / contrast / saturation are PIL's
``ImageEnhance.Brightness / Contrast / Color``, hue adds ``uint8(hue_factor * 255)`` to the H plane of the HSV image with 8-bit
wrap-around.  Same draws from the same ``random`` state, same PIL calls; parity with torchvision itself is unpinned (it cannot be
imported here).  Everything in this file runs on the host, in the loader's worker processes.

``ColorJitter.draw()`` / ``apply()`` cut a jitter into its random draws (a ``JitterPlan``) and the pixel work: the draws stay on the
host and on Python's ``random`` stream, the pixel work runs either here (``apply``: PIL) or on the device (``df_color_jitter``,
lib/preprocess.py ``color_jitter``, fed ``plan_row(plan)``) with identical results.
"""
from __future__ import annotations

import random
from typing import NamedTuple

import numpy as np
from PIL import Image, ImageEnhance


OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE, OP_NONE = 0, 1, 2, 3, 4      # op codes of a plan row (include/dfusion.h, df_color_jitter)


def hue_shift(hue_factor):
    """The 8-bit amount ``adjust_hue`` adds to the H plane: Python's int() truncates toward zero, so -0.05 -> -12 -> 244."""
    return int(hue_factor * 255) & 0xFF


def shift_hue(img, shift):
    mode = img.mode
    if mode in ("L", "1", "I", "F"):
        return img
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    np_h = (np_h.astype(np.int32) + shift).astype(np.uint8)      # uint8 addition: wraps across the boundary
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert(mode)


def adjust_hue(img, hue_factor):
    if not -0.5 <= hue_factor <= 0.5:
        raise ValueError("hue_factor is not in [-0.5, 0.5].")
    return shift_hue(img, hue_shift(hue_factor))


class JitterPlan(NamedTuple):
    """One jitter's draws.  The alphas are what PIL's blend computes with (its C float); an absent operation has alpha 1 / shift 0
    and is missing from ``order``."""
    brightness: np.float32
    contrast: np.float32
    saturation: np.float32
    hue_shift: int
    order: tuple                  # op codes in application order


IDENTITY_PLAN = JitterPlan(np.float32(1.0), np.float32(1.0), np.float32(1.0), 0, ())


def plan_row(plan):
    """The plan as the 8 floats df_color_jitter reads: three alphas, the hue shift, four op codes (OP_NONE fills the unused slots)."""
    order = list(plan.order) + [OP_NONE] * (4 - len(plan.order))
    return np.array([plan.brightness, plan.contrast, plan.saturation, plan.hue_shift] + order, dtype=np.float32)


class ColorJitter:
    def __init__(self, brightness=0.0, contrast=0.0, saturation=0.0, hue=0.0):
        self.brightness = (max(0.0, 1.0 - brightness), 1.0 + brightness) if brightness else None
        self.contrast = (max(0.0, 1.0 - contrast), 1.0 + contrast) if contrast else None
        self.saturation = (max(0.0, 1.0 - saturation), 1.0 + saturation) if saturation else None
        self.hue = (-hue, hue) if hue else None

    def get_params(self):
        ops = []
        if self.brightness is not None:
            f = random.uniform(*self.brightness)
            ops.append(lambda im, f=f: ImageEnhance.Brightness(im).enhance(f))
        if self.contrast is not None:
            f = random.uniform(*self.contrast)
            ops.append(lambda im, f=f: ImageEnhance.Contrast(im).enhance(f))
        if self.saturation is not None:
            f = random.uniform(*self.saturation)
            ops.append(lambda im, f=f: ImageEnhance.Color(im).enhance(f))
        if self.hue is not None:
            f = random.uniform(*self.hue)
            ops.append(lambda im, f=f: adjust_hue(im, f))
        random.shuffle(ops)
        return ops

    def __call__(self, img):
        for op in self.get_params():
            img = op(img)
        return img

    def draw(self, rng=random):
        """The draws of ``get_params()`` as a plan: the same ``random.uniform`` calls in the same order, then ``random.shuffle`` on a
        list of as many op codes (its consumption depends on the length only), so ``random`` is left in the state ``get_params()``
        leaves it in.  ``rng``: a ``random.Random`` to draw from instead of the module's global stream."""
        alpha, shift, ops = [np.float32(1.0)] * 3, 0, []
        for k, span in enumerate((self.brightness, self.contrast, self.saturation)):
            if span is not None:
                alpha[k] = np.float32(rng.uniform(*span))
                ops.append(k)
        if self.hue is not None:
            shift = hue_shift(rng.uniform(*self.hue))
            ops.append(OP_HUE)
        rng.shuffle(ops)
        return JitterPlan(alpha[0], alpha[1], alpha[2], shift, tuple(ops))

    @staticmethod
    def apply(img, plan):
        """The plan applied on the host with PIL: ``self(img)`` is ``apply(img, self.draw())``."""
        for op in plan.order:
            if op == OP_BRIGHTNESS:
                img = ImageEnhance.Brightness(img).enhance(float(plan.brightness))
            elif op == OP_CONTRAST:
                img = ImageEnhance.Contrast(img).enhance(float(plan.contrast))
            elif op == OP_SATURATION:
                img = ImageEnhance.Color(img).enhance(float(plan.saturation))
            elif op == OP_HUE:
                img = shift_hue(img, plan.hue_shift)
        return img


def defer_jitter(trancolor, img):
    """The host half of a jitter whose pixel work runs on the device: draws the plan (Python's ``random`` advances exactly as under
    ``trancolor(img)``) and returns (the image to upload, its plan row).  RGB goes up as it is and RGBA without its alpha plane (the
    enhancers and the hue shift treat the colour planes of both alike, and the loaders drop alpha anyway); any other mode is jittered
    here with PIL and goes up with the identity plan."""
    plan = trancolor.draw()
    if img.mode == "RGBA":
        img = img.convert("RGB")
    if img.mode != "RGB":
        return trancolor.apply(img, plan), plan_row(IDENTITY_PLAN)
    return img, plan_row(plan)


def occluder_mask(f_label, front_num=2):
    """datasets/ycb/dataset.py:122-132: `front_num` objects drawn from a synthetic frame's label image; returns the boolean mask that is
    False on those objects' pixels (None when the frame shows fewer objects)."""
    front_label = np.unique(f_label).tolist()[1:]
    if len(front_label) < front_num:
        return None
    keep = np.ones(f_label.shape, dtype=bool)
    for f_i in random.sample(front_label, front_num):
        keep &= f_label != f_i
    return keep
