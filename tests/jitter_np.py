"""The colour jitter's per-pixel arithmetic restated in numpy: the specification df_color_jitter (densefusion_amd/csrc/augment.hip)
is written from, held against PIL by tests/test_jitter_plan.py.  Every step is 8-bit or plain IEEE arithmetic; each operation's
output is uint8 before the next one starts."""
import numpy as np

OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3


def luma(rgb):
    """PIL's convert("L") of uint8 [...,3]."""
    c = rgb.astype(np.uint32)
    return ((c[..., 0] * 19595 + c[..., 1] * 38470 + c[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(d, alpha, x):
    """PIL's Image.blend(degenerate, image, alpha) per channel value: d + alpha * (x - d) in fp32 (a product, then a sum: no fused
    multiply-add), clamped to [0, 255], truncated."""
    a = np.float32(alpha)
    d, x = np.asarray(d, dtype=np.float32), np.asarray(x, dtype=np.float32)
    t = d + a * (x - d)
    return np.clip(t, np.float32(0), np.float32(255)).astype(np.uint8)


def brightness(rgb, alpha):
    return blend(np.float32(0), alpha, rgb)


def contrast_mean(rgb):
    """int(mean(L) + 0.5) over the whole frame, in integers."""
    lum = luma(rgb)
    s, n = int(lum.astype(np.int64).sum()), lum.size
    return (2 * s + n) // (2 * n)


def contrast(rgb, alpha):
    return blend(np.float32(contrast_mean(rgb)), alpha, rgb)


def saturation(rgb, alpha):
    return blend(luma(rgb)[..., None], alpha, rgb)


def rgb_to_hsv(rgb):
    """PIL's convert("HSV") of uint8 [...,3]."""
    r, g, b = (rgb[..., k].astype(np.float32) for k in range(3))
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    grey = maxc == minc
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = maxc - minc
        s = cr / maxc
        rc, gc, bc = (maxc - r) / cr, (maxc - g) / cr, (maxc - b) / cr
        h = np.where(r == maxc, bc - gc,
                     np.where(g == maxc, (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(np.float32),
                              (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(np.float32)))
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
        hi = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
        si = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    out = np.empty(rgb.shape, dtype=np.uint8)
    out[..., 0] = np.where(grey, 0, hi)
    out[..., 1] = np.where(grey, 0, si)
    out[..., 2] = rgb.max(axis=-1)
    return out


def hsv_to_rgb(hsv):
    """PIL's conversion of an "HSV" image (uint8 [...,3]) to "RGB"."""
    h, s, v = (hsv[..., k].astype(np.float64) for k in range(3))
    hh = h * 6.0 / 255.0
    i = np.floor(hh)
    f = hh - i
    fs = s / 255.0
    p = np.clip(np.round(v * (1.0 - fs)), 0, 255)
    q = np.clip(np.round(v * (1.0 - fs * f)), 0, 255)
    t = np.clip(np.round(v * (1.0 - fs * (1.0 - f))), 0, 255)
    sel = i.astype(np.int64) % 6
    table = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))
    out = np.empty(hsv.shape, dtype=np.uint8)
    for k in range(3):
        out[..., k] = np.where(hsv[..., 1] == 0, v, np.select([sel == j for j in range(6)], [table[j][k] for j in range(6)])).astype(np.uint8)
    return out


def hue(rgb, shift):
    hsv = rgb_to_hsv(rgb)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + int(shift)) & 0xFF).astype(np.uint8)
    return hsv_to_rgb(hsv)


def jitter(rgb, row):
    """A whole plan row (augment.plan_row: three alphas, the hue shift, four op codes) applied to uint8 [H,W,3]."""
    for op in (int(v) for v in row[4:8]):
        if op == OP_BRIGHTNESS:
            rgb = brightness(rgb, row[0])
        elif op == OP_CONTRAST:
            rgb = contrast(rgb, row[1])
        elif op == OP_SATURATION:
            rgb = saturation(rgb, row[2])
        elif op == OP_HUE:
            rgb = hue(rgb, int(row[3]))
    return rgb
