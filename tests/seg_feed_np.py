"""numpy restatement of ``df_seg_batch`` (steps G1..G5 of its comment in include/dfusion.h), vectorised over an item's window, and a
second, per-pixel statement in plain Python integers written straight from the steps, which the host test holds it against.  Integer
arithmetic up to the normalisation, which is data_controller.py's own float32 expression."""
import numpy as np

from cad_sensor_np import C0, C1, M32, _mix32_int, mix32

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
NOISE_VARIANCE = 1431655765


def noise_mul_of(sigma):
    return int(np.rint(sigma * 2.0 ** 32 / np.sqrt(float(NOISE_VARIANCE))))


def desc_ok(row, F, IH, IW, H, W, NB, BH, BW):
    f, y0, x0, flip, b, by0, bx0, _ = [int(v) for v in row]
    if not 0 <= f < F or not 0 <= y0 <= IH - H or not 0 <= x0 <= IW - W or not 0 <= flip <= 3 or not -1 <= b < NB:
        return False
    return b < 0 or (0 <= by0 <= BH - H and 0 <= bx0 <= BW - W)


def _shapes(rgb, back):
    F, IH, IW, _ = rgb.shape
    NB, BH, BW = (0, 0, 0) if back is None else back.shape[:3]
    return F, IH, IW, NB, BH, BW


def _outputs(B, H, W, C):
    return np.zeros((B, H, W, 4), dtype=np.float32), np.zeros((B, H, W), dtype=np.int64), np.zeros((B, C), dtype=np.int32)


def normalise(v):
    """G5's value: v [H,W,3] integers 0..255 -> [H,W,4] float32, channel 3 zero"""
    out = np.zeros(v.shape[:2] + (4,), dtype=np.float32)
    out[..., :3] = (v.astype(np.float32) - MEAN) / STD
    return out


def blur_121(c):
    """G3 on composited values c [H,W,3] int64: indices clamped to the window"""
    H, W, _ = c.shape
    acc = np.zeros_like(c)
    for di, wi in ((-1, 1), (0, 2), (1, 1)):
        ii = np.clip(np.arange(H) + di, 0, H - 1)
        for dj, wj in ((-1, 1), (0, 2), (1, 1)):
            jj = np.clip(np.arange(W) + dj, 0, W - 1)
            acc += wi * wj * c[ii][:, jj]
    return (acc + 8) >> 4


def noise_field(seed, noise_mul, H, W):
    """G4's n for every (p, k): [H,W,3] int64"""
    q = np.arange(H * W * 3, dtype=np.uint32).reshape(H, W, 3)                   # 3p + k
    s = int(seed) & M32
    h0, h1 = mix32(s ^ C0, q).astype(np.int64), mix32(s ^ C1, q).astype(np.int64)
    S = (h0 & 0xFFFF) + (h0 >> 16) + (h1 & 0xFFFF) + (h1 >> 16) - 131070
    return (int(noise_mul) * S + (1 << 31)) >> 32                                 # numpy's >> on int64 floors


def seg_batch(rgb, label, class_map, C, desc, window, back=None, blur=1, noise_mul=0):
    """(x float32 [B,H,W,4], target int64 [B,H,W], counts int32 [B,C]) of rgb uint8 [F,IH,IW,3], label uint16 [F,IH,IW], class_map
    [O+1], desc [B,8], window (H, W), back None or uint8 [NB,BH,BW,3]"""
    F, IH, IW, NB, BH, BW = _shapes(rgb, back)
    H, W = window
    cmap = np.asarray(class_map, dtype=np.int64)
    O = len(cmap) - 1
    desc = np.asarray(desc).reshape(-1, 8)
    x, target, counts = _outputs(len(desc), H, W, C)
    for n, row in enumerate(desc):
        if not desc_ok(row, F, IH, IW, H, W, NB, BH, BW):
            continue
        f, y0, x0, flip, b, by0, bx0, seed = [int(v) for v in row]
        l = label[f, y0:y0 + H, x0:x0 + W].astype(np.int64)
        cls = np.where(l <= O, cmap[np.minimum(l, O)], 0)                         # G1
        counts[n] = np.bincount(cls.ravel(), minlength=C)
        c = rgb[f, y0:y0 + H, x0:x0 + W].astype(np.int64)                         # G2
        if b >= 0:
            c = np.where((l == 0)[..., None], back[b, by0:by0 + H, bx0:bx0 + W].astype(np.int64), c)
        v = blur_121(c) if blur else c                                            # G3
        if noise_mul > 0:                                                         # G4
            v = np.clip(v + noise_field(seed, noise_mul, H, W), 0, 255)
        xn = normalise(v)                                                         # G5
        if flip & 2:
            xn, cls = xn[::-1], cls[::-1]
        if flip & 1:
            xn, cls = xn[:, ::-1], cls[:, ::-1]
        x[n], target[n] = xn, cls
    return x, target, counts


# ---- the same rule pixel by pixel, in Python integers -------------------------------------------------------------------------------
def seg_batch_slow(rgb, label, class_map, C, desc, window, back=None, blur=1, noise_mul=0):
    F, IH, IW, NB, BH, BW = _shapes(rgb, back)
    H, W = window
    O = len(class_map) - 1
    desc = np.asarray(desc).reshape(-1, 8)
    x, target, counts = _outputs(len(desc), H, W, C)
    weights = ((1, 2, 1), (2, 4, 2), (1, 2, 1))
    for n, row in enumerate(desc):
        f, y0, x0, flip, b, by0, bx0, seed = [int(v) for v in row]
        seed &= M32
        if not (0 <= f < F and 0 <= y0 and y0 + H <= IH and 0 <= x0 and x0 + W <= IW and flip in (0, 1, 2, 3) and -1 <= b < NB):
            continue
        if b >= 0 and not (0 <= by0 and by0 + H <= BH and 0 <= bx0 and bx0 + W <= BW):
            continue

        def composite(i, j, k):
            if int(label[f, y0 + i, x0 + j]) == 0 and b >= 0:
                return int(back[b, by0 + i, bx0 + j, k])
            return int(rgb[f, y0 + i, x0 + j, k])

        for i in range(H):
            for j in range(W):
                p = i * W + j
                l = int(label[f, y0 + i, x0 + j])
                cls = int(class_map[l]) if l <= O else 0
                counts[n, cls] += 1
                i2 = H - 1 - i if flip & 2 else i
                j2 = W - 1 - j if flip & 1 else j
                for k in range(3):
                    if blur:
                        v = 8
                        for di in (-1, 0, 1):
                            for dj in (-1, 0, 1):
                                v += weights[di + 1][dj + 1] * composite(min(max(i + di, 0), H - 1), min(max(j + dj, 0), W - 1), k)
                        v >>= 4
                    else:
                        v = composite(i, j, k)
                    if noise_mul > 0:
                        h0, h1 = _mix32_int(seed ^ C0, 3 * p + k), _mix32_int(seed ^ C1, 3 * p + k)
                        S = (h0 & 0xFFFF) + (h0 >> 16) + (h1 & 0xFFFF) + (h1 >> 16) - 131070
                        v = min(max(v + (noise_mul * S + 2 ** 31) // 2 ** 32, 0), 255)
                    x[n, i2, j2, k] = (np.float32(v) - MEAN[k]) / STD[k]
                target[n, i2, j2] = cls
    return x, target, counts
