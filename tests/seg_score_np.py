"""numpy restatement of ``df_seg_score`` (steps S1..S3 of its comment in include/dfusion.h) and ``df_seg_masks`` (M1), each written twice:
vectorised, and pixel by pixel in Python integers.  The arg-max is stated by hand (first maximum wins, NaN counts as maximal), not
through ``np.argmax``, so the GPU tests can pin it against ``torch.argmax`` from two sides."""
import math

import numpy as np


def argmax_first(logits, C):
    """logits [..., ld] float32 -> int32 [...]: S1 over the first C channels, one running best per pixel, channel by channel."""
    x = np.asarray(logits, dtype=np.float32)
    best = x[..., 0].copy()
    bi = np.zeros(x.shape[:-1], dtype=np.int32)
    for c in range(1, C):
        v = x[..., c]
        take = (v > best) | (np.isnan(v) & ~np.isnan(best))
        best = np.where(take, v, best)
        bi = np.where(take, np.int32(c), bi)
    return bi


def seg_score(logits, target, C):
    """logits [F,H,W,ld] float32, target [F,H,W] int64 -> (conf [F,C,C] int32, skipped [F] int32, label [F,H,W] int32), vectorised."""
    logits, target = np.asarray(logits, dtype=np.float32), np.asarray(target, dtype=np.int64)
    F = logits.shape[0]
    label = argmax_first(logits, C)
    conf, skipped = np.zeros((F, C, C), dtype=np.int32), np.zeros(F, dtype=np.int32)
    for f in range(F):
        ok = (target[f] >= 0) & (target[f] < C)
        cells = target[f][ok] * C + label[f][ok]
        conf[f] = np.bincount(cells, minlength=C * C).reshape(C, C).astype(np.int32)
        skipped[f] = int((~ok).sum())
    return conf, skipped, label


def seg_score_pixels(logits, target, C):
    """The same, pixel by pixel in Python numbers."""
    logits, target = np.asarray(logits, dtype=np.float32), np.asarray(target, dtype=np.int64)
    F, H, W, _ = logits.shape
    conf = [[[0] * C for _ in range(C)] for _ in range(F)]
    skipped, label = [0] * F, np.zeros((F, H, W), dtype=np.int32)
    for f in range(F):
        for i in range(H):
            for j in range(W):
                row = [float(v) for v in logits[f, i, j, :C]]
                best, bi = row[0], 0
                for c in range(1, C):
                    if row[c] > best or (math.isnan(row[c]) and not math.isnan(best)):
                        best, bi = row[c], c
                label[f, i, j] = bi
                t = int(target[f, i, j])
                if 0 <= t < C:
                    conf[f][t][bi] += 1
                else:
                    skipped[f] += 1
    return np.array(conf, dtype=np.int32).reshape(F, C, C), np.array(skipped, dtype=np.int32), label


def seg_masks(label, win, pairs, image_dims):
    """label [F,H,W] int32, win [F,2] {y0, x0}, pairs [N,2] {frame, class} -> mask [N,IH,IW] uint16, vectorised."""
    label = np.asarray(label, dtype=np.int32)
    _, H, W = label.shape
    IH, IW = image_dims
    pairs = np.asarray(pairs).reshape(-1, 2)
    out = np.zeros((len(pairs), IH, IW), dtype=np.uint16)
    for n, (f, c) in enumerate(pairs.tolist()):
        y0, x0 = (int(v) for v in np.asarray(win)[f])
        out[n, y0:y0 + H, x0:x0 + W] = np.where(label[f] == c, 65535, 0).astype(np.uint16)
    return out


def seg_masks_pixels(label, win, pairs, image_dims):
    """The same, pixel by pixel over the whole frame."""
    label = np.asarray(label, dtype=np.int32)
    _, H, W = label.shape
    IH, IW = image_dims
    pairs = np.asarray(pairs).reshape(-1, 2).tolist()
    out = np.zeros((len(pairs), IH, IW), dtype=np.uint16)
    for n, (f, c) in enumerate(pairs):
        y0, x0 = int(win[f][0]), int(win[f][1])
        for y in range(IH):
            for x in range(IW):
                i, j = y - y0, x - x0
                if 0 <= i < H and 0 <= j < W and int(label[f, i, j]) == c:
                    out[n, y, x] = 65535
    return out


def tie_logits(rng, F, H, W, C, ld, nans=2, pad=1e30):
    """Logits drawn from the integers -2..2 (ties are common), ``nans`` NaN entries at class channels of distinct pixels, the pad channels
    C..ld-1 filled with ``pad``: they must never win."""
    x = rng.integers(-2, 3, (F, H, W, ld)).astype(np.float32)
    x[..., C:] = pad
    flat = x.reshape(-1, ld)
    for k, p in enumerate(rng.choice(flat.shape[0], size=min(nans, flat.shape[0]), replace=False)):
        flat[p, (k + 1) % C] = np.nan
    return x
