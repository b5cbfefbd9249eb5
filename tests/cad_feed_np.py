"""``df_cad_item_table`` and ``df_cad_targets`` (include/dfusion.h) restated in numpy.  TEST INFRASTRUCTURE: the specification
densefusion_amd/csrc/cad_feed.hip is held to, bit for bit.  Every fp64 sum is spelled out element-wise in the contract's order (no ``@``,
no ``np.dot``: BLAS may fuse or reorder)."""
import numpy as np

import cad_np
from oracle.preprocess_ref import mix32


def item_table(depth, label, label_value=65535, min_side=8):
    """[F,8] int32: the row of ``cad_np.frame_stats``, the mask pixels of the half-open crop, the live flag."""
    out = []
    for d, l in zip(depth, label):
        st = cad_np.frame_stats(d, l, label_value)
        dmax, n_label, rmin, rmax, cmin, cmax = st
        count = int(np.count_nonzero((l[rmin:rmax, cmin:cmax] == label_value) & (d[rmin:rmax, cmin:cmax] != dmax))) if n_label else 0
        live = int(n_label > 0 and rmax - rmin >= min_side and cmax - cmin >= min_side and count > 0)
        out.append(st + [count, live])
    return np.array(out, dtype=np.int32).reshape(len(depth), 8)


def subset(P, M, seed):
    """The M of P indices with the smallest mix32(seed, index) keys, in increasing index order (the rule of ``cad_np.choose_rule``)."""
    return cad_np.choose_rule(np.arange(P, dtype=np.int64), M, seed & 0xFFFFFFFF)


def subset_brute(P, M, seed):
    """The same by a plain sort of (key, index) pairs in Python integers."""
    def key(i):
        x = (seed ^ (i * 0x9E3779B9)) & 0xFFFFFFFF
        x ^= x >> 16; x = (x * 0x7feb352d) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846ca68b) & 0xFFFFFFFF; x ^= x >> 16
        return x
    return np.array(sorted(i for _, i in sorted((key(i), i) for i in range(P))[:M]), dtype=np.int64)


def camera_points(m, pose):
    """X_j = ((R[j][0] m_x + R[j][1] m_y) + R[j][2] m_z) + T_j in fp64, one rounding per operation: [n,3]."""
    T = np.asarray(pose, dtype=np.float64).reshape(3, 4)
    return np.stack([((T[j, 0] * m[:, 0] + T[j, 1] * m[:, 1]) + T[j, 2] * m[:, 2]) + T[j, 3] for j in range(3)], axis=1)


def targets(model, model_scale, pose, seed, M, cloud_div=10000.0):
    """One item: (target, model_points) float32 [M,3] and the kept indices."""
    model = np.asarray(model, dtype=np.float64)
    keep = subset(len(model), M, int(seed))
    m = model[keep] * np.float64(model_scale)
    div = np.float32(cloud_div)
    return camera_points(m, pose).astype(np.float32) / div, m.astype(np.float32) / div, keep


def ulp_distance(a, b):
    """|a - b| in float32 units in the last place (finite values of one sign or around zero)."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


# ---- the fabricated frames the host and the device tests share ------------------------------------------------------------------------
def _noise(rng, F, IH, IW):
    """depth codes below 60000 with a scattered horizon, a label plane that holds only another value"""
    depth = rng.integers(1000, 60000, (F, IH, IW)).astype(np.uint16)
    depth[rng.random((F, IH, IW)) < 0.15] = 65535
    label = np.zeros((F, IH, IW), dtype=np.uint16)
    label[rng.random((F, IH, IW)) < 0.1] = 7
    return depth, label


def table_frames():
    """name -> (depth, label) uint16 [3,IH,IW], the smallest frames at which the item table can go wrong (min_side 8):
    9 x 9 (an odd pixel count: frames 1 and 2 start off an 8-byte boundary): 0 no label; 1 every pixel labelled, the box touches all four
    edges and is just live (8 x 8 crop); 2 labelled, every labelled pixel of the crop at the horizon except the last row and column;
    12 x 20: 0 a box of 8 rows (rmax - rmin = 7), dead by min_side; 1 the only depth-valid label pixels sit in the box's last row or
    last column; 2 no horizon pixel: the maximum is an object code, and the label pixels that hold it drop out of the count;
    130 x 257: one crop of more pixels than the grid has threads, plus the two small cases again at that size."""
    rng = np.random.default_rng(41)
    out = {}
    depth, label = _noise(rng, 3, 9, 9)
    label[1] = 65535
    label[2, 0:9, 0:9] = 65535
    depth[2, 0:8, 0:8] = 65535
    depth[2, 8, :] = 1234
    out["9x9"] = (depth, label)
    depth, label = _noise(rng, 3, 12, 20)
    label[0, 2:10, 3:16] = 65535                                  # rows 2..9: eight rows, rmax - rmin = 7
    label[1, 1:11, 2:15] = 65535
    depth[1, 1:10, 2:14] = 65535                                  # the crop [1:10, 2:14] holds the horizon only
    depth[1, 10, 2:15] = 2000; depth[1, 1:11, 14] = 3000          # valid pixels: row 10 and column 14, outside the crop
    depth[2] = rng.integers(1000, 40000, (12, 20)).astype(np.uint16)
    label[2, 1:12, 0:19][rng.random((11, 19)) < 0.7] = 65535
    label[2, 1, 0] = label[2, 11, 18] = 65535
    depth[2, 3:6, 4:9] = 40000                                    # the frame's maximum, on label pixels and off them
    out["12x20"] = (depth, label)
    depth, label = _noise(rng, 3, 130, 257)
    label[0, 3:128, 2:255][rng.random((125, 253)) < 0.6] = 65535
    label[0, 3, 2] = label[0, 127, 254] = 65535
    label[1, 129, 256] = 65535                                    # one pixel in the last row and column: an empty crop
    label[2, 50:58, 100:140] = 65535                              # eight rows again
    out["130x257"] = (depth, label)
    return out
