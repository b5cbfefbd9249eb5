"""numpy restatement of ``df_cad_depth_sensor`` (steps D0..D6 of its comment in include/dfusion.h), vectorised over a frame, and a
second, per-pixel statement in plain Python integers that the host test holds it against.  Integer arithmetic only."""
import numpy as np

HORIZON = 65535
MAX_CODE = 65534
C0, C1, C2, C3 = 0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344
M32 = 0xFFFFFFFF


def mix32(seed, i):
    """csrc/choose_core.h's mix32 on uint32 arrays (or scalars), wrapping mod 2^32"""
    with np.errstate(over="ignore"):
        x = np.asarray(seed, dtype=np.uint32) ^ (np.asarray(i, dtype=np.uint32) * np.uint32(0x9E3779B9))
        x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7FEB352D)
        x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846CA68B)
        x = x ^ (x >> np.uint32(16))
    return x


def frame_seed(seed, first_frame, f):
    return int(mix32(seed & M32, (first_frame + f) & M32))                                  # D0


def edge_map(c, R, edge_step):
    """D2 for every pixel of the clean frame c (int64 [IH,IW]); horizon pixels get an answer too, which nobody asks for"""
    IH, IW = c.shape
    edge = np.zeros((IH, IW), dtype=bool)
    if R == 0:
        return edge
    for dr in range(-R, R + 1):
        for dq in range(-R, R + 1):
            r0, r1, q0, q1 = max(0, -dr), min(IH, IH - dr), max(0, -dq), min(IW, IW - dq)     # the pixels whose neighbour lies in the frame
            if r0 >= r1 or q0 >= q1:
                continue
            own, nb = c[r0:r1, q0:q1], c[r0 + dr:r1 + dr, q0 + dq:q1 + dq]
            edge[r0:r1, q0:q1] |= (nb == HORIZON) | (np.abs(nb - own) > edge_step)
    return edge


def sense_frame(frame, s, record):
    """(out uint16 [IH,IW], stats int32 [4]) of one clean frame with frame seed s"""
    noise_mul, R, edge_step, edge_drop24, drop24, quant = [int(v) for v in record]
    c = frame.astype(np.int64)
    IH, IW = c.shape
    p = np.arange(IH * IW, dtype=np.uint32).reshape(IH, IW)
    live = c != HORIZON                                                                      # D1
    edge = edge_map(c, R, edge_step) & live                                                  # D2
    drop = live & ((mix32(s ^ C3, p) >> np.uint32(8)).astype(np.int64) < drop24)             # D3
    edrop = live & ~drop & edge & ((mix32(s ^ C2, p) >> np.uint32(8)).astype(np.int64) < edge_drop24)   # D4
    kept = live & ~drop & ~edrop
    h0, h1 = mix32(s ^ C0, p).astype(np.int64), mix32(s ^ C1, p).astype(np.int64)            # D5
    S = (h0 & 0xFFFF) + (h0 >> 16) + (h1 & 0xFFFF) + (h1 >> 16) - 131070
    n = (noise_mul * S + (1 << 31)) >> 32                                                    # numpy's >> on int64 floors
    c1 = np.clip(c + n, 0, MAX_CODE)
    c2 = np.minimum(MAX_CODE, (c1 + quant // 2) // quant * quant)                            # D6
    out = np.where(kept, c2, HORIZON).astype(np.uint16)
    stats = np.array([edge.sum(), drop.sum(), edrop.sum(), (kept & (c2 != c)).sum()], dtype=np.int32)
    return out, stats


def sense(depth, record, seed, first_frame=0):
    """(depth_out uint16 [F,IH,IW], stats int32 [F,4]) of clean frames depth [F,IH,IW] uint16"""
    depth = np.asarray(depth)
    assert depth.dtype == np.uint16 and depth.ndim == 3
    outs = [sense_frame(depth[f], frame_seed(seed, first_frame, f), record) for f in range(depth.shape[0])]
    return np.stack([o for o, _ in outs]), np.stack([s for _, s in outs])


# ---- the same rule pixel by pixel, in Python integers -------------------------------------------------------------------------------
def _mix32_int(seed, i):
    x = (seed ^ (i * 0x9E3779B9)) & M32
    x ^= x >> 16; x = (x * 0x7FEB352D) & M32
    x ^= x >> 15; x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def sense_slow(depth, record, seed, first_frame=0):
    noise_mul, R, edge_step, edge_drop24, drop24, quant = [int(v) for v in record]
    F, IH, IW = depth.shape
    out, stats = np.zeros((F, IH, IW), dtype=np.uint16), np.zeros((F, 4), dtype=np.int32)
    for f in range(F):
        s = _mix32_int(seed & M32, (first_frame + f) & M32)
        for r in range(IH):
            for q in range(IW):
                p, c = r * IW + q, int(depth[f, r, q])
                if c == HORIZON:
                    out[f, r, q] = HORIZON
                    continue
                edge = False
                if R > 0:
                    for rr in range(r - R, r + R + 1):
                        for qq in range(q - R, q + R + 1):
                            if 0 <= rr < IH and 0 <= qq < IW:
                                cn = int(depth[f, rr, qq])
                                edge = edge or cn == HORIZON or abs(cn - c) > edge_step
                stats[f, 0] += edge
                if (_mix32_int(s ^ C3, p) >> 8) < drop24:
                    out[f, r, q] = HORIZON
                    stats[f, 1] += 1
                    continue
                if edge and (_mix32_int(s ^ C2, p) >> 8) < edge_drop24:
                    out[f, r, q] = HORIZON
                    stats[f, 2] += 1
                    continue
                h0, h1 = _mix32_int(s ^ C0, p), _mix32_int(s ^ C1, p)
                S = (h0 & 0xFFFF) + (h0 >> 16) + (h1 & 0xFFFF) + (h1 >> 16) - 131070
                n = (noise_mul * S + 2 ** 31) // 2 ** 32                              # Python's // floors
                c1 = min(max(c + n, 0), MAX_CODE)
                c2 = min(MAX_CODE, (c1 + quant // 2) // quant * quant)
                out[f, r, q] = c2
                stats[f, 3] += c2 != c
    return out, stats


def patchy_frames(F, IH, IW, seed):
    """F frames: above the anti-diagonal a smooth region of codes 20000..20019 (where a step above ``edge_step`` or a horizon makes the
    edge), below it random codes 0..65534, and two horizon patches per frame; neighbouring frames differ, so a window that strays into
    the next frame's rows shows"""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, HORIZON, (F, IH, IW)).astype(np.uint16)
    smooth = rng.integers(20000, 20020, (F, IH, IW)).astype(np.uint16)
    upper = (np.arange(IH)[:, None] + np.arange(IW)[None, :]) < (IH + IW) // 2
    d = np.where(upper[None], smooth, d)
    for f in range(F):
        for _ in range(2):
            r, q = int(rng.integers(0, IH)), int(rng.integers(0, IW))
            d[f, r:r + max(1, IH // 3), q:q + max(1, IW // 3)] = HORIZON
    return d
