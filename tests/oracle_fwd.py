"""fp64 forward oracle for the inference engine's layer-by-layer tests: every debug tap of csrc/engine.hip (include/dfusion.h) as a stage
function of the CPU restatement (oracle/dfnet.py), channels-last like the taps, in fp64 and in fp32, and the bound rule of tests/oracle_grads.py
applied per stage.

Layer-local rule: a stage applied to the GPU's own input tap (cast to fp64 / fp32) gives ref64 / ref32, and the GPU's output tap must hold
    rel_l2(gpu, ref64) <= max(C * rel_l2(ref32, ref64), floor)
per tensor and for the worst channel (og.check, channel moved to the leading dimension).  One stage is one kernel (or a short chain of them),
so a defect shows in the stage it lives in, not only after 20 more layers.  The fp32 reference runs on one thread with oneDNN off
(og._fixed_fp32_order); fp64 uses the default thread pool.

FLOORS: (relative L2, worst channel) per stage, each 2x the largest GPU error measured on the MI355X over the fixtures and both GEMM routes
of tests/test_engine_fp64_gpu.py, rounded down (the measurement beside it).  Where the GPU's error stays inside C x the fp32 reference's, the
floor never binds.  On the forward, the Winograd-domain stages (layer2 .. layer4: F(2x2,3x3) / F(4x4,3x3) with fp32 transforms) measure
about 1e-6 relative, far below the 1e-5 of the training step's gradients (oracle_grads.GPU_FLOOR_CNN), so they keep floors of that size.
tests/test_oracle_fwd.py proves on the CPU that emulated defects (a dropped mid*mid term pair, a mean over Npad, the neighbouring object's
bias or rows, a lost Winograd edge row) break these bounds at least 3x, and names the routed stages where a lost term pair stays inside
C x the fp32 reference's own error (those, and layer4's own bf16 x 6 product, stay covered by the product-level test of the split kernel,
tests/test_split_gemm_engine_gpu.py).

Conditioning: the end-to-end poses follow an arg-max over the confidences.  A fixture is usable only if fp64 and fp32 pick the same
most-confident point with a top-two gap well above their difference (``conditioning``); otherwise change its seed, never widen a bound."""
from __future__ import annotations

import math
import time

import numpy as np
import torch
import torch.nn.functional as F

from oracle_grads import C, _fixed_fp32_order, check, rel_l2, worst_channel  # noqa: F401  (re-exported for the tests)
from densefusion_amd import synth
from oracle import dfnet, pose_math

P = "cnn.model.module."
FEATS = P + "feats."

# ---- floors (relative L2, worst channel): 2x the largest GPU error measured on the MI355X over the fixtures and both GEMM routes (the
# measurement beside each, relative L2 / worst channel), rounded down.  The relative-L2 floors bind only on layer4 (1.25x the fp32
# reference's 4x); the worst channels of the trunk and the point layers are channels a ReLU leaves nearly dead (their norm is noise), where
# the GPU's re-association alone reaches 2 - 7x the fp32 reference's 4x.  The Winograd-domain stages measure 1e-6 relative on the forward,
# not the 1e-5 of the training step's gradients (oracle_grads.GPU_FLOOR_CNN), so they need no wider floor.
FLOORS = {
    "stem": (4.5e-7, 1.6e-6),       # 2.26e-7 / 8.11e-7
    "layer1": (8.5e-7, 4.9e-5),     # 4.25e-7 / 2.47e-5
    "layer2": (1.0e-6, 8.6e-4),     # 5.14e-7 / 4.30e-4
    "layer3": (1.6e-6, 2.0e-4),     # 8.07e-7 / 1.01e-4
    "layer4": (2.6e-6, 1.3e-3),     # 1.31e-6 / 6.81e-4
    "psp": (7.3e-7, 1.2e-3),        # 3.65e-7 / 6.47e-4
    "up_1": (7.6e-7, 1.1e-5),       # 3.84e-7 / 5.67e-6
    "up_2": (8.4e-7, 6.6e-6),       # 4.24e-7 / 3.31e-6
    "up_3": (1.4e-6, 1.7e-5),       # 7.05e-7 / 8.99e-6
    "emb": (1.3e-7, 2.0e-7),        # 6.69e-8 / 1.02e-7
    "pf": (2.8e-7, 1.7e-4),         # 1.42e-7 / 8.68e-5
    "x5": (3.0e-7, 1.3e-3),         # 1.53e-7 / 6.72e-4
    "ap_x": (2.6e-7, 2.1e-4),       # 1.34e-7 / 1.07e-4
    "h1": (5.1e-7, 1.2e-3),         # 2.57e-7 / 6.27e-4
    "h2": (7.5e-7, 5.5e-3),         # 3.79e-7 / 2.76e-3
    "h3": (4.2e-7, 5.9e-4),         # 2.12e-7 / 2.98e-4
    "r": (3.3e-7, 2.5e-6),          # 1.66e-7 / 1.28e-6
    "t": (5.6e-8, 6.7e-8),          # 2.84e-8 / 3.38e-8
    "c": (3.5e-7, 3.5e-7),          # 1.75e-7 / (one channel)
    "rf_pf": (3.0e-7, 9.2e-5),      # 1.50e-7 / 4.60e-5
    "rf_x5": (3.7e-7, 1.5e-4),      # 1.85e-7 / 7.95e-5
    "rf_apx": (2.6e-7, 3.0e-4),     # 1.31e-7 / 1.51e-4
    "rf_f1": (3.4e-7, 8.8e-4),      # 1.73e-7 / 4.43e-4
    "rf_f2": (2.5e-7, 4.8e-4),      # 1.28e-7 / 2.43e-4
    "rf_r": (2.1e-7, 9.7e-7),       # 1.06e-7 / 4.87e-7
    "rf_t": (1.9e-7, 3.3e-7),       # 9.65e-8 / 1.65e-7
}
# end to end (the whole network in one comparison: r / t / c / emb of the full forward against the fp64 forward), measured likewise
E2E_FLOORS = {"emb": (4.6e-7, 7.6e-7),      # 2.33e-7 / 3.81e-7
              "r": (1.8e-6, 9.3e-6),        # 9.05e-7 / 4.68e-6
              "t": (5.6e-8, 6.6e-8),        # 2.84e-8 / 3.32e-8
              "c": (9.3e-7, 9.3e-7)}        # 4.68e-7 / (one channel)
ADD_FLOOR = 2.7e-7          # metres, ADD of the model points (measured 1.37e-7)
ANGLE_FLOOR = 3.9e-6        # radians, sign-invariant quaternion angle (measured 1.96e-6)


# ---- fixtures (K, N, crop, objects); each exists for a reason ----
FIXTURES = {
    # PSP bins over a 5 x 5 map (every bin of the 6-bin stage smaller than a pixel pair), one partial 128-row point block
    "k2_n64_40x40": dict(K=2, N=64, H=40, W=40, objs=[1], wseed=11, iseed=101),
    # three objects with different per-object bias rows and head column selection, the last class among them
    "k13_n500_80x80_b3": dict(K=13, N=500, H=80, W=80, objs=[0, 6, 12], wseed=12, iseed=7),
    # crops that are not multiples of 8 (the reference's geometry of lib/network.py:98-102)
    "k13_n500_100x140": dict(K=13, N=500, H=100, W=140, objs=[4], wseed=12, iseed=177),
    "k13_n500_88x72": dict(K=13, N=500, H=88, W=72, objs=[9], wseed=12, iseed=165),
    # the YCB shapes of the bench's buckets: two objects (first and last class) at 120 x 160, and 160 x 160, 240 x 320
    "k21_n1000_120x160_b2": dict(K=21, N=1000, H=120, W=160, objs=[0, 20], wseed=13, iseed=77),
    "k21_n1000_160x160": dict(K=21, N=1000, H=160, W=160, objs=[5], wseed=29, iseed=1280),
    "k21_n1000_240x320": dict(K=21, N=1000, H=240, W=320, objs=[11], wseed=29, iseed=1999),
    # the largest crop the datasets produce (datasets/ycb/dataset.py:247-289); one object keeps the oracle's time down
    "k21_n1000_480x640": dict(K=21, N=1000, H=480, W=640, objs=[3], wseed=29, iseed=3999),
    # num_points = 2000 (BASELINE configs[4]), and N = 129: the second 128-row block holds one valid row
    "k21_n2000_240x320": dict(K=21, N=2000, H=240, W=320, objs=[7], wseed=17, iseed=91),
    "k21_n129_80x120": dict(K=21, N=129, H=80, W=120, objs=[15], wseed=17, iseed=92),
    # the only F(2x2,3x3) route of layer3 among the datasets' crops (6 x 6 maps: layer3.0.conv2), with layer4 on F(2x2) and direct; and
    # N = 128, one full point block with no padding rows
    "k3_n128_48x48": dict(K=3, N=128, H=48, W=48, objs=[2], wseed=19, iseed=48),
}

# ---- edge fixtures: the smallest crops the entry points accept (8 <= H, W) and the documented maximum side (DF_MAX_CROP = 3200).  A crop
# side n gives a trunk map side of ((n - 1) // 2 + 1) three times over: 8 -> 1, 9 .. 16 -> 2, 17 .. 24 -> 3, 25 .. 32 -> 4, 36 -> 5,
# 3200 -> 400.  On these maps the pooling bins are wider than the map, the bilinear sources collapse onto one pixel, the Winograd axes are
# shorter than the dilation, the max-pool windows are mostly padding and the up-convolution's staged window is larger than the map.  They
# stay out of FIXTURES (tests/test_engine_edge_crops_gpu.py runs them); the seeds pass ``conditioning`` (8 x 8 with iseed 508 does not: a
# top-two confidence gap of 3e-5)
EDGE_FIXTURES = {
    "edge_8x8": dict(K=2, N=64, H=8, W=8, objs=[1], wseed=11, iseed=600),            # 1 x 1 trunk map
    "edge_16x16": dict(K=2, N=64, H=16, W=16, objs=[1], wseed=11, iseed=532),        # 2 x 2
    "edge_12x20": dict(K=2, N=64, H=12, W=20, objs=[1], wseed=11, iseed=532),        # 2 x 3
    "edge_8x24": dict(K=2, N=64, H=8, W=24, objs=[1], wseed=11, iseed=532),          # 1 x 3
    "edge_24x8": dict(K=2, N=64, H=24, W=8, objs=[1], wseed=11, iseed=532),          # 3 x 1
    "edge_32x32": dict(K=2, N=64, H=32, W=32, objs=[1], wseed=11, iseed=532),        # 4 x 4: one F(4x4) tile exactly
    "edge_36x28": dict(K=2, N=64, H=36, W=28, objs=[1], wseed=11, iseed=532),        # 5 x 4
    "edge_8x3200": dict(K=2, N=64, H=8, W=3200, objs=[1], wseed=11, iseed=3708),     # 1 x 400: the maximum side, one row
    "edge_3200x8": dict(K=2, N=64, H=3200, W=8, objs=[1], wseed=11, iseed=3708),     # 400 x 1: one column
}


def fixture(name):
    """-> (fixture dict, PoseNet state dict, refiner state dict, batch) with the batch's obj set to the fixture's objects."""
    f = FIXTURES[name] if name in FIXTURES else EDGE_FIXTURES[name]
    sdp = synth.make_state_dict(synth.posenet_spec(f["K"]), f["wseed"])
    sdr = synth.make_state_dict(synth.refiner_spec(f["K"]), f["wseed"] + 1000)
    b = synth.make_batch(f["iseed"], len(f["objs"]), f["H"], f["W"], f["N"], f["K"])
    b["obj"] = np.asarray(f["objs"], dtype=np.int64).reshape(-1, 1)
    return f, sdp, sdr, b


def npad(n):
    return (n + 127) // 128 * 128


def to_sd(sd, dtype):
    return {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}


# ---- layout helpers ----
def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def chan_first(x):
    """Channels-last [..., C] -> [C, rest] for the worst-channel check."""
    return x.reshape(-1, x.shape[-1]).t().contiguous()


def split3(x):
    """The split GEMM's cut of an fp32 operand into bf16 hi / mid / lo (csrc/split_gemm.hip, round-to-nearest at each cut), in fp64."""
    x = x.float()
    hi = x.bfloat16().float()
    r = x - hi
    mid = r.bfloat16().float()
    lo = (r - mid).bfloat16().float()
    return hi.double(), mid.double(), lo.double()


def _mid(x):
    return split3(x)[1]


def _lin(x, w, b=None, drop_midmid=False):
    """Channels-last 1x1 product x [..., I] . w[O, I(, 1, 1)]^T + b; ``drop_midmid``: leave out the split GEMM's mid*mid term pair (fp64)."""
    w = w.reshape(w.shape[0], -1)
    y = x @ w.t()
    if drop_midmid:
        y = y - _mid(x) @ _mid(w).t()
    return y if b is None else y + b


# ---- PoseNet stages (inputs and outputs in the engine's tap layouts) ----
def stage_stem(sd, img):
    return nhwc(F.relu(F.conv2d(img, sd[FEATS + "conv1.weight"], None, stride=2, padding=3)))


def _block(sd, base, x, stride, dil):
    return dfnet._basic_block(sd, base, x, stride, dil)


def stage_layer(sd, li, x, zero_last_row=False):
    """layer1 (with the max-pool in front) .. layer4 of lib/extractors.py, NHWC in and out; ``zero_last_row``: the last output row lost."""
    x = nchw(x)
    if li == 1:
        x = F.max_pool2d(x, kernel_size=3, stride=2, padding=1)
    stride, dil = ((1, 1), (2, 1), (1, 2), (1, 4))[li - 1]
    x = _block(sd, f"{FEATS}layer{li}.0.", x, stride, 1)
    x = _block(sd, f"{FEATS}layer{li}.1.", x, 1, dil)
    x = nhwc(x)
    if zero_last_row:
        x = x.clone()
        x[:, -1] = 0
    return x


def stage_psp(sd, feats, drop_midmid=False):
    """lib/pspnet.py:20-24; the bottleneck's product with the 512 feature channels (the engine's psp.fold.wfeat GEMM) split out."""
    f = nchw(feats)
    h, w = f.shape[2], f.shape[3]
    priors = []
    for i, s in enumerate((1, 2, 3, 6)):
        y = F.conv2d(F.adaptive_avg_pool2d(f, (s, s)), sd[f"{P}psp.stages.{i}.1.weight"], None)
        priors.append(F.interpolate(y, size=(h, w), mode="bilinear", align_corners=False))
    wb = sd[P + "psp.bottleneck.weight"].reshape(1024, 2560)
    out = nhwc(F.conv2d(torch.cat(priors, 1), wb[:, :2048, None, None], None))
    out = out + _lin(feats, wb[:, 2048:], sd[P + "psp.bottleneck.bias"], drop_midmid)
    return F.relu(out)


def stage_up(sd, name, x, drop_midmid=False):
    """lib/pspnet.py:27-37; ``drop_midmid`` removes mid(x) * mid(w) of every tap product (the engine forms them at low resolution)."""
    p = f"{P}{name}.conv."
    up = F.interpolate(nchw(x), scale_factor=2, mode="bilinear", align_corners=True)
    y = F.conv2d(up, sd[p + "1.weight"], sd[p + "1.bias"], padding=1)
    if drop_midmid:
        upm = F.interpolate(nchw(_mid(x)), scale_factor=2, mode="bilinear", align_corners=True)
        y = y - F.conv2d(upm, _mid(sd[p + "1.weight"]), None, padding=1)
    return nhwc(F.prelu(y, sd[p + "2.weight"]))


def stage_up3(sd, x, choose):
    """up_3 at the chosen pixels only: [B][N][64] (bilinear x2 of up_2, 3x3 patches at the chosen pixels, one product)."""
    up = F.interpolate(nchw(x), scale_factor=2, mode="bilinear", align_corners=True)
    B, Cc, H, W = up.shape
    pat = F.pad(up, (1, 1, 1, 1))
    ch = torch.as_tensor(choose).reshape(B, -1)
    yy, xx = ch // W, ch % W
    rows = []
    for b in range(B):
        taps = [pat[b, :, yy[b] + ky, xx[b] + kx] for ky in range(3) for kx in range(3)]      # 9 x [64][N]
        rows.append(torch.stack(taps, 2).permute(1, 0, 2).reshape(-1, Cc * 9))                 # [N][64 * 9], (c, ky, kx)
    w = sd[P + "up_3.conv.1.weight"].reshape(64, -1)
    y = torch.stack(rows) @ w.t() + sd[P + "up_3.conv.1.bias"]
    return F.prelu(y.permute(0, 2, 1), sd[P + "up_3.conv.2.weight"]).permute(0, 2, 1).contiguous()


def stage_emb(sd, z3):
    """final 1x1 conv + LogSoftmax over the 32 channels: [B][N][64] -> emb [B][32][N] (the engine's output layout)."""
    y = _lin(z3, sd[P + "final.0.weight"], sd[P + "final.0.bias"])
    return F.log_softmax(y, dim=2).permute(0, 2, 1).contiguous()


def stage_pf(sd, cloud, emb):
    """PoseNetFeat conv1 / e_conv1 / conv2 / e_conv2: [B][N][384] = x1 | e1 | x2 | e2 (cloud [B][N][3], emb [B][32][N])."""
    e = emb.permute(0, 2, 1)
    x1 = F.relu(_lin(cloud, sd["feat.conv1.weight"], sd["feat.conv1.bias"]))
    e1 = F.relu(_lin(e, sd["feat.e_conv1.weight"], sd["feat.e_conv1.bias"]))
    x2 = F.relu(_lin(x1, sd["feat.conv2.weight"], sd["feat.conv2.bias"]))
    e2 = F.relu(_lin(e1, sd["feat.e_conv2.weight"], sd["feat.e_conv2.bias"]))
    return torch.cat([x1, e1, x2, e2], 2)


def stage_x5(sd, pf):
    return F.relu(_lin(pf[..., 128:], sd["feat.conv5.weight"], sd["feat.conv5.bias"]))


def stage_apx(sd, x5, drop_midmid=False, over_npad=False):
    """conv6 + ReLU + AvgPool1d(N): [B][1024]; ``over_npad``: the sum divided by Npad instead of N (padding rows adding zero)."""
    y = F.relu(_lin(x5, sd["feat.conv6.weight"], sd["feat.conv6.bias"], drop_midmid))
    n = x5.shape[1]
    return y.sum(1) / (npad(n) if over_npad else n)


def stage_h1(sd, pf, apx, drop_midmid=False, roll_objects=False):
    """Head layer 1 of the three towers: [B][N][1920] = r | t | c; ``roll_objects``: each object gets its neighbour's global-feature bias."""
    if roll_objects:
        apx = torch.roll(apx, 1, 0)
    outs = []
    for h in "rtc":
        w = sd[f"conv1_{h}.weight"].reshape(640, 1408)
        g = apx @ w[:, 384:].t() + sd[f"conv1_{h}.bias"]                  # [B][640], one row per object
        outs.append(F.relu(_lin(pf, w[:, :384], None, drop_midmid) + g[:, None]))
    return torch.cat(outs, 2)


def stage_h(sd, layer, x, drop_midmid=False):
    """Head layer 2 ([B][N][1920] -> [B][N][768]) or 3 ([..768] -> [..384]), towers r | t | c."""
    ci = x.shape[2] // 3
    return torch.cat([F.relu(_lin(x[..., i * ci:(i + 1) * ci], sd[f"conv{layer}_{h}.weight"], sd[f"conv{layer}_{h}.bias"], drop_midmid))
                      for i, h in enumerate("rtc")], 2)


def stage_out(sd, h3, obj, obj_shift=0):
    """conv4 of the three towers, the rows of each object's class, sigmoid on c: r [B][N][4], t [B][N][3], c [B][N][1];
    ``obj_shift``: the rows of the next class instead."""
    K = sd["conv4_c.weight"].shape[0]
    obj = torch.as_tensor(obj).reshape(-1)
    outs = {}
    for i, (h, per) in enumerate((("r", 4), ("t", 3), ("c", 1))):
        y = _lin(h3[..., i * 128:(i + 1) * 128], sd[f"conv4_{h}.weight"], sd[f"conv4_{h}.bias"])       # [B][N][K * per]
        B, n = y.shape[:2]
        y = y.reshape(B, n, K, per)[torch.arange(B), :, (obj + obj_shift) % K]
        outs[h] = torch.sigmoid(y) if h == "c" else y
    return outs


# ---- refiner stages ----
def stage_rf_pf(sd, x, emb):
    """[B][N][384] = x1 | x2 | e1 | e2 (the engine's order; the reference's conv5 reads x1 | e1 | x2 | e2)."""
    pf = stage_pf(sd, x, emb)
    return torch.cat([pf[..., 0:64], pf[..., 128:256], pf[..., 64:128], pf[..., 256:384]], 2)


def stage_rf_x5(sd, pf):
    ref = torch.cat([pf[..., 0:64], pf[..., 192:256], pf[..., 64:192], pf[..., 256:384]], 2)       # x1 | e1 | x2 | e2
    return F.relu(_lin(ref, sd["feat.conv5.weight"], sd["feat.conv5.bias"]))


def stage_rf_f1(sd, apx):
    return torch.cat([F.relu(_lin(apx, sd[f"conv1_{h}.weight"], sd[f"conv1_{h}.bias"])) for h in "rt"], 1)


def stage_rf_f2(sd, f1):
    return torch.cat([F.relu(_lin(f1[:, i * 512:(i + 1) * 512], sd[f"conv2_{h}.weight"], sd[f"conv2_{h}.bias"])) for i, h in enumerate("rt")], 1)


def stage_rf_out(sd, f2, obj):
    obj = torch.as_tensor(obj).reshape(-1)
    outs = {}
    for i, (h, per) in enumerate((("r", 4), ("t", 3))):
        y = _lin(f2[:, i * 128:(i + 1) * 128], sd[f"conv3_{h}.weight"], sd[f"conv3_{h}.bias"])
        outs["rf_" + h] = y.reshape(y.shape[0], -1, per)[torch.arange(y.shape[0]), obj]
    return outs


# ---- the stage table: name -> (function of (sd, taps, inputs) -> output(s)) ----
def _s(name):
    return lambda sd, T, I: {
        "stem": lambda: stage_stem(sd, I["img"]),
        "layer1": lambda: stage_layer(sd, 1, T["stem"]),
        "layer2": lambda: stage_layer(sd, 2, T["layer1"]),
        "layer3": lambda: stage_layer(sd, 3, T["layer2"]),
        "layer4": lambda: stage_layer(sd, 4, T["layer3"]),
        "psp": lambda: stage_psp(sd, T["layer4"]),
        "up_1": lambda: stage_up(sd, "up_1", T["psp"]),
        "up_2": lambda: stage_up(sd, "up_2", T["up_1"]),
        "up_3": lambda: stage_up3(sd, T["up_2"], I["choose"]),
        "emb": lambda: stage_emb(sd, T["up_3"]),
        "pf": lambda: stage_pf(sd, I["cloud"], T["emb"]),
        "x5": lambda: stage_x5(sd, T["pf"]),
        "ap_x": lambda: stage_apx(sd, T["x5"]),
        "h1": lambda: stage_h1(sd, T["pf"], T["ap_x"]),
        "h2": lambda: stage_h(sd, 2, T["h1"]),
        "h3": lambda: stage_h(sd, 3, T["h2"]),
        "out": lambda: stage_out(sd, T["h3"], I["obj"]),
        "rf_pf": lambda: stage_rf_pf(sd, I["rf_x"], I["rf_emb"]),
        "rf_x5": lambda: stage_rf_x5(sd, T["rf_pf"]),
        "rf_apx": lambda: stage_apx(sd, T["rf_x5"]),
        "rf_f1": lambda: stage_rf_f1(sd, T["rf_apx"]),
        "rf_f2": lambda: stage_rf_f2(sd, T["rf_f1"]),
        "rf_out": lambda: stage_rf_out(sd, T["rf_f2"], I["obj"]),
    }[name]()


POSENET_STAGES = ("stem", "layer1", "layer2", "layer3", "layer4", "psp", "up_1", "up_2", "up_3", "emb", "pf", "x5", "ap_x", "h1", "h2", "h3", "out")
REFINER_STAGES = ("rf_pf", "rf_x5", "rf_apx", "rf_f1", "rf_f2", "rf_out")
STAGE = {n: _s(n) for n in POSENET_STAGES + REFINER_STAGES}


def _cast(d, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}


def apply_stage(name, sd, taps, inputs):
    """One stage on ``taps`` / ``inputs`` already in ``sd``'s dtype; -> {output name: tensor} (several for "out" / "rf_out")."""
    y = STAGE[name](sd, taps, inputs)
    return y if isinstance(y, dict) else {name: y}


def forward_taps(sd, inputs, stages, taps=None):
    """The stages chained on their own outputs (the oracle's taps in the engine's layouts, valid rows only)."""
    dt = next(iter(sd.values())).dtype
    taps, inputs = dict(taps or {}), _cast(inputs, dt)
    for s in stages:
        taps.update(apply_stage(s, sd, taps, inputs))
    return taps


def layer_local(sd64, sd32, gpu_taps, inputs, stages):
    """-> {output name: (ref64, ref32)} for every stage applied to the GPU's own input taps (cast to fp64 / fp32)."""
    t64, i64 = _cast(gpu_taps, torch.float64), _cast(inputs, torch.float64)
    t32, i32 = _cast(gpu_taps, torch.float32), _cast(inputs, torch.float32)
    res = {}
    for s in stages:
        y64 = apply_stage(s, sd64, t64, i64)
        with _fixed_fp32_order():
            y32 = apply_stage(s, sd32, t32, i32)
        for k in y64:
            res[k] = (y64[k], y32[k])
    return res


def channel_view(name, x):
    """The [C, ...] view of a tap / output for og.check: channel first (emb is [B][32][N] already channel-major per object)."""
    x = x.double() if torch.is_tensor(x) else torch.as_tensor(x).double()
    if name.removeprefix("e2e_") == "emb":
        return x.permute(1, 0, 2).reshape(x.shape[1], -1)
    return chan_first(x)


def bound_ratio(name, got, r64, r32, floor):
    """(GPU error, fp32 error, worst-channel GPU error, its fp32 error, ratio of the check) without asserting."""
    g, a, b = channel_view(name, got), channel_view(name, r64), channel_view(name, r32)
    e_g, e_32 = rel_l2(g, a), rel_l2(b, a)
    w_g, w_32 = (worst_channel(g, a), worst_channel(b, a)) if g.shape[0] > 1 else (0.0, 0.0)
    ratio = max(e_g / max(C * e_32, floor[0]), w_g / max(C * w_32, floor[1]))
    return e_g, e_32, w_g, w_32, ratio


def one_element_floor(name, r64, r32):
    """Worst-channel floor of a tap whose channels hold ONE element each (a 1 x 1 map; a per-object tap of a one-object fixture).  There the
    worst channel is a single number just above a ReLU's zero, and its relative error is one rounding draw over a tiny value: the fp32
    reference's error at that very element says nothing about what fp32 arithmetic may do to it (its draw may be near zero).  What does is the
    reference's typical absolute error on the tensor, the same for every element of a layer's output: the floor is C x the reference's RMS
    absolute error over the tensor, relative to the smallest channel the check looks at (norm above 1e-6 of the largest).  Computed from the two
    CPU references alone."""
    a, b = channel_view(name, r64), channel_view(name, r32)
    assert a.shape[1] == 1, f"{name}: channels of {a.shape[1]} elements"
    nb = torch.linalg.vector_norm(a, dim=1)
    live = nb > 1e-6 * float(nb.max())
    return C * float(((b - a) ** 2).mean().sqrt()) / float(nb[live].min())


# ---- end to end: the oracle's forward and estimate loop per object ----
def quat_angle(q1, q2):
    q1, q2 = np.asarray(q1, np.float64), np.asarray(q2, np.float64)
    d = abs(float(np.dot(q1 / np.linalg.norm(q1), q2 / np.linalg.norm(q2))))
    return 2.0 * math.acos(min(1.0, d))


def end_to_end(sdp, sdr, batch, dtype, iters=2):
    """dfnet.posenet_forward + the estimate loop of oracle/pose_math per object -> dict of r [B][N][4], t, c [B][N][1], emb [B][32][N],
    pose_wo [B][7], pose [B][7], which [B], gap [B] (top-two confidence gap)."""
    sp, sr = to_sd(sdp, dtype), to_sd(sdr, dtype)
    out = {k: [] for k in ("r", "t", "c", "emb", "pose_wo", "pose", "which", "gap")}
    with torch.no_grad():
        for i in range(batch["img"].shape[0]):
            img = torch.from_numpy(batch["img"][i:i + 1]).to(dtype)
            cloud = torch.from_numpy(batch["cloud"][i:i + 1]).to(dtype)
            choose = torch.from_numpy(batch["choose"][i:i + 1])
            obj = torch.from_numpy(batch["obj"][i:i + 1])
            r, t, c, emb = dfnet.posenet_forward(sp, img, cloud, choose, obj)
            my_r, my_t, which = pose_math.select_pose(r, t, c, cloud)
            wo = np.append(my_r, my_t).astype(np.float64)
            for _ in range(iters):
                my_r, my_t = pose_math.refine_step(sr, cloud, emb, obj, my_r, my_t)
            cs = torch.sort(c.reshape(-1), descending=True)[0]
            for k, v in (("r", r[0]), ("t", t[0]), ("c", c[0]), ("emb", emb[0]), ("pose_wo", torch.from_numpy(wo)),
                         ("pose", torch.from_numpy(np.append(my_r, my_t).astype(np.float64)))):
                out[k].append(v)
            out["which"].append(which)
            out["gap"].append(float(cs[0] - cs[1]))
    return {k: (torch.stack(v) if torch.is_tensor(v[0]) else v) for k, v in out.items()}


def oracle_pair(sdp, sdr, batch, iters=2):
    """fp64 and fp32 (fixed order) end-to-end results and the oracle's wall time."""
    t0 = time.time()
    e64 = end_to_end(sdp, sdr, batch, torch.float64, iters)
    with _fixed_fp32_order():
        e32 = end_to_end(sdp, sdr, batch, torch.float32, iters)
    return e64, e32, time.time() - t0


def conditioning(e64, e32):
    """Assert the fixture is well conditioned: the same most-confident point in fp64 and fp32, and a top-two gap of at least 1e-4 and 100x
    the largest confidence difference between them."""
    noise = float((e64["c"] - e32["c"].double()).abs().max())
    for i, (a, b, gap) in enumerate(zip(e64["which"], e32["which"], e64["gap"])):
        assert a == b, f"object {i}: the most confident point differs between fp64 and fp32 -- ill-conditioned fixture"
        assert gap >= max(1e-4, 100 * noise), f"object {i}: top-two confidence gap {gap:.2e} vs fp32 noise {noise:.2e} -- ill-conditioned fixture"


def add_of(p, q, model_points):
    return pose_math.add_metric(pose_math.transform_model(np.asarray(p, np.float64), model_points),
                                pose_math.transform_model(np.asarray(q, np.float64), model_points))
