"""Forced-index fp64 oracle of SegNet (vanilla_segmentation/segnet.py), eval and training, for tests/test_segnet_fp64_gpu.py and its CPU
power check tests/test_oracle_segnet.py.  A CPU torch restatement, parametrised by dtype, stage by stage and channels-last like the taps
of ``SegNet.forward(x, taps=...)``: conv + folded BatchNorm + ReLU (eval), conv then BatchNorm with batch statistics + ReLU (training), the
classifier conv, the 2x2 pool, the un-pool and the cross-entropy over the first 22 of the classifier's padded channels.

Forced indices: pool and un-pool take the window position 0..3 (2 * (y & 1) + (x & 1), the kernels' uint8 index) from a GIVEN index tensor
instead of their own arg-max.  The pooled value is gathered at that position and the un-pool scatters to it, so the gradient goes to the
forced position.  The max is continuous in its inputs, only its location is not: with the GPU's indices forced, fp64, fp32 and the GPU
compute the same smooth function and the arg-max noise of the older end-to-end tests is gone.  Whether the GPU's indices ARE the arg-max is
checked apart, exactly (``pool_exact`` / ``unpool_exact`` against F.max_pool2d / F.max_unpool2d of the GPU's own input, torch.equal).

Layer-local rule (tests/oracle_fwd.py): a stage applied to the GPU's own input tap, cast to fp64 and to fp32 (one thread, oneDNN off:
oracle_grads._fixed_fp32_order), gives ref64 / ref32, and oracle_grads.check holds the GPU's output tap to
    rel_l2(gpu, ref64) <= max(C * rel_l2(ref32, ref64), floor)
per tensor and for the worst channel.  The backward of a training stage is torch.autograd.grad(stage(a64, params64), (a64, params64), g64)
with g64 the GPU's own gradient of the stage's output tap.  The relative-L2 floor is oracle_grads.FLOOR; the worst-channel floor comes from
the two CPU references alone (``channel_floor``: C x the fp32 reference's RMS absolute error over the tensor, relative to the RMS of the
smallest live channel -- oracle_fwd.one_element_floor for channels of any length).  No floor is a GPU measurement.

The eval fold is done here, in the oracle's dtype, from the raw state dict (w g / sqrt(var + eps), (b - mean) g / sqrt(var + eps) + beta),
so SegNet._layer's fold is under test too.

Winograd-routed eval layers: the eval forward runs every convolution with Cin >= 256 through F(2x2,3x3) with fp32 transforms (``WINOGRAD``:
32 33 41 42 43 51 52 53 53d 52d 51d 43d 42d 41d 33d 32d 31d).  For those stages the fp32 reference is ``conv_f2x2`` below, an fp32
restatement of F(2x2,3x3) with the standard transform matrices: the transforms add and subtract up to four inputs and nine weights before
the channel sum, which direct summation in fp32 never pays for, so direct summation would set a bound the algorithm cannot meet.  fp64 stays
direct summation.  The training tape runs every convolution on the direct kernel, so training stages use direct summation in both dtypes.

Forced ReLU masks (training, end to end): a ReLU's value is continuous but its derivative is not, exactly as the max-pool's location is not.
Across a whole step the pre-activations of fp64 and of any fp32 run differ by ~1e-6, a few of the 10^6 .. 10^7 of them lie that close to
zero, and one such element in a stage-5 layer moves every encoder gradient by 1e-3 .. 8e-3 of its scale (measured on the CPU: the fp32 chain
against the fp64 chain with only the indices forced misses oracle_grads.check's flat 2e-3 bound on ~70 gradient tensors in 22 of 24 seeds at
2 x 32 x 64, in all seeds tried at 2 x 64 x 96 -- no seed can be found, and which elements flip differs between fp32 implementations).  So
the end-to-end step forces the device's ReLU masks together with its pool indices (``relu_masks``, ``chain(relu=...)``: y = pre * mask);
fp64, fp32 and the device then differentiate the same smooth function.  That the device's masks ARE the right ones is what the layer-local
conditioning below asserts, element by element, so forcing them hides nothing.  tests/test_oracle_segnet.py asserts both halves.

Conditioning (training): the backward follows each ReLU's mask.  ``relu_conditioning`` recomputes the pre-activation in fp64 from the GPU's
own z and compares its sign with the GPU's mask (y > 0 of the tapped output; for a pooled stage, whose full-size output the fused launch
never writes, the positions the pooled tensor fixes: the index position where the pooled value is positive, the whole window where it is
zero).  One element on the other side of zero moves dz of its layer by about 1 / sqrt(elements), far above any rounding bound, so a fixture
whose GPU mask differs from fp64's is ill-conditioned: change its seed, never mask the element.  The function reports, over the differing
elements, the smallest and largest |pre-activation| / channel std: a seed problem differs at ~1e-7, a kernel defect differs everywhere."""
from __future__ import annotations

import contextlib

import numpy as np
import torch
import torch.nn.functional as F

import oracle_grads as og
from oracle_grads import C, FLOOR, _fixed_fp32_order, rel_l2, worst_channel  # noqa: F401  (re-exported for the tests)
from densefusion_amd import synth

F64, F32 = torch.float64, torch.float32
LAYERS = synth._SEG_LAYERS
NAMES = [n for n, _, _ in LAYERS]
ENC_POOL = ("12", "22", "33", "43", "53")             # the layers a max-pool follows
DEC_UNPOOL = ("53d", "43d", "33d", "22d", "12d")      # the layers an un-pool precedes
WINOGRAD = tuple(n for n, cin, _ in LAYERS if cin >= 256)
CLASSES = 22
EPS, MOMENTUM = 1e-5, 0.1
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)

# (B, H, W, weight seed, image seed).  Stage 5 sees H/16 x W/16 maps.
EVAL_FIXTURES = {
    "e_1x32x32": (1, 32, 32, 31, 7),          # 2 x 2: the smallest input SegNet accepts, the pooled map 1 x 1
    "e_2x32x64": (2, 32, 64, 32, 8),          # 2 x 4
    "e_1x64x160": (1, 64, 160, 33, 9),        # 4 x 10, odd F(2x2) tile counts further up (5 tiles across)
    "e_1x96x128": (1, 96, 128, 34, 10),       # 6 x 8
}
TRAIN_FIXTURES = {
    "t_1x32x32": (1, 32, 32, 41, 17),         # BatchNorm over 4 values per channel at stage 5 (unbiased factor 4/3)
    "t_2x32x64": (2, 32, 64, 42, 18),
    # reseeded from (43, 19): on the MI355X one pre-activation of bn22d (of 393216) lay at 1.0e-9 channel std from zero, on the other
    # side of it than in fp64 (``relu_conditioning``)
    "t_2x64x96": (2, 64, 96, 143, 119),
}


def _frame(seed, B, H, W):
    """Seeded image of 12 coloured ellipses per frame with pixel noise, normalised, and its label map -> (x [B,3,H,W] fp32, label int64)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    label = np.zeros((B, H, W), dtype=np.int64)
    img = np.zeros((B, 3, H, W), dtype=np.float32)
    colours = rng.integers(0, 256, (22, 3)).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        for _ in range(12):
            c = int(rng.integers(1, 22))
            cy, cx, ry, rx = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(H / 10, H / 3), rng.uniform(W / 10, W / 3)
            label[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1] = c
        img[b] = colours[label[b]].transpose(2, 0, 1) + rng.normal(0, 3, (3, H, W))
    x = (img - MEAN[None, :, None, None]) / STD[None, :, None, None]
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(label)


def fixture(name):
    """-> (state dict of numpy arrays, x [B,3,H,W] fp32, label [B,H,W] int64)"""
    B, H, W, wseed, iseed = (EVAL_FIXTURES if name in EVAL_FIXTURES else TRAIN_FIXTURES)[name]
    x, label = _frame(iseed, B, H, W)
    return synth.make_segnet_state_dict(wseed), x, label


def to_sd(sd, dtype):
    """Copies of the floating-point entries of the state dict in ``dtype``."""
    return {k: torch.from_numpy(np.array(v)).to(dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}


def nhwc(x):
    return x.permute(0, 2, 3, 1)


def chan_first(x):
    """Channels-last [..., C] -> [C, rest] for the worst-channel check."""
    return x.reshape(-1, x.shape[-1]).t()


# ---- stages (channels-last in and out, differentiable) ---------------------------------------------------------------------------
def conv(a, w, b):
    """3x3 / pad 1 convolution by direct summation; a [B,H,W,>= Cin] (padding channels ignored), w [Cout,Cin,3,3] -> [B,H,W,Cout]."""
    return F.conv2d(a[..., :w.shape[1]].permute(0, 3, 1, 2), w, b, padding=1).permute(0, 2, 3, 1)


_BT = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
_G = [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]]
_AT = [[1, 1, 1, 0], [0, 1, -1, -1]]


def conv_f2x2(a, w, b):
    """The same convolution through Winograd F(2x2,3x3) in a's dtype: V = B^T d B per 4 x 4 input tile, U = G g G^T per filter, the
    channel sum per transform-domain position, Y = A^T M A.  H and W even (SegNet's maps are)."""
    dt = a.dtype
    BT, G, AT = (torch.tensor(m, dtype=dt) for m in (_BT, _G, _AT))
    x = F.pad(a[..., :w.shape[1]].permute(0, 3, 1, 2), (1, 1, 1, 1))                       # [B,Cin,H+2,W+2]
    Bn, Ci, Hp, Wp = x.shape
    th, tw = (Hp - 2) // 2, (Wp - 2) // 2
    d = x.unfold(2, 4, 2).unfold(3, 4, 2)                                                  # [B,Cin,th,tw,4,4]
    V = torch.einsum("ij,bcthjk,lk->ilbthc", BT, d, BT).reshape(16, Bn * th * tw, Ci)
    U = torch.einsum("ij,ocjk,lk->iloc", G, w, G).reshape(16, w.shape[0], Ci)
    M = torch.bmm(V, U.transpose(1, 2)).reshape(4, 4, Bn, th, tw, w.shape[0])
    Y = torch.einsum("pi,ilbtho,ql->btphqo", AT, M, AT).reshape(Bn, 2 * th, 2 * tw, w.shape[0])
    return Y + b


def fold(P, name):
    """The eval fold of BatchNorm into its convolution, in P's dtype, from the raw state dict."""
    w, b = P[f"conv{name}.weight"], P[f"conv{name}.bias"]
    if name == "11d":
        return w, b
    s = P[f"bn{name}.weight"] / torch.sqrt(P[f"bn{name}.running_var"] + EPS)
    return w * s[:, None, None, None], (b - P[f"bn{name}.running_mean"]) * s + P[f"bn{name}.bias"]


def stage_eval(P, name, a, winograd=False):
    """conv + folded BatchNorm + ReLU of layer ``name`` (the classifier 11d: the conv alone)."""
    w, b = fold(P, name)
    z = (conv_f2x2 if winograd else conv)(a, w, b)
    return z if name == "11d" else F.relu(z)


def bn_pre(z, gamma, beta):
    """Training BatchNorm before the ReLU -> (pre-activation, batch mean, biased variance), statistics over all but the last axis."""
    zz = z.reshape(-1, z.shape[-1])
    mu, var = zz.mean(0), zz.var(0, unbiased=False)
    return (z - mu) / torch.sqrt(var + EPS) * gamma + beta, mu, var


def bn_relu(z, gamma, beta):
    return F.relu(bn_pre(z, gamma, beta)[0])


def running_stats(z, rm0, rv0, momentum=MOMENTUM):
    """nn.BatchNorm2d's update of its running buffers from z's batch statistics (the UNBIASED variance into running_var)."""
    zz = z.reshape(-1, z.shape[-1])
    vu = zz.var(0, unbiased=True) if zz.shape[0] > 1 else zz.var(0, unbiased=False)
    return (1 - momentum) * rm0 + momentum * zz.mean(0), (1 - momentum) * rv0 + momentum * vu


def _windows(y):
    """[B,H,W,C] -> [B,H/2,W/2,C,4], the last axis the window position 2 * (y & 1) + (x & 1)."""
    B, H, W, Cc = y.shape
    return y.reshape(B, H // 2, 2, W // 2, 2, Cc).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, Cc, 4)


def pool_forced(y, idx):
    """The value at window position idx (uint8 / int64 [B,H/2,W/2,C]) of every 2x2 window."""
    return _windows(y).gather(4, idx.long()[..., None])[..., 0]


def unpool_forced(p, idx):
    """p [B,h,w,C] scattered to window position idx of a zero [B,2h,2w,C]."""
    B, h, w, Cc = p.shape
    out = torch.zeros(B, h, w, Cc, 4, dtype=p.dtype).scatter(4, idx.long()[..., None], p[..., None])
    return out.reshape(B, h, w, Cc, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * h, 2 * w, Cc)


def pool_exact(y):
    """F.max_pool2d(y, 2, 2, return_indices=True) of channels-last y -> (pooled, window position uint8), channels-last."""
    W = y.shape[2]
    p, flat = F.max_pool2d(y.permute(0, 3, 1, 2).contiguous(), 2, 2, return_indices=True)
    pos = ((flat // W) & 1) * 2 + ((flat % W) & 1)
    return nhwc(p).contiguous(), nhwc(pos).to(torch.uint8).contiguous()


def unpool_exact(p, idx):
    """F.max_unpool2d of channels-last p with window positions idx -> channels-last."""
    B, h, w, Cc = p.shape
    oy = torch.arange(h).reshape(1, h, 1, 1) * 2 + (idx.long() >> 1)
    ox = torch.arange(w).reshape(1, 1, w, 1) * 2 + (idx.long() & 1)
    flat = (oy * (2 * w) + ox).permute(0, 3, 1, 2).contiguous()
    return nhwc(F.max_unpool2d(p.permute(0, 3, 1, 2).contiguous(), flat, 2, 2)).contiguous()


def cross_entropy(logits, target):
    """nn.CrossEntropyLoss() over the first CLASSES channels of channels-last logits."""
    return F.cross_entropy(logits[..., :CLASSES].reshape(-1, CLASSES), target.reshape(-1))


# ---- the stage list ------------------------------------------------------------------------------------------------------------------
def stages(mode):
    """[(kind, layer, input tap, output tap, index tap)] in forward order.  Kinds: eval "cbr" (conv + folded BN + ReLU; the classifier
    without ReLU), "pool", "unpool"; training "conv", "bn", "bnpool" (BatchNorm + ReLU + pool in one launch), "unpool"."""
    out, cur, pending = [], "x", []
    for name in NAMES:
        if name in DEC_UNPOOL:
            out.append(("unpool", name, cur, "u" + name, pending.pop()))
            cur = "u" + name
        last = name == "11d"
        if mode == "eval":
            out.append(("cbr", name, cur, ("z" if last else "y") + name, None))
            cur = ("z" if last else "y") + name
            if name in ENC_POOL:
                out.append(("pool", name, cur, "p" + name, "i" + name))
        else:
            out.append(("conv", name, cur, "z" + name, None))
            cur = "z" + name
            if name in ENC_POOL:
                out.append(("bnpool", name, cur, "p" + name, "i" + name))
            elif not last:
                out.append(("bn", name, cur, "y" + name, None))
                cur = "y" + name
        if name in ENC_POOL:
            cur = "p" + name
            pending.append("i" + name)
    return out


def tap_order(mode):
    """The keys ``SegNet.forward(x, taps=...)`` fills, in order."""
    keys = ["x"]
    for kind, name, _, o, i in stages(mode):
        keys += [o, i] if kind in ("pool", "bnpool") else [o]
    return keys


def chain(P, x, mode, idx=None, taps=None, stats=None, post=None, relu=None):
    """The whole forward in P's dtype on channels-last x; ``idx``: {index tap: positions} to force (None: the chain's own arg-max, as a
    device run has it); ``relu``: {layer: mask} to force on the training ReLUs (``relu_masks``; None: the chain's own sign).  Fills ``taps`` like SegNet's own, ``stats`` with {layer: (batch mean, biased variance)} in training, and passes
    the output of layer ``name`` through ``post[name]`` (the defect emulations).  -> the classifier's output [B,H,W,CLASSES]."""
    T = {} if taps is None else taps
    T["x"] = x
    for kind, name, i, o, ik in stages(mode):
        a = T[i]
        if kind == "unpool":
            y = unpool_forced(a, T[ik])
        elif kind == "cbr":
            y = stage_eval(P, name, a, winograd=name in WINOGRAD and P["conv11.weight"].dtype == F32)
        elif kind == "conv":
            y = conv(a, P[f"conv{name}.weight"], P[f"conv{name}.bias"])
        elif kind == "pool":
            T[ik] = idx[ik] if idx is not None else pool_exact(a.detach())[1]
            y = pool_forced(a, T[ik])
        else:
            pre, mu, var = bn_pre(a, P[f"bn{name}.weight"], P[f"bn{name}.bias"])
            if stats is not None:
                stats[name] = (mu.detach(), var.detach())
            y = F.relu(pre) if relu is None or kind == "bnpool" else pre * relu[name]
            if kind == "bnpool":
                T[ik] = idx[ik] if idx is not None else pool_exact(y.detach())[1]
                y = pool_forced(y, T[ik]) if relu is None else pool_forced(pre, T[ik]) * relu[name]
        if post and name in post and kind in ("cbr", "conv"):
            y = post[name](y, a)
        T[o] = y
    return T["z11d"]


def eval_forward(sd, x, idx, dtype, post=None, taps=None):
    """End-to-end forced eval forward -> logits [B,H,W,CLASSES] (x [B,3,H,W])."""
    with torch.no_grad():
        return chain(to_sd(sd, dtype), nhwc(x).to(dtype), "eval", idx, taps=taps, post=post)


def relu_masks(taps):
    """The ReLU masks a training forward took, read off its taps: y > 0, or for a pooled stage the pooled value > 0 (the mask at the
    index position, the only one of the window that the forward value and the gradient pass through)."""
    return {o[1:]: taps[o].detach().cpu() > 0 for kind, _, _, o, _ in stages("train") if kind in ("bn", "bnpool")}


def train_step(sd, x, target, idx, dtype, taps=None, relu=None):
    """End-to-end forced training step -> (loss, {parameter: gradient}, {running buffer: value after the step})."""
    P = {k: v.requires_grad_(not k.endswith(("running_mean", "running_var"))) for k, v in to_sd(sd, dtype).items()}
    T = {} if taps is None else taps
    loss = cross_entropy(chain(P, nhwc(x).to(dtype), "train", idx, taps=T, relu=relu), target)
    keys = [k for k, v in P.items() if v.requires_grad]
    grads = dict(zip(keys, torch.autograd.grad(loss, [P[k] for k in keys])))
    run = {}
    for name in NAMES[:-1]:
        rm, rv = running_stats(T["z" + name].detach(), P[f"bn{name}.running_mean"], P[f"bn{name}.running_var"])
        run[f"bn{name}.running_mean"], run[f"bn{name}.running_var"] = rm, rv
    return loss.detach(), grads, run


# ---- layer-local references ------------------------------------------------------------------------------------------------------
def _cpu(t, dtype):
    t = t.detach().cpu()
    return t.to(dtype) if t.is_floating_point() else t


def stage_fn(P, kind, name, idx=None):
    """The stage as a function of its input tap, in P's dtype (parameters read from P at call time)."""
    if kind == "cbr":
        return lambda a: stage_eval(P, name, a, winograd=name in WINOGRAD and a.dtype == F32)
    if kind == "conv":
        return lambda a: conv(a, P[f"conv{name}.weight"], P[f"conv{name}.bias"])
    if kind == "bn":
        return lambda z: bn_relu(z, P[f"bn{name}.weight"], P[f"bn{name}.bias"])
    if kind == "bnpool":
        return lambda z: pool_forced(bn_relu(z, P[f"bn{name}.weight"], P[f"bn{name}.bias"]), idx)
    if kind == "pool":
        return lambda y: pool_forced(y, idx)
    return lambda p: unpool_forced(p, idx)


def stage_params(kind, name):
    if kind == "conv":
        return [f"conv{name}.weight", f"conv{name}.bias"]
    return [f"bn{name}.weight", f"bn{name}.bias"] if kind in ("bn", "bnpool") else []


def layer_local(sd, taps, mode, grads=None, only=None):
    """Every stage (``only``: the one whose output tap that is) on the device's own input tap -> [(kind, layer, output tap, ref64, ref32,
    backward)]; ``backward`` (training, given ``grads`` = {tap: the device's gradient of it}) is {"in" / parameter key: (ref64, ref32)}
    from autograd with the device's own gradient of the stage's output."""
    res = []
    P = {F64: to_sd(sd, F64), F32: to_sd(sd, F32)}
    for kind, name, i, o, ik in stages(mode):
        if only is not None and o != only:
            continue
        fwd, bwd = {}, {}
        for dt in (F64, F32):
            a = _cpu(taps[i], dt)
            keys = stage_params(kind, name) if grads is not None else []
            for k in keys:
                P[dt][k].requires_grad_(True)
            want_da = grads is not None and i != "x"
            a.requires_grad_(want_da)
            with torch.set_grad_enabled(grads is not None), (_fixed_fp32_order() if dt == F32 else contextlib.nullcontext()):
                y = stage_fn(P[dt], kind, name, None if ik is None else _cpu(taps[ik], dt))(a)
                if grads is not None and (keys or want_da):
                    g = _cpu(grads[o], dt)[..., :y.shape[-1]]
                    ins = ([a] if want_da else []) + [P[dt][k] for k in keys]
                    for k, v in zip((["in"] if want_da else []) + keys, torch.autograd.grad(y, ins, g)):
                        bwd.setdefault(k, {})[dt] = v
            for k in keys:
                P[dt][k].requires_grad_(False)
            fwd[dt] = y.detach()
        res.append((kind, name, o, fwd[F64], fwd[F32], {k: (v[F64], v[F32]) for k, v in bwd.items()}))
    return res


def loss_local(z11d, target):
    """The cross-entropy on the device's own logits -> {"loss": (ref64, ref32), "dlogits": (ref64, ref32) [B,H,W,CLASSES]}."""
    out = {"loss": [], "dlogits": []}
    for dt in (F64, F32):
        z = _cpu(z11d, dt)[..., :CLASSES].clone().requires_grad_(True)
        with (_fixed_fp32_order() if dt == F32 else contextlib.nullcontext()):
            loss = cross_entropy(z, target.cpu())
            g, = torch.autograd.grad(loss, z)
        out["loss"].append(loss.detach())
        out["dlogits"].append(g)
    return {k: tuple(v) for k, v in out.items()}


# ---- the bound rule --------------------------------------------------------------------------------------------------------------
def channel_floor(r64, r32):
    """Worst-channel floor of a [C, n] view from the two CPU references alone: C x the fp32 reference's RMS absolute error over the
    tensor, relative to the RMS of the smallest channel the check looks at (norm above 1e-6 of the largest), and never below FLOOR.  The
    fp32 reference's error in one channel is one draw (near zero in a channel a ReLU leaves nearly dead, or of one element); its RMS
    over the tensor is what fp32 arithmetic does to every element of the layer's output."""
    a, b = r64.double().reshape(r64.shape[0], -1), r32.double().reshape(r64.shape[0], -1)
    rms = torch.linalg.vector_norm(a, dim=1) / a.shape[1] ** 0.5
    live = rms > 1e-6 * float(rms.max())
    if not bool(live.any()):
        return FLOOR
    return max(FLOOR, C * float(((b - a) ** 2).mean().sqrt()) / float(rms[live].min()))


def view(t, activation=True):
    """The [C, n] view og.check takes: activations channel first, weight gradients [Cout, rest], vectors and scalars flat."""
    t = t.detach().cpu().double()
    if t.dim() == 4 and activation:
        return chan_first(t)
    return t.reshape(t.shape[0], -1) if t.dim() > 1 else t.reshape(-1)


def bound_ratio(got, r64, r32, activation=True):
    """(device error, fp32 error, worst-channel device error, its fp32 error, ratio to the bound, floors, the three views) without
    asserting."""
    g, a, b = (view(t, activation) for t in (got, r64, r32))
    channels = a.dim() == 2 and a.shape[0] > 1
    e_g, e_32 = rel_l2(g, a), rel_l2(b, a)
    floors = (FLOOR, channel_floor(a, b) if channels else FLOOR)
    ratio = e_g / max(C * e_32, floors[0])
    w_g = w_32 = 0.0
    if channels:
        w_g, w_32 = worst_channel(g, a), worst_channel(b, a)
        ratio = max(ratio, w_g / max(C * w_32, floors[1]))
    return e_g, e_32, w_g, w_32, ratio, floors, (g, a, b)


class Table:
    """One test's table: stage, device error, fp32 error (relative L2 and worst channel), ratio to the bound; ``finish`` prints it and
    raises on any tensor outside its bound (oracle_grads.check)."""

    def __init__(self, title):
        self.rows, self.fails, self.title, self.worst = [], [], title, (0.0, "")

    def check(self, what, got, r64, r32, activation=True):
        e_g, e_32, w_g, w_32, ratio, floors, (g, a, b) = bound_ratio(got, r64, r32, activation)
        self.rows.append(f"{what:28s} {e_g:10.2e} {e_32:10.2e} {w_g:10.2e} {w_32:10.2e} {ratio:8.3f}")
        self.worst = max(self.worst, (ratio, what))
        try:
            og.check(what, g, a, b, floor=floors)
        except AssertionError as e:
            self.fails.append(str(e))
        return ratio

    def exact(self, what, ok):
        self.rows.append(f"{what:28s} {'exact' if ok else 'DIFFERS':>10s}")
        if not ok:
            self.fails.append(f"{what}: not bit-equal")

    def finish(self):
        print(f"\n{self.title}\n{'stage':28s} {'gpu rel':>10s} {'fp32 rel':>10s} {'gpu chan':>10s} {'fp32 chan':>10s} {'ratio':>8s}")
        print("\n".join(self.rows))
        print(f"{self.title}: worst ratio to the bound {self.worst[0]:.3f} at {self.worst[1]}")
        assert not self.fails, "\n".join(self.fails)


# ---- conditioning ----------------------------------------------------------------------------------------------------------------
def relu_conditioning(sd, taps):
    """Per BatchNorm stage of a training forward: fp64's ReLU mask on the device's own z against the device's mask.
    -> {layer: (elements compared, elements that differ, smallest, largest |pre-activation| / channel std among them, smallest over all)}."""
    out = {}
    for kind, name, i, o, ik in stages("train"):
        if kind not in ("bn", "bnpool"):
            continue
        gamma = torch.from_numpy(np.array(sd[f"bn{name}.weight"])).double()
        pre = bn_pre(_cpu(taps[i], F64), gamma, torch.from_numpy(np.array(sd[f"bn{name}.bias"])).double())[0]
        m64, y = pre > 0, _cpu(taps[o], F64)
        if kind == "bn":
            known, mgpu = torch.ones_like(m64), y > 0
        else:
            # the pooled tensor fixes the mask at its index position (positive there) and over the whole window where it is zero
            at = torch.zeros(*y.shape, 4, dtype=torch.bool).scatter(4, _cpu(taps[ik], F64).long()[..., None], True)
            known = _unwindows(at | (y == 0)[..., None])
            mgpu = _unwindows(at & (y > 0)[..., None])
        margin = pre.abs() / gamma.abs()
        diff = known & (m64 != mgpu)
        out[name] = (int(known.sum()), int(diff.sum()), float(margin[diff].min()) if bool(diff.any()) else float("inf"),
                     float(margin[diff].max()) if bool(diff.any()) else 0.0, float(margin[known].min()))
    return out


def _unwindows(w):
    B, h, ww, Cc, _ = w.shape
    return w.reshape(B, h, ww, Cc, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * h, 2 * ww, Cc)


def assert_conditioned(cond, what=""):
    bad = {k: v for k, v in cond.items() if v[1]}
    assert not bad, (f"{what}: fp64's ReLU mask on the device's own z differs from the device's in "
                     + ", ".join(f"{k}: {v[1]} of {v[0]} (|pre| / std {v[2]:.1e} .. {v[3]:.1e})" for k, v in bad.items())
                     + " -- at ~1e-7 an ill-conditioned fixture (change its seed), anything larger a defect")


def label_cap(l64, l32):
    """-> (fp64 labels, mask of the pixels whose fp64 top-two gap exceeds 4 x the fp32 reference's largest logit error)."""
    top = l64.double().topk(2, dim=-1).values
    return l64.argmax(-1), (top[..., 0] - top[..., 1]) > 4 * float((l32.double() - l64.double()).abs().max())


# ---- one fixture's whole check (the device test and, with the fp32 chain standing in for the device, the CPU power check) ----------
def _scalar(tab, what, got, r64, r32):
    e_g, e_32 = abs(float(got) - float(r64)) / abs(float(r64)), abs(float(r32) - float(r64)) / abs(float(r64))
    bound = max(C * e_32, FLOOR)
    tab.rows.append(f"{what:28s} {e_g:10.2e} {e_32:10.2e} {'':10s} {'':10s} {e_g / bound:8.3f}")
    tab.worst = max(tab.worst, (e_g / bound, what))
    if e_g > bound:
        tab.fails.append(f"{what}: {e_g:.3e} > max({C} x fp32 reference's {e_32:.3e}, {FLOOR:.0e})")


def _zero_bias_rule(tab, what, db, dw):
    """The bias of a convolution a BatchNorm follows: its gradient is analytically zero, rounding noise only."""
    ok = float(db.double().norm()) <= 1e-5 * float(dw.double().norm())
    tab.rows.append(f"{what:28s} {float(db.double().norm()):10.2e} {'(zero)':>10s} {'':10s} {'':10s} {float(db.double().norm()) / (1e-5 * float(dw.double().norm())):8.3f}")
    if not ok:
        tab.fails.append(f"{what}: norm {float(db.double().norm()):.3e} > 1e-5 x the weight gradient's {float(dw.double().norm()):.3e}")


def check_eval(tab, sd, x, taps, labels):
    """Every eval stage layer-local, the logits end to end against the forced fp64 forward, and the label map under ``label_cap``.
    ``taps``: the device's (any device; read on the CPU), ``labels`` [B,H,W]: the arg-max of the forward's own output."""
    assert list(taps) == tap_order("eval"), list(taps)
    T = {k: v.detach().cpu() for k, v in taps.items()}
    for kind, name, o, r64, r32, _ in layer_local(sd, T, "eval"):
        if kind == "pool":
            p, i = pool_exact(T["y" + name])
            tab.exact(o + " = max_pool2d", torch.equal(T[o], p))
            tab.exact("i" + name + " = its indices", torch.equal(T["i" + name], i))
        elif kind == "unpool":
            i = next(s[4] for s in stages("eval") if s[3] == o)
            src = next(s[2] for s in stages("eval") if s[3] == o)
            tab.exact(o + " = max_unpool2d", torch.equal(T[o], unpool_exact(T[src], T[i])))
        else:
            c = r64.shape[-1]
            tab.check(o, T[o][..., :c], r64, r32)
            if T[o].shape[-1] > c:
                tab.exact(o + " padding channels zero", not bool(T[o][..., c:].any()))
    idx = {k: v for k, v in T.items() if k[0] == "i"}
    l64 = eval_forward(sd, x, idx, F64)
    with _fixed_fp32_order():
        l32 = eval_forward(sd, x, idx, F32)
    tab.check("logits end to end", T["z11d"][..., :CLASSES], l64, l32)
    lab64, clear = label_cap(l64, l32)
    cover = float(clear.double().mean())
    tab.rows.append(f"{'labels':28s} fp64 top-two gap clear of 4 x the fp32 logit error on {100 * cover:.3f} % of the pixels")
    if cover < 0.999:
        tab.fails.append(f"labels: the cap covers {100 * cover:.3f} % < 99.9 % of the pixels -- ill-conditioned fixture")
    if not torch.equal(l32.argmax(-1)[clear], lab64[clear]):
        tab.fails.append("labels: the fp32 reference's own labels differ from fp64's inside the cap")
    if not torch.equal(labels.cpu()[clear], lab64[clear]):
        tab.fails.append(f"labels: {int((labels.cpu()[clear] != lab64[clear]).sum())} differ from fp64's inside the cap")


def check_train(tab, sd, x, target, taps, tap_grads, loss, param_grads, buffers, pool_input):
    """One training step: conditioning, every stage forward and backward layer-local, the running statistics per layer, the loss stage,
    and loss and parameter gradients end to end against the forced fp64 step.  ``tap_grads``: {tap: the device's gradient of it};
    ``param_grads`` / ``buffers``: the module's parameter gradients / buffers after the step by state-dict key; ``pool_input(layer, z)``:
    the device's own BatchNorm + ReLU output of a pooled layer (which the fused launch does not keep)."""
    assert list(taps) == tap_order("train"), list(taps)
    T = {k: v.detach().cpu() for k, v in taps.items()}
    G = {k: v.detach().cpu() for k, v in tap_grads.items()}
    PG = {k: v.detach().cpu() for k, v in param_grads.items()}
    assert_conditioned(relu_conditioning(sd, T), tab.title)
    src = {s[3]: s for s in stages("train")}
    for kind, name, o, r64, r32, bwd in layer_local(sd, T, "train", G):
        c = r64.shape[-1]
        i = src[o][2]
        if kind == "unpool":
            tab.exact(o + " = max_unpool2d", torch.equal(T[o], unpool_exact(T[i], T[src[o][4]])))
            tab.exact(f"d{i} <- d{o} gathered", torch.equal(G[i].double(), bwd["in"][0]))
            continue
        tab.check(o, T[o][..., :c], r64, r32)
        if T[o].shape[-1] > c:
            tab.exact(o + " padding channels zero", not bool(T[o][..., c:].any()))
        if kind == "bnpool":
            p, ix = pool_exact(pool_input(name, taps[i]).detach().cpu())
            tab.exact(o + " = max_pool2d", torch.equal(T[o], p))
            tab.exact("i" + name + " = its indices", torch.equal(T["i" + name], ix))
        if "in" in bwd:
            tab.check(f"d{i} <- d{o}", G[i][..., :bwd["in"][0].shape[-1]], *bwd["in"])
        for k in stage_params(kind, name):
            if k.startswith("conv") and k.endswith(".bias") and name != "11d":
                _zero_bias_rule(tab, "d" + k, PG[k], PG[k.replace(".bias", ".weight")])
            else:
                tab.check("d" + k, PG[k], *bwd[k], activation=False)
        if kind in ("bn", "bnpool"):
            r = {dt: running_stats(T[i].to(dt), *(torch.from_numpy(np.array(sd[f"bn{name}.running_{s}"])).to(dt) for s in ("mean", "var")))
                 for dt in (F64, F32)}
            tab.check(f"bn{name}.running_mean", buffers[f"bn{name}.running_mean"], r[F64][0], r[F32][0])
            tab.check(f"bn{name}.running_var", buffers[f"bn{name}.running_var"], r[F64][1], r[F32][1])
            nbt = int(buffers[f"bn{name}.num_batches_tracked"])
            tab.exact(f"bn{name}.num_batches_tracked", nbt == int(sd[f"bn{name}.num_batches_tracked"]) + 1)
    ll = loss_local(T["z11d"], target)
    _scalar(tab, "loss <- z11d", loss, *ll["loss"])
    tab.check("dz11d <- loss", G["z11d"][..., :CLASSES], *ll["dlogits"])
    tab.exact("dz11d padding channels zero", not bool(G["z11d"][..., CLASSES:].any()))
    idx = {k: v for k, v in T.items() if k[0] == "i"}
    masks = relu_masks(T)
    l64, g64, _ = train_step(sd, x, target, idx, F64, relu=masks)
    with _fixed_fp32_order():
        l32, g32, _ = train_step(sd, x, target, idx, F32, relu=masks)
    _scalar(tab, "loss end to end", loss, l64, l32)
    for k in g64:
        if k.startswith("conv") and k.endswith(".bias") and not k.startswith("conv11d."):
            continue                                      # held to the zero rule above
        tab.check("e2e d" + k, PG[k], g64[k], g32[k], activation=False)
