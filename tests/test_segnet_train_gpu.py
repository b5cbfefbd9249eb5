"""GPU: SegNet training (csrc/segtrain.hip, segtrain_ops, SegNet.train() forward, vanilla_segmentation/loss.py) -- the BatchNorm, pooling
and cross-entropy kernels against fp64 torch, one full training step against an fp64 functional restatement and against the golden
of the imported reference (tools/dev/make_segnet_train_golden.py), eval after FlatAdam steps, learning and determinism."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from densefusion_amd import synth
from oracle_segnet import MEAN, STD, _frame

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = torch.device("cuda:0")
SEG = synth._SEG_LAYERS
ENC_POOL = {"12", "22", "33", "43", "53"}            # the layers a max-pool follows
DEC_UNPOOL = {"53d", "43d", "33d", "22d", "12d"}     # the layers an un-pool precedes


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    n = float(b.norm())
    return float((a - b).norm()) / (n if n > 0 else 1.0)


# ---- 1. BatchNorm + ReLU ---------------------------------------------------------------------------------------------------------
def _bn_relu_case(C, rows, shift, fp32_envelope):
    """BatchNormReLU forward and backward on z [rows, C] against fp64, every output within rel < 1e-5 -- or, with ``fp32_envelope``,
    within max(4 x the error of fp32 CPU F.batch_norm + autograd on the same inputs, 1e-5); the kernel's own mean / variance outputs;
    bit-identical reruns."""
    from densefusion_amd.segtrain_ops import BatchNormReLU
    g = torch.Generator().manual_seed(C + rows)
    z = (torch.randn(1, 1, rows, C, generator=g) * torch.rand(C, generator=g).add(0.5) + shift + torch.randn(C, generator=g)).float()
    gamma = torch.rand(C, generator=g).add(0.5)
    beta = torch.randn(C, generator=g) * 0.3
    dy = torch.randn(1, 1, rows, C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g).add(0.5)

    def run():
        rm, rv, nbt = rm0.clone().to(DEV), rv0.clone().to(DEV), torch.tensor(7, dtype=torch.int64, device=DEV)
        zz = z.to(DEV).requires_grad_(True)
        ga, be = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
        y = BatchNormReLU.apply(zz, ga, be, rm, rv, nbt, 0.1, 1e-5)
        y.backward(dy.to(DEV))
        return [t.detach().cpu() for t in (y, zz.grad, ga.grad, be.grad, rm, rv, nbt)]

    y, dz, dg, db, rm, rv, nbt = run()
    z64 = z.double().reshape(rows, C).requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mu, var = z64.mean(0), z64.var(0, unbiased=False)
    y64 = F.relu((z64 - mu) / torch.sqrt(var + 1e-5) * g64 + b64)
    y64.backward(dy.double().reshape(rows, C))
    wants = (y64, z64.grad, g64.grad, b64.grad, 0.9 * rm0.double() + 0.1 * mu, 0.9 * rv0.double() + 0.1 * z64.var(0, unbiased=True))
    bounds = [1e-5] * 6
    if fp32_envelope:
        z32 = z.reshape(rows, C).clone().requires_grad_(True)
        g32, b32 = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        rm32, rv32 = rm0.clone(), rv0.clone()
        y32 = F.relu(F.batch_norm(z32.t()[None], rm32, rv32, g32, b32, training=True, momentum=0.1, eps=1e-5))[0].t()
        y32.backward(dy.reshape(rows, C))
        bounds = [max(4 * rel(a, b.detach()), 1e-5) for a, b in zip((y32.detach(), z32.grad, g32.grad, b32.grad, rm32, rv32), wants)]
    names = ("y", "dz", "dgamma", "dbeta", "running_mean", "running_var")
    errs = [rel(got.reshape(want.shape), want.detach()) for got, want in zip((y, dz, dg, db, rm, rv), wants)]
    print(f"C {C} rows {rows} shift {shift}: " + ", ".join(f"{n} {e:.1e} (< {b:.1e})" for n, e, b in zip(names, errs, bounds)))
    for n, e, b in zip(names, errs, bounds):
        assert e < b, (n, e, b)
    assert int(nbt) == 8
    # mean / variance outputs of the kernel itself
    from densefusion_amd.segtrain_ops import _bn_fwd
    with torch.no_grad():
        _, m2, v, _ = _bn_fwd(z.to(DEV).contiguous(), gamma.to(DEV), beta.to(DEV), None, None, None, 0.1, 1e-5)
    assert rel(m2[:C].double().cpu() + m2[C:].double().cpu(), mu.detach()) < 1e-12 + 1e-9 * (1 + shift)
    assert rel(v.cpu(), var.detach()) < 1e-6
    again = run()
    assert all(torch.equal(a, b) for a, b in zip(again, (y, dz, dg, db, rm, rv, nbt)))          # bit-identical reruns


@pytest.mark.parametrize("C,rows,shift", [(64, 19200, 0.0), (128, 4801, 0.0), (512, 3600, 0.0), (64, 4801, 1e3), (512, 3600, 1e3)])
def test_bn_relu_against_fp64(C, rows, shift):
    _bn_relu_case(C, rows, shift, fp32_envelope=False)


# The statistics passes give lane t channels 4 (t % c4) .. +3 (c4 = C / 4) and rows t / c4, + rpi, ... (rpi = 256 // c4); they run
# ceil(rows / (16 rpi)) workgroups, at most 1024, and the finish passes take 16 channels per workgroup.  The shapes: C below 16 and no
# multiple of 16 (a finish workgroup partly idle); c4 = 3 and 129, which do not divide 256 (idle lanes: lane 255 at C = 12, 127 of 256
# at C = 516); the largest C; rows on both sides of the first grid step (16 rpi: 4096 at C = 4, 1360 at C = 12, 256 at C = 64, 64 at
# C = 256); fewer rows than lanes of a channel group; rows past the workgroup cap at rpi = 2 (32 x 1024 = 32768); a mean of 1e3 on
# the smallest of them.
BN_EDGES = [(4, 2), (4, 4095), (4, 4096), (4, 4097), (12, 3), (12, 1359), (12, 1361), (24, 2000), (64, 255), (64, 256), (64, 257),
            (256, 4), (256, 63), (256, 65), (516, 17), (1024, 2), (1024, 33), (512, 40000)]


@pytest.mark.parametrize("C,rows,shift", [(c, r, 0.0) for c, r in BN_EDGES] + [(512, 4, 1e3), (12, 3, 1e3)])
def test_bn_relu_edge_shapes_against_fp64(C, rows, shift):
    _bn_relu_case(C, rows, shift, fp32_envelope=True)


def test_bn_relu_one_row():
    """rows = 1 (torch refuses it): the rule the kernel documents.  The batch variance is 0 and xhat is 0, so y = relu(beta),
    running_var <- (1 - m) running_var + m * 0 (no unbiased factor), dz = 0, dgamma = 0 and dbeta = dy where beta > 0."""
    from densefusion_amd.segtrain_ops import BatchNormReLU
    C = 64
    g = torch.Generator().manual_seed(65)
    z, dy = torch.randn(1, 1, 1, C, generator=g) * 3 + 1, torch.randn(1, 1, 1, C, generator=g)
    gamma, beta = torch.rand(C, generator=g).add(0.5), torch.randn(C, generator=g) * 0.3
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g).add(0.5)
    rm, rv, nbt = rm0.to(DEV), rv0.to(DEV), torch.tensor(7, dtype=torch.int64, device=DEV)
    zz, ga, be = z.to(DEV).requires_grad_(True), gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    y = BatchNormReLU.apply(zz, ga, be, rm, rv, nbt, 0.1, 1e-5)
    y.backward(dy.to(DEV))
    assert torch.equal(y.detach().cpu().reshape(C), F.relu(beta))
    assert torch.equal(zz.grad.cpu(), torch.zeros_like(z)) and torch.equal(ga.grad.cpu(), torch.zeros(C))
    assert torch.equal(be.grad.cpu(), torch.where(beta > 0, dy.reshape(C), torch.zeros(C)))
    assert rel(rm, 0.9 * rm0.double() + 0.1 * z.double().reshape(C)) < 1e-7
    assert rel(rv, 0.9 * rv0.double()) < 1e-7
    assert int(nbt) == 8


@pytest.mark.parametrize("B,H,W,C", [(1, 2, 2, 512), (2, 2, 4, 12), (1, 6, 10, 64)])
def test_bn_relu_maxpool_backward_against_fp64_with_the_index_forced(B, H, W, C):
    """The pooled-gradient path of df_bn_relu_bwd against fp64 autograd of BatchNorm + ReLU + the gather at the kernel's own pool index
    (oracle_segnet.pool_forced), within max(4 x the same in fp32 on the CPU, 1e-5) like the BatchNorm cases above, the index itself
    against torch's max-pool of the unfused BatchNormReLU output, and bit-equal with the unfused pair."""
    import oracle_segnet as osn
    from densefusion_amd.segtrain_ops import BatchNormReLU, BatchNormReLUMaxPool, MaxPool2x2Idx
    g = torch.Generator().manual_seed(B * H * W + C)
    z = torch.randn(B, H, W, C, generator=g) * torch.rand(C, generator=g).add(0.5) + torch.randn(C, generator=g)
    gamma, beta = torch.rand(C, generator=g).add(0.5), torch.randn(C, generator=g) * 0.3
    dp = torch.randn(B, H // 2, W // 2, C, generator=g)
    outs = []
    for fused in (True, False):
        zz, g_, b_ = z.to(DEV).requires_grad_(True), gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
        if fused:
            p, idx = BatchNormReLUMaxPool.apply(zz, g_, b_, None, None, None, 0.1, 1e-5)
        else:
            full = BatchNormReLU.apply(zz, g_, b_, None, None, None, 0.1, 1e-5)
            p, idx = MaxPool2x2Idx.apply(full)
        p.backward(dp.to(DEV))
        outs.append([t.detach().cpu() for t in (p, idx, zz.grad, g_.grad, b_.grad)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    p, idx, dz, dg, db = outs[0]
    pe, ie = osn.pool_exact(full.detach().cpu())
    assert torch.equal(p, pe) and torch.equal(idx, ie)
    refs = {}
    for dt in (torch.float64, torch.float32):
        z_, g_, b_ = (t.to(dt).requires_grad_(True) for t in (z, gamma, beta))
        pr = osn.pool_forced(osn.bn_relu(z_, g_, b_), idx)
        refs[dt] = (pr.detach(),) + torch.autograd.grad(pr, (z_, g_, b_), dp.to(dt))
    for n, got, w64, w32 in zip(("pooled", "dz", "dgamma", "dbeta"), (p, dz, dg, db), refs[torch.float64], refs[torch.float32]):
        bound = max(4 * rel(w32, w64), 1e-5)
        print(f"{(B, H, W, C)} {n}: {rel(got, w64):.1e} (< {bound:.1e})")
        assert rel(got, w64) < bound, n


def test_bn_relu_maxpool_fused_matches_unfused():
    from densefusion_amd.segtrain_ops import BatchNormReLU, BatchNormReLUMaxPool, MaxPool2x2Idx
    torch.manual_seed(3)
    z = torch.randn(2, 12, 16, 64, device=DEV)
    ga, be = torch.rand(64, device=DEV) + 0.5, torch.randn(64, device=DEV) * 0.5
    dp = torch.randn(2, 6, 8, 64, device=DEV)
    outs = []
    for fused in (True, False):
        zz, g_, b_ = z.clone().requires_grad_(True), ga.clone().requires_grad_(True), be.clone().requires_grad_(True)
        if fused:
            p, idx = BatchNormReLUMaxPool.apply(zz, g_, b_, None, None, None, 0.1, 1e-5)
        else:
            p, idx = MaxPool2x2Idx.apply(BatchNormReLU.apply(zz, g_, b_, None, None, None, 0.1, 1e-5))
        p.backward(dp)
        outs.append((p, idx, zz.grad, g_.grad, b_.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- 2. pooling adjoints ---------------------------------------------------------------------------------------------------------
def test_pool_adjoints_bit_exact():
    from densefusion_amd.segtrain_ops import MaxPool2x2Idx, MaxUnpool2x2
    torch.manual_seed(1)
    # the last two: one window per channel group (a 1 x 1 pooled map), and C = 12 with one row of windows per image
    for B, H, W, C in ((2, 8, 12, 16), (1, 2, 2, 4), (3, 2, 6, 12)):
        _pool_adjoints_case(B, H, W, C)


def _pool_adjoints_case(B, H, W, C):
    from densefusion_amd.segtrain_ops import MaxPool2x2Idx, MaxUnpool2x2
    x = F.relu(torch.randn(B, H, W, C, device=DEV)).round()                    # ReLU zeros and rounding: many tied windows
    dy = torch.randn(B, H // 2, W // 2, C, device=DEV)
    xx = x.clone().requires_grad_(True)
    y, idx = MaxPool2x2Idx.apply(xx)
    y.backward(dy)
    xr = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    yr, ir = F.max_pool2d(xr, 2, 2, return_indices=True)
    yr.backward(dy.permute(0, 3, 1, 2))
    assert torch.equal(y.permute(0, 3, 1, 2), yr) and torch.equal(xx.grad.permute(0, 3, 1, 2), xr.grad)
    # un-pool: forward and its gather adjoint
    v = y.detach().clone().requires_grad_(True)
    up = MaxUnpool2x2.apply(v, idx)
    du = torch.randn_like(up)
    up.backward(du)
    vr = yr.detach().clone().requires_grad_(True)
    upr = F.max_unpool2d(vr, ir, 2, 2)
    upr.backward(du.permute(0, 3, 1, 2))
    assert torch.equal(up.permute(0, 3, 1, 2), upr) and torch.equal(v.grad.permute(0, 3, 1, 2), vr.grad)


# ---- 3. cross-entropy ------------------------------------------------------------------------------------------------------------
def test_cross_entropy_against_fp64():
    from densefusion_amd.segtrain_ops import CrossEntropyNHWC
    torch.manual_seed(2)
    B, H, W, K = 2, 32, 48, 22
    for scale in (3.0, 80.0):
        logits = torch.randn(B, H, W, 24, device=DEV) * scale
        if scale == 80.0:
            logits = logits.clamp(-80, 80).sign() * 80                          # +-80 everywhere
        target = torch.randint(0, K, (B, H, W), device=DEV)
        lg = logits.clone().requires_grad_(True)
        loss = CrossEntropyNHWC.apply(lg, target, K)
        loss.backward()
        l64 = logits[..., :K].double().cpu().reshape(-1, K).requires_grad_(True)
        want = F.cross_entropy(l64, target.cpu().reshape(-1))
        want.backward()
        assert torch.isfinite(loss) and torch.isfinite(lg.grad).all()
        assert abs(float(loss.detach()) - float(want)) <= 1e-6 * abs(float(want))
        assert rel(lg.grad[..., :K].reshape(-1, K), l64.grad) < 1e-6
        assert torch.equal(lg.grad[..., K:], torch.zeros_like(lg.grad[..., K:]))
    bad = target.clone()
    bad[1, 3, 5] = K
    with pytest.raises(ValueError):
        CrossEntropyNHWC.apply(logits, bad, K)
    bad[1, 3, 5] = -1
    with pytest.raises(ValueError):
        CrossEntropyNHWC.apply(logits, bad, K)
    again = CrossEntropyNHWC.apply(logits, target, K)                           # the process and the flag are fine afterwards
    assert torch.isfinite(again)


def _ce_case(rows, classes, ld, logits):
    """loss within 1e-6 relative and gradient within rel < 1e-6 of fp64 F.cross_entropy, the padding channels exactly zero."""
    from densefusion_amd.segtrain_ops import CrossEntropyNHWC
    target = torch.randint(0, classes, (rows,), generator=torch.Generator().manual_seed(rows + ld))
    lg = logits.to(DEV).requires_grad_(True)
    loss = CrossEntropyNHWC.apply(lg, target.to(DEV), classes)
    loss.backward()
    l64 = logits[:, :classes].double().requires_grad_(True)
    want = F.cross_entropy(l64, target)
    want.backward()
    grad = lg.grad.cpu()
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    print(f"rows {rows} classes {classes} ld {ld}: loss {float(loss):.7f} vs {float(want):.7f}, gradient {rel(grad[:, :classes], l64.grad):.1e}")
    assert abs(float(loss.detach()) - float(want)) <= 1e-6 * abs(float(want))
    assert rel(grad[:, :classes], l64.grad) < 1e-6
    assert torch.equal(grad[:, classes:], torch.zeros(rows, ld - classes))
    return target


# rows: one row, one workgroup of 256 less / exactly / plus one row, and 2048 * 256 + 259 (the grid of at most 2048 workgroups wraps);
# (classes, ld): the trainer's own (22 classes in the classifier's 32 padded channels), the loss module's (22 in 24), no padding at
# all, two classes
@pytest.mark.parametrize("rows,classes,ld", [(1, 22, 32), (255, 22, 32), (256, 22, 32), (257, 22, 32), (524547, 22, 32),
                                             (257, 2, 4), (257, 22, 24), (257, 32, 32)])
def test_cross_entropy_edge_shapes_against_fp64(rows, classes, ld):
    from densefusion_amd.segtrain_ops import CrossEntropyNHWC
    logits = torch.randn(rows, ld, generator=torch.Generator().manual_seed(rows * ld + classes)) * 3.0
    target = _ce_case(rows, classes, ld, logits)
    if rows == 524547:
        bad = target.clone()
        bad[-1] = classes                       # the last row, which only the wrapped grid stride reaches
        with pytest.raises(ValueError):
            CrossEntropyNHWC.apply(logits.to(DEV), bad.to(DEV), classes)
    if (rows, classes, ld) == (257, 22, 32):
        _ce_case(rows, classes, ld, torch.randn(rows, ld, generator=torch.Generator().manual_seed(5)).sign() * 80)      # +-80 everywhere


def test_cross_entropy_one_class():
    """classes = 1: every row's softmax is 1 on its label, so the loss and the gradient are exactly zero."""
    from densefusion_amd.segtrain_ops import CrossEntropyNHWC
    logits = (torch.randn(257, 4, generator=torch.Generator().manual_seed(6)) * 3.0).to(DEV).requires_grad_(True)
    loss = CrossEntropyNHWC.apply(logits, torch.zeros(257, dtype=torch.int64, device=DEV), 1)
    loss.backward()
    assert float(loss) == 0.0 and torch.equal(logits.grad, torch.zeros_like(logits))


# ---- the fp64 functional restatement of one training step ------------------------------------------------------------------------
def restate_step(sd, x, target, dtype, lr=1e-4):
    """nn.functional restatement of SegNet's train() forward, loss, backward and one Adam step (CPU) -> loss, grads, state after."""
    p = {k: torch.from_numpy(np.array(v)).to(dtype) for k, v in sd.items()}          # copies: the Adam step below updates in place
    params = {k: v.requires_grad_(True) for k, v in p.items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    bufs = {k: p[k].clone() for k in p if k.endswith(("running_mean", "running_var"))}
    a = x.to(dtype)
    idx = []
    for name, _, _ in SEG:
        if name in DEC_UNPOOL:
            a = F.max_unpool2d(a, idx.pop(), 2, 2)
        a = F.conv2d(a, params[f"conv{name}.weight"], params[f"conv{name}.bias"], padding=1)
        if name == "11d":
            break
        a = F.relu(F.batch_norm(a, bufs[f"bn{name}.running_mean"], bufs[f"bn{name}.running_var"], params[f"bn{name}.weight"],
                                params[f"bn{name}.bias"], training=True, momentum=0.1, eps=1e-5))
        if name in ENC_POOL:
            a, i = F.max_pool2d(a, 2, 2, return_indices=True)
            idx.append(i)
    loss = F.cross_entropy(a, target)
    loss.backward()
    grads = {k: v.grad.detach().clone() for k, v in params.items()}
    opt = torch.optim.Adam(list(params.values()), lr=lr)
    opt.step()
    after = {k: v.detach().clone() for k, v in params.items()}
    after.update(bufs)
    return float(loss), grads, after


def gpu_step(sd, x, target, steps=1, lr=1e-4):
    from densefusion_amd.train_utils import FlatAdam, FlatParams
    from densefusion_amd.vanilla_segmentation.loss import Loss
    from densefusion_amd.vanilla_segmentation.segnet import SegNet
    net = SegNet(trainable=True)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    net = net.to(DEV).train()
    flat = FlatParams(net)
    opt = FlatAdam(flat, lr=lr)
    crit = Loss()
    losses, grads = [], None
    for _ in range(steps):
        flat.zero_grad()
        loss = crit(net(x.to(DEV)), target.to(DEV))
        loss.backward()
        losses.append(float(loss))
        grads = {k: v.grad.detach().cpu().double() for k, v in net.named_parameters()}
        opt.step()
    return net, losses, grads, opt


def _is_bn_bias(k):
    return k.startswith("conv") and k.endswith(".bias") and not k.startswith("conv11d.")


# ---- 4. one step against the fp64 restatement ------------------------------------------------------------------------------------
def test_training_step_against_fp64_restatement():
    sd = synth.make_segnet_state_dict(23)
    x, target = _frame(5, 2, 96, 128)
    l64, g64, a64 = restate_step(sd, x, target, torch.float64)
    l32, g32, a32 = restate_step(sd, x, target, torch.float32)
    net, losses, g, _ = gpu_step(sd, x, target)
    assert abs(losses[0] - l64) <= 1e-5 * abs(l64)
    ratios = {}
    for k in g64:
        if _is_bn_bias(k):
            # analytically zero (the BatchNorm after the conv removes any per-channel shift): rounding noise only
            assert float(g[k].norm()) <= 1e-5 * float(g[k.replace(".bias", ".weight")].norm()), k
            continue
        env = max(rel(g32[k], g64[k]), 1e-7)
        ratios[k] = rel(g[k], g64[k]) / env
    state = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    for k in a64:
        if _is_bn_bias(k):
            continue                      # Adam turns the rounding noise of a zero gradient into +-lr steps, in the reference too
        if k not in g64:                                      # running statistics
            env = max(rel(a32[k], a64[k]), 1e-7)
            ratios["after/" + k] = rel(state[k], a64[k]) / env
            continue
        # Parameters after the step, on the entries whose fp64 gradient stands clear of both fp32 runs' largest error: Adam's first
        # step is ~ -lr sign(g), so an entry whose gradient lies within the rounding noise moves by +-lr whichever sign the noise
        # takes, and the GPU's noise is not the CPU's (measured: 2e-4 relative on bn41d.bias, 1900x the CPU's, from such entries).
        # The golden test below bounds the full update against the reference's own fp32-vs-fp64 envelope.
        noise = float((g32[k].double() - g64[k]).abs().max()) + float((g[k] - g64[k]).abs().max())
        m = g64[k].abs() > 2 * noise
        if not bool(m.any()):
            continue
        env = max(rel(a32[k][m], a64[k][m]), 1e-7)
        ratios["after/" + k] = rel(state[k][m], a64[k][m]) / env
    # measured on MI355X: at most 1.16x the CPU fp32 envelope (bn52.running_mean); gradients and parameters below 1.1x
    worst = sorted(ratios.items(), key=lambda kv: -kv[1])[:5]
    print("largest error / fp32-CPU envelope:", worst)
    assert all(r <= 4.0 for r in ratios.values()), worst
    assert all(int(state[f"bn{n}.num_batches_tracked"]) == 101 for n, _, _ in SEG if n != "11d")


# ---- 5. the golden of the imported reference at 480 x 640 ------------------------------------------------------------------------
def test_training_step_against_reference_golden():
    gd = np.load(os.path.join(G, "segnet_train_step.npz"))
    seed, H, W, samples = (int(v) for v in gd["meta"])

    def positions(numel, stored):
        """the entries a stored vector holds: all of them, or `samples` evenly spaced (tools/dev/make_segnet_train_golden.py)"""
        if stored == numel:
            return torch.arange(numel)
        return torch.from_numpy(np.linspace(0, numel - 1, samples).round().astype(np.int64))

    sd = synth.make_segnet_state_dict(seed)
    x = torch.from_numpy(((gd["x_u8"].astype(np.float32) - MEAN[:, None, None]) / STD[:, None, None]).astype(np.float32))[None]
    target = torch.from_numpy(gd["target"].astype(np.int64))[None]
    net, losses, g, _ = gpu_step(sd, x, target)
    assert abs(losses[0] - float(gd["loss"][0])) <= 1e-5 * abs(float(gd["loss"][0]))
    state = {k: v.detach().cpu().double() for k, v in net.state_dict().items()}
    ratios, masked = {}, {}
    for key in gd.files:
        if not key.startswith("env/"):
            continue
        kind, k = key.split("/", 2)[1:]
        env = max(float(gd[key]), 1e-7)
        if kind == "after":                                   # BatchNorm running statistics
            ratios[key] = rel(state[k], torch.from_numpy(gd["after/" + k])) / env
            continue
        if _is_bn_bias(k):
            continue
        if kind == "grad":
            pos = positions(g[k].numel(), gd["grad/" + k].size)
            ratios[key] = rel(g[k].reshape(-1)[pos], torch.from_numpy(gd["grad/" + k])) / env
        else:
            # the Adam update, on the entries whose fp64 gradient stands clear of the gradient noise the test allows (4 x the
            # reference's own fp32 error, as an RMS per entry): the first step is ~ -lr sign(g), so an entry whose gradient lies
            # within that noise moves by +-lr whichever sign the noise takes (measured: bn11.bias 1.5e4 x the reference's envelope
            # otherwise, from such entries)
            g64 = torch.from_numpy(gd["grad/" + k]).double()
            noise = 4 * float(gd["env/grad/" + k]) * float(g64.pow(2).mean().sqrt())
            gpos = positions(g[k].numel(), gd["grad/" + k].size)
            pos = positions(g[k].numel(), gd["after/" + k].size)
            g64 = g64[pos] if gpos.numel() != pos.numel() else g64
            m = g64.abs() > noise
            masked[k] = int((~m).sum())
            w0 = torch.from_numpy(np.asarray(sd[k])).double().reshape(-1)[pos][m]
            ratios[key] = rel(state[k].reshape(-1)[pos][m] - w0, torch.from_numpy(gd["after/" + k]).double()[m] - w0) / env
    # measured on MI355X: at most 1.78x the reference's envelope (bn53d.running_mean); gradients and updates below 1.3x, the
    # update checked on about half of the entries of each tensor (the rest lie within the allowed gradient noise)
    worst = sorted(ratios.items(), key=lambda kv: -kv[1])[:5]
    print("largest error / fp32-vs-fp64 envelope of the reference:", worst, "entries left out of the update check:",
          {k: v for k, v in masked.items() if v})
    assert all(r <= 4.0 for r in ratios.values()), worst


# ---- 6. eval sees the trained weights --------------------------------------------------------------------------------------------
def test_eval_after_flat_adam_steps():
    from densefusion_amd.vanilla_segmentation.segnet import SegNet

    def fresh_logits(net, x):
        other = SegNet()
        other.load_state_dict(net.state_dict())
        return other.to(DEV).eval()(x)

    sd = synth.make_segnet_state_dict(8)
    x, target = _frame(9, 2, 64, 96)
    x = x.to(DEV)
    net, _, _, opt = gpu_step(sd, x, target, steps=3)
    net.eval()
    y3 = net(x)                                                        # fills the BatchNorm-folded weight cache
    assert torch.equal(y3, fresh_logits(net, x))
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == synth.segnet_spec()
    opt.step()                                 # a 4th step on the last gradients, straight after an eval forward: the cache is stale now
    y4 = net(x)
    assert not torch.equal(y4, y3)
    assert torch.equal(y4, fresh_logits(net, x))


# ---- 7. learning and determinism -------------------------------------------------------------------------------------------------
def test_learns_and_is_deterministic():
    sd = synth.make_segnet_state_dict(12)
    x, target = _frame(13, 2, 64, 96)
    _, l1, _, _ = gpu_step(sd, x, target, steps=30, lr=1e-3)
    _, l2, _, _ = gpu_step(sd, x, target, steps=30, lr=1e-3)
    print("losses", l1[0], l1[-1])
    assert l1[-1] * 2 <= l1[0]
    assert l1 == l2


# ---- training is opt-in ----------------------------------------------------------------------------------------------------------
def test_training_is_opt_in():
    from densefusion_amd.vanilla_segmentation.segnet import SegNet
    x = torch.zeros(1, 3, 64, 64, device=DEV)
    plain = SegNet().to(DEV).train()
    with pytest.raises(NotImplementedError):
        plain(x)                                                           # the inference-only default is unchanged
    plain.trainable = True
    y = plain(x)
    assert y.shape == (1, 22, 64, 64) and y.requires_grad
    assert "trainable" not in "".join(plain.state_dict())
