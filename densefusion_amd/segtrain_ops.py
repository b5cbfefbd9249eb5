"""Autograd Functions of the SegNet training tape (csrc/segtrain.hip, csrc/trainops.hip): BatchNorm2d in training mode fused with
its ReLU (optionally with the 2x2 max-pool that follows it), the 2x2 max-pool / un-pool pair and the cross-entropy loss over
channels-last logits.  As in train_ops, torch.autograd is only the tape: every forward and backward is a HIP launch through the C ABI.
"""
from __future__ import annotations

import torch

from . import _lib


def _st():
    return _lib.current_stream()


def _ck(rc, what):
    _lib.check(rc, what)


# optional per-launch timing of the layers below (tools/segnet_train_bench.py): events on the launch stream, kind -> [(start, end)]
_PROFILE = None


def profile_begin():
    global _PROFILE
    _PROFILE = {"bn_fwd": [], "bn_bwd": [], "pool": [], "unpool": [], "ce": []}


def profile_end():
    """-> {kind: (milliseconds, launches)} since profile_begin(); synchronises."""
    global _PROFILE
    prof, _PROFILE = _PROFILE, None
    torch.cuda.synchronize()
    return {k: (sum(a.elapsed_time(b) for a, b in v), len(v)) for k, v in prof.items()}


class _Timed:
    def __init__(self, kind):
        self.kind = kind

    def __enter__(self):
        if _PROFILE is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if _PROFILE is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            _PROFILE[self.kind].append((self.a, b))
        return False


def _bn_ws(rows, C, device):
    need = int(_lib.lib().df_bn_workspace_bytes(rows, C))
    if need == 0:
        raise RuntimeError(f"BatchNormReLU: unsupported shape (rows {rows}, C {C}): C must be a multiple of 4 in [4, 1024]")
    return torch.empty(need, dtype=torch.uint8, device=device)


def _bn_fwd(z, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps):
    C = z.shape[-1]
    rows = z.numel() // C
    mean = torch.empty(2 * C, device=z.device)             # fp32 mean, then its residual (df_bn_relu_fwd_train)
    var = torch.empty(C, device=z.device)
    invstd = torch.empty(C, device=z.device)
    y = torch.empty_like(z)
    ws = _bn_ws(rows, C, z.device)
    for t in (running_mean, running_var, num_batches_tracked):
        if t is not None and not (t.is_cuda and t.is_contiguous()):
            raise RuntimeError("BatchNormReLU: the running-statistics buffers must be contiguous device tensors")
    with _Timed("bn_fwd"):
        _ck(_lib.lib().df_bn_relu_fwd_train(_lib.dptr(z), y.data_ptr(), _lib.dptr(gamma), _lib.dptr(beta),
                                            running_mean.data_ptr() if running_mean is not None else None,
                                            running_var.data_ptr() if running_var is not None else None,
                                            num_batches_tracked.data_ptr() if num_batches_tracked is not None else None,
                                            mean.data_ptr(), var.data_ptr(), invstd.data_ptr(), rows, C, float(momentum), float(eps),
                                            ws.data_ptr(), ws.numel(), _st()), "bn_relu_fwd_train")
    return y, mean, var, invstd


def _bn_bwd(dy, idx, z, mean, invstd, gamma, beta):
    B, H, W, C = z.shape
    rows = B * H * W
    dz = torch.empty_like(z)
    dgamma = torch.empty(C, device=z.device)
    dbeta = torch.empty(C, device=z.device)
    ws = _bn_ws(rows, C, z.device)
    with _Timed("bn_bwd"):
        _ck(_lib.lib().df_bn_relu_bwd(dy.data_ptr(), idx.data_ptr() if idx is not None else None, H, W, z.data_ptr(), mean.data_ptr(),
                                      invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dz.data_ptr(), dgamma.data_ptr(),
                                      dbeta.data_ptr(), rows, C, ws.data_ptr(), ws.numel(), _st()), "bn_relu_bwd")
    return dz, dgamma, dbeta


def _pool(y):
    B, H, W, C = y.shape
    p = torch.empty(B, H // 2, W // 2, C, device=y.device)
    idx = torch.empty(B, H // 2, W // 2, C, dtype=torch.uint8, device=y.device)
    with _Timed("pool"):
        _ck(_lib.lib().df_maxpool2x2_idx(y.data_ptr(), p.data_ptr(), idx.data_ptr(), B, H, W, C, _st()), "maxpool2x2_idx")
    return p, idx


class BatchNormReLU(torch.autograd.Function):
    """relu(BatchNorm2d(z)) in training mode over channels-last z [B,H,W,C] (batch statistics over B H W, the running buffers updated
    in place as nn.BatchNorm2d does).  Saves z and the batch mean / invstd, not y: the backward recomputes the ReLU mask."""

    @staticmethod
    def forward(ctx, z, gamma, beta, running_mean, running_var, num_batches_tracked, momentum=0.1, eps=1e-5):
        z = z.contiguous()
        with _lib.device_guard(z.device):
            y, mean, _, invstd = _bn_fwd(z, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps)
        ctx.save_for_backward(z, mean, invstd, gamma, beta)
        return y

    @staticmethod
    def backward(ctx, dy):
        z, mean, invstd, gamma, beta = ctx.saved_tensors
        with _lib.device_guard(z.device):
            dz, dgamma, dbeta = _bn_bwd(dy.contiguous(), None, z, mean, invstd, gamma, beta)
        return dz, dgamma, dbeta, None, None, None, None, None


class BatchNormReLUMaxPool(torch.autograd.Function):
    """The encoder's stage end, maxpool2x2(relu(BatchNorm2d(z))) -> (pooled [B,H/2,W/2,C], index uint8).  The backward reads the
    pooled gradient through the index inside the BatchNorm adjoint: the full-size, mostly zero gradient is never written."""

    @staticmethod
    def forward(ctx, z, gamma, beta, running_mean, running_var, num_batches_tracked, momentum=0.1, eps=1e-5):
        z = z.contiguous()
        if z.shape[1] % 2 or z.shape[2] % 2:
            raise RuntimeError(f"BatchNormReLUMaxPool: H and W must be even, got {tuple(z.shape)}")
        with _lib.device_guard(z.device):
            y, mean, _, invstd = _bn_fwd(z, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps)
            p, idx = _pool(y)
        ctx.mark_non_differentiable(idx)
        ctx.save_for_backward(z, mean, invstd, gamma, beta, idx)
        return p, idx

    @staticmethod
    def backward(ctx, dp, _didx):
        z, mean, invstd, gamma, beta, idx = ctx.saved_tensors
        with _lib.device_guard(z.device):
            dz, dgamma, dbeta = _bn_bwd(dp.contiguous(), idx, z, mean, invstd, gamma, beta)
        return dz, dgamma, dbeta, None, None, None, None, None


class MaxPool2x2Idx(torch.autograd.Function):
    """F.max_pool2d(x, 2, 2, return_indices=True) on channels-last x -> (y, index uint8, the 0..3 position in the window).  The
    backward is the un-pool of the gradient (df_maxunpool2x2): bit-exact with ATen, ties included (first maximum wins)."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        with _lib.device_guard(x.device):
            y, idx = _pool(x)
        ctx.mark_non_differentiable(idx)
        ctx.save_for_backward(idx)
        return y, idx

    @staticmethod
    def backward(ctx, dy, _didx):
        (idx,) = ctx.saved_tensors
        B, H, W, C = idx.shape
        dy = dy.contiguous()
        dx = torch.empty(B, 2 * H, 2 * W, C, device=dy.device)
        with _lib.device_guard(dy.device), _Timed("unpool"):
            _ck(_lib.lib().df_maxunpool2x2(dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), B, H, W, C, _st()), "maxunpool2x2")
        return dx


class MaxUnpool2x2(torch.autograd.Function):
    """F.max_unpool2d(x, idx, 2, 2) on channels-last x [B,H,W,C] -> [B,2H,2W,C]; the backward gathers the gradient at the index
    (df_maxunpool2x2_bwd)."""

    @staticmethod
    def forward(ctx, x, idx):
        x = x.contiguous()
        B, H, W, C = x.shape
        y = torch.empty(B, 2 * H, 2 * W, C, device=x.device)
        with _lib.device_guard(x.device), _Timed("unpool"):
            _ck(_lib.lib().df_maxunpool2x2(x.data_ptr(), _lib.dptr(idx), y.data_ptr(), B, H, W, C, _st()), "maxunpool2x2")
        ctx.save_for_backward(idx)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        B, H, W, C = idx.shape
        dy = dy.contiguous()
        dx = torch.empty(B, H, W, C, device=dy.device)
        with _lib.device_guard(dy.device), _Timed("unpool"):
            _ck(_lib.lib().df_maxunpool2x2_bwd(dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), B, H, W, C, _st()), "maxunpool2x2_bwd")
        return dx, None


class CrossEntropyNHWC(torch.autograd.Function):
    """nn.CrossEntropyLoss()(logits, target) with the logits channels-last [..., ld] (the first `classes` channels are the classes,
    the rest padding) and target int64 [...]: the loss and its gradient come from one pass (df_cross_entropy_nhwc); the backward only
    scales the saved gradient.  A label outside [0, classes) raises ValueError."""

    @staticmethod
    def forward(ctx, logits, target, classes):
        logits, target = logits.contiguous(), target.contiguous()
        ld = logits.shape[-1]
        rows = logits.numel() // ld
        if target.dtype != torch.int64 or target.numel() != rows:
            raise RuntimeError(f"CrossEntropyNHWC: target must be int64 with {rows} elements, got {target.dtype} {tuple(target.shape)}")
        if not 1 <= classes <= ld:
            raise RuntimeError(f"CrossEntropyNHWC: {classes} classes in rows of {ld}")
        L = _lib.lib()
        dl = torch.empty_like(logits)
        loss = torch.empty((), device=logits.device)
        bad = torch.empty(1, dtype=torch.int32, device=logits.device)
        ws = torch.empty(int(L.df_cross_entropy_workspace_bytes(rows)), dtype=torch.uint8, device=logits.device)
        with _lib.device_guard(logits.device), _Timed("ce"):
            _ck(L.df_cross_entropy_nhwc(_lib.dptr(logits), _lib.dptr(target), dl.data_ptr(), rows, ld, int(classes), loss.data_ptr(),
                                        bad.data_ptr(), ws.data_ptr(), ws.numel(), _st()), "cross_entropy_nhwc")
        if int(bad.item()):
            raise ValueError(f"CrossEntropyNHWC: a target label lies outside [0, {classes})")
        ctx.save_for_backward(dl)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g, None, None
