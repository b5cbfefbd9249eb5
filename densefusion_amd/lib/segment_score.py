"""Scoring SegNet against rendered truth, on the device, and SegNet's label map as the masks of the customCAD pose path.

``seg_score`` enqueues ``df_seg_score`` on the current stream and without a host sync: the int32 label map (``torch.argmax`` over the
classes, the rule of ``segment.detect``), per frame the confusion matrix ``conf[truth][predicted]`` against the int64 target
``preprocess.seg_batch`` wrote, and the number of pixels whose target names no class.  ``seg_masks`` (``df_seg_masks``) turns label maps
in window coordinates into the uint16 masks ``preprocess.cad_item_table`` and ``preprocess_objects_cad`` read with label value 65535.
``SegScore`` sums confusion matrices over calls on the device; ``metrics_from_confusion`` is the host arithmetic on the one read-back.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib

MAX_CLASSES = 64


def check_classes(C, ld):
    """``ValueError`` unless 2 <= C <= 64, C <= ld <= 64 and ld is a multiple of 4 (the limits of ``df_seg_score``)."""
    C, ld = int(C), int(ld)
    if not 2 <= C <= MAX_CLASSES or not C <= ld <= 64 or ld % 4:
        raise ValueError(f"seg_score: need 2 <= C <= 64, C <= ld <= 64 and ld a multiple of 4 (C {C}, ld {ld})")
    return C, ld


def check_masks_args(F, window, win, pairs, image_dims):
    """The argument rule of ``df_seg_masks`` on host integers: (win [F,2] int32, pairs [N,2] int32) as contiguous arrays, or
    ``ValueError`` for a window that leaves the frame, a pair's frame outside 0..F-1 or its class outside 0..64."""
    (H, W), (IH, IW) = (int(window[0]), int(window[1])), (int(image_dims[0]), int(image_dims[1]))
    if not (1 <= H <= IH and 1 <= W <= IW):
        raise ValueError(f"seg_masks: window {H} x {W} outside the {IH} x {IW} frame")
    win = np.asarray(win, dtype=np.int64).reshape(-1, 2)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if win.shape[0] != F:
        raise ValueError(f"seg_masks: win must hold one corner per label map ({F}), got {win.shape[0]}")
    if pairs.shape[0] == 0:
        raise ValueError("seg_masks: no pairs")
    for f, (y0, x0) in enumerate(win.tolist()):
        if not 0 <= y0 <= IH - H or not 0 <= x0 <= IW - W:
            raise ValueError(f"seg_masks: frame {f}: window corner ({y0}, {x0}) leaves the {IH} x {IW} frame for a {H} x {W} window")
    for n, (f, c) in enumerate(pairs.tolist()):
        if not 0 <= f < F or not 0 <= c <= MAX_CLASSES:
            raise ValueError(f"seg_masks: pair {n}: frame {f} outside 0..{F - 1} or class {c} outside 0..{MAX_CLASSES}")
    return np.ascontiguousarray(win, dtype=np.int32), np.ascontiguousarray(pairs, dtype=np.int32)


def seg_score(logits, target, C, label_out=None):
    """logits [F,H,W,ld] fp32 channels-last (first C channels the classes), target [F,H,W] int64: device tensors.  Returns
    (conf [F,C,C] int32, skipped [F] int32, label [F,H,W] int32) on the device; ``label_out`` (optional, contiguous int32 [F,H,W])
    receives the label map.  A pixel whose target lies outside 0..C-1 is counted in ``skipped`` and in no cell."""
    if not torch.is_tensor(logits) or not logits.is_cuda or logits.dtype != torch.float32 or logits.dim() != 4:
        raise RuntimeError("seg_score: logits must be a device fp32 [F,H,W,ld] tensor (no CPU path)")
    logits = logits.contiguous()                # a channels-last view of another layout is copied, never read as [F,H,W,ld] rows
    F, H, W, ld = logits.shape
    C, ld = check_classes(C, ld)
    if not torch.is_tensor(target) or target.device != logits.device or target.dtype != torch.int64 or tuple(target.shape) != (F, H, W):
        raise RuntimeError(f"seg_score: target must be an int64 [F,H,W] = {(F, H, W)} tensor on the logits' device")
    if F < 1 or F > 65535 or H * W < 1 or H * W > 2 ** 30:
        raise ValueError(f"seg_score: need 1 <= F <= 65535 and 1 <= H*W <= 2^30 (F {F}, H {H}, W {W})")
    dev = logits.device
    label = label_out if label_out is not None else torch.empty(F, H, W, dtype=torch.int32, device=dev)
    if label.dtype != torch.int32 or tuple(label.shape) != (F, H, W) or not label.is_contiguous() or label.device != dev:
        raise RuntimeError("seg_score: label_out must be a contiguous int32 [F,H,W] tensor on the logits' device")
    conf = torch.empty(F, C, C, dtype=torch.int32, device=dev)
    skipped = torch.empty(F, dtype=torch.int32, device=dev)
    with _lib.device_guard(dev):
        _lib.check(_lib.lib().df_seg_score(_lib.dptr(logits), _lib.dptr(target.contiguous()), F, H, W, ld, C, _lib.dptr(label),
                                           _lib.dptr(conf), _lib.dptr(skipped), _lib.current_stream()), "seg_score")
    return conf, skipped, label


def seg_masks(label, win, pairs, image_dims):
    """label [F,H,W] int32 device tensor (label maps in window coordinates), win [F,2] HOST integers {y0, x0} (each window's corner in
    its IH x IW frame), pairs [N,2] HOST integers {frame, class}, image_dims = (IH, IW).  Returns mask [N,IH,IW] uint16 on the device:
    65535 inside the window where the label equals the class, 0 everywhere else.  Arguments are checked on host integers
    (``ValueError``); no read-back, no synchronisation."""
    if not torch.is_tensor(label) or not label.is_cuda or label.dtype != torch.int32 or label.dim() != 3:
        raise RuntimeError("seg_masks: label must be a device int32 [F,H,W] tensor (no CPU path)")
    if torch.is_tensor(win) or torch.is_tensor(pairs):
        raise RuntimeError("seg_masks: win and pairs are host integers (they travel as launch arguments)")
    F, H, W = label.shape
    IH, IW = int(image_dims[0]), int(image_dims[1])
    win, pairs = check_masks_args(F, (H, W), win, pairs, (IH, IW))
    N, dev = pairs.shape[0], label.device
    mask = torch.empty(N, IH, IW, dtype=torch.int16, device=dev).view(torch.uint16)
    with _lib.device_guard(dev):
        _lib.check(_lib.lib().df_seg_masks(_lib.dptr(label.contiguous()), F, H, W, win.ctypes.data, pairs.ctypes.data, N, IH, IW,
                                           mask.data_ptr(), _lib.current_stream()), "seg_masks")
    return mask


def metrics_from_confusion(conf):
    """conf [C,C] integers, ``conf[truth][predicted]`` -> dict of float64: ``iou``, ``precision``, ``recall`` [C] (``nan`` where the
    denominator is zero: IoU of a class with neither a truth nor a predicted pixel, precision of a class never predicted, recall of a
    class never present), ``pixel_accuracy`` (``nan`` for an empty matrix), ``miou`` = the mean IoU over the classes that have a truth
    or a predicted pixel (``nan`` if there is none), and ``pixels``.  Pure numpy, exact integer sums."""
    conf = np.asarray(conf)
    if conf.ndim != 2 or conf.shape[0] != conf.shape[1] or not np.issubdtype(conf.dtype, np.integer):
        raise ValueError("metrics_from_confusion: conf must be a square integer matrix")
    conf = conf.astype(np.int64)
    tp, truth, pred, total = np.diag(conf), conf.sum(axis=1), conf.sum(axis=0), int(conf.sum())
    union = truth + pred - tp

    def ratio(num, den):
        out = np.full(den.shape, np.nan, dtype=np.float64)
        np.divide(num.astype(np.float64), den.astype(np.float64), out=out, where=den > 0)
        return out

    iou = ratio(tp, union)
    return dict(iou=iou, precision=ratio(tp, pred), recall=ratio(tp, truth),
                pixel_accuracy=float(tp.sum()) / total if total else float("nan"),
                miou=float(np.mean(iou[union > 0])) if (union > 0).any() else float("nan"), pixels=total)


class SegScore:
    """The confusion matrix of C classes summed over calls, in an int64 tensor on the device: ``add`` enqueues one sum per call and
    reads nothing back; ``summary`` is the one read-back."""

    def __init__(self, C, device="cuda"):
        self.C = check_classes(C, (int(C) + 3) // 4 * 4)[0]
        self.device = torch.device(device)
        self.conf = torch.zeros(self.C, self.C, dtype=torch.int64, device=self.device)
        self.skipped = torch.zeros((), dtype=torch.int64, device=self.device)

    def add(self, conf, skipped=None):
        """conf [F,C,C] or [C,C] int32 / int64 device tensor (``seg_score``'s), skipped [F] likewise."""
        if tuple(conf.shape[-2:]) != (self.C, self.C) or conf.dim() not in (2, 3) or conf.is_floating_point():
            raise RuntimeError(f"SegScore.add: conf must be an integer [F,{self.C},{self.C}] tensor")
        self.conf += conf.reshape(-1, self.C, self.C).sum(dim=0, dtype=torch.int64)
        if skipped is not None:
            self.skipped += skipped.sum(dtype=torch.int64)
        return self

    def update(self, logits, target, label_out=None):
        """``seg_score`` of one batch, added; returns its (conf, skipped, label)."""
        conf, skipped, label = seg_score(logits, target, self.C, label_out)
        self.add(conf, skipped)
        return conf, skipped, label

    def reset(self):
        self.conf.zero_()
        self.skipped.zero_()
        return self

    def summary(self):
        """``metrics_from_confusion`` of the sum, with ``conf`` (int64 numpy) and ``skipped``: one device -> host copy.  The sums may
        have been enqueued on another stream (a prefetcher's), so the device is synchronised first."""
        torch.cuda.synchronize(self.device)
        flat = torch.cat([self.conf.reshape(-1), self.skipped.reshape(1)]).cpu().numpy()
        conf = flat[:-1].reshape(self.C, self.C)
        out = metrics_from_confusion(conf)
        out.update(conf=conf, skipped=int(flat[-1]))
        return out
