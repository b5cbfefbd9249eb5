"""``Loss`` -- the segmentation loss of the reference (vanilla_segmentation/loss.py:11-30): ``nn.CrossEntropyLoss()`` (mean over all
pixels) of ``semantic [B,classes,H,W]`` against ``target [B,H,W]`` int64.

Kept: the call ``criterion(semantic, target)`` and its value.  Different: any H x W (the reference hard-codes 480 x 640, loss.py:14;
it equals it there), and the loss and its gradient come from one HIP pass over channels-last logits (``CrossEntropyNHWC``).  For the
output of ``SegNet`` in ``train()`` mode -- a [B,classes,H,W] view of the tape's channels-last, channel-padded logits -- that tensor is
read directly; any other tensor is laid out channels-last first.  A label outside [0, classes) raises ValueError.
"""
from __future__ import annotations

import torch.nn as nn
import torch.nn.functional as F

from ..segtrain_ops import CrossEntropyNHWC


def loss_calculation(semantic, target):
    B, K, H, W = semantic.shape
    if tuple(target.shape) != (B, H, W):
        raise RuntimeError(f"Loss: target {tuple(target.shape)} does not match semantic {tuple(semantic.shape)}")
    nhwc = getattr(semantic, "_nhwc", None)
    if nhwc is None or tuple(nhwc.shape[:3]) != (B, H, W):
        ld = (K + 3) // 4 * 4
        nhwc = F.pad(semantic.float().permute(0, 2, 3, 1), (0, ld - K))
    return CrossEntropyNHWC.apply(nhwc, target.long(), K)


class Loss(nn.Module):
    def forward(self, semantic, target):
        return loss_calculation(semantic, target)
