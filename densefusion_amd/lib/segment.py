"""Detections from SegNet's own masks, on the device: the RGB-D frame -> SegNet -> per-object mask and box step of the
reference's real-robot setting (README: "the vanilla SegNet semantic-segmentation model used in our real-robot grasping
experiment"), in the form PoseCNN's detections take (tools/eval_ycb.py reads them from results_PoseCNN_RSS2018/%06d.mat).

``segment_frames`` enqueues, on the current stream and without a host sync:

  * ``df_segment_input``: uint8 RGB [F,H,W,3] -> the normalised fp32 NHWC4 input of SegNet's eval path
    (vanilla_segmentation/data_controller.py:79, bit for bit);
  * ``SegNet.forward_nhwc`` -> channels-last logits [F,H,W,ld];
  * ``df_segment_detect``: the int32 label map (torch.argmax over the classes), per (frame, class) the pixel count, the count with
    depth != 0 and the tight box, and per frame the classes 1..num_obj with more than ``min_pixels`` depth-valid pixels -- the
    reference's ``len(mask.nonzero()[0]) > minimum_num_pt`` rule (datasets/ycb/dataset.py:87,146) -- as a fixed-size table
    [F][C][6] of rows (cls, rmin, rmax_excl, cmin, cmax_excl, n_valid) plus a per-frame count: one small device->host copy.

One detection per class per frame, like PoseCNN's ROIs; ``det_row_to_roi`` turns a table row into a PoseCNN-style ROI whose
``preprocess.get_bbox`` sees the half-open tight box (LineMOD's ``get_bbox(mask_to_bbox(...))`` convention).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from .. import _lib

DET_FIELDS = ("cls", "rmin", "rmax_excl", "cmin", "cmax_excl", "n_valid")
STAT_FIELDS = ("count", "n_valid", "rmin", "rmax_excl", "cmin", "cmax_excl")


class Segmentation(NamedTuple):
    label: torch.Tensor     # [F,H,W] int32
    stats: torch.Tensor     # [F,C,6] int32 (STAT_FIELDS)
    det: torch.Tensor       # [F,C,6] int32 (DET_FIELDS); rows >= ndet[f] are zero
    ndet: torch.Tensor      # [F] int32


def segment_input(rgb, out=None):
    """rgb [F,H,W,3] uint8 (device) -> [F,H,W,4] fp32: (rgb - MEAN) / STD per channel on the 0..255 values, channel 3 zero."""
    if not rgb.is_cuda or rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[3] != 3:
        raise RuntimeError(f"segment_input: expected a device uint8 [F,H,W,3] tensor, got {tuple(rgb.shape)} {rgb.dtype} on {rgb.device}")
    F, H, W, _ = rgb.shape
    rgb = rgb.contiguous()
    if out is None:
        out = torch.empty(F, H, W, 4, dtype=torch.float32, device=rgb.device)
    with _lib.device_guard(rgb.device):
        _lib.check(_lib.lib().df_segment_input(_lib.dptr(rgb), _lib.dptr(out), F, H, W, _lib.current_stream()), "segment_input")
    return out


def detect(logits, C, depth, num_obj, min_pixels=50, label_out=None):
    """logits [F,H,W,ld] fp32 channels-last (first C channels the classes), depth [F,H,W] int16/uint16 (device) -> Segmentation."""
    if not logits.is_cuda or logits.dtype != torch.float32 or logits.dim() != 4:
        raise RuntimeError(f"detect: logits must be a device fp32 [F,H,W,ld] tensor, got {tuple(logits.shape)} {logits.dtype} on {logits.device}")
    if not depth.is_cuda or depth.device != logits.device:
        raise RuntimeError("detect: depth must be on the logits' device")
    logits = logits.contiguous()                # a channels-last view of another layout is copied, never read as [F,H,W,ld] rows
    F, H, W, ld = logits.shape
    if tuple(depth.shape) != (F, H, W) or depth.element_size() != 2 or depth.is_floating_point():
        raise RuntimeError(f"detect: depth must be 16-bit [F,H,W] = {(F, H, W)}, got {tuple(depth.shape)} {depth.dtype}")
    dev = logits.device
    L = _lib.lib()
    label = label_out if label_out is not None else torch.empty(F, H, W, dtype=torch.int32, device=dev)
    if label.dtype != torch.int32 or tuple(label.shape) != (F, H, W) or not label.is_contiguous():
        raise RuntimeError("detect: label_out must be a contiguous int32 [F,H,W] tensor")
    stats = torch.empty(F, C, 6, dtype=torch.int32, device=dev)
    det = torch.empty(F, C, 6, dtype=torch.int32, device=dev)
    ndet = torch.empty(F, dtype=torch.int32, device=dev)
    nbytes = L.df_segment_scratch_bytes(F, H, W, C)
    if nbytes == 0:
        raise RuntimeError(f"detect: unsupported sizes F={F} H={H} W={W} C={C}")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with _lib.device_guard(dev):
        _lib.check(L.df_segment_detect(_lib.dptr(logits), _lib.dptr(depth.contiguous()), F, H, W, ld, C, int(num_obj), int(min_pixels),
                                       _lib.dptr(label), _lib.dptr(stats), _lib.dptr(det), _lib.dptr(ndet), _lib.dptr(scratch),
                                       nbytes, _lib.current_stream()), "segment_detect")
    return Segmentation(label, stats, det, ndet)


def segment_frames(segnet, rgb, depth, num_obj, min_pixels=50, label_out=None):
    """rgb [F,H,W,3] uint8, depth [F,H,W] int16/uint16: device tensors; segnet: an eval-mode SegNet with label_nbr = num_obj + 1.
    Enqueues input kernel, SegNet and the label / statistics / detection launches on the current stream (no host sync) and
    returns a Segmentation; label_out (optional, int32 [F,H,W]) receives the label map."""
    if segnet.label_nbr - 1 != num_obj:
        raise RuntimeError(f"segment_frames: SegNet has {segnet.label_nbr} classes (background included), num_obj is {num_obj}")
    if not (rgb.is_cuda and depth.is_cuda):
        raise RuntimeError("densefusion_amd needs device tensors (no CPU path)")
    logits = segnet.forward_nhwc(segment_input(rgb))
    return detect(logits, segnet.label_nbr, depth, num_obj, min_pixels, label_out)


def det_row_to_roi(row):
    """Detection row (cls, rmin, rmax_excl, cmin, cmax_excl, n_valid) -> PoseCNN ROI [0, cls, x1, y1, x2, y2, score] =
    [0, cls, cmin - 1, rmin - 1, cmax_excl + 1, rmax_excl + 1, 1.0]: preprocess.get_bbox reads it back as the half-open tight box
    (rmin, rmax_excl, cmin, cmax_excl) before snapping."""
    cls, rmin, rmax, cmin, cmax = (int(v) for v in row[:5])
    return np.array([0, cls, cmin - 1, rmin - 1, cmax + 1, rmax + 1, 1.0], dtype=np.float64)
