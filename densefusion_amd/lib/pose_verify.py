"""Render-and-compare verification of estimated poses on the device (``df_pose_verify``, include/dfusion.h): the CAD mesh of each item is
drawn at its pose into a window of the item's depth frame by the renderers' own rasteriser and compared node by node with the observed
depth codes and, optionally, a mask.  The result is twelve integer tallies per item (``STATS``); ``vsiou`` turns them into a
visible-surface IoU and ``better`` compares two candidate poses per item.  tests/pose_verify_np.py restates the call; the tallies are
compared bit for bit.  ``PoseVerifier.score`` enqueues on the current stream and without a host sync.
``RenderedPoseDataset.pose_verifier()`` builds one for its models and tools/eval_cad_render.py ``--verify`` is its user.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _lib
from .mesh_set import MeshSet

MAX_OBJECTS = 64
STATUS = ("ok", "bad item")                                         # stats[:, 0]
STATS = ("status", "rendered", "agree", "front", "behind", "missing", "mask", "mask_observed", "unexplained", "sum_abs", "triangles",
         "cut_triangles")


class PoseVerifier:
    """``meshes``: a ``lib.mesh_set.MeshSet`` or the list of (vertices [V,3], triangles [T,3]) it packs, object o being mesh o with
    ``model_scales[o]`` (one for all is accepted): the renderers' factor from file units to camera units.  ``proj`` is the renderers'
    projection matrix, ``image_dims`` = (IH, IW) of the depth frames, ``cloud_div`` what takes a pose's translation (cloud units) to
    camera units: 10000 for the customCAD loader.  ``vertices`` (file units) and ``triangles`` are the set's device tensors."""

    def __init__(self, meshes, model_scales, proj, image_dims, cloud_div=10000.0, device="cuda"):
        ms = meshes if isinstance(meshes, MeshSet) else MeshSet(meshes)
        if ms.n_objects > MAX_OBJECTS:
            raise ValueError(f"pose_verify: 1..{MAX_OBJECTS} meshes, got {ms.n_objects}")
        scales = np.asarray(model_scales, dtype=np.float64).reshape(-1)
        if scales.size not in (1, ms.n_objects) or not np.isfinite(scales).all():
            raise ValueError("pose_verify: one finite model scale per mesh, or one for all")
        self.model_scales = np.ascontiguousarray(np.broadcast_to(scales, (ms.n_objects,)), dtype=np.float64)
        self.proj = np.ascontiguousarray(proj, dtype=np.float64).reshape(-1)
        if self.proj.size != 16:
            raise ValueError("pose_verify: proj is a 4 x 4 matrix")
        self.image_dims, self.cloud_div = (int(image_dims[0]), int(image_dims[1])), float(cloud_div)
        if self.image_dims[0] < 1 or self.image_dims[1] < 1 or not (np.isfinite(self.cloud_div) and self.cloud_div > 0):
            raise ValueError("pose_verify: image_dims must be positive and cloud_div finite and > 0")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("pose_verify: needs a GPU device (no CPU path)")
        self.vertices, self.triangles, _ = ms.on(self.device)
        self.device = self.vertices.device                          # with its index
        self.tri_begin, self.n_objects, self._scratch = ms.tri_begin, ms.n_objects, None

    def scratch_bytes(self, B, window):
        return int(_lib.lib().df_pose_verify_scratch_bytes(int(B), int(window[0]), int(window[1])))

    def score(self, depth, pose, frame, obj, corner, window, tol, mask=None, mask_frame=None, mask_value=65535, cull=False):
        """depth [F,IH,IW] uint16 (observed codes, 65535 = no observation), pose [B,7] fp64 (q wxyz, t in cloud units), frame and obj [B]
        int32 or int64 (the frame and the mesh of each item), corner [B,2] int32 or int64 (the window's first row and column in the
        frame; may be negative): device tensors on the meshes' device.  ``window`` = (WH, WW), one size for the call; ``tol`` in codes.
        ``mask`` [NM,IH,IW] uint16 with ``mask_frame`` [B] (default: ``frame``) and ``mask_value`` (an int for all, or [B]).
        Returns stats [B,12] int64 = ``STATS`` on the device; nothing is read back."""
        dev, ints = self.device, (torch.int32, torch.int64)
        IH, IW = self.image_dims
        depth = _lib.need_tensor(depth, "pose_verify", "depth", (torch.uint16,), (None, IH, IW), dev)
        pose = _lib.need_tensor(pose, "pose_verify", "pose", (torch.float64,), (None, 7), dev)
        B = int(pose.shape[0])
        frame = _lib.need_tensor(frame, "pose_verify", "frame", ints, (B,), dev)
        obj = _lib.need_tensor(obj, "pose_verify", "obj", ints, (B,), dev)
        corner = _lib.need_tensor(corner, "pose_verify", "corner", ints, (B, 2), dev)
        WH, WW, tol = int(window[0]), int(window[1]), int(tol)
        if not 1 <= B <= 65535 or int(depth.shape[0]) < 1 or int(depth.shape[0]) > 65535:
            raise ValueError(f"pose_verify: need 1..65535 items and frames (B {B}, F {int(depth.shape[0])})")
        if WH < 1 or WW < 1 or WH * WW > 2 ** 30:
            raise ValueError(f"pose_verify: window {WH} x {WW} outside 1..2^30 nodes")
        if not 0 <= tol <= 65535:
            raise ValueError(f"pose_verify: tol must be 0..65535 codes, got {tol}")
        NM = 0
        if mask is not None:
            mask = _lib.need_tensor(mask, "pose_verify", "mask", (torch.uint16,), (None, IH, IW), dev)
            NM = int(mask.shape[0])
            if NM < 1:
                raise ValueError("pose_verify: an empty mask")
            mask_frame = frame if mask_frame is None else _lib.need_tensor(mask_frame, "pose_verify", "mask_frame", ints, (B,), dev)
            if torch.is_tensor(mask_value):
                mask_value = _lib.need_tensor(mask_value, "pose_verify", "mask_value", ints, (B,), dev)
        elif mask_frame is not None:
            raise ValueError("pose_verify: mask_frame without a mask")
        items = torch.zeros(B, 6, dtype=torch.int32, device=dev)
        items[:, 0], items[:, 1], items[:, 2:4] = frame, obj, corner
        if mask is not None:
            items[:, 4], items[:, 5] = mask_frame, mask_value
        return self.score_items(depth, pose, items, (WH, WW), tol, mask=mask, cull=cull)

    def score_items(self, depth, pose, items, window, tol, mask=None, cull=False):
        """``score`` with the item records [B,6] int32 = {frame, object, r0, c0, mask_frame, mask_value} already on the device: the
        call itself and nothing else is enqueued."""
        dev = self.device
        IH, IW = self.image_dims
        depth = _lib.need_tensor(depth, "pose_verify", "depth", (torch.uint16,), (None, IH, IW), dev)
        pose = _lib.need_tensor(pose, "pose_verify", "pose", (torch.float64,), (None, 7), dev)
        B = int(pose.shape[0])
        items = _lib.need_tensor(items, "pose_verify", "items", (torch.int32,), (B, 6), dev)
        WH, WW, tol = int(window[0]), int(window[1]), int(tol)
        if not 1 <= B <= 65535 or not 1 <= int(depth.shape[0]) <= 65535 or WH < 1 or WW < 1 or WH * WW > 2 ** 30 or not 0 <= tol <= 65535:
            raise ValueError(f"pose_verify: B {B}, F {int(depth.shape[0])}, window {WH} x {WW} or tol {tol} out of range")
        NM = 0
        if mask is not None:
            mask = _lib.need_tensor(mask, "pose_verify", "mask", (torch.uint16,), (None, IH, IW), dev)
            NM = int(mask.shape[0])
            if NM < 1:
                raise ValueError("pose_verify: an empty mask")
        self._scratch = _lib.grow_scratch(self._scratch, self.scratch_bytes(B, (WH, WW)), dev)
        stats = torch.empty(B, len(STATS), dtype=torch.int64, device=dev)
        with _lib.device_guard(dev):
            _lib.check(_lib.lib().df_pose_verify(
                _lib.dptr(self.vertices), int(self.vertices.shape[0]), _lib.dptr(self.triangles), int(self.triangles.shape[0]),
                self.tri_begin.ctypes.data_as(ctypes.c_void_p), self.model_scales.ctypes.data_as(ctypes.c_void_p), self.n_objects,
                self.proj.ctypes.data_as(ctypes.c_void_p), _lib.dptr(depth), int(depth.shape[0]), IH, IW,
                _lib.dptr(mask) if mask is not None else None, NM, _lib.dptr(items), _lib.dptr(pose), self.cloud_div, B, WH, WW, tol,
                1 if cull else 0, _lib.dptr(stats), _lib.dptr(self._scratch), self._scratch.numel(), _lib.current_stream()), "pose_verify")
        return stats


def vsiou(stats):
    """The visible-surface IoU of stats [B,12]: agree / (agree + behind + unexplained) in fp64, 0 where the denominator is 0.  `front`
    (an occluder) and `missing` (no observation) count neither for nor against.  Tensor in, tensor out; array in, array out."""
    if torch.is_tensor(stats):
        agree = stats[..., 2].to(torch.float64)
        den = (stats[..., 2] + stats[..., 4] + stats[..., 8]).to(torch.float64)
        return torch.where(den > 0, agree / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
    stats = np.asarray(stats)
    agree = stats[..., 2].astype(np.float64)
    den = (stats[..., 2] + stats[..., 4] + stats[..., 8]).astype(np.float64)
    return np.where(den > 0, agree / np.where(den > 0, den, 1.0), 0.0)


def better(stats_a, stats_b):
    """bool [B]: b's ``vsiou`` is strictly higher than a's."""
    return vsiou(stats_b) > vsiou(stats_a)
