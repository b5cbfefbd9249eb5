"""Dense, projective point-to-plane ICP of estimated poses against their depth windows on the device (``df_pose_refine_dense``,
include/dfusion.h): per pass the CAD mesh of each item is drawn at its current pose into the item's window by the verifier's own raster
pass, every drawn node is associated with the depth observed at the same node, and the pose moves so as to bring the observed points onto
the planes of the triangles drawn there.  Association is by pixel, so visibility is the z-buffer's; the whole window takes part and a
mask is optional.  The rule is written out as steps D1..D6 in fp64; tests/pose_dense_np.py restates it and the outputs are compared bit
for bit.  ``DensePoseRefiner.refine`` enqueues on the current stream and without a host sync.
``RenderedPoseDataset.dense_refiner()`` builds one for its models and tools/eval_cad_render.py ``--dense`` is its user.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _lib
from .mesh_set import MeshSet

MAX_OBJECTS = 64
MAX_ITERS = 64
STATUS = ("ok", "few inliers", "degenerate", "bad item")             # stats[:, 0]
STATS = ("status", "first_inliers", "first_rms", "last_inliers", "last_rms", "steps")


class DensePoseRefiner:
    """``meshes``, ``model_scales``, ``proj``, ``image_dims`` and ``cloud_div`` as for ``lib.pose_verify.PoseVerifier``: the meshes are
    drawn from the ``MeshSet``'s own device arrays in file units.  ``set_rays`` hands over the loader's ray map, which ``refine`` needs."""

    def __init__(self, meshes, model_scales, proj, image_dims, cloud_div=10000.0, device="cuda"):
        ms = meshes if isinstance(meshes, MeshSet) else MeshSet(meshes)
        if ms.n_objects > MAX_OBJECTS:
            raise ValueError(f"pose_refine_dense: 1..{MAX_OBJECTS} meshes, got {ms.n_objects}")
        scales = np.asarray(model_scales, dtype=np.float64).reshape(-1)
        if scales.size not in (1, ms.n_objects) or not np.isfinite(scales).all():
            raise ValueError("pose_refine_dense: one finite model scale per mesh, or one for all")
        self.model_scales = np.ascontiguousarray(np.broadcast_to(scales, (ms.n_objects,)), dtype=np.float64)
        self.proj = np.ascontiguousarray(proj, dtype=np.float64).reshape(-1)
        if self.proj.size != 16:
            raise ValueError("pose_refine_dense: proj is a 4 x 4 matrix")
        self.image_dims, self.cloud_div = (int(image_dims[0]), int(image_dims[1])), float(cloud_div)
        if self.image_dims[0] < 1 or self.image_dims[1] < 1 or not (np.isfinite(self.cloud_div) and self.cloud_div > 0):
            raise ValueError("pose_refine_dense: image_dims must be positive and cloud_div finite and > 0")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("pose_refine_dense: needs a GPU device (no CPU path)")
        self.vertices, self.triangles, _ = ms.on(self.device)
        self.device = self.vertices.device                          # with its index
        self.tri_begin, self.n_objects, self.rays, self._scratch = ms.tri_begin, ms.n_objects, None, None

    def set_rays(self, ray_map):
        """``ray_map`` [IH,IW,3] fp64 on the device: the loader's back-projection rays at unit depth (``UnityDepthProjector.ray_map_on``),
        which turn an observed code into a point.  ``RenderedPoseDataset.dense_refiner()`` sets it."""
        self.rays = _lib.need_tensor(ray_map, "pose_refine_dense", "ray_map", (torch.float64,), (self.image_dims[0], self.image_dims[1], 3),
                                     self.device)
        return self

    def scratch_bytes(self, B, window):
        return int(_lib.lib().df_pose_refine_dense_scratch_bytes(int(B), int(window[0]), int(window[1])))

    def refine(self, depth, pose, frame, obj, corner, window, iters=10, gate=16, mask=None, mask_frame=None, mask_value=65535, cull=False):
        """depth [F,IH,IW] uint16 (observed codes, 65535 = no observation), pose [B,7] fp64 (q wxyz, t in cloud units), frame and obj [B]
        and corner [B,2] int32 or int64 as for ``PoseVerifier.score``: device tensors on the meshes' device.  ``window`` = (WH, WW), one
        size for the call; ``iters`` in 0..64 steps (0: the call only scores the given poses); ``gate`` in 0..65535 codes, the largest
        difference between the rendered and the observed code of a node that takes part.  ``mask`` [NM,IH,IW] uint16 with ``mask_frame``
        [B] (default: ``frame``) and ``mask_value`` (an int for all, or [B]): only nodes where the mask holds the value take part.
        Returns (pose_out [B,7] fp64, a unit quaternion with w >= 0; stats [B,6] fp64 = ``STATS``, status by ``STATUS``) on the device;
        nothing is read back.  Raises ``ValueError`` without a ray map."""
        if self.rays is None:
            raise ValueError("pose_refine_dense: refine needs the loader's ray map and the frames "
                             "(RenderedPoseDataset(keep_frames=True).dense_refiner(), or set_rays)")
        dev, ints = self.device, (torch.int32, torch.int64)
        IH, IW = self.image_dims
        depth = _lib.need_tensor(depth, "pose_refine_dense", "depth", (torch.uint16,), (None, IH, IW), dev)
        pose = _lib.need_tensor(pose, "pose_refine_dense", "pose", (torch.float64,), (None, 7), dev)
        B = int(pose.shape[0])
        frame = _lib.need_tensor(frame, "pose_refine_dense", "frame", ints, (B,), dev)
        obj = _lib.need_tensor(obj, "pose_refine_dense", "obj", ints, (B,), dev)
        corner = _lib.need_tensor(corner, "pose_refine_dense", "corner", ints, (B, 2), dev)
        WH, WW, iters, gate = int(window[0]), int(window[1]), int(iters), int(gate)
        if not 1 <= B <= 65535 or not 1 <= int(depth.shape[0]) <= 65535:
            raise ValueError(f"pose_refine_dense: need 1..65535 items and frames (B {B}, F {int(depth.shape[0])})")
        if WH < 1 or WW < 1 or WH * WW > 2 ** 30:
            raise ValueError(f"pose_refine_dense: window {WH} x {WW} outside 1..2^30 nodes")
        if not 0 <= iters <= MAX_ITERS or not 0 <= gate <= 65535:
            raise ValueError(f"pose_refine_dense: iters must be 0..{MAX_ITERS} and gate 0..65535 codes, got {iters} and {gate}")
        NM = 0
        if mask is not None:
            mask = _lib.need_tensor(mask, "pose_refine_dense", "mask", (torch.uint16,), (None, IH, IW), dev)
            NM = int(mask.shape[0])
            if NM < 1:
                raise ValueError("pose_refine_dense: an empty mask")
            mask_frame = frame if mask_frame is None else _lib.need_tensor(mask_frame, "pose_refine_dense", "mask_frame", ints, (B,), dev)
            if torch.is_tensor(mask_value):
                mask_value = _lib.need_tensor(mask_value, "pose_refine_dense", "mask_value", ints, (B,), dev)
        elif mask_frame is not None:
            raise ValueError("pose_refine_dense: mask_frame without a mask")
        items = torch.zeros(B, 6, dtype=torch.int32, device=dev)
        items[:, 0], items[:, 1], items[:, 2:4] = frame, obj, corner
        if mask is not None:
            items[:, 4], items[:, 5] = mask_frame, mask_value
        self._scratch = _lib.grow_scratch(self._scratch, self.scratch_bytes(B, (WH, WW)), dev)
        pose_out = torch.empty(B, 7, dtype=torch.float64, device=dev)
        stats = torch.empty(B, len(STATS), dtype=torch.float64, device=dev)
        with _lib.device_guard(dev):
            _lib.check(_lib.lib().df_pose_refine_dense(
                _lib.dptr(self.vertices), int(self.vertices.shape[0]), _lib.dptr(self.triangles), int(self.triangles.shape[0]),
                self.tri_begin.ctypes.data_as(ctypes.c_void_p), self.model_scales.ctypes.data_as(ctypes.c_void_p), self.n_objects,
                self.proj.ctypes.data_as(ctypes.c_void_p), _lib.dptr(depth), int(depth.shape[0]), IH, IW, _lib.dptr(self.rays),
                _lib.dptr(mask) if mask is not None else None, NM, _lib.dptr(items), _lib.dptr(pose), self.cloud_div, B, WH, WW, gate,
                1 if cull else 0, iters, _lib.dptr(pose_out), _lib.dptr(stats), _lib.dptr(self._scratch), self._scratch.numel(),
                _lib.current_stream()), "pose_refine_dense")
        return pose_out, stats
