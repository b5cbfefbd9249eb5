"""Dense, projective ICP with an outline term (``df_pose_refine_contour``, include/dfusion.h): ``lib.pose_refine_dense``'s refiner, whose
planes leave a direction free on a view of one flat wall or of two faces of a box (its status ``degenerate``), with the object's outline to
hold it.  Once per call the outline of the observed object is found in the depth window (and the mask, when there is one) and every node
learns its nearest outline node within ``reach``; per pass the outline of the drawn model is pulled, across the image only, towards it, and
the pairs' sums join the planes' before the solve.  The rule is steps E1..E6 on top of D1..D6; tests/pose_contour_np.py restates it and the
outputs are compared bit for bit.  With ``contour_scale`` 0 the poses and the six dense columns are ``DensePoseRefiner.refine``'s byte for
byte.  ``RenderedPoseDataset.contour_refiner()`` builds one for its models and tools/eval_cad_render.py ``--contour`` is its user.
"""
from __future__ import annotations

import ctypes
import math

import torch

from .. import _lib
from .pose_refine_dense import MAX_ITERS, STATUS, DensePoseRefiner  # noqa: F401  (STATUS: the same four)

MAX_REACH = 64
STATS = ("status", "first_inliers", "first_rms", "last_inliers", "last_rms", "steps", "first_pairs", "last_pairs")


class ContourPoseRefiner(DensePoseRefiner):
    """Built as ``DensePoseRefiner`` (its errors carry that name); ``set_rays`` is its own."""

    def scratch_bytes(self, B, window):
        return int(_lib.lib().df_pose_refine_contour_scratch_bytes(int(B), int(window[0]), int(window[1])))

    def refine(self, depth, pose, frame, obj, corner, window, iters=10, gate=16, edge_step=65535, reach=6, contour_scale=0.1, mask=None,
               mask_frame=None, mask_value=65535, cull=False):
        """``DensePoseRefiner.refine``'s arguments, and: ``edge_step`` in 0..65535 codes, the depth step between neighbouring nodes above
        which the nearer one counts as an outline node (65535: only the border of what was observed, or drawn, is an outline; a smaller
        value must suit the frame: on a small frame a tilted wall's neighbouring nodes lie hundreds of codes apart); ``reach`` in 0..64
        nodes, the farthest observed-outline node a drawn-outline node pairs with; ``contour_scale``, finite and >= 0, the weight of an
        outline residual against a plane residual.  With a mask the observed outline is that of the masked, observed nodes: give the
        mask of the whole object, since the drawn outline is the whole model's.  Returns (pose_out [B,7] fp64, stats [B,8] fp64 =
        ``STATS``) on the device; nothing is read back."""
        if self.rays is None:
            raise ValueError("pose_refine_contour: refine needs the loader's ray map and the frames "
                             "(RenderedPoseDataset(keep_frames=True).contour_refiner(), or set_rays)")
        dev, ints = self.device, (torch.int32, torch.int64)
        IH, IW = self.image_dims
        depth = _lib.need_tensor(depth, "pose_refine_contour", "depth", (torch.uint16,), (None, IH, IW), dev)
        pose = _lib.need_tensor(pose, "pose_refine_contour", "pose", (torch.float64,), (None, 7), dev)
        B = int(pose.shape[0])
        frame = _lib.need_tensor(frame, "pose_refine_contour", "frame", ints, (B,), dev)
        obj = _lib.need_tensor(obj, "pose_refine_contour", "obj", ints, (B,), dev)
        corner = _lib.need_tensor(corner, "pose_refine_contour", "corner", ints, (B, 2), dev)
        WH, WW, iters, gate, edge_step, reach = int(window[0]), int(window[1]), int(iters), int(gate), int(edge_step), int(reach)
        contour_scale = float(contour_scale)
        if not 1 <= B <= 65535 or not 1 <= int(depth.shape[0]) <= 65535:
            raise ValueError(f"pose_refine_contour: need 1..65535 items and frames (B {B}, F {int(depth.shape[0])})")
        if WH < 1 or WW < 1 or WH * WW > 2 ** 30:
            raise ValueError(f"pose_refine_contour: window {WH} x {WW} outside 1..2^30 nodes")
        if not 0 <= iters <= MAX_ITERS or not 0 <= gate <= 65535:
            raise ValueError(f"pose_refine_contour: iters must be 0..{MAX_ITERS} and gate 0..65535 codes, got {iters} and {gate}")
        if not 0 <= edge_step <= 65535 or not 0 <= reach <= MAX_REACH:
            raise ValueError(f"pose_refine_contour: edge_step must be 0..65535 codes and reach 0..{MAX_REACH} nodes, got {edge_step} and {reach}")
        if not (math.isfinite(contour_scale) and contour_scale >= 0.0):
            raise ValueError(f"pose_refine_contour: contour_scale must be finite and >= 0, got {contour_scale}")
        NM = 0
        if mask is not None:
            mask = _lib.need_tensor(mask, "pose_refine_contour", "mask", (torch.uint16,), (None, IH, IW), dev)
            NM = int(mask.shape[0])
            if NM < 1:
                raise ValueError("pose_refine_contour: an empty mask")
            mask_frame = frame if mask_frame is None else _lib.need_tensor(mask_frame, "pose_refine_contour", "mask_frame", ints, (B,), dev)
            if torch.is_tensor(mask_value):
                mask_value = _lib.need_tensor(mask_value, "pose_refine_contour", "mask_value", ints, (B,), dev)
        elif mask_frame is not None:
            raise ValueError("pose_refine_contour: mask_frame without a mask")
        items = torch.zeros(B, 6, dtype=torch.int32, device=dev)
        items[:, 0], items[:, 1], items[:, 2:4] = frame, obj, corner
        if mask is not None:
            items[:, 4], items[:, 5] = mask_frame, mask_value
        self._scratch = _lib.grow_scratch(self._scratch, self.scratch_bytes(B, (WH, WW)), dev)
        pose_out = torch.empty(B, 7, dtype=torch.float64, device=dev)
        stats = torch.empty(B, len(STATS), dtype=torch.float64, device=dev)
        with _lib.device_guard(dev):
            _lib.check(_lib.lib().df_pose_refine_contour(
                _lib.dptr(self.vertices), int(self.vertices.shape[0]), _lib.dptr(self.triangles), int(self.triangles.shape[0]),
                self.tri_begin.ctypes.data_as(ctypes.c_void_p), self.model_scales.ctypes.data_as(ctypes.c_void_p), self.n_objects,
                self.proj.ctypes.data_as(ctypes.c_void_p), _lib.dptr(depth), int(depth.shape[0]), IH, IW, _lib.dptr(self.rays),
                _lib.dptr(mask) if mask is not None else None, NM, _lib.dptr(items), _lib.dptr(pose), self.cloud_div, B, WH, WW, gate,
                1 if cull else 0, iters, edge_step, reach, contour_scale, _lib.dptr(pose_out), _lib.dptr(stats), _lib.dptr(self._scratch),
                self._scratch.numel(), _lib.current_stream()), "pose_refine_contour")
        return pose_out, stats
