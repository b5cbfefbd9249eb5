"""The symmetry-aware BOP pose errors on the device (``df_pose_sym_error``, include/dfusion.h): MSSD, the maximum symmetry-aware surface
distance over all vertices of an item's CAD mesh, and MSPD, the same in the image plane, each the minimum over the object's whole
symmetry set (``datasets.customCAD.symmetry.symmetry_set``).  The rule is written out as steps E0..E7 in fp64; tests/pose_error_np.py
restates it and the six columns are compared bit for bit.  ``PoseErrors.sym_error`` enqueues on the current stream and without a host
sync.  ``PoseErrors.vsd`` is the third BOP error, the visible surface discrepancy (``df_pose_vsd``: both poses drawn by the verifier's
own raster pass and compared with the observed depth as distances along the loader's rays; integer tallies, ``vsd_values`` divides).
``RenderedPoseDataset.pose_errors()`` builds one for its models.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _lib
from .mesh_set import MeshSet

INT_MAX = 2 ** 31 - 1
MAX_OBJECTS = 64
STATUS = ("ok", "bad item")                                         # out[:, 0]
STATS = ("status", "mssd", "mssd_sym", "mspd", "mspd_sym", "vertices")
VSD_STATS = ("status", "union", "inter", "rendered_e")               # then bad_0 .. bad_{NT-1}, one per tau
MAX_TAU = 16


class PoseErrors:
    """``meshes``: a ``lib.mesh_set.MeshSet`` or the list of (vertices [V,3], triangles [T,3]) it packs, object o being mesh o with
    ``model_scales[o]`` (one for all is accepted): the renderers' factor from file units to camera units; ``cloud_div`` takes camera
    units to the units of the poses' translations (10000 for the customCAD loader), so the vertices read here are the ones ``MeshIcp``
    reads, ``MeshSet.scaled(model_scales / cloud_div)``.  ``sym_sets``: one float64 [S,3,4] per object, the identity first, in the units
    of the poses (``RenderedPoseDataset.symmetry_sets()``); the one new upload.  ``proj`` is the renderers' projection matrix and
    ``image_dims`` = (IH, IW) the frame the pixel distances are taken in."""

    def __init__(self, meshes, model_scales, sym_sets, proj, image_dims, cloud_div=10000.0, device="cuda"):
        ms = meshes if isinstance(meshes, MeshSet) else MeshSet(meshes)
        if ms.n_objects > MAX_OBJECTS:
            raise ValueError(f"pose_error: 1..{MAX_OBJECTS} meshes, got {ms.n_objects}")
        scales = np.asarray(model_scales, dtype=np.float64).reshape(-1)
        self.cloud_div = float(cloud_div)
        if scales.size not in (1, ms.n_objects) or not np.isfinite(scales).all() or not (np.isfinite(self.cloud_div) and self.cloud_div > 0):
            raise ValueError("pose_error: one finite model scale per mesh, or one for all, and cloud_div finite and > 0")
        self.model_scales = np.ascontiguousarray(np.broadcast_to(scales, (ms.n_objects,)), dtype=np.float64)
        scaled = ms.scaled(self.model_scales / self.cloud_div)
        sets = [np.ascontiguousarray(s, dtype=np.float64) for s in sym_sets]
        if len(sets) != ms.n_objects or any(s.ndim != 3 or s.shape[1:] != (3, 4) or len(s) < 1 for s in sets):
            raise ValueError(f"pose_error: one symmetry set [S,3,4] with S >= 1 per mesh ({ms.n_objects})")
        self.sym_begin = np.cumsum([0] + [len(s) for s in sets]).astype(np.int32)
        if 12 * int(self.sym_begin[-1]) > INT_MAX:
            raise ValueError("pose_error: too many symmetries")
        self.sym_max = max(len(s) for s in sets)
        self.proj = np.ascontiguousarray(proj, dtype=np.float64).reshape(-1)
        if self.proj.size != 16:
            raise ValueError("pose_error: proj is a 4 x 4 matrix")
        self.image_dims = (int(image_dims[0]), int(image_dims[1]))
        if self.image_dims[0] < 1 or self.image_dims[1] < 1:
            raise ValueError("pose_error: image_dims must be positive")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("pose_error: needs a GPU device (no CPU path)")
        self.vertices = torch.from_numpy(scaled).to(self.device)
        self.sym = torch.from_numpy(np.concatenate(sets).reshape(-1, 12)).to(self.device)
        self.device = self.vertices.device                          # with its index
        self.vertex_begin, self.n_objects, self._scratch = ms.vertex_begin, ms.n_objects, None
        # VSD draws the meshes as the renderer does: the set's own device arrays in file units, nothing uploaded again
        self.file_vertices, self.triangles, _ = ms.on(self.device)
        self.tri_begin, self.rays, self._vsd_scratch = ms.tri_begin, None, None

    def set_rays(self, ray_map):
        """``ray_map`` [IH,IW,3] fp64 on the device: the loader's back-projection rays at unit depth (``UnityDepthProjector.ray_map_on``),
        which ``vsd`` measures distances along.  ``RenderedPoseDataset.pose_errors()`` sets it when the dataset keeps its frames."""
        self.rays = _lib.need_tensor(ray_map, "pose_error", "ray_map", (torch.float64,), (self.image_dims[0], self.image_dims[1], 3), self.device)
        return self

    def vsd(self, depth, pose_est, pose_gt, frame, obj, corner, window, delta, tau, cull=False):
        """The tallies of the visible surface discrepancy (``df_pose_vsd``): depth [F,IH,IW] uint16 (observed codes, 65535 = no
        observation), pose_est and pose_gt [B,7] fp64, frame and obj [B] and corner [B,2] int32 or int64 as for
        ``PoseVerifier.score``: device tensors.  ``window`` = (WH, WW); ``delta`` [O] and ``tau`` [O,NT] (or [NT] for all objects), NT
        in 1..16 ascending, in camera units (cloud units x ``cloud_div``).  Returns stats [B, 4 + NT] int64 = ``VSD_STATS`` then bad_k,
        on the device; ``vsd_values`` turns them into the errors.  Raises ``ValueError`` without a ray map (a dataset that does not keep
        its frames has none to score against)."""
        if self.rays is None:
            raise ValueError("pose_error: vsd needs the loader's ray map and the frames (RenderedPoseDataset(keep_frames=True).pose_errors(), or set_rays)")
        dev, ints = self.device, (torch.int32, torch.int64)
        IH, IW = self.image_dims
        depth = _lib.need_tensor(depth, "pose_error", "depth", (torch.uint16,), (None, IH, IW), dev)
        pose_est = _lib.need_tensor(pose_est, "pose_error", "pose_est", (torch.float64,), (None, 7), dev)
        B = int(pose_est.shape[0])
        pose_gt = _lib.need_tensor(pose_gt, "pose_error", "pose_gt", (torch.float64,), (B, 7), dev)
        frame = _lib.need_tensor(frame, "pose_error", "frame", ints, (B,), dev)
        obj = _lib.need_tensor(obj, "pose_error", "obj", ints, (B,), dev)
        corner = _lib.need_tensor(corner, "pose_error", "corner", ints, (B, 2), dev)
        WH, WW = int(window[0]), int(window[1])
        delta = np.ascontiguousarray(np.broadcast_to(np.asarray(delta, dtype=np.float64).reshape(-1), (self.n_objects,)))
        tau = np.asarray(tau, dtype=np.float64)
        tau = np.ascontiguousarray(np.broadcast_to(tau if tau.ndim == 2 else tau.reshape(1, -1), (self.n_objects, tau.shape[-1])))
        NT = int(tau.shape[1])
        if not 1 <= B <= 65535 or not 1 <= int(depth.shape[0]) <= 65535 or WH < 1 or WW < 1 or WH * WW > 2 ** 30:
            raise ValueError(f"pose_error: B {B}, F {int(depth.shape[0])} or window {WH} x {WW} out of range")
        if not 1 <= NT <= MAX_TAU or not (np.isfinite(delta).all() and (delta >= 0).all()) or not (tau >= 0).all() or (np.diff(tau, axis=1) < 0).any():
            raise ValueError(f"pose_error: delta finite and >= 0, tau 1..{MAX_TAU} values >= 0 in ascending order")
        items = torch.zeros(B, 6, dtype=torch.int32, device=dev)
        items[:, 0], items[:, 1], items[:, 2:4] = frame, obj, corner
        need = int(_lib.lib().df_pose_vsd_scratch_bytes(B, WH, WW))
        self._vsd_scratch = _lib.grow_scratch(self._vsd_scratch, need, dev)
        stats = torch.empty(B, len(VSD_STATS) + NT, dtype=torch.int64, device=dev)
        with _lib.device_guard(dev):
            _lib.check(_lib.lib().df_pose_vsd(
                _lib.dptr(self.file_vertices), int(self.file_vertices.shape[0]), _lib.dptr(self.triangles), int(self.triangles.shape[0]),
                self.tri_begin.ctypes.data_as(ctypes.c_void_p), self.model_scales.ctypes.data_as(ctypes.c_void_p), self.n_objects,
                self.proj.ctypes.data_as(ctypes.c_void_p), _lib.dptr(depth), int(depth.shape[0]), IH, IW, _lib.dptr(self.rays), _lib.dptr(items),
                _lib.dptr(pose_est), _lib.dptr(pose_gt), self.cloud_div, delta.ctypes.data_as(ctypes.c_void_p), tau.ctypes.data_as(ctypes.c_void_p),
                NT, B, WH, WW, 1 if cull else 0, _lib.dptr(stats), _lib.dptr(self._vsd_scratch), self._vsd_scratch.numel(),
                _lib.current_stream()), "pose_vsd")
        return stats

    def scratch_bytes(self, B):
        return int(_lib.lib().df_pose_sym_error_scratch_bytes(int(B), self.sym_max))

    def sym_error(self, pose_est, pose_gt, obj):
        """pose_est, pose_gt [B,7] fp64 (q wxyz, t in the units of the clouds), obj [B] int32 or int64 (the mesh of each item): device
        tensors on the meshes' device.  Returns out [B,6] fp64 = ``STATS`` on the device: status (``STATUS``), MSSD in the units of the
        poses with the symmetry that gave it, MSPD in pixels with its symmetry, the vertices used.  Nothing is read back."""
        pose_est = _lib.need_tensor(pose_est, "pose_error", "pose_est", (torch.float64,), (None, 7), self.device)
        B = int(pose_est.shape[0])
        pose_gt = _lib.need_tensor(pose_gt, "pose_error", "pose_gt", (torch.float64,), (B, 7), self.device)
        obj = _lib.need_tensor(obj, "pose_error", "obj", (torch.int32, torch.int64), (B,), self.device).to(torch.int32)
        if not 1 <= B <= 65535:
            raise ValueError(f"pose_error: need 1..65535 items, got {B}")
        self._scratch = _lib.grow_scratch(self._scratch, self.scratch_bytes(B), self.device)
        out = torch.empty(B, len(STATS), dtype=torch.float64, device=self.device)
        with _lib.device_guard(self.device):
            _lib.check(_lib.lib().df_pose_sym_error(
                _lib.dptr(self.vertices), int(self.vertices.shape[0]), self.vertex_begin.ctypes.data_as(ctypes.c_void_p), _lib.dptr(self.sym),
                int(self.sym.shape[0]), self.sym_begin.ctypes.data_as(ctypes.c_void_p), self.n_objects, _lib.dptr(obj), _lib.dptr(pose_est),
                _lib.dptr(pose_gt), B, self.proj.ctypes.data_as(ctypes.c_void_p), self.image_dims[0], self.image_dims[1], _lib.dptr(out),
                _lib.dptr(self._scratch), self._scratch.numel(), _lib.current_stream()), "pose_sym_error")
        return out


def vsd_values(stats):
    """The visible surface discrepancies of stats [B, 4 + NT]: (bad_k + union - inter) / union in fp64, 1 where union = 0; [B, NT].
    Tensor in, tensor out; array in, array out."""
    if torch.is_tensor(stats):
        union, inter = stats[:, 1:2].to(torch.float64), stats[:, 2:3].to(torch.float64)
        return torch.where(union > 0, (stats[:, 4:].to(torch.float64) + union - inter) / torch.where(union > 0, union, torch.ones_like(union)),
                           torch.ones_like(stats[:, 4:], dtype=torch.float64))
    stats = np.asarray(stats)
    union, inter = stats[:, 1:2].astype(np.float64), stats[:, 2:3].astype(np.float64)
    return np.where(union > 0, (stats[:, 4:].astype(np.float64) + union - inter) / np.where(union > 0, union, 1.0), 1.0)
