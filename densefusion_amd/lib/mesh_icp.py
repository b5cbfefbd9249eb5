"""Point-to-plane ICP against the exact surface of CAD meshes on the device (``df_mesh_icp``, include/dfusion.h): B estimated poses, each
with its own observed points and object, are fitted to the triangles by the written-out rule S0, I1..I10 in fp64 (tests/mesh_icp_np.py
restates it; the outputs are compared bit for bit).  ``MeshIcp.refine`` enqueues on the current stream and without a host sync; the pose
moves on the device between the iterations.  ``RenderedPoseDataset.mesh_icp()`` builds one for its models and
tools/eval_cad_render.py ``--icp`` is its user.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _lib
from .mesh_set import MeshSet

INT_MAX = 2 ** 31 - 1
MAX_OBJECTS, MAX_ITERS = 64, 64
STATUS = ("ok", "few inliers", "degenerate", "bad object")          # stats[:, 0]
STATS = ("status", "first_inliers", "first_rms", "last_inliers", "last_rms", "steps")


class MeshIcp:
    """``meshes``: a ``lib.mesh_set.MeshSet`` or the list of (vertices [V,3], triangles [T,3]) it packs, object o being mesh o; ``scales``:
    one factor per mesh (or one for all) that takes its vertices into the units of the point clouds -- for the customCAD loader
    ``model_scale / 10000`` (``MeshSet.scaled``: fp64, rounded to fp32).  ``vertices`` (device, scaled: this object's own),
    ``triangles`` (device, the set's) and ``tri_begin`` (host) are what ``df_mesh_icp`` reads.  ``accel``: find the closest triangles
    through the set's bounding-box tree (``df_mesh_icp_tree``, ``MeshSet.tree``: built here, once per set and scale) -- the same poses
    and stats byte for byte, in a fraction of the time on meshes of 1e4 triangles and more."""

    def __init__(self, meshes, scales=1.0, device="cuda", accel=False):
        ms = meshes if isinstance(meshes, MeshSet) else MeshSet(meshes)
        if ms.n_objects > MAX_OBJECTS:
            raise ValueError(f"mesh_icp: 1..{MAX_OBJECTS} meshes, got {ms.n_objects}")
        scaled = ms.scaled(scales)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("mesh_icp: needs a GPU device (no CPU path)")
        self.vertices, self.triangles = torch.from_numpy(scaled).to(self.device), ms.on(self.device)[1]
        self.device = self.vertices.device                          # with its index
        self.tri_begin, self.n_objects, self._scratch = ms.tri_begin, ms.n_objects, None
        self.tree = ms.tree(scaled) if accel else None

    def scratch_bytes(self, B, N):
        return int(_lib.lib().df_mesh_icp_scratch_bytes(int(self.triangles.shape[0]), int(B), int(N)))

    def refine(self, points, pose, obj, iters=10, max_dist=None, cull=False):
        """points [B,N,3] fp32 (camera frame, the loader's cloud), pose [B,7] fp64 (q wxyz, t: what ``estimate_multi`` returns), obj [B]
        int32 or int64 (the mesh of each item): device tensors on the meshes' device.  ``max_dist``: None (no limit), one distance or one
        per object, in cloud units: a point further from the surface is no inlier.  ``cull``: only faces that look at the camera take
        points.  Returns (pose [B,7] fp64, stats [B,6] fp64 = ``STATS``; status as in ``STATUS``) on the device.  An item with fewer
        than six inliers or with geometry that does not hold six degrees of freedom keeps its pose."""
        points = _lib.need_tensor(points, "mesh_icp", "points", (torch.float32,), (None, None, 3), self.device)
        B, N = int(points.shape[0]), int(points.shape[1])
        pose = _lib.need_tensor(pose, "mesh_icp", "pose", (torch.float64,), (B, 7), self.device)
        obj = _lib.need_tensor(obj, "mesh_icp", "obj", (torch.int32, torch.int64), (B,), self.device).to(torch.int32)
        iters = int(iters)
        if B < 1 or N < 1 or 8 * B * N > INT_MAX:
            raise ValueError(f"mesh_icp: need B, N >= 1 and 8 B N within an int (B {B}, N {N})")
        if not 0 <= iters <= MAX_ITERS:
            raise ValueError(f"mesh_icp: iters must be 0..{MAX_ITERS}, got {iters}")
        md = np.full(self.n_objects, np.inf) if max_dist is None else np.asarray(max_dist, dtype=np.float64).reshape(-1)
        if md.size == 1:
            md = np.repeat(md, self.n_objects)
        if md.size != self.n_objects or not (md > 0).all():
            raise ValueError(f"mesh_icp: max_dist is None, one distance > 0 or one per object ({self.n_objects})")
        md = np.ascontiguousarray(md, dtype=np.float64)
        self._scratch = _lib.grow_scratch(self._scratch, self.scratch_bytes(B, N), self.device)
        pose_out = torch.empty(B, 7, dtype=torch.float64, device=self.device)
        stats = torch.empty(B, 6, dtype=torch.float64, device=self.device)
        call, name, tree = (_lib.lib().df_mesh_icp, "mesh_icp", ()) if self.tree is None else (_lib.lib().df_mesh_icp_tree, "mesh_icp_tree",
                                                                                                 self.tree.args(self.device))
        with _lib.device_guard(self.device):
            _lib.check(call(_lib.dptr(self.vertices), int(self.vertices.shape[0]), _lib.dptr(self.triangles),
                            int(self.triangles.shape[0]), self.tri_begin.ctypes.data_as(ctypes.c_void_p),
                            md.ctypes.data_as(ctypes.c_void_p), self.n_objects, _lib.dptr(obj), _lib.dptr(points), _lib.dptr(pose),
                            B, N, iters, 1 if cull else 0, _lib.dptr(pose_out), _lib.dptr(stats), _lib.dptr(self._scratch),
                            self._scratch.numel(), _lib.current_stream(), *tree), name)
        return pose_out, stats
