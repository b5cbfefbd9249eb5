"""Pose hypotheses from depth alone by point-pair-feature voting on the device (``df_pose_ppf``, include/dfusion.h; Drost et al. 2010): a
global search over the sampled CAD model and the item's depth window that needs no start pose and no trained network.  Every pair of an
oriented scene reference point and another scene point looks up the model pairs of the same quantised feature and votes for (model
point, rotation about the normal); the best cell of each reference is a hypothesis, the hypotheses are clustered greedily and the K best
clusters come back, to be refined by ``lib.pose_refine_dense.DensePoseRefiner`` and told apart by ``lib.pose_verify.PoseVerifier``.  The
rule is written out as numbered steps in fp64 with no trigonometry on the device; tests/pose_ppf_np.py restates it and the outputs are
compared bit for bit.  ``PpfModels`` samples the meshes and builds the tables once on the host (``df_ppf_model_build``);
``PpfEstimator.estimate`` enqueues on the current stream and without a host sync.  ``RenderedPoseDataset.ppf_estimator()`` builds one for
its models and tools/eval_cad_render.py ``--ppf`` is its user.
"""
from __future__ import annotations

import ctypes
import math
import time

import numpy as np
import torch

from .. import _lib
from .mesh_set import MeshSet

MAX_OBJECTS = 64
MAX_POINTS, MAX_ACC_BYTES = 1024, 150 * 1024
MAX_ND, MAX_NANG, MAX_NA = 64, 32, 64
MAX_GRID, MAX_REFS, MAX_K, MAX_STEP, MAX_REACH = 16384, 4096, 16, 64, 8
STATUS = {0: "ok", 1: "no hypothesis", 3: "bad item"}                # stats[:, 0]
STATS = ("status", "usable", "hypotheses", "clusters")


def ppf_tables(angle_bins, alpha_bins):
    """The three host tables of ``df_pose_ppf``: the boundary cosines of the feature angles [angle_bins-1], those of the upper half turn
    [alpha_bins/2-1] and (cos, sin) of the sector centres [alpha_bins,2]."""
    ang_cos = np.cos(np.arange(1, angle_bins, dtype=np.float64) * (math.pi / angle_bins))
    alpha_cos = np.cos(np.arange(1, alpha_bins // 2, dtype=np.float64) * (2.0 * math.pi / alpha_bins))
    centre = (np.arange(alpha_bins, dtype=np.float64) + 0.5) * (2.0 * math.pi / alpha_bins)
    return ang_cos, alpha_cos, np.ascontiguousarray(np.stack([np.cos(centre), np.sin(centre)], axis=1))


def sample_surface(vertices, triangles, n, rng):
    """``n`` samples of a mesh's surface with their face normals, fp64: triangles drawn by area, uniform barycentrics, from ``rng``."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    a, e1, e2 = v[t[:, 0]], v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
    nrm = np.cross(e1, e2)
    area = np.linalg.norm(nrm, axis=1)
    live = area > 0
    if not live.any():
        raise ValueError("pose_ppf: a mesh without a face cannot be sampled")
    tri = rng.choice(np.nonzero(live)[0], size=n, p=area[live] / area[live].sum())
    u, w = rng.random(n), rng.random(n)
    over = u + w > 1.0
    u, w = np.where(over, 1.0 - u, u), np.where(over, 1.0 - w, w)
    return a[tri] + u[:, None] * e1[tri] + w[:, None] * e2[tri], nrm[tri] / area[tri][:, None]


class PpfModels:
    """The sampled models and their pair tables.  ``meshes``: a ``MeshSet`` or a list of (vertices, triangles) in file units;
    ``model_scale`` (one per mesh, or one for all) and ``cloud_div`` take them to the units of the poses (x scale / cloud_div).  Per mesh
    ``points`` samples (2..1024, with points x alpha_bins x 4 <= 150 KiB) from ``numpy.random.default_rng([seed, o])``; ``dist_step`` =
    ``dist_frac`` x the diagonal of the samples' bounding box (``diameter``).  Host arrays: ``points``, ``normals`` [NM,3] fp64,
    ``point_begin``, ``dist_step``, ``diameter``, ``bucket_begin`` [O,NKEY+1], ``entry_point`` [E], ``entry_cs`` [E,2] and the tables
    ``ang_cos``, ``alpha_cos``, ``alpha_cs``; ``build_seconds`` is the host time of ``df_ppf_model_build``.  ``on(device)`` uploads once."""

    def __init__(self, meshes, model_scale, cloud_div=10000.0, points=400, seed=0, dist_frac=0.05, angle_bins=15, alpha_bins=30):
        ms = meshes if isinstance(meshes, MeshSet) else MeshSet(meshes)
        O = ms.n_objects
        if O > MAX_OBJECTS:
            raise ValueError(f"pose_ppf: 1..{MAX_OBJECTS} meshes, got {O}")
        scales = np.asarray(model_scale, dtype=np.float64).reshape(-1)
        if scales.size not in (1, O) or not (np.isfinite(scales).all() and (scales > 0).all()) or not (np.isfinite(cloud_div) and cloud_div > 0):
            raise ValueError("pose_ppf: one positive finite model scale per mesh, or one for all, and a cloud_div finite and > 0")
        scales = np.broadcast_to(scales, (O,))
        counts = np.broadcast_to(np.asarray(points, dtype=np.int64).reshape(-1), (O,))
        NANG, NA = int(angle_bins), int(alpha_bins)
        if not 1 <= NANG <= MAX_NANG or not 2 <= NA <= MAX_NA or NA % 2:
            raise ValueError(f"pose_ppf: angle_bins in 1..{MAX_NANG} and an even alpha_bins in 2..{MAX_NA}, got {NANG} and {NA}")
        if not 0 < dist_frac <= 1 or int(math.floor(1.0 / dist_frac)) + 1 > MAX_ND:
            raise ValueError(f"pose_ppf: dist_frac in (0, 1] with at most {MAX_ND} distance bins, got {dist_frac}")
        if (counts < 2).any() or (counts > MAX_POINTS).any() or (counts * NA * 4 > MAX_ACC_BYTES).any():
            raise ValueError(f"pose_ppf: 2..{MAX_POINTS} points per mesh with points x alpha_bins x 4 <= {MAX_ACC_BYTES} bytes, got {counts.tolist()}")
        self.n_objects, self.ND, self.NANG, self.NA = O, int(math.floor(1.0 / dist_frac)) + 1, NANG, NA
        self.ang_cos, self.alpha_cos, self.alpha_cs = ppf_tables(NANG, NA)
        pts, nrm, diag = [], [], []
        for o in range(O):
            v = ms.vertices[ms.vertex_begin[o]:ms.vertex_begin[o + 1]].astype(np.float64) * (float(scales[o]) / float(cloud_div))
            t = ms.triangles[ms.tri_begin[o]:ms.tri_begin[o + 1]].astype(np.int64) - int(ms.vertex_begin[o])
            p, n = sample_surface(v, t, int(counts[o]), np.random.default_rng([int(seed), o]))
            pts.append(p); nrm.append(n)
            diag.append(float(np.linalg.norm(p.max(axis=0) - p.min(axis=0))))
        self.points, self.normals = np.ascontiguousarray(np.concatenate(pts)), np.ascontiguousarray(np.concatenate(nrm))
        self.point_begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        self.diameter = np.array(diag, dtype=np.float64)
        self.dist_step = np.ascontiguousarray(self.diameter * float(dist_frac))
        if not (self.dist_step > 0).all():
            raise ValueError("pose_ppf: a model's samples span no volume")
        L = _lib.lib()
        nb, ne, used = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        _lib.check(L.df_ppf_model_sizes(self.point_begin.ctypes.data, O, self.ND, NANG, ctypes.addressof(nb), ctypes.addressof(ne)), "ppf_model_sizes")
        self.bucket_begin = np.zeros(nb.value, dtype=np.int32)
        entry_point, entry_cs = np.zeros(max(1, ne.value), dtype=np.int32), np.zeros((max(1, ne.value), 2), dtype=np.float32)
        t0 = time.perf_counter()
        _lib.check(L.df_ppf_model_build(self.points.ctypes.data, self.normals.ctypes.data, len(self.points), self.point_begin.ctypes.data,
                                        self.dist_step.ctypes.data, O, self.ND, NANG, NA, self.ang_cos.ctypes.data, self.bucket_begin.ctypes.data,
                                        entry_point.ctypes.data, entry_cs.ctypes.data, ctypes.addressof(used)), "ppf_model_build")
        self.build_seconds = time.perf_counter() - t0
        self.n_entries = int(used.value)
        # at least one element each: an empty array has no pointer to give, and the call refuses a null one
        self.entry_point, self.entry_cs = entry_point[:max(1, self.n_entries)].copy(), entry_cs[:max(1, self.n_entries)].copy()
        self.bucket_begin = self.bucket_begin.reshape(O, -1)
        self._on = {}

    def on(self, device):
        """(points, normals, bucket_begin, entry_point, entry_cs) as tensors on ``device``: uploaded on first use, then the same objects."""
        device = torch.empty(0, device=device).device
        if device not in self._on:
            self._on[device] = tuple(torch.from_numpy(a).to(device) for a in (self.points, self.normals, self.bucket_begin, self.entry_point,
                                                                              self.entry_cs))
        return self._on[device]


class PpfEstimator:
    """``models``: a ``PpfModels``; ``proj``, ``image_dims`` and ``cloud_div`` as for ``lib.pose_verify.PoseVerifier``.  ``set_rays`` hands
    over the loader's ray map, which ``estimate`` needs."""

    def __init__(self, models, proj, image_dims, cloud_div=10000.0, device="cuda"):
        if not isinstance(models, PpfModels):
            raise ValueError("pose_ppf: models must be a PpfModels")
        self.models = models
        self.proj = np.ascontiguousarray(proj, dtype=np.float64).reshape(-1)
        if self.proj.size != 16:
            raise ValueError("pose_ppf: proj is a 4 x 4 matrix")
        self.image_dims, self.cloud_div = (int(image_dims[0]), int(image_dims[1])), float(cloud_div)
        if self.image_dims[0] < 1 or self.image_dims[1] < 1 or not (np.isfinite(self.cloud_div) and self.cloud_div > 0):
            raise ValueError("pose_ppf: image_dims must be positive and cloud_div finite and > 0")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("pose_ppf: needs a GPU device (no CPU path)")
        self._dev = models.on(self.device)
        self.device = self._dev[0].device                            # with its index
        self.rays, self._scratch = None, None

    def set_rays(self, ray_map):
        """``ray_map`` [IH,IW,3] fp64 on the device: the loader's back-projection rays at unit depth (``UnityDepthProjector.ray_map_on``).
        ``RenderedPoseDataset.ppf_estimator()`` sets it."""
        self.rays = _lib.need_tensor(ray_map, "pose_ppf", "ray_map", (torch.float64,), (self.image_dims[0], self.image_dims[1], 3), self.device)
        return self

    def scratch_bytes(self, B, window, step=1, ref_step=5):
        return int(_lib.lib().df_pose_ppf_scratch_bytes(int(B), int(window[0]), int(window[1]), int(step), int(ref_step)))

    def references(self, window, step=1, ref_step=5):
        """NR: the references of one item, the second size of ``hyp``."""
        g = [(int(w) + step - 1) // step for w in window]
        return ((g[0] + ref_step - 1) // ref_step) * ((g[1] + ref_step - 1) // ref_step)

    def estimate(self, depth, frame, obj, corner, window, step=1, reach=1, gate=16, ref_step=5, k=4, cluster_deg=15.0, cluster_frac=0.1,
                 mask=None, mask_frame=None, mask_value=65535, hyp=False):
        """depth [F,IH,IW] uint16 (observed codes, 65535 = no observation), frame and obj [B] and corner [B,2] int32 or int64 as for
        ``PoseVerifier.score``: device tensors on the models' device.  ``window`` = (WH, WW), one size for the call.  The scene points are
        the window's nodes on a grid of ``step`` (at most 16384), their normals come from the neighbours at ``reach`` nodes (1..8) whose
        code differs by at most ``gate`` (0..65535); every ``ref_step``-th grid row and column holds a reference (at most 4096).  ``k`` in
        1..16 clusters come back; two hypotheses share a cluster within ``cluster_deg`` degrees and ``cluster_frac`` x the model's
        ``diameter``.  ``mask`` [NM,IH,IW] uint16 with ``mask_frame`` [B] (default: ``frame``) and ``mask_value`` (an int for all, or
        [B]): only nodes where the mask holds the value are scene points.  Returns (pose [B,k,7] fp64, rank 0 the best cluster; votes
        [B,k,2] int32 = (score, members); stats [B,4] fp64 = ``STATS``, status by ``STATUS``), with ``hyp`` also every reference's
        hypothesis [B,NR,8] = (q, t, votes), on the device; nothing is read back.  A missing rank is all zeros: a pose that draws nothing.
        Raises ``ValueError`` without a ray map."""
        if self.rays is None:
            raise ValueError("pose_ppf: estimate needs the loader's ray map and the frames "
                             "(RenderedPoseDataset(keep_frames=True).ppf_estimator(), or set_rays)")
        dev, ints, md = self.device, (torch.int32, torch.int64), self.models
        IH, IW = self.image_dims
        depth = _lib.need_tensor(depth, "pose_ppf", "depth", (torch.uint16,), (None, IH, IW), dev)
        frame = _lib.need_tensor(frame, "pose_ppf", "frame", ints, (None,), dev)
        B = int(frame.shape[0])
        obj = _lib.need_tensor(obj, "pose_ppf", "obj", ints, (B,), dev)
        corner = _lib.need_tensor(corner, "pose_ppf", "corner", ints, (B, 2), dev)
        WH, WW, step, reach, gate, ref_step, K = int(window[0]), int(window[1]), int(step), int(reach), int(gate), int(ref_step), int(k)
        if not 1 <= B <= 65535 or not 1 <= int(depth.shape[0]) <= 65535:
            raise ValueError(f"pose_ppf: need 1..65535 items and frames (B {B}, F {int(depth.shape[0])})")
        if WH < 1 or WW < 1 or WH * WW > 2 ** 30:
            raise ValueError(f"pose_ppf: window {WH} x {WW} outside 1..2^30 nodes")
        if not 1 <= step <= MAX_STEP or not 1 <= ref_step <= MAX_STEP or not 1 <= reach <= MAX_REACH or not 0 <= gate <= 65535 or not 1 <= K <= MAX_K:
            raise ValueError(f"pose_ppf: step and ref_step must be 1..{MAX_STEP}, reach 1..{MAX_REACH}, gate 0..65535 codes and k 1..{MAX_K}, got "
                             f"{step}, {ref_step}, {reach}, {gate} and {K}")
        G, NR = ((WH + step - 1) // step) * ((WW + step - 1) // step), self.references((WH, WW), step, ref_step)
        if G > MAX_GRID or NR > MAX_REFS:
            raise ValueError(f"pose_ppf: {G} grid nodes and {NR} references, at most {MAX_GRID} and {MAX_REFS}: raise step or ref_step")
        if not 0 <= cluster_deg <= 180 or not (np.isfinite(cluster_frac) and cluster_frac >= 0):
            raise ValueError(f"pose_ppf: cluster_deg in 0..180 and cluster_frac finite and >= 0, got {cluster_deg} and {cluster_frac}")
        NM = 0
        if mask is not None:
            mask = _lib.need_tensor(mask, "pose_ppf", "mask", (torch.uint16,), (None, IH, IW), dev)
            NM = int(mask.shape[0])
            if NM < 1:
                raise ValueError("pose_ppf: an empty mask")
            mask_frame = frame if mask_frame is None else _lib.need_tensor(mask_frame, "pose_ppf", "mask_frame", ints, (B,), dev)
            if torch.is_tensor(mask_value):
                mask_value = _lib.need_tensor(mask_value, "pose_ppf", "mask_value", ints, (B,), dev)
        elif mask_frame is not None:
            raise ValueError("pose_ppf: mask_frame without a mask")
        items = torch.zeros(B, 6, dtype=torch.int32, device=dev)
        items[:, 0], items[:, 1], items[:, 2:4] = frame, obj, corner
        if mask is not None:
            items[:, 4], items[:, 5] = mask_frame, mask_value
        self._scratch = _lib.grow_scratch(self._scratch, self.scratch_bytes(B, (WH, WW), step, ref_step), dev)
        pose_out = torch.empty(B, K, 7, dtype=torch.float64, device=dev)
        votes_out = torch.empty(B, K, 2, dtype=torch.int32, device=dev)
        stats = torch.empty(B, len(STATS), dtype=torch.float64, device=dev)
        hyp_out = torch.empty(B, NR, 8, dtype=torch.float64, device=dev) if hyp else None
        cluster_dist = np.ascontiguousarray(md.diameter * float(cluster_frac))
        points, normals, bucket_begin, entry_point, entry_cs = self._dev
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        with _lib.device_guard(dev):
            _lib.check(_lib.lib().df_pose_ppf(
                _lib.dptr(points), _lib.dptr(normals), int(points.shape[0]), ptr(md.point_begin), ptr(md.dist_step), ptr(cluster_dist),
                md.n_objects, _lib.dptr(bucket_begin), _lib.dptr(entry_point), _lib.dptr(entry_cs), md.n_entries, md.ND, md.NANG, md.NA,
                ptr(md.ang_cos), ptr(md.alpha_cos), ptr(md.alpha_cs), ptr(self.proj), _lib.dptr(depth), int(depth.shape[0]), IH, IW,
                _lib.dptr(self.rays), _lib.dptr(mask) if mask is not None else None, NM, _lib.dptr(items), self.cloud_div, B, WH, WW, step, reach,
                gate, ref_step, K, 1.0 + 2.0 * math.cos(math.radians(float(cluster_deg))), _lib.dptr(pose_out), _lib.dptr(votes_out),
                _lib.dptr(stats), _lib.dptr(hyp_out) if hyp else None, _lib.dptr(self._scratch), self._scratch.numel(), _lib.current_stream()),
                "pose_ppf")
        return (pose_out, votes_out, stats, hyp_out) if hyp else (pose_out, votes_out, stats)
