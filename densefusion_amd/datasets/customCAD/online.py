"""``RenderedPoseDataset`` -- customCAD items from views rendered on the fly: the interface of ``dataset.PoseDataset`` with no tree on
disk.  A view is drawn, rendered, perturbed by the depth-sensor model, jittered, boxed, counted, cropped, back-projected and given its
model points and target without its frame ever reaching the host.

Items are a pure function of the view seed.  Item i of epoch e is view v = e * frames + i, the view of seed ``first_seed + v`` drawn by
``render.sample_view`` / ``render.sample_scene`` and taken through its ``transforms.txt`` record's text exactly as
tools/render_cad_dataset.py does it (``render.draw_view_records`` / ``draw_scene_records``), so a tree the tool writes from the same
seeds with the same options holds the same frames.  In scene mode the item is the view's own model, ``seed mod n_models``; the other
models and the distractors are occluders in that frame; its mask is ``df_cad_scene_mask`` of the pair (frame, own model) and its visible
fraction comes from a second scene call with only that model present.  A view the tool would skip (``min_pixels``, ``min_visible``) and
a view the loader would not serve (no label, a crop side under 8, no mask pixel in the crop) is the six-``LongTensor([0])`` sentinel.

Different from ``PoseDataset`` by design:
  * every other draw of item v comes from ``random.Random("first_seed/v")``, never from a global stream, in this order: three
    ``uniform`` for ``add_t`` (drawn even when unused, like :144), the jitter plan (``ColorJitter.draw(rng=)``, with ``add_noise``
    only), 32 bits for the ``choose`` seed of ``df_preprocess_objects_cad``, 32 bits for the subset seed of ``df_cad_targets``;
  * the model subset follows the key rule of ``df_cad_targets`` (the rule of ``choose``, include/dfusion.h) instead of
    ``random.sample`` (:170): the same distribution, a uniformly random subset in index order, without Python's stream;
  * the colour jitter always runs on the device (``df_color_jitter``): there is no host frame to hand to PIL;
  * there is no ``host_item``: nothing of an item is CPU work that worker processes could take, so ``train_utils.Prefetcher`` feeds
    it from threads.

Per chunk of views: one render call (plus the solo call in scene mode), the sensor with ``first_frame`` = the chunk's first view seed
(a frame's noise does not depend on the chunking), the jitter, ``df_cad_item_table``, ONE read-back of the table (with the render's
pixel counts appended: [F][10] integers), then ``df_preprocess_objects_cad`` per crop size and ``df_cad_targets`` per model for the
live items.  Poses, plans, seeds and descriptors go up; nothing else crosses the bus.  ``__getitem__`` is served from a small,
lock-protected cache of prepared chunks; ``permutation`` gives an epoch order that walks the chunks one after the other.  Cache,
ready event, ``permutation`` and ``set_epoch`` are ``ChunkedViews``, which ``online_seg.RenderedSegDataset`` shares.

With ``segnet=`` (scenes only) the masks are SegNet's instead of the renderer's, and SegNet is scored against the rendered labels on the
way: between the jitter and ``df_cad_item_table`` the chunk runs ``df_seg_batch`` on the centred window, SegNet,
``df_seg_score`` and ``df_seg_masks``; the read-back stays the one table.
"""
from __future__ import annotations

import os
import random
import threading
from collections import OrderedDict

import numpy as np
import torch

from ...lib import preprocess as pp
from ...lib import segment_score as ss
from ...lib.mesh_set import MeshSet
from .. import augment
from . import render as cr
from .dataset import LABEL_VALUE, MIN_CROP, _sentinel, sample_model_points
from .project_unity_depth import UnityDepthProjector, read_proj_mat
from .symmetry import parse_sym_option


def _is_path(m):
    return isinstance(m, (str, os.PathLike))


class _Chunk:
    def __init__(self):
        self.lock = threading.Lock()
        self.items = None            # per view: the 6-tuple or the sentinel
        self.info = None             # per view: what ``view_info`` returns
        self.ready = None            # recorded on the preparing stream after the last launch


class ChunkedViews:
    """Views of consecutive seeds served from a small, lock-protected cache of prepared chunks (shared by ``RenderedPoseDataset`` and
    ``online_seg.RenderedSegDataset``).  A subclass provides ``_prepare(epoch, a, b)`` -> (items, info, ready): per view of the span
    its item and what ``view_info`` returns, and an event recorded on the preparing stream after the last launch; it holds
    ``_device_lock`` around its device work (the renderers keep one scratch buffer each)."""

    def _init_views(self, chunk, first_seed, frames, cache_chunks, device):
        if int(chunk) < 1 or int(frames) < 1 or int(first_seed) < 0:
            raise ValueError("chunk and frames must be positive, first_seed not negative")
        self.chunk, self.first_seed, self.frames, self.epoch = int(chunk), int(first_seed), int(frames), 0
        self.device = torch.device(device)
        self._cache, self._cache_chunks, self._lock, self._device_lock = OrderedDict(), max(1, int(cache_chunks)), threading.Lock(), threading.Lock()
        self._offset = 0

    def __len__(self):
        return self.frames

    def set_epoch(self, epoch):
        """Moves the seed range by ``epoch * frames``: item i becomes the view of seed ``first_seed + epoch * frames + i``."""
        if int(epoch) < 0:
            raise ValueError("epoch must not be negative")
        self.epoch = int(epoch)
        return self

    def view_seed(self, index):
        return self.first_seed + self.epoch * self.frames + int(index)

    def permutation(self, rs):
        """An epoch order from ``rs`` (a ``np.random.RandomState``) that a chunk cache can serve: the set is cut into runs of ``chunk``
        consecutive views at an offset drawn per call, the runs are shuffled and each run's views are shuffled.  (The views of
        consecutive seeds are independent draws; a plain permutation would have every fetch render a chunk to serve one item.)  The cache
        cuts its chunks at the offset of the latest call; items do not depend on the cut."""
        self._offset = off = int(rs.randint(self.chunk))
        cuts = [0] + list(range(off, self.frames, self.chunk)) if off else list(range(0, self.frames, self.chunk))
        runs = [np.arange(a, b) for a, b in zip(cuts, cuts[1:] + [self.frames])]
        return np.concatenate([rs.permutation(runs[k]) for k in rs.permutation(len(runs))])

    def _span(self, index):
        off = self._offset
        if index < off:
            return 0, min(off, self.frames)
        a = off + (index - off) // self.chunk * self.chunk
        return a, min(a + self.chunk, self.frames)

    def _chunk_of(self, index):
        index = int(index)
        if not 0 <= index < self.frames:
            raise IndexError(index)
        a, b = self._span(index)
        key = (self.epoch, a, b)
        with self._lock:
            slot = self._cache.get(key)
            if slot is None:
                slot = self._cache[key] = _Chunk()
                while len(self._cache) > self._cache_chunks:
                    self._cache.popitem(last=False)
            else:
                self._cache.move_to_end(key)
        with slot.lock:
            if slot.items is None:
                slot.items, slot.info, slot.ready = self._prepare(*key)
        torch.cuda.current_stream(self.device).wait_event(slot.ready)      # a chunk may have been prepared on another stream
        return slot, index - a


class RenderedPoseDataset(ChunkedViews):
    """``models``: a model or a list of them, each a PLY path or arrays -- (points, normals or None, colours) for ``raster="points"``,
    (vertices, triangles, colours) for ``raster="mesh"`` and for scenes.  One model is rendered by the single-object renderers;
    several models, or ``distractors``, or ``scene=True`` make scenes (meshes only; model k is object k + 1 of ``objlist``).  The
    renderer options are those of tools/render_cad_dataset.py under their names there (``image_dims`` = (--height, --width), ``light``
    none / head / random, ``sensor`` a ``render.DepthSensor`` with ``sensor_seed``, ``points`` = --points); ``num``, ``add_noise``,
    ``noise_trans``, ``refine`` are the loader's; ``first_seed`` and ``frames`` name the views: the tool's --seed and the set's length.
    ``raster="points"`` seeds ``np.random`` with ``first_seed`` before a mesh is sampled into a cloud, as the tool does; ``pt[o]`` is
    then drawn like ``ply_vtx`` draws it from the model file the tool would write.
    ``segnet`` (scenes only): an eval-mode ``SegNet`` with ``label_nbr`` = models + 1 whose masks take the place of the renderer's.  Per
    chunk, after render, sensor and jitter: ``df_seg_batch`` cuts the centred ``seg_window`` (default ``online_seg.default_window``) of
    every frame with no background, no noise, no flip and ``seg_blur``; SegNet (``_seg_logits``); ``df_seg_score`` against the rendered
    labels, summed in ``seg_score`` (a ``segment_score.SegScore``); ``df_seg_masks`` of the pairs (view, own model + 1).  From
    ``df_cad_item_table`` on the path is the same.  ``kept`` stays the truth render's, so a run with either mask judges the same views;
    ``live`` follows the mask in use.  With ``segnet=None`` nothing changes by a byte.
    ``symmetry``: "none" (``get_sym_list() == []``), "auto" (meshes only: ``symmetry.detect_symmetry`` per model at construction with
    ``tol`` = ``symmetry_tol`` and ``accel`` = ``symmetry_accel``: the same reports through each model's bounding-box tree; the reports
    are kept in ``self.symmetry`` by model index) or a list of model indices.  The list holds the
    values an item's index takes (model k = index k = object k + 1), which is what the losses, the native trainer and ``evaluate()``
    compare.  No item changes by a byte: the detection draws from a generator of its own.
    ``keep_frames``: ``view_info`` also carries ``depth`` and ``mask``, device views [IH,IW] uint16 of the frames the item was cut from
    (after the sensor; the mask in use), and ``box`` = (rmin, rmax, cmin, cmax) of its crop: what ``pose_verifier()`` scores a pose
    against.  The frames of a cached chunk then stay on the device as long as the chunk does.  No item changes by a byte."""

    def __init__(self, models, num=500, add_noise=False, noise_trans=0.0, refine=False, *, distractors=(), scene=None, raster="points",
                 splat=1, cull=1, mask="box", light="none", shading="flat", light_angle=60.0, sensor=None, sensor_seed=0, proj_mat=None,
                 image_dims=(520, 1109), center=(0.0, 0.0, 4.0), scene_scale=1.0, model_scale=10.0, min_pixels=500, min_visible=0.3,
                 p_present=0.7, lateral=0.8, depth=0.8, max_holes=3, hole_mean=30.0, hole_std=10.0, chunk=32, points=0, first_seed=0,
                 frames=2000, jitter="device", device="cuda", cache_chunks=4, segnet=None, seg_window=None, seg_blur=1, symmetry="none",
                 symmetry_tol=0.01, keep_frames=False, symmetry_accel=False):
        models = [models] if _is_path(models) or (isinstance(models, tuple) and not _is_path(models[0]) and np.ndim(models[0]) == 2) else list(models)
        distractors = list(distractors)
        self.scene = bool(scene) if scene is not None else (len(models) > 1 or len(distractors) > 0)
        if not models or (not self.scene and (len(models) != 1 or distractors)):
            raise ValueError("several models and distractors need a scene; without it exactly one model is rendered")
        if raster not in ("points", "mesh") or mask not in cr.MASK_MODES or light not in ("none", "head", "random") or shading not in ("flat", "smooth"):
            raise ValueError("raster is points / mesh, mask box / pixels, light none / head / random, shading flat / smooth")
        if jitter != "device":
            raise ValueError('a rendered frame never reaches the host: jitter must be "device"')
        if light != "none" and raster != "mesh" and not self.scene:
            raise ValueError("light needs raster mesh or a scene: the point renderer is unlit")
        if sensor is not None and not isinstance(sensor, cr.DepthSensor):
            raise ValueError("sensor must be a render.DepthSensor")
        self._init_views(chunk, first_seed, frames, cache_chunks, device)
        self.num, self.add_noise, self.noise_trans, self.refine = int(num), bool(add_noise), noise_trans, refine
        self.raster, self.splat, self.cull, self.mask = raster, int(splat), int(cull), mask
        self.light, self.light_angle, self.sensor, self.sensor_seed = light, float(light_angle), sensor, int(sensor_seed)
        self.center, self.scene_scale, self.model_scale = [float(v) for v in center], float(scene_scale), float(model_scale)
        self.min_pixels, self.min_visible = int(min_pixels), float(min_visible)
        self.p_present, self.lateral, self.depth = float(p_present), float(lateral), float(depth)
        self.max_holes, self.hole_mean, self.hole_std = int(max_holes), float(hole_mean), float(hole_std)
        self.jitter, self.keep_frames = jitter, bool(keep_frames)
        self.trancolor = augment.ColorJitter(0.2, 0.2, 0.2, 0.05)
        proj = cr.DEFAULT_PROJ if proj_mat is None else (read_proj_mat(proj_mat) if _is_path(proj_mat) else proj_mat)
        self.proj_mat = np.array(proj, dtype=np.float64).reshape(4, 4)
        self.image_dims = (int(image_dims[0]), int(image_dims[1]))
        self.udp = UnityDepthProjector.from_matrix(self.proj_mat, self.image_dims)
        self.n_models = len(models)
        self.objlist = list(range(1, self.n_models + 1))
        normals = shading if light != "none" else None
        self.pt = {}
        if self.scene:
            meshes = [cr.read_colored_mesh(m) if _is_path(m) else m for m in models + distractors]
            if any(len(m[1]) == 0 for m in meshes):
                raise ValueError("a scene needs models with faces")
            packed = MeshSet(meshes, colors=True)                # uploaded once; mesh_icp() and pose_verifier() read its prefix of models
            self.renderer = cr.CadSceneRenderer(packed, self.proj_mat, self.image_dims, [self.model_scale] * len(meshes), device=self.device,
                                                normals=normals)
            self.meshes = packed.first(self.n_models)
            self._n_points = [len(m[0]) for m in meshes]
            self._centroids = [np.asarray(m[0]).astype(np.float64).mean(axis=0) for m in meshes]
            for k in range(self.n_models):
                self.pt[k + 1] = sample_model_points(np.asarray(meshes[k][0], dtype=np.float32).astype(np.float64), np.asarray(meshes[k][1]))
        elif raster == "mesh":
            pts, tris, col = cr.read_colored_mesh(models[0]) if _is_path(models[0]) else models[0]
            if len(tris) == 0:
                raise ValueError("raster mesh needs a model with faces")
            self.meshes = MeshSet([(pts, tris, col)], colors=True)
            self.renderer = cr.CadMeshRenderer(self.meshes, None, None, self.proj_mat, self.image_dims, self.device, self.model_scale, normals)
            self._n_points, self._centroids = [len(pts)], [np.asarray(pts).astype(np.float64).mean(axis=0)]
            self.pt[1] = sample_model_points(np.asarray(pts, dtype=np.float32).astype(np.float64), np.asarray(tris))
        else:
            if _is_path(models[0]):
                np.random.seed(self.first_seed)
                pts, nrm, col = cr.load_cloud(models[0], int(points))
            else:
                pts, nrm, col = models[0]
            self.renderer = cr.CadRenderer(pts, nrm, col, self.proj_mat, self.image_dims, device=self.device, model_scale=self.model_scale)
            self._n_points, self._centroids = [len(pts)], [np.asarray(pts).astype(np.float64).mean(axis=0)]
            self.meshes = None                                   # a point cloud has no surface to fit
            self.pt[1] = sample_model_points(np.asarray(pts, dtype=np.float32).astype(np.float64), np.zeros((0, 3), dtype=np.int64))
        self._pt_dev = {o: torch.from_numpy(np.ascontiguousarray(p, dtype=np.float64)).to(self.device) for o, p in self.pt.items()}
        self.num_pt_mesh_large = self.num_pt_mesh_small = 500
        # which models take ADD-S: the values an item's index takes (model k = index k), as Loss, the trainer and evaluate() compare them
        self.symmetry, self._sym_list = {}, []
        if isinstance(symmetry, str):
            if symmetry not in ("none", "auto"):
                raise ValueError('symmetry is "none", "auto" or a list of model indices')
            if symmetry == "auto":
                if not self.scene and raster != "mesh":
                    raise ValueError('symmetry "auto" needs triangles: a scene or raster mesh (a point cloud has none)')
                from .symmetry import detect_symmetry
                found = meshes[:self.n_models] if self.scene else [(pts, tris, col)]
                with torch.cuda.device(self.device):
                    for k, (mv, mt, mc) in enumerate(found):
                        self.symmetry[k] = detect_symmetry(mv, mt, mc, tol=float(symmetry_tol), accel=bool(symmetry_accel))
                self._sym_list = [k for k in sorted(self.symmetry) if self.symmetry[k].symmetric]
        else:
            self._sym_list = sorted({int(k) for k in symmetry})
            if any(not 0 <= k < self.n_models for k in self._sym_list):
                raise ValueError(f"symmetry: model indices lie in 0..{self.n_models - 1}, got {self._sym_list}")
        self.segnet, self.mask_source = segnet, "truth" if segnet is None else "segnet"
        if segnet is not None:
            from .online_seg import check_window
            if not self.scene:
                raise ValueError("segnet masks need a scene: the label plane is the scene renderer's")
            if segnet.training or segnet.label_nbr != self.n_models + 1:
                raise ValueError(f"segnet must be in eval mode with label_nbr = {self.n_models + 1} (models + background), got "
                                 f"{segnet.label_nbr}{' in training mode' if segnet.training else ''}")
            if int(seg_blur) not in (0, 1):
                raise ValueError("seg_blur is 0 / 1")
            self.seg_window, self.seg_blur = check_window(seg_window, self.image_dims), int(seg_blur)
            # the centred window, for every view; online_seg's class map: model k is class k + 1, distractors are background
            self.seg_corner = ((self.image_dims[0] - self.seg_window[0]) // 2, (self.image_dims[1] - self.seg_window[1]) // 2)
            self.seg_class_map = np.array([0] + list(range(1, self.n_models + 1)) + [0] * len(distractors), dtype=np.int32)
            self.seg_score, self._scored = ss.SegScore(self.n_models + 1, self.device), set()

    @classmethod
    def from_options(cls, opt, models, distractors=(), *, first_seed=0, frames=2000, num=500, add_noise=False, noise_trans=0.0, refine=False,
                     device="cuda", scene=None, segnet=None, seg_window=None, seg_blur=1, symmetry=None, keep_frames=False):
        """The dataset of parsed ``render.add_view_arguments`` options: the views tools/render_cad_dataset.py renders with the same
        flags, ``--model`` = ``models``, ``--distractor`` = ``distractors`` and ``--seed`` = ``first_seed`` (several models or a
        distractor: ``--scene``, which ``scene=True`` also asks of one model alone).  ``ValueError`` for flags the tool refuses."""
        proj = read_proj_mat(opt.proj_mat) if opt.proj_mat else np.array(cr.DEFAULT_PROJ)
        sensor = cr.sensor_from_flags(proj, opt.sensor_sigma, opt.sensor_sigma_z, opt.sensor_z, opt.sensor_edge, opt.sensor_edge_step,
                                      opt.sensor_edge_drop, opt.sensor_drop, opt.sensor_quant)
        return cls(list(models), num, add_noise, noise_trans, refine, distractors=list(distractors), raster=opt.raster, splat=opt.splat,
                   cull=opt.cull, mask=opt.mask, light=opt.light, shading=opt.shading, light_angle=opt.light_angle, sensor=sensor,
                   sensor_seed=opt.sensor_seed, proj_mat=proj, image_dims=(opt.height, opt.width), center=opt.center,
                   scene_scale=opt.scene_scale, model_scale=opt.model_scale, min_pixels=opt.min_pixels, min_visible=opt.min_visible,
                   p_present=opt.p_present, lateral=opt.lateral, depth=opt.depth, max_holes=opt.max_holes, hole_mean=opt.hole_mean,
                   hole_std=opt.hole_std, chunk=opt.chunk, points=opt.points, first_seed=first_seed, frames=frames, device=device,
                   scene=scene, segnet=segnet, seg_window=seg_window, seg_blur=seg_blur,
                   symmetry=symmetry if symmetry is not None else parse_sym_option(getattr(opt, "cad_sym", "none")),
                   symmetry_tol=getattr(opt, "cad_sym_tol", 0.01), symmetry_accel=getattr(opt, "cad_sym_accel", False), keep_frames=keep_frames)

    def get_sym_list(self):
        """The item indices (model k = index k) that are trained and scored with ADD-S: [] unless ``symmetry`` asked for some."""
        return list(self._sym_list)

    def mesh_icp(self, accel=False):
        """A ``lib.mesh_icp.MeshIcp`` of the models' triangles in the units of the items' clouds (vertices x ``model_scale`` / 10000):
        an item's index k names mesh k; ``accel`` is ``MeshIcp``'s.  ``ValueError`` in point-cloud mode: there are no triangles to fit."""
        if self.meshes is None:
            raise ValueError('mesh_icp needs triangles: a scene or raster mesh (a point cloud has none)')
        from ...lib.mesh_icp import MeshIcp
        return MeshIcp(self.meshes, self.model_scale / 10000.0, device=self.device, accel=accel)

    def pose_verifier(self):
        """A ``lib.pose_verify.PoseVerifier`` of the models' triangles, in file units with the renderer's model scale, camera and frame
        size: an item's index k names mesh k, and a pose in the units of the items' clouds is drawn as the renderer would draw it.
        ``ValueError`` in point-cloud mode: there are no triangles to draw."""
        if self.meshes is None:
            raise ValueError('pose_verifier needs triangles: a scene or raster mesh (a point cloud has none)')
        from ...lib.pose_verify import PoseVerifier
        return PoseVerifier(self.meshes, self.model_scale, self.proj_mat, self.image_dims, cloud_div=10000.0, device=self.device)

    def symmetry_sets(self, step=0.01, cap=4096):
        """One symmetry set per model (``symmetry.symmetry_set``: float64 [S,3,4], the identity first) in the units of the items' clouds:
        the rotations of the report ``get_sym_list()`` was made from (no second detection), the translation column scaled like the
        vertices (x ``model_scale`` / 10000).  A model outside the list gets the identity alone.  ``ValueError`` for a model listed by
        index with no report behind it (``symmetry`` given as a list: which rotations it has is not known), and where a set does not
        close within ``cap``."""
        from .symmetry import symmetry_set
        sets = []
        for k in range(self.n_models):
            if k not in self._sym_list:
                sets.append(np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)[None])
                continue
            if k not in self.symmetry:
                raise ValueError(f'symmetry_sets: model {k} was listed by hand; its rotations come from symmetry "auto" only')
            s = symmetry_set(self.symmetry[k], step=step, cap=cap, name=f"model {k}")
            s[:, :, 3] = s[:, :, 3] * (self.model_scale / 10000.0)
            sets.append(s)
        return sets

    def pose_errors(self, step=0.01, cap=4096):
        """A ``lib.pose_error.PoseErrors`` of the models' vertices in the units of the items' clouds with ``symmetry_sets(step, cap)``,
        the renderer's camera and frame size: an item's index k names mesh k.  ``ValueError`` in point-cloud mode: the errors are taken
        over the vertices of a mesh.  With ``keep_frames`` it also carries the loader's ray map, which ``.vsd`` needs; without, ``.vsd``
        raises."""
        if self.meshes is None:
            raise ValueError('pose_errors needs a mesh: a scene or raster mesh (a point cloud has none)')
        from ...lib.pose_error import PoseErrors
        errors = PoseErrors(self.meshes, self.model_scale, self.symmetry_sets(step, cap), self.proj_mat, self.image_dims, cloud_div=10000.0,
                            device=self.device)
        # VSD scores against the frames an item was cut from: only a dataset that keeps them hands over the loader's rays
        return errors.set_rays(self.udp.ray_map_on(self.device)) if self.keep_frames else errors

    def dense_refiner(self):
        """A ``lib.pose_refine_dense.DensePoseRefiner`` of the models' triangles, in file units with the renderer's model scale, camera
        and frame size, carrying the loader's ray map: an item's index k names mesh k, and a pose in the units of the items' clouds is
        refined against the frame the item was cut from.  ``ValueError`` in point-cloud mode (there are no triangles to draw) and without
        ``keep_frames`` (there is no frame to refine against)."""
        if self.meshes is None:
            raise ValueError('dense_refiner needs triangles: a scene or raster mesh (a point cloud has none)')
        if not self.keep_frames:
            raise ValueError('dense_refiner needs the frames the items were cut from: RenderedPoseDataset(keep_frames=True)')
        from ...lib.pose_refine_dense import DensePoseRefiner
        refiner = DensePoseRefiner(self.meshes, self.model_scale, self.proj_mat, self.image_dims, cloud_div=10000.0, device=self.device)
        return refiner.set_rays(self.udp.ray_map_on(self.device))

    def contour_refiner(self):
        """A ``lib.pose_refine_contour.ContourPoseRefiner`` built as ``dense_refiner()`` builds its refiner, with the same two
        ``ValueError``s: the dense ICP with an outline term, which holds views of one or two faces that the planes alone leave free."""
        if self.meshes is None:
            raise ValueError('contour_refiner needs triangles: a scene or raster mesh (a point cloud has none)')
        if not self.keep_frames:
            raise ValueError('contour_refiner needs the frames the items were cut from: RenderedPoseDataset(keep_frames=True)')
        from ...lib.pose_refine_contour import ContourPoseRefiner
        refiner = ContourPoseRefiner(self.meshes, self.model_scale, self.proj_mat, self.image_dims, cloud_div=10000.0, device=self.device)
        return refiner.set_rays(self.udp.ray_map_on(self.device))

    def ppf_estimator(self, **model_options):
        """A ``lib.pose_ppf.PpfEstimator`` of the models' meshes sampled in the units of the items' clouds (``model_options``: the keyword
        arguments of ``lib.pose_ppf.PpfModels`` after ``cloud_div``), with the renderer's camera and frame size, carrying the loader's ray
        map: an item's index k names mesh k, and the poses it finds are in the units ``dense_refiner()`` and ``pose_verifier()`` take.
        ``ValueError`` in point-cloud mode (there is no surface to sample) and without ``keep_frames`` (there is no frame to vote on)."""
        if self.meshes is None:
            raise ValueError('ppf_estimator needs triangles: a scene or raster mesh (a point cloud has none)')
        if not self.keep_frames:
            raise ValueError('ppf_estimator needs the frames the items were cut from: RenderedPoseDataset(keep_frames=True)')
        from ...lib.pose_ppf import PpfEstimator, PpfModels
        models = PpfModels(self.meshes, self.model_scale, 10000.0, **model_options)
        estimator = PpfEstimator(models, self.proj_mat, self.image_dims, cloud_div=10000.0, device=self.device)
        return estimator.set_rays(self.udp.ray_map_on(self.device))

    def get_num_points_mesh(self):
        return self.num_pt_mesh_large if self.refine else self.num_pt_mesh_small

    # -- the draws of one item that are not its view ------------------------------------------------------------------------------------
    def _draws(self, view):
        rng = random.Random("%d/%d" % (self.first_seed, view))
        add_t = np.array([rng.uniform(-self.noise_trans, self.noise_trans) for _ in range(3)])
        plan = augment.plan_row(self.trancolor.draw(rng=rng)) if self.add_noise else None
        return add_t, plan, rng.getrandbits(32), rng.getrandbits(32)

    # -- SegNet's masks in place of the renderer's ------------------------------------------------------------------------------------
    def _seg_logits(self, x, target):
        """Channels-last logits [F,H,W,ld] of the window batch x [F,H,W,4]; ``target`` is the rendered truth, which SegNet does not
        see (the seam a test overrides to put known logits in)."""
        with torch.no_grad():
            return self.segnet.forward_nhwc(x)

    def _segnet_masks(self, rgb, label, own, seeds):
        """The masks of the pairs (view, own model + 1) from SegNet's label map of the centred window of each frame, and the frames'
        confusion matrices [F,C,C] against the rendered labels: ``df_seg_batch`` (no background, no noise, no flip), SegNet,
        ``df_seg_score``, ``df_seg_masks``.  Nothing is read back.  A view enters ``seg_score`` once, however often the cache prepares its
        chunk again (its matrix is a function of its seed)."""
        F, (y0, x0) = rgb.shape[0], self.seg_corner
        desc = np.array([[j, y0, x0, 0, -1, 0, 0, 0] for j in range(F)], dtype=np.int64)
        x, target, counts = pp.seg_batch(rgb, label, self.seg_class_map, self.n_models + 1, desc, self.seg_window, blur=self.seg_blur)
        conf, skipped, seg_label = ss.seg_score(self._seg_logits(x, target), target, self.n_models + 1)
        fresh = [j for j in range(F) if seeds[j] not in self._scored]
        if fresh:
            rows = slice(None) if len(fresh) == F else torch.tensor(fresh, dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)
            self.seg_score.add(conf[rows], skipped[rows])
            self._scored.update(seeds[j] for j in fresh)
        mask = ss.seg_masks(seg_label, [[y0, x0]] * F, [[j, own[j] + 1] for j in range(F)], self.image_dims)
        return mask, conf, counts

    # -- one chunk of consecutive views -------------------------------------------------------------------------------------------------
    def _prepare(self, epoch, a, b):
        views = [epoch * self.frames + i for i in range(a, b)]
        seeds = [self.first_seed + v for v in views]
        F = len(views)
        kw = dict(hole_mean=self.hole_mean, hole_std=self.hole_std, private=True)
        if self.scene:
            texts, poses, present = cr.draw_scene_records(seeds, self._n_points, self._centroids, self.n_models, self.center, self.scene_scale,
                                                          self.model_scale, self.max_holes, p_present=self.p_present, lateral=self.lateral,
                                                          depth=self.depth, **kw)
            own = [s % self.n_models for s in seeds]
            texts, own_pose = [texts[j][own[j]] for j in range(F)], poses[np.arange(F), own]
        else:
            texts, poses, holes = cr.draw_view_records(seeds, self._n_points[0], self._centroids[0], self.center, self.scene_scale,
                                                       self.model_scale, self.max_holes, **kw)
            own, own_pose = [0] * F, poses
        light = np.stack([cr.draw_light(self.light, s, self.light_angle)[1] for s in seeds]) if self.light != "none" else None
        draws = [self._draws(v) for v in views]
        dev = self.device
        with self._device_lock:                                  # the renderers keep one scratch buffer each
            if self.scene:
                rgb, depth, label, stats = self.renderer.render(poses, present=present, cull=self.cull, light=light)
                alone = np.zeros_like(present)
                alone[np.arange(F), own] = 1                     # the same poses with the view's own model alone: its unoccluded pixels
                solo = self.renderer.render(poses, present=alone, cull=self.cull)[3]
                pairs = torch.from_numpy(np.stack([np.arange(F), own], axis=1).astype(np.int32)).pin_memory().to(dev, non_blocking=True)
                f_idx, o_idx = pairs[:, 0].long(), pairs[:, 1].long()
                counts = torch.stack([stats[f_idx, o_idx, 0], solo[f_idx, o_idx, 0]], dim=1)
                if self.segnet is None:
                    mask = self.renderer.masks(label, stats, pairs, mask=self.mask)
            else:
                if self.raster == "mesh":
                    rgb, depth, mask, stats = self.renderer.render(poses, holes=holes, cull=self.cull, mask=self.mask, light=light)
                else:
                    rgb, depth, mask, stats = self.renderer.render(poses, holes=holes, splat=self.splat, mask=self.mask)
                counts = torch.stack([stats[:, 0], stats[:, 0]], dim=1)
            if self.sensor is not None:                          # masks and counts stay the clean render's
                depth, _ = cr.apply_sensor(depth, self.sensor, self.sensor_seed, seeds[0])
            if self.add_noise:
                rgb = pp.color_jitter(rgb, np.stack([d[1] for d in draws]), out=rgb)
            seg_conf = seg_counts = None
            if self.segnet is not None:                          # SegNet sees the frame the pose path sees; kept stays the truth render's
                mask, seg_conf, seg_counts = self._segnet_masks(rgb, label, own, seeds)
            table = pp.cad_item_table(depth, mask, LABEL_VALUE, MIN_CROP)
            rows = torch.cat([table, counts], dim=1).tolist()    # the chunk's one read-back: [F][10]
            info, live = [], []
            for j, row in enumerate(rows):
                won, solo_px = row[8], row[9]
                kept, frac = cr.scene_view_kept(won, solo_px, self.min_pixels, self.min_visible) if self.scene else \
                    (bool(cr.view_kept(won, self.min_pixels)), 1.0)
                info.append(dict(seed=seeds[j], object=self.objlist[own[j]], record=texts[j], pose=own_pose[j], table=row[:8], pixels=won,
                                 visible=float(frac), kept=bool(kept), live=bool(kept and row[7]), add_t=draws[j][0], plan=draws[j][1],
                                 choose_seed=draws[j][2], subset_seed=draws[j][3], mask_source=self.mask_source,
                                 conf=None if seg_conf is None else seg_conf[j], seg_counts=None if seg_counts is None else seg_counts[j]))
                if self.keep_frames:
                    info[-1].update(depth=depth[j], mask=mask[j], box=tuple(int(x) for x in row[2:6]))
                if info[-1]["live"]:
                    live.append(j)
            items = [_sentinel() for _ in range(F)]
            if live:
                frame_stats = table[:, :6].contiguous()
                groups, prepared = {}, {}
                for j in live:
                    rmin, rmax, cmin, cmax = rows[j][2:6]
                    groups.setdefault((rmax - rmin, cmax - cmin), []).append(j)
                for members in groups.values():
                    objs = [(j, LABEL_VALUE, tuple(rows[j][2:6]), draws[j][2]) for j in members]
                    add_t = np.stack([draws[j][0] for j in members]) if self.add_noise else None
                    img, cloud, choose, _ = pp.preprocess_objects_cad(rgb, depth, mask, objs, self.num, frame_stats, self.udp.ray_map_on(dev),
                                                                      self.proj_mat[2, 2], self.proj_mat[2, 3], add_t=add_t)
                    for n, j in enumerate(members):
                        prepared[j] = (cloud[n], choose[n], img[n])
                idx_all = torch.tensor(own, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
                for o in sorted({own[j] for j in live}):
                    members = [j for j in live if own[j] == o]
                    pose = own_pose[members].copy()              # [R|T]: R = target_r @ Y_180, T = target_t (render.transform_to_pose)
                    if self.add_noise:
                        for n, j in enumerate(members):
                            pose[n, :, 3] = pose[n, :, 3] + draws[j][0] * 10000            # target_t + add_t * 10000 (:200)
                    target, model_points = pp.cad_targets(self._pt_dev[self.objlist[o]], pose, [draws[j][3] for j in members],
                                                          self.num_pt_mesh_small, model_scale=10.0)
                    for n, j in enumerate(members):
                        idx = idx_all[j:j + 1]
                        idx._host = [own[j]]                     # the trainer's losses branch on the index: spare it a device read-back
                        items[j] = prepared[j] + (target[n], model_points[n], idx)
            ready = torch.cuda.Event()
            ready.record()
        return items, info, ready

    def __getitem__(self, index):
        slot, j = self._chunk_of(index)
        return slot.items[j]

    def batch(self, indices):
        """The 6-tuples of ``indices`` (same order)."""
        return [self[i] for i in indices]

    def view_info(self, index):
        """What is known on the host about item ``index``: its view seed, object, ``transforms.txt`` record and pose [R|t], the row of
        ``df_cad_item_table``, the pixels it won and its visible fraction, ``kept`` (the tool's skip rules), ``live`` (kept and served),
        its own draws (``add_t``, the jitter plan row, the ``choose`` and subset seeds), ``mask_source`` (truth / segnet: whose mask
        ``table`` and ``live`` follow; ``kept`` is always the truth render's) and, with a SegNet, ``conf`` and ``seg_counts``: the
        view's confusion matrix [C,C] against the rendered labels and its window's class pixel counts [C], DEVICE tensors."""
        slot, j = self._chunk_of(index)
        return slot.info[j]
