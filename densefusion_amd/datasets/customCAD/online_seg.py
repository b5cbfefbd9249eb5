"""``RenderedSegDataset`` -- SegNet training items from customCAD scenes rendered on the fly: the work of
``vanilla_segmentation.data_controller.SegDataset.__getitem__`` with no tree on disk and no frame on the host.  A view is drawn,
rendered with its label plane, jittered, cut to a window, composited over a real background where nothing was drawn, blurred, given
pixel noise, flipped, normalised and written as SegNet's channels-last input with its int64 target (``df_seg_batch``).

Items are a pure function of the view seed.  Item i of epoch e is view v = e * frames + i, the scene of seed ``first_seed + v`` drawn
by ``render.draw_scene_records`` with the options tools/render_cad_dataset.py takes, so ``--scene`` writes the same frames from the
same seeds.  Model k is class k + 1; distractors are drawn, keep their colour and are class 0.  Every view is served, also one whose
window holds no model pixel: a negative frame is a valid segmentation sample, so there is no sentinel.  Every other draw of item v
comes from ``random.Random("seg/first_seed/v")`` in the order of ``seg_draws``.

Different from ``SegDataset`` by design:
  * the index is honoured (the reference draws a random frame whatever index it is given);
  * the pixel noise is an integer sum of four uniforms (step D5 of ``df_cad_depth_sensor``) applied AFTER the composite, to object and
    background alike, and the result is clamped to 0..255; the reference adds float N(0, 5) to the synthetic frame only and lets the
    sum leave the range;
  * backgrounds are not jittered, and they carry no labels of their own: a background pixel is class 0;
  * the blur is the 3 x 3 binomial [1 2 1] x [1 2 1] / 16 in integers over the composited window, not PIL's GaussianBlur(0.8) of the
    synthetic frame, and there is no Brightness(1.5): the renderer has its own lighting;
  * a window is cut (SegNet needs multiples of 32, the 520 x 1109 frame is not), at a corner drawn per item;
  * the loader returns channels-last ``(x [H,W,4] float32, target [H,W] int64)`` device views, for ``SegNet.forward_nhwc``.

Per chunk of F views: one render call, ``df_color_jitter`` with ``use_noise``, one ``df_seg_batch``.  Poses, ``present``, lights, plan
rows and descriptors go up from pinned memory; NOTHING is read back.  Chunk cache and ready events are ``online.ChunkedViews``.
"""
from __future__ import annotations

import os
import random

import numpy as np
import torch

from ...lib import preprocess as pp
from .. import augment
from . import render as cr
from .online import ChunkedViews, _is_path
from .project_unity_depth import read_proj_mat

FLIP_OF_DRAW = (1, 2, 3, 0)           # SegDataset's randint(0, 3): 0 left-right, 1 up-down, 2 both, 3 none -> bit 0 left-right, bit 1 up-down


def default_window(image_dims):
    """The largest multiples of 32 inside the frame (512 x 1088 at 520 x 1109)."""
    return int(image_dims[0]) // 32 * 32, int(image_dims[1]) // 32 * 32


def check_window(window, image_dims):
    """(H, W) of ``window`` (None: ``default_window``); ``ValueError`` unless both are positive multiples of 32 that fit the frame."""
    H, W = default_window(image_dims) if window is None else (int(window[0]), int(window[1]))
    if H < 32 or W < 32 or H % 32 or W % 32 or H > int(image_dims[0]) or W > int(image_dims[1]):
        raise ValueError(f"window {H} x {W}: both sides must be multiples of 32 (SegNet's rule) inside the {image_dims[0]} x {image_dims[1]} frame")
    return H, W


def noise_mul_of(sigma):
    """``noise_mul`` of step G4 for noise of standard deviation ``sigma`` grey levels; 0 turns the noise off."""
    if sigma < 0:
        raise ValueError("noise_sigma must not be negative")
    mul = int(np.rint(float(sigma) * 2.0 ** 32 / np.sqrt(float(cr.NOISE_VARIANCE))))
    if mul >= 2 ** 31:
        raise ValueError("noise_sigma is too large for a 32-bit multiplier")
    return mul


def seg_draws(first_seed, view, use_noise, image_dims, window, pool=None, trancolor=None):
    """The draws of item ``view`` that are not its scene, from ``random.Random("seg/%d/%d" % (first_seed, view))`` in this order: the
    jitter plan (with ``use_noise`` only), y0 in 0..IH-H, x0 in 0..IW-W, ``randint(0, 3)`` for the flip (always drawn; without
    ``use_noise`` the flip is none), with a background ``pool`` = (NB, BH, BW) the index in 0..NB-1, by0 and bx0, then 32 bits for the
    noise seed.  Returns (plan row or None, [y0, x0, flip, b, by0, bx0, seed]); no pool gives b = -1."""
    rng = random.Random("seg/%d/%d" % (first_seed, view))
    (IH, IW), (H, W) = image_dims, window
    plan = augment.plan_row((trancolor or augment.ColorJitter(0.2, 0.2, 0.2, 0.05)).draw(rng=rng)) if use_noise else None
    y0 = rng.randint(0, IH - H)
    x0 = rng.randint(0, IW - W)
    flip = FLIP_OF_DRAW[rng.randint(0, 3)]
    b, by0, bx0 = -1, 0, 0
    if pool is not None:
        NB, BH, BW = pool
        b = rng.randint(0, NB - 1)
        by0 = rng.randint(0, BH - H)
        bx0 = rng.randint(0, BW - W)
    return plan, [y0, x0, flip if use_noise else 0, b, by0, bx0, rng.getrandbits(32)]


def load_backgrounds(directory, image_dims):
    """The images of ``directory`` (sorted by name) as one uint8 array [NB,IH,IW,3]: each scaled to cover the frame, centre-cropped."""
    from PIL import Image
    IH, IW = int(image_dims[0]), int(image_dims[1])
    out = []
    for name in sorted(os.listdir(directory)):
        if not name.lower().endswith((".png", ".jpg", ".jpeg", ".bmp")):
            continue
        img = Image.open(os.path.join(directory, name)).convert("RGB")
        s = max(IW / img.width, IH / img.height)
        w, h = max(IW, int(round(img.width * s))), max(IH, int(round(img.height * s)))
        img = img.resize((w, h), Image.BILINEAR)
        x, y = (w - IW) // 2, (h - IH) // 2
        out.append(np.asarray(img.crop((x, y, x + IW, y + IH)), dtype=np.uint8))
    if not out:
        raise ValueError(f"no images in {directory}")
    return np.stack(out)


class _Batches:
    """``dataset.batch`` over consecutive runs of ``order``, as a set ``train_utils.Prefetcher`` can walk: item k is the k-th batch,
    (x, target, the batch's class pixel counts [C] int64)."""

    def __init__(self, dataset, order, batch_size):
        self.dataset, self.order, self.batch_size = dataset, [int(i) for i in order], int(batch_size)

    def __len__(self):
        return (len(self.order) + self.batch_size - 1) // self.batch_size

    def __getitem__(self, k):
        return self.dataset.batch(self.order[k * self.batch_size:(k + 1) * self.batch_size], with_counts=True)


class RenderedSegDataset(ChunkedViews):
    """``models`` and ``distractors``: meshes, each a PLY path or (vertices, triangles, colours); always a scene
    (``render.CadSceneRenderer``), also for one model.  The view and renderer options are ``RenderedPoseDataset``'s in scene mode.
    ``window`` = (H, W), multiples of 32 inside the frame (default: the largest); ``backgrounds``: a directory of images, a uint8 array
    [NB,BH,BW,3] with BH >= H and BW >= W, or None (the renderer's grey horizon stays); ``blur`` 0 / 1; ``noise_sigma`` in grey levels
    (0: none); ``use_noise`` as ``SegDataset``'s: off means no jitter, no pixel noise and no flip (the test split), backgrounds and blur
    stay.  ``n_classes`` = models + 1."""

    def __init__(self, models, use_noise=True, *, distractors=(), window=None, backgrounds=None, blur=1, noise_sigma=5.0, cull=1, light="none",
                 shading="flat", light_angle=60.0, proj_mat=None, image_dims=(520, 1109), center=(0.0, 0.0, 4.0), scene_scale=1.0,
                 model_scale=10.0, p_present=0.7, lateral=0.8, depth=0.8, max_holes=3, hole_mean=30.0, hole_std=10.0, chunk=32, first_seed=0,
                 frames=2000, device="cuda", cache_chunks=4):
        models = [models] if _is_path(models) or (isinstance(models, tuple) and not _is_path(models[0]) and np.ndim(models[0]) == 2) else list(models)
        distractors = list(distractors)
        if not models:
            raise ValueError("at least one model")
        if light not in ("none", "head", "random") or shading not in ("flat", "smooth") or int(blur) not in (0, 1):
            raise ValueError("light is none / head / random, shading flat / smooth, blur 0 / 1")
        self._init_views(chunk, first_seed, frames, cache_chunks, device)
        self.image_dims = (int(image_dims[0]), int(image_dims[1]))
        self.window = check_window(window, self.image_dims)
        self.use_noise, self.blur, self.noise_sigma = bool(use_noise), int(blur), float(noise_sigma)
        self.noise_mul = noise_mul_of(self.noise_sigma)
        self.cull, self.light, self.light_angle = int(cull), light, float(light_angle)
        self.center, self.scene_scale, self.model_scale = [float(v) for v in center], float(scene_scale), float(model_scale)
        self.p_present, self.lateral, self.depth = float(p_present), float(lateral), float(depth)
        self.max_holes, self.hole_mean, self.hole_std = int(max_holes), float(hole_mean), float(hole_std)
        self.trancolor = augment.ColorJitter(0.2, 0.2, 0.2, 0.05)
        proj = cr.DEFAULT_PROJ if proj_mat is None else (read_proj_mat(proj_mat) if _is_path(proj_mat) else proj_mat)
        self.proj_mat = np.array(proj, dtype=np.float64).reshape(4, 4)
        meshes = [cr.read_colored_mesh(m) if _is_path(m) else m for m in models + distractors]
        if any(len(m[1]) == 0 for m in meshes):
            raise ValueError("a scene needs models with faces")
        if len(meshes) > 64:
            raise ValueError("at most 64 objects in a scene")
        self.n_models, self.n_classes = len(models), len(models) + 1
        self.class_map = np.array([0] + list(range(1, self.n_models + 1)) + [0] * len(distractors), dtype=np.int32)
        if backgrounds is not None:
            back = load_backgrounds(backgrounds, self.image_dims) if _is_path(backgrounds) else np.asarray(backgrounds)
            if back.dtype != np.uint8 or back.ndim != 4 or back.shape[3] != 3 or back.shape[0] < 1 or back.shape[1] < self.window[0] or \
                    back.shape[2] < self.window[1]:
                raise ValueError("backgrounds must be a uint8 array [NB,BH,BW,3] that holds the window")
            self.pool = tuple(int(v) for v in back.shape[:3])
            self.back = torch.from_numpy(np.ascontiguousarray(back)).to(self.device)      # the pool goes up once
        else:
            self.pool, self.back = None, None
        self.renderer = cr.CadSceneRenderer(meshes, self.proj_mat, self.image_dims, [self.model_scale] * len(meshes), device=self.device,
                                            normals=shading if light != "none" else None)
        self._n_points = [len(m[0]) for m in meshes]
        self._centroids = [np.asarray(m[0]).astype(np.float64).mean(axis=0) for m in meshes]

    @classmethod
    def from_options(cls, opt, models, distractors=(), *, first_seed=0, frames=2000, use_noise=True, window=None, backgrounds=None, blur=1,
                     noise_sigma=5.0, device="cuda"):
        """The dataset of parsed ``render.add_view_arguments`` options: the scenes ``tools/render_cad_dataset.py --scene`` renders with
        the same flags, ``--model`` = ``models``, ``--distractor`` = ``distractors`` and ``--seed`` = ``first_seed``.  The options that
        select a renderer, a mask, a depth sensor or a skip rule have no part here: a scene of meshes, every view served."""
        proj = read_proj_mat(opt.proj_mat) if opt.proj_mat else np.array(cr.DEFAULT_PROJ)
        return cls(list(models), use_noise, distractors=list(distractors), window=window, backgrounds=backgrounds, blur=blur,
                   noise_sigma=noise_sigma, cull=opt.cull, light=opt.light, shading=opt.shading, light_angle=opt.light_angle, proj_mat=proj,
                   image_dims=(opt.height, opt.width), center=opt.center, scene_scale=opt.scene_scale, model_scale=opt.model_scale,
                   p_present=opt.p_present, lateral=opt.lateral, depth=opt.depth, max_holes=opt.max_holes, hole_mean=opt.hole_mean,
                   hole_std=opt.hole_std, chunk=opt.chunk, first_seed=first_seed, frames=frames, device=device)

    def _draws(self, view):
        return seg_draws(self.first_seed, view, self.use_noise, self.image_dims, self.window, self.pool, self.trancolor)

    # -- one chunk of consecutive views -------------------------------------------------------------------------------------------------
    def _prepare(self, epoch, a, b):
        views = [epoch * self.frames + i for i in range(a, b)]
        seeds = [self.first_seed + v for v in views]
        F = len(views)
        texts, poses, present = cr.draw_scene_records(seeds, self._n_points, self._centroids, self.n_models, self.center, self.scene_scale,
                                                      self.model_scale, self.max_holes, p_present=self.p_present, lateral=self.lateral,
                                                      depth=self.depth, hole_mean=self.hole_mean, hole_std=self.hole_std, private=True)
        light = np.stack([cr.draw_light(self.light, s, self.light_angle)[1] for s in seeds]) if self.light != "none" else None
        draws = [self._draws(v) for v in views]
        desc = np.array([[j] + draws[j][1] for j in range(F)], dtype=np.int64)
        with self._device_lock:                                  # the renderer keeps one scratch buffer
            rgb, _, label, _ = self.renderer.render(poses, present=present, cull=self.cull, light=light)
            if self.use_noise:
                rgb = pp.color_jitter(rgb, np.stack([d[0] for d in draws]), out=rgb)
            x, target, counts = pp.seg_batch(rgb, label, self.class_map, self.n_classes, desc, self.window, back=self.back, blur=self.blur,
                                             noise_mul=self.noise_mul if self.use_noise else 0)
            ready = torch.cuda.Event()
            ready.record()
        items = [(x[j], target[j]) for j in range(F)]
        info = [dict(seed=seeds[j], records=texts[j], poses=poses[j], present=present[j], light=None if light is None else light[j],
                     plan=draws[j][0], desc=desc[j].copy(), counts=counts[j]) for j in range(F)]
        return items, info, ready

    def __getitem__(self, index):
        """(x [H,W,4] float32, target [H,W] int64): device views into the item's chunk."""
        slot, j = self._chunk_of(index)
        return slot.items[j]

    def batch(self, indices, with_counts=False):
        """(x [n,H,W,4], target [n,H,W]) of ``indices``, stacked in their order; ``with_counts``: and the batch's class pixel counts
        [n_classes] int64, still on the device."""
        got = [self._chunk_of(i) for i in indices]
        x = torch.stack([slot.items[j][0] for slot, j in got])
        target = torch.stack([slot.items[j][1] for slot, j in got])
        if not with_counts:
            return x, target
        return x, target, torch.stack([slot.info[j]["counts"] for slot, j in got]).sum(dim=0)

    def batches(self, order, batch_size):
        """``batch`` over consecutive runs of ``batch_size`` indices of ``order``: what ``train_utils.Prefetcher`` walks."""
        return _Batches(self, order, batch_size)

    def view_info(self, index):
        """What is known about item ``index`` without a read-back: its view seed, the scene's ``transforms.txt`` records, poses,
        ``present`` row and light, its jitter plan row (None without ``use_noise``), its descriptor row {f, y0, x0, flip, b, by0, bx0,
        seed} (f the view's place in its chunk) and ``counts``, its row of class pixel counts, a DEVICE tensor."""
        slot, j = self._chunk_of(index)
        return slot.info[j]
