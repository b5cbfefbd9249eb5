#!/usr/bin/env python
"""Evaluate a SegNet and a pose network pair on customCAD scenes rendered on the fly, with no tree on disk.

    python tools/eval_cad_render.py --cad_model a.ply b.ply --cad_distractor box.ply --segnet segnet.pth \\
        --model pose_model.pth --refine_model pose_refine_model.pth --cad_frames 500 --light random

The views are those of ``RenderedPoseDataset`` (datasets/customCAD/online.py) for ``--cad_seed`` and ``--cad_frames`` and the view
options of tools/render_cad_dataset.py.  ``--masks truth`` scores the poses from the renderer's own masks, as tools/eval_cad.py does on a
tree; ``--masks segnet`` from the masks SegNet predicts for the same frames (``df_seg_score`` and ``df_seg_masks``);
``--masks both`` (the default) runs the two on the same view seeds.  The loop is ``evaluate()`` of tools/eval_linemod.py with the
thresholds of tools/eval_cad.py: ``--threshold_frac`` x the diameter of each model's cloud.
``--cad_sym auto`` (default ``none``; or model indices) scores the models ``datasets/customCAD/symmetry.py`` finds symmetric with ADD-S
through the dataset's ``get_sym_list()``; the line ``symmetry object list: ...`` shows which.

Per mask source the log ``eval_result_logs_<source>.txt`` holds the reference-format lines, then per object and overall the ADD success
over the SERVED views (a view whose mask gives an item), the same over the KEPT views (the views the renderer's skip rules keep, the same
set for both sources: a kept view whose mask yields no item counts as a miss) and the numbers of kept and served views.  For ``segnet``
it also holds per-class IoU, precision and recall, mean IoU and pixel accuracy against the rendered labels.  ``main`` returns all of it
as a dict.

``--icp ITERS`` (default 0: off) adds a geometric last step: every mask source is scored a second time on the same view seeds with the
refined pose fitted to the item's own cloud by ``ITERS`` steps of point-to-plane ICP against the model's triangles (``df_mesh_icp``,
DESIGN.md 12j).  ``--icp_max_dist FRAC`` drops points further from the surface than that fraction of the model cloud's diameter,
``--icp_cull`` keeps only faces that look at the camera, ``--icp_accel`` finds the closest triangles through the models' bounding-box
tree (``df_mesh_icp_tree``: the same poses byte for byte).  The second result is the entry ``<source>_icp`` with its own log
``eval_result_logs_<source>_icp.txt``, which also counts the items ICP left alone (too few inliers, degenerate geometry) and gives the
mean point-to-surface rms before and after.  Without ``--icp`` nothing changes by a byte.
``--verify`` scores every pose against the depth frame it came from by drawing the model at the pose (``df_pose_verify``):
each entry's log gains the mean visible-surface IoU of its passes and of its misses, and with ``--icp`` a third entry
``<source>_icp_best`` takes, per item, the ICP pose where its IoU is strictly higher and the refiner's otherwise, and says how many items
took each.  ``--verify_tol`` is the agreement tolerance in depth codes, ``--verify_margin`` how far the window reaches beyond the item's
crop box.  Without ``--verify`` nothing changes by a byte.
``--bop`` also scores every entry by the three BOP pose errors: the symmetry-aware MSSD and MSPD (``df_pose_sym_error``)
over ALL vertices of the model's mesh and the whole symmetry set of the models ``--cad_sym auto`` finds symmetric (``--bop_step``: the
discretisation of a surface of revolution), against the true pose of the view.  Each entry's log gains, per object and over all served
views, the recall of MSSD below 0.05 .. 0.5 x the mesh's diameter (the largest vertex-to-vertex distance, exact, over the vertices
of the convex hull, once per run)
and of MSPD below 5 r .. 50 r pixels, r = width / 640, their mean AR, each model's symmetry set size and which models
were taken as surfaces of revolution; ``main``'s dict gains ``bop``
per entry.  VSD, the visible surface discrepancy (``df_pose_vsd``), draws both poses into the window of the item's crop box grown by
``--verify_margin`` and compares them with the depth frame the item came from: ``--bop_delta`` x the diameter is its visibility tolerance,
tau runs over 0.05 .. 0.5 x the diameter, and the log gives the recall of VSD below 0.05 .. 0.5 averaged over the tau.  The mean AR is over
the three errors.  Without ``--bop`` nothing changes by a byte.
``--dense K`` (default 0: off) adds the dense, projective ICP step (``df_pose_refine_dense``): every mask source is scored
once more as ``<source>_dense``, the refiner's pose taking K steps against the whole depth window of the item's crop box grown by
``--verify_margin`` (the model is drawn at the pose, every drawn node is matched with the depth observed there), and with ``--icp`` also
as ``<source>_icp_dense``: the ICP pose, then the dense steps.  ``--dense_gate`` is the largest difference in depth codes between a drawn
and an observed node that still takes part, ``--dense_mask`` lets only the nodes of the item's mask take part.  The new entries compose
with ``--verify`` and ``--bop`` like the others; each logs the items the step left alone and the mean point-to-plane rms before and
after.  Without ``--dense`` nothing changes by a byte.
``--contour K`` (default 0: off) adds the dense ICP with an outline term (``df_pose_refine_contour``), which holds the views
of one or two faces that ``--dense`` hands back as degenerate: every mask source is scored once more as ``<source>_contour`` and, with
``--icp``, as ``<source>_icp_contour``, K steps in the window ``--dense`` uses.  ``--contour_scale`` weighs an outline residual against a
plane residual, ``--contour_reach`` is the farthest outline node (in nodes) a drawn-outline node pairs with, ``--contour_edge_step`` the depth
step (codes) between neighbours that counts as an outline (65535: only the border of what was observed or drawn), ``--contour_gate`` the
plane term's gate and ``--contour_mask`` lets only the nodes of the item's mask take part (and bound the observed outline).  The entries
compose with ``--verify`` and ``--bop``; each log says how many items were left alone, the mean rms and the mean outline pairs first ->
last.  ``--ppf_contour`` makes the ``--ppf`` chain's cluster steps use this call, with ``--ppf_dense`` steps and ``--ppf_dense_gate``.
Without these flags nothing changes by a byte.
``--ppf K`` (default 0: off) adds the pose search that needs no network (``df_pose_ppf``): every mask source is scored once
more as ``<source>_ppf``.  Per item the K best clusters of point-pair-feature votes are taken from the nodes of the item's mask in the
window of its crop box grown by ``--verify_margin`` (``--ppf_points`` samples a model, every ``--ppf_step``-th node, every
``--ppf_ref_step``-th of those a reference, normals from neighbours within ``--ppf_gate`` codes), each takes ``--ppf_dense`` steps of the
dense ICP (gate ``--ppf_dense_gate``) in one call of B x K items, each is scored by the verifier, and the one with the highest
visible-surface IoU goes on (ties to the lower rank); the pose networks' estimate is not used.  The entry composes with ``--verify`` and
``--bop``; its log says how many items had no hypothesis and how often each rank was kept.  Without ``--ppf`` nothing changes by a byte.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from densefusion_amd.datasets.customCAD import render as cad_render  # noqa: E402
from densefusion_amd.datasets.customCAD import symmetry as cad_symmetry  # noqa: E402
from densefusion_amd.lib.network import PoseNet, PoseRefineNet  # noqa: E402
from eval_cad import NUM_OBJECTS, NUM_POINTS, cloud_diameter  # noqa: E402
from eval_linemod import evaluate  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cad_model", type=str, nargs="+", required=True, help="PLY mesh(es): model k is object k + 1 and SegNet's class k + 1")
    ap.add_argument("--cad_distractor", type=str, nargs="*", default=[], help="meshes that are drawn and can occlude; background for SegNet")
    ap.add_argument("--segnet", type=str, default="", help="SegNet checkpoint (tools/train_segnet.py --dataset cad_render); needed unless --masks truth")
    ap.add_argument("--model", type=str, default="trained_models/cad/pose_model_current.pth", help="PoseNet checkpoint")
    ap.add_argument("--refine_model", type=str, default="trained_models/cad/pose_refine_model_current.pth", help="PoseRefineNet checkpoint")
    ap.add_argument("--masks", type=str, default="both", choices=("truth", "segnet", "both"), help="whose masks the pose path reads")
    ap.add_argument("--cad_seed", type=int, default=0, help="seed of the first view")
    ap.add_argument("--cad_frames", type=int, default=200, help="views")
    ap.add_argument("--seg_height", type=int, default=None, help="SegNet's window height, a multiple of 32 (default: the largest inside the frame)")
    ap.add_argument("--seg_width", type=int, default=None, help="SegNet's window width, a multiple of 32 (default: the largest inside the frame)")
    ap.add_argument("--seg_blur", type=int, default=1, choices=(0, 1), help="1: the 3 x 3 binomial blur SegNet was trained behind")
    ap.add_argument("--output_result_dir", type=str, default="experiments/eval_result/cad_render")
    ap.add_argument("--iteration", type=int, default=4)
    ap.add_argument("--threshold_frac", type=float, default=0.1, help="a view passes when its ADD is below this fraction of the model cloud's diameter")
    ap.add_argument("--max_frames", type=int, default=0)
    ap.add_argument("--window", type=int, default=64, help="views per device call of the pose networks")
    ap.add_argument("--workers", type=int, default=2, help="threads that prepare chunks ahead of the device calls (0 = in the loop)")
    ap.add_argument("--feed", type=str, default="threads", choices=["threads"])
    ap.add_argument("--icp", type=int, default=0, help="steps of point-to-mesh ICP after the refiner (0 = off); scored as <source>_icp")
    ap.add_argument("--icp_max_dist", type=float, default=0.1, help="ICP drops points further from the surface than this fraction of the model cloud's diameter")
    ap.add_argument("--icp_cull", action="store_true", help="ICP fits only faces that look at the camera")
    ap.add_argument("--icp_accel", action="store_true", help="ICP finds the closest triangles through the models' bounding-box tree: the same poses, faster on large meshes")
    ap.add_argument("--verify", action="store_true", help="score every pose by render-and-compare against its depth frame; with --icp also <source>_icp_best")
    ap.add_argument("--verify_tol", type=int, default=4, help="depth codes within which rendered and observed depth agree: about three sigmas of "
                    "the sensor's noise in codes (--sensor_sigma) plus its quantum (--sensor_quant); 4 suits a clean render")
    ap.add_argument("--verify_margin", type=int, default=8, help="pixels the verification window reaches beyond the item's crop box")
    ap.add_argument("--bop", action="store_true", help="also score every entry by the BOP pose errors MSSD and MSPD over the whole mesh and symmetry set")
    ap.add_argument("--bop_delta", type=float, default=0.075, help="--bop: the visibility tolerance of VSD as a fraction of the mesh's diameter (the "
                    "user's parameter, not a measurement)")
    ap.add_argument("--bop_step", type=float, default=0.01, help="--bop: a surface of revolution counts as ceil(pi / step) rotations (the BOP toolkit's "
                    "0.01: 315); the user's parameter, not a measurement")
    ap.add_argument("--dense", type=int, default=0, help="steps of dense projective ICP against the depth window (0 = off); scored as <source>_dense "
                    "and, with --icp, <source>_icp_dense")
    ap.add_argument("--dense_gate", type=int, default=16, help="--dense: depth codes a drawn and an observed node may differ by and still take part")
    ap.add_argument("--dense_mask", action="store_true", help="--dense: only the nodes of the item's mask take part")
    ap.add_argument("--contour", type=int, default=0, help="steps of dense ICP with an outline term (0 = off); scored as <source>_contour and, with "
                    "--icp, <source>_icp_contour")
    ap.add_argument("--contour_scale", type=float, default=0.1, help="--contour, --ppf_contour: weight of an outline residual against a plane residual")
    ap.add_argument("--contour_reach", type=int, default=6, help="--contour, --ppf_contour: nodes to the farthest observed-outline node a drawn one pairs with")
    ap.add_argument("--contour_edge_step", type=int, default=65535, help="--contour, --ppf_contour: depth codes between neighbours above which the nearer is an outline node")
    ap.add_argument("--contour_gate", type=int, default=16, help="--contour: depth codes a drawn and an observed node may differ by and still take part")
    ap.add_argument("--contour_mask", action="store_true", help="--contour: only the nodes of the item's mask take part")
    ap.add_argument("--ppf_contour", action="store_true", help="--ppf: the cluster poses take their steps with the outline term")
    ap.add_argument("--ppf", type=int, default=0, help="clusters of point-pair-feature votes to refine and choose from (0 = off); scored as <source>_ppf")
    ap.add_argument("--ppf_points", type=int, default=400, help="--ppf: surface samples per model")
    ap.add_argument("--ppf_step", type=int, default=1, help="--ppf: every this many nodes of the window is a scene point")
    ap.add_argument("--ppf_ref_step", type=int, default=5, help="--ppf: every this many scene points, per row and column, is a reference")
    ap.add_argument("--ppf_gate", type=int, default=16, help="--ppf: depth codes a neighbour may differ by and still shape a node's normal")
    ap.add_argument("--ppf_dense", type=int, default=10, help="--ppf: dense ICP steps each cluster pose takes")
    ap.add_argument("--ppf_dense_gate", type=int, default=3000, help="--ppf: the gate of those steps, in depth codes")
    views = ap.add_argument_group("views", "the views and the renderer, under the names of tools/render_cad_dataset.py")
    cad_render.add_view_arguments(views)
    cad_symmetry.add_sym_arguments(views)
    return ap


def load_segnet(path, n_classes):
    from densefusion_amd.vanilla_segmentation.segnet import SegNet
    net = SegNet(label_nbr=n_classes).cuda()
    if path:
        net.load_state_dict(torch.load(path, map_location="cuda", weights_only=True))
    return net.eval()


def _rate(a, b):
    return float(a) / b if b else 0.0


class IcpStep:
    """``evaluate()``'s ``refine_pose`` from a dataset's ``mesh_icp()``; keeps every call's stats on the device until ``summary``."""

    def __init__(self, dataset, opt):
        self.icp, self.iters, self.cull, self.stats = dataset.mesh_icp(accel=bool(opt.icp_accel)), opt.icp, bool(opt.icp_cull), []
        self.max_dist = [opt.icp_max_dist * cloud_diameter(dataset.pt[obj] * 10 / 10000.) for obj in dataset.objlist]

    def __call__(self, pose, points, objs):
        obj = torch.tensor(objs, dtype=torch.int32).pin_memory().to(pose.device, non_blocking=True)
        pose, stats = self.icp.refine(points.reshape(len(objs), -1, 3), pose, obj, iters=self.iters, max_dist=self.max_dist, cull=self.cull)
        self.stats.append(stats)
        return pose

    def summary(self):
        st = torch.cat(self.stats).cpu().numpy() if self.stats else np.zeros((0, 6))
        mean = lambda a: float(a.mean()) if len(a) else 0.0
        return dict(items=len(st), few=int((st[:, 0] == 1).sum()), degenerate=int((st[:, 0] == 2).sum()), bad_object=int((st[:, 0] == 3).sum()),
                    mean_first_rms=mean(st[:, 2]), mean_last_rms=mean(st[:, 4]), mean_steps=mean(st[:, 5]))


class VerifyStep:
    """``evaluate()``'s ``select_pose`` from a dataset's ``pose_verifier()`` (the dataset keeps its frames): every candidate is scored
    against the item's own depth frame and mask in the window of its crop box grown by ``--verify_margin`` (one size per call: the
    largest).  ``choose``: of two candidates the second is taken where ``better`` says so; otherwise the last candidate goes on as it is.
    The scores stay on the device until ``summary``."""

    def __init__(self, dataset, opt, choose=False):
        self.dataset, self.ver, self.choose = dataset, dataset.pose_verifier(), bool(choose)
        self.tol, self.margin, self.cull = opt.verify_tol, opt.verify_margin, bool(dataset.cull)
        self.indices, self.scores, self.taken = [], [], []

    def __call__(self, indices, candidates, objs):
        from densefusion_amd.lib.pose_verify import better, vsiou
        infos = [self.dataset.view_info(i) for i in indices]
        dev, B = candidates[0].device, len(indices)
        depth, mask = torch.stack([f["depth"] for f in infos]), torch.stack([f["mask"] for f in infos])
        window = (max(f["box"][1] - f["box"][0] for f in infos) + 2 * self.margin, max(f["box"][3] - f["box"][2] for f in infos) + 2 * self.margin)
        rec = torch.tensor([[k, objs[k], f["box"][0] - self.margin, f["box"][2] - self.margin] for k, f in enumerate(infos)],
                           dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        stats = [self.ver.score(depth, c.contiguous(), rec[:, 0], rec[:, 1], rec[:, 2:4], window, self.tol, mask=mask, cull=self.cull)
                 for c in (candidates if self.choose else candidates[-1:])]
        pose, score = candidates[-1], vsiou(stats[-1])
        take = torch.ones(B, dtype=torch.bool, device=dev)
        if self.choose and len(candidates) == 2:
            take = better(stats[0], stats[1])
            pose, score = torch.where(take[:, None], candidates[1], candidates[0]), torch.where(take, score, vsiou(stats[0]))
        self.indices += list(indices)
        self.scores.append(score); self.taken.append(take)
        return pose

    def summary(self, passed):
        """``passed``: {dataset index: bool} of the scored items."""
        score = torch.cat(self.scores).cpu().numpy() if self.scores else np.zeros(0)
        taken = torch.cat(self.taken).cpu().numpy() if self.taken else np.zeros(0, dtype=bool)
        ok = np.array([bool(passed[i]) for i in self.indices], dtype=bool)
        mean = lambda a: float(a.mean()) if len(a) else 0.0
        return dict(items=len(score), passes=int(ok.sum()), mean_vsiou_pass=mean(score[ok]), mean_vsiou_miss=mean(score[~ok]),
                    took_last=int(taken.sum()), took_first=int((~taken).sum()), tol=self.tol, margin=self.margin)


class DenseStep:
    """``evaluate()``'s ``select_pose`` from a dataset's ``dense_refiner()`` (the dataset keeps its frames): the last candidate takes
    ``--dense`` steps of dense projective ICP against the item's own depth frame in the window of its crop box grown by
    ``--verify_margin`` (one size per call: the largest), and goes on to ``inner`` (a ``VerifyStep``) when there is one.  The stats stay on
    the device until ``summary``."""

    def __init__(self, dataset, opt, inner=None):
        self.dataset, self.ref, self.inner = dataset, dataset.dense_refiner(), inner
        self.iters, self.gate, self.use_mask, self.margin, self.cull = opt.dense, opt.dense_gate, bool(opt.dense_mask), opt.verify_margin, bool(dataset.cull)
        self.more = {}                                              # what a ``ContourStep`` adds to the call
        self.stats = []

    def __call__(self, indices, candidates, objs):
        infos = [self.dataset.view_info(i) for i in indices]
        dev = candidates[-1].device
        depth = torch.stack([f["depth"] for f in infos])
        mask = torch.stack([f["mask"] for f in infos]) if self.use_mask else None
        window = (max(f["box"][1] - f["box"][0] for f in infos) + 2 * self.margin, max(f["box"][3] - f["box"][2] for f in infos) + 2 * self.margin)
        rec = torch.tensor([[k, objs[k], f["box"][0] - self.margin, f["box"][2] - self.margin] for k, f in enumerate(infos)],
                           dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        pose, stats = self.ref.refine(depth, candidates[-1].contiguous(), rec[:, 0], rec[:, 1], rec[:, 2:4], window, iters=self.iters,
                                      gate=self.gate, mask=mask, cull=self.cull, **self.more)
        self.stats.append(stats)
        return self.inner(indices, [pose], objs) if self.inner is not None else pose

    def summary(self):
        st = torch.cat(self.stats).cpu().numpy() if self.stats else np.zeros((0, 6))
        mean = lambda a: float(a.mean()) if len(a) else 0.0
        return dict(items=len(st), few=int((st[:, 0] == 1).sum()), degenerate=int((st[:, 0] == 2).sum()), bad_item=int((st[:, 0] == 3).sum()),
                    mean_first_rms=mean(st[:, 2]), mean_last_rms=mean(st[:, 4]), mean_steps=mean(st[:, 5]), gate=self.gate, margin=self.margin,
                    mask=self.use_mask)


class ContourStep(DenseStep):
    """``DenseStep`` from a dataset's ``contour_refiner()``: the ``--contour`` steps of the dense ICP with the outline term."""

    def __init__(self, dataset, opt, inner=None):
        self.dataset, self.ref, self.inner = dataset, dataset.contour_refiner(), inner
        self.iters, self.gate, self.use_mask, self.margin, self.cull = opt.contour, opt.contour_gate, bool(opt.contour_mask), opt.verify_margin, bool(dataset.cull)
        self.more = dict(edge_step=opt.contour_edge_step, reach=opt.contour_reach, contour_scale=opt.contour_scale)
        self.stats = []

    def summary(self):
        st = torch.cat(self.stats).cpu().numpy() if self.stats else np.zeros((0, 8))
        mean = lambda a: float(a.mean()) if len(a) else 0.0
        return dict(DenseStep.summary(self), mean_first_pairs=mean(st[:, 6]), mean_last_pairs=mean(st[:, 7]), **self.more)


class PpfStep:
    """``evaluate()``'s ``select_pose`` from a dataset's ``ppf_estimator()``, ``dense_refiner()`` and ``pose_verifier()`` (the dataset keeps
    its frames): the candidates of the pose networks are set aside; the ``--ppf`` best clusters of the votes cast by the nodes of the
    item's mask take ``--ppf_dense`` dense steps as one call of B x K items, are scored by the verifier, and per item the one with the
    highest visible-surface IoU goes on to ``inner`` (a ``VerifyStep``) when there is one.  Everything stays on the device until
    ``summary``."""

    def __init__(self, dataset, opt, inner=None):
        self.dataset, self.inner = dataset, inner
        self.est = dataset.ppf_estimator(points=opt.ppf_points)
        self.ref, self.ver = dataset.contour_refiner() if opt.ppf_contour else dataset.dense_refiner(), dataset.pose_verifier()
        self.more = dict(edge_step=opt.contour_edge_step, reach=opt.contour_reach, contour_scale=opt.contour_scale) if opt.ppf_contour else {}
        self.k, self.step, self.ref_step, self.gate = opt.ppf, opt.ppf_step, opt.ppf_ref_step, opt.ppf_gate
        self.iters, self.dense_gate, self.tol, self.margin, self.cull = opt.ppf_dense, opt.ppf_dense_gate, opt.verify_tol, opt.verify_margin, bool(dataset.cull)
        self.stats, self.kept = [], []

    def __call__(self, indices, candidates, objs):
        from densefusion_amd.lib.pose_verify import vsiou
        infos = [self.dataset.view_info(i) for i in indices]
        dev, B, K = candidates[-1].device, len(indices), self.k
        depth, mask = torch.stack([f["depth"] for f in infos]), torch.stack([f["mask"] for f in infos])
        window = (max(f["box"][1] - f["box"][0] for f in infos) + 2 * self.margin, max(f["box"][3] - f["box"][2] for f in infos) + 2 * self.margin)
        rec = torch.tensor([[k, objs[k], f["box"][0] - self.margin, f["box"][2] - self.margin] for k, f in enumerate(infos)],
                           dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
        pose, votes, stats = self.est.estimate(depth, rec[:, 0], rec[:, 1], rec[:, 2:4], window, step=self.step, gate=self.gate,
                                               ref_step=self.ref_step, k=K, mask=mask)
        each = rec.repeat_interleave(K, dim=0)
        refined, _ = self.ref.refine(depth, pose.reshape(B * K, 7), each[:, 0], each[:, 1], each[:, 2:4], window, iters=self.iters,
                                     gate=self.dense_gate, cull=self.cull, **self.more)
        score = vsiou(self.ver.score(depth, refined, each[:, 0], each[:, 1], each[:, 2:4], window, self.tol, mask=mask, cull=self.cull)).reshape(B, K)
        score = torch.where(votes[:, :, 0] > 0, score, torch.full_like(score, -1.0))      # a missing rank never wins
        kept = score.argmax(dim=1)                                   # the first of the largest: ties to the lower rank
        best = refined.reshape(B, K, 7)[torch.arange(B, device=dev), kept]
        # an item without a hypothesis has no pose to give: the networks' last candidate stands in, and the log counts it
        none = stats[:, 0] != 0
        best = torch.where(none[:, None], candidates[-1].to(best.dtype), best).to(candidates[-1].dtype).contiguous()
        self.stats.append(stats); self.kept.append(torch.where(none, torch.full_like(kept, -1), kept))
        return self.inner(indices, [best], objs) if self.inner is not None else best

    def summary(self):
        st = torch.cat(self.stats).cpu().numpy() if self.stats else np.zeros((0, 4))
        kept = torch.cat(self.kept).cpu().numpy() if self.kept else np.zeros(0, dtype=np.int64)
        mean = lambda a: float(a.mean()) if len(a) else 0.0
        return dict(items=len(st), k=self.k, no_hypothesis=int((st[:, 0] == 1).sum()), bad_item=int((st[:, 0] == 3).sum()),
                    kept_rank=[int((kept == r).sum()) for r in range(self.k)], mean_usable=mean(st[:, 1]), mean_hypotheses=mean(st[:, 2]),
                    mean_clusters=mean(st[:, 3]), points=self.est.models.points.shape[0] // self.est.models.n_objects, step=self.step,
                    ref_step=self.ref_step, gate=self.gate, dense=self.iters, dense_gate=self.dense_gate, margin=self.margin)


BOP_STEPS = [0.05 * k for k in range(1, 11)]                       # the ten BOP thresholds: x the diameter (MSSD), x 100 r pixels (MSPD)


def mesh_diameter(vertices, device):
    """The largest vertex-to-vertex distance of ``vertices`` [V,3] (host array), exact: the two vertices that attain it are vertices of
    the convex hull (``scipy.spatial.ConvexHull`` on the host; a flat or otherwise degenerate mesh keeps all its vertices), and every
    pair of those is taken in fp64 by a plain device reduction."""
    from scipy.spatial import ConvexHull, QhullError
    v = np.unique(np.asarray(vertices, dtype=np.float64).reshape(-1, 3), axis=0)
    try:
        v = v[ConvexHull(v).vertices]
    except (QhullError, ValueError):
        pass
    v = torch.from_numpy(np.ascontiguousarray(v)).to(device)
    best = torch.zeros((), dtype=torch.float64, device=v.device)
    rows = max(1, (1 << 22) // len(v))
    for a in range(0, len(v), rows):
        d = v[a:a + rows, None, :] - v[None, :, :]
        best = torch.maximum(best, ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).max())
    return float(best.sqrt())


def true_pose(dataset, index):
    """[7] (q wxyz, t in the units of the clouds): the pose ``df_cad_targets`` builds item ``index``'s target from"""
    from densefusion_amd.lib.transformations import quaternion_from_matrix
    info = dataset.view_info(index)
    M = np.eye(4)
    M[:3, :3] = np.asarray(info["pose"], dtype=np.float64)[:, :3]
    t = np.asarray(info["pose"], dtype=np.float64)[:, 3] / 10000.0
    if dataset.add_noise:
        t = t + np.asarray(info["add_t"], dtype=np.float64)
    return np.concatenate([quaternion_from_matrix(M), t])


class BopScorer:
    """What ``--bop`` needs of a dataset, built once in ``main`` and shared by the entries: its ``pose_errors()`` (one upload of the scaled
    vertices and the symmetry sets), each mesh's diameter, the set sizes and which models were taken as surfaces of revolution."""

    def __init__(self, dataset, opt):
        self.errors = dataset.pose_errors(step=opt.bop_step)
        vb, scaled = self.errors.vertex_begin, self.errors.vertices.cpu().numpy()
        self.diameter = [mesh_diameter(scaled[vb[k]:vb[k + 1]], self.errors.device) for k in range(self.errors.n_objects)]
        self.set_sizes = [int(n) for n in np.diff(self.errors.sym_begin)]
        self.revolution = [k for k in dataset.get_sym_list() if k in dataset.symmetry and cad_symmetry.is_revolution(dataset.symmetry[k])]
        self.pixel = dataset.image_dims[1] / 640.0
        # VSD works in the renderer's camera units (cloud units x 10000): delta and the ten tau per object, the crop margin of --verify
        cam = [d * 10000.0 for d in self.diameter]
        self.delta, self.tau = np.array([opt.bop_delta * d for d in cam]), np.array([[f * d for f in BOP_STEPS] for d in cam])
        self.margin, self.cull = opt.verify_margin, bool(dataset.cull)


class BopStep:
    """``evaluate()``'s ``select_pose`` of one scored entry, from the dataset's ``BopScorer``: the pose that goes on (``inner``'s choice when
    a ``VerifyStep`` is composed in, otherwise the last candidate) is scored against the view's true pose; the rows stay on the device
    until ``summary``."""

    def __init__(self, dataset, scorer, inner=None):
        self.dataset, self.inner, self.errors = dataset, inner, scorer.errors
        self.diameter, self.set_sizes, self.revolution, self.pixel = scorer.diameter, scorer.set_sizes, scorer.revolution, scorer.pixel
        self.scorer, self.rows, self.objs, self.vsd = scorer, [], [], []

    def __call__(self, indices, candidates, objs):
        pose = self.inner(indices, candidates, objs) if self.inner is not None else candidates[-1]
        gt = torch.from_numpy(np.stack([true_pose(self.dataset, i) for i in indices])).pin_memory().to(pose.device, non_blocking=True)
        obj = torch.tensor(objs, dtype=torch.int32).pin_memory().to(pose.device, non_blocking=True)
        self.rows.append(self.errors.sym_error(pose.contiguous(), gt, obj))
        # VSD against the frame the item was cut from, in the window of its crop box grown by the margin (one size per call: the largest)
        infos, m = [self.dataset.view_info(i) for i in indices], self.scorer.margin
        depth = torch.stack([f["depth"] for f in infos])
        window = (max(f["box"][1] - f["box"][0] for f in infos) + 2 * m, max(f["box"][3] - f["box"][2] for f in infos) + 2 * m)
        rec = torch.tensor([[k, objs[k], f["box"][0] - m, f["box"][2] - m] for k, f in enumerate(infos)], dtype=torch.int32).pin_memory().to(
            pose.device, non_blocking=True)
        self.vsd.append(self.errors.vsd(depth, pose.contiguous(), gt, rec[:, 0], rec[:, 1], rec[:, 2:4], window, self.scorer.delta, self.scorer.tau,
                                        cull=self.scorer.cull))
        self.objs += list(objs)
        return pose

    def summary(self):
        rows = torch.cat(self.rows).cpu().numpy() if self.rows else np.zeros((0, 6))       # the one read-back of the entry
        from densefusion_amd.lib.pose_error import vsd_values
        vsd = vsd_values(torch.cat(self.vsd).cpu().numpy()) if self.vsd else np.zeros((0, len(BOP_STEPS)))      # [items, tau], with the rows' read-back
        objs = np.array(self.objs, dtype=np.int64)
        ok = rows[:, 0] == 0

        def recalls(pick):
            n = int(pick.sum())
            thr = np.array([self.diameter[k] for k in objs[pick]])
            mssd = [float(((rows[pick, 1] < f * thr) & ok[pick]).mean()) if n else 0.0 for f in BOP_STEPS]
            mspd = [float(((rows[pick, 3] < f * 100.0 * self.pixel) & ok[pick]).mean()) if n else 0.0 for f in BOP_STEPS]
            # VSD: per threshold theta the recall of vsd < theta, averaged over the ten tau
            vsd_r = [float((vsd[pick] < f).mean()) if n else 0.0 for f in BOP_STEPS]
            ar_s, ar_p, ar_v = float(np.mean(mssd)), float(np.mean(mspd)), float(np.mean(vsd_r))
            return dict(items=n, mssd_recall=mssd, mspd_recall=mspd, vsd_recall=vsd_r, ar_mssd=ar_s, ar_mspd=ar_p, ar_vsd=ar_v,
                        ar=(ar_v + ar_s + ar_p) / 3.0)
        return dict(items=len(rows), bad_items=int((~ok).sum()), set_sizes=self.set_sizes, revolution=self.revolution, diameter=self.diameter, pixel=self.pixel,
                    objects=[recalls(objs == k) for k in range(self.errors.n_objects)], all=recalls(np.ones(len(rows), dtype=bool)))


class _PassLog:
    """The log file of ``evaluate()`` with an ear: ``passed[i]`` of every "No.i Pass!" / "No.i NOT Pass! Distance" line that goes by."""

    def __init__(self, fw):
        self.fw, self.passed = fw, {}

    def write(self, text):
        head = text.split(" ", 1)
        if head[0].startswith("No.") and "Lost detection" not in text:
            self.passed[int(head[0][3:])] = head[1].startswith("Pass!")
        return self.fw.write(text)


def run_source(source, dataset, estimator, refiner, diameter, opt, icp=None, verify=None, bop=None, dense=False, ppf=False, contour=False):
    """``evaluate()`` over ``dataset`` and the tallies of one mask source; with ``icp`` (an ``IcpStep``) the poses take that last step,
    with ``verify`` (a ``VerifyStep``) they are scored, or chosen, by render-and-compare; with ``bop`` the pose that is scored is also
    scored by the BOP pose errors (``bop``: the dataset's ``BopScorer``; a ``BopStep`` of it goes around ``verify``); with ``dense`` the
    pose first takes the dense steps (a ``DenseStep`` between the two); with ``ppf`` the pose is the best refined cluster of the
    point-pair-feature votes (a ``PpfStep`` in that place); with ``contour`` it takes the steps with the outline term (a ``ContourStep``
    in that place)."""
    objlist = list(dataset.objlist)
    n = len(dataset) if opt.max_frames <= 0 else min(opt.max_frames, len(dataset))
    with open(os.path.join(opt.output_result_dir, "eval_result_logs_%s.txt" % source), "w") as fw:
        def say(m):
            print(m)
            fw.write(m + "\n")
        steps = dict(**({} if icp is None else {"refine_pose": icp}), **({} if verify is None else {"select_pose": verify}))
        if dense:
            steps["select_pose"] = dense = DenseStep(dataset, opt, inner=verify)
        if ppf:
            steps["select_pose"] = ppf = PpfStep(dataset, opt, inner=verify)
        if contour:
            steps["select_pose"] = contour = ContourStep(dataset, opt, inner=verify)
        if bop is not None:
            steps["select_pose"] = bop = BopStep(dataset, bop, inner=dense or ppf or contour or verify)
        log = fw if verify is None else _PassLog(fw)
        success, served = evaluate(dataset, estimator, refiner, diameter, opt, log, **steps)
        success, served = success[:len(objlist)], served[:len(objlist)]
        kept = [0] * len(objlist)
        for i in range(n):                                          # host records of chunks the loop has prepared (or prepares again)
            info = dataset.view_info(i)
            kept[objlist.index(info["object"])] += bool(info["kept"])
        out = dict(source=source, views=n, success=success, served=served, kept=kept,
                   success_served=[_rate(s, m) for s, m in zip(success, served)], success_kept=[_rate(s, k) for s, k in zip(success, kept)],
                   all_served=_rate(sum(success), sum(served)), all_kept=_rate(sum(success), sum(kept)))
        say("[{0} masks] views {1}, kept {2}, served {3}".format(source, n, sum(kept), sum(served)))
        for k, obj in enumerate(objlist):
            say("[{0} masks] Object {1} success rate: {2} of {3} served views, {4} of {5} kept views".format(
                source, obj, out["success_served"][k], served[k], out["success_kept"][k], kept[k]))
        say("[{0} masks] ALL success rate: {1} of served views, {2} of kept views".format(source, out["all_served"], out["all_kept"]))
        if icp is not None:
            out["icp"] = m = icp.summary()
            say("[{0} masks] ICP {1} steps: {2} items, {3} few inliers, {4} degenerate, mean rms {5:.6g} -> {6:.6g}".format(
                source, icp.iters, m["items"], m["few"], m["degenerate"], m["mean_first_rms"], m["mean_last_rms"]))
        if dense:
            out["dense"] = m = dense.summary()
            say("[{0} masks] dense {1} steps gate {2}{3}: {4} items, {5} few inliers, {6} degenerate, mean rms {7:.6g} -> {8:.6g}".format(
                source, dense.iters, m["gate"], " masked" if m["mask"] else "", m["items"], m["few"], m["degenerate"], m["mean_first_rms"],
                m["mean_last_rms"]))
        if contour:
            out["contour"] = m = contour.summary()
            say("[{0} masks] contour {1} steps gate {2}{3}, scale {4:g}, reach {5}, edge step {6}: {7} items, {8} few inliers, {9} degenerate "
                "left alone".format(source, contour.iters, m["gate"], " masked" if m["mask"] else "", m["contour_scale"], m["reach"], m["edge_step"],
                                    m["items"], m["few"], m["degenerate"]))
            say("[{0} masks] contour: mean rms {1:.6g} -> {2:.6g}, mean outline pairs {3:.1f} -> {4:.1f}".format(
                source, m["mean_first_rms"], m["mean_last_rms"], m["mean_first_pairs"], m["mean_last_pairs"]))
        if ppf:
            out["ppf"] = m = ppf.summary()
            say("[{0} masks] ppf top {1} of {2} points, step {3}, every {4}th a reference, gate {5}, {6} dense steps gate {7}: {8} items, {9} without "
                "a hypothesis, kept rank {10}".format(source, m["k"], m["points"], m["step"], m["ref_step"], m["gate"], m["dense"], m["dense_gate"],
                                                      m["items"], m["no_hypothesis"], " ".join("%d: %d" % (r, n) for r, n in enumerate(m["kept_rank"]))))
            say("[{0} masks] ppf: mean usable nodes {1:.1f}, hypotheses {2:.1f}, clusters {3:.1f} an item".format(
                source, m["mean_usable"], m["mean_hypotheses"], m["mean_clusters"]))
            if ppf.more:                                            # --ppf_contour
                m["contour"] = dict(ppf.more)
                say("[{0} masks] ppf: the cluster steps carry the outline term, scale {1:g}, reach {2}, edge step {3}".format(
                    source, ppf.more["contour_scale"], ppf.more["reach"], ppf.more["edge_step"]))
        if verify is not None:
            out["verify"] = m = verify.summary(log.passed)
            say("[{0} masks] verify tol {1} margin {2}: mean vsiou {3:.6f} over {4} passes, {5:.6f} over {6} misses".format(
                source, m["tol"], m["margin"], m["mean_vsiou_pass"], m["passes"], m["mean_vsiou_miss"], m["items"] - m["passes"]))
            if verify.choose:
                say("[{0} masks] verify: {1} items took the ICP pose, {2} kept the refiner's".format(source, m["took_last"], m["took_first"]))
        if bop is not None:
            out["bop"] = m = bop.summary()
            say("[{0} masks] bop: symmetry set sizes {1}, mesh diameters {2}, {3} items".format(
                source, m["set_sizes"], ["%.6g" % d for d in m["diameter"]], m["items"]))
            say("[{0} masks] bop: models taken as surfaces of revolution (discretised to ceil(pi / {1:g}) rotations): {2}".format(
                source, opt.bop_step, m["revolution"]))
            for name, r in [("Object %d" % obj, m["objects"][k]) for k, obj in enumerate(objlist)] + [("ALL", m["all"])]:
                say("[{0} masks] bop: {1} over {2} served views: MSSD recall at 0.05 .. 0.5 x diameter {3}".format(
                    source, name, r["items"], " ".join("%.4f" % x for x in r["mssd_recall"])))
                say("[{0} masks] bop: {1} over {2} served views: MSPD recall at {3:g} .. {4:g} px {5}".format(
                    source, name, r["items"], 5 * m["pixel"], 50 * m["pixel"], " ".join("%.4f" % x for x in r["mspd_recall"])))
                say("[{0} masks] bop: {1} over {2} served views: VSD recall below 0.05 .. 0.5 (over tau 0.05 .. 0.5 x diameter, delta {3:g} x) {4}".format(
                    source, name, r["items"], opt.bop_delta, " ".join("%.4f" % x for x in r["vsd_recall"])))
                say("[{0} masks] bop: {1} AR_VSD {2:.6f} AR_MSSD {3:.6f} AR_MSPD {4:.6f} mean AR {5:.6f}".format(
                    source, name, r["ar_vsd"], r["ar_mssd"], r["ar_mspd"], r["ar"]))
        if source == "segnet":
            m = dataset.seg_score.summary()
            out["seg"] = m
            names = ["background"] + ["object %d" % o for o in objlist]
            for c, name in enumerate(names):
                say("[segnet masks] {0}: IoU {1:.4f} precision {2:.4f} recall {3:.4f}".format(name, m["iou"][c], m["precision"][c], m["recall"][c]))
            say("[segnet masks] mIoU {0:.4f} pixel accuracy {1:.4f} over {2} pixels".format(m["miou"], m["pixel_accuracy"], m["pixels"]))
    return out


def main(argv=None):
    opt = build_parser().parse_args(argv)
    if len(opt.cad_model) > NUM_OBJECTS:
        raise SystemExit("at most %d models: the pose networks of tools/eval_cad.py have that many objects" % NUM_OBJECTS)
    if not 0 <= opt.icp <= 64 or not opt.icp_max_dist > 0:
        raise SystemExit("--icp takes 0..64 steps and --icp_max_dist a positive fraction")
    if not opt.bop_step > 0 or not (opt.bop_delta >= 0 and opt.bop_delta < float("inf")):
        raise SystemExit("--bop_step takes a positive angle step and --bop_delta a finite fraction >= 0")
    if not 0 <= opt.verify_tol <= 65535 or not 0 <= opt.verify_margin <= 4096:
        raise SystemExit("--verify_tol takes 0..65535 codes and --verify_margin 0..4096 pixels")
    if not 0 <= opt.dense <= 64 or not 0 <= opt.dense_gate <= 65535:
        raise SystemExit("--dense takes 0..64 steps and --dense_gate 0..65535 codes")
    if (not 0 <= opt.ppf <= 16 or not 2 <= opt.ppf_points <= 1024 or not 1 <= opt.ppf_step <= 64 or not 1 <= opt.ppf_ref_step <= 64
            or not 0 <= opt.ppf_gate <= 65535 or not 0 <= opt.ppf_dense <= 64 or not 0 <= opt.ppf_dense_gate <= 65535):
        raise SystemExit("--ppf takes 0..16 clusters, --ppf_points 2..1024, --ppf_step and --ppf_ref_step 1..64, --ppf_gate and --ppf_dense_gate "
                         "0..65535 codes and --ppf_dense 0..64 steps")
    if (not 0 <= opt.contour <= 64 or not 0 <= opt.contour_gate <= 65535 or not 0 <= opt.contour_edge_step <= 65535 or not 0 <= opt.contour_reach <= 64
            or not (opt.contour_scale >= 0 and opt.contour_scale < float("inf"))):
        raise SystemExit("--contour takes 0..64 steps, --contour_gate and --contour_edge_step 0..65535 codes, --contour_reach 0..64 nodes and "
                         "--contour_scale a finite weight >= 0")
    if opt.ppf_contour and not opt.ppf > 0:
        raise SystemExit("--ppf_contour needs --ppf")
    if not torch.cuda.is_available():
        raise SystemExit("eval_cad_render.py needs a GPU (densefusion_amd has no CPU path)")
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    estimator = PoseNet(num_points=NUM_POINTS, num_obj=NUM_OBJECTS).cuda()
    refiner = PoseRefineNet(num_points=NUM_POINTS, num_obj=NUM_OBJECTS).cuda()
    estimator.load_state_dict(torch.load(opt.model, map_location="cuda", weights_only=True))
    refiner.load_state_dict(torch.load(opt.refine_model, map_location="cuda", weights_only=True))
    estimator.eval(); refiner.eval()
    sources = ("truth", "segnet") if opt.masks == "both" else (opt.masks,)
    segnet = load_segnet(opt.segnet, len(opt.cad_model) + 1) if "segnet" in sources else None
    if segnet is not None and not opt.segnet:
        print("no --segnet checkpoint: SegNet runs on its initial weights")
    window = None if opt.seg_height is None and opt.seg_width is None else \
        (opt.seg_height or opt.height // 32 * 32, opt.seg_width or opt.width // 32 * 32)
    os.makedirs(opt.output_result_dir, exist_ok=True)
    result = {}
    for source in sources:
        np.random.seed(opt.cad_seed)                                # the model points of ``pt`` are drawn with np.random: the same for both
        kw = dict(segnet=segnet, seg_window=window, seg_blur=opt.seg_blur) if source == "segnet" else {}
        try:
            # SegNet's masks need the scene renderer's label plane; the truth run of the same call renders the same scenes
            dataset = RenderedPoseDataset.from_options(opt, opt.cad_model, opt.cad_distractor, first_seed=opt.cad_seed, frames=opt.cad_frames,
                                                       num=NUM_POINTS, scene=True if segnet is not None else None, **kw,
                                                       **({"keep_frames": True} if opt.verify or opt.bop or opt.dense or opt.ppf or opt.contour else {}))
        except ValueError as e:
            raise SystemExit(f"eval_cad_render.py: {e}")

        def verifier(choose=False):
            """a fresh ``VerifyStep`` for one scored entry; None without --verify"""
            return VerifyStep(dataset, opt, choose) if opt.verify else None
        try:
            first = verifier()
        except ValueError as e:
            raise SystemExit(f"eval_cad_render.py: --verify: {e}")
        # the loader's clouds are in units of 10000 (model * 10 / 10000): so is the threshold (tools/eval_cad.py)
        diameter = [opt.threshold_frac * cloud_diameter(dataset.pt[obj] * 10 / 10000.) for obj in dataset.objlist]
        diameter += [0.0] * (NUM_OBJECTS - len(diameter))
        print("symmetry object list: %s" % dataset.get_sym_list())
        scorer = None
        if opt.bop:                                                 # once per dataset: every entry of this source shares it
            try:
                scorer = BopScorer(dataset, opt)
            except ValueError as e:
                raise SystemExit(f"eval_cad_render.py: --bop: {e}")
        result[source] = run_source(source, dataset, estimator, refiner, diameter, opt, verify=first, bop=scorer)
        result[source]["sym_list"] = dataset.get_sym_list()
        if opt.icp > 0:                                             # the same views (the dataset serves them again), one more step per pose
            try:
                step = IcpStep(dataset, opt)
            except ValueError as e:
                raise SystemExit(f"eval_cad_render.py: --icp: {e}")
            result[source + "_icp"] = run_source(source + "_icp", dataset, estimator, refiner, diameter, opt, icp=step, verify=verifier(), bop=scorer)
            result[source + "_icp"]["sym_list"] = dataset.get_sym_list()
            if opt.verify:                                          # per item the pose with the higher visible-surface IoU
                name = source + "_icp_best"
                result[name] = run_source(name, dataset, estimator, refiner, diameter, opt, icp=IcpStep(dataset, opt), verify=verifier(True), bop=scorer)
                result[name]["sym_list"] = dataset.get_sym_list()
        if opt.dense > 0:                                           # the same views once more: the dense steps after the refiner, and after ICP
            for name, icp in [(source + "_dense", None)] + ([(source + "_icp_dense", True)] if opt.icp > 0 else []):
                try:
                    result[name] = run_source(name, dataset, estimator, refiner, diameter, opt, icp=IcpStep(dataset, opt) if icp else None,
                                              verify=verifier(), bop=scorer, dense=True)
                except ValueError as e:
                    raise SystemExit(f"eval_cad_render.py: --dense: {e}")
                result[name]["sym_list"] = dataset.get_sym_list()
        if opt.contour > 0:                                         # the same views once more: the dense steps with the outline term
            for name, icp in [(source + "_contour", None)] + ([(source + "_icp_contour", True)] if opt.icp > 0 else []):
                try:
                    result[name] = run_source(name, dataset, estimator, refiner, diameter, opt, icp=IcpStep(dataset, opt) if icp else None,
                                              verify=verifier(), bop=scorer, contour=True)
                except ValueError as e:
                    raise SystemExit(f"eval_cad_render.py: --contour: {e}")
                result[name]["sym_list"] = dataset.get_sym_list()
        if opt.ppf > 0:                                             # the same views once more: the pose found from depth alone
            name = source + "_ppf"
            try:
                result[name] = run_source(name, dataset, estimator, refiner, diameter, opt, verify=verifier(), bop=scorer, ppf=True)
            except ValueError as e:
                raise SystemExit(f"eval_cad_render.py: --ppf: {e}")
            result[name]["sym_list"] = dataset.get_sym_list()
    return result


if __name__ == "__main__":
    main()
