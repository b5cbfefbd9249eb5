#!/usr/bin/env python
"""YCB-Video accuracy numbers from the result ``.mat`` files of tools/eval_ycb.py -- the numeric job of the two MATLAB
scripts the reference drops into the YCB_Video_toolbox:

* ``replace_ycb_toolbox/evaluate_poses_keyframe.m`` (:36-131): for every keyframe and every ground-truth object instance,
  find the detection of the same class in the PoseCNN ``rois`` (:75), turn the estimated [q, t] row into [R|t] and take
  ``adi`` (ADD-S, gt -> est nearest neighbour, :177-193) and ``add`` (:160-175) over the object's ``points.xyz``, plus the
  rotation / translation errors; a missed detection counts as infinite distance (:107-111);
* ``replace_ycb_toolbox/plot_accuracy_keyframe.m`` (:29-53,150-170): per class and over all instances, the accuracy-vs-
  threshold curve up to 0.1 m, its area (``VOCap``, x100 = the README's "AUC") and the < 2 cm rate.

The distances of ALL instances are computed by one batched device launch per class (``df_ycb_distances``, fp64, exact
like MATLAB's KDTreeSearcher); everything else is host bookkeeping.  Output: a table on stdout, ``results_keyframe.mat``
(same variables as the MATLAB script; columns 1 = refined, 3 = without refinement, the others inf) and
``accuracy.json``.

    python tools/eval_ycb_auc.py --dataset_root <YCB_Video_Dataset> --ycb_toolbox_dir <toolbox> \
        --result_refine_dir <...> --result_wo_refine_dir <...>

Expected files: ``<toolbox>/classes.txt``, ``<toolbox>/keyframe.txt`` (``0048/000001`` per line),
``<toolbox>/results_PoseCNN_RSS2018/%06d.mat`` (``rois``; with ``--rois_from_results`` the ``rois`` of the refined result
file instead, which tools/eval_ycb.py --segnet_model writes), ``<dataset_root>/models/<class>/points.xyz``,
``<dataset_root>/data/<seq>/<frame>-meta.mat`` (``cls_indexes``, ``poses`` [3,4,n]), result dirs with ``%04d.mat``
(``poses`` [n,7]).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import scipy.io as scio
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from densefusion_amd.lib import ycb_eval  # noqa: E402


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset_root", type=str, required=True)
    ap.add_argument("--ycb_toolbox_dir", type=str, default="YCB_Video_toolbox")
    ap.add_argument("--result_refine_dir", type=str, default="experiments/eval_result/ycb/Densefusion_iterative_result")
    ap.add_argument("--result_wo_refine_dir", type=str, default="experiments/eval_result/ycb/Densefusion_wo_refine_result")
    ap.add_argument("--output_dir", type=str, default="experiments/eval_result/ycb")
    ap.add_argument("--max_keyframes", type=int, default=0)
    ap.add_argument("--rois_from_results", action="store_true",
                    help="take each keyframe's detections from the `rois` of its refined result file (eval_ycb.py --segnet_model) "
                         "instead of PoseCNN's")
    return ap


def rotation_error_deg(R_est, R_gt):
    # evaluate_poses_keyframe.m:204-207 `re`: angle of R_est inv(R_gt), clamped cosine, degrees
    c = 0.5 * (np.trace(R_est @ np.linalg.inv(R_gt)) - 1.0)
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def collect(opt):
    """-> per-instance records: cls (1-based), seq, frame, object slot, [R|t] gt, [R|t] refined / without (or None)."""
    with open(os.path.join(opt.ycb_toolbox_dir, "keyframe.txt")) as f:
        keyframes = [ln.strip() for ln in f if ln.strip()]
    if opt.max_keyframes > 0:
        keyframes = keyframes[:opt.max_keyframes]
    recs = []
    for i, name in enumerate(keyframes):
        seq, frame = name.split("/")
        ref_mat = scio.loadmat(os.path.join(opt.result_refine_dir, "%04d.mat" % i))
        det = ref_mat if opt.rois_from_results else scio.loadmat(os.path.join(opt.ycb_toolbox_dir, "results_PoseCNN_RSS2018", "%06d.mat" % i))
        rois = np.asarray(det["rois"], dtype=np.float64).reshape(-1, det["rois"].shape[-1]) if det["rois"].size else np.zeros((0, 7))
        ref = ref_mat["poses"]
        wo = scio.loadmat(os.path.join(opt.result_wo_refine_dir, "%04d.mat" % i))["poses"]
        gt = scio.loadmat(os.path.join(opt.dataset_root, "data", seq, "%s-meta.mat" % frame))
        cls_indexes = np.asarray(gt["cls_indexes"]).reshape(-1)
        poses = np.asarray(gt["poses"], dtype=np.float64).reshape(3, 4, -1)
        for j, cls in enumerate(cls_indexes):
            hit = np.flatnonzero(rois[:, 1] == cls)
            rec = {"cls": int(cls), "seq": int(seq), "frame": int(frame), "slot": j + 1, "rt_gt": poses[:, :, j], "ref": None, "wo": None}
            if hit.size:                                       # `find(...)`: MATLAB then indexes with all hits; one per class in practice
                r = int(hit[0])
                if r < len(ref) and np.any(ref[r]):
                    rec["ref"] = ycb_eval.pose_to_rt(ref[r])
                if r < len(wo) and np.any(wo[r]):
                    rec["wo"] = ycb_eval.pose_to_rt(wo[r])
            recs.append(rec)
    return recs


def evaluate(opt, device="cuda"):
    with open(os.path.join(opt.ycb_toolbox_dir, "classes.txt")) as f:
        classes = [ln.strip() for ln in f if ln.strip()]
    models = [np.loadtxt(os.path.join(opt.dataset_root, "models", c, "points.xyz"), dtype=np.float64).reshape(-1, 3) for c in classes]
    recs = collect(opt)
    n = len(recs)
    dist_sys = np.full((n, 5), np.inf)
    dist_non = np.full((n, 5), np.inf)
    err_rot = np.full((n, 5), np.inf)
    err_tr = np.full((n, 5), np.inf)
    for col, key in ((0, "ref"), (2, "wo")):
        for k in range(len(classes)):                          # one batched launch per class (all its instances share the model)
            idx = [i for i, r in enumerate(recs) if r["cls"] == k + 1 and r[key] is not None]
            if not idx:
                continue
            est = torch.from_numpy(np.stack([recs[i][key] for i in idx])).to(device)
            gtp = torch.from_numpy(np.stack([recs[i]["rt_gt"] for i in idx])).to(device)
            pts = torch.from_numpy(models[k]).to(device)[None].expand(len(idx), -1, -1).contiguous()
            add, adi = ycb_eval.ycb_distances(est, gtp, pts)
            dist_non[idx, col] = add.cpu().numpy()
            dist_sys[idx, col] = adi.cpu().numpy()
            for i in idx:
                err_rot[i, col] = rotation_error_deg(recs[i][key][:, :3], recs[i]["rt_gt"][:, :3])
                err_tr[i, col] = float(np.linalg.norm(recs[i][key][:, 3] - recs[i]["rt_gt"][:, 3]))
    cls_ids = np.array([r["cls"] for r in recs])
    table = {}
    for k, name in enumerate(classes + ["All %d objects" % len(classes)]):
        sel = np.flatnonzero(cls_ids == k + 1) if k < len(classes) else np.arange(n)
        if sel.size == 0:
            continue
        row = {"instances": int(sel.size)}
        for col, tag in ((0, "iterative"), (2, "per-pixel")):
            auc_s, lt2_s = ycb_eval.auc_and_lt2cm(dist_sys[sel, col])
            auc_n, lt2_n = ycb_eval.auc_and_lt2cm(dist_non[sel, col])
            row[tag] = {"ADD-S_AUC": auc_s * 100, "ADD-S_lt2cm": lt2_s * 100, "ADD_AUC": auc_n * 100, "ADD_lt2cm": lt2_n * 100}
        table[name] = row
    os.makedirs(opt.output_dir, exist_ok=True)
    scio.savemat(os.path.join(opt.output_dir, "results_keyframe.mat"),
                 {"distances_sys": dist_sys, "distances_non": dist_non, "errors_rotation": err_rot, "errors_translation": err_tr,
                  "results_seq_id": np.array([r["seq"] for r in recs], dtype=np.float64)[:, None],
                  "results_frame_id": np.array([r["frame"] for r in recs], dtype=np.float64)[:, None],
                  "results_object_id": np.array([r["slot"] for r in recs], dtype=np.float64)[:, None],
                  "results_cls_id": cls_ids.astype(np.float64)[:, None]})
    with open(os.path.join(opt.output_dir, "accuracy.json"), "w") as f:
        json.dump(table, f, indent=1)
    return table, dist_sys, dist_non


def main(argv=None):
    opt = build_parser().parse_args(argv)
    table, _, _ = evaluate(opt)
    print("%-28s %5s | %s" % ("class", "n", "iterative: ADD-S AUC  <2cm   ADD AUC  <2cm | per-pixel: ADD-S AUC  <2cm   ADD AUC  <2cm"))
    for name, row in table.items():
        a, b = row["iterative"], row["per-pixel"]
        print("%-28s %5d | %20.2f %6.2f %9.2f %6.2f | %20.2f %6.2f %9.2f %6.2f" % (
            name, row["instances"], a["ADD-S_AUC"], a["ADD-S_lt2cm"], a["ADD_AUC"], a["ADD_lt2cm"],
            b["ADD-S_AUC"], b["ADD-S_lt2cm"], b["ADD_AUC"], b["ADD_lt2cm"]))
    return table


if __name__ == "__main__":
    main()
