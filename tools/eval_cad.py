#!/usr/bin/env python
"""customCAD evaluation driver -- the job the reference's tools/eval_cad.py stops short of (it leaves its loop after three frames and
then fails on an undefined name), on the HIP path.

    python tools/eval_cad.py --dataset_root <dataset_processed> --model <pose_model.pth> --refine_model <pose_refine_model.pth>

For every 'test' frame: PoseNet -> arg-max pose -> ``iteration`` (4, eval_cad.py:33) refine steps in one device call, then ADD on the
device against ``--threshold_frac`` (0.1) x the diameter of the object's model cloud -- the largest pairwise distance of the loaded model
points, found on the host; the reference has no ``models_info.yml`` for this set (eval_cad.py:56-61 is commented out).  The loop is
``evaluate()`` of tools/eval_linemod.py (``--window`` frames per device call; the per-frame results do not depend on the window); the log
``eval_result_logs.txt`` has the reference's line format (eval_cad.py:71-72,143-147).

``--dump_ply N`` writes the predicted and the target model cloud of the first N frames as ``pred_pcld_NNNN.ply`` / ``target_pcld_NNNN.ply``
(binary little-endian, double x y z: what eval_cad.py:122-136 writes through open3d) into the result directory.
"""
from __future__ import annotations

import argparse
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from densefusion_amd.lib.network import PoseNet, PoseRefineNet  # noqa: E402
from eval_linemod import evaluate  # noqa: E402

NUM_OBJECTS = 5                     # eval_cad.py:31-33
NUM_POINTS = 500


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset_root", type=str, default="datasets/customCAD/dataset_processed", help="dataset root dir")
    ap.add_argument("--model", type=str, default="trained_models/cad/pose_model_current.pth", help="resume PoseNet model")
    ap.add_argument("--refine_model", type=str, default="trained_models/cad/pose_refine_model_current.pth", help="resume PoseRefineNet model")
    ap.add_argument("--output_result_dir", type=str, default="experiments/eval_result/cad")
    ap.add_argument("--objlist", type=str, default="1", help="comma-separated object directories (data/XX); the reference reads 1")
    ap.add_argument("--iteration", type=int, default=4)
    ap.add_argument("--threshold_frac", type=float, default=0.1, help="a frame passes when its ADD is below this fraction of the model cloud's diameter")
    ap.add_argument("--dump_ply", type=int, default=0, help="write pred / target clouds of the first N frames as PLY files")
    ap.add_argument("--max_frames", type=int, default=0)
    ap.add_argument("--window", type=int, default=64, help="test frames per device call (1 = frame by frame, like the reference)")
    ap.add_argument("--workers", type=int, default=8, help="frames are fetched ahead of the device calls by this many workers (0 = fetch in the loop)")
    ap.add_argument("--feed", type=str, default="threads", choices=["processes", "threads"])
    ap.add_argument("--seed", type=int, default=0, help="seed of the pixel-subset rule, of np.random (the loader's 3000 model points) and of random (its 500 "
                                                        "out of them per frame); the run repeats exactly with --workers 0, where frames are fetched in order")
    return ap


def cloud_diameter(points, block=1024):
    """Largest pairwise distance of points [n,3] (host, float64), in blocks of rows."""
    p = np.asarray(points, dtype=np.float64)
    best = 0.0
    for i in range(0, len(p), block):
        d = p[i:i + block, None, :] - p[None, :, :]
        best = max(best, float(np.sqrt((d * d).sum(-1).max())))
    return best


def write_ply(path, points):
    """Binary little-endian PLY of double x y z vertices (open3d's write_point_cloud layout, eval_cad.py:130-136)."""
    pts = np.ascontiguousarray(points, dtype="<f8").reshape(-1, 3)
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\ncomment Created by densefusion_amd\nelement vertex %d\nproperty double x\n"
                 "property double y\nproperty double z\nend_header\n" % len(pts)).encode("ascii"))
        f.write(pts.tobytes())


def cloud_dumper(out_dir, n):
    """``on_pose`` callback of ``evaluate``: for frames below n, pred = model_points @ R^T + t of the refined pose and the loader's target, the
    very clouds the logged distance is the mean distance of (eval_cad.py:122-136)."""
    from densefusion_amd.lib.transformations import quaternion_matrix

    def on_pose(i, pose, model_points, target):
        if i >= n:
            return
        pose = pose.double().cpu().numpy()
        pred = model_points.double().cpu().numpy() @ quaternion_matrix(pose[:4])[:3, :3].T + pose[4:7]
        write_ply(os.path.join(out_dir, "pred_pcld_%04d.ply" % i), pred)
        write_ply(os.path.join(out_dir, "target_pcld_%04d.ply" % i), target.double().cpu().numpy())
    return on_pose


def main(argv=None, testdataset=None):
    opt = build_parser().parse_args(argv)
    estimator = PoseNet(num_points=NUM_POINTS, num_obj=NUM_OBJECTS).cuda()
    refiner = PoseRefineNet(num_points=NUM_POINTS, num_obj=NUM_OBJECTS).cuda()
    estimator.load_state_dict(torch.load(opt.model, map_location="cuda", weights_only=True))
    refiner.load_state_dict(torch.load(opt.refine_model, map_location="cuda", weights_only=True))
    estimator.eval(); refiner.eval()
    if testdataset is None:
        from densefusion_amd.datasets.customCAD.dataset import PoseDataset as PoseDataset_cad
        np.random.seed(opt.seed)
        random.seed(opt.seed)
        testdataset = PoseDataset_cad("test", NUM_POINTS, False, opt.dataset_root, 0.0, False, seed=opt.seed,
                                      objlist=tuple(int(v) for v in opt.objlist.split(",")))
    objlist = list(testdataset.objlist)
    print("loaded dataset", len(testdataset))
    # the loader's clouds are in units of 10000 (model * 10 / 10000, dataset.py:168,209): so is the threshold
    diameter = [opt.threshold_frac * cloud_diameter(testdataset.pt[obj] * 10 / 10000.) for obj in objlist]
    diameter += [0.0] * (NUM_OBJECTS - len(diameter))
    print(diameter[:len(objlist)])
    os.makedirs(opt.output_result_dir, exist_ok=True)
    with open("{0}/eval_result_logs.txt".format(opt.output_result_dir), "w") as fw:
        success_count, num_count = evaluate(testdataset, estimator, refiner, diameter, opt, fw,
                                            on_pose=cloud_dumper(opt.output_result_dir, opt.dump_ply) if opt.dump_ply > 0 else None)
        for i in range(len(objlist)):
            if num_count[i]:
                m = "Object {0} success rate: {1}".format(objlist[i], float(success_count[i]) / num_count[i])
                print(m); fw.write(m + "\n")
        m = "ALL success rate: {0}".format(float(sum(success_count)) / max(1, sum(num_count)))
        print(m); fw.write(m + "\n")
    return success_count, num_count


if __name__ == "__main__":
    main()
