"""CPU: the detection-row -> PoseCNN ROI helper of lib/segment.py against get_bbox of the half-open tight box, and the new
flags of tools/eval_ycb.py / tools/eval_ycb_auc.py (defaults leave both tools' behaviour unchanged)."""
import os
import sys

import numpy as np

from densefusion_amd.datasets.ycb import dataset as ycb_dataset
from densefusion_amd.lib import preprocess as pp
from densefusion_amd.lib.segment import det_row_to_roi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tight_boxes(label, num_obj):
    out = []
    for c in range(1, num_obj + 1):
        rr, cc = np.nonzero(label == c)
        if rr.size:
            out.append((c, rr.min(), rr.max() + 1, cc.min(), cc.max() + 1, rr.size))
    return out


def test_roi_helper_gives_get_bbox_of_the_half_open_box():
    rng = np.random.default_rng(2)
    seen_edge = False
    for it in range(40):
        label = np.zeros((480, 640), np.int32)
        for c in range(1, 8):
            h, w = int(rng.integers(1, 300)), int(rng.integers(1, 400))
            r0, c0 = int(rng.integers(-h // 2, 480 - h // 2)), int(rng.integers(-w // 2, 640 - w // 2))
            label[max(r0, 0):r0 + h, max(c0, 0):c0 + w][rng.random((min(r0 + h, 480) - max(r0, 0), min(c0 + w, 640) - max(c0, 0))) < 0.6] = c
        label[rng.random((480, 640)) < 1e-4] = 9
        for row in _tight_boxes(label, 9):
            _, rmin, rmax, cmin, cmax, _ = row
            seen_edge |= rmin == 0 or cmin == 0 or rmax == 480 or cmax == 640
            roi = det_row_to_roi(np.array(row, np.int32))
            assert roi.shape == (7,) and roi[0] == 0 and roi[1] == row[0] and roi[6] == 1.0
            # get_bbox reads the half-open tight box back (rmin + 1 / rmax - 1 undo the ROI's one-pixel margin) and snaps it
            # like the training loader's get_bbox of the mask itself (datasets/ycb/dataset.py:251-289)
            assert (int(roi[3]) + 1, int(roi[5]) - 1, int(roi[2]) + 1, int(roi[4]) - 1) == (rmin, rmax, cmin, cmax)
            assert pp.get_bbox(roi) == ycb_dataset.get_bbox(label == row[0])
    assert seen_edge


def test_new_tool_flags_parse_and_default_off():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eval_ycb
    import eval_ycb_auc
    opt = eval_ycb.build_parser().parse_args([])
    assert opt.segnet_model == "" and opt.min_pixels == 50
    opt = eval_ycb.build_parser().parse_args(["--segnet_model", "s.pth", "--min_pixels", "7"])
    assert opt.segnet_model == "s.pth" and opt.min_pixels == 7
    opt = eval_ycb_auc.build_parser().parse_args(["--dataset_root", "d"])
    assert opt.rois_from_results is False
    assert eval_ycb_auc.build_parser().parse_args(["--dataset_root", "d", "--rois_from_results"]).rois_from_results
