"""Poses from SegNet's own masks in one device pipeline: RGB-D window -> SegNet -> labels and detections -> DenseFusion.

``SegmentPoseEstimator`` is ``WindowEstimator`` (eval_window.py) with the PoseCNN detections replaced by ``segment.segment_frames``:

  * a window's colour and depth frames go up once into a ``WindowEstimator`` slot; the label kernel writes straight into the
    slot's label buffer, so the pose stage (``WindowEstimator.run``) reads masks that never leave the device;
  * the host receives only the window's detection table [F][C][6] and counts (one small copy) and waits for nothing else before
    it builds the detection list: rows -> PoseCNN-style ROIs (``segment.det_row_to_roi``), seeds ``seed + frame_id * 64 + idx``
    (tools/eval_ycb.py's rule), bucketed by snapped crop size across the window as before;
  * ``submit`` enqueues window i's upload and segmentation first and only then blocks on window i-1's table and enqueues its pose
    stage, so with ``depth >= 2`` the device has window i's SegNet to run while the host waits.

Per detection the poses are bit-identical to ``WindowEstimator.submit`` fed with the same label map and ROIs from the host.
"""
from __future__ import annotations

import numpy as np
import torch

from . import preprocess as pp
from .eval_window import WindowEstimator
from .segment import det_row_to_roi, segment_frames


class SegmentPoseEstimator:
    def __init__(self, segnet, estimator, refiner, num_points, iteration, max_frames, depth=2, min_pixels=50,
                 frame_hw=(pp.IMG_WIDTH, pp.IMG_LENGTH), cam=pp.YCB_CAM):
        if segnet.training:
            raise RuntimeError("SegmentPoseEstimator: the SegNet must be in eval mode")
        self.segnet, self.num_obj, self.min_pixels = segnet, segnet.label_nbr - 1, int(min_pixels)
        self.we = WindowEstimator(estimator, refiner, num_points, iteration, max_frames, frame_hw, cam, depth)
        C = segnet.label_nbr
        for slot in self.we.slots:
            slot["det_host"] = torch.empty(max_frames, C, 6, dtype=torch.int32).pin_memory()
            slot["ndet_host"] = torch.empty(max_frames, dtype=torch.int32).pin_memory()
            slot["table"] = torch.cuda.Event()
        # folded on the current stream, which every window's stream waits for before its upload (WindowEstimator.upload)
        with torch.cuda.device(self.we.dev):
            segnet.fold()
        self._pending = None        # the last submitted window, whose pose stage is not enqueued yet
        self._frames = 0

    def submit(self, rgb, depth, frame_ids=None, seed=0):
        """rgb [F,IH,IW,3] uint8, depth [F,IH,IW] int16/uint16 bits: HOST tensors (pinned for an asynchronous upload).
        frame_ids: the per-frame numbers of the seed rule (default: frames counted from 0 over all submitted windows).  Enqueues
        this window's upload and segmentation, then the previous window's pose stage; returns a handle for ``collect``."""
        F = rgb.shape[0]
        frame_ids = list(range(self._frames, self._frames + F)) if frame_ids is None else [int(v) for v in frame_ids]
        if len(frame_ids) != F:
            raise RuntimeError("SegmentPoseEstimator.submit: one frame id per frame")
        self._frames += F
        slot = self.we.upload(rgb, depth)
        with torch.cuda.stream(slot["stream"]):
            seg = segment_frames(self.segnet, slot["rgb"][:F], slot["depth"][:F], self.num_obj, self.min_pixels,
                                 label_out=slot["label"][:F])
            slot["det_host"][:F].copy_(seg.det, non_blocking=True)
            slot["ndet_host"][:F].copy_(seg.ndet, non_blocking=True)
            slot["table"].record(slot["stream"])
        handle = dict(slot=slot, F=F, frame_ids=frame_ids, seed=int(seed), pose=None)
        if self._pending is not None:
            self._run_poses(self._pending)
        self._pending = handle
        return handle

    def _run_poses(self, h):
        """Waits for h's detection table (only that) and enqueues its pose stage on the slot's stream."""
        if h is self._pending:
            self._pending = None
        slot, F = h["slot"], h["F"]
        slot["table"].synchronize()
        det, ndet = slot["det_host"][:F].numpy().copy(), slot["ndet_host"][:F].numpy().copy()
        cls, rois, detections = [], [], []
        for f in range(F):
            rows = det[f, :ndet[f]]
            r = np.stack([det_row_to_roi(row) for row in rows]) if len(rows) else np.zeros((0, 7))
            cls.append(rows[:, 0].astype(np.int64))
            rois.append(r)
            detections += [(f, int(row[0]), roi, h["seed"] + h["frame_ids"][f] * 64 + idx) for idx, (row, roi) in enumerate(zip(rows, r))]
        h["cls"], h["rois"] = cls, rois
        h["pose"] = self.we.run(slot, F, detections)

    def collect(self, handle):
        """-> per frame a dict: cls [n] int64 (ascending), rois [n,7] (PoseCNN layout), pose_wo_refine [n,7], pose [n,7] (q wxyz, t),
        lost [n] bool (zero pose rows, what the reference writes for a lost detection)."""
        if handle["pose"] is None:
            self._run_poses(handle)
        wo, ref, lost = WindowEstimator.collect(handle["pose"])
        out, k = [], 0
        for cls, rois in zip(handle["cls"], handle["rois"]):
            n = len(cls)
            out.append(dict(cls=cls, rois=rois, pose_wo_refine=wo[k:k + n], pose=ref[k:k + n], lost=lost[k:k + n]))
            k += n
        return out
