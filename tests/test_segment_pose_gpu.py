"""GPU: SegmentPoseEstimator (lib/segment_pose.py) end to end on fabricated frames -- poses bit-identical to the composed path
SegNet.forward -> torch.argmax -> numpy boxes -> ROI helper -> WindowEstimator.submit with the label map and detections from the host."""
import numpy as np
import pytest
import torch

from densefusion_amd import synth
from densefusion_amd.lib import preprocess as pp
from densefusion_amd.lib.eval_window import WindowEstimator
from densefusion_amd.lib.network import PoseNet, PoseRefineNet
from densefusion_amd.lib.segment import det_row_to_roi
from densefusion_amd.lib.segment_pose import SegmentPoseEstimator
from densefusion_amd.vanilla_segmentation.segnet import SegNet

pytestmark = pytest.mark.gpu
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
BLOCKS = [[(1, 2, 3, 3, 4), (2, 8, 10, 2, 2), (3, 10, 1, 4, 6)],
          [(1, 5, 5, 5, 5), (3, 1, 14, 2, 3)],
          [],
          [(2, 0, 0, 2, 3), (1, 13, 16, 2, 4)]]          # at the frame's top-left and bottom-right edges


def _nets(K, N):
    segnet = SegNet(label_nbr=K + 1)
    segnet.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_segnet_block_state_dict(K + 1).items()})
    est, rfn = PoseNet(N, K), PoseRefineNet(N, K)
    est.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(synth.posenet_spec(K), 31).items()})
    rfn.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(synth.refiner_spec(K), 1031).items()})
    return segnet.cuda().eval(), est.cuda().eval(), rfn.cuda().eval()


def _composed(segnet, est, rfn, rgb, depth, N, iters, min_pixels, frame_ids, seed):
    x = (np.transpose(rgb, (0, 3, 1, 2)).astype(np.float32) - MEAN[None, :, None, None]) / STD[None, :, None, None]
    label = torch.argmax(segnet(torch.from_numpy(x).cuda()), 1).to(torch.int32).cpu().numpy()
    dets, rois_per_frame = [], []
    for f in range(rgb.shape[0]):
        rows = []
        for c in range(1, segnet.label_nbr):
            m = label[f] == c
            nv = int((m & (depth[f] != 0)).sum())
            if nv > min_pixels:
                rr, cc = np.nonzero(m)
                rows.append((c, rr.min(), rr.max() + 1, cc.min(), cc.max() + 1, nv))
        rois = [det_row_to_roi(r) for r in rows]
        rois_per_frame.append(np.array(rois).reshape(-1, 7))
        dets += [(f, int(roi[1]), roi, seed + frame_ids[f] * 64 + idx) for idx, roi in enumerate(rois)]
    we = WindowEstimator(est, rfn, N, iters, rgb.shape[0], depth=1)
    out = we.collect(we.submit(torch.from_numpy(rgb), torch.from_numpy(depth.view(np.int16)), torch.from_numpy(label), dets))
    return rois_per_frame, dets, out


@pytest.mark.parametrize("depth_in_flight", [1, 2])
def test_segment_pose_estimator_matches_composed_path(depth_in_flight):
    K, N, iters, min_pixels, seed = 21, 500, 2, 2, 3
    rng = np.random.default_rng(11)
    frames = [synth.block_frame(rng, b) for b in BLOCKS]
    rgb = np.stack([f[0] for f in frames])
    depth = np.stack([f[1] for f in frames])
    segnet, est, rfn = _nets(K, N)
    frame_ids = [10, 11, 12, 13]
    rois_want, dets, (wo, pose, lost) = _composed(segnet, est, rfn, rgb, depth, N, iters, min_pixels, frame_ids, seed)
    live = [pp.get_bbox(roi) for (_, _, roi, _), l in zip(dets, lost) if not l]
    buckets = {(b[1] - b[0], b[3] - b[2]) for b in live}
    assert len(live) >= 3 and len(buckets) >= 2, (len(live), buckets)

    spe = SegmentPoseEstimator(segnet, est, rfn, N, iters, max_frames=4, depth=depth_in_flight, min_pixels=min_pixels)
    rgb_h = torch.from_numpy(rgb).pin_memory()
    depth_h = torch.from_numpy(depth.view(np.int16)).pin_memory()
    # the whole window, then the same frames as two windows of 2 (the second submitted before the first is collected at depth 2)
    got = spe.collect(spe.submit(rgb_h, depth_h, frame_ids, seed))
    if depth_in_flight > 1:
        h1 = spe.submit(rgb_h[:2], depth_h[:2], frame_ids[:2], seed)
        h2 = spe.submit(rgb_h[2:], depth_h[2:], frame_ids[2:], seed)
        split = spe.collect(h1) + spe.collect(h2)
    else:
        split = spe.collect(spe.submit(rgb_h[:2], depth_h[:2], frame_ids[:2], seed))
        split += spe.collect(spe.submit(rgb_h[2:], depth_h[2:], frame_ids[2:], seed))
    k = 0
    for f, (r, s) in enumerate(zip(got, split)):
        n = len(r["cls"])
        assert np.array_equal(r["rois"], rois_want[f]), f
        assert np.array_equal(r["cls"], rois_want[f][:, 1].astype(np.int64))
        assert np.array_equal(r["pose_wo_refine"], wo[k:k + n]) and np.array_equal(r["pose"], pose[k:k + n]), f
        assert np.array_equal(r["lost"], lost[k:k + n])
        for key in ("cls", "rois", "pose_wo_refine", "pose", "lost"):
            assert np.array_equal(r[key], s[key]), (f, key)
        k += n
    assert k == len(dets) and len(got[2]["cls"]) == 0
    assert pose[~lost].any(axis=1).all()
