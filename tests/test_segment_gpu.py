"""GPU: the SegNet -> detection kernels (csrc/segment.hip through densefusion_amd.lib.segment): the input kernel against the
reference's normalisation, the label map against torch.argmax, the per-class statistics and detection lists against numpy,
determinism and window independence, and the engine's SegNet labels against the golden reference logits."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from densefusion_amd import synth
from densefusion_amd.lib import segment

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def test_input_kernel_matches_reference_normalisation():
    rng = np.random.default_rng(0)
    for shape in ((2, 480, 640), (3, 37, 53)):
        rgb = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
        got = segment.segment_input(torch.from_numpy(rgb).cuda()).cpu().numpy()
        # vanilla_segmentation/data_controller.py:78-79, fp32 on the 0..255 values
        want = (np.transpose(rgb, (0, 3, 1, 2)).astype(np.float32) - MEAN[None, :, None, None]) / STD[None, :, None, None]
        assert got.shape == shape + (4,)
        assert np.array_equal(got[..., :3].view(np.uint32), np.transpose(want, (0, 2, 3, 1)).view(np.uint32))
        assert not got[..., 3].any()


def _logits(rng, Fn, H, W, ld, C):
    x = rng.standard_normal((Fn, H, W, ld)).astype(np.float32)
    x[..., C:] = 1e30                                     # padding channels must never be looked at
    n = Fn * H * W
    flat = x.reshape(n, ld)
    rows = rng.choice(n, n // 10, replace=False)
    a, b = rng.integers(0, C, rows.size), rng.integers(0, C, rows.size)
    flat[rows, a] = flat[rows, :C].max(1) + 1.0
    flat[rows, b] = flat[rows, a]                         # exact ties at the maximum (a == b sometimes: no tie)
    flat[rng.choice(n, n // 50, replace=False), rng.integers(0, C, n // 50)] = -np.inf
    flat[rng.choice(n, n // 200, replace=False), rng.integers(0, C, n // 200)] = np.nan
    flat[rng.choice(n, 20, replace=False)] = -np.inf      # whole rows of -inf: the first index
    flat[rng.choice(n, 20, replace=False), :C] = np.nan   # whole rows of NaN
    return x


def _np_stats(label, depth, C):
    Fn = label.shape[0]
    st = np.zeros((Fn, C, 6), np.int64)
    for f in range(Fn):
        for c in range(C):
            m = label[f] == c
            if not m.any():
                continue
            rr, cc = np.nonzero(m)
            st[f, c] = (m.sum(), (m & (depth[f] != 0)).sum(), rr.min(), rr.max() + 1, cc.min(), cc.max() + 1)
    return st


def _np_det(st, num_obj, min_pixels):
    rows = []
    for c in range(1, num_obj + 1):
        if st[c, 1] > min_pixels:
            rows.append((c, st[c, 2], st[c, 3], st[c, 4], st[c, 5], st[c, 1]))
    return np.array(rows, np.int64).reshape(-1, 6)


@pytest.mark.parametrize("ld", [24, 32])
@pytest.mark.parametrize("Fn,H,W", [(1, 480, 640), (8, 480, 640), (1, 37, 53), (8, 37, 53)])
def test_label_map_equals_torch_argmax(ld, Fn, H, W):
    C = 22
    rng = np.random.default_rng(ld * 100 + Fn * 10 + H)
    x = torch.from_numpy(_logits(rng, Fn, H, W, ld, C)).cuda()
    depth = torch.from_numpy(rng.integers(0, 3, (Fn, H, W)).astype(np.int16)).cuda()
    seg = segment.detect(x, C, depth, C - 1, 50)
    want = torch.argmax(x[..., :C], -1).to(torch.int32)
    assert torch.equal(seg.label, want)


@pytest.mark.parametrize("ld,C", [(64, 64), (64, 33), (36, 33)])
def test_wide_logits_label_and_statistics(ld, C):
    """ld > 32 takes the kernel instance that holds 16 float4s per lane (above 64 KiB of LDS from ld 56 on); C = 64 is the most
    classes the per-lane statistics take."""
    rng = np.random.default_rng(ld + C)
    for Fn, H, W in ((2, 480, 640), (3, 37, 53)):
        x = torch.from_numpy(_logits(rng, Fn, H, W, ld, C)).cuda()
        depth_np = rng.integers(0, 3, (Fn, H, W)).astype(np.uint16)
        seg = segment.detect(x, C, torch.from_numpy(depth_np.view(np.int16)).cuda(), C - 1, 50)
        want = torch.argmax(x[..., :C], -1).to(torch.int32)
        assert torch.equal(seg.label, want)
        st = _np_stats(want.cpu().numpy(), depth_np, C)
        assert np.array_equal(seg.stats.cpu().numpy(), st)
        det, ndet = seg.det.cpu().numpy(), seg.ndet.cpu().numpy()
        for f in range(Fn):
            exp = _np_det(st[f], C - 1, 50)
            assert ndet[f] == len(exp) and np.array_equal(det[f, :ndet[f]], exp) and not det[f, ndet[f]:].any(), f


def test_statistics_and_detections_equal_numpy():
    rng = np.random.default_rng(7)
    C, num_obj, min_pixels, ld = 22, 20, 50, 24
    Fn, H, W = 4, 120, 160
    label = np.zeros((Fn, H, W), np.int64)
    depth = rng.integers(1, 1000, (Fn, H, W)).astype(np.uint16)
    depth[rng.random((Fn, H, W)) < 0.3] = 0
    # frame 0: blobs and scattered pixels of many classes, including class 21 (> num_obj) and the frame's edges
    for c in range(1, 22):
        r0, c0 = rng.integers(0, H - 20), rng.integers(0, W - 20)
        label[0, r0:r0 + rng.integers(5, 40), c0:c0 + rng.integers(5, 40)] = c
    label[0, rng.random((H, W)) < 0.02] = 5
    label[0, 0, 0], label[0, H - 1, W - 1] = 6, 6
    # frame 1: class 21 big, class 3 with exactly min_pixels and class 4 with min_pixels + 1 depth-valid pixels
    label[1, 50:100, 50:100] = 21
    for c, n in ((3, min_pixels), (4, min_pixels + 1)):
        idx = rng.choice(np.flatnonzero(label[1].reshape(-1) == 0), n + 7, replace=False)
        label[1].reshape(-1)[idx] = c
        depth[1].reshape(-1)[idx[:n]] = 77
        depth[1].reshape(-1)[idx[n:]] = 0
    # frame 2: background only (no detection); frame 3: noise over all classes
    label[3] = rng.integers(0, C, (H, W))
    onehot = np.full((Fn, H, W, ld), -5.0, np.float32)
    np.put_along_axis(onehot, label[..., None], 3.0, axis=-1)
    seg = segment.detect(torch.from_numpy(onehot).cuda(), C, torch.from_numpy(depth.view(np.int16)).cuda(), num_obj, min_pixels)
    assert np.array_equal(seg.label.cpu().numpy(), label)
    st = _np_stats(label, depth, C)
    assert np.array_equal(seg.stats.cpu().numpy(), st)
    det, ndet = seg.det.cpu().numpy(), seg.ndet.cpu().numpy()
    for f in range(Fn):
        want = _np_det(st[f], num_obj, min_pixels)
        assert ndet[f] == len(want), f
        assert np.array_equal(det[f, :ndet[f]], want), f
        assert not det[f, ndet[f]:].any()
        assert not np.isin(det[f, :ndet[f], 0], [0, 21]).any()
    assert ndet[2] == 0
    assert 4 in det[1, :ndet[1], 0] and 3 not in det[1, :ndet[1], 0]


def test_deterministic_and_window_independent():
    rng = np.random.default_rng(3)
    C, ld, Fn, H, W = 22, 24, 8, 480, 640
    x = torch.from_numpy(rng.standard_normal((Fn, H, W, ld)).astype(np.float32)).cuda()
    depth = torch.from_numpy(rng.integers(0, 2, (Fn, H, W)).astype(np.int16)).cuda()
    a, b = segment.detect(x, C, depth, 21, 50), segment.detect(x, C, depth, 21, 50)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for f in (0, 5):
        alone = segment.detect(x[f:f + 1].contiguous(), C, depth[f:f + 1].contiguous(), 21, 50)
        for u, v in zip(alone, a):
            assert torch.equal(u[0], v[f])


def test_engine_segnet_labels_match_golden_reference():
    """The golden logits come from the reference module itself.  The engine reproduces them to 2e-4 of their scale
    (tests/test_segnet_gpu.py), so wherever the golden top-two margin exceeds twice that bound the label must be the same."""
    from densefusion_amd.vanilla_segmentation.segnet import SegNet
    g = np.load(os.path.join(G, "segnet_small.npz"))
    net = SegNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_segnet_state_dict(int(g["meta"][0])).items()})
    net = net.cuda().eval()
    x = torch.from_numpy(g["x"]).cuda()
    x4 = F.pad(x.permute(0, 2, 3, 1), (0, 1)).contiguous()
    logits = net.forward_nhwc(x4)
    Fn, H, W = x.shape[0], x.shape[2], x.shape[3]
    depth = torch.ones(Fn, H, W, dtype=torch.int16, device="cuda")
    seg = segment.detect(logits, net.label_nbr, depth, 21, 50)
    ref = g["logits"]
    top2 = np.sort(ref, axis=1)[:, -2:]
    bound = 2 * 2e-4 * np.abs(ref).max()
    clear = (top2[:, 1] - top2[:, 0]) > bound
    assert clear.mean() > 0.99, clear.mean()          # 0.9988 of the 4096 pixels
    got = seg.label.cpu().numpy()
    assert np.array_equal(got[clear], ref.argmax(1)[clear])
    # the eval forward is forward_nhwc plus the slice and permute
    assert torch.equal(net(x), logits[..., :net.label_nbr].permute(0, 3, 1, 2).contiguous())


def test_detect_takes_views_and_rejects_other_dtypes():
    rng = np.random.default_rng(5)
    nchw = torch.from_numpy(rng.standard_normal((2, 24, 37, 53)).astype(np.float32)).cuda()
    depth = torch.ones(2, 37, 53, dtype=torch.int16, device="cuda")
    view = nchw.permute(0, 2, 3, 1)                      # channels-last view of an NCHW tensor: read through a copy
    seg = segment.detect(view, 22, depth, 21, 50)
    assert torch.equal(seg.label, torch.argmax(view[..., :22], -1).to(torch.int32))
    with pytest.raises(RuntimeError):
        segment.detect(view.double(), 22, depth, 21, 50)
    with pytest.raises(RuntimeError):
        segment.detect(view.cpu(), 22, depth, 21, 50)


def test_segment_frames_checks_class_count():
    from densefusion_amd.vanilla_segmentation.segnet import SegNet
    net = SegNet(label_nbr=5).cuda().eval()
    rgb = torch.zeros(1, 32, 32, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        segment.segment_frames(net, rgb, torch.zeros(1, 32, 32, dtype=torch.int16, device="cuda"), 21)
