"""GPU: SegNet training batches from rendered customCAD scenes.  ``df_seg_batch`` against its numpy restatement (tests/seg_feed_np.py)
bit for bit in x, target and counts, its bad descriptors and argument errors; ``SegNet`` with few classes and a channels-last input in
training mode; ``RenderedSegDataset`` against the restatement applied to the device's own renders, and its purity."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cad_raster_np as mnp
import cad_scene_np as snp
import seg_feed_np as sf

pytestmark = pytest.mark.gpu
IH, IW, NODE_PROJ = snp.IH, snp.IW, snp.NODE_PROJ
O, NB, BH, BW = 4, 3, 40, 60
SIGMA5 = sf.noise_mul_of(5.0)
CMAP = [0, 1, 2, 3, 4]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _up16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


@pytest.fixture(scope="module")
def frames():
    """The four rendered 37 x 53 frames of ``small_scene()`` (the last one empty) and a fifth, fabricated one whose label plane holds 5
    and 6, above O = 4; a fabricated pool of 3 backgrounds of 40 x 60.  Host arrays and their device copies."""
    _dev()
    from densefusion_amd.lib import preprocess as pp
    s = snp.small_scene()
    rgb, _, label, _ = pp.cad_render_scene(_up(s["vertices"]), _up(s["colors"]), _up(s["triangles"]), s["tri_begin"], s["scales"], s["poses"],
                                           NODE_PROJ, (IH, IW), present=s["present"], cull=1)
    rgb, label = rgb.cpu().numpy(), label.cpu().numpy()
    assert not label[3].any() and all(label[f].any() for f in range(3)) and int(label.max()) <= O
    rng = np.random.default_rng(5)
    rgb = np.concatenate([rgb, rng.integers(0, 256, (1, IH, IW, 3), dtype=np.uint8)])
    label = np.concatenate([label, rng.integers(0, O + 3, (1, IH, IW)).astype(np.uint16)])
    assert (label[4] > O).any()
    back = rng.integers(0, 256, (NB, BH, BW, 3), dtype=np.uint8)
    return dict(rgb=rgb, label=label, back=back, d_rgb=_up(rgb), d_label=_up16(label), d_back=_up(back))


def _both(fr, desc, window, cmap=CMAP, C=5, back=True, blur=1, mul=0, check=True):
    from densefusion_amd.lib import preprocess as pp
    got = pp.seg_batch(fr["d_rgb"], fr["d_label"], cmap, C, desc, window, back=fr["d_back"] if back else None, blur=blur, noise_mul=mul, check=check)
    want = sf.seg_batch(fr["rgb"], fr["label"], cmap, C, desc, window, fr["back"] if back else None, blur, mul)
    return tuple(g.cpu().numpy() for g in got), want


def _same(got, want, what=""):
    for name, g, w in zip(("x", "target", "counts"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        bad = np.argwhere(g.view(np.uint32 if g.dtype == np.float32 else g.dtype) != w.view(np.uint32 if w.dtype == np.float32 else w.dtype))
        assert len(bad) == 0, (what, name, bad[:5])


def _corner_desc(H, W, frames_of=(0, 1, 2, 3), flips=(0, 1, 2, 3)):
    """per flip: the window at the frame's four corners, the background window at the pool's four corners, each corner on another
    frame and background"""
    desc = []
    for flip in flips:
        for k, (top, left) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            desc.append([frames_of[k % len(frames_of)], top * (IH - H), left * (IW - W), flip, k % NB, top * (BH - H), left * (BW - W),
                         1000 * flip + k])
    return desc


# the kernel's output tile is 16 rows x 32 columns: 33 x 50 crosses its edges in both axes (rows 16 and 32, column 32), 37 x 53 too
@pytest.mark.parametrize("window", [(1, 1), (5, 7), (32, 32), (33, 50), (37, 53)])
def test_windows_flips_blur_and_noise_equal_the_restatement_bit_for_bit(frames, window):
    desc = _corner_desc(*window) + [[4, 0, 0, 3, 2, BH - window[0], 0, 0xFFFFFFFF]]
    for blur in (0, 1):
        for mul in (0, SIGMA5, 2 ** 31 - 1):
            got, want = _both(frames, desc, window, blur=blur, mul=mul)
            _same(got, want, (window, blur, mul))
            if mul == 2 ** 31 - 1 and window[0] >= 32:                         # both clamps are reached
                v = np.rint(want[0][..., :3].astype(np.float64) * sf.STD + sf.MEAN)
                assert v.min() == 0 and v.max() == 255
    assert want[2].sum() == len(desc) * window[0] * window[1]


def test_items_with_and_without_a_background_and_no_pool(frames):
    desc = _corner_desc(33, 50)
    for k in range(0, len(desc), 3):
        desc[k][4] = -1                                                        # b = -1 on some items of the call
    got, want = _both(frames, desc, (33, 50), mul=SIGMA5)
    _same(got, want)
    none = [d[:4] + [-1, 0, 0, d[7]] for d in desc]
    got0, want0 = _both(frames, none, (33, 50), back=False, mul=SIGMA5)        # NB = 0
    _same(got0, want0)
    assert np.array_equal(got0[0][0], got[0][0]) and not np.array_equal(got0[0][7], got[0][7])     # item 7: the empty frame, with a background
    assert np.array_equal(got0[2], got[2]), "the counts do not depend on the background"


def test_class_maps(frames):
    desc = _corner_desc(33, 50, frames_of=(0, 1, 2, 4))
    got, want = _both(frames, desc, (33, 50), cmap=[0, 1, 0, 2, 0], C=3)       # objects 1 and 3 are distractors
    _same(got, want)
    assert got[2][:, 1].any() and got[2][:, 2].any()
    got, want = _both(frames, desc, (33, 50), cmap=[0, 63, 17, 1, 62], C=64)
    _same(got, want)
    assert got[2].shape == (16, 64) and got[2][:, 63].any() and got[2][:, 62].any()


def test_one_item_and_seventy(frames):
    got, want = _both(frames, [[1, 2, 3, 1, 1, 4, 5, 99]], (33, 50), mul=SIGMA5)
    _same(got, want, "B = 1")
    rng = np.random.default_rng(70)
    H, W = 20, 41
    desc = [[k % 5, int(rng.integers(0, IH - H + 1)), int(rng.integers(0, IW - W + 1)), int(rng.integers(0, 4)), int(rng.integers(-1, NB)),
             int(rng.integers(0, BH - H + 1)), int(rng.integers(0, BW - W + 1)), int(rng.integers(0, 2 ** 32))] for k in range(70)]
    got, want = _both(frames, desc, (H, W), mul=SIGMA5)
    _same(got, want, "B = 70")
    # determinism: the same call again; an item alone equals the item inside the larger call
    again, _ = _both(frames, desc, (H, W), mul=SIGMA5)
    _same(again, got, "second call")
    for n in (0, 33, 69):
        solo, _ = _both(frames, [desc[n]], (H, W), mul=SIGMA5)
        _same(solo, tuple(g[n:n + 1] for g in got), ("solo", n))


BAD = {"f high": [5, 0, 0, 0, -1, 0, 0, 1], "f negative": [-1, 0, 0, 0, -1, 0, 0, 1], "y0 high": [0, IH - 33 + 1, 0, 0, -1, 0, 0, 1],
       "x0 high": [0, 0, IW - 50 + 1, 0, -1, 0, 0, 1], "y0 negative": [0, -1, 0, 0, -1, 0, 0, 1], "x0 negative": [0, 0, -1, 0, -1, 0, 0, 1],
       "flip high": [0, 0, 0, 4, -1, 0, 0, 1], "flip negative": [0, 0, 0, -1, -1, 0, 0, 1], "b high": [0, 0, 0, 0, NB, 0, 0, 1],
       "b low": [0, 0, 0, 0, -2, 0, 0, 1], "by0 high": [0, 0, 0, 0, 0, BH - 33 + 1, 0, 1], "bx0 high": [0, 0, 0, 0, 0, 0, BW - 50 + 1, 1],
       "by0 negative": [0, 0, 0, 0, 0, -1, 0, 1], "bx0 negative": [0, 0, 0, 0, 0, 0, -1, 1], "huge": [2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 0, 0, 0, 0, 1]}


def test_bad_descriptors_give_zeros_and_leave_their_neighbours(frames):
    from densefusion_amd.lib import preprocess as pp
    good = _corner_desc(33, 50, flips=(3,))
    desc = []
    for row in BAD.values():
        desc += [good[len(desc) % 4], row]
    desc.append(good[0])
    got, want = _both(frames, desc, (33, 50), mul=SIGMA5, check=False)
    _same(got, want)
    for k in range(len(BAD)):
        assert not got[0][2 * k + 1].any() and not got[1][2 * k + 1].any() and not got[2][2 * k + 1].any()
        assert got[2][2 * k].sum() == 33 * 50
    for name, row in BAD.items():                                             # the wrapper checks a host descriptor first
        with pytest.raises(ValueError):
            pp.seg_batch(frames["d_rgb"], frames["d_label"], CMAP, 5, [good[0], row], (33, 50), back=frames["d_back"])


def test_argument_errors_write_nothing(frames):
    from densefusion_amd import _lib
    L = _lib.lib()
    B, H, W, C = 2, 5, 7, 5
    x = torch.full((B, H, W, 4), 7.0, device="cuda")
    tg = torch.full((B, H, W), 7, dtype=torch.int64, device="cuda")
    ct = torch.full((B, C), 7, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(int(L.df_seg_batch_scratch_bytes(B, H, W, C)), dtype=torch.uint8, device="cuda")
    assert scratch.numel() > 0
    desc = _up(np.array([[0, 0, 0, 0, 0, 0, 0, 1], [1, 1, 1, 3, -1, 0, 0, 2]], dtype=np.int32))
    cmap = np.array(CMAP, dtype=np.int32)
    good = dict(rgb=frames["d_rgb"].data_ptr(), label=frames["d_label"].data_ptr(), F=5, IH=IH, IW=IW, back=frames["d_back"].data_ptr(), NB=NB,
                BH=BH, BW=BW, class_map=cmap.ctypes.data, O=O, C=C, desc=desc.data_ptr(), B=B, H=H, W=W, blur=1, noise_mul=SIGMA5,
                x=x.data_ptr(), target=tg.data_ptr(), counts=ct.data_ptr(), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())

    def call(**kw):
        a = dict(good, **kw)
        return L.df_seg_batch(*[a[k] for k in good], _lib.current_stream())

    def cm(*v):
        return np.array(v, dtype=np.int32)
    maps = [cm(1, 1, 2, 3, 4), cm(0, 5, 2, 3, 4), cm(0, 1, 2, 3, -1)]
    cases = [dict(rgb=None), dict(label=None), dict(class_map=None), dict(desc=None), dict(x=None), dict(target=None), dict(counts=None),
             dict(scratch=None), dict(back=None), dict(NB=0), dict(NB=-1), dict(F=0), dict(F=65536), dict(IH=0), dict(IW=0),
             dict(IH=1 << 16, IW=1 << 15), dict(H=0), dict(H=IH + 1), dict(W=0), dict(W=IW + 1), dict(IH=8192, IW=4096, H=8192, W=4096),
             dict(B=0), dict(B=65536), dict(O=0), dict(O=65), dict(C=0), dict(C=65)] + [dict(class_map=m.ctypes.data) for m in maps] + \
            [dict(BH=H - 1), dict(BW=W - 1), dict(blur=-1), dict(blur=2), dict(noise_mul=-1), dict(x=x.data_ptr() + 4), dict(target=tg.data_ptr() + 4),
             dict(scratch_bytes=0), dict(scratch_bytes=scratch.numel() - 1)]
    for kw in cases:
        assert call(**kw) == -1 and L.df_last_error(), kw
    for q in ((0, H, W, C), (65536, H, W, C), (B, 0, W, C), (B, H, 0, C), (B, 4096, 4097, C), (B, H, W, 0), (B, H, W, 65)):
        assert L.df_seg_batch_scratch_bytes(*q) == 0, q
    torch.cuda.synchronize()
    assert bool((x == 7).all()) and bool((tg == 7).all()) and bool((ct == 7).all())
    assert call() == 0
    torch.cuda.synchronize()
    want = sf.seg_batch(frames["rgb"], frames["label"], CMAP, C, desc.cpu().numpy(), (H, W), frames["back"], 1, SIGMA5)
    _same((x.cpu().numpy(), tg.cpu().numpy(), ct.cpu().numpy()), want)


# ---- SegNet: few classes, channels-last input in training mode ----------------------------------------------------------------------
def rel(a, b):                                                                  # tests/test_segnet_train_gpu.py's measure
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    n = float(b.norm())
    return float((a - b).norm()) / (n if n > 0 else 1.0)


@pytest.mark.parametrize("label_nbr", [2, 3, 5])
def test_segnet_trains_few_classes_from_a_channels_last_input(frames, label_nbr):
    """The bounds are those of tests/test_segnet_train_gpu.py::test_cross_entropy_against_fp64: the loss within 1e-6 relative of fp64
    ``F.cross_entropy`` of the returned logits, the gradient within rel < 1e-6."""
    from densefusion_amd.lib import preprocess as pp
    from densefusion_amd.vanilla_segmentation.loss import Loss
    from densefusion_amd.vanilla_segmentation.segnet import SegNet
    cmap = [0] + [1 + o % (label_nbr - 1) for o in range(O)]
    x, target, _ = pp.seg_batch(frames["d_rgb"], frames["d_label"], cmap, label_nbr, [[0, 2, 10, 1, 0, 3, 4, 5], [1, 5, 21, 2, -1, 0, 0, 6]],
                                (32, 32), back=frames["d_back"], noise_mul=SIGMA5)
    assert len(torch.unique(target)) >= 2
    torch.manual_seed(label_nbr)
    net = SegNet(label_nbr=label_nbr, trainable=True).cuda().train()
    twin = SegNet(label_nbr=label_nbr, trainable=True).cuda().train()
    twin.load_state_dict(net.state_dict())
    y = net.forward_nhwc(x)
    y2 = twin(x[..., :3].permute(0, 3, 1, 2).contiguous())
    assert tuple(y.shape) == (2, label_nbr, 32, 32) and y.requires_grad and torch.equal(y, y2)
    assert y._nhwc.shape[3] % 4 == 0 and y._nhwc.shape[3] >= label_nbr
    for (k, a), b in zip(net.state_dict().items(), twin.state_dict().values()):
        assert torch.equal(a, b), k                                            # the BatchNorm buffers moved alike
    y._nhwc.retain_grad()
    loss = Loss()(y, target)
    loss.backward()
    l64 = y.detach().double().cpu().permute(0, 2, 3, 1).reshape(-1, label_nbr)
    t = target.cpu().reshape(-1)
    want = F.cross_entropy(l64, t)
    want_bias = (torch.softmax(l64, dim=1) - F.one_hot(t, label_nbr).double()).sum(dim=0) / l64.shape[0]
    got_bias = net.conv11d.bias.grad
    print(f"label_nbr {label_nbr}: loss {float(loss.detach()):.7f} vs {float(want):.7f}, bias gradient {rel(got_bias, want_bias):.1e}")
    assert abs(float(loss.detach()) - float(want)) <= 1e-6 * abs(float(want))
    assert rel(got_bias, want_bias) < 1e-6
    pad = y._nhwc.grad[..., label_nbr:]
    assert torch.equal(pad, torch.zeros_like(pad)), "padded channels get no gradient"
    for name, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert bool(torch.isfinite(y).all())
    with pytest.raises(NotImplementedError):
        SegNet(label_nbr=label_nbr).cuda().train().forward_nhwc(x)           # training stays opt-in


# ---- RenderedSegDataset ---------------------------------------------------------------------------------------------------------------
def _meshes():
    """two icospheres of ``small_scene()``'s subdivision and radii (file units) and a box, each (vertices, triangles, colours)"""
    rng = np.random.default_rng(31)
    out = []
    for v, f in (mnp.icosphere(1, 160.0), mnp.icosphere(1, 120.0), snp.box([-90.0] * 3, [90.0] * 3)):
        out.append((v.astype(np.float32), np.asarray(f).astype(np.int32), rng.integers(0, 256, (len(v), 3), dtype=np.uint8)))
    return out


def _dataset(chunk=4, use_noise=True, first_seed=3, **kw):
    from densefusion_amd.datasets.customCAD.online_seg import RenderedSegDataset
    m = _meshes()
    back = np.random.default_rng(8).integers(0, 256, (2, 44, 80, 3), dtype=np.uint8)
    return RenderedSegDataset(m[:2], use_noise, distractors=m[2:], image_dims=(40, 72), window=(32, 64), backgrounds=back, light="random",
                              chunk=chunk, first_seed=first_seed, frames=10, **kw), back


def _expected(ds, back, i):
    """item i from the restatement, on the device's own render of the view"""
    from densefusion_amd.lib import preprocess as pp
    info = ds.view_info(i)
    rgb, _, label, _ = ds.renderer.render(info["poses"][None], present=info["present"][None], cull=ds.cull, light=info["light"][None])
    if info["plan"] is not None:
        rgb = pp.color_jitter(rgb, info["plan"][None])
    row = info["desc"].copy()
    row[0] = 0
    want = sf.seg_batch(rgb.cpu().numpy(), label.cpu().numpy(), ds.class_map, ds.n_classes, [row], ds.window, back, ds.blur,
                        ds.noise_mul if ds.use_noise else 0)
    return want, info


def test_dataset_items_equal_the_restatement_on_the_device_render():
    _dev()
    ds, back = _dataset()
    assert ds.n_classes == 3 and ds.class_map.tolist() == [0, 1, 2, 0] and len(ds) == 10
    xs, ts = ds.batch(range(10))
    assert tuple(xs.shape) == (10, 32, 64, 4) and xs.dtype == torch.float32 and tuple(ts.shape) == (10, 32, 64) and ts.dtype == torch.int64
    seen = np.zeros(3, dtype=np.int64)
    for i in range(10):
        want, info = _expected(ds, back, i)
        x, t = ds[i]
        assert x.is_cuda and tuple(x.shape) == (32, 64, 4) and tuple(t.shape) == (32, 64)
        _same((x.cpu().numpy()[None], t.cpu().numpy()[None], info["counts"].cpu().numpy()[None]), want, i)
        assert torch.equal(xs[i], x) and torch.equal(ts[i], t)
        assert info["seed"] == 3 + i and info["plan"] is not None and len(info["records"]) == 3
        seen += want[2][0]
    print("class pixels over the 10 views:", seen.tolist())
    assert seen[1] > 0 and seen[2] > 0, "both models are seen"


def test_dataset_items_are_a_pure_function_of_the_view_seed():
    _dev()
    ds, back = _dataset()
    xs, ts = ds.batch(range(10))
    for i in (0, 5, 9):
        x1, t1 = ds.batch([i])
        assert torch.equal(x1[0], xs[i]) and torch.equal(t1[0], ts[i])
    other, _ = _dataset(chunk=3)                                               # another chunking, another construction
    xo, to = other.batch(range(10))
    assert torch.equal(xo, xs) and torch.equal(to, ts)
    assert [other.view_info(i)["desc"][1:].tolist() for i in range(10)] == [ds.view_info(i)["desc"][1:].tolist() for i in range(10)]
    order = ds.permutation(np.random.RandomState(1))                           # the cut of the chunks moves: the items do not
    assert sorted(order.tolist()) == list(range(10))
    xp, tp = ds.batch(order)
    assert torch.equal(xp, xs[torch.as_tensor(order)]) and torch.equal(tp, ts[torch.as_tensor(order)])
    ds.set_epoch(1)
    assert ds.view_seed(0) == 13 and ds.view_info(0)["seed"] == 13
    want, info = _expected(ds, back, 0)
    x, t = ds[0]
    _same((x.cpu().numpy()[None], t.cpu().numpy()[None], info["counts"].cpu().numpy()[None]), want, "epoch 1")
    assert not torch.equal(x, xs[0])
    ds.set_epoch(0)
    assert torch.equal(ds[0][0], xs[0]) and torch.equal(ds[0][1], ts[0])


def test_dataset_without_noise_keeps_backgrounds_and_blur_only():
    _dev()
    ds, back = _dataset(use_noise=False)
    for i in range(10):
        want, info = _expected(ds, back, i)
        assert info["plan"] is None and info["desc"][3] == 0                   # no jitter, no flip
        x, t = ds[i]
        _same((x.cpu().numpy()[None], t.cpu().numpy()[None], info["counts"].cpu().numpy()[None]), want, i)
    assert ds.noise_mul == SIGMA5, "the setting stays; the call gets 0"
    from densefusion_amd.datasets.customCAD.online_seg import RenderedSegDataset
    m = _meshes()
    for kw in (dict(window=(32, 50)), dict(window=(64, 64)), dict(backgrounds=np.zeros((1, 31, 80, 3), dtype=np.uint8)), dict(blur=2)):
        with pytest.raises(ValueError):
            RenderedSegDataset(m[:2], image_dims=(40, 72), **dict(dict(window=(32, 64)), **kw))
