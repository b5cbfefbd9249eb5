"""GPU: ``df_seg_score`` against its numpy restatement (tests/seg_score_np.py) and ``torch.argmax`` in conf, skipped and label_out, bit
for bit; its determinism, frame independence and argument errors; ``df_seg_masks`` against the restatement and through
``df_cad_item_table``.  Integers only: no tolerance anywhere."""
import numpy as np
import pytest
import torch

import seg_score_np as ssn

pytestmark = pytest.mark.gpu
CLASSES = [(2, 4), (3, 4), (5, 8), (22, 24), (22, 32), (64, 64)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ppb():
    from densefusion_amd import _lib
    return int(_lib.lib().df_seg_score_block_pixels())


def _targets(rng, F, H, W, C):
    """uniform classes, with -1, C, 255 and 2^40 at up to four pixels of every frame"""
    t = rng.integers(0, C, (F, H, W)).astype(np.int64)
    n_bad = min(4, H * W // 2)
    for f in range(F):
        t[f].reshape(-1)[rng.choice(H * W, size=n_bad, replace=False)] = np.array([-1, C, 255, 2 ** 40])[:n_bad]
    return t, n_bad


def _check(logits, target, C, what=""):
    """the wrapper's three outputs against the restatement, and the label against torch.argmax; returns the device outputs"""
    from densefusion_amd.lib import segment_score as ss
    d_logits, d_target = _up(logits), _up(target)
    conf, skipped, label = ss.seg_score(d_logits, d_target, C)
    want_conf, want_skipped, want_label = ssn.seg_score(logits, target, C)
    for name, g, w in (("conf", conf, want_conf), ("skipped", skipped, want_skipped), ("label", label, want_label)):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, bad[:5])
    assert torch.equal(label.long(), torch.argmax(d_logits[..., :C], dim=-1)), (what, "torch.argmax")
    return conf, skipped, label


@pytest.mark.parametrize("C,ld", CLASSES)
def test_frames_of_every_size_equal_the_restatement_bit_for_bit(C, ld):
    _dev()
    P = _ppb()
    assert P == 4096, "the shapes below put a frame on each side of the kernel's pixels per workgroup"
    rng = np.random.default_rng(100 * C + ld)
    for H, W in ((1, 1), (1, 3), (5, 7), (33, 65), (64, P // 64), (17, 241)):
        assert (H, W) != (17, 241) or H * W == P + 1
        logits = ssn.tie_logits(rng, 1, H, W, C, ld)                          # integers -2..2, two NaN, pads of 1e30
        target, n_bad = _targets(rng, 1, H, W, C)
        conf, skipped, label = _check(logits, target, C, (H, W))
        assert int(skipped[0]) == n_bad and int(conf.sum()) == H * W - n_bad
        assert int(label.max()) < C, "a pad channel never wins"


@pytest.mark.parametrize("C,ld", [(3, 4), (22, 24), (64, 64)])
def test_three_frames_equal_their_solo_calls_and_two_calls_agree(C, ld):
    _dev()
    from densefusion_amd.lib import segment_score as ss
    rng = np.random.default_rng(7 + C)
    H, W = 33, 65
    logits = ssn.tie_logits(rng, 3, H, W, C, ld, nans=6)
    target, _ = _targets(rng, 3, H, W, C)
    conf, skipped, label = _check(logits, target, C)
    for f in range(3):
        c1, s1, l1 = ss.seg_score(_up(logits[f:f + 1]), _up(target[f:f + 1]), C)
        assert torch.equal(c1[0], conf[f]) and torch.equal(s1[0], skipped[f]) and torch.equal(l1[0], label[f]), f
    again = ss.seg_score(_up(logits), _up(target), C)
    assert all(torch.equal(a, b) for a, b in zip(again, (conf, skipped, label)))


def test_one_cell_and_every_cell():
    _dev()
    # the worst contention: 64 x 64 pixels that all land in cell (0, 0)
    for C, ld in ((3, 4), (22, 24)):
        logits = np.zeros((1, 64, 64, ld), dtype=np.float32)
        logits[..., 0] = 1.0
        conf, skipped, _ = _check(logits, np.zeros((1, 64, 64), dtype=np.int64), C)
        assert int(conf[0, 0, 0]) == 4096 and int(conf.sum()) == 4096 and int(skipped[0]) == 0
    # C = 64: the 4 096 pixels hit each of the 4 096 cells once
    p = np.arange(4096).reshape(64, 64)
    logits = np.zeros((1, 64, 64, 64), dtype=np.float32)
    np.put_along_axis(logits[0], (p % 64)[..., None], 1.0, axis=-1)
    conf, skipped, label = _check(logits, (p // 64)[None].astype(np.int64), 64)
    assert bool((conf == 1).all()) and int(skipped[0]) == 0


def _raw(L, logits, target, F, H, W, ld, C, label, conf, skipped):
    from densefusion_amd import _lib
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    return L.df_seg_score(ptr(logits), ptr(target), F, H, W, ld, C, ptr(label), ptr(conf), ptr(skipped), _lib.current_stream())


def test_label_out_is_optional_and_argument_errors_write_nothing():
    _dev()
    from densefusion_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(3)
    F, H, W, C, ld = 2, 5, 7, 5, 8
    logits = ssn.tie_logits(rng, F, H, W, C, ld)
    target, _ = _targets(rng, F, H, W, C)
    d_logits, d_target = _up(logits), _up(target)
    fill = lambda *s: torch.full(s, 7, dtype=torch.int32, device="cuda")
    label, conf, skipped = fill(F, H, W), fill(F, C, C), fill(F)
    good = dict(logits=d_logits, target=d_target, F=F, H=H, W=W, ld=ld, C=C, label=label, conf=conf, skipped=skipped)
    call = lambda **kw: _raw(L, **dict(good, **kw))
    cases = [dict(logits=None), dict(target=None), dict(conf=None), dict(skipped=None), dict(F=0), dict(F=65536), dict(H=0), dict(W=0),
             dict(H=1 << 16, W=(1 << 14) + 1), dict(C=1), dict(C=65, ld=68), dict(C=9), dict(ld=6), dict(ld=68), dict(ld=4),
             dict(logits=d_logits.data_ptr() + 4), dict(target=d_target.data_ptr() + 4), dict(label=label.data_ptr() + 2),
             dict(conf=conf.data_ptr() + 2), dict(skipped=skipped.data_ptr() + 2)]
    for kw in cases:
        assert call(**kw) == -1 and L.df_last_error(), kw
    torch.cuda.synchronize()
    assert bool((label == 7).all()) and bool((conf == 7).all()) and bool((skipped == 7).all())
    want = ssn.seg_score(logits, target, C)
    conf0, skipped0 = fill(F, C, C), fill(F)
    assert call(label=None, conf=conf0, skipped=skipped0) == 0                # label_out NULL: the same conf, and the call clears it
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(conf0, conf) and torch.equal(skipped0, skipped)
    for g, w in zip((conf, skipped, label), want):
        assert np.array_equal(g.cpu().numpy(), w)


# ---- df_seg_masks ----------------------------------------------------------------------------------------------------------------------
def _masks(label, win, pairs, dims):
    from densefusion_amd.lib import segment_score as ss
    got = ss.seg_masks(_up(label), win, pairs, dims)
    want = ssn.seg_masks(label, win, pairs, dims)
    g = got.cpu().view(torch.int16).numpy().view(np.uint16)
    assert g.shape == want.shape and np.array_equal(g, want)
    return got, want


def test_masks_equal_the_restatement_and_feed_the_item_table():
    _dev()
    from densefusion_amd import _lib
    from densefusion_amd.lib import preprocess as pp
    rng = np.random.default_rng(12)
    label = rng.integers(0, 3, (3, 32, 64)).astype(np.int32)
    label[:, 5:25, 10:50] = np.array([1, 2, 1])[:, None, None]                # a body per frame, noise around it
    label[2][label[2] == 2] = 0                                               # class 2 is absent from frame 2
    win = [[0, 0], [8, 8], [4, 3]]
    pairs = [[0, 1], [1, 2], [1, 2], [2, 2], [2, 1], [0, 0], [1, 64]]          # a repeated pair, an absent class, the background, class 64
    got, want = _masks(label, win, pairs, (40, 72))
    assert np.array_equal(want[1], want[2]) and not want[3].any() and not want[6].any() and want[0].any()
    assert not want[1][:8].any() and not want[1][:, :8].any(), "nothing outside the window"
    # the caller clears nothing: a pre-filled output comes back 0 outside the window
    L = _lib.lib()
    out = torch.full((len(pairs), 40, 72), -1, dtype=torch.int16, device="cuda")
    w32, p32 = np.ascontiguousarray(win, dtype=np.int32), np.ascontiguousarray(pairs, dtype=np.int32)
    d_label = _up(label)
    good = dict(label=d_label.data_ptr(), F=3, H=32, W=64, win=w32.ctypes.data, pairs=p32.ctypes.data, N=len(pairs), IH=40, IW=72,
                out=out.data_ptr())
    args = lambda **kw: [dict(good, **kw)[k] for k in good]
    bad_win, bad_pair, bad_cls = np.array([[0, 0], [9, 8], [4, 3]], dtype=np.int32), p32.copy(), p32.copy()
    bad_pair[3, 0], bad_cls[0, 1] = 3, 65
    for kw in (dict(label=None), dict(win=None), dict(pairs=None), dict(out=None), dict(F=0), dict(N=0), dict(IH=0), dict(IW=0), dict(H=41),
               dict(W=73), dict(H=0), dict(win=bad_win.ctypes.data), dict(pairs=bad_pair.ctypes.data), dict(pairs=bad_cls.ctypes.data),
               dict(out=out.data_ptr() + 1)):
        assert L.df_seg_masks(*args(**kw), _lib.current_stream()) == -1 and L.df_last_error(), kw
    torch.cuda.synchronize()
    assert bool((out == -1).all()), "an argument error writes nothing"
    assert L.df_seg_masks(*args(), _lib.current_stream()) == 0
    assert np.array_equal(out.cpu().numpy().view(np.uint16), want)
    # a 32 x 32 window equal to the frame
    sq = rng.integers(0, 4, (1, 32, 32)).astype(np.int32)
    _masks(sq, [[0, 0]], [[0, 3], [0, 0]], (32, 32))
    # what df_cad_item_table reads: the table over the device masks equals the table over the numpy masks
    depth = torch.from_numpy(rng.integers(1, 3000, (len(pairs), 40, 72)).astype(np.int16)).cuda().view(torch.uint16)
    t_got = pp.cad_item_table(depth, got, 65535, 8)
    t_want = pp.cad_item_table(depth, torch.from_numpy(want.view(np.int16)).cuda().view(torch.uint16), 65535, 8)
    assert torch.equal(t_got, t_want) and int(t_got[0, 7]) == 1 and int(t_got[3, 7]) == 0, t_got.tolist()


def test_more_pairs_than_one_launch_holds():
    _dev()
    rng = np.random.default_rng(4)
    label = rng.integers(0, 3, (2, 4, 6)).astype(np.int32)
    pairs = [[n % 2, n % 3] for n in range(131)]                              # 128 pairs travel per launch
    _masks(label, [[1, 2], [0, 0]], pairs, (5, 9))
