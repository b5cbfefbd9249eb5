"""CPU: the numpy restatement of ``df_seg_score`` / ``df_seg_masks`` (tests/seg_score_np.py) in its two forms, the identities a confusion
matrix obeys, ``metrics_from_confusion`` on hand-made matrices, and the wrappers' argument rules, which use host integers only."""
import numpy as np
import pytest

import seg_score_np as ssn


def _case(seed, F, H, W, C, ld):
    rng = np.random.default_rng(seed)
    logits = ssn.tie_logits(rng, F, H, W, C, ld)
    target = rng.integers(0, C, (F, H, W)).astype(np.int64)
    bad = rng.choice(F * H * W, size=min(4, F * H * W // 2), replace=False)
    target.reshape(-1)[bad] = np.array([-1, C, 255, 2 ** 40])[:len(bad)]
    return logits, target


@pytest.mark.parametrize("shape", [(1, 1, 3, 2, 4), (2, 5, 7, 3, 4), (1, 5, 7, 22, 24), (3, 4, 6, 5, 8)])
def test_the_two_forms_agree_and_the_sums_hold(shape):
    F, H, W, C, ld = shape
    logits, target = _case(sum(shape), *shape)
    a, b = ssn.seg_score(logits, target, C), ssn.seg_score_pixels(logits, target, C)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    conf, skipped, label = a
    assert label.max() < C, "a pad channel never wins"
    ok = (target >= 0) & (target < C)
    for f in range(F):
        assert np.array_equal(conf[f].sum(axis=1), np.bincount(target[f][ok[f]], minlength=C))          # rows: the truth's counts
        assert np.array_equal(conf[f].sum(axis=0), np.bincount(label[f][ok[f]], minlength=C))           # columns: the prediction's
        assert int(conf[f].sum()) + int(skipped[f]) == H * W
    assert int(skipped.sum()) == int((~ok).sum()) > 0
    nan = np.isnan(logits[..., :C]).any(axis=-1)                                                         # NaN is maximal, the first one wins
    assert nan.sum() >= 1 and np.array_equal(label[nan], np.isnan(logits[..., :C][nan]).argmax(axis=-1))


def test_masks_forms_agree():
    rng = np.random.default_rng(2)
    label = rng.integers(0, 4, (3, 4, 6)).astype(np.int32)
    win, pairs = [[0, 0], [2, 3], [1, 1]], [[0, 1], [1, 2], [1, 2], [2, 7], [2, 0]]
    a, b = ssn.seg_masks(label, win, pairs, (6, 9)), ssn.seg_masks_pixels(label, win, pairs, (6, 9))
    assert a.dtype == np.uint16 and np.array_equal(a, b)
    assert np.array_equal(a[1], a[2]) and not a[3].any() and set(np.unique(a)) <= {0, 65535}
    assert int((a[1] != 0).sum()) == int((label[1] == 2).sum()) and not a[1][:2].any() and not a[1][:, :3].any()


def test_metrics_from_confusion_on_hand_made_matrices():
    from densefusion_amd.lib.segment_score import metrics_from_confusion
    m = metrics_from_confusion(np.diag([5, 3, 2]).astype(np.int64))                                      # perfect
    for k in ("iou", "precision", "recall"):
        assert m[k].dtype == np.float64 and m[k].tolist() == [1.0, 1.0, 1.0]
    assert m["miou"] == 1.0 and m["pixel_accuracy"] == 1.0 and m["pixels"] == 10
    # class 2 has neither a truth nor a predicted pixel: nan, and left out of the mean
    m = metrics_from_confusion(np.array([[6, 2, 0], [1, 3, 0], [0, 0, 0]], dtype=np.int64))
    assert m["iou"][:2].tolist() == [6 / 9, 3 / 6] and np.isnan(m["iou"][2])
    assert m["precision"][:2].tolist() == [6 / 7, 3 / 5] and np.isnan(m["precision"][2])
    assert m["recall"][:2].tolist() == [6 / 8, 3 / 4] and np.isnan(m["recall"][2])
    assert m["miou"] == (6 / 9 + 3 / 6) / 2 and m["pixel_accuracy"] == 9 / 12
    # all truth in class 1, all predictions in class 0: IoU 0 for both, neither is nan
    m = metrics_from_confusion(np.array([[0, 0], [7, 0]], dtype=np.int64))
    assert m["iou"].tolist() == [0.0, 0.0] and m["miou"] == 0.0 and m["pixel_accuracy"] == 0.0
    assert m["precision"][0] == 0.0 and np.isnan(m["precision"][1]) and np.isnan(m["recall"][0]) and m["recall"][1] == 0.0
    m = metrics_from_confusion(np.zeros((2, 2), dtype=np.int32))                                          # nothing scored
    assert np.isnan(m["miou"]) and np.isnan(m["pixel_accuracy"]) and np.isnan(m["iou"]).all()
    big = np.array([[2 ** 40, 1], [0, 2 ** 40]], dtype=np.int64)                                          # int64 in: no 32-bit sum inside
    assert metrics_from_confusion(big)["pixels"] == 2 ** 41 + 1
    for bad in (np.zeros((2, 3), dtype=np.int64), np.zeros((2, 2), dtype=np.float64), np.zeros(4, dtype=np.int64)):
        with pytest.raises(ValueError):
            metrics_from_confusion(bad)


def test_wrapper_argument_rules_use_host_integers_only():
    from densefusion_amd.lib import segment_score as ss
    assert ss.check_classes(2, 4) == (2, 4) and ss.check_classes(64, 64) == (64, 64) and ss.check_classes(22, 24) == (22, 24)
    for C, ld in ((1, 4), (65, 68), (5, 4), (3, 6), (3, 68), (0, 0)):
        with pytest.raises(ValueError):
            ss.check_classes(C, ld)
    win, pairs = ss.check_masks_args(2, (32, 64), [[0, 0], [8, 8]], [[0, 1], [1, 64], [1, 0]], (40, 72))
    assert win.dtype == np.int32 and pairs.dtype == np.int32 and win.flags.c_contiguous and pairs.shape == (3, 2)
    for kw in (dict(win=[[0, 0], [9, 8]]), dict(win=[[0, 0], [8, 9]]), dict(win=[[-1, 0], [0, 0]]), dict(win=[[0, 0]]),
               dict(pairs=[[2, 1]]), dict(pairs=[[-1, 1]]), dict(pairs=[[0, 65]]), dict(pairs=[[0, -1]]), dict(pairs=[]),
               dict(window=(41, 64)), dict(window=(32, 0))):
        args = dict(dict(F=2, window=(32, 64), win=[[0, 0], [8, 8]], pairs=[[0, 1]], image_dims=(40, 72)), **kw)
        with pytest.raises(ValueError):
            ss.check_masks_args(**args)
    with pytest.raises(RuntimeError):                                          # no CPU path: a host tensor is refused before any call
        ss.seg_score(np.zeros((1, 2, 2, 4), dtype=np.float32), np.zeros((1, 2, 2), dtype=np.int64), 3)
    with pytest.raises(RuntimeError):
        ss.seg_masks(np.zeros((1, 2, 2), dtype=np.int32), [[0, 0]], [[0, 1]], (4, 4))
    with pytest.raises(ValueError):
        ss.SegScore(1, device="cpu")
