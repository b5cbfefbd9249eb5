"""GPU: the F(4x4,3x3) transforms on the packed axis layout (csrc/wino.h: the sub-lattices of a dilated axis one after another in one
strip, one zero position between neighbours) against an fp64 convolution, against the padded layout, and through the engine.

The bounds are those tests/test_conv_gpu.py applies to tile 4: 2e-5 of the output scale, and 60 x the direct kernel's error + 1e-7.  A wrong
neighbour or a separator that is not zero gives errors of order 1."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, H, W, Cin, Cout, dil) -> (H packed, W packed)
SHAPES = {
    (2, 20, 15, 16, 8, 4): (1, 0),      # H packed only
    (1, 15, 20, 8, 16, 4): (0, 1),      # W packed only
    (3, 20, 25, 8, 8, 4): (1, 1),       # both, unequal sub-lattices on W (7, 6, 6, 6 points)
    (1, 5, 7, 8, 8, 4): (1, 1),         # sub-lattices of 1 to 2 points
    (2, 3, 2, 8, 8, 4): (1, 1),         # L < d: empty residues
    (1, 10, 25, 16, 16, 2): (1, 1),     # dilation 2
    (2, 9, 11, 8, 12, 2): (1, 1),       # dilation 2, unequal sub-lattices
    (1, 40, 30, 8, 8, 4): (1, 0),       # 11 tiles in one strip against 4 strips of 3; W padded
    (1, 15, 30, 8, 8, 4): (0, 0),       # no packed axis
}
UNPACKED = [(1, 15, 30, 8, 8, 4), (2, 12, 9, 8, 8, 1)]


def _modes(L, geom):
    B, H, W, _, _, dil = geom
    py, px = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.df_wino_tiles(B, H, W, dil, 4, ctypes.byref(py), ctypes.byref(px)) > 0
    return py.value, px.value


def _errors(geom, fused):
    """(Winograd tile 4 error, direct kernel error) against fp64, relative to the output scale; and the Winograd output"""
    from densefusion_amd import ops
    import torch.nn.functional as F
    B, H, W, Cin, Cout, dil = geom
    dev = torch.device("cuda:0")
    torch.manual_seed(sum(geom))
    x = (torch.relu(torch.randn(B, H, W, Cin)) * 3).to(dev)
    w = (torch.randn(Cout, 3, 3, Cin) * (2.0 / (9 * Cin)) ** 0.5).to(dev)
    bias = torch.randn(Cout, device=dev) if fused else None
    res = torch.randn(B, H, W, Cout, device=dev) if fused else None
    act = 1 if fused else 0
    want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), bias.double() if fused else None, 1, dil, dil)
    want = want.permute(0, 2, 3, 1)
    if fused:
        want = torch.relu(want + res.double())
    got_w = ops.conv3x3_winograd_nhwc(x, w, bias, dil=dil, act=act, res=res, tile=4)
    got_d = ops.conv2d_nhwc(x, w, bias, stride=1, pad=dil, dil=dil, act=act, res=res)
    scale = float(want.abs().max())
    return float((got_w.double() - want).abs().max()) / scale, float((got_d.double() - want).abs().max()) / scale, got_w


def _hold(err_w, err_d, what):
    print(what, "winograd", err_w, "direct", err_d)
    assert err_w < 2e-5, (what, err_w, err_d)
    assert err_w < 60 * err_d + 1e-7, (what, err_w, err_d)


@pytest.mark.parametrize("geom", list(SHAPES))
@pytest.mark.parametrize("fused", [False, True])
def test_packed_tiles_match_fp64(geom, fused):
    from densefusion_amd import _lib
    assert _modes(_lib.lib(), geom) == SHAPES[geom]
    err_w, err_d, _ = _errors(geom, fused)
    _hold(err_w, err_d, (geom, fused))


_CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, %r)
from densefusion_amd import _lib
from test_wino_packed_gpu import SHAPES, UNPACKED, _errors, _modes
out = []
for geom in list(SHAPES) + [g for g in UNPACKED if g not in SHAPES]:
    for fused in (False, True):
        err_w, err_d, y = _errors(geom, fused)
        out.append({"geom": list(geom), "fused": fused, "modes": list(_modes(_lib.lib(), geom)), "err_w": err_w, "err_d": err_d,
                    "sha": hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()})
print(json.dumps(out))
"""


def _child(env_extra):
    if not os.path.exists(os.path.join(ROOT, "densefusion_amd", "libdfusion_hip_dev.so")):
        pytest.skip("development library not built")
    env = dict(os.environ, PYTHONPATH=ROOT, DF_DEV_LIB="1")
    env.pop("DF_WINO_PADDED", None)
    env.update(env_extra)
    out = subprocess.run([sys.executable, "-c", _CHILD % os.path.join(ROOT, "tests")], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_padded_switch_keeps_unpacked_shapes_bit_identical_and_packed_ones_within_bounds():
    """DF_WINO_PADDED (development library; read once, so each side is a child process) puts every axis on the padded layout.  A shape with
    no packed axis runs the same tiles either way: equal bits.  A packed shape holds the fp64 bounds on both layouts."""
    packed, padded = _child({}), _child({"DF_WINO_PADDED": "1"})
    assert len(packed) == len(padded) == 2 * (len(SHAPES) + 1)
    n_equal = 0
    for a, b in zip(packed, padded):
        geom = tuple(a["geom"])
        assert a["geom"] == b["geom"] and a["fused"] == b["fused"]
        assert b["modes"] == [0, 0], b                                  # the switch took
        assert tuple(a["modes"]) == SHAPES.get(geom, (0, 0)), a
        _hold(a["err_w"], a["err_d"], ("packed build", geom, a["fused"]))
        _hold(b["err_w"], b["err_d"], ("padded switch", geom, b["fused"]))
        if a["modes"] == [0, 0]:
            assert geom in UNPACKED
            assert a["sha"] == b["sha"], geom
            n_equal += 1
    assert n_equal == 2 * len(UNPACKED)


def test_engine_buckets_on_packed_tiles_equal_solo_runs_bit_for_bit():
    """PoseNet forward over two buckets, 3 crops of 160 x 200 (20 x 25 maps: both axes of layer4.1 packed, W of layer3.1 packed) and 3 of
    80 x 80, in one multi-bucket pass == the six one-object forwards, bit for bit: the layout is a function of the map, never of the batch
    or of the buckets that share the launch."""
    from densefusion_amd import _lib, synth
    from densefusion_amd.lib.network import PoseNet
    L = _lib.lib()
    assert L.df_wino_route(20, 25, 4, 512, 512) == 4 and _modes(L, (3, 20, 25, 512, 512, 4)) == (1, 1)
    assert L.df_wino_route(20, 25, 2, 256, 256) == 4 and _modes(L, (3, 20, 25, 256, 256, 2)) == (0, 1)
    K, N = 21, 1000
    est = PoseNet(N, K)
    est.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(synth.posenet_spec(K), 13).items()}, strict=True)
    est = est.cuda().eval()
    shapes = [(3, 160, 200), (3, 80, 80)]
    bs = [synth.make_batch(900 + i, B, H, W, N, K) for i, (B, H, W) in enumerate(shapes)]
    T = lambda b, k: torch.from_numpy(b[k]).cuda()
    cat = lambda k: torch.cat([T(b, k) for b in bs])
    outs = est.forward_multi([T(b, "img") for b in bs], cat("cloud"), cat("choose"), cat("obj"))
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    o = 0
    for b, (B, H, W) in zip(bs, shapes):
        batched = est(T(b, "img"), T(b, "cloud"), T(b, "choose"), T(b, "obj"))
        for a, m in zip(batched, outs):
            assert torch.equal(a, m[o:o + B]), (H, W)
        for i in range(B):
            solo = est(*[T(b, k)[i:i + 1] for k in ("img", "cloud", "choose", "obj")])
            for a, m in zip(solo, outs):
                assert torch.equal(a[0], m[o + i]), (H, W, i)
        o += B
