"""GPU: the bf16 x 6 split-precision GEMM (csrc/split_gemm.hip) as the inference engine's default for its routed layers.

* products at every routed engine shape, small and ragged M, each epilogue kind: error against fp64 within 1.25x the fp32-MFMA kernel's own
  error on the same operands, and bit-identical over repeats;
* the engine's PoseNet outputs and poses with the split kernel and with every launch on fp32 (development library, DF_GEMM_SPLIT_OFF=1)
  agree to fp32 rounding, and the development library without switches computes exactly what the product library computes.
Development switches are read once per process, so every variant runs in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if not os.path.exists(os.path.join(ROOT, "densefusion_amd", "libdfusion_hip_dev.so")):
        pytest.skip("development library not built")


def _child(code, env_extra, timeout=300):
    env = dict(os.environ, PYTHONPATH=ROOT, **env_extra)
    for k in ("DF_GEMM_SPLIT_OFF", "DF_GEMM_SPLIT_BF16"):
        if k not in env_extra:
            env.pop(k, None)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


# the routed engine shapes (N, K) with the epilogue each runs with in the engine, plus the other kinds on the largest one
_PRODUCTS = r"""
import json, torch
from densefusion_amd import ops
dev = torch.device("cuda")
res = []
for N, K, M, kind in ((1024, 512, 36 * 7, "plain"), (1024, 512, 4801, "residual"), (2304, 1024, 1337, "plain"), (512, 512, 3 * 129, "plain"),
                      (1920, 384, 1000, "relu"), (640, 384, 255, "relu"), (256, 640, 3001, "relu"), (1024, 512, 1024 * 2 + 77, "relu"),
                      (2304, 1024, 513, "prelu"), (2304, 1024, 700, "residual")):
    g = torch.Generator().manual_seed(N * 7 + K + M)
    x = torch.randn(M, K, generator=g).abs_().to(dev)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    r = torch.randn(M, N, generator=g).to(dev) if kind == "residual" else None
    pr = torch.tensor([0.25], device=dev) if kind == "prelu" else None
    act = {"plain": 0, "residual": 1, "relu": 1, "prelu": 2}[kind]
    outs = []
    for _ in range(3):
        y = ops.conv2d_nhwc(x.view(1, M, 1, K), w.view(N, 1, 1, K), bias=b, act=act, res=None if r is None else r.view(1, M, 1, N), prelu=pr)
        outs.append(y.view(M, N).clone())
    torch.cuda.synchronize()
    same = all(torch.equal(outs[0], o) for o in outs[1:])
    ref = x.double() @ w.double().t() + b.double()
    if r is not None: ref = ref + r.double()
    if act == 1: ref = torch.relu(ref)
    if act == 2: ref = torch.where(ref > 0, ref, 0.25 * ref)
    res.append({"shape": [M, N, K, kind], "err": float((outs[0].double() - ref).abs().max() / ref.abs().max()), "repeat_identical": same})
print(json.dumps(res))
"""


def test_routed_shapes_stay_inside_the_fp32_kernels_error_and_repeat_bit_for_bit():
    _need_gpu()
    split = _child(_PRODUCTS, {"DF_DEV_LIB": "1", "DF_GEMM_SPLIT_BF16": "1"})
    fp32 = _child(_PRODUCTS, {"DF_DEV_LIB": "1", "DF_GEMM_SPLIT_OFF": "1"})
    print("\n".join(f"{s['shape']}: split {s['err']:.2e}  fp32 {f['err']:.2e}" for s, f in zip(split, fp32)))
    for s, f in zip(split, fp32):
        assert s["repeat_identical"] and f["repeat_identical"], s
        assert s["err"] <= 1.25 * f["err"], (s, f)
        assert s["err"] < 2e-6, s


_ENGINE = r"""
import json, sys, numpy as np, torch
from densefusion_amd import synth
from densefusion_amd.lib.network import PoseEstimator, PoseNet, PoseRefineNet
K, N, H, W = 3, 1000, 120, 160
sdp, sdr = synth.make_state_dict(synth.posenet_spec(K), 21), synth.make_state_dict(synth.refiner_spec(K), 1021)
est, rfn = PoseNet(N, K), PoseRefineNet(N, K)
est.load_state_dict({k: torch.from_numpy(v) for k, v in sdp.items()})
rfn.load_state_dict({k: torch.from_numpy(v) for k, v in sdr.items()})
est, rfn = est.cuda().eval(), rfn.cuda().eval()
res = {}
for seed in (5, 6):
    o = synth.make_object(seed, H, W, N, K)
    img, cloud, choose, obj = [torch.from_numpy(o[k]).cuda() for k in ("img", "cloud", "choose", "obj")]
    with torch.no_grad():
        pr, pt, pc, emb = est(img[None], cloud[None], choose[None], obj[None])[:4]
        _, pose = PoseEstimator(est, rfn).estimate(img[None], cloud[None], choose[None], obj[None], 2)
    res[seed] = {"pred_r": pr.cpu().numpy().ravel().tolist(), "pred_t": pt.cpu().numpy().ravel().tolist(),
                 "pred_c": pc.cpu().numpy().ravel().tolist(), "pose": pose.cpu().numpy().ravel().tolist()}
print(json.dumps(res))
"""


def test_engine_outputs_agree_with_the_all_fp32_path_and_the_dev_library_routes_like_the_product():
    _need_gpu()
    prod = _child(_ENGINE, {})
    dev = _child(_ENGINE, {"DF_DEV_LIB": "1"})
    fp32 = _child(_ENGINE, {"DF_DEV_LIB": "1", "DF_GEMM_SPLIT_OFF": "1"})
    for seed in prod:
        for k in prod[seed]:
            a, b, c = (np.asarray(d[seed][k]) for d in (prod, dev, fp32))
            assert np.array_equal(a, b), (seed, k)                   # no switch: the development library routes as the product does
            scale = max(np.abs(c).max(), 1e-3)
            assert np.abs(a - c).max() <= 2e-5 * scale, (seed, k, float(np.abs(a - c).max()), scale)
