"""GPU: every tile form of the bf16 x 6 split GEMM (csrc/split_gemm.hip) computes the same bits.

Per output element all forms add the same products in the same order (k16 groups in ascending k, the six term pairs in one fixed order, then
bias, residual, activation), so whichever form the launcher picks must equal the 128 x 128 first form exactly.  (Equal forms can be equally
wrong: one entry of the shared pair table moves all three.  WHICH pairs are summed, and the k loops' odd step counts and tails, are pinned by
tests/test_split_gemm_exact_gpu.py against the exact six-pair sum.)  The first form is the witness:
DF_GEMM_SPLIT_V=1 (development library) keeps every launch on it.  The switches are read once per process, so each side runs in a child process;
the children return SHA-256 digests of the raw output bytes (equal digests = equal bits, NaN payloads and signed zeros included).

Launch kinds reached (DF_GEMM_SPLIT_VERBOSE prints one "form" line per launch; the counts below are asserted):
* products through ops.conv2d_nhwc (DF_GEMM_SPLIT_BF16=1: weights cut per launch), zcount 1, per-channel bias, epilogues plain / ReLU / PReLU /
  residual + ReLU:  one 256-row tile (M = 200), a ragged last tile, N = 640 and N = 1920 (N % 256 = 128) -> the 256 x 128 form;  M with at
  least as many 256 x 256 tiles as the card has compute units, ragged (M % 256 != 0) and at three times the compute units -> the 256 x 256 form;
* the engine (PoseNet on a batch of 48 crops + 2 refine iterations, planes cut at parameter load): the Winograd-domain zcount > 1 batches,
  the per-group (per-object) bias launches and the launches with fused column sums, on the 256 x 256 form where the batch has the tiles for it
  and on the 256 x 128 form elsewhere (the psp fold, the refiner's small launches)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SWITCHES = ("DF_GEMM_SPLIT_OFF", "DF_GEMM_SPLIT_BF16", "DF_GEMM_SPLIT_V", "DF_GEMM_SPLIT_VERBOSE", "DF_DEV_LIB")


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if not os.path.exists(os.path.join(ROOT, "densefusion_amd", "libdfusion_hip_dev.so")):
        pytest.skip("development library not built")


def _child(code, env_extra, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in _SWITCHES:
        env.pop(k, None)
    env.update(env_extra)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    forms = {}
    for line in out.stderr.splitlines():
        if line.startswith("[df-split]   form "):
            forms[line.split()[-1]] = forms.get(line.split()[-1], 0) + 1
    return json.loads(out.stdout.strip().splitlines()[-1]), forms, out.stderr


# (N, K, M, epilogue): the routed (N, K) pairs of tests/test_split_gemm_engine_gpu.py.  cu = compute units of the card: M is chosen so that the
# launch has one tile / fewer 256 x 256 tiles than compute units (-> 256 x 128 form), or at least as many (-> 256 x 256 form)
_PRODUCTS = r"""
import hashlib, json, torch
from densefusion_amd import ops
dev = torch.device("cuda")
cu = torch.cuda.get_device_properties(0).multi_processor_count
rows = lambda N, mult=1: 256 * (-(-cu * mult // (N // 256)))          # rows of the fewest row tiles that give cu * mult 256 x 256 tiles
cases = [(1024, 512, 200, "plain"), (1024, 512, 36 * 7, "relu"), (2304, 1024, 1337, "prelu"), (512, 512, 3 * 129, "residual"),
         (640, 384, 255, "relu"), (640, 384, 256 * 70 + 3, "residual"), (1920, 384, 256 * 40 + 100, "prelu"),
         (1024, 512, rows(1024) + 77, "plain"), (1024, 512, rows(1024) - 100, "relu"), (1024, 512, rows(1024, 3) + 33, "residual"),
         (2304, 1024, rows(2304) + 13, "relu"), (2304, 1024, rows(2304) - 255, "residual"), (512, 512, rows(512) + 1, "prelu"),
         (256, 640, rows(256) + 5, "relu"), (256, 640, rows(256), "plain")]
res, keep = [], []
for N, K, M, kind in cases:
    g = torch.Generator().manual_seed(N * 7 + K + M)
    x = torch.randn(M, K, generator=g).to(dev)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    r = torch.randn(M, N, generator=g).to(dev) if kind == "residual" else None
    pr = torch.tensor([0.25], device=dev) if kind == "prelu" else None
    act = {"plain": 0, "residual": 1, "relu": 1, "prelu": 2}[kind]
    y = ops.conv2d_nhwc(x.view(1, M, 1, K), w.view(N, 1, 1, K), bias=b, act=act, res=None if r is None else r.view(1, M, 1, N), prelu=pr)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
    res.append({"case": [N, K, M, kind], "sha": hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest(), "absmax": float(y.abs().max())})
    keep.append(w)
    del x, y, r
print(json.dumps(res))
"""


def test_products_equal_the_first_form_bit_for_bit_at_every_tile_form():
    _need_gpu()
    new, forms, _ = _child(_PRODUCTS, {"DF_DEV_LIB": "1", "DF_GEMM_SPLIT_BF16": "1", "DF_GEMM_SPLIT_VERBOSE": "1"})
    old, forms_old, _ = _child(_PRODUCTS, {"DF_DEV_LIB": "1", "DF_GEMM_SPLIT_BF16": "1", "DF_GEMM_SPLIT_VERBOSE": "1", "DF_GEMM_SPLIT_V": "1"})
    print("forms:", forms, "witness:", forms_old)
    assert set(forms_old) == {"128x128"} and forms_old["128x128"] == len(old), forms_old
    assert forms.get("256x128") == 7 and forms.get("256x256") == 8, forms          # the case list's split (see _PRODUCTS)
    for n, o in zip(new, old):
        print(n["case"], n["sha"][:16], o["sha"][:16], n["absmax"])
        assert n["case"] == o["case"]
    bad = [n["case"] for n, o in zip(new, old) if n["sha"] != o["sha"]]
    assert not bad, bad


_ENGINE = r"""
import hashlib, json, numpy as np, torch
from densefusion_amd import synth
from densefusion_amd.lib.network import PoseEstimator, PoseNet, PoseRefineNet
K, N, H, W, B = 3, 1000, 120, 160, 48
sdp, sdr = synth.make_state_dict(synth.posenet_spec(K), 21), synth.make_state_dict(synth.refiner_spec(K), 1021)
est, rfn = PoseNet(N, K), PoseRefineNet(N, K)
est.load_state_dict({k: torch.from_numpy(v) for k, v in sdp.items()})
rfn.load_state_dict({k: torch.from_numpy(v) for k, v in sdr.items()})
est, rfn = est.cuda().eval(), rfn.cuda().eval()
objs = [synth.make_object(40 + i, H, W, N, K) for i in range(B)]
img, cloud, choose, obj = [torch.from_numpy(np.stack([o[k] for o in objs])).cuda() for k in ("img", "cloud", "choose", "obj")]
with torch.no_grad():
    pr, pt, pc, emb = est(img, cloud, choose, obj)[:4]
    wo, pose = PoseEstimator(est, rfn).estimate(img, cloud, choose, obj, 2)
torch.cuda.synchronize()
sha = lambda t: hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()
print(json.dumps({"pred_r": sha(pr), "pred_t": sha(pt), "pred_c": sha(pc), "emb": sha(emb), "pose_wo_refine": sha(wo), "pose": sha(pose),
                  "finite": bool(torch.isfinite(pr).all() and torch.isfinite(pose).all())}))
"""


def test_engine_outputs_equal_the_first_form_bit_for_bit():
    _need_gpu()
    new, forms, err = _child(_ENGINE, {"DF_DEV_LIB": "1", "DF_GEMM_SPLIT_VERBOSE": "1"})
    old, forms_old, _ = _child(_ENGINE, {"DF_DEV_LIB": "1", "DF_GEMM_SPLIT_VERBOSE": "1", "DF_GEMM_SPLIT_V": "1"})
    prod, _, _ = _child(_ENGINE, {})
    print("forms:", forms, "witness:", forms_old)
    lines = err.splitlines()
    zforms = {lines[i + 1].split()[-1] for i, l in enumerate(lines[:-1]) if l.startswith("[df-split] M=") and " z1 " not in l and "bf16 x 6" in l}
    print("forms of the zcount > 1 launches:", zforms)
    print("\n".join(sorted({l + lines[i + 1] for i, l in enumerate(lines[:-1]) if l.startswith("[df-split] M=") and "bf16 x 6" in l})))
    assert set(forms_old) == {"128x128"}, forms_old
    assert forms.get("256x256", 0) > 0 and forms.get("256x128", 0) > 0, forms          # both 256-row forms take part in the engine's pass
    assert "256x256" in zforms, zforms                                                 # a z batch among them
    assert new["finite"]
    assert new == old, {k: (new[k][:12], old[k][:12]) for k in new if new[k] != old[k]}
    assert new == prod                                                                 # the product library picks the forms the same way
