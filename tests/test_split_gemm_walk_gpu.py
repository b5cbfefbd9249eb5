"""GPU: the tile walk of the split GEMM's 256 x 256 form changes no bit, however few workgroups walk the tiles.

In that form one workgroup walks many output tiles (csrc/split_gemm.hip: split_walk_next); between two tiles it issues the next tile's first
fetches ahead of the finished tile's epilogue, leaves the output stores in flight and reuses the LDS stages behind one workgroup barrier.
Per output element nothing moves, so every launch must equal the 128 x 128 first form (DF_GEMM_SPLIT_V=1: one tile per workgroup, no walk)
bit for bit: outputs and column-sum partials are compared by SHA-256 of their raw bytes.  DF_GEMM_SPLIT_WGS (development library, read once
per process: each setting runs in a child process) limits the workgroups of a launch: with 8 every workgroup walks 32 or more tiles, so each
hand-over (prefetch, barrier, LDS reuse, stores in flight) happens hundreds of times per case; 24 and 64 give strides that do not divide the
sequence; the default is the product's launch, one workgroup per compute unit.

Cases (df_gemm_rows, DF_GEMM_SPLIT_BF16=1: weights cut per launch): the smallest shapes that still reach the 256 x 256 form on 256 compute
units, at least 256 tiles each:
  * N = 256, K = 384, M = 65 536 - 37: a ragged last row tile;
  * N = 512, K = 416, M = 33 000: 129 row tiles (padding positions: not a multiple of 8), K / 16 even, the loads' tail clamps;
  * zcount = 3, M = 22 000, N = 256: 86 row tiles per plane, the walk crosses plane boundaries;
  * residual + ReLU, N = 256, K = 448, M = 65 536 + 5: 257 row tiles;
  * per-group bias (rows_per_group 1 024, rows_valid 1 000) with fused column sums and NO output buffer, N = 512, M = 33 x 1 024."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SWITCHES = ("DF_GEMM_SPLIT_OFF", "DF_GEMM_SPLIT_BF16", "DF_GEMM_SPLIT_V", "DF_GEMM_SPLIT_VERBOSE", "DF_GEMM_SPLIT_WGS", "DF_DEV_LIB")
_CASES = ("ragged", "k416", "z3", "residual", "groups_colsum")

_CHILD = r"""
import hashlib, json, torch
from densefusion_amd import _lib
L, dev = _lib.lib(), torch.device("cuda")
sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
ptr = lambda t: None if t is None else t.data_ptr()
def run(name, M, N, K, z=1, act=0, res=False, groups=0, valid=0, bias_ld=0, out=True):
    torch.manual_seed(M + 3 * N + 7 * K + z)
    x = torch.randn(z, M, K, device=dev)
    w = torch.randn(z, N, K, device=dev) / K ** 0.5
    b = torch.randn(M // groups, bias_ld, device=dev) if groups else torch.randn(z, N, device=dev)
    r = torch.randn(M, N, device=dev) if res else None
    y = torch.full((z, M, N), float("nan"), device=dev) if out else None
    cs = torch.full((z, 2 * ((M + 127) // 128), N), float("nan"), device=dev) if groups else None
    _lib.check(L.df_gemm_rows(ptr(x), ptr(w), ptr(b), ptr(r), ptr(y), ptr(cs), M, N, K, z, act, groups, valid, bias_ld, _lib.current_stream()), name)
    torch.cuda.synchronize()
    got = {"case": name}
    for key, t in (("out", y), ("colsum", cs)):
        if t is not None:
            assert bool(torch.isfinite(t).all()), (name, key)
            got[key] = sha(t)
            got[key + "_absmax"] = float(t.abs().max())
    return got
print(json.dumps([run("ragged", 65536 - 37, 256, 384, act=1),
                  run("k416", 33000, 512, 416),
                  run("z3", 22000, 256, 384, z=3, act=1),
                  run("residual", 65536 + 5, 256, 448, act=1, res=True),
                  run("groups_colsum", 33 * 1024, 512, 384, act=1, groups=1024, valid=1000, bias_ld=640, out=False)]))
"""


def _child(env_extra, timeout=300):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if not os.path.exists(os.path.join(ROOT, "densefusion_amd", "libdfusion_hip_dev.so")):
        pytest.skip("development library not built")
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in _SWITCHES:
        env.pop(k, None)
    env.update({"DF_DEV_LIB": "1", "DF_GEMM_SPLIT_BF16": "1", "DF_GEMM_SPLIT_VERBOSE": "1"}, **env_extra)
    out = subprocess.run([sys.executable, "-c", _CHILD], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    launches = []          # (form, workgroups) per launch
    for line in out.stderr.splitlines():
        if line.startswith("[df-split]   form "):
            launches.append([line.split()[-1], None])
        elif line.startswith("[df-split]   workgroups "):
            launches[-1][1] = int(line.split()[-1])
    return json.loads(out.stdout.strip().splitlines()[-1]), launches


@pytest.fixture(scope="module")
def witness():
    res, launches = _child({"DF_GEMM_SPLIT_V": "1"})
    assert [c["case"] for c in res] == list(_CASES)
    assert [f for f, _ in launches] == ["128x128"] * len(_CASES), launches
    return res


def _positions(M, N, z=1):
    return ((M + 255) // 256 + 7) // 8 * 8 * (N // 256) * z


_POSITIONS = [_positions(65536 - 37, 256), _positions(33000, 512), _positions(22000, 256, 3), _positions(65536 + 5, 256), _positions(33 * 1024, 512)]


@pytest.mark.parametrize("wgs", ["8", "24", "64", None])
def test_walked_tiles_equal_the_first_form_bit_for_bit(witness, wgs):
    import torch
    res, launches = _child({} if wgs is None else {"DF_GEMM_SPLIT_WGS": wgs})
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    print("launches:", launches)
    assert [f for f, _ in launches] == ["256x256"] * len(_CASES), launches                       # every case reached the form under test
    want = [min(max(8, (cu if wgs is None else int(wgs)) // 8 * 8), p) for p in _POSITIONS]
    assert [n for _, n in launches] == want, (launches, want)
    if wgs == "8":
        assert all(p // 8 >= 32 for p in _POSITIONS)                                                # 32 or more tiles per workgroup
    for new, old in zip(res, witness):
        print(new["case"], {k: (v[:16] if isinstance(v, str) else v) for k, v in new.items()})
        assert new["case"] == old["case"]
    bad = [(n["case"], k) for n, o in zip(res, witness) for k in ("out", "colsum") if n.get(k) != o.get(k)]
    assert not bad, bad
    assert "colsum" in res[-1] and "out" not in res[-1] and all("out" in r for r in res[:-1])
