"""GEMM time of the bench step by kernel (GPU box): the serial, un-graphed step of bench.py's workload with HIP events around every GEMM
launch (df_net_profile), the fp32-MFMA launches and the bf16 x 6 split-precision launches (df_gemm_route) summed apart.  Prints one JSON
line per step average:
  fp32:  ms, TFLOP/s against the fp32-MFMA peak (the kernel bench.py's roofline object describes)
  split: ms, fp32-equivalent TFLOP/s (2 M N K per launch), and the share of the bf16-pipe ceiling (6 x 2 M N K of bf16 MFMA work against
         the dense bf16 peak)
  all:   ms and fp32-equivalent TFLOP/s of every GEMM launch
    python tools/split_roofline.py [--steps 3]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402  (its workload: nets, buckets, groups, one step)
from densefusion_amd import _lib  # noqa: E402
from densefusion_amd.lib.network import PoseEstimator  # noqa: E402

BF16_PEAK_TFLOPS = 2516.8     # MI355X_MICROARCH.md: dense bf16 MFMA (v_mfma_f32_32x32x16_bf16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--per-bucket", type=int, default=40)
    args = ap.parse_args()
    dev = torch.device("cuda")
    est, ref = bench.load_nets(dev)
    buckets = bench.make_buckets(0, 1, args.per_bucket, dev)
    groups = bench.make_groups(buckets, 1, dev)
    pe = [PoseEstimator(est, ref)]
    bench.run_step(pe, groups)                      # warm-up: workspaces, weight planes
    torch.cuda.synchronize()
    L = _lib.lib()
    hs = (pe[0].estimator._handle, pe[0].refiner._handle)
    for h in hs:
        _lib.check(L.df_net_profile(h, 1), "profile")
    f32 = [0.0, 0.0, 0]
    spl = [0.0, 0.0, 0]
    for _ in range(args.steps):
        bench.run_step(pe, groups)
        torch.cuda.synchronize()
        for h in hs:
            ms, fl, us, by, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
            _lib.check(L.df_net_profile_read_split(h, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(us), ctypes.byref(n)), "profile_read_split")
            spl[0] += ms.value; spl[1] += fl.value; spl[2] += n.value
            _lib.check(L.df_net_profile_read(h, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(us), ctypes.byref(by), ctypes.byref(n)), "profile_read")
            f32[0] += ms.value; f32[1] += fl.value; f32[2] += n.value
    for h in hs:
        L.df_net_profile(h, 0)
    s = args.steps
    tf = lambda fl, ms: fl / ms / 1e9 if ms > 0 else 0.0
    out = {
        "steps": s, "poses_per_step": sum(b["img"].shape[0] for b in buckets),
        "fp32": {"kernel": "igemm_f32_v4 (v_mfma_f32_32x32x2_f32)", "gemm_ms_per_step": round(f32[0] / s, 3), "launches_per_step": f32[2] // s,
                 "tflops": round(tf(f32[1], f32[0]), 1), "frac_of_fp32_peak": round(tf(f32[1], f32[0]) / bench.FP32_PEAK_TFLOPS, 4)},
        "split": {"kernel": "gemm_split_bf16 (6 x v_mfma_f32_32x32x16_bf16)", "gemm_ms_per_step": round(spl[0] / s, 3), "launches_per_step": spl[2] // s,
                  "tflops_fp32_equivalent": round(tf(spl[1], spl[0]), 1),
                  "frac_of_bf16_ceiling": round(6 * tf(spl[1], spl[0]) / BF16_PEAK_TFLOPS, 4)},
        "all": {"gemm_ms_per_step": round((f32[0] + spl[0]) / s, 3), "tflops_fp32_equivalent": round(tf(f32[1] + spl[1], f32[0] + spl[0]), 1)},
    }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
