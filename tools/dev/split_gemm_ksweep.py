"""Dev tool (GPU box, development library): fixed cost per output tile of the bf16 x 6 split GEMM (csrc/split_gemm.hip).  Times the kernel at
fixed M and N over a sweep of K, fits  time = a + b K  by least squares and prints a (the part of a launch that does not scale with K: per-tile
prologue + epilogue, launch), b, the main-loop rate 2 M N / b (fp32-equivalent) and a's share of each K's time.
    DF_DEV_LIB=1 DF_GEMM_SPLIT_BF16=1 python tools/dev/split_gemm_ksweep.py [--m 139000] [--n 1024] [--out FILE.json]
DF_GEMM_SPLIT_V=1|2 pins a tile form (read once per process)."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from densefusion_amd import ops

assert os.environ.get("DF_DEV_LIB") and os.environ.get("DF_GEMM_SPLIT_BF16"), "needs DF_DEV_LIB=1 DF_GEMM_SPLIT_BF16=1"
ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=139000)
ap.add_argument("--n", type=int, default=1024)
ap.add_argument("--ks", type=int, nargs="+", default=[384, 512, 768, 1024, 2048])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out")
args = ap.parse_args()
dev = torch.device("cuda")
M, N = args.m, args.n
rows, keep = [], []          # (the weight-plane scratch is per stream: keep every weight alive)
for K in args.ks:
    g = torch.Generator(device="cpu").manual_seed(K)
    x = torch.randn(M, K, generator=g).abs_().to(dev)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    b = torch.randn(N, generator=g).to(dev)
    outbuf = torch.empty(1, M, 1, N, device=dev)
    run = lambda: ops.conv2d_nhwc(x.view(1, M, 1, K), w.view(N, 1, 1, K), bias=b, act=1, out=outbuf)
    for _ in range(3):
        run()
    best = None
    for _ in range(3):          # best of three windows: other work shares the host
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            run()
        e1.record(); torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / args.reps * 1e3
        best = us if best is None or us < best else best
    rows.append({"K": K, "us": round(best, 1), "tflops_fp32_equiv": round(2.0 * M * N * K / best / 1e6, 1)})
    print(json.dumps(rows[-1]), flush=True)
    keep.append(w)
    del x, outbuf
# least squares of us against K.  (the timed call also cuts the weights: N K elements against M K activations, under 1 % here)
n = len(rows)
sk, st = sum(r["K"] for r in rows), sum(r["us"] for r in rows)
skk, skt = sum(r["K"] ** 2 for r in rows), sum(r["K"] * r["us"] for r in rows)
b_ = (n * skt - sk * st) / (n * skk - sk * sk)
a_ = (st - b_ * sk) / n
fit = {"M": M, "N": N, "form": os.environ.get("DF_GEMM_SPLIT_V", "default"), "a_us": round(a_, 1), "b_us_per_k": round(b_, 4),
       "main_loop_tflops_fp32_equiv": round(2.0 * M * N / b_ / 1e6, 1), "a_in_k32_steps": round(a_ / (32 * b_), 1),
       "a_share": {str(r["K"]): round(a_ / r["us"], 3) for r in rows}, "rows": rows}
print(json.dumps(fit))
if args.out:
    json.dump(fit, open(args.out, "w"), indent=1)
