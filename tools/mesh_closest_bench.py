#!/usr/bin/env python
"""What the exact point-to-mesh distance costs on the device: ``df_mesh_closest`` on ``icosphere(4)`` (5 120 triangles) and
``icosphere(7)`` (327 680 triangles) for the queries and transforms ``detect_symmetry`` itself sends (about 300 x 6 000), the fp64
vector rate of the part measured in the same run with a register-only multiply / add loop (``df_fp64_rate_probe``), and the time of a
whole ``detect_symmetry`` call.  One JSON line.

    python tools/mesh_closest_bench.py [--subdiv 4 7] [--passes 5] [--reps 1] [--no_closest] [--accel]

``--accel`` times ``df_mesh_closest_tree`` on the same inputs right after the scan, the same way (``tree``: its times, the host time of
the tree build apart, the speed-up over this run's scan, whether the outputs are the scan's bytes) and a whole ``detect_symmetry(accel=True)``.

A pass is ``--reps`` calls between two device events; every figure is the median per call over ``--passes`` passes after one warm-up
pass, with the smallest and largest pass next to it.  ``fp64_ops`` counts the contract's arithmetic per pair (include/dfusion.h): D1 is
20 operations an edge (3 for w, 5 for the dot, 1 for iee, 6 for r, 5 for d), D2 39 (3, 18 for the two cross products, 15 for u, v and h,
1 for u + v, 2 for d): 99 a pair; compares and selects are not counted, and the probe's rate counts multiplies and adds the same way.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from densefusion_amd import _lib  # noqa: E402
from densefusion_amd.datasets.customCAD import symmetry as sym  # noqa: E402
from densefusion_amd.lib import mesh_distance as md  # noqa: E402

OPS_PER_PAIR = 3 * 20 + 39
PROBE_OPS_PER_ROUND = 16


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subdiv", type=int, nargs="+", default=[4, 7], help="subdivisions of the icospheres")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=1, help="calls per timed pass")
    ap.add_argument("--no_closest", action="store_true", help="time the call without closest_out")
    ap.add_argument("--probe_blocks", type=int, default=2048, help="workgroups of the fp64 rate loop (256 lanes each)")
    ap.add_argument("--probe_iters", type=int, default=1000000, help="rounds of 16 fp64 operations a lane runs")
    ap.add_argument("--no_detect", action="store_true", help="skip the whole detect_symmetry call")
    ap.add_argument("--accel", action="store_true", help="also time df_mesh_closest_tree (the bounding-box tree route) on the same inputs, right after the scan")
    return ap


def spread(values):
    return {"median": float(np.median(values)), "min": float(min(values)), "max": float(max(values))}


def device_ms(fn, passes, reps):
    """device milliseconds per call of ``fn()``: ``passes`` timed passes of ``reps`` calls after one warm-up pass"""
    out = []
    for k in range(passes + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        if k:
            out.append(a.elapsed_time(b) / reps)
    return out


def detection_call(vertices, triangles):
    """The (vertices, triangles, points, xf) ``detect_symmetry`` sends for this mesh with its defaults, caught at its seam."""
    seen = {}

    def catch(v, t, p, xf, want):
        seen.update(v=v, t=t, p=p, xf=xf)
        K, P = len(xf), len(p)
        return np.zeros((K, P)), np.zeros((K, P), dtype=np.int32), None

    sym.detect_symmetry(vertices, triangles, closest=catch)
    return seen["v"], seen["t"], seen["p"], seen["xf"]


def main(argv=None):
    opt = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_closest_bench needs a GPU (no CPU path)")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cad_raster_np as mnp
    dev = torch.device("cuda", torch.cuda.current_device())
    L = _lib.lib()
    out = {"passes": opt.passes, "reps": opt.reps, "closest_out": not opt.no_closest, "ops_per_pair": OPS_PER_PAIR, "cases": []}
    # the fp64 vector rate of this part, in this run
    sink = torch.empty(opt.probe_blocks * 256, dtype=torch.float64, device=dev)

    def probe():
        _lib.check(L.df_fp64_rate_probe(opt.probe_blocks, opt.probe_iters, sink.data_ptr(), _lib.current_stream()), "fp64_rate_probe")
    probe_ms = spread(device_ms(probe, opt.passes, 1))
    probe_ops = opt.probe_blocks * 256 * opt.probe_iters * PROBE_OPS_PER_ROUND
    peak = probe_ops / probe_ms["median"] / 1e9                      # Tops/s
    out["fp64_probe"] = {"blocks": opt.probe_blocks, "iters": opt.probe_iters, "ms": probe_ms, "fp64_Tops": peak}
    for n in opt.subdiv:
        v, f = mnp.icosphere(n, 60.0)
        v, f = v.astype(np.float32), np.asarray(f, dtype=np.int32)
        v, f, p, xf = detection_call(v, f)
        up = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (v, f, p, xf)]
        K, P, T = len(xf), len(p), len(f)
        scratch = torch.empty(md.scratch_bytes(T), dtype=torch.uint8, device=dev)
        ms = spread(device_ms(lambda: md.mesh_closest(*up, want_closest=not opt.no_closest, scratch=scratch), opt.passes, opt.reps))
        pairs = K * P * T
        case = {"subdiv": n, "triangles": T, "vertices": len(v), "K": K, "P": P, "pairs": pairs, "mesh_closest_ms": ms,
                "Gpairs_per_s": pairs / ms["median"] / 1e6, "fp64_Tops": pairs * OPS_PER_PAIR / ms["median"] / 1e9}
        case["share_of_probe_rate"] = case["fp64_Tops"] / peak
        if opt.accel:
            from densefusion_amd.lib.mesh_set import MeshTree
            tree = MeshTree(v, f)                                    # host, once per mesh: reported apart from the calls
            tms = spread(device_ms(lambda: md.mesh_closest(*up, want_closest=not opt.no_closest, scratch=scratch, accel=True, tree=tree), opt.passes,
                                   opt.reps))
            a = md.mesh_closest(*up, want_closest=not opt.no_closest, scratch=scratch)
            b = md.mesh_closest(*up, want_closest=not opt.no_closest, scratch=scratch, accel=True, tree=tree)
            case["tree"] = {"leaf": tree.leaf, "nodes": tree.n_nodes, "loose": tree.n_loose, "build_host_s": tree.build_seconds,
                            "mesh_closest_tree_ms": tms, "speedup": ms["median"] / tms["median"],
                            "same_bytes": all(x is None or bool(torch.equal(x.view(torch.uint8), y.view(torch.uint8))) for x, y in zip(a, b))}
            del a, b
        if not opt.no_detect:
            times = []
            for _ in range(3):                                       # host clock around a call that ends in device-to-host copies
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                report = sym.detect_symmetry(v, f)
                times.append((time.perf_counter() - t0) * 1e3)
            case["detect_symmetry_ms"] = spread(times[1:])
            if opt.accel:
                times = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fast = sym.detect_symmetry(v, f, accel=True)
                    times.append((time.perf_counter() - t0) * 1e3)
                case["tree"]["detect_symmetry_ms"] = spread(times[1:])                # with the tree build of every call
                case["tree"]["same_report"] = bool(np.array_equal(fast.residuals, report.residuals))
            case["symmetric"] = bool(report.symmetric)
        out["cases"].append(case)
        del up, scratch
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
