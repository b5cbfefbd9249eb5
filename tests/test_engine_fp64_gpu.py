"""GPU: the inference engine (csrc/engine.hip) held to fp64 layer by layer, on both GEMM routes.

Every fixture of tests/oracle_fwd.py runs twice: in this process on the product library (the bf16 x 6 split GEMM on its routed layers), and
in a child process on the development library with DF_GEMM_SPLIT_OFF=1 (every launch on the fp32 kernel; the switch is read once per process).
Per run:
  * layer-local: each debug tap against its oracle stage applied to the GPU's own input tap, in fp64 and fp32, under
    rel_l2(gpu, fp64) <= max(4 x rel_l2(fp32, fp64), floor) per tensor and for the worst channel (oracle_fwd.FLOORS);
  * end to end: r / t / c / emb of the full forward, and the poses of estimate(iters = 0 and 2) against oracle/pose_math in fp64 (ADD on
    the model points and the sign-invariant quaternion angle, each within max(4 x the fp32 oracle's, floor)).
The oracle's end-to-end pass is computed once per fixture; its layer-local references once per route (they start from that route's taps).
Each fixture prints one table: stage, route, GPU error, fp32 error (relative L2 and worst channel) and the ratio to the bound (<= 1 passes).
Also: the stand-alone PoseRefineNet.forward layer-local over the rf_* taps, and weight reloads into a handle that has already run."""
import os
import subprocess
import sys
import time

import pytest
import torch

import oracle_fwd as of
from densefusion_amd import _lib, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
POSE_TAPS = ("stem", "layer1", "layer2", "layer3", "layer4", "psp", "up_1", "up_2", "up_3", "pf", "x5", "ap_x", "h1", "h2", "h3")
RF_TAPS = ("rf_pf", "rf_x5", "rf_apx", "rf_f1", "rf_f2")
ROUTES = ("split", "fp32")


def _nets(N, K, sdp, sdr):
    from densefusion_amd.lib.network import PoseNet, PoseRefineNet
    est, ref = PoseNet(N, K), PoseRefineNet(N, K)
    est.load_state_dict({k: torch.from_numpy(v) for k, v in sdp.items()})
    ref.load_state_dict({k: torch.from_numpy(v) for k, v in sdr.items()})
    return est.to(DEV).eval(), ref.to(DEV).eval()


def _valid(name, t, N):
    """A tap in its layout with the padding rows sliced off: point taps [B][N][C], per-object taps [B][C]."""
    if name in ("ap_x", "rf_apx", "rf_f1", "rf_f2"):
        return t.reshape(t.shape[0], -1)
    if name in ("up_3", "pf", "x5", "h1", "h2", "h3", "rf_pf", "rf_x5"):
        return t[:, :N, :, 0].contiguous()
    return t


def run_engine(name):
    """One fixture through the engine of this process's library: the taps of the full forward, its outputs, the poses of estimate(0) and
    estimate(2) and the refiner taps of estimate(2)'s last iteration (host tensors)."""
    from densefusion_amd.lib.network import PoseEstimator
    f, sdp, sdr, b = of.fixture(name)
    est, ref = _nets(f["N"], f["K"], sdp, sdr)
    T = lambda k: torch.from_numpy(b[k]).to(DEV)
    est.debug_taps(True)
    ref.debug_taps(True)
    with torch.no_grad():
        r, t, c, emb = est(T("img"), T("cloud"), T("choose"), T("obj"))
        res = {k: _valid(k, est.debug_tap(k), f["N"]) for k in POSE_TAPS}          # (before estimate: its selection path re-taps the trunk)
        res.update(r=r.cpu(), t=t.cpu(), c=c.cpu(), emb=emb.cpu())
        pe = PoseEstimator(est, ref)
        res["pose_wo"] = pe.estimate(T("img"), T("cloud"), T("choose"), T("obj"), 0)[1].cpu()
        res["pose"] = pe.estimate(T("img"), T("cloud"), T("choose"), T("obj"), 2)[1].cpu()
        res.update({k: _valid(k, ref.debug_tap(k), f["N"]) for k in RF_TAPS})
    est.debug_taps(False)
    ref.debug_taps(False)
    return res


_CHILD = r"""
import os, sys, torch
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_engine_fp64_gpu as m
what, names = sys.argv[3], sys.argv[4].split(",")
torch.save({n: (m.run_engine(n) if what == "engine" else m.run_refiner(n)) for n in names}, sys.argv[2])
"""


def _child_runs(tmp, what, names, timeout=600):
    """``what`` ("engine" / "refiner") for ``names`` in a child process on the development library with every launch on fp32."""
    out = os.path.join(str(tmp), f"{what}_fp32.pt")
    env = dict(os.environ, PYTHONPATH=ROOT, DF_DEV_LIB="1", DF_GEMM_SPLIT_OFF="1")
    env.pop("DF_GEMM_SPLIT_BF16", None)
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out, what, ",".join(names)], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return torch.load(out)


@pytest.fixture(scope="module")
def fp32_runs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return _child_runs(tmp_path_factory.mktemp("fp32"), "engine", list(of.FIXTURES))


class _Table:
    def __init__(self, title):
        self.rows, self.fails, self.title, self.worst = [], [], title, (0.0, "")

    def check(self, stage, route, got, r64, r32, floor):
        e_g, e_32, w_g, w_32, ratio = of.bound_ratio(stage, got, r64, r32, floor)
        self.rows.append(f"{stage:8s} {route:6s} {e_g:10.2e} {e_32:10.2e} {w_g:10.2e} {w_32:10.2e} {ratio:7.3f}")
        self.worst = max(self.worst, (ratio, f"{stage} ({route})"))
        try:
            of.check(f"{stage} ({route})", of.channel_view(stage, got), of.channel_view(stage, r64), of.channel_view(stage, r32), floor=floor)
        except AssertionError as e:
            self.fails.append(str(e))

    def scalar(self, what, route, e_g, e_32, floor):
        bound = max(of.C * e_32, floor)
        self.rows.append(f"{what:8s} {route:6s} {e_g:10.2e} {e_32:10.2e} {'':10s} {'':10s} {e_g / bound:7.3f}")
        self.worst = max(self.worst, (e_g / bound, f"{what} ({route})"))
        if e_g > bound:
            self.fails.append(f"{what} ({route}): {e_g:.3e} > max({of.C} x fp32 oracle's {e_32:.3e}, {floor:.0e})")

    def finish(self):
        print(f"\n{self.title}\n{'stage':8s} {'route':6s} {'gpu rel':>10s} {'fp32 rel':>10s} {'gpu chan':>10s} {'fp32 chan':>10s} {'ratio':>7s}")
        print("\n".join(self.rows))
        print(f"{self.title}: worst ratio to the bound {self.worst[0]:.3f} at {self.worst[1]}")
        assert not self.fails, "\n".join(self.fails)


def _inputs(b):
    return {k: torch.from_numpy(b[k]) for k in ("img", "cloud", "choose", "obj")}


def check_fixture(name, runs, floor=lambda k, r64, r32: of.FLOORS[k]):
    """One fixture's table: ``runs`` = {route: run_engine(name) on that route}, layer-local over every tap and end to end; the caller
    finishes the table.  ``floor``: the layer-local floors of tap k (given its two references)."""
    f, sdp, sdr, b = of.fixture(name)
    e64, e32, t_e2e = of.oracle_pair(sdp, sdr, b)
    of.conditioning(e64, e32)
    sp64, sp32, sr64, sr32 = of.to_sd(sdp, torch.float64), of.to_sd(sdp, torch.float32), of.to_sd(sdr, torch.float64), of.to_sd(sdr, torch.float32)
    tab = _Table(f"{name}: K={f['K']} N={f['N']} {f['H']}x{f['W']} objects {f['objs']}")
    t_ll = time.time()
    for route in ROUTES:
        R = runs[route]
        ll = of.layer_local(sp64, sp32, R, _inputs(b), of.POSENET_STAGES)
        ll.update(of.layer_local(sr64, sr32, R, {"obj": torch.from_numpy(b["obj"])}, ("rf_x5", "rf_apx", "rf_f1", "rf_f2")))
        for k, (r64, r32) in ll.items():
            tab.check(k, route, R[k], r64, r32, floor(k, r64, r32))
    t_ll = time.time() - t_ll
    for route in ROUTES:
        R = runs[route]
        for k in ("emb", "r", "t", "c"):
            tab.check("e2e_" + k, route, R[k], e64[k], e32[k], of.E2E_FLOORS[k])
        for key in ("pose_wo", "pose"):
            for i in range(len(f["objs"])):
                mp = b["model_points"][i]
                g, p64, p32 = R[key][i].numpy(), e64[key][i].numpy(), e32[key][i].numpy()
                tab.scalar(f"ADD{i}" + ("" if key == "pose" else "_0"), route, of.add_of(g, p64, mp), of.add_of(p32, p64, mp), of.ADD_FLOOR)
                tab.scalar(f"ang{i}" + ("" if key == "pose" else "_0"), route, of.quat_angle(g[:4], p64[:4]), of.quat_angle(p32[:4], p64[:4]),
                           of.ANGLE_FLOOR)
    print(f"\n{name}: oracle wall time: end to end {t_e2e:.1f} s (fp64 + fp32), layer-local {t_ll:.1f} s (both routes)")
    return tab


@pytest.mark.parametrize("name", list(of.FIXTURES))
def test_engine_layer_by_layer_and_end_to_end_against_fp64(name, fp32_runs):
    check_fixture(name, {"split": run_engine(name), "fp32": fp32_runs[name]}).finish()


def test_fixtures_cover_every_winograd_route_of_the_trunk():
    """Together the fixtures take every route df_wino_route can choose for the stride-1 3x3 convolutions of layer2, layer3 and layer4 at
    the datasets' crops (map sides 1 .. 80: crops up to 640): a change of the route function that moves a layer onto a route no fixture
    takes fails here instead of going untested."""
    route = _lib.lib().df_wino_route

    def convs(h, w):        # (layer, route) of every stride-1 3x3 conv of layer2 .. layer4 on an h x w map
        return [("layer2", route(h, w, 1, 128, 128)),
                ("layer3", route(h, w, 1, 128, 256)), ("layer3", route(h, w, 1, 256, 256)), ("layer3", route(h, w, 2, 256, 256)),
                ("layer4", route(h, w, 1, 256, 512)), ("layer4", route(h, w, 1, 512, 512)), ("layer4", route(h, w, 4, 512, 512))]

    def trunk(n):           # stem (7, 2, 3), max-pool (3, 2, 1), layer2 (3, 2, 1)
        for _ in range(3):
            n = (n - 1) // 2 + 1
        return n

    reachable = {lr for h in range(1, 81) for w in range(1, 81) for lr in convs(h, w)}
    covered = {lr for f in of.FIXTURES.values() for lr in convs(trunk(f["H"]), trunk(f["W"]))}
    assert {r for l, r in reachable} == {0, 2, 4}
    assert reachable <= covered, f"routes no fixture takes: {sorted(reachable - covered)}"
    print(f"\nroutes taken: {sorted(covered)}")


# ---- the stand-alone refiner, layer-local over its taps ----
RF_FIXTURES = ("k13_n500_80x80_b3", "k21_n129_80x120")


def _refiner_inputs(name):
    """Oracle-made refiner inputs: the cloud moved into the frame of the fp64 oracle's selected pose (tools/eval_ycb.py:206-212) and the
    fp64 oracle's emb, per object."""
    f, sdp, sdr, b = of.fixture(name)
    e64 = of.end_to_end(sdp, sdr, b, torch.float64, iters=0)
    xs = []
    for i in range(len(f["objs"])):
        cloud = torch.from_numpy(b["cloud"][i:i + 1]).double()
        wo = e64["pose_wo"][i].numpy()
        R = torch.from_numpy(of.pose_math.quaternion_matrix(wo[:4])[:3, :3]).view(1, 3, 3)
        xs.append(torch.bmm(cloud - torch.from_numpy(wo[4:]).view(1, 1, 3), R))
    return f, sdr, b, torch.cat(xs).float(), e64["emb"].float()


def run_refiner(name):
    f, sdr, b, x, emb = _refiner_inputs(name)
    _, ref = _nets(f["N"], f["K"], synth.make_state_dict(synth.posenet_spec(f["K"]), f["wseed"]), sdr)
    ref.debug_taps(True)
    with torch.no_grad():
        r, t = ref(x.to(DEV), emb.to(DEV), torch.from_numpy(b["obj"]).to(DEV))
        res = {k: _valid(k, ref.debug_tap(k), f["N"]) for k in RF_TAPS}
    ref.debug_taps(False)
    res.update(rf_r=r.cpu(), rf_t=t.cpu())
    return res


def test_standalone_refiner_layer_by_layer_against_fp64(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    fp32 = _child_runs(tmp_path, "refiner", list(RF_FIXTURES))
    for name in RF_FIXTURES:
        f, sdr, b, x, emb = _refiner_inputs(name)
        tab = _Table(f"stand-alone refiner, {name}")
        for route, R in (("split", run_refiner(name)), ("fp32", fp32[name])):
            inputs = {"rf_x": x, "rf_emb": emb, "obj": torch.from_numpy(b["obj"])}
            ll = of.layer_local(of.to_sd(sdr, torch.float64), of.to_sd(sdr, torch.float32), R, inputs, of.REFINER_STAGES)
            for k, (r64, r32) in ll.items():
                tab.check(k, route, R[k], r64, r32, of.FLOORS[k])
        tab.finish()


# ---- weights loaded into a handle that has already run ----
RELOAD_FIXTURE = "k13_n500_80x80_b3"       # layer4 on F(4x4,3x3): its Winograd-domain weights are derived copies
RELOAD_KEYS = [("posenet", "cnn.model.module.psp.stages.1.1.weight"), ("posenet", "cnn.model.module.feats.layer4.1.conv2.weight"),
               ("posenet", "feat.conv6.weight"), ("posenet", "conv1_c.weight"), ("posenet", "conv2_r.weight"), ("refiner", "feat.conv6.weight")]


def _outputs(est, ref, b):
    from densefusion_amd.lib.network import PoseEstimator
    T = lambda k: torch.from_numpy(b[k]).to(DEV)
    with torch.no_grad():
        out = [o.cpu() for o in est(T("img"), T("cloud"), T("choose"), T("obj"))]
        out += [o.cpu() for o in PoseEstimator(est, ref).estimate(T("img"), T("cloud"), T("choose"), T("obj"), 2)]
    return out         # r, t, c, emb, pose_wo, pose


def test_reloaded_weights_equal_a_fresh_handle_and_hold_the_fp64_bound():
    """A handle that has run a forward, then takes a second state dict in full, or one tensor of it (a PSP stage, a Winograd-domain layer4
    conv, conv6 with its fused column sums, a head-1 tower, a head-2 tower, the refiner's conv6): its next outputs and poses equal a fresh
    handle's bit for bit (the PSP fold, Winograd-domain copies and bf16 planes were rebuilt) and hold the fp64 bound for the new weights."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    f, sdp, sdr, b = of.fixture(RELOAD_FIXTURE)
    route = _lib.lib().df_wino_route
    assert route(10, 10, 4, 512, 512) != 0 and f["H"] == f["W"] == 80
    sdp2 = synth.make_state_dict(synth.posenet_spec(f["K"]), f["wseed"] + 53)
    sdr2 = synth.make_state_dict(synth.refiner_spec(f["K"]), f["wseed"] + 1053)
    variants = [("all", sdp2, sdr2)]
    for net, key in RELOAD_KEYS:
        vp, vr = dict(sdp), dict(sdr)
        (vp if net == "posenet" else vr)[key] = (sdp2 if net == "posenet" else sdr2)[key]
        variants.append((f"{net} {key}", vp, vr))
    for tag, vp, vr in variants:
        est, ref = _nets(f["N"], f["K"], sdp, sdr)
        _outputs(est, ref, b)
        if tag == "all":
            est.load_state_dict({k: torch.from_numpy(v) for k, v in vp.items()})
            ref.load_state_dict({k: torch.from_numpy(v) for k, v in vr.items()})
        else:
            net, key = tag.split(" ")
            with torch.no_grad():
                dict((est if net == "posenet" else ref).named_parameters())[key].copy_(torch.from_numpy((vp if net == "posenet" else vr)[key]))
        got = _outputs(est, ref, b)
        want = _outputs(*_nets(f["N"], f["K"], vp, vr), b)
        for i, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(g, w), f"{tag}: output {i} of the reloaded handle differs from a fresh handle's by {float((g.double() - w.double()).abs().max()):.3e}"
        e64, e32, _ = of.oracle_pair(vp, vr, b)
        of.conditioning(e64, e32)
        tab = _Table(f"reload: {tag}")
        for k, g in zip(("r", "t", "c", "emb"), got[:4]):
            tab.check("e2e_" + k, "split", g, e64[k], e32[k], of.E2E_FLOORS[k])
        for i in range(len(f["objs"])):
            mp = b["model_points"][i]
            for key, g in (("pose_wo", got[4]), ("pose", got[5])):
                tab.scalar(f"ADD{i}" + ("" if key == "pose" else "_0"), "split", of.add_of(g[i].numpy(), e64[key][i].numpy(), mp),
                           of.add_of(e32[key][i].numpy(), e64[key][i].numpy(), mp), of.ADD_FLOOR)
        tab.finish()
