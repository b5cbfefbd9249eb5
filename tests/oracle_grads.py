"""fp64 gradient oracle for the training-step tests: per-frame PoseNet / PoseRefineNet outputs and parameter gradients from the CPU
restatement (oracle/dfnet.py + oracle/loss_ref.py, torch autograd), in fp64 and in fp32, and the bound rule that ties a GPU result to them.

Bound rule, per tensor (a parameter gradient, or one output kind over the frames of a step):
    rel_l2(gpu, fp64) <= max(C * rel_l2(cpu32, fp64), floor)
with the floors of GPU_FLOOR / GPU_FLOOR_CNN (below), and the same for the worst output channel (rows of the [Cout, ...] view, worst against worst), beside the flat
max|gpu - fp64| <= 2e-3 * max|fp64| of the older tests.  The fp32 reference's own distance from fp64 measures that tensor's conditioning:
a trunk tensor that sums 10^5 pixel products gets a wide bound, a head tensor of 64 points a narrow one.

The fp32 reference runs on one thread with oneDNN off (im2col + BLAS GEMMs).  Its rounding is then fixed by the library, not by the
machine's core count or by which oneDNN kernel the CPU picks: with oneDNN on, the same tensor's fp32 error moved by up to 1000x between
machines and settings, which would make the bound a property of the test machine.
C = 4; the measured worst ratio of the GPU step to this bound's reference term is 2.81 (the module docstring of
tests/test_train_window_fp64_gpu.py lists each test's).

Conditioning: the symmetric loss replaces each predicted point's target by its nearest target point (oracle/knn_ref.c, fp32).  A
fixture is usable only if the fp64 and the fp32 predictions pick the same nearest targets (up to ties within 1e-5 relative distance) and the
same most-confident point (which anchors new_points / new_target); ``posenet_oracle`` / ``refiner_oracle`` assert both.  A fixture that fails that check is
ill-conditioned: pick another seed, do not widen the bound."""
from __future__ import annotations

import numpy as np
import torch

from densefusion_amd import synth
from oracle import dfnet, loss_ref
from oracle.knn import knn_ref

C = 4.0
FLOOR = 1e-6
# floors of the GPU comparisons (relative L2, worst channel): the step's trunk runs F(4x4,3x3) Winograd-domain convolutions, whose fp32
# transforms carry ~1e-5 relative error into every activation after layer2 (measured on the MI355X: 1e-5 .. 2e-5 on every trunk / PSP
# gradient of the 37-frame window, 60 - 100x the direct-summation CPU reference's own error), and the stem / layer1 weight gradients of
# small crops follow the max-pool's choices, which such errors flip for near-equal neighbours (3e-4 .. 5e-4); the worst
# channels measured 5.2e-2 (trunk, layer4.1.conv2 of the five-frame window) and 5.7e-3 (point layers, LineMOD shape).  C x the CPU
# reference's error tightens the bound wherever fp32 summation alone is worse than that.
GPU_FLOOR_CNN = (1e-3, 8e-2)
GPU_FLOOR = (1e-4, 1e-2)
# the flat max-error check of the CNN tensors: 4.1e-3 of the scale measured on layer4.1.conv2 of the five-frame window (900 pixels), the
# ReLU-gated re-association test_native_train_gpu.py also records against the window's one-frame passes
SCALE_TOL_CNN = 5e-3
SCALE_TOL = 2e-3
OUT_KEYS = ("loss", "dis", "new_points", "new_target", "emb")
CNN_PREFIXES = ("cnn.model.module.feats.", "cnn.model.module.psp.", "cnn.model.module.up_")      # trunk, PSP, up-convs

# ---- the window fixtures (shared by the CPU power check and the GPU tests) ----
# small34: 34 crop sizes in steps of 4 between 40 and 76 (the first 17 take F(4x4,3x3) on layer3.1 at dilation 2, the last 17 do not),
# interleaved; 44 x 44 holds three frames and 68 x 52 two: 37 frames
_SMALL_F4 = [(40, 52), (40, 60), (44, 44), (44, 56), (44, 64), (48, 48), (48, 60), (52, 40), (52, 52), (52, 64), (52, 76), (56, 44),
             (56, 56), (60, 40), (60, 60), (64, 52), (64, 64)]
_SMALL_DIRECT = [(40, 40), (40, 44), (40, 68), (40, 72), (40, 76), (44, 68), (44, 76), (48, 68), (48, 76), (52, 68), (52, 72), (56, 72),
                 (68, 40), (68, 52), (72, 48), (72, 56), (76, 68)]
WINDOWS = {
    "small34": dict(K=3, N=64, M=60, wseed=41, oseed=2000,
                    sizes=[s for pair in zip(_SMALL_F4, _SMALL_DIRECT) for s in pair] + [(44, 44), (68, 52), (44, 44)]),
    # large18: 18 sizes in steps of 40 between 80 and 240, 160 x 160 among them (layer2 takes F(4x4) there), 80 x 120 twice: 19 frames
    "large18": dict(K=3, N=64, M=60, wseed=43, oseed=2100,
                    sizes=[(80, 80), (160, 160), (80, 120), (240, 240), (120, 160), (200, 80), (120, 120), (160, 240), (80, 200),
                           (240, 120), (200, 200), (120, 80), (160, 80), (80, 240), (240, 160), (200, 120), (120, 240), (160, 200),
                           (80, 120)]),
    # mixed5: the five-frame window of test_native_train_gpu.py (two 40 x 80 frames in one bucket)
    "mixed5": dict(K=3, N=128, M=60, wseed=23, oseed=900, sizes=[(40, 80), (160, 160), (80, 80), (40, 80), (120, 160)]),
    # tiny11: the smallest crops the step accepts and the maximum side (DF_MAX_CROP = 3200): trunk maps of 1 x 1 (twice), 2 x 2, 1 x 3,
    # 3 x 1, 2 x 3, 4 x 4, 5 x 4, 2 x 5, 1 x 400 and 400 x 1.  N = 70 with M = 60: the symmetric loss groups 512 // 60 = 8 poses per
    # workgroup, so its last workgroup holds 6 (every other fixture has N % 8 == 0 or one pose per workgroup); frames 1, 4, 7, 10 are symmetric
    "tiny11": dict(K=3, N=70, M=60, wseed=47, oseed=3000,
                   sizes=[(8, 8), (16, 16), (8, 24), (24, 8), (12, 20), (32, 32), (36, 28), (8, 8), (16, 40), (8, 3200), (3200, 8)]),
    # upd4: the window of the parameter-update tests (tests/test_trainer_updates_gpu.py): the smallest crops that put both routes of the
    # stride-1 3x3 trunk convolutions into one pass.  44 x 44 (6 x 6 trunk maps, the smallest square ones at which the dilated layer3.1
    # takes F(4x4,3x3); twice: a bucket of two frames), 24 x 24 (3 x 3 maps, the smallest at which any layer does: layer3.0.conv2 and
    # layer4.0.conv2) and 40 x 40 (5 x 5 maps: the direct kernel on every layer); frame 1 is symmetric.  upd5: the same frames and an
    # 80 x 120 one, for the change of shape between two steps of one handle
    "upd4": dict(K=3, N=70, M=60, wseed=61, oseed=3200, sizes=[(44, 44), (40, 40), (44, 44), (24, 24)]),
    "upd5": dict(K=3, N=70, M=60, wseed=61, oseed=3200, sizes=[(44, 44), (40, 40), (44, 44), (24, 24), (80, 120)]),
}
# the further parameter sets of the update tests: the state dict of the full reload and the one that lends its layer3.1.conv2 weight.
# With four frames of 70 points about one seed in three keeps ``point_relu_margin`` above RELU_MARGIN: the seeds, the two scales below and
# the lanes' jobs were picked one stage after the other on the CPU so that it holds at every parameter set of the sequence
# (tests/test_oracle_updates.py asserts and prints them: 1.5e-5 .. 3.3e-5)
UPDATE_WSEEDS = (101, 151)
UPDATE_KEY = "cnn.model.module.feats.layer3.1.conv2.weight"
UPDATE_GRAPH_FRAMES = (0, 2)             # the graph_safe batch step: the two 44 x 44 frames as one bucket
UPDATE_LANE_JOBS = (0, 1, 2, 0, 1)       # the five bs = 1 jobs of the lanes' window (frames of upd4: two crop sizes, one symmetric)
# one-bucket windows (no bucket to lose: tests/test_oracle_grads.py leaves them out).  ones3: three 8 x 8 frames, 1 x 1 trunk maps only, so
# that a defect of the one-pixel map cannot hide behind larger frames in the summed gradients; frame 1 is symmetric.  The seed keeps
# ``point_relu_margin`` at 2.0e-5 (oseed 3100 has a conv6 pre-activation at 1.1e-6: a ReLU the GPU's fp32 sum may flip)
ONE_BUCKET_WINDOWS = {
    "ones3": dict(K=3, N=70, M=60, wseed=49, oseed=3130, sizes=[(8, 8), (8, 8), (8, 8)]),
}
RELU_MARGIN = 1e-5      # 10x the fp32 rounding of a K = 512 sum of values of about 10


def window(name):
    """-> (K, N, M, state dict, objects): objects from synth.make_object, object index i % K (index 1 is the symmetric one)."""
    w = WINDOWS[name] if name in WINDOWS else ONE_BUCKET_WINDOWS[name]
    K, N, M = w["K"], w["N"], w["M"]
    sd = synth.make_state_dict(synth.posenet_spec(K), w["wseed"])
    objs = [synth.make_object(w["oseed"] + i, h, wd, N, K, num_points_mesh=M) for i, (h, wd) in enumerate(w["sizes"])]
    for i, o in enumerate(objs):
        o["obj"][0] = i % K
        o["symmetric"] = i % K == 1
    return K, N, M, sd, objs


# ---- the parameter-update fixtures (tests/test_trainer_updates_gpu.py, tests/test_oracle_updates.py) ----
# FlatAdam's learning rate there: Adam moves every weight by about lr whatever its size, and the stem weights are 400x smaller than the
# rest (synth.make_state_dict: std 2.9e-4), so 1e-6 moves the stem's output by about a percent and keeps the fixture's conditioning,
# while it is 500 ulp of a trunk weight of 0.03: every tensor's bits change
ADAM_LR = 1e-6
INPLACE_SCALE, REBIND_SCALE = 0.997, 1.0035          # the in-place writer and the rebound buffer scale the whole packed buffer (fp32)
REFINER_UPDATE = dict(K=3, N=70, M=60, wseeds=(1031, 1033), oseed=3300, eseed=7, size=(40, 40))


def refiner_update_frames():
    """-> (K, N, M, the two state dicts, frames): two refiner frames as tests/test_train_window_fp64_gpu.py builds them (a synthetic object's
    cloud, target and mesh, normal embeddings), frame 1 symmetric."""
    u = REFINER_UPDATE
    K, N, M = u["K"], u["N"], u["M"]
    objs = [synth.make_object(u["oseed"] + i, *u["size"], N, K, num_points_mesh=M) for i in range(2)]
    emb = np.random.default_rng(u["eseed"]).standard_normal((2, 32, N)).astype(np.float32)
    frames = [dict(points=o["cloud"], emb=emb[b], obj=b, target=o["target"], model_points=o["model_points"], symmetric=b == 1)
              for b, o in enumerate(objs)]
    return K, N, M, [synth.make_state_dict(synth.refiner_spec(K), s) for s in u["wseeds"]], frames


def second_iteration(frames, first):
    """The frames of the next refine iteration: the first one's new_points / new_target (``first``: per-frame tensors) in place of points / target."""
    return [dict(f, points=torch.as_tensor(first["new_points"][b]).detach().cpu().float().reshape(-1, 3),
                 target=torch.as_tensor(first["new_target"][b]).detach().cpu().float().reshape(-1, 3)) for b, f in enumerate(frames)]


class AdamEmu:
    """FlatAdam's rule (df_adam_step: torch.optim.Adam's defaults) on a state dict, in fp64 with the result rounded to fp32 -- the CPU
    tests' stand-in for the parameter sets a GPU run reaches.  It differs from the GPU's by the rounding of the gradients only, which
    moves a weight by a fraction of ``lr`` where the gradient is within rounding of zero."""

    def __init__(self, lr=ADAM_LR, betas=(0.9, 0.999), eps=1e-8):
        self.lr, self.betas, self.eps, self.t, self.m, self.v = lr, betas, eps, 0, {}, {}

    def step(self, sd, grads):
        self.t += 1
        b1, b2 = self.betas
        out = {}
        for k, p in sd.items():
            p = torch.as_tensor(p).double()
            g = grads[k].double().reshape(p.shape) if k in grads else torch.zeros_like(p)
            self.m[k] = self.m.get(k, 0.0) * b1 + (1 - b1) * g
            self.v[k] = self.v.get(k, 0.0) * b2 + (1 - b2) * g * g
            denom = self.v[k].sqrt() / (1 - b2 ** self.t) ** 0.5 + self.eps
            out[k] = (p - self.lr / (1 - b1 ** self.t) * self.m[k] / denom).float().numpy()
        return out


# ---- per-frame oracle passes ----
class _fixed_fp32_order:
    """One thread, oneDNN off: the fp32 reference's summation order does not depend on the machine's cores or oneDNN's kernel choice."""

    def __enter__(self):
        self.threads = torch.get_num_threads()
        self.mkldnn = torch.backends.mkldnn.flags(enabled=False)
        self.mkldnn.__enter__()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.threads)
        self.mkldnn.__exit__(*exc)


def _nn_inds(pred_r, pred_t, points, model_points, target):
    """The nearest-target index of every predicted model point (the symmetric branch of loss_ref, re-run to read its choice)."""
    q = pred_r.reshape(-1, 4)
    q = q / torch.norm(q, dim=1, keepdim=True)
    base = loss_ref.quat_to_rot_rows(q).transpose(2, 1)
    pred = torch.matmul(model_points.reshape(1, -1, 3), base) + (points + pred_t).reshape(-1, 1, 3)       # [P, M, 3]
    qry = pred.detach().permute(2, 0, 1).reshape(3, -1).numpy()[None]
    tg = target.detach().reshape(-1, 3)
    return dict(inds=knn_ref(tg.t().contiguous().numpy()[None], qry, 1)[0, 0] - 1, pred=pred.detach().reshape(-1, 3), target=tg)


def _grads(loss, psd):
    keys = list(psd)
    gs = torch.autograd.grad(loss, [psd[k] for k in keys], allow_unused=True)
    return {k: g.detach() for k, g in zip(keys, gs) if g is not None}


def posenet_frames(sd, objs, dtype, w=0.015, on_params=None):
    """One PoseNet + Loss pass per object (bs = 1) in ``dtype``: outputs and that frame's own parameter gradients.  ``on_params`` is
    called with the {key: leaf tensor} dict before the passes (an emulated defect finds a layer by the leaf its functional call gets)."""
    psd = {k: torch.as_tensor(v).to(dtype).requires_grad_() for k, v in sd.items()}
    if on_params is not None:
        on_params(psd)
    res = []
    for o in objs:
        T = lambda k: torch.from_numpy(o[k])[None].to(dtype)
        idx = torch.tensor([[int(o["obj"][0])]])
        sym = [int(o["obj"][0])] if o["symmetric"] else []
        r, t, c, emb = dfnet.posenet_forward(psd, T("img"), T("cloud"), torch.from_numpy(o["choose"]), idx)
        M = o["target"].shape[0]
        loss, dis, npt, ntg = loss_ref.loss_calculation(r, t, c, T("target"), T("model_points"), idx, T("cloud"), w, False, M, sym)
        out = dict(pred_r=r, pred_t=t, pred_c=c, emb=emb, loss=loss.reshape(1), dis=dis.reshape(1), new_points=npt, new_target=ntg)
        out = {k: v.detach() for k, v in out.items()}
        out["which"] = int(c.reshape(-1).argmax())
        out["nn"] = _nn_inds(r, t, T("cloud"), T("model_points"), T("target")) if sym else None
        out["grads"] = _grads(loss.reshape(()), psd)
        res.append(out)
    return res


def refiner_frames(sd, frames, dtype):
    """One PoseRefineNet + Loss_refine pass per frame; ``frames``: dicts of points [N,3], emb [32,N], obj, target / model_points [M,3]
    (tensors or arrays) and symmetric."""
    psd = {k: torch.as_tensor(v).to(dtype).requires_grad_() for k, v in sd.items()}
    res = []
    for f in frames:
        T = lambda k: torch.as_tensor(f[k]).detach().cpu()[None].to(dtype)
        idx = torch.tensor([[int(f["obj"])]])
        sym = [int(f["obj"])] if f["symmetric"] else []
        pr, pt = dfnet.refiner_forward(psd, T("points"), T("emb"), idx)
        M = T("target").shape[1]
        dis, npt, ntg = loss_ref.loss_refine_calculation(pr, pt, T("target"), T("model_points"), idx, T("points"), M, sym)
        out = dict(pred_r=pr.detach(), pred_t=pt.detach(), dis=dis.detach().reshape(1), new_points=npt, new_target=ntg, which=0)
        out["nn"] = _nn_inds(pr, pt, torch.zeros(1, 3, dtype=dtype), T("model_points"), T("target")) if sym else None
        out["grads"] = _grads(dis.reshape(()), psd)
        res.append(out)
    return res


def _check_conditioning(r64, r32):
    for i, (a, b) in enumerate(zip(r64, r32)):
        assert a["which"] == b["which"], f"frame {i}: the most confident point differs between fp64 and fp32 -- ill-conditioned fixture"
        if a["nn"] is not None:
            # a query whose two candidate targets lie at the same fp64 distance to within 1e-5 is a tie, not a different
            # answer: either choice gives the same loss to 1e-5 (a step of 10^5 .. 10^6 queries always holds a few such ties)
            diff = np.flatnonzero(a["nn"]["inds"] != b["nn"]["inds"])
            q, tg = a["nn"]["pred"][diff], a["nn"]["target"]
            da = torch.linalg.vector_norm(q - tg[a["nn"]["inds"][diff]], dim=1)
            db = torch.linalg.vector_norm(q - tg[b["nn"]["inds"][diff]], dim=1)
            n = int(((db - da).abs() > 1e-5 * da).sum())
            assert n == 0, f"frame {i}: fp64 and fp32 predictions pick other nearest targets for {n} queries -- ill-conditioned fixture"


def posenet_oracle(sd, objs, w=0.015):
    """-> (fp64 frames, fp32 frames), each a list of ``posenet_frames`` results, after the conditioning check."""
    r64 = posenet_frames(sd, objs, torch.float64, w)
    with _fixed_fp32_order():
        r32 = posenet_frames(sd, objs, torch.float32, w)
    _check_conditioning(r64, r32)
    return r64, r32


def refiner_oracle(sd, frames):
    r64 = refiner_frames(sd, frames, torch.float64)
    with _fixed_fp32_order():
        r32 = refiner_frames(sd, frames, torch.float32)
    _check_conditioning(r64, r32)
    return r64, r32


def point_relu_margin(sd, objs, r64):
    """Smallest |pre-activation| of feat.conv5 / feat.conv6 over the points of all frames, in fp64.  Their fp32 sums (K = 256 / 512,
    values of about 10) carry an absolute rounding error of about 1e-6; a pre-activation closer to zero than that may land on the other side
    of the ReLU on the GPU.  One such flip moves the conv6 bias gradient of a three-frame window of 70 points by 3e-4 (one of about 100
    active entries of one channel in 1024): a window that small must keep its distance from zero, a large one dilutes the flip."""
    import torch.nn.functional as F
    w = {k: torch.as_tensor(v).double() for k, v in sd.items() if k.startswith("feat.")}
    conv = lambda n, x: F.conv1d(x, w[f"feat.{n}.weight"], w[f"feat.{n}.bias"])
    margin = float("inf")
    for o, r in zip(objs, r64):
        x = torch.from_numpy(o["cloud"])[None].double().transpose(2, 1)
        x1, e1 = F.relu(conv("conv1", x)), F.relu(conv("e_conv1", r["emb"].double()))
        x2, e2 = F.relu(conv("conv2", x1)), F.relu(conv("e_conv2", e1))
        z5 = conv("conv5", torch.cat([x2, e2], 1))
        z6 = conv("conv6", F.relu(z5))
        margin = min(margin, float(z5.abs().min()), float(z6.abs().min()))
    return margin


def summed_grads(res, skip=()):
    """Sum of the frames' gradients in fp64 (frames whose index is in ``skip`` left out)."""
    tot = {}
    for i, r in enumerate(res):
        if i in skip:
            continue
        for k, g in r["grads"].items():
            tot[k] = tot[k] + g.double() if k in tot else g.double().clone()
    return tot


def stacked(res, key, rows=None):
    """One output kind over the frames (in ``rows`` order), fp64, one row per frame."""
    rows = range(len(res)) if rows is None else rows
    return torch.cat([res[j][key].double().reshape(1, -1) for j in rows])


# ---- the bound rule ----
def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float(torch.linalg.vector_norm(a - b)) / max(float(torch.linalg.vector_norm(b)), 1e-300)


def worst_channel(a, b):
    """Largest relative L2 over the rows of the [Cout, ...] view; rows of the reference below 1e-6 of its largest row norm (channels a
    ReLU kills for every pixel) are left to the flat max-error check."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    a, b = a.reshape(b.shape[0], -1), b.reshape(b.shape[0], -1)
    nb = torch.linalg.vector_norm(b, dim=1)
    live = nb > 1e-6 * float(nb.max())
    if not bool(live.any()):
        return 0.0
    return float((torch.linalg.vector_norm(a - b, dim=1)[live] / nb[live]).max())


def gpu_floor(name):
    return GPU_FLOOR_CNN if name.startswith(CNN_PREFIXES + ("cnn.model.module.final.",)) else GPU_FLOOR


def check(name, gpu, ref64, ref32, c=C, floor=(FLOOR, FLOOR)):
    """Assert the bound rule for one tensor (``floor``: relative-L2 and worst-channel floors); returns the worst ratio (GPU error / fp32
    reference error) it met."""
    gpu, ref64, ref32 = gpu.detach().cpu().double(), ref64.double(), ref32.double()
    assert gpu.shape == ref64.shape, (name, gpu.shape, ref64.shape)
    e_gpu, e_32 = rel_l2(gpu, ref64), rel_l2(ref32, ref64)
    assert e_gpu <= max(c * e_32, floor[0]), f"{name}: relative L2 vs fp64 {e_gpu:.3e} > max({c} x fp32 reference's {e_32:.3e}, {floor[0]:.0e})"
    ratio = e_gpu / max(e_32, floor[0] / c)
    if gpu.dim() >= 2 and gpu.shape[0] > 1:
        w_gpu, w_32 = worst_channel(gpu, ref64), worst_channel(ref32, ref64)
        assert w_gpu <= max(c * w_32, floor[1]), \
            f"{name}: worst channel's relative L2 vs fp64 {w_gpu:.3e} > max({c} x fp32 reference's {w_32:.3e}, {floor[1]:.0e})"
        ratio = max(ratio, w_gpu / max(w_32, floor[1] / c))
    scale = max(float(ref64.abs().max()), 1e-30)
    err = float((gpu - ref64).abs().max())
    tol = SCALE_TOL_CNN if floor == GPU_FLOOR_CNN else SCALE_TOL
    assert err <= tol * scale, f"{name}: max err {err:.3e} vs scale {scale:.3e}"
    return ratio


def check_grads(got, r64, r32, c=C):
    """Every parameter gradient of a step (grad_dict) against the summed fp64 / fp32 frames; dead classifier weights stay zero.
    -> (worst ratio, its tensor, tensors checked)."""
    g64, g32 = summed_grads(r64), summed_grads(r32)
    worst, where, n, fails = 0.0, "", 0, []
    for k, g in got.items():
        if "classifier" in k:
            assert float(g.abs().max()) == 0.0, k
            continue
        try:
            ratio = check(k, g, g64[k], g32[k], c, gpu_floor(k))
        except AssertionError as e:
            fails.append(str(e))
            continue
        n += 1
        if ratio > worst:
            worst, where = ratio, k
    assert not fails, "\n".join(fails)
    return worst, where, n


def check_outputs(out, rows, r64, r32, keys=OUT_KEYS, c=C):
    """A step's per-frame outputs (output row i = frame rows[i]) against the fp64 / fp32 frames, one output kind at a time."""
    worst, where = 0.0, ""
    for k in keys:
        ratio = check(k, out[k].reshape(len(rows), -1), stacked(r64, k, rows), stacked(r32, k, rows), c, GPU_FLOOR)
        if ratio > worst:
            worst, where = ratio, k
    return worst, where
