"""Steered fixtures for the device pose loop (csrc/pose.hip): hand-made weights under which the selected point, the selected quaternion
and every refiner output are known in closed form.  No GPU here; tests/test_pose_steered_host.py proves the recipes on the CPU oracle and
tests/test_pose_steered_gpu.py holds the kernels to them.

Every tensor of a state dict is zero (PReLU slopes 0.25) except the handful a recipe sets:
  * ``confidence_by_x``: the confidence of point n is sigmoid(relu(cloud[n].x)), for every object -- the arg-max is steered by the cloud;
  * ``constant_heads``: every point of object o predicts quaternion Q1[o] and offset T1[o], every refine iteration Q2[o], T2[o] (biases of
    the last layers; the zero weights in front of them make the image, the colour embedding and the cloud irrelevant);
  * ``centroid_refiner``: the refiner's translation is the mean of the cloud it was handed and its rotation the identity, so one iteration
    moves any running pose onto the cloud's centroid -- if, and only if, the cloud it was handed is the cloud in the running pose's frame.

The closed forms follow the kernels' own staging: the fp32 normalisation and point + offset of the selection, cast to fp64, then the fp64
quaternion -> matrix -> compose -> matrix -> quaternion chain through oracle/pose_math, iteration by iteration, with the branch of
``quaternion_from_matrix_precise`` each composition takes and whether its sign rule fires.

The default quaternion table has integer rows with integer norms, so the fp32 norm is exact whatever order the squares are summed in."""
from __future__ import annotations

import numpy as np
import torch

from densefusion_amd import synth
from oracle import pose_math

K, N, H, W = 8, 600, 40, 40          # Npad 640; three 256-strides of the arg-max
OFF = 4.0                            # centroid refiner: lifts every transformed coordinate above the ReLUs
ULP_AT_OFF = 2.0 ** -21              # one fp32 ulp of a value in [4, 8): 4.8e-7
Q1 = np.array([[1, 2, 2, 4], [2, 3, 6, 0], [1, 1, 1, 1], [0, 1, 4, 8], [-2, 4, 5, 6], [1, 2, 4, 10], [0, 0, 0, 3], [-1, -2, -2, 0]], np.float32)
Q2 = np.array([[4, 2, 2, 1], [0, 6, 3, 2], [1, -1, 1, -1], [8, 4, 1, 0], [0, 0, 5, 0], [10, 4, 2, 1], [0, 2, 0, 0], [0, 2, 1, 2]], np.float32)
WINNERS = (0, 45, 255, 256, 511, 512, 599, 300)       # first / last slot of each 256-stride, and points inside them
ROW_OBJ = (3, 7, 0, 5, 1, 6, 2, 4)                    # the object of each row of a call: a permutation, so a row index is never its object
BRANCHES = ("trace", "diag0", "diag1", "diag2")


def offsets(seed=5):
    """(T1, T2): per-object offsets of the two networks, uniform in +-0.05 and +-0.02."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(-0.05, 0.05, (K, 3)).astype(np.float32), rng.uniform(-0.02, 0.02, (K, 3)).astype(np.float32)


def zero_state_dict(spec):
    return {k: (np.full(s, 0.25, np.float32) if k.endswith(".conv.2.weight") else np.zeros(s, np.float32)) for k, s in spec}


def posenet_zero(num_obj=K):
    return zero_state_dict(synth.posenet_spec(num_obj))


def refiner_zero(num_obj=K):
    return zero_state_dict(synth.refiner_spec(num_obj))


def confidence_by_x(sd):
    """conf_n = sigmoid(relu(cloud[n].x)) for every object: x1[0] = relu(x), and column 0 of conv1_c (the 1408 inputs are
    x1 | e1 | x2 | e2 | global) carries it down the confidence tower."""
    sd["feat.conv1.weight"][0, 0, 0] = 1
    for layer in (1, 2, 3):
        sd[f"conv{layer}_c.weight"][0, 0, 0] = 1
    sd["conv4_c.weight"][:, 0, 0] = 1
    return sd


def constant_heads(sd_pose, sd_ref, q1, t1, q2, t2):
    """Every point of object o predicts (q1[o], t1[o]); every refine iteration predicts (q2[o], t2[o])."""
    sd_pose["conv4_r.bias"][:] = np.asarray(q1, np.float32).reshape(-1)
    sd_pose["conv4_t.bias"][:] = np.asarray(t1, np.float32).reshape(-1)
    sd_ref["conv3_r.bias"][:] = np.asarray(q2, np.float32).reshape(-1)
    sd_ref["conv3_t.bias"][:] = np.asarray(t2, np.float32).reshape(-1)
    return sd_pose, sd_ref


def centroid_refiner(sd_ref, off=OFF, gain=1.0):
    """out_t = gain x the mean over the points of the cloud handed in, out_r = (1, 0, 0, 0): coordinate c + off rides channel c through
    conv1, conv5 (input channel c of its 384 is x1[c]), conv6, the average pool and the translation tower, and conv3_t scales it and takes
    off away again.  Valid only while every coordinate + off is positive (``assert_no_clip``).  gain = 1 lands on the centroid in one
    iteration, after which the refiner's input is centred and its output ~0 whatever the rotation of the record; gain = 0.5 (exact in every
    number format on the way) halves the distance per iteration, so every iteration's correction is decimetres long and depends on R."""
    num_obj = sd_ref["conv3_t.bias"].shape[0] // 3
    for c in range(3):
        sd_ref["feat.conv1.weight"][c, c, 0] = 1
        sd_ref["feat.conv1.bias"][c] = off
        sd_ref["feat.conv5.weight"][c, c, 0] = 1
        sd_ref["feat.conv6.weight"][c, c, 0] = 1
        sd_ref["conv1_t.weight"][c, c] = 1
        sd_ref["conv2_t.weight"][c, c] = 1
        for o in range(num_obj):
            sd_ref["conv3_t.weight"][o * 3 + c, c] = gain
    sd_ref["conv3_t.bias"][:] = -gain * off
    sd_ref["conv3_r.bias"][:] = np.tile(np.array([1, 0, 0, 0], np.float32), num_obj)
    return sd_ref


def constant_fixture():
    """-> (PoseNet state dict, refiner state dict, T1, T2) of the constant-head recipe on the default table."""
    t1, t2 = offsets()
    sdp, sdr = constant_heads(confidence_by_x(posenet_zero()), refiner_zero(), Q1, t1, Q2, t2)
    return sdp, sdr, t1, t2


def centroid_fixture(gain=1.0):
    """-> (PoseNet state dict of the constant-head recipe, centroid refiner state dict, T1)."""
    sdp, _, t1, _ = constant_fixture()
    return sdp, centroid_refiner(refiner_zero(), gain=gain), t1


# ---- inputs ----
def inputs(seed, rows=K, h=H, w=W, n=N):
    """img: seeded noise, choose: seeded pixel indices (neither can influence a steered result), obj: ROW_OBJ."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return dict(img=rng.standard_normal((rows, 3, h, w)).astype(np.float32),
                choose=rng.integers(0, h * w, (rows, 1, n)).astype(np.int64),
                obj=np.asarray(ROW_OBJ[:rows], np.int64).reshape(rows, 1))


def steered_cloud(seed, maxima, top=0.9):
    """[rows, N, 3]: x a +-0.2 background with ``top`` at the indices ``maxima[row]`` (none: x <= 0 everywhere, all confidences equal),
    y = index * 1e-3 so that the selected translation names the winner, z seeded."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = len(maxima)
    cloud = np.empty((rows, N, 3), np.float32)
    cloud[:, :, 0] = rng.uniform(-0.2, 0.2, (rows, N))
    cloud[:, :, 1] = np.arange(N, dtype=np.float32) * np.float32(1e-3)
    cloud[:, :, 2] = rng.uniform(0.5, 1.2, (rows, N))
    for r, idx in enumerate(maxima):
        if len(idx) == 0:
            cloud[r, :, 0] = -np.abs(cloud[r, :, 0])
        for i in idx:
            cloud[r, i, 0] = top
    return cloud


def centroid_cloud(seed, rows=K, n=N):
    """+-0.2 around (0.1, -0.05, 0.7)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.uniform(-0.2, 0.2, (rows, n, 3)) + np.array([0.1, -0.05, 0.7])).astype(np.float32)


def confidence(cloud):
    """sigmoid(relu(x)) in fp64."""
    return 1.0 / (1.0 + np.exp(-np.maximum(np.asarray(cloud, np.float64)[..., 0], 0.0)))


def first_max(cloud):
    """The point torch.max picks (tools/eval_ycb.py:196): the first maximum of the confidences, i.e. of relu(x)."""
    return np.argmax(np.maximum(cloud[..., 0], 0), axis=-1)


# ---- closed forms ----
def unit32(q):
    """The kernels' fp32 normalisation: nrm = sqrt(((y0^2 + y1^2) + y2^2) + y3^2), q = y / nrm, all in float32."""
    y = np.asarray(q, np.float32)
    nrm = np.sqrt(((y[..., 0] * y[..., 0] + y[..., 1] * y[..., 1]) + y[..., 2] * y[..., 2]) + y[..., 3] * y[..., 3])
    assert nrm.dtype == np.float32
    return y / nrm[..., None]


def select_closed_form(q1, t1, cloud, which, obj):
    """pose_wo [rows, 7] fp64: the fp32 unit quaternion of the row's object and the fp32 sum cloud[which] + T1 (one IEEE add), cast."""
    obj = np.asarray(obj).reshape(-1)
    rows = np.arange(len(obj))
    t = np.asarray(cloud, np.float32)[rows, which] + np.asarray(t1, np.float32)[obj]
    assert t.dtype == np.float32
    return np.concatenate([unit32(np.asarray(q1)[obj]), t], 1).astype(np.float64)


def branch_of(rot):
    """(branch, sign rule fired) of quaternion_from_matrix_precise on the homogeneous rotation ``rot`` (lib/transformations.py:1320-1363)."""
    M = np.asarray(rot, np.float64)
    if np.trace(M[:4, :4]) > M[3, 3]:
        return "trace", False             # w = the trace, > 1
    i, j, k = 0, 1, 2
    if M[1, 1] > M[0, 0]:
        i, j, k = 1, 2, 0
    if M[2, 2] > M[i, i]:
        i, j, k = 2, 0, 1
    return f"diag{i}", bool(M[k, j] - M[j, k] < 0.0)


def compose(pose, q2, t2):
    """One refine composition in fp64 (tools/eval_ycb.py:213-229) -> (new pose [7], the composed rotation as a 4x4)."""
    m1 = pose_math.quaternion_matrix(pose[:4])
    m1[0:3, 3] = pose[4:]
    m2 = pose_math.quaternion_matrix(q2)
    m2[0:3, 3] = t2
    final = np.dot(m1, m2)
    rot = final.copy()
    rot[0:3, 3] = 0
    return np.append(pose_math.quaternion_from_matrix_precise(rot), final[0:3, 3]), rot


def closed_form(q1, t1, q2, t2, cloud, which, obj, iterations):
    """-> (poses: list of [rows, 7] fp64 after 0 .. iterations refine steps, info: {(row, iteration): (branch, fired)}, rots: the composed
    rotations {(row, iteration): 4x4}); iteration counts from 1."""
    obj = np.asarray(obj).reshape(-1)
    poses = [select_closed_form(q1, t1, cloud, which, obj)]
    q2u = unit32(np.asarray(q2)[obj]).astype(np.float64)
    t2d = np.asarray(t2, np.float32)[obj].astype(np.float64)
    info, rots = {}, {}
    for it in range(1, iterations + 1):
        nxt = np.empty_like(poses[-1])
        for r in range(len(obj)):
            nxt[r], rot = compose(poses[-1][r], q2u[r], t2d[r])
            info[(r, it)], rots[(r, it)] = branch_of(rot), rot
        poses.append(nxt)
    return poses, info, rots


def coverage(info):
    """Assert the closed form takes every branch, and every diag branch with the sign rule both firing and not firing."""
    seen = set(info.values())
    assert {b for b, _ in seen} == set(BRANCHES), sorted(seen)
    for b in BRANCHES[1:]:
        assert (b, True) in seen and (b, False) in seen, f"{b}: sign rule seen as {sorted(f for bb, f in seen if bb == b)} only"


def assert_no_clip(cloud, pose, off=OFF):
    """The centroid recipe's precondition: every coordinate of the cloud in the frame of ``pose`` [rows, 7], plus ``off``, is positive
    (tools/eval_ycb.py:206-212 in fp64; the margin asserted, 0.5, is far above fp32 rounding)."""
    for r in range(len(pose)):
        R = pose_math.quaternion_matrix(pose[r, :4])[:3, :3]
        x = (np.asarray(cloud[r], np.float64) - pose[r, 4:]) @ R
        assert x.min() + off > 0.5, f"row {r}: coordinate {x.min():.3f} + {off} is not safely positive; a ReLU would clip"


def centroid_closed_form(q1, t1, cloud, which, obj, iterations=2, gain=1.0):
    """-> list of poses [rows, 7] after 0 .. iterations centroid iterations.  With c the fp64 centroid of the cloud and t the running
    translation, R . (gain . mean((cloud - t) R)) + t = t + gain (c - t): the translation after k iterations is c + (1 - gain)^k (t0 - c)
    whatever the rotation; the rotation is pose_wo's after the sign normalisation of one matrix round trip.  Asserts the ReLU precondition
    for every iteration's input pose."""
    wo = select_closed_form(q1, t1, cloud, which, obj)
    cen = np.asarray(cloud, np.float64).mean(1)
    poses = [wo]
    for k in range(1, iterations + 1):
        assert_no_clip(cloud, poses[-1])
        pose = np.empty_like(wo)
        for r in range(len(wo)):
            pose[r, :4] = pose_math.quaternion_from_matrix_precise(pose_math.quaternion_matrix(wo[r, :4]))
        pose[:, 4:] = cen + (1.0 - gain) ** k * (wo[:, 4:] - cen)
        poses.append(pose)
    return poses


# ---- the CPU oracle on a fixture ----
def oracle_poses(sdp, sdr, batch, cloud, iterations, dtype=torch.float32):
    """oracle/pose_math's estimate loop per row -> list of [rows, 7] fp64 after 0 .. iterations refine steps (the body of
    pose_math.estimate_pose, keeping every iteration's pose)."""
    from oracle import dfnet
    sp, sr = dfnet._to_torch_sd(sdp, dtype), dfnet._to_torch_sd(sdr, dtype)
    out = [[] for _ in range(iterations + 1)]
    with torch.no_grad():
        for r in range(cloud.shape[0]):
            img = torch.from_numpy(batch["img"][r:r + 1]).to(dtype)
            cl = torch.from_numpy(cloud[r:r + 1]).to(dtype)
            choose, obj = torch.from_numpy(batch["choose"][r:r + 1]), torch.from_numpy(batch["obj"][r:r + 1])
            pr, pt, pc, emb = dfnet.posenet_forward(sp, img, cl, choose, obj)
            my_r, my_t, _ = pose_math.select_pose(pr, pt, pc, cl)
            out[0].append(np.append(my_r, my_t).astype(np.float64))
            for it in range(1, iterations + 1):
                my_r, my_t = pose_math.refine_step(sr, cl, emb, obj, my_r, my_t)
                out[it].append(np.append(my_r, my_t).astype(np.float64))
    return [np.stack(o) for o in out]
