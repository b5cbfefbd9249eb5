"""GPU: the device pose loop (csrc/pose.hip, and the engine's sequencing of its R|T record) steered through every branch with the hand-made
weights of tests/steered.py, against closed forms at the loop's own precision.  K = 8 objects, N = 600 points (Npad 640: three 256-strides
of the arg-max), 40 x 40 crops; a row's object is never its row index (steered.ROW_OBJ).

A. Constant heads, 0 .. 4 refine iterations: the selection stage bit for bit (one fp32 division per quaternion element with its sign
   kept, one fp32 add per coordinate, the winner named by the cloud's y), then the fp64 quaternion -> matrix -> compose -> matrix ->
   quaternion chain to 1e-12 absolute on all 7 numbers.  The table takes every branch of mat_to_quat_precise and every diag branch with
   and without the sign rule (asserted).  The bound is derived: about 100 fp64 operations per iteration on values <= 1 at 2.2e-16 each;
   1e-12 is four orders above that and five below what one fp32 step inside the chain would leave (6e-8).  Where the closed form's
   |w| < 1e-9 the comparison is up to a common sign (a zero w rounds to either side); everywhere else the sign must match.
B. Ties and strides of the arg-max: the first of equal maxima wins, inside one thread's stride, across threads, across strides, and when
   every confidence is equal; the full forward gives sigmoid(relu(x)) to 1e-6 and its first maximum is the same point.
C. Centroid refiner: after 1 and after 2 iterations the translation is the cloud's centroid, which holds only if the refiner saw the cloud
   in the running pose's frame (R not its transpose, t with its sign, M1 . t2 + t1) and the record was refreshed after iteration 1.  Bound
   per object: 4 x the distance of the fp32 CPU oracle on the same fixture to the fp64 centroid (the factor of oracle_grads / oracle_fwd),
   floor one fp32 ulp at OFF + 1 (4.8e-7 m).  The CPU oracle's AvgPool1d adds 600 values of about 4 one after another, the engine sums
   in partial sums.  Once on the centroid the refiner's input is centred and its output ~0 whatever rotation the record holds, so the
   record refiner_tail_kernel writes is also steered with gain 0.5: every iteration halves the distance to the centroid (closed form
   c + 0.5^k (t0 - c)), a decimetre-long correction that a transposed R in that record turns elsewhere.  Same bound rule.
D. The objects of A as two crop-size buckets through estimate_multi: bit-equal to the single-size call row by row.
E. PoseRefineNet.forward alone: out_r / out_t are the rows of the object, bit for bit.

Measured on the MI355X (default GEMM route): A worst |difference| to the closed form 3.3e-16 over iterations 1 .. 4 and all rows, every
bit-equality exact; C distance to the closed form 6.5e-8 .. 6.7e-7 m on the GPU against 4.0e-7 .. 4.1e-6 m of the fp32 CPU oracle, worst
ratio of a GPU distance to its bound 0.085 (gain 1) and 0.154 (gain 0.5) (<= 1 passes).  The module runs in about 4 s."""
import numpy as np
import pytest
import torch

import steered as st
from oracle_grads import C, _fixed_fp32_order

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12
W_ZERO = 1e-9
GAINS = (1.0, 0.5)


def _load(net, sd):
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def nets():
    """One PoseNet (confidence by x + constant heads), the constant refiner, the centroid refiner and their estimators for the module."""
    from densefusion_amd.lib.network import PoseEstimator, PoseNet, PoseRefineNet
    sdp, sdr, t1, t2 = st.constant_fixture()
    est, ref = _load(PoseNet(st.N, st.K), sdp), _load(PoseRefineNet(st.N, st.K), sdr)
    cen = {g: _load(PoseRefineNet(st.N, st.K), st.centroid_refiner(st.refiner_zero(), gain=g)) for g in GAINS}
    return dict(sdp=sdp, sdr=sdr, t1=t1, t2=t2, est=est, ref=ref, pe=PoseEstimator(est, ref), pe_cen={g: PoseEstimator(est, c) for g, c in cen.items()})


@pytest.fixture(scope="module")
def case_a(nets):
    batch = st.inputs(31)
    cloud = st.steered_cloud(32, [(w,) for w in st.WINNERS])
    poses, info, _ = st.closed_form(st.Q1, nets["t1"], st.Q2, nets["t2"], cloud, np.asarray(st.WINNERS), batch["obj"], 4)
    st.coverage(info)
    return dict(batch=batch, cloud=cloud, poses=poses, info=info)


def _dev(a):
    return torch.from_numpy(a).to(DEV)


def _estimate(pe, batch, cloud, iteration):
    wo, pose = pe.estimate(_dev(batch["img"]), _dev(cloud), _dev(batch["choose"]), _dev(batch["obj"]), iteration)
    return wo.cpu().numpy(), pose.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _bit_equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, f"{what}: {len(bad)} elements differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} vs {want[tuple(bad[0])]!r}"


def _close_pose(got, want, what):
    """All 7 numbers within TOL; the quaternion up to a common sign only where the closed form's |w| < W_ZERO.  -> worst difference."""
    worst = 0.0
    for r in range(len(want)):
        g = got[r].copy()
        if abs(want[r, 0]) < W_ZERO and np.dot(g[:4], want[r, :4]) < 0:
            g[:4] = -g[:4]
        d = np.abs(g - want[r])
        worst = max(worst, d.max())
        assert d.max() <= TOL, f"{what}, row {r} (object {st.ROW_OBJ[r]}): |difference| {d.max():.3e} > {TOL:.0e}\n got  {got[r]}\n want {want[r]}"
    return worst


@pytest.mark.parametrize("iteration", [0, 1, 2, 3, 4])
def test_constant_heads_through_every_branch(nets, case_a, iteration):
    batch, cloud, poses = case_a["batch"], case_a["cloud"], case_a["poses"]
    wo, pose = _estimate(nets["pe"], batch, cloud, iteration)
    # the selection stage, bit for bit: the winner (named by y), one IEEE add per coordinate, one correctly rounded division per element
    _bit_equal(wo[:, 4:], poses[0][:, 4:], "pose_wo translation (fp32 cloud[winner] + T1, cast)")
    _bit_equal(wo[:, :4], poses[0][:, :4], "pose_wo quaternion (fp32 y / nrm with its sign, cast)")
    if iteration == 0:
        _bit_equal(pose, wo, "pose after 0 iterations")
    else:
        worst = _close_pose(pose, poses[iteration], f"pose after {iteration} iterations")
        taken = sorted({case_a["info"][(r, iteration)] for r in range(st.K)})
        print(f"\niteration {iteration}: worst |difference| to the closed form {worst:.2e}; branches of this step {taken}")
    # img and choose cannot influence a steered result
    other = st.inputs(131)
    wo2, pose2 = _estimate(nets["pe"], dict(batch, img=other["img"], choose=other["choose"]), cloud, iteration)
    _bit_equal(wo2, wo, "pose_wo with another image")
    _bit_equal(pose2, pose, "pose with another image")


TIES = [((45, 301, 557), 45),        # all in the stride of thread 45: the thread keeps its first
        ((299, 45), 45),             # threads 43 and 45: the reduction prefers the lower index
        ((599, 256), 256),           # threads 87 and 0, third and second stride
        ((), 0)]                     # x <= 0 everywhere: every confidence is 0.5


def test_argmax_ties_and_strides(nets):
    rows = len(TIES)
    batch = st.inputs(34, rows=rows)
    cloud = st.steered_cloud(33, [t for t, _ in TIES])
    winners = np.asarray([w for _, w in TIES])
    assert np.isfinite(cloud).all() and np.array_equal(st.first_max(cloud), winners)
    want = st.select_closed_form(st.Q1, nets["t1"], cloud, winners, batch["obj"])
    wo, pose = _estimate(nets["pe"], batch, cloud, 0)
    picked = np.rint((wo[:, 5] - nets["t1"][batch["obj"].reshape(-1), 1].astype(np.float64)) / 1e-3).astype(int)
    assert np.array_equal(picked, winners), f"selected points {picked}, first maxima {winners}"
    _bit_equal(wo, want, "pose_wo")
    _bit_equal(pose, wo, "pose after 0 iterations")
    # the full forward: the same confidences, and its first maximum is the same point
    r, t, c, _ = nets["est"](_dev(batch["img"]), _dev(cloud), _dev(batch["choose"]), _dev(batch["obj"]))
    c = c.cpu().numpy().reshape(rows, st.N)
    np.testing.assert_allclose(c.astype(np.float64), st.confidence(cloud), rtol=0, atol=1e-6)
    assert np.array_equal(np.argmax(c, axis=1), winners)
    for (tied, _), row in zip(TIES, c):
        assert len({row[i].tobytes() for i in tied}) <= 1, "equal inputs must give bit-equal confidences"
    obj = batch["obj"].reshape(-1)
    _bit_equal(r.cpu().numpy(), np.broadcast_to(st.Q1[obj][:, None], (rows, st.N, 4)).copy(), "out_r of the full forward")
    _bit_equal(t.cpu().numpy(), np.broadcast_to(nets["t1"][obj][:, None], (rows, st.N, 3)).copy(), "out_t of the full forward")


@pytest.mark.parametrize("gain", GAINS)
def test_centroid_refiner_sees_the_cloud_in_the_running_frame(nets, gain):
    batch = st.inputs(41)
    cloud = st.centroid_cloud(42)
    which = st.first_max(cloud)
    x = np.sort(cloud[:, :, 0], axis=1)
    assert (x[:, -1] - x[:, -2]).min() > 1e-5, "the most confident point must be unique well above fp32 resolution"
    want = st.centroid_closed_form(st.Q1, nets["t1"], cloud, which, batch["obj"], 2, gain)
    with _fixed_fp32_order():
        cpu = st.oracle_poses(nets["sdp"], st.centroid_refiner(st.refiner_zero(), gain=gain), batch, cloud, 2)
    worst, rows, fails = 0.0, [], []
    for it in (1, 2):
        wo, pose = _estimate(nets["pe_cen"][gain], batch, cloud, it)
        _bit_equal(wo, want[0], "pose_wo")
        d_gpu = np.linalg.norm(pose[:, 4:] - want[it][:, 4:], axis=1)
        d_cpu = np.linalg.norm(cpu[it][:, 4:] - want[it][:, 4:], axis=1)
        bound = np.maximum(C * d_cpu, st.ULP_AT_OFF)
        worst = max(worst, (d_gpu / bound).max())
        for r in range(st.K):
            rows.append(f"  iteration {it} object {st.ROW_OBJ[r]}: GPU {d_gpu[r]:.2e} m  fp32 CPU {d_cpu[r]:.2e} m  bound {bound[r]:.2e} m  ratio {d_gpu[r] / bound[r]:.3f}")
            if d_gpu[r] > bound[r]:
                fails.append(rows[-1])
        _close_pose(pose[:, :4], want[it][:, :4], f"rotation after {it} centroid iterations")
    print(f"\ngain {gain}: distance of the translation to the closed form\n" + "\n".join(rows) + f"\nworst ratio to the bound {worst:.3f} (<= 1 passes)")
    assert not fails, "\n".join(fails)


def test_two_crop_size_buckets_equal_the_single_size_call(nets, case_a):
    batch, cloud, iteration = case_a["batch"], case_a["cloud"], 3
    wide = st.inputs(51, rows=3, h=40, w=80)
    imgs = [_dev(batch["img"][:5]), _dev(wide["img"])]
    choose = np.concatenate([batch["choose"][:5], wide["choose"]]).reshape(st.K, st.N)
    wo, pose = nets["pe"].estimate_multi(imgs, _dev(cloud), _dev(choose), _dev(batch["obj"].reshape(-1)), iteration)
    wo, pose = wo.cpu().numpy(), pose.cpu().numpy()
    wo1, pose1 = _estimate(nets["pe"], batch, cloud, iteration)
    _bit_equal(wo, wo1, "pose_wo of the two-bucket call")
    _bit_equal(pose, pose1, "pose of the two-bucket call")
    _bit_equal(wo, case_a["poses"][0], "pose_wo")
    _close_pose(pose, case_a["poses"][iteration], "pose of the two-bucket call")


@pytest.mark.parametrize("order", [st.ROW_OBJ, tuple(range(st.K)), (7,) * st.K])
def test_refiner_forward_selects_the_rows_of_its_object(nets, order):
    rng = np.random.Generator(np.random.PCG64(61))
    x = st.centroid_cloud(62)
    emb = rng.standard_normal((st.K, 32, st.N)).astype(np.float32)
    obj = np.asarray(order, np.int64)
    out_r, out_t = nets["ref"](_dev(x), _dev(emb), _dev(obj.reshape(-1, 1)))
    _bit_equal(out_r.cpu().numpy(), st.Q2[obj], "out_r")
    _bit_equal(out_t.cpu().numpy(), nets["t2"][obj], "out_t")
