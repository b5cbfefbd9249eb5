"""CPU: the depth-sensor model of the customCAD renders (``df_cad_depth_sensor``, steps D0..D6) as its numpy restatement
(tests/cad_sensor_np.py) states it -- against a per-pixel statement in Python integers, then what the rule does: the record
``render.DepthSensor`` makes, the statistics of the noise and of the drop-outs, the clamps, and the z-squared growth of the range noise."""
import numpy as np
import pytest

import cad_render_np as rnp
import cad_sensor_np as dnp
import fabricate_cad as fab
from densefusion_amd.datasets.customCAD import render as cr
from densefusion_amd.datasets.customCAD.project_unity_depth import UnityDepthProjector

PROJ = np.array(fab.PROJ[1])
MAX_NOISE_MUL = 2 ** 31 - 1


def tiny_frames(shape):
    if shape == (1, 1):
        return np.array([[[30000]], [[65535]], [[2]]], dtype=np.uint16)
    return dnp.patchy_frames(3, shape[0], shape[1], 5)


@pytest.mark.parametrize("quant", [1, 7, 4096])
@pytest.mark.parametrize("R", [0, 1, 2, 4])
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (5, 7)])
def test_restatement_equals_the_per_pixel_statement(shape, R, quant):
    """Every branch on tiny frames: all three mechanisms at once (edge_step 12 splits the smooth region's pixels into edge and not),
    each alone, and a noise large enough to reach both clamps."""
    depth = tiny_frames(shape)
    records = [(cr.DepthSensor(3.0, R, 12, 0.5, 0.2, quant).record()), (0, R, 12, 1 << 23, 0, quant), (0, R, 12, 0, 1 << 22, quant),
               (MAX_NOISE_MUL, R, 12, 0, 0, quant), (1 << 20, 0, 0, 0, 0, quant)]
    for rec in records:
        for seed, first in ((0, 0), (12345, 7), (2 ** 32 - 1, 2 ** 32 - 2)):
            got, want = dnp.sense(depth, rec, seed, first), dnp.sense_slow(depth, rec, seed, first)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (rec, seed, first)


def test_branches_are_all_taken_on_the_5x7_fixture():
    depth = tiny_frames((5, 7))
    out, stats = dnp.sense(depth, cr.DepthSensor(3.0, 1, 12, 0.5, 0.2, 1).record(), 0)
    live = depth != 65535
    assert (~live).any() and (stats > 0).all() and 0 < stats[:, 0].sum() < live.sum() - 5, "edge and non-edge, every count"
    assert (out[live] == depth[live]).any() and (out[~live] == 65535).all()


def test_record_values_and_errors():
    assert cr.DepthSensor().record() == (0, 0, 0, 0, 0, 1)
    s = cr.DepthSensor(sigma_code=4.0, edge_radius=2, edge_step=64, edge_drop=0.5, drop=0.01, quant=3)
    assert s.record() == (int(np.rint(4.0 * 2.0 ** 32 / np.sqrt(1431655765.0))), 2, 64, 1 << 23, int(np.rint(0.01 * 2 ** 24)), 3)
    assert s.record()[0] == 454047 and cr.DepthSensor(drop=1.0, edge_drop=1.0).record()[3:5] == (1 << 24, 1 << 24)
    top = (2 ** 31 - 1) * np.sqrt(1431655765.0) / 2.0 ** 32
    assert cr.DepthSensor(sigma_code=top * (1 - 1e-9)).record()[0] <= MAX_NOISE_MUL
    for kw in (dict(sigma_code=-1.0), dict(sigma_code=float("nan")), dict(sigma_code=float("inf")), dict(sigma_code=top * 1.001),
               dict(edge_radius=-1), dict(edge_radius=5), dict(edge_radius=1.5), dict(edge_step=-1), dict(edge_step=65536),
               dict(edge_drop=-0.1), dict(edge_drop=1.1), dict(edge_drop=float("nan")), dict(drop=-1e-9), dict(drop=1.0001),
               dict(quant=0), dict(quant=4097), dict(quant=2.0), dict(quant=True)):
        with pytest.raises(ValueError):
            cr.DepthSensor(**kw)
    with pytest.raises(ValueError):
        cr.apply_sensor(None, (0, 0, 0, 0, 0, 1), 0)


def test_sigma_code_at_is_the_slope_of_project_depth(tmp_path):
    """d z / d code by central differences of ``UnityDepthProjector.project_depth`` one code either side (the curvature term is
    below 1e-8 of the slope there) against 65534 |p23| / z^2."""
    proj = UnityDepthProjector(rnp.write_proj(tmp_path / "proj_mat.txt", PROJ), (1, 3))
    for code in (12000, 30000, 52000):
        z = proj.project_depth(np.array([[code - 1, code, code + 1]], dtype=np.uint16))[0, :, 2]
        slope = (z[2] - z[0]) / 2.0
        for sigma_z in (0.5, 3.0):
            assert np.isclose(cr.DepthSensor.sigma_code_at(PROJ, sigma_z, z[1]) * abs(slope), sigma_z, rtol=1e-6, atol=0.0), (code, sigma_z)


N = 256 * 256
FLAT = np.full((2, 256, 256), 30000, dtype=np.uint16)


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize("seed", [0, 1, 12345])
@pytest.mark.parametrize("sigma", [2, 8, 64])
def test_noise_statistics(sigma, seed):
    """256 x 256 of code 30000, noise alone: mean within 4 standard errors of 0, deviation within 1.5 % of sqrt(sigma^2 + 1/12) (the
    rounding's share), lag-1 correlation along rows, along columns and between the call's frames 0 and 1 below 4 / sqrt(N)."""
    out, stats = dnp.sense(FLAT, cr.DepthSensor(sigma_code=sigma).record(), seed)
    d = out.astype(np.float64) - 30000.0
    assert (out != 65535).all() and stats[:, :3].sum() == 0
    want = np.sqrt(sigma ** 2 + 1.0 / 12.0)
    for f in (0, 1):
        mean, dev = d[f].mean(), d[f].std()
        lags = (_corr(d[f][:, :-1], d[f][:, 1:]), _corr(d[f][:-1], d[f][1:]))
        print(f"sigma {sigma} seed {seed} frame {f}: mean {mean / (sigma / np.sqrt(N)):+.2f} s.e., deviation ratio {dev / want:.4f}, "
              f"lag-1 rows {lags[0] * np.sqrt(N):+.2f} columns {lags[1] * np.sqrt(N):+.2f} / sqrt(N)")
        assert abs(mean) <= 4.0 * sigma / np.sqrt(N)
        assert abs(dev / want - 1.0) <= 0.015
        assert abs(lags[0]) < 4.0 / np.sqrt(N) and abs(lags[1]) < 4.0 / np.sqrt(N)
    between = _corr(d[0], d[1])
    print(f"sigma {sigma} seed {seed}: frames 0 and 1 {between * np.sqrt(N):+.2f} / sqrt(N)")
    assert abs(between) < 4.0 / np.sqrt(N)


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_drop_shares(seed):
    """drop = 0.1 alone on the flat frame, and edge_drop = 0.1 alone on a checkerboard of codes 30000 / 30010 with edge_step 5 and
    R = 1, where every pixel is an edge pixel: the dropped share is within 4 standard errors sqrt(0.1 * 0.9 / N) of 0.1."""
    se = np.sqrt(0.1 * 0.9 / N)
    out, stats = dnp.sense(FLAT, cr.DepthSensor(drop=0.1).record(), seed)
    board = (30000 + 10 * ((np.arange(256)[:, None] + np.arange(256)[None, :]) & 1)).astype(np.uint16)
    eout, estats = dnp.sense(np.stack([board, board]), cr.DepthSensor(edge_radius=1, edge_step=5, edge_drop=0.1).record(), seed)
    assert (estats[:, 0] == N).all() and (estats[:, 1] == 0).all() and (stats[:, 0] == 0).all() and (stats[:, 2] == 0).all()
    for f in (0, 1):
        share, eshare = (out[f] == 65535).mean(), (eout[f] == 65535).mean()
        print(f"seed {seed} frame {f}: drop share {share:.4f} ({(share - 0.1) / se:+.2f} s.e.), edge drop share {eshare:.4f} ({(eshare - 0.1) / se:+.2f} s.e.)")
        assert stats[f, 1] == (out[f] == 65535).sum() and estats[f, 2] == (eout[f] == 65535).sum()
        assert abs(share - 0.1) <= 4.0 * se and abs(eshare - 0.1) <= 4.0 * se
        assert (out[f][out[f] != 65535] == 30000).all() and stats[f, 3] == 0, "a kept pixel without noise keeps its code"


def test_clamps_keep_the_codes_below_the_horizon():
    """Codes 0..3 and 65531..65534 under the largest noise_mul (sigma of about 18 900 codes): every output is within 0..65534, and
    both ends are reached."""
    depth = np.tile(np.array([0, 1, 2, 3, 65531, 65532, 65533, 65534], dtype=np.uint16), (2, 64, 8))
    for quant in (1, 7, 4096):
        out, stats = dnp.sense(depth, (MAX_NOISE_MUL, 0, 0, 0, 0, quant), 3)
        assert out.max() <= 65534 and (out == 0).any() and (out >= 65534 // quant * quant).any()
        assert stats[:, :3].sum() == 0 and (stats[:, 3] > 0).all()


def test_range_noise_grows_with_z_squared(tmp_path):
    """A plane tilted across the columns of a 512 x 512 frame, z from -2500 to -5500, noised with the code sigma that means 2 units of
    range at z0 = -4000 and sent back through ``project_depth``.  The range residuals of two bands of 10 columns (5120 pixels each, z
    within 60 units, so z^4 varies by 8 % across a band and the band's deviation differs from that at its mean depth by less than
    0.1 %) have deviations in the ratio (z_far / z_near)^2.  Sampling error: the deviation of n draws of the four-uniform sum (kurtosis
    2.7) has relative standard error sqrt(1.7 / (4 n)) = 0.0091; the ratio of two, 0.0129; the bound is four of those plus the 0.1 %
    (over seeds 0..199 the ratio's spread about the expected one measures 0.0132)."""
    IH = IW = 512
    proj = UnityDepthProjector(rnp.write_proj(tmp_path / "proj_mat.txt", PROJ), (IH, IW))
    z = np.broadcast_to(np.linspace(-2500.0, -5500.0, IW)[None, :], (IH, IW))
    code = np.rint(65534.0 * ((1.0 + PROJ[2, 2]) + PROJ[2, 3] / z))
    assert code.min() >= 0 and code.max() <= 65534
    clean = code.astype(np.uint16)
    sigma = cr.DepthSensor.sigma_code_at(PROJ, 2.0, -4000.0)
    out, _ = dnp.sense(clean[None], cr.DepthSensor(sigma_code=sigma).record(), 0)
    resid = proj.project_depth(out[0])[:, :, 2] - proj.project_depth(clean)[:, :, 2]
    near, far = slice(40, 50), slice(440, 450)
    z_near, z_far = z[:, near].mean(), z[:, far].mean()
    d_near, d_far = resid[:, near].std(), resid[:, far].std()
    n = IH * 10
    bound = 4.0 * np.sqrt(2.0 * 1.7 / (4.0 * n)) + 0.001
    ratio, want = d_far / d_near, (z_far / z_near) ** 2
    print(f"deviation near {d_near:.3f} (z {z_near:.0f}), far {d_far:.3f} (z {z_far:.0f}): ratio {ratio:.4f}, (z_far / z_near)^2 {want:.4f}, bound {bound:.4f}")
    assert abs(ratio / want - 1.0) <= bound
    assert abs(d_near / (2.0 * (z_near / 4000.0) ** 2) - 1.0) <= 4.0 * np.sqrt(1.7 / (4.0 * n)) + 0.001, "and the scale is sigma_z at z0"
