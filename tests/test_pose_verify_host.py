"""CPU, the restatement only (tests/pose_verify_np.py): what the tallies of ``df_pose_verify`` and the visible-surface IoU say on scenes
whose answer is known.  The fixture is the bracket of the ICP tests on 64 x 96 frames in front of a wall."""
import numpy as np
import pytest

import fabricate_cad as fab
import mesh_closest_np as m
import mesh_icp_np as icp
import pose_verify_np as pv

IH, IW, TOL, WALL = 64, 96, 1, 60000


@pytest.fixture(scope="module")
def part():
    """The bracket at its true pose: dict with the scene arguments, the pose, the rendered codes [IH,IW] (65535: not rendered)."""
    v, t = m.bracket()
    v = v * np.float32(30.0)
    q = icp.quat_mul(icp.quat_from_axis_angle([0, 1, 0], 0.6), icp.quat_from_axis_angle([1, 0, 0], 0.5))
    pose = np.concatenate([q, [0.004, -0.003, -0.28]])
    sc = dict(vertices=v, triangles=t, tri_begin=np.array([0, len(t)], np.int32), model_scale=np.array([10.0]), proj=np.array(fab.PROJ[1]))
    keys = []
    run(sc, np.full((IH, IW), WALL), None, pose, keys)
    sc["codes"] = pv.rendered_codes(keys[0], 0, 0, IH, IW)
    sc["pose"] = pose
    assert 300 < (sc["codes"] != 65535).sum() < IH * IW // 4 and sc["codes"][sc["codes"] != 65535].max() + 600 < WALL
    return sc


def run(sc, depth, mask, pose, keys_out=None, tol=TOL):
    """One item over the whole frame: its row of tallies."""
    return pv.verify_np(sc["vertices"], sc["triangles"], sc["tri_begin"], sc["model_scale"], sc["proj"], np.asarray(depth, np.uint16)[None],
                        None if mask is None else np.asarray(mask, np.uint16)[None], [[0, 0, 0, 0, 0, 65535]], [pose], pv.CLOUD_DIV, IH, IW,
                        tol, 1, keys_out)[0]


def scene(sc):
    """(observed depth: the part in front of the wall; its pixel mask)"""
    on = sc["codes"] != 65535
    return np.where(on, sc["codes"], WALL), np.where(on, 65535, 0)


def test_true_pose_scores_one(part):
    depth, mask = scene(part)
    row = run(part, depth, mask, part["pose"])
    n = int((part["codes"] != 65535).sum())
    assert row.tolist()[:10] == [0, n, n, 0, 0, 0, n, n, 0, 0] and pv.vsiou(row) == 1.0


def test_depth_shift_scores_zero(part):
    depth, mask = scene(part)
    on = part["codes"] != 65535
    n = int(on.sum())
    nearer, farther = run(part, np.where(on, depth - (TOL + 1), depth), mask, part["pose"]), run(part, np.where(on, depth + (TOL + 1), depth), mask, part["pose"])
    assert nearer[2] == 0 and nearer[3] == n and nearer[8] == n and pv.vsiou(nearer) == 0.0, "all front"
    assert farther[2] == 0 and farther[4] == n and farther[8] == 0 and pv.vsiou(farther) == 0.0, "all behind"
    assert run(part, np.where(on, depth + TOL, depth), mask, part["pose"])[2] == n, "a shift of tol still agrees"


def test_occluder_and_the_two_masks(part):
    """An occluder 500 codes nearer over the left half of the part.  With the pixel mask of what is still seen the true pose keeps
    vsiou 1: `front` is neutral.  With the box of those pixels (half-open, as the loader cuts it) the wall and the occluder inside the box
    count as unexplained."""
    depth, _ = scene(part)
    on = part["codes"] != 65535
    cols = np.where(on.any(axis=0))[0]
    half = (cols.min() + cols.max() + 1) // 2
    hidden = on & (np.arange(IW)[None, :] < half)
    depth = np.where(np.arange(IW)[None, :] < half, np.where(on, depth - 500, WALL - 700), depth)
    seen = on & ~hidden
    rows, cs = np.where(seen.any(axis=1))[0], np.where(seen.any(axis=0))[0]
    box = np.zeros((IH, IW), dtype=np.int64)
    box[rows.min():rows.max(), cs.min() - 3:cs.max()] = 65535                  # three columns of the occluder fall into the box
    pixel, boxed = run(part, depth, np.where(seen, 65535, 0), part["pose"]), run(part, depth, box, part["pose"])
    print("occluded true pose: vsiou with the pixel mask", float(pv.vsiou(pixel)), "with the box mask", float(pv.vsiou(boxed)),
          dict(zip(pv.STATS, boxed.tolist())))
    assert pixel[3] == int(hidden.sum()) > 0 and pixel[2] == int(seen.sum()) and pixel[8] == 0 and pv.vsiou(pixel) == 1.0
    assert boxed[2] == pixel[2] and boxed[8] > 0 and 0.0 < pv.vsiou(boxed) < 1.0


def test_lateral_shift_scores_lower(part):
    depth, mask = scene(part)
    cols = np.where((part["codes"] != 65535).any(axis=0))[0]
    width_px = cols.max() - cols.min() + 1
    # a pixel is 2 |z| / (p00 IW) camera units wide at range z
    shift = 0.5 * width_px * 2.0 * abs(part["pose"][6] * pv.CLOUD_DIV) / (fab.PROJ[1][0][0] * IW) / pv.CLOUD_DIV
    moved = part["pose"].copy()
    moved[4] += shift
    true, off = run(part, depth, mask, part["pose"]), run(part, depth, mask, moved)
    print("lateral shift of", width_px / 2, "px: vsiou", float(pv.vsiou(true)), "->", float(pv.vsiou(off)), dict(zip(pv.STATS, off.tolist())))
    assert off[4] > 0 and off[8] > 0 and pv.vsiou(off) < pv.vsiou(true) == 1.0
