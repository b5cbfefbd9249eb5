"""GPU: ``tools/eval_cad_render.py --dense``: the tiny run of tests/test_cad_eval_render_gpu.py with and without the flag.  The logs and
results of the existing entries are those of the run without, the new entries ``<source>_dense`` and ``<source>_icp_dense`` exist with
their summary line, and they compose with ``--verify`` and ``--bop``."""
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cad_raster_np as mnp  # noqa: E402
import cad_render_np as rnp  # noqa: E402
import cad_scene_np as snp  # noqa: E402
import fabricate_cad as fab  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS = 8


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        return importlib.import_module(name)
    finally:
        sys.path.pop(0)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the meshes as PLY files, the camera as a proj_mat.txt, and pose checkpoints of plain initial weights"""
    _dev()
    from densefusion_amd.lib.network import PoseNet, PoseRefineNet
    root = tmp_path_factory.mktemp("cad_eval_render_dense")
    paths = [mnp.write_mesh_ply(root / name, *m) for name, m in zip(("big.ply", "small.ply", "box.ply"), snp.tool_meshes())]
    pm = rnp.write_proj(root / "proj_in.txt", fab.PROJ[1])
    torch.manual_seed(3)
    torch.save(PoseNet(num_points=500, num_obj=5).state_dict(), root / "pose.pth")
    torch.save(PoseRefineNet(num_points=500, num_obj=5).state_dict(), root / "refine.pth")
    return dict(root=root, paths=[str(p) for p in paths], pm=pm, pose=str(root / "pose.pth"), refine=str(root / "refine.pth"))


def _eval_args(files, out):
    return ["--cad_model", files["paths"][0], files["paths"][1], "--cad_distractor", files["paths"][2], "--model", files["pose"], "--refine_model",
            files["refine"], "--masks", "truth", "--cad_seed", "0", "--cad_frames", str(VIEWS), "--seg_blur", "0", "--proj_mat", files["pm"],
            "--height", "64", "--width", "96", "--min_pixels", "60", "--mask", "pixels", "--chunk", "4", "--workers", "0", "--iteration", "2",
            "--output_result_dir", str(out)]


def _log(files, run, entry):
    return open(files["root"] / run / ("eval_result_logs_%s.txt" % entry)).read().splitlines()


def test_the_flag_adds_its_entry_and_changes_no_other(files):
    tool = _tool("eval_cad_render")
    plain = tool.main(_eval_args(files, files["root"] / "plain"))
    dense = tool.main(_eval_args(files, files["root"] / "dense") + ["--dense", "2"])
    assert sorted(plain) == ["truth"] and sorted(dense) == ["truth", "truth_dense"]
    assert dense["truth"] == plain["truth"] and "dense" not in dense["truth"]
    assert _log(files, "dense", "truth") == _log(files, "plain", "truth") and not any("dense" in line for line in _log(files, "plain", "truth"))
    d = dense["truth_dense"]
    served = sum(plain["truth"]["served"])
    assert served >= 3 and d["served"] == plain["truth"]["served"] and d["kept"] == plain["truth"]["kept"] and d["source"] == "truth_dense"
    m = d["dense"]
    assert m["items"] == served and m["gate"] == 16 and m["margin"] == 8 and m["mask"] is False and m["bad_item"] == 0
    assert 0 <= m["few"] + m["degenerate"] <= served and 0.0 <= m["mean_steps"] <= 2.0
    own = [line for line in _log(files, "dense", "truth_dense") if line.startswith("[truth_dense masks] dense ")]
    assert len(own) == 1 and own[0].startswith("[truth_dense masks] dense 2 steps gate 16: %d items, %d few inliers, %d degenerate, mean rms " %
                                               (served, m["few"], m["degenerate"])) and " -> " in own[0]
    masked = tool.main(_eval_args(files, files["root"] / "masked") + ["--dense", "2", "--dense_gate", "300", "--dense_mask"])
    mm = masked["truth_dense"]["dense"]
    assert mm["mask"] is True and mm["gate"] == 300 and mm["items"] == served and masked["truth"] == plain["truth"]
    assert any(line.startswith("[truth_dense masks] dense 2 steps gate 300 masked: ") for line in _log(files, "masked", "truth_dense"))
    for bad in (["--dense", "65"], ["--dense", "-1"], ["--dense", "1", "--dense_gate", "65536"]):
        with pytest.raises(SystemExit):
            tool.main(_eval_args(files, files["root"] / "bad") + bad)


def test_the_new_entries_compose_with_icp_verify_and_bop(files):
    tool = _tool("eval_cad_render")
    args = _eval_args(files, files["root"] / "base") + ["--icp", "2", "--verify", "--bop"]
    base = tool.main(args)
    args[args.index(str(files["root"] / "base"))] = str(files["root"] / "all")
    both = tool.main(args + ["--dense", "2", "--dense_gate", "200"])
    assert sorted(base) == ["truth", "truth_icp", "truth_icp_best"]
    assert sorted(both) == ["truth", "truth_dense", "truth_icp", "truth_icp_best", "truth_icp_dense"]
    for entry in base:
        assert both[entry] == base[entry], entry
        assert _log(files, "all", entry) == _log(files, "base", entry), entry
    served = sum(base["truth"]["served"])
    for entry in ("truth_dense", "truth_icp_dense"):
        r = both[entry]
        assert r["dense"]["items"] == served and r["verify"]["items"] == served and r["bop"]["items"] == served and r["bop"]["bad_items"] == 0
        assert ("icp" in r) == (entry == "truth_icp_dense")
        lines = _log(files, "all", entry)
        for head in ("dense 2 steps gate 200: ", "verify tol 4 margin 8: ", "bop: "):
            assert any(line.startswith("[%s masks] %s" % (entry, head)) for line in lines), (entry, head)
    assert any(line.startswith("[truth_icp_dense masks] ICP 2 steps: ") for line in _log(files, "all", "truth_icp_dense"))
