"""GPU: ``tools/eval_cad_render.py --ppf``: the tiny run of tests/test_eval_cad_render_dense_tool_gpu.py with and without the flag.  The
logs and results of the existing entries are those of the run without, the new entry ``<source>_ppf`` exists with its summary lines, and
it composes with ``--verify`` and ``--bop``."""
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
    root = tmp_path_factory.mktemp("cad_eval_render_ppf")
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
    ppf = tool.main(_eval_args(files, files["root"] / "ppf") + ["--ppf", "2", "--ppf_points", "200", "--ppf_ref_step", "2", "--ppf_gate", "2000",
                                                                 "--ppf_dense", "3", "--ppf_dense_gate", "2000"])
    assert sorted(plain) == ["truth"] and sorted(ppf) == ["truth", "truth_ppf"]
    assert ppf["truth"] == plain["truth"] and "ppf" not in ppf["truth"]
    assert _log(files, "ppf", "truth") == _log(files, "plain", "truth") and not any("ppf" in line for line in _log(files, "plain", "truth"))
    d = ppf["truth_ppf"]
    served = sum(plain["truth"]["served"])
    assert served >= 3 and d["served"] == plain["truth"]["served"] and d["kept"] == plain["truth"]["kept"] and d["source"] == "truth_ppf"
    m = d["ppf"]
    assert m["items"] == served and m["k"] == 2 and m["points"] == 200 and m["ref_step"] == 2 and m["gate"] == 2000 and m["margin"] == 8
    assert m["bad_item"] == 0 and m["dense"] == 3 and m["dense_gate"] == 2000 and len(m["kept_rank"]) == 2
    assert sum(m["kept_rank"]) + m["no_hypothesis"] == served and m["mean_usable"] > 0 and m["mean_hypotheses"] > 0
    own = [line for line in _log(files, "ppf", "truth_ppf") if line.startswith("[truth_ppf masks] ppf")]
    assert len(own) == 2 and own[0] == ("[truth_ppf masks] ppf top 2 of 200 points, step 1, every 2th a reference, gate 2000, 3 dense steps gate 2000: "
                                        "%d items, %d without a hypothesis, kept rank 0: %d 1: %d" % (served, m["no_hypothesis"], *m["kept_rank"]))
    assert own[1].startswith("[truth_ppf masks] ppf: mean usable nodes ")
    for bad in (["--ppf", "17"], ["--ppf", "-1"], ["--ppf", "1", "--ppf_gate", "65536"], ["--ppf", "1", "--ppf_points", "1025"],
                ["--ppf", "1", "--ppf_ref_step", "0"]):
        with pytest.raises(SystemExit):
            tool.main(_eval_args(files, files["root"] / "bad") + bad)


def test_the_new_entry_composes_with_verify_and_bop(files):
    tool = _tool("eval_cad_render")
    args = _eval_args(files, files["root"] / "base") + ["--verify", "--bop"]
    base = tool.main(args)
    args[args.index(str(files["root"] / "base"))] = str(files["root"] / "all")
    both = tool.main(args + ["--ppf", "2", "--ppf_points", "200", "--ppf_ref_step", "2", "--ppf_gate", "2000", "--ppf_dense", "3"])
    assert sorted(base) == ["truth"] and sorted(both) == ["truth", "truth_ppf"]
    assert both["truth"] == base["truth"] and _log(files, "all", "truth") == _log(files, "base", "truth")
    served = sum(base["truth"]["served"])
    r = both["truth_ppf"]
    assert r["ppf"]["items"] == served and r["verify"]["items"] == served and r["bop"]["items"] == served and r["bop"]["bad_items"] == 0
    lines = _log(files, "all", "truth_ppf")
    for head in ("ppf top 2 of 200 points, ", "verify tol 4 margin 8: ", "bop: "):
        assert any(line.startswith("[truth_ppf masks] %s" % head) for line in lines), head
