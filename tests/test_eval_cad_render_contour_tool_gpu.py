"""GPU: ``tools/eval_cad_render.py --contour`` and ``--ppf_contour``: the tiny run of tests/test_eval_cad_render_dense_tool_gpu.py with and
without the flags.  The logs and results of the existing entries are those of the run without, the new entries ``<source>_contour`` and
``<source>_icp_contour`` exist with their summary lines, and they compose with ``--icp``, ``--verify``, ``--bop`` and ``--ppf``."""
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
    root = tmp_path_factory.mktemp("cad_eval_render_contour")
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
    con = tool.main(_eval_args(files, files["root"] / "contour") + ["--contour", "2"])
    assert sorted(plain) == ["truth"] and sorted(con) == ["truth", "truth_contour"]
    assert con["truth"] == plain["truth"] and "contour" not in con["truth"]
    assert _log(files, "contour", "truth") == _log(files, "plain", "truth") and not any("contour" in line for line in _log(files, "plain", "truth"))
    d = con["truth_contour"]
    served = sum(plain["truth"]["served"])
    assert served >= 3 and d["served"] == plain["truth"]["served"] and d["kept"] == plain["truth"]["kept"] and d["source"] == "truth_contour"
    m = d["contour"]
    assert m["items"] == served and m["gate"] == 16 and m["margin"] == 8 and m["mask"] is False and m["bad_item"] == 0
    assert m["contour_scale"] == 0.1 and m["reach"] == 6 and m["edge_step"] == 65535 and m["mean_first_pairs"] >= 0 and m["mean_last_pairs"] >= 0
    assert 0 <= m["few"] + m["degenerate"] <= served and 0.0 <= m["mean_steps"] <= 2.0 and "dense" not in d
    own = [line for line in _log(files, "contour", "truth_contour") if line.startswith("[truth_contour masks] contour")]
    assert len(own) == 2
    assert own[0] == ("[truth_contour masks] contour 2 steps gate 16, scale 0.1, reach 6, edge step 65535: %d items, %d few inliers, %d degenerate "
                      "left alone" % (served, m["few"], m["degenerate"]))
    assert own[1].startswith("[truth_contour masks] contour: mean rms ") and ", mean outline pairs " in own[1] and own[1].count(" -> ") == 2
    masked = tool.main(_eval_args(files, files["root"] / "masked") + ["--contour", "2", "--contour_gate", "300", "--contour_mask", "--contour_scale", "1",
                                                                      "--contour_reach", "3", "--contour_edge_step", "500"])
    mm = masked["truth_contour"]["contour"]
    assert mm["mask"] is True and mm["gate"] == 300 and mm["items"] == served and masked["truth"] == plain["truth"] and mm["mean_first_pairs"] > 0
    assert any(line.startswith("[truth_contour masks] contour 2 steps gate 300 masked, scale 1, reach 3, edge step 500: ")
               for line in _log(files, "masked", "truth_contour"))
    for bad in (["--contour", "65"], ["--contour", "-1"], ["--contour", "1", "--contour_gate", "65536"], ["--contour", "1", "--contour_reach", "65"],
                ["--contour", "1", "--contour_edge_step", "-1"], ["--contour", "1", "--contour_scale", "-1"], ["--contour", "1", "--contour_scale", "nan"],
                ["--ppf_contour"]):
        with pytest.raises(SystemExit):
            tool.main(_eval_args(files, files["root"] / "bad") + bad)


def test_the_new_entries_compose_with_icp_verify_bop_and_ppf(files):
    tool = _tool("eval_cad_render")
    ppf = ["--ppf", "2", "--ppf_points", "200", "--ppf_ref_step", "2", "--ppf_gate", "2000", "--ppf_dense", "3", "--ppf_dense_gate", "2000"]
    args = _eval_args(files, files["root"] / "base") + ["--icp", "2", "--verify", "--bop"] + ppf
    base = tool.main(args)
    args[args.index(str(files["root"] / "base"))] = str(files["root"] / "all")
    both = tool.main(args + ["--contour", "2", "--contour_gate", "200"])
    assert sorted(base) == ["truth", "truth_icp", "truth_icp_best", "truth_ppf"]
    assert sorted(both) == ["truth", "truth_contour", "truth_icp", "truth_icp_best", "truth_icp_contour", "truth_ppf"]
    for entry in base:
        assert both[entry] == base[entry], entry
        assert _log(files, "all", entry) == _log(files, "base", entry), entry
    served = sum(base["truth"]["served"])
    for entry in ("truth_contour", "truth_icp_contour"):
        r = both[entry]
        assert r["contour"]["items"] == served and r["verify"]["items"] == served and r["bop"]["items"] == served and r["bop"]["bad_items"] == 0
        assert ("icp" in r) == (entry == "truth_icp_contour")
        lines = _log(files, "all", entry)
        for head in ("contour 2 steps gate 200, scale 0.1, ", "contour: mean rms ", "verify tol 4 margin 8: ", "bop: "):
            assert any(line.startswith("[%s masks] %s" % (entry, head)) for line in lines), (entry, head)
    assert any(line.startswith("[truth_icp_contour masks] ICP 2 steps: ") for line in _log(files, "all", "truth_icp_contour"))
    # the PPF chain's cluster steps with the outline term
    args[args.index(str(files["root"] / "all"))] = str(files["root"] / "chain")
    chain = tool.main(args + ["--ppf_contour", "--contour_scale", "0.2"])
    assert sorted(chain) == sorted(base)
    for entry in ("truth", "truth_icp", "truth_icp_best"):
        assert chain[entry] == base[entry] and _log(files, "chain", entry) == _log(files, "base", entry), entry
    r, b = chain["truth_ppf"], base["truth_ppf"]
    assert r["ppf"]["contour"] == dict(edge_step=65535, reach=6, contour_scale=0.2) and "contour" not in b["ppf"]
    assert r["ppf"]["items"] == served and r["verify"]["items"] == served and r["bop"]["items"] == served
    assert {k: v for k, v in r["ppf"].items() if k != "contour" and k != "kept_rank"} == {k: v for k, v in b["ppf"].items() if k != "kept_rank"}, \
        "the votes do not depend on the refiner"
    lines = _log(files, "chain", "truth_ppf")
    assert "[truth_ppf masks] ppf: the cluster steps carry the outline term, scale 0.2, reach 6, edge step 65535" in lines
    assert not any("outline" in line for line in _log(files, "base", "truth_ppf"))
