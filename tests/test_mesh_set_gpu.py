"""GPU: one ``MeshSet`` per ``RenderedPoseDataset``: the scene renderer, ``mesh_icp()`` and ``pose_verifier()`` read the same device
arrays, and give what wrappers built from plain lists of meshes give."""
import math

import numpy as np
import pytest
import torch

import fabricate_cad as fab
import mesh_closest_np as m
import mesh_icp_np as icp

pytestmark = pytest.mark.gpu
FRAMES, TOL, MARGIN = 16, 4, 8


def _models():
    """two bracket-sized models (24 triangles each) and a tetrahedron distractor, with colours"""
    rng = np.random.default_rng(5)
    (bv, bt), (tv, tt) = m.bracket(), m.scalene_tetrahedron()
    col = lambda v: rng.integers(0, 256, (len(v), 3), dtype=np.uint8)
    models = [(bv * np.float32(30.0), bt, col(bv)), (bv * np.float32(24.0), bt, col(bv))]
    return models, (tv * np.float32(40.0), tt, col(tv))


def _last_error(call):
    from densefusion_amd import _lib
    with pytest.raises(RuntimeError):
        call()
    return _lib.lib().df_last_error().decode()


def test_dataset_wrappers_share_one_set_and_equal_the_list_route():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from densefusion_amd.datasets.customCAD.online import RenderedPoseDataset
    from densefusion_amd.lib.mesh_icp import MeshIcp
    from densefusion_amd.lib.pose_verify import PoseVerifier
    models, distractor = _models()
    ds = RenderedPoseDataset(models, 500, False, 0.0, False, distractors=[distractor], scene=True, proj_mat=fab.PROJ[1], image_dims=(64, 96),
                             min_pixels=60, frames=FRAMES, chunk=8, keep_frames=True)
    fit, ver, ver2 = ds.mesh_icp(), ds.pose_verifier(), ds.pose_verifier()
    # -- sharing ---------------------------------------------------------------------------------------------------------------------
    assert ds.renderer.triangles.data_ptr() == fit.triangles.data_ptr() == ver.triangles.data_ptr() == ver2.triangles.data_ptr()
    assert ver.vertices.data_ptr() == ds.renderer.vertices.data_ptr() and fit.vertices.data_ptr() != ds.renderer.vertices.data_ptr()
    assert ds.renderer.n_objects == 3 and ds.renderer.tri_begin.tolist() == [0, 24, 48, 52]
    assert ver.n_objects == fit.n_objects == 2 and ver.tri_begin.tolist() == fit.tri_begin.tolist() == [0, 24, 48], "no distractor"
    assert tuple(ver.triangles.shape) == (48, 3) and tuple(ver.vertices.shape) == tuple(fit.vertices.shape) == (2 * len(models[0][0]), 3)
    assert ver is not ver2 and ver._scratch is None and ver2._scratch is None
    # -- the old route: wrappers from plain lists ----------------------------------------------------------------------------------------
    plain = [(v, t) for v, t, _ in models]
    fit0 = MeshIcp(plain, ds.model_scale / 10000.0)
    ver0 = PoseVerifier(plain, ds.model_scale, ds.proj_mat, ds.image_dims, cloud_div=10000.0)
    assert fit0.triangles.data_ptr() != fit.triangles.data_ptr()
    assert torch.equal(fit0.vertices, fit.vertices) and torch.equal(fit0.triangles, fit.triangles)
    assert torch.equal(ver0.vertices, ver.vertices) and torch.equal(ver0.triangles, ver.triangles)
    live = [i for i in range(FRAMES) if ds.view_info(i)["live"]]
    print("live views:", live)
    assert len(live) >= 1
    infos = [ds.view_info(i) for i in live]
    B, rng = len(live), np.random.default_rng(9)
    D = icp.diameter(fit.vertices.cpu().numpy())
    starts = [icp.perturb(np.concatenate([icp.quat_from_matrix(f["pose"][:, :3]), f["pose"][:, 3] / 10000.0]), rng, math.radians(2), 0.02 * D)
              for f in infos]
    before = torch.from_numpy(np.stack(starts)).cuda()
    clouds = torch.stack([ds[i][0].reshape(-1, 3) for i in live]).float().contiguous()
    obj = torch.tensor([f["object"] - 1 for f in infos], dtype=torch.int32, device="cuda")
    (after, stats), (after0, stats0) = fit.refine(clouds, before, obj, iters=3), fit0.refine(clouds, before, obj, iters=3)
    assert torch.equal(after, after0) and torch.equal(stats, stats0), "ICP: the shared set equals the list route"
    depth, mask = torch.stack([f["depth"] for f in infos]), torch.stack([f["mask"] for f in infos])
    window = (max(f["box"][1] - f["box"][0] for f in infos) + 2 * MARGIN, max(f["box"][3] - f["box"][2] for f in infos) + 2 * MARGIN)
    corner = torch.tensor([[f["box"][0] - MARGIN, f["box"][2] - MARGIN] for f in infos], dtype=torch.int32, device="cuda")
    frame = torch.arange(B, dtype=torch.int32, device="cuda")
    for pose in (before, after):
        got, got2, want = (v.score(depth, pose, frame, obj, corner, window, TOL, mask=mask, cull=bool(ds.cull)) for v in (ver, ver2, ver0))
        print("tallies:", got.tolist())
        assert got.shape == (B, 12) and torch.equal(got, want) and torch.equal(got2, want), "verify: the shared set equals the list route"
        assert (got[:, 0] == 0).all() and (got[:, 1] > 0).all(), "every item is drawn: the pose is 2 degrees and 0.02 D off the rendered one"
    assert ver._scratch.data_ptr() != ver2._scratch.data_ptr(), "every wrapper has its own scratch"
    # -- the one tri_begin check: the same text from both entry points, apart from the name in front -----------------------------------------
    ver3 = PoseVerifier(models + [distractor], ds.model_scale, ds.proj_mat, ds.image_dims, cloud_div=10000.0)       # O = 3, T = 52 as the renderer
    good = ds.renderer.tri_begin
    assert ver3.tri_begin.tolist() == good.tolist()
    poses = np.tile(np.concatenate([np.eye(3), [[0.0], [0.0], [-4000.0]]], axis=1), (1, 3, 1, 1))
    for bad, text in (([1, 24, 48, 52], "tri_begin[0] = 1, not 0"), ([0, 50, 48, 52], "tri_begin decreases from 50 to 48 at object 1"),
                      ([0, 24, 48, 51], "tri_begin[O] = 51, not T = 52")):
        ds.renderer.tri_begin = ver3.tri_begin = np.array(bad, dtype=np.int32)
        scene = _last_error(lambda: ds.renderer.render(poses))
        verify = _last_error(lambda: ver3.score(depth, before, frame, obj, corner, window, TOL))
        assert scene == "cad_render_scene: " + text and verify == "pose_verify: " + text
    ds.renderer.tri_begin = ver3.tri_begin = good
    ds.renderer.render(poses)
    assert torch.equal(ver3.score(depth, before, frame, obj, corner, window, TOL), ver.score(depth, before, frame, obj, corner, window, TOL))
