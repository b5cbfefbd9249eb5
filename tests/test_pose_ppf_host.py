"""CPU: the restatement of ``df_pose_ppf`` (tests/pose_ppf_np.py).  Quality is asserted here: the device is bit-equal to the restatement
(tests/test_pose_ppf_gpu.py), so what holds here holds there.  The chain: top K = 4 clusters, each refined by 10 steps of ``dense_np``,
each scored by ``verify_np``, the highest visible-surface IoU kept, on the bracket and ``box(1, 2, 3)`` frames of
tests/test_pose_dense_host.py (48 x 64, +-2 codes of noise) and on three more bracket poses that show three faces.  The unit rules: the
bins against ``acos`` and ``atan2``, the local frame at n = +-e_x, the model table's order (numpy and ``df_ppf_model_build``, a host
function, bit for bit), the dropped pairs, the cluster order under equal votes.

What differs from the defaults of ``PpfEstimator.estimate`` and why: ``gate`` is 3000 codes, the gate of the dense test on the same
frames (neighbouring nodes of a 48 x 64 frame lie hundreds of codes apart; 16 codes leave no node a normal), and ``ref_step`` is 3, not
5: with every fifth grid row and column a 48 x 64 frame has 10 to 12 usable references, and the bracket's good cluster (5.3 degrees, 0.042
diameters off, rank 1) then ends 0.083 diameters off after the ten dense steps; with every third it has 33 and ends at 9e-6."""
import ctypes
import math

import numpy as np
import pytest

import mesh_closest_np as m
import mesh_icp_np as icp
import pose_dense_np as dn
import pose_error_np as pe
import pose_ppf_np as pp
import pose_verify_np as pv

IH, IW = 48, 64
PROJ = np.array(pv.PROJ, dtype=np.float64)
CLOUD_DIV, SCALE = 10000.0, 600.0
MESH = {"box": m.box(1, 2, 3), "bracket": m.bracket()}
IDENT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)[None]
GATE, REF_STEP, K = 3000, 3, 4
# the poses of tests/test_pose_dense_host.py, then three more of the bracket chosen with the restatement among random poses whose camera
# centre, in the model frame, has every component above 0.25 of its length (three faces of the bracket's box show)
POSES = {"box": [[0.85, 0.25, -0.35, 0.3, 0.01, -0.005, -0.40]],
         "bracket": [[0.8, 0.35, -0.3, 0.4, -0.015, 0.01, -0.41], [0.09, -0.41, -0.32, 0.85, 0.009, 0.001, -0.42],
                     [0.36, -0.28, -0.89, 0.09, 0.006, 0.007, -0.4], [0.58, -0.01, -0.79, -0.2, -0.02, 0.003, -0.4]]}


def _box_symmetries():
    """The proper symmetries of a box with three different sides: the identity and the half turns about its three axes."""
    out = [IDENT[0]]
    for ax in range(3):
        R = -np.eye(3)
        R[ax, ax] = 1.0
        out.append(np.concatenate([R, np.zeros((3, 1))], axis=1))
    return np.stack(out)


SYM = {"box": _box_symmetries(), "bracket": IDENT}


def _scene(name, pose, noise=2, seed=4):
    """``test_pose_dense_host._scene`` at any pose: one frame drawn by the raster restatement, +-noise codes, a mask that is 1 where it drew."""
    v, t, begin = icp.concat_meshes([MESH[name]])
    codes, _ = dn.render_codes(v, t, 0, len(t), SCALE, PROJ, pose, CLOUD_DIV, IH, IW)
    drawn = codes != 65535
    obs = np.where(drawn, np.clip(codes + np.random.default_rng(seed).integers(-noise, noise + 1, codes.shape), 0, 65534), 65535)
    return dict(vertices=v, triangles=t, tri_begin=begin, model_scale=np.array([SCALE]), proj=PROJ, rays=dn.ray_map(PROJ, IH, IW),
                depth=obs[None].astype(np.uint16), mask=drawn[None].astype(np.uint16))


def _angle(qa, qb):
    Ra, Rb = np.array(icp.quat_to_mat([float(e) for e in qa])), np.array(icp.quat_to_mat([float(e) for e in qb]))
    return math.degrees(math.acos(max(-1.0, min(1.0, (float(np.trace(Ra @ Rb.T)) - 1.0) / 2.0))))


@pytest.fixture(scope="module")
def models():
    return {name: pp.make_model([pp.sample_mesh(*MESH[name], 400, 1, SCALE / CLOUD_DIV)]) for name in MESH}


def _three_faces(pose):
    o = -np.array(icp.quat_to_mat([float(e) for e in pose[:4]])).T @ pose[4:]
    return float((np.abs(o) / np.linalg.norm(o)).min())


@pytest.mark.parametrize("name,k", [(n, k) for n in ("bracket", "box") for k in range(len(POSES[n]))])
def test_chain_from_no_pose_to_the_exact_one(models, name, k):
    """K = 4, 10 degrees, 0.1 and 0.01 diameters are the conditions; what is printed is measured."""
    truth = icp.normalised(np.array(POSES[name][k], dtype=np.float64))
    sc, model = _scene(name, truth), models[name]
    if k > 0:
        assert _three_faces(truth) >= 0.25, "the added poses show three faces"
    clusters, refined, iou, kept, stats = pp.chain_np(sc, model, np.array([[0, 0, 0, 0, 0, 1]]), IH, IW, K=K, gate=GATE, ref_step=REF_STEP,
                                                      mask=sc["mask"])
    x = sc["vertices"].astype(np.float64) * (SCALE / CLOUD_DIV)
    diam = icp.diameter(x)
    Rt = np.array(icp.quat_to_mat([float(e) for e in truth[:4]]))
    near = []
    for c in clusters[0]:                                           # the cluster against the truth composed with each proper symmetry
        near.append(min((_angle(c[:4], icp.quat_mul(truth[:4], icp.quat_from_matrix(S[:, :3]))),
                         float(np.linalg.norm(c[4:] - (truth[4:] + Rt @ S[:, 3]))) / diam) for S in SYM[name]))
    mssd = [math.sqrt(pe.item_maxima(x, p, truth, SYM[name], PROJ, IH, IW)[0].min()) / diam for p in refined[0]]
    print(f"{name} {k}: ppf stats {stats[0].tolist()}, clusters (degrees, diameters) {[(round(a, 2), round(d, 4)) for a, d in near]}, "
          f"IoU {np.round(iou[0], 3).tolist()}, kept rank {int(kept[0])}, MSSD / diameter after 10 steps {['%.2e' % e for e in mssd]}")
    assert stats[0, 0] == pp.OK
    assert any(a <= 10.0 and d <= 0.1 for a, d in near), "one of the top 4 clusters lies within 10 degrees and 0.1 diameter of the truth"
    assert mssd[int(kept[0])] < 0.01, "the candidate with the highest IoU ends below 0.01 diameter"


def test_bins_agree_with_acos_and_atan2():
    NANG, NA = 15, 30
    ang_cos, alpha_cos, alpha_cs = pp.tables(NANG, NA)
    rng = np.random.default_rng(0)
    c = rng.uniform(-1.0, 1.0, 10000)
    a = np.arccos(c) / (math.pi / NANG)
    away = np.abs(a - np.round(a)) > 1e-6
    assert away.sum() > 9900 and np.array_equal(pp.bins(ang_cos, c)[away], np.floor(a).astype(np.int64)[away])
    assert np.array_equal(pp.bins(ang_cos, ang_cos), np.arange(1, NANG)), "a value on boundary k lies in the bin above it"
    assert pp.bins(ang_cos, [1.0, -1.0, np.nextafter(ang_cos[3], 2.0)]).tolist() == [0, NANG - 1, 3]
    am, as_ = rng.uniform(-math.pi, math.pi, 10000), rng.uniform(-math.pi, math.pi, 10000)
    d = np.mod(am - as_, 2.0 * math.pi) / (2.0 * math.pi / NA)
    away = (np.abs(d - np.round(d)) > 1e-6)
    got = pp.sector(np.cos(am), np.sin(am), np.cos(as_), np.sin(as_), alpha_cos, NA)
    assert away.sum() > 9900 and np.array_equal(got[away], np.floor(d).astype(np.int64)[away])
    assert np.array_equal(np.floor(np.mod(np.arctan2(alpha_cs[:, 1], alpha_cs[:, 0]), 2.0 * math.pi) / (2.0 * math.pi / NA)).astype(int), np.arange(NA))
    s = np.sqrt(1.0 - alpha_cos * alpha_cos)
    one, zero = np.ones_like(s), np.zeros_like(s)
    assert np.array_equal(pp.sector(alpha_cos, s, one, zero, alpha_cos, NA), np.arange(1, NA // 2)), "on boundary k with s >= 0: sector k"
    assert np.array_equal(pp.sector(alpha_cos, -s, one, zero, alpha_cos, NA), NA - 1 - np.arange(1, NA // 2)), "and with s < 0: NA - 1 - k"
    assert pp.sector(np.array([1.0, -1.0, 1.0]), np.array([0.0, 0.0, -0.0]), one[:3], zero[:3], alpha_cos, NA).tolist() == [0, NA // 2 - 1, 0]


def test_local_frame():
    assert np.array_equal(pp.frame_rot(np.array([1.0, 0.0, 0.0])), np.eye(3))
    assert np.array_equal(pp.frame_rot(np.array([-1.0, 0.0, 0.0])), np.diag([-1.0, -1.0, 1.0]))
    eps = 2.0 ** -20
    below = np.array([-1.0 + eps / 2, math.sqrt(1.0 - (1.0 - eps / 2) ** 2), 0.0])
    at = np.array([-1.0 + eps, math.sqrt(1.0 - (1.0 - eps) ** 2), 0.0])
    assert np.array_equal(pp.frame_rot(below), np.diag([-1.0, -1.0, 1.0])) and not np.array_equal(pp.frame_rot(at), np.diag([-1.0, -1.0, 1.0]))
    rng = np.random.default_rng(1)
    n = rng.normal(size=(1000, 3))
    n /= np.linalg.norm(n, axis=1)[:, None]
    R = pp.frame_rot(n)
    assert np.abs(np.einsum("nij,nj->ni", R, n) - np.array([1.0, 0.0, 0.0])).max() < 1e-9, "R n = e_x"
    assert np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max() < 1e-9 and np.abs(np.linalg.det(R) - 1.0).max() < 1e-9
    # the angle of a point is the turn about +x that brings it to z = 0, y > 0
    ok, c, s = pp.frame_angle(np.eye(3), np.zeros(3), np.array([[5.0, 0.0, 2.0], [1.0, 3.0, 0.0], [1.0, 0.0, 0.0]]))
    assert ok.tolist() == [True, True, False] and (c[0], s[0], c[1], s[1]) == (0.0, -1.0, 1.0, 0.0)
    # the hypothesis of a pair puts the model point on the scene point and the model normal on the scene normal
    pm, nm, ps, ns = rng.normal(size=3), n[0], rng.normal(size=3), n[1]
    pose = pp.hypothesis_pose(ps, ns, pm, nm, math.cos(0.7), math.sin(0.7))
    Rh = np.array(icp.quat_to_mat(pose[:4]))
    assert np.abs(Rh @ pm + pose[4:] - ps).max() < 1e-12 and np.abs(Rh @ nm - ns).max() < 1e-12 and pose[0] >= 0


@pytest.fixture(scope="module")
def library():
    import __graft_entry__ as g
    g.build()
    from densefusion_amd import _lib
    return _lib.lib()


def _build_c(L, pts, nrm, begin, dist_step, ND, NANG, NA, ang_cos):
    begin, dist_step = np.ascontiguousarray(begin, dtype=np.int32), np.ascontiguousarray(dist_step, dtype=np.float64)
    pts, nrm, ang_cos = np.ascontiguousarray(pts, dtype=np.float64), np.ascontiguousarray(nrm, dtype=np.float64), np.ascontiguousarray(ang_cos)
    nb, ne, used = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.df_ppf_model_sizes(begin.ctypes.data, len(begin) - 1, ND, NANG, ctypes.addressof(nb), ctypes.addressof(ne)) == 0
    bb, ep, ec = np.full(nb.value, -7, dtype=np.int32), np.full(ne.value, -7, dtype=np.int32), np.full((ne.value, 2), 9.0, dtype=np.float32)
    rc = L.df_ppf_model_build(pts.ctypes.data, nrm.ctypes.data, len(pts), begin.ctypes.data, dist_step.ctypes.data, len(begin) - 1, ND, NANG, NA,
                              ang_cos.ctypes.data, bb.ctypes.data, ep.ctypes.data, ec.ctypes.data, ctypes.addressof(used))
    return rc, bb.reshape(len(begin) - 1, -1), ep[:used.value], ec[:used.value], ne.value


def test_model_table_order_and_the_library_builder(library):
    """Two objects of 40 and 17 samples: the entries of a key are in ascending (i, j), the objects follow one another, and the host
    function of the library writes the restatement's bytes."""
    clouds = [pp.sample_mesh(*MESH["bracket"], 40, 2, SCALE / CLOUD_DIV), pp.sample_mesh(*MESH["box"], 17, 3, SCALE / CLOUD_DIV)]
    mod = pp.make_model(clouds, NANG=6, NA=30)
    ND, NANG = mod["ND"], mod["NANG"]
    ang_cos = pp.tables(NANG, 30)[0]
    at = 0
    for o, (P, N) in enumerate(clouds):
        want = {}
        for i in range(len(P)):
            for j in range(len(P)):
                key = int(pp.pair_keys(P[i], N[i], P[j], N[j], mod["dist_step"][o], ND, NANG, ang_cos)) if i != j else -1
                if key >= 0:
                    want.setdefault(key, []).append(i)
        bb = mod["bucket_begin"][o]
        assert bb[0] == at and (np.diff(bb) >= 0).all()
        for key in range(ND * NANG ** 3):
            assert mod["entry_point"][bb[key]:bb[key + 1]].tolist() == want.get(key, []), f"object {o}, key {key}"
        at = bb[-1]
    assert at == len(mod["entry_point"]) and mod["entry_cs"].dtype == np.float32
    assert np.abs(np.hypot(mod["entry_cs"][:, 0].astype(np.float64), mod["entry_cs"][:, 1]) - 1.0).max() < 1e-6
    rc, bb, ep, ec, cap = _build_c(library, mod["points"], mod["normals"], mod["point_begin"], mod["dist_step"], ND, NANG, 30, ang_cos)
    assert rc == 0 and cap == 40 * 39 + 17 * 16
    assert bb.tobytes() == mod["bucket_begin"].tobytes() and ep.tobytes() == mod["entry_point"].tobytes() and ec.tobytes() == mod["entry_cs"].tobytes()
    big = pp.make_model([pp.sample_mesh(*MESH["bracket"], 400, 1, SCALE / CLOUD_DIV)])
    rc, bb, ep, ec, _ = _build_c(library, big["points"], big["normals"], big["point_begin"], big["dist_step"], big["ND"], 15, 30, pp.tables(15, 30)[0])
    assert rc == 0 and bb.tobytes() == big["bucket_begin"].tobytes() and ep.tobytes() == big["entry_point"].tobytes() and ec.tobytes() == big["entry_cs"].tobytes()
    print("bracket, 400 samples:", len(ep), "entries, longest bucket", int(np.diff(bb[0]).max()))


def test_dropped_pairs_and_builder_refusals(library):
    ang_cos = pp.tables(15, 30)[0]
    p = np.array([[0.0, 0.0, 0.0], [0.3, 0.0, 0.1], [0.0, 0.0, 0.0], [0.1, 0.2, 0.0], [5.0, 0.0, 0.0], [0.0, 0.4, 0.0]])
    n = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [np.nan, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0]])
    key = pp.pair_keys(p[:, None], n[:, None], p[None, :], n[None, :], 0.1, 20, 15, ang_cos)
    assert key[0, 1] >= 0 and key[0, 2] == key[2, 0] == -1, "a coincident pair is dropped"
    assert (key[3] == -1).all() and (key[:, 3] == -1).all(), "a NaN normal drops every pair it is in"
    assert (key[4] == -1).all() and (key[:, 4] == -1).all(), "50 steps away: outside ND = 20"
    edge = lambda y: int(pp.pair_keys(p[0], n[0], np.array([0.0, y, 0.0]), n[5], 0.125, 16, 15, ang_cos))
    assert key[0, 5] >= 0 and edge(2.0) == -1 and edge(np.nextafter(2.0, 0.0)) >= 0, "L / dist_step = ND exactly is outside, one ulp below is the last bin"
    ok, _, _ = pp.frame_angle(pp.frame_rot(n[0]), p[0], np.array([0.0, 0.0, 0.7]))
    assert not ok, "a point on the normal's axis has no angle"
    begin = np.array([0, 6], dtype=np.int32)
    bb, ep, ec = pp.model_build(p, n, begin, [0.1], 20, 15, 30, ang_cos)
    rc, cb, cp, cc, _ = _build_c(library, p, n, begin, [0.1], 20, 15, 30, ang_cos)
    assert rc == 0 and cb.tobytes() == bb.tobytes() and cp.tobytes() == ep.tobytes() and cc.tobytes() == ec.tobytes()
    assert 3 not in ep and 4 not in ep and len(ep) == int((key >= 0).sum()) - int(((key >= 0) & ~pp.frame_angle(pp.frame_rot(n)[:, None], p[:, None], p[None, :])[0]).sum())
    refused = [dict(NA=29), dict(NA=66), dict(ND=0), dict(ND=65), dict(NANG=33), dict(dist_step=[0.0]), dict(dist_step=[np.inf]), dict(begin=[0, 5]),
               dict(begin=[1, 6]), dict(ang=ang_cos[::-1].copy())]
    for change in refused:
        a = dict(begin=begin, dist_step=[0.1], ND=20, NANG=15, NA=30, ang=ang_cos)
        a.update(change)
        nb, ne = ctypes.c_size_t(0), ctypes.c_size_t(0)
        if library.df_ppf_model_sizes(np.ascontiguousarray(a["begin"], dtype=np.int32).ctypes.data, 1, a["ND"], a["NANG"], ctypes.addressof(nb), ctypes.addressof(ne)):
            continue
        rc, cb, cp, _, _ = _build_c(library, p, n, a["begin"], a["dist_step"], a["ND"], a["NANG"], a["NA"], a["ang"])
        assert rc == -1 and (cb == -7).all() and len(cp) == 0, f"{change}: refused before anything is written"
    one = np.array([0, 1], dtype=np.int32)
    nb, ne = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert library.df_ppf_model_sizes(one.ctypes.data, 1, 20, 15, ctypes.addressof(nb), ctypes.addressof(ne)) == -1, "one point makes no pair"
    lds = np.array([0, 1024], dtype=np.int32)
    big = np.zeros((1024, 3))
    assert _build_c(library, big, big, lds, [0.1], 2, 2, 38, pp.tables(2, 38)[0])[0] == -1 and b"LDS" in library.df_last_error()


def test_cluster_order_with_equal_votes():
    """Hand-made hypotheses: equal votes go by the reference index, a hypothesis joins the FIRST cluster that fits although a later one
    fits better, a cluster's pose is its first member's, and equal scores go by creation order."""
    q = lambda deg: icp.quat_from_axis_angle([0.0, 0.0, 1.0], math.radians(deg))
    t0 = np.zeros(3)
    hyp = np.zeros((9, 8))
    rows = {7: (q(0), t0, 5), 2: (q(20), t0, 5), 5: (q(10), t0, 5), 1: (q(100), t0, 4), 0: (q(100), np.array([0.5, 0, 0]), 4),
            3: (q(0), np.array([0.09, 0, 0]), 1), 8: (q(30), t0, 9)}
    for r, (qq, tt, v) in rows.items():
        hyp[r, :4], hyp[r, 4:7], hyp[r, 7] = qq, tt, v
    pose, votes, nh, nc = pp.cluster_np(hyp, pp.cluster_trace(15.0), 0.1, 4)
    # order: 8 (9 votes); then 2, 5, 7 (5 votes, by index): 2 (20 degrees) joins 8 (30 degrees); 5 (10) joins 8's cluster?  No: 20 degrees
    # from its first member, it founds; 7 (0 degrees) is 10 from 5 and joins it; 0 and 1 (4 votes): 0 founds, 1 is 0.5 away and founds;
    # 3 joins the cluster of 5 (0 degrees against 10, 0.09 away)
    assert (nh, nc) == (7, 4)
    assert votes.tolist() == [[14, 2], [11, 3], [4, 1], [4, 1]], "scores 9 + 5, 5 + 5 + 1, and the two of 4 in creation order"
    assert m.same_bits(pose[0], hyp[8, :7]) and m.same_bits(pose[1], hyp[5, :7]) and m.same_bits(pose[2], hyp[0, :7]) and m.same_bits(pose[3], hyp[1, :7])
    pose, votes, _, _ = pp.cluster_np(hyp, pp.cluster_trace(15.0), 0.1, 6)
    assert votes[4:].tolist() == [[0, 0], [0, 0]] and not pose[4:].any(), "missing ranks are zero"
    # on the boundary: trace = the threshold itself joins, the distance itself joins
    thr = pp.cluster_trace(15.0)
    two = np.zeros((2, 8))
    two[0, :4], two[0, 7], two[1, :4], two[1, 4], two[1, 7] = q(0), 3, q(0), 0.25, 2
    assert pp.cluster_np(two, thr, 0.25, 2)[3] == 1 and pp.cluster_np(two, thr, np.nextafter(0.25, 0.0), 2)[3] == 2
    assert pp.cluster_np(two, 3.0, 0.25, 2)[3] == 1 and pp.cluster_np(two, np.nextafter(3.0, 4.0), 0.25, 2)[3] == 2
