"""CPU: the rule of ``df_mesh_closest`` restated twice (tests/mesh_closest_np.py) agrees with itself bit for bit on the shapes the GPU
test walks, and ``detect_symmetry`` on top of the restatement classifies the fixture meshes (DESIGN.md 12i records the residuals)."""
import numpy as np
import pytest

import mesh_closest_np as m
from densefusion_amd.datasets.customCAD.symmetry import SymmetryReport, detect_symmetry, parse_sym_option

TILE = 128                      # any value: the restatements have no tile; the GPU test takes the library's
SCALAR_PAIRS = 60000            # the plain-Python restatement walks every pair: it takes the cases up to this many


@pytest.mark.parametrize("name", sorted(m.make_cases(TILE)))
def test_the_two_restatements_agree(name):
    v, t, p, xf = m.make_cases(TILE)[name]
    assert len(xf) * len(p) * len(t) <= SCALAR_PAIRS
    a, b = m.closest_np(v, t, p, xf), m.closest_scalar(v, t, p, xf)
    assert all(m.same_bits(x, y) for x, y in zip(a, b))
    assert m.closest_np(v, t, p, xf, want_closest=False)[2] is None


def test_the_cases_are_what_they_claim():
    cases = m.make_cases(TILE)
    for T in (1, TILE - 1, TILE, TILE + 1):
        assert (m.closest_np(*cases["T%d" % T])[1] == T - 1).all(), "the last triangle wins"
    v, t, q, want = m.region_case()
    d2, tri, c = m.closest_np(v, t, q, m.IDENTITY[None])
    assert np.array_equal(c[0], want) and np.allclose(d2[0], ((q - want) ** 2).sum(axis=1), rtol=1e-15, atol=0)
    v, t, q, owner = m.shared_edge_case()
    d2, tri, c = m.closest_np(v, t, q, m.IDENTITY[None])
    assert np.array_equal(tri[0], owner) and (d2 == 0).all() and np.array_equal(c[0], q), "the lowest index wins a tie, d = 0 on the surface"
    d2, tri, c = m.closest_np(*cases["degenerate"])
    assert set(np.unique(tri)) <= {3, 4, 5} and {3, 4} <= set(np.unique(tri)), "dropped triangles never win; the edge-only ones do"
    assert tri[0, 0] == 4 and d2[0, 0] == 0.0, "a query on the doubled vertex: the triangle with the zero-length edge, through its other edges"
    v, t, p, xf = cases["all_dropped"]
    d2, tri, c = m.closest_np(v, t, p, xf)
    assert (tri == -1).all() and np.isposinf(d2).all() and m.same_bits(c, m.transform_np(p, xf))
    p = p.copy()
    p[2, 1] = np.nan
    bv, bt = m.bracket()
    d2, tri, c = m.closest_np(bv, bt, p, xf)
    assert (tri[:, 2] == -1).all() and np.isposinf(d2[:, 2]).all() and np.isnan(c[:, 2]).any(axis=1).all() and (tri[:, [0, 1, 3, 4]] >= 0).all()


def _detect(mesh, colors=None, **kw):
    return detect_symmetry(mesh[0], mesh[1], colors, closest=m.closest_np, **kw)


def _orders(report, axis):
    """the orders that passed about the candidate axis parallel to ``axis``"""
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    return sorted(n for a, n, _, _ in report.passed if abs(abs(float(report.axes[a] @ axis)) - 1) < 1e-6)


def test_exact_symmetries_are_found_to_rounding():
    r = _detect(m.box(1, 2, 3))
    assert isinstance(r, SymmetryReport) and r.symmetric and r.D == pytest.approx(np.sqrt(14.0)) and np.allclose(r.centroid, 0, atol=1e-12)
    assert all(_orders(r, a) == [2] for a in np.eye(3)) and len(r.passed) == 3 and max(p[2] for p in r.passed) < 1e-14
    print("box(1,2,3)", max(p[2] for p in r.passed))
    r = _detect(m.box(1, 1, 1))
    assert r.symmetric and all(_orders(r, a) == [2, 4] for a in np.eye(3)) and max(p[2] for p in r.passed) < 1e-14
    print("cube", max(p[2] for p in r.passed))
    r = _detect(m.prism(5, 1, 1.5))
    # the ring is stored in fp32: a vertex and its image each sit within 2^-24 per coordinate of the exact ring, 1.7e-7 apart at most, over D = 3.02
    assert r.symmetric and _orders(r, (0, 0, 1)) == [5] and max(p[2] for p in r.passed) < 1e-7
    print("prism(5)", max(p[2] for p in r.passed))
    r = _detect(m.regular_tetrahedron())
    assert r.symmetric and all(_orders(r, a) == [3] for a in ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))) and max(p[2] for p in r.passed) < 1e-14
    print("regular tetrahedron", max(p[2] for p in r.passed))
    assert "symmetric: yes" in str(r) and "orders 3" in str(r)


def test_tessellated_round_bodies_pass_within_tol():
    """Fewer candidates than the defaults, to keep the numpy restatement quick: the principal axes only, orders up to 3 and the probe."""
    r = _detect(m.prism(64, 1, 1.5), axes=0, max_order=3, samples=256)
    probe = [p for p in r.passed if p[1] == 0]
    assert r.symmetric and _orders(r, (0, 0, 1)) == [0, 2, 3] and len(probe) == 1 and 1e-4 < probe[0][2] < 1e-3      # the chord error of 64 sides
    print("prism(64) probe", probe[0][2])
    v, t = m.icosphere(2)
    r = _detect((v.astype(np.float32), t), axes=0, max_order=2, samples=256)
    assert r.symmetric and len(r.passed) == 6 and 1e-3 < max(p[2] for p in r.passed) < 0.01
    print("icosphere(2)", max(p[2] for p in r.passed))


def test_asymmetric_bodies_are_refused_with_room():
    r = _detect(m.bracket())
    assert not r.symmetric and r.passed == [] and 0.035 < float(r.residuals.min()) < 0.045, float(r.residuals.min())   # the 0.15 step over D = 3.78
    print("bracket", float(r.residuals.min()))
    assert "symmetric: no" in str(r)
    r = _detect(m.scalene_tetrahedron())
    assert not r.symmetric and 0.12 < float(r.residuals.min()) < 0.15, float(r.residuals.min())
    print("scalene tetrahedron", float(r.residuals.min()))


def test_colour_breaks_a_symmetry_only_when_it_is_not_symmetric_itself():
    v, t = m.box(1, 2, 3)
    grey = np.full((len(v), 3), 130, dtype=np.uint8)
    face = grey.copy()
    face[20:24] = (255, 0, 0)                                        # the +z face: its four own vertices
    r = _detect((v, t), face)
    assert r.symmetric and _orders(r, (0, 0, 1)) == [2] and _orders(r, (1, 0, 0)) == [] and _orders(r, (0, 1, 0)) == []
    # one of that face's two triangles: the face's vertices are split so that only triangle 10 is red
    assert tuple(t[10]) == (20, 21, 22) and tuple(t[11]) == (20, 22, 23)
    v2 = np.concatenate([v, v[[20, 22]]])                            # vertices 24, 25: grey copies of the diagonal's ends
    t2 = t.copy()
    t2[11] = (24, 25, 23)
    half = np.full((len(v2), 3), 130, dtype=np.uint8)
    half[[20, 21, 22]] = (255, 0, 0)
    assert not _detect((v2, t2), half).symmetric
    assert _detect((v2, t2)).symmetric


def test_the_global_numpy_stream_is_left_alone():
    np.random.seed(123)
    before = np.random.get_state()
    _detect(m.box(1, 2, 3), seed=5)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    a, b = _detect(m.bracket(), seed=5, samples=64), _detect(m.bracket(), seed=5, samples=64)
    assert m.same_bits(a.residuals, b.residuals)


def test_arguments():
    with pytest.raises(ValueError):
        detect_symmetry(np.zeros((3, 3)), np.array([[0, 0, 1]]), closest=m.closest_np)      # no valid triangle
    with pytest.raises(ValueError):
        detect_symmetry(np.zeros((3, 3)), np.array([[0, 1, 2]]), closest=m.closest_np)      # no surface
    with pytest.raises(ValueError):
        _detect(m.box(1, 2, 3), max_order=1)
    assert parse_sym_option(["none"]) == "none" and parse_sym_option("auto") == "auto" and parse_sym_option(["2", "0", "2"]) == [0, 2]
    with pytest.raises(ValueError):
        parse_sym_option(["auto", "1"])
