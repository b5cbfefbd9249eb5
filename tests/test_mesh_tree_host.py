"""CPU: the bounding-box tree of a mesh (``df_mesh_tree_build``) and the walk through it (``df_mesh_closest_tree_host``, the same
``mesh_tree_core.h`` the kernels run) against the restatement of the plain scan, ``mesh_closest_np.closest_np``, bit for bit.  The
library's host entries need no GPU.

The trees are the smallest at which the build can go wrong: 1 triangle and on each side of one and two leaves (L - 1, L, L + 1, 2 L + 1),
a mesh with dropped and edge-only triangles, a set of two objects with one empty range; the queries are every case the scan's own tests
walk and the adversarial ones of ``mesh_tree_np``: exact ties on up to six triangles in shuffled order, a triangle listed three times,
slivers (loose and not), a collinear triangle, queries 100 diameters away and at coordinates near 1e6, NaN and infinite queries, an
object with no triangle kept."""
import numpy as np
import pytest

import mesh_closest_np as m
import mesh_icp_np as icp
import mesh_tree_np as mt


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from densefusion_amd import _lib
    return _lib.lib()


def _same(got, want, name):
    for g, w, what in zip(got, want, ("dist2", "tri", "closest")):
        assert m.same_bits(g, w), f"{name}: {what} differs"


def test_tree_invariants(L):
    leaf = L.df_mesh_tree_leaf_triangles()
    assert 1 <= leaf <= 64
    meshes = {"bracket": m.bracket(), "icosphere3": m.icosphere(3), "degenerate": m.degenerate_mesh(), "slivers": mt.sliver_mesh()}
    for T in sorted({1, max(1, leaf - 1), leaf, leaf + 1, 2 * leaf + 1}):
        meshes["T%d" % T] = mt.chain_mesh(T)
    for name, (v, t) in meshes.items():
        for lf in (None, 1, 3):
            tree = mt.tree_of(v, t, leaf=lf)
            in_leaves, loose, depth = mt.check_tree(tree, v, t)
            assert mt.same_bytes(tree, mt.tree_of(v, t, leaf=lf)), f"{name}: two builds, equal bytes"
            if name == "degenerate":
                assert (in_leaves, loose) == (3, 0), "three dropped; the collinear and the doubled-vertex triangle keep their edges"
            if name == "slivers":
                assert tree.loose.tolist()[:loose] == mt.loose_np(v, t) == [24, 25, 27], "1e-3 and 1e-6 at A, 1e-3 at B; 1e-9 collapses in fp32"
    v, t, begin = icp.concat_meshes([m.bracket(), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), m.scalene_tetrahedron()])
    tree = mt.tree_of(v, t, begin)
    mt.check_tree(tree, v, t)
    assert tree.node_begin[1] == tree.node_begin[2] and tree.node_begin[3] > tree.node_begin[2] and tree.n_order == 28
    dv, dt = m.degenerate_mesh()
    none = mt.tree_of(dv, dt[:3])
    assert (none.n_nodes, none.n_order, none.n_loose) == (0, 0, 0)


def test_no_loose_triangles_on_ordinary_meshes(L):
    for mesh in (m.bracket(), m.icosphere(3), m.icosphere(5), m.box(1, 1, 1), m.prism(6, 1.0, 2.0), m.scalene_tetrahedron()):
        assert mt.tree_of(*mesh).n_loose == 0


def test_build_and_size_refusals(L):
    v, t = m.bracket()
    v, t = np.ascontiguousarray(v), np.ascontiguousarray(t)
    begin = np.array([0, len(t)], dtype=np.int32)
    nodes, order, loose = np.full((2 * len(t) + 1, 8), 7, dtype=np.int32), np.full(len(t), 7, dtype=np.int32), np.full(len(t), 7, dtype=np.int32)
    nb, lb, used = np.full(2, 7, dtype=np.int32), np.full(2, 7, dtype=np.int32), np.full(3, 7, dtype=np.uint64)
    good = dict(v=v.ctypes.data, V=len(v), t=t.ctypes.data, T=len(t), begin=begin.ctypes.data, O=1, leaf=4, nodes=nodes.ctypes.data, nb=nb.ctypes.data,
                order=order.ctypes.data, loose=loose.ctypes.data, lb=lb.ctypes.data, used=used.ctypes.data)
    bad_begin = [np.array(a, dtype=np.int32) for a in ([0, len(t) + 1], [-1, len(t)], [5, 4])]
    errors = [dict(v=None), dict(t=None), dict(begin=None), dict(nodes=None), dict(nb=None), dict(order=None), dict(loose=None), dict(lb=None),
              dict(used=None), dict(V=0), dict(T=0), dict(T=(2 ** 31 - 1) // 3 + 1), dict(O=0), dict(O=65), dict(leaf=0), dict(leaf=65),
              dict(nodes=nodes.ctypes.data + 4)] + [dict(begin=a.ctypes.data) for a in bad_begin]
    for kw in errors:
        a = dict(good, **kw)
        assert L.df_mesh_tree_build(*[a[k] for k in good]) == -1, kw
        assert len(L.df_last_error()) > 10
    assert (nodes == 7).all() and (order == 7).all() and (nb == 7).all() and (used == 7).all(), "nothing was written"
    assert L.df_mesh_tree_build(*good.values()) == 0 and used[1] == len(t) and nb[1] == used[0]
    sizes = np.zeros(3, dtype=np.uint64)
    ptr = [sizes[i:].ctypes.data for i in range(3)]
    assert L.df_mesh_tree_sizes(24, 1, *ptr) == 0 and sizes.tolist() == [48, 24, 24]
    for T, O in ((0, 1), (24, 0), (24, 65), ((2 ** 31 - 1) // 3 + 1, 1)):
        assert L.df_mesh_tree_sizes(T, O, *ptr) == -1
    assert L.df_mesh_tree_sizes(24, 1, None, ptr[1], ptr[2]) == -1


def test_host_walk_refusals(L):
    v, t = m.bracket()
    tree = mt.tree_of(v, t)
    v, t = np.ascontiguousarray(v), np.ascontiguousarray(t)
    p, X = np.zeros((2, 3)), np.ascontiguousarray(m.IDENTITY.reshape(1, 12))
    d2, tri = np.zeros(2), np.zeros(2, dtype=np.int32)
    good = dict(v=v.ctypes.data, V=len(v), t=t.ctypes.data, T=len(t), p=p.ctypes.data, P=2, X=X.ctypes.data, K=1, nodes=tree.nodes.ctypes.data,
                n_nodes=tree.n_nodes, nb=tree.node_begin.ctypes.data, order=tree.order.ctypes.data, n_order=tree.n_order, loose=tree.loose.ctypes.data,
                n_loose=tree.n_loose, lb=tree.loose_begin.ctypes.data, d2=d2.ctypes.data, tri=tri.ctypes.data, c=None, tested=None)
    assert L.df_mesh_closest_tree_host(*good.values()) == 0
    other = mt.tree_of(*m.icosphere(2))                                # 320 triangles: more nodes than 24 triangles can have
    bad_nb = [np.array(a, dtype=np.int32) for a in ([1, tree.n_nodes], [0, -1], [0, 2 * len(t)])]
    errors = [dict(nodes=None), dict(nb=None), dict(order=None), dict(loose=None), dict(lb=None), dict(d2=None), dict(tri=None), dict(P=0), dict(K=0),
              dict(nodes=tree.nodes.ctypes.data + 4), dict(order=tree.order.ctypes.data + 2), dict(n_nodes=tree.n_nodes - 1), dict(n_order=0),
              dict(n_order=len(t) + 1), dict(nb=other.node_begin.ctypes.data, n_nodes=other.n_nodes)] + [dict(nb=a.ctypes.data) for a in bad_nb]
    for kw in errors:
        a = dict(good, **kw)
        assert L.df_mesh_closest_tree_host(*[a[k] for k in good]) == -1, kw


def test_host_walk_equals_the_scan_bit_for_bit(L):
    tile = L.df_mesh_closest_tile_triangles()
    cases = dict(m.make_cases(tile), whole_path=m.whole_path_case(tile), **mt.adversarial_cases())
    for name, (v, t, p, xf) in cases.items():
        want = m.closest_np(v, t, p, xf)
        for leaf in (None, 1):
            got = mt.host_walk(v, t, p, xf, mt.tree_of(v, t, leaf=leaf))
            _same(got[:3], want, name)
    # the cases are what they claim
    v, t, q, xf = cases["shuffled_grid"]
    d2, tri, _ = m.closest_np(v, t, q, xf)
    owners = [(int((np.abs(v[t].astype(np.float64) - p).sum(axis=2) == 0).any(axis=1).sum())) for p in q[:81]]
    assert (d2 == 0).all() and max(owners) == 6, "a grid vertex lies on up to six triangles"
    assert all(int(tri[0, i]) == min(np.nonzero((np.abs(v[t].astype(np.float64) - q[i]).sum(axis=2) == 0).any(axis=1))[0]) for i in range(81))
    d2, tri, _ = m.closest_np(*cases["one_triangle_three_times"])
    assert (tri == 0).all()
    d2, tri, _ = m.closest_np(*cases["slivers"])
    assert {24, 25, 26, 27, 28} <= set(np.unique(tri).tolist()), "every sliver and the collinear triangle win somewhere"
    d2, tri, c = m.closest_np(*cases["nan_query"])
    assert (tri[:, [2, 5, 7]] == -1).all() and np.isposinf(d2[:, [2, 5, 7]]).all() and (tri[:, [0, 1, 3, 4, 6, 8]] >= 0).all()
    d2, tri, _ = m.closest_np(*cases["far_queries"])
    assert (tri >= 0).all() and d2.min() > 1e4
    d2, tri, _ = m.closest_np(*cases["all_dropped"])
    assert (tri == -1).all()


def test_the_tree_prunes(L):
    """A condition that keeps out a walk that tests everything, not a measurement: the mean number of triangles tested per query is
    below T / 8.  (Measured: DESIGN 12l.)"""
    v, t = m.icosphere(5)
    rng = np.random.default_rng(3)
    d = rng.normal(size=(256, 3))
    q = d / np.sqrt((d * d).sum(axis=1, keepdims=True)) * rng.uniform(0.95, 1.05, (256, 1))
    d2, tri, c, tested = mt.host_walk(v, t, q, m.IDENTITY[None])
    _same((d2, tri, c), m.closest_np(v, t, q, m.IDENTITY[None]), "icosphere(5)")
    print("icosphere(5): triangles tested per query: mean %.1f, max %d; boxes: mean %.1f, max %d (T = %d)"
          % (tested[..., 0].mean(), tested[..., 0].max(), tested[..., 1].mean(), tested[..., 1].max(), len(t)))
    assert len(t) == 20480 and tested[..., 0].mean() < len(t) / 8
    assert (tested[..., 0] >= 1).all()
