"""What the tests of the bounding-box tree route share (``df_mesh_tree_build``, ``df_mesh_closest_tree``, ``df_mesh_icp_tree``:
include/dfusion.h): the tree of a mesh through the library's host entry, the host walk, and the adversarial meshes and queries.  The tree
adds no numerics, so every expected output is ``mesh_closest_np.closest_np`` / ``mesh_icp_np.run_case``, used by import."""
import math

import numpy as np

import mesh_closest_np as m


def tree_of(vertices, triangles, tri_begin=None, leaf=None):
    """``lib.mesh_set.MeshTree`` of the mesh (host only: the library loads without a GPU)."""
    from densefusion_amd.lib.mesh_set import MeshTree
    return MeshTree(vertices, triangles, tri_begin, leaf)


def host_walk(vertices, triangles, points, xf, tree=None):
    """``df_mesh_closest_tree_host``: (dist2 [K,P], tri [K,P], closest [K,P,3], tested [K,P,2] int64 = triangles and boxes tested)."""
    from densefusion_amd import _lib
    L = _lib.lib()
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    X = np.ascontiguousarray(xf, dtype=np.float64).reshape(-1, 12)
    tree = tree_of(v, t) if tree is None else tree
    K, P = len(X), len(p)
    d2, tri, c, tested = np.full((K, P), 7.0), np.full((K, P), 7, dtype=np.int32), np.full((K, P, 3), 7.0), np.full((K, P, 2), 7, dtype=np.int64)
    rc = L.df_mesh_closest_tree_host(v.ctypes.data, len(v), t.ctypes.data, len(t), p.ctypes.data, P, X.ctypes.data, K, tree.nodes.ctypes.data,
                                     tree.n_nodes, tree.node_begin.ctypes.data, tree.order.ctypes.data, tree.n_order, tree.loose.ctypes.data,
                                     tree.n_loose, tree.loose_begin.ctypes.data, d2.ctypes.data, tri.ctypes.data, c.ctypes.data, tested.ctypes.data)
    assert rc == 0, L.df_last_error()
    return d2, tri, c, tested


# ---- the tree's own invariants ---------------------------------------------------------------------------------------------------------------
def check_tree(tree, vertices, triangles):
    """Asserts B1, B2 of the header on a built tree; returns (triangles in leaves, loose triangles, deepest path in inner nodes)."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    kept = m.kept_triangles(t, len(v))
    box = tree.nodes[:, :6].view(np.float32)
    seen, deepest = [], 0
    assert tree.node_begin[0] == 0 and tree.loose_begin[0] == 0 and tree.node_begin[-1] == tree.n_nodes and tree.loose_begin[-1] == tree.n_loose
    for o in range(tree.n_objects):
        lo, hi = int(tree.tri_begin[o]), int(tree.tri_begin[o + 1])
        loose = tree.loose[tree.loose_begin[o]:tree.loose_begin[o + 1]].tolist()
        assert all(lo <= x < hi for x in loose)
        seen += loose
        n0, n1 = int(tree.node_begin[o]), int(tree.node_begin[o + 1])
        if n1 == n0:
            continue

        def visit(i, depth):
            """-> the triangles below node i"""
            nonlocal deepest
            assert n0 <= i < n1
            a, b = int(tree.nodes[i, 6]), int(tree.nodes[i, 7])
            if b > 0:
                assert 0 <= a and a + b <= tree.n_order and b <= tree.leaf
                mine = tree.order[a:a + b].tolist()
                assert mine == sorted(mine) and all(lo <= x < hi for x in mine)
                deepest = max(deepest, depth)
            else:
                assert b == 0 and i + 1 < a < n1
                mine = visit(i + 1, depth + 1) + visit(a, depth + 1)
            pts = v[t[mine].reshape(-1)]
            assert (pts >= box[i, :3]).all() and (pts <= box[i, 3:]).all(), "a node's box holds its triangles' vertices"
            return mine

        seen += visit(n0, 0)
    assert sorted(seen) == np.nonzero(kept)[0].tolist(), "every kept triangle once, in a leaf or on the loose list; no dropped one"
    assert deepest <= 32
    return len(seen) - tree.n_loose, tree.n_loose, deepest


def loose_np(vertices, triangles):
    """the indices B1 of the header puts on the loose list, from the restatement's records"""
    rec = m.prepare_np(vertices, triangles)
    with np.errstate(all="ignore"):
        ee = (rec["e"] * rec["e"]).sum(axis=2)                                               # the rule's margin is far above this sum's rounding
        thin = (rec["nn"][:, None] < 2.0 ** -16 * ee * ee[:, [1, 2, 0]]).any(axis=1) & (rec["nn"] > 0)
        wild = ~np.isfinite(rec["U"]).all(axis=(1, 2)) & m.kept_triangles(triangles, len(vertices))
    return np.nonzero(thin | wild)[0].tolist()


def same_bytes(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("nodes", "order", "loose", "node_begin", "loose_begin")) and \
        (a.n_nodes, a.n_order, a.n_loose) == (b.n_nodes, b.n_order, b.n_loose)


def chain_mesh(T, seed=3):
    """T small triangles scattered in the unit cube"""
    rng = np.random.default_rng(seed)
    v = (rng.uniform(0, 1, (T, 1, 3)) + rng.uniform(-.05, .05, (T, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * T, dtype=np.int32).reshape(T, 3)


# ---- adversarial meshes and queries ----------------------------------------------------------------------------------------------------------
def shuffled_grid(n=8, seed=5):
    """A flat n x n grid of unit squares on integer coordinates, two triangles each, in shuffled order; the queries are its vertices and
    the midpoints of its edges and diagonals: d = 0 is exact on up to six triangles and the lowest index must win."""
    idx = lambda i, j: i * (n + 1) + j                                                        # noqa: E731
    v = np.array([[i, j, 0] for i in range(n + 1) for j in range(n + 1)], dtype=np.float32)
    t = []
    for i in range(n):
        for j in range(n):
            t += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    t = np.array(t, dtype=np.int32)[np.random.default_rng(seed).permutation(2 * n * n)]
    vd = v.astype(np.float64)
    mid = np.concatenate([(vd[t[:, a]] + vd[t[:, b]]) / 2 for a, b in ((0, 1), (1, 2), (2, 0))])
    return v, t, np.concatenate([vd, np.unique(mid, axis=0)])


def sliver(angle, at=(0.0, 0.0, 0.0)):
    """three vertices of a triangle with the angle ``angle`` at A, unit legs"""
    a = np.asarray(at, dtype=np.float64)
    return [a, a + [1.0, 0.0, 0.0], a + [math.cos(angle), math.sin(angle), 0.0]]


def sliver_mesh():
    """Slivers with an angle at A of 1e-3, 1e-6 and 1e-9 rad, one with a good angle at A and a thin one at B, and a collinear triangle,
    beside the bracket's well-shaped ones."""
    bv, bt = m.bracket()
    corners = sliver(1e-3, (2, 0, 0)) + sliver(1e-6, (2, 1, 0)) + sliver(1e-9, (2, 2, 0))
    corners += [np.array(p, dtype=np.float64) for p in ((2, 3, 0), (3, 3, 0), (2.0005, 3.001, 0))]     # a good angle at A, 1e-3 at B
    corners += [np.array(p, dtype=np.float64) for p in ((2, 4, 0), (2.5, 4, 0), (3, 4, 0))]            # collinear
    v = np.array(corners, dtype=np.float32)
    return m.merge((bv, bt), (v, np.arange(len(v), dtype=np.int32).reshape(-1, 3)))


def adversarial_cases():
    """name -> (vertices, triangles, points, xf), like ``mesh_closest_np.make_cases``."""
    rng = np.random.default_rng(21)
    one = m.IDENTITY[None]
    cases = {}
    v, t, q = shuffled_grid()
    cases["shuffled_grid"] = (v, t, q, one)
    bv, bt = m.bracket()
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    cases["one_triangle_three_times"] = (tri, np.array([[0, 1, 2]] * 3, dtype=np.int32), np.concatenate([tri.astype(np.float64), rng.uniform(-1, 2, (20, 3))]), one)
    sv, st = sliver_mesh()
    near = np.array([[2.5, 0.0002, 0.0], [2.5, 0.0002, 1e-5], [2.9, 1.0, 1e-7], [2.5, 2.0, 1e-8], [2.5, 2.0, 0.0], [2.995, 3.0002, 1e-6],
                     [2.7, 4.0, 0.0], [2.7, 4.0, .01], [2.2, 1.5, .3]])
    cases["slivers"] = (sv, st, np.concatenate([near, rng.uniform(-1, 4, (60, 3)) * np.array([1.0, 1.0, .2])]), m.three_xf())
    D = math.sqrt(1 + 4 + 9)                                                                  # the bracket's box(1, 2, 3)
    far = rng.normal(size=(16, 3))
    far = far / np.sqrt((far * far).sum(axis=1, keepdims=True)) * 100 * D
    cases["far_queries"] = (bv, bt, np.concatenate([far, np.array([[100 * D, 0, 0], [0, -100 * D, 0]])]), m.three_xf())
    shift = np.array([1e6, -1e6, 1e6])
    cases["near_1e6"] = ((bv.astype(np.float64) + shift).astype(np.float32), bt, rng.uniform(-2, 2, (40, 3)) + shift, one)
    pts = rng.uniform(-1, 1, (9, 3))
    pts[2, 1], pts[5, :], pts[7, 0] = np.nan, np.nan, np.inf
    cases["nan_query"] = (bv, bt, pts, m.three_xf())
    dv, dt = m.degenerate_mesh()
    cases["all_dropped"] = (dv, dt[:3], rng.uniform(-1, 1, (5, 3)), m.three_xf())
    return cases
