"""``MeshSet`` -- several CAD meshes packed the way ``df_cad_render_scene``, ``df_mesh_icp`` and ``df_pose_verify`` read them: one vertex
array, one triangle array with global indices and the ``tri_begin`` table.  Packed and checked once on the host, uploaded once per
device: the scene renderer, ``MeshIcp`` and ``PoseVerifier`` of one dataset read the same device arrays.  ``MeshTree`` is the bounding-box
tree of such a packing (``df_mesh_tree_build``, include/dfusion.h) through which ``df_mesh_closest_tree`` and ``df_mesh_icp_tree`` find
the closest triangle; ``MeshSet.tree`` builds it once per set of scaled vertices."""
import ctypes
import hashlib
import time

import numpy as np
import torch

from .. import _lib


def check_triangles(triangles, n_vertices):
    """triangles as int32 [T,3] with T >= 1; ``ValueError`` on any other shape or on an index outside 0..n_vertices-1 (host only)."""
    tri = np.asarray(triangles)
    if tri.ndim != 2 or tri.shape[1] != 3 or tri.shape[0] == 0 or not np.issubdtype(tri.dtype, np.integer):
        raise ValueError("triangles must be a non-empty integer array [T,3]")
    lo, hi = int(tri.min()), int(tri.max())
    if lo < 0 or hi >= n_vertices:
        bad = np.argwhere((tri < 0) | (tri >= n_vertices))[0]
        raise ValueError(f"triangle {bad[0]} names vertex {int(tri[bad[0], bad[1]])}, outside 0..{n_vertices - 1}")
    return np.ascontiguousarray(tri, dtype=np.int32)


class MeshTree:
    """The box tree of ``triangles`` [T,3] int32 over ``vertices`` [V,3] fp32 (the scaled ones the distance calls read) for the object
    ranges ``tri_begin`` [O+1] (None: one object, all triangles), leaves of at most ``leaf`` triangles (None: the library's).  Built on
    the host (``RuntimeError`` where the library refuses); ``build_seconds`` is the host time it took.  Host arrays: ``nodes`` int32
    [n,8] (32-byte nodes: a float32 box in the first six words), ``order``, ``loose`` int32, ``node_begin``, ``loose_begin`` int32 [O+1]."""

    def __init__(self, vertices, triangles, tri_begin=None, leaf=None):
        L = _lib.lib()
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        begin = np.array([0, len(t)], dtype=np.int32) if tri_begin is None else np.ascontiguousarray(tri_begin, dtype=np.int32).reshape(-1)
        O = len(begin) - 1
        sizes = [ctypes.c_size_t(0) for _ in range(3)]
        _lib.check(L.df_mesh_tree_sizes(len(t), O, *[ctypes.addressof(x) for x in sizes]), "mesh_tree_sizes")
        nodes = np.zeros((sizes[0].value, 8), dtype=np.int32)          # numpy's allocations are 16-byte aligned; the build checks it
        order, loose = np.zeros(sizes[1].value, dtype=np.int32), np.zeros(sizes[2].value, dtype=np.int32)
        self.node_begin, self.loose_begin = np.zeros(O + 1, dtype=np.int32), np.zeros(O + 1, dtype=np.int32)
        used = (ctypes.c_size_t * 3)()
        self.leaf = int(L.df_mesh_tree_leaf_triangles()) if leaf is None else int(leaf)
        t0 = time.perf_counter()
        _lib.check(L.df_mesh_tree_build(v.ctypes.data, len(v), t.ctypes.data, len(t), begin.ctypes.data, O, self.leaf, nodes.ctypes.data,
                                        self.node_begin.ctypes.data, order.ctypes.data, loose.ctypes.data, self.loose_begin.ctypes.data,
                                        ctypes.addressof(used)), "mesh_tree_build")
        self.build_seconds = time.perf_counter() - t0
        # at least one element each: an empty array has no pointer to give, and the calls refuse a null one
        self.nodes, self.order, self.loose = (a[:max(1, n)].copy() for a, n in zip((nodes, order, loose), used))
        self.n_nodes, self.n_order, self.n_loose, self.tri_begin, self.n_objects, self._on = int(used[0]), int(used[1]), int(used[2]), begin, O, {}

    def on(self, device):
        """(nodes, order, loose) as tensors on ``device``: uploaded on first use, then the same objects."""
        device = torch.empty(0, device=device).device
        if device not in self._on:
            self._on[device] = tuple(torch.from_numpy(a).to(device) for a in (self.nodes, self.order, self.loose))
        return self._on[device]

    def args(self, device):
        """the eight trailing arguments of ``df_mesh_closest_tree`` / ``df_mesh_icp_tree`` for the copies on ``device``"""
        nodes, order, loose = self.on(device)
        return (_lib.dptr(nodes), self.n_nodes, self.node_begin.ctypes.data, _lib.dptr(order), self.n_order, _lib.dptr(loose), self.n_loose,
                self.loose_begin.ctypes.data)


class MeshSet:
    """``meshes``: a list of (vertices [V,3], triangles [T,3][, colours [V,3], ...]), object o being meshes[o]; entries of a tuple beyond
    those asked for are ignored.  Everything is checked on the host (``ValueError``) and nothing touches a device here.  Host arrays:
    ``vertices`` float32 [V,3] in file units, ``triangles`` int32 [T,3] with global indices, ``tri_begin`` and ``vertex_begin`` int32
    [O+1] (object o owns triangles tri_begin[o] .. tri_begin[o+1]-1), ``colors`` uint8 [V,3] or None; ``n_objects``."""

    def __init__(self, meshes, colors=False):
        self._parent, self._on, self._trees = None, {}, {}          # the set this one is a prefix of; device -> tensors; trees built
        verts, tris, cols, begin, vertex_begin = [], [], [], [0], [0]
        for mesh in meshes:
            v = np.ascontiguousarray(mesh[0], dtype=np.float32).reshape(-1, 3)
            tris.append(check_triangles(mesh[1], len(v)) + np.int32(vertex_begin[-1]))
            if colors:
                cols.append(np.ascontiguousarray(mesh[2], dtype=np.uint8).reshape(-1, 3))
                if len(cols[-1]) != len(v):
                    raise ValueError("one colour per vertex")
            verts.append(v)
            begin.append(begin[-1] + len(tris[-1]))
            vertex_begin.append(vertex_begin[-1] + len(v))
        if not verts or 3 * max(vertex_begin[-1], begin[-1]) > 2 ** 31 - 1:
            raise ValueError("a mesh set needs at least one mesh, and 3 V and 3 T must fit an int")
        self.vertices, self.triangles, self.colors = np.concatenate(verts), np.concatenate(tris), np.concatenate(cols) if colors else None
        self.tri_begin, self.vertex_begin, self.n_objects = np.array(begin, dtype=np.int32), np.array(vertex_begin, dtype=np.int32), len(verts)

    def first(self, n):
        """The set of objects 0..n-1: prefix views of this set's arrays (exactly what packing the first n meshes alone gives) whose
        ``on(device)`` slices this set's device tensors, so nothing is uploaded again."""
        if not 1 <= n <= self.n_objects:
            raise ValueError(f"first: 1..{self.n_objects} objects, got {n}")
        nv, nt, sub = int(self.vertex_begin[n]), int(self.tri_begin[n]), object.__new__(MeshSet)
        sub.vertices, sub.triangles, sub.colors = self.vertices[:nv], self.triangles[:nt], None if self.colors is None else self.colors[:nv]
        sub.tri_begin, sub.vertex_begin, sub.n_objects, sub._parent, sub._on = self.tri_begin[:n + 1], self.vertex_begin[:n + 1], int(n), self, {}
        sub._trees = {}
        return sub

    def on(self, device):
        """(vertices, triangles, colors or None) as tensors on ``device`` ("cpu" included): uploaded on first use, then the same objects."""
        device = torch.empty(0, device=device).device               # with its index: "cuda" is whichever device is current
        if device not in self._on:
            host = (self.vertices, self.triangles, self.colors)     # a prefix set slices its parent's tensors (a whole set: all of its own)
            up = self._parent.on(device) if self._parent is not None else [None if a is None else torch.from_numpy(a).to(device) for a in host]
            self._on[device] = tuple(None if a is None else t[:len(a)] for a, t in zip(host, up))
        return self._on[device]

    def scaled(self, scales):
        """float32 [V,3]: the vertices of mesh o times ``scales[o]`` (or the one scale for all) in fp64, rounded to fp32; finite scales > 0."""
        s = np.asarray(scales, dtype=np.float64).reshape(-1)
        if s.size not in (1, self.n_objects) or not (np.isfinite(s).all() and (s > 0).all()):
            raise ValueError("one positive finite scale per mesh, or one for all")
        per_vertex = np.repeat(np.broadcast_to(s, (self.n_objects,)), np.diff(self.vertex_begin))
        return (self.vertices.astype(np.float64) * per_vertex[:, None]).astype(np.float32)

    def tree(self, scaled_vertices):
        """The ``MeshTree`` of this set's triangles over ``scaled_vertices`` (float32 [V,3]: ``scaled(...)``): built on first use for
        these vertices, then the same object, whose ``on(device)`` uploads once per device."""
        v = np.ascontiguousarray(scaled_vertices, dtype=np.float32).reshape(-1, 3)
        if len(v) != len(self.vertices):
            raise ValueError(f"tree: {len(self.vertices)} vertices, got {len(v)}")
        key = hashlib.sha1(v.tobytes()).digest()
        if key not in self._trees:
            self._trees[key] = MeshTree(v, self.triangles, self.tri_begin)
        return self._trees[key]
