"""``MeshSet`` -- several CAD meshes packed the way ``df_cad_render_scene``, ``df_mesh_icp`` and ``df_pose_verify`` read them: one vertex
array, one triangle array with global indices and the ``tri_begin`` table.  Packed and checked once on the host, uploaded once per
device: the scene renderer, ``MeshIcp`` and ``PoseVerifier`` of one dataset read the same device arrays."""
import numpy as np
import torch


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


class MeshSet:
    """``meshes``: a list of (vertices [V,3], triangles [T,3][, colours [V,3], ...]), object o being meshes[o]; entries of a tuple beyond
    those asked for are ignored.  Everything is checked on the host (``ValueError``) and nothing touches a device here.  Host arrays:
    ``vertices`` float32 [V,3] in file units, ``triangles`` int32 [T,3] with global indices, ``tri_begin`` and ``vertex_begin`` int32
    [O+1] (object o owns triangles tri_begin[o] .. tri_begin[o+1]-1), ``colors`` uint8 [V,3] or None; ``n_objects``."""

    def __init__(self, meshes, colors=False):
        self._parent, self._on = None, {}                           # the set this one is a prefix of; device -> tensors
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
