"""The exact closest point of a triangle mesh on the device (``df_mesh_closest``, include/dfusion.h): for P points under K transforms,
the squared distance to the mesh, the triangle that gives it and the closest point on it, all in fp64 by the written-out rule
M1..D5 (tests/mesh_closest_np.py restates it; the outputs are compared bit for bit).  ``mesh_closest`` enqueues on the current stream
and without a host sync; ``datasets/customCAD/symmetry.py`` is its user.
"""
from __future__ import annotations

import torch

from .. import _lib

INT_MAX = 2 ** 31 - 1


def check_counts(V, T, P, K):
    """``ValueError`` unless V, T, P, K >= 1 and 3 V, 3 T, 12 K and 3 K P fit an int (the limits of ``df_mesh_closest``)."""
    V, T, P, K = int(V), int(T), int(P), int(K)
    if min(V, T, P, K) < 1 or 3 * V > INT_MAX or 3 * T > INT_MAX or 12 * K > INT_MAX or 3 * K * P > INT_MAX:
        raise ValueError(f"mesh_closest: need V, T, P, K >= 1 and 3 V, 3 T, 12 K, 3 K P within an int (V {V}, T {T}, P {P}, K {K})")
    return V, T, P, K


def scratch_bytes(T):
    return int(_lib.lib().df_mesh_closest_scratch_bytes(int(T)))


def tile_triangles():
    return int(_lib.lib().df_mesh_closest_tile_triangles())


def mesh_closest(vertices, triangles, points, xf, want_closest=True, scratch=None, accel=False, tree=None):
    """vertices [V,3] fp32, triangles [T,3] int32, points [P,3] fp64, xf [K,3,4] (or [K,12]) fp64: device tensors on one device.
    Returns (dist2 [K,P] fp64, tri [K,P] int32, closest [K,P,3] fp64 or None) on the device.  ``scratch``: an optional contiguous uint8
    device tensor of at least ``scratch_bytes(T)`` bytes (one is allocated otherwise).  A triangle with a bad or repeated index is
    skipped; a query with no triangle left gets tri -1, dist2 +inf and closest = the transformed point.
    ``accel``: the same outputs byte for byte through a bounding-box tree (``df_mesh_closest_tree``).  ``tree``: the
    ``lib.mesh_set.MeshTree`` of these vertices and triangles as one object; without one it is built here from a download of the mesh,
    a host round trip per call, so a caller with many calls on one mesh builds it once."""
    vertices = _lib.need_tensor(vertices, "mesh_closest", "vertices", (torch.float32,), (None, 3), None)
    dev = vertices.device                                           # the others must be on the same one
    triangles = _lib.need_tensor(triangles, "mesh_closest", "triangles", (torch.int32,), (None, 3), dev)
    points = _lib.need_tensor(points, "mesh_closest", "points", (torch.float64,), (None, 3), dev)
    xf = _lib.need_tensor(xf, "mesh_closest", "xf", (torch.float64,), ((None, 3, 4), (None, 12)), dev)
    V, T, P, K = check_counts(vertices.shape[0], triangles.shape[0], points.shape[0], xf.shape[0])
    nbytes = scratch_bytes(T)
    if scratch is None:
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    elif (not torch.is_tensor(scratch) or scratch.device != dev or scratch.dtype != torch.uint8 or not scratch.is_contiguous()
          or scratch.numel() < nbytes or scratch.data_ptr() % 16):
        raise RuntimeError(f"mesh_closest: scratch must be a contiguous, 16-byte aligned uint8 tensor of >= {nbytes} bytes on the mesh's device")
    dist2 = torch.empty(K, P, dtype=torch.float64, device=dev)
    tri = torch.empty(K, P, dtype=torch.int32, device=dev)
    closest = torch.empty(K, P, 3, dtype=torch.float64, device=dev) if want_closest else None
    call, name, extra = _lib.lib().df_mesh_closest, "mesh_closest", ()
    if accel:
        if tree is None:
            from .mesh_set import MeshTree
            tree = MeshTree(vertices.cpu().numpy(), triangles.cpu().numpy())
        if tree.n_objects != 1 or int(tree.tri_begin[1]) != T:
            raise ValueError(f"mesh_closest: the tree is of {tree.n_objects} objects and {int(tree.tri_begin[-1])} triangles, the mesh one of {T}")
        call, name, extra = _lib.lib().df_mesh_closest_tree, "mesh_closest_tree", tree.args(dev)
    with _lib.device_guard(dev):
        _lib.check(call(_lib.dptr(vertices), V, _lib.dptr(triangles), T, _lib.dptr(points), P, _lib.dptr(xf), K, _lib.dptr(dist2), _lib.dptr(tri),
                        _lib.dptr(closest) if want_closest else None, _lib.dptr(scratch), scratch.numel(), _lib.current_stream(), *extra), name)
    return dist2, tri, closest
