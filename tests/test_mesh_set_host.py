"""Host: ``lib.mesh_set.MeshSet`` -- packing, the prefix set, scaling, the host checks and the per-device cache.  No GPU."""
import numpy as np
import pytest
import torch

import mesh_closest_np as m
from densefusion_amd.lib.mesh_set import MeshSet


def _meshes():
    rng = np.random.default_rng(3)
    out = []
    for v, t in (m.bracket(), m.scalene_tetrahedron()):
        out.append((v, t, rng.integers(0, 256, (len(v), 3), dtype=np.uint8)))
    return out


def test_packing_prefix_and_scaling():
    (bv, bt, bc), (tv, tt, tc) = bracket, tetra = _meshes()
    Vb = len(bv)
    assert len(bt) == 24 and len(tt) == 4 and len(tv) == 4
    ms = MeshSet([bracket, tetra], colors=True)
    assert ms.n_objects == 2
    assert ms.tri_begin.tolist() == [0, 24, 28] and ms.vertex_begin.tolist() == [0, Vb, Vb + 4]
    assert np.array_equal(ms.vertices, np.concatenate([bv, tv])) and np.array_equal(ms.triangles, np.concatenate([bt, tt + Vb]))
    assert np.array_equal(ms.colors, np.concatenate([bc, tc]))
    assert (ms.vertices.dtype, ms.triangles.dtype, ms.tri_begin.dtype, ms.vertex_begin.dtype, ms.colors.dtype) == \
        (np.float32, np.int32, np.int32, np.int32, np.uint8)
    assert ms.vertices.shape == (Vb + 4, 3) and ms.triangles.shape == (28, 3) and ms.colors.shape == (Vb + 4, 3)
    assert MeshSet([bracket, tetra]).colors is None, "colours only when asked for; further tuple entries are ignored"

    one, alone = ms.first(1), MeshSet([bracket], colors=True)
    assert one.n_objects == 1
    for name in ("vertices", "triangles", "colors", "tri_begin", "vertex_begin"):
        assert np.array_equal(getattr(one, name), getattr(alone, name)) and getattr(one, name).dtype == getattr(alone, name).dtype, name
        assert np.shares_memory(getattr(one, name), getattr(ms, name)), name
    for n in (0, 3):
        with pytest.raises(ValueError):
            ms.first(n)

    want = np.concatenate([(bv.astype(np.float64) * 1.0).astype(np.float32), (tv.astype(np.float64) * 2.0).astype(np.float32)])
    got = ms.scaled([1.0, 2.0])
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(ms.scaled(0.003), (ms.vertices.astype(np.float64) * 0.003).astype(np.float32)), "one scale for all"
    for bad in ([1.0, 2.0, 3.0], [], 0.0, [1.0, 0.0], -1.0, float("inf"), [1.0, float("nan")]):
        with pytest.raises(ValueError):
            ms.scaled(bad)


def test_host_checks_touch_no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch.Tensor, "to", no_device)
    (bv, bt, bc), tetra = _meshes()
    bad_sets = ([],
                [(bv, bt, bc), (tetra[0], np.array([[0, 1, 4]]), tetra[2])],            # an index equal to V
                [(bv, bt.astype(np.float32), bc)],                                     # not an integer array
                [(bv, bt, bc[:-1])])                                                   # a colour count different from V
    for bad in bad_sets:
        with pytest.raises(ValueError):
            MeshSet(bad, colors=True)
    with pytest.raises(ValueError, match="outside 0..3"):
        MeshSet(bad_sets[1])
    MeshSet([(bv, bt, bc), tetra], colors=True)                                         # and a good set touches none either


def test_device_tensors_are_cached_and_shared():
    ms = MeshSet(_meshes(), colors=True)
    first, again = ms.on("cpu"), ms.on(torch.device("cpu"))
    assert len(first) == 3 and all(a is b for a, b in zip(first, again))
    v, t, c = first
    assert (v.dtype, t.dtype, c.dtype) == (torch.float32, torch.int32, torch.uint8)
    assert np.array_equal(v.numpy(), ms.vertices) and np.array_equal(t.numpy(), ms.triangles) and np.array_equal(c.numpy(), ms.colors)
    one = ms.first(1)
    ov, ot, oc = one.on("cpu")
    assert ot.data_ptr() == t.data_ptr() and ov.data_ptr() == v.data_ptr() and oc.data_ptr() == c.data_ptr()
    assert ot.shape == (24, 3) and ov.shape == (len(one.vertices), 3) and ot.is_contiguous() and ov.is_contiguous()
    assert all(a is b for a, b in zip(one.on("cpu"), (ov, ot, oc)))
    assert MeshSet(_meshes()).on("cpu")[2] is None
