"""CPU: which fp32 kernel a convolution / plain-GEMM launch takes (df_conv_route, csrc/igemm.hip plan_conv) -- kernel, tile, loader,
split-K ranges and weight-group width -- on the inference engine's bench-step shapes, the 8-frame training shapes and the edges of
the rules.  The expected values are those of the launcher before it was split into a planner and a dispatch."""
import ctypes

import pytest

NONE, V1, V2, V4, V4_COLSUM, V4_MULTI = 0, 1, 2, 3, 4, 5
SCRATCH = 64 << 20        # split-K scratch bytes the training step passes (never touched here)


def _out(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def conv(B, H, W, Cin, Cout, k=1, stride=1, pad=0, dil=1, up=1, zcount=1, groups=0, splitk=0, res=False):
    """A launch descriptor; up > 1: the data-gradient launch of a stride-`up` convolution (output map `up` x the input's)."""
    OH, OW = (H * up, W * up) if up > 1 else (_out(H, k, stride, pad, dil), _out(W, k, stride, pad, dil))
    return dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=k, stride=stride, pad=pad, dil=dil, OH=OH, OW=OW, up=up, zcount=zcount, groups=groups,
                splitk=splitk, res=res)


# the engine at the bench's sizes: 40 objects per crop size (1024 padded point rows each), trunk maps of a 240 x 320 crop
ROWS = 40 * 1024
SINGLE = [
    # (what, launch, (kernel, tile rows, tile columns, loader, split-K ranges, column tiles per weight group))
    ("feat conv5", conv(ROWS, 1, 1, 256, 512), (V4, 128, 128, 1, 1, 4)),
    ("head 2, three towers", conv(ROWS, 1, 1, 640, 256, zcount=3), (V4, 128, 64, 1, 1, 4)),
    ("feat conv6 + column sums", conv(ROWS, 1, 1, 512, 1024, groups=1024), (V4_COLSUM, 128, 128, 1, 1, 8)),
    ("up_3 patches", conv(ROWS, 1, 1, 576, 64), (V4, 64, 64, 1, 1, 1)),
    ("up_2 1x1 taps", conv(40, 60, 80, 256, 576), (V4, 128, 64, 1, 1, 9)),
    ("layer2 downsample", conv(40, 60, 80, 64, 128, stride=2), (V4, 128, 64, 0, 1, 2)),
    ("stem 7x7 / 2", conv(40, 240, 320, 4, 64, k=7, stride=2, pad=3), (V4, 128, 64, 0, 1, 1)),
    ("layer1 3x3", conv(40, 60, 80, 64, 64, k=3, pad=1), (V4, 128, 64, 2, 1, 1)),
    ("layer3 3x3, dilation 2", conv(40, 30, 40, 256, 256, k=3, pad=2, dil=2), (V4, 128, 128, 2, 1, 2)),
    ("layer4 3x3, dilation 4", conv(40, 30, 40, 512, 512, k=3, pad=4, dil=4), (V4, 128, 128, 2, 1, 1)),
    # 8-frame training passes
    ("train layer4, split-K", conv(8, 20, 20, 512, 512, k=3, pad=4, dil=4, splitk=SCRATCH), (V4, 128, 64, 2, 6, 2)),
    ("train layer4, no scratch", conv(8, 20, 20, 512, 512, k=3, pad=4, dil=4), (V4, 128, 64, 2, 1, 2)),
    ("train layer4, z-batched", conv(8, 20, 20, 512, 512, k=3, pad=4, dil=4, zcount=2, splitk=SCRATCH), (V2, 128, 128, 0, 1, 1)),
    ("train layer4, one frame", conv(1, 20, 20, 512, 512, k=3, pad=4, dil=4, splitk=SCRATCH), (V4, 64, 64, 2, 8, 2)),
    ("train layer4 1x1, split-K", conv(8, 20, 20, 2048, 256, splitk=SCRATCH), (V4, 64, 64, 1, 6, 4)),
    ("train split-K, scratch too small", conv(8, 20, 20, 512, 512, k=3, pad=4, dil=4, splitk=1 << 20), (V4, 128, 64, 2, 1, 2)),
    ("train layer3, 256 tiles or more: no split", conv(8, 60, 80, 256, 256, k=3, pad=2, dil=2, splitk=SCRATCH), (V4, 128, 64, 2, 1, 4)),
    # edges
    ("strided-conv data gradient (input dilation)", conv(8, 30, 40, 256, 128, k=3, pad=1, up=2), (V1, 64, 64, 0, 1, 0)),
    ("Cout % 4 != 0", conv(8 * 1024, 1, 1, 128, 63), (V1, 64, 64, 0, 1, 0)),
    ("small square grid", conv(1024, 1, 1, 128, 128), (V2, 64, 64, 0, 1, 2)),
    ("small grid, residual", conv(8, 20, 20, 256, 256, k=3, pad=2, dil=2, res=True), (V2, 64, 64, 0, 1, 4)),
    ("nothing to compute", conv(0, 1, 1, 64, 64), (NONE, 0, 0, 0, 1, 0)),
]

# trunk maps of the 8-frame mixed window (crops 80 .. 320 px -> 10 .. 40 px), several frames of one crop size sharing a bucket
MIXED = [(1, 10, 10), (2, 15, 15), (1, 15, 20), (1, 20, 20), (1, 20, 25), (1, 25, 30), (1, 30, 40)]
MANY = [(1 + i % 3, 8 + i, 10 + (i * 7) % 13) for i in range(20)]
MULTI = [
    # (what, launch, buckets, first bucket of the launch, (kernel, tile rows, tile columns, loader, split-K, weight group, buckets covered))
    ("mixed window layer3", conv(1, 1, 1, 256, 256, k=3, pad=2, dil=2, splitk=SCRATCH), MIXED, 0, (V4_MULTI, 64, 64, 2, 1, 4, 7)),
    ("mixed window layer4", conv(1, 1, 1, 512, 512, k=3, pad=4, dil=4, splitk=SCRATCH), MIXED, 0, (V4_MULTI, 128, 64, 2, 1, 2, 7)),
    ("mixed window layer1", conv(1, 1, 1, 64, 64, k=3, pad=1), [(1, 40 * s, 40 * s) for s in (1, 2, 3)], 0, (V4_MULTI, 128, 64, 2, 1, 1, 3)),
    ("mixed window 1x1 (no plain-GEMM multi loader)", conv(1, 1, 1, 256, 512), MIXED, 0, (V4_MULTI, 128, 64, 0, 1, 8, 7)),
    ("one bucket: a launch_conv, split-K and all", conv(1, 1, 1, 512, 512, k=3, pad=4, dil=4, splitk=SCRATCH), [(8, 20, 20)], 0,
     (V4, 128, 64, 2, 6, 2, 1)),
    ("input dilation: one launch per bucket", conv(1, 1, 1, 256, 128, k=3, pad=1, up=2), MIXED, 0, (V1, 64, 64, 0, 1, 0, 1)),
    ("input dilation, third bucket", conv(1, 1, 1, 256, 128, k=3, pad=1, up=2), MIXED, 2, (V1, 64, 64, 0, 1, 0, 1)),
    ("20 buckets: first launch", conv(1, 1, 1, 128, 128, k=3, pad=1), MANY, 0, (V4_MULTI, 64, 64, 2, 1, 2, 16)),
    ("20 buckets: second launch", conv(1, 1, 1, 128, 128, k=3, pad=1), MANY, 16, (V4_MULTI, 64, 64, 2, 1, 2, 4)),
    ("17 buckets: the last one alone, still multi", conv(1, 1, 1, 128, 128, k=3, pad=1), MANY[:17], 16, (V4_MULTI, 64, 64, 2, 1, 2, 1)),
]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from densefusion_amd import _lib
    return _lib.lib()


def _desc(c):
    from densefusion_amd import _lib
    d = _lib.ConvDesc()
    # placeholder addresses: the route is planned on the host and reads no operand
    d.in_, d.wgt, d.out = 0x10000, 0x20000, 0x30000
    d.res = 0x40000 if c["res"] else None
    d.B, d.H, d.W, d.Cin, d.in_ld, d.in_coff = c["B"], c["H"], c["W"], c["Cin"], c["Cin"], 0
    d.OH, d.OW, d.Cout, d.out_ld, d.out_coff = c["OH"], c["OW"], c["Cout"], c["Cout"], 0
    d.res_ld, d.res_coff = (c["Cout"] if c["res"] else 0), 0
    d.KH = d.KW = c["k"]
    d.stride, d.pad, d.dil, d.act = c["stride"], c["pad"], c["dil"], 1
    d.splitk_ws, d.splitk_ws_bytes = (0x50000, c["splitk"]) if c["splitk"] else (None, 0)
    return d


def _route(L, c, buckets=None, first=0):
    from densefusion_amd import _lib
    r = (ctypes.c_int * 7)()
    arrs = [(ctypes.c_int * len(buckets))(*[b[i] for b in buckets]) for i in range(3)] if buckets else [None] * 3
    rc = L.df_conv_route(ctypes.byref(_desc(c)), len(buckets) if buckets else 0, *arrs, first, c["up"], c["zcount"], c["groups"], r)
    _lib.check(rc, "conv_route")
    return tuple(r)


@pytest.mark.parametrize("what,c,want", SINGLE, ids=[s[0] for s in SINGLE])
def test_single_launch_route(L, what, c, want):
    assert _route(L, c) == want + (1,), what


@pytest.mark.parametrize("what,c,buckets,first,want", MULTI, ids=[m[0] for m in MULTI])
def test_multi_bucket_route(L, what, c, buckets, first, want):
    assert _route(L, c, buckets, first) == want, what


def test_column_sum_tile_does_not_depend_on_the_batch(L):
    # the fused column sums group rows per wave: 1 object and 40 objects take the same 128 x 128 tile (small grids on v2)
    for B, kernel in ((1, V2), (7, V2), (40, V4_COLSUM)):
        assert _route(L, conv(B * 1024, 1, 1, 512, 1024, groups=1024))[:3] == (kernel, 128, 128)


def test_route_argument_errors(L):
    c = conv(8, 20, 20, 96, 64, k=3, pad=1)      # multi-tap with a Cin that is not a power of two
    r = (ctypes.c_int * 7)()
    assert L.df_conv_route(ctypes.byref(_desc(c)), 0, None, None, None, 0, 1, 1, 0, r) < 0
    assert b"power-of-two" in L.df_last_error()
    c = conv(1, 1, 1, 64, 64, k=3, pad=1)
    B, H, W = (ctypes.c_int * 2)(1, 1), (ctypes.c_int * 2)(40, 40), (ctypes.c_int * 2)(40, 40)
    assert L.df_conv_route(ctypes.byref(_desc(c)), 2, B, H, W, 2, 1, 1, 0, r) < 0        # no bucket 2
