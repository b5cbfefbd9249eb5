"""CPU: routing of the inference engine's plain GEMMs between the fp32-MFMA kernel and the bf16 x 6 split-precision kernel
(df_gemm_route, csrc/split_gemm.hip).  The route is a function of the layer alone -- output channels, reduction length, epilogue kind --
so B objects in one call take the same kernels as B solo calls."""
import pytest

PLAIN, RESIDUAL, GROUPS, OTHER = 0, 1, 2, 3

# (what, N, K, epilogue kind, rows per object / image at the bench's sizes): every plain-GEMM launch of the PoseNet / refiner handles
ENGINE_LAYERS = [
    ("psp fold, pooled rows", 1024, 512, PLAIN, 36),
    ("psp fold, feature rows + prior", 1024, 512, RESIDUAL, 60 * 80),
    ("up_1 1x1 taps", 2304, 1024, PLAIN, 60 * 80),
    ("up_2 1x1 taps", 576, 256, PLAIN, 120 * 160),
    ("up_3 patches", 64, 576, PLAIN, 1024),
    ("layer2 Winograd domain", 128, 128, PLAIN, 400),
    ("layer3 Winograd domain", 256, 256, PLAIN, 400),
    ("layer4 Winograd domain", 512, 512, PLAIN, 400),
    ("layer2 downsample", 128, 64, PLAIN, 19200),
    ("layer3 downsample", 256, 128, PLAIN, 4800),
    ("layer4 downsample", 512, 256, PLAIN, 4800),
    ("feat e_conv1", 64, 32, PLAIN, 1024),
    ("feat conv2", 128, 64, PLAIN, 1024),
    ("feat e_conv2", 128, 64, PLAIN, 1024),
    ("feat conv5", 512, 256, PLAIN, 1024),
    ("feat conv6 + column sums", 1024, 512, GROUPS, 1024),
    ("head 1, three towers, per-object bias", 1920, 384, GROUPS, 1024),
    ("head 1, confidence tower", 640, 384, GROUPS, 1024),
    ("head 2", 256, 640, PLAIN, 1024),
    ("head 3", 128, 256, PLAIN, 1024),
    ("refiner conv5 colour part", 512, 192, PLAIN, 1024),
    ("refiner conv5 xyz part + colour", 512, 192, RESIDUAL, 1024),
]
ROUTED = {("psp fold, pooled rows"), ("psp fold, feature rows + prior"), ("up_1 1x1 taps"), ("layer4 Winograd domain"),
          ("feat conv6 + column sums"), ("head 1, three towers, per-object bias"), ("head 1, confidence tower"), ("head 2")}


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from densefusion_amd import _lib
    return _lib.lib()


def test_route_is_a_function_of_the_layer_alone(L):
    for what, n, k, epi, rows in ENGINE_LAYERS:
        # the rows a launch covers at B = 1, 7 and 40 objects do not enter the route: the same answer, asked repeatedly
        got = {B: L.df_gemm_route(n, k, epi) for B in (1, 7, 40) for _ in range(2) if rows * B > 0}
        assert len(set(got.values())) == 1, (what, got)
        assert got[1] == (what in ROUTED), (what, n, k, epi, got[1])


def test_chained_point_layers_stay_on_fp32(L):
    # csrc/pointfeat.hip chains the K = 3 / 32 / 64 layers in one launch on fp32; their layer-by-layer form must agree bit for bit
    for n in (64, 128, 256, 512, 1024):
        for k in (3, 32, 64):
            for epi in (PLAIN, RESIDUAL, GROUPS):
                assert L.df_gemm_route(n, k, epi) == 0, (n, k, epi)


def test_shapes_outside_the_kernel_cover_stay_on_fp32(L):
    for n, k, epi in ((64, 512, PLAIN), (576, 1024, PLAIN), (1000, 512, PLAIN), (1024, 400, PLAIN), (1024, 512, OTHER), (1024, 512, 7),
                      (0, 512, PLAIN), (-128, 512, PLAIN), (1024, 0, PLAIN)):
        assert L.df_gemm_route(n, k, epi) == 0, (n, k, epi)


def test_only_handles_carry_weight_planes():
    # df_conv2d_nhwc (ops.conv2d_nhwc, SegNet, the trainers) has no way to hand planes in: its descriptor is fp32 only, so those launches
    # cannot reach the split kernel in the product library
    from densefusion_amd import _lib
    names = [f[0] for f in _lib.ConvDesc._fields_]
    assert not [n for n in names if "plane" in n or "wpl" in n or "bf16" in n], names
