// Implicit-GEMM convolution / batched per-point GEMM on fp32 MFMA (gfx950).
#pragma once
#include "common.h"

namespace df {

enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_PRELU = 2 };

// out[m][n] = act( sum_k A[m][k] * Wt[n][k] + bias[n] (+ res[m][n]) )
//   m = (b, oy, ox) over B*OH*OW output pixels (or points), n = output channel,
//   k = (ky, kx, c): A[m][k] = in[b][oy*stride - pad + ky*dil][ox*stride - pad + kx*dil][c]  (0 outside)
// Activations are channels-last (NHWC / point-major) fp32; weights are [Cout][KH*KW*Cin] fp32.
struct ConvParams {
  const float *in = nullptr;   // [B][H][W][in_ld], channels [in_coff, in_coff + Cin) are consumed
  const float *wgt = nullptr;  // [Cout][K]
  const float *bias = nullptr; // [Cout], or [groups][bias_group_ld] when bias_group_ld > 0, or null
  const float *res = nullptr;  // residual [M][res_ld] (channel offset res_coff) or null
  const float *prelu = nullptr;  // one shared slope (ACT_PRELU)
  float *out = nullptr;        // [M][out_ld], written at channel offset out_coff; may be null with colsum
  float *colsum = nullptr;     // optional [M/BM * WAVES_M][Cout] partial column sums of the activated output
  int B = 1, H = 1, W = 1, Cin = 0, in_ld = 0, in_coff = 0;
  int OH = 1, OW = 1, Cout = 0, out_ld = 0, out_coff = 0;
  int res_ld = 0, res_coff = 0;
  int KH = 1, KW = 1, stride = 1, pad = 0, dil = 1;
  // input dilation ("transposed conv" / dgrad of a strided conv): the input is read as if `up`-1 zeros sat between
  // its pixels: virtual coordinate v = o*stride - pad + k*dil is a real pixel v/up only when v % up == 0
  int up = 1;
  int act = ACT_NONE;
  // row groups (per-object point blocks): rows_per_group > 0 => row m belongs to group m / rows_per_group
  // and is a real point iff (m % rows_per_group) < rows_valid; used by bias_group_ld and colsum
  int rows_per_group = 0, rows_valid = 0, bias_group_ld = 0;
  // blockIdx.z "head" groups (the r/t/c towers): per-z element offsets
  int zcount = 1;
  long z_in_coff = 0, z_wgt = 0, z_bias = 0, z_out_coff = 0;
  // bf16 weight planes of `wgt` (csrc/split_gemm.hip): term p of wgt[i] at wpl[p * wpl_stride + i] (bf16 elements), cut by the weights'
  // owner once per parameter load (the inference engine, for the layers split_route takes).  null: fp32 kernels only
  const void *wpl = nullptr;
  long wpl_stride = 0;
  // split-K (training path only: opt-in through a caller-provided scratch, df_conv_desc.splitk_ws): launches that would fill less than
  // half the chip cut their reduction into ranges (blockIdx.z), partial sums go to the scratch and a fixed-order reduce kernel adds them
  // and applies bias / residual / activation (deterministic).  How many ranges: the launch plan (csrc/igemm.hip plan_conv).
  float *splitk_ws = nullptr;
  size_t splitk_ws_bytes = 0;
};

// Fused column sums add a tile's rows in per-wave groups, and that grouping must not depend on the batch size (a batched call stays
// bit-identical to solo calls): whatever tile a launch takes, a partial row covers COLSUM_ROWS output rows -- COLSUM_WAVES_M of them per
// COLSUM_BM-row tile, the tile the fp32 kernels keep for such launches (csrc/igemm.hip pick_cfg).  Shared with csrc/split_gemm.hip.
constexpr int COLSUM_BM = 128, COLSUM_WAVES_M = 2, COLSUM_ROWS = COLSUM_BM / COLSUM_WAVES_M;
inline long colsum_partial_rows(long M) { return ((M + COLSUM_BM - 1) / COLSUM_BM) * COLSUM_WAVES_M; }      // per z
// number of colsum partial rows a column-sum launch with these params writes (so callers can size the buffer before p.colsum is set)
int conv_colsum_rows(const ConvParams &p);
// FLOPs (2*MAC) of the launch, algorithmic (no padding)
double conv_flops(const ConvParams &p);
// algorithmic HBM bytes (inputs, weights, outputs and residual touched once)
double conv_bytes(const ConvParams &p);

// The data gradient of the forward launch `f` as a launch of its own (dY's maps in, dX's out, a forward stride as input dilation), host only.
// Geometry only: pointers, leading dimensions and channel offsets -- the residual on dX that accumulates among them -- are the caller's.
inline ConvParams dgrad_params(const ConvParams &f) {
  ConvParams q;
  q.B = f.B; q.H = f.OH; q.W = f.OW; q.Cin = f.Cout; q.OH = f.H; q.OW = f.W; q.Cout = f.Cin;
  q.KH = f.KH; q.KW = f.KW; q.stride = 1; q.up = f.stride; q.dil = f.dil; q.pad = f.dil * (f.KH - 1) - f.pad;
  return q;
}

// One crop-size bucket of a multi-bucket launch: B maps of H x W (outputs OH x OW) whose input / output pixel rows start at
// in_row0 / out_row0 of the concatenated buffers
struct WgradSeg { int B, H, W, OH, OW; long in_row0, out_row0; };

// What one launch of launch_conv / launch_conv_multi takes (csrc/igemm.hip plan_conv; df_conv_route reports it)
enum ConvKernel { CONV_NONE = 0, CONV_V1 = 1, CONV_V2 = 2, CONV_V4 = 3, CONV_V4_COLSUM = 4, CONV_V4_MULTI = 5, CONV_BF16 = 6 };
struct ConvRoute {
  int kernel = CONV_NONE;   // ConvKernel (CONV_NONE: nothing to compute)
  int bm = 0, bn = 0;       // workgroup tile
  int loader = 0;           // v4: 0 general, 1 plain GEMM, 2 tap-uniform
  int splitk = 1;           // K ranges
  int wgroup = 0;           // v2 / v4: column tiles per L2-resident weight group
  int nseg = 1;             // buckets of the call this launch covers
};
// The fp32 route of the launch that starts at bucket `first` of a launch_conv_multi call (nseg > 0), or of launch_conv(p) (nseg = 0):
// DF_OK or the DF_ERR_* code the call fails with.  Host only (no HIP calls).
int conv_route(const ConvParams &p, int nseg, const WgradSeg *segs, int first, ConvRoute &r);
// taken: the route of the launch (kernel CONV_BF16 when the bf16 x 6 kernel took it, csrc/split_gemm.hip)
int launch_conv(const ConvParams &p, hipStream_t st, ConvRoute *taken = nullptr);

// The same convolution over SEVERAL crop-size buckets whose pixel rows are concatenated in p.in / p.out / p.res (p.B / H / W / OH / OW are
// ignored): ONE launch of the product kernel (a workgroup's tile lies inside one bucket) per CONV_MAX_BUCKETS buckets.  Same
// sums in the same order per output element as per-bucket launch_conv calls without split-K.  Shapes the multi-bucket instantiations
// do not cover (input dilation, grouped / column-sum launches) fall back to one launch per bucket.
constexpr int CONV_MAX_BUCKETS = 16;
int launch_conv_multi(const ConvParams &p, int nseg, const WgradSeg *segs, hipStream_t st);

// dW[n][(ky,kx,c)] += sum_m dY[m][n] * A[m][(ky,kx,c)]  (A = the im2col view of x of the forward conv `p`; p.out = dY)
// dw / db (optional: column sums of dY) are overwritten.  The pixel range is split over workgroups; the partial tiles go to `ws`
// (wgrad_workspace_bytes) and are added in a fixed order: bit-reproducible, no atomics.
size_t wgrad_workspace_bytes(const ConvParams &p);
// accumulate != 0: dw / db += this launch's gradient (accumulation over the frames of an optimizer step)
int launch_wgrad(const ConvParams &p, float *dw, float *db, void *ws, size_t ws_bytes, hipStream_t st, int accumulate = 0);

// The same gradient over SEVERAL crop-size buckets whose pixel rows are concatenated in p.in (input) and p.out (dY): bucket g =
// B maps of H x W (outputs OH x OW) whose input / output pixel rows start at in_row0 / out_row0.  One contraction over the pixels of
// all buckets (chunks of the pixel axis never straddle buckets), one fixed-order reduction: bit-reproducible.  p.B / H / W / OH / OW
// are ignored; everything else (channels, strides, kernel geometry) comes from p.  Up to WGRAD_MAX_SEGS buckets per launch (more:
// several launches, the later ones accumulating).
constexpr int WGRAD_MAX_SEGS = 32;
size_t wgrad_multi_workspace_bytes(const ConvParams &p, int nseg, const WgradSeg *segs);
int launch_wgrad_multi(const ConvParams &p, int nseg, const WgradSeg *segs, float *dw, float *db, void *ws, size_t ws_bytes, hipStream_t st,
                       int accumulate = 0);

// fp32 GEMM on the bf16 matrix cores (csrc/split_gemm.hip).  Epilogue kinds of a plain-GEMM launch (gemm_epi_kind): bias / activation
// only, + residual, + per-row-group bias and / or fused column sums; anything else (residual with row groups) is not covered.
enum GemmEpi { GEMM_EPI_PLAIN = 0, GEMM_EPI_RESIDUAL = 1, GEMM_EPI_GROUPS = 2, GEMM_EPI_OTHER = 3 };
int gemm_epi_kind(const ConvParams &p);
// 1: a layer with N output channels, reduction K and this epilogue kind runs on the bf16 x 6 kernel when its weights have planes.  A pure
// function of the layer (no M, batch, crop size, z count, stream or device state): B objects in one call and B solo calls take the same path
int split_route(int N, int K, int epi);
// The 256 x 256 form's launch: `grid` workgroups walk `tiles_total` tile positions.  A z batch has ceil(tiles_m / 8) * 8 * tiles_n positions
// (whole groups of 8 row tiles: positions whose row tile is past tiles_m are padding), the batches lie one behind the other.  workgroups: the
// most the launch may have (one per compute unit); <= 0: one per position.  grid is a multiple of 8, at least 8 and at most tiles_total;
// workgroup b makes split_walk_trips(w, b) loop trips, padding positions included.  Host only (tests: df_split_walk)
struct SplitWalk { int grid, tiles_total; };
SplitWalk split_walk(int tiles_m, int tiles_n, int zcount, int workgroups);
int split_walk_trips(const SplitWalk &w, int b);
// cut `elems` weights into their three bf16 planes (term p of w[i] at planes[p * stride + i], bf16 elements) on stream st
void cut_weight_planes(const float *w, void *planes, long elems, long stride, hipStream_t st);
// launch_conv's first step: 1 when the launch was taken by the bf16 x 6 kernel (p.wpl set and split_route true; development build: also
// DF_GEMM_SPLIT_BF16) -- r is then its route: CONV_BF16 and the tile of the form it ran on --, 0 when it goes on to the fp32 kernels (r
// untouched), or a DF_ERR_* code
int try_split_gemm(const ConvParams &p, hipStream_t st, ConvRoute &r);

}  // namespace df
