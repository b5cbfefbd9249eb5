// The stand-alone convolution C API of libdfusion_hip.so (include/dfusion.h): df_conv2d_nhwc and its multi-bucket form, their data and weight
// gradients, the 3x3 convolution through the Winograd domain and the host-only route / geometry queries: what densefusion_amd/ops.py and the
// kernel tests call.  The engine and the trainer launch the same kernels through csrc/igemm.h and csrc/wino.h directly.
#include <vector>

#include "igemm.h"
#include "wino.h"

using namespace df;

// routing of a plain-GEMM layer of the inference engine (csrc/split_gemm.hip split_route)
extern "C" int df_gemm_route(int n, int k, int epilogue) { return split_route(n, k, epilogue); }

// the launch plan of the 256 x 256 form's tile walk (csrc/split_gemm.hip split_walk): host only
extern "C" int df_split_walk(int tiles_m, int tiles_n, int zcount, int workgroups, int *grid, int *tiles_total, int *trips, int cap) {
  if (tiles_m <= 0 || tiles_n <= 0 || zcount <= 0 || (long)((tiles_m + 7) / 8) * 8 * tiles_n * zcount >= (1L << 30))
    return set_error(DF_ERR_ARG, "split_walk: need positive tile counts with fewer than 2^30 positions");
  const SplitWalk w = split_walk(tiles_m, tiles_n, zcount, workgroups);
  if (grid) *grid = w.grid;
  if (tiles_total) *tiles_total = w.tiles_total;
  for (int b = 0; trips && b < w.grid && b < cap; ++b) trips[b] = split_walk_trips(w, b);
  return DF_OK;
}

// one plain-GEMM launch with the engine's epilogue options (kernel tests): dense operands, zcount batches one behind the other
extern "C" int df_gemm_rows(const float *in, const float *wgt, const float *bias, const float *res, float *out, float *colsum, int64_t M, int N,
                            int K, int zcount, int act, int rows_per_group, int rows_valid, int bias_group_ld, df_stream_t stream) {
  if (!in || !wgt || (!out && !colsum)) return set_error(DF_ERR_ARG, "gemm_rows: null pointer");
  if (M <= 0 || M >= (1L << 31) || N <= 0 || K <= 0 || zcount <= 0) return set_error(DF_ERR_ARG, "gemm_rows: bad shape");
  if (act != ACT_NONE && act != ACT_RELU) return set_error(DF_ERR_ARG, "gemm_rows: activation must be none or ReLU");
  if (rows_per_group < 0 || (rows_per_group == 0 ? rows_valid != 0 || bias_group_ld != 0 : M % rows_per_group != 0 || rows_valid <= 0 || rows_valid > rows_per_group))
    return set_error(DF_ERR_ARG, "gemm_rows: row groups must divide M, with 1 .. rows_per_group real rows each");
  if (zcount > 1 && (res || bias_group_ld > 0)) return set_error(DF_ERR_ARG, "gemm_rows: a z batch takes neither a residual nor per-group bias");
  ConvParams p;
  p.in = in; p.wgt = wgt; p.bias = bias; p.res = res; p.out = out; p.colsum = colsum;
  p.B = (int)M; p.Cin = K; p.in_ld = K; p.Cout = N; p.out_ld = N; p.res_ld = N; p.act = act;
  p.rows_per_group = rows_per_group; p.rows_valid = rows_valid; p.bias_group_ld = bias_group_ld;
  p.zcount = zcount; p.z_in_coff = M * K; p.z_wgt = (long)N * K; p.z_bias = bias ? N : 0; p.z_out_coff = M * N;
  return launch_conv(p, to_stream(stream));
}

static void desc_fields(const df_conv_desc *d, ConvParams &p) {
  p.in = d->in; p.wgt = d->wgt; p.bias = d->bias; p.res = d->res; p.prelu = d->prelu; p.out = d->out;
  p.B = d->B; p.H = d->H; p.W = d->W; p.Cin = d->Cin; p.in_ld = d->in_ld; p.in_coff = d->in_coff;
  p.OH = d->OH; p.OW = d->OW; p.Cout = d->Cout; p.out_ld = d->out_ld; p.out_coff = d->out_coff;
  p.res_ld = d->res_ld; p.res_coff = d->res_coff;
  p.KH = d->KH; p.KW = d->KW; p.stride = d->stride; p.pad = d->pad; p.dil = d->dil; p.act = d->act;
}

static int conv_desc_to_params(const df_conv_desc *d, ConvParams &p, const char *what) {
  if (!d) return set_error(DF_ERR_ARG, "%s: null descriptor", what);
  if (d->KH != d->KW) return set_error(DF_ERR_ARG, "%s: square kernels only", what);
  desc_fields(d, p);
  if (p.OH != conv_out(p.H, p.KH, p.stride, p.pad, p.dil) || p.OW != conv_out(p.W, p.KW, p.stride, p.pad, p.dil))
    return set_error(DF_ERR_ARG, "%s: OH/OW do not match the convolution geometry", what);
  return DF_OK;
}

static thread_local int t_last_splitk = 1;
extern "C" int df_conv_last_splitk(void) { return t_last_splitk; }

extern "C" int df_conv2d_nhwc(const df_conv_desc *d, df_stream_t stream) {
  ConvParams p;
  int rc = conv_desc_to_params(d, p, "conv2d_nhwc");
  if (rc != DF_OK) return rc;
  if (p.act == ACT_PRELU && !p.prelu) return set_error(DF_ERR_ARG, "conv2d_nhwc: PReLU needs a slope");
  p.splitk_ws = static_cast<float *>(d->splitk_ws); p.splitk_ws_bytes = d->splitk_ws ? d->splitk_ws_bytes : 0;
  ConvRoute taken;
  rc = launch_conv(p, to_stream(stream), &taken);
  t_last_splitk = taken.splitk;
  return rc;
}

// buckets of a multi-bucket convolution / weight-gradient call: pixel rows concatenated in bucket order in both operands
static int make_segs(const df_conv_desc *d, int nb, const int *B, const int *H, const int *W, std::vector<WgradSeg> &segs, const char *what) {
  if (!d) return set_error(DF_ERR_ARG, "%s: null descriptor", what);
  if (nb <= 0 || nb > 4096 || !B || !H || !W) return set_error(DF_ERR_ARG, "%s: need 1..4096 buckets with B / H / W arrays", what);
  if (d->KH != d->KW) return set_error(DF_ERR_ARG, "%s: square kernels only", what);
  long in_row = 0, out_row = 0;
  for (int i = 0; i < nb; ++i) {
    if (B[i] <= 0 || H[i] <= 0 || W[i] <= 0) return set_error(DF_ERR_ARG, "%s: bucket %d is empty", what, i);
    const int OH = conv_out(H[i], d->KH, d->stride, d->pad, d->dil), OW = conv_out(W[i], d->KW, d->stride, d->pad, d->dil);
    if (OH <= 0 || OW <= 0) return set_error(DF_ERR_ARG, "%s: bucket %d: the kernel does not fit the map", what, i);
    segs.push_back(WgradSeg{B[i], H[i], W[i], OH, OW, in_row, out_row});
    in_row += (long)B[i] * H[i] * W[i];
    out_row += (long)B[i] * OH * OW;
  }
  return DF_OK;
}

extern "C" int df_conv2d_nhwc_multi(const df_conv_desc *d, int nb, const int *B, const int *H, const int *W, df_stream_t stream) {
  std::vector<WgradSeg> segs;
  int rc = make_segs(d, nb, B, H, W, segs, "conv2d_nhwc_multi");
  if (rc != DF_OK) return rc;
  if (d->act == ACT_PRELU && !d->prelu) return set_error(DF_ERR_ARG, "conv2d_nhwc_multi: PReLU needs a slope");
  ConvParams p;
  desc_fields(d, p);
  p.B = p.H = p.W = p.OH = p.OW = 1;      // (the buckets carry the geometry)
  return launch_conv_multi(p, nb, segs.data(), to_stream(stream));
}

// host only: the fp32 route of a df_conv2d_nhwc (nb = 0) / df_conv2d_nhwc_multi launch (see include/dfusion.h)
extern "C" int df_conv_route(const df_conv_desc *d, int nb, const int *B, const int *H, const int *W, int first, int up, int zcount,
                             int groups, int *route) {
  if (!d || !route) return set_error(DF_ERR_ARG, "conv_route: null pointer");
  std::vector<WgradSeg> segs;
  if (nb > 0) {
    const int rc = make_segs(d, nb, B, H, W, segs, "conv_route");
    if (rc != DF_OK) return rc;
  }
  ConvParams p;
  desc_fields(d, p);
  if (nb > 0) p.B = p.H = p.W = p.OH = p.OW = 1;      // as df_conv2d_nhwc_multi
  p.splitk_ws = static_cast<float *>(d->splitk_ws); p.splitk_ws_bytes = d->splitk_ws ? d->splitk_ws_bytes : 0;
  p.up = up;
  p.zcount = zcount;
  if (groups > 0) {          // a column-sum launch over row groups: its partial-sum buffer is never touched here
    p.rows_per_group = p.rows_valid = groups;
    p.colsum = p.out;
  }
  ConvRoute r;
  const int rc = conv_route(p, nb, segs.data(), first, r);
  const int v[7] = {r.kernel, r.bm, r.bn, r.loader, r.splitk, r.wgroup, r.nseg};
  for (int i = 0; i < 7; ++i) route[i] = v[i];
  return rc;
}

extern "C" size_t df_conv2d_wgrad_multi_workspace_bytes(const df_conv_desc *d, int nb, const int *B, const int *H, const int *W) {
  std::vector<WgradSeg> segs;
  if (make_segs(d, nb, B, H, W, segs, "conv2d_wgrad_multi_workspace_bytes") != DF_OK) return 0;
  ConvParams p;
  p.Cin = d->Cin; p.Cout = d->Cout; p.KH = d->KH; p.KW = d->KW;
  return wgrad_multi_workspace_bytes(p, nb, segs.data());
}

extern "C" int df_conv2d_wgrad_nhwc_multi(const df_conv_desc *d, int nb, const int *B, const int *H, const int *W, const float *dy, float *dw, float *db,
                                          void *ws, size_t ws_bytes, df_stream_t stream) {
  std::vector<WgradSeg> segs;
  int rc = make_segs(d, nb, B, H, W, segs, "conv2d_wgrad_multi");
  if (rc != DF_OK) return rc;
  if (!dy || !dw || !d->in) return set_error(DF_ERR_ARG, "conv2d_wgrad_multi: null pointer");
  ConvParams p;
  p.in = d->in; p.out = const_cast<float *>(dy);
  p.Cin = d->Cin; p.in_ld = d->in_ld; p.in_coff = d->in_coff; p.Cout = d->Cout; p.out_ld = d->out_ld; p.out_coff = d->out_coff;
  p.KH = d->KH; p.KW = d->KW; p.stride = d->stride; p.pad = d->pad; p.dil = d->dil;
  return launch_wgrad_multi(p, nb, segs.data(), dw, db, ws, ws_bytes, to_stream(stream));
}

// 3x3 stride-1 pad=dil convolution through the Winograd F(2x2,3x3) / F(4x4,3x3) domain (wino.hip): weight transform, input
// transform, 16 / 36 batched GEMMs, output transform (+ bias, residual, ReLU).  scratch holds U | V | M.
static int wino_desc_ok(const df_conv_desc *d, const char *what) {
  if (!d) return set_error(DF_ERR_ARG, "%s: null descriptor", what);
  if (d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad != d->dil || d->dil < 1)
    return set_error(DF_ERR_ARG, "%s: needs a 3x3 kernel, stride 1, pad == dil", what);
  if (d->Cin % 4 || d->Cout % 4 || d->in_ld % 4 || d->in_coff % 4 || d->out_ld % 4 || d->out_coff % 4 || d->B <= 0 || d->H <= 0 || d->W <= 0)
    return set_error(DF_ERR_ARG, "%s: channel counts / strides must be multiples of 4", what);
  if (d->OH != d->H || d->OW != d->W) return set_error(DF_ERR_ARG, "%s: OH/OW must equal H/W", what);
  if (d->act != ACT_NONE && d->act != ACT_RELU) return set_error(DF_ERR_ARG, "%s: activation must be none or ReLU", what);
  return DF_OK;
}

extern "C" size_t df_conv3x3_winograd_tile_scratch_bytes(const df_conv_desc *d, int tile) {
  if (wino_desc_ok(d, "conv3x3_winograd_scratch_bytes") != DF_OK) return 0;
  if (tile != 2 && tile != 4) { set_error(DF_ERR_ARG, "conv3x3_winograd: tile must be 2 or 4"); return 0; }
  const WinoGeom g = wino_geom(d->B, d->H, d->W, d->dil, tile);
  const size_t nz = (size_t)(tile + 2) * (tile + 2);
  return (nz * d->Cout * d->Cin + nz * g.T * d->Cin + nz * g.T * d->Cout) * sizeof(float);
}

extern "C" int df_conv3x3_winograd_tile_nhwc(const df_conv_desc *d, int tile, void *scratch, size_t scratch_bytes, df_stream_t stream) {
  int rc = wino_desc_ok(d, "conv3x3_winograd_nhwc");
  if (rc != DF_OK) return rc;
  if (tile != 2 && tile != 4) return set_error(DF_ERR_ARG, "conv3x3_winograd: tile must be 2 or 4");
  if (!d->in || !d->wgt || !d->out || !scratch) return set_error(DF_ERR_ARG, "conv3x3_winograd_nhwc: null pointer");
  if (scratch_bytes < df_conv3x3_winograd_tile_scratch_bytes(d, tile)) return set_error(DF_ERR_WORKSPACE, "conv3x3_winograd_nhwc: scratch too small");
  const WinoGeom g = wino_geom(d->B, d->H, d->W, d->dil, tile);
  const int nz = (tile + 2) * (tile + 2);
  hipStream_t st = to_stream(stream);
  float *U = static_cast<float *>(scratch), *V = U + (size_t)nz * d->Cout * d->Cin, *M = V + (size_t)nz * g.T * d->Cin;
  launch_wino_weight(d->wgt, U, d->Cout, d->Cin, st, tile);
  launch_wino_input(d->in, d->in_ld, d->in_coff, V, d->B, d->H, d->W, d->Cin, d->dil, st, tile);
  ConvParams p;
  p.in = V; p.wgt = U; p.out = M;
  p.B = (int)g.T; p.Cin = d->Cin; p.in_ld = d->Cin; p.Cout = d->Cout; p.out_ld = d->Cout;
  p.zcount = nz; p.z_in_coff = g.T * d->Cin; p.z_wgt = (long)d->Cout * d->Cin; p.z_out_coff = g.T * d->Cout;
  rc = launch_conv(p, st);
  if (rc != DF_OK) return rc;
  launch_wino_output(M, d->out, d->out_ld, d->out_coff, d->bias, d->res, d->res_ld, d->res_coff, d->act, d->B, d->H, d->W, d->Cout, d->dil, st, tile);
  return check_launch("conv3x3_winograd_nhwc");
}

extern "C" int df_wino_route(int H, int W, int dil, int Cin, int Cout) { return wino_route(H, W, dil, Cin, Cout); }

extern "C" long df_wino_tiles(int B, int H, int W, int dil, int tile, int *packed_y, int *packed_x) {
  if (B <= 0 || H <= 0 || W <= 0 || dil < 1 || (tile != 2 && tile != 4)) { set_error(DF_ERR_ARG, "wino_tiles: bad geometry"); return -1; }
  const WinoGeom g = wino_geom(B, H, W, dil, tile);
  if (packed_y) *packed_y = g.ay.packed;
  if (packed_x) *packed_x = g.ax.packed;
  return g.T;
}

extern "C" int df_wino_axis_map(int L, int dil, int tile, int v) {
  if (L <= 0 || dil < 1 || (tile != 2 && tile != 4)) { set_error(DF_ERR_ARG, "wino_axis_map: bad geometry"); return -2; }
  const WinoAxis a = wino_axis(L, dil, tile);
  const int per_strip = tile * a.TT;          // positions 0 .. S * per_strip - 1: the strips one after another
  if (v < 0 || v >= a.S * per_strip) return -1;
  return wino_axis_coord(a, dil, v / per_strip, v % per_strip);
}

extern "C" size_t df_conv3x3_winograd_scratch_bytes(const df_conv_desc *d) { return df_conv3x3_winograd_tile_scratch_bytes(d, 2); }

extern "C" int df_conv3x3_winograd_nhwc(const df_conv_desc *d, void *scratch, size_t scratch_bytes, df_stream_t stream) {
  return df_conv3x3_winograd_tile_nhwc(d, 2, scratch, scratch_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
// training building blocks: data gradient and weight gradient of df_conv2d_nhwc
// ------------------------------------------------------------------------------------------------
namespace df {
// wt[c][ky][kx][n] = w[n][KH-1-ky][KW-1-kx][c]   (the forward conv's weights as seen by its data gradient)
__global__ void flip_transpose_kernel(const float *__restrict__ w, float *__restrict__ wt, int O, int T, int I, int KH, int KW) {
  const long total = (long)O * T * I;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int n = (int)(i % O);
    const long r = i / O;
    const int t = (int)(r % T);
    const long c = r / T;
    const int ky = t / KW, kx = t - ky * KW;
    const int tf = (KH - 1 - ky) * KW + (KW - 1 - kx);
    wt[i] = w[((size_t)n * T + tf) * I + c];
  }
}
}  // namespace df

extern "C" int df_conv2d_dgrad_nhwc(const df_conv_desc *d, const float *dy, float *dx, float *w_scratch, int accumulate,
                                    df_stream_t stream) {
  ConvParams f;
  int rc = conv_desc_to_params(d, f, "conv2d_dgrad");
  if (rc != DF_OK) return rc;
  if (!dy || !dx || !w_scratch || !f.wgt) return set_error(DF_ERR_ARG, "conv2d_dgrad: null pointer");
  if (f.Cout % 4) return set_error(DF_ERR_ARG, "conv2d_dgrad: Cout must be a multiple of 4");
  hipStream_t st = to_stream(stream);
  const int T = f.KH * f.KW;
  hipLaunchKernelGGL(flip_transpose_kernel, dim3(256), dim3(256), 0, st, f.wgt, w_scratch, f.Cout, T, f.Cin, f.KH, f.KW);
  ConvParams q = dgrad_params(f);
  q.in = dy; q.in_ld = f.out_ld; q.in_coff = f.out_coff;
  q.wgt = w_scratch;
  q.out = dx; q.out_ld = f.in_ld; q.out_coff = f.in_coff;
  if (q.pad < 0) return set_error(DF_ERR_ARG, "conv2d_dgrad: padding larger than the kernel reach is not supported");
  if (accumulate) { q.res = dx; q.res_ld = f.in_ld; q.res_coff = f.in_coff; }
  q.splitk_ws = static_cast<float *>(d->splitk_ws); q.splitk_ws_bytes = d->splitk_ws ? d->splitk_ws_bytes : 0;
  ConvRoute taken;
  rc = launch_conv(q, st, &taken);
  t_last_splitk = taken.splitk;
  return rc;
}

extern "C" size_t df_conv2d_wgrad_workspace_bytes(const df_conv_desc *d) {
  ConvParams f;
  if (conv_desc_to_params(d, f, "conv2d_wgrad_workspace_bytes") != DF_OK) return 0;
  return wgrad_workspace_bytes(f);
}

extern "C" int df_conv2d_wgrad_nhwc(const df_conv_desc *d, const float *dy, float *dw, float *db, void *ws, size_t ws_bytes, df_stream_t stream) {
  ConvParams f;
  int rc = conv_desc_to_params(d, f, "conv2d_wgrad");
  if (rc != DF_OK) return rc;
  if (!dy || !dw || !f.in) return set_error(DF_ERR_ARG, "conv2d_wgrad: null pointer");
  f.out = const_cast<float *>(dy);
  return launch_wgrad(f, dw, db, ws, ws_bytes, to_stream(stream));
}
