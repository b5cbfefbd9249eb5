// Training-mode layers of the SegNet mask network (vanilla_segmentation/segnet.py, train.py): BatchNorm2d + ReLU forward with the
// batch statistics and the running-statistics update, its backward, the adjoint of the 2x2 max-unpool and the cross-entropy loss
// (loss.py) with its logit gradient.  Channels-last fp32, C a multiple of 4.
//
// No atomics anywhere: every reduction is per-workgroup partials (a fixed row range per workgroup, fixed lane order inside it) added
// in workgroup order by a finish pass, and the number of workgroups depends on the shape only -- two identical runs are bit-identical.
#include "common.h"

namespace df {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int TB = 256;
constexpr int BN_MAX_PARTS = 1024;          // workgroups of a statistics pass (fewer for small maps: >= 16 rows per lane)
constexpr int CE_MAX_PARTS = 2048;

struct BnGrid {
  int c4, rpi, nb;          // float4 lanes per row, rows in flight per workgroup, workgroups
  long rows_per_blk;
};
inline BnGrid bn_grid(long rows, int C) {
  BnGrid g;
  g.c4 = C / 4;
  g.rpi = TB / g.c4;
  long nb = (rows + (long)g.rpi * 16 - 1) / ((long)g.rpi * 16);
  g.nb = (int)(nb < 1 ? 1 : (nb > BN_MAX_PARTS ? BN_MAX_PARTS : nb));
  g.rows_per_blk = (rows + g.nb - 1) / g.nb;
  return g;
}
// workspace: nb x 2C doubles of partials, then 3C floats of per-channel backward coefficients
inline size_t bn_ws_bytes(long rows, int C) { return (size_t)bn_grid(rows, C).nb * 2 * C * sizeof(double) + (size_t)3 * C * sizeof(float); }

inline int ce_parts(long rows) { long nb = (rows + TB - 1) / TB; return (int)(nb < 1 ? 1 : (nb > CE_MAX_PARTS ? CE_MAX_PARTS : nb)); }

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// The batch mean is kept as two floats, mu = hi + lo (lo the fp32 residual of the fp64 mean): z - hi is exact when z is near hi
// (Sterbenz), so xhat keeps its precision when the mean dwarfs the spread -- a plain fp32 mean of 1e3 alone is off by 3e-5.
__device__ __forceinline__ float bn_xhat(float z, float hi, float lo, float is) { return ((z - hi) - lo) * is; }
// the value before the ReLU; forward and backward call this one function (built with -ffp-contract=off), so the backward's ReLU mask
// is the forward's bit for bit
__device__ __forceinline__ float bn_pre(float z, float hi, float lo, float is, float g, float b) { return bn_xhat(z, hi, lo, is) * g + b; }

// Lane layout of the statistics passes: lane t owns channels 4 (t % c4) .. +3 and walks rows t / c4, + rpi, ... of the workgroup's
// range; the rpi lanes of one channel group meet in LDS and are added in lane order.
__device__ __forceinline__ void bn_lds_finish(double (*acc)[4], double *lds, int t, int c4, int rpi, double *out_s, double *out_q) {
  // acc[0] = sum, acc[1] = second sum (4 channels each); lds holds TB x 8 doubles
  for (int k = 0; k < 4; ++k) { lds[t * 8 + k] = acc[0][k]; lds[t * 8 + 4 + k] = acc[1][k]; }
  __syncthreads();
  if (t < c4) {
    double s[4], q[4];
    for (int k = 0; k < 4; ++k) { s[k] = lds[t * 8 + k]; q[k] = lds[t * 8 + 4 + k]; }
    for (int l = 1; l < rpi; ++l) {
      const int u = l * c4 + t;
      for (int k = 0; k < 4; ++k) { s[k] += lds[u * 8 + k]; q[k] += lds[u * 8 + 4 + k]; }
    }
    for (int k = 0; k < 4; ++k) { out_s[4 * t + k] = s[k]; out_q[4 * t + k] = q[k]; }
  }
}

// Forward statistics, pass 1: per workgroup and channel, the sum of d = z - z[row 0] and of d^2 in fp64.  Shifting by a sample of
// the channel keeps the later E[d^2] - E[d]^2 free of cancellation when the mean dwarfs the spread (mean 1e3, std 1).
__global__ __launch_bounds__(TB) void bn_stats_kernel(const float *__restrict__ z, long rows, int C, long rows_per_blk, double *__restrict__ part) {
  __shared__ double lds[TB * 8];
  const int c4 = C / 4, rpi = TB / c4, t = threadIdx.x;
  const int cg = t % c4, rl = t / c4;
  double acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  if (rl < rpi) {
    const f32x4 k = ld4(z + 4 * cg);
    const long r0 = blockIdx.x * rows_per_blk;
    const long r1 = r0 + rows_per_blk < rows ? r0 + rows_per_blk : rows;
    for (long r = r0 + rl; r < r1; r += rpi) {
      const f32x4 v = ld4(z + r * C + 4 * cg);
      for (int j = 0; j < 4; ++j) {
        const double d = (double)v[j] - (double)k[j];
        acc[0][j] += d;
        acc[1][j] += d * d;
      }
    }
  }
  double *p = part + (size_t)blockIdx.x * 2 * C;
  bn_lds_finish(acc, lds, t, c4, rpi, p, p + C);
}

// The finish passes: FIN_CH channels per workgroup, FIN_GROUPS lanes per channel; lane group q adds partials q, q + FIN_GROUPS, ...
// (independent loads in flight instead of one lane walking all of them), the groups meet in LDS and are added in group order.
constexpr int FIN_CH = 16, FIN_GROUPS = TB / FIN_CH;
__device__ __forceinline__ bool fin_sums(const double *__restrict__ part, int nb, int C, double &s, double &q, int &c) {
  __shared__ double lds[2][FIN_GROUPS][FIN_CH];
  const int cl = threadIdx.x % FIN_CH, g = threadIdx.x / FIN_CH;
  c = blockIdx.x * FIN_CH + cl;
  double a = 0.0, b = 0.0;
  if (c < C)
    for (int k = g; k < nb; k += FIN_GROUPS) { a += part[(size_t)k * 2 * C + c]; b += part[(size_t)k * 2 * C + C + c]; }
  lds[0][g][cl] = a;
  lds[1][g][cl] = b;
  __syncthreads();
  if (g != 0 || c >= C) return false;
  s = lds[0][0][cl];
  q = lds[1][0][cl];
  for (int k = 1; k < FIN_GROUPS; ++k) { s += lds[0][k][cl]; q += lds[1][k][cl]; }
  return true;
}

// pass 2: per channel the partials added in a fixed order; mean, biased variance, 1/sqrt(var + eps); the running statistics
// as nn.BatchNorm2d updates them (momentum m, the UNBIASED variance into running_var) and num_batches_tracked += 1
__global__ __launch_bounds__(TB) void bn_stats_finish_kernel(const float *__restrict__ z, const double *__restrict__ part, int nb, long rows, int C,
                                                             float momentum, float eps, float *__restrict__ mean, float *__restrict__ var,
                                                             float *__restrict__ invstd, float *__restrict__ run_mean, float *__restrict__ run_var,
                                                             int64_t *__restrict__ nbt) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && nbt) nbt[0] += 1;
  double s, q;
  int c;
  if (!fin_sums(part, nb, C, s, q, c)) return;
  const double n = (double)rows, ms = s / n;
  double v = q / n - ms * ms;
  v = v > 0.0 ? v : 0.0;
  const double mu = (double)z[c] + ms;
  const float hi = (float)mu;
  mean[c] = hi;
  mean[C + c] = (float)(mu - (double)hi);
  var[c] = (float)v;
  invstd[c] = (float)(1.0 / sqrt(v + (double)eps));
  if (run_mean) run_mean[c] = (float)((1.0 - (double)momentum) * (double)run_mean[c] + (double)momentum * mu);
  if (run_var) {
    const double vu = rows > 1 ? v * n / (n - 1.0) : v;
    run_var[c] = (float)((1.0 - (double)momentum) * (double)run_var[c] + (double)momentum * vu);
  }
}

// pass 3: y = relu(((z - mean) invstd) gamma + beta)
__global__ __launch_bounds__(TB) void bn_relu_apply_kernel(const float *__restrict__ z, float *__restrict__ y, const float *__restrict__ mean,
                                                           const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, long n4, int c4) {
  const int C = 4 * c4;
  for (long i = blockIdx.x * (long)TB + threadIdx.x; i < n4; i += (long)gridDim.x * TB) {
    const int c = (int)(i % c4) * 4;
    const f32x4 v = ld4(z + 4 * i);
    f32x4 o;
    for (int j = 0; j < 4; ++j) {
      const float a = bn_pre(v[j], mean[c + j], mean[C + c + j], invstd[c + j], gamma[c + j], beta[c + j]);
      o[j] = a > 0.f ? a : 0.f;
    }
    st4(y + 4 * i, o);
  }
}

// The upstream gradient of full-size row r, channels c .. c+3.  pidx == nullptr: dy is [rows][C].  Otherwise the layer feeds a 2x2
// max-pool and dy is the POOLED gradient [B][H/2][W/2][C]: the element reaches full-size pixel (y, x) only where the pool's index
// names that pixel (the max-pool adjoint read in place, never materialised at full size).
__device__ __forceinline__ f32x4 bn_upstream(const float *__restrict__ dy, const unsigned char *__restrict__ pidx, long r, int c, int C, int H, int W) {
  if (!pidx) return ld4(dy + r * C + c);
  const int x = (int)(r % W);
  const long t = r / W;
  const int yy = (int)(t % H);
  const long b = t / H;
  const long pr = (b * (H / 2) + yy / 2) * (W / 2) + x / 2;
  const unsigned pos = (unsigned)((yy & 1) * 2 + (x & 1));
  const f32x4 g = ld4(dy + pr * C + c);
  const unsigned ix = *reinterpret_cast<const unsigned *>(pidx + pr * C + c);
  f32x4 o;
  for (int j = 0; j < 4; ++j) o[j] = ((ix >> (8 * j)) & 0xffu) == pos ? g[j] : 0.f;
  return o;
}

// Backward, pass 1: per workgroup and channel, sum g and g * xhat in fp64, g = dy where the forward's ReLU passed
__global__ __launch_bounds__(TB) void bn_bwd_reduce_kernel(const float *__restrict__ dy, const unsigned char *__restrict__ pidx, int H, int W,
                                                           const float *__restrict__ z, const float *__restrict__ mean, const float *__restrict__ invstd,
                                                           const float *__restrict__ gamma, const float *__restrict__ beta, long rows, int C,
                                                           long rows_per_blk, double *__restrict__ part) {
  __shared__ double lds[TB * 8];
  const int c4 = C / 4, rpi = TB / c4, t = threadIdx.x;
  const int cg = t % c4, rl = t / c4, c = 4 * cg;
  double acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  if (rl < rpi) {
    float mu[4], lo[4], is[4], ga[4], be[4];
    for (int j = 0; j < 4; ++j) { mu[j] = mean[c + j]; lo[j] = mean[C + c + j]; is[j] = invstd[c + j]; ga[j] = gamma[c + j]; be[j] = beta[c + j]; }
    const long r0 = blockIdx.x * rows_per_blk;
    const long r1 = r0 + rows_per_blk < rows ? r0 + rows_per_blk : rows;
    for (long r = r0 + rl; r < r1; r += rpi) {
      const f32x4 v = ld4(z + r * C + c);
      const f32x4 g = bn_upstream(dy, pidx, r, c, C, H, W);
      for (int j = 0; j < 4; ++j) {
        if (!(bn_pre(v[j], mu[j], lo[j], is[j], ga[j], be[j]) > 0.f)) continue;
        const float xh = bn_xhat(v[j], mu[j], lo[j], is[j]);
        acc[0][j] += (double)g[j];
        acc[1][j] += (double)g[j] * (double)xh;
      }
    }
  }
  double *p = part + (size_t)blockIdx.x * 2 * C;
  bn_lds_finish(acc, lds, t, c4, rpi, p, p + C);
}

// pass 2: dbeta = sum g, dgamma = sum g xhat; coefficients of dz = gamma invstd (g - mean(g) - xhat mean(g xhat))
__global__ __launch_bounds__(TB) void bn_bwd_finish_kernel(const double *__restrict__ part, int nb, long rows, int C, const float *__restrict__ invstd,
                                                           const float *__restrict__ gamma, float *__restrict__ dgamma, float *__restrict__ dbeta,
                                                           float *__restrict__ coef) {
  double s, q;
  int c;
  if (!fin_sums(part, nb, C, s, q, c)) return;
  dbeta[c] = (float)s;
  dgamma[c] = (float)q;
  coef[c] = gamma[c] * invstd[c];
  coef[C + c] = (float)(s / (double)rows);
  coef[2 * C + c] = (float)(q / (double)rows);
}

// pass 3: dz, element-wise
__global__ __launch_bounds__(TB) void bn_bwd_apply_kernel(const float *__restrict__ dy, const unsigned char *__restrict__ pidx, int H, int W,
                                                          const float *__restrict__ z, const float *__restrict__ mean, const float *__restrict__ invstd,
                                                          const float *__restrict__ gamma, const float *__restrict__ beta,
                                                          const float *__restrict__ coef, float *__restrict__ dz, long n4, int C) {
  const int c4 = C / 4;
  for (long i = blockIdx.x * (long)TB + threadIdx.x; i < n4; i += (long)gridDim.x * TB) {
    const int c = (int)(i % c4) * 4;
    const long r = i / c4;
    const f32x4 v = ld4(z + 4 * i);
    const f32x4 g = bn_upstream(dy, pidx, r, c, C, H, W);
    f32x4 o;
    for (int j = 0; j < 4; ++j) {
      const float mu = mean[c + j], lo = mean[C + c + j], is = invstd[c + j];
      const float gg = bn_pre(v[j], mu, lo, is, gamma[c + j], beta[c + j]) > 0.f ? g[j] : 0.f;
      const float xh = bn_xhat(v[j], mu, lo, is);
      o[j] = coef[c + j] * ((gg - coef[C + c + j]) - xh * coef[2 * C + c + j]);
    }
    st4(dz + 4 * i, o);
  }
}

// adjoint of MaxUnpool2d(2, 2): every pooled element gathers the gradient at the position its index names.  The four window
// positions are read as whole float4 rows (the cache lines are touched either way) and selected per channel.
__global__ __launch_bounds__(TB) void maxunpool2x2_bwd_kernel(const float *__restrict__ dy, const unsigned char *__restrict__ idx,
                                                              float *__restrict__ dx, int B, int H, int W, int C) {   // H, W: pooled size
  const int c4 = C / 4;
  const long n4 = (long)B * H * W * c4;
  for (long i = blockIdx.x * (long)TB + threadIdx.x; i < n4; i += (long)gridDim.x * TB) {
    const int c = (int)(i % c4) * 4;
    long r = i / c4;
    const int ox = (int)(r % W); r /= W;
    const int oy = (int)(r % H);
    const long b = r / H;
    const float *q = dy + ((b * 2 * H + 2 * oy) * (2L * W) + 2 * ox) * C + c;
    const f32x4 g0 = ld4(q), g1 = ld4(q + C), g2 = ld4(q + 2L * W * C), g3 = ld4(q + 2L * W * C + C);
    const unsigned ix = *reinterpret_cast<const unsigned *>(idx + 4 * i);
    f32x4 o;
    for (int j = 0; j < 4; ++j) {
      const unsigned k = (ix >> (8 * j)) & 0xffu;
      o[j] = k == 0 ? g0[j] : (k == 1 ? g1[j] : (k == 2 ? g2[j] : g3[j]));
    }
    st4(dx + 4 * i, o);
  }
}

// nn.CrossEntropyLoss() (mean) over rows of `ld` floats whose first `classes` are logits, forward and backward in one pass: per row
// the max-shifted log-sum-exp, loss_r = lse - x[label], dlogits = (softmax - onehot) / rows, zeros in the padding channels.  Per
// workgroup the fp64 sum of loss_r; a label outside [0, classes) sets *bad and its row contributes nothing.
__global__ __launch_bounds__(TB) void ce_fwd_bwd_kernel(const float *__restrict__ x, const int64_t *__restrict__ label, float *__restrict__ dx,
                                                        long rows, int ld, int classes, double *__restrict__ part, int *__restrict__ bad) {
  __shared__ double lds[TB];
  const float inv_n = (float)(1.0 / (double)rows);
  double acc = 0.0;
  for (long r = blockIdx.x * (long)TB + threadIdx.x; r < rows; r += (long)gridDim.x * TB) {
    const float *p = x + r * ld;
    float *q = dx + r * ld;
    const int64_t lb = label[r];
    if (lb < 0 || lb >= classes) {
      *bad = 1;
      for (int c = 0; c < ld; ++c) q[c] = 0.f;
      continue;
    }
    float mx = p[0];
    for (int c = 1; c < classes; ++c) mx = p[c] > mx ? p[c] : mx;
    float s = 0.f;
    for (int c = 0; c < classes; ++c) s += expf(p[c] - mx);
    const float inv_s = 1.f / s;
    acc += (double)mx + (double)logf(s) - (double)p[lb];
    for (int c = 0; c < classes; ++c) q[c] = (expf(p[c] - mx) * inv_s - (c == (int)lb ? 1.f : 0.f)) * inv_n;
    for (int c = classes; c < ld; ++c) q[c] = 0.f;
  }
  lds[threadIdx.x] = acc;
  __syncthreads();
  for (int d = TB / 2; d >= 1; d >>= 1) { if (threadIdx.x < d) lds[threadIdx.x] += lds[threadIdx.x + d]; __syncthreads(); }
  if (threadIdx.x == 0) part[blockIdx.x] = lds[0];
}
__global__ __launch_bounds__(TB) void ce_finish_kernel(const double *__restrict__ part, int nb, long rows, float *__restrict__ loss) {
  __shared__ double lds[TB];
  double a = 0.0;
  for (int i = threadIdx.x; i < nb; i += TB) a += part[i];
  lds[threadIdx.x] = a;
  __syncthreads();
  for (int d = TB / 2; d >= 1; d >>= 1) { if (threadIdx.x < d) lds[threadIdx.x] += lds[threadIdx.x + d]; __syncthreads(); }
  if (threadIdx.x == 0) loss[0] = (float)(lds[0] / (double)rows);
}

inline int ew_blocks(long n4) { long b = (n4 + TB - 1) / TB; return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b)); }

}  // namespace
}  // namespace df

using namespace df;
#define ST to_stream(stream)
#define NN(p) if (!(p)) return set_error(DF_ERR_ARG, "%s: null pointer", __func__)

static int bn_check(long rows, int C, size_t ws_bytes, const char *what) {
  if (rows < 1 || C < 4 || C % 4 || C > 4 * TB) return set_error(DF_ERR_ARG, "%s: need rows >= 1 and C a multiple of 4 in [4, %d]", what, 4 * TB);
  if (ws_bytes < bn_ws_bytes(rows, C)) return set_error(DF_ERR_ARG, "%s: workspace of %zu bytes, need %zu", what, ws_bytes, bn_ws_bytes(rows, C));
  return DF_OK;
}

extern "C" size_t df_bn_workspace_bytes(int64_t rows, int C) {
  if (rows < 1 || C < 4 || C % 4 || C > 4 * TB) return 0;
  return bn_ws_bytes((long)rows, C);
}

extern "C" int df_bn_relu_fwd_train(const float *z, float *y, const float *gamma, const float *beta, float *running_mean, float *running_var,
                                    int64_t *num_batches_tracked, float *mean, float *var, float *invstd, int64_t rows, int C, float momentum,
                                    float eps, void *ws, size_t ws_bytes, df_stream_t stream) {
  NN(z); NN(y); NN(gamma); NN(beta); NN(mean); NN(var); NN(invstd); NN(ws);
  if (int e = bn_check((long)rows, C, ws_bytes, "bn_relu_fwd_train")) return e;
  const BnGrid g = bn_grid((long)rows, C);
  double *part = static_cast<double *>(ws);
  hipLaunchKernelGGL(bn_stats_kernel, dim3(g.nb), dim3(TB), 0, ST, z, (long)rows, C, g.rows_per_blk, part);
  hipLaunchKernelGGL(bn_stats_finish_kernel, dim3(cdiv(C, FIN_CH)), dim3(TB), 0, ST, z, part, g.nb, (long)rows, C, momentum, eps, mean, var, invstd,
                     running_mean, running_var, num_batches_tracked);
  const long n4 = (long)rows * (C / 4);
  hipLaunchKernelGGL(bn_relu_apply_kernel, dim3(ew_blocks(n4)), dim3(TB), 0, ST, z, y, mean, invstd, gamma, beta, n4, C / 4);
  return check_launch("bn_relu_fwd_train");
}

extern "C" int df_bn_relu_bwd(const float *dy, const unsigned char *pool_idx, int H, int W, const float *z, const float *mean,
                              const float *invstd, const float *gamma, const float *beta, float *dz, float *dgamma, float *dbeta, int64_t rows,
                              int C, void *ws, size_t ws_bytes, df_stream_t stream) {
  NN(dy); NN(z); NN(mean); NN(invstd); NN(gamma); NN(beta); NN(dz); NN(dgamma); NN(dbeta); NN(ws);
  if (int e = bn_check((long)rows, C, ws_bytes, "bn_relu_bwd")) return e;
  if (pool_idx && (H < 2 || W < 2 || (H & 1) || (W & 1) || rows % ((int64_t)H * W)))
    return set_error(DF_ERR_ARG, "bn_relu_bwd: a pooled gradient needs even H, W >= 2 and rows a multiple of H * W");
  const BnGrid g = bn_grid((long)rows, C);
  double *part = static_cast<double *>(ws);
  float *coef = reinterpret_cast<float *>(part + (size_t)g.nb * 2 * C);
  hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(g.nb), dim3(TB), 0, ST, dy, pool_idx, H, W, z, mean, invstd, gamma, beta, (long)rows, C,
                     g.rows_per_blk, part);
  hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3(cdiv(C, FIN_CH)), dim3(TB), 0, ST, part, g.nb, (long)rows, C, invstd, gamma, dgamma, dbeta, coef);
  const long n4 = (long)rows * (C / 4);
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(ew_blocks(n4)), dim3(TB), 0, ST, dy, pool_idx, H, W, z, mean, invstd, gamma, beta, coef, dz, n4, C);
  return check_launch("bn_relu_bwd");
}

extern "C" int df_maxunpool2x2_bwd(const float *dy, const unsigned char *idx, float *dx, int B, int H, int W, int C, df_stream_t stream) {
  NN(dy); NN(idx); NN(dx);
  if (B <= 0 || H <= 0 || W <= 0 || C < 4 || C % 4) return set_error(DF_ERR_ARG, "maxunpool2x2_bwd: bad sizes (C a multiple of 4)");
  hipLaunchKernelGGL(maxunpool2x2_bwd_kernel, dim3(ew_blocks((long)B * H * W * (C / 4))), dim3(TB), 0, ST, dy, idx, dx, B, H, W, C);
  return check_launch("maxunpool2x2_bwd");
}

extern "C" size_t df_cross_entropy_workspace_bytes(int64_t rows) { return rows < 1 ? 0 : (size_t)ce_parts((long)rows) * sizeof(double); }

extern "C" int df_cross_entropy_nhwc(const float *logits, const int64_t *target, float *dlogits, int64_t rows, int ld, int classes, float *loss,
                                     int *bad_label, void *ws, size_t ws_bytes, df_stream_t stream) {
  NN(logits); NN(target); NN(dlogits); NN(loss); NN(bad_label); NN(ws);
  if (rows < 1 || classes < 1 || ld < classes) return set_error(DF_ERR_ARG, "cross_entropy_nhwc: need rows >= 1 and 1 <= classes <= ld");
  const int nb = ce_parts((long)rows);
  if (ws_bytes < (size_t)nb * sizeof(double)) return set_error(DF_ERR_ARG, "cross_entropy_nhwc: workspace too small");
  double *part = static_cast<double *>(ws);
  hipMemsetAsync(bad_label, 0, sizeof(int), ST);
  hipLaunchKernelGGL(ce_fwd_bwd_kernel, dim3(nb), dim3(TB), 0, ST, logits, target, dlogits, (long)rows, ld, classes, part, bad_label);
  hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(TB), 0, ST, part, nb, (long)rows, loss);
  return check_launch("cross_entropy_nhwc");
}
