// Glue kernels of the native training step (train.hip includes this file, and nothing else does): what runs between the MFMA launches --
// activation / pooling / resampling adjoints, the chosen-pixel up_3 gather, the point branch's first layer, the heads' last layer, the
// refiner's tail, the weight flips and the state-dict relayout -- with the bucket table (BTab) that the memory-bound ones take as an argument.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace df {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int TB = 256;
inline unsigned nblk(long n, long cap = 16384) { long b = (n + TB - 1) / TB; return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b)); }
#define GRID_STRIDE(i, n) for (long i = blockIdx.x * (long)TB + threadIdx.x; i < (n); i += (long)gridDim.x * TB)

// ------------------------------------------------------------------------------------------------
// kernels (the glue between the MFMA launches; every sum in a fixed order)
// ------------------------------------------------------------------------------------------------

// g <- g * act'(y) in place on a [rows][C] view; PReLU (act 2) also leaves per-workgroup partial sums of dslope in `part`
__global__ __launch_bounds__(TB) void act_bwd2d_kernel(float *__restrict__ g, int g_ld, const float *__restrict__ y, int y_ld, long rows, int C4,
                                                       int act, const float *__restrict__ slope_p, float *__restrict__ part) {
  __shared__ float s_red[TB];
  const float slope = act == 2 ? slope_p[0] : 0.f;
  float ds = 0.f;
  GRID_STRIDE(i, rows * C4) {
    const long r = i / C4;
    const int c = (int)(i - r * C4) * 4;
    f32x4 gv = *reinterpret_cast<f32x4 *>(g + r * g_ld + c);
    const f32x4 yv = *reinterpret_cast<const f32x4 *>(y + r * y_ld + c);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (!(yv[e] > 0.f)) {
        if (act == 2) ds += gv[e] * (yv[e] / slope);        // x = y / slope on the negative side
        gv[e] *= slope;
      }
    *reinterpret_cast<f32x4 *>(g + r * g_ld + c) = gv;
  }
  if (act == 2) {
    s_red[threadIdx.x] = ds;
    __syncthreads();
    for (int d = TB / 2; d >= 1; d >>= 1) { if ((int)threadIdx.x < d) s_red[threadIdx.x] += s_red[threadIdx.x + d]; __syncthreads(); }
    if (threadIdx.x == 0) part[blockIdx.x] = s_red[0];
  }
}

// dst[j] (+)= sum_i part[i * n + j]: one thread per output, i ascending (n > 1); for a single output (n == 1: the PReLU slope) one
// workgroup, thread t adds part[t], part[t + 256], ... and the 256 sums meet in a fixed tree
__global__ __launch_bounds__(TB) void sum_partials_kernel(const float *__restrict__ part, int count, long n, float *__restrict__ dst, int accumulate) {
  if (n == 1) {
    __shared__ float s_red[TB];
    float a = 0.f;
    for (int i = threadIdx.x; i < count; i += TB) a += part[i];
    s_red[threadIdx.x] = a;
    __syncthreads();
    for (int d = TB / 2; d >= 1; d >>= 1) { if ((int)threadIdx.x < d) s_red[threadIdx.x] += s_red[threadIdx.x + d]; __syncthreads(); }
    if (threadIdx.x == 0) dst[0] = accumulate ? dst[0] + s_red[0] : s_red[0];
    return;
  }
  GRID_STRIDE(j, n) {
    float a = 0.f;
    for (int i = 0; i < count; ++i) a += part[(long)i * n + j];
    dst[j] = accumulate ? dst[j] + a : a;
  }
}

// dst (+)= src on [rows][C] views
__global__ __launch_bounds__(TB) void add2d_kernel(float *__restrict__ dst, int d_ld, const float *__restrict__ src, int s_ld, long rows, int C4) {
  GRID_STRIDE(i, rows * C4) {
    const long r = i / C4;
    const int c = (int)(i - r * C4) * 4;
    f32x4 a = *reinterpret_cast<f32x4 *>(dst + r * d_ld + c);
    const f32x4 b = *reinterpret_cast<const f32x4 *>(src + r * s_ld + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] += b[e];
    *reinterpret_cast<f32x4 *>(dst + r * d_ld + c) = a;
  }
}

// bilinear source (ATen UpSample semantics, fp32): align != 0 -> src = dst*(in-1)/(out-1); else half-pixel, clamped at 0
__device__ inline void bil_src(int dst, int in_size, int out_size, int align, int &i0, int &i1, float &l0, float &l1) {
  float s;
  if (align) s = (out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f) * (float)dst;
  else { s = ((float)in_size / (float)out_size) * ((float)dst + 0.5f) - 0.5f; if (s < 0.f) s = 0.f; }
  i0 = (int)s;
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = s - (float)i0;
  l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
  l0 = 1.f - l1;
}
// the destination indices that may interpolate from source index q: a conservative range, every candidate is re-checked with bil_src
__device__ inline void bil_cands(int q, int in_size, int out_size, int align, int &lo, int &hi) {
  const float inv = align ? (in_size > 1 ? (float)(out_size - 1) / (float)(in_size - 1) : (float)out_size)
                          : (float)out_size / (float)in_size;
  lo = (int)floorf(((float)q - 1.f) * inv) - 2;
  hi = (int)ceilf(((float)q + 1.5f) * inv) + 2;
  if (lo < 0 || q == 0) lo = 0;
  if (hi > out_size - 1 || q == in_size - 1) hi = out_size - 1;
}

// ------------------------------------------------------------------------------------------------
// Memory-bound kernels over ALL crop-size buckets of a level in one launch: a bucket table travels in the kernel arguments, an element
// finds its bucket by a scan of <= 16 row bounds (the buckets' pixel rows are concatenated, bucket g = B[g] maps of H[g] x W[g] from
// row row0[g]; its frames are b0[g] .. of the pass).
// ------------------------------------------------------------------------------------------------
constexpr int TAB_MAX = 16;
struct BTab {
  int n;
  int B[TAB_MAX], H[TAB_MAX], W[TAB_MAX], b0[TAB_MAX];
  long row0[TAB_MAX], row1[TAB_MAX];      // first pixel row, one past the last
  long aux0[TAB_MAX];                     // first row of the bucket in a second level (pooled / convolved maps), where a kernel needs one
};
__device__ inline int tab_of_row(const BTab &t, long row) {
  int g = 0;
  while (g + 1 < t.n && row >= t.row1[g]) ++g;
  return g;
}
__device__ inline int tab_of_frame(const BTab &t, int frame) {
  int g = 0;
  while (g + 1 < t.n && frame >= t.b0[g + 1]) ++g;
  return g;
}

// y[r][c] = x[r][c] * scale[frame(r)][c]  (Dropout2d and its adjoint)
__global__ __launch_bounds__(TB) void channel_scale_multi_kernel(const float *__restrict__ x, int x_ld, const float *__restrict__ scale, float *__restrict__ y,
                                                                 int y_ld, int C4, const BTab tab) {
  const long r_lo = tab.row0[0], nrow = tab.row1[tab.n - 1] - r_lo;
  GRID_STRIDE(i, nrow * C4) {
    const long r = r_lo + i / C4;
    const int c = (int)(i % C4) * 4;
    const int g = tab_of_row(tab, r);
    const int frame = tab.b0[g] + (int)((r - tab.row0[g]) / ((long)tab.H[g] * tab.W[g]));
    const f32x4 v = *reinterpret_cast<const f32x4 *>(x + r * x_ld + c), sc = *reinterpret_cast<const f32x4 *>(scale + (size_t)frame * C4 * 4 + c);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = v[e] * sc[e];
    *reinterpret_cast<f32x4 *>(y + r * y_ld + c) = o;
  }
}

// AdaptiveAvgPool2d adjoint of the FOUR pyramid stages (sizes 1, 2, 3, 6) at once, lib/pspnet.py:16: bin i of stage s covers
// [floor(i*H/s), ceil((i+1)*H/s)); dx[pix] (+)= sum_s sum over the stage's bins that contain the pixel of dy_s[frame][bin] / |bin| (stages
// ascending, bins row-major: a fixed order); dy_s = [frames][s*s][C] blocks
struct Ptr4 { const float *p[4]; };
struct MPtr4 { float *p[4]; };
__global__ __launch_bounds__(TB) void pool_bwd_all_kernel(const Ptr4 dy, float *__restrict__ dx, int dx_ld, int C4, int accumulate, const BTab tab) {
  const long r_lo = tab.row0[0], nrow = tab.row1[tab.n - 1] - r_lo;
  GRID_STRIDE(i, nrow * C4) {
    const long r = r_lo + i / C4;
    const int c4 = (int)(i % C4);
    const int g = tab_of_row(tab, r);
    const int H = tab.H[g], W = tab.W[g];
    long l = r - tab.row0[g];
    const int xx = (int)(l % W); l /= W;
    const int yy = (int)(l % H);
    const int frame = tab.b0[g] + (int)(l / H);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int si = 0; si < 4; ++si) {
      const int s = si == 0 ? 1 : si == 1 ? 2 : si == 2 ? 3 : 6;
      const float *d = dy.p[si] + (size_t)frame * s * s * C4 * 4;
      // the bins that contain pixel yy are exactly floor(yy*s/H) .. ceil((yy+1)*s/H) - 1: more than three of them where the map is
      // narrower than s/2 (a 1 x 1 map lies in all 36 bins of the 6-bin stage)
      for (int bi = yy * s / H; bi <= ((yy + 1) * s + H - 1) / H - 1; ++bi) {
        const int y0 = (bi * H) / s, y1 = ((bi + 1) * H + s - 1) / s;
        for (int bj = xx * s / W; bj <= ((xx + 1) * s + W - 1) / W - 1; ++bj) {
          const int x0 = (bj * W) / s, x1 = ((bj + 1) * W + s - 1) / s;
          const f32x4 v = reinterpret_cast<const f32x4 *>(d)[(size_t)(bi * s + bj) * C4 + c4];
          const float cnt = (float)((y1 - y0) * (x1 - x0));
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] += v[e] / cnt;
        }
      }
    }
    float *o = dx + r * dx_ld + c4 * 4;
    if (accumulate) {
      const f32x4 old = *reinterpret_cast<const f32x4 *>(o);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = old[e] + acc[e];
    }
    *reinterpret_cast<f32x4 *>(o) = acc;
  }
}

// the four pyramid priors (bilinear, align_corners = False, lib/pspnet.py:22) of every bucket: y[r][si * C + c] from z_si [frames][s*s][C]
__global__ __launch_bounds__(TB) void bilinear_fwd_all_kernel(const Ptr4 z, float *__restrict__ y, int y_ld, int C4, const BTab tab) {
  const long r_lo = tab.row0[0], nrow = tab.row1[tab.n - 1] - r_lo;
  GRID_STRIDE(i, nrow * 4 * C4) {
    const int c4 = (int)(i % C4);
    const int si = (int)((i / C4) % 4);
    const long r = r_lo + i / (4 * C4);
    const int g = tab_of_row(tab, r);
    const int OH = tab.H[g], OW = tab.W[g];
    long l = r - tab.row0[g];
    const int ox = (int)(l % OW); l /= OW;
    const int oy = (int)(l % OH);
    const int frame = tab.b0[g] + (int)(l / OH);
    const int s = si == 0 ? 1 : si == 1 ? 2 : si == 2 ? 3 : 6;
    int y0, y1, x0, x1;
    float wy0, wy1, wx0, wx1;
    bil_src(oy, s, OH, 0, y0, y1, wy0, wy1);
    bil_src(ox, s, OW, 0, x0, x1, wx0, wx1);
    const f32x4 *p = reinterpret_cast<const f32x4 *>(z.p[si]) + (size_t)frame * s * s * C4 + c4;
    const f32x4 v00 = p[(size_t)(y0 * s + x0) * C4], v01 = p[(size_t)(y0 * s + x1) * C4], v10 = p[(size_t)(y1 * s + x0) * C4], v11 = p[(size_t)(y1 * s + x1) * C4];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = wy0 * (wx0 * v00[e] + wx1 * v01[e]) + wy1 * (wx0 * v10[e] + wx1 * v11[e]);
    *reinterpret_cast<f32x4 *>(y + r * y_ld + (size_t)si * C4 * 4 + c4 * 4) = o;
  }
}

// their adjoint as a gather, all four stages and all buckets: dz_si[frame][q] = sum over the destination pixels that read stage pixel q of
// weight * dy; dz_si = [frames][s*s][C].  job = (stage, frame, q, group of 8 channel vectors); workgroup = 8 channel vectors x 32 pixel lanes:
// lane l takes the candidate destination pixels l, l + 32, ... of q's (row range) x (column range) window, the 32 partial sums meet in LDS
// and are added in lane order -- a fixed order, and 32 load chains per output instead of one (the 1 x 1 stage gathers the whole map into
// one pixel: with 8 row lanes it was the longest glue kernel of a mixed-size training window)
__global__ __launch_bounds__(TB) void bilinear_bwd_all_kernel(const float *__restrict__ dy, int dy_ld, const MPtr4 dz, int frames, int C4, const BTab tab) {
  __shared__ f32x4 s_p[32][8];
  const int col = threadIdx.x & 7, pl = threadIdx.x >> 3;
  const int cgroups = (C4 + 7) / 8;
  const long per_frame = 50L * cgroups;                   // 1 + 4 + 9 + 36 stage pixels
  for (long job = blockIdx.x; job < (long)frames * per_frame; job += gridDim.x) {
    const int frame = tab.b0[0] + (int)(job / per_frame);          // (`frames` counts the table's frames; dz / dy are indexed by the absolute frame)
    long rem = job - (job / per_frame) * per_frame;
    const int cg = (int)(rem % cgroups);
    int q = (int)(rem / cgroups);
    int si = 0, s = 1;
    if (q >= 14) { si = 3; s = 6; q -= 14; } else if (q >= 5) { si = 2; s = 3; q -= 5; } else if (q >= 1) { si = 1; s = 2; q -= 1; }
    const int qy = q / s, qx = q - qy * s;
    const int g = tab_of_frame(tab, frame);
    const int OH = tab.H[g], OW = tab.W[g];
    const float *src = dy + (tab.row0[g] + (long)(frame - tab.b0[g]) * OH * OW) * dy_ld + (size_t)si * C4 * 4;
    const int c4 = cg * 8 + col;
    int ylo, yhi, xlo, xhi;
    bil_cands(qy, s, OH, 0, ylo, yhi);
    bil_cands(qx, s, OW, 0, xlo, xhi);
    const int nx = xhi - xlo + 1, total = (yhi - ylo + 1) * nx;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (c4 < C4)
      for (int idx = pl; idx < total; idx += 32) {
        const int oy = ylo + idx / nx, ox = xlo + idx % nx;
        int y0, y1, x0, x1;
        float wy0, wy1, wx0, wx1;
        bil_src(oy, s, OH, 0, y0, y1, wy0, wy1);
        if (y0 != qy && y1 != qy) continue;
        bil_src(ox, s, OW, 0, x0, x1, wx0, wx1);
        if (x0 != qx && x1 != qx) continue;
        const float wy = (y0 == qy ? wy0 : 0.f) + (y1 == qy ? wy1 : 0.f);
        const float wx = (x0 == qx ? wx0 : 0.f) + (x1 == qx ? wx1 : 0.f);
        const f32x4 gv = *reinterpret_cast<const f32x4 *>(src + ((long)oy * OW + ox) * dy_ld + c4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += (wy * wx) * gv[e];
      }
    s_p[pl][col] = acc;
    __syncthreads();
    if (pl == 0 && c4 < C4) {
#pragma unroll 4
      for (int l = 1; l < 32; ++l)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += s_p[l][col][e];
      reinterpret_cast<f32x4 *>(dz.p[si])[((size_t)frame * s * s + q) * C4 + c4] = acc;
    }
    __syncthreads();
  }
}

// Adjoint of layers.hip upconv_gather (PSPUpsample through the low-resolution per-tap products) over all buckets: g [B][2h][2w][Cout] is
// the gradient of the pre-activation, its rows live at the upsampled level (4 x the low-resolution rows of each bucket);
// dY[b][qy][qx][tap][c] = sum over the upsampled positions u = P + tap - 1 (inside the image) that interpolate from (qy, qx) of
// weight(u -> q) * g[P]
__global__ __launch_bounds__(TB) void upconv_gather_bwd_multi_kernel(const float *__restrict__ gsrc, float *__restrict__ dY, int Cout, const BTab tab) {
  const int C4 = Cout / 4;
  const long r_lo = tab.row0[0], nrow = tab.row1[tab.n - 1] - r_lo;
  GRID_STRIDE(i, nrow * 9 * C4) {
    const int c = (int)(i % C4) * 4;
    long r = i / C4;
    const int tap = (int)(r % 9); r /= 9;
    const long row = r_lo + r;
    const int gi = tab_of_row(tab, row);
    const int h = tab.H[gi], w = tab.W[gi], OH = 2 * h, OW = 2 * w;
    long l = row - tab.row0[gi];
    const int qx = (int)(l % w); l /= w;
    const int qy = (int)(l % h);
    const int b = (int)(l / h);
    const float *g = gsrc + 4 * tab.row0[gi] * Cout;
    const int dy = tap / 3, dx = tap - dy * 3;
    int ylo, yhi, xlo, xhi;
    bil_cands(qy, h, OH, 1, ylo, yhi);
    bil_cands(qx, w, OW, 1, xlo, xhi);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // the column candidates' weights once per thread (not under every row candidate); the products are added in candidate order
    constexpr int MAXC = 8;      // (a source column feeds at most 5 upsampled columns at scale 2)
    float wxs[MAXC];
    int pxs[MAXC];
    int ncx = 0;
    for (int ux = xlo; ux <= xhi && ncx < MAXC; ++ux) {
      const int px = ux - dx + 1;
      if ((unsigned)px >= (unsigned)OW) continue;
      int x0, x1;
      float wx0, wx1;
      bil_src(ux, w, OW, 1, x0, x1, wx0, wx1);
      if (x0 != qx && x1 != qx) continue;
      wxs[ncx] = (x0 == qx ? wx0 : 0.f) + (x1 == qx ? wx1 : 0.f);
      pxs[ncx++] = px;
    }
    for (int uy = ylo; uy <= yhi; ++uy) {
      const int py = uy - dy + 1;
      if ((unsigned)py >= (unsigned)OH) continue;
      int y0, y1;
      float wy0, wy1;
      bil_src(uy, h, OH, 1, y0, y1, wy0, wy1);
      if (y0 != qy && y1 != qy) continue;
      const float wy = (y0 == qy ? wy0 : 0.f) + (y1 == qy ? wy1 : 0.f);
      for (int k = 0; k < ncx; ++k) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(g + ((long)(b * OH + py) * OW + pxs[k]) * Cout + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += (wy * wxs[k]) * v[e];
      }
    }
    reinterpret_cast<f32x4 *>(dY)[(row * 9 + tap) * C4 + c / 4] = acc;
  }
}

// MaxPool2d(3, stride 2, pad 1) adjoint over all buckets (trainops.hip maxpool3s2_bwd_kernel: first-maximum rule); tab = the INPUT level,
// aux0 = the buckets' first rows at the pooled level
__global__ __launch_bounds__(TB) void maxpool3s2_bwd_multi_kernel(const float *__restrict__ x, const float *__restrict__ dy, float *__restrict__ dx, int C,
                                                                  const BTab tab) {
  // thread = 4 channels of one input pixel (16-byte loads; the per-channel decisions and the order of the additions are those of the
  // one-channel form: 79 -> 25 us on the stem's 8 x 80 x 80 x 64 map)
  const int C4 = C / 4;
  const long r_lo = tab.row0[0], nrow = tab.row1[tab.n - 1] - r_lo;
  GRID_STRIDE(i, nrow * C4) {
    const int c = (int)(i % C4) * 4;
    const long row = r_lo + i / C4;
    const int g = tab_of_row(tab, row);
    const int H = tab.H[g], W = tab.W[g], OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    long l = row - tab.row0[g];
    const int ix = (int)(l % W); l /= W;
    const int iy = (int)(l % H);
    const int b = (int)(l / H);
    const float *xb = x + (tab.row0[g] + (long)b * H * W) * C + c;
    const float *dyb = dy + (tab.aux0[g] + (long)b * OH * OW) * C + c;
    const f32x4 xv = *reinterpret_cast<const f32x4 *>(xb + ((long)iy * W + ix) * C);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int oy = (iy + 1) / 2 - 1 < 0 ? 0 : (iy + 1) / 2 - 1; oy <= (iy + 1) / 2 && oy < OH; ++oy) {
      if (iy < oy * 2 - 1 || iy > oy * 2 + 1) continue;
      for (int ox = (ix + 1) / 2 - 1 < 0 ? 0 : (ix + 1) / 2 - 1; ox <= (ix + 1) / 2 && ox < OW; ++ox) {
        if (ix < ox * 2 - 1 || ix > ox * 2 + 1) continue;
        bool win[4] = {true, true, true, true};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const int yy = oy * 2 - 1 + ky;
          if ((unsigned)yy >= (unsigned)H) continue;
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const int xx = ox * 2 - 1 + kx;
            if ((unsigned)xx >= (unsigned)W) continue;
            const f32x4 v = *reinterpret_cast<const f32x4 *>(xb + ((long)yy * W + xx) * C);
            const bool earlier = yy < iy || (yy == iy && xx < ix);
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (v[e] > xv[e] || (earlier && v[e] == xv[e])) win[e] = false;
          }
        }
        const f32x4 d = *reinterpret_cast<const f32x4 *>(dyb + ((long)oy * OW + ox) * C);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += win[e] ? d[e] : 0.f;
      }
    }
    *reinterpret_cast<f32x4 *>(dx + row * C + c) = acc;
  }
}

// Data gradient of a STRIDED convolution from its per-tap products (col2im as a gather): dcol[m][tap * C + c] = sum_n dY[m][n] w[n][tap][c]
// for every output pixel m (one GEMM over the rows of all buckets); an input pixel collects the <= ceil(k / stride)^2 (tap, output pixel)
// pairs that read it, taps in row-major order (fixed order).  tab = the INPUT level, aux0 = the buckets' first rows at the output level.
__global__ __launch_bounds__(TB) void col2im_multi_kernel(const float *__restrict__ dcol, float *__restrict__ dx, int dx_ld, int C, int k, int stride, int pad,
                                                          int dil, int accumulate, const BTab tab) {
  const int C4 = C / 4;
  const long r_lo = tab.row0[0], nrow = tab.row1[tab.n - 1] - r_lo;
  GRID_STRIDE(i, nrow * C4) {
    const int c4 = (int)(i % C4);
    const long row = r_lo + i / C4;
    const int g = tab_of_row(tab, row);
    const int H = tab.H[g], W = tab.W[g];
    const int OH = (H + 2 * pad - dil * (k - 1) - 1) / stride + 1, OW = (W + 2 * pad - dil * (k - 1) - 1) / stride + 1;
    long l = row - tab.row0[g];
    const int ix = (int)(l % W); l /= W;
    const int iy = (int)(l % H);
    const int b = (int)(l / H);
    const float *src = dcol + (tab.aux0[g] + (long)b * OH * OW) * (size_t)(k * k * C);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int ky = 0; ky < k; ++ky) {
      const int ty = iy + pad - ky * dil;
      if (ty < 0 || ty % stride) continue;
      const int oy = ty / stride;
      if (oy >= OH) continue;
      for (int kx = 0; kx < k; ++kx) {
        const int tx = ix + pad - kx * dil;
        if (tx < 0 || tx % stride) continue;
        const int ox = tx / stride;
        if (ox >= OW) continue;
        const f32x4 v = *reinterpret_cast<const f32x4 *>(src + ((long)oy * OW + ox) * (size_t)(k * k * C) + (size_t)(ky * k + kx) * C + c4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += v[e];
      }
    }
    float *o = dx + row * dx_ld + c4 * 4;
    if (accumulate) {
      const f32x4 old = *reinterpret_cast<const f32x4 *>(o);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = old[e] + acc[e];
    }
    *reinterpret_cast<f32x4 *>(o) = acc;
  }
}

// Adjoint of layers.hip up3_patch (the 3x3 patch of the bilinearly upsampled half-resolution map at every chosen pixel):
// dU[b][qy][qx][c] = sum over points n (ascending) and taps (ascending) whose upsampled position interpolates from (qy, qx) of
// weight * dpatch[b][n][tap][c] -- a gather, so no atomics.  Three launches: decode every point's pixel and the range of
// half-resolution rows / columns its patch can touch; per half-resolution row the ordered list of points that touch it; then a
// thread per (pixel, 4 channels) walks its row's list (a few dozen points instead of all N).  All buckets in one grid (tab = the
// half-resolution level; rows / columns beyond a bucket's map exit): row lists and counts are laid out with the LARGEST map height hmax
// per frame.
// tabo[b][n] = {py | px << 16, rlo | rhi << 16, clo | chi << 16, 0}: the chosen pixel of point n and the range of half-resolution rows /
// columns its 3 x 3 patch of upsampled positions interpolates from
__global__ __launch_bounds__(TB) void up3_decode_multi_kernel(const int64_t *__restrict__ choose, int4 *__restrict__ tabo, int frames, int N, const BTab tab) {
  GRID_STRIDE(i, (long)frames * N) {          // (choose / tabo start at the table's first frame)
    const int g = tab_of_frame(tab, tab.b0[0] + (int)(i / N));
    const int h = tab.H[g], wd = tab.W[g];
    const int OH = 2 * h, OW = 2 * wd, HW = OH * OW;
    long pix = choose[i];
    pix = pix < 0 ? 0 : (pix >= HW ? HW - 1 : pix);
    const int py = (int)(pix / OW), px = (int)(pix % OW);
    int i0, i1, rlo, rhi, clo, chi;
    float l0, l1;
    bil_src(max(py - 1, 0), h, OH, 1, rlo, i1, l0, l1);
    bil_src(min(py + 1, OH - 1), h, OH, 1, i0, rhi, l0, l1);
    bil_src(max(px - 1, 0), wd, OW, 1, clo, i1, l0, l1);
    bil_src(min(px + 1, OW - 1), wd, OW, 1, i0, chi, l0, l1);
    tabo[i] = make_int4(py | (px << 16), rlo | (rhi << 16), clo | (chi << 16), 0);
  }
}
// rows[b][qy][...] = the points (ascending n) whose patch touches half-resolution row qy, cnt[b][qy] their number: a workgroup per row
// scans the table once, 256 points per round, and compacts the hits in order (wave ballots + a scan over the 4 waves)
__global__ __launch_bounds__(TB) void up3_rowlist_multi_kernel(const int4 *__restrict__ tabi, int *__restrict__ rows, int *__restrict__ cnt, int hmax, int N,
                                                               const BTab tab) {
  __shared__ int s_w[4];
  const int b = blockIdx.y, qy = blockIdx.x;          // b: frame relative to the table's first (tabi / rows / cnt start there)
  if (qy >= tab.H[tab_of_frame(tab, tab.b0[0] + b)]) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int *out = rows + ((size_t)b * hmax + qy) * N;
  int base = 0;
  for (int n0 = 0; n0 < N; n0 += TB) {
    const int n = n0 + threadIdx.x;
    bool hit = false;
    if (n < N) {
      const int4 e = tabi[(size_t)b * N + n];
      hit = qy >= (e.y & 0xffff) && qy <= (e.y >> 16);
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_w[wave] = __popcll(m);
    __syncthreads();
    int before = base;
    for (int w2 = 0; w2 < wave; ++w2) before += s_w[w2];
    if (hit) out[before + __popcll(m & ((1ull << lane) - 1ull))] = n;
    base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) cnt[b * hmax + qy] = base;
}
__global__ __launch_bounds__(TB) void up3_patch_bwd_multi_kernel(const float *__restrict__ dpatch, const int4 *__restrict__ tabi, const int *__restrict__ rows,
                                                                 const int *__restrict__ cnt, float *__restrict__ dU, int hmax, int N, int Npad, const BTab tab) {
  const int b = blockIdx.z, qy = blockIdx.y;          // b: frame relative to the table's first (dpatch / tabi / rows / cnt start there)
  const int g = tab_of_frame(tab, tab.b0[0] + b);
  const int h = tab.H[g], wd = tab.W[g];
  const int OH = 2 * h, OW = 2 * wd;
  const int c4 = threadIdx.x & 15, qx = blockIdx.x * (TB / 16) + (threadIdx.x >> 4);
  if (qy >= h || qx >= wd) return;
  const int *list = rows + ((size_t)b * hmax + qy) * N;
  const int count = cnt[b * hmax + qy];
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < count; ++i) {
    const int j = list[i];
    const int4 e4 = tabi[(size_t)b * N + j];
    if (qx < (e4.z & 0xffff) || qx > (e4.z >> 16)) continue;
    const float *row = dpatch + ((size_t)b * Npad + j) * 576 + c4 * 4;
    const int py = e4.x & 0xffff, px = e4.x >> 16;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int uy = py + dy - 1;
      if ((unsigned)uy >= (unsigned)OH) continue;
      int y0, y1;
      float wy0, wy1;
      bil_src(uy, h, OH, 1, y0, y1, wy0, wy1);
      if (y0 != qy && y1 != qy) continue;
      const float wy = (y0 == qy ? wy0 : 0.f) + (y1 == qy ? wy1 : 0.f);
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int ux = px + dx - 1;
        if ((unsigned)ux >= (unsigned)OW) continue;
        int x0, x1;
        float wx0, wx1;
        bil_src(ux, wd, OW, 1, x0, x1, wx0, wx1);
        if (x0 != qx && x1 != qx) continue;
        const float wx = (x0 == qx ? wx0 : 0.f) + (x1 == qx ? wx1 : 0.f);
        const f32x4 v = *reinterpret_cast<const f32x4 *>(row + (dy * 3 + dx) * 64);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += (wy * wx) * v[e];
      }
    }
  }
  *reinterpret_cast<f32x4 *>(dU + (tab.row0[g] + ((long)(tab.b0[0] + b - tab.b0[g]) * h + qy) * wd + qx) * 64 + c4 * 4) = acc;
}

// Conv1d(3, 64, 1) on the cloud (lib/network.py:54): partial sums of dW [64][3], db [64] over a chunk of 64 points;
// g = the masked gradient of its output, a [B*Npad][64] view.  part[chunk][64][4] = (dW_x, dW_y, dW_z, db)
__global__ __launch_bounds__(64) void cloud_conv1_bwd_kernel(const float *__restrict__ g, int g_ld, const float *__restrict__ cloud, int B, int N,
                                                             int Npad, float *__restrict__ part) {
  const int chunks = (N + 63) / 64;
  const int b = blockIdx.x / chunks, n0 = (blockIdx.x % chunks) * 64, n1 = min(N, n0 + 64);
  const int c = threadIdx.x;
  float ax = 0.f, ay = 0.f, az = 0.f, ab = 0.f;
  for (int n = n0; n < n1; ++n) {
    const float gv = g[((size_t)b * Npad + n) * g_ld + c];
    const float *p = cloud + ((size_t)b * N + n) * 3;
    ax += gv * p[0]; ay += gv * p[1]; az += gv * p[2]; ab += gv;
  }
  float *o = part + ((size_t)blockIdx.x * 64 + c) * 4;
  o[0] = ax; o[1] = ay; o[2] = az; o[3] = ab;
}
__global__ __launch_bounds__(64) void cloud_conv1_bwd_finish_kernel(const float *__restrict__ part, int count, float *__restrict__ dw, float *__restrict__ db) {
  const int c = threadIdx.x;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
  for (int i = 0; i < count; ++i) {        // (eight loads in flight; the additions stay in order)
    const f32x4 v = *reinterpret_cast<const f32x4 *>(part + ((size_t)i * 64 + c) * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] += v[e];
  }
  dw[c * 3 + 0] += a[0]; dw[c * 3 + 1] += a[1]; dw[c * 3 + 2] += a[2];
  db[c] += a[3];
}

// AvgPool1d(N) adjoint + ReLU mask of conv6's output: g6[r][c] = (n < N && x6[r][c] > 0) ? dap[b][c] / N : 0
__global__ __launch_bounds__(TB) void mask_bcast_kernel(const float *__restrict__ x6, const float *__restrict__ dap, float *__restrict__ g6, int B, int N,
                                                        int Npad, int C4) {
  const float inv = 1.f / (float)N;
  GRID_STRIDE(i, (long)B * Npad * C4) {
    const int c = (int)(i % C4);
    const long r = i / C4;
    const int b = (int)(r / Npad), n = (int)(r - (long)b * Npad);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (n < N) {
      const f32x4 x = reinterpret_cast<const f32x4 *>(x6)[i], d = reinterpret_cast<const f32x4 *>(dap)[(long)b * C4 + c];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = x[e] > 0.f ? d[e] * inv : 0.f;
    }
    reinterpret_cast<f32x4 *>(g6)[i] = o;
  }
}

// s[b][c] = sum over the Npad rows of object b of g[.][c]: 32 columns x 8 row lanes per workgroup, rows in ascending order per lane
__global__ __launch_bounds__(256) void colsum_obj_kernel(const float *__restrict__ g, int g_ld, float *__restrict__ s, int Npad, int C, long rows_total,
                                                         int accumulate = 0) {
  __shared__ float s_p[8][32];
  const int col = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + col, b = blockIdx.y;
  float a = 0.f;
  if (c < C) {
    const long left = rows_total - (long)b * Npad;
    const int rmax = (int)(left < Npad ? left : Npad);
#pragma unroll 8
    for (int r = rl; r < rmax; r += 8) a += g[((size_t)b * Npad + r) * g_ld + c];      // (loads ahead, the additions in row order)
  }
  s_p[rl][col] = a;
  __syncthreads();
  if (rl == 0 && c < C) {
#pragma unroll
    for (int l = 1; l < 8; ++l) a += s_p[l][col];
    s[(size_t)b * C + c] = accumulate ? s[(size_t)b * C + c] + a : a;
  }
}

// global-feature half of head layer 1 (the 1024 broadcast channels folded into a per-object bias, engine.hip posenet_points):
//   gbias[b][o] = Wg[o] . ap[b] + bias[o]   =>   dbias[o] += sum_b s[b][o],  dWg[o][j] += sum_b s[b][o] ap[b][j],  dap[b][j] = sum_o Wg[o][j] s[b][o]
// (the last one is a [B x 1920] x [1920 x 1024] product: the GEMM kernel on the cached transpose of Wg)
// with s[b][o] = the column sums over object b's points of the masked gradient of head layer 1's output
__global__ __launch_bounds__(TB) void head1_global_wgrad_kernel(const float *__restrict__ s, const float *__restrict__ ap, float *__restrict__ dWg,
                                                                float *__restrict__ dbias, int B, int O, int J4) {
  GRID_STRIDE(i, (long)O * J4) {
    const int j = (int)(i % J4);
    const int o = (int)(i / J4);
    f32x4 acc = reinterpret_cast<const f32x4 *>(dWg)[i];
    float sb = 0.f;
    for (int b = 0; b < B; ++b) {
      const float sv = s[(size_t)b * O + o];
      const f32x4 a = reinterpret_cast<const f32x4 *>(ap)[(size_t)b * J4 + j];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += sv * a[e];
      sb += sv;
    }
    reinterpret_cast<f32x4 *>(dWg)[i] = acc;
    if (j == 0) dbias[o] += sb;
  }
}
// last head layer for the frame's object only (layers.hip head_final): outputs j = 0..3 quaternion, 4..6 translation, 7 confidence
// (sigmoid).  dz[b][n][j] = upstream gradient of the pre-sigmoid outputs; dh3 = dz . W rows; partial dW rows over chunks of 128 points.
__global__ __launch_bounds__(TB) void head_final_bwd_kernel(const float *__restrict__ d_r, const float *__restrict__ d_t, const float *__restrict__ d_c,
                                                            const float *__restrict__ out_c, const float *__restrict__ w_r, const float *__restrict__ w_t,
                                                            const float *__restrict__ w_c, const int64_t *__restrict__ obj, int num_obj,
                                                            float *__restrict__ dh3, float *__restrict__ dz, int B, int N, int Npad) {
  GRID_STRIDE(i, (long)B * Npad * 96) {          // thread = (row, one float4 of the 384 feature columns)
    const int k4 = (int)(i % 96);
    const long r = i / 96;
    const int b = (int)(r / Npad), n = (int)(r - (long)b * Npad);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (n < N) {
      long ob = obj[b];
      ob = ob < 0 ? 0 : (ob >= num_obj ? num_obj - 1 : ob);
      const size_t p = (size_t)b * N + n;
      const int tower = k4 / 32, k = (k4 % 32) * 4;
      if (tower == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float gz = d_r[p * 4 + j];
          const f32x4 wv = *reinterpret_cast<const f32x4 *>(w_r + (ob * 4 + j) * 128 + k);
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] += gz * wv[e];
          if (k4 == 0) dz[p * 8 + j] = gz;
        }
      } else if (tower == 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const float gz = d_t[p * 3 + j];
          const f32x4 wv = *reinterpret_cast<const f32x4 *>(w_t + (ob * 3 + j) * 128 + k);
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] += gz * wv[e];
          if (k4 == 32) dz[p * 8 + 4 + j] = gz;
        }
      } else {
        const float cv = out_c[p];
        const float gz = d_c[p] * cv * (1.f - cv);
        const f32x4 wv = *reinterpret_cast<const f32x4 *>(w_c + ob * 128 + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = gz * wv[e];
        if (k4 == 64) dz[p * 8 + 7] = gz;
      }
    }
    *reinterpret_cast<f32x4 *>(dh3 + r * 384 + k4 * 4) = o;
  }
}
// part[b][chunk][j][k] = sum over the chunk's points of dz[n][j] * h3[n][tower(j)*128 + k]; block = (chunk, b), thread = (j pair, k)
__global__ __launch_bounds__(TB) void head_final_wgrad_kernel(const float *__restrict__ dz, const float *__restrict__ h3, float *__restrict__ part,
                                                              float *__restrict__ zpart, int N, int Npad, int chunks) {
  const int b = blockIdx.y, ch = blockIdx.x, n0 = ch * 128, n1 = min(N, n0 + 128);
  const int k = threadIdx.x & 127, jh = threadIdx.x >> 7;       // jh 0: outputs 0..3 (r), 1: outputs 4..7 (t, c)
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  for (int n = n0; n < n1; ++n) {
    const float *z = dz + ((size_t)b * N + n) * 8 + jh * 4;
    const float *hrow = h3 + ((size_t)b * Npad + n) * 384;
    const float hr = hrow[(jh == 0 ? 0 : 128) + k], hc = hrow[256 + k];
    a[0] += z[0] * hr; a[1] += z[1] * hr; a[2] += z[2] * hr;
    a[3] += z[3] * (jh == 0 ? hr : hc);
  }
  float *o = part + (((size_t)b * chunks + ch) * 8 + jh * 4) * 128 + k;
  o[0] = a[0]; o[128] = a[1]; o[256] = a[2]; o[384] = a[3];
  if (k == 0) {                       // the chunk's sums of dz (bias gradient)
    float zs[4] = {0.f, 0.f, 0.f, 0.f};
    for (int n = n0; n < n1; ++n) {
      const float *z = dz + ((size_t)b * N + n) * 8 + jh * 4;
      zs[0] += z[0]; zs[1] += z[1]; zs[2] += z[2]; zs[3] += z[3];
    }
    float *zo = zpart + ((size_t)b * chunks + ch) * 8 + jh * 4;
    zo[0] = zs[0]; zo[1] = zs[1]; zo[2] = zs[2]; zo[3] = zs[3];
  }
}
// thread = (j, k): frames in ascending order add their chunks (ascending) into the rows of their object; db from dz directly
__global__ __launch_bounds__(TB) void head_final_wgrad_finish_kernel(const float *__restrict__ part, const float *__restrict__ zpart,
                                                                     const int64_t *__restrict__ obj, int num_obj, float *__restrict__ dw_r,
                                                                     float *__restrict__ db_r, float *__restrict__ dw_t, float *__restrict__ db_t,
                                                                     float *__restrict__ dw_c, float *__restrict__ db_c, int B, int N, int chunks) {
  const int i = blockIdx.x * TB + threadIdx.x;
  if (i >= 8 * 128) return;
  const int j = i >> 7, k = i & 127;
  for (int b0 = 0; b0 < B; b0 += 4) {          // four frames' partial sums are gathered first (their loads in flight together), then added in frame order
    float a4[4] = {0.f, 0.f, 0.f, 0.f}, s4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int b = b0 + u;
      if (b >= B) break;
#pragma unroll 8
      for (int ch = 0; ch < chunks; ++ch) a4[u] += part[(((size_t)b * chunks + ch) * 8 + j) * 128 + k];
      if (k == 0) {
#pragma unroll 8
        for (int ch = 0; ch < chunks; ++ch) s4[u] += zpart[((size_t)b * chunks + ch) * 8 + j];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int b = b0 + u;
      if (b >= B) break;
      long ob = obj[b];
      ob = ob < 0 ? 0 : (ob >= num_obj ? num_obj - 1 : ob);
      float *dst = j < 4 ? dw_r + (ob * 4 + j) * 128 : j < 7 ? dw_t + (ob * 3 + (j - 4)) * 128 : dw_c + ob * 128;
      dst[k] += a4[u];
      if (k == 0) {
        float *bd = j < 4 ? db_r + ob * 4 + j : j < 7 ? db_t + ob * 3 + (j - 4) : db_c + ob;
        *bd += s4[u];
      }
    }
  }
}

// refiner tail (lib/network.py:199-204): out_r [B][4], out_t [B][3] = conv3_r / conv3_t rows of the frame's object on f2 [B][256]
__global__ __launch_bounds__(64) void refiner_tail_fwd_kernel(const float *__restrict__ f2, const float *__restrict__ w_r, const float *__restrict__ b_r,
                                                              const float *__restrict__ w_t, const float *__restrict__ b_t, const int64_t *__restrict__ obj,
                                                              int num_obj, float *__restrict__ out_r, float *__restrict__ out_t, int B) {
  const int b = blockIdx.x, j = threadIdx.x;
  if (b >= B || j >= 7) return;
  long ob = obj[b];
  ob = ob < 0 ? 0 : (ob >= num_obj ? num_obj - 1 : ob);
  const float *w = j < 4 ? w_r + (ob * 4 + j) * 128 : w_t + (ob * 3 + (j - 4)) * 128;
  const float *x = f2 + (size_t)b * 256 + (j < 4 ? 0 : 128);
  float a = 0.f;
  for (int k = 0; k < 128; ++k) a += x[k] * w[k];
  if (j < 4) out_r[b * 4 + j] = a + b_r[ob * 4 + j];
  else out_t[b * 3 + (j - 4)] = a + b_t[ob * 3 + (j - 4)];
}
// one workgroup: frames in ascending order; df2[b][tower*128 + k] = sum_j dz[j] W[j][k]; dW rows += dz[j] f2[k]; db += dz
__global__ __launch_bounds__(128) void refiner_tail_bwd_kernel(const float *__restrict__ d_r, const float *__restrict__ d_t, const float *__restrict__ f2,
                                                               const float *__restrict__ w_r, const float *__restrict__ w_t, const int64_t *__restrict__ obj,
                                                               int num_obj, float *__restrict__ df2, float *__restrict__ dw_r, float *__restrict__ db_r,
                                                               float *__restrict__ dw_t, float *__restrict__ db_t, int B) {
  const int k = threadIdx.x;
  for (int b = 0; b < B; ++b) {
    long ob = obj[b];
    ob = ob < 0 ? 0 : (ob >= num_obj ? num_obj - 1 : ob);
    float ar = 0.f, at = 0.f;
    const float xr = f2[(size_t)b * 256 + k], xt = f2[(size_t)b * 256 + 128 + k];
    for (int j = 0; j < 4; ++j) {
      const float gz = d_r[b * 4 + j];
      ar += gz * w_r[(ob * 4 + j) * 128 + k];
      dw_r[(ob * 4 + j) * 128 + k] += gz * xr;
      if (k == 0) db_r[ob * 4 + j] += gz;
    }
    for (int j = 0; j < 3; ++j) {
      const float gz = d_t[b * 3 + j];
      at += gz * w_t[(ob * 3 + j) * 128 + k];
      dw_t[(ob * 3 + j) * 128 + k] += gz * xt;
      if (k == 0) db_t[ob * 3 + j] += gz;
    }
    df2[(size_t)b * 256 + k] = ar;
    df2[(size_t)b * 256 + 128 + k] = at;
    __syncthreads();
  }
}

// Every flip of a trainer in ONE launch: wf[z][c][tap'][n] = P[z][n][tap][c], tap' = the tap mirrored through the kernel centre (what the
// data gradient convolves with).  32 x 32 (output channel, input channel) tiles through LDS: reads run along c (the source's fastest axis),
// writes along n (the destination's) -- an element-wise form reads with a stride of T * I floats (167 us per optimizer step for PoseNet's
// 86 MB; this one is bound by the copy).  Tile list: `tbegin` = first tile of the segment in the launch's tile space; a tile = (z, tap,
// n block, c block).
struct FlipTile { long off; int tbegin; int O, T, I, KH, KW, Z, nb_n, nb_c; };
__global__ __launch_bounds__(256) void flip_tiles_kernel(const float *__restrict__ P, float *__restrict__ wf, const FlipTile *__restrict__ segs, int nseg) {
  __shared__ float s_t[32][33];
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {                               // last segment whose tbegin <= blockIdx.x
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].tbegin <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const FlipTile sg = segs[lo];
  int q = (int)blockIdx.x - sg.tbegin;
  const int cb = q % sg.nb_c; q /= sg.nb_c;
  const int nb = q % sg.nb_n; q /= sg.nb_n;
  const int t = q % sg.T, z = q / sg.T;
  const int ky = t / sg.KW, kx = t - ky * sg.KW;
  const int tf = (sg.KH - 1 - ky) * sg.KW + (sg.KW - 1 - kx);
  const long per = (long)sg.O * sg.T * sg.I;
  const float *src = P + sg.off + z * per;
  float *dst = wf + sg.off + z * per;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 32 x 8
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = nb * 32 + ty + r * 8, c = cb * 32 + tx;
    s_t[ty + r * 8][tx] = n < sg.O && c < sg.I ? src[((size_t)n * sg.T + tf) * sg.I + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = cb * 32 + ty + r * 8, n = nb * 32 + tx;
    if (n < sg.O && c < sg.I) dst[((size_t)c * sg.T + t) * sg.O + n] = s_t[tx][ty + r * 8];
  }
}

// layout conversion between the reference's state-dict tensors and the flat kernel layout
//   mode 0: OIHW [O][I][T] <-> O(T)Ipad          mode 1: OIHW (T = 9) <-> tap-major [9][O][I]          (dir 0: pack, 1: unpack)
__global__ __launch_bounds__(TB) void relayout_kernel(const float *__restrict__ src, float *__restrict__ dst, int O, int I, int T, int Ipad, int mode,
                                                      int dir) {
  GRID_STRIDE(i, (long)O * T * Ipad) {
    const int c = (int)(i % Ipad);
    const long r = i / Ipad;
    const int t = (int)(r % T);
    const long o = r / T;
    const size_t ref = ((size_t)o * I + c) * T + t;
    const size_t ker = mode == 0 ? (size_t)i : ((size_t)t * O + o) * I + c;
    if (dir == 0) dst[ker] = c < I ? src[ref] : 0.f;
    else if (c < I) dst[ref] = src[ker];
  }
}
__global__ __launch_bounds__(TB) void copy2d_kernel(const float *__restrict__ src, long s_ld, float *__restrict__ dst, long d_ld, long rows, long width) {
  GRID_STRIDE(i, rows * width) {
    const long r = i / width, c = i - r * width;
    dst[r * d_ld + c] = src[r * s_ld + c];
  }
}

}  // namespace
}  // namespace df
