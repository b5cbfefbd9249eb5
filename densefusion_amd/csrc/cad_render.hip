// Point-cloud renderer for customCAD training sets: a coloured CAD cloud -> Unity-format colour, 16-bit depth and mask frames (the job of
// datasets/customCAD/cad_to_dataset.py:137-243 and mask_generator.py:20-28 of the reference, for the frames datasets/customCAD/dataset.py
// reads).  The contract -- every fp64 operation and its order -- is the comment of df_cad_render in include/dfusion.h; tests/cad_render_np.py
// restates it in numpy and the outputs are compared bit for bit.  Built with -ffp-contract=off: no fused multiply-add anywhere.
//
// Four steps on the caller's stream: the keys are set to all-ones; splat_kernel takes atomicMin of (code << 32 | point index) over every
// footprint pixel (grid = point blocks x frames); resolve_kernel turns keys into depth / colour and reduces count and box per wave before
// its integer atomics, like frame_stats_kernel of cad.hip (finish_kernel then decodes the F rows in place); mask_kernel fills the mask.
#include "cad_frame.h"

namespace df {
namespace {

constexpr int SPLAT_MAX_BLOCKS = 256;   // point blocks per frame: the threads stride over the rest

// stats[f][1] counts the points that reached the z-buffer (the row while the blocks reduce: reduce_frame_stats, cad_frame.h)
__global__ __launch_bounds__(RB) void splat_kernel(const float *__restrict__ points, const float *__restrict__ normals, int P,
                                                   const double *__restrict__ pose, double model_scale, Holes holes, int K, int f0,
                                                   Camera cam, int IH, int IW, int splat, unsigned long long *__restrict__ keys,
                                                   int *__restrict__ stats) {
  const int f = f0 + blockIdx.y;
  const double *T = pose + (size_t)f * 12;
  double R[3][3], t[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    R[j][0] = T[j * 4]; R[j][1] = T[j * 4 + 1]; R[j][2] = T[j * 4 + 2]; t[j] = T[j * 4 + 3];
  }
  unsigned long long *kf = keys + (size_t)f * IH * IW;
  int reached = 0;
  for (long i = (long)blockIdx.x * RB + threadIdx.x; i < P; i += (long)gridDim.x * RB) {
    const double mx = (double)points[i * 3], my = (double)points[i * 3 + 1], mz = (double)points[i * 3 + 2];
    bool cut = false;                                                         // 1. holes
    for (int k = 0; k < K; ++k) {
      const int h = holes.idx[blockIdx.y * K + k];
      if (h < 0) continue;
      const double cx = (double)points[(size_t)h * 3], cy = (double)points[(size_t)h * 3 + 1], cz = (double)points[(size_t)h * 3 + 2];
      const double r = holes.r[blockIdx.y * K + k];
      const double dx = mx - cx, dy = my - cy, dz = mz - cz;
      cut |= ((dx * dx + dy * dy) + dz * dz) <= r * r;
    }
    if (cut) continue;
    const double sx = mx * model_scale, sy = my * model_scale, sz = mz * model_scale;      // 2. camera space
    double X[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) X[j] = ((R[j][0] * sx + R[j][1] * sy) + R[j][2] * sz) + t[j];
    if (normals) {                                                            // 3. facing test on the point's own view ray
      const double nx = (double)normals[i * 3], ny = (double)normals[i * 3 + 1], nz = (double)normals[i * 3 + 2];
      double n[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) n[j] = (R[j][0] * nx + R[j][1] * ny) + R[j][2] * nz;
      if (!(((n[0] * (-X[0]) + n[1] * (-X[1])) + n[2] * (-X[2])) > 0.0)) continue;
    }
    const double c0 = ((cam.p0[0] * X[0] + cam.p0[1] * X[1]) + cam.p0[2] * X[2]) + cam.p0[3];      // 4. clip space
    const double c1 = ((cam.p1[0] * X[0] + cam.p1[1] * X[1]) + cam.p1[2] * X[2]) + cam.p1[3];
    const double c3 = ((cam.p3[0] * X[0] + cam.p3[1] * X[1]) + cam.p3[2] * X[2]) + cam.p3[3];
    if (!(c3 > 0.0)) continue;
    const double ndc_x = c0 / c3, ndc_y = c1 / c3;
    const double code = rint(65534.0 * ((1.0 + cam.p22) + cam.p23 / X[2]));  // 5. Unity's 16-bit depth, ties to even
    if (!(code >= 0.0 && code <= 65534.0)) continue;
    const double colf = floor(((ndc_x + 1.0) * (double)IW) * 0.5 + 0.5);      // 6. nearest node of the loader's ray grid
    const double rowf = floor(((1.0 - ndc_y) * (double)IH) * 0.5 + 0.5);
    // compared as doubles, before any conversion: a footprint that misses the frame (or a NaN) never becomes an integer
    if (!(colf >= (double)-splat && colf <= (double)(IW - 1 + splat) && rowf >= (double)-splat && rowf <= (double)(IH - 1 + splat))) continue;
    const int col = (int)colf, row = (int)rowf;
    const unsigned long long key = ((unsigned long long)(unsigned)(int)code << 32) | (unsigned)i;
    const int r0 = max(row - splat, 0), r1 = min(row + splat, IH - 1), q0 = max(col - splat, 0), q1 = min(col + splat, IW - 1);
    for (int r = r0; r <= r1; ++r)
      for (int q = q0; q <= q1; ++q) {                                        // 7. nearest code wins, then the lowest index
        unsigned long long *dst = kf + (size_t)r * IW + q;
        if (*dst > key) atomicMin(dst, key);                                  // keys only decrease: a stale read costs one atomic, no more
      }
    ++reached;                                                                // r0 <= r1 and q0 <= q1 hold after the test above
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) reached += __shfl_down(reached, off, 64);
  if ((threadIdx.x & 63) == 0 && reached) atomicAdd(&stats[(size_t)f * 6 + 1], reached);
}

__global__ __launch_bounds__(RB) void resolve_kernel(const unsigned long long *__restrict__ keys, const unsigned char *__restrict__ colors,
                                                     int IH, int IW, unsigned char *__restrict__ rgb, unsigned short *__restrict__ depth,
                                                     int *__restrict__ stats) {
  const int f = blockIdx.y;
  const int npix = IH * IW;
  const unsigned long long *kf = keys + (size_t)f * npix;
  unsigned char *cf = rgb + (size_t)f * npix * 3;
  unsigned short *df = depth + (size_t)f * npix;
  int cnt = 0, a_r = 0, b_r = 0, a_c = 0, b_c = 0;
  for (int p = blockIdx.x * RB + threadIdx.x; p < npix; p += gridDim.x * RB) {
    const unsigned long long key = kf[p];
    unsigned char *px = cf + (size_t)p * 3;
    if (key == NO_KEY) {
      df[p] = 65535;                                                          // the horizon: above every code
      px[0] = 130; px[1] = 130; px[2] = 130;
      continue;
    }
    const unsigned char *c = colors + (size_t)(unsigned)(key & 0xffffffffu) * 3;
    df[p] = (unsigned short)(key >> 32);
    px[0] = c[0]; px[1] = c[1]; px[2] = c[2];
    const int r = p / IW, q = p - r * IW;
    ++cnt;
    a_r = max(a_r, IH - r); b_r = max(b_r, r + 1);
    a_c = max(a_c, IW - q); b_c = max(b_c, q + 1);
  }
  reduce_frame_stats(cnt, a_r, b_r, a_c, b_c, stats + (size_t)f * 6);
}

}  // namespace
}  // namespace df

using namespace df;

extern "C" size_t df_cad_render_scratch_bytes(int F, int IH, int IW) {
  return sizes_ok(F, IH, IW) ? (size_t)F * IH * IW * sizeof(unsigned long long) : 0;
}

extern "C" int df_cad_render(const float *points, const float *normals, const unsigned char *colors, int P, const double *pose,
                             double model_scale, const int *hole_idx, const double *hole_r, int K, const double *proj, int F, int IH, int IW,
                             int splat, int mask_mode, unsigned char *rgb_out, unsigned short *depth_out, unsigned short *mask_out,
                             int *stats_out, void *scratch, size_t scratch_bytes, df_stream_t stream) {
  if (!points || !colors || !pose || !proj || !rgb_out || !depth_out || !mask_out || !stats_out || !scratch)
    return set_error(DF_ERR_ARG, "cad_render: null pointer");
  if (K > 0 && (!hole_idx || !hole_r)) return set_error(DF_ERR_ARG, "cad_render: null pointer (K holes need hole_idx and hole_r)");
  if (K < 0 || K > MAX_HOLES) return set_error(DF_ERR_ARG, "cad_render: K = %d holes per frame outside 0..%d", K, MAX_HOLES);
  if (P <= 0 || !sizes_ok(F, IH, IW)) return set_error(DF_ERR_ARG, "cad_render: bad sizes");
  if (splat < 0 || splat > 3) return set_error(DF_ERR_ARG, "cad_render: splat %d outside 0..3", splat);
  if (mask_mode != 0 && mask_mode != 1) return set_error(DF_ERR_ARG, "cad_render: mask_mode %d is neither 0 (box) nor 1 (pixels)", mask_mode);
  if (scratch_bytes < df_cad_render_scratch_bytes(F, IH, IW) || (reinterpret_cast<uintptr_t>(scratch) & 7u))
    return set_error(DF_ERR_ARG, "cad_render: scratch too small or not 8-byte aligned");
  if (!proj_form_ok(proj))
    return set_error(DF_ERR_ARG, "cad_render: the projection matrix needs rows 2 = (0, 0, p22, p23) and 3 = (0, 0, -1, 0)");
  for (long j = 0; j < (long)F * K; ++j)
    if (hole_idx[j] >= P) return set_error(DF_ERR_ARG, "cad_render: hole index %d of frame %ld is not below P = %d", hole_idx[j], j / K, P);
  hipStream_t st = to_stream(stream);
  const Camera cam = make_camera(proj);
  const long npix = (long)IH * IW;
  if (hipMemsetAsync(scratch, 0xff, (size_t)F * npix * sizeof(unsigned long long), st) != hipSuccess ||
      hipMemsetAsync(stats_out, 0, sizeof(int) * 6 * F, st) != hipSuccess)
    return check_launch("cad_render (clear)");
  unsigned long long *keys = static_cast<unsigned long long *>(scratch);
  const int pb = cdiv(P, RB) < SPLAT_MAX_BLOCKS ? cdiv(P, RB) : SPLAT_MAX_BLOCKS;
  const int per_launch = K > 0 ? MAX_HOLES / K : F;                        // frames per splat launch: their holes fit one Holes
  for (int f0 = 0; f0 < F; f0 += per_launch) {
    const int nf = F - f0 < per_launch ? F - f0 : per_launch;
    const Holes holes = make_holes(hole_idx, hole_r, K, f0, nf);
    hipLaunchKernelGGL(splat_kernel, dim3(pb, nf), dim3(RB), 0, st, points, normals, P, pose, model_scale, holes, K, f0, cam, IH, IW, splat,
                       keys, stats_out);
  }
  const int xb = cdiv(npix, RB) < RESOLVE_MAX_BLOCKS ? cdiv(npix, RB) : RESOLVE_MAX_BLOCKS;
  hipLaunchKernelGGL(resolve_kernel, dim3(xb, F), dim3(RB), 0, st, keys, colors, IH, IW, rgb_out, depth_out, stats_out);
  hipLaunchKernelGGL(finish_kernel, dim3(cdiv(F, RB)), dim3(RB), 0, st, F, IH, IW, stats_out);
  hipLaunchKernelGGL(mask_kernel, dim3(xb, F), dim3(RB), 0, st, depth_out, stats_out, IH, IW, mask_mode, mask_out);
  return check_launch("cad_render");
}
