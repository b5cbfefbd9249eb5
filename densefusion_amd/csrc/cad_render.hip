// Point-cloud renderer for customCAD training sets: a coloured CAD cloud -> Unity-format colour, 16-bit depth and mask frames (the job of
// datasets/customCAD/cad_to_dataset.py:137-243 and mask_generator.py:20-28 of the reference, for the frames datasets/customCAD/dataset.py
// reads).  The contract -- every fp64 operation and its order -- is the comment of df_cad_render in include/dfusion.h; tests/cad_render_np.py
// restates it in numpy and the outputs are compared bit for bit.  Built with -ffp-contract=off: no fused multiply-add anywhere.
//
// Four steps on the caller's stream: the keys are set to all-ones; splat_kernel takes atomicMin of (code << 32 | point index) over every
// footprint pixel (grid = point blocks x frames); resolve_kernel turns keys into depth / colour and reduces count and box per wave before
// its integer atomics, like frame_stats_kernel of cad.hip (finish_kernel then decodes the F rows in place); mask_kernel fills the mask.
// The pose record, the hole rule, the horizon and the host side of the entry point are those of cad_frame.h, shared with the mesh calls.
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
  const Pose M = load_pose(pose + (size_t)f * 12);
  unsigned long long *kf = keys + (size_t)f * IH * IW;
  int reached = 0;
  for (long i = (long)blockIdx.x * RB + threadIdx.x; i < P; i += (long)gridDim.x * RB) {
    if (vertex_cut(points, i, holes, blockIdx.y * K, K)) continue;            // 1. holes
    const double mx = (double)points[i * 3], my = (double)points[i * 3 + 1], mz = (double)points[i * 3 + 2];
    const double sx = mx * model_scale, sy = my * model_scale, sz = mz * model_scale;      // 2. camera space
    double X[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) X[j] = ((M.R[j][0] * sx + M.R[j][1] * sy) + M.R[j][2] * sz) + M.t[j];
    if (normals) {                                                            // 3. facing test on the point's own view ray
      const double nx = (double)normals[i * 3], ny = (double)normals[i * 3 + 1], nz = (double)normals[i * 3 + 2];
      double n[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) n[j] = (M.R[j][0] * nx + M.R[j][1] * ny) + M.R[j][2] * nz;
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
      write_horizon(df + p, px);
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
  if (int e = check_hole_args("cad_render", hole_idx, hole_r, K)) return e;
  if (P <= 0 || !sizes_ok(F, IH, IW)) return set_error(DF_ERR_ARG, "cad_render: bad sizes");
  if (splat < 0 || splat > 3) return set_error(DF_ERR_ARG, "cad_render: splat %d outside 0..3", splat);
  if (mask_mode != 0 && mask_mode != 1) return set_error(DF_ERR_ARG, "cad_render: mask_mode %d is neither 0 (box) nor 1 (pixels)", mask_mode);
  if (int e = check_scratch_and_proj("cad_render", scratch, scratch_bytes, df_cad_render_scratch_bytes(F, IH, IW), proj)) return e;
  if (int e = check_hole_indices("cad_render", hole_idx, F, K, 'P', P)) return e;
  hipStream_t st = to_stream(stream);
  const Camera cam = make_camera(proj);
  const long npix = (long)IH * IW;
  if (!clear_frames(scratch, F, npix, stats_out, F, st)) return check_launch("cad_render (clear)");
  unsigned long long *keys = static_cast<unsigned long long *>(scratch);
  const int pb = grid_blocks(P, SPLAT_MAX_BLOCKS), xb = grid_blocks(npix, RESOLVE_MAX_BLOCKS);
  for_hole_batches(hole_idx, hole_r, K, F, [&](int f0, int nf, const Holes &holes) {
    hipLaunchKernelGGL(splat_kernel, dim3(pb, nf), dim3(RB), 0, st, points, normals, P, pose, model_scale, holes, K, f0, cam, IH, IW, splat,
                       keys, stats_out);
  });
  hipLaunchKernelGGL(resolve_kernel, dim3(xb, F), dim3(RB), 0, st, keys, colors, IH, IW, rgb_out, depth_out, stats_out);
  hipLaunchKernelGGL(finish_kernel, dim3(cdiv(F, RB)), dim3(RB), 0, st, F, IH, IW, stats_out);
  hipLaunchKernelGGL(mask_kernel, dim3(xb, F), dim3(RB), 0, st, depth_out, stats_out, IH, IW, mask_mode, mask_out);
  return check_launch("cad_render");
}
