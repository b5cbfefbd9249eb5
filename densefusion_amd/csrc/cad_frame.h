// What the customCAD renderers share (cad_render.hip: points; cad_raster.hip: triangles; cad_scene.hip: several meshes with occlusion):
// the z-buffer key, the camera and hole records that travel as launch arguments, the per-frame statistics and the mask.  Each translation
// unit gets its own copy of the kernels.
#pragma once
#include "common.h"

namespace df {
namespace {

constexpr int RB = 256;                 // threads per block, every kernel of the renderers
constexpr int RESOLVE_MAX_BLOCKS = 64;  // pixel blocks per frame in the resolve pass
constexpr unsigned long long NO_KEY = ~0ull;

constexpr int MAX_HOLES = 128;          // hole records per launch (and the largest K): they travel as kernel arguments

struct Camera {
  double p0[4], p1[4], p3[4];           // rows 0, 1 and 3 of the projection matrix
  double p22, p23;
};

// The holes of the frames of one launch, [frame - f0][K]: the host arrays are checked on the host and reach the device by value, so
// the call neither copies from pageable memory nor allocates.
struct Holes {
  double r[MAX_HOLES];
  int idx[MAX_HOLES];
};

// the loader's inverse assumes z' = p22 z + p23 and w' = -z (project_unity_depth.py:42-51)
inline bool proj_form_ok(const double *proj) {
  return proj[8] == 0.0 && proj[9] == 0.0 && proj[12] == 0.0 && proj[13] == 0.0 && proj[14] == -1.0 && proj[15] == 0.0;
}

inline Camera make_camera(const double *proj) {
  Camera cam;
  for (int k = 0; k < 4; ++k) { cam.p0[k] = proj[k]; cam.p1[k] = proj[4 + k]; cam.p3[k] = proj[12 + k]; }
  cam.p22 = proj[10]; cam.p23 = proj[11];
  return cam;
}

// the hole records of frames f0 .. f0 + nf - 1; the rest of the table is dead (-1)
inline Holes make_holes(const int *hole_idx, const double *hole_r, int K, int f0, int nf) {
  Holes holes;
  for (int j = 0; j < MAX_HOLES; ++j) {
    const bool live = j < nf * K;
    holes.idx[j] = live ? hole_idx[(size_t)f0 * K + j] : -1;
    holes.r[j] = live ? hole_r[(size_t)f0 * K + j] : 0.0;
  }
  return holes;
}

// While the blocks reduce, stats[f] = {covered, items, max(IH - row), max(row + 1), max(IW - col), max(col + 1)}: maxima only, so that
// zero means "nothing seen"; finish_kernel decodes the row.  One wave's share of a resolve pass: reduced across the wave, then one set of
// integer atomics.
__device__ inline void reduce_frame_stats(int cnt, int a_r, int b_r, int a_c, int b_c, int *__restrict__ s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    cnt += __shfl_down(cnt, off, 64);
    a_r = max(a_r, __shfl_down(a_r, off, 64)); b_r = max(b_r, __shfl_down(b_r, off, 64));
    a_c = max(a_c, __shfl_down(a_c, off, 64)); b_c = max(b_c, __shfl_down(b_c, off, 64));
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
    atomicAdd(&s[0], cnt);
    atomicMax(&s[2], a_r); atomicMax(&s[3], b_r); atomicMax(&s[4], a_c); atomicMax(&s[5], b_c);
  }
}

// {covered, items, rmin, rmax, cmin, cmax}, the box inclusive; all six zero when nothing is covered (an item that reached the z-buffer
// covers at least one pixel, so `items` is zero then already)
__global__ void finish_kernel(int F, int IH, int IW, int *__restrict__ stats) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  int *s = stats + (size_t)f * 6;
  if (s[0] == 0) { s[1] = s[2] = s[3] = s[4] = s[5] = 0; return; }
  s[2] = IH - s[2]; s[3] = s[3] - 1; s[4] = IW - s[4]; s[5] = s[5] - 1;
}

// mode 0: the half-open slice [rmin:rmax, cmin:cmax] of the inclusive box (mask_generator.py:21-28); mode 1: the covered pixels
__global__ __launch_bounds__(RB) void mask_kernel(const unsigned short *__restrict__ depth, const int *__restrict__ stats, int IH, int IW,
                                                  int mode, unsigned short *__restrict__ mask) {
  const int f = blockIdx.y;
  const int npix = IH * IW;
  const int *s = stats + (size_t)f * 6;
  const int rmin = s[2], rmax = s[3], cmin = s[4], cmax = s[5];
  const unsigned short *df = depth + (size_t)f * npix;
  unsigned short *mf = mask + (size_t)f * npix;
  for (int p = blockIdx.x * RB + threadIdx.x; p < npix; p += gridDim.x * RB) {
    bool on;
    if (mode == 0) {
      const int r = p / IW, q = p - r * IW;
      on = r >= rmin && r < rmax && q >= cmin && q < cmax;
    } else {
      on = df[p] != 65535;
    }
    mf[p] = on ? 65535 : 0;
  }
}

inline bool sizes_ok(int F, int IH, int IW) { return F > 0 && F <= 65535 && IH > 0 && IW > 0 && (long)IH * IW <= (1L << 30); }

}  // namespace
}  // namespace df
