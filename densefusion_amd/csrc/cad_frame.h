// What the customCAD renderers share (cad_render.hip: points; cad_raster.hip: triangles; cad_scene.hip: several meshes with occlusion):
// the z-buffer key and the horizon, the pose, camera and hole records and the hole rule of step 1, the per-frame statistics and the mask,
// and on the host the argument checks, the two clears, the grid clamp and the hole batches of the entry points.  Each translation unit
// gets its own copy of the kernels.
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

struct Pose {
  double R[3][3], t[3];
};

__device__ inline Pose load_pose(const double *__restrict__ T) {
  Pose p;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    p.R[j][0] = T[j * 4]; p.R[j][1] = T[j * 4 + 1]; p.R[j][2] = T[j * 4 + 2]; p.t[j] = T[j * 4 + 3];
  }
  return p;
}

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

// Step 1 of df_cad_render (V1 of the mesh calls, whose centres are vertices): point v of `xyz` lies within a hole of the launch's frame
// whose records begin at `hb`
__device__ inline bool vertex_cut(const float *__restrict__ xyz, long v, const Holes &holes, int hb, int K) {
  const double mx = (double)xyz[(size_t)v * 3], my = (double)xyz[(size_t)v * 3 + 1], mz = (double)xyz[(size_t)v * 3 + 2];
  bool cut = false;
  for (int k = 0; k < K; ++k) {
    const int h = holes.idx[hb + k];
    if (h < 0) continue;
    const double cx = (double)xyz[(size_t)h * 3], cy = (double)xyz[(size_t)h * 3 + 1], cz = (double)xyz[(size_t)h * 3 + 2];
    const double r = holes.r[hb + k];
    const double dx = mx - cx, dy = my - cy, dz = mz - cz;
    cut |= ((dx * dx + dy * dy) + dz * dz) <= r * r;
  }
  return cut;
}

// an uncovered pixel: the horizon, above every code, in the loader's grey
__device__ inline void write_horizon(unsigned short *__restrict__ depth, unsigned char *__restrict__ px) {
  *depth = 65535;
  px[0] = 130; px[1] = 130; px[2] = 130;
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

// The host side of the entry points; `name` is the call's name in front of every message.

inline int check_scratch_and_proj(const char *name, const void *scratch, size_t scratch_bytes, size_t need, const double *proj) {
  if (scratch_bytes < need || (reinterpret_cast<uintptr_t>(scratch) & 7u))
    return set_error(DF_ERR_ARG, "%s: scratch too small or not 8-byte aligned", name);
  if (!proj_form_ok(proj))
    return set_error(DF_ERR_ARG, "%s: the projection matrix needs rows 2 = (0, 0, p22, p23) and 3 = (0, 0, -1, 0)", name);
  return DF_OK;
}

inline int check_hole_args(const char *name, const int *hole_idx, const double *hole_r, int K) {
  if (K > 0 && (!hole_idx || !hole_r)) return set_error(DF_ERR_ARG, "%s: null pointer (K holes need hole_idx and hole_r)", name);
  if (K < 0 || K > MAX_HOLES) return set_error(DF_ERR_ARG, "%s: K = %d holes per frame outside 0..%d", name, K, MAX_HOLES);
  return DF_OK;
}

// every hole index is below the `n` points or vertices of the call (`what` is P or V)
inline int check_hole_indices(const char *name, const int *hole_idx, int F, int K, char what, int n) {
  for (long j = 0; j < (long)F * K; ++j)
    if (hole_idx[j] >= n)
      return set_error(DF_ERR_ARG, "%s: hole index %d of frame %ld is not below %c = %d", name, hole_idx[j], j / K, what, n);
  return DF_OK;
}

// the keys of F frames to all-ones, `rows` rows of statistics to zero
inline bool clear_frames(void *keys, int F, long npix, int *stats, size_t rows, hipStream_t st) {
  return hipMemsetAsync(keys, 0xff, (size_t)F * npix * sizeof(unsigned long long), st) == hipSuccess &&
         hipMemsetAsync(stats, 0, sizeof(int) * 6 * rows, st) == hipSuccess;
}

// blocks of RB threads for `items`, at most `max_blocks`: the threads stride over the rest
inline int grid_blocks(long items, int max_blocks) { return cdiv(items, RB) < max_blocks ? cdiv(items, RB) : max_blocks; }

// The F frames of a single-object call in launches of as many frames as have their holes in one Holes: launch(f0, nf, holes)
template <class Launch>
inline void for_hole_batches(const int *hole_idx, const double *hole_r, int K, int F, Launch launch) {
  const int per_launch = K > 0 ? MAX_HOLES / K : F;
  for (int f0 = 0; f0 < F; f0 += per_launch) {
    const int nf = F - f0 < per_launch ? F - f0 : per_launch;
    launch(f0, nf, make_holes(hole_idx, hole_r, K, f0, nf));
  }
}

}  // namespace
}  // namespace df
