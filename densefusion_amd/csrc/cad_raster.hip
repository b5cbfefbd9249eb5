// Triangle rasteriser for customCAD training sets: a coloured CAD mesh -> the frames cad_render.hip writes from a cloud (Unity-format
// colour, 16-bit depth, mask), drawn from the triangles themselves: watertight, no splat parameter, the depth exact on each facet up to the
// rounding of the 16-bit code.  The contract -- every fp64 operation and its order, steps V1..V5, T1..T7 and the resolve -- is the comment
// of df_cad_render_mesh in include/dfusion.h; tests/cad_raster_np.py restates it in numpy and the outputs are compared bit for bit.
// Built with -ffp-contract=off: no fused multiply-add anywhere.
//
// Steps on the caller's stream: the keys are set to all-ones; raster_kernel (grid = triangle blocks x frames) sets up one triangle per lane,
// recomputing V1..V5 for its three corners (no per-vertex scratch: see DESIGN), and takes atomicMin of (code << 32 | triangle index) on
// every covered node: small node ranges by the lane, large ones by the whole wave.  resolve_mesh_kernel recomputes the winner's edge
// functions (the same device functions, hence the same bits) for the perspective-correct colour; its LIT instantiation
// (df_cad_render_mesh_lit with a light) multiplies that colour by the diffuse term of the frame's light record, steps L1..L6.
// The set-up, the walks and the shading
// are the device functions of cad_raster_core.h, which cad_scene.hip shares; the kernels here add the pose of the block's frame, the
// hole test (vertex_cut, cad_frame.h) and the per-wave sum of the key-test counts.  finish_kernel and mask_kernel are those of the point
// renderer (cad_frame.h).  No clipping: a triangle with a corner behind the camera is dropped whole.
#include "cad_raster_core.h"

namespace df {
namespace {

// While the blocks reduce, stats[f][1] counts the triangles that took at least one key test (the rest of the row: reduce_frame_stats).
__global__ __launch_bounds__(RB) void raster_kernel(const float *__restrict__ vertices, int V, const int *__restrict__ triangles, int T,
                                                    const double *__restrict__ pose, double model_scale, Holes holes, int K, int f0,
                                                    Camera cam, int IH, int IW, int cull, unsigned long long *__restrict__ keys,
                                                    int *__restrict__ stats) {
  const int f = f0 + blockIdx.y;
  const Pose P = load_pose(pose + (size_t)f * 12);
  unsigned long long *kf = keys + (size_t)f * IH * IW;
  const int lane = threadIdx.x & 63;
  const int hb = blockIdx.y * K;
  int reached = 0;
  // `base` is the same in all lanes of a wave, so the wave stays whole for the ballot and the shuffles of the walks
  for (long base = (long)blockIdx.x * RB + (threadIdx.x - lane); base < T; base += (long)gridDim.x * RB) {
    const long i = base + lane;
    Setup s;
    bool live = i < T && load_triangle(s.tri, triangles, i, V);
    if (live)                                                                 // V1: a triangle goes with any of its vertices
      live = !(vertex_cut(vertices, s.tri.id[0], holes, hb, K) || vertex_cut(vertices, s.tri.id[1], holes, hb, K) ||
               vertex_cut(vertices, s.tri.id[2], holes, hb, K));
    live = live && setup_triangle(s, vertices, P, model_scale, cam, IH, IW, cull);
    reached += walk_triangles(s, live, base, kf, IW);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) reached += __shfl_down(reached, off, 64);
  if (lane == 0 && reached) atomicAdd(&stats[(size_t)f * 6 + 1], reached);
}

// LIT: the covered pixels take the diffuse term of light[f] (L1..L6); normals, normal_mode and light are not read otherwise
template <bool LIT>
__global__ __launch_bounds__(RB) void resolve_mesh_kernel(const unsigned long long *__restrict__ keys, const float *__restrict__ vertices,
                                                          const unsigned char *__restrict__ colors, const int *__restrict__ triangles,
                                                          const double *__restrict__ pose, double model_scale, Camera cam, int IH, int IW,
                                                          const float *__restrict__ normals, int normal_mode,
                                                          const double *__restrict__ light, unsigned char *__restrict__ rgb,
                                                          unsigned short *__restrict__ depth, int *__restrict__ stats) {
  const int f = blockIdx.y;
  const int npix = IH * IW;
  const Pose P = load_pose(pose + (size_t)f * 12);
  Shading sh = {};
  if constexpr (LIT) sh = load_shading(normals, normal_mode, light + (size_t)f * 8);
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
    const int r = p / IW, q = p - r * IW;
    shade_winner<LIT>(key, r, q, vertices, colors, triangles, P, model_scale, cam, IH, IW, sh, df + p, px);
    ++cnt;
    a_r = max(a_r, IH - r); b_r = max(b_r, r + 1);
    a_c = max(a_c, IW - q); b_c = max(b_c, q + 1);
  }
  reduce_frame_stats(cnt, a_r, b_r, a_c, b_c, stats + (size_t)f * 6);
}

}  // namespace
}  // namespace df

using namespace df;

// the keys only: V1..V5 are recomputed per triangle corner
extern "C" size_t df_cad_render_mesh_scratch_bytes(int F, int IH, int IW, int V, int T) {
  return sizes_ok(F, IH, IW) && V > 0 && T > 0 ? (size_t)F * IH * IW * sizeof(unsigned long long) : 0;
}

// df_cad_render_mesh (light == NULL) and df_cad_render_mesh_lit: `name` is the call's name in front of every message
static int render_mesh(const char *name, const float *vertices, const unsigned char *colors, int V, const int *triangles, int T,
                       const double *pose, double model_scale, const int *hole_idx, const double *hole_r, int K, const double *proj, int F,
                       int IH, int IW, int cull, int mask_mode, const float *normals, int normal_mode, const double *light,
                       unsigned char *rgb_out, unsigned short *depth_out, unsigned short *mask_out, int *stats_out, void *scratch,
                       size_t scratch_bytes, df_stream_t stream) {
  if (!vertices || !colors || !triangles || !pose || !proj || !rgb_out || !depth_out || !mask_out || !stats_out || !scratch)
    return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (light && !normals) return set_error(DF_ERR_ARG, "%s: null pointer (a light needs normals)", name);
  if (light && normal_mode != 0 && normal_mode != 1)
    return set_error(DF_ERR_ARG, "%s: normal_mode %d is neither 0 (per triangle) nor 1 (per vertex)", name, normal_mode);
  if (int e = check_hole_args(name, hole_idx, hole_r, K)) return e;
  if (V <= 0 || T <= 0 || !sizes_ok(F, IH, IW)) return set_error(DF_ERR_ARG, "%s: bad sizes", name);
  if (cull != 0 && cull != 1) return set_error(DF_ERR_ARG, "%s: cull %d is neither 0 nor 1", name, cull);
  if (mask_mode != 0 && mask_mode != 1) return set_error(DF_ERR_ARG, "%s: mask_mode %d is neither 0 (box) nor 1 (pixels)", name, mask_mode);
  if (int e = check_scratch_and_proj(name, scratch, scratch_bytes, df_cad_render_mesh_scratch_bytes(F, IH, IW, V, T), proj)) return e;
  if (int e = check_hole_indices(name, hole_idx, F, K, 'V', V)) return e;
  hipStream_t st = to_stream(stream);
  const Camera cam = make_camera(proj);
  const long npix = (long)IH * IW;
  if (!clear_frames(scratch, F, npix, stats_out, F, st)) return check_launch(name);
  unsigned long long *keys = static_cast<unsigned long long *>(scratch);
  const int tb = grid_blocks(T, RASTER_MAX_BLOCKS), xb = grid_blocks(npix, RESOLVE_MAX_BLOCKS);
  for_hole_batches(hole_idx, hole_r, K, F, [&](int f0, int nf, const Holes &holes) {
    hipLaunchKernelGGL(raster_kernel, dim3(tb, nf), dim3(RB), 0, st, vertices, V, triangles, T, pose, model_scale, holes, K, f0, cam, IH, IW,
                       cull, keys, stats_out);
  });
  hipLaunchKernelGGL(light ? resolve_mesh_kernel<true> : resolve_mesh_kernel<false>, dim3(xb, F), dim3(RB), 0, st, keys, vertices, colors,
                     triangles, pose, model_scale, cam, IH, IW, normals, normal_mode, light, rgb_out, depth_out, stats_out);
  hipLaunchKernelGGL(finish_kernel, dim3(cdiv(F, RB)), dim3(RB), 0, st, F, IH, IW, stats_out);
  hipLaunchKernelGGL(mask_kernel, dim3(xb, F), dim3(RB), 0, st, depth_out, stats_out, IH, IW, mask_mode, mask_out);
  return check_launch(name);
}

extern "C" int df_cad_render_mesh(const float *vertices, const unsigned char *colors, int V, const int *triangles, int T, const double *pose,
                                  double model_scale, const int *hole_idx, const double *hole_r, int K, const double *proj, int F, int IH,
                                  int IW, int cull, int mask_mode, unsigned char *rgb_out, unsigned short *depth_out,
                                  unsigned short *mask_out, int *stats_out, void *scratch, size_t scratch_bytes, df_stream_t stream) {
  return render_mesh("cad_render_mesh", vertices, colors, V, triangles, T, pose, model_scale, hole_idx, hole_r, K, proj, F, IH, IW, cull,
                     mask_mode, nullptr, 0, nullptr, rgb_out, depth_out, mask_out, stats_out, scratch, scratch_bytes, stream);
}

extern "C" int df_cad_render_mesh_lit(const float *vertices, const unsigned char *colors, int V, const int *triangles, int T,
                                      const double *pose, double model_scale, const int *hole_idx, const double *hole_r, int K,
                                      const double *proj, int F, int IH, int IW, int cull, int mask_mode, const float *normals,
                                      int normal_mode, const double *light, unsigned char *rgb_out, unsigned short *depth_out,
                                      unsigned short *mask_out, int *stats_out, void *scratch, size_t scratch_bytes, df_stream_t stream) {
  return render_mesh("cad_render_mesh_lit", vertices, colors, V, triangles, T, pose, model_scale, hole_idx, hole_r, K, proj, F, IH, IW, cull,
                     mask_mode, normals, normal_mode, light, rgb_out, depth_out, mask_out, stats_out, scratch, scratch_bytes, stream);
}
