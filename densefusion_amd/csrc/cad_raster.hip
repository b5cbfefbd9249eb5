// Triangle rasteriser for customCAD training sets: a coloured CAD mesh -> the frames cad_render.hip writes from a cloud (Unity-format
// colour, 16-bit depth, mask), drawn from the triangles themselves: watertight, no splat parameter, the depth exact on each facet up to the
// rounding of the 16-bit code.  The contract -- every fp64 operation and its order, steps V1..V5, T1..T7 and the resolve -- is the comment
// of df_cad_render_mesh in include/dfusion.h; tests/cad_raster_np.py restates it in numpy and the outputs are compared bit for bit.
// Built with -ffp-contract=off: no fused multiply-add anywhere.
//
// Steps on the caller's stream: the keys are set to all-ones; raster_kernel (grid = triangle blocks x frames) sets up one triangle per lane,
// recomputing V1..V5 for its three corners (no per-vertex scratch: see DESIGN), and takes atomicMin of (code << 32 | triangle index) on
// every covered node.  A triangle whose node range is small is walked by its own lane; the wave then takes its large triangles one at a
// time (ballot, setup broadcast by shuffles) with all 64 lanes striding over the node range.  resolve_mesh_kernel recomputes the winner's
// edge functions (the same device functions, hence the same bits) for the perspective-correct colour; finish_kernel and mask_kernel are
// those of the point renderer (cad_frame.h); the per-corner and per-node device functions are in cad_raster_core.h, which cad_scene.hip
// shares.  No clipping: a triangle with a corner behind the camera is dropped whole.
#include "cad_raster_core.h"

namespace df {
namespace {

// V1 (the hole rule of step 1 of df_cad_render; the centres are vertices)
__device__ inline bool vertex_cut(const float *__restrict__ vertices, int v, const Holes &holes, int hb, int K) {
  const double mx = (double)vertices[(size_t)v * 3], my = (double)vertices[(size_t)v * 3 + 1], mz = (double)vertices[(size_t)v * 3 + 2];
  bool cut = false;
  for (int k = 0; k < K; ++k) {
    const int h = holes.idx[hb + k];
    if (h < 0) continue;
    const double cx = (double)vertices[(size_t)h * 3], cy = (double)vertices[(size_t)h * 3 + 1], cz = (double)vertices[(size_t)h * 3 + 2];
    const double r = holes.r[hb + k];
    const double dx = mx - cx, dy = my - cy, dz = mz - cz;
    cut |= ((dx * dx + dy * dy) + dz * dz) <= r * r;
  }
  return cut;
}

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
  // `base` is the same in all lanes of a wave, so the wave stays whole for the ballot and the shuffles below
  for (long base = (long)blockIdx.x * RB + (threadIdx.x - lane); base < T; base += (long)gridDim.x * RB) {
    const long i = base + lane;
    Tri tri = {};
    bool neg = false;
    int r0 = 0, r1 = -1, q0 = 0, q1 = -1;
    bool live = i < T;
    if (live) {                                                               // T1: nothing is read through an index outside 0..V-1
#pragma unroll
      for (int k = 0; k < 3; ++k) tri.id[k] = triangles[i * 3 + k];
      live = tri.id[0] >= 0 && tri.id[0] < V && tri.id[1] >= 0 && tri.id[1] < V && tri.id[2] >= 0 && tri.id[2] < V &&
             tri.id[0] != tri.id[1] && tri.id[1] != tri.id[2] && tri.id[0] != tri.id[2];
    }
    if (live)
      live = !(vertex_cut(vertices, tri.id[0], holes, hb, K) || vertex_cut(vertices, tri.id[1], holes, hb, K) ||
               vertex_cut(vertices, tri.id[2], holes, hb, K));
    if (live) {
      const bool f0_ = project_corner<0>(tri, vertices, P, model_scale, cam, IH, IW);
      const bool f1_ = project_corner<1>(tri, vertices, P, model_scale, cam, IH, IW);
      const bool f2_ = project_corner<2>(tri, vertices, P, model_scale, cam, IH, IW);
      live = f0_ && f1_ && f2_;
    }
    if (live) {
      const double A = signed_area(tri);                                      // T3
      live = A != 0.0 && A - A == 0.0 && !(cull == 1 && A > 0.0);             // A - A == 0: finite
      neg = A < 0.0;
    }
    if (live) {                                                               // T4: compared as doubles, before any conversion
      const double cq0 = fmax(ceil(fmin(fmin(tri.sx[0], tri.sx[1]), tri.sx[2])), 0.0);
      const double cq1 = fmin(floor(fmax(fmax(tri.sx[0], tri.sx[1]), tri.sx[2])), (double)(IW - 1));
      const double cr0 = fmax(ceil(fmin(fmin(tri.sy[0], tri.sy[1]), tri.sy[2])), 0.0);
      const double cr1 = fmin(floor(fmax(fmax(tri.sy[0], tri.sy[1]), tri.sy[2])), (double)(IH - 1));
      live = cq0 <= cq1 && cr0 <= cr1;
      if (live) { q0 = (int)cq0; q1 = (int)cq1; r0 = (int)cr0; r1 = (int)cr1; }
    }
    const int n = live ? (r1 - r0 + 1) * (q1 - q0 + 1) : 0;                   // at most IH * IW <= 2^30
    if (live && n <= SMALL_NODES) {
      bool hit = false;
      for (int r = r0; r <= r1; ++r)
        for (int q = q0; q <= q1; ++q) hit |= raster_node(tri, neg, r, q, (unsigned)i, kf, IW);
      reached += hit;
    }
    unsigned long long big = __ballot(live && n > SMALL_NODES);
    while (big) {                                                             // the wave's large triangles, one at a time, all lanes
      const int src = __ffsll((long long)big) - 1;
      big &= big - 1;
      Tri b;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        b.id[k] = __shfl(tri.id[k], src, 64);
        b.sx[k] = __shfl(tri.sx[k], src, 64); b.sy[k] = __shfl(tri.sy[k], src, 64); b.d[k] = __shfl(tri.d[k], src, 64);
      }
      const bool bneg = __shfl((int)neg, src, 64) != 0;
      const int br0 = __shfl(r0, src, 64), br1 = __shfl(r1, src, 64), bq0 = __shfl(q0, src, 64), bq1 = __shfl(q1, src, 64);
      const int bw = bq1 - bq0 + 1, bn = (br1 - br0 + 1) * bw;
      const unsigned bt = (unsigned)(base + src);
      bool hit = false;
      for (int j = lane; j < bn; j += 64) {
        const int jr = j / bw;
        hit |= raster_node(b, bneg, br0 + jr, bq0 + (j - jr * bw), bt, kf, IW);
      }
      if (__ballot(hit) && lane == src) ++reached;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) reached += __shfl_down(reached, off, 64);
  if (lane == 0 && reached) atomicAdd(&stats[(size_t)f * 6 + 1], reached);
}

__global__ __launch_bounds__(RB) void resolve_mesh_kernel(const unsigned long long *__restrict__ keys, const float *__restrict__ vertices,
                                                          const unsigned char *__restrict__ colors, const int *__restrict__ triangles,
                                                          const double *__restrict__ pose, double model_scale, Camera cam, int IH, int IW,
                                                          unsigned char *__restrict__ rgb, unsigned short *__restrict__ depth,
                                                          int *__restrict__ stats) {
  const int f = blockIdx.y;
  const int npix = IH * IW;
  const Pose P = load_pose(pose + (size_t)f * 12);
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
    const int r = p / IW, q = p - r * IW;
    // the winner passed T1..T7 in raster_kernel: its indices are in range and its corners in front of the camera
    const size_t t = (size_t)(unsigned)(key & 0xffffffffu);
    Tri tri;
#pragma unroll
    for (int k = 0; k < 3; ++k) tri.id[k] = triangles[t * 3 + k];
    project_corner<0>(tri, vertices, P, model_scale, cam, IH, IW);
    project_corner<1>(tri, vertices, P, model_scale, cam, IH, IW);
    project_corner<2>(tri, vertices, P, model_scale, cam, IH, IW);
    double w[3], W;
    node_weights(tri, signed_area(tri) < 0.0, r, q, w, W);
    const double u0 = w[0] / tri.c3[0], u1 = w[1] / tri.c3[1], u2 = w[2] / tri.c3[2];
    const double U = (u0 + u1) + u2;
    const unsigned char *c0 = colors + (size_t)tri.id[0] * 3, *c1 = colors + (size_t)tri.id[1] * 3, *c2 = colors + (size_t)tri.id[2] * 3;
    df[p] = (unsigned short)(key >> 32);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      px[ch] = to_channel(rint(((u0 * (double)c0[ch] + u1 * (double)c1[ch]) + u2 * (double)c2[ch]) / U));
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

extern "C" int df_cad_render_mesh(const float *vertices, const unsigned char *colors, int V, const int *triangles, int T, const double *pose,
                                  double model_scale, const int *hole_idx, const double *hole_r, int K, const double *proj, int F, int IH,
                                  int IW, int cull, int mask_mode, unsigned char *rgb_out, unsigned short *depth_out,
                                  unsigned short *mask_out, int *stats_out, void *scratch, size_t scratch_bytes, df_stream_t stream) {
  if (!vertices || !colors || !triangles || !pose || !proj || !rgb_out || !depth_out || !mask_out || !stats_out || !scratch)
    return set_error(DF_ERR_ARG, "cad_render_mesh: null pointer");
  if (K > 0 && (!hole_idx || !hole_r)) return set_error(DF_ERR_ARG, "cad_render_mesh: null pointer (K holes need hole_idx and hole_r)");
  if (K < 0 || K > MAX_HOLES) return set_error(DF_ERR_ARG, "cad_render_mesh: K = %d holes per frame outside 0..%d", K, MAX_HOLES);
  if (V <= 0 || T <= 0 || !sizes_ok(F, IH, IW)) return set_error(DF_ERR_ARG, "cad_render_mesh: bad sizes");
  if (cull != 0 && cull != 1) return set_error(DF_ERR_ARG, "cad_render_mesh: cull %d is neither 0 nor 1", cull);
  if (mask_mode != 0 && mask_mode != 1)
    return set_error(DF_ERR_ARG, "cad_render_mesh: mask_mode %d is neither 0 (box) nor 1 (pixels)", mask_mode);
  if (scratch_bytes < df_cad_render_mesh_scratch_bytes(F, IH, IW, V, T) || (reinterpret_cast<uintptr_t>(scratch) & 7u))
    return set_error(DF_ERR_ARG, "cad_render_mesh: scratch too small or not 8-byte aligned");
  if (!proj_form_ok(proj))
    return set_error(DF_ERR_ARG, "cad_render_mesh: the projection matrix needs rows 2 = (0, 0, p22, p23) and 3 = (0, 0, -1, 0)");
  for (long j = 0; j < (long)F * K; ++j)
    if (hole_idx[j] >= V)
      return set_error(DF_ERR_ARG, "cad_render_mesh: hole index %d of frame %ld is not below V = %d", hole_idx[j], j / K, V);
  hipStream_t st = to_stream(stream);
  const Camera cam = make_camera(proj);
  const long npix = (long)IH * IW;
  if (hipMemsetAsync(scratch, 0xff, (size_t)F * npix * sizeof(unsigned long long), st) != hipSuccess ||
      hipMemsetAsync(stats_out, 0, sizeof(int) * 6 * F, st) != hipSuccess)
    return check_launch("cad_render_mesh (clear)");
  unsigned long long *keys = static_cast<unsigned long long *>(scratch);
  const int tb = cdiv(T, RB) < RASTER_MAX_BLOCKS ? cdiv(T, RB) : RASTER_MAX_BLOCKS;
  const int per_launch = K > 0 ? MAX_HOLES / K : F;                        // frames per raster launch: their holes fit one Holes
  for (int f0 = 0; f0 < F; f0 += per_launch) {
    const int nf = F - f0 < per_launch ? F - f0 : per_launch;
    const Holes holes = make_holes(hole_idx, hole_r, K, f0, nf);
    hipLaunchKernelGGL(raster_kernel, dim3(tb, nf), dim3(RB), 0, st, vertices, V, triangles, T, pose, model_scale, holes, K, f0, cam, IH, IW,
                       cull, keys, stats_out);
  }
  const int xb = cdiv(npix, RB) < RESOLVE_MAX_BLOCKS ? cdiv(npix, RB) : RESOLVE_MAX_BLOCKS;
  hipLaunchKernelGGL(resolve_mesh_kernel, dim3(xb, F), dim3(RB), 0, st, keys, vertices, colors, triangles, pose, model_scale, cam, IH, IW,
                     rgb_out, depth_out, stats_out);
  hipLaunchKernelGGL(finish_kernel, dim3(cdiv(F, RB)), dim3(RB), 0, st, F, IH, IW, stats_out);
  hipLaunchKernelGGL(mask_kernel, dim3(xb, F), dim3(RB), 0, st, depth_out, stats_out, IH, IW, mask_mode, mask_out);
  return check_launch("cad_render_mesh");
}
