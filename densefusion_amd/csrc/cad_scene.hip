// Multi-object customCAD scenes with occlusion: O meshes over one shared vertex and triangle array, each with its own pose per frame, drawn
// into one z-buffer.  The contract is the comment of df_cad_render_scene in include/dfusion.h: steps V2..V5 and T1..T7 are those of
// df_cad_render_mesh, through the very device functions of cad_raster_core.h (hence the same bits); tests/cad_scene_np.py restates it in
// numpy and the outputs are compared bit for bit.  Built with -ffp-contract=off: no fused multiply-add anywhere.
//
// Steps on the caller's stream: the keys are set to all-ones and the stats to zero; scene_raster_kernel (grid = triangle blocks x frames)
// runs the set-up and the walks of cad_raster_core.h as raster_kernel does -- one triangle per lane, small node ranges walked by the
// lane, large ones by the whole wave -- with the owner looked up in the tri_begin table and the pose and model scale per lane, since
// the object ranges do not align to waves, and hands its key-test counts over per owner.  scene_resolve_kernel finds the winner's owner
// in the same table, writes depth and colour (shade_winner, with the owner's pose and scale; its LIT instantiation, for
// df_cad_render_scene_lit with a light, applies steps L1..L6 with the owner's R and the frame's light record) and the label, and
// counts pixels and boxes per owner: a lane gathers for one owner at a time, the wave reduces per distinct owner when a lane meets another one, then one set of
// integer atomics (the max-encoded scheme of reduce_frame_stats).  scene_finish_kernel decodes the boxes.  The object table (tri_begin,
// model_scale) is checked on the host and travels as a launch argument.
#include "cad_raster_core.h"
#include "mesh_objects.h"

namespace df {
namespace {

static_assert(MAX_OBJECTS == 64, "owner_of searches a table of 64 entries in six steps");

// the object table in LDS: every lane searches it with its own index
struct ObjectsLds {
  double scale[MAX_OBJECTS];
  int begin[MAX_OBJECTS];
};

__device__ inline void stage_objects(ObjectsLds &s, const ObjectTable &ob) {
  if (threadIdx.x < MAX_OBJECTS) {
    s.scale[threadIdx.x] = ob.scale[threadIdx.x];
    s.begin[threadIdx.x] = ob.begin[threadIdx.x];
  }
  __syncthreads();
}

// the largest o with begin[o] <= t: for 0 <= t < T the owner of triangle t (begin[0] == 0, non-decreasing, begin[o] == T from O on; of
// several equal entries the last one is found, which skips the empty ranges)
__device__ inline int owner_of(const ObjectsLds &s, int t) {
  int o = 0;
#pragma unroll
  for (int step = MAX_OBJECTS / 2; step > 0; step >>= 1)
    if (s.begin[o + step] <= t) o += step;
  return o;
}

// The wave's per-lane counts, each for the lane's own object `o`, added to stats[o][1]: per distinct object one wave reduction and one
// atomic.  Called by whole waves only.
__device__ inline void flush_reached(int o, int reached, int *__restrict__ sf) {
  unsigned long long todo = __ballot(reached > 0);
  while (todo) {
    const int oo = __shfl(o, __ffsll((long long)todo) - 1, 64);
    const bool mine = reached > 0 && o == oo;
    int n = mine ? reached : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&sf[(size_t)oo * 6 + 1], n);
    todo &= ~__ballot(mine);
  }
}

// While the blocks reduce, stats[f][o][1] counts the triangles of object o that took at least one key test.
__global__ __launch_bounds__(RB) void scene_raster_kernel(const float *__restrict__ vertices, int V, const int *__restrict__ triangles, int T,
                                                          ObjectTable objects, int O, const double *__restrict__ pose,
                                                          const unsigned char *__restrict__ present, Camera cam, int IH, int IW, int cull,
                                                          unsigned long long *__restrict__ keys, int *__restrict__ stats) {
  __shared__ ObjectsLds tab;
  stage_objects(tab, objects);
  const int f = blockIdx.y;
  unsigned long long *kf = keys + (size_t)f * IH * IW;
  int *sf = stats + (size_t)f * O * 6;
  const int lane = threadIdx.x & 63;
  int reached = 0, reached_o = 0;                                             // `reached` counts for object `reached_o`
  // `base` is the same in all lanes of a wave, so the wave stays whole for the ballots and the shuffles below and in the walks
  for (long base = (long)blockIdx.x * RB + (threadIdx.x - lane); base < T; base += (long)gridDim.x * RB) {
    const long i = base + lane;
    Setup s;
    bool live = i < T;
    int o = reached_o;
    if (live) {
      o = owner_of(tab, (int)i);
      live = !present || present[(size_t)f * O + o] != 0;
    }
    // a lane that moves on to another object hands its count over first (whole wave: the test is a ballot)
    if (__ballot(o != reached_o && reached > 0)) {
      flush_reached(reached_o, reached, sf);
      reached = 0;
    }
    reached_o = o;
    live = live && load_triangle(s.tri, triangles, i, V);
    if (live) live = setup_triangle(s, vertices, load_pose(pose + ((size_t)f * O + o) * 12), tab.scale[o], cam, IH, IW, cull);
    reached += walk_triangles(s, live, base, kf, IW);                         // T7: the key carries the global triangle index
  }
  flush_reached(reached_o, reached, sf);
}

// one owner's share of a wave's gathered pixels: the lanes that gathered for another owner contribute nothing
struct Gather {
  int o, cnt, a_r, b_r, a_c, b_c;
};

// Called by whole waves only: per distinct owner among the lanes that gathered anything, reduce_frame_stats into that owner's row.
__device__ inline void flush_gather(Gather &g, int *__restrict__ sf) {
  unsigned long long todo = __ballot(g.cnt > 0);
  while (todo) {
    const int oo = __shfl(g.o, __ffsll((long long)todo) - 1, 64);
    const bool mine = g.cnt > 0 && g.o == oo;
    reduce_frame_stats(mine ? g.cnt : 0, mine ? g.a_r : 0, mine ? g.b_r : 0, mine ? g.a_c : 0, mine ? g.b_c : 0, sf + (size_t)oo * 6);
    todo &= ~__ballot(mine);
  }
  g.cnt = g.a_r = g.b_r = g.a_c = g.b_c = 0;
}

// LIT: the covered pixels take the diffuse term of light[f] (L1..L6); normals, normal_mode and light are not read otherwise
template <bool LIT>
__global__ __launch_bounds__(RB) void scene_resolve_kernel(const unsigned long long *__restrict__ keys, const float *__restrict__ vertices,
                                                           const unsigned char *__restrict__ colors, const int *__restrict__ triangles,
                                                           ObjectTable objects, int O, const double *__restrict__ pose, Camera cam, int IH,
                                                           int IW, const float *__restrict__ normals, int normal_mode,
                                                           const double *__restrict__ light, unsigned char *__restrict__ rgb,
                                                           unsigned short *__restrict__ depth, unsigned short *__restrict__ label,
                                                           int *__restrict__ stats) {
  __shared__ ObjectsLds tab;
  stage_objects(tab, objects);
  const int f = blockIdx.y;
  Shading sh = {};
  if constexpr (LIT) sh = load_shading(normals, normal_mode, light + (size_t)f * 8);
  const int npix = IH * IW;
  const unsigned long long *kf = keys + (size_t)f * npix;
  unsigned char *cf = rgb + (size_t)f * npix * 3;
  unsigned short *df = depth + (size_t)f * npix;
  unsigned short *lf = label + (size_t)f * npix;
  int *sf = stats + (size_t)f * O * 6;
  const int lane = threadIdx.x & 63;
  Gather g = {0, 0, 0, 0, 0, 0};
  // `base` is the same in all lanes of a wave: the flush inside the loop is taken by whole waves
  for (int base = blockIdx.x * RB + (threadIdx.x - lane); base < npix; base += gridDim.x * RB) {
    const int p = base + lane;
    const unsigned long long key = p < npix ? kf[p] : NO_KEY;
    const bool covered = key != NO_KEY;
    int o = g.o;
    if (covered) o = owner_of(tab, (int)(unsigned)(key & 0xffffffffu));
    if (__ballot(o != g.o && g.cnt > 0)) flush_gather(g, sf);                  // a lane met another owner: the wave hands over what it has
    g.o = o;
    if (p >= npix) continue;
    unsigned char *px = cf + (size_t)p * 3;
    if (!covered) {
      write_horizon(df + p, px);
      lf[p] = 0;
      continue;
    }
    const int r = p / IW, q = p - r * IW;
    shade_winner<LIT>(key, r, q, vertices, colors, triangles, load_pose(pose + ((size_t)f * O + o) * 12), tab.scale[o], cam, IH, IW, sh, df + p,
                      px);
    lf[p] = (unsigned short)(o + 1);
    ++g.cnt;
    g.a_r = max(g.a_r, IH - r); g.b_r = max(g.b_r, r + 1);
    g.a_c = max(g.a_c, IW - q); g.b_c = max(g.b_c, q + 1);
  }
  flush_gather(g, sf);
}

// {pixels won, triangles that took a key test, rmin, rmax, cmin, cmax} per frame and object, the box inclusive; the box is zero when the
// object won nothing, and entry 1 stays as counted: a hidden object tested keys and won none
__global__ void scene_finish_kernel(int rows, int IH, int IW, int *__restrict__ stats) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= rows) return;
  int *s = stats + (size_t)j * 6;
  if (s[0] == 0) { s[2] = s[3] = s[4] = s[5] = 0; return; }
  s[2] = IH - s[2]; s[3] = s[3] - 1; s[4] = IW - s[4]; s[5] = s[5] - 1;
}

// mode 0: the half-open slice [rmin:rmax, cmin:cmax] of the object's inclusive box (mask_generator.py:21-28); mode 1: the pixels it won
__global__ __launch_bounds__(RB) void scene_mask_kernel(const unsigned short *__restrict__ label, const int *__restrict__ stats, int F, int O,
                                                        int IH, int IW, const int *__restrict__ pairs, int mode,
                                                        unsigned short *__restrict__ mask) {
  const int n = blockIdx.y;
  const int npix = IH * IW;
  const int f = pairs[(size_t)n * 2], o = pairs[(size_t)n * 2 + 1];
  const bool ok = f >= 0 && f < F && o >= 0 && o < O;                         // nothing is read through a pair outside the call
  int rmin = 0, rmax = 0, cmin = 0, cmax = 0;
  if (ok && mode == 0) {
    const int *s = stats + ((size_t)f * O + o) * 6;
    rmin = s[2]; rmax = s[3]; cmin = s[4]; cmax = s[5];
  }
  const unsigned short *lf = label + (size_t)(ok ? f : 0) * npix;
  unsigned short *mf = mask + (size_t)n * npix;
  for (int p = blockIdx.x * RB + threadIdx.x; p < npix; p += gridDim.x * RB) {
    bool on = false;
    if (ok && mode == 0) {
      const int r = p / IW, q = p - r * IW;
      on = r >= rmin && r < rmax && q >= cmin && q < cmax;
    } else if (ok) {
      on = lf[p] == o + 1;
    }
    mf[p] = on ? 65535 : 0;
  }
}

}  // namespace
}  // namespace df

using namespace df;

// the keys only, as for df_cad_render_mesh
extern "C" size_t df_cad_render_scene_scratch_bytes(int F, int IH, int IW, int V, int T, int O) {
  return sizes_ok(F, IH, IW) && V > 0 && T > 0 && objects_ok(O) ? (size_t)F * IH * IW * sizeof(unsigned long long) : 0;
}

// df_cad_render_scene (light == NULL) and df_cad_render_scene_lit: `name` is the call's name in front of every message
static int render_scene(const char *name, const float *vertices, const unsigned char *colors, int V, const int *triangles, int T,
                        const int *tri_begin, const double *model_scale, int O, const double *pose, const unsigned char *present,
                        const double *proj, int F, int IH, int IW, int cull, const float *normals, int normal_mode, const double *light,
                        unsigned char *rgb_out, unsigned short *depth_out, unsigned short *label_out, int *stats_out, void *scratch,
                        size_t scratch_bytes, df_stream_t stream) {
  if (!vertices || !colors || !triangles || !tri_begin || !model_scale || !pose || !proj || !rgb_out || !depth_out || !label_out ||
      !stats_out || !scratch)
    return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (light && !normals) return set_error(DF_ERR_ARG, "%s: null pointer (a light needs normals)", name);
  if (light && normal_mode != 0 && normal_mode != 1)
    return set_error(DF_ERR_ARG, "%s: normal_mode %d is neither 0 (per triangle) nor 1 (per vertex)", name, normal_mode);
  if (!objects_ok(O)) return set_error(DF_ERR_ARG, "%s: O = %d objects outside 1..%d", name, O, MAX_OBJECTS);
  if (V <= 0 || T <= 0 || !sizes_ok(F, IH, IW)) return set_error(DF_ERR_ARG, "%s: bad sizes", name);
  if (cull != 0 && cull != 1) return set_error(DF_ERR_ARG, "%s: cull %d is neither 0 nor 1", name, cull);
  if (int e = check_scratch_and_proj(name, scratch, scratch_bytes, df_cad_render_scene_scratch_bytes(F, IH, IW, V, T, O), proj)) return e;
  if (int e = check_tri_begin(name, tri_begin, O, T, nullptr)) return e;
  hipStream_t st = to_stream(stream);
  const Camera cam = make_camera(proj);
  const ObjectTable objects = make_object_table(tri_begin, model_scale, O, T);
  const long npix = (long)IH * IW;
  if (!clear_frames(scratch, F, npix, stats_out, (size_t)F * O, st)) return check_launch(name);
  unsigned long long *keys = static_cast<unsigned long long *>(scratch);
  const int tb = grid_blocks(T, RASTER_MAX_BLOCKS), xb = grid_blocks(npix, RESOLVE_MAX_BLOCKS);
  hipLaunchKernelGGL(scene_raster_kernel, dim3(tb, F), dim3(RB), 0, st, vertices, V, triangles, T, objects, O, pose, present, cam, IH, IW,
                     cull, keys, stats_out);
  hipLaunchKernelGGL(light ? scene_resolve_kernel<true> : scene_resolve_kernel<false>, dim3(xb, F), dim3(RB), 0, st, keys, vertices, colors,
                     triangles, objects, O, pose, cam, IH, IW, normals, normal_mode, light, rgb_out, depth_out, label_out, stats_out);
  hipLaunchKernelGGL(scene_finish_kernel, dim3(cdiv((long)F * O, RB)), dim3(RB), 0, st, F * O, IH, IW, stats_out);
  return check_launch(name);
}

extern "C" int df_cad_render_scene(const float *vertices, const unsigned char *colors, int V, const int *triangles, int T, const int *tri_begin,
                                   const double *model_scale, int O, const double *pose, const unsigned char *present, const double *proj,
                                   int F, int IH, int IW, int cull, unsigned char *rgb_out, unsigned short *depth_out,
                                   unsigned short *label_out, int *stats_out, void *scratch, size_t scratch_bytes, df_stream_t stream) {
  return render_scene("cad_render_scene", vertices, colors, V, triangles, T, tri_begin, model_scale, O, pose, present, proj, F, IH, IW, cull,
                      nullptr, 0, nullptr, rgb_out, depth_out, label_out, stats_out, scratch, scratch_bytes, stream);
}

extern "C" int df_cad_render_scene_lit(const float *vertices, const unsigned char *colors, int V, const int *triangles, int T,
                                       const int *tri_begin, const double *model_scale, int O, const double *pose,
                                       const unsigned char *present, const double *proj, int F, int IH, int IW, int cull,
                                       const float *normals, int normal_mode, const double *light, unsigned char *rgb_out,
                                       unsigned short *depth_out, unsigned short *label_out, int *stats_out, void *scratch,
                                       size_t scratch_bytes, df_stream_t stream) {
  return render_scene("cad_render_scene_lit", vertices, colors, V, triangles, T, tri_begin, model_scale, O, pose, present, proj, F, IH, IW,
                      cull, normals, normal_mode, light, rgb_out, depth_out, label_out, stats_out, scratch, scratch_bytes, stream);
}

extern "C" int df_cad_scene_mask(const unsigned short *label, const int *stats, int F, int O, int IH, int IW, const int *pairs, int N,
                                 int mask_mode, unsigned short *mask_out, df_stream_t stream) {
  if (!label || !stats || !pairs || !mask_out) return set_error(DF_ERR_ARG, "cad_scene_mask: null pointer");
  if (!objects_ok(O)) return set_error(DF_ERR_ARG, "cad_scene_mask: O = %d objects outside 1..%d", O, MAX_OBJECTS);
  if (!sizes_ok(F, IH, IW) || N <= 0 || N > 65535) return set_error(DF_ERR_ARG, "cad_scene_mask: bad sizes");
  if (mask_mode != 0 && mask_mode != 1)
    return set_error(DF_ERR_ARG, "cad_scene_mask: mask_mode %d is neither 0 (box) nor 1 (pixels)", mask_mode);
  const int xb = grid_blocks((long)IH * IW, RESOLVE_MAX_BLOCKS);
  hipLaunchKernelGGL(scene_mask_kernel, dim3(xb, N), dim3(RB), 0, to_stream(stream), label, stats, F, O, IH, IW, pairs, mask_mode, mask_out);
  return check_launch("cad_scene_mask");
}
