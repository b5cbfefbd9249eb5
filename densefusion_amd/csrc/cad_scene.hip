// Multi-object customCAD scenes with occlusion: O meshes over one shared vertex and triangle array, each with its own pose per frame, drawn
// into one z-buffer.  The contract is the comment of df_cad_render_scene in include/dfusion.h: steps V2..V5 and T1..T7 are those of
// df_cad_render_mesh, through the very device functions of cad_raster_core.h (hence the same bits); tests/cad_scene_np.py restates it in
// numpy and the outputs are compared bit for bit.  Built with -ffp-contract=off: no fused multiply-add anywhere.
//
// Steps on the caller's stream: the keys are set to all-ones and the stats to zero; scene_raster_kernel (grid = triangle blocks x frames)
// keeps raster_kernel's shape -- one triangle per lane, small node ranges walked by the lane, large ones by the whole wave after a
// ballot, the plain load before atomicMin -- with the owner looked up in the tri_begin table and the pose and model scale per lane, since
// the object ranges do not align to waves.  scene_resolve_kernel finds the winner's owner in the same table, writes depth, colour and
// label, and counts pixels and boxes per owner: a lane gathers for one owner at a time, the wave reduces per distinct owner when a lane
// meets another one, then one set of integer atomics (the max-encoded scheme of reduce_frame_stats).  scene_finish_kernel decodes the
// boxes.  The object table (tri_begin, model_scale) is checked on the host and travels as a launch argument.
#include "cad_raster_core.h"

namespace df {
namespace {

constexpr int MAX_OBJECTS = DF_CAD_SCENE_MAX_OBJECTS;
static_assert(MAX_OBJECTS == 64, "owner_of searches a table of 64 entries in six steps");

// begin[o] .. begin[o + 1] - 1 are the triangles of object o; entries past O hold T, so that a search over all 64 stays below O
struct Objects {
  double scale[MAX_OBJECTS];
  int begin[MAX_OBJECTS + 1];
};

inline Objects make_objects(const int *tri_begin, const double *model_scale, int O, int T) {
  Objects ob;
  for (int k = 0; k <= MAX_OBJECTS; ++k) ob.begin[k] = k <= O ? tri_begin[k] : T;
  for (int k = 0; k < MAX_OBJECTS; ++k) ob.scale[k] = k < O ? model_scale[k] : 0.0;
  return ob;
}

// the object table in LDS: every lane searches it with its own index
struct ObjectsLds {
  double scale[MAX_OBJECTS];
  int begin[MAX_OBJECTS];
};

__device__ inline void stage_objects(ObjectsLds &s, const Objects &ob) {
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
                                                          Objects objects, int O, const double *__restrict__ pose,
                                                          const unsigned char *__restrict__ present, Camera cam, int IH, int IW, int cull,
                                                          unsigned long long *__restrict__ keys, int *__restrict__ stats) {
  __shared__ ObjectsLds tab;
  stage_objects(tab, objects);
  const int f = blockIdx.y;
  unsigned long long *kf = keys + (size_t)f * IH * IW;
  int *sf = stats + (size_t)f * O * 6;
  const int lane = threadIdx.x & 63;
  int reached = 0, reached_o = 0;                                             // `reached` counts for object `reached_o`
  // `base` is the same in all lanes of a wave, so the wave stays whole for the ballots and the shuffles below
  for (long base = (long)blockIdx.x * RB + (threadIdx.x - lane); base < T; base += (long)gridDim.x * RB) {
    const long i = base + lane;
    Tri tri = {};
    bool neg = false;
    int r0 = 0, r1 = -1, q0 = 0, q1 = -1;
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
    if (live) {                                                               // T1: nothing is read through an index outside 0..V-1
#pragma unroll
      for (int k = 0; k < 3; ++k) tri.id[k] = triangles[i * 3 + k];
      live = tri.id[0] >= 0 && tri.id[0] < V && tri.id[1] >= 0 && tri.id[1] < V && tri.id[2] >= 0 && tri.id[2] < V &&
             tri.id[0] != tri.id[1] && tri.id[1] != tri.id[2] && tri.id[0] != tri.id[2];
    }
    if (live) {
      const Pose P = load_pose(pose + ((size_t)f * O + o) * 12);
      const double model_scale = tab.scale[o];
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
      const unsigned bt = (unsigned)(base + src);                             // T7: the global triangle index
      bool hit = false;
      for (int j = lane; j < bn; j += 64) {
        const int jr = j / bw;
        hit |= raster_node(b, bneg, br0 + jr, bq0 + (j - jr * bw), bt, kf, IW);
      }
      if (__ballot(hit) && lane == src) ++reached;
    }
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

__global__ __launch_bounds__(RB) void scene_resolve_kernel(const unsigned long long *__restrict__ keys, const float *__restrict__ vertices,
                                                           const unsigned char *__restrict__ colors, const int *__restrict__ triangles,
                                                           Objects objects, int O, const double *__restrict__ pose, Camera cam, int IH,
                                                           int IW, unsigned char *__restrict__ rgb, unsigned short *__restrict__ depth,
                                                           unsigned short *__restrict__ label, int *__restrict__ stats) {
  __shared__ ObjectsLds tab;
  stage_objects(tab, objects);
  const int f = blockIdx.y;
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
      df[p] = 65535;                                                          // the horizon: above every code
      px[0] = 130; px[1] = 130; px[2] = 130;
      lf[p] = 0;
      continue;
    }
    const int r = p / IW, q = p - r * IW;
    // the winner passed T1..T7 in scene_raster_kernel: its indices are in range and its corners in front of the camera
    const size_t t = (size_t)(unsigned)(key & 0xffffffffu);
    const Pose P = load_pose(pose + ((size_t)f * O + o) * 12);
    const double model_scale = tab.scale[o];
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
    lf[p] = (unsigned short)(o + 1);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      px[ch] = to_channel(rint(((u0 * (double)c0[ch] + u1 * (double)c1[ch]) + u2 * (double)c2[ch]) / U));
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

inline bool objects_ok(int O) { return O >= 1 && O <= MAX_OBJECTS; }

}  // namespace
}  // namespace df

using namespace df;

// the keys only, as for df_cad_render_mesh
extern "C" size_t df_cad_render_scene_scratch_bytes(int F, int IH, int IW, int V, int T, int O) {
  return sizes_ok(F, IH, IW) && V > 0 && T > 0 && objects_ok(O) ? (size_t)F * IH * IW * sizeof(unsigned long long) : 0;
}

extern "C" int df_cad_render_scene(const float *vertices, const unsigned char *colors, int V, const int *triangles, int T, const int *tri_begin,
                                   const double *model_scale, int O, const double *pose, const unsigned char *present, const double *proj,
                                   int F, int IH, int IW, int cull, unsigned char *rgb_out, unsigned short *depth_out,
                                   unsigned short *label_out, int *stats_out, void *scratch, size_t scratch_bytes, df_stream_t stream) {
  if (!vertices || !colors || !triangles || !tri_begin || !model_scale || !pose || !proj || !rgb_out || !depth_out || !label_out ||
      !stats_out || !scratch)
    return set_error(DF_ERR_ARG, "cad_render_scene: null pointer");
  if (!objects_ok(O)) return set_error(DF_ERR_ARG, "cad_render_scene: O = %d objects outside 1..%d", O, MAX_OBJECTS);
  if (V <= 0 || T <= 0 || !sizes_ok(F, IH, IW)) return set_error(DF_ERR_ARG, "cad_render_scene: bad sizes");
  if (cull != 0 && cull != 1) return set_error(DF_ERR_ARG, "cad_render_scene: cull %d is neither 0 nor 1", cull);
  if (scratch_bytes < df_cad_render_scene_scratch_bytes(F, IH, IW, V, T, O) || (reinterpret_cast<uintptr_t>(scratch) & 7u))
    return set_error(DF_ERR_ARG, "cad_render_scene: scratch too small or not 8-byte aligned");
  if (!proj_form_ok(proj))
    return set_error(DF_ERR_ARG, "cad_render_scene: the projection matrix needs rows 2 = (0, 0, p22, p23) and 3 = (0, 0, -1, 0)");
  if (tri_begin[0] != 0) return set_error(DF_ERR_ARG, "cad_render_scene: tri_begin[0] = %d, not 0", tri_begin[0]);
  for (int o = 0; o < O; ++o)
    if (tri_begin[o + 1] < tri_begin[o])
      return set_error(DF_ERR_ARG, "cad_render_scene: tri_begin decreases from %d to %d at object %d", tri_begin[o], tri_begin[o + 1], o);
  if (tri_begin[O] != T) return set_error(DF_ERR_ARG, "cad_render_scene: tri_begin[O] = %d, not T = %d", tri_begin[O], T);
  hipStream_t st = to_stream(stream);
  const Camera cam = make_camera(proj);
  const Objects objects = make_objects(tri_begin, model_scale, O, T);
  const long npix = (long)IH * IW;
  if (hipMemsetAsync(scratch, 0xff, (size_t)F * npix * sizeof(unsigned long long), st) != hipSuccess ||
      hipMemsetAsync(stats_out, 0, sizeof(int) * 6 * (size_t)F * O, st) != hipSuccess)
    return check_launch("cad_render_scene (clear)");
  unsigned long long *keys = static_cast<unsigned long long *>(scratch);
  const int tb = cdiv(T, RB) < RASTER_MAX_BLOCKS ? cdiv(T, RB) : RASTER_MAX_BLOCKS;
  hipLaunchKernelGGL(scene_raster_kernel, dim3(tb, F), dim3(RB), 0, st, vertices, V, triangles, T, objects, O, pose, present, cam, IH, IW,
                     cull, keys, stats_out);
  const int xb = cdiv(npix, RB) < RESOLVE_MAX_BLOCKS ? cdiv(npix, RB) : RESOLVE_MAX_BLOCKS;
  hipLaunchKernelGGL(scene_resolve_kernel, dim3(xb, F), dim3(RB), 0, st, keys, vertices, colors, triangles, objects, O, pose, cam, IH, IW,
                     rgb_out, depth_out, label_out, stats_out);
  hipLaunchKernelGGL(scene_finish_kernel, dim3(cdiv((long)F * O, RB)), dim3(RB), 0, st, F * O, IH, IW, stats_out);
  return check_launch("cad_render_scene");
}

extern "C" int df_cad_scene_mask(const unsigned short *label, const int *stats, int F, int O, int IH, int IW, const int *pairs, int N,
                                 int mask_mode, unsigned short *mask_out, df_stream_t stream) {
  if (!label || !stats || !pairs || !mask_out) return set_error(DF_ERR_ARG, "cad_scene_mask: null pointer");
  if (!objects_ok(O)) return set_error(DF_ERR_ARG, "cad_scene_mask: O = %d objects outside 1..%d", O, MAX_OBJECTS);
  if (!sizes_ok(F, IH, IW) || N <= 0 || N > 65535) return set_error(DF_ERR_ARG, "cad_scene_mask: bad sizes");
  if (mask_mode != 0 && mask_mode != 1)
    return set_error(DF_ERR_ARG, "cad_scene_mask: mask_mode %d is neither 0 (box) nor 1 (pixels)", mask_mode);
  const long npix = (long)IH * IW;
  const int xb = cdiv(npix, RB) < RESOLVE_MAX_BLOCKS ? cdiv(npix, RB) : RESOLVE_MAX_BLOCKS;
  hipLaunchKernelGGL(scene_mask_kernel, dim3(xb, N), dim3(RB), 0, to_stream(stream), label, stats, F, O, IH, IW, pairs, mask_mode, mask_out);
  return check_launch("cad_scene_mask");
}
