// What the two triangle rasterisers share (cad_raster.hip: one mesh per frame, with holes; cad_scene.hip: several objects per frame with
// occlusion): steps V2..V5 and T1..T7 of df_cad_render_mesh (include/dfusion.h) and the winner's shading as device functions, from the
// corner and the node up to the triangle's set-up (load_triangle, setup_triangle), the two walks of a wave (walk_triangles) and the
// covered pixel of the resolve pass, unlit or lit (shade_winner).  A kernel adds where pose, scale and owner come from, its hole test
// and how it hands its counts over.  Each translation unit gets its own copy; both are built with -ffp-contract=off, so the same code gives the same bits
// in both.
#pragma once
#include "cad_frame.h"

namespace df {
namespace {

constexpr int RASTER_MAX_BLOCKS = 256;  // triangle blocks per frame: the waves stride over the rest
constexpr int SMALL_NODES = 16;         // node ranges up to this size are walked by the lane that set the triangle up

// one triangle on the screen: corner k is vertex id[k] at (sx, sy) with depth value d (V5) and clip-space w = c3
struct Tri {
  int id[3];
  double sx[3], sy[3], d[3], c3[3];
};

// V1..V5 for corner k of tri; false when the vertex is behind (c3 > 0 fails)
template <int k>
__device__ inline bool project_corner(Tri &tri, const float *__restrict__ vertices, const Pose &P, double model_scale, const Camera &cam,
                                      int IH, int IW) {
  const int v = tri.id[k];
  const double mx = (double)vertices[(size_t)v * 3], my = (double)vertices[(size_t)v * 3 + 1], mz = (double)vertices[(size_t)v * 3 + 2];
  const double sx = mx * model_scale, sy = my * model_scale, sz = mz * model_scale;        // V2
  double X[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) X[j] = ((P.R[j][0] * sx + P.R[j][1] * sy) + P.R[j][2] * sz) + P.t[j];
  const double c0 = ((cam.p0[0] * X[0] + cam.p0[1] * X[1]) + cam.p0[2] * X[2]) + cam.p0[3];        // V3
  const double c1 = ((cam.p1[0] * X[0] + cam.p1[1] * X[1]) + cam.p1[2] * X[2]) + cam.p1[3];
  const double c3 = ((cam.p3[0] * X[0] + cam.p3[1] * X[1]) + cam.p3[2] * X[2]) + cam.p3[3];
  const double ndc_x = c0 / c3, ndc_y = c1 / c3;
  tri.sx[k] = ((ndc_x + 1.0) * (double)IW) * 0.5;                                           // V4
  tri.sy[k] = ((1.0 - ndc_y) * (double)IH) * 0.5;
  tri.d[k] = (1.0 + cam.p22) + cam.p23 / X[2];                                              // V5
  tri.c3[k] = c3;
  return c3 > 0.0;
}

// T2: the edge function of the ordered pair (corner a, corner b) at (px, py), evaluated from the lower vertex index to the higher
template <int a, int b>
__device__ inline double edge_fn(const Tri &tri, double px, double py) {
  const bool fwd = tri.id[a] < tri.id[b];
  const double xlo = fwd ? tri.sx[a] : tri.sx[b], xhi = fwd ? tri.sx[b] : tri.sx[a];
  const double ylo = fwd ? tri.sy[a] : tri.sy[b], yhi = fwd ? tri.sy[b] : tri.sy[a];
  const double e = (xhi - xlo) * (py - ylo) - (yhi - ylo) * (px - xlo);
  return fwd ? e : -e;
}

// T3
__device__ inline double signed_area(const Tri &tri) { return edge_fn<0, 1>(tri, tri.sx[2], tri.sy[2]); }

// T5: the three weights at node (r, q); false when the node is not covered
__device__ inline bool node_weights(const Tri &tri, bool neg, int r, int q, double w[3], double &W) {
  const double px = (double)q, py = (double)r;
  w[0] = edge_fn<1, 2>(tri, px, py); w[1] = edge_fn<2, 0>(tri, px, py); w[2] = edge_fn<0, 1>(tri, px, py);
  if (neg) { w[0] = -w[0]; w[1] = -w[1]; w[2] = -w[2]; }
  if (!(w[0] >= 0.0 && w[1] >= 0.0 && w[2] >= 0.0)) return false;
  W = (w[0] + w[1]) + w[2];
  return W > 0.0;
}

// T5..T7 at one node of the frame (0 <= r < IH, 0 <= q < IW by T4); true when the node took a key test
__device__ inline bool raster_node(const Tri &tri, bool neg, int r, int q, unsigned t, unsigned long long *__restrict__ kf, int IW) {
  double w[3], W;
  if (!node_weights(tri, neg, r, q, w, W)) return false;
  const double code = rint(65534.0 * (((w[0] * tri.d[0] + w[1] * tri.d[1]) + w[2] * tri.d[2]) / W));      // T6, ties to even
  if (!(code >= 0.0 && code <= 65534.0)) return false;
  const unsigned long long key = ((unsigned long long)(unsigned)(int)code << 32) | t;                      // T7
  unsigned long long *dst = kf + (size_t)r * IW + q;
  if (*dst > key) atomicMin(dst, key);                                        // keys only decrease: a stale read costs one atomic, no more
  return true;
}

// The functions below are __forceinline__: inlined before anything is optimised, a kernel compiles as if the step were written out in it.
// Left to the inliner's own time, shade_winner costs resolve_mesh_kernel six VGPRs and with them one of its 7 waves per SIMD.

// a triangle ready for the walks: its corners on the screen, its orientation and its node range (T4), which is empty until
// setup_triangle finds the triangle live
struct Setup {
  Tri tri = {};
  bool neg = false;
  int r0 = 0, r1 = -1, q0 = 0, q1 = -1;
};

// T1 for triangle i: false unless its three indices are distinct and in 0..V-1, so that nothing is read through any other
__device__ __forceinline__ bool load_triangle(Tri &tri, const int *__restrict__ triangles, long i, int V) {
#pragma unroll
  for (int k = 0; k < 3; ++k) tri.id[k] = triangles[i * 3 + k];
  return tri.id[0] >= 0 && tri.id[0] < V && tri.id[1] >= 0 && tri.id[1] < V && tri.id[2] >= 0 && tri.id[2] < V &&
         tri.id[0] != tri.id[1] && tri.id[1] != tri.id[2] && tri.id[0] != tri.id[2];
}

// V2..V5 on the three corners of a triangle that passed T1, then T3 and T4; true when the triangle is live
__device__ __forceinline__ bool setup_triangle(Setup &s, const float *__restrict__ vertices, const Pose &P, double model_scale,
                                               const Camera &cam, int IH, int IW, int cull) {
  Tri &tri = s.tri;
  const bool f0 = project_corner<0>(tri, vertices, P, model_scale, cam, IH, IW);
  const bool f1 = project_corner<1>(tri, vertices, P, model_scale, cam, IH, IW);
  const bool f2 = project_corner<2>(tri, vertices, P, model_scale, cam, IH, IW);
  if (!(f0 && f1 && f2)) return false;
  const double A = signed_area(tri);                                          // T3
  if (!(A != 0.0 && A - A == 0.0 && !(cull == 1 && A > 0.0))) return false;   // A - A == 0: finite
  s.neg = A < 0.0;
  // T4: compared as doubles, before any conversion
  const double cq0 = fmax(ceil(fmin(fmin(tri.sx[0], tri.sx[1]), tri.sx[2])), 0.0);
  const double cq1 = fmin(floor(fmax(fmax(tri.sx[0], tri.sx[1]), tri.sx[2])), (double)(IW - 1));
  const double cr0 = fmax(ceil(fmin(fmin(tri.sy[0], tri.sy[1]), tri.sy[2])), 0.0);
  const double cr1 = fmin(floor(fmax(fmax(tri.sy[0], tri.sy[1]), tri.sy[2])), (double)(IH - 1));
  if (!(cq0 <= cq1 && cr0 <= cr1)) return false;
  s.q0 = (int)cq0; s.q1 = (int)cq1; s.r0 = (int)cr0; s.r1 = (int)cr1;
  return true;
}

// The two walks of the triangles base .. base + 63, lane k holding the set-up of triangle base + k.  A live triangle whose node range
// is small is walked by its own lane; the wave then takes its large triangles one at a time (ballot, set-up broadcast by shuffles)
// with all 64 lanes striding over the node range.  Called by whole waves with `base` the same in all lanes; returns how many
// triangles that took a key test this lane is to count (the lane that set a large triangle up counts it).
__device__ __forceinline__ int walk_triangles(const Setup &s, bool live, long base, unsigned long long *__restrict__ kf, int IW) {
  const int lane = threadIdx.x & 63;
  int reached = 0;
  const int n = live ? (s.r1 - s.r0 + 1) * (s.q1 - s.q0 + 1) : 0;             // at most IH * IW <= 2^30
  if (live && n <= SMALL_NODES) {
    bool hit = false;
    for (int r = s.r0; r <= s.r1; ++r)
      for (int q = s.q0; q <= s.q1; ++q) hit |= raster_node(s.tri, s.neg, r, q, (unsigned)(base + lane), kf, IW);
    reached += hit;
  }
  unsigned long long big = __ballot(live && n > SMALL_NODES);
  while (big) {
    const int src = __ffsll((long long)big) - 1;
    big &= big - 1;
    Tri b;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      b.id[k] = __shfl(s.tri.id[k], src, 64);
      b.sx[k] = __shfl(s.tri.sx[k], src, 64); b.sy[k] = __shfl(s.tri.sy[k], src, 64); b.d[k] = __shfl(s.tri.d[k], src, 64);
    }
    const bool bneg = __shfl((int)s.neg, src, 64) != 0;
    const int br0 = __shfl(s.r0, src, 64), br1 = __shfl(s.r1, src, 64), bq0 = __shfl(s.q0, src, 64), bq1 = __shfl(s.q1, src, 64);
    const int bw = bq1 - bq0 + 1, bn = (br1 - br0 + 1) * bw;
    const unsigned bt = (unsigned)(base + src);                               // T7: the index in the call's triangle array
    bool hit = false;
    for (int j = lane; j < bn; j += 64) {
      const int jr = j / bw;
      hit |= raster_node(b, bneg, br0 + jr, bq0 + (j - jr * bw), bt, kf, IW);
    }
    if (__ballot(hit) && lane == src) ++reached;
  }
  return reached;
}

__device__ inline unsigned char to_channel(double v) { return (unsigned char)(v >= 0.0 ? (v <= 255.0 ? v : 255.0) : 0.0); }      // NaN -> 0

// What the lit resolve adds to a frame's covered pixels (steps L1..L6 of df_cad_render_mesh_lit): the normals of the call and the light
// record of the block's frame, {L, ambient, diffuse, colour}.  The record is the same in all lanes of a block (scalar loads).
struct Shading {
  const float *normals;
  int mode;                             // 0: one normal per triangle, 1: one per vertex
  double L[3], ambient, diffuse, c[3];
};

__device__ inline Shading load_shading(const float *__restrict__ normals, int mode, const double *__restrict__ rec) {
  Shading sh;
  sh.normals = normals; sh.mode = mode;
  sh.L[0] = rec[0]; sh.L[1] = rec[1]; sh.L[2] = rec[2]; sh.ambient = rec[3]; sh.diffuse = rec[4];
  sh.c[0] = rec[5]; sh.c[1] = rec[6]; sh.c[2] = rec[7];
  return sh;
}

// L1, L2: component j of the normal at n, turned by the pose's R as step 3 of df_cad_render turns a point's
__device__ inline double rotated_normal(const Pose &P, int j, const float *__restrict__ n) {
  return (P.R[j][0] * (double)n[0] + P.R[j][1] * (double)n[1]) + P.R[j][2] * (double)n[2];
}

// The covered pixel (r, q) of the resolve pass: depth from the key, the perspective-correct colour from the winner's recomputed corners
// and edge functions, with LIT times the diffuse term of the frame's light (L1..L6; `sh` is not read otherwise).  The winner passed
// T1..T7 in the raster pass: its indices are in range and its corners in front of the camera.
template <bool LIT>
__device__ __forceinline__ void shade_winner(unsigned long long key, int r, int q, const float *__restrict__ vertices,
                                             const unsigned char *__restrict__ colors, const int *__restrict__ triangles, const Pose &P,
                                             double model_scale, const Camera &cam, int IH, int IW, const Shading &sh,
                                             unsigned short *__restrict__ depth, unsigned char *__restrict__ px) {
  const size_t t = (size_t)(unsigned)(key & 0xffffffffu);
  Tri tri;
#pragma unroll
  for (int k = 0; k < 3; ++k) tri.id[k] = triangles[t * 3 + k];
  project_corner<0>(tri, vertices, P, model_scale, cam, IH, IW);
  project_corner<1>(tri, vertices, P, model_scale, cam, IH, IW);
  project_corner<2>(tri, vertices, P, model_scale, cam, IH, IW);
  double w[3], W;
  const double A = signed_area(tri);
  node_weights(tri, A < 0.0, r, q, w, W);
  const double u0 = w[0] / tri.c3[0], u1 = w[1] / tri.c3[1], u2 = w[2] / tri.c3[2];
  const double U = (u0 + u1) + u2;
  const unsigned char *c0 = colors + (size_t)tri.id[0] * 3, *c1 = colors + (size_t)tri.id[1] * 3, *c2 = colors + (size_t)tri.id[2] * 3;
  *depth = (unsigned short)(key >> 32);
  double s = 1.0;
  if constexpr (LIT) {
    double N[3];
    if (sh.mode == 0) {                                                       // L1, L2: the triangle's normal
      const float *n = sh.normals + t * 3;
#pragma unroll
      for (int j = 0; j < 3; ++j) N[j] = rotated_normal(P, j, n);
    } else {                                                                  // the corners' normals, each turned first; no re-normalising
      const float *n0 = sh.normals + (size_t)tri.id[0] * 3, *n1 = sh.normals + (size_t)tri.id[1] * 3;
      const float *n2 = sh.normals + (size_t)tri.id[2] * 3;
#pragma unroll
      for (int j = 0; j < 3; ++j)
        N[j] = ((u0 * rotated_normal(P, j, n0) + u1 * rotated_normal(P, j, n1)) + u2 * rotated_normal(P, j, n2)) / U;
    }
    if (A > 0.0) { N[0] = -N[0]; N[1] = -N[1]; N[2] = -N[2]; }                // L3: a back face is lit as the side the camera sees
    double c = (N[0] * sh.L[0] + N[1] * sh.L[1]) + N[2] * sh.L[2];            // L4
    c = c > 0.0 ? c : 0.0;                                                    // NaN -> 0
    s = sh.ambient + sh.diffuse * c;                                          // L5
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const double a = ((u0 * (double)c0[ch] + u1 * (double)c1[ch]) + u2 * (double)c2[ch]) / U;
    px[ch] = to_channel(rint(LIT ? a * (s * sh.c[ch]) : a));                  // L6
  }
}

}  // namespace
}  // namespace df
