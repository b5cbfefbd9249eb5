// What the two triangle rasterisers share (cad_raster.hip: one mesh per frame, with holes; cad_scene.hip: several objects per frame with
// occlusion): the pose and triangle records and steps V2..V5 and T2..T7 of df_cad_render_mesh (include/dfusion.h) as device functions.
// Each translation unit gets its own copy; both are built with -ffp-contract=off, so the same code gives the same bits in both.
#pragma once
#include "cad_frame.h"

namespace df {
namespace {

constexpr int RASTER_MAX_BLOCKS = 256;  // triangle blocks per frame: the waves stride over the rest
constexpr int SMALL_NODES = 16;         // node ranges up to this size are walked by the lane that set the triangle up

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

__device__ inline unsigned char to_channel(double v) { return (unsigned char)(v >= 0.0 ? (v <= 255.0 ? v : 255.0) : 0.0); }      // NaN -> 0

}  // namespace
}  // namespace df
