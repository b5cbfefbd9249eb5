// The per-node and per-tile rules of df_pose_refine_dense (steps D2..D5 of its comment in include/dfusion.h) as __host__ __device__
// functions: the accumulation kernel of pose_verify.hip calls them per lane, a CPU program can call them node by node.  The draw (D1) is
// df_pose_verify's raster pass, the sums are mesh_icp_core.h's `accumulate`, the solve and the update its `finish_pass`, all unchanged.
// fp64, one rounding per operation in the order written here; only + - * / sqrt appear.  The file that includes this is built with
// -ffp-contract=off.
#pragma once
#include "pose_vsd_core.h"

namespace df {
namespace posedense {

using meshclosest::cross3;
using meshclosest::dot3;

constexpr int MAX_GATE = 65535;
constexpr int TILE = 2048;                            // window slots per tile (D5): 8 sweeps of the 256 lanes
constexpr int SWEEPS = TILE / meshicp::LANES;
constexpr int NPART = meshicp::NSUM + 1;              // a tile's total: the 28 sums of I6 and the count (exact in fp64)
constexpr int PART_DOUBLES = 32;                      // a (item, tile) row of the scratch
constexpr int FRAME_DOUBLES = 16;                     // per item in the scratch: X of I2 (12), the vertex factor (1), 3 unused
static_assert(TILE % meshicp::LANES == 0 && NPART <= PART_DOUBLES, "a tile is whole sweeps; a row holds a total");

// the tiles of a window of `slots` slots: tile i holds the slots i * TILE .. i * TILE + TILE - 1 that are below `slots`
DF_MC_HD int tile_count(long long slots) { return (int)((slots + TILE - 1) / TILE); }

// D2: the whole gating rule, all integer.  cr = the rendered code or NO_CODE; co = the observed code; m is read only with a mask
DF_MC_HD bool candidate(int cr, int co, int gate, bool has_mask, bool m) {
  if (cr == poseverify::NO_CODE || co == poseverify::NO_OBSERVATION) return false;
  const int d = co > cr ? co - cr : cr - co;
  return d <= gate && (!has_mask || m);
}

// D3: the depth a code stands for, S2's formula with its sign: negative in front of the camera
DF_MC_HD double code_depth(int c, double p22, double p23) { return -p23 / (p22 + (1.0 - (double)c / 65534.0)); }

// D3: the observed point of a node in the model frame; X = model_frame of the pose (I2)
DF_MC_HD void observed_point(int co, const double *ray, double p22, double p23, double cloud_div, const double *X, double *x) {
  const double z = code_depth(co, p22, p23);
  const double p[3] = {(ray[0] * z) / cloud_div, (ray[1] * z) / cloud_div, (ray[2] * z) / cloud_div};
  meshclosest::transform_query(X, p, x);
}

// the factor from file units to the units of the poses, once per item
DF_MC_HD double vertex_factor(double model_scale, double cloud_div) { return model_scale / cloud_div; }

// D4: the terms (J, r, d2) of the observed point x against the plane of the triangle with the fp32 vertices va, vb, vc (file units);
// false, and zeros, when the triangle has no face or a number is not finite
DF_MC_HD bool plane_terms(const float *va, const float *vb, const float *vc, double factor, const double *x, double *term) {
  for (int e = 0; e < meshicp::TERM_DOUBLES; ++e) term[e] = 0.0;
  double a[3], e1[3], e2[3], n[3];
  for (int j = 0; j < 3; ++j) {
    a[j] = (double)va[j] * factor;
    e1[j] = (double)vb[j] * factor - a[j];
    e2[j] = (double)vc[j] * factor - a[j];
  }
  cross3(e1, e2, n);
  const double nn = dot3(n, n);
  if (!(nn > 0)) return false;
  const double sn = sqrt(nn);
  const double nh[3] = {n[0] / sn, n[1] / sn, n[2] / sn};
  const double w[3] = {x[0] - a[0], x[1] - a[1], x[2] - a[2]};
  double t[meshicp::TERM_DOUBLES];
  cross3(x, nh, t);
  t[3] = nh[0]; t[4] = nh[1]; t[5] = nh[2];
  t[6] = dot3(nh, w);
  t[7] = t[6] * t[6];
  for (int e = 0; e < meshicp::TERM_DOUBLES; ++e)
    if (!(t[e] - t[e] == 0.0)) return false;            // an infinity or a NaN
  for (int e = 0; e < meshicp::TERM_DOUBLES; ++e) term[e] = t[e];
  return true;
}

// D2..D4 for one existing node, added to a lane's accumulators (acc: NSUM doubles; *count): a CPU program's form of a lane's step
DF_MC_HD void node_step(unsigned long long key, int co, bool has_mask, bool m, int gate, const double *ray, double p22, double p23,
                        double cloud_div, const double *X, double factor, const float *vertices, const int *triangles, double *acc,
                        int *count) {
  if (!candidate(poseverify::key_code(key), co, gate, has_mask, m)) return;
  const size_t t = (size_t)(key & 0xffffffffull);
  const int i0 = triangles[3 * t], i1 = triangles[3 * t + 1], i2 = triangles[3 * t + 2];
  double x[3], term[meshicp::TERM_DOUBLES];
  observed_point(co, ray, p22, p23, cloud_div, X, x);
  if (!plane_terms(vertices + 3 * (size_t)i0, vertices + 3 * (size_t)i1, vertices + 3 * (size_t)i2, factor, x, term)) return;
  meshicp::accumulate(term, acc);
  *count += 1;
}

// D5 within a tile: the lane that takes slot s, and the order of I6: in each group of 64 lanes a binary tree (step 32, 16, .., 1: lane
// l < step adds lane l + step), the four group totals as (T0 + T1) + (T2 + T3).  lanes: LANES rows of NPART doubles, overwritten
DF_MC_HD int slot_lane(int s) { return s % meshicp::LANES; }
DF_MC_HD void tile_total(double *lanes, double *total) {
  for (int g = 0; g < meshicp::LANES / meshicp::WAVE; ++g)
    for (int step = meshicp::WAVE / 2; step >= 1; step >>= 1)
      for (int l = 0; l < step; ++l)
        for (int k = 0; k < NPART; ++k) {
          double *row = lanes + (size_t)(g * meshicp::WAVE + l) * NPART;
          row[k] = row[k] + row[(size_t)step * NPART + k];
        }
  const size_t G = (size_t)meshicp::WAVE * NPART;
  for (int k = 0; k < NPART; ++k) total[k] = (lanes[k] + lanes[G + k]) + (lanes[2 * G + k] + lanes[3 * G + k]);
}

}  // namespace posedense
}  // namespace df
