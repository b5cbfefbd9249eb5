// The per-node and per-pair rules of df_pose_refine_contour (steps E1..E5 of its comment in include/dfusion.h) as __host__ __device__
// functions: the outline, feature and accumulation kernels of pose_verify.hip call them per lane, a CPU program can call them node by
// node.  The plane term, the tiles and the tree are pose_dense_core.h's, the sums mesh_icp_core.h's `accumulate`, the solve and the update
// its `finish_pass`, all unchanged.  E1..E3 are integer; E4 is fp64, one rounding per operation in the order written here, only + - * /
// appear.  The file that includes this is built with -ffp-contract=off.
#pragma once
#include "pose_dense_core.h"

namespace df {
namespace posecontour {

using meshclosest::cross3;
using meshclosest::dot3;

constexpr int MAX_EDGE_STEP = 65535;
constexpr int MAX_REACH = 64;
constexpr int NONE = -1;                              // a feature or a row's nearest column: no outline node within reach
constexpr int NSTAT = 8;                              // the six columns of df_pose_refine_dense, then the pairs of the first and last pass
enum Stat { ST_FIRST_PAIRS = 6, ST_LAST_PAIRS = 7 };
constexpr int PAIR_TERMS = 2;                         // a pair's terms: along the camera's x axis, then along its y axis
constexpr int STRIP = 256;                            // columns of a row strip of the feature transform's first pass

// A node as E1 and E3 see it: `exists` = inside the window and the frame; `on` (only with exists) = observed (and in the mask), or drawn;
// code = co, or cr
struct Node {
  bool exists, on;
  int code;
};

// E1, E3: c is an outline node when it is on and a neighbour exists that is not on or lies more than edge_step codes behind it
DF_MC_HD bool outline(const Node &c, const Node *nb, int edge_step) {
  if (!c.exists || !c.on) return false;
  for (int k = 0; k < 4; ++k)
    if (nb[k].exists && (!nb[k].on || nb[k].code - c.code > edge_step)) return true;
  return false;
}

// E2 along a row: the outline column nearest to wc among wc - reach .. wc + reach (ties: the lower), or NONE.  flag[i] is the outline
// flag of column first + i and covers every column of 0 .. WW - 1 the search can reach
DF_MC_HD int row_nearest(const unsigned char *flag, int first, int wc, int reach, int WW) {
  for (int d = 0; d <= reach; ++d) {
    if (wc - d >= 0 && flag[wc - d - first]) return wc - d;
    if (wc + d < WW && flag[wc + d - first]) return wc + d;
  }
  return NONE;
}

// E2 along a column: over the rows wr - reach .. wr + reach of the window, the row whose nearest column g gives the smallest
// (wr - rr)^2 + (wc - g)^2 not above reach^2 (ties: the lower row); the slot of that outline node, or NONE.  g: the first pass's plane,
// [WH][WW].  Why this is E2's lowest slot among the nearest: within a row the nearest outline nodes to wc are wc - d and wc + d for one
// d, so every outline node at the smallest distance over the window is some row's nearest column or its mirror wc + d, and row_nearest
// kept the lower of the two; between rows the ascending scan with a strict comparison keeps the lower row; a slot is row-major.
DF_MC_HD int column_nearest(const int *g, int WH, int WW, int wr, int wc, int reach) {
  int best = reach * reach + 1, feat = NONE;
  const int lo = wr - reach > 0 ? wr - reach : 0, hi = wr + reach < WH - 1 ? wr + reach : WH - 1;
  for (int rr = lo; rr <= hi; ++rr) {
    const int gc = g[(size_t)rr * WW + wc];
    if (gc == NONE) continue;
    const int dr = wr - rr, dq = wc - gc, d2 = dr * dr + dq * dq;
    if (d2 < best) { best = d2; feat = (int)((long long)rr * WW + gc); }
  }
  return feat;
}

// E4: the two terms (J, r, d2 = 0) of the pair of the drawn-outline node with rendered code cr and ray ray_c and its feature with the
// observed code co and ray ray_e; X = the pass's model frame.  false, and nothing accumulated by the caller, when one of the fourteen
// numbers is not finite.  term: PAIR_TERMS rows of meshicp::TERM_DOUBLES
DF_MC_HD bool pair_terms(int cr, const double *ray_c, int co, const double *ray_e, double p22, double p23, double cloud_div,
                         const double *X, double contour_scale, double *term) {
  double a[3], x[3];
  posedense::observed_point(cr, ray_c, p22, p23, cloud_div, X, a);
  posedense::observed_point(co, ray_e, p22, p23, cloud_div, X, x);
  const double w[3] = {x[0] - a[0], x[1] - a[1], x[2] - a[2]};
  bool finite = true;
  for (int k = 0; k < PAIR_TERMS; ++k) {
    double *t = term + k * meshicp::TERM_DOUBLES;
    const double n[3] = {X[k], X[4 + k], X[8 + k]};
    cross3(x, n, t);
    for (int e = 0; e < 3; ++e) {
      t[e] = t[e] * contour_scale;
      t[3 + e] = n[e] * contour_scale;
    }
    t[6] = dot3(n, w) * contour_scale;
    t[7] = 0.0;
    for (int e = 0; e < 7; ++e) finite = finite && (t[e] - t[e] == 0.0);
  }
  return finite;
}

// E5: S = P + C entry by entry for A and G (one add each); D is P's
DF_MC_HD void add_sums(const double *P, const double *C, double *S) {
  for (int k = 0; k < meshicp::NSUM - 1; ++k) S[k] = P[k] + C[k];
  S[meshicp::NSUM - 1] = P[meshicp::NSUM - 1];
}

}  // namespace posecontour
}  // namespace df
