// The rules of df_pose_ppf and df_ppf_model_build (steps F1..F3, L1..L2, N1..N2, V1..V3, H1..H3, C1..C3 of their comment in
// include/dfusion.h) as __host__ __device__ functions: the model builder (host) and the kernels of pose_ppf.hip call the very same pair
// feature, so model and scene are never quantised differently; a CPU program can call them pair by pair.  fp64, one rounding per
// operation in the order written here; only + - * / sqrt, comparisons and integer arithmetic appear: every angle is binned by its
// cosine against a table the host hands over.  The file that includes this is built with -ffp-contract=off.
#pragma once
#include "pose_dense_core.h"

namespace df {
namespace poseppf {

using meshclosest::cross3;
using meshclosest::dot3;

constexpr int MAX_OBJECTS = 64;
constexpr int MAX_ND = 64, MAX_NANG = 32, MAX_NA = 64;
constexpr int MIN_MODEL_POINTS = 2, MAX_MODEL_POINTS = 1024;
constexpr int MAX_ACC_BYTES = 150 * 1024;             // an accumulator [NM_o][NA] of uint32 lives in the LDS of one compute unit
constexpr int MAX_GRID = 16384, MAX_REFS = 4096, MAX_K = 16, MAX_STEP = 64, MAX_REACH = 8, MAX_GATE = 65535;
constexpr int HYP_DOUBLES = 8;                        // q (4), t (3), votes
constexpr int SCENE_DOUBLES = 8;                      // per grid node in the scratch: p (3), nh (3), usable (1.0 or 0.0), unused
constexpr int ROW_DOUBLES = 20;                       // per (item, reference) in the scratch: the hypothesis (8), R of its q (9), 3 unused
constexpr int NSTAT = 4;
enum Stat { ST_STATUS = 0, ST_USABLE = 1, ST_HYPOTHESES = 2, ST_CLUSTERS = 3 };
enum Status { OK = 0, NO_HYPOTHESIS = 1, BAD_ITEM = 3 };
constexpr double FLIP_EPS = 1.0 / 1048576.0;          // 2^-20, exact: below it 1 + n_x is too small to divide by (L1)

// the host's tables and bin counts, a launch argument (1.5 KiB)
struct Tables {
  double ang_cos[MAX_NANG - 1];                       // NANG - 1 boundary cosines, descending
  double alpha_cos[MAX_NA / 2 - 1];                   // NA / 2 - 1 boundary cosines of the upper half turn, descending
  double alpha_cs[MAX_NA][2];                         // (cos, sin) of the NA sector centres
  int ND, NANG, NA;
};

DF_MC_HD bool is_finite(double x) { return x - x == 0.0; }

// F2, V2: the number of the n boundaries that v is <= (the boundaries descend, so this is the bin of the angle whose cosine v is)
DF_MC_HD int bounds_reached(const double *bound, int n, double v) {
  int k = 0;
  for (int i = 0; i < n; ++i) k += v <= bound[i] ? 1 : 0;
  return k;
}

// F1..F3: the key of the oriented pair (p1, n1), (p2, n2), or -1 when the pair is dropped
DF_MC_HD int pair_key(const double *p1, const double *n1, const double *p2, const double *n2, double dist_step, const Tables &tb) {
  const double d[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  const double L = sqrt(dot3(d, d));
  if (!(L > 0.0) || !is_finite(L)) return -1;
  const double fd = L / dist_step;
  if (!(fd < (double)tb.ND)) return -1;
  const double c1 = dot3(d, n1) / L, c2 = dot3(d, n2) / L, c3 = dot3(n1, n2);
  if (c1 != c1 || c2 != c2 || c3 != c3) return -1;
  const int bd = (int)fd;
  const int b1 = bounds_reached(tb.ang_cos, tb.NANG - 1, c1), b2 = bounds_reached(tb.ang_cos, tb.NANG - 1, c2),
            b3 = bounds_reached(tb.ang_cos, tb.NANG - 1, c3);
  return ((bd * tb.NANG + b1) * tb.NANG + b2) * tb.NANG + b3;
}

// L1: the rotation that takes the unit normal n to +x, row-major
DF_MC_HD void frame_rot(const double *n, double *R) {
  const double k = 1.0 + n[0];
  if (k < FLIP_EPS) {
    R[0] = -1.0; R[1] = 0.0; R[2] = 0.0; R[3] = 0.0; R[4] = -1.0; R[5] = 0.0; R[6] = 0.0; R[7] = 0.0; R[8] = 1.0;
    return;
  }
  const double yz = -((n[1] * n[2]) / k);
  R[0] = 1.0 - (n[1] * n[1] + n[2] * n[2]) / k; R[1] = n[1];                    R[2] = n[2];
  R[3] = -n[1];                                 R[4] = 1.0 - (n[1] * n[1]) / k; R[5] = yz;
  R[6] = -n[2];                                 R[7] = yz;                      R[8] = 1.0 - (n[2] * n[2]) / k;
}

// L2: the angle of q about the normal of the frame (R, p) as the unit vector cs = (c, s); false when q lies on the axis or a number is
// not finite
DF_MC_HD bool frame_angle(const double *R, const double *p, const double *q, double *cs) {
  const double d[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
  const double y = dot3(R + 3, d), z = dot3(R + 6, d);
  const double mm = sqrt(y * y + z * z);
  if (!(mm > 0.0) || !is_finite(mm)) return false;
  cs[0] = y / mm;
  cs[1] = -z / mm;
  return true;
}

// V2: the sector among NA of the model angle (cm, sm) less the scene angle (cs, ss)
DF_MC_HD int sector(double cm, double sm, double cs, double ss, const Tables &tb) {
  const double c = cm * cs + sm * ss, s = sm * cs - cm * ss;
  const int j = bounds_reached(tb.alpha_cos, tb.NA / 2 - 1, c);
  return s >= 0.0 ? j : tb.NA - 1 - j;
}

// V3: a cell's count and place as one number whose maximum is the winner: the largest count, then the lowest cell i * NA + bin
DF_MC_HD unsigned long long winner_key(unsigned count, int cell) { return ((unsigned long long)count << 32) | (0xffffffffu - (unsigned)cell); }
DF_MC_HD unsigned winner_count(unsigned long long key) { return (unsigned)(key >> 32); }
DF_MC_HD int winner_cell(unsigned long long key) { return (int)(0xffffffffu - (unsigned)(key & 0xffffffffull)); }

// N1: the point a code stands for in the camera frame, in the units of the poses: D3 of df_pose_refine_dense before its transform
DF_MC_HD void scene_point(int co, const double *ray, double p22, double p23, double cloud_div, double *p) {
  const double z = posedense::code_depth(co, p22, p23);
  p[0] = (ray[0] * z) / cloud_div; p[1] = (ray[1] * z) / cloud_div; p[2] = (ray[2] * z) / cloud_div;
}

// N1: whether the neighbour with code cn of a usable node with code co counts (its being in the frame and masked in is the caller's)
DF_MC_HD bool neighbour_counts(int cn, int co, int gate) {
  if (cn == poseverify::NO_OBSERVATION) return false;
  const int d = cn > co ? cn - co : co - cn;
  return d <= gate;
}

// N2: the unit normal at p from its neighbours along the columns (xm at -reach, xp at +reach) and along the rows (ym, yp); h* say
// which of them count.  false: no normal
DF_MC_HD bool scene_normal(const double *p, const double *xm, bool hxm, const double *xp, bool hxp, const double *ym, bool hym,
                           const double *yp, bool hyp, double *nh) {
  if (!(hxm || hxp) || !(hym || hyp)) return false;
  const double *xa = hxp ? xp : p, *xb = hxm ? xm : p, *ya = hyp ? yp : p, *yb = hym ? ym : p;
  const double dx[3] = {xa[0] - xb[0], xa[1] - xb[1], xa[2] - xb[2]}, dy[3] = {ya[0] - yb[0], ya[1] - yb[1], ya[2] - yb[2]};
  double n[3];
  cross3(dx, dy, n);
  const double nn = dot3(n, n);
  if (!(nn > 0.0) || !is_finite(nn)) return false;
  const double sn = sqrt(nn);
  nh[0] = n[0] / sn; nh[1] = n[1] / sn; nh[2] = n[2] / sn;
  if (dot3(nh, p) > 0.0) { nh[0] = -nh[0]; nh[1] = -nh[1]; nh[2] = -nh[2]; }
  return true;
}

// H2: the quaternion (w, x, y, z) of a rotation matrix by the largest of (trace, R00, R11, R22), tried in this order, ties to the earlier
DF_MC_HD void mat_to_quat(const double *R, double *q) {
  const double tr = (R[0] + R[4]) + R[8];
  if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
    const double s = sqrt(1.0 + tr), f = 0.5 / s;
    q[0] = 0.5 * s; q[1] = (R[7] - R[5]) * f; q[2] = (R[2] - R[6]) * f; q[3] = (R[3] - R[1]) * f;
  } else if (R[0] >= R[4] && R[0] >= R[8]) {
    const double s = sqrt(((1.0 + R[0]) - R[4]) - R[8]), f = 0.5 / s;
    q[0] = (R[7] - R[5]) * f; q[1] = 0.5 * s; q[2] = (R[1] + R[3]) * f; q[3] = (R[2] + R[6]) * f;
  } else if (R[4] >= R[8]) {
    const double s = sqrt(((1.0 + R[4]) - R[0]) - R[8]), f = 0.5 / s;
    q[0] = (R[2] - R[6]) * f; q[1] = (R[1] + R[3]) * f; q[2] = 0.5 * s; q[3] = (R[5] + R[7]) * f;
  } else {
    const double s = sqrt(((1.0 + R[8]) - R[0]) - R[4]), f = 0.5 / s;
    q[0] = (R[3] - R[1]) * f; q[1] = (R[2] + R[6]) * f; q[2] = (R[5] + R[7]) * f; q[3] = 0.5 * s;
  }
}

// H1..H3: the pose (q, t) that takes the model point (pm, nm) onto the scene point (ps, ns) and then turns by the angle (ca, sa) about
// the scene normal: T = Ts^-1 Rx Tm
DF_MC_HD void hypothesis_pose(const double *ps, const double *ns, const double *pm, const double *nm, double ca, double sa, double *pose) {
  double Rs[9], Rm[9], A[9], R[9];
  frame_rot(ns, Rs);
  frame_rot(nm, Rm);
  for (int k = 0; k < 3; ++k) {
    A[k] = Rm[k];
    A[3 + k] = ca * Rm[3 + k] - sa * Rm[6 + k];
    A[6 + k] = sa * Rm[3 + k] + ca * Rm[6 + k];
  }
  for (int j = 0; j < 3; ++j)
    for (int k = 0; k < 3; ++k) R[3 * j + k] = (Rs[j] * A[k] + Rs[3 + j] * A[3 + k]) + Rs[6 + j] * A[6 + k];
  mat_to_quat(R, pose);
  meshicp::normalise_quat(pose);
  for (int j = 0; j < 3; ++j) pose[4 + j] = ps[j] - dot3(R + 3 * j, pm);
}

// C2: whether the pose (R, t) lies within the cluster founded by (Rc, tc)
DF_MC_HD bool cluster_near(const double *R, const double *t, const double *Rc, const double *tc, double trace_min, double dist2) {
  const double tr = (dot3(R, Rc) + dot3(R + 3, Rc + 3)) + dot3(R + 6, Rc + 6);
  const double d[3] = {t[0] - tc[0], t[1] - tc[1], t[2] - tc[2]};
  return tr >= trace_min && dot3(d, d) <= dist2;
}

// the grid of a window side and the references of a grid side
DF_MC_HD int grid_side(int w, int step) { return (w + step - 1) / step; }

}  // namespace poseppf
}  // namespace df
