// The per-item rules of df_mesh_icp (steps S0, I1..I10 of its comment in include/dfusion.h) as __host__ __device__ functions: the kernels of
// mesh_icp.hip call them, a CPU program can call them item by item (plain C++: a host compiler sees the functions without the
// attributes).  The closest point is mesh_closest_core.h's, unchanged.  fp64 throughout, one rounding per operation in the order written
// here; only + - * / sqrt appear, all correctly rounded.  The file that includes this is built with -ffp-contract=off.
#pragma once
#include "mesh_closest_core.h"

namespace df {
namespace meshicp {

using meshclosest::cross3;
using meshclosest::dot3;
using meshclosest::TriRec;

constexpr int MAX_OBJECTS = 64;
constexpr int MAX_ITERS = 64;
constexpr int MIN_INLIERS = 6;
constexpr double PIVOT_REL = 1.0 / 1099511627776.0;   // 2^-40, exact: a pivot <= PIVOT_REL * (largest diagonal entry) is `degenerate`
constexpr int LANES = 256;                            // the lanes of the accumulation (I6): lane l sums the points l, l + 256, ...
constexpr int WAVE = 64;
constexpr int NSUM = 28;                              // 21 entries of A (a <= b, a-major), 6 of sum(r J), sum(d2)
enum Status { OK = 0, FEW = 1, DEGENERATE = 2, BAD_OBJECT = 3 };
enum Stat { ST_STATUS = 0, ST_FIRST_INL = 1, ST_FIRST_RMS = 2, ST_LAST_INL = 3, ST_LAST_RMS = 4, ST_STEPS = 5, NSTAT = 6 };
constexpr int TERM_DOUBLES = 8;                       // a point's terms: J (6), r, d2

// the quaternion -> rotation formula of the pose loop (pose.hip) and of df_add_metric; M row-major
DF_MC_HD void quat_to_mat(const double *q, double *M) {
  const double n = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
  if (n < 2.220446049250313e-16 * 4.0) {
    for (int i = 0; i < 9; ++i) M[i] = (i % 4 == 0) ? 1.0 : 0.0;
    return;
  }
  const double s = sqrt(2.0 / n);
  const double w = q[0] * s, x = q[1] * s, y = q[2] * s, z = q[3] * s;
  M[0] = (1.0 - y * y) - z * z; M[1] = x * y - z * w;         M[2] = x * z + y * w;
  M[3] = x * y + z * w;         M[4] = (1.0 - x * x) - z * z; M[5] = y * z - x * w;
  M[6] = x * z - y * w;         M[7] = y * z + x * w;         M[8] = (1.0 - x * x) - y * y;
}

// q / |q| with the sign rule (w < 0: every component negated).  A zero or NaN quaternion becomes NaNs; such an item finds no inlier.
DF_MC_HD void normalise_quat(double *q) {
  const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  for (int e = 0; e < 4; ++e) q[e] = q[e] / n;
  if (q[0] < 0.0)
    for (int e = 0; e < 4; ++e) q[e] = -q[e];
}

// I2: X = [R^T | o], o = -(R^T t) the camera centre in the model frame: x = X p by Q1 of df_mesh_closest (meshclosest::transform_query)
DF_MC_HD void model_frame(const double *pose, double *X) {
  double R[9];
  quat_to_mat(pose, R);
  const double *t = pose + 4;
  for (int j = 0; j < 3; ++j) {
    X[4 * j] = R[j]; X[4 * j + 1] = R[3 + j]; X[4 * j + 2] = R[6 + j];
    X[4 * j + 3] = -((R[j] * t[0] + R[3 + j] * t[1]) + R[6 + j] * t[2]);
  }
}

// I4, I5: the inlier test and the terms (J, r, d2) of the point x whose winner is (r, tri, d2); md2 = max_dist^2; o = the camera
// centre in the model frame.  A point that is no inlier gets zeros.
DF_MC_HD bool point_terms(const TriRec *rec, int tri, double d2, const double *x, double md2, int cull, const double *o, double *term) {
  for (int e = 0; e < TERM_DOUBLES; ++e) term[e] = 0.0;
  if (tri < 0 || !(d2 <= md2) || !(d2 < std::numeric_limits<double>::infinity())) return false;
  const TriRec &r = rec[tri];
  if (!(r.nn > 0)) return false;
  double c[3];
  meshclosest::tri_closest(r, x, c);
  if (cull) {
    const double v[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
    if (!(dot3(r.n, v) > 0)) return false;
  }
  const double sn = sqrt(r.nn);
  const double nh[3] = {r.n[0] / sn, r.n[1] / sn, r.n[2] / sn};
  const double w[3] = {x[0] - c[0], x[1] - c[1], x[2] - c[2]};
  cross3(x, nh, term);
  term[3] = nh[0]; term[4] = nh[1]; term[5] = nh[2];
  term[6] = dot3(nh, w);
  term[7] = d2;
  return true;
}

// I6, per lane: acc (NSUM doubles) += the sums of one inlier's terms
DF_MC_HD void accumulate(const double *term, double *acc) {
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) acc[k++] += term[a] * term[b];
  for (int a = 0; a < 6; ++a) acc[21 + a] += term[6] * term[a];
  acc[27] += term[7];
}

DF_MC_HD double rms_of(double sd2, int count) { return count > 0 ? sqrt(sd2 / (double)count) : 0.0; }

// I8: Cholesky A = L L^T of the 6 x 6 whose upper triangle is sums[0..20] (a <= b, a-major), then L y = g, L^T z = y with
// g = -sums[21..26].  false: a pivot <= PIVOT_REL * the largest diagonal entry (or a NaN); z is then not written.
DF_MC_HD bool solve6(const double *sums, double *z) {
  double A[6][6], L[6][6], y[6];
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) { A[a][b] = sums[k]; A[b][a] = sums[k]; ++k; }
  double dmax = A[0][0];
  for (int a = 1; a < 6; ++a) dmax = A[a][a] > dmax ? A[a][a] : dmax;
  const double thr = PIVOT_REL * dmax;
  for (int j = 0; j < 6; ++j) {
    double s = A[j][j];
    for (int m = 0; m < j; ++m) s = s - L[j][m] * L[j][m];
    if (!(s > thr)) return false;
    L[j][j] = sqrt(s);
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
      for (int m = 0; m < j; ++m) v = v - L[i][m] * L[j][m];
      L[i][j] = v / L[j][j];
    }
  }
  for (int i = 0; i < 6; ++i) {
    double v = -sums[21 + i];
    for (int m = 0; m < i; ++m) v = v - L[i][m] * y[m];
    y[i] = v / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
    for (int m = i + 1; m < 6; ++m) v = v - L[m][i] * z[m];
    z[i] = v / L[i][i];
  }
  return true;
}

// I9: pose (q, t) <- the step z = (omega, dt): dq = (1, omega / 2) / |.|, q <- normalise(q (x) conj(dq)), t <- t - R(q_new) dt
DF_MC_HD void update_pose(double *pose, const double *z) {
  const double h[3] = {z[0] * 0.5, z[1] * 0.5, z[2] * 0.5};
  const double m = sqrt(((1.0 + h[0] * h[0]) + h[1] * h[1]) + h[2] * h[2]);
  const double cw = 1.0 / m, cx = -(h[0] / m), cy = -(h[1] / m), cz = -(h[2] / m);
  const double qw = pose[0], qx = pose[1], qy = pose[2], qz = pose[3];
  double q[4];
  q[0] = ((qw * cw - qx * cx) - qy * cy) - qz * cz;
  q[1] = ((qw * cx + qx * cw) + qy * cz) - qz * cy;
  q[2] = ((qw * cy - qx * cz) + qy * cw) + qz * cx;
  q[3] = ((qw * cz + qx * cy) - qy * cx) + qz * cw;
  normalise_quat(q);
  double R[9];
  quat_to_mat(q, R);
  for (int e = 0; e < 4; ++e) pose[e] = q[e];
  for (int j = 0; j < 3; ++j) pose[4 + j] = pose[4 + j] - ((R[3 * j] * z[3] + R[3 * j + 1] * z[4]) + R[3 * j + 2] * z[5]);
}

// I6..I9 after the reduction, for one item and pass: `sums` (NSUM) and `count` are the pass's totals.  Writes the pass's inliers and rms
// to stats (first pass: also as the first), and with `solve` takes the step or freezes the item.
DF_MC_HD void finish_pass(const double *sums, int count, int pass, int solve, double *pose, double *stats) {
  const double rms = rms_of(sums[27], count);
  if (pass == 0) { stats[ST_FIRST_INL] = (double)count; stats[ST_FIRST_RMS] = rms; }
  stats[ST_LAST_INL] = (double)count;
  stats[ST_LAST_RMS] = rms;
  if (!solve) return;
  if (count < MIN_INLIERS) { stats[ST_STATUS] = (double)FEW; return; }
  double z[6];
  if (!solve6(sums, z)) { stats[ST_STATUS] = (double)DEGENERATE; return; }
  update_pose(pose, z);
  stats[ST_STEPS] = stats[ST_STEPS] + 1.0;
}

}  // namespace meshicp
}  // namespace df
