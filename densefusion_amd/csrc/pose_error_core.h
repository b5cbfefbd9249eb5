// The per-item rules of df_pose_sym_error (steps E0..E7 of its comment in include/dfusion.h) as __host__ __device__ functions: the kernels
// of pose_error.hip call them, a CPU program can call them item by item (plain C++: a host compiler sees the functions without the
// attributes; item_row below is the whole rule of one item as one loop).  quat_to_mat is mesh_icp_core.h's and the transform is Q1 of
// mesh_closest_core.h, both unchanged.  fp64 throughout, one rounding per operation in the order written here; only + - * / sqrt
// appear, all correctly rounded.  The file that includes this is built with -ffp-contract=off.
#pragma once
#include "mesh_icp_core.h"

namespace df {
namespace poseerr {

using meshclosest::transform_query;

constexpr int MAX_OBJECTS = 64;
enum Out { OUT_STATUS = 0, OUT_MSSD = 1, OUT_MSSD_SYM = 2, OUT_MSPD = 3, OUT_MSPD_SYM = 4, OUT_VERTICES = 5, NOUT = 6 };
enum Status { OK = 0, BAD_ITEM = 1 };

// rows 0, 1 and 3 of the projection matrix (V3 of df_cad_render_mesh reads no other) and the image size
struct View {
  double p0[4], p1[4], p3[4];
  double ih, iw;                        // (double)IH, (double)IW
};

// E0: the object is unknown, or it owns no vertex or no symmetry.  begin arrays hold O + 1 entries.
DF_MC_HD bool item_bad(int o, int O, const int *vertex_begin, const int *sym_begin) {
  if (o < 0 || o >= O) return true;     // nothing is read through a bad object
  return vertex_begin[o + 1] <= vertex_begin[o] || sym_begin[o + 1] <= sym_begin[o];
}

// E1: [R | t] of a pose (q wxyz, t) as a row-major 3 x 4
DF_MC_HD void pose_matrix(const double *pose, double *M) {
  double R[9];
  meshicp::quat_to_mat(pose, R);
  for (int j = 0; j < 3; ++j) {
    M[4 * j] = R[3 * j]; M[4 * j + 1] = R[3 * j + 1]; M[4 * j + 2] = R[3 * j + 2];
    M[4 * j + 3] = pose[4 + j];
  }
}

// E2: G = M o S for two row-major 3 x 4 (a point goes through S first): the rotation part by rows of M times columns of S, the
// translation column with M's own added last
DF_MC_HD void compose(const double *M, const double *S, double *G) {
  for (int j = 0; j < 3; ++j) {
    for (int k = 0; k < 4; ++k) G[4 * j + k] = (M[4 * j] * S[k] + M[4 * j + 1] * S[4 + k]) + M[4 * j + 2] * S[8 + k];
    G[4 * j + 3] = G[4 * j + 3] + M[4 * j + 3];
  }
}

// E4: |a - b|^2; a value that is not finite counts as +inf
DF_MC_HD double dist2(const double *a, const double *b) {
  const double d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
  const double d2 = meshclosest::dot3(d, d);
  return d2 < std::numeric_limits<double>::infinity() ? d2 : std::numeric_limits<double>::infinity();
}

// E5: the pixel coordinates (column u, row v) of the camera-frame point p by V3, V4 of df_cad_render_mesh with one reciprocal in the
// place of the two divisions, not rounded to a node.  A point at or behind the camera plane (c3 > 0 fails) gets u = NaN, so that every
// pixel distance taken from it is not finite.
DF_MC_HD void project(const View &w, const double *p, double *uv) {
  const double c0 = ((w.p0[0] * p[0] + w.p0[1] * p[1]) + w.p0[2] * p[2]) + w.p0[3];
  const double c1 = ((w.p1[0] * p[0] + w.p1[1] * p[1]) + w.p1[2] * p[2]) + w.p1[3];
  const double c3 = ((w.p3[0] * p[0] + w.p3[1] * p[1]) + w.p3[2] * p[2]) + w.p3[3];
  const double i = 1.0 / c3;
  const double u = (((c0 * i) + 1.0) * w.iw) * 0.5;
  uv[0] = c3 > 0.0 ? u : std::numeric_limits<double>::quiet_NaN();
  uv[1] = ((1.0 - (c1 * i)) * w.ih) * 0.5;
}

// E6: the squared pixel distance; not finite counts as +inf
DF_MC_HD double pixel2(const double *a, const double *b) {
  const double du = a[0] - b[0], dv = a[1] - b[1];
  const double e2 = du * du + dv * dv;
  return e2 < std::numeric_limits<double>::infinity() ? e2 : std::numeric_limits<double>::infinity();
}

// E3..E6 for one vertex x (fp32, widened exactly) whose estimate-side point pe and pixel ue are known, against the composed G
DF_MC_HD void pair_errors(const View &w, const double *G, const double *x, const double *pe, const double *ue, double *d2, double *e2) {
  double pg[3], ug[2];
  transform_query(G, x, pg);
  *d2 = dist2(pe, pg);
  project(w, pg, ug);
  *e2 = pixel2(ue, ug);
}

// E7 after the reduction: the row of an item from the smallest of the per-symmetry maxima
DF_MC_HD void write_row(double dmin, int ds, double emin, int es, int nv, double *row) {
  row[OUT_STATUS] = (double)OK;
  row[OUT_MSSD] = sqrt(dmin); row[OUT_MSSD_SYM] = (double)ds;
  row[OUT_MSPD] = sqrt(emin); row[OUT_MSPD_SYM] = (double)es;
  row[OUT_VERTICES] = (double)nv;
}

DF_MC_HD void bad_row(double *row) {
  for (int e = 0; e < NOUT; ++e) row[e] = 0.0;
  row[OUT_STATUS] = (double)BAD_ITEM;
}

// The whole rule of one item, one pair at a time: vertices [V][3] and sym [NS][12] are the call's arrays, `row` takes NOUT doubles.
DF_MC_HD void item_row(const float *vertices, const int *vertex_begin, const double *sym, const int *sym_begin, int O, int o,
                       const double *pose_est, const double *pose_gt, const View &w, double *row) {
  if (item_bad(o, O, vertex_begin, sym_begin)) { bad_row(row); return; }
  const int v0 = vertex_begin[o], nv = vertex_begin[o + 1] - v0, s0 = sym_begin[o], ns = sym_begin[o + 1] - s0;
  double E[12], M[12], G[12];
  pose_matrix(pose_est, E);
  pose_matrix(pose_gt, M);
  const double inf = std::numeric_limits<double>::infinity();
  double dmin = inf, emin = inf;
  int ds = 0, es = 0;
  for (int s = 0; s < ns; ++s) {
    compose(M, sym + 12 * (size_t)(s0 + s), G);
    double dmax = 0.0, emax = 0.0;
    for (int v = 0; v < nv; ++v) {
      const float *xf = vertices + 3 * (size_t)(v0 + v);
      const double x[3] = {(double)xf[0], (double)xf[1], (double)xf[2]};
      double pe[3], ue[2], d2, e2;
      transform_query(E, x, pe);
      project(w, pe, ue);
      pair_errors(w, G, x, pe, ue, &d2, &e2);
      dmax = d2 > dmax ? d2 : dmax;
      emax = e2 > emax ? e2 : emax;
    }
    if (s == 0 || dmax < dmin) { dmin = dmax; ds = s; }      // ties go to the lowest s
    if (s == 0 || emax < emin) { emin = emax; es = s; }
  }
  write_row(dmin, ds, emin, es, nv, row);
}

}  // namespace poseerr
}  // namespace df
