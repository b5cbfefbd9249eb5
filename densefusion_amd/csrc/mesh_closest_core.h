// The per-triangle and per-pair rules of df_mesh_closest (steps M1, M2, Q1, D1..D5 of its comment in include/dfusion.h) as
// __host__ __device__ functions: the kernels of mesh_closest.hip call them per lane, a CPU program can call them per pair (the header
// needs no HIP: a plain C++ compiler sees the functions without the attributes).  fp64 throughout, one rounding per operation in the
// order written here; the file that includes this is built with -ffp-contract=off.
#pragma once
#include <cmath>
#include <limits>

#if defined(__HIPCC__)
#define DF_MC_HD __host__ __device__ inline
#else
#define DF_MC_HD inline
#endif

namespace df {
namespace meshclosest {

// One triangle's record, 32 doubles: what M2 computes, laid out so that a wave reads it from LDS as 16-byte broadcasts.  A dropped
// triangle (M1) is a record of NaNs: every distance to it is NaN and never wins (D4).
struct TriRec {
  double U[3][3];    // A, B, C: the start points of the edges AB, BC, CA
  double e[3][3];    // B - A, C - B, A - C
  double iee[3];     // 1 / |e|^2, or 0
  double e2[3];      // C - A
  double n[3];       // e1 x e2 (e1 = e[0])
  double nn, inn;    // |n|^2 and 1 / |n|^2; nn == 0: no face
  double pad[3];
};
constexpr int REC_DOUBLES = 32;
static_assert(sizeof(TriRec) == REC_DOUBLES * sizeof(double), "TriRec is 32 doubles");

DF_MC_HD double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
DF_MC_HD void cross3(const double *a, const double *b, double *c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// M1: a triangle is kept when its three indices lie in 0..V-1 and are pairwise different
DF_MC_HD bool tri_kept(int i0, int i1, int i2, int V) {
  return i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V && i0 != i1 && i1 != i2 && i0 != i2;
}

// M1 + M2: the record of triangle (i0, i1, i2); nothing is read through a bad index
DF_MC_HD void prepare_tri(const float *vertices, int V, int i0, int i1, int i2, TriRec *r) {
  double *w = reinterpret_cast<double *>(r);
  if (!tri_kept(i0, i1, i2, V)) {
    for (int i = 0; i < REC_DOUBLES; ++i) w[i] = std::numeric_limits<double>::quiet_NaN();
    return;
  }
  const int idx[3] = {i0, i1, i2};
  for (int k = 0; k < 3; ++k)
    for (int j = 0; j < 3; ++j) r->U[k][j] = (double)vertices[3 * (size_t)idx[k] + j];
  for (int k = 0; k < 3; ++k) {
    const int k1 = k == 2 ? 0 : k + 1;
    for (int j = 0; j < 3; ++j) r->e[k][j] = r->U[k1][j] - r->U[k][j];
    const double ee = dot3(r->e[k], r->e[k]);
    r->iee[k] = ee > 0 ? 1.0 / ee : 0.0;
  }
  for (int j = 0; j < 3; ++j) r->e2[j] = r->U[2][j] - r->U[0][j];
  cross3(r->e[0], r->e2, r->n);
  r->nn = dot3(r->n, r->n);
  r->inn = r->nn > 0 ? 1.0 / r->nn : 0.0;
  r->pad[0] = r->pad[1] = r->pad[2] = 0.0;
}

// Q1: q = X p, X a row-major 3 x 4
DF_MC_HD void transform_query(const double *X, const double *p, double *q) {
  for (int j = 0; j < 3; ++j) q[j] = ((X[4 * j] * p[0] + X[4 * j + 1] * p[1]) + X[4 * j + 2] * p[2]) + X[4 * j + 3];
}

// D1: squared distance from q to the segment U + s e, s in [0, 1]; *s_out receives the clamped parameter (a NaN stays a NaN)
DF_MC_HD double segment_d2(const double *U, const double *e, double iee, const double *q, double *s_out) {
  const double w[3] = {q[0] - U[0], q[1] - U[1], q[2] - U[2]};
  double s = dot3(w, e) * iee;
  s = s < 0 ? 0.0 : (s > 1 ? 1.0 : s);
  const double r[3] = {w[0] - s * e[0], w[1] - s * e[1], w[2] - s * e[2]};
  *s_out = s;
  return dot3(r, r);
}

// D2: squared distance from q to the plane of the face where q's foot lies inside it, +inf where it does not or there is no face;
// *h_out receives (q - A) . n
DF_MC_HD double face_d2(const TriRec &r, const double *q, double *h_out) {
  const double w[3] = {q[0] - r.U[0][0], q[1] - r.U[0][1], q[2] - r.U[0][2]};
  double a[3], b[3];
  cross3(r.e[0], w, a);
  cross3(w, r.e2, b);
  const double u = dot3(a, r.n), v = dot3(b, r.n), h = dot3(w, r.n);
  const bool inside = (r.nn > 0) & (u >= 0) & (v >= 0) & (u + v <= r.nn);
  *h_out = h;
  return inside ? (h * h) * r.inn : std::numeric_limits<double>::infinity();
}

// D3: d_t, the first smallest of (AB, BC, CA, face).  A NaN candidate is never taken, so d_t is never a NaN: it is +inf where every
// candidate is a NaN or +inf (a dropped triangle, a NaN query).  Branch-free: every lane has its own query.
DF_MC_HD double tri_d2(const TriRec &r, const double *q) {
  double s, h, d = std::numeric_limits<double>::infinity();
  for (int k = 0; k < 3; ++k) {
    const double dk = segment_d2(r.U[k], r.e[k], r.iee[k], q, &s);
    d = dk < d ? dk : d;
  }
  const double df = face_d2(r, q, &h);
  return df < d ? df : d;
}

// D3 again for the winning triangle, with the closest point of the candidate that gave d_t (c = q where there is none)
DF_MC_HD double tri_closest(const TriRec &r, const double *q, double *c) {
  double s, h, d = std::numeric_limits<double>::infinity();
  c[0] = q[0]; c[1] = q[1]; c[2] = q[2];
  for (int k = 0; k < 3; ++k) {
    const double dk = segment_d2(r.U[k], r.e[k], r.iee[k], q, &s);
    if (dk < d) {
      d = dk;
      for (int j = 0; j < 3; ++j) c[j] = r.U[k][j] + s * r.e[k][j];
    }
  }
  const double df = face_d2(r, q, &h);
  if (df < d) {
    d = df;
    const double g = h * r.inn;
    for (int j = 0; j < 3; ++j) c[j] = q[j] - g * r.n[j];
  }
  return d;
}

// D4: (d, t) replaces the best (bd, bt) when it is smaller, or equal with a lower index; bt < 0 means no winner yet.  The scan walks
// t upwards and needs only `d < bd`; this is the rule by which the partial winners of a split scan meet.
DF_MC_HD bool better(double d, int t, double bd, int bt) { return t >= 0 && (bt < 0 || d < bd || (d == bd && t < bt)); }

}  // namespace meshclosest
}  // namespace df
