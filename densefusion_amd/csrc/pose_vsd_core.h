// The per-node rules of df_pose_vsd (steps S1..S4 of its comment in include/dfusion.h) as __host__ __device__ functions: the score kernel
// of pose_verify.hip calls them, a CPU program can call them node by node.  fp64, one rounding per operation in the order written here;
// only + - * / sqrt appear.  The file that includes this is built with -ffp-contract=off.
#pragma once
#include "pose_verify_core.h"

namespace df {
namespace posevsd {

constexpr int MAX_TAU = 16;
enum Stat { ST_STATUS = 0, ST_UNION = 1, ST_INTER = 2, ST_RENDERED_E = 3, ST_BAD = 4 };   // a row holds ST_BAD + NT entries
constexpr int TABLE_DOUBLES = 1 + MAX_TAU;            // per object: delta, tau[0..15]

// S1: the length of the node's back-projection ray at unit depth (the loader's ray map has z = 1)
DF_MC_HD double ray_length(const double *ray) { return sqrt((ray[0] * ray[0] + ray[1] * ray[1]) + ray[2] * ray[2]); }

// S2: the distance from the camera of the surface a code stands for at a node of ray length rho: the loader's inverse of T6, whose z is
// negative in front of the camera, taken by magnitude
DF_MC_HD double code_distance(int c, double p22, double p23, double rho) {
  const double z = -p23 / (p22 + (1.0 - (double)c / 65534.0));
  return (z < 0.0 ? -z : z) * rho;
}

// S3: visibility of the two renders at a node (codes ce, cg or NO_CODE; co the observed code) and, where both are visible, their gap
DF_MC_HD void node_visibility(int ce, int cg, int co, double p22, double p23, double rho, double delta, bool *vis_e, bool *vis_g,
                              double *gap) {
  const bool re = ce != poseverify::NO_CODE, rg = cg != poseverify::NO_CODE, seen = co != poseverify::NO_OBSERVATION;
  const double De = code_distance(re ? ce : 0, p22, p23, rho), Dg = code_distance(rg ? cg : 0, p22, p23, rho);
  const double Do = code_distance(seen ? co : 0, p22, p23, rho);
  *vis_g = rg && (!seen || Dg - Do <= delta);
  *vis_e = re && (!seen || De - Do <= delta || *vis_g);
  const double d = Dg - De;
  *gap = d < 0.0 ? -d : d;
}

// S3, S4 for one node, added to a stats row of ST_BAD + NT entries (a CPU program's form of the score pass)
DF_MC_HD void score_node(unsigned long long key_e, unsigned long long key_g, int co, const double *ray, double p22, double p23, double delta,
                         const double *tau, int NT, long long *stats) {
  bool ve, vg;
  double gap;
  const int ce = poseverify::key_code(key_e), cg = poseverify::key_code(key_g);
  node_visibility(ce, cg, co, p22, p23, ray_length(ray), delta, &ve, &vg, &gap);
  stats[ST_UNION] += ve || vg;
  stats[ST_INTER] += ve && vg;
  stats[ST_RENDERED_E] += ce != poseverify::NO_CODE;
  for (int k = 0; k < NT; ++k) stats[ST_BAD + k] += ve && vg && gap >= tau[k];
}

}  // namespace posevsd
}  // namespace df
