// The per-item and per-node rules of df_pose_verify (steps P0, P1 and P3 of its comment in include/dfusion.h) as __host__ __device__
// functions: the kernels of pose_verify.hip call them, a CPU program can call them node by node (plain C++: a host compiler sees the
// functions without the attributes).  The score is integer throughout; the pose is mesh_icp_core.h's quat_to_mat, unchanged, and one
// fp64 multiply per translation component.  The file that includes this is built with -ffp-contract=off.
#pragma once
#include "mesh_icp_core.h"

namespace df {
namespace poseverify {

constexpr int MAX_OBJECTS = 64;
constexpr int ITEM_INTS = 6;
enum Item { IT_FRAME = 0, IT_OBJECT = 1, IT_R0 = 2, IT_C0 = 3, IT_MASK_FRAME = 4, IT_MASK_VALUE = 5 };
enum Stat {
  ST_STATUS = 0, ST_RENDERED = 1, ST_AGREE = 2, ST_FRONT = 3, ST_BEHIND = 4, ST_MISSING = 5, ST_MASK = 6, ST_MASK_OBSERVED = 7,
  ST_UNEXPLAINED = 8, ST_SUM_ABS = 9, ST_TRIANGLES = 10, ST_CUT = 11, NSTAT = 12
};
enum Class { NOT_RENDERED = 0, MISSING = 1, AGREE = 2, FRONT = 3, BEHIND = 4 };
constexpr int NO_OBSERVATION = 65535;                 // the horizon of the depth frames: the sensor saw nothing
constexpr int NO_CODE = -1;                           // the node's key was never taken
constexpr unsigned long long NO_KEY = ~0ull;

// P0: nothing is read through such a record
DF_MC_HD bool item_bad(const int *item, int F, int O, bool has_mask, int NM) {
  return item[IT_FRAME] < 0 || item[IT_FRAME] >= F || item[IT_OBJECT] < 0 || item[IT_OBJECT] >= O ||
         (has_mask && (item[IT_MASK_FRAME] < 0 || item[IT_MASK_FRAME] >= NM));
}

// P1: [R | t], row-major 3 x 4, from pose = (q wxyz, t) and cloud_div
DF_MC_HD void pose_matrix(const double *pose, double cloud_div, double *M) {
  double R[9];
  meshicp::quat_to_mat(pose, R);
  for (int j = 0; j < 3; ++j) {
    M[4 * j] = R[3 * j]; M[4 * j + 1] = R[3 * j + 1]; M[4 * j + 2] = R[3 * j + 2];
    M[4 * j + 3] = pose[4 + j] * cloud_div;
  }
}

// The rows (lo[0] .. hi[0]) and columns (lo[1] .. hi[1]) of window and frame together; empty when hi < lo.  r0 + WH - 1 is taken in
// 64 bits: a corner near INT_MAX does not wrap.
DF_MC_HD void window_nodes(int r0, int c0, int WH, int WW, int IH, int IW, int *lo, int *hi) {
  const long long r1 = (long long)r0 + WH - 1, c1 = (long long)c0 + WW - 1;
  lo[0] = r0 > 0 ? r0 : 0; lo[1] = c0 > 0 ? c0 : 0;
  hi[0] = (int)(r1 < IH - 1 ? r1 : IH - 1); hi[1] = (int)(c1 < IW - 1 ? c1 : IW - 1);
  if (r1 < 0) hi[0] = -1;
  if (c1 < 0) hi[1] = -1;
}

// window slot s = wr * WW + wc (0 <= s < WH * WW; key index of item b: b * WH * WW + s) -> the node (r, q) = (r0 + wr, c0 + wc);
// false when the node is outside the frame and so does not exist
DF_MC_HD bool slot_node(int s, int r0, int c0, int WW, int IH, int IW, int *r, int *q) {
  const int wr = s / WW, wc = s - wr * WW;
  const long long rr = (long long)r0 + wr, qq = (long long)c0 + wc;
  if (rr < 0 || rr >= IH || qq < 0 || qq >= IW) return false;
  *r = (int)rr; *q = (int)qq;
  return true;
}

// the inverse, for a node inside the window
DF_MC_HD long long node_slot(int r, int q, int r0, int c0, int WW) { return ((long long)r - r0) * WW + ((long long)q - c0); }

// the code of a key (T7: code << 32 | triangle), NO_CODE when the key was never taken
DF_MC_HD int key_code(unsigned long long key) { return key == NO_KEY ? NO_CODE : (int)(key >> 32); }

// P3: the class of a node with rendered code cr (or NO_CODE) under the observed code co
DF_MC_HD int classify(int cr, int co, int tol) {
  if (cr == NO_CODE) return NOT_RENDERED;
  if (co == NO_OBSERVATION) return MISSING;
  if (co < cr - tol) return FRONT;
  if (co > cr + tol) return BEHIND;
  return AGREE;
}

// P3: a mask node that was observed and that the model does not account for
DF_MC_HD bool unexplained(bool m, int co, int cls) { return m && co != NO_OBSERVATION && (cls == NOT_RENDERED || cls == FRONT); }

// P3 for one node, added to a stats row (a CPU program's form of the score pass; the kernel counts the same predicates per wave)
DF_MC_HD void score_node(unsigned long long key, int co, bool m, int tol, long long *stats) {
  const int cr = key_code(key);
  const int cls = classify(cr, co, tol);
  stats[ST_RENDERED] += cls != NOT_RENDERED;
  stats[ST_AGREE] += cls == AGREE;
  stats[ST_FRONT] += cls == FRONT;
  stats[ST_BEHIND] += cls == BEHIND;
  stats[ST_MISSING] += cls == MISSING;
  stats[ST_MASK] += m;
  stats[ST_MASK_OBSERVED] += m && co != NO_OBSERVATION;
  stats[ST_UNEXPLAINED] += unexplained(m, co, cls);
  if (cls == AGREE) stats[ST_SUM_ABS] += co > cr ? co - cr : cr - co;
}

}  // namespace poseverify
}  // namespace df
