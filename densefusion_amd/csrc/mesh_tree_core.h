// The rules of the bounding-box tree route of df_mesh_closest_tree and df_mesh_icp_tree (include/dfusion.h) as __host__ __device__
// functions: the kernels call `walk` per lane, df_mesh_closest_tree_host and a CPU program call it per query (plain C++: a host compiler
// sees the functions without the attributes).  The tree adds no numerics: a candidate's distance is mesh_closest_core.h's tri_d2 and the
// winner is chosen by its `better`, so the answer is D4's, whatever order the triangles are met in.  Only which triangles are met
// differs, and the rule for that (box_lb, slack2, skip) is proved safe in DESIGN 12l.  fp64, one rounding per operation; the file that
// includes this is built with -ffp-contract=off.
#pragma once
#include "mesh_closest_core.h"

namespace df {
namespace meshtree {

using meshclosest::TriRec;

constexpr int MAX_DEPTH = 32;                          // inner nodes on a path from the root: what a walk's stack must hold
constexpr int LEAF_DEFAULT = 16, LEAF_MAX = 64;        // triangles per leaf: 16 by the ICP bench of DESIGN 12l
constexpr double SLACK_REL = 1.0 / 68719476736.0;      // 2^-36, exact
constexpr double LOOSE_SIN2 = 1.0 / 65536.0;           // 2^-16: a face whose smallest angle has sin^2 below this is not bounded by slack2

// 32 bytes.  The box is the fp32 min / max of the fp32 vertices of the node's triangles, so it widens to fp64 exactly.
// Leaf: b > 0 triangles, order[a] .. order[a + b - 1].  Inner node at index i: b == 0, the children are i + 1 and a (a > i + 1).
struct Node {
  float lo[3], hi[3];
  int a, b;
};
static_assert(sizeof(Node) == 32, "a node is 32 bytes");

// the squared distance from q to the box, 0 inside: never above the squared distance to anything in the box by more than its rounding
DF_MC_HD double box_lb(const Node &n, const double *q) {
  double s[3];
  for (int j = 0; j < 3; ++j) {
    const double below = (double)n.lo[j] - q[j], above = q[j] - (double)n.hi[j];
    double m = below > 0.0 ? below : 0.0;
    m = above > m ? above : m;
    s[j] = m * m;
  }
  return (s[0] + s[1]) + s[2];
}

// what a computed d_t may fall below the true squared distance by, plus box_lb's own rounding: 2^-36 R^2, R = W + E, W the largest
// |q_j - (a face of the root box)_j| (it bounds every |q_j - U_j|) and E the root box's longest side (it bounds every |e_j|).  Every
// rounding in D1, D2 and box_lb is relative to such differences, not to the coordinates, so the slack does not grow when the mesh lies
// far from the origin.  A NaN or infinite R gives a slack with which `skip` never holds.
DF_MC_HD double slack2(const Node &root, const double *q) {
  double W = 0.0, E = 0.0;
  for (int j = 0; j < 3; ++j) {
    const double l = fabs(q[j] - (double)root.lo[j]), h = fabs((double)root.hi[j] - q[j]), s = (double)root.hi[j] - (double)root.lo[j];
    W = l > W ? l : W;
    W = h > W ? h : W;
    E = s > E ? s : E;
  }
  const double R = W + E;
  return (SLACK_REL * R) * R;
}

// strictly: a triangle with d_t == cut and a lower index must still be met.  False for any NaN.
DF_MC_HD bool skip(double lb, double slack, double cut) { return lb - slack > cut; }

// a kept triangle that the tree may not hold: a vertex that is not finite, or a face (nn > 0) with an angle whose sin^2 = nn / (ee_i ee_j)
// is below 2^-16.  Its D2 candidate can fall below the true distance by more than slack2 covers; it is tested for every query instead.
DF_MC_HD bool tri_loose(const TriRec &r) {
  double ee[3];
  for (int k = 0; k < 3; ++k) {
    for (int j = 0; j < 3; ++j)
      if (!(fabs(r.U[k][j]) < std::numeric_limits<double>::infinity())) return true;
    ee[k] = meshclosest::dot3(r.e[k], r.e[k]);
  }
  if (!(r.nn > 0.0)) return false;                     // edges only: D1 is conservative whatever the shape
  for (int k = 0; k < 3; ++k)
    if (r.nn < LOOSE_SIN2 * (ee[k] * ee[k == 2 ? 0 : k + 1])) return true;
  return false;
}

// One object's tree as `walk` reads it.  Everything is indexed call-globally; [node_lo, node_hi) are the object's nodes (root node_lo,
// none when empty), [tri_lo, tri_hi) its triangles.  The ranges also bound every index read from the arrays: an index outside them is
// not followed, so arrays that no build wrote cannot take a read out of bounds or a walk round in a circle.
struct View {
  const Node *nodes;
  const int *order, *loose;
  int node_lo, node_hi, n_order, loose_lo, loose_hi, tri_lo, tri_hi;
};

// what a walk adds to when it is given one: the triangles and the boxes it tested
struct Tally {
  long tri, box;
};

// The closest triangle of q: (*bd, *bt) = D4's winner among the object's kept triangles, or (+inf, -1).  `limit`: triangles whose d_t
// lies above it need not be found (+inf: all; df_mesh_icp_tree gives max_dist^2) -- the winner is exact whenever its d_t <= limit, and
// is some triangle above the limit or none otherwise.  Stack: push(int), pop() -> int, for at most MAX_DEPTH entries.
template <class Stack>
DF_MC_HD void walk(const View &v, const TriRec *rec, const double *q, double limit, Stack &st, double *bd_out, int *bt_out, Tally *tally) {
  double bd = std::numeric_limits<double>::infinity(), cut = limit;
  int bt = -1;
  *bd_out = bd;
  *bt_out = bt;
  if (q[0] != q[0] || q[1] != q[1] || q[2] != q[2]) return;    // a NaN query: every d_t is a NaN, nothing wins (D5)
  for (int i = v.loose_lo; i < v.loose_hi; ++i) {
    const int t = v.loose[i];
    if (t < v.tri_lo || t >= v.tri_hi) continue;
    const double d = meshclosest::tri_d2(rec[t], q);
    if (tally) ++tally->tri;
    if (d < std::numeric_limits<double>::infinity() && meshclosest::better(d, t, bd, bt)) { bd = d; bt = t; cut = d < cut ? d : cut; }
  }
  if (v.node_hi > v.node_lo) {
    const double slack = slack2(v.nodes[v.node_lo], q);
    int sp = 0, node = v.node_lo;
    for (;;) {
      if (node < 0) {
        if (sp == 0) break;
        node = st.pop(--sp);
      }
      const Node n = v.nodes[node];
      if (tally) ++tally->box;
      if (skip(box_lb(n, q), slack, cut)) { node = -1; continue; }
      if (n.b > 0) {
        if (n.a >= 0 && n.b <= v.n_order - n.a)
          for (int i = 0; i < n.b; ++i) {
            const int t = v.order[n.a + i];
            if (t < v.tri_lo || t >= v.tri_hi) continue;
            const double d = meshclosest::tri_d2(rec[t], q);
            if (tally) ++tally->tri;
            if (d < std::numeric_limits<double>::infinity() && meshclosest::better(d, t, bd, bt)) { bd = d; bt = t; cut = d < cut ? d : cut; }
          }
        node = -1;
        continue;
      }
      const int l = node + 1, r = n.a;
      if (r <= l || r >= v.node_hi || sp >= MAX_DEPTH) { node = -1; continue; }
      // the nearer child first, so that the farther one meets a smaller cut when it is popped; it is tested again there
      const double ll = box_lb(v.nodes[l], q), lr = box_lb(v.nodes[r], q);
      const bool right_first = lr < ll;
      st.push(sp++, right_first ? l : r);
      node = right_first ? r : l;
    }
  }
  *bd_out = bd;
  *bt_out = bt;
}

// the stack of a host caller
struct HostStack {
  int s[MAX_DEPTH];
  void push(int at, int node) { s[at] = node; }
  int pop(int at) const { return s[at]; }
};

}  // namespace meshtree
}  // namespace df
