// The bounding-box tree of a packed mesh set and df_mesh_closest through it.  The contract is the comment of the calls in
// include/dfusion.h; the rules of the walk are mesh_tree_core.h, the distances mesh_closest_core.h's, unchanged, and the proof that a
// skipped box holds no winner is DESIGN 12l: the outputs are df_mesh_closest's bytes.
//
// df_mesh_tree_build (host): per object, the kept triangles that `tri_loose` does not take are split at the median of their centroids
// along the longest axis of the centroid bounds, ordered by (coordinate, index), until at most `leaf` remain; nodes are written in
// preorder (an inner node's left child follows it), leaves list their triangles in ascending index.  A pure function of its inputs.
// mesh_walk_kernel: one query per lane; `meshtree::walk` with its stack in LDS (32 entries x 256 lanes x 4 B); records are read from
// the prepared array through `order`.  No atomics, no barrier; a query's outputs depend on its own point, its transform and the mesh.
#include <algorithm>
#include <climits>
#include <vector>

#include "common.h"
#include "mesh_prepare.h"
#include "mesh_tree.h"

namespace df {
namespace {

using meshclosest::TriRec;
using meshtree::Node;

struct Builder {
  const float *vertices;
  const int *triangles;
  const double *centroid;     // [T][3], call-global
  int leaf;
  std::vector<Node> nodes;
  std::vector<int> order;
  bool too_deep = false;

  Node leaf_box(const int *t, int n) const {
    Node b;
    for (int j = 0; j < 3; ++j) { b.lo[j] = INFINITY; b.hi[j] = -INFINITY; }
    for (int i = 0; i < n; ++i)
      for (int c = 0; c < 3; ++c) {
        const float *p = vertices + 3 * (size_t)triangles[3 * (size_t)t[i] + c];
        for (int j = 0; j < 3; ++j) { b.lo[j] = std::min(b.lo[j], p[j]); b.hi[j] = std::max(b.hi[j], p[j]); }
      }
    return b;
  }

  // the subtree of t[0..n-1] (n >= 1) below `depth` inner nodes; returns its root's index
  int build(int *t, int n, int depth) {
    const int at = (int)nodes.size();
    nodes.push_back(Node());
    if (n <= leaf) {
      std::sort(t, t + n);
      Node b = leaf_box(t, n);
      b.a = (int)order.size();
      b.b = n;
      order.insert(order.end(), t, t + n);
      nodes[at] = b;
      return at;
    }
    if (depth >= meshtree::MAX_DEPTH) { too_deep = true; return at; }
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < 3; ++j) {
        const double c = centroid[3 * (size_t)t[i] + j];
        lo[j] = c < lo[j] ? c : lo[j];
        hi[j] = c > hi[j] ? c : hi[j];
      }
    int axis = 0;
    for (int j = 1; j < 3; ++j)
      if (hi[j] - lo[j] > hi[axis] - lo[axis]) axis = j;
    const double *c = centroid;
    const int half = n / 2;                                    // the left child takes the lower half
    std::nth_element(t, t + half, t + n, [c, axis](int x, int y) {
      const double cx = c[3 * (size_t)x + axis], cy = c[3 * (size_t)y + axis];
      return cx < cy || (cx == cy && x < y);
    });
    build(t, half, depth + 1);
    const int right = build(t + half, n - half, depth + 1);
    Node b;
    const Node &l = nodes[at + 1], &r = nodes[right];
    for (int j = 0; j < 3; ++j) { b.lo[j] = std::min(l.lo[j], r.lo[j]); b.hi[j] = std::max(l.hi[j], r.hi[j]); }
    b.a = right;
    b.b = 0;
    nodes[at] = b;
    return at;
  }
};

int check_mesh_host(const char *name, const void *vertices, int V, const void *triangles, int T, const int *tri_begin, int O) {
  if (!vertices || !triangles || !tri_begin) return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (V < 1 || T < 1 || 3L * V > INT_MAX || 3L * T > INT_MAX) return set_error(DF_ERR_ARG, "%s: need V, T >= 1 and 3 V, 3 T within an int (V %d, T %d)", name, V, T);
  if (O < 1 || O > MT_MAX_OBJECTS) return set_error(DF_ERR_ARG, "%s: O must be 1..%d (got %d)", name, MT_MAX_OBJECTS, O);
  for (int o = 0; o <= O; ++o)
    if (tri_begin[o] < 0 || tri_begin[o] > T || (o > 0 && tri_begin[o] < tri_begin[o - 1]))
      return set_error(DF_ERR_ARG, "%s: tri_begin must be non-decreasing within 0..T (entry %d is %d, T %d)", name, o, tri_begin[o], T);
  return DF_OK;
}

// grid = query blocks * K (block b: transform b / qblocks, query block b % qblocks)
__global__ __launch_bounds__(MT_BLOCK) void mesh_walk_kernel(const TriRec *__restrict__ rec, int T, TreeArgs tree, const double *__restrict__ points,
                                                             int P, const double *__restrict__ xf, int qblocks, double *__restrict__ dist2_out,
                                                             int *__restrict__ tri_out, double *__restrict__ closest_out) {
  __shared__ int stack_words[meshtree::MAX_DEPTH * MT_BLOCK];
  LdsStack stack{stack_words + threadIdx.x};
  const int k = blockIdx.x / qblocks, qi = (blockIdx.x - k * qblocks) * MT_BLOCK + threadIdx.x;
  if (qi >= P) return;                                         // no barrier follows
  double q[3], bd;
  int bt;
  meshclosest::transform_query(xf + 12 * (size_t)k, points + 3 * (size_t)qi, q);
  meshtree::walk(tree_view(tree, 0, 0, T), rec, q, INFINITY, stack, &bd, &bt, nullptr);
  const size_t o = (size_t)k * P + qi;
  double c[3] = {q[0], q[1], q[2]};                            // D5: no winner
  if (bt >= 0 && closest_out) meshclosest::tri_closest(rec[bt], q, c);
  dist2_out[o] = bd;
  tri_out[o] = bt;
  if (closest_out) { closest_out[3 * o] = c[0]; closest_out[3 * o + 1] = c[1]; closest_out[3 * o + 2] = c[2]; }
}

}  // namespace
}  // namespace df

using namespace df;

extern "C" int df_mesh_tree_leaf_triangles(void) { return meshtree::LEAF_DEFAULT; }

extern "C" int df_mesh_tree_sizes(int T, int O, size_t *nodes, size_t *order, size_t *loose) {
  if (!nodes || !order || !loose) return set_error(DF_ERR_ARG, "mesh_tree_sizes: null pointer");
  if (T < 1 || 3L * T > INT_MAX || O < 1 || O > MT_MAX_OBJECTS)
    return set_error(DF_ERR_ARG, "mesh_tree_sizes: need 1 <= T, 3 T within an int, O in 1..%d (T %d, O %d)", MT_MAX_OBJECTS, T, O);
  *nodes = 2 * (size_t)T;
  *order = (size_t)T;
  *loose = (size_t)T;
  return DF_OK;
}

extern "C" int df_mesh_tree_build(const float *vertices, int V, const int *triangles, int T, const int *tri_begin, int O, int leaf, void *nodes,
                                  int *node_begin, int *order, int *loose, int *loose_begin, size_t *used) {
  const char *name = "mesh_tree_build";
  if (int rc = check_mesh_host(name, vertices, V, triangles, T, tri_begin, O)) return rc;
  if (!nodes || !node_begin || !order || !loose || !loose_begin || !used) return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (leaf < 1 || leaf > meshtree::LEAF_MAX) return set_error(DF_ERR_ARG, "%s: leaf must be 1..%d (got %d)", name, meshtree::LEAF_MAX, leaf);
  if (reinterpret_cast<uintptr_t>(nodes) % 16) return set_error(DF_ERR_ARG, "%s: nodes must be 16-byte aligned", name);
  std::vector<double> centroid(3 * (size_t)T, 0.0);
  std::vector<int> list, loose_list;
  Builder b{vertices, triangles, centroid.data(), leaf};
  node_begin[0] = loose_begin[0] = 0;
  for (int o = 0; o < O; ++o) {
    list.clear();
    for (int t = tri_begin[o]; t < tri_begin[o + 1]; ++t) {
      const int *i = triangles + 3 * (size_t)t;
      if (!meshclosest::tri_kept(i[0], i[1], i[2], V)) continue;           // M1: a dropped triangle never wins and is in neither list
      TriRec r;
      meshclosest::prepare_tri(vertices, V, i[0], i[1], i[2], &r);
      if (meshtree::tri_loose(r)) { loose_list.push_back(t); continue; }
      for (int j = 0; j < 3; ++j) centroid[3 * (size_t)t + j] = (r.U[0][j] + r.U[1][j]) + r.U[2][j];
      list.push_back(t);
    }
    if (!list.empty()) b.build(list.data(), (int)list.size(), 0);
    if (b.too_deep) return set_error(DF_ERR_ARG, "%s: the tree of object %d is deeper than %d", name, o, meshtree::MAX_DEPTH);
    node_begin[o + 1] = (int)b.nodes.size();
    loose_begin[o + 1] = (int)loose_list.size();
  }
  std::copy(b.nodes.begin(), b.nodes.end(), static_cast<Node *>(nodes));
  std::copy(b.order.begin(), b.order.end(), order);
  std::copy(loose_list.begin(), loose_list.end(), loose);
  used[0] = b.nodes.size();
  used[1] = b.order.size();
  used[2] = loose_list.size();
  return DF_OK;
}

extern "C" int df_mesh_closest_tree_host(const float *vertices, int V, const int *triangles, int T, const double *points, int P, const double *xf,
                                         int K, const void *nodes, size_t n_nodes, const int *node_begin, const int *order, size_t n_order,
                                         const int *loose, size_t n_loose, const int *loose_begin, double *dist2_out, int *tri_out,
                                         double *closest_out, long long *tested_out) {
  const char *name = "mesh_closest_tree_host";
  const int tri_begin[2] = {0, T};
  if (int rc = check_mesh_host(name, vertices, V, triangles, T, tri_begin, 1)) return rc;
  if (!points || !xf || !nodes || !node_begin || !order || !loose || !loose_begin || !dist2_out || !tri_out)
    return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (P < 1 || K < 1 || 3L * K * P > INT_MAX) return set_error(DF_ERR_ARG, "%s: need P, K >= 1 and 3 K P within an int (P %d, K %d)", name, P, K);
  TreeArgs tree;
  if (int rc = check_tree(name, nodes, n_nodes, node_begin, order, n_order, loose, n_loose, loose_begin, tri_begin, 1, &tree)) return rc;
  std::vector<TriRec> rec((size_t)T);
  for (int t = 0; t < T; ++t) meshclosest::prepare_tri(vertices, V, triangles[3 * (size_t)t], triangles[3 * (size_t)t + 1], triangles[3 * (size_t)t + 2], &rec[t]);
  meshtree::View v{tree.nodes, tree.order, tree.loose, node_begin[0], node_begin[1], tree.n_order, loose_begin[0], loose_begin[1], 0, T};
  for (int k = 0; k < K; ++k)
    for (int p = 0; p < P; ++p) {
      const size_t o = (size_t)k * P + p;
      double q[3], bd;
      int bt;
      meshtree::HostStack stack;
      meshtree::Tally tally{0, 0};
      meshclosest::transform_query(xf + 12 * (size_t)k, points + 3 * (size_t)p, q);
      meshtree::walk(v, rec.data(), q, INFINITY, stack, &bd, &bt, &tally);
      double c[3] = {q[0], q[1], q[2]};
      if (bt >= 0) meshclosest::tri_closest(rec[bt], q, c);
      dist2_out[o] = bd;
      tri_out[o] = bt;
      if (closest_out) { closest_out[3 * o] = c[0]; closest_out[3 * o + 1] = c[1]; closest_out[3 * o + 2] = c[2]; }
      if (tested_out) { tested_out[2 * o] = tally.tri; tested_out[2 * o + 1] = tally.box; }
    }
  return DF_OK;
}

extern "C" int df_mesh_closest_tree(const float *vertices, int V, const int *triangles, int T, const double *points, int P, const double *xf, int K,
                                    double *dist2_out, int *tri_out, double *closest_out, void *scratch, size_t scratch_bytes, df_stream_t stream,
                                    const void *nodes, size_t n_nodes, const int *node_begin, const int *order, size_t n_order, const int *loose,
                                    size_t n_loose, const int *loose_begin) {
  const char *name = "mesh_closest_tree";
  if (!vertices || !triangles || !points || !xf || !dist2_out || !tri_out || !scratch || !nodes || !node_begin || !order || !loose || !loose_begin)
    return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (V < 1 || T < 1 || P < 1 || K < 1) return set_error(DF_ERR_ARG, "%s: need V, T, P, K >= 1 (V %d, T %d, P %d, K %d)", name, V, T, P, K);
  if (3L * V > INT_MAX || 3L * T > INT_MAX || 12L * K > INT_MAX || 3L * K * P > INT_MAX)
    return set_error(DF_ERR_ARG, "%s: 3 V, 3 T, 12 K and 3 K P must fit an int (V %d, T %d, P %d, K %d)", name, V, T, P, K);
  if (scratch_bytes < df_mesh_closest_scratch_bytes(T) || reinterpret_cast<uintptr_t>(scratch) % 16)
    return set_error(DF_ERR_ARG, "%s: scratch must be 16-byte aligned and hold %zu bytes (got %zu)", name, df_mesh_closest_scratch_bytes(T), scratch_bytes);
  if (reinterpret_cast<uintptr_t>(vertices) % 4 || reinterpret_cast<uintptr_t>(triangles) % 4 || reinterpret_cast<uintptr_t>(tri_out) % 4 ||
      reinterpret_cast<uintptr_t>(points) % 8 || reinterpret_cast<uintptr_t>(xf) % 8 || reinterpret_cast<uintptr_t>(dist2_out) % 8 ||
      reinterpret_cast<uintptr_t>(closest_out) % 8)
    return set_error(DF_ERR_ARG, "%s: vertices, triangles and tri_out must be 4-byte, points, xf, dist2_out and closest_out 8-byte aligned", name);
  const int tri_begin[2] = {0, T};
  TreeArgs tree;
  if (int rc = check_tree(name, nodes, n_nodes, node_begin, order, n_order, loose, n_loose, loose_begin, tri_begin, 1, &tree)) return rc;
  hipStream_t st = to_stream(stream);
  TriRec *rec = static_cast<TriRec *>(scratch);
  hipLaunchKernelGGL(mesh_prepare_kernel, dim3(cdiv(T, MESH_PREPARE_BLOCK)), dim3(MESH_PREPARE_BLOCK), 0, st, vertices, V, triangles, T, rec);
  const int qblocks = cdiv(P, MT_BLOCK);
  hipLaunchKernelGGL(mesh_walk_kernel, dim3(qblocks * K), dim3(MT_BLOCK), 0, st, rec, T, tree, points, P, xf, qblocks, dist2_out, tri_out, closest_out);
  return check_launch(name);
}
