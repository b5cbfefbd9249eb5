// What df_mesh_closest_tree (mesh_tree.hip) and df_mesh_icp_tree (mesh_icp.hip) share on the HIP side of the box tree: the per-object
// table that travels as a launch argument, the one host check of the tree arrays, and the walk's stack in LDS.
#pragma once
#include <climits>

#include "common.h"
#include "mesh_tree_core.h"

namespace df {
namespace {

constexpr int MT_BLOCK = 256;                     // threads per workgroup of a walking kernel: one query per lane
constexpr int MT_MAX_OBJECTS = 64;

// the device arrays of a tree and, by value, where each object's part of them lies
struct TreeArgs {
  const meshtree::Node *nodes;
  const int *order, *loose;
  int n_order;
  int node_begin[MT_MAX_OBJECTS + 1], loose_begin[MT_MAX_OBJECTS + 1];
};

// The refusals for the tree arrays (null pointers are the caller's check).  tri_begin [O+1] is the table the tree was built for:
// an object's nodes and loose triangles must fit its triangle range (at most 2 n - 1 nodes and n loose triangles for n triangles).
inline int check_tree(const char *name, const void *nodes, size_t n_nodes, const int *node_begin, const void *order, size_t n_order,
                      const void *loose, size_t n_loose, const int *loose_begin, const int *tri_begin, int O, TreeArgs *out) {
  if (reinterpret_cast<uintptr_t>(nodes) % 16 || reinterpret_cast<uintptr_t>(order) % 4 || reinterpret_cast<uintptr_t>(loose) % 4)
    return set_error(DF_ERR_ARG, "%s: tree nodes must be 16-byte, order and loose 4-byte aligned", name);
  if (node_begin[0] != 0 || loose_begin[0] != 0) return set_error(DF_ERR_ARG, "%s: node_begin and loose_begin must start at 0", name);
  long in_tree = 0;
  for (int o = 0; o < O; ++o) {
    const long n = (long)tri_begin[o + 1] - tri_begin[o], nn = (long)node_begin[o + 1] - node_begin[o],
               nl = (long)loose_begin[o + 1] - loose_begin[o];
    if (nn < 0 || nl < 0 || nl > n || nn > (n - nl > 0 ? 2 * (n - nl) - 1 : 0))
      return set_error(DF_ERR_ARG, "%s: object %d has %ld triangles; its tree cannot have %ld nodes and %ld loose triangles", name, o, n, nn, nl);
    in_tree += n - nl;
  }
  if ((size_t)node_begin[O] > n_nodes || (size_t)loose_begin[O] > n_loose || n_order > (size_t)INT_MAX || (node_begin[O] > 0 && n_order < 1) ||
      (long)n_order > in_tree)
    return set_error(DF_ERR_ARG, "%s: the tree arrays are short for their tables (%zu nodes for %d, %zu loose for %d, %zu order entries)", name,
                     n_nodes, node_begin[O], n_loose, loose_begin[O], n_order);
  out->nodes = static_cast<const meshtree::Node *>(nodes);
  out->order = static_cast<const int *>(order);
  out->loose = static_cast<const int *>(loose);
  out->n_order = (int)n_order;
  for (int o = 0; o <= MT_MAX_OBJECTS; ++o) {
    out->node_begin[o] = node_begin[o <= O ? o : O];
    out->loose_begin[o] = loose_begin[o <= O ? o : O];
  }
  return DF_OK;
}

__device__ inline meshtree::View tree_view(const TreeArgs &t, int o, int tri_lo, int tri_hi) {
  meshtree::View v;
  v.nodes = t.nodes; v.order = t.order; v.loose = t.loose;
  v.node_lo = t.node_begin[o]; v.node_hi = t.node_begin[o + 1];
  v.n_order = t.n_order;
  v.loose_lo = t.loose_begin[o]; v.loose_hi = t.loose_begin[o + 1];
  v.tri_lo = tri_lo; v.tri_hi = tri_hi;
  return v;
}

// the walk's stack: entry `at` of lane l is word at * MT_BLOCK + l of a workgroup's 32 KiB, so a wave's pushes and pops touch 64
// consecutive banks.  A lane reads only what it wrote: no barrier.
struct LdsStack {
  int *base;                                      // the lane's column
  __device__ void push(int at, int node) { base[at * MT_BLOCK] = node; }
  __device__ int pop(int at) const { return base[at * MT_BLOCK]; }
};

}  // namespace
}  // namespace df
