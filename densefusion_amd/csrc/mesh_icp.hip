// df_mesh_icp: point-to-plane ICP of B poses against the exact closest points of their triangle ranges, in fp64.  The contract is the
// comment of the call in include/dfusion.h (steps S0, I1..I10); the per-item rules are mesh_icp_core.h, the closest point is
// mesh_closest_core.h's; tests/mesh_icp_np.py restates them in numpy and the outputs are compared bit for bit.
//
// The launches of one call, back to back on the caller's stream: mesh_prepare_kernel (mesh_prepare.h, shared with df_mesh_closest) and
// icp_init_kernel once, then iters + 1 times icp_scan_kernel followed by icp_reduce_kernel; the first `iters` reduces also solve and move
// the pose, the last only fills the stats.  The state between launches is pose_out and stats themselves: a workgroup reads its item's
// pose and status from there, so the pose changes on the device with no host round trip and a frozen item (status != 0) is skipped.
//   icp_scan_kernel: the wave-split scan of mesh_closest.hip (N is hundreds to a few thousand per item, so B * N / 512 workgroups
//   would not fill the part): a workgroup takes one item and IC_QUERIES of its points; the four waves share them, two per lane in
//   registers, and wave w walks records w, w + 4, ... of each 128-record LDS tile of the item's range (broadcast reads, branch-free
//   selects, no division); the partial winners meet in LDS by (smaller d, then lower t).  Wave 0 then reads the winner's record back
//   and writes the point's terms (I4, I5): J, r, d2 and the inlier flag.
//   icp_reduce_kernel: one workgroup per item.  Lane l sums the terms of points l, l + 256, ... in ascending order, a binary tree runs
//   over the 64 lanes of each wave (shuffles) and over the four waves (LDS), and lane 0 does the Cholesky solve and the update (I7..I9).
//   df_mesh_icp_tree is the same call with icp_walk_kernel in the scan's place: the same winner found through the object's box tree
//   (mesh_tree_core.h), one point per lane; everything before and after it is shared, so the outputs are the same bytes.
// No atomics; an item's outputs depend on its own points, pose, object and the mesh only.
#include <climits>

#include "common.h"
#include "mesh_icp_core.h"
#include "mesh_prepare.h"
#include "mesh_tree.h"

namespace df {
namespace {

using meshclosest::TriRec;

constexpr int IC_BLOCK = 256;                    // threads per workgroup
constexpr int IC_WAVES = IC_BLOCK / 64;
constexpr int IC_QPL = 2;                        // queries per lane
constexpr int IC_QUERIES = 64 * IC_QPL;          // queries per scan workgroup
constexpr int IC_TILE = 128;                     // records per LDS tile: 32 KiB
static_assert(IC_BLOCK == meshicp::LANES && meshicp::WAVE == 64, "the accumulation order of mesh_icp_core.h is this kernel's shape");

// host arrays, passed by value as launch arguments
struct IcpObjects {
  int O;
  int tri_begin[meshicp::MAX_OBJECTS + 1];
  double md2[meshicp::MAX_OBJECTS];              // max_dist^2
};

// S0: one thread per item
__global__ __launch_bounds__(IC_BLOCK) void icp_init_kernel(IcpObjects objs, const int *__restrict__ obj, const double *__restrict__ pose_in,
                                                            int B, double *__restrict__ pose_out, double *__restrict__ stats) {
  const int b = blockIdx.x * IC_BLOCK + threadIdx.x;
  if (b >= B) return;
  double p[7];
  for (int e = 0; e < 7; ++e) p[e] = pose_in[7 * (size_t)b + e];
  meshicp::normalise_quat(p);
  for (int e = 0; e < 7; ++e) pose_out[7 * (size_t)b + e] = p[e];
  const int o = obj[b];
  const bool known = o >= 0 && o < objs.O;
  const int oc = known ? o : 0;                                // nothing is read through a bad object
  const bool bad = !known || objs.tri_begin[oc + 1] <= objs.tri_begin[oc];
  double *s = stats + meshicp::NSTAT * (size_t)b;
  for (int e = 0; e < meshicp::NSTAT; ++e) s[e] = 0.0;
  if (bad) s[meshicp::ST_STATUS] = (double)meshicp::BAD_OBJECT;
}

// grid = B * qblocks (block i: item i / qblocks, query block i % qblocks)
__global__ __launch_bounds__(IC_BLOCK) void icp_scan_kernel(const TriRec *__restrict__ rec, IcpObjects objs, const int *__restrict__ obj,
                                                            const float *__restrict__ points, int N, int qblocks, int cull,
                                                            const double *__restrict__ pose, const double *__restrict__ stats,
                                                            double *__restrict__ terms, int *__restrict__ inlier) {
  __shared__ __attribute__((aligned(16))) TriRec tile[IC_TILE];
  __shared__ double part_d[IC_WAVES][IC_QUERIES];
  __shared__ int part_t[IC_WAVES][IC_QUERIES];
  const int b = blockIdx.x / qblocks, qb = blockIdx.x - b * qblocks;
  if (stats[meshicp::NSTAT * (size_t)b + meshicp::ST_STATUS] != 0.0) return;   // frozen or bad object: the whole workgroup leaves
  const int o = obj[b];                                                        // in range: icp_init_kernel checked it
  const int tb = objs.tri_begin[o], T = objs.tri_begin[o + 1] - tb;
  const double md2 = objs.md2[o];
  rec += tb;
  const int slot = threadIdx.x % 64, part = threadIdx.x / 64;
  double X[12];
  meshicp::model_frame(pose + 7 * (size_t)b, X);
  double q[IC_QPL][3], bd[IC_QPL];
  int bt[IC_QPL], qi[IC_QPL];
#pragma unroll
  for (int j = 0; j < IC_QPL; ++j) {
    qi[j] = qb * IC_QUERIES + j * 64 + slot;
    const int qc = qi[j] < N ? qi[j] : N - 1;                  // lanes past the end compute on a valid point and never store
    const float *pf = points + 3 * ((size_t)b * N + qc);
    const double p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
    meshclosest::transform_query(X, p, q[j]);
    bd[j] = INFINITY;
    bt[j] = -1;
  }
  for (int t0 = 0; t0 < T; t0 += IC_TILE) {
    const int nt = T - t0 < IC_TILE ? T - t0 : IC_TILE;
    __syncthreads();                                           // the previous tile's readers are done
    {
      const double2 *src = reinterpret_cast<const double2 *>(rec + t0);
      double2 *dst = reinterpret_cast<double2 *>(tile);
      for (int i = threadIdx.x; i < nt * (meshclosest::REC_DOUBLES / 2); i += IC_BLOCK) dst[i] = src[i];
    }
    __syncthreads();
    for (int i = part; i < nt; i += IC_WAVES) {
      const TriRec &r = tile[i];
#pragma unroll
      for (int j = 0; j < IC_QPL; ++j) {
        const double d = meshclosest::tri_d2(r, q[j]);
        const bool win = d < bd[j];                            // ascending t: the lowest index keeps a tie, a NaN never wins
        bd[j] = win ? d : bd[j];
        bt[j] = win ? t0 + i : bt[j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < IC_QPL; ++j) {
    part_d[part][j * 64 + slot] = bd[j];
    part_t[part][j * 64 + slot] = bt[j];
  }
  __syncthreads();
  if (part != 0) return;
  const double cam[3] = {X[3], X[7], X[11]};
#pragma unroll
  for (int j = 0; j < IC_QPL; ++j) {
    for (int w = 1; w < IC_WAVES; ++w) {
      const double d = part_d[w][j * 64 + slot];
      const int t = part_t[w][j * 64 + slot];
      if (meshclosest::better(d, t, bd[j], bt[j])) { bd[j] = d; bt[j] = t; }
    }
    if (qi[j] >= N) continue;
    const size_t at = (size_t)b * N + qi[j];
    double term[meshicp::TERM_DOUBLES];
    const bool in = meshicp::point_terms(rec, bt[j], bd[j], q[j], md2, cull, cam, term);
    double2 *dst = reinterpret_cast<double2 *>(terms + meshicp::TERM_DOUBLES * at);
#pragma unroll
    for (int e = 0; e < meshicp::TERM_DOUBLES / 2; ++e) dst[e] = make_double2(term[2 * e], term[2 * e + 1]);
    inlier[at] = in ? 1 : 0;
  }
}

// df_mesh_icp_tree's scan: icp_scan_kernel's inputs and outputs with the closest triangle found through the object's box tree
// (mesh_tree_core.h's walk, its stack in LDS), one point per lane.  Triangles further than max_dist need not be found: such a point is
// no inlier whichever triangle it is given (I4).  rec and the walk's indices are call-global here; the winner's record is the same.
// grid = B * qblocks (block i: item i / qblocks, query block i % qblocks)
__global__ __launch_bounds__(MT_BLOCK) void icp_walk_kernel(const TriRec *__restrict__ rec, IcpObjects objs, TreeArgs tree, const int *__restrict__ obj,
                                                            const float *__restrict__ points, int N, int qblocks, int cull,
                                                            const double *__restrict__ pose, const double *__restrict__ stats,
                                                            double *__restrict__ terms, int *__restrict__ inlier) {
  __shared__ int stack_words[meshtree::MAX_DEPTH * MT_BLOCK];
  LdsStack stack{stack_words + threadIdx.x};
  const int b = blockIdx.x / qblocks, qi = (blockIdx.x - b * qblocks) * MT_BLOCK + threadIdx.x;
  if (stats[meshicp::NSTAT * (size_t)b + meshicp::ST_STATUS] != 0.0) return;   // frozen or bad object: the whole workgroup leaves
  if (qi >= N) return;                                                         // no barrier follows
  const int o = obj[b];                                                        // in range: icp_init_kernel checked it
  const double md2 = objs.md2[o];
  double X[12], q[3], bd;
  int bt;
  meshicp::model_frame(pose + 7 * (size_t)b, X);
  const float *pf = points + 3 * ((size_t)b * N + qi);
  const double p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
  meshclosest::transform_query(X, p, q);
  meshtree::walk(tree_view(tree, o, objs.tri_begin[o], objs.tri_begin[o + 1]), rec, q, md2, stack, &bd, &bt, nullptr);
  const double cam[3] = {X[3], X[7], X[11]};
  const size_t at = (size_t)b * N + qi;
  double term[meshicp::TERM_DOUBLES];
  const bool in = meshicp::point_terms(rec, bt, bd, q, md2, cull, cam, term);
  double2 *dst = reinterpret_cast<double2 *>(terms + meshicp::TERM_DOUBLES * at);
#pragma unroll
  for (int e = 0; e < meshicp::TERM_DOUBLES / 2; ++e) dst[e] = make_double2(term[2 * e], term[2 * e + 1]);
  inlier[at] = in ? 1 : 0;
}

// grid = B.  pass: 0 for the first scan; solve: take the step (I7..I9) after the sums
__global__ __launch_bounds__(IC_BLOCK) void icp_reduce_kernel(const double *__restrict__ terms, const int *__restrict__ inlier, int N, int pass,
                                                              int solve, double *__restrict__ pose, double *__restrict__ stats) {
  __shared__ double part_s[IC_WAVES][meshicp::NSUM];
  __shared__ int part_c[IC_WAVES];
  const int b = blockIdx.x;
  if (stats[meshicp::NSTAT * (size_t)b + meshicp::ST_STATUS] != 0.0) return;
  double acc[meshicp::NSUM];
#pragma unroll
  for (int k = 0; k < meshicp::NSUM; ++k) acc[k] = 0.0;
  int cnt = 0;
  for (int i = threadIdx.x; i < N; i += IC_BLOCK) {
    const size_t at = (size_t)b * N + i;
    if (!inlier[at]) continue;
    double term[meshicp::TERM_DOUBLES];
    const double2 *src = reinterpret_cast<const double2 *>(terms + meshicp::TERM_DOUBLES * at);
#pragma unroll
    for (int e = 0; e < meshicp::TERM_DOUBLES / 2; ++e) { const double2 v = src[e]; term[2 * e] = v.x; term[2 * e + 1] = v.y; }
    meshicp::accumulate(term, acc);
    ++cnt;
  }
  // the tree over a wave's lanes: at step s lane l < s adds lane l + s (the other lanes' values are not used afterwards)
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
    for (int k = 0; k < meshicp::NSUM; ++k) acc[k] = acc[k] + __shfl_down(acc[k], s);
    cnt += __shfl_down(cnt, s);
  }
  const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < meshicp::NSUM; ++k) part_s[wave][k] = acc[k];
    part_c[wave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sums[meshicp::NSUM];
  for (int k = 0; k < meshicp::NSUM; ++k) sums[k] = (part_s[0][k] + part_s[1][k]) + (part_s[2][k] + part_s[3][k]);
  const int count = (part_c[0] + part_c[1]) + (part_c[2] + part_c[3]);
  meshicp::finish_pass(sums, count, pass, solve, pose + 7 * (size_t)b, stats + meshicp::NSTAT * (size_t)b);
}

size_t terms_bytes(int B, int N) { return (size_t)B * N * meshicp::TERM_DOUBLES * sizeof(double); }

bool overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

}  // namespace
}  // namespace df

using namespace df;

extern "C" size_t df_mesh_icp_scratch_bytes(int T, int B, int N) {
  if (T < 1 || B < 1 || N < 1) return 0;
  return (size_t)T * sizeof(TriRec) + terms_bytes(B, N) + ((size_t)B * N * sizeof(int) + 15) / 16 * 16;
}

namespace df {
namespace {

// the tree arrays of df_mesh_icp_tree as the caller gave them
struct TreeGiven {
  const void *nodes;
  size_t n_nodes;
  const int *node_begin, *order;
  size_t n_order;
  const int *loose;
  size_t n_loose;
  const int *loose_begin;
};

// df_mesh_icp (given == nullptr) and df_mesh_icp_tree: one set of refusals, one sequence of launches; only the scan kernel differs
int icp_run(const char *name, const float *vertices, int V, const int *triangles, int T, const int *tri_begin, const double *max_dist, int O,
            const int *obj, const float *points, const double *pose_in, int B, int N, int iters, int cull, double *pose_out, double *stats,
            void *scratch, size_t scratch_bytes, df_stream_t stream, const TreeGiven *given) {
  if (given && (!given->nodes || !given->node_begin || !given->order || !given->loose || !given->loose_begin))
    return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (!vertices || !triangles || !tri_begin || !max_dist || !obj || !points || !pose_in || !pose_out || !stats || !scratch)
    return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (V < 1 || T < 1 || B < 1 || N < 1) return set_error(DF_ERR_ARG, "%s: need V, T, B, N >= 1 (V %d, T %d, B %d, N %d)", name, V, T, B, N);
  if (3L * V > INT_MAX || 3L * T > INT_MAX || 8L * B * N > INT_MAX)
    return set_error(DF_ERR_ARG, "%s: 3 V, 3 T and 8 B N must fit an int (V %d, T %d, B %d, N %d)", name, V, T, B, N);
  if (O < 1 || O > meshicp::MAX_OBJECTS) return set_error(DF_ERR_ARG, "%s: O must be 1..%d (got %d)", name, meshicp::MAX_OBJECTS, O);
  if (iters < 0 || iters > meshicp::MAX_ITERS) return set_error(DF_ERR_ARG, "%s: iters must be 0..%d (got %d)", name, meshicp::MAX_ITERS, iters);
  if (cull != 0 && cull != 1) return set_error(DF_ERR_ARG, "%s: cull must be 0 or 1 (got %d)", name, cull);
  IcpObjects objs;
  objs.O = O;
  for (int o = 0; o <= meshicp::MAX_OBJECTS; ++o) objs.tri_begin[o] = 0;
  for (int o = 0; o < meshicp::MAX_OBJECTS; ++o) objs.md2[o] = 0.0;
  for (int o = 0; o <= O; ++o) {
    if (tri_begin[o] < 0 || tri_begin[o] > T || (o > 0 && tri_begin[o] < tri_begin[o - 1]))
      return set_error(DF_ERR_ARG, "%s: tri_begin must be non-decreasing within 0..T (entry %d is %d, T %d)", name, o, tri_begin[o], T);
    objs.tri_begin[o] = tri_begin[o];
  }
  for (int o = 0; o < O; ++o) {
    if (!(max_dist[o] > 0)) return set_error(DF_ERR_ARG, "%s: max_dist must be > 0 (entry %d is %g)", name, o, max_dist[o]);
    objs.md2[o] = max_dist[o] * max_dist[o];
  }
  const size_t need = df_mesh_icp_scratch_bytes(T, B, N);
  if (scratch_bytes < need || reinterpret_cast<uintptr_t>(scratch) % 16)
    return set_error(DF_ERR_ARG, "%s: scratch must be 16-byte aligned and hold %zu bytes (got %zu)", name, need, scratch_bytes);
  if (reinterpret_cast<uintptr_t>(vertices) % 4 || reinterpret_cast<uintptr_t>(triangles) % 4 || reinterpret_cast<uintptr_t>(obj) % 4 ||
      reinterpret_cast<uintptr_t>(points) % 4 || reinterpret_cast<uintptr_t>(pose_in) % 8 || reinterpret_cast<uintptr_t>(pose_out) % 8 ||
      reinterpret_cast<uintptr_t>(stats) % 8)
    return set_error(DF_ERR_ARG, "%s: vertices, triangles, obj and points must be 4-byte, pose_in, pose_out and stats 8-byte aligned", name);
  const size_t pose_b = (size_t)B * 7 * sizeof(double), stats_b = (size_t)B * meshicp::NSTAT * sizeof(double);
  const struct { const void *p; size_t n; } ins[] = {{vertices, (size_t)V * 12}, {triangles, (size_t)T * 12}, {obj, (size_t)B * 4},
                                                     {points, (size_t)B * N * 12}, {pose_in, pose_b}, {scratch, need}};
  for (const auto &in : ins)
    if (overlap(pose_out, pose_b, in.p, in.n) || overlap(stats, stats_b, in.p, in.n))
      return set_error(DF_ERR_ARG, "%s: pose_out and stats may not overlap the inputs or the scratch", name);
  if (overlap(pose_out, pose_b, stats, stats_b)) return set_error(DF_ERR_ARG, "%s: pose_out and stats overlap", name);
  TreeArgs tree;
  if (given)
    if (int rc = check_tree(name, given->nodes, given->n_nodes, given->node_begin, given->order, given->n_order, given->loose, given->n_loose,
                            given->loose_begin, tri_begin, O, &tree))
      return rc;

  hipStream_t st = to_stream(stream);
  TriRec *rec = static_cast<TriRec *>(scratch);
  double *terms = reinterpret_cast<double *>(rec + T);
  int *inlier = reinterpret_cast<int *>(reinterpret_cast<char *>(terms) + terms_bytes(B, N));
  hipLaunchKernelGGL(mesh_prepare_kernel, dim3(cdiv(T, MESH_PREPARE_BLOCK)), dim3(MESH_PREPARE_BLOCK), 0, st, vertices, V, triangles, T, rec);
  hipLaunchKernelGGL(icp_init_kernel, dim3(cdiv(B, IC_BLOCK)), dim3(IC_BLOCK), 0, st, objs, obj, pose_in, B, pose_out, stats);
  const int qblocks = cdiv(N, IC_QUERIES), wblocks = cdiv(N, MT_BLOCK);
  for (int pass = 0; pass <= iters; ++pass) {
    if (given)
      hipLaunchKernelGGL(icp_walk_kernel, dim3(B * wblocks), dim3(MT_BLOCK), 0, st, rec, objs, tree, obj, points, N, wblocks, cull, pose_out, stats,
                         terms, inlier);
    else
      hipLaunchKernelGGL(icp_scan_kernel, dim3(B * qblocks), dim3(IC_BLOCK), 0, st, rec, objs, obj, points, N, qblocks, cull, pose_out, stats, terms,
                         inlier);
    hipLaunchKernelGGL(icp_reduce_kernel, dim3(B), dim3(IC_BLOCK), 0, st, terms, inlier, N, pass, pass < iters ? 1 : 0, pose_out, stats);
  }
  return check_launch(name);
}

}  // namespace
}  // namespace df

extern "C" int df_mesh_icp(const float *vertices, int V, const int *triangles, int T, const int *tri_begin, const double *max_dist, int O,
                           const int *obj, const float *points, const double *pose_in, int B, int N, int iters, int cull, double *pose_out,
                           double *stats, void *scratch, size_t scratch_bytes, df_stream_t stream) {
  return icp_run("mesh_icp", vertices, V, triangles, T, tri_begin, max_dist, O, obj, points, pose_in, B, N, iters, cull, pose_out, stats, scratch,
                 scratch_bytes, stream, nullptr);
}

extern "C" int df_mesh_icp_tree(const float *vertices, int V, const int *triangles, int T, const int *tri_begin, const double *max_dist, int O,
                                const int *obj, const float *points, const double *pose_in, int B, int N, int iters, int cull, double *pose_out,
                                double *stats, void *scratch, size_t scratch_bytes, df_stream_t stream, const void *nodes, size_t n_nodes,
                                const int *node_begin, const int *order, size_t n_order, const int *loose, size_t n_loose, const int *loose_begin) {
  const TreeGiven given = {nodes, n_nodes, node_begin, order, n_order, loose, n_loose, loose_begin};
  return icp_run("mesh_icp_tree", vertices, V, triangles, T, tri_begin, max_dist, O, obj, points, pose_in, B, N, iters, cull, pose_out, stats,
                 scratch, scratch_bytes, stream, &given);
}
