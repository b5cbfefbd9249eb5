// df_mesh_closest: the exact closest point of a triangle mesh for K x P transformed queries, in fp64.  The contract is the comment of
// the call in include/dfusion.h (steps M1, M2, Q1, D1..D5); the per-triangle and per-pair rules are mesh_closest_core.h;
// tests/mesh_closest_np.py restates them in numpy and the outputs are compared bit for bit.
//
// Two kernels on the caller's stream.  mesh_prepare_kernel (mesh_prepare.h, shared with df_mesh_icp): one thread per triangle writes its 32-double record (M1, M2) to scratch.
// mesh_scan_kernel<SPLIT>: the scan of the 1-NN kernels of knn.hip with triangle records in place of points.  A lane owns MC_QPL
// queries in registers (q, the best d, the best t); the records are wave-uniform: a workgroup stages MC_TILE of them at a time in LDS
// (coalesced 16-byte copies) and every lane reads the same record, so the LDS reads are broadcasts.  D1 / D2 are branch-free selects:
// every lane has its own query and region tests would diverge.  The inner loop has no fp64 division (the reciprocals are M2's).
//   SPLIT == 1: 256 lanes x MC_QPL queries per workgroup, every wave walks the whole tile.
//   SPLIT == 4 (fewer than MC_FILL workgroups otherwise: the call cannot give every compute unit one): the four waves share 64 x MC_QPL
//   queries, wave w walks records w, w + 4, ... of each tile; the partial winners meet in LDS by (smaller d, then lower t), the
//   winner of the single ascending scan, so the outputs do not depend on which kernel ran.
// The closest point is not carried through the scan: the winner's record is read back once and D3 repeated with the point kept (the
// same operations, hence the same d).  No atomics; a query's outputs depend on its own point, its transform and the mesh only.
#include <climits>

#include "common.h"
#include "mesh_closest_core.h"
#include "mesh_prepare.h"

namespace df {
namespace {

using meshclosest::TriRec;

constexpr int MC_BLOCK = 256;        // threads per workgroup
constexpr int MC_QPL = 2;            // queries per lane
constexpr int MC_TILE = 128;         // records per LDS tile: 32 KiB
constexpr int MC_FILL = 256;         // workgroups below which the triangle range is split over the waves: the compute units of the part
constexpr int MC_WAVES = MC_BLOCK / 64;

// grid = query blocks * K (block b: transform b / qblocks, query block b % qblocks)
template <int SPLIT>
__global__ __launch_bounds__(MC_BLOCK) void mesh_scan_kernel(const TriRec *__restrict__ rec, int T, const double *__restrict__ points, int P,
                                                             const double *__restrict__ xf, int qblocks, double *__restrict__ dist2_out,
                                                             int *__restrict__ tri_out, double *__restrict__ closest_out) {
  constexpr int SLOTS = MC_BLOCK / SPLIT;                      // lanes that own different queries
  __shared__ __attribute__((aligned(16))) TriRec tile[MC_TILE];
  __shared__ double part_d[SPLIT > 1 ? SPLIT : 1][SPLIT > 1 ? SLOTS * MC_QPL : 1];
  __shared__ int part_t[SPLIT > 1 ? SPLIT : 1][SPLIT > 1 ? SLOTS * MC_QPL : 1];
  const int k = blockIdx.x / qblocks, qb = blockIdx.x - k * qblocks;
  const int slot = threadIdx.x % SLOTS, part = threadIdx.x / SLOTS;   // part: the wave, with SPLIT == 4
  const double *X = xf + 12 * (size_t)k;
  double q[MC_QPL][3], bd[MC_QPL];
  int bt[MC_QPL], qi[MC_QPL];
#pragma unroll
  for (int j = 0; j < MC_QPL; ++j) {
    qi[j] = qb * (SLOTS * MC_QPL) + j * SLOTS + slot;
    const int qc = qi[j] < P ? qi[j] : P - 1;                  // lanes past the end compute on a valid point and never store
    meshclosest::transform_query(X, points + 3 * (size_t)qc, q[j]);
    bd[j] = INFINITY;
    bt[j] = -1;
  }
  for (int t0 = 0; t0 < T; t0 += MC_TILE) {
    const int nt = T - t0 < MC_TILE ? T - t0 : MC_TILE;
    __syncthreads();                                           // the previous tile's readers are done
    {
      const double2 *src = reinterpret_cast<const double2 *>(rec + t0);
      double2 *dst = reinterpret_cast<double2 *>(tile);
      for (int i = threadIdx.x; i < nt * (meshclosest::REC_DOUBLES / 2); i += MC_BLOCK) dst[i] = src[i];
    }
    __syncthreads();
    for (int i = SPLIT > 1 ? part : 0; i < nt; i += SPLIT) {
      const TriRec &r = tile[i];
#pragma unroll
      for (int j = 0; j < MC_QPL; ++j) {
        const double d = meshclosest::tri_d2(r, q[j]);
        const bool win = d < bd[j];                            // ascending t: the lowest index keeps a tie, a NaN never wins
        bd[j] = win ? d : bd[j];
        bt[j] = win ? t0 + i : bt[j];
      }
    }
  }
  if (SPLIT > 1) {
#pragma unroll
    for (int j = 0; j < MC_QPL; ++j) {
      part_d[part][j * SLOTS + slot] = bd[j];
      part_t[part][j * SLOTS + slot] = bt[j];
    }
    __syncthreads();
    if (part != 0) return;
#pragma unroll
    for (int j = 0; j < MC_QPL; ++j)
      for (int w = 1; w < SPLIT; ++w) {
        const double d = part_d[w][j * SLOTS + slot];
        const int t = part_t[w][j * SLOTS + slot];
        if (meshclosest::better(d, t, bd[j], bt[j])) { bd[j] = d; bt[j] = t; }
      }
  }
#pragma unroll
  for (int j = 0; j < MC_QPL; ++j) {
    if (qi[j] >= P) continue;
    const size_t o = (size_t)k * P + qi[j];
    double c[3] = {q[j][0], q[j][1], q[j][2]};                 // D5: no winner
    if (bt[j] >= 0 && closest_out) meshclosest::tri_closest(rec[bt[j]], q[j], c);
    dist2_out[o] = bd[j];
    tri_out[o] = bt[j];
    if (closest_out) { closest_out[3 * o] = c[0]; closest_out[3 * o + 1] = c[1]; closest_out[3 * o + 2] = c[2]; }
  }
}

// measurement only: every lane runs `iters` rounds of eight independent multiply / add chains in registers (16 fp64 operations a round,
// not contracted: the operation mix of the scan)
__global__ __launch_bounds__(MC_BLOCK) void fp64_rate_kernel(int iters, double a, double b, double *__restrict__ sink) {
  double x[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) x[i] = (double)(threadIdx.x + i) * 1e-3;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = x[i] * a + b;
  }
  double s = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += x[i];
  sink[(size_t)blockIdx.x * MC_BLOCK + threadIdx.x] = s;
}

}  // namespace
}  // namespace df

using namespace df;

extern "C" int df_mesh_closest_tile_triangles(void) { return MC_TILE; }

extern "C" size_t df_mesh_closest_scratch_bytes(int T) { return T < 1 ? 0 : (size_t)T * sizeof(TriRec); }

extern "C" int df_mesh_closest(const float *vertices, int V, const int *triangles, int T, const double *points, int P, const double *xf, int K,
                               double *dist2_out, int *tri_out, double *closest_out, void *scratch, size_t scratch_bytes, df_stream_t stream) {
  const char *name = "mesh_closest";
  if (!vertices || !triangles || !points || !xf || !dist2_out || !tri_out || !scratch) return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (V < 1 || T < 1 || P < 1 || K < 1) return set_error(DF_ERR_ARG, "%s: need V, T, P, K >= 1 (V %d, T %d, P %d, K %d)", name, V, T, P, K);
  if (3L * V > INT_MAX || 3L * T > INT_MAX || 12L * K > INT_MAX || 3L * K * P > INT_MAX)
    return set_error(DF_ERR_ARG, "%s: 3 V, 3 T, 12 K and 3 K P must fit an int (V %d, T %d, P %d, K %d)", name, V, T, P, K);
  if (scratch_bytes < df_mesh_closest_scratch_bytes(T) || reinterpret_cast<uintptr_t>(scratch) % 16)
    return set_error(DF_ERR_ARG, "%s: scratch must be 16-byte aligned and hold %zu bytes (got %zu)", name, df_mesh_closest_scratch_bytes(T), scratch_bytes);
  if (reinterpret_cast<uintptr_t>(vertices) % 4 || reinterpret_cast<uintptr_t>(triangles) % 4 || reinterpret_cast<uintptr_t>(tri_out) % 4 ||
      reinterpret_cast<uintptr_t>(points) % 8 || reinterpret_cast<uintptr_t>(xf) % 8 || reinterpret_cast<uintptr_t>(dist2_out) % 8 ||
      reinterpret_cast<uintptr_t>(closest_out) % 8)
    return set_error(DF_ERR_ARG, "%s: vertices, triangles and tri_out must be 4-byte, points, xf, dist2_out and closest_out 8-byte aligned", name);
  hipStream_t st = to_stream(stream);
  TriRec *rec = static_cast<TriRec *>(scratch);
  hipLaunchKernelGGL(mesh_prepare_kernel, dim3(cdiv(T, MESH_PREPARE_BLOCK)), dim3(MESH_PREPARE_BLOCK), 0, st, vertices, V, triangles, T, rec);
  const int whole = cdiv(P, MC_BLOCK * MC_QPL);
  if ((long)whole * K >= MC_FILL) {
    hipLaunchKernelGGL(mesh_scan_kernel<1>, dim3(whole * K), dim3(MC_BLOCK), 0, st, rec, T, points, P, xf, whole, dist2_out, tri_out, closest_out);
  } else {
    const int qblocks = cdiv(P, 64 * MC_QPL);
    hipLaunchKernelGGL(mesh_scan_kernel<MC_WAVES>, dim3(qblocks * K), dim3(MC_BLOCK), 0, st, rec, T, points, P, xf, qblocks, dist2_out, tri_out,
                       closest_out);
  }
  return check_launch(name);
}

extern "C" int df_fp64_rate_probe(int blocks, int iters, double *sink, df_stream_t stream) {
  if (!sink || blocks < 1 || blocks > 65536 || iters < 1) return set_error(DF_ERR_ARG, "fp64_rate_probe: need sink, 1 <= blocks <= 65536, iters >= 1");
  hipLaunchKernelGGL(fp64_rate_kernel, dim3(blocks), dim3(MC_BLOCK), 0, to_stream(stream), iters, 1.0000001, 1e-9, sink);
  return check_launch("fp64_rate_probe");
}
