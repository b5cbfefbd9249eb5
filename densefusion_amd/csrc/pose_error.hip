// df_pose_sym_error: the two symmetry-aware BOP pose errors of B items, MSSD (model space) and MSPD (image plane), in fp64.  The contract
// is the comment of the call in include/dfusion.h (steps E0..E7); the per-item rules are pose_error_core.h; tests/pose_error_np.py restates
// them in numpy and all six columns are compared bit for bit.  Built with -ffp-contract=off: no fused multiply-add anywhere.
//
// The launches of one call, back to back on the caller's stream, after the maxima plane is set to zero:
//   sym_compose_kernel (grid = symmetry blocks x items): E = [R_e | t_e] once per item and G_s = [R_g | t_g] o S_s once per (item, s), into
//   the scratch (E1, E2).
//   sym_error_kernel (grid = vertex blocks x items x symmetry slices): a lane holds PE_VPL vertices of its item with their estimate-side
//   points and pixels (E3, E5: they depend on (item, vertex) only) and loops the symmetries of its slice inside.  E, G_s and the camera
//   are the same in every lane: they are read through uniform addresses, so they sit in scalar registers and cost no vector register
//   and no LDS traffic.  The lane's larger d2 and e2 of the pair go to the workgroup's maxima in LDS, [tile][2] 64-bit integers: a
//   non-negative double orders like its bit pattern, so the maximum is an integer maximum, exact and order-free; a wave reads the slot
//   first and only when one of its lanes is above it reduces its 64 values by shuffles and takes one atomic, which after the first
//   sweep is rare.  After its vertices the workgroup
//   raises the item's plane [B][S_max][2] in the scratch by one integer atomicMax per slot.  The blocks per item are capped so that all
//   items together aim at PE_TARGET_BLOCKS (as verify_raster_kernel's are): the lanes stride over the rest of a large mesh, and where
//   items x vertex blocks leave the part short the symmetry range is cut into slices (gridDim.z).
//   sym_finish_kernel (one wave per item): the smallest maximum over s, the lowest s among equals, the square roots and the row; a bad
//   item's row (E0).
// Integer atomics only: the row of an item depends on its own poses, object, vertices and symmetries, not on the launch shape, B or the
// items next to it.
#include <climits>

#include "common.h"
#include "pose_error_core.h"

namespace df {
namespace {

namespace pe = poseerr;

constexpr int PE_BLOCK = 256;           // threads per workgroup
constexpr int PE_VPL = 2;               // vertices per lane and sweep
constexpr int PE_SYM_TILE = 512;        // symmetries whose maxima a workgroup holds in LDS at a time: 8 KiB
constexpr int PE_MAX_BLOCKS = 256;      // vertex blocks per item
constexpr int PE_TARGET_BLOCKS = 2048;  // workgroups a launch aims at over all items: 8 per compute unit of a 256-CU part
constexpr int PE_MIN_SLICE = 8;         // symmetries a slice holds at least: the estimate side is computed once per slice

// host arrays, passed by value as launch arguments; entries past O repeat the last
struct ErrObjects {
  int O;
  int vertex_begin[pe::MAX_OBJECTS + 1];
  int sym_begin[pe::MAX_OBJECTS + 1];
};

__device__ inline unsigned long long bits(double v) { return (unsigned long long)__double_as_longlong(v); }

// *slot (LDS) = max(*slot, the wave's largest v).  Called by whole waves.  The slot is read first: only a wave with a lane above it
// reduces (a butterfly of shuffles) and takes one atomic; a slot that is read stale costs a reduction too many, never a wrong maximum.
__device__ inline void raise_slot(unsigned long long *slot, unsigned long long v) {
  if (!__any(v > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) return;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(slot, v);
}

// grid = (symmetry blocks of the largest set, B)
__global__ __launch_bounds__(PE_BLOCK) void sym_compose_kernel(ErrObjects objs, const int *__restrict__ obj, const double *__restrict__ sym,
                                                              const double *__restrict__ pose_est, const double *__restrict__ pose_gt,
                                                              int S_max, double *__restrict__ E, double *__restrict__ G) {
  const int b = blockIdx.y, o = obj[b];
  if (pe::item_bad(o, objs.O, objs.vertex_begin, objs.sym_begin)) return;      // E0; the same in every lane of the block
  const int s = blockIdx.x * PE_BLOCK + threadIdx.x;
  if (s >= objs.sym_begin[o + 1] - objs.sym_begin[o]) return;
  double M[12], Gs[12];
  if (s == 0) {                                                                // E1, the estimate
    pe::pose_matrix(pose_est + 7 * (size_t)b, M);
    for (int e = 0; e < 12; ++e) E[12 * (size_t)b + e] = M[e];
  }
  pe::pose_matrix(pose_gt + 7 * (size_t)b, M);                                 // E1, E2
  pe::compose(M, sym + 12 * (size_t)(objs.sym_begin[o] + s), Gs);
  for (int e = 0; e < 12; ++e) G[12 * ((size_t)b * S_max + s) + e] = Gs[e];
}

// grid = (vertex blocks of the largest object, B, symmetry slices)
__global__ __launch_bounds__(PE_BLOCK) void sym_error_kernel(const float *__restrict__ vertices, ErrObjects objs, pe::View view,
                                                            const int *__restrict__ obj, const double *__restrict__ E,
                                                            const double *__restrict__ G, int S_max, unsigned long long *__restrict__ plane) {
  __shared__ unsigned long long best[PE_SYM_TILE * 2];
  const int b = blockIdx.y, o = obj[b];
  if (pe::item_bad(o, objs.O, objs.vertex_begin, objs.sym_begin)) return;      // E0; the same in every lane of the block
  const int v0 = objs.vertex_begin[o], nv = objs.vertex_begin[o + 1] - v0, S = objs.sym_begin[o + 1] - objs.sym_begin[o];
  const long sweep = (long)PE_BLOCK * PE_VPL;
  if (blockIdx.x * sweep >= nv) return;                                        // the grid is sized for the largest object
  const int slice = (S + (int)gridDim.z - 1) / (int)gridDim.z;
  const int s_lo = blockIdx.z * slice, s_hi = s_lo + slice < S ? s_lo + slice : S;
  if (s_lo >= s_hi) return;                                                    // ... and for the largest symmetry set
  const double *Eb = E + 12 * (size_t)b;                                       // uniform addresses: scalar loads
  const double *Gb = G + 12 * (size_t)b * S_max;
  unsigned long long *pb = plane + 2 * (size_t)b * S_max;
  for (int s0 = s_lo; s0 < s_hi; s0 += PE_SYM_TILE) {
    const int nt = s_hi - s0 < PE_SYM_TILE ? s_hi - s0 : PE_SYM_TILE;
    __syncthreads();                                                           // the previous tile's maxima have left
    for (int i = threadIdx.x; i < 2 * nt; i += PE_BLOCK) best[i] = 0;          // +0.0: below or equal to every d2 and e2
    __syncthreads();
    for (long base = blockIdx.x * sweep; base < nv; base += gridDim.x * sweep) {
      double x[PE_VPL][3], p[PE_VPL][3], u[PE_VPL][2];
#pragma unroll
      for (int j = 0; j < PE_VPL; ++j) {
        const long i = base + j * PE_BLOCK + threadIdx.x;
        const float *xf = vertices + 3 * (size_t)(v0 + (i < nv ? i : nv - 1));  // a lane past the end repeats the last vertex: a maximum does not see it
        x[j][0] = (double)xf[0]; x[j][1] = (double)xf[1]; x[j][2] = (double)xf[2];
        pe::transform_query(Eb, x[j], p[j]);                                   // E3
        pe::project(view, p[j], u[j]);                                         // E5
      }
      for (int s = 0; s < nt; ++s) {
        const double *g = Gb + 12 * (size_t)(s0 + s);
        double md = 0.0, me = 0.0;
#pragma unroll
        for (int j = 0; j < PE_VPL; ++j) {
          double d2, e2;
          pe::pair_errors(view, g, x[j], p[j], u[j], &d2, &e2);                // E3..E6
          md = d2 > md ? d2 : md;
          me = e2 > me ? e2 : me;
        }
        raise_slot(&best[2 * s], bits(md));
        raise_slot(&best[2 * s + 1], bits(me));
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * nt; i += PE_BLOCK)
      if (best[i]) atomicMax(&pb[2 * (size_t)s0 + i], best[i]);                // the plane starts at zero
  }
}

// grid = B, one wave per item
__global__ __launch_bounds__(64) void sym_finish_kernel(ErrObjects objs, const int *__restrict__ obj, const unsigned long long *__restrict__ plane,
                                                        int S_max, double *__restrict__ out) {
  const int b = blockIdx.x, o = obj[b], lane = threadIdx.x;
  double *row = out + pe::NOUT * (size_t)b;
  if (pe::item_bad(o, objs.O, objs.vertex_begin, objs.sym_begin)) {
    if (lane == 0) pe::bad_row(row);
    return;
  }
  const int S = objs.sym_begin[o + 1] - objs.sym_begin[o];
  const unsigned long long *pb = plane + 2 * (size_t)b * S_max;
  unsigned long long dk = ~0ull, ek = ~0ull;                                   // above the pattern of +inf: a lane with no s never wins
  int ds = 0, es = 0;
  for (int s = lane; s < S; s += 64) {                                         // ascending s: the lowest keeps a tie
    const unsigned long long kd = pb[2 * (size_t)s], ke = pb[2 * (size_t)s + 1];
    if (kd < dk) { dk = kd; ds = s; }
    if (ke < ek) { ek = ke; es = s; }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long od = __shfl_down(dk, off, 64), oe = __shfl_down(ek, off, 64);
    const int ods = __shfl_down(ds, off, 64), oes = __shfl_down(es, off, 64);
    if (od < dk || (od == dk && ods < ds)) { dk = od; ds = ods; }
    if (oe < ek || (oe == ek && oes < es)) { ek = oe; es = oes; }
  }
  if (lane == 0)                                                               // E7
    pe::write_row(__longlong_as_double((long long)dk), ds, __longlong_as_double((long long)ek), es,
                  objs.vertex_begin[o + 1] - objs.vertex_begin[o], row);
}

inline bool sizes_ok(int B, int S_max) { return B >= 1 && B <= 65535 && S_max >= 1 && 12L * S_max <= INT_MAX; }
inline size_t plane_bytes(int B, int S_max) { return (size_t)B * S_max * 2 * sizeof(unsigned long long); }

// vertex blocks per item: at most PE_MAX_BLOCKS, and PE_TARGET_BLOCKS over all B items
inline int block_cap(int B) {
  const int cap = cdiv(PE_TARGET_BLOCKS, B) < PE_MAX_BLOCKS ? cdiv(PE_TARGET_BLOCKS, B) : PE_MAX_BLOCKS;
  return cap < 1 ? 1 : cap;
}

bool overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

}  // namespace
}  // namespace df

using namespace df;

extern "C" int df_pose_sym_error_sweep_vertices(int B) { return B >= 1 ? block_cap(B) * PE_BLOCK * PE_VPL : 0; }

extern "C" size_t df_pose_sym_error_scratch_bytes(int B, int S_max) {
  if (!sizes_ok(B, S_max)) return 0;
  return plane_bytes(B, S_max) + ((size_t)B * S_max + B) * 12 * sizeof(double);
}

extern "C" int df_pose_sym_error(const float *vertices, int V, const int *vertex_begin, const double *sym, int NS, const int *sym_begin, int O,
                                 const int *obj, const double *pose_est, const double *pose_gt, int B, const double *proj, int IH, int IW,
                                 double *out, void *scratch, size_t scratch_bytes, df_stream_t stream) {
  const char *name = "pose_sym_error";
  if (!vertices || !vertex_begin || !sym || !sym_begin || !obj || !pose_est || !pose_gt || !proj || !out || !scratch)
    return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (V < 1 || NS < 1 || 3L * V > INT_MAX || 12L * NS > INT_MAX)
    return set_error(DF_ERR_ARG, "%s: need V, NS >= 1 with 3 V and 12 NS within an int (V %d, NS %d)", name, V, NS);
  if (B < 1 || B > 65535) return set_error(DF_ERR_ARG, "%s: B = %d outside 1..65535", name, B);
  if (O < 1 || O > pe::MAX_OBJECTS) return set_error(DF_ERR_ARG, "%s: O must be 1..%d (got %d)", name, pe::MAX_OBJECTS, O);
  if (IH < 1 || IW < 1 || (long)IH * IW > (1L << 30)) return set_error(DF_ERR_ARG, "%s: IH x IW = %d x %d outside 1..2^30", name, IH, IW);
  // the renderers' form (V3 reads rows 0, 1 and 3): z' = p22 z + p23 and w' = -z
  if (!(proj[8] == 0.0 && proj[9] == 0.0 && proj[12] == 0.0 && proj[13] == 0.0 && proj[14] == -1.0 && proj[15] == 0.0))
    return set_error(DF_ERR_ARG, "%s: the projection matrix needs rows 2 = (0, 0, p22, p23) and 3 = (0, 0, -1, 0)", name);
  ErrObjects objs;
  objs.O = O;
  int longest = 0, S_max = 0;
  for (int o = 0; o <= pe::MAX_OBJECTS; ++o) {
    const int k = o <= O ? o : O;
    if (vertex_begin[k] < 0 || vertex_begin[k] > V || (k > 0 && vertex_begin[k] < vertex_begin[k - 1]))
      return set_error(DF_ERR_ARG, "%s: vertex_begin must be non-decreasing within 0..V (entry %d is %d, V %d)", name, k, vertex_begin[k], V);
    if (sym_begin[k] < 0 || sym_begin[k] > NS || (k > 0 && sym_begin[k] < sym_begin[k - 1]))
      return set_error(DF_ERR_ARG, "%s: sym_begin must be non-decreasing within 0..NS (entry %d is %d, NS %d)", name, k, sym_begin[k], NS);
    objs.vertex_begin[o] = vertex_begin[k];
    objs.sym_begin[o] = sym_begin[k];
    if (k > 0) {
      longest = vertex_begin[k] - vertex_begin[k - 1] > longest ? vertex_begin[k] - vertex_begin[k - 1] : longest;
      S_max = sym_begin[k] - sym_begin[k - 1] > S_max ? sym_begin[k] - sym_begin[k - 1] : S_max;
    }
  }
  S_max = S_max < 1 ? 1 : S_max;                                               // every object empty: every item is bad, the plane is not read
  const size_t need = df_pose_sym_error_scratch_bytes(B, S_max);
  if (scratch_bytes < need || reinterpret_cast<uintptr_t>(scratch) % 8)
    return set_error(DF_ERR_ARG, "%s: scratch must be 8-byte aligned and hold %zu bytes (got %zu)", name, need, scratch_bytes);
  if (reinterpret_cast<uintptr_t>(vertices) % 4 || reinterpret_cast<uintptr_t>(obj) % 4 || reinterpret_cast<uintptr_t>(sym) % 8 ||
      reinterpret_cast<uintptr_t>(pose_est) % 8 || reinterpret_cast<uintptr_t>(pose_gt) % 8 || reinterpret_cast<uintptr_t>(out) % 8)
    return set_error(DF_ERR_ARG, "%s: vertices and obj must be 4-byte, sym, pose_est, pose_gt and out 8-byte aligned", name);
  const size_t out_b = (size_t)B * pe::NOUT * sizeof(double), pose_b = (size_t)B * 7 * sizeof(double);
  const struct { const void *p; size_t n; } ins[] = {{vertices, (size_t)V * 12}, {sym, (size_t)NS * 96}, {obj, (size_t)B * 4},
                                                     {pose_est, pose_b}, {pose_gt, pose_b}, {scratch, need}};
  for (const auto &in : ins)
    if (overlap(out, out_b, in.p, in.n)) return set_error(DF_ERR_ARG, "%s: out may not overlap the inputs or the scratch", name);

  hipStream_t st = to_stream(stream);
  unsigned long long *plane = static_cast<unsigned long long *>(scratch);
  double *G = reinterpret_cast<double *>(static_cast<char *>(scratch) + plane_bytes(B, S_max));
  double *E = G + 12 * (size_t)B * S_max;
  if (hipMemsetAsync(plane, 0, plane_bytes(B, S_max), st) != hipSuccess) return check_launch(name);
  pe::View view;
  for (int k = 0; k < 4; ++k) { view.p0[k] = proj[k]; view.p1[k] = proj[4 + k]; view.p3[k] = proj[12 + k]; }
  view.ih = (double)IH; view.iw = (double)IW;
  const int lanes = cdiv(longest > 0 ? longest : 1, PE_VPL);
  const int xb = cdiv(lanes, PE_BLOCK) < block_cap(B) ? cdiv(lanes, PE_BLOCK) : block_cap(B);
  int zb = PE_TARGET_BLOCKS / (xb * B);                                        // slices only where vertex blocks x items leave the part short
  zb = zb > cdiv(S_max, PE_MIN_SLICE) ? cdiv(S_max, PE_MIN_SLICE) : zb;
  zb = zb < 1 ? 1 : zb;
  hipLaunchKernelGGL(sym_compose_kernel, dim3(cdiv(S_max, PE_BLOCK), B), dim3(PE_BLOCK), 0, st, objs, obj, sym, pose_est, pose_gt, S_max, E, G);
  hipLaunchKernelGGL(sym_error_kernel, dim3(xb, B, zb), dim3(PE_BLOCK), 0, st, vertices, objs, view, obj, E, G, S_max, plane);
  hipLaunchKernelGGL(sym_finish_kernel, dim3(B), dim3(64), 0, st, objs, obj, plane, S_max, out);
  return check_launch(name);
}
