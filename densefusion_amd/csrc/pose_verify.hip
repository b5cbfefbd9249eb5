// Render-and-compare verification of B estimated poses: each item's CAD mesh is drawn at its pose into a window of its own depth frame and
// compared node by node with the observed depth codes and, optionally, a mask.  The contract is the comment of df_pose_verify in
// include/dfusion.h: P2 is steps V2..V5 and T1..T7 of df_cad_render_mesh through the very device functions of cad_raster_core.h (hence the
// same bits), P0, P1 and P3 are the functions of pose_verify_core.h; tests/pose_verify_np.py restates it in numpy and the twelve tallies
// are compared bit for bit.  Built with -ffp-contract=off: no fused multiply-add anywhere.
//
// Steps on the caller's stream: the keys are set to all-ones and the stats to zero; verify_raster_kernel (grid = triangle blocks of the
// largest object range x items) derives the item's [R | t] once per workgroup (one thread, handed over through LDS), sets up one triangle
// per lane, cuts its node range to the window and walks it into the item's own key plane (walk_triangles: small ranges by the lane, large
// ones by the whole wave); verify_score_kernel (grid = slot blocks x items) reads the key plane once, 8 bytes a lane along the window's
// rows, with the observed code and the mask value of the node, counts the classes per wave with ballots, adds the workgroup's waves in LDS and
// then takes one integer atomic per class and workgroup.  Integer atomics only: two identical calls give identical bytes.
#include "cad_raster_core.h"
#include "mesh_objects.h"
#include "pose_verify_core.h"
#include "pose_dense_core.h"
#include "pose_contour_core.h"
#include "pose_vsd_core.h"

namespace df {
namespace {

namespace pv = poseverify;
namespace vsd = posevsd;
namespace dense = posedense;
namespace contour = posecontour;
static_assert(pv::MAX_OBJECTS == MAX_OBJECTS, "item_bad's objects are those of the object table (mesh_objects.h)");

// Workgroups a launch aims at over all items: 8 per compute unit of a 256-CU part.  The blocks per item are capped at this over B (and
// at RASTER_MAX_BLOCKS / RESOLVE_MAX_BLOCKS); the waves stride over the rest.
constexpr int VERIFY_TARGET_BLOCKS = 2048;

struct Frames {
  const unsigned short *depth, *mask;     // mask may be null
  int F, NM, IH, IW;
};

__device__ inline void load_item(const int *__restrict__ items, int b, int *item) {
#pragma unroll
  for (int k = 0; k < pv::ITEM_INTS; ++k) item[k] = items[(size_t)b * pv::ITEM_INTS + k];
}

// a wave's total of a per-lane count, added to *dst by lane 0 (nothing when it is zero)
__device__ inline void wave_add(unsigned long long v, long long *dst) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(reinterpret_cast<unsigned long long *>(dst), v);
}

__global__ __launch_bounds__(RB) void verify_raster_kernel(const float *__restrict__ vertices, int V, const int *__restrict__ triangles,
                                                           ObjectTable tab, int O, Camera cam, Frames fr,
                                                           const int *__restrict__ items, const double *__restrict__ pose,
                                                           double cloud_div, int WH, int WW, int cull,
                                                           unsigned long long *__restrict__ keys, long long *__restrict__ stats) {
  __shared__ double M[12];
  const int b = blockIdx.y;
  int item[pv::ITEM_INTS];
  load_item(items, b, item);
  if (pv::item_bad(item, fr.F, O, fr.mask != nullptr, fr.NM)) return;         // P0; the same in every lane of the block
  const int o = item[pv::IT_OBJECT];
  const long t0 = tab.begin[o], t1 = tab.begin[o + 1];
  if ((long)blockIdx.x * RB >= t1 - t0) return;                               // the grid is sized for the largest range
  if (threadIdx.x == 0) pv::pose_matrix(pose + (size_t)b * 7, cloud_div, M);  // P1, once per workgroup
  __syncthreads();
  const Pose P = load_pose(M);
  const double scale = tab.scale[o];
  int lo[2], hi[2];
  pv::window_nodes(item[pv::IT_R0], item[pv::IT_C0], WH, WW, fr.IH, fr.IW, lo, hi);
  // node (r, q) of the window is kf[r * WW + q]: raster_node's addressing with IW := WW
  unsigned long long *kf = keys + ((long)b * WH * WW - ((long)item[pv::IT_R0] * WW + item[pv::IT_C0]));
  const int lane = threadIdx.x & 63;
  unsigned long long reached = 0, cut = 0;
  // `base` is the same in all lanes of a wave, so the wave stays whole for the ballots and the shuffles of the walks
  for (long base = t0 + (long)blockIdx.x * RB + (threadIdx.x - lane); base < t1; base += (long)gridDim.x * RB) {
    const long i = base + lane;
    Setup s;
    bool live = i < t1 && load_triangle(s.tri, triangles, i, V);
    if (live) live = setup_triangle(s, vertices, P, scale, cam, fr.IH, fr.IW, cull);
    if (live) {                                                               // P2: the T4 range within the window
      const int r0 = max(s.r0, lo[0]), r1 = min(s.r1, hi[0]), q0 = max(s.q0, lo[1]), q1 = min(s.q1, hi[1]);
      live = r0 <= r1 && q0 <= q1;                                            // emptied: dropped, and not counted as cut
      cut += live && (r0 != s.r0 || r1 != s.r1 || q0 != s.q0 || q1 != s.q1);
      s.r0 = r0; s.r1 = r1; s.q0 = q0; s.q1 = q1;
    }
    reached += walk_triangles(s, live, base, kf, WW);                         // T7: the key carries the global triangle index
  }
  long long *sb = stats + (size_t)b * pv::NSTAT;
  wave_add(reached, sb + pv::ST_TRIANGLES);
  wave_add(cut, sb + pv::ST_CUT);
}

__global__ __launch_bounds__(RB) void verify_score_kernel(const unsigned long long *__restrict__ keys, Frames fr, int O,
                                                          const int *__restrict__ items, int WH, int WW, int tol,
                                                          long long *__restrict__ stats) {
  constexpr int NTALLY = pv::ST_SUM_ABS - pv::ST_RENDERED + 1;                // the nine entries of a row this pass counts
  __shared__ unsigned long long acc[NTALLY];
  const int b = blockIdx.y;
  int item[pv::ITEM_INTS];
  load_item(items, b, item);
  long long *sb = stats + (size_t)b * pv::NSTAT;
  if (pv::item_bad(item, fr.F, O, fr.mask != nullptr, fr.NM)) {               // P0
    if (blockIdx.x == 0 && threadIdx.x == 0) sb[pv::ST_STATUS] = 1;
    return;
  }
  const int slots = WH * WW;                                                  // <= 2^30
  const size_t npix = (size_t)fr.IH * fr.IW;
  const unsigned long long *kb = keys + (size_t)b * slots;
  const unsigned short *df = fr.depth + (size_t)item[pv::IT_FRAME] * npix;
  const unsigned short *mf = fr.mask ? fr.mask + (size_t)item[pv::IT_MASK_FRAME] * npix : nullptr;
  const int r0 = item[pv::IT_R0], c0 = item[pv::IT_C0], mv = item[pv::IT_MASK_VALUE];
  const int lane = threadIdx.x & 63;
  // per-wave counts, the same in every lane (ballots); sum_abs per lane
  unsigned long long n_rend = 0, n_agree = 0, n_front = 0, n_behind = 0, n_missing = 0, n_mask = 0, n_mobs = 0, n_unex = 0, sum_abs = 0;
  for (int base = blockIdx.x * RB + (threadIdx.x - lane); base < slots; base += gridDim.x * RB) {
    const int s = base + lane;
    int r = 0, q = 0;
    const bool exists = s < slots && pv::slot_node(s, r0, c0, WW, fr.IH, fr.IW, &r, &q);
    int cls = pv::NOT_RENDERED, co = pv::NO_OBSERVATION;
    bool m = false;
    if (exists) {
      const int cr = pv::key_code(kb[s]);
      const size_t p = (size_t)r * fr.IW + q;
      co = df[p];
      m = mf && mf[p] == mv;
      cls = pv::classify(cr, co, tol);
      if (cls == pv::AGREE) sum_abs += (unsigned)(co > cr ? co - cr : cr - co);
    }
    n_rend += __popcll(__ballot(cls != pv::NOT_RENDERED));
    n_agree += __popcll(__ballot(cls == pv::AGREE));
    n_front += __popcll(__ballot(cls == pv::FRONT));
    n_behind += __popcll(__ballot(cls == pv::BEHIND));
    n_missing += __popcll(__ballot(cls == pv::MISSING));
    n_mask += __popcll(__ballot(m));
    n_mobs += __popcll(__ballot(m && co != pv::NO_OBSERVATION));
    n_unex += __popcll(__ballot(pv::unexplained(m, co, cls)));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum_abs += __shfl_down(sum_abs, off, 64);
  // the workgroup's four waves meet in LDS (integer adds: any order gives the same sum), then one atomic per non-zero class
  if (threadIdx.x < NTALLY) acc[threadIdx.x] = 0;
  __syncthreads();
  if (lane == 0) {
    const unsigned long long v[NTALLY] = {n_rend, n_agree, n_front, n_behind, n_missing, n_mask, n_mobs, n_unex, sum_abs};
#pragma unroll
    for (int k = 0; k < NTALLY; ++k)
      if (v[k]) atomicAdd(&acc[k], v[k]);
  }
  __syncthreads();
  if (threadIdx.x < NTALLY && acc[threadIdx.x])
    atomicAdd(reinterpret_cast<unsigned long long *>(sb + pv::ST_RENDERED + threadIdx.x), acc[threadIdx.x]);
}

// df_pose_vsd: delta and tau of up to VSD_TABLE_OBJECTS objects, passed by value, written to the table in the scratch
constexpr int VSD_TABLE_OBJECTS = 8;
struct VsdRows {
  double v[VSD_TABLE_OBJECTS][vsd::TABLE_DOUBLES];
};

__global__ void vsd_table_kernel(VsdRows rows, int o0, int n, double *__restrict__ table) {
  const int i = threadIdx.x;
  if (i < n * vsd::TABLE_DOUBLES) table[(size_t)o0 * vsd::TABLE_DOUBLES + i] = rows.v[i / vsd::TABLE_DOUBLES][i % vsd::TABLE_DOUBLES];
}

// S1..S4 of df_pose_vsd: verify_score_kernel's walk over the window slots with two key planes (estimate, truth), the observed code and the
// node's ray; every tally is a ballot count, added per workgroup in LDS and then by one integer atomic per non-zero entry.
__global__ __launch_bounds__(RB) void vsd_score_kernel(const unsigned long long *__restrict__ keys_e, const unsigned long long *__restrict__ keys_g,
                                                       Frames fr, const double *__restrict__ rays, int O, const int *__restrict__ items,
                                                       int WH, int WW, double p22, double p23, const double *__restrict__ table, int NT,
                                                       long long *__restrict__ stats) {
  constexpr int NTALLY = 3 + vsd::MAX_TAU;
  __shared__ unsigned long long acc[NTALLY];
  const int b = blockIdx.y;
  int item[pv::ITEM_INTS];
  load_item(items, b, item);
  long long *sb = stats + (size_t)b * (vsd::ST_BAD + NT);
  if (pv::item_bad(item, fr.F, O, false, 0)) {                                // P0
    if (blockIdx.x == 0 && threadIdx.x == 0) sb[vsd::ST_STATUS] = 1;
    return;
  }
  const int slots = WH * WW;
  const size_t npix = (size_t)fr.IH * fr.IW;
  const unsigned long long *ke = keys_e + (size_t)b * slots, *kg = keys_g + (size_t)b * slots;
  const unsigned short *df = fr.depth + (size_t)item[pv::IT_FRAME] * npix;
  const double *tb = table + (size_t)item[pv::IT_OBJECT] * vsd::TABLE_DOUBLES;
  const double delta = tb[0];
  const int r0 = item[pv::IT_R0], c0 = item[pv::IT_C0];
  const int lane = threadIdx.x & 63;
  unsigned long long n[NTALLY];                                               // per-wave counts, the same in every lane (ballots)
#pragma unroll
  for (int k = 0; k < NTALLY; ++k) n[k] = 0;
  for (int base = blockIdx.x * RB + (threadIdx.x - lane); base < slots; base += gridDim.x * RB) {
    const int s = base + lane;
    int r = 0, q = 0;
    const bool exists = s < slots && pv::slot_node(s, r0, c0, WW, fr.IH, fr.IW, &r, &q);
    bool ve = false, vg = false, re = false;
    double gap = 0.0;
    if (exists) {
      const size_t p = (size_t)r * fr.IW + q;
      const int ce = pv::key_code(ke[s]), cg = pv::key_code(kg[s]);
      const double ray[3] = {rays[3 * p], rays[3 * p + 1], rays[3 * p + 2]};
      vsd::node_visibility(ce, cg, df[p], p22, p23, vsd::ray_length(ray), delta, &ve, &vg, &gap);
      re = ce != pv::NO_CODE;
    }
    n[0] += __popcll(__ballot(ve || vg));
    n[1] += __popcll(__ballot(ve && vg));
    n[2] += __popcll(__ballot(re));
#pragma unroll
    for (int k = 0; k < vsd::MAX_TAU; ++k)
      if (k < NT) n[3 + k] += __popcll(__ballot(ve && vg && gap >= tb[1 + k]));
  }
  if (threadIdx.x < NTALLY) acc[threadIdx.x] = 0;
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NTALLY; ++k)
      if (n[k]) atomicAdd(&acc[k], n[k]);
  }
  __syncthreads();
  if (threadIdx.x < 3 + NT && acc[threadIdx.x])
    atomicAdd(reinterpret_cast<unsigned long long *>(sb + vsd::ST_UNION + threadIdx.x), acc[threadIdx.x]);
}

// ---- df_pose_refine_dense (D1..D6 of its comment in include/dfusion.h; the rules are pose_dense_core.h) ---------------------------------
// The state between the launches lives in the scratch: per item the working pose (7 doubles) and its model frame X with the
// vertex factor (posedense::FRAME_DOUBLES), which the init and the finish kernel write and the accumulation reads through uniform
// addresses (scalar loads); the status is stats[b][0] itself, as in df_mesh_icp.

constexpr int DENSE_POSE_DOUBLES = 7;                  // the raster kernel reads the working poses as a [B][7] array
static_assert(RB == meshicp::LANES, "the accumulation order of D5 is this workgroup's shape");

// S0 and P0: one thread per item
__global__ __launch_bounds__(RB) void dense_init_kernel(const int *__restrict__ items, const double *__restrict__ pose_in, ObjectTable tab,
                                                        int O, int F, int has_mask, int NM, double cloud_div, int B,
                                                        double *__restrict__ work, double *__restrict__ frames,
                                                        double *__restrict__ pose_out, double *__restrict__ stats) {
  const int b = blockIdx.x * RB + threadIdx.x;
  if (b >= B) return;
  int item[pv::ITEM_INTS];
  load_item(items, b, item);
  double p[7], X[12];
  for (int e = 0; e < 7; ++e) p[e] = pose_in[7 * (size_t)b + e];
  meshicp::normalise_quat(p);
  meshicp::model_frame(p, X);
  const bool bad = pv::item_bad(item, F, O, has_mask != 0, NM);
  for (int e = 0; e < 7; ++e) {
    pose_out[7 * (size_t)b + e] = p[e];
    work[DENSE_POSE_DOUBLES * (size_t)b + e] = p[e];
  }
  double *fb = frames + dense::FRAME_DOUBLES * (size_t)b;
  for (int e = 0; e < 12; ++e) fb[e] = X[e];
  fb[12] = bad ? 0.0 : dense::vertex_factor(tab.scale[item[pv::IT_OBJECT]], cloud_div);   // nothing is read through a bad record
  double *s = stats + meshicp::NSTAT * (size_t)b;
  for (int e = 0; e < meshicp::NSTAT; ++e) s[e] = 0.0;
  if (bad) s[meshicp::ST_STATUS] = (double)meshicp::BAD_OBJECT;
}

// D2..D5: grid = (tile blocks, items).  A workgroup takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of its item; lane l adds the
// tile's slots l, l + 256, ... in ascending order onto zero (29 accumulators in registers), the lanes of a wave meet by shuffles, the four
// waves in LDS, and the tile's total goes to its own row of `part` by plain stores: which workgroup took a tile does not show.
__global__ __launch_bounds__(RB) void dense_accum_kernel(const unsigned long long *__restrict__ keys, Frames fr,
                                                         const double *__restrict__ rays, const int *__restrict__ items,
                                                         const float *__restrict__ vertices, int V, const int *__restrict__ triangles, int T,
                                                         const double *__restrict__ frames, const double *__restrict__ stats, int WH,
                                                         int WW, int gate, double p22, double p23, double cloud_div, int ntiles,
                                                         double *__restrict__ part) {
  __shared__ double part_s[RB / 64][dense::NPART];
  const int b = blockIdx.y;
  if (stats[meshicp::NSTAT * (size_t)b + meshicp::ST_STATUS] != 0.0) return;  // frozen or bad item: the whole workgroup leaves
  int item[pv::ITEM_INTS];
  load_item(items, b, item);
  double X[12];
  const double *fb = frames + dense::FRAME_DOUBLES * (size_t)b;
#pragma unroll
  for (int e = 0; e < 12; ++e) X[e] = fb[e];
  const double factor = fb[12];
  const int slots = WH * WW;                                                  // <= 2^30
  const size_t npix = (size_t)fr.IH * fr.IW;
  const unsigned long long *kb = keys + (size_t)b * slots;
  const unsigned short *df = fr.depth + (size_t)item[pv::IT_FRAME] * npix;
  const unsigned short *mf = fr.mask ? fr.mask + (size_t)item[pv::IT_MASK_FRAME] * npix : nullptr;
  const int r0 = item[pv::IT_R0], c0 = item[pv::IT_C0], mv = item[pv::IT_MASK_VALUE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    double acc[meshicp::NSUM];
#pragma unroll
    for (int k = 0; k < meshicp::NSUM; ++k) acc[k] = 0.0;
    int cnt = 0;
    for (int j = 0; j < dense::SWEEPS; ++j) {
      const long long sl = (long long)tile * dense::TILE + j * RB + threadIdx.x;
      int r = 0, q = 0;
      if (sl >= slots || !pv::slot_node((int)sl, r0, c0, WW, fr.IH, fr.IW, &r, &q)) continue;
      const unsigned long long key = kb[sl];
      const size_t p = (size_t)r * fr.IW + q;
      const int co = df[p];
      if (!dense::candidate(pv::key_code(key), co, gate, mf != nullptr, mf && mf[p] == mv)) continue;
      const unsigned t = (unsigned)(key & 0xffffffffull);
      if (t >= (unsigned)T) continue;                                         // not a key of the raster pass: never followed
      const unsigned i0 = triangles[3 * (size_t)t], i1 = triangles[3 * (size_t)t + 1], i2 = triangles[3 * (size_t)t + 2];
      if (i0 >= (unsigned)V || i1 >= (unsigned)V || i2 >= (unsigned)V) continue;
      const double ray[3] = {rays[3 * p], rays[3 * p + 1], rays[3 * p + 2]};
      double x[3], term[meshicp::TERM_DOUBLES];
      dense::observed_point(co, ray, p22, p23, cloud_div, X, x);
      if (!dense::plane_terms(vertices + 3 * (size_t)i0, vertices + 3 * (size_t)i1, vertices + 3 * (size_t)i2, factor, x, term)) continue;
      meshicp::accumulate(term, acc);
      ++cnt;
    }
    // I6's tree over a wave's lanes: at step s lane l < s adds lane l + s (the other lanes' values are not used afterwards)
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
      for (int k = 0; k < meshicp::NSUM; ++k) acc[k] = acc[k] + __shfl_down(acc[k], s);
      cnt += __shfl_down(cnt, s);
    }
    __syncthreads();                                                          // the previous tile's readers are done
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < meshicp::NSUM; ++k) part_s[wave][k] = acc[k];
      part_s[wave][meshicp::NSUM] = (double)cnt;
    }
    __syncthreads();
    if (threadIdx.x < dense::NPART) {
      const int k = threadIdx.x;
      part[((size_t)b * ntiles + tile) * dense::PART_DOUBLES + k] = (part_s[0][k] + part_s[1][k]) + (part_s[2][k] + part_s[3][k]);
    }
  }
}

// D5, D6: grid = B, one wave.  Lane k < 29 adds entry k of the item's tile rows in ascending tile order onto zero; lane 0 then runs
// finish_pass (I6..I9) on the working pose and writes pose_out and the model frame of the next pass.
__global__ __launch_bounds__(64) void dense_finish_kernel(const double *__restrict__ part, int ntiles, int pass, int solve,
                                                          double *__restrict__ work, double *__restrict__ frames,
                                                          double *__restrict__ pose_out, double *__restrict__ stats) {
  __shared__ double sums[dense::NPART];
  const int b = blockIdx.x;
  if (stats[meshicp::NSTAT * (size_t)b + meshicp::ST_STATUS] != 0.0) return;
  if (threadIdx.x < dense::NPART) {
    const double *row = part + (size_t)b * ntiles * dense::PART_DOUBLES + threadIdx.x;
    double s = 0.0;
    for (int t = 0; t < ntiles; ++t) s = s + row[(size_t)t * dense::PART_DOUBLES];
    sums[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double tot[meshicp::NSUM], p[7], X[12];
  for (int k = 0; k < meshicp::NSUM; ++k) tot[k] = sums[k];
  for (int e = 0; e < 7; ++e) p[e] = work[DENSE_POSE_DOUBLES * (size_t)b + e];
  meshicp::finish_pass(tot, (int)sums[meshicp::NSUM], pass, solve, p, stats + meshicp::NSTAT * (size_t)b);
  meshicp::model_frame(p, X);
  for (int e = 0; e < 7; ++e) {
    work[DENSE_POSE_DOUBLES * (size_t)b + e] = p[e];
    pose_out[7 * (size_t)b + e] = p[e];
  }
  for (int e = 0; e < 12; ++e) frames[dense::FRAME_DOUBLES * (size_t)b + e] = X[e];
}

// ---- df_pose_refine_contour (E1..E6 of its comment in include/dfusion.h; the rules are pose_contour_core.h) -----------------------------
// The dense call's launches as they stand, with a status row of their own stride ([B][6], in the scratch) that the finish copies into the
// caller's [B][8] rows.  Once per call the observed outline and its feature map; per pass an accumulation of the outline pairs with the
// dense one's shape, into a second set of tile rows.

// the caller's rows after S0: the six dense columns and no pairs
__global__ __launch_bounds__(RB) void contour_stats_kernel(const double *__restrict__ stats6, int B, double *__restrict__ stats) {
  const int b = blockIdx.x * RB + threadIdx.x;
  if (b >= B) return;
  for (int e = 0; e < contour::NSTAT; ++e) stats[contour::NSTAT * (size_t)b + e] = e < meshicp::NSTAT ? stats6[meshicp::NSTAT * (size_t)b + e] : 0.0;
}

// the node at (wr, wc) of an item's window as E1 sees it: wr, wc may lie outside the window
__device__ inline contour::Node observed_node(const unsigned short *__restrict__ df, const unsigned short *__restrict__ mf, int mv, int IH, int IW,
                                              int r0, int c0, int WH, int WW, int wr, int wc) {
  contour::Node n = {false, false, pv::NO_OBSERVATION};
  const long long r = (long long)r0 + wr, q = (long long)c0 + wc;
  if (wr < 0 || wr >= WH || wc < 0 || wc >= WW || r < 0 || r >= IH || q < 0 || q >= IW) return n;
  const size_t p = (size_t)r * IW + (size_t)q;
  n.exists = true;
  n.code = df[p];
  n.on = n.code != pv::NO_OBSERVATION && (!mf || mf[p] == mv);
  return n;
}

// E1 and E2's first pass: grid = (strip blocks, items).  A workgroup takes row strips of 256 columns: the outline flags of the strip and
// of `reach` columns on either side go to LDS (each from the node's code and its four neighbours'), then lane l finds the nearest flagged
// column to its own.  g: [B][WH][WW] int32.
__global__ __launch_bounds__(RB) void contour_rows_kernel(Frames fr, const int *__restrict__ items, const double *__restrict__ stats6, int WH, int WW,
                                                          int edge_step, int reach, int *__restrict__ g) {
  __shared__ unsigned char flag_s[contour::STRIP + 2 * contour::MAX_REACH];
  const int b = blockIdx.y;
  if (stats6[meshicp::NSTAT * (size_t)b + meshicp::ST_STATUS] != 0.0) return;  // a bad item: nothing is read through its record
  int item[pv::ITEM_INTS];
  load_item(items, b, item);
  const size_t npix = (size_t)fr.IH * fr.IW;
  const unsigned short *df = fr.depth + (size_t)item[pv::IT_FRAME] * npix;
  const unsigned short *mf = fr.mask ? fr.mask + (size_t)item[pv::IT_MASK_FRAME] * npix : nullptr;
  const int r0 = item[pv::IT_R0], c0 = item[pv::IT_C0], mv = item[pv::IT_MASK_VALUE];
  const int chunks = (WW + contour::STRIP - 1) / contour::STRIP;
  const long long strips = (long long)WH * chunks;                            // <= 2^30
  int *gb = g + (size_t)b * WH * WW;
  for (long long s = blockIdx.x; s < strips; s += gridDim.x) {
    const int wr = (int)(s / chunks), first = (int)(s - (long long)wr * chunks) * contour::STRIP - reach;
    __syncthreads();                                                          // the previous strip's readers are done
    for (int i = threadIdx.x; i < contour::STRIP + 2 * reach; i += RB) {
      const int wc = first + i;
      const contour::Node c = observed_node(df, mf, mv, fr.IH, fr.IW, r0, c0, WH, WW, wr, wc);
      bool edge = false;
      if (c.on) {
        const contour::Node nb[4] = {observed_node(df, mf, mv, fr.IH, fr.IW, r0, c0, WH, WW, wr - 1, wc),
                                     observed_node(df, mf, mv, fr.IH, fr.IW, r0, c0, WH, WW, wr + 1, wc),
                                     observed_node(df, mf, mv, fr.IH, fr.IW, r0, c0, WH, WW, wr, wc - 1),
                                     observed_node(df, mf, mv, fr.IH, fr.IW, r0, c0, WH, WW, wr, wc + 1)};
        edge = contour::outline(c, nb, edge_step);
      }
      flag_s[i] = edge ? 1 : 0;
    }
    __syncthreads();
    const int wc = first + reach + (int)threadIdx.x;
    if (wc < WW) gb[(size_t)wr * WW + wc] = contour::row_nearest(flag_s, first, wc, reach, WW);
  }
}

// E2's second pass: a lane per window slot, along the rows, so that a wave reads 64 neighbouring columns of each row it scans
__global__ __launch_bounds__(RB) void contour_columns_kernel(const int *__restrict__ g, Frames fr, const int *__restrict__ items,
                                                             const double *__restrict__ stats6, int WH, int WW, int reach,
                                                             int *__restrict__ feat) {
  const int b = blockIdx.y;
  if (stats6[meshicp::NSTAT * (size_t)b + meshicp::ST_STATUS] != 0.0) return;
  int item[pv::ITEM_INTS];
  load_item(items, b, item);
  const int slots = WH * WW;                                                  // <= 2^30
  const int *gb = g + (size_t)b * slots;
  int *fb = feat + (size_t)b * slots;
  for (long long s = (long long)blockIdx.x * RB + threadIdx.x; s < slots; s += (long long)gridDim.x * RB) {
    int r = 0, q = 0;
    const int wr = (int)(s / WW), wc = (int)(s - (long long)wr * WW);
    fb[s] = pv::slot_node((int)s, item[pv::IT_R0], item[pv::IT_C0], WW, fr.IH, fr.IW, &r, &q) ? contour::column_nearest(gb, WH, WW, wr, wc, reach)
                                                                                                : contour::NONE;
  }
}

// the node at (wr, wc) of an item's window as E3 sees it, from the key plane
__device__ inline contour::Node drawn_node(const unsigned long long *__restrict__ kb, int IH, int IW, int r0, int c0, int WH, int WW, int wr,
                                           int wc) {
  contour::Node n = {false, false, pv::NO_CODE};
  const long long r = (long long)r0 + wr, q = (long long)c0 + wc;
  if (wr < 0 || wr >= WH || wc < 0 || wc >= WW || r < 0 || r >= IH || q < 0 || q >= IW) return n;
  n.exists = true;
  n.code = pv::key_code(kb[(size_t)wr * WW + wc]);
  n.on = n.code != pv::NO_CODE;
  return n;
}

// E3..E5: dense_accum_kernel's shape and order (tile blocks x items, lane l takes a tile's slots l, l + 256, .. in ascending order, I6's
// tree by shuffles, the four waves in LDS, a plain store of the tile's row), over the outline pairs: a drawn-outline node reads its
// feature, the two codes and the two rays, and adds its two terms, k = 0 first.
__global__ __launch_bounds__(RB) void contour_accum_kernel(const unsigned long long *__restrict__ keys, const int *__restrict__ feat, Frames fr,
                                                           const double *__restrict__ rays, const int *__restrict__ items,
                                                           const double *__restrict__ frames, const double *__restrict__ stats6, int WH, int WW,
                                                           int edge_step, double contour_scale, double p22, double p23, double cloud_div,
                                                           int ntiles, double *__restrict__ part) {
  __shared__ double part_s[RB / 64][dense::NPART];
  const int b = blockIdx.y;
  if (stats6[meshicp::NSTAT * (size_t)b + meshicp::ST_STATUS] != 0.0) return;
  int item[pv::ITEM_INTS];
  load_item(items, b, item);
  double X[12];
  const double *fb = frames + dense::FRAME_DOUBLES * (size_t)b;
#pragma unroll
  for (int e = 0; e < 12; ++e) X[e] = fb[e];
  const int slots = WH * WW;                                                  // <= 2^30
  const size_t npix = (size_t)fr.IH * fr.IW;
  const unsigned long long *kb = keys + (size_t)b * slots;
  const int *eb = feat + (size_t)b * slots;
  const unsigned short *df = fr.depth + (size_t)item[pv::IT_FRAME] * npix;
  const int r0 = item[pv::IT_R0], c0 = item[pv::IT_C0];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    double acc[meshicp::NSUM];
#pragma unroll
    for (int k = 0; k < meshicp::NSUM; ++k) acc[k] = 0.0;
    int cnt = 0;
    for (int j = 0; j < dense::SWEEPS; ++j) {
      const long long sl = (long long)tile * dense::TILE + j * RB + threadIdx.x;
      if (sl >= slots) continue;
      const int wr = (int)(sl / WW), wc = (int)(sl - (long long)wr * WW);
      const contour::Node c = drawn_node(kb, fr.IH, fr.IW, r0, c0, WH, WW, wr, wc);
      if (!c.on) continue;
      const contour::Node nb[4] = {drawn_node(kb, fr.IH, fr.IW, r0, c0, WH, WW, wr - 1, wc), drawn_node(kb, fr.IH, fr.IW, r0, c0, WH, WW, wr + 1, wc),
                                   drawn_node(kb, fr.IH, fr.IW, r0, c0, WH, WW, wr, wc - 1), drawn_node(kb, fr.IH, fr.IW, r0, c0, WH, WW, wr, wc + 1)};
      if (!contour::outline(c, nb, edge_step)) continue;
      const int e = eb[sl];
      int re = 0, qe = 0;
      if (e < 0 || e >= slots || !pv::slot_node(e, r0, c0, WW, fr.IH, fr.IW, &re, &qe)) continue;   // none; the rest never holds for a feature
      const size_t pc = (size_t)((long long)r0 + wr) * fr.IW + (size_t)((long long)c0 + wc), pe = (size_t)re * fr.IW + qe;
      const double ray_c[3] = {rays[3 * pc], rays[3 * pc + 1], rays[3 * pc + 2]};
      const double ray_e[3] = {rays[3 * pe], rays[3 * pe + 1], rays[3 * pe + 2]};
      double term[contour::PAIR_TERMS * meshicp::TERM_DOUBLES];
      if (!contour::pair_terms(c.code, ray_c, df[pe], ray_e, p22, p23, cloud_div, X, contour_scale, term)) continue;
      meshicp::accumulate(term, acc);
      meshicp::accumulate(term + meshicp::TERM_DOUBLES, acc);
      ++cnt;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
      for (int k = 0; k < meshicp::NSUM; ++k) acc[k] = acc[k] + __shfl_down(acc[k], s);
      cnt += __shfl_down(cnt, s);
    }
    __syncthreads();                                                          // the previous tile's readers are done
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < meshicp::NSUM; ++k) part_s[wave][k] = acc[k];
      part_s[wave][meshicp::NSUM] = (double)cnt;
    }
    __syncthreads();
    if (threadIdx.x < dense::NPART) {
      const int k = threadIdx.x;
      part[((size_t)b * ntiles + tile) * dense::PART_DOUBLES + k] = (part_s[0][k] + part_s[1][k]) + (part_s[2][k] + part_s[3][k]);
    }
  }
}

// E5, E6: dense_finish_kernel with two row sets: lane k < 29 adds entry k of the plane rows and, separately, of the outline rows in
// ascending tile order onto zero; lane 0 forms S = P + C, runs finish_pass with P's count on the item's own six columns and copies them,
// with the pass's pairs, into the caller's row.
__global__ __launch_bounds__(64) void contour_finish_kernel(const double *__restrict__ part, const double *__restrict__ cpart, int ntiles, int pass,
                                                            int solve, double *__restrict__ work, double *__restrict__ frames,
                                                            double *__restrict__ pose_out, double *__restrict__ stats6,
                                                            double *__restrict__ stats) {
  __shared__ double sums[2][dense::NPART];
  const int b = blockIdx.x;
  if (stats6[meshicp::NSTAT * (size_t)b + meshicp::ST_STATUS] != 0.0) return;
  if (threadIdx.x < dense::NPART) {
    const size_t at = (size_t)b * ntiles * dense::PART_DOUBLES + threadIdx.x;
    double sp = 0.0, sc = 0.0;
    for (int t = 0; t < ntiles; ++t) sp = sp + part[at + (size_t)t * dense::PART_DOUBLES];
    for (int t = 0; t < ntiles; ++t) sc = sc + cpart[at + (size_t)t * dense::PART_DOUBLES];
    sums[0][threadIdx.x] = sp;
    sums[1][threadIdx.x] = sc;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double tot[meshicp::NSUM], p[7], X[12];
  contour::add_sums(sums[0], sums[1], tot);
  for (int e = 0; e < 7; ++e) p[e] = work[DENSE_POSE_DOUBLES * (size_t)b + e];
  double *s6 = stats6 + meshicp::NSTAT * (size_t)b, *s8 = stats + contour::NSTAT * (size_t)b;
  meshicp::finish_pass(tot, (int)sums[0][meshicp::NSUM], pass, solve, p, s6);
  meshicp::model_frame(p, X);
  for (int e = 0; e < 7; ++e) {
    work[DENSE_POSE_DOUBLES * (size_t)b + e] = p[e];
    pose_out[7 * (size_t)b + e] = p[e];
  }
  for (int e = 0; e < 12; ++e) frames[dense::FRAME_DOUBLES * (size_t)b + e] = X[e];
  for (int e = 0; e < meshicp::NSTAT; ++e) s8[e] = s6[e];
  if (pass == 0) s8[contour::ST_FIRST_PAIRS] = sums[1][meshicp::NSUM];
  s8[contour::ST_LAST_PAIRS] = sums[1][meshicp::NSUM];
}

inline bool window_ok(int B, int WH, int WW) { return B >= 1 && B <= 65535 && WH >= 1 && WW >= 1 && (long)WH * WW <= (1L << 30); }

// blocks per item of a launch over `items` lanes' worth of work per item
inline int item_blocks(long items, int B, int max_blocks) {
  const int cap = cdiv(VERIFY_TARGET_BLOCKS, B) < max_blocks ? cdiv(VERIFY_TARGET_BLOCKS, B) : max_blocks;
  return grid_blocks(items, cap < 1 ? 1 : cap);
}

}  // namespace
}  // namespace df

using namespace df;

extern "C" size_t df_pose_verify_scratch_bytes(int B, int WH, int WW) {
  return window_ok(B, WH, WW) ? (size_t)B * WH * WW * sizeof(unsigned long long) : 0;
}

extern "C" int df_pose_verify(const float *vertices, int V, const int *triangles, int T, const int *tri_begin, const double *model_scale,
                              int O, const double *proj, const unsigned short *depth, int F, int IH, int IW, const unsigned short *mask,
                              int NM, const int *items, const double *pose, double cloud_div, int B, int WH, int WW, int tol, int cull,
                              long long *stats, void *scratch, size_t scratch_bytes, df_stream_t stream) {
  const char *name = "pose_verify";
  if (!vertices || !triangles || !tri_begin || !model_scale || !proj || !depth || !items || !pose || !stats || !scratch)
    return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (mask && NM < 1) return set_error(DF_ERR_ARG, "%s: a mask needs NM >= 1 frames, got %d", name, NM);
  if (!objects_ok(O)) return set_error(DF_ERR_ARG, "%s: O = %d objects outside 1..%d", name, O, MAX_OBJECTS);
  if (V <= 0 || T <= 0 || !sizes_ok(F, IH, IW)) return set_error(DF_ERR_ARG, "%s: bad sizes", name);
  if (!window_ok(B, WH, WW)) return set_error(DF_ERR_ARG, "%s: B = %d outside 1..65535 or WH x WW = %d x %d outside 1..2^30", name, B, WH, WW);
  if (tol < 0 || tol > 65535) return set_error(DF_ERR_ARG, "%s: tol %d outside 0..65535", name, tol);
  if (cull != 0 && cull != 1) return set_error(DF_ERR_ARG, "%s: cull %d is neither 0 nor 1", name, cull);
  if (!(cloud_div > 0.0 && cloud_div - cloud_div == 0.0)) return set_error(DF_ERR_ARG, "%s: cloud_div must be finite and > 0", name);
  if (int e = check_scratch_and_proj(name, scratch, scratch_bytes, df_pose_verify_scratch_bytes(B, WH, WW), proj)) return e;
  int longest = 0;
  if (int e = check_tri_begin(name, tri_begin, O, T, &longest)) return e;
  hipStream_t st = to_stream(stream);
  const long slots = (long)WH * WW;
  if (hipMemsetAsync(scratch, 0xff, (size_t)B * slots * sizeof(unsigned long long), st) != hipSuccess ||
      hipMemsetAsync(stats, 0, sizeof(long long) * pv::NSTAT * B, st) != hipSuccess)
    return check_launch(name);
  unsigned long long *keys = static_cast<unsigned long long *>(scratch);
  const Frames fr = {depth, mask, F, NM, IH, IW};
  const int tb = item_blocks(longest, B, RASTER_MAX_BLOCKS), xb = item_blocks(slots, B, RESOLVE_MAX_BLOCKS);
  hipLaunchKernelGGL(verify_raster_kernel, dim3(tb, B), dim3(RB), 0, st, vertices, V, triangles,
                     make_object_table(tri_begin, model_scale, O, T), O, make_camera(proj), fr, items, pose, cloud_div, WH, WW, cull, keys, stats);
  hipLaunchKernelGGL(verify_score_kernel, dim3(xb, B), dim3(RB), 0, st, keys, fr, O, items, WH, WW, tol, stats);
  return check_launch(name);
}

// the parts of df_pose_vsd's scratch: two key planes of B windows, the raster passes' own tallies (not reported), the object table
static size_t vsd_keys_bytes(int B, int WH, int WW) { return 2 * (size_t)B * WH * WW * sizeof(unsigned long long); }
static size_t vsd_side_bytes(int B) { return (size_t)B * pv::NSTAT * sizeof(long long); }

extern "C" size_t df_pose_vsd_scratch_bytes(int B, int WH, int WW) {
  if (!window_ok(B, WH, WW)) return 0;
  return vsd_keys_bytes(B, WH, WW) + vsd_side_bytes(B) + (size_t)MAX_OBJECTS * vsd::TABLE_DOUBLES * sizeof(double);
}

extern "C" int df_pose_vsd(const float *vertices, int V, const int *triangles, int T, const int *tri_begin, const double *model_scale, int O,
                           const double *proj, const unsigned short *depth, int F, int IH, int IW, const double *rays, const int *items,
                           const double *pose_est, const double *pose_gt, double cloud_div, const double *delta, const double *tau, int NT,
                           int B, int WH, int WW, int cull, long long *stats, void *scratch, size_t scratch_bytes, df_stream_t stream) {
  const char *name = "pose_vsd";
  if (!vertices || !triangles || !tri_begin || !model_scale || !proj || !depth || !rays || !items || !pose_est || !pose_gt || !delta || !tau ||
      !stats || !scratch)
    return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (!objects_ok(O)) return set_error(DF_ERR_ARG, "%s: O = %d objects outside 1..%d", name, O, MAX_OBJECTS);
  if (V <= 0 || T <= 0 || !sizes_ok(F, IH, IW)) return set_error(DF_ERR_ARG, "%s: bad sizes", name);
  if (!window_ok(B, WH, WW)) return set_error(DF_ERR_ARG, "%s: B = %d outside 1..65535 or WH x WW = %d x %d outside 1..2^30", name, B, WH, WW);
  if (NT < 1 || NT > vsd::MAX_TAU) return set_error(DF_ERR_ARG, "%s: NT = %d outside 1..%d", name, NT, vsd::MAX_TAU);
  if (cull != 0 && cull != 1) return set_error(DF_ERR_ARG, "%s: cull %d is neither 0 nor 1", name, cull);
  if (!(cloud_div > 0.0 && cloud_div - cloud_div == 0.0)) return set_error(DF_ERR_ARG, "%s: cloud_div must be finite and > 0", name);
  for (int o = 0; o < O; ++o) {
    if (!(delta[o] >= 0.0 && delta[o] - delta[o] == 0.0)) return set_error(DF_ERR_ARG, "%s: delta[%d] must be finite and >= 0", name, o);
    for (int k = 0; k < NT; ++k)
      if (!(tau[(size_t)o * NT + k] >= 0.0) || (k > 0 && !(tau[(size_t)o * NT + k] >= tau[(size_t)o * NT + k - 1])))
        return set_error(DF_ERR_ARG, "%s: tau of object %d must be >= 0 and ascending", name, o);
  }
  if (reinterpret_cast<uintptr_t>(rays) % 8 || reinterpret_cast<uintptr_t>(stats) % 8)
    return set_error(DF_ERR_ARG, "%s: rays and stats must be 8-byte aligned", name);
  if (int e = check_scratch_and_proj(name, scratch, scratch_bytes, df_pose_vsd_scratch_bytes(B, WH, WW), proj)) return e;
  int longest = 0;
  if (int e = check_tri_begin(name, tri_begin, O, T, &longest)) return e;
  hipStream_t st = to_stream(stream);
  const long slots = (long)WH * WW;
  unsigned long long *keys_e = static_cast<unsigned long long *>(scratch), *keys_g = keys_e + (size_t)B * slots;
  long long *side = reinterpret_cast<long long *>(static_cast<char *>(scratch) + vsd_keys_bytes(B, WH, WW));
  double *table = reinterpret_cast<double *>(reinterpret_cast<char *>(side) + vsd_side_bytes(B));
  if (hipMemsetAsync(scratch, 0xff, vsd_keys_bytes(B, WH, WW), st) != hipSuccess ||
      hipMemsetAsync(side, 0, vsd_side_bytes(B), st) != hipSuccess ||
      hipMemsetAsync(stats, 0, sizeof(long long) * (vsd::ST_BAD + NT) * B, st) != hipSuccess)
    return check_launch(name);
  for (int o0 = 0; o0 < O; o0 += VSD_TABLE_OBJECTS) {
    VsdRows rows;
    const int n = O - o0 < VSD_TABLE_OBJECTS ? O - o0 : VSD_TABLE_OBJECTS;
    for (int j = 0; j < VSD_TABLE_OBJECTS; ++j)
      for (int k = 0; k < vsd::TABLE_DOUBLES; ++k)
        rows.v[j][k] = j >= n ? 0.0 : (k == 0 ? delta[o0 + j] : (k - 1 < NT ? tau[(size_t)(o0 + j) * NT + k - 1] : 0.0));
    hipLaunchKernelGGL(vsd_table_kernel, dim3(1), dim3(RB), 0, st, rows, o0, n, table);
  }
  const Frames fr = {depth, nullptr, F, 0, IH, IW};
  const int tb = item_blocks(longest, B, RASTER_MAX_BLOCKS), xb = item_blocks(slots, B, RESOLVE_MAX_BLOCKS);
  const ObjectTable tab = make_object_table(tri_begin, model_scale, O, T);
  const Camera cam = make_camera(proj);
  // P0..P2 of df_pose_verify, verbatim, once per pose array: the same kernel, its own key plane
  hipLaunchKernelGGL(verify_raster_kernel, dim3(tb, B), dim3(RB), 0, st, vertices, V, triangles, tab, O, cam, fr, items, pose_est, cloud_div, WH, WW,
                     cull, keys_e, side);
  hipLaunchKernelGGL(verify_raster_kernel, dim3(tb, B), dim3(RB), 0, st, vertices, V, triangles, tab, O, cam, fr, items, pose_gt, cloud_div, WH, WW,
                     cull, keys_g, side);
  hipLaunchKernelGGL(vsd_score_kernel, dim3(xb, B), dim3(RB), 0, st, keys_e, keys_g, fr, rays, O, items, WH, WW, cam.p22, cam.p23, table, NT, stats);
  return check_launch(name);
}

// the parts of df_pose_refine_dense's scratch, one after another (each a multiple of 8 bytes): the key plane of B windows, the raster
// pass's own tallies (not reported), the working poses, the model frames, a row per (item, tile)
namespace {
struct DenseScratch {
  size_t keys, side, work, frames, part, total;
};
DenseScratch dense_scratch(int B, int WH, int WW) {
  DenseScratch s;
  s.keys = (size_t)B * WH * WW * sizeof(unsigned long long);
  s.side = (size_t)B * pv::NSTAT * sizeof(long long);
  s.work = (size_t)B * DENSE_POSE_DOUBLES * sizeof(double);
  s.frames = (size_t)B * dense::FRAME_DOUBLES * sizeof(double);
  s.part = (size_t)B * dense::tile_count((long long)WH * WW) * dense::PART_DOUBLES * sizeof(double);
  s.total = s.keys + s.side + s.work + s.frames + s.part;
  return s;
}
bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return b != nullptr && x < y + nb && y < x + na;
}
}  // namespace

extern "C" size_t df_pose_refine_dense_scratch_bytes(int B, int WH, int WW) {
  return window_ok(B, WH, WW) ? dense_scratch(B, WH, WW).total : 0;
}

extern "C" int df_pose_refine_dense(const float *vertices, int V, const int *triangles, int T, const int *tri_begin, const double *model_scale,
                                    int O, const double *proj, const unsigned short *depth, int F, int IH, int IW, const double *rays,
                                    const unsigned short *mask, int NM, const int *items, const double *pose_in, double cloud_div, int B,
                                    int WH, int WW, int gate, int cull, int iters, double *pose_out, double *stats, void *scratch,
                                    size_t scratch_bytes, df_stream_t stream) {
  const char *name = "pose_refine_dense";
  if (!vertices || !triangles || !tri_begin || !model_scale || !proj || !depth || !rays || !items || !pose_in || !pose_out || !stats || !scratch)
    return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (mask && NM < 1) return set_error(DF_ERR_ARG, "%s: a mask needs NM >= 1 frames, got %d", name, NM);
  if (!objects_ok(O)) return set_error(DF_ERR_ARG, "%s: O = %d objects outside 1..%d", name, O, MAX_OBJECTS);
  if (V <= 0 || T <= 0 || !sizes_ok(F, IH, IW)) return set_error(DF_ERR_ARG, "%s: bad sizes", name);
  if (!window_ok(B, WH, WW)) return set_error(DF_ERR_ARG, "%s: B = %d outside 1..65535 or WH x WW = %d x %d outside 1..2^30", name, B, WH, WW);
  if (gate < 0 || gate > dense::MAX_GATE) return set_error(DF_ERR_ARG, "%s: gate %d outside 0..%d", name, gate, dense::MAX_GATE);
  if (iters < 0 || iters > meshicp::MAX_ITERS) return set_error(DF_ERR_ARG, "%s: iters %d outside 0..%d", name, iters, meshicp::MAX_ITERS);
  if (cull != 0 && cull != 1) return set_error(DF_ERR_ARG, "%s: cull %d is neither 0 nor 1", name, cull);
  if (!(cloud_div > 0.0 && cloud_div - cloud_div == 0.0)) return set_error(DF_ERR_ARG, "%s: cloud_div must be finite and > 0", name);
  if (reinterpret_cast<uintptr_t>(rays) % 8 || reinterpret_cast<uintptr_t>(pose_in) % 8 || reinterpret_cast<uintptr_t>(pose_out) % 8 ||
      reinterpret_cast<uintptr_t>(stats) % 8)
    return set_error(DF_ERR_ARG, "%s: rays, pose_in, pose_out and stats must be 8-byte aligned", name);
  const DenseScratch lay = dense_scratch(B, WH, WW);
  if (int e = check_scratch_and_proj(name, scratch, scratch_bytes, lay.total, proj)) return e;
  int longest = 0;
  if (int e = check_tri_begin(name, tri_begin, O, T, &longest)) return e;
  const size_t npix = (size_t)IH * IW, pose_b = (size_t)B * 7 * sizeof(double), stats_b = (size_t)B * meshicp::NSTAT * sizeof(double);
  const struct { const void *p; size_t n; } ins[] = {{vertices, (size_t)V * 12}, {triangles, (size_t)T * 12}, {depth, (size_t)F * npix * 2},
                                                     {mask, (size_t)(mask ? NM : 0) * npix * 2}, {rays, npix * 24},
                                                     {items, (size_t)B * pv::ITEM_INTS * 4}, {pose_in, pose_b}, {scratch, lay.total}};
  for (const auto &in : ins)
    if (ranges_overlap(pose_out, pose_b, in.p, in.n) || ranges_overlap(stats, stats_b, in.p, in.n))
      return set_error(DF_ERR_ARG, "%s: pose_out and stats may not overlap the inputs or the scratch", name);
  if (ranges_overlap(pose_out, pose_b, stats, stats_b)) return set_error(DF_ERR_ARG, "%s: pose_out and stats overlap", name);

  hipStream_t st = to_stream(stream);
  const long slots = (long)WH * WW;
  char *base = static_cast<char *>(scratch);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(base);
  long long *side = reinterpret_cast<long long *>(base + lay.keys);
  double *work = reinterpret_cast<double *>(base + lay.keys + lay.side);
  double *frames = reinterpret_cast<double *>(base + lay.keys + lay.side + lay.work);
  double *part = reinterpret_cast<double *>(base + lay.keys + lay.side + lay.work + lay.frames);
  const Frames fr = {depth, mask, F, NM, IH, IW};
  const ObjectTable tab = make_object_table(tri_begin, model_scale, O, T);
  const Camera cam = make_camera(proj);
  const int ntiles = dense::tile_count(slots);
  // the tile blocks of an item: the cap of the score kernels, in tiles
  int cap = cdiv(VERIFY_TARGET_BLOCKS, B) < RESOLVE_MAX_BLOCKS ? cdiv(VERIFY_TARGET_BLOCKS, B) : RESOLVE_MAX_BLOCKS;
  cap = cap < 1 ? 1 : cap;
  const int tb = item_blocks(longest, B, RASTER_MAX_BLOCKS), xb = ntiles < cap ? ntiles : cap;
  if (hipMemsetAsync(side, 0, lay.side, st) != hipSuccess) return check_launch(name);
  hipLaunchKernelGGL(dense_init_kernel, dim3(cdiv(B, RB)), dim3(RB), 0, st, items, pose_in, tab, O, F, mask ? 1 : 0, NM, cloud_div, B, work, frames,
                     pose_out, stats);
  for (int pass = 0; pass <= iters; ++pass) {
    if (hipMemsetAsync(keys, 0xff, lay.keys, st) != hipSuccess) return check_launch(name);
    // D1: P1, P2 of df_pose_verify, verbatim, from the working poses
    hipLaunchKernelGGL(verify_raster_kernel, dim3(tb, B), dim3(RB), 0, st, vertices, V, triangles, tab, O, cam, fr, items, work, cloud_div, WH, WW,
                       cull, keys, side);
    hipLaunchKernelGGL(dense_accum_kernel, dim3(xb, B), dim3(RB), 0, st, keys, fr, rays, items, vertices, V, triangles, T, frames, stats, WH, WW, gate,
                       cam.p22, cam.p23, cloud_div, ntiles, part);
    hipLaunchKernelGGL(dense_finish_kernel, dim3(B), dim3(64), 0, st, part, ntiles, pass, pass < iters ? 1 : 0, work, frames, pose_out, stats);
  }
  return check_launch(name);
}

// the parts of df_pose_refine_contour's scratch: the dense call's, in its order; the six dense columns of every item at the stride the
// dense kernels read a status through; the feature map, one int32 per window slot (rounded up to 8 bytes); a second row per (item, tile).
// The first pass of the feature transform keeps its plane in the key planes, which no pass has drawn into yet.
namespace {
struct ContourScratch {
  DenseScratch dense;
  size_t stats6, feat, cpart, total;
};
ContourScratch contour_scratch(int B, int WH, int WW) {
  ContourScratch s;
  s.dense = dense_scratch(B, WH, WW);
  s.stats6 = (size_t)B * meshicp::NSTAT * sizeof(double);
  s.feat = (((size_t)B * WH * WW * sizeof(int) + 7) / 8) * 8;
  s.cpart = s.dense.part;
  s.total = s.dense.total + s.stats6 + s.feat + s.cpart;
  return s;
}
}  // namespace

extern "C" size_t df_pose_refine_contour_scratch_bytes(int B, int WH, int WW) {
  return window_ok(B, WH, WW) ? contour_scratch(B, WH, WW).total : 0;
}

extern "C" int df_pose_refine_contour(const float *vertices, int V, const int *triangles, int T, const int *tri_begin, const double *model_scale,
                                      int O, const double *proj, const unsigned short *depth, int F, int IH, int IW, const double *rays,
                                      const unsigned short *mask, int NM, const int *items, const double *pose_in, double cloud_div, int B,
                                      int WH, int WW, int gate, int cull, int iters, int edge_step, int reach, double contour_scale,
                                      double *pose_out, double *stats, void *scratch, size_t scratch_bytes, df_stream_t stream) {
  const char *name = "pose_refine_contour";
  if (!vertices || !triangles || !tri_begin || !model_scale || !proj || !depth || !rays || !items || !pose_in || !pose_out || !stats || !scratch)
    return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (mask && NM < 1) return set_error(DF_ERR_ARG, "%s: a mask needs NM >= 1 frames, got %d", name, NM);
  if (!objects_ok(O)) return set_error(DF_ERR_ARG, "%s: O = %d objects outside 1..%d", name, O, MAX_OBJECTS);
  if (V <= 0 || T <= 0 || !sizes_ok(F, IH, IW)) return set_error(DF_ERR_ARG, "%s: bad sizes", name);
  if (!window_ok(B, WH, WW)) return set_error(DF_ERR_ARG, "%s: B = %d outside 1..65535 or WH x WW = %d x %d outside 1..2^30", name, B, WH, WW);
  if (gate < 0 || gate > dense::MAX_GATE) return set_error(DF_ERR_ARG, "%s: gate %d outside 0..%d", name, gate, dense::MAX_GATE);
  if (iters < 0 || iters > meshicp::MAX_ITERS) return set_error(DF_ERR_ARG, "%s: iters %d outside 0..%d", name, iters, meshicp::MAX_ITERS);
  if (cull != 0 && cull != 1) return set_error(DF_ERR_ARG, "%s: cull %d is neither 0 nor 1", name, cull);
  if (edge_step < 0 || edge_step > contour::MAX_EDGE_STEP)
    return set_error(DF_ERR_ARG, "%s: edge_step %d outside 0..%d", name, edge_step, contour::MAX_EDGE_STEP);
  if (reach < 0 || reach > contour::MAX_REACH) return set_error(DF_ERR_ARG, "%s: reach %d outside 0..%d", name, reach, contour::MAX_REACH);
  if (!(contour_scale >= 0.0 && contour_scale - contour_scale == 0.0))
    return set_error(DF_ERR_ARG, "%s: contour_scale must be finite and >= 0", name);
  if (!(cloud_div > 0.0 && cloud_div - cloud_div == 0.0)) return set_error(DF_ERR_ARG, "%s: cloud_div must be finite and > 0", name);
  if (reinterpret_cast<uintptr_t>(rays) % 8 || reinterpret_cast<uintptr_t>(pose_in) % 8 || reinterpret_cast<uintptr_t>(pose_out) % 8 ||
      reinterpret_cast<uintptr_t>(stats) % 8)
    return set_error(DF_ERR_ARG, "%s: rays, pose_in, pose_out and stats must be 8-byte aligned", name);
  const ContourScratch lay = contour_scratch(B, WH, WW);
  if (int e = check_scratch_and_proj(name, scratch, scratch_bytes, lay.total, proj)) return e;
  int longest = 0;
  if (int e = check_tri_begin(name, tri_begin, O, T, &longest)) return e;
  const size_t npix = (size_t)IH * IW, pose_b = (size_t)B * 7 * sizeof(double), stats_b = (size_t)B * contour::NSTAT * sizeof(double);
  const struct { const void *p; size_t n; } ins[] = {{vertices, (size_t)V * 12}, {triangles, (size_t)T * 12}, {depth, (size_t)F * npix * 2},
                                                     {mask, (size_t)(mask ? NM : 0) * npix * 2}, {rays, npix * 24},
                                                     {items, (size_t)B * pv::ITEM_INTS * 4}, {pose_in, pose_b}, {scratch, lay.total}};
  for (const auto &in : ins)
    if (ranges_overlap(pose_out, pose_b, in.p, in.n) || ranges_overlap(stats, stats_b, in.p, in.n))
      return set_error(DF_ERR_ARG, "%s: pose_out and stats may not overlap the inputs or the scratch", name);
  if (ranges_overlap(pose_out, pose_b, stats, stats_b)) return set_error(DF_ERR_ARG, "%s: pose_out and stats overlap", name);

  hipStream_t st = to_stream(stream);
  const long slots = (long)WH * WW;
  const DenseScratch &dl = lay.dense;
  char *base = static_cast<char *>(scratch);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(base);
  long long *side = reinterpret_cast<long long *>(base + dl.keys);
  double *work = reinterpret_cast<double *>(base + dl.keys + dl.side);
  double *frames = reinterpret_cast<double *>(base + dl.keys + dl.side + dl.work);
  double *part = reinterpret_cast<double *>(base + dl.keys + dl.side + dl.work + dl.frames);
  double *stats6 = reinterpret_cast<double *>(base + dl.total);
  int *feat = reinterpret_cast<int *>(base + dl.total + lay.stats6);
  double *cpart = reinterpret_cast<double *>(base + dl.total + lay.stats6 + lay.feat);
  int *rows = reinterpret_cast<int *>(keys);                                  // the first feature pass's plane: B * slots int32
  const Frames fr = {depth, mask, F, NM, IH, IW};
  const ObjectTable tab = make_object_table(tri_begin, model_scale, O, T);
  const Camera cam = make_camera(proj);
  const int ntiles = dense::tile_count(slots);
  int cap = cdiv(VERIFY_TARGET_BLOCKS, B) < RESOLVE_MAX_BLOCKS ? cdiv(VERIFY_TARGET_BLOCKS, B) : RESOLVE_MAX_BLOCKS;
  cap = cap < 1 ? 1 : cap;
  const int tb = item_blocks(longest, B, RASTER_MAX_BLOCKS), xb = ntiles < cap ? ntiles : cap;
  const long strips = (long)WH * cdiv(WW, contour::STRIP);
  const int sb = (int)(strips < cap ? strips : cap), cb = item_blocks(slots, B, RESOLVE_MAX_BLOCKS);
  if (hipMemsetAsync(side, 0, dl.side, st) != hipSuccess) return check_launch(name);
  hipLaunchKernelGGL(dense_init_kernel, dim3(cdiv(B, RB)), dim3(RB), 0, st, items, pose_in, tab, O, F, mask ? 1 : 0, NM, cloud_div, B, work, frames,
                     pose_out, stats6);
  hipLaunchKernelGGL(contour_stats_kernel, dim3(cdiv(B, RB)), dim3(RB), 0, st, stats6, B, stats);
  // E1, E2, once per call
  hipLaunchKernelGGL(contour_rows_kernel, dim3(sb, B), dim3(RB), 0, st, fr, items, stats6, WH, WW, edge_step, reach, rows);
  hipLaunchKernelGGL(contour_columns_kernel, dim3(cb, B), dim3(RB), 0, st, rows, fr, items, stats6, WH, WW, reach, feat);
  for (int pass = 0; pass <= iters; ++pass) {
    if (hipMemsetAsync(keys, 0xff, dl.keys, st) != hipSuccess) return check_launch(name);
    // D1..D5 as they stand, then E3..E5 over the same key plane
    hipLaunchKernelGGL(verify_raster_kernel, dim3(tb, B), dim3(RB), 0, st, vertices, V, triangles, tab, O, cam, fr, items, work, cloud_div, WH, WW,
                       cull, keys, side);
    hipLaunchKernelGGL(dense_accum_kernel, dim3(xb, B), dim3(RB), 0, st, keys, fr, rays, items, vertices, V, triangles, T, frames, stats6, WH, WW, gate,
                       cam.p22, cam.p23, cloud_div, ntiles, part);
    hipLaunchKernelGGL(contour_accum_kernel, dim3(xb, B), dim3(RB), 0, st, keys, feat, fr, rays, items, frames, stats6, WH, WW, edge_step,
                       contour_scale, cam.p22, cam.p23, cloud_div, ntiles, cpart);
    hipLaunchKernelGGL(contour_finish_kernel, dim3(B), dim3(64), 0, st, part, cpart, ntiles, pass, pass < iters ? 1 : 0, work, frames, pose_out,
                       stats6, stats);
  }
  return check_launch(name);
}
