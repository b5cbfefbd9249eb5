// Pose hypotheses from depth alone by point-pair-feature voting (Drost et al. 2010): df_ppf_model_sizes / df_ppf_model_build (host) and
// df_pose_ppf (device).  The contract is their comment in include/dfusion.h; every rule is a function of pose_ppf_core.h, called here
// and by the model builder alike; tests/pose_ppf_np.py restates the call in numpy and every output is compared bit for bit.  Built with
// -ffp-contract=off: no fused multiply-add anywhere.
//
// Steps on the caller's stream: the outputs are set to zero; ppf_scene_kernel (grid = node blocks x items) writes point, normal and the
// usable flag of every grid node to the scratch; ppf_vote_kernel (grid = references x items, one workgroup per accumulator) zeroes its
// accumulator [NM_o][NA] in dynamic LDS (up to 150 KiB: one workgroup per compute unit above 80 KiB), strides its lanes over the grid
// nodes, and per node walks the bucket of the pair's key with LDS integer atomics: a bucket of up to SHORT_BUCKET entries by the lane
// that owns the node, a longer one by the whole wave, 64 entries a sweep (flat models put thousands of entries under one key; integer
// adds in any order give the same counts).  Item record, reference and tables are addressed by blockIdx only.  The winner is a 64-bit
// maximum (shuffles, then one LDS atomic per wave), and thread 0 turns it into the hypothesis: the pose kernel is the vote kernel's
// tail.  ppf_cluster_kernel (grid = items) ranks the hypotheses by counting in LDS, runs the greedy pass in rank order with the lanes
// spread over the clusters founded so far (the first cluster that fits is an LDS integer minimum), and picks the K best by K maxima.
// Integer atomics only: two identical calls give identical bytes.
#include <algorithm>
#include <climits>

#include "cad_frame.h"
#include "pose_ppf_model.h"

namespace df {
namespace {

namespace pv = poseverify;
namespace ppf = poseppf;
static_assert(pv::MAX_OBJECTS == ppf::MAX_OBJECTS, "item_bad's objects are those of the model table");

constexpr int VOTE_LANES = 1024;                       // 16 waves: above 80 KiB of LDS one workgroup owns the compute unit
constexpr int SHORT_BUCKET = 16;                      // entries a lane walks alone; a longer bucket is the whole wave's
constexpr int CLUSTER_LANES = 256;
constexpr int CLUSTER_SLOT_BYTES = 24;                // per reference in the cluster kernel's LDS: score (8), votes, order, founder, members

struct Src {
  const unsigned short *depth, *mask;                 // mask may be null
  const double *rays;
  int F, NM, IH, IW;
};

// point_begin, dist_step and cluster_dist of the objects, by value
struct Model {
  double dist_step[ppf::MAX_OBJECTS], cluster_dist[ppf::MAX_OBJECTS];
  int begin[ppf::MAX_OBJECTS + 1];
};

struct Grid {
  int GH, GW, step, reach, gate, ref_step, RW, NR;
};

__device__ inline void load_item(const int *__restrict__ items, int b, int *item) {
#pragma unroll
  for (int k = 0; k < pv::ITEM_INTS; ++k) item[k] = items[(size_t)b * pv::ITEM_INTS + k];
}

// the code of node (r, q) when it lies in the frame and, with a mask, the mask holds the item's value there; NO_OBSERVATION otherwise
__device__ inline int node_code(const Src &s, const unsigned short *df, const unsigned short *mf, int mv, long long r, long long q) {
  if (r < 0 || r >= s.IH || q < 0 || q >= s.IW) return pv::NO_OBSERVATION;
  const size_t p = (size_t)r * s.IW + (size_t)q;
  if (mf && mf[p] != mv) return pv::NO_OBSERVATION;
  return df[p];
}

// N1, N2: one lane per grid node; every slot of a good item is written
__global__ __launch_bounds__(RB) void ppf_scene_kernel(Src s, const int *__restrict__ items, int O, double p22, double p23, double cloud_div,
                                                       Grid gd, double *__restrict__ scene) {
  const int b = blockIdx.y;
  int item[pv::ITEM_INTS];
  load_item(items, b, item);
  if (pv::item_bad(item, s.F, O, s.mask != nullptr, s.NM)) return;
  const int G = gd.GH * gd.GW, g = blockIdx.x * RB + threadIdx.x;
  if (g >= G) return;
  const size_t npix = (size_t)s.IH * s.IW;
  const unsigned short *df = s.depth + (size_t)item[pv::IT_FRAME] * npix;
  const unsigned short *mf = s.mask ? s.mask + (size_t)item[pv::IT_MASK_FRAME] * npix : nullptr;
  const int mv = item[pv::IT_MASK_VALUE];
  const int gr = g / gd.GW, gc = g - gr * gd.GW;
  const long long r = (long long)item[pv::IT_R0] + (long long)gr * gd.step, q = (long long)item[pv::IT_C0] + (long long)gc * gd.step;
  double out[ppf::SCENE_DOUBLES] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const int co = node_code(s, df, mf, mv, r, q);
  if (co != pv::NO_OBSERVATION) {
    const long long nr[4] = {r, r, r - gd.reach, r + gd.reach}, nq[4] = {q - gd.reach, q + gd.reach, q, q};
    double p[3], nb[4][3], nh[3];
    bool has[4];
    const size_t at = (size_t)r * s.IW + (size_t)q;
    ppf::scene_point(co, s.rays + 3 * at, p22, p23, cloud_div, p);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int cn = node_code(s, df, mf, mv, nr[k], nq[k]);
      has[k] = ppf::neighbour_counts(cn, co, gd.gate);
      nb[k][0] = nb[k][1] = nb[k][2] = 0.0;
      if (has[k]) ppf::scene_point(cn, s.rays + 3 * ((size_t)nr[k] * s.IW + (size_t)nq[k]), p22, p23, cloud_div, nb[k]);
    }
    if (ppf::scene_normal(p, nb[0], has[0], nb[1], has[1], nb[2], has[2], nb[3], has[3], nh)) {
      out[0] = p[0]; out[1] = p[1]; out[2] = p[2]; out[3] = nh[0]; out[4] = nh[1]; out[5] = nh[2]; out[6] = 1.0;
    }
  }
  double *dst = scene + ((size_t)b * G + g) * ppf::SCENE_DOUBLES;
#pragma unroll
  for (int k = 0; k < ppf::SCENE_DOUBLES; ++k) dst[k] = out[k];
}

// V1..V3, H1..H3: one workgroup per (item, reference)
__global__ __launch_bounds__(VOTE_LANES) void ppf_vote_kernel(const double *__restrict__ scene, const int *__restrict__ items, Model mod,
                                                              ppf::Tables tb, int F, int O, int has_mask, int NMm,
                                                              const double *__restrict__ mpoints, const double *__restrict__ mnormals,
                                                              const int *__restrict__ bucket_begin, const int *__restrict__ entry_point,
                                                              const float2 *__restrict__ entry_cs, int n_entries, Grid gd,
                                                              double *__restrict__ rows, double *__restrict__ hyp_out,
                                                              unsigned long long *__restrict__ visited) {
  extern __shared__ unsigned acc[];
  __shared__ unsigned long long best;
  const int b = blockIdx.y, ri = blockIdx.x, tid = threadIdx.x;
  int item[pv::ITEM_INTS];
  load_item(items, b, item);
  if (pv::item_bad(item, F, O, has_mask != 0, NMm)) return;                  // nothing reads the rows of a bad item
  const int o = item[pv::IT_OBJECT];
  const int m0 = mod.begin[o], nm = mod.begin[o + 1] - m0, NA = tb.NA, cells = nm * NA;
  const int G = gd.GH * gd.GW;
  const int gref = (ri / gd.RW) * gd.ref_step * gd.GW + (ri % gd.RW) * gd.ref_step;
  const double *sb = scene + (size_t)b * G * ppf::SCENE_DOUBLES;
  const double *ref = sb + (size_t)gref * ppf::SCENE_DOUBLES;
  double *row = rows + ((size_t)b * gd.NR + ri) * ppf::ROW_DOUBLES;
  if (ref[6] == 0.0) {                                                       // an unusable reference: no hypothesis
    if (tid < ppf::ROW_DOUBLES) row[tid] = 0.0;
    return;
  }
  const double ps[3] = {ref[0], ref[1], ref[2]}, ns[3] = {ref[3], ref[4], ref[5]};
  double Rs[9];
  ppf::frame_rot(ns, Rs);
  for (int c = tid; c < cells; c += VOTE_LANES) acc[c] = 0u;
  if (tid == 0) best = 0ull;
  __syncthreads();
  const size_t kb = (size_t)o * ((size_t)tb.ND * tb.NANG * tb.NANG * tb.NANG + 1);
  const double ds = mod.dist_step[o];
  const int lane = tid & 63;
  unsigned long long walked = 0ull;                                          // the entries of this lane's nodes, whoever walks them
  // `base` is the same in all lanes of a wave, so the wave stays whole for the ballot and the shuffles
  for (int base = tid - lane; base < G; base += VOTE_LANES) {
    const int g = base + lane;
    int e0 = 0, e1 = 0;
    double cs[2] = {0.0, 0.0};
    if (g < G && g != gref) {
      const double *sp = sb + (size_t)g * ppf::SCENE_DOUBLES;
      if (sp[6] != 0.0) {
        const double p2[3] = {sp[0], sp[1], sp[2]}, n2[3] = {sp[3], sp[4], sp[5]};
        const int key = ppf::pair_key(ps, ns, p2, n2, ds, tb);
        if (key >= 0 && ppf::frame_angle(Rs, ps, p2, cs)) {
          e0 = bucket_begin[kb + key];
          e1 = bucket_begin[kb + key + 1];
          if (e0 < 0 || e1 > n_entries || e0 > e1) e0 = e1 = 0;              // not a table of the builder: never followed
        }
      }
    }
    const bool mine = e1 - e0 <= SHORT_BUCKET;
    walked += (unsigned)(e1 - e0);
    unsigned long long longs = __ballot(!mine);
    while (longs) {                                                          // a long bucket: the whole wave, 64 entries a sweep
      const int l = __ffsll((long long)longs) - 1;
      longs &= longs - 1;
      const int w1 = __shfl(e1, l);
      const double wc = __shfl(cs[0], l), ws = __shfl(cs[1], l);
      for (int e = __shfl(e0, l) + lane; e < w1; e += 64) {
        const unsigned i = (unsigned)entry_point[e];
        const float2 m = entry_cs[e];
        if (i < (unsigned)nm) atomicAdd(&acc[i * NA + ppf::sector((double)m.x, (double)m.y, wc, ws, tb)], 1u);
      }
    }
    if (mine)
      for (int e = e0; e < e1; ++e) {
        const unsigned i = (unsigned)entry_point[e];
        const float2 m = entry_cs[e];
        if (i < (unsigned)nm) atomicAdd(&acc[i * NA + ppf::sector((double)m.x, (double)m.y, cs[0], cs[1], tb)], 1u);
      }
  }
  __syncthreads();
  unsigned long long k = 0ull;                                               // V3: 0 = no vote at all
  for (int c = tid; c < cells; c += VOTE_LANES) {
    const unsigned n = acc[c];
    if (n) {
      const unsigned long long kk = ppf::winner_key(n, c);
      k = kk > k ? kk : k;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_down(k, off, 64);
    k = other > k ? other : k;
    walked += __shfl_down(walked, off, 64);
  }
  if (lane == 0 && k) atomicMax(&best, k);
  if (lane == 0 && walked) atomicAdd(&visited[b], walked);                   // the bench's count: one integer atomic a wave
  __syncthreads();
  if (tid != 0) return;
  double out[ppf::ROW_DOUBLES];
  for (int e = 0; e < ppf::ROW_DOUBLES; ++e) out[e] = 0.0;
  const unsigned long long w = best;
  if (ppf::winner_count(w) > 0) {
    const int cell = ppf::winner_cell(w), i = cell / NA, bin = cell - i * NA;
    const double *pm = mpoints + 3 * (size_t)(m0 + i), *nmv = mnormals + 3 * (size_t)(m0 + i);
    const double pmv[3] = {pm[0], pm[1], pm[2]}, nmm[3] = {nmv[0], nmv[1], nmv[2]};
    ppf::hypothesis_pose(ps, ns, pmv, nmm, tb.alpha_cs[bin][0], tb.alpha_cs[bin][1], out);
    out[7] = (double)ppf::winner_count(w);
    meshicp::quat_to_mat(out, out + ppf::HYP_DOUBLES);
    if (hyp_out)
      for (int e = 0; e < ppf::HYP_DOUBLES; ++e) hyp_out[((size_t)b * gd.NR + ri) * ppf::HYP_DOUBLES + e] = out[e];
  }
  for (int e = 0; e < ppf::ROW_DOUBLES; ++e) row[e] = out[e];
}

// C1..C3: one workgroup per item
__global__ __launch_bounds__(CLUSTER_LANES) void ppf_cluster_kernel(const double *__restrict__ rows, const double *__restrict__ scene,
                                                                    const int *__restrict__ items, Model mod, int F, int O, int has_mask,
                                                                    int NMm, int G, int NR, int K, double trace_min,
                                                                    double *__restrict__ pose_out, int *__restrict__ votes_out,
                                                                    double *__restrict__ stats) {
  extern __shared__ unsigned long long score[];                              // [NR] per cluster, then the four int arrays
  __shared__ int s_usable, s_hyps, s_found;
  __shared__ unsigned long long s_best;
  unsigned *votes = reinterpret_cast<unsigned *>(score + NR);                // [NR] per reference
  int *order = reinterpret_cast<int *>(votes + NR);                          // [NR] rank -> reference
  int *founder = order + NR;                                                 // [NR] per cluster: the reference of its first member
  int *members = founder + NR;                                               // [NR] per cluster
  const int b = blockIdx.x, tid = threadIdx.x;
  int item[pv::ITEM_INTS];
  load_item(items, b, item);
  double *sb = stats + (size_t)b * ppf::NSTAT;
  if (pv::item_bad(item, F, O, has_mask != 0, NMm)) {
    if (tid == 0) sb[ppf::ST_STATUS] = (double)ppf::BAD_ITEM;
    return;
  }
  const double cd = mod.cluster_dist[item[pv::IT_OBJECT]], dist2 = cd * cd;
  const double *rb = rows + (size_t)b * NR * ppf::ROW_DOUBLES;
  if (tid == 0) { s_usable = 0; s_hyps = 0; }
  for (int i = tid; i < NR; i += CLUSTER_LANES) votes[i] = (unsigned)rb[(size_t)i * ppf::ROW_DOUBLES + 7];
  __syncthreads();
  int usable = 0;
  for (int g = tid; g < G; g += CLUSTER_LANES) usable += scene[((size_t)b * G + g) * ppf::SCENE_DOUBLES + 6] != 0.0 ? 1 : 0;
  if (usable) atomicAdd(&s_usable, usable);
  // C1: the rank of a hypothesis = the number of those ahead of it (more votes, or as many and a lower reference)
  for (int i = tid; i < NR; i += CLUSTER_LANES) {
    const unsigned v = votes[i];
    if (!v) continue;
    int rank = 0;
    for (int j = 0; j < NR; ++j) rank += (votes[j] > v || (votes[j] == v && j < i)) ? 1 : 0;
    order[rank] = i;
    atomicAdd(&s_hyps, 1);
  }
  __syncthreads();
  const int NH = s_hyps;
  int nc = 0;                                                                // the same in every lane
  for (int h = 0; h < NH; ++h) {                                             // C2: sequential in rank order
    const int i = order[h];
    const double *hr = rb + (size_t)i * ppf::ROW_DOUBLES;
    if (tid == 0) s_found = INT_MAX;
    __syncthreads();
    for (int c = tid; c < nc; c += CLUSTER_LANES) {
      const double *fr = rb + (size_t)founder[c] * ppf::ROW_DOUBLES;
      if (ppf::cluster_near(hr + ppf::HYP_DOUBLES, hr + 4, fr + ppf::HYP_DOUBLES, fr + 4, trace_min, dist2)) atomicMin(&s_found, c);
    }
    __syncthreads();
    const int f = s_found;
    if (tid == 0) {
      if (f == INT_MAX) { founder[nc] = i; score[nc] = votes[i]; members[nc] = 1; }
      else { score[f] += votes[i]; members[f] += 1; }
    }
    nc += f == INT_MAX ? 1 : 0;
    __syncthreads();
  }
  for (int k = 0; k < K; ++k) {                                              // C3: the best cluster not yet taken (a taken one scores 0)
    if (tid == 0) s_best = 0ull;
    __syncthreads();
    unsigned long long mine = 0ull;
    for (int c = tid; c < nc; c += CLUSTER_LANES)
      if (score[c]) {
        const unsigned long long key = (score[c] << 12) | (unsigned long long)(ppf::MAX_REFS - 1 - c);
        mine = key > mine ? key : mine;
      }
    if (mine) atomicMax(&s_best, mine);
    __syncthreads();
    const unsigned long long w = s_best;
    if (tid == 0 && w) {
      const int c = ppf::MAX_REFS - 1 - (int)(w & (unsigned long long)(ppf::MAX_REFS - 1));
      const double *fr = rb + (size_t)founder[c] * ppf::ROW_DOUBLES;
      for (int e = 0; e < 7; ++e) pose_out[((size_t)b * K + k) * 7 + e] = fr[e];
      votes_out[((size_t)b * K + k) * 2] = score[c] > (unsigned long long)INT_MAX ? INT_MAX : (int)score[c];
      votes_out[((size_t)b * K + k) * 2 + 1] = members[c];
      score[c] = 0ull;
    }
    __syncthreads();
  }
  if (tid == 0) {
    sb[ppf::ST_STATUS] = (double)(NH > 0 ? ppf::OK : ppf::NO_HYPOTHESIS);
    sb[ppf::ST_USABLE] = (double)s_usable;
    sb[ppf::ST_HYPOTHESES] = (double)NH;
    sb[ppf::ST_CLUSTERS] = (double)nc;
  }
}

bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return a != nullptr && b != nullptr && x < y + nb && y < x + na;
}

bool descending_cosines(const double *t, int n) {
  for (int i = 0; i < n; ++i)
    if (!(t[i] < 1.0 && t[i] > -1.0) || (i > 0 && !(t[i] < t[i - 1]))) return false;
  return true;
}

// the refusals the builder and the call share: the bin counts, the angle table, point_begin and dist_step
int check_model(const char *name, int NM, const int *point_begin, const double *dist_step, int O, int ND, int NANG, int NA,
                const double *ang_cos) {
  if (O < 1 || O > ppf::MAX_OBJECTS) return set_error(DF_ERR_ARG, "%s: O = %d objects outside 1..%d", name, O, ppf::MAX_OBJECTS);
  if (ND < 1 || ND > ppf::MAX_ND || NANG < 1 || NANG > ppf::MAX_NANG || NA < 2 || NA > ppf::MAX_NA || NA % 2)
    return set_error(DF_ERR_ARG, "%s: need ND in 1..%d, NANG in 1..%d and an even NA in 2..%d (got %d, %d, %d)", name, ppf::MAX_ND,
                     ppf::MAX_NANG, ppf::MAX_NA, ND, NANG, NA);
  if (!descending_cosines(ang_cos, NANG - 1)) return set_error(DF_ERR_ARG, "%s: ang_cos must descend strictly inside (-1, 1)", name);
  if (NM < 1 || 3L * NM > INT_MAX || point_begin[0] != 0 || point_begin[O] != NM)
    return set_error(DF_ERR_ARG, "%s: point_begin must run from 0 to NM = %d", name, NM);
  for (int o = 0; o < O; ++o) {
    const long n = (long)point_begin[o + 1] - point_begin[o];
    if (n < ppf::MIN_MODEL_POINTS || n > ppf::MAX_MODEL_POINTS || n * NA * 4 > ppf::MAX_ACC_BYTES)
      return set_error(DF_ERR_ARG, "%s: object %d has %ld model points: need %d..%d and points x NA x 4 <= %d bytes of LDS", name, o, n,
                       ppf::MIN_MODEL_POINTS, ppf::MAX_MODEL_POINTS, ppf::MAX_ACC_BYTES);
    if (!(dist_step[o] > 0.0 && dist_step[o] - dist_step[o] == 0.0))
      return set_error(DF_ERR_ARG, "%s: dist_step[%d] must be finite and > 0", name, o);
  }
  return DF_OK;
}

using ppf::key_count;

struct PpfScratch {
  size_t scene, rows, visited, total;
};
bool ppf_sizes_ok(int B, int WH, int WW, int step, int ref_step) {
  if (B < 1 || B > 65535 || WH < 1 || WW < 1 || (long)WH * WW > (1L << 30)) return false;
  if (step < 1 || step > ppf::MAX_STEP || ref_step < 1 || ref_step > ppf::MAX_STEP) return false;
  const long GH = ppf::grid_side(WH, step), GW = ppf::grid_side(WW, step);
  if (GH * GW > ppf::MAX_GRID) return false;
  return (long)ppf::grid_side((int)GH, ref_step) * ppf::grid_side((int)GW, ref_step) <= ppf::MAX_REFS;
}
PpfScratch ppf_scratch(int B, int WH, int WW, int step, int ref_step) {
  const int GH = ppf::grid_side(WH, step), GW = ppf::grid_side(WW, step);
  PpfScratch s;
  s.scene = (size_t)B * GH * GW * ppf::SCENE_DOUBLES * sizeof(double);
  s.rows = (size_t)B * ppf::grid_side(GH, ref_step) * ppf::grid_side(GW, ref_step) * ppf::ROW_DOUBLES * sizeof(double);
  s.visited = (size_t)B * sizeof(unsigned long long);
  s.total = s.scene + s.rows + s.visited;
  return s;
}

}  // namespace
}  // namespace df

using namespace df;

extern "C" int df_ppf_model_sizes(const int *point_begin, int O, int ND, int NANG, size_t *buckets, size_t *entries) {
  const char *name = "ppf_model_sizes";
  if (!point_begin || !buckets || !entries) return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (O < 1 || O > ppf::MAX_OBJECTS || ND < 1 || ND > ppf::MAX_ND || NANG < 1 || NANG > ppf::MAX_NANG)
    return set_error(DF_ERR_ARG, "%s: need O in 1..%d, ND in 1..%d, NANG in 1..%d", name, ppf::MAX_OBJECTS, ppf::MAX_ND, ppf::MAX_NANG);
  size_t pairs = 0;
  for (int o = 0; o < O; ++o) {
    const long n = (long)point_begin[o + 1] - point_begin[o];
    if (n < ppf::MIN_MODEL_POINTS || n > ppf::MAX_MODEL_POINTS)
      return set_error(DF_ERR_ARG, "%s: object %d has %ld model points outside %d..%d", name, o, n, ppf::MIN_MODEL_POINTS, ppf::MAX_MODEL_POINTS);
    pairs += (size_t)n * (size_t)(n - 1);
  }
  const size_t nb = (size_t)O * (key_count(ND, NANG) + 1);
  if (nb > (size_t)INT_MAX || pairs > (size_t)INT_MAX) return set_error(DF_ERR_ARG, "%s: the table does not fit 32-bit offsets", name);
  *buckets = nb;
  *entries = pairs;
  return DF_OK;
}

extern "C" int df_ppf_model_build(const double *points, const double *normals, int NM, const int *point_begin, const double *dist_step, int O,
                                  int ND, int NANG, int NA, const double *ang_cos, int *bucket_begin, int *entry_point, float *entry_cs,
                                  size_t *used) {
  const char *name = "ppf_model_build";
  if (!points || !normals || !point_begin || !dist_step || !ang_cos || !bucket_begin || !entry_point || !entry_cs || !used)
    return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (int e = check_model(name, NM, point_begin, dist_step, O, ND, NANG, NA, ang_cos)) return e;
  size_t nb = 0, cap = 0;
  if (int e = df_ppf_model_sizes(point_begin, O, ND, NANG, &nb, &cap)) return e;
  ppf::Tables tb = {};
  tb.ND = ND; tb.NANG = NANG; tb.NA = NA;
  for (int i = 0; i < NANG - 1; ++i) tb.ang_cos[i] = ang_cos[i];
  *used = ppf::build_model(points, normals, point_begin, dist_step, O, tb, bucket_begin, entry_point, entry_cs);
  return DF_OK;
}

extern "C" size_t df_pose_ppf_scratch_bytes(int B, int WH, int WW, int step, int ref_step) {
  return ppf_sizes_ok(B, WH, WW, step, ref_step) ? ppf_scratch(B, WH, WW, step, ref_step).total : 0;
}

extern "C" int df_pose_ppf(const double *model_points, const double *model_normals, int NM, const int *point_begin, const double *dist_step,
                           const double *cluster_dist, int O, const int *bucket_begin, const int *entry_point, const float *entry_cs,
                           size_t n_entries, int ND, int NANG, int NA, const double *ang_cos, const double *alpha_cos, const double *alpha_cs,
                           const double *proj, const unsigned short *depth, int F, int IH, int IW, const double *rays,
                           const unsigned short *mask, int NMK, const int *items, double cloud_div, int B, int WH, int WW, int step, int reach,
                           int gate, int ref_step, int K, double cluster_trace, double *pose_out, int *votes_out, double *stats,
                           double *hyp_out, void *scratch, size_t scratch_bytes, df_stream_t stream) {
  const char *name = "pose_ppf";
  if (!model_points || !model_normals || !point_begin || !dist_step || !cluster_dist || !bucket_begin || !entry_point || !entry_cs || !ang_cos ||
      !alpha_cos || !alpha_cs || !proj || !depth || !rays || !items || !pose_out || !votes_out || !stats || !scratch)
    return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (mask && NMK < 1) return set_error(DF_ERR_ARG, "%s: a mask needs NM >= 1 frames, got %d", name, NMK);
  if (int e = check_model(name, NM, point_begin, dist_step, O, ND, NANG, NA, ang_cos)) return e;
  if (!descending_cosines(alpha_cos, NA / 2 - 1)) return set_error(DF_ERR_ARG, "%s: alpha_cos must descend strictly inside (-1, 1)", name);
  for (int i = 0; i < 2 * NA; ++i)
    if (!(alpha_cs[i] >= -1.0 && alpha_cs[i] <= 1.0)) return set_error(DF_ERR_ARG, "%s: alpha_cs holds cosines and sines", name);
  for (int o = 0; o < O; ++o)
    if (!(cluster_dist[o] >= 0.0 && cluster_dist[o] - cluster_dist[o] == 0.0))
      return set_error(DF_ERR_ARG, "%s: cluster_dist[%d] must be finite and >= 0", name, o);
  if (!(cluster_trace >= -1.0 && cluster_trace <= 3.0)) return set_error(DF_ERR_ARG, "%s: cluster_trace outside -1..3", name);
  if ((size_t)O * (key_count(ND, NANG) + 1) > (size_t)INT_MAX || n_entries > (size_t)INT_MAX)
    return set_error(DF_ERR_ARG, "%s: the table does not fit 32-bit offsets", name);
  if (!sizes_ok(F, IH, IW)) return set_error(DF_ERR_ARG, "%s: bad sizes", name);
  if (!ppf_sizes_ok(B, WH, WW, step, ref_step))
    return set_error(DF_ERR_ARG, "%s: need B in 1..65535, WH x WW in 1..2^30, step and ref_step in 1..%d, at most %d grid nodes and %d references "
                     "(B %d, window %d x %d, step %d, ref_step %d)", name, ppf::MAX_STEP, ppf::MAX_GRID, ppf::MAX_REFS, B, WH, WW, step, ref_step);
  if (reach < 1 || reach > ppf::MAX_REACH) return set_error(DF_ERR_ARG, "%s: reach %d outside 1..%d", name, reach, ppf::MAX_REACH);
  if (gate < 0 || gate > ppf::MAX_GATE) return set_error(DF_ERR_ARG, "%s: gate %d outside 0..%d", name, gate, ppf::MAX_GATE);
  if (K < 1 || K > ppf::MAX_K) return set_error(DF_ERR_ARG, "%s: K = %d outside 1..%d", name, K, ppf::MAX_K);
  if (!(cloud_div > 0.0 && cloud_div - cloud_div == 0.0)) return set_error(DF_ERR_ARG, "%s: cloud_div must be finite and > 0", name);
  const void *aligned8[] = {model_points, model_normals, rays, pose_out, stats, hyp_out, entry_cs};
  for (const void *p : aligned8)
    if (reinterpret_cast<uintptr_t>(p) % 8)
      return set_error(DF_ERR_ARG, "%s: model_points, model_normals, rays, entry_cs, pose_out, stats and hyp_out must be 8-byte aligned", name);
  if (reinterpret_cast<uintptr_t>(bucket_begin) % 4 || reinterpret_cast<uintptr_t>(entry_point) % 4 || reinterpret_cast<uintptr_t>(items) % 4 ||
      reinterpret_cast<uintptr_t>(votes_out) % 4 || reinterpret_cast<uintptr_t>(depth) % 2 || reinterpret_cast<uintptr_t>(mask) % 2)
    return set_error(DF_ERR_ARG, "%s: a pointer is not aligned to its element", name);
  const PpfScratch lay = ppf_scratch(B, WH, WW, step, ref_step);
  if (int e = check_scratch_and_proj(name, scratch, scratch_bytes, lay.total, proj)) return e;
  Grid gd;
  gd.GH = ppf::grid_side(WH, step); gd.GW = ppf::grid_side(WW, step); gd.step = step; gd.reach = reach; gd.gate = gate;
  gd.ref_step = ref_step; gd.RW = ppf::grid_side(gd.GW, ref_step); gd.NR = ppf::grid_side(gd.GH, ref_step) * gd.RW;
  const int G = gd.GH * gd.GW, NR = gd.NR;
  const size_t npix = (size_t)IH * IW, nkeys = (size_t)O * (key_count(ND, NANG) + 1);
  const struct { const void *p; size_t n; } outs[] = {{pose_out, (size_t)B * K * 7 * 8}, {votes_out, (size_t)B * K * 2 * 4},
                                                      {stats, (size_t)B * ppf::NSTAT * 8}, {hyp_out, (size_t)B * NR * ppf::HYP_DOUBLES * 8}},
                                             ins[] = {{model_points, (size_t)NM * 24}, {model_normals, (size_t)NM * 24}, {bucket_begin, nkeys * 4},
                                                      {entry_point, n_entries * 4}, {entry_cs, n_entries * 8}, {depth, (size_t)F * npix * 2},
                                                      {mask, (size_t)(mask ? NMK : 0) * npix * 2}, {rays, npix * 24},
                                                      {items, (size_t)B * pv::ITEM_INTS * 4}, {scratch, lay.total}};
  for (int a = 0; a < 4; ++a) {
    for (const auto &in : ins)
      if (ranges_overlap(outs[a].p, outs[a].n, in.p, in.n))
        return set_error(DF_ERR_ARG, "%s: an output overlaps an input or the scratch", name);
    for (int c = a + 1; c < 4; ++c)
      if (ranges_overlap(outs[a].p, outs[a].n, outs[c].p, outs[c].n)) return set_error(DF_ERR_ARG, "%s: two outputs overlap", name);
  }
  Model mod;
  int most = 0;
  for (int o = 0; o <= ppf::MAX_OBJECTS; ++o) mod.begin[o] = o <= O ? point_begin[o] : NM;
  for (int o = 0; o < ppf::MAX_OBJECTS; ++o) {
    mod.dist_step[o] = o < O ? dist_step[o] : 1.0;
    mod.cluster_dist[o] = o < O ? cluster_dist[o] : 0.0;
    if (o < O) most = std::max(most, point_begin[o + 1] - point_begin[o]);
  }
  ppf::Tables tb = {};
  tb.ND = ND; tb.NANG = NANG; tb.NA = NA;
  for (int i = 0; i < NANG - 1; ++i) tb.ang_cos[i] = ang_cos[i];
  for (int i = 0; i < NA / 2 - 1; ++i) tb.alpha_cos[i] = alpha_cos[i];
  for (int i = 0; i < NA; ++i) { tb.alpha_cs[i][0] = alpha_cs[2 * i]; tb.alpha_cs[i][1] = alpha_cs[2 * i + 1]; }
  // the limits are set once per kernel, to the largest accumulator and the most references either takes
  if (int e = raise_lds_limit(reinterpret_cast<const void *>(&ppf_vote_kernel), ppf::MAX_ACC_BYTES)) return e;
  if (int e = raise_lds_limit(reinterpret_cast<const void *>(&ppf_cluster_kernel), ppf::MAX_REFS * CLUSTER_SLOT_BYTES)) return e;
  hipStream_t st = to_stream(stream);
  if (hipMemsetAsync(pose_out, 0, outs[0].n, st) != hipSuccess || hipMemsetAsync(votes_out, 0, outs[1].n, st) != hipSuccess ||
      hipMemsetAsync(stats, 0, outs[2].n, st) != hipSuccess || (hyp_out && hipMemsetAsync(hyp_out, 0, outs[3].n, st) != hipSuccess))
    return check_launch(name);
  double *scene = static_cast<double *>(scratch), *rows = reinterpret_cast<double *>(static_cast<char *>(scratch) + lay.scene);
  unsigned long long *visited = reinterpret_cast<unsigned long long *>(static_cast<char *>(scratch) + lay.scene + lay.rows);
  if (hipMemsetAsync(visited, 0, lay.visited, st) != hipSuccess) return check_launch(name);
  const Src src = {depth, mask, rays, F, NMK, IH, IW};
  hipLaunchKernelGGL(ppf_scene_kernel, dim3(cdiv(G, RB), B), dim3(RB), 0, st, src, items, O, proj[10], proj[11], cloud_div, gd, scene);
  hipLaunchKernelGGL(ppf_vote_kernel, dim3(NR, B), dim3(VOTE_LANES), (size_t)most * NA * sizeof(unsigned), st, scene, items, mod, tb, F, O,
                     mask ? 1 : 0, NMK, model_points, model_normals, bucket_begin, entry_point, reinterpret_cast<const float2 *>(entry_cs),
                     (int)n_entries, gd, rows, hyp_out, visited);
  hipLaunchKernelGGL(ppf_cluster_kernel, dim3(B), dim3(CLUSTER_LANES), (size_t)NR * CLUSTER_SLOT_BYTES, st, rows, scene, items, mod, F, O,
                     mask ? 1 : 0, NMK, G, NR, K, cluster_trace, pose_out, votes_out, stats);
  return check_launch(name);
}
