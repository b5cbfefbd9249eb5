// fp32 GEMM on the bf16 matrix cores (product and development library): the inference engine's routed plain-GEMM launches.
//
// Every fp32 operand is cut into three bf16 terms, a = hi + mid + lo (round-to-nearest at each cut: |mid| <= 2^-9 |a|, |lo| <= 2^-18 |a|),
// and a product a*b is accumulated in fp32 from the six term pairs whose magnitude is above 2^-27 |a b|:
//   lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi       (v_mfma_f32_32x32x16_bf16, 16x the fp32 MFMA rate: 16 / 6 = 2.7x at equal efficiency).
// The result is inside fp32 rounding of the exact product, not bit-identical to the fp32-MFMA kernel's summation order.  Per output element
// the order depends only on K: k16 groups in ascending order, the six pairs in the fixed order above -- the same in all three tile forms,
// whatever M, the tile or the form picked: the forms are bit-identical (tests/test_split_gemm_forms_gpu.py).
// The weights are cut once per parameter load by their owner (the engine: Net planes, cut_weight_planes); the activations are cut while the
// workgroup stages its tile (global fp32 -> registers -> three bf16 planes in LDS): no extra pass over HBM.
// Covered: 1x1 / per-point / Winograd-domain launches (plain GEMMs: stride 1, no padding) with Cout % 128 == 0 and K % 32 == 0, bias (per
// channel or per row group), residual, ReLU / PReLU, fused column sums, blockIdx.z batches.  Which launches run here is split_route(N, K,
// epilogue kind) of a launch whose weights come with planes (ConvParams::wpl); everything else stays on the fp32 kernels.
// What the tests pin (tests/test_split_gemm_exact_gpu.py).  On operands s (H + Mi 2^-9 + L 2^-18) with small integers H, Mi, L and at most six
// nonzero products per output, every partial sum is a multiple of 2^-18 below 2^6, so the arithmetic has one fp32 result whatever the order
// the matrix core adds in, and each form must EQUAL the sum of the six pairs plus the epilogue: at every k32 step count that takes another exit
// of a k loop (odd counts: the 256 x 128 form's tail, the clamped prefetches), M below one tile, no bias, channel offsets, the 256 x 256 form's
// fall-back to 256 x 128 on rows that are not 16-byte aligned.  General-valued tolerances cannot pin the pair set: the error of a dropped
// 2^-18 pair grows like sqrt(K) while sum|a||b| grows like K, and max|y - ref| / max|ref| without lo*hi / hi*lo / mid*mid is 1.55e-6 / 1.44e-6 /
// 1.73e-6 at M, N, K = 1000, 1024, 512, 1.66e-6 / 2.06e-6 / 2.08e-6 at 1337, 2304, 1024 and 1.86e-6 / 1.84e-6 / 2.11e-6 at 255, 640, 384 (all six:
// 5.1e-8, 3.7e-8, 4.0e-8; numpy emulation of the cut, pairs summed in fp64) -- on the 2e-6 line of the product tests, under it at several shapes.
// Operand domain of the cut: finite values whose magnitude does not round to bf16 infinity.  An infinity, or a magnitude from 2^127 (2 - 2^-8)
// up, cuts into hi = inf, mid = -inf or NaN, and the product is NaN where the fp32 kernel's is an infinity or a finite number.
// Development build only: DF_GEMM_SPLIT_OFF=1 keeps every launch on fp32; DF_GEMM_SPLIT_BF16=1 also takes eligible launches without planes
// (their weights are cut per launch into a per-stream scratch); DF_GEMM_SPLIT_WGS=N caps the workgroups of a 256 x 256 launch (0: one per
// tile position, no walk).  Measurements: DESIGN.md section 6, profiles/r04_experiments/README.md.
//
// Layout of this file.  What the three tile forms must agree on is stated once, ahead of the kernels: the order of the six pairs (pair_a /
// pair_b), the cut of eight floats (cut4 / cut8), the tile order and z offsets (split_tile_at; split_walk_next: the 256 x 256 form's walk), the fragment addresses of the two 128-column
// forms (SPLIT_FRAG_OFFSETS), and the epilogue's rules (epi_rules, epi_finish, epi_colsum) under its two store paths.  The kernels keep what was
// tuned per form: the fetch / stage / multiply pipelines and their issue-order pins.  On the host plan_split decides everything about a
// launch (taken or not, form, grid, LDS bytes, kernel arguments) without a HIP call or an environment read; try_split_gemm reads the
// development switches, runs the plan and makes the one dispatch through the form table (FORMS / the kernel pointers beside it).
#include "igemm.h"
#include <atomic>
#include <cstdint>
#ifdef DF_DEV
#include <map>
#include <mutex>
#include <tuple>
#endif

namespace df {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int SBM = 128, SBN = 128, SBK = 32;
constexpr int PLANE_BYTES = 128 * 64;                 // 128 rows x 32 bf16

// (hi, mid, lo) of two floats, each pair packed into one dword (element 0 in the low half)
__device__ __forceinline__ void cut3(float a0, float a1, unsigned &hi, unsigned &mid, unsigned &lo) {
  const bf16x2 h = __builtin_convertvector(f32x2{a0, a1}, bf16x2);                 // v_cvt_pk_bf16_f32 (round to nearest even)
  hi = __builtin_bit_cast(unsigned, h);
  const float r0 = a0 - __builtin_bit_cast(float, hi << 16), r1 = a1 - __builtin_bit_cast(float, hi & 0xFFFF0000u);     // exact
  const bf16x2 m = __builtin_convertvector(f32x2{r0, r1}, bf16x2);
  mid = __builtin_bit_cast(unsigned, m);
  const float s0 = r0 - __builtin_bit_cast(float, mid << 16), s1 = r1 - __builtin_bit_cast(float, mid & 0xFFFF0000u);   // exact
  const bf16x2 l = __builtin_convertvector(f32x2{s0, s1}, bf16x2);
  lo = __builtin_bit_cast(unsigned, l);
}

// half H (k 0..3 or 4..7) of the (hi, mid, lo) 16-byte pieces of eight consecutive k
template <int H>
__device__ __forceinline__ void cut4(const float4 &x, uint4 &h, uint4 &m, uint4 &l) {
  if (H == 0) { cut3(x.x, x.y, h.x, m.x, l.x); cut3(x.z, x.w, h.y, m.y, l.y); }
  else { cut3(x.x, x.y, h.z, m.z, l.z); cut3(x.z, x.w, h.w, m.w, l.w); }
}
__device__ __forceinline__ void cut8(const float4 &x0, const float4 &x1, uint4 &h, uint4 &m, uint4 &l) { cut4<0>(x0, h, m, l); cut4<1>(x1, h, m, l); }

// The six term pairs in the one order every form multiplies them, small terms first (lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi): the plane
// (0 hi, 1 mid, 2 lo) of A and of B of pair q
__host__ __device__ constexpr int pair_a(int q) { constexpr int t[6] = {2, 0, 1, 1, 0, 0}; return t[q]; }
__host__ __device__ constexpr int pair_b(int q) { constexpr int t[6] = {0, 2, 1, 0, 1, 0}; return t[q]; }
__device__ __forceinline__ f32x16 mfma_pair(const bf16x8 (&fa)[3], const bf16x8 (&fb)[3], int q, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[pair_a(q)], fb[pair_b(q)], c, 0, 0, 0);
}
// (the 256 x 256 form reads a group's fragments in the phases of pairs 0..2: each of them must be the first to use its A and its B plane)
constexpr bool pair_brings_new_planes(int q) {
  for (int r = 0; r < q; ++r)
    if (pair_a(r) == pair_a(q) || pair_b(r) == pair_b(q)) return false;
  return true;
}
static_assert(pair_brings_new_planes(0) && pair_brings_new_planes(1) && pair_brings_new_planes(2), "pairs 0..2 must reach all planes of A and of B");

// planes[p * stride + i] = term p of w[i]
__global__ void cut_planes_kernel(const float *__restrict__ w, __bf16 *__restrict__ planes, long elems, long stride) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= elems) return;
  unsigned h, m, l;
  cut3(w[i], 0.f, h, m, l);
  unsigned short *pl = reinterpret_cast<unsigned short *>(planes);
  pl[i] = (unsigned short)h; pl[stride + i] = (unsigned short)m; pl[2 * stride + i] = (unsigned short)l;
}

struct SplitArgs {
  const float *in; const __bf16 *wpl; const float *bias; const float *res; const float *prelu; float *out; float *colsum;
  long M, wplane;                 // rows; elements of one weight plane
  int N, K, in_ld, in_coff, out_ld, out_coff, res_ld, res_coff, act, rows_per_group, rows_valid, bias_group_ld;
  long z_in_coff, z_wgt, z_bias, z_out_coff;
  int tiles_m, tiles_n;         // of the launched kernel's tile
  int tiles_total;              // 256 x 256 form: the tile positions of the whole launch, every z, padding included (igemm.h SplitWalk)
  long cs_rows;                 // rows of the column-sum partial buffer per z (igemm.h colsum_partial_rows)
};

// byte offset of the 16-byte piece `slot` (8 consecutive k) of row `row` inside a plane: 64-byte rows, the slot XOR-ed with bits 2..3 of the
// row so that the 16 rows a ds_read_b128 lane group touches fall on 16 different 16-byte bank slots
__device__ __forceinline__ int piece(int row, int slot) { return row * 64 + ((slot ^ ((row >> 2) & 3)) << 4); }

// A workgroup's tile and its z batch.  XCD-aware order: the 8 XCDs take whole row tiles, the column tiles of a row tile run back to back on
// one XCD (its A rows stay in that L2).  false: a padding position of the grid (no tile)
struct SplitTile { int tm, tn, z; const float *in; const __bf16 *wpl; };
__device__ __forceinline__ bool split_tile_at(const SplitArgs &a, int xcd, int seq, int z, SplitTile &t) {
  t.tm = (seq / a.tiles_n) * 8 + xcd;
  t.tn = seq % a.tiles_n;
  t.z = z;
  t.in = a.in + t.z * a.z_in_coff + a.in_coff;
  t.wpl = a.wpl + t.z * a.z_wgt;
  return t.tm < a.tiles_m;
}
// The two 128-column forms: one workgroup per position, blockIdx.z the z batch
__device__ __forceinline__ bool split_tile(const SplitArgs &a, SplitTile &t) { return split_tile_at(a, blockIdx.x & 7, blockIdx.x >> 3, blockIdx.z, t); }
// The 256 x 256 form: one workgroup walks many tiles.  The launch has a.tiles_total positions (igemm.h SplitWalk): per z batch the order above,
// the z batches one behind the other in each XCD's sequence.  A workgroup keeps its XCD (blockIdx.x & 7) and takes the sequence numbers
// (blockIdx.x >> 3) + i (gridDim.x >> 3), i = 0, 1, ...: a static stride, the loop count known on the host, no counter in memory and no wait
// between workgroups.  Moves seq on to the workgroup's next tile (padding positions are passed over); false: the walk is over
__device__ __forceinline__ bool split_walk_next(const SplitArgs &a, int &seq, SplitTile &t) {
  const int seq_z = ((a.tiles_m + 7) >> 3) * a.tiles_n;
  for (; seq < (a.tiles_total >> 3); seq += (int)(gridDim.x >> 3))
    if (split_tile_at(a, blockIdx.x & 7, seq % seq_z, seq / seq_z, t)) return true;
  return false;
}

// Steps the kernels' pipelines share, as macros over the kernels' own names like the pipeline steps they are part of (a, tid, row0, n0, wg,
// the lane roles wr / wc / fr / fh).  (Tried as an inlined function, SPLIT_FRAG_OFFSETS reordered the second form's main loop.)
// All forms: the three planes of one 16-byte piece, from the weight planes in memory (g: the piece in plane 0), and into LDS planes `stride` apart
#define SPLIT_FETCH3(p0, p1, p2, g, k0)                                          \
  do {                                                                           \
    p0 = *reinterpret_cast<const uint4 *>((g) + (k0));                           \
    p1 = *reinterpret_cast<const uint4 *>((g) + a.wplane + (k0));                \
    p2 = *reinterpret_cast<const uint4 *>((g) + 2 * a.wplane + (k0));            \
  } while (0)
#define SPLIT_STORE3(base, stride, off, p0, p1, p2)                              \
  do {                                                                           \
    *reinterpret_cast<uint4 *>((base) + (off)) = p0;                             \
    *reinterpret_cast<uint4 *>((base) + (stride) + (off)) = p1;                  \
    *reinterpret_cast<uint4 *>((base) + 2 * (stride) + (off)) = p2;              \
  } while (0)
// The two 128-column forms (waves of 64 x 64, k-steps of 32).  Fragment addresses, [k16 step][32-row / 32-column tile] (b0: byte offset of B
// plane 0), and the fragments of k16 step ks, [tile][plane]
#define SPLIT_FRAG_OFFSETS(b0)                                                   \
  int offa[2][2], offb[2][2];                                                    \
  _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                               \
  _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                \
    offa[ks][t] = piece(wr * 64 + t * 32 + fr, ks * 2 + fh);                     \
    offb[ks][t] = (b0) + piece(wc * 64 + t * 32 + fr, ks * 2 + fh);              \
  }
#define SPLIT_READ_FRAGS(base, apl, bpl)                                                                  \
  bf16x8 fa[2][3], fb[2][3];                                                                              \
  _Pragma("unroll") for (int t = 0; t < 2; ++t)                                                           \
  _Pragma("unroll") for (int p = 0; p < 3; ++p) {                                                         \
    fa[t][p] = *reinterpret_cast<const bf16x8 *>((base) + p * (apl) + offa[ks][t]);                       \
    fb[t][p] = *reinterpret_cast<const bf16x8 *>((base) + p * (bpl) + offb[ks][t]);                       \
  }
// Their staging: a thread owns two (row, 8-k) pieces of the activation tile, `half` rows (half the tile) apart: the pieces' LDS offsets, their
// global rows (the last row tile re-reads row M - 1: its results are not stored) and the weight row of the first; the fetch of a register
// set S (x / y) and its cut into the planes at `base`
#define SPLIT_STAGE_ROLES(half)                                                  \
  const int srow0 = tid >> 2, srow1 = srow0 + (half), sslot = tid & 3;           \
  const int soff0 = piece(srow0, sslot), soff1 = piece(srow1, sslot);            \
  long r0 = row0 + srow0, r1 = row0 + srow1;                                     \
  r0 = r0 < a.M ? r0 : a.M - 1;                                                  \
  r1 = r1 < a.M ? r1 : a.M - 1;                                                  \
  const float *ag0 = wg.in + r0 * a.in_ld + sslot * 8, *ag1 = wg.in + r1 * a.in_ld + sslot * 8; \
  const __bf16 *bg0 = wg.wpl + (long)(n0 + srow0) * a.K + sslot * 8
#define SPLIT_FETCH_A(S, k0)                                                     \
  do {                                                                           \
    S##a00 = *reinterpret_cast<const float4 *>(ag0 + (k0));                      \
    S##a01 = *reinterpret_cast<const float4 *>(ag0 + (k0) + 4);                  \
    S##a10 = *reinterpret_cast<const float4 *>(ag1 + (k0));                      \
    S##a11 = *reinterpret_cast<const float4 *>(ag1 + (k0) + 4);                  \
  } while (0)
#define SPLIT_CUT_STORE(x0, x1, base, stride, off)                               \
  do {                                                                           \
    uint4 h, m, l;                                                               \
    cut8(x0, x1, h, m, l);                                                       \
    SPLIT_STORE3(base, stride, off, h, m, l);                                    \
  } while (0)

// The epilogue's rules for one wave's 64 x 64 block, shared by its two store paths.  row0: first row of the workgroup's tile (inside ONE row
// group: host-checked), wrow: the block's row offset in it
struct EpiRules {
  float slope;            // PReLU
  const float *bias;      // the block's bias row (per channel, or its row group's), or null
  int limit;              // tile rows below it are real points: the rows fused column sums cover (igemm.h)
  long cs_row;            // the block's row in the column-sum partial buffer: one per COLSUM_ROWS rows, the fp32 kernel's layout
};
__device__ __forceinline__ EpiRules epi_rules(const SplitArgs &a, int z, long row0, int wrow) {
  EpiRules r;
  r.slope = a.act == ACT_PRELU ? a.prelu[0] : 0.f;
  const float *bias = a.bias ? a.bias + z * a.z_bias : nullptr;
  r.bias = bias && a.bias_group_ld > 0 ? bias + (row0 / a.rows_per_group) * a.bias_group_ld : bias;
  const int grp = a.rows_per_group > 0 ? (int)(row0 / a.rows_per_group) : 0;
  const long left = a.M - row0;
  const int valid = a.rows_per_group > 0 ? a.rows_valid - (int)(row0 - (long)grp * a.rows_per_group) : (1 << 30);
  r.limit = (int)(left < valid ? left : valid);
  r.cs_row = (row0 + wrow) / COLSUM_ROWS;
  return r;
}
// N elements (one, or four of a row), each in the one order: + bias, + residual, activation.  A null term is skipped (the row-contiguous
// path adds the residual in a second call)
template <int N>
__device__ __forceinline__ void epi_finish(float (&v)[N], const float *bias, const float *res, int act, float slope) {
  if (bias)
    for (int k = 0; k < N; ++k) v[k] += *bias;
  if (res)
    for (int k = 0; k < N; ++k) v[k] += res[k];
  if (act == ACT_RELU)
    for (int k = 0; k < N; ++k) v[k] = v[k] > 0.f ? v[k] : 0.f;
  else if (act == ACT_PRELU)
    for (int k = 0; k < N; ++k) v[k] = v[k] > 0.f ? v[k] : v[k] * slope;
}
__device__ __forceinline__ float epi_finish(float x, const float *bias, const float *res, int act, float slope) {
  float v[1] = {x};
  epi_finish(v, bias, res, act, slope);
  return v[0];
}
// a lane pair's column sum over the block's 64 rows -> the partial buffer (every partial row the buffer has is written: the finish kernel sums them all)
__device__ __forceinline__ void epi_colsum(const SplitArgs &a, const EpiRules &r, int z, int n, int fh, float csum) {
  if (a.colsum && r.cs_row < a.cs_rows) {
    csum += __shfl_xor(csum, 32);
    if (fh == 0) a.colsum[((size_t)z * a.cs_rows + (size_t)r.cs_row) * a.N + n] = csum;
  }
}

// epilogue of one wave's 64 x 64 block: lane = output channel (col), registers = 16 pixel rows: row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5).
// nb: the block's first column
__device__ __forceinline__ void split_epilogue(const SplitArgs &a, const f32x16 (&acc)[2][2], int z, long row0, int wrow, int nb, int fr, int fh) {
  const EpiRules ru = epi_rules(a, z, row0, wrow);
  float *out = a.out + z * a.z_out_coff + a.out_coff;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = nb + j * 32 + fr;
    const float b1 = ru.bias ? ru.bias[n] : 0.f;
    float csum = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int tb = wrow + i * 32 + 4 * fh;          // first tile row of this lane's 16
      const long mb = row0 + tb;
      float r[16];
      if (a.res) {          // all 16 residual loads in flight before the first use (rows past M re-read row M - 1)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          long m = mb + (e & 3) + 8 * (e >> 2);
          m = m < a.M ? m : a.M - 1;
          r[e] = a.res[m * a.res_ld + a.res_coff + n];
        }
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int tr = tb + (e & 3) + 8 * (e >> 2);
        const long m = row0 + tr;
        const float v = epi_finish(acc[i][j][e], &b1, a.res ? &r[e] : nullptr, a.act, ru.slope);
        if (a.out && m < a.M) out[m * a.out_ld + n] = v;
        csum += tr < ru.limit ? v : 0.f;
      }
    }
    epi_colsum(a, ru, z, n, fh, csum);
  }
}

// The same epilogue for the 256-column form, stores row-contiguous: the wave passes its 64 x 64 block through its own 16 KB of LDS (`blk`; the
// main loop's stages are free by then, and only this wave touches it: no workgroup barrier) and writes 4 rows x 256 bytes per instruction instead
// of 2 rows x 128; a residual is read the same way, and added (with the activation behind it) on the way out.  Column sums are taken in the
// fragment layout, in split_epilogue's order (launches with column sums have no residual: GEMM_EPI_OTHER is not routed).  Needs 16-byte aligned
// output / residual rows (plan_split checks)
// (ACT: the activation applied on the way into LDS, a constant per copy.  Inside the tile walk's loop the compiler no longer lifts the
// launch-wide choices out of the 64 elements; left to it, every element branches on them)
template <int ACT>
__device__ __forceinline__ void split_block_to_lds(const SplitArgs &a, const f32x16 (&acc)[2][2], const EpiRules &ru, int z, int wrow, int nb, int fr, int fh, float *blk) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = nb + j * 32 + fr;
    const float b1 = ru.bias ? ru.bias[n] : 0.f;
    float csum = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int br = i * 32 + 4 * fh + (e & 3) + 8 * (e >> 2);          // row inside the block
        const float v = epi_finish(acc[i][j][e], &b1, nullptr, ACT, ru.slope);
        blk[br * 64 + j * 32 + fr] = v;
        csum += wrow + br < ru.limit ? v : 0.f;
      }
    epi_colsum(a, ru, z, n, fh, csum);
  }
}
__device__ __forceinline__ void split_epilogue_rows(const SplitArgs &a, const f32x16 (&acc)[2][2], int z, long row0, int wrow, int nb, int lane, float *blk) {
  const int fr = lane & 31, fh = lane >> 5;
  const EpiRules ru = epi_rules(a, z, row0, wrow);
  const int act = a.res ? ACT_NONE : a.act;          // (with a residual the activation comes behind it, on the way out)
  if (act == ACT_RELU) split_block_to_lds<ACT_RELU>(a, acc, ru, z, wrow, nb, fr, fh, blk);
  else if (act == ACT_PRELU) split_block_to_lds<ACT_PRELU>(a, acc, ru, z, wrow, nb, fr, fh, blk);
  else split_block_to_lds<ACT_NONE>(a, acc, ru, z, wrow, nb, fr, fh, blk);
  if (!a.out) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  float *out = a.out + z * a.z_out_coff + a.out_coff;
  const int c4 = (lane & 15) * 4;
#pragma unroll 4
  for (int it = 0; it < 16; ++it) {
    const int br = it * 4 + (lane >> 4);
    const long m = row0 + wrow + br;
    float4 v = *reinterpret_cast<const float4 *>(blk + br * 64 + c4);
    if (m < a.M) {
      if (a.res) {
        const float4 r = *reinterpret_cast<const float4 *>(a.res + m * a.res_ld + a.res_coff + nb + c4);
        epi_finish(reinterpret_cast<float (&)[4]>(v), nullptr, &r.x, a.act, ru.slope);
      }
      *reinterpret_cast<float4 *>(out + m * a.out_ld + nb + c4) = v;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(256, 2) void gemm_split_bf16_kernel(const SplitArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[6 * PLANE_BYTES];       // A planes 0..2, B planes 3..5
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  SplitTile wg;
  if (!split_tile(a, wg)) return;
  const long row0 = (long)wg.tm * SBM;
  const int n0 = wg.tn * SBN;

  // staging roles: pieces tid and tid + 256 of the 512 (row, 8-k) pieces of a 128 x 32 tile, of the activations and of each weight plane
  SPLIT_STAGE_ROLES(64);
  const __bf16 *bg1 = wg.wpl + (long)(n0 + srow1) * a.K + sslot * 8;
  // the activation rows come from HBM: their loads for k-step kt + 2 are in flight while step kt is multiplied and step kt + 1 is cut and
  // written to LDS (two register sets x / y: one step of 48 MFMAs per wave = 0.65 us does not cover a miss to HBM); the weight planes sit
  // in the L2: one step ahead
  float4 xa00, xa01, xa10, xa11, ya00, ya01, ya10, ya11;
  uint4 rb00, rb01, rb02, rb10, rb11, rb12;
#define SPLIT_FETCH_B(k0)                                                        \
  do {                                                                           \
    SPLIT_FETCH3(rb00, rb01, rb02, bg0, k0);                                     \
    SPLIT_FETCH3(rb10, rb11, rb12, bg1, k0);                                     \
  } while (0)
#define SPLIT_STAGE(S)                                                           \
  do {                                                                           \
    SPLIT_CUT_STORE(S##a00, S##a01, lds, PLANE_BYTES, soff0);                    \
    SPLIT_STORE3(lds + 3 * PLANE_BYTES, PLANE_BYTES, soff0, rb00, rb01, rb02);   \
    SPLIT_CUT_STORE(S##a10, S##a11, lds, PLANE_BYTES, soff1);                    \
    SPLIT_STORE3(lds + 3 * PLANE_BYTES, PLANE_BYTES, soff1, rb10, rb11, rb12);   \
  } while (0)

  const int wr = wave >> 1, wc = wave & 1, fr = lane & 31, fh = lane >> 5;
  f32x16 acc[2][2] = {};
  SPLIT_FRAG_OFFSETS(3 * PLANE_BYTES);

#define SPLIT_COMPUTE()                                                                                   \
  _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                                      \
    SPLIT_READ_FRAGS(lds, PLANE_BYTES, PLANE_BYTES);                                                      \
    _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                         \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                         \
    _Pragma("unroll") for (int q = 0; q < 6; ++q) acc[i][j] = mfma_pair(fa[i], fb[j], q, acc[i][j]);      \
  }

  const int nk = a.K / SBK;
  SPLIT_FETCH_A(x, 0);
  SPLIT_FETCH_B(0);
  if (nk > 1) SPLIT_FETCH_A(y, SBK);
  SPLIT_STAGE(x);
  __syncthreads();
  for (int kt = 0; kt < nk; kt += 2) {
    // LDS: step kt; set y: the rows of step kt + 1
    if (kt + 1 < nk) SPLIT_FETCH_B((kt + 1) * SBK);
    if (kt + 2 < nk) SPLIT_FETCH_A(x, (kt + 2) * SBK);
    SPLIT_COMPUTE();
    if (kt + 1 >= nk) break;
    __syncthreads();
    SPLIT_STAGE(y);
    __syncthreads();
    // LDS: step kt + 1; set x: the rows of step kt + 2
    if (kt + 2 < nk) SPLIT_FETCH_B((kt + 2) * SBK);
    if (kt + 3 < nk) SPLIT_FETCH_A(y, (kt + 3) * SBK);
    SPLIT_COMPUTE();
    if (kt + 2 >= nk) break;
    __syncthreads();
    SPLIT_STAGE(x);
    __syncthreads();
  }

  split_epilogue(a, acc, wg.z, row0, wr * 64, n0 + wc * 64, fr, fh);
}

// Second form: 256 x 128 x 32 tile, 8 waves (4 x 2) of 64 x 64, TWO LDS stages (144 KB: one workgroup per CU, two waves per SIMD) and ONE barrier
// per k-step: while a wave multiplies step kt out of stage kt % 2 it cuts step kt + 1 (loaded one iteration earlier) into the other stage, and
// the loads of step kt + 2 are in flight.
constexpr int V2_APL = 256 * 64, V2_BPL = 128 * 64, V2_STAGE = 3 * V2_APL + 3 * V2_BPL;

__global__ __launch_bounds__(512, 1) void gemm_split_bf16_v2_kernel(const SplitArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds2[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  SplitTile wg;
  if (!split_tile(a, wg)) return;
  const long row0 = (long)wg.tm * 256;
  const int n0 = wg.tn * SBN;

  // staging roles: A pieces tid and tid + 512 of the 1024 (row, 8-k) pieces of the 256 x 32 tile; B piece tid of each plane's 512
  SPLIT_STAGE_ROLES(128);
  float4 xa00, xa01, xa10, xa11, ya00, ya01, ya10, ya11;
  uint4 xb0, xb1, xb2, yb0, yb1, yb2;
#define V2_FETCH(S, k0)                                                          \
  do {                                                                           \
    SPLIT_FETCH_A(S, k0);                                                        \
    SPLIT_FETCH3(S##b0, S##b1, S##b2, bg0, k0);                                  \
  } while (0)
#define V2_STAGE_TO(S, base)                                                     \
  do {                                                                           \
    SPLIT_CUT_STORE(S##a00, S##a01, base, V2_APL, soff0);                        \
    SPLIT_CUT_STORE(S##a10, S##a11, base, V2_APL, soff1);                        \
    SPLIT_STORE3((base) + 3 * V2_APL, V2_BPL, soff0, S##b0, S##b1, S##b2);       \
  } while (0)

  const int wr = wave >> 1, wc = wave & 1, fr = lane & 31, fh = lane >> 5;
  f32x16 acc[2][2] = {};
  SPLIT_FRAG_OFFSETS(3 * V2_APL);
  // pair-major order (every tile's lo*hi, then every tile's hi*lo, ...): per accumulator the order is still small terms first, and the lo / mid
  // fragments die early, which leaves registers for the next k16 step's fragments
#define V2_COMPUTE(base)                                                                                  \
  _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                                      \
    SPLIT_READ_FRAGS(base, V2_APL, V2_BPL);                                                               \
    _Pragma("unroll") for (int q = 0; q < 6; ++q)                                                         \
    _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                         \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) acc[i][j] = mfma_pair(fa[i], fb[j], q, acc[i][j]);      \
  }
  // one k-step, branch-free: loads of step kt + 2 (clamped to the last step: harmless re-read), cut of step kt + 1 into the other stage, products
  // of step kt -- ONE basic block, with the issue order pinned so that the cut's vector instructions and the LDS traffic sit in the gaps of the
  // MFMA stream of the SAME wave (a wave issuing MFMAs back to back blocks the other wave of its SIMD: DESIGN 6a)
#define V2_BODY(FS, SS, kf, cur, nxt)                                            \
  do {                                                                           \
    V2_FETCH(FS, (kf));                                                          \
    V2_STAGE_TO(SS, nxt);                                                        \
    V2_COMPUTE(cur);                                                             \
    __builtin_amdgcn_sched_group_barrier(0x020, 7, 0);                           \
    __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);                          \
    _Pragma("unroll") for (int g = 0; g < 48; ++g) {                             \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                         \
      __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);                         \
      if (g >= 8 && g < 32 && (g & 1) == 0) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); \
      if (g % 5 == 4) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);         \
    }                                                                            \
    __syncthreads();                                                             \
  } while (0)

  unsigned char *const st0 = lds2, *const st1 = lds2 + V2_STAGE;
  const int nk = a.K / SBK;
  const int klast = a.K - SBK;
  V2_FETCH(x, 0);
  V2_FETCH(y, SBK < klast ? SBK : klast);
  V2_STAGE_TO(x, st0);
  __syncthreads();
  int kt = 0;
  for (; kt + 1 < nk; kt += 2) {
    // stage 0: step kt; set y: step kt + 1
    const int k2 = (kt + 2) * SBK, k3 = (kt + 3) * SBK;
    V2_BODY(x, y, k2 < klast ? k2 : klast, st0, st1);
    // stage 1: step kt + 1; set x: step kt + 2
    V2_BODY(y, x, k3 < klast ? k3 : klast, st1, st0);
  }
  if (nk & 1) { V2_COMPUTE(st0); }       // the last step of an odd count (cut into stage 0 by the loop's second half)
  split_epilogue(a, acc, wg.z, row0, wr * 64, n0 + wc * 64, fr, fh);
}

// Third form: 256 x 256 x 16 tile, 8 waves (2 x 4) of 128 x 64, two LDS stages of one k16 group each (96 KB: one workgroup per CU) and one barrier
// per group.  Per MFMA it cuts and loads half the activations of the 256 x 128 form (a row tile is staged N / 256 times instead of N / 128) and
// reads 18 fragments per 48 MFMAs instead of 24.  Per output element nothing moves: k16 groups in ascending k, the six pairs in the same order,
// the same epilogue on 64 x 64 blocks (a wave owns two, one column-sum partial row each).
constexpr int V3_PL = 256 * 32, V3_STAGE = 6 * V3_PL;          // a plane: 256 rows x 16 bf16; a stage: A planes 0..2, B planes 3..5
constexpr int V3_LDS = 8 * 64 * 64 * 4;                          // the epilogue's eight 64 x 64 fp32 blocks: more than the two stages

// byte offset of the 16-byte half `half` (8 consecutive k) of row `row` inside a k16 plane: 32-byte rows, the half XOR-ed with bit 3 of the row:
// the 16 rows of a ds_read_b128 lane group ({0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} of a fragment's 32) then cover the 16 slots of the
// 256-byte bank row once each, and the 8 x 8-lane groups of the staging ds_write_b128 (row = tid / 2) write 128 contiguous bytes
__device__ __forceinline__ int piece16(int row, int half) { return row * 32 + ((half ^ ((row >> 3) & 1)) << 4); }

// DF_STRACE(i, s): time stamp i of every wave, filed under the tile with sequence number s, for tools/dev/split_gemm_trace.hip (which compiles
// this file with the hooks defined); nothing otherwise
#ifndef DF_STRACE
#define DF_STRACE_ENTRY()
#define DF_STRACE(i, s) ((void)(s))
#endif

// A workgroup walks its tiles (split_walk_next) with one hand-over between two of them: the next tile's first fetches (weight planes of group 0,
// activations of groups 0 and 1) are issued into the fetch registers, dead by then, BEFORE the finished tile's epilogue, whose output stores are
// issued and not waited for; one workgroup barrier separates the epilogue's last LDS read from the next tile's stage-0 write (a wave's 16 KB
// epilogue block lies across both stages).
__global__ __launch_bounds__(512, 1) void gemm_split_bf16_v3_kernel(const SplitArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds3[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  DF_STRACE_ENTRY();
  SplitTile wg;
  int seq = blockIdx.x >> 3;
  if (!split_walk_next(a, seq, wg)) return;

  // staging roles: piece tid of the 512 (row, 8-k) pieces of the activation tile and of each weight plane's tile
  const int srow = tid >> 1, shalf = tid & 1;
  const int soff = piece16(srow, shalf);
  const float *ag;
  const __bf16 *bg;
  // (the last row tile re-reads row M - 1: its results are not stored.  The empty asm keeps the address arithmetic per tile: see the epilogue's)
#define V3_TILE_ROLES()                                                          \
  do {                                                                           \
    int t = tid;                                                                 \
    asm volatile("" : "+v"(t));                                                  \
    long r = (long)wg.tm * 256 + (t >> 1);                                       \
    r = r < a.M ? r : a.M - 1;                                                   \
    ag = wg.in + r * a.in_ld + (t & 1) * 8;                                      \
    bg = wg.wpl + (long)(wg.tn * 256 + (t >> 1)) * a.K + (t & 1) * 8;            \
  } while (0)
  // activations (HBM) two groups ahead in two register sets, weight planes (L2) one group ahead
  float4 xa0, xa1, ya0, ya1;
  uint4 b0, b1, b2;
#define V3_FETCH_A(S, k0)                                                        \
  do {                                                                           \
    S##a0 = *reinterpret_cast<const float4 *>(ag + (k0));                        \
    S##a1 = *reinterpret_cast<const float4 *>(ag + (k0) + 4);                    \
  } while (0)
#define V3_FETCH_B(k0) SPLIT_FETCH3(b0, b1, b2, bg, k0)
  // (the empty asm pins a cut behind the phase boundary in front of it: without it instruction selection may start the cut right behind the
  // set's loads, and the wave then waits out the whole HBM round trip instead of covering it with a group of MFMAs)
#define V3_PIN(v) asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w))
#define V3_CUT0(S) do { V3_PIN(S##a0); cut4<0>(S##a0, ch, cm, cl); } while (0)
#define V3_CUT1(S) do { V3_PIN(S##a1); cut4<1>(S##a1, ch, cm, cl); } while (0)
#define V3_WRITE_A(base) SPLIT_STORE3(base, V3_PL, soff, ch, cm, cl)
#define V3_WRITE_B(base) SPLIT_STORE3((base) + 3 * V3_PL, V3_PL, soff, b0, b1, b2)

  const int wr = wave >> 2, wc = wave & 3, fr = lane & 31, fh = lane >> 5;
  // (a tile's 32-row offset leaves bit 3 of the row alone: the four A and two B fragments of a plane are one address plus constants)
  const int offa = piece16(wr * 128 + fr, fh), offb = 3 * V3_PL + piece16(wc * 64 + fr, fh);
  // pair-major as in the second form.  V3_READ(q), q = 0..2: the six fragments pair q is the first to use (pair_brings_new_planes)
#define V3_READ(base, q)                                                                                  \
  do {                                                                                                    \
    _Pragma("unroll") for (int t = 0; t < 4; ++t)                                                         \
      fa[t][pair_a(q)] = *reinterpret_cast<const bf16x8 *>((base) + pair_a(q) * V3_PL + offa + t * 1024); \
    _Pragma("unroll") for (int t = 0; t < 2; ++t)                                                         \
      fb[t][pair_b(q)] = *reinterpret_cast<const bf16x8 *>((base) + pair_b(q) * V3_PL + offb + t * 1024); \
  } while (0)
#define V3_MFMA(q)                                                                                        \
  do {                                                                                                    \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                         \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) acc[i >> 1][i & 1][j] = mfma_pair(fa[i], fb[j], q, acc[i >> 1][i & 1][j]); \
  } while (0)
  // n x (one MFMA, then `cnt` instructions of class `mask`): the filler sits in the MFMA gaps of the SAME wave (a wave issuing MFMAs back to back
  // blocks the other wave of its SIMD: DESIGN 6a); a full scheduling barrier closes each phase so that nothing drifts across it
#define V3_WEAVE(n, mask, cnt)                                                   \
  do {                                                                           \
    _Pragma("unroll") for (int g = 0; g < (n); ++g) {                            \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                         \
      __builtin_amdgcn_sched_group_barrier(mask, cnt, 0);                        \
    }                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                           \
  } while (0)
  // one k16 group in six phases of 8 MFMAs (one pair each): weight loads of group s + 1 and activation loads of group s + 2 (clamped to the last
  // group: harmless re-read); pairs 0 and 1 run under the fragment reads of the planes the later pairs need, pairs 2 and 3 under the cut of group
  // s + 1, pairs 4 and 5 under its LDS stores into the other stage (the weight planes last: their loads are the youngest)
#define V3_BODY(FS, SS, ka, kb, cur, nxt)                                        \
  do {                                                                           \
    bf16x8 fa[4][3], fb[2][3];                                                   \
    uint4 ch, cm, cl;                                                            \
    V3_FETCH_B(kb);                                                              \
    V3_FETCH_A(FS, ka);                                                          \
    V3_READ(cur, 0);                                                             \
    __builtin_amdgcn_sched_barrier(0);                                           \
    V3_READ(cur, 1);                                                             \
    V3_MFMA(0);                                                                  \
    V3_WEAVE(6, 0x100, 1);                                                       \
    V3_READ(cur, 2);                                                             \
    V3_MFMA(1);                                                                  \
    V3_WEAVE(6, 0x100, 1);                                                       \
    V3_CUT0(SS);                                                                 \
    V3_MFMA(2);                                                                  \
    V3_WEAVE(8, 0x002, 3);                                                       \
    V3_CUT1(SS);                                                                 \
    V3_MFMA(3);                                                                  \
    V3_WEAVE(8, 0x002, 3);                                                       \
    V3_WRITE_A(nxt);                                                             \
    V3_MFMA(4);                                                                  \
    V3_WEAVE(3, 0x200, 1);                                                       \
    V3_WRITE_B(nxt);                                                             \
    V3_MFMA(5);                                                                  \
    V3_WEAVE(3, 0x200, 1);                                                       \
    __syncthreads();                                                             \
  } while (0)

  unsigned char *const st0 = lds3, *const st1 = lds3 + V3_STAGE;
  const int nk = a.K / 16;          // even: K % 32 == 0
  const int klast = a.K - 16;
  // a tile's first fetches: weight planes of group 0, activations of groups 0 and 1
#define V3_FIRST_FETCHES()                                                       \
  do {                                                                           \
    V3_TILE_ROLES();                                                             \
    V3_FETCH_B(0);                                                               \
    V3_FETCH_A(x, 0);                                                            \
    V3_FETCH_A(y, 16);                                                           \
  } while (0)
  V3_FIRST_FETCHES();
  DF_STRACE(0, seq);
  DF_STRACE(1, seq);
  for (;;) {
    const long row0 = (long)wg.tm * 256;
    const int n0 = wg.tn * 256, z = wg.z, seq0 = seq;
    f32x16 acc[2][2][2] = {};          // [64-row block of the wave][32-row tile][32-column tile]
    {
      uint4 ch, cm, cl;
      V3_CUT0(x);
      V3_CUT1(x);
      V3_WRITE_A(st0);
      V3_WRITE_B(st0);
    }
    __syncthreads();
    DF_STRACE(2, seq0);
    for (int s = 0; s < nk; s += 2) {
      // stage 0: group s; set y: group s + 1
      const int k1 = (s + 1) * 16, k2 = (s + 2) * 16, k3 = (s + 3) * 16;
      V3_BODY(x, y, k2 < klast ? k2 : klast, k1, st0, st1);
      // stage 1: group s + 1; set x: group s + 2
      V3_BODY(y, x, k3 < klast ? k3 : klast, k2 < klast ? k2 : klast, st1, st0);
    }
    // (every wave is past the loop's last barrier: the stages are free, the fetch registers dead.)  The next tile's first fetches go out ahead
    // of this tile's epilogue and stay in flight under it
    DF_STRACE(3, seq0);
    seq += (int)(gridDim.x >> 3);
    const bool more = split_walk_next(a, seq, wg);
    if (more) {
      V3_FIRST_FETCHES();
      DF_STRACE(1, seq);
    }
    __builtin_amdgcn_sched_barrier(0);
    // (the empty asm keeps the epilogue's lane arithmetic -- 64 row numbers, as many LDS addresses -- inside the walk's loop: lifted out of it as
    // loop invariants they live across the main loop, which has no register to spare, and go to scratch)
    int et = tid;
    asm volatile("" : "+v"(et));
    const int elane = et & 63, ewr = et >> 8, ewc = (et >> 6) & 3;
    float *const blk = reinterpret_cast<float *>(lds3) + (et >> 6) * (64 * 64);          // the wave's epilogue block
    split_epilogue_rows(a, acc[0], z, row0, ewr * 128, n0 + ewc * 64, elane, blk);
    DF_STRACE(4, seq0);
    split_epilogue_rows(a, acc[1], z, row0, ewr * 128 + 64, n0 + ewc * 64, elane, blk);
    DF_STRACE(5, seq0);
    if (!more) {
      DF_STRACE(6, seq0);
      break;
    }
    __syncthreads();          // the epilogue's last LDS read of every wave, before the next tile's stage-0 write
  }
}

#ifdef DF_DEV
// development switch DF_GEMM_SPLIT_BF16: planes of weights that come without them, cut per launch into a per-(device, stream) scratch
std::mutex g_mu;
std::map<std::tuple<int, hipStream_t>, std::pair<__bf16 *, long>> g_scratch;

const __bf16 *scratch_planes(const float *w, long elems, hipStream_t st) {
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> g(g_mu);
  auto &sc = g_scratch[std::make_tuple(dev, st)];
  if (sc.second < elems) {
    if (sc.first) (void)hipFree(sc.first);          // (synchronises the device: launches reading the old planes have finished)
    sc = {nullptr, 0};
    if (hipMalloc(reinterpret_cast<void **>(&sc.first), (size_t)elems * 3 * sizeof(__bf16)) != hipSuccess) return nullptr;
    sc.second = elems;
  }
  cut_weight_planes(w, sc.first, elems, elems, st);
  return sc.first;
}
#endif

// The tile forms: what a launch of each needs.  256x128 and 256x256 take more dynamic LDS than the 64 KiB a kernel gets by default
enum SplitForm { FORM_128x128 = 0, FORM_256x128 = 1, FORM_256x256 = 2 };
struct FormDesc { const char *name; void (*kernel)(SplitArgs); int bm, bn, threads, lds; bool raise; };
const FormDesc FORMS[3] = {{"128x128", gemm_split_bf16_kernel, SBM, SBN, 256, 0, false},
                           {"256x128", gemm_split_bf16_v2_kernel, 256, SBN, 512, 2 * V2_STAGE, true},
                           {"256x256", gemm_split_bf16_v3_kernel, 256, 256, 512, V3_LDS, true}};

// Everything one launch needs, decided on the host (no HIP call, no environment: the switches and the device's compute units come in)
struct SplitPlan {
  bool examined = false;          // the launch reached the cover check (DF_GEMM_SPLIT_VERBOSE reports those)
  int form = FORM_128x128;
  int threads = 0, lds = 0;       // workgroup size; dynamic LDS bytes
  dim3 grid;
  SplitArgs a{};                  // tiles_m / tiles_n: of the form's tile.  (A development-build launch without planes: a.wpl / a.wplane are null / 0)
};

// 0: not taken (the fp32 kernels' launch), 1: taken, pl filled, DF_ERR_ARG: a routed launch outside the kernels' cover.  variant: the highest
// form allowed (DF_GEMM_SPLIT_V; 3 = all), all: DF_GEMM_SPLIT_BF16 (DF_GEMM_SPLIT_OFF never gets here), workgroups: the most a 256 x 256 launch
// may have (DF_GEMM_SPLIT_WGS; 0: one per tile position; < 0: one per compute unit)
int plan_split(const ConvParams &p, int compute_units, int variant, bool all, int workgroups, SplitPlan &pl) {
  pl = SplitPlan{};
  if (p.splitk_ws || (!p.wpl && !all)) return 0;
  pl.examined = true;
  const long M = (long)p.B * p.OH * p.OW;
  const int K = p.Cin;
  SplitArgs &a = pl.a;
  a.in = p.in; a.wpl = reinterpret_cast<const __bf16 *>(p.wpl); a.bias = p.bias; a.res = p.res; a.prelu = p.prelu; a.out = p.out; a.colsum = p.colsum;
  a.M = M; a.wplane = p.wpl_stride; a.N = p.Cout; a.K = K; a.in_ld = p.in_ld; a.in_coff = p.in_coff; a.out_ld = p.out_ld; a.out_coff = p.out_coff;
  a.res_ld = p.res_ld; a.res_coff = p.res_coff; a.act = p.act; a.rows_per_group = p.rows_per_group; a.rows_valid = p.rows_valid; a.bias_group_ld = p.bias_group_ld;
  a.z_in_coff = p.z_in_coff; a.z_wgt = p.z_wgt; a.z_bias = p.z_bias; a.z_out_coff = p.z_out_coff;
  a.cs_rows = colsum_partial_rows(M);
  // launch geometry the kernels cover (every engine plain GEMM: a property of the layer, not of M)
  const bool ok = p.KH == 1 && p.KW == 1 && p.stride == 1 && p.pad == 0 && p.up == 1 && p.H == p.OH && p.W == p.OW && (p.out || p.colsum) &&
                  p.Cout % SBN == 0 && K % SBK == 0 && K >= SBK && M >= 1 && gemm_epi_kind(p) != GEMM_EPI_OTHER &&
                  (p.rows_per_group == 0 ? p.bias_group_ld == 0 : p.rows_per_group % SBM == 0) && (p.z_wgt % 8) == 0;
  if (!ok || !(all || split_route(p.Cout, K, gemm_epi_kind(p)))) {
    // planes come only with routed layers: a routed layer the kernels cannot take is a caller error, not a quiet fp32 launch
    if (p.wpl && !all) return set_error(DF_ERR_ARG, "split gemm: routed launch M=%ld N=%d K=%d outside the kernels' cover", M, p.Cout, K);
    return 0;
  }
  // measured per shape: the 256-row forms win from K = 384 up (189 against 172 TFLOP/s on 139 000 x 2 304 x 1 024), the 128-row form below.
  // All forms add the same products in the same order per element: the choice changes no bit
  const bool v2 = variant >= 2 && K >= 384 && (p.rows_per_group == 0 || p.rows_per_group % 256 == 0);
  // the 256-column form where N allows it and its tiles still fill the card (the 1 440-row psp fold has 96 of them: it keeps 128 columns)
  const long tiles3 = ((M + 255) / 256) * (p.Cout / 256) * p.zcount;
  // (its epilogue moves whole 16-byte pieces of output and residual rows)
  const bool rows16 = (!p.out || (reinterpret_cast<uintptr_t>(p.out) % 16 == 0 && p.out_ld % 4 == 0 && p.out_coff % 4 == 0 && p.z_out_coff % 4 == 0)) &&
                      (!p.res || (reinterpret_cast<uintptr_t>(p.res) % 16 == 0 && p.res_ld % 4 == 0 && p.res_coff % 4 == 0));
  // (the walk counts the positions of all z batches, padding included, in an int)
  const bool v3 = v2 && variant >= 3 && p.Cout % 256 == 0 && rows16 && tiles3 >= compute_units && tiles3 < (1L << 27);
  pl.form = v3 ? FORM_256x256 : v2 ? FORM_256x128 : FORM_128x128;
  const FormDesc &f = FORMS[pl.form];
  a.tiles_m = (int)((M + f.bm - 1) / f.bm);
  a.tiles_n = p.Cout / f.bn;
  pl.grid = dim3((unsigned)(((a.tiles_m + 7) / 8) * 8 * a.tiles_n), 1, p.zcount);      // (whole groups of 8 row tiles: split_tile)
  if (v3) {          // one workgroup per compute unit walks the positions of all z batches (split_walk_next)
    const SplitWalk w = split_walk(a.tiles_m, a.tiles_n, p.zcount, workgroups < 0 ? compute_units : workgroups);
    a.tiles_total = w.tiles_total;
    pl.grid = dim3((unsigned)w.grid, 1, 1);
  }
  pl.threads = f.threads;
  pl.lds = f.lds;
  return 1;
}

}  // namespace

int split_route(int N, int K, int epi) {
  // measured in the bench step (profiles/r04_experiments/README.md): from K = 384 up the 256-row form beats the fp32
  // kernel on every engine shape (139 000 x 2 304 x 1 024: 189 against 142 TFLOP/s, 286 720 x 1 024 x 512: 175 - 185 against 136 - 141,
  // Winograd-domain 512 x 512: 158 against 136, 286 720 x 640 x 384: 163 against 134); at K = 192 / 256 it loses or ties (99 - 121 against
  // 118 - 128), and K <= 64 (the point layers csrc/pointfeat.hip chains) stays fp32 so that the chained and the per-layer launches agree
  if (N <= 0 || N % SBN != 0 || K % SBK != 0 || K < 384) return 0;
  return epi == GEMM_EPI_PLAIN || epi == GEMM_EPI_RESIDUAL || epi == GEMM_EPI_GROUPS;
}

SplitWalk split_walk(int tiles_m, int tiles_n, int zcount, int workgroups) {
  SplitWalk w;
  w.tiles_total = ((tiles_m + 7) / 8) * 8 * tiles_n * zcount;
  w.grid = workgroups <= 0 || workgroups >= w.tiles_total ? w.tiles_total : workgroups < 8 ? 8 : workgroups / 8 * 8;
  return w;
}

int split_walk_trips(const SplitWalk &w, int b) {
  const int seqs = w.tiles_total / 8, step = w.grid / 8, first = b / 8;
  return first < seqs ? (seqs - first + step - 1) / step : 0;
}

int gemm_epi_kind(const ConvParams &p) {
  const bool groups = p.rows_per_group > 0 || p.bias_group_ld > 0 || p.colsum;
  if (p.res) return groups ? GEMM_EPI_OTHER : GEMM_EPI_RESIDUAL;
  return groups ? GEMM_EPI_GROUPS : GEMM_EPI_PLAIN;
}

void cut_weight_planes(const float *w, void *planes, long elems, long stride, hipStream_t st) {
  hipLaunchKernelGGL(cut_planes_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, w, reinterpret_cast<__bf16 *>(planes), elems, stride);
}

// compute units of the current device (one query per device)
static int compute_units() {
  static std::atomic<int> cus[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64) return 256;
  int n = cus[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

int try_split_gemm(const ConvParams &p, hipStream_t st, ConvRoute &r) {
  static const bool off = dev_getenv("DF_GEMM_SPLIT_OFF") != nullptr;
  static const bool all = dev_getenv("DF_GEMM_SPLIT_BF16") != nullptr;
  static const bool verbose = dev_getenv("DF_GEMM_SPLIT_VERBOSE") != nullptr;
  static const int variant = dev_getenv("DF_GEMM_SPLIT_V") ? atoi(dev_getenv("DF_GEMM_SPLIT_V")) : 3;
  static const int workgroups = dev_getenv("DF_GEMM_SPLIT_WGS") ? atoi(dev_getenv("DF_GEMM_SPLIT_WGS")) : -1;
  if (off) return 0;
  SplitPlan pl;
  const int rc = plan_split(p, compute_units(), variant, all, workgroups, pl);
  if (verbose && pl.examined) fprintf(stderr, "[df-split] M=%ld N=%d K=%d z%d -> %s\n", pl.a.M, p.Cout, p.Cin, p.zcount, rc == 1 ? "bf16 x 6" : "fp32");
  if (rc != 1) return rc;
#ifdef DF_DEV
  if (!pl.a.wpl) {
    pl.a.wplane = (long)(p.zcount - 1) * p.z_wgt + (long)p.Cout * p.Cin;
    pl.a.wpl = scratch_planes(p.wgt, pl.a.wplane, st);
    if (!pl.a.wpl) return set_error(DF_ERR_LAUNCH, "split gemm: hipMalloc of the weight-plane scratch failed");
  }
#endif
  const FormDesc &f = FORMS[pl.form];
  if (verbose) fprintf(stderr, "[df-split]   form %s\n[df-split]   workgroups %u\n", f.name, pl.grid.x * pl.grid.z);
  if (f.raise) {
    const int e = raise_lds_limit(reinterpret_cast<const void *>(f.kernel), pl.lds);
    if (e != DF_OK) return e;
  }
  hipLaunchKernelGGL(f.kernel, pl.grid, dim3(pl.threads), pl.lds, st, pl.a);
  r = ConvRoute{};
  r.kernel = CONV_BF16;
  r.bm = f.bm;
  r.bn = f.bn;
  return 1;
}

}  // namespace df
