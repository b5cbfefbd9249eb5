// Scoring SegNet on the device: df_seg_score turns channels-last logits and the int64 target df_seg_batch wrote into the label map and
// a per-frame confusion matrix; df_seg_masks turns label maps into the u16 masks the customCAD pose path reads.  The contracts are
// the comments of the two calls in include/dfusion.h (steps S1..S3, M1); the per-pixel rules are seg_score_core.h; tests/seg_score_np.py
// restates them in numpy and the outputs are compared bit for bit.
//
// df_seg_score, on the caller's stream: conf and skipped are set to zero; seg_score_kernel, grid = (parts, F).  The call is read-bound
// (4 ld + 8 bytes in per pixel, 4 out with label_out), so the label pass of segment.hip is its shape: workgroup b of frame f covers
// pixels [b SCORE_PPB, (b + 1) SCORE_PPB) of the frame in tiles of TB pixels; a tile's logits come in as coalesced float4 loads, one
// tile ahead into registers, and go through LDS (rows of (ld / 4) | 1 float4s, an odd stride); lane t then takes pixel t's arg-max
// (seg_argmax.h).  The target comes in one int64 per lane, one tile ahead as well.  The C x C table lives in LDS behind the tile.  A
// rendered scene is mostly cell (0, 0), so a wave first walks the distinct cells present among its 64 pixels with ballots and makes ONE
// LDS add per distinct cell, never one per pixel; at the end the workgroup adds its non-zero cells to conf[f] with integer atomics.
// Integers only: the sums do not depend on the order, two calls give the same bytes.
//
// df_seg_masks: pairs and windows are HOST arrays, checked on the host and handed to the kernel by value, MASK_PAIRS pairs per launch
// (the way the renderers pass their hole records): no upload, no allocation.  A thread owns one pixel of one mask.
#include "common.h"
#include "seg_score_core.h"

namespace df {
namespace {

constexpr int TB = 256;              // threads = pixels per tile
constexpr int SCORE_PPB = 4096;      // pixels per workgroup
constexpr int MAX_LD4 = segscore::MAX_LD / 4;
constexpr int MASK_PAIRS = 128;      // pairs per launch of seg_masks_kernel: 2 KiB of kernel arguments

inline int score_lds_bytes(int ld, int C) { return TB * ((ld / 4) | 1) * (int)sizeof(f32x4) + (C * C + 1) * (int)sizeof(int); }

// MAXN4: the float4s per pixel the registers hold (8: ld <= 32, 16: ld <= 64).  LDS: the tile, the C x C table, the skipped count.
template <int MAXN4>
__global__ __launch_bounds__(TB) void seg_score_kernel(const float *__restrict__ logits, const int64_t *__restrict__ target, int HW, int ld,
                                                       int C, int *__restrict__ label_out, int *__restrict__ conf,
                                                       int *__restrict__ skipped) {
  extern __shared__ f32x4 tile[];
  const int f = blockIdx.y, b = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const int n4 = ld >> 2, s = n4 | 1, cells = C * C;
  int *table = reinterpret_cast<int *>(tile + TB * s);         // [cells], then the skipped count
  const long fbase = (long)f * HW;
  const int p0 = b * SCORE_PPB, p1 = p0 + SCORE_PPB < HW ? p0 + SCORE_PPB : HW;
  const f32x4 *src = reinterpret_cast<const f32x4 *>(logits) + fbase * n4;
  for (int i = t; i <= cells; i += TB) table[i] = 0;           // ordered before the first add by the loop's barriers
  f32x4 reg[MAXN4];
  int64_t treg = 0;
  int nskip = 0;                                               // this wave's, the same in every lane
  {
    const int np = p1 - p0 < TB ? p1 - p0 : TB, tot = np * n4;
#pragma unroll
    for (int k = 0; k < MAXN4; ++k)
      if (k < n4 && t + k * TB < tot) reg[k] = src[(long)p0 * n4 + t + k * TB];
    if (t < np) treg = target[fbase + p0 + t];
  }
  for (int q0 = p0; q0 < p1; q0 += TB) {
    const int np = p1 - q0 < TB ? p1 - q0 : TB, tot = np * n4;
    __syncthreads();                                           // the previous tile's readers are done
#pragma unroll
    for (int k = 0; k < MAXN4; ++k) {
      const int i = t + k * TB;
      if (k < n4 && i < tot) {
        const int px = i / n4;
        tile[px * s + (i - px * n4)] = reg[k];
      }
    }
    const int64_t tg = treg;
    __syncthreads();
    const int q1 = q0 + TB;
    if (q1 < p1) {                                             // next tile's loads in flight under this tile's arg-max
      const int np1 = p1 - q1 < TB ? p1 - q1 : TB, tot1 = np1 * n4;
#pragma unroll
      for (int k = 0; k < MAXN4; ++k)
        if (k < n4 && t + k * TB < tot1) reg[k] = src[(long)q1 * n4 + t + k * TB];
      if (t < np1) treg = target[fbase + q1 + t];
    }
    const bool live = t < np;
    int cell = -1;
    if (live) {
      int pred;
      cell = segscore::score_pixel(tile + t * s, tg, C, &pred);
      if (label_out) label_out[fbase + q0 + t] = pred;
    }
    nskip += __popcll(__ballot(live && cell < 0));
    unsigned long long rem = __ballot(cell >= 0);              // the distinct cells among this wave's pixels, lowest lane first
    while (rem) {
      const int c = __shfl(cell, __ffsll((long long)rem) - 1);
      const unsigned long long m = __ballot(cell == c);
      if (lane == 0) atomicAdd(&table[c], __popcll(m));
      rem &= ~m;
    }
  }
  if (lane == 0 && nskip) atomicAdd(&table[cells], nskip);
  __syncthreads();
  int *out = conf + (size_t)f * cells;
  for (int i = t; i < cells; i += TB) {
    const int v = table[i];
    if (v) atomicAdd(&out[i], v);
  }
  if (t == 0 && table[cells]) atomicAdd(&skipped[f], table[cells]);
}

// pair n of a launch: its frame, class and the corner of the frame's window
struct MaskPairs {
  int f[MASK_PAIRS], cls[MASK_PAIRS], y0[MASK_PAIRS], x0[MASK_PAIRS];
};

// grid = (column blocks, IH, pairs of the launch); mask points at the launch's first pair
__global__ __launch_bounds__(TB) void seg_masks_kernel(const int *__restrict__ label, int H, int W, MaskPairs mp, int IH, int IW,
                                                       unsigned short *__restrict__ mask) {
  const int n = blockIdx.z, y = blockIdx.y, x = blockIdx.x * TB + threadIdx.x;
  if (x >= IW) return;
  const int *lf = label + (size_t)mp.f[n] * H * W;
  mask[((size_t)n * IH + y) * IW + x] = segscore::mask_pixel(lf, H, W, mp.y0[n], mp.x0[n], mp.cls[n], y, x);
}

}  // namespace
}  // namespace df

using namespace df;

extern "C" int df_seg_score_block_pixels(void) { return SCORE_PPB; }

extern "C" int df_seg_score(const float *logits, const int64_t *target, int F, int H, int W, int ld, int C, int *label_out, int *conf,
                            int *skipped, df_stream_t stream) {
  const char *name = "seg_score";
  if (!logits || !target || !conf || !skipped) return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (F < 1 || F > 65535 || H < 1 || W < 1 || (long)H * W > (1L << 30))
    return set_error(DF_ERR_ARG, "%s: need 1 <= F <= 65535, H, W >= 1 and H * W <= 2^30 (F %d, H %d, W %d)", name, F, H, W);
  if (C < 2 || C > segscore::MAX_CLASSES || ld < C || ld % 4 || ld > segscore::MAX_LD)
    return set_error(DF_ERR_ARG, "%s: need 2 <= C <= %d, C <= ld <= %d, ld a multiple of 4 (C %d, ld %d)", name, segscore::MAX_CLASSES,
                     segscore::MAX_LD, C, ld);
  if (reinterpret_cast<uintptr_t>(logits) % 16 || reinterpret_cast<uintptr_t>(target) % 8 || reinterpret_cast<uintptr_t>(label_out) % 4 ||
      reinterpret_cast<uintptr_t>(conf) % 4 || reinterpret_cast<uintptr_t>(skipped) % 4)
    return set_error(DF_ERR_ARG, "%s: logits must be 16-byte, target 8-byte, label_out, conf and skipped 4-byte aligned", name);
  const int HW = H * W, parts = cdiv(HW, SCORE_PPB), lds = score_lds_bytes(ld, C);
  const bool wide = ld > 32;
  // above 64 KiB of dynamic LDS from ld 56 on; the limit is set once per kernel, to the largest tile and table it takes
  if (wide)
    if (int e = raise_lds_limit(reinterpret_cast<const void *>(seg_score_kernel<MAX_LD4>), score_lds_bytes(segscore::MAX_LD, segscore::MAX_CLASSES)))
      return e;
  hipStream_t st = to_stream(stream);
  if (hipMemsetAsync(conf, 0, sizeof(int) * (size_t)F * C * C, st) != hipSuccess || hipMemsetAsync(skipped, 0, sizeof(int) * (size_t)F, st) != hipSuccess)
    return check_launch(name);
  if (wide)
    hipLaunchKernelGGL(seg_score_kernel<MAX_LD4>, dim3(parts, F), dim3(TB), lds, st, logits, target, HW, ld, C, label_out, conf, skipped);
  else
    hipLaunchKernelGGL(seg_score_kernel<8>, dim3(parts, F), dim3(TB), lds, st, logits, target, HW, ld, C, label_out, conf, skipped);
  return check_launch(name);
}

extern "C" int df_seg_masks(const int *label, int F, int H, int W, const int *win, const int *pairs, int N, int IH, int IW,
                            unsigned short *mask_out, df_stream_t stream) {
  const char *name = "seg_masks";
  if (!label || !win || !pairs || !mask_out) return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (F < 1 || F > 65535 || N < 1 || IH < 1 || IH > 65535 || IW < 1 || (long)IH * IW > (1L << 30))
    return set_error(DF_ERR_ARG, "%s: need 1 <= F <= 65535, N >= 1, 1 <= IH <= 65535, IW >= 1 and IH * IW <= 2^30", name);
  if (H < 1 || H > IH || W < 1 || W > IW) return set_error(DF_ERR_ARG, "%s: window %d x %d outside the %d x %d frame", name, H, W, IH, IW);
  if (reinterpret_cast<uintptr_t>(label) % 4 || reinterpret_cast<uintptr_t>(mask_out) % 2)
    return set_error(DF_ERR_ARG, "%s: label must be 4-byte and mask_out 2-byte aligned", name);
  for (int f = 0; f < F; ++f)
    if (!segscore::window_ok(win[2 * f], win[2 * f + 1], H, W, IH, IW))
      return set_error(DF_ERR_ARG, "%s: frame %d: window corner (%d, %d) leaves the %d x %d frame", name, f, win[2 * f], win[2 * f + 1], IH, IW);
  for (int n = 0; n < N; ++n)
    if (!segscore::pair_ok(pairs[2 * n], pairs[2 * n + 1], F))
      return set_error(DF_ERR_ARG, "%s: pair %d: frame %d outside 0..%d or class %d outside 0..%d", name, n, pairs[2 * n], F - 1,
                       pairs[2 * n + 1], segscore::MAX_CLASSES);
  hipStream_t st = to_stream(stream);
  for (int n0 = 0; n0 < N; n0 += MASK_PAIRS) {
    const int nn = N - n0 < MASK_PAIRS ? N - n0 : MASK_PAIRS;
    MaskPairs mp = {};
    for (int k = 0; k < nn; ++k) {
      const int f = pairs[2 * (n0 + k)];
      mp.f[k] = f; mp.cls[k] = pairs[2 * (n0 + k) + 1]; mp.y0[k] = win[2 * f]; mp.x0[k] = win[2 * f + 1];
    }
    hipLaunchKernelGGL(seg_masks_kernel, dim3(cdiv(IW, TB), IH, nn), dim3(TB), 0, st, label, H, W, mp, IH, IW,
                       mask_out + (size_t)n0 * IH * IW);
  }
  return check_launch(name);
}
