// The per-frame statistics pass of the customCAD loader, shared by cad.hip (df_cad_frame_stats: rows of 6) and cad_feed.hip
// (df_cad_item_table: rows of 8, whose first six entries are the same row): one wave-then-atomic reduction scheme, stated once.  Each
// translation unit gets its own copy of the kernels.
#pragma once
#include "common.h"

namespace df {
namespace {

constexpr int SB = 256;               // frame_stats: threads per block
constexpr int STATS_MAX_BLOCKS = 64;   // ... and blocks per frame

// a wave's sum / maximum, valid in lane 0
__device__ inline int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ inline int wave_max(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_down(v, off, 64));
  return v;
}

// Per-frame integer statistics.  While the blocks reduce, a row of `stats` (`row` ints apart) holds maxima only, so that zero means
// "nothing seen": {max depth, label pixels, max(IH - row), max(row + 1), max(IW - col), max(col + 1)}; stats_finish_kernel decodes the row
// in place.  Integer atomics: the result does not depend on the order of arrival.  grid = (blocks, F).
__global__ __launch_bounds__(SB) void frame_stats_kernel(const unsigned short *__restrict__ depth, const unsigned short *__restrict__ label,
                                                         int IH, int IW, int label_value, int *__restrict__ stats, int row) {
  const int f = blockIdx.y;
  const int npix = IH * IW;
  const unsigned short *d = depth + (size_t)f * npix, *l = label + (size_t)f * npix;
  int dmax = 0, cnt = 0, a_r = 0, b_r = 0, a_c = 0, b_c = 0;
  auto see = [&](int i, int dv, int lv) {
    dmax = max(dmax, dv);
    if (lv == label_value) {
      const int r = i / IW, c = i - r * IW;
      ++cnt;
      a_r = max(a_r, IH - r); b_r = max(b_r, r + 1);
      a_c = max(a_c, IW - c); b_c = max(b_c, c + 1);
    }
  };
  const int first = blockIdx.x * SB + threadIdx.x, step = gridDim.x * SB;
  int done = 0;
  if (((reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(l)) & 7u) == 0) {       // this frame starts on an 8-byte boundary: four pixels a load
    const int nq = npix / 4;
    const ushort4 *d4 = reinterpret_cast<const ushort4 *>(d), *l4 = reinterpret_cast<const ushort4 *>(l);
    for (int q = first; q < nq; q += step) {
      const ushort4 dv = d4[q], lv = l4[q];
      see(4 * q, dv.x, lv.x); see(4 * q + 1, dv.y, lv.y); see(4 * q + 2, dv.z, lv.z); see(4 * q + 3, dv.w, lv.w);
    }
    done = 4 * nq;
  }
  for (int i = done + first; i < npix; i += step) see(i, d[i], l[i]);
  dmax = wave_max(dmax); cnt = wave_sum(cnt);
  a_r = wave_max(a_r); b_r = wave_max(b_r); a_c = wave_max(a_c); b_c = wave_max(b_c);
  if ((threadIdx.x & 63) == 0) {
    int *s = stats + (size_t)f * row;
    if (dmax) atomicMax(&s[0], dmax);
    if (cnt) {
      atomicAdd(&s[1], cnt);
      atomicMax(&s[2], a_r); atomicMax(&s[3], b_r); atomicMax(&s[4], a_c); atomicMax(&s[5], b_c);
    }
  }
}

// {depth_max, n_label, rmin, rmax, cmin, cmax}, the box inclusive like get_bbox (dataset.py:247-249); zero box without the label
__global__ void stats_finish_kernel(int F, int IH, int IW, int *__restrict__ stats, int row) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  int *s = stats + (size_t)f * row;
  if (s[1] == 0) { s[2] = s[3] = s[4] = s[5] = 0; return; }
  s[2] = IH - s[2]; s[3] = s[3] - 1; s[4] = IW - s[4]; s[5] = s[5] - 1;
}

inline bool stats_sizes_ok(int F, int IH, int IW, int label_value) {
  return F > 0 && F <= 65535 && IH > 0 && IW > 0 && (long)IH * IW <= (1L << 30) && label_value >= 0 && label_value <= 65535;
}

// blocks per frame of the statistics passes: a block for every SB quads of the frame, at most STATS_MAX_BLOCKS (the threads stride)
inline int stats_blocks(int IH, int IW) {
  const long quads = ((long)IH * IW + 3) / 4;
  return cdiv(quads, SB) < STATS_MAX_BLOCKS ? cdiv(quads, SB) : STATS_MAX_BLOCKS;
}

}  // namespace
}  // namespace df
