// The per-pixel rules of df_seg_score (steps S1..S3 of its comment in include/dfusion.h) and df_seg_masks (M1), as __host__ __device__
// functions: the kernels of seg_score.hip call them per lane, a CPU program can call them per pixel.  Integers only after the arg-max.
#pragma once
#include "seg_argmax.h"

namespace df {
namespace segscore {

constexpr int MAX_CLASSES = 64, MAX_LD = 64;

// S2: the cell of conf [C][C] a pixel of truth class `target` and predicted class `pred` adds to, truth * C + pred; -1 for a target
// outside 0..C-1, which adds to `skipped` instead (the comparison is made on all 64 bits: 2^40 is outside, not 0)
__host__ __device__ inline int cell_of(int64_t target, int pred, int C) {
  return target >= 0 && target < (int64_t)C ? (int)target * C + pred : -1;
}

// S1 + S2 of one pixel from its ld / 4 float4s: the predicted class goes to *pred, the cell (or -1) comes back
__host__ __device__ inline int score_pixel(const f32x4 *x, int64_t target, int C, int *pred) {
  *pred = seg_argmax(x, C);
  return cell_of(target, *pred, C);
}

// the rule of a df_seg_masks pair: a frame of the call, a class SegNet can name, its frame's window inside the IH x IW frame
__host__ __device__ inline bool pair_ok(int f, int cls, int F) { return f >= 0 && f < F && cls >= 0 && cls <= MAX_CLASSES; }
__host__ __device__ inline bool window_ok(int y0, int x0, int H, int W, int IH, int IW) {
  return y0 >= 0 && y0 <= IH - H && x0 >= 0 && x0 <= IW - W;
}

// M1: frame pixel (y, x) of the mask of class `cls`, from its frame's H x W label window whose corner is (y0, x0)
__host__ __device__ inline unsigned short mask_pixel(const int *label, int H, int W, int y0, int x0, int cls, int y, int x) {
  const int i = y - y0, j = x - x0;
  return i >= 0 && i < H && j >= 0 && j < W && label[(size_t)i * W + j] == cls ? (unsigned short)65535 : (unsigned short)0;
}

}  // namespace segscore
}  // namespace df
