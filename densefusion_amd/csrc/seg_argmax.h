// The label rule shared by segment.hip (df_segment_detect) and seg_score.hip (df_seg_score): one statement of the arg-max, so that the
// label map the pose path reads and the one the confusion matrix scores agree on every tie and every NaN.
#pragma once
#include "seg_norm.h"

namespace df {

// arg-max over the first C channels of one pixel's logits, x = its float4s: first maximum wins, NaN counts as maximal (torch.argmax);
// only the float4s that hold a class are read, and of the last one only the lanes below C
__host__ __device__ __forceinline__ int seg_argmax(const f32x4 *x, int C) {
  const int cq = (C + 3) >> 2;
  f32x4 v = x[0];
  float best = v[0];
  int bi = 0;
  for (int j = 0; j < cq; ++j) {
    if (j) v = x[j];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * j + e;
      if (c > 0 && c < C && (v[e] > best || (__builtin_isnan(v[e]) && !__builtin_isnan(best)))) { best = v[e]; bi = c; }
    }
  }
  return bi;
}

}  // namespace df
