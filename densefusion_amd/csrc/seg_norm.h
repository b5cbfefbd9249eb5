// SegNet's input normalisation, shared by segment.hip (df_segment_input, the eval path) and seg_feed.hip (df_seg_batch, the training
// feed): one statement of the rule, so that the two inputs agree bit for bit on the same bytes.
#pragma once
#include "common.h"

namespace df {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ((float)v - mean) / std with true division, per channel, on the 0..255 values (no / 255: the reference's own normalisation,
// vanilla_segmentation/data_controller.py:79); the constants are the fp32 roundings numpy makes of the reference's literals
__host__ __device__ __forceinline__ f32x4 seg_norm(unsigned r, unsigned g, unsigned b) {
  const float m0 = (float)0.485, m1 = (float)0.456, m2 = (float)0.406, s0 = (float)0.229, s1 = (float)0.224, s2 = (float)0.225;
  f32x4 o;
  o[0] = ((float)r - m0) / s0;
  o[1] = ((float)g - m1) / s1;
  o[2] = ((float)b - m2) / s2;
  o[3] = 0.f;
  return o;
}

}  // namespace df
