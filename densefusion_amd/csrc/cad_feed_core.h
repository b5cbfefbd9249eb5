// The per-element rules of cad_feed.hip (df_cad_item_table, df_cad_targets), host and device alike; the contract is the comment of the
// two calls in include/dfusion.h and tests/cad_feed_np.py restates it in numpy.  Built with -ffp-contract=off: no fused multiply-add.
#pragma once
#include "common.h"

namespace df {
namespace feed {

// a pixel of the loader's mask (dataset.py:120-124): the label, off the frame's depth maximum
__host__ __device__ inline bool mask_pixel(int label, int depth, int label_value, int depth_max) {
  return label == label_value && depth != depth_max;
}

// PoseDataset._live_box plus the count test: a frame that yields an item
__host__ __device__ inline int item_live(int n_label, int rmin, int rmax, int cmin, int cmax, int count, int min_side) {
  return n_label > 0 && rmax - rmin >= min_side && cmax - cmin >= min_side && count > 0;
}

// One model point in fp64, one rounding per operation: m = model * model_scale; model_points = (float)m / cloud_div in fp32;
// X_j = ((R[j][0] m_x + R[j][1] m_y) + R[j][2] m_z) + T_j; target = (float)X_j / cloud_div.  pose: 12 doubles, row-major [R|T].
__host__ __device__ inline void target_point(const double *__restrict__ model, double model_scale, const double *__restrict__ pose,
                                             float cloud_div, float *__restrict__ model_points, float *__restrict__ target) {
  const double mx = model[0] * model_scale, my = model[1] * model_scale, mz = model[2] * model_scale;
  model_points[0] = (float)mx / cloud_div; model_points[1] = (float)my / cloud_div; model_points[2] = (float)mz / cloud_div;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double *r = pose + j * 4;
    const double x = ((r[0] * mx + r[1] * my) + r[2] * mz) + r[3];
    target[j] = (float)x / cloud_div;
  }
}

}  // namespace feed
}  // namespace df
