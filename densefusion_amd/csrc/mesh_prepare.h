// The triangle-record kernel (steps M1, M2) that df_mesh_closest and df_mesh_icp both launch once per call: one thread per triangle
// writes its 32-double record.  Stated once here; each of the two files gets its own copy of the kernel.
#pragma once
#include "common.h"
#include "mesh_closest_core.h"

namespace df {
namespace {

constexpr int MESH_PREPARE_BLOCK = 256;   // threads per workgroup

__global__ __launch_bounds__(MESH_PREPARE_BLOCK) void mesh_prepare_kernel(const float *__restrict__ vertices, int V,
                                                                          const int *__restrict__ triangles, int T,
                                                                          meshclosest::TriRec *__restrict__ rec) {
  const int t = blockIdx.x * MESH_PREPARE_BLOCK + threadIdx.x;
  if (t >= T) return;
  meshclosest::TriRec r;
  meshclosest::prepare_tri(vertices, V, triangles[3 * (size_t)t], triangles[3 * (size_t)t + 1], triangles[3 * (size_t)t + 2], &r);
  rec[t] = r;
}

}  // namespace
}  // namespace df
