// What a customCAD item still needed from the host once its frame is rendered on the device: the number of mask pixels in the crop
// (PoseDataset._count) with the live test (df_cad_item_table), and the model subset with the target arithmetic (PoseDataset._targets,
// df_cad_targets).  The contract -- every operation and its order -- is the comment of the two calls in include/dfusion.h;
// tests/cad_feed_np.py restates it in numpy and the outputs are compared bit for bit.  The statistics pass and its reduction scheme are
// those of df_cad_frame_stats (cad_stats.h), the subset is choose_pixels (choose_core.h) with an all-true predicate.
// Built with -ffp-contract=off: no fused multiply-add anywhere.
#include "cad_feed_core.h"
#include "cad_stats.h"
#include "choose_core.h"

namespace df {
namespace {

using namespace prep;

constexpr int ROW = 8;                 // ints per row of the item table

// The second pass: the mask pixels of the half-open crop [rmin:rmax, cmin:cmax] of the box the first pass left in the row, into entry 6.
// grid = (blocks, F); the threads stride over the crop's pixels; wave sum, then one integer atomic per wave.
__global__ __launch_bounds__(SB) void item_count_kernel(const unsigned short *__restrict__ depth, const unsigned short *__restrict__ label,
                                                        int IH, int IW, int label_value, int *__restrict__ table) {
  const int f = blockIdx.y;
  int *s = table + (size_t)f * ROW;
  const int dmax = s[0], rmin = s[2], cmin = s[4];
  const int H = s[1] > 0 ? s[3] - rmin : 0, W = s[1] > 0 ? s[5] - cmin : 0;      // inside the frame: the box is that of its own pixels
  const size_t fbase = (size_t)f * IH * IW;
  const int HW = H * W;
  int cnt = 0;
  for (int i = blockIdx.x * SB + threadIdx.x; i < HW; i += gridDim.x * SB) {
    const int r = rmin + i / W, c = cmin + i % W;
    const size_t p = fbase + (size_t)r * IW + c;
    cnt += feed::mask_pixel(label[p], depth[p], label_value, dmax);
  }
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&s[6], cnt);
}

__global__ void item_finish_kernel(int F, int min_side, int *__restrict__ table) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  int *s = table + (size_t)f * ROW;
  s[7] = feed::item_live(s[1], s[2], s[3], s[4], s[5], s[6], min_side);
}

// grid = B items, block = 1024.  nz [B][P], ch [B][M] and count [B] are the call's scratch.
__global__ __launch_bounds__(PB) void targets_kernel(const double *__restrict__ model, int P, double model_scale,
                                                     const double *__restrict__ pose, const unsigned *__restrict__ seed, int M,
                                                     float cloud_div, int *__restrict__ nz, int64_t *__restrict__ choose,
                                                     int *__restrict__ count, float *__restrict__ model_points,
                                                     float *__restrict__ target) {
  __shared__ ChooseShared s_choose;
  const int b = blockIdx.x;
  int64_t *ch = choose + (size_t)b * M;
  choose_pixels([](int) { return true; }, seed[b], 0, P, M, nz + (size_t)b * P, ch, count + b, s_choose);
  const double *T = pose + (size_t)b * 12;
  for (int j = threadIdx.x; j < M; j += PB) {
    const size_t o = ((size_t)b * M + j) * 3;
    feed::target_point(model + (size_t)ch[j] * 3, model_scale, T, cloud_div, model_points + o, target + o);
  }
}

}  // namespace
}  // namespace df

using namespace df;

extern "C" int df_cad_item_table(const unsigned short *depth, const unsigned short *label, int num_frames, int IH, int IW, int label_value,
                                 int min_side, int *table, df_stream_t stream) {
  if (!depth || !label || !table) return set_error(DF_ERR_ARG, "cad_item_table: null pointer");
  if (!stats_sizes_ok(num_frames, IH, IW, label_value) || min_side < 0) return set_error(DF_ERR_ARG, "cad_item_table: bad sizes");
  hipStream_t st = to_stream(stream);
  if (hipMemsetAsync(table, 0, sizeof(int) * ROW * num_frames, st) != hipSuccess) return check_launch("cad_item_table (init)");
  const dim3 grid(stats_blocks(IH, IW), num_frames), rows(cdiv(num_frames, SB));
  hipLaunchKernelGGL(frame_stats_kernel, grid, dim3(SB), 0, st, depth, label, IH, IW, label_value, table, ROW);
  hipLaunchKernelGGL(stats_finish_kernel, rows, dim3(SB), 0, st, num_frames, IH, IW, table, ROW);
  hipLaunchKernelGGL(item_count_kernel, grid, dim3(SB), 0, st, depth, label, IH, IW, label_value, table);
  hipLaunchKernelGGL(item_finish_kernel, rows, dim3(SB), 0, st, num_frames, min_side, table);
  return check_launch("cad_item_table");
}

extern "C" size_t df_cad_targets_scratch_bytes(int B, int P, int M) {
  if (B <= 0 || B > 65535 || M <= 0 || P < M || P > (1 << 24)) return 0;
  return (size_t)B * ((size_t)M * sizeof(int64_t) + ((size_t)P + 1) * sizeof(int));
}

extern "C" int df_cad_targets(const double *model, int P, double model_scale, const double *pose, const unsigned *seed, int B, int M,
                              float cloud_div, void *scratch, size_t scratch_bytes, float *model_points_out, float *target_out,
                              df_stream_t stream) {
  if (!model || !pose || !seed || !scratch || !model_points_out || !target_out) return set_error(DF_ERR_ARG, "cad_targets: null pointer");
  const size_t need = df_cad_targets_scratch_bytes(B, P, M);
  if (need == 0 || !(cloud_div > 0.f))
    return set_error(DF_ERR_ARG, "cad_targets: bad sizes (B 1..65535, 1 <= M <= P <= 2^24, cloud_div > 0); got B %d, P %d, M %d", B, P, M);
  if (scratch_bytes < need || (reinterpret_cast<uintptr_t>(scratch) & 7u))
    return set_error(DF_ERR_ARG, "cad_targets: scratch too small or not 8-byte aligned");
  int64_t *ch = static_cast<int64_t *>(scratch);
  int *nz = reinterpret_cast<int *>(ch + (size_t)B * M);
  hipLaunchKernelGGL(targets_kernel, dim3(B), dim3(PB), 0, to_stream(stream), model, P, model_scale, pose, seed, M, cloud_div, nz, ch,
                     nz + (size_t)B * P, model_points_out, target_out);
  return check_launch("cad_targets");
}
