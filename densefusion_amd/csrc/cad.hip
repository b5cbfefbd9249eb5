// Input preparation for the customCAD dataset (Unity renders; datasets/customCAD/dataset.py:109-166,205 and project_unity_depth.py:42-51
// of the reference).  Differs from preprocess.hip in four ways: the mask is (label == 65535) & (depth != the frame's largest depth), the
// colour crop is grey where the depth is that "infinite" value, the cloud comes from a per-pixel ray map and Unity's non-linear depth
// decode instead of pinhole intrinsics, and the box is the mask's own (df_cad_frame_stats finds it).  The `choose` rule is the shared one
// of choose_core.h.
#include "cad_stats.h"
#include "choose_core.h"

namespace df {
namespace {

using namespace prep;

// grid = B objects, block = 1024.  rgb [F][IH][IW][3] u8, depth / label [F][IH][IW] u16, ray_map [IH][IW][3] f64.
__global__ __launch_bounds__(PB) void preprocess_cad_kernel(const unsigned char *__restrict__ rgb, const unsigned short *__restrict__ depth,
                                                            const unsigned short *__restrict__ label, const ObjDesc *__restrict__ objs,
                                                            const int *__restrict__ frame_stats, const double *__restrict__ ray_map, int F,
                                                            int IH, int IW, int H, int W, int N, double p22, double p23,
                                                            const double *__restrict__ add_t, float cloud_div, int *__restrict__ nz_scratch,
                                                            float *__restrict__ img, float *__restrict__ cloud, int64_t *__restrict__ choose,
                                                            int *__restrict__ count_out) {
  __shared__ ChooseShared s_choose;
  const int b = blockIdx.x, tid = threadIdx.x;
  const ObjDesc o = objs[b];
  int64_t *ch = choose + (size_t)b * N;
  // the descriptors are device memory the host call cannot check: a box that leaves its frame is reported as an empty object, never read
  if (o.frame < 0 || o.frame >= F || o.rmin < 0 || o.cmin < 0 || o.rmax - o.rmin != H || o.cmax - o.cmin != W || o.rmax > IH || o.cmax > IW) {
    for (int j = tid; j < N; j += PB) ch[j] = 0;
    if (tid == 0) count_out[b] = 0;
    return;
  }
  const size_t fbase = (size_t)o.frame * IH * IW;
  const int HW = H * W;
  const int dmax = frame_stats[(size_t)o.frame * 6];          // np.max(depth): Unity's far plane, "infinitely" far (dataset.py:120,132)
  auto in_mask = [&](int i) {
    const int r = o.rmin + i / W, c = o.cmin + i % W;
    const size_t p = fbase + (size_t)r * IW + c;
    return (int)label[p] == o.itemid && (int)depth[p] != dmax;       // dataset.py:120-124
  };
  choose_pixels(in_mask, o.seed, o.given, HW, N, nz_scratch + (size_t)b * HW, ch, count_out + b, s_choose);
  // 3. cloud of the chosen pixels in fp64, one rounding per step like numpy's (project_unity_depth.py:45-50; dataset.py:161-166,205)
  float *cl = cloud + (size_t)b * N * 3;
  for (int j = tid; j < N; j += PB) {
    const int i = (int)ch[j];
    const int r = o.rmin + i / W, c = o.cmin + i % W;
    const double dn = (double)depth[fbase + (size_t)r * IW + c] / 65534.0;
    const double z = -p23 / (p22 + (1.0 - dn));
    const double *ray = ray_map + ((size_t)r * IW + c) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v = (float)(ray[k] * z);                                          // .astype(np.float32), :161
      if (add_t) v = (float)((double)v + add_t[(size_t)b * 3 + k]);           // np.add(float32 cloud, float64 add_t), then .astype(np.float32)
      cl[j * 3 + k] = v / cloud_div;
    }
  }
  // 4. normalised colour crop, CHW; grey where the depth is the frame's maximum (dataset.py:97,132)
  float *im = img + (size_t)b * 3 * HW;
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  for (int i = tid; i < HW; i += PB) {
    const int r = o.rmin + i / W, c = o.cmin + i % W;
    const size_t p = fbase + (size_t)r * IW + c;
    const bool far = (int)depth[p] == dmax;
    const unsigned char *px = rgb + p * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) im[(size_t)k * HW + i] = ((float)(far ? (unsigned char)130 : px[k]) - mean[k]) / stdv[k];
  }
}

}  // namespace
}  // namespace df

using namespace df;

extern "C" int df_cad_frame_stats(const unsigned short *depth, const unsigned short *label, int num_frames, int IH, int IW, int label_value,
                                  int *stats, df_stream_t stream) {
  if (!depth || !label || !stats) return set_error(DF_ERR_ARG, "cad_frame_stats: null pointer");
  if (!stats_sizes_ok(num_frames, IH, IW, label_value))
    return set_error(DF_ERR_ARG, "cad_frame_stats: bad sizes");
  hipStream_t st = to_stream(stream);
  if (hipMemsetAsync(stats, 0, sizeof(int) * 6 * num_frames, st) != hipSuccess) return check_launch("cad_frame_stats (init)");
  hipLaunchKernelGGL(frame_stats_kernel, dim3(stats_blocks(IH, IW), num_frames), dim3(SB), 0, st, depth, label, IH, IW, label_value, stats, 6);
  hipLaunchKernelGGL(stats_finish_kernel, dim3(cdiv(num_frames, SB)), dim3(SB), 0, st, num_frames, IH, IW, stats, 6);
  return check_launch("cad_frame_stats");
}

extern "C" int df_preprocess_objects_cad(const unsigned char *rgb, const unsigned short *depth, const unsigned short *label, int num_frames,
                                         int IH, int IW, const int *obj_desc, const int *frame_stats, const double *ray_map, double p22,
                                         double p23, const double *add_t, int B, int H, int W, int num_points, float cloud_div, int *scratch,
                                         float *img_out, float *cloud_out, int64_t *choose_out, int *count_out, df_stream_t stream) {
  if (!rgb || !depth || !label || !obj_desc || !frame_stats || !ray_map || !scratch || !img_out || !cloud_out || !choose_out || !count_out)
    return set_error(DF_ERR_ARG, "preprocess_cad: null pointer");
  if (B <= 0 || num_frames <= 0 || IH <= 0 || IW <= 0 || (long)IH * IW > (1L << 30) || H <= 0 || W <= 0 || H > IH || W > IW ||
      num_points <= 0 || !(cloud_div > 0.f))
    return set_error(DF_ERR_ARG, "preprocess_cad: bad sizes");
  hipLaunchKernelGGL(preprocess_cad_kernel, dim3(B), dim3(PB), 0, to_stream(stream), rgb, depth, label,
                     reinterpret_cast<const ObjDesc *>(obj_desc), frame_stats, ray_map, num_frames, IH, IW, H, W, num_points, p22, p23, add_t,
                     cloud_div, scratch, img_out, cloud_out, choose_out, count_out);
  return check_launch("preprocess_cad");
}
