// Per-object input preparation on the device: what tools/eval_ycb.py:147-181 does in numpy
// between the detector's ROI and the network call -- mask = (depth != 0) & (label == itemid) inside the snapped
// bounding box, `choose` = up to num_points mask pixels (random subset when there are more, wrap-padding when
// fewer, eval_ycb.py:155-163), back-projection of the chosen depth pixels to a cloud (:165-173) and the
// ImageNet-normalised crop of the colour image (:175-181, on 0..255-scale values exactly like the reference).
//
// Mask compaction and the `choose` rule (steps 1-2, with the RNG contract) live in choose_core.h, shared with cad.hip.
#include "choose_core.h"

namespace df {
namespace {

using namespace prep;

// grid = B objects, block = 1024.  rgb [F][IH][IW][3] u8, depth [F][IH][IW] u16, label [F][IH][IW] i32.
__global__ __launch_bounds__(PB) void preprocess_kernel(const unsigned char *__restrict__ rgb, const unsigned short *__restrict__ depth,
                                                        const int *__restrict__ label, const ObjDesc *__restrict__ objs, int IH,
                                                        int IW, int H, int W, int N, float cx, float cy, float fx, float fy,
                                                        float cam_scale, float cloud_div, int *__restrict__ nz_scratch, float *__restrict__ img,
                                                        float *__restrict__ cloud, int64_t *__restrict__ choose,
                                                        int *__restrict__ count_out) {
  __shared__ ChooseShared s_choose;
  const int b = blockIdx.x, tid = threadIdx.x;
  const ObjDesc o = objs[b];
  const size_t fbase = (size_t)o.frame * IH * IW;
  const int HW = H * W;
  auto in_mask = [&](int i) {
    const int r = o.rmin + i / W, c = o.cmin + i % W;
    const size_t p = fbase + (size_t)r * IW + c;
    return depth[p] != 0 && label[p] == o.itemid;
  };
  int64_t *ch = choose + (size_t)b * N;
  choose_pixels(in_mask, o.seed, o.given, HW, N, nz_scratch + (size_t)b * HW, ch, count_out + b, s_choose);
  // 3. cloud from the chosen depth pixels (eval_ycb.py:165-173; xmap = row index, ymap = column index)
  float *cl = cloud + (size_t)b * N * 3;
  for (int j = tid; j < N; j += PB) {
    const int i = (int)ch[j];
    const int r = o.rmin + i / W, c = o.cmin + i % W;
    const float d = (float)depth[fbase + (size_t)r * IW + c];
    const float pt2 = d / cam_scale;
    // cloud_div: the LineMOD loader back-projects in depth units and divides the finished cloud by 1000
    // (datasets/linemod/dataset.py:152-157); the YCB path passes 1 (x / 1 == x)
    cl[j * 3 + 0] = ((float)c - cx) * pt2 / fx / cloud_div;
    cl[j * 3 + 1] = ((float)r - cy) * pt2 / fy / cloud_div;
    cl[j * 3 + 2] = pt2 / cloud_div;
  }
  // 4. normalised colour crop, CHW (eval_ycb.py:175-181)
  float *im = img + (size_t)b * 3 * HW;
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  for (int i = tid; i < HW; i += PB) {
    const int r = o.rmin + i / W, c = o.cmin + i % W;
    const unsigned char *px = rgb + (fbase + (size_t)r * IW + c) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) im[(size_t)k * HW + i] = ((float)px[k] - mean[k]) / stdv[k];
  }
}

}  // namespace
}  // namespace df

using namespace df;

extern "C" int df_preprocess_objects(const unsigned char *rgb, const unsigned short *depth, const int *label, int num_frames,
                                     int IH, int IW, const int *obj_desc, int B, int H, int W, int num_points, float cam_cx,
                                     float cam_cy, float cam_fx, float cam_fy, float cam_scale, float cloud_div, int *scratch, float *img_out,
                                     float *cloud_out, int64_t *choose_out, int *count_out, df_stream_t stream) {
  if (!rgb || !depth || !label || !obj_desc || !scratch || !img_out || !cloud_out || !choose_out || !count_out)
    return set_error(DF_ERR_ARG, "preprocess: null pointer");
  if (B <= 0 || num_frames <= 0 || H <= 0 || W <= 0 || H > IH || W > IW || num_points <= 0 || !(cam_scale > 0.f) || !(cloud_div > 0.f))
    return set_error(DF_ERR_ARG, "preprocess: bad sizes");
  hipLaunchKernelGGL(preprocess_kernel, dim3(B), dim3(PB), 0, to_stream(stream), rgb, depth, label,
                     reinterpret_cast<const ObjDesc *>(obj_desc), IH, IW, H, W, num_points, cam_cx, cam_cy, cam_fx, cam_fy, cam_scale,
                     cloud_div, scratch, img_out, cloud_out, choose_out, count_out);
  return check_launch("preprocess");
}
