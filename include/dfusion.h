/* dfusion.h -- C ABI of libdfusion_hip.so, the MI355X (gfx950) implementation of the DenseFusion
 * 6D-pose hot path.  Plain pointers and sizes only; every pointer is a DEVICE pointer unless a
 * parameter says "host".  No function allocates persistent device memory behind the caller's back
 * during a forward call, none synchronises the device, and every launch goes on the stream that is
 * passed in (so a caller may capture a call sequence into a hipGraph).
 *
 * Status convention: 0 = ok, negative = error; df_last_error() returns a thread-local message.
 * (The reference's `int knn(...)` returns 1 on success and raises through THError otherwise,
 * lib/knn/src/knn_pytorch.c:41-47; the Python shim maps a non-zero status to RuntimeError.)
 */
#ifndef DFUSION_H_
#define DFUSION_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *df_stream_t; /* a hipStream_t; NULL = the default stream */

#define DF_OK 0
#define DF_ERR_ARG (-1)       /* bad argument (THArgCheck in the reference, knn_pytorch.c:11-16) */
#define DF_ERR_LAUNCH (-2)    /* hipGetLastError() != hipSuccess after a launch (knn_pytorch.c:41-45) */
#define DF_ERR_WORKSPACE (-3) /* caller-provided workspace too small */
#define DF_ERR_STATE (-4)     /* handle not ready (missing parameters) */

const char *df_last_error(void);
int df_version(void);

/* ------------------------------------------------------------------------------------------------
 * 1-NN / k-NN  (replaces lib/knn: `knn_device`, lib/knn/src/knn_cuda_kernel.h:14-16 + .cu:211-259)
 *
 * ref_dev   [dim][ref_nb]   fp32, point index fastest (the layout knn_pytorch.c:21-29 hands over)
 * query_dev [dim][query_nb] fp32
 * ind_dev   [k][query_nb]   int64, 1-BASED row index of the k nearest reference points, nearest first;
 *                           ties go to the lowest index (strict '<' in cuInsertionSort, .cu:128,152)
 * The reference's `dist_dev` scratch (ref_nb*query_nb floats, knn_pytorch.c:31) does not exist here:
 * distances never leave registers.  dim == 3, k == 1 (the only use on the path) takes the fused
 * kernel; any other dim / k <= DF_KNN_MAX_K takes a generic one.
 */
#define DF_KNN_MAX_K 32
int df_knn_device(const float *ref_dev, int ref_nb, const float *query_dev, int query_nb, int dim, int k,
                  int64_t *ind_dev, df_stream_t stream);

/* Batched form = `int knn(ref, query, idx)` of lib/knn/src/knn_pytorch.h:1-2 with the tensors spelled out:
 * ref [batch][dim][ref_nb], query [batch][dim][query_nb], idx [batch][k][query_nb].  One launch for
 * the whole batch (the reference loops batches on the host, knn_pytorch.c:33-36). */
int df_knn(const float *ref, const float *query, int64_t *idx, int batch, int dim, int ref_nb, int query_nb,
           int k, df_stream_t stream);

/* Exact-signature replacement of the reference's native symbol (lib/knn/src/knn_cuda_kernel.h:14-16): the call at
 * lib/knn/src/knn_pytorch.c:35 binds to it unchanged.  `dist_dev` is ignored (may be NULL); `stream` is a hipStream_t;
 * failures are reported through df_last_error() (the reference's wrapper polls the runtime's last error, knn_pytorch.c:41-45). */
void knn_device(float *ref_dev, int ref_width, float *query_dev, int query_width, int height, int k, float *dist_dev,
                long *ind_dev, df_stream_t stream);

/* Measurement helper: the shader clock (MHz) the device delivers under a full-chip vector-ALU load right now (a ~1 ms spin kernel
 * read against the constant 100 MHz counter).  Synchronises `stream`.  bench.py logs it next to the 1-NN roofline fractions. */
int df_shader_clock_mhz(double *mhz_out, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Network handles (replace the nn.Module objects of lib/network.py; the Python classes of
 * densefusion_amd/lib/network.py own one handle each and keep the reference's state_dict keys)
 *
 * A handle owns device copies of the parameters in kernel-friendly layouts (channels-last conv
 * weights, the r/t/c towers stacked, head layer 1 split into its per-point and global-feature parts).
 * Parameters are handed over one state-dict tensor at a time, in the REFERENCE's layout and under the
 * REFERENCE's key (e.g. "cnn.model.module.feats.layer3.0.conv1.weight", "feat.conv5.bias",
 * "conv4_r.weight"), so a checkpoint written by tools/train.py:172-176,211-217 loads unchanged.
 * Creation/loading may allocate and synchronise; forward calls never do.
 */
typedef struct df_net df_net;

df_net *df_posenet_create(int num_points, int num_obj);   /* PoseNet(num_points, num_obj), lib/network.py:70-93 */
df_net *df_refiner_create(int num_points, int num_obj);   /* PoseRefineNet(...),          lib/network.py:170-185 */
void df_net_destroy(df_net *net);
int df_net_num_params(const df_net *net);                  /* 77 tensors for PoseNet, 24 for the refiner */
int df_net_param_info(const df_net *net, int i, char *key_out, int key_cap, int64_t *shape4, int *ndim);
/* ptr: `numel` fp32 values in the reference layout (device or host pointer).  The copy, the re-layout and the derived copies
 * (Winograd-domain, tap-major) are ENQUEUED (null stream) without host synchronisation; the next forward call on this handle waits
 * for the batch once.  A DEVICE source must stay allocated until then (a host source is consumed before the call returns). */
int df_net_load_param(df_net *net, const char *key, const float *ptr, int64_t numel);

/* Batched PoseNet.forward (lib/network.py:95-132), eval mode (Dropout2d = identity).
 *   img    [B][3][H][W] fp32 NCHW (normalised crop, tools/eval_ycb.py:175-181)
 *   cloud  [B][N][3]    fp32        choose [B][N] int64 (row-major pixel index into the H x W crop)
 *   obj    [B]          int64
 *   out_r  [B][N][4] (un-normalised quaternion w,x,y,z)   out_t [B][N][3]   out_c [B][N] (sigmoid)
 *   emb    [B][32][N]  (log-softmax colour features at the chosen pixels; what the refiner consumes)
 * ws: caller-provided scratch of at least df_posenet_workspace_bytes(net, B, H, W) bytes. */
size_t df_posenet_workspace_bytes(const df_net *net, int B, int H, int W);
int df_posenet_forward(df_net *net, int B, int H, int W, const float *img, const float *cloud, const int64_t *choose,
                       const int64_t *obj, float *out_r, float *out_t, float *out_c, float *emb, void *ws,
                       size_t ws_bytes, df_stream_t stream);

/* The same forward for nb buckets of different crop sizes in one pass: bucket i holds B[i] objects of H[i] x W[i] (img[i]:
 * [B[i]][3][H[i]][W[i]]); cloud / choose / obj / outputs are concatenated in bucket order.  Bit-identical to per-bucket
 * df_posenet_forward calls.  (The frozen estimator of the refiner phase, tools/train.py:139-145, over a whole window.) */
size_t df_posenet_multi_workspace_bytes(const df_net *net, int nb, const int *B, const int *H, const int *W);
int df_posenet_forward_multi(df_net *net, int nb, const int *B, const int *H, const int *W, const float *const *img,
                             const float *cloud, const int64_t *choose, const int64_t *obj, float *out_r, float *out_t,
                             float *out_c, float *emb, void *ws, size_t ws_bytes, df_stream_t stream);

/* Batched PoseRefineNet.forward (lib/network.py:187-206): x [B][N][3], emb [B][32][N], obj [B]
 * -> out_r [B][4], out_t [B][3]. */
size_t df_refiner_workspace_bytes(const df_net *net, int B);
int df_refiner_forward(df_net *net, int B, const float *x, const float *emb, const int64_t *obj, float *out_r,
                       float *out_t, void *ws, size_t ws_bytes, df_stream_t stream);

/* The inner loop of tools/eval_ycb.py:192-229 / tools/eval_linemod.py:81-114 for B objects, with no
 * host round trip: PoseNet -> arg-max-confidence pose -> `iters` x (cloud into the pose frame ->
 * refiner -> compose).  pose_wo (optional) and pose: [B][7] fp64 = quaternion (w,x,y,z) then
 * translation, i.e. the rows the reference writes to its result .mat files (eval_ycb.py:203,231). */
size_t df_estimate_workspace_bytes(const df_net *posenet, const df_net *refiner, int B, int H, int W);
int df_estimate_poses(df_net *posenet, df_net *refiner, int B, int H, int W, const float *img, const float *cloud,
                      const int64_t *choose, const int64_t *obj, int iters, double *pose_wo, double *pose, void *ws,
                      size_t ws_bytes, df_stream_t stream);

/* The same for a window of detections of DIFFERENT crop sizes (the objects tools/eval_ycb.py:147-237 meets over a run of frames,
 * bucketed by their snapped box size, eval_ycb.py:54-90): nb buckets, bucket i = B[i] objects of H[i] x W[i] with images
 * img[i] = [B[i]][3][H[i]][W[i]] (host arrays of nb entries; the pointers are device pointers).  cloud / choose / obj / pose_wo /
 * pose hold the objects of all buckets concatenated in bucket order ([sum B][N][3], [sum B][N], [sum B], [sum B][7]).
 * Everything that does not depend on the crop geometry (1x1 convolutions, Winograd-domain products, low-resolution up-conv
 * products, the whole per-point part and every refine iteration) is ONE launch over all buckets; results are bit-identical to
 * per-bucket df_estimate_poses calls. */
size_t df_estimate_multi_workspace_bytes(const df_net *posenet, const df_net *refiner, int nb, const int *B, const int *H,
                                         const int *W);
int df_estimate_poses_multi(df_net *posenet, df_net *refiner, int nb, const int *B, const int *H, const int *W,
                            const float *const *img, const float *cloud, const int64_t *choose, const int64_t *obj, int iters,
                            double *pose_wo, double *pose, void *ws, size_t ws_bytes, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * ADD / ADD-S loss and metric, forward (replace lib/loss.py:13-70, lib/loss_refiner.py:12-62 and the
 * metric of tools/eval_linemod.py:118-130).  One object per call, like the reference (bs = 1).
 * `symmetric` != 0 selects the nearest-neighbour (ADD-S) branch -- what `idx[0].item() in sym_list`
 * (and `not refine` for the PoseNet loss) decides in the reference; the transform, the 1-NN and the
 * distance reduction are fused, nothing of size N*M is written to memory.
 *
 * df_loss_forward:  pred_r [N][4], pred_t [N][3], pred_c [N], target [M][3], model_points [M][3],
 *   points [N][3], w  ->  loss_out[1] = mean_n(dis_n c_n - w log c_n), dis_out[1] = dis at arg-max c,
 *   new_points [N][3], new_target [M][3] (re-centred by the arg-max pose); dis_scratch: N floats.
 * df_loss_refine_forward: pred_r [4], pred_t [3], points [N][3] -> dis_out[1], new_points, new_target.
 * df_add_metric: B objects; pose [B][7] fp64 (q wxyz, t), model_points/target [B][M][3] fp32,
 *   symmetric [B] int32 or NULL -> dis_out [B] fp64 (ADD, or ADD-S pred->nearest target). */
int df_loss_forward(const float *pred_r, const float *pred_t, const float *pred_c, const float *target,
                    const float *model_points, const float *points, int N, int M, float w, int symmetric,
                    float *loss_out, float *dis_out, float *new_points, float *new_target, float *dis_scratch,
                    int *sel_out /* optional [N][M]: matched target index per transformed point, for backward */,
                    df_stream_t stream);
/* df_loss_forward for B stacked frames in a handful of launches (each frame's arithmetic is df_loss_forward's): pred_r [B][N][4],
 * pred_t [B][N][3], pred_c [B][N], target / model_points [B][M][3], points [B][N][3]; symmetric: HOST int [B] (or NULL = none)
 * -> loss_out [B], dis_out [B], new_points [B][N][3], new_target [B][M][3]; dis_scratch: B*N floats; sel_out: optional [B][N][M]
 * (needed when any frame is symmetric and the matches are wanted; NULL: the symmetric frames do not keep them).  What the trainer's
 * window passes call (tools/train.py:139-153 runs lib/loss.py once per frame). */
int df_loss_forward_frames(int B, const int *symmetric, const float *pred_r, const float *pred_t, const float *pred_c,
                           const float *target, const float *model_points, const float *points, int N, int M, float w,
                           float *loss_out, float *dis_out, float *new_points, float *new_target, float *dis_scratch,
                           int *sel_out, df_stream_t stream);
int df_loss_refine_forward(const float *pred_r, const float *pred_t, const float *target, const float *model_points,
                           const float *points, int N, int M, int symmetric, float *dis_out, float *new_points,
                           float *new_target, int *sel_out /* optional [M] */, df_stream_t stream);
/* Backward of the two losses (what autograd derives from lib/loss.py:16-50 / lib/loss_refiner.py:17-48): gradients
 * w.r.t. the un-normalised quaternions, the translations and the confidences; the nearest-neighbour match (sel, from
 * the forward call; NULL = identity) is a constant.  dis = the per-point distances the forward left in dis_scratch.
 * g_loss / g_dis = upstream gradient of the scalar output (1 for loss.backward()). */
int df_loss_backward(const float *pred_r, const float *pred_t, const float *pred_c, const float *target,
                     const float *model_points, const float *points, const int *sel, const float *dis, int N, int M,
                     float w, float g_loss, float *d_pred_r, float *d_pred_t, float *d_pred_c, df_stream_t stream);
int df_loss_refine_backward(const float *pred_r, const float *pred_t, const float *target, const float *model_points,
                            const int *sel, int M, float g_dis, float *d_pred_r, float *d_pred_t, df_stream_t stream);
int df_add_metric(const double *pose, const float *model_points, const float *target, const int *symmetric, int B,
                  int M, double *dis_out, df_stream_t stream);
/* YCB-Video toolbox distances (replace_ycb_toolbox/evaluate_poses_keyframe.m:160-193), fp64 like MATLAB:
 * rt_est / rt_gt [B][12] = 3x4 row-major [R|t], pts [B][M][3] fp64 model points ->
 * add_out [B] = mean ||est_m - gt_m||,  adi_out [B] = mean_m min_j ||est_j - gt_m|| (KDTreeSearcher direction). */
int df_ycb_distances(const double *rt_est, const double *rt_gt, const double *pts, int B, int M, double *add_out,
                     double *adi_out, df_stream_t stream);

/* Element-wise / resampling layers of the training graph (channels-last fp32), forward and backward; `backward != 0`
 * selects the adjoint (in = upstream gradient, out = input gradient).  See csrc/trainops.hip for the reference lines. */
#define DF_ACT_BWD_PARTIALS 16384   /* floats of scratch the PReLU slope gradient needs (one partial per workgroup, added in order) */
int df_act_bwd(const float *dy, const float *y, float *dx, int64_t n, int act /*1 ReLU, 2 PReLU*/, const float *slope,
               float *dslope /* PReLU: += */, float *partials /* PReLU with dslope: DF_ACT_BWD_PARTIALS floats; else may be NULL */,
               df_stream_t stream);
int df_maxpool3s2_fwd(const float *x, float *y, int B, int H, int W, int C, int OH, int OW, df_stream_t stream);
/* MaxPool2d(2, 2, return_indices) / MaxUnpool2d(2, 2) of the SegNet encoder / decoder (vanilla_segmentation/segnet.py:78-116),
 * channels-last [B][H][W][C]; idx holds the winner's position 0..3 inside its 2x2 window (first maximum wins); unpool takes
 * the POOLED size H x W and writes [B][2H][2W][C]. */
int df_maxpool2x2_idx(const float *x, float *y, unsigned char *idx, int B, int H, int W, int C, df_stream_t stream);
int df_maxunpool2x2(const float *x, const unsigned char *idx, float *y, int B, int H, int W, int C, df_stream_t stream);

/* Training-mode layers of the SegNet (csrc/segtrain.hip), channels-last fp32, C a multiple of 4 (at most 1024).  Deterministic: no
 * atomics, fixed-order reductions whose partition depends on the shape only.
 *
 * BatchNorm2d (train) + ReLU over z [rows][C]: batch mean / biased variance (fp64 partials of z minus a sample of its channel), invstd =
 * 1/sqrt(var + eps), y = relu(((z - mean) invstd) gamma + beta); running_mean / running_var (unbiased variance) updated with `momentum`
 * as nn.BatchNorm2d does and *num_batches_tracked += 1 (either may be NULL: no update).  Outputs: var / invstd [C] and mean [2C], the
 * batch mean rounded to fp32 followed by its fp32 residual (hi + lo); the backward takes mean in that form.
 * df_bn_relu_bwd: the adjoint from dy, the saved z, mean, invstd (the ReLU mask recomputed from z): dgamma, dbeta [C] and
 * dz = gamma invstd (g - mean(g) - xhat mean(g xhat)).  pool_idx != NULL: the layer feeds a 2x2 max-pool and dy is the POOLED gradient
 * [B][H/2][W/2][C] with that pool's index (df_maxpool2x2_idx), rows = B H W; pool_idx == NULL: dy is [rows][C] (H, W unused).
 * Both take df_bn_workspace_bytes(rows, C) bytes of device scratch. */
size_t df_bn_workspace_bytes(int64_t rows, int C);
int df_bn_relu_fwd_train(const float *z, float *y, const float *gamma, const float *beta, float *running_mean, float *running_var,
                         int64_t *num_batches_tracked, float *mean, float *var, float *invstd, int64_t rows, int C, float momentum,
                         float eps, void *ws, size_t ws_bytes, df_stream_t stream);
int df_bn_relu_bwd(const float *dy, const unsigned char *pool_idx, int H, int W, const float *z, const float *mean, const float *invstd,
                   const float *gamma, const float *beta, float *dz, float *dgamma, float *dbeta, int64_t rows, int C, void *ws,
                   size_t ws_bytes, df_stream_t stream);
/* Adjoint of df_maxunpool2x2: dx [B][H][W][C] (the POOLED size) gathers dy [B][2H][2W][C] at the position idx names. */
int df_maxunpool2x2_bwd(const float *dy, const unsigned char *idx, float *dx, int B, int H, int W, int C, df_stream_t stream);
/* nn.CrossEntropyLoss() (mean over rows) of logits [rows][ld] whose first `classes` channels are the classes, target int64 [rows]:
 * *loss (device) and dlogits [rows][ld] = (softmax - onehot) / rows, zero in the channels >= classes, in one pass plus an ordered
 * finish.  A label outside [0, classes) sets *bad_label (device int, cleared by the call) and its row gets zero gradient.
 * ws: df_cross_entropy_workspace_bytes(rows) bytes. */
size_t df_cross_entropy_workspace_bytes(int64_t rows);
int df_cross_entropy_nhwc(const float *logits, const int64_t *target, float *dlogits, int64_t rows, int ld, int classes, float *loss,
                          int *bad_label, void *ws, size_t ws_bytes, df_stream_t stream);
int df_maxpool3s2_bwd(const float *x, const float *dy, float *dx, int B, int H, int W, int C, int OH, int OW, df_stream_t stream);
int df_adaptive_avgpool(const float *in, float *out, int B, int H, int W, int C, int s, int backward, df_stream_t stream);
int df_bilinear(const float *in, float *out, int B, int H, int W, int C, int OH, int OW, int align_corners, int backward,
                df_stream_t stream);
int df_logsoftmax(const float *x_or_dy, const float *y, float *out, int64_t rows, int C, int backward, df_stream_t stream);
int df_dropout2d_mask(float *scale, int64_t n /* B*C */, unsigned seed, float p, df_stream_t stream);
int df_channel_scale(const float *x, const float *scale /*[B][C]*/, float *y, int B, int64_t hw, int C, df_stream_t stream);
int df_gather_rows(const float *in, const int64_t *idx, float *out, int64_t n, int C, int64_t rows, int backward, df_stream_t stream);
int df_colmean(const float *in, float *out, int64_t rows, int C, int backward, df_stream_t stream);
int df_sigmoid(const float *x_or_dy, const float *y, float *out, int64_t n, int backward, df_stream_t stream);

/* Adam update of a flat fp32 parameter buffer (the optimizer of tools/train.py:99 with its default betas / eps):
 *   m = m + (1-b1)(g' - m);  v = b2 v + (1-b2) g'^2;  p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps),  g' = grad_scale * g
 * grad_scale carries the 1/(ranks x accumulated samples) of the data-parallel gradient average. */
int df_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr, float beta1,
                 float beta2, float eps, int step, float grad_scale, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Input preparation on the device (the numpy block of tools/eval_ycb.py:147-181, per detected object):
 * mask = (depth != 0) & (label == itemid) inside the snapped box; choose = num_points mask pixels (random
 * subset / wrap-padding); back-projected cloud; ImageNet-normalised CHW crop.  B objects of one crop size
 * (H x W) per call.
 *   rgb [F][IH][IW][3] u8, depth [F][IH][IW] u16, label [F][IH][IW] i32 (F frames resident on the device)
 *   obj_desc [B][8] int32 = {frame, itemid, rmin, rmax, cmin, cmax, seed, given}; rmax-rmin == H, cmax-cmin == W;
 *   given != 0: the object's row of choose_out is an INPUT -- the caller's chosen pixel indices (how a test hands over the very subset
 *   the reference's np.random.shuffle drew); sampling is skipped, cloud / img are formed from those indices
 *   scratch: B*H*W int32.  Outputs: img_out [B][3][H][W], cloud_out [B][N][3], choose_out [B][N] int64,
 *   count_out [B] = number of mask pixels (0 = detector lost the object, eval_ycb.py:234-237).
 * Subset rule when count > N (replaces np.random.shuffle, whose stream a GPU cannot share): keep the N mask
 * pixels with the smallest mix32(seed, flat index) keys, in index order -- a uniformly random ordered subset.
 * cloud = ((col - cx) * z / fx, (row - cy) * z / fy, z) / cloud_div with z = depth / cam_scale: YCB passes (10000, 1)
 * (eval_ycb.py:165-173), LineMOD (1, 1000) and itemid 255 (datasets/linemod/dataset.py:106-112,152-157). */
int df_preprocess_objects(const unsigned char *rgb, const unsigned short *depth, const int *label, int num_frames, int IH,
                          int IW, const int *obj_desc, int B, int H, int W, int num_points, float cam_cx, float cam_cy,
                          float cam_fx, float cam_fy, float cam_scale, float cloud_div, int *scratch, float *img_out, float *cloud_out,
                          int64_t *choose_out, int *count_out, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Input preparation for the customCAD dataset (Unity renders: datasets/customCAD/dataset.py:109-166,205 and
 * project_unity_depth.py:42-51 of the reference).  Same conventions as df_preprocess_objects: no allocation, no synchronisation,
 * the caller's stream.
 *
 * df_cad_frame_stats: depth, label [F][IH][IW] u16 -> stats [F][6] int32 = {depth_max, n_label, rmin, rmax, cmin, cmax}:
 *   the frame's largest depth value (np.max(depth), :120,132), the number of pixels with label == label_value and the INCLUSIVE
 *   smallest / largest row and column of those pixels (get_bbox, :247-249; the loader slices [rmin:rmax, cmin:cmax], leaving
 *   the last row and column out).  A frame without the label gets n_label = 0 and a zero box.  The call initialises stats on the
 *   stream; integer reductions only, and a frame's row does not depend on the other frames of the call.  F <= 65535, IH*IW <= 2^30.
 * df_preprocess_objects_cad: B objects of one crop size (H x W) per call.
 *   rgb [F][IH][IW][3] u8, depth and label [F][IH][IW] u16;
 *   obj_desc [B][8] int32 = {frame, label_value, rmin, rmax, cmin, cmax, seed, given} as for df_preprocess_objects (an object
 *   whose box leaves its frame comes back with count 0); frame_stats [F][6] (device; only depth_max is read, so the two calls
 *   need no host round trip between them); ray_map [IH][IW][3] double (device): the view ray through every pixel, scaled to
 *   z = 1; p22, p23: the projection matrix' [2][2] and [2][3]; add_t [B][3] double (device) or NULL; scratch: B*H*W int32.
 *   mask = (label == label_value) & (depth != depth_max[frame]) (:120-124); choose / count_out: the contract of df_preprocess_objects;
 *   cloud (all in fp64, one rounding per operation, no fused multiply-add -- bit-equal to numpy):
 *     z = -p23 / (p22 + (1 - d / 65534)); point = (float)(ray_map[r][c][k] * z); with add_t: point = (float)((double)point + add_t[k]);
 *     cloud = point / cloud_div in fp32 (the loader passes 10000);
 *   img: the crop with (130, 130, 130) where depth == depth_max (:97,132), then ((float)px - mean) / std into CHW. */
int df_cad_frame_stats(const unsigned short *depth, const unsigned short *label, int num_frames, int IH, int IW, int label_value,
                       int *stats, df_stream_t stream);
int df_preprocess_objects_cad(const unsigned char *rgb, const unsigned short *depth, const unsigned short *label, int num_frames,
                              int IH, int IW, const int *obj_desc, const int *frame_stats, const double *ray_map, double p22,
                              double p23, const double *add_t, int B, int H, int W, int num_points, float cloud_div, int *scratch,
                              float *img_out, float *cloud_out, int64_t *choose_out, int *count_out, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The rest of a customCAD item for frames that never reach the host (rendered frames: datasets/customCAD/online.py): the count and
 * live test of PoseDataset.batch and the model subset and targets of PoseDataset._targets.  Plain launches on the caller's stream: no
 * allocation, no synchronisation; integer reductions and integer atomics only, so two identical calls give identical bytes, and a
 * row (frame or item) does not depend on the other rows of its call.  DF_ERR_ARG, before anything is launched or written: a null
 * pointer, bad sizes, a short or misaligned scratch.
 *
 * df_cad_item_table: depth, label [F][IH][IW] u16 -> table [F][8] int32 (the call initialises it on the stream); F <= 65535,
 *   IH*IW <= 2^30, label_value 0..65535, min_side >= 0.  Two passes in stream order, the host never sees the box in between:
 *   1. Entries 0..5 = {depth_max, n_label, rmin, rmax, cmin, cmax}: exactly the row of df_cad_frame_stats (the same kernels).
 *   2. Entry 6 = count: the pixels of the half-open crop [rmin:rmax, cmin:cmax] with label == label_value and depth != depth_max
 *      (the loader's mask inside its crop, :120-124,137-138; the box's last row and column are left out); 0 when n_label == 0.
 *   3. Entry 7 = live: n_label > 0 && rmax - rmin >= min_side && cmax - cmin >= min_side && count > 0, as 0 / 1 (the loader passes
 *      min_side 8, the network's smallest crop).
 * df_cad_targets: B items; model [P][3] double (DEVICE: the loader's pt[obj], file units), model_scale (the loader's 10),
 *   pose [B][12] double (DEVICE, row-major [R|T]: the caller puts R = target_r @ Y_180 and T = target_t, with noise
 *   T = target_t + add_t * 10000, computed on the host), seed [B] u32 (DEVICE), 1 <= M <= P <= 2^24, B 1..65535, cloud_div > 0 (the
 *   loader's 10000); scratch: df_cad_targets_scratch_bytes(B, P, M) bytes (B rows of M int64 and of P + 1 int32; 0 for sizes the call
 *   refuses), 8-byte aligned.  Outputs model_points_out, target_out [B][M][3] float.  Per item b:
 *   1. Subset: model point i < P gets the key mix32(seed[b], i) (the RNG contract of df_preprocess_objects, csrc/choose_core.h); the M
 *      points with the smallest keys are kept, in increasing index order (the same device routine with an all-true mask).  mix32 is a
 *      bijection in i for a fixed seed: there are no ties.  P == M keeps every point.  A uniformly random subset with the survivors in
 *      index order: what random.sample plus np.delete give (:169-171), without their stream.
 *   2. Per kept point i, all in fp64, one rounding per operation, no fused multiply-add, in exactly this order:
 *      m = model[i] * model_scale;  model_points = (float)m / cloud_div, divided in fp32;
 *      X_j = ((R[j][0]*m_x + R[j][1]*m_y) + R[j][2]*m_z) + T_j;  target = (float)X_j / cloud_div, divided in fp32. */
int df_cad_item_table(const unsigned short *depth, const unsigned short *label, int num_frames, int IH, int IW, int label_value,
                      int min_side, int *table, df_stream_t stream);
size_t df_cad_targets_scratch_bytes(int B, int P, int M);
int df_cad_targets(const double *model, int P, double model_scale, const double *pose, const unsigned *seed, int B, int M,
                   float cloud_div, void *scratch, size_t scratch_bytes, float *model_points_out, float *target_out, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Point-cloud renderer for customCAD training sets: F views of a coloured CAD cloud as the frames the customCAD loader reads (8-bit
 * colour, Unity's 16-bit depth, 16-bit mask) -- the job of datasets/customCAD/cad_to_dataset.py:137-243 and mask_generator.py:20-28 of
 * the reference without open3d, OpenCV or Unity.  No allocation, no synchronisation, the caller's stream; integer atomics only, so the
 * outputs are bit-reproducible; a frame's outputs do not depend on the other frames of the call.
 *
 * df_cad_render_scratch_bytes: F*IH*IW 64-bit keys; 0 for sizes the call refuses (F 1..65535, IH*IW 1..2^30).
 * df_cad_render:
 *   DEVICE: points [P][3] float (model file units), normals [P][3] float or NULL (no facing test), colors [P][3] u8,
 *   pose [F][12] double, row-major [R|t] into camera space (x right, y up, the camera looks along -z), the outputs, scratch (8-byte
 *   aligned).  HOST, read during the call: proj, 16 doubles row-major, and hole_idx / hole_r [F][K] (NULL when K == 0, K <= 128; they
 *   reach the kernel as launch arguments, 128 records a launch).
 *   DF_ERR_ARG, before anything is launched or written: a null pointer, bad sizes, splat outside 0..3, mask_mode outside 0..1, a
 *   short scratch, a hole index >= P, and a proj whose row 2 is not (0, 0, p22, p23) or whose row 3 is not (0, 0, -1, 0) -- the
 *   loader's inverse (project_unity_depth.py:42-51) assumes that form.
 *   Per frame f and point i, all in fp64, one rounding per operation (no fused multiply-add), in exactly this order:
 *   1. m = (double)points[i].  The point is removed when for some k with h = hole_idx[f][k] >= 0 and c = (double)points[h],
 *      r = hole_r[f][k]:  ((mx-cx)^2 + (my-cy)^2) + (mz-cz)^2 <= r*r  (radius 0 removes the centre and its exact duplicates);
 *      the job of augment_pointcloud, :137-164.
 *   2. s = m * model_scale;  X_j = ((R[j][0]*s_x + R[j][1]*s_y) + R[j][2]*s_z) + t[j].
 *   3. With normals: n'_j = (R[j][0]*n_x + R[j][1]*n_y) + R[j][2]*n_z; the point is kept only when
 *      ((n'_x*(-X_x) + n'_y*(-X_y)) + n'_z*(-X_z)) > 0: the point's own view ray (the reference, :175-176, tests against the direction
 *      to the cloud's centroid, which would need an order-dependent floating-point reduction).
 *   4. c_j = ((P[j][0]*X_x + P[j][1]*X_y) + P[j][2]*X_z) + P[j][3] for j = 0, 1, 3; dropped unless c_3 > 0;
 *      ndc_x = c_0 / c_3, ndc_y = c_1 / c_3.
 *   5. code = rint(65534 * ((1 + p22) + p23 / X_z)), ties to even; dropped unless 0 <= code <= 65534.  The exact inverse of the
 *      loader's z = -p23 / (p22 + (1 - d / 65534)); nearer points get smaller codes.
 *   6. col = floor(((ndc_x + 1) * IW) * 0.5 + 0.5), row = floor(((1 - ndc_y) * IH) * 0.5 + 0.5): the nearest node of the loader's
 *      ray grid, whose ray for pixel (r, c) passes through ndc (-1 + 2c/IW, 1 - 2r/IH).  The footprint is the (2*splat+1)^2 square
 *      around it; each of its pixels is tested against the frame on its own.
 *   7. Every footprint pixel takes atomicMin of key = (uint64)code << 32 | i: the nearest point wins, equal codes go to the lowest
 *      index, and depth and colour share the winner (the reference's assignment at :223-236 gives the colour to the farthest point).
 *   Resolve, per pixel: covered -> depth = code, rgb = colors[winner]; uncovered -> depth = 65535 (strictly above every code: the
 *   loader's `depth != np.max(depth)` and its grey fill see a horizon) and rgb = (130, 130, 130).
 *   stats [F][6] int32 = {covered pixels, points that reached the z-buffer (each once), rmin, rmax, cmin, cmax}: the INCLUSIVE box of
 *   the covered pixels; all six zero when nothing is covered.
 *   mask: mode 0 (box) 65535 on rows rmin..rmax-1 and columns cmin..cmax-1 -- the half-open slice of the inclusive box that
 *   mask_generator.py:21-28 writes, mirrored as it is; mode 1 (pixels) 65535 on the covered pixels; 0 elsewhere. */
size_t df_cad_render_scratch_bytes(int F, int IH, int IW);
int df_cad_render(const float *points, const float *normals, const unsigned char *colors, int P, const double *pose, double model_scale,
                  const int *hole_idx, const double *hole_r, int K, const double *proj, int F, int IH, int IW, int splat, int mask_mode,
                  unsigned char *rgb_out, unsigned short *depth_out, unsigned short *mask_out, int *stats_out, void *scratch,
                  size_t scratch_bytes, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Triangle rasteriser for customCAD training sets: F views of a coloured CAD mesh as the frames df_cad_render writes from a cloud, drawn
 * from the triangles themselves (the reference renders meshes in Unity; its own attempt without Unity, cad_to_dataset.py, starts from
 * read_triangle_mesh).  Watertight, no splat parameter, the depth exact on each facet up to the rounding of the 16-bit code.  The rules of
 * df_cad_render carry over: no allocation, no synchronisation, the caller's stream; integer atomics only, so the outputs are
 * bit-reproducible; a frame's outputs do not depend on the other frames of the call.
 *
 * df_cad_render_mesh_scratch_bytes: F*IH*IW 64-bit keys (V1..V5 below are recomputed per triangle corner, so nothing is kept per
 *   vertex); 0 for sizes the call refuses (F, IH, IW as for df_cad_render; V, T 1..2^31-1).
 * df_cad_render_mesh:
 *   DEVICE: vertices [V][3] float (model file units), colors [V][3] u8, triangles [T][3] int (vertex indices), pose [F][12] double as for
 *   df_cad_render, the outputs, scratch (8-byte aligned).  HOST, read during the call: proj and hole_idx / hole_r [F][K], as for
 *   df_cad_render (K <= 128, 128 records a launch); hole indices name vertices.
 *   DF_ERR_ARG, before anything is launched or written: a null pointer, bad sizes, cull or mask_mode outside 0..1, a short or
 *   misaligned scratch, a hole index >= V, and a proj that is not of df_cad_render's form.
 *   All in fp64, one rounding per operation (no fused multiply-add), in exactly this order.
 *   Per frame f and vertex v:
 *   V1. m = (double)vertices[v].  The vertex is removed by a hole by step 1 of df_cad_render (the centres are vertices).
 *   V2. s = m * model_scale;  X_j = ((R[j][0]*s_x + R[j][1]*s_y) + R[j][2]*s_z) + t[j].
 *   V3. c_0, c_1, c_3 as in step 4 of df_cad_render.  The vertex is BEHIND unless c_3 > 0.  ndc_x = c_0 / c_3, ndc_y = c_1 / c_3.
 *   V4. sx = ((ndc_x + 1) * IW) * 0.5, sy = ((1 - ndc_y) * IH) * 0.5.  Pixel (r, q) is the node sy = r, sx = q of the loader's ray
 *       grid: the grid of step 6 of df_cad_render, whose col is floor(sx + 0.5).
 *   V5. d = (1 + p22) + p23 / X_z: the depth code before scaling and rounding; affine in 1/z, hence exactly linear over the screen on
 *       a planar triangle.
 *   Per triangle t = (i0, i1, i2):
 *   T1. Dropped when an index is outside 0..V-1 (nothing is read through it), two indices are equal, a vertex is removed by a hole, or
 *       a vertex is behind.  THERE IS NO CLIPPING: a triangle that crosses the camera plane is dropped whole.
 *   T2. The edge function of the ordered pair (a, b) at a point p, with lo = min(a, b), hi = max(a, b):
 *       e = (sx_hi - sx_lo)*(p_y - sy_lo) - (sy_hi - sy_lo)*(p_x - sx_lo);  E(a,b;p) = e when a < b, else -e.  The two triangles that
 *       share an edge see exactly opposite values, so a node is never lost between them: this canonical order makes the raster watertight.
 *   T3. A = E(i0,i1; (sx_i2, sy_i2)).  Dropped when A == 0 or A is not finite.  Front-facing when A < 0 (counter-clockwise as the camera
 *       sees it, y up); cull == 1 drops the others.
 *   T4. Columns from max(ceil(min sx), 0) to min(floor(max sx), IW-1), rows alike with sy and IH; the bounds are compared as doubles
 *       before any conversion to integer.  An empty range drops the triangle.
 *   T5. At node (r, q): w0 = E(i1,i2;(q,r)), w1 = E(i2,i0;(q,r)), w2 = E(i0,i1;(q,r)), each negated when A < 0.  The node is covered
 *       when w0 >= 0, w1 >= 0, w2 >= 0 and W = (w0 + w1) + w2 > 0.
 *   T6. code = rint(65534 * (((w0*d_i0 + w1*d_i1) + w2*d_i2) / W)), ties to even; the node is dropped unless 0 <= code <= 65534 (a
 *       triangle that reaches past a code limit is cut per node).
 *   T7. atomicMin of key = (uint64)code << 32 | t: the nearest surface wins, equal codes go to the lowest triangle index.
 *   Resolve, per pixel: uncovered -> depth 65535 and rgb (130, 130, 130) as in df_cad_render.  Covered -> depth = code; the winner's
 *   w_k are recomputed by T5 (the same operations, hence the same bits); u_k = w_k / c_3(i_k) (perspective-correct);
 *   U = (u0 + u1) + u2; each channel = rint(((u0*C_i0 + u1*C_i1) + u2*C_i2) / U) clamped to 0..255 (a NaN gives 0).
 *   stats [F][6] and the two mask modes are those of df_cad_render, except stats[f][1]: the number of triangles that took at least one
 *   key test in T7. */
size_t df_cad_render_mesh_scratch_bytes(int F, int IH, int IW, int V, int T);
int df_cad_render_mesh(const float *vertices, const unsigned char *colors, int V, const int *triangles, int T, const double *pose,
                       double model_scale, const int *hole_idx, const double *hole_r, int K, const double *proj, int F, int IH, int IW,
                       int cull, int mask_mode, unsigned char *rgb_out, unsigned short *depth_out, unsigned short *mask_out,
                       int *stats_out, void *scratch, size_t scratch_bytes, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Diffuse lighting for the two triangle renderers: df_cad_render_mesh_lit and df_cad_render_scene_lit (declared after
 * df_cad_render_scene) take the parameters of df_cad_render_mesh / df_cad_render_scene with three more directly before rgb_out, and
 * write the same frames with the colour of every covered pixel multiplied by ambient + diffuse * max(N.L, 0) times a light colour.
 * Only the colour of covered pixels changes: depth, label, stats, masks, the horizon colour and every rule of V1..V5, T1..T7 and S1..S3
 * are those of the unlit calls, whose scratch-size functions these calls share (the scratch is still the keys only).  The rules carry
 * over: no allocation, no synchronisation, the caller's stream, bit-reproducible, a frame's outputs independent of the other frames.
 * The point renderer df_cad_render has no lit form.
 *
 *   DEVICE: normals, float, model space, expected to be of unit length (not checked): normal_mode 0 = one per triangle, [T][3], indexed
 *   by the call's triangle index (the GLOBAL index in a scene) -- flat shading; normal_mode 1 = one per vertex, [V][3] -- smooth shading.
 *   light [F][8] double = {Lx, Ly, Lz, ambient, diffuse, cr, cg, cb} per frame (a scene has one light per frame for all its objects):
 *   L is the direction from the surface towards the light in camera space (x right, y up, the camera looks along -z: (0, 0, 1) is a
 *   head-light), expected to be of unit length and used as given.
 *   light == NULL is the unlit call exactly: normals may then be NULL and normal_mode is ignored.
 *   DF_ERR_ARG, before anything is launched or written: light != NULL with normals == NULL or with normal_mode outside 0..1, and
 *   everything the unlit call refuses.
 *   Per covered pixel, after the resolve has recomputed the winner's w_k, u_k = w_k / c_3(i_k) and U = (u0 + u1) + u2; all in fp64, one
 *   rounding per operation (no fused multiply-add), in exactly this order; t = (i0, i1, i2) is the winner, R the rotation of pose[f]
 *   (mesh) or of pose[f][o], o the winner's owner (scene):
 *   L1. Mode 0: n = (double)normals[t].  Mode 1: n_k = (double)normals[i_k] for the three corners.
 *   L2. Rotated as step 3 of df_cad_render rotates: n'_j = (R[j][0]*n_x + R[j][1]*n_y) + R[j][2]*n_z.  Mode 0: N = n'.  Mode 1: each
 *       corner's normal is rotated first, then N_j = ((u0*n'0_j + u1*n'1_j) + u2*n'2_j) / U: the perspective-correct mix.  THE MIX IS NOT
 *       RE-NORMALISED (inside a triangle |N| falls short of 1 by at most 1 - cos(half the largest angle between two of its corner
 *       normals)), so there is no square root anywhere in the contract.  R is taken to be a rotation; this is not checked.
 *   L3. When the winner faces away (A > 0 in T3, possible only with cull == 0): N = -N.  A back face is lit as the side the camera sees.
 *   L4. c = (N_x*L_x + N_y*L_y) + N_z*L_z;  c = c > 0 ? c : 0 (a NaN gives 0).
 *   L5. s = ambient + diffuse * c.
 *   L6. Per channel, with a = ((u0*C_i0 + u1*C_i1) + u2*C_i2) / U, the value the unlit resolve rounds:
 *       channel = rint(a * (s * c_ch)) clamped to 0..255 (a NaN gives 0).  The only rounding to 8 bits is this last one.
 *   Hence the record {., ., ., 1, 0, 1, 1, 1} multiplies by exactly 1.0 and gives the unlit bytes, and a light that saturates clamps
 *   at 255. */
int df_cad_render_mesh_lit(const float *vertices, const unsigned char *colors, int V, const int *triangles, int T, const double *pose,
                           double model_scale, const int *hole_idx, const double *hole_r, int K, const double *proj, int F, int IH, int IW,
                           int cull, int mask_mode, const float *normals, int normal_mode, const double *light, unsigned char *rgb_out,
                           unsigned short *depth_out, unsigned short *mask_out, int *stats_out, void *scratch, size_t scratch_bytes,
                           df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-object customCAD scenes with occlusion: F frames of O meshes, each with its own pose per frame, drawn into one z-buffer, so that
 * a target can be covered by another object and a frame can hold distractors (the Unity scenes the reference was fed; the YCB path has
 * df_compose_frame for it).  The rules of df_cad_render_mesh carry over: no allocation, no synchronisation, the caller's stream; integer
 * atomics only, so the outputs are bit-reproducible; a frame's outputs do not depend on the other frames of the call.  There are no holes
 * in this call: occluders play that part.
 *
 * df_cad_render_scene_scratch_bytes: F*IH*IW 64-bit keys; 0 for sizes the call refuses (F, IH, IW, V, T as for df_cad_render_mesh;
 *   O 1..DF_CAD_SCENE_MAX_OBJECTS).
 * df_cad_render_scene:
 *   DEVICE: vertices [V][3] float, colors [V][3] u8 and triangles [T][3] int as for df_cad_render_mesh: one shared vertex array and one
 *   shared triangle array, the indices global; pose [F][O][12] double, row-major [R|t] of object o in frame f; present [F][O] u8
 *   (0 = object o is not in frame f) or NULL = all present; the outputs; scratch (8-byte aligned).
 *   HOST, read during the call: proj as for df_cad_render; tri_begin [O+1] int: object o owns the triangles tri_begin[o] ..
 *   tri_begin[o+1]-1 (an empty range is allowed); model_scale [O] double.  Both tables reach the kernels as launch arguments.
 *   DF_ERR_ARG, before anything is launched or written: a null pointer (present excepted), bad sizes, O outside 1..64, cull outside 0..1,
 *   a short or misaligned scratch, a proj that is not of df_cad_render's form, tri_begin[0] != 0, tri_begin[o+1] < tri_begin[o] for
 *   some o, tri_begin[O] != T.
 *   All in fp64, one rounding per operation (no fused multiply-add), in exactly this order.
 *   Per frame f and triangle t = (i0, i1, i2), with o the object that owns t (tri_begin[o] <= t < tri_begin[o+1]):
 *   S1. Dropped when present != NULL and present[f][o] == 0.
 *   S2. Steps V2..V5 of df_cad_render_mesh for its three vertices, with R, t = pose[f][o] and model_scale[o] (no vertex is removed by a
 *       hole), then T1..T6 verbatim: indices outside 0..V-1 or equal, a vertex behind (NO CLIPPING), the edge functions evaluated from
 *       the lower GLOBAL vertex index to the higher, A == 0 or not finite, cull, the node range, coverage, the code and its limits.
 *   S3. T7 with the GLOBAL triangle index: atomicMin of key = (uint64)code << 32 | t.  The nearest surface of any object wins; equal
 *       codes go to the lowest global triangle index, hence to the object listed first.
 *   Resolve, per pixel: uncovered -> depth 65535, rgb (130, 130, 130), label 0.  Covered -> the owner o of the winning triangle is found
 *   in tri_begin; depth = code and rgb exactly as in the resolve of df_cad_render_mesh with pose[f][o] and model_scale[o];
 *   label = o + 1.
 *   stats [F][O][6] int32: stats[f][o] = {pixels o won, triangles of o that took at least one key test in S3, rmin, rmax, cmin, cmax}:
 *   the INCLUSIVE box of the pixels o won, four zeros when it won none.  Entry 1 stays as counted then: an object hidden behind others
 *   reads {0, n > 0, 0, 0, 0, 0}, an absent one six zeros.
 * df_cad_scene_mask: the loader's mask of pair n = (f, o) = pairs[n], pairs DEVICE [N][2] int, N 1..65535; label and stats are the
 *   outputs of df_cad_render_scene for F, O, IH, IW.  mask_out [N][IH][IW]:
 *   mode 0 (box): 65535 on rows rmin..rmax-1 and columns cmin..cmax-1 of stats[f][o] -- the half-open slice of the inclusive box that
 *   mask_generator.py:21-28 writes, mirrored as it is (pixels of an occluder inside the box are marked: the reference's own rule);
 *   mode 1 (pixels): 65535 where label[f] == o + 1, the pixels the object actually won; 0 elsewhere.  A pair outside 0..F-1 x 0..O-1
 *   gives an all-zero mask and nothing is read through it.  DF_ERR_ARG: a null pointer, bad sizes, O outside 1..64, mask_mode outside
 *   0..1.  No allocation, no synchronisation, the caller's stream. */
#define DF_CAD_SCENE_MAX_OBJECTS 64
size_t df_cad_render_scene_scratch_bytes(int F, int IH, int IW, int V, int T, int O);
int df_cad_render_scene(const float *vertices, const unsigned char *colors, int V, const int *triangles, int T, const int *tri_begin,
                        const double *model_scale, int O, const double *pose, const unsigned char *present, const double *proj, int F,
                        int IH, int IW, int cull, unsigned char *rgb_out, unsigned short *depth_out, unsigned short *label_out,
                        int *stats_out, void *scratch, size_t scratch_bytes, df_stream_t stream);
/* the contract of the lit call is the comment of df_cad_render_mesh_lit */
int df_cad_render_scene_lit(const float *vertices, const unsigned char *colors, int V, const int *triangles, int T, const int *tri_begin,
                            const double *model_scale, int O, const double *pose, const unsigned char *present, const double *proj, int F,
                            int IH, int IW, int cull, const float *normals, int normal_mode, const double *light, unsigned char *rgb_out,
                            unsigned short *depth_out, unsigned short *label_out, int *stats_out, void *scratch, size_t scratch_bytes,
                            df_stream_t stream);
int df_cad_scene_mask(const unsigned short *label, const int *stats, int F, int O, int IH, int IW, const int *pairs, int N, int mask_mode,
                      unsigned short *mask_out, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * A depth-sensor model over rendered customCAD depth frames, applied after any of the render calls above.  It changes depth only.  The
 * Unity code rint(65534 ((1 + p22) + p23 / z)) is affine in 1 / z, a disparity; a structured-light or stereo sensor's noise is constant
 * in disparity (sigma_z ~ z^2), hence of constant sigma in code units, and the whole model is integer arithmetic on the codes.  No
 * allocation, no copy, no synchronisation, the caller's stream; integer atomics only (the counts), so the outputs are bit-reproducible.
 *
 * df_cad_depth_sensor: depth_in [F][IH][IW] u16 (the clean render), depth_out the same shape, stats [F][4] int32 -- all DEVICE; the two
 *   depth ranges must not overlap (the edge test reads the clean neighbours).  Everything else travels as launch arguments.  The call
 *   zeroes stats itself.  stats[f] = {edge pixels, pixels dropped at random, pixels dropped at an edge, kept pixels whose code changed}.
 *   DF_ERR_ARG, before anything is launched or written: a null pointer; overlapping depth ranges; F, IH, IW as for df_cad_render;
 *   noise_mul < 0; edge_radius outside 0..4; edge_step outside 0..65535; edge_drop24 or drop24 outside 0..2^24; quant outside 1..4096.
 *   mix32 is the function of df_preprocess_objects' RNG contract (csrc/choose_core.h); C0 = 0x243F6A88, C1 = 0x85A308D3,
 *   C2 = 0x13198A2E, C3 = 0x03707344.  For pixel p (flat index within its frame) of frame f with clean code c = depth_in[f][p]:
 *   D0. Frame seed: s = mix32(seed, (first_frame + f) mod 2^32).  Frame f of a call with first_frame = a is frame 0 of a call with
 *       first_frame = a + f: a frame depends on nothing else in its call.
 *   D1. Horizon: c == 65535 -> out = 65535, nothing is counted.
 *   D2. Edge: with R = edge_radius > 0, p is an edge pixel when at least one pixel of the (2R+1)^2 window around it is a horizon pixel or
 *       has |c_n - c| > edge_step.  Window pixels outside the frame are ignored (the window never reaches another frame's memory).  The
 *       test is on the CLEAN input.  stats[f][0] += 1 for an edge pixel, whatever happens to it next.
 *   D3. Random drop-out: (mix32(s ^ C3, p) >> 8) < drop24 -> out = 65535, stats[f][1] += 1.
 *   D4. Edge drop-out: otherwise, an edge pixel with (mix32(s ^ C2, p) >> 8) < edge_drop24 -> out = 65535, stats[f][2] += 1.
 *   D5. Disparity noise: otherwise h0 = mix32(s ^ C0, p), h1 = mix32(s ^ C1, p),
 *       S = (h0 & 0xFFFF) + (h0 >> 16) + (h1 & 0xFFFF) + (h1 >> 16) - 131070: a centred sum of four 16-bit uniforms, variance 1431655765;
 *       n = floor((noise_mul * S + 2^31) / 2^32) in 64-bit signed arithmetic; c1 = clamp(c + n, 0, 65534).
 *   D6. Quantisation: c2 = min(65534, ((c1 + quant / 2) / quant) * quant), integer divisions (quant == 1 leaves c1); out = c2,
 *       stats[f][3] += (c2 != c).
 *   A kept pixel is never 65535: the model invents horizon by D3 and D4 only.  noise_mul = rint(sigma * 2^32 / sqrt(1431655765)) gives
 *   noise of standard deviation sigma codes (plus the 1/12 of the rounding). */
int df_cad_depth_sensor(const unsigned short *depth_in, unsigned short *depth_out, int F, int IH, int IW, unsigned seed,
                        unsigned first_frame, int noise_mul, int edge_radius, int edge_step, int edge_drop24, int drop24, int quant,
                        int *stats, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Training-time pixel augmentation on whole uint8 frames, bit-identical to the host path (densefusion_amd/datasets/augment.py over PIL;
 * datasets/ycb/dataset.py).  Same conventions as df_preprocess_objects: no allocation, no synchronisation, the caller's stream.
 *
 * df_color_jitter: src [F][H][W][3] u8 -> dst, same layout (dst == src allowed, no other overlap); H*W <= 2^24, F <= 65535.
 *   plan [F][8] float (device): {brightness alpha, contrast alpha, saturation alpha, hue shift 0..255, op0, op1, op2, op3} -- the
 *   operations in application order, 0 brightness, 1 contrast, 2 saturation, 3 hue, anything else none (augment.plan_row).
 *   scratch [F] u32 (device): per-frame sums of L, zeroed on the stream by the call.
 *   brightness / contrast / saturation = trunc(clamp(d + a*(x - d))) in fp32 without fused multiply-add, d = 0 / the frame's rounded mean
 *   L at that point of the order / the pixel's L, L = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16; hue = PIL's RGB -> HSV, H += shift
 *   (mod 256), HSV -> RGB.  Deterministic: the only atomics add integers.
 * df_compose_frame: rgb [H][W][3] u8 in place, in u8 arithmetic: rgb += back where mask_back != 0 (wraps mod 256), then rgb = front
 *   where mask_front == 0.  Masks [H][W] u8.  back / mask_back and front / mask_front are NULL together (layer absent). */
int df_color_jitter(const unsigned char *src, const float *plan, int F, int H, int W, unsigned *scratch, unsigned char *dst,
                    df_stream_t stream);
int df_compose_frame(unsigned char *rgb, const unsigned char *back, const unsigned char *mask_back, const unsigned char *front,
                     const unsigned char *mask_front, int H, int W, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Detections from SegNet's own masks (the RGB-D frame -> SegNet -> per-object mask and box step of the reference's real-robot
 * setting; densefusion_amd/lib/segment.py).  Deterministic: no atomics, integer statistics, and a frame's results do not depend
 * on the other frames of the call.
 *
 * df_segment_input: rgb [F][H][W][3] u8 (4-byte aligned) -> out [F][H][W][4] fp32 (16-byte aligned), the SegNet eval path's input:
 *   ((float)v - mean_c) / std_c on the 0..255 values with the ImageNet mean / std (vanilla_segmentation/data_controller.py:79,
 *   true division), channel 3 = 0.
 * df_segment_detect: logits [F][H][W][ld] fp32 channels-last (16-byte aligned), the first C channels the classes; depth [F][H][W] u16.
 *   label [F][H][W] int32 = arg-max over the C classes (first maximum wins, NaN counts as maximal);
 *   stats [F][C][6] int32 = {pixels, pixels with depth != 0, rmin, rmax_excl, cmin, cmax_excl} of each class's tight box (zeros for
 *   an absent class);  det [F][C][6] int32: per frame, the classes 1..num_obj with more than min_pixels depth-valid pixels
 *   (datasets/ycb/dataset.py:87,146), ascending, as rows {cls, rmin, rmax_excl, cmin, cmax_excl, n_valid}, zero rows after them;
 *   ndet [F] the number of rows.  C <= 64, C <= ld <= 64, ld a multiple of 4, num_obj < C.
 *   scratch: df_segment_scratch_bytes(F, H, W, C) bytes (host-only query; 0 = bad sizes). */
size_t df_segment_scratch_bytes(int F, int H, int W, int C);
int df_segment_input(const unsigned char *rgb, float *out, int F, int H, int W, df_stream_t stream);
int df_segment_detect(const float *logits, const unsigned short *depth, int F, int H, int W, int ld, int C, int num_obj,
                      int min_pixels, int *label, int *stats, int *det, int *ndet, void *scratch, size_t scratch_bytes,
                      df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * SegNet training batches from rendered customCAD scenes (the work of the reference's SegDataset.__getitem__,
 * vanilla_segmentation/data_controller.py, on frames that never leave the device): B items, each a window of one rendered frame, composited
 * over a background, blurred, given pixel noise, flipped, normalised.  No allocation, no synchronisation, the caller's stream; integer
 * atomics only (the counts), so the outputs are bit-reproducible; an item's outputs do not depend on the other items of the call.
 *
 * df_seg_batch_scratch_bytes: bytes of scratch the call asks for (small: the call keeps nothing in memory between steps); 0 for sizes the
 *   call refuses (B, H*W, C below).
 * df_seg_batch:
 *   DEVICE: rgb [F][IH][IW][3] u8 and label [F][IH][IW] u16, the outputs of df_cad_render_scene[_lit] (label 0 = horizon, o + 1 = object
 *   o); back [NB][BH][BW][3] u8, NULL exactly when NB == 0; desc [B][8] int32, row n = {f, y0, x0, flip, b, by0, bx0, seed}: the frame,
 *   the window's corner in it, flip bit 0 = left-right and bit 1 = up-down, the background index (-1 = none) and its window's corner,
 *   the noise seed (taken as unsigned); the outputs; scratch.
 *   HOST, read during the call, a launch argument: class_map [O+1] int32, label value -> class 0..C-1; class_map[0] must be 0 (models
 *   map to their class, distractors to 0: they keep their colour and are background for the loss).
 *   Outputs: x_out [B][H][W][4] fp32 (16-byte aligned), the layout SegNet's channels-last input takes, channel 3 = 0;
 *   target_out [B][H][W] int64; counts_out [B][C] int32, zeroed by the call.
 *   DF_ERR_ARG, before anything is launched or written: a null pointer (back as above); F, IH, IW as for df_cad_render; H outside 1..IH
 *   or W outside 1..IW; H*W > 2^24; B outside 1..65535; O or C outside 1..64; a class_map entry outside 0..C-1 or class_map[0] != 0;
 *   NB > 0 with BH < H or BW < W; blur outside 0..1; noise_mul < 0; misaligned outputs; a short scratch.
 *   A BAD DESCRIPTOR -- f outside 0..F-1, the window not inside the frame, flip outside 0..3, b outside -1..NB-1, or (b >= 0) the
 *   background window not inside the pool -- gives zeros in all of the item's x_out, target_out and counts_out, and nothing is read
 *   through it (the rule of df_cad_scene_mask for a bad pair).
 *   Per item n and window pixel (i, j), 0 <= i < H, 0 <= j < W, which is frame pixel (y0 + i, x0 + j); p = i*W + j:
 *   G1. Class: l = label[f][y0+i][x0+j]; cls = class_map[l] if l <= O, else 0; counts_out[n][cls] += 1.
 *   G2. Composite: c_k = back[b][by0+i][bx0+j][k] if l == 0 and b >= 0, else rgb[f][y0+i][x0+j][k] (with no background the renderer's
 *       (130, 130, 130) horizon stays).
 *   G3. Blur (blur == 1): v_k = (sum of w * c_k + 8) >> 4 over the 3 x 3 neighbourhood, w = [1 2 1; 2 4 2; 1 2 1], the neighbour's
 *       indices clamped to the window 0..H-1, 0..W-1 (nothing outside the window is read); the sum is over COMPOSITED values, so an
 *       object's edge mixes with the background.  blur == 0: v_k = c_k.  Labels are never blurred.
 *   G4. Noise (noise_mul > 0): step D5 of df_cad_depth_sensor with s = seed and index 3p + k: h0 = mix32(seed ^ C0, 3p + k),
 *       h1 = mix32(seed ^ C1, 3p + k), S and n = floor((noise_mul * S + 2^31) / 2^32) as there; v_k = clamp(v_k + n, 0, 255).
 *       noise_mul = rint(sigma * 2^32 / sqrt(1431655765)); the reference's N(0, 5) is sigma = 5.
 *   G5. Write at the flipped position i' = H-1-i if flip bit 1 else i, j' = W-1-j if flip bit 0 else j:
 *       x_out[n][i'][j'] = {((float)v_k - mean_k) / std_k, 0}, the rule of df_segment_input; target_out[n][i'][j'] = cls.
 *   Noise and background are indexed in the source orientation: a flipped item is the mirror image of the unflipped one, in x and target
 *   alike, and the counts are equal.  Everything up to G5 is integer arithmetic. */
size_t df_seg_batch_scratch_bytes(int B, int H, int W, int C);
int df_seg_batch(const unsigned char *rgb, const unsigned short *label, int F, int IH, int IW, const unsigned char *back, int NB, int BH,
                 int BW, const int *class_map, int O, int C, const int *desc, int B, int H, int W, int blur, int noise_mul, float *x_out,
                 int64_t *target_out, int *counts_out, void *scratch, size_t scratch_bytes, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Scoring SegNet against rendered truth, and SegNet's label map as the masks of the customCAD pose path (densefusion_amd/lib/
 * segment_score.py).  No allocation, no synchronisation, the caller's stream; integer atomics only, so the outputs are bit-reproducible
 * and a frame's rows do not depend on the other frames of the call.
 *
 * df_seg_score_block_pixels: the pixels of a frame one workgroup of df_seg_score covers (host only; the tests put a frame on each side
 *   of it).
 * df_seg_score:
 *   DEVICE: logits [F][H][W][ld] fp32 channels-last (16-byte aligned), the first C channels the classes, as df_segment_detect reads
 *   them; target [F][H][W] int64, what df_seg_batch writes; label_out [F][H][W] int32 or NULL; conf [F][C][C] int32, indexed
 *   conf[f][truth][predicted]; skipped [F] int32.  The call sets conf and skipped to zero on the stream.
 *   DF_ERR_ARG, before anything is launched or written: a null logits, target, conf or skipped; F outside 1..65535; H or W below 1;
 *   H*W > 2^30; C outside 2..64; ld below C, above 64 or no multiple of 4; a misaligned pointer.
 *   Per frame f and pixel p:
 *   S1. pred = the arg-max of logits[f][p][0..C-1]: the first maximum wins and NaN counts as maximal (the rule of
 *       df_segment_detect, one text for both).  Channels C..ld-1 are never read as classes.  label_out[f][p] = pred, if given.
 *   S2. t = target[f][p], compared as 64 bits.  0 <= t < C: conf[f][t][pred] += 1.
 *   S3. Otherwise skipped[f] += 1 and no cell changes; label_out is written all the same.
 *   So conf[f] sums to H*W - skipped[f], its rows sum to the truth's class counts and its columns to the prediction's.
 * df_seg_masks:
 *   DEVICE: label [F][H][W] int32, F label maps in window coordinates (label_out above); mask_out [N][IH][IW] u16.
 *   HOST, read during the call, launch arguments: win [F][2] int32 = {y0, x0}, the corner of frame f's window in its IH x IW frame;
 *   pairs [N][2] int32 = {frame, class}.  A pair may repeat.
 *   DF_ERR_ARG, before anything is launched or written: a null pointer; F outside 1..65535; N below 1; IH outside 1..65535; IW below 1;
 *   IH*IW > 2^30; H outside 1..IH or W outside 1..IW; a window that leaves the frame (y0 outside 0..IH-H or x0 outside 0..IW-W); a
 *   pair's frame outside 0..F-1 or its class outside 0..64; a misaligned pointer.
 *   M1. mask_out[n][y][x] = 65535 where (y, x) lies inside the window of the pair's frame and label[frame][y-y0][x-x0] == class, and 0
 *       everywhere else.  EVERY element is written: the caller clears nothing.  The result is what df_cad_item_table and
 *       df_preprocess_objects_cad read as `label` with label_value 65535. */
int df_seg_score_block_pixels(void);
int df_seg_score(const float *logits, const int64_t *target, int F, int H, int W, int ld, int C, int *label_out, int *conf, int *skipped,
                 df_stream_t stream);
int df_seg_masks(const int *label, int F, int H, int W, const int *win, const int *pairs, int N, int IH, int IW, unsigned short *mask_out,
                 df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The exact closest point of a triangle mesh, for P points under K rigid (or any affine) transforms: what symmetry detection of a CAD
 * model needs (densefusion_amd/lib/mesh_distance.py, densefusion_amd/datasets/customCAD/symmetry.py).  A surface sample moved by a true
 * symmetry lies on the surface again, so its exact distance to the mesh is zero, whatever the sample spacing.  No allocation, no
 * synchronisation, the caller's stream; no atomics: the outputs are bit-reproducible, do not depend on the launch shape, and a query's
 * outputs do not depend on the other queries of the call.  Everything is fp64, one rounding per operation, in exactly the order
 * written below (no contraction into fused multiply-adds); a . b = (a_x b_x + a_y b_y) + a_z b_z and (a x b)_x = a_y b_z - a_z b_y,
 * cyclically, wherever a dot or a cross product appears.
 *
 * df_mesh_closest_tile_triangles: the triangles a workgroup stages at a time (host only; the tests put T on each side of it).
 * df_mesh_closest_scratch_bytes: the bytes of `scratch` for T triangles (host only; 0 for T < 1).
 * df_mesh_closest:
 *   DEVICE: vertices [V][3] fp32; triangles [T][3] int32; points [P][3] fp64; xf [K][12] fp64, K row-major 3 x 4 matrices; dist2_out
 *   [K][P] fp64; tri_out [K][P] int32; closest_out [K][P][3] fp64 or NULL; scratch (16-byte aligned, the per-triangle records).
 *   DF_ERR_ARG, before anything is launched or written: a null pointer other than closest_out; V, T, P or K below 1; 3 V, 3 T, 12 K or
 *   3 K P above INT_MAX; scratch short or misaligned; a pointer not aligned to its element.
 *   Per triangle t = (i0, i1, i2):
 *   M1. The triangle is dropped when an index lies outside 0..V-1 or two indices are equal; nothing is read through a bad index.  A
 *       dropped triangle has no distance and never wins.
 *   M2. A, B, C = (double) vertices[i0], [i1], [i2].  Edges in the order AB, BC, CA, e = (end) - (start); ee = e . e; iee = 1.0 / ee when
 *       ee > 0, otherwise 0.  e1 = B - A, e2 = C - A, n = e1 x e2, nn = n . n, inn = 1.0 / nn when nn > 0.  A triangle with nn == 0 (or
 *       a NaN) keeps its three edges and has no face.
 *   Per query (k, p):
 *   Q1. q_j = ((X[j][0] p_x + X[j][1] p_y) + X[j][2] p_z) + X[j][3], X = xf[k], p = points[p].
 *   Per pair:
 *   D1. Segment (U, e): w = q - U; s = (w . e) iee; s = s < 0 ? 0 : (s > 1 ? 1 : s) (a NaN stays a NaN); r_j = w_j - s e_j; d = r . r;
 *       closest point c_j = U_j + s e_j.
 *   D2. Face, only when nn > 0: w = q - A; u = (e1 x w) . n; v = (w x e2) . n; the foot is inside when u >= 0, v >= 0 and u + v <= nn;
 *       h = w . n; d = (h h) inn; closest point c_j = q_j - (h inn) n_j.
 *   D3. d_t = the first smallest of (AB, BC, CA, the face if the foot is inside), in that order; a NaN is no candidate.
 *   D4. The winner is the triangle of the smallest d_t; equal values go to the lowest t; a d_t that is a NaN or +inf never wins.
 *   D5. dist2_out = d_t and tri_out = t of the winner, closest_out = the closest point of the candidate that gave d_t.  With no winner
 *       (every triangle dropped, a NaN query): tri_out = -1, dist2_out = +inf, closest_out = q.
 * df_fp64_rate_probe: measurement only (tools/mesh_closest_bench.py): blocks x 256 lanes each run `iters` rounds of eight independent
 *   multiply-then-add chains in registers, 16 fp64 operations a round, and write their sums to sink [blocks * 256] (device). */
int df_mesh_closest_tile_triangles(void);
size_t df_mesh_closest_scratch_bytes(int T);
int df_mesh_closest(const float *vertices, int V, const int *triangles, int T, const double *points, int P, const double *xf, int K,
                    double *dist2_out, int *tri_out, double *closest_out, void *scratch, size_t scratch_bytes, df_stream_t stream);
int df_fp64_rate_probe(int blocks, int iters, double *sink, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Point-to-plane ICP of B estimated poses against the exact surface of their CAD meshes (densefusion_amd/lib/mesh_icp.py): the last,
 * geometric step of the customCAD pose path.  Each item brings its own observed points (camera frame), its object and a pose; the pose
 * moves on the device between iterations with no host round trip.  No allocation, no synchronisation, the caller's stream; no atomics:
 * the outputs are bit-reproducible and an item's outputs depend on its own points, pose, object and the mesh only, not on B or on the
 * items next to it.  Everything is fp64, one rounding per operation in exactly the order written below (no contraction), with the dot
 * and cross products of df_mesh_closest; only + - * / sqrt appear, so a restatement matches bit for bit (tests/mesh_icp_np.py).
 *
 * df_mesh_icp_scratch_bytes: the bytes of `scratch` for T triangles and B items of N points (host only; 0 when one is below 1).
 * df_mesh_icp:
 *   DEVICE: vertices [V][3] fp32, in the units of the points; triangles [T][3] int32; obj [B] int32; points [B][N][3] fp32; pose_in
 *   [B][7] fp64 (q wxyz, t; camera = R model + t: what df_estimate_poses_multi writes and df_add_metric reads); pose_out [B][7] fp64;
 *   stats [B][6] fp64 = {status, inliers and rms of the first pass, inliers and rms of the last pass, steps taken}; status 0 ok,
 *   1 few inliers, 2 degenerate, 3 bad object; scratch (16-byte aligned).
 *   HOST, read during the call, launch arguments: tri_begin [O+1] int32, object o owns the triangles tri_begin[o] .. tri_begin[o+1]-1;
 *   max_dist [O] fp64, the largest point-to-surface distance of an inlier (+inf: none).
 *   DF_ERR_ARG, before anything is launched or written: a null pointer; V, T, B or N below 1; 3 V, 3 T or 8 B N above INT_MAX; O outside
 *   1..64; tri_begin decreasing or outside 0..T; a max_dist that is not > 0; iters outside 0..64; cull not 0 or 1; scratch short or
 *   misaligned; a pointer not aligned to its element; pose_out or stats overlapping an input, the scratch or each other.
 *   Per item:
 *   S0. q = pose_in[0..3] / sqrt(((w w + x x) + y y) + z z), every component negated when w < 0 (the sign rule of the pose loop); t =
 *       pose_in[4..6]; stats = 0.  obj outside 0..O-1 or an empty range: status = bad object, nothing is read through it, pose_out =
 *       (q, t) and stats stay as they are now.  (A zero or NaN quaternion gives NaNs, no inlier and so `few inliers`.)
 *   Then pass k = 0 .. iters, steps I1..I6 for every item whose status is 0, and I7..I9 as well when k < iters:
 *   I1. R from q by the formula of the pose loop and of df_add_metric: n = ((w w + x x) + y y) + z z; n < 4 eps: R = I; otherwise
 *       s = sqrt(2.0 / n), (w, x, y, z) *= s, R = [(1 - y y) - z z, x y - z w, x z + y w; x y + z w, (1 - x x) - z z, y z - x w;
 *       x z - y w, y z + x w, (1 - x x) - y y].
 *   I2. The point in the model frame, x = R^T (p - t), in the form Q1 of df_mesh_closest: X = [R^T | o] with o_j = -((R[0][j] t_x +
 *       R[1][j] t_y) + R[2][j] t_z), the camera centre in the model frame; x_j = ((X[j][0] p_x + X[j][1] p_y) + X[j][2] p_z) + X[j][3],
 *       p widened exactly from fp32.
 *   I3. The closest point of the item's triangle range by M1, M2, D1..D5 of df_mesh_closest: the winner tri (-1: none), d2, c.
 *   I4. The point is an inlier when tri >= 0, d2 is finite and d2 <= max_dist[obj] * max_dist[obj], the winner has a face (nn > 0),
 *       and, with cull, n . (o - c) > 0 (n the winner's e1 x e2: the face looks at the camera).
 *   I5. sn = sqrt(nn); nh = n / sn; r = nh . (x - c); J = (x x nh, nh), six numbers.
 *   I6. Sums over the inliers: A[a][b] = sum J_a J_b (a <= b: 21), G[a] = sum r J_a (6), D = sum d2, and the count.  Order: lane l of
 *       256 adds its points l, l + 256, ... in ascending order onto 0; in each group of 64 lanes a binary tree (s = 32, 16, .., 1: lane
 *       l < s adds lane l + s); the four group totals as (T0 + T1) + (T2 + T3).  rms = sqrt(D / count), 0 with no inlier; stats' last
 *       inliers and rms = count, rms; on pass 0 the first as well.
 *   I7. count < 6: status = few inliers.  The item keeps its pose and is frozen: no later pass touches it, so its last inliers and rms
 *       are those of this pass, which a later pass would find again.
 *   I8. Cholesky A = L L^T by columns j = 0..5: s = A[j][j] - L[j][0]^2 - .. - L[j][j-1]^2 (left to right); s <= 2^-40 max_a A[a][a]
 *       (or a NaN): status = degenerate, pose kept, frozen (geometry that does not constrain six degrees of freedom: one flat face).
 *       L[j][j] = sqrt(s); L[i][j] = (A[i][j] - L[i][0] L[j][0] - .. - L[i][j-1] L[j][j-1]) / L[j][j].  Then L y = -G forwards,
 *       y_i = (-G_i - L[i][0] y_0 - ..) / L[i][i], and L^T z = y backwards, z_i = (y_i - L[i+1][i] z_{i+1} - .. - L[5][i] z_5) / L[i][i];
 *       z = (omega, dt): the model-frame motion x <- x + omega x x + dt that minimises the linearised sum of r^2.
 *   I9. h = omega * 0.5; m = sqrt(((1 + h_x h_x) + h_y h_y) + h_z h_z); c = (1 / m, -(h_x / m), -(h_y / m), -(h_z / m)), the conjugate
 *       of dq = (1, omega / 2) / |.|; q <- q (x) c (Hamilton product, each component summed left to right in the order w, x, y, z of q's
 *       components), normalised with the sign rule as in S0 (so R <- R dR^T); R from the new q by I1; t_j <- t_j - ((R[j][0] dt_x +
 *       R[j][1] dt_y) + R[j][2] dt_z); steps taken += 1.  No transcendental function.
 *   I10. pose_out = (q, t): a unit quaternion with w >= 0.  The last pass (k = iters) only scores: with iters = 0 the call is a pure fit
 *       score of the given poses. */
size_t df_mesh_icp_scratch_bytes(int T, int B, int N);
int df_mesh_icp(const float *vertices, int V, const int *triangles, int T, const int *tri_begin, const double *max_dist, int O,
                const int *obj, const float *points, const double *pose_in, int B, int N, int iters, int cull, double *pose_out,
                double *stats, void *scratch, size_t scratch_bytes, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * df_mesh_closest and df_mesh_icp through a bounding-box tree (densefusion_amd/lib/mesh_set.py `MeshSet.tree`): a second route to the
 * SAME outputs, byte for byte.  Both calls above test every query against every triangle of the object; these meet only the triangles
 * whose boxes are not provably farther than the best distance found so far.  No new numerics: a triangle's distance is D1..D3, the
 * winner is D4's (smallest d_t, then lowest t), so which triangles are met does not show in the result as long as no skipped triangle
 * could win or tie; DESIGN 12l proves that for rule B3.  The rules are densefusion_amd/csrc/mesh_tree_core.h.
 *
 * The tree (built once per mesh set on the host; its shape is not part of the contract, only the results of the walk are):
 *   B1. One binary tree per object range of tri_begin.  It holds the kept triangles (M1) that are not `loose`; a dropped triangle is in
 *       neither list.  A kept triangle is loose when a vertex is not finite, or it has a face (nn > 0) and nn < 2^-16 ee_i ee_j for two
 *       of its edges (an angle with sin^2 below 2^-16): the loose triangles of an object are tested for every query.
 *   B2. A node is 32 bytes: fp32 lo[3], hi[3] (the min / max of its triangles' fp32 vertices, exact in fp64) and int32 a, b.  Leaf: b > 0
 *       triangles, order[a] .. order[a+b-1] (call-global indices, ascending).  Inner node i: b == 0, children i + 1 and a.  A set of more
 *       than `leaf` triangles is split at the median of the centroids ((A + B) + C in fp64) along the longest axis of their bounds,
 *       ordered by (coordinate, index): the lower n / 2 go left.  At most 32 inner nodes lie on a path.
 *   B3. The walk of a query q: the loose list, then the tree from the root, the nearer child first.  A node is skipped only when
 *       lb - slack > cut, strictly, with lb = sum_j max(lo_j - q_j, 0, q_j - hi_j)^2, slack = (2^-36 R) R, R = W + E, W = max_j max(|q_j -
 *       lo_j|, |hi_j - q_j|) and E = max_j (hi_j - lo_j) of the root's box, and cut = the smaller of the best d_t so far and `limit` (+inf
 *       for df_mesh_closest_tree).
 *       A NaN query walks nothing and gets D5's result; an infinite one skips nothing.
 * df_mesh_tree_leaf_triangles: the `leaf` the wrappers build with (host only).
 * df_mesh_tree_sizes: the elements to allocate for T triangles in O objects: nodes (32 bytes each), order and loose (int32) (host only).
 *   DF_ERR_ARG: a null pointer, T below 1 or 3 T above INT_MAX, O outside 1..64.
 * df_mesh_tree_build (host only; every array is a HOST array): vertices [V][3] fp32, the scaled ones the distance calls read; triangles
 *   [T][3]; tri_begin [O+1] as for df_mesh_icp ({0, T} for df_mesh_closest_tree); leaf in 1..64.  Writes nodes (16-byte aligned) and
 *   order for all objects one after another, node_begin [O+1] and loose_begin [O+1] (object o owns nodes node_begin[o] ..
 *   node_begin[o+1]-1, its root first, and loose[loose_begin[o] .. loose_begin[o+1]-1]), and used[3] = the nodes, order entries and loose
 *   entries written.  A pure function of its inputs: two builds give equal bytes.
 *   DF_ERR_ARG, before anything is written: a null pointer; V or T below 1; 3 V or 3 T above INT_MAX; O outside 1..64; tri_begin
 *   decreasing or outside 0..T; leaf outside 1..64; nodes misaligned.  A tree deeper than 32 is refused with DF_ERR_ARG as well.
 * df_mesh_closest_tree: df_mesh_closest's arguments and outputs, then the tree of tri_begin = {0, T}: DEVICE nodes [n_nodes], order
 *   [n_order], loose [n_loose]; HOST (launch arguments) node_begin [2], loose_begin [2].  Launches df_mesh_closest's record kernel and
 *   one walking kernel: a query per lane, the walk's stack in LDS.
 *   DF_ERR_ARG, before anything is launched or written: every refusal of df_mesh_closest; a null tree pointer; nodes not 16-byte or
 *   order / loose not 4-byte aligned; node_begin or loose_begin not starting at 0, decreasing, or not fitting tri_begin (an object of n
 *   triangles, l of them loose, has at most l <= n loose entries and 2 (n - l) - 1 nodes); n_nodes below node_begin[O] or n_loose below
 *   loose_begin[O]; n_order of 0 with nodes, or above the triangles left for the trees.  Indices read from the device arrays that point
 *   outside the object's own ranges are not followed, so arrays that no build wrote give wrong answers but no read out of bounds.
 * df_mesh_closest_tree_host (host only; every array is a HOST array): the same walk on the CPU over the same arrays, for tests and
 *   stand-alone programs.  tested_out [K][P][2] int64 or NULL: the triangles and the boxes tested for the query.
 * df_mesh_icp_tree: df_mesh_icp's arguments, outputs, scratch and refusals, then the tree of the same tri_begin as above (node_begin and
 *   loose_begin [O+1]).  S0 and I1..I10 as they are, by the same kernels; only I3 is found by the walk, with limit = max_dist^2: a
 *   triangle beyond max_dist may go unfound, and such a point is no inlier either way (I4), so pose_out and stats are df_mesh_icp's. */
int df_mesh_tree_leaf_triangles(void);
int df_mesh_tree_sizes(int T, int O, size_t *nodes, size_t *order, size_t *loose);
int df_mesh_tree_build(const float *vertices, int V, const int *triangles, int T, const int *tri_begin, int O, int leaf, void *nodes,
                       int *node_begin, int *order, int *loose, int *loose_begin, size_t *used);
int df_mesh_closest_tree(const float *vertices, int V, const int *triangles, int T, const double *points, int P, const double *xf, int K,
                         double *dist2_out, int *tri_out, double *closest_out, void *scratch, size_t scratch_bytes, df_stream_t stream,
                         const void *nodes, size_t n_nodes, const int *node_begin, const int *order, size_t n_order, const int *loose,
                         size_t n_loose, const int *loose_begin);
int df_mesh_closest_tree_host(const float *vertices, int V, const int *triangles, int T, const double *points, int P, const double *xf, int K,
                              const void *nodes, size_t n_nodes, const int *node_begin, const int *order, size_t n_order, const int *loose,
                              size_t n_loose, const int *loose_begin, double *dist2_out, int *tri_out, double *closest_out,
                              long long *tested_out);
int df_mesh_icp_tree(const float *vertices, int V, const int *triangles, int T, const int *tri_begin, const double *max_dist, int O,
                     const int *obj, const float *points, const double *pose_in, int B, int N, int iters, int cull, double *pose_out,
                     double *stats, void *scratch, size_t scratch_bytes, df_stream_t stream, const void *nodes, size_t n_nodes,
                     const int *node_begin, const int *order, size_t n_order, const int *loose, size_t n_loose, const int *loose_begin);

/* ------------------------------------------------------------------------------------------------
 * Render-and-compare verification of B estimated poses (densefusion_amd/lib/pose_verify.py): the CAD mesh of each item is drawn at its
 * pose into a window of the item's own depth frame and compared, node by node, with the observed depth codes and optionally with a mask;
 * the result is twelve integer tallies per item.  No allocation, no synchronisation, the caller's stream; integer atomics only, so two
 * identical calls give identical bytes, and an item's row depends on its own record, pose, object, frame and mask only, not on B or on
 * the items next to it.  The fp64 part uses + - * / sqrt only, one rounding per operation in the order written (no contraction);
 * tests/pose_verify_np.py restates the call and all twelve columns are compared bit for bit.
 *
 * df_pose_verify_scratch_bytes: B*WH*WW 64-bit keys; 0 for sizes the call refuses (host only).
 * df_pose_verify:
 *   DEVICE: vertices [V][3] fp32 (file units) and triangles [T][3] int32 of O meshes laid one after another, as for df_cad_render_scene;
 *   depth [F][IH][IW] uint16, the observed depth codes (65535: no observation); mask [NM][IH][IW] uint16 or NULL; items [B][6] int32;
 *   pose [B][7] fp64 (q wxyz, t; camera = R model + t in cloud units: what df_estimate_poses_multi and df_mesh_icp write); stats
 *   [B][12] int64; scratch (8-byte aligned).
 *   HOST, read during the call, launch arguments: tri_begin [O+1], model_scale [O] as for df_cad_render_scene; proj, 16 doubles in
 *   df_cad_render's form.
 *   DF_ERR_ARG, before anything is launched or written: a null pointer (mask excepted); mask != NULL with NM < 1; B outside 1..65535;
 *   WH or WW below 1 or WH*WW above 2^30; F, IH, IW, V, T, O and proj as df_cad_render_scene refuses them, tri_begin by its three rules (one check for both calls); tol outside
 *   0..65535; cull not 0 or 1; cloud_div not finite or <= 0; scratch short or not 8-byte aligned.
 *   Item record: items[b] = {frame, object, r0, c0, mask_frame, mask_value}.  The window of item b is rows r0 .. r0+WH-1 and columns
 *   c0 .. c0+WW-1 of its frame; r0 and c0 may be negative and the window may hang over any edge of the frame: only the nodes inside both
 *   window and frame exist (corner + size is taken in 64 bits).  Window slot (r - r0) * WW + (q - c0) of item b is key b*WH*WW + slot.
 *   P0. Bad item: frame outside 0..F-1, object outside 0..O-1 or, with mask != NULL, mask_frame outside 0..NM-1: stats[b] = {1, 0, ...}
 *       and nothing is read through the record.  An empty triangle range is not bad: it renders nothing.
 *   P1. Pose: R from q by the formula of df_mesh_icp's step I1 (quat_to_mat of mesh_icp_core.h, unchanged: q need not be a unit
 *       quaternion; n < 4 eps gives R = I); t_j = pose[4 + j] * cloud_div.  [R | t] is a renderer's pose in its camera space (x right,
 *       y up, looking along -z).  A NaN in the pose draws nothing: T3 drops every triangle.
 *   P2. Raster, for the triangles tri_begin[object] .. tri_begin[object+1]-1: V2..V5 with model_scale[object] and T1..T6 of
 *       df_cad_render_mesh, verbatim, with no holes.  The node range of T4 is then intersected with the window; a triangle whose range
 *       becomes empty is dropped.  T7 into the item's own key plane: key = code << 32 | index of the triangle in the call's array, the
 *       smallest key per node wins (integer atomicMin).
 *   P3. Score, per existing node (r, q), all integer: cr = key >> 32, or "not rendered" when the node took no key; co =
 *       depth[frame][r][q], 65535 meaning "no observation"; m = mask != NULL and mask[mask_frame][r][q] == mask_value (a mask_value
 *       outside 0..65535 matches nothing).  A rendered node is `missing` when there is no observation, otherwise `agree` when
 *       |co - cr| <= tol, `front` when co < cr - tol (something nearer is in the way: neutral) and `behind` when co > cr + tol (the
 *       sensor sees through the model).  A node is `unexplained` when m holds, it is observed, and it is not rendered or `front`.
 *   stats[b] = {status (0, or 1: bad item), rendered, agree, front, behind, missing, mask (nodes with m), mask_observed (m and observed),
 *       unexplained, sum_abs (the sum of |co - cr| over `agree`), triangles that took at least one key test, live triangles (T1..T4)
 *       whose node range the window cut short (those it emptied are dropped and not counted)}.  A window wholly outside the frame
 *       gives a row of zeros.  Every entry is int64: sum_abs passes 2^31 on an ordinary
 *       window. */
size_t df_pose_verify_scratch_bytes(int B, int WH, int WW);
int df_pose_verify(const float *vertices, int V, const int *triangles, int T, const int *tri_begin, const double *model_scale, int O,
                   const double *proj, const unsigned short *depth, int F, int IH, int IW, const unsigned short *mask, int NM,
                   const int *items, const double *pose, double cloud_div, int B, int WH, int WW, int tol, int cull, long long *stats,
                   void *scratch, size_t scratch_bytes, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The two symmetry-aware BOP pose errors of B estimated poses against their true poses (densefusion_amd/lib/pose_error.py): MSSD, the
 * maximum symmetry-aware surface distance over ALL vertices of the item's CAD mesh, and MSPD, the same distance in the image plane; the
 * minimum runs over the whole symmetry set of the object (datasets/customCAD/symmetry.py `symmetry_set`).  No allocation, no
 * synchronisation, the caller's stream.  Every maximum and minimum is exact and order-free (a non-negative double orders like its bit
 * pattern: the maxima are integer atomics on the patterns; there is no floating-point atomic), so two identical calls give identical
 * bytes, and an item's row depends on its own poses, object, vertices and symmetries only: not on the launch shape, on B or on the items
 * next to it.  Everything is fp64, one rounding per operation in exactly the order written below (no contraction), with the dot product
 * of df_mesh_closest; only + - * / sqrt appear, so a restatement matches bit for bit (tests/pose_error_np.py).  The rules are
 * densefusion_amd/csrc/pose_error_core.h.
 *
 * df_pose_sym_error_scratch_bytes: the bytes of `scratch` for B items and S_max, the largest symmetry count of an object: per (item, s)
 *   two 64-bit maxima and the composed G_s, per item E; 0 for B outside 1..65535 or S_max < 1 (host only).
 * df_pose_sym_error_sweep_vertices: the vertices of one item that its workgroups take in one sweep at most, for a call of B items; an
 *   object with more is walked in several sweeps (host only; the tests put V on each side of it).
 * df_pose_sym_error:
 *   DEVICE: vertices [V][3] fp32, the scaled vertices df_mesh_icp reads (the units of the poses' translations); sym [NS][12] fp64, row-major
 *   3 x 4 matrices [R | c - R c], the sets of the objects one after another; obj [B] int32; pose_est, pose_gt [B][7] fp64 (q wxyz, t;
 *   camera = R model + t); out [B][6] fp64 = {status, mssd, s of mssd, mspd, s of mspd, vertices used}; status 0 ok, 1 bad item; s counts
 *   from the object's first symmetry; scratch (8-byte aligned).
 *   HOST, read during the call, launch arguments: vertex_begin [O+1] and sym_begin [O+1] int32, object o owns the vertices vertex_begin[o]
 *   .. vertex_begin[o+1]-1 and the symmetries sym_begin[o] .. sym_begin[o+1]-1; proj, 16 doubles in df_cad_render's form; IH, IW.
 *   DF_ERR_ARG, before anything is launched or written: a null pointer; V or NS below 1; 3 V or 12 NS above INT_MAX; B outside 1..65535; O
 *   outside 1..64; IH or IW below 1 or IH*IW above 2^30; proj not of df_cad_render's form (rows 2 = (0, 0, p22, p23), 3 = (0, 0, -1, 0));
 *   vertex_begin or sym_begin decreasing or outside 0..V, 0..NS; scratch short or not 8-byte aligned; a pointer not aligned to its
 *   element; out overlapping an input or the scratch.
 *   Per item, o = obj[b]:
 *   E0. Bad item: o outside 0..O-1, an empty vertex range or an empty symmetry range: out[b] = {1, 0, 0, 0, 0, 0} and nothing is read
 *       through the record.
 *   E1. R_e from pose_est's q and R_g from pose_gt's by the formula of df_mesh_icp's step I1 (quat_to_mat of mesh_icp_core.h, unchanged: q
 *       need not be a unit quaternion; n < 4 eps gives R = I); E = [R_e | t_e], M = [R_g | t_g], t = pose[4..6].
 *   E2. Per symmetry s of the object, once: G = M o S (the point goes through S first), G[j][k] = (M[j][0] S[0][k] + M[j][1] S[1][k]) +
 *       M[j][2] S[2][k] for k = 0..3, and then G[j][3] = G[j][3] + M[j][3].
 *   E3. Per vertex x, widened exactly from fp32: p_e = E x and p_g = G x in the form Q1 of df_mesh_closest:
 *       p_j = ((X[j][0] x_0 + X[j][1] x_1) + X[j][2] x_2) + X[j][3].
 *   E4. d = p_e - p_g, d2 = (d_0 d_0 + d_1 d_1) + d_2 d_2; a d2 that is not finite (a NaN included) counts as +inf.
 *   E5. The pixel of a point p, by V3 and V4 of df_cad_render_mesh on p as it stands (a projection of this form is homogeneous in p, so the
 *       units do not matter), with one reciprocal for the two divisions and no rounding to a node: c_k = ((P[k][0] p_0 + P[k][1] p_1) +
 *       P[k][2] p_2) + P[k][3] for the rows k = 0, 1, 3 of proj; i = 1.0 / c_3; u = (((c_0 i) + 1.0) IW) 0.5; v = ((1.0 - (c_1 i)) IH) 0.5.
 *       A point at or behind the camera plane (c_3 > 0 fails) has no pixel.
 *   E6. e2 = (u_e - u_g)(u_e - u_g) + (v_e - v_g)(v_e - v_g); +inf when either point has no pixel or e2 is not finite.
 *   E7. D_s = the largest d2 and P_s = the largest e2 over the object's vertices.  mssd = sqrt(min_s D_s), mspd = sqrt(min_s P_s), each
 *       with the lowest s that attains it; out[b] = {0, mssd, its s, mspd, its s, the object's vertex count}.  (A NaN pose or symmetry
 *       gives +inf with s = 0.)
 *   fp64 operations per (vertex, symmetry) pair by this count: E3 18 (p_g), E4 8, E5 27, E6 5 = 58, one of them a division. */
size_t df_pose_sym_error_scratch_bytes(int B, int S_max);
int df_pose_sym_error_sweep_vertices(int B);
int df_pose_sym_error(const float *vertices, int V, const int *vertex_begin, const double *sym, int NS, const int *sym_begin, int O,
                      const int *obj, const double *pose_est, const double *pose_gt, int B, const double *proj, int IH, int IW, double *out,
                      void *scratch, size_t scratch_bytes, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The third BOP pose error, the visible surface discrepancy of B estimated poses against their true poses and the observed depth
 * (densefusion_amd/lib/pose_error.py `PoseErrors.vsd`): both poses are drawn by df_pose_verify's own raster pass into windows of the
 * item's depth frame and compared node by node as distances from the camera.  It follows the BOP toolkit's `vsd` with visibility mode
 * `bop19` and the step cost; the toolkit was not at hand to compare with, so this comment is the definition.  No allocation, no
 * synchronisation, the caller's stream; integer atomics only: two identical calls give identical bytes, and an item's row depends on
 * its own record, poses, object and frame only.  The fp64 part uses + - * / sqrt only, one rounding per operation in the order written
 * (no contraction); tests/pose_error_np.py restates it and every column is compared bit for bit.  The rules are
 * densefusion_amd/csrc/pose_vsd_core.h.  df_pose_verify, its kernels and its outputs are unchanged.
 *
 * df_pose_vsd_scratch_bytes: two planes of B*WH*WW 64-bit keys, B*12 64-bit tallies of the raster passes and the object table; 0 for
 *   sizes the call refuses (host only).
 * df_pose_vsd: df_pose_verify's arguments without mask, NM and tol, and with
 *   DEVICE: rays [IH][IW][3] fp64, the loader's ray map (UnityDepthProjector.ray_map: the back-projection of node (r, q) at unit depth,
 *   z = 1); pose_est, pose_gt [B][7] fp64 in pose's place; stats [B][4 + NT] int64 = {status, union, inter, rendered_e, bad_0 ..
 *   bad_{NT-1}}; items [B][6] as for df_pose_verify, its two mask fields not read.
 *   HOST, read during the call: delta [O] fp64 and tau [O][NT] fp64, NT in 1..16, in the units of the distances below (the camera units
 *   of the renderer: cloud units x cloud_div).
 *   DF_ERR_ARG, before anything is launched or written: every refusal of df_pose_verify that is not about mask or tol; a null rays, pose,
 *   delta or tau; NT outside 1..16; a delta that is not finite or < 0; a tau that is < 0 (or a NaN) or below the one before it; rays or
 *   stats not 8-byte aligned.
 *   P0..P2 of df_pose_verify, verbatim, twice: with pose_est into the key plane E and with pose_gt into the key plane G (the same
 *   kernel, launched once per pose array).  A bad item (P0, no mask) has stats = {1, 0, ..}.
 *   Per existing node (r, q) of the window: c_e and c_g = key >> 32 of the planes, or "not rendered"; c_o = depth[frame][r][q], 65535
 *   meaning "no observation".
 *   S1. rho = sqrt((x x + y y) + z z) of rays[r][q].
 *   S2. D(c) = |z(c)| rho with z(c) = -p23 / (p22 + (1.0 - (double)c / 65534.0)), the loader's inverse of T6 in its order (the quotient
 *       c / 65534, the difference from 1, the sum with p22, the quotient, the negation being exact); z is negative in front of the
 *       camera and |z| = z < 0 ? -z : z.
 *   S3. vis_g = rendered_g and (no observation or D_g - D_o <= delta[object]); vis_e = rendered_e and (no observation or D_e - D_o <=
 *       delta[object] or vis_g); inter = vis_g and vis_e; union = vis_g or vis_e.
 *   S4. On inter nodes bad_k counts |D_g - D_e| >= tau[object][k] (the difference D_g - D_e, then its magnitude).
 *   The error itself is the wrapper's: vsd_k = (bad_k + union - inter) / union in fp64, 1 when union = 0. */
size_t df_pose_vsd_scratch_bytes(int B, int WH, int WW);
int df_pose_vsd(const float *vertices, int V, const int *triangles, int T, const int *tri_begin, const double *model_scale, int O,
                const double *proj, const unsigned short *depth, int F, int IH, int IW, const double *rays, const int *items,
                const double *pose_est, const double *pose_gt, double cloud_div, const double *delta, const double *tau, int NT, int B,
                int WH, int WW, int cull, long long *stats, void *scratch, size_t scratch_bytes, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Dense, projective point-to-plane ICP of B estimated poses against their whole depth windows (densefusion_amd/lib/pose_refine_dense.py):
 * the form of ICP depth trackers use.  Per pass the CAD mesh of each item is drawn at its current pose into the item's window by
 * df_pose_verify's own raster pass, every drawn node is associated with the depth observed at the same node, and the pose moves so as to
 * bring the observed points onto the planes of the triangles drawn there.  Association is by pixel, so visibility and self-occlusion are
 * the z-buffer's; the whole window takes part and a mask is optional.  The pose moves on the device between passes with no host round
 * trip.  No allocation, no synchronisation, the caller's stream; the only atomics are the raster's integer minima, there is no
 * floating-point atomic: two identical calls give identical bytes, and an item's outputs depend on its own record, pose, object, frame
 * and mask only, not on B, on the launch shape or on the items next to it.  Everything is fp64, one rounding per operation in exactly the
 * order written below (no contraction), with the dot and cross products of df_mesh_closest; only + - * / sqrt appear, so a restatement
 * matches bit for bit (tests/pose_dense_np.py).  The rules are densefusion_amd/csrc/pose_dense_core.h.  df_mesh_icp, df_pose_verify and
 * df_pose_vsd, their kernels and their outputs are unchanged.
 *
 * df_pose_refine_dense_scratch_bytes: B*WH*WW 64-bit keys, B*12 64-bit tallies of the raster pass, per item the working pose (7 doubles)
 *   and its model frame (16 doubles), and 32 doubles per (item, tile of 2048 window slots); 0 for sizes the call refuses (host only).
 * df_pose_refine_dense: df_pose_verify's arguments with `gate` in tol's place, and with
 *   DEVICE: rays [IH][IW][3] fp64, the loader's ray map as for df_pose_vsd; pose_in [B][7] fp64 in pose's place; pose_out [B][7] fp64;
 *   stats [B][6] fp64 = df_mesh_icp's columns {status, inliers and rms of the first pass, inliers and rms of the last pass, steps taken};
 *   status 0 ok, 1 few inliers, 2 degenerate, 3 bad item; scratch (8-byte aligned).
 *   DF_ERR_ARG, before anything is launched or written: every refusal of df_pose_verify (with gate outside 0..65535 for tol); a null
 *   rays, pose_in, pose_out or stats, or one that is not 8-byte aligned; iters outside 0..64; pose_out or stats overlapping a device input
 *   (vertices, triangles, depth, mask, rays, items, pose_in), the scratch or each other.
 *   Per item:
 *   S0 of df_mesh_icp: (q, t) = pose_in with q normalised and the sign rule; stats = 0.  A bad item (P0 of df_pose_verify) has status 3:
 *       nothing is read through its record, pose_out = (q, t) and stats stay as they are now.  An empty triangle range is not bad: it
 *       draws nothing and finds no inlier.  (A zero or NaN quaternion gives NaNs, draws nothing and so ends as `few inliers`.)
 *   Then pass k = 0 .. iters, D1..D5 for every item whose status is 0, and D6's solve and update as well when k < iters:
 *   D1. Draw: the item's key plane is set to "no key"; P1 and P2 of df_pose_verify, verbatim (the same kernel), from the current (q, t).
 *   D2. Per existing node (r, q) of the window (df_pose_verify's item record and slots): cr = key >> 32 or "not rendered"; co =
 *       depth[frame][r][q]; m as in P3.  The node is a candidate when it took a key, co != 65535, |co - cr| <= gate as integers and,
 *       with mask != NULL, m holds.  All integer: which nodes take part never depends on rounding.
 *   D3. The observed point: z = -p23 / (p22 + (1.0 - (double)co / 65534.0)), S2's formula with its sign (negative in front of the
 *       camera); p_k = (rays[r][q][k] z) / cloud_div for k = 0..2, the point in the units of the poses (what df_preprocess_objects_cad
 *       writes for this node and code, up to its fp32 roundings); x = X p with X = [R^T | o] of the current (q, t) by I1, I2 of
 *       df_mesh_icp: x_j = ((X[j][0] p_0 + X[j][1] p_1) + X[j][2] p_2) + X[j][3].
 *   D4. The plane: tri = the low 32 bits of the key, with the vertices A, B, C of triangles[tri] widened exactly from fp32.  f =
 *       model_scale[object] / cloud_div, once per item; a = A f, e1 = B f - a, e2 = C f - a (each product, then the difference);
 *       n = e1 x e2; nn = n . n.  No face (nn > 0 fails): no inlier.  sn = sqrt(nn); nh = n / sn; w = x - a; r = nh . w;
 *       J = (x x nh, nh), six numbers; d2 = r r.  The node is an inlier when each of the eight numbers J, r, d2 is finite.
 *   D5. The 28 sums of I6 of df_mesh_icp (A, G, D by its `accumulate`) and the count over the inliers, in an order that is a function of
 *       (WH, WW, slot) only.  The window's slots 0 .. WH*WW-1 are cut into tiles of 2048: tile i holds the slots 2048 i .. 2048 i + 2047
 *       below WH*WW.  Within a tile, lane l of 256 adds the tile's slots 2048 i + l, + 256, ... in ascending order onto 0; in each group of
 *       64 lanes a binary tree (s = 32, 16, .., 1: lane l < s adds lane l + s); the four group totals as (T0 + T1) + (T2 + T3): I6's lane
 *       order and tree.  The tile totals are then added onto 0 in ascending tile order.  rms = sqrt(D / count), 0 with no inlier.
 *   D6. I6's stats and I7..I9 of df_mesh_icp through the same function, unchanged: last inliers and rms = count, rms, on pass 0 the first
 *       as well; count < 6: status 1; a pivot <= 2^-40 of the largest diagonal entry: status 2 (one flat wall); otherwise the model-frame
 *       step, steps taken += 1.  A frozen item (status != 0) keeps its pose and its stats; whether it is still drawn is not part of the
 *       contract.
 *   I10 of df_mesh_icp: pose_out = (q, t), a unit quaternion with w >= 0; the last pass (k = iters) only scores.
 *   Launches per pass: the clear of the key planes, the raster, the accumulation (one row per (item, tile) to the scratch by plain
 *   stores) and the finish (the tile rows in order, the solve and the update; it also writes the next pass's X). */
size_t df_pose_refine_dense_scratch_bytes(int B, int WH, int WW);
int df_pose_refine_dense(const float *vertices, int V, const int *triangles, int T, const int *tri_begin, const double *model_scale, int O,
                         const double *proj, const unsigned short *depth, int F, int IH, int IW, const double *rays,
                         const unsigned short *mask, int NM, const int *items, const double *pose_in, double cloud_div, int B, int WH,
                         int WW, int gate, int cull, int iters, double *pose_out, double *stats, void *scratch, size_t scratch_bytes,
                         df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * df_pose_refine_dense with an outline term (densefusion_amd/lib/pose_refine_contour.py).  Planes alone leave a direction free on a view
 * of one flat wall or of two faces of a box (D6's status 2); the object's outline holds it.  Once per call the outline of the observed
 * object is found and every node learns its nearest outline node; per pass the outline of the drawn model is found in the key plane and
 * each of its nodes is pulled, across the image only, towards the observed outline node nearest to it.  The pairs' sums are added to
 * the planes' before the solve.  Like the dense call: no allocation, no synchronisation, the caller's stream, no floating-point atomic,
 * two identical calls give identical bytes, an item's row depends on its own record, pose, object, frame and mask only.  E1..E3 are
 * integer; E4 is fp64, one rounding per operation in the order written (no contraction), only + - * / appear; a restatement matches bit
 * for bit (tests/pose_contour_np.py).  The rules are densefusion_amd/csrc/pose_contour_core.h.  df_pose_refine_dense, df_pose_verify,
 * df_pose_vsd, df_pose_ppf and df_mesh_icp, their kernels and their outputs are unchanged: verify_raster_kernel and the dense
 * accumulation are launched as they stand.
 *
 * df_pose_refine_contour_scratch_bytes: df_pose_refine_dense_scratch_bytes, then per item the six dense columns (6 doubles, at the
 *   stride the dense kernels read a status through), one int32 per window slot for the feature map (the B*WH*WW of them rounded up to a
 *   multiple of 8 bytes), and a second set of 32 doubles per (item, tile); 0 for sizes the call refuses (host only).
 * df_pose_refine_contour: df_pose_refine_dense's arguments, and before pose_out edge_step in 0..65535 (codes), reach in 0..64 (nodes)
 *   and contour_scale, finite and >= 0.  stats [B][8] fp64 = the six columns of df_pose_refine_dense, then the outline pairs of the first
 *   and of the last pass.
 *   DF_ERR_ARG, before anything is launched or written: every refusal of df_pose_refine_dense (stats being [B][8] in the overlap rule),
 *   and edge_step, reach or contour_scale out of range.
 *   Per item: S0 and the bad-item rule of df_pose_refine_dense (a bad item's columns 6 and 7 are 0).  For a good item:
 *   E1. The observed outline, once per call, all integer.  A node exists when it lies inside the window and the frame.  on(r, q): co !=
 *       65535 and, with a mask, m holds.  A node is an observed-outline node when it is on and at least one of (r-1, q), (r+1, q),
 *       (r, q-1), (r, q+1) exists and is either not on or has co_nb - co > edge_step.  A neighbour that does not exist never makes an
 *       outline: an object cut by the frame or the window has no outline there.
 *   E2. The feature map, once per call, all integer.  Every existing node stores the slot of the observed-outline node of its own window
 *       with the smallest dr^2 + dq^2, among equals the lowest slot, and "none" when that minimum exceeds reach^2.
 *   Then pass k = 0 .. iters for every item whose status is 0: D1..D5 of df_pose_refine_dense, unchanged, give the plane sums P and their
 *   count, and
 *   E3. The drawn outline: E1's rule with "took a key" for on and cr for co.
 *   E4. A drawn-outline node c whose feature e is not "none" forms a pair.  a = X p(c, cr_c) and x = X p(e, co_e) with p by D3 (the code
 *       and the ray of the node named) and X the pass's model frame; w = x - a.  For k = 0, 1: n_k = (X[0][k], X[1][k], X[2][k]), the
 *       camera's x and y axes in the model frame; J = (x x n_k, n_k), each of the six then multiplied by contour_scale; r = (n_k . w)
 *       contour_scale; d2 = 0.  The pair counts when all fourteen numbers are finite; its two terms go through I6's `accumulate`, k = 0
 *       first.
 *   E5. The outline sums C and the pair count are reduced in D5's order by the slot of c (the same tiles, lanes and tree, a row of its
 *       own per tile).  S = P + C entry by entry for A and G, one add each; D, the count and the rms are P's.
 *   E6. D6 through the same function, unchanged, on S; the few-inlier rule uses P's count.  Columns 6 and 7 = the pair count of pass 0
 *       and of the last pass the item took part in.
 *   With contour_scale == 0, or when no pair forms, pose_out and the six dense columns equal df_pose_refine_dense's byte for byte.
 *   Launches: once per call the init, the outline with the feature transform's row pass (a row strip in LDS) and its column pass; per pass
 *   the dense call's clear, raster and accumulation, the outline accumulation and a finish that adds both row sets in order. */
size_t df_pose_refine_contour_scratch_bytes(int B, int WH, int WW);
int df_pose_refine_contour(const float *vertices, int V, const int *triangles, int T, const int *tri_begin, const double *model_scale, int O,
                           const double *proj, const unsigned short *depth, int F, int IH, int IW, const double *rays,
                           const unsigned short *mask, int NM, const int *items, const double *pose_in, double cloud_div, int B, int WH,
                           int WW, int gate, int cull, int iters, int edge_step, int reach, double contour_scale, double *pose_out,
                           double *stats, void *scratch, size_t scratch_bytes, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Pose hypotheses of B items from depth alone, by point-pair-feature voting (Drost et al. 2010; densefusion_amd/lib/pose_ppf.py): a
 * global search that needs the sampled CAD model and the item's depth window and no start pose.  Every pair of an oriented scene
 * reference point and another scene point looks up the model pairs of the same quantised feature and votes for (model point, rotation
 * about the normal); the best cell of each reference is a pose hypothesis, the hypotheses are clustered greedily and the K best clusters
 * are returned, to be refined by df_pose_refine_dense and told apart by df_pose_verify.  No allocation, no synchronisation, the caller's
 * stream; the votes are integer atomics and there is no floating-point atomic: two identical calls give identical bytes, and an item's
 * outputs depend on its own record, object, frame and mask only.  Everything that decides a result is fp64, one rounding per operation
 * in exactly the order written below (no contraction), with the dot and cross products of df_mesh_closest (dot: (a0 b0 + a1 b1) + a2 b2);
 * only + - * / sqrt, comparisons and integer arithmetic appear: no angle is ever computed, every angle is binned by its cosine against a
 * table the host passes, so a restatement matches bit for bit (tests/pose_ppf_np.py).  The rules are densefusion_amd/csrc/pose_ppf_core.h,
 * compiled for the host (the model builder) and the device (the vote) alike.  df_pose_verify, df_pose_vsd, df_pose_refine_dense and
 * df_mesh_icp, their kernels and their outputs are unchanged.
 *
 * Tables (HOST, launch arguments): ang_cos [NANG-1], the boundary cosines of the three feature angles, cos(k pi / NANG) for k = 1 ..
 *   NANG-1; alpha_cos [NA/2-1], cos(2 pi k / NA) for k = 1 .. NA/2-1; alpha_cs [NA][2], (cos, sin) of the sector centres (k + 1/2) 2 pi /
 *   NA.  Both cosine tables must descend strictly inside (-1, 1).  The bin of a value v in a table is the number of its boundaries b
 *   with v <= b.
 * The rule of a pair, shared by model and scene:
 *   F1. Oriented pair (p1, n1), (p2, n2): d = p2 - p1, L = sqrt(d . d); dropped unless L > 0 and finite.  fd = L / dist_step; dropped
 *       unless fd < ND; distance bin = (int)fd.
 *   F2. c1 = (d . n1) / L, c2 = (d . n2) / L, c3 = n1 . n2; a NaN drops the pair; each is binned in ang_cos.
 *   F3. key = ((distance bin NANG + bin1) NANG + bin2) NANG + bin3; NKEY = ND NANG^3.
 *   L1. The rotation R(n) that takes a unit normal n to +x: k = 1 + n_x; k < 2^-20: R = diag(-1, -1, 1); otherwise rows
 *       (1 - (n_y n_y + n_z n_z) / k, n_y, n_z), (-n_y, 1 - (n_y n_y) / k, -((n_y n_z) / k)), (-n_z, -((n_y n_z) / k), 1 - (n_z n_z) / k).
 *   L2. The angle of p2 about n1 as a unit vector: y = R_1 . d, z = R_2 . d (rows 1 and 2), m = sqrt(y y + z z); dropped unless m > 0 and
 *       finite; (c, s) = (y / m, -z / m): the turn about +x that brings the point into the half plane z = 0, y > 0.
 * df_ppf_model_sizes (host): buckets = O (NKEY + 1) and entries = the sum of NM_o (NM_o - 1), the sizes of bucket_begin and of the entry
 *   arrays df_ppf_model_build needs at most; DF_ERR_ARG when either passes INT_MAX, O is outside 1..64, ND outside 1..64, NANG outside
 *   1..32 or an object has fewer than 2 or more than 1024 points.
 * df_ppf_model_build (host, like df_mesh_tree_build; it reads no mesh: sampling the surface is the caller's): points, normals [NM][3]
 *   fp64 in the units of the poses, the normals of unit length; point_begin [O+1]; dist_step [O].
 *   M1. For every ordered pair i != j of an object (i, j counted from the object's first point) that keeps a key (F1..F3) and an angle
 *       (L1, L2 with n1 = n_i): the entry (i, (float)c, (float)s).
 *   M2. The entries of an object sorted stably by key, in ascending (i, j) within a key; bucket_begin[o][k] .. bucket_begin[o][k+1]-1
 *       are the entries of key k of object o in entry_point [.] int32 and entry_cs [.][2] fp32; the objects follow one another; *used =
 *       the entries written.
 *   DF_ERR_ARG: a null pointer; what df_ppf_model_sizes refuses; NA odd or outside 2..64; NM_o NA 4 > 150 KiB (the accumulator of one
 *   reference must fit the LDS of a compute unit); point_begin not running from 0 to NM; a dist_step that is not finite or <= 0; an
 *   ang_cos that does not descend inside (-1, 1).
 * df_pose_ppf_scratch_bytes: 8 doubles per (item, grid node), 20 per (item, reference) and one 64-bit count per item; 0 for sizes the call
 *   refuses (host only).  After a call the last B 64-bit words of that many bytes hold, per item, the table entries its scene pairs
 *   visited (V2): a diagnostic for tools/pose_ppf_bench.py and the tests, not an output.
 * df_pose_ppf:
 *   DEVICE: model_points, model_normals [NM][3] fp64, bucket_begin [O][NKEY+1], entry_point and entry_cs with n_entries entries, as
 *   df_ppf_model_build wrote them; depth, mask, items and rays as for df_pose_refine_dense; pose_out [B][K][7] fp64; votes_out
 *   [B][K][2] int32 = (score, members); stats [B][4] fp64 = (status, usable grid nodes, references with a hypothesis, clusters);
 *   hyp_out [B][NR][8] fp64 = (q, t, votes) per reference, or NULL; scratch (8-byte aligned).
 *   HOST, read during the call: point_begin [O+1], dist_step [O], cluster_dist [O] (the units of the poses), the three tables, proj.
 *   DF_ERR_ARG, before anything is launched or written: every refusal of df_pose_verify about pointers, mask, B, the window, F, IH, IW,
 *   proj, cloud_div and the scratch; every refusal of df_ppf_model_build; a bad alpha_cos or an alpha_cs entry outside -1..1; a
 *   cluster_dist that is not finite or < 0; cluster_trace outside -1..3; step or ref_step outside 1..64; reach outside 1..8; gate outside
 *   0..65535; K outside 1..16; more than 16384 grid nodes or 4096 references; n_entries or O (NKEY + 1) above INT_MAX; a pointer not
 *   aligned to its element (entry_cs to 8 bytes); an output overlapping a device input, the scratch or another output.
 *   Item record, window and P0 (bad item: status 3, every other output of the item zero, nothing read through the record) are
 *   df_pose_verify's.
 *   N1. Grid: GH = ceil(WH / step), GW = ceil(WW / step), G = GH GW; grid node (gr, gc), index gr GW + gc, is the node (r0 + gr step,
 *       c0 + gc step).  There is no compaction: an invalid node keeps its slot and casts no vote.  A node "counts" when it lies in the
 *       frame, its code co != 65535 and, with a mask, the mask holds the item's value there.  Its point is D3 of df_pose_refine_dense
 *       before the transform: z = -p23 / (p22 + (1.0 - (double)co / 65534.0)); p_k = (rays[r][q][k] z) / cloud_div.
 *   N2. Normal: per axis the two neighbours at -reach and +reach nodes of the frame (columns for dx, rows for dy); a neighbour takes
 *       part when it counts and |co_nb - co| <= gate as integers.  Both take part: d = P(+) - P(-); one: P(+) - P or P - P(-); none: no
 *       normal.  n = dx x dy; nn = n . n must be > 0 and finite; nh = n / sqrt(nn), negated when nh . p > 0 (the camera is the origin).
 *       A grid node is usable when it counts and has a normal.
 *   V1. References: the grid nodes whose gr and gc are multiples of ref_step, RH = ceil(GH / ref_step) rows of RW = ceil(GW / ref_step);
 *       reference index rr RW + rc; NR = RH RW.  An unusable reference has no hypothesis.  Per (item, reference) an accumulator
 *       acc [NM_o][NA] of uint32, zeroed.
 *   V2. For every other usable grid node: key by F1..F3 with (p1, n1) the reference; (c_s, s_s) by L1, L2.  For every entry (i, c_m,
 *       s_m) of the object's bucket of that key, widened exactly to fp64: c = c_m c_s + s_m s_s, s = s_m c_s - c_m s_s (the model angle
 *       less the scene angle); j = the bin of c in alpha_cos; sector = j when s >= 0, NA - 1 - j otherwise; acc[i][sector] += 1.
 *   V3. The winner is the largest count, then the lowest i, then the lowest sector.  A count of 0: no hypothesis (votes 0, pose zeros).
 *   H1. With (ca, sa) = alpha_cs[sector], Rs = R(n_ref), Rm = R(n_i): A = Rx Rm, rows Rm_0, ca Rm_1 - sa Rm_2, sa Rm_1 + ca Rm_2;
 *       R = Rs^T A, R[j][k] = (Rs[0][j] A[0][k] + Rs[1][j] A[1][k]) + Rs[2][j] A[2][k]; t_j = p_ref[j] - R_j . m_i.
 *   H2. q from R by the largest of (trace, R00, R11, R22) = (tr, ..), tried in this order with >= (a tie goes to the earlier): s =
 *       sqrt(1 + tr), f = 0.5 / s, q = (0.5 s, (R21 - R12) f, (R02 - R20) f, (R10 - R01) f); for R00: s = sqrt(((1 + R00) - R11) - R22),
 *       q = ((R21 - R12) f, 0.5 s, (R01 + R10) f, (R02 + R20) f); for R11: s = sqrt(((1 + R11) - R00) - R22), q = ((R02 - R20) f,
 *       (R01 + R10) f, 0.5 s, (R12 + R21) f); for R22: s = sqrt(((1 + R22) - R00) - R11), q = ((R10 - R01) f, (R02 + R20) f,
 *       (R12 + R21) f, 0.5 s).
 *   H3. q normalised with the sign rule of S0 of df_mesh_icp; hypothesis = (q, t, votes).
 *   C1. Per item the hypotheses with votes > 0 in the order (votes descending, reference index ascending).
 *   C2. In that order a hypothesis joins the first cluster, in creation order, whose first member (Rc, tc) is near: with R = the matrix
 *       of its q by I1 of df_mesh_icp, (R_0 . Rc_0 + R_1 . Rc_1) + R_2 . Rc_2 >= cluster_trace (the host passes 1 + 2 cos theta) and
 *       (t - tc) . (t - tc) <= cluster_dist[object] cluster_dist[object]; otherwise it founds a cluster.  A cluster's score is the
 *       integer sum of its members' votes, its pose its first member's: nothing is averaged.
 *   C3. Rank k < K of pose_out and votes_out: the k-th cluster by (score descending, creation order ascending); a score above INT_MAX
 *       is reported as INT_MAX; missing ranks stay zero.  status = 0, or 1 when the item has no hypothesis. */
int df_ppf_model_sizes(const int *point_begin, int O, int ND, int NANG, size_t *buckets, size_t *entries);
int df_ppf_model_build(const double *points, const double *normals, int NM, const int *point_begin, const double *dist_step, int O, int ND,
                       int NANG, int NA, const double *ang_cos, int *bucket_begin, int *entry_point, float *entry_cs, size_t *used);
size_t df_pose_ppf_scratch_bytes(int B, int WH, int WW, int step, int ref_step);
int df_pose_ppf(const double *model_points, const double *model_normals, int NM, const int *point_begin, const double *dist_step,
                const double *cluster_dist, int O, const int *bucket_begin, const int *entry_point, const float *entry_cs, size_t n_entries,
                int ND, int NANG, int NA, const double *ang_cos, const double *alpha_cos, const double *alpha_cs, const double *proj,
                const unsigned short *depth, int F, int IH, int IW, const double *rays, const unsigned short *mask, int NMK, const int *items,
                double cloud_div, int B, int WH, int WW, int step, int reach, int gate, int ref_step, int K, double cluster_trace,
                double *pose_out, int *votes_out, double *stats, double *hyp_out, void *scratch, size_t scratch_bytes, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Building block, exposed for unit parity tests and for callers that want single layers: channels-last
 * convolution / per-point GEMM on the fp32 matrix cores with the fused epilogue.
 *   out[b][oy][ox][out_coff + n] = act( sum_{ky,kx,c} in[b][oy*stride - pad + ky*dil][ox*stride - pad + kx*dil][in_coff + c]
 *                                        * wgt[n][ky][kx][c] + bias[n] + res[b][oy][ox][res_coff + n] )
 * in rows are in_ld floats wide, out rows out_ld, res rows res_ld; Cin, in_ld, in_coff multiples of 4;
 * multi-tap kernels need a power-of-two Cin.  act: 0 none, 1 ReLU, 2 PReLU (one slope at *prelu).
 * bias / res / prelu may be NULL. */
typedef struct df_conv_desc {
  const float *in, *wgt, *bias, *res, *prelu;
  float *out;
  int32_t B, H, W, Cin, in_ld, in_coff;
  int32_t OH, OW, Cout, out_ld, out_coff;
  int32_t res_ld, res_coff;
  int32_t KH, KW, stride, pad, dil, act;
  /* optional split-K scratch (device, owned by the caller, NULL = never split): with it df_conv2d_nhwc and df_conv2d_dgrad_nhwc cut
   * the reduction of launches that would fill less than half the chip (a few hundred pixels x a few thousand taps*channels: the
   * layer3 / layer4 convolutions of a training pass) into up to 8 ranges, keep the partial sums there and add them in a fixed order
   * with bias / residual / activation (deterministic; results differ from the unsplit launch by fp32 re-association).  Per call:
   * concurrent calls on different streams bring their own scratch.  The engine entry points never split. */
  void *splitk_ws;
  size_t splitk_ws_bytes;
} df_conv_desc;
int df_conv2d_nhwc(const df_conv_desc *d, df_stream_t stream);
/* The same convolution over nb crop-size buckets in ONE launch (the training step's direct k x k convolutions on a window of mixed crop
 * sizes): bucket i = B[i] maps of H[i] x W[i] (host arrays); the buckets' pixel rows are concatenated in bucket order in d->in, d->out and
 * d->res; d->B / H / W / OH / OW are ignored.  A workgroup's output tile lies inside one bucket; per output element the same sums in the same
 * order as a df_conv2d_nhwc call on that bucket alone without split-K: bit-identical. */
int df_conv2d_nhwc_multi(const df_conv_desc *d, int nb, const int *B, const int *H, const int *W, df_stream_t stream);
/* number of K ranges the calling thread's last df_conv2d_nhwc / df_conv2d_dgrad_nhwc launch was cut into (1 = not split): tests */
int df_conv_last_splitk(void);
/* Host only (no GPU): the fp32 kernel a df_conv2d_nhwc call on d (nb = 0; B / H / W unused) or the launch of a df_conv2d_nhwc_multi call
 * on nb buckets that starts at bucket `first` takes.  up > 1: the input dilation of a data-gradient launch; zcount: blockIdx.z batches;
 * groups > 0: a column-sum launch over row groups of that many rows (column sums into d->out); a split-K scratch in d counts for both
 * calls alike (the native trainer hands one to its multi-bucket launches).  route[7] receives the kernel (0 nothing
 * to compute, 1 v1, 2 v2, 3 v4, 4 v4 with column sums, 5 v4 over buckets), the workgroup tile's rows and columns, the v4 loader (0 general,
 * 1 plain GEMM, 2 tap-uniform), the split-K ranges, the column tiles per weight group and the buckets the launch covers.  Returns 0 or
 * the error the call fails with. */
int df_conv_route(const df_conv_desc *d, int nb, const int *B, const int *H, const int *W, int first, int up, int zcount, int groups,
                  int *route);

/* The same operator for 3x3 / stride 1 / pad == dil (any dilation) evaluated through the Winograd F(2x2,3x3) domain:
 * 16 multiplies per 2x2 outputs instead of 36 (the path the engine takes for the 256/512-channel convs of the
 * dilated ResNet trunk, lib/extractors.py:29-43,107-110).  Same descriptor; act none / ReLU; prelu unused.
 * scratch (device) of df_conv3x3_winograd_scratch_bytes(d) holds the transformed weights and both transformed
 * activations; results differ from df_conv2d_nhwc by fp32 re-association only. */
size_t df_conv3x3_winograd_scratch_bytes(const df_conv_desc *d);
int df_conv3x3_winograd_nhwc(const df_conv_desc *d, void *scratch, size_t scratch_bytes, df_stream_t stream);
/* The same with the output tile chosen: tile = 2 is the call above; tile = 4 is F(4x4,3x3) on the interpolation points
 * {0, 1, -1, 1/2, -2, inf}: 36 multiplies per 4x4 outputs (2.25 per output), transformed activations 2.25x the map instead of 4x;
 * rounding error ~4x that of tile 2 per layer (tests/test_conv_gpu.py), invisible in the selected pose.  The
 * engine picks direct / 2 / 4 per layer and map size from a cost estimate that depends on the layer geometry only. */
int df_wino_route(int H, int W, int dil, int Cin, int Cout);   /* the engine's choice for an H x W map: 0 direct, 2, 4 (host only) */
/* Host only: the tiles a B x H x W call of the given tile runs, and per axis whether it takes the packed layout (F(4x4), dilation > 1:
 * the sub-lattices of the axis laid one after another with one zero position between neighbours, where that needs fewer tiles than
 * padding each sub-lattice to whole tiles).  packed_y / packed_x may be NULL.  -1 on bad arguments. */
long df_wino_tiles(int B, int H, int W, int dil, int tile, int *packed_y, int *packed_x);
/* Host only: the map coordinate at position v of an axis of L points (the axis' strips one after another, tile * tiles-per-strip
 * positions each), or -1 for a separator, tile padding and positions outside; -2 on bad arguments. */
int df_wino_axis_map(int L, int dil, int tile, int v);
size_t df_conv3x3_winograd_tile_scratch_bytes(const df_conv_desc *d, int tile);
int df_conv3x3_winograd_tile_nhwc(const df_conv_desc *d, int tile, void *scratch, size_t scratch_bytes, df_stream_t stream);
/* Gradients of df_conv2d_nhwc (training path; `d` describes the FORWARD convolution, d->wgt = its weights):
 *   dgrad: dx[b][iy][ix][in_coff + c] (+)= sum dy[b][oy][ox][out_coff + n] * wgt[n][ky][kx][c] over the taps/outputs that
 *          read that input pixel; runs on the same MFMA kernel as the forward pass on flipped, transposed weights
 *          (w_scratch: Cout*KH*KW*Cin floats) with input dilation = the forward stride.  accumulate != 0 adds into dx.
 *   wgrad: dw[n][ky][kx][c] = sum_pixels dy[.][n] * x[. shifted by tap][c];  db[n] = sum_pixels dy[.][n] (db may be NULL).
 *          The pixel range is split over workgroups; their partial tiles go through `ws` (df_conv2d_wgrad_workspace_bytes)
 *          and are added in a fixed order, so gradients are bit-reproducible run to run (no atomics).
 * dy has the geometry of the forward output (out_ld / out_coff of `d`); activation masks are the caller's business. */
int df_conv2d_dgrad_nhwc(const df_conv_desc *d, const float *dy, float *dx, float *w_scratch, int accumulate,
                         df_stream_t stream);
size_t df_conv2d_wgrad_workspace_bytes(const df_conv_desc *d);
int df_conv2d_wgrad_nhwc(const df_conv_desc *d, const float *dy, float *dw, float *db, void *ws, size_t ws_bytes,
                         df_stream_t stream);
/* Weight gradient of df_conv2d_nhwc_multi: ONE contraction over the pixels of all buckets (bucket layout as there; dy rows concatenated like
 * d->out), dw / db overwritten; fixed-order reduction: bit-reproducible. */
size_t df_conv2d_wgrad_multi_workspace_bytes(const df_conv_desc *d, int nb, const int *B, const int *H, const int *W);
int df_conv2d_wgrad_nhwc_multi(const df_conv_desc *d, int nb, const int *B, const int *H, const int *W, const float *dy, float *dw, float *db,
                               void *ws, size_t ws_bytes, df_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Native training step (replaces the loop body of tools/train.py:146-163 of the reference: estimator / refiner forward,
 * criterion, loss.backward()) for B same-size frames, sequenced in C++ on one stream: no host synchronisation, no allocation,
 * every launch capturable in a hipGraph.  Parameters and gradients live in ONE flat fp32 buffer each, owned by the caller, in
 * KERNEL layout (conv O(HW)I, up_1 / up_2 tap-major, head layer 1 split, towers stacked); df_trainer_pack_param /
 * df_trainer_unpack_param convert a tensor from / to the reference's state-dict layout (same keys and shapes as
 * df_net_param_info), so checkpoints keep the reference's format.  Gradients are ACCUMULATED into flat_grad (loss.backward()
 * per frame, optimizer.step() every batch_size frames, tools/train.py:161-169) with fixed-order reductions only: two
 * identical steps give bit-identical gradient buffers.  param_version: any number that changes whenever flat_param's contents
 * change (the optimizer step count): the flipped weight copies of the data gradients are rebuilt only then; pass -1 to
 * rebuild them in every step (what a captured graph needs).
 *   kind 0: PoseNet + Loss (lib/network.py:95-132, lib/loss.py:13-70);  kind 1: PoseRefineNet + Loss_refine
 *   (lib/network.py:187-206, lib/loss_refiner.py:12-62).
 * df_posenet_train_step: img [B][3][H][W], cloud [B][N][3], choose [B][N] int64, obj [B] int64 (device), target /
 *   model_points [B][M][3], symmetric_host [B] (HOST ints or NULL: which frames take the nearest-neighbour branch),
 *   dropout != 0: Dropout2d of lib/pspnet.py:46,52 with masks hashed from `seed`;  outputs loss_out [B], dis_out [B],
 *   optional new_points [B][N][3], new_target [B][M][3], out_r [B][N][4], out_t [B][N][3], out_c [B][N], emb [B][32][N].
 * df_refiner_train_step: one refine iteration: points [B][N][3] (already in the current pose's frame), emb [B][32][N] ->
 *   dis_out [B], new_points, new_target for the next iteration. */
typedef struct df_trainer df_trainer;
df_trainer *df_trainer_create(int kind, int num_points, int num_obj);
void df_trainer_destroy(df_trainer *t);
int64_t df_trainer_flat_numel(const df_trainer *t);
int df_trainer_num_params(const df_trainer *t);
int df_trainer_param_info(const df_trainer *t, int i, char *key_out, int key_cap, int64_t *shape4, int *ndim);
int df_trainer_pack_param(const df_trainer *t, const char *key, const float *src, float *flat, df_stream_t stream);
int df_trainer_unpack_param(const df_trainer *t, const char *key, const float *flat, float *dst, df_stream_t stream);
size_t df_posenet_train_workspace_bytes(const df_trainer *t, int B, int H, int W, int M);
int df_posenet_train_step(df_trainer *t, const float *flat_param, float *flat_grad, int64_t param_version, int B, int H, int W,
                          const float *img, const float *cloud, const int64_t *choose, const int64_t *obj, const float *target,
                          const float *model_points, int M, const int *symmetric_host, float w, int dropout, unsigned seed,
                          float *loss_out, float *dis_out, float *new_points, float *new_target, float *out_r, float *out_t,
                          float *out_c, float *emb, void *ws, size_t ws_bytes, df_stream_t stream);
/* A window of frames of DIFFERENT crop sizes as one pass (what real data gives: the reference trains on whatever crop each frame has,
 * tools/train.py:131-176): nb crop-size buckets, bucket i = B[i] frames of H[i] x W[i] with their images at img[i] ([B_i][3][H_i][W_i],
 * device; the B / H / W / img arrays are HOST arrays); every other per-frame tensor (cloud, choose, obj, target, model_points, symmetric_host,
 * the outputs) is concatenated in bucket order, sum B frames.  Per-point layers, 1x1 convolutions, the F(4x4,3x3)-domain products and every
 * weight / bias gradient run ONCE over the rows of all buckets; direct k x k convolutions and the resampling kernels run per bucket.  The
 * gradient added to flat_grad equals the sum of the frames' one-per-pass gradients up to fp32 summation order (<= 1e-6 of each tensor's
 * scale; the order itself is fixed: bit-reproducible).  df_posenet_train_step is the one-bucket case. */
size_t df_posenet_train_multi_workspace_bytes(const df_trainer *t, int nb, const int *B, const int *H, const int *W, int M);
int df_posenet_train_step_multi(df_trainer *t, const float *flat_param, float *flat_grad, int64_t param_version, int nb, const int *B,
                                const int *H, const int *W, const float *const *img, const float *cloud, const int64_t *choose,
                                const int64_t *obj, const float *target, const float *model_points, int M, const int *symmetric_host,
                                float w, int dropout, unsigned seed, float *loss_out, float *dis_out, float *new_points,
                                float *new_target, float *out_r, float *out_t, float *out_c, float *emb, void *ws, size_t ws_bytes,
                                df_stream_t stream);
/* Per-launch timing of a trainer's MFMA launches (HIP events on the step's stream; measurement only).  df_trainer_profile(t, 1) arms
 * it; after the stream has been synchronised df_trainer_profile_read fills, per kind (0 forward, 1 data gradient, 2 weight gradient), the
 * summed launch durations in ms, the FLOPs the launches EXECUTE (2 M N K of the shapes really run, not the reference graph's) and the
 * launch counts since arming, and re-arms. */
/* Split-K of the small-grid forward / data-gradient launches of a step (default on: faster one-frame passes; results then depend on a
 * launch's grid size through fp32 re-association, and ReLU-gated gradients amplify that to ~1e-3 of a tensor's scale).  Off: every output
 * element is summed in one order whatever else shares the pass. */
int df_trainer_set_splitk(df_trainer *t, int enable);
int df_trainer_profile(df_trainer *t, int enable);
int df_trainer_profile_read(df_trainer *t, double *ms3, double *flops3, int *launches3);
size_t df_refiner_train_workspace_bytes(const df_trainer *t, int B, int M);
int df_refiner_train_step(df_trainer *t, const float *flat_param, float *flat_grad, int64_t param_version, int B, const float *points,
                          const float *emb, const int64_t *obj, const float *target, const float *model_points, int M,
                          const int *symmetric_host, float *dis_out, float *new_points, float *new_target, void *ws, size_t ws_bytes,
                          df_stream_t stream);

/* Per-launch timing of the GEMM kernel with HIP events on the call's stream (bench.py roofline).
 * df_net_profile(net, 1) arms it; after the stream has been synchronised df_net_profile_read returns the
 * summed duration (ms), the FLOPs the launches perform (2 M N K per launch, M = the rows launched), the part of them spent on
 * rows that are not padding (`gemm_useful_flops`: points beyond num_points in a 128-padded object block and Winograd tiles
 * beyond the map edge excluded), the algorithmic HBM bytes (each input, weight, output element once) and the number of GEMM
 * launches since arming, and re-arms. */
int df_net_profile(df_net *net, int enable);
int df_net_profile_read(df_net *net, double *gemm_ms, double *gemm_flops, double *gemm_useful_flops, double *gemm_bytes,
                        int *launches);
/* df_net_profile_read covers only the launches of the fp32-MFMA kernel.  The launches the bf16 x 6 split-precision kernel took
 * (df_gemm_route) are summed apart: df_net_profile_read_split returns their duration (ms), FLOPs (2 M N K, fp32-equivalent), useful
 * FLOPs and count since arming, WITHOUT re-arming; call it before df_net_profile_read. */
int df_net_profile_read_split(df_net *net, double *gemm_ms, double *gemm_flops, double *gemm_useful_flops, int *launches);

/* Which kernel a plain-GEMM layer (1x1 / per-point / Winograd-domain) of a PoseNet / refiner handle runs on: 1 = fp32 on the bf16 matrix
 * cores, operands cut into three bf16 terms, six term products (inside fp32 rounding of the exact product, not bit-identical to the fp32-MFMA
 * summation), 0 = the fp32-MFMA kernel.  n = output channels, k = reduction length, epilogue: 0 bias / activation, 1 + residual, 2 + per-object
 * bias and / or fused column sums, 3 anything else.  A pure function of these three: it does not depend on the rows, batch, crop size or
 * stream of a call.  Only the handles' own weights are routed; df_conv2d_nhwc and the trainers always run fp32. */
int df_gemm_route(int n, int k, int epilogue);

/* How the routed kernel's 256 x 256 tile form launches tiles_m x tiles_n output tiles in zcount batches (host only, no device call; for
 * tests).  The launch has *tiles_total tile positions, ceil(tiles_m / 8) * 8 * tiles_n per batch, the batches one behind the other: position
 * p belongs to XCD lane p % 8 and has sequence number s = p / 8; with S = ceil(tiles_m / 8) * tiles_n sequence numbers per batch it is batch
 * s / S, row tile (s % S / tiles_n) * 8 + p % 8 (a padding position when that is not below tiles_m) and column tile s % S % tiles_n.
 * *grid workgroups run (a multiple of 8 and at most *tiles_total; `workgroups` is the most allowed, e.g. the compute units; <= 0: one
 * per position); workgroup b keeps lane b % 8 and takes the sequence numbers b / 8 + i (*grid / 8), i = 0 .. trips[b] - 1.  trips (may be
 * NULL) receives min(*grid, cap) entries. */
int df_split_walk(int tiles_m, int tiles_n, int zcount, int workgroups, int *grid, int *tiles_total, int *trips, int cap);

/* One plain-GEMM launch as the engines make them, with every epilogue option (for kernel tests; like df_conv2d_nhwc it runs the fp32 kernels):
 *   out[z][m][n] = act(sum_k in[z][m][k] wgt[z][n][k] + bias + res[m][n]),  z < zcount, m < M, n < N, dense fp32 device operands.
 * bias: NULL, [zcount][N], or with bias_group_ld > 0 one row of bias_group_ld floats per row group (row m is in group m / rows_per_group).
 * res: NULL or [M][N] (zcount 1).  act: 0 none, 1 ReLU.  colsum: NULL, or [zcount][2 ceil(M / 128)][N]: row r receives the column sums of the
 * activated rows 64 r .. 64 r + 63 that are real (below M and, with row groups, m % rows_per_group < rows_valid); out may then be NULL.
 * rows_per_group: 0 or a multiple of 128 that divides M. */
int df_gemm_rows(const float *in, const float *wgt, const float *bias, const float *res, float *out, float *colsum, int64_t M, int N,
                 int K, int zcount, int act, int rows_per_group, int rows_valid, int bias_group_ld, df_stream_t stream);

/* Debug taps: with df_net_debug_taps(net, 1) armed, a single-bucket PoseNet forward keeps device copies of its named
 * intermediates (channels-last): "stem" [B][H/2][W/2][64] (conv1 + ReLU, lib/extractors.py:115-117), "layer1".."layer4",
 * "psp" [B][H/8][W/8][1024] (lib/pspnet.py:20-24), "up_1" [B][H/4][W/4][256], "up_2" [B][H/2][W/2][64], "up_3" [B][Npad][64]
 * (rows of the chosen pixels only, Npad = num_points rounded up to 128), "ap_x" [B][1024] (lib/network.py:65).  The full PoseNet
 * forward (not the pose-selection path of df_estimate_poses) also keeps the point layers and heads, point-major [B][Npad][C]:
 * "pf" [..][384] = x1 64 | e1 64 | x2 128 | e2 128 (pointfeat_1 | pointfeat_2, lib/network.py:57-62), "x5" [..][512] (conv5 + ReLU),
 * "h1" [..][1920] = conv1_r | conv1_t | conv1_c (640 each, + ReLU), "h2" [..][768] = conv2 r | t | c (256 each), "h3" [..][384] =
 * conv3 r | t | c (128 each).  A refiner handle keeps its last refine iteration (the only one of df_refiner_forward): "rf_pf"
 * [B][Npad][384] = x1 64 | x2 128 | e1 64 | e2 128 (NOT PoseNet's order; lib/network.py:160-163 reads x1 | e1 | x2 | e2),
 * "rf_x5" [B][Npad][512], "rf_apx" [B][1024] (the AvgPool1d of conv6 + ReLU), "rf_f1" [B][1024] = conv1_r | conv1_t (+ ReLU),
 * "rf_f2" [B][256] = conv2_r | conv2_t (+ ReLU).  Point rows N .. Npad-1 of an object's block are padding, not part of the
 * contract.  It allocates, so
 * it is for debugging / layer-level parity tests only (not under hipGraph capture).  df_net_debug_tap_read copies a tap to dst
 * (host or device, `cap` floats) after the caller has synchronised the stream and returns its shape; dst == NULL only queries
 * the shape.  df_net_debug_taps(net, 0) frees the copies. */
int df_net_debug_taps(df_net *net, int enable);
int df_net_debug_tap_read(df_net *net, const char *name, float *dst, int64_t cap, int64_t *shape4);

#ifdef __cplusplus
}
#endif
#endif /* DFUSION_H_ */
