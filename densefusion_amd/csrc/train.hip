// Native training step of PoseNet / PoseRefineNet (tools/train.py:131-176 of the reference): forward, loss and backward of B same-size
// frames sequenced in C++ on one stream -- no host synchronisation, no allocation, every launch capturable in a hipGraph.
//
//   * parameters and gradients live in ONE flat fp32 buffer each, in KERNEL layout (conv O(HW)I, up_1 / up_2 tap-major, head layer 1
//     split into its per-point and global-feature column blocks, the three head towers stacked): the caller owns both buffers
//     (Adam and the gradient all-reduce are layout-agnostic); df_trainer_pack_param / _unpack_param convert to and from the
//     reference's state-dict layout, so checkpoints keep the reference's keys and shapes (tools/train.py:172-176).
//   * gradients are ACCUMULATED into the flat gradient buffer (the reference's `loss.backward()` per frame, `optimizer.step()`
//     every batch_size frames, tools/train.py:161-169); every reduction has a fixed order -- no float atomics anywhere: two
//     identical steps give bit-identical gradient buffers.
//   * the forward half keeps the exact rewrites of the inference engine that have a cheap adjoint: concatenations written in
//     place (channel offsets), the global-feature fold of head layer 1, up_1 / up_2 as low-resolution per-tap products followed by
//     the 9-tap interpolation, up_3 + final 1x1 + LogSoftmax only at the chosen pixels, the last head layer only for the frame's
//     object (lib/network.py:119-131: the other objects' rows receive no gradient in the reference either).
//
// Reference lines mirrored: lib/extractors.py:29-43,114-124; lib/pspnet.py:20-24,27-37,64-77; lib/network.py:53-68,95-132,151-206;
// lib/loss.py:13-70; lib/loss_refiner.py:12-62.
//
// This file: the two network steps, layer by layer, and the C ABI.  train_kernels.h: the glue kernels between the MFMA launches.
// train_tape.h: the trainer handle, the step's arena / activation records / backward tape and the layer idioms the steps are written in.
#include <cstdlib>
#include <cstring>

#include "layers.h"
#include "loss.h"
#include "train_tape.h"

namespace df {
namespace {

// ------------------------------------------------------------------------------------------------
// layers of PoseNet's colour branch
// ------------------------------------------------------------------------------------------------
Act *basic_block(Step &s, Act *x, int cin, const std::string &base, int planes, int stride, int dil, bool has_ds, Act *out_into = nullptr) {
  Act *t = conv(s, x, cin, ConvW{base + "conv1.weight"}, planes, 3, stride, dil, dil, ACT_RELU);
  Act *res = x;
  if (has_ds) res = conv(s, x, cin, ConvW{base + "downsample.0.weight"}, planes, 1, stride, 0, 1, ACT_NONE);
  return conv(s, t, planes, ConvW{base + "conv2.weight"}, planes, 3, 1, dil, dil, ACT_RELU, res, out_into);
}

// Dropout2d (lib/pspnet.py:46,52): one keep / drop decision per (frame, channel); out of place -- the PReLU gradient upstream needs
// the un-scaled activation
Act *dropout2d(Step &s, Act *a, float p, unsigned seed) {
  const Level *lv = a->lv;
  float *scale = s.f((size_t)lv->frames * a->C);
  Act *o = s.act(lv, a->C);
  const std::vector<BTab> tabs = make_tabs(lv);
  if (s.live()) {
    s.fail(df_dropout2d_mask(scale, (int64_t)lv->frames * a->C, seed, p, s.st));
    for (const BTab &t : tabs)
      hipLaunchKernelGGL(channel_scale_multi_kernel, dim3(nblk(tab_rows(t) * (a->C / 4))), dim3(TB), 0, s.st, a->v.d, a->v.ld, scale, o->v.d, o->v.ld, a->C / 4, t);
  }
  s.tape.push_back([=](Step &s) {
    s.grad_of(a);
    if (s.live())
      for (const BTab &t : tabs)
        hipLaunchKernelGGL(channel_scale_multi_kernel, dim3(nblk(tab_rows(t) * (a->C / 4))), dim3(TB), 0, s.st, o->g.d, o->g.ld, scale, a->g.d, a->g.ld, a->C / 4, t);
  });
  return o;
}

// PSPUpsample through the low-resolution per-tap products (layers.hip upconv_gather): x [B][h][w][Cin] -> [B][2h][2w][Cout] per bucket;
// the product, its weight and data gradients, the activation / bias adjoints are single launches over the rows of all buckets
Act *upconv(Step &s, Act *x, const std::string &base, int cin, int cout) {
  const Level *li = x->lv;
  const int nb = li->nb();
  Act *y = s.act(li, 9 * cout);
  const ConvW cw{base + "conv.1.weight"};
  ConvParams p = flat_params(x, cin, s.p(cw.name), nullptr, y, ACT_NONE);
  s.with_splitk(p);
  s.gemm(GK_FWD, p);
  Level up;
  for (int i = 0; i < nb; ++i) up.push(li->B[i], 2 * li->H[i], 2 * li->W[i]);
  const Level *lo = s.level(up);
  Act *o = s.act(lo, cout);
  if (s.live())
    for (int i = 0; i < nb; ++i)
      s.fail(launch_upconv_gather(y->v.d + li->off[i] * 9 * cout, s.p(base + "conv.1.bias"), s.p(base + "conv.2.weight"), o->v.d + lo->off[i] * cout, li->B[i],
                                  li->H[i], li->W[i], cout, s.st));
  s.tape.push_back([=](Step &s) {
    launch_act_bwd(s, o, ACT_PRELU, s.p(base + "conv.2.weight"), s.gr(base + "conv.2.weight"));
    {   // bias gradient: column sums of the pre-activation gradient over all pixels
      const long rows = o->rows();
      const int nbk = (int)((rows + 255) / 256);
      float *part = s.f((size_t)nbk * cout);
      if (s.live()) {
        hipLaunchKernelGGL(colsum_obj_kernel, dim3((cout + 31) / 32, nbk), dim3(256), 0, s.st, o->g.d, o->g.ld, part, 256, cout, rows);
        hipLaunchKernelGGL(colsum_obj_kernel, dim3((cout + 31) / 32, 1), dim3(256), 0, s.st, part, cout, s.gr(base + "conv.1.bias"), nbk, cout, (long)nbk, 1);
      }
    }
    s.grad_of(y);
    if (s.live())
      for (const BTab &t : make_tabs(li))
        hipLaunchKernelGGL(upconv_gather_bwd_multi_kernel, dim3(nblk(tab_rows(t) * 9 * (cout / 4))), dim3(TB), 0, s.st, o->g.d, y->g.d, cout, t);
    gemm_bwd(s, p, y->g, x, cw.name, "");
  });
  return o;
}

// ------------------------------------------------------------------------------------------------
// the point branch both networks start with (PoseNetFeat lib/network.py:53-68, PoseRefineNetFeat :151-175), on point rows padded to Npad per frame
// ------------------------------------------------------------------------------------------------
struct PointFeat { Act *all, *x1, *e1, *x2, *e2; };      // [rows][384] = [x1 64 | e1 64 | x2 128 | e2 128] and its channel slices

// conv1 on the xyz rows (device [B][N][3]), e_conv1 on the embedding rows, conv2 / e_conv2, each written into its slice.  emb_dx: the
// embedding came from a network (PoseNet's colour branch) and wants e_conv1's data gradient
PointFeat point_feat(Step &s, const float *xyz, Act *emb_pm, int B, bool emb_dx) {
  const int N = s.t->N, Npad = round_up(N, 128), rows = B * Npad;
  Act *pf = s.act((long)rows, 384);
  Act *x1 = slice(s, pf, 0, 64), *e1 = slice(s, pf, 64, 64), *x2 = slice(s, pf, 128, 128), *e2 = slice(s, pf, 256, 128);
  if (s.live()) {
    hipMemsetAsync(pf->v.d, 0, (size_t)rows * 384 * sizeof(float), s.st);
    launch_cloud_conv1(xyz, nullptr, s.p("feat.conv1.weight"), s.p("feat.conv1.bias"), pf->v.d, 384, B, N, Npad, s.st);
  }
  s.tape.push_back([=](Step &s) {          // conv1's parameters (runs last of the point branch: x1's gradient is complete by then)
    Act m = *x1;
    launch_act_bwd(s, &m, ACT_RELU, nullptr, nullptr);
    const int chunks = (N + 63) / 64;
    float *part = s.f((size_t)B * chunks * 64 * 4);
    if (s.live()) {
      hipLaunchKernelGGL(cloud_conv1_bwd_kernel, dim3(B * chunks), dim3(64), 0, s.st, x1->g.d, 384, xyz, B, N, Npad, part);
      hipLaunchKernelGGL(cloud_conv1_bwd_finish_kernel, dim3(1), dim3(64), 0, s.st, part, B * chunks, s.gr("feat.conv1.weight"), s.gr("feat.conv1.bias"));
    }
  });
  conv(s, emb_pm, 32, ConvW{"feat.e_conv1.weight", 0, "feat.e_conv1.bias"}, 64, 1, 1, 0, 1, ACT_RELU, nullptr, e1, emb_dx);
  conv(s, x1, 64, ConvW{"feat.conv2.weight", 0, "feat.conv2.bias"}, 128, 1, 1, 0, 1, ACT_RELU, nullptr, x2);
  conv(s, e1, 64, ConvW{"feat.e_conv2.weight", 0, "feat.e_conv2.bias"}, 128, 1, 1, 0, 1, ACT_RELU, nullptr, e2);
  return PointFeat{pf, x1, e1, x2, e2};
}
// every slice's gradient lives in pf's ONE [rows][384] buffer, from the moment its first writer has run (PoseNet: head layer 1's data
// gradient; the refiner: conv5's)
void alias_slices(const PointFeat &pf) {
  alias_grad(pf.x1, pf.all, 0); alias_grad(pf.e1, pf.all, 64); alias_grad(pf.x2, pf.all, 128); alias_grad(pf.e2, pf.all, 256);
}

// conv6 + ReLU and its mean over each frame's N points (AvgPool1d) from the GEMM's fused column sums -> the [B][1024] mean.  The backward
// broadcasts the mean's gradient (its g, by then allocated by the caller or by a consumer's grad_of) to the points the ReLU let through
Act *conv6_mean(Step &s, Act *x5, int B) {
  const int N = s.t->N, Npad = round_up(N, 128), rows = B * Npad;
  Act *x6 = s.act((long)rows, 1024);
  ConvParams p6 = flat_params(x5, 512, s.p("feat.conv6.weight"), s.p("feat.conv6.bias"), x6, ACT_RELU);
  p6.rows_per_group = Npad; p6.rows_valid = N;
  int prow;
  {
    ConvParams q6 = p6;
    q6.out = nullptr;            // (the partial-row count is that of the column-sum launch's tile, chosen when out is null or colsum set)
    prow = conv_colsum_rows(q6);
  }
  float *partial = s.f((size_t)prow * 1024);
  p6.colsum = partial;
  s.gemm(GK_FWD, p6);
  Act *ap = s.act((long)B, 1024);
  if (s.live()) launch_colsum_finish(partial, prow / B, ap->v.d, B, 1024, N, s.st);
  s.tape.push_back([=](Step &s) {
    s.grad_of(x6);
    if (s.live()) hipLaunchKernelGGL(mask_bcast_kernel, dim3(nblk((long)rows * 256)), dim3(TB), 0, s.st, x6->v.d, ap->g.d, x6->g.d, B, N, Npad, 256);
    ConvParams f = p6;
    f.colsum = nullptr;
    gemm_bwd(s, f, x6->g, x5, "feat.conv6.weight", "feat.conv6.bias");
  });
  return ap;
}

// ------------------------------------------------------------------------------------------------
// PoseNet step
// ------------------------------------------------------------------------------------------------
struct PoseNetIO {
  int nb;                        // crop-size buckets of the pass; frames are concatenated in bucket order everywhere below
  const int *B, *H, *W;          // host [nb]
  const float *const *img;       // host [nb]: device pointers [B_i][3][H_i][W_i]
  int M;
  const float *cloud, *target, *model_points;
  const int64_t *choose, *obj;
  const int *symmetric;     // host [sum B]
  float w;
  int dropout;
  unsigned seed;
  float *loss, *dis, *new_points, *new_target;        // [B], [B], [B][N][3], [B][M][3]
  float *out_r, *out_t, *out_c, *emb;                 // optional copies of the predictions ([B][N][4] ...); emb [B][32][N]
};

void posenet_step(Step &s, const PoseNetIO &io) {
  Trainer &t = *s.t;
  const std::string C = CNN;
  int B = 0;
  for (int i = 0; i < io.nb; ++i) B += io.B[i];
  const int nb = io.nb, N = t.N, Npad = round_up(N, 128), rows = B * Npad;
  s.take_splitk((size_t)32 << 20);

  // ---- colour branch (lib/extractors.py:114-124, lib/pspnet.py:64-77) ----
  Level limg;
  for (int i = 0; i < nb; ++i) limg.push(io.B[i], io.H[i], io.W[i]);
  Act *img4 = s.act(s.level(limg), 4);
  if (s.live())
    for (int i = 0; i < nb; ++i) launch_nchw3_to_nhwc4(io.img[i], img4->v.d + img4->lv->off[i] * 4, io.B[i], io.H[i], io.W[i], s.st);
  Act *stem = conv(s, img4, 4, ConvW{C + "feats.conv1.weight"}, 64, 7, 2, 3, 1, ACT_RELU, nullptr, nullptr, false);
  Level lpool;
  for (int i = 0; i < nb; ++i) lpool.push(io.B[i], conv_out(stem->lv->H[i], 3, 2, 1, 1), conv_out(stem->lv->W[i], 3, 2, 1, 1));
  Act *x = s.act(s.level(lpool), 64);
  {
    const Level *ls = stem->lv, *lx = x->lv;
    if (s.live())
      for (int i = 0; i < nb; ++i)
        launch_maxpool3s2(stem->v.d + ls->off[i] * 64, x->v.d + lx->off[i] * 64, ls->B[i], ls->H[i], ls->W[i], 64, lx->H[i], lx->W[i], s.st);
    Act *xp = x;
    s.tape.push_back([=](Step &s) {
      s.grad_of(stem);
      if (s.live())
        for (const BTab &t : make_tabs(ls, lx))
          hipLaunchKernelGGL(maxpool3s2_bwd_multi_kernel, dim3(nblk(tab_rows(t) * 16)), dim3(TB), 0, s.st, stem->v.d, xp->g.d, stem->g.d, 64, t);
    });
  }
  int cin = 64;
  const int planes_of[4] = {64, 128, 256, 512}, stride_of[4] = {1, 2, 1, 1}, dil_of[4] = {1, 1, 2, 4};
  Act *cat = nullptr;      // [rows][2560]: the four pyramid priors then layer4's output (lib/pspnet.py:23)
  for (int li = 1; li <= 4; ++li) {
    const int planes = planes_of[li - 1];
    const std::string base = C + "feats.layer" + std::to_string(li) + ".";
    x = basic_block(s, x, cin, base + "0.", planes, stride_of[li - 1], 1, cin != planes || stride_of[li - 1] != 1);
    Act *into = nullptr;
    if (li == 4) {          // the last block writes straight into its slot of the PSP concatenation
      cat = s.act(x->lv, 2560);
      into = slice(s, cat, 2048, 512);
    }
    x = basic_block(s, x, planes, base + "1.", planes, 1, dil_of[li - 1], false, into);
    cin = planes;
  }
  const Level *l8 = cat->lv;  // the 1/8-resolution level
  // PSP module (lib/pspnet.py:20-24): pool -> 1x1 conv -> bilinear (align_corners=False) into the concat slots.  The pooled maps of
  // every frame of every bucket sit in ONE set of stage blocks ([4][B*36][512], frames in bucket order): the four stage convolutions are
  // single GEMMs; pooling and resampling (and their adjoints) run per bucket
  Act *feat = x;           // == cat[:, 2048:2560]
  float *pyr = s.f((size_t)4 * B * 36 * 512);
  if (s.live())
    for (int i = 0; i < nb; ++i)
      launch_psp_pool(feat->v.d + l8->off[i] * feat->v.ld, feat->v.ld, 0, pyr, l8->B[i], l8->H[i], l8->W[i], 512, s.st, B, l8->b0[i]);
  struct Stages { Act *pooled[4], *z[4]; };
  auto stg = std::make_shared<Stages>();
  const std::vector<BTab> tabs8 = make_tabs(l8);
  s.tape.push_back([=](Step &s) {          // (pushed first: runs after the four stage convolutions' backward) the pooling adjoint of all stages, all buckets
    const bool acc = s.grad_of(feat);
    Ptr4 dy;
    for (int si = 0; si < 4; ++si) dy.p[si] = stg->pooled[si]->g.d;
    if (s.live())
      for (const BTab &t : tabs8)
        hipLaunchKernelGGL(pool_bwd_all_kernel, dim3(nblk(tab_rows(t) * 128)), dim3(TB), 0, s.st, dy, feat->g.d, feat->g.ld, 128, acc ? 1 : 0, t);
  });
  for (int si = 0; si < 4; ++si) {
    const int sz = si == 0 ? 1 : si == 1 ? 2 : si == 2 ? 3 : 6;
    stg->pooled[si] = s.act((long)B * sz * sz, 512, pyr + (size_t)si * B * 36 * 512, 512);
    stg->z[si] = conv(s, stg->pooled[si], 512, ConvW{C + "psp.stages." + std::to_string(si) + ".1.weight"}, 512, 1, 1, 0, 1, ACT_NONE);
  }
  {
    Ptr4 z;
    for (int si = 0; si < 4; ++si) z.p[si] = stg->z[si]->v.d;
    if (s.live())
      for (const BTab &t : tabs8)
        hipLaunchKernelGGL(bilinear_fwd_all_kernel, dim3(nblk(tab_rows(t) * 4 * 128)), dim3(TB), 0, s.st, z, cat->v.d, cat->v.ld, 128, t);
  }
  s.tape.push_back([=](Step &s) {          // (runs before the stage convolutions' backward) the four resampling adjoints in one launch
    MPtr4 dz;
    for (int si = 0; si < 4; ++si) { s.grad_of(stg->z[si]); dz.p[si] = stg->z[si]->g.d; }
    if (s.live())
      for (const BTab &t : tabs8)
        hipLaunchKernelGGL(bilinear_bwd_all_kernel, dim3((unsigned)std::min<long>((long)tab_frames(t) * 50 * 16, 65535L * 16)), dim3(TB), 0, s.st, cat->g.d, cat->g.ld,
                           dz, tab_frames(t), 128, t);
  });
  // the concat's gradient buffer is one allocation; layer4's output gradient is its last 512 channels
  s.tape.push_back([=](Step &) { alias_grad(feat, cat, 2048); });
  Act *psp = conv(s, cat, 2560, ConvW{C + "psp.bottleneck.weight", 0, C + "psp.bottleneck.bias"}, 1024, 1, 1, 0, 1, ACT_RELU);
  if (io.dropout) psp = dropout2d(s, psp, 0.3f, io.seed * 4 + 1);
  Act *u1 = upconv(s, psp, C + "up_1.", 1024, 256);
  if (io.dropout) u1 = dropout2d(s, u1, 0.15f, io.seed * 4 + 2);
  Act *u2 = upconv(s, u1, C + "up_2.", 256, 64);
  if (io.dropout) u2 = dropout2d(s, u2, 0.15f, io.seed * 4 + 3);
  // up_3 + final 1x1 + LogSoftmax at the chosen pixels only (lib/network.py:98-102 reads nothing else)
  Act *patch = s.act((long)rows, 576);
  const Level *l2 = u2->lv;   // half resolution
  if (s.live())
    for (int i = 0; i < nb; ++i)
      launch_up3_patches(u2->v.d + l2->off[i] * 64, io.choose + (size_t)l2->b0[i] * N, patch->v.d + (size_t)l2->b0[i] * Npad * 576, l2->B[i], l2->H[i], l2->W[i], N,
                         Npad, s.st);
  s.tape.push_back([=](Step &s) {
    s.grad_of(u2);
    int hmax = 0, wmax = 0;
    for (int i = 0; i < nb; ++i) { hmax = std::max(hmax, l2->H[i]); wmax = std::max(wmax, l2->W[i]); }
    for (const BTab &t : make_tabs(l2)) {
      const int fr = tab_frames(t), f0 = t.b0[0];
      const size_t mark = s.off;
      int4 *tabo = reinterpret_cast<int4 *>(s.bytes((size_t)fr * N * sizeof(int4)));
      int *rowlist = reinterpret_cast<int *>(s.bytes((size_t)fr * hmax * N * sizeof(int)));
      int *rowcnt = reinterpret_cast<int *>(s.bytes((size_t)fr * hmax * sizeof(int)));
      if (s.live()) {
        hipLaunchKernelGGL(up3_decode_multi_kernel, dim3(nblk((long)fr * N)), dim3(TB), 0, s.st, io.choose + (size_t)f0 * N, tabo, fr, N, t);
        hipLaunchKernelGGL(up3_rowlist_multi_kernel, dim3(hmax, fr), dim3(TB), 0, s.st, tabo, rowlist, rowcnt, hmax, N, t);
        hipLaunchKernelGGL(up3_patch_bwd_multi_kernel, dim3((wmax + TB / 16 - 1) / (TB / 16), hmax, fr), dim3(TB), 0, s.st, patch->g.d + (size_t)f0 * Npad * 576, tabo,
                           rowlist, rowcnt, u2->g.d, hmax, N, Npad, t);
      }
      s.off = mark;
    }
  });
  Act *z3 = conv(s, patch, 576, ConvW{C + "up_3.conv.1.weight", 0, C + "up_3.conv.1.bias", 0, C + "up_3.conv.2.weight"}, 64, 1, 1, 0, 1, ACT_PRELU);
  Act *emb_pm = s.act((long)rows, 32);
  float *emb = io.emb ? io.emb : s.f((size_t)B * 32 * N);
  if (s.live()) {
    hipMemsetAsync(emb_pm->v.d, 0, (size_t)rows * 32 * sizeof(float), s.st);      // rows n >= N feed e_conv1: keep them finite
    launch_final_logsoftmax(z3->v.d, s.p(C + "final.0.weight"), s.p(C + "final.0.bias"), emb, emb_pm->v.d, B, N, Npad, s.st);
  }
  s.tape.push_back([=](Step &s) {
    // LogSoftmax adjoint on the log-probabilities, then the 1x1 conv 64 -> 32 as a GEMM over the chosen pixels' rows
    float *dlog = s.f((size_t)rows * 32);
    if (s.live()) s.fail(df_logsoftmax(emb_pm->g.d, emb_pm->v.d, dlog, rows, 32, 1, s.st));
    Act lg;
    lg.lv = z3->lv; lg.C = 32; lg.v.d = nullptr; lg.v.ld = 32;
    ConvParams f = flat_params(z3, 64, s.p(C + "final.0.weight"), nullptr, &lg, ACT_NONE);
    gemm_bwd(s, f, View{dlog, 32}, z3, C + "final.0.weight", C + "final.0.bias");
  });

  // ---- PoseNetFeat (lib/network.py:53-68) on point rows padded to Npad per frame: pf = [x1 64 | e1 64 | x2 128 | e2 128] ----
  const PointFeat pf = point_feat(s, io.cloud, emb_pm, B, true);
  Act *pf2 = slice(s, pf.all, 128, 256);
  Act *x5 = conv(s, pf2, 256, ConvW{"feat.conv5.weight", 0, "feat.conv5.bias"}, 512, 1, 1, 0, 1, ACT_RELU);
  Act *ap = conv6_mean(s, x5, B);
  ap->g = View{s.f((size_t)B * 1024), 1024};      // its gradient, allocated here: head layer 1's backward writes it, no producer asks grad_of

  // ---- heads (lib/network.py:107-131): layer 1 with the global feature folded into a per-frame bias, towers stacked r, t, c ----
  float *gbias = s.f((size_t)B * 1920), *s1 = s.f((size_t)B * 1920);
  if (s.live()) launch_fc_rows(ap->v.d, 1024, 0, s.p("head1.wg"), s.p("head1.bias"), gbias, 1920, B, 1024, 1920, 1, 0, s.st);
  Act *h1 = s.act((long)rows, 1920);
  ConvParams p1 = flat_params(pf.all, 384, s.p("head1.wpt"), gbias, h1, ACT_RELU);
  p1.rows_per_group = Npad; p1.rows_valid = N; p1.bias_group_ld = 1920;
  s.gemm(GK_FWD, p1);
  s.tape.push_back([=](Step &s) {
    launch_act_bwd(s, h1, ACT_RELU, nullptr, nullptr);
    gemm_bwd(s, p1, h1->g, pf.all, "head1.wpt", "");
    alias_slices(pf);
    alias_grad(pf2, pf.all, 128);
    if (s.live()) {
      hipLaunchKernelGGL(colsum_obj_kernel, dim3(1920 / 32, B), dim3(256), 0, s.st, h1->g.d, 1920, s1, Npad, 1920, (long)rows);
      hipLaunchKernelGGL(head1_global_wgrad_kernel, dim3(nblk((long)1920 * 256)), dim3(TB), 0, s.st, s1, ap->v.d, s.gr("head1.wg"), s.gr("head1.bias"), B, 1920, 256);
    }
    {
      ConvParams q;
      q.in = s1; q.B = B; q.Cin = 1920; q.in_ld = 1920;
      q.wgt = s.pf("head1.wg");
      q.out = ap->g.d; q.Cout = 1024; q.out_ld = 1024;
      s.with_splitk(q);
      s.gemm(GK_DGRAD, q);
    }
  });
  Act *h2 = s.act((long)rows, 768), *h3 = s.act((long)rows, 384);
  auto towers = [&](Act *in, int cin_t, Act *out, int cout_t, const std::string &wname, const std::string &bname) {
    ConvParams p = flat_params(in, cin_t, s.p(wname), s.p(bname), out, ACT_RELU);
    p.Cout = cout_t;
    p.zcount = 3; p.z_in_coff = cin_t; p.z_wgt = (long)cout_t * cin_t; p.z_bias = cout_t; p.z_out_coff = cout_t;
    s.gemm(GK_FWD, p);
    s.tape.push_back([=](Step &s) {
      launch_act_bwd(s, out, ACT_RELU, nullptr, nullptr);
      gemm_bwd(s, p, out->g, in, wname, bname);
    });
  };
  towers(h1, 640, h2, 256, "head2.w", "head2.bias");
  towers(h2, 256, h3, 128, "head3.w", "head3.bias");
  float *out_r = io.out_r ? io.out_r : s.f((size_t)B * N * 4), *out_t = io.out_t ? io.out_t : s.f((size_t)B * N * 3);
  float *out_c = io.out_c ? io.out_c : s.f((size_t)B * N);
  if (s.live())
    launch_head_final(h3->v.d, s.p("conv4_r.weight"), s.p("conv4_r.bias"), s.p("conv4_t.weight"), s.p("conv4_t.bias"), s.p("conv4_c.weight"),
                      s.p("conv4_c.bias"), io.obj, t.K, out_r, out_t, out_c, B, N, Npad, s.st);
  // ---- loss (lib/loss.py:13-70), one frame at a time like the reference, and its gradient w.r.t. the predictions ----
  float *d_r = s.f((size_t)B * N * 4), *d_t = s.f((size_t)B * N * 3), *d_c = s.f((size_t)B * N);
  float *dis_n = s.f((size_t)B * N);
  int *sel = reinterpret_cast<int *>(s.bytes((size_t)B * N * io.M * sizeof(int)));
  float *np = io.new_points ? io.new_points : s.f((size_t)B * N * 3), *nt = io.new_target ? io.new_target : s.f((size_t)B * io.M * 3);
  if (s.live()) {      // all frames of the pass in a handful of launches (csrc/loss.h), frame by frame the arithmetic of df_loss_forward / _backward
    s.fail(launch_loss_frames(B, io.symmetric, out_r, out_t, out_c, io.target, io.model_points, io.cloud, N, io.M, io.w, io.loss, io.dis, np, nt, dis_n, sel,
                              s.st));
    s.fail(launch_loss_bwd_frames(B, io.symmetric, out_r, out_t, out_c, io.target, io.model_points, io.cloud, sel, dis_n, N, io.M, io.w, 1.f, d_r, d_t, d_c,
                                  s.st));
  }
  s.dbg("forward + loss");
  // ---- backward: the last head layer by hand, then the tape in reverse ----
  {
    s.grad_of(h3);
    float *dz = s.f((size_t)B * N * 8);
    const int chunks = (N + 127) / 128;
    float *part = s.f((size_t)B * chunks * 8 * 128), *zpart = s.f((size_t)B * chunks * 8);
    if (s.live()) {
      hipLaunchKernelGGL(head_final_bwd_kernel, dim3(nblk((long)rows * 96)), dim3(TB), 0, s.st, d_r, d_t, d_c, out_c, s.p("conv4_r.weight"), s.p("conv4_t.weight"),
                         s.p("conv4_c.weight"), io.obj, t.K, h3->g.d, dz, B, N, Npad);
      hipLaunchKernelGGL(head_final_wgrad_kernel, dim3(chunks, B), dim3(TB), 0, s.st, dz, h3->v.d, part, zpart, N, Npad, chunks);
      hipLaunchKernelGGL(head_final_wgrad_finish_kernel, dim3(4), dim3(TB), 0, s.st, part, zpart, io.obj, t.K, s.gr("conv4_r.weight"), s.gr("conv4_r.bias"),
                         s.gr("conv4_t.weight"), s.gr("conv4_t.bias"), s.gr("conv4_c.weight"), s.gr("conv4_c.bias"), B, N, chunks);
    }
  }
  run_tape(s);
}

// ------------------------------------------------------------------------------------------------
// PoseRefineNet step (lib/network.py:151-206 + lib/loss_refiner.py:12-62): one refine iteration of B frames
// ------------------------------------------------------------------------------------------------
struct RefinerIO {
  int B, M;
  const float *points, *emb, *target, *model_points;      // [B][N][3], [B][32][N], [B][M][3], [B][M][3]
  const int64_t *obj;
  const int *symmetric;
  float *dis, *new_points, *new_target;                   // [B], [B][N][3], [B][M][3]
};

void refiner_step(Step &s, const RefinerIO &io) {
  Trainer &t = *s.t;
  const int B = io.B, N = t.N, Npad = round_up(N, 128), rows = B * Npad;
  s.take_splitk((size_t)8 << 20);
  Act *emb_pm = s.act((long)rows, 32);
  if (s.live()) {
    hipMemsetAsync(emb_pm->v.d, 0, (size_t)rows * 32 * sizeof(float), s.st);
    launch_emb_to_pm(io.emb, emb_pm->v.d, B, N, Npad, s.st);
  }
  const PointFeat pf = point_feat(s, io.points, emb_pm, B, false);      // pointfeat_3 (lib/network.py:160-163); the embedding is an input here
  // conv5 reads all 384 channels: its data gradient is the first writer of pf's gradient buffer
  Act *x5 = s.act((long)rows, 512);
  {
    ConvParams p5 = flat_params(pf.all, 384, s.p("feat.conv5.weight"), s.p("feat.conv5.bias"), x5, ACT_RELU);
    s.gemm(GK_FWD, p5);
    s.tape.push_back([=](Step &s) {
      launch_act_bwd(s, x5, ACT_RELU, nullptr, nullptr);
      gemm_bwd(s, p5, x5->g, pf.all, "feat.conv5.weight", "feat.conv5.bias");
      alias_slices(pf);
    });
  }
  Act *ap = conv6_mean(s, x5, B);          // (its gradient comes lazily from the FC towers' data gradients)
  // FC towers 1024 -> 512 -> 128 (lib/network.py:191-196), one row per frame; f2 = [r 128 | t 128]
  Act *f1 = s.act((long)B, 1024), *f2 = s.act((long)B, 256);
  Act *f1r = slice(s, f1, 0, 512), *f1t = slice(s, f1, 512, 512), *f2r = slice(s, f2, 0, 128), *f2t = slice(s, f2, 128, 128);
  conv(s, ap, 1024, ConvW{"conv1_r.weight", 0, "conv1_r.bias"}, 512, 1, 1, 0, 1, ACT_RELU, nullptr, f1r);
  conv(s, ap, 1024, ConvW{"conv1_t.weight", 0, "conv1_t.bias"}, 512, 1, 1, 0, 1, ACT_RELU, nullptr, f1t);
  conv(s, f1r, 512, ConvW{"conv2_r.weight", 0, "conv2_r.bias"}, 128, 1, 1, 0, 1, ACT_RELU, nullptr, f2r);
  conv(s, f1t, 512, ConvW{"conv2_t.weight", 0, "conv2_t.bias"}, 128, 1, 1, 0, 1, ACT_RELU, nullptr, f2t);
  float *out_r = s.f((size_t)B * 4), *out_t = s.f((size_t)B * 3), *d_r = s.f((size_t)B * 4), *d_t = s.f((size_t)B * 3);
  if (s.live())
    hipLaunchKernelGGL(refiner_tail_fwd_kernel, dim3(B), dim3(64), 0, s.st, f2->v.d, s.p("conv3_r.weight"), s.p("conv3_r.bias"), s.p("conv3_t.weight"),
                       s.p("conv3_t.bias"), io.obj, t.K, out_r, out_t, B);
  int *sel = reinterpret_cast<int *>(s.bytes((size_t)B * io.M * sizeof(int)));
  if (s.live()) {      // all frames in a handful of launches (csrc/loss.h)
    s.fail(launch_loss_refine_frames(B, io.symmetric, out_r, out_t, io.target, io.model_points, io.points, N, io.M, io.dis, io.new_points, io.new_target, sel,
                                     s.st));
    s.fail(launch_loss_refine_bwd_frames(B, io.symmetric, out_r, out_t, io.target, io.model_points, sel, io.M, 1.f, d_r, d_t, s.st));
  }
  {
    s.grad_of(f2);
    alias_grad(f2r, f2, 0); alias_grad(f2t, f2, 128);            // (written just below by the tail's backward)
    s.grad_of(f1);
    alias_grad(f1r, f1, 0, false); alias_grad(f1t, f1, 512, false);      // (each tower's data gradient is the first writer of its half)
    if (s.live())
      hipLaunchKernelGGL(refiner_tail_bwd_kernel, dim3(1), dim3(128), 0, s.st, d_r, d_t, f2->v.d, s.p("conv3_r.weight"), s.p("conv3_t.weight"), io.obj, t.K,
                         f2->g.d, s.gr("conv3_r.weight"), s.gr("conv3_r.bias"), s.gr("conv3_t.weight"), s.gr("conv3_t.bias"), B);
  }
  run_tape(s);
}

Trainer *as_trainer(df_trainer *h) { return reinterpret_cast<Trainer *>(h); }
const Trainer *as_trainer(const df_trainer *h) { return reinterpret_cast<const Trainer *>(h); }

}  // namespace
}  // namespace df

using namespace df;

extern "C" df_trainer *df_trainer_create(int kind, int num_points, int num_obj) {
  if ((kind != 0 && kind != 1) || num_points <= 0 || num_obj <= 0) { set_error(DF_ERR_ARG, "trainer_create: bad arguments"); return nullptr; }
  Trainer *t = new Trainer();
  t->kind = kind; t->N = num_points; t->K = num_obj;
  hipGetDevice(&t->device);
  t->params = reference_params(kind, num_obj);
  lay_out(*t);
  // the data gradients' flipped / transposed weight copies; without a device (layout / workspace queries on a CPU-only host) the
  // handle still works for everything that launches nothing, and a step reports the missing arena
  if (hipMalloc(&t->wflip, t->flat * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); t->wflip = nullptr; }
  if (t->wino_floats && hipMalloc(&t->wino_buf, t->wino_floats * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); t->wino_buf = nullptr; }
  {
    std::vector<FlipTile> tiles;
    long tb = 0;
    for (const Trainer::Flip &f : t->flips) {
      const int nb_n = (f.O + 31) / 32, nb_c = (f.I + 31) / 32;
      tiles.push_back(FlipTile{(long)f.off, (int)tb, f.O, f.T, f.I, f.KH, f.KW, f.Z, nb_n, nb_c});
      tb += (long)f.Z * f.T * nb_n * nb_c;
    }
    t->flip_ntiles = (int)tb;
    if (t->wflip && !tiles.empty() && tb < (1L << 31) && hipMalloc(&t->flip_tiles, tiles.size() * sizeof(FlipTile)) == hipSuccess)
      hipMemcpy(t->flip_tiles, tiles.data(), tiles.size() * sizeof(FlipTile), hipMemcpyHostToDevice);
    else { (void)hipGetLastError(); t->flip_tiles = nullptr; }
  }
  return reinterpret_cast<df_trainer *>(t);
}

extern "C" void df_trainer_destroy(df_trainer *h) {
  if (!h) return;
  Trainer *t = as_trainer(h);
  if (t->wflip) hipFree(t->wflip);
  if (t->wino_buf) hipFree(t->wino_buf);
  if (t->flip_tiles) hipFree(t->flip_tiles);
  delete t;
}

extern "C" int64_t df_trainer_flat_numel(const df_trainer *h) { return h ? (int64_t)as_trainer(h)->flat : 0; }
extern "C" int df_trainer_num_params(const df_trainer *h) { return h ? (int)as_trainer(h)->params.spec.size() : 0; }

extern "C" int df_trainer_param_info(const df_trainer *h, int i, char *key_out, int key_cap, int64_t *shape4, int *ndim) {
  if (!h) return set_error(DF_ERR_ARG, "trainer_param_info: null handle");
  return as_trainer(h)->params.info(i, key_out, key_cap, shape4, ndim, "trainer_param_info");
}

// dir 0: reference layout (`ref`, device) -> its place in the flat kernel-layout buffer; dir 1: back
static int relayout(const Trainer &t, const char *key, float *ref, float *flat, int dir, hipStream_t st) {
  if (!key || !ref || !flat) return set_error(DF_ERR_ARG, "trainer pack/unpack: null pointer");
  const int at = t.params.find(key);
  if (at < 0) return set_error(DF_ERR_ARG, "trainer pack/unpack: unexpected key '%s'", key);
  const ParamInfo &p = t.params.spec[at];
  const Place &q = t.place[at];
  if (q.mode == PLACE_CONV || q.mode == PLACE_TAPMAJOR) {
    const int O = (int)p.shape[0], I = (int)p.shape[1], T = (int)(p.shape[2] * p.shape[3]), Ipad = q.mode == PLACE_CONV ? (I + 3) / 4 * 4 : I;
    hipLaunchKernelGGL(relayout_kernel, dim3(nblk((long)O * T * Ipad, 2048)), dim3(TB), 0, st, dir == 0 ? ref : flat + q.off, dir == 0 ? flat + q.off : ref, O, I, T,
                       Ipad, q.mode, dir);
  } else if (q.mode == PLACE_HEAD1) {       // [640][1408] <-> [640][384] + [640][1024]
    if (dir == 0) {
      hipLaunchKernelGGL(copy2d_kernel, dim3(nblk(640L * 384)), dim3(TB), 0, st, ref, 1408L, flat + q.off, 384L, 640L, 384L);
      hipLaunchKernelGGL(copy2d_kernel, dim3(nblk(640L * 1024)), dim3(TB), 0, st, ref + 384, 1408L, flat + q.off2, 1024L, 640L, 1024L);
    } else {
      hipLaunchKernelGGL(copy2d_kernel, dim3(nblk(640L * 384)), dim3(TB), 0, st, flat + q.off, 384L, ref, 1408L, 640L, 384L);
      hipLaunchKernelGGL(copy2d_kernel, dim3(nblk(640L * 1024)), dim3(TB), 0, st, flat + q.off2, 1024L, ref + 384, 1408L, 640L, 1024L);
    }
  } else {
    const long n = (long)p.numel();
    hipLaunchKernelGGL(copy2d_kernel, dim3(nblk(n)), dim3(TB), 0, st, dir == 0 ? ref : flat + q.off, n, dir == 0 ? flat + q.off : ref, n, 1L, n);
  }
  return check_launch("trainer pack/unpack");
}

extern "C" int df_trainer_pack_param(const df_trainer *h, const char *key, const float *src, float *flat, df_stream_t stream) {
  if (!h) return set_error(DF_ERR_ARG, "trainer_pack_param: null handle");
  return relayout(*as_trainer(h), key, const_cast<float *>(src), flat, 0, to_stream(stream));
}
extern "C" int df_trainer_unpack_param(const df_trainer *h, const char *key, const float *flat, float *dst, df_stream_t stream) {
  if (!h) return set_error(DF_ERR_ARG, "trainer_unpack_param: null handle");
  return relayout(*as_trainer(h), key, dst, const_cast<float *>(flat), 1, to_stream(stream));
}

static int posenet_buckets_ok(const Trainer *t, int nb, const int *B, const int *H, const int *W, int M, const char *what) {
  if (!t || t->kind != 0) return set_error(DF_ERR_ARG, "%s: not a PoseNet trainer", what);
  if (nb <= 0 || nb > 4096 || !B || !H || !W || M <= 0) return set_error(DF_ERR_ARG, "%s: need 1..4096 buckets with B / H / W arrays and M >= 1", what);
  long tot = 0;
  for (int i = 0; i < nb; ++i) {
    if (B[i] <= 0 || H[i] < 8 || W[i] < 8 || H[i] > DF_MAX_CROP || W[i] > DF_MAX_CROP)
      return set_error(DF_ERR_ARG, "%s: bucket %d: need B >= 1 and 8 <= H, W <= %d (got %d, %d, %d)", what, i, DF_MAX_CROP, B[i], H[i], W[i]);
    tot += B[i];
  }
  if (tot > 65535) return set_error(DF_ERR_ARG, "%s: too many frames in one pass (%ld)", what, tot);
  return DF_OK;
}

extern "C" size_t df_posenet_train_multi_workspace_bytes(const df_trainer *h, int nb, const int *B, const int *H, const int *W, int M) {
  if (!h || posenet_buckets_ok(as_trainer(h), nb, B, H, W, M, "posenet_train_workspace_bytes") != DF_OK) return 0;
  Trainer &t = *const_cast<Trainer *>(as_trainer(h));
  std::vector<int> key{nb, M};
  for (int i = 0; i < nb; ++i) { key.push_back(B[i]); key.push_back(H[i]); key.push_back(W[i]); }
  PoseNetIO io{};
  io.nb = nb; io.B = B; io.H = H; io.W = W; io.M = M; io.dropout = 1;
  return sized_workspace(t, key, [&](Step &s) { posenet_step(s, io); });
}

extern "C" size_t df_posenet_train_workspace_bytes(const df_trainer *h, int B, int H, int W, int M) {
  return df_posenet_train_multi_workspace_bytes(h, 1, &B, &H, &W, M);
}

extern "C" int df_posenet_train_step_multi(df_trainer *h, const float *flat_param, float *flat_grad, int64_t param_version, int nb, const int *B,
                                           const int *H, const int *W, const float *const *img, const float *cloud, const int64_t *choose,
                                           const int64_t *obj, const float *target, const float *model_points, int M, const int *symmetric_host,
                                           float w, int dropout, unsigned seed, float *loss_out, float *dis_out, float *new_points,
                                           float *new_target, float *out_r, float *out_t, float *out_c, float *emb, void *ws, size_t ws_bytes,
                                           df_stream_t stream) {
  if (!h) return set_error(DF_ERR_ARG, "posenet_train_step: null handle");
  int rc = posenet_buckets_ok(as_trainer(h), nb, B, H, W, M, "posenet_train_step");
  if (rc != DF_OK) return rc;
  if (!flat_param || !flat_grad || !img || !cloud || !choose || !obj || !target || !model_points || !loss_out || !dis_out || !ws)
    return set_error(DF_ERR_ARG, "posenet_train_step: null pointer");
  for (int i = 0; i < nb; ++i)
    if (!img[i]) return set_error(DF_ERR_ARG, "posenet_train_step: bucket %d: null image pointer", i);
  Trainer &t = *as_trainer(h);
  if (df_posenet_train_multi_workspace_bytes(h, nb, B, H, W, M) > ws_bytes) return set_error(DF_ERR_WORKSPACE, "posenet_train_step: workspace too small");
  const PoseNetIO io{nb, B, H, W, img, M, cloud, target, model_points, choose, obj, symmetric_host, w, dropout, seed, loss_out, dis_out, new_points,
                     new_target, out_r, out_t, out_c, emb};
  return run_step(t, flat_param, flat_grad, param_version, ws, ws_bytes, stream, "posenet_train_step", [&](Step &s) { posenet_step(s, io); });
}

extern "C" int df_posenet_train_step(df_trainer *h, const float *flat_param, float *flat_grad, int64_t param_version, int B, int H, int W,
                                     const float *img, const float *cloud, const int64_t *choose, const int64_t *obj, const float *target,
                                     const float *model_points, int M, const int *symmetric_host, float w, int dropout, unsigned seed,
                                     float *loss_out, float *dis_out, float *new_points, float *new_target, float *out_r, float *out_t,
                                     float *out_c, float *emb, void *ws, size_t ws_bytes, df_stream_t stream) {
  return df_posenet_train_step_multi(h, flat_param, flat_grad, param_version, 1, &B, &H, &W, &img, cloud, choose, obj, target, model_points, M,
                                     symmetric_host, w, dropout, seed, loss_out, dis_out, new_points, new_target, out_r, out_t, out_c, emb, ws, ws_bytes,
                                     stream);
}

// Split-K of the small-grid forward / data-gradient launches (on by default: +4-8 % on one-frame passes).  Off: every output element is
// summed in ONE order whatever the grid, so the gradient of a frame no longer depends on which other frames share its pass (up to the
// weight gradients' own pixel order): what the equality tests of the multi-bucket pass switch off.
extern "C" int df_trainer_set_splitk(df_trainer *h, int enable) {
  if (!h) return set_error(DF_ERR_ARG, "trainer_set_splitk: null handle");
  as_trainer(h)->splitk = enable != 0;
  return DF_OK;
}

// Profile of the MFMA launches of the steps run on this handle since df_trainer_profile(h, 1): HIP events bracket every forward /
// data-gradient / weight-gradient GEMM on the launch stream; the FLOPs are those the launches EXECUTE (2 M N K of the shapes really run:
// low-resolution up-convolutions, folded head layer 1, chosen-pixel up_3, F(4x4,3x3)-domain products), not the reference graph's.
extern "C" int df_trainer_profile(df_trainer *h, int enable) {
  if (!h) return set_error(DF_ERR_ARG, "trainer_profile: null handle");
  as_trainer(h)->timer.arm(enable != 0);
  return DF_OK;
}

// after a stream sync: per kind (0 forward, 1 data gradient, 2 weight gradient) the summed launch durations (ms), executed FLOPs, launches
extern "C" int df_trainer_profile_read(df_trainer *h, double *ms3, double *flops3, int *launches3) {
  if (!h || !ms3 || !flops3 || !launches3) return set_error(DF_ERR_ARG, "trainer_profile_read: null pointer");
  LaunchTimer &tm = as_trainer(h)->timer;
  LaunchSum k3[3];
  static const char *const tags[3] = {"[df-train-gemm] fwd  ", "[df-train-gemm] dgrad", "[df-train-gemm] wgrad"};   // DF_PROFILE_VERBOSE
  const int rc = tm.sum(k3, [](const LaunchRecord &r) { return r.kind; }, tags, "trainer_profile_read");
  for (int k = 0; k < 3; ++k) { ms3[k] = k3[k].ms; flops3[k] = k3[k].flops; launches3[k] = k3[k].launches; }
  if (rc != DF_OK) return rc;
  tm.rec.clear();                    // re-arm
  return DF_OK;
}

extern "C" size_t df_refiner_train_workspace_bytes(const df_trainer *h, int B, int M) {
  if (!h || as_trainer(h)->kind != 1 || B <= 0 || M <= 0) return 0;
  Trainer &t = *const_cast<Trainer *>(as_trainer(h));
  RefinerIO io{};
  io.B = B; io.M = M;
  return sized_workspace(t, {B, M}, [&](Step &s) { refiner_step(s, io); });
}

extern "C" int df_refiner_train_step(df_trainer *h, const float *flat_param, float *flat_grad, int64_t param_version, int B, const float *points,
                                     const float *emb, const int64_t *obj, const float *target, const float *model_points, int M,
                                     const int *symmetric_host, float *dis_out, float *new_points, float *new_target, void *ws, size_t ws_bytes,
                                     df_stream_t stream) {
  if (!h || as_trainer(h)->kind != 1) return set_error(DF_ERR_ARG, "refiner_train_step: not a PoseRefineNet trainer");
  if (B <= 0 || M <= 0) return set_error(DF_ERR_ARG, "refiner_train_step: need B >= 1, M >= 1");
  if (!flat_param || !flat_grad || !points || !emb || !obj || !target || !model_points || !dis_out || !new_points || !new_target || !ws)
    return set_error(DF_ERR_ARG, "refiner_train_step: null pointer");
  Trainer &t = *as_trainer(h);
  if (df_refiner_train_workspace_bytes(h, B, M) > ws_bytes) return set_error(DF_ERR_WORKSPACE, "refiner_train_step: workspace too small");
  const RefinerIO io{B, M, points, emb, target, model_points, obj, symmetric_host, dis_out, new_points, new_target};
  return run_step(t, flat_param, flat_grad, param_version, ws, ws_bytes, stream, "refiner_train_step", [&](Step &s) { refiner_step(s, io); });
}
