// Host-side engine of libdfusion_hip.so: parameter store in kernel-friendly layouts, workspace
// planning, and the launch sequences of PoseNet.forward / PoseRefineNet.forward / the fused
// "estimate poses" pipeline (PoseNet -> per-pixel selection -> refine loop), all on one stream with
// no host synchronisation, no allocation and no host<->device copies inside a forward call.
//
// Reference behaviour mirrored: lib/network.py:95-132 (PoseNet.forward), :187-206
// (PoseRefineNet.forward), lib/pspnet.py:64-77, lib/extractors.py:114-124, tools/eval_ycb.py:192-229.
// Batch extension: the reference evaluates one object per call (b = 0 hard-coded, network.py:123);
// every entry point here takes B same-sized objects and evaluates them independently.
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "host_plan.h"
#include "igemm.h"
#include "layers.h"
#include "wino.h"
#include "pose.h"

namespace df {

// ------------------------------------------------------------------------------------------------
// parameter store
// ------------------------------------------------------------------------------------------------
struct Net {
  int kind = 0;   // 0 = PoseNet, 1 = PoseRefineNet
  int num_points = 0, num_obj = 0;
  ParamList params;                     // reference keys and shapes (host_plan.h)
  std::vector<char> loaded;
  std::map<std::string, float *> buf;   // packed device buffers by internal name
  int device = 0;
  LaunchTimer timer;                    // df_net_profile (bench.py roofline): every launch_conv, bf16 x 6 launches flagged
  // bf16 x 6 weight planes (csrc/split_gemm.hip) of every buffer a routed layer reads, by the buffer's address: term p of w[i] at
  // ptr[p * stride + i].  Allocated by the first ensure_derived, cut again by the first one after any parameter load (after the PSP fold;
  // the Winograd-domain U and the tap-major copies are made at load), freed by df_net_destroy: the launch path only looks them up
  struct Planes { long elems = 0, stride = 0; void *ptr = nullptr; };
  std::map<const float *, Planes> planes;
  bool planes_dirty = true;
  // debug taps (df_net_debug_taps): copies of named intermediates of the last single-bucket forward, channels-last
  bool psp_dirty = false;               // a psp.* weight changed since the folded matrices were built
  // parameter uploads are enqueued on the null stream WITHOUT host synchronisation (one staging buffer, no per-tensor malloc /
  // free / sync); the next forward call waits for them once (check_ready)
  bool upload_pending = false;
  float *stage = nullptr;
  size_t stage_cap = 0;
  bool taps_on = false;
  struct Tap { float *buf = nullptr; size_t cap = 0; int64_t shape[4] = {0, 0, 0, 0}; };
  std::map<std::string, Tap> taps;
};

static float *dev_alloc(Net &n, const std::string &name, size_t floats) {
  auto it = n.buf.find(name);
  if (it != n.buf.end()) return it->second;
  float *p = nullptr;
  if (hipMalloc(&p, floats * sizeof(float)) != hipSuccess) return nullptr;
  hipMemset(p, 0, floats * sizeof(float));
  n.buf[name] = p;
  return p;
}

// OIHW -> O (H W) Ipad
__global__ void pack_oihw_kernel(const float *__restrict__ src, float *__restrict__ dst, int O, int I, int HW, int Ipad) {
  const long total = (long)O * HW * Ipad;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % Ipad);
    const long r = i / Ipad;
    const int t = (int)(r % HW);
    const long o = r / HW;
    dst[i] = c < I ? src[(o * I + c) * HW + t] : 0.f;
  }
}

// psp fold (load time): wc[s][m][i] = sum_o wb[m][512 s + o] * ws[s][o][i], accumulated in fp64 and
// rounded once, so the folded weights carry no more error than a single fp32 rounding
__global__ void psp_fold_kernel(const float *__restrict__ wb, const float *__restrict__ ws, float *__restrict__ wc, int s) {
  const int i = blockIdx.x * 256 + threadIdx.x;          // 0..511
  const int m = blockIdx.y;
  if (i >= 512) return;
  double acc = 0.0;
  for (int o = 0; o < 512; ++o) acc += (double)wb[(size_t)m * 2560 + s * 512 + o] * (double)ws[(size_t)o * 512 + i];
  wc[((size_t)s * 1024 + m) * 512 + i] = (float)acc;
}

// copies `src` (device, reference layout) into the packed store
static int load_param(Net &n, const std::string &key, const float *src, int64_t numel) {
  const int at = n.params.find(key);
  if (at < 0) return set_error(DF_ERR_ARG, "load_param: unexpected key '%s'", key.c_str());
  const ParamInfo &pi = n.params.spec[at];
  if (numel != pi.numel())
    return set_error(DF_ERR_ARG, "load_param: size mismatch for %s: got %lld elements, expected %lld", key.c_str(),
                     (long long)numel, (long long)pi.numel());
  if (!src) return set_error(DF_ERR_ARG, "load_param: null pointer for %s", key.c_str());
  hipSetDevice(n.device);
  n.upload_pending = true;
  auto copy = [&](float *dst, const float *s, size_t cnt) { return hipMemcpyAsync(dst, s, cnt * sizeof(float), hipMemcpyDefault, 0); };
  auto copy2d = [&](float *dst, size_t dld, const float *s, size_t sld, size_t width, size_t rows) {
    return hipMemcpy2DAsync(dst, dld * sizeof(float), s, sld * sizeof(float), width * sizeof(float), rows, hipMemcpyDefault, 0);
  };
  hipError_t e = hipSuccess;
  if (pi.ndim == 4 && !ends_with(key, "classifier.0.weight")) {
    const int O = (int)pi.shape[0], I = (int)pi.shape[1], HW = (int)(pi.shape[2] * pi.shape[3]);
    const int Ipad = (I + 3) / 4 * 4;
    float *dst = dev_alloc(n, key, (size_t)O * HW * Ipad);
    if (!dst) return set_error(DF_ERR_LAUNCH, "load_param: hipMalloc failed");
    if (HW == 1 && Ipad == I) e = copy(dst, src, (size_t)numel);
    else {
      // src may be a host pointer: stage through the net's device staging buffer (grown on demand; stream order keeps a tensor's
      // pack kernel ahead of the next tensor's copy into the same buffer)
      if (n.stage_cap < (size_t)numel) {
        if (n.stage) { hipStreamSynchronize(0); hipFree(n.stage); }
        n.stage = nullptr; n.stage_cap = 0;
        if (hipMalloc(&n.stage, (size_t)numel * sizeof(float)) != hipSuccess) return set_error(DF_ERR_LAUNCH, "hipMalloc failed");
        n.stage_cap = (size_t)numel;
      }
      e = copy(n.stage, src, (size_t)numel);
      hipLaunchKernelGGL(pack_oihw_kernel, dim3(256), dim3(256), 0, 0, n.stage, dst, O, I, HW, Ipad);
    }
    if (e == hipSuccess && key.find("feats.layer") != std::string::npos && HW == 9 && I >= 128 && I % 4 == 0 && O % 4 == 0) {
      // stride-1 3x3 convs of layer2 .. layer4 may run in the Winograd domain (wino_route decides per map size): transformed copies
      // [16][O][I] for F(2x2,3x3) and [36][O][I] for F(4x4,3x3), fp64 math
      float *U = dev_alloc(n, key + ".wino", (size_t)16 * O * I), *U4 = dev_alloc(n, key + ".wino4", (size_t)36 * O * I);
      if (!U || !U4) return set_error(DF_ERR_LAUNCH, "load_param: hipMalloc failed");
      launch_wino_weight(dst, U, O, I, 0, 2);
      launch_wino_weight(dst, U4, O, I, 0, 4);
    }
    if (e == hipSuccess && (key.find(".up_1.") != std::string::npos || key.find(".up_2.") != std::string::npos) && HW == 9) {
      // up_1 / up_2 run as low-resolution 1x1 products per tap: keep a tap-major copy [9][O][I] (up_3 runs as a plain
      // [576]-deep GEMM on chosen-pixel patches and uses the packed layout as is)
      float *tm = dev_alloc(n, key + ".tm", (size_t)9 * O * I);
      if (!tm) return set_error(DF_ERR_LAUNCH, "load_param: hipMalloc failed");
      launch_tapmajor(dst, tm, O, I, 0);
    }
  } else if (n.kind == 0 && key.rfind("conv1_", 0) == 0) {
    // head layer 1 of tower h: split [640][1408] into the per-point part (first 384 input channels =
    // pointfeat_1|pointfeat_2) and the broadcast global-feature part (last 1024), towers stacked r,t,c
    const int h = key[6] == 'r' ? 0 : key[6] == 't' ? 1 : 2;
    if (ends_with(key, ".weight")) {
      float *wpt = dev_alloc(n, "head1.wpt", (size_t)1920 * 384), *wg = dev_alloc(n, "head1.wg", (size_t)1920 * 1024);
      if (!wpt || !wg) return set_error(DF_ERR_LAUNCH, "hipMalloc failed");
      e = copy2d(wpt + (size_t)h * 640 * 384, 384, src, 1408, 384, 640);
      if (e == hipSuccess) e = copy2d(wg + (size_t)h * 640 * 1024, 1024, src + 384, 1408, 1024, 640);
    } else {
      float *b = dev_alloc(n, "head1.bias", 1920);
      e = copy(b + h * 640, src, 640);
    }
  } else if (n.kind == 0 && (key.rfind("conv2_", 0) == 0 || key.rfind("conv3_", 0) == 0)) {
    const int l = key[4] - '0';
    const int h = key[6] == 'r' ? 0 : key[6] == 't' ? 1 : 2;
    const int co = l == 2 ? 256 : 128, ci = l == 2 ? 640 : 256;
    const std::string nm = std::string("head") + std::to_string(l);
    if (ends_with(key, ".weight")) e = copy(dev_alloc(n, nm + ".w", (size_t)3 * co * ci) + (size_t)h * co * ci, src, (size_t)co * ci);
    else e = copy(dev_alloc(n, nm + ".bias", 3 * co) + h * co, src, co);
  } else if (n.kind == 1 && (key.rfind("conv1_", 0) == 0 || key.rfind("conv2_", 0) == 0)) {
    const int l = key[4] - '0';
    const int h = key[6] == 'r' ? 0 : 1;
    const int co = l == 1 ? 512 : 128, ci = l == 1 ? 1024 : 512;
    const std::string nm = std::string("fc") + std::to_string(l);
    if (ends_with(key, ".weight")) e = copy(dev_alloc(n, nm + ".w", (size_t)2 * co * ci) + (size_t)h * co * ci, src, (size_t)co * ci);
    else e = copy(dev_alloc(n, nm + ".bias", 2 * co) + h * co, src, co);
  } else {
    float *dst = dev_alloc(n, key, (size_t)numel);
    if (!dst) return set_error(DF_ERR_LAUNCH, "load_param: hipMalloc failed");
    e = copy(dst, src, (size_t)numel);
  }
  if (e == hipSuccess && n.kind == 1 && key == "feat.conv5.weight") {
    // PoseRefineNetFeat.conv5 reads [x1 | e1 | x2 | e2] (lib/network.py:160-163); the colour half (e1, e2) does not change
    // between refine iterations, so its product is formed once per object: split the columns into an xyz part
    // [512][x1 64 | x2 128] and a colour part [512][e1 64 | e2 128] (the engine keeps the point features in that order)
    const float *w5 = n.buf[key];
    float *wx = dev_alloc(n, "feat.conv5.wx", (size_t)512 * 192), *we = dev_alloc(n, "feat.conv5.we", (size_t)512 * 192);
    if (!wx || !we) return set_error(DF_ERR_LAUNCH, "load_param: hipMalloc failed");
    e = copy2d(wx, 192, w5, 384, 64, 512);
    if (e == hipSuccess) e = copy2d(wx + 64, 192, w5 + 128, 384, 128, 512);
    if (e == hipSuccess) e = copy2d(we, 192, w5 + 64, 384, 64, 512);
    if (e == hipSuccess) e = copy2d(we + 64, 192, w5 + 256, 384, 128, 512);
  }
  if (e != hipSuccess) return set_error(DF_ERR_LAUNCH, "load_param(%s): %s", key.c_str(), hipGetErrorString(e));
  n.loaded[at] = 1;
  // the folded PSP matrices depend on five tensors: rebuilt once, by the next forward call (ensure_derived), not per key
  if (n.kind == 0 && key.find(".psp.") != std::string::npos && !ends_with(key, ".bias")) n.psp_dirty = true;
  return DF_OK;
}

// The engine's plain-GEMM weights: every buffer a 1x1 / per-point / Winograd-domain launch reads, with the launches' (N, K, epilogue kind).
// Those of layers split_route takes get bf16 planes; the launch path (Ctx::conv) finds them by address and fails on a routed launch
// whose buffer has none, so this table and the launches cannot drift apart silently.
struct GemmWeight { std::string name; int N, K, epi; };
static std::vector<GemmWeight> gemm_weights(const Net &n) {
  std::vector<GemmWeight> v;
  const std::string P = CNN;
  if (n.kind == 0) {
    v.push_back({"psp.fold.w", 1024, 512, GEMM_EPI_PLAIN});
    v.push_back({"psp.fold.wfeat", 1024, 512, GEMM_EPI_RESIDUAL});
    v.push_back({P + "up_1.conv.1.weight.tm", 9 * 256, 1024, GEMM_EPI_PLAIN});
    v.push_back({P + "up_2.conv.1.weight.tm", 9 * 64, 256, GEMM_EPI_PLAIN});
    v.push_back({P + "up_3.conv.1.weight", 64, 576, GEMM_EPI_PLAIN});
    for (const ParamInfo &pi : n.params.spec)
      if (pi.key.find("feats.layer") != std::string::npos && pi.ndim == 4) {
        const int O = (int)pi.shape[0], I = (int)pi.shape[1];
        if (pi.shape[2] * pi.shape[3] == 1) v.push_back({pi.key, O, I, GEMM_EPI_PLAIN});          // downsample.0 (1x1)
        else {
          v.push_back({pi.key + ".wino", O, I, GEMM_EPI_PLAIN});
          v.push_back({pi.key + ".wino4", O, I, GEMM_EPI_PLAIN});
        }
      }
    v.push_back({"feat.conv5.weight", 512, 256, GEMM_EPI_PLAIN});
    v.push_back({"head1.wpt", 1920, 384, GEMM_EPI_GROUPS});
    v.push_back({"head1.wpt", 640, 384, GEMM_EPI_GROUPS});       // (the confidence tower alone: pose selection)
    v.push_back({"head2.w", 256, 640, GEMM_EPI_PLAIN});
    v.push_back({"head3.w", 128, 256, GEMM_EPI_PLAIN});
  } else {
    v.push_back({"feat.conv5.we", 512, 192, GEMM_EPI_PLAIN});
    v.push_back({"feat.conv5.wx", 512, 192, GEMM_EPI_RESIDUAL});
  }
  v.push_back({"feat.e_conv1.weight", 64, 32, GEMM_EPI_PLAIN});
  v.push_back({"feat.conv2.weight", 128, 64, GEMM_EPI_PLAIN});
  v.push_back({"feat.e_conv2.weight", 128, 64, GEMM_EPI_PLAIN});
  v.push_back({"feat.conv6.weight", 1024, 512, GEMM_EPI_GROUPS});
  return v;
}

// element count of a packed buffer (the planes cover it whole: launches read sub-ranges and z batches of it)
static long buffer_elems(const Net &n, const std::string &name) {
  const std::string P = CNN;
  auto spec_of = [&](const std::string &key) -> const ParamInfo * {
    const int at = n.params.find(key);
    return at < 0 ? nullptr : &n.params.spec[at];
  };
  if (name == "psp.fold.w") return 4L * 1024 * 512;
  if (name == "psp.fold.wfeat") return 1024L * 512;
  if (name == "head1.wpt") return 1920L * 384;
  if (name == "head2.w") return 3L * 256 * 640;
  if (name == "head3.w") return 3L * 128 * 256;
  if (name == "feat.conv5.we" || name == "feat.conv5.wx") return 512L * 192;
  const bool wino = ends_with(name, ".wino"), wino4 = ends_with(name, ".wino4"), tm = ends_with(name, ".tm");
  const std::string key = wino ? name.substr(0, name.size() - 5) : wino4 ? name.substr(0, name.size() - 6) : tm ? name.substr(0, name.size() - 3) : name;
  const ParamInfo *pi = spec_of(key);
  if (!pi) return 0;
  const long O = pi->shape[0], I = pi->shape[1], HW = pi->ndim == 4 ? pi->shape[2] * pi->shape[3] : 1;
  if (wino) return 16 * O * I;
  if (wino4) return 36 * O * I;
  if (tm) return 9 * O * I;
  return O * HW * ((I + 3) / 4 * 4);          // packed O (H W) Ipad
}

// (re)cut the planes of every routed layer's buffer on the null stream (after the uploads and the PSP fold, in stream order)
static int cut_planes(Net &n) {
  for (const GemmWeight &g : gemm_weights(n)) {
    if (!split_route(g.N, g.K, g.epi)) continue;
    auto it = n.buf.find(g.name);
    const long elems = buffer_elems(n, g.name);
    if (it == n.buf.end() || elems <= 0) return set_error(DF_ERR_STATE, "weight planes: no packed buffer '%s'", g.name.c_str());
    Net::Planes &pl = n.planes[it->second];
    if (!pl.ptr) {
      pl.elems = elems;
      pl.stride = (elems + 63) / 64 * 64;
      if (hipMalloc(&pl.ptr, (size_t)pl.stride * 3 * 2) != hipSuccess) {
        pl.ptr = nullptr;
        return set_error(DF_ERR_LAUNCH, "weight planes of '%s': hipMalloc failed", g.name.c_str());
      }
      hipMemset(pl.ptr, 0, (size_t)pl.stride * 3 * 2);
    }
    cut_weight_planes(it->second, pl.ptr, pl.elems, pl.stride, 0);
  }
  if (check_launch("weight planes") != DF_OK) return DF_ERR_LAUNCH;
  return DF_OK;
}

// (re)build what is derived from several parameters: the PSP fold (bottleneck x stage weights, fp64 accumulation), then the bf16 planes
static int ensure_derived(Net &n) {
  if (!n.psp_dirty) {
    if (n.planes_dirty) {
      const int rc = cut_planes(n);
      if (rc != DF_OK) return rc;
      n.planes_dirty = false;
      n.upload_pending = true;
    }
    if (n.upload_pending) {               // the uploads of df_net_load_param ran on the null stream: one wait per batch of loads
      if (hipStreamSynchronize(0) != hipSuccess) return set_error(DF_ERR_LAUNCH, "parameter upload failed: %s", hipGetErrorString(hipGetLastError()));
      n.upload_pending = false;
    }
    return DF_OK;
  }
  const std::string P = CNN;
  float *wc = dev_alloc(n, "psp.fold.w", (size_t)4 * 1024 * 512), *wf = dev_alloc(n, "psp.fold.wfeat", (size_t)1024 * 512);
  if (!wc || !wf) return set_error(DF_ERR_LAUNCH, "psp fold: hipMalloc failed");
  const float *wb = n.buf[P + "psp.bottleneck.weight"];
  hipMemcpy2DAsync(wf, 512 * sizeof(float), wb + 2048, 2560 * sizeof(float), 512 * sizeof(float), 1024, hipMemcpyDeviceToDevice, 0);
  for (int st = 0; st < 4; ++st)
    hipLaunchKernelGGL(psp_fold_kernel, dim3(2, 1024, 1), dim3(256), 0, 0, wb, n.buf[P + "psp.stages." + std::to_string(st) + ".1.weight"], wc, st);
  if (check_launch("psp fold") != DF_OK) return DF_ERR_LAUNCH;
  n.psp_dirty = false;
  n.upload_pending = true;
  return ensure_derived(n);            // the planes (cut from the folded matrices too), then one wait
}

static int check_ready(const Net &n0) {
  Net &n = const_cast<Net &>(n0);
  for (size_t i = 0; i < n.params.spec.size(); ++i)
    if (!n.loaded[i]) return set_error(DF_ERR_STATE, "parameter '%s' was never loaded", n.params.spec[i].key.c_str());
  return ensure_derived(n);
}

// ------------------------------------------------------------------------------------------------
// forward plumbing
// ------------------------------------------------------------------------------------------------
// one forward call: the workspace arena (host_plan.h; scratch regions are released and reused, see conv3x3) and the net's launch stream
struct Ctx : Arena {
  Net *net;
  hipStream_t st;

  Ctx(Net *n, hipStream_t s, Arena a = Arena()) : Arena(a), net(n), st(s) {}
  const float *w(const std::string &name) {
    auto it = net->buf.find(name);
    if (it == net->buf.end()) {
      if (err == DF_OK) err = set_error(DF_ERR_STATE, "missing packed parameter '%s'", name.c_str());
      return nullptr;
    }
    return it->second;
  }
  // `useful`: the fraction of the launch's rows that are not padding (points beyond N in a 128-padded object block, Winograd
  // tiles beyond the map edge) -- only for the profile's useful-FLOP tally
  // debug tap: keep a copy of an intermediate (allocates: debug mode only, never under graph capture)
  void tap(const char *name, const float *src, int64_t d0, int64_t d1, int64_t d2, int64_t d3) {
    if (!live() || !net->taps_on || !src) return;
    Net::Tap &t = net->taps[name];
    const size_t n = (size_t)d0 * d1 * d2 * d3;
    if (t.cap < n) {
      if (t.buf) hipFree(t.buf);
      t.buf = nullptr; t.cap = 0;
      if (hipMalloc(&t.buf, n * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return; }
      t.cap = n;
    }
    t.shape[0] = d0; t.shape[1] = d1; t.shape[2] = d2; t.shape[3] = d3;
    hipMemcpyAsync(t.buf, src, n * sizeof(float), hipMemcpyDeviceToDevice, st);
  }
  double pt_useful = 1.0;      // N / Npad of the per-point launches
  void pconv(const ConvParams &p) { conv(p, pt_useful); }
  void conv(const ConvParams &p, double useful = 1.0) {
    if (!live()) return;
    Net &n = *net;
    if (n.timer.on) {
      fail(n.timer.begin(st));
      if (!live()) return;
    }
    ConvParams pc = p;
    if (p.KH * p.KW == 1 && split_route(p.Cout, p.Cin, gemm_epi_kind(p))) {
      // a routed layer: its weights' bf16 planes, cut at load (ensure_derived); looked up, never made, here
      const long extent = (long)(p.zcount - 1) * p.z_wgt + (long)p.Cout * p.Cin;
      auto it = n.planes.upper_bound(p.wgt);
      const Net::Planes *pl = nullptr;
      if (it != n.planes.begin()) {
        --it;
        if (p.wgt >= it->first && p.wgt + extent <= it->first + it->second.elems && (p.wgt - it->first) % 8 == 0) pl = &it->second;
      }
      if (!pl) {
        if (err == DF_OK) err = set_error(DF_ERR_STATE, "routed GEMM N=%d K=%d: its weights have no bf16 planes", p.Cout, p.Cin);
        return;
      }
      pc.wpl = reinterpret_cast<const char *>(pl->ptr) + (p.wgt - it->first) * 2;
      pc.wpl_stride = pl->stride;
    }
    ConvRoute taken;
    const int rc = launch_conv(pc, st, &taken);
    if (n.timer.on) {
      LaunchRecord r = launch_record(0, conv_flops(p), p);
      r.bytes = conv_bytes(p);
      r.useful = r.flops * useful;
      r.bf16 = taken.kernel == CONV_BF16;
      n.timer.end(st, r);
    }
    if (rc != DF_OK) err = rc;
  }
};

// dev switch (A/B runs): DF_POINT_UNFUSED = the K = 3 / 32 / 64 per-point layers as separate launches (round 2) instead of pointfeat.hip
static bool point_fused() {
  static const bool on = df::dev_getenv("DF_POINT_UNFUSED") == nullptr;
  return on;
}

// dev switches (A/B runs): DF_NO_WINOGRAD = direct convolutions only, DF_WINOGRAD_TILE = 2 keeps F(2x2,3x3) where a Winograd route pays
static int wino_route_for(int H, int W, int dil, int ci, int co) {
  static const bool off = df::dev_getenv("DF_NO_WINOGRAD") != nullptr;
  static const int force = df::dev_getenv("DF_WINOGRAD_TILE") ? atoi(df::dev_getenv("DF_WINOGRAD_TILE")) : 0;
  if (off) return 0;
  const int r = wino_route(H, W, dil, ci, co);
  return (r && force == 2) ? 2 : r;
}

static ConvParams point_gemm(const float *in, int in_ld, int in_coff, int cin, const float *w, const float *bias,
                             float *out, int out_ld, int out_coff, int cout, int rows, int act) {
  ConvParams p;
  p.in = in; p.wgt = w; p.bias = bias; p.out = out;
  p.B = rows; p.H = p.W = p.OH = p.OW = 1;
  p.Cin = cin; p.in_ld = in_ld; p.in_coff = in_coff;
  p.Cout = cout; p.out_ld = out_ld; p.out_coff = out_coff;
  p.act = act;
  return p;
}

static ConvParams conv2d(const float *in, int B, int H, int W, int cin, int in_ld, const float *w, const float *bias,
                         float *out, int OH, int OW, int cout, int out_ld, int out_coff, int k, int stride, int pad,
                         int dil, int act) {
  ConvParams p;
  p.in = in; p.wgt = w; p.bias = bias; p.out = out;
  p.B = B; p.H = H; p.W = W; p.OH = OH; p.OW = OW;
  p.Cin = cin; p.in_ld = in_ld; p.Cout = cout; p.out_ld = out_ld; p.out_coff = out_coff;
  p.KH = p.KW = k; p.stride = stride; p.pad = pad; p.dil = dil; p.act = act;
  return p;
}


struct PoseNetOut {
  float *out_r, *out_t, *out_c, *emb;   // caller buffers
  float *emb_pm = nullptr;              // [B][Npad][32] inside the workspace
};

// One crop-size bucket of a call: B same-sized objects.  A call evaluates a list of buckets: every launch whose arithmetic does
// not depend on the crop geometry (1x1 convs, the Winograd-domain products, the low-resolution up-conv products and the whole
// per-point part) runs ONCE over the rows of all buckets; only the direct kxk convolutions and the memory-bound glue kernels
// (transforms, pooling, interpolation) are launched per bucket, writing into / reading from the shared row-concatenated buffers.
struct Grp { int B, H, W; const float *img; };

// PSPNet colour branch (lib/pspnet.py:64-77 on top of lib/extractors.py:114-124) up to up_2's output: returns the concatenated
// half-resolution 64-channel maps and their level
static float *cnn_forward(Ctx &c, const std::vector<Grp> &gs, Level &half_lv) {
  const std::string P = CNN;
  const int nb = (int)gs.size();
  Level l0, l1;          // stem output, max-pool output
  for (const Grp &g : gs) {
    const int H1 = conv_out(g.H, 7, 2, 3, 1), W1 = conv_out(g.W, 7, 2, 3, 1);
    l0.push(g.B, H1, W1);
    l1.push(g.B, conv_out(H1, 3, 2, 1, 1), conv_out(W1, 3, 2, 1, 1));
  }
  float *x = c.f((size_t)l1.rows * 64);
  {
    const size_t mark = c.off;     // img4 / stem are dead after the pooling: their region is reused by the layers below
    for (int i = 0; i < nb; ++i) {
      const Grp &g = gs[i];
      float *img4 = c.f((size_t)g.B * g.H * g.W * 4);
      if (c.live()) launch_nchw3_to_nhwc4(g.img, img4, g.B, g.H, g.W, c.st);
      float *stem = c.f((size_t)g.B * l0.H[i] * l0.W[i] * 64);
      c.conv(conv2d(img4, g.B, g.H, g.W, 4, 4, c.w(P + "feats.conv1.weight"), nullptr, stem, l0.H[i], l0.W[i], 64, 64, 0, 7, 2, 3, 1, ACT_RELU));
      if (c.live()) launch_maxpool3s2(stem, x + l1.off[i] * 64, g.B, l0.H[i], l0.W[i], 64, l1.H[i], l1.W[i], c.st);
      if (nb == 1) c.tap("stem", stem, g.B, l0.H[i], l0.W[i], 64);
    }
    c.off = mark;
    (void)mark;
  }

  // conv3x3 (+ residual) + ReLU over all buckets: buckets whose geometry makes the Winograd-domain product pay share ONE z-batched
  // GEMM over the concatenation of their tiles (per-bucket transforms around it); the others run the direct implicit GEMM
  auto conv3x3 = [&](const float *in, const Level &li, int ci, const std::string &key, float *out, const Level &lo, int co, int stride, int dil,
                     const float *res) {
    std::vector<int> ws[2];        // buckets on the F(2x2) / F(4x4) route
    for (int i = 0; i < nb; ++i) {
      const int route = stride == 1 ? wino_route_for(li.H[i], li.W[i], dil, ci, co) : 0;
      if (route) { ws[route == 4].push_back(i); continue; }
      ConvParams p = conv2d(in + li.off[i] * ci, gs[i].B, li.H[i], li.W[i], ci, ci, c.w(key), nullptr, out + lo.off[i] * co, lo.H[i], lo.W[i], co,
                            co, 0, 3, stride, dil, dil, ACT_RELU);
      if (res) { p.res = res + lo.off[i] * co; p.res_ld = co; }
      c.conv(p);
    }
    for (int r = 0; r < 2; ++r) {
      if (ws[r].empty()) continue;       // (layers below 128 channels have no transformed weights to look up)
      const WinoPlan pl = wino_plan(li, ws[r], dil, r ? 4 : 2, true);
      wino_pass(c, c.st, pl, in, ci, ci, c.w(key + (r ? ".wino4" : ".wino")), out, co, co, res, co, ACT_RELU,
                [&](const ConvParams &p) { c.conv(p, pl.useful()); });
    }
  };

  Level lx = l1;
  int cin = 64;
  const int planes_of[4] = {64, 128, 256, 512}, stride_of[4] = {1, 2, 1, 1}, dil_of[4] = {1, 1, 2, 4};
  for (int li = 1; li <= 4; ++li) {
    const int planes = planes_of[li - 1], s = stride_of[li - 1], d = dil_of[li - 1];
    const std::string base = P + "feats.layer" + std::to_string(li) + ".";
    Level lo;
    for (int i = 0; i < nb; ++i) lo.push(gs[i].B, conv_out(lx.H[i], 3, s, 1, 1), conv_out(lx.W[i], 3, s, 1, 1));
    // block 0: built without dilation (lib/extractors.py:107); carries the stride and the 1x1 downsample
    float *t = c.f((size_t)lo.rows * planes);
    conv3x3(x, lx, cin, base + "0.conv1.weight", t, lo, planes, s, 1, nullptr);
    const float *res = x;
    if (cin != planes || s != 1) {
      float *ds = c.f((size_t)lo.rows * planes);
      if (s == 1) {     // a 1x1 stride-1 conv is a plain GEMM over pixel rows: one launch for all buckets
        c.conv(point_gemm(x, cin, 0, cin, c.w(base + "0.downsample.0.weight"), nullptr, ds, planes, 0, planes, (int)lo.rows, ACT_NONE));
      } else {
        for (int i = 0; i < nb; ++i)
          c.conv(conv2d(x + lx.off[i] * cin, gs[i].B, lx.H[i], lx.W[i], cin, cin, c.w(base + "0.downsample.0.weight"), nullptr, ds + lo.off[i] * planes,
                        lo.H[i], lo.W[i], planes, planes, 0, 1, s, 0, 1, ACT_NONE));
      }
      res = ds;
    }
    float *o0 = c.f((size_t)lo.rows * planes);
    conv3x3(t, lo, planes, base + "0.conv2.weight", o0, lo, planes, 1, 1, res);
    // block 1: dilated (lib/extractors.py:110)
    float *t1 = c.f((size_t)lo.rows * planes);
    conv3x3(o0, lo, planes, base + "1.conv1.weight", t1, lo, planes, 1, d, nullptr);
    float *o1 = c.f((size_t)lo.rows * planes);
    conv3x3(t1, lo, planes, base + "1.conv2.weight", o1, lo, planes, 1, d, o0);
    x = o1; lx = lo; cin = planes;
    if (nb == 1) c.tap(("layer" + std::to_string(li)).c_str(), x, gs[0].B, lx.H[0], lx.W[0], planes);
  }
  // PSP module (lib/pspnet.py:20-24) with the bottleneck folded through the pyramid:
  //   bottleneck(cat(up(W_s pool_s(f)), f)) = W_b[:,2048:] f + sum_s up((W_b[:,512s:512s+512] W_s) pool_s(f)) + b
  // (1x1 convs and bilinear resampling are linear and commute), so the 2560-channel concat is never built,
  // the big GEMM shrinks from K=2560 to K=512 and the four stage convs become one grouped launch on
  // 50 pooled rows per object with weights combined once at load time (psp_fold).
  float *prior = c.f((size_t)lx.rows * 1024);
  for (int i = 0; i < nb; ++i) {
    const int B = gs[i].B;
    float *pooled = c.f((size_t)4 * B * 36 * 512), *zst = c.f((size_t)4 * B * 36 * 1024);
    if (c.live()) launch_psp_pool(x + lx.off[i] * 512, 512, 0, pooled, B, lx.H[i], lx.W[i], 512, c.st);
    ConvParams p = point_gemm(pooled, 512, 0, 512, c.w("psp.fold.w"), nullptr, zst, 1024, 0, 1024, B * 36, ACT_NONE);
    p.zcount = 4; p.z_in_coff = (long)B * 36 * 512; p.z_wgt = 1024 * 512; p.z_out_coff = (long)B * 36 * 1024;
    c.conv(p);
    if (c.live()) launch_psp_prior_sum(zst, prior + lx.off[i] * 1024, B, lx.H[i], lx.W[i], 1024, c.st);
  }
  float *psp = c.f((size_t)lx.rows * 1024);
  {
    ConvParams p = point_gemm(x, 512, 0, 512, c.w("psp.fold.wfeat"), c.w(P + "psp.bottleneck.bias"), psp, 1024, 0, 1024, (int)lx.rows, ACT_RELU);
    p.res = prior; p.res_ld = 1024;
    c.conv(p);
  }
  if (nb == 1) c.tap("psp", psp, gs[0].B, lx.H[0], lx.W[0], 1024);
  // PSPUpsample stages up_1, up_2 (lib/pspnet.py:27-37,69-73; dropout = identity in eval), each as a low-resolution
  // GEMM with N = 9*Cout (one launch for all buckets) followed by the per-bucket 9-tap interpolation (layers.hip).  up_3 is NOT run
  // here: its output is read at the chosen pixels only, so the caller evaluates it there from the maps returned: [B][h][w][64].
  float *cur = psp;
  const char *ups[2] = {"up_1", "up_2"};
  const int up_in[2] = {1024, 256}, up_out[2] = {256, 64};
  for (int u = 0; u < 2; ++u) {
    const size_t mark = c.off;
    float *o = c.f((size_t)4 * lx.rows * up_out[u]);
    const size_t keep = c.off;
    float *y = c.f((size_t)lx.rows * 9 * up_out[u]);
    c.conv(point_gemm(cur, up_in[u], 0, up_in[u], c.w(P + ups[u] + ".conv.1.weight.tm"), nullptr, y, 9 * up_out[u], 0, 9 * up_out[u], (int)lx.rows,
                      ACT_NONE));
    Level lo;
    for (int i = 0; i < nb; ++i) lo.push(gs[i].B, 2 * lx.H[i], 2 * lx.W[i]);
    for (int i = 0; i < nb; ++i)
      if (c.live()) {
        const int rc = launch_upconv_gather(y + lx.off[i] * 9 * up_out[u], c.w(P + ups[u] + ".conv.1.bias"), c.w(P + ups[u] + ".conv.2.weight"),
                                            o + lo.off[i] * up_out[u], gs[i].B, lx.H[i], lx.W[i], up_out[u], c.st);
        if (rc != DF_OK) c.err = rc;
      }
    c.off = keep;        // the tap products are dead once interpolated
    (void)mark;
    lx = lo;
    cur = o;
    if (nb == 1) c.tap(ups[u], cur, gs[0].B, lx.H[0], lx.W[0], up_out[u]);
  }
  half_lv = lx;
  return cur;
}

// PoseNetFeat + heads (lib/network.py:53-68,107-131) on point-major rows padded to Npad per object
// `sel` non-null (eval loop): only the confidence tower runs over all points; the r / t towers are evaluated at the
// arg-max point alone (launch_head_select), which also writes the pose record -- out_r / out_t / out_c stay untouched.
struct SelectOut { double *pose_wo, *state; float *rt; };

static void posenet_points(Ctx &c, int B, int N, int Npad, const float *cloud, const float *emb_pm, const int64_t *obj,
                           float *out_r, float *out_t, float *out_c, const SelectOut *sel = nullptr) {
  Net &n = *c.net;
  const int rows = B * Npad;
  float *pf = c.f((size_t)rows * 384);          // [x1 64 | e1 64 | x2 128 | e2 128] = pointfeat_1 | pointfeat_2
  if (point_fused()) {        // conv1 -> conv2 and e_conv1 -> e_conv2 chained in one launch, the 64-wide intermediates in LDS
    PointFeatParams q;
    q.cloud = cloud; q.emb = emb_pm; q.pf = pf; q.ld = 384; q.cx1 = 0; q.ce1 = 64; q.cx2 = 128; q.ce2 = 256;
    q.w1 = c.w("feat.conv1.weight"); q.b1 = c.w("feat.conv1.bias"); q.w2 = c.w("feat.conv2.weight"); q.b2 = c.w("feat.conv2.bias");
    q.we1 = c.w("feat.e_conv1.weight"); q.be1 = c.w("feat.e_conv1.bias"); q.we2 = c.w("feat.e_conv2.weight"); q.be2 = c.w("feat.e_conv2.bias");
    q.B = B; q.N = N; q.Npad = Npad;
    if (c.live()) { const int rc = launch_pointfeat(q, c.st); if (rc != DF_OK) c.err = rc; }
  } else {
    if (c.live()) launch_cloud_conv1(cloud, nullptr, c.w("feat.conv1.weight"), c.w("feat.conv1.bias"), pf, 384, B, N, Npad, c.st);
    c.pconv(point_gemm(emb_pm, 32, 0, 32, c.w("feat.e_conv1.weight"), c.w("feat.e_conv1.bias"), pf, 384, 64, 64, rows, ACT_RELU));
    c.pconv(point_gemm(pf, 384, 0, 64, c.w("feat.conv2.weight"), c.w("feat.conv2.bias"), pf, 384, 128, 128, rows, ACT_RELU));
    c.pconv(point_gemm(pf, 384, 64, 64, c.w("feat.e_conv2.weight"), c.w("feat.e_conv2.bias"), pf, 384, 256, 128, rows, ACT_RELU));
  }
  if (!sel) c.tap("pf", pf, B, Npad, 384, 1);
  float *x5 = c.f((size_t)rows * 512);
  c.pconv(point_gemm(pf, 384, 128, 256, c.w("feat.conv5.weight"), c.w("feat.conv5.bias"), x5, 512, 0, 512, rows, ACT_RELU));
  if (!sel) c.tap("x5", x5, B, Npad, 512, 1);
  // conv6 + ReLU + AvgPool1d(N): the 1024-wide activation is consumed only by the mean, so it never
  // leaves the GEMM's registers -- per-wave column sums, then a tiny deterministic reduction
  ConvParams p6 = point_gemm(x5, 512, 0, 512, c.w("feat.conv6.weight"), c.w("feat.conv6.bias"), nullptr, 1024, 0, 1024, rows, ACT_RELU);
  p6.rows_per_group = Npad; p6.rows_valid = N;
  const int prow = conv_colsum_rows(p6);
  float *partial = c.f((size_t)prow * 1024);
  p6.colsum = partial;
  c.pconv(p6);
  float *apx = c.f((size_t)B * 1024);
  if (c.live()) launch_colsum_finish(partial, prow / B, apx, B, 1024, N, c.st);
  c.tap("ap_x", apx, B, 1024, 1, 1);
  // head layer 1: W[:, :384] . pointfeat + (W[:, 384:] . ap_x + b) -- the 1024 broadcast channels of the
  // 1408-wide input are identical for every point of an object, so they collapse into a per-object bias
  float *gbias = c.f((size_t)B * 1920);
  if (c.live()) launch_fc_rows(apx, 1024, 0, c.w("head1.wg"), c.w("head1.bias"), gbias, 1920, B, 1024, 1920, 1, 0, c.st);   // one row per object
  if (sel) {
    float *h1c = c.f((size_t)rows * 640), *h2c = c.f((size_t)rows * 256), *h3c = c.f((size_t)rows * 128), *conf = c.f((size_t)B * N);
    const float *w1 = c.w("head1.wpt"), *w2 = c.w("head2.w"), *b2 = c.w("head2.bias"), *w3 = c.w("head3.w"), *b3 = c.w("head3.bias");
    if (c.err != DF_OK) return;
    {
      ConvParams p = point_gemm(pf, 384, 0, 384, w1 + (size_t)2 * 640 * 384, gbias + 1280, h1c, 640, 0, 640, rows, ACT_RELU);
      p.rows_per_group = Npad; p.rows_valid = N; p.bias_group_ld = 1920;
      c.pconv(p);
    }
    c.pconv(point_gemm(h1c, 640, 0, 640, w2 + (size_t)2 * 256 * 640, b2 + 512, h2c, 256, 0, 256, rows, ACT_RELU));
    c.pconv(point_gemm(h2c, 256, 0, 256, w3 + (size_t)2 * 128 * 256, b3 + 256, h3c, 128, 0, 128, rows, ACT_RELU));
    if (c.live())
      launch_head_select(h3c, c.w("conv4_c.weight"), c.w("conv4_c.bias"), pf, gbias, w1, w2, b2, w3, b3, c.w("conv4_r.weight"),
                         c.w("conv4_r.bias"), c.w("conv4_t.weight"), c.w("conv4_t.bias"), obj, n.num_obj, cloud, B, N, Npad, conf, sel->pose_wo,
                         sel->state, sel->rt, nullptr, c.st);
    return;
  }
  float *h1 = c.f((size_t)rows * 1920);
  {
    ConvParams p = point_gemm(pf, 384, 0, 384, c.w("head1.wpt"), gbias, h1, 1920, 0, 1920, rows, ACT_RELU);
    p.rows_per_group = Npad; p.rows_valid = N; p.bias_group_ld = 1920;
    c.pconv(p);
  }
  c.tap("h1", h1, B, Npad, 1920, 1);
  float *h2 = c.f((size_t)rows * 768), *h3 = c.f((size_t)rows * 384);
  {
    ConvParams p = point_gemm(h1, 1920, 0, 640, c.w("head2.w"), c.w("head2.bias"), h2, 768, 0, 256, rows, ACT_RELU);
    p.zcount = 3; p.z_in_coff = 640; p.z_wgt = 256 * 640; p.z_bias = 256; p.z_out_coff = 256;
    c.pconv(p);
  }
  c.tap("h2", h2, B, Npad, 768, 1);
  {
    ConvParams p = point_gemm(h2, 768, 0, 256, c.w("head3.w"), c.w("head3.bias"), h3, 384, 0, 128, rows, ACT_RELU);
    p.zcount = 3; p.z_in_coff = 256; p.z_wgt = 128 * 256; p.z_bias = 128; p.z_out_coff = 128;
    c.pconv(p);
  }
  c.tap("h3", h3, B, Npad, 384, 1);
  if (c.live())
    launch_head_final(h3, c.w("conv4_r.weight"), c.w("conv4_r.bias"), c.w("conv4_t.weight"), c.w("conv4_t.bias"),
                      c.w("conv4_c.weight"), c.w("conv4_c.bias"), obj, n.num_obj, out_r, out_t, out_c, B, N, Npad, c.st);
}

static void posenet_forward(Ctx &c, const std::vector<Grp> &gs, const float *cloud, const int64_t *choose, const int64_t *obj, PoseNetOut &o,
                            const SelectOut *sel = nullptr) {
  const int N = c.net->num_points, Npad = round_up(N, 128);
  c.pt_useful = (double)N / Npad;
  int B = 0;
  for (const Grp &g : gs) B += g.B;
  Level hl;
  float *half = cnn_forward(c, gs, hl);     // up_2's outputs: half resolution, 64 channels, buckets concatenated
  // up_3 (bilinear x2 + conv3x3 + PReLU) at the chosen pixels: patch rows (per bucket: the only geometry-dependent step), then one
  // GEMM over the points of all objects with the PReLU fused, then the final 1x1 conv + LogSoftmax
  const std::string P = CNN;
  float *patch = c.f((size_t)B * Npad * 576), *z3 = c.f((size_t)B * Npad * 64);
  {
    long b0 = 0;
    for (size_t i = 0; i < gs.size(); ++i) {
      if (c.live())
        launch_up3_patches(half + hl.off[i] * 64, choose + b0 * N, patch + (size_t)b0 * Npad * 576, gs[i].B, hl.H[i], hl.W[i], N, Npad, c.st);
      b0 += gs[i].B;
    }
  }
  {
    ConvParams p = point_gemm(patch, 576, 0, 576, c.w(P + "up_3.conv.1.weight"), c.w(P + "up_3.conv.1.bias"), z3, 64, 0, 64, B * Npad, ACT_PRELU);
    p.prelu = c.w(P + "up_3.conv.2.weight");
    c.pconv(p);
  }
  if (gs.size() == 1) c.tap("up_3", z3, B, Npad, 64, 1);      // rows of the chosen pixels only
  o.emb_pm = c.f((size_t)B * Npad * 32);
  if (c.live()) launch_final_logsoftmax(z3, c.w(P + "final.0.weight"), c.w(P + "final.0.bias"), o.emb, o.emb_pm, B, N, Npad, c.st);
  posenet_points(c, B, N, Npad, cloud, o.emb_pm, obj, o.out_r, o.out_t, o.out_c, sel);
}

// PoseRefineNetFeat + FC towers (lib/network.py:151-168,187-204).  The emb branch (e_conv1/e_conv2) does
// not depend on the cloud, so `prepare` runs it once per object and `iterate` re-does only the xyz branch.
struct RefinerBufs { float *pf, *e5, *x5, *partial, *apx, *f1, *f2; int prow; };   // pf rows: [x1 64 | x2 128 | e1 64 | e2 128]

static RefinerBufs refiner_alloc(Ctx &c, int B, int N, int Npad) {
  RefinerBufs r;
  c.pt_useful = (double)N / Npad;
  const int rows = B * Npad;
  r.pf = c.f((size_t)rows * 384);
  r.e5 = c.f((size_t)rows * 512);
  r.x5 = c.f((size_t)rows * 512);
  ConvParams p6 = point_gemm(r.x5, 512, 0, 512, nullptr, nullptr, nullptr, 1024, 0, 1024, rows, ACT_RELU);
  p6.rows_per_group = Npad; p6.rows_valid = N;
  r.prow = conv_colsum_rows(p6);
  r.partial = c.f((size_t)r.prow * 1024);
  r.apx = c.f((size_t)B * 1024);
  r.f1 = c.f((size_t)B * 1024);
  r.f2 = c.f((size_t)B * 256);
  return r;
}

static void refiner_prepare(Ctx &c, const RefinerBufs &r, int B, int Npad, const float *emb_pm) {
  const int rows = B * Npad;
  if (point_fused()) {
    PointFeatParams q;
    q.emb = emb_pm; q.pf = r.pf; q.ld = 384; q.ce1 = 192; q.ce2 = 256;
    q.we1 = c.w("feat.e_conv1.weight"); q.be1 = c.w("feat.e_conv1.bias"); q.we2 = c.w("feat.e_conv2.weight"); q.be2 = c.w("feat.e_conv2.bias");
    q.B = B; q.N = c.net->num_points; q.Npad = Npad;
    if (c.live()) { const int rc = launch_pointfeat(q, c.st); if (rc != DF_OK) c.err = rc; }
  } else {
    c.pconv(point_gemm(emb_pm, 32, 0, 32, c.w("feat.e_conv1.weight"), c.w("feat.e_conv1.bias"), r.pf, 384, 192, 64, rows, ACT_RELU));
    c.pconv(point_gemm(r.pf, 384, 192, 64, c.w("feat.e_conv2.weight"), c.w("feat.e_conv2.bias"), r.pf, 384, 256, 128, rows, ACT_RELU));
  }
  // colour half of conv5 (+ its bias), once per object; the iterations add the xyz half and apply the ReLU
  c.pconv(point_gemm(r.pf, 384, 192, 192, c.w("feat.conv5.we"), c.w("feat.conv5.bias"), r.e5, 512, 0, 512, rows, ACT_NONE));
}

static void refiner_iterate(Ctx &c, const RefinerBufs &r, int B, int N, int Npad, const float *cloud, const float *rt,
                            const int64_t *obj, float *out_r, float *out_t, double *state, float *rt_next, double *pose_out) {
  const int rows = B * Npad;
  if (point_fused()) {
    PointFeatParams q;
    q.cloud = cloud; q.rt = rt; q.pf = r.pf; q.ld = 384; q.cx1 = 0; q.cx2 = 64;
    q.w1 = c.w("feat.conv1.weight"); q.b1 = c.w("feat.conv1.bias"); q.w2 = c.w("feat.conv2.weight"); q.b2 = c.w("feat.conv2.bias");
    q.B = B; q.N = N; q.Npad = Npad;
    if (c.live()) { const int rc = launch_pointfeat(q, c.st); if (rc != DF_OK) c.err = rc; }
  } else {
    if (c.live()) launch_cloud_conv1(cloud, rt, c.w("feat.conv1.weight"), c.w("feat.conv1.bias"), r.pf, 384, B, N, Npad, c.st);
    c.pconv(point_gemm(r.pf, 384, 0, 64, c.w("feat.conv2.weight"), c.w("feat.conv2.bias"), r.pf, 384, 64, 128, rows, ACT_RELU));
  }
  // (taps: every iteration overwrites them, so after a call they hold its last iteration)
  c.tap("rf_pf", r.pf, B, Npad, 384, 1);
  {
    ConvParams p = point_gemm(r.pf, 384, 0, 192, c.w("feat.conv5.wx"), nullptr, r.x5, 512, 0, 512, rows, ACT_RELU);
    p.res = r.e5; p.res_ld = 512;
    c.pconv(p);
  }
  c.tap("rf_x5", r.x5, B, Npad, 512, 1);
  ConvParams p6 = point_gemm(r.x5, 512, 0, 512, c.w("feat.conv6.weight"), c.w("feat.conv6.bias"), nullptr, 1024, 0, 1024, rows, ACT_RELU);
  p6.rows_per_group = Npad; p6.rows_valid = N; p6.colsum = r.partial;
  c.pconv(p6);
  if (c.live()) launch_colsum_finish(r.partial, r.prow / B, r.apx, B, 1024, N, c.st);
  c.tap("rf_apx", r.apx, B, 1024, 1, 1);
  // FC towers 1024 -> 512 -> 128 for r and t (lib/network.py:191-196): one row per object
  if (c.live()) {
    launch_fc_rows(r.apx, 1024, 0, c.w("fc1.w"), c.w("fc1.bias"), r.f1, 1024, B, 1024, 1024, 1, 1, c.st);
    launch_fc_rows(r.f1, 1024, 512, c.w("fc2.w"), c.w("fc2.bias"), r.f2, 256, B, 512, 128, 2, 1, c.st);
  }
  c.tap("rf_f1", r.f1, B, 1024, 1, 1);
  c.tap("rf_f2", r.f2, B, 256, 1, 1);
  if (c.live()) {
    launch_refiner_tail(r.f2, c.w("conv3_r.weight"), c.w("conv3_r.bias"), c.w("conv3_t.weight"), c.w("conv3_t.bias"), obj,
                        c.net->num_obj, out_r, out_t, state, rt_next, pose_out, B, c.st);
  }
}

static Net *as_net(df_net *h) { return reinterpret_cast<Net *>(h); }
static const Net *as_net(const df_net *h) { return reinterpret_cast<const Net *>(h); }

static int finish(Ctx &c, const char *what) {
  if (c.err != DF_OK) return c.err;
  return c.dry ? DF_OK : check_launch(what);
}

}  // namespace df

using namespace df;

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" df_net *df_posenet_create(int num_points, int num_obj) {
  if (num_points <= 0 || num_obj <= 0) { set_error(DF_ERR_ARG, "posenet_create: bad sizes"); return nullptr; }
  Net *n = new Net();
  n->kind = 0; n->num_points = num_points; n->num_obj = num_obj;
  hipGetDevice(&n->device);
  n->params = reference_params(0, num_obj);
  n->loaded.assign(n->params.spec.size(), 0);
  return reinterpret_cast<df_net *>(n);
}

extern "C" df_net *df_refiner_create(int num_points, int num_obj) {
  if (num_points <= 0 || num_obj <= 0) { set_error(DF_ERR_ARG, "refiner_create: bad sizes"); return nullptr; }
  Net *n = new Net();
  n->kind = 1; n->num_points = num_points; n->num_obj = num_obj;
  hipGetDevice(&n->device);
  n->params = reference_params(1, num_obj);
  n->loaded.assign(n->params.spec.size(), 0);
  return reinterpret_cast<df_net *>(n);
}

extern "C" void df_net_destroy(df_net *h) {
  if (!h) return;
  Net *n = as_net(h);
  for (auto &kv : n->planes) hipFree(kv.second.ptr);
  for (auto &kv : n->buf) hipFree(kv.second);
  if (n->stage) hipFree(n->stage);
  for (auto &kv : n->taps) if (kv.second.buf) hipFree(kv.second.buf);
  delete n;
}

extern "C" int df_net_num_params(const df_net *h) { return h ? (int)as_net(h)->params.spec.size() : 0; }

extern "C" int df_net_param_info(const df_net *h, int i, char *key_out, int key_cap, int64_t *shape4, int *ndim) {
  if (!h) return set_error(DF_ERR_ARG, "param_info: null handle");
  return as_net(h)->params.info(i, key_out, key_cap, shape4, ndim, "param_info");
}

extern "C" int df_net_load_param(df_net *h, const char *key, const float *ptr, int64_t numel) {
  if (!h || !key) return set_error(DF_ERR_ARG, "load_param: null handle/key");
  as_net(h)->planes_dirty = true;
  return load_param(*as_net(h), key, ptr, numel);
}

extern "C" int df_net_profile(df_net *h, int enable) {
  if (!h) return set_error(DF_ERR_ARG, "profile: null handle");
  as_net(h)->timer.arm(enable != 0);
  return DF_OK;
}

// after a stream sync: sum of the fp32-kernel GEMM launch durations (ms), their algorithmic FLOPs and count since df_net_profile(1)
// (the bf16 x 6 launches: df_net_profile_read_split, which must come first -- this call re-arms)
extern "C" int df_net_profile_read(df_net *h, double *gemm_ms, double *gemm_flops, double *gemm_useful_flops, double *gemm_bytes,
                                   int *launches) {
  if (!h) return set_error(DF_ERR_ARG, "profile_read: null handle");
  LaunchTimer &tm = as_net(h)->timer;
  LaunchSum s[2];
  static const char *const tags[2] = {"[df-gemm]", "[df-gemm-bf16]"};
  const int rc = tm.sum(s, [](const LaunchRecord &r) { return (int)r.bf16; }, tags, "profile_read");
  if (rc != DF_OK) return rc;
  if (gemm_ms) *gemm_ms = s[0].ms;
  if (gemm_flops) *gemm_flops = s[0].flops;
  if (gemm_useful_flops) *gemm_useful_flops = s[0].useful;
  if (gemm_bytes) *gemm_bytes = s[0].bytes;
  if (launches) *launches = s[0].launches;
  tm.rec.clear();                    // re-arm
  return DF_OK;
}

// after a stream sync: the same sums over the bf16 x 6 launches since df_net_profile(1); does not re-arm
extern "C" int df_net_profile_read_split(df_net *h, double *gemm_ms, double *gemm_flops, double *gemm_useful_flops, int *launches) {
  if (!h) return set_error(DF_ERR_ARG, "profile_read_split: null handle");
  LaunchSum s;
  const int rc = as_net(h)->timer.sum(&s, [](const LaunchRecord &r) { return r.bf16 ? 0 : -1; }, nullptr, "profile_read_split");
  if (rc != DF_OK) return rc;
  if (gemm_ms) *gemm_ms = s.ms;
  if (gemm_flops) *gemm_flops = s.flops;
  if (gemm_useful_flops) *gemm_useful_flops = s.useful;
  if (launches) *launches = s.launches;
  return DF_OK;
}

extern "C" int df_net_debug_taps(df_net *h, int enable) {
  if (!h) return set_error(DF_ERR_ARG, "debug_taps: null handle");
  Net *n = as_net(h);
  n->taps_on = enable != 0;
  if (!enable) {
    for (auto &kv : n->taps) if (kv.second.buf) hipFree(kv.second.buf);
    n->taps.clear();
  }
  return DF_OK;
}

extern "C" int df_net_debug_tap_read(df_net *h, const char *name, float *dst, int64_t cap, int64_t *shape4) {
  if (!h || !name) return set_error(DF_ERR_ARG, "debug_tap_read: null handle / name");
  Net *n = as_net(h);
  auto it = n->taps.find(name);
  if (it == n->taps.end() || !it->second.buf) return set_error(DF_ERR_STATE, "debug_tap_read: no tap named '%s' (arm df_net_debug_taps and run a single-bucket forward)", name);
  const Net::Tap &t = it->second;
  const int64_t numel = t.shape[0] * t.shape[1] * t.shape[2] * t.shape[3];
  if (shape4) for (int i = 0; i < 4; ++i) shape4[i] = t.shape[i];
  if (!dst) return DF_OK;          // shape query
  if (cap < numel) return set_error(DF_ERR_ARG, "debug_tap_read: destination holds %lld floats, tap '%s' has %lld", (long long)cap, name, (long long)numel);
  if (hipMemcpy(dst, t.buf, (size_t)numel * sizeof(float), hipMemcpyDefault) != hipSuccess) return set_error(DF_ERR_LAUNCH, "debug_tap_read: copy failed");
  return DF_OK;
}

static int posenet_args_ok(const Net *n, int B, int H, int W) {
  if (!n || n->kind != 0) return set_error(DF_ERR_ARG, "not a PoseNet handle");
  if (B <= 0 || H < 8 || W < 8) return set_error(DF_ERR_ARG, "posenet: need B >= 1 and H, W >= 8 (got %d, %d, %d)", B, H, W);
  // psp_prior_sum keeps per-row / per-column interpolation tables of the 1/8-resolution map in LDS (12.8 KB + 64 (h + w) bytes <= 64 KB);
  // the datasets' crops end at 480 x 640 (datasets/ycb/dataset.py:247-289)
  if (H > DF_MAX_CROP || W > DF_MAX_CROP) return set_error(DF_ERR_ARG, "posenet: crops beyond %d pixels per side are not supported (got %d x %d)", DF_MAX_CROP, H, W);
  return DF_OK;
}

// bucket list of a multi-bucket call (host arrays of nb entries); img may be null (workspace sizing)
static int make_groups(const Net *n, int nb, const int *B, const int *H, const int *W, const float *const *img, std::vector<Grp> &gs) {
  // 4096: far above the 12 x 16 = 192 crop sizes the datasets' 40-pixel snapping can produce (datasets/ycb/dataset.py:247-289)
  if (nb <= 0 || nb > 4096 || !B || !H || !W) return set_error(DF_ERR_ARG, "need 1..4096 buckets with B / H / W arrays (got nb = %d)", nb);
  long tot = 0;
  gs.clear();
  for (int i = 0; i < nb; ++i) {
    const int rc = posenet_args_ok(n, B[i], H[i], W[i]);
    if (rc != DF_OK) return rc;
    if (img && !img[i]) return set_error(DF_ERR_ARG, "bucket %d: null image pointer", i);
    gs.push_back(Grp{B[i], H[i], W[i], img ? img[i] : nullptr});
    tot += B[i];
  }
  if (tot > (1 << 20)) return set_error(DF_ERR_ARG, "too many objects in one call (%ld)", tot);
  return DF_OK;
}

extern "C" size_t df_posenet_workspace_bytes(const df_net *h, int B, int H, int W) {
  if (posenet_args_ok(as_net(h), B, H, W) != DF_OK) return 0;
  Ctx c(const_cast<Net *>(as_net(h)), nullptr);
  PoseNetOut o{};
  posenet_forward(c, {Grp{B, H, W, nullptr}}, nullptr, nullptr, nullptr, o);
  return c.peak;
}

extern "C" int df_posenet_forward(df_net *h, int B, int H, int W, const float *img, const float *cloud,
                                  const int64_t *choose, const int64_t *obj, float *out_r, float *out_t, float *out_c,
                                  float *emb, void *ws, size_t ws_bytes, df_stream_t stream) {
  int rc = posenet_args_ok(as_net(h), B, H, W);
  if (rc != DF_OK) return rc;
  if ((rc = check_ready(*as_net(h))) != DF_OK) return rc;
  if (!img || !cloud || !choose || !obj || !out_r || !out_t || !out_c || !emb || !ws) return set_error(DF_ERR_ARG, "posenet_forward: null pointer");
  Ctx c(as_net(h), to_stream(stream), Arena(ws, ws_bytes));
  if (df_posenet_workspace_bytes(h, B, H, W) > ws_bytes) return set_error(DF_ERR_WORKSPACE, "posenet_forward: workspace too small");
  PoseNetOut o{out_r, out_t, out_c, emb};
  posenet_forward(c, {Grp{B, H, W, img}}, cloud, choose, obj, o);
  return finish(c, "posenet_forward");
}

// the same forward over buckets of different crop sizes in ONE pass (objects concatenated in bucket order): what the refiner phase of
// tools/train.py:139-145 needs of its frozen estimator for a whole accumulation window
extern "C" size_t df_posenet_multi_workspace_bytes(const df_net *h, int nb, const int *B, const int *H, const int *W) {
  std::vector<Grp> gs;
  if (!h || as_net(h)->kind != 0 || make_groups(as_net(h), nb, B, H, W, nullptr, gs) != DF_OK) return 0;
  Ctx c(const_cast<Net *>(as_net(h)), nullptr);
  PoseNetOut o{};
  posenet_forward(c, gs, nullptr, nullptr, nullptr, o);
  return c.peak;
}

extern "C" int df_posenet_forward_multi(df_net *h, int nb, const int *B, const int *H, const int *W, const float *const *img, const float *cloud,
                                        const int64_t *choose, const int64_t *obj, float *out_r, float *out_t, float *out_c, float *emb, void *ws,
                                        size_t ws_bytes, df_stream_t stream) {
  if (!h || as_net(h)->kind != 0) return set_error(DF_ERR_ARG, "not a PoseNet handle");
  if (!img) return set_error(DF_ERR_ARG, "posenet_forward_multi: null pointer");
  std::vector<Grp> gs;
  int rc = make_groups(as_net(h), nb, B, H, W, img, gs);
  if (rc != DF_OK) return rc;
  if ((rc = check_ready(*as_net(h))) != DF_OK) return rc;
  if (!cloud || !choose || !obj || !out_r || !out_t || !out_c || !emb || !ws) return set_error(DF_ERR_ARG, "posenet_forward_multi: null pointer");
  if (df_posenet_multi_workspace_bytes(h, nb, B, H, W) > ws_bytes) return set_error(DF_ERR_WORKSPACE, "posenet_forward_multi: workspace too small");
  Ctx c(as_net(h), to_stream(stream), Arena(ws, ws_bytes));
  PoseNetOut o{out_r, out_t, out_c, emb};
  posenet_forward(c, gs, cloud, choose, obj, o);
  return finish(c, "posenet_forward_multi");
}

static void refiner_standalone(Ctx &c, int B, const float *x, const float *emb, const int64_t *obj, float *out_r, float *out_t) {
  const int N = c.net->num_points, Npad = round_up(N, 128);
  float *emb_pm = c.f((size_t)B * Npad * 32);
  RefinerBufs r = refiner_alloc(c, B, N, Npad);
  if (c.live()) launch_emb_to_pm(emb, emb_pm, B, N, Npad, c.st);
  refiner_prepare(c, r, B, Npad, emb_pm);
  refiner_iterate(c, r, B, N, Npad, x, nullptr, obj, out_r, out_t, nullptr, nullptr, nullptr);
}

extern "C" size_t df_refiner_workspace_bytes(const df_net *h, int B) {
  if (!h || as_net(h)->kind != 1 || B <= 0) return 0;
  Ctx c(const_cast<Net *>(as_net(h)), nullptr);
  refiner_standalone(c, B, nullptr, nullptr, nullptr, nullptr, nullptr);
  return c.peak;
}

extern "C" int df_refiner_forward(df_net *h, int B, const float *x, const float *emb, const int64_t *obj, float *out_r,
                                  float *out_t, void *ws, size_t ws_bytes, df_stream_t stream) {
  if (!h || as_net(h)->kind != 1) return set_error(DF_ERR_ARG, "not a PoseRefineNet handle");
  if (B <= 0) return set_error(DF_ERR_ARG, "refiner_forward: B must be >= 1");
  int rc = check_ready(*as_net(h));
  if (rc != DF_OK) return rc;
  if (!x || !emb || !obj || !out_r || !out_t || !ws) return set_error(DF_ERR_ARG, "refiner_forward: null pointer");
  if (df_refiner_workspace_bytes(h, B) > ws_bytes) return set_error(DF_ERR_WORKSPACE, "refiner_forward: workspace too small");
  Ctx c(as_net(h), to_stream(stream), Arena(ws, ws_bytes));
  refiner_standalone(c, B, x, emb, obj, out_r, out_t);
  return finish(c, "refiner_forward");
}

// PoseNet -> selection -> `iters` refine passes, entirely on the device, for the objects of all buckets (concatenated in bucket order)
static void estimate(Ctx &cp, Ctx &cr, const std::vector<Grp> &gs, const float *cloud, const int64_t *choose, const int64_t *obj, int iters,
                     double *pose_wo, double *pose) {
  const int N = cp.net->num_points, Npad = round_up(N, 128);
  int B = 0;
  for (const Grp &g : gs) B += g.B;
  PoseNetOut o{};
  o.emb = cp.f((size_t)B * 32 * N);
  double *state = reinterpret_cast<double *>(cp.bytes((size_t)B * 7 * sizeof(double)));
  float *rt = cp.f((size_t)B * 12);
  // eval_ycb.py:193-203 reads the r / t heads at the arg-max-confidence point only: confidence tower for all points,
  // r / t towers for that one point (posenet_points, `sel`)
  const SelectOut sel{pose_wo, state, rt};
  posenet_forward(cp, gs, cloud, choose, obj, o, &sel);
  // the refiner context continues in the same workspace
  cr.off = cp.off;
  cr.peak = cp.peak;
  RefinerBufs r = refiner_alloc(cr, B, N, Npad);
  if (iters > 0) refiner_prepare(cr, r, B, Npad, o.emb_pm);
  for (int it = 0; it < iters; ++it)
    refiner_iterate(cr, r, B, N, Npad, cloud, rt, obj, nullptr, nullptr, state, rt, it == iters - 1 ? pose : nullptr);
  if (iters == 0 && cp.live() && pose) hipMemcpyAsync(pose, state, (size_t)B * 7 * sizeof(double), hipMemcpyDeviceToDevice, cp.st);
}

static int estimate_handles_ok(const df_net *pn, const df_net *rf) {
  if (!pn || as_net(pn)->kind != 0) return set_error(DF_ERR_ARG, "estimate_poses: not a PoseNet handle");
  if (!rf || as_net(rf)->kind != 1) return set_error(DF_ERR_ARG, "estimate_poses: not a PoseRefineNet handle");
  if (as_net(rf)->num_points != as_net(pn)->num_points || as_net(rf)->num_obj != as_net(pn)->num_obj)
    return set_error(DF_ERR_ARG, "estimate_poses: estimator / refiner disagree on num_points or num_obj");
  return DF_OK;
}

extern "C" size_t df_estimate_multi_workspace_bytes(const df_net *pn, const df_net *rf, int nb, const int *B, const int *H, const int *W) {
  std::vector<Grp> gs;
  if (estimate_handles_ok(pn, rf) != DF_OK || make_groups(as_net(pn), nb, B, H, W, nullptr, gs) != DF_OK) return 0;
  Ctx cp(const_cast<Net *>(as_net(pn)), nullptr), cr(const_cast<Net *>(as_net(rf)), nullptr);
  estimate(cp, cr, gs, nullptr, nullptr, nullptr, 1, nullptr, nullptr);
  return cr.peak;
}

extern "C" int df_estimate_poses_multi(df_net *pn, df_net *rf, int nb, const int *B, const int *H, const int *W, const float *const *img,
                                       const float *cloud, const int64_t *choose, const int64_t *obj, int iters, double *pose_wo,
                                       double *pose, void *ws, size_t ws_bytes, df_stream_t stream) {
  int rc = estimate_handles_ok(pn, rf);
  if (rc != DF_OK) return rc;
  std::vector<Grp> gs;
  if (!img) return set_error(DF_ERR_ARG, "estimate_poses: null pointer");
  if ((rc = make_groups(as_net(pn), nb, B, H, W, img, gs)) != DF_OK) return rc;
  if (iters < 0) return set_error(DF_ERR_ARG, "estimate_poses: iters < 0");
  if ((rc = check_ready(*as_net(pn))) != DF_OK || (rc = check_ready(*as_net(rf))) != DF_OK) return rc;
  if (!cloud || !choose || !obj || !pose || !ws) return set_error(DF_ERR_ARG, "estimate_poses: null pointer");
  if (df_estimate_multi_workspace_bytes(pn, rf, nb, B, H, W) > ws_bytes) return set_error(DF_ERR_WORKSPACE, "estimate_poses: workspace too small");
  Ctx cp(as_net(pn), to_stream(stream), Arena(ws, ws_bytes)), cr(as_net(rf), to_stream(stream), Arena(ws, ws_bytes));
  estimate(cp, cr, gs, cloud, choose, obj, iters, pose_wo, pose);
  if (cp.err != DF_OK) return cp.err;
  return finish(cr, "estimate_poses");
}

extern "C" size_t df_estimate_workspace_bytes(const df_net *pn, const df_net *rf, int B, int H, int W) {
  return df_estimate_multi_workspace_bytes(pn, rf, 1, &B, &H, &W);
}

extern "C" int df_estimate_poses(df_net *pn, df_net *rf, int B, int H, int W, const float *img, const float *cloud,
                                 const int64_t *choose, const int64_t *obj, int iters, double *pose_wo, double *pose,
                                 void *ws, size_t ws_bytes, df_stream_t stream) {
  return df_estimate_poses_multi(pn, rf, 1, &B, &H, &W, &img, cloud, choose, obj, iters, pose_wo, pose, ws, ws_bytes, stream);
}
