// Host plumbing shared by the inference engine (engine.hip) and the native training step (train.hip): the workspace arena with its
// sizing pass, the per-launch GEMM timer behind df_net_profile / df_trainer_profile, the reference parameter list of each network,
// one resolution level of a pass over crop-size buckets and the Winograd-domain pass over some of a level's buckets.
#pragma once
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "wino.h"

// hidden: internal to the library, none of it joins the exported symbols
namespace df __attribute__((visibility("hidden"))) {

// ------------------------------------------------------------------------------------------------
// workspace arena
// ------------------------------------------------------------------------------------------------
// 256-byte aligned regions of the caller's workspace, handed out in call order; `off` may be wound back to reuse scratch, `peak` is the
// high-water mark.  The sizing pass (no workspace) walks the same code and launches nothing.  It hands out (never dereferenced) non-null
// addresses too, so that every "is there a buffer yet" decision comes out as in the real run: both passes allocate the same sequence by
// construction.
struct Arena {
  bool dry = true;
  char *base = nullptr;
  size_t off = 0, cap = 0, peak = 0;
  int err = DF_OK;                   // the first error of the pass

  Arena() = default;                 // the sizing pass
  Arena(void *ws, size_t ws_bytes) : dry(false), base(static_cast<char *>(ws)), cap(ws_bytes) {}
  void *bytes(size_t b) {
    b = (b + 255) & ~size_t(255);
    void *p = (dry ? reinterpret_cast<char *>(4096) : base) + off;
    off += b;
    if (off > peak) peak = off;
    if (!dry && off > cap && err == DF_OK) err = set_error(DF_ERR_WORKSPACE, "workspace too small (need > %zu bytes, have %zu)", off, cap);
    return p;
  }
  float *f(size_t floats) { return static_cast<float *>(bytes(floats * sizeof(float))); }
  bool live() const { return !dry && err == DF_OK; }
  void fail(int rc) { if (rc != DF_OK && err == DF_OK) err = rc; }
};

// ------------------------------------------------------------------------------------------------
// per-launch GEMM timer
// ------------------------------------------------------------------------------------------------
struct LaunchRecord {
  int kind = 0;              // the owner's bin (trainer: 0 forward, 1 data gradient, 2 weight gradient)
  double flops = 0;          // executed FLOPs
  double bytes = 0;          // algorithmic HBM bytes
  double useful = 0;         // FLOPs of the rows that are not padding
  bool bf16 = false;         // taken by the bf16 x 6 kernel
#ifdef DF_DEV
  char desc[160] = "";       // the launch's shape (DF_PROFILE_VERBOSE)
#endif
};

// the record of one launch of `p`; M: its output rows when they are not B * OH * OW (a launch over several buckets)
inline LaunchRecord launch_record(int kind, double flops, const ConvParams &p, long M = 0) {
  LaunchRecord r;
  r.kind = kind;
  r.flops = flops;
#ifdef DF_DEV
  snprintf(r.desc, sizeof(r.desc), "M=%ld N=%d K=%d k%dx%d s%d d%d z%d", M > 0 ? M : (long)p.B * p.OH * p.OW, p.Cout, p.KH * p.KW * p.Cin, p.KH, p.KW,
           p.stride, p.dil, p.zcount);
#endif
  return r;
}

struct LaunchSum { double ms = 0, flops = 0, bytes = 0, useful = 0; int launches = 0; };

// HIP event pairs on the launch stream around every timed launch.  Off, the owner calls nothing; on, begin() and end() bracket each launch.
struct LaunchTimer {
  bool on = false;
  std::vector<hipEvent_t> ev;        // pool, grown on demand: launch i of rec is timed by ev[2 i], ev[2 i + 1]
  std::vector<LaunchRecord> rec;

  LaunchTimer() = default;
  LaunchTimer(const LaunchTimer &) = delete;
  LaunchTimer &operator=(const LaunchTimer &) = delete;
  ~LaunchTimer() { for (hipEvent_t e : ev) hipEventDestroy(e); }
  void arm(bool enable) { on = enable; rec.clear(); }
  int begin(hipStream_t st) {
    while (ev.size() < 2 * rec.size() + 2) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return set_error(DF_ERR_LAUNCH, "profile: hipEventCreate failed");
      ev.push_back(e);
    }
    hipEventRecord(ev[2 * rec.size()], st);
    return DF_OK;
  }
  void end(hipStream_t st, const LaunchRecord &r) {
    hipEventRecord(ev[2 * rec.size() + 1], st);
    rec.push_back(r);
  }
  // after a stream sync: adds every launch into sums[bin(record)] (bin < 0: left out); development build with DF_PROFILE_VERBOSE set and
  // `tags` given: one stderr line per summed launch, led by tags[bin]
  template <class Bin> int sum(LaunchSum *sums, Bin bin, const char *const *tags, const char *what) const {
#ifdef DF_DEV
    static const bool verbose = dev_getenv("DF_PROFILE_VERBOSE") != nullptr;
#endif
    for (size_t i = 0; i < rec.size(); ++i) {
      const LaunchRecord &r = rec[i];
      const int b = bin(r);
      if (b < 0) continue;
      float ms = 0;
      if (hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]) != hipSuccess) return set_error(DF_ERR_LAUNCH, "%s: events not complete", what);
      LaunchSum &s = sums[b];
      s.ms += ms; s.flops += r.flops; s.bytes += r.bytes; s.useful += r.useful; ++s.launches;
#ifdef DF_DEV
      if (verbose && tags) fprintf(stderr, "%s %-44s %9.1f us %7.1f TFLOP/s\n", tags[b], r.desc, ms * 1e3, r.flops / (ms * 1e-3) / 1e12);
#endif
    }
    return DF_OK;
  }
};

// ------------------------------------------------------------------------------------------------
// reference parameter lists
// ------------------------------------------------------------------------------------------------
struct ParamInfo {
  std::string key;
  int64_t shape[4] = {1, 1, 1, 1};
  int ndim = 0;
  int64_t numel() const { int64_t n = 1; for (int i = 0; i < ndim; ++i) n *= shape[i]; return n; }
};

constexpr char CNN[] = "cnn.model.module.";

inline bool ends_with(const std::string &s, const char *suf) {
  const size_t l = strlen(suf);
  return s.size() >= l && s.compare(s.size() - l, l, suf) == 0;
}

struct ParamList {
  std::vector<ParamInfo> spec;
  std::map<std::string, int> index;
  void add(const std::string &key, std::initializer_list<int64_t> shp) {
    ParamInfo p;
    p.key = key;
    for (int64_t v : shp) p.shape[p.ndim++] = v;
    index[key] = (int)spec.size();
    spec.push_back(p);
  }
  int find(const std::string &key) const { auto it = index.find(key); return it == index.end() ? -1 : it->second; }
  // df_net_param_info / df_trainer_param_info
  int info(int i, char *key_out, int key_cap, int64_t *shape4, int *ndim, const char *what) const {
    if (i < 0 || i >= (int)spec.size()) return set_error(DF_ERR_ARG, "%s: index out of range", what);
    const ParamInfo &p = spec[i];
    if (key_out && key_cap > 0) { strncpy(key_out, p.key.c_str(), key_cap - 1); key_out[key_cap - 1] = 0; }
    if (shape4) for (int d = 0; d < 4; ++d) shape4[d] = p.shape[d];
    if (ndim) *ndim = p.ndim;
    return DF_OK;
  }
};

// The state-dict keys and shapes of PoseNet (kind 0) or PoseRefineNet (kind 1) in the reference's order: what the engine loads, what the
// trainer lays out in its flat buffer and what checkpoints carry (lib/network.py:53-206, lib/pspnet.py:20-77, lib/extractors.py:29-124).
inline ParamList reference_params(int kind, int num_obj) {
  ParamList n;
  const char *fn[6] = {"conv1", "conv2", "e_conv1", "e_conv2", "conv5", "conv6"};
  const int fo[6] = {64, 128, 64, 128, 512, 1024};
  if (kind == 1) {
    const int fi[6] = {3, 64, 32, 64, 384, 512};
    for (int i = 0; i < 6; ++i) {
      n.add(std::string("feat.") + fn[i] + ".weight", {fo[i], fi[i], 1});
      n.add(std::string("feat.") + fn[i] + ".bias", {fo[i]});
    }
    const int li[2] = {1024, 512}, lo[2] = {512, 128};
    const char *hs[2] = {"r", "t"};
    for (int l = 0; l < 2; ++l)
      for (int h = 0; h < 2; ++h) {
        const std::string nm = "conv" + std::to_string(l + 1) + "_" + hs[h];
        n.add(nm + ".weight", {lo[l], li[l]});
        n.add(nm + ".bias", {lo[l]});
      }
    const int per[2] = {4, 3};
    for (int h = 0; h < 2; ++h) {
      const std::string nm = std::string("conv3_") + hs[h];
      n.add(nm + ".weight", {(int64_t)num_obj * per[h], 128});
      n.add(nm + ".bias", {(int64_t)num_obj * per[h]});
    }
    return n;
  }
  const std::string c = CNN;
  n.add(c + "feats.conv1.weight", {64, 3, 7, 7});
  int inpl = 64;
  const int planes_of[4] = {64, 128, 256, 512};
  for (int li = 1; li <= 4; ++li) {
    const int planes = planes_of[li - 1];
    for (int blk = 0; blk < 2; ++blk) {
      const int cin = blk == 0 ? inpl : planes;
      const std::string base = c + "feats.layer" + std::to_string(li) + "." + std::to_string(blk) + ".";
      n.add(base + "conv1.weight", {planes, cin, 3, 3});
      n.add(base + "conv2.weight", {planes, planes, 3, 3});
      if (blk == 0 && cin != planes) n.add(base + "downsample.0.weight", {planes, cin, 1, 1});
    }
    inpl = planes;
  }
  for (int s = 0; s < 4; ++s) n.add(c + "psp.stages." + std::to_string(s) + ".1.weight", {512, 512, 1, 1});
  n.add(c + "psp.bottleneck.weight", {1024, 2560, 1, 1});
  n.add(c + "psp.bottleneck.bias", {1024});
  const char *ups[3] = {"up_1", "up_2", "up_3"};
  const int up_in[3] = {1024, 256, 64}, up_out[3] = {256, 64, 64};
  for (int u = 0; u < 3; ++u) {
    n.add(c + ups[u] + ".conv.1.weight", {up_out[u], up_in[u], 3, 3});
    n.add(c + ups[u] + ".conv.1.bias", {up_out[u]});
    n.add(c + ups[u] + ".conv.2.weight", {1});
  }
  n.add(c + "final.0.weight", {32, 64, 1, 1});
  n.add(c + "final.0.bias", {32});
  n.add(c + "classifier.0.weight", {256, 256});   // dead weights (lib/pspnet.py:58-62): accepted, unused
  n.add(c + "classifier.0.bias", {256});
  n.add(c + "classifier.2.weight", {21, 256});
  n.add(c + "classifier.2.bias", {21});
  const int fi[6] = {3, 64, 32, 64, 256, 512};
  for (int i = 0; i < 6; ++i) {
    n.add(std::string("feat.") + fn[i] + ".weight", {fo[i], fi[i], 1});
    n.add(std::string("feat.") + fn[i] + ".bias", {fo[i]});
  }
  const int hin[3] = {1408, 640, 256}, hout[3] = {640, 256, 128};
  const char *hs[3] = {"r", "t", "c"};
  for (int l = 0; l < 3; ++l)
    for (int h = 0; h < 3; ++h) {
      const std::string nm = "conv" + std::to_string(l + 1) + "_" + hs[h];
      n.add(nm + ".weight", {hout[l], hin[l], 1});
      n.add(nm + ".bias", {hout[l]});
    }
  const int per[3] = {4, 3, 1};
  for (int h = 0; h < 3; ++h) {
    const std::string nm = std::string("conv4_") + hs[h];
    n.add(nm + ".weight", {(int64_t)num_obj * per[h], 128, 1});
    n.add(nm + ".bias", {(int64_t)num_obj * per[h]});
  }
  return n;
}

// ------------------------------------------------------------------------------------------------
// one resolution level of a pass over crop-size buckets
// ------------------------------------------------------------------------------------------------
// The buckets' [B_i][H_i][W_i] blocks concatenated along the pixel-row axis.  Launches whose arithmetic does not depend on the crop geometry
// (1x1 convolutions, the Winograd-domain products, the low-resolution up-conv products, every weight gradient, the whole per-point part) cover
// the rows of all buckets at once; direct k x k convolutions and the memory-bound glue run per bucket on row offsets into the same buffers.
// The trainer's point rows are one bucket of H = W = 1.
struct Level {
  std::vector<int> B, H, W;
  std::vector<long> off;      // first pixel row of bucket i
  std::vector<int> b0;        // first frame of bucket i
  long rows = 0;
  int frames = 0;
  int nb() const { return (int)B.size(); }
  void push(int b, int h, int w) {
    B.push_back(b); H.push_back(h); W.push_back(w); off.push_back(rows); b0.push_back(frames);
    rows += (long)b * h * w; frames += b;
  }
};

// ------------------------------------------------------------------------------------------------
// the Winograd-domain pass over buckets of a level
// ------------------------------------------------------------------------------------------------
// The plan of buckets `idx` of a level (stride-1 layers: input and output levels have the same rows).  The layout is chosen here, once.
inline WinoPlan wino_plan(const Level &lv, const std::vector<int> &idx, int dil, int m, bool packed) {
  WinoPlan pl{dil, m, packed};
  for (int i : idx) pl.add(lv.B[i], lv.H[i], lv.W[i], lv.off[i]);
  return pl;
}

// out = act(conv3x3(in) + res) over the plan's buckets: input transform, ONE z-batched GEMM over the concatenation of their tiles against
// the transformed weights U [nz][co][ci], output transform.  V / M are scratch: the arena is wound back, so consecutive layers reuse the
// region.  gemm(p) launches (and times) the product; like the arena's owner it does nothing on a pass that is not live.
template <class Gemm>
void wino_pass(Arena &a, hipStream_t st, const WinoPlan &pl, const float *in, int in_ld, int ci, const float *U, float *out, int out_ld, int co,
               const float *res, int res_ld, int act, Gemm gemm) {
  if (pl.b.empty()) return;
  const size_t mark = a.off;
  float *V = a.f((size_t)pl.nz() * pl.T * ci), *M = a.f((size_t)pl.nz() * pl.T * co);
  if (a.live()) launch_wino_input(pl, in, in_ld, V, ci, st);
  ConvParams p;
  p.in = V; p.wgt = U; p.out = M;
  p.B = (int)pl.T; p.Cin = ci; p.in_ld = ci; p.Cout = co; p.out_ld = co;
  p.zcount = pl.nz(); p.z_in_coff = pl.T * ci; p.z_wgt = (long)co * ci; p.z_out_coff = pl.T * co;
  gemm(p);
  if (a.live()) launch_wino_output(pl, M, out, out_ld, res, res_ld, act, co, st);
  a.off = mark;
}

}  // namespace df
