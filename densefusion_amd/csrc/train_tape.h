// Host plumbing of the native training step (train.hip includes this file, and nothing else does): the trainer handle and its flat
// parameter layout, the step's workspace arena / activation records / backward tape, the ConvParams builders, and the layer idioms the two
// network steps are written in -- conv() with its backward, the backward of a hand-launched GEMM, channel slices and their gradients.
#pragma once
#include <algorithm>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "host_plan.h"
#include "igemm.h"
#include "wino.h"
#include "train_kernels.h"

namespace df {
namespace {

// ------------------------------------------------------------------------------------------------
// trainer handle: parameter spec (reference keys / shapes) and where every tensor lives in the flat buffer
// ------------------------------------------------------------------------------------------------
// where a reference tensor lives in the flat buffer (kernel layout): up to two pieces (head layer 1's weight splits into the per-point and
// the global-feature block)
enum PlaceMode {            // (the values are relayout_kernel's `mode` argument)
  PLACE_CONV = 0,           // OIHW -> O(T)Ipad
  PLACE_TAPMAJOR = 1,       // OIHW -> tap-major
  PLACE_COPY = 2,           // plain copy
  PLACE_HEAD1 = 3,          // head layer 1's weight, split into its two column blocks
};
struct Place {
  PlaceMode mode = PLACE_COPY;
  size_t off = 0, off2 = 0; // flat offsets (floats); off2: second piece of PLACE_HEAD1
};

struct Trainer {
  int kind = 0, N = 0, K = 0, device = 0;
  std::map<std::vector<int>, size_t> ws_cache;      // (B, H, W, M) -> workspace bytes (the sizing pass walks the whole step)
  ParamList params;                          // reference keys and shapes (host_plan.h)
  std::vector<Place> place;                  // per entry of params
  std::map<std::string, size_t> slot;        // internal name -> flat offset
  size_t flat = 0;
  // flipped / transposed weights for the data gradients, rebuilt when the caller's parameter version changes
  float *wflip = nullptr;
  long flip_version = -1;
  const float *flip_src = nullptr;
  struct Flip { size_t off; int O, T, I, KH, KW, Z; };
  std::vector<Flip> flips;
  // Winograd F(4x4,3x3)-domain copies of the stride-1 3x3 trunk weights with >= 128 input channels (forward: G w G^T of the packed
  // weights; data gradient: of the flipped ones), [36][O][I] each, rebuilt with the flips
  struct Wino { size_t w_off, fwd, bwd; int O, I; };
  std::map<std::string, Wino> wino;
  float *wino_buf = nullptr;
  size_t wino_floats = 0;
  FlipTile *flip_tiles = nullptr;  // device copy of `flips` as the tiled flip's segment table
  int flip_ntiles = 0;
  bool splitk = true;             // df_trainer_set_splitk
  // df_trainer_profile: every MFMA launch of a step, executed FLOPs per kind (0 fwd, 1 dgrad, 2 wgrad)
  LaunchTimer timer;
};

size_t take(Trainer &t, const std::string &name, size_t floats) {
  const size_t o = t.flat;
  t.slot[name] = o;
  t.flat += (floats + 63) / 64 * 64;          // 256-byte aligned slots
  return o;
}

// a convolution weight in O(T)Ipad, or tap-major (up_1 / up_2: the low-resolution product is a 1x1 conv with 9*O outputs).  as_gemm: the
// step uses the packed [O][(ky,kx,c)] rows as a plain GEMM operand (up_3 on chosen-pixel patches; the strided layer2.0.conv1, whose data
// gradient goes through per-tap products + a gather): its data gradient needs the plain transpose, not the tap-mirrored one
void add_conv(Trainer &t, const ParamInfo &p, bool tapmajor, bool as_gemm) {
  const std::string &key = p.key;
  const int O = (int)p.shape[0], I = (int)p.shape[1], k = (int)p.shape[2];
  const int Ipad = (I + 3) / 4 * 4, T = k * k;
  const size_t off = take(t, key, (size_t)O * T * Ipad);
  t.place.push_back({tapmajor ? PLACE_TAPMAJOR : PLACE_CONV, off});
  if (tapmajor) t.flips.push_back({off, 9 * O, 1, I, 1, 1, 1});
  else if (as_gemm) t.flips.push_back({off, O, 1, T * Ipad, 1, 1, 1});
  else t.flips.push_back({off, O, T, Ipad, k, k, 1});
  if (k == 3 && !tapmajor && !as_gemm && I >= 128 && I % 4 == 0 && O % 4 == 0 && key.find("feats.layer") != std::string::npos) {
    const size_t n = (size_t)36 * O * I;
    t.wino[key] = Trainer::Wino{off, t.wino_floats, t.wino_floats + n, O, I};
    t.wino_floats += 2 * n;
  }
}

// Lays the reference tensors out in the flat buffer, in reference order (the slots are taken in that order):
//   * 4-d convolution weights: add_conv;
//   * PoseNet head layers 1 - 3: the three towers stacked r, t, c ([1920][384] per-point block, [1920][1024] global-feature block and
//     [1920] bias of layer 1; [3][256][640], [768]; [3][128][256], [384]);
//   * the Conv1d(k=1) / Linear weights the step uses as GEMM operands (feat.conv2 .. conv6, the refiner's FC towers): plain, with a transpose;
//   * the rest -- biases, PReLU slopes, the cloud's first conv, the object-indexed last head layer, the dead classifier -- as plain copies.
void lay_out(Trainer &t) {
  const size_t npos = std::string::npos;
  size_t wpt = 0, wg = 0, hw[4] = {}, hb[4] = {};      // the stacked head layers' slots, taken at the first of them
  for (const ParamInfo &p : t.params.spec) {
    const std::string &k = p.key;
    const size_t n = (size_t)p.numel();
    const bool weight = ends_with(k, ".weight");
    const bool head = k.rfind("conv", 0) == 0;               // the towers: conv<l>_<r|t|c>
    const int l = head ? k[4] - '0' : 0, h = head ? (k[6] == 'r' ? 0 : k[6] == 't' ? 1 : 2) : 0;
    const bool last = head && l == (t.kind == 0 ? 4 : 3);
    if (p.ndim == 4) {
      add_conv(t, p, k.find(".up_1.") != npos || k.find(".up_2.") != npos, k.find(".up_3.") != npos || k.find("feats.layer2.0.conv1.") != npos);
    } else if (t.kind == 0 && head && !last) {
      if (!wpt) {
        wpt = take(t, "head1.wpt", (size_t)1920 * 384);
        wg = take(t, "head1.wg", (size_t)1920 * 1024);
        hb[1] = take(t, "head1.bias", 1920);
        hw[2] = take(t, "head2.w", (size_t)3 * 256 * 640);
        hb[2] = take(t, "head2.bias", 768);
        hw[3] = take(t, "head3.w", (size_t)3 * 128 * 256);
        hb[3] = take(t, "head3.bias", 384);
        t.flips.push_back({wpt, 1920, 1, 384, 1, 1, 1});
        t.flips.push_back({wg, 1920, 1, 1024, 1, 1, 1});
        t.flips.push_back({hw[2], 256, 1, 640, 1, 1, 3});
        t.flips.push_back({hw[3], 128, 1, 256, 1, 1, 3});
      }
      if (l == 1 && weight) t.place.push_back({PLACE_HEAD1, wpt + (size_t)h * 640 * 384, wg + (size_t)h * 640 * 1024});
      else t.place.push_back({PLACE_COPY, (weight ? hw[l] : hb[l]) + h * n});
    } else if (weight && p.ndim >= 2 && !last && k != "feat.conv1.weight" && k.find("classifier") == npos) {
      const size_t off = take(t, k, n);
      t.place.push_back({PLACE_COPY, off});
      t.flips.push_back({off, (int)p.shape[0], 1, (int)p.shape[1], 1, 1, 1});
    } else {
      t.place.push_back({PLACE_COPY, take(t, k, n)});
    }
  }
}

// ------------------------------------------------------------------------------------------------
// step plumbing: workspace arena, activation records, the backward tape
// ------------------------------------------------------------------------------------------------
struct View { float *d = nullptr; int ld = 0; };           // [rows][C] view: element (r, c) at d[r * ld + c] (d already offset to its channel)

struct Act {
  View v, g;                    // values; gradient (allocated / aliased during the backward pass)
  const Level *lv = nullptr;
  int C = 0;
  bool gset = false;
  long rows() const { return lv->rows; }
};

enum GemmKind { GK_FWD = 0, GK_DGRAD = 1, GK_WGRAD = 2 };

// one training step: the workspace arena (host_plan.h), the handle, the launch stream, the activation records and the backward tape
struct Step : Arena {
  Trainer *t;
  hipStream_t st;
  const float *P = nullptr;      // flat parameters
  float *G = nullptr;            // flat gradients (accumulated)
  float *splitk = nullptr;
  size_t splitk_bytes = 0;
  std::deque<Act> acts;
  std::deque<Level> lvs;
  std::vector<std::function<void(Step &)>> tape;     // backward closures, run last to first (run_tape)

  Step(Trainer *tr, hipStream_t s, Arena a = Arena()) : Arena(a), t(tr), st(s) {}
#ifdef DF_DEV
  // dev build, DF_TRAIN_DEBUG=1: synchronise after every phase and name it on stderr (localises a faulting launch)
  void dbg(const char *what, const std::string &extra = std::string()) {
    static const bool on = df::dev_getenv("DF_TRAIN_DEBUG") != nullptr;
    if (!on || dry) return;
    const hipError_t e = hipStreamSynchronize(st);
    fprintf(stderr, "[df-train] %s %s: %s\n", what, extra.c_str(), e == hipSuccess ? "ok" : hipGetErrorString(e));
    fflush(stderr);
  }
#else
  void dbg(const char *, const std::string & = std::string()) {}
#endif
  // every MFMA launch of the step goes through here: with df_trainer_profile on, HIP events on the launch stream bracket it and its
  // EXECUTED FLOPs are tallied per kind (forward / data gradient / weight gradient)
  template <class Launch> void timed(int kind, double flops, const ConvParams &p, long M, Launch launch) {
    LaunchTimer &tm = t->timer;
    if (tm.on) fail(tm.begin(st));
    if (!live()) return;
    fail(launch());
    if (tm.on && live()) tm.end(st, launch_record(kind, flops, p, M));
  }
  void gemm(int kind, const ConvParams &p) {
    if (!live()) return;
    timed(kind, conv_flops(p), p, 0, [&] { return launch_conv(p, st); });
  }
  // the same convolution over several buckets: one launch (launch_conv_multi)
  void gemm_multi(int kind, const ConvParams &p, const std::vector<WgradSeg> &segs) {
    if (!live() || segs.empty()) return;
    double fl = 0;
    long M = 0;
    for (const WgradSeg &g : segs) {
      fl += 2.0 * g.B * g.OH * g.OW * (double)p.Cout * p.KH * p.KW * p.Cin;
      M += (long)g.B * g.OH * g.OW;
    }
    timed(kind, fl, p, M, [&] { return launch_conv_multi(p, (int)segs.size(), segs.data(), st); });
  }
  size_t slot(const std::string &name) {
    auto it = t->slot.find(name);
    if (it == t->slot.end()) {
      if (err == DF_OK) err = set_error(DF_ERR_STATE, "trainer: no parameter slot named '%s'", name.c_str());
      return 0;
    }
    return it->second;
  }
  const float *p(const std::string &name, size_t extra = 0) { const size_t o = slot(name); return dry ? nullptr : P + o + extra; }
  float *gr(const std::string &name, size_t extra = 0) { const size_t o = slot(name); return dry ? nullptr : G + o + extra; }
  const float *pf(const std::string &name, size_t extra = 0) { const size_t o = slot(name); return dry ? nullptr : t->wflip + o + extra; }
  const Level *level(const Level &l) { lvs.push_back(l); return &lvs.back(); }
  const Level *flat_level(long rows) { Level l; l.push((int)rows, 1, 1); return level(l); }
  Act *act(const Level *lv, int C, float *d = nullptr, int ld = 0) {
    acts.emplace_back();
    Act *a = &acts.back();
    a->lv = lv; a->C = C;
    a->v.d = d ? d : f((size_t)lv->rows * C);
    a->v.ld = d ? ld : C;
    return a;
  }
  Act *act(long rows, int C, float *d = nullptr, int ld = 0) { return act(flat_level(rows), C, d, ld); }
  // gradient storage of `a` for a producer that is about to write (returns true when it has to ACCUMULATE)
  bool grad_of(Act *a) {
    if (!a->g.d) { a->g.d = f((size_t)a->rows() * a->C); a->g.ld = a->C; }
    const bool acc = a->gset;
    a->gset = true;
    return acc;
  }
  // the step's split-K scratch (allocated either way: the workspace size does not depend on df_trainer_set_splitk) ...
  void take_splitk(size_t b) {
    splitk_bytes = b;
    splitk = static_cast<float *>(bytes(b));
    if (!t->splitk) { splitk = nullptr; splitk_bytes = 0; }
  }
  // ... and the launches that may use it: conv()'s, upconv's product and every data-gradient GEMM (the hand-launched forward GEMMs do not)
  void with_splitk(ConvParams &p) const { p.splitk_ws = splitk; p.splitk_ws_bytes = splitk_bytes; }
};

// the backward pass: the tape's closures, last to first
void run_tape(Step &s) {
  for (size_t i = s.tape.size(); i-- > 0;) {
    s.tape[i](s);
    s.dbg("tape entry", std::to_string(i));
  }
}

// a plain GEMM over all rows of x: every pixel / point row is one output row (1x1 convolution, stride 1)
ConvParams flat_params(const Act *x, int cin, const float *w, const float *bias, Act *y, int act) {
  ConvParams p;
  p.in = x->v.d; p.wgt = w; p.bias = bias; p.out = y->v.d;
  p.B = (int)x->rows(); p.H = p.W = p.OH = p.OW = 1; p.Cin = cin; p.in_ld = x->v.ld;
  p.Cout = y->C; p.out_ld = y->v.ld;
  p.act = act;
  return p;
}
// bucket tables of a level, TAB_MAX buckets each (aux: a second level whose first rows go into aux0)
std::vector<BTab> make_tabs(const Level *lv, const Level *aux = nullptr) {
  std::vector<BTab> out;
  for (int g0 = 0; g0 < lv->nb(); g0 += TAB_MAX) {
    BTab t{};
    t.n = std::min(TAB_MAX, lv->nb() - g0);
    for (int i = 0; i < TAB_MAX; ++i) {
      const int g = g0 + std::min(i, t.n - 1);           // (entries past n repeat the last bucket: never selected)
      t.B[i] = lv->B[g]; t.H[i] = lv->H[g]; t.W[i] = lv->W[g]; t.b0[i] = lv->b0[g];
      t.row0[i] = lv->off[g]; t.row1[i] = lv->off[g] + (long)lv->B[g] * lv->H[g] * lv->W[g];
      t.aux0[i] = aux ? aux->off[g] : 0;
    }
    out.push_back(t);
  }
  return out;
}
inline long tab_rows(const BTab &t) { return t.row1[t.n - 1] - t.row0[0]; }
inline int tab_frames(const BTab &t) { return t.b0[t.n - 1] + t.B[t.n - 1] - t.b0[0]; }

// bucket i of a k x k convolution between two levels
ConvParams bucket_params(const Act *x, int i, int cin, const float *w, const float *bias, Act *y, int k, int stride, int pad, int dil, int act) {
  ConvParams p;
  const Level *li = x->lv, *lo = y->lv;
  p.in = x->v.d + li->off[i] * x->v.ld; p.wgt = w; p.bias = bias; p.out = y->v.d + lo->off[i] * y->v.ld;
  p.B = li->B[i]; p.H = li->H[i]; p.W = li->W[i]; p.Cin = cin; p.in_ld = x->v.ld;
  p.OH = lo->H[i]; p.OW = lo->W[i]; p.Cout = y->C; p.out_ld = y->v.ld;
  p.KH = p.KW = k; p.stride = stride; p.pad = pad; p.dil = dil; p.act = act;
  return p;
}

void launch_act_bwd(Step &s, Act *y, int act, const float *slope, float *dslope) {
  const long rows = y->rows();
  const int C4 = y->C / 4;
  const unsigned blocks = act == 2 ? nblk(rows * C4, 512) : nblk(rows * C4);
  float *part = act == 2 ? s.f(blocks) : nullptr;
  if (!s.live()) return;
  hipLaunchKernelGGL(act_bwd2d_kernel, dim3(blocks), dim3(TB), 0, s.st, y->g.d, y->g.ld, y->v.d, y->v.ld, rows, C4, act, slope, part);
  if (act == 2) hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(TB), 0, s.st, part, (int)blocks, 1L, dslope, 1);
}

// weight / bias gradient of a forward GEMM / convolution (`f`: channels, strides, kernel geometry; `segs`: the buckets) with upstream
// gradient view gy, accumulated into dw / db: ONE contraction over the pixels of all buckets
void wgrad(Step &s, ConvParams f, const std::vector<WgradSeg> &segs, View gy, float *dw, float *db) {
  f.out = gy.d; f.out_ld = gy.ld; f.out_coff = 0;
  f.bias = nullptr; f.res = nullptr; f.act = ACT_NONE; f.zcount = 1;
  f.rows_per_group = f.rows_valid = f.bias_group_ld = 0;
  const size_t mark = s.off;
  const size_t need = wgrad_multi_workspace_bytes(f, (int)segs.size(), segs.data());
  void *ws = s.bytes(need);
  if (s.live()) {
    double M = 0;
    for (const WgradSeg &g : segs) M += (double)g.B * g.OH * g.OW;
    s.timed(GK_WGRAD, 2.0 * M * f.Cout * f.KH * f.KW * f.Cin, f, (long)M,
            [&] { return launch_wgrad_multi(f, (int)segs.size(), segs.data(), dw, db, ws, need, s.st, 1); });
  }
  s.dbg("wgrad");
  s.off = mark;
}
// a launch that is one bucket by itself (plain GEMMs over rows; `f` carries B / H / W / OH / OW)
void wgrad(Step &s, const ConvParams &f, View gy, float *dw, float *db) {
  wgrad(s, f, std::vector<WgradSeg>{WgradSeg{f.B, f.H, f.W, f.OH, f.OW, 0, 0}}, gy, dw, db);
}

// data gradient of forward conv `f` (cached flipped weights): dx (+)= conv^T(gy)
void dgrad(Step &s, const ConvParams &f, View gy, View dx, const float *wflip, bool accumulate) {
  ConvParams q = dgrad_params(f);
  q.in = gy.d; q.in_ld = gy.ld;
  q.wgt = wflip;
  q.out = dx.d; q.out_ld = dx.ld;
  if (accumulate) { q.res = dx.d; q.res_ld = dx.ld; }
  if (f.zcount > 1) {      // (a split-K launch walks blockIdx.z too: the z strides must stay zero for everything else)
    q.zcount = f.zcount; q.z_in_coff = f.z_out_coff; q.z_out_coff = f.z_in_coff; q.z_wgt = (long)f.Cin * f.Cout * f.KH * f.KW;
  }
  s.with_splitk(q);
  s.gemm(GK_DGRAD, q);
  s.dbg("dgrad");
}

// backward of a hand-launched forward GEMM `f` over the rows of x, upstream gradient gy (an activation's adjoint already applied): the
// weight / bias gradients into slots `w` / `b` ("" = no bias), then the data gradient into x's gradient, accumulated iff x already has a
// writer.  Stacked towers (f.zcount > 1) contract one tower at a time and take their data gradients in one launch.
void gemm_bwd(Step &s, const ConvParams &f, View gy, Act *x, const std::string &w, const std::string &b) {
  for (int z = 0; z < f.zcount; ++z) {
    ConvParams fz = f;
    fz.in = f.in + (size_t)z * f.z_in_coff;
    fz.zcount = 1;
    wgrad(s, fz, View{gy.d + (size_t)z * f.z_out_coff, gy.ld}, s.gr(w, (size_t)z * f.z_wgt), b.empty() ? nullptr : s.gr(b, (size_t)z * f.z_bias));
  }
  const bool acc = s.grad_of(x);
  dgrad(s, f, gy, x->g, s.pf(w), acc);
}

// buckets `idx` of a convolution between two levels as the segments of a multi-bucket launch (its data gradient: the levels exchanged)
std::vector<WgradSeg> level_segs(const Level *li, const Level *lo, const std::vector<int> &idx) {
  std::vector<WgradSeg> segs;
  for (int i : idx) segs.push_back(WgradSeg{li->B[i], li->H[i], li->W[i], lo->H[i], lo->W[i], li->off[i], lo->off[i]});
  return segs;
}

struct ConvW {
  std::string name;            // slot of the weight (its flipped copy and gradient share the offset)
  size_t woff = 0;             // extra offset inside the slot
  std::string bias;            // slot of the bias ("" = none)
  size_t boff = 0;
  std::string slope;           // PReLU slope slot
};

View rows_view(View v, long row0) { return View{v.d + row0 * v.ld, v.ld}; }

// y = act(conv(x) + bias + res); registers its backward.  The first `cin` channels of x's view are consumed.  A 1x1 stride-1
// convolution is ONE GEMM over the rows of all buckets (forward, data and weight gradient); a k x k or strided one runs the direct
// kernel per bucket -- or, for the stride-1 3x3 trunk layers whose map the engine's rule sends through F(4x4,3x3), one transform-domain
// GEMM over the tiles of all such buckets, forward and data gradient alike -- and its weight gradient is one contraction over all
// buckets' pixels (launch_wgrad_multi).
Act *conv(Step &s, Act *x, int cin, const ConvW &cw, int cout, int k, int stride, int pad, int dil, int act, Act *res = nullptr, Act *into = nullptr,
          bool need_dx = true) {
  const Level *li = x->lv;
  const int nb = li->nb();
  const bool flat = k == 1 && stride == 1 && pad == 0;
  const Level *lo = li;
  if (!flat) {
    Level o;
    for (int i = 0; i < nb; ++i) o.push(li->B[i], conv_out(li->H[i], k, stride, pad, dil), conv_out(li->W[i], k, stride, pad, dil));
    lo = s.level(o);
  }
  Act *y = into ? into : s.act(lo, cout);
  if (!flat && into) y->lv = lo;
  const float *wp = s.p(cw.name, cw.woff), *bp = cw.bias.empty() ? nullptr : s.p(cw.bias, cw.boff);
  const float *slope = act == ACT_PRELU ? s.p(cw.slope) : nullptr;
  // the launches of the forward pass, kept for the backward closure
  auto plan = std::make_shared<std::vector<ConvParams>>();
  const auto wit = s.t->wino.find(cw.name);
  const bool wino_ok = !flat && wit != s.t->wino.end() && k == 3 && stride == 1 && pad == dil && cw.bias.empty() && act != ACT_PRELU;
  // the buckets by route, split once: `direct` for the direct kernel, `f4` through F(4x4,3x3) (stride 1: input and output levels have the
  // same rows, so the forward pass and the data gradient share the plan).  Padded tiles: see wino.h
  std::vector<int> all, direct, f4;
  for (int i = 0; i < nb; ++i) { all.push_back(i); (wino_ok && wino_route(li->H[i], li->W[i], dil, cin, cout) == 4 ? f4 : direct).push_back(i); }
  const WinoPlan f4plan = wino_plan(*li, f4, dil, 4, false);
  if (flat) {
    ConvParams p = flat_params(x, cin, wp, bp, y, act);
    if (res) { p.res = res->v.d; p.res_ld = res->v.ld; }
    p.prelu = slope;
    s.with_splitk(p);
    plan->push_back(p);
    s.gemm(GK_FWD, p);
  } else {
    for (int i = 0; i < nb; ++i) {
      ConvParams p = bucket_params(x, i, cin, wp, bp, y, k, stride, pad, dil, act);
      if (res) { p.res = res->v.d + lo->off[i] * res->v.ld; p.res_ld = res->v.ld; }
      p.prelu = slope;
      s.with_splitk(p);
      plan->push_back(p);
    }
    if (direct.size() == 1) s.gemm(GK_FWD, (*plan)[direct[0]]);
    else if (!direct.empty()) {      // the direct kernel over all of them in one launch (a workgroup's tile lies inside one bucket)
      ConvParams p = (*plan)[0];
      p.in = x->v.d; p.out = y->v.d;
      if (res) p.res = res->v.d;
      s.gemm_multi(GK_FWD, p, level_segs(li, lo, direct));
    }
    wino_pass(s, s.st, f4plan, x->v.d, x->v.ld, cin, s.dry || !wino_ok ? nullptr : s.t->wino_buf + wit->second.fwd, y->v.d, y->v.ld, cout, res ? res->v.d : nullptr,
              res ? res->v.ld : 0, act, [&](const ConvParams &q) { s.gemm(GK_FWD, q); });
  }
  s.dbg("conv fwd", cw.name);
  s.tape.push_back([=](Step &s) {
    s.dbg("conv bwd begin", cw.name);
    if (act != ACT_NONE) launch_act_bwd(s, y, act, slope, act == ACT_PRELU ? s.gr(cw.slope) : nullptr);
    {   // weight gradient: one contraction over every bucket's pixels
      ConvParams f = (*plan)[0];
      f.in = x->v.d;
      wgrad(s, f, flat ? std::vector<WgradSeg>{WgradSeg{(int)x->rows(), 1, 1, 1, 1, 0, 0}} : level_segs(li, lo, all), y->g, s.gr(cw.name, cw.woff),
            cw.bias.empty() ? nullptr : s.gr(cw.bias, cw.boff));
    }
    if (need_dx) {
      const bool acc = s.grad_of(x);
      if (flat) dgrad(s, (*plan)[0], y->g, x->g, s.pf(cw.name, cw.woff), acc);
      else {
        if (stride != 1) {
          // strided: dcol[m][tap * cin + c] = sum_n dY[m][n] w[n][tap][c] for every OUTPUT pixel m -- one GEMM over the rows of all buckets
          // against the plain transpose of the packed weights -- then every input pixel gathers the (tap, output pixel) pairs that read it
          // (col2im_multi_kernel).  (The dilated-input form of the direct kernel multiplies 3/4 zeros at stride 2 and runs per bucket.)
          const int kk = k * k * cin;
          const size_t mark = s.off;
          float *dcol = s.f((size_t)lo->rows * kk);
          ConvParams q;
          q.in = y->g.d; q.B = (int)lo->rows; q.Cin = cout; q.in_ld = y->g.ld;
          q.wgt = s.pf(cw.name, cw.woff);
          q.out = dcol; q.Cout = kk; q.out_ld = kk;
          s.with_splitk(q);
          s.gemm(GK_DGRAD, q);
          if (s.live())
            for (const BTab &t : make_tabs(li, lo))
              hipLaunchKernelGGL(col2im_multi_kernel, dim3(nblk(tab_rows(t) * (cin / 4))), dim3(TB), 0, s.st, dcol, x->g.d, x->g.ld, cin, k, stride, pad, dil,
                                 acc ? 1 : 0, t);
          s.off = mark;
        } else if (direct.size() == 1)
          for (int i : direct) dgrad(s, (*plan)[i], rows_view(y->g, lo->off[i]), rows_view(x->g, li->off[i]), s.pf(cw.name, cw.woff), acc);
        else if (!direct.empty()) {
          ConvParams q = dgrad_params((*plan)[0]);
          q.B = q.H = q.W = q.OH = q.OW = 1;      // (the buckets carry the geometry)
          q.in = y->g.d; q.in_ld = y->g.ld;
          q.wgt = s.pf(cw.name, cw.woff);
          q.out = x->g.d; q.out_ld = x->g.ld;
          if (acc) { q.res = x->g.d; q.res_ld = x->g.ld; }
          s.gemm_multi(GK_DGRAD, q, level_segs(lo, li, direct));
        }
        wino_pass(s, s.st, f4plan, y->g.d, y->g.ld, cout, s.dry || !wino_ok ? nullptr : s.t->wino_buf + wit->second.bwd, x->g.d, x->g.ld, cin, acc ? x->g.d : nullptr,
                  x->g.ld, ACT_NONE, [&](const ConvParams &q) { s.gemm(GK_DGRAD, q); });
      }
    }
    if (res) {
      if (!res->gset) { res->g = y->g; res->gset = true; }          // the residual's gradient IS this (masked) gradient: alias, no copy
      else if (s.live()) hipLaunchKernelGGL(add2d_kernel, dim3(nblk(y->rows() * (y->C / 4))), dim3(TB), 0, s.st, res->g.d, res->g.ld, y->g.d, y->g.ld,
                                            y->rows(), y->C / 4);
    }
  });
  return y;
}

// channel view [c0, c0 + C) of a wider activation record (shares storage; its gradient view is resolved lazily by the caller)
Act *slice(Step &s, Act *a, int c0, int C) {
  s.acts.emplace_back();
  Act *v = &s.acts.back();
  *v = *a;
  v->v.d = a->v.d + c0;
  v->C = C;
  v->g = View{};
  v->gset = false;
  return v;
}
// ... resolved: the gradient of `part` (channels from c0 of `whole`) lives in whole's gradient buffer, which must exist by now.  written:
// that buffer already holds part's gradient, so the next producer into it accumulates; false: the next producer is the first writer
void alias_grad(Act *part, const Act *whole, int c0, bool written = true) {
  part->g = View{whole->g.d + c0, whole->g.ld};
  part->gset = written;
}

int check_flips(Trainer &t, const float *P, long version, hipStream_t st) {
  if (!t.wflip || !t.flip_tiles || (t.wino_floats && !t.wino_buf))
    return set_error(DF_ERR_STATE, "trainer: created without a device (no arena or tile table for the data gradients' weight copies)");
  if (t.flip_version == version && t.flip_src == P && version >= 0) return DF_OK;
  hipLaunchKernelGGL(flip_tiles_kernel, dim3(t.flip_ntiles), dim3(256), 0, st, P, t.wflip, t.flip_tiles, (int)t.flips.size());
  {   // the F(4x4,3x3)-domain copies, forward (of the packed weights) and data gradient (of the flipped ones: [I][9][O]): one launch per 32
    WinoWTab tab;
    tab.n = 0; tab.e0[0] = 0;
    auto flush = [&]() { launch_wino4_weight_multi(P, t.wflip, t.wino_buf, tab, st); tab.n = 0; tab.e0[0] = 0; };
    auto push = [&](int O, int C, int from_b, long src, long dst) {
      if (tab.n == WINO_WMAX) flush();
      const int g = tab.n++;
      tab.O[g] = O; tab.C[g] = C; tab.from_b[g] = from_b; tab.src_off[g] = src; tab.dst_off[g] = dst;
      tab.e0[g + 1] = tab.e0[g] + (long)O * C;
    };
    for (const auto &kv : t.wino) {
      const Trainer::Wino &w = kv.second;
      push(w.O, w.I, 0, (long)w.w_off, (long)w.fwd);
      push(w.I, w.O, 1, (long)w.w_off, (long)w.bwd);
    }
    flush();
  }
  t.flip_version = version;
  t.flip_src = P;
  return check_launch("trainer: weight flips");
}

// ------------------------------------------------------------------------------------------------
// the two halves of a network's C ABI: `walk(Step &)` is posenet_step / refiner_step bound to its arguments
// ------------------------------------------------------------------------------------------------
// workspace bytes of a step: the sizing pass walks the whole step without a device; cached per shape `key`
template <class Walk> size_t sized_workspace(Trainer &t, const std::vector<int> &key, Walk walk) {
  auto it = t.ws_cache.find(key);
  if (it != t.ws_cache.end()) return it->second;
  Step s(&t, nullptr);
  walk(s);
  if (t.ws_cache.size() > 4096) t.ws_cache.clear();
  t.ws_cache[key] = s.peak;
  return s.peak;
}
// one step on the caller's workspace and stream, after its argument checks; `what` names it in a launch error
template <class Walk> int run_step(Trainer &t, const float *flat_param, float *flat_grad, int64_t param_version, void *ws, size_t ws_bytes, df_stream_t stream,
                                   const char *what, Walk walk) {
  const int rc = check_flips(t, flat_param, (long)param_version, to_stream(stream));
  if (rc != DF_OK) return rc;
  Step s(&t, to_stream(stream), Arena(ws, ws_bytes));
  s.P = flat_param; s.G = flat_grad;
  walk(s);
  if (s.err != DF_OK) return s.err;
  return check_launch(what);
}

}  // namespace
}  // namespace df
