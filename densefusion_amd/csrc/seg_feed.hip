// From rendered customCAD scenes to SegNet training batches on the device: per item a window of a rendered frame is composited over a
// background where nothing was drawn, blurred, given pixel noise, flipped, normalised and written as the channels-last input and the
// int64 target SegNet trains on, with the item's class pixel counts.  The contract is the comment of df_seg_batch in include/dfusion.h
// (steps G1..G5); the per-pixel rule is seg_feed_core.h; tests/seg_feed_np.py restates it in numpy and the outputs are compared bit
// for bit.
//
// Steps on the caller's stream: the counts are set to zero; seg_batch_kernel, grid = (tiles of the OUTPUT window, items).  The call is
// store-bound (24 bytes written per pixel, 5 to 8 read), so the tiling follows the stores: a workgroup owns TH x TW output pixels, a
// half-wave one row of TW = 32 at a time, a lane one float4 of x and one int64 of the target, so that each half of a wave-instruction
// writes 512 and 256 contiguous bytes -- whole 256-byte segments where W is a multiple of 16 -- whatever the flip.  The flip is applied
// on the way IN: the source tile of an output tile is the mirrored range of the window, and a lane reads the mirrored LDS cell.  The
// source tile and its one-pixel halo are composited once into LDS, one packed word per pixel (colour in bytes 0..2, class in byte 3),
// the indices clamped to the window, which is the blur's edge rule; a half-wave reads 32 consecutive words, in either direction, so
// its dword reads meet no bank twice.  Class counts: a wave ballots per class present among its pixels, one LDS add per class and
// wave, then at most one integer atomicAdd per non-zero class per workgroup.
#include "cad_frame.h"
#include "seg_feed_core.h"

namespace df {
namespace {

using segfeed::ClassMap;
using segfeed::Item;
using segfeed::Source;

constexpr int TW = 32, TH = 16;                  // output tile: half-wave h takes rows h, h + 8 of it
constexpr int SB = 256;
constexpr int LW = TW + 2, LH = TH + 2;          // the source tile with its halo
constexpr size_t SEG_SCRATCH = 256;              // nothing is kept in memory between steps today; the size is reserved

__global__ __launch_bounds__(SB) void seg_batch_kernel(Source src, int F, int NB, ClassMap cm, int C, const int *__restrict__ desc, int H,
                                                       int W, int tiles_x, int blur, int noise_mul, f32x4 *__restrict__ x_out,
                                                       int64_t *__restrict__ target_out, int *__restrict__ counts_out) {
  __shared__ unsigned tile[LH * LW];
  __shared__ int hist[segfeed::MAX_CLASSES];
  const int n = blockIdx.y, t = threadIdx.x, lane = t & 63, col = t & (TW - 1), row = t / TW;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int i0 = ty * TH, j0 = tx * TW;          // the tile's first output row and column
  const Item it = segfeed::load_item(desc + (size_t)n * 8);
  const size_t obase = (size_t)n * H * W;
  const int jo = j0 + col;
  if (!segfeed::item_ok(it, F, src.IH, src.IW, H, W, NB, src.BH, src.BW)) {   // uniform over the workgroup: zeros, nothing read
    for (int r = row; r < TH; r += SB / TW) {
      const int io = i0 + r;
      if (io < H && jo < W) {
        x_out[obase + (size_t)io * W + jo] = f32x4{0.f, 0.f, 0.f, 0.f};
        target_out[obase + (size_t)io * W + jo] = 0;
      }
    }
    return;
  }
  const int fx = it.flip & 1, fy = (it.flip >> 1) & 1;
  // the source tile's first row and column; below zero on the partial tiles of a flipped axis, where the clamp below takes over
  const int si0 = fy ? H - TH - i0 : i0, sj0 = fx ? W - TW - j0 : j0;
  if (t < segfeed::MAX_CLASSES) hist[t] = 0;
  for (int idx = t; idx < LH * LW; idx += SB) {
    const int li = idx / LW, lj = idx - li * LW;
    int i = si0 - 1 + li, j = sj0 - 1 + lj;
    i = i < 0 ? 0 : (i > H - 1 ? H - 1 : i);
    j = j < 0 ? 0 : (j > W - 1 ? W - 1 : j);
    tile[idx] = segfeed::composite_pixel(src, cm, it, i, j);
  }
  __syncthreads();
  for (int r = row; r < TH; r += SB / TW) {
    const int io = i0 + r;
    const bool live = io < H && jo < W;
    int cls = -1;
    if (live) {
      const int i = segfeed::flipped(io, H, fy), j = segfeed::flipped(jo, W, fx);
      const unsigned *own = tile + (i - si0 + 1) * LW + (j - sj0 + 1);
      const unsigned v = segfeed::finish_pixel([own](int di, int dj) { return own[di * LW + dj]; }, (unsigned)(i * W + j), blur, it.seed,
                                               noise_mul);
      cls = (int)(v >> 24);
      x_out[obase + (size_t)io * W + jo] = seg_norm(v & 0xffu, (v >> 8) & 0xffu, (v >> 16) & 0xffu);
      target_out[obase + (size_t)io * W + jo] = cls;
    }
    unsigned long long rem = __ballot(live);      // the classes present among this wave's pixels, lowest lane first
    while (rem) {
      const int c = __shfl(cls, __ffsll((long long)rem) - 1);
      const unsigned long long m = __ballot(cls == c);
      if (lane == 0) atomicAdd(&hist[c], __popcll(m));
      rem &= ~m;
    }
  }
  __syncthreads();
  if (t < C && hist[t]) atomicAdd(&counts_out[(size_t)n * C + t], hist[t]);
}

}  // namespace
}  // namespace df

using namespace df;

extern "C" size_t df_seg_batch_scratch_bytes(int B, int H, int W, int C) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || (long)H * W > (1L << 24) || C < 1 || C > segfeed::MAX_CLASSES) return 0;
  return SEG_SCRATCH;
}

extern "C" int df_seg_batch(const unsigned char *rgb, const unsigned short *label, int F, int IH, int IW, const unsigned char *back, int NB,
                            int BH, int BW, const int *class_map, int O, int C, const int *desc, int B, int H, int W, int blur,
                            int noise_mul, float *x_out, int64_t *target_out, int *counts_out, void *scratch, size_t scratch_bytes,
                            df_stream_t stream) {
  const char *name = "seg_batch";
  if (!rgb || !label || !class_map || !desc || !x_out || !target_out || !counts_out || !scratch)
    return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (NB < 0 || (NB == 0) != (back == nullptr)) return set_error(DF_ERR_ARG, "%s: back must be NULL exactly when NB == 0 (NB %d)", name, NB);
  if (!sizes_ok(F, IH, IW)) return set_error(DF_ERR_ARG, "%s: bad sizes", name);
  if (H < 1 || H > IH || W < 1 || W > IW || (long)H * W > (1L << 24))
    return set_error(DF_ERR_ARG, "%s: window %d x %d outside the %d x %d frame, or above 2^24 pixels", name, H, W, IH, IW);
  if (B < 1 || B > 65535) return set_error(DF_ERR_ARG, "%s: B = %d outside 1..65535", name, B);
  if (O < 1 || O > segfeed::MAX_OBJECTS || C < 1 || C > segfeed::MAX_CLASSES)
    return set_error(DF_ERR_ARG, "%s: O = %d or C = %d outside 1..64", name, O, C);
  ClassMap cm = {};
  for (int l = 0; l <= O; ++l) {
    if (class_map[l] < 0 || class_map[l] >= C || (l == 0 && class_map[0] != 0))
      return set_error(DF_ERR_ARG, "%s: class_map[%d] = %d (need 0..C-1, and 0 for label 0)", name, l, class_map[l]);
    cm.cls[l] = (unsigned char)class_map[l];
  }
  if (NB > 0 && (BH < H || BW < W)) return set_error(DF_ERR_ARG, "%s: %d x %d backgrounds are smaller than the window", name, BH, BW);
  if (blur < 0 || blur > 1) return set_error(DF_ERR_ARG, "%s: blur %d outside 0..1", name, blur);
  if (noise_mul < 0) return set_error(DF_ERR_ARG, "%s: noise_mul %d is negative", name, noise_mul);
  if (reinterpret_cast<uintptr_t>(x_out) % 16 || reinterpret_cast<uintptr_t>(target_out) % 8 || reinterpret_cast<uintptr_t>(counts_out) % 4 ||
      reinterpret_cast<uintptr_t>(desc) % 4 || reinterpret_cast<uintptr_t>(label) % 2)
    return set_error(DF_ERR_ARG, "%s: x_out must be 16-byte, target_out 8-byte, counts_out and desc 4-byte, label 2-byte aligned", name);
  const size_t need = df_seg_batch_scratch_bytes(B, H, W, C);
  if (need == 0 || scratch_bytes < need) return set_error(DF_ERR_ARG, "%s: scratch of %zu bytes, need %zu", name, scratch_bytes, need);
  hipStream_t st = to_stream(stream);
  if (hipMemsetAsync(counts_out, 0, sizeof(int) * (size_t)B * C, st) != hipSuccess) return check_launch(name);
  const int tiles_x = cdiv(W, TW), tiles_y = cdiv(H, TH);   // H * W <= 2^24: at most 2^24 tiles
  const Source src = {rgb, label, back, IH, IW, NB > 0 ? BH : 0, NB > 0 ? BW : 0, O};
  hipLaunchKernelGGL(seg_batch_kernel, dim3((unsigned)tiles_x * tiles_y, B), dim3(SB), 0, st, src, F, NB, cm, C, desc, H, W, tiles_x, blur,
                     noise_mul, reinterpret_cast<f32x4 *>(x_out), target_out, counts_out);
  return check_launch(name);
}
