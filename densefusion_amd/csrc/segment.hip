// From an RGB-D window to per-frame detections on the device (the RGB-D frame -> SegNet -> per-object mask and box step that feeds
// the pose stage, densefusion_amd/lib/segment.py):
//   * the SegNet input: uint8 RGB [F][H][W][3] -> the normalised fp32 NHWC4 tensor of the eval path (data_controller.py:79);
//   * the label map (arg-max over the first C of ld channels-last logits), per (frame, class) the pixel count, the count with
//     depth != 0 and the tight box, and the detection table: classes 1..num_obj with more than min_pixels depth-valid pixels.
//
// No atomics anywhere: every workgroup covers a fixed pixel range of ONE frame (the partition depends on H x W only) and writes its
// partial row; a finish pass combines a frame's rows.  All statistics are integers, so two calls are bit-identical and a frame's
// results do not depend on the window it is in.
#include <climits>

#include "common.h"
#include "seg_argmax.h"
#include "seg_norm.h"

namespace df {
namespace {

constexpr int TB = 256;              // threads of the label pass = pixels per tile
constexpr int SEG_PPB = 4096;        // pixels per workgroup of the label pass
constexpr int SEG_MAX_C = 64;        // classes: lane c of a wave keeps class c's running statistics
constexpr int SEG_MAX_LD4 = 16;      // ld <= 64 (float4 loads in flight per lane)
constexpr int NF = 6;                // per (workgroup, class): count, depth-valid count, rmin, rmax, cmin, cmax (inclusive)
constexpr int FIN_TB = 1024;         // finish: 16 lane groups per frame add the partial rows g, g + 16, ...

inline int seg_parts(long hw) { return cdiv(hw, SEG_PPB); }

// four pixels per lane (seg_norm: seg_norm.h): three aligned dword loads (12 bytes), four float4 stores; the npix % 4 tail pixel by pixel
__global__ __launch_bounds__(TB) void seg_input_kernel(const unsigned char *__restrict__ rgb, float *__restrict__ out, long npix) {
  f32x4 *o4 = reinterpret_cast<f32x4 *>(out);
  const long nq = npix / 4;
  for (long q = blockIdx.x * (long)TB + threadIdx.x; q < nq; q += (long)gridDim.x * TB) {
    const unsigned *s = reinterpret_cast<const unsigned *>(rgb) + 3 * q;
    const unsigned w0 = s[0], w1 = s[1], w2 = s[2];
    o4[4 * q + 0] = seg_norm(w0 & 0xffu, (w0 >> 8) & 0xffu, (w0 >> 16) & 0xffu);
    o4[4 * q + 1] = seg_norm(w0 >> 24, w1 & 0xffu, (w1 >> 8) & 0xffu);
    o4[4 * q + 2] = seg_norm((w1 >> 16) & 0xffu, w1 >> 24, w2 & 0xffu);
    o4[4 * q + 3] = seg_norm((w2 >> 8) & 0xffu, (w2 >> 16) & 0xffu, w2 >> 24);
  }
  if (blockIdx.x == 0) {
    const long p = 4 * nq + threadIdx.x;
    if (p < npix) o4[p] = seg_norm(rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]);
  }
}

// Label pass.  Grid (parts, F); workgroup b of frame f covers pixels [b SEG_PPB, (b + 1) SEG_PPB) of the frame in tiles of TB
// pixels.  A tile's logits (TB x ld floats, contiguous) come in with coalesced float4 loads, issued one tile ahead into registers,
// and go through LDS (rows of s = (ld / 4) | 1 float4s: an odd stride, so a lane's row reads are free of bank conflicts); lane t then
// takes the arg-max of pixel t over the first C channels (seg_argmax.h: first maximum wins, NaN counts as maximal, torch.argmax).
// Statistics: per tile, each wave walks the classes present among its 64 pixels (ballots); lane c of the wave adds class c's share
// to its running count / depth-valid count / box.  The waves meet in LDS at the end and lane c writes the workgroup's row for class c.
// MAXN4: the float4s per pixel the registers hold (8: ld <= 32, 16: ld <= 64).
template <int MAXN4>
__global__ __launch_bounds__(TB) void seg_label_stats_kernel(const float *__restrict__ logits, const unsigned short *__restrict__ depth,
                                                             int HW, int W, int ld, int C, int parts, int *__restrict__ label,
                                                             int *__restrict__ part) {
  extern __shared__ f32x4 tile[];
  __shared__ int wave_acc[TB / 64][SEG_MAX_C][NF];
  const int f = blockIdx.y, b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int n4 = ld >> 2, s = n4 | 1;
  const long fbase = (long)f * HW;
  const int p0 = b * SEG_PPB, p1 = p0 + SEG_PPB < HW ? p0 + SEG_PPB : HW;
  const f32x4 *src = reinterpret_cast<const f32x4 *>(logits) + fbase * n4;
  int cnt = 0, nv = 0, rmin = INT_MAX, rmax = -1, cmin = INT_MAX, cmax = -1;
  f32x4 reg[MAXN4];
  unsigned short dreg = 0;
  {
    const int np = p1 - p0 < TB ? p1 - p0 : TB, tot = np * n4;
#pragma unroll
    for (int k = 0; k < MAXN4; ++k)
      if (k < n4 && t + k * TB < tot) reg[k] = src[(long)p0 * n4 + t + k * TB];
    if (t < np) dreg = depth[fbase + p0 + t];
  }
  for (int q0 = p0; q0 < p1; q0 += TB) {
    const int np = p1 - q0 < TB ? p1 - q0 : TB, tot = np * n4;
    __syncthreads();                                           // the previous tile's readers are done
#pragma unroll
    for (int k = 0; k < MAXN4; ++k) {
      const int i = t + k * TB;
      if (k < n4 && i < tot) {
        const int px = i / n4;
        tile[px * s + (i - px * n4)] = reg[k];
      }
    }
    const unsigned short d = dreg;
    __syncthreads();
    const int q1 = q0 + TB;
    if (q1 < p1) {                                             // next tile's loads in flight under this tile's arg-max
      const int np1 = p1 - q1 < TB ? p1 - q1 : TB, tot1 = np1 * n4;
#pragma unroll
      for (int k = 0; k < MAXN4; ++k)
        if (k < n4 && t + k * TB < tot1) reg[k] = src[(long)q1 * n4 + t + k * TB];
      if (t < np1) dreg = depth[fbase + q1 + t];
    }
    const int p = q0 + t;
    int lab = -1;
    if (t < np) {
      lab = seg_argmax(tile + t * s, C);
      label[fbase + p] = lab;
    }
    const int row = p / W, col = p - row * W;
    unsigned long long rem = __ballot(lab >= 0);
    while (rem) {                                              // the classes present in this wave's pixels, lowest lane first
      const int first = __ffsll((long long)rem) - 1;
      const int c = __shfl(lab, first);
      const unsigned long long m = __ballot(lab == c), mv = __ballot(lab == c && d != 0);
      const int last = 63 - __clzll((long long)m);
      const int r0 = __shfl(row, first), r1 = __shfl(row, last);
      int c0, c1;
      if (r0 == r1) {                                          // pixels run along one row: the outermost lanes bound the columns
        c0 = __shfl(col, first);
        c1 = __shfl(col, last);
      } else {
        c0 = lab == c ? col : INT_MAX;
        c1 = lab == c ? col : -1;
        for (int o = 32; o > 0; o >>= 1) {
          const int a0 = __shfl_xor(c0, o), a1 = __shfl_xor(c1, o);
          c0 = a0 < c0 ? a0 : c0;
          c1 = a1 > c1 ? a1 : c1;
        }
      }
      if (lane == c) {
        cnt += __popcll(m);
        nv += __popcll(mv);
        rmin = r0 < rmin ? r0 : rmin;
        rmax = r1 > rmax ? r1 : rmax;
        cmin = c0 < cmin ? c0 : cmin;
        cmax = c1 > cmax ? c1 : cmax;
      }
      rem &= ~m;
    }
  }
  if (lane < C) {
    int *a = wave_acc[wv][lane];
    a[0] = cnt; a[1] = nv; a[2] = rmin; a[3] = rmax; a[4] = cmin; a[5] = cmax;
  }
  __syncthreads();
  if (t < C) {
    int r[NF];
    for (int k = 0; k < NF; ++k) r[k] = wave_acc[0][t][k];
    for (int w = 1; w < TB / 64; ++w) {
      const int *a = wave_acc[w][t];
      r[0] += a[0]; r[1] += a[1];
      r[2] = a[2] < r[2] ? a[2] : r[2];
      r[3] = a[3] > r[3] ? a[3] : r[3];
      r[4] = a[4] < r[4] ? a[4] : r[4];
      r[5] = a[5] > r[5] ? a[5] : r[5];
    }
    int *o = part + (((long)f * parts + b) * C + t) * NF;
    for (int k = 0; k < NF; ++k) o[k] = r[k];
  }
}

// Finish, one workgroup per frame: lane group g (16 of them) combines the partial rows g, g + 16, ... of class c = lane, the groups
// meet in LDS.  Wave 0 then writes stats [C][6] = {count, n_valid, rmin, rmax_excl, cmin, cmax_excl} (zeros for an absent class) and
// lists the classes 1..num_obj with n_valid > min_pixels, ascending, as det rows {cls, rmin, rmax_excl, cmin, cmax_excl, n_valid}; the
// rows after the last detection are zero and ndet holds the count.
__global__ __launch_bounds__(FIN_TB) void seg_finish_kernel(const int *__restrict__ part, int parts, int C, int num_obj, int min_pixels,
                                                            int *__restrict__ stats, int *__restrict__ det, int *__restrict__ ndet) {
  constexpr int G = FIN_TB / 64;
  __shared__ int acc[G][SEG_MAX_C][NF];
  const int f = blockIdx.x, c = threadIdx.x & 63, g = threadIdx.x >> 6;
  int r[NF] = {0, 0, INT_MAX, -1, INT_MAX, -1};
  if (c < C) {
#pragma unroll 4
    for (int k = g; k < parts; k += G) {
      const int *a = part + (((long)f * parts + k) * C + c) * NF;
      const int a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5];
      r[0] += a0; r[1] += a1;
      r[2] = a2 < r[2] ? a2 : r[2];
      r[3] = a3 > r[3] ? a3 : r[3];
      r[4] = a4 < r[4] ? a4 : r[4];
      r[5] = a5 > r[5] ? a5 : r[5];
    }
    for (int k = 0; k < NF; ++k) acc[g][c][k] = r[k];
  }
  __syncthreads();
  if (g != 0) return;
  int flag = 0;
  if (c < C) {
    for (int h = 1; h < G; ++h) {
      const int *a = acc[h][c];
      r[0] += a[0]; r[1] += a[1];
      r[2] = a[2] < r[2] ? a[2] : r[2];
      r[3] = a[3] > r[3] ? a[3] : r[3];
      r[4] = a[4] < r[4] ? a[4] : r[4];
      r[5] = a[5] > r[5] ? a[5] : r[5];
    }
    const bool any = r[0] > 0;
    int *o = stats + ((long)f * C + c) * NF;
    o[0] = r[0]; o[1] = r[1];
    o[2] = any ? r[2] : 0; o[3] = any ? r[3] + 1 : 0;
    o[4] = any ? r[4] : 0; o[5] = any ? r[5] + 1 : 0;
    flag = c >= 1 && c <= num_obj && r[1] > min_pixels;
  }
  const unsigned long long m = __ballot(flag);
  const int n = __popcll(m);
  int *drow = det + (long)f * C * NF;
  if (flag) {
    int *o = drow + __popcll(m & ((1ull << c) - 1)) * NF;
    o[0] = c; o[1] = r[2]; o[2] = r[3] + 1; o[3] = r[4]; o[4] = r[5] + 1; o[5] = r[1];
  }
  if (c < C && c >= n)
    for (int k = 0; k < NF; ++k) drow[c * NF + k] = 0;
  if (c == 0) ndet[f] = n;
}

}  // namespace
}  // namespace df

using namespace df;
#define ST to_stream(stream)
#define NN(p) if (!(p)) return set_error(DF_ERR_ARG, "%s: null pointer", __func__)

extern "C" size_t df_segment_scratch_bytes(int F, int H, int W, int C) {
  if (F < 1 || H < 1 || W < 1 || C < 1 || C > SEG_MAX_C || (long)H * W > INT_MAX) return 0;
  return (size_t)F * seg_parts((long)H * W) * C * NF * sizeof(int);
}

extern "C" int df_segment_input(const unsigned char *rgb, float *out, int F, int H, int W, df_stream_t stream) {
  NN(rgb); NN(out);
  if (F < 1 || H < 1 || W < 1) return set_error(DF_ERR_ARG, "segment_input: need F, H, W >= 1");
  if (reinterpret_cast<uintptr_t>(rgb) % 4 || reinterpret_cast<uintptr_t>(out) % 16)
    return set_error(DF_ERR_ARG, "segment_input: rgb must be 4-byte and out 16-byte aligned");
  const long npix = (long)F * H * W;
  long nb = (npix / 4 + TB - 1) / TB;
  nb = nb < 1 ? 1 : (nb > 8192 ? 8192 : nb);
  hipLaunchKernelGGL(seg_input_kernel, dim3((unsigned)nb), dim3(TB), 0, ST, rgb, out, npix);
  return check_launch("segment_input");
}

extern "C" int df_segment_detect(const float *logits, const unsigned short *depth, int F, int H, int W, int ld, int C, int num_obj,
                                 int min_pixels, int *label, int *stats, int *det, int *ndet, void *scratch, size_t scratch_bytes,
                                 df_stream_t stream) {
  NN(logits); NN(depth); NN(label); NN(stats); NN(det); NN(ndet); NN(scratch);
  if (F < 1 || H < 1 || W < 1 || (long)H * W > INT_MAX) return set_error(DF_ERR_ARG, "segment_detect: bad frame size");
  if (C < 1 || C > SEG_MAX_C || ld < C || ld % 4 || ld > 4 * SEG_MAX_LD4)
    return set_error(DF_ERR_ARG, "segment_detect: need 1 <= C <= %d, C <= ld <= %d, ld a multiple of 4 (C %d, ld %d)", SEG_MAX_C,
                     4 * SEG_MAX_LD4, C, ld);
  if (num_obj < 0 || num_obj >= C) return set_error(DF_ERR_ARG, "segment_detect: need 0 <= num_obj < C");
  if (reinterpret_cast<uintptr_t>(logits) % 16) return set_error(DF_ERR_ARG, "segment_detect: logits must be 16-byte aligned");
  if (scratch_bytes < df_segment_scratch_bytes(F, H, W, C))
    return set_error(DF_ERR_WORKSPACE, "segment_detect: scratch of %zu bytes, need %zu", scratch_bytes, df_segment_scratch_bytes(F, H, W, C));
  const int HW = H * W, parts = seg_parts(HW);
  const int lds = TB * ((ld / 4) | 1) * (int)sizeof(f32x4);
  int *part = static_cast<int *>(scratch);
  if (ld <= 32) {
    hipLaunchKernelGGL(seg_label_stats_kernel<8>, dim3(parts, F), dim3(TB), lds, ST, logits, depth, HW, W, ld, C, parts, label, part);
  } else {
    // above 64 KiB of dynamic LDS from ld 56 on; the limit is set once per kernel, to the largest tile it takes
    if (int e = raise_lds_limit(reinterpret_cast<const void *>(seg_label_stats_kernel<SEG_MAX_LD4>), TB * (SEG_MAX_LD4 | 1) * (int)sizeof(f32x4)))
      return e;
    hipLaunchKernelGGL(seg_label_stats_kernel<SEG_MAX_LD4>, dim3(parts, F), dim3(TB), lds, ST, logits, depth, HW, W, ld, C, parts, label, part);
  }
  hipLaunchKernelGGL(seg_finish_kernel, dim3(F), dim3(FIN_TB), 0, ST, part, parts, C, num_obj, min_pixels, stats, det, ndet);
  return check_launch("segment_detect");
}
