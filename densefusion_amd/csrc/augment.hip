// Training-time pixel augmentation on the device: the colour jitter of densefusion_amd/datasets/augment.py (a restatement of the pinned
// torchvision's ColorJitter over PIL) and the YCB frame composition of datasets/ycb/dataset.py (synthetic frame over a real background,
// occluders in front), both on whole uint8 frames [F][H][W][3] and both bit-identical to the host path: every step is 8-bit or plain
// IEEE arithmetic.  The random draws stay on the host (augment.ColorJitter.draw); a plan row carries them here.
//
// Jitter, per pixel, in the plan's order, each operation's output rounded to u8 before the next one starts:
//   L (PIL convert("L"))   (R*19595 + G*38470 + B*7471 + 0x8000) >> 16
//   blend                  t = d + a*(x - d) in fp32, a product then a sum (PIL's Image.blend; no fused multiply-add), clamped, truncated;
//                          d = 0 (brightness), the frame's mean L (contrast), the pixel's L (saturation)
//   contrast mean          int(mean(L) + 0.5) of the whole frame AS IT STANDS when contrast is applied = (2*sum + n) / (2*n) in integers:
//                          pass 1 applies the operations ordered before contrast in registers and adds up L -- wave shuffle, LDS across
//                          the waves, ONE integer atomicAdd per workgroup (integer sums are exact in any order); pass 2 applies all
//   hue                    RGB -> HSV, H = (H + shift) & 0xFF, HSV -> RGB, PIL's conversions: fp32 / double exactly as written below
// Four pixels are three dwords: frames whose bytes start on a dword boundary go through dword loads and stores (H*W % 4 pixels left over
// go one by one), the others (only when H*W*3 % 4 != 0 and F > 1) pixel by pixel.
#include "common.h"

#pragma clang fp contract(off)

namespace df {
namespace {

constexpr int JB = 256;              // threads of the storing kernels
constexpr int MB = 1024;             // threads of pass 1: a frame's workgroups all add to ONE word, and same-address atomics take their turns in
                                     // memory -- 75 of them per 480x640 frame instead of 300
constexpr int JIT_MAX_BLOCKS_X = 4096;
constexpr int OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3;      // anything else: no operation

struct JitterPlan {
  float alpha[3];      // brightness, contrast, saturation
  unsigned shift;      // hue
  int op[4];
};

__device__ __forceinline__ JitterPlan load_plan(const float *__restrict__ row) {
  JitterPlan p;
  p.alpha[0] = row[0]; p.alpha[1] = row[1]; p.alpha[2] = row[2];
  p.shift = (unsigned)(int)row[3] & 0xffu;
#pragma unroll
  for (int k = 0; k < 4; ++k) p.op[k] = (int)row[4 + k];
  return p;
}

struct Px { unsigned r, g, b; };

__device__ __forceinline__ unsigned luma(Px p) { return (p.r * 19595u + p.g * 38470u + p.b * 7471u + 0x8000u) >> 16; }

__device__ __forceinline__ unsigned blend(float d, float a, unsigned x) {
  const float t = __fadd_rn(d, __fmul_rn(a, __fsub_rn((float)x, d)));
  return t <= 0.f ? 0u : (t >= 255.f ? 255u : (unsigned)t);
}

__device__ __forceinline__ Px blend(float d, float a, Px p) { return Px{blend(d, a, p.r), blend(d, a, p.g), blend(d, a, p.b)}; }

__device__ __forceinline__ unsigned clip8(int v) { return v < 0 ? 0u : (v > 255 ? 255u : (unsigned)v); }

__device__ __forceinline__ Px hue(Px p, unsigned shift) {
  const unsigned maxi = max(p.r, max(p.g, p.b)), mini = min(p.r, min(p.g, p.b));
  unsigned H = 0, S = 0;
  const unsigned V = maxi;
  if (maxi != mini) {
    const float maxc = (float)maxi, cr = (float)(maxi - mini);
    const float s = cr / maxc;
    const float rc = (maxc - (float)p.r) / cr, gc = (maxc - (float)p.g) / cr, bc = (maxc - (float)p.b) / cr;
    float h;
    if (p.r == maxi) h = bc - gc;
    else if (p.g == maxi) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    const double x = (double)h / 6.0 + 1.0;          // in [5/6, 11/6]
    h = (float)(x - floor(x));                       // fmod(x, 1.0): exact
    H = clip8((int)((double)h * 255.0));
    S = clip8((int)((double)s * 255.0));
  }
  H = (H + shift) & 0xffu;
  if (S == 0) return Px{V, V, V};
  const double hh = (double)H * 6.0 / 255.0, fi = floor(hh), f = hh - fi, fs = (double)S / 255.0, v = (double)V;
  const unsigned pp = clip8((int)rint(v * (1.0 - fs)));
  const unsigned q = clip8((int)rint(v * (1.0 - fs * f)));
  const unsigned t = clip8((int)rint(v * (1.0 - fs * (1.0 - f))));
  switch ((int)fi % 6) {
    case 0: return Px{V, t, pp};
    case 1: return Px{q, V, pp};
    case 2: return Px{pp, V, t};
    case 3: return Px{pp, q, V};
    case 4: return Px{t, pp, V};
    default: return Px{V, pp, q};
  }
}

// operations [0, stop) of the plan; `mean`: the contrast degenerate (unused when contrast is not among them)
__device__ __forceinline__ Px apply_ops(Px p, const JitterPlan &pl, int stop, float mean) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {          // unrolled: the plan stays in registers
    if (k >= stop) break;
    const int op = pl.op[k];
    if (op == OP_BRIGHTNESS) p = blend(0.f, pl.alpha[0], p);
    else if (op == OP_CONTRAST) p = blend(mean, pl.alpha[1], p);
    else if (op == OP_SATURATION) p = blend((float)luma(p), pl.alpha[2], p);
    else if (op == OP_HUE) p = hue(p, pl.shift);
  }
  return p;
}

__device__ __forceinline__ int contrast_slot(const JitterPlan &pl) {
  int slot = -1;
#pragma unroll
  for (int k = 3; k >= 0; --k)
    if (pl.op[k] == OP_CONTRAST) slot = k;
  return slot;
}

// Walks one frame's pixels with the workgroups of grid row blockIdx.y: fn(Px) -> Px per pixel; STORE writes the result to dst.
template <bool STORE, int TB, class Fn>
__device__ __forceinline__ void for_pixels(const unsigned char *src, unsigned char *dst, long npix, Fn fn) {
  const long first = blockIdx.x * (long)TB + threadIdx.x, step = (long)gridDim.x * TB;
  if ((reinterpret_cast<uintptr_t>(src) & 3u) == 0 && (!STORE || (reinterpret_cast<uintptr_t>(dst) & 3u) == 0)) {
    const long nq = npix / 4;
    const unsigned *s4 = reinterpret_cast<const unsigned *>(src);
    unsigned *d4 = reinterpret_cast<unsigned *>(dst);
    for (long q = first; q < nq; q += step) {
      const unsigned w0 = s4[3 * q], w1 = s4[3 * q + 1], w2 = s4[3 * q + 2];
      const Px a = fn(Px{w0 & 0xffu, (w0 >> 8) & 0xffu, (w0 >> 16) & 0xffu});
      const Px b = fn(Px{w0 >> 24, w1 & 0xffu, (w1 >> 8) & 0xffu});
      const Px c = fn(Px{(w1 >> 16) & 0xffu, w1 >> 24, w2 & 0xffu});
      const Px d = fn(Px{(w2 >> 8) & 0xffu, (w2 >> 16) & 0xffu, w2 >> 24});
      if (STORE) {
        d4[3 * q] = a.r | (a.g << 8) | (a.b << 16) | (b.r << 24);
        d4[3 * q + 1] = b.g | (b.b << 8) | (c.r << 16) | (c.g << 24);
        d4[3 * q + 2] = c.b | (d.r << 8) | (d.g << 16) | (d.b << 24);
      }
    }
    if (blockIdx.x == 0) {
      const long p = 4 * nq + threadIdx.x;
      if (p < npix) {
        const Px o = fn(Px{src[3 * p], src[3 * p + 1], src[3 * p + 2]});
        if (STORE) { dst[3 * p] = (unsigned char)o.r; dst[3 * p + 1] = (unsigned char)o.g; dst[3 * p + 2] = (unsigned char)o.b; }
      }
    }
  } else {
    for (long p = first; p < npix; p += step) {
      const Px o = fn(Px{src[3 * p], src[3 * p + 1], src[3 * p + 2]});
      if (STORE) { dst[3 * p] = (unsigned char)o.r; dst[3 * p + 1] = (unsigned char)o.g; dst[3 * p + 2] = (unsigned char)o.b; }
    }
  }
}

// Pass 1, grid (x, F): sums[f] += the L of every pixel of frame f after the operations ordered before contrast.  Frames without contrast
// leave at once.  npix <= 2^24, so the sum fits 32 bits.
__global__ __launch_bounds__(MB) void jitter_mean_kernel(const unsigned char *__restrict__ src, const float *__restrict__ plans, long npix,
                                                         unsigned *__restrict__ sums) {
  __shared__ unsigned s_wave[MB / 64];
  const int f = blockIdx.y;
  const JitterPlan pl = load_plan(plans + 8 * f);
  const int stop = contrast_slot(pl);
  if (stop < 0) return;                  // the whole workgroup
  unsigned acc = 0;
  for_pixels<false, MB>(src + (size_t)f * npix * 3, nullptr, npix, [&](Px p) {
    acc += luma(apply_ops(p, pl, stop, 0.f));
    return p;
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned tot = 0;
#pragma unroll
    for (int w = 0; w < MB / 64; ++w) tot += s_wave[w];
    atomicAdd(&sums[f], tot);
  }
}

// Pass 2, grid (x, F): all four operations, stored.  dst may be src: a thread reads its pixels before it writes them.
__global__ __launch_bounds__(JB) void jitter_apply_kernel(const unsigned char *src, const float *__restrict__ plans, long npix,
                                                          const unsigned *__restrict__ sums, unsigned char *dst) {
  const int f = blockIdx.y;
  const JitterPlan pl = load_plan(plans + 8 * f);
  float mean = 0.f;
  if (contrast_slot(pl) >= 0) mean = (float)(unsigned)((2ull * sums[f] + (unsigned long long)npix) / (2ull * (unsigned long long)npix));
  for_pixels<true, JB>(src + (size_t)f * npix * 3, dst + (size_t)f * npix * 3, npix, [&](Px p) { return apply_ops(p, pl, 4, mean); });
}

// YCB composition in u8 arithmetic (datasets/ycb/dataset.py host_item): rgb = back * mask_back + rgb (wraps), then
// rgb = rgb * mask_front + front * !mask_front.  Masks are 0 / non-zero u8 planes; either layer may be absent (null).
__device__ __forceinline__ Px compose_px(Px p, const unsigned char *back, const unsigned char *mask_back, const unsigned char *front,
                                         const unsigned char *mask_front, long i) {
  if (back && mask_back[i]) p = Px{(p.r + back[3 * i]) & 0xffu, (p.g + back[3 * i + 1]) & 0xffu, (p.b + back[3 * i + 2]) & 0xffu};
  if (front && !mask_front[i]) p = Px{front[3 * i], front[3 * i + 1], front[3 * i + 2]};
  return p;
}

__device__ __forceinline__ unsigned sel_bytes(unsigned m) { return ((m & 0xffu) ? 0xffu : 0u) | ((m & 0xff00u) ? 0xff00u : 0u) |
                                                                   ((m & 0xff0000u) ? 0xff0000u : 0u) | ((m & 0xff000000u) ? 0xff000000u : 0u); }
// byte-wise a + b (mod 256) of two dwords
__device__ __forceinline__ unsigned add_bytes(unsigned a, unsigned b) { return ((a & 0x7f7f7f7fu) + (b & 0x7f7f7f7fu)) ^ ((a ^ b) & 0x80808080u); }
// the mask bytes m0..m3 of four pixels spread over the pixels' three dwords (R G B R | G B R G | B R G B)
__device__ __forceinline__ void spread_mask(unsigned m, unsigned &k0, unsigned &k1, unsigned &k2) {
  const unsigned s = sel_bytes(m), b0 = s & 0xffu, b1 = (s >> 8) & 0xffu, b2 = (s >> 16) & 0xffu, b3 = s >> 24;
  k0 = b0 | (b0 << 8) | (b0 << 16) | (b1 << 24);
  k1 = b1 | (b1 << 8) | (b2 << 16) | (b2 << 24);
  k2 = b2 | (b3 << 8) | (b3 << 16) | (b3 << 24);
}

__global__ __launch_bounds__(JB) void compose_kernel(unsigned char *rgb, const unsigned char *__restrict__ back,
                                                     const unsigned char *__restrict__ mask_back, const unsigned char *__restrict__ front,
                                                     const unsigned char *__restrict__ mask_front, long npix, int dwords) {
  const long first = blockIdx.x * (long)JB + threadIdx.x, step = (long)gridDim.x * JB;
  long done = 0;
  if (dwords) {                                   // every pointer on a dword boundary
    const long nq = npix / 4;
    unsigned *d4 = reinterpret_cast<unsigned *>(rgb);
    const unsigned *b4 = reinterpret_cast<const unsigned *>(back), *f4 = reinterpret_cast<const unsigned *>(front);
    const unsigned *mb4 = reinterpret_cast<const unsigned *>(mask_back), *mf4 = reinterpret_cast<const unsigned *>(mask_front);
    for (long q = first; q < nq; q += step) {
      unsigned w[3] = {d4[3 * q], d4[3 * q + 1], d4[3 * q + 2]}, k[3];
      if (back) {
        spread_mask(mb4[q], k[0], k[1], k[2]);
#pragma unroll
        for (int j = 0; j < 3; ++j) w[j] = add_bytes(w[j], b4[3 * q + j] & k[j]);
      }
      if (front) {
        spread_mask(mf4[q], k[0], k[1], k[2]);
#pragma unroll
        for (int j = 0; j < 3; ++j) w[j] = (w[j] & k[j]) | (f4[3 * q + j] & ~k[j]);
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) d4[3 * q + j] = w[j];
    }
    done = 4 * nq;
  }
  for (long i = done + first; i < npix; i += step) {
    const Px o = compose_px(Px{rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]}, back, mask_back, front, mask_front, i);
    rgb[3 * i] = (unsigned char)o.r; rgb[3 * i + 1] = (unsigned char)o.g; rgb[3 * i + 2] = (unsigned char)o.b;
  }
}

inline int blocks_for(long npix, int threads) {
  const long b = cdiv(npix / 4 > 0 ? npix / 4 : 1, threads);
  return (int)(b < JIT_MAX_BLOCKS_X ? b : JIT_MAX_BLOCKS_X);
}

}  // namespace
}  // namespace df

using namespace df;

extern "C" int df_color_jitter(const unsigned char *src, const float *plan, int F, int H, int W, unsigned *scratch, unsigned char *dst,
                               df_stream_t stream) {
  if (!src || !plan || !scratch || !dst) return set_error(DF_ERR_ARG, "color_jitter: null pointer");
  if (F <= 0 || F > 65535 || H <= 0 || W <= 0 || (long)H * W > (1L << 24)) return set_error(DF_ERR_ARG, "color_jitter: bad sizes");
  const long npix = (long)H * W;
  const size_t bytes = (size_t)F * npix * 3;
  if (dst != src && dst < src + bytes && src < dst + bytes) return set_error(DF_ERR_ARG, "color_jitter: dst overlaps src without being src");
  hipStream_t st = to_stream(stream);
  if (hipMemsetAsync(scratch, 0, sizeof(unsigned) * F, st) != hipSuccess) return check_launch("color_jitter (sums)");
  // grids sized for the dword walk (four pixels per thread and step); the byte-wise walk of an unaligned frame takes four times the steps
  hipLaunchKernelGGL(jitter_mean_kernel, dim3(blocks_for(npix, MB), F), dim3(MB), 0, st, src, plan, npix, scratch);
  hipLaunchKernelGGL(jitter_apply_kernel, dim3(blocks_for(npix, JB), F), dim3(JB), 0, st, src, plan, npix, (const unsigned *)scratch, dst);
  return check_launch("color_jitter");
}

extern "C" int df_compose_frame(unsigned char *rgb, const unsigned char *back, const unsigned char *mask_back, const unsigned char *front,
                                const unsigned char *mask_front, int H, int W, df_stream_t stream) {
  if (!rgb) return set_error(DF_ERR_ARG, "compose_frame: null pointer");
  if ((back != nullptr) != (mask_back != nullptr) || (front != nullptr) != (mask_front != nullptr))
    return set_error(DF_ERR_ARG, "compose_frame: a layer and its mask come together");
  if (H <= 0 || W <= 0) return set_error(DF_ERR_ARG, "compose_frame: bad sizes");
  if (!back && !front) return DF_OK;
  const long npix = (long)H * W;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(back) | reinterpret_cast<uintptr_t>(mask_back) |
                         reinterpret_cast<uintptr_t>(front) | reinterpret_cast<uintptr_t>(mask_front);
  hipLaunchKernelGGL(compose_kernel, dim3(blocks_for(npix, JB)), dim3(JB), 0, to_stream(stream), rgb, back, mask_back, front, mask_front, npix,
                     (bits & 3u) == 0 ? 1 : 0);
  return check_launch("compose_frame");
}
