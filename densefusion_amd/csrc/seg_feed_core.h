// The per-pixel rule of df_seg_batch (steps G1..G5 of its comment in include/dfusion.h), as __host__ __device__ functions: the kernel
// of seg_feed.hip calls them per lane with its LDS tile behind `at`, a CPU program can call seg_pixel per pixel with the frames behind
// it.  Integer arithmetic up to the normalisation, which is seg_norm (seg_norm.h): one subtraction and one division per channel.
#pragma once
#include "cad_sensor_core.h"
#include "seg_norm.h"

namespace df {
namespace segfeed {

constexpr int MAX_OBJECTS = 64, MAX_CLASSES = 64;

// class_map [O+1], checked on the host; it travels as a launch argument
struct ClassMap {
  unsigned char cls[MAX_OBJECTS + 1];
};

// one row of desc
struct Item {
  int f, y0, x0, flip, b, by0, bx0;
  unsigned seed;
};

__host__ __device__ inline Item load_item(const int *__restrict__ d) {
  return Item{d[0], d[1], d[2], d[3], d[4], d[5], d[6], (unsigned)d[7]};
}

// the descriptor rule: frame, window inside the frame, flip, background index, background window inside the pool
__host__ __device__ inline bool item_ok(const Item &it, int F, int IH, int IW, int H, int W, int NB, int BH, int BW) {
  if (it.f < 0 || it.f >= F || it.y0 < 0 || it.y0 > IH - H || it.x0 < 0 || it.x0 > IW - W) return false;
  if (it.flip < 0 || it.flip > 3 || it.b < -1 || it.b >= NB) return false;
  return it.b < 0 || (it.by0 >= 0 && it.by0 <= BH - H && it.bx0 >= 0 && it.bx0 <= BW - W);
}

// the frames of a call, as the pixel rule reads them
struct Source {
  const unsigned char *rgb;
  const unsigned short *label;
  const unsigned char *back;
  int IH, IW, BH, BW, O;
};

// G1 + G2 for window pixel (i, j), 0 <= i < H, 0 <= j < W: the composited colour in bytes 0..2, the class in byte 3
__host__ __device__ inline unsigned composite_pixel(const Source &s, const ClassMap &cm, const Item &it, int i, int j) {
  const size_t q = ((size_t)it.f * s.IH + (it.y0 + i)) * s.IW + (it.x0 + j);
  const int l = s.label[q];
  const unsigned cls = l <= s.O ? cm.cls[l] : 0u;
  const unsigned char *c = l == 0 && it.b >= 0 ? s.back + (((size_t)it.b * s.BH + (it.by0 + i)) * s.BW + (it.bx0 + j)) * 3 : s.rgb + q * 3;
  return (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16 | cls << 24;
}

// G3 + G4 for window pixel p = i * W + j: at(di, dj), di and dj in -1..1, is composite_pixel of the neighbour with its indices clamped
// to the window.  The 1-2-1 sums run on two 16-bit fields of a word at once (red and blue; green alone): 16 * 255 < 2^16.  Returns
// v_0 | v_1 << 8 | v_2 << 16 | class << 24.
template <class At>
__host__ __device__ inline unsigned finish_pixel(At at, unsigned p, int blur, unsigned seed, int noise_mul) {
  const unsigned own = at(0, 0);
  unsigned v[3] = {own & 0xffu, (own >> 8) & 0xffu, (own >> 16) & 0xffu};
  if (blur) {
    unsigned rb = 0, g = 0;
#pragma unroll
    for (int di = -1; di <= 1; ++di) {
#pragma unroll
      for (int dj = -1; dj <= 1; ++dj) {
        const unsigned w = (di == 0 ? 2u : 1u) * (dj == 0 ? 2u : 1u), c = at(di, dj);
        rb += w * (c & 0x00ff00ffu);
        g += w * ((c >> 8) & 0xffu);
      }
    }
    rb = ((rb + 0x00080008u) >> 4) & 0x00ff00ffu;
    v[0] = rb & 0xffu; v[1] = (g + 8u) >> 4; v[2] = rb >> 16;
  }
  if (noise_mul > 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int n = (int)v[k] + sensor::noise_term(seed, 3u * p + (unsigned)k, noise_mul);
      v[k] = (unsigned)(n < 0 ? 0 : (n > 255 ? 255 : n));
    }
  }
  return v[0] | v[1] << 8 | v[2] << 16 | (own & 0xff000000u);
}

// where G5 writes window pixel (i, j)
__host__ __device__ inline int flipped(int i, int n, int bit) { return bit ? n - 1 - i : i; }

// G1..G4 of one pixel straight from the frames (the kernel goes through its tile instead)
__host__ __device__ inline unsigned seg_pixel(const Source &s, const ClassMap &cm, const Item &it, int H, int W, int i, int j, int blur,
                                              int noise_mul) {
  auto at = [&](int di, int dj) {
    const int ii = i + di < 0 ? 0 : (i + di > H - 1 ? H - 1 : i + di), jj = j + dj < 0 ? 0 : (j + dj > W - 1 ? W - 1 : j + dj);
    return composite_pixel(s, cm, it, ii, jj);
  };
  return finish_pixel(at, (unsigned)(i * W + j), blur, it.seed, noise_mul);
}

}  // namespace segfeed
}  // namespace df
