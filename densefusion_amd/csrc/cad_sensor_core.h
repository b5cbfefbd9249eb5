// The per-pixel rule of df_cad_depth_sensor (steps D0..D6 of its comment in include/dfusion.h), as a __host__ __device__ function: the
// kernel of cad_sensor.hip calls it per lane, a CPU program can call it per pixel.  Integer arithmetic only: the Unity code is affine in
// 1 / z, a disparity, so a sensor whose noise is constant in disparity has constant-sigma noise in code units.
#pragma once
#include "choose_core.h"

namespace df {
namespace sensor {

constexpr unsigned C0 = 0x243F6A88u, C1 = 0x85A308D3u, C2 = 0x13198A2Eu, C3 = 0x03707344u;
constexpr int HORIZON = 65535, MAX_CODE = 65534;
constexpr int MAX_RADIUS = 4, MAX_QUANT = 4096, ONE24 = 1 << 24;

// the six integers of a sensor record; they travel as launch arguments
struct Record {
  int noise_mul, edge_radius, edge_step, edge_drop24, drop24, quant;
};

// what a pixel adds to stats[f] = {edge pixels, dropped at random, dropped at an edge, kept with another code}
struct Counts {
  int edge, drop, edge_drop, changed;
};

// D0
__host__ __device__ inline unsigned frame_seed(unsigned seed, unsigned first_frame, int f) {
  return prep::mix32(seed, first_frame + (unsigned)f);
}

// D2 on the clean frame: a horizon pixel, or a code further than edge_step from c, within the (2R+1)^2 window clamped to the frame.
// The walk stops at the first hit (the result is an OR, so the order does not matter).
__host__ __device__ inline bool is_edge(const unsigned short *__restrict__ frame, int IH, int IW, int r, int q, int c, int R, int edge_step) {
  const int r0 = r - R < 0 ? 0 : r - R, r1 = r + R > IH - 1 ? IH - 1 : r + R;
  const int q0 = q - R < 0 ? 0 : q - R, q1 = q + R > IW - 1 ? IW - 1 : q + R;
  for (int rr = r0; rr <= r1; ++rr) {
    const unsigned short *row = frame + (size_t)rr * IW;
    for (int qq = q0; qq <= q1; ++qq) {
      const int cn = row[qq];
      const int d = cn > c ? cn - c : c - cn;
      if (cn == HORIZON || d > edge_step) return true;
    }
  }
  return false;
}

// The noise term of D5 for index p under seed s: floor((noise_mul * S + 2^31) / 2^32), S the centred sum of four 16-bit uniforms.
// df_seg_batch's step G4 draws its pixel noise from the same function.
__host__ __device__ inline int noise_term(unsigned s, unsigned p, int noise_mul) {
  const unsigned h0 = prep::mix32(s ^ C0, p), h1 = prep::mix32(s ^ C1, p);
  const int S = (int)((h0 & 0xFFFFu) + (h0 >> 16) + (h1 & 0xFFFFu) + (h1 >> 16)) - 131070;
  const long long prod = (long long)noise_mul * S + (1LL << 31);                                 // |.| < 2^49
  const long long fl = prod >= 0 ? prod >> 32 : -((-prod + ((1LL << 32) - 1)) >> 32);            // floor(prod / 2^32)
  return (int)fl;
}

// D1..D6 for pixel p = r * IW + q, whose clean code is c = frame[p], of a frame whose seed is s (D0); `frame` is the CLEAN frame, of
// which only pixels inside the frame are read.  Returns the sensor's code and adds the pixel's share to `n`.
__host__ __device__ inline unsigned short sense_pixel(const unsigned short *__restrict__ frame, int IH, int IW, int r, int q, int c, unsigned s,
                                                      const Record &rec, Counts &n) {
  const unsigned p = (unsigned)(r * IW + q);
  if (c == HORIZON) return HORIZON;                                                              // D1
  const bool edge = rec.edge_radius > 0 && is_edge(frame, IH, IW, r, q, c, rec.edge_radius, rec.edge_step);   // D2
  n.edge += edge;
  if ((prep::mix32(s ^ C3, p) >> 8) < (unsigned)rec.drop24) { n.drop += 1; return HORIZON; }     // D3
  if (edge && (prep::mix32(s ^ C2, p) >> 8) < (unsigned)rec.edge_drop24) { n.edge_drop += 1; return HORIZON; }   // D4
  int c1 = c + noise_term(s, p, rec.noise_mul);                                                  // D5
  c1 = c1 < 0 ? 0 : (c1 > MAX_CODE ? MAX_CODE : c1);
  int c2 = (c1 + rec.quant / 2) / rec.quant * rec.quant;                                         // D6
  c2 = c2 > MAX_CODE ? MAX_CODE : c2;
  n.changed += c2 != c;
  return (unsigned short)c2;
}

}  // namespace sensor
}  // namespace df
