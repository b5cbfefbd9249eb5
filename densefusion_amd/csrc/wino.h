// Winograd F(2x2, 3x3) / F(4x4, 3x3) companion kernels of the batched GEMM (wino.hip).
#pragma once
#include <vector>

#include "igemm.h"

namespace df {

constexpr int WINO_MAXB = 16;
// One axis (rows or columns) of a map under dilation d, cut into strips of TT tiles.  The d residue classes of the axis (positions
// r, r + d, ...: n = ceil(L/d) points for r < R = L - d (n - 1), n - 1 for the others) are convolved independently of each other.
//   padded: S = d strips, strip r = residue r alone, TT = ceil(n / m): every residue pays its own round-up to whole tiles
//   packed: S = 1 strip of V = L + k - 1 virtual positions: the k non-empty residues in order, ONE zero position (separator)
//           between neighbours, which is the convolution's zero padding of both; TT = ceil(V / m).  Virtual position v: R slots of
//           width n + 1, then slots of width n; a slot's last position is its separator (the last slot has none: it ends at V).
// Packed is taken for m = 4 and d > 1 only, and only where it has strictly fewer tiles; a function of (L, d, m), never the batch.
struct WinoAxis { int L, n, S, TT, packed; };
WinoAxis wino_axis(int L, int d, int m);
// the point of the axis at virtual position v of a strip (padded: its v-th point), or -1: separator / outside.  Closed form.
int wino_axis_coord(const WinoAxis &a, int d, int strip, int v);
// per-bucket table of a multi-bucket transform launch (kernel argument, by value)
struct WinoTab { int n; WinoAxis ay[WINO_MAXB], ax[WINO_MAXB]; int blocks[WINO_MAXB + 1]; long T[WINO_MAXB], row0[WINO_MAXB], t0[WINO_MAXB]; };
// the two axes (strips, tiles per strip = TH / TW, layout) and the tiles in total, T = B * ay.S * ax.S * TH * TW
struct WinoGeom { int TH, TW; long T; WinoAxis ay, ax; };
// m = 2: F(2x2,3x3) (16 planes), m = 4: F(4x4,3x3) (36 planes).  packed = false keeps every axis padded: the native trainer's choice
// (its gradients are held to the direct-convolution tape within a bound that the padded tiles' rounding meets)
WinoGeom wino_geom(int B, int H, int W, int dil, int m = 2, bool packed = true);
// layer-geometry-only decision (never batch dependent): 0 = direct implicit GEMM, 2 / 4 = the transform-domain product with that tile
int wino_route(int H, int W, int dil, int Cin, int Cout);
void launch_wino_weight(const float *w_packed /*[O][3][3][C]*/, float *U /*[(m+2)^2][O][C]*/, int O, int C, hipStream_t st, int m = 2);
// F(4x4,3x3) weight transforms of up to WINO_WMAX tensors in one launch: segment g = O[g] x C[g] packed 3x3 kernels at
// (from_b[g] ? src_b : src_a) + src_off[g] -> dst + dst_off[g]; e0 = prefix of O * C
constexpr int WINO_WMAX = 32;
struct WinoWTab { int n; int O[WINO_WMAX], C[WINO_WMAX], from_b[WINO_WMAX]; long src_off[WINO_WMAX], dst_off[WINO_WMAX], e0[WINO_WMAX + 1]; };
void launch_wino4_weight_multi(const float *src_a, const float *src_b, float *dst, const WinoWTab &tab, hipStream_t st);
// one bucket that owns its planes, with a bias and channel offsets (the stand-alone C API)
void launch_wino_input(const float *x, int in_ld, int in_coff, float *V /*[(m+2)^2][T][C]*/, int B, int H, int W, int C, int dil, hipStream_t st,
                       int m = 2);
void launch_wino_output(const float *M /*[(m+2)^2][T][C]*/, float *out, int out_ld, int out_coff, const float *bias, const float *res, int res_ld,
                        int res_coff, int act, int B, int H, int W, int C, int dil, hipStream_t st, int m = 2);

// The Winograd-domain pass of a list of crop-size buckets, planned once: tile m, dilation and layout are fixed when the plan is made, and the
// sizes of V / M and the transforms on both sides of the GEMM all read the same geometry from it.  Bucket k = B maps of H x W whose pixel
// rows start at row0 of the row-concatenated x / out / res and whose tiles are rows [t0, t0 + g.T) of the T-row planes.
struct WinoBucket { WinoGeom g; long row0, t0; };
struct WinoPlan {
  int dil, m;
  bool packed;
  long T = 0;          // tiles of all buckets
  double px = 0;       // output pixels the tiles are for
  std::vector<WinoBucket> b;
  void add(int B, int H, int W, long row0) {
    b.push_back(WinoBucket{wino_geom(B, H, W, dil, m, packed), row0, T});
    T += b.back().g.T;
    px += (double)B * H * W;
  }
  int nz() const { return (m + 2) * (m + 2); }                     // planes of V / M
  double useful() const { return px / ((double)(m * m) * (double)T); }     // a tile yields m x m pixels
};
// the transforms of every bucket of the plan: m = 4 one launch per WINO_MAXB buckets, m = 2 one launch per bucket
void launch_wino_input(const WinoPlan &pl, const float *x, int in_ld, float *V /*[nz][T][C]*/, int C, hipStream_t st);
void launch_wino_output(const WinoPlan &pl, const float *M /*[nz][T][C]*/, float *out, int out_ld, const float *res, int res_ld, int act, int C,
                        hipStream_t st);

}  // namespace df
