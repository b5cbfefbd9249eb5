// A depth-sensor model over rendered customCAD depth frames: disparity noise, drop-out along depth discontinuities and at random, and
// quantisation, all in integer arithmetic on the 16-bit codes.  The contract is the comment of df_cad_depth_sensor in include/dfusion.h
// (steps D0..D6); the per-pixel rule is sense_pixel of cad_sensor_core.h; tests/cad_sensor_np.py restates it in numpy and the outputs
// are compared bit for bit.  No floating point anywhere.
//
// Steps on the caller's stream: the stats are set to zero; sensor_kernel (grid = pixel blocks x frames, a block's pixels in one frame as
// in mask_kernel) takes SENSOR_UNROLL runs of 256 consecutive pixels per sweep, consecutive lanes on consecutive pixels of a row: the
// clean codes of all runs are loaded first, so that a lane has that many reads in flight, and a horizon pixel -- most of a frame --
// costs its load and its store.  A live pixel walks the edge window of the clean frame through L1 / L2; the walk is clamped to the
// frame, so it never reads the next frame's rows.  The four counts are reduced across the wave, then one set of integer atomics per
// wave (the scheme of reduce_frame_stats).  SENSOR_MAX_BLOCKS and SENSOR_UNROLL are where the measured time of 32 full-size frames
// was lowest: with the pixels spread over more blocks per frame the call gets slower, not faster.
#include "cad_frame.h"
#include "cad_sensor_core.h"

namespace df {
namespace {

using sensor::Counts;
using sensor::Record;

constexpr int SENSOR_UNROLL = 4;        // runs of RB pixels a block takes per sweep
constexpr int SENSOR_MAX_BLOCKS = 32;   // pixel blocks per frame

__global__ __launch_bounds__(RB) void sensor_kernel(const unsigned short *__restrict__ depth_in, unsigned short *__restrict__ depth_out, int IH,
                                                    int IW, unsigned seed, unsigned first_frame, Record rec, int *__restrict__ stats) {
  const int f = blockIdx.y;
  const int npix = IH * IW;                                 // at most 2^30: base + u * RB stays below 2^31
  const unsigned s = sensor::frame_seed(seed, first_frame, f);
  const unsigned short *in = depth_in + (size_t)f * npix;
  unsigned short *out = depth_out + (size_t)f * npix;
  Counts n = {0, 0, 0, 0};
  for (int base = blockIdx.x * (RB * SENSOR_UNROLL) + threadIdx.x; base < npix; base += gridDim.x * (RB * SENSOR_UNROLL)) {
    int c[SENSOR_UNROLL];
#pragma unroll
    for (int u = 0; u < SENSOR_UNROLL; ++u) {
      const int p = base + u * RB;
      c[u] = p < npix ? in[p] : -1;
    }
#pragma unroll
    for (int u = 0; u < SENSOR_UNROLL; ++u) {
      const int p = base + u * RB;
      if (c[u] < 0) continue;                               // past the frame's end
      const int r = p / IW, q = p - r * IW;
      out[p] = sensor::sense_pixel(in, IH, IW, r, q, c[u], s, rec, n);
    }
  }
  // every lane of the block arrives here: the shuffles see the whole wave
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n.edge += __shfl_down(n.edge, off, 64); n.drop += __shfl_down(n.drop, off, 64);
    n.edge_drop += __shfl_down(n.edge_drop, off, 64); n.changed += __shfl_down(n.changed, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    int *st = stats + (size_t)f * 4;
    if (n.edge) atomicAdd(&st[0], n.edge);
    if (n.drop) atomicAdd(&st[1], n.drop);
    if (n.edge_drop) atomicAdd(&st[2], n.edge_drop);
    if (n.changed) atomicAdd(&st[3], n.changed);
  }
}

}  // namespace
}  // namespace df

using namespace df;

extern "C" int df_cad_depth_sensor(const unsigned short *depth_in, unsigned short *depth_out, int F, int IH, int IW, unsigned seed,
                                   unsigned first_frame, int noise_mul, int edge_radius, int edge_step, int edge_drop24, int drop24,
                                   int quant, int *stats, df_stream_t stream) {
  const char *name = "cad_depth_sensor";
  if (!depth_in || !depth_out || !stats) return set_error(DF_ERR_ARG, "%s: null pointer", name);
  if (!sizes_ok(F, IH, IW)) return set_error(DF_ERR_ARG, "%s: bad sizes", name);
  const long npix = (long)IH * IW;
  const uintptr_t a = reinterpret_cast<uintptr_t>(depth_in), b = reinterpret_cast<uintptr_t>(depth_out);
  const uintptr_t bytes = (uintptr_t)F * npix * sizeof(unsigned short);
  if (a < b + bytes && b < a + bytes)
    return set_error(DF_ERR_ARG, "%s: depth_in and depth_out overlap (the edge window reads the clean frame)", name);
  if (noise_mul < 0) return set_error(DF_ERR_ARG, "%s: noise_mul %d is negative", name, noise_mul);
  if (edge_radius < 0 || edge_radius > sensor::MAX_RADIUS)
    return set_error(DF_ERR_ARG, "%s: edge_radius %d outside 0..%d", name, edge_radius, sensor::MAX_RADIUS);
  if (edge_step < 0 || edge_step > 65535) return set_error(DF_ERR_ARG, "%s: edge_step %d outside 0..65535", name, edge_step);
  if (edge_drop24 < 0 || edge_drop24 > sensor::ONE24 || drop24 < 0 || drop24 > sensor::ONE24)
    return set_error(DF_ERR_ARG, "%s: edge_drop24 %d or drop24 %d outside 0..2^24", name, edge_drop24, drop24);
  if (quant < 1 || quant > sensor::MAX_QUANT) return set_error(DF_ERR_ARG, "%s: quant %d outside 1..%d", name, quant, sensor::MAX_QUANT);
  hipStream_t st = to_stream(stream);
  if (hipMemsetAsync(stats, 0, sizeof(int) * 4 * (size_t)F, st) != hipSuccess) return check_launch(name);
  const int blocks = cdiv(npix, RB * SENSOR_UNROLL) < SENSOR_MAX_BLOCKS ? cdiv(npix, RB * SENSOR_UNROLL) : SENSOR_MAX_BLOCKS;
  const Record rec = {noise_mul, edge_radius, edge_step, edge_drop24, drop24, quant};
  hipLaunchKernelGGL(sensor_kernel, dim3(blocks, F), dim3(RB), 0, st, depth_in, depth_out, IH, IW, seed, first_frame, rec, stats);
  return check_launch(name);
}
