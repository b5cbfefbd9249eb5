// Steps 1-2 of the per-object input preparation, shared by preprocess.hip (pinhole datasets) and cad.hip (customCAD): the ordered
// compaction of a crop's mask pixels and the `choose` row drawn from them.  The callers differ in the mask predicate only.
//
// RNG contract (the reference uses np.random.shuffle, whose stream cannot be shared with a GPU): every mask
// pixel gets the key mix32(seed, flat crop index); the num_points pixels with the smallest keys (ties: lower
// index) are kept, in increasing index order.  Same distribution (a uniformly random subset, order preserved),
// reproducible from `seed`; the CPU checker of the test suite implements the same contract.
#pragma once
#include "common.h"

namespace df {
namespace prep {

constexpr int PB = 1024;

__device__ __host__ inline unsigned mix32(unsigned seed, unsigned i) {
  unsigned x = seed ^ (i * 0x9E3779B9u);
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

__device__ inline int block_excl_scan(int v, int *s_buf, int &total) {
  const int tid = threadIdx.x;
  s_buf[tid] = v;
  __syncthreads();
  for (int d = 1; d < PB; d <<= 1) {
    const int t = tid >= d ? s_buf[tid - d] : 0;
    __syncthreads();
    s_buf[tid] += t;
    __syncthreads();
  }
  total = s_buf[PB - 1];
  const int r = s_buf[tid] - v;
  __syncthreads();
  return r;
}

struct ObjDesc {   // one object: frame index and bounding box (host side: get_bbox, eval_ycb.py:54-90; the mask's own box for customCAD)
  int frame, itemid, rmin, rmax, cmin, cmax;
  unsigned seed;
  int given;         // != 0: this object's row of `choose` was filled in by the caller (chosen indices as an INPUT): step 2 is skipped
};

struct ChooseShared {
  int scan[PB];
  unsigned hist[256];
  unsigned prefix, remaining;
};

// One block of PB threads per object.  in_mask(i): is flat crop index i (0 <= i < HW) a mask pixel.  nz: HW ints of scratch, ch: the
// object's N-entry row of `choose`, count_slot: where the number of mask pixels goes.  Ends with a block barrier: `ch` is complete.
template <class Pred>
__device__ inline void choose_pixels(Pred in_mask, unsigned seed, int given, int HW, int N, int *nz, int64_t *ch, int *count_slot,
                                     ChooseShared &s) {
  const int tid = threadIdx.x;
  const int chunk = (HW + PB - 1) / PB;
  const int i0 = tid * chunk, i1 = min(HW, i0 + chunk);
  // 1. ordered compaction of the mask pixels (flat crop indices)
  int cnt = 0;
  for (int i = i0; i < i1; ++i) cnt += in_mask(i);
  int total;
  int off = block_excl_scan(cnt, s.scan, total);
  for (int i = i0; i < i1; ++i)
    if (in_mask(i)) nz[off++] = i;
  if (tid == 0) *count_slot = total;
  __syncthreads();
  // 2. choose
  if (given) {
    // the caller's indices (e.g. the subset the reference's np.random.shuffle drew): clamped into the crop, otherwise taken as they are
    for (int j = tid; j < N; j += PB) { const int64_t v = ch[j]; ch[j] = v < 0 ? 0 : (v >= HW ? HW - 1 : v); }
  } else if (total == 0) {
    for (int j = tid; j < N; j += PB) ch[j] = 0;     // detector lost the object; the caller checks count
  } else if (total <= N) {
    for (int j = tid; j < N; j += PB) ch[j] = nz[j % total];        // np.pad(..., 'wrap')
  } else {
    // radix select of the N-th smallest key (4 rounds of 8 bits)
    if (tid == 0) { s.prefix = 0; s.remaining = (unsigned)N; }
    __syncthreads();
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) s.hist[tid] = 0;
      __syncthreads();
      const unsigned prefix = s.prefix, hmask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
      for (int j = tid; j < total; j += PB) {
        const unsigned k = mix32(seed, (unsigned)nz[j]);
        if ((k & hmask) == prefix) atomicAdd(&s.hist[(k >> shift) & 255], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        unsigned rem = s.remaining, bin = 0;
        while (s.hist[bin] < rem) { rem -= s.hist[bin]; ++bin; }
        s.prefix = prefix | (bin << shift);
        s.remaining = rem;          // how many keys equal to the final threshold are still to be taken
      }
      __syncthreads();
    }
    const unsigned T = s.prefix, ties = s.remaining;
    // keep keys < T, plus the `ties` lowest-index entries with key == T; ordered compaction into choose
    const int c2 = (total + PB - 1) / PB;
    const int j0 = tid * c2, j1 = min(total, j0 + c2);
    int less = 0, eq = 0;
    for (int j = j0; j < j1; ++j) {
      const unsigned k = mix32(seed, (unsigned)nz[j]);
      less += k < T; eq += k == T;
    }
    int tot_eq, tot_less;
    int eq_off = block_excl_scan(eq, s.scan, tot_eq);
    // number of selected entries before this thread's chunk = less-before + min(eq-before, ties)
    int less_off = block_excl_scan(less, s.scan, tot_less);
    int out = less_off + min(eq_off, (int)ties);
    for (int j = j0; j < j1; ++j) {
      const unsigned k = mix32(seed, (unsigned)nz[j]);
      bool take = k < T;
      if (k == T) { take = eq_off < (int)ties; ++eq_off; }
      if (take) ch[out++] = nz[j];
    }
  }
  __syncthreads();
}

}  // namespace prep
}  // namespace df
