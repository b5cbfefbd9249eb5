// M1, M2 of df_ppf_model_build (include/dfusion.h): the pair table of the sampled models, built on the host through the very functions of
// pose_ppf_core.h that the vote kernel calls.  Plain C++: no HIP, so a CPU program can run it as it stands.  The arguments are checked by
// the caller (pose_ppf.hip).
#pragma once
#include <algorithm>
#include <vector>

#include "pose_ppf_core.h"

namespace df {
namespace poseppf {

inline size_t key_count(int ND, int NANG) { return (size_t)ND * NANG * NANG * NANG; }

// bucket_begin [O][NKEY+1], entry_point [E], entry_cs [E][2] with E >= the sum of NM_o (NM_o - 1); returns the entries written
inline size_t build_model(const double *points, const double *normals, const int *point_begin, const double *dist_step, int O,
                          const Tables &tb, int *bucket_begin, int *entry_point, float *entry_cs) {
  const size_t NKEY = key_count(tb.ND, tb.NANG);
  std::vector<int> keys, cursor(NKEY + 1);
  std::vector<float> angle;
  size_t base = 0;
  for (int o = 0; o < O; ++o) {
    const int m0 = point_begin[o], n = point_begin[o + 1] - m0;
    keys.assign((size_t)n * n, -1);
    angle.assign(2 * (size_t)n * n, 0.0f);
    std::fill(cursor.begin(), cursor.end(), 0);
    for (int i = 0; i < n; ++i) {                                            // M1: every ordered pair i != j that keeps a key and an angle
      const double *pi = points + 3 * (size_t)(m0 + i), *ni = normals + 3 * (size_t)(m0 + i);
      double R[9], cs[2];
      frame_rot(ni, R);
      for (int j = 0; j < n; ++j) {
        if (j == i) continue;
        const double *pj = points + 3 * (size_t)(m0 + j), *nj = normals + 3 * (size_t)(m0 + j);
        const int key = pair_key(pi, ni, pj, nj, dist_step[o], tb);
        if (key < 0 || !frame_angle(R, pi, pj, cs)) continue;
        const size_t at = (size_t)i * n + j;
        keys[at] = key;
        angle[2 * at] = (float)cs[0];
        angle[2 * at + 1] = (float)cs[1];
        cursor[(size_t)key + 1] += 1;
      }
    }
    int *bb = bucket_begin + (size_t)o * (NKEY + 1);
    size_t run = base;                                                       // M2: a counting sort by key, stable in (i, j)
    for (size_t k = 0; k <= NKEY; ++k) {
      run += (size_t)cursor[k];
      bb[k] = (int)run;
      cursor[k] = (int)run;
    }
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        const size_t at = (size_t)i * n + j;
        if (keys[at] < 0) continue;
        const size_t e = (size_t)cursor[keys[at]]++;
        entry_point[e] = i;
        entry_cs[2 * e] = angle[2 * at];
        entry_cs[2 * e + 1] = angle[2 * at + 1];
      }
    base = run;
  }
  return base;
}

}  // namespace poseppf
}  // namespace df
