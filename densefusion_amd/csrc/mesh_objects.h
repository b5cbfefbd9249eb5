// The object table of O meshes packed into one vertex and one triangle array, as df_cad_render_scene and df_pose_verify take it: the one
// host check of tri_begin and the launch argument made from it.
// df_mesh_icp is deliberately not a user: its tri_begin need neither start at 0 nor end at T, and its table carries max_dist^2, not scales.
#pragma once
#include "common.h"

namespace df {
namespace {

constexpr int MAX_OBJECTS = DF_CAD_SCENE_MAX_OBJECTS;
inline bool objects_ok(int O) { return O >= 1 && O <= MAX_OBJECTS; }
// begin[o] .. begin[o + 1] - 1 are the triangles of object o; entries past O hold T, so that a search over all 64 stays below O
struct ObjectTable {
  double scale[MAX_OBJECTS];
  int begin[MAX_OBJECTS + 1];
};

inline ObjectTable make_object_table(const int *tri_begin, const double *model_scale, int O, int T) {
  ObjectTable tab;
  for (int k = 0; k <= MAX_OBJECTS; ++k) tab.begin[k] = k <= O ? tri_begin[k] : T;
  for (int k = 0; k < MAX_OBJECTS; ++k) tab.scale[k] = k < O ? model_scale[k] : 0.0;
  return tab;
}

// the three refusals (1 <= O <= MAX_OBJECTS is the caller's check); *longest (may be null) takes the largest range
inline int check_tri_begin(const char *name, const int *tri_begin, int O, int T, int *longest) {
  if (tri_begin[0] != 0) return set_error(DF_ERR_ARG, "%s: tri_begin[0] = %d, not 0", name, tri_begin[0]);
  int most = 0;
  for (int o = 0; o < O; ++o) {
    if (tri_begin[o + 1] < tri_begin[o])
      return set_error(DF_ERR_ARG, "%s: tri_begin decreases from %d to %d at object %d", name, tri_begin[o], tri_begin[o + 1], o);
    most = tri_begin[o + 1] - tri_begin[o] > most ? tri_begin[o + 1] - tri_begin[o] : most;
  }
  if (tri_begin[O] != T) return set_error(DF_ERR_ARG, "%s: tri_begin[O] = %d, not T = %d", name, tri_begin[O], T);
  if (longest) *longest = most;
  return DF_OK;
}

}  // namespace
}  // namespace df
