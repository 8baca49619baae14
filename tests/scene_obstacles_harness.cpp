// Test-only: the host-side rules of per-scene obstacle sets (sca_set_scene_obstacles; sca_amd/csrc/sca_scenes.h) behind a C interface for
// tests/test_scene_obstacles_cpu.py.  Plain C++, no HIP.  Not part of the product (sca_amd never loads it).
#include "sca_scenes.h"

using namespace sca;

extern "C" {

void scene_obs_constants(int *out2) { out2[0] = SCA_FORM_SCENE_OBSTACLES; out2[1] = SCA_FORM_SCENES; }
// out4: fault, scene, total, the error code sca_set_scene_obstacles returns for it
void scene_obs_check(int ctx_nscenes, int max_obstacles, int nscenes, const int32_t *obs_offsets, int have_pos, int have_radius, int *out4) {
    const SceneObsCheck k = scene_obstacles_check(ctx_nscenes, max_obstacles, nscenes, obs_offsets, have_pos != 0, have_radius != 0);
    out4[0] = k.fault; out4[1] = k.scene; out4[2] = k.total; out4[3] = scene_obstacles_error_code(k.fault);
}
void scene_obs_roots(int nscenes, const int32_t *obs_offsets, int32_t *roots) {
    for (int s = 0; s < nscenes; s++) roots[s] = scene_obstacle_root(obs_offsets, s);
}
// nodes4: [nnodes][4] = begin, end, left, right of a tree built over one scene's obstacles alone (local ids, nodes numbered from 0)
struct Node4 { int32_t begin, end, left, right; };
void scene_obs_shift(int32_t *nodes4, int nnodes, int obs_begin) {
    scene_obstacle_shift(reinterpret_cast<Node4 *>(nodes4), nnodes, obs_begin, 10);     // MAX_LEAF, kdTree.py:53
}

}  // extern "C"
