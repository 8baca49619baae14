// Test-only: the host-side rules of scene batches (sca_amd/csrc/sca_scenes.h, plan_kd_forest of sca_forms.h) behind a C interface for
// tests/test_scenes_cpu.py, tests/test_scene_obstacles_cpu.py and tests/test_scene_restart_cpu.py.  Plain C++, no HIP.  Not part of the
// product (sca_amd never loads it).
#include "sca_forms.h"
#include "sca_scenes.h"

using namespace sca;

extern "C" {

// ---- sca_set_scenes -----------------------------------------------------------------------------------------------------------------------
void scenes_constants(int *out3) { out3[0] = KD_WAVE_CAP; out3[1] = KD_FOREST_GRID_MAX; out3[2] = SCA_FORM_SCENES; }
void scenes_plan_kd_forest(int largest_scene, int nscenes, int *out2) {
    const KdForestPlan p = plan_kd_forest(largest_scene, nscenes);
    out2[0] = p.block; out2[1] = p.grid;
}
// out4: fault, scene, largest, the error code sca_set_scenes returns for it
void scenes_check_offsets(int n, int nscenes, const int32_t *offsets, int *out4) {
    const SceneCheck k = scenes_check(n, nscenes, offsets);
    out4[0] = k.fault; out4[1] = k.scene; out4[2] = k.largest; out4[3] = scenes_error_code(k.fault);
}
int scenes_perm_check(int nscenes, const int32_t *offsets, const int32_t *perm) { return scenes_perm_fault(nscenes, offsets, perm); }
int scenes_mode(int requested) { return scenes_neighbor_mode(requested); }

// ---- sca_set_scene_obstacles ----------------------------------------------------------------------------------------------------------------
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

// ---- sca_restart_scenes: scene_restart_check, scene_restart_layout --------------------------------------------------------------------------
// ctx_bits: 1 state_set, 2 scene_begun, 4 tracker_on, 8 paths_on, 16 tracker_per_agent.  out3: fault, entry, T.  Returns the error code
// sca_restart_scenes gives for the fault.
int restart_check(int nscenes, const int32_t *offsets, int ctx_bits, const uint8_t *policy_now, int count, const int32_t *scene_ids,
                  const double *pos, const float *vel, const double *heading, const double *radius, const double *pref_speed, const double *goal,
                  const uint8_t *policy, const uint8_t *zaxis, const double *max_run_dist, const double *goal_heading, int *out3) {
    const RestartCtx X{nscenes, offsets, (ctx_bits & 1) != 0, (ctx_bits & 2) != 0, (ctx_bits & 4) != 0, (ctx_bits & 8) != 0, (ctx_bits & 16) != 0, policy_now};
    const RestartArgs A{count, scene_ids, pos, vel, heading, radius, pref_speed, goal, policy, zaxis, max_run_dist, goal_heading};
    const RestartCheck k = scene_restart_check(X, A);
    out3[0] = k.fault; out3[1] = k.entry; out3[2] = k.total;
    return scene_restart_error_code(k.fault);
}
int restart_sections(void) { return RS_SECTIONS; }
void restart_layout(int cap, int64_t *off, int64_t *total) {
    const RestartLayout L = scene_restart_layout(cap);
    for (int s = 0; s < RS_SECTIONS; s++) off[s] = L.off[s];
    *total = L.total;
}

}  // extern "C"
