// Test-only: the host-side rules of sca_restart_scenes (sca_amd/csrc/sca_scenes.h: scene_restart_check, scene_restart_layout) behind a C
// interface for tests/test_scene_restart_cpu.py.  Plain C++, no HIP.  Not part of the product (sca_amd never loads it).
#include "sca_scenes.h"

using namespace sca;

extern "C" {

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
