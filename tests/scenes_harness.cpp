// Test-only: the host-side rules of scene batches (sca_amd/csrc/sca_scenes.h, plan_kd_forest of sca_forms.h) behind a C interface for
// tests/test_scenes_cpu.py.  Plain C++, no HIP.  Not part of the product (sca_amd never loads it).
#include "sca_forms.h"
#include "sca_scenes.h"

using namespace sca;

extern "C" {

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

}  // extern "C"
