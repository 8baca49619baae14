// Test-only: the closest-approach rule (sca_amd/csrc/sca_scenes.h: scene_clearance_step over clearance_pair, the function k_scene_clearance
// runs per pair, and scene_clearance_check) behind a C interface for tests/test_scene_clearance_cpu.py.  Plain C++, no HIP.  Not part of the
// product (sca_amd never loads it).  With -DSCENE_CLEARANCE_MAIN it is a program of its own that runs the rule on heap arrays of exactly
// the sizes the rule may read, for a build under -fsanitize=address,undefined.  The norm is sca_core.h's l3norm (L3Norm), as in the kernel:
// built with -ffp-contract=off like everything that includes that header.
#include "sca_core.h"
#include "sca_scenes.h"

using namespace sca;

extern "C" {

int sclr_struct_bytes() { return (int)sizeof(sca_scene_clearance); }
void sclr_empty(sca_scene_clearance *rec, int n) { for (int i = 0; i < n; i++) rec[i] = scene_clearance_empty(); }
void sclr_step(int size, const double *pos, const double *radius, const uint32_t *entry_flags, int nobs, const double *obs_pos, const double *obs_radius, int step,
               sca_scene_clearance *rec) {
    scene_clearance_step(size, pos, radius, entry_flags, nobs, obs_pos, obs_radius, step, rec, L3Norm{});
}
// out2: fault, the error code the two entry points give for it
void sclr_check(int get, int nscenes, int scene_begun, int enabled, int scene, int have_out, int struct_bytes, int *out2) {
    const ClearFault f = scene_clearance_check(get != 0, nscenes, scene_begun != 0, enabled != 0, scene, have_out != 0, struct_bytes);
    out2[0] = f; out2[1] = scene_clearance_error_code(f);
}

}  // extern "C"

#ifdef SCENE_CLEARANCE_MAIN
#include <cstdio>
#include <cstdlib>
#include <memory>
// A scene of `size` agents on a line one metre apart, radius 0.25, and `nobs` unit spheres above them; every array on the heap with exactly
// the elements the rule may read, so that the sanitizer sees any index outside them.  Agent `done` enters flagged.  Returns 0 where the
// records are what the layout says by hand.
static int line(int size, int nobs, int done) {
    std::unique_ptr<double[]> pos(new double[3 * (std::size_t)size]), radius(new double[(std::size_t)size]);
    std::unique_ptr<uint32_t[]> flags(new uint32_t[(std::size_t)size]);
    std::unique_ptr<double[]> opos(nobs ? new double[3 * (std::size_t)nobs] : nullptr), orad(nobs ? new double[(std::size_t)nobs] : nullptr);
    std::unique_ptr<sca_scene_clearance[]> rec(new sca_scene_clearance[(std::size_t)size]);
    for (int i = 0; i < size; i++) { pos[3 * i] = (double)i; pos[3 * i + 1] = 0.0; pos[3 * i + 2] = 0.0; radius[i] = 0.25; flags[i] = i == done ? 2u : 0u; rec[i] = scene_clearance_empty(); }
    for (int j = 0; j < nobs; j++) { opos[3 * j] = (double)j; opos[3 * j + 1] = 0.0; opos[3 * j + 2] = 3.0; orad[j] = 1.0; }
    for (int step = 1; step <= 2; step++) scene_clearance_step(size, pos.get(), radius.get(), flags.get(), nobs, opos.get(), orad.get(), step, rec.get(), L3Norm{});
    for (int i = 0; i < size; i++) {
        const sca_scene_clearance &r = rec[i];
        if (i == done) { if (r.agent_partner != -1 || r.agent_step != 0 || r.obs_partner != -1 || r.obs_step != 0) return 1; continue; }
        // neighbours one metre away: 1 - 0.5, the lower one first (agent 0 has only agent 1), found in step 1 and not replaced by the equal step 2
        if (size > 1 && (r.agent_clear != 0.5 || r.agent_partner != (i > 0 ? i - 1 : 1) || r.agent_step != 1)) return 2;
        if (size == 1 && (r.agent_partner != -1 || r.agent_step != 0 || r.agent_clear <= 1e300)) return 3;
        // the sphere straight above, where there is one (else the last): 3 - 1.25
        if (nobs > 0 && i < nobs && (r.obs_clear != 1.75 || r.obs_partner != i || r.obs_step != 1)) return 4;
        if (nobs > 0 && i >= nobs && (r.obs_partner != nobs - 1 || r.obs_step != 1)) return 5;
        if (nobs == 0 && (r.obs_partner != -1 || r.obs_step != 0 || r.obs_clear <= 1e300)) return 6;
    }
    return 0;
}
int main() {
    int bad = 0;
    const int cases[][3] = {{1, 0, -1}, {1, 3, -1}, {2, 0, -1}, {5, 2, 3}, {64, 7, 0}, {65, 0, 64}, {130, 131, 7}};
    for (const auto &c : cases)
        if (!bad) { bad = line(c[0], c[1], c[2]); if (bad) bad += 10 * c[0]; }
    std::printf(bad ? "scene_clearance_harness: FAILED (%d)\n" : "scene_clearance_harness: ok\n", bad);
    return bad ? 1 : 0;
}
#endif
