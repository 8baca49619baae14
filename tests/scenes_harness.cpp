// Test-only: the host-side rules of scene batches (sca_amd/csrc/sca_scenes.h, plan_kd_forest of sca_forms.h) and the host side of a
// restart call (sca_scene_restart.h) behind a C interface for tests/test_scenes_cpu.py, tests/test_scene_obstacles_cpu.py,
// tests/test_scene_restart_cpu.py and tests/test_scene_restart_pack_cpu.py.  Plain C++, no HIP.  Not part of the product (sca_amd never
// loads it).  With -DSCENES_MAIN it is a program of its own, for a build under -fsanitize=address,undefined.
#include <cstdio>
#include <string>
#include <vector>

#include "sca_forms.h"
#include "sca_scene_restart.h"
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

// ---- the whole staging block (restart_block_layout) and the host side of a call (restart_pack, the refusals' texts; sca_scene_restart.h) ------
// every section of the block in order -- the agent sections, the new sizes, the obstacle, attribute and path sections: begin and the bytes
// it must hold; returns how many, *total: the block's bytes
int restart_block_sections(int max_n, int max_m, int W, int64_t *begin, int64_t *bytes, int64_t *total) {
    int k = 0;
    const RestartBlock B = restart_block_layout(max_n, max_m, W);
    for (int s = 0; s < RS_SECTIONS; s++, k++) { begin[k] = B.L.off[s]; bytes[k] = restart_section_row_bytes(s) * (int64_t)max_n; }
    begin[k] = B.new_size_off; bytes[k] = (int64_t)sizeof(int32_t) * max_n; k++;
    for (int s = 0; s < RO_SECTIONS; s++, k++) { begin[k] = B.OL.off[s]; bytes[k] = restart_obs_section_bytes(s, max_n, max_m); }
    for (int s = 0; s < RA_SECTIONS; s++, k++) { begin[k] = B.AL.off[s]; bytes[k] = restart_attr_row_bytes(s) * (int64_t)max_n; }
    for (int s = 0; s < RP_SECTIONS; s++, k++) { begin[k] = B.PL.off[s]; bytes[k] = restart_path_section_bytes(s, max_n, W); }
    *total = B.total;
    return k;
}
// ptrs: [17] scene_ids, pos, vel, heading, radius, pref_speed, goal, policy, zaxis, max_run_dist, goal_heading, sizes, obs_counts, obs_pos,
// obs_radius, path_offsets, path_points (NULL entries stay NULL)
static RestartArgs restart_args(int count, const void *const *p) {
    RestartArgs A{count, (const int32_t *)p[0], (const double *)p[1], (const float *)p[2], (const double *)p[3], (const double *)p[4], (const double *)p[5],
                  (const double *)p[6], (const uint8_t *)p[7], (const uint8_t *)p[8], (const double *)p[9], (const double *)p[10]};
    A.sizes = (const int32_t *)p[11];
    A.obs_counts = (const int32_t *)p[12]; A.obs_pos = (const double *)p[13]; A.obs_radius = (const double *)p[14];
    A.path_offsets = (const int32_t *)p[15]; A.path_points = (const double *)p[16];
    return A;
}
// A call that has passed the checks, packed into blk (restart_block_layout(max_n, max_m, W).total bytes).  out6: has, policy_changed,
// size_changed, T, the entries of lp_list, the entries of path_len / path_vpref; size_now: [nscenes]; lp_list, path_len, path_vpref: room
// for n = offsets[nscenes] entries; maxima: radius, pref_speed.
void restart_pack_block(int max_n, int max_m, int W, int nscenes, const int32_t *offsets, int tracker_on, const uint8_t *policy_now, const int32_t *h_size,
                        const int32_t *obs_cap_offsets, int count, const void *const *ptrs, uint8_t *blk, int32_t *out6, int32_t *size_now, int32_t *lp_list,
                        int32_t *path_len, uint8_t *path_vpref, double *maxima) {
    const RestartCtx X{nscenes, offsets, true, false, tracker_on != 0, false, false, policy_now};
    const RestartPlan P = restart_pack(blk, restart_block_layout(max_n, max_m, W), X, restart_args(count, ptrs), h_size, obs_cap_offsets, W);
    out6[0] = (int32_t)P.has; out6[1] = P.policy_changed; out6[2] = P.size_changed; out6[3] = P.T; out6[4] = (int32_t)P.lp_list.size(); out6[5] = (int32_t)P.path_len.size();
    for (int s = 0; s < nscenes; s++) size_now[s] = P.size_now[(size_t)s];
    for (size_t i = 0; i < P.lp_list.size(); i++) lp_list[i] = P.lp_list[i];
    for (size_t i = 0; i < P.path_len.size(); i++) { path_len[i] = P.path_len[i]; path_vpref[i] = P.path_vpref[i]; }
    maxima[0] = P.max_radius; maxima[1] = P.max_pref_speed;
}
// what the library says for a fault of check `which` (0 scene_restart_check, 1 restart_obstacles_check, 2 restart_attrs_check, 3
// restart_paths_check) into out[cap]; returns the error code.  ptrs: as above; obs_cap_offsets: NULL for a context without obstacle slots.
int restart_refusal(int which, int fault, int entry, int total, int nscenes, const int32_t *offsets, int count, const void *const *ptrs,
                    const int32_t *obs_cap_offsets, int struct_bytes, int W, char *out, int cap) {
    const RestartCtx X{nscenes, offsets, true, false, false, false, false, nullptr};
    const RestartArgs A = restart_args(count, ptrs);
    sca_restart_attrs attrs{};
    attrs.struct_bytes = struct_bytes;
    std::string text;
    int code = 0;
    if (which == 0) { text = restart_fault_text(RestartCheck{(RestartFault)fault, entry, total}, X, A); code = scene_restart_error_code((RestartFault)fault); }
    else if (which == 1) { text = restart_obstacles_fault_text(RestartObsCheck{(RestartObsFault)fault, entry, total, 0}, A, obs_cap_offsets); code = restart_obstacles_error_code((RestartObsFault)fault); }
    else if (which == 2) { text = restart_attrs_fault_text(RestartAttrCheck{(RestartAttrFault)fault, entry}, &attrs); code = restart_attrs_error_code((RestartAttrFault)fault); }
    else { text = restart_paths_fault_text(RestartPathCheck{(RestartPathFault)fault, entry, total}, A, W); code = restart_paths_error_code((RestartPathFault)fault); }
    std::snprintf(out, (size_t)cap, "%s", text.c_str());
    return code;
}

}  // extern "C"

#ifdef SCENES_MAIN
// A program of its own, for a build under -fsanitize=address,undefined: restart_block_layout and restart_pack on heap arrays of exactly
// the sizes the call may read and a heap block of exactly the layout's bytes.  Three scenes of capacities 3, 1 and 4, max_m 4, W 2.
#define EXPECT(c) do { if (!(c)) { std::printf("scenes_harness: FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
namespace {
struct Case {
    std::vector<int32_t> ids, sizes, obs_counts, path_offsets;      // empty: NULL
    bool optional, vel, policy;                                    // the optional arrays / vel / policy present
    int W;
};
struct Packed { RestartPlan P; std::vector<uint8_t> blk; RestartBlock B; };
const int32_t OFF[4] = {0, 3, 4, 8}, OBS_CAP[4] = {0, 2, 2, 4};
const uint8_t POLICY_NOW[8] = {0, 4, 3, 4, 1, 5, 4, 2};           // (4: ORCA3D-LP at rows 1, 3, 6)
Packed pack(const Case &k, const int32_t *h_size, const uint8_t *policy_rows) {
    const RestartCtx X{3, OFF, true, false, true, false, false, POLICY_NOW};
    const int T = scene_restart_starts((int)k.ids.size(), OFF, k.ids.data(), k.sizes.empty() ? nullptr : k.sizes.data(), nullptr);
    int nobs = 0;
    for (int c : k.obs_counts) if (c > 0) nobs += c;
    const int npts = k.path_offsets.empty() ? 0 : k.path_offsets.back();
    const std::vector<double> v3((size_t)3 * T, 1.25), v1((size_t)T, 0.5), opos((size_t)3 * nobs, 2.0), orad((size_t)nobs, 0.75), pts((size_t)3 * npts, 3.5);
    const std::vector<float> vel((size_t)3 * T, 0.5f);
    const std::vector<uint8_t> pol(policy_rows, policy_rows + (k.policy ? T : 0)), z((size_t)T, 1);
    RestartArgs A{(int)k.ids.size(), k.ids.data(), v3.data(), k.vel ? vel.data() : nullptr, v3.data(), k.optional ? v1.data() : nullptr, k.optional ? v1.data() : nullptr,
                  k.optional ? v3.data() : nullptr, k.policy ? pol.data() : nullptr, k.optional ? z.data() : nullptr, k.optional ? v1.data() : nullptr,
                  k.optional ? v3.data() : nullptr};
    if (!k.sizes.empty()) A.sizes = k.sizes.data();
    if (!k.obs_counts.empty()) { A.obs_counts = k.obs_counts.data(); A.obs_pos = opos.data(); A.obs_radius = orad.data(); }
    if (!k.path_offsets.empty()) { A.path_offsets = k.path_offsets.data(); A.path_points = pts.data(); }
    Packed R;
    R.B = restart_block_layout(8, 4, k.W);
    R.blk.assign((size_t)R.B.total, 0xA5);
    R.P = restart_pack(R.blk.data(), R.B, X, A, h_size, OBS_CAP, k.W);
    return R;
}
}  // namespace
int main() {
    const int32_t full[3] = {3, 1, 4};
    const uint8_t rows[8] = {3, 1, 5, 4, 2, 0, 4, 3};               // the policies a call brings, by packed row
    {   // the layout: every section inside the block, aligned, none overlapping, for W = 0 and W = 2
        for (int W : {0, 2}) {
            int64_t begin[32], bytes[32], total = 0;
            const int n = restart_block_sections(8, 4, W, begin, bytes, &total);
            EXPECT(n == RS_SECTIONS + 1 + RO_SECTIONS + RA_SECTIONS + RP_SECTIONS);
            for (int i = 0; i < n; i++) EXPECT(begin[i] % RS_ALIGN == 0 && begin[i] + bytes[i] <= (i + 1 < n ? begin[i + 1] : total));
        }
    }
    {   // (a) all scenes full, named out of order; (c) every optional array NULL
        const Packed R = pack(Case{{2, 0, 1}, {}, {}, {}, false, false, false, 0}, full, rows);
        EXPECT(R.P.T == 8 && R.P.has == 0 && !R.P.policy_changed && !R.P.size_changed && R.P.lp_list.empty() && R.P.path_len.empty());
        const int32_t *start = (const int32_t *)(R.blk.data() + R.B.L.off[RS_START]);
        EXPECT(start[0] == 0 && start[1] == 4 && start[2] == 7);
        const float *vel = (const float *)(R.blk.data() + R.B.L.off[RS_VEL]);
        for (int i = 0; i < 24; i++) EXPECT(vel[i] == 0.0f);
    }
    {   // (b) sized, one scene partial and one full; (d) every optional array; (g) the size change drops the LP agent of row 6
        const Packed R = pack(Case{{2, 0}, {2, 3}, {}, {}, true, true, false, 0}, full, rows);
        const uint32_t all = RESTART_HAS_RADIUS | RESTART_HAS_PREF_SPEED | RESTART_HAS_GOAL | RESTART_HAS_ZAXIS | RESTART_HAS_MAX_RUN_DIST | RESTART_HAS_GOAL_HEADING;
        EXPECT(R.P.T == 5 && R.P.has == all && R.P.size_changed && !R.P.policy_changed);
        EXPECT(R.P.size_now[0] == 3 && R.P.size_now[1] == 1 && R.P.size_now[2] == 2);
        EXPECT(R.P.lp_list.size() == 2 && R.P.lp_list[0] == 1 && R.P.lp_list[1] == 3);
        EXPECT(R.P.max_radius == 0.5 && R.P.max_pref_speed == 0.5);
    }
    {   // (e) slot form without path arrays, and with lists of 0, 1 and 2 waypoints; (f) counts -1, 0 and 2; (g) a policy change
        Packed R = pack(Case{{0}, {}, {}, {}, false, true, false, 2}, full, rows);
        EXPECT(R.P.has == RESTART_HAS_PATH_SLOTS && R.P.path_len.size() == 3 && R.P.path_len[2] == 0);
        R = pack(Case{{0, 1, 2}, {3, 1, 2}, {-1, 0, 2}, {0, 0, 1, 3, 3, 4, 4}, false, true, true, 2}, full, rows);
        EXPECT(R.P.has == (RESTART_HAS_PATH_SLOTS | RESTART_HAS_PATHS) && R.P.policy_changed && R.P.size_changed);
        EXPECT(R.P.path_len.size() == 8 && R.P.path_len[1] == 1 && R.P.path_len[2] == 2 && R.P.path_len[4] == 1 && R.P.path_len[6] == 0);
        EXPECT(R.P.path_vpref[1] == 1 && R.P.path_vpref[2] == 0);                            // policy 1 is straight-line, 5 tracked
        const int32_t *head = (const int32_t *)(R.blk.data() + R.B.OL.off[RO_HEAD]);
        const int32_t want[12] = {-1, 0, 0, -1, 0, 2, 0, -1, 2, 2, 0, 4};
        for (int i = 0; i < 12; i++) EXPECT(head[i] == want[i]);
        EXPECT(R.P.lp_list.size() == 1 && R.P.lp_list[0] == 3);                               // row 3 keeps policy 4, row 1 changes it, row 6 is vacated
    }
    std::printf("scenes_harness: ok\n");
    return 0;
}
#endif
