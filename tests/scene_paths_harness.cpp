// scene_paths_harness.cpp -- TEST-ONLY host build of the waypoint lists' slot form: the pure rules of sca_scenes.h behind sca_set_path_slots and
// sca_restart_scenes_paths (path_slots_check, restart_paths_check, restart_paths_layout, path_slot_index) and the body k_waypoint and
// k_waypoint_slots share (waypoint_agent, sca_core.h), run over plain arrays in both forms, so that all of it can be checked on a machine
// without a GPU.  With -DSCENE_PATHS_MAIN it is a program of its own (for the sanitizers): it runs the same calls and prints their answers.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "sca_core.h"
#include "sca_scenes.h"

using namespace sca;

namespace {
// the members of DeviceView that waypoint_agent reads and writes
struct HostView {
    const PubRec *rec;
    const uint8_t *policy;
    const double *goal, *pref_speed;
    double *vpref_ext;
    uint8_t *vpref_mode;
};
std::vector<PubRec> records(int n, const double *pos, const double *radius, const uint8_t *flags) {
    std::vector<PubRec> rec((size_t)n);
    for (int i = 0; i < n; i++) {
        rec[i].px = pos[3 * i]; rec[i].py = pos[3 * i + 1]; rec[i].pz = pos[3 * i + 2];
        rec[i].vx = rec[i].vy = rec[i].vz = 0.0f;
        rec[i].flags = flags[i]; rec[i].radius = radius[i];
    }
    return rec;
}
}  // namespace

extern "C" {

// out: fault, entry, total; returns the error code
int slots_check(int agents_set, int partition_on, int ctx_n, int max_agents, int W, int n, const int32_t *offsets, const double *points, int *out) {
    const PathSlotCheck k = path_slots_check(agents_set != 0, partition_on != 0, ctx_n, max_agents, W, n, offsets, points);
    out[0] = (int)k.fault; out[1] = k.entry; out[2] = k.total;
    return path_slots_error_code(k.fault);
}
int paths_check(int slot_form, int W, int T, const int32_t *path_offsets, const double *path_points, int *out) {
    const RestartPathCheck k = restart_paths_check(slot_form != 0, W, T, path_offsets, path_points);
    out[0] = (int)k.fault; out[1] = k.entry; out[2] = k.total;
    return restart_paths_error_code(k.fault);
}
int refuses(int paths_on, int slot_form) { return restart_refuses_paths(paths_on != 0, slot_form != 0) ? 1 : 0; }
int64_t slot_index(int W, int a) { return path_slot_index(W, a); }
int addressable(int W, int max_agents) { return path_slots_addressable(W, max_agents) ? 1 : 0; }
int64_t points_max() { return PATH_SLOT_POINTS_MAX; }
int path_section_count() { return RP_SECTIONS; }
uint32_t path_bits() { return RESTART_HAS_PATH_SLOTS | RESTART_HAS_PATHS; }

// every section of the restart's block as sca_restart_scenes lays it out: begin / size per section, in order; returns how many
int block_sections(int max_n, int max_m, int W, int64_t *begin, int64_t *size, int64_t *total) {
    int k = 0;
    const RestartBlock B = restart_block_layout(max_n, max_m, W);
    for (int s = 0; s < RS_SECTIONS; s++, k++) { begin[k] = B.L.off[s]; size[k] = restart_section_row_bytes(s) * (int64_t)max_n; }
    begin[k] = B.new_size_off; size[k] = (int64_t)sizeof(int32_t) * max_n; k++;              // the new sizes
    for (int s = 0; s < RO_SECTIONS; s++, k++) { begin[k] = B.OL.off[s]; size[k] = restart_obs_section_bytes(s, max_n, max_m); }
    for (int s = 0; s < RA_SECTIONS; s++, k++) { begin[k] = B.AL.off[s]; size[k] = restart_attr_row_bytes(s) * (int64_t)max_n; }
    for (int s = 0; s < RP_SECTIONS; s++, k++) { begin[k] = B.PL.off[s]; size[k] = restart_path_section_bytes(s, max_n, W); }
    *total = B.total;
    return k;
}

// one pass of the shared body over n agents, the lists in block form (CSR) ...
void step_block(int n, const int32_t *off, const double *pts, int32_t *rem, double *now_goal, const double *pos, const double *radius, const uint8_t *flags,
                const uint8_t *policy, const double *goal, const double *pref_speed, double *vpref_ext, uint8_t *vpref_mode) {
    const std::vector<PubRec> rec = records(n, pos, radius, flags);
    const HostView d{rec.data(), policy, goal, pref_speed, vpref_ext, vpref_mode};
    for (int a = 0; a < n; a++) waypoint_agent(d, a, pts + 3 * (size_t)off[a], off[a + 1] > off[a], rem, now_goal);
}
// ... and in slot form: rooms[3 * W * n], row a's list from 3 * path_slot_index(W, a), len[a] elements as set
void step_slots(int n, int W, const double *rooms, const int32_t *len, int32_t *rem, double *now_goal, const double *pos, const double *radius, const uint8_t *flags,
                const uint8_t *policy, const double *goal, const double *pref_speed, double *vpref_ext, uint8_t *vpref_mode) {
    const std::vector<PubRec> rec = records(n, pos, radius, flags);
    const HostView d{rec.data(), policy, goal, pref_speed, vpref_ext, vpref_mode};
    for (int a = 0; a < n; a++) waypoint_agent(d, a, rooms + 3 * path_slot_index(W, a), len[a] > 0, rem, now_goal);
}

}  // extern "C"

#ifdef SCENE_PATHS_MAIN
int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    int out[3];
    // three rows with lists of 2, 0 and 3 waypoints; exact-size buffers, so that a read past them is the sanitizer's
    std::vector<int32_t> off{0, 2, 2, 5};
    std::vector<double> pts(15);
    for (int i = 0; i < 15; i++) pts[i] = 0.5 * i;
    int rc = slots_check(1, 0, 3, 3, 3, 3, off.data(), pts.data(), out);
    std::printf("slots ok: rc %d fault %d entry %d total %d\n", rc, out[0], out[1], out[2]);
    rc = slots_check(1, 0, 3, 3, 2, 3, off.data(), pts.data(), out);
    std::printf("slots too long: rc %d fault %d entry %d total %d\n", rc, out[0], out[1], out[2]);
    rc = slots_check(1, 0, 3, 3, 3, 3, nullptr, nullptr, out);
    std::printf("slots no lists: rc %d fault %d entry %d total %d\n", rc, out[0], out[1], out[2]);
    pts[14] = nan;
    rc = slots_check(1, 0, 3, 3, 3, 3, off.data(), pts.data(), out);
    std::printf("slots not finite: rc %d fault %d entry %d total %d\n", rc, out[0], out[1], out[2]);
    rc = paths_check(1, 3, 3, off.data(), pts.data(), out);
    std::printf("paths not finite: rc %d fault %d entry %d total %d\n", rc, out[0], out[1], out[2]);
    pts[14] = 7.0;
    rc = paths_check(1, 3, 3, off.data(), pts.data(), out);
    std::printf("paths ok: rc %d fault %d entry %d total %d\n", rc, out[0], out[1], out[2]);
    rc = paths_check(0, 0, 3, off.data(), pts.data(), out);
    std::printf("paths no slots: rc %d fault %d entry %d total %d\n", rc, out[0], out[1], out[2]);
    rc = paths_check(1, 3, 3, off.data(), nullptr, out);
    std::printf("paths no points: rc %d fault %d entry %d total %d\n", rc, out[0], out[1], out[2]);
    for (int W : {0, 5}) {
        int64_t begin[32], size[32], total = 0;
        const int k = block_sections(130, 9, W, begin, size, &total);
        std::printf("layout %d:", W);
        for (int i = k - RP_SECTIONS; i < k; i++) std::printf(" %lld+%lld", (long long)begin[i], (long long)size[i]);
        std::printf(" total %lld\n", (long long)total);
    }
    // the two forms of the step over the three rows, W = 3 (exactly the longest list) and W = 4: a straight-line agent with a list, a
    // straight-line agent without one, a tracked agent with a list; two passes
    const double pos[9] = {0, 0, 5, 3, 0, 5, 0, 3, 5}, goal[9] = {10, 0, 5, -10, 0, 5, 0, -10, 5}, radius[3] = {0.5, 0.5, 0.5}, ps[3] = {1.0, 1.0, 1.0};
    const uint8_t flags[3] = {0, 0, 0}, policy[3] = {1, 3, 0};
    for (int W : {3, 4}) {
        std::vector<double> rooms(3 * (size_t)W * 3, 0.0);
        std::vector<int32_t> len(3);
        for (int a = 0; a < 3; a++) {
            len[a] = off[a + 1] - off[a];
            for (int k = 0; k < 3 * len[a]; k++) rooms[3 * (size_t)slot_index(W, a) + k] = pts[3 * (size_t)off[a] + k];
        }
        std::vector<int32_t> rem_b(len), rem_s(len);
        std::vector<double> ng_b(9, nan), ng_s(9, nan), vp_b(9, 0.0), vp_s(9, 0.0);
        std::vector<uint8_t> mode_b(3, 0), mode_s(3, 0);
        bool same = true;
        for (int pass = 0; pass < 2; pass++) {
            step_block(3, off.data(), pts.data(), rem_b.data(), ng_b.data(), pos, radius, flags, policy, goal, ps, vp_b.data(), mode_b.data());
            step_slots(3, W, rooms.data(), len.data(), rem_s.data(), ng_s.data(), pos, radius, flags, policy, goal, ps, vp_s.data(), mode_s.data());
            for (int i = 0; i < 3; i++) same = same && rem_b[i] == rem_s[i] && mode_b[i] == mode_s[i];
            for (int i = 0; i < 9; i++) same = same && ng_b[i] == ng_s[i] && vp_b[i] == vp_s[i];
        }
        std::printf("step W %d: same %d rem %d %d %d mode %d %d %d\n", W, same ? 1 : 0, rem_s[0], rem_s[1], rem_s[2], mode_s[0], mode_s[1], mode_s[2]);
    }
    return 0;
}
#endif
