// sca_scene_restart.h -- the host side of sca_restart_scenes (include/sca_hip.h) as pure functions: no HIP, no sca_ctx.  The rules, the
// block's layout and the class table are sca_scenes.h's; here is what sca_hip.hip's restart_scenes() does with them between the checks
// and the launch, and the texts of its refusals (tests/scenes_harness.cpp runs all of it without a GPU):
//   restart_*_text     what each of the four checks' faults says, with the entry point's name and the numbers it names
//   restart_pack       the caller's arrays into the staging block, and the RestartPlan the later stages work from
// Two parts of the block need what only sca_hip.hip has -- the obstacle trees (kd_build_host) and the AgentPar rows (cos_threshold, the
// libm pointer): two helpers there fill them, and the plan's class members, between restart_pack and the launch.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "sca_scenes.h"

namespace sca {

// ---- the refusals ----------------------------------------------------------------------------------------------------------------------
// X, A: what scene_restart_check was given
inline std::string restart_fault_text(const RestartCheck &k, const RestartCtx &X, const RestartArgs &A) {
    const std::string at = std::to_string(k.entry);
    switch (k.fault) {
    case RESTART_NO_SCENES: return "sca_restart_scenes: no scenes -- sca_set_scenes first";
    case RESTART_NO_STATE: return "sca_restart_scenes: no state yet -- sca_set_state first";
    case RESTART_MID_STEP: return "sca_restart_scenes between a policy pass and its env update: finish the step first";
    case RESTART_BAD_COUNT: return "sca_restart_scenes: count must be positive and scene_ids not NULL";
    case RESTART_BAD_ID: return "sca_restart_scenes: scene_ids[" + at + "] = " + std::to_string(A.scene_ids[k.entry]) + " is not a scene of this context (0 .. " + std::to_string(X.nscenes - 1) + ")";
    case RESTART_REPEATED_ID: return "sca_restart_scenes: scene_ids[" + at + "] = " + std::to_string(A.scene_ids[k.entry]) + " is named twice";
    case RESTART_NO_ARRAYS: return "sca_restart_scenes: pos and heading must not be NULL";
    case RESTART_NOT_FINITE: return "sca_restart_scenes: row " + at + " holds a number that is not finite";
    case RESTART_BAD_POLICY: return "sca_restart_scenes: row " + at + " has a policy above SCA_POLICY_RVO3D_DUBINS";
    case RESTART_NOT_POSITIVE: return "sca_restart_scenes: row " + at + " has a radius, pref_speed or max_run_dist that is not positive";
    case RESTART_GOAL_HEADING: return "sca_restart_scenes: goal_heading without a device tracker (sca_device_tracker_enable)";
    case RESTART_BAD_SIZE: return "sca_restart_scenes_sized: sizes[" + at + "] = " + std::to_string(A.sizes[k.entry]) + ": scene " + std::to_string(A.scene_ids[k.entry]) + " holds 1 .. " +
                                  std::to_string(X.offsets[A.scene_ids[k.entry] + 1] - X.offsets[A.scene_ids[k.entry]]) + " agents (its capacity)";
    case RESTART_PATHS: return "sca_restart_scenes with waypoint lists set (sca_set_paths): the lists are one block, replacing a scene's lists is not available";
    default: return "sca_restart_scenes: row " + at + " changes an agent between a tracked and an untracked policy while per-agent tracker attributes are set "
                    "(sca_device_tracker_set_agent_params): the tracker's classes are cut by policy";
    }
}
// cap_offsets: the obstacle slots' capacities, NULL: the context has none
inline std::string restart_obstacles_fault_text(const RestartObsCheck &k, const RestartArgs &A, const int32_t *cap_offsets) {
    const std::string at = std::to_string(k.entry);
    switch (k.fault) {
    case RESTART_OBS_NO_SLOTS: return "sca_restart_scenes_obstacles: obs_counts[" + at + "] = " + std::to_string(A.obs_counts[k.entry]) + " but the context has no obstacle slots -- sca_set_scene_obstacle_slots first";
    case RESTART_OBS_BAD_COUNT: return "sca_restart_scenes_obstacles: obs_counts[" + at + "] = " + std::to_string(A.obs_counts[k.entry]) + ": scene " + std::to_string(A.scene_ids[k.entry]) +
                                       " keeps its set (-1) or takes 0 .. its obstacle capacity" + (cap_offsets ? " " + std::to_string(cap_offsets[A.scene_ids[k.entry] + 1] - cap_offsets[A.scene_ids[k.entry]]) : std::string());
    case RESTART_OBS_NO_ARRAYS: return "sca_restart_scenes_obstacles: obs_pos and obs_radius must not be NULL with " + std::to_string(k.total) + " obstacles";
    case RESTART_OBS_NOT_FINITE: return "sca_restart_scenes_obstacles: obstacle row " + at + " has a position that is not finite";
    default: return "sca_restart_scenes_obstacles: obstacle row " + at + " has a radius that is not positive";
    }
}
inline std::string restart_attrs_fault_text(const RestartAttrCheck &k, const sca_restart_attrs *attrs) {
    const std::string at = std::to_string(k.entry);
    switch (k.fault) {
    case RESTART_ATTR_STRUCT: return "sca_restart_scenes_attrs: attrs->struct_bytes = " + std::to_string(attrs->struct_bytes) + " is not a size of sca_restart_attrs (" +
                                     std::to_string(RESTART_ATTR_HEAD_BYTES) + " .. " + std::to_string(sizeof(sca_restart_attrs)) + ", whole pointers)";
    case RESTART_ATTR_RESERVED: return "sca_restart_scenes_attrs: attrs->reserved must be 0";
    case RESTART_ATTR_NO_TRACKER: return "sca_restart_scenes_attrs: turning_radius / pitch_lo / pitch_hi without a device tracker (sca_device_tracker_enable)";
    case RESTART_ATTR_SOLVER: return "sca_restart_scenes_attrs: row " + at + " has an attribute out of range (see sca_params)";
    default: return "sca_restart_scenes_attrs: row " + at + " has a turning radius / pitch limits out of range (R > 0, pitch_lo < pitch_hi)";
    }
}
// W: the room per row of the context's slot form
inline std::string restart_paths_fault_text(const RestartPathCheck &k, const RestartArgs &A, int W) {
    const std::string at = std::to_string(k.entry);
    switch (k.fault) {
    case RESTART_PATHS_NO_SLOTS: return "sca_restart_scenes_paths: path arrays, but the context's lists are not in slot form -- sca_set_path_slots first";
    case RESTART_PATHS_BAD_START: return "sca_restart_scenes_paths: path_offsets[0] must be 0";
    case RESTART_PATHS_DECREASING: return "sca_restart_scenes_paths: path_offsets decrease at row " + at;
    case RESTART_PATHS_TOO_LONG: return "sca_restart_scenes_paths: row " + at + " brings a list of " + std::to_string(A.path_offsets[k.entry + 1] - A.path_offsets[k.entry]) +
                                        " waypoints, a row has room for " + std::to_string(W) + " (sca_set_path_slots)";
    case RESTART_PATHS_NO_POINTS: return "sca_restart_scenes_paths: path_points is NULL with " + std::to_string(k.total) + " waypoints";
    default: return "sca_restart_scenes_paths: row " + at + " has a waypoint that is not finite";
    }
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------------
// What the stages behind the packing need of a call: the launch (`has`), the copies behind it, and the commit of the host mirrors.
struct RestartPlan {
    // from restart_pack
    int T = 0;                                 // the packed rows
    uint32_t has = 0;                          // RESTART_HAS_*
    bool policy_changed = false, size_changed = false;
    std::vector<int32_t> size_now;             // [nscenes] every scene's size behind the call
    std::vector<int32_t> lp_list;              // K3's list behind the call, where a policy or a size changed: the ORCA3D-LP agents of the occupied rows, ascending
    std::vector<int32_t> path_len;             // slot form: per named scene, for every row of its CAPACITY in order, the list's length (0: vacant, or no lists brought)
    std::vector<uint8_t> path_vpref;           // ... and "a straight-line agent with a path" (sca_set_vpref, paths_clear)
    double max_radius = 0, max_pref_speed = 0; // over the call's rows (0: the array was NULL)
    // from the obstacle trees' helper
    int obs_replaced = 0;                      // the named scenes whose set the call replaces (RestartObsCheck::replaced)
    double obs_max_radius = 0;
    // from the attribute sections' helper: the class-table work on copies, which replace the context's behind the synchronisation
    bool send_solver = false, send_planner = false, ap_first = false, table_on = false, cls_whole = false;
    double env_nd = 0, env_ms = 0, env_dt = 0; // the envelope of the call's solver attributes
    std::vector<TrackTriple> trip_new;
    std::vector<uint8_t> cls_new;
    ClassTable table_new;
    ClassUpdate cu{0, false, false};
};

// The caller's arrays into the block, behind the four checks: ids, starts and new sizes; the policy and vpref-mode bytes; position, heading
// and velocity (zeros where vel == NULL); every optional section with its bit; the path offsets and the points present; the four head
// words per named scene (the replaced scenes' trees follow from sca_hip.hip).  X: as scene_restart_check read it (offsets, policy_now,
// tracker_on); h_size: [nscenes] the scenes' sizes as they stand; obs_cap_offsets: the obstacle slots' capacities (read for a count >= 0
// only, which the check has refused without slots); path_W: the room per row in slot form, 0: none.
inline RestartPlan restart_pack(uint8_t *blk, const RestartBlock &B, const RestartCtx &X, const RestartArgs &A, const int32_t *h_size, const int32_t *obs_cap_offsets, int path_W) {
    RestartPlan P;
    const RestartLayout &L = B.L;
    const int count = A.count;
    const int32_t *off = X.offsets;
    int32_t *ids = (int32_t *)(blk + L.off[RS_IDS]), *start = (int32_t *)(blk + L.off[RS_START]), *new_size = (int32_t *)(blk + B.new_size_off);
    uint8_t *pol = blk + L.off[RS_POLICY], *mode = blk + L.off[RS_VPREF_MODE];
    const std::size_t T = (std::size_t)scene_restart_starts(count, off, A.scene_ids, A.sizes, start);
    P.T = (int)T;
    P.size_now.assign(h_size, h_size + X.nscenes);                     // a vacant row keeps its policy and is in no list
    for (int e = 0; e < count; e++) {
        const int s = A.scene_ids[e], lo = off[s], ns = scene_restart_rows(off, A.scene_ids, A.sizes, e);
        ids[e] = s; new_size[e] = ns;
        P.size_changed = P.size_changed || ns != h_size[s];
        P.size_now[s] = ns;
        for (int a = lo, r = start[e]; a < lo + ns; a++, r++) {
            const uint8_t p = A.policy ? A.policy[r] : X.policy_now[a];
            P.policy_changed = P.policy_changed || p != X.policy_now[a];
            pol[r] = p;
            mode[r] = X.tracker_on && restart_policy_tracked(p) ? 1 : 0;      // sca_device_tracker_enable's rule; 0 without a tracker (sca_set_agents')
            if (A.radius) P.max_radius = std::max(P.max_radius, A.radius[r]);
            if (A.pref_speed) P.max_pref_speed = std::max(P.max_pref_speed, A.pref_speed[r]);
        }
    }
    std::memcpy(blk + L.off[RS_POS], A.pos, sizeof(double) * 3 * T);
    std::memcpy(blk + L.off[RS_HEADING], A.heading, sizeof(double) * 3 * T);
    if (A.vel) std::memcpy(blk + L.off[RS_VEL], A.vel, sizeof(float) * 3 * T); else std::memset(blk + L.off[RS_VEL], 0, sizeof(float) * 3 * T);
    const auto put = [&](int sec, const void *src, std::size_t bytes, uint32_t bit) { if (src) { std::memcpy(blk + L.off[sec], src, bytes); P.has |= bit; } };
    put(RS_GOAL, A.goal, sizeof(double) * 3 * T, RESTART_HAS_GOAL);
    put(RS_GOAL_HEADING, A.goal_heading, sizeof(double) * 3 * T, RESTART_HAS_GOAL_HEADING);
    put(RS_RADIUS, A.radius, sizeof(double) * T, RESTART_HAS_RADIUS);
    put(RS_PREF_SPEED, A.pref_speed, sizeof(double) * T, RESTART_HAS_PREF_SPEED);
    put(RS_MAX_RUN_DIST, A.max_run_dist, sizeof(double) * T, RESTART_HAS_MAX_RUN_DIST);
    put(RS_ZAXIS, A.zaxis, T, RESTART_HAS_ZAXIS);
    if (path_W > 0) {                                                  // the lists travel packed: the offsets and the points actually present
        P.has |= RESTART_HAS_PATH_SLOTS;
        if (A.path_offsets) {
            std::memcpy(blk + B.PL.off[RP_OFF], A.path_offsets, sizeof(int32_t) * (T + 1));
            if (A.path_offsets[T] > 0) std::memcpy(blk + B.PL.off[RP_PTS], A.path_points, sizeof(double) * 3 * (std::size_t)A.path_offsets[T]);
            P.has |= RESTART_HAS_PATHS;
        }
        for (int e = 0; e < count; e++) {                             // the lists' lengths over the scene's capacity: the vacant rows' are empty
            const int s = A.scene_ids[e];
            for (int a = off[s], r = start[e]; a < off[s + 1]; a++, r++) {
                const int32_t len = A.path_offsets && a < off[s] + new_size[e] ? A.path_offsets[r + 1] - A.path_offsets[r] : 0;
                P.path_len.push_back(len);
                P.path_vpref.push_back(len > 0 && !restart_policy_tracked(pol[r]) ? 1 : 0);       // (len > 0: an occupied row, pol[r] is its policy)
            }
        }
    }
    int32_t *head = (int32_t *)(blk + B.OL.off[RO_HEAD]);
    for (int e = 0, at = 0; e < count; e++) {                          // at most max_obstacles rows in all: the named scenes' capacities are disjoint ranges
        const int ms = A.obs_counts ? A.obs_counts[e] : -1;            // -1: the scene keeps its set, and the words behind the count are not read
        const int base = ms >= 0 ? obs_cap_offsets[A.scene_ids[e]] : 0;
        head[RO_HEAD_WORDS * e] = ms; head[RO_HEAD_WORDS * e + 1] = base; head[RO_HEAD_WORDS * e + 2] = at; head[RO_HEAD_WORDS * e + 3] = ms > 0 ? 2 * base : -1;
        if (ms > 0) at += ms;
    }
    if (P.policy_changed || P.size_changed) {                          // K3's list (the block holds the named scenes' policies)
        std::vector<uint8_t> now(X.policy_now, X.policy_now + off[X.nscenes]);
        for (int e = 0; e < count; e++)
            for (int a = off[A.scene_ids[e]], r = start[e]; a < off[A.scene_ids[e]] + new_size[e]; a++, r++) now[a] = pol[r];
        for (int sc = 0; sc < X.nscenes; sc++)
            for (int i = off[sc]; i < off[sc] + P.size_now[sc]; i++) if (now[i] == SCA_POLICY_ORCA3D_LP) P.lp_list.push_back(i);
    }
    return P;
}

}  // namespace sca
