// sca_scenes.h -- scene batches (sca_set_scenes): the host-side rules, as pure functions.  No HIP, no sca_ctx: sca_hip.hip calls them and
// turns their answers into error codes and messages; tests/scenes_harness.cpp checks them without a GPU.
//
// One context holds B scenes; scene s is the contiguous agent range [offsets[s], offsets[s + 1]).  Each scene is one job of k_kd_block
// (its whole tree by one workgroup in LDS), hence at most KD_WAVE_CAP agents per scene.
// Also here, because a restart is what needs them: the rules of the waypoint lists' slot form (sca_set_path_slots), which works with or
// without scenes.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/sca_hip.h"
#include "sca_constants.h"

namespace sca {

enum SceneFault {
    SCENES_OK = 0,
    SCENES_NONE,            // nscenes == 0 or offsets == NULL: the context is a plain one
    SCENES_BAD_COUNT,       // nscenes < 0 or more scenes than agents
    SCENES_BAD_START,       // offsets[0] != 0
    SCENES_NOT_INCREASING,  // an empty scene, or offsets that decrease
    SCENES_BAD_END,         // offsets[nscenes] != n
    SCENES_TOO_LARGE        // a scene of more than KD_WAVE_CAP agents
};
// fault: which rule failed; scene: the first scene that breaks it (-1: none in particular); largest: the largest scene's agent count (SCENES_OK)
struct SceneCheck { SceneFault fault; int scene; int largest; };
inline SceneCheck scenes_check(int n, int nscenes, const int32_t *offsets) {
    if (nscenes == 0 || offsets == nullptr) return {SCENES_NONE, -1, 0};
    if (nscenes < 0 || nscenes > n) return {SCENES_BAD_COUNT, -1, 0};
    if (offsets[0] != 0) return {SCENES_BAD_START, 0, 0};
    int largest = 0;
    for (int s = 0; s < nscenes; s++) {
        if (offsets[s + 1] <= offsets[s]) return {SCENES_NOT_INCREASING, s, 0};
        if (offsets[s + 1] > n) return {SCENES_BAD_END, s, 0};          // (also keeps every later read of a per-agent array in bounds)
        const int size = offsets[s + 1] - offsets[s];
        if (size > KD_WAVE_CAP) return {SCENES_TOO_LARGE, s, size};
        if (size > largest) largest = size;
    }
    if (offsets[nscenes] != n) return {SCENES_BAD_END, nscenes - 1, 0};
    return {SCENES_OK, -1, largest};
}
// what sca_set_scenes returns for a fault
inline int scenes_error_code(SceneFault f) {
    return f == SCENES_OK || f == SCENES_NONE ? SCA_OK : (f == SCENES_TOO_LARGE ? SCA_ERR_UNSUPPORTED : SCA_ERR_ARG);
}

// kdTree.agentIDs of a context with scenes carries global ids, and a scene's positions hold that scene's ids only (a build permutes inside
// a job's range).  The first position whose id lies outside its scene, -1: none.  (offsets: checked by scenes_check)
inline int scenes_perm_fault(int nscenes, const int32_t *offsets, const int32_t *perm) {
    for (int s = 0; s < nscenes; s++)
        for (int p = offsets[s]; p < offsets[s + 1]; p++)
            if (perm[p] < offsets[s] || perm[p] >= offsets[s + 1]) return p;
    return -1;
}

// the neighbour mode a context with scenes runs for the one that was asked for: the forest of kd-trees is the scene form, SCA_NBR_AUTO
// resolves to it (one more place where the grid cannot help: its cell key carries no scene id), the grid and the host build have none (-1)
inline int scenes_neighbor_mode(int requested) {
    return requested == SCA_NBR_KDTREE || requested == SCA_NBR_AUTO ? (int)SCA_NBR_KDTREE : -1;
}

// ---- per-scene obstacle sets (sca_set_scene_obstacles) ---------------------------------------------------------------------------------------
// Scene s meets obstacles [obs_offsets[s], obs_offsets[s + 1]) and no others; a scene may have none.  The obstacle tree becomes a forest
// like the agents': one tree per scene, built over that scene's obstacles alone with local ids 0 .. m_s - 1 (what makes every value the
// single-scene context's), laid side by side in otree[2M] / owide[2M] with scene s's nodes numbered from 2 * obs_offsets[s] (a tree over k
// members occupies 2k - 1 nodes: the ranges are disjoint).
enum SceneObsFault {
    SCENE_OBS_OK = 0,
    SCENE_OBS_BAD_COUNT,    // nscenes is not the context's scene count
    SCENE_OBS_NO_OFFSETS,   // obs_offsets == NULL
    SCENE_OBS_BAD_START,    // obs_offsets[0] != 0
    SCENE_OBS_DECREASING,   // obs_offsets[s + 1] < obs_offsets[s] (equal is fine: a scene without obstacles)
    SCENE_OBS_TOO_MANY,     // obs_offsets[nscenes] > sca_create's max_obstacles
    SCENE_OBS_NO_ARRAYS     // a positive total with pos == NULL or radius == NULL
};
// fault: which rule failed; scene: the first scene that breaks it (-1: none in particular); total: obs_offsets[nscenes] (SCENE_OBS_OK, _TOO_MANY, _NO_ARRAYS)
struct SceneObsCheck { SceneObsFault fault; int scene; int total; };
inline SceneObsCheck scene_obstacles_check(int ctx_nscenes, int max_obstacles, int nscenes, const int32_t *obs_offsets, bool have_pos, bool have_radius) {
    if (nscenes != ctx_nscenes || nscenes <= 0) return {SCENE_OBS_BAD_COUNT, -1, 0};
    if (obs_offsets == nullptr) return {SCENE_OBS_NO_OFFSETS, -1, 0};
    if (obs_offsets[0] != 0) return {SCENE_OBS_BAD_START, 0, 0};
    for (int s = 0; s < nscenes; s++)
        if (obs_offsets[s + 1] < obs_offsets[s]) return {SCENE_OBS_DECREASING, s, 0};
    const int total = obs_offsets[nscenes];
    if (total > max_obstacles) return {SCENE_OBS_TOO_MANY, -1, total};
    if (total > 0 && !(have_pos && have_radius)) return {SCENE_OBS_NO_ARRAYS, -1, total};
    return {SCENE_OBS_OK, -1, total};
}
// what sca_set_scene_obstacles returns for a fault
inline int scene_obstacles_error_code(SceneObsFault f) { return f == SCENE_OBS_OK ? SCA_OK : SCA_ERR_ARG; }

// where scene s's obstacle walks start: the root record of its tree in the forest, -1: the scene has no obstacles (no walk at all)
inline int scene_obstacle_root(const int32_t *obs_offsets, int s) {
    return obs_offsets[s + 1] - obs_offsets[s] > 0 ? 2 * obs_offsets[s] : -1;
}

// A tree built over one scene's obstacles alone (nodes numbered from 0, members 0 .. m_s - 1; Node: begin, end, left, right) as it stands
// in the forest: member ranges shifted by obs_begin = obs_offsets[s], child links by the node base 2 * obs_begin.  A leaf (at most max_leaf
// members, kdTree.py:53) keeps its links at 0, the "no children" the build writes; unused records (begin == end) stay as they are.  The
// caller copies nodes[i] to 2 * obs_begin + i.
template <class Node>
inline void scene_obstacle_shift(Node *nodes, int nnodes, int obs_begin, int max_leaf) {
    for (int i = 0; i < nnodes; i++) {
        Node &nd = nodes[i];
        if (nd.end == nd.begin) continue;
        const bool inner = nd.end - nd.begin > max_leaf;
        nd.begin += obs_begin; nd.end += obs_begin;
        if (inner) { nd.left += 2 * obs_begin; nd.right += 2 * obs_begin; }
    }
}

// ---- restarting scenes in place (sca_restart_scenes) ------------------------------------------------------------------------------------------
// A restart puts a new episode into a slot: the named scenes get new start states and constants, every other scene is untouched.  The
// caller's arrays are packed in the order of scene_ids -- T rows in all, scene_ids[b]'s rows from the sum of the sizes before it.
enum RestartFault {
    RESTART_OK = 0,
    RESTART_NO_SCENES,      // the context holds no scenes                                                     } SCA_ERR_STATE
    RESTART_NO_STATE,       // no state yet (sca_set_state / the host block)                                   }
    RESTART_MID_STEP,       // between a policy pass and its env update                                        }
    RESTART_BAD_COUNT,      // count <= 0 or scene_ids == NULL                                                 } SCA_ERR_ARG
    RESTART_BAD_ID,         // an id outside 0 .. nscenes - 1 (entry: its index in scene_ids)                  }
    RESTART_REPEATED_ID,    // an id named twice (entry: the index of the second mention)                      }
    RESTART_NO_ARRAYS,      // pos or heading NULL                                                             }
    RESTART_NOT_FINITE,     // a number that is not finite (entry: the packed row)                             }
    RESTART_BAD_POLICY,     // a policy above SCA_POLICY_RVO3D_DUBINS (entry: the packed row)                  }
    RESTART_NOT_POSITIVE,   // radius, pref_speed or max_run_dist <= 0 (entry: the packed row)                 }
    RESTART_GOAL_HEADING,   // goal_heading passed while no device tracker is enabled                          }
    RESTART_PATHS,          // waypoint lists are set: one CSR block, replacing a scene's lists is not built   } SCA_ERR_UNSUPPORTED
    RESTART_TRACKED_CHANGE, // a policy that changes an agent's tracked / untracked status while per-agent     }
                            // tracker attributes are set: the tracker's classes are cut by policy (entry: the packed row)
    RESTART_BAD_SIZE        // sca_restart_scenes_sized: a size < 1 or above the slot's capacity (entry: its      SCA_ERR_ARG
                            // index in sizes); checked with the ids, last in the enum to keep the numbering
};
// the caller's arguments, as sca_restart_scenes takes them
struct RestartArgs {
    int count; const int32_t *scene_ids;
    const double *pos; const float *vel; const double *heading, *radius, *pref_speed, *goal; const uint8_t *policy, *zaxis;
    const double *max_run_dist, *goal_heading;
    const int32_t *sizes = nullptr;            // [count] sca_restart_scenes_sized: the rows each named scene brings; NULL: its capacity
    const int32_t *obs_counts = nullptr; const double *obs_pos = nullptr, *obs_radius = nullptr;   // sca_restart_scenes_obstacles (restart_obstacles_check)
    const int32_t *path_offsets = nullptr; const double *path_points = nullptr;                    // sca_restart_scenes_paths (restart_paths_check)
};
// what the rules read of the context
struct RestartCtx {
    int nscenes; const int32_t *offsets;       // 0 / NULL: no scenes
    bool state_set, scene_begun, tracker_on, paths_on, tracker_per_agent;
    const uint8_t *policy_now;                 // [n] the agents' policies as they stand
};
// fault: which rule failed; entry: where (-1: nowhere in particular); total: T, the rows the arrays hold (RESTART_OK and every fault found after the ids)
struct RestartCheck { RestartFault fault; int entry; int total; };
inline bool restart_policy_tracked(int pol) { return pol == SCA_POLICY_SCA || pol == SCA_POLICY_RVO3D_DUBINS; }
inline bool restart_finite(double x) { return x - x == 0.0; }       // (no <cmath>: false for NaN and both infinities)

// ---- slots of a capacity (sca_restart_scenes_sized) -------------------------------------------------------------------------------------------
// Scene s keeps its range [offsets[s], offsets[s + 1]) as a CAPACITY and holds size[s] agents, 1 <= size[s] <= capacity, in its first
// size[s] rows; the rows behind them are vacant.  A context that never calls the sized restart has size[s] == capacity throughout.
inline bool scene_size_ok(int size, int capacity) { return size >= 1 && size <= capacity; }
// the rows the b-th named scene brings: sizes[b], or the slot's capacity where sizes == NULL (ids: checked by the caller)
inline int scene_restart_rows(const int32_t *offsets, const int32_t *scene_ids, const int32_t *sizes, int b) {
    return sizes ? sizes[b] : offsets[scene_ids[b] + 1] - offsets[scene_ids[b]];
}
// the packed row each named scene's arrays start at -- the prefix sum of the rows before it -- into start[count] (may be NULL); returns T
inline int scene_restart_starts(int count, const int32_t *offsets, const int32_t *scene_ids, const int32_t *sizes, int32_t *start) {
    int total = 0;
    for (int b = 0; b < count; b++) {
        if (start) start[b] = total;
        total += scene_restart_rows(offsets, scene_ids, sizes, b);
    }
    return total;
}
// is any scene below its capacity?  While one is, a whole-context state from outside (sca_set_state, sca_set_kd_perm, sca_step_host) is refused
inline bool scenes_any_partial(int nscenes, const int32_t *offsets, const int32_t *size) {
    for (int s = 0; s < nscenes; s++) if (size[s] != offsets[s + 1] - offsets[s]) return true;
    return false;
}
// the log's agent window lies inside the rows the scene occupies (the log's pitch stays the capacity)
inline bool scene_log_agents_ok(int size, int agent_begin, int agent_count) {
    return agent_begin >= 0 && agent_count >= 0 && (int64_t)agent_begin + agent_count <= (int64_t)size;
}
inline RestartCheck scene_restart_check(const RestartCtx &C, const RestartArgs &A) {
    if (C.nscenes <= 0 || C.offsets == nullptr) return {RESTART_NO_SCENES, -1, 0};
    if (!C.state_set) return {RESTART_NO_STATE, -1, 0};
    if (C.scene_begun) return {RESTART_MID_STEP, -1, 0};
    if (A.count <= 0 || A.scene_ids == nullptr) return {RESTART_BAD_COUNT, -1, 0};
    std::vector<uint8_t> named((std::size_t)C.nscenes, (uint8_t)0);      // one mark per scene: thousands of small scenes may be named at once
    for (int b = 0; b < A.count; b++) {
        const int s = A.scene_ids[b];
        if (s < 0 || s >= C.nscenes) return {RESTART_BAD_ID, b, 0};
        if (named[s]) return {RESTART_REPEATED_ID, b, 0};
        named[s] = 1;
        if (A.sizes && !scene_size_ok(A.sizes[b], C.offsets[s + 1] - C.offsets[s])) return {RESTART_BAD_SIZE, b, 0};
    }
    const int total = scene_restart_starts(A.count, C.offsets, A.scene_ids, A.sizes, nullptr);
    if (A.pos == nullptr || A.heading == nullptr) return {RESTART_NO_ARRAYS, -1, total};
    for (int r = 0; r < total; r++) {
        bool ok = true;
        for (int k = 0; k < 3; k++) {
            ok = ok && restart_finite(A.pos[3 * r + k]) && restart_finite(A.heading[3 * r + k]);
            if (A.vel) ok = ok && restart_finite((double)A.vel[3 * r + k]);
            if (A.goal) ok = ok && restart_finite(A.goal[3 * r + k]);
            if (A.goal_heading) ok = ok && restart_finite(A.goal_heading[3 * r + k]);
        }
        if (A.radius) ok = ok && restart_finite(A.radius[r]);
        if (A.pref_speed) ok = ok && restart_finite(A.pref_speed[r]);
        if (A.max_run_dist) ok = ok && restart_finite(A.max_run_dist[r]);
        if (!ok) return {RESTART_NOT_FINITE, r, total};
    }
    if (A.policy) for (int r = 0; r < total; r++) if (A.policy[r] > SCA_POLICY_RVO3D_DUBINS) return {RESTART_BAD_POLICY, r, total};
    for (int r = 0; r < total; r++)
        if ((A.radius && !(A.radius[r] > 0.0)) || (A.pref_speed && !(A.pref_speed[r] > 0.0)) || (A.max_run_dist && !(A.max_run_dist[r] > 0.0)))
            return {RESTART_NOT_POSITIVE, r, total};
    if (A.goal_heading && !C.tracker_on) return {RESTART_GOAL_HEADING, -1, total};
    if (C.paths_on) return {RESTART_PATHS, -1, total};
    if (A.policy && C.tracker_per_agent) {
        int r = 0;
        for (int b = 0; b < A.count; b++)
            for (int a = C.offsets[A.scene_ids[b]], end = a + scene_restart_rows(C.offsets, A.scene_ids, A.sizes, b); a < end; a++, r++)
                if (restart_policy_tracked(A.policy[r]) != restart_policy_tracked(C.policy_now[a])) return {RESTART_TRACKED_CHANGE, r, total};
    }
    return {RESTART_OK, -1, total};
}
// what sca_restart_scenes returns for a fault
inline int scene_restart_error_code(RestartFault f) {
    return f == RESTART_OK ? SCA_OK : f <= RESTART_MID_STEP ? SCA_ERR_STATE : f <= RESTART_GOAL_HEADING || f == RESTART_BAD_SIZE ? SCA_ERR_ARG : SCA_ERR_UNSUPPORTED;
}

// The page-locked staging block sca_restart_scenes copies the caller's arrays into and k_scene_restart reads across the link: one section
// per array, each sized for `cap` rows (sca_create's max_agents: T and the scene count are at most that) and aligned to 64 bytes, as the
// host state block's are (host_state_layout, sca_core.h).
enum RestartSection : int { RS_IDS = 0, RS_START, RS_POS, RS_HEADING, RS_GOAL, RS_GOAL_HEADING, RS_RADIUS, RS_PREF_SPEED, RS_MAX_RUN_DIST, RS_VEL,
                            RS_POLICY, RS_ZAXIS, RS_VPREF_MODE, RS_SECTIONS };
constexpr int64_t RS_ALIGN = 64;
struct RestartLayout { int64_t off[RS_SECTIONS]; int64_t total; };
inline int64_t restart_section_row_bytes(int s) {
    // ids / start i32 (one per named scene); pos, heading, goal, goal_heading f64 x 3; radius, pref_speed, max_run_dist f64; vel f32 x 3; the rest u8
    return s == RS_IDS || s == RS_START ? 4 : s >= RS_POS && s <= RS_GOAL_HEADING ? 24 : s >= RS_RADIUS && s <= RS_MAX_RUN_DIST ? 8 : s == RS_VEL ? 12 : 1;
}
inline RestartLayout scene_restart_layout(int cap) {
    RestartLayout L;
    int64_t at = 0;
    for (int s = 0; s < RS_SECTIONS; s++) {
        L.off[s] = at;
        at += (restart_section_row_bytes(s) * (int64_t)cap + RS_ALIGN - 1) / RS_ALIGN * RS_ALIGN;
    }
    L.total = at;
    return L;
}
// which of the optional arrays the block carries (the others keep the slot's values)
constexpr uint32_t RESTART_HAS_RADIUS = 1, RESTART_HAS_PREF_SPEED = 2, RESTART_HAS_GOAL = 4, RESTART_HAS_ZAXIS = 8, RESTART_HAS_MAX_RUN_DIST = 16,
                   RESTART_HAS_GOAL_HEADING = 32;

// ---- obstacle slots (sca_set_scene_obstacle_slots) ------------------------------------------------------------------------------------------------
// Scene s's obstacle range [cap_offsets[s], cap_offsets[s + 1]) is a CAPACITY, as its agent range is with sca_restart_scenes_sized: it holds
// counts[s] obstacles, 0 <= counts[s] <= capacity, in its first rows, and its tree -- 2 counts[s] - 1 nodes numbered from 2 * cap_offsets[s]
// -- always fits the 2 x capacity node records of the range.  The offsets obey scene_obstacles_check's rules; pos / radius are packed
// densely in scene order (sum(counts) rows).
enum ObsSlotFault {
    OBS_SLOT_OK = 0,
    OBS_SLOT_OFFSETS,       // a rule of scene_obstacles_check (its fault is reported beside this one)
    OBS_SLOT_BAD_COUNT,     // counts[s] outside 0 .. capacity (scene: s)
    OBS_SLOT_NO_ARRAYS,     // a positive sum of counts with pos == NULL or radius == NULL
    OBS_SLOT_NOT_FINITE,    // a position that is not finite (scene: its scene, row: the packed row)
    OBS_SLOT_BAD_RADIUS     // a radius that is not positive -- NaN included (scene, row as above)
};
// offsets: scene_obstacles_check's answer (SCENE_OBS_OK unless fault == OBS_SLOT_OFFSETS); total: sum(counts) where the counts passed; capacity: cap_offsets[nscenes]
struct ObsSlotCheck { ObsSlotFault fault; SceneObsFault offsets; int scene; int row; int total; int capacity; };
inline bool obs_slot_count_ok(int count, int capacity) { return count >= 0 && count <= capacity; }
// the first packed row whose position is not finite (*bad_radius = false) or whose radius is not positive (*bad_radius = true), -1: none
inline int obstacle_rows_fault(int rows, const double *pos, const double *radius, bool *bad_radius) {
    for (int r = 0; r < rows; r++) {
        if (!(restart_finite(pos[3 * r]) && restart_finite(pos[3 * r + 1]) && restart_finite(pos[3 * r + 2]))) { *bad_radius = false; return r; }
        if (!(radius[r] > 0.0) || !restart_finite(radius[r])) { *bad_radius = true; return r; }
    }
    return -1;
}
inline ObsSlotCheck obstacle_slots_check(int ctx_nscenes, int max_obstacles, int nscenes, const int32_t *cap_offsets, const int32_t *counts,
                                         const double *pos, const double *radius) {
    const SceneObsCheck o = scene_obstacles_check(ctx_nscenes, max_obstacles, nscenes, cap_offsets, true, true);
    if (o.fault != SCENE_OBS_OK) return {OBS_SLOT_OFFSETS, o.fault, o.scene, -1, 0, o.total};
    int total = 0;
    if (counts)
        for (int s = 0; s < nscenes; s++) {
            if (!obs_slot_count_ok(counts[s], cap_offsets[s + 1] - cap_offsets[s])) return {OBS_SLOT_BAD_COUNT, SCENE_OBS_OK, s, -1, 0, o.total};
            total += counts[s];                                         // (at most max_obstacles: no overflow)
        }
    if (total > 0 && !(pos && radius)) return {OBS_SLOT_NO_ARRAYS, SCENE_OBS_OK, -1, -1, total, o.total};
    bool bad_radius = false;
    const int r = total > 0 ? obstacle_rows_fault(total, pos, radius, &bad_radius) : -1;
    if (r >= 0) {
        int s = 0;
        for (int before = 0; before + counts[s] <= r; before += counts[s], s++) {}
        return {bad_radius ? OBS_SLOT_BAD_RADIUS : OBS_SLOT_NOT_FINITE, SCENE_OBS_OK, s, r, total, o.total};
    }
    return {OBS_SLOT_OK, SCENE_OBS_OK, -1, -1, total, o.total};
}
inline int obstacle_slots_error_code(ObsSlotFault f) { return f == OBS_SLOT_OK ? SCA_OK : SCA_ERR_ARG; }
// where a slot's walks start: its first node record, -1 while it is empty
inline int obstacle_slot_root(const int32_t *cap_offsets, const int32_t *counts, int s) { return counts[s] > 0 ? 2 * cap_offsets[s] : -1; }

// ---- a restart that brings obstacles (sca_restart_scenes_obstacles) -------------------------------------------------------------------------------
// obs_counts[e] for scene scene_ids[e]: -1 keeps the slot's set, 0 .. capacity replaces it; the replaced scenes' obstacles are packed in
// the order of scene_ids.  Looked at behind scene_restart_check (the ids are valid then).
enum RestartObsFault {
    RESTART_OBS_OK = 0,
    RESTART_OBS_NO_SLOTS,   // a count >= 0 while the context has no obstacle slots (entry: its index)         SCA_ERR_STATE
    RESTART_OBS_BAD_COUNT,  // a count below -1 or above the slot's capacity (entry: its index)                } SCA_ERR_ARG
    RESTART_OBS_NO_ARRAYS,  // obs_pos or obs_radius NULL with a positive total                                }
    RESTART_OBS_NOT_FINITE, // an obstacle position that is not finite (entry: the packed obstacle row)        }
    RESTART_OBS_BAD_RADIUS  // an obstacle radius that is not positive (entry: the packed obstacle row)        }
};
// total: the obstacle rows the arrays hold; replaced: the entries with a count >= 0 (RESTART_OBS_OK)
struct RestartObsCheck { RestartObsFault fault; int entry; int total; int replaced; };
inline RestartObsCheck restart_obstacles_check(bool slots_on, const int32_t *cap_offsets, int count, const int32_t *scene_ids, const int32_t *obs_counts,
                                               const double *obs_pos, const double *obs_radius) {
    if (obs_counts == nullptr) return {RESTART_OBS_OK, -1, 0, 0};
    int total = 0, replaced = 0;
    for (int e = 0; e < count; e++) {
        const int k = obs_counts[e];
        if (k < -1) return {RESTART_OBS_BAD_COUNT, e, 0, 0};
        if (k == -1) continue;
        if (!slots_on) return {RESTART_OBS_NO_SLOTS, e, 0, 0};
        if (k > cap_offsets[scene_ids[e] + 1] - cap_offsets[scene_ids[e]]) return {RESTART_OBS_BAD_COUNT, e, 0, 0};
        total += k; replaced++;
    }
    if (total > 0 && !(obs_pos && obs_radius)) return {RESTART_OBS_NO_ARRAYS, -1, total, replaced};
    bool bad_radius = false;
    const int r = total > 0 ? obstacle_rows_fault(total, obs_pos, obs_radius, &bad_radius) : -1;
    if (r >= 0) return {bad_radius ? RESTART_OBS_BAD_RADIUS : RESTART_OBS_NOT_FINITE, r, total, replaced};
    return {RESTART_OBS_OK, -1, total, replaced};
}
inline int restart_obstacles_error_code(RestartObsFault f) { return f == RESTART_OBS_OK ? SCA_OK : f == RESTART_OBS_NO_SLOTS ? SCA_ERR_STATE : SCA_ERR_ARG; }

// The obstacle sections of the restart's page-locked block, behind the agent sections and the new sizes: per named scene four words
// (count or -1, the scene's obstacle base, where its rows start in the packed sections, its new root; behind a count of -1 -- the scene
// keeps its set, and the context may have no set per scene -- the base is 0 and the kernel reads none of the three), then the packed ObsRec rows, the
// sorted rows, the permutation with global ids, and the KdNode / KdWide records -- two per obstacle row, a tree over k rows at records
// [2 * start, 2 * start + 2k - 1).  Every section starts on a 64-byte boundary and every record is a multiple of 16 bytes, so a record is
// read as whole 16-byte pieces; the sizes depend on sca_create's max_agents (at most that many scenes) and max_obstacles alone.
enum RestartObsSection : int { RO_HEAD = 0, RO_REC, RO_SORTED, RO_PERM, RO_TREE, RO_WIDE, RO_SECTIONS };
constexpr int RO_HEAD_WORDS = 4;            // count, base, start, root
constexpr int64_t RO_REC_BYTES = 32, RO_TREE_BYTES = 64, RO_WIDE_BYTES = 128;
struct RestartObsLayout { int64_t off[RO_SECTIONS]; int64_t total; };
inline int64_t restart_obs_section_bytes(int s, int max_n, int max_obstacles) {
    return s == RO_HEAD ? 4 * RO_HEAD_WORDS * (int64_t)max_n : s == RO_REC || s == RO_SORTED ? RO_REC_BYTES * max_obstacles : s == RO_PERM ? 4 * (int64_t)max_obstacles
           : (s == RO_TREE ? RO_TREE_BYTES : RO_WIDE_BYTES) * 2 * (int64_t)max_obstacles;
}
// begin: where the sections start in the block (a multiple of RS_ALIGN is kept one)
inline RestartObsLayout restart_obstacles_layout(int64_t begin, int max_n, int max_obstacles) {
    RestartObsLayout L;
    int64_t at = (begin + RS_ALIGN - 1) / RS_ALIGN * RS_ALIGN;
    for (int s = 0; s < RO_SECTIONS; s++) {
        L.off[s] = at;
        at += (restart_obs_section_bytes(s, max_n, max_obstacles) + RS_ALIGN - 1) / RS_ALIGN * RS_ALIGN;
    }
    L.total = at;
    return L;
}

// ---- a restart that brings attributes (sca_restart_scenes_attrs) ------------------------------------------------------------------------------------
// The named scenes' occupied rows take the episode's solver attributes (sca_set_agent_params') and planner attributes
// (sca_device_tracker_set_agent_params').  Looked at behind scene_restart_check and restart_obstacles_check (ids, sizes and policies are
// valid then).  A NULL array means the value a context alone would have -- sca_params', the enable call's -- never "what the row had".
enum RestartAttrFault {
    RESTART_ATTR_OK = 0,
    RESTART_ATTR_STRUCT,    // struct_bytes below the leading integers, above the library's struct, or cutting a pointer in two    } SCA_ERR_ARG
    RESTART_ATTR_RESERVED,  // reserved != 0                                                                                        }
    RESTART_ATTR_NO_TRACKER,// turning_radius / pitch_lo / pitch_hi given while no device tracker is enabled                       }
    RESTART_ATTR_SOLVER,    // a solver attribute out of sca_set_agent_params' range (entry: the packed row)                       }
    RESTART_ATTR_PLANNER    // a tracked row whose turning radius / pitch limits are out of range (entry: the packed row)          }
};
// the descriptor as the library reads it: every member the caller's struct_bytes does not reach is NULL
struct RestartAttrs {
    const double *neighbor_dist = nullptr; const int32_t *max_neighbors = nullptr;
    const double *time_step = nullptr, *time_horizon = nullptr, *max_speed = nullptr, *max_heading_change = nullptr, *dt_nominal = nullptr;
    const double *turning_radius = nullptr, *pitch_lo = nullptr, *pitch_hi = nullptr;
    bool solver() const { return neighbor_dist || max_neighbors || time_step || time_horizon || max_speed || max_heading_change || dt_nominal; }
    bool planner() const { return turning_radius || pitch_lo || pitch_hi; }
};
// what a NULL array stands for: sca_create's sca_params and sca_device_tracker_enable's values
struct AttrDefaults {
    double neighbor_dist, time_step, time_horizon, max_speed, max_heading_change, dt_nominal; int max_neighbors;
    double turning_radius, pitch_lo, pitch_hi;
};
struct RestartAttrCheck { RestartAttrFault fault; int entry; };
constexpr int RESTART_ATTR_HEAD_BYTES = 8;                              // struct_bytes, reserved
inline bool restart_attr_positive(double x) { return restart_finite(x) && x > 0.0; }
// one row's solver attributes by sca_set_agent_params' rule
inline bool restart_attr_solver_ok(double nd, int mn, double ts, double th, double ms, double mhc, double dt) {
    return restart_attr_positive(nd) && restart_attr_positive(ts) && restart_attr_positive(th) && restart_attr_positive(ms) && restart_attr_positive(dt) &&
           mn >= 1 && mn <= SCA_MAX_NEIGHBORS && mhc >= 0.0 && mhc <= 3.14159265358979323846;
}
// one tracked row's planner attributes by sca_device_tracker_set_agent_params' rule
inline bool restart_attr_planner_ok(double R, double lo, double hi) { return restart_attr_positive(R) && restart_finite(lo) && restart_finite(hi) && lo < hi; }
// in: the caller's struct (not NULL); out: its members as far as struct_bytes reaches.  C, A: what scene_restart_check passed.
inline RestartAttrCheck restart_attrs_check(const RestartCtx &C, const RestartArgs &A, const sca_restart_attrs *in, const AttrDefaults &D, RestartAttrs *out) {
    const int sb = in->struct_bytes;
    if (sb < RESTART_ATTR_HEAD_BYTES || sb > (int)sizeof(sca_restart_attrs) || (sb - RESTART_ATTR_HEAD_BYTES) % (int)sizeof(void *) != 0) return {RESTART_ATTR_STRUCT, -1};
    if (in->reserved != 0) return {RESTART_ATTR_RESERVED, -1};
    sca_restart_attrs full{};                                          // (members behind struct_bytes stay NULL)
    char *to = (char *)&full;
    const char *from = (const char *)in;
    for (int i = 0; i < sb; i++) to[i] = from[i];
    RestartAttrs R;
    R.neighbor_dist = full.neighbor_dist; R.max_neighbors = full.max_neighbors; R.time_step = full.time_step; R.time_horizon = full.time_horizon;
    R.max_speed = full.max_speed; R.max_heading_change = full.max_heading_change; R.dt_nominal = full.dt_nominal;
    R.turning_radius = full.turning_radius; R.pitch_lo = full.pitch_lo; R.pitch_hi = full.pitch_hi;
    if (R.planner() && !C.tracker_on) return {RESTART_ATTR_NO_TRACKER, -1};
    const int total = scene_restart_starts(A.count, C.offsets, A.scene_ids, A.sizes, nullptr);
    if (R.solver())
        for (int r = 0; r < total; r++)
            if (!restart_attr_solver_ok(R.neighbor_dist ? R.neighbor_dist[r] : D.neighbor_dist, R.max_neighbors ? R.max_neighbors[r] : D.max_neighbors,
                                        R.time_step ? R.time_step[r] : D.time_step, R.time_horizon ? R.time_horizon[r] : D.time_horizon,
                                        R.max_speed ? R.max_speed[r] : D.max_speed, R.max_heading_change ? R.max_heading_change[r] : D.max_heading_change,
                                        R.dt_nominal ? R.dt_nominal[r] : D.dt_nominal))
                return {RESTART_ATTR_SOLVER, r};
    if (R.planner()) {
        int r = 0;
        for (int b = 0; b < A.count; b++)
            for (int a = C.offsets[A.scene_ids[b]], end = a + scene_restart_rows(C.offsets, A.scene_ids, A.sizes, b); a < end; a++, r++) {
                if (!restart_policy_tracked(A.policy ? A.policy[r] : C.policy_now[a])) continue;          // untracked rows' entries are ignored
                if (!restart_attr_planner_ok(R.turning_radius ? R.turning_radius[r] : D.turning_radius, R.pitch_lo ? R.pitch_lo[r] : D.pitch_lo,
                                             R.pitch_hi ? R.pitch_hi[r] : D.pitch_hi))
                    return {RESTART_ATTR_PLANNER, r};
            }
    }
    *out = R;
    return {RESTART_ATTR_OK, -1};
}
inline int restart_attrs_error_code(RestartAttrFault f) { return f == RESTART_ATTR_OK ? SCA_OK : SCA_ERR_ARG; }

// The attribute sections of the restart's page-locked block, behind the obstacle sections: per packed row one AgentPar record (64 bytes,
// read as four 16-byte pieces), the row's neighborDist alone (the tracker's array), the planner triple (turning radius, pitch_lo,
// pitch_hi) and the row's class byte.  Every section starts on a 64-byte boundary; the sizes depend on sca_create's max_agents alone.
enum RestartAttrSection : int { RA_PAR = 0, RA_ND, RA_TRIPLE, RA_CLASS, RA_SECTIONS };
constexpr int64_t RA_PAR_BYTES = 64;
struct RestartAttrLayout { int64_t off[RA_SECTIONS]; int64_t total; };
inline int64_t restart_attr_row_bytes(int s) { return s == RA_PAR ? RA_PAR_BYTES : s == RA_ND ? 8 : s == RA_TRIPLE ? 24 : 1; }
// begin: where the sections start in the block (RestartObsLayout::total)
inline RestartAttrLayout restart_attrs_layout(int64_t begin, int max_n) {
    RestartAttrLayout L;
    int64_t at = (begin + RS_ALIGN - 1) / RS_ALIGN * RS_ALIGN;
    for (int s = 0; s < RA_SECTIONS; s++) {
        L.off[s] = at;
        at += (restart_attr_row_bytes(s) * (int64_t)max_n + RS_ALIGN - 1) / RS_ALIGN * RS_ALIGN;
    }
    L.total = at;
    return L;
}
// the attribute sections travel / the planner sections travel (the others keep the slot's values: every call without `attrs`)
constexpr uint32_t RESTART_HAS_ATTRS = 64, RESTART_HAS_PLANNER = 128;

// The tracker's classes under restarts.  The re-plan kernels run once per class of equal (turning radius, pitch_lo, pitch_hi) with the
// class's values as kernel arguments, and an agent's class byte says which launch plans it (sca_device_tracker_set_agent_params).  A
// restart changes which triples are in use, so the table is recomputed after every call over the OCCUPIED TRACKED rows -- rows behind a
// scene's size and rows of untracked policies are not counted -- and a class keeps its index while any such row uses it: the class bytes
// of the scenes that were not named need not move.  More than TRK_CLASS_CAP distinct triples: the per-agent form (`many`), which reads
// the per-row arrays and no class byte; back at or below the cap the table is dealt afresh.
constexpr int TRK_CLASS_CAP = 16;
struct TrackTriple { double R, lo, hi; };
inline bool operator==(const TrackTriple &a, const TrackTriple &b) { return a.R == b.R && a.lo == b.lo && a.hi == b.hi; }
struct ClassTable {
    TrackTriple val[TRK_CLASS_CAP] = {};
    int32_t users[TRK_CLASS_CAP] = {};     // occupied tracked rows of the class; 0: the index is free
    bool many = false;
};
// classes: distinct triples in use (TRK_CLASS_CAP + 1: more than the cap); moved: a class byte changed in a row whose byte does not
// travel with the call (the caller uploads the whole array then)
struct ClassUpdate { int classes; bool many; bool moved; };
// policy, trip: [n] as they will be after the restart; size: [nscenes] likewise; cls: [n] the class bytes, rewritten for the occupied
// tracked rows (untouched while `many`); travels: [n] 1 for the rows whose byte the restart's block carries, or NULL: none does
inline ClassUpdate scene_class_table(ClassTable &tab, int nscenes, const int32_t *offsets, const int32_t *size, const uint8_t *policy, const TrackTriple *trip,
                                     uint8_t *cls, const uint8_t *travels) {
    TrackTriple seen[TRK_CLASS_CAP];
    int nseen = 0;
    bool many = false;
    for (int s = 0; s < nscenes && !many; s++)
        for (int a = offsets[s]; a < offsets[s] + size[s]; a++) {
            if (!restart_policy_tracked(policy[a])) continue;
            int k = 0;
            while (k < nseen && !(seen[k] == trip[a])) k++;
            if (k < nseen) continue;
            if (nseen == TRK_CLASS_CAP) { many = true; break; }
            seen[nseen++] = trip[a];
        }
    if (many) {
        for (int k = 0; k < TRK_CLASS_CAP; k++) tab.users[k] = 0;
        tab.many = true;
        return {TRK_CLASS_CAP + 1, true, false};
    }
    bool keep[TRK_CLASS_CAP], placed[TRK_CLASS_CAP];
    for (int k = 0; k < TRK_CLASS_CAP; k++) {                          // an index stays its class's while a row still uses the class
        keep[k] = false;
        if (tab.many || tab.users[k] == 0) continue;
        for (int j = 0; j < nseen; j++) if (seen[j] == tab.val[k]) keep[k] = true;
    }
    for (int j = 0; j < nseen; j++) {
        placed[j] = false;
        for (int k = 0; k < TRK_CLASS_CAP; k++) if (keep[k] && tab.val[k] == seen[j]) placed[j] = true;
    }
    for (int j = 0, k = 0; j < nseen; j++) {                           // new triples take the lowest free indices, in order of appearance
        if (placed[j]) continue;
        while (keep[k]) k++;
        tab.val[k] = seen[j]; keep[k] = true;
    }
    for (int k = 0; k < TRK_CLASS_CAP; k++) tab.users[k] = 0;
    tab.many = false;
    bool moved = false;
    for (int s = 0; s < nscenes; s++)
        for (int a = offsets[s]; a < offsets[s] + size[s]; a++) {
            if (!restart_policy_tracked(policy[a])) continue;
            int k = 0;
            while (!(keep[k] && tab.val[k] == trip[a])) k++;
            tab.users[k]++;
            if (cls[a] != (uint8_t)k) { cls[a] = (uint8_t)k; if (!travels || !travels[a]) moved = true; }
        }
    return {nseen, false, moved};
}
// the classes in use, and the one index in use where there is exactly one (-1 otherwise)
inline int class_table_used(const ClassTable &tab, int *only) {
    int used = 0, last = -1;
    for (int k = 0; k < TRK_CLASS_CAP; k++) if (tab.users[k] > 0) { used++; last = k; }
    if (only) *only = used == 1 ? last : -1;
    return used;
}

// ---- waypoint lists in slot form (sca_set_path_slots) and a restart that brings lists (sca_restart_scenes_paths) -----------------------------------
// In slot form every agent row owns room for W waypoints: row a's list is pts[3 * (W * a + j)], j < len[a] <= W.  A row's list has a place
// that depends on nothing else, so a restart writes the rows of a scene independently and nothing is compacted; an episode fits a slot if
// its longest list is at most W.  The price is 24 * W bytes per agent row.
// the first point of row a's room, in points from the allocation's start.  The kernels that read and write and the host that uploads call this.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int64_t path_slot_index(int W, int a) { return (int64_t)W * (int64_t)a; }
// W * max_agents points must stay addressable: every coordinate index 3 * (W * a + j) below 2^31
constexpr int64_t PATH_SLOT_POINTS_MAX = INT32_MAX / 3;
inline bool path_slots_addressable(int W, int max_agents) { return (int64_t)W * (int64_t)max_agents <= PATH_SLOT_POINTS_MAX; }

enum PathSlotFault {
    PATH_SLOTS_OK = 0,
    PATH_SLOTS_NO_AGENTS,   // before sca_set_agents                                                            SCA_ERR_STATE
    PATH_SLOTS_PARTITION,   // under the cell-owner partition: path state does not migrate with the agents     SCA_ERR_UNSUPPORTED
    PATH_SLOTS_BAD_N,       // n is not the context's agent count                                              } SCA_ERR_ARG
    PATH_SLOTS_BAD_W,       // points_per_agent < 1                                                            }
    PATH_SLOTS_TOO_LARGE,   // points_per_agent * max_agents is not addressable                                }
    PATH_SLOTS_BAD_START,   // offsets[0] != 0                                                                 }
    PATH_SLOTS_DECREASING,  // offsets decrease (entry: the agent)                                             }
    PATH_SLOTS_TOO_LONG,    // a list longer than points_per_agent (entry: the agent)                          }
    PATH_SLOTS_NO_POINTS,   // points NULL with points to read                                                 }
    PATH_SLOTS_NOT_FINITE   // a point that is not finite (entry: the point)                                   }
};
// total: offsets[n] (0 with offsets == NULL: every list empty), from PATH_SLOTS_NO_POINTS on
struct PathSlotCheck { PathSlotFault fault; int entry; int total; };
inline PathSlotCheck path_slots_check(bool agents_set, bool partition_on, int ctx_n, int max_agents, int W, int n, const int32_t *offsets, const double *points) {
    if (!agents_set) return {PATH_SLOTS_NO_AGENTS, -1, 0};
    if (partition_on) return {PATH_SLOTS_PARTITION, -1, 0};
    if (n != ctx_n) return {PATH_SLOTS_BAD_N, -1, 0};
    if (W < 1) return {PATH_SLOTS_BAD_W, -1, 0};
    if (!path_slots_addressable(W, max_agents)) return {PATH_SLOTS_TOO_LARGE, -1, 0};
    if (offsets == nullptr) return {PATH_SLOTS_OK, -1, 0};
    if (offsets[0] != 0) return {PATH_SLOTS_BAD_START, 0, 0};
    for (int i = 0; i < n; i++) {
        if (offsets[i + 1] < offsets[i]) return {PATH_SLOTS_DECREASING, i, 0};
        if (offsets[i + 1] - offsets[i] > W) return {PATH_SLOTS_TOO_LONG, i, 0};
    }
    const int total = offsets[n];                                       // (at most W * n: addressable)
    if (total > 0 && points == nullptr) return {PATH_SLOTS_NO_POINTS, -1, total};
    for (int k = 0; k < total; k++)
        if (!(restart_finite(points[3 * (int64_t)k]) && restart_finite(points[3 * (int64_t)k + 1]) && restart_finite(points[3 * (int64_t)k + 2])))
            return {PATH_SLOTS_NOT_FINITE, k, total};
    return {PATH_SLOTS_OK, -1, total};
}
inline int path_slots_error_code(PathSlotFault f) {
    return f == PATH_SLOTS_OK ? SCA_OK : f == PATH_SLOTS_NO_AGENTS ? SCA_ERR_STATE : f == PATH_SLOTS_PARTITION ? SCA_ERR_UNSUPPORTED : SCA_ERR_ARG;
}

// the block-form refusal (RESTART_PATHS) stands while the lists are one CSR block; in slot form a restart is accepted -- what
// scene_restart_check is told for RestartCtx::paths_on
inline bool restart_refuses_paths(bool paths_on, bool slot_form) { return paths_on && !slot_form; }

// path_offsets: CSR over the call's T packed rows, packed like pos; NULL: the call brings no lists (in slot form the named rows then get
// empty ones).  Looked at behind scene_restart_check (T is known then).
enum RestartPathFault {
    RESTART_PATHS_OK = 0,
    RESTART_PATHS_NO_SLOTS,   // path arrays while the context is not in slot form                              SCA_ERR_STATE
    RESTART_PATHS_BAD_START,  // path_offsets[0] != 0                                                           } SCA_ERR_ARG
    RESTART_PATHS_DECREASING, // offsets decrease (entry: the packed row)                                       }
    RESTART_PATHS_TOO_LONG,   // a row's list longer than W (entry: the packed row)                             }
    RESTART_PATHS_NO_POINTS,  // path_points NULL with points to read                                           }
    RESTART_PATHS_NOT_FINITE  // a point that is not finite (entry: the packed row whose list holds it)         }
};
// total: path_offsets[T], the points the call brings (RESTART_PATHS_OK and the faults found after the offsets)
struct RestartPathCheck { RestartPathFault fault; int entry; int total; };
inline RestartPathCheck restart_paths_check(bool slot_form, int W, int T, const int32_t *path_offsets, const double *path_points) {
    if (path_offsets == nullptr) return {RESTART_PATHS_OK, -1, 0};
    if (!slot_form) return {RESTART_PATHS_NO_SLOTS, -1, 0};
    if (path_offsets[0] != 0) return {RESTART_PATHS_BAD_START, 0, 0};
    for (int r = 0; r < T; r++) {
        if (path_offsets[r + 1] < path_offsets[r]) return {RESTART_PATHS_DECREASING, r, 0};
        if (path_offsets[r + 1] - path_offsets[r] > W) return {RESTART_PATHS_TOO_LONG, r, 0};
    }
    const int total = path_offsets[T];
    if (total > 0 && path_points == nullptr) return {RESTART_PATHS_NO_POINTS, -1, total};
    for (int r = 0; r < T; r++)
        for (int64_t k = 3 * (int64_t)path_offsets[r]; k < 3 * (int64_t)path_offsets[r + 1]; k++)
            if (!restart_finite(path_points[k])) return {RESTART_PATHS_NOT_FINITE, r, total};
    return {RESTART_PATHS_OK, -1, total};
}
inline int restart_paths_error_code(RestartPathFault f) { return f == RESTART_PATHS_OK ? SCA_OK : f == RESTART_PATHS_NO_SLOTS ? SCA_ERR_STATE : SCA_ERR_ARG; }

// The path sections of the restart's page-locked block, behind the attribute sections: the CSR offsets over the call's packed rows
// (T + 1 <= max_n + 1 words) and the points actually present, packed -- not padded to W; room for the most a call can bring, W per row.
// Every section starts on a 64-byte boundary.  W == 0 (the context is not in slot form): no room, and the kernel reads neither.
enum RestartPathSection : int { RP_OFF = 0, RP_PTS, RP_SECTIONS };
struct RestartPathLayout { int64_t off[RP_SECTIONS]; int64_t total; };
inline int64_t restart_path_section_bytes(int s, int max_n, int W) {
    return W <= 0 ? 0 : s == RP_OFF ? 4 * ((int64_t)max_n + 1) : 24 * (int64_t)W * (int64_t)max_n;
}
// begin: where the sections start in the block (RestartAttrLayout::total)
inline RestartPathLayout restart_paths_layout(int64_t begin, int max_n, int W) {
    RestartPathLayout L;
    int64_t at = (begin + RS_ALIGN - 1) / RS_ALIGN * RS_ALIGN;
    for (int s = 0; s < RP_SECTIONS; s++) {
        L.off[s] = at;
        at += (restart_path_section_bytes(s, max_n, W) + RS_ALIGN - 1) / RS_ALIGN * RS_ALIGN;
    }
    L.total = at;
    return L;
}
// the rows' lists are written (slot form): from the block's path sections, or empty where the call brought none
constexpr uint32_t RESTART_HAS_PATH_SLOTS = 256, RESTART_HAS_PATHS = 512;

// The whole staging block: the agent sections, behind them the named scenes' new sizes (one int32 per named scene, at most max_n of them),
// then the obstacle, attribute and path sections.  The ONE place that knows the order of the parts: sca_restart_scenes allocates `total`
// bytes and launches with the members, the harnesses walk the same value.
struct RestartBlock { RestartLayout L; int64_t new_size_off; RestartObsLayout OL; RestartAttrLayout AL; RestartPathLayout PL; int64_t total; };
inline RestartBlock restart_block_layout(int max_n, int max_m, int W) {
    RestartBlock B;
    B.L = scene_restart_layout(max_n);
    B.new_size_off = B.L.total;
    B.OL = restart_obstacles_layout(B.new_size_off + (int64_t)sizeof(int32_t) * (int64_t)max_n, max_n, max_m);
    B.AL = restart_attrs_layout(B.OL.total, max_n);
    B.PL = restart_paths_layout(B.AL.total, max_n, W);
    B.total = B.PL.total;
    return B;
}

// ---- scene checkpoints (sca_save_scenes / sca_load_scenes) ------------------------------------------------------------------------------------------
// A scene's whole MUTABLE state as one blob of bytes: what scene_restart_fill / scene_restart_paths reset plus what PartMig carries
// (sca_partition.hip.h), for the rows the scene occupies.  The episode's definition (constants, attributes, obstacles, waypoint lists, goal
// headings) is not in it: a resume is a restart with the definition, then a load.  The blob is pointer-free and speaks scene-local terms
// (the permutation 0 .. size - 1), so it loads into any slot of any context.  Layout: a fixed header, then the sections in the order of
// CkptSection, each on a 16-byte boundary; a section the blob does not carry (tracker, cursors) has length 0.  Everything per row is whole
// 4-byte words -- the records 16-byte pieces -- so k_scene_save / k_scene_load (sca_scenes.hip.h) move a section as consecutive words by
// consecutive lanes; the one byte-sized column, vpref_mode, travels as a word per row for that reason.
constexpr uint32_t CKPT_MAGIC = 0x504b4353u;       // "SCKP"
constexpr int32_t CKPT_FORMAT = 1;
constexpr int32_t CKPT_LIB_VERSION = 103;          // sca_version() (sca_hip.hip asserts it)
constexpr int64_t CKPT_ALIGN = 16;
constexpr int32_t CKPT_REC_BYTES = 48;             // sizeof(PubRec): px py pz f64, vx vy vz f32, flags u32, radius f64
constexpr int32_t CKPT_COUNT_MAX = 1 << 20;        // bound of AgentTrack's sample count / cursor: compute_sampling yields about a thousand samples (finish_plan)
struct CkptHeader {                                // 64 bytes
    uint32_t magic; int32_t format, lib_version, size;
    int32_t trk_words, rec_bytes, has_track, has_paths;
    int32_t steps, live, prev, reserved;
    int64_t total_bytes;                           // header + sections
    uint64_t checksum;                             // scene_checkpoint_sum over the bytes behind the header
};
static_assert(sizeof(CkptHeader) == 64, "the checkpoint's header is 64 bytes");
enum CkptSection : int { CK_POLICY = 0,            // [size] u8: the rows' policies, which the loading scene must have (written by the host)
                         CK_REC, CK_HEADING, CK_HEADING_KEEP, CK_VPREF_EXT, CK_TOTAL_DIST, CK_STEP_NUM, CK_STATUS, CK_PERM, CK_VPREF_MODE,
                         CK_TRK_NBR0, CK_TRACK,    // with the tracker's records
                         CK_REM, CK_NOW_GOAL,      // with the waypoint cursors
                         CK_SECTIONS };
struct CkptLayout { int64_t off[CK_SECTIONS]; int64_t len[CK_SECTIONS]; int64_t total; };
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int64_t ckpt_section_row_bytes(int s, int trk_words, int has_paths) {
    return s == CK_POLICY ? 1 : s == CK_REC ? CKPT_REC_BYTES : s == CK_HEADING || s == CK_HEADING_KEEP || s == CK_VPREF_EXT ? 24
           : s == CK_TOTAL_DIST ? 8 : s == CK_STEP_NUM || s == CK_STATUS || s == CK_PERM || s == CK_VPREF_MODE ? 4
           : s == CK_TRK_NBR0 ? (trk_words > 0 ? 8 : 0) : s == CK_TRACK ? (trk_words > 0 ? 4 * (int64_t)trk_words : 0)
           : s == CK_REM ? (has_paths ? 4 : 0) : (has_paths ? 24 : 0);
}
// a pure function of (size, trk_words, has_paths): the kernels and the host both call it
#if defined(__HIPCC__)
__host__ __device__
#endif
inline CkptLayout scene_checkpoint_layout(int size, int trk_words, int has_paths) {
    CkptLayout L;
    int64_t at = (int64_t)sizeof(CkptHeader);
    for (int s = 0; s < CK_SECTIONS; s++) {
        L.off[s] = at;
        L.len[s] = ckpt_section_row_bytes(s, trk_words, has_paths) * (int64_t)size;
        at += (L.len[s] + CKPT_ALIGN - 1) / CKPT_ALIGN * CKPT_ALIGN;
    }
    L.total = at;
    return L;
}
// FNV-1a over 64-bit words (every blob is a whole number of them): any one changed byte changes the sum
inline uint64_t scene_checkpoint_sum(const void *bytes, int64_t count) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char *p = (const unsigned char *)bytes;
    for (int64_t i = 0; i + 8 <= count; i += 8) {
        uint64_t w = 0;
        for (int k = 0; k < 8; k++) w |= (uint64_t)p[i + k] << (8 * k);
        h = (h ^ w) * 0x100000001b3ull;
    }
    return h;
}
// where the integers of one AgentTrack record (sca_dubins.hpp) stand, in bytes from the record's start: the ones a kernel uses as a
// cursor, a count or a switch.  Filled with offsetof where the type is known (sca_hip.hip, tests/scene_checkpoint_harness.cpp).
struct CkptTrackFields {
    int words;                                     // sizeof(AgentTrack) / 4
    int use_dubins, plan_ok, h_ok, v_ok;           // bool bytes
    int h_mode, v_mode, plan_mode;                 // char[3], char[3], char[7]: Dubins words, 'L' 'S' 'R' or 0
    int iters, rounds, replans;                    // int32
    int count, next;                               // int64 (long)
};
enum CkptFault {
    CKPT_OK = 0,
    CKPT_SHORT,             // fewer bytes than a header, or a NULL blob                              } the envelope: SCA_ERR_ARG
    CKPT_MAGIC_BAD,         // not a checkpoint                                                       }
    CKPT_FORMAT_BAD,        // another format version                                                 }
    CKPT_RECORD,            // trk_words or the record size are not this library's                    }
    CKPT_SIZE_RANGE,        // size outside 1 .. KD_WAVE_CAP, or flag words that are not 0 / 1        }
    CKPT_BYTES,             // the byte count is not the layout's                                     }
    CKPT_CHECKSUM,          // the payload's sum is not the header's                                  }
    CKPT_SCENE_SIZE,        // size is not the scene's current size                                   } against the scene: SCA_ERR_ARG
    CKPT_POLICY,            // a row's policy byte differs from the scene's (entry: the row)          }
    CKPT_TRACKER,           // tracker records present / absent against what the scene needs here     }
    CKPT_NO_LISTS,          // a cursor with rem > 0 while no lists are set (entry: the row)          }
    CKPT_REM_RANGE,         // rem[i] outside 0 .. the row's list length as set (entry: the row)      }
    CKPT_PERM,              // the permutation is not one of 0 .. size - 1 (entry: the position)      } the payload: SCA_ERR_ARG
    CKPT_FLAGS,             // unknown flag bits, or a vpref_mode other than 0 / 1 (entry: the row)   }
    CKPT_NOT_FINITE,        // a position that is not finite, a radius that is not positive (entry: the row) }
    CKPT_COUNTERS,          // steps / live / prev out of range, or live is not the rows without flags }
    CKPT_TRACK_RANGE        // an AgentTrack integer outside its range (entry: the row)               }
};
struct CkptCheck { CkptFault fault; int entry; };
// what the rules read of the loading scene; NULL: the envelope and the payload alone (sca_scene_checkpoint_info)
struct CkptScene {
    int size;                                      // the rows the scene occupies now
    const uint8_t *policy;                         // [size] their policies
    bool tracker_on;                               // the context's device tracker
    bool paths_on;                                 // waypoint lists are set
    const int32_t *path_len;                       // [size] the rows' list lengths as set (paths_on)
};
inline int64_t ckpt_i64(const unsigned char *p) { int64_t v; unsigned char *q = (unsigned char *)&v; for (int k = 0; k < 8; k++) q[k] = p[k]; return v; }
inline int32_t ckpt_i32(const unsigned char *p) { int32_t v; unsigned char *q = (unsigned char *)&v; for (int k = 0; k < 4; k++) q[k] = p[k]; return v; }
inline double ckpt_f64(const unsigned char *p) { double v; unsigned char *q = (unsigned char *)&v; for (int k = 0; k < 8; k++) q[k] = p[k]; return v; }
inline bool ckpt_word_ok(const unsigned char *m, int n) { for (int k = 0; k < n; k++) if (m[k] != 0 && m[k] != 'L' && m[k] != 'S' && m[k] != 'R') return false; return true; }
// THE check of a blob, whole: envelope, then the blob against the scene, then every payload value a kernel would use as an index, a count
// or a switch.  Reads bytes [0, bytes) of `blob` and nothing else; head (nullable) receives the header once the envelope holds.
inline CkptCheck scene_checkpoint_check(const void *blob, int64_t bytes, const CkptTrackFields &F, const CkptScene *scene, CkptHeader *head) {
    if (blob == nullptr || bytes < (int64_t)sizeof(CkptHeader)) return {CKPT_SHORT, -1};
    const unsigned char *b = (const unsigned char *)blob;
    CkptHeader H;
    { unsigned char *q = (unsigned char *)&H; for (std::size_t k = 0; k < sizeof(CkptHeader); k++) q[k] = b[k]; }
    if (H.magic != CKPT_MAGIC) return {CKPT_MAGIC_BAD, -1};
    if (H.format != CKPT_FORMAT) return {CKPT_FORMAT_BAD, -1};
    if (H.rec_bytes != CKPT_REC_BYTES || (H.trk_words != 0 && H.trk_words != F.words)) return {CKPT_RECORD, -1};
    if (H.size < 1 || H.size > KD_WAVE_CAP || (H.has_track != 0 && H.has_track != 1) || (H.has_paths != 0 && H.has_paths != 1) || (H.has_track != 0) != (H.trk_words != 0))
        return {CKPT_SIZE_RANGE, -1};
    const CkptLayout L = scene_checkpoint_layout(H.size, H.trk_words, H.has_paths);
    if (H.total_bytes != L.total || bytes != L.total) return {CKPT_BYTES, -1};
    if (scene_checkpoint_sum(b + sizeof(CkptHeader), L.total - (int64_t)sizeof(CkptHeader)) != H.checksum) return {CKPT_CHECKSUM, -1};
    if (head) *head = H;
    const int N = H.size;
    const unsigned char *pol = b + L.off[CK_POLICY];
    if (scene) {
        if (scene->size != N) return {CKPT_SCENE_SIZE, -1};
        bool tracked = false;
        for (int i = 0; i < N; i++) {
            if (pol[i] != scene->policy[i]) return {CKPT_POLICY, i};
            tracked = tracked || restart_policy_tracked(pol[i]);
        }
        if ((scene->tracker_on && tracked) != (H.has_track != 0)) return {CKPT_TRACKER, -1};
        for (int i = 0; i < N; i++) {
            const int rem = H.has_paths ? ckpt_i32(b + L.off[CK_REM] + 4 * (int64_t)i) : 0;
            const int len = scene->paths_on ? scene->path_len[i] : 0;
            if (!scene->paths_on && rem > 0) return {CKPT_NO_LISTS, i};
            if (H.has_paths ? (rem < 0 || rem > len) : len > 0) return {CKPT_REM_RANGE, i};
        }
    }
    for (int i = 0; i < N; i++) if (pol[i] > SCA_POLICY_RVO3D_DUBINS) return {CKPT_POLICY, i};
    {
        std::vector<uint8_t> seen((std::size_t)N, (uint8_t)0);
        for (int p = 0; p < N; p++) {
            const int32_t a = ckpt_i32(b + L.off[CK_PERM] + 4 * (int64_t)p);
            if (a < 0 || a >= N || seen[(std::size_t)a]) return {CKPT_PERM, p};
            seen[(std::size_t)a] = 1;
        }
    }
    int running = 0;
    for (int i = 0; i < N; i++) {
        const unsigned char *r = b + L.off[CK_REC] + (int64_t)CKPT_REC_BYTES * i;
        const uint32_t flags = (uint32_t)ckpt_i32(r + 36);
        const uint32_t mode = (uint32_t)ckpt_i32(b + L.off[CK_VPREF_MODE] + 4 * (int64_t)i);
        if ((flags & ~7u) != 0 || mode > 1u) return {CKPT_FLAGS, i};
        running += (flags & 7u) ? 0 : 1;
        bool ok = true;
        for (int k = 0; k < 3; k++) ok = ok && restart_finite(ckpt_f64(r + 8 * k));
        const double radius = ckpt_f64(r + 40);
        ok = ok && restart_finite(radius) && radius > 0.0;                // (feeds the conservative reach filters, like a restart's radius)
        if (!ok) return {CKPT_NOT_FINITE, i};
        if (ckpt_i32(b + L.off[CK_STEP_NUM] + 4 * (int64_t)i) < 0) return {CKPT_COUNTERS, i};
    }
    if (H.steps < 0 || H.prev < 0 || H.prev > N || H.live != running) return {CKPT_COUNTERS, -1};
    if (H.has_track)
        for (int i = 0; i < N; i++) {
            const unsigned char *t = b + L.off[CK_TRACK] + 4 * (int64_t)F.words * i;
            const int64_t count = ckpt_i64(t + F.count), next = ckpt_i64(t + F.next);
            const bool ok = t[F.use_dubins] <= 1 && t[F.plan_ok] <= 1 && t[F.h_ok] <= 1 && t[F.v_ok] <= 1 && ckpt_word_ok(t + F.h_mode, 3) && ckpt_word_ok(t + F.v_mode, 3) &&
                            ckpt_word_ok(t + F.plan_mode, 7) && ckpt_i32(t + F.iters) >= 0 && ckpt_i32(t + F.rounds) >= 0 && ckpt_i32(t + F.replans) >= 0 &&
                            count >= 0 && count <= CKPT_COUNT_MAX && next >= 0 && next <= count;
            if (!ok) return {CKPT_TRACK_RANGE, i};
        }
    return {CKPT_OK, -1};
}
inline int scene_checkpoint_error_code(CkptFault f) { return f == CKPT_OK ? SCA_OK : SCA_ERR_ARG; }

// the call's own rules, for both entry points (op: 0 save, 1 load; bufs / sizes: the callers' arrays)
enum CkptCallFault {
    CKPT_CALL_OK = 0,
    CKPT_CALL_NO_SCENES,    // the context holds no scenes                                            } SCA_ERR_STATE
    CKPT_CALL_NO_STATE,     // no state yet                                                           }
    CKPT_CALL_MID_STEP,     // between a policy pass and its env update                               }
    CKPT_CALL_BAD_COUNT,    // count <= 0 or a NULL array                                             } SCA_ERR_ARG
    CKPT_CALL_BAD_ID,       // an id outside 0 .. nscenes - 1 (entry: its index)                      }
    CKPT_CALL_REPEATED_ID,  // an id named twice (entry: the index of the second mention)             }
    CKPT_CALL_NO_BUFFER     // bufs[entry] is NULL                                                    }
};
struct CkptCallCheck { CkptCallFault fault; int entry; };
inline CkptCallCheck scene_checkpoint_call_check(int nscenes, bool state_set, bool scene_begun, int count, const int32_t *scene_ids, const void *const *bufs,
                                                 const int64_t *sizes) {
    if (nscenes <= 0) return {CKPT_CALL_NO_SCENES, -1};
    if (!state_set) return {CKPT_CALL_NO_STATE, -1};
    if (scene_begun) return {CKPT_CALL_MID_STEP, -1};
    if (count <= 0 || scene_ids == nullptr || bufs == nullptr || sizes == nullptr) return {CKPT_CALL_BAD_COUNT, -1};
    std::vector<uint8_t> named((std::size_t)nscenes, (uint8_t)0);
    for (int e = 0; e < count; e++) {
        const int s = scene_ids[e];
        if (s < 0 || s >= nscenes) return {CKPT_CALL_BAD_ID, e};
        if (named[(std::size_t)s]) return {CKPT_CALL_REPEATED_ID, e};
        named[(std::size_t)s] = 1;
        if (bufs[e] == nullptr) return {CKPT_CALL_NO_BUFFER, e};
    }
    return {CKPT_CALL_OK, -1};
}
inline int scene_checkpoint_call_error_code(CkptCallFault f) { return f == CKPT_CALL_OK ? SCA_OK : f <= CKPT_CALL_MID_STEP ? SCA_ERR_STATE : SCA_ERR_ARG; }
// The page-locked block both calls go through: one 32-byte entry per named scene (scene id, occupied rows, the two words the layout
// depends on, the byte the scene's blob starts at), then the blobs, each on a 128-byte boundary.
struct CkptEntry { int32_t scene, size, trk_words, has_paths; int64_t at, reserved; };
static_assert(sizeof(CkptEntry) == 32, "one table entry is two 16-byte pieces");
constexpr int64_t CKPT_BLOCK_ALIGN = 128;
inline int64_t ckpt_block_round(int64_t x) { return (x + CKPT_BLOCK_ALIGN - 1) / CKPT_BLOCK_ALIGN * CKPT_BLOCK_ALIGN; }

// ---- a trajectory log per scene (sca_scene_history_enable) -------------------------------------------------------------------------------------
// One allocation of capacity x n rows of SCENE_LOG_ROW_BYTES (HistRow, sca_kernels.hip.h).  Scene s owns rows [capacity * offsets[s],
// capacity * offsets[s + 1]); inside its part the layout is [row][agent] with pitch n_s, so any window of rows of one scene is one contiguous
// range.  Row r of a scene is the scene's r-th own step (steps[s] - 1 while that step runs): a restart, which zeroes steps[s], starts the log
// over, and rows of the episode before are simply beyond rows_logged.  Everything in int64_t: capacity x n passes 2^31 long before the log
// passes the memory of a device.
constexpr int64_t SCENE_LOG_ROW_BYTES = 64;
// where row r of scene-local agent i stands, in rows from the allocation's start (scene_begin = offsets[s], scene_size = n_s).  The kernel
// that writes and the host that reads back both call this.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int64_t scene_log_index(int capacity, int scene_begin, int scene_size, int r, int i) {
    return (int64_t)capacity * (int64_t)scene_begin + (int64_t)r * (int64_t)scene_size + (int64_t)i;
}
inline int64_t scene_log_bytes(int capacity, int n) { return SCENE_LOG_ROW_BYTES * (int64_t)capacity * (int64_t)n; }
// Steps beyond the capacity are counted, never written.
inline int scene_log_rows_logged(int steps, int capacity) { return steps < capacity ? steps : capacity; }
inline int scene_log_rows_dropped(int steps, int capacity) { return steps > capacity ? steps - capacity : 0; }

enum SceneLogFault {
    SCENE_LOG_OK = 0,
    SCENE_LOG_NO_SCENES,    // the context holds no scenes                                                     } SCA_ERR_STATE
    SCENE_LOG_MID_STEP,     // between a policy pass and its env update                                        }
    SCENE_LOG_STEPPED,      // enable: a scene has taken a step already (scene: the first such)                }
    SCENE_LOG_OFF,          // rows / read-back: the log is not enabled                                        }
    SCENE_LOG_BAD_CAPACITY, // enable: a negative capacity                                                     } SCA_ERR_ARG
    SCENE_LOG_BAD_SCENE,    // read-back: a scene outside 0 .. nscenes - 1                                     }
    SCENE_LOG_BAD_ROWS,     // read-back: a row window outside [0, rows_logged[scene])                         }
    SCENE_LOG_BAD_AGENTS    // read-back: an agent window outside the scene                                    }
};
struct SceneLogCheck { SceneLogFault fault; int scene; };
// sca_scene_history_enable.  steps: [nscenes] the scenes' step counters as they stand (may be NULL where capacity <= 0 or there are no
// scenes: it is read last).  Rows are indexed by a scene's own step count, so a log enabled behind a step would report rows it never wrote;
// capacity 0 only frees and may come at any step count.
inline SceneLogCheck scene_log_enable_check(int nscenes, bool scene_begun, const int32_t *steps, int capacity) {
    if (nscenes <= 0) return {SCENE_LOG_NO_SCENES, -1};
    if (scene_begun) return {SCENE_LOG_MID_STEP, -1};
    if (capacity < 0) return {SCENE_LOG_BAD_CAPACITY, -1};
    if (capacity > 0)
        for (int s = 0; s < nscenes; s++) if (steps[s] > 0) return {SCENE_LOG_STEPPED, s};
    return {SCENE_LOG_OK, -1};
}
// sca_scene_history_rows (window == false: the scene and the windows are not looked at) and sca_get_scene_history.  offsets: checked by
// scenes_check; steps_of_scene: steps[scene] where the scene is valid (read by the caller behind the checks that need no device value --
// pass 0 for a first round of them).
// size: [nscenes] the agents each scene holds (sca_restart_scenes_sized), NULL: every scene is full.
inline SceneLogCheck scene_log_check(int nscenes, const int32_t *offsets, bool enabled, int capacity, bool window, int scene, int steps_of_scene,
                                     int first_row, int nrows, int agent_begin, int agent_count, const int32_t *size = nullptr) {
    if (nscenes <= 0) return {SCENE_LOG_NO_SCENES, -1};
    if (!enabled) return {SCENE_LOG_OFF, -1};
    if (!window) return {SCENE_LOG_OK, -1};
    if (scene < 0 || scene >= nscenes) return {SCENE_LOG_BAD_SCENE, scene};
    const int64_t have = scene_log_rows_logged(steps_of_scene, capacity);
    if (!scene_log_agents_ok(size ? size[scene] : offsets[scene + 1] - offsets[scene], agent_begin, agent_count)) return {SCENE_LOG_BAD_AGENTS, scene};
    if (first_row < 0 || nrows < 0 || (int64_t)first_row + nrows > have) return {SCENE_LOG_BAD_ROWS, scene};
    return {SCENE_LOG_OK, scene};
}
inline int scene_log_error_code(SceneLogFault f) { return f == SCENE_LOG_OK ? SCA_OK : f <= SCENE_LOG_OFF ? SCA_ERR_STATE : SCA_ERR_ARG; }

// ---- finished scenes hand over their result with the step (sca_scene_harvest_enable) -----------------------------------------------------------
// One page-locked block of the library's, written by k_scene_harvest, the last kernel of a step: every scene's `live` and `steps` counters
// on every step, and for a scene that finished in the step its occupied rows (the columns of sca_get_state) and one sca_scene_summary.
// Every scene writes at ITS OWN place -- counters 2 s, summary s, rows offsets[s] + i, the index the rows have in the context -- so there is
// no cursor, no atomic and no order that depends on scheduling, and since a scene finishes at most once between two restarts nothing is
// ever overwritten before the host had its chance to read it.  Sections in the order of sca_scene_harvest's pointers, each on a 128-byte
// boundary (a line of the link's writes is never shared by two sections).
enum HarvestSection : int { HV_COUNTERS = 0, HV_SUMMARY, HV_POS, HV_VEL, HV_HEADING, HV_FLAGS, HV_TOTAL_DIST, HV_STEP_NUM, HV_SECTIONS };
constexpr int64_t HV_ALIGN = 128;
static_assert(sizeof(sca_scene_summary) == 64, "one summary record is half a 128-byte line");
struct HarvestLayout { int64_t off[HV_SECTIONS]; int64_t total; };
// counters: live, steps (i32 x 2) and the summary per SCENE; the rest per AGENT ROW, as in the host state block (host_section_row_bytes)
inline int64_t harvest_section_bytes(int s, int nscenes, int n) {
    return s == HV_COUNTERS ? 8 * (int64_t)nscenes : s == HV_SUMMARY ? (int64_t)sizeof(sca_scene_summary) * nscenes
           : (s == HV_POS || s == HV_HEADING ? 24 : s == HV_VEL ? 12 : s == HV_TOTAL_DIST ? 8 : s == HV_STEP_NUM ? 4 : 1) * (int64_t)n;
}
inline HarvestLayout scene_harvest_layout(int nscenes, int n) {
    HarvestLayout L;
    int64_t at = 0;
    for (int s = 0; s < HV_SECTIONS; s++) {
        L.off[s] = at;
        at += (harvest_section_bytes(s, nscenes, n) + HV_ALIGN - 1) / HV_ALIGN * HV_ALIGN;
    }
    L.total = at;
    return L;
}

enum HarvestFault {
    HARVEST_OK = 0,
    HARVEST_NO_SCENES,      // the context holds no scenes                                                     } SCA_ERR_STATE
    HARVEST_MID_STEP,       // enable / disable between a policy pass and its env update                       }
    HARVEST_OFF,            // get / collect: the harvest is not enabled                                       }
    HARVEST_NO_OUT,         // get / collect: an output pointer is NULL                                        } SCA_ERR_ARG
    HARVEST_BAD_STRUCT      // get: struct_bytes outside [the leading integers, the library's struct]          }
};
enum HarvestOp { HARVEST_ENABLE = 0, HARVEST_GET, HARVEST_COLLECT };        // (enable: on or off, the rules are the same)
// struct_bytes is looked at for HARVEST_GET only: at least sca_scene_harvest's leading integers, at most the struct (sca_host_state_get's rule)
inline HarvestFault scene_harvest_check(HarvestOp op, int nscenes, bool scene_begun, bool enabled, bool have_out, int struct_bytes) {
    if (nscenes <= 0) return HARVEST_NO_SCENES;
    if (op == HARVEST_ENABLE) return scene_begun ? HARVEST_MID_STEP : HARVEST_OK;
    if (!enabled) return HARVEST_OFF;
    if (!have_out) return HARVEST_NO_OUT;
    if (op == HARVEST_GET && (struct_bytes < (int)offsetof(sca_scene_harvest, counters) || struct_bytes > (int)sizeof(sca_scene_harvest))) return HARVEST_BAD_STRUCT;
    return HARVEST_OK;
}
inline int scene_harvest_error_code(HarvestFault f) { return f == HARVEST_OK ? SCA_OK : f <= HARVEST_OFF ? SCA_ERR_STATE : SCA_ERR_ARG; }

// sca_scene_harvest_collect's answer from the summaries as they stand: the scenes whose `fresh` word is set, ascending (batch_step, scene
// id), into ids[nscenes]; returns how many.  Reads only (the caller clears the words).
inline int scene_harvest_order(int nscenes, const sca_scene_summary *sum, int32_t *ids) {
    int count = 0;
    for (int s = 0; s < nscenes; s++) if (sum[s].fresh) ids[count++] = s;
    std::stable_sort(ids, ids + count, [sum](int32_t a, int32_t b) { return sum[a].batch_step < sum[b].batch_step; });   // stable: ids of one batch step stay ascending
    return count;
}

// ---- closest approach per agent, measured with the step (sca_scene_clearance_enable) -----------------------------------------------------------
// The rule mirrors the env's own collision test (mampenv.py:61-75: dis = l3norm(p_a, p_b), collision where dis <= r_a + r_b).  Agent row a
// of a scene is updated at every step of the scene's own that the scene began with somebody live and that a ENTERED unfinished (none of
// at-goal / collision / timed-out in its entry flags -- the step in which it gains one still counts).  For every other occupied row b,
// whatever its flags (a finished drone stays where it is and the reference still collides with it), c = l3norm(p_a, p_b) - (r_a + r_b):
// p the positions this step moved to, l3norm the reference's rounded norm (util.py:104; sca_core.h's, the exact one), the radius sum formed
// first, then subtracted.  The step's candidate is the smallest c, the lowest b on equal values; it replaces the record only where
// strictly smaller, so the earliest step wins ties.  The same over the scene's obstacles in their set order.  Never a partner: rows behind
// the scene's size, obstacle rows behind a slot's count, anything of another scene -- the caller passes the scene's occupied rows and its
// own obstacles, and nothing else.  k_scene_clearance (sca_scenes.hip.h) runs clearance_pair per pair; scene_clearance_step is one step of
// one scene over plain arrays, for the host (tests/scene_clearance_harness.cpp).  The norm is a parameter -- both pass L3Norm, sca_core.h's
// l3norm on plain coordinates -- so that this header stays free of the solver's arithmetic and its libm.
#if defined(__HIPCC__)
#define SCA_SCENES_HD __host__ __device__ inline
#else
#define SCA_SCENES_HD inline
#endif
constexpr uint32_t CLEAR_DONE_FLAGS = 7;           // FLAG_AT_GOAL | FLAG_COLLISION | FLAG_TIMEOUT (sca_core.h; sca_scenes.hip.h asserts it)
static_assert(sizeof(sca_scene_clearance) == 32, "one clearance record is two 16-byte pieces");
struct ClearPoint { double x, y, z, r; };          // a partner as the kernel stages it in LDS: position and radius, 32 bytes
SCA_SCENES_HD sca_scene_clearance scene_clearance_empty() {
    sca_scene_clearance e;
    e.agent_clear = __builtin_huge_val(); e.obs_clear = __builtin_huge_val();
    e.agent_partner = -1; e.agent_step = 0; e.obs_partner = -1; e.obs_step = 0;
    return e;
}
// One pair against one half of a record; partners arrive in ascending order, so "strictly smaller" keeps the lowest partner of a step and
// the earliest step.  The exact rounding (round5_py: a product, an fma, a division) is taken only by a pair that can still beat `clear`:
// with t = clear + rs + 2e-5, |a - b|^2 > t^2 means l3norm >= |a - b| - 0.5e-5 > clear + rs + 1e-5, far outside what the rounding of t, of
// its square and of the sum of squares (relative 2^-52 each) can move -- so every skipped pair has c > clear and the stored values are
// the rule's.  clear == +inf never skips (t^2 = +inf); t <= 0 never skips either.
template <class Norm>
SCA_SCENES_HD void clearance_pair(const ClearPoint &a, const ClearPoint &b, int partner, int step, double &clear, int32_t &who, int32_t &when, Norm norm) {
    const double rs = a.r + b.r;
    const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    double s = dx * dx + dy * dy;
    s = s + dz * dz;                                                   // (l3norm's own sum)
    const double t = clear + rs + 2e-5;
    if (t > 0.0 && s > t * t) return;
    const double c = norm(a.x, a.y, a.z, b.x, b.y, b.z) - rs;
    if (c < clear) { clear = c; who = partner; when = step; }
}
// one step of one scene: pos [size * 3] the moved positions of its occupied rows, radius [size], entry_flags [size] the flags the rows
// entered the step with, obs_pos [nobs * 3] / obs_radius [nobs] the scene's obstacles in set order, step = steps[s] (1-based), rec [size]
// updated in place
template <class Norm>
SCA_SCENES_HD void scene_clearance_step(int size, const double *pos, const double *radius, const uint32_t *entry_flags, int nobs, const double *obs_pos,
                                        const double *obs_radius, int step, sca_scene_clearance *rec, Norm norm) {
    for (int a = 0; a < size; a++) {
        if (entry_flags[a] & CLEAR_DONE_FLAGS) continue;
        const ClearPoint pa = {pos[3 * a], pos[3 * a + 1], pos[3 * a + 2], radius[a]};
        sca_scene_clearance r = rec[a];
        for (int b = 0; b < size; b++) {
            if (b == a) continue;
            const ClearPoint pb = {pos[3 * b], pos[3 * b + 1], pos[3 * b + 2], radius[b]};
            clearance_pair(pa, pb, b, step, r.agent_clear, r.agent_partner, r.agent_step, norm);
        }
        for (int j = 0; j < nobs; j++) {
            const ClearPoint po = {obs_pos[3 * j], obs_pos[3 * j + 1], obs_pos[3 * j + 2], obs_radius[j]};
            clearance_pair(pa, po, j, step, r.obs_clear, r.obs_partner, r.obs_step, norm);
        }
        rec[a] = r;
    }
}
// sca_scene_clearance_enable / sca_get_scene_clearance
enum ClearFault {
    CLEAR_OK = 0,
    CLEAR_NO_SCENES,        // the context holds no scenes                                                     } SCA_ERR_STATE
    CLEAR_MID_STEP,         // enable / disable between a policy pass and its env update                       }
    CLEAR_OFF,              // get: the feature is not enabled                                                 }
    CLEAR_BAD_SCENE,        // get: a scene outside 0 .. nscenes - 1                                           } SCA_ERR_ARG
    CLEAR_NO_OUT,           // get: out is NULL                                                                }
    CLEAR_BAD_STRUCT        // get: struct_bytes is not sizeof(sca_scene_clearance)                            }
};
inline ClearFault scene_clearance_check(bool get, int nscenes, bool scene_begun, bool enabled, int scene, bool have_out, int struct_bytes) {
    if (nscenes <= 0) return CLEAR_NO_SCENES;
    if (!get) return scene_begun ? CLEAR_MID_STEP : CLEAR_OK;
    if (!enabled) return CLEAR_OFF;
    if (scene < 0 || scene >= nscenes) return CLEAR_BAD_SCENE;
    if (!have_out) return CLEAR_NO_OUT;
    if (struct_bytes != (int)sizeof(sca_scene_clearance)) return CLEAR_BAD_STRUCT;
    return CLEAR_OK;
}
inline int scene_clearance_error_code(ClearFault f) { return f == CLEAR_OK ? SCA_OK : f <= CLEAR_OFF ? SCA_ERR_STATE : SCA_ERR_ARG; }

}  // namespace sca
