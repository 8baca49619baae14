// sca_respawn.h -- respawning agents in place (sca_respawn_agents) and the list of finished rows (sca_get_finished), include/sca_hip.h.
//
// A plain context (no scenes) whose agents get new missions one by one: the rows a call names become what sca_set_agents + sca_set_state
// (+ sca_device_tracker_enable) leave for an agent with the call's values, every other row keeps every word it had -- the reference's rule
// for assigning to one Agent object between two env.step() calls (mampenv.py:16-19; the kd-tree keeps its agentIDs order, kdTree.py:43-45).
//
// Everything here is pure and compiles for the host (tests/respawn_harness.cpp):
//   respawn_check      every refusal of the two entry points, with its code
//   respawn_layout     the sections of the page-locked block a call's arrays travel in
//   respawn_pack       the caller's arrays into that block (the host side of the call)
//   respawn_row        what one named row's scalar words become: the function k_respawn calls per row
//   finished_offsets   the scan rule of the ordered compaction behind sca_get_finished (finished_rank: a row's place inside its tile)
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "sca_core.h"
#include "sca_scenes.h"

namespace sca {

// ---- the refusals ------------------------------------------------------------------------------------------------------------------------
enum RespawnCall { RSP_CALL_RESPAWN = 0, RSP_CALL_FINISHED };
enum RespawnFault {
    RSP_OK = 0,
    RSP_NO_AGENTS,          // sca_set_agents first                                                           } SCA_ERR_STATE
    RSP_NO_STATE,           // no state yet                                                                   }
    RSP_MID_STEP,           // respawn between a policy pass and its env update                               }
    RSP_BAD_COUNT,          // count <= 0                                                                     } SCA_ERR_ARG
    RSP_NO_ARRAYS,          // a required array is NULL                                                       }
    RSP_BAD_ID,             // an id outside 0 .. n - 1 (entry: where)                                        }
    RSP_REPEATED_ID,        // an id named twice (entry: the later place)                                     }
    RSP_NOT_FINITE,         // a position that is not finite (entry: the packed row)                          }
    RSP_NOT_POSITIVE,       // radius, pref_speed or max_run_dist not positive and finite                     }
    RSP_GOAL_HEADING,       // goal_heading == NULL with a tracked row named under the device tracker         }
    RSP_PATH_HALF,          // only one of path_offsets / path_points                                         }
    RSP_PATH_OFFSETS,       // offsets negative at the start or decreasing (entry: the row)                   }
    RSP_PATH_TOO_LONG,      // a list longer than the room per row                                            }
    RSP_PATH_NOT_FINITE,    // a waypoint that is not finite (entry: the waypoint)                            }
    RSP_FIN_ARGS,           // sca_get_finished: capacity < 0, NULL count, NULL rows with capacity > 0, bad struct_bytes }
    RSP_SCENES,             // scenes are set: sca_restart_scenes                                             } SCA_ERR_UNSUPPORTED
    RSP_SHARD,              // a shard with count < n                                                         }
    RSP_COMM,               // a communicator                                                                 }
    RSP_PARTITION,          // the cell-owner partition                                                       }
    RSP_PATH_BLOCK,         // waypoint lists in block form: sca_set_path_slots                               }
    RSP_PATH_NO_SLOTS       // path arrays while no slot form is set                                          }
};
inline int respawn_error_code(RespawnFault f) {
    return f == RSP_OK ? SCA_OK : f <= RSP_MID_STEP ? SCA_ERR_STATE : f <= RSP_FIN_ARGS ? SCA_ERR_ARG : SCA_ERR_UNSUPPORTED;
}
// what the rules read of the context
struct RespawnCtx {
    bool agents, state, mid_step, scenes, comm, partition;
    int n, shard_count;
    bool tracker_on;                           // the device tracker (sca_device_tracker_enable)
    bool paths_block;                          // waypoint lists in block form (sca_set_paths)
    int path_W;                                // room per row in slot form, 0: no slot form
    const uint8_t *policy_now;                 // [n] the agents' policies as they stand
};
struct RespawnArgs {
    int count; const int32_t *ids;
    const double *pos; const float *vel; const double *heading, *radius, *pref_speed, *goal;
    const uint8_t *zaxis;                      // nullable: the rows keep theirs
    const double *max_run_dist, *goal_heading;
    const int32_t *path_offsets; const double *path_points;
};
// fault: which rule failed; entry: where (-1: nowhere in particular); path_total: the waypoints the call brings
struct RespawnCheck { RespawnFault fault; int entry; int path_total; };

// the context-wide part, shared by the two entry points
inline RespawnFault respawn_context_check(RespawnCall call, const RespawnCtx &C) {
    if (!C.agents) return RSP_NO_AGENTS;
    if (!C.state) return RSP_NO_STATE;
    if (call == RSP_CALL_RESPAWN && C.mid_step) return RSP_MID_STEP;
    if (C.scenes) return RSP_SCENES;
    if (C.comm) return RSP_COMM;
    if (C.partition) return RSP_PARTITION;
    if (C.shard_count < C.n) return RSP_SHARD;
    return RSP_OK;
}
inline RespawnCheck respawn_check(const RespawnCtx &C, const RespawnArgs &A) {
    if (const RespawnFault f = respawn_context_check(RSP_CALL_RESPAWN, C)) return {f, -1, 0};
    if (A.count <= 0) return {RSP_BAD_COUNT, -1, 0};
    if (!A.ids || !A.pos || !A.vel || !A.heading || !A.radius || !A.pref_speed || !A.goal || !A.max_run_dist) return {RSP_NO_ARRAYS, -1, 0};
    for (int r = 0; r < A.count; r++) if (A.ids[r] < 0 || A.ids[r] >= C.n) return {RSP_BAD_ID, r, 0};
    {   // a repeated id, found in time that grows with the call and not with the swarm: the (id, place) pairs sorted
        std::vector<std::pair<int32_t, int>> s((std::size_t)A.count);
        for (int r = 0; r < A.count; r++) s[(std::size_t)r] = {A.ids[r], r};
        std::sort(s.begin(), s.end());
        int at = -1;
        for (int k = 1; k < A.count; k++) if (s[(std::size_t)k].first == s[(std::size_t)k - 1].first && (at < 0 || s[(std::size_t)k].second < at)) at = s[(std::size_t)k].second;
        if (at >= 0) return {RSP_REPEATED_ID, at, 0};
    }
    for (int r = 0; r < A.count; r++)
        for (int k = 0; k < 3; k++) if (!restart_finite(A.pos[3 * r + k])) return {RSP_NOT_FINITE, r, 0};
    for (int r = 0; r < A.count; r++) {
        const double v[3] = {A.radius[r], A.pref_speed[r], A.max_run_dist[r]};
        for (int k = 0; k < 3; k++) if (!(v[k] > 0.0) || !restart_finite(v[k])) return {RSP_NOT_POSITIVE, r, 0};
    }
    if (C.tracker_on && !A.goal_heading)
        for (int r = 0; r < A.count; r++) if (restart_policy_tracked(C.policy_now[A.ids[r]])) return {RSP_GOAL_HEADING, r, 0};
    if ((A.path_offsets == nullptr) != (A.path_points == nullptr)) return {RSP_PATH_HALF, -1, 0};
    if (C.paths_block) return {RSP_PATH_BLOCK, -1, 0};
    if (!A.path_offsets) return {RSP_OK, -1, 0};
    if (C.path_W <= 0) return {RSP_PATH_NO_SLOTS, -1, 0};
    if (A.path_offsets[0] < 0) return {RSP_PATH_OFFSETS, 0, 0};
    for (int r = 0; r < A.count; r++) {
        if (A.path_offsets[r + 1] < A.path_offsets[r]) return {RSP_PATH_OFFSETS, r, 0};
        if (A.path_offsets[r + 1] - A.path_offsets[r] > C.path_W) return {RSP_PATH_TOO_LONG, r, 0};
    }
    const int first = A.path_offsets[0], total = A.path_offsets[A.count] - first;
    for (int64_t k = 3 * (int64_t)first; k < 3 * ((int64_t)first + total); k++) if (!restart_finite(A.path_points[k])) return {RSP_PATH_NOT_FINITE, (int)(k / 3), total};
    return {RSP_OK, -1, total};
}
// sca_get_finished(rows, capacity, count, struct_bytes)
constexpr int FINISHED_ROW_BYTES = 48;
inline RespawnFault finished_check(const RespawnCtx &C, bool have_rows, int capacity, bool have_count, int struct_bytes) {
    if (!C.agents) return RSP_NO_AGENTS;
    if (!C.state) return RSP_NO_STATE;
    if (capacity < 0 || !have_count || (capacity > 0 && !have_rows) || struct_bytes != FINISHED_ROW_BYTES) return RSP_FIN_ARGS;
    const RespawnFault f = respawn_context_check(RSP_CALL_FINISHED, C);
    return f;
}

// ---- the block ---------------------------------------------------------------------------------------------------------------------------
// The page-locked block a call's arrays travel in, sized for `cap` named rows and W waypoints of room per row (0: no slot form): one section
// per array, aligned to 64 bytes as the restart block's are.  RSB_REC holds whole public records (48 bytes: position, float32 velocity,
// flags 0, radius), which the kernel copies as 16-byte pieces; RSB_BITS one byte per row (RSP_BIT_*).
enum RespawnSection : int { RSB_IDS = 0, RSB_REC, RSB_HEADING, RSB_GOAL, RSB_GOAL_HEADING, RSB_PREF_SPEED, RSB_MAX_RUN_DIST, RSB_ZAXIS, RSB_BITS,
                            RSB_PATH_OFF, RSB_PATH_PTS, RSB_SECTIONS };
constexpr int64_t RSP_ALIGN = 64;
constexpr int RSP_REC_BYTES = 48;
static_assert(sizeof(PubRec) == RSP_REC_BYTES, "the block's records are public records");
struct RespawnLayout { int64_t off[RSB_SECTIONS]; int64_t total; };
inline int64_t respawn_section_bytes(int s, int cap, int W) {
    switch (s) {
    case RSB_IDS: return 4 * (int64_t)cap;
    case RSB_REC: return RSP_REC_BYTES * (int64_t)cap;
    case RSB_HEADING: case RSB_GOAL: case RSB_GOAL_HEADING: return 24 * (int64_t)cap;
    case RSB_PREF_SPEED: case RSB_MAX_RUN_DIST: return 8 * (int64_t)cap;
    case RSB_ZAXIS: case RSB_BITS: return (int64_t)cap;
    case RSB_PATH_OFF: return W > 0 ? 4 * ((int64_t)cap + 1) : 0;
    default: return W > 0 ? 24 * (int64_t)W * (int64_t)cap : 0;
    }
}
inline RespawnLayout respawn_layout(int cap, int W) {
    RespawnLayout L;
    int64_t at = 0;
    for (int s = 0; s < RSB_SECTIONS; s++) {
        L.off[s] = at;
        at += (respawn_section_bytes(s, cap, W) + RSP_ALIGN - 1) / RSP_ALIGN * RSP_ALIGN;
    }
    L.total = at;
    return L;
}
// what the block carries beyond the required arrays
constexpr uint32_t RESPAWN_HAS_ZAXIS = 1,        // the rows take the call's zaxis bytes (else they keep theirs)
                   RESPAWN_HAS_PATH_SLOTS = 2,   // the lists are in slot form: every named row's cursors are written
                   RESPAWN_HAS_PATHS = 4;        // ... and the call brings lists (else the named rows' lists become empty)
// a row's byte in RSB_BITS
constexpr uint8_t RSP_BIT_TRACKED = 1,           // the device tracker is on and the row's policy is SCA / RVO3D+Dubins: the initial AgentTrack, goal_heading, vpref_mode 1, vpref_ext 0
                  RSP_BIT_MODE_RESET = 2;        // a straight-line row whose v_pref k_waypoint was writing (it had a list): vpref_mode 0, its policy's own rule
                                                 // again -- k_waypoint sets it back at the next pass where the new list is not empty
// The caller's arrays into the block (the host side of sca_respawn_agents, behind respawn_check).  path_vpref: [n] 1 where the row is a
// straight-line agent with a list at the moment (null: no lists).  Returns the `has` word.  The path offsets are rebased to start at 0.
inline uint32_t respawn_pack(uint8_t *blk, const RespawnLayout &L, const RespawnCtx &C, const RespawnArgs &A, const uint8_t *path_vpref) {
    const int T = A.count;
    uint32_t has = 0;
    std::memcpy(blk + L.off[RSB_IDS], A.ids, sizeof(int32_t) * (std::size_t)T);
    PubRec *rec = (PubRec *)(blk + L.off[RSB_REC]);
    uint8_t *bits = blk + L.off[RSB_BITS];
    for (int r = 0; r < T; r++) {
        PubRec p;
        p.px = A.pos[3 * r]; p.py = A.pos[3 * r + 1]; p.pz = A.pos[3 * r + 2];
        p.vx = A.vel[3 * r]; p.vy = A.vel[3 * r + 1]; p.vz = A.vel[3 * r + 2];
        p.flags = 0u; p.radius = A.radius[r];
        rec[r] = p;
        const int a = A.ids[r];
        const bool tracked = C.tracker_on && restart_policy_tracked(C.policy_now[a]);
        bits[r] = (uint8_t)((tracked ? RSP_BIT_TRACKED : 0) | (!tracked && path_vpref && path_vpref[a] ? RSP_BIT_MODE_RESET : 0));
    }
    std::memcpy(blk + L.off[RSB_HEADING], A.heading, sizeof(double) * 3 * (std::size_t)T);
    std::memcpy(blk + L.off[RSB_GOAL], A.goal, sizeof(double) * 3 * (std::size_t)T);
    if (A.goal_heading) std::memcpy(blk + L.off[RSB_GOAL_HEADING], A.goal_heading, sizeof(double) * 3 * (std::size_t)T);
    else std::memset(blk + L.off[RSB_GOAL_HEADING], 0, sizeof(double) * 3 * (std::size_t)T);      // (read only for tracked rows, which respawn_check refused without it)
    std::memcpy(blk + L.off[RSB_PREF_SPEED], A.pref_speed, sizeof(double) * (std::size_t)T);
    std::memcpy(blk + L.off[RSB_MAX_RUN_DIST], A.max_run_dist, sizeof(double) * (std::size_t)T);
    if (A.zaxis) { std::memcpy(blk + L.off[RSB_ZAXIS], A.zaxis, (std::size_t)T); has |= RESPAWN_HAS_ZAXIS; }
    if (C.path_W > 0) {
        has |= RESPAWN_HAS_PATH_SLOTS;
        if (A.path_offsets) {
            int32_t *off = (int32_t *)(blk + L.off[RSB_PATH_OFF]);
            const int32_t first = A.path_offsets[0];
            for (int r = 0; r <= T; r++) off[r] = A.path_offsets[r] - first;
            if (off[T] > 0) std::memcpy(blk + L.off[RSB_PATH_PTS], A.path_points + 3 * (std::size_t)first, sizeof(double) * 3 * (std::size_t)off[T]);
            has |= RESPAWN_HAS_PATHS;
        }
    }
    return has;
}

// ---- one row -----------------------------------------------------------------------------------------------------------------------------
// The scalar words of a named row behind the call, from its byte of RSB_BITS, the flags its old record carried and the call's `has` word
// (the three-component arrays and the public record travel as they are).  What a fresh context holds for the agent:
//   total_dist 0, step_num 0, status 0                       sca_set_agents / sca_set_state
//   nbr_n 0, nbr_valid 0, near_n -1, nbr0 -1                 no pass of this mission has left a list (sca_device_tracker_enable's values)
//   done_delta                                               K4's striped done_count: + 1 for a row that was done (k_scene_load's rule)
//   write_mode / mode                                        vpref_mode is written: 1 for a tracked row (vpref_ext 0 with it), 0 for a reset row;
//                                                            otherwise the row's fed vpref_ext / vpref_mode stay (sca_set_vpref refreshes them)
//   path_len                                                 slot form: len = rem = the row's list length, now_goal None; -1: no slot form, nothing written
struct RespawnRow {
    double total_dist, nbr0;
    int32_t step_num, status, nbr_n, near_n, done_delta, path_len;
    uint8_t nbr_valid, tracked, write_mode, mode, write_zaxis;
};
constexpr uint32_t RSP_DONE_FLAGS = FLAG_AT_GOAL | FLAG_COLLISION | FLAG_TIMEOUT;
SCA_HD RespawnRow respawn_row(uint8_t bits, uint32_t old_flags, uint32_t has, int32_t list_len) {
    RespawnRow w;
    w.total_dist = 0.0; w.nbr0 = -1.0;
    w.step_num = 0; w.status = 0; w.nbr_n = 0; w.near_n = -1;
    w.done_delta = (old_flags & RSP_DONE_FLAGS) ? 1 : 0;
    w.path_len = (has & RESPAWN_HAS_PATH_SLOTS) ? ((has & RESPAWN_HAS_PATHS) ? list_len : 0) : -1;
    w.nbr_valid = 0;
    w.tracked = (bits & RSP_BIT_TRACKED) ? 1 : 0;
    w.write_mode = (bits & (RSP_BIT_TRACKED | RSP_BIT_MODE_RESET)) ? 1 : 0;
    w.mode = w.tracked;
    w.write_zaxis = (has & RESPAWN_HAS_ZAXIS) ? 1 : 0;
    return w;
}

// ---- the row write -------------------------------------------------------------------------------------------------------------------------
// What one lane of the wavefront that serves row `a` stores (lane 0 .. 63), shared by k_respawn (the source of the values: the call's
// block, RespawnBlockSrc) and k_mission_advance (the row's table entry, MissionSrc in sca_missions.h), so that the two cannot drift apart:
//   public record     three 16-byte pieces by lanes 0 .. 2
//   three-component   heading, goal (goal_heading, vpref_ext, now_goal): one component per lane 0 .. 2
//   scalar fields     lane 0 (respawn_row says which and what)
//   AgentTrack        consecutive 4-byte words by consecutive lanes from the one initial record (tracked rows under the device tracker)
// Dev: the arrays a respawn writes (RespawnDev in sca_respawn.hip.h; plain host arrays in the tests' harnesses); null pointers (no tracker,
// no lists, no closest-approach records) are skipped.  Not here: the done_count stripe (an atomic) and the waypoints (respawn_write_list).
struct __attribute__((may_alias, aligned(16))) RespawnPiece { uint32_t w[4]; };
// a piece from its values, word by word (no local array whose address is taken: nothing of it goes to scratch)
SCA_HD void piece_put64(RespawnPiece &q, int half, double x) { uint64_t u; __builtin_memcpy(&u, &x, 8); q.w[2 * half] = (uint32_t)u; q.w[2 * half + 1] = (uint32_t)(u >> 32); }
SCA_HD uint32_t piece_bits32(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }
struct RespawnBlockSrc {
    const uint8_t *blk; const RespawnLayout &L; int r;
    SCA_HD RespawnPiece piece(int lane, const PubRec *) const { return ((const RespawnPiece *)(blk + L.off[RSB_REC] + (int64_t)RSP_REC_BYTES * r))[lane]; }
    SCA_HD bool writes_heading() const { return true; }
    SCA_HD double heading(int k) const { return ((const double *)(blk + L.off[RSB_HEADING]))[3 * (int64_t)r + k]; }
    SCA_HD double goal(int k) const { return ((const double *)(blk + L.off[RSB_GOAL]))[3 * (int64_t)r + k]; }
    SCA_HD double goal_heading(int k) const { return ((const double *)(blk + L.off[RSB_GOAL_HEADING]))[3 * (int64_t)r + k]; }
    SCA_HD double pref_speed() const { return ((const double *)(blk + L.off[RSB_PREF_SPEED]))[r]; }
    SCA_HD double max_run_dist() const { return ((const double *)(blk + L.off[RSB_MAX_RUN_DIST]))[r]; }
    SCA_HD uint8_t zaxis() const { return (blk + L.off[RSB_ZAXIS])[r]; }
};
template <class Dev, class Src>
SCA_HD void respawn_write_row(const Dev &d, int a, int lane, const RespawnRow &w, const Src &s) {
    if (lane < RSP_REC_BYTES / 16) ((RespawnPiece *)(d.rec + a))[lane] = s.piece(lane, d.rec + a);
    if (lane < 3) {
        const int64_t g = 3 * (int64_t)a + lane;
        if (s.writes_heading()) d.heading[g] = s.heading(lane);
        d.goal[g] = s.goal(lane);
        if (w.tracked) { d.vpref_ext[g] = 0.0; if (d.trk_goal_heading) d.trk_goal_heading[g] = s.goal_heading(lane); }
        if (w.path_len >= 0 && d.now_goal) d.now_goal[g] = __builtin_nan("");
    }
    if (lane == 0) {
        d.total_dist[a] = w.total_dist; d.step_num[a] = w.step_num; d.status[a] = w.status;
        d.pref_speed[a] = s.pref_speed();
        d.max_run_dist[a] = s.max_run_dist();
        if (w.write_zaxis) d.zaxis[a] = s.zaxis();
        if (w.write_mode) d.vpref_mode[a] = w.mode;
        d.nbr_n[a] = w.nbr_n; d.nbr_valid[a] = w.nbr_valid; d.near_n[a] = w.near_n;
        if (d.trk_nbr0) d.trk_nbr0[a] = w.nbr0;
        if (w.path_len >= 0 && d.path_len) { d.path_len[a] = w.path_len; d.path_rem[a] = w.path_len; }
        if (d.clear) d.clear[a] = scene_clearance_empty();            // the new mission has met nobody yet; other rows keep this one as a partner
    }
    if (w.tracked && d.trk_st)                                         // the AgentTrack record, word by word from the one initial record
        for (int k = lane; k < d.trk_words; k += 64) d.trk_st[(int64_t)a * d.trk_words + k] = d.trk_init[k];
}

// ---- the list write --------------------------------------------------------------------------------------------------------------------------
// A row's new list into its own room pts[3 (W a + k)]: consecutive lanes of the wavefront that serves row `a` on consecutive coordinates,
// behind respawn_write_row (which has written len = rem = `len` and now_goal None).  src: the list's first coordinate -- in the call's block
// (k_respawn) or in the tables' packed lists (k_mission_advance, k_mission_gate_take): the three share this copy so that they cannot drift
// apart.  Room behind the list's length is never read (rem <= len) and is left as it is.
SCA_HD void respawn_write_list(double *pts, int W, int a, int lane, const double *src, int32_t len) {
    double *dst = pts + 3 * path_slot_index(W, a);
    for (int k = lane; k < 3 * len; k += 64) dst[k] = src[k];
}

// ---- the finished list -------------------------------------------------------------------------------------------------------------------
// An ORDERED compaction: the rows that carry any of at-goal / collision / timeout, ascending ids.  The swarm is cut into tiles of
// FIN_TILE consecutive rows (one workgroup each); a tile counts its finished rows, finished_offsets turns the counts into each tile's first
// place (an exclusive scan, the total behind it), and a finished row stands at its tile's offset plus the number of finished rows before
// it in the tile (finished_rank over the tile's flag words).
constexpr int FIN_TILE = 256;
inline int finished_tiles(int n) { return (n + FIN_TILE - 1) / FIN_TILE; }
SCA_HD bool finished_flag(uint32_t flags) { return (flags & RSP_DONE_FLAGS) != 0; }
// what the list holds: a vacant row (sca_vacancy.h) is settled for good but has not "finished" -- nobody is to give it a new mission by this list
SCA_HD bool finished_listed(uint32_t flags) { return finished_flag(flags) && !(flags & FLAG_VACANT); }
// offsets[t] = counts[0] + .. + counts[t - 1]; returns the total
SCA_HD int finished_offsets(const int32_t *counts, int tiles, int32_t *offsets) {
    int at = 0;
    for (int t = 0; t < tiles; t++) { offsets[t] = at; at += counts[t]; }
    return at;
}
// the finished rows among the first `lane` of a wavefront whose finished lanes are the set bits of `mask`
SCA_HD int finished_rank(unsigned long long mask, int lane) { return __builtin_popcountll(mask & ((1ull << lane) - 1ull)); }

}  // namespace sca
