// sca_missions.h -- mission tables: a row that ends inside a step takes its next mission there (sca_set_missions, sca_get_mission_results,
// sca_get_mission_totals, sca_get_mission_state; include/sca_hip.h).
//
// Every agent row has room for M entries (slot form, entry[M a + j], as the path slots are laid out) and a ring of R result records.  The
// step's last kernel (k_mission_advance, sca_missions.hip.h) finds the rows that ENDED in the step, writes a result for each and, where the
// ended flight names a successor, makes the row what sca_respawn_agents naming that row with the entry's values leaves -- through the one
// row write the respawn kernel uses (respawn_write_row, sca_respawn.h).
//
// Everything here is pure and compiles for the host (tests/missions_harness.cpp):
//   mission_check       every refusal of sca_set_missions and of the getters, with its code; which entries are reachable
//   mission_paths_check every refusal of sca_set_missions_paths: mission_check's, then the lists' (one packed CSR over the flat entry index)
//   mission_ended       did a row end in this step (the flag words in front of and behind K4)
//   mission_take        the outcome of an ended row and the successor it names
//   MissionSrc          an entry as the source of respawn_write_row's values
//   mission_take_bits   the bits byte and the `has` word respawn_row reads for a taken row, with and without lists (mission_take_has)
//   mission_new         how many results of a row's ring have not been collected (the collect's count per row)
// and the admission gate in front of the take (sca_set_mission_gate; the kernels: sca_mission_gate.hip.h):
//   mission_gate_check  every refusal of sca_set_mission_gate and of the gate's getters, the cap and the scratch a gate needs
//   mission_gate_place  a candidate's place in the step's offer order from its class, its rank in the class and the waiting rows' count
//   mission_gate_query  the sphere a candidate is tested as (START_HERE: where the row stands)
//   mission_gate_settle a verdict into the row's waiting / verdict / refusal words and the counter that moves
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

#include "sca_respawn.h"
#include "sca_spawn.h"

namespace sca {

static_assert(sizeof(sca_mission) == 128, "sca_mission is 128 bytes: eight 16-byte pieces");
static_assert(sizeof(sca_mission_result) == 96, "sca_mission_result is 96 bytes: six 16-byte pieces");
static_assert(sizeof(sca_mission_totals) == 64, "sca_mission_totals is eight 64-bit counters");
static_assert(offsetof(PubRec, px) == 0 && offsetof(PubRec, py) == 8 && offsetof(PubRec, pz) == 16 && offsetof(PubRec, vx) == 24 && offsetof(PubRec, vy) == 28 &&
              offsetof(PubRec, vz) == 32 && offsetof(PubRec, flags) == 36 && offsetof(PubRec, radius) == 40, "MissionSrc::piece builds the public record's three pieces");
static_assert(offsetof(sca_mission_result, total_dist) == 16 && offsetof(sca_mission_result, update) == 48 && offsetof(sca_mission_result, clear) == 64 &&
              offsetof(sca_scene_clearance, agent_partner) == 16, "k_mission_advance builds the result's six pieces");
constexpr int MISSION_MAX_M = 127;                 // successors are int8 entry indices of the same row
constexpr int MISSION_MAX_R = 1 << 16;
constexpr int64_t MISSION_MAX_SLOTS = 1 << 24;     // M x n and R x n: the tables and the rings stay below 2 GiB each
constexpr uint8_t MISSION_KNOWN_FLAGS = SCA_MISSION_START_HERE | SCA_MISSION_KEEP_ZAXIS;

// ---- the refusals ------------------------------------------------------------------------------------------------------------------------
enum MissionFault {
    MSF_OK = 0,
    MSF_NO_AGENTS,          // sca_set_agents first                                                           } SCA_ERR_STATE
    MSF_MID_STEP,           // between a policy pass and its env update                                       }
    MSF_OFF,                // a getter while no tables are set                                               }
    MSF_BAD_M,              // M outside 1 .. MISSION_MAX_M                                                   } SCA_ERR_ARG
    MSF_BAD_R,              // R outside 1 .. MISSION_MAX_R                                                   }
    MSF_BAD_N,              // n other than the agent count                                                   }
    MSF_NO_ARRAYS,          // a NULL array                                                                   }
    MSF_TOO_LARGE,          // M x n or R x n not addressable                                                 }
    MSF_BAD_SUCCESSOR,      // a successor outside -1 .. M - 1 (entry: the row, or the flat entry index)      }
    MSF_NOT_FINITE,         // a reachable entry with a position, heading, goal or velocity that is not finite }
    MSF_NOT_POSITIVE,       // a reachable entry whose pref_speed or max_run_dist is not positive and finite  }
    MSF_BAD_ZAXIS,          // a reachable entry with a zaxis byte above 1 and no KEEP_ZAXIS                  }
    MSF_BAD_FLAGS,          // a reachable entry with unknown flag bits                                       }
    MSF_GET_ARGS,           // a getter: bad struct_bytes, capacity, range or a NULL output                   }
    MSF_SCENES,             // scenes are set                                                                 } SCA_ERR_UNSUPPORTED
    MSF_SHARD,              // a shard with count < n                                                         }
    MSF_COMM,               // a communicator                                                                 }
    MSF_PARTITION,          // the cell-owner partition                                                       }
    MSF_PATHS,              // waypoint lists in either form                                                  }
    MSF_STEP_HOST,          // sca_step_host while tables are set                                             }
    // sca_set_missions_paths' own (behind the older values, which keep their numbers)
    MSF_PATH_NO_SLOTS,      // path_offsets while the context's lists are not in slot form                    } SCA_ERR_STATE
    MSF_PATH_START,         // path_offsets[0] != 0                                                           } SCA_ERR_ARG
    MSF_PATH_DECREASING,    // offsets that decrease (entry: the flat entry index)                            }
    MSF_PATH_NO_POINTS,     // path_points == NULL with points to read                                        }
    MSF_PATH_TOTAL,         // more than MISSION_PATH_MAX_POINTS points                                       }
    MSF_PATH_TOO_LONG,      // a reachable entry whose list is longer than the room per row                   }
    MSF_PATH_NOT_FINITE,    // a reachable entry whose list holds a point that is not finite                  }
    MSF_PATH_CLEAR          // sca_set_paths(0 / NULL) while tables with lists stand                          } SCA_ERR_UNSUPPORTED
};
inline int mission_error_code(MissionFault f) {
    if (f > MSF_STEP_HOST) return f == MSF_PATH_NO_SLOTS ? SCA_ERR_STATE : f <= MSF_PATH_NOT_FINITE ? SCA_ERR_ARG : SCA_ERR_UNSUPPORTED;
    return f == MSF_OK ? SCA_OK : f <= MSF_OFF ? SCA_ERR_STATE : f <= MSF_GET_ARGS ? SCA_ERR_ARG : SCA_ERR_UNSUPPORTED;
}
// what the rules read of the context (path_W: read by mission_paths_check alone -- the room per row while the lists are in slot form, 0:
// no slot form; `paths` stays "lists in either form")
struct MissionCtx {
    bool agents, mid_step, scenes, comm, partition, paths;
    int n, shard_count;
    int path_W = 0;
};
struct MissionArgs { int M, R, n; const sca_mission *entries; const int32_t *first_ok, *first_fail; };
// fault: which rule failed; entry: where (a row for first_ok / first_fail, else the flat entry index M a + j; -1: nowhere in particular);
// max_pref_speed: the largest pref_speed among the reachable entries (0: none reachable)
struct MissionCheck { MissionFault fault; int64_t entry; double max_pref_speed; };

// what else the context runs: the part that is also asked the other way round (an entry point that would bring scenes, a shard, a
// communicator, the partition or lists while tables stand refuses with the same fault)
inline MissionFault mission_context_check(const MissionCtx &C) {
    if (C.scenes) return MSF_SCENES;
    if (C.comm) return MSF_COMM;
    if (C.partition) return MSF_PARTITION;
    if (C.shard_count < C.n) return MSF_SHARD;
    if (C.paths) return MSF_PATHS;
    return MSF_OK;
}
inline MissionFault mission_entry_check(const sca_mission &e) {
    if (e.flags & ~MISSION_KNOWN_FLAGS) return MSF_BAD_FLAGS;
    const bool here = (e.flags & SCA_MISSION_START_HERE) != 0;
    for (int k = 0; k < 3; k++) {
        if (!here && (!restart_finite(e.pos[k]) || !restart_finite(e.heading[k]))) return MSF_NOT_FINITE;
        if (!restart_finite(e.goal[k]) || !restart_finite(e.goal_heading[k]) || !restart_finite((double)e.vel[k])) return MSF_NOT_FINITE;
    }
    if (!(e.pref_speed > 0.0) || !restart_finite(e.pref_speed) || !(e.max_run_dist > 0.0) || !restart_finite(e.max_run_dist)) return MSF_NOT_POSITIVE;
    if (!(e.flags & SCA_MISSION_KEEP_ZAXIS) && e.zaxis > 1) return MSF_BAD_ZAXIS;
    return MSF_OK;
}
// reached (nullable): [M n] 1 where an entry is reachable from its row's first_ok / first_fail through successors
inline MissionCheck mission_check(const MissionCtx &C, const MissionArgs &A, uint8_t *reached = nullptr) {
    if (!C.agents) return {MSF_NO_AGENTS, -1, 0.0};
    if (C.mid_step) return {MSF_MID_STEP, -1, 0.0};
    if (const MissionFault f = mission_context_check(C)) return {f, -1, 0.0};
    if (A.M < 1 || A.M > MISSION_MAX_M) return {MSF_BAD_M, -1, 0.0};
    if (A.R < 1 || A.R > MISSION_MAX_R) return {MSF_BAD_R, -1, 0.0};
    if (A.n != C.n) return {MSF_BAD_N, -1, 0.0};
    if (!A.entries || !A.first_ok || !A.first_fail) return {MSF_NO_ARRAYS, -1, 0.0};
    if ((int64_t)A.M * A.n > MISSION_MAX_SLOTS || (int64_t)A.R * A.n > MISSION_MAX_SLOTS) return {MSF_TOO_LARGE, -1, 0.0};
    const int M = A.M;
    for (int a = 0; a < A.n; a++)
        if (A.first_ok[a] < -1 || A.first_ok[a] >= M || A.first_fail[a] < -1 || A.first_fail[a] >= M) return {MSF_BAD_SUCCESSOR, a, 0.0};
    for (int64_t e = 0; e < (int64_t)M * A.n; e++)                       // (every entry's successors, reachable or not: the kernel never reads an index it could not follow)
        if (A.entries[e].next_ok < -1 || A.entries[e].next_ok >= M || A.entries[e].next_fail < -1 || A.entries[e].next_fail >= M) return {MSF_BAD_SUCCESSOR, e, 0.0};
    double top = 0.0;
    std::vector<int> todo;
    std::vector<uint8_t> seen((std::size_t)M);
    for (int a = 0; a < A.n; a++) {
        std::fill(seen.begin(), seen.end(), (uint8_t)0);
        todo.clear();
        const auto push = [&](int j) { if (j >= 0 && !seen[(std::size_t)j]) { seen[(std::size_t)j] = 1; todo.push_back(j); } };
        push(A.first_ok[a]); push(A.first_fail[a]);
        while (!todo.empty()) {
            const int j = todo.back();
            todo.pop_back();
            const sca_mission &e = A.entries[(int64_t)M * a + j];
            push(e.next_ok); push(e.next_fail);
        }
        for (int j = 0; j < M; j++) {                                    // (in entry order: the first fault reported is the lowest flat index)
            if (reached) reached[(int64_t)M * a + j] = seen[(std::size_t)j];
            if (!seen[(std::size_t)j]) continue;
            const sca_mission &e = A.entries[(int64_t)M * a + j];
            if (const MissionFault f = mission_entry_check(e)) return {f, (int64_t)M * a + j, 0.0};
            if (e.pref_speed > top) top = e.pref_speed;
        }
    }
    return {MSF_OK, -1, top};
}
// sca_set_missions_paths(M, R, n, entries, first_ok, first_fail, path_offsets, path_points): one packed CSR of lists over the flat entry
// index M a + j.  Decided in this order: mission_check's context faults (lists in SLOT form are no fault here, lists in block form are
// MSF_PATHS), offsets without a slot form, mission_check's argument faults, then the lists' own -- the offsets of every entry, the lengths
// and the points of the REACHABLE entries only, lowest flat index first (an entry nobody reaches is not inspected beyond its offsets, as
// its values are not).  path_offsets == NULL: every entry brings the empty list.
constexpr int64_t MISSION_PATH_MAX_POINTS = ((int64_t)1 << 31) / 3;    // every coordinate index 3 k + 2 stays below 2^31
struct MissionPathArgs { const int32_t *path_offsets; const double *path_points; };
// total: the points the call brings; the rest as MissionCheck
struct MissionPathsCheck { MissionFault fault; int64_t entry; double max_pref_speed; int64_t total; };
inline MissionPathsCheck mission_paths_check(const MissionCtx &C, const MissionArgs &A, const MissionPathArgs &P, uint8_t *reached = nullptr) {
    MissionCtx B = C;
    if (C.path_W > 0) B.paths = false;
    std::vector<uint8_t> own;
    if (!reached && A.M >= 1 && A.M <= MISSION_MAX_M && A.n == C.n && A.n > 0 && (int64_t)A.M * A.n <= MISSION_MAX_SLOTS) { own.assign((std::size_t)A.M * (std::size_t)A.n, 0); reached = own.data(); }
    const MissionCheck k = mission_check(B, A, reached);
    if (k.fault != MSF_OK && mission_error_code(k.fault) != SCA_ERR_ARG) return {k.fault, k.entry, 0.0, 0};
    if (P.path_offsets && C.path_W <= 0) return {MSF_PATH_NO_SLOTS, -1, 0.0, 0};
    if (k.fault != MSF_OK) return {k.fault, k.entry, 0.0, 0};
    if (!P.path_offsets) return {MSF_OK, -1, k.max_pref_speed, 0};
    const int64_t E = (int64_t)A.M * A.n;
    if (P.path_offsets[0] != 0) return {MSF_PATH_START, -1, 0.0, 0};
    for (int64_t e = 0; e < E; e++) if (P.path_offsets[e + 1] < P.path_offsets[e]) return {MSF_PATH_DECREASING, e, 0.0, 0};
    const int64_t total = P.path_offsets[E];
    if (total > 0 && !P.path_points) return {MSF_PATH_NO_POINTS, -1, 0.0, total};
    if (total > MISSION_PATH_MAX_POINTS) return {MSF_PATH_TOTAL, -1, 0.0, total};
    for (int64_t e = 0; e < E; e++) {
        if (!reached[e]) continue;
        const int64_t lo = P.path_offsets[e], hi = P.path_offsets[e + 1];
        if (hi - lo > C.path_W) return {MSF_PATH_TOO_LONG, e, 0.0, total};
        for (int64_t q = 3 * lo; q < 3 * hi; q++) if (!restart_finite(P.path_points[q])) return {MSF_PATH_NOT_FINITE, e, 0.0, total};
    }
    return {MSF_OK, -1, k.max_pref_speed, total};
}
// sca_get_mission_paths(points_per_agent, total_points)
inline MissionFault mission_paths_get_check(bool agents, bool on, bool have_outputs) {
    if (!agents) return MSF_NO_AGENTS;
    if (!on) return MSF_OFF;
    if (!have_outputs) return MSF_GET_ARGS;
    return MSF_OK;
}
// the getters
inline MissionFault mission_results_check(bool agents, bool on, bool have_out, int capacity, bool have_count, int struct_bytes) {
    if (!agents) return MSF_NO_AGENTS;
    if (!on) return MSF_OFF;
    if (capacity < 0 || !have_count || (capacity > 0 && !have_out) || struct_bytes != (int)sizeof(sca_mission_result)) return MSF_GET_ARGS;
    return MSF_OK;
}
inline MissionFault mission_totals_check(bool agents, bool on, bool have_out, int struct_bytes) {
    if (!agents) return MSF_NO_AGENTS;
    if (!on) return MSF_OFF;
    if (!have_out || struct_bytes != (int)sizeof(sca_mission_totals)) return MSF_GET_ARGS;
    return MSF_OK;
}
inline MissionFault mission_state_check(bool agents, bool on, int n, int begin, int count, bool have_cursor, bool have_ended) {
    if (!agents) return MSF_NO_AGENTS;
    if (!on) return MSF_OFF;
    if (begin < 0 || count < 0 || begin > n || count > n - begin || (count > 0 && (!have_cursor || !have_ended))) return MSF_GET_ARGS;
    return MSF_OK;
}

// ---- taking a mission --------------------------------------------------------------------------------------------------------------------
// A row ENDED in a step when it entered the step without any of at-goal / collision / timeout (old: the flags it entered with -- NOT the old
// record's at the end of the step, where the pass has set the collision bit of a row it served; the kernel keeps a word per row) and leaves
// K4 with one (now: d.rec_new).
SCA_HD bool mission_ended(uint32_t old_flags, uint32_t new_flags) { return !(old_flags & RSP_DONE_FLAGS) && (new_flags & RSP_DONE_FLAGS); }
enum MissionOutcome { MISSION_ARRIVED = 0, MISSION_COLLIDED = 1, MISSION_TIMED_OUT = 2 };
struct MissionTake { int outcome, next; };
// flags: an ended row's flag word.  A collision wins over an arrival, an arrival over a time-out (lifelong.run_lifelong's precedence); the
// successor is `ok` for an arrival and `fail` otherwise; -1: the row stays finished as it is.
SCA_HD MissionTake mission_take(uint32_t flags, int ok, int fail) {
    MissionTake t;
    t.outcome = (flags & FLAG_COLLISION) ? MISSION_COLLIDED : (flags & FLAG_AT_GOAL) ? MISSION_ARRIVED : MISSION_TIMED_OUT;
    t.next = t.outcome == MISSION_ARRIVED ? ok : fail;
    return t;
}
// a row has a table where either successor of the flight in the air at sca_set_missions is an entry
SCA_HD bool mission_has_table(int first_ok, int first_fail) { return first_ok >= 0 || first_fail >= 0; }

// ---- an entry as the source of a row write -------------------------------------------------------------------------------------------------
// respawn_write_row's second source (the first: the call's block, RespawnBlockSrc).  START_HERE: the position comes from the record the
// row holds (piece) and the heading is not written; the radius is always the row's.
struct MissionSrc {
    const sca_mission *e;
    SCA_HD RespawnPiece piece(int lane, const PubRec *cur) const {
        const bool here = (e->flags & SCA_MISSION_START_HERE) != 0;
        RespawnPiece q;
        if (lane == 0) { piece_put64(q, 0, here ? cur->px : e->pos[0]); piece_put64(q, 1, here ? cur->py : e->pos[1]); }
        else if (lane == 1) { piece_put64(q, 0, here ? cur->pz : e->pos[2]); q.w[2] = piece_bits32(e->vel[0]); q.w[3] = piece_bits32(e->vel[1]); }
        else { q.w[0] = piece_bits32(e->vel[2]); q.w[1] = 0u; piece_put64(q, 1, cur->radius); }      // (flags 0; the radius stays the row's)
        return q;
    }
    SCA_HD bool writes_heading() const { return !(e->flags & SCA_MISSION_START_HERE); }
    SCA_HD double heading(int k) const { return e->heading[k]; }
    SCA_HD double goal(int k) const { return e->goal[k]; }
    SCA_HD double goal_heading(int k) const { return e->goal_heading[k]; }
    SCA_HD double pref_speed() const { return e->pref_speed; }
    SCA_HD double max_run_dist() const { return e->max_run_dist; }
    SCA_HD uint8_t zaxis() const { return e->zaxis; }
};
// the `has` word and the bits byte respawn_row reads for a row taken from entry e of tables WITHOUT lists (no path word is touched)
SCA_HD uint32_t mission_has(const sca_mission &e) { return (e.flags & SCA_MISSION_KEEP_ZAXIS) ? 0u : RESPAWN_HAS_ZAXIS; }
SCA_HD uint8_t mission_bits(uint8_t policy, bool tracker_on) {      // (restart_policy_tracked's rule, for the device too)
    return tracker_on && (policy == SCA_POLICY_SCA || policy == SCA_POLICY_RVO3D_DUBINS) ? RSP_BIT_TRACKED : 0;
}
// ... and of tables WITH lists (sca_set_missions_paths in slot form): the entry brings its list as a respawn's path arrays do, and a
// straight-line row that HAD a list (old_len: len[a] in front of the take -- what the host's "straight-line agent with a list" byte mirrors,
// respawn_pack) goes back to its policy's own v_pref rule until k_waypoint_slots finds the new list not empty
SCA_HD uint32_t mission_take_has(const sca_mission &e, bool lists) { return mission_has(e) | (lists ? RESPAWN_HAS_PATH_SLOTS | RESPAWN_HAS_PATHS : 0u); }
SCA_HD uint8_t mission_take_bits(uint8_t policy, bool tracker_on, int32_t old_len) {
    const bool straight = !(policy == SCA_POLICY_SCA || policy == SCA_POLICY_RVO3D_DUBINS);
    return (uint8_t)(mission_bits(policy, tracker_on) | (straight && old_len > 0 ? RSP_BIT_MODE_RESET : 0));
}
// entry fe's list in the tables' packed CSR (off null: every entry brings the empty list)
struct MissionList { int32_t first, len; };
SCA_HD MissionList mission_list(const int32_t *off, int64_t fe) {
    MissionList l;
    l.first = off ? off[fe] : 0;
    l.len = off ? off[fe + 1] - l.first : 0;
    return l;
}
// What one lane of the wavefront that serves row `a` stores where the step takes entry e (flat index fe) for it: the shared row write with
// the entry as its source, then -- tables with lists -- the entry's list into the row's room.  old_len: len[a], loaded in front of every
// store of the row.  Dev: RespawnDev (the kernels) or plain host arrays with the same members (tests/mission_paths_harness.cpp).
template <class Dev>
SCA_HD RespawnRow mission_take_write(const Dev &d, int a, int lane, uint8_t policy, uint32_t flags, const sca_mission *e, bool lists, int32_t old_len,
                                     const int32_t *path_off, const double *path_pts, int64_t fe) {
    MissionList l = mission_list(lists ? path_off : nullptr, fe);
    if (lists && l.len > d.W) l.len = d.W;                                 // (never taken: mission_paths_check holds every reachable list against the room)
    const bool tracker_on = d.trk_st != nullptr;
    const uint8_t bits = lists ? mission_take_bits(policy, tracker_on, old_len) : mission_bits(policy, tracker_on);
    const RespawnRow w = respawn_row(bits, flags, mission_take_has(*e, lists), l.len);
    respawn_write_row(d, a, lane, w, MissionSrc{e});
    if (w.path_len > 0) respawn_write_list(d.path_pts, d.W, a, lane, path_pts + 3 * (int64_t)l.first, w.path_len);
    return w;
}

// ---- the results ---------------------------------------------------------------------------------------------------------------------------
// A row's ring holds its last R results: the result of ending number e (0-based) stands at e % R.  ended counts the endings, collected the
// value of ended at the last collect: the results not yet collected are the last min(ended - collected, R), oldest first.
SCA_HD int mission_new(uint32_t ended, uint32_t collected, int R) { const uint32_t d = ended - collected; return d < (uint32_t)R ? (int)d : R; }
SCA_HD int mission_ring_slot(uint32_t ended, int fresh, int k, int R) { return (int)((ended - (uint32_t)fresh + (uint32_t)k) % (uint32_t)R); }
constexpr int MISSION_HEAD_BYTES = 64;             // the collect's page-locked block: the count in its first word, the results behind the head
enum MissionTotal { MST_UPDATES = 0, MST_AGENT_STEPS, MST_ARRIVED, MST_COLLIDED, MST_TIMED_OUT, MST_TAKEN, MST_STOPPED, MST_WORDS = 8 };

// ---- the admission gate in front of the take ---------------------------------------------------------------------------------------------
// While a gate is set an ended row whose flight names successor j does not take it at once: it becomes a CANDIDATE for entry j.  A step's
// candidates are offered in this order: the rows WAITING since an earlier step in ascending id, then the step's NEW candidates in
// ascending id (lifelong.run_lifelong's offer order).  The first `cap` of them are tested by sca_respawn_agents_gated's rule (sca_spawn.h:
// spawn_world, spawn_entry_blocks, spawn_verdict), the others wait with SCA_SPAWN_OVER_CAP.  An admitted row is written by
// respawn_write_row; a refused row keeps every word and waits: waiting[a] = j, verdict[a] the word, refusals[a] + 1.
enum MissionGateFault {
    MGF_OK = 0,
    MGF_NO_TABLES,          // no mission tables are set                                                      } SCA_ERR_STATE
    MGF_MID_STEP,           // between a policy pass and its env update                                       }
    MGF_NEVER_SET,          // a getter while no gate has been set since the tables arrived                   }
    MGF_BAD_MARGIN,         // a margin that is negative or not finite                                        } SCA_ERR_ARG
    MGF_BAD_CAP,            // max_per_step outside 0 .. n                                                    }
    MGF_TOO_LARGE,          // the partials (spawn_tiles x cap x 32 bytes) above MISSION_GATE_MAX_SCRATCH     }
    MGF_GET_ARGS            // a getter: bad struct_bytes, range or a NULL output                             }
};
inline int mission_gate_error_code(MissionGateFault f) { return f == MGF_OK ? SCA_OK : f <= MGF_NEVER_SET ? SCA_ERR_STATE : SCA_ERR_ARG; }
constexpr int64_t MISSION_GATE_MAX_SCRATCH = (int64_t)1 << 30;
// cap: the candidates tested per step (0 asked: min(n, SPAWN_BATCH)); scratch: the partials' bytes for n agents and m obstacles
struct MissionGateCheck { MissionGateFault fault; int cap; int64_t scratch; };
SCA_HD int mission_gate_cap(int n, int32_t max_per_step) { return max_per_step > 0 ? max_per_step : n < SPAWN_BATCH ? n : SPAWN_BATCH; }
inline int64_t mission_gate_scratch(int n, int m, int cap) { return spawn_partials(n, m, cap, SPAWN_TILE) * (int64_t)sizeof(SpawnPartial); }
// sca_set_mission_gate(on, margin, max_per_step): `on` 0 reads neither the margin nor the cap
inline MissionGateCheck mission_gate_check(bool tables, bool mid_step, int n, int m, int on, double margin, int32_t max_per_step) {
    if (!tables) return {MGF_NO_TABLES, 0, 0};
    if (mid_step) return {MGF_MID_STEP, 0, 0};
    if (!on) return {MGF_OK, 0, 0};
    if (!(margin >= 0.0) || !restart_finite(margin)) return {MGF_BAD_MARGIN, 0, 0};
    if (max_per_step < 0 || max_per_step > n) return {MGF_BAD_CAP, 0, 0};
    const int cap = mission_gate_cap(n, max_per_step);
    const int64_t scratch = mission_gate_scratch(n, m, cap);
    if (scratch > MISSION_GATE_MAX_SCRATCH) return {MGF_TOO_LARGE, cap, scratch};
    return {MGF_OK, cap, scratch};
}
inline MissionGateFault mission_gate_state_check(bool tables, bool ever, int n, int begin, int count, bool have_outputs) {
    if (!tables) return MGF_NO_TABLES;
    if (!ever) return MGF_NEVER_SET;
    if (begin < 0 || count < 0 || begin > n || count > n - begin || (count > 0 && !have_outputs)) return MGF_GET_ARGS;
    return MGF_OK;
}
inline MissionGateFault mission_gate_totals_check(bool tables, bool ever, bool have_out, int struct_bytes) {
    if (!tables) return MGF_NO_TABLES;
    if (!ever) return MGF_NEVER_SET;
    if (!have_out || struct_bytes != (int)sizeof(sca_mission_gate_totals)) return MGF_GET_ARGS;
    return MGF_OK;
}
// a row's class in a step: `waiting` its waiting word behind the endings (the entry it is a candidate for, -1: none), fresh: it ended in
// this very step
enum MissionGateClass { MGC_NONE = 0, MGC_WAITING = 1, MGC_NEW = 2 };
SCA_HD int mission_gate_class(int32_t waiting, bool fresh) { return waiting < 0 ? MGC_NONE : fresh ? MGC_NEW : MGC_WAITING; }
// rank: the candidates of the same class with a lower id; waiting_total: the context's waiting candidates
SCA_HD int mission_gate_place(int cls, int rank, int waiting_total) { return cls == MGC_NEW ? waiting_total + rank : rank; }
// the candidate's sphere: the row's own radius at the entry's start, with START_HERE where the row stands now
SCA_HD ClearPoint mission_gate_query(const sca_mission &e, const PubRec &cur) {
    const bool here = (e.flags & SCA_MISSION_START_HERE) != 0;
    ClearPoint q;
    q.x = here ? cur.px : e.pos[0]; q.y = here ? cur.py : e.pos[1]; q.z = here ? cur.pz : e.pos[2]; q.r = cur.radius;
    return q;
}
// the gate's totals: the device's eight words in sca_mission_gate_totals' order; a verdict v moves word MGT_ADMITTED + v
enum MissionGateTotal { MGT_OFFERED = 0, MGT_ADMITTED, MGT_BLOCKED_AGENT, MGT_BLOCKED_OBSTACLE, MGT_BLOCKED_ENTRY, MGT_OVER_CAP, MGT_DROPPED, MGT_WORDS = 8 };
static_assert(MGT_ADMITTED + SCA_SPAWN_BLOCKED_AGENT == MGT_BLOCKED_AGENT && MGT_ADMITTED + SCA_SPAWN_BLOCKED_OBSTACLE == MGT_BLOCKED_OBSTACLE &&
              MGT_ADMITTED + SCA_SPAWN_BLOCKED_ENTRY == MGT_BLOCKED_ENTRY && MGT_ADMITTED + SCA_SPAWN_OVER_CAP == MGT_OVER_CAP, "a verdict names its counter");
static_assert(sizeof(sca_mission_gate_totals) == 8 * MGT_WORDS, "sca_mission_gate_totals is eight 64-bit counters");
// what a verdict leaves of the candidate for entry j: take -- the row is written (cursor = flying = j, live 1, its done_count stripe + 1,
// MST_TAKEN + 1); else the row keeps every word and waits.  counter: the gate's total that moves by one.
struct MissionGateSettle { int32_t waiting, verdict, refusals; int counter; bool take; };
SCA_HD MissionGateSettle mission_gate_settle(int32_t verdict, int32_t entry, int32_t refusals) {
    MissionGateSettle s;
    s.take = verdict == SCA_SPAWN_ADMITTED;
    s.waiting = s.take ? -1 : entry;
    s.verdict = verdict;
    s.refusals = s.take ? refusals : refusals + 1;
    s.counter = MGT_ADMITTED + verdict;
    return s;
}

}  // namespace sca
