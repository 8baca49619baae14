// sca_vacancy.h -- vacant rows anywhere in a plain context's id range (sca_retire_agents, sca_get_vacant, sca_get_population; a respawn
// that names a vacant row admits it), include/sca_hip.h.
//
// The reference indexes agents[agentIDs[i]] by id and has no removal in place; the library defines vacancy as the plain list edit on
// kdTree.agentIDs: retiring id a is agentIDs.remove(a), admitting it agentIDs.append(a), nothing else of the order moves.  The occupied
// rows are then, bit for bit, a context that holds only those agents renumbered in ascending id.  The permutation always reads
//   [0, m)   the occupied ids in carried order          [m, n)   the vacant ids, ascending
// and the kd build takes m for its size, so a vacant row stands in no tree and is nobody's neighbour, collision or clearance partner.
//
// Everything here is pure and compiles for the host (tests/vacancy_harness.cpp):
//   vacancy_check      every refusal of sca_retire_agents, with its code
//   vacant_row         what a retired row's scalar words become, vacate_write_row the row write k_vacate calls per lane
//   vac_pick           the predicate of the three ordered compactions of the permutation edit (VAC_KEEP, VAC_TAIL, VAC_ADMIT)
//   vacancy_compact    the tiled edit on the host, by the scan rule of sca_respawn.h (finished_offsets / finished_rank): what the
//                      kernels of sca_vacancy.hip.h do with one workgroup per tile
#pragma once
#include "sca_respawn.h"

namespace sca {

// (FLAG_VACANT = 8, sca_core.h: SCA_FLAG_VACANT)
constexpr uint32_t VACANT_FLAGS = FLAG_AT_GOAL | FLAG_COLLISION | FLAG_VACANT;   // what sca_get_state shows for a vacant row: 11
SCA_HD bool vacant_flag(uint32_t flags) { return (flags & FLAG_VACANT) != 0; }

// ---- the refusals ------------------------------------------------------------------------------------------------------------------------
enum VacancyFault {
    VCF_OK = 0,
    VCF_NO_AGENTS,          // sca_set_agents first                                                           } SCA_ERR_STATE
    VCF_NO_STATE,           // no state yet                                                                   }
    VCF_MID_STEP,           // between a policy pass and its env update                                       }
    VCF_BAD_COUNT,          // count <= 0                                                                     } SCA_ERR_ARG
    VCF_NO_IDS,             // ids is NULL                                                                    }
    VCF_BAD_ID,             // an id outside 0 .. n - 1 (entry: where)                                        }
    VCF_REPEATED_ID,        // an id named twice (entry: the later place)                                     }
    VCF_ALREADY_VACANT,     // an id that is vacant already (entry: where)                                    }
    VCF_LAST_ROW,           // the call would leave no occupied row                                           }
    VCF_LIST_ARGS,          // sca_get_vacant / sca_get_population: capacity < 0, a NULL count, NULL ids with a capacity }
    VCF_SCENES,             // scenes are set                                                                 } SCA_ERR_UNSUPPORTED
    VCF_SHARD,              // a shard with count < n                                                         }
    VCF_COMM,               // a communicator                                                                 }
    VCF_PARTITION,          // the cell-owner partition                                                       }
    VCF_PATH_BLOCK          // waypoint lists in block form                                                   }
};
inline int vacancy_error_code(VacancyFault f) {
    return f == VCF_OK ? SCA_OK : f <= VCF_MID_STEP ? SCA_ERR_STATE : f <= VCF_LIST_ARGS ? SCA_ERR_ARG : SCA_ERR_UNSUPPORTED;
}
struct VacancyCheck { VacancyFault fault; int entry; };
// the context-wide part: what sca_respawn_agents refuses, under this call's own codes (mid_step: the getters may run there)
inline VacancyFault vacancy_context_check(const RespawnCtx &C, bool changes) {
    if (!C.agents) return VCF_NO_AGENTS;
    if (!C.state) return VCF_NO_STATE;
    if (changes && C.mid_step) return VCF_MID_STEP;
    if (C.scenes) return VCF_SCENES;
    if (C.comm) return VCF_COMM;
    if (C.partition) return VCF_PARTITION;
    if (C.shard_count < C.n) return VCF_SHARD;
    if (changes && C.paths_block) return VCF_PATH_BLOCK;
    return VCF_OK;
}
// sca_retire_agents(count, ids).  vacant: [n] 1 where the row is vacant now, null: no row is; occupied: the rows that are not
inline VacancyCheck vacancy_check(const RespawnCtx &C, const uint8_t *vacant, int occupied, int count, const int32_t *ids) {
    if (const VacancyFault f = vacancy_context_check(C, true)) return {f, -1};
    if (count <= 0) return {VCF_BAD_COUNT, -1};
    if (!ids) return {VCF_NO_IDS, -1};
    for (int r = 0; r < count; r++) if (ids[r] < 0 || ids[r] >= C.n) return {VCF_BAD_ID, r};
    {   // (the (id, place) pairs sorted, as respawn_check finds a repeated id: time that grows with the call, not with the swarm)
        std::vector<std::pair<int32_t, int>> s((std::size_t)count);
        for (int r = 0; r < count; r++) s[(std::size_t)r] = {ids[r], r};
        std::sort(s.begin(), s.end());
        int at = -1;
        for (int k = 1; k < count; k++) if (s[(std::size_t)k].first == s[(std::size_t)k - 1].first && (at < 0 || s[(std::size_t)k].second < at)) at = s[(std::size_t)k].second;
        if (at >= 0) return {VCF_REPEATED_ID, at};
    }
    if (vacant) for (int r = 0; r < count; r++) if (vacant[ids[r]]) return {VCF_ALREADY_VACANT, r};
    if (count >= occupied) return {VCF_LAST_ROW, -1};                  // m >= 1 always: k_kd_gather's first workgroup also resets the step's counters
    return {VCF_OK, -1};
}
// sca_get_vacant(ids, capacity, count)
inline VacancyFault vacant_list_check(const RespawnCtx &C, bool have_ids, int capacity, bool have_count) {
    if (!C.agents) return VCF_NO_AGENTS;
    if (!C.state) return VCF_NO_STATE;
    if (capacity < 0 || !have_count || (capacity > 0 && !have_ids)) return VCF_LIST_ARGS;
    return vacancy_context_check(C, false);
}

// ---- one row -----------------------------------------------------------------------------------------------------------------------------
// The scalar words of a retired row, by the rule scene_restart_vacate and collide_finish_body already have: settled for good (at-goal |
// collision) plus the vacant bit, so every policy kernel skips it, K4 never traverses for it and cannot add a flag (total_dist 0 never
// passes max_run_dist), the integrate stage leaves its position and a zero heading, the tracker does not own it (tracker_owns wants
// flags 0).  done_delta: K4's striped done_count counts the rows that are not done -- a row that was live leaves it, the restart's rule.
// path_len: slot form: len = rem = 0, now_goal None; -1: no slot form, nothing written.  Kept: position, radius, goal, pref_speed,
// max_run_dist, policy, zaxis, the v_pref mode and the fed v_pref, the solver and planner attributes, the tracker record.
struct VacantRow {
    double total_dist;
    uint32_t flags;
    int32_t step_num, status, nbr_n, near_n, done_delta, path_len, diag;
    uint8_t nbr_valid;
};
SCA_HD VacantRow vacant_row(uint32_t old_flags, bool slots) {
    VacantRow w;
    w.total_dist = 0.0;
    w.flags = VACANT_FLAGS;
    w.step_num = 0; w.status = 0; w.nbr_n = 0; w.near_n = -1;
    w.done_delta = (old_flags & RSP_DONE_FLAGS) ? 0 : -1;
    w.path_len = slots ? 0 : -1;
    w.diag = -1;
    w.nbr_valid = 0;
    return w;
}
// What one lane of the wavefront that serves row `a` stores (lane 0 .. 63):
//   public record     16-byte pieces 1 and 2 by lanes 1 and 2, read, changed and stored whole: piece 1 holds pz | vx vy, piece 2 vz | flags |
//                     radius; piece 0 (px, py) stays
//   three-component   heading 0 (now_goal None in slot form): one component per lane 0 .. 2
//   action row        zero, lanes 0 .. 6; diag -1, lanes 0 .. 7
//   scalar fields     lane 0
// Dev: RespawnDev (sca_respawn.hip.h) plus action and diag; plain host arrays in the tests' harness.  Not here: the done_count stripe.
static_assert(offsetof(PubRec, pz) == 16 && offsetof(PubRec, vx) == 24 && offsetof(PubRec, vz) == 32 && offsetof(PubRec, flags) == 36 && offsetof(PubRec, radius) == 40,
              "vacate_write_row edits the record's second and third 16-byte piece");
// the outputs of the last pass, which no later pass writes for a vacant row (lanes 0 .. 7): vacate_write_row's part that a context
// checkpoint's load repeats for the vacant rows of its blob (sca_checkpoint.h: the outputs are not in a blob).  Dev: action, diag, nbr_n,
// nbr_valid, near_n
template <class Dev>
SCA_HD void vacate_write_outputs(const Dev &d, int64_t a, int lane, const VacantRow &w) {
    if (lane < 7) d.action[8 * a + lane] = 0.0f;
    if (lane < 8) d.diag[8 * a + lane] = w.diag;
    if (lane == 0) { d.nbr_n[a] = w.nbr_n; d.nbr_valid[a] = w.nbr_valid; d.near_n[a] = w.near_n; }
}
template <class Dev>
SCA_HD void vacate_write_row(const Dev &d, int a, int lane, const VacantRow &w) {
    if (lane == 1 || lane == 2) {
        RespawnPiece *p = (RespawnPiece *)(d.rec + a) + lane;
        RespawnPiece q = *p;
        if (lane == 1) { q.w[2] = 0u; q.w[3] = 0u; }                   // vx, vy
        else { q.w[0] = 0u; q.w[1] = w.flags; }                        // vz, flags
        *p = q;
    }
    if (lane < 3) {
        const int64_t g = 3 * (int64_t)a + lane;
        d.heading[g] = 0.0;
        if (w.path_len >= 0 && d.now_goal) d.now_goal[g] = __builtin_nan("");
    }
    vacate_write_outputs(d, (int64_t)a, lane, w);
    if (lane == 0) {
        d.total_dist[a] = w.total_dist; d.step_num[a] = w.step_num; d.status[a] = w.status;
        if (w.path_len >= 0 && d.path_len) { d.path_len[a] = w.path_len; d.path_rem[a] = w.path_len; }
        if (d.clear) d.clear[a] = scene_clearance_empty();
    }
}

// ---- the permutation edit ------------------------------------------------------------------------------------------------------------------
// Three ordered compactions, each over `items` consecutive items cut into tiles (one workgroup each on the device), by sca_get_finished's
// rule: a count per tile, finished_offsets over the counts, a picked item at its tile's offset + its rank in the tile.  No atomic cursor:
// the order IS the contract.
//   VAC_KEEP    item p: position p < m of the permutation; picked where its id is not vacant; writes the id   (the stable deletion of a retire)
//   VAC_TAIL    item a: id a < n; picked where the row is vacant; writes the id                                 (the ascending vacant tail)
//   VAC_ADMIT   item r: named row r < count of a respawn; picked where ids[r] is vacant and the gated call's verdict (null: every row)
//               admits it; writes the id                                                                        (the append, in call order)
// The flags are read as they stand when the compaction runs: VAC_KEEP and VAC_TAIL behind k_vacate, VAC_ADMIT in front of k_respawn (which
// clears the admitted rows' vacant bit) and the VAC_TAIL of an admission behind it.
enum VacMode : int { VAC_KEEP = 0, VAC_TAIL, VAC_ADMIT };
struct VacView {
    const PubRec *rec;          // [n]
    const int32_t *perm;        // [n] VAC_KEEP reads [0, m)
    const int32_t *ids;         // [count] VAC_ADMIT
    const int32_t *verdict;     // [count] VAC_ADMIT, nullable
    int n, m, count;
};
SCA_HD int vac_items(const VacView &v, int mode) { return mode == VAC_KEEP ? v.m : mode == VAC_TAIL ? v.n : v.count; }
SCA_HD bool vac_pick(const VacView &v, int mode, int item, int32_t &id) {
    id = -1;
    if (item >= vac_items(v, mode)) return false;
    if (mode == VAC_TAIL) { id = item; return vacant_flag(v.rec[item].flags); }
    id = mode == VAC_KEEP ? v.perm[item] : v.ids[item];
    if (id < 0 || id >= v.n) return false;                             // (a permutation holds ids, and the host has checked the call's: never taken)
    if (mode == VAC_KEEP) return !vacant_flag(v.rec[id].flags);
    return vacant_flag(v.rec[id].flags) && !(v.verdict && v.verdict[item] != 0);
}
inline int vac_tiles(int items, int tile) { return (items + tile - 1) / tile; }
// The tiled compaction on the host: out[base + place] = id for the picked items, in item order; returns how many.  TILE: a multiple of 64.
// A tile's wavefronts are its groups of 64 consecutive items; an item's place is offsets[tile] + the picks of the tile's earlier
// wavefronts + finished_rank inside its own -- word for word what k_vac_count / k_finished_scan / k_vac_write compute.
template <int TILE>
inline int vacancy_compact(const VacView &v, int mode, int32_t *out, int base) {
    static_assert(TILE % 64 == 0, "a tile is whole wavefronts");
    const int items = vac_items(v, mode), tiles = vac_tiles(items, TILE);
    std::vector<int32_t> counts((std::size_t)tiles + 1, 0), offsets((std::size_t)tiles + 1, 0);
    auto ballot = [&](int first, int32_t *ids) {
        unsigned long long mask = 0ull;
        for (int l = 0; l < 64; l++) if (vac_pick(v, mode, first + l, ids[l])) mask |= 1ull << l;
        return mask;
    };
    int32_t ids[64];
    for (int t = 0; t < tiles; t++)
        for (int w = 0; w < TILE / 64; w++) counts[(std::size_t)t] += __builtin_popcountll(ballot(t * TILE + 64 * w, ids));
    const int total = finished_offsets(counts.data(), tiles, offsets.data());
    for (int t = 0; t < tiles; t++) {
        int before = 0;
        for (int w = 0; w < TILE / 64; w++) {
            const unsigned long long mask = ballot(t * TILE + 64 * w, ids);
            for (int l = 0; l < 64; l++) if ((mask >> l) & 1ull) out[base + offsets[(std::size_t)t] + before + finished_rank(mask, l)] = ids[l];
            before += __builtin_popcountll(mask);
        }
    }
    return total;
}

}  // namespace sca
