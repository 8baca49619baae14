// sca_spawn.h -- spawn admission: how free is a point now (sca_probe_clearance) and respawning only the rows whose start is free
// (sca_respawn_agents_gated), include/sca_hip.h.
//
// The probe is the closest-approach rule (sca_scenes.h: clearance_pair; sca_clearance.h: clearance_member, clearance_better) for arbitrary
// spheres BETWEEN two steps, against the records as they are now: query q keeps the smallest c = l3norm(p_q, p_b) - (r_q + r_b) over every
// agent row b but ignore[q], the lowest b on equal values, and the same over the obstacles in set order.  The search is brute force over
// the records on purpose -- between two steps the agent tree has no known age and the grid mode has none -- cut into tiles so that the
// minimum on (c, id), which is associative and commutative, is formed in any order with the same result.
//
// Everything here is pure and compiles for the host (tests/spawn_harness.cpp); the kernels of sca_spawn.hip.h call these very functions:
//   spawn_check         every refusal of the two entry points' own arguments, with its code (the context-wide part is respawn_context_check)
//   spawn_tiles         the tiling of the partners (agents first, then obstacles) and spawn_partial_index, a partial's place
//   spawn_tile_partial  one lane's walk over one slice of a tile: its query against the staged partners
//   spawn_fold          the tiles' partials into the record, spawn_world the world test's verdict of a record
//   spawn_entry_blocks  the entry test's pair, spawn_gate_walk one lane's share of the earlier rows (k_spawn_gate runs it strided), spawn_verdict
#pragma once
#include "sca_clearance.h"
#include "sca_respawn.h"

namespace sca {

// ---- the refusals ------------------------------------------------------------------------------------------------------------------------
enum SpawnFault {
    SPF_OK = 0,
    SPF_NO_AGENTS,          // sca_set_agents first                                                           } SCA_ERR_STATE
    SPF_NO_STATE,           // no state yet                                                                   }
    SPF_MID_STEP,           // between a policy pass and its env update                                       }
    SPF_BAD_COUNT,          // count <= 0                                                                     } SCA_ERR_ARG
    SPF_NO_ARRAYS,          // pos, radius or out is NULL                                                     }
    SPF_NOT_FINITE,         // a position that is not finite (entry: the query)                               }
    SPF_BAD_RADIUS,         // a radius that is negative or not finite (0 is a point probe)                   }
    SPF_BAD_IGNORE,         // an ignore outside -1 .. n - 1                                                  }
    SPF_BAD_STRUCT,         // struct_bytes is not sizeof(sca_scene_clearance)                                }
    SPF_BAD_MARGIN,         // gated respawn: a margin that is negative or not finite                         }
    SPF_NO_VERDICT,         // gated respawn: verdict is NULL                                                 }
    SPF_SCENES,             // scenes are set                                                                 } SCA_ERR_UNSUPPORTED
    SPF_SHARD,              // a shard with count < n                                                         }
    SPF_COMM,               // a communicator                                                                 }
    SPF_PARTITION           // the cell-owner partition                                                       }
};
inline int spawn_error_code(SpawnFault f) { return f == SPF_OK ? SCA_OK : f <= SPF_MID_STEP ? SCA_ERR_STATE : f <= SPF_NO_VERDICT ? SCA_ERR_ARG : SCA_ERR_UNSUPPORTED; }
struct SpawnCheck { SpawnFault fault; int entry; };
inline SpawnFault spawn_context_fault(RespawnFault f) {
    switch (f) {
    case RSP_OK: return SPF_OK;
    case RSP_NO_AGENTS: return SPF_NO_AGENTS;
    case RSP_NO_STATE: return SPF_NO_STATE;
    case RSP_MID_STEP: return SPF_MID_STEP;
    case RSP_SCENES: return SPF_SCENES;
    case RSP_COMM: return SPF_COMM;
    case RSP_PARTITION: return SPF_PARTITION;
    default: return SPF_SHARD;
    }
}
// sca_probe_clearance(count, pos, radius, ignore, out, struct_bytes)
inline SpawnCheck spawn_check(const RespawnCtx &C, int count, const double *pos, const double *radius, const int32_t *ignore, bool have_out, int struct_bytes) {
    if (const RespawnFault f = respawn_context_check(RSP_CALL_RESPAWN, C)) return {spawn_context_fault(f), -1};
    if (count <= 0) return {SPF_BAD_COUNT, -1};
    if (!pos || !radius || !have_out) return {SPF_NO_ARRAYS, -1};
    for (int q = 0; q < count; q++)
        for (int k = 0; k < 3; k++) if (!restart_finite(pos[3 * (int64_t)q + k])) return {SPF_NOT_FINITE, q};
    for (int q = 0; q < count; q++) if (!(radius[q] >= 0.0) || !restart_finite(radius[q])) return {SPF_BAD_RADIUS, q};
    if (ignore) for (int q = 0; q < count; q++) if (ignore[q] < -1 || ignore[q] >= C.n) return {SPF_BAD_IGNORE, q};
    if (struct_bytes != (int)sizeof(sca_scene_clearance)) return {SPF_BAD_STRUCT, -1};
    return {SPF_OK, -1};
}
// what sca_respawn_agents_gated adds to respawn_check
inline SpawnFault spawn_gate_check(double margin, bool have_verdict) {
    if (!(margin >= 0.0) || !restart_finite(margin)) return SPF_BAD_MARGIN;
    if (!have_verdict) return SPF_NO_VERDICT;
    return SPF_OK;
}

// ---- the tiling --------------------------------------------------------------------------------------------------------------------------
// The partners are the n agent rows followed by the m obstacles, global index g: an agent where g < n (id g), else obstacle g - n.  They
// are cut into tiles of P consecutive partners, the queries into chunks of SPAWN_CHUNK (one query per lane of a wavefront).  A workgroup
// of SPAWN_WAVES wavefronts takes one (tile, chunk): it stages the tile once, wavefront w walks slice w of it (P / SPAWN_WAVES partners)
// for the chunk's queries, and the wavefronts' results are folded before the one partial per (tile, query) is stored.  A call with more
// than SPAWN_BATCH queries runs the probe and the fold once per batch over the same partials.
constexpr int SPAWN_CHUNK = 64;
constexpr int SPAWN_WAVES = 4;
constexpr int SPAWN_TILE = 512;                        // P of the library (DESIGN.md has the reason); the rule holds for any P > 0
static_assert(SPAWN_TILE % SPAWN_WAVES == 0, "a tile is cut into one slice per wavefront");
constexpr int SPAWN_BATCH = 4096;                      // queries per launch: the partials hold tiles x min(room, SPAWN_BATCH) records however many a call brings
SCA_SCENES_HD int spawn_tiles(int n, int m, int P) { return (int)(((int64_t)n + m + P - 1) / P); }
SCA_SCENES_HD int spawn_chunks(int count) { return (count + SPAWN_CHUNK - 1) / SPAWN_CHUNK; }
SCA_SCENES_HD int64_t spawn_partial_index(int tile, int query, int cap) { return (int64_t)tile * cap + query; }
// a staged partner's id: the agent row or the obstacle's place in the set
SCA_SCENES_HD int32_t spawn_partner_id(int64_t g, int n) { return (int32_t)(g < n ? g : g - n); }
// what the staging puts in the place of a vacant row's id (sca_vacancy.h): spawn_tile_partial passes over it, so a vacant row is nobody's partner
constexpr int32_t SPAWN_VACANT_ID = INT32_MIN;

// One query's running minimum, both halves: what a lane holds in registers and what a partial stores (32 bytes, the record's own layout
// with the step words unused).
struct SpawnPartial { ClearBest agent, obs; };
SCA_SCENES_HD SpawnPartial spawn_partial_none() { SpawnPartial p; p.agent = clearance_none(); p.obs = clearance_none(); return p; }
SCA_SCENES_HD void spawn_merge(ClearBest &into, const ClearBest &x) { if (clearance_better(x.c, x.id, into.c, into.id)) into = x; }
SCA_SCENES_HD void spawn_merge(SpawnPartial &into, const SpawnPartial &x) { spawn_merge(into.agent, x.agent); spawn_merge(into.obs, x.obs); }

// One lane's walk: the partners staged at pts[j] / ids[j] for j = begin .. end - 1 are the global partners g0 + j.  clearance_member with
// the running best as the limit takes the exact rounding only for a pair that can still win; clearance_better keeps the lowest id on equal
// values, whatever the order the tiles and slices are folded in.
template <class Norm>
SCA_SCENES_HD void spawn_tile_partial(const ClearPoint &q, int32_t ignore, const ClearPoint *pts, const int32_t *ids, int begin, int end, int64_t g0, int n,
                                      SpawnPartial &acc, Norm norm) {
    for (int j = begin; j < end; j++) {
        const int32_t id = ids[j];
        if (g0 + j < n) {
            if (id == ignore || id == SPAWN_VACANT_ID) continue;
            spawn_merge(acc.agent, clearance_member(q, pts[j], id, acc.agent.c, norm));
        } else {
            spawn_merge(acc.obs, clearance_member(q, pts[j], id, acc.obs.c, norm));
        }
    }
}
// the record of a query from its folded minimum: both step fields 0, an empty half +inf, -1, 0
SCA_SCENES_HD sca_scene_clearance spawn_record(const SpawnPartial &p) {
    sca_scene_clearance r = scene_clearance_empty();
    if (p.agent.id != CLEAR_NO_ID) { r.agent_clear = p.agent.c; r.agent_partner = p.agent.id; }
    if (p.obs.id != CLEAR_NO_ID) { r.obs_clear = p.obs.c; r.obs_partner = p.obs.id; }
    return r;
}
// the tiles' partials of one query, [tile][query] with `cap` queries of room per tile
SCA_SCENES_HD sca_scene_clearance spawn_fold(const SpawnPartial *partials, int tiles, int query, int cap) {
    SpawnPartial acc = spawn_partial_none();
    for (int t = 0; t < tiles; t++) spawn_merge(acc, partials[spawn_partial_index(t, query, cap)]);
    return spawn_record(acc);
}

// ---- the admission rule ------------------------------------------------------------------------------------------------------------------
// (the verdict values are include/sca_hip.h's SCA_SPAWN_*)
// the world test: neither half at or below the margin; an empty half (+inf) never blocks
SCA_SCENES_HD int32_t spawn_world(const sca_scene_clearance &r, double margin) {
    return r.agent_clear <= margin ? SCA_SPAWN_BLOCKED_AGENT : r.obs_clear <= margin ? SCA_SPAWN_BLOCKED_OBSTACLE : SCA_SPAWN_ADMITTED;
}
// The entry test's pair: c = l3norm(p_a, p_b) - (r_a + r_b) <= margin.  The exact rounding is taken only where it can decide, by
// clearance_pair's own filter: with t = margin + rs + 2e-5, |a - b|^2 > t^2 means l3norm > margin + rs + 1e-5, so c > margin.
template <class Norm>
SCA_SCENES_HD bool spawn_entry_blocks(const ClearPoint &a, const ClearPoint &b, double margin, Norm norm) {
    const double rs = a.r + b.r;
    const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    double s = dx * dx + dy * dy;
    s = s + dz * dz;
    const double t = margin + rs + 2e-5;
    if (s > t * t) return false;
    return norm(a.x, a.y, a.z, b.x, b.y, b.z) - rs <= margin;
}
// One row of the call: blocked by the world as spawn_world says, else by any EARLIER row of the call that is world-clear (world[r'] == 0)
// and within the margin of it -- an earlier row the world blocked blocks nobody.  first / stride: the rows r' = first, first + stride, ...
// below r (a lane's share on the device, 0 / 1 for the whole walk); returns whether any of them blocks.
template <class Norm>
SCA_SCENES_HD bool spawn_gate_walk(const ClearPoint *rows, const int32_t *world, int r, double margin, int first, int stride, Norm norm) {
    bool blocked = false;
    const ClearPoint me = rows[r];
    for (int k = first; k < r; k += stride)
        if (world[k] == SCA_SPAWN_ADMITTED && spawn_entry_blocks(me, rows[k], margin, norm)) blocked = true;
    return blocked;
}
SCA_SCENES_HD int32_t spawn_verdict(int32_t world, bool entry_blocked) { return world != SCA_SPAWN_ADMITTED ? world : entry_blocked ? SCA_SPAWN_BLOCKED_ENTRY : SCA_SPAWN_ADMITTED; }

// ---- the block and the scratch ------------------------------------------------------------------------------------------------------------
// The page-locked block of the two calls, sized for `cap` queries: the queries go in (the point and radius as a ClearPoint, the ignore
// word), the records and the verdict words come back.  Sections aligned to 64 bytes, as the respawn block's are.
enum SpawnSection : int { SPB_QUERY = 0, SPB_IGNORE, SPB_OUT, SPB_VERDICT, SPB_SECTIONS };
struct SpawnLayout { int64_t off[SPB_SECTIONS]; int64_t total; };
inline int64_t spawn_section_bytes(int s, int cap) { return (s == SPB_QUERY || s == SPB_OUT ? 32 : 4) * (int64_t)cap; }
inline SpawnLayout spawn_layout(int cap) {
    SpawnLayout L;
    int64_t at = 0;
    for (int s = 0; s < SPB_SECTIONS; s++) {
        L.off[s] = at;
        at += (spawn_section_bytes(s, cap) + RSP_ALIGN - 1) / RSP_ALIGN * RSP_ALIGN;
    }
    L.total = at;
    return L;
}
static_assert(sizeof(ClearPoint) == 32 && sizeof(SpawnPartial) == 32, "a query and a partial are two 16-byte pieces each");
// the caller's arrays into the block's query sections
inline void spawn_pack(uint8_t *blk, const SpawnLayout &L, int count, const double *pos, const double *radius, const int32_t *ignore) {
    ClearPoint *q = (ClearPoint *)(blk + L.off[SPB_QUERY]);
    int32_t *ig = (int32_t *)(blk + L.off[SPB_IGNORE]);
    for (int k = 0; k < count; k++) {
        q[k].x = pos[3 * (int64_t)k]; q[k].y = pos[3 * (int64_t)k + 1]; q[k].z = pos[3 * (int64_t)k + 2]; q[k].r = radius[k];
        ig[k] = ignore ? ignore[k] : -1;
    }
}
// the partials a launch of `cap` queries against n + m partners needs, in records of 32 bytes
inline int64_t spawn_partials(int n, int m, int cap, int P) { return (int64_t)spawn_tiles(n, m, P) * cap; }
// a call's queries go through the kernels in batches of at most SPAWN_BATCH, all behind the call's one synchronisation
SCA_SCENES_HD int spawn_batch_room(int cap) { return cap < SPAWN_BATCH ? cap : SPAWN_BATCH; }

}  // namespace sca
