// sca_respawn.hip.h -- the kernels behind sca_respawn_agents and sca_get_finished (the rules: sca_respawn.h).  Launched on the context's
// stream only by those two entry points: a context that never calls them enqueues exactly what it did.
#pragma once
#include "sca_kernels.hip.h"
#include "sca_scenes.hip.h"
#include "sca_respawn.h"
#include "sca_respawn_attrs.h"

namespace sca {

// ---- respawning agents in place ----------------------------------------------------------------------------------------------------------
// One WAVEFRONT per named row; the call's arrays are read across the link from the library's page-locked block (RespawnLayout), as
// k_scene_restart reads its own.  Afterwards every per-agent word of the row that a later pass READS BEFORE IT WRITES is what
// sca_set_agents + sca_set_state (+ sca_device_tracker_enable) leave for an agent with the call's values; words of other rows are not
// touched, the kd permutation neither.  The one shared word written is the row's stripe of K4's done_count (the only atomic).
//   public record     three 16-byte pieces by lanes 0 .. 2 (restart_piece)
//   AgentTrack        consecutive 4-byte words by consecutive lanes from the one initial record (tracked rows under the device tracker)
//   three-component   heading, goal (goal_heading, vpref_ext, now_goal): one component per lane 0 .. 2
//   scalar fields     lane 0, plain vector stores (respawn_row says which and what)
//   waypoints         consecutive lanes on consecutive coordinates into the row's own room pts[3 (W a + j)] (respawn_write_list, sca_respawn.h)
// Null device pointers (no tracker, no lists, no closest-approach records) are skipped by a uniform branch.
// Not written, as under a scene restart: action, diag, vpref_used, vpost, is_fb, prep, coll_new, nbr_id, nbr_dsq, near_id, the kd nodes --
// a pass writes each of them for every agent it serves before anybody reads it.
struct RespawnDev {
    PubRec *rec;
    double *heading, *goal, *pref_speed, *max_run_dist, *total_dist, *vpref_ext;
    int32_t *step_num, *status, *nbr_n, *near_n, *done_count;
    uint8_t *zaxis, *vpref_mode, *nbr_valid;
    // the device tracker's, null without one
    double *trk_nbr0, *trk_goal_heading;
    restart_u32 *trk_st;
    const restart_u32 *trk_init;
    int trk_words;
    // the lists in slot form, null otherwise
    double *path_pts, *now_goal;
    int32_t *path_len, *path_rem;
    int W;
    sca_scene_clearance *clear;     // the closest-approach records (sca_clearance_enable), null: off
    int n;
};
constexpr int RESPAWN_WAVES = 4;
// verdict (nullable): the gated call's word per named row (sca_spawn.h) -- a row whose word is not 0 returns before it touches anything,
// its done_count stripe included; null: every named row is written.
__global__ __launch_bounds__(RESPAWN_WAVES * 64) void k_respawn(RespawnDev d, const uint8_t *blk, RespawnLayout L, uint32_t has, int count, const int32_t *verdict) {
    const int lane = (int)threadIdx.x & 63;
    const int r = (int)blockIdx.x * RESPAWN_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);     // wave-uniform
    if (r >= count) return;
    if (verdict && verdict[r] != 0) return;                            // (wave-uniform: one row per wavefront)
    const int a = ((const int32_t *)(blk + L.off[RSB_IDS]))[r];
    if (a < 0 || a >= d.n) return;                                     // (the host has checked the ids: never taken)
    const bool lists = (has & RESPAWN_HAS_PATHS) != 0;
    const int32_t *poff = (const int32_t *)(blk + L.off[RSB_PATH_OFF]);
    const int32_t first = lists ? poff[r] : 0, len = lists ? poff[r + 1] - first : 0;
    const uint32_t old_flags = d.rec[a].flags;
    const RespawnRow w = respawn_row((blk + L.off[RSB_BITS])[r], old_flags, has, len);
    // K4's counters of the last step, before the record is replaced: a row that was done runs again (sca_active_count between steps)
    if (lane == 0 && w.done_delta) atomicAdd(&d.done_count[(a & 255) * 32], w.done_delta);
    respawn_write_row(d, a, lane, w, RespawnBlockSrc{blk, L, r});      // (sca_respawn.h: the row write k_mission_advance shares)
    if (w.path_len > 0 && d.path_pts)                                // the row's list into its own room
        respawn_write_list(d.path_pts, d.W, a, lane, (const double *)(blk + L.off[RSB_PATH_PTS]) + 3 * (int64_t)first, w.path_len);
}

// ---- a respawn that brings the agent's own policy and attributes (sca_respawn_agents_attrs, sca_respawn_agents_gated_attrs) ---------------
// k_respawn's launch shape and row rule (the same shared functions, so that the two cannot drift apart), and beside them, from a second
// page-locked block (RespawnAttrLayout, sca_respawn_attrs.h): the row's policy byte, its 64-byte AgentPar record as four 16-byte pieces by
// lanes 0 .. 3, its neighborDist in the tracker's array, its planner triple by lanes 0 .. 2 and its class byte, and for a row that
// leaves the tracked policies under the device tracker what k_scene_restart leaves there (vpref_ext 0, the initial AgentTrack; vpref_mode 0 by RSP_BIT_MODE_RESET).  Plain vector stores; no LDS, no
// scratch, and the done_count stripe stays the one atomic.  A kernel of its own rather than a nullable argument of k_respawn: that kernel,
// and with it every context that never brings attributes, stays instruction for instruction what it was.
struct RespawnAttrDev {
    uint8_t *policy;                // [n] DeviceView::policy
    AgentPar *ap;                   // [n] DeviceView::ap
    double *ap_nd;                  // [n] TrackView::nd_per_agent
    double *trk_R, *trk_plo, *trk_phi;   // [n] TrackView::R_pa / plo_pa / phi_pa (read only with RESPAWN_HAS_PLANNER)
    uint8_t *trk_cls;               // [n] TrackView::cls
};
__global__ __launch_bounds__(RESPAWN_WAVES * 64) void k_respawn_attrs(RespawnDev d, RespawnAttrDev at, const uint8_t *blk, RespawnLayout L, const uint8_t *ablk,
                                                                      RespawnAttrLayout AL, uint32_t has, int count, const int32_t *verdict) {
    const int lane = (int)threadIdx.x & 63;
    const int r = (int)blockIdx.x * RESPAWN_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);     // wave-uniform
    if (r >= count) return;
    if (verdict && verdict[r] != 0) return;                            // a refused row keeps every word, policy and attributes included
    const int a = ((const int32_t *)(blk + L.off[RSB_IDS]))[r];
    if (a < 0 || a >= d.n) return;                                     // (the host has checked the ids: never taken)
    const bool lists = (has & RESPAWN_HAS_PATHS) != 0;
    const int32_t *poff = (const int32_t *)(blk + L.off[RSB_PATH_OFF]);
    const int32_t first = lists ? poff[r] : 0, len = lists ? poff[r + 1] - first : 0;
    const uint32_t old_flags = d.rec[a].flags;
    const uint8_t bits = (blk + L.off[RSB_BITS])[r];
    const RespawnRow w = respawn_row(bits, old_flags, has, len);
    if (lane == 0 && w.done_delta) atomicAdd(&d.done_count[(a & 255) * 32], w.done_delta);
    respawn_write_row(d, a, lane, w, RespawnBlockSrc{blk, L, r});
    respawn_attrs_write_row(d, at, a, lane, bits, has, RespawnAttrSrc{ablk, AL, r});
    if (w.path_len > 0 && d.path_pts)
        respawn_write_list(d.path_pts, d.W, a, lane, (const double *)(blk + L.off[RSB_PATH_PTS]) + 3 * (int64_t)first, w.path_len);
}

// ---- the finished list -------------------------------------------------------------------------------------------------------------------
// The ordered compaction of sca_respawn.h in three launches: a count per tile (ballot and popcount per wavefront, the wavefronts' counts
// summed in LDS), the scan of the counts by one workgroup (finished_offsets' rule: an exclusive prefix sum, the total behind it), and the
// write -- every tile recomputes its ballots, a finished row stands at its tile's offset + the finished rows of the tile's earlier
// wavefronts + finished_rank inside its own, and the first `capacity` rows go into the page-locked block as 48-byte rows.  No atomics.
struct FinishedDev {
    const PubRec *rec;
    const double *total_dist;
    const int32_t *step_num;
    int32_t *counts, *offsets;      // [tiles]
    int n, tiles;
};
static_assert(FIN_TILE == 256, "k_finished_* run four wavefronts per tile");
__device__ __forceinline__ unsigned long long finished_ballot(const FinishedDev &f, int row, uint32_t &flags) {
    flags = row < f.n ? f.rec[row].flags : 0u;
    return __ballot(finished_listed(flags));
}
__global__ __launch_bounds__(FIN_TILE) void k_finished_count(FinishedDev f) {
    __shared__ int32_t wsum[FIN_TILE / 64];
    const int t = (int)threadIdx.x, row = (int)blockIdx.x * FIN_TILE + t;
    uint32_t flags;
    const unsigned long long mask = finished_ballot(f, row, flags);
    if ((t & 63) == 0) wsum[t >> 6] = __popcll(mask);
    __syncthreads();
    if (t == 0) f.counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
// one workgroup: the tiles in chunks of FIN_TILE, a running carry between the chunks; head[0] = the total
__global__ __launch_bounds__(FIN_TILE) void k_finished_scan(FinishedDev f, int32_t *head) {
    __shared__ int32_t part[FIN_TILE];
    __shared__ int32_t carry;
    const int t = (int)threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < f.tiles; base += FIN_TILE) {
        const int i = base + t;
        const int32_t mine = i < f.tiles ? f.counts[i] : 0;
        part[t] = mine;
        __syncthreads();
        for (int step = 1; step < FIN_TILE; step <<= 1) {              // inclusive scan of the chunk
            const int32_t add = t >= step ? part[t - step] : 0;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        if (i < f.tiles) f.offsets[i] = carry + part[t] - mine;
        __syncthreads();
        if (t == FIN_TILE - 1) carry += part[t];
        __syncthreads();
    }
    if (t == 0) head[0] = carry;
}
constexpr int FIN_HEAD_BYTES = 64;                                     // the block: the count in its first word, the rows behind the head
__global__ __launch_bounds__(FIN_TILE) void k_finished_write(FinishedDev f, uint8_t *blk, int capacity) {
    __shared__ int32_t wsum[FIN_TILE / 64];
    const int t = (int)threadIdx.x, row = (int)blockIdx.x * FIN_TILE + t, wave = t >> 6;
    uint32_t flags;
    const unsigned long long mask = finished_ballot(f, row, flags);
    if ((t & 63) == 0) wsum[wave] = __popcll(mask);
    __syncthreads();
    if (!finished_listed(flags)) return;
    int at = f.offsets[blockIdx.x] + finished_rank(mask, t & 63);
    for (int k = 0; k < wave; k++) at += wsum[k];
    if (at >= capacity) return;
    const PubRec me = f.rec[row];
    sca_finished_row out;
    out.id = row; out.flags = flags; out.step_num = f.step_num[row]; out.reserved = 0;
    out.total_dist = f.total_dist[row];
    out.pos[0] = me.px; out.pos[1] = me.py; out.pos[2] = me.pz;
    ((sca_finished_row *)(blk + FIN_HEAD_BYTES))[at] = out;
}

}  // namespace sca
