// sca_vacancy.hip.h -- the kernels behind sca_retire_agents, sca_get_vacant and the admission of vacant rows by a respawn (the rules:
// sca_vacancy.h).  Launched on the context's stream only by those entry points: a context that never retires a row allocates nothing of
// this and enqueues exactly what it did.
#pragma once
#include "sca_respawn.hip.h"
#include "sca_vacancy.h"

namespace sca {

// ---- retiring rows -------------------------------------------------------------------------------------------------------------------------
// One WAVEFRONT per named row, as k_respawn: the record's pieces and the per-agent words by vacate_write_row (plain vector stores), and
// the row's stripe of K4's done_count for a row that was live (the only atomic).  Words of other rows are not touched.
struct VacateDev {
    PubRec *rec;
    double *heading, *total_dist;
    float *action;              // [n*8]
    int32_t *diag;              // [n*8]
    int32_t *step_num, *status, *nbr_n, *near_n, *done_count;
    uint8_t *nbr_valid;
    // the lists in slot form, null otherwise
    double *now_goal;
    int32_t *path_len, *path_rem;
    sca_scene_clearance *clear; // the closest-approach records (sca_clearance_enable), null: off
    int n;
};
__global__ __launch_bounds__(RESPAWN_WAVES * 64) void k_vacate(VacateDev d, const int32_t *ids, int count) {
    const int lane = (int)threadIdx.x & 63;
    const int r = (int)blockIdx.x * RESPAWN_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);     // wave-uniform
    if (r >= count) return;
    const int a = ids[r];
    if (a < 0 || a >= d.n) return;                                   // (the host has checked the ids: never taken)
    const uint32_t old_flags = d.rec[a].flags;
    const VacantRow w = vacant_row(old_flags, d.path_len != nullptr);
    if (lane == 0 && w.done_delta) atomicAdd(&d.done_count[(a & 255) * 32], w.done_delta);
    vacate_write_row(d, a, lane, w);
}

// ---- the permutation edit ------------------------------------------------------------------------------------------------------------------
// vac_pick's three ordered compactions in sca_get_finished's three launches: a count per tile of FIN_TILE items (ballot and popcount per
// wavefront, summed in LDS), k_finished_scan over the counts (its total goes to `head`), and the write: a picked item's id at
// base + (base_dev ? *base_dev : 0) + its tile's offset + the picks of the tile's earlier wavefronts + finished_rank in its own, where
// that place is below `cap`.  No atomics.
struct VacEditDev {
    VacView v;
    int32_t *counts, *offsets;  // [tiles]
    int32_t *out;               // where the ids go
    const int32_t *base_dev;    // nullable: a count an earlier compaction of the same call left on the device (the admitted rows)
    int base, cap, mode;
};
__device__ __forceinline__ unsigned long long vac_ballot(const VacEditDev &e, int item, int32_t &id, bool &mine) {
    mine = vac_pick(e.v, e.mode, item, id);
    return __ballot(mine);
}
__global__ __launch_bounds__(FIN_TILE) void k_vac_count(VacEditDev e) {
    __shared__ int32_t wsum[FIN_TILE / 64];
    const int t = (int)threadIdx.x;
    int32_t id; bool mine;
    const unsigned long long mask = vac_ballot(e, (int)blockIdx.x * FIN_TILE + t, id, mine);
    if ((t & 63) == 0) wsum[t >> 6] = __popcll(mask);
    __syncthreads();
    if (t == 0) e.counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
__global__ __launch_bounds__(FIN_TILE) void k_vac_write(VacEditDev e) {
    __shared__ int32_t wsum[FIN_TILE / 64];
    const int t = (int)threadIdx.x, wave = t >> 6;
    int32_t id; bool mine;
    const unsigned long long mask = vac_ballot(e, (int)blockIdx.x * FIN_TILE + t, id, mine);
    if ((t & 63) == 0) wsum[wave] = __popcll(mask);
    __syncthreads();
    if (!mine) return;
    int at = e.offsets[blockIdx.x] + finished_rank(mask, t & 63);
    for (int k = 0; k < wave; k++) at += wsum[k];
    at += e.base + (e.base_dev ? e.base_dev[0] : 0);
    if (at < 0 || at >= e.cap) return;                                 // (a permutation edit never leaves [0, n): the host's counts say so)
    e.out[at] = id;
}

}  // namespace sca
