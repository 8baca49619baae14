// sca_missions.hip.h -- the kernels behind the mission tables (the rules: sca_missions.h).  k_mission_advance is enqueued by
// launch_collide_finish behind K4 and in front of the buffer swap, only while tables are set; k_mission_count / k_mission_write only by
// sca_get_mission_results, k_mission_live / k_mission_host_flight by the host calls that change flags between two steps: a context without tables enqueues exactly what it did.
// Tables whose entries bring their own waypoint lists (sca_set_missions_paths) add no kernel: the take (mission_take_row, shared with
// k_mission_gate_take) also copies the entry's list into the row's room, through the copy k_respawn makes (respawn_write_list).
#pragma once
#include "sca_respawn.hip.h"
#include "sca_missions.h"

namespace sca {

// ---- taking the next mission inside the step -----------------------------------------------------------------------------------------------
// One LANE per agent row finds out whether its row ended in this step; the WAVEFRONT then serves its ended rows one after the other (a
// wave-uniform loop over the ballot's set bits): the result record as six 16-byte pieces by lanes 0 .. 5, and, where the ended flight names
// a successor, the row through respawn_write_row -- k_respawn's row write, with the row's table entry as the source of the values.
//   row.rec          the records K4 has just written (DeviceView::rec_new: the current ones behind the swap)
//   live             1 where the row entered this step without a done flag.  The old record cannot tell: a policy pass sets the collision bit
//                    there for a row it serves (k_action).  The kernel leaves the word for the next step; the host calls that change flags
//                    between two steps (sca_set_state, sca_respawn_agents, sca_set_missions itself) refresh it with k_mission_live
//   cursor           the entry whose successors the row's next ending follows (-1: first_ok / first_fail)
//   flying           the entry the row flies (-1: the flight in the air at sca_set_missions, or one the host gave)
//   ended            the row's endings so far: the ring index of its next result
// Vector stores throughout; the atomics: the totals (64-bit adds, one per wavefront and counter, only where non-zero) and the taken rows'
// stripes of K4's done_count.
struct MissionDev {
    RespawnDev row;
    int32_t *live;
    const uint8_t *policy;
    const sca_mission *entries;
    const int32_t *first_ok, *first_fail;
    int32_t *cursor, *flying;
    uint32_t *ended;
    sca_mission_result *results;
    unsigned long long *totals;     // [MST_WORDS]
    long long update;               // the env update this launch belongs to, counted from sca_set_missions (1-based)
    int M, R;
    // tables with lists (sca_set_missions_paths in slot form; row.path_len .. row.W are set with them, null / 0 otherwise): the packed CSR
    // the call brought, immutable until the tables are replaced -- path_off [M n + 1] over the flat entry index (null: every entry brings
    // the empty list), path_pts the points
    const int32_t *path_off;
    const double *path_pts;
};
// The take of entry nx by row a, by the whole wavefront (everything wave-uniform): the row becomes what sca_respawn_agents naming it with the
// entry's values -- and, with lists, the entry's list as its path arrays -- leaves.  flags: the flag word the row ended with.  The caller
// has fenced its own loads of the row's old words; the old length is loaded here in front of every store of the row (see below).
__device__ __forceinline__ RespawnRow mission_take_row(const MissionDev &m, int a, int nx, uint32_t flags, int lane) {
    const bool lists = m.row.path_len != nullptr;
    const int32_t old_len = lists ? m.row.path_len[a] : 0;
    // The loads of the row's old words (the result's, the flag word, the old length) stand in front of the row's stores in the ONE
    // wavefront that does both.  For the result's per-lane VECTOR loads the argument is the older one: the wavefront's vector memory
    // instructions issue in program order and go down one path to the same cache, and the fence only keeps the compiler from moving the
    // stores up.  The old length is different: its address is the same for the whole wavefront, so the compiler may fetch it through the
    // SCALAR path, which is not ordered against the vector stores.  It is held by two things that ARE relied on: every store of a path
    // word and of vpref_mode is issued behind the fence, and the seq_cst fence at workgroup scope makes the compiler wait for every
    // outstanding load, scalar ones included, before anything behind it issues; and `bits`, which decides the mode store, is computed
    // from the loaded value.
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    const int64_t fe = (int64_t)m.M * a + nx;
    return mission_take_write(m.row, a, lane, m.policy[a], flags, m.entries + fe, lists, old_len, m.path_off, m.path_pts, fe);
}
constexpr int MISSION_T = 256;
__device__ __forceinline__ void mission_total(unsigned long long *totals, int which, unsigned long long mask, int lane) {
    if (lane == 0 && mask) atomicAdd(&totals[which], (unsigned long long)__popcll(mask));
}
__global__ __launch_bounds__(MISSION_T) void k_mission_advance(MissionDev m) {
    const int lane = (int)threadIdx.x & 63;
    const int row = (int)blockIdx.x * MISSION_T + (int)threadIdx.x;
    const int row0 = __builtin_amdgcn_readfirstlane(row - lane);           // the wavefront's first row (wave-uniform)
    const bool in = row < m.row.n;
    const uint32_t fo = in && m.live[row] ? 0u : RSP_DONE_FLAGS, fn = in ? m.row.rec[row].flags : 0u;
    int ok = -1, fail = -1, cur = -1;
    bool table = false;
    if (in) {
        const int32_t f_ok = m.first_ok[row], f_fail = m.first_fail[row];
        table = mission_has_table(f_ok, f_fail);
        cur = m.cursor[row];
        if (table && cur >= 0) { const sca_mission *e = m.entries + ((int64_t)m.M * row + cur); ok = e->next_ok; fail = e->next_fail; }
        else if (table) { ok = f_ok; fail = f_fail; }
    }
    const bool ended = in && mission_ended(fo, fn);
    const MissionTake t = mission_take(fn, ok, fail);
    const int next = ended && table ? t.next : -1;
    const uint32_t en = ended && table ? m.ended[row] : 0u;
    const int fly = ended && table ? m.flying[row] : -1;
    // the totals: every row of the context counts, with or without a table
    mission_total(m.totals, MST_AGENT_STEPS, __ballot(in && !(fo & RSP_DONE_FLAGS)), lane);
    mission_total(m.totals, MST_ARRIVED, __ballot(ended && t.outcome == MISSION_ARRIVED), lane);
    mission_total(m.totals, MST_COLLIDED, __ballot(ended && t.outcome == MISSION_COLLIDED), lane);
    mission_total(m.totals, MST_TIMED_OUT, __ballot(ended && t.outcome == MISSION_TIMED_OUT), lane);
    mission_total(m.totals, MST_TAKEN, __ballot(ended && next >= 0), lane);
    mission_total(m.totals, MST_STOPPED, __ballot(ended && next < 0), lane);
    if (row == 0) atomicAdd(&m.totals[MST_UPDATES], 1ull);
    unsigned long long todo = __ballot(ended && table);
    while (todo) {
        const int l0 = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int a = row0 + l0;                                           // wave-uniform from here on
        const int nx = __builtin_amdgcn_readlane(next, l0);
        const uint32_t flags = (uint32_t)__builtin_amdgcn_readlane((int)fn, l0);
        sca_mission_result *out = m.results + ((int64_t)m.R * a + (int)((uint32_t)__builtin_amdgcn_readlane((int)en, l0) % (uint32_t)m.R));
        if (lane < (int)(sizeof(sca_mission_result) / 16)) {
            const PubRec *me = m.row.rec + a;
            RespawnPiece q;
            if (lane == 0) {
                q.w[0] = (uint32_t)a; q.w[1] = (uint32_t)__builtin_amdgcn_readlane(fly, l0); q.w[2] = flags; q.w[3] = (uint32_t)m.row.step_num[a];
            } else if (lane == 1) {
                piece_put64(q, 0, m.row.total_dist[a]); piece_put64(q, 1, me->px);
            } else if (lane == 2) {
                piece_put64(q, 0, me->py); piece_put64(q, 1, me->pz);
            } else if (lane == 3) {
                q.w[0] = (uint32_t)(unsigned long long)m.update; q.w[1] = (uint32_t)((unsigned long long)m.update >> 32); q.w[2] = (uint32_t)nx; q.w[3] = 0u;
            } else if (m.row.clear) {
                q = ((const RespawnPiece *)(m.row.clear + a))[lane - 4];
            } else {                                                       // no records: the empty one
                const sca_scene_clearance none = scene_clearance_empty();
                if (lane == 4) { piece_put64(q, 0, none.agent_clear); piece_put64(q, 1, none.obs_clear); }
                else { q.w[0] = (uint32_t)none.agent_partner; q.w[1] = (uint32_t)none.agent_step; q.w[2] = (uint32_t)none.obs_partner; q.w[3] = (uint32_t)none.obs_step; }
            }
            ((RespawnPiece *)out)[lane] = q;
        }
        if (nx < 0) continue;                                              // the row stays finished as it is
        (void)mission_take_row(m, a, nx, flags, lane);                     // (the result's loads above stay in front of the row's stores: its note)
    }
    if (in) m.live[row] = next >= 0 || !(fn & RSP_DONE_FLAGS) ? 1 : 0;
    if (ended && table) {
        m.ended[row] = en + 1u;
        m.flying[row] = next;                                              // (-1: stopped -- what flies next, if anything, is the host's)
        if (next >= 0) {
            m.cursor[row] = next;
            atomicAdd(&m.row.done_count[(row & 255) * 32], 1);           // K4 counted the row as done: it runs again
        }
    }
}

// the rows that will enter the next step without a done flag, from the records as they stand between two steps
__global__ __launch_bounds__(MISSION_T) void k_mission_live(const PubRec *rec, int32_t *live, int n) {
    const int row = (int)blockIdx.x * MISSION_T + (int)threadIdx.x;
    if (row < n) live[row] = (rec[row].flags & RSP_DONE_FLAGS) ? 0 : 1;
}
// A host respawn while tables stand (enqueued behind its k_respawn): what the named rows fly now is not an entry, whether they had
// stopped or were still flying one.  One lane per named row; `ids` / `verdict` as k_respawn reads them (a gated call's refused rows are
// left alone, as there).  The cursors stay: the flight's ending follows the same successors.
__global__ __launch_bounds__(MISSION_T) void k_mission_host_flight(const int32_t *ids, const int32_t *verdict, int count, int n, int32_t *flying) {
    const int r = (int)blockIdx.x * MISSION_T + (int)threadIdx.x;
    if (r >= count) return;
    if (verdict && verdict[r] != 0) return;
    const int a = ids[r];
    if (a < 0 || a >= n) return;                                           // (the host has checked the ids: never taken)
    flying[a] = -1;
}

// ---- collecting the results ------------------------------------------------------------------------------------------------------------------
// sca_get_finished's ordered compaction with a COUNT per row instead of a flag: a tile's count (k_mission_count), the scan of the tiles by
// k_finished_scan, and the write -- a row's fresh results stand at its tile's offset plus the fresh results of the tile's earlier rows, oldest
// first.  No atomic cursor.  The write marks the results collected; where the block has no room for all of them it writes and marks nothing.
struct MissionCollectDev {
    const uint32_t *ended;
    uint32_t *collected;
    const sca_mission_result *results;
    int32_t *counts, *offsets;      // [tiles]
    int32_t *total;                 // [1] the scan's total on the device
    int n, tiles, R;
};
static_assert(MISSION_T == FIN_TILE, "the collect's tiles are k_finished_scan's");
__device__ __forceinline__ int mission_fresh(const MissionCollectDev &c, int row) { return row < c.n ? mission_new(c.ended[row], c.collected[row], c.R) : 0; }
// the inclusive scan of the tile's per-row counts in LDS; returns this thread's inclusive sum, part[FIN_TILE - 1] the tile's
__device__ __forceinline__ int32_t mission_tile_scan(int32_t *part, int t, int32_t mine) {
    part[t] = mine;
    __syncthreads();
    for (int step = 1; step < FIN_TILE; step <<= 1) {
        const int32_t add = t >= step ? part[t - step] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    return part[t];
}
__global__ __launch_bounds__(FIN_TILE) void k_mission_count(MissionCollectDev c) {
    __shared__ int32_t part[FIN_TILE];
    const int t = (int)threadIdx.x;
    mission_tile_scan(part, t, mission_fresh(c, (int)blockIdx.x * FIN_TILE + t));
    if (t == 0) c.counts[blockIdx.x] = part[FIN_TILE - 1];
}
__global__ __launch_bounds__(FIN_TILE) void k_mission_write(MissionCollectDev c, uint8_t *blk, int capacity) {
    __shared__ int32_t part[FIN_TILE];
    const int t = (int)threadIdx.x, row = (int)blockIdx.x * FIN_TILE + t;
    const int fresh = mission_fresh(c, row);
    const int32_t before = mission_tile_scan(part, t, fresh) - fresh;
    const int32_t total = c.total[0];
    if (row == 0) *(int32_t *)blk = total;
    if (total > capacity || fresh == 0) return;
    const uint32_t en = c.ended[row];
    RespawnPiece *out = (RespawnPiece *)(blk + MISSION_HEAD_BYTES) + (int64_t)(sizeof(sca_mission_result) / 16) * (c.offsets[blockIdx.x] + before);
    for (int k = 0; k < fresh; k++) {
        const RespawnPiece *in = (const RespawnPiece *)(c.results + ((int64_t)c.R * row + mission_ring_slot(en, fresh, k, c.R)));
        for (int p = 0; p < (int)(sizeof(sca_mission_result) / 16); p++) out[(int64_t)(sizeof(sca_mission_result) / 16) * k + p] = in[p];
    }
    c.collected[row] = en;
}

}  // namespace sca
