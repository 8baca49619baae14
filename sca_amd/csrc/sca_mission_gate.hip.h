// sca_mission_gate.hip.h -- the kernels behind sca_set_mission_gate (the rules: sca_missions.h, sca_spawn.h).  While a gate is on
// missions_advance enqueues the five kernels of this file IN PLACE of k_mission_advance, on the context's stream, behind K4 and in front of
// the buffer swap; the host calls that change flags between two steps add k_mission_gate_named / k_mission_gate_clear behind their own
// kernels.  A context without a gate enqueues nothing of this.
//   k_mission_gate_end     a lane per row: k_mission_advance's endings, results and totals without the row write; an ended row whose flight
//                          names a successor becomes a new candidate (waiting[a] = j, fresh[a] = 1); the waiting and the new candidates
//                          counted per tile of 256 rows
//   k_mission_gate_place   a candidate's place in the offer order (waiting rows first, ascending id inside a class) from the tiles' counts;
//                          its query, row and entry into the list; the rows past the cap get their OVER_CAP words; the count on the device
//   k_mission_gate_probe   k_spawn_probe's tiling with the query count read from device memory
//   k_mission_gate_fold    spawn_fold + spawn_world: the world word per candidate
//   k_mission_gate_take    a wavefront per candidate: spawn_gate_walk over the earlier candidates, then its own row
// No atomic cursor, no wait between workgroups: the order is the launches' and the scan's.  Vector stores throughout.
#pragma once
#include "sca_missions.hip.h"
#include "sca_spawn.hip.h"

namespace sca {

struct MissionGateDev {
    MissionDev m;                   // the tables' view (row.rec: the records K4 has just written)
    const ObsRec *obs;              // [n_obs] the obstacles in set order
    int32_t *waiting, *verdict, *refusals, *fresh;      // [n] each
    int32_t *tile_counts;           // [2 tiles]: the waiting candidates per tile, the new ones behind them
    int32_t *count;                 // [1] the step's tested candidates, min(candidates, cap)
    ClearPoint *query;              // [cap] the list, in offer order
    int32_t *ids, *entry, *world;   // [cap] each
    SpawnPartial *partials;         // [ptiles][cap]
    unsigned long long *totals;     // [MGT_WORDS]
    double margin;
    int n_obs, cap, tiles, ptiles;  // tiles: of 256 rows; ptiles: of SPAWN_TILE partners
};
static_assert(MISSION_T == FIN_TILE && FIN_TILE == 256, "the gate's row tiles are four wavefronts");

// ---- endings and counts ------------------------------------------------------------------------------------------------------------------------
// KEEP IN STEP with k_mission_advance (sca_missions.hip.h): the table lookup, the totals and the six-piece result below are that kernel's,
// line for line, without its row write and its MST_TAKEN (a change to what an ending is, to a total or to sca_mission_result belongs in
// both; tests/test_gpu_mission_gate.py holds a gate that was set and taken off against tables alone, and every result against the twin's).
__global__ __launch_bounds__(MISSION_T) void k_mission_gate_end(MissionGateDev g) {
    __shared__ int32_t wsum[2][MISSION_T / 64];
    const MissionDev &m = g.m;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int row = (int)blockIdx.x * MISSION_T + (int)threadIdx.x;
    const int row0 = __builtin_amdgcn_readfirstlane(row - lane);
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
    mission_total(m.totals, MST_AGENT_STEPS, __ballot(in && !(fo & RSP_DONE_FLAGS)), lane);
    mission_total(m.totals, MST_ARRIVED, __ballot(ended && t.outcome == MISSION_ARRIVED), lane);
    mission_total(m.totals, MST_COLLIDED, __ballot(ended && t.outcome == MISSION_COLLIDED), lane);
    mission_total(m.totals, MST_TIMED_OUT, __ballot(ended && t.outcome == MISSION_TIMED_OUT), lane);
    mission_total(m.totals, MST_STOPPED, __ballot(ended && next < 0), lane);           // (MST_TAKEN moves where a candidate is admitted)
    if (row == 0) atomicAdd(&m.totals[MST_UPDATES], 1ull);
    unsigned long long todo = __ballot(ended && table);
    while (todo) {                                                         // the results, as k_mission_advance writes them
        const int l0 = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int a = row0 + l0;
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
            } else {
                const sca_scene_clearance none = scene_clearance_empty();
                if (lane == 4) { piece_put64(q, 0, none.agent_clear); piece_put64(q, 1, none.obs_clear); }
                else { q.w[0] = (uint32_t)none.agent_partner; q.w[1] = (uint32_t)none.agent_step; q.w[2] = (uint32_t)none.obs_partner; q.w[3] = (uint32_t)none.obs_step; }
            }
            ((RespawnPiece *)out)[lane] = q;
        }
    }
    int32_t wait = in ? g.waiting[row] : -1;
    const bool fresh = next >= 0;
    if (fresh) wait = next;                                                // a new candidate for entry `next`
    if (in) {
        m.live[row] = (fn & RSP_DONE_FLAGS) ? 0 : 1;                       // (an admitted row's word becomes 1 in k_mission_gate_take)
        g.fresh[row] = fresh ? 1 : 0;
        if (fresh) g.waiting[row] = wait;
    }
    if (ended && table) {
        m.ended[row] = en + 1u;
        m.flying[row] = next;
    }
    const int cls = mission_gate_class(wait, fresh);
    const unsigned long long mw = __ballot(cls == MGC_WAITING), mn = __ballot(cls == MGC_NEW);
    if (lane == 0) { wsum[0][wave] = __popcll(mw); wsum[1][wave] = __popcll(mn); }
    __syncthreads();
    if (threadIdx.x == 0) {
        g.tile_counts[blockIdx.x] = wsum[0][0] + wsum[0][1] + wsum[0][2] + wsum[0][3];
        g.tile_counts[g.tiles + blockIdx.x] = wsum[1][0] + wsum[1][1] + wsum[1][2] + wsum[1][3];
    }
}

// ---- ordered placement -------------------------------------------------------------------------------------------------------------------------
// Every workgroup sums the tiles' counts itself (the waiting rows of the whole context, the waiting and the new rows of the tiles in front
// of its own): 2 x tiles words from L2 per workgroup instead of one more dependent dispatch for k_finished_scan.
__global__ __launch_bounds__(MISSION_T) void k_mission_gate_place(MissionGateDev g) {
    __shared__ int32_t red[4][MISSION_T];
    __shared__ int32_t wsum[2][MISSION_T / 64];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, tile = (int)blockIdx.x;
    const int row = tile * MISSION_T + t;
    const bool in = row < g.m.row.n;
    int32_t s_wall = 0, s_wbefore = 0, s_nall = 0, s_nbefore = 0;
    for (int i = t; i < g.tiles; i += MISSION_T) {
        const int32_t cw = g.tile_counts[i], cn = g.tile_counts[g.tiles + i];
        s_wall += cw; s_nall += cn;
        if (i < tile) { s_wbefore += cw; s_nbefore += cn; }
    }
    red[0][t] = s_wall; red[1][t] = s_wbefore; red[2][t] = s_nall; red[3][t] = s_nbefore;
    const int32_t wait = in ? g.waiting[row] : -1;
    const int cls = mission_gate_class(wait, in && g.fresh[row] != 0);
    const unsigned long long mw = __ballot(cls == MGC_WAITING), mn = __ballot(cls == MGC_NEW);
    if (lane == 0) { wsum[0][wave] = __popcll(mw); wsum[1][wave] = __popcll(mn); }
    __syncthreads();
    for (int step = MISSION_T / 2; step > 0; step >>= 1) {
        if (t < step) { red[0][t] += red[0][t + step]; red[1][t] += red[1][t + step]; red[2][t] += red[2][t + step]; red[3][t] += red[3][t + step]; }
        __syncthreads();
    }
    const int32_t wall = red[0][0], wbefore = red[1][0], nall = red[2][0], nbefore = red[3][0];
    const int32_t total = wall + nall, tested = total < g.cap ? total : g.cap;
    if (tile == 0 && t == 0) {
        g.count[0] = tested;
        if (total) atomicAdd(&g.totals[MGT_OFFERED], (unsigned long long)total);
        if (total > tested) atomicAdd(&g.totals[MGT_OVER_CAP], (unsigned long long)(total - tested));
    }
    if (total == 0) return;                                                // nobody is offered in this step (uniform over the grid: every workgroup formed the same sums)
    if (cls == MGC_NONE) return;
    const int c = cls == MGC_NEW ? 1 : 0;
    int rank = (cls == MGC_NEW ? nbefore : wbefore) + finished_rank(c ? mn : mw, lane);
    for (int k = 0; k < wave; k++) rank += wsum[c][k];
    const int place = mission_gate_place(cls, rank, wall);
    if (place < g.cap) {
        const sca_mission *e = g.m.entries + ((int64_t)g.m.M * row + wait);
        g.query[place] = mission_gate_query(*e, g.m.row.rec[row]);
        g.ids[place] = row;
        g.entry[place] = wait;
    } else {                                                               // not tested in this step: it waits, in front of every later arrival
        const MissionGateSettle s = mission_gate_settle(SCA_SPAWN_OVER_CAP, wait, g.refusals[row]);
        g.waiting[row] = s.waiting; g.verdict[row] = s.verdict; g.refusals[row] = s.refusals;
    }
}

// ---- probe and fold ----------------------------------------------------------------------------------------------------------------------------
// grid (ptiles, slots): the workgroups of a tile share its chunks, slot y takes the chunks y, y + slots, ... below the count the device
// holds; a workgroup with no chunk returns before it stages anything.  Everything else is k_spawn_probe.
constexpr int MISSION_GATE_SLOTS = 8;
__global__ __launch_bounds__(SPAWN_WAVES * 64) void k_mission_gate_probe(MissionGateDev g) {
    __shared__ ClearPoint pts[SPAWN_TILE];
    __shared__ int32_t ids[SPAWN_TILE];
    __shared__ SpawnPartial meet[SPAWN_WAVES - 1][SPAWN_CHUNK];
    const int count = g.count[0];                                         // (<= cap: k_mission_gate_place's minimum)
    const int chunks = spawn_chunks(count);
    if ((int)blockIdx.y >= chunks) return;
    const int t = (int)threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tile = (int)blockIdx.x, n = g.m.row.n;
    const int64_t g0 = (int64_t)tile * SPAWN_TILE, total = (int64_t)n + g.n_obs;
    const int have = (int)(total - g0 < SPAWN_TILE ? total - g0 : SPAWN_TILE);
    for (int j = t; j < have; j += SPAWN_WAVES * 64) {
        const int64_t p = g0 + j;
        ClearPoint c;
        if (p < n) { const PubRec a = g.m.row.rec[p]; c.x = a.px; c.y = a.py; c.z = a.pz; c.r = a.radius; }
        else { const ObsRec o = g.obs[p - n]; c.x = o.px; c.y = o.py; c.z = o.pz; c.r = o.radius; }
        pts[j] = c;
        ids[j] = p < n && (g.m.row.rec[p].flags & FLAG_VACANT) ? SPAWN_VACANT_ID : spawn_partner_id(p, n);
    }
    __syncthreads();
    for (int chunk = (int)blockIdx.y; chunk < chunks; chunk += (int)gridDim.y) {      // (uniform over the workgroup)
        const int q = chunk * SPAWN_CHUNK + lane;
        const bool live = q < count;
        SpawnPartial acc = spawn_partial_none();
        if (live) {
            constexpr int SLICE = SPAWN_TILE / SPAWN_WAVES;
            const int begin = wave * SLICE, end = begin + SLICE < have ? begin + SLICE : have;
            spawn_tile_partial(g.query[q], g.ids[q], pts, ids, begin, end, g0, n, acc, L3Norm{});
        }
        if (wave > 0) meet[wave - 1][lane] = acc;
        __syncthreads();
        if (wave == 0 && live) {
#pragma unroll
            for (int w = 0; w < SPAWN_WAVES - 1; w++) spawn_merge(acc, meet[w][lane]);
            g.partials[spawn_partial_index(tile, q, g.cap)] = acc;
        }
        __syncthreads();                                                   // (the next chunk's wavefronts write `meet` again)
    }
}
__global__ __launch_bounds__(256) void k_mission_gate_fold(MissionGateDev g) {
    const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (q >= g.count[0]) return;
    g.world[q] = spawn_world(spawn_fold(g.partials, g.ptiles, q, g.cap), g.margin);
}

// ---- gate and take -----------------------------------------------------------------------------------------------------------------------------
// One WAVEFRONT per candidate r: the entry walk over the earlier candidates reads only the list and the world words, never a row, so the
// wavefronts that already write their rows do not disturb it.  Then the wavefront serves its own row: respawn_write_row where admitted,
// the waiting / verdict / refusal words where not.
constexpr int MISSION_GATE_WAVES = 4;
__global__ __launch_bounds__(MISSION_GATE_WAVES * 64) void k_mission_gate_take(MissionGateDev g) {
    const MissionDev &m = g.m;
    const int lane = (int)threadIdx.x & 63;
    const int r = (int)blockIdx.x * MISSION_GATE_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);      // wave-uniform
    if (r >= g.count[0]) return;
    const int32_t world = g.world[r];
    bool blocked = false;
    if (world == SCA_SPAWN_ADMITTED) blocked = spawn_gate_walk(g.query, g.world, r, g.margin, lane, 64, L3Norm{});
    const int32_t v = spawn_verdict(world, __ballot(blocked) != 0ull);
    const int a = g.ids[r], j = g.entry[r];                               // (r < count: k_mission_gate_place wrote both in this step)
    const MissionGateSettle s = mission_gate_settle(v, j, g.refusals[a]);
    if (s.take) {
        const uint32_t flags = m.row.rec[a].flags;
        const RespawnRow w = mission_take_row(m, a, j, flags, lane);      // (the row's loads stay in front of its stores: mission_take_row's note)
        if (lane == 0) {
            m.cursor[a] = j; m.flying[a] = j; m.live[a] = 1;
            if (w.done_delta) atomicAdd(&m.row.done_count[(a & 255) * 32], w.done_delta);
            atomicAdd(&m.totals[MST_TAKEN], 1ull);
        }
    }
    if (lane == 0) {
        g.waiting[a] = s.waiting; g.verdict[a] = s.verdict; g.refusals[a] = s.refusals;
        atomicAdd(&g.totals[s.counter], 1ull);
    }
}

// ---- the host calls between two steps ----------------------------------------------------------------------------------------------------------
// a host respawn (behind its k_respawn and k_mission_host_flight): a named row the call wrote loses its pending mission.  One lane per
// NAMED row, so `dropped` counts a row once only because no call names a row twice: respawn_check refuses a repeated id on the host
// (RSP_REPEATED_ID) before anything is enqueued, for the plain and the gated call alike.
__global__ __launch_bounds__(MISSION_T) void k_mission_gate_named(const int32_t *ids, const int32_t *verdict, int count, int n, int32_t *waiting, unsigned long long *totals) {
    const int r = (int)blockIdx.x * MISSION_T + (int)threadIdx.x;
    bool drop = false;
    if (r < count && !(verdict && verdict[r] != 0)) {
        const int a = ids[r];
        if (a >= 0 && a < n && waiting[a] >= 0) { waiting[a] = -1; drop = true; }
    }
    mission_total(totals, MGT_DROPPED, __ballot(drop), (int)threadIdx.x & 63);
}
// rec != null: the rows that are unfinished in the records as they stand (a new state); null: every row (the gate goes off)
__global__ __launch_bounds__(MISSION_T) void k_mission_gate_clear(const PubRec *rec, int32_t *waiting, int n, unsigned long long *totals) {
    const int row = (int)blockIdx.x * MISSION_T + (int)threadIdx.x;
    bool drop = false;
    if (row < n && waiting[row] >= 0 && (!rec || !(rec[row].flags & RSP_DONE_FLAGS))) { waiting[row] = -1; drop = true; }
    mission_total(totals, MGT_DROPPED, __ballot(drop), (int)threadIdx.x & 63);
}

}  // namespace sca
