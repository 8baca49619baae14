// sca_spawn.hip.h -- the kernels behind sca_probe_clearance and sca_respawn_agents_gated (the rules, the tiling and the block: sca_spawn.h).
// Launched on the context's stream only by those two entry points: a context that never calls them allocates and enqueues nothing of this.
#pragma once
#include "sca_kernels.hip.h"
#include "sca_scenes.hip.h"
#include "sca_spawn.h"

namespace sca {

struct SpawnDev {
    const PubRec *rec;              // [n] the agents' public records as they are now
    const ObsRec *obs;              // [m] the obstacles in set order
    const ClearPoint *query;        // [count] the device copy of the block's query section
    const int32_t *ignore;          // [count]
    SpawnPartial *partials;         // [tiles][cap]
    int32_t *world, *verdict;       // the world test's word and the verdict per query of the call (gated calls)
    int n, m, tiles;
    int first, count, cap;          // the launch's queries: first .. first + count - 1 of the call, `cap` of room per tile in the partials
};

// ---- the probe ---------------------------------------------------------------------------------------------------------------------------
// grid (tiles, chunks), SPAWN_WAVES wavefronts: the workgroup stages its tile's partners -- ClearPoint plus id, 36 bytes each -- in LDS,
// every lane holds ONE query of the chunk with its running (c, id) of both halves in registers, wavefront w walks slice w of the tile (the
// staged partners are read at a wave-uniform index: LDS broadcasts), the wavefronts' minima meet in LDS and lane q of wavefront 0 stores
// the one partial at [tile][query].  No atomics: the minimum on (c, id) does not depend on the order it is formed in.
__global__ __launch_bounds__(SPAWN_WAVES * 64) void k_spawn_probe(SpawnDev s) {
    __shared__ ClearPoint pts[SPAWN_TILE];
    __shared__ int32_t ids[SPAWN_TILE];
    __shared__ SpawnPartial meet[SPAWN_WAVES - 1][SPAWN_CHUNK];
    const int t = (int)threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int tile = (int)blockIdx.x;
    const int64_t g0 = (int64_t)tile * SPAWN_TILE, total = (int64_t)s.n + s.m;
    const int have = (int)(total - g0 < SPAWN_TILE ? total - g0 : SPAWN_TILE);            // (tile < tiles: have >= 1)
    for (int j = t; j < have; j += SPAWN_WAVES * 64) {
        const int64_t g = g0 + j;
        ClearPoint p;
        if (g < s.n) { const PubRec a = s.rec[g]; p.x = a.px; p.y = a.py; p.z = a.pz; p.r = a.radius; }
        else { const ObsRec o = s.obs[g - s.n]; p.x = o.px; p.y = o.py; p.z = o.pz; p.r = o.radius; }
        pts[j] = p;
        ids[j] = g < s.n && (s.rec[g].flags & FLAG_VACANT) ? SPAWN_VACANT_ID : spawn_partner_id(g, s.n);
    }
    __syncthreads();
    const int q = (int)blockIdx.y * SPAWN_CHUNK + lane;
    const bool live = q < s.count;
    SpawnPartial acc = spawn_partial_none();
    if (live) {
        constexpr int SLICE = SPAWN_TILE / SPAWN_WAVES;
        const int begin = wave * SLICE, end = begin + SLICE < have ? begin + SLICE : have;
        spawn_tile_partial(s.query[s.first + q], s.ignore[s.first + q], pts, ids, begin, end, g0, s.n, acc, L3Norm{});
    }
    if (wave > 0) meet[wave - 1][lane] = acc;
    __syncthreads();
    if (wave == 0 && live) {
#pragma unroll
        for (int w = 0; w < SPAWN_WAVES - 1; w++) spawn_merge(acc, meet[w][lane]);
        s.partials[spawn_partial_index(tile, q, s.cap)] = acc;
    }
}

// One lane per query folds the tiles' partials (spawn_fold) and writes the 32-byte record into the page-locked block as two 16-byte
// pieces; under a gated call (margin >= 0) also the world test's word, for k_spawn_gate.
__global__ __launch_bounds__(256) void k_spawn_reduce(SpawnDev s, uint8_t *blk, SpawnLayout L, double margin, int gated) {
    const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (q >= s.count) return;
    const sca_scene_clearance r = spawn_fold(s.partials, s.tiles, q, s.cap);
    const restart_piece *from = (const restart_piece *)&r;
    restart_piece *to = (restart_piece *)(blk + L.off[SPB_OUT] + 32 * ((int64_t)s.first + q));
    to[0] = from[0];
    to[1] = from[1];
    if (gated) s.world[s.first + q] = spawn_world(r, margin);
}

// The entry test: one WAVEFRONT per row r of the call walks the rows r' < r, lanes strided (spawn_gate_walk), and a ballot says whether any
// lane found a blocking one; lane 0 writes the verdict word to the device array k_respawn reads and to the block.  One launch over all
// the call's rows (first 0, count the call's).
constexpr int SPAWN_GATE_WAVES = 4;
__global__ __launch_bounds__(SPAWN_GATE_WAVES * 64) void k_spawn_gate(SpawnDev s, uint8_t *blk, SpawnLayout L, double margin) {
    const int lane = (int)threadIdx.x & 63;
    const int r = (int)blockIdx.x * SPAWN_GATE_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);      // wave-uniform
    if (r >= s.count) return;
    const int32_t world = s.world[r];
    bool blocked = false;
    if (world == SCA_SPAWN_ADMITTED) blocked = spawn_gate_walk(s.query, s.world, r, margin, lane, 64, L3Norm{});
    const bool any = __ballot(blocked) != 0ull;
    if (lane == 0) {
        const int32_t v = spawn_verdict(world, any);
        s.verdict[r] = v;
        ((int32_t *)(blk + L.off[SPB_VERDICT]))[r] = v;
    }
}

}  // namespace sca
