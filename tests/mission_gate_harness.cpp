// The pure rules of the mission tables' admission gate (sca_amd/csrc/sca_missions.h: mission_gate_check, mission_gate_place,
// mission_gate_query, mission_gate_settle; the probe and the gate: sca_spawn.h) behind C entry points (tests/test_mission_gate_cpu.py), and
// -- with -DMISSION_GATE_MAIN -- as a program of its own for the sanitizers: every buffer on the heap in exactly the size the rules may touch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sca_missions.h"

using namespace sca;

namespace {

// One step's gate on host arrays, kernel by kernel, with the functions the kernels call:
//   k_mission_gate_place   the classes counted per tile of FIN_TILE rows, a candidate's place from the tiles' counts, the list, the over-cap words
//   k_mission_gate_probe   partials of exactly ptiles x cap records, tile by tile and slice by slice; k_mission_gate_fold: the world words
//   k_mission_gate_take    spawn_gate_walk lane by lane, mission_gate_settle
// waiting / verdict / refusals: the rows' words (in and out); fresh: 1 where the row ended in this step; take[r]: 1 where list place r is
// admitted (the caller writes the row).  Returns the number of candidates (tested: min(that, cap)).
int gate_step(int n, int M, const sca_mission *entries, const PubRec *rec, int m, const double *obs_pos, const double *obs_radius, double margin, int cap,
              int32_t *waiting, int32_t *verdict, int32_t *refusals, const int32_t *fresh, int32_t *list_ids, int32_t *list_entry, int32_t *list_verdict,
              sca_scene_clearance *list_probe, uint64_t *totals) {
    const int tiles = finished_tiles(n);
    std::vector<int32_t> counts(2 * (size_t)tiles, 0);
    for (int row = 0; row < n; row++) {
        const int cls = mission_gate_class(waiting[row], fresh[row] != 0);
        if (cls == MGC_WAITING) counts[(size_t)(row / FIN_TILE)]++;
        if (cls == MGC_NEW) counts[(size_t)tiles + (size_t)(row / FIN_TILE)]++;
    }
    int wall = 0, nall = 0;
    for (int t = 0; t < tiles; t++) { wall += counts[(size_t)t]; nall += counts[(size_t)tiles + (size_t)t]; }
    const int total = wall + nall, tested = total < cap ? total : cap;
    if (total) totals[MGT_OFFERED] += (uint64_t)total;
    if (total > tested) totals[MGT_OVER_CAP] += (uint64_t)(total - tested);
    std::vector<ClearPoint> query((size_t)(tested ? tested : 1));
    for (int tile = tiles - 1; tile >= 0; tile--) {                       // (any order of the workgroups)
        int wbefore = 0, nbefore = 0;
        for (int t = 0; t < tile; t++) { wbefore += counts[(size_t)t]; nbefore += counts[(size_t)tiles + (size_t)t]; }
        int rank_w = 0, rank_n = 0;
        for (int i = 0; i < FIN_TILE; i++) {
            const int row = tile * FIN_TILE + i;
            if (row >= n) break;
            const int cls = mission_gate_class(waiting[row], fresh[row] != 0);
            if (cls == MGC_NONE) continue;
            const int rank = cls == MGC_NEW ? nbefore + rank_n++ : wbefore + rank_w++;
            const int place = mission_gate_place(cls, rank, wall);
            if (place < cap) {
                if (place >= tested) std::abort();
                query[(size_t)place] = mission_gate_query(entries[(int64_t)M * row + waiting[row]], rec[row]);
                list_ids[place] = row; list_entry[place] = waiting[row];
            } else {
                const MissionGateSettle s = mission_gate_settle(SCA_SPAWN_OVER_CAP, waiting[row], refusals[row]);
                waiting[row] = s.waiting; verdict[row] = s.verdict; refusals[row] = s.refusals;
            }
        }
    }
    const int ptiles = spawn_tiles(n, m, SPAWN_TILE);
    SpawnPartial *partials = (SpawnPartial *)std::malloc(sizeof(SpawnPartial) * (size_t)(spawn_partials(n, m, cap, SPAWN_TILE) ? spawn_partials(n, m, cap, SPAWN_TILE) : 1));
    const int64_t all = (int64_t)n + m;
    for (int tile = 0; tile < ptiles; tile++) {
        const int64_t g0 = (int64_t)tile * SPAWN_TILE;
        const int have = (int)(all - g0 < SPAWN_TILE ? all - g0 : SPAWN_TILE);
        std::vector<ClearPoint> pts((size_t)have);
        std::vector<int32_t> ids((size_t)have);
        for (int j = 0; j < have; j++) {
            const int64_t g = g0 + j;
            pts[(size_t)j] = g < n ? ClearPoint{rec[g].px, rec[g].py, rec[g].pz, rec[g].radius}
                                   : ClearPoint{obs_pos[3 * (g - n)], obs_pos[3 * (g - n) + 1], obs_pos[3 * (g - n) + 2], obs_radius[g - n]};
            ids[(size_t)j] = spawn_partner_id(g, n);
        }
        for (int q = 0; q < tested; q++) {
            SpawnPartial acc = spawn_partial_none();
            constexpr int SLICE = SPAWN_TILE / SPAWN_WAVES;
            for (int wave = 0; wave < SPAWN_WAVES; wave++) {
                SpawnPartial mine = spawn_partial_none();
                const int begin = wave * SLICE, end = begin + SLICE < have ? begin + SLICE : have;
                spawn_tile_partial(query[(size_t)q], list_ids[q], pts.data(), ids.data(), begin, end, g0, n, mine, L3Norm{});
                spawn_merge(acc, mine);
            }
            partials[spawn_partial_index(tile, q, cap)] = acc;
        }
    }
    std::vector<int32_t> world((size_t)(tested ? tested : 1));
    for (int q = 0; q < tested; q++) {
        list_probe[q] = spawn_fold(partials, ptiles, q, cap);
        world[(size_t)q] = spawn_world(list_probe[q], margin);
    }
    std::free(partials);
    for (int r = tested - 1; r >= 0; r--) {                                // (any order of the wavefronts: the walk reads no row)
        bool any = false;
        if (world[(size_t)r] == SCA_SPAWN_ADMITTED)
            for (int lane = 0; lane < 64; lane++) any = spawn_gate_walk(query.data(), world.data(), r, margin, lane, 64, L3Norm{}) || any;
        const int32_t v = spawn_verdict(world[(size_t)r], any);
        const int a = list_ids[r];
        const MissionGateSettle s = mission_gate_settle(v, list_entry[r], refusals[a]);
        waiting[a] = s.waiting; verdict[a] = s.verdict; refusals[a] = s.refusals;
        totals[s.counter] += 1;
        list_verdict[r] = v;
        if (s.take != (v == SCA_SPAWN_ADMITTED)) std::abort();
    }
    return total;
}

}  // namespace

extern "C" {

void mg_sizes(int *out) {
    out[0] = (int)sizeof(sca_mission_gate_totals); out[1] = SCA_SPAWN_OVER_CAP; out[2] = SPAWN_BATCH; out[3] = SPAWN_TILE; out[4] = FIN_TILE; out[5] = MGT_WORDS;
    out[6] = (int)(MISSION_GATE_MAX_SCRATCH >> 20);
}
// out: fault, its code, cap; scratch: the partials' bytes
void mg_check(int tables, int mid_step, int n, int m, int on, double margin, int32_t max_per_step, int *out, long long *scratch) {
    const MissionGateCheck k = mission_gate_check(tables != 0, mid_step != 0, n, m, on, margin, max_per_step);
    out[0] = k.fault; out[1] = mission_gate_error_code(k.fault); out[2] = k.cap;
    *scratch = k.scratch;
}
void mg_getter_checks(int tables, int ever, int n, int begin, int count, int have_outputs, int have_out, int struct_bytes, int *out4) {
    const MissionGateFault a = mission_gate_state_check(tables != 0, ever != 0, n, begin, count, have_outputs != 0);
    const MissionGateFault b = mission_gate_totals_check(tables != 0, ever != 0, have_out != 0, struct_bytes);
    out4[0] = a; out4[1] = mission_gate_error_code(a); out4[2] = b; out4[3] = mission_gate_error_code(b);
}
int mg_class(int32_t waiting, int fresh) { return mission_gate_class(waiting, fresh != 0); }
int mg_place(int cls, int rank, int waiting_total) { return mission_gate_place(cls, rank, waiting_total); }
void mg_query(const sca_mission *e, const double *pos, double radius, double *out4) {
    PubRec cur{};
    cur.px = pos[0]; cur.py = pos[1]; cur.pz = pos[2]; cur.radius = radius;
    const ClearPoint q = mission_gate_query(*e, cur);
    out4[0] = q.x; out4[1] = q.y; out4[2] = q.z; out4[3] = q.r;
}
void mg_settle(int32_t verdict, int32_t entry, int32_t refusals, int *out5) {
    const MissionGateSettle s = mission_gate_settle(verdict, entry, refusals);
    out5[0] = s.waiting; out5[1] = s.verdict; out5[2] = s.refusals; out5[3] = s.counter; out5[4] = s.take;
}
// one step's gate: pos [n][3], radius [n] the records behind the step; the lists have room for min(candidates, cap) <= cap entries
int mg_step(int n, int M, const sca_mission *entries, const double *pos, const double *radius, int m, const double *obs_pos, const double *obs_radius, double margin,
            int cap, int32_t *waiting, int32_t *verdict, int32_t *refusals, const int32_t *fresh, int32_t *list_ids, int32_t *list_entry, int32_t *list_verdict,
            sca_scene_clearance *list_probe, uint64_t *totals) {
    std::vector<PubRec> rec((size_t)n);
    for (int i = 0; i < n; i++) { rec[(size_t)i] = PubRec{}; rec[(size_t)i].px = pos[3 * i]; rec[(size_t)i].py = pos[3 * i + 1]; rec[(size_t)i].pz = pos[3 * i + 2]; rec[(size_t)i].radius = radius[i]; }
    return gate_step(n, M, entries, rec.data(), m, obs_pos, obs_radius, margin, cap, waiting, verdict, refusals, fresh, list_ids, list_entry, list_verdict, list_probe, totals);
}

}  // extern "C"

#ifdef MISSION_GATE_MAIN
template <class T> T *heap(size_t k, T v = T()) { T *p = (T *)std::malloc(sizeof(T) * (k ? k : 1)); for (size_t i = 0; i < k; i++) p[i] = v; return p; }
int main() {
    unsigned seed = 97531u;
    const auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (seed >> 8) / (double)(1u << 24); };
    int fails = 0;
    for (int trial = 0; trial < 60; trial++) {
        const int n = 1 + (int)(rnd() * 900), M = 1 + (int)(rnd() * 3), m = trial % 3 == 0 ? 0 : (int)(rnd() * 40);
        const int cap = trial % 4 == 0 ? mission_gate_cap(n, 0) : 1 + (int)(rnd() * n);
        const double side = 3.0 + rnd() * 12.0, margin = 0.5;
        sca_mission *e = heap<sca_mission>((size_t)M * n);
        for (int k = 0; k < M * n; k++) {
            std::memset(&e[k], 0, sizeof e[k]);
            for (int q = 0; q < 3; q++) e[k].pos[q] = rnd() * side;
            e[k].flags = (uint8_t)((int)(rnd() * 4));
        }
        double *pos = heap<double>(3 * (size_t)n), *radius = heap<double>(n, 0.4), *opos = heap<double>(3 * (size_t)m), *orad = heap<double>(m, 0.7);
        for (int i = 0; i < 3 * n; i++) pos[i] = rnd() * side;
        for (int i = 0; i < 3 * m; i++) opos[i] = rnd() * side;
        int32_t *waiting = heap<int32_t>(n, -1), *verdict = heap<int32_t>(n), *refusals = heap<int32_t>(n), *fresh = heap<int32_t>(n);
        uint64_t *totals = heap<uint64_t>(MGT_WORDS);
        uint64_t waiting_now = 0, arrived = 0;
        for (int step = 0; step < 4; step++) {
            int cand = 0;
            for (int i = 0; i < n; i++) {
                fresh[i] = 0;
                if (waiting[i] < 0 && rnd() < 0.3) { waiting[i] = (int)(rnd() * M); fresh[i] = 1; arrived++; }
                cand += waiting[i] >= 0;
            }
            const int room = cand < cap ? cand : cap;
            int32_t *ids = heap<int32_t>(room, -7), *ent = heap<int32_t>(room, -7), *ver = heap<int32_t>(room, -7);
            sca_scene_clearance *probe = heap<sca_scene_clearance>(room);
            const int got = mg_step(n, M, e, pos, radius, m, opos, orad, margin, cap, waiting, verdict, refusals, fresh, ids, ent, ver, probe, totals);
            if (got != cand) { std::printf("trial %d step %d: %d candidates, %d counted\n", trial, step, cand, got); fails++; }
            bool seen_new = false;
            for (int r = 0; r < room; r++) {                               // the order: waiting rows first, ascending ids inside a class
                const bool is_new = fresh[ids[r]] != 0;
                if (r > 0 && is_new == (fresh[ids[r - 1]] != 0) && ids[r] <= ids[r - 1]) { std::printf("trial %d step %d: order at %d\n", trial, step, r); fails++; break; }
                if (!is_new && seen_new) { std::printf("trial %d step %d: a waiting row behind a new one at %d\n", trial, step, r); fails++; break; }
                seen_new = seen_new || is_new;
                if ((ver[r] == SCA_SPAWN_ADMITTED) != (waiting[ids[r]] < 0)) { std::printf("trial %d step %d: words of %d\n", trial, step, ids[r]); fails++; break; }
            }
            std::free(ids); std::free(ent); std::free(ver); std::free(probe);
        }
        for (int i = 0; i < n; i++) waiting_now += waiting[i] >= 0;
        if (totals[MGT_OFFERED] != totals[MGT_ADMITTED] + totals[MGT_BLOCKED_AGENT] + totals[MGT_BLOCKED_OBSTACLE] + totals[MGT_BLOCKED_ENTRY] + totals[MGT_OVER_CAP] ||
            arrived != totals[MGT_ADMITTED] + waiting_now)
            { std::printf("trial %d: totals\n", trial); fails++; }
        std::free(e); std::free(pos); std::free(radius); std::free(opos); std::free(orad); std::free(waiting); std::free(verdict); std::free(refusals); std::free(fresh); std::free(totals);
    }
    std::printf(fails ? "mission_gate_harness: %d FAILED\n" : "mission_gate_harness: ok\n", fails);
    return fails ? 1 : 0;
}
#endif
