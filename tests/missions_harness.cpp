// The pure rules of sca_amd/csrc/sca_missions.h (and respawn_write_row of sca_respawn.h with a table entry as its source) behind C entry
// points (tests/test_missions_cpu.py), and -- with -DMISSIONS_MAIN -- as a program of its own for the sanitizers: every buffer on the heap
// in exactly the size the rules may touch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sca_missions.h"
#include "sca_forms.h"

using namespace sca;

namespace {

// the per-agent arrays a taken row writes, as plain host arrays of n rows (null: the context has none of it): respawn_write_row's Dev
struct Rows {
    int n;
    PubRec *rec;
    double *heading, *goal, *pref_speed, *max_run_dist, *total_dist, *vpref_ext;
    int32_t *step_num, *status, *nbr_n, *near_n;
    uint8_t *zaxis, *vpref_mode, *nbr_valid;
    double *trk_nbr0, *trk_goal_heading;
    int32_t *path_len, *path_rem;
    double *now_goal;
    sca_scene_clearance *clear;
    uint32_t *trk_st;
    const uint32_t *trk_init;
    int trk_words;
};
constexpr int TRK_WORDS = 5;
const uint32_t TRK_INIT[TRK_WORDS] = {11u, 22u, 33u, 44u, 55u};

// k_mission_advance wavefront by wavefront and lane by lane: the same order of reads and writes, the same functions
void advance_emulate(const Rows &d, int32_t *live, int M, int R, const uint8_t *policy, const sca_mission *entries, const int32_t *first_ok,
                     const int32_t *first_fail, int32_t *cursor, int32_t *flying, uint32_t *ended, sca_mission_result *results, uint64_t *totals, int64_t update,
                     int32_t *done_count) {
    const int n = d.n;
    totals[MST_UPDATES] += 1;
    for (int row0 = 0; row0 < n; row0 += 64) {
        int next[64], fly[64];
        uint32_t fn[64], en[64];
        unsigned long long todo = 0;
        bool end_tab[64];
        for (int lane = 0; lane < 64; lane++) {
            const int row = row0 + lane;
            end_tab[lane] = false; next[lane] = -1; fly[lane] = -1; fn[lane] = 0; en[lane] = 0;
            if (row >= n) continue;
            const uint32_t fo = live[row] ? 0u : RSP_DONE_FLAGS;
            fn[lane] = d.rec[row].flags;
            int ok = -1, fail = -1;
            const bool table = mission_has_table(first_ok[row], first_fail[row]);
            const int cur = cursor[row];
            if (table && cur >= 0) { const sca_mission &e = entries[(int64_t)M * row + cur]; ok = e.next_ok; fail = e.next_fail; }
            else if (table) { ok = first_ok[row]; fail = first_fail[row]; }
            const bool ended_now = mission_ended(fo, fn[lane]);
            const MissionTake t = mission_take(fn[lane], ok, fail);
            next[lane] = ended_now && table ? t.next : -1;
            if (!(fo & RSP_DONE_FLAGS)) totals[MST_AGENT_STEPS]++;
            if (ended_now) {
                totals[t.outcome == MISSION_ARRIVED ? MST_ARRIVED : t.outcome == MISSION_COLLIDED ? MST_COLLIDED : MST_TIMED_OUT]++;
                totals[next[lane] >= 0 ? MST_TAKEN : MST_STOPPED]++;
            }
            if (ended_now && table) { end_tab[lane] = true; en[lane] = ended[row]; fly[lane] = flying[row]; todo |= 1ull << lane; }
            live[row] = next[lane] >= 0 || !(fn[lane] & RSP_DONE_FLAGS) ? 1 : 0;
        }
        while (todo) {
            const int l0 = __builtin_ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int a = row0 + l0, nx = next[l0];
            sca_mission_result out;
            std::memset(&out, 0, sizeof out);
            out.id = a; out.entry = fly[l0]; out.flags = fn[l0]; out.step_num = d.step_num[a]; out.total_dist = d.total_dist[a];
            out.pos[0] = d.rec[a].px; out.pos[1] = d.rec[a].py; out.pos[2] = d.rec[a].pz;
            out.update = update; out.next = nx; out.reserved = 0;
            out.clear = d.clear ? d.clear[a] : scene_clearance_empty();
            results[(int64_t)R * a + (int)(en[l0] % (uint32_t)R)] = out;
            if (nx < 0) continue;
            const sca_mission *e = entries + ((int64_t)M * a + nx);
            const RespawnRow w = respawn_row(mission_bits(policy[a], d.trk_st != nullptr), fn[l0], mission_has(*e), 0);
            for (int lane = 0; lane < 64; lane++) respawn_write_row(d, a, lane, w, MissionSrc{e});
        }
        for (int lane = 0; lane < 64; lane++) {
            if (!end_tab[lane]) continue;
            const int row = row0 + lane;
            ended[row] = en[lane] + 1u;
            flying[row] = next[lane];
            if (next[lane] >= 0) { cursor[row] = next[lane]; done_count[(row & 255) * 32] += 1; }
        }
    }
}

// the collect's three kernels tile by tile: (row, ring slot) of every fresh result in order; returns the total; nothing is written or
// marked where the total exceeds the capacity
int collect_emulate(int n, int R, const uint32_t *ended, uint32_t *collected, int capacity, int32_t *out_row, int32_t *out_slot, int32_t *counts, int32_t *offsets) {
    const int tiles = finished_tiles(n);
    for (int t = 0; t < tiles; t++) {
        int c = 0;
        for (int i = 0; i < FIN_TILE; i++) { const int row = t * FIN_TILE + i; if (row < n) c += mission_new(ended[row], collected[row], R); }
        counts[t] = c;
    }
    const int total = finished_offsets(counts, tiles, offsets);
    if (total > capacity) return total;
    for (int t = 0; t < tiles; t++) {
        int before = 0;
        for (int i = 0; i < FIN_TILE; i++) {
            const int row = t * FIN_TILE + i;
            if (row >= n) break;
            const int fresh = mission_new(ended[row], collected[row], R);
            for (int k = 0; k < fresh; k++) { out_row[offsets[t] + before + k] = row; out_slot[offsets[t] + before + k] = mission_ring_slot(ended[row], fresh, k, R); }
            before += fresh;
            collected[row] = ended[row];
        }
    }
    return total;
}

MissionCtx ctx_of(const int *c) {
    MissionCtx X;
    X.agents = c[0]; X.mid_step = c[1]; X.scenes = c[2]; X.comm = c[3]; X.partition = c[4]; X.paths = c[5]; X.n = c[6]; X.shard_count = c[7];
    return X;
}

}  // namespace

extern "C" {

void msn_sizes(int *out) {
    out[0] = (int)sizeof(sca_mission); out[1] = (int)sizeof(sca_mission_result); out[2] = (int)sizeof(sca_mission_totals);
    out[3] = (int)offsetof(sca_mission, pref_speed); out[4] = (int)offsetof(sca_mission, vel); out[5] = (int)offsetof(sca_mission, next_ok);
    out[6] = (int)offsetof(sca_mission, flags); out[7] = (int)offsetof(sca_mission_result, update); out[8] = (int)offsetof(sca_mission_result, clear);
    out[9] = MISSION_MAX_M; out[10] = MISSION_MAX_R; out[11] = (int)MISSION_MAX_SLOTS; out[12] = SCA_MISSION_START_HERE; out[13] = SCA_MISSION_KEEP_ZAXIS;
    out[14] = MISSION_HEAD_BYTES; out[15] = FIN_TILE;
}
void msn_check(const int *c, int M, int R, int n, const sca_mission *entries, const int32_t *first_ok, const int32_t *first_fail, int64_t *out3, double *top, uint8_t *reached) {
    const MissionCheck k = mission_check(ctx_of(c), MissionArgs{M, R, n, entries, first_ok, first_fail}, reached);
    out3[0] = (int64_t)k.fault; out3[1] = k.entry; out3[2] = mission_error_code(k.fault);
    *top = k.max_pref_speed;
}
void msn_getter_checks(int agents, int on, int n, int have_out, int capacity, int have_count, int struct_bytes, int begin, int count, int have_cursor, int have_ended, int *out6) {
    const MissionFault a = mission_results_check(agents, on, have_out, capacity, have_count, struct_bytes);
    const MissionFault b = mission_totals_check(agents, on, have_out, struct_bytes);
    const MissionFault s = mission_state_check(agents, on, n, begin, count, have_cursor, have_ended);
    out6[0] = a; out6[1] = mission_error_code(a); out6[2] = b; out6[3] = mission_error_code(b); out6[4] = s; out6[5] = mission_error_code(s);
}
void msn_take(uint32_t old_flags, uint32_t new_flags, int ok, int fail, int *out3) {
    const MissionTake t = mission_take(new_flags, ok, fail);
    out3[0] = mission_ended(old_flags, new_flags); out3[1] = t.outcome; out3[2] = t.next;
}
// One env update's k_mission_advance on host arrays.  S: pos, vel, flags (the state behind K4; uint8), radius, heading, goal, pref_speed,
// max_run_dist, total_dist, step_num, status, nbr_n, near_n, zaxis, vpref_mode, nbr_valid, vpref_ext, trk_nbr0, trk_goal_heading, clear,
// trk_st ([n][TRK_WORDS] words), done_count ([256 * 32]) -- the last five nullable together with tracker_on / the records.
void msn_advance(int n, int M, int R, const uint8_t *policy, const sca_mission *entries, const int32_t *first_ok, const int32_t *first_fail, int32_t *cursor,
                 int32_t *flying, uint32_t *ended, void **S, const uint8_t *before, sca_mission_result *results, uint64_t *totals, int64_t update) {
    double *s_pos = (double *)S[0];
    float *s_vel = (float *)S[1];
    uint8_t *s_flags = (uint8_t *)S[2];
    double *s_radius = (double *)S[3];
    std::vector<PubRec> rec((size_t)n);
    std::vector<int32_t> live((size_t)n);
    for (int i = 0; i < n; i++) {
        rec[i].px = s_pos[3 * i]; rec[i].py = s_pos[3 * i + 1]; rec[i].pz = s_pos[3 * i + 2];
        rec[i].vx = s_vel[3 * i]; rec[i].vy = s_vel[3 * i + 1]; rec[i].vz = s_vel[3 * i + 2];
        rec[i].flags = s_flags[i]; rec[i].radius = s_radius[i];
        live[i] = (before[i] & RSP_DONE_FLAGS) ? 0 : 1;                  // (k_mission_live's rule on the flags the rows entered the step with)
    }
    Rows d{};
    d.n = n; d.rec = rec.data();
    d.heading = (double *)S[4]; d.goal = (double *)S[5]; d.pref_speed = (double *)S[6]; d.max_run_dist = (double *)S[7]; d.total_dist = (double *)S[8];
    d.step_num = (int32_t *)S[9]; d.status = (int32_t *)S[10]; d.nbr_n = (int32_t *)S[11]; d.near_n = (int32_t *)S[12];
    d.zaxis = (uint8_t *)S[13]; d.vpref_mode = (uint8_t *)S[14]; d.nbr_valid = (uint8_t *)S[15]; d.vpref_ext = (double *)S[16];
    d.trk_nbr0 = (double *)S[17]; d.trk_goal_heading = (double *)S[18]; d.clear = (sca_scene_clearance *)S[19];
    d.trk_st = (uint32_t *)S[20]; d.trk_init = TRK_INIT; d.trk_words = TRK_WORDS;
    advance_emulate(d, live.data(), M, R, policy, entries, first_ok, first_fail, cursor, flying, ended, results, totals, update, (int32_t *)S[21]);
    for (int i = 0; i < n; i++) if (live[i] != ((rec[i].flags & RSP_DONE_FLAGS) ? 0 : 1)) std::abort();   // the word the kernel leaves is k_mission_live's of the new records
    for (int i = 0; i < n; i++) {
        s_pos[3 * i] = rec[i].px; s_pos[3 * i + 1] = rec[i].py; s_pos[3 * i + 2] = rec[i].pz;
        s_vel[3 * i] = rec[i].vx; s_vel[3 * i + 1] = rec[i].vy; s_vel[3 * i + 2] = rec[i].vz;
        s_flags[i] = (uint8_t)rec[i].flags; s_radius[i] = rec[i].radius;
    }
}
int msn_trk_words(uint32_t *init) { for (int k = 0; k < TRK_WORDS; k++) init[k] = TRK_INIT[k]; return TRK_WORDS; }
int msn_collect(int n, int R, const uint32_t *ended, uint32_t *collected, int capacity, int32_t *out_row, int32_t *out_slot, int32_t *counts, int32_t *offsets) {
    return collect_emulate(n, R, ended, collected, capacity, out_row, out_slot, counts, offsets);
}
// plan_step with the StepIn fields in declaration order (ints), missions_on last; out: moved_on_action, build_ahead, fork_rides
void msn_plan_step(const int *i, int missions_on, int with_field, int *out3) {
    StepIn in{i[0], i[1], i[2], i[3] != 0, i[4] != 0, i[5] != 0, i[6] != 0, i[7] != 0, i[8] != 0, i[9] != 0, i[10] != 0, i[11] != 0, i[12] != 0, i[13] != 0, i[14] != 0,
              i[15], i[16], i[17], i[18]};                                 // (the aggregate initialiser of the callers that predate the field)
    if (with_field) in.missions_on = missions_on != 0;
    const StepPlan p = plan_step(in);
    out3[0] = p.moved_on_action; out3[1] = p.build_ahead; out3[2] = p.fork_rides;
}

}  // extern "C"

#ifdef MISSIONS_MAIN
// every array on the heap in exactly its size: a read or write beyond a row, a table, a ring or the collect's lists is the sanitizer's to find
template <class T> T *heap(size_t k, T v = T()) { T *p = (T *)std::malloc(sizeof(T) * (k ? k : 1)); for (size_t i = 0; i < k; i++) p[i] = v; return p; }
int main() {
    unsigned seed = 4321u;
    const auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (seed >> 8) / (double)(1u << 24); };
    int fails = 0;
    for (int trial = 0; trial < 120; trial++) {
        const int n = 1 + (int)(rnd() * 700), M = 1 + (int)(rnd() * 4), R = 1 + (int)(rnd() * 3), trk = trial % 2, clr = trial % 3 == 0;
        sca_mission *e = heap<sca_mission>((size_t)M * n);
        int32_t *fok = heap<int32_t>(n), *ffail = heap<int32_t>(n), *cursor = heap<int32_t>(n, -1), *flying = heap<int32_t>(n, -1);
        uint32_t *ended = heap<uint32_t>(n), *collected = heap<uint32_t>(n);
        uint8_t *policy = heap<uint8_t>(n);
        for (int i = 0; i < n; i++) { fok[i] = (int)(rnd() * (M + 1)) - 1; ffail[i] = (int)(rnd() * (M + 1)) - 1; policy[i] = (uint8_t)(rnd() * 6); }
        for (int k = 0; k < M * n; k++) {
            std::memset(&e[k], 0, sizeof e[k]);
            for (int q = 0; q < 3; q++) { e[k].pos[q] = rnd() * 10; e[k].goal[q] = rnd() * 10; e[k].heading[q] = rnd(); e[k].goal_heading[q] = rnd(); e[k].vel[q] = (float)rnd(); }
            e[k].pref_speed = 0.5 + rnd(); e[k].max_run_dist = 1.0 + rnd() * 9;
            e[k].next_ok = (int8_t)((int)(rnd() * (M + 1)) - 1); e[k].next_fail = (int8_t)((int)(rnd() * (M + 1)) - 1);
            e[k].zaxis = (uint8_t)(rnd() < 0.5); e[k].flags = (uint8_t)((int)(rnd() * 4));
        }
        const int c[8] = {1, 0, 0, 0, 0, 0, n, n};
        int64_t out3[3];
        double top;
        uint8_t *reached = heap<uint8_t>((size_t)M * n);
        msn_check(c, M, R, n, e, fok, ffail, out3, &top, reached);
        if (out3[0] != MSF_OK) { std::printf("trial %d: refused %d at %d\n", trial, (int)out3[0], (int)out3[1]); fails++; }
        double *pos = heap<double>(3 * n), *radius = heap<double>(n, 0.4), *heading = heap<double>(3 * n, 0.25), *goal = heap<double>(3 * n), *ps = heap<double>(n, 1.0);
        double *mrd = heap<double>(n, 5.0), *td = heap<double>(n, 3.0), *ext = heap<double>(3 * n, 7.0);
        float *vel = heap<float>(3 * n, 0.5f);
        uint8_t *flags = heap<uint8_t>(n), *before = heap<uint8_t>(n), *hit = heap<uint8_t>(n), *zaxis = heap<uint8_t>(n), *mode = heap<uint8_t>(n, 0), *valid = heap<uint8_t>(n, 1);
        int32_t *sn = heap<int32_t>(n, 5), *status = heap<int32_t>(n, 8), *nn = heap<int32_t>(n, 4), *near = heap<int32_t>(n, 2), *done = heap<int32_t>(256 * 32);
        double *nbr0 = trk ? heap<double>(n, 2.0) : nullptr, *tgh = trk ? heap<double>(3 * n) : nullptr;
        uint32_t *trk_st = trk ? heap<uint32_t>((size_t)TRK_WORDS * n, 9u) : nullptr;
        sca_scene_clearance *clear = clr ? heap<sca_scene_clearance>(n) : nullptr;
        sca_mission_result *ring = heap<sca_mission_result>((size_t)R * n);
        uint64_t *totals = heap<uint64_t>(MST_WORDS);
        for (int i = 0; i < 3 * n; i++) pos[i] = rnd() * 10;
        void *S[22] = {pos, vel, flags, radius, heading, goal, ps, mrd, td, sn, status, nn, near, zaxis, mode, valid, ext, nbr0, tgh, clear, trk_st, done};
        uint64_t endings = 0, with_table = 0;
        for (int step = 1; step <= 4; step++) {
            for (int i = 0; i < n; i++) {                                  // a step: some of the running rows end
                before[i] = flags[i]; hit[i] = 0;
                if (!flags[i] && rnd() < 0.4) { flags[i] = (uint8_t)(1 << (int)(rnd() * 3)); hit[i] = 1; endings++; with_table += mission_has_table(fok[i], ffail[i]); }
            }
            msn_advance(n, M, R, policy, e, fok, ffail, cursor, flying, ended, S, before, ring, totals, step);
            for (int i = 0; i < n; i++) {
                if (!hit[i] || !mission_has_table(fok[i], ffail[i])) continue;
                if (flags[i] == 0 && !(td[i] == 0.0 && sn[i] == 0 && status[i] == 0 && near[i] == -1 && valid[i] == 0 && radius[i] == 0.4 && cursor[i] >= 0 && cursor[i] == flying[i]))
                    { std::printf("trial %d step %d: taken row %d\n", trial, step, i); fails++; break; }
                // (a row that ended and was taken has flags 0 again; td / sn restart for the check of the next step)
                if (flags[i] == 0) { td[i] = 3.0; sn[i] = 5; status[i] = 8; near[i] = 2; valid[i] = 1; }
            }
        }
        uint64_t sum = 0;
        for (int i = 0; i < n; i++) sum += ended[i];
        if (totals[MST_ARRIVED] + totals[MST_COLLIDED] + totals[MST_TIMED_OUT] != endings || totals[MST_TAKEN] + totals[MST_STOPPED] != endings || sum != with_table || totals[MST_UPDATES] != 4)
            { std::printf("trial %d: totals\n", trial); fails++; }
        const int tiles = finished_tiles(n);
        int32_t *counts = heap<int32_t>(tiles), *offsets = heap<int32_t>(tiles);
        int want = 0;
        for (int i = 0; i < n; i++) want += mission_new(ended[i], collected[i], R);
        const int cap = trial % 4 == 3 ? want / 2 : want;
        int32_t *orow = heap<int32_t>(cap), *oslot = heap<int32_t>(cap);
        const int total = msn_collect(n, R, ended, collected, cap, orow, oslot, counts, offsets);
        if (total != want) { std::printf("trial %d: collect total %d, want %d\n", trial, total, want); fails++; }
        if (total <= cap) {
            for (int k = 1; k < total; k++) if (orow[k] < orow[k - 1]) { std::printf("trial %d: collect order\n", trial); fails++; break; }
            for (int k = 0; k < total; k++) if (ring[(int64_t)R * orow[k] + oslot[k]].id != orow[k]) { std::printf("trial %d: ring slot\n", trial); fails++; break; }
            if (msn_collect(n, R, ended, collected, cap, orow, oslot, counts, offsets) != 0) { std::printf("trial %d: collected twice\n", trial); fails++; }
        }
        for (void *p : {(void *)e, (void *)fok, (void *)ffail, (void *)cursor, (void *)flying, (void *)ended, (void *)collected, (void *)policy, (void *)reached, (void *)pos, (void *)radius,
                        (void *)heading, (void *)goal, (void *)ps, (void *)mrd, (void *)td, (void *)ext, (void *)vel, (void *)flags, (void *)before, (void *)hit, (void *)zaxis, (void *)mode, (void *)valid,
                        (void *)sn, (void *)status, (void *)nn, (void *)near, (void *)done, (void *)nbr0, (void *)tgh, (void *)trk_st, (void *)clear, (void *)ring, (void *)totals,
                        (void *)counts, (void *)offsets, (void *)orow, (void *)oslot})
            std::free(p);
    }
    std::printf(fails ? "missions_harness: %d failures\n" : "missions_harness: ok\n", fails);
    return fails ? 1 : 0;
}
#endif
