// Mission tables whose entries bring their own waypoint lists (sca_set_missions_paths) on the host: mission_paths_check and the take --
// mission_take_write of sca_amd/csrc/sca_missions.h, i.e. the shared row write (respawn_write_row) plus the shared list write
// (respawn_write_list of sca_respawn.h) -- behind C entry points (tests/test_mission_paths_cpu.py), and, with -DMISSION_PATHS_MAIN, as a
// program of its own for the sanitizers: every buffer on the heap in exactly the size the rules may touch, the rooms at exactly 24 W n bytes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sca_missions.h"

using namespace sca;

namespace {

// the per-agent arrays a taken row writes, as plain host arrays of n rows (null: the context has none of it): mission_take_write's Dev
struct Rows {
    int n;
    PubRec *rec;
    double *heading, *goal, *pref_speed, *max_run_dist, *total_dist, *vpref_ext;
    int32_t *step_num, *status, *nbr_n, *near_n;
    uint8_t *zaxis, *vpref_mode, *nbr_valid;
    double *trk_nbr0, *trk_goal_heading;
    double *path_pts, *now_goal;
    int32_t *path_len, *path_rem;
    int W;
    sca_scene_clearance *clear;
    uint32_t *trk_st;
    const uint32_t *trk_init;
    int trk_words;
};
constexpr int TRK_WORDS = 5;
const uint32_t TRK_INIT[TRK_WORDS] = {11u, 22u, 33u, 44u, 55u};

// the take of entry nx by row a as the wavefront does it: the loads of the row's old words (the flag word, the old length) in front of
// every store, then the 64 lanes' stores
void take_emulate(const Rows &d, int a, int nx, int M, const uint8_t *policy, const sca_mission *entries, bool lists, const int32_t *path_off, const double *path_pts,
                  int32_t *done_count) {
    const uint32_t flags = d.rec[a].flags;
    const int32_t old_len = lists ? d.path_len[a] : 0;
    const int64_t fe = (int64_t)M * a + nx;
    RespawnRow w{};
    for (int lane = 0; lane < 64; lane++) w = mission_take_write(d, a, lane, policy[a], flags, entries + fe, lists, old_len, path_off, path_pts, fe);
    if (w.done_delta) done_count[(a & 255) * 32] += w.done_delta;
}

}  // namespace

extern "C" {

// c: MissionCtx's agents, mid_step, scenes, comm, partition, paths, n, shard_count, path_W; out4: fault, entry, code, total
void mpt_check(const int *c, int M, int R, int n, const sca_mission *entries, const int32_t *first_ok, const int32_t *first_fail, const int32_t *path_off,
               const double *path_pts, int64_t *out4, double *top, uint8_t *reached) {
    MissionCtx X;
    X.agents = c[0]; X.mid_step = c[1]; X.scenes = c[2]; X.comm = c[3]; X.partition = c[4]; X.paths = c[5]; X.n = c[6]; X.shard_count = c[7]; X.path_W = c[8];
    const MissionPathsCheck k = mission_paths_check(X, MissionArgs{M, R, n, entries, first_ok, first_fail}, MissionPathArgs{path_off, path_pts}, reached);
    out4[0] = (int64_t)k.fault; out4[1] = k.entry; out4[2] = mission_error_code(k.fault); out4[3] = k.total;
    *top = k.max_pref_speed;
}
void mpt_get_check(int agents, int on, int have_outputs, int *out2) {
    const MissionFault f = mission_paths_get_check(agents, on, have_outputs);
    out2[0] = f; out2[1] = mission_error_code(f);
}
void mpt_consts(int64_t *out) {
    out[0] = MSF_STEP_HOST; out[1] = MSF_PATH_NO_SLOTS; out[2] = MSF_PATH_START; out[3] = MSF_PATH_DECREASING; out[4] = MSF_PATH_NO_POINTS; out[5] = MSF_PATH_TOTAL;
    out[6] = MSF_PATH_TOO_LONG; out[7] = MSF_PATH_NOT_FINITE; out[8] = MSF_PATH_CLEAR; out[9] = MISSION_PATH_MAX_POINTS; out[10] = mission_error_code(MSF_PATH_CLEAR);
    out[11] = RESPAWN_HAS_PATH_SLOTS | RESPAWN_HAS_PATHS; out[12] = RSP_BIT_MODE_RESET; out[13] = RSP_BIT_TRACKED;
}
// mission_take_bits / mission_take_has for one row; out: bits, has (with lists), has (without)
void mpt_bits(int policy, int tracker_on, int old_len, int entry_flags, int *out3) {
    sca_mission e;
    std::memset(&e, 0, sizeof e);
    e.flags = (uint8_t)entry_flags;
    out3[0] = mission_take_bits((uint8_t)policy, tracker_on != 0, old_len); out3[1] = (int)mission_take_has(e, true); out3[2] = (int)mission_take_has(e, false);
}
// The takes of one env update on host arrays: row ids[k] takes entry nxt[k].  S: pos, vel, flags (the state behind K4; uint8), radius,
// heading, goal, pref_speed, max_run_dist, total_dist, step_num, status, nbr_n, near_n, zaxis, vpref_mode, nbr_valid, vpref_ext, rooms
// ([3 W n]), path_len, path_rem, now_goal, trk_nbr0, trk_goal_heading, trk_st ([n][TRK_WORDS]; the last three null without a tracker),
// done_count ([256 * 32]).  lists 0: tables without lists -- no path word may move.
void mpt_take(int n, int M, int W, int lists, const uint8_t *policy, const sca_mission *entries, const int32_t *path_off, const double *path_pts, int count,
              const int32_t *ids, const int32_t *nxt, void **S) {
    double *s_pos = (double *)S[0];
    float *s_vel = (float *)S[1];
    uint8_t *s_flags = (uint8_t *)S[2];
    double *s_radius = (double *)S[3];
    std::vector<PubRec> rec((size_t)n);
    for (int i = 0; i < n; i++) {
        rec[i].px = s_pos[3 * i]; rec[i].py = s_pos[3 * i + 1]; rec[i].pz = s_pos[3 * i + 2];
        rec[i].vx = s_vel[3 * i]; rec[i].vy = s_vel[3 * i + 1]; rec[i].vz = s_vel[3 * i + 2];
        rec[i].flags = s_flags[i]; rec[i].radius = s_radius[i];
    }
    Rows d{};
    d.n = n; d.rec = rec.data();
    d.heading = (double *)S[4]; d.goal = (double *)S[5]; d.pref_speed = (double *)S[6]; d.max_run_dist = (double *)S[7]; d.total_dist = (double *)S[8];
    d.step_num = (int32_t *)S[9]; d.status = (int32_t *)S[10]; d.nbr_n = (int32_t *)S[11]; d.near_n = (int32_t *)S[12];
    d.zaxis = (uint8_t *)S[13]; d.vpref_mode = (uint8_t *)S[14]; d.nbr_valid = (uint8_t *)S[15]; d.vpref_ext = (double *)S[16];
    if (lists) { d.path_pts = (double *)S[17]; d.path_len = (int32_t *)S[18]; d.path_rem = (int32_t *)S[19]; d.now_goal = (double *)S[20]; d.W = W; }
    d.trk_nbr0 = (double *)S[21]; d.trk_goal_heading = (double *)S[22];
    d.trk_st = (uint32_t *)S[23]; d.trk_init = TRK_INIT; d.trk_words = TRK_WORDS;
    for (int k = 0; k < count; k++) take_emulate(d, ids[k], nxt[k], M, policy, entries, lists != 0, path_off, path_pts, (int32_t *)S[24]);
    for (int i = 0; i < n; i++) {
        s_pos[3 * i] = rec[i].px; s_pos[3 * i + 1] = rec[i].py; s_pos[3 * i + 2] = rec[i].pz;
        s_vel[3 * i] = rec[i].vx; s_vel[3 * i + 1] = rec[i].vy; s_vel[3 * i + 2] = rec[i].vz;
        s_flags[i] = (uint8_t)rec[i].flags; s_radius[i] = rec[i].radius;
    }
}
int mpt_trk_words(uint32_t *init) { for (int k = 0; k < TRK_WORDS; k++) init[k] = TRK_INIT[k]; return TRK_WORDS; }

}  // extern "C"

#ifdef MISSION_PATHS_MAIN
// every array on the heap in exactly its size: a read or write beyond a row, a table, the packed lists or a room is the sanitizer's to find
template <class T> T *heap(size_t k, T v = T()) { T *p = (T *)std::malloc(sizeof(T) * (k ? k : 1)); for (size_t i = 0; i < k; i++) p[i] = v; return p; }
int main() {
    unsigned seed = 97531u;
    const auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (seed >> 8) / (double)(1u << 24); };
    int fails = 0;
    for (int trial = 0; trial < 120; trial++) {
        const int n = 1 + (int)(rnd() * 400), M = 1 + (int)(rnd() * 4), W = 1 + (int)(rnd() * 4), trk = trial % 2;
        const size_t E = (size_t)M * n;
        sca_mission *e = heap<sca_mission>(E);
        int32_t *fok = heap<int32_t>(n), *ffail = heap<int32_t>(n);
        uint8_t *policy = heap<uint8_t>(n);
        for (int i = 0; i < n; i++) { fok[i] = (int)(rnd() * (M + 1)) - 1; ffail[i] = (int)(rnd() * (M + 1)) - 1; policy[i] = (uint8_t)(rnd() * 6); }
        for (size_t k = 0; k < E; k++) {
            std::memset(&e[k], 0, sizeof e[k]);
            for (int q = 0; q < 3; q++) { e[k].pos[q] = rnd() * 10; e[k].goal[q] = rnd() * 10; e[k].heading[q] = rnd(); e[k].goal_heading[q] = rnd(); e[k].vel[q] = (float)rnd(); }
            e[k].pref_speed = 0.5 + rnd(); e[k].max_run_dist = 1.0 + rnd() * 9;
            e[k].next_ok = (int8_t)((int)(rnd() * (M + 1)) - 1); e[k].next_fail = (int8_t)((int)(rnd() * (M + 1)) - 1);
            e[k].zaxis = (uint8_t)(rnd() < 0.5); e[k].flags = (uint8_t)((int)(rnd() * 4));
        }
        int32_t *off = heap<int32_t>(E + 1);
        for (size_t k = 0; k < E; k++) off[k + 1] = off[k] + (rnd() < 0.34 ? 0 : 1 + (int)(rnd() * W));       // 0 .. W points, W among them
        const int total = off[E];
        double *pts = heap<double>(3 * (size_t)total);
        for (int k = 0; k < 3 * total; k++) pts[k] = 100.0 + k;
        const int c[9] = {1, 0, 0, 0, 0, 1, n, n, W};
        int64_t out4[4];
        double top;
        uint8_t *reached = heap<uint8_t>(E);
        mpt_check(c, M, 2, n, e, fok, ffail, off, pts, out4, &top, reached);
        if (out4[0] != MSF_OK || out4[3] != total) { std::printf("trial %d: refused %d at %d\n", trial, (int)out4[0], (int)out4[1]); fails++; }
        if (total > 0) {                                                   // one refusal per trial, in turn; the arrays are left as they were
            const int which = trial % 3;
            size_t victim = 0;
            for (size_t k = 0; k < E; k++) if (reached[k] && off[k + 1] > off[k]) { victim = k + 1; break; }
            if (victim) {
                const size_t k = victim - 1;
                if (which == 0) {
                    const double keep = pts[3 * off[k]];
                    pts[3 * off[k]] = NAN;
                    mpt_check(c, M, 2, n, e, fok, ffail, off, pts, out4, &top, reached);
                    if (out4[0] != MSF_PATH_NOT_FINITE || out4[1] != (int64_t)k) { std::printf("trial %d: a NaN waypoint passed\n", trial); fails++; }
                    pts[3 * off[k]] = keep;
                } else if (which == 1) {
                    const int c2[9] = {1, 0, 0, 0, 0, 1, n, n, off[k + 1] - off[k] - 1};
                    mpt_check(c2, M, 2, n, e, fok, ffail, off, pts, out4, &top, reached);
                    if (off[k + 1] - off[k] > 1 && out4[0] != MSF_PATH_TOO_LONG) { std::printf("trial %d: a long list passed\n", trial); fails++; }
                } else {
                    mpt_check(c, M, 2, n, e, fok, ffail, off, nullptr, out4, &top, reached);
                    if (out4[0] != MSF_PATH_NO_POINTS) { std::printf("trial %d: NULL points passed\n", trial); fails++; }
                }
                mpt_check(c, M, 2, n, e, fok, ffail, off, pts, out4, &top, reached);
            }
        }
        double *pos = heap<double>(3 * (size_t)n), *radius = heap<double>(n, 0.4), *heading = heap<double>(3 * (size_t)n, 0.25), *goal = heap<double>(3 * (size_t)n), *ps = heap<double>(n, 1.0);
        double *mrd = heap<double>(n, 5.0), *td = heap<double>(n, 3.0), *ext = heap<double>(3 * (size_t)n, 7.0);
        float *vel = heap<float>(3 * (size_t)n, 0.5f);
        uint8_t *flags = heap<uint8_t>(n), *zaxis = heap<uint8_t>(n), *mode = heap<uint8_t>(n, 3), *valid = heap<uint8_t>(n, 1);
        int32_t *sn = heap<int32_t>(n, 5), *status = heap<int32_t>(n, 8), *nn = heap<int32_t>(n, 4), *near = heap<int32_t>(n, 2), *done = heap<int32_t>(256 * 32);
        double *rooms = heap<double>(3 * (size_t)W * n, -1.0);             // exactly 24 W n bytes
        int32_t *plen = heap<int32_t>(n), *prem = heap<int32_t>(n);
        double *ng = heap<double>(3 * (size_t)n, 4.0);
        double *nbr0 = trk ? heap<double>(n, 2.0) : nullptr, *tgh = trk ? heap<double>(3 * (size_t)n) : nullptr;
        uint32_t *trk_st = trk ? heap<uint32_t>((size_t)TRK_WORDS * n, 9u) : nullptr;
        for (int i = 0; i < n; i++) { plen[i] = (int)(rnd() * (W + 1)); prem[i] = (int)(rnd() * (plen[i] + 1)); }
        void *S[25] = {pos, vel, flags, radius, heading, goal, ps, mrd, td, sn, status, nn, near, zaxis, mode, valid, ext, rooms, plen, prem, ng, nbr0, tgh, trk_st, done};
        int32_t *ids = heap<int32_t>(n), *nxt = heap<int32_t>(n), *old = heap<int32_t>(n);
        for (int round = 0; round < 3; round++) {
            int count = 0;
            for (int i = 0; i < n; i++) {                                  // some rows end and take a reachable entry: a first successor
                const int j = rnd() < 0.5 ? fok[i] : ffail[i];
                old[i] = plen[i];
                if (j < 0 || rnd() < 0.5) continue;
                flags[i] = (uint8_t)(1 << (int)(rnd() * 3));
                ids[count] = i; nxt[count] = j; count++;
            }
            mpt_take(n, M, W, 1, policy, e, off, pts, count, ids, nxt, S);
            for (int k = 0; k < count; k++) {
                const int a = ids[k];
                const size_t fe = (size_t)M * a + nxt[k];
                const int len = off[fe + 1] - off[fe];
                const bool tracked = trk && (policy[a] == 0 || policy[a] == 5), straight = !(policy[a] == 0 || policy[a] == 5);
                bool ok = flags[a] == 0 && plen[a] == len && prem[a] == len && std::isnan(ng[3 * a]) && std::isnan(ng[3 * a + 1]) && std::isnan(ng[3 * a + 2]);
                for (int q = 0; q < 3 * len; q++) ok = ok && rooms[3 * (size_t)W * a + q] == pts[3 * (size_t)off[fe] + q];
                ok = ok && mode[a] == (tracked ? 1 : straight && old[a] > 0 ? 0 : 3);
                if (!ok) { std::printf("trial %d round %d: taken row %d\n", trial, round, a); fails++; break; }
                mode[a] = 3;
            }
        }
        for (void *p : {(void *)e, (void *)fok, (void *)ffail, (void *)policy, (void *)off, (void *)pts, (void *)reached, (void *)pos, (void *)radius, (void *)heading, (void *)goal,
                        (void *)ps, (void *)mrd, (void *)td, (void *)ext, (void *)vel, (void *)flags, (void *)zaxis, (void *)mode, (void *)valid, (void *)sn, (void *)status, (void *)nn,
                        (void *)near, (void *)done, (void *)rooms, (void *)plen, (void *)prem, (void *)ng, (void *)nbr0, (void *)tgh, (void *)trk_st, (void *)ids, (void *)nxt, (void *)old})
            std::free(p);
    }
    std::printf(fails ? "mission_paths_harness: %d failures\n" : "mission_paths_harness: ok\n", fails);
    return fails ? 1 : 0;
}
#endif
