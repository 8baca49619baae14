// The pure rules of sca_amd/csrc/sca_respawn.h behind C entry points (tests/test_respawn_cpu.py), and -- with -DRESPAWN_MAIN -- as a
// program of its own for the sanitizers: every buffer on the heap in exactly the size the rules may touch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sca_respawn.h"

using namespace sca;

namespace {

RespawnCtx ctx_of(const int *c, const uint8_t *policy) {
    RespawnCtx X;
    X.agents = c[0]; X.state = c[1]; X.mid_step = c[2]; X.scenes = c[3]; X.comm = c[4]; X.partition = c[5];
    X.n = c[6]; X.shard_count = c[7]; X.tracker_on = c[8]; X.paths_block = c[9]; X.path_W = c[10];
    X.policy_now = policy;
    return X;
}

// the per-agent arrays a call writes, as plain host arrays of n rows (null: the context has none of it)
struct Rows {
    int n;
    PubRec *rec;
    double *heading, *goal, *pref_speed, *max_run_dist, *total_dist, *vpref_ext;
    int32_t *step_num, *status, *nbr_n, *near_n;
    uint8_t *zaxis, *vpref_mode, *nbr_valid;
    double *trk_nbr0, *trk_goal_heading;
    int32_t *path_len, *path_rem;
    double *now_goal, *path_pts;
    int W;
};

// k_respawn's body for packed row r, lane by lane where the kernel spreads a store over lanes; returns done_delta; *tracked: the row takes
// the initial tracker record
int apply_row(const Rows &d, const uint8_t *blk, const RespawnLayout &L, uint32_t has, int r, int *tracked) {
    const int a = ((const int32_t *)(blk + L.off[RSB_IDS]))[r];
    const bool lists = (has & RESPAWN_HAS_PATHS) != 0;
    const int32_t *poff = (const int32_t *)(blk + L.off[RSB_PATH_OFF]);
    const int32_t first = lists ? poff[r] : 0, len = lists ? poff[r + 1] - first : 0;
    const RespawnRow w = respawn_row((blk + L.off[RSB_BITS])[r], d.rec[a].flags, has, len);
    for (int lane = 0; lane < RSP_REC_BYTES / 16; lane++) std::memcpy((uint8_t *)(d.rec + a) + 16 * lane, blk + L.off[RSB_REC] + (int64_t)RSP_REC_BYTES * r + 16 * lane, 16);
    for (int lane = 0; lane < 3; lane++) {
        const int64_t g = 3 * (int64_t)a + lane, s = 3 * (int64_t)r + lane;
        d.heading[g] = ((const double *)(blk + L.off[RSB_HEADING]))[s];
        d.goal[g] = ((const double *)(blk + L.off[RSB_GOAL]))[s];
        if (w.tracked) { d.vpref_ext[g] = 0.0; if (d.trk_goal_heading) d.trk_goal_heading[g] = ((const double *)(blk + L.off[RSB_GOAL_HEADING]))[s]; }
        if (w.path_len >= 0 && d.now_goal) d.now_goal[g] = __builtin_nan("");
    }
    d.total_dist[a] = w.total_dist; d.step_num[a] = w.step_num; d.status[a] = w.status;
    d.pref_speed[a] = ((const double *)(blk + L.off[RSB_PREF_SPEED]))[r];
    d.max_run_dist[a] = ((const double *)(blk + L.off[RSB_MAX_RUN_DIST]))[r];
    if (w.write_zaxis) d.zaxis[a] = (blk + L.off[RSB_ZAXIS])[r];
    if (w.write_mode) d.vpref_mode[a] = w.mode;
    d.nbr_n[a] = w.nbr_n; d.nbr_valid[a] = w.nbr_valid; d.near_n[a] = w.near_n;
    if (d.trk_nbr0) d.trk_nbr0[a] = w.nbr0;
    if (w.path_len >= 0 && d.path_len) { d.path_len[a] = w.path_len; d.path_rem[a] = w.path_len; }
    if (w.path_len > 0 && d.path_pts)
        for (int k = 0; k < 3 * w.path_len; k++) d.path_pts[3 * path_slot_index(d.W, a) + k] = ((const double *)(blk + L.off[RSB_PATH_PTS]))[3 * (int64_t)first + k];
    *tracked = w.tracked;
    return w.done_delta;
}

// the three kernels of the finished list, wavefront by wavefront: ids of the finished rows in order, at most `capacity` written; returns the total
int finished_emulate(int n, const uint32_t *flags, int capacity, int32_t *ids_out, int32_t *counts, int32_t *offsets) {
    const int tiles = finished_tiles(n);
    const auto ballot = [&](int row0) {
        unsigned long long m = 0;
        for (int lane = 0; lane < 64; lane++) if (row0 + lane < n && finished_flag(flags[row0 + lane])) m |= 1ull << lane;
        return m;
    };
    for (int t = 0; t < tiles; t++) {
        int c = 0;
        for (int wv = 0; wv < FIN_TILE / 64; wv++) c += __builtin_popcountll(ballot(t * FIN_TILE + 64 * wv));
        counts[t] = c;
    }
    const int total = finished_offsets(counts, tiles, offsets);
    for (int t = 0; t < tiles; t++) {
        int before = 0;
        for (int wv = 0; wv < FIN_TILE / 64; wv++) {
            const unsigned long long m = ballot(t * FIN_TILE + 64 * wv);
            for (int lane = 0; lane < 64; lane++) {
                if (!((m >> lane) & 1ull)) continue;
                const int at = offsets[t] + before + finished_rank(m, lane);
                if (at < capacity) ids_out[at] = t * FIN_TILE + 64 * wv + lane;
            }
            before += __builtin_popcountll(m);
        }
    }
    return total;
}

}  // namespace

extern "C" {

void rsp_check(const int *c, const uint8_t *policy, int count, const int32_t *ids, const double *pos, const float *vel, const double *heading,
               const double *radius, const double *pref_speed, const double *goal, const uint8_t *zaxis, const double *max_run_dist,
               const double *goal_heading, const int32_t *path_offsets, const double *path_points, int *out4) {
    const RespawnArgs A{count, ids, pos, vel, heading, radius, pref_speed, goal, zaxis, max_run_dist, goal_heading, path_offsets, path_points};
    const RespawnCheck k = respawn_check(ctx_of(c, policy), A);
    out4[0] = (int)k.fault; out4[1] = k.entry; out4[2] = respawn_error_code(k.fault); out4[3] = k.path_total;
}
void rsp_finished_check(const int *c, int have_rows, int capacity, int have_count, int struct_bytes, int *out2) {
    const RespawnFault f = finished_check(ctx_of(c, nullptr), have_rows != 0, capacity, have_count != 0, struct_bytes);
    out2[0] = (int)f; out2[1] = respawn_error_code(f);
}
int rsp_sections(void) { return RSB_SECTIONS; }
int rsp_tile(void) { return FIN_TILE; }
int rsp_finished_row_bytes(void) { return (int)sizeof(sca_finished_row); }
void rsp_layout(int cap, int W, int64_t *off, int64_t *total) {
    const RespawnLayout L = respawn_layout(cap, W);
    for (int s = 0; s < RSB_SECTIONS; s++) off[s] = L.off[s];
    *total = L.total;
}
// One whole call on host arrays (the state of n agents: pos / vel / flags / radius as separate arrays, packed into public records here):
// respawn_pack into a heap block of exactly the layout's size, then apply_row per named row.  words: per agent total_dist, and ints
// step_num, status, nbr_n, near_n as [n] arrays; modes: vpref_mode, nbr_valid, zaxis.  Returns the sum of done_delta.
int rsp_apply(const int *c, const uint8_t *policy, const uint8_t *path_vpref, int count, const int32_t *ids, const double *pos, const float *vel,
              const double *heading, const double *radius, const double *pref_speed, const double *goal, const uint8_t *zaxis, const double *max_run_dist,
              const double *goal_heading, const int32_t *path_offsets, const double *path_points,
              double *s_pos, float *s_vel, uint8_t *s_flags, double *s_radius, double *s_heading, double *s_goal, double *s_pref_speed, double *s_max_run_dist,
              double *s_total_dist, int32_t *s_step_num, int32_t *s_status, int32_t *s_nbr_n, int32_t *s_near_n, uint8_t *s_zaxis, uint8_t *s_vpref_mode,
              uint8_t *s_nbr_valid, double *s_vpref_ext, double *s_trk_nbr0, double *s_trk_goal_heading, int32_t *s_path_len, int32_t *s_path_rem,
              double *s_now_goal, double *s_path_pts, int32_t *tracked_out) {
    const RespawnCtx X = ctx_of(c, policy);
    const RespawnArgs A{count, ids, pos, vel, heading, radius, pref_speed, goal, zaxis, max_run_dist, goal_heading, path_offsets, path_points};
    const RespawnLayout L = respawn_layout(count, X.path_W);
    uint8_t *blk = (uint8_t *)std::malloc((size_t)L.total);
    const uint32_t has = respawn_pack(blk, L, X, A, path_vpref);
    const int n = X.n;
    std::vector<PubRec> rec((size_t)n);
    for (int i = 0; i < n; i++) {
        rec[i].px = s_pos[3 * i]; rec[i].py = s_pos[3 * i + 1]; rec[i].pz = s_pos[3 * i + 2];
        rec[i].vx = s_vel[3 * i]; rec[i].vy = s_vel[3 * i + 1]; rec[i].vz = s_vel[3 * i + 2];
        rec[i].flags = s_flags[i]; rec[i].radius = s_radius[i];
    }
    const Rows d{n, rec.data(), s_heading, s_goal, s_pref_speed, s_max_run_dist, s_total_dist, s_vpref_ext, s_step_num, s_status, s_nbr_n, s_near_n,
                 s_zaxis, s_vpref_mode, s_nbr_valid, s_trk_nbr0, s_trk_goal_heading, s_path_len, s_path_rem, s_now_goal, s_path_pts, X.path_W};
    int delta = 0;
    for (int r = 0; r < count; r++) delta += apply_row(d, blk, L, has, r, tracked_out + r);
    for (int i = 0; i < n; i++) {
        s_pos[3 * i] = rec[i].px; s_pos[3 * i + 1] = rec[i].py; s_pos[3 * i + 2] = rec[i].pz;
        s_vel[3 * i] = rec[i].vx; s_vel[3 * i + 1] = rec[i].vy; s_vel[3 * i + 2] = rec[i].vz;
        s_flags[i] = (uint8_t)rec[i].flags; s_radius[i] = rec[i].radius;
    }
    std::free(blk);
    return delta;
}
int rsp_finished(int n, const uint32_t *flags, int capacity, int32_t *ids_out, int32_t *counts, int32_t *offsets) {
    return finished_emulate(n, flags, capacity, ids_out, counts, offsets);
}

}  // extern "C"

#ifdef RESPAWN_MAIN
// every array on the heap in exactly its size: a read or write beyond a row, the block or the list's room is the sanitizer's to find
template <class T> T *heap(size_t k, T v = T()) { T *p = (T *)std::malloc(sizeof(T) * (k ? k : 1)); for (size_t i = 0; i < k; i++) p[i] = v; return p; }
int main() {
    unsigned seed = 12345u;
    const auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (seed >> 8) / (double)(1u << 24); };
    int fails = 0;
    for (int trial = 0; trial < 200; trial++) {
        const int n = 1 + (int)(rnd() * 700), W = trial % 3 == 0 ? 0 : 1 + (int)(rnd() * 4), trk = trial % 2;
        const int count = 1 + (int)(rnd() * n);
        const int c[11] = {1, 1, 0, 0, 0, 0, n, n, trk, 0, W};
        uint8_t *policy = heap<uint8_t>(n), *path_vpref = heap<uint8_t>(n);
        for (int i = 0; i < n; i++) { policy[i] = (uint8_t)(rnd() * 6); path_vpref[i] = W > 0 && rnd() < 0.3 && policy[i] != 0 && policy[i] != 5; }
        int32_t *ids = heap<int32_t>(count);
        {   // `count` distinct ids in a shuffled order
            std::vector<int32_t> all((size_t)n);
            for (int i = 0; i < n; i++) all[i] = i;
            for (int i = n - 1; i > 0; i--) std::swap(all[i], all[(int)(rnd() * (i + 1))]);
            for (int r = 0; r < count; r++) ids[r] = all[r];
        }
        double *pos = heap<double>(3 * count), *heading = heap<double>(3 * count), *goal = heap<double>(3 * count), *gh = heap<double>(3 * count);
        float *vel = heap<float>(3 * count);
        double *radius = heap<double>(count, 0.5), *ps = heap<double>(count, 1.0), *mrd = heap<double>(count, 9.0);
        uint8_t *zaxis = trial % 4 == 1 ? nullptr : heap<uint8_t>(count, 1);
        for (int k = 0; k < 3 * count; k++) { pos[k] = rnd() * 10; heading[k] = rnd(); goal[k] = rnd() * 10; gh[k] = rnd(); vel[k] = (float)rnd(); }
        int32_t *poff = nullptr;
        double *ppts = nullptr;
        if (W > 0 && trial % 5 != 0) {
            poff = heap<int32_t>(count + 1);
            for (int r = 0; r < count; r++) poff[r + 1] = poff[r] + (int)(rnd() * (W + 1));
            ppts = heap<double>(3 * (size_t)poff[count], 1.5);
        }
        int out4[4];
        rsp_check(c, policy, count, ids, pos, vel, heading, radius, ps, goal, zaxis, mrd, gh, poff, ppts, out4);
        if (out4[0] != RSP_OK) { std::printf("trial %d: refused %d at %d\n", trial, out4[0], out4[1]); fails++; continue; }
        double *s_pos = heap<double>(3 * n), *s_radius = heap<double>(n, 0.3), *s_heading = heap<double>(3 * n), *s_goal = heap<double>(3 * n);
        float *s_vel = heap<float>(3 * n);
        uint8_t *s_flags = heap<uint8_t>(n), *s_zaxis = heap<uint8_t>(n), *s_mode = heap<uint8_t>(n, 1), *s_valid = heap<uint8_t>(n, 1);
        for (int i = 0; i < n; i++) s_flags[i] = (uint8_t)(rnd() < 0.5 ? 1 << (int)(rnd() * 3) : 0);
        double *s_ps = heap<double>(n), *s_mrd = heap<double>(n), *s_td = heap<double>(n, 3.0), *s_ext = heap<double>(3 * n, 7.0);
        int32_t *s_sn = heap<int32_t>(n, 5), *s_st = heap<int32_t>(n, 8), *s_nn = heap<int32_t>(n, 4), *s_near = heap<int32_t>(n, 2);
        double *s_nbr0 = trk ? heap<double>(n, 2.0) : nullptr, *s_tgh = trk ? heap<double>(3 * n) : nullptr;
        int32_t *s_len = W ? heap<int32_t>(n) : nullptr, *s_rem = W ? heap<int32_t>(n) : nullptr;
        double *s_ng = W ? heap<double>(3 * n) : nullptr, *s_pts = W ? heap<double>(3 * (size_t)W * n) : nullptr;
        int32_t *tracked = heap<int32_t>(count);
        int done = 0;
        for (int r = 0; r < count; r++) done += s_flags[ids[r]] != 0;
        const int delta = rsp_apply(c, policy, path_vpref, count, ids, pos, vel, heading, radius, ps, goal, zaxis, mrd, gh, poff, ppts, s_pos, s_vel, s_flags, s_radius,
                                    s_heading, s_goal, s_ps, s_mrd, s_td, s_sn, s_st, s_nn, s_near, s_zaxis, s_mode, s_valid, s_ext, s_nbr0, s_tgh, s_len, s_rem, s_ng, s_pts, tracked);
        if (delta != done) { std::printf("trial %d: done_delta %d, %d rows were done\n", trial, delta, done); fails++; }
        for (int r = 0; r < count; r++) {
            const int a = ids[r];
            const bool t = trk && (policy[a] == 0 || policy[a] == 5);
            bool ok = s_flags[a] == 0 && s_radius[a] == 0.5 && s_td[a] == 0.0 && s_sn[a] == 0 && s_st[a] == 0 && s_nn[a] == 0 && s_near[a] == -1 && s_valid[a] == 0 &&
                      s_pos[3 * a + 1] == pos[3 * r + 1] && s_vel[3 * a + 2] == vel[3 * r + 2] && s_goal[3 * a] == goal[3 * r] && s_heading[3 * a + 2] == heading[3 * r + 2] &&
                      tracked[r] == (int)t && s_zaxis[a] == (zaxis ? 1 : 0) && s_mode[a] == (t ? 1 : path_vpref[a] ? 0 : 1) && (t ? s_ext[3 * a] == 0.0 : s_ext[3 * a] == 7.0);
            if (trk) ok = ok && s_nbr0[a] == -1.0 && (!t || s_tgh[3 * a + 1] == gh[3 * r + 1]);
            if (W) ok = ok && s_len[a] == (poff ? poff[r + 1] - poff[r] : 0) && s_rem[a] == s_len[a] && std::isnan(s_ng[3 * a]) && (s_len[a] == 0 || s_pts[3 * (size_t)W * a] == 1.5);
            if (!ok) { std::printf("trial %d: row %d (agent %d)\n", trial, r, a); fails++; break; }
        }
        // the finished list over the flags as they stand now
        uint32_t *fl = heap<uint32_t>(n);
        for (int i = 0; i < n; i++) fl[i] = s_flags[i];
        const int tiles = finished_tiles(n), cap = trial % 3 == 2 ? n / 3 : n;
        int32_t *out = heap<int32_t>(cap), *counts = heap<int32_t>(tiles), *offsets = heap<int32_t>(tiles);
        const int total = rsp_finished(n, fl, cap, out, counts, offsets);
        int at = 0;
        for (int i = 0; i < n; i++) if (fl[i] & 7u) { if (at < cap && out[at] != i) { std::printf("trial %d: finished[%d] = %d, want %d\n", trial, at, out[at], i); fails++; break; } at++; }
        if (at != total) { std::printf("trial %d: finished count %d, want %d\n", trial, total, at); fails++; }
        for (void *p : {(void *)policy, (void *)path_vpref, (void *)ids, (void *)pos, (void *)heading, (void *)goal, (void *)gh, (void *)vel, (void *)radius, (void *)ps, (void *)mrd,
                        (void *)zaxis, (void *)poff, (void *)ppts, (void *)s_pos, (void *)s_radius, (void *)s_heading, (void *)s_goal, (void *)s_vel, (void *)s_flags, (void *)s_zaxis,
                        (void *)s_mode, (void *)s_valid, (void *)s_ps, (void *)s_mrd, (void *)s_td, (void *)s_ext, (void *)s_sn, (void *)s_st, (void *)s_nn, (void *)s_near,
                        (void *)s_nbr0, (void *)s_tgh, (void *)s_len, (void *)s_rem, (void *)s_ng, (void *)s_pts, (void *)tracked, (void *)fl, (void *)out, (void *)counts, (void *)offsets})
            std::free(p);
    }
    std::printf(fails ? "respawn_harness: %d failures\n" : "respawn_harness: ok\n", fails);
    return fails ? 1 : 0;
}
#endif
