// The pure rules of sca_amd/csrc/sca_respawn_attrs.h behind C entry points (tests/test_respawn_attrs_cpu.py), and -- with
// -DRESPAWN_ATTRS_MAIN -- as a program of its own for the sanitizers: every buffer on the heap in exactly the size the rules may touch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sca_respawn_attrs.h"

using namespace sca;

namespace {

RespawnCtx ctx_of(const int *c, const uint8_t *policy) {
    RespawnCtx X;
    X.agents = c[0]; X.state = c[1]; X.mid_step = c[2]; X.scenes = c[3]; X.comm = c[4]; X.partition = c[5];
    X.n = c[6]; X.shard_count = c[7]; X.tracker_on = c[8]; X.paths_block = c[9]; X.path_W = c[10];
    X.policy_now = policy;
    return X;
}
// the arrays a call writes, as plain host arrays of n rows: RespawnDev's members (null: the context has none of it) ...
struct Rows {
    PubRec *rec;
    double *heading, *goal, *pref_speed, *max_run_dist, *total_dist, *vpref_ext;
    int32_t *step_num, *status, *nbr_n, *near_n;
    uint8_t *zaxis, *vpref_mode, *nbr_valid;
    double *trk_nbr0, *trk_goal_heading;
    uint32_t *trk_st;
    const uint32_t *trk_init;
    int trk_words;
    double *path_pts, *now_goal;
    int32_t *path_len, *path_rem;
    int W;
    sca_scene_clearance *clear;
    int n;
};
// ... and RespawnAttrDev's
struct AttrRows { uint8_t *policy; AgentPar *ap; double *ap_nd; double *trk_R, *trk_plo, *trk_phi; uint8_t *trk_cls; };
const AttrDefaults DEFAULTS{10.0, 0.1, 10.0, 1.0, 3.14159265358979323846 / 4, 0.1, 16, 1.5, -0.785, 0.785};

// k_respawn_attrs' body for packed row r: the 64 lanes one after the other; returns done_delta
int serve_row(const Rows &d, const AttrRows &at, const uint8_t *blk, const RespawnLayout &L, const uint8_t *ablk, const RespawnAttrLayout &AL, uint32_t has, int r) {
    const int a = ((const int32_t *)(blk + L.off[RSB_IDS]))[r];
    const uint8_t bits = (blk + L.off[RSB_BITS])[r];
    const RespawnRow w = respawn_row(bits, d.rec[a].flags, has, 0);
    for (int lane = 0; lane < 64; lane++) {
        respawn_write_row(d, a, lane, w, RespawnBlockSrc{blk, L, r});
        respawn_attrs_write_row(d, at, a, lane, bits, has, RespawnAttrSrc{ablk, AL, r});
    }
    return w.done_delta;
}

}  // namespace

extern "C" {

int rsa_sections(void) { return RAB_SECTIONS; }
void rsa_layout(int cap, int64_t *off, int64_t *total) {
    const RespawnAttrLayout L = respawn_attrs_layout(cap);
    for (int s = 0; s < RAB_SECTIONS; s++) off[s] = L.off[s];
    *total = L.total;
}
// respawn_attrs_check over a call whose other arrays are valid (radius: nullable, the one hook into respawn_check's own refusals).
// out: base fault, base entry, base code, fault, entry, code; merged: [n]
void rsa_check(const int *c, const uint8_t *policy_now, int count, const int32_t *ids, const uint8_t *policy, const sca_restart_attrs *attrs,
               const double *radius, int have_goal_heading, int *out6, uint8_t *merged_out) {
    const size_t k = (size_t)(count > 0 ? count : 1);
    std::vector<double> three(3 * k, 1.0), one(k, 1.0);
    std::vector<float> vel(3 * k, 0.0f);
    const RespawnArgs A{count, ids, three.data(), vel.data(), three.data(), radius, one.data(), three.data(), nullptr, one.data(),
                        have_goal_heading ? three.data() : nullptr, nullptr, nullptr};
    std::vector<uint8_t> merged;
    RestartAttrs R;
    const RespawnAttrCheck q = respawn_attrs_check(ctx_of(c, policy_now), A, policy, attrs, DEFAULTS, merged, &R);
    out6[0] = (int)q.base.fault; out6[1] = q.base.entry; out6[2] = respawn_error_code(q.base.fault);
    out6[3] = (int)q.fault; out6[4] = q.entry; out6[5] = respawn_attrs_error_code(q.fault);
    if (merged_out && !merged.empty()) std::memcpy(merged_out, merged.data(), merged.size());
}
// One whole call on host arrays: respawn_pack and respawn_attrs_pack into heap blocks of exactly the layouts' sizes, respawn_attrs_bits, then
// serve_row per named row.  policy / par: nullable.  s_*: the state of n agents (pos / vel / flags / radius packed into public records
// here).  path_vpref: [n].  trk: the tracker's arrays exist (trk_words words per record, all of s_trk_init).  Returns the sum of done_delta.
int rsa_apply(const int *c, const uint8_t *policy_now, const uint8_t *path_vpref, int count, const int32_t *ids, const uint8_t *policy, const AgentPar *par,
              const double *pos, const float *vel, const double *heading, const double *radius, const double *pref_speed, const double *goal,
              const double *max_run_dist, const double *goal_heading,
              double *s_pos, float *s_vel, uint8_t *s_flags, double *s_radius, double *s_heading, double *s_goal, double *s_pref_speed, double *s_max_run_dist,
              double *s_total_dist, int32_t *s_step_num, int32_t *s_status, int32_t *s_nbr_n, int32_t *s_near_n, uint8_t *s_zaxis, uint8_t *s_vpref_mode,
              uint8_t *s_nbr_valid, double *s_vpref_ext, double *s_trk_nbr0, double *s_trk_goal_heading, uint32_t *s_trk_st, const uint32_t *s_trk_init, int trk_words,
              uint8_t *s_policy, AgentPar *s_ap, double *s_ap_nd, uint8_t *bits_out,
              const double *trip3, const uint8_t *cls, double *s_R, double *s_plo, double *s_phi, uint8_t *s_cls) {
    RespawnCtx X = ctx_of(c, policy_now);
    const int n = X.n;
    std::vector<uint8_t> merged(policy_now, policy_now + n);
    if (policy) for (int r = 0; r < count; r++) merged[(size_t)ids[r]] = policy[r];
    X.policy_now = merged.data();
    const RespawnArgs A{count, ids, pos, vel, heading, radius, pref_speed, goal, nullptr, max_run_dist, goal_heading, nullptr, nullptr};
    const RespawnLayout L = respawn_layout(count, 0);
    const RespawnAttrLayout AL = respawn_attrs_layout(count);
    uint8_t *blk = (uint8_t *)std::aligned_alloc(64, (size_t)L.total), *ablk = (uint8_t *)std::aligned_alloc(64, (size_t)AL.total);
    uint32_t has = respawn_pack(blk, L, X, A, path_vpref);
    std::vector<TrackTriple> trip;
    if (trip3) for (int r = 0; r < count; r++) trip.push_back(TrackTriple{trip3[3 * r], trip3[3 * r + 1], trip3[3 * r + 2]});
    has |= respawn_attrs_pack(ablk, AL, count, policy, par, trip3 ? trip.data() : nullptr, cls);
    if (policy) respawn_attrs_bits(blk + L.off[RSB_BITS], count, ids, policy_now, merged.data(), X.tracker_on);
    if (bits_out) std::memcpy(bits_out, blk + L.off[RSB_BITS], (size_t)count);
    PubRec *rec = (PubRec *)std::aligned_alloc(16, sizeof(PubRec) * (size_t)n);
    for (int i = 0; i < n; i++) {
        rec[i].px = s_pos[3 * i]; rec[i].py = s_pos[3 * i + 1]; rec[i].pz = s_pos[3 * i + 2];
        rec[i].vx = s_vel[3 * i]; rec[i].vy = s_vel[3 * i + 1]; rec[i].vz = s_vel[3 * i + 2];
        rec[i].flags = s_flags[i]; rec[i].radius = s_radius[i];
    }
    const Rows d{rec, s_heading, s_goal, s_pref_speed, s_max_run_dist, s_total_dist, s_vpref_ext, s_step_num, s_status, s_nbr_n, s_near_n, s_zaxis, s_vpref_mode,
                 s_nbr_valid, s_trk_nbr0, s_trk_goal_heading, s_trk_st, s_trk_init, trk_words, nullptr, nullptr, nullptr, nullptr, 0, nullptr, n};
    const AttrRows at{s_policy, s_ap, s_ap_nd, s_R, s_plo, s_phi, s_cls};
    int delta = 0;
    for (int r = 0; r < count; r++) delta += serve_row(d, at, blk, L, ablk, AL, has, r);
    for (int i = 0; i < n; i++) {
        s_pos[3 * i] = rec[i].px; s_pos[3 * i + 1] = rec[i].py; s_pos[3 * i + 2] = rec[i].pz;
        s_vel[3 * i] = rec[i].vx; s_vel[3 * i + 1] = rec[i].vy; s_vel[3 * i + 2] = rec[i].vz;
        s_flags[i] = (uint8_t)rec[i].flags; s_radius[i] = rec[i].radius;
    }
    std::free(rec); std::free(blk); std::free(ablk);
    return delta;
}
// the ORCA3D-LP list of [n] policies against `now` (count_now ids): the list into out (room n), its length into *len; returns `changed`
int rsa_lp_list(const uint8_t *policy, int n, const int32_t *now, int count_now, int32_t *out, int *len) {
    std::vector<int32_t> have(now, now + count_now), list;
    const bool changed = respawn_lp_list(policy, n, have, list);
    std::memcpy(out, list.data(), sizeof(int32_t) * list.size());
    *len = (int)list.size();
    return changed ? 1 : 0;
}
// The tracker's classes in a plain context, call after call: a table that lives across rsa_table_step calls.  mask (nullable): the rows
// that count.  out: classes, many, moved.  Beside it the SCENE form on the compacted masked rows from a table of its own: the two must
// agree on the classes' values and users and on the masked tracked rows' class bytes (returns 0 where they do).
struct TablePair { ClassTable plain, scene; std::vector<uint8_t> scene_cls; };
void *rsa_table_new(void) { return new TablePair(); }
void rsa_table_free(void *h) { delete (TablePair *)h; }
int rsa_table_step(void *h, int n, const uint8_t *mask, const uint8_t *policy, const double *trip3, uint8_t *cls, const uint8_t *travels, int *out3) {
    TablePair &P = *(TablePair *)h;
    std::vector<TrackTriple> trip((size_t)n), ctrip;
    std::vector<uint8_t> cpol, ccls;
    std::vector<int> where;
    for (int i = 0; i < n; i++) {
        trip[(size_t)i] = TrackTriple{trip3[3 * i], trip3[3 * i + 1], trip3[3 * i + 2]};
        if (!mask || mask[i]) { ctrip.push_back(trip[(size_t)i]); cpol.push_back(policy[i]); where.push_back(i); }
    }
    const ClassUpdate u = plain_class_table(P.plain, n, mask, policy, trip.data(), cls, travels);
    out3[0] = u.classes; out3[1] = u.many; out3[2] = u.moved;
    // the scene form keeps its bytes by COMPACTED place only while the mask stands still; the caller keeps the mask fixed per table
    P.scene_cls.resize(cpol.size(), 0);
    const int32_t off[2] = {0, (int32_t)cpol.size()}, size[1] = {(int32_t)cpol.size()};
    const ClassUpdate v = scene_class_table(P.scene, 1, off, size, cpol.data(), ctrip.data(), P.scene_cls.data(), nullptr);
    if (u.classes != v.classes || u.many != v.many) return 1;
    if (u.many) return 0;
    for (int k = 0; k < TRK_CLASS_CAP; k++) if (P.plain.users[k] != P.scene.users[k] || (P.plain.users[k] && !(P.plain.val[k] == P.scene.val[k]))) return 2;
    for (size_t j = 0; j < where.size(); j++) if (restart_policy_tracked(cpol[j]) && cls[where[j]] != P.scene_cls[j]) return 3;
    return 0;
}

}  // extern "C"

#ifdef RESPAWN_ATTRS_MAIN
// every array on the heap in exactly its size (16-byte aligned where the rule stores 16-byte pieces): a read or write beyond a row or a
// section is the sanitizer's to find
template <class T> T *heap(size_t k, T v = T()) {
    T *p = (T *)std::aligned_alloc(16, (sizeof(T) * (k ? k : 1) + 15) / 16 * 16);
    for (size_t i = 0; i < k; i++) p[i] = v;
    return p;
}
int main() {
    unsigned seed = 4711u;
    const auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (seed >> 8) / (double)(1u << 24); };
    int fails = 0;
    const int counts[5] = {1, 63, 64, 65, 257};
    for (int trial = 0; trial < 100; trial++) {
        const int count = trial < 5 ? counts[trial] : 1 + (int)(rnd() * 300), n = count + (int)(rnd() * 300), trk = trial % 2, words = 37;
        const int c[11] = {1, 1, 0, 0, 0, 0, n, n, trk, 0, 0};
        uint8_t *policy_now = heap<uint8_t>(n), *path_vpref = heap<uint8_t>(n), *policy = trial % 4 == 3 ? nullptr : heap<uint8_t>(count);
        for (int i = 0; i < n; i++) { policy_now[i] = (uint8_t)(rnd() * 6); path_vpref[i] = rnd() < 0.3 && policy_now[i] != 0 && policy_now[i] != 5; }
        int32_t *ids = heap<int32_t>(count);
        {
            std::vector<int32_t> all((size_t)n);
            for (int i = 0; i < n; i++) all[i] = i;
            for (int i = n - 1; i > 0; i--) std::swap(all[i], all[(int)(rnd() * (i + 1))]);
            for (int r = 0; r < count; r++) ids[r] = all[r];
        }
        AgentPar *par = trial % 3 == 2 ? nullptr : heap<AgentPar>(count);
        for (int r = 0; r < count; r++) {
            if (policy) policy[r] = (uint8_t)(rnd() * 6);
            if (par) par[r] = AgentPar{1.0 + r, 0.1, 10.0, 1.0, 0.7, 0.1, 1 + r % 16, 0, (1.0 + r) * (1.0 + r)};
        }
        double *pos = heap<double>(3 * count, 2.0), *heading = heap<double>(3 * count, 0.5), *goal = heap<double>(3 * count, 4.0), *gh = heap<double>(3 * count, 0.25);
        float *vel = heap<float>(3 * count);
        double *radius = heap<double>(count, 0.5), *ps = heap<double>(count, 1.0), *mrd = heap<double>(count, 9.0);
        int out6[6];
        uint8_t *merged = heap<uint8_t>(n);
        rsa_check(c, policy_now, count, ids, policy, nullptr, radius, 1, out6, merged);
        if (out6[0] != RSP_OK || out6[3] != RSA_OK) { std::printf("trial %d: refused %d / %d\n", trial, out6[0], out6[3]); fails++; continue; }
        double *s_pos = heap<double>(3 * n), *s_radius = heap<double>(n, 0.3), *s_heading = heap<double>(3 * n), *s_goal = heap<double>(3 * n);
        float *s_vel = heap<float>(3 * n);
        uint8_t *s_flags = heap<uint8_t>(n), *s_zaxis = heap<uint8_t>(n), *s_mode = heap<uint8_t>(n, 1), *s_valid = heap<uint8_t>(n, 1), *s_policy = heap<uint8_t>(n);
        for (int i = 0; i < n; i++) { s_flags[i] = (uint8_t)(rnd() < 0.5 ? 1 << (int)(rnd() * 3) : 0); s_policy[i] = policy_now[i]; }
        double *s_ps = heap<double>(n), *s_mrd = heap<double>(n), *s_td = heap<double>(n, 3.0), *s_ext = heap<double>(3 * n, 7.0), *s_nd = heap<double>(n, 10.0);
        int32_t *s_sn = heap<int32_t>(n, 5), *s_st = heap<int32_t>(n, 8), *s_nn = heap<int32_t>(n, 4), *s_near = heap<int32_t>(n, 2);
        double *s_nbr0 = trk ? heap<double>(n, 2.0) : nullptr, *s_tgh = trk ? heap<double>(3 * n) : nullptr;
        uint32_t *s_st32 = trk ? heap<uint32_t>((size_t)words * n, 9u) : nullptr, *s_init = trk ? heap<uint32_t>(words, 1u) : nullptr;
        AgentPar *s_ap = heap<AgentPar>(n, AgentPar{10.0, 0.1, 10.0, 1.0, 0.7, 0.1, 16, 0, 100.0});
        uint8_t *bits = heap<uint8_t>(count);
        const bool planner = trk && trial % 5 != 4;
        double *trip3 = planner ? heap<double>(3 * count) : nullptr, *s_R = trk ? heap<double>(n, 1.5) : nullptr, *s_plo = trk ? heap<double>(n, -0.7) : nullptr,
               *s_phi = trk ? heap<double>(n, 0.7) : nullptr;
        uint8_t *cls = planner ? heap<uint8_t>(count) : nullptr, *s_cls = trk ? heap<uint8_t>(n, 15) : nullptr;
        for (int r = 0; planner && r < count; r++) { trip3[3 * r] = 2.0 + r; trip3[3 * r + 1] = -0.5; trip3[3 * r + 2] = 0.5 + r; cls[r] = (uint8_t)(r % 16); }
        int done = 0;
        for (int r = 0; r < count; r++) done += s_flags[ids[r]] != 0;
        const int delta = rsa_apply(c, policy_now, path_vpref, count, ids, policy, par, pos, vel, heading, radius, ps, goal, mrd, gh, s_pos, s_vel, s_flags, s_radius, s_heading,
                                    s_goal, s_ps, s_mrd, s_td, s_sn, s_st, s_nn, s_near, s_zaxis, s_mode, s_valid, s_ext, s_nbr0, s_tgh, s_st32, s_init, words, s_policy,
                                    s_ap, s_nd, bits, trip3, cls, s_R, s_plo, s_phi, s_cls);
        if (delta != done) { std::printf("trial %d: done_delta %d, %d rows were done\n", trial, delta, done); fails++; }
        std::vector<uint8_t> named((size_t)n, 0);
        for (int r = 0; r < count; r++) {
            const int a = ids[r];
            named[(size_t)a] = 1;
            const uint8_t pnew = policy ? policy[r] : policy_now[a];
            const bool was = policy_now[a] == 0 || policy_now[a] == 5, now = pnew == 0 || pnew == 5, t = trk && now, left = trk && was && !now;
            bool ok = s_policy[a] == pnew && merged[a] == pnew && s_flags[a] == 0 && s_radius[a] == 0.5 && s_td[a] == 0.0 && s_valid[a] == 0 && s_pos[3 * a + 1] == 2.0 &&
                      s_mode[a] == (t ? 1 : (left || path_vpref[a]) ? 0 : 1) && ((t || left) ? s_ext[3 * a + 2] == 0.0 : s_ext[3 * a + 2] == 7.0) &&
                      (par ? s_ap[a].neighbor_dist == 1.0 + r && s_ap[a].max_neighbors == 1 + r % 16 && s_ap[a].range_sq == (1.0 + r) * (1.0 + r) && s_nd[a] == 1.0 + r
                           : s_ap[a].neighbor_dist == 10.0 && s_nd[a] == 10.0);
            if (trk) ok = ok && s_st32[(size_t)words * a] == ((t || left) ? 1u : 9u) && s_st32[(size_t)words * a + words - 1] == ((t || left) ? 1u : 9u);
            if (trk) ok = ok && (planner ? s_R[a] == 2.0 + r && s_plo[a] == -0.5 && s_phi[a] == 0.5 + r && s_cls[a] == (uint8_t)(r % 16)
                                         : s_R[a] == 1.5 && s_plo[a] == -0.7 && s_phi[a] == 0.7 && s_cls[a] == 15);
            if (!ok) { std::printf("trial %d: row %d (agent %d)\n", trial, r, a); fails++; break; }
        }
        for (int i = 0; i < n; i++)
            if (!named[(size_t)i] && !(s_policy[i] == policy_now[i] && s_ap[i].neighbor_dist == 10.0 && s_nd[i] == 10.0 && s_mode[i] == 1 && s_td[i] == 3.0 && s_ext[3 * i] == 7.0 &&
                                      (!trk || (s_st32[(size_t)words * i] == 9u && s_R[i] == 1.5 && s_plo[i] == -0.7 && s_phi[i] == 0.7 && s_cls[i] == 15)))) { std::printf("trial %d: agent %d was not named and changed\n", trial, i); fails++; break; }
        for (void *p : {(void *)policy_now, (void *)path_vpref, (void *)policy, (void *)ids, (void *)par, (void *)pos, (void *)heading, (void *)goal, (void *)gh, (void *)vel,
                        (void *)radius, (void *)ps, (void *)mrd, (void *)merged, (void *)s_pos, (void *)s_radius, (void *)s_heading, (void *)s_goal, (void *)s_vel, (void *)s_flags,
                        (void *)s_zaxis, (void *)s_mode, (void *)s_valid, (void *)s_policy, (void *)s_ps, (void *)s_mrd, (void *)s_td, (void *)s_ext, (void *)s_nd, (void *)s_sn,
                        (void *)s_st, (void *)s_nn, (void *)s_near, (void *)s_nbr0, (void *)s_tgh, (void *)s_st32, (void *)s_init, (void *)s_ap, (void *)bits, (void *)trip3, (void *)s_R,
                        (void *)s_plo, (void *)s_phi, (void *)cls, (void *)s_cls})
            std::free(p);
    }
    std::printf(fails ? "respawn_attrs_harness: %d failures\n" : "respawn_attrs_harness: ok\n", fails);
    return fails ? 1 : 0;
}
#endif
