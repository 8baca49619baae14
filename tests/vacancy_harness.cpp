// The pure rules of sca_amd/csrc/sca_vacancy.h (and the vacancy rows of sca_forms.h) behind C entry points (tests/test_vacancy_cpu.py),
// and -- with -DVACANCY_MAIN -- as a program of its own for the sanitizers: every buffer on the heap in exactly the size the rules may touch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sca_vacancy.h"
#include "sca_forms.h"

using namespace sca;

namespace {

RespawnCtx ctx_of(const int *c) {
    RespawnCtx X;
    X.agents = c[0]; X.state = c[1]; X.mid_step = c[2]; X.scenes = c[3]; X.comm = c[4]; X.partition = c[5];
    X.n = c[6]; X.shard_count = c[7]; X.tracker_on = c[8]; X.paths_block = c[9]; X.path_W = c[10];
    X.policy_now = nullptr;
    return X;
}

// the per-agent arrays k_vacate writes, as plain host arrays of n rows (null: the context has none of it)
struct Rows {
    PubRec *rec;
    double *heading, *total_dist;
    float *action;
    int32_t *diag, *step_num, *status, *nbr_n, *near_n;
    uint8_t *nbr_valid;
    double *now_goal;
    int32_t *path_len, *path_rem;
    sca_scene_clearance *clear;
};

// k_vacate's body for row a, lane by lane; returns done_delta
int vacate_row(const Rows &d, int a) {
    const VacantRow w = vacant_row(d.rec[a].flags, d.path_len != nullptr);
    for (int lane = 0; lane < 64; lane++) vacate_write_row(d, a, lane, w);
    return w.done_delta;
}

std::vector<PubRec> recs_of(const uint8_t *flags, int n) {
    std::vector<PubRec> rec((size_t)n, PubRec{});
    for (int i = 0; i < n; i++) rec[(size_t)i].flags = flags[i];
    return rec;
}

}  // namespace

extern "C" {

// out: fault, entry, code
void vac_check(const int *ctx, const uint8_t *vacant, int occupied, int count, const int32_t *ids, int *out) {
    const VacancyCheck k = vacancy_check(ctx_of(ctx), vacant, occupied, count, ids);
    out[0] = k.fault; out[1] = k.entry; out[2] = vacancy_error_code(k.fault);
}
void vac_list_check(const int *ctx, int have_ids, int capacity, int have_count, int *out) {
    const VacancyFault f = vacant_list_check(ctx_of(ctx), have_ids != 0, capacity, have_count != 0);
    out[0] = f; out[1] = -1; out[2] = vacancy_error_code(f);
}
// vacate the rows ids[0 .. count) of host arrays of n rows; delta[r]: the row's done_delta.  state: pos (n*3), vel f32 (n*3), flags u8,
// radius travel as columns and come back as columns
void vac_vacate(int n, int count, const int32_t *ids, double *pos, float *vel, uint8_t *flags, double *radius, double *heading, double *total_dist,
                float *action, int32_t *diag, int32_t *step_num, int32_t *status, int32_t *nbr_n, int32_t *near_n, uint8_t *nbr_valid, double *now_goal,
                int32_t *path_len, int32_t *path_rem, double *clear_agent, int32_t *clear_partner, int32_t *delta) {
    std::vector<PubRec> rec((size_t)n);
    std::vector<sca_scene_clearance> clr(clear_agent ? (size_t)n : 0);
    for (int i = 0; i < n; i++) {
        PubRec &r = rec[(size_t)i];
        r.px = pos[3 * i]; r.py = pos[3 * i + 1]; r.pz = pos[3 * i + 2]; r.vx = vel[3 * i]; r.vy = vel[3 * i + 1]; r.vz = vel[3 * i + 2];
        r.flags = flags[i]; r.radius = radius[i];
        if (clear_agent) { clr[(size_t)i] = scene_clearance_empty(); clr[(size_t)i].agent_clear = clear_agent[i]; clr[(size_t)i].agent_partner = clear_partner[i]; }
    }
    const Rows d{rec.data(), heading, total_dist, action, diag, step_num, status, nbr_n, near_n, nbr_valid, now_goal, path_len, path_rem, clear_agent ? clr.data() : nullptr};
    for (int r = 0; r < count; r++) delta[r] = vacate_row(d, ids[r]);
    for (int i = 0; i < n; i++) {
        const PubRec &r = rec[(size_t)i];
        pos[3 * i] = r.px; pos[3 * i + 1] = r.py; pos[3 * i + 2] = r.pz; vel[3 * i] = r.vx; vel[3 * i + 1] = r.vy; vel[3 * i + 2] = r.vz;
        flags[i] = (uint8_t)r.flags; radius[i] = r.radius;
        if (clear_agent) { clear_agent[i] = clr[(size_t)i].agent_clear; clear_partner[i] = clr[(size_t)i].agent_partner; }
    }
}
// one ordered compaction in tiles of `tile` (256 or 64) items; returns how many were written, -1: an unknown tile size
int vac_compact(int tile, int mode, const uint8_t *flags, const int32_t *perm, const int32_t *ids, const int32_t *verdict, int n, int m, int count,
                int32_t *out, int base) {
    const std::vector<PubRec> rec = recs_of(flags, n);
    const VacView v{rec.data(), perm, ids, verdict, n, m, count};
    if (tile == 256) return vacancy_compact<256>(v, mode, out, base);
    if (tile == 64) return vacancy_compact<64>(v, mode, out, base);
    return -1;
}
// plan_auto / auto_next with vacancy_on (with_arg 0: the defaulted form); out: auto_pass, auto_backoff, kdq_last, auto_next
void vac_plan_auto(int fits, int tracked, int kd_ahead, int kdq_last, int auto_div, int auto_backoff, int shard_count, int vacancy_on, int with_arg, int *out) {
    const AutoPlan p = with_arg ? plan_auto(fits != 0, tracked != 0, kd_ahead != 0, kdq_last, auto_div, auto_backoff, shard_count, vacancy_on != 0)
                                : plan_auto(fits != 0, tracked != 0, kd_ahead != 0, kdq_last, auto_div, auto_backoff, shard_count);
    out[0] = p.auto_pass; out[1] = p.auto_backoff; out[2] = p.kdq_last;
    out[3] = with_arg ? auto_next(fits != 0, tracked != 0, false, kdq_last, auto_div, auto_backoff, shard_count, vacancy_on != 0)
                      : auto_next(fits != 0, tracked != 0, false, kdq_last, auto_div, auto_backoff, shard_count);
}
// plan_step with the StepIn fields in declaration order (ints), missions_on and vacancy_on last; out: moved_on_action, build_ahead, fork_rides
void vac_plan_step(const int *i, int vacancy_on, int with_field, int *out3) {
    StepIn in{i[0], i[1], i[2], i[3] != 0, i[4] != 0, i[5] != 0, i[6] != 0, i[7] != 0, i[8] != 0, i[9] != 0, i[10] != 0, i[11] != 0, i[12] != 0, i[13] != 0, i[14] != 0,
              i[15], i[16], i[17], i[18]};
    in.missions_on = i[19] != 0;
    if (with_field) in.vacancy_on = vacancy_on != 0;
    const StepPlan p = plan_step(in);
    out3[0] = p.moved_on_action; out3[1] = p.build_ahead; out3[2] = p.fork_rides;
}
int vac_finished_listed(unsigned flags) { return finished_listed(flags) ? 1 : 0; }

}  // extern "C"

#ifdef VACANCY_MAIN
// Random retires and admissions on heap arrays of exactly n rows, the permutation edited by the tiled compactions at both tile sizes and
// checked against the plain list edit.
int main() {
    unsigned long long s = 88172645463325252ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int n : {1, 2, 63, 64, 65, 255, 256, 257, 700}) {
        std::vector<uint8_t> flags((size_t)n, 0), vacant((size_t)n, 0);
        std::vector<int32_t> perm((size_t)n);
        for (int i = 0; i < n; i++) { perm[(size_t)i] = i; flags[(size_t)i] = (uint8_t)(rnd() % 5 == 0 ? 1 + rnd() % 4 : 0); }
        for (int i = n - 1; i > 0; i--) std::swap(perm[(size_t)i], perm[(size_t)(rnd() % (unsigned)(i + 1))]);
        int m = n;
        std::vector<double> pos(3 * (size_t)n, 1.0), radius((size_t)n, 0.5), heading(3 * (size_t)n, 0.3), td((size_t)n, 2.0), now_goal(3 * (size_t)n, 1.0), ca((size_t)n, 0.1);
        std::vector<float> vel(3 * (size_t)n, 0.5f), action(8 * (size_t)n, 1.0f);
        std::vector<int32_t> diag(8 * (size_t)n, 3), sn((size_t)n, 4), status((size_t)n, 1), nbr_n((size_t)n, 2), near_n((size_t)n, 1), plen((size_t)n, 2), prem((size_t)n, 1),
            cp((size_t)n, 0);
        std::vector<uint8_t> nv((size_t)n, 1);
        for (int round = 0; round < 12; round++) {
            // retire some occupied rows (never the last), in shuffled order
            std::vector<int32_t> ids;
            for (int i = 0; i < n; i++) if (!vacant[(size_t)i] && rnd() % 3 == 0 && (int)ids.size() + 1 < m) ids.push_back(i);
            for (int i = (int)ids.size() - 1; i > 0; i--) std::swap(ids[(size_t)i], ids[(size_t)(rnd() % (unsigned)(i + 1))]);
            if (!ids.empty()) {
                const int ctx[11] = {1, 1, 0, 0, 0, 0, n, n, 0, 0, 2};
                int out[3];
                vac_check(ctx, vacant.data(), m, (int)ids.size(), ids.data(), out);
                if (out[0] != VCF_OK) { std::printf("a legal retire was refused: %d\n", out[0]); return 1; }
                std::vector<int32_t> delta(ids.size());
                vac_vacate(n, (int)ids.size(), ids.data(), pos.data(), vel.data(), flags.data(), radius.data(), heading.data(), td.data(), action.data(), diag.data(), sn.data(),
                           status.data(), nbr_n.data(), near_n.data(), nv.data(), now_goal.data(), plen.data(), prem.data(), ca.data(), cp.data(), delta.data());
                std::vector<int32_t> want;
                for (int p = 0; p < m; p++) if (!(flags[(size_t)perm[(size_t)p]] & FLAG_VACANT)) want.push_back(perm[(size_t)p]);
                for (int32_t a : ids) vacant[(size_t)a] = 1;
                for (int i = 0; i < n; i++) if (vacant[(size_t)i]) want.push_back(i);
                for (int tile : {256, 64}) {
                    std::vector<int32_t> tmp((size_t)n), got = perm;
                    const int kept = vac_compact(tile, VAC_KEEP, flags.data(), perm.data(), nullptr, nullptr, n, m, 0, tmp.data(), 0);
                    if (kept != m - (int)ids.size()) { std::printf("kept %d of %d\n", kept, m); return 1; }
                    const int tail = vac_compact(tile, VAC_TAIL, flags.data(), perm.data(), nullptr, nullptr, n, m, 0, got.data(), kept);
                    if (kept + tail != n) { std::printf("the edit lost a row\n"); return 1; }
                    std::memcpy(got.data(), tmp.data(), sizeof(int32_t) * (size_t)kept);
                    if (got != want) { std::printf("retire: the tiled edit differs from the list edit (n %d, tile %d)\n", n, tile); return 1; }
                }
                perm = want; m -= (int)ids.size();
            }
            // admit some vacant rows among occupied ones, under a verdict
            std::vector<int32_t> call, verdict;
            for (int i = 0; i < n; i++) if (rnd() % 4 == 0) { call.push_back(i); verdict.push_back(rnd() % 3 == 0 ? 1 : 0); }
            for (int i = (int)call.size() - 1; i > 0; i--) { const size_t j = (size_t)(rnd() % (unsigned)(i + 1)); std::swap(call[(size_t)i], call[j]); std::swap(verdict[(size_t)i], verdict[j]); }
            if (!call.empty()) {
                std::vector<int32_t> want(perm.begin(), perm.begin() + m), in;
                for (size_t r = 0; r < call.size(); r++) if (vacant[(size_t)call[r]] && verdict[r] == 0) in.push_back(call[r]);
                want.insert(want.end(), in.begin(), in.end());
                std::vector<uint8_t> after = flags;
                for (int32_t a : in) after[(size_t)a] = 0;
                for (int i = 0; i < n; i++) if (after[(size_t)i] & FLAG_VACANT) want.push_back(i);
                for (int tile : {256, 64}) {
                    std::vector<int32_t> got = perm;
                    const int k = vac_compact(tile, VAC_ADMIT, flags.data(), perm.data(), call.data(), verdict.data(), n, m, (int)call.size(), got.data(), m);
                    if (k != (int)in.size()) { std::printf("admitted %d of %d\n", k, (int)in.size()); return 1; }
                    const int tail = vac_compact(tile, VAC_TAIL, after.data(), perm.data(), nullptr, nullptr, n, m, 0, got.data(), m + k);
                    if (m + k + tail != n) { std::printf("the admission lost a row\n"); return 1; }
                    if (got != want) { std::printf("admit: the tiled edit differs from the list edit (n %d, tile %d)\n", n, tile); return 1; }
                }
                flags = after; perm = want; m += (int)in.size();
                for (int32_t a : in) vacant[(size_t)a] = 0;
            }
        }
    }
    std::printf("vacancy_harness: ok\n");
    return 0;
}
#endif
