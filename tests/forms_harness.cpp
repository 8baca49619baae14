// Test-only: the form decisions of the host side (sca_amd/csrc/sca_forms.h) behind a C interface for tests/test_forms_cpu.py.  Plain C++, no
// HIP.  A Tunables travels as its ints, in the order of the TUNABLES table.  Not part of the product (sca_amd never loads it).
#include <cstring>

#include "sca_forms.h"

using namespace sca;

constexpr int NTUN = (int)(sizeof(TUNABLES) / sizeof(TUNABLES[0]));
static_assert(sizeof(Tunables) == NTUN * sizeof(int), "one table row per member");

static Tunables tun_of(const int *v) {
    Tunables t{};
    for (int i = 0; i < NTUN; i++) t.*TUNABLES[i].member = v[i];
    return t;
}

extern "C" {

int forms_tunable_count(void) { return NTUN; }
const char *forms_tunable_name(int i) { return TUNABLES[i].name; }
// what sca_create followed by sca_device_tracker_enable would hold in the environment of the moment
void forms_tunables_from_env(int simds, int *out) {
    Tunables t{};
    tunables_from_env(t, simds, TUN_AT_CREATE);
    tunables_from_env(t, simds, TUN_AT_TRACKER);
    for (int i = 0; i < NTUN; i++) out[i] = t.*TUNABLES[i].member;
}
// only the rows of sca_device_tracker_enable are read again: the others keep what `inout` holds
void forms_tunables_tracker_again(int simds, int *inout) {
    Tunables t = tun_of(inout);
    tunables_from_env(t, simds, TUN_AT_TRACKER);
    for (int i = 0; i < NTUN; i++) inout[i] = t.*TUNABLES[i].member;
}
void forms_constants(int *out7) {
    const int v[7] = {KD_WAVE_CAP, KD_WAVE_FLOOR, KD_CHUNK, KD_MAX_LEVELS, KT_M, KDQ_BLOCKS, KDQ_BLOCKS_FEW};
    std::memcpy(out7, v, sizeof(v));
}

void forms_plan_auto(int fits, int tracked, int kd_ahead, int kdq_last, int auto_div, int auto_backoff, int shard_count, int *out4) {
    const AutoPlan p = plan_auto(fits, tracked, kd_ahead, kdq_last, auto_div, auto_backoff, shard_count);
    out4[0] = p.auto_pass; out4[1] = p.auto_backoff; out4[2] = p.kdq_last; out4[3] = p.kdq_blocks;
}
int forms_auto_next(int fits, int tracked, int part_on, int kdq_last, int auto_div, int auto_backoff, int shard_count) {
    return auto_next(fits, tracked, part_on, kdq_last, auto_div, auto_backoff, shard_count);
}
int forms_auto_tail_form(int tail_ok, int waitvalue, unsigned seq, int kdq_last, int auto_tail_max) {
    return auto_tail_form(tail_ok, waitvalue, seq, kdq_last, auto_tail_max);
}

// out: seq, tail, record_slot, wait_slot, gather_slot (a slot that is none: -1)
void forms_plan_auto_build(int tail_ok, int waitvalue, unsigned auto_seq, int kdq_last, int auto_tail_max, unsigned on_kd, unsigned builds, long long *out5) {
    const AutoBuildPlan b = plan_auto_build(tail_ok, waitvalue, auto_seq, kdq_last, auto_tail_max, on_kd, builds);
    const long long v[5] = {b.seq, b.tail, b.record_slot, b.wait_slot, b.gather_slot};
    std::memcpy(out5, v, sizeof(v));
}
// out: seq, parity, reuse_slot, tail, kdq_slot, on_kd_stream, on_kd, copy_count, passes, wait, gather_slot
void forms_plan_auto_pass(unsigned auto_seq, unsigned tail_seq, unsigned on_kd, int waitvalue, int count_pending, unsigned passes, unsigned builds, long long *out11) {
    const AutoPassPlan p = plan_auto_pass(auto_seq, tail_seq, on_kd, waitvalue, count_pending, passes, builds);
    const long long v[11] = {p.seq, p.parity, p.reuse_slot, p.tail, p.kdq_slot, p.on_kd_stream, p.on_kd, p.copy_count, p.passes, p.wait, p.gather_slot};
    std::memcpy(out11, v, sizeof(v));
}

// in19: StepIn's members in their order; out: moved_on_action, build_ahead, fork_rides
void forms_plan_step(const int *in19, int *out3) {
    const int *v = in19;
    const StepIn i{v[0], v[1], v[2], v[3] != 0, v[4] != 0, v[5] != 0, v[6] != 0, v[7] != 0, v[8] != 0, v[9] != 0, v[10] != 0, v[11] != 0, v[12] != 0,
                   v[13] != 0, v[14] != 0, v[15], v[16], v[17], v[18]};
    const StepPlan p = plan_step(i);
    out3[0] = p.moved_on_action; out3[1] = p.build_ahead; out3[2] = p.fork_rides;
}
// out: k4 (FinishK4), carrier (FinishCarrier), harvest, others
void forms_plan_finish(int scenes_on, int obs_on, int harvest_on, int part_on, int shard_below_n, int last_mode, int *out4) {
    const FinishPlan p = plan_finish(scenes_on, obs_on, harvest_on, part_on, shard_below_n, last_mode);
    out4[0] = p.k4; out4[1] = p.carrier; out4[2] = p.harvest; out4[3] = p.others;
}
// the fault (StepFault) of an entry point that makes `checks`; out2: its error code and the length of its text, which goes to text[cap]
int forms_step_check(int checks, int state_set, int steps, int mode, int part_on, int part_ranks_apart, int *out2, char *text, int cap) {
    const StepFault f = step_check(checks, state_set, steps, mode, part_on, part_ranks_apart);
    const char *t = step_fault_text(f);
    out2[0] = step_fault_code(f); out2[1] = (int)std::strlen(t);
    if (cap > 0) { const size_t k = std::min((size_t)out2[1], (size_t)cap - 1); std::memcpy(text, t, k); text[k] = 0; }
    return f;
}

int forms_choose_solve_split(const int *tun, int simds, int overlap, int cnt, int trk_last_count) {
    return choose_solve_split(tun_of(tun), simds, overlap, cnt, trk_last_count);
}
void forms_plan_solve(const int *tun, int simds, int cnt, int part_on, int part_nranks, long long lp_total, int lp_in_shard, int overlap,
                      int trk_last_count, int no_sweep_scratch, int *out7) {
    const SolvePlan p = plan_solve(tun_of(tun), simds, cnt, part_on, part_nranks, lp_total, lp_in_shard, overlap, trk_last_count, no_sweep_scratch);
    out7[0] = p.packed; out7[1] = p.split; out7[2] = p.solve_fb; out7[3] = p.lpw; out7[4] = p.lp_kernel; out7[5] = p.action_fb; out7[6] = p.forms;
}

// out: fused, group_fused, forms, n, then n x (kernel, lo, hi, plans, lanes)
void forms_plan_replans(const int *tun, int cnt, int last_count, int trk_many, int in_pass, int part_on, int *out29) {
    const ReplanPlan p = plan_replans(tun_of(tun), cnt, last_count, trk_many, in_pass, part_on);
    out29[0] = p.fused; out29[1] = p.group_fused; out29[2] = p.forms; out29[3] = p.n;
    for (int i = 0; i < p.n; i++) {
        const ReplanLaunch &l = p.launch[i];
        const int v[5] = {l.kernel, l.lo, l.hi, l.plans, l.lanes};
        std::memcpy(out29 + 4 + 5 * i, v, sizeof(v));
    }
}

void forms_plan_kd_build(const int *tun, int n, int beside, int single_hint, int chunk_cap, int rank_capacity, int *out9) {
    const KdBuildPlan p = plan_kd_build(tun_of(tun), n, beside, single_hint, chunk_cap, rank_capacity);
    const int v[9] = {p.top, p.wave_max, p.block, p.level_passes, p.first_single, p.grid, p.ticket, p.levels, p.sgrid};
    std::memcpy(out9, v, sizeof(v));
}

}  // extern "C"

#ifdef FORMS_MAIN
// The harness as a program of its own (tests/test_forms_cpu.py builds it with -fsanitize=address,undefined): every entry point above into
// heap arrays of exactly the length it documents, the two AUTO plans over every slot state on both sides of the wrap of `seq`.
#include <cstdio>
#include <memory>
int main() {
    std::unique_ptr<int[]> tun(new int[NTUN]), k7(new int[7]), o4(new int[4]), o7(new int[7]), o9(new int[9]), o29(new int[29]);
    std::unique_ptr<long long[]> b5(new long long[5]), p11(new long long[11]);
    forms_tunables_from_env(1024, tun.get());
    forms_tunables_tracker_again(512, tun.get());
    forms_tunables_from_env(1024, tun.get());
    forms_constants(k7.get());
    long long sum = forms_tunable_count() + (forms_tunable_name(NTUN - 1) != nullptr) + k7[6];
    for (int last : {-1, 0, 126, 1 << 30}) {
        forms_plan_auto(1, 0, last & 1, last, 8, last == 0 ? 3 : 0, 1000, o4.get());
        sum += o4[0] + o4[3] + forms_auto_next(1, 0, 0, last, 8, 0, 1000) + forms_auto_tail_form(1, 1, 7u, last, 0);
    }
    for (unsigned at : {0u, 0xFFFFFFF0u})
        for (unsigned i = 0; i < 32; i++)
            for (unsigned on_kd = 0; on_kd < 16; on_kd++)
                for (int form = 0; form < 4; form++) {       // kdq_last -1 / 0, the wait-value form on / off
                    const unsigned seq = at + i;
                    forms_plan_auto_build(1, form & 2, seq, (form & 1) - 1, 0, on_kd, i, b5.get());
                    forms_plan_auto_pass(seq, b5[1] ? (unsigned)b5[0] : seq - 1u, on_kd, form & 2, i & 1, i, i + 1, p11.get());
                    if (p11[4] != (long long)((seq + 1u) & 3u) || p11[6] < 0 || p11[6] > 15 || b5[3] > 3 || p11[2] > 3) { std::printf("forms_harness: a slot out of range\n"); return 1; }
                    sum += b5[2] + b5[3] + b5[4] + p11[1] + p11[2] + p11[8] + p11[9] + p11[10];
                }
    // the step's plans over every combination of their flags (bursts of 3, every mode), the refusals into a text buffer of exactly their length
    std::unique_ptr<int[]> in19(new int[19]), o3(new int[3]), o2(new int[2]);
    for (int mode = SCA_NBR_KDTREE; mode <= SCA_NBR_AUTO; mode++)
        for (int s = 0; s < 3; s++)
            for (unsigned bits = 0; bits < (1u << 12); bits++) {
                const int v[19] = {mode, s, 3, (int)(bits & 1), (int)(bits >> 1 & 1), (int)(bits >> 2 & 1), (int)(bits >> 3 & 1), (int)(bits >> 4 & 1), (int)(bits >> 5 & 1),
                                   (int)(bits >> 6 & 1), (int)(bits >> 7 & 1), (int)(bits >> 8 & 1), (int)(bits >> 9 & 1), (int)(bits >> 10 & 1), (int)(bits >> 11 & 1), -1, 8, 0, 1000};
                std::memcpy(in19.get(), v, sizeof(v));
                forms_plan_step(in19.get(), o3.get());
                if (o3[1] && o3[2]) { std::printf("forms_harness: a step builds ahead and carries a fork\n"); return 1; }
                sum += o3[0] + o3[1] + o3[2];
            }
    for (int bits = 0; bits < 32; bits++)
        for (int mode = SCA_NBR_KDTREE; mode <= SCA_NBR_AUTO; mode++) {
            forms_plan_finish(bits & 1, bits >> 1 & 1, bits >> 2 & 1, bits >> 3 & 1, bits >> 4 & 1, mode, o4.get());
            if (o4[0] < K4_SCENE_OBS || o4[0] > K4_PLAIN || o4[1] < CARRY_K4 || o4[1] > CARRY_OTHERS) { std::printf("forms_harness: a finish plan out of range\n"); return 1; }
            sum += o4[0] + o4[1] + o4[2] + o4[3];
        }
    for (int checks = 0; checks <= STEP_CHK_ALL; checks++)
        for (int bits = 0; bits < 16; bits++) {
            forms_step_check(checks, bits & 1, (bits >> 1 & 1) - 1, SCA_NBR_KDTREE - 1 + 3 * (bits >> 2 & 1), 1, bits >> 3 & 1, o2.get(), nullptr, 0);
            std::unique_ptr<char[]> text(new char[(size_t)o2[1] + 1]);
            sum += forms_step_check(checks, bits & 1, (bits >> 1 & 1) - 1, SCA_NBR_KDTREE - 1 + 3 * (bits >> 2 & 1), 1, bits >> 3 & 1, o2.get(), text.get(), o2[1] + 1) + (int)std::strlen(text.get());
        }
    for (int cnt : {1, 2048, 30000, 100000, 2000000}) {
        sum += forms_choose_solve_split(tun.get(), 1024, 1, cnt, cnt / 2);
        forms_plan_solve(tun.get(), 1024, cnt, 0, 1, cnt / 3, cnt / 3, cnt & 1, -1, 0, o7.get());
        forms_plan_replans(tun.get(), cnt, -1, 0, 1, 0, o29.get());
        forms_plan_kd_build(tun.get(), cnt, 0, 0, 1 << 30, 1 << 30, o9.get());
        sum += o7[6] + o29[3] + o9[8];
    }
    std::printf("forms_harness: ok (%lld)\n", sum);
    return 0;
}
#endif
