// sca_forms.h -- which kernel forms a pass runs: the tunables (thresholds and switches, read from the environment in ONE place) and the
// pure functions that turn a shard size, the SIMD count and the counts read back from earlier passes into a plan.  No HIP, no sca_ctx:
// sca_hip.hip polls its readbacks, calls one of these, and enqueues what the plan says; tests/test_forms_cpu.py checks them without a GPU.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>

#include "../../include/sca_hip.h"
#include "sca_constants.h"

namespace sca {

// every launch heuristic is stated in wavefronts per SIMD and scaled with the device's SIMD count; the figures were measured on a 256-CU MI355X
inline int per_simd(int simds, long long at_1024_simds) { return (int)std::min<long long>(INT_MAX, at_1024_simds * simds / 1024); }

// ---- the tunables -------------------------------------------------------------------------------------------------------------------------------
// (all int, so that one table of member pointers can fill them; the defaults are in the table below)
struct Tunables {
    // read at sca_create
    int k1_force;        // SCA_K1_PACKED: K1 variant, -1 choose by shard size, 0 one agent per wavefront, 1 four (k_neighbors_kd4)
    int auto_div;        // SCA_AUTO_BACKOFF_DIV (1 .. 64): SCA_NBR_AUTO backs off to the plain kd pass (for 256 passes) once the grid query lists more
                         // than 1 / auto_div of the shard for the kd query
    int auto_no_tail;    // SCA_AUTO_NO_TAIL (set = 1): never the launch-free form of the listed agents' kd query
    int auto_tail_max;   // SCA_AUTO_TAIL_MAX: ... which is taken while the list lengths that come back stay at or below this.  0: while NOBODY is
                         // listed -- one workgroup answering even a handful of agents per pass lost against the launch form over a whole c3
                         // episode (3000 steps: 0.172 ms per step at 32, 0.121-0.125 at 8, 0.099-0.101 at 0, 0.104 launch form)
    int solve_split;     // SCA_SOLVE_SPLIT: k_solve in two launches (k_solve_sweep beside the re-plans, k_solve_pick4 behind them): -1 by
                         // choose_solve_split, 0 never, 1 always (the parity tests run both)
    int hs_staged;       // SCA_HOST_STEP_STAGED=1 (A/B measurements, tests): the host state block crosses the link as copies into / out of a device
                         // staging buffer.  Default: the two kernels read and write the page-locked block across the link themselves -- faster at
                         // N = 1024, 4096 and 100 000 by more than the spread (profiles/host_step_cost.json)
    int kd_top;          // SCA_KD_TOP=0: trees of <= KT_M members through the level passes as well (tests, measurements)
    int ext_stop;        // SCA_EXT_STOP=0: the fork / join / hand-over events as records of their own instead of stop events of the kernels they follow
    int kd_force_ticket; // SCA_KD_TICKET=1: k_kd_lv_rank takes its chunks by arrival at any size (tests)
    int kd_wave_cap;     // SCA_KD_WAVE_CAP (256 .. 1536): largest subtree handed to k_kd_block; 0: chosen per build
    int solve_fb_max;    // SCA_SOLVE_FB_MAX: shards up to this many agents solve and fall back in one launch (k_solve_fb): while all the shard's
                         // wavefronts are resident at once even at the fallback sweep's 252 registers (two per SIMD)
    int action_fb_max;   // SCA_ACTION_FB_MAX: shards up to this many agents run the fallback sweep inside the epilogue's launch (k_action_fb)
    int lp_form;         // SCA_LP_FORM=lane|wave: 1 / 0 forces the K3 form of a shard (A/B measurements); -1 by the LP agents in the shard
    // read at sca_device_tracker_enable
    int trk_fuse;        // SCA_TRACKER_FUSE (set = 1): k_track_replan allowed (no list, hence no ordering by expected length: opt-in)
    int trk_group_fuse;  // SCA_TRACKER_NOGROUPFUSE (set = 0): k_track_group (decision + 64-lane search in one launch) for shards of <= spec4_max agents
    int spec4_max, spec3_max, spec2_max, mid_max;   // SCA_TRK_SPEC4_MAX ... SCA_TRK_MID_MAX: re-plans of a pass up to which k_replan_group<64 / 32 / 16 / 4>
                                                    // takes them (TRK_*_MAX per 1024 SIMDs); above mid_max one lane per plan
};

enum TunKind { TUN_FLAG01, TUN_SET, TUN_CLEAR, TUN_INT, TUN_LPFORM };   // atoi != 0 | set -> 1 | set -> 0 | atoi clamped to [lo, hi] | first letter l / w
enum TunWhen { TUN_AT_CREATE, TUN_AT_TRACKER };
struct TunRow { const char *name; int Tunables::*member; TunKind kind; TunWhen when; long long def; bool def_per_simd; int lo, hi; };
inline constexpr TunRow TUNABLES[] = {
    {"SCA_K1_PACKED", &Tunables::k1_force, TUN_FLAG01, TUN_AT_CREATE, -1, false, 0, 0},
    {"SCA_AUTO_BACKOFF_DIV", &Tunables::auto_div, TUN_INT, TUN_AT_CREATE, 8, false, 1, 64},
    {"SCA_AUTO_NO_TAIL", &Tunables::auto_no_tail, TUN_SET, TUN_AT_CREATE, 0, false, 0, 0},
    {"SCA_AUTO_TAIL_MAX", &Tunables::auto_tail_max, TUN_INT, TUN_AT_CREATE, 0, false, 0, INT_MAX},
    {"SCA_SOLVE_SPLIT", &Tunables::solve_split, TUN_FLAG01, TUN_AT_CREATE, -1, false, 0, 0},
    {"SCA_HOST_STEP_STAGED", &Tunables::hs_staged, TUN_FLAG01, TUN_AT_CREATE, 0, false, 0, 0},
    {"SCA_KD_TOP", &Tunables::kd_top, TUN_FLAG01, TUN_AT_CREATE, 1, false, 0, 0},
    {"SCA_EXT_STOP", &Tunables::ext_stop, TUN_FLAG01, TUN_AT_CREATE, 1, false, 0, 0},
    {"SCA_KD_TICKET", &Tunables::kd_force_ticket, TUN_FLAG01, TUN_AT_CREATE, 0, false, 0, 0},
    {"SCA_KD_WAVE_CAP", &Tunables::kd_wave_cap, TUN_INT, TUN_AT_CREATE, 0, false, 2 * KD_WAVE_FLOOR, KD_WAVE_CAP},
    {"SCA_SOLVE_FB_MAX", &Tunables::solve_fb_max, TUN_INT, TUN_AT_CREATE, 2048, true, INT_MIN, INT_MAX},
    {"SCA_ACTION_FB_MAX", &Tunables::action_fb_max, TUN_INT, TUN_AT_CREATE, 16384, true, INT_MIN, INT_MAX},
    {"SCA_LP_FORM", &Tunables::lp_form, TUN_LPFORM, TUN_AT_CREATE, -1, false, 0, 0},
    {"SCA_TRACKER_FUSE", &Tunables::trk_fuse, TUN_SET, TUN_AT_TRACKER, 0, false, 0, 0},
    {"SCA_TRACKER_NOGROUPFUSE", &Tunables::trk_group_fuse, TUN_CLEAR, TUN_AT_TRACKER, 1, false, 0, 0},
    {"SCA_TRK_SPEC4_MAX", &Tunables::spec4_max, TUN_INT, TUN_AT_TRACKER, TRK_SPEC4_MAX, true, INT_MIN, INT_MAX},
    {"SCA_TRK_SPEC3_MAX", &Tunables::spec3_max, TUN_INT, TUN_AT_TRACKER, TRK_SPEC3_MAX, true, INT_MIN, INT_MAX},
    {"SCA_TRK_SPEC2_MAX", &Tunables::spec2_max, TUN_INT, TUN_AT_TRACKER, TRK_SPEC2_MAX, true, INT_MIN, INT_MAX},
    {"SCA_TRK_MID_MAX", &Tunables::mid_max, TUN_INT, TUN_AT_TRACKER, TRK_MID_MAX, true, INT_MIN, INT_MAX},
};
// the rows of one moment: the default, then the environment.  A switch takes effect when its row is read and keeps its value until the next
// sca_create / sca_device_tracker_enable.
inline void tunables_from_env(Tunables &t, int simds, TunWhen when) {
    for (const TunRow &r : TUNABLES) {
        if (r.when != when) continue;
        int &v = t.*r.member;
        v = r.def_per_simd ? per_simd(simds, r.def) : (int)r.def;
        const char *e = std::getenv(r.name);
        if (!e) continue;
        switch (r.kind) {
        case TUN_FLAG01: v = std::atoi(e) != 0; break;
        case TUN_SET: v = 1; break;
        case TUN_CLEAR: v = 0; break;
        case TUN_INT: v = std::min(r.hi, std::max(r.lo, std::atoi(e))); break;
        case TUN_LPFORM: v = e[0] == 'l' ? 1 : (e[0] == 'w' ? 0 : -1); break;
        }
    }
}

// ---- SCA_NBR_AUTO ---------------------------------------------------------------------------------------------------------------------------
// SCA_NBR_AUTO resolves to a plain kd pass where it cannot help (the grid's candidate lists need the collision reach inside one cell: `fits`;
// a pass with the tracker inside runs its whole neighbour branch beside the re-plans already: nothing to gain, a grid build to lose) or where
// the grid keeps listing a large part of the swarm for the kd query anyway (a lattice of identical cells: ties everywhere) -- it is tried
// again every 256 passes.  A tree built ahead for this pass (sca_run_steps) makes it an AUTO pass whatever the counts say: the build must
// not run twice.
constexpr int AUTO_BACKOFF_PASSES = 256;
inline bool auto_lists_too_many(int kdq_last, int auto_div, int shard_count) { return kdq_last >= 0 && (long long)kdq_last * auto_div > (long long)shard_count; }
// auto_pass (false: a plain SCA_NBR_KDTREE pass) | the context's Auto::backoff and Auto::last after this decision | workgroups of
// k_neighbors_kd_auto, should the listed agents' kd query be a launch
struct AutoPlan { bool auto_pass; int auto_backoff, kdq_last, kdq_blocks; };
// vacancy_on: a row of the plain context is vacant (sca_vacancy.h) -- the grid build does not skip vacant rows, so the pass is the plain kd
// pass, as with scenes; nothing of the back-off is touched, and AUTO passes come back with the last admission (no tree is ever built ahead
// across a call, so kd_ahead is false there)
inline AutoPlan plan_auto(bool fits, bool tracked_pass, bool kd_ahead, int kdq_last, int auto_div, int auto_backoff, int shard_count, bool vacancy_on = false) {
    AutoPlan p{true, auto_backoff, kdq_last, KDQ_BLOCKS};
    if (vacancy_on) { p.auto_pass = false; return p; }
    if (!kd_ahead && auto_backoff == 0 && auto_lists_too_many(kdq_last, auto_div, shard_count)) { p.auto_backoff = AUTO_BACKOFF_PASSES; p.kdq_last = -1; }
    if (!kd_ahead && (!fits || tracked_pass || p.auto_backoff > 0)) {
        if (p.auto_backoff > 0) p.auto_backoff--;
        p.auto_pass = false;
    }
    if (p.kdq_last >= 0 && p.kdq_last <= KDQ_BLOCKS_FEW * K1_WAVES) p.kdq_blocks = KDQ_BLOCKS_FEW;
    return p;
}
// will the next pass of an SCA_NBR_AUTO run be an AUTO pass (and not a plain kd pass)?  Decides whether its tree may be built ahead.
inline bool auto_next(bool fits, bool tracked_pass, bool part_on, int kdq_last, int auto_div, int auto_backoff, int shard_count, bool vacancy_on = false) {
    return !vacancy_on && fits && auto_backoff == 0 && !part_on && !tracked_pass && !auto_lists_too_many(kdq_last, auto_div, shard_count);
}
// the launch-free form of the listed agents' kd query (the grid query's own last workgroup answers them, KdTail) for the build of pass `seq`:
// while the list lengths that have come back say "nobody" (auto_tail_max), and only with the wait-value form of the pass's wait
inline bool auto_tail_form(bool tail_ok, bool waitvalue, unsigned seq, int kdq_last, int auto_tail_max) {
    return tail_ok && waitvalue && seq != 0 && kdq_last >= 0 && kdq_last <= auto_tail_max;   // (seq wraps: the pass numbered 0 never takes the tail form)
}

// ---- the slot rule of an AUTO pass ---------------------------------------------------------------------------------------------------------------
// Pass `seq` (sca_ctx::Auto::seq + 1 while it is being enqueued; unsigned, it wraps) owns three slots.  Its list is the one of parity
// seq & 1: the pass two before filled and read the same one.  Event slot seq & 3 of Auto::ev_kdq fires when its kd query is through:
// recorded behind k_neighbors_kd_auto on the kd stream (the launch form), or behind its build's k_kd_block (the tail form, where the grid
// query's own last workgroup answers on the pass's stream).  `on_kd` has bit s set while the pass that last recorded slot s ran the launch
// form: only then must the list's next user wait for that slot before it resets and refills the list.  Slot builds & 1 of Auto::ev_gather
// is recorded behind every build's gather, the last kernel that reads a record buffer.
constexpr int AUTO_NO_SLOT = -1;
inline bool auto_on_kd(unsigned on_kd, unsigned slot) { return (on_kd >> (slot & 3u)) & 1u; }
// the build of pass seq = auto_seq + 1, enqueued inside that pass or ahead of it
struct AutoBuildPlan {
    unsigned seq;
    bool tail;          // auto_tail_form: the build's k_kd_block takes a KdTail and the pass launches no kd query
    int record_slot;    // ev_kdq slot recorded behind k_kd_block (the tail form only)
    int wait_slot;      // ev_kdq slot the PASS's stream waits on before this build is enqueued (the tail form only): the list's last reader
    int gather_slot;    // ev_gather slot recorded behind this build's gather (Auto::builds counts it afterwards)
};
inline AutoBuildPlan plan_auto_build(bool tail_ok, bool waitvalue, unsigned auto_seq, int kdq_last, int auto_tail_max, unsigned on_kd, unsigned builds) {
    AutoBuildPlan b{auto_seq + 1u, false, AUTO_NO_SLOT, AUTO_NO_SLOT, (int)(builds & 1u)};
    b.tail = auto_tail_form(tail_ok, waitvalue, b.seq, kdq_last, auto_tail_max);
    if (!b.tail) return b;
    b.record_slot = (int)(b.seq & 3u);
    // (seq wraps: passes 1 and 2 behind the wrap skip the wait like a context's first two, pass 0 never gets here)
    if (b.seq >= 3u && auto_on_kd(on_kd, b.seq - 2u)) b.wait_slot = (int)((b.seq - 2u) & 3u);
    return b;
}
enum AutoWait { AUTO_WAIT_NONE, AUTO_WAIT_VALUE, AUTO_WAIT_EVENT };   // how the pass's stream learns that the lists are final
struct AutoPassPlan {
    unsigned seq;       // what Auto::seq becomes with this pass
    int parity;         // the list this pass fills and reads
    int reuse_slot;     // ev_kdq slot the pass's stream waits on in front of its grid build (the kd query of two passes ago), or none
    bool tail;          // this pass's build was enqueued in the tail form: no kd query launch
    int kdq_slot;       // ev_kdq slot of this pass: recorded behind its kd query (on_kd_stream) or, by its build, behind k_kd_block
    bool on_kd_stream;  // the kd query is a launch on the kd stream: what bit kdq_slot of Auto::on_kd becomes
    unsigned on_kd;     // Auto::on_kd behind this pass
    bool copy_count;    // the list length is copied back behind this pass's kd query
    unsigned passes;    // Auto::passes behind this pass (it stands still while a copy is pending)
    int wait;           // AutoWait
    int gather_slot;    // ev_gather slot the integrate stage waits on: the build BEFORE this pass's read the buffer it writes
};
// after this pass's build has been enqueued (tail_seq and builds include it)
inline AutoPassPlan plan_auto_pass(unsigned auto_seq, unsigned tail_seq, unsigned on_kd, bool waitvalue, bool count_pending, unsigned passes, unsigned builds) {
    AutoPassPlan p{};
    p.seq = auto_seq + 1u;
    p.parity = (int)(p.seq & 1u);
    p.tail = tail_seq == p.seq && tail_seq != 0u;
    // (a build enqueued in the tail form has made the pass's stream wait already; seq wraps: pass 0 waits unless tail_seq is 0, passes 1 and 2 behind it do not)
    p.reuse_slot = auto_seq >= 2u && tail_seq != p.seq && auto_on_kd(on_kd, p.seq - 2u) ? (int)((p.seq - 2u) & 3u) : AUTO_NO_SLOT;
    p.kdq_slot = (int)(p.seq & 3u);
    p.on_kd_stream = !p.tail;
    p.on_kd = (on_kd & ~(1u << p.kdq_slot)) | ((p.on_kd_stream ? 1u : 0u) << p.kdq_slot);
    p.copy_count = !count_pending && (passes & 3u) == 0u;
    p.passes = count_pending ? passes : passes + 1u;
    p.wait = p.tail ? AUTO_WAIT_NONE : waitvalue ? AUTO_WAIT_VALUE : AUTO_WAIT_EVENT;
    p.gather_slot = (int)(builds & 1u);              // [builds & 1] = the one before the last
    return p;
}

// ---- a step of a burst: the events that ride --------------------------------------------------------------------------------------------------
// sca_run_steps knows, inside one call, what follows a step, and lets three things ride on kernels the step launches anyway (stop events
// of their dispatches, Tunables::ext_stop) or start early.  The single-step entry points plan none of them.
struct StepIn {
    int mode;                   // the neighbour mode the burst was called with
    int step, steps;            // this step of so many
    bool kd_stream;             // sca_ctx::Auto::stream exists (the first AUTO pass of a context creates it)
    bool ext_stop;              // Tunables::ext_stop
    bool comm;                  // a communicator is active
    bool whole;                 // the shard is the whole swarm
    bool trk_on, trk_in_pass, trk_fork;   // the tracker is enabled | runs inside the pass | its fork event exists
    bool paths_on;              // waypoint lists are set
    bool clear_on;              // the closest-approach records of the whole context are on
    bool auto_ran;              // the pass of this step was an AUTO pass
    bool fits, part_on; int kdq_last, auto_div, auto_backoff, shard_count;   // auto_next's inputs (tracked_pass is trk_on && trk_in_pass)
    bool missions_on = false;   // mission tables are set (sca_set_missions): the step's last kernel may still replace rows
    bool vacancy_on = false;    // a row is vacant (sca_retire_agents): every pass is the plain kd pass, nothing of SCA_NBR_AUTO rides or starts early
};
struct StepPlan {
    bool moved_on_action;       // k_action carries Auto::ev_moved.  None of its inputs is a result of the step's pass: asked in front of it
    bool build_ahead;           // the next pass's kd build is enqueued behind this step's collision check ...
    bool fork_rides;            // ... or the next pass's fork rides on this step's last kernel (plan_finish); both asked behind the pass
};
inline StepPlan plan_step(const StepIn &i) {
    StepPlan p{};
    const bool more = i.step + 1 < i.steps;
    // (SCA_NBR_AUTO, another step to follow: the moved positions' event rides on k_action -- the next pass's kd build waits on it)
    // (a shard: the records of the others arrive after k_action)
    p.moved_on_action = i.mode == SCA_NBR_AUTO && !i.vacancy_on && more && i.kd_stream && i.ext_stop && !i.comm && i.whole;
    // SCA_NBR_AUTO: the NEXT pass's kd build needs the moved positions only -- k_collide_finish changes flags, and in an AUTO pass its
    // fallback looks into the grid, not into the tree -- so it starts beside the collision check and the next pass's grid build and query.
    // Only inside one call: a caller who reads the permutation between calls sees as many builds as steps.
    // (not with the closest-approach records on: k_clearance reads this step's tree, which a build enqueued ahead would overwrite beside it)
    p.build_ahead = i.mode == SCA_NBR_AUTO && i.auto_ran && more && !i.clear_on &&
                    auto_next(i.fits, i.trk_on && i.trk_in_pass, i.part_on, i.kdq_last, i.auto_div, i.auto_backoff, i.shard_count, i.vacancy_on);
    // the next pass's fork (tracker in the pass, its neighbour branch on the side stream) rides on this step's last kernel
    // (not while waypoint lists are set: the next pass's k_waypoint must come before its fork)
    // (a step that builds ahead took the other branch: no tracker in an AUTO pass, no fork to carry)
    p.fork_rides = !p.build_ahead && more && i.ext_stop && i.trk_on && i.trk_in_pass && i.trk_fork && !i.paths_on;
    // mission tables: k_mission_advance, behind K4, may replace a row's position, heading and tracker record -- nothing of the next pass
    // starts from the moved positions before it has run, and the step's last kernel is not the one the fork would ride on
    if (i.missions_on) p = StepPlan{};
    return p;
}
// the env update's launches: which K4 instance runs, what follows it, and which of them is the step's last kernel -- the one that carries the
// event sca_run_steps hands over (plan_step's fork), if it hands one over
enum FinishK4 { K4_SCENE_OBS, K4_SCENES, K4_GRID, K4_PLAIN };              // k_collide_finish_scenes<SceneObsRoots | SceneRoots>, _grid, k_collide_finish
enum FinishCarrier { CARRY_K4, CARRY_HARVEST, CARRY_OTHERS };             // K4 | k_scene_harvest | k_goal_flags_others
struct FinishPlan { int k4, carrier; bool harvest, others; };
// harvest_on: the harvest block exists; last_mode: the neighbour structure of the last pass (sca_ctx::nbr_mode: K4's fallback looks there)
inline FinishPlan plan_finish(bool scenes_on, bool obs_on, bool harvest_on, bool part_on, bool shard_below_n, int last_mode) {
    FinishPlan p{};
    p.k4 = scenes_on ? (obs_on ? K4_SCENE_OBS : K4_SCENES) : last_mode == SCA_NBR_GRID ? K4_GRID : K4_PLAIN;
    p.others = part_on || shard_below_n;            // k_goal_flags_others behind K4 (and behind the harvest)
    p.harvest = scenes_on && harvest_on;            // (with the harvest the step's last kernel is k_scene_harvest, and the event rides on that one)
    p.carrier = p.others ? CARRY_OTHERS : p.harvest ? CARRY_HARVEST : CARRY_K4;
    return p;
}

// ---- the refusals of the entry points that step --------------------------------------------------------------------------------------------
// One list, in the order sca_run_steps makes them; an entry point names the checks it makes (sca_step_begin: no step count, and a mode out
// of range is the pass's to refuse; sca_step_host: the mode alone, under its own name) and its prefix.
enum StepCheck { STEP_CHK_STATE = 1, STEP_CHK_STEPS = 2, STEP_CHK_MODE = 4, STEP_CHK_RANKS = 8, STEP_CHK_PART_MODE = 16, STEP_CHK_ALL = 31 };
enum StepFault { STEPF_OK, STEPF_NO_STATE, STEPF_NEGATIVE_STEPS, STEPF_MODE, STEPF_PART_RANKS, STEPF_PART_MODE };
// part_ranks_apart: the partition spans several ranks and shard emulation is off
inline StepFault step_check(int checks, bool state_set, int steps, int mode, bool part_on, bool part_ranks_apart) {
    if ((checks & STEP_CHK_STATE) && !state_set) return STEPF_NO_STATE;
    if ((checks & STEP_CHK_STEPS) && steps < 0) return STEPF_NEGATIVE_STEPS;
    if ((checks & STEP_CHK_MODE) && (mode < SCA_NBR_KDTREE || mode > SCA_NBR_AUTO)) return STEPF_MODE;   // (also for steps == 0: a wrong mode is a wrong call)
    if ((checks & STEP_CHK_RANKS) && part_on && part_ranks_apart) return STEPF_PART_RANKS;
    if ((checks & STEP_CHK_PART_MODE) && part_on && mode != SCA_NBR_GRID) return STEPF_PART_MODE;
    return STEPF_OK;
}
inline const char *step_fault_text(StepFault f) {
    switch (f) {
    case STEPF_NO_STATE: return "sca_set_state first";
    case STEPF_NEGATIVE_STEPS: return "steps must not be negative";
    case STEPF_MODE: return "neighbor mode not available in this build";
    case STEPF_PART_RANKS: return "cell-owner partition over several ranks: drive the step with sca_step_begin / sca_partition_pack / [exchange] / "
                                  "sca_partition_unpack / sca_partition_commit / sca_step_end (sca_amd.distributed.PartitionedStepper)";
    case STEPF_PART_MODE: return "the cell-owner partition is a mode of SCA_NBR_GRID";
    default: return "";
    }
}
inline int step_fault_code(StepFault f) {
    return f == STEPF_OK ? 0 : f == STEPF_NEGATIVE_STEPS ? SCA_ERR_ARG : f == STEPF_MODE || f == STEPF_PART_MODE ? SCA_ERR_UNSUPPORTED : SCA_ERR_STATE;
}

// ---- the solve and its neighbours ------------------------------------------------------------------------------------------------------------
// K3 form: one lane per agent (k_lp) once the shard has enough LP agents to fill the chip that way -- measured: 100 000 agents 65 vs 106 us,
// 4096 agents 23 vs 12 us (a lane alone needs ~12 us for its 16 planes and the LP) --, else the wave-per-agent form (k_solve_lpw).
constexpr int LP_LANE_MIN = 16384;              // one lane per LP agent once they fill the chip: 16 agents per SIMD
// (under the cell-owner partition ownership is dynamic: the LP kernels walk all owned agents and skip the others, the share of LP agents
// decides the form, and SCA_LP_FORM does not apply)
inline int choose_lp_form(const Tunables &t, int simds, bool part_on, int part_nranks, long long lp_total, int lp_in_shard) {
    if (part_on) return lp_total / std::max(1, part_nranks) >= per_simd(simds, LP_LANE_MIN) ? 1 : 0;
    if (t.lp_form == 1) return lp_in_shard > 0 ? 1 : 0;
    if (t.lp_form == 0) return 0;
    return lp_in_shard >= per_simd(simds, LP_LANE_MIN) ? 1 : 0;
}
// k_solve as k_solve_sweep (beside the re-plans) + k_solve_pick4 (behind them)?  It pays while the re-plans are the longer
// branch of the pass: the lane-per-plan kernel takes ~0.2 + 0.235 * (wavefronts per SIMD, rounded up) ms whatever the
// count inside a round, the neighbour chain grows with the shard.  Measured on the circle (96 % of the agents re-plan per
// step), shard sizes 24 576 ... 262 144: a gain of 5-10 % of the step up to 61 440 agents in the first round and up to
// ~114 000 in the second, a loss of 3-7 % elsewhere (the sweep then lengthens the branch that already ends last).
inline bool choose_solve_split(const Tunables &t, int simds, bool overlap, int cnt, int trk_last_count) {
    if (t.solve_split >= 0) return t.solve_split != 0;
    if (!overlap) return false;
    const int est = trk_last_count >= 0 ? trk_last_count : cnt;    // re-plans of a recent pass (all agents before the first readback)
    if (est <= t.mid_max) return false;           // the many-lanes-per-plan forms: short re-plans, nothing to hide behind (measured equal
                                                  // with and without at 18 000 .. 30 000 agents)
    const int per_round = 64 * simds;             // plans of the lane-per-plan kernel that are one wavefront per SIMD
    const int rounds = (est + per_round - 1) / per_round;
    return rounds == 1 ? cnt <= per_simd(simds, 61440) : (rounds == 2 ? cnt <= per_simd(simds, 114688) : false);
}
struct SolvePlan {
    bool packed;       // K1 of a kd pass: four agents per wavefront (k_neighbors_kd4)
    bool split;        // k_solve_sweep + k_solve_pick4
    bool solve_fb;     // k_solve_fb (solves and finishes its own fallbacks)
    bool lpw;          // k_solve_lpw behind k_solve: the shard's (few) LP agents, one wavefront each
    int lp_kernel;     // 1: k_lp, one lane per LP agent (DeviceView::lp_kernel)
    bool action_fb;    // k_action_fb (else k_fallback, unless solve_fb, + k_action)
    int forms;         // SCA_FORM_SOLVE_SPLIT | SOLVE_FB | LP_LANE | ACTION_FB
};
// cnt: agents of the shard; lp_in_shard: its LP agents (under the partition: the range the LP kernels walk); overlap: the neighbour branch
// runs beside the tracker's re-plans; no_sweep_scratch: the two-launch solve was wanted and its scratch could not be allocated -- the pass
// runs the one-launch k_solve instead (and, as ever, not k_solve_fb)
inline SolvePlan plan_solve(const Tunables &t, int simds, int cnt, bool part_on, int part_nranks, long long lp_total, int lp_in_shard, bool overlap,
                            int trk_last_count, bool no_sweep_scratch) {
    SolvePlan p{};
    // packed K1 wins once the shard fills the chip (measured: 2.3x at 16k agents, equal at 6000); below that the one-agent-per-wave form
    // with its record stack has the shorter critical path (4096 random: 30 % faster)
    p.packed = t.k1_force < 0 ? cnt >= per_simd(simds, 6144) : t.k1_force != 0;
    const bool split_wanted = choose_solve_split(t, simds, overlap, cnt, trk_last_count);
    p.split = split_wanted && !no_sweep_scratch;
    // k_solve_fb: ... and while nobody else feeds the fallback list (k_lp does)
    p.solve_fb = !split_wanted && lp_in_shard == 0 && !part_on && cnt <= t.solve_fb_max;
    p.lp_kernel = choose_lp_form(t, simds, part_on, part_nranks, lp_total, lp_in_shard);
    if (p.split && lp_in_shard > 0) p.lp_kernel = 1;               // k_solve_pick4 carries no LP: its agents go to k_lp
    p.lpw = !p.split && !p.solve_fb && !p.lp_kernel && lp_in_shard > 0;
    p.action_fb = !p.solve_fb && cnt <= t.action_fb_max;          // (small shards: the fallback sweep rides in the epilogue's launch)
    p.forms = (p.split ? SCA_FORM_SOLVE_SPLIT : 0) | (p.solve_fb ? SCA_FORM_SOLVE_FB : 0) | (p.lp_kernel ? SCA_FORM_LP_LANE : 0) |
              (p.action_fb ? SCA_FORM_ACTION_FB : 0);
    return p;
}

// ---- the tracker's re-plans --------------------------------------------------------------------------------------------------------------------
// The device-side count of a pass decides which re-plan kernel does the work: every launched kernel reads it and returns unless it falls
// into its range (lo, hi].  Launching all five every pass would cost four empty launches on the critical path; the count of an earlier pass
// (`last_count`, -1: unknown) says which of them can be left out (25 % hysteresis on both sides of a form's natural range) -- the ranges
// of those that are launched are widened so that every count is still somebody's (a count that jumps is then re-planned by a form that is
// slower for it, never by nobody).  When nearly the whole shard re-plans in the lane-per-plan form, k_track's list is not worth its launch
// either: k_track_replan does both (`fused`); a shard of so few agents that each can have a wavefront (and a SIMD) gets decision and
// search in one launch (k_track_group, `group_fused`).  trk_many, the per-agent form (more classes of (turning radius, pitch limits) than
// launches are worth): a wavefront per plan at ANY count.
enum ReplanKernel { RP_GROUP64, RP_GROUP32, RP_GROUP16, RP_GROUP4, RP_LANE, RP_TRACK_GROUP, RP_TRACK_REPLAN };
// a launch takes the pass when lo < (re-plans of the pass) <= hi; its grid must hold `plans` plans at `lanes` lanes each
struct ReplanLaunch { int kernel /* ReplanKernel */, lo, hi, plans, lanes; };
struct ReplanPlan {
    bool fused, group_fused;   // k_track_replan / k_track_group: no k_track launch in front
    int n;                     // launches, in order (per class of tracked agents)
    ReplanLaunch launch[5];
    int forms;                 // SCA_FORM_TRACK_FUSED | REPLAN_FEW | REPLAN_LANE
};
inline ReplanPlan plan_replans(const Tunables &t, int cnt, int last_count, bool trk_many, bool in_pass, bool part_on) {
    static constexpr int LANES[5] = {64, 32, 16, 4, 1};
    ReplanPlan p{};
    const int lc = last_count;
    const bool known = lc >= 0;
    // forms 0..3: k_replan_group<64 / 32 / 16 / 4> with the natural ranges (up[i - 1], up[i]]; form 4: one lane per plan, above
    int up[5] = {t.spec4_max, t.spec3_max, t.spec2_max, t.mid_max, INT_MAX};
    for (int i = 1; i < 4; i++) up[i] = std::max(up[i], up[i - 1]);
    bool want[5];
    int nwant = 0;
    for (int i = 0; i < 5; i++) {
        const long long lower = i ? up[i - 1] : -1, upper = up[i];
        const bool possible = cnt > lower && upper > lower;
        want[i] = possible && (!known || (lc > lower - lower / 4 && (i == 4 || lc <= upper + upper / 4)));
        nwant += want[i];
    }
    if (nwant == 0) { want[4] = true; nwant = 1; }
    if (trk_many) { want[0] = true; for (int i = 1; i < 5; i++) want[i] = false; nwant = 1; }
    const bool lane = want[4];
    p.fused = in_pass && lane && nwant == 1 && t.trk_fuse && !part_on && (long long)lc * 4 >= (long long)cnt * 3;
    p.group_fused = in_pass && t.trk_group_fuse && !part_on && cnt <= t.spec4_max;
    if (p.group_fused) {
        p.forms = SCA_FORM_TRACK_FUSED | SCA_FORM_REPLAN_FEW;
        p.launch[p.n++] = ReplanLaunch{RP_TRACK_GROUP, -1, INT_MAX, cnt, 64};
        return p;
    }
    p.forms = (p.fused ? SCA_FORM_TRACK_FUSED : 0) | (nwant > (lane ? 1 : 0) ? SCA_FORM_REPLAN_FEW : 0) | (lane ? SCA_FORM_REPLAN_LANE : 0);
    if (p.fused) {
        p.launch[p.n++] = ReplanLaunch{RP_TRACK_REPLAN, -1, INT_MAX, cnt, 1};
        return p;
    }
    int prev_up = -1, left = nwant;
    for (int i = 0; i < 5; i++) {
        if (!want[i]) continue;
        left--;
        const int lo = prev_up, hi = left ? up[i] : INT_MAX;           // the first launched form starts at 0, the last one takes the rest
        prev_up = up[i];
        const int plans = hi == INT_MAX ? cnt : std::min(cnt, up[i]);
        if (plans <= 0) continue;                                      // (a range moved to nothing by the tuning switches)
        p.launch[p.n++] = ReplanLaunch{i, lo, hi, plans, LANES[i]};
    }
    return p;
}

// ---- the kd build ------------------------------------------------------------------------------------------------------------------------------
// wave_max, the size of the subtrees handed to k_kd_block: 1.25 x the average node size of the first level that fits (n / 2^k), so that
// the nodes of that level -- all within a few per cent of the average -- are on one side of it.
// Subtrees of up to 1536 members (one workgroup of 12 wavefronts each) when the build has the chip to itself; up to 1024 when it
// runs beside the tracker's re-plans (a side stream): twice as many, smaller workgroups spread over twice as many CUs, each
// competing with fewer re-plan wavefronts -- measured at c5 (N = 16 384, 16 subtrees of ~1024 against 32 of ~512): step 0.284
// -> 0.268 ms; c3 (no tracker, 4 against 8 subtrees) the other way round: 0.127 against 0.129.
// A tree of up to KT_M members: its top by one workgroup in LDS (k_kd_top), which is cheap enough per level to go one level
// further down than the level passes would -- subtrees of ~512 instead of ~1024 members for k_kd_block
// (not beside the tracker's re-plans, whose ~250-register wavefronts sit on every SIMD: a workgroup of sixteen wavefronts and 139 KB
// of LDS then waits for room and for issue slots -- measured as a middle tier under the level passes: 60 us instead of 30 at c5).
// Level passes: two launches per level (rank | swap) while the nodes span several chunks, then ONE launch (k_kd_level_tail) in which every
// remaining node's workgroup finishes its whole subtree down to wave_max.  Where the switch happens (first_single) only sets the speed --
// the tail handles any node size and any depth -- so it is taken from the statistics of an earlier build when they have arrived
// (single_hint: 1 + the first level whose nodes all fit one chunk, 0: unknown), otherwise from the balanced tree.
struct KdBuildPlan {
    bool top;             // k_kd_top instead of the level passes
    int wave_max;         // KdScratch::wave_max
    int block;            // the k_kd_block<block, block / 2> instance: the smallest form that holds wave_max members (two positions per thread)
    bool level_passes;    // first_single x (k_kd_lv_rank | k_kd_lv_swap), then k_kd_level_tail at level first_single
    int first_single, grid;
    bool ticket;          // k_kd_lv_rank<true>: chunks by arrival, once a level can have more chunks than are resident at once (or forced)
    int levels;           // what k_kd_block is told: the levels above it
    int sgrid;            // workgroups of k_kd_block
};
inline KdBuildPlan plan_kd_build(const Tunables &t, int n, bool beside, int single_hint, int chunk_cap, int rank_capacity) {
    KdBuildPlan p{};
    p.top = t.kd_top && n <= KT_M && !beside;
    const int cap = t.kd_wave_cap > 0 ? t.kd_wave_cap : (p.top ? 768 : (beside ? 1024 : KD_WAVE_CAP));
    p.wave_max = (n <= 1024 && cap >= 1024) ? 1024 : cap;   // a tree that fits one workgroup: the smaller one if it can
    if (n > cap) {
        double sz = (double)n;
        while (sz > cap / 1.25) sz *= 0.5;
        p.wave_max = std::min(cap, std::max(cap / 2 + 1, (int)std::ceil(1.25 * sz)));
    }
    p.block = p.wave_max <= 256 ? 256 : p.wave_max <= 512 ? 512 : p.wave_max <= 768 ? 768 : p.wave_max <= 1024 ? 1024 : p.wave_max <= 1280 ? 1280 : KD_WAVE_CAP;
    if (n > p.wave_max && p.top) p.levels = 1;
    else if (n > p.wave_max) {
        p.level_passes = true;
        p.first_single = 1;
        while (((long long)KD_CHUNK << p.first_single) < n) p.first_single++;   // n / 2^l <= KD_CHUNK
        p.first_single += 1;                                                    // uneven midpoint splits
        if (single_hint > 0) p.first_single = single_hint - 1;
        p.first_single = std::min(p.first_single, KD_MAX_LEVELS - 2);
        p.levels = p.first_single + 1;
        p.grid = std::min(chunk_cap, n / KD_CHUNK + n / (p.wave_max / 2 + 1) + 8);   // >= chunks of any level of n agents (a node of the level passes has > wave_max members... its children > 0)
        p.ticket = p.grid > rank_capacity || t.kd_force_ticket;
    }
    p.sgrid = std::max(1, std::min(1024, 4 * n / p.wave_max + 2));
    return p;
}

// The forest of a context with scenes (sca_set_scenes): every scene is a root job of k_kd_block -- no top, no level passes.  The instance is
// the smallest that holds the largest scene, one workgroup per scene up to the grid cap of the plain build, strided beyond it.
constexpr int KD_FOREST_GRID_MAX = 1024;
struct KdForestPlan {
    int block;            // the k_kd_block<block, block / 2> instance
    int grid;             // its workgroups
};
inline KdForestPlan plan_kd_forest(int largest_scene, int nscenes) {
    KdForestPlan p{};
    p.block = largest_scene <= 256 ? 256 : largest_scene <= 512 ? 512 : largest_scene <= 768 ? 768 : largest_scene <= 1024 ? 1024 : largest_scene <= 1280 ? 1280 : KD_WAVE_CAP;
    p.grid = std::max(1, std::min(KD_FOREST_GRID_MAX, nscenes));
    return p;
}

}  // namespace sca
