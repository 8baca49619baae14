// sca_scenes.hip.h -- scene batches (sca_set_scenes): many isolated episodes stepped by one context's passes.
//
// Scene s is the contiguous agent range [offsets[s], offsets[s + 1]).  Everything per agent in a pass (prologue, solve, LP, tracker, epilogue,
// integrate) neither knows nor cares which scene an agent belongs to and is launched unchanged on the whole range.  Three places do care,
// and their scene forms live here:
//   the kd-tree     a FOREST: scene s is one root job of k_kd_block, its nodes numbered from 2 * offsets[s] (kdTree.py:60-122 numbers a
//                   subtree contiguously from its root: k members occupy 2k - 1 nodes, so the ranges are disjoint inside awide[2n]); a job
//                   only permutes inside [begin, end), so the permutation never leaves a scene -- k_kd_scene_jobs writes the job table behind
//                   the unchanged k_kd_gather
//   the two queries k_neighbors_kd_scenes<HAS_OBS, Roots> / k_neighbors_kd4_scenes<HAS_OBS, Roots> start an agent's traversal of the agent
//                   tree at its scene's root; a shared obstacle tree (sca_set_obstacles) starts at 0
//   collide / done  k_collide_finish_scenes<Roots>: the bootstrap traversal from the scene's root, and the live count per scene as well as in total
// A context without scenes launches none of these, and SceneView is an argument of these kernels only (as PathView is of k_waypoint's).
//
// One obstacle set per scene (sca_set_scene_obstacles): the obstacle tree is a forest too, built on the host (sca_scenes.h), and the
// three kernels above are templated on where an agent's walks start: SceneRoots (the scene's agent root, obstacle walks from 0) or
// SceneObsRoots, whose obstacle walks start at the scene's own obstacle root, or do not happen for a scene without obstacles.  Those roots
// travel in SceneObsView, a member of SceneObsRoots only: a context with a shared set runs the SceneRoots instances, the code it ran before.
// Obstacle slots (sca_set_scene_obstacle_slots): a scene's obstacle range is a capacity, and since the walks start at a root word they load
// and reach obstacles only through the tree's links, a restart that brings obstacles (k_scene_restart) installs a new tree into the
// scene's part of the forest and rewrites that word -- the three kernels above do not change.  k_scene_restart is the ONE restart kernel,
// behind sca_restart_scenes, _sized and _obstacles alike: a scene filled to its capacity vacates an empty range, a scene that keeps its
// obstacle set returns behind its agent rows, so the narrower calls are degenerate cases of the widest and need no kernels of their own.
// Waypoint lists (Agent.path) under restarts: the block form of sca_set_paths is one CSR block for the whole context, which no kernel can
// edit per scene; in slot form (sca_set_path_slots; PathSlotView and k_waypoint_slots, sca_kernels.hip.h) every agent row owns room for W
// waypoints, and k_scene_restart also scatters a named scene's lists to its rows' rooms and resets their cursors (scene_restart_paths,
// behind sca_restart_scenes_paths) -- and gives the rows empty lists where the call brought none.
#pragma once
#include "sca_kdbuild.hip.h"
#include "sca_scenes.h"

namespace sca {

struct SceneView {
    const int32_t *scene_of;  // [n] the agent's scene
    const int32_t *offsets;   // [nscenes + 1]
    int32_t *live;            // [nscenes * 32] agents of the scene that are not done after the last env update, ONE 128-BYTE LINE PER SCENE
                              // (atomics serialise per line at the L2, DeviceView::done_count) -- and a wavefront adds its agents of a scene at once
    int32_t *prev;            // [nscenes] `live` as the step that is under way found it (between a policy pass and its env update)
    int32_t *steps;           // [nscenes] steps taken while the scene was live
    double *heading_keep;     // [n * 3] the headings as the last step of a LIVE scene left them: what a finished scene's agents get back (SceneCount)
    int nscenes;
};
constexpr int SCENE_LINE = 32;           // int32 per counter line

struct SceneObsView {
    const int32_t *oroot;     // [nscenes] record of owide / otree the scene's obstacle walks start at (2 * obs_offsets[s]), -1: the scene has no obstacles
                              // (behind it in the same allocation: [nscenes] the obstacles each scene holds, which no kernel of a step reads)
};
// Where an agent's walks start (RootZero, sca_kernels.hip.h): one kernel argument, by value.  Two dependent loads per agent and root (its
// scene, the scene's root); every lane that serves an agent reads the same words.
struct SceneRoots {           // one obstacle set shared by all scenes, or none
    SceneView v;
    __device__ __forceinline__ int operator()(int agent) const { return 2 * v.offsets[v.scene_of[agent]]; }
    __device__ __forceinline__ int obstacles(int) const { return 0; }
};
struct SceneObsRoots {        // one obstacle set per scene (sca_set_scene_obstacles)
    SceneView v;
    SceneObsView o;
    __device__ __forceinline__ int operator()(int agent) const { return 2 * v.offsets[v.scene_of[agent]]; }
    __device__ __forceinline__ int obstacles(int agent) const { return o.oroot[v.scene_of[agent]]; }
};

// start of a step, one thread per scene: a scene that is live when a step begins has taken that step (the reference's `while not env.step()`
// calls env.step() done_step + 1 times); the live counter starts from zero for this step's k_collide_finish_scenes
__device__ __forceinline__ void scene_begin_one(const SceneView &v, int s) {
    const int was = v.live[s * SCENE_LINE];
    v.prev[s] = was;
    if (was > 0) v.steps[s] += 1;
    v.live[s * SCENE_LINE] = 0;
}
__global__ __launch_bounds__(256) void k_scene_begin(SceneView v) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < v.nscenes) scene_begin_one(v, s);
}

// The forest's job table, behind k_kd_gather (which rewrites the single root job, the counts and the root's chunk records on every build):
// one root job per scene and nothing for the level passes.  begin: this build opens a step (scene_begin_one).  size: [nscenes] the agents a
// scene holds in the first rows of its range (sca_restart_scenes_sized; the range's length where it is full) -- the rows behind them are in
// no tree.  An argument of its own: SceneView travels by value to the K1 and K4 scene kernels, which do not need it.
__global__ __launch_bounds__(256) void k_kd_scene_jobs(KdScratch s, SceneView v, const int32_t *size, int begin) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) { s.counts[0] = 0; s.nchunks[0] = 0; s.counts[KD_MAX_LEVELS] = v.nscenes; }
    if (t >= v.nscenes) return;
    KdJob j; j.begin = v.offsets[t]; j.end = j.begin + size[t]; j.node = 2 * j.begin; j.pad = -1;     // pad = -1: a root, no parent record
    s.small[t] = j;
    if (begin) scene_begin_one(v, t);
}

// the live counters from the records themselves (a state that came from outside: sca_set_scenes, sca_set_state, the host state block), one
// wavefront per scene
__global__ __launch_bounds__(256) void k_scene_recount(DeviceView d, SceneView v) {
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (s >= v.nscenes) return;
    int cnt = 0;
    for (int a = v.offsets[s] + lane; a < v.offsets[s + 1]; a += 64) {
        cnt += (d.rec[a].flags & (FLAG_AT_GOAL | FLAG_COLLISION | FLAG_TIMEOUT)) ? 0 : 1;
        for (int k = 0; k < 3; k++) v.heading_keep[a * 3 + k] = d.heading[a * 3 + k];
    }
    cnt = wave_sum_i32(cnt);
    if (lane == 0) v.live[s * SCENE_LINE] = cnt;
}

// ---- restarting scenes in place (sca_restart_scenes) ------------------------------------------------------------------------------------------
// One workgroup per named scene, striding over the scene's agents; the new episode is read across the link from the library's page-locked
// staging block (RestartLayout, sca_scenes.h), as k_host_ingest reads the host state block.  Afterwards every per-agent word of the scene
// that a later pass READS BEFORE IT WRITES is what sca_set_agents + sca_set_state (+ sca_device_tracker_enable) leave in a context of that
// episode alone -- the arrays are listed in DESIGN.md section 5 with the reason for each.  Words of other scenes are not touched: the only
// shared words written are the step counters of K4 (done_count: an agent that was done counts as running again).
typedef uint32_t __attribute__((may_alias)) restart_u32;
struct RestartDev {
    // the arrays of DeviceView / SceneView / TrackDev a restart writes
    PubRec *rec;
    double *heading, *heading_keep, *total_dist, *goal, *pref_speed, *max_run_dist, *vpref_ext;
    int32_t *step_num;
    uint8_t *policy, *zaxis, *vpref_mode, *nbr_valid;
    int32_t *aperm, *nbr_n, *near_n, *done_count;
    const int32_t *offsets;
    int32_t *live, *prev, *steps;
    // the device tracker's, null without one
    double *trk_nbr0, *trk_goal_heading;
    restart_u32 *trk_st;            // the AgentTrack records as 4-byte words
    const restart_u32 *trk_init;    // one default-constructed record
    int trk_words;                  // sizeof(AgentTrack) / 4
    sca_scene_clearance *clear;     // [n] the closest-approach records (sca_scene_clearance_enable), null: off
};
constexpr int RESTART_T = 256;
// rows [lo, lo + ns) of a named scene from the block's rows row0 .. row0 + ns - 1: what a restart writes for a row an agent occupies
__device__ __forceinline__ void scene_restart_fill(const RestartDev &d, const uint8_t *blk, const RestartLayout &L, uint32_t has, int row0, int lo, int ns, int t) {
    const double *pos = (const double *)(blk + L.off[RS_POS]) + 3 * (int64_t)row0;
    const double *head = (const double *)(blk + L.off[RS_HEADING]) + 3 * (int64_t)row0;
    const double *goal = (const double *)(blk + L.off[RS_GOAL]) + 3 * (int64_t)row0;
    const double *gh = (const double *)(blk + L.off[RS_GOAL_HEADING]) + 3 * (int64_t)row0;
    const float *vel = (const float *)(blk + L.off[RS_VEL]) + 3 * (int64_t)row0;
    // three-component rows: consecutive lanes read and write consecutive words
    for (int w = t; w < 3 * ns; w += RESTART_T) {
        const int64_t g = 3 * (int64_t)lo + w;
        const double h = head[w];
        d.heading[g] = h; d.heading_keep[g] = h;
        d.vpref_ext[g] = 0.0;
        if (has & RESTART_HAS_GOAL) d.goal[g] = goal[w];
        if ((has & RESTART_HAS_GOAL_HEADING) && d.trk_goal_heading) d.trk_goal_heading[g] = gh[w];
    }
    for (int i = t; i < ns; i += RESTART_T) {
        const int a = lo + i, r = row0 + i;
        const PubRec old = d.rec[a];
        PubRec nw;
        nw.px = pos[3 * i]; nw.py = pos[3 * i + 1]; nw.pz = pos[3 * i + 2];
        nw.vx = vel[3 * i]; nw.vy = vel[3 * i + 1]; nw.vz = vel[3 * i + 2];
        nw.flags = 0u;
        nw.radius = (has & RESTART_HAS_RADIUS) ? ((const double *)(blk + L.off[RS_RADIUS]))[r] : old.radius;
        d.rec[a] = nw;
        // K4's counters of the last step: an agent that was done runs again (sca_active_count between steps).  Right while the counters
        // describe the last step's records; directly behind sca_set_state they are zero until the first step recounts
        if (old.flags & (FLAG_AT_GOAL | FLAG_COLLISION | FLAG_TIMEOUT)) atomicAdd(&d.done_count[(a & 255) * 32], 1);
        d.total_dist[a] = 0.0; d.step_num[a] = 0;
        if (has & RESTART_HAS_PREF_SPEED) d.pref_speed[a] = ((const double *)(blk + L.off[RS_PREF_SPEED]))[r];
        if (has & RESTART_HAS_MAX_RUN_DIST) d.max_run_dist[a] = ((const double *)(blk + L.off[RS_MAX_RUN_DIST]))[r];
        d.policy[a] = (blk + L.off[RS_POLICY])[r];
        if (has & RESTART_HAS_ZAXIS) d.zaxis[a] = (blk + L.off[RS_ZAXIS])[r];
        d.vpref_mode[a] = (blk + L.off[RS_VPREF_MODE])[r];
        d.aperm[a] = a;                                                // the scene's kdTree.agentIDs starts as 0 .. n_s - 1 again
        d.nbr_n[a] = 0; d.nbr_valid[a] = 0; d.near_n[a] = -1;
        if (d.trk_nbr0) d.trk_nbr0[a] = -1.0;
    }
    if (d.trk_st)                                                      // the AgentTrack records, word by word from the one initial record
        for (int64_t w = t; w < (int64_t)ns * d.trk_words; w += RESTART_T) d.trk_st[(int64_t)lo * d.trk_words + w] = d.trk_init[w % d.trk_words];
}

// Slots of a capacity (sca_restart_scenes_sized): the named scene takes new_size[b] agents into its first rows, and the rows behind them,
// up to the capacity offsets[s + 1], are VACATED.  A vacant row is an agent that is settled for good, by the rule collide_finish_body
// already has: flags FLAG_AT_GOAL | FLAG_COLLISION.  Every policy kernel skips it (mampenv.py:35) and its action row stays zero; K4 never
// traverses for it (settled, and not `arrived_only`, which asks for FLAG_AT_GOAL alone) and cannot add a flag (total_dist 0 never passes
// max_run_dist); the integrate stage leaves its position, a zero heading (pi_2_pi(0) = 0), total_dist and -- at its goal -- step_num as
// they are; the tracker does not own it (tracker_owns wants flags 0).  It stands in no tree: k_kd_scene_jobs ends the scene's job at
// size[s], so nobody's neighbour list, near list or collision walk can hold it, and the permutation behind the job stays the identity this
// kernel writes.  The row keeps its position, radius and constants (goal, pref_speed, max_run_dist, policy, zaxis, v_pref mode): valid
// numbers for the passes that still read them, replaced when an episode occupies the row again.
// done_count (live agents of the last step): an occupied row that was done counts again (scene_restart_fill), a vacated row that was
// running no longer does; done -> vacant and running -> occupied change nothing.
__device__ __forceinline__ void scene_restart_vacate(const RestartDev &d, int lo, int hi, int t) {
    for (int64_t g = 3 * (int64_t)lo + t; g < 3 * (int64_t)hi; g += RESTART_T) { d.heading[g] = 0.0; d.heading_keep[g] = 0.0; d.vpref_ext[g] = 0.0; }
    for (int a = lo + t; a < hi; a += RESTART_T) {
        PubRec *r = d.rec + a;                                         // (position and radius stay)
        if (!(r->flags & (FLAG_AT_GOAL | FLAG_COLLISION | FLAG_TIMEOUT))) atomicAdd(&d.done_count[(a & 255) * 32], -1);
        r->vx = 0.0f; r->vy = 0.0f; r->vz = 0.0f;
        r->flags = FLAG_AT_GOAL | FLAG_COLLISION;
        d.total_dist[a] = 0.0; d.step_num[a] = 0;
        d.aperm[a] = a;
        d.nbr_n[a] = 0; d.nbr_valid[a] = 0; d.near_n[a] = -1;
        if (d.trk_nbr0) d.trk_nbr0[a] = -1.0;
    }
    if (d.trk_st)
        for (int64_t w = (int64_t)lo * d.trk_words + t; w < (int64_t)hi * d.trk_words; w += RESTART_T) d.trk_st[w] = d.trk_init[w % d.trk_words];
}
// The one restart kernel, behind all three entry points.  new_size: [count] the rows each named scene brings, in the order of the block's
// ids (host memory, read across the link like the block); size: [nscenes] the device's sizes, which k_kd_scene_jobs reads.  The host has
// checked 1 <= new_size[b] <= capacity (scene_restart_check).  The agent rows by the functions above, then, for a scene whose head words
// say so, its part of the obstacle forest from the block's obstacle sections (RestartObsLayout, sca_scenes.h): records, sorted records,
// permutation, both node arrays, and last the root word the scene's walks start at and the count.  One kernel suffices because the two
// narrower calls are its degenerate cases, bit for bit: a scene that fills its capacity (sca_restart_scenes) vacates an empty range and
// writes the size it has, and a scene that keeps its set (head count -1: every scene of a call without obs_counts) returns behind the agent
// rows, before anything of RestartObsDev is read -- whose pointers are null in a context without a set per scene.
// Every obstacle word written lies in the named scene's rows [base, base + k) or node records [2 base, 2 base + 2k - 1), inside its
// capacity (the host checked k against it); rows and records behind them keep what an earlier set left -- no link of the new tree leads
// there, and the root is the only way in.  No atomics.
// The 32-, 64- and 128-byte records travel as 16-byte pieces, consecutive lanes on consecutive pieces: a wavefront's load covers 1 KB of
// consecutive bytes of the block across the link, and its store the same in device memory.
typedef uint32_t __attribute__((ext_vector_type(4), may_alias)) restart_piece;
static_assert(sizeof(ObsRec) == RO_REC_BYTES && sizeof(KdNode) == RO_TREE_BYTES && sizeof(KdWide) == RO_WIDE_BYTES, "RestartObsLayout's records");
struct RestartObsDev {
    ObsRec *obs, *obs_sorted;     // [M]
    int32_t *operm;               // [M]
    KdNode *otree;                // [2M]
    KdWide *owide;                // [2M]
    int32_t *oroot, *ocount;      // [nscenes]
};
__device__ __forceinline__ void scene_restart_pieces(void *dst, const void *src, int64_t pieces, int t) {
    restart_piece *to = (restart_piece *)dst;
    const restart_piece *from = (const restart_piece *)src;
    for (int64_t w = t; w < pieces; w += RESTART_T) to[w] = from[w];
}
// A restart that brings attributes (sca_restart_scenes_attrs): with RESTART_HAS_ATTRS the block's attribute sections (RestartAttrLayout,
// sca_scenes.h) hold one AgentPar record and one neighborDist per packed row, with RESTART_HAS_PLANNER the planner triple and the class
// byte; they go to rows [lo, lo + ns) of the context's per-agent arrays -- the rows the episode occupies, and no others: a vacant row
// keeps its attributes, as it keeps its constants.  The 64-byte records travel as 16-byte pieces like the obstacle records.  Without
// the bits (every call without `attrs`) nothing of RestartAttrDev is read; its pointers may be null then.
static_assert(sizeof(AgentPar) == RA_PAR_BYTES, "RestartAttrLayout's records");
struct RestartAttrDev {
    AgentPar *ap;                 // [n] DeviceView::ap
    double *ap_nd;                // [n] TrackView::nd_per_agent
    double *trk_R, *trk_plo, *trk_phi;   // [n] TrackView::R_pa / plo_pa / phi_pa
    uint8_t *trk_cls;             // [n] TrackView::cls
};
__device__ __forceinline__ void scene_restart_attrs(const RestartAttrDev &at, const uint8_t *blk, const RestartAttrLayout &AL, uint32_t has, int row0, int lo, int ns, int t) {
    if (has & RESTART_HAS_ATTRS) {
        scene_restart_pieces(at.ap + lo, blk + AL.off[RA_PAR] + RA_PAR_BYTES * row0, (int64_t)ns * (RA_PAR_BYTES / 16), t);
        const double *nd = (const double *)(blk + AL.off[RA_ND]) + row0;
        for (int i = t; i < ns; i += RESTART_T) at.ap_nd[lo + i] = nd[i];
    }
    if (has & RESTART_HAS_PLANNER) {
        const double *trip = (const double *)(blk + AL.off[RA_TRIPLE]) + 3 * (int64_t)row0;
        const uint8_t *cl = blk + AL.off[RA_CLASS] + row0;
        for (int i = t; i < ns; i += RESTART_T) {
            at.trk_R[lo + i] = trip[3 * i]; at.trk_plo[lo + i] = trip[3 * i + 1]; at.trk_phi[lo + i] = trip[3 * i + 2];
            at.trk_cls[lo + i] = cl[i];
        }
    }
}
// A restart that brings waypoint lists (sca_restart_scenes_paths; the context's lists are in slot form, sca_set_path_slots).  With
// RESTART_HAS_PATH_SLOTS every row of the named scene's range gets its cursors: an occupied row len = rem = its list's length and
// now_goal = None (NaN x 3) -- what sca_set_paths leaves --, a vacated row len = rem = 0 and None.  With RESTART_HAS_PATHS the block's
// path sections (RestartPathLayout, sca_scenes.h) hold the CSR offsets over the call's packed rows and the points actually present; the
// scene's points stand together in the block, so consecutive lanes read consecutive coordinates across the link, and each finds its row
// by bisection of the scene's offsets, staged in LDS (a scene holds at most KD_WAVE_CAP rows), and writes to the row's own room
// (path_slot_index).  Without the bit (every entry point without path arrays) the rows get empty lists: the episode brings none.  Room
// behind a list's length keeps what an earlier list left: rem never exceeds len, nobody reads it.  Without RESTART_HAS_PATH_SLOTS (the
// context is not in slot form) nothing of RestartPathDev is read; its pointers are null then.
struct RestartPathDev {
    double *pts;                  // [3 * W * max_agents] PathSlotView::pts
    int32_t *len, *rem;           // [n] PathSlotView::len / rem
    double *now_goal;             // [n * 3]
    int W;
};
__device__ __forceinline__ void scene_restart_paths(const RestartPathDev &p, const uint8_t *blk, const RestartPathLayout &PL, uint32_t has, int row0, int lo, int ns,
                                                    int hi, int t) {
    __shared__ int32_t poff[KD_WAVE_CAP + 1];
    const bool lists = (has & RESTART_HAS_PATHS) != 0;
    if (lists) {
        const int32_t *off = (const int32_t *)(blk + PL.off[RP_OFF]) + row0;
        for (int i = t; i <= ns; i += RESTART_T) poff[i] = off[i];
    }
    __syncthreads();                                                   // (`has` is uniform over the grid: every lane of every workgroup arrives)
    for (int i = t; i < hi - lo; i += RESTART_T) {
        const int32_t k = lists && i < ns ? poff[i + 1] - poff[i] : 0;
        p.len[lo + i] = k; p.rem[lo + i] = k;
    }
    const double none = __builtin_nan("");
    for (int64_t g = 3 * (int64_t)lo + t; g < 3 * (int64_t)hi; g += RESTART_T) p.now_goal[g] = none;
    if (!lists) return;
    const int32_t first = poff[0], count = poff[ns] - first;           // the scene's points: [first, first + count) of the packed section
    const double *src = (const double *)(blk + PL.off[RP_PTS]) + 3 * (int64_t)first;
    for (int w = t; w < 3 * count; w += RESTART_T) {
        const int32_t k = first + w / 3;
        int a = 0, b = ns;                                             // poff[a] <= k < poff[b]
        while (b - a > 1) { const int m = (a + b) >> 1; if (poff[m] <= k) a = m; else b = m; }
        p.pts[3 * (path_slot_index(p.W, lo + a) + (k - poff[a])) + w % 3] = src[w];
    }
}
__global__ __launch_bounds__(RESTART_T) void k_scene_restart(RestartDev d, const uint8_t *blk, RestartLayout L, uint32_t has, const int32_t *new_size, int32_t *size,
                                                             RestartObsDev o, RestartObsLayout OL, RestartAttrDev at, RestartAttrLayout AL,
                                                             RestartPathDev p, RestartPathLayout PL) {
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    const int s = ((const int32_t *)(blk + L.off[RS_IDS]))[b];
    const int row0 = ((const int32_t *)(blk + L.off[RS_START]))[b];
    const int lo = d.offsets[s], hi = d.offsets[s + 1], ns = new_size[b];
    scene_restart_fill(d, blk, L, has, row0, lo, ns, t);
    scene_restart_vacate(d, lo + ns, hi, t);
    if (t == 0) { d.live[s * SCENE_LINE] = ns; d.prev[s] = ns; d.steps[s] = 0; size[s] = ns; }
    if (d.clear)                                                       // the new episode has met nobody yet: the whole capacity, vacant rows too
        for (int a = lo + t; a < hi; a += RESTART_T) d.clear[a] = scene_clearance_empty();
    scene_restart_attrs(at, blk, AL, has, row0, lo, ns, t);
    if (has & RESTART_HAS_PATH_SLOTS) scene_restart_paths(p, blk, PL, has, row0, lo, ns, hi, t);
    const int32_t *head = (const int32_t *)(blk + OL.off[RO_HEAD]) + RO_HEAD_WORDS * b;
    const int k = head[0];
    if (k < 0) return;                                                 // this scene keeps its set (uniform over the workgroup)
    const int64_t base = head[1], st = head[2];
    const int64_t nodes = k > 0 ? 2 * (int64_t)k - 1 : 0;
    scene_restart_pieces(o.obs + base, blk + OL.off[RO_REC] + RO_REC_BYTES * st, k * (RO_REC_BYTES / 16), t);
    scene_restart_pieces(o.obs_sorted + base, blk + OL.off[RO_SORTED] + RO_REC_BYTES * st, k * (RO_REC_BYTES / 16), t);
    const int32_t *perm = (const int32_t *)(blk + OL.off[RO_PERM]) + st;
    for (int i = t; i < k; i += RESTART_T) o.operm[base + i] = perm[i];
    scene_restart_pieces(o.otree + 2 * base, blk + OL.off[RO_TREE] + RO_TREE_BYTES * 2 * st, nodes * (RO_TREE_BYTES / 16), t);
    scene_restart_pieces(o.owide + 2 * base, blk + OL.off[RO_WIDE] + RO_WIDE_BYTES * 2 * st, nodes * (RO_WIDE_BYTES / 16), t);
    if (t == 0) { o.oroot[s] = head[3]; o.ocount[s] = k; }
}

// The wavefront-per-agent forms keep both roots in scalar registers: the obstacle phase is taken or skipped by the whole wavefront (the
// constant 0 of SceneRoots folds away).
template <bool HAS_OBS, class Roots>
__global__ __launch_bounds__(K1_WAVES * 64) void k_neighbors_kd_scenes(DeviceView d, Params P, double agent_reach, double obs_reach,
                                                                       double max_radius, Roots r) {
    SCA_TL(d, TL_NBR_KD);
    __shared__ double rstacks[K1_WAVES][KD_RSTACK][16];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int i = blockIdx.x * K1_WAVES + wid; i < d.shard_count; i += gridDim.x * K1_WAVES) {
        const int agent = d.shard_begin + i;
        neighbors_one<HAS_OBS>(d, P, agent_reach, obs_reach, max_radius, rstacks[wid], agent, lane, __builtin_amdgcn_readfirstlane(r(agent)),
                               __builtin_amdgcn_readfirstlane(r.obstacles(agent)));
    }
}

// four agents per wavefront: a 16-lane group whose scene has no obstacles enters the obstacle phase with nothing to do (the loop keeps its
// shape, see neighbors_kd4_body)
template <bool HAS_OBS, class Roots>
__global__ __launch_bounds__(K1P_WAVES * 64) void k_neighbors_kd4_scenes(DeviceView d, Params P, double agent_reach, double obs_reach,
                                                                        double max_radius, Roots r) {
    SCA_TL(d, TL_NBR_KD);
    SCA_K1_SETPRIO();
    __shared__ int stacks[K1P_WAVES][K1P_APW][KD_STACK];
    neighbors_kd4_body<HAS_OBS>(d, P, agent_reach, obs_reach, max_radius, stacks, r);
}

// The wavefront's K4_APW agents are consecutive ids, so those of one scene are consecutive groups: the first head lane of every run of
// equal scenes adds the run's live agents to the scene's line in one atomic.
// A FINISHED scene stays what its last step left.  The reference stops calling env.step() for it; here its agents, all flagged, still pass
// through update_velocitie with a zero action row like the done agents of a live scene (mampenv.py:42-49: velocity zeroed, step_num
// advanced unless at the goal, heading through pi_2_pi once more, and a timed-out agent may still gain the collision flag).  So for a scene
// that had nobody live when the step began, the head lane takes all of that back: the old record whole, step_num, and the heading kept
// from the last step the scene was live in.
struct SceneCount {
    const DeviceView &d;
    const SceneView &v;
    __device__ __forceinline__ void operator()(bool head, bool live, int agent) const {
        const int lane = threadIdx.x & 63;
        const int sc = head ? v.scene_of[agent] : -1;
        if (head) {
            if (v.prev[sc] == 0) {
                const PubRec old = d.rec[agent];
                d.rec_new[agent] = old;
                if (!(old.flags & FLAG_AT_GOAL)) d.step_num[agent] -= 1;
                for (int k = 0; k < 3; k++) d.heading[agent * 3 + k] = v.heading_keep[agent * 3 + k];
            } else {
                for (int k = 0; k < 3; k++) v.heading_keep[agent * 3 + k] = d.heading[agent * 3 + k];
            }
        }
        int mine = 0;
        bool first = head;
#pragma unroll
        for (int g = 0; g < K4_APW; g++) {
            const int sg = __shfl(sc, g * NEAR_MAX);
            const int lg = __shfl((int)live, g * NEAR_MAX);
            if (sg == sc) { mine += lg; if (g * NEAR_MAX < lane) first = false; }
        }
        if (first && mine > 0) atomicAdd(&v.live[sc * SCENE_LINE], mine);
    }
};
template <class Roots>
__global__ __launch_bounds__(K4_WAVES * 64) void k_collide_finish_scenes(DeviceView d, Params P, double agent_reach, double obs_reach,
                                                                       int check_arrived, Roots r) {
    SCA_TL(d, TL_COLLIDE);
    __shared__ int stacks[K4_WAVES][KD_STACK];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    collide_finish_body(d, P, check_arrived, [&](int ag, bool obs_only) {
        int st = 0;
        const bool hit = collide_traverse(d, agent_reach, obs_reach, stacks[wid], ag, lane, obs_only, st, __builtin_amdgcn_readfirstlane(r(ag)),
                                          __builtin_amdgcn_readfirstlane(r.obstacles(ag)));
        collide_flag_walk(d, ag, lane, st);
        return hit;
    }, SceneCount{d, r.v});
}

// ---- a trajectory log per scene (sca_scene_history_enable; the layout and its index are sca_scenes.h's) -------------------------------------
// Enqueued in front of k_collide_finish_scenes, the one place every step form passes through: d.rec_new holds the moved records with the
// flags the agents entered the step with, d.heading the integrated angles, prev / steps are final for the step -- the fields integrate_agent
// puts into a HistRow of the context-wide log.  A scene that had nobody live when the step began writes nothing (the reference stopped
// calling env.step() for it), nor does a step beyond the capacity; either way no other scene's rows are touched.
// Four lanes per row, one 16-byte quarter each: a wavefront's store covers 1 KB of consecutive bytes while its 16 agents are of one scene
// (agents of a scene are consecutive in a row of the log).
static_assert(sizeof(HistRow) == SCENE_LOG_ROW_BYTES, "the scene log's rows are HistRow");
struct SceneLogView {
    HistRow *rows;            // [capacity * n]
    int capacity;             // rows per scene
};
typedef double __attribute__((ext_vector_type(2), may_alias)) scene_log_quarter;
constexpr int SCENE_LOG_T = 256;
__global__ __launch_bounds__(SCENE_LOG_T) void k_scene_log(DeviceView d, SceneView v, SceneLogView L) {
    const int t = blockIdx.x * SCENE_LOG_T + threadIdx.x;
    const int agent = t >> 2, q = t & 3;
    if (agent >= d.n) return;
    const int s = v.scene_of[agent];
    if (v.prev[s] == 0) return;
    const int row = v.steps[s] - 1;
    if (row < 0 || row >= L.capacity) return;
    const int lo = v.offsets[s];
    const PubRec *r = d.rec_new + agent;
    scene_log_quarter w;
    if (q == 0) { w.x = r->px; w.y = r->py; }                                      // HistRow: px py | pz a | b g | vx vy vz flags
    else if (q == 1) { w.x = r->pz; w.y = d.heading[agent * 3 + 0]; }
    else if (q == 2) { w.x = d.heading[agent * 3 + 1]; w.y = d.heading[agent * 3 + 2]; }
    else __builtin_memcpy(&w, &r->vx, 16);                                         // vx vy vz flags stand in PubRec as they do in HistRow
    reinterpret_cast<scene_log_quarter *>(L.rows + scene_log_index(L.capacity, lo, v.offsets[s + 1] - lo, row, agent - lo))[q] = w;
}

// ---- closest approach per agent, measured with the step (sca_scene_clearance_enable; the rule and clearance_pair are sca_scenes.h's) ---------
// Enqueued beside k_scene_log, in front of k_collide_finish_scenes: d.rec_new holds the moved records, prev / steps are final for the step.
// The flags an agent ENTERED the step with are the moved record's minus one case: the epilogue of this step's policy pass has already put
// a collision found by the neighbour insertion into the record (action_one, agent.py:84), and K1 sets coll_new[a] for exactly those agents
// -- unflagged at entry -- and clears it for everybody it skipped.  So an agent entered unfinished where its record has no flag or
// coll_new[a] is set; coll_new is null for an env update without a policy pass, which changes no flag before this kernel.
// One workgroup per scene; a scene that had nobody live when the step began returns at
// once.  The occupied rows' positions and radii are staged in LDS (ClearPoint, 32 bytes a row: at most KD_WAVE_CAP x 32 B = 48 KB; the
// launch asks for the largest scene's room, not the cap's), the scene's obstacles stream through a tile of CLEAR_OBS_TILE behind them.
// Every lane owns WHOLE agent rows -- row t, t + T, ... -- and walks all partners in ascending order, every lane of a wavefront reading the
// same LDS word (a broadcast): the record lives in the lane's registers for the step and goes back as the lane's own two 16-byte vector
// stores.  No atomics, no reduction across lanes, no order that depends on scheduling.  A scene of more rows than the workgroup has lanes
// takes several passes and streams its obstacles once per pass.
// Obstacles: o == null is the shared set (rows 0 .. shared_m - 1 of d.obs, set order); else the scene's own rows of the forest's d.obs,
// from oroot[s] / 2 (the root record of its tree is 2 x its first row), o[nscenes + s] of them -- a slot's count, never its capacity.
constexpr int CLEAR_OBS_TILE = 128;
static_assert(CLEAR_DONE_FLAGS == (FLAG_AT_GOAL | FLAG_COLLISION | FLAG_TIMEOUT), "the flags that finish an agent");
inline int clearance_lds_bytes(int largest) { return (int)sizeof(ClearPoint) * (largest + CLEAR_OBS_TILE); }
__global__ __launch_bounds__(256) void k_scene_clearance(DeviceView d, SceneView v, const int32_t *size, sca_scene_clearance *rec, const int32_t *o, int shared_m,
                                                         int agent_room, const uint32_t *coll_new) {
    extern __shared__ ClearPoint clear_lds[];
    const int s = (int)blockIdx.x, t = (int)threadIdx.x, T = (int)blockDim.x;
    if (v.prev[s] == 0) return;                                        // (uniform over the workgroup)
    const int lo = v.offsets[s], ns = min(size[s], agent_room), step = v.steps[s];
    ClearPoint *ag = clear_lds, *ob = clear_lds + agent_room;
    for (int i = t; i < ns; i += T) {
        const PubRec *r = d.rec_new + lo + i;
        ClearPoint p; p.x = r->px; p.y = r->py; p.z = r->pz; p.r = r->radius;
        ag[i] = p;
    }
    const int ocount = o ? o[v.nscenes + s] : shared_m;
    const ObsRec *obs = d.obs + (o && ocount > 0 ? o[s] >> 1 : 0);
    __syncthreads();
    for (int i0 = 0; i0 < ns; i0 += T) {                               // (uniform trip counts: every lane reaches every barrier)
        const int i = i0 + t;
        const bool mine = i < ns && (!(d.rec_new[lo + i].flags & CLEAR_DONE_FLAGS) || (coll_new && coll_new[lo + i]));
        sca_scene_clearance c = scene_clearance_empty();
        ClearPoint pa = {0.0, 0.0, 0.0, 0.0};
        if (mine) {
            c = rec[lo + i];
            pa = ag[i];
            for (int b = 0; b < ns; b++)
                if (b != i) clearance_pair(pa, ag[b], b, step, c.agent_clear, c.agent_partner, c.agent_step, L3Norm{});
        }
        for (int j0 = 0; j0 < ocount; j0 += CLEAR_OBS_TILE) {
            const int nj = min(CLEAR_OBS_TILE, ocount - j0);
            __syncthreads();                                           // the tile before has been read by everybody
            for (int j = t; j < nj; j += T) {
                const ObsRec q = obs[j0 + j];
                ClearPoint p; p.x = q.px; p.y = q.py; p.z = q.pz; p.r = q.radius;
                ob[j] = p;
            }
            __syncthreads();
            if (mine)
                for (int j = 0; j < nj; j++) clearance_pair(pa, ob[j], j0 + j, step, c.obs_clear, c.obs_partner, c.obs_step, L3Norm{});
        }
        if (mine) rec[lo + i] = c;
    }
}

// ---- finished scenes hand over their result with the step (sca_scene_harvest_enable; the block's layout is sca_scenes.h's) -------------------
// Enqueued BEHIND k_collide_finish_scenes, the last kernel of a step in every step form: live[s] is the step's final count, prev[s] what the
// step found, and the records K4 wrote (`rec`: the buffer the host swaps in behind this launch) carry the final flags.  One workgroup per
// scene.  Its counters go into the block on every step; everything else only in the one step per episode the scene finishes in -- a
// finished scene has prev == 0 on every later step until a restart makes it live again -- so the block's rows and summary of a scene are
// written at most once between two restarts.  Rows behind size[s] (vacant, sca_restart_scenes_sized) are never touched, nor is anything of
// another scene: the flag bytes of a scene that does not begin or end on a 4-byte boundary are written as bytes at its edges.
// The block is host memory: every section is written as consecutive 4-byte words (16 flag bytes per lane in the interior) by consecutive
// lanes, as k_host_egress writes the host state block.
struct HarvestDev {
    const PubRec *rec;        // [n] the records this step's K4 wrote
    const double *heading;    // [n*3]
    const double *total_dist; // [n]
    const int32_t *step_num;  // [n]
    const int32_t *size;      // [nscenes] the rows each scene occupies (k_kd_scene_jobs' array)
    uint8_t *blk;             // the page-locked block
    HarvestLayout L;
    int32_t batch_step;       // the context's env updates since the harvest was enabled, this one included
};
typedef uint32_t __attribute__((may_alias)) harvest_u32;
constexpr int HARVEST_T = 256;
__global__ __launch_bounds__(HARVEST_T) void k_scene_harvest(SceneView v, HarvestDev h) {
    const int s = (int)blockIdx.x, t = (int)threadIdx.x;
    const int live = v.live[s * SCENE_LINE], steps = v.steps[s];
    if (t < 2) ((int32_t *)(h.blk + h.L.off[HV_COUNTERS]))[2 * s + t] = t == 0 ? live : steps;
    if (!(v.prev[s] > 0 && live == 0)) return;                              // (uniform over the workgroup)
    const int lo = v.offsets[s], ns = h.size[s];
    const harvest_u32 *rec = (const harvest_u32 *)(h.rec + lo);             // 12 words per record: px py pz (0-5), vx vy vz (6-8), flags (9)
    constexpr int RW = (int)(sizeof(PubRec) / 4);
    static_assert(sizeof(PubRec) == 48, "k_scene_harvest reads the records as 12 words");
    harvest_u32 *pos = (harvest_u32 *)(h.blk + h.L.off[HV_POS]) + 6 * (int64_t)lo;
    for (int w = t; w < 6 * ns; w += HARVEST_T) pos[w] = rec[(w / 6) * RW + w % 6];
    harvest_u32 *vel = (harvest_u32 *)(h.blk + h.L.off[HV_VEL]) + 3 * (int64_t)lo;
    for (int w = t; w < 3 * ns; w += HARVEST_T) vel[w] = rec[(w / 3) * RW + 6 + w % 3];
    harvest_u32 *head = (harvest_u32 *)(h.blk + h.L.off[HV_HEADING]) + 6 * (int64_t)lo;
    const harvest_u32 *head_in = (const harvest_u32 *)(h.heading + 3 * (int64_t)lo);
    for (int w = t; w < 6 * ns; w += HARVEST_T) head[w] = head_in[w];
    harvest_u32 *td = (harvest_u32 *)(h.blk + h.L.off[HV_TOTAL_DIST]) + 2 * (int64_t)lo;
    const harvest_u32 *td_in = (const harvest_u32 *)(h.total_dist + lo);
    for (int w = t; w < 2 * ns; w += HARVEST_T) td[w] = td_in[w];
    int32_t *sn = (int32_t *)(h.blk + h.L.off[HV_STEP_NUM]) + lo;
    for (int i = t; i < ns; i += HARVEST_T) sn[i] = h.step_num[lo + i];
    // flags, (uint8_t)rec.flags as sca_get_state gives them: bytes up to the first 4-byte boundary of the section, words, bytes behind the last
    uint8_t *fl = h.blk + h.L.off[HV_FLAGS] + lo;
    const int head_bytes = min(ns, (4 - (lo & 3)) & 3), words = (ns - head_bytes) / 4;
    for (int w = t; w < words; w += HARVEST_T) {
        uint32_t x = 0;
        for (int b = 0; b < 4; b++) x |= (rec[(head_bytes + 4 * w + b) * RW + 9] & 0xffu) << (8 * b);
        ((harvest_u32 *)(fl + head_bytes))[w] = x;
    }
    for (int i = t; i < ns - 4 * words; i += HARVEST_T) {
        const int a = i < head_bytes ? i : 4 * words + i;
        fl[a] = (uint8_t)rec[a * RW + 9];
    }
    // the summary: counts and the integer sum through LDS, the distance by one lane in ascending row order (metrics.episode_metrics adds
    // Python floats in that order, and the sum of doubles depends on it)
    __shared__ int cnt[4];
    __shared__ unsigned long long step_sum;
    if (t < 4) cnt[t] = 0;
    if (t == 0) step_sum = 0ull;
    __syncthreads();
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    long long st = 0;
    for (int i = t; i < ns; i += HARVEST_T) {
        const uint32_t f = rec[i * RW + 9];
        c0 += (f & FLAG_AT_GOAL) ? 1 : 0; c1 += (f & FLAG_COLLISION) ? 1 : 0; c2 += (f & FLAG_TIMEOUT) ? 1 : 0;
        if (!(f & (FLAG_COLLISION | FLAG_TIMEOUT))) { c3 += 1; st += h.step_num[lo + i]; }
    }
    if (c0) atomicAdd(&cnt[0], c0);
    if (c1) atomicAdd(&cnt[1], c1);
    if (c2) atomicAdd(&cnt[2], c2);
    if (c3) { atomicAdd(&cnt[3], c3); atomicAdd(&step_sum, (unsigned long long)st); }
    __syncthreads();
    if (t != 0) return;
    double dist = 0.0;
    for (int i = 0; i < ns; i++)
        if (!(rec[i * RW + 9] & (FLAG_COLLISION | FLAG_TIMEOUT))) dist += h.total_dist[lo + i];
    sca_scene_summary r;
    r.fresh = 1; r.steps = steps; r.batch_step = h.batch_step;
    r.arrived = cnt[0]; r.collided = cnt[1]; r.timed_out = cnt[2]; r.successful_num = cnt[3]; r.reserved0 = 0;
    r.all_step_num = (int64_t)step_sum; r.all_distance = dist; r.reserved1[0] = 0; r.reserved1[1] = 0;
    ((sca_scene_summary *)(h.blk + h.L.off[HV_SUMMARY]))[s] = r;
}


// ---- scene checkpoints (sca_save_scenes / sca_load_scenes; the blob's layout and its check are sca_scenes.h's) -----------------------------------
// One workgroup per named scene, between two steps.  k_scene_save gathers the scene's occupied rows into the library's page-locked block
// (CkptEntry table in front, the blobs behind it), k_scene_load scatters a blob the host has CHECKED (scene_checkpoint_check: sizes,
// permutation, cursors and tracker integers are in range before this kernel sees them) back into the rows at offsets[s].  The block is host
// memory: every section travels as consecutive 4-byte words -- the records as 16-byte pieces -- by consecutive lanes, as k_scene_harvest
// and k_host_egress write theirs.  The permutation is stored in scene-local terms and rebased on the way in; the kd-tree, the neighbour
// lists, action rows, diag and vpref_used are not state: the next pass rebuilds them from what is here before it reads them.
// Nothing outside the named scenes' occupied rows and counters is written; the only shared words are K4's striped done_count, adjusted
// for the rows whose done-ness changes by the rule scene_restart_fill / scene_restart_vacate have.  No other atomics.
struct CkptDev {
    PubRec *rec;
    double *heading, *heading_keep, *vpref_ext, *total_dist;
    int32_t *step_num, *status, *aperm;
    uint8_t *vpref_mode;
    int32_t *done_count;
    const int32_t *offsets;
    int32_t *live, *prev, *steps;
    double *trk_nbr0;               // the device tracker's, null without one
    restart_u32 *trk_st;
    int32_t *rem;                   // the waypoint cursors, null without lists
    double *now_goal;
};
static_assert(sizeof(PubRec) == CKPT_REC_BYTES, "CkptLayout's records");
constexpr int CKPT_T = RESTART_T;
constexpr int CKPT_HEAD_STEPS = 8;  // CkptHeader::steps, live, prev as words of the header
__device__ __forceinline__ void ckpt_words(void *dst, const void *src, int64_t words, int t) {
    restart_u32 *to = (restart_u32 *)dst;
    const restart_u32 *from = (const restart_u32 *)src;
    for (int64_t w = t; w < words; w += CKPT_T) to[w] = from[w];
}
__global__ __launch_bounds__(CKPT_T) void k_scene_save(CkptDev d, uint8_t *blk) {
    const int t = (int)threadIdx.x;
    const CkptEntry e = ((const CkptEntry *)blk)[blockIdx.x];
    const int s = e.scene, N = e.size, tw = e.trk_words;
    const int64_t lo = d.offsets[s];
    const CkptLayout L = scene_checkpoint_layout(N, tw, e.has_paths);
    uint8_t *o = blk + e.at;
    scene_restart_pieces(o + L.off[CK_REC], d.rec + lo, (int64_t)N * (CKPT_REC_BYTES / 16), t);
    ckpt_words(o + L.off[CK_HEADING], d.heading + 3 * lo, 6 * (int64_t)N, t);
    ckpt_words(o + L.off[CK_HEADING_KEEP], d.heading_keep + 3 * lo, 6 * (int64_t)N, t);
    ckpt_words(o + L.off[CK_VPREF_EXT], d.vpref_ext + 3 * lo, 6 * (int64_t)N, t);
    ckpt_words(o + L.off[CK_TOTAL_DIST], d.total_dist + lo, 2 * (int64_t)N, t);
    ckpt_words(o + L.off[CK_STEP_NUM], d.step_num + lo, N, t);
    ckpt_words(o + L.off[CK_STATUS], d.status + lo, N, t);
    int32_t *perm = (int32_t *)(o + L.off[CK_PERM]);
    restart_u32 *mode = (restart_u32 *)(o + L.off[CK_VPREF_MODE]);
    for (int i = t; i < N; i += CKPT_T) { perm[i] = d.aperm[lo + i] - (int32_t)lo; mode[i] = d.vpref_mode[lo + i]; }
    if (tw > 0) {
        ckpt_words(o + L.off[CK_TRK_NBR0], d.trk_nbr0 + lo, 2 * (int64_t)N, t);
        ckpt_words(o + L.off[CK_TRACK], d.trk_st + lo * tw, (int64_t)N * tw, t);
    }
    if (e.has_paths) {
        ckpt_words(o + L.off[CK_REM], d.rem + lo, N, t);
        ckpt_words(o + L.off[CK_NOW_GOAL], d.now_goal + 3 * lo, 6 * (int64_t)N, t);
    }
    if (t < 3) ((int32_t *)o)[CKPT_HEAD_STEPS + t] = t == 0 ? d.steps[s] : t == 1 ? d.live[s * SCENE_LINE] : d.prev[s];
}
__global__ __launch_bounds__(CKPT_T) void k_scene_load(CkptDev d, const uint8_t *blk) {
    const int t = (int)threadIdx.x;
    const CkptEntry e = ((const CkptEntry *)blk)[blockIdx.x];
    const int s = e.scene, N = e.size, tw = e.trk_words;
    const int64_t lo = d.offsets[s];
    const CkptLayout L = scene_checkpoint_layout(N, tw, e.has_paths);
    const uint8_t *in = blk + e.at;
    // K4's counters of the last step, before the records are replaced: a row that was done and runs again counts, a row that ran and is done no longer does
    const restart_u32 *rec_in = (const restart_u32 *)(in + L.off[CK_REC]);
    constexpr int RW = CKPT_REC_BYTES / 4;
    constexpr uint32_t DONE = FLAG_AT_GOAL | FLAG_COLLISION | FLAG_TIMEOUT;
    for (int i = t; i < N; i += CKPT_T) {
        const bool was = (d.rec[lo + i].flags & DONE) != 0, is = (rec_in[i * RW + 9] & DONE) != 0;
        if (was != is) atomicAdd(&d.done_count[((lo + i) & 255) * 32], was ? 1 : -1);
    }
    __syncthreads();
    scene_restart_pieces(d.rec + lo, in + L.off[CK_REC], (int64_t)N * (CKPT_REC_BYTES / 16), t);
    ckpt_words(d.heading + 3 * lo, in + L.off[CK_HEADING], 6 * (int64_t)N, t);
    ckpt_words(d.heading_keep + 3 * lo, in + L.off[CK_HEADING_KEEP], 6 * (int64_t)N, t);
    ckpt_words(d.vpref_ext + 3 * lo, in + L.off[CK_VPREF_EXT], 6 * (int64_t)N, t);
    ckpt_words(d.total_dist + lo, in + L.off[CK_TOTAL_DIST], 2 * (int64_t)N, t);
    ckpt_words(d.step_num + lo, in + L.off[CK_STEP_NUM], N, t);
    ckpt_words(d.status + lo, in + L.off[CK_STATUS], N, t);
    const int32_t *perm = (const int32_t *)(in + L.off[CK_PERM]);
    const restart_u32 *mode = (const restart_u32 *)(in + L.off[CK_VPREF_MODE]);
    for (int i = t; i < N; i += CKPT_T) { d.aperm[lo + i] = (int32_t)lo + perm[i]; d.vpref_mode[lo + i] = (uint8_t)mode[i]; }
    if (tw > 0) {
        ckpt_words(d.trk_nbr0 + lo, in + L.off[CK_TRK_NBR0], 2 * (int64_t)N, t);
        ckpt_words(d.trk_st + lo * tw, in + L.off[CK_TRACK], (int64_t)N * tw, t);
    }
    if (e.has_paths && d.rem) {
        ckpt_words(d.rem + lo, in + L.off[CK_REM], N, t);
        ckpt_words(d.now_goal + 3 * lo, in + L.off[CK_NOW_GOAL], 6 * (int64_t)N, t);
    }
    if (t == 0) {
        const int32_t *head = (const int32_t *)in + CKPT_HEAD_STEPS;
        d.steps[s] = head[0]; d.live[s * SCENE_LINE] = head[1]; d.prev[s] = head[2];
    }
}

}  // namespace sca
