// sca_hip.hip -- host side of libsca_hip.so: context, HBM layout, launches, C-ABI (include/sca_hip.h).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>          // types and prototypes only: the library is loaded with dlopen when sca_comm_init is called
#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/sca_hip.h"
#include "sca_kernels.hip.h"
#include "sca_kdbuild.hip.h"
#include "sca_grid.hip.h"
#include "sca_dubins.hpp"
#include "sca_tracker.hip.h"
#include "sca_partition.hip.h"
#include "sca_hostio.hip.h"
#include "sca_forms.h"
#include "sca_scenes.h"
#include "sca_scene_restart.h"
#include "sca_scenes.hip.h"
#include "sca_clearance.h"
#include "sca_clearance.hip.h"
#include "sca_respawn.h"
#include "sca_respawn.hip.h"
#include "sca_vacancy.h"
#include "sca_vacancy.hip.h"
#include "sca_missions.h"
#include "sca_missions.hip.h"
#include "sca_mission_gate.hip.h"
#include "sca_spawn.h"
#include "sca_spawn.hip.h"
#include "sca_checkpoint.h"
#include "sca_checkpoint.hip.h"

using namespace sca;

namespace {

// grid cap for the wave-per-agent kernels (they grid-stride): 256 CUs x 8 workgroups
constexpr int MAX_GRID = 1 << 30;      // one agent per wavefront: measured faster than grid-striding (k_solve keeps 2 waves/SIMD)

// libm calls that must not be folded by the compiler (the candidate table follows the reference's
// Python expression literally: z ** 2 is pow(z, 2), not z * z)
double (*volatile p_pow)(double, double) = std::pow;
double (*volatile p_acos)(double) = std::acos;

// Replica of KDTree.buildAgentTreeRecursive / buildObstacleTreeRecursive (kdTree.py:60-122,162-227),
// iterative with an explicit work list.  Children live at node+1 and node+2*leftSize.
void kd_build_host(int n, const double *pos, int32_t *ids, std::vector<KdNode> &tree) {
    tree.assign(n > 0 ? (size_t)(2 * n) : 1, KdNode{});
    if (n <= 0) return;
    struct Job { int begin, end, node; };
    std::vector<Job> work;
    work.push_back({0, n, 0});
    while (!work.empty()) {
        const Job jb = work.back();
        work.pop_back();
        KdNode &nd = tree[jb.node];
        nd.begin = jb.begin; nd.end = jb.end; nd.left = 0; nd.right = 0;
        for (int k = 0; k < 3; k++) nd.mn[k] = nd.mx[k] = pos[3 * ids[jb.begin] + k];
        for (int i = jb.begin + 1; i < jb.end; i++)
            for (int k = 0; k < 3; k++) {
                const double v = pos[3 * ids[i] + k];
                if (v > nd.mx[k]) nd.mx[k] = v;
                if (v < nd.mn[k]) nd.mn[k] = v;
            }
        if (jb.end - jb.begin > MAX_LEAF) {
            const double d0 = nd.mx[0] - nd.mn[0], d1 = nd.mx[1] - nd.mn[1], d2 = nd.mx[2] - nd.mn[2];
            const int c = (d0 > d1 && d0 > d2) ? 0 : (d1 > d2 ? 1 : 2);
            const double split = 0.5 * (nd.mx[c] + nd.mn[c]);
            int lo = jb.begin, hi = jb.end;
            while (lo < hi) {
                while (lo < hi && pos[3 * ids[lo] + c] < split) lo++;
                while (hi > lo && pos[3 * ids[hi - 1] + c] >= split) hi--;
                if (lo < hi) { std::swap(ids[lo], ids[hi - 1]); lo++; hi--; }
            }
            int leftSize = lo - jb.begin;
            if (leftSize == 0) { leftSize = 1; lo++; }
            nd.left = jb.node + 1;
            nd.right = jb.node + 2 * leftSize;
            // order of construction does not matter: the two sub-ranges are disjoint
            work.push_back({lo, jb.end, nd.right});
            work.push_back({jb.begin, lo, nd.left});
        }
    }
}

// query view of a host-built tree: node headers + both children's boxes (KdWide)
void kd_widen_host(int n, const std::vector<KdNode> &tree, std::vector<KdWide> &wide) {
    wide.assign(n > 0 ? (size_t)(2 * n) : 1, KdWide{});
    if (n <= 0) return;
    std::vector<int> st{0};
    while (!st.empty()) {
        const int i = st.back();
        st.pop_back();
        const KdNode &nd = tree[i];
        KdWide &w = wide[i];
        w.begin = nd.begin; w.end = nd.end; w.left = nd.left; w.right = nd.right;
        if (nd.end - nd.begin > MAX_LEAF) {
            for (int k = 0; k < 3; k++) {
                w.bx[kdw_idx(0, 0, k)] = tree[nd.left].mn[k]; w.bx[kdw_idx(0, 1, k)] = tree[nd.left].mx[k];
                w.bx[kdw_idx(1, 0, k)] = tree[nd.right].mn[k]; w.bx[kdw_idx(1, 1, k)] = tree[nd.right].mx[k];
            }
            st.push_back(nd.left); st.push_back(nd.right);
        }
    }
}

void candidate_table_host(int num_N, double *unit, double *phi) {
    const double param_phi = (std::sqrt(5.0) - 1.0) / 2.0;                         // scaPolicy.py:191
    for (int n = 1; n <= num_N; n++) {
        const double z_n = (double)(2 * n - 1) / num_N - 1;                        // :197
        const double c = std::sqrt(1 - p_pow(z_n, 2.0));
        const double ang = 2 * M_PI * n * param_phi;
        const double x_n = c * std::cos(ang), y_n = c * std::sin(ang);             // :198-199
        unit[n - 1] = x_n; unit[num_N + n - 1] = y_n; unit[2 * num_N + n - 1] = z_n;
        // get_phi (util.py:145) of the direction; rad in {0.5, 1.0} scales both atan2 arguments exactly
        double ph = (y_n >= 0) ? std::atan2(y_n, x_n) : 2 * M_PI + std::atan2(y_n, x_n);
        double t = std::trunc(ph * EPS5);
        if (t == 0.0) t = 0.0;
        phi[n - 1] = t;
    }
}

// smallest double c with acos(c) <= mhc under the host libm: `theta <= max_heading_change` (util.py:16-17)
// becomes `costheta >= thr` exactly (acos is monotone).
double cos_threshold(double mhc) {
    if (p_acos(-1.0) <= mhc) return -1.0;
    if (!(p_acos(1.0) <= mhc)) return 2.0;      // nothing satisfies
    double lo = -1.0, hi = 1.0;                 // acos(lo) > mhc, acos(hi) <= mhc
    while (std::nextafter(lo, 2.0) < hi) {
        const double mid = lo + (hi - lo) * 0.5;
        if (mid <= lo || mid >= hi) break;
        if (p_acos(mid) <= mhc) hi = mid; else lo = mid;
    }
    return hi;
}

}  // namespace

// RCCL entry points, resolved at run time (a box without RCCL still loads libsca_hip.so; single-GPU use never touches it)
struct RcclApi {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
static RcclApi g_rccl;
static const char *rccl_load() {
    if (g_rccl.handle) return nullptr;
    void *h = nullptr;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { h = dlopen(name, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
    if (!h) return "librccl.so not found (dlopen)";
    RcclApi a;
    a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    a.CommInitRank = (decltype(a.CommInitRank))dlsym(h, "ncclCommInitRank");
    a.CommDestroy = (decltype(a.CommDestroy))dlsym(h, "ncclCommDestroy");
    a.AllGather = (decltype(a.AllGather))dlsym(h, "ncclAllGather");
    a.GetErrorString = (decltype(a.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.AllGather || !a.GetErrorString) return "librccl.so lacks an expected symbol";
    a.handle = h;
    g_rccl = a;
    return nullptr;
}

struct sca_ctx {
    int device = 0;
    int max_n = 0, max_m = 0, n = 0, m = 0;
    Params P{};
    DeviceView d{};
    PubRec *rec_own = nullptr, *rec_new_own = nullptr;
    hipStream_t stream_own = nullptr, stream = nullptr;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // policy pass: 0..3, env update: 4, 5
    float ms_nbr = 0, ms_solve = 0, ms_update = 0;
    // per-launch profiling of sca_run_steps: event pairs around every k_neighbors_kd / k_solve launch
    bool profiling = false;
    std::vector<hipEvent_t> pool;       // 4 events per profiled pass: around K1 (on its stream), around k_solve
    int pool_used = 0;
    std::vector<hipEvent_t> pool_kd;    // 2 events around every 16th kd build while profiling (sca_last_kd_build_ms)
    int pool_kd_used = 0;
    float ms_kd_build = 0.0f;
    std::vector<hipEvent_t> pool_xch;   // 2 events per profiled step around the in-library ncclAllGather (sca_last_exchange_ms)
    int pool_xch_used = 0;
    float ms_exchange = 0.0f;
    std::vector<hipEvent_t> pool_trk;   // 2 events per step on the stream the re-plan kernels run on: before / after them
    int pool_trk_used = 0;
    float ms_replan = 0;
    // K3: the ORCA3D-LP agents, ascending ids (static: sca_set_agents), solved one lane per agent by k_lp
    int32_t *lp_list = nullptr;
    std::vector<int32_t> h_lp_list;
    bool shard_emulation = false;       // measurement aid: a partial shard without a communicator, the others stand still
    std::vector<double> h_pos;          // host mirror of positions for the kd build
    bool h_pos_valid = false;
    std::vector<int32_t> h_perm;
    std::vector<KdNode> h_tree;
    std::vector<PubRec> h_rec;
    KdScratch kd{};
    GridDev grid{};                     // SCA_NBR_GRID (sca_grid.hip.h)
    int nbr_mode = SCA_NBR_KDTREE;      // neighbour structure of the last policy pass: K4's fallback looks there
    // depth of the large-node part of the tree, read back asynchronously (never waited for) to size the next build
    int *kd_host_counts = nullptr;      // pinned
    hipEvent_t kd_ev = nullptr;
    bool kd_ev_pending = false;
    unsigned kd_builds = 0;             // device builds so far: the level statistics are read back every 8th
    unsigned kd_gen = 0, kd_ev_gen = 0; // positions replaced from outside (sca_set_state ...): statistics of older trees do not apply
    int kd_single_hint = 0;             // 1 + first level whose nodes all fit one chunk in an earlier build (0: unknown)
    unsigned kd_token = 0;              // launch token of the chained scan (never reused)
    bool perm_on_device = false;        // the live agentIDs permutation is d.aperm (device build) rather than h_perm
    bool agents_set = false, state_set = false;
    bool state_fresh = false;           // flags came from sca_set_state: the next env update checks arrived agents against obstacles once
    bool near_valid = false;            // K1's collision-candidate lists describe the current records
    sca_scene_clearance *clear = nullptr;   // [n] the closest-approach records of the whole context (sca_clearance_enable), null: off -- a step then enqueues nothing for them
    int32_t clear_step = 0;             // env updates enqueued since the enable call: k_clearance's step number
    double max_radius = 0, max_obs_radius = 0, max_pref_speed = 0;
    std::string err;
    double *tab = nullptr;
    // device-side v_pref tracker (sca_tracker.hip.h)
    TrackDev trk{};
    sca_dubins::TrackView trk_view{};
    double *trk_goal_heading = nullptr;
    bool trk_on = false, trk_in_pass = false;
    // the re-plans run on a stream of their own, next to the kd build and the neighbour query of the same pass
    hipStream_t trk_stream = nullptr;   // round 2: the re-plans are the critical path and stay on the main stream; the neighbour
                                        // structure (K0) and the neighbour query (K1) of the pass run on this one beside them
    hipEvent_t trk_fork = nullptr, trk_join = nullptr;
    hipStream_t nbr_stream = nullptr;   // where K0 / K1 of the current pass go: trk_stream when overlapped, else the main stream
    Params P_ctx{};                     // sca_create's parameters; P holds the ENVELOPE of the agents' own while sca_set_agent_params is in force
    AgentPar *ap_dev = nullptr;         // [n] per-agent solver attributes on the device (DeviceView::ap), null: one value per context
    double *ap_nd = nullptr;            // [n] the agents' neighborDist alone, for the tracker (TrackView::nd_per_agent)
    int32_t *h_done = nullptr;          // pinned: K4's 256 counters (stride 32) + the kd build's error word (read_active)
    std::vector<std::array<double, 3>> trk_classes;   // (turning radius, pitch_lo, pitch_hi) of every class of tracked agents; empty: one class = the view's scalars
    double *trk_R_pa = nullptr;         // [n] agent.turning_radius (device), for the decision
    uint8_t *trk_cls = nullptr;         // [n] the agent's class (device)
    double *trk_plo_pa = nullptr, *trk_phi_pa = nullptr;   // [n] agent.pitchlims (device): the per-agent form (more than TRK_MAX_CLASSES classes)
    bool trk_many = false;              // the per-agent form: every re-plan by a wavefront of its own, which reads ITS agent's three values
    double trk_enable_vals[3] = {1.5, 0, 0};   // (turning radius, pitch_lo, pitch_hi) of sca_device_tracker_enable: what "back to one value" restores
    int *trk_host_count = nullptr;      // pinned: the re-plan count of an earlier pass, copied back without ever being waited for
    hipEvent_t trk_count_ev = nullptr;
    bool trk_count_pending = false;
    int trk_last_count = -1;            // -1: unknown
    unsigned trk_passes = 0;
    int forms = 0;                      // SCA_FORM_* of the last policy pass
    // cell-owner partition of SCA_NBR_GRID (sca_partition.hip.h)
    PartDev part{};
    bool part_on = false;
    int part_rank = 0, part_nranks = 1;
    int part_counts[8] = {0};            // [0] owned, [1] halo: UPPER BOUNDS the launches are sized with (the kernels read the exact
                                        // counts on the device); [4] error bits as last seen
    int *part_host = nullptr;            // pinned: the counts of an earlier commit, copied back without being waited for
    hipEvent_t part_ev = nullptr;
    bool part_pending = false;
    int part_known[2] = {0, 0};          // the last exact counts the host has seen, and how many commits ago
    int part_age = 0, part_copy_age = 0;
    uint8_t *part_scratch[2] = {nullptr, nullptr};   // outgoing messages of a rank that runs alone (sca_run_steps: one rank, or emulation)
    int cus = 256, simds = 1024;         // the device's compute units / SIMDs (hipDeviceProp)
    Tunables tun{};                     // every threshold and switch the environment sets (sca_forms.h)
    int kd_rank_capacity = 1 << 30;     // workgroups of k_kd_lv_rank the device holds at once (occupancy x CUs)
    // SCA_NBR_AUTO: the grid query for everybody, the kd query for the agents it lists; the kd BUILD (the permutation is history: it
    // runs every step) on a stream of its own beside the grid build and query
    struct Auto {                       // (the slot rule -- which event and list a pass takes -- is plan_auto_build / plan_auto_pass, sca_forms.h)
        hipStream_t stream = nullptr;   // the kd stream
        hipEvent_t ev_fork = nullptr, ev_k1g = nullptr, ev_kd = nullptr, ev_moved = nullptr, ev_cnt = nullptr;
        int32_t *list = nullptr, *count = nullptr;   // two lists and their lengths, alternating by pass (DeviceView::kdq_list / kdq_count point at this pass's)
        int *ticket = nullptr;          // k_neighbors_kd_auto's last-workgroup ticket
        unsigned *busy = nullptr;       // device word, bit 0: somebody is listed for the kd query and it has not answered yet (hipStreamWaitValue32)
        unsigned seq = 0;               // AUTO passes so far (it may wrap)
        bool waitvalue = true;          // false once hipStreamWaitValue32 was refused: an event wait behind the kd query instead (the build is then on every pass's path)
        hipEvent_t ev_kdq[4] = {nullptr, nullptr, nullptr, nullptr};   // [seq & 3] behind the kd query of pass seq (a launch on the kd stream) or, in the launch-free form, behind its build's last kernel
        unsigned *sync = nullptr;       // device words of the launch-free form (KdTail): [0] k_kd_block's ticket, [1] the last pass whose tree is complete, [2] the grid query's ticket
        bool tail_ok = false;           // the tail form is available (with the wait-value form of the pass's wait; Tunables::auto_no_tail: never)
        unsigned tail_seq = 0;          // the pass whose build was enqueued in the tail form (0: none)
        unsigned on_kd = 0;             // bit [seq & 3]: pass seq's kd query was a launch on the kd stream (its list's next user must wait for it)
        hipEvent_t ev_gather[2] = {nullptr, nullptr};   // the gather kernel of the last two builds: the integrate stage must not write into
        unsigned builds = 0;                            // the record buffer a build's gather still reads (the two buffers alternate)
        bool lazy_join = false;         // sca_env_step left the kd stream unjoined: the next entry point other than sca_env_step joins (API_ENTER)
        bool unjoined = false;          // the kd stream may still be working on the last AUTO pass's tree / kd query
        int *count_host = nullptr;      // pinned: the list length of an earlier pass (never waited for)
        bool count_pending = false;
        int last = -1;                  // that length; -1: unknown
        int backoff = 0;                // passes left to run as plain SCA_NBR_KDTREE (the grid listed too many agents: ties everywhere)
        bool ran = false, fits = false; // the last pass was an AUTO pass / the grid's candidate lists cover the collision reach
        bool ahead = false;             // the kd build of the NEXT pass is already enqueued on the kd stream (sca_run_steps, behind the integrate stage)
        unsigned passes = 0;
        int fill(sca_ctx *c);           // the stream, the events and the device words, on first use
        void forget() { ahead = false; last = -1; backoff = 0; }   // the counts say nothing any more, and no tree is built ahead
        void release() {                // behind a synchronised context; (ev_kd aliases ev_kdq[])
            if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
            for (hipEvent_t e : {ev_fork, ev_k1g, ev_moved, ev_cnt, ev_gather[0], ev_gather[1], ev_kdq[0], ev_kdq[1], ev_kdq[2], ev_kdq[3]}) if (e) (void)hipEventDestroy(e);
            for (void *p : {(void *)list, (void *)count, (void *)busy, (void *)sync, (void *)ticket}) if (p) (void)hipFree(p);
            if (count_host) (void)hipHostFree(count_host);
            *this = Auto{};
        }
    } au;
    unsigned prof_tick = 0;             // with profiling on, every 16th pass carries the event pairs (six records, ~35 us on that pass)
    // multi-GPU exchange inside the library (sca_comm_init): one ncclAllGather of the shard's moved records per step
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_nranks = 1;
    // waypoint lists (Agent.path, sca_set_paths): while they are set, k_waypoint runs at the head of every pass
    bool paths_on = false;
    PathView path{};                    // device CSR + cursors + now_goal (sca_kernels.hip.h)
    size_t path_pts_cap = 0;            // doubles path.pts holds
    std::vector<int32_t> h_path_off;    // [n + 1] the CSR offsets as set
    std::vector<uint8_t> h_path_vpref;  // [n] 1: a straight-line agent with a path -- k_waypoint writes its v_pref (vpref_mode = 1)
    // the lists in slot form (sca_set_path_slots): path_W > 0, k_waypoint_slots runs instead; the cursors are path.rem / path.now_goal
    int path_W = 0;                     // room per agent row, in waypoints
    double *pslot_pts = nullptr;        // [3 * pslot_cap] row a's room from 3 * path_slot_index(path_W, a)
    size_t pslot_cap = 0;               // points pslot_pts holds (>= path_W * max_n)
    int32_t *pslot_len = nullptr;       // [max_n] the lists' lengths as set
    std::vector<int32_t> h_path_len;    // [n] host mirror of pslot_len (sca_set_path_state's bound; follows a restart behind its synchronisation)
    // pinned host state block (sca_host_state_get / sca_step_host): allocated once for max_n, freed by sca_destroy
    uint8_t *hs_host = nullptr;         // page-locked, the caller reads and writes it in place
    uint8_t *hs_dev = nullptr;          // the staging buffer of the staged form (Tunables::hs_staged): same size and layout
    // scene batches (sca_set_scenes, sca_scenes.hip.h): while they are set a pass builds a forest and runs the scene forms of K1 and K4
    struct Scenes {
        bool on = false;
        SceneView v{};                  // device arrays; live | prev | steps are one allocation (counters)
        int32_t *counters = nullptr;    // [nscenes * (SCENE_LINE + 2)]
        std::vector<int32_t> h_off;     // [nscenes + 1] the offsets as set
        int32_t *size = nullptr;        // device [nscenes]: the agents a scene holds in the first rows of its range (k_kd_scene_jobs, k_scene_restart)
        std::vector<int32_t> h_size;    // ... and the host's copy; the range's length until sca_restart_scenes_sized says otherwise
        bool partial = false;           // scenes_any_partial(h_size): a whole-context state from outside is refused meanwhile
        int largest = 0;                // agents of the largest scene: picks the k_kd_block instance
        bool live_valid = false;        // SceneView::live describes the current records (else: k_scene_recount before anybody reads it)
        bool begun = false;             // a policy pass has opened a step (scene_begin_one) that no env update has closed yet
        bool obs_on = false;            // one obstacle set per scene (sca_set_scene_obstacles): d.obs .. d.owide hold a forest, K1 and K4 run their SceneObsRoots instances
        SceneObsView ov{};              // device array [nscenes]
        std::vector<int32_t> h_obs_off; // [nscenes + 1] the obstacle offsets as set: each scene's range is its capacity (sca_set_scene_obstacle_slots)
        std::vector<int32_t> h_obs_count; // [nscenes] the obstacles each scene holds in the first rows of its range; the device's copy stands behind ov.oroot
        uint8_t *rs_host = nullptr;     // sca_restart_scenes' page-locked staging block (RestartLayout of max_n, sca_scenes.h), allocated on first use
        size_t rs_bytes = 0;            // ... and its size: it grows when the lists' slot form, or a larger room per row, arrives later
        SceneLogView log{};             // the trajectory log per scene (sca_scene_history_enable), rows null: off -- a step then enqueues nothing for it
        uint8_t *hv_host = nullptr;     // the harvest block (sca_scene_harvest_enable; HarvestLayout of nscenes and n, sca_scenes.h), null: off -- a step then enqueues nothing for it
        HarvestLayout hv_layout{};
        int32_t hv_batch_step = 0;      // env updates enqueued since the harvest was enabled
        uint8_t *ck_host = nullptr;     // sca_save_scenes' / sca_load_scenes' page-locked block (CkptEntry table + blobs, sca_scenes.h), allocated on first use
        size_t ck_bytes = 0;            // ... and its size: it grows when a call needs more
        sca_scene_clearance *clear = nullptr;   // [n] the closest-approach records (sca_scene_clearance_enable), null: off -- a step then enqueues nothing for them
        void release() {                // the device and page-locked allocations, behind a synchronised stream; the flags and host vectors stay
            for (void *p : {(void *)v.scene_of, (void *)v.offsets, (void *)counters, (void *)v.heading_keep, (void *)ov.oroot, (void *)log.rows, (void *)size, (void *)clear}) if (p) (void)hipFree(p);
            if (rs_host) (void)hipHostFree(rs_host);
            if (hv_host) (void)hipHostFree(hv_host);
            if (ck_host) (void)hipHostFree(ck_host);
            ck_host = nullptr; ck_bytes = 0;
            v = SceneView{}; counters = nullptr; size = nullptr; ov = SceneObsView{}; rs_host = nullptr; rs_bytes = 0; log = SceneLogView{}; hv_host = nullptr; clear = nullptr;
        }
    } scenes;
    std::vector<uint8_t> h_policy;      // [n] the agents' policies as they stand (sca_set_agents, sca_restart_scenes)
    sca_dubins::AgentTrack *trk_init = nullptr;   // one default-constructed tracker record on the device (sca_device_tracker_enable)
    // a restart that brings attributes (sca_restart_scenes_attrs): host mirrors of the planner's per-row arrays and the class table
    std::vector<TrackTriple> h_trk_trip;    // [n] (turning radius, pitch_lo, pitch_hi) per row as the device holds them; empty: one value per context
    std::vector<uint8_t> h_trk_cls;         // [n] trk_cls as the device holds it
    ClassTable trk_table;                   // the classes in use over the occupied tracked rows (scene_class_table)
    bool trk_attr_on = false;               // the table governs trk_classes / trk_many / the view (since the first restart that brought planner attributes)
    // respawning agents in place (sca_respawn_agents, sca_get_finished; sca_respawn.h): nothing of it exists until the first call
    uint8_t *rsp_host = nullptr;            // sca_respawn_agents' page-locked block (RespawnLayout of rsp_cap rows and rsp_W waypoints per row)
    int rsp_cap = 0, rsp_W = 0;
    // ... that brings a policy or attributes (sca_respawn_agents_attrs; sca_respawn_attrs.h): nothing of it exists until the first such call
    uint8_t *rspa_host = nullptr;           // the page-locked block of the policy bytes and AgentPar records (RespawnAttrLayout of rspa_cap rows)
    int rspa_cap = 0;
    std::vector<int32_t> rspa_lp[2];        // what the ORCA3D-LP list is uploaded from, by turns: a gated call's copy runs behind its synchronisation
    int rspa_turn = 0;                      //   and is over before the call after the next touches its source (every call synchronises once)
    std::vector<AgentPar> rspa_fill_ap;     // the first-use fill of ap_dev / ap_nd: the context's own values for every row
    std::vector<double> rspa_fill_nd;
    AgentPar *rspa_ap_new = nullptr;        // the first-use arrays until the call that made them has come through: they become ap_dev / ap_nd only
    double *rspa_nd_new = nullptr;          //   behind its synchronisation, so ap_dev != nullptr always means "per-agent arrays in force"
    std::vector<double> rspa_fill_trk[3];   // the first-use fill of the planner's per-row arrays
    std::vector<uint8_t> rspa_cls[2];       // what the class bytes are uploaded from, by turns like rspa_lp
    uint8_t *fin_host = nullptr;            // sca_get_finished's page-locked block: the count's head, fin_cap rows behind it
    int fin_cap = 0;
    int32_t *fin_counts = nullptr;          // device [2 * tiles of max_n]: the tiles' counts, their offsets behind them
    // vacant rows (sca_retire_agents, sca_get_vacant; sca_vacancy.h): nothing of it exists until the first retire
    struct Vacancy {
        bool on = false;                    // a row is vacant: m < n
        int m = 0;                          // the occupied rows while on (else the context's n)
        std::vector<uint8_t> h;             // [n] 1 where the row is vacant (empty until the first retire)
        int32_t *dev = nullptr;             // device: [max_n] the named ids of a retire, [max_n] the edited prefix, the tiles' counts and offsets, one head word
        uint8_t *host = nullptr;            // sca_get_vacant's page-locked block: the count's head, max_n ids behind it
    } vac;
    // spawn admission (sca_probe_clearance, sca_respawn_agents_gated; sca_spawn.h): nothing of it exists until the first call
    uint8_t *spn_host = nullptr;            // the page-locked block (SpawnLayout of spn_cap queries)
    uint8_t *spn_dev = nullptr;             // device: the copy of the block's query sections, the world words and the verdict words behind it
    int spn_cap = 0;
    SpawnPartial *spn_partials = nullptr;   // device [tiles][spn_cap]
    int64_t spn_partials_room = 0;          // ... how many it has room for
    // context checkpoints (sca_save_context, sca_load_context; sca_checkpoint.h): nothing of it exists until the first call
    uint8_t *cx_host = nullptr;             // the page-locked block both calls go through: the blob, the load's done_count stripes behind it
    size_t cx_bytes = 0;                    // ... and its size: it grows when a call needs more
    // mission tables (sca_set_missions; sca_missions.h): nothing of it exists while no tables are set
    struct Missions {
        bool on = false;
        int M = 0, R = 0;
        sca_mission *entries = nullptr;     // device [M n]
        int32_t *words = nullptr;           // device [7 n]: first_ok, first_fail, cursor, flying, ended, collected, live
        sca_mission_result *results = nullptr;   // device [R n]: the rows' rings
        unsigned long long *totals = nullptr;    // device [MST_WORDS]
        int32_t *counts = nullptr;          // device [2 tiles + 1]: the collect's counts per tile, their offsets, the total
        uint8_t *host = nullptr;            // the collect's page-locked block: the count's head, host_cap results behind it
        int64_t host_cap = 0;
        long long updates = 0;              // env updates enqueued since sca_set_missions
        // tables with lists (sca_set_missions_paths on a context in slot form): a take brings the entry's list into the row's room.  Nothing
        // of it exists for tables without lists
        bool lists = false;
        int32_t *path_store = nullptr;      // device, one allocation: the offsets [M n + 1] (padded to 8 bytes), the points behind them; null: every entry brings the empty list
        double *path_pts = nullptr;         // ... the points inside it
        int64_t path_total = 0;             // points the lists hold
        // the admission gate (sca_set_mission_gate): nothing of it exists until a gate is set; freed with the tables
        struct Gate {
            bool on = false;
            double margin = 0.0;
            int cap = 0;
            int32_t *words = nullptr;       // device [4 n]: waiting, verdict, refusals, fresh
            unsigned long long *totals = nullptr;    // device [MGT_WORDS]
            int32_t *list = nullptr;        // device: the count (16 words), the tiles' counts [2 tiles], ids / entry / world [cap] each
            ClearPoint *query = nullptr;    // device [cap]
            SpawnPartial *partials = nullptr;        // device [ptiles][cap]
            int64_t partials_room = 0;      // ... how many it has room for
        } gate;
    } ms;
};

#define CHK(ctx, call)                                                                         \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                    \
            return SCA_ERR_HIP;                                                                \
        }                                                                                      \
    } while (0)
#define ARG(ctx, cond)                                                                         \
    do {                                                                                       \
        if (!(cond)) { (ctx)->err = std::string("bad argument: ") + #cond; return SCA_ERR_ARG; } \
    } while (0)

// a kernel and "record `ev` behind it": the event as the dispatch's own completion signal (hipExtLaunchKernelGGL's stopEvent) -- one packet in
// the queue instead of a dispatch and a barrier packet
#define LAUNCH_REC(ctx, ev, kern, grid, block, stream, ...)                                                            \
    do {                                                                                                               \
        if ((ctx)->tun.ext_stop) hipExtLaunchKernelGGL(kern, grid, block, 0, stream, nullptr, ev, 0, __VA_ARGS__);         \
        else { hipLaunchKernelGGL(kern, grid, block, 0, stream, __VA_ARGS__); CHK(ctx, hipEventRecord(ev, stream)); }  \
    } while (0)
// ... with an event only if there is one (`ev` may be null: a plain launch)
#define LAUNCH_OPT(ctx, ev, kern, grid, block, stream, ...)                                                            \
    do {                                                                                                               \
        if ((ev) != nullptr) LAUNCH_REC(ctx, ev, kern, grid, block, stream, __VA_ARGS__);                              \
        else hipLaunchKernelGGL(kern, grid, block, 0, stream, __VA_ARGS__);                                            \
    } while (0)

template <class T>
static int dalloc(sca_ctx *c, T **p, size_t count) {
    CHK(c, hipMalloc((void **)p, sizeof(T) * (count ? count : 1)));
    CHK(c, hipMemsetAsync(*p, 0, sizeof(T) * (count ? count : 1), c->stream));
    return 0;
}
// positions replaced from outside (sca_set_state ...): the level statistics of older trees do not apply
static void positions_replaced(sca_ctx *c) { c->kd_single_hint = 0; c->kd_gen++; }
// a whole state arrived from outside (sca_set_state, sca_step_host with SCA_HOST_IN_STATE).  h_pos_valid is the caller's: only sca_set_state keeps a host mirror
static void state_replaced(sca_ctx *c) {
    positions_replaced(c);                // a new state: the previous trees' depth profile says nothing
    c->au.forget();                       // ... and neither do the AUTO passes' counts (no tree is built ahead across calls: sca_run_steps consumes its own or abandons it)
    c->near_valid = false; c->state_set = true; c->state_fresh = true; c->scenes.live_valid = false; c->scenes.begun = false;
}
// the next event of a profiling pool that grows on demand, up to `cap` in use (beyond it: *e stays as it is)
static int pool_take(sca_ctx *c, std::vector<hipEvent_t> &pool, int &used, int cap, hipEvent_t *e) {
    if (used >= cap) return 0;
    if (used == (int)pool.size()) { hipEvent_t n_; CHK(c, hipEventCreate(&n_)); pool.push_back(n_); }
    *e = pool[used++];
    return 0;
}
static int pool_event(sca_ctx *c, hipEvent_t *out) { return pool_take(c, c->pool, c->pool_used, 4 * 4096, out); }
// the mean time from event `at` to event `at + 1` over every `stride` events a pool has handed out
static int pool_mean_ms(sca_ctx *c, const std::vector<hipEvent_t> &pool, int used, int stride, int at, float *ms) {
    double sum = 0;
    const int k = used / stride;
    for (int s = 0; s < k; s++) { float t = 0; CHK(c, hipEventElapsedTime(&t, pool[stride * s + at], pool[stride * s + at + 1])); sum += t; }
    *ms = (float)(sum / k);
    return 0;
}

// sca_env_step (the drop-in loop's one call per step) returns without putting the kd stream in front of the context's stream -- an SCA_NBR_AUTO
// pass leaves the tree build and the kd query of the listed agents there, and the next pass copes with that by itself, as inside a burst of
// sca_run_steps.  Every OTHER entry point joins first: it may read the tree, the permutation or the lists, or enqueue work that does.
static int auto_join(sca_ctx *c);
static int clearance_drop(sca_ctx *c);
static int missions_drop(sca_ctx *c);
static int missions_standing(sca_ctx *c, const char *who, MissionFault f);
static int mission_refuse(sca_ctx *c, const char *who, MissionFault f, int64_t entry);
static int missions_refresh_live(sca_ctx *c);
static int missions_host_flight(sca_ctx *c, const int32_t *ids, const int32_t *verdict, int count);
static int missions_retired(sca_ctx *c, const int32_t *ids, int count);
static int missions_gate_new_state(sca_ctx *c);
static int missions_gate_partials(sca_ctx *c, int m);
static int missions_path_mirrors(sca_ctx *c);
static ClearanceState clearance_state(const sca_ctx *c);
static int clearance_refuse(sca_ctx *c, const char *who, ClearanceFault f);
static int api_enter(sca_ctx *c);
#define API_ENTER(ctx)                                                                          \
    do {                                                                                       \
        if (!(ctx)) return SCA_ERR_ARG;                                                        \
        if (int r_ = api_enter(ctx)) return r_;                                                \
    } while (0)

extern "C" {

// A version-100 caller's sca_params is 56 bytes (no dt_nominal) with `reserved` = 0 where struct_bytes now sits: sca_default_params keeps
// writing exactly those 56 bytes, sca_create reads dt_nominal only from a struct that says it has one.
void sca_default_params_v2(sca_params *p, int32_t struct_bytes) {
    p->neighbor_dist = 10.0; p->time_step = 0.1; p->time_horizon = 10.0; p->max_speed = 1.0;
    p->max_heading_change = M_PI / 4; p->near_goal_threshold = 0.5; p->max_neighbors = 16;
    const bool has_dt = struct_bytes >= (int32_t)(offsetof(sca_params, dt_nominal) + sizeof(double));
    p->struct_bytes = has_dt ? struct_bytes : 0;
    if (has_dt) p->dt_nominal = 0.1;
}
void sca_default_params(sca_params *p) { sca_default_params_v2(p, 0); }
int sca_version(void) { return 103; }   // 103: sca_set_paths / sca_get_path_state / sca_set_path_state, SCA_FORM_WAYPOINTS
                                        // 102: sca_params.struct_bytes + sca_default_params_v2, selftest codes 11-14, SCA_FORM_ACTION_FB / _AUTO_TAIL

const char *sca_last_error(const sca_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int sca_candidate_table(int num_N, double *unit, double *phi_num) {
    if (num_N <= 0 || !unit || !phi_num) return SCA_ERR_ARG;
    candidate_table_host(num_N, unit, phi_num);
    return 0;
}

int sca_kd_build_host(int n, const double *pos, int32_t *perm, double *tree_out) {
    if (n < 0 || (n > 0 && (!pos || !perm))) return SCA_ERR_ARG;
    std::vector<KdNode> tree;
    kd_build_host(n, pos, perm, tree);
    if (tree_out)
        for (int i = 0; i < 2 * n - 1; i++) {
            double *t = tree_out + 10 * (size_t)i;
            t[0] = tree[i].begin; t[1] = tree[i].end; t[2] = tree[i].left; t[3] = tree[i].right;
            for (int k = 0; k < 3; k++) { t[4 + k] = tree[i].mn[k]; t[7 + k] = tree[i].mx[k]; }
        }
    return 0;
}

// ---- what the tracker's parity claim is conditional on ----------------------------------------------------------------------
// The tracker (host and device) computes sin / cos / atan2 / acos / x ** 2 with a restatement of ONE libm build: GNU C Library
// 2.35, x86-64, the FMA variants its ifunc resolvers pick on AVX2 machines (sca_glibc_math.h) -- the libm the golden fixtures were
// recorded with.  A Python reference run on THIS host calls THIS host's libm; where that is another build (another glibc, a CPU
// without FMA, aarch64) the reference itself would print other last bits than the fixtures, and the library would keep printing
// 2.35's.  sca_libm_check compares the two on a fixed argument set (5 x 4096 points over the ranges a flight path produces) so
// that the condition is visible at run time: 0 = this host's libm gives the restated bits, 1 = it does not (mismatch counts per
// function in mismatches[5]: sin, cos, atan2, acos, pow(x, 2)).  Informational: nothing in the library changes its behaviour.
static double (*volatile p_sin)(double) = std::sin;
static double (*volatile p_cos)(double) = std::cos;
static double (*volatile p_atan2)(double, double) = std::atan2;
static int g_libm_state = -1;                   // -1 unknown, 0 equal, 1 different
static int64_t g_libm_bad[5] = {0, 0, 0, 0, 0};
static std::once_flag g_libm_once;              // trackers may be created from several threads: one check, no race on the statics
static void libm_check_once();
static int libm_check_run() {
    std::call_once(g_libm_once, libm_check_once);
    return g_libm_state;
}
static void libm_check_once() {
    unsigned long long st = 0x9E3779B97F4A7C15ull;
    auto u01 = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (double)(st >> 11) * (1.0 / 9007199254740992.0); };
    auto same = [](double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0 || (a != a && b != b); };
    int64_t bad[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < 4096; i++) {
        const int k = i & 7;
        // angles: fractions of a turn, many turns (path angles are un-reduced sums), tiny, next to multiples of pi / 2
        double a = k < 3 ? (u01() - 0.5) * 4.0 * M_PI : k < 5 ? (u01() - 0.5) * 2000.0 : k == 5 ? (u01() - 0.5) * std::ldexp(1.0, -(int)(u01() * 60))
                 : (double)(int)(u01() * 64 - 32) * M_PI_2 + (u01() - 0.5) * 1e-6;
        if (!same(sca_gm::g_sin(a), p_sin(a))) bad[0]++;
        if (!same(sca_gm::g_cos(a), p_cos(a))) bad[1]++;
        // arctangents: both components over fourteen decades, every quadrant, quotients on both sides of 1/16 and of 1
        const double y = (u01() - 0.5) * std::pow(10.0, u01() * 14 - 9), x = (u01() - 0.5) * std::pow(10.0, u01() * 14 - 9);
        if (!same(sca_gm::g_atan2(y, x), p_atan2(y, x))) bad[2]++;
        const double cth = k < 6 ? u01() * 2.0 - 1.0 : (k == 6 ? 1.0 - u01() * 1e-9 : -1.0 + u01() * 1e-9);
        if (!same(sca_gm::g_acos(cth), p_acos(cth))) bad[3]++;
        const double b = (u01() - 0.5) * std::pow(10.0, u01() * 12 - 6);
        if (!same(sca_gm::g_pow2(b), p_pow(b, 2.0))) bad[4]++;
    }
    int64_t total = 0;
    for (int q = 0; q < 5; q++) { g_libm_bad[q] = bad[q]; total += bad[q]; }
    g_libm_state = total ? 1 : 0;
    if (g_libm_state && !getenv("SCA_QUIET"))
        fprintf(stderr, "[libsca_hip] note: this host's libm differs from the restated glibc 2.35 x86-64 FMA build in %lld of 20480 test "
                        "arguments (sin %lld, cos %lld, atan2 %lld, acos %lld, pow(x,2) %lld): the Dubins tracker reproduces the bits of THAT "
                        "libm (the one the golden vectors were recorded with); a Python reference run on this host would differ from both "
                        "in the last bit of some path lengths.\n",
                (long long)total, (long long)bad[0], (long long)bad[1], (long long)bad[2], (long long)bad[3], (long long)bad[4]);
}
int sca_libm_check(int64_t *mismatches /*5, nullable*/) {
    const int r = libm_check_run();
    if (mismatches) for (int q = 0; q < 5; q++) mismatches[q] = g_libm_bad[q];
    return r;
}

// ---- native v_pref tracker (host only, no GPU needed): scaPolicy.py:264-338 + dubinsmaneuver2d/3d.py ----------------
void *sca_tracker_create(int n, const double *goal, const double *goal_heading, const double *pref_speed,
                         const uint8_t *zaxis, double turning_radius, double pitch_min, double pitch_max,
                         double neighbor_dist) {
    if (n <= 0 || !goal || !goal_heading || !pref_speed) return nullptr;
    (void)libm_check_run();                                              // one note on stderr when this host's libm is another build
    auto *T = new sca_dubins::Tracker();
    T->n = n;
    T->goal.assign(goal, goal + 3 * (size_t)n);
    T->goal_heading.assign(goal_heading, goal_heading + 3 * (size_t)n);
    T->pref_speed.assign(pref_speed, pref_speed + n);
    T->zaxis.assign((size_t)n, 0);
    if (zaxis) T->zaxis.assign(zaxis, zaxis + n);
    T->turning_radius = turning_radius; T->pitchlims[0] = pitch_min; T->pitchlims[1] = pitch_max;
    T->neighbor_dist = neighbor_dist;
    T->st.assign((size_t)n, sca_dubins::AgentTrack());
    return T;
}
int sca_tracker_set_neighbor_dist(void *tr, const double *neighbor_dist /*n, nullable: back to the one value*/) {
    if (!tr) return SCA_ERR_ARG;
    auto *T = (sca_dubins::Tracker *)tr;
    if (neighbor_dist) T->nd_per_agent.assign(neighbor_dist, neighbor_dist + T->n); else T->nd_per_agent.clear();
    return 0;
}
int sca_tracker_set_agent_params(void *tr, const double *turning_radius, const double *pitch_lo, const double *pitch_hi) {
    if (!tr) return SCA_ERR_ARG;
    auto *T = (sca_dubins::Tracker *)tr;
    auto put = [&](std::vector<double> &v, const double *a) { if (a) v.assign(a, a + T->n); else v.clear(); };
    put(T->R_pa, turning_radius); put(T->plo_pa, pitch_lo); put(T->phi_pa, pitch_hi);
    return 0;
}
void sca_tracker_destroy(void *tr) {
    auto *T = (sca_dubins::Tracker *)tr;
    if (T) { delete T->pool; delete T; }
}
int sca_tracker_vpref(void *tr, const double *pos, const float *vel, const double *heading, const uint8_t *active,
                      const double *nbr0_dsq, double *vpref_out, int nthreads) {
    if (!tr || !pos || !vel || !heading || !active || !nbr0_dsq || !vpref_out) return SCA_ERR_ARG;
    sca_dubins::step_all(*(sca_dubins::Tracker *)tr, pos, vel, heading, active, nbr0_dsq, vpref_out, nthreads);
    return 0;
}
// diagnostics: the tracker record of one agent as 24 doubles (host tracker / device tracker): horizontal maneuver r_min, t, p,
// length; vertical r_min, t, p, length; plan length, sampling size, 0, 0, next, count, now_goal[3], v_pref[3], words
static void track_dump(const sca_dubins::AgentTrack &a, double *o) {
    const sca_dubins::Plan3D &P = a.plan;
    o[0] = P.h.r_min; o[1] = P.h.t; o[2] = P.h.p; o[3] = P.h.length; o[4] = P.v.r_min; o[5] = P.v.t; o[6] = P.v.p; o[7] = P.v.length;
    o[8] = P.length; o[9] = P.sampling_size; o[10] = (double)P.rounds; o[11] = 0.0; o[12] = (double)a.next; o[13] = (double)P.count;
    for (int q = 0; q < 3; q++) { o[14 + q] = a.now_goal[q]; o[17 + q] = a.v_pref[q]; }
    o[20] = P.mode[0] * 65536.0 + P.mode[1] * 256.0 + P.mode[2]; o[21] = P.mode[3] * 65536.0 + P.mode[4] * 256.0 + P.mode[5];
    o[22] = 64.0 * P.iters; o[23] = (double)a.replans;
}
int sca_tracker_debug(void *tr, int agent, double *out24) {
    if (!tr || !out24) return SCA_ERR_ARG;
    auto *T = (sca_dubins::Tracker *)tr;
    if (agent < 0 || agent >= T->n) return SCA_ERR_ARG;
    track_dump(T->st[agent], out24);
    return 0;
}
int sca_tracker_replans(void *tr, int32_t *replans) {
    if (!tr || !replans) return SCA_ERR_ARG;
    auto *T = (sca_dubins::Tracker *)tr;
    for (int i = 0; i < T->n; i++) replans[i] = T->st[i].replans;
    return 0;
}
int sca_dubins_plan(const double *qi5, const double *qf5, double rmin, double pitch_min, double pitch_max, double *length,
                    char *mode7, int32_t *n_samples, double *samples, int cap) {
    if (!qi5 || !qf5 || !length || !mode7) return SCA_ERR_ARG;
    const double pl[2] = {pitch_min, pitch_max};
    const sca_dubins::Plan3D P = sca_dubins::plan3d(qi5, qf5, rmin, pl);
    if (!P.ok) return SCA_ERR_STATE;
    *length = P.length;
    std::memcpy(mode7, P.mode, 7);
    const int cnt = (int)P.count;
    if (n_samples) *n_samples = cnt;
    if (samples) for (int i = 0; i < std::min(cnt, cap); i++) P.sample(i, samples + 5 * (size_t)i);
    return 0;
}

// host self-test: the lean search of the device's lane-per-plan kernels (sca_dubins.hpp, plan3d_lean, compiled for the host)
// against the literal plan3d on the given poses, bit for bit
int sca_selftest_plan3d_lean(int n, const double *q, double turning_radius, double pitch_lo, double pitch_hi, int64_t *mismatches,
                             int64_t *lean_candidates, int64_t *literal_candidates) {
    if (n < 0 || !q || !mismatches) return SCA_ERR_ARG;
    const double pl[2] = {pitch_lo, pitch_hi};
    auto same = [](double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0 || (a != a && b != b); };
    int64_t bad = 0;
    sca_dubins::lean::g_host_fast = sca_dubins::lean::g_host_literal = 0;
    for (int i = 0; i < n; i++) {
        const double *qi = q + 10 * (size_t)i, *qf = qi + 5;
        const sca_dubins::Plan3D A = sca_dubins::plan3d(qi, qf, turning_radius, pl), B = sca_dubins::plan3d_lean(qi, qf, turning_radius, pl);
        bool ok = A.ok == B.ok && A.iters == B.iters && A.count == B.count && same(A.length, B.length) && same(A.sampling_size, B.sampling_size) &&
                  std::memcmp(A.mode, B.mode, 7) == 0;
        const sca_dubins::Maneuver2D *ma[2] = {&A.h, &A.v}, *mb[2] = {&B.h, &B.v};
        for (int k = 0; k < 2 && ok && A.ok; k++)
            ok = same(ma[k]->r_min, mb[k]->r_min) && same(ma[k]->t, mb[k]->t) && same(ma[k]->p, mb[k]->p) && same(ma[k]->length, mb[k]->length) &&
                 same(ma[k]->yaw, mb[k]->yaw);
        if (!ok) bad++;
    }
    *mismatches = bad;
    if (lean_candidates) *lean_candidates = sca_dubins::lean::g_host_fast;
    if (literal_candidates) *literal_candidates = sca_dubins::lean::g_host_literal;
    return 0;
}

// host self-test: the sign-parametrised CSC word of the device's four-lane planner against the literal word(), bit for bit
int sca_selftest_dubins_words(int n, const double *alpha, const double *beta, const double *d, int64_t *mismatches) {
    if (n < 0 || !alpha || !beta || !d || !mismatches) return SCA_ERR_ARG;
    int64_t bad = 0;
    auto same = [](double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0 || (a != a && b != b); };
    for (int i = 0; i < n; i++) {
        double sa, sb, ca, cb;
        sca_dubins::m_sincos(alpha[i], sa, ca);
        sca_dubins::m_sincos(beta[i], sb, cb);
        const double c_ab = sca_dubins::m_cos(alpha[i] - beta[i]);
        const double mb = sca_dubins::mod2pi(beta[i]);
        for (int w = 0; w < 4; w++) {
            double t0 = 0, p0 = 0, q0 = 0, t1 = 0, p1 = 0, q1 = 0;
            char mode[3];
            const bool ok0 = sca_dubins::word(w, alpha[i], beta[i], d[i], sa, sb, ca, cb, c_ab, t0, p0, q0, mode);
            const bool ok1 = sca_dubins::csc_word_uniform(w, alpha[i], beta[i], mb, d[i], sa, sb, ca, cb, c_ab, t1, p1, q1);
            if (ok0 != ok1 || (ok0 && !(same(t0, t1) && same(p0, p1) && same(q0, q1)))) bad++;
        }
    }
    *mismatches = bad;
    return 0;
}

// ---- the same tracker on the device (sca_tracker.hip.h) ---------------------------------------------------------------
static int launch_tracker(sca_ctx *c, bool from_lists, bool in_pass, int &forms);
static int part_free(sca_ctx *c);
static int part_classify(sca_ctx *c);
static int agent_params_clear(sca_ctx *c);
static int paths_clear(sca_ctx *c, bool reset_mode);
static int tracker_free(sca_ctx *c) {
    if (!c->trk.st) { c->trk_on = false; return 0; }
    CHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(c->trk.st); (void)hipFree(c->trk.nbr0); (void)hipFree(c->trk.list); (void)hipFree(c->trk.count); (void)hipFree(c->trk.bcount);
    (void)hipFree(c->trk_goal_heading);
    if (c->trk_init) { (void)hipFree(c->trk_init); c->trk_init = nullptr; }
    if (c->trk_R_pa) { (void)hipFree(c->trk_R_pa); c->trk_R_pa = nullptr; }
    if (c->trk_cls) { (void)hipFree(c->trk_cls); c->trk_cls = nullptr; }
    if (c->trk_plo_pa) { (void)hipFree(c->trk_plo_pa); c->trk_plo_pa = nullptr; }
    if (c->trk_phi_pa) { (void)hipFree(c->trk_phi_pa); c->trk_phi_pa = nullptr; }
    c->trk_many = false;
    c->trk_classes.clear();
    c->trk_attr_on = false; c->h_trk_trip.clear(); c->h_trk_cls.clear(); c->trk_table = ClassTable{};
    if (c->trk_stream) { (void)hipStreamSynchronize(c->trk_stream); (void)hipStreamDestroy(c->trk_stream); c->trk_stream = nullptr; }
    if (c->trk_fork) { (void)hipEventDestroy(c->trk_fork); c->trk_fork = nullptr; }
    if (c->trk_join) { (void)hipEventDestroy(c->trk_join); c->trk_join = nullptr; }
    if (c->trk_count_ev) { (void)hipEventDestroy(c->trk_count_ev); c->trk_count_ev = nullptr; }
    if (c->trk_host_count) { (void)hipHostFree(c->trk_host_count); c->trk_host_count = nullptr; }
    c->trk_count_pending = false; c->trk_last_count = -1;
    c->kd.skip_prep = 0;
    c->trk = TrackDev{}; c->trk_goal_heading = nullptr; c->trk_on = false; c->trk_in_pass = false;
    c->d.trk_nbr0 = nullptr;
    // the tracked agents go back to their policy's own v_pref rule (rvo3dPolicy.py:182-196): until round 5 they kept vpref_mode = 1 and the
    // tracker's LAST output, frozen -- bench.py's `solver_only` legs ran on that instead of the straight-line rule they are labelled with
    if (c->d.vpref_mode && c->n > 0) { CHK(c, hipMemsetAsync(c->d.vpref_mode, 0, c->n, c->stream)); CHK(c, hipStreamSynchronize(c->stream)); }
    return 0;
}
int sca_device_tracker_enable(sca_ctx *c, const double *goal_heading, double turning_radius, double pitch_min, double pitch_max,
                              int in_pass) {
    API_ENTER(c);
    if (!c->agents_set) { c->err = "sca_set_agents first"; return SCA_ERR_STATE; }
    ARG(c, goal_heading && turning_radius > 0);
    if (int r = tracker_free(c)) return r;
    const int n = c->n;
    CHK(c, hipMalloc((void **)&c->trk.st, sizeof(sca_dubins::AgentTrack) * n));
    CHK(c, hipMalloc((void **)&c->trk.nbr0, sizeof(double) * n));
    CHK(c, hipMalloc((void **)&c->trk.list, sizeof(int32_t) * (size_t)n * TRK_BUCKETS));
    CHK(c, hipMalloc((void **)&c->trk.count, sizeof(int32_t) * 4));
    CHK(c, hipMalloc((void **)&c->trk.bcount, sizeof(int32_t) * 4 * TRK_BUCKETS));
    c->trk.n = n;
    CHK(c, hipMalloc((void **)&c->trk_goal_heading, sizeof(double) * 3 * n));
    CHK(c, hipMalloc((void **)&c->trk_init, sizeof(sca_dubins::AgentTrack)));     // what a restarted scene's records go back to (k_scene_restart)
    CHK(c, hipStreamCreateWithFlags(&c->trk_stream, hipStreamNonBlocking));
    CHK(c, hipEventCreateWithFlags(&c->trk_fork, hipEventDisableTiming));
    CHK(c, hipEventCreateWithFlags(&c->trk_join, hipEventDisableTiming));
    CHK(c, hipEventCreateWithFlags(&c->trk_count_ev, hipEventDisableTiming));
    CHK(c, hipHostMalloc((void **)&c->trk_host_count, sizeof(int) * 2));
    c->trk_count_pending = false; c->trk_last_count = -1;
    std::vector<sca_dubins::AgentTrack> init((size_t)n);
    std::vector<double> nb((size_t)n, -1.0);
    std::vector<uint8_t> pol((size_t)n), mode((size_t)n);
    CHK(c, hipMemcpyAsync(pol.data(), c->d.policy, n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipMemcpyAsync(c->trk.st, init.data(), sizeof(sca_dubins::AgentTrack) * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->trk_init, init.data(), sizeof(sca_dubins::AgentTrack), hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->trk.nbr0, nb.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->trk_goal_heading, goal_heading, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemsetAsync(c->trk.count, 0, sizeof(int32_t) * 4, c->stream));
    CHK(c, hipMemsetAsync(c->trk.bcount, 0, sizeof(int32_t) * 4 * TRK_BUCKETS, c->stream));
    CHK(c, hipMemsetAsync(c->d.nbr_valid, 0, n, c->stream));            // no policy pass of this agent set has left lists yet
    CHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; i++) mode[i] = (pol[i] == SCA_POLICY_SCA || pol[i] == SCA_POLICY_RVO3D_DUBINS) ? 1 : 0;
    CHK(c, hipMemcpyAsync(c->d.vpref_mode, mode.data(), n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemsetAsync(c->d.vpref_ext, 0, sizeof(double) * 3 * n, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    c->trk.parity = 0;
    c->trk_view = sca_dubins::TrackView{c->d.goal, c->trk_goal_heading, c->d.pref_speed, c->d.zaxis, turning_radius, pitch_min,
                                        pitch_max, c->P.neighbor_dist, c->ap_nd, nullptr, nullptr, nullptr, nullptr, 0};
    c->trk_classes.clear();
    c->trk_many = false;
    c->trk_enable_vals[0] = turning_radius; c->trk_enable_vals[1] = pitch_min; c->trk_enable_vals[2] = pitch_max;
    {   // resolve the tracker's kernels now: the first launch of a kernel pays for looking it up in the code object, and the
        // forms are picked while the episode runs (k_track_replan's first launch used to fall into a timed step)
        hipFuncAttributes fa;
        for (const void *f : {(const void *)k_track, (const void *)k_replan, (const void *)k_replan_group<64>, (const void *)k_replan_group<32>,
                              (const void *)k_replan_group<16>, (const void *)k_replan_group<4>,
                              (const void *)k_track_replan, (const void *)k_solve_sweep, (const void *)k_solve_pick4})
            (void)hipFuncGetAttributes(&fa, f);
    }
    (void)libm_check_run();              // informational: one note on stderr, the verdict through sca_libm_check(); sca_last_error stays for failures
    c->trk_on = true; c->trk_in_pass = in_pass != 0;
    c->d.trk_nbr0 = c->trk_in_pass ? c->trk.nbr0 : nullptr;
    c->trk_passes = 0;
    tunables_from_env(c->tun, c->simds, TUN_AT_TRACKER);
    return 0;
}
// agent.turning_radius / agent.pitchlims per agent (scaPolicy.py:95,272,302 read the agent's own).  Arrays of n, any of them NULL = the value of
// sca_device_tracker_enable for everybody; all NULL: back to that one value.  Untracked agents' entries (policy not SCA / RVO3D+Dubins) are ignored.
// Up to TRK_MAX_CLASSES distinct (R, lo, hi) among the tracked agents: CLASSES -- the re-plan kernels run once per class with the class's
// values as kernel arguments (scalar registers throughout the search).  More than that (the reference has no limit, agent.py:24-29): the
// PER-AGENT form -- every re-plan gets a wavefront of its own (k_replan_group<64> / k_track_group at any count), which loads ITS agent's
// three values into scalar registers; slower than the lane-per-plan forms for large counts, never refused.
// The view a set of classes gives (trk_R_pa is current for every row, and where `many`, trk_plo_pa / trk_phi_pa; otherwise trk_cls).
// classes: by index; an index nobody uses holds a NaN radius and gets no launch.  many: the per-agent arrays.  Two or more classes: a
// filter by the class byte, one launch per index in use.  One: its values in the scalars and no filter.  None: the enable call's values.
static void tracker_view_apply(sca_ctx *c, bool many, const std::vector<std::array<double, 3>> &classes) {
    sca_dubins::TrackView &V = c->trk_view;
    V.R_pa = c->trk_R_pa; V.plo_pa = nullptr; V.phi_pa = nullptr; V.cls = nullptr; V.class_id = 0;
    V.turning_radius = c->trk_enable_vals[0]; V.pitch_lo = c->trk_enable_vals[1]; V.pitch_hi = c->trk_enable_vals[2];
    c->trk_classes.clear(); c->trk_many = many;
    if (many) { V.plo_pa = c->trk_plo_pa; V.phi_pa = c->trk_phi_pa; return; }
    int used = 0, only = -1;
    for (size_t q = 0; q < classes.size(); q++) if (!std::isnan(classes[q][0])) { used++; only = (int)q; }
    if (used > 1) { c->trk_classes = classes; V.cls = c->trk_cls; }
    else if (used == 1) { V.turning_radius = classes[only][0]; V.pitch_lo = classes[only][1]; V.pitch_hi = classes[only][2]; }
}
constexpr size_t TRK_MAX_CLASSES = 16;
static_assert(TRK_MAX_CLASSES == (size_t)TRK_CLASS_CAP, "scene_class_table deals the classes sca_device_tracker_set_agent_params deals");
int sca_device_tracker_set_agent_params(sca_ctx *c, int n, const double *turning_radius, const double *pitch_lo, const double *pitch_hi) {
    API_ENTER(c);
    if (!c->trk_on) { c->err = "sca_device_tracker_enable first"; return SCA_ERR_STATE; }
    CHK(c, hipStreamSynchronize(c->stream));
    // (every call starts from the enable-time values: a one-class call overwrites the view's scalars, and "any of them NULL" / "all NULL"
    // promise sca_device_tracker_enable's values, not the previous call's -- ADVICE r5)
    c->trk_view.turning_radius = c->trk_enable_vals[0]; c->trk_view.pitch_lo = c->trk_enable_vals[1]; c->trk_view.pitch_hi = c->trk_enable_vals[2];
    c->trk_classes.clear();
    c->trk_many = false;
    c->trk_view.R_pa = nullptr; c->trk_view.plo_pa = nullptr; c->trk_view.phi_pa = nullptr; c->trk_view.cls = nullptr; c->trk_view.class_id = 0;
    c->trk_attr_on = false; c->h_trk_trip.clear(); c->h_trk_cls.clear(); c->trk_table = ClassTable{};   // (a later attribute restart starts from this call's values)
    if (!turning_radius && !pitch_lo && !pitch_hi) return 0;
    ARG(c, n == c->n);
    // tracked = by POLICY, as the kernels decide it (tracker_owns), not by the v_pref mode of the moment (sca_set_vpref may change that later)
    std::vector<uint8_t> pol((size_t)n), cls((size_t)n, 0);
    CHK(c, hipMemcpy(pol.data(), c->d.policy, (size_t)n, hipMemcpyDeviceToHost));
    std::vector<std::array<double, 3>> classes;
    std::vector<double> R((size_t)n), LO((size_t)n), HI((size_t)n);
    bool many = false;
    for (int i = 0; i < n; i++) {
        const std::array<double, 3> v = {turning_radius ? turning_radius[i] : c->trk_enable_vals[0], pitch_lo ? pitch_lo[i] : c->trk_enable_vals[1],
                                         pitch_hi ? pitch_hi[i] : c->trk_enable_vals[2]};
        R[i] = v[0]; LO[i] = v[1]; HI[i] = v[2];
        if (pol[i] != SCA_POLICY_SCA && pol[i] != SCA_POLICY_RVO3D_DUBINS) continue;     // not a tracked agent
        if (!(std::isfinite(v[0]) && v[0] > 0.0) || !std::isfinite(v[1]) || !std::isfinite(v[2]) || !(v[1] < v[2])) {
            c->err = "sca_device_tracker_set_agent_params: agent " + std::to_string(i) + " has a turning radius / pitch limits out of range (R > 0, pitch_lo < pitch_hi)";
            return SCA_ERR_ARG;
        }
        if (many) continue;
        size_t k = 0;
        while (k < classes.size() && classes[k] != v) k++;
        if (k == classes.size()) {
            if (classes.size() == TRK_MAX_CLASSES) { many = true; continue; }
            classes.push_back(v);
        }
        cls[i] = (uint8_t)k;
    }
    if (!c->trk_R_pa) { CHK(c, hipMalloc((void **)&c->trk_R_pa, sizeof(double) * (size_t)c->max_n)); CHK(c, hipMalloc((void **)&c->trk_cls, (size_t)c->max_n)); }
    c->h_trk_trip.resize((size_t)n);
    for (int i = 0; i < n; i++) c->h_trk_trip[i] = TrackTriple{R[i], LO[i], HI[i]};
    CHK(c, hipMemcpy(c->trk_R_pa, R.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    c->trk_view.R_pa = c->trk_R_pa;
    if (many) {
        if (!c->trk_plo_pa) {
            CHK(c, hipMalloc((void **)&c->trk_plo_pa, sizeof(double) * (size_t)c->max_n));
            CHK(c, hipMalloc((void **)&c->trk_phi_pa, sizeof(double) * (size_t)c->max_n));
        }
        CHK(c, hipMemcpy(c->trk_plo_pa, LO.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
        CHK(c, hipMemcpy(c->trk_phi_pa, HI.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    } else CHK(c, hipMemcpy(c->trk_cls, cls.data(), (size_t)n, hipMemcpyHostToDevice));
    tracker_view_apply(c, many, classes);
    return 0;
}
int sca_device_tracker_disable(sca_ctx *c) {
    API_ENTER(c);
    return tracker_free(c);
}
int sca_device_tracker_vpref(sca_ctx *c, const double *nbr0_dsq, double *vpref_out) {
    API_ENTER(c);
    if (!c->trk_on || !c->state_set) { c->err = "sca_device_tracker_enable and sca_set_state first"; return SCA_ERR_STATE; }
    if (nbr0_dsq) CHK(c, hipMemcpyAsync(c->trk.nbr0, nbr0_dsq, sizeof(double) * c->n, hipMemcpyHostToDevice, c->stream));
    int forms = 0;
    if (int r = launch_tracker(c, nbr0_dsq == nullptr, false, forms)) return r;
    c->forms |= forms;
    if (vpref_out) CHK(c, hipMemcpyAsync(vpref_out, c->d.vpref_ext, sizeof(double) * 3 * c->n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
int sca_device_tracker_debug(sca_ctx *c, int agent, double *out24) {
    if (!c || !out24) return SCA_ERR_ARG;
    if (int r_ = api_enter(c)) return r_;
    if (!c->trk_on || agent < 0 || agent >= c->n) { c->err = "no device tracker / bad agent"; return SCA_ERR_STATE; }
    sca_dubins::AgentTrack a;
    CHK(c, hipStreamSynchronize(c->stream));
    CHK(c, hipMemcpy(&a, c->trk.st + agent, sizeof(a), hipMemcpyDeviceToHost));
    track_dump(a, out24);
    return 0;
}
int sca_device_tracker_replans(sca_ctx *c, int32_t *replans) {
    API_ENTER(c);
    ARG(c, replans);
    if (!c->trk_on) { c->err = "sca_device_tracker_enable first"; return SCA_ERR_STATE; }
    int32_t *tmp = (int32_t *)c->trk.list;                              // free between passes
    hipLaunchKernelGGL(k_track_replans, dim3((c->n + 255) / 256), dim3(256), 0, c->stream, c->trk.st, tmp, c->n);
    CHK(c, hipMemcpyAsync(replans, tmp, sizeof(int32_t) * c->n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int sca_create(const sca_params *p, int device, int max_agents, int max_obstacles, sca_ctx **out) {
    if (!out || max_agents <= 0 || max_obstacles < 0) return SCA_ERR_ARG;
    sca_ctx *c = new sca_ctx();
    *out = c;
    sca_params def, own;
    sca_default_params_v2(&def, (int32_t)sizeof(sca_params));
    if (!p) p = &def;
    if (p->struct_bytes < (int32_t)(offsetof(sca_params, dt_nominal) + sizeof(double))) {     // a version-100 struct: 56 bytes, no dt_nominal
        memcpy(&own, p, offsetof(sca_params, dt_nominal));
        own.struct_bytes = (int32_t)sizeof(sca_params);
        own.dt_nominal = own.time_step;
        p = &own;
    }
    if (p->max_neighbors < 1 || p->max_neighbors > SCA_MAX_NEIGHBORS) { c->err = "max_neighbors out of range (1 .. 16)"; return SCA_ERR_ARG; }
    {   // the kernels divide by these, size grid cells with them and bisect acos on max_heading_change: refuse what they were not built for
        auto pos = [](double x) { return std::isfinite(x) && x > 0.0; };
        const char *bad = !pos(p->neighbor_dist) ? "neighbor_dist" : !pos(p->time_step) ? "time_step" : !pos(p->time_horizon) ? "time_horizon"
                        : !pos(p->max_speed) ? "max_speed" : !pos(p->dt_nominal) ? "dt_nominal"
                        : !(std::isfinite(p->near_goal_threshold) && p->near_goal_threshold >= 0.0) ? "near_goal_threshold"
                        : !(p->max_heading_change >= 0.0 && p->max_heading_change <= M_PI) ? "max_heading_change" : nullptr;
        if (bad) { c->err = std::string("sca_params.") + bad + " out of range"; return SCA_ERR_ARG; }
    }
    c->device = device; c->max_n = max_agents; c->max_m = max_obstacles;
    c->P.neighbor_dist = p->neighbor_dist; c->P.time_step = p->time_step; c->P.time_horizon = p->time_horizon;
    c->P.max_speed = p->max_speed; c->P.max_heading_change = p->max_heading_change;
    c->P.near_goal_threshold = p->near_goal_threshold; c->P.max_neighbors = p->max_neighbors; c->P.pad = 0; c->P.dt_nominal = p->dt_nominal;
    c->P.range_sq = sca_gm::g_pow2(c->P.neighbor_dist);                 // neighborDist ** 2 (scaPolicy.py:112): glibc's pow, restated
    c->P.cos_heading_thr = cos_threshold(p->max_heading_change);
    c->P_ctx = c->P;
    int ndev = 0;
    CHK(c, hipGetDeviceCount(&ndev));
    if (ndev <= 0) { c->err = "no HIP device: libsca_hip has no CPU path"; return SCA_ERR_HIP; }
    CHK(c, hipSetDevice(device));
    CHK(c, hipStreamCreateWithFlags(&c->stream_own, hipStreamNonBlocking));
    c->stream = c->stream_own;
    {
        hipDeviceProp_t prop;
        CHK(c, hipGetDeviceProperties(&prop, device));
        c->cus = std::max(1, prop.multiProcessorCount);
        c->simds = 4 * c->cus;
        tunables_from_env(c->tun, c->simds, TUN_AT_CREATE);
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_kd_lv_rank<false>, KD_LV_T, 0) == hipSuccess && per_cu > 0)
            c->kd_rank_capacity = per_cu * c->cus;
        else (void)hipGetLastError();
    }
    for (auto &e : c->ev) CHK(c, hipEventCreate(&e));
    CHK(c, hipEventCreateWithFlags(&c->kd_ev, hipEventDisableTiming));
    CHK(c, hipHostMalloc((void **)&c->kd_host_counts, sizeof(int) * (2 * KD_MAX_LEVELS + 3)));   // counts | nchunks
    const size_t N = (size_t)max_agents, M = (size_t)max_obstacles;
    DeviceView &d = c->d;
    int r = 0;
    r |= dalloc(c, &c->rec_own, N); d.rec = c->rec_own;
    r |= dalloc(c, &c->rec_new_own, N); d.rec_new = c->rec_new_own;
    r |= dalloc(c, &d.heading, 3 * N); r |= dalloc(c, &d.goal, 3 * N); r |= dalloc(c, &d.pref_speed, N);
    r |= dalloc(c, &d.vpref_ext, 3 * N); r |= dalloc(c, &d.total_dist, N); r |= dalloc(c, &d.max_run_dist, N);
    r |= dalloc(c, &d.step_num, N); r |= dalloc(c, &d.vpref_mode, N); r |= dalloc(c, &d.policy, N);
    r |= dalloc(c, &d.zaxis, N); r |= dalloc(c, &c->lp_list, N);
    r |= dalloc(c, &d.obs, M); r |= dalloc(c, &d.atree, 2 * N); r |= dalloc(c, &d.aperm, N);
    r |= dalloc(c, &d.obs_sorted, M); r |= dalloc(c, &d.awide, 2 * N); r |= dalloc(c, &d.owide, 2 * M);
    r |= dalloc(c, &d.otree, 2 * M); r |= dalloc(c, &d.operm, M);
    r |= dalloc(c, &d.nbr_n, N); r |= dalloc(c, &d.nbr_id, N * K_MAX); r |= dalloc(c, &d.nbr_dsq, N * K_MAX);
    r |= dalloc(c, &d.coll_new, N); r |= dalloc(c, &d.nbr_valid, N);
    r |= dalloc(c, &d.near_n, N); r |= dalloc(c, &d.near_id, N * NEAR_MAX);
    r |= dalloc(c, &d.action, N * 8); r |= dalloc(c, &d.vpref_used, 3 * N); r |= dalloc(c, &d.vpost, 3 * N);
    r |= dalloc(c, &d.fb_list, N); r |= dalloc(c, &d.fb_count, 1); r |= dalloc(c, &d.is_fb, N);
    { Prep *pp = nullptr; r |= dalloc(c, &pp, N); d.prep = pp; } r |= dalloc(c, &d.diag, N * 8);
    r |= dalloc(c, &d.status, N); r |= dalloc(c, &d.done_count, 256 * 32); r |= dalloc(c, &d.agent_steps, 256 * 16);
    r |= dalloc(c, &c->kd.kx, N); r |= dalloc(c, &c->kd.ky, N); r |= dalloc(c, &c->kd.kz, N);
    r |= dalloc(c, &c->kd.mr, N);
    d.kx = c->kd.kx; d.ky = c->kd.ky; d.kz = c->kd.kz;
    c->kd.job_cap = (int)(N / 64 + 64);
    r |= dalloc(c, &c->kd.jobs[0], (size_t)c->kd.job_cap); r |= dalloc(c, &c->kd.jobs[1], (size_t)c->kd.job_cap);
    r |= dalloc(c, &c->kd.small, N); r |= dalloc(c, &c->kd.counts, (size_t)2 * KD_MAX_LEVELS + 4); r |= dalloc(c, &c->kd.ticket, (size_t)KD_MAX_LEVELS + 1);   // counts | nchunks (one readback) | tail slot counter
    c->kd.chunk_cap = (int)(N / KD_CHUNK + N / KD_WAVE_FLOOR + 8);
    r |= dalloc(c, &c->kd.nbox, (size_t)2 * c->kd.job_cap * 6); r |= dalloc(c, &c->kd.nge, (size_t)2 * c->kd.job_cap);
    r |= dalloc(c, &c->kd.ps, N);
    r |= dalloc(c, &c->kd.cbox, (size_t)2 * c->kd.job_cap * 12); r |= dalloc(c, &c->kd.chain, (size_t)c->kd.chunk_cap);
    r |= dalloc(c, &c->kd.chunks[0], (size_t)c->kd.chunk_cap); r |= dalloc(c, &c->kd.chunks[1], (size_t)c->kd.chunk_cap);
    c->kd.nchunks = c->kd.counts ? c->kd.counts + KD_MAX_LEVELS + 2 : nullptr;
    {   // grid of SCA_NBR_GRID: at least two buckets per agent
        GridDev &g = c->grid;
        g.hbits = 10;
        while (((size_t)1 << g.hbits) < 2 * N) g.hbits++;
        const size_t H = (size_t)1 << g.hbits;
        r |= dalloc(c, &g.count, H); r |= dalloc(c, &g.range, H); r |= dalloc(c, &g.cursor, 1);
        r |= dalloc(c, &g.bucket, N); r |= dalloc(c, &g.slot, N);
        r |= dalloc(c, &g.gx, N); r |= dalloc(c, &g.gy, N); r |= dalloc(c, &g.gz, N);
        r |= dalloc(c, &g.gid, N); r |= dalloc(c, &g.gkey, N);
        g.skip_prep = 0;
        g.inv_cell = grid_inv_cell(c->P.neighbor_dist);
    }
    if (!r) {   // the root's accumulators start empty (every build's last kernel resets them for the next one)
        unsigned long long h[12];
        const double pinf = INFINITY, ninf = -INFINITY;
        unsigned long long kp, kn;
        { unsigned long long u; std::memcpy(&u, &pinf, 8); kp = (u >> 63) ? ~u : (u | 0x8000000000000000ull); }
        { unsigned long long u; std::memcpy(&u, &ninf, 8); kn = (u >> 63) ? ~u : (u | 0x8000000000000000ull); }
        for (int q = 0; q < 12; q++) h[q] = (q % 6) < 3 ? kp : kn;
        CHK(c, hipMemcpyAsync(c->kd.nbox, h, sizeof(unsigned long long) * 6, hipMemcpyHostToDevice, c->stream));
        CHK(c, hipMemcpyAsync(c->kd.cbox, h, sizeof(unsigned long long) * 12, hipMemcpyHostToDevice, c->stream));
        CHK(c, hipStreamSynchronize(c->stream));
    }
    if (r) return SCA_ERR_HIP;
    // candidate tables: [unit256 (768) | unit128 (384) | phi256 (256) | phi128 (128)]
    std::vector<double> tab(768 + 384 + 256 + 128);
    candidate_table_host(256, tab.data(), tab.data() + 768 + 384);
    candidate_table_host(128, tab.data() + 768, tab.data() + 768 + 384 + 256);
    // k_solve's posture pre-filter treats the table directions as unit vectors (|u|^2 = 1 inside its 1e-13 margin): make sure
    for (int set = 0; set < 2; set++) {
        const int nn = set ? 128 : 256;
        const double *u = tab.data() + (set ? 768 : 0);
        for (int i = 0; i < nn; i++) {
            const double n2 = u[i] * u[i] + u[nn + i] * u[nn + i] + u[2 * nn + i] * u[2 * nn + i];
            if (std::fabs(n2 - 1.0) > 1e-14) { c->err = "candidate table is not unit length"; return SCA_ERR_STATE; }
        }
    }
    if (dalloc(c, &c->tab, tab.size())) return SCA_ERR_HIP;
    CHK(c, hipMemcpyAsync(c->tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    d.unit256 = c->tab; d.unit128 = c->tab + 768; d.phi256 = c->tab + 768 + 384; d.phi128 = c->tab + 768 + 384 + 256;
    d.n = 0; d.m = 0; d.shard_begin = 0; d.shard_count = 0;
    return 0;
}

void sca_destroy(sca_ctx *c) {
    if (!c) return;
    DeviceView &d = c->d;
    if (c->stream_own) (void)hipStreamSynchronize(c->stream_own);
    if (c->comm) { (void)hipStreamSynchronize(c->stream); (void)g_rccl.CommDestroy(c->comm); c->comm = nullptr; }
    (void)tracker_free(c);
    (void)part_free(c);
    (void)missions_drop(c);                                            // (in front of the lists: tables with lists read the rows' lengths back once more)
    for (void *p : {(void *)c->path.off, (void *)c->path.pts, (void *)c->path.rem, (void *)c->path.now_goal, (void *)c->pslot_pts, (void *)c->pslot_len}) if (p) (void)hipFree(p);
    c->scenes.release();
    if (c->clear) { (void)hipFree(c->clear); c->clear = nullptr; }
    if (c->h_done) { (void)hipHostFree(c->h_done); c->h_done = nullptr; }
    if (c->hs_host) { (void)hipHostFree(c->hs_host); c->hs_host = nullptr; }
    if (c->hs_dev) { (void)hipFree(c->hs_dev); c->hs_dev = nullptr; }
    if (c->rsp_host) { (void)hipHostFree(c->rsp_host); c->rsp_host = nullptr; }
    if (c->rspa_host) { (void)hipHostFree(c->rspa_host); c->rspa_host = nullptr; }
    if (c->rspa_ap_new) { (void)hipFree(c->rspa_ap_new); (void)hipFree(c->rspa_nd_new); c->rspa_ap_new = nullptr; c->rspa_nd_new = nullptr; }
    if (c->fin_host) { (void)hipHostFree(c->fin_host); c->fin_host = nullptr; }
    if (c->fin_counts) { (void)hipFree(c->fin_counts); c->fin_counts = nullptr; }
    if (c->vac.dev) { (void)hipFree(c->vac.dev); c->vac.dev = nullptr; }
    if (c->vac.host) { (void)hipHostFree(c->vac.host); c->vac.host = nullptr; }
    if (c->spn_host) { (void)hipHostFree(c->spn_host); c->spn_host = nullptr; }
    if (c->spn_dev) { (void)hipFree(c->spn_dev); c->spn_dev = nullptr; }
    if (c->spn_partials) { (void)hipFree(c->spn_partials); c->spn_partials = nullptr; }
    if (c->cx_host) { (void)hipHostFree(c->cx_host); c->cx_host = nullptr; c->cx_bytes = 0; }
    if (c->ap_dev) { (void)hipFree(c->ap_dev); (void)hipFree(c->ap_nd); c->ap_dev = nullptr; c->ap_nd = nullptr; }
    void *ptrs[] = {c->rec_own, c->rec_new_own, d.heading, d.goal, d.pref_speed, d.vpref_ext, d.total_dist, d.max_run_dist,
                    d.step_num, d.vpref_mode, d.policy, d.zaxis, d.obs, d.obs_sorted, d.awide, d.owide, d.atree, d.aperm, d.otree, d.operm, d.nbr_n,
                    d.nbr_id, d.nbr_dsq, d.coll_new, d.nbr_valid, d.near_n, d.near_id, d.action, d.vpref_used, d.vpost, d.fb_list, d.fb_count, d.is_fb, d.prep, d.diag, d.status,
                    d.done_count, d.agent_steps, c->tab, c->kd.kx, c->kd.ky, c->kd.kz, c->kd.mr,
                    c->kd.jobs[0], c->kd.jobs[1], c->kd.small, c->kd.counts, c->kd.nbox, c->kd.nge, c->kd.ps, c->kd.cbox, c->kd.chain, c->kd.chunks[0], c->kd.chunks[1], d.hist,
                    c->grid.count, c->grid.range, c->grid.cursor, c->grid.bucket, c->grid.slot, c->grid.gx, c->grid.gy, c->grid.gz,
                    c->grid.gid, c->grid.gkey, c->lp_list, d.sw_slot, d.sw_surv, d.sw_n};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    for (auto &e : c->ev) if (e) (void)hipEventDestroy(e);
    for (auto *pool : {&c->pool, &c->pool_trk, &c->pool_xch, &c->pool_kd}) for (hipEvent_t e : *pool) (void)hipEventDestroy(e);
    c->au.release();
    if (c->d.kdq_stats) (void)hipFree(c->d.kdq_stats);
    if (c->kd_ev) (void)hipEventDestroy(c->kd_ev);
    if (c->kd_host_counts) (void)hipHostFree(c->kd_host_counts);
    if (c->stream_own) (void)hipStreamDestroy(c->stream_own);
    delete c;
}

static int scene_obstacles_drop(sca_ctx *c);
int sca_set_obstacles(sca_ctx *c, int m, const double *pos, const double *radius) {
    API_ENTER(c);
    ARG(c, m >= 0 && m <= c->max_m);
    ARG(c, m == 0 || (pos && radius));
    if (c->ms.gate.on) if (int r = missions_gate_partials(c, m)) return r;    // (a mission gate probes every obstacle: its partials follow the set, or the call is refused with nothing changed)
    if (int r = scene_obstacles_drop(c)) return r;                     // one shared set again (sca_set_scene_obstacles)
    c->m = m; c->d.m = m;
    c->max_obs_radius = 0;
    for (int i = 0; i < m; i++) c->max_obs_radius = std::max(c->max_obs_radius, radius[i]);
    if (m == 0) return 0;
    std::vector<ObsRec> h(m);
    for (int i = 0; i < m; i++) { h[i].px = pos[3 * i]; h[i].py = pos[3 * i + 1]; h[i].pz = pos[3 * i + 2]; h[i].radius = radius[i]; }
    std::vector<int32_t> perm(m);
    for (int i = 0; i < m; i++) perm[i] = i;                           // kdTree.py:51-52
    std::vector<KdNode> tree;
    kd_build_host(m, pos, perm.data(), tree);                          // mampenv.py:20, built once
    CHK(c, hipMemcpyAsync(c->d.obs, h.data(), sizeof(ObsRec) * m, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->d.operm, perm.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->d.otree, tree.data(), sizeof(KdNode) * (2 * m - 1), hipMemcpyHostToDevice, c->stream));
    std::vector<KdWide> wide;
    kd_widen_host(m, tree, wide);
    std::vector<ObsRec> sorted(m);
    for (int i = 0; i < m; i++) sorted[i] = h[perm[i]];
    CHK(c, hipMemcpyAsync(c->d.owide, wide.data(), sizeof(KdWide) * (2 * m - 1), hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->d.obs_sorted, sorted.data(), sizeof(ObsRec) * m, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

static int agent_params_clear(sca_ctx *c) {
    if (!c->ap_dev) return 0;
    CHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(c->ap_dev); (void)hipFree(c->ap_nd);
    c->ap_dev = nullptr; c->ap_nd = nullptr; c->d.ap = nullptr;
    c->P = c->P_ctx;
    c->grid.inv_cell = grid_inv_cell(c->P.neighbor_dist);
    if (c->trk_on) c->trk_view.nd_per_agent = nullptr;
    return 0;
}
// One agent's solver record from the per-agent arrays (sca_set_agent_params', sca_restart_scenes_attrs'): a NULL array stands for the
// context's value, so all NULL is the record Params stands for, cos_heading_thr as sca_create derived it; range_sq by libm's pow, the
// threshold by the host bisection, looked up first among the values met so far (few distinct ones).  The ranges are the caller's to check
// (restart_attr_solver_ok): cos_threshold ends for any input.
struct SolverArrays { const double *neighbor_dist; const int32_t *max_neighbors; const double *time_step, *time_horizon, *max_speed, *max_heading_change, *dt_nominal; };
using ThrCache = std::vector<std::pair<double, double>>;               // (max_heading_change, its cosine threshold)
static AgentPar agent_par_row(const Params &P, const SolverArrays &S, int r, ThrCache &thr_cache) {
    AgentPar a;
    a.neighbor_dist = S.neighbor_dist ? S.neighbor_dist[r] : P.neighbor_dist;
    a.time_step = S.time_step ? S.time_step[r] : P.time_step;
    a.time_horizon = S.time_horizon ? S.time_horizon[r] : P.time_horizon;
    a.max_speed = S.max_speed ? S.max_speed[r] : P.max_speed;
    a.dt_nominal = S.dt_nominal ? S.dt_nominal[r] : P.dt_nominal;
    a.max_neighbors = S.max_neighbors ? S.max_neighbors[r] : P.max_neighbors;
    a.pad = 0;
    a.range_sq = sca_gm::g_pow2(a.neighbor_dist);
    a.cos_heading_thr = P.cos_heading_thr;
    if (S.max_heading_change) {
        const double mhc = S.max_heading_change[r];
        bool hit = false;
        for (auto &e : thr_cache) if (e.first == mhc) { a.cos_heading_thr = e.second; hit = true; break; }
        if (!hit) { a.cos_heading_thr = cos_threshold(mhc); thr_cache.push_back({mhc, a.cos_heading_thr}); }
    }
    return a;
}
// The reference keeps maxNeighbors / neighborDist / timeStep / timeHorizon / maxSpeed / max_heading_change / dt_nominal on every Agent object
// (agent.py:24-41) and every policy reads its own agent's (scaPolicy.py:112, util.py:8,17, orca3dPolicyOfficial.py:44,98,108, agent.py:87-99,
// mampenv.py:90-92).  Arrays of n = the agents of sca_set_agents; a NULL array keeps the context's value for everybody; n = 0 (or all NULL)
// returns to one value per context.  The grid's cells are sized for the largest neighborDist, the collision reach for the largest step.
int sca_set_agent_params(sca_ctx *c, int n, const double *neighbor_dist, const int32_t *max_neighbors, const double *time_step,
                         const double *time_horizon, const double *max_speed, const double *max_heading_change, const double *dt_nominal) {
    API_ENTER(c);
    if (!c->agents_set) { c->err = "sca_set_agents first"; return SCA_ERR_STATE; }
    const bool any = neighbor_dist || max_neighbors || time_step || time_horizon || max_speed || max_heading_change || dt_nominal;
    // (with the cell-owner partition on: only while the grid's cell size stays what the slabs were cut with -- checked below)
    if (n == 0 || !any) {
        if (c->part_on && c->ap_dev && grid_inv_cell(c->P_ctx.neighbor_dist) != c->part.inv_cell) {
            c->err = "sca_set_agent_params: this would change the grid's cell size under the cell-owner partition's slabs: sca_partition_disable first"; return SCA_ERR_STATE;
        }
        return agent_params_clear(c);
    }
    ARG(c, n == c->n);
    std::vector<AgentPar> h((size_t)n);
    std::vector<double> nd((size_t)n);
    const SolverArrays S{neighbor_dist, max_neighbors, time_step, time_horizon, max_speed, max_heading_change, dt_nominal};
    ThrCache thr_cache;
    Params env = c->P_ctx;
    double nd_max = 0, ms_max = 0, dt_max = 0;
    for (int i = 0; i < n; i++) {
        const AgentPar a = agent_par_row(c->P_ctx, S, i, thr_cache);
        if (!restart_attr_solver_ok(a.neighbor_dist, a.max_neighbors, a.time_step, a.time_horizon, a.max_speed,
                                    max_heading_change ? max_heading_change[i] : c->P_ctx.max_heading_change, a.dt_nominal)) {
            c->err = "sca_set_agent_params: agent " + std::to_string(i) + " has an attribute out of range (see sca_params)";
            return SCA_ERR_ARG;
        }
        h[i] = a; nd[i] = a.neighbor_dist;
        nd_max = std::max(nd_max, a.neighbor_dist); ms_max = std::max(ms_max, a.max_speed); dt_max = std::max(dt_max, a.dt_nominal);
    }
    if (c->part_on && grid_inv_cell(nd_max) != c->part.inv_cell) {
        c->err = "sca_set_agent_params: the largest neighbor_dist would change the grid's cell size under the cell-owner partition's slabs: call it "
                 "before sca_partition_init (or sca_partition_disable first)";
        return SCA_ERR_STATE;
    }
    CHK(c, hipStreamSynchronize(c->stream));
    if (!c->ap_dev) { CHK(c, hipMalloc((void **)&c->ap_dev, sizeof(AgentPar) * (size_t)c->max_n)); CHK(c, hipMalloc((void **)&c->ap_nd, sizeof(double) * (size_t)c->max_n)); }
    CHK(c, hipMemcpy(c->ap_dev, h.data(), sizeof(AgentPar) * (size_t)n, hipMemcpyHostToDevice));
    CHK(c, hipMemcpy(c->ap_nd, nd.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    c->d.ap = c->ap_dev;
    // the context's own Params become the envelope: what sizes the grid's cells (largest range) and the collision reach (largest step)
    env.neighbor_dist = nd_max; env.max_speed = ms_max; env.dt_nominal = dt_max; env.range_sq = sca_gm::g_pow2(nd_max);
    c->P = env;
    c->grid.inv_cell = grid_inv_cell(c->P.neighbor_dist);
    if (c->trk_on) c->trk_view.nd_per_agent = c->ap_nd;
    c->near_valid = false;
    return 0;
}

static int scenes_clear(sca_ctx *c);
static void scene_harvest_clear_fresh(sca_ctx *c, int count, const int32_t *scene_ids);
// what works on whole id ranges, while a row of the plain context is vacant (sca_retire_agents): it works again once every row is occupied
static int vacancy_refuse(sca_ctx *c, const char *who) {
    if (!c->vac.on) return 0;
    c->err = std::string(who) + ": " + std::to_string(c->n - c->vac.m) + " of the context's rows are vacant (sca_retire_agents) -- the call works on the whole id range, "
             "which cannot say which rows are; admit every vacant row first (a respawn that names it)";
    return SCA_ERR_UNSUPPORTED;
}
// a whole-context state from outside while a scene is below its capacity (sca_restart_scenes_sized): the vacant rows are the library's
static int scenes_refuse_partial(sca_ctx *c, const char *who) {
    if (!c->scenes.on || !c->scenes.partial) return 0;
    c->err = std::string(who) + ": a scene holds fewer agents than its capacity (sca_restart_scenes_sized) -- the rows behind them are vacant, and a state "
             "for the whole range cannot say so; fill every slot to its capacity first";
    return SCA_ERR_UNSUPPORTED;
}
int sca_set_agents(sca_ctx *c, int n, const double *radius, const double *pref_speed, const double *goal,
                   const uint8_t *policy, const uint8_t *zaxis, const double *max_run_dist) {
    API_ENTER(c);
    ARG(c, n > 0 && n <= c->max_n);
    ARG(c, radius && pref_speed && goal && policy && max_run_dist);
    for (int i = 0; i < n; i++) ARG(c, policy[i] <= SCA_POLICY_RVO3D_DUBINS);        // (before anything of the previous set is torn down)
    if (c->d.hist) {                                                  // the log's pitch is n: a new agent set starts a new log
        CHK(c, hipStreamSynchronize(c->stream));
        CHK(c, hipFree(c->d.hist));
        c->d.hist = nullptr; c->d.hist_cap = 0; c->d.hist_row = 0;
    }
    if (int r = tracker_free(c)) return r;                            // the tracker records belong to the old agent set
    if (int r = agent_params_clear(c)) return r;                      // ... and so do the agents' own solver attributes
    if (int r = part_free(c)) return r;                               // ... and so do the partition's lists
    if (int r = paths_clear(c, false)) return r;                      // ... and so do the waypoint lists (vpref_mode is reset below)
    if (int r = scenes_clear(c)) return r;                            // ... and so do the scenes
    if (int r = clearance_drop(c)) return r;                          // ... and so do the closest-approach records
    if (int r = missions_drop(c)) return r;                           // ... and so do the mission tables
    c->vac.on = false; c->vac.m = 0; c->vac.h.clear();                // ... and so does every vacancy: the new set occupies all its rows
    if (c->comm && n % c->comm_nranks) { c->err = "agent count must be a multiple of the communicator's rank count"; return SCA_ERR_ARG; }
    c->n = n; c->d.n = n; c->d.shard_begin = 0; c->d.shard_count = n;
    if (c->comm) { c->d.shard_count = n / c->comm_nranks; c->d.shard_begin = c->comm_rank * c->d.shard_count; }
    c->h_rec.assign(n, PubRec{});
    c->max_radius = 0; c->max_pref_speed = 0;
    for (int i = 0; i < n; i++) {
        c->h_rec[i].radius = radius[i];
        c->max_radius = std::max(c->max_radius, radius[i]);
        c->max_pref_speed = std::max(c->max_pref_speed, pref_speed[i]);
    }
    c->h_policy.assign(policy, policy + n);
    c->h_lp_list.clear();
    for (int i = 0; i < n; i++) if (policy[i] == SCA_POLICY_ORCA3D_LP) c->h_lp_list.push_back(i);
    c->d.lp_kernel = 0;                                               // decided per pass from the shard's LP agent count
    if (!c->h_lp_list.empty())
        CHK(c, hipMemcpyAsync(c->lp_list, c->h_lp_list.data(), sizeof(int32_t) * c->h_lp_list.size(), hipMemcpyHostToDevice, c->stream));
    c->h_perm.resize(n);
    for (int i = 0; i < n; i++) c->h_perm[i] = i;                     // kdTree.py:43-45
    c->perm_on_device = false;
    std::vector<uint8_t> z(n, 0), mode(n, 0);
    if (zaxis) z.assign(zaxis, zaxis + n);
    CHK(c, hipMemcpyAsync(c->d.pref_speed, pref_speed, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->d.goal, goal, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->d.policy, policy, n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->d.zaxis, z.data(), n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->d.vpref_mode, mode.data(), n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->d.max_run_dist, max_run_dist, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemsetAsync(c->d.total_dist, 0, sizeof(double) * n, c->stream));
    CHK(c, hipMemsetAsync(c->d.step_num, 0, sizeof(int32_t) * n, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    c->agents_set = true; c->state_set = false; c->h_pos_valid = false;
    c->au.forget(); c->au.ran = false;
    return 0;
}

int sca_set_state(sca_ctx *c, const double *pos, const float *vel, const double *heading, const uint8_t *flags,
                  const double *total_dist, const int32_t *step_num) {
    API_ENTER(c);
    if (!c->agents_set) { c->err = "sca_set_agents first"; return SCA_ERR_STATE; }
    ARG(c, pos && vel && heading && flags);
    if (int r = scenes_refuse_partial(c, "sca_set_state")) return r;
    if (int r = vacancy_refuse(c, "sca_set_state")) return r;
    const int n = c->n;
    for (int i = 0; i < n; i++) {
        PubRec &r = c->h_rec[i];
        r.px = pos[3 * i]; r.py = pos[3 * i + 1]; r.pz = pos[3 * i + 2];
        r.vx = vel[3 * i]; r.vy = vel[3 * i + 1]; r.vz = vel[3 * i + 2];
        r.flags = flags[i];
    }
    c->h_pos.assign(pos, pos + 3 * (size_t)n);
    c->h_pos_valid = true;
    CHK(c, hipMemcpyAsync(c->d.rec, c->h_rec.data(), sizeof(PubRec) * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->d.heading, heading, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
    if (total_dist) CHK(c, hipMemcpyAsync(c->d.total_dist, total_dist, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    if (step_num) CHK(c, hipMemcpyAsync(c->d.step_num, step_num, sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    state_replaced(c);
    if (int r = missions_refresh_live(c)) return r;                       // (mission tables stay; which rows enter the next step running follows the new flags)
    if (int r = missions_gate_new_state(c)) return r;                     // (a gate: the rows that are unfinished now lose their pending mission)
    scene_harvest_clear_fresh(c, 0, nullptr);                             // (a state from outside: nothing that finished before it is reported after it)
    if (c->part_on) return part_classify(c);                              // a complete state again: ownership follows from it
    return 0;
}

static int fetch_records(sca_ctx *c) {
    CHK(c, hipMemcpyAsync(c->h_rec.data(), c->d.rec, sizeof(PubRec) * c->n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int sca_get_state(sca_ctx *c, double *pos, float *vel, double *heading, uint8_t *flags, double *total_dist,
                  int32_t *step_num) {
    API_ENTER(c);
    if (!c->state_set) { c->err = "no state"; return SCA_ERR_STATE; }
    const int n = c->n;
    if (int r = fetch_records(c)) return r;
    for (int i = 0; i < n; i++) {
        const PubRec &r = c->h_rec[i];
        if (pos) { pos[3 * i] = r.px; pos[3 * i + 1] = r.py; pos[3 * i + 2] = r.pz; }
        if (vel) { vel[3 * i] = r.vx; vel[3 * i + 1] = r.vy; vel[3 * i + 2] = r.vz; }
        if (flags) flags[i] = (uint8_t)r.flags;
    }
    if (heading) CHK(c, hipMemcpyAsync(heading, c->d.heading, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, c->stream));
    if (total_dist) CHK(c, hipMemcpyAsync(total_dist, c->d.total_dist, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    if (step_num) CHK(c, hipMemcpyAsync(step_num, c->d.step_num, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int sca_set_kd_perm(sca_ctx *c, const int32_t *perm) {
    API_ENTER(c);
    ARG(c, perm && c->agents_set);
    if (int r = scenes_refuse_partial(c, "sca_set_kd_perm")) return r;
    if (int r = vacancy_refuse(c, "sca_set_kd_perm")) return r;
    if (c->scenes.on) {
        const int at = scenes_perm_fault(c->scenes.v.nscenes, c->scenes.h_off.data(), perm);
        if (at >= 0) {
            c->err = "sca_set_kd_perm: position " + std::to_string(at) + " holds agent " + std::to_string(perm[at]) + ", which is not of that position's scene (sca_set_scenes)";
            return SCA_ERR_ARG;
        }
    }
    c->h_perm.assign(perm, perm + c->n);
    c->perm_on_device = false;
    return 0;
}
int sca_get_kd_perm(sca_ctx *c, int32_t *perm) {
    API_ENTER(c);
    ARG(c, perm && c->agents_set);
    if (c->perm_on_device) {
        CHK(c, hipMemcpyAsync(c->h_perm.data(), c->d.aperm, sizeof(int32_t) * c->n, hipMemcpyDeviceToHost, c->stream));
        CHK(c, hipStreamSynchronize(c->stream));
    }
    std::memcpy(perm, c->h_perm.data(), sizeof(int32_t) * c->n);
    return 0;
}

int sca_get_kd_tree(sca_ctx *c, double *tree_out) {
    API_ENTER(c);
    ARG(c, tree_out && c->agents_set);
    if (c->scenes.on) { c->err = "sca_get_kd_tree with scenes set (sca_set_scenes): the context holds a forest, one tree per scene"; return SCA_ERR_UNSUPPORTED; }
    if (int r = vacancy_refuse(c, "sca_get_kd_tree")) return r;
    const int n = c->n;
    std::vector<KdNode> t((size_t)2 * n, KdNode{});
    if (!c->perm_on_device) {
        // host-built tree: the node array itself was uploaded
        CHK(c, hipMemcpyAsync(t.data(), c->d.atree, sizeof(KdNode) * (2 * n - 1), hipMemcpyDeviceToHost, c->stream));
        CHK(c, hipStreamSynchronize(c->stream));
    } else {
        // device-built tree: the build only writes the query records (header + both children's boxes) and the root's
        // node; the node array of kdTree.py:14-21 is put together here
        std::vector<KdWide> w((size_t)2 * n);
        CHK(c, hipMemcpyAsync(w.data(), c->d.awide, sizeof(KdWide) * (2 * n - 1), hipMemcpyDeviceToHost, c->stream));
        CHK(c, hipMemcpyAsync(t.data(), c->d.atree, sizeof(KdNode), hipMemcpyDeviceToHost, c->stream));
        CHK(c, hipStreamSynchronize(c->stream));
        std::vector<int> st{0};
        while (!st.empty()) {
            const int i = st.back();
            st.pop_back();
            t[i].begin = w[i].begin; t[i].end = w[i].end; t[i].left = w[i].left; t[i].right = w[i].right;
            if (w[i].end - w[i].begin > MAX_LEAF) {
                const int ch[2] = {w[i].left, w[i].right};
                for (int sd = 0; sd < 2; sd++) {
                    if (ch[sd] <= i || ch[sd] >= 2 * n - 1) { c->err = "corrupt kd tree"; return SCA_ERR_STATE; }
                    for (int k = 0; k < 3; k++) { t[ch[sd]].mn[k] = w[i].bx[kdw_idx(sd, 0, k)]; t[ch[sd]].mx[k] = w[i].bx[kdw_idx(sd, 1, k)]; }
                    st.push_back(ch[sd]);
                }
            } else { t[i].left = 0; t[i].right = 0; }
        }
    }
    for (int i = 0; i < 2 * n - 1; i++) {
        double *o = tree_out + 10 * (size_t)i;
        o[0] = t[i].begin; o[1] = t[i].end; o[2] = t[i].left; o[3] = t[i].right;
        for (int k = 0; k < 3; k++) { o[4 + k] = t[i].mn[k]; o[7 + k] = t[i].mx[k]; }
    }
    return 0;
}

int sca_set_vpref(sca_ctx *c, const double *vpref, const uint8_t *mode) {
    API_ENTER(c);
    ARG(c, vpref && mode && c->agents_set);
    if (int r = missions_path_mirrors(c)) return r;                    // (tables with lists: which rows follow a list now is the device's to say)
    if (c->paths_on)
        for (int i = 0; i < c->n; i++)
            if (mode[i] && c->h_path_vpref[i]) {
                c->err = "sca_set_vpref: agent " + std::to_string(i) + " follows a waypoint list (sca_set_paths): its v_pref is its policy's, toward the waypoint";
                return SCA_ERR_ARG;
            }
    CHK(c, hipMemcpyAsync(c->d.vpref_ext, vpref, sizeof(double) * 3 * c->n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->d.vpref_mode, mode, c->n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- waypoint lists (Agent.path, agent.py:44; get_trajectory, e.g. rvo3dPolicy.py:71-85) ------------------------------------------------
// reset_mode: the straight-line agents that had a path take v_pref from their policy's own rule again (k_waypoint set vpref_mode = 1 for them)
static int paths_clear(sca_ctx *c, bool reset_mode) {
    if (!c->paths_on) return 0;
    if (int r = missions_path_mirrors(c)) return r;                    // (tables with lists: the rows that had a list are the device's to say)
    CHK(c, hipStreamSynchronize(c->stream));
    if (reset_mode && c->n > 0) {
        std::vector<uint8_t> mode((size_t)c->n);
        CHK(c, hipMemcpyAsync(mode.data(), c->d.vpref_mode, c->n, hipMemcpyDeviceToHost, c->stream));
        CHK(c, hipStreamSynchronize(c->stream));
        for (int i = 0; i < c->n; i++) if (c->h_path_vpref[i]) mode[i] = 0;
        CHK(c, hipMemcpyAsync(c->d.vpref_mode, mode.data(), c->n, hipMemcpyHostToDevice, c->stream));
        CHK(c, hipStreamSynchronize(c->stream));
    }
    c->paths_on = false;
    c->path_W = 0;
    c->h_path_off.clear(); c->h_path_vpref.clear(); c->h_path_len.clear();
    return 0;
}
// the cursors both forms of the lists share
static int paths_alloc_cursors(sca_ctx *c) {
    if (c->path.rem) return 0;
    CHK(c, hipMalloc((void **)&c->path.rem, sizeof(int32_t) * (size_t)c->max_n));
    CHK(c, hipMalloc((void **)&c->path.now_goal, sizeof(double) * 3 * (size_t)c->max_n));
    return 0;
}
int sca_set_paths(sca_ctx *c, int n, const int32_t *offsets, const double *points) {
    API_ENTER(c);
    if (!c->agents_set) { c->err = "sca_set_agents first"; return SCA_ERR_STATE; }
    if ((n == 0 || !offsets) && c->ms.on && c->ms.lists) return mission_refuse(c, "sca_set_paths", MSF_PATH_CLEAR, -1);
    if (n == 0 || !offsets) return paths_clear(c, true);
    // (lists for the whole id range would give a vacant row a list; in block form no vacant row could be admitted again.  Clearing stays legal)
    if (int r = vacancy_refuse(c, "sca_set_paths")) return r;
    if (int r = missions_standing(c, "sca_set_paths", MSF_PATHS)) return r;
    if (c->part_on) { c->err = "sca_set_paths under the cell-owner partition: path state does not migrate with the agents"; return SCA_ERR_UNSUPPORTED; }
    if (n != c->n) { c->err = "sca_set_paths: n = " + std::to_string(n) + " is not the agent count " + std::to_string(c->n); return SCA_ERR_ARG; }
    if (offsets[0] != 0) { c->err = "sca_set_paths: offsets[0] must be 0"; return SCA_ERR_ARG; }
    for (int i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) { c->err = "sca_set_paths: offsets decrease at agent " + std::to_string(i); return SCA_ERR_ARG; }
    const size_t total = (size_t)offsets[n];
    if (total > 0 && !points) { c->err = "sca_set_paths: points is NULL"; return SCA_ERR_ARG; }
    for (size_t k = 0; k < 3 * total; k++)
        if (!std::isfinite(points[k])) { c->err = "sca_set_paths: waypoint " + std::to_string(k / 3) + " is not finite"; return SCA_ERR_ARG; }
    std::vector<uint8_t> pol((size_t)n);
    CHK(c, hipStreamSynchronize(c->stream));
    CHK(c, hipMemcpyAsync(pol.data(), c->d.policy, n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    if (int r = paths_clear(c, true)) return r;
    PathView &w = c->path;
    if (!w.off) CHK(c, hipMalloc((void **)&w.off, sizeof(int32_t) * ((size_t)c->max_n + 1)));
    if (int r = paths_alloc_cursors(c)) return r;
    if (3 * total > c->path_pts_cap || !w.pts) {
        if (w.pts) { (void)hipFree((void *)w.pts); w.pts = nullptr; c->path_pts_cap = 0; }
        CHK(c, hipMalloc((void **)&w.pts, sizeof(double) * std::max<size_t>(3 * total, 3)));
        c->path_pts_cap = std::max<size_t>(3 * total, 3);
    }
    std::vector<int32_t> rem((size_t)n);
    for (int i = 0; i < n; i++) rem[i] = offsets[i + 1] - offsets[i];
    const std::vector<double> none(3 * (size_t)n, std::numeric_limits<double>::quiet_NaN());
    CHK(c, hipMemcpyAsync((void *)w.off, offsets, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream));
    if (total) CHK(c, hipMemcpyAsync((void *)w.pts, points, sizeof(double) * 3 * total, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(w.rem, rem.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(w.now_goal, none.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    c->h_path_off.assign(offsets, offsets + n + 1);
    c->h_path_vpref.assign((size_t)n, 0);
    for (int i = 0; i < n; i++)
        c->h_path_vpref[i] = rem[i] > 0 && pol[i] != SCA_POLICY_SCA && pol[i] != SCA_POLICY_RVO3D_DUBINS;
    c->paths_on = true;
    return 0;
}
// The lists in slot form (include/sca_hip.h): sca_set_paths' rules and refusals plus the room's (path_slots_check, sca_scenes.h).  The rows'
// rooms are uploaded as one block built on the host; room behind a list's length is never read (rem <= len).
int sca_set_path_slots(sca_ctx *c, int points_per_agent, int n, const int32_t *offsets, const double *points) {
    API_ENTER(c);
    const int W = points_per_agent;
    if (int r = vacancy_refuse(c, "sca_set_path_slots")) return r;      // (a vacant row's list is empty, and a list per row for the whole range cannot say so)
    if (W > 0) if (int r = missions_standing(c, "sca_set_path_slots", MSF_PATHS)) return r;    // (W <= 0 is path_slots_check's SCA_ERR_ARG, tables or not)
    const PathSlotCheck k = path_slots_check(c->agents_set, c->part_on, c->n, c->max_n, W, n, offsets, points);
    if (k.fault != PATH_SLOTS_OK) {
        const std::string at = std::to_string(k.entry);
        switch (k.fault) {
        case PATH_SLOTS_NO_AGENTS: c->err = "sca_set_agents first"; break;
        case PATH_SLOTS_PARTITION: c->err = "sca_set_path_slots under the cell-owner partition: path state does not migrate with the agents"; break;
        case PATH_SLOTS_BAD_N: c->err = "sca_set_path_slots: n = " + std::to_string(n) + " is not the agent count " + std::to_string(c->n); break;
        case PATH_SLOTS_BAD_W: c->err = "sca_set_path_slots: points_per_agent = " + std::to_string(W) + " must be at least 1"; break;
        case PATH_SLOTS_TOO_LARGE: c->err = "sca_set_path_slots: points_per_agent = " + std::to_string(W) + " x max_agents = " + std::to_string(c->max_n) + " points are not addressable (at most " +
                                            std::to_string(PATH_SLOT_POINTS_MAX) + ")"; break;
        case PATH_SLOTS_BAD_START: c->err = "sca_set_path_slots: offsets[0] must be 0"; break;
        case PATH_SLOTS_DECREASING: c->err = "sca_set_path_slots: offsets decrease at agent " + at; break;
        case PATH_SLOTS_TOO_LONG: c->err = "sca_set_path_slots: agent " + at + " has a list of " + std::to_string(offsets[k.entry + 1] - offsets[k.entry]) + " waypoints, its row has room for " + std::to_string(W); break;
        case PATH_SLOTS_NO_POINTS: c->err = "sca_set_path_slots: points is NULL"; break;
        default: c->err = "sca_set_path_slots: waypoint " + at + " is not finite";
        }
        return path_slots_error_code(k.fault);
    }
    std::vector<uint8_t> pol((size_t)n);
    CHK(c, hipStreamSynchronize(c->stream));
    CHK(c, hipMemcpyAsync(pol.data(), c->d.policy, n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    if (int r = paths_clear(c, true)) return r;
    if (int r = paths_alloc_cursors(c)) return r;
    const size_t room = (size_t)W * (size_t)c->max_n;
    if (room > c->pslot_cap || !c->pslot_pts) {
        if (c->pslot_pts) { (void)hipFree(c->pslot_pts); c->pslot_pts = nullptr; c->pslot_cap = 0; }
        CHK(c, hipMalloc((void **)&c->pslot_pts, sizeof(double) * 3 * room));
        c->pslot_cap = room;
        CHK(c, hipMemsetAsync(c->pslot_pts, 0, sizeof(double) * 3 * room, c->stream));
    }
    if (!c->pslot_len) CHK(c, hipMalloc((void **)&c->pslot_len, sizeof(int32_t) * (size_t)c->max_n));
    std::vector<int32_t> len((size_t)n, 0);
    std::vector<double> rooms(3 * (size_t)W * (size_t)n, 0.0);
    if (offsets)
        for (int i = 0; i < n; i++) {
            len[i] = offsets[i + 1] - offsets[i];
            if (len[i]) std::memcpy(rooms.data() + 3 * path_slot_index(W, i), points + 3 * (size_t)offsets[i], sizeof(double) * 3 * (size_t)len[i]);
        }
    const std::vector<double> none(3 * (size_t)n, std::numeric_limits<double>::quiet_NaN());
    if (k.total) CHK(c, hipMemcpyAsync(c->pslot_pts, rooms.data(), sizeof(double) * rooms.size(), hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->pslot_len, len.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->path.rem, len.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->path.now_goal, none.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    c->h_path_vpref.assign((size_t)n, 0);
    for (int i = 0; i < n; i++) c->h_path_vpref[i] = len[i] > 0 && pol[i] != SCA_POLICY_SCA && pol[i] != SCA_POLICY_RVO3D_DUBINS;
    c->h_path_len.swap(len);
    c->path_W = W;
    c->paths_on = true;
    return 0;
}
int sca_get_path_slots(sca_ctx *c, int *points_per_agent) {
    API_ENTER(c);
    ARG(c, points_per_agent);
    *points_per_agent = c->path_W;
    return 0;
}
int sca_get_path_state(sca_ctx *c, int32_t *remaining, double *now_goal) {
    API_ENTER(c);
    if (!c->paths_on) { c->err = "no waypoint lists (sca_set_paths)"; return SCA_ERR_STATE; }
    CHK(c, hipStreamSynchronize(c->stream));
    if (remaining) CHK(c, hipMemcpyAsync(remaining, c->path.rem, sizeof(int32_t) * c->n, hipMemcpyDeviceToHost, c->stream));
    if (now_goal) CHK(c, hipMemcpyAsync(now_goal, c->path.now_goal, sizeof(double) * 3 * c->n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
// read-only: the lists as the rows hold them in slot form -- the lengths as set (by sca_set_path_slots, a respawn, a restart or a take) and
// the rooms whole, W points per row (what stands behind a list's length is whatever an earlier list left there)
int sca_get_path_slot_lists(sca_ctx *c, int32_t *len, double *rooms) {
    API_ENTER(c);
    if (!c->paths_on || c->path_W <= 0) { c->err = "sca_get_path_slot_lists: the lists are not in slot form (sca_set_path_slots)"; return SCA_ERR_STATE; }
    ARG(c, len || rooms);
    CHK(c, hipStreamSynchronize(c->stream));
    if (len) CHK(c, hipMemcpyAsync(len, c->pslot_len, sizeof(int32_t) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
    if (rooms) CHK(c, hipMemcpyAsync(rooms, c->pslot_pts, sizeof(double) * 3 * (size_t)c->path_W * (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
// read-only: the rows' vpref_mode bytes as the next pass will read them (fed by sca_set_vpref, 1 where a pass aimed a straight-line row at
// its waypoint or the device tracker tracks the row, 0 behind a respawn or a take that reset it)
int sca_get_vpref_mode(sca_ctx *c, uint8_t *mode) {
    API_ENTER(c);
    ARG(c, mode && c->agents_set);
    CHK(c, hipStreamSynchronize(c->stream));
    CHK(c, hipMemcpyAsync(mode, c->d.vpref_mode, (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
int sca_set_path_state(sca_ctx *c, const int32_t *remaining, const double *now_goal) {
    API_ENTER(c);
    if (!c->paths_on) { c->err = "no waypoint lists (sca_set_paths)"; return SCA_ERR_STATE; }
    ARG(c, remaining && now_goal);
    if (int r = vacancy_refuse(c, "sca_set_path_state")) return r;      // (a vacant row's now_goal is None)
    if (int r = missions_path_mirrors(c)) return r;                    // (tables with lists: the bound is the device's lengths)
    const int n = c->n;
    for (int i = 0; i < n; i++) {
        if (remaining[i] < 0 || remaining[i] > (c->path_W ? c->h_path_len[i] : c->h_path_off[i + 1] - c->h_path_off[i])) {
            c->err = "sca_set_path_state: remaining[" + std::to_string(i) + "] is outside 0 .. the length of the agent's list"; return SCA_ERR_ARG;
        }
        const double *g = now_goal + 3 * (size_t)i;
        const bool none = std::isnan(g[0]) && std::isnan(g[1]) && std::isnan(g[2]);
        if (!none && !(std::isfinite(g[0]) && std::isfinite(g[1]) && std::isfinite(g[2]))) {
            c->err = "sca_set_path_state: now_goal of agent " + std::to_string(i) + " is neither finite nor all NaN (None)"; return SCA_ERR_ARG;
        }
    }
    CHK(c, hipStreamSynchronize(c->stream));
    CHK(c, hipMemcpyAsync(c->path.rem, remaining, sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->path.now_goal, now_goal, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- scene batches (sca_scenes.h: the rules; sca_scenes.hip.h: the kernels) -----------------------------------------------------------------
// The per-scene obstacle sets go with the scenes they were cut for -- and the context is left without obstacles: the shared set they
// replaced is not kept.
static int scene_obstacles_drop(sca_ctx *c) {
    if (!c->scenes.obs_on) return 0;
    CHK(c, hipStreamSynchronize(c->stream));
    if (c->scenes.ov.oroot) (void)hipFree((void *)c->scenes.ov.oroot);
    c->scenes.ov = SceneObsView{};
    c->scenes.h_obs_off.clear(); c->scenes.h_obs_count.clear();
    c->scenes.obs_on = false;
    c->m = 0; c->d.m = 0; c->max_obs_radius = 0;
    c->near_valid = false;
    return 0;
}
// ... and so does the log per scene: its layout is cut by the scenes' offsets
static int scene_log_drop(sca_ctx *c) {
    if (!c->scenes.log.rows) return 0;
    CHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(c->scenes.log.rows);
    c->scenes.log = SceneLogView{};
    return 0;
}
// ... and the harvest block: its places are cut by the scenes' offsets too
static int scene_harvest_drop(sca_ctx *c) {
    if (!c->scenes.hv_host) return 0;
    CHK(c, hipStreamSynchronize(c->stream));
    (void)hipHostFree(c->scenes.hv_host);
    c->scenes.hv_host = nullptr;
    return 0;
}
// ... and the closest-approach records: one per agent row of the scenes as they were cut
static int scene_clearance_drop(sca_ctx *c) {
    if (!c->scenes.clear) return 0;
    CHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(c->scenes.clear);
    c->scenes.clear = nullptr;
    return 0;
}
// the `fresh` words of the harvest, all of them or those of the named scenes.  Host stores into the block: only behind a synchronised
// stream, when no k_scene_harvest is in flight.
static void scene_harvest_clear_fresh(sca_ctx *c, int count, const int32_t *scene_ids) {
    if (!c->scenes.hv_host) return;
    sca_scene_summary *sum = (sca_scene_summary *)(c->scenes.hv_host + c->scenes.hv_layout.off[HV_SUMMARY]);
    if (scene_ids) for (int e = 0; e < count; e++) sum[scene_ids[e]].fresh = 0;
    else for (int s = 0; s < c->scenes.v.nscenes; s++) sum[s].fresh = 0;
}
static int scenes_clear(sca_ctx *c) {
    if (!c->scenes.on) return 0;
    if (int r = scene_obstacles_drop(c)) return r;
    if (int r = scene_log_drop(c)) return r;
    if (int r = scene_harvest_drop(c)) return r;
    if (int r = scene_clearance_drop(c)) return r;
    CHK(c, hipStreamSynchronize(c->stream));
    c->scenes.on = false;
    c->scenes.h_off.clear();
    c->scenes.h_size.clear(); c->scenes.partial = false;
    c->scenes.largest = 0; c->scenes.live_valid = false; c->scenes.begun = false;
    return 0;
}
int sca_set_scenes(sca_ctx *c, int nscenes, const int32_t *offsets) {
    API_ENTER(c);
    if (!c->agents_set) { c->err = "sca_set_agents first"; return SCA_ERR_STATE; }
    if (int r = vacancy_refuse(c, "sca_set_scenes")) return r;
    const int n = c->n;
    const SceneCheck k = scenes_check(n, nscenes, offsets);
    if (k.fault != SCENES_OK && k.fault != SCENES_NONE) {
        const std::string at = k.scene >= 0 ? " (scene " + std::to_string(k.scene) + ")" : "";
        switch (k.fault) {
        case SCENES_BAD_COUNT: c->err = "sca_set_scenes: nscenes must be 0 .. the agent count " + std::to_string(n); break;
        case SCENES_BAD_START: c->err = "sca_set_scenes: offsets[0] must be 0"; break;
        case SCENES_NOT_INCREASING: c->err = "sca_set_scenes: offsets must increase strictly -- no empty scene" + at; break;
        case SCENES_BAD_END: c->err = "sca_set_scenes: offsets[nscenes] must be the agent count " + std::to_string(n) + at; break;
        default: c->err = "sca_set_scenes: a scene of " + std::to_string(k.largest) + " agents" + at + ": a scene holds at most KD_WAVE_CAP = " + std::to_string(KD_WAVE_CAP) + " (its tree is one workgroup's)";
        }
        return scenes_error_code(k.fault);
    }
    if (k.fault == SCENES_NONE) return scenes_clear(c);
    if (int r = clearance_refuse(c, "sca_set_scenes", clearance_check(CLR_SET_SCENES, clearance_state(c), 0, 0, true, 0))) return r;
    if (int r = missions_standing(c, "sca_set_scenes", MSF_SCENES)) return r;
    if (c->comm) { c->err = "sca_set_scenes with an active communicator (sca_comm_init): scenes are one rank's"; return SCA_ERR_UNSUPPORTED; }
    if (c->part_on) { c->err = "sca_set_scenes under the cell-owner partition (sca_partition_init): a mode of SCA_NBR_GRID, which has no scene form"; return SCA_ERR_UNSUPPORTED; }
    if (c->d.shard_begin != 0 || c->d.shard_count != n) { c->err = "sca_set_scenes on a shard (sca_set_shard): scenes are stepped by one rank, whole"; return SCA_ERR_UNSUPPORTED; }
    CHK(c, hipStreamSynchronize(c->stream));
    if (int r = scene_obstacles_drop(c)) return r;                    // (cut for the scenes that go)
    c->scenes.release(); c->scenes.on = false;
    int32_t *so = nullptr, *off = nullptr;
    CHK(c, hipMalloc((void **)&so, sizeof(int32_t) * (size_t)n));
    c->scenes.v.scene_of = so;
    CHK(c, hipMalloc((void **)&off, sizeof(int32_t) * ((size_t)nscenes + 1)));
    c->scenes.v.offsets = off;
    const size_t words = (size_t)nscenes * (SCENE_LINE + 2);
    CHK(c, hipMalloc((void **)&c->scenes.counters, sizeof(int32_t) * words));
    c->scenes.v.live = c->scenes.counters; c->scenes.v.prev = c->scenes.counters + (size_t)nscenes * SCENE_LINE; c->scenes.v.steps = c->scenes.v.prev + nscenes;
    c->scenes.v.nscenes = nscenes;
    CHK(c, hipMalloc((void **)&c->scenes.v.heading_keep, sizeof(double) * 3 * (size_t)n));       // (written by k_scene_recount before any step reads it)
    CHK(c, hipMalloc((void **)&c->scenes.size, sizeof(int32_t) * (size_t)nscenes));
    std::vector<int32_t> full((size_t)nscenes);                      // every scene starts filled to its capacity
    for (int sc = 0; sc < nscenes; sc++) full[sc] = offsets[sc + 1] - offsets[sc];
    std::vector<int32_t> of((size_t)n);
    for (int sc = 0; sc < nscenes; sc++) for (int a = offsets[sc]; a < offsets[sc + 1]; a++) of[a] = sc;
    CHK(c, hipMemcpyAsync(so, of.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(off, offsets, sizeof(int32_t) * ((size_t)nscenes + 1), hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemsetAsync(c->scenes.counters, 0, sizeof(int32_t) * words, c->stream));
    CHK(c, hipMemcpyAsync(c->scenes.size, full.data(), sizeof(int32_t) * (size_t)nscenes, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    c->scenes.h_off.assign(offsets, offsets + nscenes + 1);
    c->scenes.h_size.swap(full); c->scenes.partial = false;
    c->scenes.largest = k.largest;
    for (int i = 0; i < n; i++) c->h_perm[i] = i;                     // every scene's kdTree.agentIDs starts as 0 .. n_s - 1 (kdTree.py:43-45)
    c->perm_on_device = false;
    c->scenes.live_valid = false; c->scenes.begun = false;
    positions_replaced(c); c->au.forget(); c->near_valid = false;      // (not state_replaced: no state arrived, state_set and state_fresh stay as they are)
    c->nbr_mode = SCA_NBR_KDTREE;
    c->scenes.on = true;
    return 0;
}
// One scene's part of the obstacle forest, by the routine sca_set_obstacles uses on that scene's `ms` obstacles alone with local ids, as
// it stands at obstacle base `lo` (scene_obstacle_shift): sca_set_scene_obstacles, sca_set_scene_obstacle_slots and the restart that
// brings obstacles all build through here, into the forest's arrays or into the restart's staging block.  rec / sorted / perm: [ms];
// tree / wide: [2 ms - 1], to stand at record 2 * lo.  perm carries global ids (lo + local), as the agents' permutation does.
static void scene_obstacle_build(int lo, int ms, const double *pos, const double *radius, ObsRec *rec, ObsRec *sorted, int32_t *perm, KdNode *tree_out, KdWide *wide_out) {
    if (ms <= 0) return;
    std::vector<KdNode> tree;
    std::vector<KdWide> wide;
    std::vector<int32_t> local((size_t)ms);
    for (int i = 0; i < ms; i++) { rec[i].px = pos[3 * i]; rec[i].py = pos[3 * i + 1]; rec[i].pz = pos[3 * i + 2]; rec[i].radius = radius[i]; }
    for (int i = 0; i < ms; i++) local[i] = i;                         // kdTree.py:51-52, the scene's own ids
    kd_build_host(ms, pos, local.data(), tree);
    kd_widen_host(ms, tree, wide);
    scene_obstacle_shift(tree.data(), 2 * ms - 1, lo, MAX_LEAF);
    scene_obstacle_shift(wide.data(), 2 * ms - 1, lo, MAX_LEAF);
    for (int i = 0; i < 2 * ms - 1; i++) { tree_out[i] = tree[i]; wide_out[i] = wide[i]; }
    for (int i = 0; i < ms; i++) { perm[i] = lo + local[i]; sorted[i] = rec[local[i]]; }
}
// The whole forest from the host: scene sc owns rows [off[sc], off[sc + 1]) and holds counts[sc] obstacles in the first of them (NULL:
// every range is full); pos / radius are packed densely in scene order.  The arguments are checked, the stream is synchronised.
static int scene_obstacles_install(sca_ctx *c, const int32_t *off, const int32_t *counts, const double *pos, const double *radius) {
    const int B = c->scenes.v.nscenes, M = off[B];
    std::vector<ObsRec> h((size_t)M, ObsRec{}), sorted((size_t)M, ObsRec{});
    std::vector<int32_t> perm((size_t)M, 0), roots(2 * (size_t)B);    // roots | counts, one upload
    std::vector<KdNode> forest(2 * (size_t)M, KdNode{});
    std::vector<KdWide> wforest(2 * (size_t)M, KdWide{});
    double max_r = 0;
    size_t at = 0;
    for (int sc = 0; sc < B; sc++) {
        const int lo = off[sc], ms = counts ? counts[sc] : off[sc + 1] - lo;
        roots[sc] = ms > 0 ? 2 * lo : -1;                              // (scene_obstacle_root / obstacle_slot_root)
        roots[(size_t)B + sc] = ms;
        scene_obstacle_build(lo, ms, pos + 3 * at, radius + at, h.data() + lo, sorted.data() + lo, perm.data() + lo, forest.data() + 2 * (size_t)lo, wforest.data() + 2 * (size_t)lo);
        for (int i = 0; i < ms; i++) max_r = std::max(max_r, radius[at + i]);
        at += (size_t)ms;
    }
    int32_t *dr = nullptr;
    CHK(c, hipMalloc((void **)&dr, sizeof(int32_t) * 2 * (size_t)B));
    if (c->scenes.ov.oroot) (void)hipFree((void *)c->scenes.ov.oroot);
    c->scenes.ov.oroot = dr;
    CHK(c, hipMemcpyAsync(dr, roots.data(), sizeof(int32_t) * 2 * (size_t)B, hipMemcpyHostToDevice, c->stream));
    if (M > 0) {
        CHK(c, hipMemcpyAsync(c->d.obs, h.data(), sizeof(ObsRec) * (size_t)M, hipMemcpyHostToDevice, c->stream));
        CHK(c, hipMemcpyAsync(c->d.operm, perm.data(), sizeof(int32_t) * (size_t)M, hipMemcpyHostToDevice, c->stream));
        CHK(c, hipMemcpyAsync(c->d.otree, forest.data(), sizeof(KdNode) * 2 * (size_t)M, hipMemcpyHostToDevice, c->stream));
        CHK(c, hipMemcpyAsync(c->d.owide, wforest.data(), sizeof(KdWide) * 2 * (size_t)M, hipMemcpyHostToDevice, c->stream));
        CHK(c, hipMemcpyAsync(c->d.obs_sorted, sorted.data(), sizeof(ObsRec) * (size_t)M, hipMemcpyHostToDevice, c->stream));
    }
    CHK(c, hipStreamSynchronize(c->stream));
    c->m = M; c->d.m = M; c->max_obs_radius = max_r;
    c->scenes.h_obs_off.assign(off, off + B + 1);
    c->scenes.h_obs_count.assign(roots.begin() + B, roots.end());
    c->near_valid = false;
    c->scenes.obs_on = true;
    return 0;
}
// One obstacle set per scene.  The reference builds a scene's obstacle tree once, over its own obstacles (mampenv.py:20, kdTree.py:162-227):
// here the same routine runs per scene on that scene's obstacles alone, with local ids -- so the tree, the leaf order and with them every
// list and every distSq are the single-scene context's -- and the trees are laid side by side (scene_obstacle_shift, sca_scenes.h).
// max_obs_radius, and with it the collision reach, stays one value per context: a conservative filter, as max_radius is for scenes.
int sca_set_scene_obstacles(sca_ctx *c, int nscenes, const int32_t *obs_offsets, const double *pos, const double *radius) {
    API_ENTER(c);
    if (!c->scenes.on) { c->err = "sca_set_scene_obstacles: no scenes -- sca_set_scenes first"; return SCA_ERR_STATE; }
    const int B = c->scenes.v.nscenes;
    const SceneObsCheck k = scene_obstacles_check(B, c->max_m, nscenes, obs_offsets, pos != nullptr, radius != nullptr);
    if (k.fault != SCENE_OBS_OK) {
        switch (k.fault) {
        case SCENE_OBS_BAD_COUNT: c->err = "sca_set_scene_obstacles: nscenes = " + std::to_string(nscenes) + ", the context holds " + std::to_string(B) + " scenes (sca_set_scenes)"; break;
        case SCENE_OBS_NO_OFFSETS: c->err = "sca_set_scene_obstacles: obs_offsets is NULL"; break;
        case SCENE_OBS_BAD_START: c->err = "sca_set_scene_obstacles: obs_offsets[0] must be 0"; break;
        case SCENE_OBS_DECREASING: c->err = "sca_set_scene_obstacles: obs_offsets must not decrease (scene " + std::to_string(k.scene) + ")"; break;
        case SCENE_OBS_TOO_MANY: c->err = "sca_set_scene_obstacles: " + std::to_string(k.total) + " obstacles in all, sca_create's max_obstacles is " + std::to_string(c->max_m); break;
        default: c->err = "sca_set_scene_obstacles: pos and radius must not be NULL with " + std::to_string(k.total) + " obstacles";
        }
        return scene_obstacles_error_code(k.fault);
    }
    const int M = k.total;
    CHK(c, hipStreamSynchronize(c->stream));
    if (M == 0) {                                                     // "no obstacles": the forms of a context without any
        if (int r = scene_obstacles_drop(c)) return r;
        c->m = 0; c->d.m = 0; c->max_obs_radius = 0; c->near_valid = false;
        return 0;
    }
    return scene_obstacles_install(c, obs_offsets, nullptr, pos, radius);
}
// Obstacle slots (include/sca_hip.h): the same forest with every scene's range a capacity.  The rules are obstacle_slots_check's.
int sca_set_scene_obstacle_slots(sca_ctx *c, int nscenes, const int32_t *cap_offsets, const int32_t *counts, const double *pos, const double *radius) {
    API_ENTER(c);
    if (!c->scenes.on) { c->err = "sca_set_scene_obstacle_slots: no scenes -- sca_set_scenes first"; return SCA_ERR_STATE; }
    const int B = c->scenes.v.nscenes;
    const ObsSlotCheck k = obstacle_slots_check(B, c->max_m, nscenes, cap_offsets, counts, pos, radius);
    if (k.fault != OBS_SLOT_OK) {
        const std::string sc = std::to_string(k.scene), row = std::to_string(k.row);
        switch (k.fault) {
        case OBS_SLOT_OFFSETS:
            switch (k.offsets) {
            case SCENE_OBS_BAD_COUNT: c->err = "sca_set_scene_obstacle_slots: nscenes = " + std::to_string(nscenes) + ", the context holds " + std::to_string(B) + " scenes (sca_set_scenes)"; break;
            case SCENE_OBS_NO_OFFSETS: c->err = "sca_set_scene_obstacle_slots: cap_offsets is NULL"; break;
            case SCENE_OBS_BAD_START: c->err = "sca_set_scene_obstacle_slots: cap_offsets[0] must be 0"; break;
            case SCENE_OBS_DECREASING: c->err = "sca_set_scene_obstacle_slots: cap_offsets must not decrease (scene " + sc + ")"; break;
            default: c->err = "sca_set_scene_obstacle_slots: a capacity of " + std::to_string(k.capacity) + " obstacles in all, sca_create's max_obstacles is " + std::to_string(c->max_m);
            }
            break;
        case OBS_SLOT_BAD_COUNT: c->err = "sca_set_scene_obstacle_slots: counts[" + sc + "] = " + std::to_string(counts[k.scene]) + ": the slot holds 0 .. " +
                                          std::to_string(cap_offsets[k.scene + 1] - cap_offsets[k.scene]) + " obstacles (its capacity)"; break;
        case OBS_SLOT_NO_ARRAYS: c->err = "sca_set_scene_obstacle_slots: pos and radius must not be NULL with " + std::to_string(k.total) + " obstacles"; break;
        case OBS_SLOT_NOT_FINITE: c->err = "sca_set_scene_obstacle_slots: obstacle row " + row + " (scene " + sc + ") has a position that is not finite"; break;
        default: c->err = "sca_set_scene_obstacle_slots: obstacle row " + row + " (scene " + sc + ") has a radius that is not positive";
        }
        return obstacle_slots_error_code(k.fault);
    }
    CHK(c, hipStreamSynchronize(c->stream));
    const std::vector<int32_t> none((size_t)B, 0);
    return scene_obstacles_install(c, cap_offsets, counts ? counts : none.data(), pos, radius);
}
int sca_get_scene_obstacle_counts(sca_ctx *c, int32_t *counts, int32_t *capacities) {
    API_ENTER(c);
    if (!c->scenes.on) { c->err = "sca_get_scene_obstacle_counts: no scenes (sca_set_scenes)"; return SCA_ERR_STATE; }
    if (!c->scenes.obs_on) { c->err = "sca_get_scene_obstacle_counts: no obstacle set per scene (sca_set_scene_obstacle_slots, sca_set_scene_obstacles)"; return SCA_ERR_STATE; }
    for (int sc = 0; sc < c->scenes.v.nscenes; sc++) {
        if (counts) counts[sc] = c->scenes.h_obs_count[sc];
        if (capacities) capacities[sc] = c->scenes.h_obs_off[sc + 1] - c->scenes.h_obs_off[sc];
    }
    return 0;
}
// SceneView::live from the records, where the state came from outside since the last env update (on `s`, which the records are final on)
static int scenes_recount(sca_ctx *c, hipStream_t s) {
    if (c->scenes.live_valid) return 0;
    hipLaunchKernelGGL(k_scene_recount, dim3((c->scenes.v.nscenes + 3) / 4), dim3(256), 0, s, c->d, c->scenes.v);
    CHK(c, hipGetLastError());
    c->scenes.live_valid = true;
    return 0;
}
int sca_get_scene_state(sca_ctx *c, int32_t *active, int32_t *steps) {
    API_ENTER(c);
    if (!c->scenes.on) { c->err = "no scenes (sca_set_scenes)"; return SCA_ERR_STATE; }
    if (!c->state_set) { c->err = "sca_set_state first"; return SCA_ERR_STATE; }
    const int B = c->scenes.v.nscenes;
    if (!c->scenes.begun) { if (int r = scenes_recount(c, c->stream)) return r; }
    std::vector<int32_t> h((size_t)B * (SCENE_LINE + 2));
    CHK(c, hipMemcpyAsync(h.data(), c->scenes.counters, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    // (between a policy pass and its env update the step under way has emptied `live`: what it found is in `prev`)
    if (active) for (int sc = 0; sc < B; sc++) active[sc] = c->scenes.begun ? h[(size_t)B * SCENE_LINE + sc] : h[(size_t)sc * SCENE_LINE];
    if (steps) for (int sc = 0; sc < B; sc++) steps[sc] = h[(size_t)B * (SCENE_LINE + 1) + sc];
    return 0;
}

// A new episode into a slot while the other slots keep running (include/sca_hip.h).  The rules are scene_restart_check's (sca_scenes.h); the
// caller's arrays are copied into the page-locked staging block, ONE launch of k_scene_restart (a workgroup per named scene) reads it across
// the link and writes every per-agent array of the named scenes, and the call's one synchronisation follows that launch: the block may be
// written again when the call returns.  Nothing context-wide is reset -- see DESIGN.md section 5 for trk.parity, trk_passes, kd_single_hint
// and state_fresh.
// sizes (sca_restart_scenes_sized): the rows each named scene brings, NULL: its capacity.  The kernel also vacates the rows behind the
// episode and writes the device's size[s]: for a scene that fills its capacity an empty range and the value it holds.
// obs_counts (sca_restart_scenes_obstacles): per named scene -1, the slot keeps its obstacle set, or 0 .. its obstacle capacity, the set is
// replaced by the next rows of obs_pos / obs_radius (restart_obstacles_check).  The named scenes' trees are built here, by the routine that
// built the forest (scene_obstacle_build), straight into the block's obstacle sections, and the kernel copies them to the scene's place
// and rewrites its root.  Every named scene gets its head words on every call: count -1 -- NULL, or the entry says so -- and the kernel
// returns behind the scene's agent rows.  So the three entry points are one launch of one kernel, and the two narrower ones its
// degenerate cases.
// The stages, in the order restart_scenes() runs them: the four checks (sca_scenes.h; their texts and restart_pack are sca_scene_restart.h's),
// restart_block, restart_pack with restart_pack_obstacles and restart_pack_attrs, restart_first_use, restart_launch, the copies behind
// the launch, the synchronisation, restart_commit.
static int restart_refuse(sca_ctx *c, const std::string &text, int code) { c->err = text; return code; }
// the staging block of at least `bytes`: mapped and coherent, as the host state block is -- the kernel reads it in place
static int restart_block(sca_ctx *c, size_t bytes) {
    if (c->scenes.rs_host && c->scenes.rs_bytes < bytes) {                       // the slot form, or a larger room per row, arrived behind the first restart: the
        CHK(c, hipStreamSynchronize(c->stream));                                 // block grows (every call ends with its synchronisation: no launch still reads it)
        (void)hipHostFree(c->scenes.rs_host);
        c->scenes.rs_host = nullptr; c->scenes.rs_bytes = 0;
    }
    if (!c->scenes.rs_host) {
        CHK(c, hipHostMalloc((void **)&c->scenes.rs_host, bytes, hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(c->scenes.rs_host, 0, bytes);
        c->scenes.rs_bytes = bytes;
    }
    return 0;
}
// the replaced scenes' trees, built where the kernel reads them, at the places restart_pack's head words name
static void restart_pack_obstacles(uint8_t *b, const RestartObsLayout &OL, const RestartArgs &A, RestartPlan &plan) {
    const int32_t *head = (const int32_t *)(b + OL.off[RO_HEAD]);
    ObsRec *rec = (ObsRec *)(b + OL.off[RO_REC]), *sorted = (ObsRec *)(b + OL.off[RO_SORTED]);
    int32_t *perm = (int32_t *)(b + OL.off[RO_PERM]);
    KdNode *tree = (KdNode *)(b + OL.off[RO_TREE]);
    KdWide *wide = (KdWide *)(b + OL.off[RO_WIDE]);
    for (int e = 0; e < A.count; e++) {
        const int ms = head[RO_HEAD_WORDS * e], base = head[RO_HEAD_WORDS * e + 1], at = head[RO_HEAD_WORDS * e + 2];
        if (ms <= 0) continue;
        scene_obstacle_build(base, ms, A.obs_pos + 3 * (size_t)at, A.obs_radius + at, rec + at, sorted + at, perm + at, tree + 2 * (size_t)at, wide + 2 * (size_t)at);
        for (int i = 0; i < ms; i++) plan.obs_max_radius = std::max(plan.obs_max_radius, A.obs_radius[at + i]);
    }
}
// ---- the episodes' attributes (sca_restart_scenes_attrs) ----
// Solver attributes travel when the call names any, or when the context carries per-agent arrays already (a NULL array then means the
// context's value, which the rows must take); planner attributes likewise, with a tracker.  A context without per-agent arrays whose
// call names none has nothing to write: every row computes from Params / the view's scalars, which ARE the context's values.
// The planner's per-row triples and the classes are worked out on the plan's copies, which replace the context's in restart_commit.
static void restart_pack_attrs(const sca_ctx *c, uint8_t *b, const RestartBlock &B, const RestartArgs &A, bool attrs, const RestartAttrs &RA, RestartPlan &plan) {
    const int n_all = c->n, count = A.count;
    const int32_t *off = c->scenes.h_off.data(), *start = (const int32_t *)(b + B.L.off[RS_START]), *new_size = (const int32_t *)(b + B.new_size_off);
    const uint8_t *pol = b + B.L.off[RS_POLICY];
    plan.send_solver = attrs && (RA.solver() || c->ap_dev);
    plan.send_planner = attrs && c->trk_on && (RA.planner() || c->trk_attr_on || c->trk_view.R_pa);
    plan.ap_first = plan.send_solver && !c->ap_dev;
    if (plan.send_solver) {
        AgentPar *par = (AgentPar *)(b + B.AL.off[RA_PAR]);
        double *ndv = (double *)(b + B.AL.off[RA_ND]);
        const SolverArrays S{RA.neighbor_dist, RA.max_neighbors, RA.time_step, RA.time_horizon, RA.max_speed, RA.max_heading_change, RA.dt_nominal};
        ThrCache thr_cache;
        for (int r = 0; r < plan.T; r++) {
            const AgentPar a = agent_par_row(c->P_ctx, S, r, thr_cache);
            par[r] = a; ndv[r] = a.neighbor_dist;
            plan.env_nd = std::max(plan.env_nd, a.neighbor_dist); plan.env_ms = std::max(plan.env_ms, a.max_speed); plan.env_dt = std::max(plan.env_dt, a.dt_nominal);
        }
        plan.has |= RESTART_HAS_ATTRS;
    }
    plan.table_new = c->trk_table;
    plan.table_on = plan.send_planner || (c->trk_on && c->trk_attr_on);          // (a call without `attrs` still changes which rows are occupied)
    if (!plan.table_on) return;
    const TrackTriple def{c->trk_enable_vals[0], c->trk_enable_vals[1], c->trk_enable_vals[2]};
    plan.trip_new = c->h_trk_trip; plan.cls_new = c->h_trk_cls;
    plan.trip_new.resize((size_t)n_all, def); plan.cls_new.resize((size_t)n_all, 0);
    std::vector<uint8_t> pol_after = c->h_policy, travels((size_t)n_all, 0);
    double *trip = (double *)(b + B.AL.off[RA_TRIPLE]);
    for (int e = 0; e < count; e++)
        for (int a = off[A.scene_ids[e]], r = start[e]; a < off[A.scene_ids[e]] + new_size[e]; a++, r++) {
            pol_after[a] = pol[r];
            if (!plan.send_planner) continue;
            plan.trip_new[a] = TrackTriple{RA.turning_radius ? RA.turning_radius[r] : def.R, RA.pitch_lo ? RA.pitch_lo[r] : def.lo, RA.pitch_hi ? RA.pitch_hi[r] : def.hi};
            trip[3 * r] = plan.trip_new[a].R; trip[3 * r + 1] = plan.trip_new[a].lo; trip[3 * r + 2] = plan.trip_new[a].hi;
            travels[a] = 1;
        }
    if (!c->trk_attr_on) plan.table_new.many = true;                  // first use: whatever classes an earlier call dealt, the table starts afresh
    plan.cu = scene_class_table(plan.table_new, c->scenes.v.nscenes, off, plan.size_now.data(), pol_after.data(), plan.trip_new.data(), plan.cls_new.data(), travels.data());
    plan.cls_whole = plan.cu.moved || !c->trk_attr_on;                // (first use: the device's bytes are an earlier call's, or none)
    if (plan.send_planner) {
        uint8_t *cl = b + B.AL.off[RA_CLASS];
        for (int e = 0; e < count; e++)
            for (int a = off[A.scene_ids[e]], r = start[e]; a < off[A.scene_ids[e]] + new_size[e]; a++, r++) cl[r] = plan.cls_new[a];
        plan.has |= RESTART_HAS_PLANNER;
    }
}
// what the first-use fills are copied from: alive until the call's synchronisation
struct RestartFills { std::vector<AgentPar> ap; std::vector<double> nd, trk[3]; };
// The first call that sends solver attributes, and the first that deals classes, allocate the per-row arrays and fill them for EVERY row
// with the context's own values, enqueued in front of the launch (which overwrites the rows of this call).
static int restart_first_use(sca_ctx *c, const RestartPlan &plan, RestartFills &F) {
    if (plan.ap_first) {
        // From here on every agent of the context reads d.ap[a] instead of Params: the rows of the scenes that are not named get the
        // record Params stands for -- range_sq and cos_heading_thr as sca_create derived them -- and so compute the bits they computed
        // before.  d.ap / nd_per_agent point at the arrays only in restart_commit.
        ThrCache none;
        const AgentPar a0 = agent_par_row(c->P_ctx, SolverArrays{}, 0, none);
        F.ap.assign((size_t)c->max_n, a0); F.nd.assign((size_t)c->max_n, a0.neighbor_dist);
        CHK(c, hipMalloc((void **)&c->ap_dev, sizeof(AgentPar) * (size_t)c->max_n));
        CHK(c, hipMalloc((void **)&c->ap_nd, sizeof(double) * (size_t)c->max_n));
        CHK(c, hipMemcpyAsync(c->ap_dev, F.ap.data(), sizeof(AgentPar) * (size_t)c->max_n, hipMemcpyHostToDevice, c->stream));
        CHK(c, hipMemcpyAsync(c->ap_nd, F.nd.data(), sizeof(double) * (size_t)c->max_n, hipMemcpyHostToDevice, c->stream));
    }
    if (plan.table_on && !c->trk_attr_on) {
        // the four per-row arrays exist from here on and are current for EVERY row -- the per-agent form (more classes than launches are
        // worth) reads them the moment the count passes the cap
        const size_t n_all = (size_t)c->n;
        if (!c->trk_R_pa) { CHK(c, hipMalloc((void **)&c->trk_R_pa, sizeof(double) * (size_t)c->max_n)); CHK(c, hipMalloc((void **)&c->trk_cls, (size_t)c->max_n)); }
        if (!c->trk_plo_pa) {
            CHK(c, hipMalloc((void **)&c->trk_plo_pa, sizeof(double) * (size_t)c->max_n));
            CHK(c, hipMalloc((void **)&c->trk_phi_pa, sizeof(double) * (size_t)c->max_n));
        }
        for (auto &v : F.trk) v.resize(n_all);
        for (size_t a = 0; a < n_all; a++) {
            const TrackTriple &x = plan.trip_new[a];
            F.trk[0][a] = x.R; F.trk[1][a] = x.lo; F.trk[2][a] = x.hi;
        }
        CHK(c, hipMemcpyAsync(c->trk_R_pa, F.trk[0].data(), sizeof(double) * n_all, hipMemcpyHostToDevice, c->stream));
        CHK(c, hipMemcpyAsync(c->trk_plo_pa, F.trk[1].data(), sizeof(double) * n_all, hipMemcpyHostToDevice, c->stream));
        CHK(c, hipMemcpyAsync(c->trk_phi_pa, F.trk[2].data(), sizeof(double) * n_all, hipMemcpyHostToDevice, c->stream));
    }
    return 0;
}
// ONE launch of k_scene_restart, a workgroup per named scene, over the block
static int restart_launch(sca_ctx *c, int count, const RestartBlock &B, uint32_t has) {
    const uint8_t *b = c->scenes.rs_host;
    RestartAttrDev at_dev{c->ap_dev, c->ap_nd, c->trk_R_pa, c->trk_plo_pa, c->trk_phi_pa, c->trk_cls};
    RestartDev d{};
    d.rec = c->d.rec;
    d.heading = c->d.heading; d.heading_keep = c->scenes.v.heading_keep; d.total_dist = c->d.total_dist; d.goal = c->d.goal;
    d.pref_speed = c->d.pref_speed; d.max_run_dist = c->d.max_run_dist; d.vpref_ext = c->d.vpref_ext; d.step_num = c->d.step_num;
    d.policy = c->d.policy; d.zaxis = c->d.zaxis; d.vpref_mode = c->d.vpref_mode; d.nbr_valid = c->d.nbr_valid;
    d.aperm = c->d.aperm; d.nbr_n = c->d.nbr_n; d.near_n = c->d.near_n; d.done_count = c->d.done_count;
    d.offsets = c->scenes.v.offsets; d.live = c->scenes.v.live; d.prev = c->scenes.v.prev; d.steps = c->scenes.v.steps;
    d.clear = c->scenes.clear;                                         // (null while the feature is off: the kernel skips the rows' records)
    if (c->trk_on) {
        static_assert(sizeof(sca_dubins::AgentTrack) % 4 == 0, "k_scene_restart copies the tracker record as 4-byte words");
        d.trk_nbr0 = c->trk.nbr0; d.trk_goal_heading = c->trk_goal_heading;
        d.trk_st = (restart_u32 *)c->trk.st; d.trk_init = (const restart_u32 *)c->trk_init; d.trk_words = (int)(sizeof(sca_dubins::AgentTrack) / 4);
    }
    // The kernel writes the named scenes' parts of the forest on c->stream, behind every reader of it: a step's K1 and K4 run on
    // c->stream or, where the tracker overlaps, K1 on trk_stream -- and the step joins trk_stream back into c->stream before it ends, so
    // whatever was enqueued by an earlier call stands in front of this launch in stream order.  Without a set per scene the forest's
    // pointers are null: restart_obstacles_check has refused every count >= 0, so the kernel returns before it reads them.
    RestartObsDev o{};
    if (c->scenes.obs_on) o = RestartObsDev{c->d.obs, c->d.obs_sorted, c->d.operm, c->d.otree, c->d.owide, (int32_t *)c->scenes.ov.oroot, (int32_t *)c->scenes.ov.oroot + c->scenes.v.nscenes};
    hipLaunchKernelGGL(k_scene_restart, dim3(count), dim3(RESTART_T), 0, c->stream, d, b, B.L, has, (const int32_t *)(b + B.new_size_off), c->scenes.size, o, B.OL, at_dev, B.AL,
                       RestartPathDev{c->pslot_pts, c->pslot_len, c->path.rem, c->path.now_goal, c->path_W}, B.PL);
    CHK(c, hipGetLastError());
    return 0;
}
// The device has the new episodes: now the host mirrors follow (a call that failed before has left them alone) -- policies, the radius a
// later sca_set_state uploads, the kd permutation while the host holds it; the maxima only grow (conservative filters).  "A refused call
// changes nothing" is about the refusals of the checks.  A runtime error of the list copy or the synchronisation behind the launch is not
// one: the device may then hold the new episode while h_policy, h_rec and h_perm hold the old -- as after any failed HIP call, the context
// is to be set up again (sca_set_agents), not stepped on.
static void restart_commit(sca_ctx *c, const RestartBlock &B, const RestartArgs &A, RestartPlan &plan) {
    const uint8_t *b = c->scenes.rs_host;
    const int32_t *off = c->scenes.h_off.data(), *start = (const int32_t *)(b + B.L.off[RS_START]), *new_size = (const int32_t *)(b + B.new_size_off);
    const uint8_t *pol = b + B.L.off[RS_POLICY];
    for (int e = 0, k = 0; e < A.count; e++) {
        const int lo = off[A.scene_ids[e]], hi = off[A.scene_ids[e] + 1];
        for (int a = lo, r = start[e]; a < lo + new_size[e]; a++, r++) {
            c->h_policy[a] = pol[r];
            if (A.radius) c->h_rec[a].radius = A.radius[r];
        }
        for (int a = lo; a < hi; a++) c->h_perm[a] = a;                // (the vacant rows' too: the identity over the capacity)
        if (c->path_W > 0)                                            // the lists' lengths and the "straight-line agent with a path" bytes, over the capacity
            for (int a = lo; a < hi; a++, k++) { c->h_path_len[a] = plan.path_len[k]; c->h_path_vpref[a] = plan.path_vpref[k]; }
    }
    c->max_radius = std::max(c->max_radius, plan.max_radius);
    c->max_pref_speed = std::max(c->max_pref_speed, plan.max_pref_speed);
    if (plan.policy_changed || plan.size_changed) c->h_lp_list.swap(plan.lp_list);
    c->scenes.h_size.swap(plan.size_now);
    if (plan.obs_replaced > 0) {
        for (int e = 0; e < A.count; e++) if (A.obs_counts[e] >= 0) c->scenes.h_obs_count[A.scene_ids[e]] = A.obs_counts[e];
        c->max_obs_radius = std::max(c->max_obs_radius, plan.obs_max_radius);    // only grows: a conservative filter (sca_set_scene_obstacles)
    }
    if (plan.send_solver) {
        if (plan.ap_first) {
            c->d.ap = c->ap_dev;
            if (c->trk_on) c->trk_view.nd_per_agent = c->ap_nd;
        }
        // The context's Params are the ENVELOPE of the agents' own while per-agent attributes are in force, and like max_radius,
        // max_pref_speed and max_obs_radius above the envelope only grows under restarts: with scenes it feeds collide_reach (a
        // conservative filter of K1's candidate lists and K4's walks) and nothing that reaches a value -- every kernel reads d.ap[a] for
        // the fields below (agent_params), the grid and SCA_NBR_AUTO's `fits`, which read neighbor_dist, have no scene form.
        if (plan.env_nd > c->P.neighbor_dist) { c->P.neighbor_dist = plan.env_nd; c->P.range_sq = sca_gm::g_pow2(plan.env_nd); c->grid.inv_cell = grid_inv_cell(plan.env_nd); }
        c->P.max_speed = std::max(c->P.max_speed, plan.env_ms);
        c->P.dt_nominal = std::max(c->P.dt_nominal, plan.env_dt);
    }
    if (plan.table_on) {
        c->h_trk_trip.swap(plan.trip_new); c->h_trk_cls.swap(plan.cls_new); c->trk_table = plan.table_new; c->trk_attr_on = true;
        std::vector<std::array<double, 3>> classes;                    // by index: one the table does not use holds NaN
        for (int q = 0; q < TRK_CLASS_CAP && !plan.cu.many; q++)
            if (plan.table_new.users[q] > 0) {
                classes.resize((size_t)q + 1, std::array<double, 3>{std::nan(""), 0.0, 0.0});
                classes[q] = {plan.table_new.val[q].R, plan.table_new.val[q].lo, plan.table_new.val[q].hi};
            }
        tracker_view_apply(c, plan.cu.many, classes);
    }
    c->scenes.partial = scenes_any_partial(c->scenes.v.nscenes, off, c->scenes.h_size.data());
    scene_harvest_clear_fresh(c, A.count, A.scene_ids);                // an uncollected harvest of a restarted scene is gone (behind the call's synchronisation)
    c->h_pos_valid = false;                                            // (no host mirror of the positions is kept, as in sca_step_host)
    c->near_valid = false;
    // (scene_live_valid stays what it is: the kernel wrote the named scenes' counters itself, and where the others' are stale the recount
    // that is due anyway finds n_s live agents in a restarted scene too)
}
// A: the caller's arrays as the entry point took them (an entry point that does not take an array leaves it NULL); attrs: NULL but for
// sca_restart_scenes_attrs / _paths
static int restart_scenes(sca_ctx *c, const RestartArgs &A, const sca_restart_attrs *attrs = nullptr) {
    // (with `attrs` a policy may move an agent between tracked and untracked: the classes are recomputed, not cut by policy)
    const RestartCtx X{c->scenes.on ? c->scenes.v.nscenes : 0, c->scenes.on ? c->scenes.h_off.data() : nullptr, c->state_set, c->scenes.begun, c->trk_on,
                       restart_refuses_paths(c->paths_on, c->path_W > 0), !attrs && c->trk_on && c->trk_view.R_pa != nullptr, c->h_policy.data()};
    const RestartCheck k = scene_restart_check(X, A);
    if (k.fault != RESTART_OK) return restart_refuse(c, restart_fault_text(k, X, A), scene_restart_error_code(k.fault));
    const int32_t *obs_cap = c->scenes.obs_on ? c->scenes.h_obs_off.data() : nullptr;
    const RestartObsCheck ko = restart_obstacles_check(obs_cap != nullptr, obs_cap, A.count, A.scene_ids, A.obs_counts, A.obs_pos, A.obs_radius);
    if (ko.fault != RESTART_OBS_OK) return restart_refuse(c, restart_obstacles_fault_text(ko, A, obs_cap), restart_obstacles_error_code(ko.fault));
    RestartAttrs RA;                                                   // every member NULL without `attrs`
    if (attrs) {
        const AttrDefaults D{c->P_ctx.neighbor_dist, c->P_ctx.time_step, c->P_ctx.time_horizon, c->P_ctx.max_speed, c->P_ctx.max_heading_change, c->P_ctx.dt_nominal,
                             c->P_ctx.max_neighbors, c->trk_enable_vals[0], c->trk_enable_vals[1], c->trk_enable_vals[2]};
        const RestartAttrCheck ka = restart_attrs_check(X, A, attrs, D, &RA);
        if (ka.fault != RESTART_ATTR_OK) return restart_refuse(c, restart_attrs_fault_text(ka, attrs), restart_attrs_error_code(ka.fault));
    }
    // the episodes' waypoint lists (sca_restart_scenes_paths): in slot form every entry point is accepted, and a call without path arrays
    // gives the named rows empty lists
    const RestartPathCheck kp = restart_paths_check(c->path_W > 0, c->path_W, k.total, A.path_offsets, A.path_points);
    if (kp.fault != RESTART_PATHS_OK) return restart_refuse(c, restart_paths_fault_text(kp, A, c->path_W), restart_paths_error_code(kp.fault));

    const RestartBlock B = restart_block_layout(c->max_n, c->max_m, c->path_W);
    if (int r = restart_block(c, (size_t)B.total)) return r;
    uint8_t *b = c->scenes.rs_host;
    RestartPlan plan = restart_pack(b, B, X, A, c->scenes.h_size.data(), obs_cap, c->path_W);
    plan.obs_replaced = ko.replaced;
    restart_pack_obstacles(b, B.OL, A, plan);
    restart_pack_attrs(c, b, B, A, attrs != nullptr, RA, plan);
    RestartFills fills;
    if (int r = restart_first_use(c, plan, fills)) return r;
    if (int r = restart_launch(c, A.count, B, plan.has)) return r;
    // the classes came back from the per-agent form, or an index moved in a scene that was not named: the whole class array, one byte per
    // agent, behind the launch (its rows of the named scenes are the bytes the launch wrote) and in front of the call's one synchronisation
    if (plan.cls_whole) CHK(c, hipMemcpyAsync(c->trk_cls, plan.cls_new.data(), (size_t)c->n, hipMemcpyHostToDevice, c->stream));
    if (!plan.lp_list.empty()) CHK(c, hipMemcpyAsync(c->lp_list, plan.lp_list.data(), sizeof(int32_t) * plan.lp_list.size(), hipMemcpyHostToDevice, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    restart_commit(c, B, A, plan);
    return 0;
}
int sca_restart_scenes(sca_ctx *c, int count, const int32_t *scene_ids, const double *pos, const float *vel, const double *heading,
                       const double *radius, const double *pref_speed, const double *goal, const uint8_t *policy, const uint8_t *zaxis,
                       const double *max_run_dist, const double *goal_heading) {
    API_ENTER(c);
    return restart_scenes(c, RestartArgs{count, scene_ids, pos, vel, heading, radius, pref_speed, goal, policy, zaxis, max_run_dist, goal_heading});
}
int sca_restart_scenes_sized(sca_ctx *c, int count, const int32_t *scene_ids, const int32_t *sizes, const double *pos, const float *vel,
                             const double *heading, const double *radius, const double *pref_speed, const double *goal, const uint8_t *policy,
                             const uint8_t *zaxis, const double *max_run_dist, const double *goal_heading) {
    API_ENTER(c);
    return restart_scenes(c, RestartArgs{count, scene_ids, pos, vel, heading, radius, pref_speed, goal, policy, zaxis, max_run_dist, goal_heading, sizes});
}
int sca_restart_scenes_obstacles(sca_ctx *c, int count, const int32_t *scene_ids, const int32_t *sizes, const int32_t *obs_counts, const double *obs_pos,
                                 const double *obs_radius, const double *pos, const float *vel, const double *heading, const double *radius,
                                 const double *pref_speed, const double *goal, const uint8_t *policy, const uint8_t *zaxis, const double *max_run_dist,
                                 const double *goal_heading) {
    API_ENTER(c);
    return restart_scenes(c, RestartArgs{count, scene_ids, pos, vel, heading, radius, pref_speed, goal, policy, zaxis, max_run_dist, goal_heading, sizes, obs_counts, obs_pos, obs_radius});
}
int sca_restart_scenes_attrs(sca_ctx *c, int count, const int32_t *scene_ids, const int32_t *sizes, const int32_t *obs_counts, const double *obs_pos,
                             const double *obs_radius, const sca_restart_attrs *attrs, const double *pos, const float *vel, const double *heading,
                             const double *radius, const double *pref_speed, const double *goal, const uint8_t *policy, const uint8_t *zaxis,
                             const double *max_run_dist, const double *goal_heading) {
    API_ENTER(c);
    return restart_scenes(c, RestartArgs{count, scene_ids, pos, vel, heading, radius, pref_speed, goal, policy, zaxis, max_run_dist, goal_heading, sizes, obs_counts, obs_pos, obs_radius}, attrs);
}
int sca_restart_scenes_paths(sca_ctx *c, int count, const int32_t *scene_ids, const int32_t *sizes, const int32_t *obs_counts, const double *obs_pos,
                             const double *obs_radius, const sca_restart_attrs *attrs, const int32_t *path_offsets, const double *path_points,
                             const double *pos, const float *vel, const double *heading, const double *radius, const double *pref_speed, const double *goal,
                             const uint8_t *policy, const uint8_t *zaxis, const double *max_run_dist, const double *goal_heading) {
    API_ENTER(c);
    return restart_scenes(c, RestartArgs{count, scene_ids, pos, vel, heading, radius, pref_speed, goal, policy, zaxis, max_run_dist, goal_heading, sizes, obs_counts, obs_pos, obs_radius, path_offsets, path_points}, attrs);
}
// ---- scene checkpoints (include/sca_hip.h; the layout, the check and the calls' rules are sca_scenes.h's, the kernels sca_scenes.hip.h's) ---------
static_assert(CKPT_LIB_VERSION == 103, "CkptHeader::lib_version is sca_version()");
static_assert(sizeof(sca_dubins::AgentTrack) % 4 == 0 && sizeof(long) == 8, "the checkpoint moves the tracker record as 4-byte words and reads its cursors as 64-bit");
static CkptTrackFields ckpt_track_fields() {
    using sca_dubins::AgentTrack; using sca_dubins::Plan3D; using sca_dubins::Maneuver2D;
    const int plan = (int)offsetof(AgentTrack, plan);
    CkptTrackFields F;
    F.words = (int)(sizeof(AgentTrack) / 4);
    F.use_dubins = (int)offsetof(AgentTrack, is_use_dubins);
    F.plan_ok = plan + (int)offsetof(Plan3D, ok);
    F.h_ok = plan + (int)offsetof(Plan3D, h) + (int)offsetof(Maneuver2D, ok); F.v_ok = plan + (int)offsetof(Plan3D, v) + (int)offsetof(Maneuver2D, ok);
    F.h_mode = plan + (int)offsetof(Plan3D, h) + (int)offsetof(Maneuver2D, mode); F.v_mode = plan + (int)offsetof(Plan3D, v) + (int)offsetof(Maneuver2D, mode);
    F.plan_mode = plan + (int)offsetof(Plan3D, mode);
    F.iters = plan + (int)offsetof(Plan3D, iters); F.rounds = plan + (int)offsetof(Plan3D, rounds); F.replans = (int)offsetof(AgentTrack, replans);
    F.count = plan + (int)offsetof(Plan3D, count); F.next = (int)offsetof(AgentTrack, next);
    return F;
}
static std::string ckpt_fault_text(const CkptCheck &k) {
    const std::string at = std::to_string(k.entry);
    switch (k.fault) {
    case CKPT_SHORT: return "the blob is NULL or shorter than a checkpoint's header";
    case CKPT_MAGIC_BAD: return "the blob is not a scene checkpoint (magic)";
    case CKPT_FORMAT_BAD: return "the blob has another format version than this library writes (" + std::to_string(CKPT_FORMAT) + ")";
    case CKPT_RECORD: return "the blob's tracker record or public record size is not this library's";
    case CKPT_SIZE_RANGE: return "the blob's header holds a size outside 1 .. " + std::to_string(KD_WAVE_CAP) + " or a flag word that is not 0 / 1";
    case CKPT_BYTES: return "the byte count is not the layout's for the blob's size (sca_scene_checkpoint_layout)";
    case CKPT_CHECKSUM: return "the payload's checksum is not the header's";
    case CKPT_SCENE_SIZE: return "the blob's size is not the scene's current size: restart the scene with the episode first";
    case CKPT_POLICY: return "row " + at + " has another policy in the blob than in the scene (or none the library knows): restart the scene with the episode first";
    case CKPT_TRACKER: return "tracker records are present in the blob and not needed by the scene in this context, or needed and absent";
    case CKPT_NO_LISTS: return "row " + at + " has waypoints left (rem > 0) and the context has no waypoint lists set";
    case CKPT_REM_RANGE: return "row " + at + " has a cursor outside 0 .. the length of the row's list as set";
    case CKPT_PERM: return "the permutation is not one of 0 .. size - 1 (position " + at + ")";
    case CKPT_FLAGS: return "row " + at + " has unknown flag bits or a v_pref mode other than 0 / 1";
    case CKPT_NOT_FINITE: return "row " + at + " has a position that is not finite or a radius that is not positive";
    case CKPT_COUNTERS: return "steps / live / prev or a step count are out of range, or live is not the number of rows without a flag";
    case CKPT_TRACK_RANGE: return "row " + at + " has a tracker record with a cursor, count or word outside its range";
    default: return "ok";
    }
}
static int ckpt_call_refuse(sca_ctx *c, const char *who, const CkptCallCheck &k, const int32_t *scene_ids) {
    const std::string w(who), at = std::to_string(k.entry);
    switch (k.fault) {
    case CKPT_CALL_NO_SCENES: c->err = w + ": no scenes -- sca_set_scenes first"; break;
    case CKPT_CALL_NO_STATE: c->err = w + ": no state yet -- sca_set_state first"; break;
    case CKPT_CALL_MID_STEP: c->err = w + " between a policy pass and its env update: finish the step first"; break;
    case CKPT_CALL_BAD_COUNT: c->err = w + ": count must be positive and no array NULL"; break;
    case CKPT_CALL_BAD_ID: c->err = w + ": scene_ids[" + at + "] = " + std::to_string(scene_ids[k.entry]) + " is not a scene of this context (0 .. " + std::to_string(c->scenes.v.nscenes - 1) + ")"; break;
    case CKPT_CALL_REPEATED_ID: c->err = w + ": scene_ids[" + at + "] = " + std::to_string(scene_ids[k.entry]) + " is named twice"; break;
    default: c->err = w + ": buffer " + at + " is NULL";
    }
    return scene_checkpoint_call_error_code(k.fault);
}
// the words a scene's layout depends on, as the scene stands in this context
static void ckpt_scene_words(const sca_ctx *c, int s, int *size, int *trk_words, int *has_paths) {
    const int lo = c->scenes.h_off[s], ns = c->scenes.h_size[s];
    bool tracked = false;
    for (int a = lo; a < lo + ns; a++) tracked = tracked || restart_policy_tracked(c->h_policy[a]);
    *size = ns;
    *trk_words = c->trk_on && tracked ? (int)(sizeof(sca_dubins::AgentTrack) / 4) : 0;
    *has_paths = c->paths_on ? 1 : 0;
}
static int ckpt_block(sca_ctx *c, size_t bytes) {
    if (c->scenes.ck_host && c->scenes.ck_bytes >= bytes) return 0;
    CHK(c, hipStreamSynchronize(c->stream));                            // (every call ends with its synchronisation: no launch still uses the block)
    if (c->scenes.ck_host) (void)hipHostFree(c->scenes.ck_host);
    c->scenes.ck_host = nullptr; c->scenes.ck_bytes = 0;
    CHK(c, hipHostMalloc((void **)&c->scenes.ck_host, bytes, hipHostMallocMapped | hipHostMallocCoherent));
    c->scenes.ck_bytes = bytes;
    return 0;
}
static CkptDev ckpt_dev(sca_ctx *c) {
    CkptDev d{};
    d.rec = c->d.rec; d.heading = c->d.heading; d.heading_keep = c->scenes.v.heading_keep; d.vpref_ext = c->d.vpref_ext; d.total_dist = c->d.total_dist;
    d.step_num = c->d.step_num; d.status = c->d.status; d.aperm = c->d.aperm; d.vpref_mode = c->d.vpref_mode; d.done_count = c->d.done_count;
    d.offsets = c->scenes.v.offsets; d.live = c->scenes.v.live; d.prev = c->scenes.v.prev; d.steps = c->scenes.v.steps;
    if (c->trk_on) { d.trk_nbr0 = c->trk.nbr0; d.trk_st = (restart_u32 *)c->trk.st; }
    if (c->paths_on) { d.rem = c->path.rem; d.now_goal = c->path.now_goal; }
    return d;
}
int sca_scene_checkpoint_layout(int size, int trk_words, int has_paths, int64_t *offsets, int64_t *total_bytes) {
    if (size < 1 || size > KD_WAVE_CAP || trk_words < 0 || (has_paths != 0 && has_paths != 1) || !offsets || !total_bytes) return SCA_ERR_ARG;
    const CkptLayout L = scene_checkpoint_layout(size, trk_words, has_paths);
    for (int s = 0; s < CK_SECTIONS; s++) offsets[s] = L.off[s];
    *total_bytes = L.total;
    return 0;
}
int sca_scene_checkpoint_info(const void *blob, int64_t bytes, struct sca_scene_checkpoint_info *out, int32_t struct_bytes) {
    if (!out || struct_bytes < (int32_t)offsetof(struct sca_scene_checkpoint_info, format) || struct_bytes > (int32_t)sizeof(struct sca_scene_checkpoint_info)) return SCA_ERR_ARG;
    CkptHeader H;
    const CkptCheck k = scene_checkpoint_check(blob, bytes, ckpt_track_fields(), nullptr, &H);
    if (k.fault != CKPT_OK) return scene_checkpoint_error_code(k.fault);
    struct sca_scene_checkpoint_info I{};
    I.struct_bytes = struct_bytes; I.reserved = 0; I.format = H.format; I.lib_version = H.lib_version; I.size = H.size; I.trk_words = H.trk_words; I.record_bytes = H.rec_bytes;
    I.has_tracker = H.has_track; I.has_paths = H.has_paths; I.steps = H.steps; I.live = H.live; I.prev = H.prev; I.total_bytes = H.total_bytes; I.checksum = H.checksum;
    std::memcpy(out, &I, (size_t)struct_bytes);
    out->struct_bytes = struct_bytes;
    return 0;
}
int sca_scene_checkpoint_bytes(sca_ctx *c, int scene, int64_t *bytes) {
    API_ENTER(c);
    ARG(c, bytes);
    if (!c->scenes.on) { c->err = "sca_scene_checkpoint_bytes: no scenes -- sca_set_scenes first"; return SCA_ERR_STATE; }
    if (scene < 0 || scene >= c->scenes.v.nscenes) { c->err = "sca_scene_checkpoint_bytes: scene " + std::to_string(scene) + " is not a scene of this context"; return SCA_ERR_ARG; }
    int ns, tw, hp;
    ckpt_scene_words(c, scene, &ns, &tw, &hp);
    *bytes = scene_checkpoint_layout(ns, tw, hp).total;
    return 0;
}
// One launch of k_scene_save (a workgroup per named scene) into the page-locked block, one synchronisation, then the host completes the
// headers -- policies, sizes, the checksum -- and copies the blobs out.  Where the state came from outside since the last env update the
// scenes' counters are recounted first, as every reader of them does (scenes_recount).
int sca_save_scenes(sca_ctx *c, int count, const int32_t *scene_ids, void *const *out, const int64_t *out_bytes) {
    API_ENTER(c);
    const CkptCallCheck k = scene_checkpoint_call_check(c->scenes.on ? c->scenes.v.nscenes : 0, c->state_set, c->scenes.begun, count, scene_ids, (const void *const *)out, out_bytes);
    if (k.fault != CKPT_CALL_OK) return ckpt_call_refuse(c, "sca_save_scenes", k, scene_ids);
    std::vector<CkptEntry> tab((size_t)count);
    int64_t at = ckpt_block_round((int64_t)sizeof(CkptEntry) * count);
    for (int e = 0; e < count; e++) {
        CkptEntry &x = tab[(size_t)e];
        x.scene = scene_ids[e]; x.reserved = 0;
        ckpt_scene_words(c, x.scene, &x.size, &x.trk_words, &x.has_paths);
        const int64_t need = scene_checkpoint_layout(x.size, x.trk_words, x.has_paths).total;
        if (out_bytes[e] < need) {
            c->err = "sca_save_scenes: buffer " + std::to_string(e) + " holds " + std::to_string(out_bytes[e]) + " bytes, scene " + std::to_string(x.scene) + " needs " + std::to_string(need) +
                     " (sca_scene_checkpoint_bytes)";
            return SCA_ERR_ARG;
        }
        x.at = at;
        at = ckpt_block_round(at + need);
    }
    if (int r = ckpt_block(c, (size_t)at)) return r;
    uint8_t *b = c->scenes.ck_host;
    std::memset(b, 0, (size_t)at);                                       // (the bytes between the sections are part of the sum)
    std::memcpy(b, tab.data(), sizeof(CkptEntry) * (size_t)count);
    if (int r = scenes_recount(c, c->stream)) return r;
    hipLaunchKernelGGL(k_scene_save, dim3(count), dim3(CKPT_T), 0, c->stream, ckpt_dev(c), b);
    CHK(c, hipGetLastError());
    CHK(c, hipStreamSynchronize(c->stream));
    for (int e = 0; e < count; e++) {
        const CkptEntry &x = tab[(size_t)e];
        const CkptLayout L = scene_checkpoint_layout(x.size, x.trk_words, x.has_paths);
        uint8_t *o = b + x.at;
        const int lo = c->scenes.h_off[x.scene];
        std::memcpy(o + L.off[CK_POLICY], c->h_policy.data() + lo, (size_t)x.size);
        if (!c->perm_on_device) {                                       // the live permutation is still the host's (no device build since it was set)
            int32_t *perm = (int32_t *)(o + L.off[CK_PERM]);
            for (int i = 0; i < x.size; i++) perm[i] = c->h_perm[lo + i] - lo;
        }
        CkptHeader H;
        std::memcpy(&H, o, sizeof H);                                   // (steps, live, prev: the kernel's)
        H.magic = CKPT_MAGIC; H.format = CKPT_FORMAT; H.lib_version = sca_version(); H.size = x.size; H.trk_words = x.trk_words; H.rec_bytes = CKPT_REC_BYTES;
        H.has_track = x.trk_words > 0 ? 1 : 0; H.has_paths = x.has_paths; H.reserved = 0; H.total_bytes = L.total;
        H.checksum = scene_checkpoint_sum(o + sizeof H, L.total - (int64_t)sizeof H);
        std::memcpy(o, &H, sizeof H);
        std::memcpy(out[e], o, (size_t)L.total);
    }
    return 0;
}
// Every blob is checked whole on the host (scene_checkpoint_check) before any device work; then the blobs go into the page-locked block,
// ONE launch of k_scene_load scatters them, and the call's one synchronisation follows.  Behind it the host mirrors follow, as after a
// restart: the permutation while the host holds it, the radius, the harvest's fresh words.
int sca_load_scenes(sca_ctx *c, int count, const int32_t *scene_ids, const void *const *in, const int64_t *in_bytes) {
    API_ENTER(c);
    const CkptCallCheck k = scene_checkpoint_call_check(c->scenes.on ? c->scenes.v.nscenes : 0, c->state_set, c->scenes.begun, count, scene_ids, in, in_bytes);
    if (k.fault != CKPT_CALL_OK) return ckpt_call_refuse(c, "sca_load_scenes", k, scene_ids);
    const CkptTrackFields F = ckpt_track_fields();
    std::vector<CkptEntry> tab((size_t)count);
    int64_t at = ckpt_block_round((int64_t)sizeof(CkptEntry) * count);
    for (int e = 0; e < count; e++) {
        const int s = scene_ids[e], lo = c->scenes.h_off[s];
        const CkptScene X{c->scenes.h_size[s], c->h_policy.data() + lo, c->trk_on, c->paths_on,
                          !c->paths_on ? nullptr : c->path_W > 0 ? c->h_path_len.data() + lo : nullptr};
        std::vector<int32_t> len;
        CkptScene Y = X;
        if (c->paths_on && c->path_W == 0) {                            // the block form: lengths from the offsets as set
            len.resize((size_t)X.size);
            for (int i = 0; i < X.size; i++) len[(size_t)i] = c->h_path_off[lo + i + 1] - c->h_path_off[lo + i];
            Y.path_len = len.data();
        }
        CkptHeader H;
        const CkptCheck kc = scene_checkpoint_check(in[e], in_bytes[e], F, &Y, &H);
        if (kc.fault != CKPT_OK) {
            c->err = "sca_load_scenes: blob " + std::to_string(e) + " (scene " + std::to_string(s) + "): " + ckpt_fault_text(kc);
            return scene_checkpoint_error_code(kc.fault);
        }
        CkptEntry &x = tab[(size_t)e];
        x.scene = s; x.size = H.size; x.trk_words = H.trk_words; x.has_paths = H.has_paths; x.reserved = 0; x.at = at;
        at = ckpt_block_round(at + H.total_bytes);
    }
    if (int r = ckpt_block(c, (size_t)at)) return r;
    uint8_t *b = c->scenes.ck_host;
    std::memcpy(b, tab.data(), sizeof(CkptEntry) * (size_t)count);
    for (int e = 0; e < count; e++) std::memcpy(b + tab[(size_t)e].at, in[e], (size_t)in_bytes[e]);
    hipLaunchKernelGGL(k_scene_load, dim3(count), dim3(CKPT_T), 0, c->stream, ckpt_dev(c), (const uint8_t *)b);
    CHK(c, hipGetLastError());
    CHK(c, hipStreamSynchronize(c->stream));
    for (int e = 0; e < count; e++) {
        const CkptEntry &x = tab[(size_t)e];
        const CkptLayout L = scene_checkpoint_layout(x.size, x.trk_words, x.has_paths);
        const uint8_t *o = b + x.at;
        const int lo = c->scenes.h_off[x.scene];
        const int32_t *perm = (const int32_t *)(o + L.off[CK_PERM]);
        for (int i = 0; i < x.size; i++) {
            c->h_perm[lo + i] = lo + perm[i];
            double radius;
            std::memcpy(&radius, o + L.off[CK_REC] + (size_t)CKPT_REC_BYTES * i + 40, sizeof radius);
            c->h_rec[lo + i].radius = radius; c->max_radius = std::max(c->max_radius, radius);   // only grows: a conservative filter, as under restarts
        }
    }
    scene_harvest_clear_fresh(c, count, scene_ids);                    // like a restart: what the slot's earlier episode handed over is gone
    c->h_pos_valid = false;
    c->near_valid = false;
    return 0;
}
int sca_get_scene_sizes(sca_ctx *c, int32_t *size) {
    API_ENTER(c);
    ARG(c, size);
    if (!c->scenes.on) { c->err = "no scenes (sca_set_scenes)"; return SCA_ERR_STATE; }
    std::memcpy(size, c->scenes.h_size.data(), sizeof(int32_t) * c->scenes.h_size.size());
    return 0;
}

// KDTree.buildAgentTree (mampenv.py:28) on the HOST from a position read-back (SCA_NBR_KDTREE_HOSTBUILD: the A/B reference of
// the device build below, which is what SCA_NBR_KDTREE runs).
static int build_agent_tree(sca_ctx *c) {
    if (!c->h_pos_valid) {
        if (int r = fetch_records(c)) return r;
        c->h_pos.resize(3 * (size_t)c->n);
        for (int i = 0; i < c->n; i++) { c->h_pos[3 * i] = c->h_rec[i].px; c->h_pos[3 * i + 1] = c->h_rec[i].py; c->h_pos[3 * i + 2] = c->h_rec[i].pz; }
        c->h_pos_valid = true;
    }
    // (vacant rows, sca_vacancy.h: the tree holds the occupied prefix of the permutation and nothing else; the vacant tail stays as it is)
    const int n = c->vac.on ? c->vac.m : c->n;
    kd_build_host(n, c->h_pos.data(), c->h_perm.data(), c->h_tree);
    CHK(c, hipMemcpyAsync(c->d.atree, c->h_tree.data(), sizeof(KdNode) * (2 * n - 1), hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->d.aperm, c->h_perm.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
    std::vector<KdWide> wide;
    kd_widen_host(n, c->h_tree, wide);
    std::vector<double> k((size_t)3 * n);
    for (int p = 0; p < n; p++)
        for (int a = 0; a < 3; a++) k[(size_t)a * n + p] = c->h_pos[3 * (size_t)c->h_perm[p] + a];
    CHK(c, hipMemcpyAsync(c->d.awide, wide.data(), sizeof(KdWide) * (2 * n - 1), hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->kd.kx, k.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->kd.ky, k.data() + n, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(c->kd.kz, k.data() + 2 * (size_t)n, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));                             // the staging vectors die with this scope
    CHK(c, hipMemsetAsync(c->d.done_count, 0, sizeof(int32_t) * 256 * 32, c->stream));
    return 0;
}

// KDTree.buildAgentTree on the device (sca_kdbuild.hip.h): gather, one launch per level of large nodes, one launch
// that finishes every small subtree.  Everything is enqueued on `ks`; nothing comes back to the host.
struct KdBuildArgs {                     // what an SCA_NBR_AUTO build adds (auto_enqueue_kd_build); a build inside a kd pass takes the defaults
    KdTail tail = {};                    // what the build hands its k_kd_block (seq = 0: not the tail form)
    hipEvent_t block_stop = nullptr;     // ... and the event to record behind it, if any
    int aux = 0;                         // KdScratch::aux
    hipEvent_t gather_stop = nullptr;    // the event to record behind the gather, the last kernel of the build that reads the record buffer
    bool next_pass = false;              // (timeline builds: the build belongs to the next pass)
};
static int build_agent_tree_device(sca_ctx *c, hipStream_t ks, DeviceView d, const KdBuildArgs &a = {}) {
#ifdef SCA_TIMELINE
    if (a.next_pass) d.tl_step++;
#endif
    // the tree's size: the occupied rows (sca_vacancy.h) -- the build kernels read DeviceView::n as the tree's size and as nothing else
    // (k_kd_gather, k_kd_top), so the view they get says m; the vacant tail of the permutation, behind m, is nobody's to touch
    const int n = c->vac.on ? c->vac.m : c->n;
    d.n = n;
    // poll: the level statistics of an earlier build, if they have arrived (never waited for)
    if (c->kd_ev_pending && hipEventQuery(c->kd_ev) == hipSuccess) {
        if (c->kd_ev_gen == c->kd_gen) {
            int depth = 0;
            while (depth < KD_MAX_LEVELS && c->kd_host_counts[depth] > 0) depth++;
            const int *nch = c->kd_host_counts + KD_MAX_LEVELS + 2;
            int single = depth;
            while (single > 0 && nch[single - 1] == c->kd_host_counts[single - 1]) single--;
            c->kd_single_hint = c->kd_host_counts[KD_MAX_LEVELS + 1] ? 0 : single + 1;        // 1-based
        }                                                                                     // (else stale: positions replaced since)
        c->kd_ev_pending = false;
    }
    // plan (no size limit: a level with more chunks than the chip holds at once takes its chunks by arrival, k_kd_lv_rank<true>)
    // (scenes: the forest plan -- every scene a root job of k_kd_block, no top, no level passes, no statistics)
    KdBuildPlan B{};
    if (c->scenes.on) {
        const KdForestPlan F = plan_kd_forest(c->scenes.largest, c->scenes.v.nscenes);
        B.wave_max = F.block; B.block = F.block; B.sgrid = F.grid;
        if (int r = scenes_recount(c, ks)) return r;                   // (a state from outside: the live counts the step opens with)
    } else B = plan_kd_build(c->tun, n, c->trk_on && c->trk_in_pass && ks != c->stream, c->kd_single_hint, c->kd.chunk_cap, c->kd_rank_capacity);
    if (B.top && KT_M / (B.wave_max + 1) >= KT_NODES) { c->err = "k_kd_top: wave_max below its table bound"; return SCA_ERR_STATE; }   // (static_assert'ed unreachable)
    // enqueue
    if (!c->perm_on_device) {
        CHK(c, hipMemcpyAsync(d.aperm, c->h_perm.data(), sizeof(int32_t) * c->n, hipMemcpyHostToDevice, ks));
        c->perm_on_device = true;
    }
    c->kd.wave_max = B.wave_max;
    KdScratch kd = c->kd;                                               // (by value into every kernel of the build)
    kd.aux = a.aux;
    hipEvent_t kb0 = nullptr, kb1 = nullptr;                            // profiling: the build's device time on the stream it runs on, every 16th build
    if (c->profiling && (c->kd_builds & 15u) == 0 && c->pool_kd_used + 2 <= 2 * 1024) {
        for (hipEvent_t *ev : {&kb0, &kb1}) if (int r = pool_take(c, c->pool_kd, c->pool_kd_used, 2 * 1024, ev)) return r;
        CHK(c, hipEventRecord(kb0, ks));
    }
    if (a.gather_stop) {                                                // SCA_NBR_AUTO
        LAUNCH_REC(c, a.gather_stop, k_kd_gather, dim3((n + 255) / 256), dim3(256), ks, d, kd, c->P);
        c->au.builds++;
    } else hipLaunchKernelGGL(k_kd_gather, dim3((n + 255) / 256), dim3(256), 0, ks, d, kd, c->P);
    if (c->scenes.on) {
        // the forest's job table behind the gather (which rewrites the single root job and the counts on every build); opens the step
        hipLaunchKernelGGL(k_kd_scene_jobs, dim3((c->scenes.v.nscenes + 255) / 256), dim3(256), 0, ks, kd, c->scenes.v, (const int32_t *)c->scenes.size, c->scenes.begun ? 0 : 1);
        c->scenes.begun = true;
    }
    if (B.top && B.levels) hipLaunchKernelGGL(k_kd_top, dim3(1), dim3(KT_T), 0, ks, d, kd);
    if (B.level_passes) {
        for (int l = 0; l < B.first_single; l++) {
            if (B.ticket) hipLaunchKernelGGL(k_kd_lv_rank<true>, dim3(B.grid), dim3(KD_LV_T), 0, ks, kd, l, ++c->kd_token);
            else hipLaunchKernelGGL(k_kd_lv_rank<false>, dim3(B.grid), dim3(KD_LV_T), 0, ks, kd, l, ++c->kd_token);
            hipLaunchKernelGGL(k_kd_lv_swap, dim3(B.grid), dim3(KD_LV_T + 64), 0, ks, d, kd, l);   // + the bookkeeping wavefront
        }
        hipLaunchKernelGGL(k_kd_level_tail, dim3(B.grid), dim3(KD_LV_T), 0, ks, d, kd, B.first_single, ++c->kd_token);
    }
    // one workgroup per subtree, in LDS (LAUNCH_OPT: an AUTO build in the tail form records the pass's kd-query event behind this kernel)
#define KD_BLOCK(M) LAUNCH_OPT(c, a.block_stop, (k_kd_block<M, M / 2>), dim3(B.sgrid), dim3(M / 2), ks, d, kd, B.levels, a.tail)
    switch (B.block) {
    case 256: KD_BLOCK(256); break;
    case 512: KD_BLOCK(512); break;
    case 768: KD_BLOCK(768); break;
    case 1024: KD_BLOCK(1024); break;
    case 1280: KD_BLOCK(1280); break;
    default: KD_BLOCK(KD_WAVE_CAP);
    }
#undef KD_BLOCK
    CHK(c, hipGetLastError());
    if (kb1) CHK(c, hipEventRecord(kb1, ks));
    // the tree's depth profile changes slowly: one small readback (a copy sits in the stream between the build and K1) every
    // 8th build, every build while no hint exists yet
    c->kd_builds++;
    if (B.level_passes && !c->kd_ev_pending && (c->kd_single_hint == 0 || (c->kd_builds & 7u) == 0)) {
        CHK(c, hipMemcpyAsync(c->kd_host_counts, c->kd.counts, sizeof(int) * (2 * KD_MAX_LEVELS + 3), hipMemcpyDeviceToHost, ks));
        CHK(c, hipEventRecord(c->kd_ev, ks));
        c->kd_ev_pending = true;
        c->kd_ev_gen = c->kd_gen;
    }
    return 0;
}
// SCA_NBR_GRID: counting sort of all agents into cells of neighborDist (sca_grid.hip.h), three launches
static int build_agent_grid_device(sca_ctx *c) {
    const int n = std::max(256, c->part_on ? c->d.n_present : c->n);      // k_grid_count's first 256 lanes also reset the step's counters
    const int H = 1 << c->grid.hbits;
    hipLaunchKernelGGL(k_grid_count, dim3((n + 255) / 256), dim3(256), 0, c->nbr_stream, c->d, c->grid, c->P);
    hipLaunchKernelGGL(k_grid_alloc, dim3((H + 256 * GRID_ALLOC_PER - 1) / (256 * GRID_ALLOC_PER)), dim3(256), 0, c->nbr_stream, c->grid);
    hipLaunchKernelGGL(k_grid_fill, dim3((n + 255) / 256), dim3(256), 0, c->nbr_stream, c->d, c->grid);
    CHK(c, hipGetLastError());
    return 0;
}
static int check_kd_overflow(sca_ctx *c) {
    int flag = 0;
    CHK(c, hipMemcpyAsync(&flag, c->kd.counts + KD_MAX_LEVELS + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    if (flag) {
        c->kd_single_hint = 0;
        CHK(c, hipMemsetAsync(c->kd.counts + KD_MAX_LEVELS + 1, 0, sizeof(int), c->stream));      // reported: start afresh
        c->err = "device kd-tree build overflow (a build since the last check ran out of levels or table space): results are invalid; "
                 "use SCA_NBR_KDTREE_HOSTBUILD for this scene [code " + std::to_string(flag) + "]";
        return SCA_ERR_STATE;
    }
    return 0;
}

// A pair that touches after the move was within r_a + r_b + 2 * max_step of each other before it (an obstacle:
// r_a + r_o + max_step); l3norm rounds to 5 dp, hence the 1e-4.  The kernels add the agent's own radius.
static double collide_max_step(const sca_ctx *c) { return 1.01 * std::max(c->max_pref_speed, c->P.max_speed) * c->P.dt_nominal; }
static void collide_reach(const sca_ctx *c, double &agent_reach, double &obs_reach) {
    const double max_step = collide_max_step(c);
    agent_reach = c->max_radius + 2.0 * max_step + 1e-4;
    obs_reach = c->max_obs_radius + max_step + 1e-4;
}
// k_clearance's bound (clearance_bound, sca_clearance.h): a partner has moved by at most max_step since the tree was built and is at most
// max_radius wide; the obstacle tree is static.  The kernel adds the agent's own radius.
static void clearance_reach(const sca_ctx *c, double &agent_reach, double &obs_reach) {
    agent_reach = collide_max_step(c) + c->max_radius + 1e-4;
    obs_reach = c->max_obs_radius + 1e-4;
}

// v_pref of the SCA / RVO3D+Dubins agents of the shard, before anything of the pass reads it (the per-agent prologue does).
// in_pass = true (a policy pass with the tracker inside): agent.neighbors[0] comes from trk.nbr0, which the previous pass's
// epilogue saved -- so nothing here reads the neighbour lists, and the neighbour query of this pass may run beside it.
// in_pass = false (sca_device_tracker_vpref): from the lists as they are (from_lists) or from what the caller uploaded.
// `forms`: the SCA_FORM_* bits of what was launched.
static int launch_tracker(sca_ctx *c, bool from_lists, bool in_pass, int &forms) {
    const int cnt = c->d.shard_count;
    // poll: the re-plan count of an earlier pass (copied back on the side stream, never waited for -- except the first count of an episode,
    // once: a caller that enqueues a long burst of steps runs far ahead of the device, and without it the whole burst would be launched
    // with the forms of "count unknown")
    if (c->trk_count_pending && c->trk_last_count < 0) CHK(c, hipEventSynchronize(c->trk_count_ev));
    if (c->trk_count_pending && hipEventQuery(c->trk_count_ev) == hipSuccess) { c->trk_last_count = c->trk_host_count[0]; c->trk_count_pending = false; }
    // plan
    const ReplanPlan R = plan_replans(c->tun, cnt, c->trk_last_count, c->trk_many, in_pass, c->part_on);
    forms = R.forms;
    // enqueue
    TrackDev K = c->trk;
    K.nbr0_from_lists = (from_lists && !in_pass) ? 1 : 0;
    if (!in_pass) K.prep = 0;
    if (!R.fused && !R.group_fused) hipLaunchKernelGGL(k_track, dim3((cnt + 255) / 256), dim3(256), 0, c->stream, c->d, c->trk_view, K);
    hipStream_t rs = c->stream;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (c->profiling && (c->prof_tick & 15u) == 0 && c->pool_trk_used + 2 <= 2 * 4096) {
        for (hipEvent_t *e : {&t0, &t1}) if (int r = pool_take(c, c->pool_trk, c->pool_trk_used, 2 * 4096, e)) return r;
        CHK(c, hipEventRecord(t0, rs));
    }
    // tracked agents whose turning radius / pitch limits differ (sca_device_tracker_set_agent_params) are planned class by class: the same
    // launches once per class of equal values, each with ITS values in the view's scalars; an agent of another class leaves at once
    const int nclass = c->trk_classes.empty() ? 1 : (int)c->trk_classes.size();
    for (int cl = 0; cl < nclass; cl++) {
        if (!c->trk_classes.empty() && !(c->trk_classes[cl][0] > 0.0)) continue;     // an index no occupied row uses (scene_class_table keeps the others' stable)
        sca_dubins::TrackView V = c->trk_view;
        if (!c->trk_classes.empty()) { V.class_id = cl; V.turning_radius = c->trk_classes[cl][0]; V.pitch_lo = c->trk_classes[cl][1]; V.pitch_hi = c->trk_classes[cl][2]; }
        for (int i = 0; i < R.n; i++) {
            const ReplanLaunch &L = R.launch[i];
            K.lo = L.lo; K.hi = L.hi;
            // workgroups of four wavefronts, one per SIMD of a CU: the forms need <= 256 registers, so a SIMD can hold two of
            // their wavefronts, and with one-wavefront workgroups the dispatcher doubles some SIMDs up while others stay empty
            static_assert(TRK_GROUP_THREADS == TRK_REPLAN_LANES, "one workgroup size for every re-plan kernel");
            const dim3 blk(TRK_GROUP_THREADS), grid((unsigned)(((long long)L.plans * L.lanes + TRK_GROUP_THREADS - 1) / TRK_GROUP_THREADS));
            switch (L.kernel) {
            case RP_GROUP64: hipLaunchKernelGGL(k_replan_group<64>, grid, blk, 0, rs, c->d, V, K); break;
            case RP_GROUP32: hipLaunchKernelGGL(k_replan_group<32>, grid, blk, 0, rs, c->d, V, K); break;
            case RP_GROUP16: hipLaunchKernelGGL(k_replan_group<16>, grid, blk, 0, rs, c->d, V, K); break;
            case RP_GROUP4: hipLaunchKernelGGL(k_replan_group<4>, grid, blk, 0, rs, c->d, V, K); break;
            case RP_LANE: hipLaunchKernelGGL(k_replan, grid, blk, 0, rs, c->d, V, K); break;
            case RP_TRACK_GROUP: hipLaunchKernelGGL(k_track_group, grid, blk, 0, rs, c->d, V, K); break;
            default: hipLaunchKernelGGL(k_track_replan, grid, blk, 0, rs, c->d, V, K);
            }
        }
    }
    if (t1) CHK(c, hipEventRecord(t1, rs));
    CHK(c, hipGetLastError());
    c->trk.parity = (c->trk.parity + 1) & 3;
    return 0;
}

// An SCA_NBR_AUTO step is bound by what the HOST needs to enqueue it (tools/gpu/exp_host.py: 79 us per step of 91 at N = 4096 -- twelve
// launches at ~2.3 us and ten event operations at ~5 us), so a cross-stream wait is only enqueued when the event it would wait for has
// not fired yet (in the steady state the kd stream is a whole pass ahead of what these guards protect; the query costs < 1 us).
static int wait_if_pending(sca_ctx *c, hipStream_t s, hipEvent_t e) {
    // (launch errors of the kernels enqueued before this call are sticky in hipGetLastError: look at them BEFORE the query below, whose
    // hipErrorNotReady has to be cleared -- ADVICE r5: a failed launch in front of a pending event used to be dropped with it)
    {
        const hipError_t le = hipGetLastError();                         // (an earlier query's hipErrorNotReady is an answer, not a failure)
        if (le != hipSuccess && le != hipErrorNotReady) CHK(c, le);
    }
    const hipError_t q = hipEventQuery(e);
    if (q == hipSuccess) return 0;
    if (q != hipErrorNotReady) CHK(c, q);                                // a real error of the query is an error
    (void)hipGetLastError();                                             // (hipErrorNotReady is an answer, not a failure)
    CHK(c, hipStreamWaitEvent(s, e, 0));
    return 0;
}
// SCA_NBR_AUTO's resources, on first use
int sca_ctx::Auto::fill(sca_ctx *c) {
    if (stream) return 0;
    CHK(c, hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    for (hipEvent_t *e : {&ev_fork, &ev_k1g, &ev_moved, &ev_cnt}) CHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    // two lists, alternating by pass: a pass's kd query may still be reading its list's length (to find it empty) when the next
    // pass's grid build resets and refills the other one
    CHK(c, hipMalloc((void **)&list, 2 * sizeof(int32_t) * (size_t)c->max_n));
    if (int r = dalloc(c, &count, 2)) return r;
    if (int r = dalloc(c, &busy, 1)) return r;
    if (int r = dalloc(c, &c->d.kdq_stats, 4)) return r;
    if (int r = dalloc(c, &ticket, 1)) return r;
    if (int r = dalloc(c, &sync, 8)) return r;
    CHK(c, hipStreamSynchronize(c->stream));
    for (hipEvent_t &e : ev_gather) CHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (hipEvent_t &e : ev_kdq) CHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    seq = 0; builds = 0; tail_seq = 0; waitvalue = true; count_pending = false;
    tail_ok = !c->tun.auto_no_tail;
    CHK(c, hipHostMalloc((void **)&count_host, sizeof(int)));
    c->d.kdq_list = list; c->d.kdq_count = count; c->d.kdq_busy = busy;
    forget();
    return 0;
}
// the kd build of a pass on the kd stream, beside whatever runs on the other streams (aux: it leaves the step's counters and the solve's
// prologue to the grid's kernels).  `positions`: the record buffer that holds the positions to build from; `ahead`: enqueued by
// sca_run_steps behind the previous step's integrate stage.
static int auto_enqueue_kd_build(sca_ctx *c, hipEvent_t after, const PubRec *positions, bool ahead) {
    sca_ctx::Auto &A = c->au;
    CHK(c, hipStreamWaitEvent(A.stream, after, 0));
    DeviceView v = c->d;
    v.rec = const_cast<PubRec *>(positions);
    // The kd query of the agents this pass's grid query will list: answered by that query's own last workgroup, once this build's last
    // kernel has published its tree (KdTail), while the list lengths that have come back say "nobody" -- otherwise a launch of
    // its own behind the build (pass_query_auto).  The build belongs to the pass whose grid query comes next: seq + 1, whether it is
    // enqueued inside that pass or ahead of it (sca_run_steps) -- in front of that grid query in the host's order either way.
    const AutoBuildPlan B = plan_auto_build(A.tail_ok, A.waitvalue, A.seq, A.last, c->tun.auto_tail_max, A.on_kd, A.builds);
    KdBuildArgs a;
    a.aux = 1; a.next_pass = ahead; a.gather_stop = A.ev_gather[B.gather_slot];
    if (B.tail) {
        // (the list of this parity was last read by the kd query of two passes ago, whose event slot is about to be recorded anew: the
        // pass's stream waits for it HERE instead of in front of its grid build)
        // (... if that query was a launch on the kd stream; in the launch-free form it ran inside the pass's own grid query, on this stream)
        if (B.wait_slot != AUTO_NO_SLOT) { if (int r = wait_if_pending(c, c->stream, A.ev_kdq[B.wait_slot])) return r; }
        a.tail.seq = B.seq; a.tail.sync = A.sync;
        A.tail_seq = B.seq;
        a.block_stop = A.ev_kdq[B.record_slot];
    }
    return build_agent_tree_device(c, A.stream, v, a);
}

// everything the kd stream was given has to be through before a caller reads the tree, the permutation or the lists, and before a pass that
// is not an AUTO pass builds in place: the context's stream waits for the last kd query
static int api_enter(sca_ctx *c) { return c->au.lazy_join ? auto_join(c) : 0; }
static int auto_join(sca_ctx *c) {
    c->au.lazy_join = false;
    if (!c->au.unjoined) return 0;
    CHK(c, hipStreamWaitEvent(c->stream, c->au.ev_kd, 0));
    c->au.unjoined = false;
    return 0;
}

// the refusals of the entry points that step (step_check, sca_forms.h): `checks` names the ones this caller makes, `who` is its prefix
static int step_refuse(sca_ctx *c, const char *who, int checks, int steps, int mode) {
    const StepFault f = step_check(checks, c->state_set, steps, mode, c->part_on, c->part_nranks > 1 && !c->shard_emulation);
    if (f != STEPF_OK) c->err = std::string(who) + step_fault_text(f);
    return step_fault_code(f);
}
// ---- a policy pass: what its stages share, then the stages in the order launch_policy runs them ---------------------------------------------------
struct PassPlan {
    bool timed = false, fuse_integrate = false;   // launch_policy's arguments
    hipEvent_t action_stop = nullptr;   // ... PassRide: the event to record behind k_action (the moved positions), if any
    bool fork_ready = false;            // ... PassRide: the fork rode on the previous step's last kernel
    int mode = 0;                      // the neighbour mode as resolved: SCA_NBR_AUTO has become SCA_NBR_KDTREE where it is a plain kd pass
    bool auto_mode = false;             // an AUTO pass
    bool kd_prebuilt = false;           // ... whose tree sca_run_steps has enqueued ahead
    AutoPassPlan A{};                   // ... and its slots (sca_forms.h), planned behind its build; A.tail: the grid query's last workgroup answers the listed agents
    int kdq_blocks = KDQ_BLOCKS;
    bool tracked = false;               // the tracker runs inside the pass
    bool overlap = false;               // ... and the neighbour branch beside its re-plans, on trk_stream
    unsigned parity_now = 0;            // TrackDev::parity in front of the tracker's launches
    int lp_lo = 0, lp_hi = 0;           // the shard's LP agents: [lp_lo, lp_hi) of lp_ids (under the partition ownership is dynamic: the LP
    const int32_t *lp_ids = nullptr;    // kernels walk all owned agents and skip the others)
    int cnt = 0;                        // agents of the shard
    SolvePlan S{};
    int forms = 0;                      // SCA_FORM_* as they accumulate
    bool prof = false;                  // this pass carries the profiling pool's event pairs
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};   // [e0, e1] = K1, [e2, e3] = the solve, when timed or prof
    hipEvent_t k1_stop = nullptr, sweep_stop = nullptr;       // the join as the stop event of the side stream's last kernel
    double agent_reach = 0, obs_reach = 0;                    // collide_reach: K1's and K4's collision candidates
};

// the refusals, the SCA_NBR_AUTO decision, the LP range and the solve's forms; nothing is launched (a pass that is not an AUTO pass joins the kd stream)
static int pass_resolve(sca_ctx *c, int mode, PassPlan &p) {
    if (int r = clearance_refuse(c, "a policy pass", clearance_check(CLR_PASS, clearance_state(c), mode, 0, true, 0))) return r;
#ifdef SCA_TIMELINE
    c->d.tl_step++;
#endif
    // the tracker's re-plans overlap the device kd build and the neighbour query; the per-agent prologue (which reads
    // v_pref) of the tracker's agents then moves from k_kd_gather to the tracker's kernels (track_store)
    p.tracked = c->trk_on && c->trk_in_pass;
    if (c->scenes.on && scenes_neighbor_mode(mode) < 0) {
        c->err = "scenes are set (sca_set_scenes): the scene form of the neighbour search is SCA_NBR_KDTREE (SCA_NBR_AUTO resolves to it)";
        return SCA_ERR_UNSUPPORTED;
    }
    if (mode == SCA_NBR_GRID) if (int r = vacancy_refuse(c, "a pass in SCA_NBR_GRID")) return r;   // (the grid build does not skip vacant rows)
    // SCA_NBR_AUTO: an AUTO pass, or a plain kd pass where that cannot help (plan_auto; the cell-owner partition has its own structures)
    sca_ctx::Auto &A = c->au;
    double &ar = p.agent_reach, &orr = p.obs_reach;
    collide_reach(c, ar, orr);
    if (mode == SCA_NBR_AUTO) {
        // (scenes: the grid's cell key carries no scene id -- one more place where it cannot help)
        const bool fits = !c->scenes.on && c->max_radius + ar <= c->P.neighbor_dist && c->max_radius + orr <= c->P.neighbor_dist;
        if (int r = step_refuse(c, "", STEP_CHK_PART_MODE, 0, mode)) return r;
        if (int r = A.fill(c)) return r;
        if (A.count_pending && hipEventQuery(A.ev_cnt) == hipSuccess) { A.last = A.count_host[0]; A.count_pending = false; }   // poll
        // (sca_run_steps only builds ahead when auto_next() holds)
        const AutoPlan P = plan_auto(fits, p.tracked, A.ahead, A.last, c->tun.auto_div, A.backoff, c->d.shard_count, c->vac.on);
        A.backoff = P.auto_backoff; A.last = P.kdq_last; p.kdq_blocks = P.kdq_blocks;
        p.auto_mode = P.auto_pass;
        if (!p.auto_mode) mode = SCA_NBR_KDTREE;
        A.fits = fits;
    }
    p.mode = mode;
    p.kd_prebuilt = p.auto_mode && A.ahead;
    A.ahead = false;
    A.ran = p.auto_mode;
    if (!p.auto_mode) { if (int r = auto_join(c)) return r; }          // (a pass that builds its tree in place: the kd stream must be through)
    const DeviceView &d = c->d;
    const int cnt = p.cnt = d.shard_count;
    p.lp_hi = c->h_lp_list.empty() ? 0 : cnt;
    p.lp_ids = c->part_on ? d.own : c->lp_list;
    if (!c->part_on) {
        p.lp_lo = (int)(std::lower_bound(c->h_lp_list.begin(), c->h_lp_list.end(), d.shard_begin) - c->h_lp_list.begin());
        p.lp_hi = (int)(std::lower_bound(c->h_lp_list.begin(), c->h_lp_list.end(), d.shard_begin + cnt) - c->h_lp_list.begin());
    }
    p.overlap = p.tracked && (mode == SCA_NBR_KDTREE || mode == SCA_NBR_GRID || p.auto_mode);
    // plan: K1's form, k_solve's (its v_pref-independent half right behind the neighbour query, i.e. beside the re-plans when they are
    // overlapped; or the form that finishes its own fallbacks), K3's and the epilogue's
    const auto plan = [&](bool no_scratch) {
        return plan_solve(c->tun, c->simds, cnt, c->part_on, c->part_nranks, (long long)c->h_lp_list.size(), p.lp_hi - p.lp_lo, p.overlap, c->trk_last_count, no_scratch);
    };
    p.S = plan(false);
    if (p.S.split && !c->d.sw_slot) {
        // scratch of the two-launch solve (cones + survivor lists, ~2 KB per agent): all three buffers or none, and a pass that
        // cannot have them runs the one-launch k_solve instead of failing
        const size_t N = (size_t)c->max_n;
        double *a = nullptr; uint16_t *b = nullptr; int32_t *e = nullptr;
        const bool ok = hipMalloc((void **)&a, sizeof(double) * N * K_MAX * SLOTF) == hipSuccess &&
                        hipMalloc((void **)&b, sizeof(uint16_t) * N * 512) == hipSuccess &&
                        hipMalloc((void **)&e, sizeof(int32_t) * N) == hipSuccess;
        if (ok) { c->d.sw_slot = a; c->d.sw_surv = b; c->d.sw_n = e; }
        else { (void)hipGetLastError(); if (a) (void)hipFree(a); if (b) (void)hipFree(b); if (e) (void)hipFree(e); p.S = plan(true); }
    }
    c->d.lp_kernel = p.S.lp_kernel;
    p.forms = p.S.forms | (c->paths_on ? SCA_FORM_WAYPOINTS : 0) | (c->scenes.on ? SCA_FORM_SCENES : 0) |
              (c->scenes.obs_on ? SCA_FORM_SCENE_OBSTACLES : 0) | (c->vac.on ? SCA_FORM_VACANCY : 0);   // (the waypoint, scene and vacancy bits are state, not a choice)
    c->kd.skip_prep = c->grid.skip_prep = p.overlap ? 1 : 0;
    // K4's candidate lists and its fallback cover one cell around the agent: the collision reach must fit into it
    if (mode == SCA_NBR_GRID && (c->max_radius + ar > c->P.neighbor_dist || c->max_radius + orr > c->P.neighbor_dist)) {
        c->err = "SCA_NBR_GRID needs radius + collision reach <= neighbor_dist"; return SCA_ERR_UNSUPPORTED;
    }
    return 0;
}
// k_waypoint*, the fork onto the side stream, the AUTO pass's kd build
static int pass_fork(sca_ctx *c, PassPlan &p) {
    // Streams.  Without the tracker everything is one chain on the main stream.  With it (overlap): the pass's critical path
    // k_track -> re-plans -> prologue -> pick stays on the main stream, and the neighbour structure + query (+ the sweep half of
    // k_solve), which depend on nothing of the tracker -- it reads agent.neighbors[0] from what the previous pass's epilogue
    // saved, not from the lists K1 overwrites -- run beside them on trk_stream:
    //   main: [fork] k_track re-plans (or k_track_replan) ........ [wait join] k_solve / k_solve_pick4 ...
    //   side: [wait fork] K0 ...... K1 (k_solve_sweep) [join]
    c->nbr_stream = p.overlap ? c->trk_stream : c->stream;
    // waypoint lists: get_trajectory (the head of every find_next_action) on the main stream, in front of the fork below and of the AUTO
    // build's -- so in front of every prologue site on every stream (k_kd_gather / the grid's first kernel on either stream, k_prep, k_solve*,
    // track_store).  sca_run_steps records no fork on the previous step's last kernel while paths are set (fork_ready is false here then);
    // an AUTO build enqueued ahead (aux) computes no prologue.
    if (c->paths_on) {
        if (p.fork_ready) { c->err = "internal: a fork recorded ahead of k_waypoint"; return SCA_ERR_STATE; }
        if (p.cnt > 0 && c->path_W)
            hipLaunchKernelGGL(k_waypoint_slots, dim3((p.cnt + 255) / 256), dim3(256), 0, c->stream, c->d,
                               PathSlotView{c->pslot_pts, c->pslot_len, c->path.rem, c->path.now_goal, c->path_W});
        else if (p.cnt > 0) hipLaunchKernelGGL(k_waypoint, dim3((p.cnt + 255) / 256), dim3(256), 0, c->stream, c->d, c->path);
    }
    p.parity_now = (unsigned)c->trk.parity;
    if (p.overlap) {
        if (!p.fork_ready) CHK(c, hipEventRecord(c->trk_fork, c->stream));   // (fork_ready: it rode on the previous step's last kernel, sca_run_steps)
        CHK(c, hipStreamWaitEvent(c->trk_stream, c->trk_fork, 0));
    }
    sca_ctx::Auto &A = c->au;
    if (p.auto_mode && !p.kd_prebuilt) {   // SCA_NBR_AUTO: the kd build (its permutation is history: every step) on a stream of its own, from the pass's start
        CHK(c, hipEventRecord(A.ev_fork, c->stream));
        if (int r = auto_enqueue_kd_build(c, A.ev_fork, c->d.rec, false)) return r;
    }
    if (p.auto_mode)                    // (A.tail, the launch-free form: the grid query's last workgroup answers whoever is listed, from the tree its pass's build publishes)
        p.A = plan_auto_pass(A.seq, A.tail_seq, A.on_kd, A.waitvalue, A.count_pending, A.passes, A.builds);
    c->trk.prep = p.overlap ? 1 : 0; c->trk.P = c->P;
    return 0;
}
// K0: the neighbour structure of the pass, on nbr_stream
static int pass_structure(sca_ctx *c, const PassPlan &p) {
    c->nbr_mode = p.auto_mode ? (int)SCA_NBR_GRID : p.mode;           // (what K4's fallback looks into: the grid in an AUTO pass)
    if (p.auto_mode) {
        c->d.kdq_cap = std::max(1, c->d.shard_count / c->tun.auto_div);
        // this pass's list (the previous pass's kd query may still be looking at the other one's length)
        c->d.kdq_list = c->au.list + (size_t)p.A.parity * c->max_n;
        c->d.kdq_count = c->au.count + p.A.parity;
        // ... which the kd query of two passes ago must be through with (it is, unless the kd stream lags by two whole passes)
        if (p.A.reuse_slot != AUTO_NO_SLOT) { if (int r = wait_if_pending(c, c->nbr_stream, c->au.ev_kdq[p.A.reuse_slot])) return r; }
        return build_agent_grid_device(c);
    }
    if (p.mode == SCA_NBR_KDTREE) return build_agent_tree_device(c, c->nbr_stream, c->d);
    if (p.mode == SCA_NBR_GRID) return build_agent_grid_device(c);
    if (p.mode != SCA_NBR_KDTREE_HOSTBUILD) { c->err = "neighbor mode not available in this build"; return SCA_ERR_UNSUPPORTED; }
    if (c->perm_on_device) {
        CHK(c, hipMemcpyAsync(c->h_perm.data(), c->d.aperm, sizeof(int32_t) * c->n, hipMemcpyDeviceToHost, c->stream));
        CHK(c, hipStreamSynchronize(c->stream));
        c->perm_on_device = false;
    }
    if (int r = build_agent_tree(c)) return r;
    hipLaunchKernelGGL(k_prep, dim3((c->n + 255) / 256), dim3(256), 0, c->stream, c->d, c->P);
    return 0;
}
// the listed agents of an AUTO pass: their kd query, the list length's copy, the wait for final lists
static int pass_query_auto(sca_ctx *c, PassPlan &p) {
    sca_ctx::Auto &A = c->au;
    hipStream_t ns = c->nbr_stream;
    // the agents the grid query listed (more than max_neighbors in range, equal distances) get the kd-tree's answer: behind the
    // build on the kd stream, and nothing reads a list before that query is through
    A.seq = p.A.seq;                                                   // (its parity picked the list; it may wrap)
    A.on_kd = p.A.on_kd;
    // (the launch-free form: the grid query's own last workgroup has answered the listed agents from this pass's tree (KdTail) -- no
    // launch, no cross-stream wait on the build's stream, no stream wait operation on this one)
    if (p.A.tail) p.forms |= SCA_FORM_AUTO_TAIL;
    else {
        CHK(c, hipStreamWaitEvent(A.stream, A.ev_k1g, 0));            // (recorded behind the grid query)
        // (ev_kdq: also "the last kd query": auto_join and the event form of the wait)
        LAUNCH_REC(c, A.ev_kdq[p.A.kdq_slot], k_neighbors_kd_auto, dim3(p.kdq_blocks), dim3(K1_WAVES * 64), A.stream, c->d, c->P, p.agent_reach, p.obs_reach, c->max_radius, A.ticket);
    }
    // (ADVICE.md questions this copy's place on the kd stream, behind the build: moving it is a behaviour change for a pull request of its own)
    if (p.A.copy_count) {                                              // how many were listed: for later passes' choice, never waited for
        CHK(c, hipMemcpyAsync(A.count_host, c->d.kdq_count, sizeof(int), hipMemcpyDeviceToHost, A.stream));
        CHK(c, hipEventRecord(A.ev_cnt, A.stream));
        A.count_pending = true;
    }
    A.passes = p.A.passes;
    A.ev_kd = A.ev_kdq[p.A.kdq_slot];
    // (AUTO_WAIT_NONE, the launch-free form: the lists are final when the grid query's launch ends -- its last workgroup answered whoever was listed)
    if (p.A.wait == AUTO_WAIT_VALUE) {
        // lists final: at once when the grid query listed nobody, else behind the kd query (see k_neighbors_kd_auto)
        if (hipStreamWaitValue32(ns, A.busy, 0u, hipStreamWaitValueEq, 1u) != hipSuccess) {
            (void)hipGetLastError();                                  // a platform without stream memory operations: the event wait from now on
            A.waitvalue = false;
            CHK(c, hipStreamWaitEvent(ns, A.ev_kd, 0));
        }
    } else if (p.A.wait == AUTO_WAIT_EVENT) CHK(c, hipStreamWaitEvent(ns, A.ev_kd, 0));
    // [e0, e1] of an AUTO pass: the grid query AND the wait for the kd query of the listed agents behind it (the lists are final here)
    if (p.timed || p.prof) CHK(c, hipEventRecord(p.e[1], ns));
    return 0;
}
// K1 in its forms, on nbr_stream
static int pass_query(sca_ctx *c, PassPlan &p) {
    const DeviceView &d = c->d;
    const int cnt = p.cnt;
    const SolvePlan &S = p.S;
    hipStream_t ns = c->nbr_stream;
    for (int i = 0; i < 4; i++) p.e[i] = c->ev[i];
    p.prof = !p.timed && c->profiling && (c->prof_tick++ & 15u) == 0 && c->pool_used + 4 <= 4 * 4096;
    if (p.prof) { for (hipEvent_t &e : p.e) if (pool_event(c, &e)) return SCA_ERR_HIP; }
    if (p.timed || p.prof) CHK(c, hipEventRecord(p.e[0], ns));
    const double agent_reach = p.agent_reach, obs_reach = p.obs_reach;
    // (overlapped: the join rides on the side stream's last kernel -- the neighbour query, or the sweep behind it)
    const hipEvent_t k1_stop = p.k1_stop = p.overlap && !S.split && c->tun.ext_stop ? c->trk_join : nullptr;
    p.sweep_stop = p.overlap && S.split && c->tun.ext_stop ? c->trk_join : nullptr;
    const bool obs = d.m > 0;                                           // (scenes without obstacles: the K1 forms without the obstacle phase, see neighbors_one)
    const dim3 k1p_grid((cnt + K1P_WAVES * K1P_APW - 1) / (K1P_WAVES * K1P_APW)), k1p_block(K1P_WAVES * 64);
    if (p.auto_mode) {
        c->d.auto_sync = p.A.tail ? c->au.sync : nullptr;                 // (d is c->d)
        c->d.auto_pass_seq = p.A.seq;
        c->d.auto_err = c->kd.counts + KD_MAX_LEVELS + 1;
        const auto k1 = obs ? k_neighbors_grid<true, true> : k_neighbors_grid<true, false>;
        LAUNCH_REC(c, c->au.ev_k1g, k1, k1p_grid, k1p_block, ns, d, c->grid, c->P, agent_reach, obs_reach, c->max_radius);
    } else if (p.mode == SCA_NBR_GRID) {
        const auto k1 = obs ? k_neighbors_grid<false, true> : k_neighbors_grid<false, false>;
        LAUNCH_OPT(c, k1_stop, k1, k1p_grid, k1p_block, ns, d, c->grid, c->P, agent_reach, obs_reach, c->max_radius);
    } else if (c->scenes.on) {                                          // (obs_on: per-scene sets with at least one obstacle, always the obstacle phase)
        const auto k1 = [&](auto roots, auto has_obs) -> int {          // Roots and HAS_OBS picked once, then the packed or the unpacked form
            const auto kd4 = k_neighbors_kd4_scenes<decltype(has_obs)::value, decltype(roots)>, kd = k_neighbors_kd_scenes<decltype(has_obs)::value, decltype(roots)>;
            if (S.packed) LAUNCH_OPT(c, k1_stop, kd4, k1p_grid, k1p_block, ns, d, c->P, agent_reach, obs_reach, c->max_radius, roots);
            else LAUNCH_OPT(c, k1_stop, kd, dim3(std::min((cnt + K1_WAVES - 1) / K1_WAVES, MAX_GRID)), dim3(K1_WAVES * 64), ns, d, c->P, agent_reach, obs_reach, c->max_radius, roots);
            return 0;
        };
        if (int r = c->scenes.obs_on ? k1(SceneObsRoots{c->scenes.v, c->scenes.ov}, std::true_type()) : obs ? k1(SceneRoots{c->scenes.v}, std::true_type()) : k1(SceneRoots{c->scenes.v}, std::false_type())) return r;
    } else if (S.packed) {
        const auto k1 = obs ? k_neighbors_kd4<true> : k_neighbors_kd4<false>;
        LAUNCH_OPT(c, k1_stop, k1, k1p_grid, k1p_block, ns, d, c->P, agent_reach, obs_reach, c->max_radius);
    } else {
        const auto k1 = obs ? k_neighbors_kd<true> : k_neighbors_kd<false>;
        LAUNCH_OPT(c, k1_stop, k1, dim3(std::min((cnt + K1_WAVES - 1) / K1_WAVES, MAX_GRID)), dim3(K1_WAVES * 64), ns, d, c->P, agent_reach, obs_reach, c->max_radius);
    }
    c->near_valid = true;
    if (p.auto_mode) return pass_query_auto(c, p);
    if (p.timed || p.prof) CHK(c, hipEventRecord(p.e[1], ns));          // [e0, e1] = K1
    return 0;
}
// the sweep half of a split solve, the re-plan count's copy, the join of the side stream
static int pass_join(sca_ctx *c, const PassPlan &p) {
    hipStream_t ns = c->nbr_stream;
    if (p.S.split) LAUNCH_OPT(c, p.sweep_stop, k_solve_sweep, dim3((p.cnt + SOLVE_WAVES - 1) / SOLVE_WAVES), dim3(SOLVE_WAVES * 64), ns, c->d, c->P);
    if (p.overlap) {
        // the re-plan count of this pass for a later pass's launch decision: on the side stream, every 4th pass, never waited for
        const unsigned pass = c->trk_passes++;
        if (!c->trk_count_pending && (pass & 3u) == 1) {                    // the previous pass's slot: final since before the fork
                                                                            // (first at the second pass: the forms settle within three)
            CHK(c, hipMemcpyAsync(c->trk_host_count, c->trk.count + ((p.parity_now + 3u) & 3u), sizeof(int), hipMemcpyDeviceToHost, ns));
            CHK(c, hipEventRecord(c->trk_count_ev, ns));
            c->trk_count_pending = true;
        }
        if (!p.k1_stop && !p.sweep_stop) CHK(c, hipEventRecord(c->trk_join, ns));
        CHK(c, hipStreamWaitEvent(c->stream, c->trk_join, 0));                // (the prologue: track_store / the gather)
    }
    if (p.timed || p.prof) CHK(c, hipEventRecord(p.e[2], c->stream));
    return 0;
}
// k_solve in its forms and K3, on the main stream
static int pass_solve(sca_ctx *c, const PassPlan &p) {
    const DeviceView &d = c->d;
    const int cnt = p.cnt;
    if (p.S.split) hipLaunchKernelGGL(k_solve_pick4, dim3((cnt + SOLVE_WAVES * PICK_APW - 1) / (SOLVE_WAVES * PICK_APW)), dim3(SOLVE_WAVES * 64), 0, c->stream, d, c->P);
    else if (p.S.solve_fb) hipLaunchKernelGGL(k_solve_fb, dim3((cnt + SOLVE_WAVES - 1) / SOLVE_WAVES), dim3(SOLVE_WAVES * 64), 0, c->stream, d, c->P);
    else {
        hipLaunchKernelGGL(k_solve, dim3((cnt + SOLVE_WAVES - 1) / SOLVE_WAVES), dim3(SOLVE_WAVES * 64), 0, c->stream, d, c->P);
        if (p.S.lpw)                                                  // K3, one wavefront per LP agent (few of them)
            hipLaunchKernelGGL(k_solve_lpw, dim3((p.lp_hi - p.lp_lo + SOLVE_WAVES - 1) / SOLVE_WAVES), dim3(SOLVE_WAVES * 64), 0, c->stream, d, c->P,
                               p.lp_ids, p.lp_lo, p.lp_hi);
    }
    if (p.S.lp_kernel)                                                // K3: the LP agents of the shard, one lane each
        hipLaunchKernelGGL(k_lp, dim3((p.lp_hi - p.lp_lo + 63) / 64), dim3(64), 0, c->stream, d, c->P, p.lp_ids, p.lp_lo, p.lp_hi);
    if (p.timed || p.prof) CHK(c, hipEventRecord(p.e[3], c->stream));  // [e2, e3] = k_solve (+ k_lp) (what rocprofv3 reports for them)
    return 0;
}
// the agents without any suitable candidate (rare; one wavefront each), then the epilogue (one lane per agent)
static int pass_epilogue(sca_ctx *c, const PassPlan &p) {
    const DeviceView &d = c->d;
    const int ablocks = (p.cnt + 255) / 256;
    if (p.auto_mode && c->au.waitvalue) {
        // nothing of this pass waited for the kd build any more.  Two things still must: (i) the integrate stage writes the record
        // buffer that the build BEFORE this pass's read its positions from (the two buffers alternate): wait for that build's gather;
        if (int r = wait_if_pending(c, c->stream, c->au.ev_gather[p.A.gather_slot])) return r;
        c->au.unjoined = true;                                          // (ii) see auto_join
    }
    // (small shards: the fallback sweep rides in the epilogue's launch -- k_action_fb -- instead of in front of it)
    const hipEvent_t action_stop = p.fuse_integrate ? p.action_stop : nullptr;
    if (p.S.action_fb) {
        const auto k = p.fuse_integrate ? k_action_fb<true> : k_action_fb<false>;
        LAUNCH_OPT(c, action_stop, k, dim3(ablocks + FB_BLOCKS_SMALL), dim3(SOLVE_WAVES * 64), c->stream, d, c->P, ablocks);
    } else {
        const auto kf = p.fuse_integrate ? k_fallback<true> : k_fallback<false>;
        const auto ka = p.fuse_integrate ? k_action<true> : k_action<false>;
        if (!p.S.solve_fb) hipLaunchKernelGGL(kf, dim3(FB_BLOCKS), dim3(SOLVE_WAVES * 64), 0, c->stream, d, c->P);
        LAUNCH_OPT(c, action_stop, ka, dim3(ablocks), dim3(256), c->stream, d, c->P);
    }
    c->forms = p.forms;
    CHK(c, hipGetLastError());
    if (p.fuse_integrate && c->d.hist) c->d.hist_row++;
    return 0;
}
struct PassRide { hipEvent_t action_stop = nullptr; bool fork_ready = false; };   // what a step of a burst hands to its pass (plan_step); every other caller hands over nothing
static int launch_policy(sca_ctx *c, int mode, bool timed, bool fuse_integrate, const PassRide &ride) {
    PassPlan p{timed, fuse_integrate, ride.action_stop, ride.fork_ready};
    if (int r = pass_resolve(c, mode, p)) return r;
    if (int r = pass_fork(c, p)) return r;
    if (p.tracked) { int f = 0; if (int r = launch_tracker(c, true, true, f)) return r; p.forms |= f; }
    if (int r = pass_structure(c, p)) return r;
    if (int r = pass_query(c, p)) return r;
    if (int r = pass_join(c, p)) return r;
    if (int r = pass_solve(c, p)) return r;
    return pass_epilogue(c, p);
}

static int launch_integrate(sca_ctx *c) {
    hipLaunchKernelGGL(k_integrate, dim3((c->d.shard_count + 255) / 256), dim3(256), 0, c->stream, c->d, c->P);
    CHK(c, hipGetLastError());
    if (c->d.hist) c->d.hist_row++;
    return 0;
}
// ---- the env update (check_agent_state + is_done): its stages in the order launch_collide_finish runs them ---------------------------------------
// no policy pass before: the counters, the candidate lists, the grid and the scenes' step are the update's own to prepare
static int finish_prepare(sca_ctx *c) {
    DeviceView &d = c->d;
    if (!c->near_valid) CHK(c, hipMemsetAsync(d.done_count, 0, sizeof(int32_t) * 256 * 32, c->stream));   // no policy pass before
    if (!c->near_valid) hipLaunchKernelGGL(k_invalidate_near, dim3((d.n + 255) / 256), dim3(256), 0, c->stream, d);
    if (!c->near_valid && c->nbr_mode == SCA_NBR_GRID) {                  // the fallback reads the grid: make it describe these records
        c->grid.skip_prep = 2;
        c->nbr_stream = c->stream;
        if (int r = build_agent_grid_device(c)) return r;
    }
    if (c->scenes.on && !c->scenes.begun) {                                // no policy pass before: the update opens the step itself
        if (int r = scenes_recount(c, c->stream)) return r;
        hipLaunchKernelGGL(k_scene_begin, dim3((c->scenes.v.nscenes + 255) / 256), dim3(256), 0, c->stream, c->scenes.v);
    }
    c->near_valid = false;
    return 0;
}
// what watches the step: a scene's log and closest approach, then the closest approach over the whole context
static int finish_observers(sca_ctx *c) {
    const DeviceView &d = c->d;
    const bool passed = c->scenes.on && c->scenes.begun;                   // a policy pass opened this step: coll_new describes it (k_scene_clearance)
    if (c->scenes.on && c->scenes.log.rows)                                // the scene log's row of this step: behind k_scene_begin, in front of the step's last kernel
        hipLaunchKernelGGL(k_scene_log, dim3((unsigned)((4 * (int64_t)d.n + SCENE_LOG_T - 1) / SCENE_LOG_T)), dim3(SCENE_LOG_T), 0, c->stream, d, c->scenes.v, c->scenes.log);
    if (c->scenes.on && c->scenes.clear) {                                 // the closest approach of this step: beside the log's row, on the same records
        const int T = std::min(256, (c->scenes.largest + 63) / 64 * 64);  // a lane per agent row of the largest scene, whole wavefronts, at most 256
        hipLaunchKernelGGL(k_scene_clearance, dim3(c->scenes.v.nscenes), dim3(T), (size_t)clearance_lds_bytes(c->scenes.largest), c->stream, d, c->scenes.v,
                           (const int32_t *)c->scenes.size, c->scenes.clear, c->scenes.obs_on ? c->scenes.ov.oroot : (const int32_t *)nullptr, c->scenes.obs_on ? 0 : d.m,
                           c->scenes.largest, passed ? (const uint32_t *)d.coll_new : (const uint32_t *)nullptr);
    }
    if (!c->clear) return 0;                                               // the closest approach of this step over the whole context: a wavefront per agent
    // The agent tree of this step.  A kd pass built it on the pass's own streams, joined into this one in front of the solve -- the order
    // K4's traversal relies on.  An AUTO pass built it on the kd stream, which nothing of the step waits for (K4 looks into the grid there):
    // this stream waits for that build here.
    if (c->au.ran) { if (int r = auto_join(c)) return r; }
    double car, cor; clearance_reach(c, car, cor);
    hipLaunchKernelGGL(k_clearance, dim3((unsigned)((d.n + CLR_WAVES - 1) / CLR_WAVES)), dim3(CLR_WAVES * 64), 0, c->stream, d, c->clear, car, cor, ++c->clear_step);
    return 0;
}
// K4 in the instance plan_finish chose
static int finish_k4(sca_ctx *c, int k4, hipEvent_t stop) {
    const DeviceView &d = c->d;
    double agent_reach, obs_reach; collide_reach(c, agent_reach, obs_reach);
    const dim3 grid((d.shard_count + K4_WAVES * K4_APW - 1) / (K4_WAVES * K4_APW)), block(K4_WAVES * 64);
    const int fresh = c->state_fresh ? 1 : 0;                             // (flags came from sca_set_state: arrived agents are checked against obstacles once)
    switch (k4) {
    case K4_SCENE_OBS: LAUNCH_OPT(c, stop, k_collide_finish_scenes<SceneObsRoots>, grid, block, c->stream, d, c->P, agent_reach, obs_reach, fresh, SceneObsRoots{c->scenes.v, c->scenes.ov}); break;
    case K4_SCENES: LAUNCH_OPT(c, stop, k_collide_finish_scenes<SceneRoots>, grid, block, c->stream, d, c->P, agent_reach, obs_reach, fresh, SceneRoots{c->scenes.v}); break;
    case K4_GRID: LAUNCH_OPT(c, stop, k_collide_finish_grid, grid, block, c->stream, d, c->grid, c->P, agent_reach, obs_reach, fresh); break;
    default: LAUNCH_OPT(c, stop, k_collide_finish, grid, block, c->stream, d, c->P, agent_reach, obs_reach, fresh);
    }
    return 0;
}
static int missions_advance(sca_ctx *c);
// `ride`: the event for the step's last kernel, if sca_run_steps hands one over (the next pass's fork).  Afterwards the moved records are the current ones (buffer swap, no copy)
static int launch_collide_finish(sca_ctx *c, bool timed, hipEvent_t ride) {
    DeviceView &d = c->d;
    const FinishPlan f = plan_finish(c->scenes.on, c->scenes.obs_on, c->scenes.hv_host != nullptr, c->part_on, d.shard_count < d.n, c->nbr_mode);
    const auto stop_of = [&](int carrier) { return f.carrier == carrier ? ride : nullptr; };
    if (int r = finish_prepare(c)) return r;
    if (int r = finish_observers(c)) return r;
    if (int r = finish_k4(c, f.k4, stop_of(CARRY_K4))) return r;
    if (c->scenes.on) { c->scenes.begun = false; c->scenes.live_valid = true; }
    if (f.harvest) {                    // the scenes that finished in this step hand over their result; d.rec_new: what K4 just wrote, the current records behind the swap below
        const HarvestDev h{d.rec_new, d.heading, d.total_dist, d.step_num, c->scenes.size, c->scenes.hv_host, c->scenes.hv_layout, ++c->scenes.hv_batch_step};
        LAUNCH_OPT(c, stop_of(CARRY_HARVEST), k_scene_harvest, dim3(c->scenes.v.nscenes), dim3(HARVEST_T), c->stream, c->scenes.v, h);
    }
    c->state_fresh = false;
    if (f.others) {                     // the goal flags of the agents that are not this shard's
        // the partition, sized with the whole present bound: d.shard_count and d.n_present are the host's UPPER bounds (part_bounds clamps the halo bound
        // to n - owned bound, i.e. to 0 for small swarms), so their difference says nothing about the halo count -- the kernel reads the exact counts and
        // returns beyond them (halo copies that arrived at their goal kept flying for their neighbours on this rank for one step)
        const int rows = c->part_on ? std::max(1, d.n_present) : d.n;
        LAUNCH_OPT(c, stop_of(CARRY_OTHERS), k_goal_flags_others, dim3((rows + 255) / 256), dim3(256), c->stream, d, c->P);
    }
    if (c->ms.on) if (int r = missions_advance(c)) return r;    // the rows that ended in this step take their next mission: behind K4, on the records it wrote, in front of the swap
    if (timed) CHK(c, hipEventRecord(c->ev[5], c->stream));
    CHK(c, hipGetLastError());
    std::swap(d.rec, d.rec_new);
    c->h_pos_valid = false;
    return 0;
}
static int update_refuse(sca_ctx *c, const char *who) {                    // (the closest-approach records need this step's agent tree: refused before anything is enqueued)
    return clearance_refuse(c, who, clearance_check(CLR_UPDATE, clearance_state(c), c->near_valid ? 1 : 0, c->nbr_mode == SCA_NBR_GRID && !c->au.ran ? 1 : 0, true, 0));
}

int sca_policy_pass(sca_ctx *c, int neighbor_mode) {
    API_ENTER(c);
    if (int r = step_refuse(c, "", STEP_CHK_STATE, 0, neighbor_mode)) return r;
    if (int r = launch_policy(c, neighbor_mode, true, false, PassRide{})) return r;
    if (int r = auto_join(c)) return r;
    CHK(c, hipStreamSynchronize(c->stream));
    if (neighbor_mode == SCA_NBR_KDTREE || neighbor_mode == SCA_NBR_AUTO) { if (int r = check_kd_overflow(c)) return r; }
    CHK(c, hipEventElapsedTime(&c->ms_nbr, c->ev[0], c->ev[1]));
    CHK(c, hipEventElapsedTime(&c->ms_solve, c->ev[2], c->ev[3]));
    return 0;
}

// K4's counters (and the kd build's error word) in ONE round trip through a pinned buffer: this is the per-step synchronisation of the
// drop-in loop `while not env.step()` (round 4: two pageable copies with a stream synchronisation each)
static int read_active(sca_ctx *c, int *active, bool kd_word) {
    constexpr int PARTS = 256 * 32;
    if (!c->h_done) CHK(c, hipHostMalloc((void **)&c->h_done, sizeof(int32_t) * (PARTS + 1)));
    c->h_done[PARTS] = 0;
    CHK(c, hipMemcpyAsync(c->h_done, c->d.done_count, sizeof(int32_t) * PARTS, hipMemcpyDeviceToHost, c->stream));
    if (kd_word) CHK(c, hipMemcpyAsync(c->h_done + PARTS, c->kd.counts + KD_MAX_LEVELS + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    if (c->h_done[PARTS]) return check_kd_overflow(c);                      // (reports, resets the word)
    int n = 0;
    for (int i = 0; i < PARTS; i += 32) n += c->h_done[i];
    *active = n;
    return 0;
}
int sca_env_update(sca_ctx *c, int *all_done) {
    API_ENTER(c);
    if (int r = step_refuse(c, "", STEP_CHK_STATE, 0, 0)) return r;
    if (int r = update_refuse(c, "sca_env_update")) return r;
    CHK(c, hipEventRecord(c->ev[4], c->stream));
    if (int r = launch_integrate(c)) return r;
    if (int r = launch_collide_finish(c, true, nullptr)) return r;
    if (all_done) {
        int active = 0;
        if (int r = read_active(c, &active, false)) return r;
        CHK(c, hipEventElapsedTime(&c->ms_update, c->ev[4], c->ev[5]));
        *all_done = (active == 0);
    }
    return 0;
}
int sca_active_count(sca_ctx *c, int *active) {
    API_ENTER(c);
    ARG(c, active);
    if (int r = step_refuse(c, "", STEP_CHK_STATE, 0, 0)) return r;
    return read_active(c, active, c->perm_on_device);
}

// the step's exchange: every rank contributes its shard's moved records, in place
static int exchange_moved_records(sca_ctx *c) {
    const size_t bytes = sizeof(PubRec) * (size_t)c->d.shard_count;
    hipEvent_t x0 = nullptr, x1 = nullptr;
    if (c->profiling && c->pool_xch_used + 2 <= 2 * 4096) {              // the collective's device time, on the stream it is enqueued on
        for (hipEvent_t *ev : {&x0, &x1}) if (int r = pool_take(c, c->pool_xch, c->pool_xch_used, 2 * 4096, ev)) return r;
        CHK(c, hipEventRecord(x0, c->stream));
    }
    const ncclResult_t e = g_rccl.AllGather((const char *)c->d.rec_new + sizeof(PubRec) * (size_t)c->d.shard_begin, c->d.rec_new, bytes,
                                            ncclChar, c->comm, c->stream);
    if (e != ncclSuccess) { c->err = std::string("ncclAllGather: ") + g_rccl.GetErrorString(e); return SCA_ERR_HIP; }
    if (x1) CHK(c, hipEventRecord(x1, c->stream));
    return 0;
}

// A failure in the middle of the loop (an exchange, a launch, a partition commit) must not leave the AUTO bookkeeping pointing at a tree
// built ahead from positions the caller is about to replace: forget the build-ahead, let the context's stream wait for whatever
// the kd stream still holds, and have the next AUTO pass decide afresh.
static void auto_abandon(sca_ctx *c) {
    c->au.forget();
    c->au.lazy_join = false; c->au.count_pending = false; c->au.tail_seq = 0; c->au.on_kd = 0;
    if (c->au.stream) { (void)hipStreamSynchronize(c->au.stream); (void)hipGetLastError(); }
    if (c->au.sync) {
        // (tickets of a pass that was cut short: the words start from zero again)
        (void)hipStreamSynchronize(c->stream);
        (void)hipMemset(c->au.sync, 0, 8 * sizeof(unsigned));
        (void)hipGetLastError();
    }
    c->au.unjoined = false;
}
// what plan_step asks of the context, as it stands when it is asked
static StepIn step_in(const sca_ctx *c, int mode, int s, int steps) {
    return StepIn{mode, s, steps, c->au.stream != nullptr, c->tun.ext_stop != 0, c->comm != nullptr, c->d.shard_count == c->n, c->trk_on, c->trk_in_pass, c->trk_fork != nullptr,
                  c->paths_on, c->clear != nullptr, c->au.ran, c->au.fits, c->part_on, c->au.last, c->tun.auto_div, c->au.backoff, c->d.shard_count, c->ms.on, c->vac.on};
}
// between the pass and the update: what the shard moved reaches the others, or what stands in for that
static int step_exchange(sca_ctx *c) {
    if (c->part_on) {                                                      // one rank (or one rank alone, emulation): nobody to exchange with
        if (c->part_nranks > 1) { if (int r = sca_partition_pack(c, c->part_scratch[0], c->part_scratch[1])) return r; }
        if (int r = sca_partition_commit(c)) return r;
    }
    if (c->comm) return exchange_moved_records(c);
    if (c->shard_emulation && !c->part_on && c->d.shard_count < c->n) {      // (partition: the halo copies stand still by themselves)
        // stand-in for the all-gather's arrivals: the other ranks' agents stand still (their records are copied over)
        const int b = c->d.shard_begin, e = b + c->d.shard_count;
        if (b > 0) CHK(c, hipMemcpyAsync(c->d.rec_new, c->d.rec, sizeof(PubRec) * (size_t)b, hipMemcpyDeviceToDevice, c->stream));
        if (e < c->n) CHK(c, hipMemcpyAsync(c->d.rec_new + e, c->d.rec + e, sizeof(PubRec) * (size_t)(c->n - e), hipMemcpyDeviceToDevice, c->stream));
    }
    return 0;
}
// the update, then the NEXT pass's kd build from the moved positions (plan_step says why it may start here)
static int finish_then_build_ahead(sca_ctx *c, bool moved_recorded) {
    // (the collision check goes to its stream FIRST: the host needs ~5 us per launch, and the build's eight or more launches in
    // front of it left the main stream idle for 50 us at N = 4096)
    if (!moved_recorded) CHK(c, hipEventRecord(c->au.ev_moved, c->stream));
    if (int r = launch_collide_finish(c, false, nullptr)) return r;       // (swaps the record buffers: the moved ones are c->d.rec now)
    if (int r = auto_enqueue_kd_build(c, c->au.ev_moved, c->d.rec, true)) return r;
    c->au.ahead = true;
    return 0;
}
static int run_steps_loop(sca_ctx *c, int steps, int neighbor_mode, bool lazy) {
    if (int r = step_refuse(c, "", STEP_CHK_ALL, steps, neighbor_mode)) return r;
    for (int k = 0; k < 2 && c->part_on && c->part_nranks > 1; k++)          // emulation: this rank alone, its messages go nowhere
        if (!c->part_scratch[k]) CHK(c, hipMalloc((void **)&c->part_scratch[k], part_message_bytes(c->part.cap_halo, c->part.cap_mig)));
    bool fork_ready = false;                                               // the fork of step s rode on the last kernel of step s - 1
    for (int s = 0; s < steps; s++) {
        const bool moved = plan_step(step_in(c, neighbor_mode, s, steps)).moved_on_action;
        if (int r = launch_policy(c, neighbor_mode, false, true, PassRide{moved ? c->au.ev_moved : nullptr, fork_ready})) return r;   // integrate fused into k_solve
        if (int r = step_exchange(c)) return r;
        const StepPlan p = plan_step(step_in(c, neighbor_mode, s, steps));  // (behind the pass: Auto::ran and auto_next's inputs are its results)
        fork_ready = p.fork_rides;
        if (p.build_ahead) { if (int r = finish_then_build_ahead(c, moved)) return r; }
        else if (int r = launch_collide_finish(c, false, p.fork_rides ? c->trk_fork : nullptr)) return r;
    }
    if (lazy && c->au.unjoined && c->au.ran) { c->au.lazy_join = true; return 0; }   // (sca_env_step: see API_ENTER)
    return auto_join(c);
}
static int run_steps_guarded(sca_ctx *c, int steps, int neighbor_mode, bool lazy) {
    const int r = run_steps_loop(c, steps, neighbor_mode, lazy);
    if (r != 0) { const std::string keep = c->err; auto_abandon(c); c->err = keep; }
    return r;
}
int sca_run_steps(sca_ctx *c, int steps, int neighbor_mode) {
    API_ENTER(c);
    return run_steps_guarded(c, steps, neighbor_mode, false);
}
int sca_env_step(sca_ctx *c, int neighbor_mode, int *active) {
    if (!c) return SCA_ERR_ARG;                                           // (not API_ENTER: a step after a step needs no join)
    ARG(c, active);
    if (int r = run_steps_guarded(c, 1, neighbor_mode, true)) return r;
    // (the kd build's error word is read from the context's stream: a build still running on the kd stream is seen one step later)
    return read_active(c, active, c->perm_on_device);
}
// ---- the env loop with the host as the owner of the state (mampenv.py:27-59): a pinned state block and one call per step ------------------
int sca_host_state_layout(int n, int64_t *offsets, int64_t *total_bytes) {
    if (n <= 0 || !offsets || !total_bytes) return SCA_ERR_ARG;
    const HostLayout L = host_state_layout(n);
    for (int s = 0; s < HS_SECTIONS; s++) offsets[s] = L.off[s];
    *total_bytes = L.total;
    return 0;
}
static int host_block_alloc(sca_ctx *c) {
    if (c->hs_host && (c->hs_dev || !c->tun.hs_staged)) return 0;
    const size_t bytes = (size_t)host_state_layout(c->max_n).total;       // (every section grows with n: the layout of any n <= max_n fits)
    if (!c->hs_host) {                                                    // mapped into the device's address space and coherent: the kernels access it
        CHK(c, hipHostMalloc((void **)&c->hs_host, bytes, hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(c->hs_host, 0, bytes);
    }
    if (c->tun.hs_staged && !c->hs_dev) {
        CHK(c, hipMalloc((void **)&c->hs_dev, bytes));
        CHK(c, hipMemsetAsync(c->hs_dev, 0, bytes, c->stream));
    }
    return 0;
}
int sca_host_state_get(sca_ctx *c, sca_host_state *out, int32_t struct_bytes) {
    API_ENTER(c);
    ARG(c, out);
    if (struct_bytes < (int32_t)offsetof(sca_host_state, pos) || struct_bytes > (int32_t)sizeof(sca_host_state)) {
        c->err = "sca_host_state_get: struct_bytes must be sizeof(sca_host_state) as the caller compiled it (" +
                 std::to_string(offsetof(sca_host_state, pos)) + " .. " + std::to_string(sizeof(sca_host_state)) + ")";
        return SCA_ERR_ARG;
    }
    if (!c->agents_set) { c->err = "sca_host_state_get: sca_set_agents first (the block's layout is that of the current n)"; return SCA_ERR_STATE; }
    if (int r = host_block_alloc(c)) return r;
    const HostLayout L = host_state_layout(c->n);
    sca_host_state h;
    std::memset(&h, 0, sizeof h);
    h.struct_bytes = struct_bytes; h.n = c->n;
    uint8_t *b = c->hs_host;
    h.pos = (double *)(b + L.off[HS_POS]); h.vel = (float *)(b + L.off[HS_VEL]); h.heading = (double *)(b + L.off[HS_HEADING]);
    h.flags = b + L.off[HS_FLAGS]; h.total_dist = (double *)(b + L.off[HS_TOTAL_DIST]); h.step_num = (int32_t *)(b + L.off[HS_STEP_NUM]);
    h.vpref = (double *)(b + L.off[HS_VPREF]); h.vpref_mode = b + L.off[HS_VPREF_MODE]; h.action = (float *)(b + L.off[HS_ACTION]);
    // only the members that fit entirely into the caller's struct
    size_t fit = offsetof(sca_host_state, pos);
    while (fit + sizeof(void *) <= (size_t)struct_bytes) fit += sizeof(void *);
    std::memcpy(out, &h, fit);
    return 0;
}
// sca_step_host's refusals (and the block's allocation among them, where it always was)
static int host_step_refuse(sca_ctx *c, int neighbor_mode, uint32_t in_mask) {
    if (!c->agents_set) { c->err = "sca_step_host: sca_set_agents first"; return SCA_ERR_STATE; }
    if (int r = step_refuse(c, "sca_step_host: ", STEP_CHK_MODE, 0, neighbor_mode)) return r;
    if (c->comm) { c->err = "sca_step_host with an active communicator: the block is the whole swarm's state on one rank (sca_comm_destroy first)"; return SCA_ERR_UNSUPPORTED; }
    if (c->part_on) { c->err = "sca_step_host under the cell-owner partition: the block is the whole swarm's state on one rank (sca_partition_disable first)"; return SCA_ERR_UNSUPPORTED; }
    if (c->d.shard_count < c->n) { c->err = "sca_step_host on a shard (sca_set_shard with count < n): the block is the whole swarm's state on one rank"; return SCA_ERR_STATE; }
    if (int r = scenes_refuse_partial(c, "sca_step_host")) return r;
    if (!(in_mask & SCA_HOST_IN_STATE) && !c->state_set) { c->err = "sca_step_host: no state yet -- write the block and pass SCA_HOST_IN_STATE (or sca_set_state first)"; return SCA_ERR_STATE; }
    if (in_mask && !c->hs_host) { c->err = "sca_step_host: sca_host_state_get first -- nothing can have been written to a block nobody has fetched"; return SCA_ERR_STATE; }
    if (int r = host_block_alloc(c)) return r;
    if ((in_mask & SCA_HOST_IN_VPREF) && c->paths_on) {                    // sca_set_vpref's rule, on the block's vpref_mode
        const uint8_t *mode = c->hs_host + host_state_layout(c->n).off[HS_VPREF_MODE];
        for (int i = 0; i < c->n; i++)
            if (mode[i] && c->h_path_vpref[i]) {
                c->err = "sca_set_vpref: agent " + std::to_string(i) + " follows a waypoint list (sca_set_paths): its v_pref is its policy's, toward the waypoint";
                return SCA_ERR_ARG;
            }
    }
    return 0;
}
// the device side of the block's two kernels, on the current records; what they read and write is the staging buffer in the staged form
static HostIoDev host_io(const sca_ctx *c) { return HostIoDev{c->d.rec, c->d.heading, c->d.total_dist, c->d.step_num, c->d.vpref_ext, c->d.vpref_mode, c->d.action}; }
static uint8_t *host_io_block(const sca_ctx *c) { return c->tun.hs_staged ? c->hs_dev : c->hs_host; }
// the sections the caller wrote, into the device's arrays
static int host_ingest(sca_ctx *c, uint32_t in_mask) {
    const int n = c->n; const HostLayout L = host_state_layout(n);
    if ((in_mask & SCA_HOST_IN_STATE) && c->scenes.hv_host) {              // sca_set_state's rule for the harvest; the words are the host's to
        CHK(c, hipStreamSynchronize(c->stream));                           // write only while no step is in flight (idle behind a sca_step_host)
        scene_harvest_clear_fresh(c, 0, nullptr);
    }
    if (!in_mask) return 0;
    // (staged form: the up-going sections are contiguous, [pos .. step_num] [vpref, vpref_mode] -- one copy takes what was written)
    const int64_t lo = (in_mask & SCA_HOST_IN_STATE) ? L.off[HS_POS] : L.off[HS_VPREF];
    const int64_t hi = (in_mask & SCA_HOST_IN_VPREF) ? L.off[HS_ACTION] : L.off[HS_VPREF];
    if ((in_mask & SCA_HOST_IN_STATE) && !c->state_set)                   // the first state of this agent set: `radius` reaches the device with it
        CHK(c, hipMemcpyAsync(c->d.rec, c->h_rec.data(), sizeof(PubRec) * n, hipMemcpyHostToDevice, c->stream));
    if (c->tun.hs_staged) CHK(c, hipMemcpyAsync(c->hs_dev + lo, c->hs_host + lo, (size_t)(hi - lo), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_host_ingest, dim3((n + HIO_TILE - 1) / HIO_TILE), dim3(HIO_TILE), 0, c->stream, host_io(c), (const uint8_t *)host_io_block(c), n, in_mask);
    CHK(c, hipGetLastError());
    if (in_mask & SCA_HOST_IN_STATE) { state_replaced(c); c->h_pos_valid = false; }   // (no host mirror of the positions is kept)
    return 0;
}
// the moved state and the action rows, into the block (the step swapped the record arrays: host_io takes the current ones)
static int host_egress(sca_ctx *c) {
    const int n = c->n; const HostLayout L = host_state_layout(n);
    hipLaunchKernelGGL(k_host_egress, dim3((n + HIO_TILE - 1) / HIO_TILE), dim3(HIO_TILE), 0, c->stream, host_io(c), host_io_block(c), n);
    CHK(c, hipGetLastError());
    // (staged form, down: the state sections and the action rows; the caller's v_pref sections between them are never written)
    if (c->tun.hs_staged) CHK(c, hipMemcpyAsync(c->hs_host + L.off[HS_POS], c->hs_dev + L.off[HS_POS], (size_t)(L.off[HS_VPREF] - L.off[HS_POS]), hipMemcpyDeviceToHost, c->stream));
    if (c->tun.hs_staged) CHK(c, hipMemcpyAsync(c->hs_host + L.off[HS_ACTION], c->hs_dev + L.off[HS_ACTION], (size_t)(L.total - L.off[HS_ACTION]), hipMemcpyDeviceToHost, c->stream));
    return 0;
}
int sca_step_host(sca_ctx *c, int neighbor_mode, uint32_t in_mask, int *active) {
    API_ENTER(c);                                                         // (the block replaces or reads state: an AUTO pass's kd stream is joined first)
    ARG(c, active);
    ARG(c, (in_mask & ~(uint32_t)(SCA_HOST_IN_STATE | SCA_HOST_IN_VPREF)) == 0);
    if (int r = missions_standing(c, "sca_step_host", MSF_STEP_HOST)) return r;
    if (int r = vacancy_refuse(c, "sca_step_host")) return r;
    if (int r = host_step_refuse(c, neighbor_mode, in_mask)) return r;
    if (int r = host_ingest(c, in_mask)) return r;
    if (int r = run_steps_guarded(c, 1, neighbor_mode, false)) return r;  // integrate fused into the pass, k_collide_finish; joins the kd stream
    if (int r = host_egress(c)) return r;
    return read_active(c, active, c->perm_on_device);                     // ... and the count (and the kd build's error word): the call's one synchronisation
}
int sca_set_shard_emulation(sca_ctx *c, int on) {
    API_ENTER(c);
    if (c->comm && on) { c->err = "sca_set_shard_emulation with an active communicator: the exchange is real"; return SCA_ERR_STATE; }
    c->shard_emulation = on != 0;
    return 0;
}
int sca_last_pass_forms(sca_ctx *c, int *forms) {
    API_ENTER(c);
    ARG(c, forms);
    *forms = c->forms;
    return 0;
}
int sca_last_kd_build_ms(sca_ctx *c, float *kd_build_ms) {
    API_ENTER(c);
    ARG(c, kd_build_ms);
    *kd_build_ms = c->ms_kd_build;
    return 0;
}
int sca_auto_stats(sca_ctx *c, int64_t *out4, int reset) {
    API_ENTER(c);
    ARG(c, out4);
    for (int k = 0; k < 4; k++) out4[k] = 0;
    if (!c->d.kdq_stats) return 0;                                       // no SCA_NBR_AUTO pass has run
    if (c->au.stream) CHK(c, hipStreamSynchronize(c->au.stream));
    unsigned long long h[4];
    CHK(c, hipMemcpy(h, c->d.kdq_stats, sizeof(h), hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; k++) out4[k] = (int64_t)h[k];
    if (reset) CHK(c, hipMemset(c->d.kdq_stats, 0, sizeof(h)));
    return 0;
}
int sca_last_exchange_ms(sca_ctx *c, float *exchange_ms) {
    API_ENTER(c);
    ARG(c, exchange_ms);
    *exchange_ms = c->ms_exchange;
    return 0;
}
int sca_last_replan_ms(sca_ctx *c, float *replan_ms) {
    API_ENTER(c);
    if (replan_ms) *replan_ms = c->ms_replan;
    return 0;
}

// ---- RCCL inside the library (SURVEY.md 8b `sca_comm_init`, 8e) ---------------------------------------------------------
int sca_comm_probe(void) {
    return rccl_load() ? SCA_ERR_UNSUPPORTED : 0;
}
int sca_comm_unique_id(void *id_out) {
    if (!id_out) return SCA_ERR_ARG;
    if (rccl_load()) return SCA_ERR_UNSUPPORTED;
    ncclUniqueId id;
    if (g_rccl.GetUniqueId(&id) != ncclSuccess) return SCA_ERR_HIP;
    std::memcpy(id_out, &id, sizeof(id));
    return 0;
}
int sca_comm_init(sca_ctx *c, int rank, int nranks, const void *unique_id) {
    API_ENTER(c);
    ARG(c, unique_id && nranks >= 1 && rank >= 0 && rank < nranks);
    if (!c->agents_set) { c->err = "sca_set_agents first"; return SCA_ERR_STATE; }
    if (c->comm) { c->err = "communicator already initialised (sca_comm_destroy first)"; return SCA_ERR_STATE; }
    if (c->part_on) { c->err = "sca_comm_init with the cell-owner partition active"; return SCA_ERR_STATE; }
    if (c->scenes.on) { c->err = "sca_comm_init with scenes set (sca_set_scenes): scenes are one rank's"; return SCA_ERR_UNSUPPORTED; }
    if (int r = vacancy_refuse(c, "sca_comm_init")) return r;
    if (int r = clearance_refuse(c, "sca_comm_init", clearance_check(CLR_COMM_INIT, clearance_state(c), 0, 0, true, 0))) return r;
    if (int r = missions_standing(c, "sca_comm_init", MSF_COMM)) return r;
    if (c->n % nranks) { c->err = "agent count must be a multiple of the rank count"; return SCA_ERR_ARG; }
    if (const char *e = rccl_load()) { c->err = e; return SCA_ERR_UNSUPPORTED; }
    CHK(c, hipSetDevice(c->device));
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    const ncclResult_t e = g_rccl.CommInitRank(&c->comm, nranks, id, rank);
    if (e != ncclSuccess) { c->comm = nullptr; c->err = std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(e); return SCA_ERR_HIP; }
    c->comm_rank = rank; c->comm_nranks = nranks;
    c->d.shard_count = c->n / nranks; c->d.shard_begin = rank * c->d.shard_count;
    return 0;
}
int sca_comm_destroy(sca_ctx *c) {
    API_ENTER(c);
    if (c->comm) {
        CHK(c, hipStreamSynchronize(c->stream));
        (void)g_rccl.CommDestroy(c->comm);
        c->comm = nullptr; c->comm_rank = 0; c->comm_nranks = 1;
        c->d.shard_begin = 0; c->d.shard_count = c->n;
    }
    return 0;
}

// ---- cell-owner partition of SCA_NBR_GRID with halo exchange (sca_partition.hip.h) ---------------------
static void part_view(sca_ctx *c) {
    c->d.own = c->d.present = c->part.present[c->part.cur];
    c->d.count_dev = c->part.counts;
    c->d.shard_begin = 0;
    // launch BOUNDS (the kernels read the exact counts, shard_size / present_count): never 0 -- a rank that owns nothing right after
    // sca_partition_init or sca_set_state, where the bounds are the exact counts, would otherwise launch empty grids
    c->d.shard_count = std::max(1, c->part_counts[0]);
    c->d.n_present = std::max(c->d.shard_count, c->part_counts[0] + c->part_counts[1]);
}
static int part_free(sca_ctx *c) {
    if (!c->part_on && !c->part.counts) return 0;
    CHK(c, hipStreamSynchronize(c->stream));
    for (void *q : {(void *)c->part.present[0], (void *)c->part.present[1], (void *)c->part.halo_tmp, (void *)c->part.counts, (void *)c->part.emig})
        if (q) (void)hipFree(q);
    if (c->part_host) { (void)hipHostFree(c->part_host); c->part_host = nullptr; }
    for (int k = 0; k < 2; k++) if (c->part_scratch[k]) { (void)hipFree(c->part_scratch[k]); c->part_scratch[k] = nullptr; }
    if (c->part_ev) { (void)hipEventDestroy(c->part_ev); c->part_ev = nullptr; }
    c->part = PartDev{};
    c->part_on = false; c->part_rank = 0; c->part_nranks = 1; c->part_pending = false;
    c->d.own = c->d.present = nullptr; c->d.count_dev = nullptr; c->d.n_present = 0;
    c->d.shard_begin = 0; c->d.shard_count = c->n;
    return 0;
}
// The launch bounds from what the host knows: the exact counts of a commit one or two steps back + room for what can have
// arrived since.  Agents move 0.1 m per step and cells are 10 m wide, so a step changes an owner's count by the few agents within
// 0.1 m of a cut; the margin is a sixteenth of the rank's agents (+ 4096) per commit of age -- and k_part_keep checks it: a launch
// that turned out too small sets an error bit instead of leaving agents out silently.
static void part_bounds(sca_ctx *c) {
    const long long grow = (long long)c->part_age + 1;
    c->part_counts[0] = (int)std::min<long long>(c->n, c->part_known[0] + grow * (c->part_known[0] / 16 + 4096));
    c->part_counts[1] = (int)std::min<long long>(c->n, c->part_known[1] + grow * (c->part_known[1] / 4 + 4096));
    if (c->part_counts[0] + c->part_counts[1] > c->n) c->part_counts[1] = c->n - c->part_counts[0];
}
static int part_report(sca_ctx *c, int bits) {
    if (!bits) return 0;
    c->err = bits & 4 ? "partition: owned + halo exceed the agent count (corrupt lists)"
           : bits & 8 ? "partition: a rank's agent count outgrew the launch bound between two read-backs (results of that step are incomplete)"
                      : "partition: a halo / migration message overflowed its capacity (sca_partition_init caps)";
    return SCA_ERR_STATE;
}
// lists being built -> current lists (behind k_part_close), without waiting for the device: the counts move on the device, the
// host asks for a copy and sizes its launches with bounds until it has arrived.  wait: get the exact counts now.
static int part_adopt(sca_ctx *c, bool wait) {
    c->part.cur ^= 1;
    c->part_age++;
    if (c->part_pending) c->part_copy_age++;
    if (c->part_pending && hipEventQuery(c->part_ev) == hipSuccess) {
        c->part_known[0] = c->part_host[0]; c->part_known[1] = c->part_host[1]; c->part_counts[4] = c->part_host[4];
        c->part_age = c->part_copy_age;                                     // commits since that snapshot
        c->part_pending = false;
    }
    if (!c->part_pending || wait) {
        if (c->part_pending) CHK(c, hipEventSynchronize(c->part_ev));
        CHK(c, hipMemcpyAsync(c->part_host, c->part.counts, sizeof(int) * 5, hipMemcpyDeviceToHost, c->stream));   // a snapshot behind this commit
        CHK(c, hipEventRecord(c->part_ev, c->stream));
        c->part_copy_age = 0;
        c->part_pending = true;
    }
    if (wait) {
        CHK(c, hipEventSynchronize(c->part_ev));
        c->part_known[0] = c->part_host[0]; c->part_known[1] = c->part_host[1]; c->part_counts[4] = c->part_host[4];
        c->part_age = 0; c->part_pending = false;
        c->part_counts[0] = c->part_known[0]; c->part_counts[1] = c->part_known[1];
    } else part_bounds(c);
    part_view(c);
    return part_report(c, c->part_counts[4]);
}
static int part_classify(sca_ctx *c) {                                      // from records every rank holds completely
    const int n = c->n;
    CHK(c, hipMemsetAsync(c->part.counts, 0, sizeof(int) * 16, c->stream));
    hipLaunchKernelGGL(k_part_init, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d, c->part);
    hipLaunchKernelGGL(k_part_init_halo, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d, c->part);
    hipLaunchKernelGGL(k_part_close<false>, dim3(64), dim3(256), 0, c->stream, c->d, c->part);
    CHK(c, hipGetLastError());
    CHK(c, hipMemcpyAsync(c->part.counts, c->part.counts + 2, sizeof(int) * 2, hipMemcpyDeviceToDevice, c->stream));   // current = built
    CHK(c, hipMemsetAsync(c->part.counts + 2, 0, sizeof(int) * 2, c->stream));
    return part_adopt(c, true);
}
int sca_partition_init(sca_ctx *c, int rank, int nranks, int axis, const double *cuts, int cap_halo, int cap_mig) {
    // (per-agent solver attributes -- sca_set_agent_params, like every static per-agent input indexed by GLOBAL id and replicated on every
    // rank -- need nothing of the messages: the slabs are cut in cells of the LARGEST neighborDist (c->P is the envelope), so one layer of
    // cells is a halo wide enough for every agent's own range, and the collision reach is the largest step's)
    API_ENTER(c);
    ARG(c, nranks >= 1 && rank >= 0 && rank < nranks && axis >= 0 && axis <= 2 && cap_halo >= 0 && cap_mig >= 0);
    if (!c->agents_set || !c->state_set) { c->err = "sca_set_agents and sca_set_state (the complete state, on every rank) first"; return SCA_ERR_STATE; }
    if (c->comm) { c->err = "sca_partition_init with an active communicator (the all-gather mode)"; return SCA_ERR_STATE; }
    if (int r = vacancy_refuse(c, "sca_partition_init")) return r;
    if (c->scenes.on) { c->err = "sca_partition_init with scenes set (sca_set_scenes): a mode of SCA_NBR_GRID, which has no scene form"; return SCA_ERR_UNSUPPORTED; }
    if (c->paths_on) { c->err = "sca_partition_init with waypoint lists set (sca_set_paths): path state does not migrate with the agents"; return SCA_ERR_UNSUPPORTED; }
    if (int r = clearance_refuse(c, "sca_partition_init", clearance_check(CLR_PARTITION_INIT, clearance_state(c), 0, 0, true, 0))) return r;
    if (int r = missions_standing(c, "sca_partition_init", MSF_PARTITION)) return r;
    if (int r = part_free(c)) return r;
    const int n = c->n;
    const double inv_cell = grid_inv_cell(c->P.neighbor_dist);
    // the cuts: given (coordinates along the axis, nranks - 1 of them, ascending), or equal shares of the agents as they stand
    // now; moved onto cell boundaries either way.  Identical on every rank: they all hold the same state.
    std::vector<long long> cell_cut((size_t)nranks + 1);
    cell_cut[0] = LLONG_MIN; cell_cut[nranks] = LLONG_MAX;
    if (cuts) {
        for (int r = 1; r < nranks; r++) cell_cut[r] = (long long)std::floor(cuts[r - 1] * inv_cell);
    } else {
        if (int r = fetch_records(c)) return r;
        std::vector<long long> cells((size_t)n);
        for (int i = 0; i < n; i++) {
            const PubRec &q = c->h_rec[i];
            cells[i] = (long long)std::floor((axis == 0 ? q.px : (axis == 1 ? q.py : q.pz)) * inv_cell);
        }
        std::sort(cells.begin(), cells.end());
        for (int r = 1; r < nranks; r++) cell_cut[r] = cells[(size_t)((long long)r * n / nranks)];
    }
    // an INTERIOR rank needs two layers of cells: with one, an agent that migrates into it lands in a cell that is the next rank's
    // halo layer as well, and that rank hears of it one step late (only the sender's two slab neighbours get messages)
    for (int r = 2; r < nranks; r++)
        if (cell_cut[r] - cell_cut[r - 1] < 2) { c->err = "partition: the cuts leave an interior rank fewer than two layers of cells (too many ranks for this swarm along this axis)"; return SCA_ERR_ARG; }
    if (nranks > 1 && cell_cut[1] == LLONG_MIN) { c->err = "partition: bad cut"; return SCA_ERR_ARG; }
    PartDev &P = c->part;
    for (int k = 0; k < 2; k++) CHK(c, hipMalloc((void **)&P.present[k], sizeof(int32_t) * n));
    CHK(c, hipMalloc((void **)&P.halo_tmp, sizeof(int32_t) * n));
    CHK(c, hipMalloc((void **)&P.counts, sizeof(int32_t) * 16));
    CHK(c, hipMalloc((void **)&P.emig, n));
    for (int k = 0; k < 2; k++) CHK(c, hipMemsetAsync(P.present[k], 0, sizeof(int32_t) * n, c->stream));   // entries beyond the exact counts are
    CHK(c, hipMemsetAsync(P.halo_tmp, 0, sizeof(int32_t) * n, c->stream));                                  // never meant to be read; if a bound
    CHK(c, hipMemsetAsync(P.emig, 0, n, c->stream));                                                        // slips, the read is agent 0, not garbage
    CHK(c, hipHostMalloc((void **)&c->part_host, sizeof(int) * 8));
    CHK(c, hipEventCreateWithFlags(&c->part_ev, hipEventDisableTiming));
    c->part_pending = false; c->part_age = 0;
    P.cur = 0; P.axis = axis; P.inv_cell = inv_cell;
    P.lo_cell = cell_cut[rank]; P.hi_cell = cell_cut[rank + 1];
    P.has_peer[0] = rank > 0; P.has_peer[1] = rank + 1 < nranks;
    P.cap_halo = cap_halo > 0 ? cap_halo : std::max(1024, n / 4);
    P.cap_mig = cap_mig > 0 ? cap_mig : std::max(256, n / 16);
    P.trk_st = c->trk_on ? c->trk.st : nullptr;
    P.trk_nbr0 = c->trk_on ? c->trk.nbr0 : nullptr;
    c->part_on = true; c->part_rank = rank; c->part_nranks = nranks;
    return part_classify(c);
}
int sca_partition_disable(sca_ctx *c) {
    API_ENTER(c);
    return part_free(c);
}
int64_t sca_partition_message_bytes(sca_ctx *c) {
    if (!c || !c->part_on) return 0;
    return (int64_t)part_message_bytes(c->part.cap_halo, c->part.cap_mig);
}
int sca_partition_counts(sca_ctx *c, int *owned, int *halo) {
    API_ENTER(c);
    if (!c->part_on) { c->err = "sca_partition_init first"; return SCA_ERR_STATE; }
    int h[5];
    CHK(c, hipMemcpyAsync(h, c->part.counts, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    if (owned) *owned = h[0];
    if (halo) *halo = h[1];
    return part_report(c, h[4]);
}
int sca_partition_owned(sca_ctx *c, int32_t *ids, int *count) {
    API_ENTER(c);
    ARG(c, ids && count);
    if (!c->part_on) { c->err = "sca_partition_init first"; return SCA_ERR_STATE; }
    CHK(c, hipMemcpyAsync(count, c->part.counts, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    CHK(c, hipMemcpyAsync(ids, c->part.present[c->part.cur], sizeof(int32_t) * (size_t)*count, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
int sca_partition_pack(sca_ctx *c, void *device_buf_lower, void *device_buf_upper) {
    API_ENTER(c);
    if (!c->part_on) { c->err = "sca_partition_init first"; return SCA_ERR_STATE; }
    ARG(c, (device_buf_lower || !c->part.has_peer[0]) && (device_buf_upper || !c->part.has_peer[1]));
    c->part.trk_st = c->trk_on ? c->trk.st : nullptr;
    c->part.trk_nbr0 = c->trk_on ? c->trk.nbr0 : nullptr;
    const int cnt = std::max(1, c->d.shard_count);
    hipLaunchKernelGGL(k_part_pack, dim3((cnt + 255) / 256), dim3(256), 0, c->stream, c->d, c->part,
                       c->part.has_peer[0] ? (uint8_t *)device_buf_lower : nullptr, c->part.has_peer[1] ? (uint8_t *)device_buf_upper : nullptr);
    CHK(c, hipGetLastError());
    return 0;
}
int sca_partition_unpack(sca_ctx *c, const void *device_buf_lower, const void *device_buf_upper) {
    API_ENTER(c);
    if (!c->part_on) { c->err = "sca_partition_init first"; return SCA_ERR_STATE; }
    ARG(c, (device_buf_lower || !c->part.has_peer[0]) && (device_buf_upper || !c->part.has_peer[1]));
    if (!c->part.has_peer[0] && !c->part.has_peer[1]) return 0;
    const int lanes = std::max(c->part.cap_halo, c->part.cap_mig);
    hipLaunchKernelGGL(k_part_unpack, dim3((lanes + 255) / 256), dim3(256), 0, c->stream, c->d, c->part,
                       c->part.has_peer[0] ? (const uint8_t *)device_buf_lower : nullptr, c->part.has_peer[1] ? (const uint8_t *)device_buf_upper : nullptr);
    CHK(c, hipGetLastError());
    return 0;
}
int sca_partition_commit(sca_ctx *c) {
    API_ENTER(c);
    if (!c->part_on) { c->err = "sca_partition_init first"; return SCA_ERR_STATE; }
    const int cnt = std::max(1, c->d.shard_count);
    hipLaunchKernelGGL(k_part_keep, dim3((cnt + 255) / 256), dim3(256), 0, c->stream, c->d, c->part);
    hipLaunchKernelGGL(k_part_close<true>, dim3(16), dim3(256), 0, c->stream, c->d, c->part);
    CHK(c, hipGetLastError());
    return part_adopt(c, false);
}

int sca_step_begin(sca_ctx *c, int neighbor_mode) {
    API_ENTER(c);
    if (int r = step_refuse(c, "", STEP_CHK_STATE | STEP_CHK_PART_MODE, 0, neighbor_mode)) return r;   // (a mode out of range: the pass refuses it)
    if (int r = launch_policy(c, neighbor_mode, false, true, PassRide{})) return r;
    return auto_join(c);                                                  // (the caller may read anything between the two halves of a step)
}
int sca_step_end(sca_ctx *c) {
    API_ENTER(c);
    if (int r = update_refuse(c, "sca_step_end")) return r;
    return launch_collide_finish(c, false, nullptr);
}

int sca_synchronize(sca_ctx *c) {
    API_ENTER(c);
    CHK(c, hipStreamSynchronize(c->stream));
    if (c->part_on) { int h[5]; CHK(c, hipMemcpy(h, c->part.counts, sizeof(h), hipMemcpyDeviceToHost)); if (int r = part_report(c, h[4])) return r; }
    if (c->perm_on_device) { if (int r = check_kd_overflow(c)) return r; }
    if (c->profiling && c->pool_used >= 4) {
        if (int r = pool_mean_ms(c, c->pool, c->pool_used, 4, 0, &c->ms_nbr)) return r;        // K1, on the stream it ran on
        if (int r = pool_mean_ms(c, c->pool, c->pool_used, 4, 2, &c->ms_solve)) return r;      // k_solve (+ k_lp)
        c->pool_used = 0;
    }
    if (c->profiling && c->pool_kd_used >= 2) {
        if (c->au.stream) CHK(c, hipStreamSynchronize(c->au.stream));
        if (c->trk_stream) CHK(c, hipStreamSynchronize(c->trk_stream));
        if (int r = pool_mean_ms(c, c->pool_kd, c->pool_kd_used, 2, 0, &c->ms_kd_build)) return r;
        c->pool_kd_used = 0;
    }
    if (c->profiling && c->pool_xch_used >= 2) {
        if (int r = pool_mean_ms(c, c->pool_xch, c->pool_xch_used, 2, 0, &c->ms_exchange)) return r;
        c->pool_xch_used = 0;
    }
    if (c->profiling && c->pool_trk_used >= 2) {
        if (c->trk_stream) CHK(c, hipStreamSynchronize(c->trk_stream));
        if (int r = pool_mean_ms(c, c->pool_trk, c->pool_trk_used, 2, 0, &c->ms_replan)) return r;
        c->pool_trk_used = 0;
    }
    return 0;
}

int sca_set_profiling(sca_ctx *c, int on) {
    API_ENTER(c);
    c->profiling = on != 0;
    c->pool_used = c->pool_trk_used = c->pool_xch_used = c->pool_kd_used = 0;
    c->prof_tick = 0;
    return 0;
}

int sca_agent_steps(sca_ctx *c, int64_t *count, int reset) {
    API_ENTER(c);
    std::vector<unsigned long long> parts(256 * 16);
    CHK(c, hipMemcpyAsync(parts.data(), c->d.agent_steps, sizeof(unsigned long long) * parts.size(), hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    unsigned long long v = 0;
    for (unsigned long long x : parts) v += x;
    if (count) *count = (int64_t)v;
    if (reset) {
        CHK(c, hipMemsetAsync(c->d.agent_steps, 0, sizeof(unsigned long long) * parts.size(), c->stream));
        CHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}

#ifdef SCA_KB_TIMING
int sca_debug_read_ps(sca_ctx *c, int *out, int count) {      // debug builds only: k_kd_block's per-phase ticks
    CHK(c, hipStreamSynchronize(c->stream));
    CHK(c, hipMemcpy(out, c->kd.ps, sizeof(int) * count, hipMemcpyDeviceToHost));
    return 0;
}
#endif

#ifdef SCA_TIMELINE
// debug builds only (SCA_BUILD_DEFS=-DSCA_TIMELINE): the device-side timeline of the next TL_RING steps (tools/device_timeline.py)
int sca_debug_timeline_enable(sca_ctx *c) {
    API_ENTER(c);
    const size_t cells = (size_t)TL_KERNELS * TL_RING;
    if (!c->d.tl) CHK(c, hipMalloc((void **)&c->d.tl, sizeof(unsigned long long) * 2 * cells));
    std::vector<unsigned long long> init(2 * cells);
    for (size_t i = 0; i < cells; i++) { init[2 * i] = ~0ull; init[2 * i + 1] = 0ull; }
    CHK(c, hipDeviceSynchronize());
    CHK(c, hipMemcpy(c->d.tl, init.data(), sizeof(unsigned long long) * 2 * cells, hipMemcpyHostToDevice));
    c->d.tl_step = -1;                                                  // the next pass is ring entry 0
    return 0;
}
int sca_debug_timeline_read(sca_ctx *c, unsigned long long *out /*[TL_KERNELS][TL_RING][2]*/, int *kernels, int *ring) {
    if (!c || !c->d.tl) return SCA_ERR_ARG;
    CHK(c, hipDeviceSynchronize());
    CHK(c, hipMemcpy(out, c->d.tl, sizeof(unsigned long long) * 2 * TL_KERNELS * TL_RING, hipMemcpyDeviceToHost));
    *kernels = TL_KERNELS; *ring = TL_RING;
    return 0;
}
#endif

#ifdef SCA_KT_TIMING
int sca_debug_read_kdq(sca_ctx *c, int *out, int count) {     // debug builds only: k_track's per-phase ticks
    CHK(c, hipDeviceSynchronize());
    CHK(c, hipMemcpy(out, c->d.kdq_list, sizeof(int) * (count < 16 ? count : 16), hipMemcpyDeviceToHost));
    if (count >= 48) CHK(c, hipMemcpyFromSymbol(out + 16, HIP_SYMBOL(sca_dubins::g_td_ticks), sizeof(int) * 32));
    return 0;
}
#endif

int sca_selftest_l3norm(sca_ctx *c, int n, const double *a, const double *b, double *fast, double *exact) {
    API_ENTER(c);
    ARG(c, n > 0 && a && b && fast && exact);
    double *da = nullptr, *db = nullptr, *df = nullptr, *de = nullptr;
    CHK(c, hipMalloc((void **)&da, sizeof(double) * 3 * n)); CHK(c, hipMalloc((void **)&db, sizeof(double) * 3 * n));
    CHK(c, hipMalloc((void **)&df, sizeof(double) * n)); CHK(c, hipMalloc((void **)&de, sizeof(double) * n));
    CHK(c, hipMemcpyAsync(da, a, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
    CHK(c, hipMemcpyAsync(db, b, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_selftest_l3norm, dim3((n + 63) / 64), dim3(64), 0, c->stream, da, db, n, df, de);
    CHK(c, hipMemcpyAsync(fast, df, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipMemcpyAsync(exact, de, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(df); (void)hipFree(de);
    return 0;
}

// the restated glibc functions (sca_glibc_math.h): fn 0 sin(a), 1 cos(a), 2 acos(a), 3 atan2(a, b), 4 pow(a, 2) in the branch-free
// forms the kernels call; 5 sin, 6 cos, 7 atan2, 8 pow as the literal restatements (glibc's control flow); 9 / 10 the sine / cosine
// of the fused sincos; 11 atan2, 12 sin, 13 cos, 14 pow(a, 2) as the policy epilogue and the env update call them (sca_core.h m_*)
static double libm_eval_host(int fn, double a, double b) {
    double s2, c2;
    switch (fn) {
    case 0: return sca_gm::g_sin(a);
    case 1: return sca_gm::g_cos(a);
    case 2: return sca_gm::g_acos(a);
    case 3: return sca_gm::g_atan2(a, b);
    case 4: return sca_gm::g_pow2(a);
    case 5: return sca_gm::g_sin_ref(a);
    case 6: return sca_gm::g_cos_ref(a);
    case 7: return sca_gm::g_atan2_ref(a, b);
    case 8: return sca_gm::g_pow2_ref(a);
    case 9: sca_gm::g_sincos(a, s2, c2); return s2;
    case 10: sca_gm::g_sincos(a, s2, c2); return c2;
    case 11: return sca::m_atan2(a, b);
    case 12: sca::m_sincos(a, s2, c2); return s2;
    case 13: sca::m_sincos(a, s2, c2); return c2;
    default: return sca::m_pow2(a);
    }
}
int sca_selftest_libm_host(int fn, int n, const double *a, const double *b, double *out) {
    if (fn < 0 || fn > 14 || n < 0 || !a || !out || ((fn == 3 || fn == 7 || fn == 11) && !b)) return SCA_ERR_ARG;
    for (int i = 0; i < n; i++) out[i] = libm_eval_host(fn, a[i], b ? b[i] : 0.0);
    return 0;
}
int sca_selftest_libm(sca_ctx *c, int fn, int n, const double *a, const double *b, double *out) {
    API_ENTER(c);
    ARG(c, fn >= 0 && fn <= 14 && n > 0 && a && out && ((fn != 3 && fn != 7 && fn != 11) || b));
    double *da = nullptr, *db = nullptr, *dout = nullptr;
    for (double **p : {&da, &db, &dout}) CHK(c, hipMalloc((void **)p, sizeof(double) * n));
    CHK(c, hipMemcpyAsync(da, a, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    if (b) CHK(c, hipMemcpyAsync(db, b, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    else CHK(c, hipMemsetAsync(db, 0, sizeof(double) * n, c->stream));
    hipLaunchKernelGGL(k_selftest_libm, dim3((n + 255) / 256), dim3(256), 0, c->stream, fn, da, db, n, dout);
    CHK(c, hipMemcpyAsync(out, dout, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    for (double *p : {da, db, dout}) (void)hipFree(p);
    return 0;
}

// ---- trajectory log (Agent.history_info, agent.py:75-77,126-148) kept in HBM --------------------------------------
int sca_history_enable(sca_ctx *c, int capacity_rows) {
    if (!c || capacity_rows < 0) return SCA_ERR_ARG;
    if (int r_ = api_enter(c)) return r_;
    if (c->n <= 0) { c->err = "sca_set_agents first"; return SCA_ERR_STATE; }
    CHK(c, hipStreamSynchronize(c->stream));
    if (c->d.hist) { CHK(c, hipFree(c->d.hist)); c->d.hist = nullptr; }
    c->d.hist_cap = 0; c->d.hist_row = 0;
    if (capacity_rows == 0) return 0;
    CHK(c, hipMalloc((void **)&c->d.hist, sizeof(HistRow) * (size_t)capacity_rows * (size_t)c->n));
    c->d.hist_cap = capacity_rows;
    return 0;
}
int sca_history_rows(sca_ctx *c, int *rows_logged, int *rows_dropped) {
    API_ENTER(c);
    const int r = c->d.hist ? c->d.hist_row : 0;
    if (rows_logged) *rows_logged = std::min(r, c->d.hist_cap);
    if (rows_dropped) *rows_dropped = std::max(0, r - c->d.hist_cap);
    return 0;
}
int sca_get_history(sca_ctx *c, int first_row, int nrows, int agent_begin, int agent_count, double *pos, double *heading, float *vel) {
    API_ENTER(c);
    if (!c->d.hist) { c->err = "sca_history_enable first"; return SCA_ERR_STATE; }
    const int have = std::min(c->d.hist_row, c->d.hist_cap);
    if (first_row < 0 || nrows < 0 || first_row + nrows > have || agent_begin < 0 || agent_count < 0 || agent_begin + agent_count > c->n) {
        c->err = "history window out of range"; return SCA_ERR_ARG;
    }
    if (nrows == 0 || agent_count == 0) return 0;
    std::vector<HistRow> tmp((size_t)nrows * agent_count);
    CHK(c, hipMemcpy2DAsync(tmp.data(), sizeof(HistRow) * (size_t)agent_count,
                            c->d.hist + (size_t)first_row * c->n + agent_begin, sizeof(HistRow) * (size_t)c->n,
                            sizeof(HistRow) * (size_t)agent_count, (size_t)nrows, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < tmp.size(); i++) {
        const HistRow &h = tmp[i];
        if (pos) { pos[3 * i] = h.px; pos[3 * i + 1] = h.py; pos[3 * i + 2] = h.pz; }
        if (heading) { heading[3 * i] = h.a; heading[3 * i + 1] = h.b; heading[3 * i + 2] = h.g; }
        if (vel) { vel[3 * i] = h.vx; vel[3 * i + 1] = h.vy; vel[3 * i + 2] = h.vz; }
    }
    return 0;
}

// ---- a trajectory log per scene (include/sca_hip.h; the rules and the layout are sca_scenes.h's, the kernel is k_scene_log) ------------------
// the scenes' step counts as far as their rows are written: between a policy pass and its env update a live scene's counter is one ahead
// of its log (scene_begin_one has counted the step, k_scene_log has not run).  One copy, one synchronisation.
static int scene_log_steps(sca_ctx *c, std::vector<int32_t> &steps) {
    const int B = c->scenes.v.nscenes;
    std::vector<int32_t> h(2 * (size_t)B);                                 // prev | steps stand side by side behind the live lines
    CHK(c, hipMemcpyAsync(h.data(), c->scenes.v.prev, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    steps.assign(h.begin() + B, h.end());
    if (c->scenes.begun) for (int s = 0; s < B; s++) if (h[s] > 0) steps[s] -= 1;
    return 0;
}
static int scene_log_refuse(sca_ctx *c, const char *who, const SceneLogCheck &k) {
    switch (k.fault) {
    case SCENE_LOG_OK: return 0;
    case SCENE_LOG_NO_SCENES: c->err = std::string(who) + ": no scenes -- sca_set_scenes first"; break;
    case SCENE_LOG_MID_STEP: c->err = std::string(who) + " between a policy pass and its env update: finish the step first"; break;
    case SCENE_LOG_STEPPED: c->err = std::string(who) + ": scene " + std::to_string(k.scene) + " has taken a step already -- enable the log behind sca_set_scenes / sca_set_state, before the first step"; break;
    case SCENE_LOG_OFF: c->err = std::string(who) + ": sca_scene_history_enable first"; break;
    case SCENE_LOG_BAD_CAPACITY: c->err = std::string(who) + ": capacity_rows must not be negative"; break;
    case SCENE_LOG_BAD_SCENE: c->err = std::string(who) + ": scene " + std::to_string(k.scene) + " is not a scene of this context (0 .. " + std::to_string(c->scenes.v.nscenes - 1) + ")"; break;
    case SCENE_LOG_BAD_ROWS: c->err = std::string(who) + ": row window outside the rows scene " + std::to_string(k.scene) + " has logged"; break;
    default: c->err = std::string(who) + ": agent window outside the agents scene " + std::to_string(k.scene) + " holds";
    }
    return scene_log_error_code(k.fault);
}
int sca_scene_history_enable(sca_ctx *c, int capacity_rows) {
    API_ENTER(c);
    const int B = c->scenes.on ? c->scenes.v.nscenes : 0;
    std::vector<int32_t> steps;
    if (B > 0 && !c->scenes.begun && capacity_rows > 0) { if (int r = scene_log_steps(c, steps)) return r; }
    if (int r = scene_log_refuse(c, "sca_scene_history_enable", scene_log_enable_check(B, c->scenes.begun, steps.data(), capacity_rows))) return r;
    HistRow *rows = nullptr;
    if (capacity_rows > 0) CHK(c, hipMalloc((void **)&rows, (size_t)scene_log_bytes(capacity_rows, c->n)));   // (before the old log goes: a refused call changes nothing)
    if (int r = scene_log_drop(c)) { if (rows) (void)hipFree(rows); return r; }
    c->scenes.log.rows = rows; c->scenes.log.capacity = rows ? capacity_rows : 0;
    return 0;
}
int sca_scene_history_rows(sca_ctx *c, int32_t *rows_logged, int32_t *rows_dropped) {
    API_ENTER(c);
    const int B = c->scenes.on ? c->scenes.v.nscenes : 0;
    if (int r = scene_log_refuse(c, "sca_scene_history_rows", scene_log_check(B, nullptr, c->scenes.log.rows != nullptr, c->scenes.log.capacity, false, 0, 0, 0, 0, 0, 0))) return r;
    std::vector<int32_t> steps;
    if (int r = scene_log_steps(c, steps)) return r;
    for (int s = 0; s < B; s++) {
        if (rows_logged) rows_logged[s] = scene_log_rows_logged(steps[s], c->scenes.log.capacity);
        if (rows_dropped) rows_dropped[s] = scene_log_rows_dropped(steps[s], c->scenes.log.capacity);
    }
    return 0;
}
int sca_get_scene_history(sca_ctx *c, int scene, int first_row, int nrows, int agent_begin, int agent_count, double *pos, double *heading, float *vel) {
    API_ENTER(c);
    const int B = c->scenes.on ? c->scenes.v.nscenes : 0;
    const SceneLogView &L = c->scenes.log;
    const int32_t *off = c->scenes.h_off.data();
    // the faults that need no device value first (an empty row window passes this round), then the row window against the scene's step count
    if (int r = scene_log_refuse(c, "sca_get_scene_history", scene_log_check(B, off, L.rows != nullptr, L.capacity, true, scene, 0, 0, 0, agent_begin, agent_count, c->scenes.h_size.data()))) return r;
    std::vector<int32_t> steps;
    if (int r = scene_log_steps(c, steps)) return r;
    if (int r = scene_log_refuse(c, "sca_get_scene_history", scene_log_check(B, off, true, L.capacity, true, scene, steps[scene], first_row, nrows, agent_begin, agent_count, c->scenes.h_size.data()))) return r;
    if (nrows == 0 || agent_count == 0) return 0;
    // rows [first_row, first_row + nrows) of the scene are one contiguous range; the agent window is cut out of it while unpacking
    const int lo = off[scene], ns = off[scene + 1] - lo;
    std::vector<HistRow> tmp((size_t)nrows * ns);
    CHK(c, hipMemcpyAsync(tmp.data(), L.rows + scene_log_index(L.capacity, lo, ns, first_row, 0), sizeof(HistRow) * tmp.size(), hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    for (int r = 0; r < nrows; r++)
        for (int a = 0; a < agent_count; a++) {
            const HistRow &h = tmp[(size_t)r * ns + agent_begin + a];
            const size_t i = (size_t)r * agent_count + a;
            if (pos) { pos[3 * i] = h.px; pos[3 * i + 1] = h.py; pos[3 * i + 2] = h.pz; }
            if (heading) { heading[3 * i] = h.a; heading[3 * i + 1] = h.b; heading[3 * i + 2] = h.g; }
            if (vel) { vel[3 * i] = h.vx; vel[3 * i + 1] = h.vy; vel[3 * i + 2] = h.vz; }
        }
    return 0;
}

// ---- closest approach per agent (include/sca_hip.h; the rule is sca_scenes.h's, the kernel is k_scene_clearance, enqueued by
// launch_collide_finish) -----------------------------------------------------------------------------------------------------------------------
static int scene_clearance_refuse(sca_ctx *c, const char *who, ClearFault f) {
    switch (f) {
    case CLEAR_OK: return 0;
    case CLEAR_NO_SCENES: c->err = std::string(who) + ": no scenes -- sca_set_scenes first"; break;
    case CLEAR_MID_STEP: c->err = std::string(who) + ": between a policy pass and its env update"; break;
    case CLEAR_OFF: c->err = std::string(who) + ": sca_scene_clearance_enable first"; break;
    case CLEAR_BAD_SCENE: c->err = std::string(who) + ": scene must be 0 .. " + std::to_string(c->scenes.v.nscenes - 1); break;
    case CLEAR_NO_OUT: c->err = std::string(who) + ": out is NULL"; break;
    default: c->err = std::string(who) + ": struct_bytes must be sizeof(sca_scene_clearance) = " + std::to_string(sizeof(sca_scene_clearance));
    }
    return scene_clearance_error_code(f);
}
int sca_scene_clearance_enable(sca_ctx *c, int on) {
    API_ENTER(c);
    const int B = c->scenes.on ? c->scenes.v.nscenes : 0;
    if (int r = scene_clearance_refuse(c, "sca_scene_clearance_enable", scene_clearance_check(false, B, c->scenes.begun, c->scenes.clear != nullptr, 0, true, 0))) return r;
    if (!on) return scene_clearance_drop(c);
    sca_scene_clearance *rec = nullptr;
    CHK(c, hipMalloc((void **)&rec, sizeof(sca_scene_clearance) * (size_t)c->n));     // (before the old records go: a refused call changes nothing)
    const std::vector<sca_scene_clearance> empty((size_t)c->n, scene_clearance_empty());
    if (hipMemcpyAsync(rec, empty.data(), sizeof(sca_scene_clearance) * (size_t)c->n, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipFree(rec); c->err = "sca_scene_clearance_enable: the upload of the empty records failed"; return SCA_ERR_HIP; }
    if (int r = scene_clearance_drop(c)) { (void)hipFree(rec); return r; }
    c->scenes.clear = rec;
    return 0;
}
int sca_get_scene_clearance(sca_ctx *c, int scene, sca_scene_clearance *out, int32_t struct_bytes) {
    API_ENTER(c);
    const int B = c->scenes.on ? c->scenes.v.nscenes : 0;
    if (int r = scene_clearance_refuse(c, "sca_get_scene_clearance", scene_clearance_check(true, B, c->scenes.begun, c->scenes.clear != nullptr, scene, out != nullptr, struct_bytes))) return r;
    CHK(c, hipMemcpyAsync(out, c->scenes.clear + c->scenes.h_off[scene], sizeof(sca_scene_clearance) * (size_t)c->scenes.h_size[scene], hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- closest approach per agent for a whole context (include/sca_hip.h; the rule, the bound, the descent and every refusal are
// sca_clearance.h's, the kernel is k_clearance, enqueued by launch_collide_finish) --------------------------------------------------------------
static ClearanceState clearance_state(const sca_ctx *c) {
    ClearanceState s;
    s.enabled = c->clear != nullptr; s.agents = c->agents_set; s.state = c->state_set; s.mid_step = c->near_valid;
    s.scenes = c->scenes.on; s.comm = c->comm != nullptr; s.partition = c->part_on; s.n = c->n; s.shard_count = c->d.shard_count;
    return s;
}
static int clearance_refuse(sca_ctx *c, const char *who, ClearanceFault f) {
    const std::string w = std::string(who);
    switch (f) {
    case CLRF_OK: return 0;
    case CLRF_NO_AGENTS: c->err = w + ": sca_set_agents first"; break;
    case CLRF_NO_STATE: c->err = w + ": no state yet -- sca_set_state first"; break;
    case CLRF_MID_STEP: c->err = w + ": between a policy pass and its env update"; break;
    case CLRF_OFF: c->err = w + ": sca_clearance_enable first"; break;
    case CLRF_RANGE: c->err = w + ": agent_begin .. agent_begin + agent_count must lie inside 0 .. " + std::to_string(c->n); break;
    case CLRF_NO_OUT: c->err = w + ": out is NULL"; break;
    case CLRF_BAD_STRUCT: c->err = w + ": struct_bytes must be sizeof(sca_scene_clearance) = " + std::to_string(sizeof(sca_scene_clearance)); break;
    case CLRF_SCENES: c->err = w + ": the closest-approach records of a whole context and scenes (sca_set_scenes) exclude each other -- scenes have sca_scene_clearance_enable"; break;
    case CLRF_SHARD: c->err = w + ": the closest-approach records (sca_clearance_enable) need the whole swarm on this rank, not a shard with count < n (sca_set_shard)"; break;
    case CLRF_COMM: c->err = w + ": the closest-approach records (sca_clearance_enable) need the whole swarm on this rank, not a communicator (sca_comm_init)"; break;
    case CLRF_PARTITION: c->err = w + ": the closest-approach records (sca_clearance_enable) descend the agent kd-tree, which the cell-owner partition (sca_partition_init) never builds"; break;
    case CLRF_GRID_PASS: c->err = w + ": the closest-approach records are on (sca_clearance_enable) and a pass in SCA_NBR_GRID mode builds no agent tree of this step -- SCA_NBR_KDTREE, SCA_NBR_AUTO or SCA_NBR_KDTREE_HOSTBUILD"; break;
    default: c->err = w + ": the closest-approach records are on (sca_clearance_enable) and no policy pass opened this step -- there is no agent tree of this step";
    }
    return clearance_error_code(f);
}
static int clearance_drop(sca_ctx *c) {
    if (!c->clear) return 0;
    CHK(c, hipStreamSynchronize(c->stream));
    (void)hipFree(c->clear);
    c->clear = nullptr; c->clear_step = 0;
    return 0;
}
int sca_clearance_enable(sca_ctx *c, int on) {
    API_ENTER(c);
    if (int r = clearance_refuse(c, "sca_clearance_enable", clearance_check(on ? CLR_ENABLE : CLR_DISABLE, clearance_state(c), 0, 0, true, 0))) return r;
    if (!on) return clearance_drop(c);
    sca_scene_clearance *rec = nullptr;
    CHK(c, hipMalloc((void **)&rec, sizeof(sca_scene_clearance) * (size_t)c->n));     // (before the old records go: a refused call changes nothing)
    const std::vector<sca_scene_clearance> empty((size_t)c->n, scene_clearance_empty());
    if (hipMemcpyAsync(rec, empty.data(), sizeof(sca_scene_clearance) * (size_t)c->n, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) { (void)hipFree(rec); c->err = "sca_clearance_enable: the upload of the empty records failed"; return SCA_ERR_HIP; }
    if (int r = clearance_drop(c)) { (void)hipFree(rec); return r; }
    c->clear = rec; c->clear_step = 0;
    return 0;
}
int sca_get_clearance(sca_ctx *c, int agent_begin, int agent_count, sca_scene_clearance *out, int32_t struct_bytes) {
    API_ENTER(c);
    if (int r = clearance_refuse(c, "sca_get_clearance", clearance_check(CLR_GET, clearance_state(c), agent_begin, agent_count, out != nullptr, struct_bytes))) return r;
    if (agent_count > 0) CHK(c, hipMemcpyAsync(out, c->clear + agent_begin, sizeof(sca_scene_clearance) * (size_t)agent_count, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- respawning agents in place (include/sca_hip.h; the rules, the block and the scan rule are sca_respawn.h's, the kernels
// sca_respawn.hip.h's, enqueued here and nowhere else) -----------------------------------------------------------------------------------------
static RespawnCtx respawn_ctx(const sca_ctx *c) {
    RespawnCtx X;
    X.agents = c->agents_set; X.state = c->state_set; X.mid_step = c->near_valid;
    X.scenes = c->scenes.on; X.comm = c->comm != nullptr; X.partition = c->part_on; X.n = c->n; X.shard_count = c->d.shard_count;
    X.tracker_on = c->trk_on; X.paths_block = c->paths_on && c->path_W == 0; X.path_W = c->paths_on ? c->path_W : 0;
    X.policy_now = c->h_policy.data();
    return X;
}
static int respawn_refuse(sca_ctx *c, const char *who, RespawnFault f, int entry) {
    const std::string w = std::string(who), at = std::to_string(entry);
    switch (f) {
    case RSP_OK: return 0;
    case RSP_NO_AGENTS: c->err = w + ": sca_set_agents first"; break;
    case RSP_NO_STATE: c->err = w + ": no state yet -- sca_set_state first"; break;
    case RSP_MID_STEP: c->err = w + " between a policy pass and its env update: finish the step first"; break;
    case RSP_BAD_COUNT: c->err = w + ": count must be positive"; break;
    case RSP_NO_ARRAYS: c->err = w + ": ids, pos, vel, heading, radius, pref_speed, goal and max_run_dist must not be NULL"; break;
    case RSP_BAD_ID: c->err = w + ": ids[" + at + "] is not an agent of this context (0 .. " + std::to_string(c->n - 1) + ")"; break;
    case RSP_REPEATED_ID: c->err = w + ": ids[" + at + "] is named twice"; break;
    case RSP_NOT_FINITE: c->err = w + ": row " + at + " has a position that is not finite"; break;
    case RSP_NOT_POSITIVE: c->err = w + ": row " + at + " has a radius, pref_speed or max_run_dist that is not positive and finite"; break;
    case RSP_GOAL_HEADING: c->err = w + ": row " + at + " is tracked by the device tracker (sca_device_tracker_enable) and goal_heading is NULL"; break;
    case RSP_PATH_HALF: c->err = w + ": path_offsets and path_points come together or not at all"; break;
    case RSP_PATH_OFFSETS: c->err = w + ": path_offsets are negative or decrease at row " + at; break;
    case RSP_PATH_TOO_LONG: c->err = w + ": row " + at + " brings a list longer than the room per row, " + std::to_string(c->path_W) + " (sca_set_path_slots)"; break;
    case RSP_PATH_NOT_FINITE: c->err = w + ": waypoint " + at + " is not finite"; break;
    case RSP_FIN_ARGS: c->err = w + ": capacity must not be negative, count not NULL, rows not NULL with a capacity, struct_bytes sizeof(sca_finished_row) = " + std::to_string(sizeof(sca_finished_row)); break;
    case RSP_SCENES: c->err = w + " with scenes set (sca_set_scenes): a scene's agents are replaced by sca_restart_scenes"; break;
    case RSP_SHARD: c->err = w + " on a shard with count < n (sca_set_shard): the call names rows of the whole swarm on one rank"; break;
    case RSP_COMM: c->err = w + " with an active communicator: the call names rows of the whole swarm on one rank (sca_comm_destroy first)"; break;
    case RSP_PARTITION: c->err = w + " under the cell-owner partition: the rows' state does not follow the owners (sca_partition_disable first)"; break;
    case RSP_PATH_BLOCK: c->err = w + " with waypoint lists in block form (sca_set_paths): one row's list cannot be replaced there -- sca_set_path_slots"; break;
    default: c->err = w + ": path arrays, but the context's lists are not in slot form -- sca_set_path_slots first";
    }
    return respawn_error_code(f);
}
static_assert(sizeof(sca_finished_row) == FINISHED_ROW_BYTES, "sca_finished_row is 48 bytes");
// ---- spawn admission (include/sca_hip.h; the rules, the tiling and the block are sca_spawn.h's, the kernels sca_spawn.hip.h's) --------------
static int spawn_refuse(sca_ctx *c, const char *who, SpawnFault f, int entry) {
    const std::string w = std::string(who), at = std::to_string(entry);
    switch (f) {
    case SPF_OK: return 0;
    case SPF_NO_AGENTS: c->err = w + ": sca_set_agents first"; break;
    case SPF_NO_STATE: c->err = w + ": no state yet -- sca_set_state first"; break;
    case SPF_MID_STEP: c->err = w + " between a policy pass and its env update: finish the step first"; break;
    case SPF_BAD_COUNT: c->err = w + ": count must be positive"; break;
    case SPF_NO_ARRAYS: c->err = w + ": pos, radius and out must not be NULL"; break;
    case SPF_NOT_FINITE: c->err = w + ": query " + at + " has a position that is not finite"; break;
    case SPF_BAD_RADIUS: c->err = w + ": query " + at + " has a radius that is negative or not finite"; break;
    case SPF_BAD_IGNORE: c->err = w + ": ignore[" + at + "] is neither -1 nor an agent of this context (0 .. " + std::to_string(c->n - 1) + ")"; break;
    case SPF_BAD_STRUCT: c->err = w + ": struct_bytes must be sizeof(sca_scene_clearance) = " + std::to_string(sizeof(sca_scene_clearance)); break;
    case SPF_BAD_MARGIN: c->err = w + ": margin must be finite and not negative"; break;
    case SPF_NO_VERDICT: c->err = w + ": verdict must not be NULL"; break;
    case SPF_SCENES: c->err = w + " with scenes set (sca_set_scenes): probing per scene is not supported"; break;
    case SPF_SHARD: c->err = w + " on a shard with count < n (sca_set_shard): the probe reads the records of the whole swarm on one rank"; break;
    case SPF_COMM: c->err = w + " with an active communicator: the probe reads the records of the whole swarm on one rank (sca_comm_destroy first)"; break;
    default: c->err = w + " under the cell-owner partition: the rows' state does not follow the owners (sca_partition_disable first)";
    }
    return spawn_error_code(f);
}
// the block and the scratch for `count` queries against the records as they are: allocated on first use, grown like the respawn block
static int spawn_room(sca_ctx *c, int count) {
    if (count > c->spn_cap) {
        const int cap = std::max(count, std::max(1024, 2 * c->spn_cap));
        const SpawnLayout L = spawn_layout(cap);
        uint8_t *blk = nullptr, *dev = nullptr;
        CHK(c, hipHostMalloc((void **)&blk, (size_t)L.total, hipHostMallocMapped | hipHostMallocCoherent));
        if (hipMalloc((void **)&dev, (size_t)L.off[SPB_OUT] + 2 * sizeof(int32_t) * (size_t)cap) != hipSuccess) { (void)hipHostFree(blk); c->err = "spawn admission: no device memory for the queries"; return SCA_ERR_HIP; }
        if (c->spn_host) (void)hipHostFree(c->spn_host);              // (every call ends with its synchronisation: no launch still uses them)
        if (c->spn_dev) (void)hipFree(c->spn_dev);
        c->spn_host = blk; c->spn_dev = dev; c->spn_cap = cap;
    }
    const int64_t want = spawn_partials(c->n, c->d.m, spawn_batch_room(c->spn_cap), SPAWN_TILE);
    if (want > c->spn_partials_room) {
        SpawnPartial *p = nullptr;
        CHK(c, hipMalloc((void **)&p, sizeof(SpawnPartial) * (size_t)want));
        if (c->spn_partials) (void)hipFree(c->spn_partials);
        c->spn_partials = p; c->spn_partials_room = want;
    }
    return 0;
}
// the queries are in the block: their copy to the device, k_spawn_probe, k_spawn_reduce and, gated, k_spawn_gate on c->stream, no synchronisation
static int spawn_enqueue(sca_ctx *c, int count, bool gated, double margin, SpawnDev &s) {
    const SpawnLayout L = spawn_layout(c->spn_cap);
    s = SpawnDev{};
    s.rec = c->d.rec; s.obs = c->d.obs;
    s.query = (const ClearPoint *)(c->spn_dev + L.off[SPB_QUERY]); s.ignore = (const int32_t *)(c->spn_dev + L.off[SPB_IGNORE]);
    s.partials = c->spn_partials;
    s.world = (int32_t *)(c->spn_dev + L.off[SPB_OUT]); s.verdict = s.world + c->spn_cap;
    s.n = c->n; s.m = c->d.m; s.tiles = spawn_tiles(c->n, c->d.m, SPAWN_TILE);
    s.cap = spawn_batch_room(c->spn_cap);
    CHK(c, hipMemcpyAsync(c->spn_dev, c->spn_host, (size_t)L.off[SPB_IGNORE] + sizeof(int32_t) * (size_t)count, hipMemcpyHostToDevice, c->stream));
    for (int first = 0; first < count; first += SPAWN_BATCH) {        // (stream order: a batch's fold has read the partials before the next probe writes them)
        s.first = first; s.count = std::min(SPAWN_BATCH, count - first);
        hipLaunchKernelGGL(k_spawn_probe, dim3(s.tiles, spawn_chunks(s.count)), dim3(SPAWN_WAVES * 64), 0, c->stream, s);
        hipLaunchKernelGGL(k_spawn_reduce, dim3((s.count + 255) / 256), dim3(256), 0, c->stream, s, c->spn_host, L, margin, gated ? 1 : 0);
    }
    s.first = 0; s.count = count;
    if (gated) hipLaunchKernelGGL(k_spawn_gate, dim3((count + SPAWN_GATE_WAVES - 1) / SPAWN_GATE_WAVES), dim3(SPAWN_GATE_WAVES * 64), 0, c->stream, s, c->spn_host, L, margin);
    CHK(c, hipGetLastError());
    return 0;
}
int sca_probe_clearance(sca_ctx *c, int count, const double *pos, const double *radius, const int32_t *ignore, sca_scene_clearance *out, int32_t struct_bytes) {
    API_ENTER(c);
    const SpawnCheck k = spawn_check(respawn_ctx(c), count, pos, radius, ignore, out != nullptr, struct_bytes);
    if (int r = spawn_refuse(c, "sca_probe_clearance", k.fault, k.entry)) return r;
    if (int r = spawn_room(c, count)) return r;
    const SpawnLayout L = spawn_layout(c->spn_cap);
    spawn_pack(c->spn_host, L, count, pos, radius, ignore);
    SpawnDev s;
    if (int r = spawn_enqueue(c, count, false, 0.0, s)) return r;
    CHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(out, c->spn_host + L.off[SPB_OUT], sizeof(sca_scene_clearance) * (size_t)count);
    return 0;
}

// ---- vacant rows (include/sca_hip.h; the rules and the tiled edit are sca_vacancy.h's, the kernels sca_vacancy.hip.h's, enqueued here and
// nowhere else) ------------------------------------------------------------------------------------------------------------------------------
static int vacancy_call_refuse(sca_ctx *c, const char *who, VacancyFault f, int entry) {
    const std::string w = std::string(who), at = std::to_string(entry);
    switch (f) {
    case VCF_OK: return 0;
    case VCF_NO_AGENTS: c->err = w + ": sca_set_agents first"; break;
    case VCF_NO_STATE: c->err = w + ": no state yet -- sca_set_state first"; break;
    case VCF_MID_STEP: c->err = w + " between a policy pass and its env update: finish the step first"; break;
    case VCF_BAD_COUNT: c->err = w + ": count must be positive"; break;
    case VCF_NO_IDS: c->err = w + ": ids must not be NULL"; break;
    case VCF_BAD_ID: c->err = w + ": ids[" + at + "] is not an agent of this context (0 .. " + std::to_string(c->n - 1) + ")"; break;
    case VCF_REPEATED_ID: c->err = w + ": ids[" + at + "] is named twice"; break;
    case VCF_ALREADY_VACANT: c->err = w + ": ids[" + at + "] is vacant already"; break;
    case VCF_LAST_ROW: c->err = w + ": the call would leave no occupied row (a context keeps at least one)"; break;
    case VCF_LIST_ARGS: c->err = w + ": capacity must not be negative, count not NULL, ids not NULL with a capacity"; break;
    case VCF_SCENES: c->err = w + " with scenes set (sca_set_scenes): a scene's rows are vacated by sca_restart_scenes_sized"; break;
    case VCF_SHARD: c->err = w + " on a shard with count < n (sca_set_shard): the call names rows of the whole swarm on one rank"; break;
    case VCF_COMM: c->err = w + " with an active communicator: the call names rows of the whole swarm on one rank (sca_comm_destroy first)"; break;
    case VCF_PARTITION: c->err = w + " under the cell-owner partition: the rows' state does not follow the owners (sca_partition_disable first)"; break;
    default: c->err = w + " with waypoint lists in block form (sca_set_paths): one row's list cannot be emptied there -- sca_set_path_slots";
    }
    return vacancy_error_code(f);
}
// the device scratch of the permutation edit, allocated by the first retire
struct VacScratch { int32_t *ids, *tmp, *counts, *offsets, *head; };
static VacScratch vacancy_scratch(const sca_ctx *c) {
    const size_t N = (size_t)c->max_n, T = (size_t)finished_tiles(c->max_n) + 1;
    return VacScratch{c->vac.dev, c->vac.dev + N, c->vac.dev + 2 * N, c->vac.dev + 2 * N + T, c->vac.dev + 2 * N + 2 * T};
}
static int vacancy_room(sca_ctx *c) {
    if (c->vac.dev) return 0;
    const size_t N = (size_t)c->max_n, T = (size_t)finished_tiles(c->max_n) + 1;
    CHK(c, hipMalloc((void **)&c->vac.dev, sizeof(int32_t) * (2 * N + 2 * T + 16)));
    return 0;
}
// the live permutation onto the device, where it is still the host's: the edit runs there
static int vacancy_perm_to_device(sca_ctx *c) {
    if (c->perm_on_device) return 0;
    CHK(c, hipMemcpyAsync(c->d.aperm, c->h_perm.data(), sizeof(int32_t) * (size_t)c->n, hipMemcpyHostToDevice, c->stream));
    c->perm_on_device = true;
    return 0;
}
// one ordered compaction of sca_vacancy.h on c->stream, no synchronisation: the picked ids to out[base + (base_dev ? *base_dev : 0) + place]
// below `cap`, their number to head[0] (device memory, or the page-locked block)
static int vacancy_compact_enqueue(sca_ctx *c, const VacView &v, int mode, int32_t *out, int base, const int32_t *base_dev, int cap, int32_t *head) {
    const int items = vac_items(v, mode), tiles = vac_tiles(items, FIN_TILE);
    const VacScratch s = vacancy_scratch(c);
    const VacEditDev e{v, s.counts, s.offsets, out, base_dev, base, cap, mode};
    const FinishedDev f{nullptr, nullptr, nullptr, s.counts, s.offsets, items, tiles};
    if (tiles > 0) hipLaunchKernelGGL(k_vac_count, dim3(tiles), dim3(FIN_TILE), 0, c->stream, e);
    hipLaunchKernelGGL(k_finished_scan, dim3(1), dim3(FIN_TILE), 0, c->stream, f, head);      // (no tiles: the total is 0)
    if (tiles > 0) hipLaunchKernelGGL(k_vac_write, dim3(tiles), dim3(FIN_TILE), 0, c->stream, e);
    CHK(c, hipGetLastError());
    return 0;
}
static int vacancy_occupied(const sca_ctx *c) { return c->vac.on ? c->vac.m : c->n; }

// sca_respawn_agents and sca_respawn_agents_gated (gate != nullptr) behind their refusals
struct RespawnGate { double margin; int32_t *verdict; sca_scene_clearance *probe; int32_t *admitted; };
// what sca_respawn_agents_attrs / _gated_attrs bring beside the other arrays (null: the two entry points as they always were)
struct RespawnBrings {
    const uint8_t *policy = nullptr;        // [count] the call's policy bytes, null: the rows keep theirs
    bool send_solver = false;               // the rows take AgentPar records ...
    std::vector<AgentPar> par;              // ... [count], derived as sca_set_agent_params derives them
    std::vector<uint8_t> merged;            // [n] the policies behind a call that writes every named row
    bool send_planner = false;              // the rows take planner triples and class bytes ...
    std::vector<TrackTriple> trip;          // ... [count]: the call's values, sca_device_tracker_enable's where an array is NULL
    bool table_on = false;                  // the tracker's classes are recomputed (the call changes which triples the tracked rows use)
};
static int respawn_run(sca_ctx *c, const RespawnCtx &X, const RespawnArgs &A, const RespawnGate *gate, const RespawnBrings *brings = nullptr);
// the refusals the _attrs entry points add (sca_respawn_attrs.h), and what the call brings
static int respawn_brings(sca_ctx *c, const char *who, const RespawnCtx &X, const RespawnArgs &A, const uint8_t *policy, const sca_restart_attrs *attrs, RespawnBrings &B) {
    const AttrDefaults D{c->P_ctx.neighbor_dist, c->P_ctx.time_step, c->P_ctx.time_horizon, c->P_ctx.max_speed, c->P_ctx.max_heading_change, c->P_ctx.dt_nominal,
                         c->P_ctx.max_neighbors, c->trk_enable_vals[0], c->trk_enable_vals[1], c->trk_enable_vals[2]};
    RestartAttrs RA;
    const RespawnAttrCheck k = respawn_attrs_check(X, A, policy, attrs, D, B.merged, &RA);
    if (int r = respawn_refuse(c, who, k.base.fault, k.base.entry)) return r;
    const std::string w = std::string(who), at = std::to_string(k.entry);
    switch (k.fault) {
    case RSA_OK: break;
    case RSA_BAD_POLICY: c->err = w + ": row " + at + " has a policy byte above SCA_POLICY_RVO3D_DUBINS"; break;
    case RSA_STRUCT: c->err = w + ": attrs->struct_bytes = " + std::to_string(attrs->struct_bytes) + " is not a size of sca_restart_attrs (" +
                              std::to_string(RESTART_ATTR_HEAD_BYTES) + " .. " + std::to_string(sizeof(sca_restart_attrs)) + ", whole pointers)"; break;
    case RSA_RESERVED: c->err = w + ": attrs->reserved must be 0"; break;
    case RSA_NO_TRACKER: c->err = w + ": turning_radius / pitch_lo / pitch_hi without a device tracker (sca_device_tracker_enable)"; break;
    case RSA_SOLVER: c->err = w + ": row " + at + " has an attribute out of range (see sca_params)"; break;
    default: c->err = w + ": row " + at + " has a turning radius / pitch limits out of range (R > 0, pitch_lo < pitch_hi)";
    }
    if (k.fault != RSA_OK) return respawn_attrs_error_code(k.fault);
    B.policy = policy;
    // (as under sca_restart_scenes_attrs: a descriptor of NULL arrays in a context without per-agent arrays has nothing to write -- every
    // row computes from Params, which ARE the context's values)
    B.send_solver = attrs && (RA.solver() || c->d.ap);
    if (B.send_solver) {
        const SolverArrays S{RA.neighbor_dist, RA.max_neighbors, RA.time_step, RA.time_horizon, RA.max_speed, RA.max_heading_change, RA.dt_nominal};
        ThrCache thr_cache;
        B.par.resize((size_t)A.count);
        for (int r = 0; r < A.count; r++) B.par[(size_t)r] = agent_par_row(c->P_ctx, S, r, thr_cache);
    }
    // (as under sca_restart_scenes_attrs) planner attributes travel when the call names any, or when the tracker carries per-row arrays
    // already -- a NULL array then means sca_device_tracker_enable's value, which the rows must take; and the classes are dealt again
    // whenever per-row triples are in force and the call may change which of them the tracked rows use
    const bool per_row = c->trk_on && (c->trk_attr_on || c->trk_view.R_pa);
    B.send_planner = attrs && c->trk_on && (RA.planner() || per_row);
    B.table_on = B.send_planner || (per_row && policy);
    if (B.send_planner) {
        B.trip.resize((size_t)A.count);
        for (int r = 0; r < A.count; r++)
            B.trip[(size_t)r] = TrackTriple{RA.turning_radius ? RA.turning_radius[r] : D.turning_radius, RA.pitch_lo ? RA.pitch_lo[r] : D.pitch_lo,
                                            RA.pitch_hi ? RA.pitch_hi[r] : D.pitch_hi};
    }
    return 0;
}
int sca_respawn_agents_attrs(sca_ctx *c, int count, const int32_t *ids, const uint8_t *policy, const sca_restart_attrs *attrs, const double *pos, const float *vel,
                             const double *heading, const double *radius, const double *pref_speed, const double *goal, const uint8_t *zaxis,
                             const double *max_run_dist, const double *goal_heading, const int32_t *path_offsets, const double *path_points) {
    if (!policy && !attrs) return sca_respawn_agents(c, count, ids, pos, vel, heading, radius, pref_speed, goal, zaxis, max_run_dist, goal_heading, path_offsets, path_points);
    API_ENTER(c);
    const RespawnCtx X = respawn_ctx(c);
    const RespawnArgs A{count, ids, pos, vel, heading, radius, pref_speed, goal, zaxis, max_run_dist, goal_heading, path_offsets, path_points};
    RespawnBrings B;
    if (int r = respawn_brings(c, "sca_respawn_agents_attrs", X, A, policy, attrs, B)) return r;
    return respawn_run(c, X, A, nullptr, &B);
}
int sca_respawn_agents_gated_attrs(sca_ctx *c, int count, const int32_t *ids, const uint8_t *policy, const sca_restart_attrs *attrs, const double *pos,
                                   const float *vel, const double *heading, const double *radius, const double *pref_speed, const double *goal,
                                   const uint8_t *zaxis, const double *max_run_dist, const double *goal_heading, const int32_t *path_offsets,
                                   const double *path_points, double margin, int32_t *verdict, sca_scene_clearance *probe, int32_t *admitted) {
    if (!policy && !attrs)
        return sca_respawn_agents_gated(c, count, ids, pos, vel, heading, radius, pref_speed, goal, zaxis, max_run_dist, goal_heading, path_offsets, path_points, margin,
                                        verdict, probe, admitted);
    API_ENTER(c);
    const RespawnCtx X = respawn_ctx(c);
    const RespawnArgs A{count, ids, pos, vel, heading, radius, pref_speed, goal, zaxis, max_run_dist, goal_heading, path_offsets, path_points};
    RespawnBrings B;
    if (int r = respawn_brings(c, "sca_respawn_agents_gated_attrs", X, A, policy, attrs, B)) return r;
    if (int r = spawn_refuse(c, "sca_respawn_agents_gated_attrs", spawn_gate_check(margin, verdict != nullptr), -1)) return r;
    const RespawnGate gate{margin, verdict, probe, admitted};
    return respawn_run(c, X, A, &gate, &B);
}
int sca_respawn_agents(sca_ctx *c, int count, const int32_t *ids, const double *pos, const float *vel, const double *heading, const double *radius,
                       const double *pref_speed, const double *goal, const uint8_t *zaxis, const double *max_run_dist, const double *goal_heading,
                       const int32_t *path_offsets, const double *path_points) {
    API_ENTER(c);
    const RespawnCtx X = respawn_ctx(c);
    const RespawnArgs A{count, ids, pos, vel, heading, radius, pref_speed, goal, zaxis, max_run_dist, goal_heading, path_offsets, path_points};
    const RespawnCheck k = respawn_check(X, A);
    if (int r = respawn_refuse(c, "sca_respawn_agents", k.fault, k.entry)) return r;
    return respawn_run(c, X, A, nullptr);
}
int sca_respawn_agents_gated(sca_ctx *c, int count, const int32_t *ids, const double *pos, const float *vel, const double *heading, const double *radius,
                             const double *pref_speed, const double *goal, const uint8_t *zaxis, const double *max_run_dist, const double *goal_heading,
                             const int32_t *path_offsets, const double *path_points, double margin, int32_t *verdict, sca_scene_clearance *probe,
                             int32_t *admitted) {
    API_ENTER(c);
    const RespawnCtx X = respawn_ctx(c);
    const RespawnArgs A{count, ids, pos, vel, heading, radius, pref_speed, goal, zaxis, max_run_dist, goal_heading, path_offsets, path_points};
    const RespawnCheck k = respawn_check(X, A);
    if (int r = respawn_refuse(c, "sca_respawn_agents_gated", k.fault, k.entry)) return r;
    if (int r = spawn_refuse(c, "sca_respawn_agents_gated", spawn_gate_check(margin, verdict != nullptr), -1)) return r;
    const RespawnGate gate{margin, verdict, probe, admitted};
    return respawn_run(c, X, A, &gate);
}
static int respawn_run(sca_ctx *c, const RespawnCtx &X0, const RespawnArgs &A, const RespawnGate *gate, const RespawnBrings *brings) {
    // (a call that brings policies: the rows' bits -- tracked, mode reset -- and their lists' v_pref bytes follow the NEW policies)
    RespawnCtx X = X0;
    if (brings && brings->policy) X.policy_now = brings->merged.data();
    const int count = A.count;
    const int32_t *ids = A.ids, *path_offsets = A.path_offsets;
    const double *pos = A.pos, *heading = A.heading, *radius = A.radius, *pref_speed = A.pref_speed;
    const float *vel = A.vel;
    if (gate) if (int r = spawn_room(c, count)) return r;
    // the block: page-locked, mapped and coherent as the restart block is -- the kernel reads it in place.  It grows when a call names more
    // rows than any before it (at once to 1024 rows or twice the last size, at most max_agents) or a larger room per row has arrived
    if (count > c->rsp_cap || X.path_W != c->rsp_W) {
        const int cap = count > c->rsp_cap ? std::max(count, std::min(c->max_n, std::max(1024, 2 * c->rsp_cap))) : c->rsp_cap;
        uint8_t *blk = nullptr;
        CHK(c, hipHostMalloc((void **)&blk, (size_t)respawn_layout(cap, X.path_W).total, hipHostMallocMapped | hipHostMallocCoherent));
        if (c->rsp_host) (void)hipHostFree(c->rsp_host);              // (every call ends with its synchronisation: no launch still reads it)
        c->rsp_host = blk; c->rsp_cap = cap; c->rsp_W = X.path_W;
    }
    const RespawnLayout L = respawn_layout(c->rsp_cap, c->rsp_W);
    const bool slots = X.path_W > 0;
    if (int r = missions_path_mirrors(c)) return r;                    // (tables with lists: the named rows' mode bit follows the lists they hold NOW)
    uint32_t has = respawn_pack(c->rsp_host, L, X, A, slots ? c->h_path_vpref.data() : nullptr);
    // the policy bytes and the AgentPar records in a block of their own, which exists from the first call that brings any
    RespawnAttrLayout AL{};
    struct { std::vector<TrackTriple> trip, old_trip; std::vector<uint8_t> cls, old_cls, row_cls; ClassTable table, old_table; ClassUpdate cu{0, false, false}; bool first = false; } T;
    const int turn = c->rspa_turn;                                     // this call's upload sources (the ORCA3D-LP list, the class bytes)
    if (brings) c->rspa_turn ^= 1;
    if (brings) {
        if (count > c->rspa_cap) {
            const int cap = std::max(count, std::min(c->max_n, std::max(1024, 2 * c->rspa_cap)));
            uint8_t *blk = nullptr;
            CHK(c, hipHostMalloc((void **)&blk, (size_t)respawn_attrs_layout(cap).total, hipHostMallocMapped | hipHostMallocCoherent));
            if (c->rspa_host) (void)hipHostFree(c->rspa_host);        // (every call ends with its synchronisation: no launch still reads it)
            c->rspa_host = blk; c->rspa_cap = cap;
        }
        AL = respawn_attrs_layout(c->rspa_cap);
        if (brings->table_on) {
            // The tracker's classes behind a call that writes every named row (scene_class_table's rule over the plain context, every row
            // counted: a vacant row keeps its triple and its class byte, and a plain respawn that admits it later deals no classes).  The
            // named rows' bytes travel with the call; where another row's byte moved, or on first use, the whole array goes up.
            const TrackTriple def{c->trk_enable_vals[0], c->trk_enable_vals[1], c->trk_enable_vals[2]};
            T.trip = c->h_trk_trip; T.cls = c->h_trk_cls; T.table = c->trk_table;
            T.trip.resize((size_t)c->n, def); T.cls.resize((size_t)c->n, 0);
            T.first = !c->trk_attr_on;
            if (T.first) {                                             // the four per-row arrays exist from here on and are current for EVERY row
                T.table.many = true;                                   // (whatever classes an earlier call dealt, the table starts afresh)
                if (!c->trk_R_pa) { CHK(c, hipMalloc((void **)&c->trk_R_pa, sizeof(double) * (size_t)c->max_n)); CHK(c, hipMalloc((void **)&c->trk_cls, (size_t)c->max_n)); }
                if (!c->trk_plo_pa) {
                    CHK(c, hipMalloc((void **)&c->trk_plo_pa, sizeof(double) * (size_t)c->max_n));
                    CHK(c, hipMalloc((void **)&c->trk_phi_pa, sizeof(double) * (size_t)c->max_n));
                }
                for (auto &v : c->rspa_fill_trk) v.resize((size_t)c->n);
                for (size_t a = 0; a < (size_t)c->n; a++) { c->rspa_fill_trk[0][a] = T.trip[a].R; c->rspa_fill_trk[1][a] = T.trip[a].lo; c->rspa_fill_trk[2][a] = T.trip[a].hi; }
                CHK(c, hipMemcpyAsync(c->trk_R_pa, c->rspa_fill_trk[0].data(), sizeof(double) * (size_t)c->n, hipMemcpyHostToDevice, c->stream));
                CHK(c, hipMemcpyAsync(c->trk_plo_pa, c->rspa_fill_trk[1].data(), sizeof(double) * (size_t)c->n, hipMemcpyHostToDevice, c->stream));
                CHK(c, hipMemcpyAsync(c->trk_phi_pa, c->rspa_fill_trk[2].data(), sizeof(double) * (size_t)c->n, hipMemcpyHostToDevice, c->stream));
            }
            T.old_trip = T.trip; T.old_cls = T.cls; T.old_table = T.table;
            std::vector<uint8_t> travels((size_t)c->n, 0);
            if (brings->send_planner) for (int r = 0; r < count; r++) { T.trip[(size_t)ids[r]] = brings->trip[(size_t)r]; travels[(size_t)ids[r]] = 1; }
            T.cu = plain_class_table(T.table, c->n, nullptr, X.policy_now, T.trip.data(), T.cls.data(), brings->send_planner ? travels.data() : nullptr);
            if (brings->send_planner) { T.row_cls.resize((size_t)count); for (int r = 0; r < count; r++) T.row_cls[(size_t)r] = T.cls[(size_t)ids[r]]; }
        }
        has |= respawn_attrs_pack(c->rspa_host, AL, count, brings->policy, brings->send_solver ? brings->par.data() : nullptr,
                                  brings->send_planner ? brings->trip.data() : nullptr, brings->send_planner ? T.row_cls.data() : nullptr);
        if (brings->policy) respawn_attrs_bits(c->rsp_host + L.off[RSB_BITS], count, ids, c->h_policy.data(), brings->merged.data(), X.tracker_on);
        if (brings->send_solver && !c->d.ap) {
            // The first attributes in a context without per-agent arrays: from here on every agent reads d.ap[a] instead of Params, so every
            // row gets the record Params stands for -- range_sq and cos_heading_thr as sca_create derived them -- in front of the launch that
            // overwrites the named rows: the others compute the bits they computed before.  d.ap points at the array behind the synchronisation.
            ThrCache none;
            const AgentPar a0 = agent_par_row(c->P_ctx, SolverArrays{}, 0, none);
            c->rspa_fill_ap.assign((size_t)c->max_n, a0); c->rspa_fill_nd.assign((size_t)c->max_n, a0.neighbor_dist);
            if (!c->rspa_ap_new) {
                CHK(c, hipMalloc((void **)&c->rspa_ap_new, sizeof(AgentPar) * (size_t)c->max_n));
                if (hipMalloc((void **)&c->rspa_nd_new, sizeof(double) * (size_t)c->max_n) != hipSuccess) {
                    (void)hipFree(c->rspa_ap_new); c->rspa_ap_new = nullptr; c->err = "sca_respawn_agents_attrs: no device memory for the per-agent arrays"; return SCA_ERR_HIP;
                }
            }
            CHK(c, hipMemcpyAsync(c->rspa_ap_new, c->rspa_fill_ap.data(), sizeof(AgentPar) * (size_t)c->max_n, hipMemcpyHostToDevice, c->stream));
            CHK(c, hipMemcpyAsync(c->rspa_nd_new, c->rspa_fill_nd.data(), sizeof(double) * (size_t)c->max_n, hipMemcpyHostToDevice, c->stream));
        }
    }
    RespawnDev d{};
    d.rec = c->d.rec; d.heading = c->d.heading; d.goal = c->d.goal; d.pref_speed = c->d.pref_speed; d.max_run_dist = c->d.max_run_dist;
    d.total_dist = c->d.total_dist; d.vpref_ext = c->d.vpref_ext; d.step_num = c->d.step_num; d.status = c->d.status; d.nbr_n = c->d.nbr_n;
    d.near_n = c->d.near_n; d.done_count = c->d.done_count; d.zaxis = c->d.zaxis; d.vpref_mode = c->d.vpref_mode; d.nbr_valid = c->d.nbr_valid;
    if (c->trk_on) {
        static_assert(sizeof(sca_dubins::AgentTrack) % 4 == 0, "k_respawn copies the tracker record as 4-byte words");
        d.trk_nbr0 = c->trk.nbr0; d.trk_goal_heading = c->trk_goal_heading;
        d.trk_st = (restart_u32 *)c->trk.st; d.trk_init = (const restart_u32 *)c->trk_init; d.trk_words = (int)(sizeof(sca_dubins::AgentTrack) / 4);
    }
    if (slots) { d.path_pts = c->pslot_pts; d.now_goal = c->path.now_goal; d.path_len = c->pslot_len; d.path_rem = c->path.rem; d.W = c->path_W; }
    d.clear = c->clear;
    d.n = c->n;
    // vacant rows among the named ones (sca_vacancy.h): the call admits them -- their ids are appended to the permutation's occupied prefix in
    // the call's order, in front of k_respawn (which clears their vacant bit), and the vacant tail behind the prefix is written again behind it
    int vac_named = 0;
    if (c->vac.on) for (int r = 0; r < count; r++) vac_named += c->vac.h[(size_t)ids[r]];
    if (vac_named) if (int r = vacancy_perm_to_device(c)) return r;
    const VacView vv{c->d.rec, c->d.aperm, (const int32_t *)(c->rsp_host + L.off[RSB_IDS]), nullptr, c->n, vacancy_occupied(c), count};
    // on c->stream, behind every reader of the rows: a step's kernels run there or on streams the step joins back before it ends
    // the gate in front of it: the world test of every named start (the row itself ignored), the entry test among the call's rows
    SpawnDev sd{};
    SpawnLayout SL{};
    if (gate) {
        SL = spawn_layout(c->spn_cap);
        spawn_pack(c->spn_host, SL, count, pos, radius, ids);
        if (int r = spawn_enqueue(c, count, true, gate->margin, sd)) return r;
    }
    if (vac_named) {                                                   // (a gated call: the verdict decides on the device which ids are appended)
        VacView va = vv;
        va.verdict = gate ? (const int32_t *)sd.verdict : nullptr;
        if (int r = vacancy_compact_enqueue(c, va, VAC_ADMIT, c->d.aperm, vv.m, nullptr, c->n, vacancy_scratch(c).head)) return r;
    }
    if (!brings)
        hipLaunchKernelGGL(k_respawn, dim3((count + RESPAWN_WAVES - 1) / RESPAWN_WAVES), dim3(RESPAWN_WAVES * 64), 0, c->stream, d, (const uint8_t *)c->rsp_host, L, has, count,
                           (const int32_t *)(gate ? sd.verdict : nullptr));
    else
        hipLaunchKernelGGL(k_respawn_attrs, dim3((count + RESPAWN_WAVES - 1) / RESPAWN_WAVES), dim3(RESPAWN_WAVES * 64), 0, c->stream, d,
                           RespawnAttrDev{c->d.policy, c->d.ap ? c->ap_dev : c->rspa_ap_new, c->d.ap ? c->ap_nd : c->rspa_nd_new, c->trk_R_pa, c->trk_plo_pa, c->trk_phi_pa,
                                          c->trk_cls}, (const uint8_t *)c->rsp_host, L, (const uint8_t *)c->rspa_host, AL, has, count,
                           (const int32_t *)(gate ? sd.verdict : nullptr));
    CHK(c, hipGetLastError());
    // The ORCA3D-LP list (ascending ids), uploaded again only where a row entered or left that policy.  An ungated call writes every named
    // row, so the list goes up in front of the synchronisation; a gated call learns the verdicts there and enqueues it behind (below).
    bool lp_moves = false;
    if (brings && brings->policy)
        for (int r = 0; r < count && !lp_moves; r++) lp_moves = (brings->policy[r] == SCA_POLICY_ORCA3D_LP) != (c->h_policy[(size_t)ids[r]] == SCA_POLICY_ORCA3D_LP);
    std::vector<int32_t> &lp_up = c->rspa_lp[turn];
    std::vector<uint8_t> &cls_up = c->rspa_cls[turn];
    if (brings && brings->table_on && !gate && !T.cu.many && (T.cu.moved || T.first)) {       // (the per-agent form reads no class byte)
        cls_up = T.cls;
        CHK(c, hipMemcpyAsync(c->trk_cls, cls_up.data(), (size_t)c->n, hipMemcpyHostToDevice, c->stream));
    }
    if (lp_moves && !gate) {
        respawn_lp_list(brings->merged.data(), c->n, c->h_lp_list, lp_up);
        if (!lp_up.empty()) CHK(c, hipMemcpyAsync(c->lp_list, lp_up.data(), sizeof(int32_t) * lp_up.size(), hipMemcpyHostToDevice, c->stream));
    }
    if (vac_named) {                                                   // the rows that are still vacant, ascending, behind the admitted ones
        const VacScratch vs = vacancy_scratch(c);
        if (int r = vacancy_compact_enqueue(c, vv, VAC_TAIL, c->d.aperm, vv.m, vs.head, c->n, vs.head + 1)) return r;
    }
    // (mission tables: the named rows -- a gated call's admitted ones -- fly a flight that is not an entry and enter the next step running)
    if (int r = missions_host_flight(c, (const int32_t *)(c->rsp_host + L.off[RSB_IDS]), gate ? (const int32_t *)sd.verdict : nullptr, count)) return r;
    CHK(c, hipStreamSynchronize(c->stream));
    const int32_t *verdict = nullptr;
    if (gate) {
        verdict = (const int32_t *)(c->spn_host + SL.off[SPB_VERDICT]);
        int in = 0;
        for (int r = 0; r < count; r++) in += verdict[r] == SCA_SPAWN_ADMITTED;
        std::memcpy(gate->verdict, verdict, sizeof(int32_t) * (size_t)count);
        if (gate->probe) std::memcpy(gate->probe, c->spn_host + SL.off[SPB_OUT], sizeof(sca_scene_clearance) * (size_t)count);
        if (gate->admitted) *gate->admitted = in;
        if (in == 0) {                                                 // nobody admitted: nothing has changed, on the device or here
            return 0;                                                  // (first-use arrays this call made wait, unused, for the next call that brings attributes)
        }
    }
    if (brings && brings->send_solver && !c->d.ap) {                   // first use: every row holds the context's values or, named and admitted, its own
        c->ap_dev = c->rspa_ap_new; c->ap_nd = c->rspa_nd_new; c->rspa_ap_new = nullptr; c->rspa_nd_new = nullptr;
        c->d.ap = c->ap_dev;
        if (c->trk_on) c->trk_view.nd_per_agent = c->ap_nd;
    }
    // the device has the new missions: the host mirrors follow the rows that were written (a refused call has left them alone)
    const HostLayout HL = host_state_layout(c->n);
    for (int r = 0; r < count; r++) {
        if (verdict && verdict[r] != SCA_SPAWN_ADMITTED) continue;
        const int a = ids[r];
        if (brings && brings->policy) c->h_policy[(size_t)a] = brings->policy[r];
        if (brings && brings->send_solver) {
            // The context's Params are the ENVELOPE of the agents' own while per-agent attributes are in force, and like max_radius it only
            // grows under respawns.  Every kernel reads d.ap[a] for these fields; the envelope sizes the grid's cells, feeds SCA_NBR_AUTO's
            // `fits`, the collision reach and the clearance descent's bound -- conservative filters, no values.
            const AgentPar &p = brings->par[(size_t)r];
            if (p.neighbor_dist > c->P.neighbor_dist) { c->P.neighbor_dist = p.neighbor_dist; c->P.range_sq = sca_gm::g_pow2(p.neighbor_dist); c->grid.inv_cell = grid_inv_cell(p.neighbor_dist); }
            c->P.max_speed = std::max(c->P.max_speed, p.max_speed);
            c->P.dt_nominal = std::max(c->P.dt_nominal, p.dt_nominal);
        }
        if (vac_named && c->vac.h[(size_t)a]) { c->vac.h[(size_t)a] = 0; c->vac.m++; }   // admitted
        c->h_rec[a].radius = radius[r];
        c->max_radius = std::max(c->max_radius, radius[r]);           // the envelope only grows (conservative filters, as under the restarts)
        c->max_pref_speed = std::max(c->max_pref_speed, pref_speed[r]);
        if (slots) {
            const int32_t len = path_offsets ? path_offsets[r + 1] - path_offsets[r] : 0;
            c->h_path_len[a] = len;
            c->h_path_vpref[a] = len > 0 && !restart_policy_tracked(c->h_policy[a]);
        }
        if (c->hs_host) {                                              // the state block, if the caller has one: a later SCA_HOST_IN_STATE step must not bring the old row back
            uint8_t *b = c->hs_host;
            std::memcpy((double *)(b + HL.off[HS_POS]) + 3 * (size_t)a, pos + 3 * (size_t)r, sizeof(double) * 3);
            std::memcpy((float *)(b + HL.off[HS_VEL]) + 3 * (size_t)a, vel + 3 * (size_t)r, sizeof(float) * 3);
            std::memcpy((double *)(b + HL.off[HS_HEADING]) + 3 * (size_t)a, heading + 3 * (size_t)r, sizeof(double) * 3);
            (b + HL.off[HS_FLAGS])[a] = 0;
            ((double *)(b + HL.off[HS_TOTAL_DIST]))[a] = 0.0;
            ((int32_t *)(b + HL.off[HS_STEP_NUM]))[a] = 0;
        }
    }
    if (brings && brings->table_on) {
        if (gate) {
            // gated: the classes over what the ADMITTED rows brought -- dealt again from the table as it stood, the whole class array
            // enqueued behind the synchronisation on the context's stream (the kernel wrote the admitted rows' triples itself)
            T.trip = T.old_trip; T.cls = T.old_cls; T.table = T.old_table;
            if (brings->send_planner) for (int r = 0; r < count; r++) if (verdict[r] == SCA_SPAWN_ADMITTED) T.trip[(size_t)ids[r]] = brings->trip[(size_t)r];
            T.cu = plain_class_table(T.table, c->n, nullptr, c->h_policy.data(), T.trip.data(), T.cls.data(), nullptr);
            if (!T.cu.many) {
                cls_up = T.cls;
                CHK(c, hipMemcpyAsync(c->trk_cls, cls_up.data(), (size_t)c->n, hipMemcpyHostToDevice, c->stream));
            }
        }
        c->h_trk_trip.swap(T.trip); c->h_trk_cls.swap(T.cls); c->trk_table = T.table; c->trk_attr_on = true;
        std::vector<std::array<double, 3>> classes;                    // by index: one the table does not use holds NaN
        for (int q = 0; q < TRK_CLASS_CAP && !T.cu.many; q++)
            if (T.table.users[q] > 0) {
                classes.resize((size_t)q + 1, std::array<double, 3>{std::nan(""), 0.0, 0.0});
                classes[q] = {T.table.val[q].R, T.table.val[q].lo, T.table.val[q].hi};
            }
        tracker_view_apply(c, T.cu.many, classes);
    }
    if (lp_moves) {
        // gated: the list over the ADMITTED rows' new policies, enqueued behind the synchronisation on the context's stream -- the next pass
        // runs there behind it; its source is a member of the context, which no call touches before another synchronisation has passed
        if (gate && respawn_lp_list(c->h_policy.data(), c->n, c->h_lp_list, lp_up) && !lp_up.empty())
            CHK(c, hipMemcpyAsync(c->lp_list, lp_up.data(), sizeof(int32_t) * lp_up.size(), hipMemcpyHostToDevice, c->stream));
        c->h_lp_list = lp_up;
    }
    c->h_pos_valid = false; c->near_valid = false;
    if (c->vac.on && c->vac.m == c->n) c->vac.on = false;              // every row is occupied again: whatever vacancy refused works again
    positions_replaced(c);                                             // (a sizing hint, no value; not state_replaced: the form heuristics, the AUTO passes' counts among them, are left alone)
    return 0;
}
int sca_get_finished(sca_ctx *c, sca_finished_row *rows, int capacity, int *count, int32_t struct_bytes) {
    API_ENTER(c);
    if (int r = respawn_refuse(c, "sca_get_finished", finished_check(respawn_ctx(c), rows != nullptr, capacity, count != nullptr, struct_bytes), -1)) return r;
    const int n = c->n, tiles = finished_tiles(n), cap = std::min(capacity, n);
    if (!c->fin_counts) CHK(c, hipMalloc((void **)&c->fin_counts, sizeof(int32_t) * 2 * (size_t)finished_tiles(c->max_n)));
    if (!c->fin_host || cap > c->fin_cap) {
        const int want = std::min(c->max_n, std::max(cap, std::max(1024, 2 * c->fin_cap)));
        uint8_t *blk = nullptr;
        CHK(c, hipHostMalloc((void **)&blk, (size_t)FIN_HEAD_BYTES + sizeof(sca_finished_row) * (size_t)want, hipHostMallocMapped | hipHostMallocCoherent));
        if (c->fin_host) (void)hipHostFree(c->fin_host);              // (every call ends with its synchronisation: no launch still writes it)
        c->fin_host = blk; c->fin_cap = want;
    }
    const FinishedDev f{c->d.rec, c->d.total_dist, c->d.step_num, c->fin_counts, c->fin_counts + finished_tiles(c->max_n), n, tiles};
    hipLaunchKernelGGL(k_finished_count, dim3(tiles), dim3(FIN_TILE), 0, c->stream, f);
    hipLaunchKernelGGL(k_finished_scan, dim3(1), dim3(FIN_TILE), 0, c->stream, f, (int32_t *)c->fin_host);
    hipLaunchKernelGGL(k_finished_write, dim3(tiles), dim3(FIN_TILE), 0, c->stream, f, c->fin_host, cap);
    CHK(c, hipGetLastError());
    CHK(c, hipStreamSynchronize(c->stream));
    const int total = *(const int32_t *)c->fin_host;
    *count = total;
    if (std::min(total, cap) > 0) std::memcpy(rows, c->fin_host + FIN_HEAD_BYTES, sizeof(sca_finished_row) * (size_t)std::min(total, cap));
    return 0;
}

// One launch of k_vacate, the stable deletion of the named ids from the permutation's occupied prefix (into scratch, copied back), the
// ascending vacant tail behind it, one synchronisation.
int sca_retire_agents(sca_ctx *c, int count, const int32_t *ids) {
    API_ENTER(c);
    const RespawnCtx X = respawn_ctx(c);
    const int n = c->n, m = vacancy_occupied(c);
    const VacancyCheck k = vacancy_check(X, c->vac.on ? c->vac.h.data() : nullptr, m, count, ids);
    if (int r = vacancy_call_refuse(c, "sca_retire_agents", k.fault, k.entry)) return r;
    if (int r = vacancy_room(c)) return r;
    if (int r = missions_path_mirrors(c)) return r;                    // (tables with lists: the host's mirrors of the lengths follow the rows as they are NOW)
    const VacScratch s = vacancy_scratch(c);
    const int m_new = m - count;
    const bool slots = X.path_W > 0;
    CHK(c, hipMemcpyAsync(s.ids, ids, sizeof(int32_t) * (size_t)count, hipMemcpyHostToDevice, c->stream));
    if (int r = vacancy_perm_to_device(c)) return r;
    VacateDev d{};
    d.rec = c->d.rec; d.heading = c->d.heading; d.total_dist = c->d.total_dist; d.action = c->d.action; d.diag = c->d.diag;
    d.step_num = c->d.step_num; d.status = c->d.status; d.nbr_n = c->d.nbr_n; d.near_n = c->d.near_n; d.done_count = c->d.done_count;
    d.nbr_valid = c->d.nbr_valid;
    if (slots) { d.now_goal = c->path.now_goal; d.path_len = c->pslot_len; d.path_rem = c->path.rem; }
    d.clear = c->clear;
    d.n = n;
    // on c->stream, behind every reader of the rows (as k_respawn)
    hipLaunchKernelGGL(k_vacate, dim3((count + RESPAWN_WAVES - 1) / RESPAWN_WAVES), dim3(RESPAWN_WAVES * 64), 0, c->stream, d, (const int32_t *)s.ids, count);
    CHK(c, hipGetLastError());
    const VacView v{c->d.rec, c->d.aperm, nullptr, nullptr, n, m, 0};
    if (int r = vacancy_compact_enqueue(c, v, VAC_KEEP, s.tmp, 0, nullptr, n, s.head + 1)) return r;
    if (int r = vacancy_compact_enqueue(c, v, VAC_TAIL, c->d.aperm, m_new, nullptr, n, s.head + 1)) return r;
    CHK(c, hipMemcpyAsync(c->d.aperm, s.tmp, sizeof(int32_t) * (size_t)m_new, hipMemcpyDeviceToDevice, c->stream));
    if (int r = missions_retired(c, s.ids, count)) return r;           // (mission tables: a waiting word is dropped, the rows enter the next step done)
    CHK(c, hipStreamSynchronize(c->stream));
    // the host's mirrors follow
    if (c->vac.h.size() != (size_t)n) c->vac.h.assign((size_t)n, 0);
    const HostLayout HL = host_state_layout(n);
    for (int r = 0; r < count; r++) {
        const int a = ids[r];
        c->vac.h[(size_t)a] = 1;
        if (slots) { c->h_path_len[a] = 0; c->h_path_vpref[a] = 0; }
        if (c->hs_host) {                                              // the state block, if the caller has one (sca_step_host is refused while a row is vacant; the block stays true)
            uint8_t *b = c->hs_host;
            std::memset((float *)(b + HL.off[HS_VEL]) + 3 * (size_t)a, 0, sizeof(float) * 3);
            std::memset((double *)(b + HL.off[HS_HEADING]) + 3 * (size_t)a, 0, sizeof(double) * 3);
            (b + HL.off[HS_FLAGS])[a] = (uint8_t)VACANT_FLAGS;
            ((double *)(b + HL.off[HS_TOTAL_DIST]))[a] = 0.0;
            ((int32_t *)(b + HL.off[HS_STEP_NUM]))[a] = 0;
        }
    }
    c->vac.on = true; c->vac.m = m_new;
    c->h_pos_valid = false;
    positions_replaced(c);                                             // (the tree's size has changed: no sizing hint from older trees)
    return 0;
}
int sca_get_vacant(sca_ctx *c, int32_t *ids, int capacity, int *count) {
    API_ENTER(c);
    if (int r = vacancy_call_refuse(c, "sca_get_vacant", vacant_list_check(respawn_ctx(c), ids != nullptr, capacity, count != nullptr), -1)) return r;
    if (!c->vac.on) { *count = 0; return 0; }                          // (a context that never retires enqueues nothing)
    const int n = c->n, cap = std::min(capacity, n);
    if (!c->vac.host) CHK(c, hipHostMalloc((void **)&c->vac.host, (size_t)FIN_HEAD_BYTES + sizeof(int32_t) * (size_t)c->max_n, hipHostMallocMapped | hipHostMallocCoherent));
    const VacView v{c->d.rec, c->d.aperm, nullptr, nullptr, n, c->vac.m, 0};
    if (int r = vacancy_compact_enqueue(c, v, VAC_TAIL, (int32_t *)(c->vac.host + FIN_HEAD_BYTES), 0, nullptr, cap, (int32_t *)c->vac.host)) return r;
    CHK(c, hipStreamSynchronize(c->stream));
    const int total = *(const int32_t *)c->vac.host;
    *count = total;
    if (std::min(total, cap) > 0) std::memcpy(ids, c->vac.host + FIN_HEAD_BYTES, sizeof(int32_t) * (size_t)std::min(total, cap));
    return 0;
}
int sca_get_population(sca_ctx *c, int *occupied) {
    API_ENTER(c);
    ARG(c, occupied);
    if (!c->agents_set) { c->err = "sca_get_population: sca_set_agents first"; return SCA_ERR_STATE; }
    *occupied = vacancy_occupied(c);
    return 0;
}

// ---- mission tables (include/sca_hip.h; the rules are sca_missions.h's, the kernels sca_missions.hip.h's; k_mission_advance is enqueued by
// launch_collide_finish, the collect's kernels here and nowhere else) ---------------------------------------------------------------------------
static int mission_refuse(sca_ctx *c, const char *who, MissionFault f, int64_t entry) {
    const std::string w = std::string(who), at = std::to_string(entry);
    switch (f) {
    case MSF_OK: return 0;
    case MSF_NO_AGENTS: c->err = w + ": sca_set_agents first"; break;
    case MSF_MID_STEP: c->err = w + " between a policy pass and its env update: finish the step first"; break;
    case MSF_OFF: c->err = w + ": no mission tables are set -- sca_set_missions first"; break;
    case MSF_BAD_M: c->err = w + ": M must be 1 .. " + std::to_string(MISSION_MAX_M) + " (0 with entries == NULL drops the tables)"; break;
    case MSF_BAD_R: c->err = w + ": R must be 1 .. " + std::to_string(MISSION_MAX_R); break;
    case MSF_BAD_N: c->err = w + ": n is not the agent count " + std::to_string(c->n); break;
    case MSF_NO_ARRAYS: c->err = w + ": entries, first_ok and first_fail must not be NULL"; break;
    case MSF_TOO_LARGE: c->err = w + ": M x n and R x n must not exceed " + std::to_string(MISSION_MAX_SLOTS); break;
    case MSF_BAD_SUCCESSOR: c->err = w + ": a successor outside -1 .. M - 1 at " + at + " (a row of first_ok / first_fail, else the flat entry index)"; break;
    case MSF_NOT_FINITE: c->err = w + ": reachable entry " + at + " has a position, heading, goal or velocity that is not finite"; break;
    case MSF_NOT_POSITIVE: c->err = w + ": reachable entry " + at + " has a pref_speed or max_run_dist that is not positive and finite"; break;
    case MSF_BAD_ZAXIS: c->err = w + ": reachable entry " + at + " has a zaxis byte above 1 without SCA_MISSION_KEEP_ZAXIS"; break;
    case MSF_BAD_FLAGS: c->err = w + ": reachable entry " + at + " has unknown flag bits"; break;
    case MSF_GET_ARGS: c->err = w + ": a NULL output, a negative capacity, a range outside 0 .. n or struct_bytes other than the struct's size"; break;
    case MSF_SCENES: c->err = w + ": mission tables and scenes (sca_set_scenes) exclude each other: a scene's agents are replaced by sca_restart_scenes"; break;
    case MSF_SHARD: c->err = w + ": mission tables and a shard with count < n (sca_set_shard) exclude each other: the tables name rows of the whole swarm on one rank"; break;
    case MSF_COMM: c->err = w + ": mission tables and a communicator exclude each other (sca_comm_destroy first)"; break;
    case MSF_PARTITION: c->err = w + ": mission tables and the cell-owner partition exclude each other: the rows' state does not follow the owners"; break;
    case MSF_PATHS: c->err = w + ": these mission tables and waypoint lists exclude each other: tables whose entries bring their own lists come through sca_set_missions_paths, on a context whose lists are in slot form (sca_set_path_slots) before the tables arrive"; break;
    case MSF_PATH_NO_SLOTS: c->err = w + ": path_offsets, but the context's lists are not in slot form -- sca_set_path_slots first"; break;
    case MSF_PATH_START: c->err = w + ": path_offsets[0] must be 0"; break;
    case MSF_PATH_DECREASING: c->err = w + ": path_offsets decrease at the flat entry index " + at; break;
    case MSF_PATH_NO_POINTS: c->err = w + ": path_points is NULL"; break;
    case MSF_PATH_TOTAL: c->err = w + ": the lists hold more than " + std::to_string(MISSION_PATH_MAX_POINTS) + " points"; break;
    case MSF_PATH_TOO_LONG: c->err = w + ": reachable entry " + at + " brings a list longer than the room per row, " + std::to_string(c->path_W) + " (sca_set_path_slots)"; break;
    case MSF_PATH_NOT_FINITE: c->err = w + ": reachable entry " + at + " brings a waypoint that is not finite"; break;
    case MSF_PATH_CLEAR: c->err = w + ": clearing the waypoint lists while mission tables with lists stand would take the rows' rooms away under the step (drop the tables first: sca_set_missions with M = 0)"; break;
    default: c->err = w + " while mission tables are set: the host owns the state there (drop the tables: sca_set_missions with M = 0)";
    }
    return mission_error_code(f);
}
// an entry point that would bring what tables exclude, while tables stand
static int missions_standing(sca_ctx *c, const char *who, MissionFault f) { return c->ms.on ? mission_refuse(c, who, f, -1) : 0; }
static void missions_gate_free_scratch(sca_ctx::Missions::Gate &g) {
    if (g.list) (void)hipFree(g.list);
    if (g.query) (void)hipFree(g.query);
    if (g.partials) (void)hipFree(g.partials);
    g.list = nullptr; g.query = nullptr; g.partials = nullptr; g.partials_room = 0;
}
static int missions_drop(sca_ctx *c) {
    sca_ctx::Missions &m = c->ms;
    if (!m.entries && !m.host && !m.path_store) { m = sca_ctx::Missions{}; return 0; }
    (void)hipStreamSynchronize(c->stream);                             // (no launch still uses them)
    (void)missions_path_mirrors(c);                                    // (tables with lists: the rows' current lists stay, and from here on the host follows them again)
    if (m.path_store) (void)hipFree(m.path_store);
    if (m.entries) (void)hipFree(m.entries);
    if (m.words) (void)hipFree(m.words);
    if (m.results) (void)hipFree(m.results);
    if (m.totals) (void)hipFree(m.totals);
    if (m.counts) (void)hipFree(m.counts);
    if (m.host) (void)hipHostFree(m.host);
    missions_gate_free_scratch(m.gate);
    if (m.gate.words) (void)hipFree(m.gate.words);
    if (m.gate.totals) (void)hipFree(m.gate.totals);
    m = sca_ctx::Missions{};
    return 0;
}
enum MissionGateWord { MGW_WAITING = 0, MGW_VERDICT, MGW_REFUSALS, MGW_FRESH, MGW_WORDS };
constexpr int MGL_HEAD = 16;               // the gate's list: the count in its first word, the tiles' counts behind the head
enum MissionWord { MSW_FIRST_OK = 0, MSW_FIRST_FAIL, MSW_CURSOR, MSW_FLYING, MSW_ENDED, MSW_COLLECTED, MSW_LIVE, MSW_WORDS };
// flags changed between two steps (a new state, a respawn, the tables' arrival): which rows enter the next step without a done flag
static int missions_refresh_live(sca_ctx *c) {
    if (!c->ms.on || !c->state_set) return 0;
    hipLaunchKernelGGL(k_mission_live, dim3((c->n + MISSION_T - 1) / MISSION_T), dim3(MISSION_T), 0, c->stream, (const PubRec *)c->d.rec, c->ms.words + (size_t)MSW_LIVE * c->n, c->n);
    CHK(c, hipGetLastError());
    return 0;
}
// a host respawn while tables stand, behind its k_respawn on c->stream: `ids` / `verdict` as that kernel reads them (device-visible)
static int missions_host_flight(sca_ctx *c, const int32_t *ids, const int32_t *verdict, int count) {
    if (!c->ms.on) return 0;
    hipLaunchKernelGGL(k_mission_host_flight, dim3((count + MISSION_T - 1) / MISSION_T), dim3(MISSION_T), 0, c->stream, ids, verdict, count, c->n, c->ms.words + (size_t)MSW_FLYING * c->n);
    CHK(c, hipGetLastError());
    if (c->ms.gate.on) {                                                   // a gate: a named row the call wrote loses its pending mission
        hipLaunchKernelGGL(k_mission_gate_named, dim3((count + MISSION_T - 1) / MISSION_T), dim3(MISSION_T), 0, c->stream, ids, verdict, count, c->n,
                           c->ms.gate.words + (size_t)MGW_WAITING * c->n, c->ms.gate.totals);
        CHK(c, hipGetLastError());
    }
    return missions_refresh_live(c);
}
// sca_retire_agents while tables stand, behind its k_vacate on c->stream: a retired row waiting at the gate loses its pending mission
// (`dropped` + 1); a row retired in flight writes no result and moves no total -- it enters the next step done (k_mission_live), so the
// step's last kernel sees no ending -- and never ends again, so no table takes it.  ids: device memory.
static int missions_retired(sca_ctx *c, const int32_t *ids, int count) {
    if (!c->ms.on) return 0;
    if (c->ms.gate.on) {
        hipLaunchKernelGGL(k_mission_gate_named, dim3((count + MISSION_T - 1) / MISSION_T), dim3(MISSION_T), 0, c->stream, ids, (const int32_t *)nullptr, count, c->n,
                           c->ms.gate.words + (size_t)MGW_WAITING * c->n, c->ms.gate.totals);
        CHK(c, hipGetLastError());
    }
    return missions_refresh_live(c);
}
static int missions_gate_new_state(sca_ctx *c) {
    if (!c->ms.on || !c->ms.gate.on) return 0;
    hipLaunchKernelGGL(k_mission_gate_clear, dim3((c->n + MISSION_T - 1) / MISSION_T), dim3(MISSION_T), 0, c->stream, (const PubRec *)c->d.rec,
                       c->ms.gate.words + (size_t)MGW_WAITING * c->n, c->n, c->ms.gate.totals);
    CHK(c, hipGetLastError());
    return 0;
}
// The partials for m obstacles: sized by sca_set_mission_gate for the set as it stands and by sca_set_obstacles, in front of everything
// else it does, when a larger set arrives under a standing gate -- never inside a step.  A refusal changes nothing.
static int missions_gate_partials(sca_ctx *c, int m) {
    sca_ctx::Missions::Gate &g = c->ms.gate;
    const int64_t want = spawn_partials(c->n, m, g.cap, SPAWN_TILE);
    if (want <= g.partials_room) return 0;
    if (want * (int64_t)sizeof(SpawnPartial) > MISSION_GATE_MAX_SCRATCH) { c->err = "sca_set_obstacles: with this many obstacles the mission gate's scratch (partner tiles x max_per_step x 32 bytes) would exceed 1 GiB -- set the gate again with a smaller max_per_step first"; return SCA_ERR_ARG; }
    SpawnPartial *p = nullptr;
    CHK(c, hipStreamSynchronize(c->stream));                              // (no launch still uses the old ones)
    CHK(c, hipMalloc((void **)&p, sizeof(SpawnPartial) * (size_t)want));
    if (g.partials) (void)hipFree(g.partials);
    g.partials = p; g.partials_room = want;
    return 0;
}
static int missions_advance(sca_ctx *c) {
    const sca_ctx::Missions &s = c->ms;
    const int n = c->n;
    MissionDev m{};
    RespawnDev &d = m.row;
    d.rec = c->d.rec_new; d.heading = c->d.heading; d.goal = c->d.goal; d.pref_speed = c->d.pref_speed; d.max_run_dist = c->d.max_run_dist;
    d.total_dist = c->d.total_dist; d.vpref_ext = c->d.vpref_ext; d.step_num = c->d.step_num; d.status = c->d.status; d.nbr_n = c->d.nbr_n;
    d.near_n = c->d.near_n; d.done_count = c->d.done_count; d.zaxis = c->d.zaxis; d.vpref_mode = c->d.vpref_mode; d.nbr_valid = c->d.nbr_valid;
    if (c->trk_on) {
        d.trk_nbr0 = c->trk.nbr0; d.trk_goal_heading = c->trk_goal_heading;
        d.trk_st = (restart_u32 *)c->trk.st; d.trk_init = (const restart_u32 *)c->trk_init; d.trk_words = (int)(sizeof(sca_dubins::AgentTrack) / 4);
    }
    if (s.lists) {                        // tables with lists: the rows' rooms, lengths and cursors, as respawn_run hands them to k_respawn
        d.path_pts = c->pslot_pts; d.now_goal = c->path.now_goal; d.path_len = c->pslot_len; d.path_rem = c->path.rem; d.W = c->path_W;
        m.path_off = s.path_store; m.path_pts = s.path_pts;
    }
    d.clear = c->clear;
    d.n = n;
    m.live = s.words + (size_t)MSW_LIVE * n; m.policy = c->d.policy; m.entries = s.entries;
    m.first_ok = s.words + (size_t)MSW_FIRST_OK * n; m.first_fail = s.words + (size_t)MSW_FIRST_FAIL * n;
    m.cursor = s.words + (size_t)MSW_CURSOR * n; m.flying = s.words + (size_t)MSW_FLYING * n; m.ended = (uint32_t *)(s.words + (size_t)MSW_ENDED * n);
    m.results = s.results; m.totals = s.totals; m.update = ++c->ms.updates; m.M = s.M; m.R = s.R;
    if (s.gate.on) {                      // the gate: the endings, the candidates' places, their probe, the world words, the gate and the take
        const sca_ctx::Missions::Gate &q = s.gate;
        MissionGateDev g{};
        const int tiles = finished_tiles(n);
        g.m = m; g.obs = c->d.obs;
        g.waiting = q.words + (size_t)MGW_WAITING * n; g.verdict = q.words + (size_t)MGW_VERDICT * n; g.refusals = q.words + (size_t)MGW_REFUSALS * n;
        g.fresh = q.words + (size_t)MGW_FRESH * n;
        g.count = q.list; g.tile_counts = q.list + MGL_HEAD; g.ids = g.tile_counts + 2 * (size_t)tiles; g.entry = g.ids + q.cap; g.world = g.entry + q.cap;
        g.query = q.query; g.partials = q.partials; g.totals = q.totals; g.margin = q.margin;
        g.n_obs = c->d.m; g.cap = q.cap; g.tiles = tiles; g.ptiles = spawn_tiles(n, c->d.m, SPAWN_TILE);
        hipLaunchKernelGGL(k_mission_gate_end, dim3(tiles), dim3(MISSION_T), 0, c->stream, g);
        hipLaunchKernelGGL(k_mission_gate_place, dim3(tiles), dim3(MISSION_T), 0, c->stream, g);
        hipLaunchKernelGGL(k_mission_gate_probe, dim3(g.ptiles, std::min(MISSION_GATE_SLOTS, spawn_chunks(q.cap))), dim3(SPAWN_WAVES * 64), 0, c->stream, g);
        hipLaunchKernelGGL(k_mission_gate_fold, dim3((q.cap + 255) / 256), dim3(256), 0, c->stream, g);
        hipLaunchKernelGGL(k_mission_gate_take, dim3((q.cap + MISSION_GATE_WAVES - 1) / MISSION_GATE_WAVES), dim3(MISSION_GATE_WAVES * 64), 0, c->stream, g);
    } else {
        hipLaunchKernelGGL(k_mission_advance, dim3((n + MISSION_T - 1) / MISSION_T), dim3(MISSION_T), 0, c->stream, m);
    }
    CHK(c, hipGetLastError());
    positions_replaced(c);                // a taken row may stand anywhere now and the host does not learn of it: no sizing hint from older trees (no value)
    return 0;
}
// The tables' arrival, behind the check of the entry point that brings them (`who`).  lists: the context is in slot form and the call is
// sca_set_missions_paths -- path_offsets (nullable: every entry brings the empty list) / path_points are its packed CSR of `total` points.
static int missions_set(sca_ctx *c, const char *who, int M, int R, int n, const sca_mission *entries, const int32_t *first_ok, const int32_t *first_fail,
                        double max_pref_speed, bool lists, const int32_t *path_offsets, const double *path_points, int64_t total);
int sca_set_missions(sca_ctx *c, int M, int R, int n, const sca_mission *entries, const int32_t *first_ok, const int32_t *first_fail) {
    API_ENTER(c);
    if (!entries && M == 0) return missions_drop(c);
    MissionCtx X;
    X.agents = c->agents_set; X.mid_step = c->near_valid; X.scenes = c->scenes.on; X.comm = c->comm != nullptr; X.partition = c->part_on;
    X.paths = c->paths_on; X.n = c->n; X.shard_count = c->d.shard_count;
    const MissionCheck k = mission_check(X, MissionArgs{M, R, n, entries, first_ok, first_fail});
    if (int r = mission_refuse(c, "sca_set_missions", k.fault, k.entry)) return r;
    return missions_set(c, "sca_set_missions", M, R, n, entries, first_ok, first_fail, k.max_pref_speed, false, nullptr, nullptr, 0);
}
int sca_set_missions_paths(sca_ctx *c, int M, int R, int n, const sca_mission *entries, const int32_t *first_ok, const int32_t *first_fail,
                           const int32_t *path_offsets, const double *path_points) {
    API_ENTER(c);
    if (!entries && M == 0) return missions_drop(c);
    MissionCtx X;
    X.agents = c->agents_set; X.mid_step = c->near_valid; X.scenes = c->scenes.on; X.comm = c->comm != nullptr; X.partition = c->part_on;
    X.paths = c->paths_on; X.n = c->n; X.shard_count = c->d.shard_count; X.path_W = c->paths_on ? c->path_W : 0;
    const MissionPathsCheck k = mission_paths_check(X, MissionArgs{M, R, n, entries, first_ok, first_fail}, MissionPathArgs{path_offsets, path_points});
    if (int r = mission_refuse(c, "sca_set_missions_paths", k.fault, k.entry)) return r;
    return missions_set(c, "sca_set_missions_paths", M, R, n, entries, first_ok, first_fail, k.max_pref_speed, X.path_W > 0, path_offsets, path_points, k.total);
}
int sca_get_mission_paths(sca_ctx *c, int *points_per_agent, int64_t *total_points) {
    API_ENTER(c);
    if (int r = mission_refuse(c, "sca_get_mission_paths", mission_paths_get_check(c->agents_set, c->ms.on, points_per_agent && total_points), -1)) return r;
    *points_per_agent = c->ms.lists ? c->path_W : 0;
    *total_points = c->ms.lists ? c->ms.path_total : 0;
    return 0;
}
// While tables with lists stand a take moves len[a] on the device without the host knowing: the two host mirrors of the lists (h_path_len,
// sca_set_path_state's bound; h_path_vpref, "a straight-line agent with a list at the moment") are read back from the device's lengths at
// the head of every host entry point that reads them -- one copy of n words behind a synchronisation, never inside a step.
static int missions_path_mirrors(sca_ctx *c) {
    if (!c->ms.on || !c->ms.lists || !c->paths_on || c->path_W <= 0 || c->n <= 0) return 0;
    c->h_path_len.resize((size_t)c->n); c->h_path_vpref.resize((size_t)c->n);
    CHK(c, hipStreamSynchronize(c->stream));
    CHK(c, hipMemcpyAsync(c->h_path_len.data(), c->pslot_len, sizeof(int32_t) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < c->n; i++) c->h_path_vpref[i] = c->h_path_len[i] > 0 && !restart_policy_tracked(c->h_policy[i]);
    return 0;
}
static int missions_set(sca_ctx *c, const char *who, int M, int R, int n, const sca_mission *entries, const int32_t *first_ok, const int32_t *first_fail,
                        double max_pref_speed, bool lists, const int32_t *path_offsets, const double *path_points, int64_t total) {
    if (int r = missions_drop(c)) return r;
    sca_ctx::Missions &m = c->ms;
    const int tiles = finished_tiles(n);
    std::vector<int32_t> words((size_t)MSW_WORDS * n, 0);
    for (int a = 0; a < n; a++) {
        words[(size_t)MSW_FIRST_OK * n + a] = first_ok[a]; words[(size_t)MSW_FIRST_FAIL * n + a] = first_fail[a];
        words[(size_t)MSW_CURSOR * n + a] = -1; words[(size_t)MSW_FLYING * n + a] = -1;
    }
    const auto fail = [&](hipError_t e, const char *what) { c->err = std::string(who) + ": " + what + ": " + hipGetErrorString(e); (void)missions_drop(c); return SCA_ERR_HIP; };
    hipError_t e;
    if (lists && path_offsets) {          // the packed lists: the offsets, padded to 8 bytes, and the points behind them in one allocation
        const size_t off_bytes = (sizeof(int32_t) * ((size_t)M * n + 1) + 7) / 8 * 8;
        if ((e = hipMalloc((void **)&m.path_store, off_bytes + sizeof(double) * 3 * (size_t)std::max<int64_t>(total, 1))) != hipSuccess) return fail(e, "no device memory for the lists");
        m.path_pts = (double *)((uint8_t *)m.path_store + off_bytes);
        if ((e = hipMemcpyAsync(m.path_store, path_offsets, sizeof(int32_t) * ((size_t)M * n + 1), hipMemcpyHostToDevice, c->stream)) != hipSuccess) return fail(e, "the upload of the lists' offsets");
        if (total > 0 && (e = hipMemcpyAsync(m.path_pts, path_points, sizeof(double) * 3 * (size_t)total, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return fail(e, "the upload of the lists");
        m.path_total = total;
    }
    m.lists = lists;
    if ((e = hipMalloc((void **)&m.entries, sizeof(sca_mission) * (size_t)M * n)) != hipSuccess) return fail(e, "no device memory for the tables");
    if ((e = hipMalloc((void **)&m.words, sizeof(int32_t) * words.size())) != hipSuccess) return fail(e, "no device memory for the cursors");
    if ((e = hipMalloc((void **)&m.results, sizeof(sca_mission_result) * (size_t)R * n)) != hipSuccess) return fail(e, "no device memory for the results");
    if ((e = hipMalloc((void **)&m.totals, sizeof(unsigned long long) * MST_WORDS)) != hipSuccess) return fail(e, "no device memory for the totals");
    if ((e = hipMalloc((void **)&m.counts, sizeof(int32_t) * (2 * (size_t)tiles + 1))) != hipSuccess) return fail(e, "no device memory for the collect");
    if ((e = hipMemcpyAsync(m.entries, entries, sizeof(sca_mission) * (size_t)M * n, hipMemcpyHostToDevice, c->stream)) != hipSuccess) return fail(e, "the upload of the tables");
    if ((e = hipMemcpyAsync(m.words, words.data(), sizeof(int32_t) * words.size(), hipMemcpyHostToDevice, c->stream)) != hipSuccess) return fail(e, "the upload of the cursors");
    if ((e = hipMemsetAsync(m.results, 0, sizeof(sca_mission_result) * (size_t)R * n, c->stream)) != hipSuccess) return fail(e, "clearing the results");
    if ((e = hipMemsetAsync(m.totals, 0, sizeof(unsigned long long) * MST_WORDS, c->stream)) != hipSuccess) return fail(e, "clearing the totals");
    m.M = M; m.R = R; m.updates = 0; m.on = true;
    if (missions_refresh_live(c)) { (void)missions_drop(c); return SCA_ERR_HIP; }
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return fail(e, "the upload");
    c->max_pref_speed = std::max(c->max_pref_speed, max_pref_speed);     // the envelope only grows, as under respawns
    return 0;
}
int sca_get_mission_results(sca_ctx *c, sca_mission_result *out, int capacity, int *count, int32_t struct_bytes) {
    API_ENTER(c);
    if (int r = mission_refuse(c, "sca_get_mission_results", mission_results_check(c->agents_set, c->ms.on, out != nullptr, capacity, count != nullptr, struct_bytes), -1)) return r;
    sca_ctx::Missions &m = c->ms;
    const int n = c->n, tiles = finished_tiles(n);
    const int64_t cap = std::min((int64_t)capacity, (int64_t)m.R * n);
    if (!m.host || cap > m.host_cap) {
        const int64_t want = std::min((int64_t)m.R * n, std::max(cap, std::max((int64_t)1024, 2 * m.host_cap)));
        uint8_t *blk = nullptr;
        CHK(c, hipHostMalloc((void **)&blk, (size_t)MISSION_HEAD_BYTES + sizeof(sca_mission_result) * (size_t)want, hipHostMallocMapped | hipHostMallocCoherent));
        if (m.host) (void)hipHostFree(m.host);                         // (every call ends with its synchronisation: no launch still writes it)
        m.host = blk; m.host_cap = want;
    }
    const MissionCollectDev k{(const uint32_t *)(m.words + (size_t)MSW_ENDED * n), (uint32_t *)(m.words + (size_t)MSW_COLLECTED * n), m.results, m.counts, m.counts + tiles,
                              m.counts + 2 * tiles, n, tiles, m.R};
    const FinishedDev f{nullptr, nullptr, nullptr, k.counts, k.offsets, n, tiles};
    hipLaunchKernelGGL(k_mission_count, dim3(tiles), dim3(FIN_TILE), 0, c->stream, k);
    hipLaunchKernelGGL(k_finished_scan, dim3(1), dim3(FIN_TILE), 0, c->stream, f, k.total);
    hipLaunchKernelGGL(k_mission_write, dim3(tiles), dim3(FIN_TILE), 0, c->stream, k, m.host, (int)cap);
    CHK(c, hipGetLastError());
    CHK(c, hipStreamSynchronize(c->stream));
    const int total = *(const int32_t *)m.host;
    *count = total;
    if (total > 0 && total <= cap) std::memcpy(out, m.host + MISSION_HEAD_BYTES, sizeof(sca_mission_result) * (size_t)total);
    return 0;
}
int sca_get_mission_totals(sca_ctx *c, sca_mission_totals *out, int32_t struct_bytes) {
    API_ENTER(c);
    if (int r = mission_refuse(c, "sca_get_mission_totals", mission_totals_check(c->agents_set, c->ms.on, out != nullptr, struct_bytes), -1)) return r;
    static_assert(sizeof(sca_mission_totals) == sizeof(unsigned long long) * MST_WORDS, "the totals are the device's eight words");
    CHK(c, hipMemcpyAsync(out, c->ms.totals, sizeof(sca_mission_totals), hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
// ---- the admission gate in front of the take (the rules: sca_missions.h; the kernels: sca_mission_gate.hip.h) --------------------------------
static int mission_gate_refuse(sca_ctx *c, const char *who, MissionGateFault f) {
    const std::string w = std::string(who);
    switch (f) {
    case MGF_OK: return 0;
    case MGF_NO_TABLES: c->err = w + ": no mission tables are set -- sca_set_missions first"; break;
    case MGF_MID_STEP: c->err = w + " between a policy pass and its env update: finish the step first"; break;
    case MGF_NEVER_SET: c->err = w + ": no gate has been set since the tables arrived -- sca_set_mission_gate first"; break;
    case MGF_BAD_MARGIN: c->err = w + ": margin must be finite and not negative"; break;
    case MGF_BAD_CAP: c->err = w + ": max_per_step must be 0 (min(n, " + std::to_string(SPAWN_BATCH) + ")) or 1 .. " + std::to_string(c->n); break;
    case MGF_TOO_LARGE: c->err = w + ": the probe's scratch (partner tiles x max_per_step x 32 bytes) would exceed 1 GiB: a smaller max_per_step"; break;
    default: c->err = w + ": a NULL output, a range outside 0 .. n or struct_bytes other than the struct's size";
    }
    return mission_gate_error_code(f);
}
int sca_set_mission_gate(sca_ctx *c, int on, double margin, int32_t max_per_step) {
    API_ENTER(c);
    const MissionGateCheck k = mission_gate_check(c->ms.on, c->near_valid, c->n, c->d.m, on, margin, max_per_step);
    if (int r = mission_gate_refuse(c, "sca_set_mission_gate", k.fault)) return r;
    sca_ctx::Missions::Gate &g = c->ms.gate;
    const int n = c->n;
    if (!on) {
        if (!g.on) return 0;
        hipLaunchKernelGGL(k_mission_gate_clear, dim3((n + MISSION_T - 1) / MISSION_T), dim3(MISSION_T), 0, c->stream, (const PubRec *)nullptr,
                           g.words + (size_t)MGW_WAITING * n, n, g.totals);
        CHK(c, hipGetLastError());
        CHK(c, hipStreamSynchronize(c->stream));
        g.on = false;
        return 0;
    }
    // A call that fails leaves the gate as it stood -- on or off, its scratch, its cap and its margin: everything new is allocated into
    // locals and taken over at the end, so that rows waiting under a standing gate are neither stranded nor lost to `dropped`.
    CHK(c, hipStreamSynchronize(c->stream));                              // (no launch still uses the scratch of an earlier gate)
    const auto fail = [&](hipError_t e, const char *what) { c->err = std::string("sca_set_mission_gate: ") + what + ": " + hipGetErrorString(e); return SCA_ERR_HIP; };
    hipError_t e;
    int32_t *w = nullptr, *list = nullptr;
    unsigned long long *t = nullptr;
    ClearPoint *query = nullptr;
    SpawnPartial *partials = nullptr;
    const auto undo = [&](hipError_t err, const char *what) {
        if (w) (void)hipFree(w);
        if (t) (void)hipFree(t);
        if (list) (void)hipFree(list);
        if (query) (void)hipFree(query);
        if (partials) (void)hipFree(partials);
        return fail(err, what);
    };
    if (!g.words) {                                                        // the first gate behind these tables: nobody waits, nothing is counted
        std::vector<int32_t> words((size_t)MGW_WORDS * n, 0);
        std::fill(words.begin() + (size_t)MGW_WAITING * n, words.begin() + (size_t)(MGW_WAITING + 1) * n, -1);
        if ((e = hipMalloc((void **)&w, sizeof(int32_t) * words.size())) != hipSuccess) return undo(e, "no device memory for the words");
        if ((e = hipMalloc((void **)&t, sizeof(unsigned long long) * MGT_WORDS)) != hipSuccess) return undo(e, "no device memory for the totals");
        if ((e = hipMemcpyAsync(w, words.data(), sizeof(int32_t) * words.size(), hipMemcpyHostToDevice, c->stream)) == hipSuccess &&
            (e = hipMemsetAsync(t, 0, sizeof(unsigned long long) * MGT_WORDS, c->stream)) == hipSuccess)
            e = hipStreamSynchronize(c->stream);                           // (`words` is the host's: the upload has read it when this returns)
        if (e != hipSuccess) return undo(e, "the upload of the words");
    }
    const bool fresh = k.cap != g.cap || !g.list;
    const int64_t want = spawn_partials(n, c->d.m, k.cap, SPAWN_TILE);    // (mission_gate_check has held it against MISSION_GATE_MAX_SCRATCH)
    if (fresh) {                                                           // another cap: a list, queries and partials of its own
        const size_t words = (size_t)MGL_HEAD + 2 * (size_t)finished_tiles(n) + 3 * (size_t)k.cap;
        if ((e = hipMalloc((void **)&list, sizeof(int32_t) * words)) != hipSuccess) return undo(e, "no device memory for the candidates");
        if ((e = hipMemsetAsync(list, 0, sizeof(int32_t) * words, c->stream)) != hipSuccess || (e = hipStreamSynchronize(c->stream)) != hipSuccess) return undo(e, "clearing the candidates");
        if ((e = hipMalloc((void **)&query, sizeof(ClearPoint) * (size_t)k.cap)) != hipSuccess) return undo(e, "no device memory for the queries");
        if ((e = hipMalloc((void **)&partials, sizeof(SpawnPartial) * (size_t)std::max<int64_t>(want, 1))) != hipSuccess) return undo(e, "no device memory for the probe's partials");
    } else if (int r = missions_gate_partials(c, c->d.m)) {               // the same cap: the partials only grow (a failure leaves the old ones)
        (void)undo(hipSuccess, "");
        return r;
    }
    if (w) { g.words = w; g.totals = t; }                                  // nothing can fail from here on
    if (fresh) {
        missions_gate_free_scratch(g);
        g.list = list; g.query = query; g.partials = partials; g.partials_room = want; g.cap = k.cap;
    }
    g.margin = margin; g.on = true;
    return 0;
}
int sca_get_mission_gate_state(sca_ctx *c, int begin, int count, int32_t *waiting, int32_t *verdict, int32_t *refusals) {
    API_ENTER(c);
    const sca_ctx::Missions::Gate &g = c->ms.gate;
    if (int r = mission_gate_refuse(c, "sca_get_mission_gate_state", mission_gate_state_check(c->ms.on, g.words != nullptr, c->n, begin, count, waiting && verdict && refusals))) return r;
    const int n = c->n;
    if (count > 0) {
        CHK(c, hipMemcpyAsync(waiting, g.words + (size_t)MGW_WAITING * n + begin, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
        CHK(c, hipMemcpyAsync(verdict, g.words + (size_t)MGW_VERDICT * n + begin, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
        CHK(c, hipMemcpyAsync(refusals, g.words + (size_t)MGW_REFUSALS * n + begin, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
    }
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
int sca_get_mission_gate_totals(sca_ctx *c, sca_mission_gate_totals *out, int32_t struct_bytes) {
    API_ENTER(c);
    const sca_ctx::Missions::Gate &g = c->ms.gate;
    if (int r = mission_gate_refuse(c, "sca_get_mission_gate_totals", mission_gate_totals_check(c->ms.on, g.words != nullptr, out != nullptr, struct_bytes))) return r;
    CHK(c, hipMemcpyAsync(out, g.totals, sizeof(sca_mission_gate_totals), hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
int sca_get_mission_state(sca_ctx *c, int begin, int count, int32_t *cursor, int32_t *ended) {
    API_ENTER(c);
    if (int r = mission_refuse(c, "sca_get_mission_state", mission_state_check(c->agents_set, c->ms.on, c->n, begin, count, cursor != nullptr, ended != nullptr), -1)) return r;
    const int n = c->n;
    if (count > 0) {
        CHK(c, hipMemcpyAsync(cursor, c->ms.words + (size_t)MSW_CURSOR * n + begin, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
        CHK(c, hipMemcpyAsync(ended, c->ms.words + (size_t)MSW_ENDED * n + begin, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
    }
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- context checkpoints (include/sca_hip.h; the layout, the check, the calls' rules and the row move are sca_checkpoint.h's, the kernels
// sca_checkpoint.hip.h's, enqueued here and nowhere else) -----------------------------------------------------------------------------------------
static_assert(CTXCK_MS_WORDS == MSW_WORDS && CTXCK_MS_LIVE == MSW_LIVE && CTXCK_MS_FIRST_OK == MSW_FIRST_OK && CTXCK_MS_FIRST_FAIL == MSW_FIRST_FAIL &&
              CTXCK_MS_CURSOR == MSW_CURSOR && CTXCK_MS_FLYING == MSW_FLYING && CTXCK_MS_ENDED == MSW_ENDED && CTXCK_MS_COLLECTED == MSW_COLLECTED, "the blob's mission words are the device's");
static_assert(CTXCK_GATE_WORDS == MGW_WORDS && CTXCK_GATE_WAITING == MGW_WAITING && CTXCK_GATE_VERDICT == MGW_VERDICT && CTXCK_GATE_REFUSALS == MGW_REFUSALS, "the blob's gate words are the device's");
static_assert(CTXCK_TOTAL_WORDS == MST_WORDS && CTXCK_TOTAL_WORDS == MGT_WORDS && MISSION_MAX_M == 127, "the blob's totals are the device's eight words; ctx_shape_ok's bound of M");
static_assert(sizeof(sca_context_checkpoint_shape) == 4 + sizeof(CtxShape) && CX_SECTIONS == SCA_CONTEXT_CHECKPOINT_SECTIONS, "sca_context_checkpoint_shape is struct_bytes + CtxShape");
// the context as a layout sees it
static CtxShape ctx_ckpt_shape(const sca_ctx *c) {
    CtxShape S{};
    S.n = c->n; S.trk_words = c->trk_on ? (int)(sizeof(sca_dubins::AgentTrack) / 4) : 0;
    S.list_form = !c->paths_on ? CTXCK_LISTS_NONE : c->path_W > 0 ? CTXCK_LISTS_SLOTS : CTXCK_LISTS_BLOCK;
    S.W = c->paths_on ? c->path_W : 0;
    S.M = c->ms.on ? c->ms.M : 0; S.R = c->ms.on ? c->ms.R : 0;
    S.has_gate = c->ms.on && c->ms.gate.words ? 1 : 0;                    // (the words and totals outlive a gate that was switched off)
    S.has_clearance = c->clear ? 1 : 0;
    return S;
}
static CtxDev ctx_ckpt_dev(sca_ctx *c) {
    CtxDev d{};
    d.rec = c->d.rec; d.heading = c->d.heading; d.goal = c->d.goal; d.pref_speed = c->d.pref_speed; d.max_run_dist = c->d.max_run_dist; d.vpref_ext = c->d.vpref_ext;
    d.total_dist = c->d.total_dist; d.step_num = c->d.step_num; d.status = c->d.status; d.aperm = c->d.aperm; d.zaxis = c->d.zaxis; d.vpref_mode = c->d.vpref_mode;
    d.done_count = c->d.done_count;
    if (c->trk_on) { d.trk_goal_heading = c->trk_goal_heading; d.trk_nbr0 = c->trk.nbr0; d.trk_st = (ctx_u32 *)c->trk.st; }
    if (c->paths_on) { d.rem = c->path.rem; d.now_goal = c->path.now_goal; }
    if (c->paths_on && c->path_W > 0) { d.len = c->pslot_len; d.rooms = c->pslot_pts; }
    if (c->ms.on) { d.ms_words = c->ms.words; d.ms_results = c->ms.results; d.ms_totals = c->ms.totals; }
    if (c->ms.on && c->ms.gate.words) { d.gate_words = c->ms.gate.words; d.gate_totals = c->ms.gate.totals; }
    d.clear = c->clear;
    return d;
}
static int ctx_ckpt_call_refuse(sca_ctx *c, const char *who, bool buffer) {
    const CtxCallState s{c->agents_set, c->state_set, c->near_valid, c->scenes.on, c->comm != nullptr, c->part_on, c->n, c->d.shard_count};
    const CtxCallFault f = ctx_checkpoint_call_check(s, buffer);
    const std::string w(who);
    switch (f) {
    case CXC_OK: return 0;
    case CXC_NO_AGENTS: c->err = w + ": sca_set_agents first"; break;
    case CXC_NO_STATE: c->err = w + ": no state yet -- sca_set_state first"; break;
    case CXC_MID_STEP: c->err = w + " between a policy pass and its env update: finish the step first"; break;
    case CXC_SCENES: c->err = w + " with scenes set (sca_set_scenes): scenes have checkpoints of their own -- sca_save_scenes / sca_load_scenes"; break;
    case CXC_SHARD: c->err = w + " on a shard with count < n (sca_set_shard): the blob is the whole swarm's, on one rank"; break;
    case CXC_COMM: c->err = w + " with an active communicator: the blob is the whole swarm's, on one rank (sca_comm_destroy first)"; break;
    case CXC_PARTITION: c->err = w + " under the cell-owner partition: the rows' state does not follow the owners (sca_partition_disable first)"; break;
    default: c->err = w + ": the buffer is NULL";
    }
    return ctx_checkpoint_call_error_code(f);
}
static std::string ctx_ckpt_fault_text(const CtxCheck &k) {
    const std::string at = std::to_string(k.entry);
    switch (k.fault) {
    case CXF_SHORT: return "the blob is NULL or shorter than a context checkpoint's header";
    case CXF_MAGIC: return "the blob is not a context checkpoint (magic)";
    case CXF_FORMAT: return "the blob has another format version than this library writes (" + std::to_string(CTXCK_FORMAT) + ")";
    case CXF_RECORD: return "the blob's tracker record or public record size is not this library's";
    case CXF_HEADER_RANGE: return "the blob's header holds n < 1, unknown bits, or words that contradict each other (list form / W, M / R, the gate without tables, the vacancy bit / occupied)";
    case CXF_BYTES: return "the byte count is not the layout's for the blob's header (sca_context_checkpoint_layout)";
    case CXF_CHECKSUM: return "the payload's checksum is not the header's";
    case CXF_N: return "n: the blob's agent count is not the context's";
    case CXF_POLICY: return "policy: row " + at + " has another policy in the blob than in the context (or none the library knows)";
    case CXF_TRACKER: return "tracker: tracker records are present in the blob and the context has no device tracker, or absent and it has one (sca_device_tracker_enable)";
    case CXF_LISTS: return "lists: the blob's waypoint lists are absent, in block form or in slot form, and the context's are not the same (sca_set_paths / sca_set_path_slots)";
    case CXF_LIST_W: return "lists, W: the blob's room per row is not the context's (sca_set_path_slots)";
    case CXF_TABLES: return "tables: the blob's mission tables are present or absent against the context's, or have another M or R (sca_set_missions)";
    case CXF_GATE: return "gate: the mission gate's words are present in the blob and the context has never set a gate, or absent and it has (sca_set_mission_gate)";
    case CXF_CLEARANCE: return "clearance: closest-approach records are present in the blob and off in the context, or absent and on (sca_clearance_enable)";
    case CXF_PERM: return "the permutation is not one of 0 .. n - 1 (position " + at + ")";
    case CXF_FLAGS: return "row " + at + " has unknown flag bits, or a v_pref mode or z-axis word other than 0 / 1";
    case CXF_NOT_FINITE: return "row " + at + " has a position that is not finite";
    case CXF_NOT_POSITIVE: return "row " + at + " has a radius, pref_speed or max_run_dist that is not positive and finite";
    case CXF_COUNTERS: return "a step count is negative (row " + at + "; -1: the header's clear_step or updates)";
    case CXF_LEN_RANGE: return "row " + at + " has a list length outside 0 .. W";
    case CXF_REM_RANGE: return "row " + at + " has a cursor outside 0 .. the length of the row's list";
    case CXF_MISSION_RANGE: return "row " + at + " has a successor, cursor, flying or waiting word outside -1 .. M - 1";
    case CXF_COLLECTED: return "row " + at + " has more results collected than endings";
    case CXF_VERDICT: return "row " + at + " has a verdict word above SCA_SPAWN_OVER_CAP or a negative refusal count";
    case CXF_CLEAR_PARTNER: return "row " + at + " has a closest-approach partner outside its range or a negative step";
    case CXF_TRACK_RANGE: return "row " + at + " has a tracker record with a cursor, count or word outside its range";
    case CXF_VACANT_FLAGS: return "row " + at + " has the vacant bit and a flag word other than 11";
    case CXF_VACANT_COUNT: return "the rows with the vacant bit are not n - occupied of the header";
    case CXF_VACANT_PERM: return "the permutation does not hold the occupied ids in front of the vacant ids ascending (position " + at + ")";
    case CXF_VACANT_BLOCK: return "vacant rows with waypoint lists in block form, which sca_retire_agents refuses";
    case CXF_VACANT_WORDS: return "vacant row " + at + " is not as sca_retire_agents leaves a row: a velocity, heading or total_dist that is not zero, a list that is not empty or a mission waiting at the gate";
    default: return "ok";
    }
}
// the block for a blob of `bytes` and the load's stripes behind it
static int64_t ctx_ckpt_stripes_at(int64_t bytes) { return ckpt_block_round(bytes); }
static int ctx_ckpt_block(sca_ctx *c, int64_t bytes) {
    const size_t want = (size_t)(ctx_ckpt_stripes_at(bytes) + (int64_t)sizeof(int32_t) * CTXCK_STRIPES);
    if (c->cx_host && c->cx_bytes >= want) return 0;
    CHK(c, hipStreamSynchronize(c->stream));                              // (every call ends with its synchronisation: no launch still uses the block)
    uint8_t *blk = nullptr;
    CHK(c, hipHostMalloc((void **)&blk, want, hipHostMallocMapped | hipHostMallocCoherent));
    if (c->cx_host) (void)hipHostFree(c->cx_host);
    c->cx_host = blk; c->cx_bytes = want;
    return 0;
}
static CtxShape ctx_ckpt_public_shape(const sca_context_checkpoint_shape *s) {
    return CtxShape{s->n, s->trk_words, s->list_form, s->W, s->M, s->R, s->has_gate, s->has_clearance};
}
int sca_context_checkpoint_layout(const sca_context_checkpoint_shape *shape, int64_t *offsets, int64_t *total_bytes) {
    if (!shape || shape->struct_bytes != (int32_t)sizeof(sca_context_checkpoint_shape) || !offsets || !total_bytes) return SCA_ERR_ARG;
    const CtxShape S = ctx_ckpt_public_shape(shape);
    if (!ctx_shape_ok(S)) return SCA_ERR_ARG;
    const CtxLayout L = ctx_checkpoint_layout(S);
    for (int s = 0; s < CX_SECTIONS; s++) offsets[s] = L.off[s];
    *total_bytes = L.total;
    return 0;
}
int sca_context_checkpoint_info(const void *blob, int64_t bytes, struct sca_context_checkpoint_info *out, int32_t struct_bytes) {
    if (!out || struct_bytes < (int32_t)offsetof(struct sca_context_checkpoint_info, format) || struct_bytes > (int32_t)sizeof(struct sca_context_checkpoint_info)) return SCA_ERR_ARG;
    CtxHeader H;
    const CtxCheck k = ctx_checkpoint_check(blob, bytes, ckpt_track_fields(), nullptr, &H, true);
    if (k.fault != CXF_OK) return ctx_checkpoint_error_code(k.fault);
    struct sca_context_checkpoint_info I{};
    I.struct_bytes = struct_bytes; I.reserved = 0; I.format = H.format; I.lib_version = H.lib_version; I.n = H.n; I.trk_words = H.trk_words; I.record_bytes = H.rec_bytes;
    I.has_tracker = (H.present & CTXCK_HAS_TRACKER) ? 1 : 0; I.list_form = H.list_form; I.W = H.W; I.M = H.M; I.R = H.R;
    I.has_gate = (H.present & CTXCK_HAS_GATE) ? 1 : 0; I.has_clearance = (H.present & CTXCK_HAS_CLEARANCE) ? 1 : 0; I.clear_step = H.clear_step; I.state_fresh = H.state_fresh;
    I.updates = H.updates; I.total_bytes = H.total_bytes; I.checksum = H.checksum;
    I.occupied = (H.present & CTXCK_HAS_VACANCY) ? H.occupied : H.n; I.reserved1 = 0;
    std::memcpy(out, &I, (size_t)struct_bytes);
    out->struct_bytes = struct_bytes;
    return 0;
}
// The three calls behind both forms of their entry points: `options` is 0 for sca_context_checkpoint_bytes / sca_save_context /
// sca_load_context, which stay what they were -- the vacancy refusal included -- and what the caller passed for the _opt forms.
static int ctx_ckpt_options_refuse(sca_ctx *c, const char *who, uint32_t options) {
    if ((options & ~(uint32_t)SCA_CHECKPOINT_VACANCY) != 0) { c->err = std::string(who) + ": unknown option bits (SCA_CHECKPOINT_VACANCY is the only one)"; return SCA_ERR_ARG; }
    if (!(options & SCA_CHECKPOINT_VACANCY)) return vacancy_refuse(c, who);                 // (vacancy is in the blob only where the caller asks for it)
    return 0;
}
static int ctx_ckpt_bytes(sca_ctx *c, const char *who, uint32_t options, int64_t *bytes) {
    ARG(c, bytes);
    if (int r = ctx_ckpt_options_refuse(c, who, options)) return r;
    if (int r = ctx_ckpt_call_refuse(c, who, true)) return r;             // (a size only where a save is possible)
    *bytes = ctx_checkpoint_layout(ctx_ckpt_shape(c)).total;
    return 0;
}
int sca_context_checkpoint_bytes(sca_ctx *c, int64_t *bytes) {
    API_ENTER(c);
    return ctx_ckpt_bytes(c, "sca_context_checkpoint_bytes", 0, bytes);
}
int sca_context_checkpoint_bytes_opt(sca_ctx *c, uint32_t options, int64_t *bytes) {
    API_ENTER(c);
    return ctx_ckpt_bytes(c, "sca_context_checkpoint_bytes_opt", options, bytes);
}
// One launch of k_ctx_save into the page-locked block, one synchronisation, then the host completes the blob -- the policies, the
// permutation while the host still holds it, the header, the checksum -- and copies it out.
// With vacant rows (SCA_CHECKPOINT_VACANCY) the kernel and the launch are the same: a vacant row's flag word, the permutation with its
// occupied prefix and ascending vacant tail, the row's constants, tracker record, table words and cursor are sections the blob always had;
// the host adds CTXCK_HAS_VACANCY and the occupied count to the header.  With no vacant row the header, and so the blob, is the old one.
static int ctx_ckpt_save(sca_ctx *c, const char *who_, uint32_t options, void *out, int64_t out_bytes) {
    const std::string who(who_);
    if (int r = ctx_ckpt_options_refuse(c, who_, options)) return r;
    if (int r = ctx_ckpt_call_refuse(c, who_, out != nullptr)) return r;
    const CtxShape S = ctx_ckpt_shape(c);
    const CtxLayout L = ctx_checkpoint_layout(S);
    if (out_bytes < L.total) {
        c->err = who + ": the buffer holds " + std::to_string(out_bytes) + " bytes, the context needs " + std::to_string(L.total) + " (sca_context_checkpoint_bytes)";
        return SCA_ERR_ARG;
    }
    if (int r = ctx_ckpt_block(c, L.total)) return r;
    uint8_t *b = c->cx_host;
    for (int s = 0; s < CX_SECTIONS; s++) {                              // the bytes between the sections are part of the sum: at most 15 behind each,
        const int64_t end = L.off[s] + L.len[s], next = s + 1 < CX_SECTIONS ? L.off[s + 1] : L.total;   // the sections themselves are written whole
        if (next > end) std::memset(b + end, 0, (size_t)(next - end));
    }
    hipLaunchKernelGGL(k_ctx_save, dim3(ctx_checkpoint_blocks(L.total)), dim3(CTXCK_T), 0, c->stream, ctx_ckpt_dev(c), b, L, S);
    CHK(c, hipGetLastError());
    CHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(b + L.off[CX_POLICY], c->h_policy.data(), (size_t)S.n);
    if (!c->perm_on_device) std::memcpy(b + L.off[CX_PERM], c->h_perm.data(), sizeof(int32_t) * (size_t)S.n);   // the live permutation is still the host's (no device build since it was set)
    CtxHeader H{};
    H.magic = CTXCK_MAGIC; H.format = CTXCK_FORMAT; H.lib_version = sca_version(); H.n = S.n; H.trk_words = S.trk_words; H.rec_bytes = CKPT_REC_BYTES;
    H.present = ctx_shape_present(S) | (c->vac.on ? (uint32_t)CTXCK_HAS_VACANCY : 0u); H.occupied = c->vac.on ? c->vac.m : 0; H.list_form = S.list_form; H.W = S.W; H.M = S.M; H.R = S.R; H.clear_step = c->clear ? c->clear_step : 0;
    H.state_fresh = c->state_fresh ? 1 : 0; H.updates = c->ms.on ? (int64_t)c->ms.updates : 0; H.total_bytes = L.total;
    H.checksum = scene_checkpoint_sum(b + sizeof H, L.total - (int64_t)sizeof H);
    std::memcpy(b, &H, sizeof H);
    std::memcpy(out, b, (size_t)L.total);
    return 0;
}
int sca_save_context(sca_ctx *c, void *out, int64_t out_bytes) {
    API_ENTER(c);
    return ctx_ckpt_save(c, "sca_save_context", 0, out, out_bytes);
}
int sca_save_context_opt(sca_ctx *c, uint32_t options, void *out, int64_t out_bytes) {
    API_ENTER(c);
    return ctx_ckpt_save(c, "sca_save_context_opt", options, out, out_bytes);
}
// The blob is checked whole on the host (ctx_checkpoint_check) before any device work; then it goes into the page-locked block with K4's
// counters for its flags behind it, ONE launch of k_ctx_load scatters it, and the call's one synchronisation follows.  Behind it the host
// mirrors follow, as after sca_respawn_agents: the radius mirror, the envelopes (they only grow), the permutation, the lists' lengths, the
// host state block where one exists.  state_replaced's effects apply, except that state_fresh takes the blob's value.
// With SCA_CHECKPOINT_VACANCY the blob may hold vacant rows and so may the context: the load replaces vacancy wholesale.  The launch is
// then k_ctx_load_vacancy, which also leaves the vacant rows' outputs as a retire left them; the host's vacancy mirrors (which rows, how
// many are occupied) come from the checked blob, the retire's scratch is allocated in front of any device work where the blob needs it.
static int ctx_ckpt_load(sca_ctx *c, const char *who_, uint32_t options, const void *in, int64_t in_bytes) {
    const std::string who(who_);
    const bool vacancy = (options & SCA_CHECKPOINT_VACANCY) != 0;
    if (int r = ctx_ckpt_options_refuse(c, who_, options)) return r;
    if (int r = ctx_ckpt_call_refuse(c, who_, in != nullptr)) return r;
    CtxExpect X{};
    X.shape = ctx_ckpt_shape(c); X.policy = c->h_policy.data(); X.n_obs = c->d.m;
    std::vector<int32_t> block_len;
    if (X.shape.list_form == CTXCK_LISTS_BLOCK) {
        block_len.resize((size_t)c->n);
        for (int i = 0; i < c->n; i++) block_len[(size_t)i] = c->h_path_off[i + 1] - c->h_path_off[i];
        X.block_len = block_len.data();
    }
    CtxHeader H;
    const CtxCheck k = ctx_checkpoint_check(in, in_bytes, ckpt_track_fields(), &X, &H, vacancy);
    if (k.fault != CXF_OK) { c->err = who + ": " + ctx_ckpt_fault_text(k); return ctx_checkpoint_error_code(k.fault); }
    const bool brings_vacant = (H.present & CTXCK_HAS_VACANCY) != 0;
    if (brings_vacant) if (int r = vacancy_room(c)) return r;          // (as the first retire allocates it: a respawn that admits a row edits the permutation there)
    const CtxShape S = X.shape;
    const CtxLayout L = ctx_checkpoint_layout(S);
    if (int r = ctx_ckpt_block(c, L.total)) return r;
    uint8_t *b = c->cx_host;
    std::memcpy(b, in, (size_t)L.total);
    int32_t *stripes = (int32_t *)(b + ctx_ckpt_stripes_at(L.total));
    ctx_checkpoint_stripes(b, L, S.n, stripes);
    if (vacancy)
        hipLaunchKernelGGL(k_ctx_load_vacancy, dim3(ctx_checkpoint_blocks(L.total)), dim3(CTXCK_T), 0, c->stream, ctx_ckpt_dev(c),
                           CtxVacDev{c->d.action, c->d.diag, c->d.nbr_n, c->d.near_n, c->d.nbr_valid}, (const uint8_t *)b, L, S, (const int32_t *)stripes);
    else
        hipLaunchKernelGGL(k_ctx_load, dim3(ctx_checkpoint_blocks(L.total)), dim3(CTXCK_T), 0, c->stream, ctx_ckpt_dev(c), (const uint8_t *)b, L, S, (const int32_t *)stripes);
    CHK(c, hipGetLastError());
    CHK(c, hipStreamSynchronize(c->stream));
    const int n = S.n;
    std::memcpy(c->h_perm.data(), b + L.off[CX_PERM], sizeof(int32_t) * (size_t)n);
    c->perm_on_device = false;                                          // (as behind sca_set_kd_perm: the next build takes the host's)
    const double *ps = (const double *)(b + L.off[CX_PREF_SPEED]);
    const int32_t *len = S.list_form == CTXCK_LISTS_SLOTS ? (const int32_t *)(b + L.off[CX_LEN]) : nullptr;
    if (len) { c->h_path_len.resize((size_t)n); c->h_path_vpref.resize((size_t)n); }
    const HostLayout HL = host_state_layout(n);
    if (vacancy) {                                                      // vacancy is replaced wholesale (sca_set_agents' words where the blob brings none)
        c->vac.on = brings_vacant; c->vac.m = brings_vacant ? H.occupied : 0;
        if (brings_vacant) c->vac.h.assign((size_t)n, 0); else c->vac.h.clear();
    }
    for (int a = 0; a < n; a++) {
        PubRec r;
        std::memcpy(&r, b + L.off[CX_REC] + (size_t)CKPT_REC_BYTES * a, sizeof r);
        if (brings_vacant) c->vac.h[(size_t)a] = vacant_flag(r.flags) ? 1 : 0;
        c->h_rec[a].radius = r.radius;
        c->max_radius = std::max(c->max_radius, r.radius);             // the envelopes only grow (conservative filters, as under respawns)
        c->max_pref_speed = std::max(c->max_pref_speed, ps[a]);
        if (len) { c->h_path_len[a] = len[a]; c->h_path_vpref[a] = len[a] > 0 && !restart_policy_tracked(c->h_policy[a]); }
        if (c->hs_host) {                                              // the state block, if the caller has one: a later SCA_HOST_IN_STATE step must not bring the old rows back
            uint8_t *h = c->hs_host;
            const double pos[3] = {r.px, r.py, r.pz};
            const float vel[3] = {r.vx, r.vy, r.vz};
            std::memcpy((double *)(h + HL.off[HS_POS]) + 3 * (size_t)a, pos, sizeof pos);
            std::memcpy((float *)(h + HL.off[HS_VEL]) + 3 * (size_t)a, vel, sizeof vel);
            std::memcpy((double *)(h + HL.off[HS_HEADING]) + 3 * (size_t)a, b + L.off[CX_HEADING] + 24 * (size_t)a, 24);
            (h + HL.off[HS_FLAGS])[a] = (uint8_t)r.flags;
            std::memcpy((double *)(h + HL.off[HS_TOTAL_DIST]) + a, b + L.off[CX_TOTAL_DIST] + 8 * (size_t)a, 8);
            std::memcpy((int32_t *)(h + HL.off[HS_STEP_NUM]) + a, b + L.off[CX_STEP_NUM] + 4 * (size_t)a, 4);
        }
    }
    if (c->clear) c->clear_step = H.clear_step;
    if (c->ms.on) c->ms.updates = (long long)H.updates;
    c->h_pos_valid = false;
    state_replaced(c);
    c->state_fresh = H.state_fresh != 0;
    return 0;
}
int sca_load_context(sca_ctx *c, const void *in, int64_t in_bytes) {
    API_ENTER(c);
    return ctx_ckpt_load(c, "sca_load_context", 0, in, in_bytes);
}
int sca_load_context_opt(sca_ctx *c, uint32_t options, const void *in, int64_t in_bytes) {
    API_ENTER(c);
    return ctx_ckpt_load(c, "sca_load_context_opt", options, in, in_bytes);
}

// ---- finished scenes hand over their result with the step (include/sca_hip.h; the rules and the layout are sca_scenes.h's, the kernel is
// k_scene_harvest, enqueued by launch_collide_finish) ------------------------------------------------------------------------------------------
static int scene_harvest_refuse(sca_ctx *c, const char *who, HarvestFault f) {
    switch (f) {
    case HARVEST_OK: return 0;
    case HARVEST_NO_SCENES: c->err = std::string(who) + ": no scenes -- sca_set_scenes first"; break;
    case HARVEST_MID_STEP: c->err = std::string(who) + " between a policy pass and its env update: finish the step first"; break;
    case HARVEST_OFF: c->err = std::string(who) + ": sca_scene_harvest_enable first"; break;
    case HARVEST_NO_OUT: c->err = std::string(who) + ": an output pointer is NULL"; break;
    default: c->err = std::string(who) + ": struct_bytes must be sizeof(sca_scene_harvest) as the caller compiled it (" +
                      std::to_string(offsetof(sca_scene_harvest, counters)) + " .. " + std::to_string(sizeof(sca_scene_harvest)) + ")";
    }
    return scene_harvest_error_code(f);
}
int sca_scene_harvest_layout(int nscenes, int n, int64_t *offsets, int64_t *total_bytes) {
    if (nscenes <= 0 || n < nscenes || !offsets || !total_bytes) return SCA_ERR_ARG;
    const HarvestLayout L = scene_harvest_layout(nscenes, n);
    for (int s = 0; s < HV_SECTIONS; s++) offsets[s] = L.off[s];
    *total_bytes = L.total;
    return 0;
}
int sca_scene_harvest_enable(sca_ctx *c, int on) {
    API_ENTER(c);
    const int B = c->scenes.on ? c->scenes.v.nscenes : 0;
    if (int r = scene_harvest_refuse(c, "sca_scene_harvest_enable", scene_harvest_check(HARVEST_ENABLE, B, c->scenes.begun, c->scenes.hv_host != nullptr, true, 0))) return r;
    if (!on) return scene_harvest_drop(c);
    const HarvestLayout L = scene_harvest_layout(B, c->n);
    uint8_t *blk = nullptr;                                               // (before the old block goes: a call that fails here changes nothing)
    CHK(c, hipHostMalloc((void **)&blk, (size_t)L.total, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(blk, 0, (size_t)L.total);
    if (c->state_set) {                                                   // the counters as the scenes stand: what a step's k_scene_harvest writes from then on
        std::vector<int32_t> live((size_t)B), steps((size_t)B);
        if (int r = sca_get_scene_state(c, live.data(), steps.data())) { (void)hipHostFree(blk); return r; }
        int32_t *cnt = (int32_t *)(blk + L.off[HV_COUNTERS]);
        for (int s = 0; s < B; s++) { cnt[2 * s] = live[s]; cnt[2 * s + 1] = steps[s]; }
    }
    if (int r = scene_harvest_drop(c)) { (void)hipHostFree(blk); return r; }
    c->scenes.hv_host = blk; c->scenes.hv_layout = L; c->scenes.hv_batch_step = 0;
    return 0;
}
int sca_scene_harvest_get(sca_ctx *c, sca_scene_harvest *out, int32_t struct_bytes) {
    API_ENTER(c);
    const int B = c->scenes.on ? c->scenes.v.nscenes : 0;
    if (int r = scene_harvest_refuse(c, "sca_scene_harvest_get", scene_harvest_check(HARVEST_GET, B, c->scenes.begun, c->scenes.hv_host != nullptr, out != nullptr, struct_bytes))) return r;
    const HarvestLayout &L = c->scenes.hv_layout;
    uint8_t *b = c->scenes.hv_host;
    sca_scene_harvest h;
    std::memset(&h, 0, sizeof h);
    h.struct_bytes = struct_bytes; h.nscenes = B; h.n = c->n;
    h.counters = (int32_t *)(b + L.off[HV_COUNTERS]); h.summary = (sca_scene_summary *)(b + L.off[HV_SUMMARY]);
    h.pos = (double *)(b + L.off[HV_POS]); h.vel = (float *)(b + L.off[HV_VEL]); h.heading = (double *)(b + L.off[HV_HEADING]);
    h.flags = b + L.off[HV_FLAGS]; h.total_dist = (double *)(b + L.off[HV_TOTAL_DIST]); h.step_num = (int32_t *)(b + L.off[HV_STEP_NUM]);
    size_t fit = offsetof(sca_scene_harvest, counters);                  // only the members that fit entirely into the caller's struct
    while (fit + sizeof(void *) <= (size_t)struct_bytes) fit += sizeof(void *);
    std::memcpy(out, &h, fit);
    return 0;
}
int sca_scene_harvest_collect(sca_ctx *c, int32_t *scene_ids, int32_t *count) {
    API_ENTER(c);
    const int B = c->scenes.on ? c->scenes.v.nscenes : 0;
    if (int r = scene_harvest_refuse(c, "sca_scene_harvest_collect", scene_harvest_check(HARVEST_COLLECT, B, c->scenes.begun, c->scenes.hv_host != nullptr, scene_ids && count, 0))) return r;
    CHK(c, hipStreamSynchronize(c->stream));                              // (nothing to wait for directly behind sca_env_step)
    sca_scene_summary *sum = (sca_scene_summary *)(c->scenes.hv_host + c->scenes.hv_layout.off[HV_SUMMARY]);
    *count = scene_harvest_order(B, sum, scene_ids);
    scene_harvest_clear_fresh(c, *count, scene_ids);
    return 0;
}

int sca_get_actions(sca_ctx *c, float *action) {
    API_ENTER(c);
    ARG(c, action);
    std::vector<float> tmp((size_t)c->n * 8);
    CHK(c, hipMemcpyAsync(tmp.data(), c->d.action, sizeof(float) * 8 * c->n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < c->n; i++) std::memcpy(action + 7 * (size_t)i, tmp.data() + 8 * (size_t)i, 7 * sizeof(float));
    return 0;
}

int sca_get_neighbors(sca_ctx *c, int32_t *nbr_n, int32_t *nbr_id, uint8_t *nbr_kind, double *nbr_dsq, uint8_t *nbr_valid) {
    API_ENTER(c);
    const int n = c->n;
    std::vector<int32_t> ids((size_t)n * K_MAX);
    CHK(c, hipMemcpyAsync(ids.data(), c->d.nbr_id, sizeof(int32_t) * K_MAX * n, hipMemcpyDeviceToHost, c->stream));
    if (nbr_n) CHK(c, hipMemcpyAsync(nbr_n, c->d.nbr_n, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    if (nbr_dsq) CHK(c, hipMemcpyAsync(nbr_dsq, c->d.nbr_dsq, sizeof(double) * K_MAX * n, hipMemcpyDeviceToHost, c->stream));
    if (nbr_valid) CHK(c, hipMemcpyAsync(nbr_valid, c->d.nbr_valid, n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < ids.size(); i++) {
        const int32_t v = ids[i];
        const bool ob = v >= 0 && (v & NBR_OBSTACLE_BIT);
        if (nbr_id) nbr_id[i] = v < 0 ? -1 : (v & ~NBR_OBSTACLE_BIT);
        if (nbr_kind) nbr_kind[i] = ob ? 1 : 0;
    }
    return 0;
}

int sca_get_nbr0(sca_ctx *c, double *dsq0) {
    API_ENTER(c);
    ARG(c, dsq0 && c->agents_set);
    double *tmp = c->kd.kx;      // build scratch, free between passes
    hipLaunchKernelGGL(k_nbr0, dim3((c->n + 255) / 256), dim3(256), 0, c->stream, c->d, tmp);
    CHK(c, hipMemcpyAsync(dsq0, tmp, sizeof(double) * c->n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int sca_get_diag(sca_ctx *c, int32_t *diag, int32_t *status, double *vpref_used) {
    API_ENTER(c);
    const int n = c->n;
    std::vector<int32_t> tmp((size_t)n * 8);
    CHK(c, hipMemcpyAsync(tmp.data(), c->d.diag, sizeof(int32_t) * 8 * n, hipMemcpyDeviceToHost, c->stream));
    if (status) CHK(c, hipMemcpyAsync(status, c->d.status, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    if (vpref_used) CHK(c, hipMemcpyAsync(vpref_used, c->d.vpref_used, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, c->stream));
    CHK(c, hipStreamSynchronize(c->stream));
    if (diag) for (int i = 0; i < n; i++) std::memcpy(diag + 5 * (size_t)i, tmp.data() + 8 * (size_t)i, 5 * sizeof(int32_t));
    return 0;
}

int sca_set_shard(sca_ctx *c, int begin, int count) {
    API_ENTER(c);
    ARG(c, begin >= 0 && count >= 0 && begin + count <= c->n);
    // with a communicator the shard IS rank * n / nranks: the in-place ncclAllGather of sca_run_steps relies on it
    if (c->part_on) { c->err = "sca_set_shard with the cell-owner partition active (sca_partition_disable first)"; return SCA_ERR_STATE; }
    if (c->comm) { c->err = "sca_set_shard with an active communicator (the shard follows from rank / nranks; sca_comm_destroy first)"; return SCA_ERR_STATE; }
    if (c->scenes.on && (begin != 0 || count != c->n)) { c->err = "sca_set_shard with scenes set (sca_set_scenes): scenes are stepped by one rank, whole"; return SCA_ERR_UNSUPPORTED; }
    if (count < c->n) if (int r = vacancy_refuse(c, "sca_set_shard with count < n")) return r;
    if (int r = clearance_refuse(c, "sca_set_shard", clearance_check(CLR_SET_SHARD, clearance_state(c), count, 0, true, 0))) return r;
    if (count < c->n) if (int r = missions_standing(c, "sca_set_shard", MSF_SHARD)) return r;
    c->d.shard_begin = begin; c->d.shard_count = count;
    c->au.forget();                                                       // another shard: the AUTO passes' counts described the old one
    return 0;
}
int sca_public_records(sca_ctx *c, int which, void **device_ptr, int64_t *bytes_per_agent) {
    API_ENTER(c);
    if (device_ptr) *device_ptr = which ? (void *)c->d.rec_new : (void *)c->d.rec;
    if (bytes_per_agent) *bytes_per_agent = (int64_t)sizeof(PubRec);
    return 0;
}
int sca_bind_public_records(sca_ctx *c, void *current, void *moved, int64_t bytes_each) {
    API_ENTER(c);
    ARG(c, (current == nullptr) == (moved == nullptr));
    if (!c->agents_set) { c->err = "sca_set_agents first"; return SCA_ERR_STATE; }
    const size_t live = sizeof(PubRec) * (size_t)c->n;                    // only the n live records move, never max_agents
    if (current) {
        ARG(c, bytes_each >= (int64_t)live);
        // carry the live records over into the caller's buffer
        CHK(c, hipMemcpyAsync(current, c->d.rec, live, hipMemcpyDeviceToDevice, c->stream));
        CHK(c, hipStreamSynchronize(c->stream));
        c->d.rec = (PubRec *)current; c->d.rec_new = (PubRec *)moved;
    } else {
        CHK(c, hipMemcpyAsync(c->rec_own, c->d.rec, live, hipMemcpyDeviceToDevice, c->stream));
        CHK(c, hipStreamSynchronize(c->stream));
        c->d.rec = c->rec_own; c->d.rec_new = c->rec_new_own;
    }
    return 0;
}
int sca_set_stream(sca_ctx *c, void *hip_stream) {
    API_ENTER(c);
    CHK(c, hipStreamSynchronize(c->stream));                             // work already enqueued finishes where it was
    c->stream = (hipStream_t)hip_stream;                                 // NULL is HIP's null stream (torch's default stream), taken literally
    return 0;
}
int sca_use_own_stream(sca_ctx *c) {
    API_ENTER(c);
    CHK(c, hipStreamSynchronize(c->stream));
    c->stream = c->stream_own;
    return 0;
}
int sca_last_kernel_ms(sca_ctx *c, float *neighbors_ms, float *solve_ms, float *update_ms) {
    API_ENTER(c);
    if (neighbors_ms) *neighbors_ms = c->ms_nbr;
    if (solve_ms) *solve_ms = c->ms_solve;
    if (update_ms) *update_ms = c->ms_update;
    return 0;
}

}  // extern "C"
