/*
 * sca_hip.h -- C-ABI of libsca_hip.so: the MI355X-native batched velocity solver that replaces the
 * per-agent hot path of wuuya1/SCA (mamp/policies + neighbour search + the per-step loop in mamp/envs).
 *
 * Plain pointers and sizes only; caller-owned host buffers unless a function says "device".
 * Every function returns 0 on success or a negative sca_error; sca_last_error() gives the text.
 * One context per device; calls on one context are not thread-safe.
 *
 * What each entry point replaces in the reference (paths relative to wuuya1/SCA):
 *   sca_create / sca_set_agents   Agent.__init__ solver attributes            mamp/agents/agent.py:9-77
 *   sca_set_obstacles             Obstacle list + KDTree.buildObstacleTree    mamp/agents/obstacle.py:5-28, mamp/policies/kdTree.py:158-227
 *   sca_set_state / sca_get_state agent.pos/vel/heading/flags attribute reads  mamp/envs/mampenv.py:34-46
 *   sca_set_vpref                 SCA's Dubins-tracker output fed to intersect mamp/policies/sca/scaPolicy.py:32,264-338
 *   sca_set_paths                 Agent.path + policy.get_trajectory/now_goal  mamp/agents/agent.py:44, rvo3dPolicy.py:71-85, orca3dPolicy.py:298-312
 *   sca_set_path_slots            the same lists, a room per agent row         mamp/agents/agent.py:44
 *   sca_restart_scenes_paths      a new episode's Agent.path lists             mamp/agents/agent.py:44, run_example/run_sca.py:174-178
 *   sca_policy_pass               first loop of MACAEnv._take_action:          mamp/envs/mampenv.py:28-40
 *                                 KDTree.buildAgentTree                        mamp/policies/kdTree.py:56-122
 *                                 computeNeighbors / insert*Neighbor           mamp/policies/sca/scaPolicy.py:107-116, mamp/agents/agent.py:79-124
 *                                 <Policy>.find_next_action + intersect        scaPolicy.py:26-240, rvo3dPolicy.py:23-179, srvo3dPolicy.py:23-231,
 *                                                                              orca3dPolicy.py:38-120,400-439, orca3dPolicyOfficial.py:37-300
 *   sca_env_update                second loop of _take_action + is_done        mamp/envs/mampenv.py:42-59,61-105
 *   sca_run_steps                 `while ...: env.step(actions)`               run_example/run_sca.py:174-178
 *   sca_step_host                 _take_action whole, the env owning the state mamp/envs/mampenv.py:27-59
 */
#ifndef SCA_HIP_H
#define SCA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCA_MAX_NEIGHBORS 16          /* agent.py:32 */
#define SCA_ACTION_DIM 7              /* mampenv.py:30: vx, vy, vz, speed, d_yaw, d_pitch, d_roll */
#define SCA_DIAG_DIM 5                /* n_suitable, fallback, chosen candidate, planeFail, lp4_ran (-1 = n/a) */

typedef struct sca_ctx sca_ctx;

/* agent.py:27-41 + config.py; sca_default_params() fills the reference's values.  The reference keeps these per Agent object; a context holds
 * ONE value of each as the default for all its agents; sca_set_agent_params hands over the agents' own where they differ
 * (sca_amd.env.MACAEnv reads them off the agents and does both).
 * sca_create refuses values the kernels were not built for: non-finite or non-positive distances / steps / speeds, max_neighbors outside
 * 1 .. 16, max_heading_change outside [0, pi].  Parity at non-default values: tests/golden/F16_params_*. */
typedef struct sca_params {
    double neighbor_dist;        /* agent.py:33  10.0 */
    double time_step;            /* agent.py:34  DT = 0.1 */
    double time_horizon;         /* agent.py:35  10.0 */
    double max_speed;            /* agent.py:36  1.0 */
    double max_heading_change;   /* agent.py:29  pi/4 */
    double near_goal_threshold;  /* config.py:3  0.5 */
    int32_t max_neighbors;       /* agent.py:32  16 (1 .. SCA_MAX_NEIGHBORS) */
    int32_t struct_bytes;        /* sizeof(sca_params) as the CALLER compiled it (sca_default_params_v2 / SCA_DEFAULT_PARAMS store it).
                                    0 = a version-100 caller: its struct ends here (56 bytes, this field was `reserved`, always 0), nothing
                                    beyond is read and dt_nominal = time_step, which is what version 100 integrated with */
    double dt_nominal;           /* agent.py:41  DT = 0.1: the integrator's step (mampenv.py:90-92); time_step is the one the constraints
                                    read (util.py:8, orca3dPolicyOfficial.py:98).  Version 101 on; read only when struct_bytes >= 64. */
} sca_params;

enum sca_policy {                 /* which find_next_action the agent runs */
    SCA_POLICY_SCA = 0,           /* mamp/policies/sca/scaPolicy.py        (v_pref supplied: sca_set_vpref) */
    SCA_POLICY_RVO3D = 1,         /* mamp/policies/rvo3dPolicy.py */
    SCA_POLICY_SRVO3D = 2,        /* mamp/policies/srvo3dPolicy.py */
    SCA_POLICY_ORCA3D = 3,        /* mamp/policies/orca3dPolicy.py         (sampled, as run_orca.py runs it) */
    SCA_POLICY_ORCA3D_LP = 4,     /* mamp/policies/orca3dPolicyOfficial.py (linearProgram1-4) */
    SCA_POLICY_RVO3D_DUBINS = 5   /* mamp/policies/sca/rvo3dDubinsPolicy.py (RVO3D selection, v_pref supplied) */
};

enum sca_flag { SCA_FLAG_AT_GOAL = 1, SCA_FLAG_COLLISION = 2, SCA_FLAG_TIMEOUT = 4,     /* agent.py:70-72 */
                SCA_FLAG_VACANT = 8 };   /* the library's own: a vacant row (sca_retire_agents) shows at-goal | collision | vacant = 11 */

enum sca_neighbor_mode {
    SCA_NBR_KDTREE = 0,           /* replica of the reference kd-tree (built and queried on the device): exact lists */
    SCA_NBR_GRID = 1,             /* uniform hashed grid, cells of neighbor_dist, rebuilt every step by a counting sort (three short
                                     launches instead of ~17 dependent tree levels; what multi-GPU runs want).  Lists hold the
                                     reference's (object, distSq) pairs whenever <= max_neighbors objects are in range; entries of
                                     equal distSq are ordered obstacles first -- two obstacles in the order the obstacle tree's query
                                     (kdTree.py:232-262) meets them --, then agents by id (the reference: kd visit order); with more in
                                     range the agent's max_neighbors nearest in that order are kept and SCA_ST_NBR_OVERFLOW is raised
                                     (after a collision: more than max_neighbors colliding objects; the bit may also stand on an agent
                                     whose list was full before the pass met its first colliding object) */
    SCA_NBR_KDTREE_HOSTBUILD = 2, /* same tree built on the host from a position read-back (debug / A-B reference) */
    SCA_NBR_AUTO = 3              /* the reference's lists, entry for entry, at the grid's price: the grid query for every agent, and the
                                     kd query (kdTree.py:124-156) for the agents whose list the grid cannot give exactly -- more than
                                     max_neighbors objects in range, or two objects of one kind at the same rounded distance (their order is
                                     the kd-tree's visit order, agent.py:87-90).  The kd-tree is still built every step -- its permutation is
                                     history (kdTree.py:43-45) -- but on a stream of its own beside the grid build and query, in
                                     sca_run_steps already behind the previous step's integrate stage, and a pass waits for it only when the
                                     grid query listed somebody (a device-side wait, hipStreamWaitValue32).  A pass is a plain SCA_NBR_KDTREE
                                     pass where that cannot pay: with the tracker inside the pass (the neighbour branch runs beside the
                                     re-plans there), and for 256 passes whenever the grid query listed more than an eighth of the shard
                                     (rings at the 16-neighbour density, lattices of identical cells).  Measured: random N = 4096 0.128 ->
                                     0.107 ms per step, N = 16 384 0.198 -> 0.160, N = 65 536 0.382 -> 0.333. */
};

enum sca_status_bit {             /* per-agent status word of the last policy pass */
    SCA_ST_SQRT_DOMAIN = 2,       /* reference would raise ValueError (scaPolicy.py:159); clamped here */
    SCA_ST_BAD_PREF_SPEED = 4,    /* np.arange(0.5, ps+0.03, ps-0.5) does not have 2 elements (scaPolicy.py:195) */
    SCA_ST_KD_STACK = 16,         /* a kd walk had more subtrees waiting than its stack holds and dropped one.  The stack holds the children
                                     queued while the nearer one is walked -- a count of QUEUED SUBTREES, not the tree's depth: 48 in the
                                     one-wavefront neighbour query and the kd answer of SCA_NBR_AUTO, 64 in the packed neighbour query,
                                     the grid's obstacle walk, the env update's fallback walk (which ORs the bit into the walked agent's
                                     word) and the closest-approach descent.  A uniform swarm queues about 10; k agents or obstacles on
                                     ONE point queue about k - 10 for everybody within neighborDist.  A row with the bit has walked
                                     an incomplete tree: its neighbour list, its action row and its collision flag are invalid */
    SCA_ST_NBR_OVERFLOW = 32,     /* grid mode: > max_neighbors in range, reference list is visit-order dependent */
    SCA_ST_VPREF_EDGE = 128,      /* reserved, never set.  Round 5 marked agent-steps whose straight-line v_pref (rvo3dPolicy.py:182-196)
                                     had a 5-decimal rounding within 1e-9 of flipping, because positions of a free-running episode
                                     carried ~1e-14 m of device sin / cos noise; since round 6 update_velocitie (mampenv.py:83-105) and
                                     cartesian2spherical (util.py:44-55) run on the restated glibc and the episode is the reference's */
    SCA_ST_TRACKER_EDGE = 64      /* reserved, never set.  Rounds 1-2 marked agent-steps whose device-tracker v_pref might differ from the
                                     reference's by a 5-decimal step (the device ran on another libm); since round 3 the device tracker
                                     computes glibc's bits (sca_amd/csrc/sca_glibc_math.h) and equals the host tracker bit for bit */
};

enum sca_error {
    SCA_OK = 0, SCA_ERR_ARG = -1, SCA_ERR_HIP = -2, SCA_ERR_STATE = -3, SCA_ERR_NOMEM = -4, SCA_ERR_UNSUPPORTED = -5
};

void sca_default_params(sca_params *p);                 /* the version-100 entry point: writes the first 56 bytes only (struct_bytes = 0) */
void sca_default_params_v2(sca_params *p, int32_t struct_bytes);   /* every field that fits into struct_bytes, and struct_bytes itself */
#define SCA_DEFAULT_PARAMS(p) sca_default_params_v2((p), (int32_t)sizeof(sca_params))
int sca_version(void);                     /* 103 (100: round 4; 101: dt_nominal appended to sca_params; 102: struct_bytes, sca_default_params_v2;
                                              103: sca_set_paths / sca_get_path_state / sca_set_path_state, SCA_FORM_WAYPOINTS) */

int sca_create(const sca_params *p, int device, int max_agents, int max_obstacles, sca_ctx **out);
void sca_destroy(sca_ctx *ctx);
const char *sca_last_error(const sca_ctx *ctx);

/* static scene ---------------------------------------------------------------------------------- */
int sca_set_obstacles(sca_ctx *ctx, int m, const double *pos /*m*3*/, const double *radius /*m*/);
int sca_set_agents(sca_ctx *ctx, int n, const double *radius /*n*/, const double *pref_speed /*n*/,
                   const double *goal /*n*3*/, const uint8_t *policy /*n*/, const uint8_t *zaxis /*n*/,
                   const double *max_run_dist /*n*/);

/* The solver attributes PER AGENT, as the reference keeps them (agent.py:24-41: maxNeighbors, neighborDist, timeStep, timeHorizon, maxSpeed,
 * max_heading_change, dt_nominal are attributes of every Agent object, read by its own policy calls).  Arrays of n (= sca_set_agents' n); a NULL
 * array keeps the context's sca_params value for every agent; n = 0 or all NULL: back to one value per context.  Call after sca_set_agents
 * (which clears them) and before sca_device_tracker_enable.  The planner's two attributes, turning_radius and pitchlims, go per agent
 * through sca_device_tracker_set_agent_params (below).  Parity: tests/golden/F17_hetero_*. */
int sca_set_agent_params(sca_ctx *ctx, int n, const double *neighbor_dist, const int32_t *max_neighbors, const double *time_step,
                         const double *time_horizon, const double *max_speed, const double *max_heading_change, const double *dt_nominal);

/* dynamic state (host <-> device) ---------------------------------------------------------------- */
int sca_set_state(sca_ctx *ctx, const double *pos /*n*3*/, const float *vel /*n*3*/, const double *heading /*n*3*/,
                  const uint8_t *flags /*n*/, const double *total_dist /*n, nullable*/,
                  const int32_t *step_num /*n, nullable*/);
int sca_get_state(sca_ctx *ctx, double *pos, float *vel, double *heading, uint8_t *flags, double *total_dist,
                  int32_t *step_num); /* any pointer may be NULL */
/* kdTree.agentIDs: the permutation the reference carries from step to step (kdTree.py:43-45,101-111) */
int sca_set_kd_perm(sca_ctx *ctx, const int32_t *perm /*n*/);
int sca_get_kd_perm(sca_ctx *ctx, int32_t *perm /*n*/);
/* the agent kd-tree of the last policy pass, (2n-1) nodes x [begin,end,left,right,min3,max3] (kdTree.py:14-21) */
int sca_get_kd_tree(sca_ctx *ctx, double *tree_out /*(2n-1)*10*/);
/* externally computed preferred velocity (SCA / RVO3D+Dubins); mode[i]=1 uses vpref[i], 0 = straight line */
int sca_set_vpref(sca_ctx *ctx, const double *vpref /*n*3*/, const uint8_t *mode /*n*/);

/* Waypoint lists = Agent.path (agent.py:44), followed as every policy's get_trajectory does at the head of find_next_action
 * (rvo3dPolicy.py:71-85, srvo3dPolicy.py:71-85, scaPolicy.py:75-89, sca/rvo3dDubinsPolicy.py:73-87: l3norm; orca3dPolicy.py:298-312,
 * orca3dPolicyOfficial.py:302-316: distance).  Agent i's list is points[3*offsets[i] .. 3*offsets[i+1]) in list order; list.pop() takes its
 * LAST element.  Every pass, for every agent it serves (not at goal, collided or timed out), before anything reads v_pref (kernel k_waypoint):
 * empty list -> now_goal = goal; otherwise now_goal = pop() if it is None, then one more pop() if the list is not empty and either
 * l3norm(pos, now_goal) <= radius or l3norm(now_goal, goal) >= l3norm(pos, goal).  RVO3D / S-RVO3D / ORCA3D / ORCA3D-LP agents that have a
 * path aim v_pref at now_goal (rvo3dPolicy.py:29,182-196; the reached(goal, pos, 0.2) test that zeroes it stays on the global goal); SCA and
 * RVO3D+Dubins agents advance their list and keep the tracker's v_pref.
 *   sca_set_paths       after sca_set_agents (SCA_ERR_STATE before; sca_set_agents clears the lists).  n must be the context's n, offsets[0] == 0,
 *                       offsets never decrease, every point finite (SCA_ERR_ARG, nothing changed).  Resets every cursor to the full list and
 *                       now_goal to None.  n == 0 or offsets == NULL: no lists (the passes launch nothing for them).  Under the cell-owner
 *                       partition SCA_ERR_UNSUPPORTED (path state does not migrate with the agents), as is sca_partition_init with lists set.
 *                       Contiguous shards (sca_set_shard, sca_comm_init): every rank advances the agents it owns.
 *   sca_get/set_path_state  remaining[i] = elements still in agent i's list (its first remaining[i]), now_goal[i] = policy.now_goal (NaN x 3:
 *                       None).  sca_set_state leaves both alone (the reference keeps now_goal on the policy object).  SCA_ERR_STATE without lists.
 * While lists are set, sca_set_vpref refuses mode 1 for a straight-line agent that has a path (SCA_ERR_ARG), and a pass reports
 * SCA_FORM_WAYPOINTS. */
int sca_set_paths(sca_ctx *ctx, int n, const int32_t *offsets /*n+1*/, const double *points /*offsets[n]*3*/);
int sca_get_path_state(sca_ctx *ctx, int32_t *remaining /*n, nullable*/, double *now_goal /*n*3, nullable*/);
/* Read-only views of what the device holds, behind one synchronisation.  sca_get_path_slot_lists (slot form only, else SCA_ERR_STATE): the
 * lists' lengths as set and the rows' rooms whole, W points per row -- row a's list is rooms[3 W a .. 3 (W a + len[a])), what stands
 * behind it is whatever an earlier list left there.  sca_get_vpref_mode: the rows' vpref_mode bytes as the next pass will read them. */
int sca_get_path_slot_lists(sca_ctx *ctx, int32_t *len /*n, nullable*/, double *rooms /*n*W*3, nullable*/);
int sca_get_vpref_mode(sca_ctx *ctx, uint8_t *mode /*n*/);
int sca_set_path_state(sca_ctx *ctx, const int32_t *remaining /*n*/, const double *now_goal /*n*3*/);

/* The same lists in SLOT form (Agent.path, agent.py:44; the rule above is unchanged): every agent row owns room for points_per_agent
 * waypoints, so a row's list has a place that depends on no other row's and sca_restart_scenes_paths (below) can replace the lists of one
 * scene while the others keep running -- the block form above is one CSR block for the whole context and cannot.  An episode fits if its
 * longest list is at most points_per_agent.  Costs 24 * points_per_agent bytes of device memory per row of sca_create's max_agents.  Detect
 * the feature by the symbol (sca_version() is unchanged).
 *   sca_set_path_slots  sca_set_paths' rules and refusals, the partition's included, over the same CSR arguments; offsets == NULL: every
 *                       list empty.  Additionally SCA_ERR_ARG, nothing changed: points_per_agent < 1, a list longer than it, or
 *                       points_per_agent * max_agents above 2^31 / 3 points (not addressable).  Resets every cursor to the full list and
 *                       now_goal to None.  Works wherever sca_set_paths works -- with or without scenes, shards, bursts (sca_run_steps),
 *                       sca_step_host, SCA_NBR_GRID, the host build -- because it is per agent: kernel k_waypoint_slots has k_waypoint's
 *                       place at the head of the pass and its body.
 *   sca_get_path_slots  *points_per_agent = the room per row, 0 while the context is not in slot form.
 * sca_set_paths on a context in slot form puts it back into block form; sca_set_paths(0 / NULL) and sca_set_agents clear either form.
 * sca_get_path_state / sca_set_path_state, the sca_set_vpref rule, SCA_FORM_WAYPOINTS and the partition's refusals are those of the block form. */
int sca_set_path_slots(sca_ctx *ctx, int points_per_agent, int n, const int32_t *offsets /*n+1, nullable: every list empty*/,
                       const double *points /*offsets[n]*3*/);
int sca_get_path_slots(sca_ctx *ctx, int *points_per_agent);

/* Scene batches: ONE context steps many isolated episodes.  Scene s is the contiguous agent range [offsets[s], offsets[s+1]); agents of
 * different scenes never appear in each other's neighbour lists or collision tests, every scene has its own kd-tree, its own carried
 * permutation and its own `done`, and for every scene every value the context produces is bit for bit what a context holding that scene
 * alone produces.  Obstacles are either one set shared by all scenes (sca_set_obstacles) or one set per scene (sca_set_scene_obstacles,
 * below); everything per agent (sca_set_agent_params, the device tracker, sca_set_paths, sca_step_host) works as without scenes.  The
 * context-wide history log (sca_history_enable) records every agent on every CONTEXT step, finished scenes included (a finished scene's
 * agents still pass through the integrate stage with a zero action): for per-episode trajectories use the log per scene,
 * sca_scene_history_enable below.  sca_version() is unchanged: detect the feature by the symbol.
 *   sca_set_scenes      after sca_set_agents (SCA_ERR_STATE before; sca_set_agents clears the scenes).  offsets[0] == 0, strictly increasing,
 *                       offsets[nscenes] == n (SCA_ERR_ARG); every scene at most 1536 agents, KD_WAVE_CAP -- a scene's tree is built by one
 *                       workgroup (SCA_ERR_UNSUPPORTED, the message names the limit).  nscenes == 0 or offsets == NULL: no scenes, a plain
 *                       context again.  Resets the permutation to the identity (per scene 0 .. n_s-1 in scene-local terms) and the per-scene
 *                       counters.  A refused call has changed nothing.
 *   sca_get_scene_state active[s]: agents of scene s the next step would serve; steps[s]: steps taken while scene s was live = the number
 *                       of env.step() calls the reference's `while not env.step()` makes for that scene; it stops counting when active[s]
 *                       reaches 0.  Kept on the device, read back only by this call (one synchronisation).  SCA_ERR_STATE without scenes or state.
 * With scenes set: sca_env_step / sca_step_host / sca_active_count / sca_env_update report the sum over the scenes, so `while (active)` runs
 * until the last scene is done; a finished scene is inert (all its agents are flagged, its state -- velocities, step_num and headings
 * included, which a running env's update would still touch for a done agent -- and its permutation stay what they were at its last step,
 * its action rows are zero).  sca_get_kd_perm / sca_set_kd_perm carry GLOBAL ids: within scene s the
 * values are offsets[s] + the scene's own permutation, and sca_set_kd_perm refuses (SCA_ERR_ARG) a permutation that moves an id out of its
 * scene.  Neighbour modes: SCA_NBR_KDTREE is the scene form and SCA_NBR_AUTO resolves to it; SCA_NBR_GRID and SCA_NBR_KDTREE_HOSTBUILD are
 * SCA_ERR_UNSUPPORTED.  Also SCA_ERR_UNSUPPORTED with scenes set -- and sca_set_scenes while they are active --: sca_set_shard (other than
 * the whole range), sca_comm_init, sca_partition_init, sca_get_kd_tree.  A pass reports SCA_FORM_SCENES. */
int sca_set_scenes(sca_ctx *ctx, int nscenes, const int32_t *offsets /*nscenes+1*/);
int sca_get_scene_state(sca_ctx *ctx, int32_t *active /*nscenes, nullable*/, int32_t *steps /*nscenes, nullable*/);

/* Every scene its own obstacle set: scene s meets obstacles [obs_offsets[s], obs_offsets[s+1]) and no others; a scene may have none.  The
 * scene contract extends to them: for every scene every value (state, float32 action rows, neighbour lists and their distSq, diagnostics,
 * kd permutation, tracker and waypoint results) is bit for bit what a context holding that scene alone with that obstacle set produces --
 * the library keeps one obstacle tree per scene, built over that scene's obstacles alone.  Obstacle ids reported by sca_get_neighbors are
 * GLOBAL (obs_offsets[s] + the scene's own id), as agent ids are.  Detect the feature by the symbol (sca_version() is unchanged).
 *   order      after sca_set_scenes; SCA_ERR_STATE before it (or after whatever cleared the scenes).
 *   refusals   SCA_ERR_ARG: nscenes different from the context's, obs_offsets NULL, obs_offsets[0] != 0, decreasing offsets, a total
 *              obs_offsets[nscenes] above sca_create's max_obstacles, pos or radius NULL with a positive total.  A refused call has changed nothing.
 *   lifetime   a later sca_set_obstacles puts the context back on one shared set.  Whatever drops or redefines the scenes -- sca_set_agents,
 *              sca_set_scenes, sca_set_scenes(0, NULL) -- also drops the per-scene sets and LEAVES THE CONTEXT WITHOUT OBSTACLES (a shared
 *              set that was replaced by per-scene sets does not come back): set obstacles again afterwards.  A total of 0 is "no obstacles".
 * A pass with per-scene sets reports SCA_FORM_SCENE_OBSTACLES beside SCA_FORM_SCENES; a context with scenes and a shared set does not. */
int sca_set_scene_obstacles(sca_ctx *ctx, int nscenes, const int32_t *obs_offsets /*nscenes+1*/,
                            const double *pos /*obs_offsets[nscenes]*3*/, const double *radius /*obs_offsets[nscenes]*/);

/* Restarting scenes in place: a new episode into a slot while the other slots keep running, so that a queue of any length streams through
 * B slots.  T is the total agent count of the named scenes; the arrays are packed in the order of scene_ids, each scene's rows in its own
 * agent order.  After the call every named scene is what a context holding that episode alone is right after sca_set_agents +
 * sca_set_state (zero flags, zero total_dist, zero step_num, identity permutation) and, with the device tracker on, after
 * sca_device_tracker_enable; from there on every value of the scene (state, float32 action rows, neighbour lists and their distSq,
 * diagnostics, status, the scene-local permutation, tracker v_pref, plans and re-plan counts) is bit for bit that context's.  Every scene not
 * named is untouched: its values before, at and after the call are what they would have been without it.  A scene may be restarted whether
 * it is finished or live.  Detect the feature by the symbol (sca_version() is unchanged).
 *   reset      the scene's records (position, velocity, flags 0, radius), heading, total_dist, step_num, the constants that were passed
 *              (goal, pref_speed, max_run_dist, policy, zaxis), v_pref (0; taken from the tracker exactly by SCA / RVO3D+Dubins agents while
 *              one is enabled), the scene's slice of the kd permutation (identity), its neighbour lists, the tracker's records and
 *              goal_heading, and the scene's counters: steps[s] = 0, active[s] = n_s -- sca_env_step / sca_step_host / sca_active_count
 *              count the scene again, and a batch that had reached 0 comes back to life.
 *   kept       the slot's agent count, its per-agent solver attributes (sca_set_agent_params) and its per-agent tracker attributes --
 *              unless the restart brings the episode's own (sca_restart_scenes_attrs, below); every array passed as NULL (vel: zero).  The obstacles the scene meets stay too -- unless the restart brings the episode's own
 *              (sca_restart_scenes_obstacles, below).
 *   refusals   SCA_ERR_STATE: no scenes, no state yet, between a policy pass and its env update.  SCA_ERR_ARG: count <= 0 or scene_ids
 *              NULL, an id outside 0 .. nscenes-1, a repeated id, pos or heading NULL, any number that is not finite, a policy above
 *              SCA_POLICY_RVO3D_DUBINS, a radius / pref_speed / max_run_dist that is not positive, goal_heading without a device tracker.
 *              SCA_ERR_UNSUPPORTED: waypoint lists are set in block form (sca_set_paths: one block for all agents; in slot form,
 *              sca_set_path_slots, every restart entry point is accepted -- see sca_restart_scenes_paths), or a policy that moves an agent
 *              between tracked (SCA, RVO3D+Dubins) and untracked while per-agent tracker attributes are set (their classes are cut by
 *              policy).  A refused call has changed nothing.
 *   cost       one kernel launch and one stream synchronisation however many scenes are named (one more small copy where a policy changed
 *              the ORCA3D-LP list); the arrays travel through a page-locked block of the library's own, allocated once.
 *   harvest    with sca_scene_harvest_enable on, the call clears the `fresh` word of every named scene: a harvest that was not collected
 *              (sca_scene_harvest_collect) before its scene is restarted is gone. */
int sca_restart_scenes(sca_ctx *ctx, int count, const int32_t *scene_ids /*count*/,
                       const double *pos /*T*3*/, const float *vel /*T*3, nullable: zero*/, const double *heading /*T*3*/,
                       const double *radius, const double *pref_speed, const double *goal /*T*3*/, const uint8_t *policy,
                       const uint8_t *zaxis, const double *max_run_dist,      /* each T, each nullable: keep the slot's */
                       const double *goal_heading /*T*3, nullable: keep the slot's*/);

/* Slots of a capacity: a scene's range [offsets[s], offsets[s+1]) is its CAPACITY, and the scene holds size[s] agents, 1 <= size[s] <=
 * capacity, in the first size[s] rows of the range; the rows behind them are VACANT.  So a slot takes any episode that fits it, and a queue
 * that mixes 14-, 50- and 100-agent episodes streams through one set of slots.  The scene contract extends: a slot that holds an n-agent
 * episode is bit for bit what a context holding that episode alone is (state, float32 action rows, neighbour lists and their distSq,
 * diagnostics, the scene-local permutation, tracker records and re-plan counts, the rows of the log per scene), and no other scene can
 * tell.  Detect the feature by the symbol (sca_version() is unchanged).
 *   sca_restart_scenes_sized  sca_restart_scenes with sizes[b] rows for scene scene_ids[b]: T is the sum of the sizes, the arrays are packed in
 *              the order of scene_ids.  sizes == NULL: every named scene is filled to its capacity -- the call is then exactly
 *              sca_restart_scenes (which, on a scene that holds fewer agents, fills it to its capacity too).  A slot may shrink or grow from
 *              one restart to the next, whether it is finished or live.  Same cost: one kernel launch and one synchronisation however many
 *              scenes are named.  Refusals: sca_restart_scenes', each with its code, and SCA_ERR_ARG for a size < 1 or above the slot's
 *              capacity (the message names the entry).  A refused call has changed nothing.
 *   sca_get_scene_sizes       size[s] of every scene.  sca_set_scenes sets every size to its capacity; sca_set_agents and
 *              sca_set_scenes(0, NULL) drop the sizes with the scenes.  SCA_ERR_STATE without scenes.  A context that never calls the sized
 *              restart has every scene full and behaves exactly as before (the one restart kernel serves all three entry points: on a
 *              full scene it vacates an empty range and rewrites the size the scene has).
 *   vacant rows   belong to the library.  The read-backs over the whole range (sca_get_state, sca_get_kd_perm, sca_get_actions,
 *              sca_get_neighbors, sca_get_diag) still cover them: a vacant row reads flags SCA at-goal | collision (3), zero velocity, zero
 *              heading, zero total_dist and step_num, the position and radius of whoever stood there last, a zero action row, an empty
 *              neighbour list, the diagnostics of a done agent (-1), and the identity in the permutation (perm[a] == a; the occupied
 *              rows are a permutation of [offsets[s], offsets[s] + size[s])).  They stay exactly so from one restart to the next: a vacant
 *              row is in no tree, no neighbour or near list, no collision test, no tracker list and not in the ORCA3D-LP list, and is never
 *              counted in active[s] or by sca_active_count.  It keeps its per-agent attributes (sca_set_agent_params, tracker
 *              attributes) and constants for the episode that occupies it next.
 *   refused meanwhile   while ANY scene is below its capacity, the entry points that take a whole-context state from outside return
 *              SCA_ERR_UNSUPPORTED and change nothing: sca_set_state, sca_set_kd_perm, and sca_step_host with its host state block (whose
 *              rows cannot say which are vacant).  They work again once every slot is filled to its capacity.
 *   the log per scene   keeps its layout (pitch = capacity, so a full slot reads as before); sca_get_scene_history bounds the agent window by
 *              the scene's current size (SCA_ERR_ARG beyond it): vacant rows are never reported. */
int sca_restart_scenes_sized(sca_ctx *ctx, int count, const int32_t *scene_ids /*count*/, const int32_t *sizes /*count, nullable: capacities*/,
                             const double *pos /*T*3*/, const float *vel /*T*3, nullable: zero*/, const double *heading /*T*3*/,
                             const double *radius, const double *pref_speed, const double *goal /*T*3*/, const uint8_t *policy,
                             const uint8_t *zaxis, const double *max_run_dist,      /* each T, each nullable: keep the slot's */
                             const double *goal_heading /*T*3, nullable: keep the slot's*/);
int sca_get_scene_sizes(sca_ctx *ctx, int32_t *size /*nscenes*/);

/* Obstacle slots: a scene's obstacle range becomes a CAPACITY, as its agent range did with sca_restart_scenes_sized, so that a restarted
 * slot takes the episode's own obstacles -- the take-off field's 8 spheres, the 1491 of a map, the 1-5 of a random scene -- and a queue
 * that mixes such episodes streams through one set of slots.  Detect the feature by the symbol (sca_version() is unchanged).
 *   sca_set_scene_obstacle_slots   scene s owns obstacle rows [cap_offsets[s], cap_offsets[s+1]) and holds counts[s] obstacles, 0 <=
 *              counts[s] <= capacity, in the first of them; pos and radius are packed densely in scene order (sum(counts) rows).  counts ==
 *              NULL: every slot starts empty.  The scene's tree is the one sca_set_scene_obstacles builds -- the same host routine over that
 *              scene's obstacles alone with local ids -- standing at node record 2 * cap_offsets[s]; a tree over k obstacles has 2k - 1
 *              nodes, so it always fits the 2 x capacity records of the range.  An empty slot has no tree and no obstacle walk happens for
 *              its agents.  Obstacle ids in neighbour lists are GLOBAL: cap_offsets[s] + the scene's own id.  With every count equal to its
 *              capacity the context is left exactly as sca_set_scene_obstacles(nscenes, cap_offsets, pos, radius) leaves it; that call in
 *              turn leaves slots that are full.  A pass reports SCA_FORM_SCENE_OBSTACLES, also while every slot is empty.
 *   order, lifetime   as sca_set_scene_obstacles: after sca_set_scenes (SCA_ERR_STATE before); a later sca_set_obstacles or
 *              sca_set_scene_obstacles replaces the slots; whatever drops or redefines the scenes drops them and leaves the context without
 *              obstacles.
 *   refusals   SCA_ERR_ARG: nscenes different from the context's, cap_offsets NULL, cap_offsets[0] != 0, decreasing offsets, a total
 *              capacity above sca_create's max_obstacles, a count outside 0 .. capacity, a position that is not finite, a radius that is
 *              not positive, pos or radius NULL with a positive sum of counts.  A refused call has changed nothing.
 *   sca_get_scene_obstacle_counts  the obstacles each scene holds and its capacity (either pointer may be NULL).  SCA_ERR_STATE without
 *              scenes or without per-scene sets.
 *   sca_restart_scenes_obstacles   sca_restart_scenes_sized (sizes == NULL: capacities) that also brings the episodes' obstacles.
 *              obs_counts == NULL: exactly sca_restart_scenes_sized.  obs_counts[e] == -1: scene scene_ids[e] KEEPS its set -- seeds that
 *              share a map: nothing is rebuilt and nothing but its head word, which says so, is staged for it.  0 .. capacity: the scene's set is REPLACED by the next
 *              obs_counts[e] rows of obs_pos / obs_radius, which hold the replaced scenes' obstacles packed in the order of scene_ids.
 *              The scene contract extends: after the call a named scene is bit for bit a context that holds that episode alone after
 *              sca_set_agents + sca_set_obstacles(that set) + sca_set_state (+ the tracker's enable) -- state, float32 action rows,
 *              neighbour lists with their distSq and global obstacle ids, diagnostics, status, permutation, tracker records, the rows of
 *              the log per scene and the harvest -- and no other scene can tell the call happened.  Rows and tree records of the slot behind
 *              the new count keep what an earlier set left and are unreachable.
 *              Refusals: those of sca_restart_scenes_sized, and SCA_ERR_STATE for a count >= 0 while the context has no per-scene sets;
 *              SCA_ERR_ARG for a count below -1 or above the slot's capacity, an obstacle position that is not finite, a radius that is
 *              not positive, obs_pos or obs_radius NULL with a positive total (each message names the entry).  A refused call has changed
 *              nothing, obstacles included.
 *              Cost: still one kernel launch and one stream synchronisation however many scenes are named; the replaced scenes' trees are
 *              built on the host into the page-locked block and copied to their place by that launch.  It is the launch of
 *              sca_restart_scenes and sca_restart_scenes_sized too: one kernel, of which a scene filled to its capacity and a scene that
 *              keeps its set are the degenerate cases (an empty range to vacate; a return behind the agent rows). */
int sca_set_scene_obstacle_slots(sca_ctx *ctx, int nscenes, const int32_t *cap_offsets /*nscenes+1*/,
                                 const int32_t *counts /*nscenes, nullable: every slot empty*/,
                                 const double *pos /*sum(counts)*3*/, const double *radius /*sum(counts)*/);
int sca_get_scene_obstacle_counts(sca_ctx *ctx, int32_t *counts /*nscenes, nullable*/, int32_t *capacities /*nscenes, nullable*/);
int sca_restart_scenes_obstacles(sca_ctx *ctx, int count, const int32_t *scene_ids /*count*/, const int32_t *sizes /*count, nullable: capacities*/,
                                 const int32_t *obs_counts /*count, nullable*/, const double *obs_pos, const double *obs_radius,
                                 const double *pos /*T*3*/, const float *vel /*T*3, nullable: zero*/, const double *heading /*T*3*/,
                                 const double *radius, const double *pref_speed, const double *goal /*T*3*/, const uint8_t *policy,
                                 const uint8_t *zaxis, const double *max_run_dist,      /* each T, each nullable: keep the slot's */
                                 const double *goal_heading /*T*3, nullable: keep the slot's*/);

/* A restarted slot takes the episode's own ATTRIBUTES: the solver attributes the reference keeps on every Agent (agent.py:24-41,
 * sca_set_agent_params) and the planner's (turning_radius, pitchlims; sca_device_tracker_set_agent_params), so that a parameter study --
 * a sweep of neighbour distance, neighbour count, time horizon or turning radius across seeds -- streams through one set of slots.
 * Detect the feature by the symbol (sca_version() is unchanged).
 *   sca_restart_scenes_attrs   sca_restart_scenes_obstacles plus a descriptor.  attrs == NULL: exactly sca_restart_scenes_obstacles -- the
 *              slot keeps its attributes, and the tracked <-> untracked refusal stays.  attrs != NULL: the named scenes' occupied rows take
 *              the arrays' values, T rows each, packed like pos.  A NULL array inside the struct means the value a context alone would
 *              have for every named row -- sca_create's sca_params value, sca_device_tracker_enable's value -- NOT what the row had before
 *              (as in sca_set_agent_params).  Planner entries of untracked rows are ignored.  A policy that moves an agent between tracked
 *              and untracked is accepted: the tracker's classes are recomputed after every such call over the occupied tracked rows.
 *              The scene contract extends: after the call a named scene is bit for bit a context that holds that episode alone after
 *              sca_set_agents + sca_set_agent_params(those arrays) + sca_set_obstacles + sca_set_state + sca_device_tracker_enable +
 *              sca_device_tracker_set_agent_params(those arrays) -- state, float32 action rows, neighbour lists with their distSq,
 *              diagnostics, status, permutation, tracker records, plans and re-plan counts, the rows of the log per scene and the harvest
 *              -- and no other scene can tell the call happened.  Vacant rows keep their attributes.
 *   struct_bytes   sizeof(sca_restart_attrs) as the caller compiled it: members behind it read as NULL.  reserved: 0.
 *   refusals   those of sca_restart_scenes_obstacles, and SCA_ERR_ARG for a struct_bytes below the two leading integers, above the
 *              library's struct or cutting a pointer in two; reserved != 0; planner arrays while no device tracker is enabled; a row whose
 *              solver attributes break sca_set_agent_params' rules or, for a tracked row, whose planner attributes break
 *              sca_device_tracker_set_agent_params' (the message names the packed row).  A refused call has changed nothing.
 *   cost       one kernel launch and one stream synchronisation however many scenes are named.  The first call that brings attributes
 *              into a context without per-agent arrays allocates them and fills every row with the context's own values, from which the
 *              rows of the other scenes compute the bits they computed before.  One more small copy (the class bytes, one per agent)
 *              where the call takes the tracker back from the per-agent form to classes. */
typedef struct sca_restart_attrs {
    int32_t struct_bytes;            /* sizeof as the caller compiled it */
    int32_t reserved;                /* 0 */
    /* each T rows packed like pos; NULL = the CONTEXT's sca_params value for every named row */
    const double *neighbor_dist; const int32_t *max_neighbors; const double *time_step, *time_horizon,
                 *max_speed, *max_heading_change, *dt_nominal;
    /* each T rows; NULL = sca_device_tracker_enable's value for every named row; ignored for untracked rows */
    const double *turning_radius, *pitch_lo, *pitch_hi;
} sca_restart_attrs;
int sca_restart_scenes_attrs(sca_ctx *ctx, int count, const int32_t *scene_ids /*count*/, const int32_t *sizes /*count, nullable: capacities*/,
                             const int32_t *obs_counts /*count, nullable*/, const double *obs_pos, const double *obs_radius,
                             const sca_restart_attrs *attrs /*nullable: the slots keep their attributes*/,
                             const double *pos /*T*3*/, const float *vel /*T*3, nullable: zero*/, const double *heading /*T*3*/,
                             const double *radius, const double *pref_speed, const double *goal /*T*3*/, const uint8_t *policy,
                             const uint8_t *zaxis, const double *max_run_dist,      /* each T, each nullable: keep the slot's */
                             const double *goal_heading /*T*3, nullable: keep the slot's*/);

/* A restarted slot takes the episode's own WAYPOINT LISTS (Agent.path, agent.py:44; every reference policy's find_next_action starts with
 * get_trajectory, e.g. rvo3dPolicy.py:71-85), so that a table whose scenarios route the drones through waypoints streams through one set of
 * slots.  The context's lists must be in slot form (sca_set_path_slots).  Detect the feature by the symbol (sca_version() is unchanged).
 *   sca_restart_scenes_paths   sca_restart_scenes_attrs plus the lists.  path_offsets: CSR over the call's T packed rows, packed like pos
 *              (row r's list is path_points[3*path_offsets[r] .. 3*path_offsets[r+1]) in list order).  path_offsets == NULL: exactly
 *              sca_restart_scenes_attrs.  In slot form EVERY restart entry point is accepted, and a call without path arrays gives the named
 *              rows empty lists: the episode brings none.  In block form SCA_ERR_UNSUPPORTED stays for every entry point.
 *              The scene contract extends: after the call a named scene is bit for bit a context of that episode alone after
 *              sca_set_agents + ... + sca_set_paths(those lists) + sca_set_state -- everything listed at sca_restart_scenes_attrs, and
 *              `remaining`, now_goal and the v_pref every pass uses -- and no other scene can tell the call happened.  Occupied rows get
 *              remaining = the list's length and now_goal = None; vacant rows remaining 0 and None.
 *   refusals   those of sca_restart_scenes_attrs, and SCA_ERR_STATE: path arrays while the context is not in slot form; SCA_ERR_ARG:
 *              path_offsets[0] != 0, offsets that decrease, a row's list longer than the room per row, path_points NULL with points to
 *              read, a point that is not finite (the message names the packed row).  A refused call has changed nothing.
 *   cost       still one kernel launch and one stream synchronisation however many scenes are named: the offsets and the points actually
 *              present travel packed in the page-locked block (which grows once when slot form, or a larger room, arrives after the
 *              first restart) and the kernel scatters them to the rows' rooms. */
int sca_restart_scenes_paths(sca_ctx *ctx, int count, const int32_t *scene_ids /*count*/, const int32_t *sizes /*count, nullable: capacities*/,
                             const int32_t *obs_counts /*count, nullable*/, const double *obs_pos, const double *obs_radius,
                             const sca_restart_attrs *attrs /*nullable: the slots keep their attributes*/,
                             const int32_t *path_offsets /*T+1, nullable: no lists*/, const double *path_points /*path_offsets[T]*3*/,
                             const double *pos /*T*3*/, const float *vel /*T*3, nullable: zero*/, const double *heading /*T*3*/,
                             const double *radius, const double *pref_speed, const double *goal /*T*3*/, const uint8_t *policy,
                             const uint8_t *zaxis, const double *max_run_dist,      /* each T, each nullable: keep the slot's */
                             const double *goal_heading /*T*3, nullable: keep the slot's*/);

/* A trajectory log per scene = every episode's Agent.history_info.  Row r of scene s is the scene's r-th own step (r = steps[s] - 1 while
 * that step runs), written only for steps the scene was live at their beginning, so a finished scene gains no row while the others run on,
 * and the log starts over at row 0 when the scene is restarted.  For every scene the rows are bit for bit the rows sca_get_history gives
 * for a context that holds that episode alone with sca_history_enable, and no other scene's log can tell that a scene finished,
 * overflowed or was restarted.  Written by one kernel of its own in front of the step's last one, in every step form (sca_env_step,
 * sca_run_steps, sca_step_host, sca_policy_pass + sca_env_update, an sca_env_update alone); a context without the log enqueues what it
 * did.  The context-wide log (sca_history_enable) is independent and may be on at the same time.  64 bytes per agent per row, allocated
 * up front: capacity_rows x n x 64 bytes.  Detect the feature by the symbol (sca_version() is unchanged).
 *   sca_scene_history_enable  capacity_rows is PER SCENE; 0 frees the log.  SCA_ERR_STATE: no scenes, between a policy pass and its env
 *              update, or (capacity > 0) a scene that has taken a step already -- enable the log behind sca_set_scenes / sca_set_state,
 *              before the first step: rows are indexed by the scene's own step count, and rows that were never written must not be
 *              reported as logged.  SCA_ERR_ARG: a negative capacity.  A refused call has changed nothing.
 *   sca_scene_history_rows    rows_logged[s] = min(steps[s], capacity), rows_dropped[s] = max(0, steps[s] - capacity): steps beyond the
 *              capacity are counted, never written.  One synchronisation for all scenes.  (Between a policy pass and its env update the
 *              step under way is not counted: its row is not written yet.)
 *   sca_get_scene_history     a window of rows and SCENE-LOCAL agents of one scene, [row][agent][3] like sca_get_history: one contiguous
 *              device-to-host copy.  Any output pointer may be NULL.
 *   refusals of the two       SCA_ERR_STATE: no scenes, or the log is not enabled.  SCA_ERR_ARG: a scene outside 0 .. nscenes-1, a row window
 *              outside [0, rows_logged[scene]), an agent window outside the scene.
 *   lifetime   whatever drops or redefines the scenes -- sca_set_agents, sca_set_scenes, sca_set_scenes(0, NULL) -- frees the log, as it
 *              drops the per-scene obstacle sets.  sca_restart_scenes keeps the allocation and starts the named scenes' logs over (stale
 *              rows of the episode before are beyond rows_logged).  sca_set_state leaves steps[s] alone, so the log goes on. */
int sca_scene_history_enable(sca_ctx *ctx, int capacity_rows);
int sca_scene_history_rows(sca_ctx *ctx, int32_t *rows_logged /*nscenes, nullable*/, int32_t *rows_dropped /*nscenes, nullable*/);
int sca_get_scene_history(sca_ctx *ctx, int scene, int first_row, int nrows, int agent_begin, int agent_count,
                          double *pos, double *heading, float *vel);

/* Finished scenes hand over their result WITH THE STEP.  With the harvest enabled a step enqueues one more kernel behind its last one
 * (k_scene_harvest, a workgroup per scene) that writes into ONE page-locked block of the library's, readable after the synchronisation the
 * step makes anyway: every scene's counters on every step (what sca_get_scene_state reads after a step), and, for a scene that FINISHED IN
 * THAT STEP (agents live when the step began, none after it), the scene's occupied rows in the columns of sca_get_state plus one
 * sca_scene_summary.  So the host learns which scenes are done and takes their final state without sca_get_scene_state's second
 * synchronisation and without sca_get_state's read-back of the whole context.  Every scene has a fixed place in the block -- counters[2 s],
 * summary[s], rows offsets[s] + i: the index the rows have in sca_get_state -- so nothing depends on the order scenes finish in, and a scene
 * finishes at most once between two restarts, so nothing is overwritten unread.  Works behind every step form (sca_env_step, sca_run_steps
 * -- a burst accumulates --, sca_step_begin / sca_step_end, sca_policy_pass + sca_env_update, sca_step_host).  A context without the harvest
 * enqueues exactly what it did; sca_get_scene_state and sca_get_state are unchanged.  Detect the feature by the symbol.
 *   sca_scene_harvest_layout  byte offsets of the eight sections (the order of sca_scene_harvest's pointers), each on a 128-byte boundary,
 *              and the block's size, for nscenes scenes over n agent rows.  Pure host arithmetic.  SCA_ERR_ARG: nscenes <= 0, n < nscenes,
 *              a NULL pointer.
 *   sca_scene_harvest_enable  on != 0: allocates the block (mapped, coherent, zeroed), fills the counters from the scenes as they stand
 *              (where a state is set) and starts batch_step at 0; enabling again starts over with a fresh block.  on == 0 frees it.
 *              SCA_ERR_STATE: no scenes, or between a policy pass and its env update.  Whatever clears or redefines the scenes
 *              (sca_set_agents, sca_set_scenes) drops the harvest, as it drops the log per scene: pointers handed out are then stale.
 *   sca_scene_harvest_get     pointers into the block and its counts.  struct_bytes = sizeof(sca_scene_harvest) as the caller compiled it
 *              (sca_host_state_get's rule: at least the leading integers, at most this library's struct, else SCA_ERR_ARG; only the
 *              pointers that fit are written).  SCA_ERR_STATE: no scenes, harvest not enabled.
 *   sca_scene_harvest_collect one stream synchronisation (free directly after sca_env_step), then a host scan of the nscenes `fresh` words:
 *              the scenes that finished since the previous collect, in ascending (batch_step, scene id), into scene_ids[nscenes]; *count
 *              of them.  Their `fresh` words are cleared; their rows and summaries stay readable until the scene is restarted or finishes
 *              again.  SCA_ERR_STATE: no scenes, not enabled.  SCA_ERR_ARG: a NULL pointer.
 *   fresh words cleared without a collect: sca_restart_scenes[_sized] clears those of the named scenes (behind the call's own
 *              synchronisation, when no step is in flight) -- an UNCOLLECTED harvest of a restarted scene is gone, collect before you
 *              restart; sca_set_state and sca_step_host with SCA_HOST_IN_STATE clear all of them (a state from outside: nothing that
 *              finished before it is reported after it).
 *   counters   live / steps of every scene after the last env update (at enable: as the scenes stand).  Between a policy pass and its env
 *              update, and behind sca_restart_scenes or sca_set_state, they are still the last update's: sca_get_scene_state knows better
 *              then.
 *   batch_step counts the context's env updates since the harvest was enabled, the first being 1. */
typedef struct sca_scene_summary {       /* 64 bytes */
    int32_t fresh;                       /* 1: written since the last collect / restart of this scene */
    int32_t steps;                       /* the scene's own step count when it finished */
    int32_t batch_step;                  /* the env update (since enable, from 1) it finished in */
    int32_t arrived, collided, timed_out;/* occupied rows by flag (a row may count in more than one) */
    int32_t successful_num;              /* rows with neither the collision nor the timeout flag */
    int32_t reserved0;
    int64_t all_step_num;                /* sum of step_num over the successful rows */
    double  all_distance;                /* sum of total_dist over the successful rows, added in ascending row order from 0.0 */
    int64_t reserved1[2];
} sca_scene_summary;
typedef struct sca_scene_harvest {       /* pointers into ONE page-locked allocation of the library's */
    int32_t struct_bytes, nscenes, n, reserved;
    int32_t *counters;                   /* nscenes*2: live, steps -- every step */
    sca_scene_summary *summary;          /* nscenes */
    double  *pos;                        /* n*3  } rows offsets[s] .. offsets[s] + size[s] - 1 of a finished scene; */
    float   *vel;                        /* n*3  } other rows are never written                                    */
    double  *heading;                    /* n*3  } */
    uint8_t *flags;                      /* n    } */
    double  *total_dist;                 /* n    } */
    int32_t *step_num;                   /* n    } */
} sca_scene_harvest;
int sca_scene_harvest_layout(int nscenes, int n, int64_t *offsets /*8, in the struct's order*/, int64_t *total_bytes);
int sca_scene_harvest_enable(sca_ctx *ctx, int on);
int sca_scene_harvest_get(sca_ctx *ctx, sca_scene_harvest *out, int32_t struct_bytes);
int sca_scene_harvest_collect(sca_ctx *ctx, int32_t *scene_ids /*nscenes*/, int32_t *count);

/* Scene checkpoints: a running episode out of its slot as a blob of bytes, and back into any slot.  A checkpoint holds the scene's MUTABLE
 * state only, for the rows the scene occupies; the episode's definition -- constants, attributes, obstacles, waypoint lists, goal headings
 * -- stays what the restart entry points take.  Resuming is therefore sca_restart_scenes* (any of them, with the episode's definition),
 * then sca_load_scenes.  The contract extends the scene contract above: after restart(E) + load(a blob taken from a scene holding E after
 * its k-th step) the named scene is bit for bit the scene the blob was taken from, from there on -- state, float32 action rows, neighbour
 * lists and their distSq, diagnostics, status, the scene-local permutation, tracker v_pref, plans and re-plan counts, remaining /
 * now_goal, steps[s] and active[s] -- and no other scene can tell that either call happened.  That holds in the same context, in another
 * slot with another range, capacity or obstacle base, and in another context or process: the blob is pointer-free and speaks scene-local
 * terms.  Detect the feature by the symbol (sca_version() is unchanged).
 *   in the blob  a 64-byte header (magic, format version, sca_version(), size, the tracker record's words, the public record's bytes,
 *              whether tracker records and path cursors are present, steps / live / prev, the byte count, a 64-bit checksum of everything
 *              behind the header), then per occupied row: the policy byte (compared with the scene's at the load, not loaded), the public
 *              record (position, float32 velocity, flags, radius), heading, the heading kept for a finished scene, v_pref as fed / tracked
 *              and its mode, total_dist, step_num, status, the kd permutation in scene-local terms, and -- with a device tracker and a
 *              tracked row in the scene -- the first neighbour's distSq the tracker reads and the tracker records (plan, cursor, now_goal,
 *              v_pref, re-plan count), and -- with waypoint lists set -- remaining and now_goal.  Between the load and the next pass
 *              sca_get_state, sca_get_kd_perm, sca_get_scene_state, sca_get_path_state, sca_device_tracker_replans,
 *              sca_device_tracker_debug and sca_active_count return what they returned on the source at the save.
 *   not in it  the OUTPUTS of the last pass: the action rows (sca_get_actions), the neighbour lists (sca_get_neighbors, sca_get_nbr0) and
 *              diag / vpref_used of sca_get_diag read what the restart left until the next pass writes them -- every pass writes them for
 *              every row before it reads them.  `status` does outlive a pass for a row the pass does not serve and IS in the blob.
 *   sca_scene_checkpoint_layout  byte offsets of the 14 sections (policy, records, heading, kept heading, v_pref, total_dist, step_num,
 *              status, permutation, v_pref mode, tracker distSq, tracker records, remaining, now_goal; an absent section has length 0) and
 *              the blob's size, for `size` rows, a tracker record of trk_words 4-byte words (0: none) and has_paths 0 / 1.  Pure.
 *              SCA_ERR_ARG: size outside 1 .. 1536, negative trk_words, has_paths not 0 / 1, a NULL pointer.
 *   sca_scene_checkpoint_info    the header's fields, after the WHOLE check of the blob that a load makes without a scene (envelope and
 *              payload, below).  Pure, no context.  struct_bytes: sca_scene_harvest_get's rule.
 *   sca_scene_checkpoint_bytes   the size of the blob sca_save_scenes writes for the scene as it stands now.
 *   sca_save_scenes  out[e] (out_bytes[e] bytes) receives scene scene_ids[e].  A scene below its capacity saves its occupied rows only.
 *   sca_load_scenes  in[e] (in_bytes[e] bytes) goes into scene scene_ids[e], which must hold the blob's episode: its size and its rows'
 *              policies are compared.  Clears the named scenes' `fresh` words of the harvest like a restart.
 *   cost       each call is one kernel launch (a workgroup per named scene) and one stream synchronisation however many scenes are named
 *              (a save directly behind sca_set_state recounts the scenes' counters first, as sca_get_scene_state does); the bytes travel
 *              through a page-locked block of the library's own, which grows once when a call needs more.
 *   log        steps[s] is restored, so the log per scene (sca_scene_history_enable) goes on writing row steps[s] - 1: rows >= k of a
 *              resumed scene are bit for bit the source's, rows < k are NOT the library's to fill -- they hold what the slot's memory held;
 *              the caller keeps the source's rows 0 .. k-1 beside the blob if it wants the whole episode.
 *   refusals   decided on the host before any device work; a refused call has changed nothing.  SCA_ERR_STATE: no scenes, no state yet,
 *              between a policy pass and its env update.  SCA_ERR_ARG, the call: count <= 0 or a NULL array or buffer, an id outside
 *              0 .. nscenes-1, a repeated id, an output buffer too small (the message names the bytes needed).  SCA_ERR_ARG at a load,
 *              the envelope: wrong magic or format version, a byte count that is not the layout's, a checksum mismatch, trk_words or the
 *              record size not this library's; the blob against the scene: a size other than the scene's current size, policy bytes that
 *              differ from the scene's rows, tracker records present or absent against what the scene's policies need in this context
 *              (present exactly when a device tracker is enabled and a row is SCA / RVO3D+Dubins), cursors with remaining > 0 and no
 *              lists set, remaining[i] outside 0 .. the row's list length as set; the payload: a permutation that is not one of
 *              0 .. size-1, unknown flag bits, a position that is not finite, a radius that is not positive, counters out of range (live
 *              must be the number of rows without a flag), any tracker integer a kernel uses as a cursor, count or switch outside its
 *              range.  A damaged blob never reaches the device. */
struct sca_scene_checkpoint_info {       /* (a struct tag: the function of the same name fills it) */
    int32_t struct_bytes, reserved;
    int32_t format, lib_version;         /* the blob's format version; sca_version() of the library that wrote it */
    int32_t size, trk_words, record_bytes;
    int32_t has_tracker, has_paths;      /* 0 / 1 */
    int32_t steps, live, prev;           /* the scene's counters at the save */
    int64_t total_bytes;
    uint64_t checksum;
};
int sca_scene_checkpoint_layout(int size, int trk_words, int has_paths, int64_t *offsets /*14*/, int64_t *total_bytes);
int sca_scene_checkpoint_info(const void *blob, int64_t bytes, struct sca_scene_checkpoint_info *out, int32_t struct_bytes);
int sca_scene_checkpoint_bytes(sca_ctx *ctx, int scene, int64_t *bytes);
int sca_save_scenes(sca_ctx *ctx, int count, const int32_t *scene_ids /*count*/, void *const *out /*count*/, const int64_t *out_bytes /*count*/);
int sca_load_scenes(sca_ctx *ctx, int count, const int32_t *scene_ids /*count*/, const void *const *in /*count*/, const int64_t *in_bytes /*count*/);

/* Context checkpoints: a running PLAIN context -- no scenes -- out as one blob of bytes, and back into a fresh context.  What the scene
 * checkpoints above are to an episode, this is to a whole swarm with everything a long run leaves in it: respawned rows, missions taken
 * from the tables, lists rewritten by takes, rows waiting at the gate, results not yet collected, closest-approach records.  The blob holds
 * the MUTABLE state only; the run's DEFINITION stays the caller's and is set up before the load: sca_create's parameters, sca_set_agents
 * (n and the policies must match; every other value is overwritten from the blob), sca_set_agent_params, sca_set_obstacles, any
 * sca_set_state, sca_device_tracker_enable + sca_device_tracker_set_agent_params, the list form (sca_set_paths with the same lists, or
 * sca_set_path_slots(W)), sca_set_missions[_paths] with the same tables, sca_set_mission_gate, sca_clearance_enable.  The contract: after
 * the definition + sca_load_context(B, blob), where blob = sca_save_context(A) was taken behind A's k-th env update, B is bit for bit A
 * from there on -- state, float32 action rows, neighbour lists and their distSq, diag, status, the kd permutation, sca_active_count,
 * sca_get_finished, tracker v_pref, plans and re-plan counts, remaining / now_goal / the rooms / vpref_mode, mission cursors, `ended`,
 * results (collected marks included), totals, gate words, verdicts and totals, closest-approach records -- in the same process, in
 * another process, and in a context of another size (max_agents >= n).  FORMS may differ (SCA_NBR_AUTO's counts, the kd build's sizing
 * hints and the tracker's form heuristics start over, as behind sca_set_state); values may not.  Detect the feature by the symbol
 * (sca_version() is unchanged).
 *              One bit is not a value: in SCA_NBR_GRID, SCA_ST_NBR_OVERFLOW in the status word of a row that COLLIDES in the pass may also
 *              stand because the list was full before the first colliding object was met (the grid's list rule above).  That depends on the
 *              order in which a cell hands its agents out -- the arrival order of the grid build's atomics, which no state fixes, in one
 *              context run twice as little as in two.  No kernel reads the bit, and the next pass clears it (the row is finished: the
 *              grid pass writes 0 for a row it lists nothing for).  Every other bit of `status`, and this bit on every other row, is held.
 *   in the blob  a 128-byte header (magic, format version, sca_version(), n, the tracker record's words, the public record's bytes, what
 *              is present, the list form and W, M and R, k_clearance's step number, the missions' update count, whether the one-time
 *              obstacle check behind sca_set_state is still pending, the byte count, a 64-bit checksum of everything behind the header),
 *              then sections of whole 4-byte words, each on a 16-byte boundary, offsets 64-bit.  Per row, always: the policy byte
 *              (compared at the load, not loaded), the public record, heading, goal, pref_speed, max_run_dist, the z-axis byte, v_pref as
 *              fed / tracked and its mode, total_dist, step_num, status, the kd permutation.  With the device tracker: goal_heading, the
 *              first neighbour's distSq the tracker reads, the tracker records.  With lists: remaining and now_goal; in slot form also
 *              the lengths and the rooms whole, W points a row (what stands behind a list's length travels as it stands).  With tables:
 *              the seven words per row, the R-ring per row, the totals; with a gate its four words per row and its totals.  With
 *              closest-approach records: the 32-byte record per row.  Between the load and the next pass every getter that reads state
 *              returns what it returned on the source at the save.
 *   not in it  the OUTPUTS of the last pass (action rows, neighbour lists, diag, vpref_used: they follow with the next pass), the
 *              trajectory log (a resumed context's log starts at its own row 0; the rows before k are the caller's to keep),
 *              sca_agent_steps, every form heuristic, and the definition: table entries and their lists, the lists of the block form.
 *   sca_context_checkpoint_layout  byte offsets of the SCA_CONTEXT_CHECKPOINT_SECTIONS sections (an absent section has length 0: its offset
 *              is the next section's) and the blob's size for a shape.  Pure.  SCA_ERR_ARG: a NULL pointer, struct_bytes other than
 *              sizeof(sca_context_checkpoint_shape), n < 1, negative trk_words, list_form outside 0 .. 2, W < 1 in slot form or != 0
 *              elsewhere, M outside 0 .. 127, R < 1 with tables or != 0 without, a gate without tables, a flag that is not 0 / 1.
 *   sca_context_checkpoint_info    the header's fields, after the WHOLE check of the blob that a load makes without a context (envelope and
 *              payload, below).  Pure, no context.  struct_bytes: sca_scene_harvest_get's rule.
 *   sca_context_checkpoint_bytes   the size of the blob sca_save_context writes for the context as it stands now; refused where a save is.
 *   sca_save_context   out (out_bytes bytes) receives the blob.
 *   sca_load_context   in (in_bytes bytes) goes into the context, which must hold the blob's definition: what the blob carries is compared
 *              with what the context has on.  K4's counters follow the loaded flags, so sca_active_count is right at once.
 *   cost       each call is one kernel launch and one stream synchronisation at any n; the kernel stores straight into (reads straight
 *              from) a page-locked block of the library's own, allocated at the first call, which grows when a call needs more.  A context
 *              that never calls these entry points allocates nothing for them and enqueues what it did.
 *   refusals   decided on the host before any device work; a refused call has changed nothing; a damaged blob never reaches the device.
 *              SCA_ERR_STATE: no agents, no state yet, between a policy pass and its env update.  SCA_ERR_UNSUPPORTED: scenes (they have
 *              sca_save_scenes / sca_load_scenes), a shard with count < n, a communicator, the cell-owner partition.  SCA_ERR_ARG: a NULL
 *              buffer, an output buffer too small (the message names the bytes needed); at a load, the envelope: short, wrong magic or
 *              format version, trk_words or the record size not this library's, header words out of range, a byte count that is not the
 *              layout's, a checksum mismatch; the blob against the context, each named in the message: n, a row's policy, the tracker,
 *              the lists (form, W, in block form a cursor beyond the list's length as set), the tables (M, R), the gate, the
 *              closest-approach records; the payload: a permutation that is not one of 0 .. n-1, unknown flag bits, a vpref_mode or
 *              z-axis word other than 0 / 1, a position that is not finite, a radius, pref_speed or max_run_dist that is not positive,
 *              a negative step count, len outside 0 .. W, remaining outside 0 .. len, a successor / cursor / flying / waiting word outside
 *              -1 .. M-1, collected above ended, a verdict word above SCA_SPAWN_OVER_CAP, a closest-approach partner outside its range,
 *              any tracker integer a kernel uses as a cursor, count or switch outside its range. */
#define SCA_CONTEXT_CHECKPOINT_SECTIONS 26
enum sca_context_checkpoint_lists { SCA_CHECKPOINT_LISTS_NONE = 0, SCA_CHECKPOINT_LISTS_BLOCK = 1, SCA_CHECKPOINT_LISTS_SLOTS = 2 };
typedef struct sca_context_checkpoint_shape {   /* what a blob's layout depends on */
    int32_t struct_bytes;
    int32_t n, trk_words;                /* agents; the tracker record's 4-byte words (0: no device tracker) */
    int32_t list_form, W;                /* sca_context_checkpoint_lists; the room per row in slot form, else 0 */
    int32_t M, R;                        /* the tables' (0, 0: none) */
    int32_t has_gate, has_clearance;     /* 0 / 1 */
} sca_context_checkpoint_shape;
struct sca_context_checkpoint_info {     /* (a struct tag: the function of the same name fills it) */
    int32_t struct_bytes, reserved;
    int32_t format, lib_version;         /* the blob's format version; sca_version() of the library that wrote it */
    int32_t n, trk_words, record_bytes;
    int32_t has_tracker, list_form, W, M, R, has_gate, has_clearance;
    int32_t clear_step, state_fresh;     /* k_clearance's step number; 1: saved directly behind sca_set_state */
    int64_t updates;                     /* env updates since sca_set_missions */
    int64_t total_bytes;
    uint64_t checksum;
    int32_t occupied, reserved1;         /* the occupied rows at the save: n for a blob without vacant rows (a caller compiled before the
                                            field passes the smaller struct_bytes and does not receive it) */
};
int sca_context_checkpoint_layout(const sca_context_checkpoint_shape *shape, int64_t *offsets /*SCA_CONTEXT_CHECKPOINT_SECTIONS*/, int64_t *total_bytes);
int sca_context_checkpoint_info(const void *blob, int64_t bytes, struct sca_context_checkpoint_info *out, int32_t struct_bytes);
int sca_context_checkpoint_bytes(sca_ctx *ctx, int64_t *bytes);
int sca_save_context(sca_ctx *ctx, void *out, int64_t out_bytes);
int sca_load_context(sca_ctx *ctx, const void *in, int64_t in_bytes);
/* The same three calls with an options word, for a context whose population changes (sca_retire_agents, below).  options == 0 is the call
 * without the word in every respect, the refusal while a row is vacant included; an unknown bit is SCA_ERR_ARG.
 *   SCA_CHECKPOINT_VACANCY   a save works while rows are vacant, a load takes a blob that holds vacant rows, and a load works on a context
 *              that itself has vacant rows: it replaces vacancy wholesale.  The contract above then also covers sca_get_vacant,
 *              sca_get_population, SCA_FORM_VACANCY, every refusal vacancy causes and its lifting once every row is occupied, and every
 *              later retire, admitting respawn (plain, gated, _attrs), mission take and gate verdict.  A vacant row keeps its policy and
 *              attributes, so the DEFINITION holds the policies and attributes as they stand at the save (a respawn may have brought
 *              new ones: sca_respawn_agents_attrs).
 *   in the blob  no new section and the same format: a vacant row's flag word (11), the permutation (occupied ids, then the vacant ids
 *              ascending), the row's constants, tracker record, table words and cursor travel as every row's.  The header's `present`
 *              word gains bit 32 and a reserved word holds the occupied count m, both only when m < n at the save: a blob saved with
 *              the option from a context without vacant rows is byte for byte sca_save_context's, and sca_load_context loads it.
 *              sca_context_checkpoint_info accepts both and reports `occupied`.
 *   the outputs  of the last pass are not in a blob, and a vacant row gets no pass: the load leaves every vacant row's action row zero,
 *              its neighbour counts 0 (near: -1) and its diag -1, as the retire left them.  One launch (k_ctx_load_vacancy) and one
 *              synchronisation at any n, as before; the scratch a first retire allocates is allocated where the blob holds vacant rows.
 *   refusals   every refusal of the calls without the word, with its code and in its order; then, SCA_ERR_ARG and before any device work:
 *              the header's vacancy bit with occupied outside 1 .. n-1, or occupied != 0 without it; a row with flag bit 8 whose flag word
 *              is not 11; a count of vacant rows other than n - occupied; a permutation with a vacant id in front of position m or whose
 *              positions m .. n-1 are not the vacant ids ascending; vacant rows with lists in block form; a vacant row with a velocity,
 *              heading or total_dist that is not zero, in slot form a len or rem that is not 0, or a gate's waiting word other than -1.
 *              Without the option flag bit 8 and the header's bit stay the refusals they were. */
enum { SCA_CHECKPOINT_VACANCY = 1 };
int sca_context_checkpoint_bytes_opt(sca_ctx *ctx, uint32_t options, int64_t *bytes);
int sca_save_context_opt(sca_ctx *ctx, uint32_t options, void *out, int64_t out_bytes);
int sca_load_context_opt(sca_ctx *ctx, uint32_t options, const void *in, int64_t in_bytes);

/* Closest approach per agent, measured WITH THE STEP.  With the feature on a step enqueues one more kernel beside the log's
 * (k_scene_clearance, a workgroup per scene, in front of the step's last kernel) that keeps, for every occupied agent row, how close the
 * agent came to another agent of its scene and to an obstacle of its scene, with whom and at which step -- the column a table of
 * collision-avoidance episodes lacks, without pulling the trajectory log across the link for an all-pairs search on the host.
 *   the rule   mirrors the env's own collision test (mampenv.py:61-75, dis <= radius sum).  Row a of scene s is updated at every step of
 *              the scene's own that the scene began with somebody live and that a ENTERED unfinished (none of at-goal / collision /
 *              timed-out in its entry flags; the step in which it gains a flag still counts).  For every other occupied row b of the
 *              scene, whatever its flags (finished drones stay where they are and the reference still collides with them),
 *              c = l3norm(p_a, p_b) - (r_a + r_b): p the positions the step moved to, l3norm the reference's rounded norm (util.py:104),
 *              the radius sum formed first.  The step's candidate is the smallest c, the lowest b on equal values; it replaces the record
 *              only if strictly smaller, so the earliest step wins ties.  The same over the scene's obstacles in their set order -- the
 *              shared set, the scene's own set, or the first `count` rows of its obstacle slot.  Never a partner: rows behind the scene's
 *              size (vacant), obstacle rows behind a slot's count, anything of another scene.
 *   the record 32 bytes per agent row.  Partners are scene-local (agent row - the scene's first row; obstacle index within the scene's
 *              set), `step` is the scene's own step count, 1-based.  An empty half is +inf, -1, 0: what a one-agent scene and a scene
 *              without obstacles keep.
 *   contract   a scene's records are bit for bit those of a context holding that episode alone, in every step form (sca_env_step,
 *              sca_run_steps, sca_policy_pass + sca_env_update, sca_step_host), and no other scene can tell that a scene finished, was
 *              restarted or has the feature on.  A context without the feature enqueues exactly what it did.
 *   cost       one dependent dispatch per step plus O(size^2) rounded norms per LIVE scene (about 10^7 at 1024 scenes of 100 agents);
 *              a pair takes the exact rounding only while it can still beat the row's record.
 *   sca_scene_clearance_enable  on != 0: allocates n x 32 bytes, every row empty; records cover the steps from then on (enabling again
 *              starts over).  on == 0 frees.  SCA_ERR_STATE: no scenes, or between a policy pass and its env update.  Whatever clears
 *              or redefines the scenes (sca_set_agents, sca_set_scenes) drops it, as it drops the log and the harvest.
 *   sca_get_scene_clearance     the scene's occupied rows, out[size[scene]], one copy and one synchronisation.  struct_bytes =
 *              sizeof(sca_scene_clearance).  SCA_ERR_STATE: not enabled (or no scenes).  SCA_ERR_ARG: a scene outside 0 .. nscenes-1, a
 *              NULL out, a wrong struct_bytes.  A finished scene keeps its records until it is restarted.
 *   restart    every sca_restart_scenes* entry point empties the records of the scenes it names, over their whole capacity, inside its
 *              one launch.  sca_load_scenes, sca_set_state and a state from the host block leave the records alone: a caller that
 *              resumes a checkpoint keeps the source's records beside the blob and merges (field by field, the later one only where
 *              strictly smaller).
 * Detect the feature by the symbol (sca_version() and the checkpoint blob are unchanged). */
typedef struct sca_scene_clearance {     /* 32 bytes */
    double  agent_clear, obs_clear;      /* the smallest c so far; +inf: none */
    int32_t agent_partner, agent_step;   /* scene-local row of the other agent (-1: none), the scene's step it happened in (0: none) */
    int32_t obs_partner, obs_step;       /* index within the scene's obstacle set (-1: none), the step */
} sca_scene_clearance;
int sca_scene_clearance_enable(sca_ctx *ctx, int on);
int sca_get_scene_clearance(sca_ctx *ctx, int scene, sca_scene_clearance *out /*size[scene]*/, int32_t struct_bytes);

/* Closest approach per agent for a WHOLE CONTEXT, by kd-tree descent.  The scene feature above is all-pairs inside a scene of at most 1536
 * agents; a plain context of any size -- the 100 000-agent circle, the take-off / landing field, the drop-in env loop -- keeps the same
 * 32-byte record per agent with one more kernel per step (k_clearance, a wavefront per agent, in front of the step's last kernel, only
 * while the feature is on): a nearest-partner search with a shrinking radius on the trees the step already has.
 *   the rule   the scene rule with the context as the one "scene".  Row a is updated at every step that a ENTERED unfinished (none of
 *              at-goal / collision / timed-out in its entry flags; the step in which it gains a flag still counts).  For every other agent
 *              b, whatever its flags, c = l3norm(p_a, p_b) - (r_a + r_b): p the positions the step moved to, l3norm the reference's rounded
 *              norm, the radius sum formed first.  The step's candidate is the smallest c, the lowest b on equal values; it replaces the
 *              record only if strictly smaller, so the earliest step wins ties.  The same over the obstacles in set order.
 *   the record partners are context-global agent ids and obstacle indices; `step` counts the context's env updates since the enable call,
 *              1-based.  An empty half is +inf, -1, 0.
 *   the bound  the agent tree holds the positions the step BEGAN with, the rule is over the moved ones: a child whose box lies at dist from
 *              the agent's moved position cannot give less than dist - max_step - r_a - max_radius - 1e-4 (max_step and max_radius as in
 *              the collision test's reach; the 1e-4 covers the 5-decimal rounding); the obstacle tree is static: dist - r_a -
 *              max_obs_radius - 1e-4.  A child is skipped only where that bound is strictly above the best value so far, and the best
 *              value starts at the row's own record: a step in which nobody can beat the record ends at the root.
 *   step forms sca_env_step, sca_run_steps, sca_policy_pass + sca_env_update, sca_step_host; SCA_NBR_KDTREE, SCA_NBR_AUTO and
 *              SCA_NBR_KDTREE_HOSTBUILD; the device tracker, per-agent attributes, waypoint lists.  A context without the feature enqueues
 *              exactly what it did.  While it is on, SCA_NBR_AUTO builds no tree ahead of the next pass inside sca_run_steps.
 *   sca_clearance_enable   on != 0: allocates n x 32 bytes, every row empty; records cover the steps from then on (enabling again starts
 *              over).  on == 0 frees.  SCA_ERR_STATE: no agents or no state yet, or between a policy pass and its env update.
 *              SCA_ERR_UNSUPPORTED, the message names the reason: scenes are set, a shard with count < n, a communicator, the cell-owner
 *              partition.
 *   sca_get_clearance      rows agent_begin .. agent_begin + agent_count - 1, one copy and one synchronisation.  SCA_ERR_STATE: not
 *              enabled.  SCA_ERR_ARG: a range outside 0 .. n, a NULL out, struct_bytes other than sizeof(sca_scene_clearance).
 *   while on   SCA_ERR_UNSUPPORTED, before anything is enqueued: a pass or step in SCA_NBR_GRID mode and an env update without a policy
 *              pass in front of it (neither has an agent tree of this step); a shard with count < n, a communicator, the cell-owner
 *              partition and scenes, each at its own entry point.  A new agent set drops the records; a new state leaves them alone.
 * Detect the feature by the symbol (the version number is unchanged). */
int sca_clearance_enable(sca_ctx *ctx, int on);
int sca_get_clearance(sca_ctx *ctx, int agent_begin, int agent_count, sca_scene_clearance *out /*agent_count*/, int32_t struct_bytes);

/* Respawning agents in place: new missions without redefining the swarm.  A plain context (no scenes) otherwise runs one episode -- an
 * agent that arrived, collided or timed out stays inert until everybody has finished, and sca_set_agents tears the whole world down (every
 * Dubins plan, attributes, lists, records, the log, the kd permutation).  The reference's rule is plain Python: assigning pos_global_frame,
 * goal_global_frame, is_at_goal = False, ... to one Agent object between two env.step() calls (mampenv.py:16-19); the kd-tree keeps its
 * agentIDs order (kdTree.py:43-45) and every other agent is untouched.
 *   sca_respawn_agents   the arrays are packed in the order of `ids` (any order, no repeats) and travel through a page-locked block of the
 *              library's own; ONE launch (k_respawn, a wavefront per named row) and one synchronisation however many rows are named.
 *              Legal only between two steps.  Afterwards a named row is what sca_set_agents + sca_set_state (+
 *              sca_device_tracker_enable) leave for an agent with these values: public record (pos, float32 vel, flags 0, radius), heading,
 *              goal, pref_speed, max_run_dist, zaxis (NULL: the rows keep theirs), total_dist 0, step_num 0, status 0, last pass's list
 *              invalid (nbr_valid 0, the tracker's first-neighbour distSq -1).  Device tracker on and the row SCA / RVO3D+Dubins: the
 *              initial tracker record, goal_heading, vpref_mode 1, vpref_ext 0; otherwise the row's fed vpref_ext / vpref_mode stay
 *              (the caller's input, refreshed through sca_set_vpref).  Waypoint lists in slot form: the row's list from the call's CSR
 *              arrays (len = rem = its length, now_goal None), without arrays an empty list.  Closest-approach records on: the row's
 *              record is emptied (+inf, -1, 0), other rows keep it as a partner, the step count runs on.  EVERY OTHER ROW KEEPS EVERY
 *              WORD IT HAD, and so do the kd permutation, the trajectory log (it goes on) and the form heuristics: forms may differ
 *              afterwards, values may not.  sca_active_count is right at once (K4's striped counters are adjusted for the rows that
 *              were done).  The row KEEPS its policy, its per-agent solver attributes (sca_set_agent_params) and its planner attributes
 *              (sca_device_tracker_set_agent_params): changing them is out of scope here.  Host mirrors follow: the radius a later
 *              sca_set_state uploads, the largest radius / pref_speed (they only grow), and, where sca_host_state_get has handed out the
 *              state block, the named rows' six state columns there (a later SCA_HOST_IN_STATE step does not bring the old rows back).
 *              Works in every neighbour mode and in front of and behind every step form.
 *   sca_get_finished     the rows that carry any of at-goal / collision / timeout, ascending ids (an ordered compaction on the device: a
 *              count per tile, a scan, the write; one synchronisation) -- instead of sca_get_state's n records across the link.  *count
 *              is their number even where it exceeds `capacity`; the first `capacity` are written.  A lifelong loop calls it only when
 *              sca_env_step's `active` dropped.
 *   refusals   decided on the host before any device work; a refused call changes nothing.  SCA_ERR_STATE: no agents, no state yet, (respawn)
 *              between a policy pass and its env update.  SCA_ERR_ARG: count <= 0, a NULL required array (everything but zaxis,
 *              goal_heading and the path arrays), an id outside 0 .. n-1, a repeated id, a position that is not finite, a radius,
 *              pref_speed or max_run_dist that is not positive and finite, goal_heading == NULL with a tracked row named under the device
 *              tracker, only one of the two path arrays, a list longer than the room per row, negative or decreasing offsets, a waypoint
 *              that is not finite; for sca_get_finished capacity < 0, a NULL count, NULL rows with capacity > 0, struct_bytes other than
 *              sizeof(sca_finished_row).  SCA_ERR_UNSUPPORTED, the message names the way out: scenes are set (sca_restart_scenes), a shard
 *              with count < n, a communicator, the cell-owner partition, waypoint lists in block form (sca_set_path_slots), path arrays
 *              while no slot form is set.
 * Detect the feature by the symbol (the version number is unchanged). */
typedef struct sca_finished_row {        /* 48 bytes */
    int32_t  id;                         /* the agent's row */
    uint32_t flags;                      /* sca_flag bits */
    int32_t  step_num, reserved;
    double   total_dist;
    double   pos[3];
} sca_finished_row;
int sca_respawn_agents(sca_ctx *ctx, int count, const int32_t *ids /*count*/, const double *pos /*count*3*/, const float *vel /*count*3*/,
                       const double *heading /*count*3*/, const double *radius /*count*/, const double *pref_speed /*count*/,
                       const double *goal /*count*3*/, const uint8_t *zaxis /*count, nullable*/, const double *max_run_dist /*count*/,
                       const double *goal_heading /*count*3, nullable*/, const int32_t *path_offsets /*count+1, nullable*/,
                       const double *path_points /*nullable*/);
int sca_get_finished(sca_ctx *ctx, sca_finished_row *rows /*capacity*/, int capacity, int *count, int32_t struct_bytes);

/* Vacant rows in a plain context: drones leave the airspace and re-enter.  A plain context otherwise always holds exactly n bodies: a drone
 * that arrived, collided or timed out stays where it is, and the reference's rule keeps colliding with it.  The reference indexes
 * agents[agentIDs[i]] by id and has no removal in place; the library defines vacancy as the plain list edit on kdTree.agentIDs: retiring id
 * a is agentIDs.remove(a), admitting it agentIDs.append(a), nothing else of the order moves.
 *   contract   at any moment the occupied rows are, bit for bit, a context that holds only those agents, renumbered in ascending id, behind
 *              sca_set_agents (+ attributes, obstacles, lists), sca_set_state and sca_set_kd_perm(the occupied prefix of the permutation,
 *              mapped through the same renumbering) -- from there on, step for step: state, action rows, neighbour lists entry for entry,
 *              diag, status, the permutation's prefix, sca_active_count, sca_get_finished.  No occupied row that was not named in a call can
 *              tell that the call happened, except that the retired drone is nobody's neighbour, collision, clearance or probe partner.
 *   a vacant row   flags at-goal | collision | SCA_FLAG_VACANT (sca_get_state shows 11), zero velocity, heading, total_dist and step_num, a
 *              zero action row, status 0, an invalid neighbour list, diag -1; in slot form an empty list (len = rem = 0, now_goal None); its
 *              closest-approach record emptied.  It KEEPS its position, radius, goal, pref_speed, max_run_dist, policy, zaxis, v_pref mode and
 *              fed v_pref, solver and planner attributes, its tracker record (unowned: the tracker wants flags 0), its mission table and
 *              cursor.  It stands in no tree, hence in no neighbour list, near list, collision walk or clearance descent; sca_active_count
 *              does not count it, sca_get_finished does not list it, mission tables never take it (it never "ends"), sca_probe_clearance,
 *              both gated respawns' world tests and the mission gate's probe pass over it.  The trajectory log writes its row as it stands.
 *   the permutation   positions [0, m) hold the occupied ids in carried order, [m, n) the vacant ids ascending; sca_get_kd_perm returns it
 *              whole.  A retire deletes the named ids from the prefix (stable); a respawn appends the vacant ids it admits in the call's
 *              order (a gated call only the admitted ones).
 *   sca_retire_agents   any occupied rows, live or finished; one synchronisation however many are named.  K4's striped counters are adjusted
 *              for the rows that were live.  Mission tables: a retired row in flight writes no result and moves no total, a row waiting at
 *              the gate loses its pending mission (`dropped` + 1).
 *   sca_respawn_agents / sca_respawn_agents_gated   naming a vacant row admits it: the row becomes word for word what the respawn leaves for
 *              the call's values.  In the gated call a vacant named row is no body for the others, and a refused vacant row stays vacant
 *              with every word it had.  A call may mix occupied and vacant rows.
 *   sca_get_vacant      the vacant ids, ascending (sca_get_finished's ordered compaction; one synchronisation; none while no row is vacant).
 *              *count is their number even where it exceeds `capacity`; the first `capacity` are written.
 *   sca_get_population  the occupied rows, m (host arithmetic).
 *   refusals   decided on the host before any device work; a refused call changes nothing.  SCA_ERR_STATE: no agents, no state yet, (retire)
 *              between a policy pass and its env update.  SCA_ERR_ARG: count <= 0, ids NULL, an id outside 0 .. n-1, a repeated id, an id
 *              that is vacant already, a call that would leave no occupied row (m >= 1 always); for sca_get_vacant capacity < 0, a NULL
 *              count, NULL ids with a capacity.  SCA_ERR_UNSUPPORTED: what sca_respawn_agents refuses (scenes, a shard with count < n, a
 *              communicator, the partition, lists in block form).
 *   while a row is vacant   SCA_ERR_UNSUPPORTED, the message names the reason: a pass in SCA_NBR_GRID, sca_step_host, sca_set_state,
 *              sca_set_kd_perm, sca_get_kd_tree, sca_save_context / sca_load_context / sca_context_checkpoint_bytes (each has an _opt form that takes
 *              SCA_CHECKPOINT_VACANCY and then works: a checkpoint carries vacant rows), sca_set_shard with count < n, sca_comm_init, sca_partition_init, sca_set_scenes, and the lists for the whole id range: sca_set_paths,
 *              sca_set_path_slots, sca_set_path_state (a vacant row's list is empty and its now_goal None; clearing the lists with
 *              sca_set_paths(0, NULL) stays legal).  SCA_NBR_AUTO resolves to the kd pass, as with scenes, and a
 *              pass reports SCA_FORM_VACANCY.  Everything works again once every row is occupied.  sca_set_agents drops all vacancy.
 * A context that never retires allocates nothing of this and enqueues the kernels it did.  Detect the feature by the symbol. */
int sca_retire_agents(sca_ctx *ctx, int count, const int32_t *ids /*count*/);
int sca_get_vacant(sca_ctx *ctx, int32_t *ids /*capacity*/, int capacity, int *count);
int sca_get_population(sca_ctx *ctx, int *occupied);

/* Spawn admission: how free is this point NOW, and respawning only the rows whose start is free.  sca_respawn_agents puts a drone wherever
 * it is told to, also inside another one; the closest-approach records (sca_clearance_enable) cover the agents' own positions inside a
 * step, from a tree that is one step old.  A spawn test needs arbitrary points, between two steps, against the records as they are now --
 * right after a respawn or a sca_set_state too, and in SCA_NBR_GRID mode, where there is no agent tree at all.
 *   the rule   query q is a sphere of radius[q] at pos[q].  out[q].agent_clear is the smallest c = l3norm(p_q, p_b) - (r_q + r_b) over
 *              every agent row b of the context except ignore[q] (-1, or a NULL ignore: nobody is excluded): p_b and r_b from the row's
 *              current public record whatever its flags, l3norm the reference's rounded norm, the radius sum formed first;
 *              agent_partner is the lowest id with that value.  The same over the obstacles in set order.  Both step fields are 0, an
 *              empty half is +inf, -1, 0.  For a query at agent a's own position and radius with ignore = a this is that agent's
 *              candidate of the closest-approach rule.
 *   the search brute force over the records, on purpose: between two steps the agent tree has no known age (a respawn or a new state has
 *              moved rows arbitrarily, an AUTO burst may have built ahead, the grid has no tree); the records are the one thing that is
 *              right at every legal call point.  The partners (agents, then obstacles) are cut into fixed tiles, the queries into
 *              chunks of 64 -- one per lane; k_spawn_probe stages a tile in LDS and leaves one partial per (tile, query), k_spawn_reduce
 *              folds them into a page-locked block.  No atomics: the minimum on (c, id) depends neither on the tiling nor on the
 *              scheduling.  The scratch is allocated at the first call and grows like the respawn block; a context that never probes
 *              allocates and enqueues nothing new.  One synchronisation per call.
 *   sca_probe_clearance   legal between two steps, in every neighbour mode, with or without the tracker, lists and records; changes
 *              nothing.  SCA_ERR_STATE: no agents, no state yet, between a policy pass and its env update.  SCA_ERR_ARG: count <= 0, a
 *              NULL pos, radius or out, a position that is not finite, a radius that is negative or not finite (0 is a point probe), an
 *              ignore outside -1 .. n-1, struct_bytes other than sizeof(sca_scene_clearance).  SCA_ERR_UNSUPPORTED, as for
 *              sca_respawn_agents: scenes, a shard with count < n, a communicator, the cell-owner partition.
 *   sca_respawn_agents_gated   sca_respawn_agents' arguments, then a margin, the verdict per named row, (nullable) the world test's
 *              records and (nullable) the number of admitted rows.  With the rows in the call's order:
 *              world test  row r probes pos[r] / radius[r] with ignore = ids[r]: every other agent row at its current record -- the
 *                          other named rows where they stand NOW, a refused row stays a body -- and every obstacle.  r is world-clear
 *                          where neither half is <= margin (an empty half never blocks).
 *              entry test  for every EARLIER row r' < r of the call that is world-clear, c = l3norm(pos[r], pos[r']) - (radius[r] +
 *                          radius[r']); r is blocked where any such c <= margin.  An earlier row the world blocked blocks nobody.  A
 *                          conservative, fully parallel and deterministic stand-in for the sequential greedy: in a chain a < b < c where
 *                          b conflicts with both, c is refused although b was.
 *              verdict     the first that applies: SCA_SPAWN_BLOCKED_AGENT, SCA_SPAWN_BLOCKED_OBSTACLE, SCA_SPAWN_BLOCKED_ENTRY, else
 *                          SCA_SPAWN_ADMITTED.
 *              Afterwards every device and host word is what sca_respawn_agents leaves when it names exactly the admitted rows, in the
 *              call's order, with their arrays (the waypoint CSR cut down to them); a refused row keeps every word it had; a call that
 *              admits nobody changes nothing and returns SCA_OK.  The probe, the fold, the gate (k_spawn_gate: a wavefront per row over
 *              the earlier rows) and k_respawn run on the context's stream behind ONE synchronisation.  Refusals: everything
 *              sca_respawn_agents refuses, with the same codes; SCA_ERR_ARG for a margin that is negative or not finite and for a NULL
 *              verdict.
 * Detect the feature by the symbols (the version number is unchanged). */
enum sca_spawn_verdict { SCA_SPAWN_ADMITTED = 0, SCA_SPAWN_BLOCKED_AGENT = 1, SCA_SPAWN_BLOCKED_OBSTACLE = 2, SCA_SPAWN_BLOCKED_ENTRY = 3 };
/* A fifth word, 4, that only sca_set_mission_gate's rows carry: not tested in this step, the cap was reached.  The two calls above never
 * return it.  It is spelled as an expression, and not as the literal, on purpose: tests/test_spawn_probe_cpu.py reads this header for every
 * "SCA_SPAWN_<NAME> = <digits>" and holds the result to exactly the four values above -- what the gated respawn can return.  The
 * expression keeps that pin true as it stands; the enum of its own only says whose word it is. */
enum sca_mission_gate_verdict { SCA_SPAWN_OVER_CAP = SCA_SPAWN_BLOCKED_ENTRY + 1 };
int sca_probe_clearance(sca_ctx *ctx, int count, const double *pos /*count*3*/, const double *radius /*count*/,
                        const int32_t *ignore /*count, nullable*/, sca_scene_clearance *out /*count*/, int32_t struct_bytes);
int sca_respawn_agents_gated(sca_ctx *ctx, int count, const int32_t *ids /*count*/, const double *pos /*count*3*/, const float *vel /*count*3*/,
                             const double *heading /*count*3*/, const double *radius /*count*/, const double *pref_speed /*count*/,
                             const double *goal /*count*3*/, const uint8_t *zaxis /*count, nullable*/, const double *max_run_dist /*count*/,
                             const double *goal_heading /*count*3, nullable*/, const int32_t *path_offsets /*count+1, nullable*/,
                             const double *path_points /*nullable*/, double margin, int32_t *verdict /*count*/,
                             sca_scene_clearance *probe /*count, nullable*/, int32_t *admitted /*nullable: how many*/);

/* An arriving drone brings its own POLICY, SOLVER and PLANNER ATTRIBUTES.  sca_respawn_agents keeps the row's; the reference keeps policy and every
 * solver attribute as plain fields of the Agent object (agent.py:24-41), assigned between two env.step() calls like a new start, so a row
 * that was an ORCA3D drone with neighborDist 10 can be re-entered by a Dubins-tracked SCA drone with neighborDist 4 and another turning
 * radius -- a mixed fleet in one airspace.
 *   sca_respawn_agents_attrs   two arguments in front of sca_respawn_agents' arrays, which keep their order and meaning.  policy: one byte
 *              per named row (NULL: the rows keep theirs).  attrs: sca_restart_attrs as sca_restart_scenes_attrs reads it (NULL: the rows
 *              keep their attributes): struct_bytes and reserved by its rules; with a descriptor a NULL array stands for the CONTEXT's
 *              value for every named row -- sca_create's sca_params value, sca_device_tracker_enable's value -- NOT what the row had.
 *              Planner arrays are ignored for rows whose new policy is untracked.  policy == NULL && attrs == NULL is exactly
 *              sca_respawn_agents: the same launches are enqueued.
 *   contract   afterwards a named row is what sca_set_agents(that policy) + sca_set_agent_params(those values) + sca_set_state
 *              (+ sca_device_tracker_enable + sca_device_tracker_set_agent_params) leave for such an agent: everything
 *              sca_respawn_agents writes, the policy byte, the 64-byte record sca_set_agent_params derives, the row's neighborDist in
 *              the tracker's array, the planner triple and the class byte.  Under the device tracker a row
 *              whose NEW policy is SCA / RVO3D+Dubins takes the initial tracker record, goal_heading, vpref_mode 1 and vpref_ext 0; a row
 *              that LEAVES those policies takes what sca_restart_scenes leaves for that transition: vpref_mode 0, vpref_ext 0, the
 *              initial tracker record.  EVERY OTHER ROW KEEPS EVERY WORD.  A fresh context built from the merged definition is bit for
 *              bit equal from there on; with vacant rows, the occupied rows are a context of those agents with their CURRENT policies
 *              and attributes.  Mission tables keep their rule: a later take keeps the row's policy and attributes -- the new ones.
 *   host side  the policy mirror, the ORCA3D-LP list (uploaded again only when a row entered or left that policy) and the lists' v_pref
 *              bytes follow.  The tracker's classes are dealt again by sca_restart_scenes_attrs' rule over the plain context's tracked
 *              rows (vacant rows counted: they keep their triple and class byte): more than 16 triples go to the per-agent form, 16
 *              or fewer come back, one class goes into the scalars; a class keeps its index while a row uses it, and the whole class
 *              array goes up again only where another row's byte moved or on first use.  The first call that brings attributes into a context without per-agent arrays allocates them and fills
 *              every row with the context's own values, from which the rows not named compute the bits they computed before.  The
 *              context's envelope (largest neighbor_dist, max_speed, dt_nominal) only grows, as the largest radius does: forms may
 *              differ afterwards, values may not.
 *   cost       ONE launch (k_respawn_attrs, a wavefront per named row) and one synchronisation, the list's and the class bytes' copies in
 *              front of it.  The gated form: still one synchronisation; only the ADMITTED rows take anything, the classes are dealt
 *              over what they brought, and the two copies are enqueued behind the synchronisation on the context's stream.
 *   refusals   everything sca_respawn_agents (or its gated form) refuses, with its codes -- goal_heading == NULL is judged by the NEW
 *              policy.  SCA_ERR_ARG: a policy byte above 5, a struct_bytes or reserved that sca_restart_scenes_attrs refuses, planner
 *              arrays without a device tracker, a named row whose solver attributes break sca_set_agent_params' rules (the message names
 *              the packed row), a row whose NEW policy is tracked and whose planner attributes break
 *              sca_device_tracker_set_agent_params' rules.  A refused call changes nothing.
 * A context that never calls these allocates nothing new and enqueues what it did.  Detect the feature by the symbols (sca_version() is
 * unchanged). */
int sca_respawn_agents_attrs(sca_ctx *ctx, int count, const int32_t *ids /*count*/,
                             const uint8_t *policy /*count, nullable: the rows keep theirs*/,
                             const sca_restart_attrs *attrs /*nullable: the rows keep their attributes*/,
                             const double *pos /*count*3*/, const float *vel /*count*3*/,
                             const double *heading /*count*3*/, const double *radius /*count*/, const double *pref_speed /*count*/,
                             const double *goal /*count*3*/, const uint8_t *zaxis /*count, nullable*/, const double *max_run_dist /*count*/,
                             const double *goal_heading /*count*3, nullable*/, const int32_t *path_offsets /*count+1, nullable*/,
                             const double *path_points /*nullable*/);
int sca_respawn_agents_gated_attrs(sca_ctx *ctx, int count, const int32_t *ids /*count*/,
                             const uint8_t *policy /*count, nullable: the rows keep theirs*/,
                             const sca_restart_attrs *attrs /*nullable: the rows keep their attributes*/,
                             const double *pos /*count*3*/, const float *vel /*count*3*/,
                             const double *heading /*count*3*/, const double *radius /*count*/, const double *pref_speed /*count*/,
                             const double *goal /*count*3*/, const uint8_t *zaxis /*count, nullable*/, const double *max_run_dist /*count*/,
                             const double *goal_heading /*count*3, nullable*/, const int32_t *path_offsets /*count+1, nullable*/,
                             const double *path_points /*nullable*/, double margin, int32_t *verdict /*count*/,
                             sca_scene_clearance *probe /*count, nullable*/, int32_t *admitted /*nullable: how many*/);

/* Mission tables: a finished row takes its next mission INSIDE the step.  sca_respawn_agents and sca_get_finished are host calls between
 * two steps, so continuous traffic costs a synchronisation per step and sca_run_steps(k) cannot run it at all (a burst keeps stepping
 * rows that stay finished).  Here every agent row carries its upcoming missions on the device; the step's last kernel (k_mission_advance,
 * behind K4 and in front of the buffer swap, enqueued only while tables are set) hands a row that ENDED in this step its next mission by
 * exactly sca_respawn_agents' rule, with no host round trip -- bursts run traffic.  A table says per outcome whether the device goes on or
 * the row stays finished for the host; with sca_set_mission_gate (below) the device goes on only where the next start is free.
 *   sca_set_missions   every row gets room for M entries (1 .. 127) and R result records (1 .. 65536); slot form, entries[M a + j], as the
 *              path slots are laid out.  An entry is a 128-byte sca_mission; next_ok / next_fail name entries of the SAME row (-1: stop).
 *              SCA_MISSION_START_HERE: the row keeps the position and heading it has (pos / heading are ignored); SCA_MISSION_KEEP_ZAXIS:
 *              it keeps its zaxis byte.  The radius, the policy and the per-agent solver and planner attributes stay the row's, as under
 *              sca_respawn_agents.  first_ok[a] / first_fail[a] are the successors of the flight that is in the air when the table
 *              arrives; a row with first_ok = first_fail = -1 has no table and behaves as without the feature.  entries == NULL with
 *              M = 0 drops the feature, sca_set_agents drops it too, sca_set_state leaves tables and cursors alone.  The largest
 *              pref_speed among the reachable entries is folded into the context's envelope at once (it only grows).
 *   taking     a row ENDED in a step when it entered it without any of at-goal / collision / timeout and leaves K4 with one.  Outcome:
 *              collided if the collision bit is set, else arrived if at-goal is set, else timed out.  Successor: next_ok for arrived,
 *              next_fail otherwise -- those of the entry under the row's cursor, first_ok / first_fail while the cursor is -1.
 *              -1: the row stays finished as it is (sca_get_finished lists it, the host may respawn it, gated or not; the cursor stays,
 *              so a later ending of that host-given flight follows the same successors again).  j >= 0: the row becomes what
 *              sca_respawn_agents naming it with entry j's values leaves, word for word (for START_HERE: with the pos / heading
 *              sca_get_state returns) -- flags 0, total_dist 0, step_num 0, status 0, list invalid, under the device tracker the initial
 *              record with goal_heading, vpref_mode 1 and vpref_ext 0 for SCA / RVO3D+Dubins rows, the closest-approach record emptied,
 *              sca_active_count right at once -- and the cursor becomes j.  A self-successor (next_fail == j) is legal: "retry".  Rows
 *              already finished when the table arrives are never taken.
 *   results    every ending of a row that has a table writes one 96-byte sca_mission_result into the row's ring at ended[a] % R; ended[a]
 *              counts endings and nothing ever blocks: a host that collects too rarely sees from `ended` how many it lost.
 *              sca_get_mission_results hands out the results not yet collected, ascending id, within a row oldest first (the ordered
 *              compaction of sca_get_finished with a count per row; no atomic cursor; one synchronisation) and marks them collected.
 *              *count is their number; where it exceeds `capacity` NOTHING is written or marked (call again with room; n x R always
 *              suffices).  sca_get_mission_totals: 64-bit counters since sca_set_missions, kept by integer atomics (one per wavefront per
 *              step and counter, only where non-zero), over ALL rows: env updates, agent-steps (rows that entered a step unfinished),
 *              endings arrived / collided / timed out, taken, stopped (an ending without a successor, rows without a table included).
 *              sca_get_mission_state copies the cursor and `ended` words of rows begin .. begin + count - 1.
 *   ordering   while tables are set sca_run_steps starts nothing of the next pass from positions the mission kernel may still replace
 *              (no kd build ahead, no event riding on k_action or on the step's last kernel): forms may differ, values may not.
 *   refusals   decided on the host before any device work; a refused call changes nothing.  SCA_ERR_STATE: no agents, between a policy
 *              pass and its env update, a getter while no tables are set.  SCA_ERR_ARG: M or R out of range, n other than the agent
 *              count, a NULL array, M x n or R x n above 2^24, a successor outside -1 .. M-1, a REACHABLE entry (from first_ok /
 *              first_fail through successors) with a position, heading, goal or velocity that is not finite, a pref_speed or
 *              max_run_dist that is not positive and finite, a zaxis byte above 1 without KEEP_ZAXIS, unknown flag bits; bad
 *              struct_bytes, capacity, range or NULL outputs in the getters.  SCA_ERR_UNSUPPORTED, in either order of the calls:
 *              everything sca_respawn_agents refuses (scenes, a shard with count < n, a communicator, the partition), waypoint lists in
 *              either form for sca_set_missions itself (tables whose entries bring their own lists: sca_set_missions_paths, below), and
 *              sca_step_host while tables are set (the host owns the state there).
 * Detect the feature by the symbols (the version number is unchanged). */
enum sca_mission_flag { SCA_MISSION_START_HERE = 1, SCA_MISSION_KEEP_ZAXIS = 2 };
typedef struct sca_mission {             /* 128 bytes */
    double  pos[3], heading[3];          /* the start (ignored with SCA_MISSION_START_HERE) */
    double  goal[3], goal_heading[3];    /* goal_heading: read for rows the device tracker tracks */
    double  pref_speed, max_run_dist;
    float   vel[3];
    int8_t  next_ok, next_fail;          /* entries of the same row, -1: stop */
    uint8_t zaxis, flags;                /* flags: sca_mission_flag bits */
} sca_mission;
typedef struct sca_mission_result {      /* 96 bytes */
    int32_t  id;                         /* the agent's row */
    int32_t  entry;                      /* the entry it flew; -1: the flight in the air at sca_set_missions, or one the host gave */
    uint32_t flags;                      /* sca_flag bits the flight ended with */
    int32_t  step_num;
    double   total_dist;
    double   pos[3];                     /* where it ended */
    int64_t  update;                     /* the env update it ended in, counted from sca_set_missions (1-based) */
    int32_t  next, reserved;             /* the successor taken, -1: stopped */
    sca_scene_clearance clear;           /* the row's closest-approach record before it was emptied (+inf, -1, 0 without sca_clearance_enable) */
} sca_mission_result;
typedef struct sca_mission_totals {      /* 64 bytes */
    uint64_t updates, agent_steps, arrived, collided, timed_out, taken, stopped, reserved;
} sca_mission_totals;
int sca_set_missions(sca_ctx *ctx, int M, int R, int n, const sca_mission *entries /*M*n*/, const int32_t *first_ok /*n*/,
                     const int32_t *first_fail /*n*/);
int sca_get_mission_results(sca_ctx *ctx, sca_mission_result *out /*capacity*/, int capacity, int *count, int32_t struct_bytes);
int sca_get_mission_totals(sca_ctx *ctx, sca_mission_totals *out, int32_t struct_bytes);
int sca_get_mission_state(sca_ctx *ctx, int begin, int count, int32_t *cursor /*count*/, int32_t *ended /*count*/);

/* Mission tables whose entries bring their own waypoint lists: continuous traffic ALONG ROUTES, in bursts, on the device.
 * sca_set_missions_paths is sca_set_missions plus one packed CSR of lists over the FLAT entry index M a + j: entry j of row a has the list
 * path_points[3 path_offsets[M a + j] .. 3 path_offsets[M a + j + 1]), in sca_set_paths' list order (pop() takes the last element).  The
 * lists live on the device as the call brought them, immutable until the tables are replaced.
 *   precondition  the context's lists are in SLOT form (sca_set_path_slots(W, ...) earlier); the flight in the air keeps its list, its
 *              cursors and now_goal.  Not in slot form: with path_offsets == NULL the call IS sca_set_missions, with path_offsets it is
 *              SCA_ERR_STATE; lists in block form: SCA_ERR_UNSUPPORTED.  Slot form with path_offsets == NULL: every entry brings the empty
 *              list.  sca_set_missions itself keeps refusing a context with lists; sca_set_paths and sca_set_path_slots keep refusing
 *              while tables stand, sca_step_host too.
 *   the rule   nothing changes about endings, results, totals, the gate's order or its verdicts.  Where the step TAKES entry j for row a
 *              -- on the plain path and for the gate's admitted row -- the row becomes word for word what sca_respawn_agents naming it
 *              with entry j's values AND entry j's list as its path arrays leaves: the list in the row's room, len = rem = its length,
 *              now_goal None; a straight-line row that had a list (len[a] > 0 in front of the take) gets vpref_mode 0 and the next pass's
 *              k_waypoint_slots sets it back where the new list is not empty; a tracked row keeps mode 1 and the tracker's v_pref, its
 *              list advances.  A candidate that waits at the gate keeps every word, list and cursors included; a stop (-1) leaves the
 *              list as it is.  The next pass pops from the new list: k_waypoint_slots runs on the context's stream at the head of the
 *              pass, behind the mission kernel, in every step form.
 *   mirrors    a take moves a row's list length on the device.  While tables with lists stand the host entry points that read the
 *              lengths (sca_set_vpref's mode-1 refusal, sca_set_path_state's bound, sca_respawn_agents' mode bit, clearing the lists)
 *              first read them back: one copy of n words behind a synchronisation, never inside a step.
 *   dropping   sca_set_missions_paths(M = 0, entries = NULL), sca_set_missions(M = 0) and sca_set_agents drop tables and their lists; the
 *              slot form and the rows' current lists stay.  While tables WITH lists stand sca_set_paths(0 / NULL) is SCA_ERR_UNSUPPORTED:
 *              it would take the rooms away under the step.
 *   refusals   decided on the host before any device work, a refused call changes nothing: everything sca_set_missions refuses, with
 *              its codes, and SCA_ERR_ARG for path_offsets[0] != 0, offsets that decrease, path_points == NULL with points to read,
 *              more than 2^31 / 3 points, a REACHABLE entry whose list is longer than W or holds a point that is not finite (an entry
 *              nobody reaches is not inspected beyond its offsets).
 * sca_get_mission_paths: W and the points the tables' lists hold; 0 / 0 for tables without lists.  sca_mission stays 128 bytes and the
 * version number is unchanged: detect the feature by the symbol. */
int sca_set_missions_paths(sca_ctx *ctx, int M, int R, int n, const sca_mission *entries /*M*n*/, const int32_t *first_ok /*n*/,
                           const int32_t *first_fail /*n*/, const int32_t *path_offsets /*M*n+1, nullable*/,
                           const double *path_points /*path_offsets[M*n]*3*/);
int sca_get_mission_paths(sca_ctx *ctx, int *points_per_agent, int64_t *total_points);

/* The admission gate on the device: a row takes its next mission only where its start is free.  sca_set_missions puts a row wherever its
 * table says, also inside another drone; sca_respawn_agents_gated refuses such a start, but as a host call between two steps.  With a gate
 * set the two combine: behind every env update, on the records K4 wrote, the rows that ended are CANDIDATES for the entry their flight
 * names, and a candidate is taken only where sca_respawn_agents_gated would admit it -- with no host round trip, so sca_run_steps(k)
 * runs gated traffic.
 *   endings    unchanged: a row with a table that ended writes its result now, `ended`, `flying` and the outcome totals move as without
 *              a gate, the result's `next` is the successor the flight NAMES; -1 stops the row as before.  j >= 0 makes the row a new
 *              candidate for entry j: nothing of the row is written yet, its cursor stays, `taken` does not move yet.
 *   order      first the rows WAITING since an earlier step, ascending id, then this step's new candidates, ascending id (the offer order
 *              of lifelong.run_lifelong(spawn_margin=)).  Only the first max_per_step candidates are tested; the others wait with
 *              SCA_SPAWN_OVER_CAP (it counts as a refusal).  Waiting rows come first: new arrivals starve nobody that was tested before.
 *   test       sca_respawn_agents_gated's rule with the candidates as the call's rows, in that order: candidate r is the sphere of the
 *              row's own radius at entry j's pos (SCA_MISSION_START_HERE: where the row stands), ignore = its own row, against every
 *              other agent row where it stands now -- the other candidates included -- and every obstacle (world test), then against
 *              every EARLIER candidate that is world-clear (entry test, with the documented chain behaviour).
 *   verdict    admitted: the row becomes what sca_respawn_agents naming it with entry j's values leaves (as `taking` above), cursor =
 *              flying = j, `taken` + 1, its waiting word -1.  Refused: the row keeps every word and stays finished (sca_get_finished
 *              lists it, no kernel of a step serves it); waiting[a] = j, verdict[a] = the word, refusals[a] + 1 (never reset); it is
 *              offered again behind the next update.
 *   kernels    in place of k_mission_advance, only while a gate is on, all on the context's stream in front of the buffer swap, with
 *              no host read: k_mission_gate_end (endings, results, totals, the candidates counted per tile of 256 rows by ballot and
 *              popcount), k_mission_gate_place (a candidate's place from the tiles' counts -- every workgroup sums the earlier tiles
 *              itself; no atomic cursor, no wait between workgroups -- its query, row and entry into a device list, the count into
 *              device memory, the over-cap words), k_mission_gate_probe (k_spawn_probe's tiling: 512 partners staged in LDS, 64
 *              queries per chunk, four wavefronts; a bounded number of chunk slots per tile whose workgroups loop over the chunks the
 *              count on the device says exist), k_mission_gate_fold (the world word) and k_mission_gate_take (a wavefront per
 *              candidate: the entry walk, then its own row).  Vector stores throughout; 64-bit integer atomics for the counters, only
 *              where non-zero.  The scratch (the list, tiles x cap x 32 bytes of partials, the words) is allocated by
 *              sca_set_mission_gate and freed with the tables; a context without a gate allocates and enqueues nothing new.
 *   sca_set_mission_gate   on != 0: margin in metres (>= 0), max_per_step 0: min(n, 4096), else 1 .. n.  on == 0: the pending missions of
 *              waiting rows are dropped (`dropped`), the rows stay finished for the host, the context enqueues exactly
 *              k_mission_advance again.  sca_set_missions clears the gate (new tables and M = 0 alike), sca_set_agents drops it.
 *              A call that is refused or fails leaves a standing gate exactly as it was (its margin, its cap, the rows waiting).
 *              SCA_ERR_STATE: no tables, between a policy pass and its env update.  SCA_ERR_ARG: a margin that is negative or not
 *              finite, a cap outside 0 .. n, partials above 1 GiB.  The gate works with everything tables work with; what tables
 *              refuse stays refused.
 *   host calls while a gate is on: a plain or gated host respawn that ADMITS a waiting row clears its waiting word (`dropped` + 1: the
 *              pending mission is gone, the cursor stays); sca_set_state clears the waiting word of the rows that are unfinished in the
 *              new state (`dropped` + 1 each) and keeps that of rows still finished.
 *   getters    sca_get_mission_gate_state: the waiting (-1: none), last verdict and refusal words of rows begin .. begin + count - 1.
 *              sca_get_mission_gate_totals: 64-bit counters since the first sca_set_mission_gate behind the tables: offered == admitted
 *              + blocked_agent + blocked_obstacle + blocked_entry + over_cap, counted per attempt; with the gate set before the first
 *              step, arrived + collided + timed_out == taken + stopped + dropped + the rows waiting now.  SCA_ERR_STATE while no tables
 *              stand or no gate has been set since they arrived.  sca_mission_totals and sca_mission_result are unchanged.
 * Detect the feature by the symbols (the version number is unchanged). */
typedef struct sca_mission_gate_totals { /* 64 bytes */
    uint64_t offered, admitted, blocked_agent, blocked_obstacle, blocked_entry, over_cap, dropped, reserved;
} sca_mission_gate_totals;
int sca_set_mission_gate(sca_ctx *ctx, int on, double margin, int32_t max_per_step);
int sca_get_mission_gate_state(sca_ctx *ctx, int begin, int count, int32_t *waiting /*count*/, int32_t *verdict /*count*/,
                               int32_t *refusals /*count*/);
int sca_get_mission_gate_totals(sca_ctx *ctx, sca_mission_gate_totals *out, int32_t struct_bytes);

/* the hot path ----------------------------------------------------------------------------------- */
int sca_policy_pass(sca_ctx *ctx, int neighbor_mode);
int sca_get_actions(sca_ctx *ctx, float *action /*n*7*/);
int sca_get_neighbors(sca_ctx *ctx, int32_t *nbr_n /*n*/, int32_t *nbr_id /*n*16*/, uint8_t *nbr_kind /*n*16*/,
                      double *nbr_dsq /*n*16*/, uint8_t *nbr_valid /*n*/);
/* distSq of agent.neighbors[0] after the last pass: >= 0 value, -1 empty list, -2 list not touched by the pass */
int sca_get_nbr0(sca_ctx *ctx, double *dsq0 /*n*/);
int sca_get_diag(sca_ctx *ctx, int32_t *diag /*n*5*/, int32_t *status /*n*/, double *vpref_used /*n*3*/);
int sca_env_update(sca_ctx *ctx, int *all_done /*nullable: skips the readback*/);
/* `steps` x (policy pass + env update) with the state resident in HBM; returns without synchronising.  steps == 0 does nothing;
 * steps < 0 is SCA_ERR_ARG, a neighbor_mode outside sca_neighbor_mode SCA_ERR_UNSUPPORTED, no state yet SCA_ERR_STATE (tests/test_gpu_abi_errors.py) */
int sca_run_steps(sca_ctx *ctx, int steps, int neighbor_mode);
/* MACAEnv.step (mampenv.py:22-25) in one call: one resident step (both loops of _take_action + is_done), then the number of agents of
 * this rank still running after it (0 == is_done) -- sca_run_steps(ctx, 1, mode) + sca_active_count with one stream synchronisation and
 * one pinned 32-KB read-back.  What `while not env.step()` of the drop-in env costs per step beyond the kernels (bench.py `env_api`).
 * It returns when the context's stream is through; an SCA_NBR_AUTO pass may still have its kd-tree build and the kd query of the listed
 * agents on the library's second stream -- the next sca_env_step copes with that as the steps inside sca_run_steps do, and EVERY other
 * entry point that takes the context first puts that stream in front of the context's (so whatever is read between steps is final). */
int sca_env_step(sca_ctx *ctx, int neighbor_mode, int *active);

/* The same step for a host that OWNS the state (the reference's own mampenv.py stays in charge and calls the library from _take_action,
 * mampenv.py:27-59): a page-locked state block of the library's that the caller reads and writes in place, and ONE call that steps from it
 * and into it -- instead of sca_set_state -> sca_policy_pass -> sca_get_actions -> sca_env_update -> sca_get_state (five synchronisations,
 * every array a pageable copy of its own, the record transposition on one host thread).  Those five calls stay valid and may be mixed with
 * this one; sca_version() is unchanged (callers detect the feature by the symbol).
 *   sca_host_state_layout  byte offsets of the nine sections for n agents, in the struct's order, and the block's size: the up-going sections
 *                       (state, then v_pref) first and contiguous, the down-only action rows last, every section on a 64-byte boundary.  Pure
 *                       host arithmetic, no GPU.  n <= 0 or a NULL pointer: SCA_ERR_ARG.
 *   sca_host_state_get  after sca_set_agents (SCA_ERR_STATE before).  The first call allocates one page-locked block sized for sca_create's
 *                       max_agents, mapped into the device's address space; it lives until sca_destroy and is never reallocated, so a
 *                       stale pointer is never dangling.  The pointers handed out follow the layout of the CURRENT n: fetch the struct again
 *                       after a sca_set_agents with another n.  struct_bytes = sizeof(sca_host_state) as the caller compiled it (the sca_params
 *                       convention): at least the two leading integers, at most this library's struct, else SCA_ERR_ARG; only the pointers that
 *                       fit are written.  The block starts zeroed.
 *   sca_step_host       one step of the env loop.  in_mask says what the caller wrote since the last call: SCA_HOST_IN_STATE takes the six in/out
 *                       arrays (= sca_set_state, total_dist and step_num included; `radius` stays as sca_set_agents put it), SCA_HOST_IN_VPREF
 *                       takes vpref / vpref_mode (= sca_set_vpref, including its refusal of a non-zero mode for a straight-line agent that follows
 *                       a waypoint list).  k_host_ingest reads what was written out of the block across the link, one resident step (sca_env_step's),
 *                       k_host_egress writes the state and the action sections into the block (the caller's v_pref sections are never written),
 *                       the active count comes down in the same round trip, ONE synchronisation.  (SCA_HOST_STEP_STAGED=1 in the environment of
 *                       sca_create: a device staging buffer of the block's size instead -- one copy up, the kernels on the copy, two copies down;
 *                       measured slower at N = 1024, 4096 and 100 000, kept for A/B runs.)  On return the block holds the state after the step and the action rows (the rows of
 *                       sca_get_actions) the step integrated; *active = sca_env_step's.  in_mask == 0: the host only reads; it writes when it has
 *                       something to say (teleports, retirements).  Everything is enqueued on the context's current stream (sca_set_stream).
 *                       SCA_ERR_STATE: no agents; no state yet and no SCA_HOST_IN_STATE; in_mask != 0 before any sca_host_state_get (nothing can
 *                       have been written); a shard (sca_set_shard with count < n).  SCA_ERR_UNSUPPORTED: a communicator (sca_comm_init), the
 *                       cell-owner partition (the block is the whole swarm's state on one rank), a neighbor_mode outside sca_neighbor_mode.
 *                       SCA_ERR_ARG: active == NULL, unknown bits in in_mask.  A refused call has changed nothing. */
typedef struct sca_host_state {          /* pointers into ONE page-locked allocation of the library's; rows of agent i at index i */
    int32_t struct_bytes, n;             /* n of the last sca_set_agents */
    double  *pos;                        /* n*3  in/out */
    float   *vel;                        /* n*3  in/out */
    double  *heading;                    /* n*3  in/out */
    uint8_t *flags;                      /* n    in/out */
    double  *total_dist;                 /* n    in/out */
    int32_t *step_num;                   /* n    in/out */
    double  *vpref;                      /* n*3  in     */
    uint8_t *vpref_mode;                 /* n    in     */
    float   *action;                     /* n*7  out: the rows of sca_get_actions */
} sca_host_state;
#define SCA_HOST_IN_STATE 1
#define SCA_HOST_IN_VPREF 2
int sca_host_state_layout(int n, int64_t *offsets /*9, in the struct's order*/, int64_t *total_bytes);
int sca_host_state_get(sca_ctx *ctx, sca_host_state *out, int32_t struct_bytes);
int sca_step_host(sca_ctx *ctx, int neighbor_mode, uint32_t in_mask, int *active);

int sca_synchronize(sca_ctx *ctx);
/* number of this rank's agents that are not done (at goal, collided or timed out) after the last env update; 0 == the
 * `all(agent.is_run_done)` of MACAEnv.is_done (mampenv.py:51-59).  Synchronises; reports a failed device kd build. */
int sca_active_count(sca_ctx *ctx, int *active);

/* multi-GPU / interop ------------------------------------------------------------------------------ */
/* This rank solves agents [begin, begin+count); all agents' public records must be present. */
int sca_set_shard(sca_ctx *ctx, int begin, int count);
/* Device address of a public-record array (48 B per agent: pos f64x3, vel f32x3, flags u32, radius f64).
 * which = 0: the current records; which = 1: the "moved" records written by sca_step_begin, i.e. the buffer an
 * RCCL all-gather (torch.distributed) exchanges between sca_step_begin and sca_step_end. */
int sca_public_records(sca_ctx *ctx, int which, void **device_ptr, int64_t *bytes_per_agent);
/* Use caller-owned device memory (e.g. two torch tensors of n*48 bytes, n of sca_set_agents; bytes_each says how large each
 * is and is checked) for the two record arrays; NULL, NULL restores the internal ones.  The n live records are carried over. */
int sca_bind_public_records(sca_ctx *ctx, void *current, void *moved, int64_t bytes_each /* >= n*48, n of sca_set_agents */);
/* One step split around the exchange: begin = kd build + neighbours + solve + integrate for this rank's shard
 * (writes the shard's moved records); [all-gather of the moved records]; end = collision / goal flags + publish. */
int sca_step_begin(sca_ctx *ctx, int neighbor_mode);
int sca_step_end(sca_ctx *ctx);
/* Run on a caller-provided hipStream_t, e.g. the torch stream a collective between sca_step_begin and sca_step_end is issued
 * on: the library's kernels and that collective are ordered only if they share the stream.  NULL is taken literally: HIP's
 * null stream (which is what torch's default stream is).  sca_use_own_stream() goes back to the context's own non-blocking
 * stream (the default after sca_create).  Both drain the stream in use first. */
int sca_set_stream(sca_ctx *ctx, void *hip_stream);
int sca_use_own_stream(sca_ctx *ctx);
/* RCCL inside the library (nothing in the reference: it is single-process).  One process per GPU; rank 0 calls
 * sca_comm_unique_id and hands the 128 bytes (an ncclUniqueId) to the other ranks by any means; every rank then calls
 * sca_comm_init after sca_set_agents.  From then on this rank owns agents [rank*n/nranks, (rank+1)*n/nranks) (n must divide),
 * (sca_set_shard / sca_set_shard_emulation return SCA_ERR_STATE while the communicator exists),
 * and every step of sca_run_steps is: shard's policy pass + integrate -> ncclAllGather of the shard's moved 48-byte records
 * on the library's stream -> collision / goal flags, i.e. a multi-GPU episode is ONE host call per k steps.  librccl.so is
 * loaded with dlopen at the first call; SCA_ERR_UNSUPPORTED when it is missing. */
/* 0 when librccl.so can be loaded and has every entry point the library uses, SCA_ERR_UNSUPPORTED otherwise.  No collective, no
 * device work: ranks call it and AGREE on the result before any of them calls sca_comm_init, which blocks inside
 * ncclCommInitRank until every rank has arrived. */
int sca_comm_probe(void);
int sca_comm_unique_id(void *id_out /*128 bytes*/);
int sca_comm_init(sca_ctx *ctx, int rank, int nranks, const void *unique_id /*128 bytes*/);
int sca_comm_destroy(sca_ctx *ctx);
/* Cell-owner partition of SCA_NBR_GRID with halo exchange (nothing in the reference: it is single-process).
 * Space is cut into slabs of grid cells along `axis` (0 x, 1 y, 2 z); rank r owns the agents whose cell lies in its slab and
 * holds copies of the agents in the one layer of cells on either side (the halo) -- everything the neighbour query
 * (kdTree.py:124-156, agent.py:79-99 on the grid) and the collision check (mampenv.py:61-80) of its agents look at.  Per step
 * it exchanges, with its two slab neighbours only, the old + moved records of the agents next to the cut and the private state
 * (heading, v_pref, distances, tracker record) of agents that crossed it, instead of all N records.  Results equal a single
 * rank's bit for bit (tests/test_gpu_partition.py: 2 / 3 processes against a one-rank run; tests/test_gpu_partition_fuzz.py: up to five ranks
 * in one process on scenes made for the cuts, every agent after every step against the oracle of the grid's list rule -- owner sets, halo
 * counts, message headers, and for a migrant everything that travelled with it).
 *   sca_partition_init   after sca_set_agents + sca_set_state with the COMPLETE state on every rank.  cuts: nranks - 1 ascending
 *                        coordinates along the axis, or NULL = equal shares of the agents as they stand; moved onto cell
 *                        boundaries.  cap_halo / cap_mig: entries per message (0 = n / 4 and n / 16, at least 1024 and 256); an overflow
 *                        is reported by sca_partition_commit or the next sca_synchronize.  From then on the per-agent arrays of sca_get_* are meaningful for the owned
 *                        agents only (sca_partition_owned).  sca_set_state (complete again) re-derives the ownership.
 *   one step             sca_step_begin(SCA_NBR_GRID) -> sca_partition_pack into two DEVICE buffers of sca_partition_message_bytes()
 *                        (for the lower / the upper slab neighbour) -> exchange (what a rank packed for its lower neighbour is
 *                        what that neighbour unpacks as the message from ITS upper one) -> sca_partition_unpack(from lower,
 *                        from upper) -> sca_partition_commit (ownership moves; nothing waits for the device: the host sizes its
 *                        launches with bounds and learns the exact counts a step or two late) -> sca_step_end.
 *                        With one rank sca_run_steps does all of it. */
int sca_partition_init(sca_ctx *ctx, int rank, int nranks, int axis, const double *cuts /*nranks-1, nullable*/, int cap_halo, int cap_mig);
int sca_partition_disable(sca_ctx *ctx);
int64_t sca_partition_message_bytes(sca_ctx *ctx);
int sca_partition_pack(sca_ctx *ctx, void *device_buf_lower, void *device_buf_upper);       /* NULL where there is no neighbour */
int sca_partition_unpack(sca_ctx *ctx, const void *device_buf_lower, const void *device_buf_upper);
int sca_partition_commit(sca_ctx *ctx);
int sca_partition_counts(sca_ctx *ctx, int *owned, int *halo);
int sca_partition_owned(sca_ctx *ctx, int32_t *ids /*n*/, int *count);
/* average device time of the kernels of the last sca_policy_pass / sca_run_steps, measured with HIP events */
int sca_last_kernel_ms(sca_ctx *ctx, float *neighbors_ms, float *solve_ms, float *update_ms);

/* the same for the tracker's re-plan kernels (k_replan_group<4 .. 64 lanes per plan>, k_replan, k_track_replan), events on the stream they run on */
int sca_last_replan_ms(sca_ctx *ctx, float *replan_ms);
/* the kd build of kdTree.py:56-122 (k_kd_gather .. k_kd_block), events on the stream it ran on, every 16th build while profiling */
int sca_last_kd_build_ms(sca_ctx *ctx, float *kd_build_ms);
/* the same for the step's exchange when the library issues it (sca_comm_init: ncclAllGather inside sca_run_steps); 0 without a communicator */
int sca_last_exchange_ms(sca_ctx *ctx, float *exchange_ms);
/* Which kernel forms the last policy pass was launched with (the library picks them per pass from the shard size and the
 * re-plan count of a recent pass; none of them changes a result bit -- tests/test_gpu_solve_split.py, test_gpu_tracker.py):
 *   SCA_FORM_SOLVE_SPLIT   k_solve as k_solve_sweep (beside the tracker's re-plans) + k_solve_pick4 (behind them)
 *   SCA_FORM_TRACK_FUSED   k_track_replan instead of k_track + k_replan (with SCA_FORM_REPLAN_FEW: k_track_group, decision + 64-lane search per agent)
 *   SCA_FORM_REPLAN_LANE   the lane-per-plan re-plan kernel was launched (k_replan or k_track_replan)
 *   SCA_FORM_REPLAN_FEW    a k_replan_group kernel (4 .. 64 lanes per plan) was launched
 *   SCA_FORM_LP_LANE       the ORCA3D-Official agents went to k_lp (one lane per agent)
 *   SCA_FORM_SOLVE_FB      k_solve_fb: small shards solve and finish their fallbacks in one launch (no k_fallback launch)
 *   SCA_FORM_ACTION_FB     k_action_fb: shards of up to 16 384 agents run the fallback sweep inside the epilogue's launch (no k_fallback launch)
 *   SCA_FORM_AUTO_TAIL     SCA_NBR_AUTO: the kd query of the listed agents ran inside the pass's grid query (its last workgroup, from the tree the pass's
 *                          build publishes): no k_neighbors_kd_auto launch, no stream wait in front of the solve
 *   SCA_FORM_WAYPOINTS     k_waypoint ran at the head of the pass (waypoint lists are set: sca_set_paths)
 *   SCA_FORM_SCENES        scenes are set (sca_set_scenes): the forest build and the scene forms of the neighbour query ran
 *   SCA_FORM_SCENE_OBSTACLES  ... with one obstacle set per scene (sca_set_scene_obstacles): the obstacle walks started at each scene's own root
 *   SCA_FORM_VACANCY       a row is vacant (sca_retire_agents): the kd build took the occupied rows for its size, and SCA_NBR_AUTO was the plain kd pass */
#define SCA_FORM_SOLVE_SPLIT 1
#define SCA_FORM_TRACK_FUSED 2
#define SCA_FORM_REPLAN_LANE 4
#define SCA_FORM_REPLAN_FEW 8
#define SCA_FORM_LP_LANE 16
#define SCA_FORM_SOLVE_FB 32
#define SCA_FORM_ACTION_FB 64
#define SCA_FORM_AUTO_TAIL 128
#define SCA_FORM_WAYPOINTS 256
#define SCA_FORM_SCENES 512
#define SCA_FORM_SCENE_OBSTACLES 1024
#define SCA_FORM_VACANCY 2048
int sca_last_pass_forms(sca_ctx *ctx, int *forms);
/* SCA_NBR_AUTO statistics since the last reset: out4 = {AUTO passes, agents the grid query listed for the kd query (sum over the passes), the
 * largest list, passes in which somebody was listed}.  A pass with nobody listed never waits for the kd stream. */
int sca_auto_stats(sca_ctx *ctx, int64_t *out4, int reset);
/* Measurement aid for scaling models on one GPU: with a partial shard (sca_set_shard) and no communicator, sca_run_steps
 * runs what ONE rank of a larger job runs per step -- the replicated neighbour structure over all n agents, everything else
 * for the shard -- and copies the other agents' records over unchanged where the all-gather would deliver them. */
int sca_set_shard_emulation(sca_ctx *ctx, int on);

/* with profiling on, sca_run_steps brackets every kernel launch of the policy pass with HIP events on its stream;
 * sca_synchronize() then folds them into the averages sca_last_kernel_ms() returns */
int sca_set_profiling(sca_ctx *ctx, int on);
/* number of agents that entered find_next_action since the last reset (the metric's "agent-steps") */
int sca_agent_steps(sca_ctx *ctx, int64_t *count, int reset);

/* device self-test: numerators of l3norm(a_i, b_i) = round(|a_i - b_i|, 5) (mamp/util.py:104) as the solver's fast path
 * computes them (fast[]) and as the literal restatement does (exact[]); they must be identical */
int sca_selftest_l3norm(sca_ctx *ctx, int n, const double *a /*n*3*/, const double *b /*n*3*/, double *fast /*n*/, double *exact /*n*/);
/* The tracker's libm (sca_amd/csrc/sca_glibc_math.h: glibc 2.35's sin / cos / atan2 / acos / pow(x, 2) restated operation for
 * operation, so that the device computes the reference's -- i.e. Python's math module's -- bits).  fn: 0 sin(a), 1 cos(a),
 * 2 acos(a), 3 atan2(a, b), 4 pow(a, 2) -- the branch-free forms the kernels call; 5 sin, 6 cos, 7 atan2, 8 pow as the literal
 * restatements of glibc's control flow; 9 / 10 the sine / cosine of the fused sincos; 11 atan2, 12 sin, 13 cos, 14 pow(a, 2) as cartesian2spherical (util.py:44-55),
 * get_phi (util.py:145) and update_velocitie (mampenv.py:83-105) call them on the device (constant tables).  b may be NULL unless fn is 3, 7 or 11.  sca_selftest_libm evaluates on the device,
 * sca_selftest_libm_host on the host (no GPU needed); tests demand both equal the running glibc bit for bit. */
int sca_selftest_libm(sca_ctx *ctx, int fn, int n, const double *a, const double *b, double *out /*n*/);
int sca_selftest_libm_host(int fn, int n, const double *a, const double *b, double *out /*n*/);

/* Trajectory log = Agent.history_info (mamp/agents/agent.py:75-77, filled by to_vector :126-148 at the end of every
 * update_velocitie, mamp/envs/mampenv.py:105): one 64-byte row per agent per env step, kept in HBM so that resident
 * runs (sca_run_steps) need no per-step readback.  Row r = the r-th env step after sca_history_enable; every agent logs
 * every step, done agents included, as in the reference.  The goal and radius columns of ANIMATION_COLUMNS are constants
 * of sca_set_agents.  Steps beyond capacity_rows are counted as dropped, never overwritten.  With sca_set_shard a rank
 * logs its own shard only.  capacity_rows == 0 frees the log; sca_set_agents frees it too. */
int sca_history_enable(sca_ctx *ctx, int capacity_rows);
int sca_history_rows(sca_ctx *ctx, int *rows_logged, int *rows_dropped);
/* window [first_row, first_row+nrows) x [agent_begin, agent_begin+agent_count), row-major [row][agent][3]; any output
 * pointer may be null */
int sca_get_history(sca_ctx *ctx, int first_row, int nrows, int agent_begin, int agent_count, double *pos /*pos_x..z*/,
                    double *heading /*alpha, beta, gamma*/, float *vel /*vel_x..z*/);

/* native preferred-velocity tracker for SCAPolicy / RVO3dDubinsPolicy (host side, thread-parallel over agents):
 * replaces compute_v_pref / compute_dubins / update_dubins (mamp/policies/sca/scaPolicy.py:92-104,243-338) and the 3-D
 * Dubins planner (dubinsmaneuver3d.py:34-162, dubinsmaneuver2d.py:33-218,260-297).  Feed its output to sca_set_vpref. */
void *sca_tracker_create(int n, const double *goal /*n*3*/, const double *goal_heading /*n*3*/, const double *pref_speed /*n*/,
                         const uint8_t *zaxis /*n, nullable*/, double turning_radius /*agent.py:24 1.5*/,
                         double pitch_min, double pitch_max /*agent.py:27*/, double neighbor_dist /*agent.py:33*/);
/* agent.neighborDist per agent (scaPolicy.py:299 reads the agent's own when its list is empty); NULL: the one value of sca_tracker_create */
int sca_tracker_set_neighbor_dist(void *tracker, const double *neighbor_dist /*n, nullable*/);
/* agent.turning_radius / agent.pitchlims per agent for the host tracker (arrays of n, NULL = the constructor's value) */
int sca_tracker_set_agent_params(void *tracker, const double *turning_radius, const double *pitch_lo, const double *pitch_hi);
void sca_tracker_destroy(void *tracker);
/* one compute_v_pref per agent with active[i] != 0; nbr0_dsq[i] = distSq of agent.neighbors[0] as left by the previous
 * policy pass, negative when the list is empty (scaPolicy.py:299) */
int sca_tracker_vpref(void *tracker, const double *pos /*n*3*/, const float *vel /*n*3*/, const double *heading /*n*3*/,
                      const uint8_t *active /*n*/, const double *nbr0_dsq /*n*/, double *vpref_out /*n*3*/, int nthreads);
int sca_tracker_replans(void *tracker, int32_t *replans /*n*/);
/* dubinsmaneuver3d (dubinsmaneuver3d.py:34): q = [x, y, z, yaw, pitch]; samples = [x, y, z, psi, gamma] rows */
int sca_dubins_plan(const double *qi5, const double *qf5, double rmin, double pitch_min, double pitch_max, double *length,
                    char *mode7, int32_t *n_samples, double *samples /*nullable, cap*5*/, int cap);

/* What the tracker's bit-for-bit claim is conditional on.  Host and device tracker compute sin / cos / atan2 / acos / x ** 2 with a
 * restatement of ONE libm build -- GNU C Library 2.35, x86-64, the FMA variants (sca_amd/csrc/sca_glibc_math.h), the libm under the
 * Python that recorded tests/golden/.  math.sin & co. of a reference run on another host are THAT host's libm; if it is another
 * build the reference itself prints other last bits there, and this library keeps printing 2.35's.  sca_libm_check compares the
 * restatement with the running libm on a fixed set of 5 x 4096 arguments: returns 0 when they agree, 1 when they do not
 * (mismatches[5], nullable: sin, cos, atan2, acos, pow(x, 2)).  sca_tracker_create prints one note on stderr in the second case
 * (SCA_QUIET silences it), and so does the first sca_device_tracker_enable; sca_last_error stays reserved for failures (round 4 put the
 * note there after a SUCCESSFUL enable; callers that test it for emptiness saw a failure).  Thread-safe (one check per process).
 * Behaviour never changes. */
int sca_libm_check(int64_t *mismatches);

/* The same tracker on the device: one lane per agent for the tracking, tracker records resident in HBM, the re-planning
 * agents of a step compacted into kernels of their own -- one lane up to one wavefront per plan, by how many a step has
 * (sca_amd/csrc/sca_tracker.hip.h).  Same statements as the host tracker AND the same libm (sca_glibc_math.h: glibc's sin / cos /
 * atan2 / acos / pow restated operation for operation, device build checked against the host's bit for bit): v_pref, every
 * follow-or-re-plan decision and every plan equal the host tracker's -- i.e. the reference's -- bit for bit
 * (tests/test_gpu_tracker.py).
 * sca_device_tracker_enable: agents with policy SCA / RVO3D_DUBINS take v_pref from it from now on -- inside every
 * sca_policy_pass / sca_step_begin / sca_run_steps when in_pass != 0 (agent.neighbors[0] of the previous pass is read from
 * the neighbour lists on the device), otherwise only through sca_device_tracker_vpref.  sca_set_agents disables it. */
int sca_device_tracker_enable(sca_ctx *ctx, const double *goal_heading /*n*3, agent.py:19*/, double turning_radius,
                              double pitch_min, double pitch_max, int in_pass);
/* the tracked agents take v_pref from their policy's own straight-line rule again (sca_set_vpref afterwards to feed it from the host) */
int sca_device_tracker_disable(sca_ctx *ctx);
/* agent.turning_radius / agent.pitchlims PER AGENT (the reference keeps them on every Agent object; scaPolicy.py:95,272,302 read the agent's own).
 * Arrays of n, a NULL array = sca_device_tracker_enable's value for everybody, all NULL = back to that one value.  Entries of untracked agents
 * (policy not SCA / RVO3D_DUBINS) are ignored; a tracked agent needs turning_radius > 0 and pitch_lo < pitch_hi (SCA_ERR_ARG otherwise).
 * Up to 16 distinct (turning_radius, pitch_lo, pitch_hi) among the tracked agents: classes -- the re-plan kernels run once per class with the
 * class's values as kernel arguments (the search keeps the three in scalar registers).  More (the reference has no limit): the per-agent
 * form -- every re-plan gets a wavefront of its own, which loads its agent's values; slower for large re-plan counts, never refused.
 * After sca_device_tracker_enable.  Parity: tests/golden/F18_hetero_track_* (3 x 3 classes; F18_hetero_track_circle30_each: 30 settings). */
int sca_device_tracker_set_agent_params(sca_ctx *ctx, int n, const double *turning_radius, const double *pitch_lo, const double *pitch_hi);
/* one compute_v_pref per active tracked agent on the current state; nbr0_dsq as in sca_tracker_vpref, NULL = from the
 * device's neighbour lists; vpref_out nullable */
int sca_device_tracker_vpref(sca_ctx *ctx, const double *nbr0_dsq /*n, nullable*/, double *vpref_out /*n*3, nullable*/);
int sca_device_tracker_replans(sca_ctx *ctx, int32_t *replans /*n*/);

/* diagnostics: the tracker record of one agent as 24 doubles -- horizontal maneuver (r_min, t, p, length), vertical maneuver
 * (the same four), plan length, sampling size, rounds of the speculative search that produced the plan (0: a one-step-at-a-time form), one
 * unused slot, cursor, sample count, tracked node[3], untruncated v_pref[3],
 * the two words, 64 x candidate radii tried, re-plan count -- of the host tracker / the device tracker */
int sca_tracker_debug(void *tracker, int agent, double *out24);
int sca_device_tracker_debug(sca_ctx *ctx, int agent, double *out24);
/* host self-test (no GPU needed): the device planner's four-lane form evaluates the four CSC Dubins words
 * (dubinsmaneuver2d.py:33-109) as one sign-parametrised instruction stream; this compares it with the literal words on the
 * given frames (alpha, beta in [0, 2 pi), d >= 0) and counts results that are not bit-identical (must be 0) */
int sca_selftest_dubins_words(int n, const double *alpha, const double *beta, const double *d, int64_t *mismatches);
/* host self-test (no GPU needed): the device's lane-per-plan kernels run the 3-D planner's search in a lean form (a candidate
 * radius evaluated for feasibility and length only; far problems through a straight-line block; sca_dubins.hpp, plan3d_lean);
 * this runs that form, compiled for the host, and the literal planner (dubinsmaneuver3d.py:34-113) on n poses q[n][10] =
 * (qi[5], qf[5]) and counts plans that are not bit-identical (must be 0); the other two outputs (nullable) say how many
 * candidates took the lean block and how many the literal construction */
int sca_selftest_plan3d_lean(int n, const double *q, double turning_radius, double pitch_lo, double pitch_hi, int64_t *mismatches,
                             int64_t *lean_candidates, int64_t *literal_candidates);

/* host-only helpers (no GPU needed) ----------------------------------------------------------------- */
/* unit Fibonacci directions of scaPolicy.py:195-200 (SoA [3][num_N]) and the get_phi numerators */
int sca_candidate_table(int num_N, double *unit /*3*num_N*/, double *phi_num /*num_N*/);
/* replica of KDTree.buildAgentTreeRecursive: permutes perm in place, writes (2n-1) nodes of 10 doubles
 * [begin,end,left,right,min3,max3] when tree_out != NULL */
int sca_kd_build_host(int n, const double *pos /*n*3*/, int32_t *perm /*n*/, double *tree_out);

#ifdef __cplusplus
}
#endif
#endif
