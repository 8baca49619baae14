"""Drop-in host side for mamp.envs / mamp.agents / mamp.policies of wuuya1/SCA, backed by libsca_hip.

Same names, arguments and attribute surface as the reference (file:line cites are into wuuya1/SCA):
    Agent(start_pos, goal_pos, vel, radius, pref_speed, policy, id, dt)      mamp/agents/agent.py:9
    Obstacle(pos, shape_dict, id)                                            mamp/agents/obstacle.py:5
    SCAPolicy / RVO3DPolicy / SRVO3DPolicy / ORCA3DPolicy / ORCA3DPolicyOfficial / RVO3dDubinsPolicy
        .find_next_action(dict_comm, agent, kdTree) -> action[7]             e.g. mamp/policies/rvo3dPolicy.py:23
    MACAEnv().set_agents(agents, obstacles=[...]); MACAEnv.step(actions) -> bool   mamp/envs/mampenv.py:16-25

Differences that matter:
  * the env makes ONE library call per step for all agents (the reference calls find_next_action per agent,
    mampenv.py:34-40); `agent.policy.find_next_action(...)` still works for a single agent -- it runs the same
    batched pass and returns that agent's row;
  * per-agent state lives in structure-of-arrays owned by the env; the Agent attributes the reference exposes
    (pos_global_frame, vel_global_frame, heading_global_frame, is_at_goal, ...) are views / properties over them;
  * SCAPolicy and RVO3dDubinsPolicy take v_pref from the reference's Dubins tracker (scaPolicy.py:264-338), a host-side,
    per-agent stateful planner outside the kernel boundary.  The native restatement is sca_amd.tracker.DubinsTracker:
    pass it as MACAEnv(v_pref_fn=tracker) (any `v_pref_fn(env) -> [N,3]` works; bit-exact, host-bound), or use
    MACAEnv(device_tracker=True): the same tracker as kernels inside every pass (state stays in HBM; equal to the host
    tracker bit for bit -- same statements, same restated glibc libm); without either the straight-line rule of rvo3dPolicy.py:182-196
    is used and `env.dubins_tracker` is False;
  * the solver attributes of agent.py:24-41 -- turning_radius and pitchlims included -- are read off the agents in set_agents and travel per
    agent where the agents differ;
  * Agent.path (agent.py:44) is followed on the device (k_waypoint, see include/sca_hip.h sca_set_paths): the lists are uploaded by
    set_agents; `agent.path` then reads the env's mirror (the agent's own list, shortened in place to what the reference's pops leave,
    refreshed on first read after a step) and `agent.policy.now_goal` the device's now_goal (None before the first pass).  ASSIGNING
    `agent.path = [...]` after set_agents takes effect at the next step (in a SceneBatch(path_slots=W) too, through the lists' slot form,
    sca_set_path_slots); editing the list in place (append, insert, pop) is NOT tracked;
  * history logging (agent.py:126-147, pandas) and the per-step prints are not reproduced.
There is no CPU path: constructing the env without a GPU raises.
"""
import math

import numpy as np

from . import _lib
from . import scenarios as _sc
from . import solver as S

DT = 0.1                      # mamp/configs/config.py:2
NEAR_GOAL_THRESHOLD = 0.5     # mamp/configs/config.py:3


class _Policy:
    policy_id = None
    needs_external_vpref = False

    def __init__(self):                      # constructible with no arguments (agent.py:11 `policy()`)
        self._env = None
        self._agent_id = None
        self.now_goal = None
        self.type = 'internal'

    @property
    def now_goal(self):
        """get_trajectory's current target (rvo3dPolicy.py:71-85): with waypoint lists in the env, the device's (None before the first pass)"""
        env = self._env
        if env is not None and env._paths_on and self._agent_id is not None:
            return env._now_goal_of(self._agent_id)
        return self._now_goal

    @now_goal.setter
    def now_goal(self, value):
        self._now_goal = value

    def find_next_action(self, dict_comm, agent, kdTree):
        """Single-agent entry point of the reference API.  Runs the batched policy pass of the owning env (cached per
        step) and returns this agent's [vx, vy, vz, speed, d_yaw, d_pitch, d_roll]."""
        if self._env is None:
            raise RuntimeError('policy is not attached to a MACAEnv (call env.set_agents first)')
        row = self._env._policy_row(agent.id)
        if not self._env._paths_on:
            self.now_goal = agent.goal_global_frame      # get_trajectory with an empty agent.path (scaPolicy.py:89)
        return row


class SCAPolicy(_Policy):
    policy_id = S.POL_SCA
    needs_external_vpref = True


class RVO3DPolicy(_Policy):
    policy_id = S.POL_RVO3D


class SRVO3DPolicy(_Policy):
    policy_id = S.POL_SRVO3D


class ORCA3DPolicy(_Policy):                 # mamp/policies/orca3dPolicy.py (sampled, the one run_orca.py imports)
    policy_id = S.POL_ORCA3D


class ORCA3DPolicyOfficial(_Policy):         # mamp/policies/orca3dPolicyOfficial.py (linearProgram1-4)
    policy_id = S.POL_ORCA3D_LP


class RVO3dDubinsPolicy(_Policy):
    policy_id = S.POL_RVO3D_DUBINS
    needs_external_vpref = True


class Obstacle:
    def __init__(self, pos, shape_dict, id):
        self.shape = shape_dict['shape']
        self.feature = shape_dict['feature']
        if self.shape == 'cube':                                    # obstacle.py:9-11: bounding sphere
            self.length, self.width, self.height = shape_dict['feature']
            self.radius = math.sqrt(self.length ** 2 + self.width ** 2 + self.height ** 2) / 2
        elif self.shape == 'sphere':
            self.radius = shape_dict['feature']
        else:
            raise NotImplementedError
        self.pos_global_frame = np.array(pos, dtype='float64')
        self.vel_global_frame = np.array([0.0, 0.0, 0.0])
        self.pos = pos
        self.id = id
        self.is_at_goal = True
        self.is_obstacle = True
        self.is_collision = False


class Agent:
    def __init__(self, start_pos, goal_pos, vel, radius, pref_speed, policy, id, dt=0.1):
        self.group = 0
        self.policy = policy()
        self.initial_pos = np.array(start_pos, dtype='float64')
        self.goal_pos = np.array(goal_pos, dtype='float64')
        self._pos = np.array(start_pos[:3], dtype='float64')
        self.goal_global_frame = np.array(goal_pos[:3], dtype='float64')
        self._heading = np.array(start_pos[3:], dtype='float64')
        self.goal_heading_frame = np.array(goal_pos[3:], dtype='float64')
        self.initial_heading = np.array(start_pos[3:], dtype='float64')
        self._vel = np.array(vel, dtype=np.float32)
        self.radius = radius
        self.turning_radius = 1.5
        self.id = id
        self.pref_speed = pref_speed
        self.pitchlims = [-math.pi / 4, math.pi / 4]
        self.min_heading_change = self.pitchlims[0]
        self.max_heading_change = self.pitchlims[1]
        self.maxNeighbors = 16
        self.neighborDist = 10.0
        self.timeStep = DT
        self.timeHorizon = 10.0
        self.maxSpeed = 1.0
        self.dt_nominal = DT
        self._path = []
        self._v_pref = np.zeros(3)
        self.is_obstacle = False
        d = float(np.sqrt(((self.initial_pos[:3] - self.goal_pos[:3]) ** 2).sum()))
        self.straight_path_length = round(d, 5) - 0.5               # agent.py:51
        self.desire_steps = int(self.straight_path_length / (pref_speed * DT))
        self.max_run_dist = 3.0 * round(d, 5)                       # agent.py:74
        self._env = None
        self._flags = 0
        self._total_dist = 0.0
        self._step_num = 0

    # --- state: views over the env's arrays once attached -------------------------------------------------------------
    def _get(self, name, local):
        return local if self._env is None else getattr(self._env, name)[self.id]

    # The three attributes the reference's callers read per agent per step (run_sca.py:181-196).  The env's host mirrors are refreshed IN
    # PLACE (one bulk read-back on first use after a step), so an agent's row view is made once and stays valid: a read is an attribute
    # test, a staleness test and a return (100 000 reads per step went through three property hops and a fresh view).
    _row_pos = _row_vel = _row_heading = None

    @property
    def pos_global_frame(self):
        env = self._env
        if env is None:
            return self._pos
        if env._stale:
            env._state('pos')
        r = self._row_pos
        if r is None:
            r = self._row_pos = env._mirror['pos'][self.id]
        return r

    @property
    def vel_global_frame(self):
        env = self._env
        if env is None:
            return self._vel
        if env._stale:
            env._state('vel')
        r = self._row_vel
        if r is None:
            r = self._row_vel = env._mirror['vel'][self.id]
        return r

    @property
    def heading_global_frame(self):
        env = self._env
        if env is None:
            return self._heading
        if env._stale:
            env._state('heading')
        r = self._row_heading
        if r is None:
            r = self._row_heading = env._mirror['heading'][self.id]
        return r

    @property
    def path(self):
        """agent.path (agent.py:44): the waypoint list get_trajectory pops from the end.  Attached to an env with lists, the list object is
        shortened in place to what the device's passes have left of it (on first read after a step)."""
        env = self._env
        if env is not None and env._paths_on and env._path_stale:
            env._refresh_paths()
        return self._path

    @path.setter
    def path(self, value):
        env = self._env
        if env is not None and getattr(env, '_missions', None) is not None and env._path_slots:
            # (the upload would be sca_set_path_slots, which the library refuses while tables stand -- in the middle of the next step)
            raise RuntimeError('agent.path is read-only while mission tables stand on a MACAEnv(path_slots=W): the rows take their lists from '
                               'the tables\' entries (MissionTable(path=...)); drop the tables first (set_missions(None))')
        self._path = value
        if env is not None:
            env._path_assigned.add(self.id)               # uploaded in front of the next step

    @property
    def total_time(self):
        """agent.total_time (scaPolicy.py:30,35-37,62-64): wall time this agent's find_next_action calls took.  The batched
        pass serves every active agent at once, so a step's wall time is shared equally among the agents it served."""
        if self._env is None:
            return 0.0
        cum = self._env._time_cum
        return cum[min(self.step_num, len(cum) - 1)]

    @property
    def v_pref(self):
        """agent.v_pref as the last find_next_action left it (scaPolicy.py:337, rvo3dPolicy.py:195)"""
        if self._env is None:
            return self._v_pref
        return self._env._vpref_of(self.id)

    @property
    def total_dist(self):
        return float(self._get('total_dist', self._total_dist))

    @property
    def step_num(self):
        return int(self._get('step_num', self._step_num))

    def _flag(self, bit):
        f = self._flags if self._env is None else int(self._env.flags[self.id])
        return bool(f & bit)

    @property
    def is_at_goal(self):
        return self._flag(S.FLAG_AT_GOAL)

    @property
    def is_collision(self):
        return self._flag(S.FLAG_COLLISION)

    @property
    def is_out_of_max_time(self):
        return self._flag(S.FLAG_TIMEOUT)

    @property
    def is_vacant(self):
        """the row is vacant (MACAEnv.retire): out of the world until a respawn names it; its flags read 11"""
        return self._flag(S.FLAG_VACANT)

    @property
    def is_run_done(self):
        return self.is_at_goal or self.is_collision or self.is_out_of_max_time

    @property
    def neighbors(self):
        """[(object, distSq)] of the last policy pass, as agent.py:79-124 leaves it."""
        if self._env is None:
            return []
        return self._env._neighbors_of(self.id)


class MissionTable:
    """One agent row's upcoming missions (MACAEnv.set_missions).  entries: Agent-like objects (start, goal, velocity, pref_speed,
    max_run_dist and goal heading are read off them as respawn() reads them; the id is ignored).  Per entry: start_here -- the row
    keeps the position and heading it has, the entry's start is ignored; keep_zaxis -- it keeps its z-axis flag; next_ok / next_fail
    -- the entry flown after an arrival / after a collision or time-out, -1: the row stays finished for the host.  first_ok /
    first_fail: the successors of the flight that is in the air when the table is set.
    path: one waypoint list per entry (None: each entry's own Agent.path, usually empty) -- the route the row follows while it flies the
    entry, in Agent.path's order (get_trajectory pops from the end).  Needs MACAEnv(path_slots=W) with W >= the longest list."""
    def __init__(self, entries, next_ok, next_fail, first_ok=0, first_fail=-1, start_here=True, keep_zaxis=False, path=None):
        k = len(entries)
        if path is not None and len(path) != k:
            raise ValueError('MissionTable: one path per entry (an empty list for an entry without a route)')
        self.paths = [[list(map(float, w[:3])) for w in (a._path if path is None else path[j])] for j, a in enumerate(entries)]
        here = [bool(start_here)] * k if isinstance(start_here, (bool, int)) else [bool(x) for x in start_here]
        keep = [bool(keep_zaxis)] * k if isinstance(keep_zaxis, (bool, int)) else [bool(x) for x in keep_zaxis]
        self.entries = [(a, here[j], keep[j]) for j, a in enumerate(entries)]
        self.next_ok, self.next_fail = [int(x) for x in next_ok], [int(x) for x in next_fail]
        self.first_ok, self.first_fail = int(first_ok), int(first_fail)
        for x in self.next_ok + self.next_fail + [self.first_ok, self.first_fail]:
            if not -1 <= x < k:
                raise ValueError(f'MissionTable: successor {x} names no entry (-1 .. {k - 1})')
        if k < 1 or len(self.next_ok) != k or len(self.next_fail) != k or len(here) != k or len(keep) != k:
            raise ValueError('MissionTable: one next_ok, next_fail, start_here and keep_zaxis per entry, and at least one entry')

    @staticmethod
    def _fail(on_fail, j):
        return -1 if on_fail == 'stop' else j if on_fail == 'retry' else int(on_fail)

    @classmethod
    def chain(cls, entries, on_fail='stop', **kw):
        """entry 0, then 1, ... each after an arrival, the last one stops; on_fail: 'stop', 'retry' (the same entry again) or an index"""
        k = len(entries)
        return cls(entries, [j + 1 if j + 1 < k else -1 for j in range(k)], [cls._fail(on_fail, j) for j in range(k)],
                   first_ok=0, first_fail=cls._fail(on_fail, 0), **kw)

    @classmethod
    def cycle(cls, entries, on_fail='stop', **kw):
        """as chain, but the last entry is followed by entry 0 again"""
        k = len(entries)
        return cls(entries, [(j + 1) % k for j in range(k)], [cls._fail(on_fail, j) for j in range(k)], first_ok=0, first_fail=cls._fail(on_fail, 0), **kw)


class _KdTreeView:
    """Stand-in for mamp.policies.kdTree.KDTree: the tree itself lives on the device; the permutation the reference
    carries from step to step (kdTree.py:43-45) is readable."""

    def __init__(self, env):
        self._env = env
        self.max_leaf_size = 10

    @property
    def agentIDs(self):
        return list(self._env.solver.get_kd_perm())


# the solver attributes the reference keeps per Agent (agent.py:24-41) and its policies read per call (scaPolicy.py:95,112,272,302, util.py:8,17,
# orca3dPolicyOfficial.py:44,98,108, agent.py:87-99, mampenv.py:90-92): sca_params field -> (Agent attribute, type)
_ATTRS = dict(neighbor_dist=('neighborDist', float), max_neighbors=('maxNeighbors', int), time_step=('timeStep', float),
              time_horizon=('timeHorizon', float), max_speed=('maxSpeed', float), max_heading_change=('max_heading_change', float),
              dt_nominal=('dt_nominal', float))


def _planner_triple(a):
    """the planner's attributes (agent.turning_radius, agent.pitchlims: scaPolicy.py:95,272,302)"""
    return float(a.turning_radius), float(a.pitchlims[0]), float(a.pitchlims[1])


def _obstacle_arrays(obstacles):
    return (np.array([o.pos_global_frame for o in obstacles], dtype=np.float64).reshape(len(obstacles), 3),
            np.array([o.radius for o in obstacles], dtype=np.float64))


def _bind(agents, env):
    for a in agents:
        a._env = env
        a._row_pos = a._row_vel = a._row_heading = None        # (row views belong to the mirrors of the env they were made for)
        a.policy._env = env
        a.policy._agent_id = a.id


class _FlatAgents:
    """What MACAEnv and SceneBatch (scenes.py) share: a flat list of agents on one solver context -- the host mirrors, the hand-over of the
    agents' attributes, the device tracker's rule, the waypoint lists and the decoding of the neighbour lists."""

    def _create(self, flat, device, max_obstacles, obstacles=None, before_state=None):
        """Solver context for the agents of `flat`, in the order of calls a context wants: sca_create, the shared `obstacles` (None: the caller
        sets its own in `before_state`), the agents, per-agent attributes, before_state(), the state, the device tracker."""
        n = len(flat)
        self._flat = flat
        self._mirror = dict(pos=np.array([a._pos for a in flat], dtype=np.float64).reshape(n, 3),
                            vel=np.array([a._vel for a in flat], dtype=np.float32).reshape(n, 3),
                            heading=np.array([a._heading for a in flat], dtype=np.float64).reshape(n, 3),
                            flags=np.zeros(n, np.uint8), total_dist=np.zeros(n), step_num=np.zeros(n, np.int32))
        self._stale = False
        self.goal = np.array([a.goal_global_frame for a in flat], dtype=np.float64).reshape(n, 3)
        self.policy_ids = np.array([a.policy.policy_id for a in flat], np.uint8)
        self._ext = np.array([a.policy.needs_external_vpref for a in flat], bool)
        start = np.array([a.initial_pos for a in flat], dtype=np.float64)
        goal6 = np.array([a.goal_pos for a in flat], dtype=np.float64)
        # Attributes all agents agree on become the context's sca_params; the ones that differ from agent to agent go to the device as
        # per-agent arrays (sca_set_agent_params), the context keeping the first agent's value as its default.
        params, per_agent = {}, {}
        for name, (attr, conv) in _ATTRS.items():
            vals = [conv(getattr(a, attr)) for a in flat]
            params[name] = vals[0]
            if any(v != vals[0] for v in vals):
                per_agent[name] = vals
        sol = self.solver = S.BatchedSolver(max_agents=n, max_obstacles=max(max_obstacles, 1), device=device, params=params)
        if obstacles is not None:
            sol.set_obstacles(*_obstacle_arrays(obstacles))
        sol.set_agents([a.radius for a in flat], [a.pref_speed for a in flat], self.goal, self.policy_ids, S.zaxis_flags(start, goal6),
                       [a.max_run_dist for a in flat])
        if per_agent:
            sol.set_agent_params(**per_agent)
        if before_state is not None:
            before_state()
        sol.set_state(self._mirror['pos'], self._mirror['vel'], self._mirror['heading'], self._mirror['flags'])
        # the first tracked agent's planner attributes become the tracker's defaults, and where the tracked agents differ every agent's own go
        # over (classes of equal values on the device).  _trk_*: what a later agent of a slot is held against (SceneBatch.restart)
        self._trk_on, self._trk_first, self._trk_trip = False, None, None
        # (attribute_slots: a tracked drone may arrive later in a fleet that starts without one -- the tracker stands from the start)
        if self.device_tracker and (self._ext.any() or getattr(self, '_attr_slots', False)):
            trip = [_planner_triple(a) for a in flat]
            first = trip[int(np.argmax(self._ext))]
            sol.device_tracker_enable(goal6[:, 3:6], turning_radius=first[0], pitchlims=(first[1], first[2]))
            if any(t != first for t, ext in zip(trip, self._ext) if ext):
                sol.device_tracker_set_agent_params([t[0] for t in trip], [t[1] for t in trip], [t[2] for t in trip])
                self._trk_trip = trip
            self._trk_on, self._trk_first = True, first
        return sorted(per_agent)

    def _planner_of(self, i):
        """the planner attributes the device tracker holds for agent i"""
        return self._trk_first if self._trk_trip is None else self._trk_trip[i]

    def _reset_paths(self):
        self._paths_on = False          # waypoint lists on the device (Agent.path)
        self._path_stale = False        # ... and the host mirrors (agents' lists, _path_ng) behind it
        self._path_assigned = set(range(len(self._flat)))     # agents whose .path was assigned since the last upload
        self._path_ng = None
        self._sync_paths()
        self._nbr_cache = None
        self._vpref_cache = None

    # ---- host mirrors of the device state, refreshed in place on first use after a step (the reference's per-agent attributes) -------
    def _state(self, name):
        if self._stale:
            st = self.solver.get_state()
            for k in self._mirror:
                self._mirror[k][...] = st[k]
            self._stale = False
        return self._mirror[name]

    def _vpref_of(self, i):
        if self._vpref_cache is None:
            self._vpref_cache = np.nan_to_num(self.solver.diag()['vpref'])
        return self._vpref_cache[i]

    def _neighbors(self, i, agents, obstacles, lo=0, obs_lo=0):
        """[(object, distSq)] of agent i of the context; `agents` and `obstacles` start at the context's ids lo and obs_lo"""
        if self._nbr_cache is None:
            self._nbr_cache = self.solver.neighbors()
        nb = self._nbr_cache
        out = []
        for k in range(int(nb['nbr_n'][i])):
            j = int(nb['nbr_id'][i, k])
            obj = obstacles[j - obs_lo] if nb['nbr_kind'][i, k] else agents[j - lo]
            out.append((obj, float(nb['nbr_dsq'][i, k])))
        return out

    # ---- waypoint lists (Agent.path): uploaded when assigned, mirrored lazily -----------------------------------------------
    def _refresh_paths(self, skip=()):
        rem, self._path_ng = self.solver.get_path_state()
        for i, a in enumerate(self._flat):
            if i not in skip and len(a._path) > rem[i]:
                del a._path[int(rem[i]):]                         # what list.pop() from the end has left
        self._path_stale = False

    def _sync_paths(self):
        """Uploads the agents' lists when one was assigned since the last upload: the others keep their place and every now_goal its value."""
        if not self._path_assigned:
            return
        assigned, self._path_assigned = self._path_assigned, set()
        lists = self._path_lists()
        n = len(lists)
        if self._paths_on:
            self._refresh_paths(skip=assigned)
            ng = self._path_ng.copy()
        else:
            if not any(len(p) for p in lists) and not self._path_slots:
                return
            ng = np.full((n, 3), np.nan)
            served = self._state('step_num') > 0                   # agents that ran get_trajectory already hold now_goal = goal
            ng[served] = self.goal[served]
        self._lists_set = [[list(map(float, w[:3])) for w in p] for p in lists]     # as the device holds them (block form: what a checkpoint's definition keeps)
        self._upload_paths(self._lists_set)
        self.solver.set_path_state(np.array([len(p) for p in lists], np.int32), ng)
        self._paths_on = True
        self._path_ng = ng
        self._path_stale = False

    _path_slots = 0                      # SceneBatch(path_slots=W): the lists live in slot form, from the start and with no list at all

    def _path_lists(self):
        return [a._path for a in self._flat]

    def _upload_paths(self, lists):
        self.solver.set_paths(lists)

    def _now_goal_of(self, i):
        if self._path_stale:
            self._refresh_paths()
        g = self._path_ng[i]
        return None if np.isnan(g[0]) else g.copy()


class MACAEnv(_FlatAgents):
    def __init__(self, v_pref_fn=None, device=0, neighbor_mode=S.NBR_KDTREE, history_capacity=0, device_tracker=False, clearance=False,
                 path_slots=0, attribute_slots=False):
        self.agents = None
        self._attr_slots = bool(attribute_slots)       # respawn() takes agents whose policy or solver attributes differ from the row's
                                                       # (sca_respawn_agents_attrs; SceneBatch's name for the same thing)
        self._path_slots = int(path_slots)             # W > 0: the waypoint lists live in slot form (sca_set_path_slots), room for W per agent --
                                                       # what respawn() needs to give one agent a new list while the others keep theirs
        self.clearance_on = bool(clearance)            # every step also keeps each agent's closest approach (sca_clearance_enable): env.clearance
        self.obstacles = []
        self.kdTree = None
        self.solver = None
        self.v_pref_fn = v_pref_fn
        self.device_tracker = bool(device_tracker)     # SCA / RVO3D+Dubins v_pref from the tracker kernels inside every pass
        if self.device_tracker and v_pref_fn is not None:
            raise ValueError('device_tracker=True and v_pref_fn are alternatives')
        self.dubins_tracker = v_pref_fn is not None or self.device_tracker
        self.device = device
        self.neighbor_mode = neighbor_mode
        self.history_capacity = history_capacity      # env steps of Agent.history_info kept on the device (0: no log);
        self.history_budget_bytes = 64 << 30          # 64 B per agent per step, allocated up front: capped to this budget
        self._row_cache = None
        self._last_neighbors = None     # neighbour lists of the previous policy pass (read by the v_pref tracker)
        self._time_cum = [0.0]          # [s] = seconds of policy wall time per served agent over the first s env steps
        self._active = 0                # agents the next step will serve
        self._vpref_cache = None
        self._paths_on = False
        self._path_stale = False
        self._path_assigned = set()
        self._missions = None           # the tables of set_missions (None: none stand)
        self._mission_gate = False      # set_missions(spawn_margin=): the admission gate on the device
        self._mission_pending = {}      # ... id -> (entry, where the flight that named it ended): named, not known to be admitted yet
        self._mission_args = None       # (results, spawn_margin, max_per_step) of set_missions: what a checkpoint keeps beside the tables

    def set_agents(self, agents, obstacles=None):
        if obstacles is None:
            raise TypeError('obstacles must be a list (the reference crashes on None too, kdTree.py:48)')
        for i, a in enumerate(agents):
            if a.id != i:
                raise ValueError('agent.id must equal its list index (kdTree.py:64)')
        self.agents = agents
        self.obstacles = obstacles
        self._missions = None           # (a new agent set drops the mission tables, here as in the library)
        self._mission_gate, self._mission_pending = False, {}
        n = len(agents)
        # which attributes the agents disagree on (empty: one value per context)
        self.per_agent_attributes = self._create(agents, self.device, len(obstacles), obstacles)
        if self._trk_trip is not None:
            self.per_agent_attributes = sorted(self.per_agent_attributes + ['turning_radius / pitchlims'])
        _bind(agents, self)
        self._reset_paths()
        self.kdTree = _KdTreeView(self)
        self._row_cache = None
        self._time_cum = [0.0]
        self._active = n
        # the log costs 64 B x rows x agents of HBM up front: cap it to a budget instead of failing in hipMalloc
        if self.history_capacity and 64 * self.history_capacity * n > self.history_budget_bytes:
            capped = max(1, self.history_budget_bytes // (64 * n))
            import warnings
            warnings.warn(f'history_capacity {self.history_capacity} x {n} agents x 64 B exceeds the {self.history_budget_bytes >> 30} GiB '
                          f'budget: keeping the first {capped} env steps (later steps are counted as dropped)')
            self.history_capacity = capped
        if self.history_capacity:
            self.solver.history_enable(self.history_capacity)
        if self.clearance_on:
            self.solver.clearance_enable()

    @property
    def clearance(self):
        """The closest-approach records of the episode so far (MACAEnv(clearance=True)): one record per agent in sca_scene_clearance's
        layout (_lib.CLEARANCE_DTYPE), partners are agent ids and indices into the obstacle list, `step` counts env.step() calls from 1.
        metrics.clearance_metrics(env) reads them."""
        if not self.clearance_on:
            raise RuntimeError('clearance: a MACAEnv(clearance=True) keeps the closest approach per agent; this one was built without')
        if self._row_cache is not None:
            raise RuntimeError('clearance: between a policy pass and its env update (agent.find_next_action was called): env.step() first')
        return self.solver.clearance()

    def _upload_paths(self, lists):
        if not self._path_slots:
            return super()._upload_paths(lists)
        for i, p in enumerate(lists):
            if len(p) > self._path_slots:
                raise ValueError(f'agent {i} has a path of {len(p)} waypoints, MACAEnv(path_slots={self._path_slots}) has room for {self._path_slots}')
        self.solver.set_path_slots(self._path_slots, lists)

    # ---- new missions without redefining the swarm (sca_respawn_agents / sca_get_finished) ---------------------------------
    def probe(self, pos, radius, ignore=None):
        """How free is each point now (sca_probe_clearance): spheres of `radius` at `pos` (Q, 3) against every agent where it stands --
        but ignore[q], None or -1: nobody is excluded -- and every obstacle.  A structured array of _lib.CLEARANCE_DTYPE (agent_clear,
        obs_clear, agent_partner, obs_partner; an empty half is +inf, -1).  Between two env.step() calls; changes nothing."""
        if self.agents is None:
            raise RuntimeError('probe: set_agents first')
        if self._row_cache is not None:
            raise RuntimeError('probe: between a policy pass and its env update (agent.find_next_action was called): env.step() first')
        return self.solver.probe_clearance(pos, radius, ignore)

    def respawn(self, agents, margin=None):
        """New missions for some agents while everybody else flies on: each Agent of `agents` replaces env.agents[agent.id] -- the
        reference's rule for assigning pos_global_frame, goal_global_frame, is_at_goal = False, ... to an Agent object between two
        env.step() calls.  Start, goal, velocity, radius, pref_speed, max_run_dist, goal heading, path and the z-axis flag are read off
        the agent as set_agents reads them; the row keeps its policy and its per-agent attributes, so an agent whose policy or
        attributes differ from the row's is a ValueError, raised before any device call.  A path needs MACAEnv(path_slots=W).
        MACAEnv(attribute_slots=True): the arriving agent brings its own policy, solver attributes and, under the device tracker, its
        turning_radius / pitchlims (sca_respawn_agents_attrs) -- an ORCA3D row can be re-entered by a Dubins-tracked SCA drone with
        another neighborDist and turning radius; env.agents[i], policy_ids, per_agent_attributes and the v_pref and planner mirrors
        follow the admitted agents.
        margin (None: no gate, returns None): only the agents whose start is free by `margin` metres are admitted
        (sca_respawn_agents_gated: clear of every other agent where it stands now, of every obstacle, and of the admitted agents earlier
        in `agents`); they replace their rows and are returned as a list, `last_spawn` holds (verdict, probe) of the call; a refused
        agent leaves env.agents and its row untouched."""
        if self.agents is None:
            raise RuntimeError('respawn: set_agents first')
        if self._row_cache is not None:
            raise RuntimeError('respawn: between a policy pass and its env update (agent.find_next_action was called): env.step() first')
        agents = list(agents)
        if not agents:
            return None if margin is None else []
        n = len(self.agents)
        ids = [int(a.id) for a in agents]
        if min(ids) < 0 or max(ids) >= n or len(set(ids)) != len(ids):
            raise ValueError('respawn: agent.id names a row of this env, 0 .. %d, and no row twice' % (n - 1))
        for a in agents:
            old = self.agents[a.id]
            ext = bool(a.policy.needs_external_vpref) if self._attr_slots else bool(self._ext[a.id])
            if not self._attr_slots:
                if a.policy.policy_id != old.policy.policy_id:
                    raise ValueError(f'respawn: agent {a.id} has policy {type(a.policy).__name__}, the row runs {type(old.policy).__name__} (a row keeps its policy)')
                for attr, conv in _ATTRS.values():
                    if conv(getattr(a, attr)) != conv(getattr(old, attr)):
                        raise ValueError(f'respawn: agent {a.id} has {attr} = {getattr(a, attr)}, the row has {getattr(old, attr)} (a row keeps its attributes)')
            if not self._attr_slots and self._trk_on and ext and _planner_triple(a) != self._planner_of(a.id):
                raise ValueError(f'respawn: agent {a.id} has turning_radius / pitchlims {_planner_triple(a)}, the row has {self._planner_of(a.id)}')
            if self.v_pref_fn is not None and ext:
                raise ValueError(f'respawn: agent {a.id} takes v_pref from the host-side v_pref_fn, whose per-agent state the env cannot reset '
                                 '(use MACAEnv(device_tracker=True))')
            if len(a._path) > self._path_slots:
                raise ValueError(f'respawn: agent {a.id} brings a path of {len(a._path)} waypoints: MACAEnv(path_slots=W) with W >= that keeps '
                                 'the lists in slot form, where one agent\'s list can be replaced')
        if self._paths_on and not self._path_slots:
            raise ValueError('respawn: the env follows waypoint lists in block form; MACAEnv(path_slots=W) keeps them in slot form, where one '
                             'agent\'s list can be replaced')
        self._sync_paths()                                      # lists assigned since the last step go up first
        was_done = (self._state('flags')[ids] & 7) != 0
        start = np.array([a.initial_pos for a in agents], dtype=np.float64)
        goal6 = np.array([a.goal_pos for a in agents], dtype=np.float64)
        lists = [[list(map(float, w[:3])) for w in a._path] for a in agents] if self._paths_on else None
        got = self.solver.respawn(ids, [a._pos for a in agents], [a._vel for a in agents], [a._heading for a in agents], [a.radius for a in agents],
                                  [a.pref_speed for a in agents], goal6[:, :3], [a.max_run_dist for a in agents], zaxis=S.zaxis_flags(start, goal6),
                                  goal_heading=goal6[:, 3:6] if self._trk_on else None, paths=lists, margin=margin, **self._brings(agents))
        if margin is not None:
            self.last_spawn = got
            admitted = got[0] == S.SPAWN_ADMITTED
            agents = [a for a, ok in zip(agents, admitted) if ok]
            was_done = was_done[admitted]
            if not agents:
                return []
        for a in agents:
            if self.agents[a.id] is not a:
                self.agents[a.id]._env = None                    # (the replaced object reads its own attributes again)
            self.agents[a.id] = a
            self.goal[a.id] = a.goal_global_frame
            self._mission_pending.pop(a.id, None)                # (a mission gate: the row's pending mission is gone with this respawn)
            self._path_assigned.discard(a.id)
            if self._attr_slots:                                 # the mirrors follow the admitted agents only
                self.policy_ids[a.id] = a.policy.policy_id
                self._ext[a.id] = bool(a.policy.needs_external_vpref)
                if self._trk_on and (self._trk_trip is not None or (self._ext[a.id] and _planner_triple(a) != self._trk_first)):
                    if self._trk_trip is None:
                        self._trk_trip = [self._trk_first] * len(self.agents)
                    self._trk_trip[a.id] = _planner_triple(a)
        if self._attr_slots:
            differ = [name for name, (attr, conv) in _ATTRS.items() if len({conv(getattr(b, attr)) for b in self.agents}) > 1]
            self.per_agent_attributes = sorted(differ + (['turning_radius / pitchlims'] if self._trk_trip is not None else []))
        _bind(agents, self)
        self._active += int(was_done.sum())
        self._stale = True
        self._path_stale = self._paths_on
        self._nbr_cache = None
        self._vpref_cache = None
        return None if margin is None else agents

    def _brings(self, agents):
        """what respawn() hands BatchedSolver.respawn beside the missions: nothing, or with attribute_slots the agents' policies and a full
        row of solver attributes each and, under the device tracker, of planner attributes"""
        if not self._attr_slots:
            return {}
        attrs = {name: [conv(getattr(a, attr)) for a in agents] for name, (attr, conv) in _ATTRS.items()}
        if self._trk_on:
            trip = [_planner_triple(a) for a in agents]
            attrs.update(turning_radius=[t[0] for t in trip], pitch_lo=[t[1] for t in trip], pitch_hi=[t[2] for t in trip])
        return dict(policy=[a.policy.policy_id for a in agents], attrs=attrs)

    def finished(self, capacity=None):
        """The rows that carry any of at-goal / collision / timeout, ascending ids, compacted on the device (sca_get_finished): a
        structured array of _lib.FINISHED_DTYPE (id, flags, step_num, total_dist, pos).  Vacant rows are not among them."""
        return self.solver.finished(capacity)

    def retire(self, agents):
        """The drones leave the airspace (sca_retire_agents): `agents` are Agent objects of this env or row ids, occupied, live or finished.
        Their rows become vacant -- env.agents keeps the objects, which read is_vacant, flags 11, zero velocity and heading -- and are
        nobody's neighbour, collision, clearance or probe partner any more; everybody else flies on untouched.  respawn() with an Agent
        whose id is a vacant row admits a drone there.  At least one row stays occupied."""
        if self.agents is None:
            raise RuntimeError('retire: set_agents first')
        if self._row_cache is not None:
            raise RuntimeError('retire: between a policy pass and its env update (agent.find_next_action was called): env.step() first')
        ids = [int(getattr(a, 'id', a)) for a in agents]
        if not ids:
            return
        n = len(self.agents)
        if min(ids) < 0 or max(ids) >= n or len(set(ids)) != len(ids):
            raise ValueError('retire: a row of this env, 0 .. %d, and no row twice' % (n - 1))
        self._sync_paths()
        live = (self._state('flags')[ids] & 7) == 0
        self.solver.retire(ids)
        for i in ids:
            self._mission_pending.pop(i, None)
            self._path_assigned.discard(i)
        self._active -= int(live.sum())
        self._stale = True
        self._path_stale = self._paths_on
        self._nbr_cache = None
        self._vpref_cache = None

    @property
    def vacant(self):
        """the vacant rows' ids, ascending (sca_get_vacant)"""
        return self.solver.vacant()

    @property
    def population(self):
        """the occupied rows (sca_get_population)"""
        return self.solver.population()

    # ---- mission tables: finished rows take their next mission inside the step (sca_set_missions) ---------------------------
    def set_missions(self, tables, results=4, spawn_margin=None, max_per_step=None):
        """tables: a dict from agent id to a MissionTable (rows that are not named have no table); results: the room of every row's
        result ring -- at least the endings a row can have between two mission_results() calls.  From now on a row that ends inside a
        step takes the successor its table names there, by respawn()'s rule and without a host round trip, so run_steps(k) runs
        traffic; a row whose ended flight names no successor stays finished (finished() lists it, respawn() may restart it).  The
        entries are read off Agent-like objects as respawn() reads them; a row keeps its radius, its policy and its attributes, so an
        entry whose policy differs from the row's is a ValueError.  None or {} drops the tables.
        An entry's zaxis byte (start and goal share x and y) is worked out from the entry's OWN start and goal, as respawn() does.  For a
        start_here entry that is its nominal start (the Agent-like object's initial_pos), not the spot the row will stand on when it
        takes the entry, which nobody knows yet: where the two may differ in x or y by more than the rule's 1e-5, give the entry
        keep_zaxis, or a nominal start that says what the leg is.
        spawn_margin (metres): the admission gate on the device (sca_set_mission_gate) -- a row takes its successor only where the
        start is free by that margin, as respawn(margin=) decides it; a refused row stays finished and is offered again behind every
        step, waiting rows first.  max_per_step: the candidates tested per step (None: min(n, 4096)).
        Routes: an entry's waypoint list (MissionTable(path=...) or the entry's own Agent.path) needs MACAEnv(path_slots=W) -- a row that
        takes the entry gets the list as under respawn() (sca_set_missions_paths); a list above W is a ValueError before any device
        call.  mission_results() then sets agent.path to the taken entry's list, cut to what the passes since have left of it.  While
        such tables stand agent.path is read-only: assigning it raises a RuntimeError (drop the tables first)."""
        if self.agents is None:
            raise RuntimeError('set_missions: set_agents first')
        if self._row_cache is not None:
            raise RuntimeError('set_missions: between a policy pass and its env update (agent.find_next_action was called): env.step() first')
        if not tables:
            self.solver.set_missions(0, 0, None, None, None)
            self._missions = None
            self._mission_gate, self._mission_pending = False, {}
            return
        n = len(self.agents)
        M = max(len(t.entries) for t in tables.values())
        e = np.zeros((n, M), _lib.MISSION_DTYPE)
        e['pref_speed'] = e['max_run_dist'] = 1.0                     # (rows and slots nobody reaches: legal values, never read)
        e['next_ok'] = e['next_fail'] = -1
        first_ok, first_fail = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        lists = {}                                                    # MACAEnv(path_slots=W): (row, entry) -> the entry's waypoint list
        for i, t in tables.items():
            if not 0 <= int(i) < n:
                raise ValueError('set_missions: %r names no row of this env, 0 .. %d' % (i, n - 1))
            old = self.agents[i]
            for j, (a, here, keep) in enumerate(t.entries):
                if a.policy.policy_id != old.policy.policy_id:
                    raise ValueError(f'set_missions: entry {j} of agent {i} has policy {type(a.policy).__name__}, the row runs {type(old.policy).__name__} (a row keeps its policy)')
                if len(t.paths[j]) > self._path_slots:
                    raise ValueError(f'set_missions: entry {j} of agent {i} brings a path of {len(t.paths[j])} waypoints: MACAEnv(path_slots=W) with W >= that '
                                     'keeps the lists in slot form, where a row that takes an entry gets the entry\'s list')
                if self._path_slots:
                    lists[(int(i), j)] = t.paths[j]
                start, goal6 = np.asarray(a.initial_pos, np.float64), np.asarray(a.goal_pos, np.float64)
                r = e[i, j]
                r['pos'], r['heading'], r['goal'], r['goal_heading'], r['vel'] = a._pos, a._heading, goal6[:3], goal6[3:6], a._vel
                r['pref_speed'], r['max_run_dist'] = a.pref_speed, a.max_run_dist
                r['zaxis'] = S.zaxis_flags(start[None, :], goal6[None, :])[0]
                r['flags'] = (S.MISSION_START_HERE if here else 0) | (S.MISSION_KEEP_ZAXIS if keep else 0)
                r['next_ok'], r['next_fail'] = t.next_ok[j], t.next_fail[j]
            first_ok[i], first_fail[i] = t.first_ok, t.first_fail
        if self._path_slots:                                          # the lists live in slot form: every entry brings its list, the empty one too
            self._sync_paths()                                        # (lists assigned since the last step go up first: the flight in the air keeps its own)
            self.solver.set_missions(M, int(results), e, first_ok, first_fail, paths=lists)
        else:
            self.solver.set_missions(M, int(results), e, first_ok, first_fail)
        self._missions = dict(tables)
        self._mission_args = (int(results), spawn_margin, max_per_step)
        self._mission_gate, self._mission_pending = spawn_margin is not None, {}
        if self._mission_gate:
            self.solver.set_mission_gate(spawn_margin, 0 if max_per_step is None else int(max_per_step))

    def mission_results(self):
        """The results not yet collected (sca_get_mission_results): a structured array of _lib.MISSION_RESULT_DTYPE, ascending id and
        within a row oldest first.  env.agents[i]'s goal / start mirrors move to the entry the row flies now (the Agent object stays:
        its state views read the device)."""
        if self._missions is None:
            raise RuntimeError('mission_results: no mission tables are set -- set_missions first')
        res = self.solver.mission_results()
        if self._mission_gate:
            # A named successor may still be waiting: a row's mirrors move when it is ADMITTED.  The results are in ascending id and within
            # a row oldest first, and a waiting row cannot end: a row that ended again was admitted in between (a self-successor too, whose
            # cursor does not change), and the last named entry of a row was admitted if the row does not wait now.  A start_here entry
            # starts where the flight that named it ended.
            moved, pending = [], self._mission_pending
            for r in res:
                i = int(r['id'])
                if i in pending:
                    moved.append((i,) + pending.pop(i))
                if int(r['next']) >= 0:
                    pending[i] = (int(r['next']), r['pos'].copy())
            if pending:
                waiting = self.solver.mission_gate_state()[0]
                for i in sorted(pending):
                    if waiting[i] < 0:
                        moved.append((i,) + pending.pop(i))
        else:
            moved = [(int(r['id']), int(r['next']), r['pos']) for r in res]
        for i, j, pos in moved:
            if j < 0:
                continue
            r = dict(pos=pos)
            a, (src, here, _) = self.agents[i], self._missions[i].entries[j]
            a.goal_pos, a.goal_global_frame, a.goal_heading_frame = src.goal_pos.copy(), src.goal_global_frame.copy(), src.goal_heading_frame.copy()
            a.initial_pos = np.concatenate([r['pos'], a.initial_pos[3:]]) if here else src.initial_pos.copy()
            a.pref_speed, a.max_run_dist = src.pref_speed, src.max_run_dist
            self.goal[i] = a.goal_global_frame
            if self._path_slots:                                      # the entry's whole list; the next read cuts it to what the passes since have left
                a._path = [list(w) for w in self._missions[i].paths[j]]
                self._path_assigned.discard(i)
        if len(res) or moved:
            self._stale = True
            self._path_stale = self._paths_on
        return res

    # ---- context checkpoints: the running env out as one object, and back as a fresh env (sca_save_context / sca_load_context) ------------
    def checkpoint(self):
        """The env as it stands between two env.step() calls, as a checkpoint.ContextCheckpoint: the definition -- the agents with every
        attribute, the obstacles, the env's options, the waypoint lists, the mission tables with their lists, results room and gate -- as
        plain arrays, the library's blob of the context's whole mutable state (sca_save_context) and the steps so far.
        MACAEnv.from_checkpoint() resumes it in this or another process; write(path) / read(path) keep it as one .npz without pickle.
        Not kept: the trajectory log (a resumed env's log starts at its own row 0) and a host-side v_pref_fn's state (a RuntimeError)."""
        from . import checkpoint as _ck
        return _ck.env_checkpoint(self)

    @classmethod
    def from_checkpoint(cls, ckpt, device=0):
        """A fresh MACAEnv that is bit for bit the env ckpt was taken from, from there on: the definition set up, the blob loaded.  Its
        `agents` mirrors (start, goal, radius, pref_speed, path, flags, position ...) show the checkpoint's values at once; mission tables
        stand as they stood, so lifelong.run_missions(env, None, steps) goes on with them."""
        from . import checkpoint as _ck
        return _ck.env_from_checkpoint(cls, ckpt, device)

    def run_steps(self, k):
        """k resident steps in one library call (sca_run_steps) and one synchronisation; with mission tables set the rows that end on
        the way take their next missions there.  Returns the number of running agents."""
        import time
        if self._row_cache is not None or self.v_pref_fn is not None:
            raise RuntimeError('run_steps: the steps are resident -- not between a policy pass and its env update, not with a host-side v_pref_fn')
        self._sync_paths()
        t0 = time.perf_counter()
        served = max(1, self._active)
        self.solver.run_steps(int(k), self.neighbor_mode)
        self._active = self.solver.active_count()                  # (synchronises: the burst is over when this returns)
        per_step = (time.perf_counter() - t0) / max(1, int(k)) / served
        for _ in range(int(k)):
            self._time_cum.append(self._time_cum[-1] + per_step)
        self._stale = True
        self._path_stale = self._paths_on
        self._nbr_cache = None
        self._vpref_cache = None
        return self._active

    pos = property(lambda self: self._state('pos'))
    vel = property(lambda self: self._state('vel'))
    heading = property(lambda self: self._state('heading'))
    flags = property(lambda self: self._state('flags'))
    total_dist = property(lambda self: self._state('total_dist'))
    step_num = property(lambda self: self._state('step_num'))

    # ---- one step = MACAEnv.step (mampenv.py:22-25) ---------------------------------------------------------------------
    def _policy_pass(self):
        self._sync_paths()
        if self._row_cache is None:
            if self.v_pref_fn is not None and self._ext.any():
                vp = np.asarray(self.v_pref_fn(self), dtype=np.float64).reshape(len(self.agents), 3)
                self.solver.set_vpref(vp, self._ext.astype(np.uint8))
            self.solver.policy_pass(self.neighbor_mode)
            self._path_stale = self._paths_on
            self._row_cache = self.solver.actions()
            self._nbr_cache = None
            if self.v_pref_fn is not None:
                self._nbr_cache = self._last_neighbors = self.solver.neighbors()
            self._stale = True                                    # is_collision set inside insert*Neighbor (agent.py:84)
        return self._row_cache

    @property
    def all_actions(self):
        """The [N, 7] float32 action rows of the last step (the reference's `all_actions` inside _take_action, mampenv.py:31,40): read back
        from the device when asked for."""
        if self._row_cache is not None:
            return self._row_cache
        return self.solver.actions()

    def _policy_row(self, i):
        return list(self._policy_pass()[i])

    def _neighbors_of(self, i):
        return self._neighbors(i, self.agents, self.obstacles)

    def step(self, actions=None):
        """`actions` is ignored, as in the reference (mampenv.py:22).  Without a host-side v_pref_fn the whole step (both loops
        of _take_action, mampenv.py:27-49) is one resident library call and nothing but the done count comes back: the
        per-agent attributes are read from the device the next time somebody looks at them."""
        import time
        self._sync_paths()
        t0 = time.perf_counter()
        served = max(1, self._active)
        if self._row_cache is None and self.v_pref_fn is None:
            self._active = self.solver.env_step(self.neighbor_mode)   # one call; synchronises: the step is over when this returns
            t_policy = time.perf_counter() - t0
            done = self._active == 0
            self._nbr_cache = None
        else:
            self._policy_pass()
            t_policy = time.perf_counter() - t0                  # the reference times find_next_action only
            done = self.solver.env_update()
            self._active = self.solver.active_count()
        self._time_cum.append(self._time_cum[-1] + t_policy / served)
        self._stale = True
        self._path_stale = self._paths_on
        self._row_cache = None
        self._vpref_cache = None
        return done


def build_circle_agents(n, policy=RVO3DPolicy, rad=None, radius=0.5, pref_speed=1.0):
    """run_example/run_sca.py:106-126 build_agents for the circle scenario."""
    sc = _sc.circle(n, rad=rad)
    return [Agent(start_pos=list(sc['start'][i]), goal_pos=list(sc['goal'][i]), vel=[0.0, 0.0, 0.0], radius=radius,
                  pref_speed=pref_speed, policy=policy, id=i, dt=DT) for i in range(n)]
