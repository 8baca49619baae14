"""SceneBatch: many isolated episodes stepped by ONE library context (include/sca_hip.h, sca_set_scenes).

The reference's users run many small episodes -- a paper's table is policies x scenarios x seeds, each a scene of 14-100 drones -- and a small
scene alone is a chain of dependent dispatches, not work for the chip.  A SceneBatch holds B such scenes in one context: every scene has its
own kd-tree, its own carried permutation and its own `done`, agents of different scenes never meet, and every value of a scene is bit for
bit what a MACAEnv holding that scene alone produces.  Obstacles are either one list shared by all scenes (`obstacles`) or one list per
scene (`scene_obstacles`, sca_set_scene_obstacles): then every scene meets its own obstacles and no others -- an open circle, a take-off
field with its spheres and two seeds of an obstacle scenario share one batch -- and is still bit for bit the MACAEnv of that scene alone.
With `obstacle_capacities` a scene's obstacle range is a capacity too (sca_set_scene_obstacle_slots): SceneBatch.restart(..., obstacles=...)
then brings a new episode's own obstacles into the slot, and run_episodes(episode_obstacles=...) streams a queue whose episodes differ in
their obstacles.  With `path_slots` the waypoint lists (Agent.path) live in slot form -- room for W waypoints per agent row
(sca_set_path_slots) -- and SceneBatch.restart / run_episodes(path_slots=...) bring every episode's own lists into the slot it takes.
With `clearance=True` the device keeps every agent's closest approach with the step (sca_scene_clearance_enable): `batch.env(s).clearance`
is the scene's record, metrics.clearance_metrics(batch.env(s)) the table's missing column -- how close the drones came.

    batch = SceneBatch([build_agents(seed) for seed in seeds], obstacles, device_tracker=True)   # each list numbered 0 .. n_s - 1
    while not batch.step():
        pass
    rows = [metrics.episode_metrics(batch.env(s)) for s in range(len(batch))]

    batch = SceneBatch(scenes, scene_obstacles=[[], spheres, other_spheres], device_tracker=True)     # one list of Obstacle per scene

`batch.env(s)` is a view with the surface the reference's callers and sca_amd.metrics read of a MACAEnv: `.agents`, `.obstacles` (the
scene's own list where there is one per scene), `.kdTree.agentIDs` (scene-local ids); the agents' attributes (pos_global_frame, is_at_goal, total_dist, path, policy.now_goal, ...) read the
batch's host mirrors at offsets[s] + id.  With `capacities` a scene's range is a capacity: the slot holds any episode of 1 .. capacity agents in
the first rows of its range (SceneBatch.restart takes any such episode), and the view follows the episode's size.  A host-side v_pref_fn is not supported: SCA / RVO3D+Dubins agents take v_pref from the device
tracker (device_tracker=True), or from the straight-line rule without it, as in MACAEnv.
"""
import copy
import time

import numpy as np

from . import metrics
from . import solver as S
from . import env as _env
from .env import _ATTRS, _FlatAgents, _bind, _obstacle_arrays, _planner_triple


class _SceneKdTree:
    """kdTree.agentIDs of one scene, in the scene's own ids (the context carries global ids: offsets[s] + these)"""

    def __init__(self, view):
        self._view = view
        self.max_leaf_size = 10

    @property
    def agentIDs(self):
        v = self._view
        return list(v._batch.solver.get_kd_perm()[v._lo:v._hi] - v._lo)


class _SceneLog:
    """What sca_amd.metrics reads of an env's `.solver`: the trajectory log of ONE scene, in the scene's own agents (sca_scene_history_*)"""

    def __init__(self, view):
        self._view = view

    def history_rows(self):
        rows = self._view._batch.solver.scene_history_rows()
        return int(rows['logged'][self._view.scene]), int(rows['dropped'][self._view.scene])

    def history(self, first_row=0, nrows=None, agent_begin=0, agent_count=None):
        """(a scene resumed from a SceneCheckpoint: the rows of the steps before the save are the checkpoint's, stitched in front of the
        device's -- the library restores the step count and goes on writing behind them)"""
        head = self._view._log_head
        sol, s = self._view._batch.solver, self._view.scene
        if head is None:
            return sol.scene_history(s, first_row, nrows, agent_begin, agent_count)
        k = len(head['pos'])
        if nrows is None:
            nrows = self.history_rows()[0] - first_row
        if agent_count is None:
            agent_count = len(self._view.agents) - agent_begin
        end, cols = first_row + nrows, slice(agent_begin, agent_begin + agent_count)
        saved = {key: v[first_row:min(k, end), cols] for key, v in head.items()}
        if end <= k:
            return saved
        live = sol.scene_history(s, max(first_row, k), end - max(first_row, k), agent_begin, agent_count)
        return {key: np.concatenate([saved[key], live[key]]) for key in live}


class _Assigned:
    """agent.path = [...] after the batch was built: the batch uploads the lists in front of its next step"""

    def __init__(self, view):
        self._view = view

    def add(self, i):
        self._view._batch._path_assigned.add(self._view._lo + i)


class SceneEnv:
    """One scene of a SceneBatch with a MACAEnv's read surface.  Agents index it with their scene-local id."""

    def __init__(self, batch, s, agents, lo, hi):
        self._batch, self.scene, self._lo = batch, s, lo
        self._obs_lo = 0 if batch.scene_obstacles is None else int(batch.obstacle_offsets[s])      # the context's obstacle ids are global
        self.obstacles = batch.obstacles if batch.scene_obstacles is None else batch.scene_obstacles[s]    # (restart(obstacles=...) replaces the list)
        self.kdTree = _SceneKdTree(self)
        self._occupy(agents, hi)
        self._time_cum = [0.0]
        self._log_head = None                                       # the log rows a SceneCheckpoint brought (restart({s: checkpoint}))
        self._clear_head = None                                     # ... and the closest-approach records of the steps before its save
        self._path_assigned = _Assigned(self)
        self.device_tracker = batch.device_tracker
        self.solver = _SceneLog(self)                               # (metrics.trajectories / write_episode_log: needs SceneBatch(scene_history=rows))

    def _occupy(self, agents, hi):
        """the episode the slot holds: rows [lo, hi) of the batch's arrays, the first len(agents) of the slot's capacity"""
        self.agents, self._hi = agents, hi
        self._mirror = {k: v[self._lo:hi] for k, v in self._batch._mirror.items()}       # views: refreshed in place by the batch
        self.goal = self._batch.goal[self._lo:hi]

    @property
    def per_agent_attributes(self):
        """the attributes the episode's agents disagree on, in MACAEnv.per_agent_attributes' names (read from the agents the slot holds now)"""
        out = [name for name, (attr, conv) in _ATTRS.items() if len({conv(getattr(a, attr)) for a in self.agents}) > 1]
        if self._batch._trk_on and len({_planner_triple(a) for a in self.agents if a.policy.needs_external_vpref}) > 1:
            out.append('turning_radius / pitchlims')
        return sorted(out)

    _stale = property(lambda self: self._batch._stale)
    _paths_on = property(lambda self: self._batch._paths_on)
    _path_stale = property(lambda self: self._batch._path_stale)

    def _state(self, name):
        self._batch._state(name)
        return self._mirror[name]

    pos = property(lambda self: self._state('pos'))
    vel = property(lambda self: self._state('vel'))
    heading = property(lambda self: self._state('heading'))
    flags = property(lambda self: self._state('flags'))
    total_dist = property(lambda self: self._state('total_dist'))
    step_num = property(lambda self: self._state('step_num'))
    done = property(lambda self: bool(self._batch.done[self.scene]))
    steps = property(lambda self: int(self._batch.steps[self.scene]))

    @property
    def clearance(self):
        """The episode's closest-approach records so far (SceneBatch(clearance=True)): one record per agent in sca_scene_clearance's layout
        (_lib.CLEARANCE_DTYPE), partners and steps in the scene's own terms.  A scene resumed from a SceneCheckpoint: the checkpoint's
        record merged with the device's (metrics.merge_clearance), which is the uninterrupted episode's."""
        if not self._batch.clearance:
            raise RuntimeError('clearance: a SceneBatch(clearance=True) keeps the closest approach per agent; this one was built without')
        rec = self._batch.solver.scene_clearance(self.scene)
        return rec if self._clear_head is None else metrics.merge_clearance(self._clear_head, rec)

    def _refresh_paths(self):
        self._batch._refresh_paths()

    def _now_goal_of(self, i):
        return self._batch._now_goal_of(self._lo + i)

    def _vpref_of(self, i):
        return self._batch._vpref_of(self._lo + i)

    def _policy_row(self, i):
        raise RuntimeError('a SceneBatch serves every agent of every scene in batch.step(): there is no single-agent find_next_action')

    def _neighbors_of(self, i):
        return self._batch._neighbors(self._lo + i, self.agents, self.obstacles, self._lo, self._obs_lo)


_POLICIES = {c.policy_id: c for c in (_env.SCAPolicy, _env.RVO3DPolicy, _env.SRVO3DPolicy, _env.ORCA3DPolicy, _env.ORCA3DPolicyOfficial,
                                      _env.RVO3dDubinsPolicy)}
_AGENT_SCALARS = ('radius', 'pref_speed', 'turning_radius', 'maxNeighbors', 'neighborDist', 'timeStep', 'timeHorizon', 'maxSpeed', 'dt_nominal',
                  'min_heading_change', 'max_heading_change', 'max_run_dist', 'group')


class SceneCheckpoint:
    """A running episode out of its slot (SceneBatch.checkpoint(s)): the episode's DEFINITION -- its agents and obstacles, as plain arrays
    an Agent / Obstacle is rebuilt from through its constructor --, the library's blob of the scene's mutable state (sca_save_scenes),
    `steps`, when the batch keeps a log per scene, the log rows so far, and, when it keeps the closest approach per agent, the record so
    far.  SceneBatch.restart({s: checkpoint}) resumes it in any slot of any batch that could take the episode; write(path) / read(path)
    keep it as one .npz of plain arrays (no pickle; a file written without the record still reads)."""

    def __init__(self, definition, blob, steps, log=None, time_cum=(0.0,), clearance=None):
        self.definition = {k: np.asarray(v) for k, v in definition.items()}
        self.blob = np.ascontiguousarray(blob, np.uint8)
        self.steps = int(steps)
        self.log = None if log is None else {k: np.asarray(v) for k, v in log.items()}
        self.time_cum = [float(x) for x in time_cum]
        self.clearance = None if clearance is None else np.array(clearance)

    def __len__(self):
        return len(self.definition['policy_id'])

    @staticmethod
    def define(agents, path_set, obstacles):
        """the arrays an episode's agents and obstacles are rebuilt from; path_set: the agents' waypoint lists as they were handed to the
        device (the agents' own are shortened to what is left)"""
        d = dict(start=np.array([a.initial_pos for a in agents], np.float64).reshape(len(agents), 6),
                 goal=np.array([a.goal_pos for a in agents], np.float64).reshape(len(agents), 6),
                 policy_id=np.array([a.policy.policy_id for a in agents], np.uint8),
                 pitchlims=np.array([a.pitchlims for a in agents], np.float64).reshape(len(agents), 2),
                 path_off=np.concatenate([[0], np.cumsum([len(p) for p in path_set])]).astype(np.int32),
                 path_pts=np.array([w[:3] for p in path_set for w in p], np.float64).reshape(-1, 3))
        for k in _AGENT_SCALARS:
            d[k] = np.array([getattr(a, k) for a in agents], np.float64)
        shapes = sorted({o.shape for o in obstacles})
        if any(sh != 'sphere' for sh in shapes):
            raise ValueError(f'SceneCheckpoint: obstacles of shape {shapes} (only spheres are kept as arrays)')
        d['obs_pos'] = np.array([o.pos_global_frame for o in obstacles], np.float64).reshape(len(obstacles), 3)
        d['obs_radius'] = np.array([o.radius for o in obstacles], np.float64)
        return d

    def agents(self):
        """the episode's agents, fresh through Agent's constructor: at their start, carrying their lists as they were handed to the device"""
        d = self.definition
        out = []
        for i in range(len(self)):
            a = _env.Agent(start_pos=list(d['start'][i]), goal_pos=list(d['goal'][i]), vel=[0.0, 0.0, 0.0], radius=float(d['radius'][i]),
                           pref_speed=float(d['pref_speed'][i]), policy=_POLICIES[int(d['policy_id'][i])], id=i)
            for k in _AGENT_SCALARS:
                setattr(a, k, int(d[k][i]) if k in ('maxNeighbors', 'group') else float(d[k][i]))
            a.pitchlims = [float(d['pitchlims'][i][0]), float(d['pitchlims'][i][1])]
            a._path = [list(map(float, w)) for w in d['path_pts'][d['path_off'][i]:d['path_off'][i + 1]]]
            out.append(a)
        return out

    def obstacles(self):
        d = self.definition
        return [_env.Obstacle(list(map(float, p)), dict(shape='sphere', feature=float(r)), id=i) for i, (p, r) in enumerate(zip(d['obs_pos'], d['obs_radius']))]

    def write(self, path):
        """one .npz of plain arrays"""
        arrays = {'def_' + k: v for k, v in self.definition.items()}
        arrays.update(blob=self.blob, steps=np.array(self.steps, np.int64), time_cum=np.array(self.time_cum, np.float64), has_log=np.array(self.log is not None))
        if self.log is not None:
            arrays.update({'log_' + k: v for k, v in self.log.items()})
        if self.clearance is not None:
            arrays.update(clearance=self.clearance)
        with open(path, 'wb') as f:
            np.savez(f, **arrays)
        return path

    @classmethod
    def read(cls, path):
        with np.load(path, allow_pickle=False) as z:
            definition = {k[4:]: z[k] for k in z.files if k.startswith('def_')}
            log = {k[4:]: z[k] for k in z.files if k.startswith('log_')} if bool(z['has_log']) else None
            return cls(definition, z['blob'], int(z['steps']), log, z['time_cum'], z['clearance'] if 'clearance' in z.files else None)


class SceneBatch(_FlatAgents):
    def __init__(self, scenes, obstacles=(), scene_obstacles=None, neighbor_mode=S.NBR_KDTREE, device_tracker=False, history_capacity=0, scene_history=0, device=0,
                 capacities=None, harvest=False, obstacle_capacities=None, attribute_slots=False, path_slots=None, clearance=False):
        """clearance: every step also keeps each agent's closest approach to another agent and to an obstacle of its scene
        (sca_scene_clearance_enable: one more kernel per step, O(size^2) per live scene); env(s).clearance reads a scene's records.
        path_slots: W, the waypoints every agent row has room for, or 'max' (the longest list among the initial agents, at least 1);
        None: the lists are one block, as a batch always had them.  The lists are then uploaded in SLOT form (sca_set_path_slots) and a
        restarted slot takes the episode's own lists (sca_restart_scenes_paths): restart() accepts agents that carry paths, none longer
        than W, and a later `agent.path = [...]` keeps working through the slot form.
        attribute_slots: a restarted slot takes the episode's own solver attributes (neighborDist, maxNeighbors, timeStep, timeHorizon,
        maxSpeed, max_heading_change, dt_nominal) and planner attributes (turning_radius, pitchlims) instead of keeping its own
        (sca_restart_scenes_attrs): restart() then accepts agents whose attributes differ from the slot's, and agents that change between a
        tracked and an untracked policy.  A parameter study -- one attribute swept across seeds -- streams through one batch.
        obstacle_capacities: one obstacle capacity per scene, each >= len(scene_obstacles[s]), or 'max' (every slot holds the largest
        list); None: none.  The scenes' obstacle ranges are then OBSTACLE SLOTS (sca_set_scene_obstacle_slots): the initial lists
        (scene_obstacles; None: every slot starts empty) go through the slots call, and restart(..., obstacles={s: [...]}) brings a new
        episode's own list of up to that many obstacles into a slot.
        harvest: finished scenes hand over their result with the step (sca_scene_harvest_enable): step() reads `active` / `steps` from the
        harvest block behind the step's own synchronisation instead of a second read-back, finished() names the scenes that ended since it
        was last called and harvested(s) gives a finished scene's final rows and summary without a read-back of the batch.
        capacities: one agent capacity per scene, each >= len(scene) (None: the scene's own length).  Scene s then owns capacities[s] rows
        of the context and holds its episode in the first of them; the rows behind are vacant (sca_restart_scenes_sized), and a later
        restart may bring any episode of 1 .. capacities[s] agents (without `capacities` a slot keeps its size).  The spare rows are set up as copies of the scene's last agent, so a slot's
        solver and planner attributes are those of the episode it started with."""
        scenes = [list(a) for a in scenes]
        if not scenes or any(len(a) == 0 for a in scenes):
            raise ValueError('a SceneBatch needs at least one scene and no empty one')
        for s, agents in enumerate(scenes):
            for i, a in enumerate(agents):
                if a.id != i:
                    raise ValueError(f'scene {s}: agent.id must equal its index in its scene (kdTree.py:64), as for an env of its own')
        self.obstacles = list(obstacles)
        self.scene_obstacles = None if scene_obstacles is None else [list(o) for o in scene_obstacles]
        self.obstacle_slots = obstacle_capacities is not None
        if self.obstacle_slots and self.scene_obstacles is None:
            self.scene_obstacles = [[] for _ in scenes]
        if self.scene_obstacles is not None:
            if self.obstacles:
                raise ValueError('a SceneBatch takes either `obstacles` (one list shared by all scenes) or `scene_obstacles` (one list per scene)')
            if len(self.scene_obstacles) != len(scenes):
                raise ValueError(f'scene_obstacles: {len(self.scene_obstacles)} lists for {len(scenes)} scenes')
            held = [len(o) for o in self.scene_obstacles]
            if isinstance(obstacle_capacities, str):
                if obstacle_capacities != 'max':
                    raise ValueError(f"obstacle_capacities: None, 'max' or one capacity per scene, got {obstacle_capacities!r}")
                obstacle_capacities = [max(held)] * len(scenes)
            ocaps = held if obstacle_capacities is None else [int(c) for c in obstacle_capacities]
            if len(ocaps) != len(scenes) or any(c < m for c, m in zip(ocaps, held)):
                raise ValueError(f"obstacle_capacities: one per scene, each at least the scene's obstacle count ({held}), got {ocaps}")
            self.obstacle_offsets = np.concatenate([[0], np.cumsum(ocaps)]).astype(np.int32)     # a scene's range: its capacity where there are slots
        self.neighbor_mode = neighbor_mode
        self.device_tracker = bool(device_tracker)
        self.capacity_slots = capacities is not None               # else: a slot keeps its size, as a batch always did
        self.attribute_slots = bool(attribute_slots)               # else: a slot keeps its attributes, as a batch always did
        if isinstance(path_slots, str):
            if path_slots != 'max':
                raise ValueError(f"path_slots: None, 'max' or the waypoints a row has room for, got {path_slots!r}")
            path_slots = max([1] + [len(a._path) for agents in scenes for a in agents])
        self._path_set = None                                       # the lists as last handed to the device, row by row (None: never)
        self.path_slots = 0 if path_slots is None else int(path_slots)     # 0: the lists are one block, and restart() refuses them
        if path_slots is not None and self.path_slots < 1:
            raise ValueError(f'path_slots: a row needs room for at least 1 waypoint, got {path_slots!r}')
        self._path_slots = self.path_slots
        self.sizes = np.array([len(a) for a in scenes], np.int32)   # agents each scene holds ...
        caps = self.sizes.copy() if capacities is None else np.array([int(c) for c in capacities], np.int32)
        if len(caps) != len(scenes) or (caps < self.sizes).any():
            raise ValueError(f'capacities: one per scene, each at least the scene\'s agent count ({list(self.sizes)}), got {list(caps)}')
        self.offsets = np.concatenate([[0], np.cumsum(caps)]).astype(np.int32)          # ... in the first rows of its range, its capacity
        flat = []
        for agents, cap in zip(scenes, caps):
            flat.extend(agents)
            for i in range(len(agents), int(cap)):                  # spare rows: valid constants and the slot's attributes, vacated below
                pad = copy.copy(agents[-1])
                pad.id, pad._path = i, []
                flat.append(pad)
        B = len(scenes)

        def set_scenes():                                             # between the agents' attributes and the state
            self.solver.set_scenes(self.offsets)
            if self.obstacle_slots:
                self.solver.set_scene_obstacle_slots(np.diff(self.obstacle_offsets), [_obstacle_arrays(obs) for obs in self.scene_obstacles])
            elif self.scene_obstacles is not None:
                self.solver.set_scene_obstacles([_obstacle_arrays(obs) for obs in self.scene_obstacles])

        shared = self.scene_obstacles is None
        self._create(flat, device, len(self.obstacles) if shared else int(self.obstacle_offsets[-1]), self.obstacles if shared else None, set_scenes)
        self._envs = [SceneEnv(self, s, scenes[s], int(self.offsets[s]), int(self.offsets[s]) + len(scenes[s])) for s in range(B)]
        for view in self._envs:
            _bind(view.agents, view)
        self._reset_paths()
        spare = [(s, scenes[s]) for s in range(B) if caps[s] > self.sizes[s]]
        if spare:                                                     # one sized restart before the first step vacates the spare rows
            self._send_restart(spare)
        self.active = self.sizes.copy()                               # agents of each scene the next step will serve
        self.steps = np.zeros(B, np.int32)                            # steps each scene has taken while it was live
        if history_capacity:
            self.solver.history_enable(int(history_capacity))
        # scene_history: rows PER SCENE of the log per scene (metrics.trajectories(batch.env(s))); history_capacity above stays the
        # context-wide log, a row per batch step.  64 B x rows x agents of HBM up front: capped to a budget, as MACAEnv caps its log
        self.scene_history = int(scene_history)
        self.history_budget_bytes = 64 << 30
        n = len(flat)
        if self.scene_history and 64 * self.scene_history * n > self.history_budget_bytes:
            capped = max(1, self.history_budget_bytes // (64 * n))
            import warnings
            warnings.warn(f'scene_history {self.scene_history} x {n} agents x 64 B exceeds the {self.history_budget_bytes >> 30} GiB '
                          f'budget: keeping the first {capped} steps of every scene (later steps are counted as dropped)')
            self.scene_history = capped
        if self.scene_history:
            self.solver.scene_history_enable(self.scene_history)
        self.harvest = bool(harvest)
        if self.harvest:
            self.solver.scene_harvest_enable()
            self._harvest = self.solver.scene_harvest()           # views of the block: read behind a step's synchronisation
        self.clearance = bool(clearance)
        if self.clearance:                                            # (behind the restart that vacated the spare rows: every row starts empty)
            self.solver.scene_clearance_enable()

    def __len__(self):
        return len(self._envs)

    # ---- the lists in slot form (SceneBatch(path_slots=W)) -----------------------------------------------------------------------------------
    def _path_lists(self):
        """the agents' lists, row by row; a vacant row (behind its slot's episode) has none"""
        lists = [a._path for a in self._flat]
        if self.path_slots:
            for i in self._vacant_rows():
                lists[i] = []
        return lists

    def _vacant_rows(self):
        return {i for s in range(len(self.sizes)) for i in range(int(self.offsets[s]) + int(self.sizes[s]), int(self.offsets[s + 1]))}

    def _refresh_paths(self, skip=()):
        """(the agents that stand in vacant rows belong to an episode that has left its slot: their lists stay what that episode left)"""
        super()._refresh_paths(set(skip) | self._vacant_rows() if self.path_slots else skip)

    def _upload_paths(self, lists):
        self._path_set = [[list(w) for w in p] for p in lists]      # the lists as the device holds them (SceneBatch.checkpoint)
        if not self.path_slots:
            return super()._upload_paths(lists)
        self._check_path_room([(i, p) for i, p in enumerate(lists)], 'agent.path')
        self.solver.set_path_slots(self.path_slots, lists)

    def _check_path_room(self, rows, who):
        for i, p in rows:
            if len(p) > self.path_slots:
                raise ValueError(f'{who}: row {i} carries a list of {len(p)} waypoints, a row has room for {self.path_slots} (SceneBatch(path_slots=...))')

    def env(self, s):
        return self._envs[s]

    @property
    def done(self):
        return self.active == 0

    def close(self):
        self._harvest = None
        self.solver.close()

    # ---- finished scenes hand over their result with the step (SceneBatch(harvest=True)) ----------------------------------------------------
    def finished(self):
        """the scenes that finished since the last call, in the order they finished (batch step, then scene id)"""
        if not self.harvest:
            raise RuntimeError('finished(): a SceneBatch(harvest=True) hands finished scenes over; this one was built without')
        return self.solver.scene_harvest_collect()

    def harvested(self, s):
        """dict(pos, vel, heading, flags, total_dist, step_num, summary) of a finished scene: its occupied rows as the step that finished it
        left them (what solver.get_state() gives for them) and the device's summary (steps, batch_step, arrived, collided, timed_out,
        successful_num, all_step_num, all_distance).  Copies: the block's rows are overwritten when the slot finishes again.  Take them
        before the scene is restarted."""
        if not self.harvest:
            raise RuntimeError('harvested(): a SceneBatch(harvest=True) hands finished scenes over; this one was built without')
        s = int(s)
        lo = int(self.offsets[s])
        hi = lo + int(self.sizes[s])
        out = {k: self._harvest[k][lo:hi].copy() for k in self._mirror}
        rec = self._harvest['summary'][s]
        out['summary'] = {k: rec[k].item() for k in ('steps', 'batch_step', 'arrived', 'collided', 'timed_out', 'successful_num', 'all_step_num',
                                                     'all_distance')}
        return out

    # ---- a running episode out of its slot, and back into any (sca_save_scenes / sca_load_scenes) ---------------------------------------------
    def checkpoint(self, s):
        """SceneCheckpoint of scene s as it stands between two steps: the episode's definition, the library's blob, `steps`, and the log
        rows so far when the batch keeps a log per scene"""
        s = int(s)
        if not 0 <= s < len(self._envs):
            raise ValueError(f'checkpoint: no scene {s} in a batch of {len(self._envs)}')
        self._sync_paths()                                          # (an `agent.path = [...]` since the last step is part of the episode)
        view = self._envs[s]
        lo = int(self.offsets[s])
        path_set = [[] for _ in view.agents] if self._path_set is None else self._path_set[lo:lo + len(view.agents)]
        blob = self.solver.save_scenes([s])[0]
        steps = int(self.solver.scene_checkpoint_info(blob)['steps'])
        log = None
        if self.scene_history:
            rows, _ = view.solver.history_rows()
            log = view.solver.history(0, rows)
        return SceneCheckpoint(SceneCheckpoint.define(view.agents, path_set, view.obstacles), blob, steps, log, view._time_cum,
                               view.clearance if self.clearance else None)

    # ---- a new episode into a slot while the others keep running (sca_restart_scenes) -------------------------------------------------------
    def restart(self, scenes, obstacles=None):
        """{s: agents}: scene s starts over with the new Agent list (numbered 0 .. n - 1; n is the slot's count, or, in a batch built with
        `capacities`, any 1 <= n <= the slot's capacity), every other scene is untouched.  A slot keeps its capacity, its obstacles (unless
        `obstacles` brings new ones) and its per-agent solver and planner attributes: ValueError, before any device
        call, for an episode that does not fit, an agent whose attributes differ from its row's, or one that carries a path.  From here on
        the scene is bit for bit the MACAEnv of the new episode alone, like a scene of a fresh batch.
        obstacles ({s: [Obstacle, ...]}, a batch built with obstacle_capacities): the restarted scene s meets this list from now on (at
        most its obstacle capacity; [] for none) -- bit for bit the MACAEnv of the new episode with that list --; a restarted scene absent
        from it keeps its list.  ValueError before any device call for a list above the slot's capacity, a scene that is not restarted, or
        `obstacles` on a batch without obstacle slots."""
        resumed = {int(s): x for s, x in dict(scenes).items() if isinstance(x, SceneCheckpoint)}
        items = sorted((int(s), x.agents() if isinstance(x, SceneCheckpoint) else list(x)) for s, x in dict(scenes).items())
        new_obs = None if obstacles is None else {int(s): list(o) for s, o in dict(obstacles).items()}
        for s, ck in resumed.items():                                # a checkpoint brings its episode's obstacles: into an obstacle slot, or
            own = ck.obstacles()                                     # the scene must meet exactly that set already
            if new_obs is not None and s in new_obs:
                continue
            if self.obstacle_slots:
                new_obs = dict(new_obs or {})
                new_obs[s] = own
            elif 0 <= s < len(self._envs) and not (np.array_equal(_obstacle_arrays(own)[0], _obstacle_arrays(self._envs[s].obstacles)[0]) and
                                                   np.array_equal(_obstacle_arrays(own)[1], _obstacle_arrays(self._envs[s].obstacles)[1])):
                raise ValueError(f"restart: scene {s}: the checkpoint's episode meets {len(own)} obstacles of its own, which this batch cannot bring "
                                 'into the slot (SceneBatch(obstacle_capacities=...))')
            if ck.log is not None and self.scene_history and len(ck.log['pos']) < min(ck.steps, self.scene_history):
                raise ValueError(f'restart: scene {s}: the checkpoint holds {len(ck.log["pos"])} log rows of its {ck.steps} steps')
        if new_obs is not None:
            if not self.obstacle_slots:
                raise ValueError('restart: obstacles for a batch without obstacle slots (SceneBatch(obstacle_capacities=...))')
            for s, obs in new_obs.items():
                if s not in dict(items):
                    raise ValueError(f'restart: obstacles for scene {s}, which is not restarted')
                cap = int(self.obstacle_offsets[s + 1] - self.obstacle_offsets[s])
                if len(obs) > cap:
                    raise ValueError(f'restart: scene {s} holds up to {cap} obstacles, the new episode brings {len(obs)} (a slot keeps its obstacle capacity)')
        if not items:
            return
        if self._paths_on and not self.path_slots:
            raise ValueError('restart: waypoint lists are set in this batch (they are one block for all scenes; SceneBatch(path_slots=...) '
                             'gives every row room of its own)')
        for s, agents in items:
            if not 0 <= s < len(self._envs):
                raise ValueError(f'restart: no scene {s} in a batch of {len(self._envs)}')
            lo, hi = int(self.offsets[s]), int(self.offsets[s + 1])
            if not self.capacity_slots and len(agents) != hi - lo:
                raise ValueError(f'restart: scene {s} holds {hi - lo} agents, the new episode has {len(agents)} (a slot keeps its size; '
                                 'SceneBatch(capacities=...) makes slots that take any episode that fits)')
            if not 1 <= len(agents) <= hi - lo:
                raise ValueError(f'restart: scene {s} holds 1 .. {hi - lo} agents, the new episode has {len(agents)} (a slot keeps its capacity)')
            for i, (a, old) in enumerate(zip(agents, self._flat[lo:hi])):     # (over the rows the episode occupies)
                if a.id != i:
                    raise ValueError(f'restart: scene {s}: agent.id must equal its index in its scene')
                if len(a._path) and not self.path_slots:
                    raise ValueError(f'restart: scene {s}, agent {i} carries a path: waypoint lists cannot be replaced per scene '
                                     '(SceneBatch(path_slots=...) makes slots that take the episode\'s own lists)')
                if len(a._path) > self.path_slots > 0:
                    raise ValueError(f'restart: scene {s}, agent {i} carries a list of {len(a._path)} waypoints, a row has room for {self.path_slots}')
                for name, (attr, conv) in _ATTRS.items():
                    if not self.attribute_slots and conv(getattr(a, attr)) != conv(getattr(old, attr)):
                        raise ValueError(f"restart: scene {s}, agent {i}: {attr} differs from the slot's (a slot keeps its solver attributes; "
                                         'SceneBatch(attribute_slots=True) makes slots that take the episode\'s own)')
                if not self.attribute_slots and self._trk_trip is not None and bool(a.policy.needs_external_vpref) != bool(old.policy.needs_external_vpref):
                    raise ValueError(f'restart: scene {s}, agent {i} changes between a tracked (SCA, RVO3D+Dubins) and an untracked policy while the '
                                     "batch carries planner attributes per agent: the tracker's classes are cut by policy")
                if a.policy.needs_external_vpref and self.device_tracker:
                    if not self._trk_on:
                        raise ValueError(f'restart: scene {s}, agent {i} needs the device tracker, which a batch built without such agents has not enabled')
                    if not self.attribute_slots and _planner_triple(a) != self._planner_of(lo + i):
                        raise ValueError(f"restart: scene {s}, agent {i}: turning_radius / pitchlims differ from the slot's (a slot keeps its planner attributes)")
        self._send_restart(items, new_obs)
        if resumed:                                                  # the episodes are in their slots: now their state, one call
            ids = sorted(resumed)
            self.solver.load_scenes(ids, [resumed[s].blob for s in ids])
        for s, agents in items:
            lo = int(self.offsets[s])
            view = self._envs[s]
            if new_obs and s in new_obs:
                self.scene_obstacles[s] = view.obstacles = new_obs[s]
            self._flat[lo:lo + len(agents)] = agents                 # (the rows behind keep the agents that carry the slot's attributes)
            view._occupy(agents, lo + len(agents))
            view._time_cum = list(resumed[s].time_cum) if s in resumed else [0.0]
            view._log_head = resumed[s].log if s in resumed and self.scene_history else None
            view._clear_head = resumed[s].clearance if s in resumed and self.clearance else None      # (the restart emptied the slot's records)
            _bind(agents, view)
        self._stale = True                                           # the mirrors (views of the batch's arrays) refresh in place on first use
        self._path_stale = self._paths_on                            # (slot form: the new agents' whole lists, now_goal None, read back on first use)
        self._nbr_cache = None
        self._vpref_cache = None
        if self.harvest and not resumed:                             # what the restart leaves, without a read-back: all of the episode live, no step taken
            for s, agents in items:
                self.active[s], self.steps[s] = len(agents), 0
        else:
            st = self.solver.scene_state()
            self.active, self.steps = st['active'], st['steps']

    def _send_restart(self, items, new_obs=None):
        """the episodes' arrays to the device (one call), and the batch's per-agent host arrays behind them"""
        flat = [a for _, agents in items for a in agents]
        T = len(flat)
        start = np.array([a.initial_pos for a in flat], dtype=np.float64).reshape(T, 6)
        goal6 = np.array([a.goal_pos for a in flat], dtype=np.float64).reshape(T, 6)
        goal = np.array([a.goal_global_frame for a in flat], dtype=np.float64).reshape(T, 3)
        policy = np.array([a.policy.policy_id for a in flat], np.uint8)
        # (a batch whose slots are all full, before and after, makes the plain call: sca_restart_scenes)
        full = all(len(agents) == self.offsets[s + 1] - self.offsets[s] for s, agents in items) and (self.sizes == np.diff(self.offsets)).all()
        attrs = None
        if self.attribute_slots:                                     # every attribute of every agent: the rows take exactly the episode's
            attrs = {name: [conv(getattr(a, attr)) for a in flat] for name, (attr, conv) in _ATTRS.items()}
            if self._trk_on:
                trip = [_planner_triple(a) for a in flat]
                attrs.update(turning_radius=[t[0] for t in trip], pitch_lo=[t[1] for t in trip], pitch_hi=[t[2] for t in trip])
        self.solver.restart_scenes([s for s, _ in items], np.array([a._pos for a in flat], dtype=np.float64).reshape(T, 3),
                                   np.array([a._heading for a in flat], dtype=np.float64).reshape(T, 3),
                                   vel=np.array([a._vel for a in flat], dtype=np.float32).reshape(T, 3), radius=[a.radius for a in flat],
                                   pref_speed=[a.pref_speed for a in flat], goal=goal, policy=policy, zaxis=S.zaxis_flags(start, goal6),
                                   max_run_dist=[a.max_run_dist for a in flat], goal_heading=goal6[:, 3:6] if self._trk_on else None,
                                   sizes=None if full else [len(agents) for _, agents in items],
                                   obstacles=[_obstacle_arrays(new_obs[s]) if s in new_obs else None for s, _ in items] if new_obs else None,
                                   attrs=attrs, paths=[[list(map(float, w[:3])) for w in a._path] for a in flat] if self.path_slots else None)
        if attrs is not None and self._trk_on:                       # the planner attributes the device holds per row (_planner_of)
            if self._trk_trip is None:
                self._trk_trip = [self._trk_first] * len(self._flat)
            at = 0
            for s, agents in items:
                lo = int(self.offsets[s])
                self._trk_trip[lo:lo + len(agents)] = trip[at:at + len(agents)]
                at += len(agents)
        at = 0
        for s, agents in items:
            lo, n = int(self.offsets[s]), len(agents)
            if self._path_set is not None:                           # (the rows behind the episode hold no list)
                self._path_set[lo:int(self.offsets[s + 1])] = [[list(map(float, w[:3])) for w in a._path] if self.path_slots else [] for a in agents] + \
                    [[] for _ in range(int(self.offsets[s + 1]) - lo - n)]
            self.goal[lo:lo + n] = goal[at:at + n]                   # (view.goal is a view of these rows)
            self.policy_ids[lo:lo + n] = policy[at:at + n]
            self._ext[lo:lo + n] = [a.policy.needs_external_vpref for a in agents]
            self.sizes[s] = n
            at += n

    # ---- one step of every live scene ------------------------------------------------------------------------------------------------------
    def step(self, actions=None):
        """One resident step of all scenes (finished scenes are inert).  True when every scene is done."""
        self._sync_paths()
        t0 = time.perf_counter()
        live = self.active > 0
        served = max(1, int(self.active.sum()))
        total = self.solver.env_step(self.neighbor_mode)
        share = (time.perf_counter() - t0) / served               # a step's policy wall time, shared among the agents it served
        if self.harvest:                                          # written by the step's last kernel, readable behind env_step's synchronisation
            self.active, self.steps = self._harvest['active'].copy(), self._harvest['steps'].copy()
        else:
            st = self.solver.scene_state()
            self.active, self.steps = st['active'], st['steps']
        for view, was in zip(self._envs, live):
            if was:
                view._time_cum.append(view._time_cum[-1] + share)
        self._stale = True
        self._path_stale = self._paths_on
        self._nbr_cache = None
        self._vpref_cache = None
        return total == 0


# ---- a queue of any length through B slots -----------------------------------------------------------------------------------------------
def plan_slots(sizes, slots):
    """Which queue entries the slots start with: entry i in slot i, after one slot has been reserved for every distinct agent count in the
    queue (a slot keeps its size, so a count without a slot could never run).  Returns the entries in slot order -- min(slots, len(sizes))
    of them; ValueError when there are fewer slots than distinct counts."""
    sizes = [int(n) for n in sizes]
    first = {}
    for i, n in enumerate(sizes):
        first.setdefault(n, i)
    if slots < len(first):
        raise ValueError(f'{slots} slots for a queue with {len(first)} distinct agent counts: every count needs a slot of its own')
    chosen = set(first.values())
    for i in range(len(sizes)):
        if len(chosen) >= min(slots, len(sizes)):
            break
        chosen.add(i)
    return sorted(chosen)


def next_episode(slot_size, pending_sizes):
    """The position in `pending_sizes` (the agent counts of the episodes not started yet, in queue order) of the episode a finished slot of
    `slot_size` agents takes: the first of its size; None when there is none -- the slot then stays done."""
    for k, n in enumerate(pending_sizes):
        if int(n) == int(slot_size):
            return k
    return None


def next_fitting(capacity, pending_sizes):
    """The position in `pending_sizes` of the episode a finished slot of `capacity` agent rows takes: the first, in queue order, that fits
    (1 .. capacity agents); None when there is none -- the slot then stays done."""
    for k, n in enumerate(pending_sizes):
        if int(n) <= int(capacity):
            return k
    return None


def next_fitting2(capacity, obs_capacity, pending):
    """next_fitting over both capacities: `pending` holds (agents, obstacles) per episode not started yet, in queue order; the position of
    the first that fits a slot of `capacity` agent rows AND `obs_capacity` obstacle rows, None when there is none."""
    for k, (n, m) in enumerate(pending):
        if int(n) <= int(capacity) and int(m) <= int(obs_capacity):
            return k
    return None


def plan_capacity_slots2(sizes, capacities):
    """plan_capacity_slots over both capacities: sizes = [(agents, obstacles)] per episode, capacities = [(agent rows, obstacle rows)] per
    slot.  One entry per slot (None: nothing fits it); ValueError when some episode fits no slot at all."""
    sizes = [(int(n), int(m)) for n, m in sizes]
    capacities = [(int(c), int(oc)) for c, oc in capacities]
    if not capacities or min(c for c, _ in capacities) < 1 or min(oc for _, oc in capacities) < 0:
        raise ValueError(f'slot capacities must be positive (obstacles: not negative), got {capacities}')
    for i, (n, m) in enumerate(sizes):
        if not any(n <= c and m <= oc for c, oc in capacities):
            raise ValueError(f'episode {i} has {n} agents and {m} obstacles and fits no slot (capacities {capacities})')
    pending = list(range(len(sizes)))
    holding = []
    for c, oc in capacities:
        k = next_fitting2(c, oc, [sizes[j] for j in pending])
        holding.append(None if k is None else pending.pop(k))
    return holding


def plan_capacity_slots(sizes, capacities):
    """Which queue entry every slot starts with when slot s holds any episode of up to capacities[s] agents: the slots choose in their own
    order, each the first entry in queue order that fits it and that no earlier slot took (next_fitting).  Returns one entry per slot, None
    for a slot no remaining entry fits -- it never will, the queue only shrinks.  ValueError when some episode fits no slot at all."""
    sizes, capacities = [int(n) for n in sizes], [int(c) for c in capacities]
    if not capacities or min(capacities) < 1:
        raise ValueError(f'slot capacities must be positive, got {capacities}')
    for i, n in enumerate(sizes):
        if n > max(capacities):
            raise ValueError(f'episode {i} has {n} agents and fits no slot (capacities {capacities})')
    pending = list(range(len(sizes)))
    holding = []
    for cap in capacities:
        k = next_fitting(cap, [sizes[j] for j in pending])
        holding.append(None if k is None else pending.pop(k))
    return holding


def plan_queue(sizes, slots, capacities=None):
    """(holding, slot_capacities): the queue entry each slot of the batch starts with and the agent rows it owns.  capacities None: slots of
    fixed size (plan_slots: a slot takes episodes of exactly its own count); 'max': `slots` slots that each hold the largest episode; a
    list: one capacity per slot.  Slots that would start empty are left out of the batch."""
    sizes = [int(n) for n in sizes]
    if capacities is None:
        holding = plan_slots(sizes, slots)
        return holding, [sizes[i] for i in holding]
    if isinstance(capacities, str):
        if capacities != 'max':
            raise ValueError(f"capacities: None, 'max' or a list of slot capacities, got {capacities!r}")
        capacities = [max(sizes)] * int(slots)
    capacities = [int(c) for c in capacities]
    if len(capacities) != int(slots):
        raise ValueError(f'{len(capacities)} capacities for {slots} slots')
    holding = plan_capacity_slots(sizes, capacities)
    used = [s for s, i in enumerate(holding) if i is not None]
    return [holding[s] for s in used], [capacities[s] for s in used]


def _harvest_policy_time(view, h):
    """what episode_metrics sums by default -- agent.total_time over the successful agents, in agent order -- from the harvested rows"""
    cum = view._time_cum
    ok = (h['flags'] & (S.FLAG_COLLISION | S.FLAG_TIMEOUT)) == 0
    return sum(cum[min(int(k), len(cum) - 1)] for k, good in zip(h['step_num'], ok) if good)


def run_episodes(episodes, slots, obstacles=(), device_tracker=False, on_done=None, max_steps=None, stats=None, history_rows=0, capacities=None,
                 harvest=False, episode_obstacles=None, obstacle_capacities='max', attributes=False, path_slots=None, checkpoint_at=None,
                 clearance=False):
    """Streams a queue of episodes (Agent lists, each numbered 0 .. n - 1) through `slots` scenes of ONE SceneBatch: when a scene finishes,
    its metrics, step count and final state are taken and the slot restarts with the next episode of its size (SceneBatch.restart), while
    the other slots keep running.  Obstacles are one list shared by all episodes (`obstacles`), or -- mutually exclusive with it --
    episode_obstacles, one list of Obstacle per episode: every episode then brings its own obstacles into its slot (obstacle slots,
    SceneBatch(obstacle_capacities=...)), and a finished slot takes the first pending episode that fits BOTH its agent and its obstacle
    capacity (next_fitting2).  obstacle_capacities: 'max' sizes every slot for the largest list in the queue; a list gives one obstacle
    capacity per slot (ValueError up front when some episode fits no slot).  Without `capacities` the slots' agent capacities are those
    of 'max' as well: a queue with per-episode obstacles always runs on capacity slots.  Returns one dict per episode in queue order:
    episode, slot, metrics (metrics.episode_metrics), steps, state (pos, vel, heading, flags, total_dist, step_num); on_done(result) is
    called as each finishes.  With device_tracker, the tracker is enabled by the episodes the slots START with: a queue whose first tracked
    (SCA, RVO3D+Dubins) episode comes later is refused here, before the first step (ValueError).  An episode that a slot cannot take (SceneBatch.restart's
    rules: a path, other solver or planner attributes) raises when its turn comes.  The dict of an episode that max_steps cut short is None.  `stats`, a dict, receives batch_steps, agent_steps
    (agents served, summed over the steps) and live_fraction (their mean share of the batch's agents per step).  history_rows=K keeps a trajectory
    log of K rows per slot (SceneBatch(scene_history=K)): every result gains `trajectories` ([n, rows, 13], metrics.ANIMATION_COLUMNS, the
    episode's first K steps at most), `rows_dropped` (its steps beyond K) and `info` (metrics.episode_info: with the trajectories, what
    metrics.write_log_files writes an episode's folder from), read when the slot finishes, before it is refilled; an episode
    longer than K does not stop the queue.  capacities='max' (or a list, one agent capacity per slot) makes the slots CAPACITY slots: a slot
    starts with, and later takes, the first pending episode in queue order that fits it, whatever its agent count (plan_capacity_slots,
    next_fitting), so a queue that mixes counts streams through one set of slots; ValueError before the first step when an episode fits no
    slot.  live_fraction then counts the slots' capacities as the batch's agent rows.  harvest=True: the same results, on_done order and
    stats, taken from what the finishing step itself handed over (SceneBatch(harvest=True): finished() / harvested()) -- one
    synchronisation per step and, per finished episode, its own rows instead of a read-back of the whole batch.  attributes=True: the slots
    take every episode's own solver and planner attributes (SceneBatch(attribute_slots=True)), so a queue whose episodes differ in them --
    a sweep of neighborDist across seeds -- streams through one batch instead of raising when such an episode's turn comes.
    path_slots=W or 'max' (the longest list in the whole queue, at least 1): the slots take every episode's own waypoint lists
    (SceneBatch(path_slots=W)), so a queue whose drones carry paths streams through one batch; results, on_done order and stats are those
    of the same queue run as one MACAEnv per episode, and every result gains `path_left`, the waypoints left in each agent's list when the
    episode finished (the agents' own lists are shortened to that).  ValueError up front for a list longer than W.
    A queue entry may be a SceneCheckpoint instead of an Agent list: the episode then enters its slot where the checkpoint left it
    (SceneBatch.restart({s: checkpoint})), and its result is that of the uninterrupted episode; with episode_obstacles its entry may be
    None (the checkpoint's own obstacles).  checkpoint_at=(batch_step, directory): behind that many batch steps every slot that still
    holds an episode is written there as a checkpoint (slotSSS_episodeEEEEE.npz) and the run stops; the results of the episodes that have
    not finished are None, and `stats` receives `checkpoints` ({slot: (episode, path)}) and `pending` (the episodes that never started) --
    a second run_episodes over the checkpoints in slot order plus the pending episodes finishes the queue as one run would have.
    clearance=True: every result gains `clearance`, the episode's closest-approach records (SceneBatch(clearance=True); one record per
    agent, metrics.clearance_metrics reads them), taken when the slot finishes, before it is refilled, with `harvest` on or off."""
    import os
    cks = {i: e for i, e in enumerate(episodes) if isinstance(e, SceneCheckpoint)}
    episodes = [e.agents() if isinstance(e, SceneCheckpoint) else list(e) for e in episodes]
    if isinstance(path_slots, str):
        if path_slots != 'max':
            raise ValueError(f"run_episodes: path_slots is None, 'max' or the waypoints a row has room for, got {path_slots!r}")
        path_slots = max([1] + [len(a._path) for e in episodes for a in e])
    if path_slots is not None:
        for i, e in enumerate(episodes):
            for a in e:
                if len(a._path) > int(path_slots):
                    raise ValueError(f'run_episodes: episode {i}, agent {a.id} carries a list of {len(a._path)} waypoints, path_slots is {path_slots}')
    sizes = [len(e) for e in episodes]
    ocaps = None
    if episode_obstacles is not None:
        if len(obstacles):
            raise ValueError('run_episodes: either `obstacles` (one list shared by all episodes) or `episode_obstacles` (one list per episode)')
        episode_obstacles = [cks[i].obstacles() if o is None and i in cks else list(o) for i, o in enumerate(episode_obstacles)]
        if len(episode_obstacles) != len(episodes):
            raise ValueError(f'run_episodes: {len(episode_obstacles)} obstacle lists for {len(episodes)} episodes')
        osizes = [len(o) for o in episode_obstacles]
        capacities = 'max' if capacities is None else capacities
        acaps = [max(sizes)] * int(slots) if isinstance(capacities, str) and capacities == 'max' else capacities
        ocaps = [max(osizes)] * int(slots) if isinstance(obstacle_capacities, str) and obstacle_capacities == 'max' else obstacle_capacities
        if isinstance(acaps, str) or isinstance(ocaps, str) or ocaps is None:
            raise ValueError(f"run_episodes: capacities and obstacle_capacities are 'max' or one capacity per slot, got {capacities!r} and {obstacle_capacities!r}")
        if len(acaps) != int(slots) or len(ocaps) != int(slots):
            raise ValueError(f'run_episodes: {len(acaps)} agent and {len(ocaps)} obstacle capacities for {slots} slots')
        both = list(zip(sizes, osizes))
        holding = plan_capacity_slots2(both, list(zip(acaps, ocaps)))
        used = [s for s, i in enumerate(holding) if i is not None]         # slots that would start empty are left out of the batch
        holding, caps, ocaps = [holding[s] for s in used], [int(acaps[s]) for s in used], [int(ocaps[s]) for s in used]
    else:
        holding, caps = plan_queue(sizes, slots, capacities)
    batch_agents = sum(caps)                                    # the slots keep their rows: the batch's agent count, for live_fraction
    pending = [i for i in range(len(episodes)) if i not in set(holding)]
    tracked = [any(a.policy.needs_external_vpref for a in e) for e in episodes]
    if device_tracker and any(tracked[i] for i in pending) and not any(tracked[i] for i in holding):
        raise ValueError('run_episodes: episode %d needs the device tracker, but none of the episodes the slots start with does, so the batch '
                         'would run without one: put a tracked episode among the first %d' % (min(i for i in pending if tracked[i]), len(holding)))
    batch = SceneBatch([episodes[i] for i in holding], obstacles, device_tracker=device_tracker, scene_history=history_rows,
                       capacities=None if capacities is None else caps, harvest=harvest, attribute_slots=attributes, path_slots=path_slots,
                       scene_obstacles=None if ocaps is None else [episode_obstacles[i] for i in holding], obstacle_capacities=ocaps, clearance=clearance)
    results = [None] * len(episodes)
    batch_steps = served = 0
    written = None
    try:
        if any(i in cks for i in holding):                            # the slots that start with a checkpoint: its state into the episode it was built with
            batch.restart({s: cks[i] for s, i in enumerate(holding) if i in cks},
                          obstacles=None if ocaps is None else {s: episode_obstacles[i] for s, i in enumerate(holding) if i in cks})
        while any(h is not None for h in holding) and (max_steps is None or batch_steps < max_steps):
            served += int(batch.active.sum())
            batch.step()
            batch_steps += 1
            refill, refill_obs, path_rem = {}, {}, None
            # (one step per collect: finished() is in slot order, as the scan of batch.done is)
            for s in (batch.finished() if harvest else [s for s, i in enumerate(holding) if i is not None and batch.done[s]]):
                i = holding[s]
                view, info_args = batch.env(s), {}
                if harvest:
                    h = batch.harvested(s)
                    t_policy = _harvest_policy_time(view, h)
                    m = metrics.episode_metrics_from_harvest(episodes[i], h, t_policy)
                    results[i] = dict(episode=i, slot=s, metrics=m, steps=int(h['summary']['steps']), state={k: h[k] for k in batch._mirror})
                    info_args = dict(total_policy_time_s=t_policy, m=m)
                else:
                    lo, hi = int(batch.offsets[s]), int(batch.offsets[s]) + int(batch.sizes[s])
                    results[i] = dict(episode=i, slot=s, metrics=metrics.episode_metrics(view), steps=int(batch.steps[s]),
                                      state={k: batch._state(k)[lo:hi].copy() for k in batch._mirror})
                if batch.path_slots:                              # what is left of the episode's lists, before its rows are given away
                    if path_rem is None:                          # (one read-back per batch step in which a scene finished)
                        path_rem = batch.solver.get_path_state()[0]
                    lo = int(batch.offsets[s])
                    for k, a in enumerate(episodes[i]):
                        del a._path[int(path_rem[lo + k]):]
                    results[i]['path_left'] = [len(a._path) for a in episodes[i]]
                if clearance:                                     # a finished scene keeps its records until the restart below
                    results[i]['clearance'] = view.clearance
                if batch.scene_history:
                    rows, dropped = view.solver.history_rows()
                    results[i].update(trajectories=metrics.trajectories(view, rows=rows), rows_dropped=dropped, info=metrics.episode_info(view, **info_args))
                if on_done is not None:
                    on_done(results[i])
                left = [sizes[j] for j in pending]
                if ocaps is not None:
                    k = next_fitting2(caps[s], ocaps[s], [both[j] for j in pending])
                else:
                    k = next_episode(sizes[i], left) if capacities is None else next_fitting(caps[s], left)
                holding[s] = None if k is None else pending.pop(k)
                if holding[s] is not None:
                    refill[s] = cks.get(holding[s], episodes[holding[s]])
                    if ocaps is not None:
                        refill_obs[s] = episode_obstacles[holding[s]]
            if refill:
                batch.restart(refill, obstacles=refill_obs if ocaps is not None else None)
            if checkpoint_at is not None and batch_steps == int(checkpoint_at[0]):
                os.makedirs(checkpoint_at[1], exist_ok=True)
                written = {}
                for s, i in enumerate(holding):
                    if i is not None:
                        written[s] = (i, batch.checkpoint(s).write(os.path.join(checkpoint_at[1], 'slot%03d_episode%05d.npz' % (s, i))))
                break
    finally:
        batch.close()
    if stats is not None and written is not None:
        stats.update(checkpoints=written, pending=list(pending))
    if stats is not None:
        stats.update(batch_steps=batch_steps, agent_steps=served, live_fraction=served / max(1, batch_steps * batch_agents))
    return results
