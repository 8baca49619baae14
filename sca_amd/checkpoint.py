"""Context checkpoints as files: a running plain context's DEFINITION as plain arrays, its blob (BatchedSolver.save_context) and its step
count in one .npz, no pickle.

    ck = ContextCheckpoint(ContextCheckpoint.define(...), sol.save_context(), steps)
    ck.write('run.npz')
    ...                                                     # another process, another GPU, a larger context
    sol = ContextCheckpoint.read('run.npz').solver()        # the definition set up in a fresh context, the blob loaded: bit for bit the run

The blob holds the mutable state only (include/sca_hip.h: what a blob holds); the definition is what the caller set the context up with
and stays the caller's to keep -- this class keeps it as arrays: policies, attributes, obstacles, the state it was first given, the fed
v_pref, tracker parameters, the list form and W with the block form's lists, the mission tables and their lists, the gate's margin and
cap, whether closest-approach records are on, the neighbour mode the run steps with.  A blob may hold vacant rows (BatchedSolver.retire):
solver() and MACAEnv.from_checkpoint load with vacancy=True, and a vacant row keeps its policy and attributes, so the definition holds them
as they stand at the save."""
import numpy as np

from . import _lib
from . import solver as S

_ATTR_KEYS = ('neighbor_dist', 'max_neighbors', 'time_step', 'time_horizon', 'max_speed', 'max_heading_change', 'dt_nominal')
_PARAM_KEYS = _ATTR_KEYS + ('near_goal_threshold',)


def _lists_arrays(prefix, lists):
    off, pts = S.paths_csr([[list(map(float, w[:3])) for w in p] for p in lists])
    return {prefix + '_off': off, prefix + '_pts': pts}


def _lists_of(d, prefix):
    off, pts = d[prefix + '_off'], d[prefix + '_pts']
    return [pts[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


class ContextCheckpoint:
    """definition: what define() returns; blob: a uint8 array (None: nothing to load -- solver() then builds the run's starting context);
    steps: the env updates behind which the blob was taken"""

    def __init__(self, definition, blob, steps=0):
        self.definition = dict(definition)
        self.blob = None if blob is None else np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray)) else blob, np.uint8).reshape(-1)
        self.steps = int(steps)

    def __len__(self):
        return len(self.definition['policy' if 'policy' in self.definition else 'agents_policy_id'])

    @staticmethod
    def define(radius, pref_speed, goal, policy, zaxis, max_run_dist, obstacles=None, state=None, vpref=None, params=None, agent_params=None, tracker=None,
               lists=None, missions=None, gate=None, clearance=False, neighbor_mode=S.NBR_KDTREE):
        """The definition as a dict of plain arrays.  obstacles: (pos (m, 3), radius (m,)); state: dict(pos, vel, heading, flags) -- the state
        the context is first given (None: zeros).  With a blob it is a placeholder only: a load needs SOME state set and overwrites every
        word of it; it matters for a checkpoint without a blob, the run's starting context.  neighbor_mode is kept for the caller
        (ContextCheckpoint.neighbor_mode: the mode to go on stepping with), nothing in solver() reads it; vpref: (vpref (n, 3), mode (n,)), the fed v_pref; params: sca_params fields the
        context is created with; agent_params: BatchedSolver.set_agent_params' arrays; tracker: dict(goal_heading (n, 3), turning_radius,
        pitchlims (lo, hi), and per agent turning_radius_pa / pitch_lo_pa / pitch_hi_pa); lists: ('block', paths) or ('slots', W, paths);
        missions: dict(M, R, entries (n, M) of _lib.MISSION_DTYPE, first_ok, first_fail, paths: one list per flat entry or None);
        gate: (margin, max_per_step)."""
        n = len(np.asarray(policy).reshape(-1))
        d = dict(radius=np.asarray(radius, np.float64).reshape(n), pref_speed=np.asarray(pref_speed, np.float64).reshape(n), goal=np.asarray(goal, np.float64).reshape(n, 3),
                 policy=np.asarray(policy, np.uint8).reshape(n), zaxis=np.asarray(zaxis, np.uint8).reshape(n), max_run_dist=np.asarray(max_run_dist, np.float64).reshape(n),
                 clearance=np.array([1 if clearance else 0], np.int32), neighbor_mode=np.array([int(neighbor_mode)], np.int32))
        pos, rad = obstacles if obstacles is not None else (np.zeros((0, 3)), np.zeros(0))
        d['obs_pos'], d['obs_radius'] = np.asarray(pos, np.float64).reshape(-1, 3), np.asarray(rad, np.float64).reshape(-1)
        st = state or dict(pos=np.zeros((n, 3)), vel=np.zeros((n, 3)), heading=np.zeros((n, 3)), flags=np.zeros(n))
        d.update(state_pos=np.asarray(st['pos'], np.float64).reshape(n, 3), state_vel=np.asarray(st['vel'], np.float32).reshape(n, 3),
                 state_heading=np.asarray(st['heading'], np.float64).reshape(n, 3), state_flags=np.asarray(st['flags'], np.uint8).reshape(n))
        if vpref is not None:
            d['vpref'], d['vpref_mode'] = np.asarray(vpref[0], np.float64).reshape(n, 3), np.asarray(vpref[1], np.uint8).reshape(n)
        for k, v in (params or {}).items():
            if k not in _PARAM_KEYS:
                raise ValueError('define: %r is no field of sca_params' % k)
            d['param_' + k] = np.array([v], np.int32 if k == 'max_neighbors' else np.float64)
        for k, v in (agent_params or {}).items():
            if k not in _ATTR_KEYS:
                raise ValueError('define: %r is no per-agent attribute' % k)
            if v is not None:
                d['attr_' + k] = np.asarray(v, np.int32 if k == 'max_neighbors' else np.float64).reshape(n)
        if tracker is not None:
            d['trk_goal_heading'] = np.asarray(tracker['goal_heading'], np.float64).reshape(n, 3)
            lo, hi = tracker.get('pitchlims', (-np.pi / 4, np.pi / 4))
            d['trk_scalars'] = np.array([tracker.get('turning_radius', 1.5), lo, hi], np.float64)
            if tracker.get('turning_radius_pa') is not None:
                d['trk_per_agent'] = np.stack([np.asarray(tracker[k], np.float64).reshape(n) for k in ('turning_radius_pa', 'pitch_lo_pa', 'pitch_hi_pa')])
        if lists is not None:
            form, W, paths = (lists[0], 0, lists[1]) if lists[0] == 'block' else lists
            if form not in ('block', 'slots') or len(paths) != n:
                raise ValueError("define: lists is ('block', paths) or ('slots', W, paths) with one list per agent")
            d['list_form'] = np.array([1 if form == 'block' else 2, int(W)], np.int32)
            d.update(_lists_arrays('lists', paths))
        if missions is not None:
            e = np.ascontiguousarray(missions['entries'], _lib.MISSION_DTYPE).reshape(n, int(missions['M']))
            d['ms_shape'] = np.array([int(missions['M']), int(missions['R'])], np.int32)
            d['ms_entries'] = np.frombuffer(e.tobytes(), np.uint8).copy()      # (the records as bytes: a structured dtype would need pickle's help)
            d['ms_first_ok'], d['ms_first_fail'] = np.asarray(missions['first_ok'], np.int32).reshape(n), np.asarray(missions['first_fail'], np.int32).reshape(n)
            if missions.get('paths') is not None:
                d.update(_lists_arrays('ms_lists', missions['paths']))
        if gate is not None:
            d['gate'] = np.array([float(gate[0]), float(gate[1])], np.float64)
        return d

    def solver(self, max_agents=None, device=0):
        """A fresh BatchedSolver with the definition set up in the order a context wants it and, if there is one, the blob loaded"""
        d, n = self.definition, len(self)
        params = {k[6:]: (int(v[0]) if k == 'param_max_neighbors' else float(v[0])) for k, v in d.items() if k.startswith('param_')}
        sol = S.BatchedSolver(max_agents=max(n, int(max_agents or n)), max_obstacles=max(1, len(d['obs_radius'])), device=device, params=params or None)
        try:
            sol.set_obstacles(d['obs_pos'], d['obs_radius'])
            sol.set_agents(d['radius'], d['pref_speed'], d['goal'], d['policy'], d['zaxis'], d['max_run_dist'])
            attrs = {k[5:]: v for k, v in d.items() if k.startswith('attr_')}
            if attrs:
                sol.set_agent_params(**attrs)
            if 'list_form' in d:
                form, W = (int(x) for x in d['list_form'])
                lists = _lists_of(d, 'lists')
                if form == 1:
                    sol.set_paths(lists)
                else:
                    sol.set_path_slots(W, lists)
            if 'vpref' in d:
                sol.set_vpref(d['vpref'], d['vpref_mode'])
            sol.set_state(d['state_pos'], d['state_vel'], d['state_heading'], d['state_flags'])
            if 'trk_goal_heading' in d:
                r, lo, hi = (float(x) for x in d['trk_scalars'])
                sol.device_tracker_enable(d['trk_goal_heading'], turning_radius=r, pitchlims=(lo, hi))
                if 'trk_per_agent' in d:
                    sol.device_tracker_set_agent_params(*d['trk_per_agent'])
            if int(d['clearance'][0]):
                sol.clearance_enable()
            if 'ms_shape' in d:
                M, R = (int(x) for x in d['ms_shape'])
                entries = np.frombuffer(d['ms_entries'].tobytes(), _lib.MISSION_DTYPE).reshape(n, M)
                sol.set_missions(M, R, entries, d['ms_first_ok'], d['ms_first_fail'], paths=_lists_of(d, 'ms_lists') if 'ms_lists_off' in d else None)
            if 'gate' in d:
                sol.set_mission_gate(float(d['gate'][0]), int(d['gate'][1]))
            if self.blob is not None:
                sol.load_context(self.blob, vacancy=True)            # (a blob may hold vacant rows; one without is what it always was)
        except BaseException:
            sol.close()
            raise
        return sol

    @property
    def neighbor_mode(self):
        return int(self.definition['neighbor_mode'][0])

    def write(self, path):
        """one .npz of plain arrays (readable with pickle refused); returns the path"""
        arrays = {'def_' + k: v for k, v in self.definition.items()}
        arrays['steps'] = np.array([self.steps], np.int64)
        if self.blob is not None:
            arrays['blob'] = self.blob
        with open(path, 'wb') as f:
            np.savez(f, **arrays)
        return path

    @classmethod
    def read(cls, path):
        with np.load(path, allow_pickle=False) as z:
            definition = {k[4:]: z[k] for k in z.files if k.startswith('def_')}
            return cls(definition, z['blob'] if 'blob' in z.files else None, int(z['steps'][0]))


# ---- a whole MACAEnv (MACAEnv.checkpoint / MACAEnv.from_checkpoint) ------------------------------------------------------------------------
# The definition at the env's level: the agents and obstacles as scenes.SceneCheckpoint.define keeps an episode's (rebuilt through their
# constructors), the env's options, and the mission tables -- every entry an Agent-like object, kept the same way -- with their successors,
# flags, lists, results room and gate.  The agents are kept AS THE ENV SHOWS THEM at the checkpoint (mission_results() has moved their
# goal / start / pref_speed mirrors to the entries they fly), their lists cut to what the passes have left: the context is set up from them
# and the blob then overwrites every word of the rows, so the mirrors and the device agree at once.
def _prefixed(prefix, d):
    return {prefix + k: np.asarray(v) for k, v in d.items()}


def _unprefixed(prefix, d):
    return {k[len(prefix):]: v for k, v in d.items() if k.startswith(prefix)}


def env_checkpoint(env):
    from . import scenes as _scenes
    if env.agents is None:
        raise RuntimeError('checkpoint: set_agents first')
    if env._row_cache is not None:
        raise RuntimeError('checkpoint: between a policy pass and its env update (agent.find_next_action was called): env.step() first')
    if env.v_pref_fn is not None:
        raise RuntimeError('checkpoint: a host-side v_pref_fn keeps per-agent state the env cannot save (use MACAEnv(device_tracker=True))')
    env._sync_paths()                                                # lists assigned since the last step go up first
    if env._paths_on:
        env._refresh_paths()                                         # ... and the agents' own are cut to what is left
    if env._paths_on and not env._path_slots:                        # block form: the lists AS SET are definition (whether a row was given one is read by the pass)
        lists = env._lists_set
    else:                                                            # slot form: lengths and rooms travel in the blob
        lists = [[list(map(float, w[:3])) for w in a._path] for a in env.agents]
    d = _prefixed('agents_', _scenes.SceneCheckpoint.define(env.agents, lists, env.obstacles))
    # (the agents above are the CURRENT ones: an attribute respawn's policies and attributes.  A sixth option only for an env with
    # attribute_slots: every other env writes the five it always wrote)
    d['env_options'] = np.array([int(env.neighbor_mode), int(env.device_tracker), int(env.clearance_on), int(env._path_slots), int(env._paths_on)] +
                                ([1] if env._attr_slots else []), np.int32)
    d['env_time_cum'] = np.asarray(env._time_cum, np.float64)
    if env._missions is not None:
        ids = sorted(env._missions)
        tabs = [env._missions[i] for i in ids]
        ents = [a for t in tabs for a, _, _ in t.entries]
        d.update(_prefixed('entries_', _scenes.SceneCheckpoint.define(ents, [p for t in tabs for p in t.paths], [])))
        d['entries_vel'] = np.array([a._vel for a in ents], np.float32).reshape(len(ents), 3)
        d['tables_ids'] = np.array(ids, np.int32)
        d['tables_k'] = np.array([len(t.entries) for t in tabs], np.int32)
        d['tables_first'] = np.array([[t.first_ok, t.first_fail] for t in tabs], np.int32).reshape(len(tabs), 2)
        d['tables_next'] = np.array([[t.next_ok[j], t.next_fail[j]] for t in tabs for j in range(len(t.entries))], np.int32).reshape(len(ents), 2)
        d['tables_flags'] = np.array([[here, keep] for t in tabs for _, here, keep in t.entries], np.uint8).reshape(len(ents), 2)
        results, margin, cap = env._mission_args
        d['tables_args'] = np.array([results, -1.0 if margin is None else margin, -1 if cap is None else cap], np.float64)
        pend = sorted(env._mission_pending)
        d['pending_ids'] = np.array(pend, np.int32)
        d['pending_entry'] = np.array([env._mission_pending[i][0] for i in pend], np.int32)
        d['pending_pos'] = np.array([env._mission_pending[i][1] for i in pend], np.float64).reshape(len(pend), 3)
    # (vacant rows, MACAEnv.retire: they are in the blob; env.agents keeps their objects, so the definition has their policies and attributes)
    return ContextCheckpoint(d, env.solver.save_context(vacancy=True), len(env._time_cum) - 1)


def env_from_checkpoint(cls, ckpt, device=0):
    from . import env as _env
    from . import scenes as _scenes
    d = ckpt.definition
    if 'env_options' not in d:
        raise ValueError('from_checkpoint: the checkpoint holds a solver-level definition (ContextCheckpoint.define), not an env -- .solver() resumes it')
    mode, tracker, clearance, slots, paths_on = (int(x) for x in d['env_options'][:5])
    attr_slots = len(d['env_options']) > 5 and bool(d['env_options'][5])      # (a checkpoint from before attribute_slots holds five options)
    whole = _scenes.SceneCheckpoint(_unprefixed('agents_', d), np.zeros(0, np.uint8), 0)
    agents = whole.agents()
    env = cls(device=device, neighbor_mode=mode, device_tracker=bool(tracker), clearance=bool(clearance), path_slots=slots, attribute_slots=attr_slots)
    env.set_agents(agents, obstacles=whole.obstacles())
    if 'tables_ids' in d:
        ents = _scenes.SceneCheckpoint(_unprefixed('entries_', d), np.zeros(0, np.uint8), 0).agents()
        for a, v in zip(ents, d['entries_vel']):
            a._vel = np.array(v, np.float32)
        tables, at = {}, 0
        for t, (i, k) in enumerate(zip(d['tables_ids'], d['tables_k'])):
            rows = slice(at, at + int(k))
            tables[int(i)] = _env.MissionTable(ents[rows], d['tables_next'][rows, 0], d['tables_next'][rows, 1], first_ok=int(d['tables_first'][t, 0]),
                                               first_fail=int(d['tables_first'][t, 1]), start_here=[bool(x) for x in d['tables_flags'][rows, 0]],
                                               keep_zaxis=[bool(x) for x in d['tables_flags'][rows, 1]], path=[a._path for a in ents[rows]])
            at += int(k)
        results, margin, cap = d['tables_args']
        env.set_missions(tables, results=int(results), spawn_margin=None if margin < 0 else float(margin), max_per_step=None if cap < 0 else int(cap))
        env._mission_pending = {int(i): (int(j), np.array(p, np.float64)) for i, j, p in zip(d['pending_ids'], d['pending_entry'], d['pending_pos'])}
    env.solver.load_context(ckpt.blob, vacancy=True)                # (the mirrors are stale from here: Agent.is_vacant, env.vacant and env.population read the loaded rows)
    env._time_cum = [float(x) for x in d['env_time_cum']]
    env._active = env.solver.active_count()
    env._path_assigned = set()
    env._stale = True
    env._path_stale = env._paths_on
    env._nbr_cache = env._vpref_cache = None
    return env
