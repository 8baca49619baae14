"""BatchedSolver: numpy-facing wrapper of one libsca_hip context (include/sca_hip.h).

All heavy lifting happens in the HIP kernels; this class only marshals arrays.  It mirrors the quantities the
reference keeps on its Agent objects (mamp/agents/agent.py) as structure-of-arrays.
"""
import ctypes as C
import math

import numpy as np

from . import _lib

POL_SCA, POL_RVO3D, POL_SRVO3D, POL_ORCA3D, POL_ORCA3D_LP, POL_RVO3D_DUBINS = range(6)
FLAG_AT_GOAL, FLAG_COLLISION, FLAG_TIMEOUT = 1, 2, 4
CHECKPOINT_VACANCY = 1                                          # SCA_CHECKPOINT_VACANCY: a context checkpoint that carries vacant rows
FLAG_VACANT = 8                                                 # a vacant row (retire): always with at-goal | collision, get_state shows 11
MISSION_START_HERE, MISSION_KEEP_ZAXIS = 1, 2                  # sca_mission_flag
SPAWN_ADMITTED, SPAWN_BLOCKED_AGENT, SPAWN_BLOCKED_OBSTACLE, SPAWN_BLOCKED_ENTRY = 0, 1, 2, 3      # SCA_SPAWN_*: a gated respawn's verdict per row
SPAWN_OVER_CAP = 4                                               # ... and, under set_mission_gate only, "not tested in this step"
NBR_KDTREE, NBR_GRID, NBR_KDTREE_HOSTBUILD, NBR_AUTO = 0, 1, 2, 3
FORM_SOLVE_SPLIT, FORM_TRACK_FUSED, FORM_REPLAN_LANE, FORM_REPLAN_FEW, FORM_LP_LANE, FORM_SOLVE_FB, FORM_ACTION_FB, FORM_AUTO_TAIL = 1, 2, 4, 8, 16, 32, 64, 128   # sca_last_pass_forms
FORM_WAYPOINTS = 256                                          # k_waypoint ran (waypoint lists are set)
FORM_SCENES = 512                                             # scenes are set: forest build, scene forms of K1 / K4
FORM_SCENE_OBSTACLES = 1024                                   # ... with one obstacle set per scene (set_scene_obstacles)
FORM_VACANCY = 2048                                           # a row is vacant (retire): the tree holds the occupied rows, NBR_AUTO was the kd pass
K = _lib.K
_ATTR_NAMES = tuple(name for name, _ in _lib.RestartAttrs._fields_[2:])   # sca_restart_attrs' arrays, in the struct's order


class ScaError(RuntimeError):
    pass


class _BlockOwner:
    """What a view of the host state block holds on to: the solver, whose context owns the page-locked memory."""
    def __init__(self, solver):
        self.solver = solver


class BatchedSolver:
    def __init__(self, max_agents, max_obstacles=0, device=0, params=None):
        self.L = _lib.lib()
        p = _lib.Params()
        self.L.sca_default_params_v2(C.byref(p), C.sizeof(p))
        for k, v in (params or {}).items():
            setattr(p, k, v)
        self.params = p
        self.ctx = C.c_void_p()
        rc = self.L.sca_create(C.byref(p), int(device), int(max_agents), int(max_obstacles), C.byref(self.ctx))
        if rc != 0:
            msg = self.L.sca_last_error(self.ctx).decode() if self.ctx else 'sca_create failed'
            if self.ctx:
                self.L.sca_destroy(self.ctx)
                self.ctx = None
            raise ScaError(f'sca_create: {msg} (rc={rc})')
        self.n = 0
        self.m = 0
        self.nscenes = 0
        self.scene_offsets = None
        self._host_state = None
        self._harvest = None

    def close(self):
        if getattr(self, 'ctx', None):
            self.L.sca_destroy(self.ctx)                          # (frees the host state block: views of it must not be used after close())
            self.ctx = None
        self._host_state = None
        self._harvest = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise ScaError(f'{what}: {self.L.sca_last_error(self.ctx).decode()} (rc={rc})')

    # ---- static scene ------------------------------------------------------------------------------
    def set_obstacles(self, pos, radius):
        pos = _lib.as_d(pos).reshape(-1, 3)
        radius = _lib.as_d(radius).reshape(-1)
        self.m = len(radius)
        self._chk(self.L.sca_set_obstacles(self.ctx, self.m, _lib.ptr(pos, C.c_double), _lib.ptr(radius, C.c_double)),
                  'sca_set_obstacles')

    def set_agents(self, radius, pref_speed, goal, policy, zaxis=None, max_run_dist=None):
        radius = _lib.as_d(radius).reshape(-1)
        n = len(radius)
        pref_speed = _lib.as_d(np.broadcast_to(pref_speed, (n,)))
        goal = _lib.as_d(goal).reshape(n, 3)
        policy = np.ascontiguousarray(np.broadcast_to(policy, (n,)), np.uint8)
        zaxis = np.zeros(n, np.uint8) if zaxis is None else np.ascontiguousarray(zaxis, np.uint8)
        mrd = np.full(n, np.inf) if max_run_dist is None else _lib.as_d(max_run_dist).reshape(n)
        self.n = n
        self._host_state = None                                   # the block's layout follows n: host_state() fetches it again
        self.nscenes = 0                                          # (sca_set_agents clears the scenes)
        self.scene_offsets = None
        self._harvest = None                                      # (... and with them the harvest block)
        self._chk(self.L.sca_set_agents(self.ctx, n, _lib.ptr(radius, C.c_double), _lib.ptr(pref_speed, C.c_double),
                                        _lib.ptr(goal, C.c_double), _lib.ptr(policy, C.c_uint8),
                                        _lib.ptr(zaxis, C.c_uint8), _lib.ptr(mrd, C.c_double)), 'sca_set_agents')

    def set_agent_params(self, neighbor_dist=None, max_neighbors=None, time_step=None, time_horizon=None, max_speed=None,
                         max_heading_change=None, dt_nominal=None):
        """The solver attributes per agent (the reference keeps them on every Agent object, agent.py:24-41): arrays of n, None = the context's
        value for everybody; with no argument: back to one value per context.  After set_agents, before device_tracker_enable."""
        n = self.n
        keep = []

        def arr(a, dt, ct):
            if a is None:
                return None
            b = np.ascontiguousarray(np.broadcast_to(a, (n,)), dt)
            keep.append(b)
            return _lib.ptr(b, ct)
        args = [arr(neighbor_dist, np.float64, C.c_double), arr(max_neighbors, np.int32, C.c_int32), arr(time_step, np.float64, C.c_double),
                arr(time_horizon, np.float64, C.c_double), arr(max_speed, np.float64, C.c_double), arr(max_heading_change, np.float64, C.c_double),
                arr(dt_nominal, np.float64, C.c_double)]
        self._chk(self.L.sca_set_agent_params(self.ctx, n if keep else 0, *args), 'sca_set_agent_params')

    # ---- dynamic state -------------------------------------------------------------------------------
    def set_state(self, pos, vel, heading, flags, total_dist=None, step_num=None):
        n = self.n
        pos = _lib.as_d(pos).reshape(n, 3)
        vel = np.ascontiguousarray(vel, np.float32).reshape(n, 3)
        heading = _lib.as_d(heading).reshape(n, 3)
        flags = np.ascontiguousarray(flags, np.uint8).reshape(n)
        td = None if total_dist is None else _lib.as_d(total_dist).reshape(n)
        sn = None if step_num is None else np.ascontiguousarray(step_num, np.int32).reshape(n)
        self._chk(self.L.sca_set_state(self.ctx, _lib.ptr(pos, C.c_double), _lib.ptr(vel, C.c_float),
                                       _lib.ptr(heading, C.c_double), _lib.ptr(flags, C.c_uint8),
                                       None if td is None else _lib.ptr(td, C.c_double),
                                       None if sn is None else _lib.ptr(sn, C.c_int32)), 'sca_set_state')

    def get_state(self):
        n = self.n
        out = dict(pos=np.zeros((n, 3)), vel=np.zeros((n, 3), np.float32), heading=np.zeros((n, 3)),
                   flags=np.zeros(n, np.uint8), total_dist=np.zeros(n), step_num=np.zeros(n, np.int32))
        self._chk(self.L.sca_get_state(self.ctx, _lib.ptr(out['pos'], C.c_double), _lib.ptr(out['vel'], C.c_float),
                                       _lib.ptr(out['heading'], C.c_double), _lib.ptr(out['flags'], C.c_uint8),
                                       _lib.ptr(out['total_dist'], C.c_double), _lib.ptr(out['step_num'], C.c_int32)),
                  'sca_get_state')
        return out

    def set_kd_perm(self, perm):
        perm = np.ascontiguousarray(perm, np.int32).reshape(self.n)
        self._chk(self.L.sca_set_kd_perm(self.ctx, _lib.ptr(perm, C.c_int32)), 'sca_set_kd_perm')

    def get_kd_perm(self):
        perm = np.zeros(self.n, np.int32)
        self._chk(self.L.sca_get_kd_perm(self.ctx, _lib.ptr(perm, C.c_int32)), 'sca_get_kd_perm')
        return perm

    def get_kd_tree(self):
        t = np.zeros((2 * self.n - 1, 10))
        self._chk(self.L.sca_get_kd_tree(self.ctx, _lib.ptr(t, C.c_double)), 'sca_get_kd_tree')
        return t

    def set_vpref(self, vpref, mode):
        vpref = _lib.as_d(np.nan_to_num(vpref)).reshape(self.n, 3)
        mode = np.ascontiguousarray(np.broadcast_to(mode, (self.n,)), np.uint8)
        self._chk(self.L.sca_set_vpref(self.ctx, _lib.ptr(vpref, C.c_double), _lib.ptr(mode, C.c_uint8)), 'sca_set_vpref')

    # ---- waypoint lists: Agent.path + policy.now_goal (agent.py:44, get_trajectory e.g. rvo3dPolicy.py:71-85) --------------------
    def set_paths(self, paths):
        """One list of [x, y, z] waypoints per agent (list order; the reference pops from the end), or None / [] for no lists at all.
        Resets every cursor and now_goal (None).  After set_agents."""
        if paths is None or len(paths) == 0:
            self._chk(self.L.sca_set_paths(self.ctx, 0, None, None), 'sca_set_paths')
            return
        off, pts = paths_csr(paths)
        self._chk(self.L.sca_set_paths(self.ctx, len(paths), _lib.ptr(off, C.c_int32), _lib.ptr(pts, C.c_double)), 'sca_set_paths')

    def set_path_slots(self, W, paths=None):
        """The lists in SLOT form (sca_set_path_slots): every agent row owns room for W waypoints, so restart_scenes(paths=...) can replace
        the lists of one scene while the others keep running.  paths: as set_paths', no list longer than W; None: every list empty.
        Resets every cursor and now_goal (None).  set_paths puts the context back into block form."""
        if paths is None:
            self._chk(self.L.sca_set_path_slots(self.ctx, int(W), self.n, None, None), 'sca_set_path_slots')
            return
        off, pts = paths_csr(paths)
        self._chk(self.L.sca_set_path_slots(self.ctx, int(W), len(paths), _lib.ptr(off, C.c_int32), _lib.ptr(pts, C.c_double)), 'sca_set_path_slots')

    @property
    def path_slots(self):
        """the room per agent row, in waypoints, while the lists are in slot form; 0 otherwise (sca_get_path_slots)"""
        w = C.c_int(0)
        self._chk(self.L.sca_get_path_slots(self.ctx, C.byref(w)), 'sca_get_path_slots')
        return int(w.value)

    def get_path_state(self):
        """(remaining [n] int32: elements still in each list, now_goal [n, 3]: NaN rows = None)"""
        rem = np.zeros(self.n, np.int32)
        ng = np.zeros((self.n, 3))
        self._chk(self.L.sca_get_path_state(self.ctx, _lib.ptr(rem, C.c_int32), _lib.ptr(ng, C.c_double)), 'sca_get_path_state')
        return rem, ng

    def path_slot_lists(self):
        """(len [n] int32, rooms [n, W, 3]): the lists as the rows hold them in slot form (sca_get_path_slot_lists) -- row a's list is
        rooms[a, :len[a]], in list order; what stands behind it is whatever an earlier list left there"""
        W = self.path_slots
        ln, rooms = np.zeros(self.n, np.int32), np.zeros((self.n, max(W, 1), 3))
        self._chk(self.L.sca_get_path_slot_lists(self.ctx, _lib.ptr(ln, C.c_int32), _lib.ptr(rooms, C.c_double)), 'sca_get_path_slot_lists')
        return ln, rooms

    def vpref_mode(self):
        """the rows' vpref_mode bytes as the next pass will read them (sca_get_vpref_mode)"""
        mode = np.zeros(self.n, np.uint8)
        self._chk(self.L.sca_get_vpref_mode(self.ctx, _lib.ptr(mode, C.c_uint8)), 'sca_get_vpref_mode')
        return mode

    def set_path_state(self, remaining, now_goal):
        rem = np.ascontiguousarray(remaining, np.int32).reshape(self.n)
        ng = _lib.as_d(now_goal).reshape(self.n, 3)
        self._chk(self.L.sca_set_path_state(self.ctx, _lib.ptr(rem, C.c_int32), _lib.ptr(ng, C.c_double)), 'sca_set_path_state')

    # ---- scene batches: many isolated episodes in one context (sca_set_scenes) ------------------------------------------
    def set_scenes(self, offsets):
        """Scene s = agents [offsets[s], offsets[s + 1]); None / [] for a plain context again.  After set_agents; resets the kd permutation to
        the identity and the per-scene counters.  A scene holds at most 1536 agents."""
        self._harvest = None                                      # (redefining or clearing the scenes drops the harvest block)
        if offsets is None or len(offsets) == 0:
            self._chk(self.L.sca_set_scenes(self.ctx, 0, None), 'sca_set_scenes')
            self.nscenes = 0
            self.scene_offsets = None
            return
        off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        self._chk(self.L.sca_set_scenes(self.ctx, len(off) - 1, _lib.ptr(off, C.c_int32)), 'sca_set_scenes')
        self.nscenes = len(off) - 1
        self.scene_offsets = off.copy()

    def set_scene_obstacles(self, lists):
        """One (pos [m_s, 3], radius [m_s]) pair per scene: scene s meets its own obstacles and no others (m_s may be 0).  After set_scenes;
        a later set_obstacles puts the context back on one shared set, and whatever clears or redefines the scenes (set_agents, set_scenes)
        leaves it without obstacles.  Obstacle ids in neighbors() are global: scene_obstacle_offsets[s] + the scene's own id."""
        if len(lists) != self.nscenes:
            raise ValueError(f'set_scene_obstacles: {len(lists)} obstacle sets for {self.nscenes} scenes')
        radius = [_lib.as_d(r).reshape(-1) for _, r in lists]
        pos = [_lib.as_d(p) for p, _ in lists]
        for s, (p, r) in enumerate(zip(pos, radius)):
            if p.size != 3 * len(r):
                raise ValueError(f'set_scene_obstacles: scene {s} has {p.size} coordinates for {len(r)} radii')
        pos = [p.reshape(len(r), 3) for p, r in zip(pos, radius)]
        off = np.zeros(len(lists) + 1, np.int32)
        off[1:] = np.cumsum([len(r) for r in radius])
        allp = np.ascontiguousarray(np.concatenate(pos)) if len(pos) else np.zeros((0, 3))
        allr = np.ascontiguousarray(np.concatenate(radius)) if len(radius) else np.zeros(0)
        self._chk(self.L.sca_set_scene_obstacles(self.ctx, len(lists), _lib.ptr(off, C.c_int32), _lib.ptr(allp, C.c_double), _lib.ptr(allr, C.c_double)),
                  'sca_set_scene_obstacles')
        self.m = int(off[-1])
        self.scene_obstacle_offsets = off

    def set_scene_obstacle_slots(self, capacities, sets=None):
        """Obstacle slots (sca_set_scene_obstacle_slots): scene s may hold up to capacities[s] obstacles and starts with sets[s] = (pos
        [m_s, 3], radius [m_s]), m_s <= capacities[s]; None (for the list or an entry): empty.  A later restart_scenes(obstacles=...) replaces
        a scene's set.  Obstacle ids in neighbors() are global: scene_obstacle_offsets[s] + the scene's own id."""
        caps = np.ascontiguousarray(capacities, np.int64).reshape(-1)
        if len(caps) != self.nscenes:
            raise ValueError(f'set_scene_obstacle_slots: {len(caps)} capacities for {self.nscenes} scenes')
        if sets is not None and len(sets) != self.nscenes:
            raise ValueError(f'set_scene_obstacle_slots: {len(sets)} obstacle sets for {self.nscenes} scenes')
        off = np.zeros(len(caps) + 1, np.int32)
        off[1:] = np.cumsum(caps)
        counts, allp, allr = self._pack_obstacle_sets(sets if sets is not None else [None] * len(caps), 'set_scene_obstacle_slots')
        counts = np.maximum(counts, 0)                            # (None: empty)
        self._chk(self.L.sca_set_scene_obstacle_slots(self.ctx, len(caps), _lib.ptr(off, C.c_int32), _lib.ptr(counts, C.c_int32),
                                                      _lib.ptr(allp, C.c_double), _lib.ptr(allr, C.c_double)), 'sca_set_scene_obstacle_slots')
        self.m = int(off[-1])
        self.scene_obstacle_offsets = off

    @staticmethod
    def _pack_obstacle_sets(sets, who):
        """counts [len(sets)] int32 (-1 for None), pos [sum, 3], radius [sum]: the sets packed in order"""
        counts = np.full(len(sets), -1, np.int32)
        pos, radius = [np.zeros((0, 3))], [np.zeros(0)]
        for e, st in enumerate(sets):
            if st is None:
                continue
            r = _lib.as_d(st[1]).reshape(-1)
            p = _lib.as_d(st[0])
            if p.size != 3 * len(r):
                raise ValueError(f'{who}: set {e} has {p.size} coordinates for {len(r)} radii')
            counts[e] = len(r)
            pos.append(p.reshape(len(r), 3))
            radius.append(r)
        return counts, np.ascontiguousarray(np.concatenate(pos)), np.ascontiguousarray(np.concatenate(radius))

    def scene_obstacle_counts(self):
        """dict(counts [B] int32: the obstacles each scene holds, capacities [B] int32) (sca_get_scene_obstacle_counts)"""
        out = dict(counts=np.zeros(self.nscenes, np.int32), capacities=np.zeros(self.nscenes, np.int32))
        self._chk(self.L.sca_get_scene_obstacle_counts(self.ctx, _lib.ptr(out['counts'], C.c_int32), _lib.ptr(out['capacities'], C.c_int32)),
                  'sca_get_scene_obstacle_counts')
        return out

    def restart_scenes(self, ids, pos, heading, vel=None, radius=None, pref_speed=None, goal=None, policy=None, zaxis=None, max_run_dist=None,
                       goal_heading=None, sizes=None, obstacles=None, attrs=None, paths=None):
        """New episodes into the scenes `ids` while the others keep running (sca_restart_scenes).  The arrays hold T rows, the named scenes'
        agents in the order of `ids`; None keeps the slot's values (vel: zero).  Afterwards each named scene is what a context of that
        episode alone is after set_agents + set_state (+ device_tracker_enable); its per-agent attributes stay, and its obstacle set unless
        `obstacles` replaces it.
        sizes (sca_restart_scenes_sized): the agents each named scene takes, 1 .. its capacity (the length of its range) -- T is their sum,
        and the rows of the range behind them are vacant; None fills every named scene to its capacity.
        obstacles (sca_restart_scenes_obstacles; obstacle slots set): per named scene None -- it keeps its set -- or (pos [m, 3], radius [m])
        with m at most the slot's obstacle capacity -- its set is replaced.  None: every named scene keeps its set.
        attrs (sca_restart_scenes_attrs): a dict -- the named scenes' rows take the episode's own attributes: neighbor_dist, max_neighbors,
        time_step, time_horizon, max_speed, max_heading_change, dt_nominal (set_agent_params' names) and, with the device tracker on,
        turning_radius, pitch_lo, pitch_hi, each an array of T rows or a scalar for all of them.  A name that is absent means the value a
        context alone would have -- its sca_params, device_tracker_enable's value -- not what the row had; {} puts every named row back
        on those.  A policy may then move an agent between tracked and untracked.  None: the slots keep their attributes (the entry
        points above); 'keep': the same through sca_restart_scenes_attrs with attrs == NULL, which is exactly that call.
        paths (sca_restart_scenes_paths; the lists in slot form, set_path_slots): one list of [x, y, z] waypoints per packed row, T in all,
        none longer than the room per row -- the named scenes' rows take the episode's own lists.  None: the call brings none (in slot
        form the named rows then get empty lists)."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        keep = [ids]
        if obstacles is not None and len(obstacles) != len(ids):
            raise ValueError(f'restart_scenes: {len(obstacles)} obstacle sets for {len(ids)} scenes')
        if sizes is not None:
            sizes = np.ascontiguousarray(sizes, np.int32).reshape(-1)
            if len(sizes) != len(ids):
                raise ValueError(f'restart_scenes: {len(sizes)} sizes for {len(ids)} scenes')
            keep.append(sizes)
        # T, where the ids name scenes of this context (else the library refuses the call before it reads an array): every array is held
        # against it here, because the library cannot know how long the caller's buffers are
        off = self.scene_offsets
        T = None
        if off is not None and len(ids) and ids.min() >= 0 and ids.max() < self.nscenes:
            T = int((off[ids + 1] - off[ids]).sum())
            if sizes is not None and sizes.min() >= 1 and (sizes <= off[ids + 1] - off[ids]).all():
                T = int(sizes.sum())                               # (else the library refuses the call, naming the entry)

        def arr(a, dt, ct, cols):
            if a is None:
                return None
            b = np.ascontiguousarray(a, dt)
            if T is not None and b.size != T * (cols or 1):
                raise ValueError(f'restart_scenes: an array of {b.size} values where the named scenes hold {T} agents x {cols or 1}')
            b = b.reshape((-1, cols) if cols else (-1,))
            keep.append(b)
            return _lib.ptr(b, ct)
        d3 = lambda a: arr(a, np.float64, C.c_double, 3)
        d1 = lambda a: arr(a, np.float64, C.c_double, 0)
        u1 = lambda a: arr(a, np.uint8, C.c_uint8, 0)
        rest = (d3(pos), arr(vel, np.float32, C.c_float, 3), d3(heading), d1(radius), d1(pref_speed), d3(goal), u1(policy), u1(zaxis), d1(max_run_dist),
                d3(goal_heading))
        path_args = None
        if paths is not None:
            if T is not None and len(paths) != T:
                raise ValueError(f'restart_scenes: {len(paths)} waypoint lists where the named scenes hold {T} agents')
            poff, ppts = paths_csr(paths)
            keep += [poff, ppts]
            path_args = (_lib.ptr(poff, C.c_int32), _lib.ptr(ppts, C.c_double))
            attrs = 'keep' if attrs is None else attrs                # (sca_restart_scenes_paths with attrs == NULL: the slots keep theirs)
        if attrs is not None:
            keep_attrs = isinstance(attrs, str)
            if keep_attrs and attrs != 'keep':
                raise ValueError(f"restart_scenes: attrs is None, 'keep' or a dict, got {attrs!r}")
            unknown = [] if keep_attrs else sorted(set(attrs) - set(_ATTR_NAMES))
            if unknown:
                raise ValueError(f'restart_scenes: attrs names {unknown}, sca_restart_attrs has {list(_ATTR_NAMES)}')
            desc = _lib.RestartAttrs(struct_bytes=C.sizeof(_lib.RestartAttrs), reserved=0)
            for name, v in ({} if keep_attrs else attrs).items():
                if v is None:
                    continue
                i32 = name == 'max_neighbors'
                v = np.asarray(v, np.int32 if i32 else np.float64)
                if v.ndim == 0 and T is not None:
                    v = np.full(T, v)
                setattr(desc, name, arr(v, np.int32 if i32 else np.float64, C.c_int32 if i32 else C.c_double, 0))
            ocnt, opos, orad = self._pack_obstacle_sets(obstacles, 'restart_scenes') if obstacles is not None else (None, None, None)
            op = lambda a, ct: None if a is None else _lib.ptr(a, ct)
            head = (self.ctx, len(ids), _lib.ptr(ids, C.c_int32), None if sizes is None else _lib.ptr(sizes, C.c_int32),
                    op(ocnt, C.c_int32), op(opos, C.c_double), op(orad, C.c_double), None if keep_attrs else C.byref(desc))
            if path_args is not None:
                self._chk(self.L.sca_restart_scenes_paths(*head, *path_args, *rest), 'sca_restart_scenes_paths')
            else:
                self._chk(self.L.sca_restart_scenes_attrs(*head, *rest), 'sca_restart_scenes_attrs')
        elif obstacles is not None:
            ocnt, opos, orad = self._pack_obstacle_sets(obstacles, 'restart_scenes')
            self._chk(self.L.sca_restart_scenes_obstacles(self.ctx, len(ids), _lib.ptr(ids, C.c_int32), None if sizes is None else _lib.ptr(sizes, C.c_int32),
                                                          _lib.ptr(ocnt, C.c_int32), _lib.ptr(opos, C.c_double), _lib.ptr(orad, C.c_double), *rest),
                      'sca_restart_scenes_obstacles')
        elif sizes is None:
            self._chk(self.L.sca_restart_scenes(self.ctx, len(ids), _lib.ptr(ids, C.c_int32), *rest), 'sca_restart_scenes')
        else:
            self._chk(self.L.sca_restart_scenes_sized(self.ctx, len(ids), _lib.ptr(ids, C.c_int32), _lib.ptr(sizes, C.c_int32), *rest),
                      'sca_restart_scenes_sized')

    def scene_sizes(self):
        """[B] int32: the agents each scene holds, in the first rows of its range (sca_get_scene_sizes); the range's length unless a sized
        restart said otherwise"""
        out = np.zeros(self.nscenes, np.int32)
        self._chk(self.L.sca_get_scene_sizes(self.ctx, _lib.ptr(out, C.c_int32)), 'sca_get_scene_sizes')
        return out

    def scene_state(self):
        """dict(active [B] int32: agents of each scene the next step would serve, steps [B] int32: steps taken while the scene was live)"""
        b = self.nscenes
        out = dict(active=np.zeros(b, np.int32), steps=np.zeros(b, np.int32))
        self._chk(self.L.sca_get_scene_state(self.ctx, _lib.ptr(out['active'], C.c_int32), _lib.ptr(out['steps'], C.c_int32)), 'sca_get_scene_state')
        return out

    # ---- a trajectory log per scene (sca_scene_history_enable) -----------------------------------------------------------
    def scene_history_enable(self, rows):
        """`rows` per scene (0 frees the log).  Behind set_scenes / set_state, before the first step.  Row r of a scene is its r-th own step:
        a finished scene gains no row, a restarted one starts over at row 0."""
        self._chk(self.L.sca_scene_history_enable(self.ctx, int(rows)), 'sca_scene_history_enable')

    def scene_history_rows(self):
        """dict(logged [B] int32, dropped [B] int32): steps beyond the capacity are counted, never written"""
        b = self.nscenes
        out = dict(logged=np.zeros(b, np.int32), dropped=np.zeros(b, np.int32))
        self._chk(self.L.sca_scene_history_rows(self.ctx, _lib.ptr(out['logged'], C.c_int32), _lib.ptr(out['dropped'], C.c_int32)), 'sca_scene_history_rows')
        return out

    def scene_history(self, scene, first_row=0, nrows=None, agent_begin=0, agent_count=None):
        """Rows [first_row, first_row+nrows) of scene-local agents [agent_begin, +agent_count) of one scene: dict of [nrows, agents, 3] arrays."""
        scene = int(scene)
        inside = self.scene_offsets is not None and 0 <= scene < self.nscenes
        if nrows is None:
            nrows = int(self.scene_history_rows()['logged'][scene]) - first_row if inside else 0
        if agent_count is None:
            agent_count = int(self.scene_sizes()[scene]) - agent_begin if inside else 0
        shape = (max(0, int(nrows)), max(0, int(agent_count)), 3)                # (a window the library will refuse still gets arrays it could fill)
        out = dict(pos=np.zeros(shape), heading=np.zeros(shape), vel=np.zeros(shape, np.float32))
        self._chk(self.L.sca_get_scene_history(self.ctx, scene, int(first_row), int(nrows), int(agent_begin), int(agent_count),
                                               _lib.ptr(out['pos'], C.c_double), _lib.ptr(out['heading'], C.c_double),
                                               _lib.ptr(out['vel'], C.c_float)), 'sca_get_scene_history')
        return out

    # ---- finished scenes hand over their result with the step (sca_scene_harvest_enable) ----------------------------------
    def scene_harvest_enable(self, on=True):
        """From now on every step ends with k_scene_harvest: the scenes' counters, and the rows and summary of every scene that finished in
        the step, stand in a page-locked block after the step's own synchronisation (scene_harvest(), scene_harvest_collect()).  on=False
        frees the block: views handed out before must not be used any more."""
        self._harvest = None
        self._chk(self.L.sca_scene_harvest_enable(self.ctx, 1 if on else 0), 'sca_scene_harvest_enable')

    def scene_harvest(self):
        """The harvest block as a dict of numpy VIEWS (no copies), made once per scene_harvest_enable: active, steps (B,) i32 -- every step --;
        summary (B,) records (_lib.SUMMARY_DTYPE); pos (n, 3) f64, vel (n, 3) f32, heading (n, 3) f64, flags (n,) u8, total_dist (n,) f64,
        step_num (n,) i32 -- rows [offsets[s], offsets[s] + size[s]) of a scene once it has finished, valid until it is restarted or finishes
        again.  The views keep the solver alive; set_agents, set_scenes, scene_harvest_enable and close() free the block under them."""
        if self._harvest is None:
            h = _lib.SceneHarvest()
            self._chk(self.L.sca_scene_harvest_get(self.ctx, C.byref(h), C.sizeof(h)), 'sca_scene_harvest_get')
            n, b = h.n, h.nscenes
            owner = _BlockOwner(self)

            def view(p, ct, dt, shape):
                count = int(np.prod(shape))
                buf = (ct * count).from_address(C.addressof(p.contents))
                buf._sca_owner = owner
                return np.frombuffer(buf, dtype=dt, count=count).reshape(shape)
            counters = view(h.counters, C.c_int32, np.int32, (b, 2))
            self._harvest = dict(
                active=counters[:, 0], steps=counters[:, 1], summary=view(h.summary, _lib.SceneSummary, _lib.SUMMARY_DTYPE, (b,)),
                pos=view(h.pos, C.c_double, np.float64, (n, 3)), vel=view(h.vel, C.c_float, np.float32, (n, 3)),
                heading=view(h.heading, C.c_double, np.float64, (n, 3)), flags=view(h.flags, C.c_uint8, np.uint8, (n,)),
                total_dist=view(h.total_dist, C.c_double, np.float64, (n,)), step_num=view(h.step_num, C.c_int32, np.int32, (n,)))
        return self._harvest

    def scene_harvest_collect(self):
        """The scenes that finished since the last call, a list of ids in ascending (batch step, id); synchronises the context's stream
        (nothing to wait for directly behind env_step).  An uncollected scene that is restarted is never reported."""
        ids = np.zeros(max(1, self.nscenes), np.int32)
        count = C.c_int32(0)
        self._chk(self.L.sca_scene_harvest_collect(self.ctx, _lib.ptr(ids, C.c_int32), C.byref(count)), 'sca_scene_harvest_collect')
        return [int(s) for s in ids[:count.value]]

    # ---- closest approach per agent, measured with the step (sca_scene_clearance_enable) ------------------------------------
    def scene_clearance_enable(self, on=True):
        """From now on every step runs k_scene_clearance: every occupied agent row keeps how close it came to another agent and to an
        obstacle of its scene, with whom and at which of the scene's steps (include/sca_hip.h has the rule).  Every row starts empty;
        on=False frees the records."""
        self._chk(self.L.sca_scene_clearance_enable(self.ctx, 1 if on else 0), 'sca_scene_clearance_enable')

    def scene_clearance(self, scene):
        """The records of one scene's occupied rows, a structured array (_lib.CLEARANCE_DTYPE: agent_clear, obs_clear f64, agent_partner,
        agent_step, obs_partner, obs_step i32; an empty half is +inf, -1, 0).  One copy, one synchronisation."""
        scene = int(scene)
        inside = self.scene_offsets is not None and 0 <= scene < self.nscenes
        out = np.zeros(int(self.scene_sizes()[scene]) if inside else 1, _lib.CLEARANCE_DTYPE)      # (a scene the library will refuse still gets a buffer)
        self._chk(self.L.sca_get_scene_clearance(self.ctx, scene, out.ctypes.data_as(C.POINTER(_lib.SceneClearance)), _lib.CLEARANCE_DTYPE.itemsize),
                  'sca_get_scene_clearance')
        return out

    # ---- closest approach per agent for the whole context, by kd-tree descent (sca_clearance_enable) -------------------------
    def clearance_enable(self, on=True):
        """From now on every step runs k_clearance: every agent keeps how close it came to another agent and to an obstacle, with whom
        and at which env update since this call (include/sca_hip.h has the rule and what is refused while it is on).  Every row starts
        empty; on=False frees the records.  A context with scenes has scene_clearance_enable instead."""
        self._chk(self.L.sca_clearance_enable(self.ctx, 1 if on else 0), 'sca_clearance_enable')

    def clearance(self, begin=0, count=None):
        """The records of agents begin .. begin + count - 1 (all from `begin` on by default), a structured array (_lib.CLEARANCE_DTYPE:
        agent_clear, obs_clear f64, agent_partner, agent_step, obs_partner, obs_step i32; an empty half is +inf, -1, 0).  One copy, one
        synchronisation."""
        begin = int(begin)
        count = max(0, int(self.n) - begin) if count is None else int(count)
        out = np.zeros(max(count, 1), _lib.CLEARANCE_DTYPE)               # (a range the library will refuse still gets a buffer)
        self._chk(self.L.sca_get_clearance(self.ctx, begin, count, out.ctypes.data_as(C.POINTER(_lib.SceneClearance)), _lib.CLEARANCE_DTYPE.itemsize),
                  'sca_get_clearance')
        return out[:max(count, 0)]

    # ---- respawning agents in place (sca_respawn_agents / sca_get_finished) ----------------------------------------------------
    def respawn(self, ids, pos, vel, heading, radius, pref_speed, goal, max_run_dist, zaxis=None, goal_heading=None, paths=None, margin=None,
                policy=None, attrs=None):
        """New missions for the rows `ids` (any order, no repeats) while every other row keeps every word it had (sca_respawn_agents).
        margin (None: no gate, returns None): only the rows whose start is free are respawned (sca_respawn_agents_gated; the admission rule
        is include/sca_hip.h's) and the call returns (verdict, probe): an int32 word per named row -- SPAWN_ADMITTED 0, SPAWN_BLOCKED_AGENT 1,
        SPAWN_BLOCKED_OBSTACLE 2, SPAWN_BLOCKED_ENTRY 3 -- and the world test's records (_lib.CLEARANCE_DTYPE); a refused row keeps every
        word it had.
        The arrays hold len(ids) rows in the order of `ids`.  Afterwards a named row is what set_agents + set_state (+
        device_tracker_enable) leave for an agent with these values; it keeps its policy and its per-agent attributes.  zaxis None: the
        rows keep theirs.  goal_heading: needed when a named row is tracked by the device tracker.  paths (the lists in slot form,
        set_path_slots): one list of [x, y, z] waypoints per named row; None: the named rows' lists become empty.  Only between two
        steps; one launch and one synchronisation however many rows are named.
        policy (one byte per named row) / attrs (a dict of set_agent_params' names, one value per named row or a scalar): the arriving
        agents' own policy and solver attributes (sca_respawn_agents_attrs / _gated_attrs).  None: the rows keep theirs; with a dict, a name
        that is missing or None stands for the CONTEXT's value for every named row, not for what the row had.  The planner's names
        (turning_radius, pitch_lo, pitch_hi) need the device tracker; they are read for the rows whose new policy is tracked."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        T = len(ids)

        def arr(a, dt, ct, cols):
            if a is None:
                return None, None
            b = np.asarray(a, dt)
            b = np.ascontiguousarray(np.broadcast_to(b, (T, cols) if cols else (T,)) if b.ndim == 0 else b)
            if b.size != T * (cols or 1):
                raise ValueError(f'respawn: an array of {b.size} values where {T} rows x {cols or 1} are named')
            return b, _lib.ptr(b, ct)
        keep = [arr(pos, np.float64, C.c_double, 3), arr(vel, np.float32, C.c_float, 3), arr(heading, np.float64, C.c_double, 3),
                arr(radius, np.float64, C.c_double, 0), arr(pref_speed, np.float64, C.c_double, 0), arr(goal, np.float64, C.c_double, 3),
                arr(zaxis, np.uint8, C.c_uint8, 0), arr(max_run_dist, np.float64, C.c_double, 0), arr(goal_heading, np.float64, C.c_double, 3)]
        poff = ppts = None
        if paths is not None:
            if len(paths) != T:
                raise ValueError(f'respawn: {len(paths)} waypoint lists where {T} rows are named')
            poff, ppts = paths_csr(paths)
        brings = []
        if policy is not None or attrs is not None:
            desc = None
            if attrs is not None:
                unknown = sorted(set(attrs) - set(_ATTR_NAMES))
                if unknown:
                    raise ValueError(f'respawn: attrs names {unknown}, sca_restart_attrs has {list(_ATTR_NAMES)}')
                desc = _lib.RestartAttrs(struct_bytes=C.sizeof(_lib.RestartAttrs), reserved=0)
                for name, v in attrs.items():
                    if v is None:
                        continue
                    i32 = name == 'max_neighbors'
                    held = arr(v, np.int32 if i32 else np.float64, C.c_int32 if i32 else C.c_double, 0)
                    keep.append(held)                                  # (alive until the call returns)
                    setattr(desc, name, held[1])
            pol = arr(policy, np.uint8, C.c_uint8, 0)
            keep.append(pol)
            brings = [pol[1], None if desc is None else C.byref(desc)]
        rows = keep[:9]
        args = [self.ctx, T, _lib.ptr(ids, C.c_int32)] + brings + [p for _, p in rows] + \
            [None if poff is None else _lib.ptr(poff, C.c_int32), None if ppts is None else _lib.ptr(ppts, C.c_double)]
        plain, gated = ('sca_respawn_agents_attrs', 'sca_respawn_agents_gated_attrs') if brings else ('sca_respawn_agents', 'sca_respawn_agents_gated')
        if margin is None:
            self._chk(getattr(self.L, plain)(*args), plain)
            return None
        verdict, probe = np.zeros(max(T, 1), np.int32), np.zeros(max(T, 1), _lib.CLEARANCE_DTYPE)
        self._chk(getattr(self.L, gated)(*args, float(margin), _lib.ptr(verdict, C.c_int32), probe.ctypes.data_as(C.POINTER(_lib.SceneClearance)), None), gated)
        return verdict[:T], probe[:T]

    def probe_clearance(self, pos, radius, ignore=None):
        """How free is each point now: spheres of `radius` (a scalar or one per point) at `pos` (Q, 3) against every agent row's current
        record but ignore[q] (None or -1: nobody is excluded) and against every obstacle (sca_probe_clearance).  A structured array of
        _lib.CLEARANCE_DTYPE: agent_clear / obs_clear the smallest l3norm - (radius sum), agent_partner / obs_partner the lowest id with it,
        both step fields 0, an empty half +inf, -1, 0.  Only between two steps; changes nothing; one synchronisation."""
        pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
        Q = len(pos)
        radius = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float64), (Q,)))
        if ignore is not None:
            ignore = np.ascontiguousarray(np.broadcast_to(np.asarray(ignore, np.int32), (Q,)))
        out = np.zeros(max(Q, 1), _lib.CLEARANCE_DTYPE)                   # (a count the library will refuse still gets a buffer)
        self._chk(self.L.sca_probe_clearance(self.ctx, Q, _lib.ptr(pos, C.c_double), _lib.ptr(radius, C.c_double),
                                             None if ignore is None else _lib.ptr(ignore, C.c_int32), out.ctypes.data_as(C.POINTER(_lib.SceneClearance)),
                                             _lib.CLEARANCE_DTYPE.itemsize), 'sca_probe_clearance')
        return out[:Q]

    def finished(self, capacity=None):
        """The rows that carry any of at-goal / collision / timeout, ascending ids: a structured array (_lib.FINISHED_DTYPE: id i32, flags
        u32, step_num i32, reserved, total_dist f64, pos 3 x f64), compacted on the device -- one synchronisation, and only the finished
        rows cross the link (sca_get_finished).  capacity: at most that many rows are fetched (None: all); `finished_count` holds their
        number in either case."""
        cap = int(self.n) if capacity is None else int(capacity)
        out = np.zeros(max(cap, 1), _lib.FINISHED_DTYPE)
        cnt = C.c_int(0)
        self._chk(self.L.sca_get_finished(self.ctx, out.ctypes.data_as(C.POINTER(_lib.FinishedRow)), cap, C.byref(cnt), _lib.FINISHED_DTYPE.itemsize),
                  'sca_get_finished')
        self.finished_count = int(cnt.value)
        return out[:max(0, min(cap, self.finished_count))]

    # ---- vacant rows: drones leave the airspace and re-enter (sca_retire_agents / sca_get_vacant / sca_get_population) ---------
    def retire(self, ids):
        """Takes the occupied rows `ids` (any order, no repeats; live or finished) out of the world (sca_retire_agents): each becomes a
        vacant row -- flags 11 (at-goal | collision | FLAG_VACANT), zero velocity, heading, travelled distance and step count, position and
        constants kept -- that stands in no tree and is nobody's neighbour, collision, clearance or probe partner; every other row keeps
        every word it had.  The kd permutation keeps the occupied ids in carried order in front and the vacant ids ascending behind them.
        `respawn` with a vacant id admits the row again.  Only between two steps; one synchronisation however many rows are named."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        self._chk(self.L.sca_retire_agents(self.ctx, len(ids), _lib.ptr(ids, C.c_int32)), 'sca_retire_agents')

    def vacant(self, capacity=None):
        """The vacant rows' ids, ascending (sca_get_vacant: compacted on the device, one synchronisation; nothing is enqueued while no row
        is vacant).  capacity: at most that many ids are fetched (None: all); `vacant_count` holds their number in either case."""
        cap = int(self.n) if capacity is None else int(capacity)
        out = np.zeros(max(cap, 1), np.int32)
        cnt = C.c_int(0)
        self._chk(self.L.sca_get_vacant(self.ctx, _lib.ptr(out, C.c_int32), cap, C.byref(cnt)), 'sca_get_vacant')
        self.vacant_count = int(cnt.value)
        return out[:max(0, min(cap, self.vacant_count))]

    def population(self):
        """The occupied rows, m <= n (sca_get_population)."""
        m = C.c_int(0)
        self._chk(self.L.sca_get_population(self.ctx, C.byref(m)), 'sca_get_population')
        return int(m.value)

    # ---- mission tables: finished rows take their next mission inside the step (sca_set_missions) ------------------------------
    def set_missions(self, M, R, entries, first_ok, first_fail, paths=None):
        """Every row gets room for M mission entries and a ring of R result records (sca_set_missions; include/sca_hip.h has the rule and
        what is refused).  entries: a structured array of _lib.MISSION_DTYPE, (n, M) or flat in slot form entries[M a + j]; first_ok /
        first_fail: per row the successors of the flight in the air (-1 / -1: the row has no table).  M = 0 with entries None drops the
        tables.
        paths (sca_set_missions_paths; the lists in slot form, set_path_slots first): every entry brings its own waypoint list, which a
        row that takes the entry gets as under respawn(paths=...).  One list of [x, y, z] waypoints per FLAT entry M a + j (list order:
        the reference pops from the end), or a dict {(row, j): [...]} whose missing entries bring the empty list."""
        if entries is None and int(M) == 0:
            self._chk(self.L.sca_set_missions(self.ctx, 0, 0, 0, None, None, None), 'sca_set_missions')
            self._missions = None
            return
        entries = np.ascontiguousarray(entries, _lib.MISSION_DTYPE).reshape(-1)
        first_ok = np.ascontiguousarray(first_ok, np.int32).reshape(-1)
        first_fail = np.ascontiguousarray(first_fail, np.int32).reshape(-1)
        if len(entries) != int(M) * len(first_ok) or len(first_fail) != len(first_ok):
            raise ValueError(f'set_missions: {len(entries)} entries, {len(first_ok)} / {len(first_fail)} first successors where M = {M}')
        if paths is None:
            self._chk(self.L.sca_set_missions(self.ctx, int(M), int(R), len(first_ok), entries.ctypes.data_as(C.POINTER(_lib.Mission)),
                                              _lib.ptr(first_ok, C.c_int32), _lib.ptr(first_fail, C.c_int32)), 'sca_set_missions')
        else:
            if isinstance(paths, dict):
                flat = [[] for _ in range(len(entries))]
                for (a, j), lst in paths.items():
                    if not (0 <= int(a) < len(first_ok) and 0 <= int(j) < int(M)):
                        raise ValueError(f'set_missions: paths names entry ({a}, {j}) where there are {len(first_ok)} rows of M = {M} entries')
                    flat[int(M) * int(a) + int(j)] = lst
                paths = flat
            if len(paths) != len(entries):
                raise ValueError(f'set_missions: {len(paths)} waypoint lists where there are {len(entries)} entries')
            off, pts = paths_csr(paths)
            self._chk(self.L.sca_set_missions_paths(self.ctx, int(M), int(R), len(first_ok), entries.ctypes.data_as(C.POINTER(_lib.Mission)),
                                                    _lib.ptr(first_ok, C.c_int32), _lib.ptr(first_fail, C.c_int32), _lib.ptr(off, C.c_int32),
                                                    _lib.ptr(pts, C.c_double)), 'sca_set_missions_paths')
        self._missions = (int(M), int(R))

    def mission_paths(self):
        """(W, total): the room per row and the points the tables' lists hold (sca_get_mission_paths); (0, 0) for tables without lists"""
        w, total = C.c_int(0), C.c_int64(0)
        self._chk(self.L.sca_get_mission_paths(self.ctx, C.byref(w), C.byref(total)), 'sca_get_mission_paths')
        return int(w.value), int(total.value)

    def mission_results(self, capacity=None):
        """The results not yet collected, ascending id and within a row oldest first: a structured array of _lib.MISSION_RESULT_DTYPE
        (id, entry, flags, step_num, total_dist, pos, update, next, clear); they are marked collected.  capacity None: room for every
        ring.  `mission_result_count` holds their number; where it exceeds `capacity` nothing is handed out or marked."""
        R = (getattr(self, '_missions', None) or (0, 1))[1]
        cap = int(self.n) * R if capacity is None else int(capacity)
        out = np.zeros(max(cap, 1), _lib.MISSION_RESULT_DTYPE)
        cnt = C.c_int(0)
        self._chk(self.L.sca_get_mission_results(self.ctx, out.ctypes.data_as(C.POINTER(_lib.MissionResult)), cap, C.byref(cnt),
                                                 _lib.MISSION_RESULT_DTYPE.itemsize), 'sca_get_mission_results')
        self.mission_result_count = int(cnt.value)
        return out[:self.mission_result_count if self.mission_result_count <= cap else 0]

    def mission_totals(self):
        """dict(updates, agent_steps, arrived, collided, timed_out, taken, stopped): 64-bit counters since set_missions, over all rows"""
        t = _lib.MissionTotals()
        self._chk(self.L.sca_get_mission_totals(self.ctx, C.byref(t), C.sizeof(t)), 'sca_get_mission_totals')
        return {k: int(getattr(t, k)) for k, _ in _lib.MissionTotals._fields_ if k != 'reserved'}

    def mission_state(self, begin=0, count=None):
        """(cursor, ended) of rows begin .. begin + count - 1: the entry whose successors the row's next ending follows (-1: first_ok /
        first_fail) and the number of its endings so far, int32 each"""
        begin = int(begin)
        count = max(0, int(self.n) - begin) if count is None else int(count)
        cursor, ended = np.zeros(max(count, 1), np.int32), np.zeros(max(count, 1), np.int32)
        self._chk(self.L.sca_get_mission_state(self.ctx, begin, count, _lib.ptr(cursor, C.c_int32), _lib.ptr(ended, C.c_int32)), 'sca_get_mission_state')
        return cursor[:max(count, 0)], ended[:max(count, 0)]

    # ---- the admission gate in front of the take (sca_set_mission_gate) --------------------------------------------------------
    def set_mission_gate(self, margin, max_per_step=0):
        """While tables stand a row takes its next mission only where its start is free by `margin` metres (sca_set_mission_gate; the
        rule is sca_respawn_agents_gated's, include/sca_hip.h); a refused row waits and is offered again behind every step.
        max_per_step: the candidates tested per step (0: min(n, 4096)).  margin None: the gate goes off, pending missions are dropped."""
        if margin is None:
            self._chk(self.L.sca_set_mission_gate(self.ctx, 0, 0.0, 0), 'sca_set_mission_gate')
        else:
            self._chk(self.L.sca_set_mission_gate(self.ctx, 1, float(margin), int(max_per_step)), 'sca_set_mission_gate')

    def mission_gate_state(self, begin=0, count=None):
        """(waiting, verdict, refusals) of rows begin .. begin + count - 1, int32 each: the entry a row waits for (-1: none), the word of
        its last test (SPAWN_*) and how often it has been refused"""
        begin = int(begin)
        count = max(0, int(self.n) - begin) if count is None else int(count)
        out = [np.zeros(max(count, 1), np.int32) for _ in range(3)]
        self._chk(self.L.sca_get_mission_gate_state(self.ctx, begin, count, *[_lib.ptr(a, C.c_int32) for a in out]), 'sca_get_mission_gate_state')
        return tuple(a[:max(count, 0)] for a in out)

    def mission_gate_totals(self):
        """dict(offered, admitted, blocked_agent, blocked_obstacle, blocked_entry, over_cap, dropped): 64-bit counters since the first
        gate behind the tables; offered == admitted + blocked_* + over_cap"""
        t = _lib.MissionGateTotals()
        self._chk(self.L.sca_get_mission_gate_totals(self.ctx, C.byref(t), C.sizeof(t)), 'sca_get_mission_gate_totals')
        return {k: int(getattr(t, k)) for k, _ in _lib.MissionGateTotals._fields_ if k != 'reserved'}

    # ---- scene checkpoints (sca_save_scenes / sca_load_scenes) ---------------------------------------------------------------
    def scene_checkpoint_bytes(self, scene):
        """the size of the blob save_scenes writes for the scene as it stands now"""
        out = C.c_int64(0)
        self._chk(self.L.sca_scene_checkpoint_bytes(self.ctx, int(scene), C.byref(out)), 'sca_scene_checkpoint_bytes')
        return int(out.value)

    def save_scenes(self, ids):
        """The named scenes' mutable state, one uint8 array each (include/sca_hip.h: what a blob holds).  One launch, one synchronisation."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        inside = [s for s in ids if self.scene_offsets is not None and 0 <= s < self.nscenes]
        sizes = {int(s): self.scene_checkpoint_bytes(s) for s in set(inside)}        # (an id the library will refuse still gets a buffer)
        blobs = [np.zeros(sizes.get(int(s), 64), np.uint8) for s in ids]
        self._save_into(ids, blobs)
        return blobs

    def _save_into(self, ids, blobs):
        ptrs = (C.c_void_p * max(1, len(blobs)))(*[b.ctypes.data for b in blobs])
        nbytes = np.array([b.size for b in blobs] or [0], np.int64)
        self._chk(self.L.sca_save_scenes(self.ctx, len(ids), _lib.ptr(ids, C.c_int32), ptrs, _lib.ptr(nbytes, C.c_int64)), 'sca_save_scenes')

    def load_scenes(self, ids, blobs):
        """blobs[e] (bytes or a uint8 array, from save_scenes of any context) into scene ids[e], which a restart has given the blob's episode.
        Every blob is checked whole before the device sees it; ScaError (SCA_ERR_ARG) names what is wrong."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        blobs = [np.ascontiguousarray(np.frombuffer(b, np.uint8) if isinstance(b, (bytes, bytearray)) else b, np.uint8).reshape(-1) for b in blobs]
        if len(blobs) != len(ids):
            raise ValueError('load_scenes: %d ids and %d blobs' % (len(ids), len(blobs)))
        ptrs = (C.c_void_p * max(1, len(blobs)))(*[b.ctypes.data for b in blobs])
        nbytes = np.array([b.size for b in blobs] or [0], np.int64)
        self._chk(self.L.sca_load_scenes(self.ctx, len(ids), _lib.ptr(ids, C.c_int32), ptrs, _lib.ptr(nbytes, C.c_int64)), 'sca_load_scenes')

    def scene_checkpoint_info(self, blob):
        """The header of a blob as a dict, after the whole check a load makes without a scene; plus `offsets`, the byte offsets of its
        sections (sca_scene_checkpoint_layout), and `policy`, the rows' policy bytes."""
        return scene_checkpoint_info(blob)

    # ---- context checkpoints (sca_save_context / sca_load_context) -------------------------------------------------------------
    # vacancy=True: the _opt entry points with SCA_CHECKPOINT_VACANCY -- the checkpoint carries vacant rows (retire_agents); without it each
    # call is the entry point it always was, refused while a row is vacant
    def context_checkpoint_bytes(self, vacancy=False):
        """the size of the blob save_context writes for the context as it stands now"""
        out = C.c_int64(0)
        if vacancy:
            self._chk(self.L.sca_context_checkpoint_bytes_opt(self.ctx, CHECKPOINT_VACANCY, C.byref(out)), 'sca_context_checkpoint_bytes_opt')
        else:
            self._chk(self.L.sca_context_checkpoint_bytes(self.ctx, C.byref(out)), 'sca_context_checkpoint_bytes')
        return int(out.value)

    def save_context(self, vacancy=False):
        """The whole context's mutable state as one uint8 array (include/sca_hip.h: what a blob holds).  One launch, one synchronisation."""
        blob = np.zeros(self.context_checkpoint_bytes(vacancy), np.uint8)
        if vacancy:
            self._chk(self.L.sca_save_context_opt(self.ctx, CHECKPOINT_VACANCY, C.c_void_p(blob.ctypes.data), blob.size), 'sca_save_context_opt')
        else:
            self._chk(self.L.sca_save_context(self.ctx, C.c_void_p(blob.ctypes.data), blob.size), 'sca_save_context')
        return blob

    def load_context(self, blob, vacancy=False):
        """blob (bytes or a uint8 array, from save_context of any context) into this context, which has been given the run's definition.
        The blob is checked whole before the device sees it; ScaError (SCA_ERR_ARG) names what is wrong."""
        b = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray)) else blob, np.uint8).reshape(-1)
        if vacancy:
            self._chk(self.L.sca_load_context_opt(self.ctx, CHECKPOINT_VACANCY, C.c_void_p(b.ctypes.data), b.size), 'sca_load_context_opt')
        else:
            self._chk(self.L.sca_load_context(self.ctx, C.c_void_p(b.ctypes.data), b.size), 'sca_load_context')

    def context_checkpoint_info(self, blob):
        """The header of a blob as a dict, after the whole check a load makes without a context; plus `offsets`, the byte offsets of its
        sections (sca_context_checkpoint_layout), and `policy`, the rows' policy bytes."""
        return context_checkpoint_info(blob)

    # ---- SCA's v_pref tracker on the device (scaPolicy.py:264-338) ---------------------------------------
    def device_tracker_enable(self, goal_heading, turning_radius=1.5, pitchlims=(-math.pi / 4, math.pi / 4), in_pass=True):
        """From now on the SCA / RVO3D+Dubins agents take v_pref from the device tracker: inside every policy pass
        (in_pass=True) or only when device_tracker_vpref() is called."""
        gh = _lib.as_d(goal_heading).reshape(self.n, 3)
        self._chk(self.L.sca_device_tracker_enable(self.ctx, _lib.ptr(gh, C.c_double), float(turning_radius), float(pitchlims[0]),
                                                   float(pitchlims[1]), int(bool(in_pass))), 'sca_device_tracker_enable')

    def device_tracker_set_agent_params(self, turning_radius=None, pitch_lo=None, pitch_hi=None):
        """agent.turning_radius / agent.pitchlims per agent (arrays of n; None = device_tracker_enable's value); after device_tracker_enable"""
        keep = []

        def arr(a):
            if a is None:
                return None
            b = _lib.as_d(np.broadcast_to(a, (self.n,)))
            keep.append(b)
            return _lib.ptr(b, C.c_double)
        self._chk(self.L.sca_device_tracker_set_agent_params(self.ctx, self.n, arr(turning_radius), arr(pitch_lo), arr(pitch_hi)),
                  'sca_device_tracker_set_agent_params')

    def device_tracker_disable(self):
        self._chk(self.L.sca_device_tracker_disable(self.ctx), 'sca_device_tracker_disable')

    def device_tracker_vpref(self, nbr0_dsq=None):
        """One compute_v_pref for every active tracked agent on the current state; nbr0_dsq[i] = distSq of agent.neighbors[0]
        of the previous pass (negative: empty), None = taken from the neighbour lists on the device."""
        out = np.zeros((self.n, 3))
        nb = None if nbr0_dsq is None else _lib.as_d(nbr0_dsq).reshape(self.n)
        self._chk(self.L.sca_device_tracker_vpref(self.ctx, None if nb is None else _lib.ptr(nb, C.c_double),
                                                  _lib.ptr(out, C.c_double)), 'sca_device_tracker_vpref')
        return out

    def device_tracker_replans(self):
        r = np.zeros(self.n, np.int32)
        self._chk(self.L.sca_device_tracker_replans(self.ctx, _lib.ptr(r, C.c_int32)), 'sca_device_tracker_replans')
        return r

    def device_tracker_debug(self, agent):
        """The device tracker's record of one agent as 24 doubles (sca_device_tracker_debug: the plan, its cursor, now_goal, v_pref, re-plans)"""
        out = np.zeros(24)
        self._chk(self.L.sca_device_tracker_debug(self.ctx, int(agent), _lib.ptr(out, C.c_double)), 'sca_device_tracker_debug')
        return out

    # ---- hot path --------------------------------------------------------------------------------------
    def policy_pass(self, mode=NBR_KDTREE):
        self._chk(self.L.sca_policy_pass(self.ctx, int(mode)), 'sca_policy_pass')

    def env_update(self, want_done=True):
        done = C.c_int(0)
        self._chk(self.L.sca_env_update(self.ctx, C.byref(done) if want_done else None), 'sca_env_update')
        return bool(done.value)

    def run_steps(self, steps, mode=NBR_KDTREE):
        self._chk(self.L.sca_run_steps(self.ctx, int(steps), int(mode)), 'sca_run_steps')

    def env_step(self, mode=NBR_KDTREE):
        """One resident step + the agents still running after it (MACAEnv.step in one library call; synchronises)."""
        v = C.c_int(0)
        self._chk(self.L.sca_env_step(self.ctx, int(mode), C.byref(v)), 'sca_env_step')
        return int(v.value)

    # ---- the env loop with the HOST as the owner of the state (mampenv.py:27-59): pinned state block + one call per step ------------
    def host_state(self):
        """The library's page-locked state block as a dict of numpy VIEWS (no copies): pos (n, 3) f64, vel (n, 3) f32, heading (n, 3) f64,
        flags (n,) u8, total_dist (n,) f64, step_num (n,) i32 -- read and written in place --, vpref (n, 3) f64, vpref_mode (n,) u8 -- written --,
        action (n, 7) f32 -- read.  Made once per set_agents and cached; the views keep the solver (and with it the block) alive."""
        if self._host_state is None:
            h = _lib.HostState()
            self._chk(self.L.sca_host_state_get(self.ctx, C.byref(h), C.sizeof(h)), 'sca_host_state_get')
            n = h.n
            owner = _BlockOwner(self)

            def view(p, ct, dt, shape):
                count = int(np.prod(shape))
                buf = (ct * count).from_address(C.addressof(p.contents))
                buf._sca_owner = owner                            # (numpy keeps `buf` as the array's base: the solver outlives the view)
                return np.frombuffer(buf, dtype=dt, count=count).reshape(shape)
            self._host_state = dict(
                pos=view(h.pos, C.c_double, np.float64, (n, 3)), vel=view(h.vel, C.c_float, np.float32, (n, 3)),
                heading=view(h.heading, C.c_double, np.float64, (n, 3)), flags=view(h.flags, C.c_uint8, np.uint8, (n,)),
                total_dist=view(h.total_dist, C.c_double, np.float64, (n,)), step_num=view(h.step_num, C.c_int32, np.int32, (n,)),
                vpref=view(h.vpref, C.c_double, np.float64, (n, 3)), vpref_mode=view(h.vpref_mode, C.c_uint8, np.uint8, (n,)),
                action=view(h.action, C.c_float, np.float32, (n, 7)))
        return self._host_state

    def step_host(self, mode=NBR_KDTREE, state=True, vpref=False):
        """One env step from the block and into it (sca_step_host): state=True takes the six in/out arrays of host_state() as written,
        vpref=True takes vpref / vpref_mode; afterwards the block holds the state after the step and the action rows.  Returns the number
        of agents still running (0 == MACAEnv.is_done)."""
        v = C.c_int(0)
        mask = (_lib.HOST_IN_STATE if state else 0) | (_lib.HOST_IN_VPREF if vpref else 0)
        self._chk(self.L.sca_step_host(self.ctx, int(mode), mask, C.byref(v)), 'sca_step_host')
        return int(v.value)

    def synchronize(self):
        self._chk(self.L.sca_synchronize(self.ctx), 'sca_synchronize')

    def active_count(self):
        """Agents of this rank not yet done after the last env update (0 == MACAEnv.is_done); synchronises."""
        v = C.c_int(0)
        self._chk(self.L.sca_active_count(self.ctx, C.byref(v)), 'sca_active_count')
        return int(v.value)

    def actions(self):
        a = np.zeros((self.n, 7), np.float32)
        self._chk(self.L.sca_get_actions(self.ctx, _lib.ptr(a, C.c_float)), 'sca_get_actions')
        return a

    def neighbors(self):
        n = self.n
        out = dict(nbr_n=np.zeros(n, np.int32), nbr_id=np.zeros((n, K), np.int32), nbr_kind=np.zeros((n, K), np.uint8),
                   nbr_dsq=np.zeros((n, K)), nbr_valid=np.zeros(n, np.uint8))
        self._chk(self.L.sca_get_neighbors(self.ctx, _lib.ptr(out['nbr_n'], C.c_int32), _lib.ptr(out['nbr_id'], C.c_int32),
                                           _lib.ptr(out['nbr_kind'], C.c_uint8), _lib.ptr(out['nbr_dsq'], C.c_double),
                                           _lib.ptr(out['nbr_valid'], C.c_uint8)), 'sca_get_neighbors')
        return out

    def nbr0(self):
        a = np.zeros(self.n)
        self._chk(self.L.sca_get_nbr0(self.ctx, _lib.ptr(a, C.c_double)), 'sca_get_nbr0')
        return a

    def diag(self):
        n = self.n
        out = dict(diag=np.zeros((n, 5), np.int32), status=np.zeros(n, np.int32), vpref=np.zeros((n, 3)))
        self._chk(self.L.sca_get_diag(self.ctx, _lib.ptr(out['diag'], C.c_int32), _lib.ptr(out['status'], C.c_int32),
                                      _lib.ptr(out['vpref'], C.c_double)), 'sca_get_diag')
        return out

    def kernel_ms(self):
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        self._chk(self.L.sca_last_kernel_ms(self.ctx, C.byref(a), C.byref(b), C.byref(c)), 'sca_last_kernel_ms')
        return dict(neighbors=a.value, solve=b.value, update=c.value)

    def replan_ms(self):
        a = C.c_float(0)
        self._chk(self.L.sca_last_replan_ms(self.ctx, C.byref(a)), 'sca_last_replan_ms')
        return a.value

    def auto_stats(self, reset=False):
        """SCA_NBR_AUTO since the last reset: passes, agents listed for the kd query per pass (mean, max), share of passes with a list"""
        a = (C.c_int64 * 4)()
        self._chk(self.L.sca_auto_stats(self.ctx, a, 1 if reset else 0), 'sca_auto_stats')
        p = max(int(a[0]), 1)
        return {'auto_passes': int(a[0]), 'listed_per_pass_mean': a[1] / p, 'listed_per_pass_max': int(a[2]), 'passes_with_a_list_frac': a[3] / p}

    def kd_build_ms(self):
        a = C.c_float(0)
        self._chk(self.L.sca_last_kd_build_ms(self.ctx, C.byref(a)), 'sca_last_kd_build_ms')
        return a.value

    def exchange_ms(self):
        """mean device time of the in-library all-gather over the profiled steps (0.0 without a communicator)"""
        a = C.c_float(0)
        self._chk(self.L.sca_last_exchange_ms(self.ctx, C.byref(a)), 'sca_last_exchange_ms')
        return a.value

    def pass_forms(self):
        """SCA_FORM_* bits of the last policy pass (which kernel forms the library picked)"""
        a = C.c_int(0)
        self._chk(self.L.sca_last_pass_forms(self.ctx, C.byref(a)), 'sca_last_pass_forms')
        return a.value

    def set_shard_emulation(self, on=True):
        self._chk(self.L.sca_set_shard_emulation(self.ctx, 1 if on else 0), 'sca_set_shard_emulation')

    def set_profiling(self, on=True):
        self._chk(self.L.sca_set_profiling(self.ctx, 1 if on else 0), 'sca_set_profiling')

    def agent_steps(self, reset=False):
        v = C.c_int64(0)
        self._chk(self.L.sca_agent_steps(self.ctx, C.byref(v), 1 if reset else 0), 'sca_agent_steps')
        return int(v.value)

    # ---- trajectory log (Agent.history_info) kept on the device -----------------------------------------
    def history_enable(self, capacity_rows):
        self._chk(self.L.sca_history_enable(self.ctx, int(capacity_rows)), 'sca_history_enable')

    def history_rows(self):
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self.L.sca_history_rows(self.ctx, C.byref(a), C.byref(b)), 'sca_history_rows')
        return a.value, b.value

    def history(self, first_row=0, nrows=None, agent_begin=0, agent_count=None):
        """Rows [first_row, first_row+nrows) of agents [agent_begin, +agent_count): dict of [nrows, agents, 3] arrays."""
        if nrows is None:
            nrows = self.history_rows()[0] - first_row
        if agent_count is None:
            agent_count = self.n - agent_begin
        out = dict(pos=np.zeros((nrows, agent_count, 3)), heading=np.zeros((nrows, agent_count, 3)),
                   vel=np.zeros((nrows, agent_count, 3), np.float32))
        self._chk(self.L.sca_get_history(self.ctx, int(first_row), int(nrows), int(agent_begin), int(agent_count),
                                         _lib.ptr(out['pos'], C.c_double), _lib.ptr(out['heading'], C.c_double),
                                         _lib.ptr(out['vel'], C.c_float)), 'sca_get_history')
        return out

    # ---- multi-GPU --------------------------------------------------------------------------------------
    def set_shard(self, begin, count):
        self._chk(self.L.sca_set_shard(self.ctx, int(begin), int(count)), 'sca_set_shard')

    def public_records(self, which=0):
        p = C.c_void_p()
        b = C.c_int64()
        self._chk(self.L.sca_public_records(self.ctx, int(which), C.byref(p), C.byref(b)), 'sca_public_records')
        return p.value, b.value

    def bind_public_records(self, current_ptr, moved_ptr, bytes_each=0):
        self._chk(self.L.sca_bind_public_records(self.ctx, C.c_void_p(current_ptr), C.c_void_p(moved_ptr), int(bytes_each)),
                  'sca_bind_public_records')

    def step_begin(self, mode=NBR_KDTREE):
        self._chk(self.L.sca_step_begin(self.ctx, int(mode)), 'sca_step_begin')

    def step_end(self):
        self._chk(self.L.sca_step_end(self.ctx), 'sca_step_end')

    def set_stream(self, stream_ptr):
        """Run on this hipStream_t; 0 / None is HIP's null stream (torch's default stream), taken literally."""
        self._chk(self.L.sca_set_stream(self.ctx, C.c_void_p(stream_ptr)), 'sca_set_stream')

    def use_own_stream(self):
        self._chk(self.L.sca_use_own_stream(self.ctx), 'sca_use_own_stream')

    # ---- cell-owner partition of SCA_NBR_GRID with halo exchange (sca_partition_*) ---------------------------
    def partition_init(self, rank, nranks, axis=0, cuts=None, cap_halo=0, cap_mig=0):
        c = None if cuts is None else _lib.ptr(_lib.as_d(cuts), C.c_double)
        self._chk(self.L.sca_partition_init(self.ctx, int(rank), int(nranks), int(axis), c, int(cap_halo), int(cap_mig)), 'sca_partition_init')

    def partition_disable(self):
        self._chk(self.L.sca_partition_disable(self.ctx), 'sca_partition_disable')

    def partition_message_bytes(self):
        return int(self.L.sca_partition_message_bytes(self.ctx))

    def partition_pack(self, lower_ptr, upper_ptr):
        self._chk(self.L.sca_partition_pack(self.ctx, C.c_void_p(lower_ptr), C.c_void_p(upper_ptr)), 'sca_partition_pack')

    def partition_unpack(self, lower_ptr, upper_ptr):
        self._chk(self.L.sca_partition_unpack(self.ctx, C.c_void_p(lower_ptr), C.c_void_p(upper_ptr)), 'sca_partition_unpack')

    def partition_commit(self):
        self._chk(self.L.sca_partition_commit(self.ctx), 'sca_partition_commit')

    def partition_counts(self):
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self.L.sca_partition_counts(self.ctx, C.byref(a), C.byref(b)), 'sca_partition_counts')
        return a.value, b.value

    def partition_owned(self):
        ids = np.zeros(self.n, np.int32)
        k = C.c_int(0)
        self._chk(self.L.sca_partition_owned(self.ctx, _lib.ptr(ids, C.c_int32), C.byref(k)), 'sca_partition_owned')
        return ids[:k.value].copy()

    # RCCL inside the library: run_steps then exchanges the shard's moved records itself, one host call per k steps
    def comm_probe(self):
        """True when the library can load RCCL (no collective: safe to call before the ranks agree on using it)."""
        return self.L.sca_comm_probe() == 0

    def comm_unique_id(self):
        buf = C.create_string_buffer(128)
        rc = self.L.sca_comm_unique_id(buf)
        if rc != 0:
            raise ScaError(f'sca_comm_unique_id: rc={rc} (librccl.so missing?)')
        return buf.raw

    def comm_init(self, rank, nranks, unique_id):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._chk(self.L.sca_comm_init(self.ctx, int(rank), int(nranks), buf), 'sca_comm_init')

    def comm_destroy(self):
        self._chk(self.L.sca_comm_destroy(self.ctx), 'sca_comm_destroy')


def scene_checkpoint_layout(size, trk_words, has_paths):
    """(offsets [14] int64, total bytes) of a scene checkpoint (sca_scene_checkpoint_layout); pure, no device"""
    off = np.zeros(_lib.CHECKPOINT_SECTIONS, np.int64)
    total = C.c_int64(0)
    rc = _lib.lib().sca_scene_checkpoint_layout(int(size), int(trk_words), int(has_paths), _lib.ptr(off, C.c_int64), C.byref(total))
    if rc != 0:
        raise ScaError('sca_scene_checkpoint_layout: bad argument (rc=%d)' % rc)
    return off, int(total.value)


def scene_checkpoint_info(blob):
    """see BatchedSolver.scene_checkpoint_info; pure, no device"""
    b = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray)) else blob, np.uint8).reshape(-1)
    info = _lib.SceneCheckpointInfo()
    rc = _lib.lib().sca_scene_checkpoint_info(C.c_void_p(b.ctypes.data), b.size, C.byref(info), C.sizeof(info))
    if rc != 0:
        raise ScaError('sca_scene_checkpoint_info: not a valid scene checkpoint (rc=%d)' % rc)
    out = {k: int(getattr(info, k)) for k, _ in info._fields_ if k not in ('struct_bytes', 'reserved')}
    out['offsets'], _ = scene_checkpoint_layout(out['size'], out['trk_words'], out['has_paths'])
    out['policy'] = b[out['offsets'][0]:out['offsets'][0] + out['size']].copy()
    return out


def context_checkpoint_layout(n, trk_words=0, list_form=0, W=0, M=0, R=0, has_gate=0, has_clearance=0):
    """(offsets [26] int64, total bytes) of a context checkpoint (sca_context_checkpoint_layout); pure, no device"""
    shape = _lib.ContextCheckpointShape(C.sizeof(_lib.ContextCheckpointShape), int(n), int(trk_words), int(list_form), int(W), int(M), int(R),
                                        int(has_gate), int(has_clearance))
    off = np.zeros(_lib.CONTEXT_CHECKPOINT_SECTIONS, np.int64)
    total = C.c_int64(0)
    rc = _lib.lib().sca_context_checkpoint_layout(C.byref(shape), _lib.ptr(off, C.c_int64), C.byref(total))
    if rc != 0:
        raise ScaError('sca_context_checkpoint_layout: bad argument (rc=%d)' % rc)
    return off, int(total.value)


def context_checkpoint_info(blob):
    """see BatchedSolver.context_checkpoint_info; pure, no device"""
    b = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray)) else blob, np.uint8).reshape(-1)
    info = _lib.ContextCheckpointInfo()
    rc = _lib.lib().sca_context_checkpoint_info(C.c_void_p(b.ctypes.data), b.size, C.byref(info), C.sizeof(info))
    if rc != 0:
        raise ScaError('sca_context_checkpoint_info: not a valid context checkpoint (rc=%d)' % rc)
    out = {k: int(getattr(info, k)) for k, _ in info._fields_ if k not in ('struct_bytes', 'reserved', 'reserved1')}
    out['offsets'], _ = context_checkpoint_layout(out['n'], out['trk_words'], out['list_form'], out['W'], out['M'], out['R'], out['has_gate'], out['has_clearance'])
    out['policy'] = b[out['offsets'][0]:out['offsets'][0] + out['n']].copy()
    return out


def paths_csr(paths):
    """Per-agent waypoint lists -> (offsets [n + 1] int32, points [total, 3] float64), the form sca_set_paths takes."""
    lens = [len(p) for p in paths]
    off = np.zeros(len(paths) + 1, np.int32)
    off[1:] = np.cumsum(lens)
    flat = [w for p in paths for w in p]                           # (one conversion for all lists: a restart brings a list per row)
    pts = np.asarray(flat, dtype=np.float64).reshape(len(flat), 3) if flat else np.zeros((0, 3))
    return off, pts


def zaxis_flags(start, goal):
    """is_zAxis of scaPolicy.py:188-189: start and goal share x and y."""
    d = np.asarray(goal, float)[:, :3] - np.asarray(start, float)[:, :3]
    return ((np.abs(d[:, 0]) <= 1e-5) & (np.abs(d[:, 1]) <= 1e-5)).astype(np.uint8)
