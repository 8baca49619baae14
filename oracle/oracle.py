"""ctypes binding of oracle/liboracle.so -- TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
The product path (sca_amd) never does.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
K = 16

POL_SCA, POL_RVO, POL_SRVO, POL_ORCA, POL_ORCA_LP, POL_RVO_DUBINS = 0, 1, 2, 3, 4, 5
FLAG_AT_GOAL, FLAG_COLLISION, FLAG_TIMEOUT = 1, 2, 4


def build(force=False):
    so = os.path.join(_HERE, 'liboracle.so')
    srcs = [os.path.join(_HERE, f) for f in ('sca_oracle.c', 'sca_dubins_oracle.c', 'Makefile')]
    if force or not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(['make', '-C', _HERE, '-s'])
    return so


def lib():
    global _LIB
    if _LIB is None:
        so = os.environ.get('SCA_ORACLE_SO') or os.path.join(_HERE, 'liboracle.so')    # SCA_ORACLE_SO: the sanitizer build
        if not os.path.exists(so):
            build()
        L = C.CDLL(so)
        dp, fp, ip, bp = (C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8))
        L.orc_round5_py.restype = C.c_double
        L.orc_round5_py.argtypes = [C.c_double]
        L.orc_round5_np.restype = C.c_double
        L.orc_round5_np.argtypes = [C.c_double]
        L.orc_trunc5.restype = C.c_double
        L.orc_trunc5.argtypes = [C.c_double]
        for nm in ('orc_l3norm', 'orc_l3normsq', 'orc_distance'):
            getattr(L, nm).restype = C.c_double
            getattr(L, nm).argtypes = [dp, dp]
        L.orc_l3norm_mixed.restype = C.c_double
        L.orc_l3norm_mixed.argtypes = [dp, fp]
        L.orc_l3norm_f32zero.restype = C.c_double
        L.orc_l3norm_f32zero.argtypes = [fp]
        L.orc_get_phi.restype = C.c_double
        L.orc_get_phi.argtypes = [dp]
        L.orc_pi_2_pi.restype = C.c_double
        L.orc_pi_2_pi.argtypes = [C.c_double]
        L.orc_mod2pi.restype = C.c_double
        L.orc_mod2pi.argtypes = [C.c_double]
        L.orc_is_intersect.restype = C.c_int
        L.orc_is_intersect.argtypes = [dp, dp, C.c_double, dp]
        L.orc_satisfied_constraint.restype = C.c_int
        L.orc_satisfied_constraint.argtypes = [fp, C.c_double, dp]
        L.orc_cartesian2spherical.restype = None
        L.orc_cartesian2spherical.argtypes = [dp, dp, C.c_int, dp]
        L.orc_candidate_table.restype = C.c_int
        L.orc_candidate_table.argtypes = [C.c_double, C.c_int, dp, C.c_int]
        L.orc_kd_build.restype = None
        L.orc_kd_build.argtypes = [C.c_int, dp, ip, dp]
        L.orc_straight_v_pref.restype = None
        L.orc_straight_v_pref.argtypes = [dp, dp, C.c_double, C.c_int, dp]
        L.orc_set_params.restype = None
        L.orc_set_params.argtypes = [C.c_double, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]
        L.orc_set_dt_nominal.restype = None
        L.orc_set_dt_nominal.argtypes = [C.c_double]
        L.orc_set_agent_params.restype = None
        L.orc_set_agent_params.argtypes = [C.c_int, dp, ip, dp, dp, dp, dp, dp]
        L.orc_set_list_rule.restype = None
        L.orc_set_list_rule.argtypes = [C.c_int]
        L.orc_policy_step.restype = C.c_int
        L.orc_policy_step.argtypes = [C.c_int, C.c_int, dp, fp, dp, dp, dp, bp, dp, bp, bp, dp, bp, ip, dp, dp, dp, fp,
                                      ip, ip, bp, dp, bp, dp, ip, ip, C.c_int]
        L.orc_env_update.restype = C.c_int
        L.orc_env_update.argtypes = [C.c_int, C.c_int, dp, fp, dp, dp, bp, dp, fp, dp, dp, ip, dp, dp]
        L.orc_num_threads.restype = C.c_int
        i64p = C.POINTER(C.c_int64)
        L.orc_dubins_plan.restype = C.c_int
        L.orc_dubins_plan.argtypes = [dp, dp, C.c_double, C.c_double, C.c_double, dp, C.c_char_p, i64p, C.c_int, dp]
        L.orc_dubins_plan_batch.restype = C.c_int
        L.orc_dubins_plan_batch.argtypes = [C.c_int, dp, dp, dp, dp, dp, C.c_int]
        L.orc_tracker_create.restype = C.c_void_p
        L.orc_tracker_create.argtypes = [C.c_int, dp, dp, dp, bp, C.c_double, C.c_double, C.c_double, C.c_double]
        L.orc_tracker_destroy.restype = None
        L.orc_tracker_destroy.argtypes = [C.c_void_p]
        L.orc_tracker_set_params.restype = C.c_int
        L.orc_tracker_set_params.argtypes = [C.c_void_p, dp, dp, dp, dp]
        L.orc_tracker_vpref.restype = C.c_int
        L.orc_tracker_vpref.argtypes = [C.c_void_p, dp, fp, dp, bp, dp, dp, C.c_int]
        L.orc_tracker_replans.restype = C.c_int
        L.orc_tracker_replans.argtypes = [C.c_void_p, ip]
        L.orc_tracker_debug.restype = C.c_int
        L.orc_tracker_debug.argtypes = [C.c_void_p, C.c_int, dp]
        _LIB = L
    return _LIB


DEFAULT_PARAMS = dict(neighbor_dist=10.0, max_neighbors=16, time_step=0.1, time_horizon=10.0, max_speed=1.0,
                      max_heading_change=math.pi / 4, near_goal_threshold=0.5, dt_nominal=0.1)


def set_params(**kw):
    """The solver attributes of agent.py:27-41 / config.py:3 for every following call (process-wide); set_params() restores the
    reference's defaults."""
    p = dict(DEFAULT_PARAMS)
    unknown = set(kw) - set(p)
    if unknown:
        raise TypeError(f'unknown oracle parameter(s): {sorted(unknown)}')
    p.update(kw)
    L = lib()
    L.orc_set_params(p['neighbor_dist'], int(p['max_neighbors']), p['time_step'], p['time_horizon'], p['max_speed'],
                     p['max_heading_change'], p['near_goal_threshold'])
    L.orc_set_dt_nominal(p['dt_nominal'])


def set_agent_params(n=0, neighbor_dist=None, max_neighbors=None, time_step=None, time_horizon=None, max_speed=None, max_heading_change=None,
                     dt_nominal=None):
    """Per-agent solver attributes (the reference keeps them on every Agent object): arrays of n, None = the scene's value (set_params).
    set_agent_params() switches them off again."""
    L = lib()
    keep = []

    def arr(a, dt, ct):
        if a is None or n == 0:
            return None
        b = np.ascontiguousarray(a, dt).reshape(n)
        keep.append(b)
        return _p(b, ct)
    L.orc_set_agent_params(int(n), arr(neighbor_dist, np.float64, C.c_double), arr(max_neighbors, np.int32, C.c_int32), arr(time_step, np.float64, C.c_double),
                           arr(time_horizon, np.float64, C.c_double), arr(max_speed, np.float64, C.c_double), arr(max_heading_change, np.float64, C.c_double),
                           arr(dt_nominal, np.float64, C.c_double))


def set_list_rule(rule=0):
    """Which lists policy_step builds (process-wide).  0: the reference's -- kd visit order, the last entry popped when the list is full.
    1: the rule SCA_NBR_GRID documents -- sorted by (distSq, obstacles first, agent id), the nearest max_neighbors kept, status bit 32 where
    more objects were admitted than the list holds; everything behind the list (cones, planes, sweep, LP) is the same code."""
    if rule not in (0, 1):
        raise ValueError(f'unknown list rule {rule!r}')
    lib().orc_set_list_rule(int(rule))


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _d(a):
    return _p(a, C.c_double)


def vec3(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def policy_step(pos, vel, heading, radius, pref_speed, flags, goal, policy, zaxis, vpref_ext, vpref_mode, perm,
                obs_pos, obs_radius, nthreads=1):
    """One pass of the first loop of MACAEnv._take_action (mampenv.py:28-40).
    Returns a dict; `flags` and `perm` are copied, the updated copies are returned."""
    L = lib()
    n = int(len(radius))
    m = int(len(obs_radius))
    pos = np.ascontiguousarray(pos, np.float64).reshape(n, 3)
    vel = np.ascontiguousarray(vel, np.float32).reshape(n, 3)
    heading = np.ascontiguousarray(heading, np.float64).reshape(n, 3)
    radius = np.ascontiguousarray(radius, np.float64)
    pref_speed = np.ascontiguousarray(pref_speed, np.float64)
    flags = np.array(flags, np.uint8, copy=True)
    goal = np.ascontiguousarray(goal, np.float64).reshape(n, 3)
    policy = np.ascontiguousarray(policy, np.uint8)
    zaxis = np.ascontiguousarray(zaxis, np.uint8)
    vpref_ext = np.ascontiguousarray(np.nan_to_num(vpref_ext), np.float64).reshape(n, 3)
    vpref_mode = np.ascontiguousarray(vpref_mode, np.uint8)
    perm = np.array(perm, np.int32, copy=True)
    obs_pos = np.ascontiguousarray(obs_pos, np.float64).reshape(m, 3)
    obs_radius = np.ascontiguousarray(obs_radius, np.float64)
    out = dict(action64=np.zeros((n, 7)), action=np.zeros((n, 7), np.float32), nbr_n=np.zeros(n, np.int32),
               nbr_id=np.full((n, K), -1, np.int32), nbr_kind=np.zeros((n, K), np.uint8), nbr_dsq=np.zeros((n, K)),
               nbr_valid=np.zeros(n, np.uint8), vpref=np.zeros((n, 3)), diag=np.zeros((n, 5), np.int32),
               status=np.zeros(n, np.int32))
    L.orc_policy_step(n, m, _d(pos), _p(vel, C.c_float), _d(heading), _d(radius), _d(pref_speed), _p(flags, C.c_uint8),
                      _d(goal), _p(policy, C.c_uint8), _p(zaxis, C.c_uint8), _d(vpref_ext), _p(vpref_mode, C.c_uint8),
                      _p(perm, C.c_int32), _d(obs_pos), _d(obs_radius), _d(out['action64']),
                      _p(out['action'], C.c_float), _p(out['nbr_n'], C.c_int32), _p(out['nbr_id'], C.c_int32),
                      _p(out['nbr_kind'], C.c_uint8), _d(out['nbr_dsq']), _p(out['nbr_valid'], C.c_uint8),
                      _d(out['vpref']), _p(out['diag'], C.c_int32), _p(out['status'], C.c_int32), int(nthreads))
    out['flags'] = flags
    out['perm'] = perm
    return out


def env_update(pos, vel, heading, radius, flags, goal, action, total_dist, max_run_dist, step_num, obs_pos, obs_radius):
    """Second loop of _take_action + is_done (mampenv.py:42-59). Arrays are copied; updated copies returned."""
    L = lib()
    n = int(len(radius))
    m = int(len(obs_radius))
    pos = np.array(pos, np.float64, copy=True).reshape(n, 3)
    vel = np.array(vel, np.float32, copy=True).reshape(n, 3)
    heading = np.array(heading, np.float64, copy=True).reshape(n, 3)
    flags = np.array(flags, np.uint8, copy=True)
    total_dist = np.array(total_dist, np.float64, copy=True)
    step_num = np.array(step_num, np.int32, copy=True)
    radius = np.ascontiguousarray(radius, np.float64)
    goal = np.ascontiguousarray(goal, np.float64).reshape(n, 3)
    action = np.ascontiguousarray(action, np.float32).reshape(n, 7)
    max_run_dist = np.ascontiguousarray(max_run_dist, np.float64)
    obs_pos = np.ascontiguousarray(obs_pos, np.float64).reshape(m, 3)
    obs_radius = np.ascontiguousarray(obs_radius, np.float64)
    done = L.orc_env_update(n, m, _d(pos), _p(vel, C.c_float), _d(heading), _d(radius), _p(flags, C.c_uint8), _d(goal),
                            _p(action, C.c_float), _d(total_dist), _d(max_run_dist), _p(step_num, C.c_int32),
                            _d(obs_pos), _d(obs_radius))
    return dict(pos=pos, vel=vel, heading=heading, flags=flags, total_dist=total_dist, step_num=step_num, done=bool(done))


# ---------------------------------------------------------------------------------------------------- Dubins planner / v_pref tracker
# (sca_dubins_oracle.c: dubinsmaneuver2d.py / dubinsmaneuver3d.py / scaPolicy.py:92-104,243-338 on the host's libm)
PLAN_FIELDS = ('length', 'h_r', 'h_t', 'h_p', 'h_q', 'v_r', 'v_t', 'v_p', 'v_q', 'sampling', 'count', 'iters')


def dubins_plan(qi, qf, rmin=1.5, pitchlims=(-math.pi / 4, math.pi / 4), ks=()):
    """dubinsmaneuver3d.dubinsmaneuver3d(qi, qf, Rmin, pitchlims): dict of PLAN_FIELDS + 'mode' (six letters) + 'samples' (the path
    elements of the indices ks, [len(ks), 5]).  Raises when the reference would not return a plan."""
    L = lib()
    qi = np.ascontiguousarray(qi, np.float64)[:5].copy()
    qf = np.ascontiguousarray(qf, np.float64)[:5].copy()
    ks = np.ascontiguousarray(ks, np.int64).reshape(-1)
    out = np.zeros(12)
    mode = C.create_string_buffer(8)
    samples = np.zeros((max(len(ks), 1), 5))
    rc = L.orc_dubins_plan(_d(qi), _d(qf), float(rmin), float(pitchlims[0]), float(pitchlims[1]), _d(out), mode,
                           _p(ks, C.c_int64), len(ks), _d(samples))
    if rc != 0:
        raise RuntimeError(f'orc_dubins_plan status {rc}')
    r = dict(zip(PLAN_FIELDS, out.tolist()))
    r['count'], r['iters'] = int(r['count']), int(r['iters'])
    r['mode'] = mode.value.decode()
    r['samples'] = samples[:len(ks)]
    return r


def dubins_plan_batch(q, rmin, pitch_lo, pitch_hi, nthreads=0):
    """Many plans: q [n, 10] = qi[5] | qf[5]; rmin / pitch_lo / pitch_hi scalars or arrays of n.  Returns [n, 16]: PLAN_FIELDS, the two
    words packed as 65536 c0 + 256 c1 + c2 (the product's debug record's form), the status (0 = a plan the reference would return), 0."""
    L = lib()
    q = np.ascontiguousarray(q, np.float64).reshape(-1, 10)
    n = len(q)
    r, lo, hi = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), (n,))) for a in (rmin, pitch_lo, pitch_hi))
    out = np.zeros((n, 16))
    L.orc_dubins_plan_batch(n, _d(q), _d(r), _d(lo), _d(hi), _d(out), int(nthreads))
    return out


class Tracker:
    """The v_pref tracker of SCAPolicy / RVO3dDubinsPolicy, one state per agent (compute_v_pref, scaPolicy.py:264-338)."""

    def __init__(self, goal, goal_heading, pref_speed, zaxis, turning_radius=1.5, pitchlims=(-math.pi / 4, math.pi / 4),
                 neighbor_dist=10.0):
        self.L = lib()
        goal = np.ascontiguousarray(goal, np.float64).reshape(-1, 3)
        self.n = n = len(goal)
        gh = np.ascontiguousarray(goal_heading, np.float64).reshape(n, 3)
        ps = np.ascontiguousarray(np.broadcast_to(np.asarray(pref_speed, np.float64), (n,)))
        za = np.ascontiguousarray(zaxis, np.uint8).reshape(n)
        self.h = self.L.orc_tracker_create(n, _d(goal), _d(gh), _d(ps), _p(za, C.c_uint8), float(turning_radius), float(pitchlims[0]),
                                           float(pitchlims[1]), float(neighbor_dist))
        if not self.h:
            raise RuntimeError('orc_tracker_create failed')
        self.nbr0 = np.full(n, -1.0)           # agent.neighbors[0][1] as the last policy pass left it (-1: empty)

    def set_params(self, neighbor_dist=None, turning_radius=None, pitch_lo=None, pitch_hi=None):
        """per-agent agent.neighborDist / turning_radius / pitchlims (arrays of n; None = the constructor's value)"""
        keep = []

        def arr(a):
            if a is None:
                return None
            b = np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), (self.n,)))
            keep.append(b)
            return _d(b)
        if self.L.orc_tracker_set_params(self.h, arr(neighbor_dist), arr(turning_radius), arr(pitch_lo), arr(pitch_hi)) != 0:
            raise RuntimeError('orc_tracker_set_params failed')

    def note_neighbors(self, nbr_valid, nbr_n, nbr_dsq):
        """agent.neighbors[0] after a policy pass: only the agents whose list the pass recomputed (scaPolicy.py:45,108)"""
        v = np.asarray(nbr_valid).astype(bool)
        first = np.where(np.asarray(nbr_n) > 0, np.asarray(nbr_dsq)[:, 0], -1.0)
        self.nbr0[v] = first[v]

    def note_nbr0(self, nbr0):
        """the same from the product's compact form (sca_get_nbr0: -2 = list untouched by the pass)"""
        nbr0 = np.asarray(nbr0)
        m = nbr0 > -2.0
        self.nbr0[m] = nbr0[m]

    def vpref(self, pos, vel, heading, active, nthreads=0):
        """V_des of every active agent (rows of the others: nan).  Raises when an agent met a case where the reference raises or
        loops forever."""
        n = self.n
        pos = np.ascontiguousarray(pos, np.float64).reshape(n, 3)
        vel = np.ascontiguousarray(vel, np.float32).reshape(n, 3)
        heading = np.ascontiguousarray(heading, np.float64).reshape(n, 3)
        active = np.ascontiguousarray(active, np.uint8).reshape(n)
        out = np.full((n, 3), np.nan)
        bad = self.L.orc_tracker_vpref(self.h, _d(pos), _p(vel, C.c_float), _d(heading), _p(active, C.c_uint8), _d(self.nbr0), _d(out),
                                       int(nthreads))
        if bad != 0:
            raise RuntimeError(f'oracle tracker: {bad} agents met a case the reference does not survive')
        return out

    def replans(self):
        r = np.zeros(self.n, np.int32)
        self.L.orc_tracker_replans(self.h, _p(r, C.c_int32))
        return r

    def debug(self, i):
        """agent i's plan and tracking state in the layout of the product's sca_tracker_debug record"""
        o = np.zeros(24)
        if self.L.orc_tracker_debug(self.h, int(i), _d(o)) != 0:
            raise IndexError(i)
        return o

    def close(self):
        if getattr(self, 'h', None):
            self.L.orc_tracker_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
