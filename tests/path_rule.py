"""The waypoint rule of the reference, restated in plain Python for the tests: get_trajectory (the first statement of every policy's
find_next_action) and the straight-line policies' compute_v_pref toward policy.now_goal.  Written from the reference's behaviour:

    rvo3dPolicy.py:71-85, srvo3dPolicy.py:71-85, scaPolicy.py:75-89, sca/rvo3dDubinsPolicy.py:73-87   measure with l3norm (util.py:104)
    orca3dPolicy.py:298-312, orca3dPolicyOfficial.py:302-316                                          measure with distance (util.py:140)
    rvo3dPolicy.py:29,182-196 / orca3dPolicy.py:49,348-362                                            v_pref toward now_goal, zeroed at the goal

A list is a Python list of [x, y, z]; list.pop() takes the last element.  now_goal None = no waypoint taken yet.
"""
import math

import numpy as np

POL_SCA, POL_RVO3D, POL_SRVO3D, POL_ORCA3D, POL_ORCA3D_LP, POL_RVO3D_DUBINS = range(6)
ORCA = (POL_ORCA3D, POL_ORCA3D_LP)
TRACKED = (POL_SCA, POL_RVO3D_DUBINS)
EPS = 10 ** 5


def l3norm(p, q):
    return round(math.sqrt((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 + (p[2] - q[2]) ** 2), 5)


def distance(p, q):
    return round(math.sqrt((p[0] - q[0]) ** 2 + (p[1] - q[1]) ** 2 + (p[2] - q[2]) ** 2) + 1e-5, 5)


def advance(path, now_goal, pos, goal, radius, policy):
    """One get_trajectory call.  Pops from `path` in place; returns the new now_goal (an array, or goal itself for an empty list)."""
    if not path:
        return np.asarray(goal, dtype=np.float64)
    dist = distance if policy in ORCA else l3norm
    if now_goal is None:
        now_goal = np.array(path.pop(), dtype=np.float64)
    near = dist(pos, now_goal) <= 1.0 * radius
    behind = dist(now_goal, goal) >= dist(pos, goal)
    if near or behind:
        if path:
            now_goal = np.array(path.pop(), dtype=np.float64)
    return now_goal


def v_pref_toward(aim, pos, goal, pref_speed, policy):
    """compute_v_pref(now_goal, agent) of the straight-line policies: the truncated V_des."""
    dist = distance if policy in ORCA else l3norm
    dif = np.asarray(aim, dtype=np.float64) - np.asarray(pos, dtype=np.float64)
    norm = int(dist(dif, [0, 0, 0]) * EPS) / EPS
    with np.errstate(divide='ignore', invalid='ignore'):
        v = dif * pref_speed / norm
    if l3norm(goal, pos) < 0.2:
        v = np.zeros(3)
    return np.array([int(v[0] * EPS) / EPS, int(v[1] * EPS) / EPS, int(v[2] * EPS) / EPS])


def pass_rule(paths, now_goal, pos, goal, radius, pref_speed, policy, flags, has_path=None):
    """The rule over a swarm for one pass, in place on `paths` (lists) and `now_goal` ([n, 3], NaN rows = None).  Returns (vpref_ext [n, 3],
    mode [n] uint8): the v_pref a straight-line agent with a path aims at its waypoint with (mode 1), zeros / 0 for everybody else.
    has_path[i]: the agent was given a non-empty list (default: its list is not empty now)."""
    n = len(paths)
    vp = np.zeros((n, 3))
    mode = np.zeros(n, np.uint8)
    for i in range(n):
        if flags[i] & 7:
            continue
        ng = None if np.isnan(now_goal[i, 0]) else now_goal[i].copy()
        hp = bool(paths[i]) if has_path is None else bool(has_path[i])
        ng = advance(paths[i], ng, pos[i], goal[i], float(radius[i]), int(policy[i]))
        now_goal[i] = ng
        if hp and int(policy[i]) not in TRACKED:
            vp[i] = v_pref_toward(ng, pos[i], goal[i], float(pref_speed[i]), int(policy[i]))
            mode[i] = 1
    return vp, mode


def csr(paths):
    """(offsets [n + 1] int32, points [total, 3]) of per-agent lists"""
    lens = [len(p) for p in paths]
    off = np.zeros(len(paths) + 1, np.int32)
    off[1:] = np.cumsum(lens)
    pts = np.zeros((int(off[-1]), 3))
    for i, p in enumerate(paths):
        if p:
            pts[off[i]:off[i + 1]] = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    return off, pts


def lists_from_csr(off, pts, remaining=None):
    """per-agent lists (their first remaining[i] elements) from the CSR form"""
    n = len(off) - 1
    out = []
    for i in range(n):
        k = int(off[i + 1] - off[i]) if remaining is None else int(remaining[i])
        out.append([list(map(float, pts[off[i] + j])) for j in range(k)])
    return out


def _round5(a):
    """Python's round(x, 5) element by element (numpy's round is not the same rounding)"""
    return np.array([round(x, 5) for x in np.asarray(a, dtype=np.float64).tolist()])


def _dist(p, q, use_distance):
    d = np.asarray(p, dtype=np.float64) - np.asarray(q, dtype=np.float64)
    s = np.sqrt((d[:, 0] ** 2 + d[:, 1] ** 2) + d[:, 2] ** 2)
    return _round5(np.where(use_distance, s + 1e-5, s))


def pass_rule_csr(off, pts, remaining, now_goal, pos, goal, radius, pref_speed, policy, flags):
    """pass_rule over arrays, for swarms too large for a loop over agents: the lists are the CSR form (off, pts) with remaining[i] elements
    left.  Returns (remaining, now_goal, vpref_ext, mode) as new arrays.  Equal to pass_rule, the sign of a zero included: the oracle's
    heading comes from atan2 of this v_pref (tests/test_paths_cpu.py, tests/test_form_fuzz_cpu.py)."""
    n = len(off) - 1
    off = np.asarray(off, np.int64)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    rem = np.array(remaining, np.int64, copy=True)
    ng = np.array(now_goal, dtype=np.float64, copy=True)
    pos = np.asarray(pos, dtype=np.float64)
    goal = np.asarray(goal, dtype=np.float64)
    policy = np.asarray(policy)
    served = (np.asarray(flags) & 7) == 0
    orca = np.isin(policy, ORCA)
    ng[served & (rem == 0)] = goal[served & (rem == 0)]
    act = served & (rem > 0)
    first = act & np.isnan(ng[:, 0])
    ng[first] = pts[off[:-1][first] + rem[first] - 1]
    rem[first] -= 1
    dis, dis_goal, dis_pos = _dist(pos, ng, orca), _dist(ng, goal, orca), _dist(pos, goal, orca)
    with np.errstate(invalid='ignore'):
        again = act & ((dis <= radius) | (dis_goal >= dis_pos)) & (rem > 0)
    ng[again] = pts[off[:-1][again] + rem[again] - 1]
    rem[again] -= 1
    mode = served & (np.diff(off) > 0) & ~np.isin(policy, TRACKED)
    vp = np.zeros((n, 3))
    m = np.flatnonzero(mode)
    if m.size:
        dif = ng[m] - pos[m]
        nrm = np.trunc(_dist(dif, np.zeros((m.size, 3)), orca[m]) * EPS) / EPS
        with np.errstate(divide='ignore', invalid='ignore'):
            v = dif * np.asarray(pref_speed, dtype=np.float64)[m, None] / nrm[:, None]
        v[_dist(goal[m], pos[m], np.zeros(m.size, bool)) < 0.2] = 0.0
        vp[m] = np.trunc(v * EPS) / EPS + 0.0                                    # (int(-0.6) / EPS is 0.0 where trunc(-0.6) / EPS is -0.0)
    return rem.astype(np.int32), ng, vp, mode.astype(np.uint8)
