"""Respawning agents in place, stated with the oracle alone: the free-running oracle trajectory of a fuzz scene (tests/form_fuzz.py) in
which, before every step -- step 0 included -- each row that carries a done flag gets a new mission with probability 0.5.  The reference's
rule is plain Python: assigning pos_global_frame, goal_global_frame, is_at_goal = False, ... to one Agent object between two env.step()
calls (mampenv.py:16-19); the kd-tree keeps its agentIDs order and every other agent is untouched -- here: the named rows of the state and
definition arrays are overwritten, `perm` is carried as it is.  Shared by tests/test_respawn_cpu.py (what the corpus holds) and
tests/test_gpu_respawn.py (every kernel form against it).  Test infrastructure: it drives the oracle, the product never imports it."""
import collections

import numpy as np

import form_fuzz as F
import path_rule as R

STEPS = 12
SEEDS = range(40)
RNG_BASE = 10_000
DEF_KEYS = ('radius', 'pref_speed', 'goal', 'max_run_dist')
DONE = 7


def box_of(scene):
    """the half side of the scene's box in x and y (form_fuzz draws -side .. side), from what the scene holds; at least 1 m"""
    return max(1.0, float(np.abs(scene['pos'][:, :2]).max()), float(np.abs(scene['goal'][:, :2]).max()))


def draw(rng, flags, side):
    """The missions drawn before a step for the rows of `flags` that are done: None, or a dict of packed arrays in ascending id order.
    Position and goal uniform in the box with z = |z| + 1, every fourth named row's goal 0.6 .. 2 m from its new start, a random yaw, zero
    velocity, radius from {0.3, 0.5, 1.0}, pref_speed from {1.0, 0.8, 1.5}, max_run_dist = 3 |start - goal| + 1."""
    n = len(flags)
    take = ((np.asarray(flags) & DONE) != 0) & (rng.random(n) < 0.5)
    ids = np.flatnonzero(take).astype(np.int32)
    k = len(ids)
    if k == 0:
        return None
    pos = rng.uniform(-side, side, (k, 3))
    pos[:, 2] = np.abs(pos[:, 2]) + 1.0
    goal = rng.uniform(-side, side, (k, 3))
    goal[:, 2] = np.abs(goal[:, 2]) + 1.0
    u = rng.normal(0, 1, (k, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    near = pos + u * rng.uniform(0.6, 2.0, (k, 1))
    near[:, 2] = np.abs(near[:, 2])
    fourth = np.arange(k) % 4 == 3
    goal[fourth] = near[fourth]
    heading = np.zeros((k, 3))
    heading[:, 0] = rng.uniform(0, 2 * np.pi, k)
    return dict(ids=ids, pos=pos, vel=np.zeros((k, 3), np.float32), heading=heading, radius=rng.choice([0.3, 0.5, 1.0], k),
                pref_speed=rng.choice([1.0, 0.8, 1.5], k), goal=goal, max_run_dist=3.0 * np.linalg.norm(pos - goal, axis=1) + 1.0)


def random_lists(rng, mission, radius):
    """0 .. 3 waypoints for every named row of a mission, between its start and its goal (rounded to 3 places), some within the radius"""
    out = []
    for j in range(len(mission['ids'])):
        p, g = mission['pos'][j], mission['goal'][j]
        lst = []
        for _ in range(int(rng.choice([0, 1, 2, 3]))):
            w = p + (g - p) * rng.uniform(0.0, 0.9) + rng.normal(0, 0.3 * float(radius[j]), 3)
            lst.append([float(x) for x in np.round(w, 3)])
        out.append(lst)
    return out


def apply(state, defs, mission):
    """the named rows of the state (pos, vel, heading, flags, total_dist, step_num) and of the definition become the mission's, in place"""
    ids = mission['ids']
    state['pos'][ids] = mission['pos']
    state['vel'][ids] = mission['vel']
    state['heading'][ids] = mission['heading']
    state['flags'][ids] = 0
    state['total_dist'][ids] = 0.0
    state['step_num'][ids] = 0
    for k in DEF_KEYS:
        defs[k][ids] = mission[k]


_RUNS = collections.OrderedDict()
_RUNS_MAX = 24


def oracle_run(oracle, scene, steps=STEPS, list_rule=0, respawn_every=1, lists=None):
    """The trajectory with respawns.  One dict per step: `mission` (what was respawned before the step, or None), `active_before` (rows
    without a done flag when the step starts), `defs` (the definition the step ran with), everything form_fuzz.oracle_run records
    (action, lists, diag, perm, `before`, `flags_policy`, the state after the step) and `finished` (np.flatnonzero of the done flags after
    the step).  respawn_every: missions are drawn only before steps t with t % respawn_every == 0 (a burst of steps between respawns).
    lists: W > 0 -- the scene runs with waypoint lists in slot form: random_paths(seed) at the start (cut to W), every mission brings
    random_lists or, every third mission, none (the rows lose their lists); path_rule advances them as in form_fuzz.oracle_run.
    Memoised; the arrays are shared: nobody writes to them."""
    key = scene['key'] + (steps, list_rule, respawn_every, lists)
    if key in _RUNS:
        _RUNS.move_to_end(key)
        return _RUNS[key]
    s, n = scene, scene['n']
    seed = scene['key'][1]
    rng = np.random.default_rng(RNG_BASE + seed)
    side = box_of(s)
    zaxis = F.zaxis_of(s)
    st = dict(pos=s['pos'].copy(), vel=s['vel'].copy(), heading=s['heading'].copy(), flags=s['flags'].copy(), total_dist=np.zeros(n),
              step_num=np.zeros(n, np.int32))
    defs = {k: np.array(s[k], np.float64, copy=True) for k in DEF_KEYS}
    perm = np.arange(n, dtype=np.int32)
    if lists:
        paths = [lst[:lists] for lst in F.random_paths(seed, s)]
        missions = 0
    out = []
    try:
        oracle.set_list_rule(list_rule)
        if lists:
            rem, ng = np.array([len(p) for p in paths], np.int32), np.full((n, 3), np.nan)
        for t in range(steps):
            mission = draw(rng, st['flags'], side) if t % respawn_every == 0 else None
            if mission is not None:
                st = {k: v.copy() for k, v in st.items()}
                defs = {k: v.copy() for k, v in defs.items()}
                apply(st, defs, mission)
                if lists:
                    missions += 1
                    mission['paths'] = None if missions % 3 == 0 else random_lists(rng, mission, mission['radius'])
                    paths = list(paths)
                    rem, ng = rem.copy(), ng.copy()
                    for j, a in enumerate(mission['ids']):
                        paths[a] = [] if mission['paths'] is None else mission['paths'][j]
                        rem[a] = len(paths[a])
                        ng[a] = np.nan
            vpref, vmode, path = s['vpref'], s['vmode'], {}
            if lists:
                off, pts = R.csr(paths)
                path = dict(path_left_before=rem, now_goal_before=ng, pos_before=st['pos'], path_off=off, path_pts=pts)
                rem, ng, vp, mode = R.pass_rule_csr(off, pts, rem, ng, st['pos'], defs['goal'], defs['radius'], defs['pref_speed'], s['policy'], st['flags'])
                aimed = mode.astype(bool)
                vpref, vmode = np.where(aimed[:, None], vp, s['vpref']), np.where(aimed, 1, s['vmode']).astype(np.uint8)
                path.update(path_left=rem, now_goal=ng, vpref_rule=vp, path_mode=mode)
            r = oracle.policy_step(st['pos'], st['vel'], st['heading'], defs['radius'], defs['pref_speed'], st['flags'], defs['goal'], s['policy'],
                                   zaxis, vpref, vmode, perm, s['obs_pos'], s['obs_radius'], nthreads=8)
            perm = r['perm']
            u = oracle.env_update(st['pos'], st['vel'], st['heading'], defs['radius'], r['flags'], defs['goal'], r['action'], st['total_dist'],
                                  defs['max_run_dist'], st['step_num'], s['obs_pos'], s['obs_radius'])
            step = {k: r[k] for k in ('action', 'nbr_valid', 'nbr_n', 'nbr_id', 'nbr_kind', 'nbr_dsq', 'diag', 'perm', 'status', 'vpref')}
            step.update(mission=mission, before=st['flags'], active_before=int(((st['flags'] & DONE) == 0).sum()), flags_policy=r['flags'], defs=defs)
            step.update(path)
            st = {k: u[k] for k in F.STATE_KEYS}
            step.update(st)
            step['finished'] = np.flatnonzero((st['flags'] & DONE) != 0)
            out.append(step)
    finally:
        oracle.set_list_rule(0)
    _RUNS[key] = out
    while len(_RUNS) > _RUNS_MAX:
        _RUNS.popitem(last=False)
    return out


QUANTITIES = ('respawns', 'repeats', 'collisions', 'arrivals', 'lp_rows', 'tracked_rows', 'list_entries')


def corpus_counts(scene, run):
    """What a run feeds the respawn with, counted from the oracle's records and the rule alone: rows respawned, those respawned before
    (repeats), done flags respawned rows gained afterwards (collisions: bit 2, arrivals: bit 1), ORCA3D-LP and tracked (SCA /
    RVO3D+Dubins) rows respawned, and neighbour-list entries that name an agent that has been respawned."""
    n = scene['n']
    c = dict.fromkeys(QUANTITIES, 0)
    ever = np.zeros(n, bool)
    for st in run:
        m = st['mission']
        if m is not None:
            ids = m['ids']
            c['respawns'] += len(ids)
            c['repeats'] += int(ever[ids].sum())
            c['lp_rows'] += int((scene['policy'][ids] == 4).sum())
            c['tracked_rows'] += int(np.isin(scene['policy'][ids], (0, 5)).sum())
            ever[ids] = True
        gained = st['flags'] & ~st['before']
        c['collisions'] += int((ever & ((gained & 2) != 0)).sum())
        c['arrivals'] += int((ever & ((gained & 1) != 0)).sum())
        in_list = (np.arange(F.K)[None, :] < st['nbr_n'][:, None]) & (st['nbr_valid'][:, None] != 0) & (st['nbr_kind'] == 0)
        ids_named = np.where(in_list, st['nbr_id'], 0)
        c['list_entries'] += int((in_list & ever[ids_named]).sum())
    return c
