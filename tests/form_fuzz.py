"""The random-scene corpus of the fuzz tests and its oracle runs, shared by tests/test_gpu_parity.py (the default kernel forms),
tests/test_gpu_form_fuzz.py (every other form of sca_forms.h forced at the same small sizes), tests/test_gpu_path_fuzz.py (the same forms with
waypoint lists: random_paths, oracle_run(paths=...)) and tests/test_form_fuzz_cpu.py (what the corpus holds, counted from the oracle and the
rule of tests/path_rule.py alone).  Test infrastructure: it drives the oracle, the product never imports it."""
import collections
import math

import numpy as np

import path_rule as R

K = 16
STATE_KEYS = ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num')
BLOCK = 20                                     # seeds per test
PLAIN_SEEDS = range(0, 120)
PER_AGENT_SEEDS = range(1000, 1060)
SWITCH_SIZES = (2047, 2049, 6143, 6145)        # either side of k_solve_fb's and of packed K1's default threshold at 1024 SIMDs

# the form rows: the SCA_* switches of sca_forms.h that force a form at any size (read by sca_create)
ROWS = {
    'packed': {'SCA_K1_PACKED': '1'},
    'split': {'SCA_SOLVE_SPLIT': '1'},                                   # with LP agents in the scene this also routes them to k_lp
    'lp_lane': {'SCA_LP_FORM': 'lane'},
    'fallback_launch': {'SCA_SOLVE_FB_MAX': '0', 'SCA_ACTION_FB_MAX': '0'},
    'solve_fb': {},                                                      # the default of a shard without LP agents: the no_lp variant
    'large_shard': {'SCA_K1_PACKED': '1', 'SCA_SOLVE_SPLIT': '1', 'SCA_SOLVE_FB_MAX': '0', 'SCA_ACTION_FB_MAX': '0'},
    'kd_levels': {'SCA_KD_TOP': '0', 'SCA_KD_WAVE_CAP': '256', 'SCA_KD_TICKET': '1'},
}
PER_AGENT_ROWS = ('packed', 'split', 'lp_lane', 'large_shard')


def random_scene(seed):
    """A random scene for the fuzz test: any agent count, obstacles, mixed policies, agents that are done from the start,
    dense boxes (collisions, > 16 in range), agents on the ground, zero velocities, goals straight above the start."""
    rng = np.random.default_rng(seed)
    n = int(rng.choice([1, 2, 3, 9, 17, 33, 64, 100, 257, 400, 900, 1600]))
    m = int(rng.choice([0, 0, 1, 5, 30]))
    side = float(rng.choice([4.0, 10.0, 30.0, 80.0]))
    pos = rng.uniform(-side, side, (n, 3))
    pos[:, 2] = np.abs(pos[:, 2]) + rng.choice([0.0, 1.0, 20.0])
    goal = rng.uniform(-side, side, (n, 3))
    goal[:, 2] = np.abs(goal[:, 2]) + 1.0
    if rng.random() < 0.3:
        goal[: n // 2, :2] = pos[: n // 2, :2]                             # is_zAxis agents (scaPolicy.py:188-190)
    head = np.zeros((n, 3))
    head[:, 0] = rng.uniform(0, 2 * np.pi, n)
    head[:, 1] = rng.uniform(-0.5, 0.5, n)
    v = rng.normal(0, 1, (n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v *= rng.uniform(0, 1, (n, 1))
    if rng.random() < 0.3:
        v[rng.random(n) < 0.3] = 0.0                                       # bootstrap branch for some
    policy = rng.integers(0, 6, n).astype(np.uint8)
    flags = ((rng.random(n) < 0.1) * rng.choice([1, 2, 4], n)).astype(np.uint8)
    obs_pos = rng.uniform(-side, side, (m, 3))
    obs_pos[:, 2] = np.abs(obs_pos[:, 2])
    vpx = np.trunc(rng.normal(0, 0.6, (n, 3)) * 1e5) / 1e5                 # "tracker output" for SCA / RVO3D+Dubins
    return dict(n=n, m=m, pos=pos, goal=goal, heading=head, vel=v.astype(np.float32), radius=rng.choice([0.3, 0.5, 1.0], n),
                pref_speed=rng.choice([1.0, 1.0, 0.8, 1.5], n), policy=policy, flags=flags, obs_pos=obs_pos,
                obs_radius=rng.choice([0.2, 1.0, 2.0], m), vpref=vpx, vmode=np.isin(policy, (0, 5)).astype(np.uint8),
                max_run_dist=3.0 * np.linalg.norm(pos - goal, axis=1) + 1.0, key=('random', seed))


def per_agent_attributes(seed, n):
    """The solver attributes of the per-agent fuzz for random_scene(seed): (per, params, uniform).  `per`: one draw per agent; every third
    scene is `uniform` -- agent 0's draw for the whole scene, as `params` (sca_params), and no per-agent arrays."""
    rng = np.random.default_rng(77 + seed)
    mhc = rng.choice([0.3, math.pi / 6, math.pi / 4, 1.2, math.pi / 2], n)
    per = dict(neighbor_dist=rng.choice([1.5, 2.5, 4.0, 10.0, 15.0, 30.0], n), max_neighbors=rng.choice([1, 2, 4, 8, 12, 16], n).astype(np.int32),
               time_step=rng.choice([0.05, 0.1, 0.2], n), time_horizon=rng.choice([1.0, 3.0, 10.0, 20.0], n), max_speed=rng.choice([0.7, 1.0, 1.5, 3.0], n),
               max_heading_change=mhc, dt_nominal=rng.choice([0.05, 0.1], n))
    uniform = seed % 3 == 0
    params = {k: (int(v[0]) if k == 'max_neighbors' else float(v[0])) for k, v in per.items()} if uniform else {}
    return per, params, uniform


PATH_SEED = 5000                               # random_paths draws from default_rng(PATH_SEED + seed): the scenes themselves do not change


def random_paths(seed, scene):
    """Waypoint lists (Agent.path) for random_scene(seed) / switch_scene(seed): 0-5 waypoints per agent, each one of five kinds, rounded to 3
    places (p = start, g = goal, u = the unit vector from p to g, r = radius):
        0 near     p + u * U(0, r + 0.8) + N(0, 0.05)    within the radius now or after a few steps
        1 behind   p - u * U(0.5, 5)
        2 ahead    p + (g - p) * U(0.1, 0.9) + N(0, 1)
        3 the goal itself
        4 around the radius' edge   p + N(0, r)
    A list is in list order: get_trajectory pops from its end."""
    rng = np.random.default_rng(PATH_SEED + seed)
    paths = []
    for i in range(scene['n']):
        p, g, r = scene['pos'][i], scene['goal'][i], float(scene['radius'][i])
        d = float(np.linalg.norm(g - p))
        u = (g - p) / d if d > 0 else np.zeros(3)
        lst = []
        for _ in range(int(rng.choice([0, 0, 1, 2, 3, 5]))):
            kind = int(rng.integers(0, 5))
            if kind == 0:
                w = p + u * rng.uniform(0, r + 0.8) + rng.normal(0, 0.05, 3)
            elif kind == 1:
                w = p - u * rng.uniform(0.5, 5)
            elif kind == 2:
                w = p + (g - p) * rng.uniform(0.1, 0.9) + rng.normal(0, 1, 3)
            elif kind == 3:
                w = g
            else:
                w = p + rng.normal(0, r, 3)
            lst.append([float(x) for x in np.round(w, 3)])
        paths.append(lst)
    return paths


def switch_scene(n):
    """A scene of n agents drawn as tests/fuzz_oracle.py draws its scenes, at one setting: 0.05 agents per cubic metre, 40 obstacles, all six
    policies mixed, 5 % of the agents done from the start (seeded by n)."""
    rng = np.random.default_rng(n)
    m = 40
    side = max(2.0, 0.5 * (n / 0.05) ** (1.0 / 3.0))
    pos = rng.uniform(-side, side, (n, 3))
    pos[:, 2] = np.abs(pos[:, 2]) + float(rng.choice([0.0, 1.0, 20.0]))
    goal = rng.uniform(-side, side, (n, 3))
    goal[:, 2] = np.abs(goal[:, 2]) + 1.0
    if rng.random() < 0.3:
        goal[: n // 2, :2] = pos[: n // 2, :2]
    head = np.zeros((n, 3))
    head[:, 0] = rng.uniform(0, 2 * np.pi, n)
    head[:, 1] = rng.uniform(-0.5, 0.5, n)
    v = rng.normal(0, 1, (n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v *= rng.uniform(0, 1, (n, 1))
    if rng.random() < 0.3:
        v[rng.random(n) < 0.3] = 0.0
    policy = rng.integers(0, 6, n).astype(np.uint8)
    flags = ((rng.random(n) < 0.05) * rng.choice([1, 2, 4], n)).astype(np.uint8)
    obs_pos = rng.uniform(-side, side, (m, 3))
    obs_pos[:, 2] = np.abs(obs_pos[:, 2])
    vpx = np.trunc(rng.normal(0, 0.6, (n, 3)) * 1e5) / 1e5
    return dict(n=n, m=m, pos=pos, goal=goal, heading=head, vel=v.astype(np.float32), radius=rng.choice([0.3, 0.5, 1.0], n),
                pref_speed=rng.choice([1.0, 1.0, 0.8, 1.5], n), policy=policy, flags=flags, obs_pos=obs_pos,
                obs_radius=rng.choice([0.2, 1.0, 2.0], m), vpref=vpx, vmode=np.isin(policy, (0, 5)).astype(np.uint8),
                max_run_dist=3.0 * np.linalg.norm(pos - goal, axis=1) + 1.0, key=('switch', n))


def no_lp(scene):
    """the same scene with the ORCA3D-LP agents (policy 4) as ORCA3D agents (3): a shard without LP agents, which k_solve_fb may take"""
    s = dict(scene)
    s['policy'] = np.where(scene['policy'] == 4, 3, scene['policy']).astype(np.uint8)
    s['key'] = scene['key'] + ('no_lp',)
    return s


def zaxis_of(scene):
    """is_zAxis of scaPolicy.py:188-189 (sca_amd.solver.zaxis_flags, restated: this module runs without the product)"""
    d = scene['goal'] - scene['pos']
    return ((np.abs(d[:, 0]) <= 1e-5) & (np.abs(d[:, 1]) <= 1e-5)).astype(np.uint8)


_RUNS = collections.OrderedDict()
_RUNS_MAX = 3 * BLOCK                          # the rows of one block run one after the other: a block or two stay, the rest goes


def oracle_run(oracle, scene, steps, per_agent=None, list_rule=0, paths=None):
    """The free-running oracle trajectory of a scene: policy_step then env_update per step, from the scene's own state.  One dict per step:
    action, nbr_valid, nbr_n, nbr_id, nbr_kind, nbr_dsq, diag, perm, `before` (the flags the step started from), `flags_policy` (the flags after
    the policy pass) and the state after the step (STATE_KEYS).  per_agent: what per_agent_attributes returned.  list_rule: 0 the reference's lists
    (what SCA_NBR_KDTREE and SCA_NBR_AUTO return), 1 the lists SCA_NBR_GRID documents (oracle.set_list_rule); `status` then carries bit 32 on the
    rows that overflowed.  paths: what random_paths returned -- before each policy_step the rule (path_rule.pass_rule_csr) advances the lists; its
    v_pref goes in on the rows it aims at a waypoint (mode 1), the scene's fed vpref / vmode stay on the tracked rows (their lists advance, their
    v_pref stays fed, as in k_waypoint) and every other row gets mode 0; each step then also records path_left, now_goal, vpref_rule and path_mode
    (after the rule), path_left_before, now_goal_before, pos_before (what the rule started from) and the lists' CSR form (path_off, path_pts).  Memoised per scene and variant: every form
    row of a block compares against one run.  The arrays are shared: nobody writes to them."""
    key = scene['key'] + (per_agent is not None,) + (('rule', list_rule) if list_rule else ()) + (('paths',) if paths is not None else ())
    have = _RUNS.get(key)
    if have is not None and len(have) >= steps:
        _RUNS.move_to_end(key)
        return have[:steps]
    s, n = scene, scene['n']
    zaxis = zaxis_of(s)
    p, ve, he, fl = s['pos'].copy(), s['vel'].copy(), s['heading'].copy(), s['flags'].copy()
    td, sn, perm = np.zeros(n), np.zeros(n, np.int32), np.arange(n, dtype=np.int32)
    out = []
    if paths is not None:
        off, pts = R.csr(paths)
        rem, ng = np.diff(off).astype(np.int32), np.full((n, 3), np.nan)
    try:
        oracle.set_list_rule(list_rule)
        if per_agent is not None:
            per, params, uniform = per_agent
            oracle.set_params(**params)
            if uniform:
                oracle.set_agent_params()
            else:
                oracle.set_agent_params(n, **per)
        for _ in range(steps):
            vpref, vmode, path = s['vpref'], s['vmode'], {}
            if paths is not None:
                path = dict(path_left_before=rem, now_goal_before=ng, pos_before=p, path_off=off, path_pts=pts)
                rem, ng, vp, mode = R.pass_rule_csr(off, pts, rem, ng, p, s['goal'], s['radius'], s['pref_speed'], s['policy'], fl)
                aimed = mode.astype(bool)
                vpref, vmode = np.where(aimed[:, None], vp, s['vpref']), np.where(aimed, 1, s['vmode']).astype(np.uint8)
                path.update(path_left=rem, now_goal=ng, vpref_rule=vp, path_mode=mode)
            r = oracle.policy_step(p, ve, he, s['radius'], s['pref_speed'], fl, s['goal'], s['policy'], zaxis, vpref, vmode,
                                   perm, s['obs_pos'], s['obs_radius'], nthreads=8)
            perm = r['perm']
            u = oracle.env_update(p, ve, he, s['radius'], r['flags'], s['goal'], r['action'], td, s['max_run_dist'], sn,
                                  s['obs_pos'], s['obs_radius'])
            step = {k: r[k] for k in ('action', 'nbr_valid', 'nbr_n', 'nbr_id', 'nbr_kind', 'nbr_dsq', 'diag', 'perm', 'status')}
            step['before'], step['flags_policy'] = fl, r['flags']
            step.update(path)
            p, ve, he, fl, td, sn = u['pos'], u['vel'], u['heading'], u['flags'], u['total_dist'], u['step_num']
            step.update(pos=p, vel=ve, heading=he, flags=fl, total_dist=td, step_num=sn)
            out.append(step)
    finally:
        oracle.set_params()
        oracle.set_agent_params()
        oracle.set_list_rule(0)
    _RUNS[key] = out
    while len(_RUNS) > _RUNS_MAX:
        _RUNS.popitem(last=False)
    return out


QUANTITIES = ('lp_active', 'lp4', 'lp_obstacle', 'fallback', 'full_lists', 'new_collisions', 'done_at_start')
# ... and of a run with lists: what the rule did, counted from the rule's own inputs and outputs
PATH_QUANTITIES = ('served', 'first_takes', 'double_pops', 'later_pops_reached', 'later_pops_behind', 'steps_with_later_pop', 'exhausted',
                   'orca_pops', 'tracked_with_list', 'aimed', 'aimed_zeroed_at_goal', 'at_waypoint', 'non_finite')
# the branches of get_trajectory, per distance measure (l3norm / distance) and per pass (`first`: now_goal was None, `later`): the waypoint is
# within the radius, it is not but lies behind, neither (kept); within or behind with nothing left to pop (a first pass only: a later pass
# with an empty list takes the next branch); the list is empty and now_goal the goal (`first`: it was never given one, `later`: it ran out)
BRANCHES = tuple((m, w, b) for m in ('l3norm', 'distance') for w in ('first', 'later') for b in ('empty', 'near', 'behind', 'keep')) + \
    (('l3norm', 'first', 'nothing_left'), ('distance', 'first', 'nothing_left'))


def path_counts(scene, run):
    """PATH_QUANTITIES and BRANCHES of a run with lists (oracle_run(paths=...)), summed over its steps: rows, but steps_with_later_pop
    (steps of the scene).  orca_pops: passes in which an ORCA3D / ORCA3D-LP agent popped; tracked_with_list: served SCA / RVO3D+Dubins
    rows whose list is not empty when the pass begins."""
    s = scene
    c = dict.fromkeys(PATH_QUANTITIES + BRANCHES, 0)
    orca, tracked = np.isin(s['policy'], R.ORCA), np.isin(s['policy'], R.TRACKED)
    for st in run:
        served = (st['before'] & 7) == 0
        given = np.diff(st['path_off']) > 0
        rem0, rem1, ng0, ng1, pos = st['path_left_before'], st['path_left'], st['now_goal_before'], st['now_goal'], st['pos_before']
        first = served & (rem0 > 0) & np.isnan(ng0[:, 0])
        later = served & (rem0 > 0) & ~np.isnan(ng0[:, 0])
        popped = rem0 - rem1
        # the waypoint the pass tested: the one it took (first pass) or the one it had
        took = np.where(first[:, None], _last(st, rem0), ng0)
        with np.errstate(invalid='ignore'):
            near = R._dist(pos, took, orca) <= s['radius']
            behind = R._dist(took, s['goal'], orca) >= R._dist(pos, s['goal'], orca)
        left = rem0 - first                                                       # what the list held when the test was made
        c['served'] += int(served.sum())
        c['first_takes'] += int(first.sum())
        c['double_pops'] += int((popped == 2).sum())
        c['later_pops_reached'] += int((later & (popped == 1) & near).sum())
        c['later_pops_behind'] += int((later & (popped == 1) & ~near).sum())
        c['steps_with_later_pop'] += int((later & (popped == 1)).any())
        c['exhausted'] += int(((rem0 > 0) & (rem1 == 0)).sum())
        c['orca_pops'] += int((orca & (popped > 0)).sum())
        c['tracked_with_list'] += int((served & tracked & (rem0 > 0)).sum())
        aimed = st['path_mode'].astype(bool)
        c['aimed'] += int(aimed.sum())
        c['aimed_zeroed_at_goal'] += int((aimed & (R._dist(s['goal'], pos, np.zeros(s['n'], bool)) < 0.2)).sum())
        c['at_waypoint'] += int((aimed & (np.linalg.norm(np.nan_to_num(ng1) - pos, axis=1) < 1e-4)).sum())
        c['non_finite'] += int((~np.isfinite(st['vpref_rule'])).any(axis=1).sum())
        for m, sel in (('l3norm', ~orca), ('distance', orca)):
            c[(m, 'first', 'empty')] += int((served & (rem0 == 0) & sel & ~given).sum())
            c[(m, 'later', 'empty')] += int((served & (rem0 == 0) & sel & given).sum())
            for w, rows in (('first', first & sel), ('later', later & sel)):
                c[(m, w, 'near')] += int((rows & near & (left > 0)).sum())
                c[(m, w, 'behind')] += int((rows & ~near & behind & (left > 0)).sum())
                c[(m, w, 'keep')] += int((rows & ~near & ~behind).sum())
            c[(m, 'first', 'nothing_left')] += int((first & sel & (near | behind) & (left == 0)).sum())
    return c


def _last(st, rem0):
    """the last element of every list as the pass found it (NaN where the list was empty)"""
    off, pts = st['path_off'].astype(np.int64), st['path_pts']
    out = np.full((len(rem0), 3), np.nan)
    have = rem0 > 0
    out[have] = pts[off[:-1][have] + rem0[have] - 1]
    return out


def corpus_counts(scene, run):
    """what a scene's oracle run feeds the forms with, summed over the steps of `run` (QUANTITIES; of a run with lists also PATH_QUANTITIES
    and BRANCHES)"""
    c = dict.fromkeys(QUANTITIES, 0)
    if run and 'path_left' in run[0]:
        c.update(path_counts(scene, run))
    c['done_at_start'] = int(((scene['flags'] & 7) != 0).sum())
    for st in run:
        active = (st['before'] & 7) == 0
        lp = active & (scene['policy'] == 4)
        lp4 = lp & (st['diag'][:, 4] == 1)                                      # planeFail < K: linearProgram4
        in_list = np.arange(K)[None, :] < st['nbr_n'][:, None]
        c['lp_active'] += int(lp.sum())
        c['lp4'] += int(lp4.sum())
        c['lp_obstacle'] += int((lp & ((st['nbr_kind'] == 1) & in_list).any(axis=1)).sum())     # isob planes among the LP's
        c['fallback'] += int((st['diag'][:, 1] == 1).sum())
        c['full_lists'] += int(((st['nbr_valid'] != 0) & (st['nbr_n'] == K)).sum())
        c['new_collisions'] += int((((st['flags_policy'] & 2) != 0) & ((st['before'] & 2) == 0)).sum())      # set by the policy pass (agent.py:83-85)
    return c
