"""The degenerate-geometry family (tests/golden/F20_edge_*.npz, tools/gen_golden.py::edge_scenes) as scenes for the oracle and the device,
shared by tests/test_edge_corpus_cpu.py (what the family holds, counted from the recordings and the oracle alone; the oracle free-running
against the recordings) and tests/test_gpu_edge_corpus.py (every kernel form, AUTO, the grid, bursts and the host step against the oracle).

A scene here has form_fuzz.random_scene's keys and starts from a RECORDED state: step t of a fixture, with the kd permutation and the
travelled distance the reference's step started from and the v_pref its tracker fed (the SCA / RVO3D+Dubins rows).  Test infrastructure:
it drives the oracle, the product never imports it."""
import numpy as np

import form_fuzz as F
from golden_util import edge_fixtures, load, static_inputs

K = F.K
_FX, _STEPS = {}, {}


def fixture(name):
    if name not in _FX:
        _FX[name] = load(name)
    return _FX[name]


def steps_of(name):
    return len(fixture(name)['step'])


def differ(got, want):
    """Elementwise `got != want` under the family's one relaxation (golden_util.equal_for): NaN equals NaN at the same place and
    nothing else.  -0.0 and +0.0 compare equal here as they do under np.array_equal everywhere in the suite."""
    got, want = np.asarray(got), np.asarray(want)
    d = got != want
    if got.dtype.kind == 'f' and want.dtype.kind == 'f':
        d &= ~(np.isnan(got) & np.isnan(want))
    return d


def same(got, want):
    return not differ(got, want).any()


def step_scene(name, t=0):
    """step t of a fixture as a scene: the recorded state the reference's step started from"""
    fx = fixture(name)
    st = static_inputs(fx)
    n = len(st['radius'])
    return dict(n=n, m=len(st['obs_radius']), pos=fx['pos'][t], goal=fx['goal'][t], heading=fx['heading'][t], vel=fx['vel'][t],
                radius=st['radius'], pref_speed=st['pref_speed'], policy=st['policy'], flags=fx['flags'][t], obs_pos=st['obs_pos'],
                obs_radius=st['obs_radius'], vpref=np.nan_to_num(fx['vpref'][t]), vmode=st['vpref_mode'], max_run_dist=st['max_run_dist'],
                zaxis=st['zaxis'], perm=fx['perm'][t], total_dist=fx['total_dist'][t], key=('edge', name, t))


def concat(scenes, shifts):
    """several scenes as one: agents and obstacles one after the other, scene j moved by shifts[j] (positions, goals, obstacles); the kd
    permutation starts as the identity (the scenes' own permutations do not compose).  Returns (scene, agent offsets, obstacle offsets)."""
    off = np.concatenate([[0], np.cumsum([s['n'] for s in scenes])])
    ooff = np.concatenate([[0], np.cumsum([s['m'] for s in scenes])])
    out = dict(n=int(off[-1]), m=int(ooff[-1]), key=('concat',) + tuple(s['key'] for s in scenes))
    for k in ('pos', 'goal', 'obs_pos'):
        out[k] = np.concatenate([s[k].reshape(-1, 3) + np.asarray(sh, np.float64) for s, sh in zip(scenes, shifts)])
    for k in ('heading', 'vel', 'radius', 'pref_speed', 'policy', 'flags', 'obs_radius', 'vpref', 'vmode', 'max_run_dist', 'zaxis', 'total_dist'):
        out[k] = np.concatenate([s[k] for s in scenes])
    out['perm'] = np.arange(out['n'], dtype=np.int32)
    return out, off, ooff


def concat_shift(scene, j):
    """where scene j of a concatenation goes: 4096 * (j + 1) m along an axis on which that sum is exact for every coordinate of the scene (y for
    the geometries in an x-z plane and the lattices, z for the rings), so that the move changes no difference of two coordinates"""
    pts = np.concatenate([scene['pos'], scene['goal'], scene['obs_pos'].reshape(-1, 3)])
    for axis in (1, 2):
        sh = np.zeros(3)
        sh[axis] = 4096.0 * (j + 1)
        if ((pts[:, axis] + sh[axis]) - sh[axis] == pts[:, axis]).all():        # (exact: integers and short binary fractions)
            return sh
    return None


def concat_groups(limit=600):
    """the family's fixtures in name order, cut into groups of at most `limit` agents: one context each"""
    groups, size = [[]], 0
    for name in edge_fixtures():
        n = len(fixture(name)['radius'])
        if size + n > limit:
            groups.append([])
            size = 0
        groups[-1].append(name)
        size += n
    return groups


def oracle_step(oracle, scene, list_rule=0):
    """One step of the oracle from the scene's state: policy_step then env_update, the record form_fuzz.oracle_run makes per step (action,
    lists, diag, perm, status, the v_pref used, `before`, `flags_policy`, the state after).  Memoised per scene and rule; nobody writes
    to the arrays."""
    key = scene['key'] + (list_rule,)
    if key in _STEPS:
        return _STEPS[key]
    s, n = scene, scene['n']
    try:
        oracle.set_list_rule(list_rule)
        r = oracle.policy_step(s['pos'], s['vel'], s['heading'], s['radius'], s['pref_speed'], s['flags'], s['goal'], s['policy'], s['zaxis'],
                               s['vpref'], s['vmode'], s['perm'], s['obs_pos'], s['obs_radius'], nthreads=4)
    finally:
        oracle.set_list_rule(0)
    u = oracle.env_update(s['pos'], s['vel'], s['heading'], s['radius'], r['flags'], s['goal'], r['action'], s['total_dist'], s['max_run_dist'],
                          np.zeros(n, np.int32), s['obs_pos'], s['obs_radius'])
    step = {k: r[k] for k in ('action', 'nbr_valid', 'nbr_n', 'nbr_id', 'nbr_kind', 'nbr_dsq', 'diag', 'perm', 'status', 'vpref')}
    step['before'], step['flags_policy'] = s['flags'], r['flags']
    step.update({k: u[k] for k in F.STATE_KEYS})
    if len(_STEPS) > 400:
        _STEPS.clear()
    _STEPS[key] = step
    return step


# ---- what the family holds -------------------------------------------------------------------------------------------------------------
QUANTITIES = ('pair_ties', 'triple_ties', 'ties_at_the_cut', 'dist_eq_R', 'dist_lt_R', 'relpos_zero', 'dist_eq_range', 'collisions_at_equality', 'fallback',
              'lp4', 'lp1_parallel', 'sqrt_domain', 'far_agents', 'nan_action_rows')


def _rounded_dsq(p, q):
    d = q - p
    s = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    s = s + d[:, 2] * d[:, 2]
    return np.rint(s * 1e5) / 1e5                                              # util.py:100 l3normsq


def census(name, oracle, lp_parallel=None):
    """QUANTITIES of one fixture, from its recorded rows (lists, decisions, states) and the oracle's status words; lp_parallel(fx, t, i):
    the lp1 calls of agent i's linearProgram3 that took the parallel branch (tests/core_harness.cpp), None: not counted."""
    fx = fixture(name)
    st = static_inputs(fx)
    c = dict.fromkeys(QUANTITIES, 0)
    rad, orad, n = st['radius'], st['obs_radius'], len(st['radius'])
    for t in range(len(fx['step'])):
        pos, pos_after = fx['pos'][t], fx['pos_after'][t]
        served = (fx['flags'][t] & 7) == 0
        for i in np.flatnonzero(fx['nbr_valid'][t]):
            k = int(fx['nbr_n'][t][i])
            dsq = fx['nbr_dsq'][t][i][:k]
            c['pair_ties'] += int(k >= 2 and np.unique(dsq, return_counts=True)[1].max() == 2)
            c['triple_ties'] += int(k >= 3 and np.unique(dsq, return_counts=True)[1].max() >= 3)
            ids, kinds = fx['nbr_id'][t][i][:k], fx['nbr_kind'][t][i][:k]
            for j, kind in zip(ids, kinds):
                pB, rB = (st['obs_pos'][j], orad[j]) if kind else (pos[j], rad[j])
                d = pB - pos[i]
                R = (rB + 0.05) + (rad[i] + 0.05)
                dist = float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
                c['dist_eq_R'] += int(dist == R)
                c['dist_lt_R'] += int(dist < R)
                c['relpos_zero'] += int(not d.any())
            c['dist_eq_range'] += int((_rounded_dsq(pos[i][None, :], pos) == 100.0).sum())        # distSq == rangeSq: `<` keeps it out
            # the 16th and 17th candidate: everybody in range by the rounded distance, the agent not colliding (a collision clears the list)
            if k == K and not fx['coll_after_policy'][t][i]:
                d2 = _rounded_dsq(pos[i][None, :], pos)
                d2[i] = np.inf
                d2 = np.sort(d2[d2 < 100.0])
                c['ties_at_the_cut'] += int(len(d2) > K and d2[K - 1] == d2[K])
        # new collisions of the env's own test (mampenv.py:61-76), at exactly dis == radius sum
        new = ((fx['flags_after'][t] & 2) != 0) & (fx['coll_after_policy'][t] == 0) & ((fx['flags'][t] & 2) == 0)
        for i in np.flatnonzero(new):
            d = np.sqrt(((pos_after - pos_after[i]) ** 2).sum(axis=1))
            dis = np.array([round(float(x), 5) for x in d])
            at = (dis == rad + rad[i])
            at[i] = False
            do = np.array([round(float(np.sqrt(((o - pos_after[i]) ** 2).sum())), 5) for o in st['obs_pos']]).reshape(-1)
            c['collisions_at_equality'] += int(at.any() or (do == orad + rad[i]).any())
        c['fallback'] += int((fx['fallback'][t] == 1).sum())
        c['lp4'] += int((fx['lp4'][t] == 1).sum())
        c['far_agents'] += int((np.abs(pos).max(axis=1) > 1.0e6).sum()) if t == 0 else 0
        c['nan_action_rows'] += int(np.isnan(fx['action'][t]).any(axis=1).sum())
        c['sqrt_domain'] += int(((oracle_step(oracle, step_scene(name, t))['status'] & 2) != 0).sum())
        if lp_parallel is not None:
            for i in np.flatnonzero(served & (st['policy'] == 4) & (fx['plane_fail'][t] >= 0)):       # (the rows whose linearProgram3 ran)
                c['lp1_parallel'] += lp_parallel(fx, st, t, int(i))
    return c
