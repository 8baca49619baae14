"""Spawn admission (sca_probe_clearance, sca_respawn_agents_gated; include/sca_hip.h) restated in Python, for
tests/test_spawn_probe_cpu.py and tests/test_gpu_spawn_probe.py.  Nothing here calls the library.

probe()  the closest-approach rule of tests/clearance_rule.py (step_minimum: Python's round(math.sqrt(...), 5) per pair, the radius sum
         first, the lowest partner on equal values) for arbitrary spheres against the agents' records and the obstacles.
gate()   the admission rule: the world test of every named row (ignore = its own id), then the entry test against the EARLIER rows of
         the call that are world-clear.
oracle_run_gated()  respawn_rule.oracle_run with the drawn missions filtered through gate() before they are applied: the free-running
         oracle trajectory of a fuzz scene in which a finished row gets a new mission only where its start is free."""
import collections

import numpy as np

import clearance_rule as CR
import form_fuzz as F
import path_rule as R
import respawn_rule as RR

ADMITTED, BLOCKED_AGENT, BLOCKED_OBSTACLE, BLOCKED_ENTRY = 0, 1, 2, 3          # SCA_SPAWN_*
MARGIN = 0.5                                                                   # the gating corpus's margin, metres
PAIR_EVERY = 5                                                                 # every fifth named row of a draw is moved next to the row before it


def probe(qpos, qrad, ignore, pos, radius, obs_pos, obs_radius, ties=None):
    """one record per query (clearance_rule.DTYPE, both step fields 0); ties: a list that receives, per query, how many agent partners share
    the minimum"""
    qpos = np.asarray(qpos, np.float64).reshape(-1, 3)
    out = CR.empty(len(qpos))
    opos = np.asarray(obs_pos, np.float64).reshape(-1, 3)
    for q in range(len(qpos)):
        ig = -1 if ignore is None else int(ignore[q])
        if ig >= 0:
            c, who, t = CR.step_minimum(qpos[q], float(qrad[q]), ig, pos, radius, True)
        else:
            c, who, t = CR.step_minimum(qpos[q], float(qrad[q]), 0, pos, radius, False)
        out['agent_clear'][q], out['agent_partner'][q] = c, who
        c, who, _ = CR.step_minimum(qpos[q], float(qrad[q]), 0, opos, obs_radius, False)
        out['obs_clear'][q], out['obs_partner'][q] = c, who
        if ties is not None:
            ties.append(t)
    return out


def world(rec, margin):
    """the world test's word per record: an empty half (+inf) never blocks"""
    return np.where(rec['agent_clear'] <= margin, BLOCKED_AGENT, np.where(rec['obs_clear'] <= margin, BLOCKED_OBSTACLE, ADMITTED)).astype(np.int32)


def entry_c(pa, ra, pb, rb):
    return CR.l3norm([float(x) for x in pa], [float(x) for x in pb]) - (float(ra) + float(rb))


def gate(ids, qpos, qrad, margin, pos, radius, obs_pos, obs_radius, chains=None):
    """(verdict int32 per named row, the world test's records).  chains: a list that receives every (r', r) where r' < r was blocked by the
    world, lies within the margin of r and so blocks nobody, and r is admitted"""
    qpos = np.asarray(qpos, np.float64).reshape(-1, 3)
    rec = probe(qpos, qrad, ids, pos, radius, obs_pos, obs_radius)
    w = world(rec, margin)
    verdict = w.copy()
    for r in range(len(w)):
        if w[r] != ADMITTED or r == 0:
            continue
        d = np.linalg.norm(qpos[:r] - qpos[r], axis=1) - (np.asarray(qrad[:r], np.float64) + float(qrad[r]))
        near = [k for k in np.flatnonzero(d <= margin + 2e-5) if entry_c(qpos[r], qrad[r], qpos[k], qrad[k]) <= margin]
        if any(w[k] == ADMITTED for k in near):
            verdict[r] = BLOCKED_ENTRY
        elif near and chains is not None:
            chains.extend((int(k), r) for k in near)
    return verdict, rec


def cut(mission, keep):
    """the mission cut down to the rows keep (a boolean mask), None where nobody is left; lists too"""
    if not keep.any():
        return None
    out = {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in mission.items() if k != 'paths'}
    if mission.get('paths') is not None:
        out['paths'] = [p for p, ok in zip(mission['paths'], keep) if ok]
    elif 'paths' in mission:
        out['paths'] = None
    return out


def draw_gated(rng, flags, side):
    """respawn_rule.draw, then every PAIR_EVERY-th named row is moved to within the margin of the row before it (0.2 .. 0.45 m between the
    two spheres): uniform draws in a large box almost never produce an entry block"""
    m = RR.draw(rng, flags, side)
    if m is None:
        return None
    k = len(m['ids'])
    for j in range(PAIR_EVERY - 1, k, PAIR_EVERY):
        u = rng.normal(0, 1, 3)
        u /= np.linalg.norm(u)
        gap = m['radius'][j] + m['radius'][j - 1] + rng.uniform(0.2, 0.45)
        m['pos'][j] = m['pos'][j - 1] + u * gap
        m['pos'][j, 2] = abs(m['pos'][j, 2])
    m['max_run_dist'] = 3.0 * np.linalg.norm(m['pos'] - m['goal'], axis=1) + 1.0
    return m


_RUNS = collections.OrderedDict()
_RUNS_MAX = 24


def oracle_run_gated(oracle, scene, steps=RR.STEPS, margin=MARGIN, list_rule=0, lists=None):
    """respawn_rule.oracle_run with the gate: one dict per step as there, `mission` the ADMITTED rows of what was offered (None where
    nobody was), and beside it `offered` (the whole draw, or None), `verdict`, `probe` (gate()'s, per offered row), `chains`, and
    `pos_at_gate` / `radius_at_gate`, what the rule looked at.  Memoised; the arrays are shared: nobody writes to them."""
    key = scene['key'] + ('gated', steps, margin, list_rule, lists)
    if key in _RUNS:
        _RUNS.move_to_end(key)
        return _RUNS[key]
    s, n = scene, scene['n']
    seed = scene['key'][1]
    rng = np.random.default_rng(RR.RNG_BASE + 500 + seed)
    side = RR.box_of(s)
    zaxis = F.zaxis_of(s)
    st = dict(pos=s['pos'].copy(), vel=s['vel'].copy(), heading=s['heading'].copy(), flags=s['flags'].copy(), total_dist=np.zeros(n),
              step_num=np.zeros(n, np.int32))
    defs = {k: np.array(s[k], np.float64, copy=True) for k in RR.DEF_KEYS}
    perm = np.arange(n, dtype=np.int32)
    if lists:
        paths = [lst[:lists] for lst in F.random_paths(seed, s)]
        missions = 0
        rem, ng = np.array([len(p) for p in paths], np.int32), np.full((n, 3), np.nan)
    out = []
    try:
        oracle.set_list_rule(list_rule)
        for t in range(steps):
            offered = draw_gated(rng, st['flags'], side)
            mission, gated = None, {}
            if offered is not None:
                if lists:
                    missions += 1
                    offered['paths'] = None if missions % 3 == 0 else RR.random_lists(rng, offered, offered['radius'])
                chains = []
                verdict, rec = gate(offered['ids'], offered['pos'], offered['radius'], margin, st['pos'], defs['radius'], s['obs_pos'], s['obs_radius'], chains)
                gated = dict(verdict=verdict, probe=rec, chains=chains, pos_at_gate=st['pos'], radius_at_gate=defs['radius'])
                mission = cut(offered, verdict == ADMITTED)
            if mission is not None:
                st = {k: v.copy() for k, v in st.items()}
                defs = {k: v.copy() for k, v in defs.items()}
                RR.apply(st, defs, mission)
                if lists:
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
            step.update(mission=mission, offered=offered, before=st['flags'], active_before=int(((st['flags'] & RR.DONE) == 0).sum()), flags_policy=r['flags'],
                        defs=defs)
            step.update(gated)
            step.update(path)
            st = {k: u[k] for k in F.STATE_KEYS}
            step.update(st)
            step['finished'] = np.flatnonzero((st['flags'] & RR.DONE) != 0)
            out.append(step)
    finally:
        oracle.set_list_rule(0)
    _RUNS[key] = out
    while len(_RUNS) > _RUNS_MAX:
        _RUNS.popitem(last=False)
    return out


VERDICTS = ('admitted', 'blocked_agent', 'blocked_obstacle', 'blocked_entry')


def corpus_counts(run):
    """what a gated run holds: named rows per verdict, the chain cases, calls that admit nobody and calls that admit only a part"""
    c = dict.fromkeys(VERDICTS + ('chains', 'calls', 'calls_none', 'calls_partly'), 0)
    for st in run:
        if st['offered'] is None:
            continue
        v = st['verdict']
        for k, name in enumerate(VERDICTS):
            c[name] += int((v == k).sum())
        c['chains'] += len(st['chains'])
        c['calls'] += 1
        c['calls_none'] += int(not (v == ADMITTED).any())
        c['calls_partly'] += int((v == ADMITTED).any() and (v != ADMITTED).any())
    return c
