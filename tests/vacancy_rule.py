"""Vacant rows in a plain context, stated with the oracle alone: the free-running oracle trajectory of a fuzz scene (tests/form_fuzz.py) in
which, before every step -- step 0 included -- occupied rows are retired (a finished row often, a live row rarely), vacant rows are admitted
with new missions and finished rows are plainly respawned (respawn_rule.draw's values).  The reference indexes agents[agentIDs[i]] by id and
has no removal in place; vacancy is the plain list edit on kdTree.agentIDs -- retiring id a is agentIDs.remove(a), admitting it
agentIDs.append(a), nothing else of the order moves -- and agent ids enter no value of the reference (only the self-exclusions of agent.py:80
and mampenv.py:69), so every step here COMPACTS the occupied rows in ascending id, runs oracle.policy_step / env_update on them alone with
the occupied prefix of the permutation mapped through the same renumbering, and scatters the results back to the global rows.  A vacant row
reads flags 11, zero velocity, heading, total_dist and step_num, a zero action row, an invalid list, diag -1; it keeps its position.
Shared by tests/test_vacancy_cpu.py (what the corpus holds) and tests/test_gpu_vacancy.py (the kernels against it).  Test infrastructure: it
drives the oracle, the product never imports it."""
import collections

import numpy as np

import form_fuzz as F
import respawn_rule as RR

STEPS = 12
SEEDS = range(40)
RNG_BASE = 20_000
VACANT = 11                                    # at-goal | collision | the vacant bit
DONE = 7
P_RETIRE_FINISHED = 0.35                       # a finished occupied row is retired
P_RETIRE_LIVE = (0.02, 0.05, 0.15)             # a live row is retired: one of these per seed
P_OFFER = (1.0, 1.0, 0.25)                     # a vacant row is offered to the step's mission: with the third pair the population falls below n / 2
# (respawn_rule.draw takes each row it is offered with probability 0.5: a vacant row is admitted, a finished row plainly respawned)


def retire(st, perm, vacant, ids):
    """the rule of a retire, in place on copies the caller owns: the rows' words, and the list edit; returns the new permutation"""
    vacant[ids] = True
    st['vel'][ids] = 0
    st['heading'][ids] = 0
    st['flags'][ids] = VACANT
    st['total_dist'][ids] = 0
    st['step_num'][ids] = 0
    m_old = len(perm) - (int(vacant.sum()) - len(ids))
    prefix = [int(a) for a in perm[:m_old]]
    for a in ids:
        prefix.remove(int(a))
    return np.array(prefix + [int(a) for a in np.flatnonzero(vacant)], np.int32)


def admit(perm, vacant, ids):
    """the list edit of a respawn that names `ids` (call order): the vacant ones among them are appended to the occupied prefix"""
    m_old = len(perm) - int(vacant.sum())
    prefix = [int(a) for a in perm[:m_old]]
    for a in ids:
        if vacant[a]:
            prefix.append(int(a))
            vacant[a] = False
    return np.array(prefix + [int(a) for a in np.flatnonzero(vacant)], np.int32)


def draw(rng, st, vacant, p_live, p_offer, side):
    """what happens before a step: (the ids to retire, ascending, or None; the mission, or None).  The last occupied row is never retired;
    the mission is offered the rows that were vacant before this step's retire and the finished occupied rows it leaves."""
    n = len(vacant)
    occ = ~vacant
    fin = occ & ((st['flags'] & DONE) != 0)
    u = rng.random(n)
    take = (fin & (u < P_RETIRE_FINISHED)) | (occ & ~fin & (u < p_live))
    if take.sum() >= occ.sum():
        take[np.flatnonzero(take)[-1]] = False
    ids = np.flatnonzero(take).astype(np.int32)
    offered = ((vacant & (rng.random(n) < p_offer)) | (fin & ~take)).astype(np.uint8)
    mission = RR.draw(rng, offered, side)
    return (ids if len(ids) else None), mission


def compact_step(oracle, scene, zaxis, st, defs, perm, vacant):
    """one step of the occupied rows alone; returns (the pass's record in global rows, the state after the step, the new permutation)"""
    s, n = scene, scene['n']
    occ = np.flatnonzero(~vacant).astype(np.int32)
    m = len(occ)
    g2c = np.full(n, -1, np.int32)
    g2c[occ] = np.arange(m, dtype=np.int32)
    perm_c = g2c[perm[:m]]
    assert (perm_c >= 0).all() and len(set(perm_c.tolist())) == m, 'the prefix holds the occupied ids'
    r = oracle.policy_step(st['pos'][occ], st['vel'][occ], st['heading'][occ], defs['radius'][occ], defs['pref_speed'][occ], st['flags'][occ],
                           defs['goal'][occ], s['policy'][occ], zaxis[occ], s['vpref'][occ], s['vmode'][occ], perm_c, s['obs_pos'], s['obs_radius'], nthreads=8)
    u = oracle.env_update(st['pos'][occ], st['vel'][occ], st['heading'][occ], defs['radius'][occ], r['flags'], defs['goal'][occ], r['action'],
                          st['total_dist'][occ], defs['max_run_dist'][occ], st['step_num'][occ], s['obs_pos'], s['obs_radius'])
    step = {}
    for k, fill in (('action', 0), ('nbr_valid', 0), ('nbr_n', 0), ('nbr_id', -1), ('nbr_kind', 0), ('nbr_dsq', 0), ('diag', -1), ('status', 0), ('vpref', np.nan)):
        full = np.full((n,) + r[k].shape[1:], fill, r[k].dtype)
        full[occ] = r[k]
        step[k] = full
    ids = step['nbr_id']
    agent = (step['nbr_kind'] == 0) & (ids >= 0)
    step['nbr_id'] = np.where(agent, occ[np.where(agent, ids, 0)], ids).astype(ids.dtype)
    step['flags_policy'] = st['flags'].copy()
    step['flags_policy'][occ] = r['flags']
    new = {k: st[k].copy() for k in F.STATE_KEYS}
    for k in F.STATE_KEYS:
        new[k][occ] = u[k]
    perm = np.concatenate([occ[r['perm']], np.flatnonzero(vacant)]).astype(np.int32)
    step['perm'] = perm
    return step, new, perm


_RUNS = collections.OrderedDict()
_RUNS_MAX = 24


def oracle_run(oracle, scene, steps=STEPS):
    """The trajectory with retires and admissions.  One dict per step: `retire` (ids retired before the step, or None), `mission` (what was
    respawned behind that, vacant rows admitted among it, or None), `vacant_call` / `perm_call` / `state_call` (the vacancy mask, the
    permutation and the state behind the calls, in front of the step), `active_before`, `defs`, everything compact_step records in global
    rows (action, lists, diag, status, perm, flags_policy), `before`, the state after the step, `vacant` (the mask during the step),
    `finished` (np.flatnonzero of the done flags of the occupied rows after the step).  Memoised; the arrays are shared: nobody writes to
    them."""
    key = scene['key'] + (steps,)
    if key in _RUNS:
        _RUNS.move_to_end(key)
        return _RUNS[key]
    s, n = scene, scene['n']
    seed = scene['key'][1]
    rng = np.random.default_rng(RNG_BASE + seed)
    p_live, p_offer = P_RETIRE_LIVE[seed % len(P_RETIRE_LIVE)], P_OFFER[seed % len(P_OFFER)]
    side = RR.box_of(s)
    zaxis = F.zaxis_of(s)
    st = dict(pos=s['pos'].copy(), vel=s['vel'].copy(), heading=s['heading'].copy(), flags=s['flags'].copy(), total_dist=np.zeros(n),
              step_num=np.zeros(n, np.int32))
    defs = {k: np.array(s[k], np.float64, copy=True) for k in RR.DEF_KEYS}
    perm = np.arange(n, dtype=np.int32)
    vacant = np.zeros(n, bool)
    out = []
    for _ in range(steps):
        ids, mission = draw(rng, st, vacant, p_live, p_offer, side)
        st = {k: v.copy() for k, v in st.items()}
        defs = {k: v.copy() for k, v in defs.items()}
        vacant = vacant.copy()
        if ids is not None:
            perm = retire(st, perm, vacant, ids)
        if mission is not None:
            perm = admit(perm, vacant, mission['ids'])
            RR.apply(st, defs, mission)
        step, new, perm_after = compact_step(oracle, s, zaxis, st, defs, perm, vacant)
        step.update(retire=ids, mission=mission, vacant=vacant, vacant_call=vacant, perm_call=perm, state_call=st, before=st['flags'], defs=defs,
                    active_before=int((~vacant & ((st['flags'] & DONE) == 0)).sum()))
        st, perm = new, perm_after
        step.update(st)
        step['finished'] = np.flatnonzero(~vacant & ((st['flags'] & DONE) != 0))
        out.append(step)
    _RUNS[key] = out
    while len(_RUNS) > _RUNS_MAX:
        _RUNS.popitem(last=False)
    return out


QUANTITIES = ('retired_finished', 'retired_live', 'admissions', 'respawns', 'repeats', 'list_entries', 'retired_tracked', 'retired_lp', 'steps_below_half',
              'single_leaf', 'admitted_collisions', 'mixed_calls')


def corpus_counts(scene, run):
    """What a run feeds the feature with, counted from the rule and the oracle's records alone: finished and live rows retired, vacant rows
    admitted and occupied rows plainly respawned, rows retired or admitted that had been before (repeats), neighbour-list entries that named
    a row in the step before it was retired, tracked (SCA / RVO3D+Dubins) and ORCA3D-LP rows retired, steps with m below n / 2, whether the
    scene reaches m <= 10 (one leaf), collisions gained by a row after an admission, and respawn calls that mix occupied and vacant rows."""
    n = scene['n']
    c = dict.fromkeys(QUANTITIES, 0)
    retired_ever, admitted_ever = np.zeros(n, bool), np.zeros(n, bool)
    prev, vac_before = None, np.zeros(n, bool)
    least = n
    for st in run:
        ids = st['retire']
        if ids is not None:
            flags_in = prev['flags'] if prev is not None else scene['flags']
            c['retired_finished'] += int(((flags_in[ids] & DONE) != 0).sum())
            c['retired_live'] += int(((flags_in[ids] & DONE) == 0).sum())
            c['repeats'] += int(retired_ever[ids].sum())
            c['retired_tracked'] += int(np.isin(scene['policy'][ids], (0, 5)).sum())
            c['retired_lp'] += int((scene['policy'][ids] == 4).sum())
            retired_ever[ids] = True
            if prev is not None:
                in_list = (np.arange(F.K)[None, :] < prev['nbr_n'][:, None]) & (prev['nbr_valid'][:, None] != 0) & (prev['nbr_kind'] == 0)
                c['list_entries'] += int((in_list & np.isin(prev['nbr_id'], ids)).sum())
        m = st['mission']
        if m is not None:
            was = vac_before.copy()
            if ids is not None:
                was[ids] = False                                           # (the mission is offered the rows vacant BEFORE this step's retire)
            adm = was[m['ids']]
            c['admissions'] += int(adm.sum())
            c['respawns'] += int((~adm).sum())
            c['repeats'] += int(admitted_ever[m['ids'][adm]].sum())
            c['mixed_calls'] += int(adm.any() and (~adm).any())
            admitted_ever[m['ids'][adm]] = True
        gained = st['flags'] & ~st['before']
        c['admitted_collisions'] += int((admitted_ever & ~st['vacant'] & ((gained & 2) != 0)).sum())
        occupied = int((~st['vacant']).sum())
        c['steps_below_half'] += int(2 * occupied < n)
        least = min(least, occupied)
        prev, vac_before = st, st['vacant']
    c['single_leaf'] = int(least <= 10)
    return c
