"""A respawn that brings the arriving agent's own policy and solver attributes, stated with the oracle alone (sca_respawn_agents_attrs).

tests/respawn_rule.py's corpus -- the fuzz scenes of tests/form_fuzz.py stepped free-running, before every step each finished row gets a
new mission with probability 0.5 -- where every scene starts from the context's DEFAULT parameters with no per-agent arrays and every
call also brings
  a policy 0 .. 5 per named row, and
  with probability 0.5 a full attribute row per named row (form_fuzz.per_agent_attributes' value sets),
  with probability 0.25 a descriptor in which some arrays are missing: those names fall back to the CONTEXT's value for every named row,
  with probability 0.25 no descriptor: the rows keep their attributes.
The reference keeps policy and attributes as plain fields of the Agent object (agent.py:24-41), so the rule is assignment: the named rows
of the policy array and of the attribute table are overwritten, the oracle is stepped with set_agent_params and the policy array as they
stand before each step.  v_pref / its mode are fed as form_fuzz.random_scene defines them, for the CURRENT policies (mode 1 on SCA and
RVO3D+Dubins rows, the scene's `vpref` values), as a caller without a device tracker would feed them behind every call.
The module also models the context's envelope: a running maximum per attribute, which never shrinks -- and the planner attributes a call
brings under a device tracker (turning radius, pitch limits): with a descriptor, half the calls bring a triple per named row from a wide
palette (24 triples) or a narrow one (2), from a stream of their own; the model keeps the per-row triples by the library's rule (from the
first such call on a descriptor without planner arrays brings the tracker's own values) and counts the classes among the tracked rows.
The corpus runs without a tracker, so these draws reach the class-table rule (tests/test_respawn_attrs_cpu.py) and not the GPU corpus;
tests/test_gpu_respawn_attrs.py's tracker test passes planner attributes on the GPU.
Test infrastructure: it drives the oracle, the product never imports it."""
import collections
import math

import numpy as np

import form_fuzz as F
import respawn_rule as RR

ATTR_NAMES = ('neighbor_dist', 'max_neighbors', 'time_step', 'time_horizon', 'max_speed', 'max_heading_change', 'dt_nominal')
# form_fuzz.per_agent_attributes' value sets, and a dt_nominal above the context's 0.1: without it the envelope's dt_nominal never grows
ATTR_VALUES = dict(neighbor_dist=[1.5, 2.5, 4.0, 10.0, 15.0, 30.0], max_neighbors=[1, 2, 4, 8, 12, 16], time_step=[0.05, 0.1, 0.2],
                   time_horizon=[1.0, 3.0, 10.0, 20.0], max_speed=[0.7, 1.0, 1.5, 3.0],
                   max_heading_change=[0.3, math.pi / 6, math.pi / 4, 1.2, math.pi / 2], dt_nominal=[0.05, 0.1, 0.2])
# sca_default_params / oracle.DEFAULT_PARAMS: what a missing name of a descriptor stands for
CONTEXT = dict(neighbor_dist=10.0, max_neighbors=16, time_step=0.1, time_horizon=10.0, max_speed=1.0, max_heading_change=math.pi / 4, dt_nominal=0.1)
ENVELOPE = ('neighbor_dist', 'max_speed', 'dt_nominal')
RNG_BASE = 20_000
PLANNER_RNG_BASE = 30_000
TRACKER = (1.5, -math.pi / 4, math.pi / 4)                         # sca_device_tracker_enable's defaults: what a missing planner array stands for
PITCH = ((-math.pi / 4, math.pi / 4), (-0.5, 0.6), (-0.3, 0.3))
WIDE = [(R, lo, hi) for R in (1.0, 1.25, 1.5, 1.75, 2.0, 2.5, 3.0, 4.0) for lo, hi in PITCH]
NARROW = [(1.5, -math.pi / 4, math.pi / 4), (2.0, -0.5, 0.6)]
CLASS_CAP = 16
TRACKED = (0, 5)
LP = 4


def dtype_of(name):
    return np.int32 if name == 'max_neighbors' else np.float64


def context_table(n):
    """every row holds the context's values: what a context without per-agent arrays computes from"""
    return {k: np.full(n, CONTEXT[k], dtype_of(k)) for k in ATTR_NAMES}


def draw_brings(rng, k):
    """what a call that names k rows brings: (policy [k], attrs): attrs None (the rows keep theirs) or a dict name -> [k]; a name that is
    missing stands for the context's value"""
    policy = rng.integers(0, 6, k).astype(np.uint8)
    kind = rng.random()
    if kind < 0.25:
        return policy, None
    names = list(ATTR_NAMES)
    if kind < 0.5:
        names = [nm for nm in ATTR_NAMES if rng.random() < 0.5]
    return policy, {nm: rng.choice(ATTR_VALUES[nm], k).astype(dtype_of(nm)) for nm in names}


def apply_brings(policy, table, ids, new_policy, attrs):
    """the named rows of the policy array and of the attribute table become the call's, in place"""
    if new_policy is not None:
        policy[ids] = new_policy
    if attrs is not None:
        for nm in ATTR_NAMES:
            table[nm][ids] = attrs[nm] if nm in attrs else CONTEXT[nm]


def draw_planner(rng, k, attrs):
    """the planner triples a call brings, [k, 3], or None; only a call with a descriptor can bring any"""
    kind, wide = rng.random(), rng.random() < 0.5
    if attrs is None or kind < 0.5:
        return None
    palette = WIDE if wide else NARROW
    return np.array([palette[i] for i in rng.integers(0, len(palette), k)], np.float64)


def apply_planner(trip, per_row, ids, attrs, planner):
    """the named rows of the [n, 3] triples become the call's, in place, by the library's rule; returns whether per-row triples are in
    force behind the call"""
    if attrs is not None and (planner is not None or per_row):
        trip[ids] = TRACKER if planner is None else planner
        return True
    return per_row


def classes_of(policy, trip):
    """distinct triples among the rows whose policy is tracked"""
    t = np.isin(policy, TRACKED)
    return len({tuple(x) for x in trip[t]})


def vmode_of(policy):
    return np.isin(policy, TRACKED).astype(np.uint8)


def grow(envelope, attrs):
    """the envelope behind a call: a running maximum over what the calls brought (a missing name brings the context's value, which the
    envelope started from)"""
    out = dict(envelope)
    for nm in ENVELOPE:
        if attrs is not None and nm in attrs:
            out[nm] = max(out[nm], float(np.max(attrs[nm])))
    return out


_RUNS = collections.OrderedDict()
_RUNS_MAX = 24


def oracle_run(oracle, scene, steps=RR.STEPS, list_rule=0):
    """The trajectory with respawns that bring policies and attributes.  One dict per step: everything respawn_rule.oracle_run records, the
    mission with `policy` and `attrs` (draw_brings), `policy_before` / `table_before` (what the rows held in front of the call), `policy` /
    `table` (what the step ran with), `vmode`, `envelope` (behind the call) and `list_len_before` (nbr_n of the last pass where the list was
    valid).  Memoised; the arrays are shared: nobody writes to them."""
    key = scene['key'] + (steps, list_rule)
    if key in _RUNS:
        _RUNS.move_to_end(key)
        return _RUNS[key]
    s, n = scene, scene['n']
    seed = scene['key'][1]
    rng = np.random.default_rng(RR.RNG_BASE + seed)
    rng2 = np.random.default_rng(RNG_BASE + seed)                          # (a stream of its own: the missions are respawn_rule's)
    rng3 = np.random.default_rng(PLANNER_RNG_BASE + seed)
    trip, per_row = np.tile(np.array(TRACKER), (n, 1)), False
    side = RR.box_of(s)
    zaxis = F.zaxis_of(s)
    st = dict(pos=s['pos'].copy(), vel=s['vel'].copy(), heading=s['heading'].copy(), flags=s['flags'].copy(), total_dist=np.zeros(n),
              step_num=np.zeros(n, np.int32))
    defs = {k: np.array(s[k], np.float64, copy=True) for k in RR.DEF_KEYS}
    policy, table = s['policy'].copy(), context_table(n)
    envelope = {k: CONTEXT[k] for k in ENVELOPE}
    perm = np.arange(n, dtype=np.int32)
    list_len = np.zeros(n, np.int32)
    out = []
    try:
        oracle.set_list_rule(list_rule)
        oracle.set_params()
        for t in range(steps):
            mission = RR.draw(rng, st['flags'], side)
            policy_before, table_before, trip_before = policy, table, trip
            if mission is not None:
                st = {k: v.copy() for k, v in st.items()}
                defs = {k: v.copy() for k, v in defs.items()}
                RR.apply(st, defs, mission)
                mission['policy'], mission['attrs'] = draw_brings(rng2, len(mission['ids']))
                policy, table = policy.copy(), {k: v.copy() for k, v in table.items()}
                apply_brings(policy, table, mission['ids'], mission['policy'], mission['attrs'])
                envelope = grow(envelope, mission['attrs'])
                mission['planner'] = draw_planner(rng3, len(mission['ids']), mission['attrs'])
                trip = trip.copy()
                per_row = apply_planner(trip, per_row, mission['ids'], mission['attrs'], mission['planner'])
            vmode = vmode_of(policy)
            oracle.set_agent_params(n, **table)
            r = oracle.policy_step(st['pos'], st['vel'], st['heading'], defs['radius'], defs['pref_speed'], st['flags'], defs['goal'], policy,
                                   zaxis, s['vpref'], vmode, perm, s['obs_pos'], s['obs_radius'], nthreads=8)
            perm = r['perm']
            u = oracle.env_update(st['pos'], st['vel'], st['heading'], defs['radius'], r['flags'], defs['goal'], r['action'], st['total_dist'],
                                  defs['max_run_dist'], st['step_num'], s['obs_pos'], s['obs_radius'])
            step = {k: r[k] for k in ('action', 'nbr_valid', 'nbr_n', 'nbr_id', 'nbr_kind', 'nbr_dsq', 'diag', 'perm', 'status', 'vpref')}
            step.update(mission=mission, before=st['flags'], active_before=int(((st['flags'] & RR.DONE) == 0).sum()), flags_policy=r['flags'], defs=defs,
                        policy=policy, table=table, policy_before=policy_before, table_before=table_before, vmode=vmode, envelope=dict(envelope),
                        list_len_before=list_len, trip=trip, trip_before=trip_before, per_row=per_row)
            list_len = np.where(r['nbr_valid'] != 0, r['nbr_n'], list_len).astype(np.int32)
            st = {k: u[k] for k in F.STATE_KEYS}
            step.update(st)
            step['finished'] = np.flatnonzero((st['flags'] & RR.DONE) != 0)
            out.append(step)
    finally:
        oracle.set_params()
        oracle.set_agent_params()
        oracle.set_list_rule(0)
    _RUNS[key] = out
    while len(_RUNS) > _RUNS_MAX:
        _RUNS.popitem(last=False)
    return out


def scene_of(scene, step):
    """the scene with the step's policies, for the comparisons that read scene['policy']"""
    return dict(scene, policy=step['policy'], vmode=step['vmode'])


QUANTITIES = ('respawns', 'policy_changes', 'lp_enter', 'lp_leave', 'tracked_enter', 'tracked_leave', 'max_neighbors_below_list', 'full_rows',
              'partial_descriptors', 'no_descriptor', 'grow_neighbor_dist', 'grow_max_speed', 'grow_dt_nominal', 'planner_calls', 'classes_pass_16',
              'classes_come_back')


def corpus_counts(scene, run):
    """What a run feeds the call with, counted from the rule alone: (counts, pairs) -- QUANTITIES and the 6 x 6 table of ordered (old,
    new) policy pairs over the respawned rows."""
    c = dict.fromkeys(QUANTITIES, 0)
    pairs = np.zeros((6, 6), np.int64)
    envelope = {k: CONTEXT[k] for k in ENVELOPE}
    for st in run:
        m = st['mission']
        if m is None:
            continue
        ids = m['ids']
        old, new = st['policy_before'][ids], m['policy']
        np.add.at(pairs, (old, new), 1)
        c['respawns'] += len(ids)
        c['policy_changes'] += int((old != new).sum())
        c['lp_enter'] += int(((old != LP) & (new == LP)).sum())
        c['lp_leave'] += int(((old == LP) & (new != LP)).sum())
        c['tracked_enter'] += int((~np.isin(old, TRACKED) & np.isin(new, TRACKED)).sum())
        c['tracked_leave'] += int((np.isin(old, TRACKED) & ~np.isin(new, TRACKED)).sum())
        c['max_neighbors_below_list'] += int((st['table']['max_neighbors'][ids] < st['list_len_before'][ids]).sum())
        a = m['attrs']
        if a is None:
            c['no_descriptor'] += 1
        elif len(a) == len(ATTR_NAMES):
            c['full_rows'] += 1
        else:
            c['partial_descriptors'] += 1
        for nm in ENVELOPE:
            c['grow_' + nm] += int(st['envelope'][nm] > envelope[nm])
        c['planner_calls'] += int(m['planner'] is not None)
        was, now = classes_of(st['policy_before'], st['trip_before']), classes_of(st['policy'], st['trip'])
        c['classes_pass_16'] += int(was <= CLASS_CAP < now)
        c['classes_come_back'] += int(now <= CLASS_CAP < was)
        envelope = st['envelope']
    return c, pairs


def grid_fits(scene, run):
    """the grid's condition for every step: max_radius + reach <= the envelope's neighbor_dist for the agents' reach (the largest radius
    + two largest steps + 1e-4) and the obstacles' (the largest obstacle radius + one largest step + 1e-4); the largest radius and
    pref_speed are running maxima too, the largest step 1.01 x max(pref_speed, max_speed) x dt_nominal over the envelope"""
    max_radius, max_pref = float(scene['radius'].max()), float(scene['pref_speed'].max())
    obs = float(scene['obs_radius'].max()) if scene['m'] else 0.0
    for st in run:
        m = st['mission']
        if m is not None:
            max_radius, max_pref = max(max_radius, float(m['radius'].max())), max(max_pref, float(m['pref_speed'].max()))
        e = st['envelope']
        step = 1.01 * max(max_pref, e['max_speed']) * e['dt_nominal']
        if max_radius + max(max_radius + 2.0 * step, obs + step) + 1e-4 > e['neighbor_dist']:
            return False
    return True
