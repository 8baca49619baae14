"""Mission tables, stated with the oracle alone: the free-running oracle trajectory of a fuzz scene (tests/form_fuzz.py) in which every row
carries a drawn table of M = 3 missions and, BEHIND every step, each row that ended in the step (it entered without a done flag and left
with one) takes the successor its ended flight names -- exactly tests/respawn_rule.py's `apply` for that row with the entry's values, the
position and heading kept where the entry says START_HERE, the zaxis byte kept where it says KEEP_ZAXIS.  Rows with first_ok = first_fail =
-1 have no table.  Shared by tests/test_missions_cpu.py (what the corpus holds, the host-compiled row write) and
tests/test_gpu_missions.py (every kernel form against it).  Test infrastructure: it drives the oracle, the product never imports it."""
import collections

import numpy as np

import form_fuzz as F
import respawn_rule as RR

M = 3
STEPS = RR.STEPS
SEEDS = RR.SEEDS
RNG_BASE = 20_000
START_HERE, KEEP_ZAXIS = 1, 2
ARRIVED, COLLIDED, TIMED_OUT = 0, 1, 2
# sca_mission / sca_mission_result as numpy sees them (tests/test_missions_cpu.py holds them against the header's and _lib's)
CLEAR = np.dtype([('agent_clear', np.float64), ('obs_clear', np.float64), ('agent_partner', np.int32), ('agent_step', np.int32),
                  ('obs_partner', np.int32), ('obs_step', np.int32)])
MISSION = np.dtype([('pos', np.float64, (3,)), ('heading', np.float64, (3,)), ('goal', np.float64, (3,)), ('goal_heading', np.float64, (3,)),
                    ('pref_speed', np.float64), ('max_run_dist', np.float64), ('vel', np.float32, (3,)), ('next_ok', np.int8), ('next_fail', np.int8),
                    ('zaxis', np.uint8), ('flags', np.uint8)])
RESULT = np.dtype([('id', np.int32), ('entry', np.int32), ('flags', np.uint32), ('step_num', np.int32), ('total_dist', np.float64),
                   ('pos', np.float64, (3,)), ('update', np.int64), ('next', np.int32), ('reserved', np.int32), ('clear', CLEAR)])
TOTALS = ('updates', 'agent_steps', 'arrived', 'collided', 'timed_out', 'taken', 'stopped')


def empty_clear(k):
    c = np.zeros(k, CLEAR)
    c['agent_clear'] = c['obs_clear'] = np.inf
    c['agent_partner'] = c['obs_partner'] = -1
    return c


def draw_tables(seed, scene, m=M):
    """A table of m entries for every row: (entries (n, m) of MISSION, first_ok, first_fail).  Successors (the entries' and the first ones)
    uniform over {-1, 0 .. m-1} -- self-successors ("retry") and rows without a table (-1 / -1) among them; START_HERE or an explicit
    start inside the box (z = |z| + 1, a random yaw) with probability 0.5 each; KEEP_ZAXIS with probability 0.5, else a drawn byte; every
    fourth explicit entry's goal 0.6 .. 2 m from its start; one entry in five has a max_run_dist of 5 cm (it times out in its first
    step), the others 3 |start - goal| + 1 (START_HERE: the box's diagonal stands in for the distance)."""
    n = scene['n']
    rng = np.random.default_rng(RNG_BASE + seed)
    side = RR.box_of(scene)
    e = np.zeros((n, m), MISSION)
    pos = rng.uniform(-side, side, (n, m, 3))
    pos[..., 2] = np.abs(pos[..., 2]) + 1.0
    goal = rng.uniform(-side, side, (n, m, 3))
    goal[..., 2] = np.abs(goal[..., 2]) + 1.0
    u = rng.normal(0, 1, (n, m, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    near = pos + u * rng.uniform(0.6, 2.0, (n, m, 1))
    near[..., 2] = np.abs(near[..., 2])
    here = rng.random((n, m)) < 0.5
    fourth = ((np.arange(n * m).reshape(n, m) % 4) == 3) & ~here
    goal[fourth] = near[fourth]
    e['pos'], e['goal'] = pos, goal
    e['heading'][..., 0] = rng.uniform(0, 2 * np.pi, (n, m))
    e['goal_heading'][..., 0] = rng.uniform(0, 2 * np.pi, (n, m))
    e['pref_speed'] = rng.choice([1.0, 0.8, 1.5], (n, m))
    dist = np.where(here, 2.0 * np.sqrt(3.0) * side, np.linalg.norm(pos - goal, axis=2))
    e['max_run_dist'] = np.where(rng.random((n, m)) < 0.2, 0.05, 3.0 * dist + 1.0)
    e['next_ok'] = rng.integers(-1, m, (n, m))
    e['next_fail'] = rng.integers(-1, m, (n, m))
    keep = rng.random((n, m)) < 0.5
    e['zaxis'] = rng.integers(0, 2, (n, m))
    e['flags'] = np.where(here, START_HERE, 0) | np.where(keep, KEEP_ZAXIS, 0)
    first_ok = rng.integers(-1, m, n).astype(np.int32)
    first_fail = rng.integers(-1, m, n).astype(np.int32)
    return e, first_ok, first_fail


def outcome_of(flags):
    return COLLIDED if flags & 2 else ARRIVED if flags & 1 else TIMED_OUT


class Tables:
    """the per-row words of the feature and the rule that advances them behind a step"""
    def __init__(self, entries, first_ok, first_fail):
        self.e, self.first_ok, self.first_fail = entries, np.asarray(first_ok, np.int32), np.asarray(first_fail, np.int32)
        n = len(self.first_ok)
        self.has = (self.first_ok >= 0) | (self.first_fail >= 0)
        self.cursor, self.flying, self.ended = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
        self.totals = dict.fromkeys(TOTALS, 0)

    def host_flight(self, ids):
        """the host respawned rows `ids` (a stopped row flies again): what flies is not an entry; the cursors stay"""
        self.flying[ids] = -1

    def advance(self, before, st, defs, zaxis, clear=None):
        """Behind a step: `before` the flags the rows entered it with, st / defs / zaxis the state and definitions after it -- the taken rows
        are overwritten IN PLACE (the caller hands copies).  clear: the closest-approach records in front of the step's respawns (None: the
        empty record).  Returns the step's results in ascending id and the ids taken."""
        n = len(before)
        self.totals['updates'] += 1
        self.totals['agent_steps'] += int(((before & 7) == 0).sum())
        rows = np.flatnonzero(((before & 7) == 0) & ((st['flags'] & 7) != 0))
        res = np.zeros(int(self.has[rows].sum()), RESULT)
        res['clear'] = empty_clear(len(res))
        k, taken = 0, []
        for a in rows:
            f = int(st['flags'][a])
            out = outcome_of(f)
            self.totals[('arrived', 'collided', 'timed_out')[out]] += 1
            nxt = -1
            if self.has[a]:
                c = self.cursor[a]
                ok, fail = (self.first_ok[a], self.first_fail[a]) if c < 0 else (self.e['next_ok'][a, c], self.e['next_fail'][a, c])
                nxt = int(ok if out == ARRIVED else fail)
                r = res[k]
                k += 1
                r['id'], r['entry'], r['flags'], r['step_num'], r['total_dist'], r['pos'] = a, self.flying[a], f, st['step_num'][a], st['total_dist'][a], st['pos'][a]
                r['update'], r['next'] = self.totals['updates'], nxt
                if clear is not None:
                    r['clear'] = clear[a]
                self.ended[a] += 1
                self.flying[a] = nxt
            self.totals['taken' if nxt >= 0 else 'stopped'] += 1
            if nxt < 0:
                continue
            e = self.e[a, nxt]
            if not e['flags'] & START_HERE:
                st['pos'][a], st['heading'][a] = e['pos'], e['heading']
            st['vel'][a] = e['vel']
            st['flags'][a], st['total_dist'][a], st['step_num'][a] = 0, 0.0, 0
            defs['goal'][a], defs['pref_speed'][a], defs['max_run_dist'][a] = e['goal'], e['pref_speed'], e['max_run_dist']
            if not e['flags'] & KEEP_ZAXIS:
                zaxis[a] = e['zaxis']
            self.cursor[a] = nxt
            taken.append(a)
        assert n == len(self.has)
        return res, np.array(taken, np.int64)


_RUNS = collections.OrderedDict()
_RUNS_MAX = 24


def oracle_run(oracle, scene, steps=STEPS, m=M, list_rule=0):
    """The trajectory with tables.  One dict per step: everything respawn_rule.oracle_run records of a step (action, lists, diag, perm,
    `before`, `defs` the step ran with, the state behind K4 as `ended_state`), then what the rule leaves behind the step: the state (pos ..
    step_num) with the taken rows replaced, `zaxis`, `results` (RESULT records, ascending id), `taken`, `cursor`, `ended`, `flying`,
    `totals`, `finished` (np.flatnonzero of the done flags the NEXT step starts with) and `active`.  list_rule: the oracle's (1: the lists the
    grid documents).  Memoised; nobody writes to the arrays."""
    key = scene['key'] + (steps, m, list_rule, 'missions')
    if key in _RUNS:
        _RUNS.move_to_end(key)
        return _RUNS[key]
    s, n = scene, scene['n']
    seed = scene['key'][1]
    entries, first_ok, first_fail = draw_tables(seed, s, m)
    T = Tables(entries, first_ok, first_fail)
    zaxis = np.array(F.zaxis_of(s), np.uint8, copy=True)
    st = dict(pos=s['pos'].copy(), vel=s['vel'].copy(), heading=s['heading'].copy(), flags=s['flags'].copy(), total_dist=np.zeros(n),
              step_num=np.zeros(n, np.int32))
    defs = {k: np.array(s[k], np.float64, copy=True) for k in RR.DEF_KEYS}
    perm = np.arange(n, dtype=np.int32)
    out = []
    oracle.set_list_rule(list_rule)
    for t in range(steps):
        r = oracle.policy_step(st['pos'], st['vel'], st['heading'], defs['radius'], defs['pref_speed'], st['flags'], defs['goal'], s['policy'],
                               zaxis, s['vpref'], s['vmode'], perm, s['obs_pos'], s['obs_radius'], nthreads=8)
        perm = r['perm']
        u = oracle.env_update(st['pos'], st['vel'], st['heading'], defs['radius'], r['flags'], defs['goal'], r['action'], st['total_dist'],
                              defs['max_run_dist'], st['step_num'], s['obs_pos'], s['obs_radius'])
        step = {k: r[k] for k in ('action', 'nbr_valid', 'nbr_n', 'nbr_id', 'nbr_kind', 'nbr_dsq', 'diag', 'perm', 'status', 'vpref')}
        step.update(before=st['flags'], flags_policy=r['flags'], defs=defs, zaxis_before=zaxis)
        ended_state = {k: u[k] for k in F.STATE_KEYS}
        st = {k: np.array(v, copy=True) for k, v in ended_state.items()}
        defs = {k: v.copy() for k, v in defs.items()}
        zaxis = zaxis.copy()
        res, taken = T.advance(step['before'], st, defs, zaxis)
        step.update(st)
        step.update(ended_state=ended_state, results=res, taken=taken, zaxis=zaxis, defs_after=defs, cursor=T.cursor.copy(), ended=T.ended.copy(),
                    flying=T.flying.copy(), totals=dict(T.totals), finished=np.flatnonzero((st['flags'] & 7) != 0))
        step['active'] = n - len(step['finished'])
        out.append(step)
    oracle.set_list_rule(0)
    run = dict(steps=out, entries=entries, first_ok=first_ok, first_fail=first_fail, has=T.has)
    _RUNS[key] = run
    while len(_RUNS) > _RUNS_MAX:
        _RUNS.popitem(last=False)
    return run


CLASSES = ('take_arrived', 'take_collided', 'take_timed_out', 'stops', 'retries', 'retries_ending_next_step', 'start_here', 'explicit_start',
           'tracked_taken', 'lp_taken', 'group_doubles', 'ring_overflow_r1')


def corpus_counts(scene, run):
    """What a run feeds the feature with, from the oracle's records and the rule alone: takes by the ended flight's outcome, stops (endings
    of rows with a table that name no successor), self-successor retries and those whose retried flight ends again in the very next step,
    entries taken with START_HERE and with an explicit start, tracked (SCA / RVO3D+Dubins) and ORCA3D-LP rows taken, steps x 64-row groups
    in which two or more rows with a table ended, and rows that ended more than once (a ring of R = 1 collected at the end overflowed)."""
    c = dict.fromkeys(CLASSES, 0)
    e = run['entries']
    retried_last = np.zeros(scene['n'], bool)
    for st in run['steps']:
        res = st['results']
        took = res['next'] >= 0
        out = np.array([outcome_of(int(f)) for f in res['flags']], np.int64)
        for name, o in (('take_arrived', ARRIVED), ('take_collided', COLLIDED), ('take_timed_out', TIMED_OUT)):
            c[name] += int((took & (out == o)).sum())
        c['stops'] += int((~took).sum())
        retry = took & (res['next'] == res['entry'])
        c['retries'] += int(retry.sum())
        c['retries_ending_next_step'] += int(retried_last[res['id']].sum())
        retried_last[:] = False
        retried_last[res['id'][retry]] = True
        fl = e['flags'][res['id'][took], res['next'][took]]
        c['start_here'] += int(((fl & START_HERE) != 0).sum())
        c['explicit_start'] += int(((fl & START_HERE) == 0).sum())
        pol = scene['policy'][res['id'][took]]
        c['tracked_taken'] += int(np.isin(pol, (0, 5)).sum())
        c['lp_taken'] += int((pol == 4).sum())
        c['group_doubles'] += int((np.bincount(res['id'] // 64) >= 2).sum()) if len(res) else 0
    c['ring_overflow_r1'] = int((run['steps'][-1]['ended'] >= 2).sum())
    return c
