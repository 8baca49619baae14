"""The admission gate in front of the mission tables' take (sca_set_mission_gate; include/sca_hip.h), stated with the oracle alone: the
composition of tests/mission_rule.py (Tables.advance: who ended, the result, the successor the ended flight names) and tests/spawn_rule.py
(gate: the world test and the entry test of sca_respawn_agents_gated).  Behind every step

  1. endings are mission_rule's: results, `ended`, `flying`, the outcome totals; a named successor -1 stops the row; j >= 0 makes the row a
     NEW candidate for entry j -- nothing of it is written, its cursor stays, `taken` does not move
  2. the candidates in offer order: the rows waiting since an earlier step in ascending id, then the step's new ones in ascending id
  3. only the first `cap` are tested, the others wait with OVER_CAP (a refusal like the others)
  4. spawn_rule.gate over the tested ones, in that order, against the state as it stands behind the step (START_HERE: the row's position)
  5. an admitted row is overwritten as mission_rule does it (cursor = flying = j, taken + 1, waiting cleared); a refused row keeps every
     word: waiting = j, verdict = the word, refusals + 1

Shared by tests/test_mission_gate_cpu.py (what the corpus holds, the host-compiled place / query / settle) and
tests/test_gpu_mission_gate.py (the kernels against it).  Test infrastructure: it drives the oracle, the product never imports it."""
import collections

import numpy as np

import form_fuzz as F
import mission_rule as MR
import respawn_rule as RR
import spawn_rule as SR

OVER_CAP = 4                                                                   # SCA_SPAWN_OVER_CAP
MARGIN = SR.MARGIN
GATE_TOTALS = ('offered', 'admitted', 'blocked_agent', 'blocked_obstacle', 'blocked_entry', 'over_cap', 'dropped')
VERDICT_TOTAL = ('admitted', 'blocked_agent', 'blocked_obstacle', 'blocked_entry', 'over_cap')
SPAWN_BATCH = 4096


def default_cap(n):
    return min(n, SPAWN_BATCH)


def place(cls_new, rank, waiting_total):
    """a candidate's place in the offer order: its rank inside its class, the new ones behind all waiting ones"""
    return waiting_total + rank if cls_new else rank


def settle(verdict, entry, refusals):
    """(waiting, verdict, refusals, counter name, take) for a candidate of entry `entry` whose row has been refused `refusals` times"""
    take = verdict == SR.ADMITTED
    return (-1 if take else entry, verdict, refusals if take else refusals + 1, VERDICT_TOTAL[verdict], take)


class GatedTables(MR.Tables):
    """mission_rule.Tables with the gate's words (waiting, verdict, refusals per row) and totals"""
    def __init__(self, entries, first_ok, first_fail, margin, cap=0):
        super().__init__(entries, first_ok, first_fail)
        n = len(self.first_ok)
        self.margin, self.cap = float(margin), int(cap) if cap else default_cap(n)
        self.waiting, self.verdict, self.refusals = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.gate_totals = dict.fromkeys(GATE_TOTALS, 0)

    def query(self, a, j, st):
        e = self.e[a, j]
        return np.array(st['pos'][a] if e['flags'] & MR.START_HERE else e['pos'], np.float64)

    def take(self, a, j, st, defs, zaxis):
        """mission_rule's overwrite of row a with entry j"""
        e = self.e[a, j]
        if not e['flags'] & MR.START_HERE:
            st['pos'][a], st['heading'][a] = e['pos'], e['heading']
        st['vel'][a] = e['vel']
        st['flags'][a], st['total_dist'][a], st['step_num'][a] = 0, 0.0, 0
        defs['goal'][a], defs['pref_speed'][a], defs['max_run_dist'][a] = e['goal'], e['pref_speed'], e['max_run_dist']
        if not e['flags'] & MR.KEEP_ZAXIS:
            zaxis[a] = e['zaxis']
        self.cursor[a] = self.flying[a] = j
        self.totals['taken'] += 1

    def host_clears(self, ids):
        """a host call made rows `ids` fly again (a respawn that admitted them, a new state in which they are unfinished)"""
        for a in ids:
            if self.waiting[a] >= 0:
                self.waiting[a] = -1
                self.gate_totals['dropped'] += 1

    def gate_off(self):
        self.host_clears(np.flatnonzero(self.waiting >= 0))

    def advance(self, before, st, defs, zaxis, obs_pos, obs_radius, clear=None):
        """Behind a step, as mission_rule.Tables.advance: st / defs / zaxis are overwritten in place for the ADMITTED rows.  Returns the
        step's results (ascending id), the ids taken, and a dict of what the gate saw: order (row, entry) in offer order, the number
        tested, verdict per tested candidate, probe (the world records), chains, n_waiting (how many of the order were waiting)."""
        self.totals['updates'] += 1
        self.totals['agent_steps'] += int(((before & 7) == 0).sum())
        rows = np.flatnonzero(((before & 7) == 0) & ((st['flags'] & 7) != 0))
        res = np.zeros(int(self.has[rows].sum()), MR.RESULT)
        res['clear'] = MR.empty_clear(len(res))
        k, new = 0, []
        for a in rows:
            f = int(st['flags'][a])
            out = MR.outcome_of(f)
            self.totals[('arrived', 'collided', 'timed_out')[out]] += 1
            nxt = -1
            if self.has[a]:
                c = self.cursor[a]
                ok, fail = (self.first_ok[a], self.first_fail[a]) if c < 0 else (self.e['next_ok'][a, c], self.e['next_fail'][a, c])
                nxt = int(ok if out == MR.ARRIVED else fail)
                r = res[k]
                k += 1
                r['id'], r['entry'], r['flags'], r['step_num'], r['total_dist'], r['pos'] = a, self.flying[a], f, st['step_num'][a], st['total_dist'][a], st['pos'][a]
                r['update'], r['next'] = self.totals['updates'], nxt
                if clear is not None:
                    r['clear'] = clear[a]
                self.ended[a] += 1
                self.flying[a] = nxt
            if nxt < 0:
                self.totals['stopped'] += 1
            else:
                new.append((int(a), nxt))
        waiting = [(int(a), int(self.waiting[a])) for a in np.flatnonzero(self.waiting >= 0)]
        order = waiting + new
        saw = dict(order=order, n_waiting=len(waiting), tested=min(len(order), self.cap), verdict=np.zeros(0, np.int32), probe=None, chains=[])
        taken = []
        if not order:
            return res, np.array(taken, np.int64), saw
        self.gate_totals['offered'] += len(order)
        tested = order[:self.cap]
        ids = np.array([a for a, _ in tested], np.int32)
        qpos = np.array([self.query(a, j, st) for a, j in tested]).reshape(-1, 3)
        qrad = np.asarray(defs['radius'], np.float64)[ids]
        verdict, rec = SR.gate(ids, qpos, qrad, self.margin, st['pos'], defs['radius'], obs_pos, obs_radius, saw['chains'])
        saw.update(verdict=verdict, probe=rec)
        for (a, j), v in list(zip(tested, verdict)) + [(c, OVER_CAP) for c in order[self.cap:]]:
            self.waiting[a], self.verdict[a], self.refusals[a], name, take = settle(int(v), j, int(self.refusals[a]))
            self.gate_totals[name] += 1
            if take:
                self.take(a, j, st, defs, zaxis)
                taken.append(a)
        return res, np.array(sorted(taken), np.int64), saw


_RUNS = collections.OrderedDict()
_RUNS_MAX = 24


def oracle_run(oracle, scene, steps=MR.STEPS, margin=MARGIN, cap=0, m=MR.M, list_rule=0):
    """mission_rule.oracle_run with the gate.  One dict per step as there, and: `waiting`, `verdict`, `refusals` (the words behind the
    step), `gate_totals`, `saw` (GatedTables.advance's).  Memoised; nobody writes to the arrays."""
    key = scene['key'] + (steps, m, list_rule, margin, cap, 'mission gate')
    if key in _RUNS:
        _RUNS.move_to_end(key)
        return _RUNS[key]
    s, n = scene, scene['n']
    seed = scene['key'][1]
    entries, first_ok, first_fail = MR.draw_tables(seed, s, m)
    T = GatedTables(entries, first_ok, first_fail, margin, cap)
    zaxis = np.array(F.zaxis_of(s), np.uint8, copy=True)
    st = dict(pos=s['pos'].copy(), vel=s['vel'].copy(), heading=s['heading'].copy(), flags=s['flags'].copy(), total_dist=np.zeros(n),
              step_num=np.zeros(n, np.int32))
    defs = {k: np.array(s[k], np.float64, copy=True) for k in RR.DEF_KEYS}
    perm = np.arange(n, dtype=np.int32)
    out = []
    oracle.set_list_rule(list_rule)
    try:
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
            res, taken, saw = T.advance(step['before'], st, defs, zaxis, s['obs_pos'], s['obs_radius'])
            step.update(st)
            step.update(ended_state=ended_state, results=res, taken=taken, zaxis=zaxis, defs_after=defs, cursor=T.cursor.copy(), ended=T.ended.copy(),
                        flying=T.flying.copy(), totals=dict(T.totals), finished=np.flatnonzero((st['flags'] & 7) != 0), waiting=T.waiting.copy(),
                        verdict=T.verdict.copy(), refusals=T.refusals.copy(), gate_totals=dict(T.gate_totals), saw=saw)
            step['active'] = n - len(step['finished'])
            out.append(step)
    finally:
        oracle.set_list_rule(0)
    run = dict(steps=out, entries=entries, first_ok=first_ok, first_fail=first_fail, has=T.has, cap=T.cap)
    _RUNS[key] = run
    while len(_RUNS) > _RUNS_MAX:
        _RUNS.popitem(last=False)
    return run


CLASSES = ('steps_with_candidates', 'steps_all', 'steps_part', 'steps_none',
           'new_admitted', 'new_blocked_agent', 'new_blocked_obstacle', 'new_blocked_entry', 'new_over_cap',
           'wait_admitted', 'wait_admitted_after_refusals', 'wait_blocked_agent', 'wait_blocked_obstacle', 'wait_blocked_entry', 'wait_over_cap',
           'chains', 'here_admitted', 'here_refused', 'waiting_at_end', 'scenes_wait_admitted', 'scenes_wait_blocked_entry', 'overtaken')
_NAMES = ('admitted', 'blocked_agent', 'blocked_obstacle', 'blocked_entry', 'over_cap')


def corpus_counts(run):
    """What a gated run holds, from the oracle's records and the rule alone: steps with candidates and how many of them admit everybody, a
    part, nobody; new and waiting candidates per verdict; the refusals the admitted waiting rows had collected; chain cases; START_HERE
    candidates admitted and refused; missions waiting at the end; whether the scene has a waiting row admitted / entry-blocked; and
    `overtaken`: tested waiting rows that stand BEHIND a new candidate in a step's order (the order forbids it: always 0)."""
    c = dict.fromkeys(CLASSES, 0)
    e = run['entries']
    refusals_before = np.zeros(len(run['first_ok']), np.int64)
    for st in run['steps']:
        saw = st['saw']
        order = saw['order']
        if order:
            words = list(saw['verdict']) + [OVER_CAP] * (len(order) - saw['tested'])
            ok = sum(1 for v in words if v == SR.ADMITTED)
            c['steps_with_candidates'] += 1
            c['steps_all' if ok == len(order) else 'steps_part' if ok else 'steps_none'] += 1
            seen_new = False
            for k, ((a, j), v) in enumerate(zip(order, words)):
                cls = 'wait' if k < saw['n_waiting'] else 'new'
                seen_new = seen_new or cls == 'new'
                if cls == 'wait' and seen_new:
                    c['overtaken'] += 1
                c[cls + '_' + _NAMES[v]] += 1
                if cls == 'wait' and v == SR.ADMITTED:
                    c['wait_admitted_after_refusals'] += int(refusals_before[a])
                if v != OVER_CAP and e['flags'][a, j] & MR.START_HERE:
                    c['here_admitted' if v == SR.ADMITTED else 'here_refused'] += 1
            c['chains'] += len(saw['chains'])
        refusals_before = st['refusals'].astype(np.int64)
    c['waiting_at_end'] = int((run['steps'][-1]['waiting'] >= 0).sum())
    c['scenes_wait_admitted'] = int(c['wait_admitted'] > 0)
    c['scenes_wait_blocked_entry'] = int(c['wait_blocked_entry'] > 0)
    return c
