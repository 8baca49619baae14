"""Mission tables whose entries bring their own waypoint lists (sca_set_missions_paths), stated with the oracle alone: the composition of
tests/mission_rule.py (Tables.advance: who ended, the result, the successor taken), tests/mission_gate_rule.py (the same behind the gate)
and tests/path_rule.py (get_trajectory and the straight-line policies' v_pref toward now_goal).  Per step

  1. path_rule.pass_rule_csr advances the rows' lists from the state the step starts with; the oracle is stepped with the v_pref it yields
     on the rows it aims at a waypoint (mode 1), the scene's fed v_pref elsewhere -- as tests/form_fuzz.py and tests/respawn_rule.py feed it
  2. the oracle's policy_step and env_update
  3. Tables.advance (or GatedTables.advance) behind the step; where it TAKES entry j for row a the row's list becomes entry (a, j)'s whole
     list, now_goal None -- tests/respawn_rule.py's rule for a respawn that brings lists.  A row that stops, and a candidate that waits at
     the gate, keeps list, cursor and now_goal

The lists are in slot form with W = 3 points of room per row.  Every entry of the drawn three-entry tables gets a list of 0 .. W points
from form_fuzz.random_paths' five kinds (a third of the entries empty), drawn around the entry's own start and goal (START_HERE: the
scene's start of the row stands in for the unknown one); the rows' initial lists are form_fuzz.random_paths' cut to W.  Shared by
tests/test_mission_paths_cpu.py and tests/test_gpu_mission_paths.py.  Test infrastructure: it drives the oracle, the product never
imports it."""
import collections

import numpy as np

import form_fuzz as F
import mission_gate_rule as GR
import mission_rule as MR
import path_rule as R
import respawn_rule as RR

W = 3
STEPS = MR.STEPS
SEEDS = MR.SEEDS
LIST_SEED = 30_000
GATE_MARGIN = 0.5


def draw_lists(seed, scene, entries, w=W):
    """one list per entry, (n, m) nested: empty with probability 1 / 3, else 1 .. w points of form_fuzz.random_paths' kinds around the
    entry's start p and goal g (rounded to 3 places); list order -- get_trajectory pops from the end"""
    rng = np.random.default_rng(LIST_SEED + seed)
    n, m = entries.shape
    out = []
    for a in range(n):
        row = []
        for j in range(m):
            e = entries[a, j]
            p = np.array(scene['pos'][a] if e['flags'] & MR.START_HERE else e['pos'], np.float64)
            g, r = np.array(e['goal'], np.float64), float(scene['radius'][a])
            d = float(np.linalg.norm(g - p))
            u = (g - p) / d if d > 0 else np.zeros(3)
            lst = []
            k = 0 if rng.random() < 1.0 / 3.0 else int(rng.integers(1, w + 1))
            for _ in range(k):
                kind = int(rng.integers(0, 5))
                if kind == 0:
                    q = p + u * rng.uniform(0, r + 0.8) + rng.normal(0, 0.05, 3)
                elif kind == 1:
                    q = p - u * rng.uniform(0.5, 5)
                elif kind == 2:
                    q = p + (g - p) * rng.uniform(0.1, 0.9) + rng.normal(0, 1, 3)
                elif kind == 3:
                    q = g
                else:
                    q = p + rng.normal(0, r, 3)
                lst.append([float(x) for x in np.round(q, 3)])
            row.append(lst)
        out.append(row)
    return out


def flat_lists(lists):
    """the lists over the flat entry index M a + j, as sca_set_missions_paths takes them"""
    return [lst for row in lists for lst in row]


def initial_paths(seed, scene, w=W):
    return [lst[:w] for lst in F.random_paths(seed, scene)]


_RUNS = collections.OrderedDict()
_RUNS_MAX = 24


def oracle_run(oracle, scene, steps=STEPS, w=W, gate=None, list_rule=0, tables=None):
    """The trajectory with tables and lists.  One dict per step: everything mission_rule.oracle_run records of a step (gate = (margin,
    cap): mission_gate_rule.oracle_run's), and the lists -- path_left_before / now_goal_before / pos_before / path_off / path_pts (what the
    pass's rule started from), path_left / now_goal / vpref_rule / path_mode (behind the pass's rule: what tests' check_paths reads), and
    behind the step's takes path_len_after / path_left_after / now_goal_after / rooms_after (the rows' lists as nested Python lists) and
    mode_reset (rows taken that had a list: their vpref_mode is 0 until the next pass) and vpref_mode_after (every row's byte: the fed
    one, 1 where a pass aimed the row at a waypoint, 0 behind a reset; no device tracker in these runs).  tables: a hand-built (entries, first_ok,
    first_fail, lists, initial lists) in place of the drawn ones (not memoised).  Memoised; nobody writes to the arrays."""
    key = scene['key'] + (steps, w, gate, list_rule, 'mission paths')
    if tables is None and key in _RUNS:
        _RUNS.move_to_end(key)
        return _RUNS[key]
    s, n = scene, scene['n']
    seed = scene['key'][1]
    if tables is None:
        entries, first_ok, first_fail = MR.draw_tables(seed, s)
        lists, initial = draw_lists(seed, s, entries, w), initial_paths(seed, s, w)
    else:
        entries, first_ok, first_fail, lists, initial = tables
    T = MR.Tables(entries, first_ok, first_fail) if gate is None else GR.GatedTables(entries, first_ok, first_fail, gate[0], gate[1])
    zaxis = np.array(F.zaxis_of(s), np.uint8, copy=True)
    st = dict(pos=s['pos'].copy(), vel=s['vel'].copy(), heading=s['heading'].copy(), flags=s['flags'].copy(), total_dist=np.zeros(n),
              step_num=np.zeros(n, np.int32))
    defs = {k: np.array(s[k], np.float64, copy=True) for k in RR.DEF_KEYS}
    perm = np.arange(n, dtype=np.int32)
    paths = [list(p) for p in initial]
    rem, ng = np.array([len(p) for p in paths], np.int32), np.full((n, 3), np.nan)
    mode_word = np.array(s['vmode'], np.uint8, copy=True)      # the rows' vpref_mode bytes: fed, 1 where a pass aimed the row, 0 behind a reset
    out = []
    oracle.set_list_rule(list_rule)
    try:
        for t in range(steps):
            off, pts = R.csr(paths)
            path = dict(path_left_before=rem, now_goal_before=ng, pos_before=st['pos'], path_off=off, path_pts=pts)
            rem, ng, vp, mode = R.pass_rule_csr(off, pts, rem, ng, st['pos'], defs['goal'], defs['radius'], defs['pref_speed'], s['policy'], st['flags'])
            aimed = mode.astype(bool)
            vpref, vmode = np.where(aimed[:, None], vp, s['vpref']), np.where(aimed, 1, s['vmode']).astype(np.uint8)
            path.update(path_left=rem, now_goal=ng, vpref_rule=vp, path_mode=mode)
            mode_word = np.where(aimed, 1, mode_word).astype(np.uint8)
            r = oracle.policy_step(st['pos'], st['vel'], st['heading'], defs['radius'], defs['pref_speed'], st['flags'], defs['goal'], s['policy'],
                                   zaxis, vpref, vmode, perm, s['obs_pos'], s['obs_radius'], nthreads=8)
            perm = r['perm']
            u = oracle.env_update(st['pos'], st['vel'], st['heading'], defs['radius'], r['flags'], defs['goal'], r['action'], st['total_dist'],
                                  defs['max_run_dist'], st['step_num'], s['obs_pos'], s['obs_radius'])
            step = {k: r[k] for k in ('action', 'nbr_valid', 'nbr_n', 'nbr_id', 'nbr_kind', 'nbr_dsq', 'diag', 'perm', 'status', 'vpref')}
            step.update(before=st['flags'], flags_policy=r['flags'], defs=defs, zaxis_before=zaxis)
            step.update(path)
            ended_state = {k: u[k] for k in F.STATE_KEYS}
            st = {k: np.array(v, copy=True) for k, v in ended_state.items()}
            defs = {k: v.copy() for k, v in defs.items()}
            zaxis = zaxis.copy()
            if gate is None:
                res, taken = T.advance(step['before'], st, defs, zaxis)
            else:
                res, taken, saw = T.advance(step['before'], st, defs, zaxis, s['obs_pos'], s['obs_radius'])
                step.update(waiting=T.waiting.copy(), verdict=T.verdict.copy(), refusals=T.refusals.copy(), gate_totals=dict(T.gate_totals), saw=saw)
            paths = list(paths)
            rem, ng = rem.copy(), ng.copy()
            old_len = np.array([len(p) for p in paths], np.int32)
            for a in taken:
                paths[a] = lists[a][int(T.cursor[a])]
                rem[a] = len(paths[a])
                ng[a] = np.nan
            step.update(st)
            step.update(ended_state=ended_state, results=res, taken=taken, taken_entry=T.cursor[taken].copy(), zaxis=zaxis, defs_after=defs,
                        cursor=T.cursor.copy(), ended=T.ended.copy(), flying=T.flying.copy(), totals=dict(T.totals),
                        finished=np.flatnonzero((st['flags'] & 7) != 0), old_len=old_len, path_len_after=np.array([len(p) for p in paths], np.int32),
                        path_left_after=rem, now_goal_after=ng, rooms_after=paths,
                        mode_reset=np.array([a for a in taken if old_len[a] > 0 and int(s['policy'][a]) not in R.TRACKED], np.int64))
            mode_word = mode_word.copy()
            mode_word[step['mode_reset']] = 0
            step['vpref_mode_after'] = mode_word
            step['active'] = n - len(step['finished'])
            out.append(step)
    finally:
        oracle.set_list_rule(0)
    run = dict(steps=out, entries=entries, first_ok=first_ok, first_fail=first_fail, has=T.has, lists=lists, initial=initial, w=w)
    if gate is not None:
        run['cap'] = T.cap
    if tables is not None:
        return run
    _RUNS[key] = run
    while len(_RUNS) > _RUNS_MAX:
        _RUNS.popitem(last=False)
    return run


CLASSES = ('takes_with_list', 'takes_empty_onto_list_untracked', 'takes_empty_onto_list_tracked', 'takes_full_room', 'pops_right_after_take',
           'pops_later_after_take', 'orca_taken', 'tracked_taken_with_list', 'rows_taken_twice_different_lists')
GATE_CLASSES = ('gate_admitted', 'gate_waiting_rows_list_unmoved')


def corpus_counts(scene, run):
    """What a run feeds the feature with, from the oracle's records and the rule alone: takes that bring a non-empty list; takes that
    bring the empty list onto a row that had one (the MODE_RESET case), straight-line and tracked (SCA / RVO3D+Dubins) rows apart; takes
    of a list of exactly W points; pops by a taken row in the pass right after its take and in a later pass of the same flight; taken
    ORCA3D / ORCA3D-LP rows (they measure with `distance`); taken tracked rows whose entry brings a list; rows taken twice with
    different lists."""
    c = dict.fromkeys(CLASSES, 0)
    n, w = scene['n'], run['w']
    pol = scene['policy']
    since = np.full(n, -1, np.int64)                     # passes since the row's last take (-1: never taken)
    seen = [None] * n
    twice = np.zeros(n, bool)
    for st in run['steps']:
        popped = st['path_left'] < st['path_left_before']
        c['pops_right_after_take'] += int((popped & (since == 0)).sum())
        c['pops_later_after_take'] += int((popped & (since > 0)).sum())
        since[since >= 0] += 1
        for a, j in zip(st['taken'], st['taken_entry']):
            lst = run['lists'][a][int(j)]
            tracked = int(pol[a]) in R.TRACKED
            c['takes_with_list'] += bool(lst)
            if not lst and st['old_len'][a] > 0:
                c['takes_empty_onto_list_tracked' if tracked else 'takes_empty_onto_list_untracked'] += 1
            c['takes_full_room'] += len(lst) == w
            c['orca_taken'] += int(pol[a]) in R.ORCA
            c['tracked_taken_with_list'] += bool(lst) and tracked
            if seen[a] is not None and seen[a] != lst:
                twice[a] = True
            seen[a] = lst
            since[a] = 0
    c['rows_taken_twice_different_lists'] = int(twice.sum())
    return {k: int(v) for k, v in c.items()}


def gate_counts(scene, run):
    """Under the gate: rows admitted, and waiting rows (finished: no pass serves them) whose list, cursor and now_goal are behind the
    step what they were in front of it"""
    c = dict.fromkeys(GATE_CLASSES, 0)
    earlier = np.zeros(scene['n'], bool)                                   # waiting since an earlier step
    for st in run['steps']:
        c['gate_admitted'] += len(st['taken'])
        wait = st['waiting'] >= 0
        kept = (st['path_left_after'] == st['path_left']) & (st['path_len_after'] == st['old_len'])      # the gate's refusal touched nothing
        assert kept[wait].all()
        still = wait & earlier
        assert (st['path_left'] == st['path_left_before'])[still].all()   # ... and no pass serves a finished row
        c['gate_waiting_rows_list_unmoved'] += int(still.sum())
        earlier = wait
    return c
