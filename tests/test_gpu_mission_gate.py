"""The mission tables' admission gate (sca_set_mission_gate: a row takes its next mission only where its start is free) on the GPU (-m gpu).
Equality, no tolerance.

Two references.  The corpus of tests/mission_gate_rule.py: the fuzz scenes of tests/form_fuzz.py stepped free-running by the oracle while
every row carries a drawn table and the Python rule (mission_rule's endings, spawn_rule's gate, waiting rows first) is applied behind every
step at margin 0.5 -- state, action rows, lists, diag, permutation, sca_active_count, sca_get_finished, cursors, `ended`, results, both
totals and the waiting / verdict / refusal words equal the rule's behind every call.  And a TWIN context without tables that calls
sca_respawn_agents_gated between its steps, naming the first max_per_step candidates in the offer order with the entries' values (class
GateTwin): equal word for word, tracker records and re-plan counts included, its calls' verdicts the words the gate leaves."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import form_fuzz as F
import mission_gate_rule as GR
import mission_rule as MR
import spawn_rule as SR
from test_gpu_form_fuzz import compare_with_oracle, context_of
from test_gpu_missions import behind, by_row, context_for, same, traffic_scene

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


@pytest.fixture()
def row_env(monkeypatch):
    """only the row's switches (form_fuzz.ROWS) are set while its contexts are created"""
    def set_row(row):
        for k in list(os.environ):
            if k.startswith('SCA_') and k != 'SCA_QUIET':
                monkeypatch.delenv(k)
        for k, v in (F.ROWS[row] if row else {}).items():
            monkeypatch.setenv(k, v)
    return set_row


def check_gate_words(sol, waiting, verdict, refusals, gate_totals, at):
    w, v, r = sol.mission_gate_state()
    assert np.array_equal(w, waiting), at + ('waiting', np.flatnonzero(w != waiting)[:8])
    assert np.array_equal(v, verdict), at + ('verdict', np.flatnonzero(v != verdict)[:8])
    assert np.array_equal(r, refusals), at + ('refusals', np.flatnonzero(r != refusals)[:8])
    t = sol.mission_gate_totals()
    assert t == gate_totals, at + ('gate totals', t, gate_totals)
    assert t['offered'] == sum(t[k] for k in GR.VERDICT_TOTAL), at + (t,)


def check_rule_words(sol, r, at):
    cursor, ended = sol.mission_state()
    assert np.array_equal(cursor, r['cursor']) and np.array_equal(ended, r['ended']), at + ('cursor / ended',)
    t = sol.mission_totals()
    assert t == r['totals'], at + ('totals', t, r['totals'])
    check_gate_words(sol, r['waiting'], r['verdict'], r['refusals'], r['gate_totals'], at)


# ---- the twin ------------------------------------------------------------------------------------------------------------------------------
class GateTwin:
    """The gated tables' rule done by the host on a context WITHOUT tables: behind every step sca_get_finished, the endings' results, and
    ONE sca_respawn_agents_gated naming the first `cap` candidates in the offer order (waiting rows in ascending id, then the step's new
    ones) -- with the pos / heading sca_get_state returns for START_HERE, the row's own zaxis byte for KEEP_ZAXIS.  Keeps the cursors,
    `ended`, the results, both totals and the gate's words as the device should."""
    def __init__(self, sol, n, entries, first_ok, first_fail, radius, zaxis, margin, cap=0, tracker=False, clearance=False, running=None):
        self.sol, self.sc = sol, dict(n=n)
        self.e, self.first_ok, self.first_fail = entries, np.asarray(first_ok, np.int32), np.asarray(first_fail, np.int32)
        self.has = (self.first_ok >= 0) | (self.first_fail >= 0)
        self.cursor, self.flying, self.ended = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
        self.running = np.ones(n, bool) if running is None else np.array(running, bool)
        self.radius, self.zaxis = np.asarray(radius, np.float64), np.array(zaxis, np.uint8)
        self.totals = dict.fromkeys(MR.TOTALS, 0)
        self.margin, self.cap = margin, cap or GR.default_cap(n)
        self.tracker, self.clearance = tracker, clearance
        self.waiting, self.verdict, self.refusals = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.gate_totals = dict.fromkeys(GR.GATE_TOTALS, 0)
        self.results, self.calls = [], []

    def step(self, nbr, stepper=None):
        self.totals['updates'] += 1
        self.totals['agent_steps'] += int(self.running.sum())
        if stepper is None:
            self.sol.run_steps(1, nbr)
        else:
            stepper(self.sol)
        fin = self.sol.finished()
        ended = fin[self.running[fin['id']]]
        self.running[fin['id']] = False
        clear = self.sol.clearance() if self.clearance else None
        res = np.zeros(int(self.has[ended['id']].sum()), MR.RESULT)
        res['clear'] = MR.empty_clear(len(res))
        k, new = 0, []
        for row in ended:
            a, f = int(row['id']), int(row['flags'])
            out = MR.outcome_of(f)
            self.totals[('arrived', 'collided', 'timed_out')[out]] += 1
            nxt = -1
            if self.has[a]:
                c = self.cursor[a]
                ok, fail = (self.first_ok[a], self.first_fail[a]) if c < 0 else (self.e['next_ok'][a, c], self.e['next_fail'][a, c])
                nxt = int(ok if out == MR.ARRIVED else fail)
                r = res[k]
                k += 1
                r['id'], r['entry'], r['flags'], r['step_num'], r['total_dist'], r['pos'] = a, self.flying[a], f, row['step_num'], row['total_dist'], row['pos']
                r['update'], r['next'] = self.totals['updates'], nxt
                if clear is not None:
                    r['clear'] = clear[a]
                self.ended[a] += 1
                self.flying[a] = nxt
            if nxt < 0:
                self.totals['stopped'] += 1
            else:
                new.append((a, nxt))
        self.results.append(res)
        order = [(int(a), int(self.waiting[a])) for a in np.flatnonzero(self.waiting >= 0)] + new
        call = dict(order=order, verdict=np.zeros(0, np.int32), probe=None)
        self.calls.append(call)
        if not order:
            return res
        self.gate_totals['offered'] += len(order)
        tested = order[:self.cap]
        ids, js = np.array([a for a, _ in tested], np.int32), np.array([j for _, j in tested])
        e = self.e[ids, js]
        st = self.sol.get_state()
        here = ((e['flags'] & MR.START_HERE) != 0)[:, None]
        keep = (e['flags'] & MR.KEEP_ZAXIS) != 0
        zaxis = np.where(keep, self.zaxis[ids], e['zaxis']).astype(np.uint8)
        verdict, probe = self.sol.respawn(ids, np.where(here, st['pos'][ids], e['pos']), e['vel'], np.where(here, st['heading'][ids], e['heading']), self.radius[ids],
                                          e['pref_speed'], e['goal'], e['max_run_dist'], zaxis=zaxis, goal_heading=e['goal_heading'] if self.tracker else None,
                                          margin=self.margin)
        call.update(verdict=verdict.copy(), probe=probe.copy())
        for (a, j), v, z in list(zip(tested, verdict, zaxis)) + [(c, GR.OVER_CAP, 0) for c in order[self.cap:]]:
            self.waiting[a], self.verdict[a], self.refusals[a], name, take = GR.settle(int(v), j, int(self.refusals[a]))
            self.gate_totals[name] += 1
            if take:
                self.cursor[a] = self.flying[a] = j
                self.zaxis[a] = z
                self.running[a] = True
                self.totals['taken'] += 1
        return res

    def host_respawned(self, ids):
        """rows the host respawned on BOTH contexts (the caller did): what flies is not an entry, a pending mission is gone"""
        ids = np.atleast_1d(ids)
        self.flying[ids] = -1
        self.running[ids] = True
        for a in ids:
            if self.waiting[a] >= 0:
                self.waiting[a] = -1
                self.gate_totals['dropped'] += 1


def same_gated(A, B, tw, at, served=None, tracker=False, results=None):
    same(A, B, tw, at, served, tracker, results)
    check_gate_words(A, tw.waiting, tw.verdict, tw.refusals, tw.gate_totals, at)
    t, g = tw.totals, tw.gate_totals
    assert t['arrived'] + t['collided'] + t['timed_out'] == t['taken'] + t['stopped'] + g['dropped'] + int((tw.waiting >= 0).sum()), at


# ---- the corpus ----------------------------------------------------------------------------------------------------------------------------
def run_corpus(S, oracle, scene, nbr, ctx, steps=MR.STEPS, R=2, cap=0, per_call=1, twin=False):
    """context A (tables and the gate) against the rule behind every call of `per_call` steps; twin: a context B without tables does the
    rule through sca_respawn_agents_gated step by step, its verdicts and world records are the rule's and A equals it behind every call"""
    run = GR.oracle_run(oracle, scene, steps, cap=cap)
    n = scene['n']
    sol = context_of(S, scene)
    B = None
    try:
        sol.set_missions(MR.M, R, run['entries'], run['first_ok'], run['first_fail'])
        sol.set_mission_gate(GR.MARGIN, cap)
        if twin:
            B = context_of(S, scene)
            tw = GateTwin(B, n, run['entries'], run['first_ok'], run['first_fail'], scene['radius'], F.zaxis_of(scene), GR.MARGIN, cap, running=(scene['flags'] & 7) == 0)
        for t0 in range(0, steps, per_call):
            at = ctx + ('n', n, 'step', t0, 'cap', cap)
            sol.run_steps(per_call, nbr)
            sol.synchronize()
            r = run['steps'][t0 + per_call - 1]
            compare_with_oracle(sol, behind(r), scene, at)
            assert sol.active_count() == r['active'], at + ('active_count', sol.active_count(), r['active'])
            assert np.array_equal(sol.finished()['id'], r['finished']), at + ('finished ids',)
            check_rule_words(sol, r, at)
            want = by_row([s['results'] for s in run['steps'][t0:t0 + per_call]])
            if R < per_call:                                                # a row's last R results of the burst
                keep = np.ones(len(want), bool)
                for a in np.unique(want['id']):
                    mine = np.flatnonzero(want['id'] == a)
                    keep[mine[:-R]] = False
                want = want[keep]
            assert sol.mission_results().tobytes() == want.tobytes(), at + ('results',)
            if twin:
                for t in range(t0, t0 + per_call):
                    tw.step(nbr)
                    saw, call = run['steps'][t]['saw'], tw.calls[-1]
                    assert call['order'] == saw['order'], at + ('the twin offers in the rule\'s order',)
                    assert np.array_equal(call['verdict'], saw['verdict']), at + ('the twin\'s verdicts',)
                    if saw['tested']:
                        assert call['probe'].tobytes() == np.ascontiguousarray(saw['probe']).astype(call['probe'].dtype).tobytes(), at + ('world records',)
                same_gated(sol, B, tw, at)
    finally:
        sol.close()
        if B is not None:
            B.close()
    return run


@pytest.mark.parametrize('block', range(4))
def test_corpus_kd_default_forms(S, oracle, row_env, block):
    """kd mode, default forms, all 40 seeds (1 .. 1600 agents), 12 steps, everything compared behind every step; every second scene with
    the twin beside it"""
    row_env(None)
    for seed in MR.SEEDS[10 * block:10 * block + 10]:
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_KDTREE, ('kd', 'seed', seed), twin=seed % 2 == 0)


@pytest.mark.parametrize('row,mode', [(None, 'auto'), ('large_shard', 'kd'), ('large_shard', 'auto')])
def test_corpus_auto_and_large_shard(S, oracle, row_env, row, mode):
    """SCA_NBR_AUTO and the forms every large shard runs, ten seeds each"""
    row_env(row)
    for seed in MR.SEEDS[:10]:
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE, (row, mode, 'seed', seed))


def test_corpus_at_a_cap_of_8(S, oracle, row_env):
    """max_per_step = 8: rows over the cap wait with SCA_SPAWN_OVER_CAP, in front of every later arrival"""
    row_env(None)
    over = []
    for seed in (5, 12, 17, 33):
        run = run_corpus(S, oracle, F.random_scene(seed), S.NBR_KDTREE, ('cap 8', 'seed', seed), cap=8, twin=seed in (12, 17))
        over.append(run['steps'][-1]['gate_totals']['over_cap'])
    assert sum(1 for v in over if v > 0) >= 2, over


def test_corpus_hostbuild(S, oracle, row_env):
    """SCA_NBR_KDTREE_HOSTBUILD: the host builds the tree from positions it fetches behind the device-side respawns"""
    row_env(None)
    for seed in MR.SEEDS[:10]:
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_KDTREE_HOSTBUILD, ('hostbuild', 'seed', seed), steps=6)


def test_corpus_grid(S, oracle, row_env):
    """SCA_NBR_GRID against the oracle under list rule 1, on the scenes the grid takes (a scene it refuses ends at the refusal)"""
    from test_gpu_grid_fuzz import compare_grid_step
    row_env(None)
    whole = 0
    for seed in MR.SEEDS[:10]:
        scene = F.random_scene(seed)
        run = GR.oracle_run(oracle, scene, 6, list_rule=1)
        sol = context_of(S, scene, perm=False)
        try:
            sol.set_missions(MR.M, 1, run['entries'], run['first_ok'], run['first_fail'])
            sol.set_mission_gate(GR.MARGIN)
            for t, r in enumerate(run['steps']):
                at = ('grid', 'seed', seed, 'step', t)
                try:
                    sol.run_steps(1, S.NBR_GRID)
                except S.ScaError as e:
                    assert 'SCA_NBR_GRID needs' in str(e), at + (str(e),)
                    break
                sol.synchronize()
                compare_grid_step(sol, behind(r), scene, at)
                assert np.array_equal(sol.finished()['id'], r['finished']), at
                check_rule_words(sol, r, at)
                assert sol.mission_results().tobytes() == r['results'].tobytes(), at + ('results',)
            else:
                whole += 1
        finally:
            sol.close()
    assert whole >= 5, whole


@pytest.mark.parametrize('per_call', [3, 12])
def test_corpus_bursts(S, oracle, row_env, per_call):
    """sca_run_steps(3) and (12) with no host call in between, kd and AUTO: waiting rows are offered again inside the burst"""
    row_env(None)
    offered_again = 0
    for seed, nbr, R in ((5, S.NBR_KDTREE, 12), (12, S.NBR_AUTO, 12), (17, S.NBR_AUTO, 1), (33, S.NBR_KDTREE, 1)):
        run = run_corpus(S, oracle, F.random_scene(seed), nbr, ('burst', per_call, 'seed', seed, 'R', R), R=R, per_call=per_call)
        offered_again += sum(s['saw']['n_waiting'] for s in run['steps'])
    assert offered_again > 0


# ---- shapes where the kernels can go wrong ---------------------------------------------------------------------------------------------------
def shape_scene(n, count, n_obs, spacing=3.0):
    """n rows on a grid `spacing` apart at z = 10 that fly 30 m up; the first `count` rows time out in their FIRST step (max_run_dist 5 cm)
    and become candidates for entry 0, whose start depends on i % 4 --
      0: 1.5 m above its own grid point (free, unless an obstacle stands beside it);  1: 0.9 m beside the start of row i - 1 (within the
      margin of an earlier candidate: entry-blocked where that one is world-clear);  2: START_HERE (free);  3: the grid point of row i + 1 (a
      drone stands there: blocked by an agent).
    Obstacle k (radius 0.5) stands 0.9 m beside the entry-0 start of row 4 k while such a row exists (that start is blocked by an
    obstacle), the others far below the scene.  Entry 0 retries itself after a failure and goes on with entry 1 (START_HERE) after an arrival."""
    side = int(math.ceil(math.sqrt(n)))
    i = np.arange(n)
    grid = np.stack([spacing * (i % side), spacing * (i // side), np.full(n, 10.0)], 1)
    up = np.array([0.0, 0.0, 1.5])
    e = np.zeros((n, 2), MR.MISSION)
    pos0 = grid + up
    pos0[i % 4 == 1] = (grid + up)[np.flatnonzero(i % 4 == 1) - 1] + [0.9, 0.0, 0.0]
    pos0[i % 4 == 3] = grid[(np.flatnonzero(i % 4 == 3) + 1) % n]
    e['pos'][:, 0] = pos0
    e['goal'][:, 0] = grid + [0.0, 0.0, 30.0]
    e['goal'][:, 1] = grid + [0.0, 0.0, 20.0]
    e['pref_speed'], e['max_run_dist'] = 1.0, 200.0
    e['flags'][:, 0] = np.where(i % 4 == 2, MR.START_HERE, 0)
    e['flags'][:, 1] = MR.START_HERE
    e['next_ok'], e['next_fail'] = np.array([1, 0], np.int8)[None, :], np.array([0, 0], np.int8)[None, :]
    mrd = np.full(n, 200.0)
    mrd[:count] = 0.05
    obs_pos = np.tile([0.0, 0.0, -60.0], (n_obs, 1)) + np.arange(n_obs)[:, None] * [2.0, 0.0, 0.0]
    near = [k for k in range(n_obs) if 4 * k < n]
    for k in near:
        obs_pos[k] = grid[4 * k] + up + [0.0, 0.9, 0.0]
    return dict(n=n, start=grid, goal=grid + [0.0, 0.0, 30.0], heading=np.zeros((n, 3)), mrd=mrd, policy=np.array([(1, 3, 4)[k % 3] for k in range(n)], np.uint8),
                zaxis=np.zeros(n, np.uint8), radius=np.full(n, 0.5), entries=e, first_ok=np.ones(n, np.int32), first_fail=np.zeros(n, np.int32), gh=np.zeros((n, 3)),
                tracker=False, obs_pos=obs_pos, obs_radius=np.full(n_obs, 0.5))


def shape_context(S, sc, flags=None):
    n = sc['n']
    sol = S.BatchedSolver(max_agents=n, max_obstacles=max(1, len(sc['obs_radius'])))
    try:
        sol.set_obstacles(sc['obs_pos'], sc['obs_radius'])
        sol.set_agents(sc['radius'], np.ones(n), sc['goal'], sc['policy'], sc['zaxis'], sc['mrd'])
        sol.set_state(sc['start'], np.zeros((n, 3), np.float32), sc['heading'], np.zeros(n, np.uint8) if flags is None else flags)
    except BaseException:
        sol.close()
        raise
    return sol


def offers(tw):
    """the twin's calls that offered somebody, in order (a max_run_dist of 5 cm is passed in the SECOND step of a flight that starts at
    rest: the first call of a shape scene offers nobody)"""
    return [c for c in tw.calls if c['order']]


def run_shape(S, sc, at, steps=4, cap=0, margin=0.5, nbr=None):
    """the gated tables against the twin on a shape scene; returns the twin (both contexts closed)"""
    A = B = None
    M = sc['entries'].shape[1]
    try:
        A, B = shape_context(S, sc), shape_context(S, sc)
        A.set_missions(M, 2, sc['entries'], sc['first_ok'], sc['first_fail'])
        A.set_mission_gate(margin, cap)
        tw = GateTwin(B, sc['n'], sc['entries'], sc['first_ok'], sc['first_fail'], sc['radius'], sc['zaxis'], margin, cap)
        for t in range(steps):
            served = tw.running.copy()
            A.run_steps(1, nbr or S.NBR_KDTREE)
            res = tw.step(nbr or S.NBR_KDTREE)
            same_gated(A, B, tw, at + ('step', t), served, False, res)
    finally:
        for s in (A, B):
            if s is not None:
                s.close()
    return tw


@pytest.mark.parametrize('n', [1, 2, 511, 512, 513, 1025])
@pytest.mark.parametrize('n_obs', [0, 1, 23])
def test_partner_counts(S, row_env, n, n_obs):
    """1, 2, one tile less one, exactly one, one more and two tiles and one of agents, with 0, 1 and 23 obstacles behind them; a third of the
    rows end in the first step.  n = 1: the agent half of the probe is empty and the row is admitted."""
    row_env(None)
    count = max(1, n // 3)
    tw = run_shape(S, shape_scene(n, count, n_obs), ('partners', n, n_obs))
    first = offers(tw)[0]
    assert len(first['order']) == count, (len(first['order']), tw.gate_totals)
    if n == 1:                                                             # (with obstacles: one stands beside row 0's start)
        assert list(first['verdict']) == [SR.BLOCKED_OBSTACLE if n_obs else SR.ADMITTED] and first['probe']['agent_partner'][0] == -1
    if n_obs == 0 or n > 2:
        assert tw.gate_totals['admitted'] > 0, tw.gate_totals
    if n >= 511:
        assert tw.gate_totals['blocked_agent'] > 0 and tw.gate_totals['blocked_entry'] > 0, tw.gate_totals
        assert (tw.gate_totals['blocked_obstacle'] > 0) == (n_obs > 0), tw.gate_totals


def test_a_maps_worth_of_synthetic_obstacles(S, row_env):
    """1491 spheres behind 300 agents, most of them far below the scene (the real map: the next test)"""
    row_env(None)
    tw = run_shape(S, shape_scene(300, 100, 1491), ('map',), steps=3)
    assert tw.gate_totals['blocked_obstacle'] > 0 and tw.gate_totals['admitted'] > 0, tw.gate_totals


def exp3_scene():
    """64 drones among the exp3 map's 1491 spheres (the fixture F10_sca_exp3_map: r = 0.2, voxels 0.1 .. 0.2 m apart, so they overlap and a
    point between two of them has two equal minima).  The drones stand on points of a 1 m lattice at z = 2 that are clear of every sphere by
    more than 1.2 m and 3 m apart; all of them pass their max_run_dist of 5 cm at once and become candidates for entry 0, whose start
    depends on i % 4 -- 0: the centre of a sphere (inside: a negative clearance);  1: beside a sphere, 0.3 m between the two surfaces
    (blocked at margin 0.5);  2: another clear lattice point (free);  3: midway between a sphere and its nearest neighbour (a tie between
    the two, the lower id wins).  The spheres used are more than 2.5 m from every drone.  Entry 0 retries itself after a failure."""
    import edge_corpus as E
    fx = E.step_scene('F10_sca_exp3_map', 0)
    assert fx['m'] == 1491
    obs, rad = np.ascontiguousarray(fx['obs_pos'], np.float64).reshape(-1, 3), np.ascontiguousarray(fx['obs_radius'], np.float64)
    lo, hi = obs.min(0), obs.max(0)
    g = np.stack(np.meshgrid(np.arange(lo[0], hi[0], 1.0), np.arange(lo[1], hi[1], 1.0), [2.0], indexing='ij'), -1).reshape(-1, 3)
    clear = (np.linalg.norm(g[:, None] - obs[None], axis=2) - rad[None]).min(1) - 0.5
    pick = []
    for q in g[clear > 1.2]:
        if all(np.linalg.norm(q - w) >= 3.0 for w in pick):
            pick.append(q)
    n = 64
    assert len(pick) >= n + n // 4, len(pick)
    start, free = np.array(pick[:n]), np.array(pick[n:n + n // 4])
    away = np.flatnonzero(np.linalg.norm(obs[:, None] - start[None], axis=2).min(1) > 2.5)
    d = np.linalg.norm(obs[:, None] - obs[None], axis=2)
    np.fill_diagonal(d, np.inf)
    nearest = d.argmin(1)
    i = np.arange(n)
    k = away[(np.arange(n) * 7) % len(away)]                               # the sphere row i's start is built on
    pos0 = obs[k].copy()
    pos0[i % 4 == 1] += [0.2 + 0.5 + 0.3, 0.0, 0.0]
    pos0[i % 4 == 2] = free
    pos0[i % 4 == 3] = 0.5 * (obs[k] + obs[nearest[k]])[i % 4 == 3]
    e = np.zeros((n, 1), MR.MISSION)
    e['pos'][:, 0], e['goal'][:, 0] = pos0, start + [0.0, 0.0, 30.0]
    e['pref_speed'], e['max_run_dist'], e['next_ok'], e['next_fail'] = 1.0, 200.0, -1, 0
    return dict(n=n, start=start, goal=start + [0.0, 0.0, 30.0], heading=np.zeros((n, 3)), mrd=np.full(n, 0.05), policy=np.array([(1, 3, 4)[q % 3] for q in range(n)], np.uint8),
                zaxis=np.ones(n, np.uint8), radius=np.full(n, 0.5), entries=e, first_ok=np.full(n, -1, np.int32), first_fail=np.zeros(n, np.int32), gh=np.zeros((n, 3)),
                tracker=False, obs_pos=obs, obs_radius=rad)


def test_among_the_1491_spheres_of_the_exp3_map(S, row_env):
    """the real map behind 64 agents: four partner tiles, three of them obstacles only, and the obstacle half decides -- starts inside a
    sphere, beside one, between two and clear of all; the gated tables against the twin for four steps, and the first offer's verdicts and
    world records (the twin's call outputs) against the Python rule"""
    row_env(None)
    sc = exp3_scene()
    tw = run_shape(S, sc, ('exp3 map',), steps=4)
    first = offers(tw)[0]
    n = sc['n']
    assert [a for a, _ in first['order']] == list(range(n))
    v, rec = first['verdict'], first['probe']
    i = np.arange(n)
    assert (rec['obs_clear'][i % 4 == 0] < 0).all() and (v[i % 4 == 0] == SR.BLOCKED_OBSTACLE).all()
    beside = 1.0 - (0.5 + 0.2)                                             # the centres 1.0 apart, the radius sum first: 0.3 m as doubles give it
    assert (rec['obs_clear'][i % 4 == 1] <= beside).all() and (v[i % 4 == 1] != SR.ADMITTED).all()
    assert (v[i % 4 == 2] == SR.ADMITTED).sum() >= 8, v[i % 4 == 2]
    assert (v[i % 4 == 3] == SR.BLOCKED_OBSTACLE).all()
    assert (v == SR.BLOCKED_OBSTACLE).sum() >= n // 2
    # the rule on what the step left: the rows stand where they ended (5 cm above their starts; the probe is taken there)
    qpos = sc['entries']['pos'][:, 0]
    ended = by_row([r for r in tw.results if len(r)][:1])
    assert np.array_equal(ended['id'], i)
    want_v, want_rec = SR.gate(i.astype(np.int32), qpos, sc['radius'], 0.5, ended['pos'], sc['radius'], sc['obs_pos'], sc['obs_radius'])
    assert np.array_equal(v, want_v)
    assert rec.tobytes() == np.ascontiguousarray(want_rec).astype(rec.dtype).tobytes()
    ties = 0
    for q in np.flatnonzero(i % 4 == 3):                                   # equal minima: the lower obstacle id is the partner
        c = np.round(np.linalg.norm(sc['obs_pos'] - qpos[q], axis=1), 5) - (0.5 + sc['obs_radius'])
        same_min = np.flatnonzero(c == c.min())
        ties += len(same_min) > 1
        assert rec['obs_partner'][q] == same_min[0], (q, same_min, rec['obs_partner'][q])
    assert ties >= 8, ties


@pytest.mark.parametrize('count', [0, 1, 63, 64, 65, 257])
def test_candidate_counts(S, row_env, count):
    """no candidate, one, one chunk less one, exactly one, one more, and more than four chunks in one step"""
    row_env(None)
    tw = run_shape(S, shape_scene(300, count, 5), ('candidates', count))
    assert (count == 0) == (tw.gate_totals['offered'] == 0)
    if count:
        assert len(offers(tw)[0]['order']) == count and tw.gate_totals['offered'] > count


@pytest.mark.parametrize('cap', [1, 64])
def test_a_cap_against_65_candidates(S, row_env, cap):
    """max_per_step 1 and 64 against 65 candidates: the rest waits over the cap and comes first behind the next step"""
    row_env(None)
    tw = run_shape(S, shape_scene(300, 65, 5), ('cap', cap), steps=5, cap=cap)
    first, second = offers(tw)[:2]
    assert len(first['order']) == 65 and len(first['verdict']) == cap and tw.gate_totals['over_cap'] >= 65 - cap
    assert [c for c in second['order'] if c in first['order'][cap:]] == first['order'][cap:]       # who waited over the cap is offered again, in order


def test_every_row_ends_at_once_under_the_default_cap(S, row_env):
    """n = 2049: every row a candidate in the first step, 33 chunks over the probe's eight slots per tile"""
    row_env(None)
    tw = run_shape(S, shape_scene(2049, 2049, 3), ('all', 2049), steps=3)
    first = offers(tw)[0]
    assert len(first['order']) == 2049 == len(first['verdict'])
    v = first['verdict']
    assert all((v == k).any() for k in range(4)), np.bincount(v)


@pytest.mark.parametrize('n,mode', [(48, 'kd'), (64, 'kd'), (33, 'auto')])
def test_twin_with_the_device_tracker(S, row_env, n, mode):
    """tracked rows (SCA / RVO3D+Dubins) among the others on the dense traffic ring (coincident pairs, START_HERE entries that stand on
    their partner), the tracker inside the pass, closest-approach records on in kd mode: plans, re-plan counts and records equal the twin's
    behind every step, and a result carries the record of the ended flight"""
    row_env(None)
    sc = traffic_scene(n, True)
    nbr = S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE
    clearance = mode == 'kd'
    A, B = context_for(S, sc, True, clearance), context_for(S, sc, True, clearance)
    try:
        A.set_missions(3, 2, sc['entries'], sc['first_ok'], sc['first_fail'])
        A.set_mission_gate(0.5)
        tw = GateTwin(B, n, sc['entries'], sc['first_ok'], sc['first_fail'], sc['radius'], sc['zaxis'], 0.5, tracker=True, clearance=clearance)
        for t in range(14):
            served = tw.running.copy()
            A.run_steps(1, nbr)
            res = tw.step(nbr)
            same_gated(A, B, tw, ('tracker', n, mode, 'step', t), served, True, res)
            if clearance:
                assert np.array_equal(A.clearance(), B.clearance())
        g = tw.gate_totals
        assert g['admitted'] > 0 and g['blocked_agent'] > 0, g
        took = [a for c in tw.calls for (a, _), v in zip(c['order'], c['verdict']) if v == SR.ADMITTED]
        assert np.isin(sc['policy'][took], (0, 5)).any()
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize('form', ['env_step', 'pass_update', 'run3', 'run12'])
def test_step_forms_and_the_log(S, row_env, form):
    """sca_env_step, sca_policy_pass + sca_env_update and bursts of 3 and 12 equal the stepwise twin; the trajectory log holds the same rows"""
    row_env(None)
    sc = traffic_scene(96, True)
    A, B = context_for(S, sc, history=16), context_for(S, sc, history=16)
    try:
        A.set_missions(3, 12, sc['entries'], sc['first_ok'], sc['first_fail'])
        A.set_mission_gate(0.5)
        tw = GateTwin(B, 96, sc['entries'], sc['first_ok'], sc['first_fail'], sc['radius'], sc['zaxis'], 0.5, tracker=True)
        per = dict(run3=3, run12=12).get(form, 1)
        for t0 in range(0, 12, per):
            if form == 'env_step':
                A.env_step(S.NBR_KDTREE)
            elif form == 'pass_update':
                A.policy_pass(S.NBR_KDTREE)
                A.env_update()
            else:
                A.run_steps(per, S.NBR_KDTREE)
            res = [tw.step(S.NBR_KDTREE) for _ in range(per)]
            same_gated(A, B, tw, (form, 'step', t0), None, True, by_row(res))
        assert tw.gate_totals['admitted'] > 0 and tw.gate_totals['offered'] > tw.gate_totals['admitted']
        ha, hb = A.history(), B.history()
        for k in ha:
            assert np.array_equal(ha[k], hb[k], equal_nan=True), (form, 'log', k)
    finally:
        A.close()
        B.close()


# ---- hand-built cases with exact expectations ------------------------------------------------------------------------------------------------
def hand_scene(start, goal, mrd, entries, first_ok, first_fail, flags=None):
    n = len(start)
    return dict(n=n, start=np.array(start, np.float64), goal=np.array(goal, np.float64), heading=np.zeros((n, 3)), mrd=np.array(mrd, np.float64),
                policy=np.full(n, 1, np.uint8), zaxis=np.zeros(n, np.uint8), radius=np.full(n, 0.5), entries=entries, first_ok=np.array(first_ok, np.int32),
                first_fail=np.array(first_fail, np.int32), obs_pos=np.zeros((0, 3)), obs_radius=np.zeros(0), flags=None if flags is None else np.array(flags, np.uint8))


def entry_table(n, starts, flags=0, next_fail=-1):
    """one entry per row: an explicit start (or START_HERE), a goal 40 m above it, stopping after whatever comes"""
    e = np.zeros((n, 1), MR.MISSION)
    e['pos'][:, 0] = starts
    e['goal'][:, 0] = np.asarray(starts, np.float64) + [0.0, 0.0, 40.0]
    e['pref_speed'], e['max_run_dist'] = 1.0, 200.0
    e['flags'], e['next_ok'], e['next_fail'] = flags, -1, next_fail
    return e


def hand_context(S, sc, margin, cap=0, R=4, warm=True):
    """tables and gate set; warm: one step taken, in which nobody ends -- a flight that starts at rest passes a max_run_dist of 5 cm in its
    SECOND step, so that the rows built to time out do so in the caller's first step"""
    sol = shape_context(S, sc, sc['flags'])
    try:
        sol.set_missions(sc['entries'].shape[1], R, sc['entries'], sc['first_ok'], sc['first_fail'])
        sol.set_mission_gate(margin, cap)
        if warm:
            sol.run_steps(1, S.NBR_KDTREE)
            assert sol.mission_gate_totals()['offered'] == 0 and sol.mission_state()[1].sum() == 0
    except BaseException:
        sol.close()
        raise
    return sol


def respawn_away(sol, a, where):
    sol.respawn([a], [where], np.zeros((1, 3), np.float32), np.zeros((1, 3)), [0.5], [1.0], [np.asarray(where, np.float64) + [0.0, 0.0, 40.0]], [200.0])


FAR = 50.0


def test_a_row_waits_until_the_parked_drone_is_gone(S, row_env):
    """(a) row 0 times out in step 1; a parked drone (row 1, finished from the start) stands within the margin of its next start.  The row
    waits, two steps; the host respawns the parked drone elsewhere; the row is admitted at the end of the next step with refusals 2"""
    row_env(None)
    P = np.array([20.0, 0.0, 10.0])
    sc = hand_scene([[0, 0, 10], P + [1.2, 0, 0]], [[0, 0, 50], [0, 0, 60]], [0.05, 200.0], entry_table(2, [P, P]), [-1, -1], [0, -1], flags=[0, 1])
    sol = hand_context(S, sc, 0.5)
    try:
        for t in (1, 2):
            sol.run_steps(1, S.NBR_KDTREE)
            w, v, r = sol.mission_gate_state()
            assert (w[0], v[0], r[0]) == (0, SR.BLOCKED_AGENT, t) and w[1] == -1
            assert sol.mission_state()[0][0] == -1 and list(sol.finished()['id']) == [0, 1] and sol.active_count() == 0
        assert sol.mission_results()['next'].tolist() == [0]
        respawn_away(sol, 1, [FAR, FAR, 10.0])
        sol.run_steps(1, S.NBR_KDTREE)
        w, v, r = sol.mission_gate_state()
        assert (w[0], v[0], r[0]) == (-1, SR.ADMITTED, 2)
        st = sol.get_state()
        assert np.array_equal(st['pos'][0], P) and st['flags'][0] == 0 and st['step_num'][0] == 0 and sol.mission_state()[0][0] == 0
        g = sol.mission_gate_totals()
        assert (g['offered'], g['admitted'], g['blocked_agent'], g['dropped']) == (3, 1, 2, 0)
        assert sol.mission_totals()['taken'] == 1 and sol.active_count() == 2
    finally:
        sol.close()


@pytest.mark.parametrize('margin,want', [(1.0, SR.BLOCKED_AGENT), (np.nextafter(1.0, 0.0), SR.ADMITTED)])
def test_the_boundary_pair(S, row_env, margin, want):
    """(b) the start exactly 2.0 from a parked drone, radius sum 1.0: c = 1.0 is refused at margin 1.0 and admitted just below it"""
    row_env(None)
    P = np.array([20.0, 0.0, 10.0])
    sc = hand_scene([[0, 0, 10], P + [2.0, 0, 0]], [[0, 0, 50], [0, 0, 60]], [0.05, 200.0], entry_table(2, [P, P]), [-1, -1], [0, -1], flags=[0, 1])
    sol = hand_context(S, sc, margin)
    try:
        sol.run_steps(1, S.NBR_KDTREE)
        w, v, r = sol.mission_gate_state()
        assert sol.mission_gate_totals()['offered'] == 1
        assert v[0] == want and (w[0] == -1) == (want == SR.ADMITTED) and r[0] == (want != SR.ADMITTED)
        assert sol.mission_state()[0][0] == (0 if want == SR.ADMITTED else -1)
    finally:
        sol.close()


def test_the_chain(S, row_env):
    """(c) a < b < c end together; b's start lies within the margin of a's and of c's, a's and c's are apart: a is admitted, b is blocked
    by a, and c is refused although b was -- b is world-clear, which is all the entry test asks"""
    row_env(None)
    A0 = np.array([20.0, 0.0, 10.0])
    starts = [A0, A0 + [1.3, 0, 0], A0 + [2.6, 0, 0]]
    sc = hand_scene([[0, 0, 10], [0, 5, 10], [0, 10, 10]], [[0, 0, 50], [0, 5, 50], [0, 10, 50]], [0.05] * 3, entry_table(3, starts), [-1] * 3, [0] * 3)
    sol = hand_context(S, sc, 0.5)
    try:
        sol.run_steps(1, S.NBR_KDTREE)
        w, v, r = sol.mission_gate_state()
        assert v.tolist() == [SR.ADMITTED, SR.BLOCKED_ENTRY, SR.BLOCKED_ENTRY] and w.tolist() == [-1, 0, 0] and r.tolist() == [0, 1, 1]
        sol.run_steps(1, S.NBR_KDTREE)                                      # a flies from its start now: b is blocked by an agent and blocks nobody, c goes
        w, v, r = sol.mission_gate_state()
        assert v.tolist() == [SR.ADMITTED, SR.BLOCKED_AGENT, SR.ADMITTED] and w.tolist() == [-1, 0, -1] and r.tolist() == [0, 2, 1]
    finally:
        sol.close()


def test_waiting_rows_come_first(S, row_env):
    """(d) row 5 waits (a parked drone, row 7, at its start); the host gives row 1 a flight that ends two steps later and moves row 7 away in
    front of that step; the starts of 5 and 1 lie within the margin of each other.  The waiting row is admitted and the new one entry-blocked; ascending id alone would
    give the opposite"""
    row_env(None)
    P = np.array([20.0, 0.0, 10.0])
    n = 8
    start = [[3.0 * i, -20.0, 10.0] for i in range(n)]
    start[7] = list(P + [1.2, 0, 0])
    starts = np.array([[100.0 + 3 * i, 0, 10] for i in range(n)])
    starts[5], starts[1] = P, P + [0, 1.3, 0]
    mrd = [200.0] * n
    mrd[5] = 0.05
    fail = [-1] * n
    fail[5] = fail[1] = 0
    sc = hand_scene(start, [[s[0], s[1], 60.0] for s in start], mrd, entry_table(n, starts), [-1] * n, fail, flags=[0] * 7 + [1])
    sol = hand_context(S, sc, 0.5)
    try:
        sol.run_steps(1, S.NBR_KDTREE)
        w, v, r = sol.mission_gate_state()
        assert (w[5], v[5], r[5]) == (0, SR.BLOCKED_AGENT, 1)
        st = sol.get_state()
        sol.respawn([1], [st['pos'][1]], np.zeros((1, 3), np.float32), np.zeros((1, 3)), [0.5], [1.0], [[3.0, -20.0, 60.0]], [0.05])     # row 1 ends in the step after the next
        sol.run_steps(1, S.NBR_KDTREE)
        w, v, r = sol.mission_gate_state()
        assert (w[5], v[5], r[5]) == (0, SR.BLOCKED_AGENT, 2) and w[1] == -1
        respawn_away(sol, 7, [FAR, FAR, 10.0])
        sol.run_steps(1, S.NBR_KDTREE)
        w, v, r = sol.mission_gate_state()
        assert (w[5], v[5], r[5]) == (-1, SR.ADMITTED, 2), (w, v, r)
        assert (w[1], v[1], r[1]) == (0, SR.BLOCKED_ENTRY, 1), (w, v, r)
        g = sol.mission_gate_totals()
        assert (g['offered'], g['admitted'], g['blocked_agent'], g['blocked_entry']) == (4, 1, 2, 1)
    finally:
        sol.close()


def test_start_here_after_a_collision(S, row_env):
    """(e) rows 0 and 1 start on one spot and collide in step 1; row 0's successor starts where it stands -- on its partner, which has no
    table and stays: it waits; once the host has respawned the partner away it goes, from where it stands"""
    row_env(None)
    sc = hand_scene([[0, 0, 10], [0, 0, 10]], [[0, 0, 50], [0, 0, 60]], [200.0, 200.0], entry_table(2, [[0, 0, 0]] * 2, flags=MR.START_HERE), [-1, -1], [0, -1])
    sol = hand_context(S, sc, 0.5, warm=False)
    try:
        for t in (1, 2, 3):
            sol.run_steps(1, S.NBR_KDTREE)
            w, v, r = sol.mission_gate_state()
            assert (w[0], v[0], r[0]) == (0, SR.BLOCKED_AGENT, t)
        res = sol.mission_results()
        assert len(res) == 1 and res['flags'][0] & 2 and res['next'][0] == 0
        stood = sol.get_state()['pos'][0].copy()
        respawn_away(sol, 1, [FAR, FAR, 10.0])
        sol.run_steps(1, S.NBR_KDTREE)
        w, v, r = sol.mission_gate_state()
        st = sol.get_state()
        assert (w[0], v[0], r[0]) == (-1, SR.ADMITTED, 3) and st['flags'][0] == 0 and np.array_equal(st['pos'][0], stood)
    finally:
        sol.close()


def test_a_self_successor_retries_under_the_gate(S, row_env):
    """(f) an entry that times out in its first step and names itself: taken again behind every step, never refused"""
    row_env(None)
    P = np.array([20.0, 0.0, 10.0])
    e = entry_table(1, [P], next_fail=0)
    e['max_run_dist'] = 0.05
    sc = hand_scene([[0, 0, 10]], [[0, 0, 50]], [0.05], e, [-1], [0])
    sol = hand_context(S, sc, 0.5)
    try:
        sol.run_steps(7, S.NBR_KDTREE)
        cursor, ended = sol.mission_state()
        assert cursor[0] == 0 and ended[0] >= 3 and sol.mission_gate_state()[2][0] == 0
        t, g = sol.mission_totals(), sol.mission_gate_totals()
        assert t['taken'] == ended[0] == t['timed_out'] == g['admitted'] == g['offered']
        res = sol.mission_results()
        assert len(res) == min(4, ended[0]) and (res['entry'][1:] == 0).all() and (res['next'] == 0).all()       # (a ring of four: the last endings)
        assert sol.active_count() == 1
    finally:
        sol.close()


# ---- lifecycle ---------------------------------------------------------------------------------------------------------------------------------
def test_the_gate_set_after_some_steps_and_taken_off_again(S, row_env):
    """tables alone for four steps (rows are put wherever the table says), the gate for six (the twin follows from the words the tables
    left), then off with rows waiting: their missions are dropped and counted, the rows stay finished, and the context goes on as one with
    tables alone does"""
    row_env(None)
    sc = traffic_scene(64, False)
    n = 64
    A, B = context_for(S, sc), context_for(S, sc)
    try:
        from test_gpu_missions import Twin
        A.set_missions(3, 2, sc['entries'], sc['first_ok'], sc['first_fail'])
        with pytest.raises(S.ScaError):
            A.mission_gate_state()                                          # no gate has been set since the tables arrived
        tw0 = Twin(B, sc)
        for t in range(4):
            A.run_steps(1, S.NBR_KDTREE)
            tw0.step(S.NBR_KDTREE)
        A.set_mission_gate(0.5)
        tw = GateTwin(B, n, sc['entries'], sc['first_ok'], sc['first_fail'], sc['radius'], tw0.zaxis, 0.5, running=tw0.running)
        tw.cursor, tw.flying, tw.ended, tw.totals = tw0.cursor, tw0.flying, tw0.ended, tw0.totals
        A.mission_results()
        for t in range(6):
            served = tw.running.copy()
            A.run_steps(1, S.NBR_KDTREE)
            res = tw.step(S.NBR_KDTREE)
            same_gated(A, B, tw, ('late gate', t), served, False, res)
        waiting = int((tw.waiting >= 0).sum())
        assert waiting > 0 and tw.gate_totals['admitted'] > 0
        fin = A.finished()['id'].copy()
        A.set_mission_gate(None)
        w, v, r = A.mission_gate_state()
        assert (w == -1).all() and np.array_equal(r, tw.refusals) and A.mission_gate_totals()['dropped'] == waiting
        assert np.array_equal(A.finished()['id'], fin)
        A.set_mission_gate(None)                                            # off twice: nothing more is dropped
        assert A.mission_gate_totals()['dropped'] == waiting
        # from here on A is a context with tables alone: B follows with the plain tables' twin
        tw0.running, tw0.zaxis = tw.running, tw.zaxis
        tw0.cursor, tw0.flying, tw0.ended, tw0.totals = tw.cursor, tw.flying, tw.ended, tw.totals
        for t in range(4):
            served = tw0.running.copy()
            A.run_steps(1, S.NBR_KDTREE)
            res = tw0.step(S.NBR_KDTREE)
            same(A, B, tw0, ('gate off', t), served, False, res)
        assert A.mission_gate_totals()['offered'] == tw.gate_totals['offered']
    finally:
        for s in (A, B):
            s.close()


def test_tables_without_a_gate_equal_tables_that_never_heard_of_one(S, row_env):
    """a gate set and taken off before the first step leaves a context that is, step by step, the one with tables alone"""
    row_env(None)
    sc = traffic_scene(48, True)
    A, B = context_for(S, sc), context_for(S, sc)
    try:
        for s in (A, B):
            s.set_missions(3, 2, sc['entries'], sc['first_ok'], sc['first_fail'])
        A.set_mission_gate(0.5, 7)
        A.set_mission_gate(None)
        for t in range(8):
            A.run_steps(1, S.NBR_KDTREE)
            B.run_steps(1, S.NBR_KDTREE)
            ga, gb = A.get_state(), B.get_state()
            assert all(np.array_equal(ga[k], gb[k]) for k in ga), t
            assert A.mission_totals() == B.mission_totals() and A.mission_results().tobytes() == B.mission_results().tobytes()
        assert A.mission_totals()['taken'] > 0 and A.mission_gate_totals() == dict.fromkeys(GR.GATE_TOTALS, 0)
    finally:
        A.close()
        B.close()


def test_the_obstacle_set_grows_under_a_standing_gate(S, row_env):
    """the gate is set while the context has no obstacle; 700 arrive afterwards (two more partner tiles): the partials follow"""
    row_env(None)
    sc = shape_scene(300, 100, 700)
    A = B = None
    try:
        A, B = shape_context(S, sc), shape_context(S, sc)
        A.set_obstacles(np.zeros((0, 3)), np.zeros(0))
        A.set_missions(2, 2, sc['entries'], sc['first_ok'], sc['first_fail'])
        A.set_mission_gate(0.5)
        A.set_obstacles(sc['obs_pos'], sc['obs_radius'])
        tw = GateTwin(B, 300, sc['entries'], sc['first_ok'], sc['first_fail'], sc['radius'], sc['zaxis'], 0.5)
        for t in range(3):
            served = tw.running.copy()
            A.run_steps(1, S.NBR_KDTREE)
            res = tw.step(S.NBR_KDTREE)
            same_gated(A, B, tw, ('obstacles grow', t), served, False, res)
        assert tw.gate_totals['blocked_obstacle'] > 0, tw.gate_totals
    finally:
        for s in (A, B):
            if s is not None:
                s.close()


def waiting_pair(S):
    """rows 0 and 2 wait (parked drones 1 and 3 stand at their next starts)"""
    P, Q = np.array([20.0, 0.0, 10.0]), np.array([40.0, 0.0, 10.0])
    sc = hand_scene([[0, 0, 10], P + [1.2, 0, 0], [0, 6, 10], Q + [1.2, 0, 0]], [[0, 0, 50], [0, 0, 60], [0, 6, 50], [0, 0, 60]], [0.05, 200.0, 0.05, 200.0],
                    entry_table(4, [P, P, Q, Q]), [-1] * 4, [0, -1, 0, -1], flags=[0, 1, 0, 1])
    sol = hand_context(S, sc, 0.5)
    sol.run_steps(1, S.NBR_KDTREE)
    assert sol.mission_gate_state()[0].tolist() == [0, -1, 0, -1]
    return sol, sc


def test_set_state_under_a_standing_gate(S, row_env):
    """a new state: row 0 is unfinished in it and loses its pending mission (dropped + 1), row 2 is still finished and keeps waiting"""
    row_env(None)
    sol, sc = waiting_pair(S)
    try:
        st = sol.get_state()
        flags = st['flags'].copy()
        flags[0] = 0
        sol.set_state(st['pos'], st['vel'], st['heading'], flags, st['total_dist'], st['step_num'])
        w, v, r = sol.mission_gate_state()
        assert w.tolist() == [-1, -1, 0, -1] and r.tolist() == [1, 0, 1, 0] and sol.mission_gate_totals()['dropped'] == 1
        sol.run_steps(1, S.NBR_KDTREE)
        w, v, r = sol.mission_gate_state()
        assert w[2] == 0 and r[2] == 2 and w[0] in (-1, 0)
        t, g = sol.mission_totals(), sol.mission_gate_totals()
        assert t['arrived'] + t['collided'] + t['timed_out'] == t['taken'] + t['stopped'] + g['dropped'] + int((w >= 0).sum())
    finally:
        sol.close()


def test_a_host_respawn_of_a_waiting_row(S, row_env):
    """a plain respawn of waiting row 0 clears its word (dropped + 1); a gated respawn that REFUSES waiting row 2 leaves it waiting, one
    that admits it clears it"""
    row_env(None)
    sol, sc = waiting_pair(S)
    try:
        respawn_away(sol, 0, [FAR, FAR, 10.0])
        assert sol.mission_gate_state()[0].tolist() == [-1, -1, 0, -1] and sol.mission_gate_totals()['dropped'] == 1
        args = (np.zeros((1, 3), np.float32), np.zeros((1, 3)), [0.5], [1.0], [[40.0, 0.0, 60.0]], [200.0])
        verdict, _ = sol.respawn([2], [[41.2, 0.0, 10.0]], *args, margin=0.5)          # on the parked drone 3: refused
        assert verdict[0] == SR.BLOCKED_AGENT and sol.mission_gate_state()[0][2] == 0 and sol.mission_gate_totals()['dropped'] == 1
        verdict, _ = sol.respawn([2], [[-FAR, -FAR, 10.0]], *args, margin=0.5)
        assert verdict[0] == SR.ADMITTED and sol.mission_gate_state()[0][2] == -1 and sol.mission_gate_totals()['dropped'] == 2
        sol.run_steps(2, S.NBR_KDTREE)
        assert sol.active_count() == 2 and sol.mission_gate_totals()['offered'] == 2
    finally:
        sol.close()


def test_new_tables_clear_the_gate_and_every_refusal(S, row_env):
    row_env(None)
    sol, sc = waiting_pair(S)
    try:
        def refused(code, *a):
            with pytest.raises(S.ScaError) as e:
                sol.set_mission_gate(*a)
            assert '(rc=%d)' % code in str(e.value), (a, str(e.value))
        for bad in (-0.1, float('nan'), float('inf')):
            refused(ERR_ARG, bad)
        refused(ERR_ARG, 0.5, -1)
        refused(ERR_ARG, 0.5, 5)                                            # n = 4
        sol.policy_pass(S.NBR_KDTREE)
        refused(ERR_STATE, 0.5)
        sol.env_update()
        assert sol.mission_gate_state()[0].tolist() == [0, -1, 0, -1]      # a refused call changed nothing
        before = sol.mission_gate_totals()
        sol.set_mission_gate(0.25, 2)                                       # another margin and cap under a standing gate: who waits goes on waiting
        assert sol.mission_gate_state()[0].tolist() == [0, -1, 0, -1] and sol.mission_gate_totals() == before
        sol.run_steps(1, S.NBR_KDTREE)                                      # (the parked drones stand 0.2 m from the starts: still blocked at 0.25)
        w, v, r = sol.mission_gate_state()
        assert w.tolist() == [0, -1, 0, -1] and v.tolist()[0::2] == [SR.BLOCKED_AGENT] * 2 and r.tolist() == [3, 0, 3, 0]       # (the step of waiting_pair, the pass + update above, this one)
        assert sol.mission_gate_totals()['offered'] == before['offered'] + 2
        sol.set_missions(1, 4, sc['entries'], sc['first_ok'], sc['first_fail'])
        with pytest.raises(S.ScaError) as e:
            sol.mission_gate_totals()                                       # new tables: no gate
        assert '(rc=%d)' % ERR_STATE in str(e.value)
        sol.set_mission_gate(0.5, 4)
        assert sol.mission_gate_state()[0].tolist() == [-1] * 4 and sol.mission_gate_totals() == dict.fromkeys(GR.GATE_TOTALS, 0)
        sol.set_missions(0, 0, None, None, None)
        refused(ERR_STATE, 0.5)
        with pytest.raises(S.ScaError) as e:
            sol.mission_gate_state()
        assert '(rc=%d)' % ERR_STATE in str(e.value)
        sol.set_missions(1, 4, sc['entries'], sc['first_ok'], sc['first_fail'])
        sol.set_mission_gate(0.5)
        sol.set_agents(sc['radius'], np.ones(4), sc['goal'], sc['policy'], sc['zaxis'], sc['mrd'])
        refused(ERR_STATE, 0.5)                                             # a new agent set drops tables and gate
    finally:
        sol.close()


# ---- Python ------------------------------------------------------------------------------------------------------------------------------------
def ring_run(how, n, rad, steps, burst=1):
    """the example's ping-pong on a ring of n ORCA3D drones: an arrived drone flies back to where its mission began, a collided or
    timed-out one starts its original mission again -- by the host loop (how = 'host') or as a table of three entries on the device"""
    import sca_amd.env as E
    import sca_amd.scenarios as scenarios
    import sca_amd.solver as S
    from sca_amd.lifelong import run_lifelong, run_missions
    sc = scenarios.circle(n, rad=rad)
    pol = E.ORCA3DPolicy
    agents = [E.Agent(start_pos=list(sc['start'][i]), goal_pos=list(sc['goal'][i]), vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=pol, id=i) for i in range(n)]
    env = E.MACAEnv()
    env.set_agents(agents, obstacles=[])
    first = {a.id: (list(a.initial_pos), list(a.goal_pos)) for a in agents}
    if how == 'host':
        def next_mission(agent, row):
            if int(row['flags']) & S.FLAG_COLLISION or not int(row['flags']) & S.FLAG_AT_GOAL:
                start, goal = first[agent.id]
            else:
                start = list(row['pos']) + list(agent.heading_global_frame)
                goal = list(agent.initial_pos)
            return E.Agent(start_pos=start, goal_pos=goal, vel=[0.0, 0.0, 0.0], radius=agent.radius, pref_speed=agent.pref_speed, policy=pol, id=agent.id)
        stats = run_lifelong(env, next_mission, steps, spawn_margin=0.5)
        words = None
    else:
        def entry(i, start, goal):
            return E.Agent(start_pos=start, goal_pos=goal, vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=pol, id=i)
        tables = {i: E.MissionTable([entry(i, goal, start), entry(i, start, goal), entry(i, start, goal)], next_ok=[1, 0, 0], next_fail=[2, 2, 2],
                                    first_ok=0, first_fail=2, start_here=[True, True, False]) for i, (start, goal) in first.items()}
        last = {}
        stats = run_missions(env, tables, steps, burst=burst, spawn_margin=0.5, on_result=lambda agent, r: last.__setitem__(int(r['id']), r['pos'].copy()))
        words = env.solver.mission_gate_state()
        # the mirrors stand for the entry each row flies: the cursor's, also while a later one is still waiting
        cursor, _ = env.solver.mission_state()
        checked = 0
        for i in range(n):
            if cursor[i] < 0:
                continue
            src, here, _keep = tables[i].entries[cursor[i]]
            a = env.agents[i]
            assert np.array_equal(a.goal_pos, src.goal_pos) and np.array_equal(env.goal[i], src.goal_global_frame), (i, cursor[i])
            if words[0][i] < 0:                                             # (nothing pending: the last ending is the one this flight began at)
                assert np.array_equal(a.initial_pos[:3], last[i] if here else src.initial_pos[:3]), (i, cursor[i])
                checked += 1
        assert checked > n // 2
    state = env.solver.get_state()
    env.solver.close()
    return stats, state, words


def test_run_missions_against_run_lifelong_under_the_gate(row_env):
    """the three-entry ping-pong table on a small dense ring (64 drones 1.2 m apart: they meet in the middle, and a start is often taken
    by the drone that has just arrived there): lifelong.run_missions(spawn_margin=0.5) at burst 1 and 8 gives the stats of
    lifelong.run_lifelong(spawn_margin=0.5), `deferred` and `waiting` included, and the same final state; refusals and later admissions
    of refused rows both happen"""
    row_env(None)
    n, steps = 64, 480
    rad = 1.2 * n / (2 * math.pi)
    host, host_state, _ = ring_run('host', n, rad, steps)
    assert host['deferred'] > 0 and host['respawned'] > 0 and host['steps'] == steps, host
    for burst in (1, 8):
        dev, dev_state, (waiting, verdict, refusals) = ring_run('device', n, rad, steps, burst)
        assert dev == host, (burst, dev, host)
        for k in host_state:
            assert np.array_equal(dev_state[k], host_state[k]), (burst, k)
        assert ((refusals > 0) & (waiting < 0)).any(), 'no refused row was admitted later'
        assert int((waiting >= 0).sum()) == dev['waiting']


def test_the_mirrors_follow_a_start_here_retry(row_env):
    """one drone whose only entry starts where it stands, times out after 30 cm and names itself: the cursor never changes, and still
    MACAEnv.mission_results() moves the drone's start mirror to where the flight in the air began -- where the last ending happened"""
    row_env(None)
    import sca_amd.env as E
    start, goal = [0.0, 0.0, 10.0, 0.0, 0.0, 0.0], [40.0, 0.0, 10.0, 0.0, 0.0, 0.0]
    agent = E.Agent(start_pos=start, goal_pos=goal, vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=E.ORCA3DPolicy, id=0)
    agent.max_run_dist = 0.3
    again = E.Agent(start_pos=start, goal_pos=goal, vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=E.ORCA3DPolicy, id=0)
    again.max_run_dist = 0.3
    env = E.MACAEnv()
    try:
        env.set_agents([agent], obstacles=[])
        env.set_missions({0: E.MissionTable([again], next_ok=[-1], next_fail=[0], first_ok=-1, first_fail=0, start_here=True, keep_zaxis=True)}, results=8, spawn_margin=0.5)
        seen = []
        for _ in range(4):
            env.run_steps(6)
            res = env.mission_results()
            assert len(res) >= 1 and (res['next'] == 0).all() and env.solver.mission_gate_state()[0][0] == -1
            assert np.array_equal(env.agents[0].initial_pos[:3], res[-1]['pos']), (env.agents[0].initial_pos, res['pos'])
            seen.append(res[-1]['pos'][0])
        assert seen == sorted(seen) and seen[0] < seen[-1] and env.solver.mission_state()[0][0] == 0
    finally:
        env.solver.close()


def test_the_example_takes_the_flag_pair(row_env):
    row_env(None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'run_sca.py'), '--scenario', 'circle', '--agents', '32', '--policy', 'orca', '--no-obstacles',
                          '--lifelong', '120', '--device-missions', '--spawn-margin', '0.5', '--burst', '8'], capture_output=True, text=True, cwd=ROOT,
                         env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'spawn margin 0.5 m:' in out.stdout and 'missions still waiting' in out.stdout, out.stdout[-2000:]
