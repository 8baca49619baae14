"""Mission tables (sca_set_missions: finished rows take their next mission inside the step) on the GPU (-m gpu).  Equality, no tolerance.

Two references.  The corpus of tests/mission_rule.py: the fuzz scenes of tests/form_fuzz.py (1 .. 1600 agents, obstacles, six policies)
stepped free-running by the oracle while every row carries a drawn table and the Python rule is applied behind every step -- state,
action rows, lists, diag, permutation, sca_active_count, cursors, `ended`, results and totals equal the rule's after every step.  And a TWIN
context that does the same through sca_get_finished + sca_respawn_agents between its steps (class Twin), equal word for word, tracker
records and re-plan counts included -- in every step form, at the sizes where the kernels change path, with retries, stops, records, the
log, a new state and dropped tables."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import form_fuzz as F
import mission_rule as MR
from test_gpu_form_fuzz import compare_with_oracle, context_of

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5


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


def by_row(results):
    """a list of result arrays in the collect's order: ascending id, within a row oldest first"""
    if not results:
        return np.zeros(0, MR.RESULT)
    r = np.concatenate(results)
    return r[np.argsort(r['id'], kind='stable')]


def behind(r):
    """the oracle's record of a step as the context holds it behind the mission kernel: a taken row's list of the pass is invalid (the
    respawn's rule) and its status word 0, everything else of the pass stays"""
    out = dict(r)
    out['nbr_valid'] = r['nbr_valid'].copy()
    out['nbr_valid'][r['taken']] = 0
    out['status'] = r['status'].copy()
    out['status'][r['taken']] = 0
    return out


def check_words(sol, r, at):
    cursor, ended = sol.mission_state()
    assert np.array_equal(cursor, r['cursor']) and np.array_equal(ended, r['ended']), at + ('cursor / ended',)
    t = sol.mission_totals()
    assert t == r['totals'], at + ('totals', t, r['totals'])


# ---- the corpus ----------------------------------------------------------------------------------------------------------------------------
def run_corpus(S, oracle, scene, nbr, ctx, steps=MR.STEPS, R=2):
    run = MR.oracle_run(oracle, scene, steps)
    sol = context_of(S, scene)
    try:
        sol.set_missions(MR.M, R, run['entries'], run['first_ok'], run['first_fail'])
        for t, r in enumerate(run['steps']):
            at = ctx + ('n', scene['n'], 'step', t)
            sol.run_steps(1, nbr)
            sol.synchronize()
            compare_with_oracle(sol, behind(r), scene, at)
            assert sol.active_count() == r['active'], at + ('active_count', sol.active_count(), r['active'])
            fin = sol.finished()
            assert np.array_equal(fin['id'], r['finished']), at + ('finished ids',)
            check_words(sol, r, at)
            res = sol.mission_results()
            assert res.tobytes() == r['results'].tobytes(), at + ('results', len(res), len(r['results']))
        assert len(sol.mission_results()) == 0
    finally:
        sol.close()


@pytest.mark.parametrize('block', range(4))
def test_corpus_kd_default_forms(S, oracle, row_env, block):
    """kd mode, default forms, all 40 seeds (1 .. 1600 agents), 12 steps, the results collected behind every step"""
    row_env(None)
    for seed in MR.SEEDS[10 * block:10 * block + 10]:
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_KDTREE, ('kd', 'seed', seed))


@pytest.mark.parametrize('row,mode,block', [(row, mode, b) for b in range(2) for row, mode in ((None, 'auto'), ('large_shard', 'kd'), ('large_shard', 'auto'))])
def test_corpus_auto_and_large_shard(S, oracle, row_env, row, mode, block):
    """SCA_NBR_AUTO and the forms every large shard runs on the first 20 seeds"""
    row_env(row)
    for seed in MR.SEEDS[10 * block:10 * block + 10]:
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE, (row, mode, 'seed', seed))


def test_corpus_hostbuild(S, oracle, row_env):
    """SCA_NBR_KDTREE_HOSTBUILD: the host builds the tree from positions it fetches behind the device-side respawns"""
    row_env(None)
    for seed in (3, 5, 12):
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_KDTREE_HOSTBUILD, ('hostbuild', 'seed', seed), steps=6)


def test_corpus_grid(S, oracle, row_env):
    """SCA_NBR_GRID against the oracle under list rule 1, on the scenes the grid takes (a scene it refuses ends at the refusal)"""
    from test_gpu_grid_fuzz import compare_grid_step
    row_env(None)
    whole = 0
    for seed in MR.SEEDS[:20]:
        scene = F.random_scene(seed)
        run = MR.oracle_run(oracle, scene, 6, list_rule=1)
        sol = context_of(S, scene, perm=False)
        try:
            sol.set_missions(MR.M, 1, run['entries'], run['first_ok'], run['first_fail'])
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
                check_words(sol, r, at)
                assert sol.mission_results().tobytes() == r['results'].tobytes(), at + ('results',)
            else:
                whole += 1
        finally:
            sol.close()
    assert whole >= 10, whole


@pytest.mark.parametrize('steps_per_call', [3, 12])
def test_corpus_bursts(S, oracle, row_env, steps_per_call):
    """sca_run_steps(3) and (12) with no host call in between, kd and AUTO: the state behind the burst, and the burst's results out of rings
    of R = 12 (every ending kept) and R = 1 (each row's last one; `ended` says how many were lost)"""
    row_env(None)
    for seed, nbr, R in ((5, S.NBR_KDTREE, 12), (12, S.NBR_AUTO, 12), (17, S.NBR_AUTO, 1), (33, S.NBR_KDTREE, 1)):
        scene = F.random_scene(seed)
        run = MR.oracle_run(oracle, scene)
        sol = context_of(S, scene)
        try:
            sol.set_missions(MR.M, R, run['entries'], run['first_ok'], run['first_fail'])
            lost = R > 1
            for t0 in range(0, MR.STEPS, steps_per_call):
                at = ('burst', steps_per_call, 'seed', seed, 'R', R, 'step', t0)
                sol.run_steps(steps_per_call, nbr)
                sol.synchronize()
                r = run['steps'][t0 + steps_per_call - 1]
                compare_with_oracle(sol, behind(r), scene, at)
                assert sol.active_count() == r['active'], at
                check_words(sol, r, at)
                want = by_row([s['results'] for s in run['steps'][t0:t0 + steps_per_call]])
                if R == 1:                                                  # a row's last result of the burst
                    last = np.concatenate([want['id'][1:] != want['id'][:-1], [True]]) if len(want) else np.zeros(0, bool)
                    lost = lost or bool((~last).any())
                    want = want[last]
                assert sol.mission_results().tobytes() == want.tobytes(), at + ('results',)
            assert lost, ('no ring overflowed', seed, R)
        finally:
            sol.close()


# ---- the twin ------------------------------------------------------------------------------------------------------------------------------
def traffic_scene(n, tracker):
    """n agents on a circle 1.5 m apart at z = 10, built so that rows end every few steps: row kinds by i % 8 --
    2, 6: the goal 0.8 m from the start (arrives); 1, 5: a max_run_dist of 25 cm (times out); 3 and 7 of one group of eight stand on the SAME
    spot (collide in the first step, and again after every explicit restart: their entry 2 starts coincide too); 0, 4: fly across.
    Tables of three entries: 0 back to the start from where the row stands (START_HERE | KEEP_ZAXIS, a short max_run_dist: arrives or times
    out), 1 to the near goal from where it stands (START_HERE, a zaxis byte of its own), 2 an explicit start with a velocity, retrying
    itself after a failure."""
    rad = max(4.0, 1.5 * n / (2 * math.pi))
    ang = 2 * math.pi * np.arange(n) / n
    kind = np.arange(n) % 8
    start = np.stack([rad * np.cos(ang), rad * np.sin(ang), np.full(n, 10.0)], 1)
    pair = (kind == 7)
    start[pair] = start[np.flatnonzero(pair) - 4]
    out = np.stack([np.cos(ang), np.sin(ang), np.zeros(n)], 1)
    near = start + 0.8 * out
    goal = np.where(np.isin(kind, (2, 6))[:, None], near, -start + [0.0, 0.0, 20.0])
    heading = np.stack([ang + math.pi, np.zeros(n), np.zeros(n)], 1)
    mrd = np.where(np.isin(kind, (1, 5)), 0.25, 3.0 * np.linalg.norm(start - goal, axis=1) + 1.0)
    policy = np.array([(0, 5, 1, 4, 3, 5, 1, 4)[i % 8] if tracker else (1, 3, 4, 4, 3, 1, 2, 4)[i % 8] for i in range(n)], np.uint8)
    e = np.zeros((n, 3), MR.MISSION)
    e['goal'][:, 0], e['goal'][:, 1], e['goal'][:, 2] = start, near, near
    e['goal_heading'][..., 0] = (ang + 0.3)[:, None] + np.arange(3)[None, :]
    e['pref_speed'] = np.array([1.0, 0.8, 1.0])[None, :]
    e['max_run_dist'] = np.array([0.35, 4.0, 4.0])[None, :]
    e['pos'][:, 2] = start + 0.05 * out
    e['heading'][:, 2] = heading + [0.1, 0.0, 0.0]
    e['vel'][:, 2] = (0.05 * out).astype(np.float32)
    e['zaxis'][:, 1] = 1
    e['flags'] = np.array([MR.START_HERE | MR.KEEP_ZAXIS, MR.START_HERE, 0], np.uint8)[None, :]
    e['next_ok'] = np.array([1, 0, 0], np.int8)[None, :]
    e['next_fail'] = np.array([2, 2, 2], np.int8)[None, :]
    return dict(n=n, start=start, goal=goal, heading=heading, mrd=mrd, policy=policy, zaxis=np.zeros(n, np.uint8), radius=np.full(n, 0.5), entries=e,
                first_ok=np.zeros(n, np.int32), first_fail=np.full(n, 2, np.int32), gh=np.stack([ang, np.zeros(n), np.zeros(n)], 1), tracker=tracker)


def context_for(S, sc, tracker_in_pass=True, clearance=False, history=0):
    n = sc['n']
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    try:
        sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
        sol.set_agents(sc['radius'], np.ones(n), sc['goal'], sc['policy'], sc['zaxis'], sc['mrd'])
        sol.set_state(sc['start'], np.zeros((n, 3), np.float32), sc['heading'], np.zeros(n, np.uint8))
        if sc['tracker']:
            sol.device_tracker_enable(sc['gh'], in_pass=tracker_in_pass)
        if clearance:
            sol.clearance_enable()
        if history:
            sol.history_enable(history)
    except BaseException:
        sol.close()
        raise
    return sol


class Twin:
    """The tables' rule done by the host on a context WITHOUT tables: behind every step sca_get_finished, and sca_respawn_agents for the rows
    that ended in the step and whose flight names a successor -- with the pos / heading sca_get_state returns for START_HERE, the row's own
    zaxis byte for KEEP_ZAXIS.  Keeps the cursors, `ended`, the results and the totals as the device should."""
    def __init__(self, sol, sc, clearance=False):
        self.sol, self.sc, n = sol, sc, sc['n']
        self.e, self.first_ok, self.first_fail = sc['entries'], sc['first_ok'], sc['first_fail']
        self.has = (self.first_ok >= 0) | (self.first_fail >= 0)
        self.cursor, self.flying, self.ended = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
        self.running = np.ones(n, bool)
        self.zaxis = sc['zaxis'].copy()
        self.totals = dict.fromkeys(MR.TOTALS, 0)
        self.clearance = clearance
        self.results = []

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
        k, ids, nxts = 0, [], []
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
            self.totals['taken' if nxt >= 0 else 'stopped'] += 1
            if nxt >= 0:
                self.cursor[a] = nxt
                ids.append(a)
                nxts.append(nxt)
        self.results.append(res)
        if ids:
            ids, nxts = np.array(ids, np.int32), np.array(nxts)
            e = self.e[ids, nxts]
            st = self.sol.get_state()
            here = ((e['flags'] & MR.START_HERE) != 0)[:, None]
            keep = (e['flags'] & MR.KEEP_ZAXIS) != 0
            self.zaxis[ids] = np.where(keep, self.zaxis[ids], e['zaxis'])
            self.sol.respawn(ids, np.where(here, st['pos'][ids], e['pos']), e['vel'], np.where(here, st['heading'][ids], e['heading']), self.sc['radius'][ids],
                             e['pref_speed'], e['goal'], e['max_run_dist'], zaxis=self.zaxis[ids], goal_heading=e['goal_heading'] if self.sc['tracker'] else None)
            self.running[ids] = True
        return res

    def host_respawn(self, ids, **m):
        """a stopped row restarted by the host, on BOTH contexts by the caller: what flies is not an entry"""
        self.flying[ids] = -1
        self.running[ids] = True


def same(A, B, tw, at, served=None, tracker=False, results=None):
    """context A (tables) against the twin's context B: the state, the permutation, sca_active_count, the finished list, the pass's results
    on the rows it served, the tracker's records and re-plan counts, cursors / ended / totals, and the results A hands out"""
    ga, gb = A.get_state(), B.get_state()
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), at + (k, np.flatnonzero((ga[k] != gb[k]).reshape(len(ga[k]), -1).any(1))[:8])
    assert np.array_equal(A.get_kd_perm(), B.get_kd_perm()), at + ('perm',)
    assert A.active_count() == B.active_count() == int(tw.running.sum()), at + ('active_count', A.active_count(), B.active_count(), int(tw.running.sum()))
    assert A.finished().tobytes() == B.finished().tobytes(), at + ('finished',)
    if served is not None:
        assert np.array_equal(A.actions()[served], B.actions()[served]), at + ('action',)
        na, nb = A.neighbors(), B.neighbors()
        for k in na:
            assert np.array_equal(na[k][served], nb[k][served]), at + ('lists', k)
        da, db = A.diag(), B.diag()
        for k in da:
            assert np.array_equal(da[k][served], db[k][served], equal_nan=da[k].dtype.kind == 'f'), at + ('diag', k)
    if tracker:
        assert np.array_equal(A.device_tracker_replans(), B.device_tracker_replans()), at + ('re-plans',)
        for i in range(tw.sc['n']):
            assert np.array_equal(A.device_tracker_debug(i), B.device_tracker_debug(i), equal_nan=True), at + ('tracker record', i)
    cursor, ended = A.mission_state()
    assert np.array_equal(cursor, tw.cursor) and np.array_equal(ended, tw.ended), at + ('cursor / ended',)
    assert A.mission_totals() == tw.totals, at + ('totals', A.mission_totals(), tw.totals)
    if results is not None:
        got = A.mission_results()
        assert got.tobytes() == results.tobytes(), at + ('results', len(got), len(results))


def run_twin(S, sc, nbr, steps, at, R=2, tracker_in_pass=True, clearance=False, check_tracker=None):
    """both contexts step by step; returns (A, B, twin) still open in a list for the caller to go on with and close"""
    A, B = context_for(S, sc, tracker_in_pass, clearance), context_for(S, sc, tracker_in_pass, clearance)
    try:
        A.set_missions(3, R, sc['entries'], sc['first_ok'], sc['first_fail'])
        tw = Twin(B, sc, clearance)
        for t in range(steps):
            served = tw.running.copy()
            A.run_steps(1, nbr)
            res = tw.step(nbr)
            same(A, B, tw, at + ('step', t), served, sc['tracker'] if check_tracker is None else check_tracker, res)
    except BaseException:
        A.close()
        B.close()
        raise
    return A, B, tw


@pytest.mark.parametrize('n,mode', [(48, 'kd'), (64, 'kd'), (33, 'auto')])
def test_twin_with_the_device_tracker(S, row_env, n, mode):
    """tracked rows (SCA / RVO3D+Dubins) among RVO3D, ORCA3D and ORCA3D-LP rows, the tracker inside the pass: a taken tracked row starts from
    the initial tracker record with the entry's goal heading, as under sca_respawn_agents; every row's plan (sca_device_tracker_debug) and
    re-plan count equal the twin's after every step; closest-approach records on: a result carries the record the twin reads
    (sca_get_clearance) before its respawn"""
    row_env(None)
    sc = traffic_scene(n, True)
    A, B, tw = run_twin(S, sc, S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE, 14, ('tracker', n, mode), clearance=mode == 'kd')
    try:
        t = tw.totals
        assert t['arrived'] > 0 and t['collided'] > 0 and t['timed_out'] > 0 and t['taken'] > n // 2, t
        took = by_row(tw.results)
        took = took[took['next'] >= 0]
        assert np.isin(sc['policy'][took['id']], (0, 5)).any() and (sc['policy'][took['id']] == 4).any()
        assert (took['next'] == took['entry']).any()                        # a retry chain: the coincident rows collide again after every restart
        if mode == 'kd':
            assert np.isfinite(by_row(tw.results)['clear']['agent_clear']).any()
            assert np.array_equal(A.clearance(), B.clearance())
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_twin_sizes(S, row_env, n):
    """one row, one wavefront less one, exactly one, one more, and more than one workgroup"""
    row_env(None)
    sc = traffic_scene(n, False)
    sc['mrd'][0] = 0.25                                                    # (n = 1: the one row times out, restarts, arrives)
    A, B, tw = run_twin(S, sc, S.NBR_KDTREE, 8, ('size', n))
    try:
        assert tw.totals['taken'] > 0
        assert tw.totals['arrived'] + tw.totals['collided'] + tw.totals['timed_out'] > 0
    finally:
        A.close()
        B.close()


def edge_scene(n, count):
    """n rows on a grid 3 m apart that fly 30 m up; `count` of them end in the FIRST step: coincident pairs placed by hand (rows 2k and 2k + 1
    on one spot), and, for an odd count, one row whose goal is 0.3 m from its start.  Every row's table: restart 1.5 m above its grid point
    (explicit), retrying after a failure, going on from where it stands after an arrival."""
    side = int(math.ceil(math.sqrt(n)))
    i = np.arange(n)
    grid = np.stack([3.0 * (i % side), 3.0 * (i // side), np.full(n, 10.0)], 1)
    start = grid.copy()
    goal = grid + [0.0, 0.0, 30.0]
    pairs = count // 2
    start[1:2 * pairs:2] = start[0:2 * pairs:2]
    if count % 2:
        goal[2 * pairs] = start[2 * pairs] + [0.3, 0.0, 0.0]
    e = np.zeros((n, 2), MR.MISSION)
    e['pos'][:, 0], e['goal'][:, 0] = grid + [0.0, 0.0, 1.5], goal
    e['goal'][:, 1] = grid + [0.0, 0.0, 20.0]
    e['pref_speed'], e['max_run_dist'] = 1.0, 200.0
    e['flags'][:, 1] = MR.START_HERE
    e['next_ok'], e['next_fail'] = np.array([1, 0], np.int8)[None, :], np.array([0, 0], np.int8)[None, :]
    return dict(n=n, start=start, goal=goal, heading=np.zeros((n, 3)), mrd=np.full(n, 200.0), policy=np.array([(1, 3, 4)[k % 3] for k in range(n)], np.uint8),
                zaxis=np.zeros(n, np.uint8), radius=np.full(n, 0.5), entries=e, first_ok=np.ones(n, np.int32), first_fail=np.zeros(n, np.int32), gh=np.zeros((n, 3)), tracker=False)


@pytest.mark.parametrize('n,count', [(n, c) for n in (2049, 6145) for c in (0, 1, 63, 64, 65, -1)])
def test_twin_form_switches(S, row_env, n, count):
    """2049 / 6145 rows (the sizes at which the passes change form) with 0, 1, 63, 64, 65 and all rows ending in one step"""
    row_env(None)
    k = n if count < 0 else count
    sc = edge_scene(n, k)
    A = B = None
    try:
        A, B = context_for(S, sc), context_for(S, sc)
        A.set_missions(2, 1, sc['entries'], sc['first_ok'], sc['first_fail'])
        tw = Twin(B, sc)
        for t in range(3):
            served = tw.running.copy()
            A.run_steps(1, S.NBR_KDTREE)
            res = tw.step(S.NBR_KDTREE)
            if t == 0:
                assert len(res) == k and (res['next'] >= 0).all(), (n, count, len(res))
            same(A, B, tw, ('edge', n, count, 'step', t), served, False, res)
    finally:
        for s in (A, B):
            if s is not None:
                s.close()


@pytest.mark.parametrize('form', ['env_step', 'pass_update', 'run1', 'run3', 'run12'])
@pytest.mark.parametrize('mode', ['kd', 'auto'])
def test_step_forms(S, row_env, form, mode):
    """sca_env_step, sca_policy_pass + sca_env_update, sca_run_steps(1), (3) and (12) with no host call in between: all equal the stepwise
    twin (with the tracker in the pass: the fork must not ride on a step whose last kernel may still replace tracker records)"""
    row_env(None)
    nbr = S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE
    sc = traffic_scene(96, True)
    A = B = None
    try:
        A, B = context_for(S, sc), context_for(S, sc)
        A.set_missions(3, 12, sc['entries'], sc['first_ok'], sc['first_fail'])
        tw = Twin(B, sc)
        per = dict(run3=3, run12=12).get(form, 1)
        for t0 in range(0, 12, per):
            if form == 'env_step':
                active = A.env_step(nbr)
            elif form == 'pass_update':
                A.policy_pass(nbr)
                with pytest.raises(S.ScaError, match='between a policy pass'):
                    A.set_missions(3, 12, sc['entries'], sc['first_ok'], sc['first_fail'])
                A.env_update()
                active = A.active_count()
            else:
                A.run_steps(per, nbr)
                active = A.active_count()
            served = tw.running.copy()
            res = by_row([tw.step(nbr) for _ in range(per)])
            assert active == int(tw.running.sum()), (form, mode, t0)
            same(A, B, tw, (form, mode, 'step', t0), served if per == 1 else None, True, res)
        assert tw.totals['taken'] > 48
    finally:
        for s in (A, B):
            if s is not None:
                s.close()


def test_m1_r1_stop_and_host_respawn(S, row_env):
    """M = 1 and R = 1: one entry that retries itself after a failure and stops after an arrival; rows without a table among them end and
    stay; a stopped row respawned by the host (on both contexts) flies a flight that is not an entry (-1 in its result), ends again and
    follows the same successors; sca_set_state under standing tables leaves tables and cursors alone; dropping the tables: the context
    steps on as one without, the getters refuse"""
    row_env(None)
    sc = traffic_scene(80, False)
    sc['entries'] = sc['entries'][:, 2:3].copy()
    sc['entries']['next_ok'], sc['entries']['next_fail'] = -1, 0
    sc['entries']['goal'][:, 0] = sc['entries']['pos'][:, 0] + [0.7, 0.0, 0.0]          # arrives two or three steps after the explicit restart
    sc['first_ok'], sc['first_fail'] = np.zeros(80, np.int32), np.zeros(80, np.int32)
    sc['first_ok'][::5] = sc['first_fail'][::5] = -1                       # no table
    A = B = None
    try:
        A, B = context_for(S, sc), context_for(S, sc)
        A.set_missions(1, 1, sc['entries'], sc['first_ok'], sc['first_fail'])
        tw = Twin(B, sc)
        nbr = S.NBR_KDTREE
        for t in range(10):
            served = tw.running.copy()
            A.run_steps(1, nbr)
            res = tw.step(nbr)
            same(A, B, tw, ('m1r1', 'step', t), served, False, res)
        stopped = np.flatnonzero(~tw.running & tw.has & (tw.ended > 0))[:6].astype(np.int32)
        assert len(stopped) == 6 and tw.totals['stopped'] > 6 and (~tw.has & ~tw.running).any()
        # ... and two rows that still FLY an entry (the pairs that collide again after every restart): theirs is the host's flight too
        flying = np.flatnonzero(tw.running & (tw.flying >= 0))[:2].astype(np.int32)
        assert len(flying) == 2
        stopped = np.concatenate([stopped, flying])
        k = len(stopped)
        lift = np.concatenate([np.full(6, 2.0), [4.0, 5.5]])[:, None] * [0.0, 0.0, 1.0]
        m = dict(pos=sc['start'][stopped] + lift, vel=np.zeros((k, 3), np.float32), heading=sc['heading'][stopped], radius=np.full(k, 0.5), pref_speed=np.ones(k),
                 goal=sc['start'][stopped] + lift + [0.6, 0.0, 0.0], max_run_dist=np.full(k, 9.0))
        for sol in (A, B):
            sol.respawn(stopped, m['pos'], m['vel'], m['heading'], m['radius'], m['pref_speed'], m['goal'], m['max_run_dist'])
        tw.host_respawn(stopped)
        seen = []
        for t in range(10, 16):
            served = tw.running.copy()
            A.run_steps(1, nbr)
            res = tw.step(nbr)
            seen.append(res)
            same(A, B, tw, ('m1r1', 'step', t), served, False, res)
        again = by_row(seen)
        again = again[np.isin(again['id'], stopped)]
        assert np.isin(stopped, again['id']).all() and (again['entry'][np.unique(again['id'], return_index=True)[1]] == -1).all(), again
        # a new state under standing tables
        g = A.get_state()
        g['flags'][:] = 0
        for sol in (A, B):
            sol.set_state(g['pos'], g['vel'], g['heading'], g['flags'], g['total_dist'], g['step_num'])
        tw.running[:] = True
        cursor, ended = A.mission_state()
        assert np.array_equal(cursor, tw.cursor) and np.array_equal(ended, tw.ended)
        for t in range(16, 19):
            A.run_steps(1, nbr)
            res = tw.step(nbr)
            same(A, B, tw, ('m1r1', 'step', t), None, False, res)
        # dropping the tables: A runs on as a context without; the rows that end now stay finished in both
        A.set_missions(0, 0, None, None, None)
        with pytest.raises(S.ScaError, match='no mission tables'):
            A.mission_totals()
        with pytest.raises(S.ScaError, match='no mission tables'):
            A.mission_results()
        for t in range(3):
            A.run_steps(1, nbr)
            B.run_steps(1, nbr)
        ga, gb = A.get_state(), B.get_state()
        for key in ga:
            assert np.array_equal(ga[key], gb[key]), ('dropped', key)
        assert A.active_count() == B.active_count()
    finally:
        for s in (A, B):
            if s is not None:
                s.close()


def test_trajectory_log_goes_on(S, row_env):
    """the log's rows of the steps in front of and behind a device-side respawn equal the twin's"""
    row_env(None)
    sc = traffic_scene(40, False)
    A = B = None
    try:
        A, B = context_for(S, sc, history=16), context_for(S, sc, history=16)
        A.set_missions(3, 2, sc['entries'], sc['first_ok'], sc['first_fail'])
        tw = Twin(B, sc)
        for t in range(10):
            A.run_steps(1, S.NBR_KDTREE)
            tw.step(S.NBR_KDTREE)
        assert tw.totals['taken'] > 10
        ha, hb = A.history(), B.history()
        for k in ha:
            assert np.array_equal(ha[k], hb[k], equal_nan=np.asarray(ha[k]).dtype.kind == 'f'), k
    finally:
        for s in (A, B):
            if s is not None:
                s.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def snapshot(sol, missions=True, plain=True):
    """plain=False: the context holds something tables exclude (lists, a shard, the partition, scenes), under which sca_get_finished is
    refused itself -- the copies of the state, the permutation, the lists and the diagnostics are taken all the same"""
    out = dict(sol.get_state())
    out['perm'] = sol.get_kd_perm()
    out.update({'nbr_' + k: v for k, v in sol.neighbors().items()})
    out.update({'diag_' + k: v for k, v in sol.diag().items()})
    if plain:
        out['active'] = np.array([sol.active_count()])
        out['finished'] = sol.finished()
    if missions:
        out['cursor'], out['ended'] = sol.mission_state()
        out['totals'] = np.array(list(sol.mission_totals().values()))
    return out


def test_refusals_change_nothing_in_either_order(S, oracle, row_env):
    """every refusal with its code, decided before any device work -- sca_set_missions where something it excludes stands, and the entry
    points that would bring such a thing while tables stand; the state, the cursors and the totals are the same before and after.
    The communicator: sca_comm_init while tables stand is refused before the collective library is loaded, so one GPU shows it; the other
    order -- sca_set_missions under a communicator -- needs a real communicator of several ranks and is covered by the rule alone
    (mission_check's `comm` outcome, tests/test_missions_cpu.py)"""
    import sca_amd._lib as _lib
    row_env(None)
    scene = F.random_scene(5)                                               # (257 rows, a hundred endings in every step)
    n = scene['n']
    run = MR.oracle_run(oracle, scene)
    ent, fok, ffail = run['entries'], run['first_ok'], run['first_fail']
    ip = lambda a: None if a is None else _lib.ptr(a, C.c_int32)

    def raw(sol, M=MR.M, R=2, n_=n, entries=ent, first_ok=fok, first_fail=ffail):
        e = None if entries is None else np.ascontiguousarray(entries).reshape(-1)
        rc = sol.L.sca_set_missions(sol.ctx, M, R, n_, None if e is None else e.ctypes.data_as(C.POINTER(_lib.Mission)), ip(first_ok), ip(first_fail))
        return rc, sol.L.sca_last_error(sol.ctx).decode()

    def unchanged(sol, before, what, missions=True, plain=True):
        after = snapshot(sol, missions, plain)
        for k in before:
            assert np.array_equal(before[k], after[k], equal_nan=before[k].dtype.kind == 'f'), (what, k)
    sol = S.BatchedSolver(max_agents=n, max_obstacles=max(1, scene['m']))
    try:
        assert raw(sol)[0] == ERR_STATE                                     # no agents
        t = _lib.MissionTotals()
        assert sol.L.sca_get_mission_totals(sol.ctx, C.byref(t), 64) == ERR_STATE
    finally:
        sol.close()
    # A: no tables yet -- sca_set_missions is the one refused
    sol = context_of(S, scene)
    try:
        sol.run_steps(2, S.NBR_KDTREE)
        sol.synchronize()
        before = snapshot(sol, False)

        def edited(key, value, at=(3, 1)):
            e = ent.copy()
            e[key][at] = value
            f = fok.copy()
            f[at[0]] = at[1]                                               # (reachable)
            return dict(entries=e, first_ok=f)
        cases = [('M 0', dict(M=0), ERR_ARG), ('M 128', dict(M=128), ERR_ARG), ('R 0', dict(R=0), ERR_ARG), ('R 65537', dict(R=65537), ERR_ARG), ('n', dict(n_=n - 1), ERR_ARG),
                 ('NULL entries', dict(entries=None), ERR_ARG), ('NULL first_ok', dict(first_ok=None), ERR_ARG), ('NULL first_fail', dict(first_fail=None), ERR_ARG),
                 ('first_ok 3', dict(first_ok=np.where(np.arange(n) == 2, 3, fok).astype(np.int32)), ERR_ARG),
                 ('first_fail -2', dict(first_fail=np.where(np.arange(n) == 2, -2, ffail).astype(np.int32)), ERR_ARG),
                 ('next_ok 3', edited('next_ok', 3), ERR_ARG), ('next_fail -2', edited('next_fail', -2), ERR_ARG),
                 ('nan goal', edited('goal', np.nan), ERR_ARG), ('inf vel', edited('vel', np.inf), ERR_ARG),
                 ('nan pos', dict(edited('pos', np.nan), **{}), ERR_ARG), ('pref_speed 0', edited('pref_speed', 0.0), ERR_ARG),
                 ('max_run_dist inf', edited('max_run_dist', np.inf), ERR_ARG), ('flags 4', edited('flags', 4), ERR_ARG)]
        cases[14][1]['entries']['flags'][3, 1] = 0                          # (an explicit start: its position is read)
        z = edited('zaxis', 2)
        z['entries']['flags'][3, 1] = MR.START_HERE
        cases.append(('zaxis 2', z, ERR_ARG))
        for what, kw, code in cases:
            rc, msg = raw(sol, **kw)
            assert rc == code and 'sca_set_missions' in msg, (what, rc, msg)
            unchanged(sol, before, what, False)
        for name, args in (('sca_get_mission_totals', (C.byref(_lib.MissionTotals()), 64)), ('sca_get_mission_state', (0, 0, None, None))):
            assert getattr(sol.L, name)(sol.ctx, *args) == ERR_STATE, name       # no tables
        sol.policy_pass(S.NBR_KDTREE)
        assert raw(sol)[0] == ERR_STATE                                     # between a policy pass and its env update
        sol.env_update()
        sol.synchronize()
        before = snapshot(sol, False)
        for what, setup, undo, word in (('lists, block form', lambda: sol.set_paths([[] for _ in range(n - 1)] + [[[1.0, 2.0, 3.0]]]), lambda: sol.set_paths(None), 'waypoint'),
                                        ('lists, slot form', lambda: sol.set_path_slots(2), lambda: sol.set_paths(None), 'waypoint'),
                                        ('shard', lambda: sol.set_shard(0, n - 1), lambda: sol.set_shard(0, n), 'shard'),
                                        ('partition', lambda: sol.partition_init(0, 1), lambda: sol.partition_disable(), 'partition'),
                                        ('scenes', lambda: sol.set_scenes([0, n // 2, n]), lambda: sol.set_scenes(None), 'scenes')):
            setup()
            standing = snapshot(sol, False, False)
            rc, msg = raw(sol)
            assert rc == ERR_UNSUPPORTED and word in msg, (what, rc, msg)
            unchanged(sol, standing, what, False, False)                    # the refused call left the context as it stood
            for name, args in (('sca_get_mission_totals', (C.byref(_lib.MissionTotals()), 64)), ('sca_get_mission_state', (0, 0, None, None))):
                assert getattr(sol.L, name)(sol.ctx, *args) == ERR_STATE, (what, name)   # ... and no tables
            undo()
            if what == 'shard':
                unchanged(sol, before, 'lists and a shard', False)
    finally:
        sol.close()
    # B: tables stand -- the entry points that would bring what they exclude are refused, and the getters' own arguments
    sol = context_of(S, scene)
    try:
        sol.set_missions(MR.M, 2, ent, fok, ffail)
        sol.run_steps(2, S.NBR_KDTREE)
        sol.synchronize()
        sol.mission_results()
        before = snapshot(sol)
        for what, call, word in (('sca_set_paths', lambda: sol.set_paths([[] for _ in range(n - 1)] + [[[1.0, 2.0, 3.0]]]), 'waypoint'),
                                 ('sca_set_path_slots', lambda: sol.set_path_slots(2), 'waypoint'),
                                 ('sca_set_shard', lambda: sol.set_shard(0, n - 1), 'shard'),
                                 ('sca_partition_init', lambda: sol.partition_init(0, 1), 'partition'),
                                 ('sca_set_scenes', lambda: sol.set_scenes([0, n // 2, n]), 'scenes'),
                                 ('sca_step_host', lambda: sol.step_host(S.NBR_KDTREE, state=False), 'host owns the state')):
            with pytest.raises(S.ScaError, match=word) as ei:
                call()
            assert '(rc=%d)' % ERR_UNSUPPORTED in str(ei.value) and what in str(ei.value), (what, str(ei.value))
            unchanged(sol, before, what)
        uid = (C.c_char * 128)()                                            # (never read: the call is refused in front of the library's load)
        assert sol.L.sca_comm_init(sol.ctx, 0, 1, uid) == ERR_UNSUPPORTED
        msg = sol.L.sca_last_error(sol.ctx).decode()
        assert 'sca_comm_init' in msg and 'communicator' in msg and 'mission tables' in msg, msg
        unchanged(sol, before, 'sca_comm_init')
        assert sol.L.sca_set_path_slots(sol.ctx, -1, n, None, None) == ERR_ARG      # (the call's own argument fault, tables or not)
        unchanged(sol, before, 'sca_set_path_slots -1')
        out = np.zeros(4, _lib.MISSION_RESULT_DTYPE)
        op, cnt = out.ctypes.data_as(C.POINTER(_lib.MissionResult)), C.c_int(0)
        for args in ((op, -1, C.byref(cnt), 96), (op, 4, None, 96), (None, 4, C.byref(cnt), 96), (op, 4, C.byref(cnt), 88), (op, 4, C.byref(cnt), 104)):
            assert sol.L.sca_get_mission_results(sol.ctx, *args) == ERR_ARG, args[1:]
        t = _lib.MissionTotals()
        for args in ((None, 64), (C.byref(t), 56), (C.byref(t), 72)):
            assert sol.L.sca_get_mission_totals(sol.ctx, *args) == ERR_ARG, args[1:]
        w = np.zeros(n, np.int32)
        for args in ((-1, 1, ip(w), ip(w)), (0, n + 1, ip(w), ip(w)), (n, 1, ip(w), ip(w)), (0, 4, None, ip(w)), (0, 4, ip(w), None)):
            assert sol.L.sca_get_mission_state(sol.ctx, *args) == ERR_ARG, args[:2]
        unchanged(sol, before, 'getters')
        # results that do not fit are neither handed out nor marked
        sol.run_steps(3, S.NBR_KDTREE)
        sol.synchronize()
        part = sol.mission_results(capacity=1)
        total = sol.mission_result_count
        assert total > 1 and len(part) == 0
        assert len(sol.mission_results()) == total and len(sol.mission_results()) == 0
        # the envelope: a table whose reachable entries are faster than every agent still steps to the oracle's values (run_corpus) -- here
        # only that a second sca_set_missions replaces the first and starts the counters again
        sol.set_missions(MR.M, 2, ent, fok, ffail)
        assert sol.mission_totals() == dict.fromkeys(MR.TOTALS, 0) and not sol.mission_state()[1].any()
    finally:
        sol.close()


# ---- the Python layers -------------------------------------------------------------------------------------------------------------------
def test_run_missions_against_run_lifelong(S, row_env):
    """32 drones on the example's circle with obstacles, 600 steps of the ping-pong rule: run_missions at burst 1 and 8 gives the same stats
    and final state as run_lifelong driven by the same rule"""
    from sca_amd import env as E
    from sca_amd.lifelong import run_lifelong, run_missions
    row_env(None)
    n = 32

    def world():
        agents = E.build_circle_agents(n, policy=E.RVO3DPolicy, rad=8.0)
        obstacles = [E.Obstacle(pos=[round(2.5 * math.cos(2 * j * math.pi / 8), 2), round(2.5 * math.sin(2 * j * math.pi / 8), 2), 10.0],
                                shape_dict={'shape': 'sphere', 'feature': 0.3}, id=j) for j in range(8)]
        env = E.MACAEnv()
        env.set_agents(agents, obstacles=obstacles)
        first = {a.id: (list(a.initial_pos), list(a.goal_pos)) for a in agents}
        return env, first

    def agent(i, start, goal):
        return E.Agent(start_pos=list(start), goal_pos=list(goal), vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=E.RVO3DPolicy, id=i)

    def tables(first):
        """here -> start, here -> goal, and the explicit start -> goal as every failure's successor"""
        out = {}
        for i, (start, goal) in first.items():
            out[i] = E.MissionTable([agent(i, goal, start), agent(i, start, goal), agent(i, start, goal)], next_ok=[1, 0, 0], next_fail=[2, 2, 2], first_ok=0, first_fail=2,
                                    start_here=[True, True, False])
        return out
    env, first = world()
    T = tables(first)
    state = {i: -1 for i in first}                                          # the entry a row flies, as the tables would have it

    def next_mission(a, row):
        f = int(row['flags'])
        arrived = bool(f & 1) and not f & 2
        j = (T[a.id].first_ok if arrived else T[a.id].first_fail) if state[a.id] < 0 else (T[a.id].next_ok[state[a.id]] if arrived else T[a.id].next_fail[state[a.id]])
        state[a.id] = j
        src, here, _ = T[a.id].entries[j]
        start = list(row['pos']) + list(a.heading_global_frame) if here else list(src.initial_pos)
        new = agent(a.id, start, src.goal_pos)
        new.max_run_dist = src.max_run_dist
        return new
    want = run_lifelong(env, next_mission, 600)
    want_state = env.solver.get_state()
    assert want['respawned'] >= n and want['retired'] == 0, want
    for burst in (1, 8):
        env2, first2 = world()
        seen = []
        got = run_missions(env2, tables(first2), 600, burst=burst, on_result=lambda a, r: seen.append((a.id, int(r['next']))))
        assert got == want, (burst, got, want)
        g = env2.solver.get_state()
        for k in want_state:
            assert np.array_equal(g[k], want_state[k]), (burst, k)
        assert len(seen) == want['respawned'] and all(env2.agents[i].id == i for i, _ in seen)
        last = {}
        for i, j in seen:
            last[i] = j
        for i, j in last.items():                                           # the goal mirrors follow the entry the row flies now
            assert np.array_equal(env2.agents[i].goal_global_frame, T[i].entries[j][0].goal_global_frame), (burst, i, j)
