"""Respawning agents in place (sca_respawn_agents, sca_get_finished) on the GPU against the oracle (-m gpu).  Equality, no tolerance.

The corpus is tests/respawn_rule.py's: the fuzz scenes of tests/form_fuzz.py (1 .. 1600 agents, obstacles, six policies, agents done from
the start) stepped free-running while, before every step, each finished row gets a new mission with probability 0.5 -- respawned rows
collide, arrive and are respawned again.  After every step state, action rows, lists entry for entry, diag, the permutation,
sca_active_count and sca_get_finished equal the oracle's."""
import ctypes as C
import os

import numpy as np
import pytest

import form_fuzz as F
import respawn_rule as RR
from test_gpu_form_fuzz import check_paths, compare_with_oracle, context_of

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


def respawn(sol, m, **kw):
    sol.respawn(m['ids'], m['pos'], m['vel'], m['heading'], m['radius'], m['pref_speed'], m['goal'], m['max_run_dist'], **kw)


def check_finished(sol, r, at):
    """sca_get_finished against np.flatnonzero of the oracle's flags, with the rows' step_num / total_dist / pos"""
    fin = sol.finished()
    want = r['finished']
    assert sol.finished_count == len(want) and np.array_equal(fin['id'], want), at + ('finished ids', sol.finished_count, len(want))
    assert np.array_equal(fin['flags'], r['flags'][want]) and np.array_equal(fin['step_num'], r['step_num'][want]), at + ('finished flags / step_num',)
    assert np.array_equal(fin['total_dist'], r['total_dist'][want]) and np.array_equal(fin['pos'], r['pos'][want]), at + ('finished total_dist / pos',)
    assert not fin['reserved'].any()


def run_corpus(S, oracle, scene, nbr, ctx, steps=RR.STEPS):
    """one context through the scene's run with respawns; compare_with_oracle reads the scene's policies only, which never change"""
    ref = RR.oracle_run(oracle, scene, steps)
    sol = context_of(S, scene)
    try:
        for t, r in enumerate(ref):
            at = ctx + ('n', scene['n'], 'step', t)
            if r['mission'] is not None:
                respawn(sol, r['mission'])
                if t > 0:                                                   # (directly behind set_state the counters are not counted yet)
                    assert sol.active_count() == r['active_before'], at + ('active_count behind the respawn', sol.active_count(), r['active_before'])
            sol.run_steps(1, nbr)
            sol.synchronize()
            compare_with_oracle(sol, r, scene, at)
            assert sol.active_count() == scene['n'] - len(r['finished']), at + ('active_count',)
            check_finished(sol, r, at)
    finally:
        sol.close()


# ---- the corpus --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('block', range(4))
def test_corpus_kd_default_forms(S, oracle, row_env, block):
    """kd mode, default forms, all 40 seeds (1 .. 1600 agents), 12 steps with respawns before every one"""
    row_env(None)
    for seed in RR.SEEDS[10 * block:10 * block + 10]:
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_KDTREE, ('kd', 'seed', seed))


@pytest.mark.parametrize('row,mode,block', [(row, mode, b) for b in range(2) for row, mode in ((None, 'auto'), ('large_shard', 'kd'), ('large_shard', 'auto'))])
def test_corpus_auto_and_large_shard(S, oracle, row_env, row, mode, block):
    """SCA_NBR_AUTO and the forms every large shard runs (packed K1, two-launch solve, fallback launches) on the first 20 seeds"""
    row_env(row)
    for seed in RR.SEEDS[10 * block:10 * block + 10]:
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE, (row, mode, 'seed', seed))


# ---- form switches -------------------------------------------------------------------------------------------------------------------------
def mission_for(scene, ids, seed):
    """a mission for exactly the rows `ids`, drawn as the corpus draws its missions"""
    flags = np.zeros(scene['n'], np.uint8)
    flags[ids] = 1

    class All:                                                             # every named row is taken
        def __init__(self, rng):
            self.rng = rng

        def random(self, n):
            return np.zeros(n)

        def __getattr__(self, k):
            return getattr(self.rng, k)
    return RR.draw(All(np.random.default_rng(seed)), flags, RR.box_of(scene))


@pytest.mark.parametrize('n,count', [(n, c) for n in (2049, 6145) for c in (1, 63, 64, 65, 0)])
def test_form_switches(S, oracle, row_env, n, count):
    """switch_scene(2049) and (6145) -- either side of k_solve_fb's and the packed K1's thresholds -- 3 steps, naming 1, 63, 64, 65 rows and
    all rows (count 0) before every step: against the oracle stepped from the merged state"""
    row_env(None)
    scene = F.switch_scene(n)
    zaxis = F.zaxis_of(scene)
    count = count or n
    rng = np.random.default_rng(n + count)
    st = dict(pos=scene['pos'].copy(), vel=scene['vel'].copy(), heading=scene['heading'].copy(), flags=scene['flags'].copy(), total_dist=np.zeros(n),
              step_num=np.zeros(n, np.int32))
    defs = {k: np.array(scene[k], np.float64, copy=True) for k in RR.DEF_KEYS}
    perm = np.arange(n, dtype=np.int32)
    sol = context_of(S, scene)
    try:
        for t in range(3):
            ids = np.sort(rng.choice(n, count, replace=False)).astype(np.int32)
            m = mission_for(scene, ids, 100 * n + 10 * count + t)
            assert np.array_equal(m['ids'], ids)
            RR.apply(st, defs, m)
            respawn(sol, m)
            r = oracle.policy_step(st['pos'], st['vel'], st['heading'], defs['radius'], defs['pref_speed'], st['flags'], defs['goal'], scene['policy'], zaxis,
                                   scene['vpref'], scene['vmode'], perm, scene['obs_pos'], scene['obs_radius'], nthreads=8)
            perm = r['perm']
            u = oracle.env_update(st['pos'], st['vel'], st['heading'], defs['radius'], r['flags'], defs['goal'], r['action'], st['total_dist'],
                                  defs['max_run_dist'], st['step_num'], scene['obs_pos'], scene['obs_radius'])
            st = {k: u[k] for k in F.STATE_KEYS}
            r.update(st)
            r['finished'] = np.flatnonzero((st['flags'] & 7) != 0)
            sol.run_steps(1, S.NBR_KDTREE)
            sol.synchronize()
            at = ('switch', n, 'rows', count, 'step', t)
            compare_with_oracle(sol, r, scene, at)
            check_finished(sol, r, at)
    finally:
        sol.close()


# ---- a fresh context is the same --------------------------------------------------------------------------------------------------------
def test_fresh_context_equivalence(S, oracle, row_env):
    """An untracked scene: respawn at step 4 in context A; context B is made fresh from the merged definition + set_state + set_kd_perm.
    A and B are bit for bit equal for 6 more steps: state, actions, lists, diag, status, permutation."""
    row_env(None)
    scene = F.random_scene(5)                                               # 257 agents, 30 obstacles, all six policies
    n = scene['n']
    ref = RR.oracle_run(oracle, scene, 5)
    a = context_of(S, scene)
    b = None
    try:
        for r in ref[:4]:
            if r['mission'] is not None:
                respawn(a, r['mission'])
            a.run_steps(1, S.NBR_KDTREE)
        m = ref[4]['mission']
        assert m is not None and len(m['ids']) > 3
        before = a.get_state()
        perm = a.get_kd_perm()
        respawn(a, m)
        defs = ref[4]['defs']
        merged = dict(scene, **{k: defs[k] for k in RR.DEF_KEYS})
        b = S.BatchedSolver(max_agents=n, max_obstacles=max(1, scene['m']))
        b.set_obstacles(scene['obs_pos'], scene['obs_radius'])
        b.set_agents(merged['radius'], merged['pref_speed'], merged['goal'], scene['policy'], F.zaxis_of(scene), merged['max_run_dist'])
        b.set_vpref(scene['vpref'], scene['vmode'])
        st = {k: before[k].copy() for k in F.STATE_KEYS}
        RR.apply(st, {k: defs[k].copy() for k in RR.DEF_KEYS}, m)
        b.set_state(st['pos'], st['vel'], st['heading'], st['flags'], st['total_dist'], st['step_num'])
        b.set_kd_perm(perm)
        ga = a.get_state()
        for k in F.STATE_KEYS:
            assert np.array_equal(ga[k], st[k]), ('behind the respawn', k)
        for t in range(6):
            a.run_steps(1, S.NBR_KDTREE)
            b.run_steps(1, S.NBR_KDTREE)
            ga, gb = a.get_state(), b.get_state()
            for k in F.STATE_KEYS:
                assert np.array_equal(ga[k], gb[k]), (t, k)
            assert np.array_equal(a.get_kd_perm(), b.get_kd_perm()) and np.array_equal(a.actions(), b.actions()), t
            na, nb = a.neighbors(), b.neighbors()
            served = na['nbr_valid'].astype(bool)                          # (rows no pass of B has served hold nothing: A's hold an earlier pass's)
            assert np.array_equal(na['nbr_valid'], nb['nbr_valid']) and np.array_equal(na['nbr_n'], nb['nbr_n']), t
            in_list = served[:, None] & (np.arange(S.K)[None, :] < na['nbr_n'][:, None])
            for k in ('nbr_id', 'nbr_kind', 'nbr_dsq'):
                assert np.array_equal(na[k][in_list], nb[k][in_list]), (t, k)
            da, db = a.diag(), b.diag()
            assert np.array_equal(da['status'], db['status']), t
            for k in ('diag', 'vpref'):
                assert np.array_equal(da[k][served], db[k][served], equal_nan=True), (t, k)
            assert a.active_count() == b.active_count()
    finally:
        a.close()
        if b is not None:
            b.close()


# ---- the finished list -------------------------------------------------------------------------------------------------------------------
def test_finished_list_sizes_and_capacity(S, row_env):
    """the ordered compaction at sizes around the 256-row tile and the 64-lane wavefront: nobody finished, everybody, random sets; with a
    capacity below the count the first `capacity` rows are written and the count is still the whole number"""
    row_env(None)
    rng = np.random.default_rng(7)
    for n in (1, 63, 64, 65, 255, 256, 257, 1000, 70000):
        sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
        try:
            sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
            sol.set_agents(np.full(n, 0.5), 1.0, rng.uniform(-5, 5, (n, 3)), 3)
            pos = rng.uniform(-50, 50, (n, 3))
            td, sn = rng.uniform(0, 9, n), rng.integers(0, 99, n).astype(np.int32)
            for kind in ('none', 'all', 'random', 'sparse'):
                flags = {'none': np.zeros(n), 'all': rng.choice([1, 2, 4, 3], n), 'random': (rng.random(n) < 0.5) * rng.choice([1, 2, 4], n),
                         'sparse': (rng.random(n) < 0.01) * 2}[kind].astype(np.uint8)
                sol.set_state(pos, np.zeros((n, 3), np.float32), np.zeros((n, 3)), flags, td, sn)
                want = np.flatnonzero(flags)
                for cap in (None, 0, 1, len(want) // 2, len(want) + 5):
                    fin = sol.finished(cap)
                    k = len(want) if cap is None else min(cap, len(want))
                    assert sol.finished_count == len(want) and len(fin) == k, (n, kind, cap)
                    assert np.array_equal(fin['id'], want[:k]) and np.array_equal(fin['flags'], flags[want[:k]]), (n, kind, cap)
                    assert np.array_equal(fin['pos'], pos[want[:k]]) and np.array_equal(fin['total_dist'], td[want[:k]]), (n, kind, cap)
                    assert np.array_equal(fin['step_num'], sn[want[:k]]), (n, kind, cap)
        finally:
            sol.close()


# ---- the other neighbour modes -----------------------------------------------------------------------------------------------------------
def test_corpus_hostbuild(S, oracle, row_env):
    """SCA_NBR_KDTREE_HOSTBUILD: the host builds the tree from positions it fetches -- the mirror it kept is invalid behind a respawn"""
    row_env(None)
    for seed in (3, 5, 12):
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_KDTREE_HOSTBUILD, ('hostbuild', 'seed', seed), steps=6)


def test_corpus_grid(S, oracle, row_env):
    """SCA_NBR_GRID against the oracle under list rule 1 (the lists the grid documents), on the scenes the grid takes: a scene it refuses
    (more objects in a cell's reach than it lists) ends at the refusal"""
    from test_gpu_grid_fuzz import compare_grid_step
    row_env(None)
    whole = 0
    for seed in RR.SEEDS[:20]:
        scene = F.random_scene(seed)
        ref = RR.oracle_run(oracle, scene, 6, list_rule=1)
        sol = context_of(S, scene, perm=False)
        try:
            for t, r in enumerate(ref):
                at = ('grid', 'seed', seed, 'step', t)
                if r['mission'] is not None:
                    respawn(sol, r['mission'])
                try:
                    sol.run_steps(1, S.NBR_GRID)
                except S.ScaError as e:
                    assert 'SCA_NBR_GRID needs' in str(e), at + (str(e),)
                    break
                sol.synchronize()
                compare_grid_step(sol, r, scene, at)
                check_finished(sol, r, at)
            else:
                whole += 1
        finally:
            sol.close()
    assert whole >= 10, whole


# ---- step forms ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['env_step', 'pass_update', 'burst3', 'step_host', 'step_host_in_state'])
def test_step_forms(S, oracle, row_env, form):
    """the respawn in front of and behind every step form: sca_env_step, sca_policy_pass + sca_env_update, a burst sca_run_steps(3) between
    respawns, sca_step_host with in_mask 0 and with SCA_HOST_IN_STATE (the block's named rows were written by the respawn)"""
    row_env(None)
    for seed, nbr in ((5, S.NBR_KDTREE), (12, S.NBR_AUTO), (3, S.NBR_KDTREE)):
        scene = F.random_scene(seed)
        every = 3 if form == 'burst3' else 1
        ref = RR.oracle_run(oracle, scene, 9, respawn_every=every)
        sol = context_of(S, scene)
        try:
            if form.startswith('step_host'):
                sol.host_state()                                            # the block exists from the start: the respawn writes its rows too
            t = 0
            while t < len(ref):
                r = ref[t]
                at = (form, 'seed', seed, 'step', t)
                if r['mission'] is not None:
                    respawn(sol, r['mission'])
                if form == 'env_step':
                    assert sol.env_step(nbr) == scene['n'] - len(r['finished']), at
                elif form == 'pass_update':
                    sol.policy_pass(nbr)
                    with pytest.raises(S.ScaError, match='between a policy pass'):        # only between two steps
                        respawn(sol, ref[0]['mission'] or ref[1]['mission'] or ref[2]['mission'])
                    sol.env_update()
                elif form == 'burst3':
                    sol.run_steps(3, nbr)
                    t += 2
                    r = ref[t]
                elif form == 'step_host':
                    assert sol.step_host(nbr, state=False) == scene['n'] - len(r['finished']), at
                else:
                    h = sol.host_state()
                    if t == 0:
                        g = sol.get_state()
                        for k in F.STATE_KEYS:
                            h[k][...] = g[k]
                    assert sol.step_host(nbr, state=True) == scene['n'] - len(r['finished']), at
                    for k in F.STATE_KEYS:
                        assert np.array_equal(h[k], r[k]), at + ('block', k)
                sol.synchronize()
                compare_with_oracle(sol, r, scene, at)
                check_finished(sol, r, at)
                t += 1
        finally:
            sol.close()


# ---- waypoint lists ------------------------------------------------------------------------------------------------------------------------
def test_lists_in_slot_form(S, oracle, row_env):
    """slot-form lists against tests/path_rule.py: a mission brings the named rows' lists, every third mission none -- rows lose their
    lists and regain them at a later respawn"""
    row_env(None)
    W = 5
    lost_and_regained = 0
    for seed in (3, 5, 12, 21):
        scene = F.random_scene(seed)
        ref = RR.oracle_run(oracle, scene, 9, lists=W)
        sol = context_of(S, scene)
        try:
            sol.set_path_slots(W, [lst[:W] for lst in F.random_paths(seed, scene)])
            sol.set_vpref(scene['vpref'], scene['vmode'])
            state = np.zeros(scene['n'], np.int8)                            # 1: lost its list at a respawn, 2: regained one afterwards
            for t, r in enumerate(ref):
                at = ('lists', 'seed', seed, 'step', t)
                m = r['mission']
                if m is not None:
                    respawn(sol, m, paths=m['paths'])
                    for j, a in enumerate(m['ids']):
                        got = 0 if m['paths'] is None else len(m['paths'][j])
                        state[a] = 1 if got == 0 and state[a] == 0 else 2 if got > 0 and state[a] == 1 else state[a]
                sol.run_steps(1, S.NBR_KDTREE)
                sol.synchronize()
                assert sol.pass_forms() & S.FORM_WAYPOINTS, at
                compare_with_oracle(sol, r, scene, at)
                check_paths(sol, r, scene, at)
        finally:
            sol.close()
        lost_and_regained += int((state == 2).sum())
    assert lost_and_regained > 0


# ---- closest-approach records --------------------------------------------------------------------------------------------------------------
def test_clearance_records_restart_at_the_respawn(S, oracle, row_env):
    """sca_clearance_enable on, against tests/clearance_rule.py with the named rows' records emptied at the respawn: other rows keep a
    respawned row as their partner, and the step count runs on"""
    import clearance_rule as CR
    row_env(None)
    for seed in (5, 12):
        scene = F.random_scene(seed)
        n = scene['n']
        ref = RR.oracle_run(oracle, scene, 8)
        sol = context_of(S, scene)
        try:
            sol.clearance_enable()
            rule = CR.empty(n)
            kept = 0
            for t, r in enumerate(ref):
                m = r['mission']
                if m is not None:
                    before = sol.clearance()
                    respawn(sol, m)
                    rule[m['ids']] = CR.empty(len(m['ids']))
                    after = sol.clearance()
                    others = np.setdiff1d(np.arange(n), m['ids'])
                    assert np.array_equal(after[others], before[others]) and np.array_equal(after[m['ids']], CR.empty(len(m['ids']))), (seed, t)
                    kept += int(np.isin(after['agent_partner'][others], m['ids']).sum())
                sol.run_steps(1, S.NBR_KDTREE)
                sol.synchronize()
                CR.step(rule, r['pos'], r['defs']['radius'], r['before'].astype(np.uint32), scene['obs_pos'], scene['obs_radius'], t + 1)
                got = sol.clearance()
                bad = np.flatnonzero(got != rule)
                assert bad.size == 0, (seed, t, bad[:8].tolist(), got[bad[:2]], rule[bad[:2]])
            assert kept > 0, seed
        finally:
            sol.close()


# ---- the trajectory log --------------------------------------------------------------------------------------------------------------------
def test_trajectory_log_goes_on(S, oracle, row_env):
    row_env(None)
    scene = F.random_scene(5)
    ref = RR.oracle_run(oracle, scene, 8)
    sol = context_of(S, scene)
    try:
        sol.history_enable(16)
        for r in ref:
            if r['mission'] is not None:
                respawn(sol, r['mission'])
            sol.run_steps(1, S.NBR_KDTREE)
        sol.synchronize()
        assert sol.history_rows()[0] == len(ref)
        h = sol.history()
        for t, r in enumerate(ref):
            served = (r['before'] & 7) == 0
            for k in ('pos', 'heading', 'vel'):
                assert np.array_equal(h[k][t][served], r[k][served]), (t, k)
    finally:
        sol.close()


# ---- the device tracker ----------------------------------------------------------------------------------------------------------------------
def tracked_scene(n, seed):
    """a circle of n agents, two in three tracked (SCA / RVO3D+Dubins), the others RVO3D and ORCA3D"""
    from sca_amd import scenarios
    sc = scenarios.circle(n, rad=12.0)
    policy = np.array([(0, 5, 1, 0, 3, 5)[i % 6] for i in range(n)], np.uint8)
    return dict(n=n, sc=sc, policy=policy, zaxis=S_zaxis(sc), mrd=scenarios.max_run_dist(sc['start'], sc['goal']), seed=seed)


def S_zaxis(sc):
    import sca_amd.solver as S
    return S.zaxis_flags(sc['start'], sc['goal'])


@pytest.mark.parametrize('n,mode', [(48, 'kd'), (64, 'kd'), (33, 'auto')])
def test_device_tracker_two_tracker_rule(S, oracle, row_env, n, mode):
    """Tracked rows respawned among tracked others, the tracker inside the pass.  The oracle keeps two trackers: the original definitions,
    and the edited ones created at the respawn; a row takes its v_pref from the newest tracker created since its last respawn (trackers are
    per agent and independent).  The call leaves the NOT-named rows' plans (sca_device_tracker_debug) and re-plan counts word for word."""
    row_env(None)
    nbr = S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE
    sc_ = tracked_scene(n, n)
    sc = sc_['sc']
    ext = np.isin(sc_['policy'], (0, 5))
    rng = np.random.default_rng(500 + n)
    radius, ps, goal, gh = np.full(n, 0.5), np.ones(n), np.ascontiguousarray(sc['goal'][:, :3]), np.ascontiguousarray(sc['goal'][:, 3:6])
    mrd = np.array(sc_['mrd'], np.float64)
    obs_pos, obs_radius = np.zeros((0, 3)), np.zeros(0)
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    trackers = []
    try:
        sol.set_obstacles(obs_pos, obs_radius)
        sol.set_agents(radius, ps, goal, sc_['policy'], sc_['zaxis'], mrd)
        sol.set_state(sc['start'][:, :3], np.zeros((n, 3), np.float32), sc['start'][:, 3:6], np.zeros(n, np.uint8))
        sol.device_tracker_enable(gh, in_pass=True)
        trackers.append(oracle.Tracker(goal, gh, ps, sc_['zaxis']))
        owner = np.zeros(n, np.int64)                                      # which tracker a row takes its v_pref from
        base = np.zeros(n, np.int64)                                       # (its re-plan count starts there)
        pos, vel, head = sc['start'][:, :3].copy(), np.zeros((n, 3), np.float32), sc['start'][:, 3:6].copy()
        flags, td, sn, perm = np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.int32), np.arange(n, dtype=np.int32)
        for t in range(14):
            if t in (5, 9):
                # a mission for some rows, tracked and not: a new start on a smaller circle, the goal across, a new goal heading
                ids = np.sort(rng.choice(n, n // 3, replace=False)).astype(np.int32)
                ang = rng.uniform(0, 2 * np.pi, len(ids))
                r0 = rng.uniform(6.0, 9.0, len(ids))
                new_pos = np.stack([r0 * np.cos(ang), r0 * np.sin(ang), rng.uniform(8.0, 12.0, len(ids))], 1)
                new_goal = np.stack([-r0 * np.cos(ang), -r0 * np.sin(ang), rng.uniform(8.0, 12.0, len(ids))], 1)
                new_head = np.stack([ang + np.pi, np.zeros(len(ids)), np.zeros(len(ids))], 1)
                new_gh = np.stack([ang + np.pi + rng.uniform(-0.5, 0.5, len(ids)), np.zeros(len(ids)), np.zeros(len(ids))], 1)
                new_ps = rng.choice([1.0, 0.8], len(ids))
                new_mrd = 3.0 * np.linalg.norm(new_pos - new_goal, axis=1) + 1.0
                others = np.setdiff1d(np.arange(n), ids)
                dbg = [sol.device_tracker_debug(int(i)) for i in others]
                rep = sol.device_tracker_replans()
                sol.respawn(ids, new_pos, np.zeros((len(ids), 3), np.float32), new_head, np.full(len(ids), 0.5), new_ps, new_goal, new_mrd, goal_heading=new_gh)
                for k, i in enumerate(others):
                    assert np.array_equal(sol.device_tracker_debug(int(i)), dbg[k], equal_nan=True), (t, int(i))
                rep2 = sol.device_tracker_replans()
                assert np.array_equal(rep2[others], rep[others]) and not rep2[ids][ext[ids]].any(), t
                pos, vel, head, flags, td, sn = (a.copy() for a in (pos, vel, head, flags, td, sn))
                goal, gh, ps, mrd = goal.copy(), gh.copy(), ps.copy(), mrd.copy()
                pos[ids], vel[ids], head[ids], flags[ids], td[ids], sn[ids] = new_pos, 0, new_head, 0, 0, 0
                goal[ids], gh[ids], ps[ids], mrd[ids] = new_goal, new_gh, new_ps, new_mrd
                trackers.append(oracle.Tracker(goal, gh, ps, sc_['zaxis']))
                owner[ids] = len(trackers) - 1
            active = ((flags & 7) == 0) & ext
            vp = np.zeros((n, 3))
            for k, tr in enumerate(trackers):
                mine = active & (owner == k)
                if mine.any():
                    vp[mine] = tr.vpref(pos, vel, head, mine.astype(np.uint8), nthreads=8)[mine]
            r = oracle.policy_step(pos, vel, head, radius, ps, flags, goal, sc_['policy'], sc_['zaxis'], vp, ext.astype(np.uint8), perm, obs_pos, obs_radius, nthreads=8)
            for tr in trackers:
                tr.note_neighbors(r['nbr_valid'], r['nbr_n'], r['nbr_dsq'])
            perm = r['perm']
            u = oracle.env_update(pos, vel, head, radius, r['flags'], goal, r['action'], td, mrd, sn, obs_pos, obs_radius)
            pos, vel, head, flags, td, sn = u['pos'], u['vel'], u['heading'], u['flags'], u['total_dist'], u['step_num']
            sol.run_steps(1, nbr)
            sol.synchronize()
            g = sol.get_state()
            for key, want in (('pos', pos), ('vel', vel), ('heading', head), ('flags', flags), ('total_dist', td), ('step_num', sn)):
                assert np.array_equal(g[key], want), (n, mode, t, key, np.flatnonzero((g[key] != want).reshape(n, -1).any(1))[:8])
            vd = sol.diag()['vpref']
            assert np.array_equal(vd[active], r['vpref'][active]), (n, mode, t, 'vpref')
            want_rep = np.zeros(n, np.int64)
            for k, tr in enumerate(trackers):
                want_rep[owner == k] = tr.replans()[owner == k]
            assert np.array_equal(sol.device_tracker_replans()[ext], want_rep[ext]), (n, mode, t, 're-plans')
        assert (owner > 0).any() and (owner[ext] == 0).any()
    finally:
        sol.close()
        for tr in trackers:
            tr.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def snapshot(sol):
    out = dict(sol.get_state())
    out['perm'] = sol.get_kd_perm()
    out.update({'nbr_' + k: v for k, v in sol.neighbors().items()})
    out.update({'diag_' + k: v for k, v in sol.diag().items()})
    out['active'] = np.array([sol.active_count()])
    out['finished'] = sol.finished()
    return out


def test_refusals_change_nothing(S, oracle, row_env):
    """every refusal with its code, decided before any device work: the state before and after a refused call is the same"""
    import sca_amd._lib as _lib
    row_env(None)
    scene = F.random_scene(12)
    n = scene['n']
    m = mission_for(scene, np.array([3, 7, 20, 41], np.int32), 1)
    ip, dp, fp = (lambda a: _lib.ptr(a, C.c_int32)), (lambda a: _lib.ptr(a, C.c_double)), (lambda a: _lib.ptr(a, C.c_float))

    def raw(sol, **kw):
        a = dict(m, zaxis=None, goal_heading=None, path_offsets=None, path_points=None, count=len(m['ids']))
        a.update(kw)
        keep = {k: (None if a[k] is None else np.ascontiguousarray(a[k], {'ids': np.int32, 'vel': np.float32, 'path_offsets': np.int32, 'zaxis': np.uint8}.get(k, np.float64)))
                for k in a if k != 'count' and k != 'paths'}
        p = lambda k, f: None if keep[k] is None else f(keep[k])
        rc = sol.L.sca_respawn_agents(sol.ctx, a['count'], p('ids', ip), p('pos', dp), p('vel', fp), p('heading', dp), p('radius', dp), p('pref_speed', dp),
                                      p('goal', dp), p('zaxis', lambda z: _lib.ptr(z, C.c_uint8)), p('max_run_dist', dp), p('goal_heading', dp),
                                      p('path_offsets', ip), p('path_points', dp))
        return rc, sol.L.sca_last_error(sol.ctx).decode()

    # no agents, no state
    sol = S.BatchedSolver(max_agents=n, max_obstacles=max(1, scene['m']))
    try:
        assert raw(sol)[0] == ERR_STATE
        sol.set_obstacles(scene['obs_pos'], scene['obs_radius'])
        sol.set_agents(scene['radius'], scene['pref_speed'], scene['goal'], scene['policy'], F.zaxis_of(scene), scene['max_run_dist'])
        assert raw(sol)[0] == ERR_STATE
        cnt = C.c_int(0)
        assert sol.L.sca_get_finished(sol.ctx, None, 0, C.byref(cnt), 48) == ERR_STATE
    finally:
        sol.close()
    sol = context_of(S, scene)
    try:
        sol.run_steps(2, S.NBR_KDTREE)
        sol.synchronize()
        before = snapshot(sol)

        def unchanged(what):
            after = snapshot(sol)
            for k in before:
                assert np.array_equal(before[k], after[k], equal_nan=before[k].dtype.kind == 'f'), (what, k)
        bad = lambda k, v, j=1: np.concatenate([np.asarray(m[k])[:j], [v], np.asarray(m[k])[j + 1:]])
        nan_pos = m['pos'].copy()
        nan_pos[2, 1] = np.nan
        cases = [('count 0', dict(count=0), ERR_ARG), ('count -1', dict(count=-1), ERR_ARG)]
        cases += [('NULL ' + k, {k: None}, ERR_ARG) for k in ('ids', 'pos', 'vel', 'heading', 'radius', 'pref_speed', 'goal', 'max_run_dist')]
        cases += [('id -1', dict(ids=bad('ids', -1)), ERR_ARG), ('id n', dict(ids=bad('ids', n)), ERR_ARG), ('repeated id', dict(ids=bad('ids', 3)), ERR_ARG),
                  ('nan position', dict(pos=nan_pos), ERR_ARG), ('inf position', dict(pos=np.where(np.isnan(nan_pos), np.inf, nan_pos)), ERR_ARG),
                  ('radius 0', dict(radius=bad('radius', 0.0)), ERR_ARG), ('radius nan', dict(radius=bad('radius', np.nan)), ERR_ARG),
                  ('pref_speed < 0', dict(pref_speed=bad('pref_speed', -1.0)), ERR_ARG), ('max_run_dist inf', dict(max_run_dist=bad('max_run_dist', np.inf)), ERR_ARG),
                  ('offsets alone', dict(path_offsets=np.zeros(5, np.int32)), ERR_ARG), ('points alone', dict(path_points=np.zeros(3)), ERR_ARG),
                  ('paths without slots', dict(path_offsets=np.zeros(5, np.int32), path_points=np.zeros(3)), ERR_UNSUPPORTED)]
        for what, kw, code in cases:
            rc, msg = raw(sol, **kw)
            assert rc == code and 'sca_respawn_agents' in msg, (what, rc, msg)
            unchanged(what)
        # sca_get_finished's own
        rows = np.zeros(n, _lib.FINISHED_DTYPE)
        rp = rows.ctypes.data_as(C.POINTER(_lib.FinishedRow))
        cnt = C.c_int(0)
        for args in ((rp, -1, C.byref(cnt), 48), (rp, n, None, 48), (None, 4, C.byref(cnt), 48), (rp, n, C.byref(cnt), 40), (rp, n, C.byref(cnt), 56)):
            assert sol.L.sca_get_finished(sol.ctx, *args) == ERR_ARG, args[1:]
        assert sol.L.sca_get_finished(sol.ctx, None, 0, C.byref(cnt), 48) == 0 and cnt.value == len(before['finished'])
        unchanged('sca_get_finished')
        # between a policy pass and its env update
        sol.policy_pass(S.NBR_KDTREE)
        assert raw(sol)[0] == ERR_STATE
        sol.env_update()
        sol.synchronize()
        before = snapshot(sol)
        # waypoint lists: block form; slot form with a list that is too long, offsets that are negative or decrease
        sol.set_paths([[] for _ in range(n)][:-1] + [[[1.0, 2.0, 3.0]]])
        rc, msg = raw(sol)
        assert rc == ERR_UNSUPPORTED and 'sca_set_path_slots' in msg, msg
        sol.set_path_slots(2)
        pts = np.zeros((8, 3))
        for what, off in (('too long', [0, 3, 3, 3, 3]), ('decreasing', [0, 2, 1, 1, 1]), ('negative', [-1, 0, 0, 0, 0])):
            rc, msg = raw(sol, path_offsets=np.array(off, np.int32), path_points=pts)
            assert rc == ERR_ARG, (what, rc, msg)
        rc, msg = raw(sol, path_offsets=np.array([0, 1, 1, 1, 1], np.int32), path_points=np.full((1, 3), np.nan))
        assert rc == ERR_ARG, msg
        sol.set_paths(None)
        unchanged('lists')
        # the device tracker: a tracked row without goal_heading
        tracked = np.flatnonzero(np.isin(scene['policy'], (0, 5)))[:4].astype(np.int32)
        sol.device_tracker_enable(np.zeros((n, 3)))
        rc, msg = raw(sol, ids=tracked)
        assert rc == ERR_ARG and 'goal_heading' in msg, msg
        sol.device_tracker_disable()
        # a shard, the cell-owner partition, scenes
        sol.set_shard(0, n - 1)
        rc, msg = raw(sol)
        assert rc == ERR_UNSUPPORTED and 'shard' in msg, msg
        assert sol.L.sca_get_finished(sol.ctx, rp, n, C.byref(cnt), 48) == ERR_UNSUPPORTED
        sol.set_shard(0, n)
        sol.partition_init(0, 1)
        rc, msg = raw(sol)
        assert rc == ERR_UNSUPPORTED and 'partition' in msg, msg
        assert sol.L.sca_get_finished(sol.ctx, rp, n, C.byref(cnt), 48) == ERR_UNSUPPORTED
        sol.partition_disable()
        sol.set_scenes([0, n // 2, n])
        rc, msg = raw(sol)
        assert rc == ERR_UNSUPPORTED and 'sca_restart_scenes' in msg, msg
        assert sol.L.sca_get_finished(sol.ctx, rp, n, C.byref(cnt), 48) == ERR_UNSUPPORTED
    finally:
        sol.close()


# ---- the Python layers -------------------------------------------------------------------------------------------------------------------
def test_run_lifelong_on_a_circle_with_obstacles(S, row_env):
    """run_lifelong on a 16-drone circle among eight obstacle spheres: the missions add up, on_done's rows are finished()'s, a respawned
    Agent replaces its row's object, and an agent whose policy or attributes differ from the row's is a ValueError before any device call"""
    import math
    from sca_amd import env as E
    from sca_amd.lifelong import run_lifelong
    row_env(None)
    n = 16
    agents = E.build_circle_agents(n, policy=E.RVO3DPolicy, rad=4.0)
    obstacles = [E.Obstacle(pos=[round(1.5 * math.cos(2 * j * math.pi / 8), 2), round(1.5 * math.sin(2 * j * math.pi / 8), 2), 10.0],
                            shape_dict={'shape': 'sphere', 'feature': 0.3}, id=j) for j in range(8)]
    env = E.MACAEnv()
    env.set_agents(agents, obstacles=obstacles)
    first = {a.id: (list(a.initial_pos), list(a.goal_pos)) for a in agents}
    seen = []

    def on_done(agent, row):
        assert env.agents[int(row['id'])] is agent and int(row['flags']) == int(env.flags[agent.id]) and int(row['flags']) & 7
        assert np.array_equal(row['pos'], env.pos[agent.id]) and row['step_num'] == env.step_num[agent.id] and row['total_dist'] == env.total_dist[agent.id]
        seen.append((int(row['id']), int(row['flags'])))

    def next_mission(agent, row):
        if len([1 for i, _ in seen if i == agent.id]) >= 3:
            return None                                                     # retired after three missions
        start, goal = first[agent.id]
        if int(row['flags']) == 1:                                          # arrived: fly back
            start, goal = list(row['pos']) + list(agent.heading_global_frame), list(agent.initial_pos)
        return E.Agent(start_pos=start, goal_pos=goal, vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=E.RVO3DPolicy, id=agent.id)

    stats = run_lifelong(env, next_mission, 400, on_done=on_done)
    missions = stats['arrived'] + stats['collided'] + stats['timed_out']
    assert missions == len(seen) == stats['respawned'] + stats['retired'] and missions >= n, stats
    assert stats['arrived'] == sum(1 for _, f in seen if f & 1 and not f & 2) and stats['collided'] == sum(1 for _, f in seen if f & 2), stats
    assert 0.0 < stats['live_fraction'] <= 1.0 and stats['agent_steps'] <= n * stats['steps'], stats
    assert stats['respawned'] > 0 and all(a._env is env for a in env.agents)
    fin = env.finished()
    assert np.array_equal(fin['id'], np.flatnonzero(env.flags & 7))
    # a row keeps its policy and its attributes
    live = [a for a in env.agents if not a.is_run_done]
    keep = env.solver.get_state()
    other = E.Agent(start_pos=first[0][0], goal_pos=first[0][1], vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=E.ORCA3DPolicy, id=0)
    with pytest.raises(ValueError, match='policy'):
        env.respawn([other])
    other = E.Agent(start_pos=first[0][0], goal_pos=first[0][1], vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=E.RVO3DPolicy, id=0)
    other.neighborDist = 5.0
    with pytest.raises(ValueError, match='neighborDist'):
        env.respawn([other])
    other = E.Agent(start_pos=first[0][0], goal_pos=first[0][1], vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=E.RVO3DPolicy, id=0)
    other.path = [[1.0, 1.0, 10.0]]
    with pytest.raises(ValueError, match='path_slots'):
        env.respawn([other])
    after = env.solver.get_state()
    for k in keep:
        assert np.array_equal(keep[k], after[k]), k
    assert len(live) == env._active
