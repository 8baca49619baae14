"""Vacant rows in a plain context (sca_retire_agents, sca_get_vacant, sca_get_population, a respawn that admits) on the GPU against the
oracle (-m gpu).  Equality, no tolerance.

The corpus is tests/vacancy_rule.py's: the fuzz scenes of tests/form_fuzz.py stepped free-running while, before every step, occupied rows
are retired, vacant rows admitted and finished rows respawned; every step of the rule runs the oracle on the occupied rows alone, compacted
in ascending id.  Behind every call and every step the context equals the rule on EVERY row, occupied or vacant: state, action rows, lists
in global ids, diag, the whole permutation, sca_active_count, sca_get_finished, sca_get_vacant, sca_get_population."""
import os

import numpy as np
import pytest

import form_fuzz as F
import respawn_rule as RR
import vacancy_rule as V
from test_gpu_form_fuzz import compare_with_oracle, context_of
from test_gpu_respawn import check_finished, mission_for, respawn

pytestmark = pytest.mark.gpu


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


def refused(S, code, call, *a, **kw):
    with pytest.raises(S.ScaError) as e:
        call(*a, **kw)
    assert '(rc=%d)' % code in str(e.value), str(e.value)
    return str(e.value)


ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5


def check_calls(sol, state, perm, vacant, at, active=None):
    """what the context holds behind a retire / respawn, in front of the step: the state of every row, the whole permutation, the vacant
    list, the population and (where the counters have been counted) sca_active_count"""
    g = sol.get_state()
    for k in F.STATE_KEYS:
        assert np.array_equal(g[k], state[k]), at + ('behind the calls', k, np.flatnonzero((g[k] != state[k]).reshape(len(vacant), -1).any(1))[:8])
    assert np.array_equal(sol.get_kd_perm(), perm), at + ('perm behind the calls',)
    want = np.flatnonzero(vacant)
    assert np.array_equal(sol.vacant(), want) and sol.vacant_count == len(want), at + ('vacant list',)
    assert sol.population() == len(vacant) - len(want), at + ('population',)
    if active is not None:
        assert sol.active_count() == active, at + ('active_count behind the calls', sol.active_count(), active)


def check_step(sol, r, scene, at):
    """what the context holds behind a step, every row: compare_with_oracle (state, the whole permutation, action rows, lists, diag),
    status, the counts and the lists of finished and vacant rows"""
    compare_with_oracle(sol, r, scene, at)
    assert np.array_equal(sol.diag()['status'], r['status']), at + ('status',)
    vac = r['vacant']
    assert sol.active_count() == int((~vac & ((r['flags'] & 7) == 0)).sum()), at + ('active_count',)
    check_finished(sol, r, at)
    assert np.array_equal(sol.vacant(), np.flatnonzero(vac)), at + ('vacant list behind the step',)
    g = sol.get_state()
    assert (g['flags'][vac] == V.VACANT).all() and not g['vel'][vac].any() and not g['heading'][vac].any(), at + ('the vacant rows as they read',)
    assert not sol.actions()[vac].any() and not sol.neighbors()['nbr_valid'][vac].any() and (sol.diag()['diag'][vac][:, :5] == -1).all(), at + ('the vacant rows\' pass words',)


def run_corpus(S, oracle, scene, nbr, ctx, steps=V.STEPS, stepper=None):
    ref = V.oracle_run(oracle, scene, steps)
    sol = context_of(S, scene)
    try:
        for t, r in enumerate(ref):
            at = ctx + ('n', scene['n'], 'step', t)
            if r['retire'] is not None:
                sol.retire(r['retire'])
            if r['mission'] is not None:
                respawn(sol, r['mission'])
            check_calls(sol, r['state_call'], r['perm_call'], r['vacant_call'], at, r['active_before'] if t > 0 else None)
            if stepper:
                stepper(sol, t)
            else:
                sol.run_steps(1, nbr)
            sol.synchronize()
            if r['vacant'].any():
                assert sol.pass_forms() & S.FORM_VACANCY, at + ('the form word says vacancy',)
            check_step(sol, r, scene, at)
    finally:
        sol.close()


# ---- the corpus --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('block', range(4))
def test_corpus_kd(S, oracle, row_env, block):
    """kd mode, default forms, all 40 seeds (1 .. 1600 agents), 12 steps with retires and admissions before every one"""
    row_env(None)
    for seed in V.SEEDS[10 * block:10 * block + 10]:
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_KDTREE, ('kd', 'seed', seed))


@pytest.mark.parametrize('row,mode', [(None, 'hostbuild'), (None, 'auto'), ('large_shard', 'kd'), ('kd_levels', 'kd')])
def test_corpus_host_build_auto_and_form_rows(S, oracle, row_env, row, mode):
    """the host build, SCA_NBR_AUTO (it resolves to the kd pass while a row is vacant: no AUTO pass is counted in those steps), the forms
    every large shard runs and the kd build's level passes forced at these sizes, ten seeds each"""
    row_env(row)
    nbr = {'hostbuild': S.NBR_KDTREE_HOSTBUILD, 'auto': S.NBR_AUTO, 'kd': S.NBR_KDTREE}[mode]
    for seed in V.SEEDS[:10]:
        scene = F.random_scene(seed)
        if mode != 'auto':
            run_corpus(S, oracle, scene, nbr, (row, mode, 'seed', seed))
            continue
        ref = V.oracle_run(oracle, scene)
        seen = {}

        def stepper(sol, t, ref=ref, seen=seen):
            before = sol.auto_stats()['auto_passes']
            sol.run_steps(1, S.NBR_AUTO)
            sol.synchronize()
            if ref[t]['vacant'].any():
                assert sol.auto_stats()['auto_passes'] == before, ('an AUTO pass while a row is vacant', seed, t)
                seen['kd'] = True
        run_corpus(S, oracle, scene, nbr, (row, mode, 'seed', seed), stepper=stepper)
        assert seen or scene['n'] == 1


def test_corpus_env_step_burst_and_pass_update(S, oracle, row_env):
    """the other ways to step: sca_env_step, a pass + its update, and sca_run_steps(3) between calls (the rule steps three times)"""
    row_env(None)
    for seed in (2, 5, 8):
        scene = F.random_scene(seed)

        def stepper(sol, t):
            if t % 2:
                sol.env_step(S.NBR_KDTREE)
            else:
                sol.policy_pass(S.NBR_KDTREE)
                sol.env_update()
        run_corpus(S, oracle, scene, S.NBR_KDTREE, ('steppers', 'seed', seed), steps=6, stepper=stepper)
    scene = F.random_scene(5)
    rule = Rule(oracle, scene)
    sol = context_of(S, scene)
    try:
        rng = np.random.default_rng(3)
        for burst in range(3):
            ids = np.sort(rng.choice(np.flatnonzero(~rule.vacant), 40, replace=False)).astype(np.int32)
            rule.retire(ids)
            sol.retire(ids)
            for _ in range(3):
                r = rule.step()
            sol.run_steps(3, S.NBR_KDTREE)
            sol.synchronize()
            check_step(sol, r, scene, ('burst', burst))
    finally:
        sol.close()


# ---- the rule beside a context, for scripted calls -----------------------------------------------------------------------------------------
class Rule:
    """vacancy_rule's state and calls for a scene, driven by the test"""
    def __init__(self, oracle, scene):
        s, n = scene, scene['n']
        self.oracle, self.scene, self.zaxis = oracle, s, F.zaxis_of(s)
        self.st = dict(pos=s['pos'].copy(), vel=s['vel'].copy(), heading=s['heading'].copy(), flags=s['flags'].copy(), total_dist=np.zeros(n),
                       step_num=np.zeros(n, np.int32))
        self.defs = {k: np.array(s[k], np.float64, copy=True) for k in RR.DEF_KEYS}
        self.perm, self.vacant = np.arange(n, dtype=np.int32), np.zeros(n, bool)

    def retire(self, ids):
        self.perm = V.retire(self.st, self.perm, self.vacant, np.asarray(ids))

    def respawn(self, m, admitted=None):
        """admitted: the rows of the mission that are written (a gated call), None: all"""
        keep = np.ones(len(m['ids']), bool) if admitted is None else np.asarray(admitted, bool)
        part = {k: v[keep] for k, v in m.items()}
        self.perm = V.admit(self.perm, self.vacant, part['ids'])
        RR.apply(self.st, self.defs, part)

    def step(self):
        r, self.st, self.perm = V.compact_step(self.oracle, self.scene, self.zaxis, self.st, self.defs, self.perm, self.vacant)
        r.update(self.st)
        r['vacant'] = self.vacant.copy()
        r['finished'] = np.flatnonzero(~self.vacant & ((self.st['flags'] & 7) != 0))
        return r

    def check_calls(self, sol, at, active=None):
        check_calls(sol, self.st, self.perm, self.vacant, at, active)


def scripted(S, oracle, scene, script, at):
    """script: (ids to retire or None, ids to admit / respawn or None) per step; every call and every step against the rule"""
    rule = Rule(oracle, scene)
    sol = context_of(S, scene)
    try:
        for t, (out, back) in enumerate(script):
            if out is not None:
                out = np.asarray(out, np.int32)
                rule.retire(out)
                sol.retire(out)
            if back is not None:
                m = mission_for(scene, np.sort(np.asarray(back, np.int32)), 7000 + 13 * t + scene['n'])
                rule.respawn(m)
                respawn(sol, m)
            rule.check_calls(sol, at + ('step', t))
            r = rule.step()
            sol.run_steps(1, S.NBR_KDTREE)
            sol.synchronize()
            check_step(sol, r, scene, at + ('step', t, 'm', int((~rule.vacant).sum())))
    finally:
        sol.close()


def sized_scene(n, seed=0):
    """switch_scene(n) for the large sizes (its oracle steps are cheap: a sparse box), a dense random box below them"""
    if n >= 2047:
        return F.switch_scene(n)
    rng = np.random.default_rng(9000 + n + seed)
    side = max(2.0, 0.9 * n ** (1 / 3))
    pos = rng.uniform(-side, side, (n, 3))
    pos[:, 2] = np.abs(pos[:, 2]) + 1.0
    goal = rng.uniform(-side, side, (n, 3))
    goal[:, 2] = np.abs(goal[:, 2]) + 1.0
    head = np.zeros((n, 3))
    head[:, 0] = rng.uniform(0, 2 * np.pi, n)
    v = rng.normal(0, 0.5, (n, 3))
    policy = rng.integers(0, 6, n).astype(np.uint8)
    return dict(n=n, m=0, pos=pos, goal=goal, heading=head, vel=v.astype(np.float32), radius=rng.choice([0.3, 0.5], n), pref_speed=rng.choice([1.0, 0.8, 1.5], n),
                policy=policy, flags=np.zeros(n, np.uint8), obs_pos=np.zeros((0, 3)), obs_radius=np.zeros(0), vpref=np.trunc(rng.normal(0, 0.6, (n, 3)) * 1e5) / 1e5,
                vmode=np.isin(policy, (0, 5)).astype(np.uint8), max_run_dist=3.0 * np.linalg.norm(pos - goal, axis=1) + 1.0, key=('sized', n, seed))


# ---- sizes -------------------------------------------------------------------------------------------------------------------------------
def test_small_sizes(S, oracle, row_env):
    """n = 2 (one row left, then both again); 11 -> 10 -> 1 -> 11 (a single leaf, a single agent); 63 / 64 / 65 and 257 with a wavefront's
    and a tile's worth of rows retired and admitted"""
    row_env(None)
    scripted(S, oracle, sized_scene(2), [([1], None), (None, [1]), ([0], None), (None, [0])], ('n', 2))
    scripted(S, oracle, sized_scene(11), [([4], None), ([0, 1, 2, 3, 5, 6, 7, 8, 9], None), (None, None), (None, list(range(10))), (None, None)], ('n', 11))
    for n in (63, 64, 65):
        rng = np.random.default_rng(n)
        a = np.sort(rng.choice(n, n - 1, replace=False))
        scripted(S, oracle, sized_scene(n), [([n // 2], None), (None, [n // 2]), (a, None), (None, a[::2]), (None, a[1::2])], ('n', n))
    rng = np.random.default_rng(257)
    a = np.sort(rng.choice(257, 256, replace=False))
    scripted(S, oracle, sized_scene(257), [(a[:1], None), (a[1:], None), (None, a[:128]), (a[:3], a[128:]), (None, None)], ('n', 257))


@pytest.mark.parametrize('n,targets', [(2049, (2048, 2047, 2049)), (6145, (4097, 4096, 4095, 769, 768, 767, 4095, 4097, 6145))])
def test_either_side_of_every_build_switch(S, oracle, row_env, n, targets):
    """the population walks down and up again across every switch of plan_kd_build: 4097 / 4096 / 4095 (k_kd_top's bound), 769 / 768 / 767
    (the tree that one k_kd_block holds) and, at 2049, the level passes' chunk -- one step at each size against the oracle of that size"""
    row_env(None)
    scene = sized_scene(n)
    rng = np.random.default_rng(n)
    order = rng.permutation(n)                                             # occupied = order[:m]
    script, m = [], n
    for want in targets:
        if want < m:
            script.append((np.sort(order[want:m]), None))
        else:
            script.append((None, np.sort(order[m:want])))
        m = want
    scripted(S, oracle, scene, script, ('n', n))


@pytest.mark.parametrize('count', (1, 255, 256, 257))
def test_rows_named_in_one_call(S, oracle, row_env, count):
    """1, 255, 256 and 257 rows named in one retire and in one admission (either side of the compaction's tile), in shuffled call order --
    the admitted ids are appended in the call's order"""
    row_env(None)
    scene = sized_scene(600)
    rule = Rule(oracle, scene)
    sol = context_of(S, scene)
    try:
        sol.run_steps(2, S.NBR_KDTREE)                                     # (a carried order that is not the identity)
        rule.step(), rule.step()
        rng = np.random.default_rng(count)
        ids = rng.permutation(600)[:count].astype(np.int32)
        rule.retire(ids), sol.retire(ids)
        rule.check_calls(sol, ('retire', count))
        r = rule.step()
        sol.run_steps(1, S.NBR_KDTREE)
        check_step(sol, r, scene, ('retired', count))
        m = mission_for(scene, np.sort(ids), count)
        shuffle = rng.permutation(count)
        m = {k: v[shuffle] for k, v in m.items()}
        rule.respawn(m), respawn(sol, m)
        rule.check_calls(sol, ('admit', count))
        assert np.array_equal(sol.get_kd_perm()[600 - count:], m['ids']) and sol.population() == 600
        r = rule.step()
        sol.run_steps(1, S.NBR_KDTREE)
        check_step(sol, r, scene, ('admitted', count))
    finally:
        sol.close()


# ---- the contract itself ---------------------------------------------------------------------------------------------------------------------
def test_occupied_rows_are_a_context_of_their_own(S, oracle, row_env):
    """behind the calls of step 6 a fresh context B is made of the occupied rows alone -- set_agents, set_state and set_kd_perm(the occupied
    prefix, renumbered) -- and runs six more steps beside the original A (no further calls): state, action rows, lists, diag, status,
    permutation prefix and active count stay equal after mapping B's ids back"""
    row_env(None)
    scene = F.random_scene(5)                                               # 257 agents, 30 obstacles, all six policies
    n = scene['n']
    ref = V.oracle_run(oracle, scene, 7)
    a = context_of(S, scene)
    b = None
    try:
        for t, r in enumerate(ref):
            if r['retire'] is not None:
                a.retire(r['retire'])
            if r['mission'] is not None:
                respawn(a, r['mission'])
            if t == 6:
                break
            a.run_steps(1, S.NBR_KDTREE)
        vac = ref[6]['vacant_call']
        occ = np.flatnonzero(~vac)
        m = len(occ)
        assert 0 < m < n
        g2c = np.full(n, -1, np.int32)
        g2c[occ] = np.arange(m, dtype=np.int32)
        defs, st = ref[6]['defs'], a.get_state()
        b = S.BatchedSolver(max_agents=m, max_obstacles=max(1, scene['m']))
        b.set_obstacles(scene['obs_pos'], scene['obs_radius'])
        b.set_agents(defs['radius'][occ], defs['pref_speed'][occ], defs['goal'][occ], scene['policy'][occ], F.zaxis_of(scene)[occ], defs['max_run_dist'][occ])
        b.set_vpref(scene['vpref'][occ], scene['vmode'][occ])
        b.set_state(*(st[k][occ] for k in F.STATE_KEYS))
        b.set_kd_perm(g2c[a.get_kd_perm()[:m]])
        for t in range(6):
            a.run_steps(1, S.NBR_KDTREE)
            b.run_steps(1, S.NBR_KDTREE)
            ga, gb = a.get_state(), b.get_state()
            for k in F.STATE_KEYS:
                assert np.array_equal(ga[k][occ], gb[k]), (t, k)
                assert np.array_equal(ga[k][vac], st[k][vac]), (t, k, 'a vacant row moved')
            assert np.array_equal(g2c[a.get_kd_perm()[:m]], b.get_kd_perm()) and np.array_equal(a.get_kd_perm()[m:], np.flatnonzero(vac)), t
            assert np.array_equal(a.actions()[occ], b.actions()) and a.active_count() == b.active_count(), t
            na, nb = a.neighbors(), b.neighbors()
            assert np.array_equal(na['nbr_valid'][occ], nb['nbr_valid']) and np.array_equal(na['nbr_n'][occ], nb['nbr_n']), t
            served = nb['nbr_valid'].astype(bool)
            in_list = served[:, None] & (np.arange(S.K)[None, :] < nb['nbr_n'][:, None])
            agent = in_list & (nb['nbr_kind'] == 0)
            assert np.array_equal(na['nbr_id'][occ][agent], occ[nb['nbr_id'][agent]]), (t, 'list ids')
            for k in ('nbr_kind', 'nbr_dsq'):
                assert np.array_equal(na[k][occ][in_list], nb[k][in_list]), (t, k)
            assert np.array_equal(na['nbr_id'][occ][in_list & ~agent], nb['nbr_id'][in_list & ~agent]), (t, 'obstacle ids')
            da, db = a.diag(), b.diag()
            assert np.array_equal(da['status'][occ], db['status']) and np.array_equal(da['diag'][occ][served], db['diag'][served]), t
    finally:
        a.close()
        if b is not None:
            b.close()


# ---- probes and gates ------------------------------------------------------------------------------------------------------------------------
def test_probe_and_gated_respawn_pass_over_vacant_rows(S, oracle, row_env):
    """sca_probe_clearance at a vacant row's own position does not find it; a gated respawn onto a vacant row's position is admitted, a
    vacant named row whose start is blocked stays vacant with every word it had, and the admitted vacant rows alone join the permutation"""
    row_env(None)
    scene = sized_scene(65)
    scene['pos'] = scene['pos'] * 6.0                                       # sparse: every row's own start is free
    scene['pos'][:, 2] = np.abs(scene['pos'][:, 2]) + 1.0
    rule = Rule(oracle, scene)
    sol = context_of(S, scene)
    try:
        before = sol.probe_clearance(scene['pos'][[7, 9]], 0.5)
        assert list(before['agent_partner']) == [7, 9]
        rule.retire([7, 20, 33]), sol.retire([7, 20, 33])
        after = sol.probe_clearance(scene['pos'][[7, 9]], 0.5)
        assert after['agent_partner'][0] != 7 and after['agent_clear'][0] > 0.0 and after['agent_partner'][1] == 9
        m = mission_for(scene, np.array([5, 7, 20, 33], np.int32), 65)
        m['pos'] = np.array([scene['pos'][33], scene['pos'][7] + [0.1, 0, 0], scene['pos'][9] + [0.05, 0, 0], scene['pos'][20]])
        # row 5 (occupied) lands on vacant row 33's place: free.  Row 7 (vacant) lands beside its own old place: free.  Row 20 (vacant)
        # lands on occupied row 9: blocked.  Row 33 (vacant) lands on vacant row 20's place: free.
        held = {k: v.copy() for k, v in sol.get_state().items()}
        verdict, _ = respawn_gated(sol, m, 0.0)
        assert list(verdict) == [S.SPAWN_ADMITTED, S.SPAWN_ADMITTED, S.SPAWN_BLOCKED_AGENT, S.SPAWN_ADMITTED], verdict
        rule.respawn(m, verdict == S.SPAWN_ADMITTED)
        rule.check_calls(sol, ('gated',))
        g = sol.get_state()
        for k in F.STATE_KEYS:
            assert np.array_equal(g[k][20], held[k][20]), k
        assert list(sol.vacant()) == [20] and list(sol.get_kd_perm()[-3:]) == [7, 33, 20]
        r = rule.step()
        sol.run_steps(1, S.NBR_KDTREE)
        check_step(sol, r, scene, ('behind the gated call',))
    finally:
        sol.close()


def respawn_gated(sol, m, margin):
    return sol.respawn(m['ids'], m['pos'], m['vel'], m['heading'], m['radius'], m['pref_speed'], m['goal'], m['max_run_dist'], margin=margin)


def test_clearance_records_and_the_log(S, oracle, row_env):
    """with the closest-approach records on, no record written after a retire names the vacant row, and the retired row's own record is
    emptied; the trajectory log goes on writing the vacant row as it stands"""
    row_env(None)
    scene = sized_scene(64)
    sol = context_of(S, scene)
    try:
        sol.clearance_enable(True)
        sol.history_enable(8)
        sol.run_steps(2, S.NBR_KDTREE)
        gone = np.array([3, 30, 31], np.int32)
        sol.retire(gone)
        rec = sol.clearance()
        assert np.isinf(rec['agent_clear'][gone]).all() and (rec['agent_partner'][gone] == -1).all()
        sol.clearance_enable(False), sol.clearance_enable(True)           # (start over: what the others measured while the three were there is gone)
        sol.run_steps(3, S.NBR_KDTREE)
        sol.synchronize()
        rec = sol.clearance()
        assert not np.isin(rec['agent_partner'], gone).any() and np.isinf(rec['agent_clear'][gone]).all()
        h, g = sol.history(), sol.get_state()
        assert sol.history_rows()[0] == 5
        for t in (2, 3, 4):
            assert np.array_equal(h['pos'][t][gone], g['pos'][gone]) and not h['vel'][t][gone].any() and not h['heading'][t][gone].any(), t
    finally:
        sol.close()


def test_slot_lists_lost_and_regained(S, oracle, row_env):
    """waypoint lists in slot form: a retired row's list is emptied (remaining 0, now_goal None), an admitted row gets the call's"""
    row_env(None)
    scene = sized_scene(33)
    paths = [[[float(i), 1.0, 2.0], [float(i), 2.0, 2.0]] for i in range(33)]
    sol = context_of(S, scene)
    try:
        sol.set_path_slots(3, paths)
        sol.run_steps(1, S.NBR_KDTREE)
        rem0, ng0 = sol.get_path_state()
        sol.retire([4, 5])
        rem, ng = sol.get_path_state()
        others = np.setdiff1d(np.arange(33), [4, 5])
        assert list(rem[[4, 5]]) == [0, 0] and np.isnan(ng[[4, 5]]).all()
        assert np.array_equal(rem[others], rem0[others]) and np.array_equal(ng[others], ng0[others], equal_nan=True) and rem0.any()
        sol.run_steps(1, S.NBR_KDTREE)
        m = mission_for(scene, np.array([4], np.int32), 33)
        respawn(sol, m, paths=[[[0.5, 0.5, 3.0]]])
        rem, ng = sol.get_path_state()
        assert rem[4] == 1 and rem[5] == 0 and list(sol.vacant()) == [5]
        sol.run_steps(1, S.NBR_KDTREE)
        rem, ng = sol.get_path_state()
        assert rem[5] == 0
        for call, args in ((sol.set_path_state, (rem, ng)), (sol.set_path_slots, (3, paths)), (sol.set_paths, (paths,))):
            assert 'vacant' in refused(S, ERR_UNSUPPORTED, call, *args)
        rem2, ng2 = sol.get_path_state()
        assert np.array_equal(rem2, rem) and np.array_equal(ng2, ng, equal_nan=True)
        respawn(sol, mission_for(scene, np.array([5], np.int32), 34), paths=[[]])
        sol.set_path_state(*sol.get_path_state())                         # every row occupied again
        sol.retire([6])
        sol.set_paths(None)                                                # clearing the lists stays legal while a row is vacant
        sol.run_steps(1, S.NBR_KDTREE)
    finally:
        sol.close()


# ---- the device tracker ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', (48, 64, 33))
def test_device_tracker_others_untouched(S, row_env, n):
    """tracked rows retired and admitted among tracked others, the tracker inside the pass: the calls leave the NOT-named rows' plans
    (sca_device_tracker_debug) and re-plan counts word for word, a retired row's record stays as it was, and an admitted tracked row starts
    from the initial record (no re-plans counted)"""
    from test_gpu_respawn import tracked_scene
    row_env(None)
    sc_ = tracked_scene(n, n)
    sc = sc_['sc']
    ext = np.isin(sc_['policy'], (0, 5))
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    try:
        sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
        sol.set_agents(np.full(n, 0.5), np.ones(n), np.ascontiguousarray(sc['goal'][:, :3]), sc_['policy'], sc_['zaxis'], np.array(sc_['mrd'], np.float64))
        sol.set_state(sc['start'][:, :3], np.zeros((n, 3), np.float32), sc['start'][:, 3:6], np.zeros(n, np.uint8))
        sol.device_tracker_enable(np.ascontiguousarray(sc['goal'][:, 3:6]), in_pass=True)
        initial = [sol.device_tracker_debug(int(i)) for i in range(n)]
        sol.run_steps(4, S.NBR_KDTREE)
        ids = np.arange(0, n, 5, dtype=np.int32)
        others = np.setdiff1d(np.arange(n), ids)
        dbg = [sol.device_tracker_debug(int(i)) for i in range(n)]
        dbg_ran = dbg
        rep = sol.device_tracker_replans()
        sol.retire(ids)
        for i in range(n):
            assert np.array_equal(sol.device_tracker_debug(i), dbg[i], equal_nan=True), ('retire', i)
        assert np.array_equal(sol.device_tracker_replans(), rep)
        sol.run_steps(2, S.NBR_KDTREE)
        assert np.array_equal(sol.device_tracker_replans()[ids], rep[ids]), 'a vacant row is not the tracker\'s'
        dbg = [sol.device_tracker_debug(int(i)) for i in others]
        rep = sol.device_tracker_replans()
        k = len(ids)
        start = sol.get_state()['pos'][ids] + [0.0, 0.0, 6.0]
        sol.respawn(ids, start, np.zeros((k, 3), np.float32), sc['start'][ids, 3:6], np.full(k, 0.5), np.ones(k), sc['goal'][ids, :3],
                    np.full(k, 200.0), goal_heading=sc['goal'][ids, 3:6])
        for j, i in enumerate(others):
            assert np.array_equal(sol.device_tracker_debug(int(i)), dbg[j], equal_nan=True), ('admit', int(i))
        rep2 = sol.device_tracker_replans()
        assert np.array_equal(rep2[others], rep[others]) and not rep2[ids][ext[ids]].any()
        assert sol.population() == n and len(sol.vacant()) == 0
        tracked = [int(i) for i in ids if ext[i]]
        assert tracked
        for i in tracked:                                                   # the initial record: what device_tracker_enable left for every row
            assert np.array_equal(sol.device_tracker_debug(i), initial[i], equal_nan=True), ('the admitted row starts from the initial record', i)
            assert not np.array_equal(dbg_ran[i], initial[i], equal_nan=True), ('the row had a plan before it was retired', i)
        sol.run_steps(2, S.NBR_KDTREE)
        assert sol.active_count() > 0
    finally:
        sol.close()


def test_the_contract_with_the_device_tracker(S, row_env):
    """the contract under the tracker inside the pass: rows retired before the first step (every tracker record is still the initial one),
    a fresh context B of the occupied rows alone with its own tracker beside the original A for eight steps: state, action rows, the v_pref
    the pass used, the tracker's records (plans, cursors, now_goal) and re-plan counts stay equal after mapping B's ids back"""
    from test_gpu_respawn import tracked_scene
    row_env(None)
    n = 48
    sc_ = tracked_scene(n, 7)
    sc = sc_['sc']
    gone = np.arange(1, n, 3, dtype=np.int32)
    occ = np.setdiff1d(np.arange(n), gone)
    ext = np.isin(sc_['policy'], (0, 5))
    mrd = np.array(sc_['mrd'], np.float64)

    def make(rows):
        k = len(rows)
        sol = S.BatchedSolver(max_agents=k, max_obstacles=1)
        sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
        sol.set_agents(np.full(k, 0.5), np.ones(k), np.ascontiguousarray(sc['goal'][rows, :3]), sc_['policy'][rows], sc_['zaxis'][rows], mrd[rows])
        sol.set_state(np.ascontiguousarray(sc['start'][rows, :3]), np.zeros((k, 3), np.float32), np.ascontiguousarray(sc['start'][rows, 3:6]), np.zeros(k, np.uint8))
        sol.device_tracker_enable(np.ascontiguousarray(sc['goal'][rows, 3:6]), in_pass=True)
        return sol
    a = make(np.arange(n))
    b = make(occ)
    try:
        a.retire(gone)
        assert ext[gone].any() and ext[occ].any()
        for t in range(8):
            a.run_steps(1, S.NBR_KDTREE)
            b.run_steps(1, S.NBR_KDTREE)
            ga, gb = a.get_state(), b.get_state()
            for k in F.STATE_KEYS:
                assert np.array_equal(ga[k][occ], gb[k]), (t, k)
            assert np.array_equal(a.actions()[occ], b.actions()) and a.active_count() == b.active_count(), t
            assert np.array_equal(a.diag()['vpref'][occ], b.diag()['vpref'], equal_nan=True), (t, 'the v_pref the pass used')
            assert np.array_equal(a.device_tracker_replans()[occ], b.device_tracker_replans()), (t, 're-plans')
            for j, i in enumerate(occ):
                if ext[i]:
                    assert np.array_equal(a.device_tracker_debug(int(i)), b.device_tracker_debug(j), equal_nan=True), (t, int(i), 'the plan')
        assert b.device_tracker_replans().any() and not a.device_tracker_replans()[gone].any()
    finally:
        a.close()
        b.close()


# ---- mission tables ----------------------------------------------------------------------------------------------------------------------
def test_mission_tables_never_take_a_vacant_row(S, row_env):
    """standing tables: a row retired in flight writes no result and moves no total, and no later step takes it"""
    row_env(None)
    n = 16
    from sca_amd import scenarios
    sc = scenarios.circle(n, rad=10.0)
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    try:
        sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
        hop = np.ascontiguousarray(sc['start'][:, :3] + [0.0, 0.0, 0.6])      # a short hop straight up: every flight ends within a few steps
        sol.set_agents(np.full(n, 0.5), np.ones(n), hop, np.full(n, 1, np.uint8), np.ones(n, np.uint8), np.full(n, 500.0))
        sol.set_state(sc['start'][:, :3], np.zeros((n, 3), np.float32), sc['start'][:, 3:6], np.zeros(n, np.uint8))
        from sca_amd import _lib
        entries = np.zeros((n, 1), _lib.MISSION_DTYPE)
        entries['pos'][:, 0] = sc['start'][:, :3]
        entries['heading'][:, 0] = sc['start'][:, 3:6]
        entries['goal'][:, 0] = hop
        entries['zaxis'][:, 0] = 1
        entries['pref_speed'][:, 0] = 1.0
        entries['max_run_dist'][:, 0] = 50.0
        entries['next_ok'][:, 0] = 0
        entries['next_fail'][:, 0] = 0
        sol.set_missions(1, 8, entries, np.zeros(n, np.int32), np.zeros(n, np.int32))
        sol.run_steps(1, S.NBR_KDTREE)
        sol.retire([2, 3])
        totals = sol.mission_totals()
        sol.run_steps(40, S.NBR_KDTREE)
        sol.synchronize()
        res = sol.mission_results()
        assert not np.isin(res['id'], [2, 3]).any(), 'a vacant row wrote a result'
        g = sol.get_state()
        assert (g['flags'][[2, 3]] == V.VACANT).all() and list(sol.vacant()) == [2, 3]
        assert sol.mission_totals()['taken'] > totals['taken'], 'the others go on taking missions'
    finally:
        sol.close()


def test_the_mission_gate_with_vacant_rows(S, row_env):
    """Standing tables under a gate (tests/test_gpu_mission_gate.py's waiting pair: rows 0 and 2 wait, the parked drones 1 and 3 stand
    within the margin of their next starts).  (1) Waiting row 0 is retired: its word is cleared, `dropped` rises by exactly 1, and no later
    step offers or takes it.  (2) Row 2 is blocked while the parked drone 3 is occupied and admitted in the step after 3 is retired: the
    probe's partner staging passes over the vacant row.  (3) Row 2 is then retired in flight: no total of the tables or of the gate moves
    in the steps that follow, and no result is written."""
    from test_gpu_mission_gate import SR, waiting_pair
    row_env(None)
    sol, sc = waiting_pair(S)
    try:
        Q = np.array([40.0, 0.0, 10.0])
        g0, t0 = sol.mission_gate_totals(), sol.mission_totals()
        assert g0['dropped'] == 0 and sol.mission_gate_state()[0].tolist() == [0, -1, 0, -1]
        cursor0 = sol.mission_state()[0].copy()
        # (1)
        sol.retire([0])
        w, v, r = sol.mission_gate_state()
        g1 = sol.mission_gate_totals()
        assert w.tolist() == [-1, -1, 0, -1] and g1['dropped'] == 1 and {k: g1[k] for k in g1 if k != 'dropped'} == {k: g0[k] for k in g0 if k != 'dropped'}
        sol.run_steps(1, S.NBR_KDTREE)
        w, v, r = sol.mission_gate_state()
        g2 = sol.mission_gate_totals()
        assert w.tolist() == [-1, -1, 0, -1] and v[2] == SR.BLOCKED_AGENT, 'row 2 is still blocked by the parked drone, row 0 is not offered'
        assert g2['offered'] == g1['offered'] + 1 and g2['blocked_agent'] == g1['blocked_agent'] + 1 and g2['dropped'] == 1
        st = sol.get_state()
        assert st['flags'][0] == V.VACANT and sol.mission_state()[0][0] == cursor0[0] and list(sol.vacant()) == [0]
        # (2)
        sol.retire([3])
        assert sol.mission_gate_totals() == g2, 'the parked drone had no pending mission: nothing is dropped'
        sol.run_steps(1, S.NBR_KDTREE)
        w, v, r = sol.mission_gate_state()
        g3 = sol.mission_gate_totals()
        st = sol.get_state()
        assert w[2] == -1 and v[2] == SR.ADMITTED and np.array_equal(st['pos'][2], Q) and st['flags'][2] == 0, 'a vacant row is no body at the gate'
        assert g3['offered'] == g2['offered'] + 1 and g3['admitted'] == g2['admitted'] + 1 and g3['dropped'] == 1
        assert sol.mission_totals()['taken'] == t0['taken'] + 1 and sol.active_count() == 1
        sol.mission_results()                                               # (collected: what follows starts from no fresh result)
        # (3)
        keys = ('arrived', 'collided', 'timed_out', 'taken', 'stopped')
        t3 = sol.mission_totals()
        sol.retire([2])
        assert sol.active_count() == 0 and list(sol.vacant()) == [0, 2, 3]
        sol.run_steps(5, S.NBR_KDTREE)
        sol.synchronize()
        t4 = sol.mission_totals()
        assert {k: t4[k] for k in keys} == {k: t3[k] for k in keys}, 'a row retired in flight moves no total'
        assert sol.mission_gate_totals() == g3 and len(sol.mission_results()) == 0 and sol.mission_result_count == 0
        assert sol.mission_gate_state()[0].tolist() == [-1] * 4 and (sol.get_state()['flags'][[0, 2, 3]] == V.VACANT).all()
    finally:
        sol.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_their_lifting(S, row_env):
    """every refusal of sca_retire_agents with its code, what is refused while a row is vacant, each of them working again once every row
    is occupied, and sca_set_agents dropping all vacancy"""
    row_env(None)
    scene = sized_scene(40)
    n = 40
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    try:
        refused(S, ERR_STATE, sol.retire, [1])                              # no agents
        sol.set_obstacles(scene['obs_pos'], scene['obs_radius'])
        sol.set_agents(scene['radius'], scene['pref_speed'], scene['goal'], scene['policy'], F.zaxis_of(scene), scene['max_run_dist'])
        sol.set_vpref(scene['vpref'], scene['vmode'])
        refused(S, ERR_STATE, sol.retire, [1])                              # no state
        assert sol.population() == n
        sol.set_state(scene['pos'], scene['vel'], scene['heading'], scene['flags'], np.zeros(n), np.zeros(n, np.int32))
        assert len(sol.vacant()) == 0 and sol.vacant_count == 0
        sol.policy_pass(S.NBR_KDTREE)
        refused(S, ERR_STATE, sol.retire, [1])                              # between a pass and its update
        sol.env_update()
        before = {k: v.copy() for k, v in sol.get_state().items()}
        perm = sol.get_kd_perm()
        blob0 = sol.save_context()
        refused(S, ERR_ARG, sol.retire, [])
        for bad in ([-1], [n], [3, 4, 3], list(range(n))):
            refused(S, ERR_ARG, sol.retire, bad)
        rc = sol.L.sca_retire_agents(sol.ctx, 2, None)
        assert rc == ERR_ARG
        sol.retire([3, 9])
        refused(S, ERR_ARG, sol.retire, [9])                                # vacant already
        refused(S, ERR_ARG, sol.retire, [a for a in range(n) if a not in (3, 9)])   # would leave nobody
        cnt = sol.vacant(capacity=1)
        assert list(cnt) == [3] and sol.vacant_count == 2                    # (the count says how much room is needed)
        g = sol.get_state()
        others = np.setdiff1d(np.arange(n), [3, 9])
        for k in F.STATE_KEYS:
            assert np.array_equal(g[k][others], before[k][others]), k
        assert np.array_equal(sol.get_kd_perm(), np.array([a for a in perm if a not in (3, 9)] + [3, 9]))
        # while a row is vacant
        st = [scene['pos'], scene['vel'], scene['heading'], scene['flags'], np.zeros(n), np.zeros(n, np.int32)]
        calls = [(sol.run_steps, (1, S.NBR_GRID)), (sol.policy_pass, (S.NBR_GRID,)), (sol.set_state, tuple(st)), (sol.set_kd_perm, (np.arange(n, dtype=np.int32),)),
                 (sol.get_kd_tree, ()), (sol.save_context, ()), (sol.context_checkpoint_bytes, ()), (sol.set_shard, (0, n // 2)),
                 (sol.partition_init, (0, 1)), (sol.set_scenes, ([0, n // 2, n],)), (sol.load_context, (blob0,)), (sol.comm_init, (0, 1, bytes(128))),
                 (sol.set_path_slots, (2,)), (sol.set_paths, ([[[1.0, 2.0, 3.0]]] * n,))]
        for call, args in calls:
            msg = refused(S, ERR_UNSUPPORTED, call, *args)
            assert 'vacant' in msg, msg
        sol.host_state()
        assert 'vacant' in refused(S, ERR_UNSUPPORTED, sol.step_host, S.NBR_KDTREE)
        sol.run_steps(1, S.NBR_KDTREE)
        # every row occupied again: all of it works
        m = mission_for(scene, np.array([3, 9], np.int32), 1)
        respawn(sol, m)
        assert sol.population() == n and len(sol.vacant()) == 0
        sol.run_steps(1, S.NBR_GRID)
        assert not sol.pass_forms() & S.FORM_VACANCY
        sol.get_kd_tree()
        blob = sol.save_context()
        sol.load_context(blob)
        sol.set_kd_perm(sol.get_kd_perm())
        sol.set_shard(0, n // 2), sol.set_shard(0, n)
        sol.step_host(S.NBR_KDTREE, state=False)
        assert sol.context_checkpoint_bytes() == blob.size
        sol.set_scenes([0, n // 2, n]), sol.set_scenes(None)
        sol.partition_init(0, 1), sol.partition_disable()
        sol.set_path_slots(2), sol.set_paths([[[1.0, 2.0, 3.0]]] * n), sol.set_paths(None)
        if sol.comm_probe():                                                # (the library is there: the call goes through; else it is refused for that reason alone)
            sol.comm_init(0, 1, sol.comm_unique_id()), sol.comm_destroy()
        else:
            assert 'vacant' not in refused(S, ERR_UNSUPPORTED, sol.comm_init, 0, 1, bytes(128))
        # sca_set_agents drops all vacancy
        sol.retire([0, 1, 2])
        sol.set_agents(scene['radius'], scene['pref_speed'], scene['goal'], scene['policy'], F.zaxis_of(scene), scene['max_run_dist'])
        assert sol.population() == n
        sol.set_state(*st)
        assert len(sol.vacant()) == 0 and np.array_equal(sol.get_kd_perm(), np.arange(n))
        sol.run_steps(1, S.NBR_GRID)
    finally:
        sol.close()


# ---- the Python layers -------------------------------------------------------------------------------------------------------------------
def ring_env(E, n=16):
    import math
    agents = E.build_circle_agents(n, policy=E.RVO3DPolicy, rad=4.0)
    obstacles = [E.Obstacle(pos=[round(1.5 * math.cos(2 * j * math.pi / 8), 2), round(1.5 * math.sin(2 * j * math.pi / 8), 2), 10.0],
                            shape_dict={'shape': 'sphere', 'feature': 0.3}, id=j) for j in range(8)]
    env = E.MACAEnv()
    env.set_agents(agents, obstacles=obstacles)
    return env, {a.id: (list(a.initial_pos), list(a.goal_pos)) for a in agents}


@pytest.mark.parametrize('margin', (None, 0.5))
def test_run_lifelong_with_retire_and_arrivals_against_plain_calls(S, row_env, margin):
    """run_lifelong(next_mission -> RETIRE for an arrival, arrivals every fifth step) against the same loop written with env.step,
    env.finished, env.retire and env.respawn: the same final state and permutation, and the stats add up"""
    from sca_amd import env as E
    from sca_amd.lifelong import RETIRE, run_lifelong
    row_env(None)
    steps = 150

    def fresh(i, first):
        return E.Agent(start_pos=first[i][0], goal_pos=first[i][1], vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=E.RVO3DPolicy, id=i)

    # -- the library's loop
    env, first = ring_env(E)
    n = len(env.agents)

    def next_mission(agent, row):
        return RETIRE if int(row['flags']) == 1 else fresh(agent.id, first)

    def arrivals(step, vacant_ids):
        assert list(vacant_ids) == sorted(vacant_ids) and all(env.agents[i].is_vacant for i in vacant_ids)
        return [fresh(i, first) for i in vacant_ids[:2]] if step % 5 == 0 else []

    stats = run_lifelong(env, next_mission, steps, spawn_margin=margin, arrivals=arrivals)
    got, got_perm = env.solver.get_state(), env.solver.get_kd_perm()
    assert stats['retired_rows'] > 0 and stats['admitted'] > 0, stats
    assert stats['population_min'] < n and stats['population_min'] <= stats['population_mean'] <= stats['population_max'] <= n, stats
    assert env.population == n - len(env.vacant) and [a.id for a in env.agents if a.is_vacant] == list(env.vacant)
    waiting = stats.get('waiting', 0)
    assert stats['arrived'] + stats['collided'] + stats['timed_out'] == stats['respawned'] + stats['retired'] + waiting, stats
    assert stats['retired_rows'] - stats['admitted'] == len(env.vacant), stats
    # -- the same loop with plain calls
    env2, first2 = ring_env(E)
    vacant, waiting2, arriving = set(), {}, set()
    active = env2._active
    for step in range(1, steps + 1):
        env2.step()
        new, leaving = [], []
        if env2._active < active:
            for row in env2.finished():
                i = int(row['id'])
                if i in waiting2:
                    continue
                if int(row['flags']) == 1:
                    leaving.append(i)
                else:
                    new.append(fresh(i, first2))
        if leaving and len(leaving) >= n - len(vacant):
            leaving.pop()
        if leaving:
            env2.retire(leaving)
            vacant.update(leaving)
        free = sorted(vacant - set(waiting2))
        came = [fresh(i, first2) for i in free[:2]] if free and step % 5 == 0 else []
        arriving.update(a.id for a in came)
        new = new + came
        if margin is None:
            if new:
                env2.respawn(new)
            vacant.difference_update(a.id for a in new)
        else:
            offer = [waiting2[i] for i in sorted(waiting2)] + new
            if offer:
                admitted = env2.respawn(offer, margin=margin)
                waiting2 = {a.id: a for a in offer}
                for a in admitted:
                    del waiting2[a.id]
                    vacant.discard(a.id)
        active = env2._active
    want = env2.solver.get_state()
    for k in F.STATE_KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got_perm, env2.solver.get_kd_perm()) and np.array_equal(env.vacant, env2.vacant)
    # -- without the new arguments the stats are what they were
    env3, first3 = ring_env(E)
    plain = run_lifelong(env3, lambda agent, row: fresh(agent.id, first3), 40)
    assert sorted(plain) == sorted(('steps', 'arrived', 'collided', 'timed_out', 'respawned', 'retired', 'agent_steps', 'live_fraction')), plain


def test_the_example_with_and_without_traffic(row_env):
    import subprocess
    import sys
    row_env(None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, 'examples', 'run_sca.py'), '--scenario', 'circle', '--agents', '32', '--policy', 'orca', '--no-obstacles', '--lifelong', '150']
    env = dict(os.environ, PYTHONPATH=root)
    plain = subprocess.run(base, capture_output=True, text=True, cwd=root, env=env)
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-2000:]
    assert 'traffic' not in plain.stdout and 'lifelong: 150 steps' in plain.stdout, plain.stdout[-2000:]
    out = subprocess.run(base + ['--traffic', '0.2', '--spawn-margin', '0.5'], capture_output=True, text=True, cwd=root, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'traffic 0.2 arrivals/step:' in out.stdout and 'drones left' in out.stdout and 'population' in out.stdout, out.stdout[-2000:]
