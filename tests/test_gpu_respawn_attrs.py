"""A respawn that brings the arriving agent's own policy and solver attributes (sca_respawn_agents_attrs, sca_respawn_agents_gated_attrs) on the
GPU (-m gpu).  Equality, no tolerance.

The corpus is tests/respawn_attrs_rule.py's: respawn_rule's missions on the fuzz scenes, every scene from the context's default parameters
with no per-agent arrays, every call with a policy per row and a full, a partial or no attribute descriptor.  After every step state,
action rows, lists entry for entry, diag, the permutation, sca_active_count and sca_get_finished equal the oracle's, which is stepped with
set_agent_params and the policy array as they stand."""
import ctypes as C
import os

import numpy as np
import pytest

import form_fuzz as F
import respawn_attrs_rule as RA
import respawn_rule as RR
from test_gpu_form_fuzz import compare_with_oracle, context_of
from test_gpu_respawn import check_finished, mission_for

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


def respawn(sol, m, scene=None, policy_after=None, **kw):
    """the call with what the mission brings; scene / policy_after: the fed v_pref and its mode again for the policies behind the call, as a
    caller without a device tracker feeds them"""
    out = sol.respawn(m['ids'], m['pos'], m['vel'], m['heading'], m['radius'], m['pref_speed'], m['goal'], m['max_run_dist'], policy=m.get('policy'),
                      attrs=m.get('attrs'), **kw)
    if scene is not None:
        sol.set_vpref(scene['vpref'], RA.vmode_of(policy_after))
    return out


def run_corpus(S, oracle, scene, nbr, ctx, steps=RR.STEPS):
    ref = RA.oracle_run(oracle, scene, steps)
    sol = context_of(S, scene)
    try:
        for t, r in enumerate(ref):
            at = ctx + ('n', scene['n'], 'step', t)
            if r['mission'] is not None:
                respawn(sol, r['mission'], scene, r['policy'])
                if t > 0:                                                   # (directly behind set_state the counters are not counted yet)
                    assert sol.active_count() == r['active_before'], at + ('active_count behind the respawn', sol.active_count(), r['active_before'])
            sol.run_steps(1, nbr)
            sol.synchronize()
            compare_with_oracle(sol, r, RA.scene_of(scene, r), at)
            assert sol.active_count() == scene['n'] - len(r['finished']), at + ('active_count',)
            check_finished(sol, r, at)
    finally:
        sol.close()


# ---- the corpus --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('block', range(4))
def test_corpus_kd_default_forms(S, oracle, row_env, block):
    """kd mode, default forms, all 40 seeds (1 .. 1600 agents), 12 steps with calls before every one"""
    row_env(None)
    for seed in RR.SEEDS[10 * block:10 * block + 10]:
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_KDTREE, ('kd', 'seed', seed))


@pytest.mark.parametrize('row,mode,block', [(row, mode, b) for b in range(2) for row, mode in ((None, 'auto'), ('large_shard', 'kd'), ('large_shard', 'auto'))])
def test_corpus_auto_and_large_shard(S, oracle, row_env, row, mode, block):
    """SCA_NBR_AUTO (whose `fits` reads the envelope) and the forms every large shard runs, on the first 20 seeds"""
    row_env(row)
    for seed in RR.SEEDS[10 * block:10 * block + 10]:
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE, (row, mode, 'seed', seed))


def test_corpus_hostbuild(S, oracle, row_env):
    row_env(None)
    for seed in (3, 5, 12):
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_KDTREE_HOSTBUILD, ('hostbuild', 'seed', seed), steps=6)


@pytest.mark.parametrize('block', range(4))
def test_corpus_grid(S, oracle, row_env, block):
    """SCA_NBR_GRID against the oracle under list rule 1, EVERY scene and step: the envelope sizes the cells, and a larger cell yields the
    same 27-cell candidate set under that rule.  respawn_attrs_rule.grid_fits holds for every scene and step
    (tests/test_respawn_attrs_cpu.py), so the grid's one refusal -- "SCA_NBR_GRID needs radius + collision reach <= neighbor_dist", which a
    wrongly grown envelope would raise -- must never occur: no scene is left out, any ScaError fails the test."""
    from test_gpu_grid_fuzz import compare_grid_step
    row_env(None)
    for seed in RR.SEEDS[10 * block:10 * block + 10]:
        scene = F.random_scene(seed)
        ref = RA.oracle_run(oracle, scene, RR.STEPS, list_rule=1)
        sol = context_of(S, scene, perm=False)
        try:
            for t, r in enumerate(ref):
                at = ('grid', 'seed', seed, 'step', t)
                if r['mission'] is not None:
                    respawn(sol, r['mission'], scene, r['policy'])
                sol.run_steps(1, S.NBR_GRID)
                sol.synchronize()
                compare_grid_step(sol, r, RA.scene_of(scene, r), at)
                check_finished(sol, r, at)
        finally:
            sol.close()


# ---- two contexts side by side -----------------------------------------------------------------------------------------------------------
def same_step(S, a, b, t, rows_a=slice(None), ids_of_b=None):
    """A and B behind a step: state, permutation, action rows, lists entry for entry, diag, status, active count"""
    ga, gb = a.get_state(), b.get_state()
    for k in F.STATE_KEYS:
        assert np.array_equal(ga[k][rows_a], gb[k]), (t, k, np.flatnonzero((ga[k][rows_a] != gb[k]).reshape(len(gb[k]), -1).any(1))[:8])
    assert np.array_equal(a.actions()[rows_a], b.actions()), (t, 'actions')
    na, nb = a.neighbors(), b.neighbors()
    served = nb['nbr_valid'].astype(bool)                                    # (rows no pass of B has served hold nothing: A's hold an earlier pass's)
    assert np.array_equal(na['nbr_valid'][rows_a], nb['nbr_valid']) and np.array_equal(na['nbr_n'][rows_a], nb['nbr_n']), (t, 'list lengths')
    in_list = served[:, None] & (np.arange(S.K)[None, :] < nb['nbr_n'][:, None])
    agent = in_list & (nb['nbr_kind'] == 0)
    ids_b = nb['nbr_id'] if ids_of_b is None else np.where(agent, ids_of_b[np.where(agent, nb['nbr_id'], 0)], nb['nbr_id'])
    for k, vb in (('nbr_id', ids_b), ('nbr_kind', nb['nbr_kind']), ('nbr_dsq', nb['nbr_dsq'])):
        assert np.array_equal(na[k][rows_a][in_list], vb[in_list]), (t, k)
    da, db = a.diag(), b.diag()
    assert np.array_equal(da['status'][rows_a], db['status']), (t, 'status')
    for k in ('diag', 'vpref'):
        assert np.array_equal(da[k][rows_a][served], db[k][served], equal_nan=True), (t, k)
    assert a.active_count() == b.active_count(), (t, 'active_count')


def fresh_context(S, scene, defs, policy, table, state, perm, rows=slice(None), max_agents=None):
    """a context made fresh from the merged definition: policies, per-agent arrays (table None: none), the fed v_pref, the state and the
    permutation; rows: the agents it holds"""
    n = len(defs['radius'][rows])
    b = S.BatchedSolver(max_agents=max_agents or n, max_obstacles=max(1, scene['m']))
    try:
        b.set_obstacles(scene['obs_pos'], scene['obs_radius'])
        b.set_agents(defs['radius'][rows], defs['pref_speed'][rows], defs['goal'][rows], policy[rows], F.zaxis_of(scene)[rows], defs['max_run_dist'][rows])
        if table is not None:
            b.set_agent_params(**{k: v[rows] for k, v in table.items()})
        b.set_vpref(scene['vpref'][rows], RA.vmode_of(policy)[rows])
        b.set_state(*(state[k][rows] for k in F.STATE_KEYS))
        b.set_kd_perm(perm)
    except BaseException:
        b.close()
        raise
    return b


def first_call(ref, want):
    """the first step of a run whose call satisfies `want`"""
    for t, r in enumerate(ref):
        if r['mission'] is not None and want(r):
            return t
    raise AssertionError('the corpus run holds no such call')


@pytest.mark.parametrize('kind', ['full', 'partial', 'policy_only'])
def test_fresh_context_equivalence(S, oracle, row_env, kind):
    """The contract.  Context A runs respawn_attrs_rule's seed 5 (257 agents, 30 obstacles) up to a call that brings a full / a partial / no
    descriptor; context B is made fresh from the merged definition (policies, per-agent arrays) + set_state + set_kd_perm.  A and B are
    bit for bit equal for six more steps."""
    row_env(None)
    scene = F.random_scene(5)
    ref = RA.oracle_run(oracle, scene, RR.STEPS)
    want = {'full': lambda r: r['mission']['attrs'] is not None and len(r['mission']['attrs']) == 7 and len(r['mission']['ids']) > 3,
            'partial': lambda r: r['mission']['attrs'] is not None and 0 < len(r['mission']['attrs']) < 7,
            'policy_only': lambda r: r['mission']['attrs'] is None}[kind]
    at = first_call(ref, want)
    assert at <= RR.STEPS - 1
    a = context_of(S, scene)
    b = None
    try:
        for r in ref[:at]:
            if r['mission'] is not None:
                respawn(a, r['mission'], scene, r['policy'])
            a.run_steps(1, S.NBR_KDTREE)
        r = ref[at]
        before, perm = a.get_state(), a.get_kd_perm()
        respawn(a, r['mission'], scene, r['policy'])
        st = {k: before[k].copy() for k in F.STATE_KEYS}
        RR.apply(st, {k: r['defs'][k].copy() for k in RR.DEF_KEYS}, r['mission'])
        # (a context that never brought attributes computes from Params: B gets per-agent arrays only where A has them)
        any_attrs = any(q['mission'] is not None and q['mission']['attrs'] for q in ref[:at + 1])
        b = fresh_context(S, scene, r['defs'], r['policy'], r['table'] if any_attrs else None, st, perm)
        ga = a.get_state()
        for k in F.STATE_KEYS:
            assert np.array_equal(ga[k], st[k]), ('behind the call', k)
        for t in range(6):
            a.run_steps(1, S.NBR_KDTREE)
            b.run_steps(1, S.NBR_KDTREE)
            same_step(S, a, b, t)
            assert np.array_equal(a.get_kd_perm(), b.get_kd_perm()), t
    finally:
        a.close()
        if b is not None:
            b.close()


def test_null_null_is_the_plain_respawn(S, oracle, row_env):
    """policy == NULL && attrs == NULL through the new symbols, plain and gated, beside a twin that calls sca_respawn_agents /
    sca_respawn_agents_gated: equal word for word, and the context has allocated no per-agent arrays (its blob has the twin's size)"""
    import sca_amd._lib as _lib
    row_env(None)
    scene = F.random_scene(5)
    ref = RR.oracle_run(oracle, scene, 8)
    a, b = context_of(S, scene), context_of(S, scene)
    dp, ip = (lambda x: _lib.ptr(np.ascontiguousarray(x, np.float64), C.c_double)), (lambda x: _lib.ptr(np.ascontiguousarray(x, np.int32), C.c_int32))
    try:
        for t, r in enumerate(ref):
            m = r['mission']
            if m is not None:
                T = len(m['ids'])
                vel = np.ascontiguousarray(m['vel'], np.float32)
                rows = (dp(m['pos']), _lib.ptr(vel, C.c_float), dp(m['heading']), dp(m['radius']), dp(m['pref_speed']), dp(m['goal']), None, dp(m['max_run_dist']),
                        None, None, None)
                if t % 2 == 0:
                    assert a.L.sca_respawn_agents_attrs(a.ctx, T, ip(m['ids']), None, None, *rows) == 0
                    b.respawn(m['ids'], m['pos'], m['vel'], m['heading'], m['radius'], m['pref_speed'], m['goal'], m['max_run_dist'])
                else:
                    va, vb = np.zeros(T, np.int32), None
                    assert a.L.sca_respawn_agents_gated_attrs(a.ctx, T, ip(m['ids']), None, None, *rows, 0.25, _lib.ptr(va, C.c_int32), None, None) == 0
                    vb, _ = b.respawn(m['ids'], m['pos'], m['vel'], m['heading'], m['radius'], m['pref_speed'], m['goal'], m['max_run_dist'], margin=0.25)
                    assert np.array_equal(va, vb), t
            a.run_steps(1, S.NBR_KDTREE)
            b.run_steps(1, S.NBR_KDTREE)
            same_step(S, a, b, t)
            assert a.save_context().tobytes() == b.save_context().tobytes(), t
    finally:
        a.close()
        b.close()


def test_gated_form_against_a_twin_naming_the_admitted(S, oracle, row_env):
    """sca_respawn_agents_gated_attrs: half the starts stand inside other drones.  Only the admitted rows take anything -- policy, attributes,
    the ORCA3D-LP list behind the synchronisation --: a twin that names exactly the admitted subset through the ungated call is equal word
    for word for six steps, and so are the blobs.  A second call that admits nobody changes nothing."""
    row_env(None)
    scene = F.random_scene(5)
    n = scene['n']
    a, b = context_of(S, scene), context_of(S, scene)
    try:
        for sol in (a, b):
            sol.run_steps(3, S.NBR_KDTREE)
        st = a.get_state()
        policy = scene['policy'].copy()
        for call in range(2):
            ids = np.sort(np.random.default_rng(7 + call).choice(n, 24, replace=False)).astype(np.int32)
            m = mission_for(scene, ids, 70 + call)
            others = np.setdiff1d(np.arange(n), ids)                        # (a body whatever its flags)
            m['pos'][::2] = st['pos'][others[:12]] + 0.05                   # every other start inside a drone that is not named
            m['pos'][1::2, 2] += 100.0 + 5.0 * np.arange(12)                # ... the others high above the box, clear of everything
            rng = np.random.default_rng(700 + call)
            m['policy'] = np.where(np.arange(24) % 3 == 0, 4, rng.integers(0, 6, 24)).astype(np.uint8)     # rows enter ORCA3D-LP, others leave it
            m['attrs'] = {k: rng.choice(RA.ATTR_VALUES[k], 24).astype(RA.dtype_of(k)) for k in ('neighbor_dist', 'max_neighbors', 'time_horizon', 'max_speed')}
            verdict, _ = respawn(a, m, margin=0.25)
            inn = verdict == S.SPAWN_ADMITTED
            assert 0 < inn.sum() < 24, verdict
            policy[ids[inn]] = m['policy'][inn]
            cut = {k: (v[inn] if isinstance(v, np.ndarray) else v) for k, v in m.items() if k != 'attrs'}
            cut['attrs'] = {k: v[inn] for k, v in m['attrs'].items()}
            respawn(b, cut)
            for sol in (a, b):
                sol.set_vpref(scene['vpref'], RA.vmode_of(policy))
            assert a.save_context().tobytes() == b.save_context().tobytes(), call
            for t in range(3):
                a.run_steps(1, S.NBR_AUTO if call else S.NBR_KDTREE)
                b.run_steps(1, S.NBR_AUTO if call else S.NBR_KDTREE)
                same_step(S, a, b, (call, t))
            st = a.get_state()
        # nobody admitted: every start inside a drone that is not named
        ids = np.flatnonzero(st['flags'] != 0)[:4].astype(np.int32)
        m = mission_for(scene, ids, 99)
        m['pos'][:] = st['pos'][np.setdiff1d(np.arange(n), ids)[:4]]
        m['policy'], m['attrs'] = np.full(4, 4, np.uint8), dict(neighbor_dist=np.full(4, 30.0))
        blob = a.save_context().tobytes()
        verdict, _ = respawn(a, m, margin=0.25)
        assert (verdict != S.SPAWN_ADMITTED).all() and a.save_context().tobytes() == blob
    finally:
        a.close()
        b.close()


# ---- the rows a call names ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,count', [(n, c) for n in (257, 2049) for c in (1, 63, 64, 65, 0)])
def test_rows_named_in_one_call(S, oracle, row_env, n, count):
    """n = 257 (seed 5) and switch_scene(2049), 3 steps, naming 1, 63, 64, 65 rows and all rows (count 0) before every one with a policy and
    a full attribute row each: against the oracle stepped from the merged state and definition"""
    row_env(None)
    scene = F.random_scene(5) if n == 257 else F.switch_scene(n)
    assert scene['n'] == n
    zaxis = F.zaxis_of(scene)
    count = count or n
    rng = np.random.default_rng(n + count)
    st = dict(pos=scene['pos'].copy(), vel=scene['vel'].copy(), heading=scene['heading'].copy(), flags=scene['flags'].copy(), total_dist=np.zeros(n),
              step_num=np.zeros(n, np.int32))
    defs = {k: np.array(scene[k], np.float64, copy=True) for k in RR.DEF_KEYS}
    policy, table = scene['policy'].copy(), RA.context_table(n)
    perm = np.arange(n, dtype=np.int32)
    sol = context_of(S, scene)
    try:
        oracle.set_params()
        for t in range(3):
            ids = np.sort(rng.choice(n, count, replace=False)).astype(np.int32)
            m = mission_for(scene, ids, 100 * n + 10 * count + t)
            m['policy'] = rng.integers(0, 6, count).astype(np.uint8)
            m['attrs'] = {k: rng.choice(RA.ATTR_VALUES[k], count).astype(RA.dtype_of(k)) for k in RA.ATTR_NAMES}
            RR.apply(st, defs, m)
            RA.apply_brings(policy, table, ids, m['policy'], m['attrs'])
            respawn(sol, m, scene, policy)
            oracle.set_agent_params(n, **table)
            r = oracle.policy_step(st['pos'], st['vel'], st['heading'], defs['radius'], defs['pref_speed'], st['flags'], defs['goal'], policy, zaxis,
                                   scene['vpref'], RA.vmode_of(policy), perm, scene['obs_pos'], scene['obs_radius'], nthreads=8)
            perm = r['perm']
            u = oracle.env_update(st['pos'], st['vel'], st['heading'], defs['radius'], r['flags'], defs['goal'], r['action'], st['total_dist'],
                                  defs['max_run_dist'], st['step_num'], scene['obs_pos'], scene['obs_radius'])
            st = {k: u[k] for k in F.STATE_KEYS}
            r.update(st)
            r['finished'] = np.flatnonzero((st['flags'] & 7) != 0)
            sol.run_steps(1, S.NBR_KDTREE)
            sol.synchronize()
            at = ('rows', n, count, 'step', t)
            compare_with_oracle(sol, r, dict(scene, policy=policy.copy()), at)
            check_finished(sol, r, at)
    finally:
        oracle.set_agent_params()
        sol.close()


# ---- step forms ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['env_step', 'pass_update', 'burst3', 'step_host'])
def test_step_forms(S, oracle, row_env, form):
    """the call in front of and behind every step form: sca_env_step, sca_policy_pass + sca_env_update (refused in between), a burst
    sca_run_steps(3) behind a call, sca_step_host with its block's rows"""
    row_env(None)
    for seed, nbr in ((5, S.NBR_KDTREE), (12, S.NBR_AUTO)):
        scene = F.random_scene(seed)
        ref = RA.oracle_run(oracle, scene, 9)
        # (a burst: the missions of its three steps cannot be given inside it -- the run is compared up to the first step that has one)
        sol = context_of(S, scene)
        try:
            if form == 'step_host':
                sol.host_state()
            t = 0
            while t < len(ref):
                r = ref[t]
                at = (form, 'seed', seed, 'step', t)
                if r['mission'] is not None:
                    respawn(sol, r['mission'], scene, r['policy'])
                if form == 'env_step':
                    assert sol.env_step(nbr) == scene['n'] - len(r['finished']), at
                elif form == 'pass_update':
                    sol.policy_pass(nbr)
                    with pytest.raises(S.ScaError, match='between a policy pass'):
                        respawn(sol, next(q['mission'] for q in ref if q['mission'] is not None))
                    sol.env_update()
                elif form == 'burst3':
                    k = 1
                    while k < 3 and t + k < len(ref) and ref[t + k]['mission'] is None:
                        k += 1
                    sol.run_steps(k, nbr)
                    t += k - 1
                    r = ref[t]
                else:
                    assert sol.step_host(nbr, state=False) == scene['n'] - len(r['finished']), at
                sol.synchronize()
                compare_with_oracle(sol, r, RA.scene_of(scene, r), at)
                check_finished(sol, r, at)
                t += 1
        finally:
            sol.close()


# ---- vacancy -----------------------------------------------------------------------------------------------------------------------------------
def test_a_retired_orca_row_is_admitted_as_an_sca_drone(S, oracle, row_env):
    """Vacant rows: ORCA3D rows are retired; three of them are admitted as SCA drones with another neighborDist, one as an ORCA3D-LP drone.
    The occupied rows are then a context of their own with their CURRENT policies and attributes, for six steps."""
    row_env(None)
    scene = F.random_scene(5)
    n = scene['n']
    a = context_of(S, scene)
    b = None
    try:
        a.run_steps(3, S.NBR_KDTREE)
        orca = np.flatnonzero(scene['policy'] == 3)[:8].astype(np.int32)
        a.retire(orca)
        a.run_steps(2, S.NBR_KDTREE)
        ids = orca[[1, 4, 6, 7]]
        m = mission_for(scene, ids, 31)
        m['policy'] = np.array([0, 0, 4, 0], np.uint8)
        m['attrs'] = dict(neighbor_dist=np.array([4.0, 15.0, 2.5, 30.0]), max_neighbors=np.array([4, 16, 8, 2], np.int32))
        policy, table = scene['policy'].copy(), RA.context_table(n)
        RA.apply_brings(policy, table, ids, m['policy'], m['attrs'])
        defs = {k: np.array(scene[k], np.float64, copy=True) for k in RR.DEF_KEYS}
        st = {k: v.copy() for k, v in a.get_state().items() if k in F.STATE_KEYS}
        RR.apply(st, defs, m)
        respawn(a, m, scene, policy)
        vac = np.zeros(n, bool)
        vac[np.setdiff1d(orca, ids)] = True
        assert np.array_equal(a.vacant(), np.flatnonzero(vac)) and a.population() == n - 4
        occ = np.flatnonzero(~vac)
        g2c = np.full(n, -1, np.int32)
        g2c[occ] = np.arange(len(occ), dtype=np.int32)
        b = fresh_context(S, scene, defs, policy, table, st, g2c[a.get_kd_perm()[:len(occ)]], rows=occ)
        for t in range(6):
            a.run_steps(1, S.NBR_KDTREE)
            b.run_steps(1, S.NBR_KDTREE)
            same_step(S, a, b, t, rows_a=occ, ids_of_b=occ)
            assert np.array_equal(g2c[a.get_kd_perm()[:len(occ)]], b.get_kd_perm()), t
        assert (a.get_state()['flags'][vac] == 11).all()
    finally:
        a.close()
        if b is not None:
            b.close()


# ---- a checkpoint behind the call ------------------------------------------------------------------------------------------------------------
def test_checkpoint_behind_the_call_resumes_in_a_fresh_context(S, oracle, row_env):
    """the blob compares the policy byte and the attributes are definition: A is saved behind a call that brought both; B, made fresh from
    the merged definition with an unrelated state, loads the blob and runs beside A"""
    row_env(None)
    scene = F.random_scene(12)
    ref = RA.oracle_run(oracle, scene, RR.STEPS)
    at = first_call(ref[2:], lambda r: r['mission']['attrs'] is not None and len(r['mission']['attrs']) == 7) + 2
    a = context_of(S, scene)
    b = stale = None
    try:
        for r in ref[:at]:
            if r['mission'] is not None:
                respawn(a, r['mission'], scene, r['policy'])
            a.run_steps(1, S.NBR_KDTREE)
        r = ref[at]
        respawn(a, r['mission'], scene, r['policy'])
        blob = a.save_context()
        start = {k: scene[k] for k in ('pos', 'vel', 'heading', 'flags')}
        start.update(total_dist=np.zeros(scene['n']), step_num=np.zeros(scene['n'], np.int32))
        b = fresh_context(S, scene, r['defs'], r['policy'], r['table'], start, np.arange(scene['n'], dtype=np.int32))
        b.load_context(blob)
        assert b.save_context().tobytes() == blob.tobytes()
        # the definition BEFORE the call is another definition: its policies differ
        if not np.array_equal(r['policy_before'], r['policy']):
            stale = fresh_context(S, scene, r['defs'], r['policy_before'], r['table'], start, np.arange(scene['n'], dtype=np.int32))
            with pytest.raises(S.ScaError):
                stale.load_context(blob)
        for t in range(6):
            a.run_steps(1, S.NBR_KDTREE)
            b.run_steps(1, S.NBR_KDTREE)
            same_step(S, a, b, t)
    finally:
        for sol in (a, b, stale):
            if sol is not None:
                sol.close()


# ---- the device tracker ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,mode', [(48, 'kd'), (64, 'kd'), (33, 'auto')])
def test_device_tracker_rows_enter_and_leave_with_their_planner_attributes(S, oracle, row_env, n, mode):
    """Rows move ORCA3D / RVO3D -> SCA and SCA / RVO3D+Dubins -> ORCA3D among tracked others, the tracker inside the pass, and every named
    row brings its own turning radius and pitch limits: three calls -- a few classes; every named row its own radius (at n = 64 and 48
    more than 16 classes among the tracked rows: the per-agent form); two radii again (back to classes).  The oracle keeps one tracker
    per call (tests/test_gpu_respawn.py's two-tracker rule) with the per-agent planner attributes as they stand; a row takes its v_pref
    from the newest tracker created since its last respawn while its CURRENT policy is tracked, and its policy's own rule otherwise.
    A call leaves the not-named rows' plans and re-plan counts word for word; a row that entered starts from no plan, a row that left
    holds the initial record."""
    from test_gpu_respawn import tracked_scene
    row_env(None)
    nbr = S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE
    sc_ = tracked_scene(n, n)
    sc = sc_['sc']
    policy = sc_['policy'].copy()
    rng = np.random.default_rng(900 + n)
    radius, ps, goal, gh = np.full(n, 0.5), np.ones(n), np.ascontiguousarray(sc['goal'][:, :3]), np.ascontiguousarray(sc['goal'][:, 3:6])
    mrd = np.array(sc_['mrd'], np.float64)
    nd, R, plo, phi = np.full(n, 10.0), np.full(n, 1.5), np.full(n, -np.pi / 4), np.full(n, np.pi / 4)
    obs_pos, obs_radius = np.zeros((0, 3)), np.zeros(0)
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    trackers = []
    try:
        sol.set_obstacles(obs_pos, obs_radius)
        sol.set_agents(radius, ps, goal, policy, sc_['zaxis'], mrd)
        sol.set_state(sc['start'][:, :3], np.zeros((n, 3), np.float32), sc['start'][:, 3:6], np.zeros(n, np.uint8))
        sol.device_tracker_enable(gh, in_pass=True)
        trackers.append(oracle.Tracker(goal, gh, ps, sc_['zaxis']))
        owner = np.zeros(n, np.int64)
        pos, vel, head = sc['start'][:, :3].copy(), np.zeros((n, 3), np.float32), sc['start'][:, 3:6].copy()
        flags, td, sn, perm = np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.int32), np.arange(n, dtype=np.int32)
        entered = left = 0
        most = 0
        blank = None
        wide = None
        for t in range(16):
            if t in (4, 8, 12):
                call = (4, 8, 12).index(t)
                if call == 0:
                    ids = np.sort(rng.choice(n, n // 3, replace=False)).astype(np.int32)
                elif call == 1:
                    ids = wide = np.sort(rng.choice(n, 2 * n // 3, replace=False)).astype(np.int32)
                else:
                    ids = wide
                k = len(ids)
                was = np.isin(policy[ids], (0, 5))
                # every other named row changes sides, the others keep theirs (one of them swaps SCA <-> RVO3D+Dubins: tracked both ways)
                new_pol = policy[ids].copy()
                flip = np.arange(k) % 2 == 0
                new_pol[flip & was] = 3
                new_pol[flip & ~was] = 0
                stay = np.flatnonzero(~flip & was)
                if len(stay):
                    new_pol[stay[0]] = 5 if policy[ids][stay[0]] == 0 else 0
                new_R = (rng.choice([1.5, 2.0, 2.5], k), 1.2 + 0.05 * np.arange(k), rng.choice([1.5, 2.0], k))[call]
                new_lo = np.where(np.arange(k) % 3 == 0, -0.5, -np.pi / 4)
                new_hi = np.where(np.arange(k) % 3 == 0, 0.6, np.pi / 4)
                new_nd = np.where(np.arange(k) % 3 == 0, 4.0, 10.0)
                ang = rng.uniform(0, 2 * np.pi, k)
                r0 = rng.uniform(6.0, 9.0, k)
                new_pos = np.stack([r0 * np.cos(ang), r0 * np.sin(ang), rng.uniform(8.0, 12.0, k)], 1)
                new_goal = np.stack([-r0 * np.cos(ang), -r0 * np.sin(ang), rng.uniform(8.0, 12.0, k)], 1)
                new_head = np.stack([ang + np.pi, np.zeros(k), np.zeros(k)], 1)
                new_gh = np.stack([ang + np.pi + rng.uniform(-0.5, 0.5, k), np.zeros(k), np.zeros(k)], 1)
                new_ps = rng.choice([1.0, 0.8], k)
                new_mrd = 3.0 * np.linalg.norm(new_pos - new_goal, axis=1) + 1.0
                others = np.setdiff1d(np.arange(n), ids)
                dbg = [sol.device_tracker_debug(int(i)) for i in others]
                rep = sol.device_tracker_replans()
                if blank is None:
                    never = np.flatnonzero(~np.isin(policy, (0, 5)))[0]      # an untracked row of the enable call: the initial record
                    blank = sol.device_tracker_debug(int(never))
                attrs = dict(neighbor_dist=new_nd, turning_radius=new_R, pitch_lo=new_lo, pitch_hi=new_hi)
                with pytest.raises(S.ScaError, match='goal_heading'):       # judged by the NEW policy: rows become tracked
                    sol.respawn(ids, new_pos, np.zeros((k, 3), np.float32), new_head, np.full(k, 0.5), new_ps, new_goal, new_mrd, policy=new_pol, attrs=attrs)
                now = np.isin(new_pol, (0, 5))
                bad_R = np.where(np.arange(k) == int(np.flatnonzero(now)[0]), 0.0, new_R)
                with pytest.raises(S.ScaError, match='turning radius'):     # a tracked row's planner attributes by the tracker's rules
                    sol.respawn(ids, new_pos, np.zeros((k, 3), np.float32), new_head, np.full(k, 0.5), new_ps, new_goal, new_mrd, goal_heading=new_gh, policy=new_pol,
                                attrs=dict(attrs, turning_radius=bad_R))
                bad_R = np.where(np.arange(k) == int(np.flatnonzero(~now)[0]), 0.0, new_R)          # ... an untracked row's entries are ignored
                sol.respawn(ids, new_pos, np.zeros((k, 3), np.float32), new_head, np.full(k, 0.5), new_ps, new_goal, new_mrd, goal_heading=new_gh, policy=new_pol,
                            attrs=dict(attrs, turning_radius=bad_R))
                for j, i in enumerate(others):
                    assert np.array_equal(sol.device_tracker_debug(int(i)), dbg[j], equal_nan=True), (t, int(i))
                rep2 = sol.device_tracker_replans()
                assert np.array_equal(rep2[others], rep[others]) and not rep2[ids].any(), t
                for i in ids[was & ~now]:
                    assert np.array_equal(sol.device_tracker_debug(int(i)), blank, equal_nan=True), (t, int(i), 'a row that left the tracker')
                assert np.array_equal(sol.vpref_mode()[ids], now.astype(np.uint8)), (t, 'vpref_mode of the named rows')
                entered += int((~was & now).sum())
                left += int((was & ~now).sum())
                pos, vel, head, flags, td, sn = (a.copy() for a in (pos, vel, head, flags, td, sn))
                goal, gh, ps, mrd, policy, nd, R, plo, phi = (a.copy() for a in (goal, gh, ps, mrd, policy, nd, R, plo, phi))
                pos[ids], vel[ids], head[ids], flags[ids], td[ids], sn[ids] = new_pos, 0, new_head, 0, 0, 0
                goal[ids], gh[ids], ps[ids], mrd[ids], policy[ids] = new_goal, new_gh, new_ps, new_mrd, new_pol
                nd[ids], R[ids], plo[ids], phi[ids] = new_nd, new_R, new_lo, new_hi
                oracle.set_agent_params(n, neighbor_dist=nd)
                trackers.append(oracle.Tracker(goal, gh, ps, sc_['zaxis']))
                trackers[-1].set_params(neighbor_dist=nd, turning_radius=R, pitch_lo=plo, pitch_hi=phi)
                owner[ids] = len(trackers) - 1
                tracked_now = np.isin(policy, (0, 5))
                most = max(most, len({(a, b, c) for a, b, c in zip(R[tracked_now], plo[tracked_now], phi[tracked_now])}))
                if call == 2:
                    assert len({(a, b, c) for a, b, c in zip(R[tracked_now], plo[tracked_now], phi[tracked_now])}) <= 16
            ext = np.isin(policy, (0, 5))
            active = ((flags & 7) == 0) & ext
            vp = np.zeros((n, 3))
            for k_, tr in enumerate(trackers):
                mine = active & (owner == k_)
                if mine.any():
                    vp[mine] = tr.vpref(pos, vel, head, mine.astype(np.uint8), nthreads=8)[mine]
            r = oracle.policy_step(pos, vel, head, radius, ps, flags, goal, policy, sc_['zaxis'], vp, ext.astype(np.uint8), perm, obs_pos, obs_radius, nthreads=8)
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
            assert np.array_equal(sol.actions(), r['action']), (n, mode, t, 'actions')
            vd = sol.diag()['vpref']
            assert np.array_equal(vd[active], r['vpref'][active]), (n, mode, t, 'vpref')
            want_rep = np.zeros(n, np.int64)
            for k_, tr in enumerate(trackers):
                want_rep[owner == k_] = tr.replans()[owner == k_]
            assert np.array_equal(sol.device_tracker_replans()[ext], want_rep[ext]), (n, mode, t, 're-plans')
        assert entered >= 4 and left >= 4, (entered, left)
        assert most > 16 or n < 64, ('distinct planner triples among the tracked rows at most', most)
    finally:
        oracle.set_agent_params()
        sol.close()
        for tr in trackers:
            tr.close()


# ---- standing features ---------------------------------------------------------------------------------------------------------------------
def test_slot_lists_across_a_straight_line_tracked_change(S, oracle, row_env):
    """waypoint lists in slot form, no device tracker: a straight-line row with a list (k_waypoint writes its v_pref, mode 1) becomes an SCA
    row -- its mode goes back to 0 and the caller's fed v_pref counts again -- and an SCA row becomes a straight-line row with a list.
    Beside a fresh context with the merged definition, the lists and the same cursors."""
    row_env(None)
    scene = F.random_scene(12)
    n = scene['n']
    W = 3
    paths = [lst[:W] for lst in F.random_paths(12, scene)]
    a = context_of(S, scene)
    b = None
    try:
        a.set_path_slots(W, paths)
        a.set_vpref(scene['vpref'], scene['vmode'])
        a.run_steps(2, S.NBR_KDTREE)
        mode = a.vpref_mode()
        straight = np.flatnonzero((mode == 1) & ~np.isin(scene['policy'], (0, 5)))[:3]
        tracked = np.flatnonzero(np.isin(scene['policy'], (0, 5)))[:3]
        assert len(straight) == 3 and len(tracked) == 3
        ids = np.sort(np.concatenate([straight, tracked])).astype(np.int32)
        m = mission_for(scene, ids, 5)
        policy = scene['policy'].copy()
        policy[straight], policy[tracked] = 0, 3
        m['policy'] = policy[ids]
        m['paths'] = RR.random_lists(np.random.default_rng(3), m, m['radius'])
        for j in range(len(ids)):
            m['paths'][j] = (m['paths'][j] + [[float(x) for x in np.round(0.5 * (m['pos'][j] + m['goal'][j]), 3)]])[:W]     # every named row brings a list
        before, perm = a.get_state(), a.get_kd_perm()
        respawn(a, m, paths=m['paths'])
        assert not a.vpref_mode()[straight].any(), 'the mode bit of a row that became an SCA row'
        a.set_vpref(scene['vpref'], RA.vmode_of(policy))
        st = {k: before[k].copy() for k in F.STATE_KEYS}
        defs = {k: np.array(scene[k], np.float64, copy=True) for k in RR.DEF_KEYS}
        RR.apply(st, defs, m)
        ln, rooms = a.path_slot_lists()
        lists = [rooms[i, :ln[i]].tolist() for i in range(n)]
        rem, ng = a.get_path_state()
        b = fresh_context(S, scene, defs, policy, None, st, perm)
        b.set_path_slots(W, lists)
        b.set_path_state(rem, ng)
        b.set_vpref(scene['vpref'], RA.vmode_of(policy))
        for t in range(6):
            a.run_steps(1, S.NBR_KDTREE)
            b.run_steps(1, S.NBR_KDTREE)
            same_step(S, a, b, t)
            (ra, ga), (rb, gb) = a.get_path_state(), b.get_path_state()
            assert np.array_equal(ra, rb) and np.array_equal(ga, gb, equal_nan=True) and np.array_equal(a.vpref_mode(), b.vpref_mode()), t
    finally:
        a.close()
        if b is not None:
            b.close()


def test_clearance_records_restart_at_the_call(S, oracle, row_env):
    """sca_clearance_enable on, against tests/clearance_rule.py with the named rows' records emptied at the call: other rows keep a
    respawned row as their partner whatever it has become, and the step count runs on"""
    import clearance_rule as CR
    row_env(None)
    for seed in (5, 12):
        scene = F.random_scene(seed)
        n = scene['n']
        ref = RA.oracle_run(oracle, scene, 8)
        sol = context_of(S, scene)
        try:
            sol.clearance_enable()
            rule = CR.empty(n)
            kept = 0
            for t, r in enumerate(ref):
                m = r['mission']
                if m is not None:
                    before = sol.clearance()
                    respawn(sol, m, scene, r['policy'])
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


def test_trajectory_log_goes_on(S, oracle, row_env):
    """the log's rows across calls that change policies and attributes: one row per step, the served agents' poses the oracle's"""
    row_env(None)
    scene = F.random_scene(5)
    ref = RA.oracle_run(oracle, scene, 8)
    sol = context_of(S, scene)
    try:
        sol.history_enable(16)
        for r in ref:
            if r['mission'] is not None:
                respawn(sol, r['mission'], scene, r['policy'])
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


@pytest.mark.parametrize('gate', [None, 0.3])
def test_mission_tables_take_with_the_new_policy(S, oracle, row_env, gate):
    """standing mission tables, without and with the admission gate: a row respawned as another kind is later taken by its table -- the take keeps the row's policy and
    attributes, the NEW ones -- beside a twin that was defined with them from the start (sca_set_agents + sca_set_agent_params) and got the
    same plain respawn"""
    import sca_amd._lib as _lib
    row_env(None)
    scene = F.random_scene(12)
    n = scene['n']
    ids = np.flatnonzero(scene['flags'] != 0)[:6].astype(np.int32)
    assert len(ids) == 6
    m = mission_for(scene, ids, 8)
    m['goal'] = m['pos'] + np.array([0.7, 0.0, 0.0])                        # arrives within a few steps: the table's entry is taken
    m['max_run_dist'] = np.full(6, 50.0)
    policy, table = scene['policy'].copy(), RA.context_table(n)
    m['policy'] = np.array([0, 1, 2, 3, 4, 5], np.uint8)
    m['attrs'] = dict(neighbor_dist=np.array([4.0, 15.0, 2.5, 30.0, 10.0, 4.0]), max_speed=np.array([1.5, 1.0, 0.7, 3.0, 1.0, 1.5]))
    RA.apply_brings(policy, table, ids, m['policy'], m['attrs'])
    entries = np.zeros(n, _lib.MISSION_DTYPE)
    rng = np.random.default_rng(4)
    side = RR.box_of(scene)
    entries['pos'] = rng.uniform(-side, side, (n, 3))
    entries['pos'][:, 2] = np.abs(entries['pos'][:, 2]) + 1.0
    entries['goal'] = entries['pos'] + np.array([0.0, 3.0, 0.0])
    entries['pref_speed'], entries['max_run_dist'] = 1.0, 20.0
    entries['next_ok'], entries['next_fail'], entries['flags'] = -1, -1, 2     # (one entry per row, then stop; SCA_MISSION_KEEP_ZAXIS)
    first = np.zeros(n, np.int32)
    a = context_of(S, scene)
    b = None
    try:
        defs = {k: np.array(scene[k], np.float64, copy=True) for k in RR.DEF_KEYS}
        start = dict(pos=scene['pos'], vel=scene['vel'], heading=scene['heading'], flags=scene['flags'], total_dist=np.zeros(n), step_num=np.zeros(n, np.int32))
        b = fresh_context(S, scene, defs, policy, table, start, np.arange(n, dtype=np.int32))
        for sol in (a, b):
            sol.set_missions(1, 4, entries, first, first)
            if gate is not None:                                        # ... with the admission gate in front of every take
                sol.set_mission_gate(gate)
        respawn(a, m, scene, policy)
        plain = {k: v for k, v in m.items() if k not in ('policy', 'attrs')}
        respawn(b, plain, scene, policy)
        for t in range(12):
            a.run_steps(1, S.NBR_KDTREE)
            b.run_steps(1, S.NBR_KDTREE)
            same_step(S, a, b, t)
            assert a.mission_totals() == b.mission_totals(), t
            if gate is not None:
                assert a.mission_gate_totals() == b.mission_gate_totals(), t
        cursor, _ = a.mission_state()
        assert (cursor[ids] == 0).any(), 'no named row took its entry: the test shows nothing'
    finally:
        a.close()
        if b is not None:
            b.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(S, oracle, row_env):
    """every refusal the two entry points add, with its code, decided before any device work: the context's own blob stays byte-equal"""
    import sca_amd._lib as _lib
    row_env(None)
    scene = F.random_scene(12)
    n = scene['n']
    m = mission_for(scene, np.array([3, 7, 20, 41], np.int32), 1)
    ip, dp, fp, bp = (lambda a: _lib.ptr(a, C.c_int32)), (lambda a: _lib.ptr(a, C.c_double)), (lambda a: _lib.ptr(a, C.c_float)), (lambda a: _lib.ptr(a, C.c_uint8))
    full = C.sizeof(_lib.RestartAttrs)

    def raw(sol, gated=False, desc=None, struct_bytes=full, reserved=0, margin=0.25, **kw):
        a = dict(m, zaxis=None, goal_heading=None, path_offsets=None, path_points=None, count=len(m['ids']), policy=None)
        a.update(kw)
        keep = {k: (None if a[k] is None else np.ascontiguousarray(a[k], {'ids': np.int32, 'vel': np.float32, 'path_offsets': np.int32, 'zaxis': np.uint8,
                                                                           'policy': np.uint8}.get(k, np.float64))) for k in a if k != 'count'}
        p = lambda k, f: None if keep[k] is None else f(keep[k])
        d, held = None, []
        if desc is not None:
            d = _lib.RestartAttrs(struct_bytes=struct_bytes, reserved=reserved)
            for name, v in desc.items():
                v = np.ascontiguousarray(v, RA.dtype_of(name))
                held.append(v)
                setattr(d, name, ip(v) if name == 'max_neighbors' else dp(v))
        args = (sol.ctx, a['count'], p('ids', ip), p('policy', bp), None if d is None else C.byref(d), p('pos', dp), p('vel', fp), p('heading', dp), p('radius', dp),
                p('pref_speed', dp), p('goal', dp), p('zaxis', bp), p('max_run_dist', dp), p('goal_heading', dp), p('path_offsets', ip), p('path_points', dp))
        if gated:
            verdict = np.zeros(max(1, a['count']), np.int32)
            rc = sol.L.sca_respawn_agents_gated_attrs(*args, margin, ip(verdict), None, None)
        else:
            rc = sol.L.sca_respawn_agents_attrs(*args)
        return rc, sol.L.sca_last_error(sol.ctx).decode()

    pol = np.array([0, 3, 4, 5], np.uint8)
    sol = S.BatchedSolver(max_agents=n, max_obstacles=max(1, scene['m']))
    try:
        assert raw(sol, policy=pol)[0] == ERR_STATE
    finally:
        sol.close()
    sol = context_of(S, scene)
    try:
        sol.run_steps(2, S.NBR_KDTREE)
        sol.synchronize()
        before = sol.save_context().tobytes()

        def unchanged(what):
            assert sol.save_context().tobytes() == before, what
        bad = lambda k, v, j=1: np.concatenate([np.asarray(m[k])[:j], [v], np.asarray(m[k])[j + 1:]])
        # what sca_respawn_agents refuses, through both symbols, with its codes
        cases = [('count 0', dict(count=0), ERR_ARG), ('NULL pos', dict(pos=None), ERR_ARG), ('id n', dict(ids=bad('ids', n)), ERR_ARG),
                 ('repeated id', dict(ids=bad('ids', 3)), ERR_ARG), ('radius 0', dict(radius=bad('radius', 0.0)), ERR_ARG),
                 ('offsets alone', dict(path_offsets=np.zeros(5, np.int32)), ERR_ARG),
                 ('paths without slots', dict(path_offsets=np.zeros(5, np.int32), path_points=np.zeros(3)), ERR_UNSUPPORTED)]
        for gated in (False, True):
            who = 'sca_respawn_agents_gated_attrs' if gated else 'sca_respawn_agents_attrs'
            for what, kw, code in cases:
                rc, msg = raw(sol, gated=gated, policy=pol, **kw)
                assert rc == code and who in msg, (what, rc, msg)
                unchanged(what)
            # the new ones
            ok = dict(neighbor_dist=np.full(4, 4.0))
            new = [('policy 6', dict(policy=np.array([0, 6, 1, 2], np.uint8)), {}, 'row 1'),
                   ('struct_bytes 4', dict(policy=pol, desc=ok, struct_bytes=4), {}, 'struct_bytes'),
                   ('struct_bytes cuts a pointer', dict(policy=pol, desc=ok, struct_bytes=12), {}, 'struct_bytes'),
                   ('struct_bytes too large', dict(policy=pol, desc=ok, struct_bytes=full + 8), {}, 'struct_bytes'),
                   ('reserved', dict(policy=pol, desc=ok, reserved=1), {}, 'reserved'),
                   ('planner without a tracker', dict(desc=dict(turning_radius=np.full(4, 2.0))), {}, 'device tracker'),
                   ('neighbor_dist 0', dict(desc=dict(neighbor_dist=np.array([4.0, 4.0, 0.0, 4.0]))), {}, 'row 2'),
                   ('max_neighbors 17', dict(desc=dict(max_neighbors=np.array([4, 4, 4, 17], np.int32))), {}, 'row 3'),
                   ('max_heading_change 4', dict(policy=pol, desc=dict(max_heading_change=np.array([4.0, 0.3, 0.3, 0.3]))), {}, 'row 0'),
                   ('dt_nominal nan', dict(desc=dict(dt_nominal=np.array([0.1, np.nan, 0.1, 0.1]))), {}, 'row 1')]
            for what, kw, _, word in new:
                rc, msg = raw(sol, gated=gated, **kw)
                assert rc == ERR_ARG and who in msg and word in msg, (what, rc, msg)
                unchanged(what)
            if gated:
                rc, msg = raw(sol, gated=True, policy=pol, margin=-1.0)
                assert rc == ERR_ARG and 'margin' in msg, msg
                unchanged('margin')
        # a descriptor that reaches only as far as the solver's arrays is a valid size: the planner's read as NULL
        rc, msg = raw(sol, policy=pol, desc=dict(neighbor_dist=np.full(4, 4.0)), struct_bytes=8 + 7 * C.sizeof(C.c_void_p))
        assert rc == 0, msg
        sol.set_vpref(scene['vpref'], RA.vmode_of(np.where(np.isin(np.arange(n), m['ids']), 0, scene['policy'])))      # (the fed mode: not read below)
        before = sol.save_context().tobytes()
        # between a policy pass and its env update
        sol.policy_pass(S.NBR_KDTREE)
        assert raw(sol, policy=pol)[0] == ERR_STATE
        sol.env_update()
        sol.synchronize()
        before = sol.save_context().tobytes()
        # the device tracker: a row whose NEW policy is tracked without goal_heading
        was_untracked = np.flatnonzero(~np.isin(scene['policy'], (0, 5)) & ~np.isin(np.arange(n), m['ids']))[:4].astype(np.int32)
        sol.device_tracker_enable(np.zeros((n, 3)))
        before = sol.save_context().tobytes()
        rc, msg = raw(sol, ids=was_untracked, policy=np.array([3, 3, 0, 3], np.uint8))
        assert rc == ERR_ARG and 'goal_heading' in msg and 'row 2' in msg, msg
        unchanged('goal_heading by the new policy')
        rc, msg = raw(sol, ids=was_untracked, policy=np.array([3, 3, 1, 3], np.uint8))          # all untracked afterwards: no goal_heading needed
        assert rc == 0, msg
        before = sol.save_context().tobytes()
        # a row whose NEW policy is tracked and whose planner attributes break sca_device_tracker_set_agent_params' rules; an untracked row's are ignored
        for what, desc in (('R 0', dict(turning_radius=np.array([2.0, 0.0, 2.0, 2.0]))), ('R nan', dict(turning_radius=np.array([2.0, np.nan, 2.0, 2.0]))),
                           ('lo >= hi', dict(pitch_lo=np.array([-0.5, 0.7, -0.5, -0.5]), pitch_hi=np.full(4, 0.6))),
                           ('hi inf', dict(pitch_hi=np.array([0.6, np.inf, 0.6, 0.6])))):
            rc, msg = raw(sol, ids=was_untracked, goal_heading=np.zeros((4, 3)), policy=np.array([3, 0, 3, 3], np.uint8), desc=desc)
            assert rc == ERR_ARG and 'row 1' in msg and 'turning radius' in msg, (what, rc, msg)
            unchanged(what)
        rc, msg = raw(sol, ids=was_untracked, goal_heading=np.zeros((4, 3)), policy=np.array([3, 1, 3, 3], np.uint8), desc=dict(turning_radius=np.array([2.0, 0.0, 2.0, 2.0])))
        assert rc == 0, msg
        # per-agent planner attributes set by sca_device_tracker_set_agent_params: a change of sides is accepted, the classes are dealt again
        sol.device_tracker_set_agent_params(turning_radius=np.where(np.arange(n) % 2 == 0, 1.5, 2.0))
        rc, msg = raw(sol, ids=was_untracked, goal_heading=np.zeros((4, 3)), policy=np.array([3, 0, 3, 5], np.uint8))
        assert rc == 0, msg
        sol.run_steps(2, S.NBR_KDTREE)
        sol.synchronize()
        sol.device_tracker_disable()
        # a shard, the cell-owner partition, scenes
        sol.set_shard(0, n - 1)
        rc, msg = raw(sol, policy=pol)
        assert rc == ERR_UNSUPPORTED and 'shard' in msg, msg
        sol.set_shard(0, n)
        sol.partition_init(0, 1)
        rc, msg = raw(sol, policy=pol)
        assert rc == ERR_UNSUPPORTED and 'partition' in msg, msg
        sol.partition_disable()
        sol.set_scenes([0, n // 2, n])
        rc, msg = raw(sol, policy=pol)
        assert rc == ERR_UNSUPPORTED and 'sca_restart_scenes' in msg, msg
    finally:
        sol.close()


# ---- the Python layers -------------------------------------------------------------------------------------------------------------------
def mixed(E, i, first, kind, nd):
    a = E.Agent(start_pos=first[i][0], goal_pos=first[i][1], vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=kind, id=i)
    a.neighborDist = nd
    return a


def test_env_attribute_slots_and_its_mirrors(S, row_env):
    """MACAEnv(attribute_slots=True).respawn takes agents of another policy and neighborDist -- the mirrors follow the ADMITTED agents only --
    and equals the solver-level call; without the flag every ValueError stays; the env's checkpoint carries the current policies and
    attributes and resumes in a fresh env"""
    from sca_amd import env as E
    from test_gpu_vacancy import ring_env
    row_env(None)
    plain, first = ring_env(E)
    with pytest.raises(ValueError, match='a row keeps its policy'):
        plain.respawn([mixed(E, 3, first, E.ORCA3DPolicy, 10.0)])
    with pytest.raises(ValueError, match='a row keeps its attributes'):
        plain.respawn([mixed(E, 3, first, E.RVO3DPolicy, 4.0)])
    agents = E.build_circle_agents(16, policy=E.RVO3DPolicy, rad=4.0)
    env = E.MACAEnv(attribute_slots=True)
    env.set_agents(agents, obstacles=plain.obstacles)
    twin, _ = ring_env(E)
    assert env.per_agent_attributes == []
    for e in (env, twin):
        for _ in range(5):
            e.step()
    # agent 2 starts where agent 9 stands: refused under the gate, and its row keeps the old object, policy and mirrors
    new = [mixed(E, 1, first, E.ORCA3DPolicy, 4.0), mixed(E, 2, first, E.ORCA3DPolicyOfficial, 15.0), mixed(E, 6, first, E.SRVO3DPolicy, 10.0)]
    new[1]._pos = np.array(env.agents[9].pos_global_frame, dtype=np.float64)
    old2 = env.agents[2]
    admitted = env.respawn(new, margin=0.4)
    assert [a.id for a in admitted] == [1, 6] and env.agents[2] is old2 and env.agents[1] is new[0] and env.agents[6] is new[2]
    assert env.policy_ids.tolist() == [1, 3, 1, 1, 1, 1, 2] + [1] * 9 and env.per_agent_attributes == ['neighbor_dist']
    ids = np.array([1, 6], np.int32)
    start = np.array([first[i][0] for i in ids], np.float64)
    goal = np.array([first[i][1] for i in ids], np.float64)
    twin.solver.respawn(ids, start[:, :3], np.zeros((2, 3), np.float32), start[:, 3:6], [0.5, 0.5], [1.0, 1.0], goal[:, :3], [a.max_run_dist for a in admitted],
                        zaxis=S.zaxis_flags(start, goal), policy=[3, 2],
                        attrs={k: [conv(getattr(a, attr)) for a in admitted] for k, (attr, conv) in E._ATTRS.items()})
    for t in range(10):
        env.step()
        twin.solver.run_steps(1, S.NBR_KDTREE)
        same_step(S, env.solver, twin.solver, t)
    ck = env.checkpoint()
    back = E.MACAEnv.from_checkpoint(ck)
    assert back._attr_slots and back.policy_ids.tolist() == env.policy_ids.tolist() and back.agents[1].neighborDist == 4.0
    for t in range(5):
        env.step()
        back.step()
        same_step(S, env.solver, back.solver, t)
    # ... and the resumed env still takes another kind
    assert back.respawn([mixed(E, 0, first, E.ORCA3DPolicy, 2.5)]) is None and back.policy_ids[0] == 3


def test_run_lifelong_with_a_mixed_fleet_against_plain_calls(S, row_env):
    """run_lifelong on a MACAEnv(attribute_slots=True): arrivals of any policy and neighborDist enter any vacant row -- against the same loop
    written with env.step, env.finished, env.retire and env.respawn; without the flag the same arrivals are a ValueError"""
    from sca_amd import env as E
    from sca_amd.lifelong import RETIRE, run_lifelong
    from test_gpu_vacancy import ring_env
    row_env(None)
    steps = 120
    kinds = (E.ORCA3DPolicy, E.RVO3DPolicy, E.ORCA3DPolicyOfficial, E.SRVO3DPolicy)
    plain, first = ring_env(E)

    def make():
        env = E.MACAEnv(attribute_slots=True)
        env.set_agents(E.build_circle_agents(16, policy=E.RVO3DPolicy, rad=4.0), obstacles=plain.obstacles)
        return env

    def arrival(i, step):
        return mixed(E, i, first, kinds[(i + step) % 4], (4.0, 10.0, 15.0)[(i + step) % 3])

    def again(agent):
        return mixed(E, agent.id, first, type(agent.policy), agent.neighborDist)
    env = make()
    stats = run_lifelong(env, lambda agent, row: RETIRE if int(row['flags']) == 1 else again(agent), steps,
                         arrivals=lambda step, vacant: [arrival(i, step) for i in vacant[:2]] if step % 5 == 0 else [])
    assert stats['admitted'] > 0 and len(set(env.policy_ids.tolist())) > 1, (stats, env.policy_ids)
    assert [a.policy.policy_id for a in env.agents] == env.policy_ids.tolist()
    env2 = make()
    vacant, active = set(), env2._active
    for step in range(1, steps + 1):
        env2.step()
        new, leaving = [], []
        if env2._active < active:
            for row in env2.finished():
                i = int(row['id'])
                if int(row['flags']) == 1:
                    leaving.append(i)
                else:
                    new.append(again(env2.agents[i]))
        if leaving and len(leaving) >= 16 - len(vacant):
            leaving.pop()
        if leaving:
            env2.retire(leaving)
            vacant.update(leaving)
        free = sorted(vacant)
        new = new + ([arrival(i, step) for i in free[:2]] if free and step % 5 == 0 else [])
        if new:
            env2.respawn(new)
        vacant.difference_update(a.id for a in new)
        active = env2._active
    got, want = env.solver.get_state(), env2.solver.get_state()
    for k in F.STATE_KEYS:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(env.solver.get_kd_perm(), env2.solver.get_kd_perm()) and env.policy_ids.tolist() == env2.policy_ids.tolist()
    with pytest.raises(ValueError, match='a row keeps its'):
        run_lifelong(plain, lambda agent, row: RETIRE if int(row['flags']) == 1 else again(agent), steps,
                     arrivals=lambda step, vacant: [arrival(i, step) for i in vacant[:2]] if step % 5 == 0 else [])


def test_the_example_with_and_without_a_fleet(row_env):
    import subprocess
    import sys
    row_env(None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, os.path.join(root, 'examples', 'run_sca.py'), '--scenario', 'circle', '--agents', '32', '--policy', 'orca', '--no-obstacles', '--lifelong', '150',
            '--traffic', '0.3', '--spawn-margin', '0.5']
    env = dict(os.environ, PYTHONPATH=root)
    plain = subprocess.run(base, capture_output=True, text=True, cwd=root, env=env)
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-2000:]
    assert 'entered,' not in plain.stdout.split('population')[-1] and 'traffic 0.3 arrivals/step:' in plain.stdout, plain.stdout[-2000:]
    out = subprocess.run(base + ['--fleet', 'sca,orca,rvo'], capture_output=True, text=True, cwd=root, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('  ') and 'entered,' in ln]
    assert len(lines) >= 2 and any(ln.strip().startswith('SCAPolicy:') for ln in lines), out.stdout[-2000:]
    entered = sum(int(ln.split(':')[1].split()[0]) for ln in lines)
    admitted = int(out.stdout.split('drones left,')[1].split()[0])
    assert entered == admitted > 0, out.stdout[-2000:]


def test_env_an_orca_row_is_reentered_by_a_tracked_sca_drone_with_its_own_turning_radius(S, row_env):
    """the scenario the feature is for: MACAEnv(attribute_slots=True, device_tracker=True), a fleet of ORCA3D drones; rows are re-entered by
    Dubins-tracked SCA drones with another neighborDist and turning radius.  The env's checkpoint -- whose fresh env is defined through
    set_agents + sca_device_tracker_set_agent_params, the other route to the same attributes -- runs beside it, re-plan counts included"""
    from sca_amd import env as E
    row_env(None)
    agents = E.build_circle_agents(16, policy=E.ORCA3DPolicy, rad=6.0)
    first = {a.id: (list(a.initial_pos), list(a.goal_pos)) for a in agents}
    env = E.MACAEnv(attribute_slots=True, device_tracker=True)
    env.set_agents(agents, obstacles=[])
    for _ in range(5):
        env.step()
    new = []
    for i, R in ((3, 2.5), (8, 2.0), (12, 2.5)):
        a = mixed(E, i, first, E.SCAPolicy, 4.0)
        a.turning_radius = R
        new.append(a)
    assert env.respawn(new) is None
    assert env.policy_ids[[3, 8, 12]].tolist() == [0, 0, 0] and env._planner_of(3)[0] == 2.5 and env._planner_of(8)[0] == 2.0 and env._planner_of(0)[0] == 1.5
    assert 'turning_radius / pitchlims' in env.per_agent_attributes and 'neighbor_dist' in env.per_agent_attributes
    assert np.array_equal(env.solver.vpref_mode(), np.isin(np.arange(16), (3, 8, 12)).astype(np.uint8))
    for _ in range(3):
        env.step()
    back = E.MACAEnv.from_checkpoint(env.checkpoint())
    assert back.agents[3].turning_radius == 2.5 and back.policy_ids.tolist() == env.policy_ids.tolist()
    for t in range(12):
        env.step()
        back.step()
        same_step(S, env.solver, back.solver, t)
        assert np.array_equal(env.solver.device_tracker_replans(), back.solver.device_tracker_replans()), t
    assert env.solver.device_tracker_replans()[[3, 8, 12]].all(), 'the tracked drones never planned: the test shows nothing'
