"""Context checkpoints on the GPU (-m gpu): sca_save_context / sca_load_context.  Equality, no tolerance.

The TWIN: context A runs; a fresh context B is given the run's definition and loads A's blob taken behind step k; after every further step
of both, every getter of the contract is compared -- the state, the kd permutation, sca_active_count, sca_get_finished, status, the pass's
results on the rows the pass served (float32 action rows, neighbour lists and their distSq, diag, the v_pref used), and with the features
on: remaining / now_goal / the rooms whole / vpref_mode, tracker records and re-plan counts, mission cursors / ended / results / totals,
gate words and totals, closest-approach records.  Right behind the load the getters that read state return on B what they return on A, and
B's own save is A's blob byte for byte.  Against the RULE, so that the two cannot be wrong together: the gated corpus of
tests/mission_paths_rule.py resumed at step 6, steps 7 .. 12 compared with the rule as tests/test_gpu_mission_paths.py compares a context
that was never cut (what the corpus holds at the save: tests/test_context_checkpoint_cpu.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import form_fuzz as F
import mission_paths_rule as PR
import mission_rule as MR
from test_context_checkpoint_cpu import CORPUS_SAVE, CORPUS_SEEDS
from test_gpu_form_fuzz import compare_with_oracle
from test_gpu_mission_gate import check_gate_words
from test_gpu_mission_paths import check_lists, corpus_context, lists_for
from test_gpu_missions import behind, by_row, check_words, traffic_scene

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 12
W = PR.W


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


# ---- definitions -------------------------------------------------------------------------------------------------------------------------------
def fuzz_context(S, scene, extra=0, per_agent=None, paths=None, slots=None, perm=True, clearance=False):
    """a context of max_agents = n + extra that holds a fuzz scene as test_gpu_form_fuzz.context_of sets it up; slots = (W, lists): the
    lists in slot form"""
    s, n = scene, scene['n']
    sol = S.BatchedSolver(max_agents=n + extra, max_obstacles=max(1, s['m']), params=per_agent[1] if per_agent else None)
    try:
        sol.set_obstacles(s['obs_pos'], s['obs_radius'])
        sol.set_agents(s['radius'], s['pref_speed'], s['goal'], s['policy'], F.zaxis_of(s), s['max_run_dist'])
        if per_agent and not per_agent[2]:
            sol.set_agent_params(**per_agent[0])
        if paths is not None:
            sol.set_paths(paths)
        if slots is not None:
            sol.set_path_slots(*slots)
        sol.set_vpref(s['vpref'], s['vmode'])
        sol.set_state(s['pos'], s['vel'], s['heading'], s['flags'], np.zeros(n), np.zeros(n, np.int32))
        if perm:
            sol.set_kd_perm(np.arange(n, dtype=np.int32))
        if clearance:
            sol.clearance_enable()
    except BaseException:
        sol.close()
        raise
    return sol


def traffic_context(S, sc, extra=0, clearance=False, slots=None, missions=None, gate=None):
    """test_gpu_missions.context_for with max_agents = n + extra, and on top: slots = (W, initial lists), missions = (M, R, lists or None),
    gate = (margin, cap)"""
    n = sc['n']
    sol = S.BatchedSolver(max_agents=n + extra, max_obstacles=1)
    try:
        sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
        sol.set_agents(sc['radius'], np.ones(n), sc['goal'], sc['policy'], sc['zaxis'], sc['mrd'])
        sol.set_state(sc['start'], np.zeros((n, 3), np.float32), sc['heading'], np.zeros(n, np.uint8))
        if sc['tracker']:
            sol.device_tracker_enable(sc['gh'], in_pass=True)
        if clearance:
            sol.clearance_enable()
        if slots is not None:
            sol.set_path_slots(*slots)
        if missions is not None:
            M, R, lists = missions
            sol.set_missions(M, R, sc['entries'][:, :M], sc['first_ok'], sc['first_fail'], paths=None if lists is None else PR.flat_lists(lists))
        if gate is not None:
            sol.set_mission_gate(*gate)
    except BaseException:
        sol.close()
        raise
    return sol


# ---- what is compared ------------------------------------------------------------------------------------------------------------------------------
def features(info):
    return dict(tracker=bool(info['has_tracker']), lists=info['list_form'], tables=info['M'] > 0, gate=bool(info['has_gate']), clear=bool(info['has_clearance']))


def state_view(sol, f, active=True, results=False):
    """every getter that reads STATE, as a dict of arrays / bytes"""
    out = dict(sol.get_state())
    out['perm'] = sol.get_kd_perm()
    out['status'] = sol.diag()['status']
    out['vpref_mode'] = sol.vpref_mode()
    if active:
        out['active'] = np.array([sol.active_count()])
    out['finished'] = np.frombuffer(sol.finished().tobytes(), np.uint8)
    if f['lists']:
        out['remaining'], out['now_goal'] = sol.get_path_state()
    if f['lists'] == 2:
        out['len'], out['rooms'] = sol.path_slot_lists()
    if f['tracker']:
        out['replans'] = sol.device_tracker_replans()
        out['tracks'] = np.array([sol.device_tracker_debug(i) for i in range(0, sol.n, max(1, sol.n // 64))])
    if f['tables']:
        out['cursor'], out['ended'] = sol.mission_state()
        out['totals'] = np.array(list(sol.mission_totals().values()))
        if results:
            out['results'] = np.frombuffer(sol.mission_results().tobytes(), np.uint8)      # (marks them collected, on both contexts alike)
    if f['gate']:
        out['waiting'], out['verdict'], out['refusals'] = sol.mission_gate_state()
        out['gate_totals'] = np.array(list(sol.mission_gate_totals().values()))
    if f['clear']:
        out['clearance'] = np.frombuffer(sol.clearance().tobytes(), np.uint8)
    return out


def same_views(a, b, at):
    assert a.keys() == b.keys(), at
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, at + (k, x.shape, y.shape)
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == 'f'), at + (k, np.flatnonzero((x != y).reshape(len(x), -1).any(1))[:8])


def same_pass(A, B, served, at):
    """the last pass's results on the rows it served: the action rows and the v_pref used whole, the neighbour lists entry for entry up to
    their length, the decisions' diagnostics"""
    assert np.array_equal(A.actions()[served], B.actions()[served]), at + ('action',)
    na, nb = A.neighbors(), B.neighbors()
    for k in ('nbr_valid', 'nbr_n'):
        assert np.array_equal(na[k][served], nb[k][served]), at + (k,)
    inside = served[:, None] & (na['nbr_valid'] != 0)[:, None] & (np.arange(F.K)[None, :] < na['nbr_n'][:, None])
    for k in ('nbr_id', 'nbr_kind', 'nbr_dsq'):
        assert np.array_equal(na[k][inside], nb[k][inside]), at + (k,)
    da, db = A.diag(), B.diag()
    assert np.array_equal(da['diag'][served], db['diag'][served]), at + ('diag',)
    assert np.array_equal(da['vpref'][served], db['vpref'][served], equal_nan=True), at + ('v_pref used',)


def stepper_of(S, mode, form='run'):
    if form == 'pass+update':
        def step(sol, k=1):
            for _ in range(k):
                sol.policy_pass(mode)
                sol.env_update()
    elif form == 'env_step':
        def step(sol, k=1):
            for _ in range(k):
                sol.env_step(mode)
    else:
        def step(sol, k=1):
            sol.run_steps(k, mode)
            sol.synchronize()
    return step


def twin(S, make, k, step, at, steps=STEPS, per_call=1, results=True, at_save=None, grid=False):
    """A = make(0) runs k steps and is saved; B = make(37), a larger context with the same definition, loads the blob; both go on to
    `steps`, compared behind every call.  at_save(A, info): the caller's look at what the blob holds.  Returns the blob's header.
    grid: SCA_NBR_GRID -- on a row that collides in the pass SCA_ST_NBR_OVERFLOW may also stand because the list was full before the
    first colliding object was met, which depends on the order a cell hands its agents out: the arrival order of k_grid_count's atomics,
    which no state fixes (sca_grid.hip.h, include/sca_hip.h; tests/test_gpu_grid_fuzz.py allows the same against the oracle).  That one
    bit of such a row's status word is an output of the pass and is left out; every other bit of the word, and the whole word of every
    other row, is compared -- and one step later the word of such a row must be 0 on both contexts: the bit is read by nobody and does
    not outlive the next pass"""
    A = B = None
    try:
        A = make(0)
        if k:
            step(A, k)
        blob = A.save_context()
        info = S.context_checkpoint_info(blob)
        f = features(info)
        assert info['n'] == A.n and info['total_bytes'] == len(blob) == A.context_checkpoint_bytes() and info['state_fresh'] == (1 if k == 0 else 0), at + (info,)
        if at_save is not None:
            at_save(A, info)
        B = make(37)
        assert B.context_checkpoint_bytes() == len(blob), at
        B.load_context(blob)
        # (behind sca_set_state alone K4's counters have counted nothing yet: sca_active_count is compared from the first step on)
        same_views(state_view(A, f, active=k > 0), state_view(B, f, active=k > 0), at + ('behind the load',))
        assert B.save_context().tobytes() == blob.tobytes(), at + ('load, then save',)
        if k > 0:
            assert B.active_count() == int((B.get_state()['flags'] == 0).sum()), at + ('active_count behind the load',)
        gone = np.zeros(A.n, bool)
        for t in range(k, steps, per_call):
            served = (A.get_state()['flags'] & 7) == 0
            step(A, per_call)
            step(B, per_call)
            here = at + ('step', t + per_call)
            va, vb = state_view(A, f, results=results), state_view(B, f, results=results)
            if grid:
                for v in (va, vb):                                           # last step's colliding rows: the grid pass has written 0
                    assert not v['status'][gone].any(), here + ('the overflow bit of a row that collided outlived a pass', np.flatnonzero(v['status'] & gone)[:8])
                gone = served & ((va['flags'] & 2) != 0)
                for v in (va, vb):
                    v['status'] = np.where(gone, v['status'] & ~32, v['status'])
            same_views(va, vb, here)
            if per_call == 1:
                same_pass(A, B, served, here)
            else:                                                           # a burst: the rows that ran through all of it
                same_pass(A, B, served & ((A.get_state()['flags'] & 7) == 0), here)
        return info
    finally:
        for s in (A, B):
            if s is not None:
                s.close()


# ---- the twin on fuzz scenes, through the forms ----------------------------------------------------------------------------------------------------
FORMS = [('kd', None, 'run', 1), ('auto', None, 'run', 1), ('hostbuild', None, 'run', 1), ('kd', 'large_shard', 'run', 1), ('auto', 'large_shard', 'run', 1),
         ('kd', None, 'run', 3), ('auto', None, 'run', 3), ('kd', None, 'pass+update', 1), ('auto', None, 'env_step', 1)]


def mode_of(S, name):
    return dict(kd=S.NBR_KDTREE, auto=S.NBR_AUTO, hostbuild=S.NBR_KDTREE_HOSTBUILD, grid=S.NBR_GRID)[name]


@pytest.mark.parametrize('mode,row,form,per_call', FORMS)
@pytest.mark.parametrize('k', [0, 1, 6])
def test_twin_through_the_forms(S, row_env, mode, row, form, per_call, k):
    """fuzz scenes (mixed policies, obstacles, rows done from the start, fed v_pref), saved directly behind sca_set_state -- the one-time
    obstacle check still pending: an obstacle is put where a row that arrived stands --, behind step 1 and behind step 6"""
    row_env(row)
    if per_call == 3 and k == 1:
        k = 3
    for seed in (19, 5):
        scene = dict(F.random_scene(seed))
        arrived = np.flatnonzero(scene['flags'] == 1)
        if len(arrived) and scene['m']:
            scene['obs_pos'] = scene['obs_pos'].copy()
            scene['obs_pos'][0] = scene['pos'][arrived[0]]
        twin(S, lambda extra: fuzz_context(S, scene, extra), k, stepper_of(S, mode_of(S, mode), form), (mode, row, form, per_call, 'seed', seed, 'k', k), per_call=per_call)


@pytest.mark.parametrize('k', [0, 1, 6])
def test_twin_on_the_grid(S, row_env, k):
    """SCA_NBR_GRID on the scenes the grid takes (no tree: the permutation is left alone)"""
    row_env(None)
    whole = 0
    for seed in (12, 16, 19, 25, 31):
        scene = F.random_scene(seed)
        probe = fuzz_context(S, scene, perm=False)
        try:
            probe.run_steps(STEPS, S.NBR_GRID)
        except S.ScaError as e:
            assert 'SCA_NBR_GRID needs' in str(e), str(e)
            continue
        finally:
            probe.close()
        twin(S, lambda extra: fuzz_context(S, scene, extra, perm=False), k, stepper_of(S, S.NBR_GRID), ('grid', 'seed', seed, 'k', k), grid=True)
        whole += 1
    assert whole >= 1, whole


def ending_scene(n=40):
    """straight-line agents 3 m apart on a line, each with its goal 0.6 .. 1.3 m ahead: they arrive one after the other within a few steps"""
    i = np.arange(n)
    pos = np.stack([3.0 * i, np.zeros(n), np.full(n, 5.0)], 1)
    goal = pos + np.stack([np.zeros(n), 0.6 + 0.1 * (i % 8), np.zeros(n)], 1)
    head = np.zeros((n, 3))
    head[:, 0] = np.pi / 2
    return dict(n=n, m=0, pos=pos, goal=goal, heading=head, vel=np.zeros((n, 3), np.float32), radius=np.full(n, 0.3), pref_speed=np.ones(n),
                policy=np.array([1, 2, 3, 4], np.uint8)[i % 4], flags=np.zeros(n, np.uint8), obs_pos=np.zeros((0, 3)), obs_radius=np.zeros(0),
                vpref=np.zeros((n, 3)), vmode=np.zeros(n, np.uint8), max_run_dist=np.full(n, 50.0), key=('ending', n))


@pytest.mark.parametrize('mode', ['kd', 'auto'])
def test_twin_behind_the_step_in_which_the_last_row_finishes(S, row_env, mode):
    row_env(None)
    scene = ending_scene()
    probe = fuzz_context(S, scene)
    try:
        last = next(t + 1 for t in range(STEPS) if probe.env_step(mode_of(S, mode)) == 0)
    finally:
        probe.close()
    assert 2 <= last < STEPS, last

    def at_save(A, info):
        assert A.active_count() == 0 and (A.get_state()['flags'] != 0).all()
    twin(S, lambda extra: fuzz_context(S, scene, extra), last, stepper_of(S, mode_of(S, mode)), ('ending', mode, 'k', last), at_save=at_save)
    twin(S, lambda extra: fuzz_context(S, scene, extra), last - 1, stepper_of(S, mode_of(S, mode)), ('ending', mode, 'k', last - 1))


# ---- against the rule --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', CORPUS_SEEDS)
def test_the_gated_corpus_resumed_at_step_6_against_the_rule(S, oracle, row_env, seed):
    """tables + gate (margin 0.5) + lists: A runs steps 1 .. 6 in one burst and collects nothing; B, a fresh context with the definition,
    loads A's blob and runs steps 7 .. 12 against tests/mission_paths_rule.py as tests/test_gpu_mission_paths.py's run_corpus does"""
    row_env(None)
    scene = F.random_scene(seed)
    gate, R = (PR.GATE_MARGIN, 0), 4
    run = PR.oracle_run(oracle, scene, STEPS, gate=gate)
    A = corpus_context(S, scene, run, R, gate=gate)
    try:
        A.run_steps(CORPUS_SAVE, S.NBR_KDTREE)
        blob = A.save_context()
    finally:
        A.close()
    sol = corpus_context(S, scene, run, R, gate=gate)
    try:
        sol.load_context(blob)
        first = 0                                                          # the first step whose results nobody has collected
        for t in range(CORPUS_SAVE, STEPS):
            at = ('resumed corpus', 'seed', seed, 'n', scene['n'], 'step', t)
            sol.run_steps(1, S.NBR_KDTREE)
            sol.synchronize()
            assert sol.pass_forms() & S.FORM_WAYPOINTS, at
            r = run['steps'][t]
            compare_with_oracle(sol, behind(r), scene, at)
            check_lists(sol, r, scene, at)
            assert sol.active_count() == r['active'], at + ('active_count', sol.active_count(), r['active'])
            assert np.array_equal(sol.finished()['id'], r['finished']), at + ('finished ids',)
            check_words(sol, r, at)
            check_gate_words(sol, r['waiting'], r['verdict'], r['refusals'], r['gate_totals'], at)
            want = by_row([s['results'] for s in run['steps'][first:t + 1]])
            keep = np.ones(len(want), bool)                                 # a row's last R results
            for a in np.unique(want['id']):
                keep[np.flatnonzero(want['id'] == a)[:-R]] = False
            assert sol.mission_results().tobytes() == want[keep].tobytes(), at + ('results',)
            first = t + 1
    finally:
        sol.close()


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 255, 256, 257, 2049])
def test_sizes_save_load_save(S, row_env, n):
    """one row, one below / at / one above the copy kernels' 256-lane workgroup, and 2049: a blob loaded into a fresh, larger context and
    saved from it again is the blob; one more step of both agrees"""
    row_env(None)
    scene = F.switch_scene(n)
    twin(S, lambda extra: fuzz_context(S, scene, extra), 2, stepper_of(S, S.NBR_KDTREE), ('size', n), steps=3)


# ---- each feature alone, and all together ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [33, 48, 64])
def test_the_device_tracker(S, row_env, n):
    """plans and re-plan counts word for word for six steps behind the load"""
    row_env(None)
    sc = traffic_scene(n, True)

    def at_save(A, info):
        assert info['has_tracker'] == 1 and info['trk_words'] == 112 and A.device_tracker_replans().sum() > 0
    twin(S, lambda extra: traffic_context(S, sc, extra), 6, stepper_of(S, S.NBR_KDTREE), ('tracker', n), at_save=at_save)


def test_per_agent_attributes(S, row_env):
    row_env(None)
    for seed in (1001, 1004):
        scene = F.random_scene(seed)
        per = F.per_agent_attributes(seed, scene['n'])
        twin(S, lambda extra: fuzz_context(S, scene, extra, per_agent=per), 6, stepper_of(S, S.NBR_KDTREE), ('per agent', seed))


def test_block_form_lists(S, row_env):
    row_env(None)
    for seed, mode in ((19, 'kd'), (5, 'auto')):
        scene = F.random_scene(seed)
        paths = F.random_paths(seed, scene)

        def at_save(A, info):
            rem, ng = A.get_path_state()
            assert info['list_form'] == 1 and (rem < [len(p) for p in paths]).any() and not np.isnan(ng[:, 0]).all()
        twin(S, lambda extra: fuzz_context(S, scene, extra, paths=paths), 6, stepper_of(S, mode_of(S, mode)), ('block lists', seed, mode), at_save=at_save)


def test_slot_form_lists_after_host_respawns_changed_them(S, row_env):
    """A respawns its finished rows behind steps 2 and 4 with new missions and new lists; B is given the lists as they were SET -- what the
    respawns made of the rows' constants, lengths and rooms comes from the blob"""
    row_env(None)
    seed = 19
    scene = F.random_scene(seed)
    n = scene['n']
    initial = PR.initial_paths(seed, scene)
    rng = np.random.default_rng(seed)

    def make(extra):
        return fuzz_context(S, scene, extra, slots=(W, initial))

    def step(sol, k=1):
        """A's steps before the save carry the respawns; every later call is a plain step"""
        for _ in range(k):
            sol.run_steps(1, S.NBR_KDTREE)
            sol.synchronize()
            if step.respawns and step.count in (1, 3):
                ids = sol.finished()['id']
                assert len(ids) > 0
                m = len(ids)
                pos = rng.uniform(-40, 40, (m, 3)) + [0, 0, 100.0]
                lists = [[[float(x) for x in np.round(pos[j] + [1.0 + q, 0.5, 0.0], 3)] for q in range((j % (W + 1)))] for j in range(m)]
                goal = pos + np.where((np.arange(m) % 2 == 0)[:, None], [0.3, 0.0, 0.0], [5.0, 0.0, 0.0])      # every second one arrives at once: it is respawned again
                sol.respawn(ids, pos, np.zeros((m, 3), np.float32), np.zeros((m, 3)), rng.choice([0.3, 0.6], m), rng.choice([0.9, 1.7], m), goal,
                            np.full(m, 30.0), zaxis=np.zeros(m, np.uint8), paths=lists)
            step.count += 1
    step.respawns, step.count = True, 0

    def at_save(A, info):
        step.respawns = False
        ln, rooms = A.path_slot_lists()
        assert info['list_form'] == 2 and info['W'] == W and (ln != [len(p) for p in initial]).any()
    twin(S, make, 6, step, ('slot lists', seed), at_save=at_save)


def test_tables_with_r_1_and_an_overflowed_ring(S, row_env):
    """nothing is collected before the save: rows that ended more than once have overwritten their one-slot ring"""
    row_env(None)
    sc = traffic_scene(48, False)

    def at_save(A, info):
        cursor, ended = A.mission_state()
        assert info['M'] == 3 and info['R'] == 1 and info['updates'] == 8 and (ended >= 2).any(), ended
    twin(S, lambda extra: traffic_context(S, sc, extra, missions=(3, 1, None)), 8, stepper_of(S, S.NBR_KDTREE), ('R = 1',), at_save=at_save)


def test_a_gate_with_rows_waiting(S, row_env):
    row_env(None)
    sc = traffic_scene(48, False)

    def at_save(A, info):
        waiting, verdict, refusals = A.mission_gate_state()
        assert info['has_gate'] == 1 and (waiting >= 0).any() and A.mission_gate_totals()['admitted'] > 0, waiting
    twin(S, lambda extra: traffic_context(S, sc, extra, missions=(3, 2, None), gate=(0.5, 0)), 6, stepper_of(S, S.NBR_KDTREE), ('gate',), at_save=at_save)


def test_closest_approach_records(S, row_env):
    """the resumed records are the uninterrupted run's: no merge, the step numbers go on counting from the save"""
    row_env(None)
    scene = F.random_scene(19)

    def at_save(A, info):
        c = A.clearance()
        assert info['has_clearance'] == 1 and info['clear_step'] == 6 and (c['agent_step'] > 0).any()
    twin(S, lambda extra: fuzz_context(S, scene, extra, clearance=True), 6, stepper_of(S, S.NBR_KDTREE), ('clearance',), at_save=at_save)
    twin(S, lambda extra: fuzz_context(S, scene, extra, clearance=True), 6, stepper_of(S, S.NBR_AUTO), ('clearance', 'auto'))


def test_23_obstacles(S, row_env):
    row_env(None)
    scene = dict(F.random_scene(19))
    rng = np.random.default_rng(23)
    scene.update(m=23, obs_pos=np.concatenate([scene['pos'][:8] + [1.2, 0.0, 0.0], rng.uniform(-30, 30, (15, 3))]), obs_radius=rng.choice([0.2, 1.0, 2.0], 23), key=('obstacles', 23))
    twin(S, lambda extra: fuzz_context(S, scene, extra, clearance=True), 6, stepper_of(S, S.NBR_KDTREE), ('23 obstacles',))


@pytest.mark.parametrize('n,mode', [(48, 'kd'), (33, 'auto')])
def test_all_features_together(S, row_env, n, mode):
    """the device tracker, lists in slot form, tables whose entries bring lists, the gate, closest-approach records"""
    row_env(None)
    sc = traffic_scene(n, True)
    lists, initial = lists_for(sc)

    def at_save(A, info):
        assert (info['has_tracker'], info['list_form'], info['W'], info['M'], info['R'], info['has_gate'], info['has_clearance']) == (1, 2, W, 3, 2, 1, 1), info
        assert A.mission_totals()['taken'] > 0
    twin(S, lambda extra: traffic_context(S, sc, extra, clearance=True, slots=(W, initial), missions=(3, 2, lists), gate=(0.5, 0)), 6,
         stepper_of(S, mode_of(S, mode)), ('all', n, mode), at_save=at_save)


# ---- another process ---------------------------------------------------------------------------------------------------------------------------------
CHILD = r'''
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import numpy as np
import form_fuzz as F
import sca_amd.solver as S
from sca_amd.checkpoint import ContextCheckpoint
from test_gpu_context_checkpoint import fuzz_definition
scene = F.random_scene(19)
d = fuzz_definition(scene, F.random_paths(19, scene))
sol = ContextCheckpoint(d, None, 0).solver()
sol.run_steps(6, S.NBR_KDTREE)
ContextCheckpoint(d, sol.save_context(), 6).write(sys.argv[1])
sol.close()
'''


def fuzz_definition(scene, paths):
    from sca_amd.checkpoint import ContextCheckpoint
    s, n = scene, scene['n']
    return ContextCheckpoint.define(radius=s['radius'], pref_speed=s['pref_speed'], goal=s['goal'], policy=s['policy'], zaxis=F.zaxis_of(s), max_run_dist=s['max_run_dist'],
                                    obstacles=(s['obs_pos'], s['obs_radius']), state=dict(pos=s['pos'], vel=s['vel'], heading=s['heading'], flags=s['flags']),
                                    vpref=(s['vpref'], s['vmode']), lists=('block', paths), clearance=True, neighbor_mode=0)


def test_written_in_a_child_process_resumed_in_this_one(S, row_env, tmp_path):
    """the child runs six steps, writes the .npz and exits; this process reads it, resumes, and ends where its own uncut run ends"""
    from sca_amd.checkpoint import ContextCheckpoint
    row_env(None)
    path = str(tmp_path / 'run.npz')
    run = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests')), path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    with np.load(path, allow_pickle=False) as z:
        assert all(z[k].dtype != object for k in z.files)
    ck = ContextCheckpoint.read(path)
    scene = F.random_scene(19)
    A = B = None
    try:
        A = fuzz_context(S, scene, paths=F.random_paths(19, scene), clearance=True)
        A.run_steps(6, S.NBR_KDTREE)
        B = ck.solver(max_agents=scene['n'] + 11)
        assert ck.steps == 6 and B.save_context().tobytes() == ck.blob.tobytes() == A.save_context().tobytes()
        f = features(S.context_checkpoint_info(ck.blob))
        for t in range(6, STEPS):
            served = (A.get_state()['flags'] & 7) == 0
            A.run_steps(1, S.NBR_KDTREE)
            B.run_steps(1, S.NBR_KDTREE)
            same_views(state_view(A, f), state_view(B, f), ('child', t))
            same_pass(A, B, served, ('child', t))
    finally:
        for s in (A, B):
            if s is not None:
                s.close()


# ---- the Python layers ---------------------------------------------------------------------------------------------------------------------------
def traffic_env(n=16, K=2, tracker=False, clearance=True):
    """examples/run_sca.py --lifelong --device-missions [--waypoints K] as objects: the circle among the eight spheres, every drone with the
    ping-pong table of three entries whose legs follow routes of K seeded waypoints; (env, tables)"""
    import math
    from sca_amd import env as E, scenarios
    pol = E.SCAPolicy if tracker else E.ORCA3DPolicy
    sc = scenarios.circle(n, rad=10.0)
    obstacles = [E.Obstacle(pos=[round(4.0 * math.cos(2 * j * math.pi / 8), 2), round(4.0 * math.sin(2 * j * math.pi / 8), 2), 5.0],
                            shape_dict={'shape': 'sphere', 'feature': 1.0}, id=j) for j in range(8)]
    agents = [E.Agent(start_pos=list(sc['start'][i]), goal_pos=list(sc['goal'][i]), vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=pol, id=i) for i in range(n)]
    agents[3].neighborDist, agents[5].maxNeighbors = 7.5, 9                   # (per-agent attributes travel with the definition)
    first = {a.id: (list(a.initial_pos), list(a.goal_pos)) for a in agents}
    route = {}
    for i, (start, goal) in first.items():
        rng = np.random.default_rng(1000 + i)
        p, g = np.asarray(start[:3], float), np.asarray(goal[:3], float)
        route[i] = [[float(x) for x in np.round(p + (g - p) * (k + 1) / (K + 1) + rng.normal(0.0, 0.5, 3), 3)] for k in range(K)]
    if K:
        for a in agents:
            a.path = [w[:] for w in route[a.id][::-1]]
    env = E.MACAEnv(device_tracker=tracker, clearance=clearance, path_slots=K)
    env.set_agents(agents, obstacles=obstacles)

    def entry(i, start, goal):
        e = E.Agent(start_pos=start, goal_pos=goal, vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=pol, id=i)
        e.neighborDist, e.maxNeighbors = agents[i].neighborDist, agents[i].maxNeighbors
        return e
    tables = {i: E.MissionTable([entry(i, goal, start), entry(i, start, goal), entry(i, start, goal)], next_ok=[1, 0, 0], next_fail=[2, 2, 2], first_ok=0, first_fail=2,
                                start_here=[True, True, False], path=[route[i][:], route[i][::-1], route[i][::-1]] if K else None) for i, (start, goal) in first.items()}
    return env, tables


MIRRORS = ('initial_pos', 'goal_pos', 'goal_global_frame', 'goal_heading_frame', 'pos_global_frame', 'vel_global_frame', 'heading_global_frame')


def same_mirrors(A, B, at):
    """what env.agents shows on both envs: start, goal, radius, pref_speed, max_run_dist, the path as the passes have left it, the flags, the state"""
    for a, b in zip(A.agents, B.agents):
        here = at + ('agent', a.id)
        assert type(a.policy) is type(b.policy) and a.id == b.id, here
        for k in MIRRORS:
            assert np.array_equal(getattr(a, k), getattr(b, k)), here + (k, getattr(a, k), getattr(b, k))
        for k in ('radius', 'pref_speed', 'max_run_dist', 'neighborDist', 'maxNeighbors', 'is_at_goal', 'is_collision', 'is_out_of_max_time', 'total_dist', 'step_num'):
            assert getattr(a, k) == getattr(b, k), here + (k, getattr(a, k), getattr(b, k))
        assert a.path == b.path, here + ('path', a.path, b.path)
    assert A._active == B._active and np.array_equal(A.solver.get_kd_perm(), B.solver.get_kd_perm()), at


@pytest.mark.parametrize('tracker,margin', [(False, None), (False, 0.5), (True, 0.5)])
def test_from_checkpoint_mirrors(S, row_env, tmp_path, tracker, margin):
    """an env cut at step 300 of its traffic: the env read back from the file shows the checkpoint's values at once -- agents that fly their
    second or third mission have the entry's start, goal and route --, and both envs go on alike on the standing tables"""
    from sca_amd import env as E
    from sca_amd.checkpoint import ContextCheckpoint
    from sca_amd.lifelong import run_missions
    row_env(None)
    A, tables = traffic_env(tracker=tracker)
    B = None
    try:
        path = str(tmp_path / 'env.npz')
        first = run_missions(A, tables, 400, burst=4, spawn_margin=margin, checkpoint_at=(300, path))
        assert first['steps'] == 300 and first['respawned'] > 0, first
        ck = ContextCheckpoint.read(path)
        assert ck.steps == 300 and len(ck) == 16
        B = E.MACAEnv.from_checkpoint(ck)
        moved = [a.id for a in B.agents if not np.array_equal(a.goal_pos, tables[a.id].entries[1][0].goal_pos)]
        assert moved, 'no agent flies back at the cut'
        same_mirrors(A, B, ('behind the load',))
        assert B.solver.save_context().tobytes() == ck.blob.tobytes() == A.solver.save_context().tobytes()
        for chunk in range(3):
            sa, sb = run_missions(A, None, 20, burst=4), run_missions(B, None, 20, burst=4)
            assert sa == sb and sa['steps'] == 320 + 20 * chunk and (margin is None) == ('waiting' not in sa), (sa, sb)
            same_mirrors(A, B, ('chunk', chunk))
            assert A.clearance.tobytes() == B.clearance.tobytes()
    finally:
        for e in (A, B):
            if e is not None and e.solver is not None:
                e.solver.close()


@pytest.mark.parametrize('margin,burst', [(None, 8), (0.5, 8), (0.5, 1)])
def test_run_missions_cut_at_300_of_600_and_resumed(S, row_env, tmp_path, margin, burst):
    """the stats of the resumed run are the stats of the run that was never cut"""
    from sca_amd import env as E
    from sca_amd.checkpoint import ContextCheckpoint
    from sca_amd.lifelong import run_missions
    row_env(None)
    envs = []
    try:
        whole_env, tables = traffic_env()
        envs.append(whole_env)
        whole = run_missions(whole_env, tables, 600, burst=burst, spawn_margin=margin)
        cut_env, tables = traffic_env()
        envs.append(cut_env)
        path = str(tmp_path / 'cut.npz')
        half = run_missions(cut_env, tables, 600, burst=burst, spawn_margin=margin, checkpoint_at=(300, path))
        assert half['steps'] == 300 and half != whole
        resumed = E.MACAEnv.from_checkpoint(ContextCheckpoint.read(path))
        envs.append(resumed)
        rest = run_missions(resumed, None, 300, burst=burst)
        assert rest == whole and whole['steps'] == 600 and whole['respawned'] > 16, (rest, whole)
        assert np.array_equal(resumed.pos, whole_env.pos) and np.array_equal(resumed.flags, whole_env.flags)
    finally:
        for e in envs:
            if e.solver is not None:
                e.solver.close()


def test_the_example_saved_and_resumed_against_one_run(row_env, tmp_path):
    """examples/run_sca.py: --save-at 200 and --resume against the run that was never cut -- the last line is the same"""
    row_env(None)
    common = [sys.executable, os.path.join(ROOT, 'examples', 'run_sca.py'), '--policy', 'orca', '--lifelong', '400', '--device-missions', '--waypoints', '2', '--burst', '8']
    f = str(tmp_path / 'example.npz')

    def last_line(extra):
        run = subprocess.run(common + extra, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
        return run.stdout.strip().split('\n')
    whole = last_line([])[-1]
    saved = last_line(['--save-at', '200', '--save-file', f])
    assert any(x.startswith('saved behind step 200') for x in saved) and os.path.exists(f) and saved[-1] != whole, saved
    assert last_line(['--resume', f])[-1] == whole and whole.startswith("{'arrived':"), whole


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
def refused(S, call, code, *words):
    with pytest.raises(S.ScaError) as e:
        call()
    msg = str(e.value)
    assert '(rc=%d)' % code in msg and all(w in msg for w in words), msg


def test_refusals_of_both_calls(S, row_env):
    """every refusal with its code, decided before any device work: around each refused load the context's own save is byte-equal"""
    row_env(None)
    sc = traffic_scene(33, True)
    lists, initial = lists_for(sc)
    full = dict(clearance=True, slots=(W, initial), missions=(3, 2, lists), gate=(0.5, 0))
    A = traffic_context(S, sc, **full)
    made = []

    def ctx(**kw):
        made.append(traffic_context(S, sc if 'sc' not in kw else kw.pop('sc'), **kw))
        return made[-1]
    try:
        A.run_steps(4, S.NBR_KDTREE)
        blob = A.save_context()
        off = S.context_checkpoint_info(blob)['offsets']

        def unchanged(sol, load, code, *words):
            before = sol.save_context()
            refused(S, load, code, *words)
            assert sol.save_context().tobytes() == before.tobytes(), words
        # the blob against the context, each named
        plain = dict(sc, tracker=False)
        unchanged(ctx(sc=plain, **full), lambda: made[-1].load_context(blob), ERR_ARG, 'tracker')        # a blob with the tracker into a context without it
        unchanged(ctx(**dict(full, slots=(W + 1, initial), missions=None, gate=None)), lambda: made[-1].load_context(blob), ERR_ARG, 'lists, W')     # W = 3 into W = 4
        unchanged(ctx(**dict(full, slots=None, missions=(3, 2, None))), lambda: made[-1].load_context(blob), ERR_ARG, 'lists')
        unchanged(ctx(**dict(full, missions=None, gate=None)), lambda: made[-1].load_context(blob), ERR_ARG, 'tables')
        unchanged(ctx(**dict(full, missions=(3, 1, lists))), lambda: made[-1].load_context(blob), ERR_ARG, 'tables')
        unchanged(ctx(**dict(full, gate=None)), lambda: made[-1].load_context(blob), ERR_ARG, 'gate')
        unchanged(ctx(**dict(full, clearance=False)), lambda: made[-1].load_context(blob), ERR_ARG, 'clearance')
        other = dict(sc, policy=np.where(np.arange(33) == 7, 5 - sc['policy'], sc['policy']).astype(np.uint8))
        unchanged(ctx(sc=other, **full), lambda: made[-1].load_context(blob), ERR_ARG, 'policy', 'row 7')
        small = traffic_scene(32, True)
        l32, i32 = lists_for(small)
        unchanged(ctx(sc=small, **dict(full, slots=(W, i32), missions=(3, 2, l32))), lambda: made[-1].load_context(blob), ERR_ARG, 'n:')
        # the envelope and the payload, into a context that would take the blob
        B = ctx(**full)

        def bad(edits, seal=True):
            b = blob.copy()
            for at, v in edits:
                b[at] = v
            if seal:                                                        # the sum by the header's own words: FNV-1a over 64-bit words
                h, words = 0xcbf29ce484222325, np.frombuffer(b[128:].tobytes(), '<u8')
                for w in words.tolist():
                    h = ((h ^ w) * 0x100000001b3) & 0xffffffffffffffff
                b[72:80] = np.frombuffer(np.array([h], '<u8').tobytes(), np.uint8)
            return b
        assert S.context_checkpoint_info(bad([]))['checksum'] == S.context_checkpoint_info(blob)['checksum']
        unchanged(B, lambda: B.load_context(blob[:100]), ERR_ARG, 'shorter')
        unchanged(B, lambda: B.load_context(blob[:-16]), ERR_ARG, 'byte count')
        unchanged(B, lambda: B.load_context(bad([(0, 0)])), ERR_ARG, 'magic')
        unchanged(B, lambda: B.load_context(bad([(4, 2)])), ERR_ARG, 'format')
        unchanged(B, lambda: B.load_context(bad([(20, 40)])), ERR_ARG, 'record')
        unchanged(B, lambda: B.load_context(bad([(off[2] + 5, 1)], seal=False)), ERR_ARG, 'checksum')
        unchanged(B, lambda: B.load_context(bad([(off[12], blob[off[12] + 4])])), ERR_ARG, 'permutation')
        unchanged(B, lambda: B.load_context(bad([(off[1] + 36, 8)])), ERR_ARG, 'flag')
        unchanged(B, lambda: B.load_context(bad([(off[1] + 6, 0xf0), (off[1] + 7, 0x7f)])), ERR_ARG, 'not finite')
        unchanged(B, lambda: B.load_context(bad([(off[1] + 47, 0xbf)])), ERR_ARG, 'not positive')
        unchanged(B, lambda: B.load_context(bad([(off[18], W + 1)])), ERR_ARG, 'list length')
        unchanged(B, lambda: B.load_context(bad([(off[16] + 3, 0x80)])), ERR_ARG, 'cursor outside')
        unchanged(B, lambda: B.load_context(bad([(off[20] + 4 * 2 * 33, 3), (off[20] + 4 * 2 * 33 + 1, 0), (off[20] + 4 * 2 * 33 + 2, 0), (off[20] + 4 * 2 * 33 + 3, 0)])), ERR_ARG, 'M - 1')
        unchanged(B, lambda: B.load_context(bad([(off[20] + 4 * 5 * 33 + 3, 0x7f)])), ERR_ARG, 'collected')
        unchanged(B, lambda: B.load_context(bad([(off[23] + 4 * 1 * 33, 5)])), ERR_ARG, 'verdict')
        unchanged(B, lambda: B.load_context(bad([(off[25] + 16, 33), (off[25] + 17, 0), (off[25] + 18, 0), (off[25] + 19, 0)])), ERR_ARG, 'partner')
        unchanged(B, lambda: B.load_context(bad([(off[15] + k, 0xff) for k in range(448)])), ERR_ARG, 'tracker record')
        B.load_context(blob)                                                # ... and the blob itself is taken
        assert B.save_context().tobytes() == blob.tobytes()
        # the calls' own rules
        import ctypes as C
        buf = np.zeros(len(blob), np.uint8)
        assert A.L.sca_save_context(A.ctx, None, len(blob)) == ERR_ARG and A.L.sca_load_context(A.ctx, None, len(blob)) == ERR_ARG
        assert A.L.sca_save_context(A.ctx, C.c_void_p(buf.ctypes.data), len(blob) - 1) == ERR_ARG
        assert str(len(blob)) in A.L.sca_last_error(A.ctx).decode()
        assert not buf.any()
        A.policy_pass(S.NBR_KDTREE)
        refused(S, A.save_context, ERR_STATE, 'between a policy pass')
        refused(S, lambda: A.load_context(blob), ERR_STATE, 'between a policy pass')
        A.env_update()
        fresh = S.BatchedSolver(max_agents=33, max_obstacles=1)
        made.append(fresh)
        refused(S, fresh.save_context, ERR_STATE, 'sca_set_agents')
        refused(S, lambda: fresh.load_context(blob), ERR_STATE, 'sca_set_agents')
        fresh.set_obstacles(np.zeros((0, 3)), np.zeros(0))
        fresh.set_agents(sc['radius'], np.ones(33), sc['goal'], sc['policy'], sc['zaxis'], sc['mrd'])
        refused(S, fresh.save_context, ERR_STATE, 'no state')
        refused(S, lambda: fresh.load_context(blob), ERR_STATE, 'no state')
        fresh.set_state(sc['start'], np.zeros((33, 3), np.float32), sc['heading'], np.zeros(33, np.uint8))
        fresh.set_shard(0, 20)
        refused(S, fresh.save_context, ERR_UNSUPPORTED, 'shard')
        refused(S, lambda: fresh.load_context(blob), ERR_UNSUPPORTED, 'shard')
        fresh.set_shard(0, 33)
        fresh.set_scenes([0, 16, 33])
        refused(S, fresh.save_context, ERR_UNSUPPORTED, 'scenes')
        refused(S, lambda: fresh.load_context(blob), ERR_UNSUPPORTED, 'scenes')
    finally:
        A.close()
        for s in made:
            s.close()


def test_refusals_under_the_partition(S, row_env):
    row_env(None)
    sol = traffic_context(S, traffic_scene(33, False))
    try:
        blob = sol.save_context()
        sol.partition_init(0, 1)
        refused(S, sol.save_context, ERR_UNSUPPORTED, 'partition')
        refused(S, lambda: sol.load_context(blob), ERR_UNSUPPORTED, 'partition')
    finally:
        sol.close()
