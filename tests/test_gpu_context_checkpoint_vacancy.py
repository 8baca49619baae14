"""Context checkpoints with vacant rows on the GPU (-m gpu): sca_save_context_opt / sca_load_context_opt / sca_context_checkpoint_bytes_opt
with SCA_CHECKPOINT_VACANCY.  Equality, no tolerance.

The corpus is tests/vacancy_rule.py's (retires, admissions and respawns before every step, against the oracle on the occupied rows): a
context A runs it up to a save point, a fresh and larger context B loads A's blob and goes on with the corpus' calls, every row, list and
the whole permutation against the rule behind every call and step.  Twins: A goes on beside B, both take the same later retires and
admissions, and every getter that reads state, the pass's results and the contexts' own blobs agree behind every call."""
import os
import subprocess
import sys

import numpy as np
import pytest

import form_fuzz as F
import mission_paths_rule as PR
import vacancy_rule as V
from test_context_checkpoint_vacancy_cpu import SAVE_POINTS
from test_gpu_context_checkpoint import (ROOT, features, fuzz_context, same_pass, same_views, state_view, traffic_context)
from test_gpu_mission_paths import lists_for
from test_gpu_missions import traffic_scene
from test_gpu_respawn import mission_for, respawn
from test_gpu_vacancy import check_calls, check_step, sized_scene

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5
W = PR.W
EXTRA = 37                                                          # B is this much larger than A


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


def refused(S, call, code, *words):
    with pytest.raises(S.ScaError) as e:
        call()
    msg = str(e.value)
    assert '(rc=%d)' % code in msg and all(w in msg for w in words), msg


def closed(*sols):
    for s in sols:
        if s is not None:
            s.close()


def vacant_outputs(sol, vac, at):
    """what a retire leaves of the last pass's outputs and no pass writes again: a zero action row, no list, diag -1"""
    nb, dg = sol.neighbors(), sol.diag()
    assert not sol.actions()[vac].any() and not nb['nbr_valid'][vac].any() and not nb['nbr_n'][vac].any() and (dg['diag'][vac] == -1).all(), at + ('the vacant rows\' outputs',)


# ---- the vacancy corpus against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', SAVE_POINTS)
@pytest.mark.parametrize('row,mode', [(None, 'kd'), (None, 'hostbuild'), (None, 'auto'), ('large_shard', 'kd')])
def test_the_corpus_resumed_against_the_oracle(S, oracle, row_env, row, mode, k):
    """A runs the corpus' calls and steps 0 .. k-1 and is saved behind step k; B, fresh and 37 rows larger, holds the scene as it was first
    set up, loads the blob and goes on with the corpus' calls and steps k .. 11 against the rule"""
    row_env(row)
    nbr = dict(kd=S.NBR_KDTREE, hostbuild=S.NBR_KDTREE_HOSTBUILD, auto=S.NBR_AUTO)[mode]
    held = 0
    for seed in V.SEEDS[:10]:
        scene = F.random_scene(seed)
        n = scene['n']
        ref = V.oracle_run(oracle, scene)
        A = B = None
        try:
            A = fuzz_context(S, scene)
            for r in ref[:k]:
                if r['retire'] is not None:
                    A.retire(r['retire'])
                if r['mission'] is not None:
                    respawn(A, r['mission'])
                A.run_steps(1, nbr)
            last = ref[k - 1]
            vac = last['vacant']
            m = n - int(vac.sum())
            at = (row, mode, 'seed', seed, 'n', n, 'k', k, 'm', m)
            blob = A.save_context(vacancy=True)
            info = S.context_checkpoint_info(blob)
            assert info['occupied'] == m and info['n'] == n and len(blob) == A.context_checkpoint_bytes(vacancy=True), at
            B = fuzz_context(S, scene, EXTRA)
            B.load_context(blob, vacancy=True)
            check_calls(B, last, last['perm'], vac, at + ('behind the load',), int((~vac & ((last['flags'] & 7) == 0)).sum()))
            vacant_outputs(B, vac, at)
            assert B.save_context(vacancy=True).tobytes() == blob.tobytes(), at + ('load, then save',)
            held += int(m < n)
            for t in range(k, V.STEPS):
                r = ref[t]
                here = at + ('step', t)
                if r['retire'] is not None:
                    B.retire(r['retire'])
                if r['mission'] is not None:
                    respawn(B, r['mission'])
                check_calls(B, r['state_call'], r['perm_call'], r['vacant_call'], here, r['active_before'])
                before = B.auto_stats()['auto_passes'] if mode == 'auto' else 0
                B.run_steps(1, nbr)
                B.synchronize()
                if r['vacant'].any():
                    assert B.pass_forms() & S.FORM_VACANCY, here + ('the form word says vacancy',)
                    assert mode != 'auto' or B.auto_stats()['auto_passes'] == before, here + ('an AUTO pass while a row is vacant',)
                check_step(B, r, scene, here)
        finally:
            closed(A, B)
    assert held >= 5, held


# ---- twins ---------------------------------------------------------------------------------------------------------------------------------------
def look(sol, f):
    out = state_view(sol, f)
    out['vacant'] = sol.vacant()
    out['population'] = np.array([sol.population()])
    out['blob'] = sol.save_context(vacancy=True)
    return out


def run_ops(S, A, B, f, ops, at, nbr=None):
    """ops: ('step', k) | ('retire', ids) | ('call', fn(sol)) on both contexts, compared behind each"""
    nbr = S.NBR_KDTREE if nbr is None else nbr
    for i, (kind, arg) in enumerate(ops):
        here = at + (i, kind)
        if kind == 'step':
            for _ in range(arg):
                served = (A.get_state()['flags'] & 7) == 0
                A.run_steps(1, nbr)
                B.run_steps(1, nbr)
                same_views(look(A, f), look(B, f), here)
                same_pass(A, B, served, here)
                vac = (A.get_state()['flags'] & 8) != 0
                assert bool(A.pass_forms() & S.FORM_VACANCY) == bool(B.pass_forms() & S.FORM_VACANCY) == bool(vac.any()), here
                vacant_outputs(A, vac, here + ('A',))
                vacant_outputs(B, vac, here + ('B',))
            continue
        for sol in (A, B):
            if kind == 'retire':
                sol.retire(np.asarray(arg, np.int32))
            else:
                arg(sol)
        same_views(look(A, f), look(B, f), here)


def vtwin(S, make, prologue, ops, at, used=None, nbr=None, at_save=None):
    """A = make(0) runs `prologue` (steps, retires, admissions) and is saved; B = make(37) -- made to differ by used(B), if given -- loads
    the blob; then both take `ops`.  Returns nothing; at_save(A, info, blob) looks at what the blob holds."""
    A = B = None
    try:
        A = make(0)
        for kind, arg in prologue:
            if kind == 'step':
                A.run_steps(arg, S.NBR_KDTREE if nbr is None else nbr)
            elif kind == 'retire':
                A.retire(np.asarray(arg, np.int32))
            else:
                arg(A)
        blob = A.save_context(vacancy=True)
        info = S.context_checkpoint_info(blob)
        f = features(info)
        vac = (A.get_state()['flags'] & 8) != 0
        assert info['occupied'] == A.population() == A.n - int(vac.sum()) and len(blob) == A.context_checkpoint_bytes(vacancy=True), at + (info,)
        if at_save is not None:
            at_save(A, info, blob)
        B = make(EXTRA)
        if used is not None:
            used(B)
        B.load_context(blob, vacancy=True)
        same_views(look(A, f), look(B, f), at + ('behind the load',))
        vacant_outputs(B, vac, at + ('behind the load',))
        assert B.active_count() == int((B.get_state()['flags'] == 0).sum()), at + ('active_count behind the load',)
        run_ops(S, A, B, f, ops, at, nbr)
    finally:
        closed(A, B)


def fuzz_twin(S, scene, out, more, back, at, **kw):
    """two steps, `out` retired, a step, saved; then a step, `more` retired, a step, `back` admitted with new missions, two steps"""
    ops = [('step', 1)]
    if len(more):
        ops += [('retire', more), ('step', 1)]
    if len(back):
        m = mission_for(scene, np.sort(np.asarray(back, np.int32)), 4000 + scene['n'])
        ops += [('call', lambda sol: respawn(sol, m)), ('step', 2)]
    vtwin(S, lambda extra: fuzz_context(S, scene, extra), [('step', 2), ('retire', out), ('step', 1)], ops, at, **kw)


@pytest.mark.parametrize('n', [2, 63, 64, 65, 257, 2049])
def test_twins_through_the_sizes(S, row_env, n):
    """n = 2 with one row vacant; a wavefront less one, whole, and one more; 257 with vacant rows on both sides of position 256 of the
    permutation and of the id range (the compaction's tile); 2049.  Later retires and admissions on both"""
    row_env(None)
    scene = sized_scene(n)
    if n == 2:
        fuzz_twin(S, scene, [1], [], [1], ('n', n))
        return
    rng = np.random.default_rng(n)
    order = rng.permutation(n - 2)                                         # (ids 255 and 256 of 257 rows: n - 2 and n - 1 are retired by name)
    third = n // 3
    out = np.sort(np.concatenate([order[:third], [n - 2, n - 1]]))
    fuzz_twin(S, scene, out, np.sort(order[third:third + 5]), np.concatenate([out[::2], order[third:third + 2]]), ('n', n))
    if n == 257:                                                           # one occupied row left of 257: the tail straddles position 256 whatever the order
        fuzz_twin(S, scene, np.delete(np.arange(n), 100), [], np.arange(0, n, 2)[:60], ('n', n, 'm', 1))


# ---- loading into other contexts -------------------------------------------------------------------------------------------------------------------
def test_loading_into_contexts_that_are_not_fresh(S, row_env):
    """B has run, holds other vacant rows than the blob (some the same), or holds none; then a blob WITHOUT vacant rows goes into a context
    that has some: every row is occupied again and what vacancy refused works again"""
    row_env(None)
    scene = sized_scene(257)
    n = 257
    out = np.array([3, 100, 255, 256], np.int32)

    def other_rows(B):
        B.run_steps(3, S.NBR_KDTREE)
        B.retire(np.array([3, 7, 8, 200, 256], np.int32))
        B.run_steps(1, S.NBR_KDTREE)

    def no_rows(B):
        B.run_steps(4, S.NBR_KDTREE)
    for name, used in (('other rows', other_rows), ('none', no_rows)):
        fuzz_twin(S, scene, out, [5, 6], [3, 255, 5], ('into', name), used=used)
    A = B = None
    try:
        A = fuzz_context(S, scene)
        A.run_steps(3, S.NBR_KDTREE)
        blob = A.save_context(vacancy=True)
        assert blob.tobytes() == A.save_context().tobytes() and S.context_checkpoint_info(blob)['occupied'] == n       # byte for byte the old call's blob
        B = fuzz_context(S, scene, EXTRA)
        other_rows(B)
        refused(S, lambda: B.load_context(blob), ERR_UNSUPPORTED, 'vacant')                                            # options = 0: the old refusal
        refused(S, B.save_context, ERR_UNSUPPORTED, 'vacant')
        refused(S, B.context_checkpoint_bytes, ERR_UNSUPPORTED, 'vacant')
        B.load_context(blob, vacancy=True)
        assert B.population() == n and len(B.vacant()) == 0 and B.save_context().tobytes() == blob.tobytes() and B.context_checkpoint_bytes() == len(blob)
        f = features(S.context_checkpoint_info(blob))
        same_views(look(A, f), look(B, f), ('a blob without vacant rows',))
        probe = fuzz_context(S, scene)                                  # does the grid take this scene at all?
        try:
            probe.run_steps(3, S.NBR_KDTREE)
            probe.run_steps(1, S.NBR_GRID)
            grid = True
        except S.ScaError as e:
            assert 'SCA_NBR_GRID needs' in str(e), str(e)
            grid = False
        finally:
            probe.close()
        if grid:                                                          # ... then it takes B again, which refused it while a row was vacant
            A.run_steps(1, S.NBR_GRID)
            B.run_steps(1, S.NBR_GRID)
        run_ops(S, A, B, f, [('step', 1), ('retire', [9]), ('step', 1)], ('a blob without vacant rows',))
        # ... and the old load takes a blob the option wrote where no row was vacant
        C_ = fuzz_context(S, scene, 5)
        try:
            C_.load_context(blob)
            assert C_.save_context().tobytes() == blob.tobytes()
        finally:
            C_.close()
    finally:
        closed(A, B)


# ---- each feature with vacant rows in the blob -----------------------------------------------------------------------------------------------------
def traffic_mission(sc, ids, seed):
    """new missions for the rows `ids` of a traffic scene: their starts pushed 0.4 m outward, a goal across the circle, a goal heading"""
    ids = np.asarray(ids, np.int32)
    k = len(ids)
    rng = np.random.default_rng(seed)
    pos = sc['start'][ids] * [1.05, 1.05, 1.0] + np.round(rng.uniform(-0.1, 0.1, (k, 3)), 3)
    return dict(ids=ids, pos=pos, vel=np.zeros((k, 3), np.float32), heading=sc['heading'][ids], radius=sc['radius'][ids], pref_speed=np.full(k, 0.9),
                goal=-pos + [0.0, 0.0, 20.0], max_run_dist=np.full(k, 60.0), goal_heading=sc['gh'][ids])


def traffic_respawn(m, **kw):
    def call(sol):
        sol.respawn(m['ids'], m['pos'], m['vel'], m['heading'], m['radius'], m['pref_speed'], m['goal'], m['max_run_dist'], goal_heading=m['goal_heading'], **kw)
    return call


@pytest.mark.parametrize('n', [33, 64])
def test_the_device_tracker_with_vacant_tracked_rows(S, row_env, n):
    """tracked rows (policies 0 and 5) are retired in flight; the blob carries their tracker records; one is admitted behind the load and
    plans anew, the plans and re-plan counts of every row word for word for six steps"""
    row_env(None)
    sc = traffic_scene(n, True)
    tracked = np.flatnonzero(np.isin(sc['policy'], (0, 5)))
    out = np.sort(np.concatenate([tracked[:4], [2, 11]])).astype(np.int32)

    def at_save(A, info, blob):
        assert info['has_tracker'] == 1 and A.device_tracker_replans().sum() > 0
    back = traffic_mission(sc, [tracked[0], tracked[2], 11], n)
    vtwin(S, lambda extra: traffic_context(S, sc, extra), [('step', 4), ('retire', out), ('step', 2)],
          [('step', 1), ('call', traffic_respawn(back)), ('step', 3), ('retire', [tracked[5]]), ('step', 2)], ('tracker', n), at_save=at_save)


def test_slot_form_lists_with_vacant_rows(S, row_env):
    """rows in the middle of their lists are retired (len = rem = 0 in the blob, the rooms as they stand); an admission behind the load
    brings lists of its own"""
    row_env(None)
    seed = 19
    scene = F.random_scene(seed)
    initial = PR.initial_paths(seed, scene)
    with_list = np.flatnonzero(np.array([len(p) for p in initial]) > 0)
    out = np.unique(np.concatenate([with_list[:6], [1, 2]])).astype(np.int32)
    back = np.sort(out[::2])
    m = mission_for(scene, back, 77)
    lists = [[[float(x) for x in np.round(m['pos'][j] + [1.0 + q, 0.5, 0.0], 3)] for q in range(j % (W + 1))] for j in range(len(back))]

    def at_save(A, info, blob):
        ln, rooms = A.path_slot_lists()
        assert info['list_form'] == 2 and not ln[out].any() and ln.any()
    vtwin(S, lambda extra: fuzz_context(S, scene, extra, slots=(W, initial)), [('step', 2), ('retire', out), ('step', 2)],
          [('step', 1), ('call', lambda sol: respawn(sol, m, zaxis=np.zeros(len(back), np.uint8), paths=lists)), ('step', 3)], ('slot lists',), at_save=at_save)


@pytest.mark.parametrize('gate', [None, (0.5, 0)])
def test_tables_with_and_without_the_gate(S, row_env, gate):
    """mission tables while rows are vacant: a vacant row takes nothing; with the gate a row is retired WHILE a mission waits for it (its
    waiting word is dropped), and mission takes and gate verdicts go on alike behind the load"""
    row_env(None)
    sc = traffic_scene(48, False)
    probe = traffic_context(S, sc, missions=(3, 2, None), gate=gate)
    try:
        probe.run_steps(6, S.NBR_KDTREE)
        waiting = np.flatnonzero(probe.mission_gate_state()[0] >= 0) if gate else np.zeros(0, np.int64)
        finished = probe.finished()['id']
    finally:
        probe.close()
    assert gate is None or len(waiting) > 0
    out = np.unique(np.concatenate([waiting[:2], finished[:2], [0, 4, 9]])).astype(np.int32)

    def at_save(A, info, blob):
        assert info['M'] == 3 and info['has_gate'] == (1 if gate else 0) and A.mission_totals()['taken'] > 0
        if gate:
            assert (A.mission_gate_state()[0][out] == -1).all()
    back = traffic_mission(sc, out[:3], 48)
    back.pop('goal_heading')
    vtwin(S, lambda extra: traffic_context(S, sc, extra, missions=(3, 2, None), gate=gate), [('step', 6), ('retire', out), ('step', 2)],
          [('step', 2), ('call', lambda sol: sol.respawn(back['ids'], back['pos'], back['vel'], back['heading'], back['radius'], back['pref_speed'], back['goal'], back['max_run_dist'])),
           ('step', 4)], ('tables', gate), at_save=at_save)


def test_closest_approach_records_with_vacant_rows(S, row_env):
    row_env(None)
    scene = F.random_scene(19)
    out = np.arange(3, scene['n'], 7, dtype=np.int32)

    def at_save(A, info, blob):
        assert info['has_clearance'] == 1 and (A.clearance()['agent_step'] > 0).any()
    fuzz = lambda extra: fuzz_context(S, scene, extra, clearance=True)
    m = mission_for(scene, out[::2], 5)
    vtwin(S, fuzz, [('step', 3), ('retire', out), ('step', 2)], [('step', 1), ('call', lambda sol: respawn(sol, m)), ('step', 3)], ('clearance',), at_save=at_save)


def test_per_agent_attributes_and_an_attrs_admission(S, row_env):
    """A admits a vacant row with a policy and attributes of its own before the save: B's definition carries the policies as they stand at
    the save (a vacant row keeps its policy); behind the load both admit another row with attributes of its own"""
    row_env(None)
    seed = 1001
    scene = F.random_scene(seed)
    per = F.per_agent_attributes(seed, scene['n'])
    n = scene['n']
    out = np.arange(1, n, 5, dtype=np.int32)
    first, second = out[:2], out[2:4]
    m1, m2 = mission_for(scene, first, 11), mission_for(scene, second, 12)
    pol1, pol2 = np.array([3, 1], np.uint8), np.array([2, 4], np.uint8)
    attrs1, attrs2 = dict(neighbor_dist=[6.5, 9.0], max_neighbors=[5, 12]), dict(neighbor_dist=[4.0, 7.5], max_speed=[1.5, 0.8])

    def make(extra):
        B = fuzz_context(S, scene, extra, per_agent=per)
        if extra:                                                        # the definition holds the policies and attributes as they stand at the save: the admitted rows' own
            respawn(B, mission_for(scene, first, 11), policy=pol1, attrs=attrs1)
        return B
    vtwin(S, make, [('step', 2), ('retire', out), ('step', 1), ('call', lambda sol: respawn(sol, m1, policy=pol1, attrs=attrs1)), ('step', 2)],
          [('step', 1), ('call', lambda sol: respawn(sol, m2, policy=pol2, attrs=attrs2)), ('step', 3)], ('attrs',))


# ---- a file written in a child process -------------------------------------------------------------------------------------------------------------
CHILD = r'''
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import numpy as np
import form_fuzz as F
import sca_amd.solver as S
from sca_amd.checkpoint import ContextCheckpoint
s = scene = F.random_scene(19)
d = ContextCheckpoint.define(radius=s['radius'], pref_speed=s['pref_speed'], goal=s['goal'], policy=s['policy'], zaxis=F.zaxis_of(s), max_run_dist=s['max_run_dist'],
                             obstacles=(s['obs_pos'], s['obs_radius']), state=dict(pos=s['pos'], vel=s['vel'], heading=s['heading'], flags=s['flags']),
                             vpref=(s['vpref'], s['vmode']), clearance=True, neighbor_mode=0)
sol = ContextCheckpoint(d, None, 0).solver()
sol.run_steps(3, S.NBR_KDTREE)
sol.retire(np.arange(2, scene['n'], 3, dtype=np.int32))
sol.run_steps(3, S.NBR_KDTREE)
ContextCheckpoint(d, sol.save_context(vacancy=True), 6).write(sys.argv[1])
sol.close()
'''


def test_written_in_a_child_process_resumed_in_this_one(S, row_env, tmp_path):
    """the child (a fresh process) runs six steps with a third of its rows retired behind step 3, writes the .npz and exits; this process
    reads it, resumes through ContextCheckpoint.solver(), and goes on beside its own uncut run"""
    from sca_amd.checkpoint import ContextCheckpoint
    row_env(None)
    path = str(tmp_path / 'run.npz')
    run = subprocess.run([sys.executable, '-c', CHILD % dict(root=ROOT, tests=os.path.join(ROOT, 'tests')), path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    ck = ContextCheckpoint.read(path)
    scene = F.random_scene(19)
    out = np.arange(2, scene['n'], 3, dtype=np.int32)
    A = B = None
    try:
        A = fuzz_context(S, scene, clearance=True)
        A.run_steps(3, S.NBR_KDTREE)
        A.retire(out)
        A.run_steps(3, S.NBR_KDTREE)
        B = ck.solver(max_agents=scene['n'] + 11)
        info = S.context_checkpoint_info(ck.blob)
        assert ck.steps == 6 and info['occupied'] == scene['n'] - len(out) == B.population()
        assert B.save_context(vacancy=True).tobytes() == ck.blob.tobytes() == A.save_context(vacancy=True).tobytes()
        m = mission_for(scene, out[:5], 3)
        run_ops(S, A, B, features(info), [('step', 2), ('call', lambda sol: respawn(sol, m)), ('step', 2)], ('child',))
    finally:
        closed(A, B)


# ---- the Python layers ---------------------------------------------------------------------------------------------------------------------------
def ring(n=16, fleet=False):
    """the 16-drone circle without obstacles: (env, first) -- first[i] = (start, goal) of drone i's original mission"""
    from sca_amd import env as E, scenarios
    sc = scenarios.circle(n, rad=10.0)
    agents = [E.Agent(start_pos=list(sc['start'][i]), goal_pos=list(sc['goal'][i]), vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=E.ORCA3DPolicy, id=i) for i in range(n)]
    env = E.MACAEnv(clearance=True, attribute_slots=fleet)
    env.set_agents(agents, obstacles=[])
    return env, {a.id: (list(a.initial_pos), list(a.goal_pos)) for a in agents}


def traffic_rule(first, rng, env_of, fleet=False):
    """examples/run_sca.py --traffic as objects: an arrived drone leaves, a failed one starts over; seeded arrivals at vacant rows"""
    from sca_amd import env as E
    from sca_amd.lifelong import RETIRE
    kinds = [E.ORCA3DPolicy, E.RVO3DPolicy]

    def next_mission(agent, row):
        f = int(row['flags'])
        if f & 1 and not f & 2:
            return RETIRE
        start, goal = first[agent.id]
        return E.Agent(start_pos=start, goal_pos=goal, vel=[0.0, 0.0, 0.0], radius=agent.radius, pref_speed=agent.pref_speed, policy=type(agent.policy), id=agent.id)

    def arrivals(step, vacant_ids):
        k = min(len(vacant_ids), int(rng.poisson(0.3)))
        out = []
        for i in sorted(int(x) for x in rng.permutation(vacant_ids)[:k]):
            start, goal = first[i]
            kind = kinds[int(rng.integers(2))] if fleet else E.ORCA3DPolicy
            a = E.Agent(start_pos=start, goal_pos=goal, vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=kind, id=i)
            if fleet:
                a.neighborDist = 6.0 + (step % 3)
            out.append(a)
        return out
    return next_mission, arrivals


@pytest.mark.parametrize('margin,fleet', [(None, False), (0.5, False), (0.5, True)])
def test_run_lifelong_cut_at_half_and_resumed(S, row_env, tmp_path, margin, fleet):
    """the 16-drone ring with RETIRE, seeded arrivals and a spawn margin: the run cut behind step 200 of 400 and resumed in a fresh env
    returns the stats of the run that was never cut, equal on every key; the resumed env's mirrors show the checkpoint at once"""
    import json
    from sca_amd import env as E
    from sca_amd.checkpoint import ContextCheckpoint
    from sca_amd.lifelong import resume_user_state, run_lifelong
    row_env(None)
    envs = []
    try:
        env, first = ring(fleet=fleet)
        envs.append(env)
        rng = np.random.default_rng(7)
        nm, arr = traffic_rule(first, rng, env, fleet)
        whole = run_lifelong(env, nm, 400, spawn_margin=margin, arrivals=arr)
        assert whole['steps'] == 400 and whole['retired_rows'] > 0 and whole['admitted'] > 0, whole
        cut_env, first = ring(fleet=fleet)
        envs.append(cut_env)
        rng = np.random.default_rng(7)
        nm, arr = traffic_rule(first, rng, cut_env, fleet)
        path = str(tmp_path / 'cut.npz')
        half = run_lifelong(cut_env, nm, 400, spawn_margin=margin, arrivals=arr, checkpoint_at=(200, path), user_state=lambda: json.dumps(rng.bit_generator.state))
        assert half['steps'] == 200 and half != whole
        with np.load(path, allow_pickle=False) as z:
            assert all(z[k].dtype != object for k in z.files)
        ck = ContextCheckpoint.read(path)
        info = S.context_checkpoint_info(ck.blob)
        assert ck.steps == 200 and info['occupied'] == cut_env.population
        resumed = E.MACAEnv.from_checkpoint(ck)
        envs.append(resumed)
        # the mirrors show the checkpoint at once
        assert resumed.population == cut_env.population and resumed.vacant.tolist() == cut_env.vacant.tolist()
        assert [a.is_vacant for a in resumed.agents] == [a.is_vacant for a in cut_env.agents] and resumed._active == cut_env._active
        assert [type(a.policy) for a in resumed.agents] == [type(a.policy) for a in cut_env.agents]
        assert [a.neighborDist for a in resumed.agents] == [a.neighborDist for a in cut_env.agents]
        assert resumed.per_agent_attributes == cut_env.per_agent_attributes
        for k in ('pos_global_frame', 'vel_global_frame', 'heading_global_frame', 'goal_global_frame'):
            assert all(np.array_equal(getattr(a, k), getattr(b, k)) for a, b in zip(resumed.agents, cut_env.agents)), k
        assert resumed.solver.save_context(vacancy=True).tobytes() == ck.blob.tobytes()
        rng2 = np.random.default_rng(0)
        rng2.bit_generator.state = json.loads(resume_user_state(ck))
        nm, arr = traffic_rule(first, rng2, resumed, fleet)
        rest = run_lifelong(resumed, nm, 200, spawn_margin=margin, arrivals=arr, resume=ck)
        assert rest == whole, (rest, whole)
        assert np.array_equal(resumed.pos, env.pos) and np.array_equal(resumed.flags, env.flags) and resumed.vacant.tolist() == env.vacant.tolist()
    finally:
        for e in envs:
            if e.solver is not None:
                e.solver.close()


@pytest.mark.parametrize('extra', [[], ['--spawn-margin', '0.5', '--fleet', 'orca,rvo']])
def test_the_example_saved_and_resumed_against_one_run(row_env, tmp_path, extra):
    """examples/run_sca.py --lifelong 300 --traffic 0.2: --save-at 150 and --resume against the run that was never cut -- the summary lines
    behind the timing line are the same"""
    row_env(None)
    common = [sys.executable, os.path.join(ROOT, 'examples', 'run_sca.py'), '--policy', 'orca', '--no-obstacles', '--lifelong', '300', '--traffic', '0.2'] + extra
    f = str(tmp_path / 'example.npz')

    def lines(more):
        run = subprocess.run(common + more, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
        out = run.stdout.strip().split('\n')
        at = next(i for i, x in enumerate(out) if x.startswith('lifelong:'))
        return out, out[at + 1:]
    _, whole = lines([])
    saved, cut = lines(['--save-at', '150', '--save-file', f])
    assert any(x.startswith('saved behind step 150') for x in saved) and os.path.exists(f) and cut != whole, saved
    _, resumed = lines(['--resume', f])
    assert resumed == whole and whole[0].startswith("{'arrived':") and any(x.startswith('traffic') for x in whole), (resumed, whole)


# ---- every refusal -------------------------------------------------------------------------------------------------------------------------------
def seal(b):
    """the header's checksum from the bytes as they stand: FNV-1a over the 64-bit words behind the header"""
    h = 0xcbf29ce484222325
    for w in np.frombuffer(b[128:].tobytes(), '<u8').tolist():
        h = ((h ^ w) * 0x100000001b3) & 0xffffffffffffffff
    b[72:80] = np.frombuffer(np.array([h], '<u8').tobytes(), np.uint8)
    return b


def test_refusals(S, row_env):
    """options = 0 while a row is vacant, an unknown option bit, and each new fault through the C call -- decided before any device work:
    the context's own save is byte-equal around every refused load"""
    import ctypes as C
    row_env(None)
    sc = traffic_scene(33, True)
    lists, initial = lists_for(sc)
    full = dict(clearance=True, slots=(W, initial), missions=(3, 2, lists), gate=(0.5, 0))
    A = B = D = None
    try:
        A = traffic_context(S, sc, **full)
        A.run_steps(4, S.NBR_KDTREE)
        out = np.array([1, 8, 20, 32], np.int32)
        A.retire(out)
        A.run_steps(1, S.NBR_KDTREE)
        n, m = 33, 29
        # options = 0 is the old call, under either name; an unknown bit is an argument error
        size = C.c_int64(0)
        buf = np.zeros(A.context_checkpoint_bytes(vacancy=True), np.uint8)
        ptr = C.c_void_p(buf.ctypes.data)
        for call in (lambda: A.L.sca_save_context_opt(A.ctx, 0, ptr, buf.size), lambda: A.L.sca_load_context_opt(A.ctx, 0, ptr, buf.size),
                     lambda: A.L.sca_context_checkpoint_bytes_opt(A.ctx, 0, C.byref(size)), lambda: A.L.sca_save_context(A.ctx, ptr, buf.size)):
            assert call() == ERR_UNSUPPORTED and 'vacant' in A.L.sca_last_error(A.ctx).decode()
        for bits in (2, 3, 0x80000000):
            assert A.L.sca_save_context_opt(A.ctx, bits, ptr, buf.size) == ERR_ARG and A.L.sca_load_context_opt(A.ctx, bits, ptr, buf.size) == ERR_ARG
            assert A.L.sca_context_checkpoint_bytes_opt(A.ctx, bits, C.byref(size)) == ERR_ARG and 'option' in A.L.sca_last_error(A.ctx).decode()
        assert A.L.sca_save_context_opt(A.ctx, 1, None, buf.size) == ERR_ARG and A.L.sca_save_context_opt(A.ctx, 1, ptr, buf.size - 1) == ERR_ARG
        blob = A.save_context(vacancy=True)
        info = S.context_checkpoint_info(blob)
        off = info['offsets']
        assert info['occupied'] == m and blob[24] == 63
        with pytest.raises(S.ScaError):                                    # (the check without a context refuses what the load refuses)
            S.context_checkpoint_info(seal(np.concatenate([blob[:52], [0, 0, 0, 0], blob[56:]]).astype(np.uint8)))
        B = traffic_context(S, sc, EXTRA, **full)
        B.run_steps(2, S.NBR_KDTREE)
        B.retire(np.array([5], np.int32))

        def bad(edits):
            b = blob.copy()
            for at, v in edits:
                b[at] = v
            return seal(b)

        def unchanged(load, *words):
            before = B.save_context(vacancy=True)
            refused(S, load, ERR_ARG, *words)
            assert B.save_context(vacancy=True).tobytes() == before.tobytes() and B.vacant().tolist() == [5] and B.population() == n - 1, words
        word = lambda at, v: [(at + k, (v >> (8 * k)) & 255) for k in range(4)]
        perm = np.frombuffer(blob[off[12]:off[12] + 4 * n].tobytes(), np.int32)
        assert perm[m:].tolist() == out.tolist()
        load = lambda b: (lambda: B.load_context(b, vacancy=True))
        unchanged(load(bad(word(52, 0))), 'header')
        unchanged(load(bad(word(52, n))), 'header')
        unchanged(load(bad([(24, 127)])), 'header')
        unchanged(load(bad([(off[1] + 48 * 8 + 36, 9)])), 'row 8', 'flag word other than 11')
        unchanged(load(bad(word(52, m - 1))), 'n - occupied')
        unchanged(load(bad(word(off[12], int(perm[m])) + word(off[12] + 4 * m, int(perm[0])))), 'position 0')
        unchanged(load(bad(word(off[12] + 4 * m, 8) + word(off[12] + 4 * (m + 1), 1))), 'position %d' % m)
        unchanged(load(bad([(off[1] + 48 * 20 + 27, 0x3f)])), 'vacant row 20')
        unchanged(load(bad([(off[2] + 24 * 20 + 7, 0x3f)])), 'vacant row 20')
        unchanged(load(bad([(off[9] + 8 * 32 + 7, 0x3f)])), 'vacant row 32')
        unchanged(load(bad([(off[18] + 4 * 1, 1)])), 'vacant row 1')
        unchanged(load(bad(word(off[23] + 4 * 8, 0))), 'vacant row 8')
        # without the option the same blob is refused for its header, and a loadable blob is still taken
        before = B.save_context(vacancy=True)
        refused(S, lambda: B.load_context(blob), ERR_UNSUPPORTED, 'vacant')
        assert B.save_context(vacancy=True).tobytes() == before.tobytes()
        B.load_context(blob, vacancy=True)
        assert B.save_context(vacancy=True).tobytes() == blob.tobytes() and B.vacant().tolist() == out.tolist()
        # vacancy with lists in block form, which no save can write: a block-form blob edited by hand
        scene = F.random_scene(19)
        D = fuzz_context(S, scene, paths=F.random_paths(19, scene))
        D.run_steps(2, S.NBR_KDTREE)
        bb = D.save_context(vacancy=True)
        io = S.context_checkpoint_info(bb)['offsets']
        nn = scene['n']
        p = np.frombuffer(bb[io[12]:io[12] + 4 * nn].tobytes(), np.int32)
        row = nn - 1                                                         # the last id vacant: moved to the permutation's end
        q = np.concatenate([p[p != row], [row]]).astype('<i4')
        bb = bb.copy()
        bb[io[12]:io[12] + 4 * nn] = np.frombuffer(q.tobytes(), np.uint8)
        bb[io[1] + 48 * row + 24:io[1] + 48 * row + 36] = 0
        bb[io[1] + 48 * row + 36:io[1] + 48 * row + 40] = [11, 0, 0, 0]
        bb[io[2] + 24 * row:io[2] + 24 * row + 24] = 0
        bb[io[9] + 8 * row:io[9] + 8 * row + 8] = 0
        bb[24] |= 32
        bb[52:56] = np.frombuffer(np.array([nn - 1], '<i4').tobytes(), np.uint8)
        before = D.save_context()
        refused(S, lambda: D.load_context(seal(bb), vacancy=True), ERR_ARG, 'block form')
        assert D.save_context().tobytes() == before.tobytes()
    finally:
        closed(A, B, D)
