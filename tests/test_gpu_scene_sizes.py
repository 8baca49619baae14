"""Slots of a capacity (-m gpu): sca_restart_scenes_sized puts an episode of ANY agent count 1 .. capacity into a slot of a scene batch; the
rows of the slot's range behind the episode are vacant.  The bar is equality, no tolerance: a slot that holds an n-agent episode is held
against a fresh context of that episode alone (every value of the contract: state, action rows, neighbour lists and distSq, diagnostics,
the scene-local permutation, tracker records and re-plan counts, the log per scene) and, where the reference recorded the episode, against
its records; the vacant rows are held against what include/sca_hip.h says they read."""
import numpy as np
import pytest

from scene_util import (NO_OBSTACLES, SizedSlots, alone, assert_slots_equal_alone, assert_vacant, circle_scene, context, everything, load_any, observe,
                        padded, partial_batch, rc_of, restart_all, step_all)

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -5                                   # include/sca_hip.h
ORCA, SCA = 3, 0                                                    # SCA_POLICY_ORCA3D, SCA_POLICY_SCA
MIX = np.array([0, 1, 2, 3, 4, 5], np.uint8)


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


def _mix(n, shift=0):
    return np.roll(np.resize(MIX, n), shift)


def test_recorded_episodes_into_larger_slots(S):
    """three recorded 100-agent episodes, 10 steps; then slot 1 <- the 60-agent packed ORCA episode (its 14 spheres are slot 1's own set)
    and slot 2 <- the 8-agent SCA circle (tracked, a root-leaf tree), 25 steps; then slot 2 grows back to a 100-agent S-RVO circle, 15
    steps.  Restarted slots against the records of their new episode from record 0 and against a fresh context of it alone, slot 0
    against its own records straight through; sizes, active, steps and sca_active_count right behind each call."""
    packed = load_any('F5_orca_packed60')
    sets = [NO_OBSTACLES, (packed['obs_pos'].reshape(-1, 3), packed['obs_radius']), NO_OBSTACLES]
    b = SizedSlots(S, ['F2_orca_circle100', 'F2_sca_circle100', 'F3_rvo_random100'], obstacles=sets)
    assert b.sol.scene_sizes().tolist() == [100, 100, 100]
    compared = b.run_and_check(10, label='full slots')
    assert compared.tolist() == [10, 10, 10]
    live = b.sol.scene_state()['active']
    assert b.sol.active_count() == int(live.sum()) and live[1] > 60 and live[2] > 8
    b.restart({1: 'F5_orca_packed60', 2: 'F1_sca_circle8'})
    assert b.sol.scene_sizes().tolist() == [100, 60, 8]
    assert b.sol.active_count() == int(live[0]) + 60 + 8            # rows that were running and are vacant now no longer count
    sc = b.sol.scene_state()
    assert sc['active'].tolist() == [int(live[0]), 60, 8] and sc['steps'].tolist() == [10, 0, 0]
    solos = {s: alone(S, b.names[s]) for s in (1, 2)}
    obs_lo = {1: 0, 2: 14}

    def beside(t):
        step_all(S, *(x for x, _ in solos.values()))
        got = assert_slots_equal_alone(b.sol, b.off, {s: e for s, (_, e) in solos.items()}, {s: x for s, (x, _) in solos.items()},
                                       ('beside', 'batch step', t), obs_lo=obs_lo)
        assert_vacant(got, b.off, b.size, ('batch step', t))
    compared = b.run_and_check(25, after_step=beside, label='60 and 8 agents in slots of 100')
    assert compared.tolist() == [25, 1, 25]                         # (the packed episode has one record, the circle 246)
    assert b.sol.scene_state()['steps'].tolist() == [35, 25, 25]
    for x, _ in solos.values():
        x.close()
    # grow: slot 2 back to 100 agents while slot 1 stays at 60
    b.restart({2: 'F2_srvo_circle100'})
    assert b.sol.scene_sizes().tolist() == [100, 60, 100]
    sc = b.sol.scene_state()
    assert sc['active'][2] == 100 and sc['steps'].tolist() == [35, 25, 0]
    assert b.sol.active_count() == int(sc['active'].sum())
    solos = {2: alone(S, 'F2_srvo_circle100')}
    compared = b.run_and_check(15, after_step=beside, label='grown back to 100')
    assert compared.tolist() == [5, 0, 15]                          # (slot 0's 40 records end at batch step 40)
    b.sol.close()
    solos[2][0].close()


SIZES = (1, 10, 11, 63, 64, 65, 127, 129, 130)


def test_boundary_sizes(S):
    """nine slots of capacity 130 holding 1 .. 130 agents by ONE sized restart: a single agent, the root-leaf limit (10, 11), a wavefront
    edge (63, 64, 65), vacancies that begin inside K4's group of 8 and the log kernel's 16 agents, capacity - 1 and the capacity; ORCA and
    SCA circles in turn.  12 steps, every slot against a context of its scene alone."""
    eps = [circle_scene(S, n, ORCA if k % 2 else SCA, rad=max(2.0, 0.2 * n), turn=k) for k, n in enumerate(SIZES)]
    sol, off = partial_batch(S, eps, 130)
    assert sol.scene_sizes().tolist() == list(SIZES) and sol.scene_state()['active'].tolist() == list(SIZES)
    solos = {s: context(S, [e])[0] for s, e in enumerate(eps)}
    held = dict(enumerate(eps))
    for t in range(12):
        step_all(S, sol, *solos.values())
        got = assert_slots_equal_alone(sol, off, held, solos, ('boundary sizes', 'step', t))
        assert_vacant(got, off, SIZES, ('boundary sizes', 'step', t))
        assert sol.active_count() == sum(x.active_count() for x in solos.values())
    assert sol.scene_state()['steps'].tolist() == [12] * len(SIZES)
    for x in [sol] + list(solos.values()):
        x.close()


def test_vacant_rows_are_inert_and_invisible(S):
    """a 100-agent circle runs to its natural finish -- every agent on the circle again -- and the slot takes a 50-agent circle of the same
    radius: live agents start on top of the vacant rows' old positions.  30 steps equal to the 50-agent context alone; no list holds a
    vacant id; the vacant rows stay bit for bit what the restart left."""
    rad = 20.0
    big, small = circle_scene(S, 100, ORCA, rad=rad), circle_scene(S, 50, ORCA, rad=rad)
    other = circle_scene(S, 12, _mix(12))
    sol, off = context(S, [other, big])
    lo, hi = int(off[1]), int(off[2])
    for _ in range(40):                                             # 100 steps at a time until the scene is done (40 m at 0.1 m a step, and the detours)
        step_all(S, sol, k=100)
        if sol.scene_state()['active'][1] == 0:
            break
    st = sol.get_state()
    assert sol.scene_state()['active'][1] == 0 and (st['flags'][lo:hi] & 7).all()
    arrived = st['pos'][lo + 50:hi][(st['flags'][lo + 50:hi] & 1) == 1]        # rows that will be vacant, at their goals on the circle
    on_top = (np.linalg.norm(small['pos'][:, None] - arrived[None], axis=2) < 1.0).any(axis=1).sum()
    assert on_top >= 10, on_top                                    # new agents start within touching distance (2 radii) of them
    restart_all(sol, [1], [small], sizes='own')
    left = everything(sol)
    vac = slice(lo + 50, hi)
    assert np.array_equal(left['pos'][vac], st['pos'][vac])         # a vacant row keeps the position of whoever stood there
    solo = context(S, [small])[0]
    for t in range(30):
        step_all(S, sol, solo)
        got = assert_slots_equal_alone(sol, off, {1: small}, {1: solo}, ('on top of vacant rows', 'step', t))
        assert_vacant(got, off, [12, 50], ('step', t))
        for key in ('nbr_id',):
            ids = got[key][lo:lo + 50]
            assert (ids < lo + 50).all(), ('a list holds a vacant id', t)
        assert np.array_equal(np.sort(got['perm'][lo:lo + 50]), np.arange(lo, lo + 50)) and np.array_equal(got['perm'][vac], np.arange(lo + 50, hi))
        for key in ('pos', 'heading', 'total_dist', 'step_num', 'flags', 'vel'):
            assert np.array_equal(got[key][vac], left[key][vac]), ('a vacant row moved', key, t)
        assert not got['action'][vac].any()
    for x in (sol, solo):
        x.close()


def test_every_step_form_behind_a_sized_restart(S):
    """sca_env_step, sca_run_steps(k) and policy pass + sca_env_update on one partial batch each: the same states, and the contexts alone'"""
    eps = [circle_scene(S, n, _mix(n, k), rad=3.0 + k, turn=k) for k, n in enumerate((5, 12, 9))]
    forms = dict(env_step=lambda x: [x.env_step(S.NBR_KDTREE) for _ in range(6)],
                 run_steps=lambda x: (x.run_steps(6, S.NBR_KDTREE), x.synchronize()),
                 split=lambda x: [(x.policy_pass(S.NBR_KDTREE), x.env_update()) for _ in range(6)])
    solos = {s: context(S, [e])[0] for s, e in enumerate(eps)}
    step_all(S, *solos.values(), k=6)
    results = {}
    for name, form in forms.items():
        sol, off = partial_batch(S, eps, 12)
        form(sol)
        results[name] = assert_slots_equal_alone(sol, off, dict(enumerate(eps)), solos, ('step form', name))
        assert_vacant(results[name], off, [5, 12, 9], ('step form', name))
        assert sol.scene_state()['steps'].tolist() == [6, 6, 6]
        sol.close()
    for key in ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num', 'perm'):
        assert np.array_equal(results['env_step'][key], results['run_steps'][key]) and np.array_equal(results['env_step'][key], results['split'][key]), key
    for x in solos.values():
        x.close()


def test_the_log_per_scene(S):
    """the rows of a partially filled slot equal sca_get_history of the context alone; a slot shrunk by a restart starts at row 0; an
    agent window past the size is SCA_ERR_ARG; a neighbouring full slot's rows are unchanged by the call"""
    full, first, second = circle_scene(S, 12, _mix(12)), circle_scene(S, 9, _mix(9, 1), rad=3.0), circle_scene(S, 5, _mix(5, 2), rad=2.5, turn=1)
    sol, off = context(S, [full, padded(first, 12)])
    sol.scene_history_enable(16)
    restart_all(sol, [1], [first], sizes='own')
    solos = []
    for e in (full, first, second):
        x = context(S, [e])[0]
        x.history_enable(16)
        solos.append(x)
    step_all(S, sol, solos[0], solos[1], k=4)
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in ('pos', 'heading', 'vel'))
    assert sol.scene_history_rows()['logged'].tolist() == [4, 4]
    assert same(sol.scene_history(1), solos[1].history()) and sol.scene_history(1)['pos'].shape == (4, 9, 3)
    assert same(sol.scene_history(1, 1, 2, 3, 6), solos[1].history(1, 2, 3, 6))
    assert rc_of(S, lambda: sol.scene_history(1, 0, 4, 0, 10)) == ERR_ARG          # size + 1
    assert rc_of(S, lambda: sol.scene_history(1, 0, 4, 9, 1)) == ERR_ARG
    before = sol.scene_history(0)
    restart_all(sol, [1], [second], sizes='own')                  # shrink 9 -> 5 while the slot is running
    assert sol.scene_history_rows()['logged'].tolist() == [4, 0]
    assert same(sol.scene_history(0), before)
    step_all(S, sol, solos[0], solos[2], k=3)
    assert sol.scene_history_rows()['logged'].tolist() == [7, 3]
    assert same(sol.scene_history(1), solos[2].history()) and sol.scene_history(1)['pos'].shape == (3, 5, 3)
    assert same(sol.scene_history(0), solos[0].history())
    assert rc_of(S, lambda: sol.scene_history(1, 0, 3, 0, 6)) == ERR_ARG
    for x in [sol] + solos:
        x.close()


def test_per_scene_obstacle_sets(S):
    """slot 0: a 24-agent SCA circle whose own set is the take-off field's 8 spheres, slot 1: the same circle with none.  Slot 0 <- the
    recorded 16-agent take-off episode: its records and the context alone, 40 steps; slot 1 is unaffected"""
    takeoff = load_any('F4_sca_takeoff16')
    spheres = (takeoff['obs_pos'].reshape(-1, 3), takeoff['obs_radius'])
    circle = circle_scene(S, 24, SCA, rad=8.0)
    b = SizedSlots(S, [circle, circle], obstacles=[spheres, NO_OBSTACLES])
    other = context(S, [circle])[0]
    b.run_and_check(5, after_step=lambda t: step_all(S, other), label='two circles')
    b.restart({0: 'F4_sca_takeoff16'})
    assert b.sol.scene_sizes().tolist() == [16, 24]
    solo, ep = alone(S, 'F4_sca_takeoff16')

    def beside(t):
        step_all(S, solo, other)
        got = assert_slots_equal_alone(b.sol, b.off, {0: ep, 1: circle}, {0: solo, 1: other}, ('take-off field', 'batch step', t), obs_lo={0: 0, 1: 8})
        assert_vacant(got, b.off, [16, 24], ('batch step', t))
    compared = b.run_and_check(40, after_step=beside, label='take-off episode in a slot of 24')
    assert compared.tolist() == [40, 0]
    for x in (b.sol, solo, other):
        x.close()


def test_refusals_and_equivalence(S):
    first, new, small = circle_scene(S, 12, _mix(12)), circle_scene(S, 12, _mix(12, 3), turn=2), circle_scene(S, 7, _mix(7, 1), rad=3.0)
    sol, off = context(S, [first] * 3)
    twin, _ = context(S, [first] * 3)
    step_all(S, sol, twin, k=5)
    before = observe(sol)
    for size in (0, 13, -1):                                         # size 0, capacity + 1 (the arrays hold the capacity's 12 rows: the library decides)
        assert rc_of(S, lambda: restart_all(sol, [1], [new], sizes=[size])) == ERR_ARG, size
        after = observe(sol)
        for key in before:
            assert np.array_equal(before[key], after[key]), ('a refused call changed', key, size)
    # sizes == NULL is sca_restart_scenes
    restart_all(sol, [2, 0], [new, new])
    cat = lambda key: np.concatenate([new[key], new[key]])
    twin.restart_scenes([2, 0], cat('pos'), cat('heading'), vel=cat('vel'), radius=cat('radius'), pref_speed=cat('pref_speed'), goal=cat('goal'),
                        policy=cat('policy'), zaxis=cat('zaxis'), max_run_dist=cat('max_run_dist'), goal_heading=cat('goal_heading'))
    for k in range(2):
        a, b_ = everything(sol), everything(twin)
        for key in a:
            assert np.array_equal(a[key], b_[key], equal_nan=True), ('sizes == NULL against sca_restart_scenes', key, k)
        assert sol.scene_sizes().tolist() == [12, 12, 12] and sol.active_count() == twin.active_count()
        step_all(S, sol, twin, k=3)
    twin.close()
    # a partial slot: the entry points that take a whole-context state from outside are refused, and nothing changes
    st, perm = sol.get_state(), sol.get_kd_perm()
    sol.host_state()
    restart_all(sol, [1], [small], sizes='own')
    assert sol.scene_sizes().tolist() == [12, 7, 12]
    partial = observe(sol)
    assert rc_of(S, lambda: sol.set_state(st['pos'], st['vel'], st['heading'], st['flags'], st['total_dist'], st['step_num'])) == ERR_UNSUPPORTED
    assert rc_of(S, lambda: sol.set_kd_perm(perm)) == ERR_UNSUPPORTED
    assert rc_of(S, lambda: sol.step_host(S.NBR_KDTREE, state=False)) == ERR_UNSUPPORTED
    for key, v in observe(sol).items():
        assert np.array_equal(partial[key], v), key
    # every slot full again: they work
    restart_all(sol, [1], [new], sizes='own')                     # (sizes [12]: the capacity)
    assert sol.scene_sizes().tolist() == [12, 12, 12]
    st, perm = sol.get_state(), sol.get_kd_perm()
    sol.set_state(st['pos'], st['vel'], st['heading'], st['flags'], st['total_dist'], st['step_num'])
    sol.set_kd_perm(perm)
    assert sol.step_host(S.NBR_KDTREE, state=False) == sol.active_count()
    # ... and sca_restart_scenes itself fills a partial slot to its capacity
    restart_all(sol, [0], [small], sizes='own')
    sol.restart_scenes([0], new['pos'], new['heading'])
    assert sol.scene_sizes().tolist() == [12, 12, 12] and sol.scene_state()['active'][0] == 12
    sol.set_kd_perm(sol.get_kd_perm())
    # the sizes go with the scenes
    sol.set_scenes(off)
    assert sol.scene_sizes().tolist() == [12, 12, 12]
    sol.set_scenes(None)
    assert rc_of(S, sol.scene_sizes) == -3
    sol.close()


def _episodes(counts):
    from sca_amd import scenarios
    from sca_amd.env import Agent, ORCA3DPolicy, SCAPolicy
    out = []
    for k, n in enumerate(counts):
        sc = scenarios.circle(n, rad=3.0 + 0.5 * (k % 4))
        pol = (ORCA3DPolicy, SCAPolicy)[k % 2]
        out.append([Agent(start_pos=list(sc['start'][i]), goal_pos=list(sc['goal'][i]), vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=pol, id=i) for i in range(n)])
    return out


def test_streaming_a_mixed_queue(S):
    """twelve ORCA3D / SCA circle episodes of 6, 11 and 16 drones through three capacity slots: every episode's final state, steps, metrics
    and trajectories equal a SceneBatch of that episode alone; capacities=None still runs the queue as before; an episode that fits no
    slot is a ValueError before any step"""
    from sca_amd import metrics
    from sca_amd.scenes import SceneBatch, run_episodes
    counts = [6, 11, 16, 16, 6, 11, 11, 16, 6, 6, 11, 16]
    stats = {}
    results = run_episodes(_episodes(counts), 3, device_tracker=True, stats=stats, history_rows=1500, capacities='max')
    assert all(r is not None for r in results) and [len(r['state']['flags']) for r in results] == counts
    assert 0.0 < stats['live_fraction'] <= 1.0 and {r['slot'] for r in results} == {0, 1, 2}
    fixed = run_episodes(_episodes(counts), 3, device_tracker=True, history_rows=1500)        # capacities=None: a slot per count
    for i, (n, r, f, eps) in enumerate(zip(counts, results, fixed, _episodes(counts))):
        solo = SceneBatch([eps], device_tracker=True, scene_history=1500)
        while not solo.step():
            pass
        view = solo.env(0)
        assert r['steps'] == f['steps'] == int(solo.steps[0]), i
        want = {k: solo._state(k)[:n] for k in solo._mirror}
        for key, v in want.items():
            assert np.array_equal(r['state'][key], v), ('capacity slots', i, key)
            assert np.array_equal(f['state'][key], v), ('fixed slots', i, key)
        m = metrics.episode_metrics(view)
        for key, v in m.items():
            if key != 'AverageCost':                               # (wall time)
                assert np.array_equal(r['metrics'][key], v, equal_nan=True), ('metrics', i, key)
        rows, dropped = view.solver.history_rows()
        assert dropped == 0 and r['rows_dropped'] == 0
        assert np.array_equal(r['trajectories'], metrics.trajectories(view, rows=rows)), ('trajectories', i)
        solo.close()
    with pytest.raises(ValueError):
        run_episodes(_episodes([6, 20, 11]), 3, device_tracker=True, capacities=[16, 16, 16])
