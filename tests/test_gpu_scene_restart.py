"""sca_restart_scenes (-m gpu): a new episode into a slot of a scene batch while the other slots keep running.  The bar is equality, no
tolerance: a restarted slot is held against the reference's recorded episode of what it now holds, from that episode's record 0, and --
for the values the recordings do not hold -- against a fresh context holding that episode alone; every slot that was not named is held
against its own records straight through the call."""
import ctypes as C

import numpy as np
import pytest

from scene_util import (Slots, assert_scene_equals_alone, assert_slots_equal_alone, assert_vacant, circle_scene, context, everything, load_any, observe, rc_of,
                        restart_all)

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5                   # include/sca_hip.h

TWELVE = ['F2_%s_circle100' % p for p in ('orca', 'orcalp', 'rvo', 'rvodubins', 'sca', 'srvo')] + \
         ['F3_%s_random100' % p for p in ('orca', 'orcalp', 'rvo', 'srvo')] + ['F3_orcalp_sphere100', 'F3_srvo_sphere100']
# slot -> the episode it is given at batch step 10.  Slots 0, 1, 2 and 5 (F2 orca / orcalp / rvo / srvo, 40 records each) are left alone.
PLAN = {3: 'F3_orca_random100',        # RVO3D+Dubins (tracked)  -> ORCA (untracked)
        4: 'F2_orcalp_circle100',      # SCA (tracked)           -> ORCA3D-LP (untracked; joins the LP list)
        6: 'F2_sca_circle100',         # ORCA (untracked)        -> SCA (tracked)
        7: 'F2_rvodubins_circle100',   # ORCA3D-LP               -> RVO3D+Dubins (tracked; leaves the LP list)
        8: 'F3_orcalp_sphere100',      # RVO                     -> ORCA3D-LP (joins the LP list)
        9: 'F3_srvo_sphere100',        # S-RVO random            -> S-RVO sphere
        10: 'F3_rvo_random100',        # ORCA3D-LP               -> RVO (leaves the LP list)
        11: 'F2_srvo_circle100'}       # S-RVO sphere            -> S-RVO circle


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


def _beside(S, b, solos):
    """after_step hook: every slot of `solos` ({slot: a Slots of the same episode alone, stepped here}) against the batch, every value"""
    def hook(t):
        tracked = {s: np.flatnonzero(np.isin(x.fx[0]['policy'], (0, 5))) for s, x in solos.items()}
        lo_of = {s: int(b.off[s]) for s in solos}
        got = everything(b.sol, [lo_of[s] + a for s in solos for a in tracked[s]])
        for s, x in solos.items():
            x.sol.run_steps(1, S.NBR_KDTREE)
            x.sol.synchronize()
            alone = everything(x.sol, tracked[s])
            assert_scene_equals_alone(got, lo_of[s], int(b.off[s + 1]), 0, alone, ('beside', 'batch step', t, 'slot', s, x.names[0]))
    return hook


def test_live_restart_and_policy_change(S):
    """twelve recorded 100-agent episodes, the tracker in the pass; 10 steps; eight slots get another recorded episode (tracked <-> untracked,
    LP <-> non-LP among them) while four fly on; 25 more steps.  Restarted slots against records 0, 1, ... of their NEW episode, untouched
    slots against their own records 10 .. 34, before and after every step; steps[s] / active[s]; and two restarted slots (one now tracked, one
    now ORCA3D-LP) against a fresh context of that episode alone: neighbour lists and distSq, diagnostics, action rows, tracker records,
    re-plan counts."""
    b = Slots(S, TWELVE)
    assert b.n == 1200 and b.tracker
    compared = b.run_and_check(10, label='before the restart')
    assert compared.tolist() == [10] * 12
    b.restart(PLAN)
    sc = b.sol.scene_state()
    assert sc['steps'].tolist() == [0 if s in PLAN else 10 for s in range(12)] and sc['active'].tolist() == [100] * 12
    solos = {6: Slots(S, [PLAN[6]]), 8: Slots(S, [PLAN[8]])}
    compared = b.run_and_check(25, after_step=_beside(S, b, solos), label='after the restart')
    want = [min(25, len(load_any(PLAN[s])['step'])) if s in PLAN else 25 for s in range(12)]
    assert compared.tolist() == want and want[7] == 12 and want[3] == 25
    assert b.sol.scene_state()['steps'].tolist() == [25 if s in PLAN else 35 for s in range(12)]
    for x in [b] + list(solos.values()):
        x.sol.close()


def test_restart_after_a_natural_finish_with_obstacles_and_the_tracker(S):
    """three 16-agent scenes sharing the take-off field's 8 spheres, stepped with sca_env_step; scene 0 finishes after its recorded 285
    steps and is restarted with F4_sca_circle16_obs's episode: every record of that episode up to its done_step (289 steps), beside a fresh
    context of it alone; the other two finish and stay inert as recorded; the total drops to 0 only at the very end"""
    b = Slots(S, ['F4_sca_takeoff16', 'F4_mixed_takeoff16', 'F4_sca_circle16_obs'])
    assert len(b.obs_radius) == 8
    totals = []
    step = lambda: totals.append(b.sol.env_step(S.NBR_KDTREE))
    compared = b.run_and_check(285, step_fn=step, label='first episode')
    assert compared[0] == 285 and b.sol.scene_state()['active'][0] == 0 and all(v > 0 for v in totals)
    b.restart({0: 'F4_sca_circle16_obs'})
    assert b.sol.active_count() == totals[-1] + 16                  # the batch counts the slot again
    solo = Slots(S, ['F4_sca_circle16_obs'])
    compared = b.run_and_check(289, step_fn=step, after_step=_beside(S, b, {0: solo}), label='second episode')
    records = len(b.fx[0]['step'])
    assert compared[0] == records == 100 and int(b.fx[0]['done_step']) == 288
    sc = b.sol.scene_state()
    assert sc['steps'].tolist() == [289, 331, 289] and not sc['active'].any()
    assert all(v > 0 for v in totals[:-1]) and totals[-1] == 0 and len(totals) == 285 + 289
    b.sol.close()
    solo.sol.close()


MIX = np.array([0, 1, 2, 3, 4, 5] * 2, np.uint8)


def test_per_scene_obstacle_sets(S):
    """three scenes with their own spheres / none / other spheres; after 15 steps the scene WITHOUT obstacles and the last one, whose
    obstacle ids start at 12, are given another episode: both equal a fresh context of that episode alone with the slot's obstacle set for 30
    steps, the first equals its own context straight through, and the neighbours' obstacle ids stay global"""
    first = circle_scene(S, 12, MIX)
    unit = first['goal'] - first['pos']
    unit /= np.linalg.norm(unit, axis=1)[:, None]
    sets = [(np.round(first['pos'] + 3.0 * unit, 2), np.full(12, 0.6)), (np.zeros((0, 3)), np.zeros(0)),
            (np.round(first['pos'] + 5.0 * unit + [0.0, 0.0, 0.4], 2)[::2], np.full(6, 0.9))]
    obs_off = [0, 12, 12, 18]
    sol, off = context(S, [first] * 3, obstacles=sets)
    alone = {0: context(S, [first], obstacles=[sets[0]])[0]}
    for x in [sol, alone[0]]:
        x.run_steps(15, S.NBR_KDTREE)
        x.synchronize()
    new = {2: circle_scene(S, 12, MIX[::-1], turn=3), 1: circle_scene(S, 12, np.roll(MIX, 1), rad=3.0, turn=5)}
    restart_all(sol, [2, 1], [new[2], new[1]])                         # (named out of order: the arrays follow scene_ids)
    for s in (1, 2):
        alone[s] = context(S, [new[s]], obstacles=[sets[s]])[0]
    seen_obstacle = {0: False, 1: False, 2: False}
    for t in range(30):
        for x in [sol] + list(alone.values()):
            x.run_steps(1, S.NBR_KDTREE)
            x.synchronize()
        got = everything(sol)
        for s in range(3):
            lo, hi = int(off[s]), int(off[s + 1])
            assert_scene_equals_alone(got, lo, hi, obs_off[s], everything(alone[s]), ('per-scene obstacles', 'step', t, 'scene', s))
            ids = got['nbr_id'][lo:hi][got['nbr_kind'][lo:hi] == 1]
            assert ((ids >= obs_off[s]) & (ids < obs_off[s + 1])).all(), ('obstacle ids are global', t, s)
            seen_obstacle[s] = seen_obstacle[s] or len(ids) > 0
    assert seen_obstacle[2] and not seen_obstacle[1]
    for x in [sol] + list(alone.values()):
        x.close()


def test_other_entry_points(S):
    """after a restart: sca_run_steps(k) with no synchronisation in between gives what k single steps give (and what the episode alone gives);
    sca_step_host with in_mask == 0 leaves the block holding the restarted state's successor and its action rows"""
    first, new = circle_scene(S, 12, MIX), circle_scene(S, 12, MIX[::-1], rad=3.5, turn=2)
    ctxs = [context(S, [first] * 3)[0] for _ in range(3)]
    for x in ctxs:
        x.host_state()
        x.run_steps(8, S.NBR_KDTREE)
        restart_all(x, [1], [new])
    solo = context(S, [new])[0]
    burst, single, host = ctxs
    burst.run_steps(6, S.NBR_KDTREE)
    for _ in range(6):
        single.run_steps(1, S.NBR_KDTREE)
        single.synchronize()
    solo.run_steps(6, S.NBR_KDTREE)
    a, b_ = everything(burst), everything(single)
    for key in a:
        assert np.array_equal(a[key], b_[key], equal_nan=True), ('burst against single steps', key)
    assert_scene_equals_alone(a, 12, 24, 0, everything(solo), ('burst against the episode alone',))
    # the host block
    solo1 = context(S, [new])[0]
    solo1.run_steps(1, S.NBR_KDTREE)
    active = host.step_host(S.NBR_KDTREE, state=False)
    blk, want, st = host.host_state(), solo1.get_state(), host.get_state()
    assert active == host.active_count() == int(((st['flags'] & 7) == 0).sum())
    for key in ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num'):
        assert np.array_equal(blk[key], st[key]), ('block against the device state', key)
        assert np.array_equal(blk[key][12:24], want[key]), ('block against the episode alone', key)
    assert np.array_equal(blk['action'], host.actions()) and np.array_equal(blk['action'][12:24], solo1.actions())
    assert blk['step_num'][12:24].tolist() == [1] * 12
    for x in ctxs + [solo, solo1]:
        x.close()


def test_refusals_change_nothing(S):
    first, new = circle_scene(S, 12, MIX), circle_scene(S, 12, MIX[::-1], turn=2)
    sol, _ = context(S, [first] * 3)
    sol.run_steps(5, S.NBR_KDTREE)
    before = observe(sol)

    def refused(code, ids=(1,), eps=None, **kw):
        eps = [new] * len(ids) if eps is None else eps
        assert rc_of(S, lambda: restart_all(sol, list(ids), eps, **kw)) == code, (code, ids, sorted(kw))
        after = observe(sol)
        for key in before:
            assert np.array_equal(before[key], after[key]), ('a refused call changed', key, ids, sorted(kw))
    bad = lambda key, value, row=5, col=None: {key: _with(new[key], row, col, value)}
    refused(ERR_ARG, ids=(), eps=[new])                              # count <= 0
    refused(ERR_ARG, ids=(-1,))
    refused(ERR_ARG, ids=(3,))                                       # ids at both ends of the range, outside
    refused(ERR_ARG, ids=(1, 2, 1))                                  # a repeated id
    for key, value, col in (('vel', np.nan, 0), ('goal', np.inf, 2), ('goal_heading', -np.inf, 1), ('radius', np.nan, None),
                            ('pref_speed', np.inf, None), ('max_run_dist', np.nan, None)):
        refused(ERR_ARG, **bad(key, value, col=col))
    refused(ERR_ARG, policy=_with(new['policy'], 11, None, 6))       # a policy above SCA_POLICY_RVO3D_DUBINS
    for key, value in (('radius', 0.0), ('pref_speed', -1.0), ('max_run_dist', 0.0)):
        refused(ERR_ARG, **bad(key, value))
    # pos / heading: NULL, and not finite (the binding always passes them: through the library itself)
    ids = np.array([1], np.int32)
    p, h = np.ascontiguousarray(new['pos']), np.ascontiguousarray(new['heading'])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    raw = lambda idp, pos, head: sol.L.sca_restart_scenes(sol.ctx, 1, idp, pos, None, head, None, None, None, None, None, None, None)
    assert raw(ids.ctypes.data_as(C.POINTER(C.c_int32)), None, dp(h)) == ERR_ARG
    assert raw(ids.ctypes.data_as(C.POINTER(C.c_int32)), dp(p), None) == ERR_ARG
    assert raw(None, dp(p), dp(h)) == ERR_ARG                        # scene_ids NULL
    assert rc_of(S, lambda: sol.restart_scenes([1], _with(new['pos'], 0, 2, np.nan), new['heading'])) == ERR_ARG
    assert rc_of(S, lambda: sol.restart_scenes([1], new['pos'], _with(new['heading'], 3, 0, np.inf))) == ERR_ARG
    after = observe(sol)
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    # between a policy pass and its env update
    sol.policy_pass(S.NBR_KDTREE)
    mid = observe(sol)
    assert rc_of(S, lambda: restart_all(sol, [1], [new])) == ERR_STATE
    for key, v in observe(sol).items():
        assert np.array_equal(mid[key], v), key
    sol.env_update()
    # per-agent tracker attributes: a policy array that moves an agent between tracked and untracked is refused, one that does not is taken
    sol.device_tracker_set_agent_params(turning_radius=np.where(np.arange(36) % 2, 1.5, 2.0))
    before = observe(sol)
    refused(ERR_UNSUPPORTED, policy=np.roll(MIX, 1))                 # agent 1: RVO -> SCA, untracked -> tracked
    restart_all(sol, [1], [new])                                        # MIX reversed: SCA <-> RVO3D+Dubins only, tracked stays tracked
    assert sol.scene_state()['steps'].tolist() == [6, 0, 6]
    sol.close()


def _with(a, row, col, value):
    out = np.array(a, copy=True)
    if col is None:
        out[row] = value
    else:
        out[row, col] = value
    return out


def test_refusals_by_state(S):
    """no scenes, no state yet, goal_heading without a tracker, waypoint lists set"""
    first, new = circle_scene(S, 12, MIX), circle_scene(S, 12, MIX[::-1], turn=2)
    n = 24
    cat = lambda key: np.concatenate([first[key]] * 2)
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    sol.set_agents(cat('radius'), cat('pref_speed'), cat('goal'), cat('policy'), cat('zaxis'), cat('max_run_dist'))
    sol.set_state(cat('pos'), cat('vel'), cat('heading'), np.zeros(n, np.uint8))
    plain = dict(sol.get_state(), perm=sol.get_kd_perm())
    assert rc_of(S, lambda: restart_all(sol, [0], [new], goal_heading=None)) == ERR_STATE          # no scenes
    for key, v in dict(sol.get_state(), perm=sol.get_kd_perm()).items():
        assert np.array_equal(plain[key], v), key
    assert rc_of(S, sol.scene_state) == ERR_STATE                                               # (still none)
    sol.set_agents(cat('radius'), cat('pref_speed'), cat('goal'), cat('policy'), cat('zaxis'), cat('max_run_dist'))
    sol.set_scenes([0, 12, 24])
    perm = sol.get_kd_perm()
    assert rc_of(S, lambda: restart_all(sol, [0], [new], goal_heading=None)) == ERR_STATE          # no state yet
    assert np.array_equal(perm, sol.get_kd_perm())
    assert rc_of(S, sol.get_state) == ERR_STATE and rc_of(S, sol.scene_state) == ERR_STATE        # (still no state: nothing to compare but the permutation)
    sol.set_state(cat('pos'), cat('vel'), cat('heading'), np.zeros(n, np.uint8))
    sol.run_steps(3, S.NBR_KDTREE)
    before = observe(sol)
    assert rc_of(S, lambda: restart_all(sol, [0], [new])) == ERR_ARG                               # goal_heading, and no tracker is enabled
    sol.set_paths([[[1.0, 2.0, 10.0]]] + [[] for _ in range(n - 1)])
    assert rc_of(S, lambda: restart_all(sol, [0], [new], goal_heading=None)) == ERR_UNSUPPORTED    # waypoint lists are set
    after = observe(sol)
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    sol.set_paths(None)
    with pytest.raises(ValueError):                                                           # the binding holds every array against T
        restart_all(sol, [0], [new], goal_heading=None, radius=new['radius'][:11])
    with pytest.raises(ValueError):
        sol.restart_scenes([0, 1], new['pos'], new['heading'])
    for key, v in observe(sol).items():
        assert np.array_equal(before[key], v), key
    restart_all(sol, [0], [new], goal_heading=None)                                              # ... and without them it is taken
    assert sol.scene_state()['steps'].tolist() == [0, 3]
    sol.close()


def _alone(S, e, obstacles=None, solver=None, planner=None, lists=None):
    """a fresh context of the episode alone with what a restart can bring: its obstacle set, attributes and waypoint lists"""
    n = e['n']
    sol = S.BatchedSolver(max_agents=n, max_obstacles=max(len(obstacles[1]) if obstacles else 0, 1))
    sol.set_agents(e['radius'], e['pref_speed'], e['goal'], e['policy'], e['zaxis'], e['max_run_dist'])
    if solver:
        sol.set_agent_params(**solver)
    sol.set_scenes(np.array([0, n], np.int32))
    if obstacles and len(obstacles[1]):
        sol.set_scene_obstacles([obstacles])
    if lists is not None:
        sol.set_paths(lists)
    sol.set_state(e['pos'], e['vel'], e['heading'], np.zeros(n, np.uint8))
    sol.device_tracker_enable(e['goal_heading'], in_pass=True)
    if planner:
        sol.device_tracker_set_agent_params(**planner)
    return sol


def test_first_uses_in_one_context(S):
    """The three allocate-and-fill stages around the launch, crossed in ONE context: scenes of capacities 3, 1 and 4, the tracker, obstacle
    slots and path slots (W = 2) on, tracked, ORCA3D-LP and other policies mixed.  Scene 2 is restarted five times -- plain; sized (2 of 4);
    with 2 obstacles; with attributes (the first use of the per-agent solver records and of the planner's per-row arrays and classes);
    with lists -- and after each restart and two steps every scene equals a fresh context of its episode alone, every value: the scenes
    that are never named run on through the first-use fills as if nothing had happened."""
    cap, obs_cap, obs_lo = [3, 1, 4], [2, 0, 2], [0, 2, 2]
    ep = lambda n, policy, turn=0: circle_scene(S, n, np.asarray(policy, np.uint8), rad=3.0, turn=turn)
    spheres = lambda k, z: (np.array([[0.5 * i, 0.25, z] for i in range(k)]), np.full(k, 0.4))
    base = [ep(3, [0, 4, 1]), ep(1, [5]), ep(4, [4, 0, 3, 2])]
    set0 = spheres(1, 10.0)
    sol, off = context(S, base, obstacles=[set0, None, None], obs_slots=obs_cap)
    sol.set_path_slots(2)
    assert np.diff(off).tolist() == cap
    solos = {0: _alone(S, base[0], obstacles=set0), 1: _alone(S, base[1])}
    held = {0: base[0], 1: base[1]}
    solver = dict(neighbor_dist=np.array([6.0, 10.0, 4.0, 8.0]), max_neighbors=np.array([3, 16, 2, 5], np.int32), max_heading_change=np.array([0.5, 0.7, 0.5, 0.9]))
    planner = dict(turning_radius=np.array([1.5, 2.0, 1.0, 1.0]), pitch_lo=np.full(4, -0.5), pitch_hi=np.array([0.5, 0.6, 0.5, 0.5]))
    lists = [[], [[1.0, 0.5, 10.0]], [[0.0, 1.0, 10.0], [2.0, 2.0, 10.5]], [[-1.0, 0.0, 9.5]]]
    two = spheres(2, 10.2)
    # (the episode, what the call brings, what the fresh context is given).  The obstacles of stage 3 and the attributes of stage 4 stay
    # with the slot; behind stage 4 a call without attributes must keep every row tracked or untracked as it was.
    stages = [('plain', ep(4, [0, 4, 5, 1], 1), {}, {}),
              ('sized', ep(2, [4, 0], 2), dict(sizes=[2]), {}),
              ('obstacles', ep(3, [5, 4, 2], 3), dict(sizes=[3], obstacles=[two]), dict(obstacles=two)),
              ('attrs', ep(4, [0, 5, 4, 1], 4), dict(attrs=dict(solver, **planner)), dict(obstacles=two, solver=solver, planner=planner)),
              ('lists', ep(4, [5, 0, 1, 4], 5), dict(paths=lists), dict(obstacles=two, solver=solver, planner=planner, lists=lists))]
    for k, (name, e, brings, alone_kw) in enumerate(stages):
        restart_all(sol, [2], [e], **brings)
        assert sol.scene_sizes().tolist() == [3, 1, e['n']], name
        held[2], solos[2] = e, _alone(S, e, **alone_kw)
        for x in [sol] + list(solos.values()):
            x.run_steps(2, S.NBR_KDTREE)
            x.synchronize()
        got = assert_slots_equal_alone(sol, off, held, solos, ('stage', k, name), obs_lo=obs_lo)
        assert_vacant(got, off, [3, 1, e['n']], ('stage', k, name))
        assert sol.scene_state()['steps'].tolist() == [2 * (k + 1), 2 * (k + 1), 2], name
        solos.pop(2).close()
    for x in [sol] + list(solos.values()):
        x.close()
