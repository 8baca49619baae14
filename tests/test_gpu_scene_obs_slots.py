"""Obstacle slots (-m gpu): sca_set_scene_obstacle_slots makes a scene's obstacle range a capacity and sca_restart_scenes_obstacles brings a
new episode's own obstacles into the slot it takes.  The bar is the scene contract, no tolerance: a restarted slot is bit for bit a fresh
context that holds that episode alone after sca_set_agents + sca_set_obstacles(that set) + sca_set_state (+ the tracker's enable) -- state,
action rows, neighbour lists with their distSq and global obstacle ids, diagnostics, permutation, tracker records, log rows, harvest --
and, where the reference recorded the episode, its records; and no other scene can tell the call happened."""
import ctypes as C
import json

import numpy as np
import pytest

from scene_util import (NO_OBSTACLES, SizedSlots, agents_of, assert_scene_equals_alone, assert_slots_equal_alone, assert_summary, circle_scene, context,
                        everything, load_any, loop_summary, padded, recorded_arrays, restart_all, same, step_all, tracked)

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3                                         # include/sca_hip.h
MIX = np.array([0, 1, 2, 3, 4, 5], np.uint8)
BATCH = ['F4_sca_takeoff16', 'F4_sca_circle16_obs', 'F14_fuzz_episode_00', 'F1_sca_circle8']      # 8, 8, 4 and 0 obstacles of their own


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


def own_set(ep):
    return ep['obs_pos'], ep['obs_radius']


def alone(S, ep, obstacles=NO_OBSTACLES, tracker=True, history=0):
    """the episode in a context of its own, no scenes: sca_set_agents + sca_set_obstacles(that set) + sca_set_state (+ the tracker)"""
    n = ep['n']
    sol = S.BatchedSolver(max_agents=n, max_obstacles=max(len(obstacles[1]), 1))
    sol.set_obstacles(np.asarray(obstacles[0], float).reshape(-1, 3), np.asarray(obstacles[1], float))
    sol.set_agents(ep['radius'], ep['pref_speed'], ep['goal'], ep['policy'], ep['zaxis'], ep['max_run_dist'])
    if tracker:
        sol.device_tracker_enable(ep['goal_heading'], in_pass=True)
    sol.set_state(ep['pos'], ep['vel'], ep['heading'], np.zeros(n, np.uint8))
    if history:
        sol.history_enable(history)
    return sol


class Lockstep:
    """a context alone beside a slot: stepped while it is live and no further -- a finished scene of a batch is inert, the reference has
    stopped calling env.step() for it, whereas a context of its own would go on passing its done agents through the update"""

    def __init__(self, S, sol):
        self.S, self.sol, self.live, self.was_live, self.steps = S, sol, True, True, 0

    def step(self, k=1):
        for _ in range(k):
            self.was_live = self.live                                # ... when the last step began
            if self.live:
                self.live = self.sol.env_step(self.S.NBR_KDTREE) > 0
                self.steps += 1


def assert_beside(sol, off, held, beside, ctx, obs_lo):
    """every slot of the batch against its context alone (beside: {slot: Lockstep}), every value of the contract; a slot whose episode had
    ended before the last step is inert instead: the state its last step left, its action rows zero"""
    running = {s: x.sol for s, x in beside.items() if x.was_live}
    got = assert_slots_equal_alone(sol, off, {s: held[s] for s in running}, running, ctx, obs_lo=obs_lo)
    for s, x in beside.items():
        if not x.was_live:
            lo, st = int(off[s]), x.sol.get_state()
            for k in st:
                assert np.array_equal(got[k][lo:lo + held[s]['n']], st[k]), ctx + ('inert', s, k)
            assert np.array_equal(got['perm'][lo:lo + held[s]['n']] - lo, x.sol.get_kd_perm()) and not got['action'][lo:lo + held[s]['n']].any(), ctx + ('inert', s)
    return got


def spheres(seed, m, radius=0.3, spread=2.0, z=10.0):
    """m seeded spheres around the middle of the hand-made circles (radius 3 .. 4 at z = 10): none touches a start position"""
    rng = np.random.default_rng(seed)
    pos = np.round(np.concatenate([rng.uniform(-spread, spread, (m, 2)), z + rng.uniform(-0.5, 0.5, (m, 1))], axis=1), 2)
    return pos, np.full(m, radius)


def raw_restart(sol, ids, ep, sizes=None, obs_counts=None, obs_pos=None, obs_radius=None, tracker=True):
    """sca_restart_scenes_obstacles itself, any pointer NULL: (rc, message)"""
    from sca_amd import _lib
    keep = []

    def p(a, dt, ct):
        if a is None:
            return None
        b = np.ascontiguousarray(a, dt)
        keep.append(b)
        return _lib.ptr(b, ct)
    i32, f64 = (lambda a: p(a, np.int32, C.c_int32)), (lambda a: p(a, np.float64, C.c_double))
    rc = sol.L.sca_restart_scenes_obstacles(sol.ctx, len(ids), i32(ids), i32(sizes), i32(obs_counts), f64(obs_pos), f64(obs_radius), f64(ep['pos']),
                                            p(ep['vel'], np.float32, C.c_float), f64(ep['heading']), f64(ep['radius']), f64(ep['pref_speed']), f64(ep['goal']),
                                            p(ep['policy'], np.uint8, C.c_uint8), p(ep['zaxis'], np.uint8, C.c_uint8), f64(ep['max_run_dist']),
                                            f64(ep['goal_heading']) if tracker else None)
    return rc, sol.L.sca_last_error(sol.ctx).decode()


def batch_of_test_1(S, slots=True):
    eps = [recorded_arrays(load_any(n)) for n in BATCH]
    sets = [own_set(e) for e in eps]
    if slots:
        sol, off = context(S, eps, obstacles=sets, obs_slots=[len(r) for _, r in sets])
    else:
        sol, off = context(S, eps, obstacles=sets)
    return sol, off, eps, sets


def all_tracked(off, eps):
    return [int(off[s]) + a for s, e in enumerate(eps) for a in tracked(e)]


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------
def test_slots_equal_sets(S):
    """the batch through sca_set_scene_obstacles and through the slots call with count == capacity, free-running to the end: everything()
    equal at every step -- neighbour lists, obstacle ids and form bits included"""
    a, off, eps, sets = batch_of_test_1(S, slots=False)
    b = batch_of_test_1(S, slots=True)[0]
    assert [len(r) for _, r in sets] == [8, 8, 4, 0]
    oc = b.scene_obstacle_counts()
    assert oc['counts'].tolist() == [8, 8, 4, 0] and oc['capacities'].tolist() == [8, 8, 4, 0]
    oc = a.scene_obstacle_counts()                                   # sca_set_scene_obstacles leaves slots that are full
    assert oc['counts'].tolist() == [8, 8, 4, 0] and oc['capacities'].tolist() == [8, 8, 4, 0]
    ids = all_tracked(off, eps)
    same(everything(a, ids), everything(b, ids), ('before the first step',))
    saw_obstacle = False
    for t in range(600):
        left = a.env_step(S.NBR_KDTREE)
        assert b.env_step(S.NBR_KDTREE) == left
        some = ids if t % 25 == 0 or left == 0 else ()               # (a tracker record is a read-back per agent: every 25th step and at the end)
        ea, eb = everything(a, some), everything(b, some)
        same(ea, eb, ('slots against sets', 'step', t))
        assert a.pass_forms() == b.pass_forms() and a.pass_forms() & S.FORM_SCENE_OBSTACLES
        saw_obstacle = saw_obstacle or bool((ea['nbr_kind'] == 1).any())
        if left == 0:
            break
    assert t >= 288 and saw_obstacle                                 # (the circle among the spheres ends at step 288, the take-off field at 284)
    sa, sb = a.scene_state(), b.scene_state()
    assert np.array_equal(sa['steps'], sb['steps']) and np.array_equal(sa['active'], sb['active']) and sa['steps'].tolist()[:2] == [285, 289]
    a.close(); b.close()


# ---- 2 and 10: recorded episodes through refilled slots ------------------------------------------------------------------------------------------
AGENT_CAPS, OBS_CAPS = [16, 20, 40], [8, 8, 5]
START = ['F4_sca_takeoff16', 'F13_fuzz_track_00', 'F14_fuzz_episode_01']                        # 16 / 8, 12 / 3, 40 / 4 (agents / obstacles)
# batch step -> {slot: episode}.  Slot 0's take-off episode runs to its end (285 steps) and is refilled as a FINISHED slot; the fuzz
# episodes have no end in their records (40 and 20 steps): slots 1 and 2 are refilled IN FLIGHT.  Sets shrink (4 -> 3, 8 -> 4) and grow
# (3 -> 4, 4 -> 8) in both of them.
REFILLS = {20: {1: 'F14_fuzz_episode_00', 2: 'F13_fuzz_track_01'}, 40: {1: 'F4_mixed_takeoff16', 2: 'F14_fuzz_episode_02'}, 60: {2: 'F13_fuzz_track_02'},
           100: {2: 'F13_fuzz_track_03'}, 285: {0: 'F4_sca_circle16_obs', 1: 'F14_fuzz_episode_02', 2: 'F14_fuzz_episode_01'}}
END = 310


class ObsSlots(SizedSlots):
    """Recorded episodes as slots of an agent AND an obstacle capacity: slot s starts with names[s] and its recorded set; restart() brings a
    recorded episode of any count that fits together with ITS recorded set (one sca_restart_scenes_obstacles call)."""

    def __init__(self, S, names, agent_caps, obs_caps, max_obstacles=None):
        self.S, self.B = S, len(names)
        self.names = list(names)
        self.fx = [load_any(x) for x in names]
        ep = [recorded_arrays(f) for f in self.fx]
        self.tracker = True
        self.sol, self.off = context(S, [padded(e, c) for e, c in zip(ep, agent_caps)], obstacles=[own_set(e) for e in ep], obs_slots=obs_caps,
                                     max_obstacles=max_obstacles)
        self.obs_off = np.concatenate([[0], np.cumsum(obs_caps)]).astype(np.int32)
        restart_all(self.sol, list(range(self.B)), ep, sizes='own')  # vacates the rows behind the episodes; no obstacle argument: the sets stay
        self.size = np.array([e['n'] for e in ep])
        self.held = ep
        self.n = int(self.off[-1])
        self.t = 0
        self.t0 = [0] * self.B
        self.steps_want = np.zeros(self.B, np.int64)
        self._bind()

    def restart(self, plan):
        ids = sorted(plan)
        fx = {s: load_any(plan[s]) for s in ids}
        ep = [recorded_arrays(fx[s]) for s in ids]
        restart_all(self.sol, ids, ep, sizes='own', obstacles=[own_set(e) for e in ep])
        for s, e in zip(ids, ep):
            self.fx[s], self.names[s], self.t0[s], self.steps_want[s], self.size[s], self.held[s] = fx[s], plan[s], self.t, 0, e['n'], e
        self._bind()

    def counts(self):
        return self.sol.scene_obstacle_counts()['counts'].tolist()


def test_recorded_episodes_through_refilled_slots(S):
    b = ObsSlots(S, START, AGENT_CAPS, OBS_CAPS)
    assert b.counts() == [8, 3, 4] and b.sol.scene_obstacle_counts()['capacities'].tolist() == OBS_CAPS
    compared, want, shrank, grew, in_flight = np.zeros(3, np.int64), np.zeros(3, np.int64), 0, 0, 0
    phase = {s: (0, n) for s, n in enumerate(START)}                 # slot -> (the batch step its episode came in, its name)
    marks = sorted(REFILLS) + [END]
    for upto in marks:
        compared += b.run_and_check(upto - b.t, label='refilled slots')
        if upto == END:
            break
        before, active = b.counts(), b.sol.scene_state()['active']
        for s in REFILLS[upto]:
            f = load_any(phase[s][1])
            want[s] += sum(1 for t in f['step'] if int(t) < upto - phase[s][0])
            phase[s] = (upto, REFILLS[upto][s])
            in_flight += int(active[s] > 0)
        if upto == 285:
            assert active[0] == 0                                    # slot 0 had finished: the take-off episode ends with its step 284
        b.restart(REFILLS[upto])
        after = b.counts()
        shrank += sum(after[s] < before[s] for s in REFILLS[upto])
        grew += sum(after[s] > before[s] for s in REFILLS[upto])
        assert after == [len(e['obs_radius']) for e in b.held], upto
        assert b.sol.scene_sizes().tolist() == [e['n'] for e in b.held]
    for s, (t0, name) in phase.items():
        want[s] += sum(1 for t in load_any(name)['step'] if int(t) < END - t0)
    assert compared.tolist() == want.tolist() and (compared >= [285, 20 + 20 + 245, 20 + 20 + 20 + 40 + 40 + 20]).all(), (compared, want)
    assert shrank >= 2 and grew >= 2                                 # a set smaller than the one before it and a larger one both occur
    assert in_flight >= 4                                            # (the refills at steps 20 and 40 at the least: those episodes have no end in their records)
    assert b.sol.pass_forms() & S.FORM_SCENE_OBSTACLES
    b.sol.close()


def test_log_harvest_and_tracker_through_refilled_slots(S):
    """the schedule above once more with the log per scene, the harvest and the device tracker on: every episode's log rows equal
    sca_get_history of a context of that episode alone, every value equals it when the episode leaves, and the harvest of the episodes that
    finish (the two take-off episodes) equals the summary loop over the context alone"""
    b = ObsSlots(S, START, AGENT_CAPS, OBS_CAPS)
    b.sol.scene_history_enable(64)
    b.sol.scene_harvest_enable()
    hv = b.sol.scene_harvest()
    solo = {s: Lockstep(S, alone(S, b.held[s], own_set(b.held[s]), history=64)) for s in range(3)}
    same_log = lambda s: all(np.array_equal(b.sol.scene_history(s)[k], solo[s].sol.history()[k]) for k in ('pos', 'heading', 'vel'))
    harvested = []
    t = 0
    for upto in sorted(REFILLS) + [END]:
        for _ in range(upto - t):
            b.sol.env_step(S.NBR_KDTREE)
            for x in solo.values():
                x.step()
        for s in b.sol.scene_harvest_collect():
            st = solo[s].sol.get_state()
            assert not solo[s].live
            assert_summary(hv['summary'][s], loop_summary(st, 0, b.held[s]['n']), solo[s].steps, b.t0[s] + solo[s].steps, ('harvest', b.names[s]))
            lo = int(b.off[s])
            for k in ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num'):
                assert np.array_equal(hv[k][lo:lo + b.held[s]['n']], st[k]), ('harvested rows', b.names[s], k)
            harvested.append(b.names[s])
        t = b.t = upto
        assert_beside(b.sol, b.off, dict(enumerate(b.held)), solo, ('batch step', upto), dict(enumerate(b.obs_off[:-1].tolist())))
        rows, steps = b.sol.scene_history_rows()['logged'].tolist(), b.sol.scene_state()['steps'].tolist()
        for s in range(3):
            assert steps[s] == solo[s].steps and rows[s] == min(64, steps[s]) == solo[s].sol.history_rows()[0] and same_log(s), ('log', upto, s, b.names[s])
        if upto == END:
            break
        b.restart(REFILLS[upto])
        for s in REFILLS[upto]:
            solo[s].sol.close()
            solo[s] = Lockstep(S, alone(S, b.held[s], own_set(b.held[s]), history=64))
            assert b.sol.scene_history_rows()['logged'][s] == 0
    assert 'F4_sca_takeoff16' in harvested and (solo[0].steps, harvested.count('F4_sca_takeoff16')) == (25, 1)
    for x in [b.sol] + [x.sol for x in solo.values()]:
        x.close()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------
def test_count_edges_against_a_context_alone(S):
    """a 4-agent slot of obstacle capacity 23 (behind a neighbour of capacity 5) takes sets of 0, 1, 10, 11, 21, 23 and again 1 spheres: no
    tree, one leaf, a full leaf, the first split, a deeper tree, the capacity, and back.  Each episode 40 steps against a fresh context with
    sca_set_obstacles of that set."""
    other, other_set = circle_scene(S, 6, MIX, rad=4.0), spheres(5, 5)
    first = circle_scene(S, 4, MIX[:4], rad=3.0)
    sol, off = context(S, [other, first], obstacles=[other_set, None], obs_slots=[5, 23])
    beside = Lockstep(S, alone(S, other, other_set))
    saw = set()
    for k, m in enumerate((0, 1, 10, 11, 21, 23, 1)):
        ep = circle_scene(S, 4, np.roll(MIX, k)[:4], rad=3.0, turn=k)
        new = spheres(100 + k, m)
        restart_all(sol, [1], [ep], sizes='own', obstacles=[new])
        oc = sol.scene_obstacle_counts()
        assert oc['counts'].tolist() == [5, m] and oc['capacities'].tolist() == [5, 23]
        solo = Lockstep(S, alone(S, ep, new))
        for t in range(40):
            sol.env_step(S.NBR_KDTREE)
            solo.step(); beside.step()
            got = assert_beside(sol, off, {0: other, 1: ep}, {0: beside, 1: solo}, ('count', m, 'step', t), {0: 0, 1: 5})
            assert sol.scene_state()['steps'].tolist() == [beside.steps, solo.steps]
            if (got['nbr_kind'][4 + 2:] == 1).any():
                saw.add(m)
                listed = got['nbr_id'][6:][got['nbr_kind'][6:] == 1]
                assert (listed >= 5).all() and (listed < 5 + m).all(), ('an obstacle id outside the slot\'s occupied rows', m, t)
        solo.sol.close()
    assert saw >= {1, 10, 11, 21, 23}, saw                           # every set was met by somebody
    sol.close(); beside.sol.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------
def _ghost_sets():
    """twelve spheres (a root and two leaves), one of them in the middle of the circle, where every agent's straight line passes; and one
    sphere far above everything"""
    pos, radius = spheres(7, 12, radius=0.4, spread=1.5)
    pos[0] = [0.0, 0.0, 10.0]
    radius[0] = 0.8
    return (pos, radius), (np.array([[0.0, 0.0, 60.0]]), np.array([0.5]))


@pytest.mark.parametrize('order', ['sphere first', 'sphere second'])
def test_through_the_ghost(S, order):
    """an episode whose sphere sits on the agents' straight lines takes a detour or collides; the slot restarted with a set that has no
    sphere there runs like the obstacle-free context, no obstacle in any list -- the rows and nodes of the twelve-sphere tree behind the
    new count are unreachable.  And the other way round."""
    middle, far = _ghost_sets()
    ep = circle_scene(S, 4, [3, 1, 2, 4], rad=3.0)
    free = alone(S, ep)
    step_all(S, free, k=40)
    want_free = everything(free)
    sets = [middle, far] if order == 'sphere first' else [far, middle]
    sol, off = context(S, [ep], obstacles=[sets[0]], obs_slots=[12])
    for k, now in enumerate(sets):
        if k:
            restart_all(sol, [0], [ep], sizes='own', obstacles=[now])
            assert sol.scene_obstacle_counts()['counts'].tolist() == [len(now[1])]
        solo = Lockstep(S, alone(S, ep, now))
        saw_obstacle = False
        for t in range(40):
            sol.env_step(S.NBR_KDTREE)
            solo.step()
            got = assert_beside(sol, off, {0: ep}, {0: solo}, (order, 'set', k, 'step', t), {0: 0})
            saw_obstacle = saw_obstacle or bool((got['nbr_kind'] == 1).any())
        if now is middle:
            assert saw_obstacle and ((got['flags'] & 2).any() or not np.array_equal(got['pos'], want_free['pos'])), 'neither a collision nor a detour'
        else:
            assert not saw_obstacle
            assert solo.steps == 40                                  # (nobody within 6 m of a goal 40 steps in: both ran all of them)
            same(got, want_free, (order, 'against the obstacle-free context'), keys=[k_ for k_ in want_free if k_ != 'track'])
        solo.sol.close()
    sol.close(); free.close()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------
def test_keep(S):
    """obs_counts[e] = -1 and obs_counts = NULL both equal sca_restart_scenes_sized on the same batch: state and everything() for 10 steps"""
    new = recorded_arrays(load_any('F4_mixed_takeoff16'))            # 16 agents into scene 1, which keeps the circle's 8 spheres
    batches = [batch_of_test_1(S) for _ in range(3)]
    off, eps = batches[0][1], batches[0][2]
    for sol, *_ in batches:
        step_all(S, sol, k=5)
    restart_all(batches[0][0], [1, 3], [new, eps[3]], sizes='own')
    restart_all(batches[1][0], [1, 3], [new, eps[3]], sizes='own', obstacles=[None, None])
    both = {k: np.concatenate([new[k], eps[3][k]]) for k in new if k not in ('n', 'obs_pos', 'obs_radius')}
    rc, msg = raw_restart(batches[2][0], [1, 3], both, sizes=[16, 8], obs_counts=None)
    assert rc == 0, msg
    ids = all_tracked(off, [eps[0], new, eps[2], eps[3]])
    for t in range(11):
        want = everything(batches[0][0], ids)
        for k, (sol, *_) in enumerate(batches[1:]):
            same(want, everything(sol, ids), ('keep', ('-1', 'NULL')[k], 'step', t))
            assert sol.scene_obstacle_counts()['counts'].tolist() == [8, 8, 4, 0]
        for sol, *_ in batches:
            step_all(S, sol)
    for sol, *_ in batches:
        sol.close()


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------------
def test_no_other_scene_can_tell(S):
    """20 steps with scene 1 restarted at step 7 with a new episode and a new set, and 20 steps without: scenes 0, 2 and 3 equal at every step"""
    a, off, eps, _ = batch_of_test_1(S)
    b = batch_of_test_1(S)[0]
    new, new_set = circle_scene(S, 16, np.resize(MIX, 16), rad=4.0), spheres(11, 6)
    ids = [int(off[s]) + i for s in (0, 2, 3) for i in tracked(eps[s])]
    for t in range(20):
        if t == 7:
            restart_all(a, [1], [new], sizes='own', obstacles=[new_set])
            assert a.scene_obstacle_counts()['counts'].tolist() == [8, 6, 4, 0] and b.scene_obstacle_counts()['counts'].tolist() == [8, 8, 4, 0]
        ea, eb = everything(a, ids), everything(b, ids)
        for s in (0, 2, 3):
            sl = slice(int(off[s]), int(off[s + 1]))
            for key in ea:
                if key == 'track':
                    for i in ea[key]:
                        assert np.array_equal(ea[key][i], eb[key][i], equal_nan=True), ('scene', s, 'step', t, key, i)
                else:
                    assert np.array_equal(ea[key][sl], eb[key][sl], equal_nan=True), ('scene', s, 'step', t, key)
        if t >= 7:
            assert not np.array_equal(ea['pos'][16:32], eb['pos'][16:32])
        step_all(S, a, b)
    a.close(); b.close()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_filter_stays_a_filter(S):
    """one slot is restarted with radius-3 spheres, afterwards another with radius-0.2 spheres: the context's obstacle reach has grown to
    the large radius and stays there, and the second scene still equals its own context alone, whose reach is that of 0.2"""
    big_ep, small_ep = circle_scene(S, 6, MIX, rad=9.0), circle_scene(S, 8, np.resize(MIX, 8), rad=3.0)
    big = (np.array([[0.0, 0.0, 10.0], [0.0, 0.0, 17.0]]), np.full(2, 3.0))
    small = spheres(3, 9, radius=0.2, spread=2.2)
    sol, off = context(S, [big_ep, small_ep], obs_slots=[4, 9])
    step_all(S, sol, k=3)
    restart_all(sol, [0], [big_ep], sizes='own', obstacles=[big])
    step_all(S, sol, k=2)
    restart_all(sol, [1], [small_ep], sizes='own', obstacles=[small])
    solo, beside = Lockstep(S, alone(S, small_ep, small)), Lockstep(S, alone(S, big_ep, big))
    beside.step(2)
    saw = False
    for t in range(40):
        sol.env_step(S.NBR_KDTREE)
        solo.step(); beside.step()
        got = assert_beside(sol, off, {0: big_ep, 1: small_ep}, {0: beside, 1: solo}, ('filter', 'step', t), {0: 0, 1: 4})
        saw = saw or bool((got['nbr_kind'][6:] == 1).any())
    assert saw
    for x in (sol, solo.sol, beside.sol):
        x.close()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------------
def test_every_step_form_behind_an_obstacle_restart(S):
    """sca_env_step, sca_run_steps(5), sca_policy_pass + sca_env_update and sca_step_host (every agent slot full) on the batch of test 1
    behind one obstacle restart of scene 1: the states of the sca_env_step run"""
    new, new_set = circle_scene(S, 16, np.resize(MIX, 16), rad=4.0), spheres(21, 7)
    forms = dict(env_step=lambda x: [x.env_step(S.NBR_KDTREE) for _ in range(5)],
                 run_steps=lambda x: (x.run_steps(5, S.NBR_KDTREE), x.synchronize()),
                 split=lambda x: [(x.policy_pass(S.NBR_KDTREE), x.env_update()) for _ in range(5)],
                 step_host=lambda x: [x.step_host(S.NBR_KDTREE, state=(k == 0)) for k in range(5)])
    results = {}
    for name, form in forms.items():
        sol, off, eps, _ = batch_of_test_1(S)
        step_all(S, sol, k=4)
        if name == 'step_host':
            h = sol.host_state()
        restart_all(sol, [1], [new], sizes='own', obstacles=[new_set])
        if name == 'step_host':
            st = sol.get_state()
            for k in ('pos', 'heading', 'flags', 'total_dist', 'step_num', 'vel'):
                h[k][...] = st[k]
        form(sol)
        results[name] = everything(sol)
        assert sol.pass_forms() & S.FORM_SCENE_OBSTACLES and sol.scene_state()['steps'].tolist() == [9, 5, 9, 9], name
        sol.close()
    solo = alone(S, new, new_set)
    step_all(S, solo, k=5)
    assert_scene_equals_alone(results['env_step'], 16, 32, 8, everything(solo), ('env_step', 'scene 1 alone'))
    solo.close()
    for name in ('run_steps', 'split', 'step_host'):
        same(results['env_step'], results[name], ('step form', name), keys=('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num', 'perm', 'action'))


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------------------
def test_exp3_map_into_a_slot(S):
    """a slot of obstacle capacity 1491 holds the 8-sphere take-off episode, is restarted with the exp3 search among its 1491 spheres (its
    first 12 recorded steps), then with the take-off episode again: 8 obstacles in front of 1483 stale rows and 2966 stale nodes"""
    b = ObsSlots(S, ['F4_sca_takeoff16'], [16], [1491])
    assert b.counts() == [8]
    assert b.run_and_check(6, label='take-off in the map slot').tolist() == [6]
    b.restart({0: 'F10_sca_exp3_map'})
    assert b.counts() == [1491]
    saw = []
    assert b.run_and_check(12, label='exp3', after_step=lambda t: saw.append(bool((b.sol.neighbors()['nbr_kind'] == 1).any()))).tolist() == [12]
    assert any(saw)
    b.restart({0: 'F4_sca_takeoff16'})
    assert b.counts() == [8]
    assert b.run_and_check(12, label='take-off again').tolist() == [12]
    b.sol.close()


# ---- 11 --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(S):
    from sca_amd import _lib
    eps = [circle_scene(S, 6, MIX, rad=4.0), circle_scene(S, 4, MIX[:4], rad=3.0)]
    sets = [spheres(31, 3), spheres(32, 2)]
    sol, off = context(S, eps, obstacles=sets, obs_slots=[5, 4], max_obstacles=9)
    twin = context(S, eps, obstacles=sets, obs_slots=[5, 4], max_obstacles=9)[0]
    pos, rad = np.concatenate([p for p, _ in sets]), np.concatenate([r for _, r in sets])

    def unchanged(ctx):
        same(everything(twin), everything(sol), ctx)
        ca, cb = twin.scene_obstacle_counts(), sol.scene_obstacle_counts()
        assert ca['counts'].tolist() == cb['counts'].tolist() == [3, 2] and cb['capacities'].tolist() == [5, 4], ctx
        for t in range(3):
            step_all(S, sol, twin)
            same(everything(twin), everything(sol), ctx + ('step', t))

    def slots(offsets, counts, nscenes=None, p=pos, r=rad):
        o = None if offsets is None else np.ascontiguousarray(offsets, np.int32)
        c = None if counts is None else np.ascontiguousarray(counts, np.int32)
        rc = sol.L.sca_set_scene_obstacle_slots(sol.ctx, 2 if nscenes is None else nscenes, None if o is None else _lib.ptr(o, C.c_int32),
                                                None if c is None else _lib.ptr(c, C.c_int32), None if p is None else _lib.ptr(np.ascontiguousarray(p), C.c_double),
                                                None if r is None else _lib.ptr(np.ascontiguousarray(r), C.c_double))
        return rc, sol.L.sca_last_error(sol.ctx).decode()
    bad_pos, zero_r = pos.copy(), rad.copy()
    bad_pos[4, 1], zero_r[3] = np.nan, 0.0
    for kw, needle in [(dict(offsets=[0, 5, 9], counts=[3, 2], nscenes=3), 'the context holds 2 scenes'), (dict(offsets=None, counts=[3, 2]), 'cap_offsets is NULL'),
                       (dict(offsets=[1, 5, 9], counts=[3, 2]), 'cap_offsets[0] must be 0'), (dict(offsets=[0, 5, 4], counts=[3, 2]), 'must not decrease (scene 1)'),
                       (dict(offsets=[0, 5, 10], counts=[3, 2]), "sca_create's max_obstacles is 9"), (dict(offsets=[0, 2, 9], counts=[3, 2]), 'counts[0] = 3'),
                       (dict(offsets=[0, 5, 9], counts=[3, -1]), 'counts[1] = -1'), (dict(offsets=[0, 5, 9], counts=[3, 2], p=bad_pos), 'obstacle row 4 (scene 1) has a position that is not finite'),
                       (dict(offsets=[0, 5, 9], counts=[3, 2], r=zero_r), 'obstacle row 3 (scene 1) has a radius that is not positive'),
                       (dict(offsets=[0, 5, 9], counts=[3, 2], p=None), 'must not be NULL with 5 obstacles'), (dict(offsets=[0, 5, 9], counts=[3, 2], r=None), 'must not be NULL')]:
        rc, msg = slots(**kw)
        assert rc == ERR_ARG and needle in msg and msg.startswith('sca_set_scene_obstacle_slots'), (kw, rc, msg)
        unchanged(('slots call', needle))
    ep, new = eps[1], spheres(33, 4)
    bad_new, neg_r = new[0].copy(), new[1].copy()
    bad_new[2, 0], neg_r[1] = np.inf, -0.3
    for kw, needle in [(dict(obs_counts=[-2], obs_pos=new[0], obs_radius=new[1]), 'obs_counts[0] = -2'), (dict(obs_counts=[5], obs_pos=new[0], obs_radius=new[1]), 'obs_counts[0] = 5'),
                       (dict(obs_counts=[4], obs_pos=bad_new, obs_radius=new[1]), 'obstacle row 2 has a position that is not finite'),
                       (dict(obs_counts=[4], obs_pos=new[0], obs_radius=neg_r), 'obstacle row 1 has a radius that is not positive'),
                       (dict(obs_counts=[4], obs_pos=None, obs_radius=new[1]), 'must not be NULL with 4 obstacles'),
                       (dict(obs_counts=[4], obs_pos=new[0], obs_radius=None), 'must not be NULL with 4 obstacles')]:
        rc, msg = raw_restart(sol, [1], ep, sizes=[4], **kw)
        assert rc == ERR_ARG and needle in msg and msg.startswith('sca_restart_scenes_obstacles'), (kw, rc, msg)
        unchanged(('restart', needle))
    # the sized restart's own refusals come first, and leave the obstacles alone too
    rc, msg = raw_restart(sol, [1], ep, sizes=[5], obs_counts=[4], obs_pos=new[0], obs_radius=new[1])
    assert rc == ERR_ARG and 'sizes[0] = 5' in msg
    unchanged(('restart', 'a size above the capacity'))
    sol.close(); twin.close()
    # SCA_ERR_STATE: no scenes; and a count >= 0 in a context that has scenes but no obstacle slots (-1 and NULL are fine there)
    bare, _ = context(S, eps)
    twin, _ = context(S, eps)
    rc, msg = raw_restart(bare, [1], ep, sizes=[4], obs_counts=[0])
    assert rc == ERR_STATE and 'no obstacle slots' in msg and 'obs_counts[0] = 0' in msg, (rc, msg)
    with pytest.raises(S.ScaError):
        bare.scene_obstacle_counts()
    same(everything(twin), everything(bare), ('no slots',))
    assert raw_restart(bare, [1], ep, sizes=[4], obs_counts=[-1])[0] == 0
    restart_all(twin, [1], [ep], sizes='own')
    for t in range(3):
        step_all(S, bare, twin)
        same(everything(twin), everything(bare), ('keep without slots', t))
    bare.set_scenes(None)
    o, c = np.array([0, 5, 9], np.int32), np.array([3, 2], np.int32)
    rc = bare.L.sca_set_scene_obstacle_slots(bare.ctx, 2, _lib.ptr(o, C.c_int32), _lib.ptr(c, C.c_int32), _lib.ptr(pos, C.c_double), _lib.ptr(rad, C.c_double))
    assert rc == ERR_STATE and 'sca_set_scenes' in bare.L.sca_last_error(bare.ctx).decode()
    bare.close(); twin.close()


def test_lifetime_of_the_slots(S):
    """all slots empty keeps the forest forms and walks nothing; sca_set_scene_obstacles and sca_set_obstacles replace the slots; whatever
    redefines the scenes drops them"""
    eps = [circle_scene(S, 6, MIX, rad=4.0), circle_scene(S, 4, MIX[:4], rad=3.0)]
    sol, off = context(S, eps, obs_slots=[5, 4])                          # every slot empty
    free = [alone(S, e) for e in eps]
    step_all(S, sol, *free, k=6)
    assert sol.pass_forms() & S.FORM_SCENE_OBSTACLES and not free[0].pass_forms() & S.FORM_SCENE_OBSTACLES
    assert sol.scene_obstacle_counts()['counts'].tolist() == [0, 0]
    assert_slots_equal_alone(sol, off, dict(enumerate(eps)), dict(enumerate(free)), ('empty slots',), obs_lo={0: 0, 1: 5})
    sol.set_scene_obstacles([spheres(41, 2), spheres(42, 3)])
    oc = sol.scene_obstacle_counts()
    assert oc['counts'].tolist() == [2, 3] and oc['capacities'].tolist() == [2, 3]     # replaced: the ranges are the sets' own again
    sol.set_obstacles(*spheres(43, 4))
    with pytest.raises(S.ScaError):
        sol.scene_obstacle_counts()
    sol.set_scene_obstacle_slots([5, 4], [spheres(41, 2), None])
    assert sol.scene_obstacle_counts()['counts'].tolist() == [2, 0]
    sol.set_scenes(off)
    with pytest.raises(S.ScaError):
        sol.scene_obstacle_counts()
    for x in [sol] + free:
        x.close()


# ---- 12: Python ------------------------------------------------------------------------------------------------------------------------------
def _obstacles(pos, radius):
    from sca_amd import env as E
    return [E.Obstacle(pos=list(map(float, p)), shape_dict={'shape': 'sphere', 'feature': float(r)}, id=i) for i, (p, r) in enumerate(zip(pos, radius))]


def _queue():
    """nine 16-agent episodes: the open circle, the take-off field with its 8 spheres, random scenes among 1-5 spheres; SCA, ORCA3D and
    RVO3D in turn.  (specs: built anew for every run, Agent objects carry state)"""
    from sca_amd import env as E, scenarios
    specs = []
    for k in range(9):
        policy = (E.SCAPolicy, E.ORCA3DPolicy, E.RVO3DPolicy)[k % 3]
        if k % 4 == 0:
            sc, obs = scenarios.circle(16, rad=6.0 + k), ([], [])
        elif k % 4 == 1:
            sc = scenarios.takeoff_landing(16)
            obs = (sc['obs_pos'], sc['obs_radius'])
        else:
            sc = scenarios.random_cube(16, seed=k)
            rng = np.random.default_rng(50 + k)
            lo, hi = sc['start'][:, :3].min(0), sc['start'][:, :3].max(0)
            ends = np.concatenate([sc['start'][:, :3], sc['goal'][:, :3]])
            pts = []
            while len(pts) < 1 + k % 5:
                p = np.round(rng.uniform(lo, hi), 2)
                if np.linalg.norm(ends - p, axis=1).min() > 2.5:
                    pts.append(p)
            obs = (pts, [1.0] * len(pts))
        specs.append((sc, policy, obs))
    return specs


@pytest.fixture(scope='module')
def queue_alone():
    """every episode of the queue as a MACAEnv of its own, to its end: metrics, steps, final state -- computed once"""
    from sca_amd import env as E, metrics
    out = []
    for sc, policy, obs in _queue():
        env = E.MACAEnv(device_tracker=True)
        env.set_agents(agents_of(sc, policy), obstacles=_obstacles(*obs))
        steps = 1
        while not env.step({}) and steps < 4000:
            steps += 1
        assert steps < 4000
        out.append(dict(metrics=metrics.episode_metrics(env), steps=steps, state={k: getattr(env, k).copy() for k in ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num')}))
        env.solver.close()
    return out


@pytest.mark.parametrize('harvest', [False, True])
def test_run_episodes_with_episode_obstacles(queue_alone, harvest):
    from sca_amd.scenes import run_episodes
    specs = _queue()
    assert sorted({len(o[1]) for _, _, o in specs}) == [0, 2, 3, 4, 8]
    done, stats = [], {}
    results = run_episodes([agents_of(sc, p) for sc, p, _ in specs], 3, device_tracker=True, episode_obstacles=[_obstacles(*o) for _, _, o in specs],
                           obstacle_capacities='max', harvest=harvest, on_done=lambda r: done.append(r['episode']), stats=stats, max_steps=12000)
    assert sorted(done) == list(range(9)) and stats['batch_steps'] > 0
    for i, (r, want) in enumerate(zip(results, queue_alone)):
        assert r is not None and r['steps'] == want['steps'], (i, r and r['steps'], want['steps'])
        for key in want['state']:
            assert np.array_equal(r['state'][key], want['state'][key]), (i, key)
        for key in want['metrics']:
            if key != 'AverageCost':                                # a wall time
                a, b = r['metrics'][key], want['metrics'][key]
                assert a == b or (a != a and b != b), (i, key, a, b)
    with pytest.raises(ValueError):
        run_episodes([agents_of(sc, p) for sc, p, _ in specs], 3, _obstacles([[0, 0, 5]], [1.0]), episode_obstacles=[[] for _ in specs])
    with pytest.raises(ValueError, match='fits no slot'):
        run_episodes([agents_of(sc, p) for sc, p, _ in specs], 3, episode_obstacles=[_obstacles(*o) for _, _, o in specs], obstacle_capacities=[4, 4, 4])


def test_scene_batch_restart_with_obstacles(tmp_path):
    """SceneBatch(obstacle_capacities=...): restart's ValueErrors come before any device call (the state is unchanged); a refilled slot's
    view and its episode log list the new obstacles"""
    from sca_amd import env as E, metrics
    from sca_amd.scenes import SceneBatch
    specs = _queue()
    (sc0, p0, o0), (sc1, p1, o1), (sc2, p2, o2) = specs[1], specs[2], specs[3]         # 8, 3 and 4 obstacles
    batch = SceneBatch([agents_of(sc0, p0), agents_of(sc1, p1)], scene_obstacles=[_obstacles(*o0), _obstacles(*o1)], obstacle_capacities=[8, 4], device_tracker=True,
                       scene_history=8)
    plain = SceneBatch([agents_of(sc0, p0), agents_of(sc1, p1)], scene_obstacles=[_obstacles(*o0), _obstacles(*o1)], device_tracker=True)
    for _ in range(3):
        batch.step()
        plain.step()
    before = {k: v.copy() for k, v in batch.solver.get_state().items()}
    with pytest.raises(ValueError, match='holds up to 4 obstacles'):
        batch.restart({1: agents_of(sc0, p1)}, obstacles={1: _obstacles(*o0)})
    with pytest.raises(ValueError, match='not restarted'):
        batch.restart({1: agents_of(sc2, p1)}, obstacles={0: _obstacles(*o2)})
    with pytest.raises(ValueError, match='without obstacle slots'):
        plain.restart({1: agents_of(sc2, p1)}, obstacles={1: _obstacles(*o2)})
    for b_, want in ((batch, before), (plain, before)):
        st = b_.solver.get_state()
        for k in want:
            assert np.array_equal(st[k], want[k]), k
        assert len(b_.env(1).obstacles) == 3
    assert batch.solver.scene_obstacle_counts()['counts'].tolist() == [8, 3]
    new = _obstacles(*o2)
    batch.restart({1: agents_of(sc2, p1)}, obstacles={1: new})
    assert batch.solver.scene_obstacle_counts()['counts'].tolist() == [8, 4] and batch.env(1).obstacles == new and batch.env(1)._obs_lo == 8
    env = E.MACAEnv(device_tracker=True)
    env.set_agents(agents_of(sc2, p1), obstacles=_obstacles(*o2))
    for t in range(6):
        batch.step()
        env.step({})
        for a, b_ in zip(batch.env(1).agents, env.agents):
            assert [(type(o), d) for o, d in a.neighbors] == [(type(o), d) for o, d in b_.neighbors], (t, a.id)
            for (oa, _), (ob, _) in zip(a.neighbors, b_.neighbors):
                if isinstance(oa, E.Obstacle):
                    assert oa is new[oa.id] and oa.id == ob.id
    for key in ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num'):
        assert np.array_equal(getattr(batch.env(1), key), getattr(env, key)), key
    paths = metrics.write_episode_log(batch.env(1), str(tmp_path / 'refilled'), xlsx=False)
    listed = json.load(open(paths['env_cfg']))['all_obstacle']
    assert [o['position'] for o in listed] == [list(o.pos) for o in new] and len(listed) == 4
    batch.restart({1: agents_of(sc1, p1)})                             # absent from `obstacles`: the slot keeps its list
    assert batch.env(1).obstacles == new and batch.solver.scene_obstacle_counts()['counts'].tolist() == [8, 4]
    env.solver.close(); batch.close(); plain.close()


# ---- 13: one kernel behind the three entry points -----------------------------------------------------------------------------------------------
def test_one_kernel_behind_the_three_entry_points(S):
    """k_scene_restart serves sca_restart_scenes, sca_restart_scenes_sized and sca_restart_scenes_obstacles alike.  The same restart of
    scene 1 of three 12-agent circles (the six policies, the tracker on) through each of them -- sizes = the capacity, obs_counts = [-1] --
    on a context without any obstacle arrays and on one whose obstacle slots of capacity 4 hold 3 spheres each.  Behind each of 5 steps
    the slot is a fresh context of the new episode alone with the slot's set, every value of everything(), and on the slots context its
    lists hold obstacles of its own set.  Directly behind the call it is that context in what a restart resets (include/sca_hip.h: state,
    permutation, empty neighbour lists, tracker records and re-plan counts, counters) -- action rows, list entries and diagnostics are the
    last pass's output until the next pass, and a fresh context has had none.  Scenes 0 and 2 are those of a twin batch that was never
    restarted, at the call and at every step, and the obstacle counts stay."""
    mix = np.resize(MIX, 12)
    first, new = circle_scene(S, 12, mix, rad=4.0), circle_scene(S, 12, mix[::-1], rad=4.0, turn=2)
    sets = [spheres(50 + s, 3) for s in range(3)]
    ways = dict(plain={}, sized=dict(sizes=[12]), keep=dict(sizes=[12], obstacles=[None]))
    for where, kw in (('no obstacles', {}), ('slots', dict(obstacles=sets, obs_slots=[4] * 3))):
        for way, how in ways.items():
            sol, off = context(S, [first] * 3, **kw)
            twin = context(S, [first] * 3, **kw)[0]
            solo = alone(S, new, sets[1] if kw else NO_OBSTACLES)
            step_all(S, sol, twin, k=5)
            restart_all(sol, [1], [new], **how)
            others = [int(off[s]) + a for s in (0, 2) for a in tracked(first)]
            saw_obstacle = False
            for t in range(6):
                ctx = (where, way, 'step', t)
                if t:
                    step_all(S, sol, twin, solo)
                    got = assert_slots_equal_alone(sol, off, {1: new}, {1: solo}, ctx, obs_lo={1: 4 if kw else 0})
                    listed = got['nbr_id'][12:24][got['nbr_kind'][12:24] == 1]
                    assert ((listed >= 4) & (listed < 7)).all(), ctx + ('an obstacle id outside the slot\'s set',)
                    saw_obstacle = saw_obstacle or len(listed) > 0
                else:
                    got = dict(sol.get_state(), perm=sol.get_kd_perm() - 12, nbr_n=sol.neighbors()['nbr_n'], replans=sol.device_tracker_replans())
                    want = dict(solo.get_state(), perm=solo.get_kd_perm(), nbr_n=solo.neighbors()['nbr_n'], replans=solo.device_tracker_replans())
                    for key in want:
                        assert np.array_equal(got[key][12:24], want[key]), ctx + ('behind the call', key)
                    for a in tracked(new):
                        assert np.array_equal(sol.device_tracker_debug(12 + int(a)), solo.device_tracker_debug(int(a)), equal_nan=True), ctx + ('behind the call', 'tracker record', a)
                ea, eb = everything(sol, others), everything(twin, others)
                for s in (0, 2):
                    sl = slice(int(off[s]), int(off[s + 1]))
                    for key in ea:
                        if key == 'track':
                            for i in ea[key]:
                                assert np.array_equal(ea[key][i], eb[key][i], equal_nan=True), ctx + ('scene', s, key, i)
                        else:
                            assert np.array_equal(ea[key][sl], eb[key][sl], equal_nan=True), ctx + ('scene', s, key)
                if kw:
                    assert sol.scene_obstacle_counts()['counts'].tolist() == [3, 3, 3], ctx
                assert sol.scene_state()['steps'].tolist() == [5 + t, t, 5 + t] and sol.scene_sizes().tolist() == [12, 12, 12], ctx
            assert saw_obstacle == bool(kw), (where, way, 'an obstacle of the slot\'s own set in a list of the restarted scene')
            for x in (sol, twin, solo):
                x.close()
