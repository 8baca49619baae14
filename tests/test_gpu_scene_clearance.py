"""Closest approach per agent, measured with the step (-m gpu): sca_scene_clearance_enable / sca_get_scene_clearance and what is built on
them.  Expected records come from the rule restated in Python (tests/clearance_rule.py: round(math.sqrt(...), 5) per pair) over positions
the kernel under test did not produce -- the reference's recordings, or the state read back around a step -- and from the contract: a
scene's records are bit for bit those of a context holding that episode alone, in every step form.  Every comparison is equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import clearance_rule as R
from scene_util import NO_OBSTACLES, circle_scene, context, everything, partial_batch, rc_of, restart_all, same, step_all

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3                                        # include/sca_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDED = ['F2_orcalp_circle100', 'F4_sca_takeoff16', 'F16_params_timestep02', 'F14_fuzz_episode_02', 'F9_hetero_mixed60', 'F10_sca_exp3_map',
            'F1_sca_circle8']
MIX = [0, 1, 2, 3, 4, 5]


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


def scene(S, start, goal, policy=1):
    """agents from start to goal positions ([n, 3] each, headings along the way), the arrays sca_set_agents / sca_restart_scenes take"""
    from sca_amd import scenarios
    start, goal = np.asarray(start, float).reshape(-1, 3), np.asarray(goal, float).reshape(-1, 3)
    n = len(start)
    yaw = np.arctan2(goal[:, 1] - start[:, 1], goal[:, 0] - start[:, 0])
    start6 = np.hstack([start, yaw[:, None], np.zeros((n, 2))])
    goal6 = np.hstack([goal, yaw[:, None], np.zeros((n, 2))])
    return dict(n=n, pos=start, heading=start6[:, 3:6], vel=np.zeros((n, 3), np.float32), radius=np.full(n, 0.5), pref_speed=np.ones(n), goal=goal,
                policy=np.resize(np.asarray(policy, np.uint8), n), zaxis=S.zaxis_flags(start6, goal6), max_run_dist=scenarios.max_run_dist(start6, goal6),
                goal_heading=goal6[:, 3:6])


def tight_circle(S, n, turn=0, policy=MIX):
    """n drones on a circle about 1.3 m apart (two: 3.8 m): neighbours within a few tenths of a metre from the first steps on"""
    return circle_scene(S, n, np.resize(np.asarray(policy, np.uint8), n), rad=0.2 * n + 1.5, turn=turn)


def crossing(S, n, y=0.0, policy=1):
    """n drones on a line along x, 2 m apart, each bound for the mirror image of its start about (0, y, 10) (off centre by 0.3 m: nobody
    starts at its goal)"""
    x = 2.0 * (np.arange(n) - (n - 1) / 2) + 0.3
    start = np.stack([x, np.full(n, y), np.full(n, 10.0)], 1)
    return scene(S, start, start * [-1, 1, 1], policy)


def records(sol, scenes):
    return [sol.scene_clearance(s) for s in scenes]


class Follower:
    """The Python rule beside a context: step() reads the state in front of and behind ONE step of the batch and applies the rule to every
    scene that began the step with somebody live -- entry flags from the state before, moved positions from the state after, the scene's
    step count kept here."""

    def __init__(self, sol, off, radius, obstacles):
        self.sol, self.off, self.radius = sol, off, np.asarray(radius, float)
        self.B = len(off) - 1
        self.obstacles = list(obstacles)                           # per scene (pos, radius)
        self.steps = [0] * self.B
        self.want = [R.empty(int(n)) for n in sol.scene_sizes()]

    def restarted(self, s, obstacles=None):
        self.steps[s], self.want[s] = 0, R.empty(int(self.sol.scene_sizes()[s]))
        if obstacles is not None:
            self.obstacles[s] = obstacles

    def step(self, step_fn):
        before, sizes = self.sol.get_state(), self.sol.scene_sizes()
        step_fn(self.sol)
        after = self.sol.get_state()
        for s in range(self.B):
            occ = slice(int(self.off[s]), int(self.off[s]) + int(sizes[s]))
            if ((before['flags'][occ] & 7) == 0).any():
                self.steps[s] += 1
                R.step(self.want[s], after['pos'][occ], self.radius[occ], before['flags'][occ], *self.obstacles[s], self.steps[s])

    def check(self, ctx):
        for s in range(self.B):
            got = self.sol.scene_clearance(s)
            assert np.array_equal(got, self.want[s]), ctx + ('scene', s, np.flatnonzero(got != self.want[s]).tolist())


def one_step(S):
    return lambda x: (x.run_steps(1, S.NBR_KDTREE), x.synchronize())


# ---- the reference's recordings ----------------------------------------------------------------------------------------------------------------
def test_recordings_as_one_free_running_batch(S):
    """the corpus of tests/test_scene_clearance_cpu.py as one batch, every scene with its own recorded obstacles and attributes, free-running
    from the start states: the records against the Python rule over the RECORDED positions -- after every step for the scenes of at most
    24 agents, at three steps and at their last record for the larger ones (the positions the batch is at are checked against the records
    at those steps too).  F1 finishes at its step 246 and keeps its records to the end."""
    from test_gpu_scene_obstacles import ObsBatch
    b = ObsBatch(S, RECORDED)
    sol = b.sol
    sol.scene_clearance_enable()
    fx = b.fx
    want = [R.empty(len(f['radius'])) for f in fx]
    rows = [len(f['step']) for f in fx]
    at = [set(range(k)) if len(f['radius']) <= 24 else {0, k // 3, 2 * k // 3, k - 1} for f, k in zip(fx, rows)]
    compared = 0
    for t in range(max(rows)):
        sol.run_steps(1, S.NBR_KDTREE)
        sol.synchronize()
        pos = None
        for s, f in enumerate(fx):
            if t >= rows[s]:
                continue
            R.step(want[s], f['pos_after'][t], f['radius'], f['flags'][t], f['obs_pos'], f['obs_radius'], t + 1)
            if t in at[s]:
                pos = sol.get_state()['pos'] if pos is None else pos
                assert np.array_equal(pos[b.sl(s)], f['pos_after'][t]), (RECORDED[s], t, 'the batch left its recording')
                got = sol.scene_clearance(s)
                assert np.array_equal(got, want[s]), (RECORDED[s], 'step', t + 1, np.flatnonzero(got != want[s]).tolist())
                compared += 1
    assert compared == 285 + 20 + 160 + 246 + 3 * 4
    s = RECORDED.index('F1_sca_circle8')
    assert rows[s] == 246 and sol.scene_state()['active'][s] == 0 and sol.scene_state()['steps'][s] == 246
    assert np.array_equal(sol.scene_clearance(s), want[s])
    assert len(fx[RECORDED.index('F10_sca_exp3_map')]['obs_radius']) == 1491       # (twelve tiles of the kernel's obstacle stream)
    sol.close()


# ---- sizes -------------------------------------------------------------------------------------------------------------------------------------
def test_sizes_in_slots_of_130(S):
    """slots of 130 rows holding 1, 2, 63, 64, 65 and 129 agents (the spare rows are copies of the last agent, vacated): every scene's
    records equal those of a context of that episode alone at every step; the one-agent scene stays empty; no record names a vacant row"""
    sizes = [1, 2, 63, 64, 65, 129]
    eps = [tight_circle(S, n, turn=k) for k, n in enumerate(sizes)]
    sol, off = partial_batch(S, eps, 130)
    sol.scene_clearance_enable()
    solos = [context(S, [e])[0] for e in eps]
    for x in solos:
        x.scene_clearance_enable()
    for t in range(8):
        step_all(S, sol, *solos)
        for s, n in enumerate(sizes):
            got, alone = sol.scene_clearance(s), solos[s].scene_clearance(0)
            assert len(got) == n and np.array_equal(got, alone), (t, 'slot', s, np.flatnonzero(got != alone).tolist())
            assert (got['agent_partner'] < n).all() and (got['obs_partner'] == -1).all(), (t, s)
    assert np.array_equal(sol.scene_clearance(0), R.empty(1))
    for s, n in enumerate(sizes[1:], 1):
        got = sol.scene_clearance(s)
        assert (got['agent_partner'] >= 0).all() and (got['agent_step'] >= 1).all() and np.isfinite(got['agent_clear']).all(), s
        assert got['agent_clear'][n - 1] > -1.0                    # (the last agent against a copy of itself would be 0 - 2 r)
    for x in [sol] + solos:
        x.close()


# ---- obstacle forms ----------------------------------------------------------------------------------------------------------------------------
def _spheres(*rows):
    a = np.asarray(rows, float).reshape(-1, 4)
    return a[:, :3].copy(), a[:, 3].copy()


def test_obstacle_forms(S):
    """the shared set, one set per scene, an obstacle slot that holds fewer spheres than the set it held before -- with a sphere of the old
    set on the agents' line --, and a slot that holds none: the records against the Python rule over the state read back around every step"""
    eps = [crossing(S, 6, y=0.0), crossing(S, 5, y=40.0), tight_circle(S, 9)]
    cat = lambda key: np.concatenate([e[key] for e in eps])
    on_line = _spheres([0.0, 1.2, 10.0, 0.6], [0.0, 38.5, 10.0, 0.7], [3.0, -1.5, 10.5, 0.4])
    # one set for all scenes
    sol, off = context(S, eps, shared=on_line, tracker=False)
    sol.scene_clearance_enable()
    f = Follower(sol, off, cat('radius'), [on_line] * 3)
    for t in range(6):
        f.step(one_step(S))
        f.check(('shared', t))
    assert (sol.scene_clearance(0)['obs_partner'] >= 0).all() and sol.scene_clearance(0)['obs_clear'].min() < 1.0
    sol.close()
    # one set per scene: a scene meets its own and no other's; scene 2 has none
    sets = [_spheres([0.0, 1.2, 10.0, 0.6], [50.0, 0.0, 10.0, 1.0]), _spheres([0.0, 38.5, 10.0, 0.7]), NO_OBSTACLES]
    sol, off = context(S, eps, obstacles=sets, tracker=False)
    sol.scene_clearance_enable()
    f = Follower(sol, off, cat('radius'), sets)
    for t in range(6):
        f.step(one_step(S))
        f.check(('per scene', t))
    assert np.isinf(sol.scene_clearance(2)['obs_clear']).all() and (sol.scene_clearance(2)['obs_partner'] == -1).all()
    assert set(sol.scene_clearance(1)['obs_partner'].tolist()) == {0}
    sol.close()
    # obstacle slots of four rows: scene 0 holds three spheres, the third on the agents' line; a restart brings ONE sphere far away (rows 1
    # and 2 of the slot keep the old set's records), then none at all
    held = [_spheres([30.0, 0.0, 10.0, 1.0], [40.0, 0.0, 10.0, 1.0], [0.0, 0.6, 10.0, 0.6]), _spheres([0.0, 38.5, 10.0, 0.7]), NO_OBSTACLES]
    sol, off = context(S, eps, obstacles=held, obs_slots=[4, 4, 4], tracker=False)
    sol.scene_clearance_enable()
    f = Follower(sol, off, cat('radius'), held)
    for t in range(3):
        f.step(one_step(S))
        f.check(('slots', t))
    assert 2 in sol.scene_clearance(0)['obs_partner']
    far = _spheres([0.0, 25.0, 10.0, 1.0])
    restart_all(sol, [0], [eps[0]], obstacles=[far], tracker=False)
    f.restarted(0, far)
    assert np.array_equal(sol.scene_clearance(0), R.empty(6))
    for t in range(5):
        f.step(one_step(S))
        f.check(('fewer spheres', t))
    got = sol.scene_clearance(0)
    assert (got['obs_partner'] == 0).all() and got['obs_clear'].min() > 20.0          # (the old sphere on the line would be within 1 m)
    restart_all(sol, [0, 1], [eps[0], eps[1]], obstacles=[NO_OBSTACLES, None], tracker=False)
    f.restarted(0, NO_OBSTACLES)
    f.restarted(1)
    for t in range(4):
        f.step(one_step(S))
        f.check(('no spheres', t))
    assert np.isinf(sol.scene_clearance(0)['obs_clear']).all() and (sol.scene_clearance(0)['obs_step'] == 0).all()
    assert (sol.scene_clearance(1)['obs_partner'] == 0).all()      # (scene 1 kept its set through its restart)
    sol.close()


# ---- finished agents and finished scenes -------------------------------------------------------------------------------------------------------
def test_a_finished_agent_stays_a_partner(S):
    """agent 0 arrives in the first step and stands still; agent 1 passes it a metre away twenty steps later, agent 2 flies far off.  Agent
    0's record stops at its arrival, agent 1's goes on naming it."""
    e = scene(S, [[0.0, 0.0, 10.0], [-3.0, 1.1, 10.0], [0.0, 60.0, 10.0]], [[0.3, 0.0, 10.0], [5.0, 1.1, 10.0], [9.0, 60.0, 10.0]])
    sol, off = context(S, [e], tracker=False)
    sol.scene_clearance_enable()
    f = Follower(sol, off, e['radius'], [NO_OBSTACLES])
    f.step(one_step(S))
    f.check(('first step',))
    assert sol.get_state()['flags'][0] & 1
    arrived = sol.scene_clearance(0)[0].copy()
    assert arrived['agent_step'] == 1 and arrived['agent_partner'] == 1
    for t in range(40):
        f.step(one_step(S))
        f.check(('step', t + 2))
    got = sol.scene_clearance(0)
    assert got[0] == arrived
    assert got['agent_partner'][1] == 0 and got['agent_step'][1] > 20 and got['agent_clear'][1] < arrived['agent_clear']
    sol.close()


def test_a_finished_scene_keeps_its_records(S):
    """scene 0's agents are all at their goals after a few steps: its records stay bit for bit while scene 1 runs on, and until a restart"""
    done_soon = scene(S, [[0.0, 0.0, 10.0], [1.5, 0.0, 10.0], [0.0, 1.4, 10.0]], [[0.6, 0.0, 10.0], [2.1, 0.0, 10.0], [0.0, 2.0, 10.0]])
    eps = [done_soon, tight_circle(S, 12)]
    sol, off = context(S, eps, tracker=False)
    sol.scene_clearance_enable()
    f = Follower(sol, off, np.concatenate([e['radius'] for e in eps]), [NO_OBSTACLES] * 2)
    for t in range(20):
        f.step(one_step(S))
        f.check(('step', t))
        if sol.scene_state()['active'][0] == 0:
            break
    st = sol.scene_state()
    assert st['active'][0] == 0 and st['steps'][0] == t + 1 and st['active'][1] > 0
    kept = sol.scene_clearance(0)
    assert (kept['agent_step'] >= 1).all() and (kept['agent_step'] <= st['steps'][0]).all()
    for t in range(6):
        f.step(one_step(S))
        assert sol.scene_clearance(0).tobytes() == kept.tobytes(), t
    f.check(('end',))
    sol.close()


# ---- step forms --------------------------------------------------------------------------------------------------------------------------------
def test_step_forms_leave_identical_records(S):
    eps = [crossing(S, 6, policy=MIX), tight_circle(S, 20), crossing(S, 3, y=40.0)]
    sets = [_spheres([0.0, 1.2, 10.0, 0.6]), NO_OBSTACLES, _spheres([0.0, 38.5, 10.0, 0.7], [9.0, 40.0, 10.0, 0.5])]
    forms = dict(env_step=lambda x: [x.env_step(S.NBR_KDTREE) for _ in range(6)],
                 run_steps_1=lambda x: [(x.run_steps(1, S.NBR_KDTREE), x.synchronize()) for _ in range(6)],
                 run_steps_3=lambda x: [(x.run_steps(3, S.NBR_KDTREE), x.synchronize()) for _ in range(2)],
                 split=lambda x: [(x.policy_pass(S.NBR_KDTREE), x.env_update()) for _ in range(6)],
                 step_host=lambda x: [x.step_host(S.NBR_KDTREE, state=False) for _ in range(6)])
    got = {}
    for name, run in forms.items():
        sol, off = context(S, eps, obstacles=sets)
        sol.scene_clearance_enable()
        if name == 'step_host':
            sol.host_state()
        if name == 'env_step':                                     # ... and this one against the rule, step by step
            f = Follower(sol, off, np.concatenate([e['radius'] for e in eps]), sets)
            for t in range(6):
                f.step(lambda x: x.env_step(S.NBR_KDTREE))
                f.check((name, t))
        else:
            run(sol)
        assert sol.scene_state()['steps'].tolist() == [6, 6, 6], name
        got[name] = records(sol, range(3))
        sol.close()
    for name, recs in got.items():
        for s in range(3):
            assert np.array_equal(recs[s], got['env_step'][s]), (name, 'scene', s)
    assert np.isfinite(got['env_step'][0]['obs_clear']).all() and np.isinf(got['env_step'][1]['obs_clear']).all()


# ---- restart in flight, non-interference -------------------------------------------------------------------------------------------------------
def test_restart_in_flight(S):
    """four slots of 12 rows; behind five steps slot 1 takes a new episode of 12 (sca_restart_scenes) and slot 3 one of 7
    (sca_restart_scenes_sized): the named slots start empty and from there equal the episode alone, the others equal a twin batch that
    was never restarted"""
    eps = [tight_circle(S, 12, turn=k) for k in range(4)]
    new = {1: crossing(S, 12, policy=MIX), 3: tight_circle(S, 7, turn=2)}
    sol, off = context(S, eps)
    twin, _ = context(S, eps)
    for x in (sol, twin):
        x.scene_clearance_enable()
    step_all(S, sol, twin, k=5)
    for s in range(4):
        assert np.array_equal(sol.scene_clearance(s), twin.scene_clearance(s)), s
    restart_all(sol, [1], [new[1]])
    restart_all(sol, [3], [new[3]], sizes='own')
    solos = {s: context(S, [e])[0] for s, e in new.items()}
    for x in solos.values():
        x.scene_clearance_enable()
    for s, e in new.items():
        assert np.array_equal(sol.scene_clearance(s), R.empty(e['n'])), s
    for t in range(6):
        step_all(S, sol, twin, *solos.values())
        for s in (0, 2):
            assert np.array_equal(sol.scene_clearance(s), twin.scene_clearance(s)), (t, 'unnamed', s)
        for s, x in solos.items():
            got, alone = sol.scene_clearance(s), x.scene_clearance(0)
            assert np.array_equal(got, alone), (t, 'named', s, np.flatnonzero(got != alone).tolist())
            assert (got['agent_step'] <= t + 1).all() and (got['agent_step'] >= 1).all()
    for x in [sol, twin] + list(solos.values()):
        x.close()


def test_the_feature_changes_nothing_else(S):
    """a batch with the feature on and a twin with it off agree in everything scene_util.everything reads, through steps, a restart and the
    feature's own off and on"""
    eps = [crossing(S, 6, policy=MIX), tight_circle(S, 20), tight_circle(S, 5, turn=1)]
    on, off_ = context(S, eps)
    plain, _ = context(S, eps)
    on.scene_clearance_enable()
    tracked = [int(i) for i in np.flatnonzero(np.isin(np.concatenate([e['policy'] for e in eps]), (0, 5)))]
    for t in range(4):
        step_all(S, on, plain)
        same(everything(on, tracked), everything(plain, tracked), ('step', t))
    for x in (on, plain):
        restart_all(x, [2], [tight_circle(S, 5, turn=3)])
    on.scene_clearance_enable(False)
    step_all(S, on, plain)
    assert rc_of(S, lambda: on.scene_clearance(0)) == ERR_STATE
    on.scene_clearance_enable()
    assert np.array_equal(on.scene_clearance(1), R.empty(20))      # records cover the steps from the call on
    for t in range(3):
        step_all(S, on, plain)
        same(everything(on, tracked), everything(plain, tracked), ('behind the restart', t))
    assert np.array_equal(on.scene_state()['steps'], plain.scene_state()['steps'])
    assert (on.scene_clearance(1)['agent_step'] >= 6).all()        # (the scene's own step count, not steps since the call)
    on.close()
    plain.close()


# ---- checkpoints -------------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_resumed_in_another_context_and_slot(S):
    """scene 1 of a source batch saved behind its step 4 and resumed in slot 0 of another context: merge(the record at the save, the
    resumed slot's record) equals the uninterrupted source at every later step -- sca_load_scenes leaves the records alone"""
    from sca_amd import metrics
    ep = crossing(S, 7, policy=MIX)
    src, _ = context(S, [tight_circle(S, 5), ep])
    src.scene_clearance_enable()
    step_all(S, src, k=4)
    blob, saved = src.save_scenes([1])[0], src.scene_clearance(1)
    assert np.isfinite(saved['agent_clear']).all()
    dst, _ = context(S, [tight_circle(S, 7, turn=1), tight_circle(S, 9), tight_circle(S, 3)])
    dst.scene_clearance_enable()
    step_all(S, dst, k=2)
    other = dst.scene_clearance(1)
    restart_all(dst, [0], [ep])
    dst.load_scenes([0], [blob])
    assert np.array_equal(dst.scene_clearance(0), R.empty(7)) and np.array_equal(dst.scene_clearance(1), other)
    for t in range(8):
        step_all(S, src, dst)
        merged = metrics.merge_clearance(saved, dst.scene_clearance(0))
        assert np.array_equal(merged, src.scene_clearance(1)), (t, np.flatnonzero(merged != src.scene_clearance(1)).tolist())
    steps = dst.scene_clearance(0)['agent_step']                   # the resumed scene goes on counting from the source's steps; an agent
    assert ((steps == 0) | (steps >= 5)).all() and (steps >= 5).sum() >= 5            # that had arrived before the save keeps an empty record here
    assert not np.array_equal(src.scene_clearance(1), saved)       # (the later steps did come closer)
    src.close()
    dst.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(S):
    import ctypes as C
    from sca_amd import _lib
    e = tight_circle(S, 6)
    sol = S.BatchedSolver(max_agents=12, max_obstacles=1)
    sol.set_agents(*(np.concatenate([e[k], e[k]]) for k in ('radius', 'pref_speed', 'goal', 'policy', 'zaxis', 'max_run_dist')))
    assert rc_of(S, lambda: sol.scene_clearance_enable()) == ERR_STATE            # no scenes
    assert rc_of(S, lambda: sol.scene_clearance_enable(False)) == ERR_STATE
    sol.set_scenes(np.array([0, 6, 12], np.int32))
    sol.set_state(np.concatenate([e['pos'], e['pos'] + [40.0, 0, 0]]), np.zeros((12, 3), np.float32), np.concatenate([e['heading']] * 2), np.zeros(12, np.uint8))
    assert rc_of(S, lambda: sol.scene_clearance(0)) == ERR_STATE                  # not enabled
    sol.policy_pass(S.NBR_KDTREE)
    assert rc_of(S, lambda: sol.scene_clearance_enable()) == ERR_STATE            # between a policy pass and its env update
    sol.env_update()
    sol.scene_clearance_enable()
    assert np.array_equal(sol.scene_clearance(1), R.empty(6))
    assert rc_of(S, lambda: sol.scene_clearance(-1)) == ERR_ARG and rc_of(S, lambda: sol.scene_clearance(2)) == ERR_ARG
    out = np.zeros(6, _lib.CLEARANCE_DTYPE)
    p = out.ctypes.data_as(C.POINTER(_lib.SceneClearance))
    assert sol.L.sca_get_scene_clearance(sol.ctx, 0, p, 24) == ERR_ARG and sol.L.sca_get_scene_clearance(sol.ctx, 0, p, 40) == ERR_ARG
    assert sol.L.sca_get_scene_clearance(sol.ctx, 0, None, 32) == ERR_ARG
    assert sol.L.sca_get_scene_clearance(sol.ctx, 0, p, 32) == 0 and np.array_equal(out, R.empty(6))
    sol.run_steps(2, S.NBR_KDTREE)
    sol.synchronize()
    assert np.isfinite(sol.scene_clearance(0)['agent_clear']).all()
    sol.set_scenes(np.array([0, 4, 12], np.int32))                  # redefining the scenes drops the records, as it drops the log
    assert rc_of(S, lambda: sol.scene_clearance(0)) == ERR_STATE
    sol.scene_clearance_enable()
    sol.set_scenes(None)                                            # ... and so does clearing them
    assert rc_of(S, lambda: sol.scene_clearance(0)) == ERR_STATE
    sol.close()


# ---- the Python layers -------------------------------------------------------------------------------------------------------------------------
def _agents(E, n, policy, rad):
    return E.build_circle_agents(n, policy=policy, rad=rad)


def test_scene_batch_run_episodes_and_metrics(S, tmp_path):
    from sca_amd import env as E, metrics
    from sca_amd.scenes import SceneBatch, SceneCheckpoint, run_episodes
    lone = lambda: [E.Agent(start_pos=[-3.0, 0.0, 10.0, 0.0, 0.0, 0.0], goal_pos=[3.0, 0.0, 10.0, 0.0, 0.0, 0.0], vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0,
                            policy=E.RVO3DPolicy, id=0)]
    make = lambda: [_agents(E, 6, E.RVO3DPolicy, 3.0), _agents(E, 9, E.ORCA3DPolicy, 4.0), lone(), _agents(E, 6, E.SRVO3DPolicy, 3.5)]
    obstacle = [E.Obstacle(pos=[0.0, 0.0, 11.5], shape_dict={'shape': 'sphere', 'feature': 0.5}, id=0)]
    # a batch run to the end: env(s).clearance is the solver's record, clearance_metrics reads it
    batch = SceneBatch(make(), obstacle, clearance=True)
    plain = SceneBatch(make(), obstacle)
    with pytest.raises(RuntimeError):
        plain.env(0).clearance
    plain.close()
    steps = 0
    while not batch.step() and steps < 2000:
        steps += 1
    assert batch.done.all()
    whole = [batch.env(s).clearance for s in range(4)]
    for s in range(4):
        assert np.array_equal(whole[s], batch.solver.scene_clearance(s)) and whole[s].dtype == R.DTYPE
    rec = whole[1]
    margin = float(np.sort(np.minimum(rec['agent_clear'], rec['obs_clear']))[4])       # the median drone's: five of the nine are near misses at least
    m = metrics.clearance_metrics(batch.env(1), margin=margin)
    a = int(np.argmin(rec['agent_clear']))
    assert m['MinClearance'] == rec['agent_clear'].min() and m['MinClearancePair'] == (a, int(rec['agent_partner'][a])) and m['MinClearanceStep'] == rec['agent_step'][a]
    o = int(np.argmin(rec['obs_clear']))
    assert (m['MinObstacleClearance'], m['MinObstacleClearanceAgent'], m['MinObstacleClearanceObstacle'], m['MinObstacleClearanceStep']) == \
        (rec['obs_clear'].min(), o, 0, rec['obs_step'][o])
    assert m['NearMisses'] == [i for i in range(9) if min(rec['agent_clear'][i], rec['obs_clear'][i]) <= margin] and 5 <= len(m['NearMisses']) <= 9
    assert metrics.clearance_metrics(rec, margin=margin) == m      # the array itself serves as well
    assert metrics.clearance_metrics(rec, margin=float(m['MinClearance']) - 1.0)['NearMisses'] == []
    one = metrics.clearance_metrics(batch.env(2))
    assert one['MinClearance'] == np.inf and one['MinClearancePair'] is None and one['MinClearanceStep'] == 0 and np.isfinite(one['MinObstacleClearance'])
    batch.close()
    # the same episodes as a queue through two capacity slots, the harvest on and off: every result carries its episode's record
    for harvest in (False, True):
        results = run_episodes(make(), 2, obstacles=obstacle, capacities='max', harvest=harvest, clearance=True, max_steps=2000)
        for i, r in enumerate(results):
            assert np.array_equal(r['clearance'], whole[i]), (harvest, i)
    assert 'clearance' not in run_episodes(make()[:1], 1, obstacles=obstacle, max_steps=2000)[0]
    # a checkpoint carries the record so far; resumed in another slot, env(s).clearance is the merge: the uninterrupted episode's
    src = SceneBatch(make(), obstacle, clearance=True)
    for _ in range(5):
        src.step()
    ck = src.checkpoint(1)
    assert np.array_equal(ck.clearance, src.env(1).clearance)
    back = SceneCheckpoint.read(ck.write(str(tmp_path / 'ck.npz')))
    assert back.clearance.dtype == R.DTYPE and np.array_equal(back.clearance, ck.clearance)
    old = SceneCheckpoint(ck.definition, ck.blob, ck.steps)        # a file written without the record still reads
    assert SceneCheckpoint.read(old.write(str(tmp_path / 'old.npz'))).clearance is None
    dst = SceneBatch([_agents(E, 9, E.RVO3DPolicy, 6.0), _agents(E, 4, E.RVO3DPolicy, 3.0)], obstacle, clearance=True)
    dst.step()
    dst.restart({0: back})
    assert np.array_equal(dst.env(0).clearance, ck.clearance)
    for t in range(6):
        src.step()
        dst.step()
        assert np.array_equal(dst.env(0).clearance, src.env(1).clearance), t
    src.close()
    dst.close()


def test_the_example_prints_the_columns():
    """examples/run_scenes.py --clearance as a child process: every row carries the two minima and the near-miss count"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'run_scenes.py'), '--agents', '6', '--seeds', '1', '--max-steps', '25', '--clearance',
                        '--margin', '0.3'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln for ln in r.stdout.splitlines() if 'SuccessRate' in ln]
    assert len(rows) == 12 and all('MinClearance ' in ln and 'MinObstacleClearance inf' in ln and 'NearMisses ' in ln for ln in rows), r.stdout
