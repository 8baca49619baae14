"""SceneBatch.restart and scenes.run_episodes (-m gpu): a queue of episodes streamed through a few slots against the same queue run in waves
of fresh SceneBatches -- the only way there was.  Per episode the metrics rows (the wall-time column left out), the step counts and the final
states must be equal: a slot that is refilled in the middle of a batch is, from there on, the episode alone."""
import numpy as np
import pytest

from scene_util import agents_of

pytestmark = pytest.mark.gpu

WALL = ('AverageCost',)                                             # wall time of the policy calls: differs from run to run


@pytest.fixture(scope='module')
def mods():
    from sca_amd import env as E, metrics, scenarios, scenes
    return E, metrics, scenarios, scenes


def _queue(E, scenarios):
    """14 episodes: the take-off/landing scene and a circle of 16 for each of the six policies, and two circles of 14 at the end; all among
    the take-off field's 8 spheres.  A fresh list of Agent objects at every call."""
    pols = [E.SCAPolicy, E.RVO3DPolicy, E.SRVO3DPolicy, E.ORCA3DPolicy, E.ORCA3DPolicyOfficial, E.RVO3dDubinsPolicy]
    take, circ, c14 = scenarios.takeoff_landing(16), scenarios.circle(16, rad=6.0, z=12.0), scenarios.circle(14, rad=5.0, z=12.0)
    eps = []
    for p in pols:
        eps += [agents_of(take, p), agents_of(circ, p)]
    eps += [agents_of(c14, E.SCAPolicy), agents_of(c14, E.ORCA3DPolicy)]
    obstacles = [E.Obstacle(pos=list(p), shape_dict={'shape': 'sphere', 'feature': float(r)}, id=i)
                 for i, (p, r) in enumerate(zip(take['obs_pos'], take['obs_radius']))]
    return eps, obstacles


def _waves(mods, eps, obstacles, slots):
    E, metrics, scenarios, scenes = mods
    out, steps_total = [], 0
    for w in range(0, len(eps), slots):
        batch = scenes.SceneBatch(eps[w:w + slots], obstacles, device_tracker=True)
        taken = 1
        while not batch.step():
            taken += 1
            assert taken < 5000, ('a wave that does not end', w)
        steps_total += taken
        for s in range(len(batch)):
            lo, hi = int(batch.offsets[s]), int(batch.offsets[s + 1])
            out.append(dict(metrics=metrics.episode_metrics(batch.env(s)), steps=int(batch.steps[s]),
                            state={k: batch._state(k)[lo:hi].copy() for k in batch._mirror}))
        batch.close()
    return out, steps_total


def test_stream_equals_waves(mods):
    E, metrics, scenarios, scenes = mods
    slots = 4
    eps, obstacles = _queue(E, scenarios)
    assert len(eps) >= 3 * slots
    stats, order = {}, []
    got = scenes.run_episodes(eps, slots, obstacles=obstacles, device_tracker=True, on_done=lambda r: order.append(r['episode']), stats=stats,
                              max_steps=20000)
    eps2, obstacles2 = _queue(E, scenarios)
    want, wave_steps = _waves(mods, eps2, obstacles2, slots)
    assert [r['episode'] for r in got] == list(range(len(eps))) and sorted(order) == list(range(len(eps)))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g['steps'] == w['steps'] > 1, (i, g['steps'], w['steps'])
        for key in w['metrics']:
            if key not in WALL:
                assert np.array_equal(g['metrics'][key], w['metrics'][key], equal_nan=True), (i, key, g['metrics'][key], w['metrics'][key])
        for key in w['state']:
            assert np.array_equal(g['state'][key], w['state'][key]), (i, key)
    sizes = [len(e) for e in eps]
    assert {r['slot'] for r, n in zip(got, sizes) if n == 14} == {3}               # the reserved slot: entries 0, 1, 2 and the first 14
    assert all(r['slot'] != 3 for r, n in zip(got, sizes) if n == 16)
    assert stats['batch_steps'] <= wave_steps and 0.0 < stats['live_fraction'] <= 1.0
    print('batch steps: stream %d, waves %d; live fraction of the stream %.3f' % (stats['batch_steps'], wave_steps, stats['live_fraction']))


def test_restart_rebinds_the_views_and_refuses_what_a_slot_cannot_hold(mods):
    E, metrics, scenarios, scenes = mods
    eps, obstacles = _queue(E, scenarios)
    batch = scenes.SceneBatch(eps[:3], obstacles, device_tracker=True)
    for _ in range(20):
        batch.step()
    old = batch.env(1).agents
    moved = old[0].pos_global_frame.copy()
    new = eps[5]
    batch.restart({1: new})
    view = batch.env(1)
    assert view.agents is not old and all(a is b for a, b in zip(view.agents, new))             # the new objects
    assert batch.steps.tolist() == [20, 0, 20] and batch.active[1] == 16
    assert np.array_equal(new[0].pos_global_frame, new[0].initial_pos[:3]) and not np.array_equal(new[0].pos_global_frame, moved)
    assert new[3].step_num == 0 and new[3].total_dist == 0.0 and not new[3].is_run_done and new[3].total_time == 0.0
    assert np.array_equal(view.goal, [a.goal_global_frame for a in new])
    assert np.array_equal(batch.policy_ids[16:32], [a.policy.policy_id for a in new])
    assert view.kdTree.agentIDs == list(range(16))
    batch.step()
    assert batch.steps.tolist() == [21, 1, 21] and new[3].step_num == 1
    before = {k: batch._state(k).copy() for k in batch._mirror}
    path = agents_of(scenarios.circle(16), E.RVO3DPolicy)
    path[2].path = [[0.0, 0.0, 10.0]]
    other = agents_of(scenarios.circle(16), E.RVO3DPolicy)
    other[4].neighborDist = 7.0
    turn = agents_of(scenarios.circle(16), E.SCAPolicy)
    turn[1].turning_radius = 2.5
    ids = agents_of(scenarios.circle(16), E.RVO3DPolicy)
    ids[0].id = 1
    for bad in ({0: path}, {0: other}, {0: turn}, {0: ids}, {0: eps[12]}, {3: eps[6]}):
        with pytest.raises(ValueError):
            batch.restart(bad)
    for k, v in before.items():                                                                  # raised before any device call
        assert np.array_equal(batch.solver.get_state()[k], v), k
    assert batch.steps.tolist() == [21, 1, 21]
    batch.close()


def test_what_the_queue_and_the_planner_attributes_refuse(mods):
    """planner attributes per agent: a new agent on the other side of tracked / untracked is a ValueError before any device call; a queue
    whose first tracked episode comes after the slots' first episodes is refused before the first step"""
    E, metrics, scenarios, scenes = mods
    sc = scenarios.circle(16, rad=6.0, z=12.0)
    mixed = [E.Agent(start_pos=list(sc['start'][i]), goal_pos=list(sc['goal'][i]), vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0,
                     policy=E.SCAPolicy if i % 2 else E.RVO3DPolicy, id=i) for i in range(16)]
    mixed[1].turning_radius = 2.0                                                                # (two classes: the attributes go per agent)
    batch = scenes.SceneBatch([mixed, agents_of(sc, E.RVO3DPolicy)], [], device_tracker=True)
    batch.step()
    before = batch.solver.get_state()
    with pytest.raises(ValueError):
        batch.restart({1: agents_of(sc, E.SCAPolicy)})                                          # untracked rows become tracked
    with pytest.raises(ValueError):
        batch.restart({0: agents_of(sc, E.RVO3DPolicy)})                                        # tracked rows become untracked
    for k, v in batch.solver.get_state().items():
        assert np.array_equal(before[k], v), k
    batch.restart({1: agents_of(sc, E.ORCA3DPolicy)})                                           # untracked stays untracked: taken
    assert batch.steps.tolist() == [1, 0]
    batch.close()
    eps, obstacles = _queue(E, scenarios)
    late = [eps[2], eps[3], eps[6], eps[0]]                                                      # RVO, RVO, ORCA ... then SCA
    with pytest.raises(ValueError):
        scenes.run_episodes(late, 2, obstacles=obstacles, device_tracker=True)
