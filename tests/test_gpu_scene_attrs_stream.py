"""scenes.run_episodes(..., attributes=True) (-m gpu): a queue that mixes default episodes, episodes with one non-default setting for all
agents (F16 style) and episodes whose agents each carry their own (F17 / F18 style) streams through four slots.  Per episode the metrics
rows (the wall-time column left out), the step count and the final state are what a MACAEnv holding that episode alone gives."""
import numpy as np
import pytest

from scene_util import agents_of

pytestmark = pytest.mark.gpu

WALL = ('AverageCost',)                                             # wall time of the policy calls: differs from run to run
STATE = ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num')


@pytest.fixture(scope='module')
def mods():
    from sca_amd import env as E, metrics, scenarios, scenes
    return E, metrics, scenarios, scenes


def _queue(E, scenarios):
    """ten episodes of 20 .. 60 drones, a fresh list of Agent objects at every call: default attributes, one setting for the whole episode,
    and settings of the agents' own (drawn from the values the F17 / F18 recordings use)"""
    rng = np.random.default_rng(5)
    pols = [E.SCAPolicy, E.RVO3DPolicy, E.SRVO3DPolicy, E.ORCA3DPolicy, E.ORCA3DPolicyOfficial, E.RVO3dDubinsPolicy]
    eps = []

    def circle(n, policy, rad):
        return agents_of(scenarios.circle(n, rad=rad, z=12.0), policy)

    def mixed(n, rad):
        sc = scenarios.circle(n, rad=rad, z=12.0)
        return [E.Agent(start_pos=list(sc['start'][i]), goal_pos=list(sc['goal'][i]), vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0,
                        policy=pols[i % 6], id=i) for i in range(n)]
    eps.append(circle(20, E.RVO3DPolicy, 5.0))                      # 0: default
    e = circle(24, E.ORCA3DPolicy, 6.0)                             # 1: neighborDist 4, maxNeighbors 4 for everybody
    for a in e:
        a.neighborDist, a.maxNeighbors = 4.0, 4
    eps.append(e)
    e = mixed(36, 8.0)                                              # 2: every agent its own solver attributes
    for a in e:
        a.neighborDist, a.maxNeighbors = float(rng.choice([2.5, 5.0, 10.0, 15.0])), int(rng.choice([2, 4, 8, 16]))
        a.timeHorizon, a.maxSpeed = float(rng.choice([3.0, 5.0, 10.0])), float(rng.choice([1.0, 1.5]))
    eps.append(e)
    eps.append(circle(20, E.SCAPolicy, 6.0))                        # 3: default, tracked
    e = circle(20, E.SCAPolicy, 6.0)                                # 4: turning radius 3 for everybody
    for a in e:
        a.turning_radius = 3.0
    eps.append(e)
    e = mixed(60, 12.0)                                             # 5: time step 0.2, and planner attributes of the agents' own
    for a in e:
        a.timeStep = 0.2
        a.turning_radius, a.pitchlims = float(rng.choice([0.8, 1.5, 3.0])), [-0.5, float(rng.choice([0.5, 0.9]))]
    eps.append(e)
    eps.append(circle(30, E.ORCA3DPolicyOfficial, 7.0))             # 6: default, ORCA3D-LP
    e = circle(30, E.SRVO3DPolicy, 7.0)                             # 7: time horizon 3, max_heading_change pi / 6
    for a in e:
        a.timeHorizon, a.max_heading_change = 3.0, np.pi / 6
    eps.append(e)
    e = mixed(48, 10.0)                                             # 8: dt_nominal 0.05 and neighborDist of the agents' own
    for a in e:
        a.dt_nominal, a.neighborDist = 0.05, float(rng.choice([5.0, 10.0]))
    eps.append(e)
    eps.append(mixed(24, 6.0))                                      # 9: default, all six policies
    return eps


def _alone(mods, agents):
    E, metrics, scenarios, scenes = mods
    env = E.MACAEnv(device_tracker=True)
    env.set_agents(agents, obstacles=[])
    steps = 1
    while not env.step({}) and steps < 4000:
        steps += 1
    assert steps < 4000
    out = dict(metrics=metrics.episode_metrics(env), steps=steps, state={k: getattr(env, k).copy() for k in STATE})
    env.solver.close()
    return out


def test_a_queue_of_mixed_attributes_streams_through_four_slots(mods):
    E, metrics, scenarios, scenes = mods
    eps = _queue(E, scenarios)
    assert 20 <= min(map(len, eps)) and max(map(len, eps)) == 60
    stats = {}
    got = scenes.run_episodes(eps, 4, device_tracker=True, capacities='max', attributes=True, stats=stats, max_steps=20000)
    want = [_alone(mods, e) for e in _queue(E, scenarios)]
    assert len({r['slot'] for r in got}) == 4 and stats['batch_steps'] < sum(w['steps'] for w in want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g is not None and g['steps'] == w['steps'] > 1, (i, g and g['steps'], w['steps'])
        for key in w['metrics']:
            if key not in WALL:
                assert np.array_equal(g['metrics'][key], w['metrics'][key], equal_nan=True), (i, key, g['metrics'][key], w['metrics'][key])
        for key in STATE:
            assert np.array_equal(g['state'][key], w['state'][key]), (i, key)


def test_the_views_follow_the_attributes(mods):
    """SceneBatch(attribute_slots=True).restart: accepted, the mirrors current; a tracked <-> untracked change among them"""
    E, metrics, scenarios, scenes = mods
    eps = _queue(E, scenarios)
    batch = scenes.SceneBatch([eps[3], eps[0]], device_tracker=True, capacities=[60, 60], attribute_slots=True)
    assert batch.env(0).per_agent_attributes == [] and batch.env(1).per_agent_attributes == []
    batch.step()
    batch.restart({1: eps[5], 0: eps[2]})                           # slot 0: SCA agents -> all six policies
    assert batch.env(1).per_agent_attributes == ['turning_radius / pitchlims']
    assert batch.env(0).per_agent_attributes == ['max_neighbors', 'max_speed', 'neighbor_dist', 'time_horizon']
    lo = int(batch.offsets[1])
    assert all(batch._planner_of(lo + a.id) == (float(a.turning_radius), float(a.pitchlims[0]), float(a.pitchlims[1])) for a in eps[5])
    batch.step()
    assert batch.steps.tolist() == [1, 1]
    batch.close()


def test_without_the_flag_the_queue_still_raises(mods):
    E, metrics, scenarios, scenes = mods
    with pytest.raises(ValueError, match='a slot keeps its'):
        scenes.run_episodes(_queue(E, scenarios), 4, device_tracker=True, capacities='max', max_steps=20000)
