"""Helpers of tests/test_gpu_scene_sizes.py: slots of a capacity (sca_restart_scenes_sized).  SizedSlots is scene_util.Slots with one
obstacle set per slot and a restart that may bring an episode of another agent count; context / sized_restart / alone build synthetic
batches.  Everything is compared with array_equal."""
import numpy as np

from scene_util import Slots, assert_scene_equals_alone, episode_arrays, everything, load_any

NO_OBSTACLES = (np.zeros((0, 3)), np.zeros(0))


def circle_scene(S, n, policy, rad=None, turn=0):
    """n agents on a circle (scenarios.circle), goals at the antipodes, the arrays sca_set_agents / sca_restart_scenes take"""
    from sca_amd import scenarios
    sc = scenarios.circle(n, rad=rad)
    start, goal = np.roll(sc['start'], turn, axis=0), np.roll(sc['goal'], turn, axis=0)
    if n == 1:                                                     # (a circle of one has its goal where it starts: send it 6 m across instead)
        goal = goal + [-6.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    return dict(n=n, pos=start[:, :3], heading=start[:, 3:6], vel=np.zeros((n, 3), np.float32), radius=np.full(n, 0.5), pref_speed=np.ones(n),
                goal=goal[:, :3], policy=np.broadcast_to(np.asarray(policy, np.uint8), (n,)).copy(), zaxis=S.zaxis_flags(start, goal),
                max_run_dist=scenarios.max_run_dist(start, goal), goal_heading=goal[:, 3:6])


def padded(ep, cap):
    """the episode's arrays with its last agent repeated up to `cap` rows: what fills a slot of that capacity before it is vacated"""
    idx = np.minimum(np.arange(cap), ep['n'] - 1)
    return {k: (cap if k == 'n' else v[idx]) for k, v in ep.items() if k not in ('obs_pos', 'obs_radius')}


def context(S, eps, obstacles=None, tracker=True):
    """episodes as the scenes of one context, every scene full; obstacles: one (pos, radius) per scene.  Returns (solver, offsets)."""
    off = np.concatenate([[0], np.cumsum([e['n'] for e in eps])]).astype(np.int32)
    n = int(off[-1])
    cat = lambda key: np.concatenate([e[key] for e in eps])
    m = sum(len(r) for _, r in obstacles) if obstacles else 0
    sol = S.BatchedSolver(max_agents=n, max_obstacles=max(m, 1))
    sol.set_agents(cat('radius'), cat('pref_speed'), cat('goal'), cat('policy'), cat('zaxis'), cat('max_run_dist'))
    sol.set_scenes(off)
    if obstacles:
        sol.set_scene_obstacles(obstacles)
    if tracker:
        sol.device_tracker_enable(cat('goal_heading'), in_pass=True)
    sol.set_state(cat('pos'), cat('vel'), cat('heading'), np.zeros(n, np.uint8))
    return sol, off


def sized_restart(sol, ids, eps, sizes='own', tracker=True, **drop):
    """one sca_restart_scenes_sized call: scene ids[b] takes episode eps[b]; sizes 'own': the episodes' agent counts, None: NULL"""
    cat = lambda key: np.concatenate([e[key] for e in eps])
    kw = dict(vel=cat('vel'), radius=cat('radius'), pref_speed=cat('pref_speed'), goal=cat('goal'), policy=cat('policy'), zaxis=cat('zaxis'),
              max_run_dist=cat('max_run_dist'), goal_heading=cat('goal_heading') if tracker else None)
    kw.update(drop)
    sol.restart_scenes(ids, cat('pos'), cat('heading'), sizes=[e['n'] for e in eps] if isinstance(sizes, str) else sizes, **kw)


def partial_batch(S, eps, cap, obstacles=None):
    """len(eps) slots of capacity `cap`, slot s holding eps[s]: a full batch of the padded episodes, then ONE sized restart of all slots"""
    sol, off = context(S, [padded(e, cap) for e in eps], obstacles=obstacles)
    sized_restart(sol, list(range(len(eps))), eps)
    return sol, off


def tracked(ep):
    return np.flatnonzero(np.isin(ep['policy'], (0, 5)))


def assert_slots_equal_alone(sol, off, held, solos, ctx, obs_lo=None):
    """slot s of the batch, its first held[s]['n'] rows, against solos[s], a context of that episode alone: every value of the contract"""
    got = everything(sol, [int(off[s]) + a for s in solos for a in tracked(held[s])])
    for s, x in solos.items():
        lo = int(off[s])
        assert_scene_equals_alone(got, lo, lo + held[s]['n'], 0 if obs_lo is None else obs_lo[s], everything(x, tracked(held[s])), ctx + ('slot', s))
    return got


def assert_vacant(got, off, sizes, ctx):
    """what include/sca_hip.h says the rows behind a slot's episode read"""
    for s, size in enumerate(sizes):
        v = slice(int(off[s]) + int(size), int(off[s + 1]))
        assert (got['flags'][v] == 3).all() and not got['vel'][v].any() and not got['heading'][v].any(), ctx + (s, 'vacant state')
        assert not got['total_dist'][v].any() and not got['step_num'][v].any() and not got['action'][v].any(), ctx + (s, 'vacant counters / action')
        assert not got['nbr_n'][v].any() and np.array_equal(got['perm'][v], np.arange(v.start, v.stop)), ctx + (s, 'vacant lists / perm')
        occ = slice(int(off[s]), v.start)
        assert np.array_equal(np.sort(got['perm'][occ]), np.arange(occ.start, occ.stop)), ctx + (s, 'perm of the occupied rows')
        ids = got['nbr_id'][occ][got['nbr_kind'][occ] == 0]
        assert ((ids < v.start) & ((ids >= occ.start) | (ids < 0))).all(), ctx + (s, 'a neighbour list holds a vacant or foreign id')


def recorded_arrays(fx):
    """episode_arrays of a recorded episode that starts at its record 0, with the velocities that record holds: the packed episodes were
    recorded with agents already moving, and a restart takes the velocities as it takes the positions"""
    assert int(fx['step'][0]) == 0 and np.array_equal(fx['pos'][0], fx['start'][:, :3])
    return dict(episode_arrays(fx), vel=fx['vel'][0])


class SizedSlots(Slots):
    """Episodes as slots of a capacity: slot s starts full with scenes[s] -- the name of a recorded episode, or a dict of arrays
    (circle_scene), which has no records -- and restart() may give it a recorded episode of any smaller count.  obstacles: one (pos, radius)
    per slot, a recorded episode's own set where it has one."""

    def __init__(self, S, scenes, obstacles=None):
        self.S, self.B = S, len(scenes)
        self.names = [x if isinstance(x, str) else 'synthetic' for x in scenes]
        self.fx = [load_any(x) if isinstance(x, str) else None for x in scenes]
        ep = [x if f is None else recorded_arrays(f) for x, f in zip(scenes, self.fx)]
        self.obstacles = obstacles
        self.tracker = True
        self.sol, self.off = context(S, ep, obstacles=obstacles)
        self.size = np.diff(self.off)
        self.n = int(self.off[-1])
        self.t = 0
        self.t0 = [0] * self.B
        self.steps_want = np.zeros(self.B, np.int64)
        self._bind()

    def _bind(self):
        self.index = [{} if f is None else {int(t): k for k, t in enumerate(f['step'])} for f in self.fx]
        self.done_step = [int(f['done_step']) if f is not None and 'done_step' in f else -1 for f in self.fx]

    def sl(self, s):
        return slice(int(self.off[s]), int(self.off[s]) + int(self.size[s]))

    def restart(self, plan):
        """{slot: fixture name}: one sized restart with every array passed"""
        ids = sorted(plan)
        fx = {s: load_any(plan[s]) for s in ids}
        ep = [recorded_arrays(fx[s]) for s in ids]
        for s, e in zip(ids, ep):                                  # the episode was recorded with the obstacle set its slot has
            want = NO_OBSTACLES if self.obstacles is None else self.obstacles[s]
            assert np.array_equal(e['obs_pos'], want[0]) and np.array_equal(e['obs_radius'], want[1]), plan[s]
        sized_restart(self.sol, ids, ep)
        for s, e in zip(ids, ep):
            self.fx[s], self.names[s], self.t0[s], self.steps_want[s], self.size[s] = fx[s], plan[s], self.t, 0, e['n']
        self._bind()


def alone(S, name):
    """a recorded episode in a context of its own, with its own obstacles as the one scene's set"""
    e = recorded_arrays(load_any(name))
    return context(S, [e], obstacles=[(e['obs_pos'], e['obs_radius'])] if len(e['obs_radius']) else None)[0], e
