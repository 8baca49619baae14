"""Helpers of the scene tests (tests/test_gpu_scene*.py), the one module they share.  load_any, everything and assert_scene_equals_alone
serve all of them.  Slots: recorded episodes as the slots of one context, where a slot may be given another recorded episode while the
batch runs (sca_restart_scenes); every slot is held against the reference's records of the episode it holds AT THAT MOMENT, counted from
the step the episode was put in.  SizedSlots: Slots with one obstacle set per slot and a restart that may bring an episode of another
agent count (sca_restart_scenes_sized).  circle_scene / context / restart_all / partial_batch build synthetic batches; rc_of, step_all,
same, observe, agents_of and the harvest's summary loop are what several modules need once.  Everything is compared with array_equal."""
import os

import numpy as np
import pytest

from golden_util import GOLDEN, static_inputs


def load_any(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False))


def episode_arrays(fx):
    """what sca_set_agents / sca_set_state / sca_device_tracker_enable -- and sca_restart_scenes -- take of a recorded episode"""
    st = static_inputs(fx)
    n = len(st['radius'])
    return dict(n=n, pos=fx['start'][:, :3], heading=fx['start'][:, 3:6], vel=np.zeros((n, 3), np.float32), radius=st['radius'],
                pref_speed=st['pref_speed'], goal=fx['goal'][0], policy=st['policy'], zaxis=st['zaxis'], max_run_dist=st['max_run_dist'],
                goal_heading=fx['goal6'][:, 3:6], obs_pos=st['obs_pos'].reshape(-1, 3), obs_radius=st['obs_radius'])


class Slots:
    """B recorded episodes in one context, each a scene (shared obstacles, device tracker in the pass)"""

    def __init__(self, S, names, scenes=True):
        self.S, self.B = S, len(names)
        self.names = list(names)
        self.fx = [load_any(n) for n in names]
        ep = [episode_arrays(f) for f in self.fx]
        self.off = np.concatenate([[0], np.cumsum([e['n'] for e in ep])]).astype(np.int32)
        self.n = int(self.off[-1])
        cat = lambda key: np.concatenate([e[key] for e in ep])
        with_obs = [e for e in ep if len(e['obs_radius'])]
        self.obs_pos = with_obs[0]['obs_pos'] if with_obs else np.zeros((0, 3))
        self.obs_radius = with_obs[0]['obs_radius'] if with_obs else np.zeros(0)
        for e in ep:                                               # one shared set: every episode of the batch was recorded with it
            assert np.array_equal(e['obs_pos'], self.obs_pos) and np.array_equal(e['obs_radius'], self.obs_radius)
        sol = self.sol = S.BatchedSolver(max_agents=self.n, max_obstacles=max(len(self.obs_radius), 1))
        sol.set_obstacles(self.obs_pos, self.obs_radius)
        sol.set_agents(cat('radius'), cat('pref_speed'), cat('goal'), cat('policy'), cat('zaxis'), cat('max_run_dist'))
        if scenes:
            sol.set_scenes(self.off)
        self.tracker = bool(np.isin(cat('policy'), (0, 5)).any())
        if self.tracker:
            sol.device_tracker_enable(cat('goal_heading'), in_pass=True)
        sol.set_state(cat('pos'), cat('vel'), cat('heading'), np.zeros(self.n, np.uint8), np.zeros(self.n), np.zeros(self.n, np.int32))
        sol.set_kd_perm(np.arange(self.n, dtype=np.int32))
        self.t = 0                                                 # batch steps taken
        self.t0 = [0] * self.B                                     # the batch step each slot's episode started at
        self.steps_want = np.zeros(self.B, np.int64)
        self._bind()

    def _bind(self):
        self.index = [{int(t): k for k, t in enumerate(f['step'])} for f in self.fx]
        self.done_step = [int(f['done_step']) if 'done_step' in f else -1 for f in self.fx]

    def sl(self, s):
        return slice(int(self.off[s]), int(self.off[s + 1]))

    def restart(self, plan):
        """{slot: fixture name}: one sca_restart_scenes call with every array passed"""
        ids = sorted(plan)
        fx = {s: load_any(plan[s]) for s in ids}
        ep = [episode_arrays(fx[s]) for s in ids]
        for s, e in zip(ids, ep):
            assert e['n'] == self.off[s + 1] - self.off[s]
        cat = lambda key: np.concatenate([e[key] for e in ep])
        self.sol.restart_scenes(ids, cat('pos'), cat('heading'), vel=cat('vel'), radius=cat('radius'), pref_speed=cat('pref_speed'), goal=cat('goal'),
                                policy=cat('policy'), zaxis=cat('zaxis'), max_run_dist=cat('max_run_dist'),
                                goal_heading=cat('goal_heading') if self.tracker else None)
        for s in ids:
            self.fx[s], self.names[s], self.t0[s], self.steps_want[s] = fx[s], plan[s], self.t, 0
        self._bind()

    def snapshot(self):
        return dict(state=self.sol.get_state(), perm=self.sol.get_kd_perm())

    def check_state(self, snap, s, k, when, ctx):
        f, sl, lo = self.fx[s], self.sl(s), int(self.off[s])
        ctx = ctx + (s, self.names[s], 'record', k, when or 'before')
        for key in ('pos', 'heading', 'total_dist', 'flags'):
            assert np.array_equal(snap['state'][key][sl], f[key + when][k]), ctx + (key,)
        assert np.array_equal(snap['state']['vel'][sl][:, :3], f['vel' + when][k]), ctx + ('vel',)
        assert np.array_equal(snap['perm'][sl] - lo, f['perm' + when][k]), ctx + ('perm',)

    def live(self, snap):
        return np.array([((snap['state']['flags'][self.sl(s)] & 7) == 0).sum() for s in range(self.B)])

    def run_and_check(self, steps, step_fn=None, after_step=None, label=''):
        """`steps` batch steps; every slot that has a record of its episode's step (batch step - the step it was put in) is compared before
        and after it; a slot beyond its episode's `done_step` stays what the last record left, its action rows zero; steps[s] / active[s]
        follow.  after_step(t): called behind every step's checks.  Returns the (slot, step) records compared, per slot."""
        S, sol = self.S, self.sol
        step_fn = step_fn or (lambda: (sol.run_steps(1, S.NBR_KDTREE), sol.synchronize()))
        compared = np.zeros(self.B, np.int64)
        snap = self.snapshot()
        for _ in range(steps):
            t, ctx = self.t, (label, 'batch step', self.t)
            live_before = self.live(snap)
            for s in range(self.B):
                if t - self.t0[s] in self.index[s]:
                    self.check_state(snap, s, self.index[s][t - self.t0[s]], '', ctx)
            step_fn()
            self.t += 1
            self.steps_want += live_before > 0
            snap = self.snapshot()
            a, status = sol.actions(), sol.diag()['status']
            for s in range(self.B):
                sl, local = self.sl(s), t - self.t0[s]
                if local in self.index[s]:
                    k, f = self.index[s][local], self.fx[s]
                    called = f['called'][k].astype(bool)
                    assert np.array_equal(a[sl][called], f['action'][k][called]), ctx + (s, self.names[s], 'action')
                    assert not status[sl].any(), ctx + (s, self.names[s], 'status')
                    self.check_state(snap, s, k, '_after', ctx)
                    compared[s] += 1
                elif 0 <= self.done_step[s] < local and self.done_step[s] == int(self.fx[s]['step'][-1]):      # finished: inert
                    self.check_state(snap, s, len(self.fx[s]['step']) - 1, '_after', ctx + ('inert',))
                    assert not a[sl].any(), ctx + (s, self.names[s], 'action rows of a finished scene')
            sc = sol.scene_state()
            live = self.live(snap)
            assert np.array_equal(sc['active'], live), ctx + ('active', sc['active'].tolist(), live.tolist())
            assert np.array_equal(sc['steps'], self.steps_want), ctx + ('steps', sc['steps'].tolist(), self.steps_want.tolist())
            assert sol.active_count() == int(live.sum()), ctx
            if after_step is not None:
                after_step(t)
        return compared


def everything(sol, tracker_agents=()):
    """every value the contract names that a context can be asked for between steps; tracker_agents: ids whose tracker records are read"""
    out = dict(sol.get_state())
    out['action'] = sol.actions()
    out['perm'] = sol.get_kd_perm()
    nb = sol.neighbors()
    out.update({k: nb[k] for k in ('nbr_n', 'nbr_id', 'nbr_kind', 'nbr_dsq', 'nbr_valid')})
    d = sol.diag()
    out.update(diag=d['diag'], status=d['status'], vpref=d['vpref'])
    if len(tracker_agents):
        out['replans'] = sol.device_tracker_replans()
        out['track'] = {int(a): sol.device_tracker_debug(int(a)) for a in tracker_agents}
    return out


def assert_scene_equals_alone(got, lo, hi, obs_lo, alone, ctx):
    """agents [lo, hi) of a batch against a context that holds them alone: ids are global in the batch (agents + lo, obstacles + obs_lo)"""
    for key, want in alone.items():
        if key == 'track':
            for a, rec in want.items():
                assert np.array_equal(got['track'][lo + a], rec, equal_nan=True), ctx + ('tracker record', a)
            continue
        have = got[key][lo:hi]
        if key == 'perm':
            have = have - lo
        elif key == 'nbr_id':
            kind = got['nbr_kind'][lo:hi]
            have = have - np.where(have >= 0, np.where(kind == 1, obs_lo, lo), 0)
        assert np.array_equal(have, want, equal_nan=key == 'vpref'), ctx + (key,)


def rc_of(S, fn):
    """the library's return code of a call that must fail"""
    with pytest.raises(S.ScaError) as e:
        fn()
    return int(str(e.value).rsplit('rc=', 1)[1].rstrip(')'))


def step_all(S, *sols, k=1):
    for x in sols:
        x.run_steps(k, S.NBR_KDTREE)
        x.synchronize()


def same(a, b, ctx, keys=None, nan_keys=None):
    """two everything() dicts, key by key; nan_keys: the keys in which a NaN equals a NaN (None: every key)"""
    for key in (keys or a):
        nan = nan_keys is None or key in nan_keys
        if key == 'track':
            for i in a[key]:
                assert np.array_equal(a[key][i], b[key][i], equal_nan=nan), ctx + (key, i)
        else:
            assert np.array_equal(a[key], b[key], equal_nan=nan), ctx + (key,)


def observe(sol):
    """what a refused call must leave as it was: the state, the permutation, the scenes' counters and sizes"""
    out = dict(sol.get_state())
    out['perm'] = sol.get_kd_perm()
    out.update(sol.scene_state())
    out['sizes'] = sol.scene_sizes()
    return out


def agents_of(sc, policy, count=None):
    """the scenario's first `count` agents (all of them) as fresh E.Agent objects of one policy"""
    from sca_amd import env as E
    n = len(sc['start']) if count is None else count
    return [E.Agent(start_pos=list(sc['start'][i]), goal_pos=list(sc['goal'][i]), vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0,
                    policy=policy, id=i) for i in range(n)]


def loop_summary(st, lo, hi):
    """metrics.episode_metrics' loop over sca_get_state: Python ints and floats, agent order"""
    f = st['flags'][lo:hi]
    num, dist, steps = 0, 0.0, 0
    for i in range(lo, hi):
        if not (int(st['flags'][i]) & 6):
            num += 1
            dist += float(st['total_dist'][i])
            steps += int(st['step_num'][i])
    return dict(arrived=int(((f & 1) != 0).sum()), collided=int(((f & 2) != 0).sum()), timed_out=int(((f & 4) != 0).sum()), successful_num=num,
                all_step_num=steps, all_distance=dist)


def assert_summary(rec, want, steps, batch_step, ctx):
    for k, v in want.items():
        assert rec[k].item() == v, ctx + (k, rec[k].item(), v)
    assert (int(rec['steps']), int(rec['batch_step'])) == (steps, batch_step), ctx + ('steps / batch_step', int(rec['steps']), int(rec['batch_step']))


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


def context(S, eps, obstacles=None, obs_slots=None, shared=None, tracker=True, max_obstacles=None):
    """episodes as the scenes of one context, every scene full.  obstacles: one (pos, radius) per scene (sca_set_scene_obstacles); with
    obs_slots, the obstacle capacity of every scene, they are what the slots hold (sca_set_scene_obstacle_slots; None: empty); shared: one
    (pos, radius) for all scenes (sca_set_obstacles).  Returns (solver, offsets)."""
    off = np.concatenate([[0], np.cumsum([e['n'] for e in eps])]).astype(np.int32)
    n = int(off[-1])
    cat = lambda key: np.concatenate([e[key] for e in eps])
    if max_obstacles is None:
        m = sum(obs_slots) if obs_slots is not None else sum(len(r) for _, r in obstacles) if obstacles else len(shared[1]) if shared else 0
        max_obstacles = max(int(m), 1)
    sol = S.BatchedSolver(max_agents=n, max_obstacles=max_obstacles)
    if shared:
        sol.set_obstacles(*shared)
    sol.set_agents(cat('radius'), cat('pref_speed'), cat('goal'), cat('policy'), cat('zaxis'), cat('max_run_dist'))
    sol.set_scenes(off)
    if obs_slots is not None:
        sol.set_scene_obstacle_slots(obs_slots, obstacles)
    elif obstacles:
        sol.set_scene_obstacles(obstacles)
    if tracker:
        sol.device_tracker_enable(cat('goal_heading'), in_pass=True)
    sol.set_state(cat('pos'), cat('vel'), cat('heading'), np.zeros(n, np.uint8))
    return sol, off


def restart_all(sol, ids, eps, sizes=None, obstacles=None, tracker=True, **drop):
    """one restart call with every array passed: scene ids[b] takes episode eps[b].  sizes 'own': the episodes' agent counts, a list: as
    given; obstacles: per named scene (pos, radius), or None for a scene that keeps its set.  Neither is sca_restart_scenes, sizes alone
    sca_restart_scenes_sized, obstacles sca_restart_scenes_obstacles.  drop: arrays passed differently (None: not at all)."""
    cat = lambda key: np.concatenate([e[key] for e in eps])
    kw = dict(vel=cat('vel'), radius=cat('radius'), pref_speed=cat('pref_speed'), goal=cat('goal'), policy=cat('policy'), zaxis=cat('zaxis'),
              max_run_dist=cat('max_run_dist'), goal_heading=cat('goal_heading') if tracker else None)
    kw.update(drop)
    sol.restart_scenes(ids, cat('pos'), cat('heading'), sizes=[e['n'] for e in eps] if isinstance(sizes, str) else sizes, obstacles=obstacles, **kw)


def partial_batch(S, eps, cap, obstacles=None):
    """len(eps) slots of capacity `cap`, slot s holding eps[s]: a full batch of the padded episodes, then ONE sized restart of all slots"""
    sol, off = context(S, [padded(e, cap) for e in eps], obstacles=obstacles)
    restart_all(sol, list(range(len(eps))), eps, sizes='own')
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
        restart_all(self.sol, ids, ep, sizes='own')
        for s, e in zip(ids, ep):
            self.fx[s], self.names[s], self.t0[s], self.steps_want[s], self.size[s] = fx[s], plan[s], self.t, 0, e['n']
        self._bind()


def alone(S, name):
    """a recorded episode in a context of its own, with its own obstacles as the one scene's set"""
    e = recorded_arrays(load_any(name))
    return context(S, [e], obstacles=[(e['obs_pos'], e['obs_radius'])] if len(e['obs_radius']) else None)[0], e


# ---- seeded random scenes and their oracle runs (test_gpu_scenes.py, test_gpu_scene_obstacles.py) --------------------------------------------
RANDOM_SIZES = [1, 2, 3, 9, 10, 11, 20, 21, 257, 1023, 1024, 1025, 1536]


def random_scenes(S):
    """64 scenes: every size of RANDOM_SIZES once, the rest drawn from the small ones; mixed policies; six shared obstacles"""
    from sca_amd import scenarios
    rng = np.random.default_rng(2024)
    sizes = RANDOM_SIZES + [int(x) for x in rng.choice(RANDOM_SIZES[:9], 64 - len(RANDOM_SIZES))]
    obs_pos = np.round(rng.uniform(-8, 8, (6, 3)) + [0, 0, 12.0], 2)
    obs_radius = np.full(6, 1.0)
    scenes = []
    for s, size in enumerate(sizes):
        if size >= 257:
            sc = scenarios.circle(size) if s % 2 else scenarios.random_cube(size, seed=s)
        else:
            # small scenes: a few metres apart, so that neighbours, obstacles and collisions happen within the six steps
            pos = np.round(rng.uniform(-6, 6, (size, 3)) * [1, 1, 0.5] + [0, 0, 12.0], 2)
            goal = np.round(-pos * [1, 1, 0] + [0, 0, 1] * pos + rng.uniform(-1, 1, (size, 3)), 2)
            start = np.zeros((size, 6)); start[:, :3] = pos
            start[:, 3] = np.arctan2(goal[:, 1] - pos[:, 1], goal[:, 0] - pos[:, 0])
            g6 = np.zeros((size, 6)); g6[:, :3] = goal
            sc = dict(start=start, goal=g6)
        policy = rng.integers(0, 6, size).astype(np.uint8) if s % 3 else np.full(size, s % 6, np.uint8)
        scenes.append(dict(start=sc['start'], goal=sc['goal'], policy=policy, zaxis=S.zaxis_flags(sc['start'], sc['goal']),
                           mrd=scenarios.max_run_dist(sc['start'], sc['goal']), n=size))
    return scenes, sizes, obs_pos, obs_radius


_ORACLE_RUNS = {}


def oracle_scene_runs(oracle, key, scenes, obstacle_sets, steps=6, stop_when_done=False):
    """Every scene alone through the oracle (policy_step / env_update / Tracker), `steps` free-running steps, made once per `key` and shared by
    the K1 forms that are compared with it.  Per scene: `steps` (one dict per step: p = policy_step's result, active = the tracked agents it
    served, and the state after the step -- or, with stop_when_done, None from the step on at which every agent was done: the reference's
    `while not env.step()` has stopped by then), `last` (the state the scene ended on), ext and the tracker's re-plan counts."""
    if key in _ORACLE_RUNS:
        return _ORACLE_RUNS[key]
    out = []
    for sc, (obs_pos, obs_radius) in zip(scenes, obstacle_sets):
        m = sc['n']
        r = dict(pos=sc['start'][:, :3].copy(), vel=np.zeros((m, 3), np.float32), head=sc['start'][:, 3:6].copy(), flags=np.zeros(m, np.uint8),
                 td=np.zeros(m), sn=np.zeros(m, np.int32), perm=np.arange(m, dtype=np.int32))
        ext = np.isin(sc['policy'], (0, 5))
        tr = oracle.Tracker(np.ascontiguousarray(sc['goal'][:, :3]), sc['goal'][:, 3:6], np.ones(m), sc['zaxis'])
        radius, ps, goal = np.full(m, 0.5), np.ones(m), np.ascontiguousarray(sc['goal'][:, :3])
        rows = []
        for t in range(steps):
            if stop_when_done and (r['flags'] & 7).all():
                rows.append(None)
                continue
            active = ((r['flags'] & 7) == 0) & ext
            vp = tr.vpref(r['pos'], r['vel'], r['head'], active.astype(np.uint8), nthreads=16)
            p = oracle.policy_step(r['pos'], r['vel'], r['head'], radius, ps, r['flags'], goal, sc['policy'], sc['zaxis'], vp, ext.astype(np.uint8),
                                   r['perm'], obs_pos, obs_radius, nthreads=16)
            tr.note_neighbors(p['nbr_valid'], p['nbr_n'], p['nbr_dsq'])
            u = oracle.env_update(r['pos'], r['vel'], r['head'], radius, p['flags'], goal, p['action'], r['td'], sc['mrd'], r['sn'], obs_pos, obs_radius)
            r = dict(pos=u['pos'], vel=u['vel'], head=u['heading'], flags=u['flags'], td=u['total_dist'], sn=u['step_num'], perm=p['perm'])
            rows.append(dict(r, p=p, active=active))
        out.append(dict(steps=rows, last=r, ext=ext, replans=tr.replans()))
        tr.close()
    _ORACLE_RUNS[key] = out
    return out
