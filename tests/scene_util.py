"""Helpers of the scene tests (tests/test_gpu_scene*.py).  load_any, everything and assert_scene_equals_alone serve all of them; Slots is
test_gpu_scene_restart.py's: recorded episodes as the slots of one context, where a slot may be given another recorded episode while the
batch runs (sca_restart_scenes).  Every slot is held against the reference's records of the episode it holds AT THAT MOMENT, counted from
the step the episode was put in."""
import os

import numpy as np

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
