"""Scene batches (-m gpu): many isolated episodes stepped by ONE context (sca_set_scenes).  The bar is the contract's: for every scene every
value the context produces -- state, float32 action rows, diagnostics, kd permutation, what the device tracker and the waypoint lists leave --
is bit for bit what a context holding that scene alone produces, i.e. the reference's.  Batches 1-4 rest on reference-recorded episodes
only: free-running from the scenario's start state, nothing fed from the fixtures, every scene compared after every step it has a record
of.  No tolerance anywhere."""
import math

import numpy as np
import pytest

from golden_util import fixture_agent_params, fixture_params, fixture_tracker_agent_params, static_inputs
from scene_util import load_any, oracle_scene_runs, random_scenes

pytestmark = pytest.mark.gpu

BATCH1 = ['F1_sca_circle8'] + ['F2_%s_circle100' % p for p in ('orca', 'orcalp', 'rvo', 'rvodubins', 'sca', 'srvo')] + \
         ['F3_%s_random100' % p for p in ('orca', 'orcalp', 'rvo', 'srvo')] + ['F3_orcalp_sphere100', 'F3_srvo_sphere100', 'F15_sca_circle1024']
BATCH2 = ['F4_mixed_takeoff16', 'F4_sca_takeoff16', 'F4_sca_circle16_obs', 'F16_params_pitch30', 'F18_hetero_track_takeoff16']
BATCH3 = ['paths/F19_path_%s' % p for p in ('edge10', 'orcalp_random30', 'rvo_circle16', 'srvo_circle16')]
# the reference's defaults (agent.py:24-41): what a scene recorded at the defaults holds in a batch that carries the attributes per agent
DEFAULTS = dict(neighbor_dist=10.0, max_neighbors=16, time_step=0.1, time_horizon=10.0, max_speed=1.0, max_heading_change=math.pi / 4, dt_nominal=0.1)
TRK_DEFAULTS = dict(turning_radius=1.5, pitch_lo=-math.pi / 4, pitch_hi=math.pi / 4)


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


class Batch:
    """B recorded episodes in one context, each a scene; `sol` is stepped from the start states."""

    def __init__(self, S, names, scenes=True, tracker=True):
        self.S, self.names = S, list(names)
        self.fx = [load_any(n) for n in self.names]
        self.st = [static_inputs(f) for f in self.fx]
        sizes = [len(s['radius']) for s in self.st]
        self.off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        self.n, self.B = int(self.off[-1]), len(self.names)
        cat = lambda key: np.concatenate([s[key] for s in self.st])
        with_obs = [s for s in self.st if len(s['obs_radius'])]
        self.obs_pos = with_obs[0]['obs_pos'] if with_obs else np.zeros((0, 3))
        self.obs_radius = with_obs[0]['obs_radius'] if with_obs else np.zeros(0)
        for s in self.st:                                          # obstacles are shared: every scene of a batch has the same, or none in a batch without
            assert np.array_equal(s['obs_pos'], self.obs_pos) and np.array_equal(s['obs_radius'], self.obs_radius)
        self.start = np.concatenate([f['start'] for f in self.fx])
        self.goal6 = np.concatenate([f['goal6'] for f in self.fx])
        self.ext = cat('vpref_mode').astype(bool)
        sol = self.sol = S.BatchedSolver(max_agents=self.n, max_obstacles=max(len(self.obs_radius), 1))
        sol.set_obstacles(self.obs_pos, self.obs_radius)
        sol.set_agents(cat('radius'), cat('pref_speed'), np.concatenate([f['goal'][0] for f in self.fx]), cat('policy'), cat('zaxis'), cat('max_run_dist'))
        # scene-wide (F16) and per-agent (F17 / F18) attributes, expanded to one array per attribute over the whole batch
        if any(fixture_params(f)[0] or fixture_agent_params(f) for f in self.fx):
            arrays = {}
            for key, dflt in DEFAULTS.items():
                parts = []
                for f, size in zip(self.fx, sizes):
                    own = fixture_agent_params(f).get(key)
                    parts.append(np.asarray(own) if own is not None else np.full(size, fixture_params(f)[0].get(key, dflt)))
                arrays[key] = np.concatenate(parts).astype(np.int32 if key == 'max_neighbors' else np.float64)
            sol.set_agent_params(**arrays)
        if scenes:
            sol.set_scenes(self.off)
        if tracker and self.ext.any():
            sol.device_tracker_enable(self.goal6[:, 3:6], in_pass=True)
            if any(fixture_params(f)[1] or fixture_tracker_agent_params(f) for f in self.fx):
                arrays = {}
                for key, dflt in TRK_DEFAULTS.items():
                    parts = []
                    for f, size in zip(self.fx, sizes):
                        own = fixture_tracker_agent_params(f).get(key)
                        t = fixture_params(f)[1]
                        scene = {'turning_radius': t.get('turning_radius'), 'pitch_lo': t['pitchlims'][0] if t else None,
                                 'pitch_hi': t['pitchlims'][1] if t else None}[key]
                        parts.append(np.asarray(own) if own is not None else np.full(size, dflt if scene is None else scene))
                    arrays[key] = np.concatenate(parts)
                sol.device_tracker_set_agent_params(**arrays)
        self.paths = any('path_off' in f for f in self.fx)
        if self.paths:
            lists = []
            for f, size in zip(self.fx, sizes):
                if 'path_off' in f:
                    lists += [[list(map(float, w)) for w in f['path_pts'][f['path_off'][i]:f['path_off'][i + 1]]] for i in range(size)]
                else:
                    lists += [[] for _ in range(size)]
            sol.set_paths(lists)
        self.reset()

    def reset(self):
        n = self.n
        self.sol.set_state(self.start[:, :3], np.zeros((n, 3), np.float32), self.start[:, 3:6], np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.int32))
        self.sol.set_kd_perm(np.arange(n, dtype=np.int32))
        self.index = [{int(t): k for k, t in enumerate(f['step'])} for f in self.fx]
        self.done_step = [int(f['done_step']) if 'done_step' in f else -1 for f in self.fx]

    def sl(self, s):
        return slice(int(self.off[s]), int(self.off[s + 1]))

    def snapshot(self):
        sol = self.sol
        out = dict(state=sol.get_state(), perm=sol.get_kd_perm())
        if self.paths:
            out['rem'], out['now_goal'] = sol.get_path_state()
        return out

    def check_state(self, snap, s, k, when, ctx):
        """scene s against record k of its fixture: `when` = '' (what the step started from) or '_after'"""
        f, sl, lo = self.fx[s], self.sl(s), int(self.off[s])
        ctx = ctx + (self.names[s], 'record', k, when or 'before')
        for key in ('pos', 'heading', 'total_dist', 'flags'):
            assert np.array_equal(snap['state'][key][sl], f[key + when][k]), ctx + (key,)
        assert np.array_equal(snap['state']['vel'][sl][:, :3], f['vel' + when][k]), ctx + ('vel',)
        assert np.array_equal(snap['perm'][sl] - lo, f['perm' + when][k]), ctx + ('perm',)
        if 'path_off' in f:
            w = '_after' if when else '_before'
            assert np.array_equal(snap['rem'][sl], f['path_left' + w][k]), ctx + ('path_left',)
            assert np.array_equal(snap['now_goal'][sl], f['now_goal' + w][k], equal_nan=True), ctx + ('now_goal',)

    def run_and_check(self, steps, step_fn=None, compare_at=None, label=''):
        """`steps` steps, one per call of step_fn (default sca_run_steps); every scene that has a record of a step is compared before and after
        it (compare_at: only at these steps); a scene beyond its `done` stays what its last record left, its action rows zero; the
        per-scene counters follow the flags.  Returns the number of (scene, step) records compared."""
        S, sol = self.S, self.sol
        step_fn = step_fn or (lambda: (sol.run_steps(1, S.NBR_KDTREE), sol.synchronize()))
        snap = self.snapshot()
        steps_want = np.zeros(self.B, np.int64)
        compared = 0
        for t in range(steps):
            look = compare_at is None or t in compare_at
            ctx = (label, 'step', t)
            live_before = np.array([((snap['state']['flags'][self.sl(s)] & 7) == 0).sum() for s in range(self.B)])
            if look:
                for s in range(self.B):
                    if t in self.index[s]:
                        self.check_state(snap, s, self.index[s][t], '', ctx)
            step_fn()
            steps_want += live_before > 0
            snap = self.snapshot()
            if not look:
                continue
            a, status = sol.actions(), sol.diag()['status']
            assert sol.pass_forms() & S.FORM_SCENES, ctx
            for s in range(self.B):
                sl = self.sl(s)
                if t in self.index[s]:
                    k, f = self.index[s][t], self.fx[s]
                    called = f['called'][k].astype(bool)
                    assert np.array_equal(a[sl][called], f['action'][k][called]), ctx + (self.names[s], 'action')
                    assert not status[sl].any(), ctx + (self.names[s], 'status')
                    self.check_state(snap, s, k, '_after', ctx)
                    compared += 1
                elif 0 <= self.done_step[s] < t:                   # finished: inert
                    self.check_state(snap, s, len(self.fx[s]['step']) - 1, '_after', ctx + ('inert',))
                    assert not a[sl].any(), ctx + (self.names[s], 'action rows of a finished scene')
            live = np.array([((snap['state']['flags'][self.sl(s)] & 7) == 0).sum() for s in range(self.B)])
            sc = sol.scene_state()
            assert np.array_equal(sc['active'], live), ctx + ('active', sc['active'].tolist(), live.tolist())
            assert np.array_equal(sc['steps'], steps_want), ctx + ('steps', sc['steps'].tolist(), steps_want.tolist())
            assert sol.active_count() == int(live.sum()), ctx
        return compared


def test_batch1_all_six_policies_without_obstacles(S):
    """14 scenes, 2232 agents; the six F2 scenes start on the same coordinates: a leak between scenes shows at step 1.  260 steps: F1 is done at
    245 (246 steps) and stays inert while the others go on."""
    b = Batch(S, BATCH1)
    assert b.n == 2232 and b.B == 14
    compared = b.run_and_check(260, label='batch1')
    assert compared == 246 + 5 * 40 + 12 + 6 * 25 + 4
    sc = b.sol.scene_state()
    assert sc['steps'][0] == 246 and sc['active'][0] == 0
    b.sol.close()


def test_batch2_shared_obstacles_and_per_agent_attributes(S):
    """the same 8 obstacles for five scenes; F16 / F18 bring scene-wide and per-agent solver and planner attributes, passed per agent.  Three
    scenes finish, at different steps; the total is 0 only after the last."""
    b = Batch(S, BATCH2)
    totals = []
    compared = b.run_and_check(331, step_fn=lambda: totals.append(b.sol.env_step(S.NBR_KDTREE)), label='batch2')
    assert compared == 331 + 285 + 100 + 60 + 60
    sc = b.sol.scene_state()
    assert sc['steps'][:3].tolist() == [331, 285, 289] and not sc['active'][:3].any()
    assert all(v > 0 for v in totals[:288])                        # (F16 / F18 are recorded for 60 steps and fly on)
    b.sol.close()


def test_batch3_waypoint_lists(S):
    b = Batch(S, BATCH3)
    longest = max(int(f['step'][-1]) for f in b.fx) + 1
    compared = b.run_and_check(longest, label='batch3')
    assert compared == sum(len(f['step']) for f in b.fx)
    assert b.sol.pass_forms() & S.FORM_WAYPOINTS
    b.sol.close()


def test_order_of_the_scenes_does_not_matter(S):
    b = Batch(S, BATCH1[::-1])
    assert b.run_and_check(41, label='reversed') == 41 + 5 * 40 + 12 + 6 * 25 + 4
    b.sol.close()


def test_560_scenes_packed_query_and_strided_forest(S):
    """batch 1 forty times: 89 280 agents (the packed K1 form), 560 forest jobs; every copy against the fixtures -- hence equal to copy 0 -- at
    steps 1, 2, 3, 4 and 40"""
    b = Batch(S, BATCH1 * 40)
    assert b.n == 89280 and b.B == 560
    compared = b.run_and_check(40, compare_at={0, 1, 2, 3, 39}, label='x40')
    assert compared == 40 * (4 * 14 + 6)                           # (at step 40: F1 and the five F2 scenes recorded for 40 steps)
    st, perm = b.sol.get_state(), b.sol.get_kd_perm()
    for c in range(1, 40):
        lo = c * 2232
        for key in st:
            assert np.array_equal(st[key][lo:lo + 2232], st[key][:2232]), (c, key)
        assert np.array_equal(perm[lo:lo + 2232] - lo, perm[:2232]), c
    b.sol.close()


@pytest.mark.parametrize('packed', [0, 1])
def test_random_scenes_against_the_oracle(S, oracle, packed, monkeypatch):
    """64 seeded scenes of sizes at the leaf boundary, the block instances' edges and the cap, mixed policies, shared obstacles, 6 free-running
    steps: every scene against the oracle run on that scene alone (policy_step / env_update / Tracker), equality.  In both K1 scene forms:
    the 6884 agents are a packed pass by default (k_neighbors_kd4_scenes: the scenes of 1, 2 and 3 agents share their wavefront with other
    scenes' groups), SCA_K1_PACKED=0 sends them through k_neighbors_kd_scenes."""
    monkeypatch.setenv('SCA_K1_PACKED', str(packed))                 # read by sca_create
    scenes, sizes, obs_pos, obs_radius = random_scenes(S)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(off[-1])
    cat = lambda key: np.concatenate([sc[key] for sc in scenes])
    start, goal6, policy = cat('start'), cat('goal'), cat('policy')
    sol = S.BatchedSolver(max_agents=n, max_obstacles=6)
    sol.set_obstacles(obs_pos, obs_radius)
    sol.set_agents(np.full(n, 0.5), np.ones(n), goal6[:, :3], policy, cat('zaxis'), cat('mrd'))
    sol.set_scenes(off)
    sol.device_tracker_enable(goal6[:, 3:6], in_pass=True)
    sol.set_state(start[:, :3], np.zeros((n, 3), np.float32), start[:, 3:6], np.zeros(n, np.uint8))
    ref = oracle_scene_runs(oracle, 'shared obstacles', scenes, [(obs_pos, obs_radius)] * len(scenes))
    for t in range(6):
        sol.run_steps(1, S.NBR_KDTREE)
        sol.synchronize()
        g, a, vd, perm, nb = sol.get_state(), sol.actions(), sol.diag()['vpref'], sol.get_kd_perm(), sol.neighbors()
        for s, sc in enumerate(scenes):
            m, sl, lo = sc['n'], slice(int(off[s]), int(off[s + 1])), int(off[s])
            r = ref[s]['steps'][t]
            p, active = r['p'], r['active']
            ctx = ('scene', s, 'size', m, 'step', t)
            assert np.array_equal(a[sl], p['action']), ctx + ('action',)
            valid = p['nbr_valid'].astype(bool)
            assert np.array_equal(nb['nbr_valid'][sl].astype(bool), valid), ctx
            assert np.array_equal(nb['nbr_n'][sl][valid], p['nbr_n'][valid]), ctx + ('nbr_n',)
            ids = nb['nbr_id'][sl] - np.where((nb['nbr_kind'][sl] == 0) & (nb['nbr_id'][sl] >= 0), lo, 0)       # agents: global ids
            assert np.array_equal(ids[valid], p['nbr_id'][valid]), ctx + ('nbr_id',)
            assert np.array_equal(nb['nbr_kind'][sl][valid], p['nbr_kind'][valid]), ctx + ('nbr_kind',)
            assert np.array_equal(nb['nbr_dsq'][sl][valid], p['nbr_dsq'][valid]), ctx + ('nbr_dsq',)
            assert np.array_equal(vd[sl][active], p['vpref'][active]), ctx + ('vpref',)
            assert np.array_equal(perm[sl] - lo, r['perm']), ctx + ('perm',)
            for key, want in (('pos', r['pos']), ('vel', r['vel']), ('heading', r['head']), ('flags', r['flags']), ('total_dist', r['td']), ('step_num', r['sn'])):
                assert np.array_equal(g[key][sl], want), ctx + (key,)
    rd = sol.device_tracker_replans()
    for s, r in enumerate(ref):
        sl = slice(int(off[s]), int(off[s + 1]))
        assert np.array_equal(rd[sl][r['ext']], r['replans'][r['ext']]), ('re-plans', s)
    sol.close()


def test_entry_points_agree(S):
    """batch 2 through sca_env_step, sca_step_host and sca_policy_pass + sca_env_update: each loop's states, action rows, permutation and
    per-scene counters equal the sca_run_steps loop's"""
    ref = Batch(S, BATCH2)
    others = dict(env_step=Batch(S, BATCH2), step_host=Batch(S, BATCH2), pass_update=Batch(S, BATCH2))
    h = others['step_host'].sol.host_state()
    for k in ('pos', 'heading', 'flags', 'total_dist', 'step_num', 'vel'):
        h[k][...] = ref.sol.get_state()[k]
    for t in range(40):
        ref.sol.run_steps(1, S.NBR_KDTREE)
        ref.sol.synchronize()
        want = ref.snapshot()
        want_actions, want_sc = ref.sol.actions(), ref.sol.scene_state()
        total = int(want_sc['active'].sum())
        assert others['env_step'].sol.env_step(S.NBR_AUTO) == total                    # (AUTO resolves to the scene form)
        assert others['step_host'].sol.step_host(S.NBR_KDTREE, state=(t == 0)) == total
        others['pass_update'].sol.policy_pass(S.NBR_KDTREE)
        assert others['pass_update'].sol.env_update() == (total == 0)
        for name, b in others.items():
            got = b.snapshot()
            for key in want['state']:
                assert np.array_equal(got['state'][key], want['state'][key]), (name, t, key)
            assert np.array_equal(got['perm'], want['perm']), (name, t)
            assert np.array_equal(b.sol.actions(), want_actions), (name, t)
            sc = b.sol.scene_state()
            assert np.array_equal(sc['active'], want_sc['active']) and np.array_equal(sc['steps'], want_sc['steps']), (name, t)
            assert b.sol.pass_forms() & S.FORM_SCENES, name
        for key in ('pos', 'heading', 'flags', 'total_dist', 'step_num'):
            assert np.array_equal(h[key], want['state'][key]), ('host block', t, key)
        assert np.array_equal(h['action'], want_actions), ('host block', t)
    for b in list(others.values()) + [ref]:
        b.sol.close()


def test_set_state_and_perm_mid_episode(S):
    """fed from the fixtures' step 20 (state, permutation in global ids), the batch goes on as the recorded episodes do"""
    b = Batch(S, ['F2_orca_circle100', 'F3_srvo_random100', 'F2_rvo_circle100'])
    k = 20
    cat = lambda key: np.concatenate([f[key][k] for f in b.fx])
    b.sol.set_state(cat('pos'), cat('vel'), cat('heading'), cat('flags'), cat('total_dist'))
    b.sol.set_kd_perm(np.concatenate([f['perm'][k] + int(lo) for f, lo in zip(b.fx, b.off[:-1])]))
    for t in range(k, 25):
        b.sol.run_steps(1, S.NBR_KDTREE)
        b.sol.synchronize()
        snap = b.snapshot()
        for s in range(b.B):
            b.check_state(snap, s, t, '_after', ('mid-episode', t))
    sc = b.sol.scene_state()
    assert np.array_equal(sc['steps'], np.full(b.B, 5)) and (sc['active'] > 0).all()
    b.sol.close()


def _plain(S, n=40, pol=1, seed=3):
    from sca_amd import scenarios
    sc = scenarios.random_cube(n, seed=seed)
    sol = S.BatchedSolver(max_agents=2000, max_obstacles=1)
    sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))

    def agents(m=n, scn=None):
        scn = sc if m == n else scenarios.random_cube(m, seed=seed)
        sol.set_agents(np.full(m, 0.5), np.ones(m), scn['goal'][:, :3], np.full(m, pol, np.uint8), S.zaxis_flags(scn['start'], scn['goal']),
                       scenarios.max_run_dist(scn['start'], scn['goal']))
        return scn

    def state(scn=sc):
        m = len(scn['start'])
        sol.set_state(scn['start'][:, :3], np.zeros((m, 3), np.float32), scn['start'][:, 3:6], np.zeros(m, np.uint8))
    return sol, sc, agents, state


def test_refusals_leave_the_context_usable(S):
    sol, sc, agents, state = _plain(S)
    rc = lambda fn, *a: fn(sol.ctx, *a)
    import ctypes as C
    from sca_amd import _lib
    off = np.array([0, 15, 40], np.int32)
    p = lambda a: _lib.ptr(a, C.c_int32)
    assert rc(sol.L.sca_set_scenes, 2, p(off)) == -3                        # SCA_ERR_STATE: before sca_set_agents
    agents(); state()
    for bad in ([0, 15, 15, 40], [0, 20, 15, 40], [1, 15, 40], [0, 15, 39], [0, 15, 41]):
        a = np.array(bad, np.int32)
        assert rc(sol.L.sca_set_scenes, len(a) - 1, p(a)) == -1, bad          # SCA_ERR_ARG
    sol.set_scenes(off)
    sol.set_scenes(off)                                                       # twice: the same thing again
    sol.set_scenes(np.array([0, 10, 20, 40], np.int32))
    sol.set_scenes(off)
    one = C.c_int(0)
    assert rc(sol.L.sca_policy_pass, S.NBR_GRID) == -5 and rc(sol.L.sca_policy_pass, S.NBR_KDTREE_HOSTBUILD) == -5
    assert rc(sol.L.sca_run_steps, 1, S.NBR_GRID) == -5 and rc(sol.L.sca_env_step, S.NBR_KDTREE_HOSTBUILD, C.byref(one)) == -5
    assert rc(sol.L.sca_set_shard, 0, 20) == -5 and rc(sol.L.sca_set_shard, 0, 40) == 0
    tree = np.zeros((79, 10))
    assert rc(sol.L.sca_get_kd_tree, _lib.ptr(tree, C.c_double)) == -5
    assert rc(sol.L.sca_partition_init, 0, 1, 0, None, 0, 0) == -5
    assert rc(sol.L.sca_comm_init, 0, 1, C.create_string_buffer(128)) == -5
    perm = np.arange(40, dtype=np.int32); perm[[14, 15]] = perm[[15, 14]]
    assert rc(sol.L.sca_set_kd_perm, p(perm)) == -1
    assert b'scene' in sol.L.sca_last_error(sol.ctx)
    # still usable: the batch steps, and equals two contexts of one scene each
    sol.run_steps(5, S.NBR_KDTREE); sol.synchronize()
    got = sol.get_state()
    assert sol.pass_forms() & S.FORM_SCENES
    from sca_amd import scenarios
    for lo, hi in ((0, 15), (15, 40)):
        alone = S.BatchedSolver(max_agents=hi - lo, max_obstacles=1)
        alone.set_obstacles(np.zeros((0, 3)), np.zeros(0))
        alone.set_agents(np.full(hi - lo, 0.5), np.ones(hi - lo), sc['goal'][lo:hi, :3], np.full(hi - lo, 1, np.uint8),
                         S.zaxis_flags(sc['start'][lo:hi], sc['goal'][lo:hi]), scenarios.max_run_dist(sc['start'][lo:hi], sc['goal'][lo:hi]))
        alone.set_state(sc['start'][lo:hi, :3], np.zeros((hi - lo, 3), np.float32), sc['start'][lo:hi, 3:6], np.zeros(hi - lo, np.uint8))
        alone.run_steps(5, S.NBR_KDTREE); alone.synchronize()
        st = alone.get_state()
        for key in st:
            assert np.array_equal(got[key][lo:hi], st[key]), (lo, key)
        assert np.array_equal(sol.get_kd_perm()[lo:hi] - lo, alone.get_kd_perm())
        alone.close()
    # a scene of 1537 agents
    big = agents(1537)
    assert rc(sol.L.sca_set_scenes, 1, p(np.array([0, 1537], np.int32))) == -5
    assert b'1536' in sol.L.sca_last_error(sol.ctx)
    state(big)
    sol.run_steps(1, S.NBR_KDTREE); sol.synchronize()
    assert not sol.pass_forms() & S.FORM_SCENES
    sol.close()


def test_set_agents_clears_the_scenes(S):
    sol, sc, agents, state = _plain(S)
    agents(); state()
    sol.set_scenes(np.array([0, 15, 40], np.int32))
    sol.run_steps(3, S.NBR_KDTREE); sol.synchronize()
    assert sol.pass_forms() & S.FORM_SCENES
    agents(); state()
    fresh, _, fagents, fstate = _plain(S)
    fagents(); fstate()
    for s in (sol, fresh):
        s.run_steps(6, S.NBR_KDTREE); s.synchronize()
    assert not sol.pass_forms() & S.FORM_SCENES
    a, b = sol.get_state(), fresh.get_state()
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(sol.get_kd_perm(), fresh.get_kd_perm()) and np.array_equal(sol.actions(), fresh.actions())
    assert sol.L.sca_get_scene_state(sol.ctx, None, None) == -3
    # ... and so does sca_set_scenes(0, NULL)
    sol.set_scenes(np.array([0, 15, 40], np.int32))
    sol.set_scenes(None)
    sol.run_steps(1, S.NBR_KDTREE); sol.synchronize()
    assert not sol.pass_forms() & S.FORM_SCENES
    sol.close(); fresh.close()


def test_scene_batch_equals_separate_envs(S):
    """SceneBatch of three circle scenes (different policies and sizes, one with device-tracker agents) against three MACAEnv loops"""
    from sca_amd import env as E, metrics
    from sca_amd.scenes import SceneBatch
    spec = [(E.RVO3DPolicy, 12), (E.SCAPolicy, 20), (E.ORCA3DPolicy, 7)]
    batch = SceneBatch([E.build_circle_agents(n, policy=p) for p, n in spec], [], device_tracker=True)
    loops = 0
    while not batch.step() and loops < 5000:
        loops += 1
    assert batch.done.all()
    for s, (p, n) in enumerate(spec):
        env = E.MACAEnv(device_tracker=True)
        env.set_agents(E.build_circle_agents(n, policy=p), obstacles=[])
        count = 1
        while not env.step({}):
            count += 1
        view = batch.env(s)
        assert int(batch.steps[s]) == count == view.steps, (s, int(batch.steps[s]), count)
        for key in ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num'):
            assert np.array_equal(getattr(view, key), getattr(env, key)), (s, key)
        for a, b in zip(view.agents, env.agents):
            assert np.array_equal(a.pos_global_frame, b.pos_global_frame) and a.is_at_goal == b.is_at_goal and a.total_dist == b.total_dist
        assert view.kdTree.agentIDs == env.kdTree.agentIDs
        ma, mb = metrics.episode_metrics(view), metrics.episode_metrics(env)
        assert set(ma) == set(mb)
        for key in ma:
            if key != 'AverageCost':                                # a wall time
                assert ma[key] == mb[key] or (ma[key] != ma[key] and mb[key] != mb[key]), (s, key, ma[key], mb[key])
        assert metrics.episode_info(view)['all_agent_info'] == metrics.episode_info(env)['all_agent_info']
        env.solver.close()
    batch.close()
