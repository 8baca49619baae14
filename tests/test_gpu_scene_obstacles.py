"""Per-scene obstacle sets (-m gpu): sca_set_scene_obstacles gives every scene of a batch its own obstacles.  The bar is the scene contract
extended to obstacles: for every scene every value the context produces -- state, float32 action rows, neighbour lists and their distSq,
diagnostics, kd permutation, what the device tracker and the waypoint lists leave -- is bit for bit what a context holding that scene alone
with that obstacle set produces, i.e. the reference's.  Tests 1 and 2 rest on reference-recorded episodes only, free-running from the start
states.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_parity as TP
import test_gpu_scenes as TS
from golden_util import fixture_agent_params, fixture_params, fixture_tracker_agent_params, static_inputs
from scene_util import agents_of, assert_scene_equals_alone, everything, load_any, oracle_scene_runs, random_scenes, same

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3                                      # include/sca_hip.h
PATH_OBS = 'paths/F19_path_orca_circle16_obs'


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


def reference_names():
    """every free-running recorded episode (tests/test_gpu_parity.py) plus the waypoint episode among obstacles"""
    return TP._free_running_fixtures() + [PATH_OBS]


class ObsBatch(TS.Batch):
    """B recorded episodes in one context, each a scene WITH ITS OWN RECORDED OBSTACLES (tests/test_gpu_scenes.py::Batch shares one set);
    mode: 'scene' = sca_set_scene_obstacles, 'none' = leave the context without obstacles"""

    def __init__(self, S, names, tracker=True, mode='scene'):
        self.S, self.names = S, list(names)
        self.fx = [load_any(n) for n in self.names]
        self.st = [static_inputs(f) for f in self.fx]
        sizes = [len(s['radius']) for s in self.st]
        self.off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        self.n, self.B = int(self.off[-1]), len(self.names)
        cat = lambda key: np.concatenate([s[key] for s in self.st])
        self.obs = [(s['obs_pos'].reshape(-1, 3), s['obs_radius']) for s in self.st]
        self.obs_off = np.concatenate([[0], np.cumsum([len(r) for _, r in self.obs])]).astype(np.int32)
        self.start = np.concatenate([f['start'] for f in self.fx])
        self.goal6 = np.concatenate([f['goal6'] for f in self.fx])
        self.ext = cat('vpref_mode').astype(bool)
        sol = self.sol = S.BatchedSolver(max_agents=self.n, max_obstacles=max(int(self.obs_off[-1]), 1))
        sol.set_agents(cat('radius'), cat('pref_speed'), np.concatenate([f['goal'][0] for f in self.fx]), cat('policy'), cat('zaxis'), cat('max_run_dist'))
        if any(fixture_params(f)[0] or fixture_agent_params(f) for f in self.fx):
            arrays = {}
            for key, dflt in TS.DEFAULTS.items():
                parts = []
                for f, size in zip(self.fx, sizes):
                    own = fixture_agent_params(f).get(key)
                    parts.append(np.asarray(own) if own is not None else np.full(size, fixture_params(f)[0].get(key, dflt)))
                arrays[key] = np.concatenate(parts).astype(np.int32 if key == 'max_neighbors' else np.float64)
            sol.set_agent_params(**arrays)
        sol.set_scenes(self.off)
        if mode == 'scene':
            sol.set_scene_obstacles(self.obs)
        if tracker and self.ext.any():
            sol.device_tracker_enable(self.goal6[:, 3:6], in_pass=True)
            if any(fixture_params(f)[1] or fixture_tracker_agent_params(f) for f in self.fx):
                arrays = {}
                for key, dflt in TS.TRK_DEFAULTS.items():
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
        super().reset()
        # run_and_check holds a finished scene against its LAST record; a sampled fixture whose last record is not its final step (the
        # waypoint episode: done at 327, recorded every other step up to 326) has no record of that state -- see still_after_done
        self.done_step = [d if d == int(f['step'][-1]) else -1 for d, f in zip(self.done_step, self.fx)]

    def records_up_to(self, steps, at=None):
        """(scene, step) records the fixtures hold for steps 0 .. steps - 1 (at: only these steps), from their `step` arrays"""
        return sum(int(sum(1 for t in f['step'] if int(t) < steps and (at is None or int(t) in at))) for f in self.fx)


def test_the_reference_set():
    """what the batch below consists of: 22 episodes among obstacles (their recorded sets: 17 distinct ones of 1 .. 1491 obstacles -- six
    episodes share the take-off field's 8 spheres) and the obstacle-free ones"""
    names = reference_names()
    fx = [load_any(n) for n in names]
    with_obs = [n for n, f in zip(names, fx) if len(f['obs_radius'])]
    assert len(with_obs) == 22
    assert len({(f['obs_pos'].tobytes(), f['obs_radius'].tobytes()) for f in fx if len(f['obs_radius'])}) == 17
    assert sorted({len(f['obs_radius']) for f in fx}) == [0, 1, 2, 3, 4, 5, 8, 1491]
    for want in (['F10_sca_exp3_map'] + ['F13_fuzz_track_%02d' % k for k in range(4)] + ['F14_fuzz_episode_%02d' % k for k in range(3)] +
                 ['F9_hetero_mixed60', 'F4_mixed_takeoff16', 'F4_sca_takeoff16', 'F4_sca_circle16_obs', PATH_OBS]):
        assert want in with_obs, want
    assert sum(n.startswith('F16_params_') for n in with_obs) == 5
    assert sum(n.startswith('F17_') for n in with_obs) == 2 and sum(n.startswith('F18_') for n in with_obs) == 2
    free = [n for n in names if n not in with_obs]
    for prefix in ('F1_', 'F2_', 'F3_', 'F15_'):
        assert any(n.startswith(prefix) for n in free), prefix
    f10 = fx[names.index('F10_sca_exp3_map')]
    assert len(f10['obs_radius']) == 1491 and len(f10['step']) == 160
    assert max(len(f['step']) for f in fx) == 331


def test_reference_only_batch_every_scene_its_own_recorded_obstacles(S):
    """every free-running recorded episode in ONE context, each with its own recorded obstacles, from the start states, 331 steps (the longest
    record): every scene against every record it has of those steps, before and after the step; finished scenes inert; per-scene counters"""
    b = ObsBatch(S, reference_names())
    assert b.B == 46 and int(b.obs_off[-1]) == sum(len(r) for _, r in b.obs) > 1491
    compared = b.run_and_check(331, label='reference batch')
    assert compared == b.records_up_to(331)
    assert compared >= 331 + 285 + 160                              # (F4_mixed_takeoff16 whole, F4_sca_takeoff16 whole, F10 whole, ...)
    assert b.sol.pass_forms() & S.FORM_SCENE_OBSTACLES and b.sol.pass_forms() & S.FORM_SCENES
    assert b.sol.pass_forms() & S.FORM_WAYPOINTS
    # the waypoint episode among obstacles finished at step 327, past its last record: inert since then
    s = b.names.index(PATH_OBS)
    assert int(b.fx[s]['done_step']) == 327 and b.sol.scene_state()['steps'][s] == 328 and b.sol.scene_state()['active'][s] == 0
    before = b.snapshot()
    b.sol.run_steps(2, S.NBR_KDTREE)
    b.sol.synchronize()
    after = b.snapshot()
    for key in before['state']:
        assert np.array_equal(before['state'][key][b.sl(s)], after['state'][key][b.sl(s)]), ('inert', key)
    assert np.array_equal(before['perm'][b.sl(s)], after['perm'][b.sl(s)]) and not b.sol.actions()[b.sl(s)].any()
    b.sol.close()


def test_packed_form_reversed_and_replicated(S):
    """the same batch in reverse order, as many copies as make 6144 agents (the packed query form, four agents per wavefront): steps 0-3
    and 39 against the fixtures, every copy against copy 0"""
    names = reference_names()[::-1]
    one = sum(len(load_any(n)['radius']) for n in names)
    copies = -(-6144 // one)
    b = ObsBatch(S, names * copies)
    assert b.n == one * copies >= 6144 and copies >= 2
    at = {0, 1, 2, 3, 39}
    compared = b.run_and_check(40, compare_at=at, label='packed')
    assert compared == b.records_up_to(40, at) and compared >= copies * 4 * len(names)
    assert b.sol.pass_forms() & S.FORM_SCENE_OBSTACLES
    st, perm = b.sol.get_state(), b.sol.get_kd_perm()
    a, nb = b.sol.actions(), b.sol.neighbors()
    m_one = int(b.obs_off[len(names)])
    for c in range(1, copies):
        lo = c * one
        for key in st:
            assert np.array_equal(st[key][lo:lo + one], st[key][:one]), (c, key)
        assert np.array_equal(perm[lo:lo + one] - lo, perm[:one]), c
        assert np.array_equal(a[lo:lo + one], a[:one]), c
        ids, kind = nb['nbr_id'][lo:lo + one], nb['nbr_kind'][lo:lo + one]
        local = ids - np.where(ids >= 0, np.where(kind == 1, c * m_one, lo), 0)
        assert np.array_equal(local, nb['nbr_id'][:one]) and np.array_equal(nb['nbr_dsq'][lo:lo + one], nb['nbr_dsq'][:one]), c
    b.sol.close()


def _scene_dict(S, start, goal, policy):
    from sca_amd import scenarios
    n = len(start)
    return dict(start=start, goal=goal, policy=np.broadcast_to(np.asarray(policy, np.uint8), (n,)).copy(), zaxis=S.zaxis_flags(start, goal),
                mrd=scenarios.max_run_dist(start, goal), n=n)


def _context(S, scenes, obstacles, mode='scene', max_obstacles=None, tracker=True):
    """scenes: dicts of _scene_dict; obstacles: one (pos, radius) per scene ('scene'), or one pair for all ('shared'), or nothing ('none')"""
    off = np.concatenate([[0], np.cumsum([sc['n'] for sc in scenes])]).astype(np.int32)
    n = int(off[-1])
    cat = lambda key: np.concatenate([sc[key] for sc in scenes])
    start, goal6 = cat('start'), cat('goal')
    total = sum(len(r) for _, r in obstacles) if mode == 'scene' else (len(obstacles[1]) if mode == 'shared' else 0)
    sol = S.BatchedSolver(max_agents=n, max_obstacles=max(total, 1) if max_obstacles is None else max_obstacles)
    if mode == 'shared':
        sol.set_obstacles(*obstacles)
    sol.set_agents(np.full(n, 0.5), np.ones(n), goal6[:, :3], cat('policy'), cat('zaxis'), cat('mrd'))
    if len(scenes) > 1 or mode == 'scene':
        sol.set_scenes(off)
    if mode == 'scene':
        sol.set_scene_obstacles(obstacles)
    if tracker:
        sol.device_tracker_enable(goal6[:, 3:6], in_pass=True)
    sol.set_state(start[:, :3], np.zeros((n, 3), np.float32), start[:, 3:6], np.zeros(n, np.uint8))
    return sol, off


def test_obstacles_do_not_leak_between_scenes(S):
    """three scenes with identical agents: obstacles on the straight lines to the goals, none, a different set -- each equals a context
    holding it alone over 40 steps, and the first two differ from each other"""
    from sca_amd import scenarios
    sc = scenarios.circle(12)
    start, goal = sc['start'], sc['goal']
    unit = goal[:, :3] - start[:, :3]
    unit /= np.linalg.norm(unit, axis=1)[:, None]
    on_line = (np.round(start[:, :3] + 3.0 * unit, 2), np.full(12, 0.6))
    other = (np.round(start[:, :3] + 5.0 * unit + [0.0, 0.0, 0.4], 2)[::2], np.full(6, 0.9))
    none = (np.zeros((0, 3)), np.zeros(0))
    policy = np.array([0, 1, 2, 3, 4, 5] * 2, np.uint8)
    scenes = [_scene_dict(S, start, goal, policy) for _ in range(3)]
    sets = [on_line, none, other]
    sol, off = _context(S, scenes, sets)
    alone = [_context(S, [scenes[s]], [sets[s]])[0] for s in range(3)]
    obs_off = [0, 12, 12, 18]
    differ = False
    for t in range(40):
        for x in [sol] + alone:
            x.run_steps(1, S.NBR_KDTREE)
            x.synchronize()
        got = everything(sol)
        for s in range(3):
            assert_scene_equals_alone(got, int(off[s]), int(off[s + 1]), obs_off[s], everything(alone[s]), ('leak', 'step', t, 'scene', s))
        differ = differ or not np.array_equal(got['pos'][0:12], got['pos'][12:24])
    assert differ, 'the scene with obstacles on the lines to the goals moved exactly like the one without any'
    assert sol.pass_forms() & S.FORM_SCENE_OBSTACLES
    assert not alone[1].pass_forms() & S.FORM_SCENE_OBSTACLES      # (a total of 0 is "no obstacles")
    for x in [sol] + alone:
        x.close()


def test_arrived_agents_of_a_state_from_outside_meet_their_own_scenes_obstacles(S):
    """sca_set_state with the at-goal flag set: the first env update looks once whether an arrived agent touches an obstacle (the
    whole-wavefront walk of the obstacle tree, from the scene's own root).  Three scenes with the same agents, some of them arrived inside
    an obstacle of the FIRST scene's set only: flagged there and nowhere else, each scene as in a context of its own."""
    from sca_amd import scenarios
    sc = scenarios.circle(12)
    start, goal = sc['start'], sc['goal']
    inside = (start[:6, :3] + [0.1, 0.0, 0.0], np.full(6, 0.2))               # inside the first six agents (their neighbours, 1.23 m away, stay clear: reach 0.7)
    far = (start[:4, :3] + [0.0, 0.0, 30.0], np.full(4, 0.8))
    none = (np.zeros((0, 3)), np.zeros(0))
    scenes = [_scene_dict(S, start, goal, 1) for _ in range(3)]
    sets = [inside, none, far]
    flags = np.zeros(12, np.uint8)
    flags[[0, 2, 4, 7, 9]] = 1                                                # FLAG_AT_GOAL

    def feed(sol, copies):
        n = 12 * copies
        sol.set_state(np.tile(start[:, :3], (copies, 1)), np.zeros((n, 3), np.float32), np.tile(start[:, 3:6], (copies, 1)), np.tile(flags, copies))
    sol, off = _context(S, scenes, sets, tracker=False)
    feed(sol, 3)
    alone = [_context(S, [scenes[s]], [sets[s]], tracker=False)[0] for s in range(3)]
    for t in range(3):
        for x, copies in [(sol, 3)] + [(x, 1) for x in alone]:
            if t == 0:
                feed(x, copies)
            x.run_steps(1, S.NBR_KDTREE)
            x.synchronize()
        got = sol.get_state()
        for s in range(3):
            want = alone[s].get_state()
            for key in want:
                assert np.array_equal(got[key][12 * s:12 * s + 12], want[key]), ('arrived', t, s, key)
        if t == 0:
            coll = (got['flags'] & 2).astype(bool).reshape(3, 12)
            assert coll[0, [0, 2, 4]].all()                                     # arrived, and inside an obstacle of their own scene's set
            assert coll[0, [1, 3, 5]].all() and not coll[0, 6:].any()           # (the others inside one; the arrived agents 7 and 9 are not)
            assert not coll[1].any() and not coll[2].any()                      # the same agents in the scenes that do not have these obstacles
    for x in [sol] + alone:
        x.close()


OBS_COUNTS = [0, 1, 2, 10, 11, 21, 300]                           # none, one node, leaf boundaries (MAX_LEAF = 10), a deep tree


def _random_obstacles(nscenes):
    """one seeded obstacle set per scene, the counts of OBS_COUNTS in turn (scene s: OBS_COUNTS[(s + s // 7) % 7], so that every scene size
    class meets several counts); around the small scenes' volume (scene_util.random_scenes), the 300 spread wider"""
    rng = np.random.default_rng(777)
    out = []
    for s in range(nscenes):
        m = OBS_COUNTS[(s + s // 7) % 7]
        spread = 25.0 if m == 300 else 8.0
        pos = np.round(rng.uniform(-spread, spread, (m, 3)) * [1, 1, 0.5] + [0, 0, 12.0], 2)
        out.append((pos, np.round(rng.uniform(0.3, 1.2, m), 2)))
    return out


@pytest.mark.parametrize('packed', [0, 1])
def test_random_scenes_with_their_own_obstacles_against_the_oracle(S, oracle, packed, monkeypatch):
    """64 seeded scenes (sizes as in test_gpu_scenes.test_random_scenes_against_the_oracle), each with its own 0 / 1 / 2 / 10 / 11 / 21 / 300
    obstacles, mixed policies, 6 free-running steps: every scene against the oracle run on that scene alone with its own obstacles.  In both
    K1 scene forms (SCA_K1_PACKED: 1 is what 6884 agents run by default -- a wavefront's four groups can belong to four scenes, some of them
    without obstacles --, 0 is k_neighbors_kd_scenes)."""
    monkeypatch.setenv('SCA_K1_PACKED', str(packed))                 # read by sca_create
    scenes, sizes, _, _ = random_scenes(S)
    obstacles = _random_obstacles(len(scenes))
    assert sorted({len(r) for _, r in obstacles}) == OBS_COUNTS
    sol, off = _context(S, scenes, obstacles)
    obs_off = np.concatenate([[0], np.cumsum([len(r) for _, r in obstacles])]).astype(np.int32)
    ref = oracle_scene_runs(oracle, 'own obstacles', scenes, obstacles, stop_when_done=True)
    saw_obstacle_neighbour, finished = set(), set()
    for t in range(6):
        sol.run_steps(1, S.NBR_KDTREE)
        sol.synchronize()
        assert sol.pass_forms() & S.FORM_SCENE_OBSTACLES
        g, a, vd, perm, nb = sol.get_state(), sol.actions(), sol.diag()['vpref'], sol.get_kd_perm(), sol.neighbors()
        for s, sc in enumerate(scenes):
            m, sl, lo, olo = sc['n'], slice(int(off[s]), int(off[s + 1])), int(off[s]), int(obs_off[s])
            obs_pos, obs_radius = obstacles[s]
            r = ref[s]['steps'][t]
            if r is None:
                # every agent is done: the reference's `while not env.step()` has stopped calling env.step() for this scene, and in the
                # batch it is inert -- its state what its last step left, its action rows zero
                r = ref[s]['last']
                finished.add(s)
                assert not a[sl].any(), ('finished scene', s, 'step', t, 'action')
                assert np.array_equal(perm[sl] - lo, r['perm']), ('finished scene', s, 'step', t, 'perm')
                for key, want in (('pos', r['pos']), ('vel', r['vel']), ('heading', r['head']), ('flags', r['flags']), ('total_dist', r['td']), ('step_num', r['sn'])):
                    assert np.array_equal(g[key][sl], want), ('finished scene', s, 'step', t, key)
                continue
            p, active = r['p'], r['active']
            ctx = ('scene', s, 'size', m, 'obstacles', len(obs_radius), 'step', t)
            assert np.array_equal(a[sl], p['action']), ctx + ('action',)
            valid = p['nbr_valid'].astype(bool)
            assert np.array_equal(nb['nbr_valid'][sl].astype(bool), valid), ctx
            assert np.array_equal(nb['nbr_n'][sl][valid], p['nbr_n'][valid]), ctx + ('nbr_n',)
            have = nb['nbr_id'][sl]
            ids = have - np.where(have >= 0, np.where(nb['nbr_kind'][sl] == 1, olo, lo), 0)        # global ids: agents + lo, obstacles + obs_offsets[s]
            assert np.array_equal(ids[valid], p['nbr_id'][valid]), ctx + ('nbr_id',)
            assert np.array_equal(nb['nbr_kind'][sl][valid], p['nbr_kind'][valid]), ctx + ('nbr_kind',)
            assert np.array_equal(nb['nbr_dsq'][sl][valid], p['nbr_dsq'][valid]), ctx + ('nbr_dsq',)
            if (nb['nbr_kind'][sl][valid] == 1).any():
                saw_obstacle_neighbour.add(len(obs_radius))
                listed = have[valid][nb['nbr_kind'][sl][valid] == 1]
                assert (listed >= olo).all() and (listed < int(obs_off[s + 1])).all(), ctx + ('an obstacle of another scene',)
            assert np.array_equal(vd[sl][active], p['vpref'][active]), ctx + ('vpref',)
            assert np.array_equal(perm[sl] - lo, r['perm']), ctx + ('perm',)
            for key, want in (('pos', r['pos']), ('vel', r['vel']), ('heading', r['head']), ('flags', r['flags']), ('total_dist', r['td']), ('step_num', r['sn'])):
                assert np.array_equal(g[key][sl], want), ctx + (key,)
    assert saw_obstacle_neighbour >= {1, 2, 10, 11, 21, 300}, saw_obstacle_neighbour      # every count was met by somebody
    assert len(finished) < len(scenes) // 4, sorted(finished)     # (a few one- and two-agent scenes start inside an obstacle)
    rd = sol.device_tracker_replans()
    for s, r in enumerate(ref):
        sl = slice(int(off[s]), int(off[s + 1]))
        assert np.array_equal(rd[sl][r['ext']], r['replans'][r['ext']]), ('re-plans', s)
    sol.close()


ENTRY = ['F4_mixed_takeoff16', 'F1_sca_circle8', 'F13_fuzz_track_00', 'F16_params_pitch30', 'F14_fuzz_episode_01', 'F2_orca_circle100',
         'F17_hetero_mixed48', 'F4_sca_circle16_obs']


def test_entry_points_agree_with_per_scene_sets(S):
    """sca_env_step, sca_step_host (block contents included) and sca_policy_pass + sca_env_update against sca_run_steps, 40 steps, on a batch
    whose scenes have 8, 0, 3, 8, 4, 0, 5 and 8 obstacles of their own"""
    ref = ObsBatch(S, ENTRY)
    assert [len(r) for _, r in ref.obs] == [8, 0, 3, 8, 4, 0, 5, 8]
    others = dict(env_step=ObsBatch(S, ENTRY), step_host=ObsBatch(S, ENTRY), pass_update=ObsBatch(S, ENTRY))
    h = others['step_host'].sol.host_state()
    for k in ('pos', 'heading', 'flags', 'total_dist', 'step_num', 'vel'):
        h[k][...] = ref.sol.get_state()[k]
    for t in range(40):
        ref.sol.run_steps(1, S.NBR_KDTREE)
        ref.sol.synchronize()
        want = ref.snapshot()
        want_actions, want_sc, want_nb = ref.sol.actions(), ref.sol.scene_state(), ref.sol.neighbors()
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
            nb = b.sol.neighbors()
            for key in want_nb:
                assert np.array_equal(nb[key], want_nb[key]), (name, t, key)
            sc = b.sol.scene_state()
            assert np.array_equal(sc['active'], want_sc['active']) and np.array_equal(sc['steps'], want_sc['steps']), (name, t)
            assert b.sol.pass_forms() & S.FORM_SCENES and b.sol.pass_forms() & S.FORM_SCENE_OBSTACLES, name
        for key in ('pos', 'heading', 'flags', 'total_dist', 'step_num'):
            assert np.array_equal(h[key], want['state'][key]), ('host block', t, key)
        assert np.array_equal(h['action'], want_actions), ('host block', t)
    # ... and that loop is the recorded one: the fixtures' records of step 39
    snap = ref.snapshot()
    for s in range(ref.B):
        if 39 in ref.index[s]:
            ref.check_state(snap, s, ref.index[s][39], '_after', ('entry points', 39))
    for b in list(others.values()) + [ref]:
        b.sol.close()


def _lifetime_scenes(S):
    """three small scenes in one volume (policies that need no planner: a re-used context carries no plan from an earlier run), and
    obstacle sets in their way"""
    rng = np.random.default_rng(99)
    scenes = []
    for size in (9, 14, 11):
        pos = np.round(rng.uniform(-6, 6, (size, 3)) * [1, 1, 0.5] + [0, 0, 12.0], 2)
        goal = np.round(-pos * [1, 1, 0] + [0, 0, 1] * pos + rng.uniform(-1, 1, (size, 3)), 2)
        start = np.zeros((size, 6)); start[:, :3] = pos
        start[:, 3] = np.arctan2(goal[:, 1] - pos[:, 1], goal[:, 0] - pos[:, 0])
        g6 = np.zeros((size, 6)); g6[:, :3] = goal
        scenes.append(_scene_dict(S, start, g6, rng.integers(1, 5, size)))
    sets = [(np.round(rng.uniform(-5, 5, (m, 3)) * [1, 1, 0.5] + [0, 0, 12.0], 2), np.full(m, 0.8)) for m in (4, 0, 12)]
    return scenes, sets


def _run(S, sol, steps=8):
    sol.run_steps(steps, S.NBR_KDTREE)
    sol.synchronize()
    return everything(sol)


def _restart(sol, scenes):
    start = np.concatenate([sc['start'] for sc in scenes])
    n = len(start)
    sol.set_state(start[:, :3], np.zeros((n, 3), np.float32), start[:, 3:6], np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.int32))
    sol.set_kd_perm(np.arange(n, dtype=np.int32))


def test_refusals_change_nothing(S):
    from sca_amd import _lib
    scenes, sets = _lifetime_scenes(S)
    off = np.concatenate([[0], np.cumsum([sc['n'] for sc in scenes])]).astype(np.int32)
    n = int(off[-1])
    cat = lambda key: np.concatenate([sc[key] for sc in scenes])
    sol = S.BatchedSolver(max_agents=n, max_obstacles=16)
    pos, rad = np.concatenate([p for p, _ in sets]), np.concatenate([r for _, r in sets])

    def call(offsets, nscenes=None, p=pos, r=rad):
        o = None if offsets is None else np.ascontiguousarray(offsets, np.int32)
        rc = sol.L.sca_set_scene_obstacles(sol.ctx, (len(o) - 1) if nscenes is None else nscenes, None if o is None else _lib.ptr(o, C.c_int32),
                                           None if p is None else _lib.ptr(p, C.c_double), None if r is None else _lib.ptr(r, C.c_double))
        return rc, sol.L.sca_last_error(sol.ctx).decode()
    good = [0, 4, 4, 16]
    rc, msg = call(good)
    assert rc == ERR_STATE and 'sca_set_scenes' in msg                          # no agents, no scenes
    sol.set_agents(np.full(n, 0.5), np.ones(n), cat('goal')[:, :3], cat('policy'), cat('zaxis'), cat('mrd'))
    rc, msg = call(good)
    assert rc == ERR_STATE and 'sca_set_scenes' in msg                          # agents, no scenes yet
    sol.set_scenes(off)
    sol.set_scene_obstacles(sets)
    refusals = [(dict(offsets=[0, 4, 16]), 'the context holds 3 scenes'), (dict(offsets=[0, 4, 4, 16, 16]), 'the context holds 3 scenes'),
                (dict(offsets=good, nscenes=0), 'the context holds 3 scenes'), (dict(offsets=None, nscenes=3), 'obs_offsets is NULL'),
                (dict(offsets=[1, 4, 4, 16]), 'obs_offsets[0] must be 0'), (dict(offsets=[0, 4, 3, 16]), 'must not decrease (scene 1)'),
                (dict(offsets=[0, 4, 4, 17]), "17 obstacles in all, sca_create's max_obstacles is 16"),
                (dict(offsets=good, p=None), 'must not be NULL'), (dict(offsets=good, r=None), 'must not be NULL')]
    for kw, needle in refusals:
        rc, msg = call(**kw)
        assert rc == ERR_ARG and needle in msg and msg.startswith('sca_set_scene_obstacles'), (kw, rc, msg)
    # ... and the context is what it was: the sets of the accepted call, as in a fresh context
    _restart(sol, scenes)
    fresh = _context(S, scenes, sets, tracker=False)[0]
    same(_run(S, sol), _run(S, fresh), ('after the refusals',), nan_keys=('vpref',))
    assert sol.pass_forms() & S.FORM_SCENE_OBSTACLES
    sol.close(); fresh.close()


def test_lifetime_of_the_per_scene_sets(S):
    scenes, sets = _lifetime_scenes(S)
    shared = sets[2]
    # sca_set_obstacles afterwards: one shared set again, as in a batch that never had per-scene sets
    sol = _context(S, scenes, sets, max_obstacles=16, tracker=False)[0]
    _run(S, sol, 3)
    sol.set_obstacles(*shared)
    _restart(sol, scenes)
    fresh = _context(S, scenes, shared, mode='shared', max_obstacles=16, tracker=False)[0]
    same(_run(S, sol), _run(S, fresh), ('back on a shared set',), nan_keys=('vpref',))
    assert sol.pass_forms() & S.FORM_SCENES and not sol.pass_forms() & S.FORM_SCENE_OBSTACLES
    assert fresh.pass_forms() & S.FORM_SCENES and not fresh.pass_forms() & S.FORM_SCENE_OBSTACLES     # scenes + a shared set: what it reported before
    fresh.close()
    # per-scene sets again, then sca_set_scenes: the sets go, the context has no obstacles
    off = np.concatenate([[0], np.cumsum([sc['n'] for sc in scenes])]).astype(np.int32)
    bare = _context(S, scenes, None, mode='none', max_obstacles=16, tracker=False)[0]
    want = _run(S, bare)
    assert not bare.pass_forms() & S.FORM_SCENE_OBSTACLES
    sol.set_scene_obstacles(sets)
    _restart(sol, scenes)
    _run(S, sol, 2)
    assert sol.pass_forms() & S.FORM_SCENE_OBSTACLES
    for how in ('set_scenes', 'set_scenes(None) + set_scenes', 'set_agents'):
        if how == 'set_scenes':
            sol.set_scenes(off)
        elif how == 'set_agents':
            cat = lambda key: np.concatenate([sc[key] for sc in scenes])
            n = int(off[-1])
            sol.set_agents(np.full(n, 0.5), np.ones(n), cat('goal')[:, :3], cat('policy'), cat('zaxis'), cat('mrd'))
            sol.set_scenes(off)
        else:
            sol.set_scenes(None)
            sol.set_scenes(off)
        _restart(sol, scenes)
        same(_run(S, sol), want, (how,), nan_keys=('vpref',))
        assert sol.pass_forms() & S.FORM_SCENES and not sol.pass_forms() & S.FORM_SCENE_OBSTACLES, how
        sol.set_scene_obstacles(sets)                             # (and on again for the next way of dropping them)
    # a total of 0 is "no obstacles"
    sol.set_scene_obstacles([(np.zeros((0, 3)), np.zeros(0))] * 3)
    _restart(sol, scenes)
    same(_run(S, sol), want, ('a total of 0',), nan_keys=('vpref',))
    assert not sol.pass_forms() & S.FORM_SCENE_OBSTACLES
    sol.close(); bare.close()


def test_scene_batch_with_scene_obstacles_equals_separate_envs(S):
    """SceneBatch(scene_obstacles=...) of an open circle, a take-off/landing scene with its 8 spheres and a circle among a few spheres
    against three MACAEnv loops"""
    from sca_amd import env as E, metrics, scenarios
    from sca_amd.scenes import SceneBatch

    def spheres(pos, radius):
        return [E.Obstacle(pos=list(map(float, p)), shape_dict={'shape': 'sphere', 'feature': float(r)}, id=i) for i, (p, r) in enumerate(zip(pos, radius))]

    tk = scenarios.takeoff_landing(16)
    assert len(tk['obs_radius']) == 8
    few = ([[1.5, 0.5, 10.0], [-2.0, 1.0, 10.5], [0.0, -2.5, 9.5]], [0.7, 0.5, 0.9])
    spec = [(scenarios.circle(12), E.RVO3DPolicy, ([], [])), (tk, E.SCAPolicy, (tk['obs_pos'], tk['obs_radius'])), (scenarios.circle(10), E.ORCA3DPolicy, few)]
    with pytest.raises(ValueError):
        SceneBatch([agents_of(sc, p) for sc, p, _ in spec], spheres(*few), scene_obstacles=[spheres(*o) for _, _, o in spec])
    batch = SceneBatch([agents_of(sc, p) for sc, p, _ in spec], scene_obstacles=[spheres(*o) for _, _, o in spec], device_tracker=True)
    envs = []
    for sc, p, o in spec:
        env = E.MACAEnv(device_tracker=True)
        env.set_agents(agents_of(sc, p), obstacles=spheres(*o))
        envs.append(env)
    counts, done_env = [0, 0, 0], [False, False, False]
    saw_obstacle = False
    for loops in range(6000):
        done = batch.step()
        for s, env in enumerate(envs):
            if not done_env[s]:
                done_env[s] = env.step({})
                counts[s] += 1
        if loops < 60 or loops % 50 == 0:                           # the neighbour lists, object by object
            for s, env in enumerate(envs):
                view = batch.env(s)
                if view.done or done_env[s]:
                    continue
                for a, b in zip(view.agents, env.agents):
                    na, nb = a.neighbors, b.neighbors
                    assert len(na) == len(nb), (loops, s, a.id)
                    for (oa, da), (ob, db) in zip(na, nb):
                        assert type(oa) is type(ob) and da == db, (loops, s, a.id)
                        if isinstance(oa, E.Obstacle):
                            saw_obstacle = True
                            assert oa is view.obstacles[view.obstacles.index(oa)] and np.array_equal(oa.pos_global_frame, ob.pos_global_frame) and oa.radius == ob.radius
                        else:
                            assert oa.id == ob.id and oa is view.agents[oa.id], (loops, s, a.id)
        if done:
            break
    assert batch.done.all() and all(done_env) and saw_obstacle
    for s, env in enumerate(envs):
        view = batch.env(s)
        assert int(batch.steps[s]) == counts[s] == view.steps, (s, int(batch.steps[s]), counts[s])
        assert len(view.obstacles) == len(env.obstacles) == len(spec[s][2][1])
        for key in ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num'):
            assert np.array_equal(getattr(view, key), getattr(env, key)), (s, key)
        assert view.kdTree.agentIDs == env.kdTree.agentIDs
        ma, mb = metrics.episode_metrics(view), metrics.episode_metrics(env)
        assert set(ma) == set(mb)
        for key in ma:
            if key != 'AverageCost':                                # a wall time
                assert ma[key] == mb[key] or (ma[key] != ma[key] and mb[key] != mb[key]), (s, key, ma[key], mb[key])
        env.solver.close()
    assert batch.solver.pass_forms() & S.FORM_SCENE_OBSTACLES
    batch.close()
