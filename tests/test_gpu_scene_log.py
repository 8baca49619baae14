"""The trajectory log per scene (-m gpu; sca_scene_history_enable / _rows / sca_get_scene_history, SceneBatch(scene_history=...),
run_episodes(history_rows=...)).  The bar is the scene contract's: for every scene the rows are bit for bit the rows sca_get_history gives
for a context that holds that episode alone with sca_history_enable, stepped as often as the scene was -- and no other scene's log can tell
that a scene finished, overflowed or was restarted.  No tolerance anywhere.

The synthetic scenes are seeded; a scene's log alone (`solo`) is computed once per (scene, steps, step form) and shared."""
import ctypes as C
import json

import numpy as np
import pytest

from scene_util import agents_of, everything, load_any, restart_all

pytestmark = pytest.mark.gpu

SCA, RVO3D, ORCA3D = 0, 1, 3
KEYS = ('pos', 'heading', 'vel')


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


# ---- seeded synthetic scenes ------------------------------------------------------------------------------------------------------------------
def make_scene(seed, n, policies, goal_dist):
    """n agents in a box of 0.02 agents per cubic metre (at least 6 m wide), random headings, every goal `goal_dist` metres from its start in a
    random direction: at 0.1 m per step the distance sets the step the scene finishes at.  policies: drawn per agent."""
    rng = np.random.default_rng(seed)
    side = max(3.0, 0.5 * (n / 0.02) ** (1.0 / 3.0))
    pos = rng.uniform(-side, side, (n, 3))
    pos[:, 2] += side + 5.0
    d = rng.normal(0, 1, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 2] *= 0.3                                                   # mostly level: inside the tracker's pitch limits
    goal = pos + goal_dist * d / np.linalg.norm(d, axis=1, keepdims=True)
    heading = np.zeros((n, 3))
    heading[:, 0] = np.arctan2(d[:, 1], d[:, 0]) + rng.uniform(-0.6, 0.6, n)
    goal_heading = np.zeros((n, 3))
    goal_heading[:, 0] = np.arctan2(d[:, 1], d[:, 0])
    policy = rng.choice(np.asarray(policies, np.uint8), n).astype(np.uint8)
    return dict(key=(seed, n, tuple(policies), goal_dist), n=n, pos=pos, heading=heading, vel=np.zeros((n, 3), np.float32), goal=goal,
                goal_heading=goal_heading, policy=policy, radius=np.full(n, 0.5), pref_speed=np.ones(n), zaxis=np.zeros(n, np.uint8),
                max_run_dist=np.full(n, 3.0 * goal_dist + 1.0))


# test 1: the wavefront boundaries of k_scene_log (16 agents per wavefront) and of the scene kernels, scenes that end inside 40 steps and
# scenes that do not.  (size, policies, metres to the goal)
SCENES1 = [(1, (ORCA3D,), 0.8), (7, (RVO3D,), 1.2), (16, (SCA,), 6.0), (17, (ORCA3D, RVO3D), 1.6), (64, (RVO3D, ORCA3D, SCA), 30.0),
           (65, (SCA, ORCA3D), 30.0), (100, (ORCA3D, RVO3D, SCA), 30.0)]
STEPS1 = 40


def scenes1():
    return [make_scene(100 + k, n, pol, dist) for k, (n, pol, dist) in enumerate(SCENES1)]


def cat(scenes, key):
    return np.concatenate([s[key] for s in scenes])


def offsets(scenes):
    return np.concatenate([[0], np.cumsum([s['n'] for s in scenes])]).astype(np.int32)


def context(S, scenes, as_scenes):
    """the scenes side by side in one context (as_scenes) or, for a list of one, the plain context that holds the episode alone.  Not
    scene_util.context: this one sets an empty shared obstacle set, makes scenes only where asked, enables the tracker only where a tracked
    policy is present, passes total_dist and step_num with the state, sets the permutation, and returns the solver alone."""
    n = int(sum(s['n'] for s in scenes))
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
    sol.set_agents(cat(scenes, 'radius'), cat(scenes, 'pref_speed'), cat(scenes, 'goal'), cat(scenes, 'policy'), cat(scenes, 'zaxis'), cat(scenes, 'max_run_dist'))
    if as_scenes:
        sol.set_scenes(offsets(scenes))
    if np.isin(cat(scenes, 'policy'), (0, 5)).any():
        sol.device_tracker_enable(cat(scenes, 'goal_heading'), in_pass=True)
    sol.set_state(cat(scenes, 'pos'), cat(scenes, 'vel'), cat(scenes, 'heading'), np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.int32))
    sol.set_kd_perm(np.arange(n, dtype=np.int32))
    return sol


def run_steps_1(S, sol):
    sol.run_steps(1, S.NBR_KDTREE)
    sol.synchronize()


_SOLO = {}


def solo(S, scene, steps, form='run1', step_fn=None):
    """the context-wide log of the episode alone after `steps` steps: dict of [steps, n, 3] arrays (shared, nobody writes to them)"""
    key = (scene['key'], steps, form)
    if key not in _SOLO:
        sol = context(S, [scene], False)
        sol.history_enable(max(steps, 1))
        for t in range(steps):
            (step_fn or run_steps_1)(S, sol)
        sol.synchronize()
        assert sol.history_rows() == (steps, 0)
        _SOLO[key] = sol.history() if steps else {k: np.zeros((0, scene['n'], 3)) for k in KEYS}
        sol.close()
    return _SOLO[key]


def assert_log_equals(got, want, ctx):
    for k in KEYS:
        assert got[k].shape == want[k].shape, ctx + (k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), ctx + (k, int((got[k] != want[k]).any(axis=(1, 2)).argmax()))


def oracle_steps_live(oracle, scene, steps):
    """The scene alone through the oracle's free-running step (policy_step / env_update / Tracker, as tests/form_fuzz.py and
    tests/test_gpu_tracker_oracle.py drive it): the number of steps it is live for, at most `steps`."""
    n = scene['n']
    ext = np.isin(scene['policy'], (0, 5))
    tr = oracle.Tracker(scene['goal'], scene['goal_heading'], scene['pref_speed'], scene['zaxis'])
    pos, vel, head = scene['pos'].copy(), scene['vel'].copy(), scene['heading'].copy()
    flags, td, sn, perm = np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.int32), np.arange(n, dtype=np.int32)
    none = np.zeros((0, 3)), np.zeros(0)
    taken = 0
    while taken < steps and ((flags & 7) == 0).any():
        active = ((flags & 7) == 0) & ext
        vp = tr.vpref(pos, vel, head, active.astype(np.uint8), nthreads=8)
        r = oracle.policy_step(pos, vel, head, scene['radius'], scene['pref_speed'], flags, scene['goal'], scene['policy'], scene['zaxis'], vp,
                               ext.astype(np.uint8), perm, none[0], none[1], nthreads=8)
        tr.note_neighbors(r['nbr_valid'], r['nbr_n'], r['nbr_dsq'])
        perm = r['perm']
        u = oracle.env_update(pos, vel, head, scene['radius'], r['flags'], scene['goal'], r['action'], td, scene['max_run_dist'], sn, none[0], none[1])
        pos, vel, head, flags, td, sn = u['pos'], u['vel'], u['heading'], u['flags'], u['total_dist'], u['step_num']
        taken += 1
    tr.close()
    return taken, bool(((flags & 7) == 0).any())


def test_equals_the_context_alone_across_wavefront_and_scene_boundaries(S, oracle):
    """Scenes of 1, 7, 16, 17, 64, 65 and 100 agents, ORCA3D / RVO3D / SCA with the device tracker, 40 batch steps: every scene's log is the
    log of the context alone stepped steps[s] times, rows_logged == steps, and a scene that finished early gained no row afterwards."""
    scenes = scenes1()
    # on the CPU first: does the batch show both cases?
    alone = [oracle_steps_live(oracle, sc, STEPS1) for sc in scenes]
    finished = [s for s, (taken, live) in enumerate(alone) if not live and taken < STEPS1]
    still_live = [s for s, (taken, live) in enumerate(alone) if live]
    assert len(finished) >= 2 and len(still_live) >= 2, alone
    sol = context(S, scenes, True)
    off = offsets(scenes)
    sol.scene_history_enable(STEPS1)
    assert sol.scene_history_rows()['logged'].tolist() == [0] * len(scenes)
    rows_at = []
    for t in range(STEPS1):
        run_steps_1(S, sol)
        rows_at.append(sol.scene_history_rows()['logged'].copy())
    st = sol.scene_state()
    rows = sol.scene_history_rows()
    assert np.array_equal(rows['logged'], st['steps']) and not rows['dropped'].any()
    assert st['steps'].tolist() == [taken for taken, _ in alone], (st['steps'].tolist(), alone)         # the oracle's step counts
    for s in finished:                                              # no row while the others ran on
        assert all(r[s] == st['steps'][s] for r in rows_at[int(st['steps'][s]) - 1:]), (s, [int(r[s]) for r in rows_at])
    for s, sc in enumerate(scenes):
        got = sol.scene_history(s)
        assert got['pos'].shape == (int(st['steps'][s]), sc['n'], 3)
        assert_log_equals(got, solo(S, sc, int(st['steps'][s])), ('scene', s))
    # the last row of a live scene is the state the context reports
    now = sol.get_state()
    for s in still_live:
        lo, hi = int(off[s]), int(off[s + 1])
        last = sol.scene_history(s, first_row=STEPS1 - 1, nrows=1)
        assert np.array_equal(last['pos'][0], now['pos'][lo:hi]) and np.array_equal(last['heading'][0], now['heading'][lo:hi])
    # windows: rows and scene-local agents
    w = sol.scene_history(6, first_row=3, nrows=4, agent_begin=17, agent_count=50)
    whole = sol.scene_history(6)
    for k in KEYS:
        assert np.array_equal(w[k], whole[k][3:7, 17:67]), k
    sol.close()


def test_the_references_own_log(tmp_path):
    """Both recorded episodes with the reference's logger on (F11: 16 agents each, different obstacle sets) as two scenes of one SceneBatch,
    run to done: metrics.trajectories of each scene view is the reference's history_info on all 13 columns, and write_episode_log writes
    what tests/test_episode_log.py checks of a MACAEnv's."""
    from sca_amd import env as E, metrics, scenes
    from test_episode_log import FIXTURES, _agents_and_obstacles
    fxs = [load_any(n) for n in FIXTURES]
    built = [_agents_and_obstacles(fx, E) for fx in fxs]
    batch = scenes.SceneBatch([a for a, _ in built], scene_obstacles=[o for _, o in built], device_tracker=True, scene_history=700)
    steps = 1
    while not batch.step():
        steps += 1
        assert steps < 700
    assert steps == max(int(fx['steps_run']) for fx in fxs)
    for s, fx in enumerate(fxs):
        view = batch.env(s)
        assert view.steps == int(fx['steps_run'])
        traj = metrics.trajectories(view)
        want = fx['hist']
        assert traj.shape == want.shape
        for lo, hi, what in ((0, 3, 'pos'), (3, 6, 'heading'), (6, 9, 'vel'), (9, 13, 'goal and radius')):
            assert np.array_equal(traj[:, :, lo:hi], want[:, :, lo:hi]), (FIXTURES[s], what)
        paths = metrics.write_episode_log(view, str(tmp_path / str(s)), xlsx=False)
        cfg = json.load(open(paths['env_cfg']))
        ref = json.loads(str(fx['env_cfg']))
        assert list(cfg.keys()) == list(ref.keys())
        for k in ('all_agent_info', 'all_obstacle', 'successful_num', 'all_desire_step_num', 'all_step_num', 'SuccessRate', 'ExtraTime',
                  'all_straight_distance'):
            assert cfg[k] == ref[k], k
        for k in ('all_distance', 'ExtraDistance', 'AverageSpeed'):
            assert abs(cfg[k] - ref[k]) <= 1e-4, k
        back = metrics.read_trajs(paths['trajs'])
        assert len(back) == 16 and list(back[0].keys()) == metrics.ANIMATION_COLUMNS and len(back[0]['pos_x']) == int(fx['steps_run'])
        assert back[3]['pos_x'] == want[3, :, 0].tolist()
    batch.close()


def test_restart_starts_the_log_over(S):
    """Three slots.  Slot 1 is replaced in flight at batch step 10, slot 0 -- which finished by itself before -- is refilled at step 12; after
    15 more steps slot 1's and slot 0's logs are the new episodes' logs alone from row 0, slot 2's is its uninterrupted one."""
    first = [make_scene(200, 7, (ORCA3D,), 0.8), make_scene(201, 17, (RVO3D, SCA), 30.0), make_scene(202, 20, (SCA, ORCA3D), 30.0)]
    new0, new1 = make_scene(203, 7, (RVO3D,), 30.0), make_scene(204, 17, (ORCA3D, SCA), 30.0)
    sol = context(S, first, True)
    sol.scene_history_enable(30)
    for t in range(10):
        run_steps_1(S, sol)
    st = sol.scene_state()
    done0 = int(st['steps'][0])
    assert st['active'][0] == 0 and done0 < 10 and st['steps'].tolist()[1:] == [10, 10], st        # slot 0 has finished by itself
    assert sol.scene_history_rows()['logged'].tolist() == [done0, 10, 10]
    before0 = sol.scene_history(0)
    assert_log_equals(before0, solo(S, first[0], done0), ('slot 0 before the refill',))
    restart_all(sol, [1], [new1])
    assert sol.scene_history_rows()['logged'].tolist() == [done0, 0, 10]                            # the log starts over
    with pytest.raises(S.ScaError):
        sol.scene_history(1, first_row=0, nrows=1)                                                  # stale rows are beyond rows_logged
    assert_log_equals(sol.scene_history(0), before0, ('slot 0 behind the restart of slot 1',))
    for t in range(2):
        run_steps_1(S, sol)
    restart_all(sol, [0], [new0])
    for t in range(13):
        run_steps_1(S, sol)
    st, rows = sol.scene_state(), sol.scene_history_rows()
    assert st['steps'].tolist() == [13, 15, 25]
    assert np.array_equal(rows['logged'], st['steps']) and not rows['dropped'].any()
    assert_log_equals(sol.scene_history(0), solo(S, new0, 13), ('slot 0',))
    assert_log_equals(sol.scene_history(1), solo(S, new1, 15), ('slot 1',))
    assert_log_equals(sol.scene_history(2), solo(S, first[2], 25), ('slot 2',))
    sol.close()


def test_capacity(S):
    """Capacity 5, 12 steps, three live scenes: 5 logged and 7 dropped, rows 0-4 the log alone, and every scene's part still its own (a
    write beyond the capacity would land in the next scene's)."""
    scenes = [make_scene(300, 17, (ORCA3D, RVO3D), 30.0), make_scene(301, 33, (SCA, RVO3D), 30.0), make_scene(302, 9, (ORCA3D,), 30.0)]
    sol = context(S, scenes, True)
    sol.scene_history_enable(5)
    for t in range(12):
        run_steps_1(S, sol)
    rows = sol.scene_history_rows()
    assert sol.scene_state()['steps'].tolist() == [12, 12, 12]
    assert rows['logged'].tolist() == [5, 5, 5] and rows['dropped'].tolist() == [7, 7, 7]
    for s, sc in enumerate(scenes):
        want = solo(S, sc, 12)
        assert_log_equals(sol.scene_history(s), {k: want[k][:5] for k in KEYS}, ('scene', s))
    with pytest.raises(S.ScaError):
        sol.scene_history(0, first_row=0, nrows=6)
    sol.close()


# ---- step forms ---------------------------------------------------------------------------------------------------------------------------------
def scenes5():
    return [make_scene(400, 7, (ORCA3D,), 1.0), make_scene(401, 17, (RVO3D, SCA), 30.0), make_scene(402, 65, (SCA, ORCA3D, RVO3D), 30.0)]


def test_step_forms(S):
    """The same three-scene batch (one scene finishes on the way) through sca_env_step, sca_run_steps(1), sca_run_steps(6), sca_step_host and
    sca_policy_pass + sca_env_update: the same log as sca_run_steps(1) -- test 1's form -- leaves, which is the log of every scene alone."""
    scenes = scenes5()
    T = 12

    def host_form(S, sol):
        sol.step_host(S.NBR_KDTREE, state=sol._first)
        sol._first = False

    forms = {
        'run_steps(1)': lambda S, sol: run_steps_1(S, sol),
        'env_step': lambda S, sol: sol.env_step(S.NBR_KDTREE),
        'step_host': host_form,
        'pass + update': lambda S, sol: (sol.policy_pass(S.NBR_KDTREE), sol.env_update()),
    }
    logs = {}
    for name, fn in list(forms.items()) + [('run_steps(6)', None)]:
        sol = context(S, scenes, True)
        sol.scene_history_enable(T)
        if name == 'step_host':
            h, st = sol.host_state(), sol.get_state()
            for k in ('pos', 'heading', 'flags', 'total_dist', 'step_num', 'vel'):
                h[k][...] = st[k]
            sol._first = True
        if fn is None:
            sol.run_steps(6, S.NBR_KDTREE)
            sol.run_steps(6, S.NBR_KDTREE)
            sol.synchronize()
        else:
            for t in range(T):
                fn(S, sol)
        st = sol.scene_state()
        assert 0 < st['steps'][0] < T and st['steps'].tolist()[1:] == [T, T], (name, st)
        assert np.array_equal(sol.scene_history_rows()['logged'], st['steps']), name
        logs[name] = [sol.scene_history(s) for s in range(3)]
        sol.close()
    steps0 = len(logs['run_steps(1)'][0]['pos'])
    for s, sc in enumerate(scenes):
        assert_log_equals(logs['run_steps(1)'][s], solo(S, sc, steps0 if s == 0 else T), ('run_steps(1)', s))
    for name, log in logs.items():
        for s in range(3):
            assert_log_equals(log[s], logs['run_steps(1)'][s], (name, s))


def test_env_update_without_a_pass(S):
    """sca_env_update with no policy pass before it opens the step itself (k_scene_begin in launch_collide_finish) and integrates the action rows
    as they stand: 3 whole steps, 2 updates alone, 2 whole steps -- the scene log is the log of each scene alone through the same calls."""
    scenes = scenes5()[1:]

    def sequence(S, sol):
        for t in range(3):
            run_steps_1(S, sol)
        for t in range(2):
            sol.env_update()
        for t in range(2):
            run_steps_1(S, sol)

    sol = context(S, scenes, True)
    sol.scene_history_enable(7)
    sequence(S, sol)
    assert sol.scene_state()['steps'].tolist() == [7, 7] and sol.scene_history_rows()['logged'].tolist() == [7, 7]
    for s, sc in enumerate(scenes):
        one = context(S, [sc], False)
        one.history_enable(7)
        sequence(S, one)
        assert one.history_rows() == (7, 0)
        assert_log_equals(sol.scene_history(s), one.history(), ('scene', s))
        one.close()
    sol.close()


def test_both_logs_at_once(S):
    """The context-wide log's rows of a live scene are the scene log's rows, and enabling the scene log changes no value the context can be
    asked for."""
    scenes = scenes5()
    off = offsets(scenes)
    T = 12
    a, b = context(S, scenes, True), context(S, scenes, True)
    a.history_enable(T)
    a.scene_history_enable(T)
    tracked = np.flatnonzero(np.isin(cat(scenes, 'policy'), (0, 5)))[:6]
    for t in range(T):
        run_steps_1(S, a)
        run_steps_1(S, b)
        if t in (0, 5, T - 1):
            ea, eb = everything(a, tracked), everything(b, tracked)
            for k in eb:
                if k == 'track':
                    for i in eb[k]:
                        assert np.array_equal(ea[k][i], eb[k][i], equal_nan=True), (t, k, i)
                else:
                    assert np.array_equal(ea[k], eb[k], equal_nan=True), (t, k)
    wide = a.history()
    assert a.history_rows() == (T, 0)
    steps = a.scene_state()['steps']
    assert 0 < steps[0] < T
    for s in range(3):
        lo, hi = int(off[s]), int(off[s + 1])
        own = a.scene_history(s)
        for k in KEYS:
            assert np.array_equal(own[k], wide[k][:int(steps[s]), lo:hi]), (s, k)
    a.close()
    b.close()


def test_refusals_and_lifetime(S):
    """every refusal of include/sca_hip.h with its code, a refused call changing nothing, and what frees the log"""
    from sca_amd import _lib
    ERR_ARG, ERR_STATE = -1, -3
    scenes = scenes5()
    off = offsets(scenes)
    sol = context(S, scenes[:1], False)                              # a plain context: no scenes
    n = int(off[-1])
    rc = lambda f, *a: f(sol.ctx, *a)
    i32 = lambda a: _lib.ptr(a, C.c_int32)
    logged, dropped = np.full(3, -7, np.int32), np.full(3, -7, np.int32)
    pos = np.zeros((12, n, 3))
    get = lambda scene, first, nrows, ab, ac: rc(sol.L.sca_get_scene_history, scene, first, nrows, ab, ac, _lib.ptr(pos, C.c_double), None, None)
    assert rc(sol.L.sca_scene_history_enable, 8) == ERR_STATE        # no scenes
    assert rc(sol.L.sca_scene_history_enable, 0) == ERR_STATE
    assert rc(sol.L.sca_scene_history_rows, i32(logged), i32(dropped)) == ERR_STATE and get(0, 0, 0, 0, 0) == ERR_STATE
    sol.close()
    sol = context(S, scenes, True)
    assert rc(sol.L.sca_scene_history_rows, i32(logged), i32(dropped)) == ERR_STATE and get(0, 0, 0, 0, 0) == ERR_STATE      # not enabled
    assert logged.tolist() == [-7] * 3
    assert rc(sol.L.sca_scene_history_enable, -1) == ERR_ARG
    assert rc(sol.L.sca_scene_history_rows, None, None) == ERR_STATE                                 # ... and changed nothing
    assert rc(sol.L.sca_scene_history_enable, 8) == 0
    assert rc(sol.L.sca_scene_history_enable, 12) == 0                                               # again before the first step: a new capacity
    assert rc(sol.L.sca_scene_history_rows, i32(logged), None) == 0 and logged.tolist() == [0, 0, 0]
    assert rc(sol.L.sca_scene_history_rows, None, None) == 0
    sol.policy_pass(S.NBR_KDTREE)
    assert rc(sol.L.sca_scene_history_enable, 8) == ERR_STATE        # between a policy pass and its env update
    assert rc(sol.L.sca_scene_history_enable, 0) == ERR_STATE
    assert rc(sol.L.sca_scene_history_rows, i32(logged), i32(dropped)) == 0 and logged.tolist() == [0, 0, 0]     # the step under way has no row yet
    sol.env_update()
    assert rc(sol.L.sca_scene_history_rows, i32(logged), i32(dropped)) == 0 and logged.tolist() == [1, 1, 1] and dropped.tolist() == [0, 0, 0]
    assert rc(sol.L.sca_scene_history_enable, 8) == ERR_STATE        # after a step
    assert rc(sol.L.sca_scene_history_enable, -1) == ERR_ARG
    for t in range(3):
        run_steps_1(S, sol)
    assert sol.scene_history_rows()['logged'].tolist() == [4, 4, 4]  # the refused calls left the log of capacity 12 running
    want = sol.scene_history(1)
    # windows
    assert get(1, 0, 4, 0, 17) == 0 and np.array_equal(pos.reshape(-1)[:4 * 17 * 3].reshape(4, 17, 3), want['pos'])
    assert get(1, 3, 1, 16, 1) == 0 and get(1, 4, 0, 17, 0) == 0 and get(2, 0, 4, 0, 65) == 0
    assert get(-1, 0, 1, 0, 1) == ERR_ARG and get(3, 0, 1, 0, 1) == ERR_ARG
    assert get(1, 0, 5, 0, 17) == ERR_ARG and get(1, 4, 1, 0, 17) == ERR_ARG and get(1, -1, 2, 0, 17) == ERR_ARG and get(1, 0, -1, 0, 17) == ERR_ARG
    assert get(1, 0, 4, 0, 18) == ERR_ARG and get(1, 0, 4, 17, 1) == ERR_ARG and get(1, 0, 4, -1, 2) == ERR_ARG and get(1, 0, 4, 0, -1) == ERR_ARG
    assert get(0, 0, 4, 0, 8) == ERR_ARG                             # scene 0 holds 7
    # sca_set_state leaves the step counts alone: the log goes on
    st = sol.get_state()
    sol.set_state(st['pos'], st['vel'], st['heading'], st['flags'], st['total_dist'], st['step_num'])
    run_steps_1(S, sol)
    assert sol.scene_history_rows()['logged'].tolist() == [5, 5, 5]
    assert np.array_equal(sol.scene_history(1, nrows=4)['pos'], want['pos'])
    # 0 frees; whatever redefines or drops the scenes frees
    assert rc(sol.L.sca_scene_history_enable, 0) == 0
    assert rc(sol.L.sca_scene_history_rows, i32(logged), None) == ERR_STATE and get(1, 0, 1, 0, 1) == ERR_STATE
    assert rc(sol.L.sca_scene_history_enable, 8) == ERR_STATE        # the scenes have stepped
    sol.set_scenes(off)                                              # new counters: the log may be enabled again ...
    assert rc(sol.L.sca_scene_history_enable, 8) == 0
    sol.set_scenes(off)                                              # ... and goes with the scenes it was cut for
    assert rc(sol.L.sca_scene_history_rows, i32(logged), None) == ERR_STATE
    assert rc(sol.L.sca_scene_history_enable, 8) == 0
    sol.set_scenes(None)
    assert rc(sol.L.sca_scene_history_rows, i32(logged), None) == ERR_STATE and rc(sol.L.sca_scene_history_enable, 8) == ERR_STATE
    sol.set_scenes(off)
    assert rc(sol.L.sca_scene_history_enable, 8) == 0
    sol.set_agents(cat(scenes, 'radius'), cat(scenes, 'pref_speed'), cat(scenes, 'goal'), cat(scenes, 'policy'), cat(scenes, 'zaxis'), cat(scenes, 'max_run_dist'))
    assert rc(sol.L.sca_scene_history_rows, i32(logged), None) == ERR_STATE
    sol.close()


def test_run_episodes_hands_the_trajectories_over():
    """A queue of six 12-agent episodes through two slots with history_rows=K, one of them longer than K: every `trajectories` is the log
    of the MACAEnv of that episode alone, rows_dropped is right for the long one, and the queue completes."""
    from sca_amd import env as E, metrics, scenarios, scenes
    K = 150
    circ = scenarios.circle(12, rad=5.0, z=12.0)
    wide = scenarios.circle(12, rad=12.0, z=12.0)                    # 24 m to fly at 0.1 m per step: more than K steps

    def queue():
        return [agents_of(circ, E.SCAPolicy), agents_of(circ, E.RVO3DPolicy), agents_of(wide, E.ORCA3DPolicy), agents_of(circ, E.ORCA3DPolicy),
                agents_of(circ, E.RVO3dDubinsPolicy), agents_of(circ, E.SRVO3DPolicy)]

    got = scenes.run_episodes(queue(), 2, device_tracker=True, history_rows=K, max_steps=5000)
    assert all(r is not None for r in got) and [r['episode'] for r in got] == list(range(6))          # the queue completes
    long_ones = 0
    for i, (r, eps) in enumerate(zip(got, queue())):
        env = E.MACAEnv(history_capacity=r['steps'], device_tracker=True)
        env.set_agents(eps, obstacles=[])
        steps = 1
        while not env.step({}):
            steps += 1
            assert steps <= 5000
        assert steps == r['steps'], (i, steps, r['steps'])
        want = metrics.trajectories(env)
        assert r['rows_dropped'] == max(0, steps - K), (i, r['rows_dropped'], steps)
        long_ones += steps > K
        assert r['trajectories'].shape == (12, min(steps, K), 13)
        assert np.array_equal(r['trajectories'], want[:, :K]), i
        env.solver.close()
    assert long_ones >= 1
