"""Waypoint lists (Agent.path) on the device (-m gpu): k_waypoint's get_trajectory and the straight-line v_pref toward policy.now_goal,
against the reference-recorded F19 episodes (tests/golden/paths, tools/gen_golden_paths.py) and against the CPU oracle fed from the
restatement of the rule (tests/path_rule.py).  Bar: equality -- states, action rows, v_pref, flags, now_goal and what is left of every list."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import path_rule as R
from golden_util import static_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS_DIR = os.path.join(ROOT, 'tests', 'golden', 'paths')
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(PATHS_DIR, 'F19_path_*.npz')))


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


def load(name):
    return dict(np.load(os.path.join(PATHS_DIR, name + '.npz'), allow_pickle=False))


def fixture_lists(fx, left=None):
    return R.lists_from_csr(fx['path_off'], fx['path_pts'], left)


def make_solver(S, fx, paths=True):
    st = static_inputs(fx)
    n = len(st['radius'])
    sol = S.BatchedSolver(max_agents=n, max_obstacles=max(len(st['obs_radius']), 1))
    sol.set_obstacles(st['obs_pos'], st['obs_radius'])
    sol.set_agents(st['radius'], st['pref_speed'], fx['goal6'][:, :3], st['policy'], st['zaxis'], st['max_run_dist'])
    if paths:
        sol.set_paths(fixture_lists(fx))
    return sol, st


def check_path_state(sol, left, now_goal, ctx):
    rem, ng = sol.get_path_state()
    assert np.array_equal(rem, left), ctx + ('path_left', np.flatnonzero(rem != left)[:8].tolist())
    assert np.array_equal(ng, now_goal, equal_nan=True), ctx + ('now_goal',)


NBR = {'kd': 0, 'auto': 3}


def run_recorded_episode(S, name, nbr, ctx, grid=False, on_refusal=None, on_overflow=None):
    """A recorded episode from its start state, nothing fed: sca_run_steps between the recorded steps (two steps per call in the circles), the
    device tracker inside every pass for the SCA / RVO3D+Dubins agents.  Every recorded step equals the reference's.  grid=True: the mode
    is SCA_NBR_GRID -- it builds no tree, so the kd permutation is not compared, and the run ends at the first pass in which a list
    overflows (SCA_ST_NBR_OVERFLOW: from there the grid keeps the nearest max_neighbors where the reference's list depends on its tree's
    visit order, include/sca_hip.h), after on_overflow(step) where the caller gave one.  on_refusal(error): called where the library refuses the episode's first pass
    (the episode is then not run); None: a refusal is an error.  Returns the recorded steps compared."""
    fx = load(name)
    sol, st = make_solver(S, fx)
    compared = 0
    try:
        if st['vpref_mode'].any():
            sol.device_tracker_enable(fx['goal6'][:, 3:6], in_pass=True)
        n = len(st['radius'])
        sol.set_state(fx['start'][:, :3], np.zeros((n, 3), np.float32), fx['start'][:, 3:6], np.zeros(n, np.uint8))
        check_path_state(sol, np.diff(fx['path_off']), np.full((n, 3), np.nan), ctx + ('initial',))
        now = 0

        def run(count):
            """False: the library refused the episode's first pass and the caller has a word to say about it"""
            try:
                sol.run_steps(count, nbr)
            except S.ScaError as e:
                if on_refusal is None or now:
                    raise
                on_refusal(e)
                return False
            sol.synchronize()
            return True
        for k, t in enumerate(int(x) for x in fx['step']):
            at = ctx + (t,)
            if t > now:
                if not run(t - now):
                    return 0
                now = t
            s = sol.get_state()
            for key in ('pos', 'heading', 'total_dist', 'flags'):
                assert np.array_equal(s[key], fx[key][k]), at + ('before', key)
            assert np.array_equal(s['vel'], fx['vel'][k]), at + ('before', 'vel')
            check_path_state(sol, fx['path_left_before'][k], fx['now_goal_before'][k], at + ('before',))
            if not run(1):
                return 0
            now += 1
            called = fx['called'][k].astype(bool)
            assert sol.pass_forms() & S.FORM_WAYPOINTS, at
            dg = sol.diag()
            if grid and (dg['status'] & 32).any():
                assert not (dg['status'] & ~32).any(), at
                if on_overflow is not None:
                    on_overflow(t)
                return compared
            a = sol.actions()
            assert np.array_equal(a[called], fx['action'][k][called]), at + ('action',)
            assert np.array_equal(dg['vpref'][called], fx['vpref'][k][called]), at + ('vpref_used',)
            assert not dg['status'].any(), at
            s = sol.get_state()
            for key, want in (('pos', 'pos_after'), ('heading', 'heading_after'), ('total_dist', 'total_dist_after'), ('flags', 'flags_after')):
                assert np.array_equal(s[key], fx[want][k]), at + ('after', key)
            assert np.array_equal(s['vel'], fx['vel_after'][k]), at + ('after', 'vel')
            if not grid:
                assert np.array_equal(sol.get_kd_perm(), fx['perm_after'][k]), at + ('perm after',)
            check_path_state(sol, fx['path_left_after'][k], fx['now_goal_after'][k], at + ('after',))
            compared += 1
    finally:
        sol.close()
    return compared


@pytest.mark.parametrize('mode', ['kd', 'auto'])
@pytest.mark.parametrize('name', FIXTURES)
def test_free_running_episode_with_paths_is_the_reference(S, name, mode):
    """From the start state, nothing fed: sca_run_steps between the recorded steps (two steps per call in the circles), the device tracker
    inside every pass for the SCA / RVO3D+Dubins agents.  Every recorded step equals the reference's."""
    assert run_recorded_episode(S, name, NBR[mode], (name, mode)) == len(load(name)['step'])


@pytest.mark.parametrize('mode', ['kd', 'auto'])
@pytest.mark.parametrize('name', FIXTURES)
def test_drop_in_env_with_agent_path_is_the_reference(S, name, mode):
    """The same episodes through sca_amd.env: Agent.path set before set_agents, env.step() per step; agent.path, agent.policy.now_goal and
    the agents' state read through the reference's attribute surface."""
    from sca_amd import env as E
    fx = load(name)
    st = static_inputs(fx)
    n = len(st['radius'])
    cls = {0: E.SCAPolicy, 1: E.RVO3DPolicy, 2: E.SRVO3DPolicy, 3: E.ORCA3DPolicy, 4: E.ORCA3DPolicyOfficial, 5: E.RVO3dDubinsPolicy}
    agents = [E.Agent(start_pos=list(fx['start'][i]), goal_pos=list(fx['goal6'][i]), vel=[0.0, 0.0, 0.0], radius=float(st['radius'][i]),
                      pref_speed=float(st['pref_speed'][i]), policy=cls[int(st['policy'][i])], id=i) for i in range(n)]
    for a, p in zip(agents, fixture_lists(fx)):
        a.path = p
    obstacles = [E.Obstacle(pos=list(p), shape_dict={'shape': 'sphere', 'feature': float(r)}, id=j)
                 for j, (p, r) in enumerate(zip(st['obs_pos'], st['obs_radius']))]
    env = E.MACAEnv(neighbor_mode=NBR[mode], device_tracker=bool(st['vpref_mode'].any()))
    env.set_agents(agents, obstacles=obstacles)
    assert all(a.policy.now_goal is None for a in agents if a.path)
    rec = {int(t): k for k, t in enumerate(fx['step'])}
    for t in range(int(fx['n_steps_run'])):
        k = rec.get(t)
        if k is not None:
            assert np.array_equal(env.pos, fx['pos'][k]), (name, t)
            assert [len(a.path) for a in agents] == list(fx['path_left_before'][k]), (name, t)
        done = env.step()
        if k is None:
            continue
        ctx = (name, mode, t)
        called = fx['called'][k].astype(bool)
        assert np.array_equal(env.all_actions[called], fx['action'][k][called]), ctx
        assert np.array_equal(env.pos, fx['pos_after'][k]) and np.array_equal(env.flags, fx['flags_after'][k]), ctx
        left = fx['path_left_after'][k]
        for i, a in enumerate(agents):
            assert a.path == fixture_lists(fx, left)[i], ctx + (i,)
            g = a.policy.now_goal
            want = fx['now_goal_after'][k][i]
            assert (g is None and np.isnan(want[0])) or np.array_equal(g, want), ctx + (i, g, want)
    assert done == (int(fx['done_step']) >= 0)
    env.solver.close()


def test_assigning_agent_path_after_set_agents_takes_effect_at_the_next_step(S):
    """edge10 with agent 1's list assigned only after set_agents (and agent 0's emptied list assigned too): the same episode."""
    from sca_amd import env as E
    fx = load('F19_path_edge10')
    st = static_inputs(fx)
    n = len(st['radius'])
    cls = {0: E.SCAPolicy, 1: E.RVO3DPolicy, 2: E.SRVO3DPolicy, 3: E.ORCA3DPolicy, 4: E.ORCA3DPolicyOfficial, 5: E.RVO3dDubinsPolicy}
    agents = [E.Agent(start_pos=list(fx['start'][i]), goal_pos=list(fx['goal6'][i]), vel=[0.0, 0.0, 0.0], radius=float(st['radius'][i]),
                      pref_speed=float(st['pref_speed'][i]), policy=cls[int(st['policy'][i])], id=i) for i in range(n)]
    lists = fixture_lists(fx)
    for i, a in enumerate(agents):
        if i != 1:
            a.path = lists[i]
    env = E.MACAEnv(device_tracker=True)
    env.set_agents(agents, obstacles=[])
    agents[1].path = lists[1]
    agents[0].path = []
    for t in range(40):
        env.step()
        k = t
        assert np.array_equal(env.pos, fx['pos_after'][k]), t
        assert [len(a.path) for a in agents] == list(fx['path_left_after'][k]), t
    env.solver.close()


@pytest.mark.parametrize('name', FIXTURES)
def test_fed_passes_from_every_record(S, name):
    """set_state + set_path_state from each record, then ONE pass: the recorded actions, v_pref, now_goal and list lengths (the tracked
    agents' v_pref fed from the record: sca_set_vpref mode 1 is theirs)."""
    fx = load(name)
    sol, st = make_solver(S, fx)
    for k in range(len(fx['step'])):
        ctx = (name, int(fx['step'][k]))
        sol.set_state(fx['pos'][k], fx['vel'][k], fx['heading'][k], fx['flags'][k], fx['total_dist'][k])
        sol.set_kd_perm(fx['perm'][k])
        sol.set_path_state(fx['path_left_before'][k], fx['now_goal_before'][k])
        if st['vpref_mode'].any():
            sol.set_vpref(np.nan_to_num(fx['vpref'][k]), st['vpref_mode'])
        sol.policy_pass(S.NBR_KDTREE)
        called = fx['called'][k].astype(bool)
        assert np.array_equal(sol.actions()[called], fx['action'][k][called]), ctx
        assert np.array_equal(sol.diag()['vpref'][called], fx['vpref'][k][called]), ctx
        check_path_state(sol, fx['path_left_after'][k], fx['now_goal_after'][k], ctx)
    sol.close()


def _mixed_scene(S, n=64, seed=5):
    from sca_amd import scenarios
    sc = scenarios.circle(n)
    pol = np.where(np.arange(n) % 2 == 0, S.POL_SCA, S.POL_RVO3D).astype(np.uint8)
    rng = np.random.default_rng(seed)
    paths = []
    for i in range(n):
        s, g = sc['start'][i, :3], sc['goal'][i, :3]
        k = int(rng.integers(0, 5))
        paths.append([list(np.round(s + t * (g - s) + rng.normal(0, 2.0, 3) * [1, 1, 0.3], 2)) for t in np.sort(rng.uniform(0.1, 0.9, k))[::-1]])
    return sc, pol, paths


def _mixed_solver(S, sc, pol, paths):
    from sca_amd import scenarios
    n = len(pol)
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
    sol.set_agents(np.full(n, 0.5), np.full(n, 1.0), sc['goal'][:, :3], pol, S.zaxis_flags(sc['start'], sc['goal']),
                   scenarios.max_run_dist(sc['start'], sc['goal']))
    sol.device_tracker_enable(sc['goal'][:, 3:6], in_pass=True)
    sol.set_paths(paths)
    sol.set_state(sc['start'][:, :3], np.zeros((n, 3), np.float32), sc['start'][:, 3:6], np.zeros(n, np.uint8))
    return sol


def test_tracked_agents_beside_path_agents_in_one_burst(S):
    """Tracked SCA agents (re-plans on the main stream, the neighbour branch on the tracker's side stream) beside RVO3D agents that follow
    lists: 200 steps in ONE sca_run_steps call equal 200 calls of one step each, and the path agents' v_pref in the last pass is the
    restatement's from the state the pass started from."""
    sc, pol, paths = _mixed_scene(S)
    a = _mixed_solver(S, sc, pol, paths)
    b = _mixed_solver(S, sc, pol, paths)
    a.run_steps(199, S.NBR_KDTREE)
    for _ in range(199):
        b.run_steps(1, S.NBR_KDTREE)
    a.synchronize(); b.synchronize()
    sa, sb = a.get_state(), b.get_state()
    ra, ga = a.get_path_state()
    rb, gb = b.get_path_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert np.array_equal(ra, rb) and np.array_equal(ga, gb, equal_nan=True)
    # the 200th pass, checked against the rule from its own start
    left = [p[:int(r)] for p, r in zip(paths, ra)]
    ng = ga.copy()
    vp, mode = R.pass_rule(left, ng, sa['pos'], sc['goal'][:, :3], np.full(len(pol), 0.5), np.full(len(pol), 1.0), pol, sa['flags'],
                           [len(p) > 0 for p in paths])
    a.run_steps(1, S.NBR_KDTREE); a.synchronize()
    assert a.pass_forms() & S.FORM_WAYPOINTS
    use = mode.astype(bool)
    assert use.any()
    assert np.array_equal(a.diag()['vpref'][use], vp[use])
    check_path_state(a, [len(p) for p in left], ng, ('burst',))
    assert int(ra.sum()) < sum(len(p) for p in paths)
    a.close(); b.close()


SCALE = [('random4096_orca_auto', 4096, 3, 3, 20), ('random16384_rvo_kd', 16384, 1, 0, 8), ('random100000_rvo_kd', 100000, 1, 0, 4)]


def _sparse_swarm(n, seed):
    """n agents in a cube sized for ~3 others within neighbor_dist each (what keeps the CPU oracle's pass short at 100 000), goals up to 30 m
    away, headings toward them"""
    rng = np.random.default_rng(seed)
    side = (n * 1400.0) ** (1.0 / 3.0)
    pos = np.round(rng.uniform(0.0, side, (n, 3)) + [0.0, 0.0, 5.0], 3)
    goal = np.round(pos + rng.uniform(-30.0, 30.0, (n, 3)), 3)
    goal[:, 2] = np.maximum(goal[:, 2], 1.0)
    start = np.zeros((n, 6)); start[:, :3] = pos
    start[:, 3] = np.arctan2(goal[:, 1] - pos[:, 1], goal[:, 0] - pos[:, 0])
    g6 = np.zeros((n, 6)); g6[:, :3] = goal
    return dict(start=start, goal=g6, obs_pos=np.zeros((0, 3)), obs_radius=np.zeros(0))


@pytest.mark.parametrize('label,n,pol,mode,steps', SCALE)
def test_at_scale_free_running_equals_the_oracle_fed_from_the_rule(S, oracle, label, n, pol, mode, steps):
    """0-6 random waypoints per agent; the device runs free (sca_run_steps, one step per call so that every pass is compared), the oracle
    takes the same pass with vpref_ext / vpref_mode from tests/path_rule.py."""
    from sca_amd import scenarios
    sc = _sparse_swarm(n, seed=19)
    rng = np.random.default_rng(n)
    goal = sc['goal'][:, :3].copy()
    pos = sc['start'][:, :3].copy()
    radius, ps = np.full(n, 0.5), np.full(n, 1.0)
    policy = np.full(n, pol, np.uint8)
    zaxis = S.zaxis_flags(sc['start'], sc['goal'])
    mrd = scenarios.max_run_dist(sc['start'], sc['goal'])
    paths = []
    for i in range(n):
        k = int(rng.integers(0, 7))
        paths.append([list(np.round(pos[i] + rng.uniform(-4, 4, 3) + (goal[i] - pos[i]) * rng.uniform(0.1, 0.9), 3)) for _ in range(k)])
    off, pts = R.csr(paths)
    sol = S.BatchedSolver(max_agents=n, max_obstacles=max(len(sc['obs_radius']), 1))
    sol.set_obstacles(sc['obs_pos'], sc['obs_radius'])
    sol.set_agents(radius, ps, goal, policy, zaxis, mrd)
    sol.set_paths(paths)
    vel, head = np.zeros((n, 3), np.float32), sc['start'][:, 3:6].copy()
    flags, td, sn = np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.int32)
    sol.set_state(pos, vel, head, flags)
    perm = np.arange(n, dtype=np.int32)
    rem = np.diff(off)
    ng = np.full((n, 3), np.nan)
    for t in range(steps):
        rem, ng, vp, vmode = R.pass_rule_csr(off, pts, rem, ng, pos, goal, radius, ps, policy, flags)
        ref = oracle.policy_step(pos, vel, head, radius, ps, flags, goal, policy, zaxis, vp, vmode, perm, sc['obs_pos'], sc['obs_radius'],
                                 nthreads=16)
        sol.run_steps(1, mode)
        sol.synchronize()
        ctx = (label, t)
        assert np.array_equal(sol.actions(), ref['action']), ctx
        perm = ref['perm']
        s = sol.get_state()
        if n <= 20000:
            u = oracle.env_update(pos, vel, head, radius, ref['flags'], goal, ref['action'], td, mrd, sn, sc['obs_pos'], sc['obs_radius'])
            pos, vel, head, flags, td, sn = u['pos'], u['vel'], u['heading'], u['flags'], u['total_dist'], u['step_num']
            for key, want in (('pos', pos), ('vel', vel), ('heading', head), ('flags', flags), ('total_dist', td)):
                assert np.array_equal(s[key], want), ctx + (key,)
        else:
            # (the oracle's env update checks every pair for collisions: at 100 000 agents the next pass starts from the device's state)
            pos, vel, head, flags = s['pos'], s['vel'], s['heading'], s['flags']
        check_path_state(sol, rem, ng, ctx)
    assert int(rem.sum()) < int(off[-1])
    sol.close()


WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))
import numpy as np, torch, torch.distributed as dist
from sca_amd import scenarios, solver as S
from sca_amd.distributed import ShardedStepper
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
torch.cuda.set_device(0)
dist.init_process_group('gloo')
n, steps = 2000, 15
sc = scenarios.random_cube(n, seed=3)
pol = (np.arange(n) % 5).astype(np.uint8)
rng = np.random.default_rng(7)
paths = [[list(np.round(sc['start'][i, :3] + rng.uniform(-4, 4, 3), 3)) for _ in range(int(rng.integers(0, 5)))] for i in range(n)]

def make():
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1, device=0)
    sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
    sol.set_agents(np.full(n, 0.5), np.full(n, 1.0), sc['goal'][:, :3], pol, S.zaxis_flags(sc['start'], sc['goal']),
                   scenarios.max_run_dist(sc['start'], sc['goal']))
    sol.set_state(sc['start'][:, :3], np.zeros((n, 3), np.float32), sc['start'][:, 3:6], np.zeros(n, np.uint8))
    return sol

sol = make()
st = ShardedStepper(sol, rank, world, torch_mod=torch, dist_mod=dist, staged=True, mode=0, paths=paths)
st.run(steps); st.sync()
got = sol.get_state(); grem, gng = sol.get_path_state()
ref_sol = make(); ref_sol.set_paths(paths)
ref_sol.run_steps(steps, 0); ref_sol.synchronize()
ref = ref_sol.get_state(); rrem, rng_ = ref_sol.get_path_state()
lo, hi = st.begin, st.begin + st.count
ok = np.array_equal(got['pos'], ref['pos']) and np.array_equal(got['vel'], ref['vel'])
ok = ok and np.array_equal(got['heading'][lo:hi], ref['heading'][lo:hi]) and np.array_equal(got['flags'][lo:hi], ref['flags'][lo:hi])
ok = ok and np.array_equal(grem[lo:hi], rrem[lo:hi]) and np.array_equal(gng[lo:hi], rng_[lo:hi], equal_nan=True)
ok = ok and int(rrem.sum()) < sum(len(p) for p in paths)
print('RANK', rank, 'OK' if ok else 'MISMATCH', flush=True)
dist.destroy_process_group()
sys.exit(0 if ok else 1)
'''


def test_two_ranks_one_gpu_with_paths_equal_one_rank(tmp_path):
    """ShardedStepper(paths=...): every rank holds every list and advances its own shard's; equal to the single-rank run."""
    script = tmp_path / 'worker.py'
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29547')
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                        '--master-addr', '127.0.0.1', '--master-port', '29547', str(script), ROOT],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count('OK') == 2, r.stdout[-3000:]


def _small(S, n=40, pol=1):
    from sca_amd import scenarios
    sc = scenarios.random_cube(n, seed=11)
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
    sol.set_agents(np.full(n, 0.5), np.full(n, 1.0), sc['goal'][:, :3], np.full(n, pol, np.uint8), S.zaxis_flags(sc['start'], sc['goal']),
                   scenarios.max_run_dist(sc['start'], sc['goal']))
    sol.set_state(sc['start'][:, :3], np.zeros((n, 3), np.float32), sc['start'][:, 3:6], np.zeros(n, np.uint8))
    return sol, sc


def test_argument_errors_and_refusals(S):
    from sca_amd import _lib
    L = _lib.lib()
    n = 40
    fresh = S.BatchedSolver(max_agents=n, max_obstacles=1)
    off = np.zeros(n + 1, np.int32)
    pts = np.zeros((1, 3))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))                      # noqa: E731
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                     # noqa: E731
    assert L.sca_set_paths(fresh.ctx, n, ip(off), dp(pts)) == -3               # SCA_ERR_STATE before sca_set_agents
    fresh.close()
    sol, sc = _small(S, n)
    assert L.sca_get_path_state(sol.ctx, None, None) == -3                     # no lists
    bad = [(n - 1, off, pts, 'agent count'), (n, np.r_[1, np.ones(n, np.int32)].astype(np.int32), pts, 'offsets[0]')]
    dec = np.zeros(n + 1, np.int32); dec[5] = 2; dec[6] = 1; dec[6:] = 1
    bad.append((n, dec, np.zeros((2, 3)), 'decrease'))
    one = np.zeros(n + 1, np.int32); one[3:] = 1
    bad.append((n, one, np.array([[0.0, np.inf, 1.0]]), 'not finite'))
    for nn, o, p, what in bad:
        assert L.sca_set_paths(sol.ctx, nn, ip(o), dp(np.ascontiguousarray(p))) == -1, what
        assert what in L.sca_last_error(sol.ctx).decode(), (what, L.sca_last_error(sol.ctx))
        assert L.sca_get_path_state(sol.ctx, None, None) == -3                 # nothing was set
    paths = [[] for _ in range(n)]
    paths[3] = [[1.0, 2.0, 3.0]]
    sol.set_paths(paths)
    # remaining beyond the list, a half-None now_goal
    with pytest.raises(S.ScaError):
        sol.set_path_state(np.full(n, 2, np.int32), np.full((n, 3), np.nan))
    ng = np.full((n, 3), np.nan); ng[0, 1] = 1.0
    with pytest.raises(S.ScaError):
        sol.set_path_state(np.zeros(n, np.int32), ng)
    # sca_set_vpref mode 1 for a straight-line agent with a path: refused; for one without, accepted
    mode = np.zeros(n, np.uint8); mode[3] = 1
    with pytest.raises(S.ScaError, match='waypoint'):
        sol.set_vpref(np.zeros((n, 3)), mode)
    mode[3] = 0; mode[4] = 1
    sol.set_vpref(np.zeros((n, 3)), mode)
    # the cell-owner partition: refused with lists set, and lists refused under it
    with pytest.raises(S.ScaError) as e:
        sol.partition_init(0, 1)
    assert 'rc=-5' in str(e.value)
    sol.set_paths(None)
    sol.partition_init(0, 1)
    with pytest.raises(S.ScaError) as e:
        sol.set_paths(paths)
    assert 'rc=-5' in str(e.value)
    sol.partition_disable()
    sol.close()
    from sca_amd.distributed import PartitionedStepper
    with pytest.raises(ValueError):
        PartitionedStepper(None, 0, 1, None, None, paths=paths)


@pytest.mark.parametrize('mode', [0, 3])
def test_cleared_paths_equal_a_fresh_context(S, mode):
    """sca_set_paths(ctx, 0, NULL, NULL) after a run with lists: from a fresh state, the same episode as a context that never had any --
    and no pass of it reports SCA_FORM_WAYPOINTS."""
    n = 40
    a, sc = _small(S, n, pol=3)
    rng = np.random.default_rng(2)
    a.set_paths([[list(sc['start'][i, :3] + rng.uniform(-3, 3, 3))] * int(rng.integers(0, 3)) for i in range(n)])
    a.run_steps(5, mode); a.synchronize()
    a.set_paths(None)
    a.set_state(sc['start'][:, :3], np.zeros((n, 3), np.float32), sc['start'][:, 3:6], np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.int32))
    b, _ = _small(S, n, pol=3)
    for _ in range(30):
        a.run_steps(1, mode); b.run_steps(1, mode)
        a.synchronize(); b.synchronize()
        assert not a.pass_forms() & S.FORM_WAYPOINTS and not b.pass_forms() & S.FORM_WAYPOINTS
        assert np.array_equal(a.actions(), b.actions())
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    a.close(); b.close()


@pytest.mark.parametrize('mode', [0, 1, 3])
@pytest.mark.parametrize('track', [False, True])
def test_runs_without_paths_never_report_waypoints(S, mode, track):
    n = 64
    sol, sc = _small(S, n, pol=0 if track else 1)
    if track:
        sol.device_tracker_enable(sc['goal'][:, 3:6], in_pass=True)
    for _ in range(3):
        sol.run_steps(2, mode); sol.synchronize()
        assert not sol.pass_forms() & S.FORM_WAYPOINTS
    sol.policy_pass(mode)
    assert not sol.pass_forms() & S.FORM_WAYPOINTS
    sol.close()
