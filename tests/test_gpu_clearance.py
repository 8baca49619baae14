"""Closest approach per agent of a whole context on the device (sca_clearance_enable, k_clearance): the records after every step against
the rule restated in Python (tests/clearance_rule.py) over the positions THE DEVICE ITSELF reports after that step and the flags it
reported before it -- free-running, every comparison equality, nothing expected comes from the code under test.  Sizes either side of
the leaf, the wavefront and the first form switch; kd, AUTO and host-built trees; obstacles, the device tracker, per-agent attributes,
waypoint lists; the tie and the stale-tree scenes; the scene kernel (k_scene_clearance, all pairs) as an independent second
implementation; every step form; the lifecycle; every refusal; the Python layers and the example."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import clearance_rule as R
import clearance_scenes as CS
import edge_corpus as E
import form_fuzz as F
from test_gpu_form_fuzz import S, context_of                                          # noqa: F401 (S: fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 6
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5


def differ(got, want):
    """rows whose records differ; NaN equals NaN (a NaN position is nobody's partner, but the comparison must not trip over one)"""
    bad = np.zeros(len(want), bool)
    for f in want.dtype.names:
        bad |= E.differ(got[f], want[f])
    return np.flatnonzero(bad)


class Run:
    """a context with the feature on, and the Python rule over what the device reports"""

    def __init__(self, S, sol, scene, mode, chunked=False):
        self.S, self.sol, self.s, self.mode, self.chunked = S, sol, scene, mode, chunked
        self.rule = R.empty(scene['n'])
        self.step_no, self.ties, self.flips = 0, [], 0
        self.opos = np.ascontiguousarray(scene['obs_pos'], np.float64).reshape(-1, 3)
        sol.clearance_enable()

    def rule_step(self, flags_before, pos_before, pos_after):
        self.step_no += 1
        if self.chunked:
            CS.all_pairs_chunked(self.rule, pos_after, self.s['radius'], flags_before, self.opos, self.s['obs_radius'], self.step_no, R)
        else:
            R.step(self.rule, pos_after, self.s['radius'], flags_before, self.opos, self.s['obs_radius'], self.step_no, self.ties)
        self.flips += int((CS.nearest(pos_before) != CS.nearest(pos_after)).sum()) if self.s['n'] <= 300 else 0

    def check(self, what):
        got = self.sol.clearance()
        bad = differ(got, self.rule)
        assert bad.size == 0, (what, 'step', self.step_no, bad[:8].tolist(), got[bad[:3]], self.rule[bad[:3]])
        assert not (self.sol.diag()['status'] & 16).any(), (what, 'ST_KD_STACK')

    def steps(self, count, what, stepper=None):
        for _ in range(count):
            before = self.sol.get_state()
            (stepper or (lambda: self.sol.env_step(self.mode)))()
            self.rule_step(before['flags'], before['pos'], self.sol.get_state()['pos'])
            self.check(what)


def mode_of(S, name):
    return {'kd': S.NBR_KDTREE, 'auto': S.NBR_AUTO, 'host': S.NBR_KDTREE_HOSTBUILD, 'grid': S.NBR_GRID}[name]


# ---- records against the Python rule -----------------------------------------------------------------------------------------------------
SIZED = [(n, mode, m) for n in (1, 2, 10, 11, 64, 65, 257, 1024, 2049) for mode, m in (('kd', 0), ('kd', 11), ('auto', 11))] + [(257, 'host', 11), (65, 'auto', 0)]


@pytest.mark.parametrize('n,mode,m', SIZED)
def test_records_free_running(S, n, mode, m):
    scene = CS.sized_scene(n, m)
    sol = context_of(S, scene)
    try:
        run = Run(S, sol, scene, mode_of(S, mode))
        run.steps(STEPS, (n, mode, m))
        if mode == 'auto':
            assert sol.auto_stats()['auto_passes'] >= 1                               # really AUTO passes: their tree comes from the kd stream
        live = scene['flags'] == 0
        assert np.isfinite(run.rule['agent_clear'][live]).all() == (n > 1) and np.isfinite(run.rule['obs_clear'][live]).all() == (m > 0)
    finally:
        sol.close()


def test_records_among_the_1491_spheres_of_the_exp3_map(S):
    scene = E.step_scene('F10_sca_exp3_map', 0)
    assert scene['m'] == 1491
    sol = context_of(S, scene)
    try:
        run = Run(S, sol, scene, S.NBR_KDTREE)
        run.steps(STEPS, 'exp3')
        assert np.isfinite(run.rule['obs_clear']).all() and len(set(run.rule['obs_partner'].tolist())) > 1
    finally:
        sol.close()


def test_records_with_the_device_tracker(S):
    scene = dict(CS.sized_scene(65, 11, seed=1))
    scene['policy'] = np.where(np.arange(65) % 2 == 0, 0, scene['policy']).astype(np.uint8)      # SCA agents: the tracker's
    scene['vmode'] = np.zeros(65, np.uint8)
    scene['key'] = scene['key'] + ('tracked',)
    sol = context_of(S, scene)
    try:
        sol.device_tracker_enable(np.zeros((65, 3)), in_pass=True)
        run = Run(S, sol, scene, S.NBR_KDTREE)
        run.steps(STEPS, 'tracker')
        run.steps(2, 'tracker, a burst', stepper=lambda: (sol.run_steps(1, S.NBR_KDTREE), sol.synchronize()))
    finally:
        sol.close()


@pytest.mark.parametrize('mode', ['kd', 'auto'])
def test_records_with_per_agent_attributes(S, mode):
    seed = 1001
    scene = F.random_scene(seed)
    per_agent = F.per_agent_attributes(seed, scene['n'])
    assert not per_agent[2]
    sol = context_of(S, scene, per_agent=per_agent)
    try:
        Run(S, sol, scene, mode_of(S, mode)).steps(STEPS, ('per agent', mode))
    finally:
        sol.close()


def test_records_with_waypoint_lists(S):
    scene = F.random_scene(7)
    sol = context_of(S, scene, paths=F.random_paths(7, scene))
    try:
        Run(S, sol, scene, S.NBR_KDTREE).steps(STEPS, 'paths')
    finally:
        sol.close()


# ---- special scenes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['F20_edge_lattice4_s2_orca', 'F20_edge_lattice3_s2_a', 'F20_edge_lattice4_s10_mixed', 'F20_edge_coincident_a',
                                  'F20_edge_coincident_b', 'F20_edge_touching_env'])
def test_lattice_and_coincident_scenes(S, name):
    """equal distances to 6 / 12 / 8 partners and coincident agents: the lowest id wins within a step, the earliest step keeps a tie"""
    scene = E.step_scene(name, 0)
    sol = context_of(S, scene)
    try:
        sol.set_kd_perm(scene['perm'])
        run = Run(S, sol, scene, S.NBR_KDTREE)
        run.steps(3, name)
        tied = sum(1 for _, ties, _, _ in run.ties if ties > 1)
        assert tied >= (5 if 'lattice' in name else 0), (name, tied)                    # (the oracle's free run holds 166 / 77 / 10 on the three lattices)
        if 'coincident' in name:
            assert run.rule['agent_clear'].min() < -0.9                                  # agents on top of each other: c < 0 at distance 0
    finally:
        sol.close()


@pytest.mark.parametrize('kind,mode', [('plain', 'kd'), ('pref', 'kd'), ('max_speed', 'kd'), ('pref', 'auto')])
def test_stale_tree(S, kind, mode):
    scene, per_agent = CS.stale_scene(kind)
    sol = context_of(S, scene, per_agent=per_agent)
    try:
        run = Run(S, sol, scene, mode_of(S, mode))
        run.steps(STEPS, ('stale', kind, mode))
        assert run.flips >= 8, run.flips                                              # the nearest partner after the move is not the tree's nearest
    finally:
        sol.close()


# ---- against the scene kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [100, 1536])
def test_a_plain_context_equals_a_batch_of_one_scene(S, n):
    """k_scene_clearance (all pairs, a workgroup per scene) on the same episode: local ids are global ids, the step counts agree"""
    scene = CS.sized_scene(n, 11, seed=2)
    plain, batch = context_of(S, scene), context_of(S, scene, state=False)
    try:
        batch.set_scenes(np.array([0, n], np.int32))
        batch.set_state(scene['pos'], scene['vel'], scene['heading'], scene['flags'], np.zeros(n), np.zeros(n, np.int32))
        batch.set_kd_perm(np.arange(n, dtype=np.int32))
        plain.clearance_enable()
        batch.scene_clearance_enable()
        for k in range(STEPS):
            plain.env_step(S.NBR_KDTREE)
            batch.env_step(S.NBR_KDTREE)
            a, b = plain.clearance(), batch.scene_clearance(0)
            assert differ(a, b).size == 0, (n, k, differ(a, b)[:8].tolist())
        assert np.array_equal(plain.get_state()['pos'], batch.get_state()['pos'])
        assert np.isfinite(a['agent_clear'][scene['flags'] == 0]).all() and a['agent_step'].max() > 1
    finally:
        plain.close()
        batch.close()


# ---- one larger swarm --------------------------------------------------------------------------------------------------------------------
def test_6145_agents_in_auto_mode(S):
    scene = CS.sized_scene(6145, 23)
    sol = context_of(S, scene)
    try:
        Run(S, sol, scene, S.NBR_AUTO, chunked=True).steps(3, 6145)
        assert sol.auto_stats()['auto_passes'] >= 1
    finally:
        sol.close()


# ---- step forms --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['kd', 'auto'])
def test_step_forms(S, mode):
    """six single steps (checked against the rule) and: two bursts of three, policy pass + env update, the host step, the two halves of
    sca_step_begin / sca_step_end -- identical records"""
    scene = CS.sized_scene(257, 11, seed=3)
    m = mode_of(S, mode)
    sols = [context_of(S, scene) for _ in range(5)]
    try:
        single, burst, split, host, halves = sols
        run = Run(S, single, scene, m)
        run.steps(STEPS, ('single', mode))
        for sol in (burst, split, host, halves):
            sol.clearance_enable()
        burst.run_steps(3, m)
        burst.run_steps(3, m)
        burst.synchronize()
        for _ in range(STEPS):
            split.policy_pass(m)
            split.env_update()
        for _ in range(STEPS):
            halves.step_begin(m)
            halves.step_end()
        halves.synchronize()
        host.host_state()
        for k in range(STEPS):
            host.step_host(m, state=k % 2 == 1)                                        # (the block holds the state the step before left)
        want = single.clearance()
        for name, sol in (('run_steps', burst), ('pass + update', split), ('step_host', host), ('step_begin + step_end', halves)):
            got = sol.clearance()
            assert differ(got, want).size == 0, (mode, name, differ(got, want)[:8].tolist())
            assert np.array_equal(sol.get_state()['pos'], single.get_state()['pos']), (mode, name)
        assert want['agent_step'].max() > 3                                           # the second burst's step numbers went on from the first's
    finally:
        for sol in sols:
            sol.close()


# ---- lifecycle ---------------------------------------------------------------------------------------------------------------------------
def test_finished_agents_keep_their_record_and_remain_partners(S):
    scene = dict(CS.sized_scene(11, 0, seed=4))
    scene['pos'] = scene['pos'].copy()
    scene['flags'] = np.zeros(11, np.uint8)
    scene['flags'][1] = 1                                                             # at its goal from the start, right beside agent 0
    scene['pos'][1] = scene['pos'][0] + [0.9, 0.0, 0.0]
    scene['key'] = scene['key'] + ('finished',)
    sol = context_of(S, scene)
    try:
        run = Run(S, sol, scene, S.NBR_KDTREE)
        run.steps(2, 'finished')
        rec = sol.clearance()
        assert rec['agent_partner'][0] == 1 and rec['agent_partner'][1] == -1 and np.isinf(rec['agent_clear'][1]) and rec['agent_step'][1] == 0
        flags = sol.get_state()['flags']
        flags[0] |= 4                                                                 # agent 0 times out: from now on its record stays
        st = sol.get_state()
        sol.set_state(st['pos'], st['vel'], st['heading'], flags, st['total_dist'], st['step_num'])
        assert differ(sol.clearance(), rec).size == 0                                 # a new state leaves the records alone
        run.steps(2, 'finished, later')
        after = sol.clearance()
        assert after[0] == rec[0] and after['agent_step'].max() >= 3                  # ... and the step count goes on
    finally:
        sol.close()


def test_enabling_again_starts_over(S):
    scene = CS.sized_scene(64, 11, seed=5)
    sol = context_of(S, scene)
    try:
        run = Run(S, sol, scene, S.NBR_KDTREE)
        run.steps(3, 'first')
        sol.clearance_enable()
        assert differ(sol.clearance(), R.empty(64)).size == 0
        run.rule, run.step_no = R.empty(64), 0
        run.steps(2, 'again')
        assert sol.clearance()['agent_step'].max() <= 2
        sol.clearance_enable(False)
        with pytest.raises(S.ScaError, match='sca_clearance_enable first'):
            sol.clearance()
        sol.env_step(S.NBR_GRID)                                                      # off: nothing is refused
    finally:
        sol.close()


@pytest.mark.parametrize('mode', ['kd', 'auto'])
def test_a_twin_without_the_feature_ends_in_the_same_state(S, mode):
    scene = F.random_scene(7)
    paths = F.random_paths(7, scene)
    on, off = context_of(S, scene, paths=paths), context_of(S, scene, paths=paths)
    try:
        on.clearance_enable()
        for sol in (on, off):
            sol.run_steps(2, mode_of(S, mode))
            for _ in range(3):
                sol.env_step(mode_of(S, mode))
        a, b = on.get_state(), off.get_state()
        for k in a:
            assert E.same(a[k], b[k]), (mode, k)
        assert E.same(on.actions(), off.actions())
        na, nb = on.neighbors(), off.neighbors()
        for k in na:
            assert E.same(na[k], nb[k]), (mode, 'lists', k)
        pa, pb = on.get_path_state(), off.get_path_state()
        assert all(E.same(x, y) for x, y in zip(pa, pb))
        assert np.array_equal(on.diag()['status'], off.diag()['status'])
    finally:
        on.close()
        off.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(S):
    from sca_amd import _lib
    scene = CS.sized_scene(10, 1, seed=6)
    n = 10
    rec = np.zeros(n, _lib.CLEARANCE_DTYPE)
    out = rec.ctypes.data_as(C.POINTER(_lib.SceneClearance))
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    L, ctx = sol.L, sol.ctx
    err = lambda: L.sca_last_error(ctx).decode()
    try:
        assert L.sca_clearance_enable(ctx, 1) == ERR_STATE and 'sca_set_agents' in err()             # no agents
        assert L.sca_get_clearance(ctx, 0, 0, out, 32) == ERR_STATE
        sol.set_obstacles(scene['obs_pos'], scene['obs_radius'])
        sol.set_agents(scene['radius'], scene['pref_speed'], scene['goal'], scene['policy'], F.zaxis_of(scene), scene['max_run_dist'])
        assert L.sca_clearance_enable(ctx, 1) == ERR_STATE and 'state' in err()                      # no state
        state = lambda: sol.set_state(scene['pos'], scene['vel'], scene['heading'], scene['flags'], np.zeros(n), np.zeros(n, np.int32))
        state()
        sol.policy_pass(S.NBR_KDTREE)
        assert L.sca_clearance_enable(ctx, 1) == ERR_STATE and 'between a policy pass' in err()      # mid-step
        assert L.sca_clearance_enable(ctx, 0) == ERR_STATE
        sol.env_update()
        # what excludes the feature
        sol.set_scenes(np.array([0, 4, n], np.int32))
        assert L.sca_clearance_enable(ctx, 1) == ERR_UNSUPPORTED and 'sca_scene_clearance_enable' in err()
        sol.set_scenes(None)
        sol.set_shard(0, n - 1)
        assert L.sca_clearance_enable(ctx, 1) == ERR_UNSUPPORTED and 'shard' in err()
        sol.set_shard(0, n)
        sol.partition_init(0, 1)
        assert L.sca_clearance_enable(ctx, 1) == ERR_UNSUPPORTED and 'partition' in err()
        sol.partition_disable()
        assert L.sca_get_clearance(ctx, 0, n, out, 32) == ERR_STATE and 'sca_clearance_enable first' in err()
        # on
        assert L.sca_clearance_enable(ctx, 1) == 0
        for a, b in ((-1, 1), (0, n + 1), (n, 1), (n + 1, 0), (0, -1)):
            assert L.sca_get_clearance(ctx, a, b, out, 32) == ERR_ARG, (a, b)
        assert L.sca_get_clearance(ctx, 0, n, None, 32) == ERR_ARG and 'NULL' in err()
        assert L.sca_get_clearance(ctx, 0, n, out, 24) == ERR_ARG and 'struct_bytes' in err()
        assert L.sca_get_clearance(ctx, 0, n, out, 32) == 0 and L.sca_get_clearance(ctx, n, 0, out, 32) == 0 and L.sca_get_clearance(ctx, 3, 2, out, 32) == 0
        # while on: no agent tree of this step
        active = C.c_int(0)
        before = sol.get_state()
        assert L.sca_env_step(ctx, S.NBR_GRID, C.byref(active)) == ERR_UNSUPPORTED and 'SCA_NBR_GRID' in err()
        assert L.sca_run_steps(ctx, 2, S.NBR_GRID) == ERR_UNSUPPORTED
        assert L.sca_policy_pass(ctx, S.NBR_GRID) == ERR_UNSUPPORTED
        assert L.sca_step_host(ctx, S.NBR_GRID, 0, C.byref(active)) == ERR_UNSUPPORTED
        assert L.sca_env_update(ctx, None) == ERR_UNSUPPORTED and 'no policy pass' in err()
        assert L.sca_step_end(ctx) == ERR_UNSUPPORTED and L.sca_step_begin(ctx, S.NBR_GRID) == ERR_UNSUPPORTED
        after = sol.get_state()
        assert all(E.same(before[k], after[k]) for k in before)                                     # refused before anything was enqueued
        # while on: what would take the whole swarm away from this rank
        assert L.sca_set_shard(ctx, 0, n - 1) == ERR_UNSUPPORTED and L.sca_set_shard(ctx, 0, n) == 0
        uid = (C.c_char * 128)()
        assert L.sca_comm_init(ctx, 0, 1, uid) == ERR_UNSUPPORTED and 'communicator' in err()
        assert L.sca_partition_init(ctx, 0, 1, 0, None, 0, 0) == ERR_UNSUPPORTED and 'partition' in err()
        off = np.array([0, 4, n], np.int32)
        assert L.sca_set_scenes(ctx, 2, off.ctypes.data_as(C.POINTER(C.c_int32))) == ERR_UNSUPPORTED and 'scenes' in err()
        # still usable, and the records are those of the steps that ran
        sol.env_step(S.NBR_KDTREE)
        assert sol.clearance()['agent_step'].max() == 1
        state()                                                                                     # a new state: the records stay
        assert sol.clearance()['agent_step'].max() == 1
        # a new agent set drops them
        sol.set_agents(scene['radius'], scene['pref_speed'], scene['goal'], scene['policy'], F.zaxis_of(scene), scene['max_run_dist'])
        assert L.sca_get_clearance(ctx, 0, n, out, 32) == ERR_STATE
        state()
        sol.env_step(S.NBR_GRID)                                                                    # ... and nothing is refused any more
    finally:
        sol.close()


# ---- the Python layers -------------------------------------------------------------------------------------------------------------------
def test_macaenv_and_the_metrics(S):
    from sca_amd import env as EV, metrics
    envs = []
    for clearance in (True, False):
        agents = EV.build_circle_agents(24, policy=EV.ORCA3DPolicy, rad=6.0)
        obstacles = [EV.Obstacle(pos=[0.0, 0.0, 10.0], shape_dict={'shape': 'sphere', 'feature': 1.0}, id=0)]
        env = EV.MACAEnv(clearance=clearance)
        env.set_agents(agents, obstacles=obstacles)
        envs.append(env)
    on, off = envs
    pos = [on.pos.copy()]
    flags = [on.flags.copy()]
    for _ in range(12):
        on.step({})
        off.step({})
        pos.append(on.pos.copy())
        flags.append(on.flags.copy())
    assert np.array_equal(on.pos, off.pos) and np.array_equal(on.flags, off.flags)
    with pytest.raises(RuntimeError, match='clearance=True'):
        off.clearance
    want = R.empty(24)
    radius = np.full(24, 0.5)
    for k in range(12):
        R.step(want, pos[k + 1], radius, flags[k], np.array([[0.0, 0.0, 10.0]]), np.array([1.0]), k + 1)
    rec = on.clearance
    assert differ(rec, want).size == 0
    m = metrics.clearance_metrics(on, margin=0.5)
    assert m == metrics.clearance_metrics(rec, margin=0.5)
    a = int(np.argmin(want['agent_clear']))
    assert m['MinClearance'] == want['agent_clear'].min() and m['MinClearancePair'] == (a, int(want['agent_partner'][a])) and m['MinClearanceStep'] == want['agent_step'][a]
    o = int(np.argmin(want['obs_clear']))
    assert m['MinObstacleClearance'] == want['obs_clear'].min() and m['MinObstacleClearanceAgent'] == o and m['MinObstacleClearanceObstacle'] == 0
    assert m['NearMisses'] == np.flatnonzero(np.minimum(want['agent_clear'], want['obs_clear']) <= 0.5).tolist()
    for env in envs:
        env.solver.close()


def test_the_example_prints_the_minima(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, 'examples', 'run_sca.py'), '--agents', '100', '--policy', 'orca', '--no-obstacles', '--max-steps', '40',
           '--log-dir', str(tmp_path), '--clearance', '--margin', '0.25']
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("{'MinClearance'")]
    assert len(at) == 1 and lines[at[0] - 1].startswith("{'SuccessRate'") and lines[at[0] + 1].startswith('wrote'), r.stdout
    for key in ('MinClearancePair', 'MinClearanceStep', 'MinObstacleClearance', 'NearMisses'):
        assert key in lines[at[0]]
    assert "'MinObstacleClearance': inf" in lines[at[0]]                               # no obstacles: the empty half
