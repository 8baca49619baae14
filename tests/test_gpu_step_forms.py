"""A burst equals single steps, bit for bit (-m gpu).  sca_run_steps knows what follows a step and lets events ride on kernels the step
launches anyway -- the moved positions' event on k_action, the next pass's fork on the step's last kernel (K4, k_scene_harvest or
k_goal_flags_others) -- or builds the next tree ahead (plan_step / plan_finish, sca_forms.h; tests/test_forms_cpu.py has the rule).  The
single-step entry points plan none of that, so run_steps(k) against k single steps in every form checks each branch of the plan against
the branch-free path.  Every row is the smallest shape that takes its branch; bursts of 1, 3 and 2 in a row, so that a fork or a tree
left over between calls would show.  (The tracked kd and the AUTO bursts under SCA_EXT_STOP=0 at larger sizes:
tests/test_gpu_auto.py::test_events_as_stop_events_change_no_bit.)"""
import numpy as np
import pytest

from scene_util import circle_scene, context
from test_gpu_auto import _scene, _solver

pytestmark = pytest.mark.gpu

BURSTS = (1, 3, 2)
SINGLE_FORMS = ('single', 'halves', 'pass_update', 'env_step')


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


def _plain(kind, n, tracked):
    sc, pol, n = _scene(kind, n, seed=13)
    return _solver(sc, pol, n, tracked)


def _scenes(S, obstacles):
    eps = [circle_scene(S, 16, 0, turn=t) for t in range(4)]
    sets = [(ep['pos'].mean(0)[None] + [[0.3 * (t + 1), 0.2, 0.1]], np.array([0.5])) for t, ep in enumerate(eps)] if obstacles else None
    sol, _ = context(S, eps, obstacles=sets, tracker=True)
    sol.scene_harvest_enable()
    return sol


def build(S, row):
    """(solver, neighbour mode)"""
    if row == 'tracked_kd':                                        # the fork rides on K4
        return _plain('circle', 256, True), S.NBR_KDTREE
    if row == 'shard':                                             # ... on k_goal_flags_others
        sol = _plain('circle', 256, True)
        sol.set_shard(0, 128); sol.set_shard_emulation(True)
        return sol, S.NBR_KDTREE
    if row == 'scenes_harvest':                                    # ... on k_scene_harvest
        return _scenes(S, False), S.NBR_KDTREE
    if row == 'scene_obstacles':                                   # the SceneObsRoots instance of K4
        return _scenes(S, True), S.NBR_KDTREE
    if row == 'paths':                                             # waypoint lists on a quarter of the agents (RVO3D beside the tracked ones): no fork ahead
        sc, pol, n = _scene('circle', 256, seed=13)
        pol[::4] = 1
        sol = _solver(sc, pol, n, True)
        s, g = sc['start'][:, :3], sc['goal'][:, :3]
        sol.set_paths([[list(g[i]), list(np.round(s[i] + 0.5 * (g[i] - s[i]) + [1.5, -1.0, 0.5], 2))] if i % 4 == 0 else [] for i in range(n)])
        return sol, S.NBR_KDTREE
    if row.startswith('auto'):                                     # an event on k_action and a build ahead; with the closest-approach records on: no build ahead
        sol = _plain('cube' if 'cube' in row else 'dense', 512 if 'cube' in row else 400, False)
        if row.endswith('clear'):
            sol.clearance_enable()
        return sol, S.NBR_AUTO
    assert row == 'grid'                                           # the grid instance of K4
    return _plain('cube', 512, False), S.NBR_GRID


# (the shard's stand-in for the exchange is sca_run_steps' own: the two forms that step outside it are no forms of that row)
ROWS = ('tracked_kd', 'shard', 'scenes_harvest', 'scene_obstacles', 'paths', 'auto_cube', 'auto_dense', 'auto_cube_clear', 'auto_dense_clear', 'grid')


def snapshot(sol):
    sol.synchronize()
    out = dict(sol.get_state())
    out.update(action=sol.actions(), nbr_id=sol.neighbors()['nbr_id'], perm=sol.get_kd_perm())
    return out


def advance(sol, form, k, mode):
    if form == 'burst':
        return sol.run_steps(k, mode)
    for _ in range(k):
        if form == 'single':
            sol.run_steps(1, mode)
        elif form == 'halves':
            sol.step_begin(mode); sol.step_end()
        elif form == 'pass_update':
            sol.policy_pass(mode); sol.env_update()
        else:
            sol.env_step(mode)


def run(S, row, form):
    sol, mode = build(S, row)
    shots = []
    for k in BURSTS:
        advance(sol, form, k, mode)
        shots.append(snapshot(sol))
    sol.close()
    return shots


_burst = {}


def burst_of(S, row):
    """the burst's snapshots, computed once per row"""
    if row not in _burst:
        _burst[row] = run(S, row, 'burst')
    return _burst[row]


def assert_same(got, want, ctx):
    assert len(got) == len(want)
    for at, (a, b) in enumerate(zip(got, want)):
        for key in b:
            assert np.array_equal(a[key], b[key]), ctx + (BURSTS[at], key, int((np.asarray(a[key]) != np.asarray(b[key])).sum()))


@pytest.mark.parametrize('row,form', [(r, f) for r in ROWS for f in SINGLE_FORMS if not (r == 'shard' and f in ('halves', 'pass_update'))])
def test_a_burst_equals_single_steps(S, row, form):
    moved = burst_of(S, row)
    assert not np.array_equal(moved[0]['pos'], moved[-1]['pos'])   # (the row does step)
    assert_same(run(S, row, form), moved, (row, form))


@pytest.mark.parametrize('row', ('shard', 'scenes_harvest', 'scene_obstacles', 'paths', 'auto_dense_clear', 'grid'))
def test_events_as_records_of_their_own_change_no_bit_in_any_carrier(S, row, monkeypatch):
    """SCA_EXT_STOP=0 (read at sca_create): every event a record of its own behind its kernel instead of the kernel's stop event -- the same
    bits in the rows whose carrier test_gpu_auto.py's test does not reach"""
    monkeypatch.setenv('SCA_EXT_STOP', '0')
    got = run(S, row, 'burst')
    monkeypatch.delenv('SCA_EXT_STOP')
    assert_same(got, burst_of(S, row), (row, 'SCA_EXT_STOP=0'))


@pytest.mark.parametrize('row', ('tracked_kd', 'auto_cube'))
def test_a_refused_burst_leaves_nothing_behind(S, row):
    """a negative step count and a mode out of range are refused before anything is enqueued: in front of the first burst and between two
    bursts, the context goes on as one that never saw them"""
    sol, mode = build(S, row)
    shots = []
    for k in BURSTS:
        for bad in ((-1, mode), (2, 7), (2, -1)):
            with pytest.raises(S.ScaError):
                sol.run_steps(*bad)
        sol.run_steps(k, mode)
        shots.append(snapshot(sol))
    sol.close()
    assert_same(shots, burst_of(S, row), (row, 'refused calls in between'))
