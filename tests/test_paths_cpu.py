"""Waypoint lists (Agent.path) without a GPU: the restatement of the rule (tests/path_rule.py) against the reference-recorded F19 fixtures,
the host build of sca_core.h's waypoint helpers against the restatement, and the C-ABI entries of sca_set_paths & co."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import path_rule as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS_DIR = os.path.join(ROOT, 'tests', 'golden', 'paths')


def path_fixtures():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(PATHS_DIR, 'F19_path_*.npz')))


def load(name):
    return dict(np.load(os.path.join(PATHS_DIR, name + '.npz'), allow_pickle=False))


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_the_five_fixtures_are_there():
    assert path_fixtures() == ['F19_path_edge10', 'F19_path_orca_circle16_obs', 'F19_path_orcalp_random30', 'F19_path_rvo_circle16',
                               'F19_path_srvo_circle16']
    for nm in path_fixtures():
        assert os.path.getsize(os.path.join(PATHS_DIR, nm + '.npz')) < 1 << 20


@pytest.mark.parametrize('name', path_fixtures())
def test_restatement_reproduces_every_recorded_step(name):
    """From each recorded pre-step state (positions, flags, now_goal, what is left of every list): the rule gives the recorded now_goal and
    list lengths after the step, and the straight-line agents with a path the recorded v_pref, bit for bit."""
    fx = load(name)
    off, pts = fx['path_off'], fx['path_pts']
    has_path = np.diff(off) > 0
    goal = fx['goal6'][:, :3]
    popped = 0
    for k in range(len(fx['step'])):
        paths = R.lists_from_csr(off, pts, fx['path_left_before'][k])
        ng = fx['now_goal_before'][k].copy()
        vp, mode = R.pass_rule(paths, ng, fx['pos'][k], goal, fx['radius'], fx['pref_speed'], fx['policy'], fx['flags'][k], has_path)
        ctx = (name, int(fx['step'][k]))
        assert same(ng, fx['now_goal_after'][k]), ctx
        assert np.array_equal([len(p) for p in paths], fx['path_left_after'][k]), ctx
        use = mode.astype(bool) & fx['called'][k].astype(bool)
        assert np.array_equal(vp[use], fx['vpref'][k][use]), ctx
        popped += int((fx['path_left_before'][k] - fx['path_left_after'][k]).sum())
    assert popped > 0, name


def test_edge_scene_covers_the_quirks():
    fx = load('F19_path_edge10')
    off = fx['path_off']
    lens = np.diff(off)
    left0 = fx['path_left_after'][0]
    assert lens[0] == 0 and np.array_equal(fx['now_goal_after'][0][0], fx['goal6'][0, :3])        # empty list: now_goal = goal
    assert lens[2] == 2 and left0[2] == 0                                                            # first call pops twice (within radius)
    assert lens[3] == 2 and left0[3] == 0                                                            # ... and through the elif branch
    assert lens[1] == 1 and left0[1] == 0                                                            # a single waypoint: one pop
    # the waypoint popped last is aimed at for exactly one pass: once the list is empty, the next pass makes now_goal the goal
    k = next(k for k in range(1, len(fx['step'])) if fx['path_left_before'][k][1] == 0)
    assert np.array_equal(fx['now_goal_after'][k][1], fx['goal6'][1, :3])
    # reached its goal with waypoints left
    assert fx['flags_after'][-1][8] & 1 and fx['path_left_after'][-1][8] > 0
    # the tracked agents' lists advance as well
    assert fx['path_left_after'][-1][6] < lens[6] and fx['path_left_after'][-1][7] < lens[7]
    # the duplicates are popped one by one
    assert lens[4] == 3 and 0 in {int(x) for x in fx['path_left_after'][:, 4]}


# ---- host build of the sca_core.h helpers ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def harness():
    out = os.path.join(ROOT, 'tests', '_build', 'libpath_harness.so')
    src = os.path.join(ROOT, 'tests', 'path_harness.cpp')
    hdrs = [os.path.join(ROOT, 'sca_amd', 'csrc', h) for h in ('sca_core.h', 'sca_glibc_math.h', 'sca_glibc_tables.h')]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(['g++', '-std=c++17', '-fPIC', '-shared', '-O2', '-ffp-contract=off', '-mfma', '-fno-builtin-pow',
                               '-I' + os.path.join(ROOT, 'sca_amd', 'csrc'), '-o', out, src])
    H = C.CDLL(out)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    H.path_advance.restype = None
    H.path_advance.argtypes = [dp, ip, dp, dp, dp, C.c_double, C.c_int]
    H.path_vpref.restype = None
    H.path_vpref.argtypes = [dp, dp, dp, C.c_double, C.c_int, dp]
    return H


def _p(a, t=C.c_double):
    return a.ctypes.data_as(C.POINTER(t))


def harness_advance(H, pts, rem, ng, pos, goal, radius, policy):
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1)
    r = np.array([rem], np.int32)
    g = np.ascontiguousarray(ng, np.float64).copy()
    H.path_advance(_p(pts) if len(pts) else None, _p(r, C.c_int32), _p(g), _p(np.ascontiguousarray(pos, np.float64)),
                   _p(np.ascontiguousarray(goal, np.float64)), float(radius), int(policy in R.ORCA))
    return int(r[0]), g


def harness_vpref(H, aim, pos, goal, ps, policy):
    out = np.zeros(3)
    H.path_vpref(_p(np.ascontiguousarray(aim, np.float64)), _p(np.ascontiguousarray(goal, np.float64)),
                 _p(np.ascontiguousarray(pos, np.float64)), float(ps), int(policy in R.ORCA), out.ctypes.data_as(C.POINTER(C.c_double)))
    return out


def _check_one(H, path, ng, pos, goal, radius, ps, policy):
    pts = np.array(path, dtype=np.float64).reshape(-1, 3)
    lst = [list(w) for w in path]
    want = R.advance(lst, None if np.isnan(ng[0]) else ng.copy(), pos, goal, radius, policy)
    rem, got = harness_advance(H, pts, len(path), ng, pos, goal, radius, policy)
    assert rem == len(lst) and np.array_equal(got, np.asarray(want, np.float64)), (path, ng, pos, goal, radius, policy)
    assert np.array_equal(harness_vpref(H, got, pos, goal, ps, policy), R.v_pref_toward(want, pos, goal, ps, policy))


def test_host_build_agrees_with_the_restatement_on_random_cases(harness):
    rng = np.random.default_rng(1901)
    for t in range(4000):
        policy = int(rng.integers(0, 6))
        radius = float(rng.choice([0.3, 0.5, 1.0, 2.0]))
        pos = np.round(rng.uniform(-5, 5, 3), int(rng.integers(1, 6)))
        goal = np.round(rng.uniform(-5, 5, 3), 2)
        k = int(rng.integers(0, 5))
        path = [list(np.round(pos + rng.normal(0, radius * 1.5, 3), 3)) if rng.random() < 0.4 else list(np.round(rng.uniform(-6, 6, 3), 2))
                for _ in range(k)]
        if k and rng.random() < 0.2:
            path[-1] = list(goal)
        ng = np.full(3, np.nan) if rng.random() < 0.5 else np.round(rng.uniform(-5, 5, 3), 3)
        _check_one(harness, path, ng, pos, goal, radius, float(rng.choice([0.8, 1.0, 1.3])), policy)


@pytest.mark.parametrize('name', path_fixtures())
def test_host_build_agrees_with_the_restatement_on_fixture_states(harness, name):
    fx = load(name)
    off, pts = fx['path_off'], fx['path_pts']
    goal = fx['goal6'][:, :3]
    for k in range(0, len(fx['step']), 3):
        for i in range(len(off) - 1):
            if fx['flags'][k][i] & 7:
                continue
            path = R.lists_from_csr(off, pts, fx['path_left_before'][k])[i]
            _check_one(harness, path, fx['now_goal_before'][k][i], fx['pos'][k][i], goal[i], float(fx['radius'][i]),
                       float(fx['pref_speed'][i]), int(fx['policy'][i]))


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------------------
def test_path_entry_points_are_exported_and_declared():
    from sca_amd import _lib
    from sca_amd import solver as S
    L = _lib.lib()
    for nm in ('sca_set_paths', 'sca_get_path_state', 'sca_set_path_state'):
        assert hasattr(L, nm) and nm in _lib.SIGNATURES, nm
    assert L.sca_version() == 103
    hdr = open(os.path.join(ROOT, 'include', 'sca_hip.h')).read()
    assert '#define SCA_FORM_WAYPOINTS 256' in hdr and S.FORM_WAYPOINTS == 256


def test_paths_csr_round_trip():
    from sca_amd.solver import paths_csr
    paths = [[], [[1, 2, 3]], [[0, 0, 0], [4.5, 5, 6]], []]
    off, pts = paths_csr(paths)
    assert off.tolist() == [0, 0, 1, 3, 3] and pts.shape == (3, 3)
    assert R.lists_from_csr(off, pts) == [[list(map(float, w)) for w in p] for p in paths]


@pytest.mark.parametrize('name', path_fixtures())
def test_array_form_of_the_rule_equals_the_loop(name):
    """pass_rule_csr (what the GPU tests at 16 384 / 100 000 agents feed the oracle from) against pass_rule on every recorded step"""
    fx = load(name)
    off, pts = fx['path_off'], fx['path_pts']
    goal = fx['goal6'][:, :3]
    for k in range(len(fx['step'])):
        paths = R.lists_from_csr(off, pts, fx['path_left_before'][k])
        ng = fx['now_goal_before'][k].copy()
        vp, mode = R.pass_rule(paths, ng, fx['pos'][k], goal, fx['radius'], fx['pref_speed'], fx['policy'], fx['flags'][k], np.diff(off) > 0)
        rem2, ng2, vp2, mode2 = R.pass_rule_csr(off, pts, fx['path_left_before'][k], fx['now_goal_before'][k], fx['pos'][k], goal,
                                                fx['radius'], fx['pref_speed'], fx['policy'], fx['flags'][k])
        assert np.array_equal(rem2, [len(p) for p in paths]) and same(ng2, ng) and np.array_equal(mode2, mode)
        assert vp2[mode2.astype(bool)].tobytes() == vp[mode.astype(bool)].tobytes()                # (bytes: -0.0 is not 0.0)


def test_array_form_of_the_rule_equals_the_loop_on_random_swarms():
    rng = np.random.default_rng(77)
    for t in range(20):
        n = 300
        pos = np.round(rng.uniform(-8, 8, (n, 3)), 3)
        goal = np.round(rng.uniform(-8, 8, (n, 3)), 2)
        paths = [[list(np.round(pos[i] + rng.normal(0, 1.0, 3), 2)) for _ in range(int(rng.integers(0, 7)))] for i in range(n)]
        off, pts = R.csr(paths)
        ng = np.where(rng.random((n, 1)) < 0.5, np.nan, np.round(rng.uniform(-8, 8, (n, 3)), 2))
        radius, ps = rng.choice([0.3, 0.5, 1.0], n), rng.choice([0.8, 1.0, 1.3], n)
        policy, flags = rng.integers(0, 6, n), (rng.random(n) < 0.1).astype(np.uint8)
        rem2, ng2, vp2, mode2 = R.pass_rule_csr(off, pts, np.diff(off), ng, pos, goal, radius, ps, policy, flags)
        vp, mode = R.pass_rule(paths, ng, pos, goal, radius, ps, policy, flags, np.diff(off) > 0)
        assert np.array_equal(rem2, [len(p) for p in paths]) and same(ng2, ng) and np.array_equal(mode2, mode)
        assert vp2.tobytes() == vp.tobytes()
