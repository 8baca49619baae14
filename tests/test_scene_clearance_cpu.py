"""Closest approach per agent without a GPU: the record's layout, the host-side rule of sca_scenes.h (scene_clearance_step, over the
per-pair function the kernel runs) behind tests/scene_clearance_harness.cpp against the rule restated in Python (tests/clearance_rule.py)
on the reference's recorded episodes, what that corpus holds, metrics.merge_clearance, and the rule as a program of its own under the
sanitizers.  Every comparison is equality; no expected value comes from the code under test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import clearance_rule as R
import harness_util
from golden_util import episode_fixtures, load

OK, NO_SCENES, MID_STEP, OFF, BAD_SCENE, NO_OUT, BAD_STRUCT = range(7)     # ClearFault
ERR_ARG, ERR_STATE = -1, -3                                        # include/sca_hip.h
CORPUS = ['F2_orcalp_circle100', 'F4_sca_takeoff16', 'F16_params_timestep02', 'F14_fuzz_episode_02', 'F9_hetero_mixed60', 'F10_sca_exp3_map',
          'F1_sca_circle8']


SRC = os.path.join(harness_util.ROOT, 'tests', 'scene_clearance_harness.cpp')
# the arithmetic of sca_core.h as the library builds it (unfused; the restated libm with -mfma); the header's `#pragma unroll` is hipcc's
FLAGS = ['-std=c++17', '-ffp-contract=off', '-mfma', '-fno-builtin-pow', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I' + harness_util.CSRC]


@pytest.fixture(scope='module')
def H():
    out = os.path.join(harness_util.BUILD, 'libscene_clearance_harness.so')
    deps = [SRC, os.path.join(harness_util.ROOT, 'include', 'sca_hip.h')] + \
        [os.path.join(harness_util.CSRC, f) for f in ('sca_scenes.h', 'sca_core.h', 'sca_glibc_math.h', 'sca_glibc_tables.h', 'sca_constants.h')]
    os.makedirs(harness_util.BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(['g++', '-O2', '-fPIC', '-shared'] + FLAGS + ['-o', out, SRC])
    return C.CDLL(out)


_RULE = {}


def python_rule(name):
    """the Python rule over a recorded episode, made once: (the fixture, the records after every step, (step, agent, partners that share
    the step's agent minimum, that minimum, the step's obstacle minimum) per updated agent)"""
    if name not in _RULE:
        fx = load(name)
        after, ties = [], []
        R.over_records(fx, per_step=lambda k, rec: after.append(rec.copy()), count_ties=ties)
        _RULE[name] = (fx, after, ties)
    return _RULE[name]


def test_the_struct_and_the_dtype(H):
    from sca_amd import _lib
    assert H.sclr_struct_bytes() == 32 == C.sizeof(_lib.SceneClearance) == _lib.CLEARANCE_DTYPE.itemsize
    assert _lib.CLEARANCE_DTYPE == R.DTYPE
    assert [(n, _lib.CLEARANCE_DTYPE.fields[n][1]) for n in _lib.CLEARANCE_DTYPE.names] == \
        [('agent_clear', 0), ('obs_clear', 8), ('agent_partner', 16), ('agent_step', 20), ('obs_partner', 24), ('obs_step', 28)]
    assert [(n, getattr(_lib.SceneClearance, n).offset) for n, _ in _lib.SceneClearance._fields_] == \
        [('agent_clear', 0), ('obs_clear', 8), ('agent_partner', 16), ('agent_step', 20), ('obs_partner', 24), ('obs_step', 28)]
    rec = np.zeros(3, R.DTYPE)
    H.sclr_empty(rec.ctypes.data_as(C.c_void_p), 3)
    assert np.array_equal(rec, R.empty(3))
    assert rec['agent_clear'][0] == np.inf and rec['agent_partner'][0] == -1 and rec['agent_step'][0] == 0


@pytest.mark.parametrize('name', CORPUS)
def test_host_rule_equals_the_python_rule_on_the_recordings(H, name):
    fx, after, _ = python_rule(name)
    n, m = len(fx['radius']), len(fx['obs_radius'])
    rec = R.empty(n)
    radius, opos, orad = np.ascontiguousarray(fx['radius']), np.ascontiguousarray(fx['obs_pos'].reshape(-1, 3)), np.ascontiguousarray(fx['obs_radius'])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for k in range(len(after)):
        pos, flags = np.ascontiguousarray(fx['pos_after'][k]), np.ascontiguousarray(fx['flags'][k], np.uint32)
        H.sclr_step(n, dp(pos), dp(radius), flags.ctypes.data_as(C.POINTER(C.c_uint32)), m, dp(opos), dp(orad), k + 1, rec.ctypes.data_as(C.c_void_p))
        assert np.array_equal(rec, after[k]), (name, 'step', k + 1, np.flatnonzero(rec != after[k]).tolist())


def test_what_the_corpus_holds():
    """the cases the comparisons above rest on, evaluated with the Python rule: they cannot silently vanish from the fixtures"""
    fx, after, ties = python_rule('F2_orcalp_circle100')
    assert sum(1 for _, _, t, _, _ in ties if t == 2) == 72 and not any(t > 2 for _, _, t, _, _ in ties)
    fx, after, ties = python_rule('F4_sca_takeoff16')
    assert sum(1 for _, _, t, _, _ in ties if t == 2) == 61 and len(after) == 285 and len(fx['obs_radius']) == 8
    fx, after, _ = python_rule('F16_params_timestep02')
    assert int((after[-1]['agent_clear'] <= 0).sum()) == 22 and after[-1]['agent_clear'].min() == -0.71848
    fx, after, _ = python_rule('F14_fuzz_episode_02')
    assert round(float(after[-1]['obs_clear'].min()), 9) == -0.73147
    fx, after, _ = python_rule('F9_hetero_mixed60')
    assert round(float(after[-1]['agent_clear'].min()), 9) == -0.179 and round(float(after[-1]['obs_clear'].min()), 9) == -1.63437
    fx, after, _ = python_rule('F10_sca_exp3_map')
    assert len(fx['obs_radius']) == 1491
    assert round(float(after[-1]['agent_clear'].min()), 9) == 0.1059 and round(float(after[-1]['obs_clear'].min()), 9) == 0.10227
    fx, after, _ = python_rule('F1_sca_circle8')
    assert len(after) == 246
    assert np.isinf(after[-1]['obs_clear']).all() and (after[-1]['obs_partner'] == -1).all() and not after[-1]['obs_step'].any()


def test_a_clearance_at_or_below_zero_goes_with_the_collision_flag():
    """Over all whole-episode fixtures of at most 130 agents: a step minimum <= 0, agent or obstacle, of an agent that entered the step
    unfinished means the collision flag after that step (mampenv.py:61-75 is the same test).  The converse is not claimed:
    F6_orcalp_circle100_long ends with 47 collided agents at a minimum of +0.00613 -- flagged by the neighbour insertion's unrounded test."""
    names = [n for n in episode_fixtures() if R.whole_episode(load(n)) and len(load(n)['radius']) <= 130]
    assert len(names) >= 60 and all(c in names for c in CORPUS)
    touching = 0
    for name in names:
        fx, _, ties = python_rule(name)
        for k, a, _, c_agent, c_obs in ties:
            if min(c_agent, c_obs) <= 0:
                touching += 1
                assert fx['flags_after'][k][a] & 2, (name, k, a, c_agent, c_obs)
    assert touching >= 22
    fx = load('F6_orcalp_circle100_long')
    rec = R.over_records(fx)                                       # (its records are every tenth step: the rule over those positions alone)
    assert int(((fx['flags_after'][-1] & 2) != 0).sum()) == 47 and round(float(rec['agent_clear'].min()), 9) == 0.00613


def test_merge_clearance_on_hand_made_records():
    from sca_amd import metrics
    before, after = R.empty(5), R.empty(5)
    before[0] = (1.5, 2.0, 3, 10, 1, 12)
    after[0] = (1.25, 2.5, 4, 30, 0, 31)                           # the agent half is smaller later, the obstacle half is not
    before[1] = (0.5, 0.75, 2, 7, 0, 8)
    after[1] = (0.5, 0.75, 3, 40, 1, 41)                           # ties: the earlier record stays, partner and step with it
    after[2] = (0.125, np.inf, 1, 33, -1, 0)                       # nothing before
    before[3] = (0.25, 0.375, 0, 5, 2, 6)                          # nothing after
    got = metrics.merge_clearance(before, after)
    want = R.empty(5)
    want[0] = (1.25, 2.0, 4, 30, 1, 12)
    want[1] = before[1]
    want[2] = after[2]
    want[3] = before[3]
    assert got.dtype == R.DTYPE and np.array_equal(got, want)
    assert np.array_equal(before[0], np.array((1.5, 2.0, 3, 10, 1, 12), R.DTYPE))       # the arguments are left alone
    assert np.array_equal(metrics.merge_clearance(R.empty(2), R.empty(2)), R.empty(2))
    with pytest.raises(ValueError):
        metrics.merge_clearance(R.empty(2), R.empty(3))


def test_merge_equals_the_uninterrupted_run():
    """the rule over steps 1 .. k, then from empty records over k + 1 .. end, merged, is the rule over all of them (F4_sca_takeoff16, whose
    step minima are shared 61 times, at three cuts)"""
    from sca_amd import metrics
    fx, after, _ = python_rule('F4_sca_takeoff16')
    for k in (1, 120, 284):
        rest = R.empty(len(fx['radius']))
        for j in range(k, len(after)):
            R.step(rest, fx['pos_after'][j], fx['radius'], fx['flags'][j], fx['obs_pos'], fx['obs_radius'], j + 1)
        assert np.array_equal(metrics.merge_clearance(after[k - 1], rest), after[-1]), k


def test_refusals_of_the_two_calls(H):
    def check(*args):
        out = (C.c_int * 2)()
        H.sclr_check(*args, out)
        return out[0], out[1]
    # enable / disable: get = 0
    assert check(0, 0, 0, 0, 0, 1, 0) == (NO_SCENES, ERR_STATE)
    assert check(0, 3, 1, 0, 0, 1, 0) == (MID_STEP, ERR_STATE)
    assert check(0, 3, 0, 0, 0, 1, 0) == (OK, 0) and check(0, 3, 0, 1, 0, 1, 0) == (OK, 0)
    # get
    assert check(1, 0, 0, 1, 0, 1, 32) == (NO_SCENES, ERR_STATE)
    assert check(1, 3, 0, 0, 0, 1, 32) == (OFF, ERR_STATE)
    assert check(1, 3, 0, 1, -1, 1, 32) == (BAD_SCENE, ERR_ARG) and check(1, 3, 0, 1, 3, 1, 32) == (BAD_SCENE, ERR_ARG)
    assert check(1, 3, 0, 1, 2, 0, 32) == (NO_OUT, ERR_ARG)
    assert check(1, 3, 0, 1, 2, 1, 24) == (BAD_STRUCT, ERR_ARG) and check(1, 3, 0, 1, 2, 1, 40) == (BAD_STRUCT, ERR_ARG)
    assert check(1, 3, 0, 1, 2, 1, 32) == (OK, 0) and check(1, 3, 1, 1, 0, 1, 32) == (OK, 0)


def test_standalone_under_sanitizers():
    """The rule as a program of its own (its main runs it on heap arrays of exactly the sizes it may read) under
    -fsanitize=address,undefined.  Host code only; nothing of it is loaded into python."""
    exe = os.path.join(harness_util.BUILD, 'scene_clearance_harness_san')
    os.makedirs(harness_util.BUILD, exist_ok=True)
    subprocess.check_call(['g++', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan',
                           '-DSCENE_CLEARANCE_MAIN'] + FLAGS + ['-o', exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'scene_clearance_harness: ok' in r.stdout
