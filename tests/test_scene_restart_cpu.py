"""The host-side rules of sca_restart_scenes without a GPU: scene_restart_check (every fault with the entry it names, T for a valid list) and
the staging block's layout (sca_scenes.h), behind tests/scenes_harness.cpp.  Every expectation is a literal worked out by hand from
the rules in include/sca_hip.h -- none comes from the code under test."""
import ctypes as C

import numpy as np
import pytest

from harness_util import load_harness

(OK, NO_SCENES, NO_STATE, MID_STEP, BAD_COUNT, BAD_ID, REPEATED_ID, NO_ARRAYS, NOT_FINITE, BAD_POLICY, NOT_POSITIVE, GOAL_HEADING, PATHS,
 TRACKED_CHANGE) = range(14)                                        # RestartFault
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5                   # include/sca_hip.h
STATE, BEGUN, TRACKER, PATHS_ON, PER_AGENT = 1, 2, 4, 8, 16
OFFSETS = [0, 3, 8, 10]                                            # three scenes of 3, 5 and 2 agents
POLICY_NOW = [0, 1, 2, 3, 4, 5, 0, 1, 2, 3]


@pytest.fixture(scope='module')
def H():
    return load_harness('scenes_harness', ('sca_forms.h', 'sca_scenes.h', 'sca_scene_restart.h'))


def episode(T):
    """T rows of valid arrays"""
    return dict(pos=np.arange(3.0 * T).reshape(T, 3), vel=np.zeros((T, 3), np.float32), heading=np.zeros((T, 3)), radius=np.full(T, 0.5),
                pref_speed=np.ones(T), goal=np.ones((T, 3)), policy=np.zeros(T, np.uint8), zaxis=np.zeros(T, np.uint8),
                max_run_dist=np.full(T, 30.0), goal_heading=np.zeros((T, 3)))


def check(H, ids, ctx=STATE | TRACKER, offsets=OFFSETS, count=None, **arrays):
    """(fault, entry, T, error code); arrays: the episode's, None for a NULL pointer"""
    T = 0 if ids is None else sum(OFFSETS[s + 1] - OFFSETS[s] for s in ids if 0 <= s < 3)
    a = episode(max(T, 1))
    a.update(arrays)
    keep = []

    def p(x, dt):
        if x is None:
            return None
        x = np.ascontiguousarray(x, dt)
        keep.append(x)
        return x.ctypes.data_as(C.c_void_p)
    out = (C.c_int * 3)()
    off = None if offsets is None else np.ascontiguousarray(offsets, np.int32)
    idv = None if ids is None else np.ascontiguousarray(list(ids) + [0], np.int32)
    rc = H.restart_check(0 if off is None else len(off) - 1, p(off, np.int32), ctx, p(POLICY_NOW, np.uint8),
                         (0 if ids is None else len(ids)) if count is None else count, p(idv, np.int32),
                         p(a['pos'], np.float64), p(a['vel'], np.float32), p(a['heading'], np.float64), p(a['radius'], np.float64),
                         p(a['pref_speed'], np.float64), p(a['goal'], np.float64), p(a['policy'], np.uint8), p(a['zaxis'], np.uint8),
                         p(a['max_run_dist'], np.float64), p(a['goal_heading'], np.float64), out)
    return (out[0], out[1], out[2], rc)


def put(T, key, row, value, col=None):
    a = episode(T)[key]
    if col is None:
        a[row] = value
    else:
        a[row, col] = value
    return {key: a}


def test_valid_lists_and_their_T(H):
    assert check(H, [0]) == (OK, -1, 3, 0)
    assert check(H, [2]) == (OK, -1, 2, 0)                         # ids at both ends of the range
    assert check(H, [0, 2]) == (OK, -1, 5, 0)
    assert check(H, [2, 1, 0]) == (OK, -1, 10, 0)                  # any order, all of them
    assert check(H, [1], vel=None, radius=None, pref_speed=None, goal=None, policy=None, zaxis=None, max_run_dist=None, goal_heading=None) == (OK, -1, 5, 0)
    assert check(H, [1], ctx=STATE, goal_heading=None) == (OK, -1, 5, 0)                           # no tracker, no goal_heading
    assert check(H, [0], ctx=STATE | TRACKER | PER_AGENT, policy=[5, 2, 1]) == (OK, -1, 3, 0)      # 0 -> 5 stays tracked, 1 -> 2 and 2 -> 1 untracked
    assert check(H, [0], ctx=STATE | TRACKER, policy=[1, 0, 0]) == (OK, -1, 3, 0)                  # a change of status without per-agent attributes


def test_state_faults_come_first(H):
    assert check(H, [0], offsets=None) == (NO_SCENES, -1, 0, ERR_STATE)
    assert check(H, [0], ctx=TRACKER) == (NO_STATE, -1, 0, ERR_STATE)
    assert check(H, [0], ctx=STATE | BEGUN) == (MID_STEP, -1, 0, ERR_STATE)
    assert check(H, [7], ctx=0) == (NO_STATE, -1, 0, ERR_STATE)    # (before the ids are looked at)


def test_id_faults_name_the_entry(H):
    assert check(H, []) == (BAD_COUNT, -1, 0, ERR_ARG)
    assert check(H, [0], count=-2) == (BAD_COUNT, -1, 0, ERR_ARG)
    assert check(H, None, count=1) == (BAD_COUNT, -1, 0, ERR_ARG)  # scene_ids NULL
    assert check(H, [-1]) == (BAD_ID, 0, 0, ERR_ARG)
    assert check(H, [3]) == (BAD_ID, 0, 0, ERR_ARG)                # one past the last scene
    assert check(H, [0, 2, 3]) == (BAD_ID, 2, 0, ERR_ARG)
    assert check(H, [1, 1]) == (REPEATED_ID, 1, 0, ERR_ARG)
    assert check(H, [2, 0, 1, 0]) == (REPEATED_ID, 3, 0, ERR_ARG)  # the second mention
    assert check(H, [0, 0, 9]) == (REPEATED_ID, 1, 0, ERR_ARG)     # entries are looked at in order


def test_array_faults_name_the_row(H):
    assert check(H, [1], pos=None) == (NO_ARRAYS, -1, 5, ERR_ARG)
    assert check(H, [1], heading=None) == (NO_ARRAYS, -1, 5, ERR_ARG)
    for key, col in (('pos', 0), ('heading', 2), ('vel', 1), ('goal', 2), ('goal_heading', 0), ('radius', None), ('pref_speed', None), ('max_run_dist', None)):
        for value in (np.nan, np.inf, -np.inf):
            assert check(H, [0, 1], **put(8, key, 6, value, col)) == (NOT_FINITE, 6, 8, ERR_ARG), (key, value)
    assert check(H, [1], **put(5, 'pos', 0, np.nan, 0)) == (NOT_FINITE, 0, 5, ERR_ARG)
    assert check(H, [1], **put(5, 'policy', 4, 6)) == (BAD_POLICY, 4, 5, ERR_ARG)
    assert check(H, [1], **put(5, 'policy', 4, 5)) == (OK, -1, 5, 0)                               # SCA_POLICY_RVO3D_DUBINS itself
    for key in ('radius', 'pref_speed', 'max_run_dist'):
        assert check(H, [2, 0], **put(5, key, 3, 0.0)) == (NOT_POSITIVE, 3, 5, ERR_ARG), key
        assert check(H, [2, 0], **put(5, key, 1, -0.5)) == (NOT_POSITIVE, 1, 5, ERR_ARG), key
    assert check(H, [1], ctx=STATE) == (GOAL_HEADING, -1, 5, ERR_ARG)                              # goal_heading passed, no tracker


def test_unsupported(H):
    assert check(H, [1], ctx=STATE | TRACKER | PATHS_ON) == (PATHS, -1, 5, ERR_UNSUPPORTED)
    # scene 1 holds policies 3 4 5 0 1 (tracked: rows 2 and 3); the arrays follow scene_ids, so with [2, 1] its rows are 2 .. 6
    assert check(H, [1], ctx=STATE | TRACKER | PER_AGENT, policy=[3, 4, 5, 0, 0]) == (TRACKED_CHANGE, 4, 5, ERR_UNSUPPORTED)
    assert check(H, [1], ctx=STATE | TRACKER | PER_AGENT, policy=[3, 4, 1, 0, 1]) == (TRACKED_CHANGE, 2, 5, ERR_UNSUPPORTED)
    assert check(H, [2, 1], ctx=STATE | TRACKER | PER_AGENT, policy=[2, 3, 3, 4, 0, 5, 5]) == (TRACKED_CHANGE, 6, 7, ERR_UNSUPPORTED)
    assert check(H, [2, 1], ctx=STATE | TRACKER | PER_AGENT, policy=[2, 3, 3, 4, 0, 5, 1]) == (OK, -1, 7, 0)
    assert check(H, [1], ctx=STATE | TRACKER | PER_AGENT, policy=None) == (OK, -1, 5, 0)           # no policy array: nothing changes


def test_staging_block_layout(H):
    """one section per array, each sized for `cap` rows and aligned to 64 bytes: ids, start (i32), pos, heading, goal, goal_heading (3 f64),
    radius, pref_speed, max_run_dist (f64), vel (3 f32), policy, zaxis, vpref_mode (u8)"""
    assert H.restart_sections() == 13
    row = [4, 4, 24, 24, 24, 24, 8, 8, 8, 12, 1, 1, 1]
    off, total = (C.c_int64 * 13)(), C.c_int64()
    for cap in (1, 7, 16, 100, 1537, 89280):
        H.restart_layout(cap, off, C.byref(total))
        at = 0
        for s in range(13):
            assert off[s] == at and off[s] % 64 == 0, (cap, s)
            at += -(-row[s] * cap // 64) * 64
        assert total.value == at
    H.restart_layout(100, off, C.byref(total))
    assert list(off)[:4] == [0, 448, 896, 3328] and total.value == 448 * 2 + 2432 * 4 + 832 * 3 + 1216 + 128 * 3
