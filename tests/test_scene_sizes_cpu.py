"""Slots of a capacity without a GPU: the host-side rules of sca_restart_scenes_sized (sca_scenes.h: the size check, the packed-row starts,
"is any scene partial", the log's agent window) behind tests/scene_sizes_harness.cpp, the same rules as a program of its own under the
sanitizers, and the queue planning of run_episodes(capacities=...) (sca_amd/scenes.py).  Every expectation is a literal worked out by hand
from the rules in include/sca_hip.h -- none comes from the code under test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import harness_util
from harness_util import load_harness

OK, TRACKED_CHANGE, BAD_SIZE = 0, 13, 14                            # RestartFault
LOG_OK, LOG_BAD_AGENTS = 0, 8                                       # SceneLogFault
ERR_ARG, ERR_UNSUPPORTED = -1, -5                                   # include/sca_hip.h
OFFSETS = [0, 3, 8, 10]                                             # three slots of capacity 3, 5 and 2
POLICY_NOW = [0, 1, 2, 3, 4, 5, 0, 1, 2, 3]


@pytest.fixture(scope='module')
def H():
    return load_harness('scene_sizes_harness', ('sca_scenes.h',))


def i32(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)


def ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def test_size_check(H):
    for cap in (1, 5, 130):
        assert not H.size_ok(0, cap) and not H.size_ok(-1, cap) and not H.size_ok(cap + 1, cap)
        assert H.size_ok(cap, cap) and H.size_ok(1, cap)
    assert H.size_ok(4, 5) and not H.size_ok(-2147483648, 5)


def starts(H, ids, sizes):
    ids, sizes = i32(ids), i32(sizes)
    out = np.full(len(ids), -7, np.int32)
    T = H.restart_starts(len(ids), ip(i32(OFFSETS)), ip(ids), ip(sizes), ip(out))
    return out.tolist(), T


def test_packed_row_starts(H):
    assert starts(H, [0, 1, 2], [1, 4, 2]) == ([0, 1, 5], 7)
    assert starts(H, [2, 0, 1], [1, 3, 4]) == ([0, 1, 4], 8)       # the arrays follow scene_ids, not the scenes' order
    assert starts(H, [1], [5]) == ([0], 5)
    assert starts(H, [1], [1]) == ([0], 1)
    # sizes == NULL: every named scene filled to its capacity -- the same as passing the capacities
    for ids in ([0, 1, 2], [2, 1, 0], [1], [2, 0]):
        caps = [OFFSETS[s + 1] - OFFSETS[s] for s in ids]
        assert starts(H, ids, None) == starts(H, ids, caps)
    assert starts(H, [2, 1, 0], None) == ([0, 2, 7], 10)


def check(H, ids, sizes, rows, policy=None, per_agent=0):
    ids, sz, off = i32(ids), i32(sizes), i32(OFFSETS)
    now = np.ascontiguousarray(POLICY_NOW, np.uint8)
    pol = None if policy is None else np.ascontiguousarray(policy, np.uint8)
    out = (C.c_int * 3)()
    rc = H.sized_check(3, ip(off), now.ctypes.data_as(C.c_void_p), per_agent, len(ids), ip(ids), ip(sz), rows,
                       None if pol is None else pol.ctypes.data_as(C.c_void_p), out)
    return out[0], out[1], out[2], rc


def test_restart_check_with_sizes(H):
    assert check(H, [1], [5], 5) == (OK, -1, 5, 0)                 # the capacity itself
    assert check(H, [1], [1], 1) == (OK, -1, 1, 0)
    assert check(H, [1], None, 5) == (OK, -1, 5, 0)                # NULL: the capacity
    assert check(H, [2, 0, 1], [1, 3, 4], 8) == (OK, -1, 8, 0)
    assert check(H, [1], [0], 1) == (BAD_SIZE, 0, 0, ERR_ARG)
    assert check(H, [1], [-1], 1) == (BAD_SIZE, 0, 0, ERR_ARG)
    assert check(H, [1], [6], 6) == (BAD_SIZE, 0, 0, ERR_ARG)      # capacity + 1
    assert check(H, [0, 2, 1], [3, 3, 5], 11) == (BAD_SIZE, 1, 0, ERR_ARG)     # the entry is the index in sizes; scene 2 holds at most 2
    # per-agent tracker attributes: the tracked / untracked rule runs over the rows the episode occupies, packed by the sizes.  Slot 1 holds
    # policies 3 4 5 0 1 (tracked: its rows 2 and 3); with [2, 1] and sizes [1, 3] slot 1's rows are packed rows 1 .. 3
    assert check(H, [2, 1], [1, 3], 4, policy=[2, 3, 4, 5], per_agent=1) == (OK, -1, 4, 0)
    assert check(H, [2, 1], [1, 3], 4, policy=[2, 3, 4, 1], per_agent=1) == (TRACKED_CHANGE, 3, 4, ERR_UNSUPPORTED)
    assert check(H, [2, 1], [1, 2], 3, policy=[2, 3, 4], per_agent=1) == (OK, -1, 3, 0)       # the tracked rows are not occupied


def test_any_partial(H):
    off = i32(OFFSETS)
    assert not H.any_partial(3, ip(off), ip(i32([3, 5, 2])))
    assert H.any_partial(3, ip(off), ip(i32([3, 5, 1])))
    assert H.any_partial(3, ip(off), ip(i32([1, 5, 2])))


def window(H, size, scene, agent_begin, agent_count):
    out = (C.c_int * 2)()
    rc = H.log_window(3, ip(i32(OFFSETS)), ip(i32(size)), 8, scene, 3, 0, 3, agent_begin, agent_count, out)
    return out[0], out[1], rc


def test_log_window_is_bounded_by_the_size(H):
    assert H.log_agents_ok(4, 0, 4) and not H.log_agents_ok(4, 0, 5)             # at size, at size + 1
    assert H.log_agents_ok(4, 3, 1) and not H.log_agents_ok(4, 3, 2) and H.log_agents_ok(4, 4, 0)
    assert not H.log_agents_ok(4, 2147483647, 1) and not H.log_agents_ok(4, -1, 1) and not H.log_agents_ok(4, 0, -1)
    assert window(H, [3, 4, 2], 1, 0, 4) == (LOG_OK, 1, 0)
    assert window(H, [3, 4, 2], 1, 0, 5) == (LOG_BAD_AGENTS, 1, ERR_ARG)        # slot 1 of capacity 5 holds 4
    assert window(H, None, 1, 0, 5) == (LOG_OK, 1, 0)                           # every scene full: as before
    assert window(H, [3, 5, 2], 1, 0, 5) == (LOG_OK, 1, 0)
    assert window(H, [3, 5, 2], 1, 0, 6) == (LOG_BAD_AGENTS, 1, ERR_ARG)


def test_standalone_under_sanitizers():
    """The same rules as a program of its own (heap arrays of exactly the sizes the rules may read) under -fsanitize=address,undefined.
    Host code only; nothing of it is loaded into python."""
    exe = os.path.join(harness_util.BUILD, 'scene_sizes_harness_san')
    os.makedirs(harness_util.BUILD, exist_ok=True)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan',
                           '-DSCENE_SIZES_MAIN', '-I' + harness_util.CSRC, '-o', exe, os.path.join(harness_util.ROOT, 'tests', 'scene_sizes_harness.cpp')])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'scene_sizes_harness: ok' in r.stdout


# ---- the queue planning of run_episodes(capacities=...) ------------------------------------------------------------------------------------
def test_next_fitting():
    from sca_amd.scenes import next_fitting
    assert next_fitting(16, [20, 16, 6]) == 1                      # the first in queue order that fits, not the best fit
    assert next_fitting(16, [6, 16]) == 0
    assert next_fitting(5, [6, 16]) is None
    assert next_fitting(16, []) is None
    assert next_fitting(6, [6]) == 0


def test_plan_capacity_slots():
    from sca_amd.scenes import plan_capacity_slots
    assert plan_capacity_slots([6, 11, 16, 6, 11], [16, 16, 16]) == [0, 1, 2]                  # queue order preserved
    assert plan_capacity_slots([16, 6, 11, 6], [6, 16, 11]) == [1, 0, 2]                       # each slot its first fitting entry
    assert plan_capacity_slots([16, 16, 6], [6, 16]) == [2, 0]
    assert plan_capacity_slots([6], [16, 16]) == [0, None]                                     # more slots than episodes
    assert plan_capacity_slots([16, 11], [16, 6]) == [0, None]                                 # nothing left fits the small slot
    with pytest.raises(ValueError, match='episode 1 has 20 agents and fits no slot'):
        plan_capacity_slots([6, 20, 11], [16, 16, 16])
    with pytest.raises(ValueError):
        plan_capacity_slots([6], [])


def test_plan_queue():
    from sca_amd.scenes import plan_queue, plan_slots
    for sizes, slots in (([6, 11, 16, 6, 11, 16], 3), ([6, 6, 6, 11], 3), ([5], 4), ([7, 7, 9, 7], 2)):
        holding, caps = plan_queue(sizes, slots, None)             # None: today's plan, slots of the sizes of what they start with
        assert holding == plan_slots(sizes, slots) and caps == [sizes[i] for i in holding]
    with pytest.raises(ValueError):
        plan_queue([6, 11, 16], 2, None)                           # three distinct counts, two fixed-size slots ...
    assert plan_queue([6, 11, 16], 2, 'max') == ([0, 1], [16, 16])  # ... stream through two capacity slots
    assert plan_queue([6, 11, 16, 6], 3, 'max') == ([0, 1, 2], [16, 16, 16])
    assert plan_queue([6], 3, 'max') == ([0], [6])                 # slots that would start empty are left out
    assert plan_queue([16, 6, 6], 3, [6, 16, 6]) == ([1, 0, 2], [6, 16, 6])
    with pytest.raises(ValueError):
        plan_queue([20, 6], 3, [16, 16, 16])                       # an episode that fits nowhere
    with pytest.raises(ValueError):
        plan_queue([6, 6], 3, [16, 16])                            # one capacity per slot
    with pytest.raises(ValueError):
        plan_queue([6, 6], 3, 'min')
