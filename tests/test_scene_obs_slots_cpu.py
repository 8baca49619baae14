"""Obstacle slots without a GPU: the host-side rules of sca_set_scene_obstacle_slots and sca_restart_scenes_obstacles (sca_scenes.h: the
slot check, the restart's obstacle check, the obstacle sections of the restart's page-locked block, where a slot's tree stands in the
forest) behind tests/scene_obs_slots_harness.cpp, the same rules as a program of its own under the sanitizers, the queue planning of
run_episodes(episode_obstacles=...) (sca_amd/scenes.py), and the three symbols in the header, the library and _lib.SIGNATURES.  Every
expectation is a literal worked out by hand from the rules in include/sca_hip.h -- none comes from the code under test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import harness_util
from harness_util import load_harness
from test_scene_obstacles_cpu import TREES                          # trees over 1, 10, 11 and 23 members, written out by hand

SLOT_OK, SLOT_OFFSETS, SLOT_BAD_COUNT, SLOT_NO_ARRAYS, SLOT_NOT_FINITE, SLOT_BAD_RADIUS = range(6)        # ObsSlotFault
OFF_OK, OFF_BAD_COUNT, OFF_NO_OFFSETS, OFF_BAD_START, OFF_DECREASING, OFF_TOO_MANY = range(6)             # SceneObsFault
R_OK, R_NO_SLOTS, R_BAD_COUNT, R_NO_ARRAYS, R_NOT_FINITE, R_BAD_RADIUS = range(6)                         # RestartObsFault
ERR_ARG, ERR_STATE = -1, -3                                         # include/sca_hip.h
CAP = [0, 8, 8, 13]                                                 # three slots of obstacle capacity 8, 0 and 5
NEW = ('sca_set_scene_obstacle_slots', 'sca_get_scene_obstacle_counts', 'sca_restart_scenes_obstacles')


@pytest.fixture(scope='module')
def H():
    return load_harness('scene_obs_slots_harness', ('sca_scenes.h',))


def i32(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)


def f64(a):
    return None if a is None else np.ascontiguousarray(a, np.float64)


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def slots(H, counts, rows=None, nscenes=3, ctx=3, max_obstacles=13, cap=CAP, pos='ok', radius='ok'):
    """(fault, offsets' fault, scene, row, total, capacity, code) of the slots call; pos / radius 'ok': valid arrays of `rows` rows"""
    rows = (sum(counts) if counts is not None else 0) if rows is None else rows
    p = f64(np.full((rows, 3), 1.5)) if isinstance(pos, str) else f64(pos)
    r = f64(np.full(rows, 0.5)) if isinstance(radius, str) else f64(radius)
    out = (C.c_int * 7)()
    H.slots_check(ctx, max_obstacles, nscenes, vp(i32(cap)), vp(i32(counts)), vp(p), vp(r), out)
    return tuple(out)


def test_count_check(H):
    for cap in (0, 1, 8, 1491):
        assert H.count_ok(0, cap) and H.count_ok(cap, cap) and not H.count_ok(cap + 1, cap) and not H.count_ok(-1, cap)
    assert not H.count_ok(-2147483648, 8) and not H.count_ok(2147483647, 8)


def test_slots_accepted(H):
    assert slots(H, [8, 0, 5]) == (SLOT_OK, OFF_OK, -1, -1, 13, 13, 0)           # every slot full: what sca_set_scene_obstacles takes
    assert slots(H, [0, 0, 0]) == (SLOT_OK, OFF_OK, -1, -1, 0, 13, 0)
    assert slots(H, None, pos=None, radius=None) == (SLOT_OK, OFF_OK, -1, -1, 0, 13, 0)       # counts NULL: every slot empty, no arrays needed
    assert slots(H, [0, 0, 0], pos=None, radius=None) == (SLOT_OK, OFF_OK, -1, -1, 0, 13, 0)
    assert slots(H, [3, 0, 1]) == (SLOT_OK, OFF_OK, -1, -1, 4, 13, 0)
    assert slots(H, [1491], nscenes=1, ctx=1, max_obstacles=1491, cap=[0, 1491]) == (SLOT_OK, OFF_OK, -1, -1, 1491, 1491, 0)


def test_slots_refused(H):
    # the offsets' rules are sca_set_scene_obstacles', in its order
    assert slots(H, [8, 0, 5], nscenes=2) == (SLOT_OFFSETS, OFF_BAD_COUNT, -1, -1, 0, 0, ERR_ARG)
    assert slots(H, [8, 0, 5], cap=None) == (SLOT_OFFSETS, OFF_NO_OFFSETS, -1, -1, 0, 0, ERR_ARG)
    assert slots(H, [8, 0, 5], cap=[1, 8, 8, 13]) == (SLOT_OFFSETS, OFF_BAD_START, 0, -1, 0, 0, ERR_ARG)
    assert slots(H, [8, 0, 5], cap=[0, 8, 7, 13]) == (SLOT_OFFSETS, OFF_DECREASING, 1, -1, 0, 0, ERR_ARG)
    assert slots(H, [8, 0, 5], max_obstacles=12) == (SLOT_OFFSETS, OFF_TOO_MANY, -1, -1, 0, 13, ERR_ARG)      # the CAPACITIES count, not what the slots hold
    assert slots(H, [1, 0, 0], max_obstacles=12) == (SLOT_OFFSETS, OFF_TOO_MANY, -1, -1, 0, 13, ERR_ARG)
    # a count outside 0 .. capacity
    assert slots(H, [9, 0, 4], rows=13) == (SLOT_BAD_COUNT, OFF_OK, 0, -1, 0, 13, ERR_ARG)
    assert slots(H, [8, 1, 4], rows=13) == (SLOT_BAD_COUNT, OFF_OK, 1, -1, 0, 13, ERR_ARG)                     # a slot of capacity 0 holds nothing
    assert slots(H, [8, 0, -1], rows=13) == (SLOT_BAD_COUNT, OFF_OK, 2, -1, 0, 13, ERR_ARG)
    # arrays
    assert slots(H, [3, 0, 1], pos=None) == (SLOT_NO_ARRAYS, OFF_OK, -1, -1, 4, 13, ERR_ARG)
    assert slots(H, [3, 0, 1], radius=None) == (SLOT_NO_ARRAYS, OFF_OK, -1, -1, 4, 13, ERR_ARG)
    pos = np.full((4, 3), 1.5)
    pos[3, 1] = np.inf                                               # packed row 3 is slot 2's first
    assert slots(H, [3, 0, 1], pos=pos) == (SLOT_NOT_FINITE, OFF_OK, 2, 3, 4, 13, ERR_ARG)
    pos[3, 1], pos[2, 0] = 0.0, np.nan
    assert slots(H, [3, 0, 1], pos=pos) == (SLOT_NOT_FINITE, OFF_OK, 0, 2, 4, 13, ERR_ARG)
    for bad in (0.0, -1.0, np.nan, np.inf):
        radius = np.full(4, 0.5)
        radius[1] = bad
        assert slots(H, [3, 0, 1], radius=radius) == (SLOT_BAD_RADIUS, OFF_OK, 0, 1, 4, 13, ERR_ARG), bad
    # the first broken rule is the one reported: offsets, counts, arrays
    assert slots(H, [9, 0, 4], rows=13, cap=[0, 8, 7, 13], pos=None)[:2] == (SLOT_OFFSETS, OFF_DECREASING)
    assert slots(H, [9, 0, 4], rows=13, pos=None)[0] == SLOT_BAD_COUNT


def test_slot_roots(H):
    """counts[s] > 0 ? 2 * cap_offsets[s] : -1 -- an empty slot has no tree, whatever its capacity"""
    def roots(cap, counts):
        out = np.full(len(counts), 7, np.int32)
        H.slot_roots(len(counts), vp(i32(cap)), vp(i32(counts)), vp(out))
        return out.tolist()
    assert roots(CAP, [8, 0, 5]) == [0, -1, 16]
    assert roots(CAP, [0, 0, 0]) == [-1, -1, -1]
    assert roots(CAP, [1, 0, 1]) == [0, -1, 16]                      # the root stands at the CAPACITY's base, not behind what the slots before it hold
    assert roots([0, 23, 46], [0, 23]) == [-1, 46]


def restart(H, ids, counts, rows=None, on=True, pos='ok', radius='ok'):
    """(fault, entry, total, replaced, code) of the restart's obstacle check on CAP's slots"""
    rows = sum(c for c in (counts or []) if c > 0) if rows is None else rows
    p = f64(np.full((rows, 3), 0.25)) if isinstance(pos, str) else f64(pos)
    r = f64(np.full(rows, 1.0)) if isinstance(radius, str) else f64(radius)
    out = (C.c_int * 5)()
    H.restart_obs_check(int(on), vp(i32(CAP)) if on else None, len(ids), vp(i32(ids)), vp(i32(counts)), vp(p), vp(r), out)
    return tuple(out)


def test_restart_obstacle_check(H):
    assert restart(H, [2, 0], None) == (R_OK, -1, 0, 0, 0)                                    # NULL: exactly the sized restart
    assert restart(H, [2, 0], None, on=False) == (R_OK, -1, 0, 0, 0)
    assert restart(H, [2, 0], [-1, -1]) == (R_OK, -1, 0, 0, 0)                                # keep: nothing replaced, nothing staged
    assert restart(H, [2, 0], [-1, -1], on=False) == (R_OK, -1, 0, 0, 0)                      # ... which a context without slots may say too
    assert restart(H, [2, 0], [5, 8]) == (R_OK, -1, 13, 2, 0)                                 # the capacities
    assert restart(H, [2, 0, 1], [0, -1, 0]) == (R_OK, -1, 0, 2, 0)                           # emptied: replaced by a set of none
    assert restart(H, [2, 0], [3, -1]) == (R_OK, -1, 3, 1, 0)
    assert restart(H, [2, 0], [0, -1], pos=None, radius=None) == (R_OK, -1, 0, 1, 0)          # a total of 0 needs no arrays
    assert restart(H, [2, 0], [-1, 0], on=False) == (R_NO_SLOTS, 1, 0, 0, ERR_STATE)
    assert restart(H, [2, 0], [5, 8], on=False) == (R_NO_SLOTS, 0, 0, 0, ERR_STATE)
    assert restart(H, [2, 0], [6, 8], rows=14) == (R_BAD_COUNT, 0, 0, 0, ERR_ARG)             # capacity + 1
    assert restart(H, [2, 0], [5, 9], rows=14) == (R_BAD_COUNT, 1, 0, 0, ERR_ARG)
    assert restart(H, [1], [1], rows=1) == (R_BAD_COUNT, 0, 0, 0, ERR_ARG)                    # the slot of capacity 0
    assert restart(H, [2, 0], [5, -2], rows=5) == (R_BAD_COUNT, 1, 0, 0, ERR_ARG)
    assert restart(H, [2, 0], [-2, 5], rows=5, on=False) == (R_BAD_COUNT, 0, 0, 0, ERR_ARG)   # below -1 is an argument error with or without slots
    assert restart(H, [2, 0], [3, -1], pos=None) == (R_NO_ARRAYS, -1, 3, 1, ERR_ARG)
    assert restart(H, [2, 0], [3, -1], radius=None) == (R_NO_ARRAYS, -1, 3, 1, ERR_ARG)
    pos = np.full((4, 3), 0.25)
    pos[3, 2] = -np.inf
    assert restart(H, [2, 0], [3, 1], pos=pos) == (R_NOT_FINITE, 3, 4, 2, ERR_ARG)
    for bad in (0.0, -0.5, np.nan):
        radius = np.ones(4)
        radius[2] = bad
        assert restart(H, [2, 0], [3, 1], radius=radius) == (R_BAD_RADIUS, 2, 4, 2, ERR_ARG), bad


def test_block_layout(H):
    """behind the agent sections and the sizes: head words (4 x int32 per named scene, at most max_n scenes), ObsRec rows and sorted rows
    (32 B), perm (4 B), KdNode (64 B) and KdWide (128 B) records, two per obstacle row; every section on a 64-byte boundary"""
    k = (C.c_int * 6)()
    H.obs_layout_constants(k)
    assert tuple(k) == (6, 4, 32, 64, 128, 64)
    up = lambda x: (x + 63) // 64 * 64
    for max_n, max_m in ((1, 0), (1, 1), (16, 8), (60, 1491), (100, 13), (1536, 100000)):
        off, size = (C.c_longlong * 7)(), (C.c_longlong * 6)()
        begin = H.obs_layout(max_n, max_m, off, size)
        want = [16 * max_n, 32 * max_m, 32 * max_m, 4 * max_m, 128 * max_m, 256 * max_m]
        assert list(size) == want, (max_n, max_m)
        at = up(begin)
        for s in range(6):
            assert off[s] == at and off[s] % 16 == 0 and off[s] >= begin, (max_n, max_m, s)       # aligned, behind the agent sections
            at += up(want[s])                                                                  # ... and no two overlap
        assert off[6] == at
        again, again_size = (C.c_longlong * 7)(), (C.c_longlong * 6)()
        assert H.obs_layout(max_n, max_m, again, again_size) == begin and list(again) == list(off)  # a function of max_n and max_obstacles alone


def placed(H, k, obs_begin):
    nodes = np.zeros((max(2 * k - 1, 0), 4), np.int32)
    for i, rec in (TREES[k].items() if k else ()):
        nodes[i] = rec
    if k:
        H.slot_shift(vp(nodes), len(nodes), obs_begin)
    return nodes


def test_forest_placement_in_a_slot(H):
    """a slot of capacity 23 between two others (obstacle rows [5, 28), node records [10, 56)) holding 0, 1, 10, 11 and 23 obstacles: one
    leaf, a full leaf, the first split, the capacity.  Every node inside the slot's records, every link inside them, the root -1 when empty."""
    cap = [0, 5, 28, 30]
    lo, hi = cap[1], cap[2]
    for k in (0, 1, 10, 11, 23):
        out = np.full(3, 7, np.int32)
        H.slot_roots(3, vp(i32(cap)), vp(i32([5, k, 2])), vp(out))
        assert out.tolist() == [0, 2 * lo if k else -1, 56], k
        nodes = placed(H, k, lo)
        assert 2 * lo + len(nodes) <= 2 * hi, k                      # 2k - 1 records always fit 2 x capacity
        used = 0
        for i, (b, e, left, right) in enumerate(nodes.tolist()):
            if e == b:
                assert (b, e, left, right) == (0, 0, 0, 0), (k, i)   # a record the tree does not use
                continue
            used += 1
            assert lo <= b < e <= lo + k <= hi, (k, i)               # members: the slot's first k rows
            if e - b > 10:
                for child in (left, right):
                    assert 2 * lo < child < 2 * lo + len(nodes) <= 2 * hi, (k, i)             # links never leave the slot's records
                    assert nodes[child - 2 * lo][1] > nodes[child - 2 * lo][0], (k, i)
                assert nodes[left - 2 * lo][0] == b and nodes[left - 2 * lo][1] == nodes[right - 2 * lo][0] and nodes[right - 2 * lo][1] == e, (k, i)
            else:
                assert (left, right) == (0, 0), (k, i)
        assert used == len(TREES.get(k, {})), k
    # by hand: 11 obstacles at base 5 -- the root [5, 16) with children at records 11 and 20, leaves [5, 10) and [10, 16)
    assert placed(H, 11, 5)[[0, 1, 10]].tolist() == [[5, 16, 11, 20], [5, 10, 0, 0], [10, 16, 0, 0]]


def test_standalone_under_sanitizers():
    """The same rules as a program of its own (heap arrays of exactly the sizes the rules may read) under -fsanitize=address,undefined.
    Host code only; nothing of it is loaded into python."""
    exe = os.path.join(harness_util.BUILD, 'scene_obs_slots_harness_san')
    os.makedirs(harness_util.BUILD, exist_ok=True)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan',
                           '-DSCENE_OBS_SLOTS_MAIN', '-I' + harness_util.CSRC, '-o', exe, os.path.join(harness_util.ROOT, 'tests', 'scene_obs_slots_harness.cpp')])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'scene_obs_slots_harness: ok' in r.stdout


# ---- the queue planning of run_episodes(episode_obstacles=...) -----------------------------------------------------------------------------
QUEUE = [(16, 8), (16, 1491), (60, 0), (8, 5), (16, 8), (60, 0), (8, 5), (16, 1491)]          # (agents, obstacles): take-off, exp3, open circle, random


def test_next_fitting2():
    from sca_amd.scenes import next_fitting2
    assert next_fitting2(16, 8, QUEUE) == 0
    assert next_fitting2(16, 7, QUEUE) == 3                          # the agents fit, the obstacles do not: the first that fits BOTH
    assert next_fitting2(60, 0, QUEUE) == 2
    assert next_fitting2(15, 1491, QUEUE) == 3
    assert next_fitting2(16, 1491, QUEUE[1:]) == 0
    assert next_fitting2(7, 1491, QUEUE) is None and next_fitting2(60, 8, []) is None
    assert next_fitting2(8, 5, [(8, 5)]) == 0 and next_fitting2(8, 4, [(8, 5)]) is None


def simulate(queue, capacities):
    """the slots' plan and refills as run_episodes makes them, the slots finishing in turn: [(episode, slot)] in placing order"""
    from sca_amd.scenes import next_fitting2, plan_capacity_slots2
    holding = plan_capacity_slots2(queue, capacities)
    pending = [i for i in range(len(queue)) if i not in holding]
    placed_in = [(i, s) for s, i in enumerate(holding) if i is not None]
    while any(h is not None for h in holding):
        for s, (c, oc) in enumerate(capacities):
            if holding[s] is None:
                continue
            k = next_fitting2(c, oc, [queue[j] for j in pending])
            holding[s] = None if k is None else pending.pop(k)
            if holding[s] is not None:
                placed_in.append((holding[s], s))
    return placed_in, pending


@pytest.mark.parametrize('capacities', [[(60, 1491)] * 3, [(60, 1491)], [(16, 1491), (60, 8), (8, 5)], [(60, 0), (16, 1491), (16, 8), (8, 5), (8, 5)],
                                        [(8, 5), (60, 1491)]])
def test_every_episode_is_placed_once_and_where_it_fits(capacities):
    placed_in, left = simulate(QUEUE, capacities)
    assert left == [] and sorted(i for i, _ in placed_in) == list(range(len(QUEUE)))
    for i, s in placed_in:
        assert QUEUE[i][0] <= capacities[s][0] and QUEUE[i][1] <= capacities[s][1], (i, s)


def test_plan_capacity_slots2():
    from sca_amd.scenes import plan_capacity_slots2
    assert plan_capacity_slots2(QUEUE, [(60, 1491)] * 3) == [0, 1, 2]                          # queue order
    assert plan_capacity_slots2(QUEUE, [(16, 1491), (60, 8), (8, 5)]) == [0, 2, 3]             # each slot its first fitting entry nobody took
    assert plan_capacity_slots2(QUEUE, [(8, 5), (60, 1491)]) == [3, 0]
    assert plan_capacity_slots2([(8, 5)], [(60, 0), (8, 5)]) == [None, 0]                      # nothing fits the first slot
    with pytest.raises(ValueError, match='episode 1 has 16 agents and 1491 obstacles and fits no slot'):
        plan_capacity_slots2(QUEUE, [(60, 8), (16, 8)])
    with pytest.raises(ValueError, match='episode 2 has 60 agents and 0 obstacles and fits no slot'):
        plan_capacity_slots2(QUEUE, [(16, 1491), (16, 8)])                                     # each capacity is large enough somewhere, but not in ONE slot ...
    with pytest.raises(ValueError):
        plan_capacity_slots2([(60, 1491)], [(60, 8), (16, 1491)])                              # ... as here
    with pytest.raises(ValueError):
        plan_capacity_slots2(QUEUE, [])


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_the_three_symbols():
    from sca_amd import _lib
    from test_abi import declared_symbols
    L, declared = _lib.lib(), declared_symbols()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    ip, dp, fp, bp = _lib.ip, _lib.dp, _lib.fp, _lib.bp
    sized = _lib.SIGNATURES['sca_restart_scenes_sized']
    assert _lib.SIGNATURES['sca_set_scene_obstacle_slots'] == (C.c_int, [C.c_void_p, C.c_int, ip, ip, dp, dp])
    assert _lib.SIGNATURES['sca_get_scene_obstacle_counts'] == (C.c_int, [C.c_void_p, ip, ip])
    # the sized restart's arguments with obs_counts, obs_pos, obs_radius between the sizes and the agent arrays
    assert _lib.SIGNATURES['sca_restart_scenes_obstacles'] == (sized[0], sized[1][:4] + [ip, dp, dp] + sized[1][4:])
    assert sized[1][4:] == [dp, fp, dp, dp, dp, dp, bp, bp, dp, dp]
