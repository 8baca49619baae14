"""The host side of the scene harvest without a GPU: the block's layout, the refusals and the collect order (sca_scenes.h:
scene_harvest_layout, scene_harvest_check, scene_harvest_order) behind tests/scene_harvest_harness.cpp, and
metrics.episode_metrics_from_harvest against metrics.episode_metrics on fabricated episodes.  Every expectation of the C++ rules is a
literal worked out by hand from what include/sca_hip.h states -- none comes from the code under test."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import harness_util
from harness_util import load_harness

COUNTERS, SUMMARY, POS, VEL, HEADING, FLAGS, TOTAL_DIST, STEP_NUM = range(8)      # HarvestSection
ROW_BYTES = {POS: 24, VEL: 12, HEADING: 24, FLAGS: 1, TOTAL_DIST: 8, STEP_NUM: 4}
OK, NO_SCENES, MID_STEP, OFF, NO_OUT, BAD_STRUCT = range(6)                       # HarvestFault
ENABLE, GET, COLLECT = range(3)                                                   # HarvestOp
ERR_ARG, ERR_STATE = -1, -3                                                       # include/sca_hip.h


@pytest.fixture(scope='module')
def H():
    h = load_harness('scene_harvest_harness', ('sca_scenes.h',))
    h.hv_section_bytes.restype = C.c_int64
    return h


def layout(H, nscenes, n):
    out = (C.c_int64 * 9)()
    H.hv_layout(nscenes, n, out)
    return list(out[:8]), out[8]


def test_layout_literals(H):
    # 3 scenes over 10 rows: counters 24 B, summaries 192 B, pos 240, vel 120, heading 240, flags 10, total_dist 80, step_num 40 -- each
    # section rounded up to 128
    off, total = layout(H, 3, 10)
    assert off == [0, 128, 384, 640, 768, 1024, 1152, 1280] and total == 1408
    # 1024 scenes of 100: 8 KB of counters, 64 KB of summaries, then 102400 rows
    off, total = layout(H, 1024, 102400)
    assert off[:3] == [0, 8192, 8192 + 65536]
    assert total == 8192 + 65536 + 102400 * (24 + 12 + 24 + 1 + 8 + 4)             # every section a multiple of 128 already
    sizes = (C.c_int * 3)()
    H.hv_struct_sizes(sizes)
    assert list(sizes) == [64, 80, 16]                                             # the summary record; the struct; its four leading integers


@pytest.mark.parametrize('offsets', [[0, 3, 8, 10], [0, 1], [0, 1, 64, 129, 384, 641, 1000], [0, 130]])
def test_sections_are_aligned_and_disjoint_and_rows_land_at_offsets(H, offsets):
    B, n = len(offsets) - 1, offsets[-1]
    off, total = layout(H, B, n)
    owner = np.zeros(total, np.int32)
    for s in range(8):
        assert off[s] % 128 == 0
        end = off[s + 1] if s < 7 else total
        assert off[s] + H.hv_section_bytes(s, B, n) <= end                         # a section ends before the next begins
    for sc in range(B):
        owner[off[COUNTERS] + 8 * sc:off[COUNTERS] + 8 * sc + 8] += 1
        owner[off[SUMMARY] + 64 * sc:off[SUMMARY] + 64 * sc + 64] += 1
        for s, row in ROW_BYTES.items():
            assert H.hv_section_bytes(s, B, n) == row * n
            owner[off[s] + row * offsets[sc]:off[s] + row * offsets[sc + 1]] += 1      # the scene's rows stand at offsets[sc], as in sca_get_state
    assert owner.max() == 1                                                        # no byte has two owners
    assert owner.sum() == 8 * B + 64 * B + sum(ROW_BYTES.values()) * n             # ... and everything outside is padding


def test_a_layout_for_fewer_agents_fits_the_one_for_more(H):
    for B, n, max_n in [(3, 10, 11), (3, 10, 4096), (1, 1, 2), (7, 1000, 1001)]:
        small, big = layout(H, B, n), layout(H, B, max_n)
        assert all(a <= b for a, b in zip(small[0], big[0])) and small[1] <= big[1]


def check(H, op, nscenes=3, begun=0, enabled=1, have_out=1, struct_bytes=80):
    out = (C.c_int * 1)()
    rc = H.hv_check(op, nscenes, begun, enabled, have_out, struct_bytes, out)
    return out[0], rc


def test_every_refusal(H):
    # enable / disable: needs scenes, and no step under way; whether it is on already does not matter
    assert check(H, ENABLE) == (OK, 0)
    assert check(H, ENABLE, enabled=0) == (OK, 0)
    assert check(H, ENABLE, nscenes=0) == (NO_SCENES, ERR_STATE)
    assert check(H, ENABLE, begun=1) == (MID_STEP, ERR_STATE)
    assert check(H, ENABLE, nscenes=0, begun=1) == (NO_SCENES, ERR_STATE)          # the order of the refusals
    # get: scenes, enabled, a struct to write into, of a size between the leading integers and the library's struct
    assert check(H, GET) == (OK, 0)
    assert check(H, GET, begun=1) == (OK, 0)                                       # reading the pointers is fine mid-step
    assert check(H, GET, nscenes=0) == (NO_SCENES, ERR_STATE)
    assert check(H, GET, enabled=0) == (OFF, ERR_STATE)
    assert check(H, GET, have_out=0) == (NO_OUT, ERR_ARG)
    assert check(H, GET, struct_bytes=15) == (BAD_STRUCT, ERR_ARG)
    assert check(H, GET, struct_bytes=16) == (OK, 0)                               # the integers alone
    assert check(H, GET, struct_bytes=81) == (BAD_STRUCT, ERR_ARG)
    assert check(H, GET, struct_bytes=-1) == (BAD_STRUCT, ERR_ARG)
    assert check(H, GET, enabled=0, have_out=0, struct_bytes=0) == (OFF, ERR_STATE)      # state before arguments
    # collect: the same, without a struct
    assert check(H, COLLECT, struct_bytes=0) == (OK, 0)
    assert check(H, COLLECT, nscenes=0) == (NO_SCENES, ERR_STATE)
    assert check(H, COLLECT, enabled=0) == (OFF, ERR_STATE)
    assert check(H, COLLECT, have_out=0) == (NO_OUT, ERR_ARG)


def order(H, fresh, batch_step):
    B = len(fresh)
    f, b = np.ascontiguousarray(fresh, np.int32), np.ascontiguousarray(batch_step, np.int32)
    ids = np.full(B, -1, np.int32)
    count = H.hv_order(B, f.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p))
    assert (ids[count:] == -1).all()                                               # nothing written behind the count
    return ids[:count].tolist()


def test_collect_order(H):
    assert order(H, [0, 0, 0], [5, 5, 5]) == []
    assert order(H, [1, 0, 1, 1], [4, 4, 4, 4]) == [0, 2, 3]                       # one step: ascending ids
    assert order(H, [1, 0, 1, 1, 0, 1], [7, 3, 2, 7, 1, 2]) == [2, 5, 0, 3]        # a burst: by batch step first; stale steps of unfinished scenes do not count
    assert order(H, [1, 1, 1], [3, 2, 1]) == [2, 1, 0]
    assert order(H, [1], [1]) == [0]


def test_standalone_under_sanitizers():
    """The same functions as a program of its own (its own main marks every byte every scene owns on arrays of exactly the block's size)
    under -fsanitize=address,undefined.  Host code only; nothing of it is loaded into python."""
    exe = os.path.join(harness_util.BUILD, 'scene_harvest_harness_san')
    os.makedirs(harness_util.BUILD, exist_ok=True)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan',
                           '-DSCENE_HARVEST_MAIN', '-I' + harness_util.CSRC, '-o', exe, os.path.join(harness_util.ROOT, 'tests', 'scene_harvest_harness.cpp')])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'scene_harvest_harness: ok' in r.stdout


# ---- metrics.episode_metrics_from_harvest ----------------------------------------------------------------------------------------------------
def fabricated(n, seed, flag_choices):
    """an episode as episode_metrics reads it (agents with the reference's attributes) and as a finished scene hands it over: the summary the
    way the device makes it -- integer counts, and the distances of the successful agents added one by one in agent order from 0.0"""
    rng = np.random.default_rng(seed)
    flags = rng.choice(np.array(flag_choices, np.uint8), size=n)
    total_dist = rng.uniform(0.0, 300.0, n) * rng.choice([1.0, 1e-3, 1e3], size=n)         # magnitudes apart: the order of the adds shows
    step_num = rng.integers(1, 4000, n).astype(np.int32)
    agents = [types.SimpleNamespace(is_collision=bool(f & 2), is_out_of_max_time=bool(f & 4), total_dist=float(d), step_num=int(k),
                                    straight_path_length=float(rng.uniform(5.0, 40.0)), desire_steps=int(rng.integers(50, 400)), total_time=0.25 * (i + 1))
              for i, (f, d, k) in enumerate(zip(flags, total_dist, step_num))]
    ok = (flags & 6) == 0
    dist = 0.0
    for d, good in zip(total_dist, ok):
        if good:
            dist = dist + float(d)
    summary = dict(steps=int(step_num.max()), batch_step=1, arrived=int((flags & 1).astype(bool).sum()), collided=int((flags & 2).astype(bool).sum()),
                   timed_out=int((flags & 4).astype(bool).sum()), successful_num=int(ok.sum()), all_step_num=int(step_num[ok].astype(np.int64).sum()),
                   all_distance=dist)
    harvested = dict(flags=flags, total_dist=total_dist, step_num=step_num, summary=summary)
    return agents, harvested, ok


@pytest.mark.parametrize('n,seed,flag_choices', [(100, 5, [1, 1, 1, 2, 4, 3, 5]), (257, 6, [1]), (14, 7, [2, 4, 6]), (1, 8, [1])])
def test_metrics_from_harvest_equal_episode_metrics(n, seed, flag_choices):
    from sca_amd import metrics
    agents, harvested, ok = fabricated(n, seed, flag_choices)
    env = types.SimpleNamespace(agents=agents)
    want = metrics.episode_metrics(env)                                            # (AverageCost from the agents' total_time)
    t = sum(a.total_time for a, good in zip(agents, ok) if good)
    got = metrics.episode_metrics_from_harvest(agents, harvested, t)
    assert list(got) == list(want)                                                 # the same keys in the same order
    for k in want:
        assert got[k] == want[k] or (got[k] != got[k] and want[k] != want[k]), (k, got[k], want[k])      # equality; nan where nobody succeeded
    if n >= 100:
        # the bar is equality with a sequential sum: the same numbers added pairwise (numpy) give another double here
        assert float(np.sum(harvested['total_dist'][ok])) != want['all_distance']
