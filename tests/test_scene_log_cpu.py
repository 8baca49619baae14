"""The host-side rules of the trajectory log per scene without a GPU (sca_scenes.h: scene_log_index, scene_log_bytes, scene_log_enable_check,
scene_log_check), behind tests/scene_log_harness.cpp.  Every expectation is a literal worked out by hand from the layout and the refusals
include/sca_hip.h states -- none comes from the code under test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import harness_util
from harness_util import load_harness

OK, NO_SCENES, MID_STEP, STEPPED, OFF, BAD_CAPACITY, BAD_SCENE, BAD_ROWS, BAD_AGENTS = range(9)      # SceneLogFault
ERR_ARG, ERR_STATE = -1, -3                                        # include/sca_hip.h
OFFSETS = [0, 3, 8, 10]                                            # three scenes of 3, 5 and 2 agents
CAP = 4


@pytest.fixture(scope='module')
def H():
    h = load_harness('scene_log_harness', ('sca_scenes.h',))
    h.slog_index.restype = C.c_int64
    h.slog_bytes.restype = C.c_int64
    return h


def index(H, s, r, i, cap=CAP, off=OFFSETS):
    return H.slog_index(cap, off[s], off[s + 1] - off[s], r, i)


def test_index_literals(H):
    # scene 0 owns [0, 12), scene 1 [12, 32), scene 2 [32, 40): capacity x offsets
    assert index(H, 0, 0, 0) == 0
    assert index(H, 0, 1, 0) == 3                                  # pitch n_0 = 3
    assert index(H, 0, 3, 2) == 11
    assert index(H, 1, 0, 0) == 12
    assert index(H, 1, 2, 3) == 25                                 # 12 + 2 * 5 + 3
    assert index(H, 1, 3, 4) == 31
    assert index(H, 2, 0, 0) == 32
    assert index(H, 2, 3, 1) == 39                                 # the last row of the last agent
    assert H.slog_bytes(CAP, 10) == 2560                           # 40 rows of 64 bytes
    assert H.slog_bytes(0, 10) == 0


def test_regions_are_disjoint_and_cover(H):
    regions = []
    for s in range(3):
        n_s = OFFSETS[s + 1] - OFFSETS[s]
        cells = [index(H, s, r, i) for r in range(CAP) for i in range(n_s)]
        assert cells == list(range(cells[0], cells[0] + CAP * n_s))      # [row][agent], contiguous: a window of rows is one copy
        regions.append(set(cells))
    assert regions[0] == set(range(0, 12)) and regions[1] == set(range(12, 32)) and regions[2] == set(range(32, 40))
    assert not (regions[0] & regions[1]) and not (regions[1] & regions[2]) and not (regions[0] & regions[2])
    assert regions[0] | regions[1] | regions[2] == set(range(40))


def test_sixty_four_bits(H):
    # capacity 100 000 x N 1 000 000: 1e11 rows, 6.4e12 bytes -- both beyond 2^32
    assert H.slog_bytes(100000, 1000000) == 6400000000000
    assert H.slog_index(100000, 999000, 1000, 99999, 999) == 99999999999         # the last cell: capacity x N - 1
    assert H.slog_index(100000, 500000, 1000, 0, 0) == 50000000000


def test_rows_logged_and_dropped(H):
    out = (C.c_int * 2)()
    for steps, cap, want in [(0, 5, (0, 0)), (3, 5, (3, 0)), (5, 5, (5, 0)), (12, 5, (5, 7)), (1, 1, (1, 0)), (2, 1, (1, 1))]:
        H.slog_rows(steps, cap, out)
        assert (out[0], out[1]) == want


def enable(H, nscenes, begun, steps, capacity):
    out = (C.c_int * 2)()
    st = None if steps is None else np.ascontiguousarray(steps, np.int32)
    rc = H.slog_enable_check(nscenes, begun, None if st is None else st.ctypes.data_as(C.c_void_p), capacity, out)
    return out[0], out[1], rc


def test_enable_faults(H):
    assert enable(H, 3, 0, [0, 0, 0], 100) == (OK, -1, 0)
    assert enable(H, 0, 0, None, 100) == (NO_SCENES, -1, ERR_STATE)
    assert enable(H, 3, 1, None, 100) == (MID_STEP, -1, ERR_STATE)
    assert enable(H, 3, 0, None, -1) == (BAD_CAPACITY, -1, ERR_ARG)
    assert enable(H, 3, 0, [0, 2, 1], 100) == (STEPPED, 1, ERR_STATE)
    assert enable(H, 3, 0, [0, 0, 1], 1) == (STEPPED, 2, ERR_STATE)
    assert enable(H, 3, 0, None, 0) == (OK, -1, 0)                 # 0 frees: at any step count, the counters are not read
    assert enable(H, 0, 1, None, -1) == (NO_SCENES, -1, ERR_STATE)  # the order of the refusals: state first


def window(H, scene, steps, first, nrows, ab, ac, enabled=1, nscenes=3, window=1, cap=CAP):
    out = (C.c_int * 2)()
    off = np.ascontiguousarray(OFFSETS, np.int32)
    rc = H.slog_check(nscenes, off.ctypes.data_as(C.c_void_p), enabled, cap, window, scene, steps, first, nrows, ab, ac, out)
    return out[0], out[1], rc


def test_window_faults(H):
    assert window(H, 1, 3, 0, 3, 0, 5) == (OK, 1, 0)
    assert window(H, 1, 3, 2, 1, 4, 1) == (OK, 1, 0)
    assert window(H, 1, 3, 0, 0, 0, 0) == (OK, 1, 0)               # empty windows are fine
    assert window(H, 1, 0, 0, 0, 0, 5) == (OK, 1, 0)
    assert window(H, 0, 3, 0, 1, 0, 1, nscenes=0) == (NO_SCENES, -1, ERR_STATE)
    assert window(H, 0, 3, 0, 1, 0, 1, enabled=0) == (OFF, -1, ERR_STATE)
    assert window(H, 0, 0, 0, 0, 0, 0, enabled=0, window=0) == (OFF, -1, ERR_STATE)
    assert window(H, 9, 0, 0, 0, 0, 0, window=0) == (OK, -1, 0)    # sca_scene_history_rows names no scene
    assert window(H, -1, 3, 0, 1, 0, 1) == (BAD_SCENE, -1, ERR_ARG)
    assert window(H, 3, 3, 0, 1, 0, 1) == (BAD_SCENE, 3, ERR_ARG)
    assert window(H, 1, 3, 0, 4, 0, 5) == (BAD_ROWS, 1, ERR_ARG)    # 3 rows logged
    assert window(H, 1, 3, 3, 1, 0, 5) == (BAD_ROWS, 1, ERR_ARG)
    assert window(H, 1, 3, -1, 1, 0, 5) == (BAD_ROWS, 1, ERR_ARG)
    assert window(H, 1, 3, 0, -1, 0, 5) == (BAD_ROWS, 1, ERR_ARG)
    assert window(H, 1, 9, 0, 5, 0, 5) == (BAD_ROWS, 1, ERR_ARG)    # 9 steps, capacity 4: rows 4 .. 8 were counted, never written
    assert window(H, 1, 9, 0, 4, 0, 5) == (OK, 1, 0)
    assert window(H, 1, 3, 0, 1, 0, 6) == (BAD_AGENTS, 1, ERR_ARG)  # scene 1 holds 5
    assert window(H, 2, 3, 0, 1, 1, 2) == (BAD_AGENTS, 2, ERR_ARG)
    assert window(H, 2, 3, 0, 1, -1, 1) == (BAD_AGENTS, 2, ERR_ARG)
    assert window(H, 2, 3, 0, 1, 0, -1) == (BAD_AGENTS, 2, ERR_ARG)
    assert window(H, 1, 3, 2147483647, 1, 0, 1) == (BAD_ROWS, 1, ERR_ARG)      # first_row + nrows does not wrap
    assert window(H, 1, 3, 0, 1, 2147483647, 1) == (BAD_AGENTS, 1, ERR_ARG)


def test_standalone_under_sanitizers():
    """The same functions as a program of its own (its own main walks whole layouts on arrays of exactly the log's size) under
    -fsanitize=address,undefined.  Host code only; nothing of it is loaded into python."""
    exe = os.path.join(harness_util.BUILD, 'scene_log_harness_san')
    os.makedirs(harness_util.BUILD, exist_ok=True)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan',
                           '-DSCENE_LOG_MAIN', '-I' + harness_util.CSRC, '-o', exe, os.path.join(harness_util.ROOT, 'tests', 'scene_log_harness.cpp')])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'scene_log_harness: ok' in r.stdout
