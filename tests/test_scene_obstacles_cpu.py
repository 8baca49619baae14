"""The host-side rules of per-scene obstacle sets (sca_set_scene_obstacles) without a GPU: the offsets check and its error codes, the
per-scene obstacle root, and the shift of a single-scene tree into the forest (sca_scenes.h), behind tests/scenes_harness.cpp.
As in tests/test_scenes_cpu.py every expectation is a literal worked out by hand from the documented rules -- none comes from the code
under test."""
import ctypes as C
import os

import numpy as np
import pytest

from harness_util import ROOT, load_harness

OK, BAD_COUNT, NO_OFFSETS, BAD_START, DECREASING, TOO_MANY, NO_ARRAYS = range(7)               # SceneObsFault
ERR_ARG = -1                                                                                  # include/sca_hip.h


@pytest.fixture(scope='module')
def H():
    return load_harness('scenes_harness', ('sca_forms.h', 'sca_scenes.h', 'sca_scene_restart.h'))


def i32(a):
    return np.ascontiguousarray(a, np.int32)


def check(H, ctx_nscenes, max_obstacles, offsets, nscenes=None, pos=True, radius=True):
    off = None if offsets is None else i32(offsets)
    out = (C.c_int * 4)()
    H.scene_obs_check(ctx_nscenes, max_obstacles, (len(off) - 1) if nscenes is None else nscenes,
                      None if off is None else off.ctypes.data_as(C.c_void_p), int(pos), int(radius), out)
    return tuple(out)


def roots(H, offsets):
    off = i32(offsets)
    out = np.zeros(len(off) - 1, np.int32)
    H.scene_obs_roots(len(off) - 1, off.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out.tolist()


def test_the_form_bit_is_the_next_free_one(H):
    out = (C.c_int * 2)()
    H.scene_obs_constants(out)
    assert tuple(out) == (1024, 512)                           # SCA_FORM_SCENE_OBSTACLES, SCA_FORM_SCENES
    from sca_amd import solver as S
    assert S.FORM_SCENE_OBSTACLES == 1024
    hdr = open(os.path.join(ROOT, 'include', 'sca_hip.h')).read()
    assert '#define SCA_FORM_SCENE_OBSTACLES 1024' in hdr


def test_offsets_accepted(H):
    assert check(H, 3, 100, [0, 8, 8, 20]) == (OK, -1, 20, 0)                   # a scene without obstacles in the middle
    assert check(H, 3, 20, [0, 0, 8, 20]) == (OK, -1, 20, 0)                    # ... first, and a total that is exactly max_obstacles
    assert check(H, 3, 20, [0, 8, 20, 20]) == (OK, -1, 20, 0)                   # ... last
    assert check(H, 1, 1491, [0, 1491]) == (OK, -1, 1491, 0)
    assert check(H, 4, 5, [0, 0, 0, 0, 0]) == (OK, -1, 0, 0)                    # a total of 0 is "no obstacles"
    assert check(H, 4, 5, [0, 0, 0, 0, 0], pos=False, radius=False) == (OK, -1, 0, 0)   # ... and needs no arrays
    assert check(H, 2, 0, [0, 0, 0]) == (OK, -1, 0, 0)


def test_offsets_refused(H):
    assert check(H, 3, 100, [0, 8, 20]) == (BAD_COUNT, -1, 0, ERR_ARG)          # two sets for three scenes
    assert check(H, 3, 100, [0, 8, 20, 21, 30]) == (BAD_COUNT, -1, 0, ERR_ARG)  # four sets for three scenes
    assert check(H, 3, 100, [0, 8, 8, 20], nscenes=0) == (BAD_COUNT, -1, 0, ERR_ARG)
    assert check(H, 3, 100, [0, 8, 8, 20], nscenes=-3) == (BAD_COUNT, -1, 0, ERR_ARG)
    assert check(H, 3, 100, None, nscenes=3) == (NO_OFFSETS, -1, 0, ERR_ARG)
    assert check(H, 3, 100, [1, 8, 8, 20]) == (BAD_START, 0, 0, ERR_ARG)
    assert check(H, 3, 100, [-1, 8, 8, 20]) == (BAD_START, 0, 0, ERR_ARG)
    assert check(H, 3, 100, [0, 8, 7, 20]) == (DECREASING, 1, 0, ERR_ARG)
    assert check(H, 3, 100, [0, 8, 20, 19]) == (DECREASING, 2, 0, ERR_ARG)
    assert check(H, 3, 100, [0, -1, 20, 30]) == (DECREASING, 0, 0, ERR_ARG)     # (so no offset is negative)
    assert check(H, 3, 19, [0, 8, 8, 20]) == (TOO_MANY, -1, 20, ERR_ARG)        # one above max_obstacles
    assert check(H, 3, 0, [0, 0, 0, 1]) == (TOO_MANY, -1, 1, ERR_ARG)
    assert check(H, 3, 100, [0, 8, 8, 20], pos=False) == (NO_ARRAYS, -1, 20, ERR_ARG)
    assert check(H, 3, 100, [0, 8, 8, 20], radius=False) == (NO_ARRAYS, -1, 20, ERR_ARG)
    assert check(H, 3, 100, [0, 0, 0, 1], pos=False, radius=False) == (NO_ARRAYS, -1, 1, ERR_ARG)
    # the first broken rule is the one reported: the count before the start, the start before the order, the order before the total
    assert check(H, 2, 100, [1, 8, 7, 200]) == (BAD_COUNT, -1, 0, ERR_ARG)
    assert check(H, 3, 100, [1, 8, 7, 200]) == (BAD_START, 0, 0, ERR_ARG)
    assert check(H, 3, 100, [0, 8, 7, 200]) == (DECREASING, 1, 0, ERR_ARG)
    assert check(H, 3, 100, [0, 8, 9, 200], pos=False) == (TOO_MANY, -1, 200, ERR_ARG)


def test_root_rule(H):
    """m_s > 0 ? 2 * obs_offsets[s] : -1"""
    assert roots(H, [0, 8]) == [0]
    assert roots(H, [0, 0]) == [-1]
    assert roots(H, [0, 0, 8, 20]) == [-1, 0, 16]                               # an empty scene first: the next one still starts at record 0
    assert roots(H, [0, 8, 8, 20]) == [0, -1, 16]                               # ... in the middle
    assert roots(H, [0, 8, 20, 20]) == [0, 16, -1]                              # ... last
    assert roots(H, [0, 0, 0, 0]) == [-1, -1, -1]
    assert roots(H, [0, 0, 1, 11, 22, 45]) == [-1, 0, 2, 22, 44]
    assert roots(H, [0, 1491, 1491, 1499]) == [0, -1, 2982]


# Trees over 1, 10, 11 and 23 members as kdTree.py:162-227 numbers them -- children of node i at i + 1 and i + 2 * leftSize, a node of <= 10
# members is a leaf with links 0 -- written out by hand: (begin, end, left, right) per node index; the other records of the 2k - 1 are unused.
#   11 members split 5 | 6:  0 [0,11) -> 1, 10;  1 [0,5);  10 [5,11)
#   23 members split 12 | 11, then 6 | 6 and 5 | 6:  0 [0,23) -> 1, 24;  1 [0,12) -> 2, 13;  2 [0,6);  13 [6,12);  24 [12,23) -> 25, 34;  25 [12,17);  34 [17,23)
TREES = {1: {0: (0, 1, 0, 0)},
         10: {0: (0, 10, 0, 0)},
         11: {0: (0, 11, 1, 10), 1: (0, 5, 0, 0), 10: (5, 11, 0, 0)},
         23: {0: (0, 23, 1, 24), 1: (0, 12, 2, 13), 2: (0, 6, 0, 0), 13: (6, 12, 0, 0), 24: (12, 23, 25, 34), 25: (12, 17, 0, 0), 34: (17, 23, 0, 0)}}
# ... and the same trees where scenes of 0, 1, 10, 11 and 23 obstacles put them: obs_offsets = 0 0 1 11 22 45, node bases 2 * obs_offsets
FOREST = {1: {0: (0, 1, 0, 0)},
          10: {0: (1, 11, 0, 0)},
          11: {0: (11, 22, 23, 32), 1: (11, 16, 0, 0), 10: (16, 22, 0, 0)},
          23: {0: (22, 45, 45, 68), 1: (22, 34, 46, 57), 2: (22, 28, 0, 0), 13: (28, 34, 0, 0), 24: (34, 45, 69, 78), 25: (34, 39, 0, 0), 34: (39, 45, 0, 0)}}
OBS_OFF = [0, 0, 1, 11, 22, 45]


def shifted(H, k, obs_begin):
    nodes = np.zeros((2 * k - 1, 4), np.int32)
    for i, rec in TREES[k].items():
        nodes[i] = rec
    H.scene_obs_shift(nodes.ctypes.data_as(C.c_void_p), len(nodes), obs_begin)
    return nodes


def test_forest_shift_on_a_hand_worked_case(H):
    sizes = np.diff(OBS_OFF).tolist()
    assert sizes == [0, 1, 10, 11, 23]
    used = np.zeros(2 * OBS_OFF[-1], bool)                                      # records of otree[2M] / owide[2M] some scene owns
    for s, k in enumerate(sizes):
        if k == 0:
            continue
        lo, hi, base = OBS_OFF[s], OBS_OFF[s + 1], 2 * OBS_OFF[s]
        nodes = shifted(H, k, lo)
        want = np.zeros((2 * k - 1, 4), np.int32)
        for i, rec in FOREST[k].items():
            want[i] = rec
        assert np.array_equal(nodes, want), (k, nodes.tolist())
        # the scene's node range [base, base + 2k - 1) lies inside the arrays and overlaps nobody's
        assert base + 2 * k - 1 <= 2 * OBS_OFF[-1]
        assert not used[base:base + 2 * k - 1].any(), s
        used[base:base + 2 * k - 1] = True
        for i in FOREST[k]:
            b, e, left, right = nodes[i].tolist()
            assert lo <= b < e <= hi, (k, i)
            if e - b > 10:                                                      # an inner node: both children inside the scene's node range
                assert base < left < base + 2 * k - 1 and base < right < base + 2 * k - 1, (k, i)
                assert tuple(nodes[left - base][:2]) == (b, nodes[right - base][0]) and nodes[right - base][1] == e, (k, i)
            else:
                assert (left, right) == (0, 0), (k, i)
        for i in range(2 * k - 1):                                              # unused records stay untouched
            if i not in FOREST[k]:
                assert not nodes[i].any(), (k, i)
    assert used.sum() == 1 + 19 + 21 + 45


def test_shift_by_zero_is_the_single_scene_tree(H):
    for k in TREES:
        want = np.zeros((2 * k - 1, 4), np.int32)
        for i, rec in TREES[k].items():
            want[i] = rec
        assert np.array_equal(shifted(H, k, 0), want), k
