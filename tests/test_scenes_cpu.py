"""The host-side rules of scene batches (sca_set_scenes) without a GPU: the forest plan (sca_forms.h, plan_kd_forest), the offsets and
permutation checks and the neighbour-mode mapping (sca_scenes.h), behind tests/scenes_harness.cpp.  As in tests/test_forms_cpu.py every
expectation is a literal worked out by hand from the documented rules -- none comes from the code under test."""
import ctypes as C

import numpy as np
import pytest

from harness_util import load_harness

OK, NONE, BAD_COUNT, BAD_START, NOT_INCREASING, BAD_END, TOO_LARGE = range(7)                 # SceneFault
ERR_ARG, ERR_UNSUPPORTED = -1, -5                                                             # include/sca_hip.h
NBR_KDTREE, NBR_GRID, NBR_HOSTBUILD, NBR_AUTO = 0, 1, 2, 3


@pytest.fixture(scope='module')
def H():
    return load_harness('scenes_harness', ('sca_forms.h', 'sca_scenes.h', 'sca_scene_restart.h'))


def i32(a):
    return np.ascontiguousarray(a, np.int32)


def check(H, n, offsets, nscenes=None):
    off = None if offsets is None else i32(offsets)
    out = (C.c_int * 4)()
    H.scenes_check_offsets(n, (len(off) - 1) if nscenes is None else nscenes, None if off is None else off.ctypes.data_as(C.c_void_p), out)
    return tuple(out)


def test_constants(H):
    out = (C.c_int * 3)()
    H.scenes_constants(out)
    assert tuple(out) == (1536, 1024, 512)                     # KD_WAVE_CAP, the grid cap of k_kd_block, SCA_FORM_SCENES


def test_forest_plan_instance_is_the_smallest_that_holds_the_largest_scene(H):
    """the k_kd_block instances are 256, 512, 768, 1024, 1280, 1536 members; one workgroup per scene up to 1024, strided beyond"""
    def instance(size):                                         # the table, written out: edges belong to the smaller instance
        for cap in (256, 512, 768, 1024, 1280, 1536):
            if size <= cap:
                return cap
    out = (C.c_int * 2)()
    for size in range(1, 1537):
        for b in (1, 2, 14, 560, 1023, 1024, 1025, 5000):
            H.scenes_plan_kd_forest(size, b, out)
            assert out[0] == instance(size) and out[0] >= size, (size, b, out[0])
            assert out[1] == min(b, 1024) and 1 <= out[1] <= 1024, (size, b, out[1])
    for b in range(1, 5001):
        H.scenes_plan_kd_forest(100, b, out)
        assert tuple(out) == (256, b if b <= 1024 else 1024), b
    for size, want in ((1, 256), (3, 256), (10, 256), (11, 256), (256, 256), (257, 512), (512, 512), (513, 768), (768, 768), (769, 1024),
                       (1023, 1024), (1024, 1024), (1025, 1280), (1280, 1280), (1281, 1536), (1536, 1536)):
        H.scenes_plan_kd_forest(size, 7, out)
        assert tuple(out) == (want, 7), size


def test_offsets_accepted(H):
    assert check(H, 10, [0, 10]) == (OK, -1, 10, 0)
    assert check(H, 10, [0, 3, 4, 10]) == (OK, -1, 6, 0)
    assert check(H, 3, [0, 1, 2, 3]) == (OK, -1, 1, 0)                         # as many scenes as agents
    assert check(H, 2232, [0, 8, 108, 208, 1232, 2232]) == (OK, -1, 1024, 0)
    assert check(H, 1536, [0, 1536]) == (OK, -1, 1536, 0)                      # the cap itself
    assert check(H, 3072, [0, 1536, 3072]) == (OK, -1, 1536, 0)


def test_no_scenes(H):
    assert check(H, 10, None, nscenes=3) == (NONE, -1, 0, 0)                   # offsets == NULL
    assert check(H, 10, [0, 10], nscenes=0) == (NONE, -1, 0, 0)                # nscenes == 0


def test_offsets_refused(H):
    assert check(H, 10, [0, 4, 4, 10]) == (NOT_INCREASING, 1, 0, ERR_ARG)      # an empty scene
    assert check(H, 10, [0, 6, 4, 10]) == (NOT_INCREASING, 1, 0, ERR_ARG)      # decreasing
    assert check(H, 10, [1, 4, 10]) == (BAD_START, 0, 0, ERR_ARG)
    assert check(H, 10, [0, 4, 9]) == (BAD_END, 1, 0, ERR_ARG)                 # wrong end: short
    assert check(H, 10, [0, 4, 11]) == (BAD_END, 1, 0, ERR_ARG)                # wrong end: long
    assert check(H, 10, [0, 12, 14]) == (BAD_END, 0, 0, ERR_ARG)               # (beyond n in the middle: never read past a per-agent array)
    assert check(H, 10, [0, 10], nscenes=-1) == (BAD_COUNT, -1, 0, ERR_ARG)
    assert check(H, 2, [0, 1, 2, 3]) == (BAD_COUNT, -1, 0, ERR_ARG)            # more scenes than agents
    assert check(H, 1537, [0, 1537]) == (TOO_LARGE, 0, 1537, ERR_UNSUPPORTED)  # one agent over the cap
    assert check(H, 3000, [0, 100, 2000, 3000]) == (TOO_LARGE, 1, 1900, ERR_UNSUPPORTED)


def test_permutation_must_stay_inside_its_scene(H):
    off = i32([0, 3, 8])

    def fault(perm):
        p = i32(perm)
        return H.scenes_perm_check(2, off.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p))
    assert fault([0, 1, 2, 3, 4, 5, 6, 7]) == -1
    assert fault([2, 0, 1, 7, 6, 5, 4, 3]) == -1                               # any order inside a scene
    assert fault([0, 1, 3, 2, 4, 5, 6, 7]) == 2                                # ids 2 and 3 swapped across the boundary: position 2 first
    assert fault([0, 1, 2, 3, 4, 5, 6, 0]) == 7                                # scene 1 holds an id of scene 0
    assert fault([0, 1, 2, 3, 4, 5, 6, 8]) == 7                                # beyond n
    assert fault([-1, 1, 2, 3, 4, 5, 6, 7]) == 0


def test_neighbor_mode_of_a_context_with_scenes(H):
    assert H.scenes_mode(NBR_KDTREE) == NBR_KDTREE
    assert H.scenes_mode(NBR_AUTO) == NBR_KDTREE                                # one more place where the grid cannot help
    assert H.scenes_mode(NBR_GRID) == -1
    assert H.scenes_mode(NBR_HOSTBUILD) == -1
    assert H.scenes_mode(4) == -1 and H.scenes_mode(-1) == -1
