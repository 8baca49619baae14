"""The host-side rules of sca_restart_scenes_attrs without a GPU (sca_scenes.h behind tests/scene_attrs_harness.cpp): every refusal of the
descriptor's check with its entry and code, the attribute sections of the staging block, and the tracker's class table as a pure function.
Every expectation is a literal worked out by hand from the rules in include/sca_hip.h -- none comes from the code under test.  The same
harness then runs as a program of its own under AddressSanitizer and UBSan."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from harness_util import BUILD, CSRC, ROOT, load_harness

OK, STRUCT, RESERVED, NO_TRACKER, SOLVER, PLANNER = range(6)       # RestartAttrFault
ERR_ARG = -1
STATE, BEGUN, TRACKER = 1, 2, 4
OFFSETS = [0, 4, 24, 30]                                           # three slots of capacity 4, 20 and 6
POLICY_NOW = [i % 6 for i in range(30)]                            # rows 0, 5, 6, 11, ... are tracked (SCA 0, RVO3D+Dubins 5)
DEFAULTS = [10.0, 0.1, 10.0, 1.0, math.pi / 4, 0.1, 16.0, 1.5, -0.5, 0.5]
NAMES = ('neighbor_dist', 'max_neighbors', 'time_step', 'time_horizon', 'max_speed', 'max_heading_change', 'dt_nominal', 'turning_radius',
         'pitch_lo', 'pitch_hi')
STRUCT_BYTES = 88                                                  # two int32 and ten pointers
IDS, SIZES = [1, 0], [20, 4]                                       # packed rows 0 .. 19: scene 1's rows 4 .. 23; 20 .. 23: scene 0's rows 0 .. 3
T = 24


@pytest.fixture(scope='module')
def H():
    h = load_harness('scene_attrs_harness', ('sca_scenes.h',))
    h.class_table_new.restype = C.c_void_p
    h.class_table_free.argtypes = [C.c_void_p]
    return h


def valid():
    return dict(neighbor_dist=np.full(T, 5.0), max_neighbors=np.full(T, 8, np.int32), time_step=np.full(T, 0.2), time_horizon=np.full(T, 3.0),
                max_speed=np.full(T, 1.5), max_heading_change=np.full(T, 0.5), dt_nominal=np.full(T, 0.05), turning_radius=np.full(T, 3.0),
                pitch_lo=np.full(T, -0.3), pitch_hi=np.full(T, 0.3))


def check(H, ctx=STATE | TRACKER, struct_bytes=STRUCT_BYTES, reserved=0, policy=None, ids=IDS, sizes=SIZES, **arrays):
    """(fault, entry, mask of the members read, error code); arrays: replace valid()'s, None for a NULL member"""
    a = valid()
    a.update(arrays)
    keep = []

    def p(x, dt):
        if x is None:
            return None
        x = np.ascontiguousarray(x, dt)
        keep.append(x)
        return x.ctypes.data_as(C.c_void_p)
    ptrs = (C.c_void_p * 10)(*[None if a[k] is None else p(a[k], np.int32 if k == 'max_neighbors' else np.float64).value for k in NAMES])
    out = (C.c_int * 3)()
    rc = H.attrs_check(3, p(OFFSETS, np.int32), ctx, p(POLICY_NOW, np.uint8), len(ids), p(ids, np.int32), p(sizes, np.int32), p(policy, np.uint8),
                       struct_bytes, reserved, ptrs, p(DEFAULTS, np.float64), out)
    return out[0], out[1], out[2], rc


def put(key, row, value):
    a = valid()[key]
    a[row] = value
    return {key: a}


def test_a_valid_descriptor_and_how_far_struct_bytes_reaches(H):
    assert H.attrs_struct_bytes() == STRUCT_BYTES
    assert check(H) == (OK, -1, 0x3ff, 0)
    assert check(H, struct_bytes=64) == (OK, -1, 0x07f, 0)             # a caller compiled before the planner members: they read as NULL
    assert check(H, struct_bytes=8) == (OK, -1, 0, 0)                  # the two integers alone: every array NULL
    assert check(H, **{k: None for k in NAMES}) == (OK, -1, 0, 0)
    assert check(H, ctx=STATE, turning_radius=None, pitch_lo=None, pitch_hi=None) == (OK, -1, 0x07f, 0)       # no tracker, no planner arrays
    assert check(H, ctx=STATE, struct_bytes=64) == (OK, -1, 0x07f, 0)  # ... or planner arrays behind what the struct claims


@pytest.mark.parametrize('struct_bytes', [-1, 0, 4, 7, 12, 87, 89, 96])
def test_struct_bytes_that_is_no_size_of_the_struct(H, struct_bytes):
    """below the two leading integers, above the library's struct, or cutting a pointer in two"""
    assert check(H, struct_bytes=struct_bytes) == (STRUCT, -1, 0, ERR_ARG)


def test_reserved_and_planner_arrays_without_a_tracker(H):
    assert check(H, reserved=1) == (RESERVED, -1, 0, ERR_ARG)
    for k in ('turning_radius', 'pitch_lo', 'pitch_hi'):
        only = {n: None for n in NAMES if n != k}
        assert check(H, ctx=STATE, **only) == (NO_TRACKER, -1, 0, ERR_ARG), k
        assert check(H, **only)[0] == OK, k


@pytest.mark.parametrize('key,value', [('neighbor_dist', 0.0), ('neighbor_dist', float('nan')), ('neighbor_dist', float('inf')), ('max_neighbors', 0),
                                       ('max_neighbors', 17), ('time_step', -0.1), ('time_horizon', 0.0), ('max_speed', float('inf')),
                                       ('max_heading_change', -0.1), ('max_heading_change', 3.2), ('max_heading_change', float('nan')),
                                       ('dt_nominal', 0.0)])
def test_solver_attributes_out_of_range_name_their_row(H, key, value):
    """sca_set_agent_params' rules per row, whatever the row's policy; the first bad row is named"""
    for row in (0, 19, 20, 23):                                    # both ends of both named scenes' packed rows
        assert check(H, **put(key, row, value)) == (SOLVER, row, 0, ERR_ARG), row
    two = valid()[key]
    two[[7, 3]] = value
    assert check(H, **{key: two}) == (SOLVER, 3, 0, ERR_ARG)


def test_the_limits_themselves_pass(H):
    assert check(H, **put('max_neighbors', 5, 1))[0] == OK and check(H, **put('max_neighbors', 5, 16))[0] == OK
    assert check(H, **put('max_heading_change', 5, 0.0))[0] == OK and check(H, **put('max_heading_change', 5, math.pi))[0] == OK


@pytest.mark.parametrize('key,value', [('turning_radius', 0.0), ('turning_radius', float('nan')), ('turning_radius', float('inf')),
                                       ('pitch_lo', 0.3), ('pitch_lo', float('nan')), ('pitch_hi', -0.3), ('pitch_hi', float('inf'))])
def test_planner_attributes_are_checked_on_tracked_rows_only(H, key, value):
    """packed row r of scene 1 is context row 4 + r, policy (4 + r) % 6: tracked for r = 1 (5), 2 (0), 7, 8, ...; packed row 20 is row 0 (0)"""
    for row in (1, 2, 7, 20):
        assert check(H, **put(key, row, value)) == (PLANNER, row, 0, ERR_ARG), row
    for row in (0, 3, 19, 21):                                     # policies 4, 1, 5 -> no: (4 + 19) % 6 = 5 is tracked
        want = (PLANNER, row, 0, ERR_ARG) if POLICY_NOW[(4 + row) if row < 20 else row - 20] in (0, 5) else (OK, -1, 0x3ff, 0)
        assert check(H, **put(key, row, value)) == want, row
    # the episode's own policies decide, where it brings them: all ORCA -> nobody is tracked; all SCA -> everybody
    assert check(H, policy=np.full(T, 3), **put(key, 1, value))[0] == OK
    assert check(H, policy=np.full(T, 0), **put(key, 0, value)) == (PLANNER, 0, 0, ERR_ARG)


def test_a_null_planner_array_stands_for_the_enable_value(H):
    """pitch_lo NULL = -0.5 for every row: a pitch_hi of -0.5 is then out of range, one of 0.0 is not"""
    assert check(H, pitch_lo=None, **put('pitch_hi', 1, -0.5)) == (PLANNER, 1, 0, ERR_ARG)
    assert check(H, pitch_lo=None, **put('pitch_hi', 1, 0.0))[0] == OK


def test_a_solver_fault_is_found_before_a_planner_fault(H):
    a = dict(put('turning_radius', 1, 0.0), **put('time_step', 9, 0.0))
    assert check(H, **a) == (SOLVER, 9, 0, ERR_ARG)


# ---- the block's sections ------------------------------------------------------------------------------------------------------------------
def sections(H, max_n, max_m):
    begin, size, total = (C.c_int64 * 32)(), (C.c_int64 * 32)(), C.c_int64()
    k = H.block_sections(max_n, max_m, begin, size, C.byref(total))
    return list(begin[:k]), list(size[:k]), total.value


@pytest.mark.parametrize('max_n,max_m', [(1, 1), (60, 1), (130, 9), (1536, 1491), (4097, 3)])
def test_sections_are_disjoint_aligned_and_inside_the_block(H, max_n, max_m):
    begin, size, total = sections(H, max_n, max_m)
    assert len(begin) == 13 + 1 + 6 + 4 and H.attr_section_count() == 4
    for k in range(len(begin)):
        assert begin[k] % 64 == 0 and begin[k] % 16 == 0, k
        assert begin[k] + size[k] <= (begin[k + 1] if k + 1 < len(begin) else total), k
    assert size[-4:] == [64 * max_n, 8 * max_n, 24 * max_n, max_n]         # AgentPar rows, neighborDist, the planner triple, the class byte
    assert total % 64 == 0


def test_the_attribute_sections_at_one_row(H):
    """max_n = 1: each of the four sections is one 64-byte unit, behind the obstacle sections"""
    begin, size, total = sections(H, 1, 1)
    obs_end = begin[-5] + 64 * 4                                   # RO_WIDE: 128 bytes x 2 records x 1 obstacle = 256
    assert begin[-4:] == [obs_end, obs_end + 64, obs_end + 128, obs_end + 192] and total == obs_end + 256


# ---- the class table -----------------------------------------------------------------------------------------------------------------------
A, B_, C_, D_, E_ = (1.5, -0.5, 0.5), (3.0, -0.5, 0.5), (1.5, -0.2, 0.5), (1.5, -0.5, 0.2), (8.0, -1.0, 1.0)


class Table:
    """three slots (OFFSETS), every row tracked unless said otherwise"""

    def __init__(self, H):
        self.H, self.t = H, C.c_void_p(H.class_table_new())
        self.size = np.array([4, 20, 6], np.int32)
        self.policy = np.zeros(30, np.uint8)
        self.trip = np.tile(np.array(A), (30, 1))
        self.cls = np.zeros(30, np.uint8)

    def close(self):
        self.H.class_table_free(self.t)

    def update(self, travels=()):
        tv = np.zeros(30, np.uint8)
        for s in travels:
            tv[OFFSETS[s]:OFFSETS[s + 1]] = 1
        out = (C.c_int * 3)()
        off = np.array(OFFSETS, np.int32)
        self.trip = np.ascontiguousarray(self.trip, np.float64)
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        self.H.class_table_update(self.t, 3, vp(off), vp(self.size), vp(self.policy), vp(self.trip), 30, vp(self.cls), vp(tv), out)
        val, users, many, only = (C.c_double * 48)(), (C.c_int32 * 16)(), C.c_int(), C.c_int()
        used = self.H.class_table_get(self.t, val, users, C.byref(many), C.byref(only))
        self.val = [tuple(val[3 * k:3 * k + 3]) for k in range(16)]
        self.users = list(users)
        return dict(classes=out[0], many=out[1], moved=out[2], used=used, only=only.value)

    def scene(self, s, trip):
        self.trip[OFFSETS[s]:OFFSETS[s + 1]] = trip


@pytest.fixture
def table(H):
    t = Table(H)
    yield t
    t.close()


def test_one_class_means_scalars(table):
    r = table.update()
    assert r == dict(classes=1, many=0, moved=0, used=1, only=0) and not table.cls.any()
    assert table.val[0] == A and table.users == [30] + [0] * 15


def test_indices_are_stable_while_a_row_uses_the_class(table):
    table.scene(1, B_); table.scene(2, C_)
    r = table.update(travels=(1, 2))
    assert r == dict(classes=3, many=0, moved=0, used=3, only=-1)
    assert table.cls.tolist() == [0] * 4 + [1] * 20 + [2] * 6 and table.users[:3] == [4, 20, 6]
    # scene 0 takes D: nobody uses A any more, its index is free and D is the first to ask -- scenes 1 and 2 keep 1 and 2
    table.scene(0, D_)
    r = table.update(travels=(0,))
    assert r == dict(classes=3, many=0, moved=0, used=3, only=-1)
    assert table.cls.tolist() == [0] * 4 + [1] * 20 + [2] * 6 and table.val[:3] == [D_, B_, C_]
    # scene 1 takes C: index 1 falls free, and stays free -- scene 0 and scene 2 do not move
    table.scene(1, C_)
    r = table.update(travels=(1,))
    assert r == dict(classes=2, many=0, moved=0, used=2, only=-1)
    assert table.cls.tolist() == [0] * 4 + [2] * 20 + [2] * 6 and table.users[:3] == [4, 0, 26]
    # half of scene 0 takes E, the lowest free index: 1
    table.trip[2:4] = E_
    r = table.update(travels=(0,))
    assert r == dict(classes=3, many=0, moved=0, used=3, only=-1)
    assert table.cls.tolist() == [0, 0, 1, 1] + [2] * 26 and table.val[1] == E_
    # back to one class: index 2 alone, whose values go into the scalars
    table.scene(0, C_)
    r = table.update(travels=(0,))
    assert r == dict(classes=1, many=0, moved=0, used=1, only=2) and table.val[2] == C_


def test_a_byte_that_moves_outside_the_block_is_reported(table):
    table.scene(1, B_)
    assert table.update(travels=(1,))['moved'] == 0
    table.scene(2, C_)
    assert table.update(travels=())['moved'] == 1                  # scene 2's bytes became 2 and travel with nobody
    assert table.update(travels=())['moved'] == 0                  # ... once


def test_a_seventeenth_triple_gives_the_per_agent_form_and_sixteen_give_classes_again(table):
    table.scene(2, B_)
    for i in range(15):                                            # scene 1: fifteen triples of its own -> A, B and these: 17
        table.trip[4 + i] = (10.0 + i, -0.5, 0.5)
    before = table.cls.copy()
    r = table.update(travels=(1, 2))
    assert r == dict(classes=17, many=1, moved=0, used=0, only=-1)
    assert np.array_equal(table.cls, before) and table.users == [0] * 16
    table.trip[18] = A                                             # one fewer: 16 triples, classes again, dealt afresh in row order
    r = table.update(travels=(1,))
    assert (r['classes'], r['many'], r['used']) == (16, 0, 16)
    assert r['moved'] == 1                                         # scene 2's rows were 0 and are B's index now
    assert table.cls[:4].tolist() == [0] * 4 and table.cls[4:18].tolist() == list(range(1, 15)) and table.cls[18] == 0
    assert table.cls[19:24].tolist() == [0] * 5 and table.cls[24:].tolist() == [15] * 6
    assert table.val[15] == B_ and table.val[1] == (10.0, -0.5, 0.5)


def test_exactly_sixteen_are_classes(table):
    for i in range(15):
        table.trip[4 + i] = (10.0 + i, -0.5, 0.5)
    r = table.update(travels=(1,))
    assert (r['classes'], r['many'], r['used']) == (16, 0, 16)


def test_vacant_rows_and_untracked_policies_are_not_counted(table):
    for i in range(20):                                            # scene 1: twenty triples of its own ...
        table.trip[4 + i] = (10.0 + i, -0.5, 0.5)
    table.size[1] = 2                                              # ... of which two rows are occupied
    table.policy[24:30] = [1, 2, 3, 4, 1, 2]                       # scene 2: nobody tracked, whatever its triples
    table.scene(2, E_)
    before = table.cls.copy()
    r = table.update(travels=(1,))
    assert r == dict(classes=3, many=0, moved=0, used=3, only=-1)
    assert table.users[:3] == [4, 1, 1] and table.val[:3] == [A, (10.0, -0.5, 0.5), (11.0, -0.5, 0.5)]
    assert table.cls[:6].tolist() == [0, 0, 0, 0, 1, 2] and np.array_equal(table.cls[6:], before[6:])    # vacant and untracked rows keep their bytes
    table.policy[24] = 5                                           # one row of scene 2 becomes tracked: E counts
    r = table.update(travels=(2,))
    assert (r['classes'], table.cls[24], table.val[3]) == (4, 3, E_)


# ---- the harness as a program of its own under the sanitizers ---------------------------------------------------------------------------------
def test_the_harness_alone_under_asan_and_ubsan(H):
    """tests/scene_attrs_harness.cpp with its own main, -fsanitize=address,undefined: no report, and every line it prints is what the same
    calls answer here"""
    probe = subprocess.run(['gcc', '-print-file-name=libasan.so'], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip('libasan.so not found')
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, 'scene_attrs_asan')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-Wall', '-Wextra', '-Werror', '-DSCENE_ATTRS_MAIN', '-I' + CSRC, '-o', exe, os.path.join(ROOT, 'tests', 'scene_attrs_harness.cpp')])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1'))
    out = run.stdout[-4000:] + '\n' + run.stderr[-6000:]
    assert run.returncode == 0 and 'AddressSanitizer' not in out and 'runtime error' not in out, out
    lines = run.stdout.strip().split('\n')
    sb = STRUCT_BYTES
    want = ['check bytes 0: rc 0 fault 0 entry -1 read 899',           # members 0, 1, 7, 8, 9: 1 + 2 + 128 + 256 + 512
            'check bytes -24: rc 0 fault 0 entry -1 read 3',
            'check bytes %d: rc 0 fault 0 entry -1 read 0' % (8 - sb),
            'check bytes %d: rc -1 fault 1 entry -1 read 0' % (4 - sb),
            'check bytes 8: rc -1 fault 1 entry -1 read 0',
            'check bytes %d: rc -1 fault 1 entry -1 read 0' % (12 - sb),
            'check no tracker: rc -1 fault 3 entry -1',
            'check reserved: rc -1 fault 2 entry -1',
            'check solver row: rc -1 fault 4 entry 17',
            'check planner row: rc -1 fault 5 entry 19']               # packed row 17 is context row 21, policy 3: untracked; 19 -> row 23, policy 5
    assert lines[:10] == want, lines[:10]
    for line, (max_n, max_m) in zip(lines[10:12], [(1, 9), (130, 9)]):
        begin, size, total = sections(H, max_n, max_m)
        assert line == 'layout %d:' % max_n + ''.join(' %d+%d' % bs for bs in zip(begin, size)) + ' total %d' % total
    three = [i % 3 for i in range(30)]
    back = list(three)
    for k, i in enumerate(range(4, 14)):
        back[i] = 3 + k                                            # indices 0, 1, 2 are in use by scenes 0 and 2; the ten new triples take 3 .. 12
    assert lines[12] == 'table three: classes 3 many 0 moved 1 used 3 only -1 cls ' + ' '.join(map(str, three))
    assert lines[13] == 'table many: classes 17 many 1 moved 0 used 0 only -1 cls ' + ' '.join(map(str, three))
    assert lines[14].startswith('table back: classes 13 many 0 moved 1 used 13 only -1 cls ')
    got = [int(x) for x in lines[14].split(' cls ')[1].split()]
    assert got[14:24] == three[14:24]                              # the vacant rows keep their bytes
    assert sorted(set(got[4:14])) == sorted(set(range(13)) - set(got[:4]) - set(got[24:])) and len(set(got[4:14])) == 10
    assert lines[15].startswith('table one: classes 1 many 0 moved 1 used 1 only ')
    assert len(lines) == 16
