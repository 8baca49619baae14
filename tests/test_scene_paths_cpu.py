"""The waypoint lists' slot form without a GPU (sca_scenes.h and sca_core.h behind tests/scene_paths_harness.cpp): every branch and code of
path_slots_check (sca_set_path_slots) and restart_paths_check (sca_restart_scenes_paths), the path sections of the restart's staging block,
the row-to-place index, the header's three new exports, and the body k_waypoint and k_waypoint_slots share, compiled for the host and run
in slot form over the path corpus of tests/test_form_fuzz_cpu.py against tests/path_rule.py and against the block form.  Expectations of the
checks are literals worked out by hand from the rules in include/sca_hip.h -- none comes from the code under test.  The same harness then
runs as a program of its own under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import form_fuzz as F
import path_rule as R
from harness_util import BUILD, CSRC, ROOT

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5
# PathSlotFault / RestartPathFault
S_OK, S_NO_AGENTS, S_PARTITION, S_BAD_N, S_BAD_W, S_TOO_LARGE, S_BAD_START, S_DECREASING, S_TOO_LONG, S_NO_POINTS, S_NOT_FINITE = range(11)
P_OK, P_NO_SLOTS, P_BAD_START, P_DECREASING, P_TOO_LONG, P_NO_POINTS, P_NOT_FINITE = range(7)
SRC = os.path.join(ROOT, 'tests', 'scene_paths_harness.cpp')
# the arithmetic of sca_core.h as the library and tests/path_harness.cpp build it (unfused, the restated libm with -mfma); the header's
# `#pragma unroll` is the device compiler's
FLAGS = ['-std=c++17', '-ffp-contract=off', '-mfma', '-fno-builtin-pow', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I' + CSRC]
OFF = [0, 2, 2, 5, 6]                                              # four rows: lists of 2, 0, 3 and 1 waypoints
PTS = np.arange(18, dtype=np.float64).reshape(6, 3)


@pytest.fixture(scope='module')
def H():
    out = os.path.join(BUILD, 'libscene_paths_harness.so')
    deps = [SRC, os.path.join(ROOT, 'include', 'sca_hip.h')] + [os.path.join(CSRC, f) for f in
                                                                ('sca_scenes.h', 'sca_core.h', 'sca_glibc_math.h', 'sca_glibc_tables.h', 'sca_constants.h')]
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(['g++', '-O2', '-fPIC', '-shared'] + FLAGS + ['-o', out, SRC])
    h = C.CDLL(out)
    h.slot_index.restype = C.c_int64
    h.points_max.restype = C.c_int64
    h.path_bits.restype = C.c_uint32
    return h


def _p(x, dt, keep):
    if x is None:
        return None
    x = np.ascontiguousarray(x, dt)
    keep.append(x)
    return x.ctypes.data_as(C.c_void_p)


def slots(H, agents_set=1, partition=0, ctx_n=4, max_agents=8, W=3, n=4, off=OFF, pts=PTS):
    """(fault, entry, total, code) of path_slots_check"""
    keep, out = [], (C.c_int * 3)()
    rc = H.slots_check(agents_set, partition, ctx_n, max_agents, W, n, _p(off, np.int32, keep), _p(pts, np.float64, keep), out)
    return out[0], out[1], out[2], rc


def paths(H, slot_form=1, W=3, T=4, off=OFF, pts=PTS):
    """(fault, entry, total, code) of restart_paths_check"""
    keep, out = [], (C.c_int * 3)()
    rc = H.paths_check(slot_form, W, T, _p(off, np.int32, keep), _p(pts, np.float64, keep), out)
    return out[0], out[1], out[2], rc


# ---- sca_set_path_slots' rules ------------------------------------------------------------------------------------------------------------------
def test_valid_lists_and_no_lists_at_all(H):
    assert slots(H) == (S_OK, -1, 6, 0)
    assert slots(H, W=100) == (S_OK, -1, 6, 0)
    assert slots(H, off=None, pts=None) == (S_OK, -1, 0, 0)            # offsets NULL: every list empty
    assert slots(H, off=[0, 0, 0, 0, 0], pts=None) == (S_OK, -1, 0, 0) # ... as are four empty lists, whose points may be NULL
    assert slots(H, ctx_n=1, n=1, W=1, off=[0, 1], pts=[[1.0, 2.0, 3.0]]) == (S_OK, -1, 1, 0)


def test_the_refusals_of_set_paths_in_its_order(H):
    assert slots(H, agents_set=0, partition=1, n=9, W=0) == (S_NO_AGENTS, -1, 0, ERR_STATE)
    assert slots(H, partition=1, n=9, W=0) == (S_PARTITION, -1, 0, ERR_UNSUPPORTED)
    assert slots(H, n=3, W=0) == (S_BAD_N, -1, 0, ERR_ARG)
    assert slots(H, off=[1, 2, 2, 5, 6]) == (S_BAD_START, 0, 0, ERR_ARG)
    assert slots(H, off=[0, 2, 1, 5, 6]) == (S_DECREASING, 1, 0, ERR_ARG)
    assert slots(H, pts=None) == (S_NO_POINTS, -1, 6, ERR_ARG)
    for k, comp, bad in [(0, 0, np.nan), (3, 1, np.inf), (5, 2, -np.inf)]:
        pts = PTS.copy()
        pts[k, comp] = bad
        assert slots(H, pts=pts) == (S_NOT_FINITE, k, 6, ERR_ARG), (k, comp)
    two = PTS.copy()
    two[[4, 1], 0] = np.nan
    assert slots(H, pts=two) == (S_NOT_FINITE, 1, 6, ERR_ARG)          # the first bad point is named


def test_the_rooms_own_refusals(H):
    for W in (0, -1, -2 ** 31):
        assert slots(H, W=W) == (S_BAD_W, -1, 0, ERR_ARG), W
    assert slots(H, W=2) == (S_TOO_LONG, 2, 0, ERR_ARG)                # row 2 holds three
    assert slots(H, W=1) == (S_TOO_LONG, 0, 0, ERR_ARG)                # the first too long row is named
    assert slots(H, W=3)[0] == S_OK                                    # exactly W fits
    assert slots(H, W=2, off=[0, 2, 1, 5, 6]) == (S_DECREASING, 1, 0, ERR_ARG)     # row by row: row 1 decreases before row 2 is too long
    # W * max_agents points must stay addressable: every coordinate index below 2^31
    assert H.points_max() == (2 ** 31 - 1) // 3 == 715827882
    assert H.addressable(1, 715827882) == 1 and H.addressable(1, 715827883) == 0
    assert H.addressable(715827882, 1) == 1 and H.addressable(2, 357913941) == 1 and H.addressable(2, 357913942) == 0
    assert H.addressable(2 ** 31 - 1, 2 ** 31 - 1) == 0                # (the product is formed in 64 bits)
    assert slots(H, max_agents=357913941, W=2, off=None, pts=None)[0] == S_OK              # 2 x 357913941 points: the last that are; W = 3 there is refused, before the lists are read
    assert slots(H, max_agents=357913941, W=3, off=[1]) == (S_TOO_LARGE, -1, 0, ERR_ARG)


def test_the_row_to_place_index(H):
    assert [H.slot_index(5, a) for a in (0, 1, 2, 129)] == [0, 5, 10, 645]
    assert H.slot_index(1, 7) == 7
    assert H.slot_index(30, 2 ** 31 - 1) == 30 * (2 ** 31 - 1)         # 64 bits: no wrap at any row
    assert H.slot_index(2 ** 31 - 1, 2 ** 31 - 1) == (2 ** 31 - 1) ** 2


# ---- sca_restart_scenes_paths' rules -------------------------------------------------------------------------------------------------------------
def test_a_restart_with_and_without_lists(H):
    assert paths(H) == (P_OK, -1, 6, 0)
    assert paths(H, off=None, pts=None) == (P_OK, -1, 0, 0)            # no path arrays: exactly sca_restart_scenes_attrs
    assert paths(H, slot_form=0, W=0, off=None, pts=None) == (P_OK, -1, 0, 0)      # ... in any context
    assert paths(H, off=[0, 0, 0, 0, 0], pts=None) == (P_OK, -1, 0, 0)
    assert paths(H, T=1, W=1, off=[0, 1], pts=[[1.0, 2.0, 3.0]]) == (P_OK, -1, 1, 0)


def test_the_refusals_of_a_restart_with_lists(H):
    assert paths(H, slot_form=0, W=0) == (P_NO_SLOTS, -1, 0, ERR_STATE)
    assert paths(H, slot_form=0, W=0, off=[1, 0]) == (P_NO_SLOTS, -1, 0, ERR_STATE)     # before the arrays are read
    assert paths(H, off=[3, 3, 3, 5, 6]) == (P_BAD_START, 0, 0, ERR_ARG)
    assert paths(H, off=[0, 2, 2, 1, 6]) == (P_DECREASING, 2, 0, ERR_ARG)
    assert paths(H, off=[0, 2, 2, 6, 6]) == (P_TOO_LONG, 2, 0, ERR_ARG)                # row 2 brings four, W = 3
    assert paths(H, W=1) == (P_TOO_LONG, 0, 0, ERR_ARG)
    assert paths(H, W=2, off=[0, 2, 1, 5, 6]) == (P_DECREASING, 1, 0, ERR_ARG)
    assert paths(H, pts=None) == (P_NO_POINTS, -1, 6, ERR_ARG)
    # the message names the packed ROW whose list holds the point: points 0-1 are row 0's, 2-4 row 2's, 5 row 3's
    for k, row in [(0, 0), (1, 0), (2, 2), (4, 2), (5, 3)]:
        for comp, bad in [(0, np.nan), (1, np.inf), (2, -np.inf)]:
            pts = PTS.copy()
            pts[k, comp] = bad
            assert paths(H, pts=pts) == (P_NOT_FINITE, row, 6, ERR_ARG), (k, comp)
    two = PTS.copy()
    two[[5, 3], 1] = np.nan
    assert paths(H, pts=two) == (P_NOT_FINITE, 2, 6, ERR_ARG)


def test_block_form_keeps_its_refusal_and_slot_form_lifts_it(H):
    """what scene_restart_check is told for RestartCtx::paths_on"""
    assert [H.refuses(p, s) for p, s in [(0, 0), (1, 0), (1, 1), (0, 1)]] == [0, 1, 0, 0]


# ---- the block's sections ----------------------------------------------------------------------------------------------------------------------
def sections(H, max_n, max_m, W):
    begin, size, total = (C.c_int64 * 32)(), (C.c_int64 * 32)(), C.c_int64()
    k = H.block_sections(max_n, max_m, W, begin, size, C.byref(total))
    return list(begin[:k]), list(size[:k]), total.value


@pytest.mark.parametrize('max_n,max_m,W', [(1, 1, 1), (60, 1, 5), (130, 9, 30), (1536, 1491, 7), (4097, 3, 2)])
def test_sections_are_disjoint_aligned_and_inside_the_block(H, max_n, max_m, W):
    begin, size, total = sections(H, max_n, max_m, W)
    assert len(begin) == 13 + 1 + 6 + 4 + 2 and H.path_section_count() == 2
    for k in range(len(begin)):
        assert begin[k] % 64 == 0, k
        assert begin[k] + size[k] <= (begin[k + 1] if k + 1 < len(begin) else total), k
    assert size[-2:] == [4 * (max_n + 1), 24 * W * max_n]              # T + 1 offsets; at most W points per row, three doubles each
    assert total % 64 == 0
    # the sections in front are where they were: the block of a context that is not in slot form ends where the path sections begin
    b0, s0, t0 = sections(H, max_n, max_m, 0)
    assert b0[:-2] == begin[:-2] and s0[:-2] == size[:-2] and s0[-2:] == [0, 0] and t0 == begin[-2] == b0[-2] == b0[-1]


def test_the_path_sections_at_one_row_and_the_bits(H):
    """max_n = 1, W = 1: two offsets in one 64-byte unit, one point in another"""
    begin, size, total = sections(H, 1, 1, 1)
    attr_end = begin[-3] + 64                                          # RA_CLASS: one byte, one unit
    assert begin[-2:] == [attr_end, attr_end + 64] and size[-2:] == [8, 24] and total == attr_end + 128
    assert H.path_bits() == 256 | 512                                  # beside RESTART_HAS_ATTRS = 64 and _PLANNER = 128


# ---- the header ----------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_three_exports():
    text = open(os.path.join(ROOT, 'include', 'sca_hip.h')).read()
    flat = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    flat = re.sub(r'\s+', ' ', flat)
    assert 'int sca_set_path_slots(sca_ctx *ctx, int points_per_agent, int n, const int32_t *offsets , const double *points );' in flat
    assert 'int sca_get_path_slots(sca_ctx *ctx, int *points_per_agent);' in flat
    m = re.search(r'int sca_restart_scenes_paths\((.*?)\);', flat)
    assert m is not None
    args = [a.strip() for a in m.group(1).split(',')]
    assert args == ['sca_ctx *ctx', 'int count', 'const int32_t *scene_ids', 'const int32_t *sizes', 'const int32_t *obs_counts', 'const double *obs_pos',
                    'const double *obs_radius', 'const sca_restart_attrs *attrs', 'const int32_t *path_offsets', 'const double *path_points',
                    'const double *pos', 'const float *vel', 'const double *heading', 'const double *radius', 'const double *pref_speed',
                    'const double *goal', 'const uint8_t *policy', 'const uint8_t *zaxis', 'const double *max_run_dist', 'const double *goal_heading']


# ---- the shared body in slot form over the path corpus -------------------------------------------------------------------------------------------
PATH_STEPS = 6
PATH_CORPUS = {'plain': range(0, 40), 'per_agent': range(1000, 1020)}       # tests/test_form_fuzz_cpu.py's


def rooms_of(H, off, pts, W):
    """the lists in slot form: rooms [n * W, 3] (NaN where no list reaches: the body must never read there), len [n]"""
    n = len(off) - 1
    rooms = np.full((n * W, 3), np.nan)
    for a in range(n):
        at = H.slot_index(W, a)
        rooms[at:at + off[a + 1] - off[a]] = pts[off[a]:off[a + 1]]
    return rooms, np.diff(off).astype(np.int32)


def run_step(H, s, st, off, pts, W):
    """one pass from the state step `st` of the oracle run started from, through the harness: (rem, now_goal, vpref, mode) in block form (W
    None) or slot form"""
    n, keep = s['n'], []
    rem = np.array(st['path_left_before'], np.int32)
    ng = np.array(st['now_goal_before'], np.float64)
    vp, mode = np.zeros((n, 3)), np.zeros(n, np.uint8)
    vpp = lambda x: x.ctypes.data_as(C.c_void_p)
    rest = (vpp(rem), vpp(ng), _p(st['pos_before'], np.float64, keep), _p(s['radius'], np.float64, keep), _p(st['before'], np.uint8, keep),
            _p(s['policy'], np.uint8, keep), _p(s['goal'], np.float64, keep), _p(s['pref_speed'], np.float64, keep), vpp(vp), vpp(mode))
    if W is None:
        H.step_block(n, _p(off, np.int32, keep), _p(pts, np.float64, keep), *rest)
    else:
        rooms, ln = rooms_of(H, off, pts, W)
        H.step_slots(n, W, _p(rooms, np.float64, keep), _p(ln, np.int32, keep), *rest)
    return rem, ng, vp, mode


@pytest.mark.parametrize('corpus', list(PATH_CORPUS))
def test_the_slot_form_step_equals_the_rule_and_the_block_form(H, oracle, corpus):
    """every step of every corpus scene: remaining, now_goal and the aimed v_pref (as bytes: the sign of a zero counts) of the slot form, with
    W the longest list and W three more, against path_rule.pass_rule_csr (what the oracle run recorded) and against the block form"""
    aimed = pops = 0
    for seed in PATH_CORPUS[corpus]:
        s = F.random_scene(seed)
        lists = F.random_paths(seed, s)
        per = F.per_agent_attributes(seed, s['n']) if corpus == 'per_agent' else None
        run = F.oracle_run(oracle, s, PATH_STEPS, per, paths=lists)
        off, pts = R.csr(lists)
        longest = max(1, int(np.diff(off).max()))
        for t, st in enumerate(run):
            block = run_step(H, s, st, off, pts, None)
            for W in (longest, longest + 3):
                got = run_step(H, s, st, off, pts, W)
                ctx = (corpus, seed, t, W)
                for have, rule, blk, name in zip(got, (st['path_left'], st['now_goal'], st['vpref_rule'], st['path_mode']), block,
                                                 ('remaining', 'now_goal', 'vpref', 'mode')):
                    assert np.array_equal(have, rule, equal_nan=True) and np.array_equal(have, blk, equal_nan=True), ctx + (name,)
                assert got[2].tobytes() == st['vpref_rule'].tobytes() == block[2].tobytes(), ctx + ('the sign of a zero',)
            aimed += int(st['path_mode'].sum())
            pops += int((st['path_left_before'] - st['path_left']).sum())
    # (the corpus' own floors are tests/test_form_fuzz_cpu.py's; here only: the comparison was not empty)
    assert aimed > 1000 and pops > 1000, (aimed, pops)


# ---- the harness as a program of its own under the sanitizers ---------------------------------------------------------------------------------
def test_the_harness_alone_under_asan_and_ubsan(H):
    """tests/scene_paths_harness.cpp with its own main, -fsanitize=address,undefined, on buffers of exactly the size the rules may read: no
    report, and every line it prints is what the rules say (worked out by hand) or what the same calls answer here"""
    probe = subprocess.run(['gcc', '-print-file-name=libasan.so'], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip('libasan.so not found')
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, 'scene_paths_asan')
    subprocess.check_call(['g++', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-DSCENE_PATHS_MAIN'] + FLAGS + ['-o', exe, SRC])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1'))
    out = run.stdout[-4000:] + '\n' + run.stderr[-6000:]
    assert run.returncode == 0 and 'AddressSanitizer' not in out and 'runtime error' not in out, out
    lines = run.stdout.strip().split('\n')
    want = ['slots ok: rc 0 fault 0 entry -1 total 5',
            'slots too long: rc -1 fault 8 entry 2 total 0',           # W = 2, row 2 holds three
            'slots no lists: rc 0 fault 0 entry -1 total 0',
            'slots not finite: rc -1 fault 10 entry 4 total 5',        # the last point
            'paths not finite: rc -1 fault 6 entry 2 total 5',         # ... which is row 2's
            'paths ok: rc 0 fault 0 entry -1 total 5',
            'paths no slots: rc -3 fault 1 entry -1 total 0',
            'paths no points: rc -1 fault 5 entry -1 total 5']
    assert lines[:8] == want, lines[:8]
    for line, W in zip(lines[8:10], (0, 5)):
        begin, size, total = sections(H, 130, 9, W)
        assert line == 'layout %d:' % W + ''.join(' %d+%d' % bs for bs in zip(begin[-2:], size[-2:])) + ' total %d' % total
    # row 0 (RVO3D, two waypoints) takes its last and keeps it: 3.5 m away, nearer the goal than the agent; row 1 has no list; row 2 (SCA,
    # three waypoints, all farther from its goal than it is) pops twice in the first pass and once in the second, and its v_pref stays the tracker's
    assert lines[10:] == ['step W 3: same 1 rem 1 0 0 mode 1 0 0', 'step W 4: same 1 rem 1 0 0 mode 1 0 0'], lines[10:]
