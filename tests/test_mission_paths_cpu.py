"""Mission tables whose entries bring their own waypoint lists (sca_set_missions_paths) without a GPU: mission_paths_check of
sca_amd/csrc/sca_missions.h compiled for the host behind tests/mission_paths_harness.cpp -- every outcome with its code and index --, the
bits byte and the `has` word of a take, the host-compiled take (the shared row write plus the shared list write, mission_take_write)
against the Python rule of tests/mission_paths_rule.py on the corpus, ungated and behind the gate, the harness as a program of its own
under the sanitizers with the rooms at exactly 24 W n bytes, the symbols, and what the corpus holds (counted from the oracle and the rule
alone)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import form_fuzz as F
import harness_util
import mission_paths_rule as PR
import mission_rule as MR
import path_rule as R

SRC = os.path.join(harness_util.ROOT, 'tests', 'mission_paths_harness.cpp')
FLAGS = ['-std=c++17', '-ffp-contract=off', '-mfma', '-fno-builtin-pow', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I' + harness_util.CSRC]
OK, NO_AGENTS, MID_STEP, BAD_M, NO_ARRAYS, BAD_SUCCESSOR, NOT_FINITE, SCENES, SHARD, COMM, PARTITION, PATHS, STEP_HOST = 0, 1, 2, 4, 7, 9, 10, 15, 16, 17, 18, 19, 20
NO_SLOTS, START, DECREASING, NO_POINTS, TOTAL, TOO_LONG, PATH_NOT_FINITE, CLEAR = range(21, 29)      # MissionFault, behind the older values
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5
CTX_KEYS = ('agents', 'mid_step', 'scenes', 'comm', 'partition', 'paths', 'n', 'shard_count', 'path_W')


@pytest.fixture(scope='module')
def H():
    out = os.path.join(harness_util.BUILD, 'libmission_paths_harness.so')
    deps = [SRC, os.path.join(harness_util.ROOT, 'include', 'sca_hip.h')] + \
        [os.path.join(harness_util.CSRC, f) for f in ('sca_missions.h', 'sca_respawn.h', 'sca_spawn.h', 'sca_scenes.h', 'sca_core.h', 'sca_constants.h')]
    os.makedirs(harness_util.BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(['g++', '-O2', '-fPIC', '-shared'] + FLAGS + ['-o', out, SRC])
    h = C.CDLL(out)
    for name in ('mpt_check', 'mpt_get_check', 'mpt_consts', 'mpt_bits', 'mpt_take'):
        getattr(h, name).restype = None
    h.mpt_check.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8
    h.mpt_get_check.argtypes = [C.c_int] * 3 + [C.c_void_p]
    h.mpt_consts.argtypes = [C.c_void_p]
    h.mpt_bits.argtypes = [C.c_int] * 4 + [C.c_void_p]
    h.mpt_take.argtypes = [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3
    h.mpt_trk_words.argtypes = [C.c_void_p]
    return h


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def table(n=6, m=3, lens=None, **over):
    """test_missions_cpu's legal table (every entry explicit, successors a cycle, every row flies into entry 0) with a list of lens[a][j]
    points per entry (default: (a + j) % 3)"""
    e = np.zeros((n, m), MR.MISSION)
    e['pos'], e['goal'] = 1.0, 2.0
    e['pref_speed'], e['max_run_dist'] = 1.0, 10.0
    e['next_ok'] = (np.arange(m) + 1) % m
    e['next_fail'] = -1
    lens = (np.arange(n)[:, None] + np.arange(m)[None, :]) % 3 if lens is None else np.asarray(lens)
    off = np.zeros(n * m + 1, np.int32)
    off[1:] = np.cumsum(lens.reshape(-1))
    t = dict(M=m, R=2, n=n, entries=e, first_ok=np.zeros(n, np.int32), first_fail=np.full(n, -1, np.int32), off=off, pts=np.arange(3.0 * off[-1]).reshape(-1, 3) + 0.5)
    t.update(over)
    return t


def check(H, t, **state):
    s = dict(agents=1, mid_step=0, scenes=0, comm=0, partition=0, paths=1, n=6, shard_count=6, path_W=2)
    s.update(state)
    c = np.array([s[k] for k in CTX_KEYS], np.int32)
    out, top = np.zeros(4, np.int64), np.zeros(1)
    e = None if t['entries'] is None else np.ascontiguousarray(t['entries']).reshape(-1)
    reached = np.zeros(max(1, t['M'] * t['n']), np.uint8)
    H.mpt_check(vp(c), t['M'], t['R'], t['n'], vp(e), vp(t['first_ok']), vp(t['first_fail']), vp(t['off']), vp(t['pts']), vp(out), vp(top), vp(reached))
    return tuple(int(x) for x in out)


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------
def test_every_outcome_of_mission_paths_check(H):
    z = np.zeros(16, np.int64)
    H.mpt_consts(vp(z))
    assert tuple(z[:9]) == (STEP_HOST, NO_SLOTS, START, DECREASING, NO_POINTS, TOTAL, TOO_LONG, PATH_NOT_FINITE, CLEAR) and z[9] == 2 ** 31 // 3 and z[10] == ERR_UNSUPPORTED
    total = int(table()['off'][-1])
    assert check(H, table()) == (OK, -1, 0, total)
    # everything sca_set_missions refuses, with its codes -- the context first, lists in SLOT form being no fault here
    assert check(H, table(), agents=0)[:3] == (NO_AGENTS, -1, ERR_STATE)
    assert check(H, table(), mid_step=1)[:3] == (MID_STEP, -1, ERR_STATE)
    for key, fault in (('scenes', SCENES), ('comm', COMM), ('partition', PARTITION)):
        assert check(H, table(), **{key: 1})[:3] == (fault, -1, ERR_UNSUPPORTED), key
    assert check(H, table(), shard_count=5)[:3] == (SHARD, -1, ERR_UNSUPPORTED)
    assert check(H, table(), path_W=0)[:3] == (PATHS, -1, ERR_UNSUPPORTED)                 # lists in block form
    assert check(H, table(M=0))[:3] == (BAD_M, -1, ERR_ARG)
    assert check(H, table(entries=None))[:3] == (NO_ARRAYS, -1, ERR_ARG)
    t = table()
    t['entries']['next_ok'][5, 2] = 3
    assert check(H, t)[:3] == (BAD_SUCCESSOR, 17, ERR_ARG)
    t = table()
    t['entries']['goal'][3, 1, 2] = np.nan
    assert check(H, t)[:3] == (NOT_FINITE, 10, ERR_ARG)
    # no slot form: with offsets SCA_ERR_STATE -- behind the context's faults, in front of the arguments' --, without them sca_set_missions
    assert check(H, table(), paths=0, path_W=0)[:3] == (NO_SLOTS, -1, ERR_STATE)
    assert check(H, table(M=0), paths=0, path_W=0)[:3] == (NO_SLOTS, -1, ERR_STATE)
    assert check(H, table(), paths=0, path_W=0, scenes=1)[:3] == (SCENES, -1, ERR_UNSUPPORTED)
    assert check(H, table(off=None, pts=None), paths=0, path_W=0) == (OK, -1, 0, 0)
    assert check(H, table(off=None, pts=None, M=0), paths=0, path_W=0)[:3] == (BAD_M, -1, ERR_ARG)
    # slot form without offsets: every entry brings the empty list
    assert check(H, table(off=None, pts=None)) == (OK, -1, 0, 0)
    assert check(H, table(off=None, pts=np.zeros((1, 3)))) == (OK, -1, 0, 0)
    # the offsets of EVERY entry
    t = table()
    t['off'] = t['off'] + 1
    assert check(H, t)[:3] == (START, -1, ERR_ARG)
    t = table(first_ok=np.full(6, -1, np.int32))                            # (nobody reachable: the offsets are inspected all the same)
    t['off'] = t['off'].copy()
    t['off'][12] = t['off'][11] - 1
    assert check(H, t)[:3] == (DECREASING, 11, ERR_ARG)
    assert check(H, table(pts=None))[:3] == (NO_POINTS, -1, ERR_ARG)
    assert check(H, table(lens=np.zeros((6, 3), int), pts=None)) == (OK, -1, 0, 0)   # nothing to read: no points needed
    big = table(n=1, m=1, lens=[[0]])
    big['off'] = np.array([0, 2 ** 31 // 3 + 1], np.int32)
    assert check(H, big, n=1, shard_count=1, path_W=2 ** 30)[:3] == (TOTAL, -1, ERR_ARG)   # refused before a point is read
    big['off'] = np.array([0, 2 ** 31 // 3], np.int32)
    big['first_ok'] = np.full(1, -1, np.int32)                               # (unreachable: its points are never read)
    assert check(H, big, n=1, shard_count=1, path_W=1) == (OK, -1, 0, 2 ** 31 // 3)
    # the lengths and the points of REACHABLE entries only: rows 0 .. 4 reach 0 -> 1 -> 2, row 5 has no table; lowest flat index first
    first_ok = np.array([0, 0, 0, 0, 0, -1], np.int32)
    lens = np.ones((6, 3), int)
    lens[3, 1] = lens[4, 0] = lens[5, 2] = 3
    assert check(H, table(lens=lens, first_ok=first_ok))[:3] == (TOO_LONG, 10, ERR_ARG)
    assert check(H, table(lens=lens, first_ok=first_ok), path_W=3)[0] == OK
    lens[3, 1] = lens[4, 0] = 2                                               # exactly W fits; the long list of row 5 is not looked at
    assert check(H, table(lens=lens, first_ok=first_ok))[0] == OK
    for bad in (np.nan, np.inf, -np.inf):
        t = table(first_ok=first_ok)
        t['pts'][t['off'][10], 1] = bad                                       # entry (3, 1) holds ((3 + 1) % 3) = 1 point
        assert check(H, t)[:3] == (PATH_NOT_FINITE, 10, ERR_ARG), bad
        t['pts'][t['off'][13], 2] = bad                                       # ... and (4, 1) too: the lower index is reported
        assert check(H, t)[:3] == (PATH_NOT_FINITE, 10, ERR_ARG), bad
        t = table(first_ok=first_ok)
        t['pts'][t['off'][15]:t['off'][18]] = bad                             # row 5: not reachable, not looked at
        assert check(H, t)[0] == OK, bad
    # a value fault of an entry is reported in front of a list fault of a lower entry (mission_check's faults come first)
    t = table(lens=lens, first_ok=first_ok)
    t['entries']['pref_speed'][4, 2] = 0.0
    assert check(H, t, path_W=1)[:2] == (11, 14)                              # MSF_NOT_POSITIVE at (4, 2)
    out = np.zeros(2, np.int32)
    for args, want in (((1, 1, 1), (OK, 0)), ((0, 1, 1), (NO_AGENTS, ERR_STATE)), ((1, 0, 1), (3, ERR_STATE)), ((1, 1, 0), (14, ERR_ARG))):
        H.mpt_get_check(*args, vp(out))
        assert tuple(out) == want, args


def test_the_bits_and_the_has_word_of_a_take(H):
    z = np.zeros(16, np.int64)
    H.mpt_consts(vp(z))
    slots_paths, reset, tracked_bit = int(z[11]), int(z[12]), int(z[13])
    out = np.zeros(3, np.int32)
    for policy in range(6):
        for tracker in (0, 1):
            for old_len in (0, 1, 3):
                for flags in (0, MR.START_HERE, MR.KEEP_ZAXIS, 3):
                    H.mpt_bits(policy, tracker, old_len, flags, vp(out))
                    straight = policy not in R.TRACKED
                    assert out[0] == (tracked_bit if tracker and not straight else 0) | (reset if straight and old_len > 0 else 0), (policy, tracker, old_len)
                    zaxis = 0 if flags & MR.KEEP_ZAXIS else 1
                    assert out[1] == zaxis | slots_paths and out[2] == zaxis, flags


def test_the_symbols():
    from sca_amd import _lib
    L = _lib.lib()
    for name in ('sca_set_missions_paths', 'sca_get_mission_paths', 'sca_get_path_slot_lists', 'sca_get_vpref_mode'):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert L.sca_version() == 103 and C.sizeof(_lib.Mission) == 128
    hdr = open(os.path.join(harness_util.ROOT, 'include', 'sca_hip.h')).read()
    assert 'int sca_set_missions_paths(sca_ctx *ctx, int M, int R, int n, const sca_mission *entries' in hdr and 'int sca_get_mission_paths(sca_ctx *ctx' in hdr


# ---- the host-compiled take against the Python rule ----------------------------------------------------------------------------------------
def run_harness(H, scene, run, tracker=False, lists=True):
    """the run's takes through mpt_take: the state behind K4 in, the state behind the rule out; the rooms, lengths, cursors and now_goal are
    carried from step to step as the context carries them (between the steps path_rule's pass moves the cursors)"""
    n, m, w = scene['n'], run['entries'].shape[1], run['w']
    e = np.ascontiguousarray(run['entries']).reshape(-1)
    off, pts = R.csr(PR.flat_lists(run['lists']))
    pts = np.ascontiguousarray(pts)
    policy = np.ascontiguousarray(scene['policy'], np.uint8)
    tracked = np.isin(policy, R.TRACKED) & tracker
    init = np.zeros(8, np.uint32)
    words = H.mpt_trk_words(vp(init))
    rooms = np.full((n, w, 3), -7.0)
    for a, lst in enumerate(run['initial']):
        rooms[a, :len(lst)] = np.asarray(lst).reshape(-1, 3)
    plen = np.array([len(p) for p in run['initial']], np.int32)
    for t, st in enumerate(run['steps']):
        u = st['ended_state']
        pos, vel, flags = u['pos'].copy(), np.ascontiguousarray(u['vel'], np.float32).copy(), np.ascontiguousarray(u['flags'], np.uint8).copy()
        radius, heading = st['defs']['radius'].copy(), u['heading'].copy()
        goal, ps, mrd = st['defs']['goal'].copy(), st['defs']['pref_speed'].copy(), st['defs']['max_run_dist'].copy()
        td, sn = u['total_dist'].copy(), np.ascontiguousarray(u['step_num'], np.int32).copy()
        status, nbr_n, near_n = np.full(n, 8, np.int32), np.full(n, 4, np.int32), np.full(n, 2, np.int32)
        zaxis, mode, valid = st['zaxis_before'].copy(), np.full(n, 3, np.uint8), np.ones(n, np.uint8)
        ext = np.full((n, 3), 7.0)
        nbr0, tgh, trk_st = (np.full(n, 2.0), np.full((n, 3), 9.0), np.full((n, words), 99, np.uint32)) if tracker else (None, None, None)
        if not lists and t > 0:                                             # (the harness moved no path word: the rule's lists of the last step)
            plen = st['old_len'].copy()
            for a_, lst in enumerate(run['steps'][t - 1]['rooms_after']):
                rooms[a_, :len(lst)] = np.asarray(lst, np.float64).reshape(-1, 3)
        assert np.array_equal(plen, st['old_len'])
        prem, ng = st['path_left'].copy(), st['now_goal'].copy()            # behind the pass
        rooms_in, plen_in = rooms.copy(), plen.copy()
        done = np.zeros(256 * 32, np.int32)
        ids, nxt = np.ascontiguousarray(st['taken'], np.int32), np.ascontiguousarray(st['taken_entry'], np.int32)
        arrays = [pos, vel, flags, radius, heading, goal, ps, mrd, td, sn, status, nbr_n, near_n, zaxis, mode, valid, ext, rooms, plen, prem, ng, nbr0, tgh, trk_st, done]
        S = (C.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])
        H.mpt_take(n, m, w, int(lists), vp(policy), vp(e), vp(off), vp(pts), len(ids), vp(ids), vp(nxt), S)
        at = (scene['key'], 'step', t)
        for k, got in (('pos', pos), ('vel', vel), ('flags', flags), ('heading', heading), ('total_dist', td), ('step_num', sn)):
            assert np.array_equal(got, st[k]), at + (k,)
        for k, got in (('goal', goal), ('pref_speed', ps), ('max_run_dist', mrd), ('radius', radius)):
            assert np.array_equal(got, st['defs_after'][k]), at + (k,)
        assert np.array_equal(zaxis, st['zaxis']), at + ('zaxis',)
        tk = np.zeros(n, bool)
        tk[st['taken']] = True
        assert np.array_equal(status, np.where(tk, 0, 8)) and np.array_equal(nbr_n, np.where(tk, 0, 4)) and np.array_equal(near_n, np.where(tk, -1, 2)), at + ('scalar words',)
        assert np.array_equal(done.reshape(256, 32)[:, 0], np.bincount(st['taken'] & 255, minlength=256)) and not done.reshape(256, 32)[:, 1:].any(), at + ('done_count',)
        if not lists:                                                       # tables without lists: no path word moves, no mode is reset
            assert np.array_equal(rooms, rooms_in) and np.array_equal(plen, plen_in) and np.array_equal(prem, st['path_left']), at
            assert np.array_equal(ng, st['now_goal'], equal_nan=True) and np.array_equal(mode, np.where(tk & tracked, 1, 3)), at
            continue
        reset = np.zeros(n, bool)
        reset[st['mode_reset']] = True
        assert np.array_equal(mode, np.where(tk & tracked, 1, np.where(reset, 0, 3))), at + ('vpref_mode',)
        assert np.array_equal(ext, np.where((tk & tracked)[:, None], np.zeros((n, 3)), 7.0)), at + ('vpref_ext',)
        assert np.array_equal(plen, st['path_len_after']) and np.array_equal(prem, st['path_left_after']), at + ('len / rem',)
        assert np.array_equal(ng, st['now_goal_after'], equal_nan=True), at + ('now_goal',)
        assert np.array_equal(rooms[~tk], rooms_in[~tk]), at + ('rooms of the other rows',)
        for a in st['taken']:
            lst = st['rooms_after'][a]
            assert np.array_equal(rooms[a, :len(lst)], np.asarray(lst, np.float64).reshape(-1, 3)), at + ('room', a)
            assert np.array_equal(rooms[a, len(lst):], rooms_in[a, len(lst):]), at + ('room behind the list', a)
        if tracker:
            gh = run['entries']['goal_heading'][np.arange(n), np.maximum(st['cursor'], 0)]
            assert np.array_equal(tgh, np.where((tk & tracked)[:, None], gh, 9.0)), at + ('goal_heading',)
            assert np.array_equal(trk_st, np.where((tk & tracked)[:, None], np.broadcast_to(init[:words], (n, words)), 99)), at + ('AgentTrack',)


def test_take_against_the_python_rule_on_the_corpus(H, oracle):
    for seed in PR.SEEDS:
        scene = F.random_scene(seed)
        run_harness(H, scene, PR.oracle_run(oracle, scene))


def test_take_with_the_tracker_behind_the_gate_and_without_lists(H, oracle):
    for seed in (3, 12, 27):
        scene = F.random_scene(seed)
        run_harness(H, scene, PR.oracle_run(oracle, scene), tracker=True)
        run_harness(H, scene, PR.oracle_run(oracle, scene, gate=(PR.GATE_MARGIN, 0)))
        run_harness(H, scene, PR.oracle_run(oracle, scene, gate=(PR.GATE_MARGIN, 8)), tracker=True)
        run_harness(H, scene, PR.oracle_run(oracle, scene), tracker=True, lists=False)


# ---- the harness as a program under the sanitizers ---------------------------------------------------------------------------------------
def test_standalone_under_sanitizers():
    """The check and the take as a program of their own (its main draws tables and packed lists into heap arrays of exactly M n entries,
    M n + 1 offsets and the lists' points, rooms of exactly 24 W n bytes, lets rows take reachable entries and holds the rooms against the
    lists) under -fsanitize=address,undefined.  Host code only; nothing of it is loaded into python."""
    exe = os.path.join(harness_util.BUILD, 'mission_paths_harness_san')
    os.makedirs(harness_util.BUILD, exist_ok=True)
    subprocess.check_call(['g++', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan',
                           '-DMISSION_PATHS_MAIN'] + FLAGS + ['-o', exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'mission_paths_harness: ok' in r.stdout


# ---- what the corpus holds -----------------------------------------------------------------------------------------------------------------
CORPUS = dict(takes_with_list=22642, takes_empty_onto_list_untracked=2378, takes_empty_onto_list_tracked=1128, takes_full_room=7916, pops_right_after_take=20959,
              pops_later_after_take=125, orca_taken=11191, tracked_taken_with_list=7102, rows_taken_twice_different_lists=2101)
GATED = dict(gate_admitted=290, gate_waiting_rows_list_unmoved=29580)


def test_what_the_corpus_holds(oracle):
    """counted from the oracle's records and the Python rule alone; every class must be non-empty"""
    total = dict.fromkeys(PR.CLASSES, 0)
    for seed in PR.SEEDS:
        scene = F.random_scene(seed)
        c = PR.corpus_counts(scene, PR.oracle_run(oracle, scene))
        for k in total:
            total[k] += c[k]
    assert all(v > 0 for v in total.values()), total
    assert total == CORPUS, total


def test_what_the_gated_corpus_holds(oracle):
    """under the gate at margin 0.5 (the default cap, and a cap of 8): admitted rows, and waiting rows whose list does not move"""
    total = dict.fromkeys(PR.GATE_CLASSES, 0)
    for seed in PR.SEEDS[:10]:
        scene = F.random_scene(seed)
        for cap in (0, 8):
            c = PR.gate_counts(scene, PR.oracle_run(oracle, scene, gate=(PR.GATE_MARGIN, cap)))
            for k in total:
                total[k] += c[k]
    assert all(v > 0 for v in total.values()), total
    assert total == GATED, total
