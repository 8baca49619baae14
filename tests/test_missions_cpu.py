"""Mission tables (sca_set_missions) without a GPU: the pure rules of sca_amd/csrc/sca_missions.h, compiled for the host behind
tests/missions_harness.cpp -- every outcome of mission_check and of the getters' checks with its code, the layout of the three structs,
mission_take over all flag x successor combinations, the host-compiled row write (k_mission_advance's order of reads and writes around
respawn_write_row, the function k_respawn shares) against the Python rule of tests/mission_rule.py on the corpus, the collect's count /
offset / rank against numpy with rings that overflowed, plan_step's rows with missions_on, the harness as a program of its own under the
sanitizers, the symbols, and what the corpus holds (counted from the oracle and the rule alone)."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import form_fuzz as F
import harness_util
import mission_rule as MR

SRC = os.path.join(harness_util.ROOT, 'tests', 'missions_harness.cpp')
FLAGS = ['-std=c++17', '-ffp-contract=off', '-mfma', '-fno-builtin-pow', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I' + harness_util.CSRC]
(OK, NO_AGENTS, MID_STEP, OFF, BAD_M, BAD_R, BAD_N, NO_ARRAYS, TOO_LARGE, BAD_SUCCESSOR, NOT_FINITE, NOT_POSITIVE, BAD_ZAXIS, BAD_FLAGS, GET_ARGS,
 SCENES, SHARD, COMM, PARTITION, PATHS, STEP_HOST) = range(21)               # MissionFault
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5
CTX_KEYS = ('agents', 'mid_step', 'scenes', 'comm', 'partition', 'paths', 'n', 'shard_count')


@pytest.fixture(scope='module')
def H():
    out = os.path.join(harness_util.BUILD, 'libmissions_harness.so')
    deps = [SRC, os.path.join(harness_util.ROOT, 'include', 'sca_hip.h')] + \
        [os.path.join(harness_util.CSRC, f) for f in ('sca_missions.h', 'sca_respawn.h', 'sca_forms.h', 'sca_scenes.h', 'sca_core.h', 'sca_constants.h')]
    os.makedirs(harness_util.BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(['g++', '-O2', '-fPIC', '-shared'] + FLAGS + ['-o', out, SRC])
    h = C.CDLL(out)
    for name in ('msn_sizes', 'msn_check', 'msn_getter_checks', 'msn_take', 'msn_advance', 'msn_plan_step'):
        getattr(h, name).restype = None
    h.msn_check.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
    h.msn_getter_checks.argtypes = [C.c_int] * 11 + [C.c_void_p]
    h.msn_take.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    h.msn_advance.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11 + [C.c_int64]
    h.msn_collect.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4
    h.msn_plan_step.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    h.msn_trk_words.argtypes = [C.c_void_p]
    return h


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def sizes(H):
    out = np.zeros(16, np.int32)
    H.msn_sizes(vp(out))
    return out


def table(n=6, m=3, **over):
    """a legal table: every entry explicit, successors a cycle, every row flies into entry 0"""
    e = np.zeros((n, m), MR.MISSION)
    e['pos'], e['goal'] = 1.0, 2.0
    e['pref_speed'], e['max_run_dist'] = 1.0, 10.0
    e['next_ok'] = (np.arange(m) + 1) % m
    e['next_fail'] = -1
    t = dict(M=m, R=2, n=n, entries=e, first_ok=np.zeros(n, np.int32), first_fail=np.full(n, -1, np.int32))
    t.update(over)
    return t


def check(H, t, **state):
    s = dict(agents=1, mid_step=0, scenes=0, comm=0, partition=0, paths=0, n=6, shard_count=6)
    s.update(state)
    c = np.array([s[k] for k in CTX_KEYS], np.int32)
    out, top = np.zeros(3, np.int64), np.zeros(1)
    e = None if t['entries'] is None else np.ascontiguousarray(t['entries']).reshape(-1)
    reached = np.zeros(max(1, t['M'] * t['n']), np.uint8)
    H.msn_check(vp(c), t['M'], t['R'], t['n'], vp(e), vp(t['first_ok']), vp(t['first_fail']), vp(out), vp(top), vp(reached))
    return int(out[0]), int(out[1]), int(out[2]), float(top[0]), reached


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------
def test_every_outcome_of_mission_check(H):
    z = sizes(H)
    assert check(H, table())[:3] == (OK, -1, 0)
    assert check(H, table(), agents=0)[:3] == (NO_AGENTS, -1, ERR_STATE)
    assert check(H, table(), mid_step=1)[:3] == (MID_STEP, -1, ERR_STATE)
    for key, fault in (('scenes', SCENES), ('comm', COMM), ('partition', PARTITION), ('paths', PATHS)):
        assert check(H, table(), **{key: 1})[:3] == (fault, -1, ERR_UNSUPPORTED), key
    assert check(H, table(), shard_count=5)[:3] == (SHARD, -1, ERR_UNSUPPORTED)
    for m in (0, -1, int(z[9]) + 1):
        assert check(H, table(M=m))[:3] == (BAD_M, -1, ERR_ARG), m
    for r in (0, -3, int(z[10]) + 1):
        assert check(H, table(R=r))[:3] == (BAD_R, -1, ERR_ARG), r
    assert check(H, table(n=5))[:3] == (BAD_N, -1, ERR_ARG)
    for key in ('entries', 'first_ok', 'first_fail'):
        assert check(H, table(**{key: None}))[:3] == (NO_ARRAYS, -1, ERR_ARG), key
    big = int(z[11]) // 3 + 1                                               # M x n above the bound; refused before any array is read
    assert check(H, dict(M=3, R=1, n=big, entries=np.zeros(1, MR.MISSION), first_ok=np.zeros(1, np.int32), first_fail=np.zeros(1, np.int32)), n=big, shard_count=big)[:3] == \
        (TOO_LARGE, -1, ERR_ARG)
    big = int(z[11]) // 8 + 1                                               # ... and R x n
    assert check(H, dict(M=1, R=8, n=big, entries=np.zeros(1, MR.MISSION), first_ok=np.zeros(1, np.int32), first_fail=np.zeros(1, np.int32)), n=big, shard_count=big)[:3] == \
        (TOO_LARGE, -1, ERR_ARG)
    # successors: the first ones by row, the entries' by flat index -- reachable or not
    for key in ('first_ok', 'first_fail'):
        for bad in (3, -2):
            t = table()
            t[key] = t[key].copy()
            t[key][4] = bad
            assert check(H, t)[:3] == (BAD_SUCCESSOR, 4, ERR_ARG), (key, bad)
    for key in ('next_ok', 'next_fail'):
        t = table(first_ok=np.full(6, -1, np.int32))
        t['entries'][5, 2][key] = 3
        assert check(H, t)[:3] == (BAD_SUCCESSOR, 17, ERR_ARG), key
    # the values of REACHABLE entries only: rows 0 .. 4 reach 0 -> 1 -> 2, row 5 has no table
    first_ok = np.array([0, 0, 0, 0, 0, -1], np.int32)
    cases = [('pos', np.nan, NOT_FINITE), ('heading', np.inf, NOT_FINITE), ('goal', -np.inf, NOT_FINITE), ('goal_heading', np.nan, NOT_FINITE), ('vel', np.inf, NOT_FINITE),
             ('pref_speed', 0.0, NOT_POSITIVE), ('pref_speed', np.inf, NOT_POSITIVE), ('max_run_dist', -1.0, NOT_POSITIVE), ('max_run_dist', np.nan, NOT_POSITIVE),
             ('zaxis', 2, BAD_ZAXIS), ('flags', 4, BAD_FLAGS), ('flags', 128 | 1, BAD_FLAGS)]
    for key, bad, fault in cases:
        t = table(first_ok=first_ok)
        if t['entries'][key].ndim == 3:
            t['entries'][key][3, 1, 2] = bad
        else:
            t['entries'][key][3, 1] = bad
        assert check(H, t)[:3] == (fault, 10, ERR_ARG), (key, bad)
        t['entries'][key][5] = bad                                         # the same in a row without a table: not reachable, not looked at
        t['entries'][key][3, 1] = table()['entries'][key][3, 1]
        assert check(H, t)[0] == OK, (key, bad)
    # START_HERE: pos / heading are ignored; KEEP_ZAXIS: the byte is
    t = table()
    t['entries']['pos'][2, 0] = np.nan
    t['entries']['heading'][2, 0] = np.inf
    t['entries']['flags'][2, 0] = MR.START_HERE
    t['entries']['zaxis'][2, 1] = 200
    t['entries']['flags'][2, 1] = MR.KEEP_ZAXIS
    assert check(H, t)[0] == OK
    # an entry nobody reaches is not looked at, reachable or not is what `reached` says, the envelope is the reachable entries'
    t = table(m=4, first_ok=np.array([0, 1, -1, 3, 0, 2], np.int32), first_fail=np.array([-1, -1, -1, 3, 2, -1], np.int32))
    t['entries']['next_ok'] = np.array([1, 0, 2, -1], np.int8)             # 0 <-> 1, 2 -> 2, 3 stops
    t['entries']['pref_speed'] = np.arange(24).reshape(6, 4) + 1.0
    t['entries']['pref_speed'][2] = np.nan                                 # row 2 has no table
    t['entries']['pref_speed'][0, 2:] = -1.0                               # row 0 reaches 0 and 1 only
    fault, entry, code, top, reached = check(H, t)
    assert (fault, entry, code) == (OK, -1, 0)
    want = np.array([[1, 1, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1], [1, 1, 1, 0], [0, 0, 1, 0]], np.uint8)
    assert np.array_equal(reached.reshape(6, 4), want)
    assert top == t['entries']['pref_speed'][want.astype(bool)].max() == 23.0


def test_every_outcome_of_the_getters_checks(H):
    z = sizes(H)

    def g(agents=1, on=1, n=10, have_out=1, capacity=4, have_count=1, struct_bytes=int(z[1]), begin=0, count=10, have_cursor=1, have_ended=1):
        out = np.zeros(6, np.int32)
        H.msn_getter_checks(agents, on, n, have_out, capacity, have_count, struct_bytes, begin, count, have_cursor, have_ended, vp(out))
        return [tuple(out[2 * k:2 * k + 2]) for k in range(3)]
    assert g()[0] == (OK, 0) and g(struct_bytes=int(z[2]))[1] == (OK, 0) and g()[2] == (OK, 0)
    assert g(agents=0) == [(NO_AGENTS, ERR_STATE)] * 3
    assert g(on=0) == [(OFF, ERR_STATE)] * 3
    for kw in (dict(capacity=-1), dict(have_count=0), dict(have_out=0), dict(struct_bytes=95)):
        assert g(**kw)[0] == (GET_ARGS, ERR_ARG), kw
    assert g(have_out=0, capacity=0)[0] == (OK, 0)
    for kw in (dict(have_out=0, struct_bytes=int(z[2])), dict(struct_bytes=int(z[2]) - 8)):
        assert g(**kw)[1] == (GET_ARGS, ERR_ARG), kw
    for kw in (dict(begin=-1), dict(count=-1), dict(begin=11, count=0), dict(begin=4, count=7), dict(have_cursor=0), dict(have_ended=0)):
        assert g(**kw)[2] == (GET_ARGS, ERR_ARG), kw
    assert g(begin=10, count=0, have_cursor=0, have_ended=0)[2] == (OK, 0)


# ---- the layout --------------------------------------------------------------------------------------------------------------------------
def test_the_structs_and_the_symbols(H):
    from sca_amd import _lib
    z = sizes(H)
    assert z[0] == 128 == MR.MISSION.itemsize == _lib.MISSION_DTYPE.itemsize == C.sizeof(_lib.Mission)
    assert z[1] == 96 == MR.RESULT.itemsize == _lib.MISSION_RESULT_DTYPE.itemsize == C.sizeof(_lib.MissionResult)
    assert z[2] == 64 == C.sizeof(_lib.MissionTotals)
    assert MR.MISSION == _lib.MISSION_DTYPE and MR.RESULT == _lib.MISSION_RESULT_DTYPE and MR.CLEAR == _lib.CLEARANCE_DTYPE
    f = MR.MISSION.fields
    assert [f[k][1] for k in MR.MISSION.names] == [0, 24, 48, 72, 96, 104, 112, 124, 125, 126, 127]
    assert (z[3], z[4], z[5], z[6]) == (96, 112, 124, 127)
    r = MR.RESULT.fields
    assert [r[k][1] for k in MR.RESULT.names] == [0, 4, 8, 12, 16, 24, 48, 56, 60, 64] and (z[7], z[8]) == (48, 64)
    assert [getattr(_lib.Mission, k).offset for k in MR.MISSION.names] == [f[k][1] for k in MR.MISSION.names]
    assert [getattr(_lib.MissionResult, k).offset for k in MR.RESULT.names] == [r[k][1] for k in MR.RESULT.names]
    assert [k for k, _ in _lib.MissionTotals._fields_] == list(MR.TOTALS) + ['reserved']
    import sca_amd.solver as S
    assert (z[12], z[13]) == (MR.START_HERE, MR.KEEP_ZAXIS) == (S.MISSION_START_HERE, S.MISSION_KEEP_ZAXIS)
    assert z[15] == 256
    hdr = open(os.path.join(harness_util.ROOT, 'include', 'sca_hip.h')).read()
    assert re.search(r'SCA_MISSION_START_HERE\s*=\s*1\b', hdr) and re.search(r'SCA_MISSION_KEEP_ZAXIS\s*=\s*2\b', hdr)
    L = _lib.lib()
    for name in ('sca_set_missions', 'sca_get_mission_results', 'sca_get_mission_totals', 'sca_get_mission_state'):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert L.sca_version() == 103


# ---- taking ------------------------------------------------------------------------------------------------------------------------------
def test_mission_take_over_all_flag_and_successor_combinations(H):
    out = np.zeros(3, np.int32)
    for old, new, ok, fail in itertools.product(range(8), range(8), (-1, 0, 2), (-1, 1, 2)):
        H.msn_take(old, new, ok, fail, vp(out))
        assert out[0] == int(old == 0 and new != 0), (old, new)
        want = MR.outcome_of(new)
        assert out[1] == want and out[2] == (ok if want == MR.ARRIVED else fail), (old, new, ok, fail)
    # flag bits beyond the three done flags neither end a row nor keep it from ending
    H.msn_take(8, 8 | 4, 5, 6, vp(out))
    assert tuple(out) == (1, MR.TIMED_OUT, 6)
    H.msn_take(8, 8, 5, 6, vp(out))
    assert out[0] == 0


# ---- the host-compiled row write against the Python rule ----------------------------------------------------------------------------------
def run_harness(H, scene, run, R, tracker=False, clearance=False):
    """the run's steps through msn_advance: the state behind K4 in, the state behind the rule out, with the words the rule does not speak
    of (status, the list counters, vpref words, the tracker's) prefilled and held against respawn_row's values"""
    n, m = scene['n'], run['entries'].shape[1]
    e = np.ascontiguousarray(run['entries']).reshape(-1)
    cursor, flying, ended = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.uint32)
    ring, totals = np.zeros(n * R, MR.RESULT), np.zeros(8, np.uint64)
    policy = np.ascontiguousarray(scene['policy'], np.uint8)
    tracked = np.isin(policy, (0, 5)) & tracker
    init = np.zeros(8, np.uint32)
    words = H.msn_trk_words(vp(init))
    collected = []
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
        clear = None
        if clearance:
            clear = np.zeros(n, MR.CLEAR)
            clear['agent_clear'], clear['agent_partner'], clear['agent_step'] = np.arange(n) + 0.5, np.arange(n)[::-1], t + 1
        clear_in = None if clear is None else clear.copy()
        done = np.zeros(256 * 32, np.int32)
        before = np.ascontiguousarray(st['before'], np.uint8)
        arrays = [pos, vel, flags, radius, heading, goal, ps, mrd, td, sn, status, nbr_n, near_n, zaxis, mode, valid, ext, nbr0, tgh, clear, trk_st, done]
        S = (C.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])
        H.msn_advance(n, m, R, vp(policy), vp(e), vp(run['first_ok']), vp(run['first_fail']), vp(cursor), vp(flying), vp(ended), S, vp(before), vp(ring), vp(totals), t + 1)
        at = (scene['key'], 'step', t)
        for k, got in (('pos', pos), ('vel', vel), ('flags', flags), ('heading', heading), ('total_dist', td), ('step_num', sn)):
            assert np.array_equal(got, st[k]), at + (k,)
        for k, got in (('goal', goal), ('pref_speed', ps), ('max_run_dist', mrd), ('radius', radius)):
            assert np.array_equal(got, st['defs_after'][k]), at + (k,)
        assert np.array_equal(zaxis, st['zaxis']), at + ('zaxis',)
        assert np.array_equal(cursor, st['cursor']) and np.array_equal(flying, st['flying']) and np.array_equal(ended.astype(np.int32), st['ended']), at + ('cursors',)
        assert [int(x) for x in totals[:7]] == [st['totals'][k] for k in MR.TOTALS], at + ('totals', totals, st['totals'])
        tk = np.zeros(n, bool)
        tk[st['taken']] = True
        assert np.array_equal(status, np.where(tk, 0, 8)) and np.array_equal(nbr_n, np.where(tk, 0, 4)) and np.array_equal(near_n, np.where(tk, -1, 2)), at + ('scalar words',)
        assert np.array_equal(valid, np.where(tk, 0, 1)), at + ('nbr_valid',)
        assert np.array_equal(mode, np.where(tk & tracked, 1, 3)) and np.array_equal(ext, np.where((tk & tracked)[:, None], np.zeros((n, 3)), 7.0)), at + ('vpref words',)
        assert np.array_equal(done.reshape(256, 32)[:, 0], np.bincount(st['taken'] & 255, minlength=256)) and not done.reshape(256, 32)[:, 1:].any(), at + ('done_count',)
        if tracker:
            assert np.array_equal(nbr0, np.where(tk, -1.0, 2.0)), at + ('nbr0',)
            gh = run['entries']['goal_heading'][np.arange(n), np.maximum(st['cursor'], 0)]
            assert np.array_equal(tgh, np.where((tk & tracked)[:, None], gh, 9.0)), at + ('goal_heading',)
            assert np.array_equal(trk_st, np.where((tk & tracked)[:, None], np.broadcast_to(init[:words], (n, words)), 99)), at + ('AgentTrack',)
        want = st['results'].copy()
        if clearance:
            want['clear'] = clear_in[want['id']]
            assert np.array_equal(clear[tk], MR.empty_clear(int(tk.sum()))) and np.array_equal(clear[~tk], clear_in[~tk]), at + ('records emptied',)
        # the ring: this step's result of row a stands at (ended[a] - 1) % R
        got = ring[want['id'] * R + (st['ended'][want['id']] - 1) % R]
        assert got.tobytes() == want.tobytes(), at + ('results',)
        collected.append(want)
    return ring, ended, collected


def test_row_write_against_the_python_rule_on_the_corpus(H, oracle):
    for seed in MR.SEEDS:
        scene = F.random_scene(seed)
        run_harness(H, scene, MR.oracle_run(oracle, scene), R=1 + seed % 3)


def test_row_write_with_tracker_and_records(H, oracle):
    for seed in (3, 12, 27):
        scene = F.random_scene(seed)
        run_harness(H, scene, MR.oracle_run(oracle, scene), R=2, tracker=True, clearance=True)
        run_harness(H, scene, MR.oracle_run(oracle, scene), R=1, tracker=False, clearance=True)


# ---- the collect ---------------------------------------------------------------------------------------------------------------------------
def test_collect_count_offset_rank_against_numpy(H, oracle):
    """the compaction on the rings a run leaves (R = 1 and 2: rows that ended more often have lost results) and on drawn counters"""
    def collect(n, R, ended, collected, cap):
        tiles = (n + 255) // 256
        rows, slots, counts, offsets = np.full(max(cap, 1), -1, np.int32), np.full(max(cap, 1), -1, np.int32), np.zeros(tiles, np.int32), np.zeros(tiles, np.int32)
        total = H.msn_collect(n, R, vp(ended), vp(collected), cap, vp(rows), vp(slots), vp(counts), vp(offsets))
        return total, rows, slots, counts, offsets

    def want_of(n, R, ended, collected):
        fresh = np.minimum(ended - collected, R).astype(np.int64)
        rows = np.repeat(np.arange(n), fresh)
        k = np.arange(len(rows)) - np.repeat(np.cumsum(fresh) - fresh, fresh)
        return fresh, rows, (np.repeat(ended.astype(np.int64), fresh) - np.repeat(fresh, fresh) + k) % R
    rng = np.random.default_rng(77)
    cases = []
    for seed in (5, 17, 33, 39):
        scene = F.random_scene(seed)
        run = MR.oracle_run(oracle, scene)
        for R in (1, 2):
            cases.append((scene['n'], R, run['steps'][-1]['ended'].astype(np.uint32), run))
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        cases.append((n, 3, rng.integers(0, 7, n).astype(np.uint32), None))
    for n, R, ended, run in cases:
        collected = np.zeros(n, np.uint32)
        fresh, rows, slots = want_of(n, R, ended, collected)
        assert run is None or R > 1 or (ended > R).any()                   # (rings that overflowed)
        total, grow, gslot, counts, offsets = collect(n, R, ended, collected.copy(), max(0, int(fresh.sum()) - 1))
        assert total == fresh.sum() and (grow == -1).all() or fresh.sum() == 0   # no room: nothing written
        c2 = collected.copy()
        total, grow, gslot, counts, offsets = collect(n, R, ended, c2, int(fresh.sum()))
        assert total == fresh.sum()
        assert np.array_equal(counts, np.add.reduceat(np.concatenate([fresh, np.zeros(-n % 256, np.int64)]), np.arange(0, n, 256)))
        assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(counts)[:-1]]))
        assert np.array_equal(grow[:total], rows) and np.array_equal(gslot[:total], slots)
        assert np.array_equal(c2, ended)                                   # marked collected
        assert collect(n, R, ended, c2, 0)[0] == 0
        if run is not None:                                                # the slots hold the rows' LAST min(ended, R) results, oldest first
            per_row = {}
            for st in run['steps']:
                for r in st['results']:
                    per_row.setdefault(int(r['id']), []).append(int(r['update']))
            ring_update = np.zeros((n, R), np.int64)
            for a, ups in per_row.items():
                for k, up in enumerate(ups):
                    ring_update[a, k % R] = up
            got = ring_update[grow[:total], gslot[:total]]
            want = np.concatenate([np.array(per_row[a][-min(len(per_row[a]), R):], np.int64) for a in sorted(per_row)]) if per_row else np.zeros(0, np.int64)
            assert np.array_equal(got, want)


# ---- plan_step -----------------------------------------------------------------------------------------------------------------------------
def test_plan_step_rows_with_missions_on(H):
    """with tables set a step plans no build ahead, no event on k_action and no fork riding on its last kernel; without them, and for a
    caller whose aggregate initialiser predates the field, every row is what it was"""
    AUTO, KD = 3, 0
    keys = ('mode', 'step', 'steps', 'kd_stream', 'ext_stop', 'comm', 'whole', 'trk_on', 'trk_in_pass', 'trk_fork', 'paths_on', 'clear_on', 'auto_ran',
            'fits', 'part_on', 'kdq_last', 'auto_div', 'auto_backoff', 'shard_count')
    seen = set()
    for mode, step, kd_stream, ext_stop, whole, trk, paths_on, clear_on, auto_ran, fits in itertools.product((AUTO, KD), (0, 2), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
        v = dict(mode=mode, step=step, steps=3, kd_stream=kd_stream, ext_stop=ext_stop, comm=0, whole=whole, trk_on=trk, trk_in_pass=trk, trk_fork=trk, paths_on=paths_on,
                 clear_on=clear_on, auto_ran=auto_ran and mode == AUTO, fits=fits, part_on=0, kdq_last=0, auto_div=8, auto_backoff=0, shard_count=4096)
        i = np.array([int(v[k]) for k in keys], np.int32)
        old, off, on = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(3, np.int32)
        H.msn_plan_step(vp(i), 0, 0, vp(old))
        H.msn_plan_step(vp(i), 0, 1, vp(off))
        H.msn_plan_step(vp(i), 1, 1, vp(on))
        assert np.array_equal(old, off) and not on.any(), v
        seen.add(tuple(old))
    assert {(1, 0, 0), (0, 0, 1), (0, 0, 0)} <= seen and any(s[1] for s in seen)   # every event occurs in the rows without tables


# ---- the harness as a program under the sanitizers ---------------------------------------------------------------------------------------
def test_standalone_under_sanitizers():
    """The rules as a program of their own (its main draws tables into heap arrays of exactly M n entries, steps rows into endings, applies
    k_mission_advance's host twin to heap arrays of exactly n rows and R n results, then collects) under -fsanitize=address,undefined.
    Host code only; nothing of it is loaded into python."""
    exe = os.path.join(harness_util.BUILD, 'missions_harness_san')
    os.makedirs(harness_util.BUILD, exist_ok=True)
    subprocess.check_call(['g++', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan',
                           '-DMISSIONS_MAIN'] + FLAGS + ['-o', exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'missions_harness: ok' in r.stdout


# ---- what the corpus holds -----------------------------------------------------------------------------------------------------------------
CORPUS = dict(take_arrived=84, take_collided=33620, take_timed_out=367, stops=3026, retries=18584, retries_ending_next_step=16515, start_here=17876,
              explicit_start=16195, tracked_taken=10918, lp_taken=5795, group_doubles=1713, ring_overflow_r1=4631)


def test_what_the_corpus_holds(oracle):
    """counted from the oracle's records and the Python rule alone (README: the mission tables' section records the same numbers)"""
    total = dict.fromkeys(MR.CLASSES, 0)
    for seed in MR.SEEDS:
        scene = F.random_scene(seed)
        c = MR.corpus_counts(scene, MR.oracle_run(oracle, scene))
        for k in total:
            total[k] += c[k]
    assert all(v > 0 for v in total.values()), total
    assert total == CORPUS, total
