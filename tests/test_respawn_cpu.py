"""Respawning agents in place (sca_respawn_agents, sca_get_finished) without a GPU: the pure rules of sca_amd/csrc/sca_respawn.h, compiled
for the host behind tests/respawn_harness.cpp -- every outcome of respawn_check with its code, respawn_layout, respawn_row (the function
k_respawn calls per row) against the Python rule of tests/respawn_rule.py on the corpus, finished_offsets against np.flatnonzero -- the
harness as a program of its own under the sanitizers, the symbols, and what the corpus holds (counted from the oracle and the rule alone)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import form_fuzz as F
import harness_util
import respawn_rule as RR

SRC = os.path.join(harness_util.ROOT, 'tests', 'respawn_harness.cpp')
FLAGS = ['-std=c++17', '-ffp-contract=off', '-mfma', '-fno-builtin-pow', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I' + harness_util.CSRC]
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5                   # include/sca_hip.h
(OK, NO_AGENTS, NO_STATE, MID_STEP, BAD_COUNT, NO_ARRAYS, BAD_ID, REPEATED_ID, NOT_FINITE, NOT_POSITIVE, GOAL_HEADING, PATH_HALF, PATH_OFFSETS,
 PATH_TOO_LONG, PATH_NOT_FINITE, FIN_ARGS, SCENES, SHARD, COMM, PARTITION, PATH_BLOCK, PATH_NO_SLOTS) = range(22)        # RespawnFault
CTX_KEYS = ('agents', 'state', 'mid_step', 'scenes', 'comm', 'partition', 'n', 'shard_count', 'tracker_on', 'paths_block', 'path_W')


@pytest.fixture(scope='module')
def H():
    out = os.path.join(harness_util.BUILD, 'librespawn_harness.so')
    deps = [SRC, os.path.join(harness_util.ROOT, 'include', 'sca_hip.h')] + \
        [os.path.join(harness_util.CSRC, f) for f in ('sca_respawn.h', 'sca_scenes.h', 'sca_core.h', 'sca_glibc_math.h', 'sca_glibc_tables.h', 'sca_constants.h')]
    os.makedirs(harness_util.BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(['g++', '-O2', '-fPIC', '-shared'] + FLAGS + ['-o', out, SRC])
    h = C.CDLL(out)
    h.rsp_check.restype = None
    h.rsp_check.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 13
    h.rsp_finished_check.restype = None
    h.rsp_layout.restype = None
    h.rsp_layout.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    h.rsp_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 36
    h.rsp_finished.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return h


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def ctx_of(**state):
    s = dict(agents=1, state=1, mid_step=0, scenes=0, comm=0, partition=0, n=10, shard_count=10, tracker_on=0, paths_block=0, path_W=0)
    s.update(state)
    return np.array([s[k] for k in CTX_KEYS], np.int32)


def mission(k=4, **over):
    m = dict(ids=np.arange(k, dtype=np.int32), pos=np.ones((k, 3)), vel=np.zeros((k, 3), np.float32), heading=np.zeros((k, 3)), radius=np.full(k, 0.5),
             pref_speed=np.ones(k), goal=np.full((k, 3), 4.0), zaxis=None, max_run_dist=np.full(k, 9.0), goal_heading=None, path_offsets=None,
             path_points=None, count=k)
    m.update(over)
    return m


def check(H, m, policy=None, **state):
    c = ctx_of(**state)
    policy = np.full(int(c[6]), 3, np.uint8) if policy is None else np.ascontiguousarray(policy, np.uint8)
    out = np.zeros(4, np.int32)
    keep = {k: (None if m[k] is None else np.ascontiguousarray(m[k], {'ids': np.int32, 'vel': np.float32, 'path_offsets': np.int32, 'zaxis': np.uint8}.get(k, np.float64)))
            for k in m if k != 'count'}
    H.rsp_check(vp(c), vp(policy), int(m['count']), *[vp(keep[k]) for k in ('ids', 'pos', 'vel', 'heading', 'radius', 'pref_speed', 'goal', 'zaxis', 'max_run_dist',
                                                                           'goal_heading', 'path_offsets', 'path_points')], vp(out))
    return int(out[0]), int(out[2]), int(out[1])


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def test_every_outcome_of_respawn_check(H):
    assert check(H, mission())[:2] == (OK, 0)
    # the state of the context, in the order the rules look at it
    assert check(H, mission(), agents=0, state=0)[:2] == (NO_AGENTS, ERR_STATE) and check(H, mission(), state=0)[:2] == (NO_STATE, ERR_STATE)
    assert check(H, mission(), mid_step=1)[:2] == (MID_STEP, ERR_STATE)
    assert check(H, mission(), scenes=1)[:2] == (SCENES, ERR_UNSUPPORTED) and check(H, mission(), comm=1)[:2] == (COMM, ERR_UNSUPPORTED)
    assert check(H, mission(), partition=1)[:2] == (PARTITION, ERR_UNSUPPORTED) and check(H, mission(), shard_count=9)[:2] == (SHARD, ERR_UNSUPPORTED)
    # the arguments
    assert check(H, mission(count=0))[:2] == (BAD_COUNT, ERR_ARG) and check(H, mission(count=-3))[:2] == (BAD_COUNT, ERR_ARG)
    for k in ('ids', 'pos', 'vel', 'heading', 'radius', 'pref_speed', 'goal', 'max_run_dist'):
        assert check(H, mission(**{k: None}))[:2] == (NO_ARRAYS, ERR_ARG), k
    assert check(H, mission(zaxis=np.ones(4, np.uint8)))[:2] == (OK, 0)                     # (nullable, and accepted)
    assert check(H, mission(ids=[0, -1, 2, 3])) == (BAD_ID, ERR_ARG, 1) and check(H, mission(ids=[0, 1, 2, 10])) == (BAD_ID, ERR_ARG, 3)
    assert check(H, mission(ids=[9, 1, 2, 0]))[:2] == (OK, 0)                                # (any order)
    assert check(H, mission(ids=[5, 1, 2, 5])) == (REPEATED_ID, ERR_ARG, 3) and check(H, mission(ids=[7, 7, 2, 7])) == (REPEATED_ID, ERR_ARG, 1)
    for bad in (np.nan, np.inf, -np.inf):
        p = np.ones((4, 3))
        p[2, 1] = bad
        assert check(H, mission(pos=p)) == (NOT_FINITE, ERR_ARG, 2), bad
    for k in ('radius', 'pref_speed', 'max_run_dist'):
        for bad in (0.0, -1.0, np.nan, np.inf):
            v = np.ones(4)
            v[3] = bad
            assert check(H, mission(**{k: v})) == (NOT_POSITIVE, ERR_ARG, 3), (k, bad)
    # the device tracker: goal_heading is needed only when a named row is tracked
    pol = np.array([3, 1, 0, 5, 2, 4, 3, 3, 3, 3], np.uint8)
    assert check(H, mission(), pol, tracker_on=1) == (GOAL_HEADING, ERR_ARG, 2)
    assert check(H, mission(ids=[4, 1, 5, 3]), pol, tracker_on=1) == (GOAL_HEADING, ERR_ARG, 3)
    assert check(H, mission(ids=[4, 1, 5, 9]), pol, tracker_on=1)[:2] == (OK, 0) and check(H, mission(), pol)[:2] == (OK, 0)
    assert check(H, mission(goal_heading=np.zeros((4, 3))), pol, tracker_on=1)[:2] == (OK, 0)
    # the lists
    off, pts = np.array([0, 1, 1, 3, 4], np.int32), np.ones((4, 3))
    assert check(H, mission(path_offsets=off))[:2] == (PATH_HALF, ERR_ARG) and check(H, mission(path_points=pts))[:2] == (PATH_HALF, ERR_ARG)
    assert check(H, mission(), paths_block=1)[:2] == (PATH_BLOCK, ERR_UNSUPPORTED)
    assert check(H, mission(path_offsets=off, path_points=pts), paths_block=1)[:2] == (PATH_BLOCK, ERR_UNSUPPORTED)
    assert check(H, mission(path_offsets=off, path_points=pts))[:2] == (PATH_NO_SLOTS, ERR_UNSUPPORTED)
    assert check(H, mission(path_offsets=off, path_points=pts), path_W=2)[:2] == (OK, 0) and check(H, mission(), path_W=2)[:2] == (OK, 0)
    assert check(H, mission(path_offsets=off, path_points=pts), path_W=1) == (PATH_TOO_LONG, ERR_ARG, 2)
    assert check(H, mission(path_offsets=[0, 2, 1, 3, 4], path_points=pts), path_W=3) == (PATH_OFFSETS, ERR_ARG, 1)
    assert check(H, mission(path_offsets=[-1, 0, 1, 2, 3], path_points=pts), path_W=3) == (PATH_OFFSETS, ERR_ARG, 0)
    bad = pts.copy()
    bad[2, 0] = np.nan
    assert check(H, mission(path_offsets=off, path_points=bad), path_W=2) == (PATH_NOT_FINITE, ERR_ARG, 2)


def test_every_outcome_of_finished_check(H):
    def fin(have_rows=1, capacity=10, have_count=1, struct_bytes=48, **state):
        out = np.zeros(2, np.int32)
        H.rsp_finished_check(vp(ctx_of(**state)), have_rows, capacity, have_count, struct_bytes, vp(out))
        return int(out[0]), int(out[1])
    assert fin() == (OK, 0) and fin(have_rows=0, capacity=0) == (OK, 0) and fin(mid_step=1) == (OK, 0)      # (reading between a pass and its update is legal)
    assert fin(agents=0) == (NO_AGENTS, ERR_STATE) and fin(state=0) == (NO_STATE, ERR_STATE)
    assert fin(capacity=-1) == (FIN_ARGS, ERR_ARG) and fin(have_count=0) == (FIN_ARGS, ERR_ARG) and fin(have_rows=0) == (FIN_ARGS, ERR_ARG)
    assert fin(struct_bytes=40) == (FIN_ARGS, ERR_ARG) and fin(struct_bytes=56) == (FIN_ARGS, ERR_ARG)
    assert fin(scenes=1) == (SCENES, ERR_UNSUPPORTED) and fin(comm=1) == (COMM, ERR_UNSUPPORTED)
    assert fin(partition=1) == (PARTITION, ERR_UNSUPPORTED) and fin(shard_count=3) == (SHARD, ERR_UNSUPPORTED)


# ---- the block -------------------------------------------------------------------------------------------------------------------------
def test_respawn_layout(H):
    """ids i32, public records of 48 bytes, heading / goal / goal_heading 3 x f64, pref_speed / max_run_dist f64, zaxis and the rows' bits u8,
    and with a slot form count + 1 offsets and room for W points per row: sections in this order, each aligned to 64 bytes, none overlapping"""
    row_bytes = [4, 48, 24, 24, 24, 8, 8, 1, 1]
    assert H.rsp_sections() == 11
    for cap in (1, 3, 64, 1000, 100000):
        for W in (0, 1, 5):
            off, total = np.zeros(11, np.int64), np.zeros(1, np.int64)
            H.rsp_layout(cap, W, vp(off), vp(total))
            sizes = [b * cap for b in row_bytes] + ([4 * (cap + 1), 24 * W * cap] if W else [0, 0])
            at = 0
            for s in range(11):
                assert off[s] == at and off[s] % 64 == 0, (cap, W, s)
                at += (sizes[s] + 63) // 64 * 64
            assert total[0] == at


# ---- one row: the host-compiled rule against the Python rule on the corpus ---------------------------------------------------------------
def apply_harness(H, n, policy, m, st, defs, extra, tracker_on=0, W=0, path_vpref=None, paths=None):
    """one call through respawn_pack + respawn_row on the arrays of st / defs / extra, in place; returns (done_delta, tracked per row)"""
    c = ctx_of(n=n, shard_count=n, tracker_on=tracker_on, path_W=W)
    k = len(m['ids'])
    tracked = np.zeros(k, np.int32)
    poff = ppts = None
    if paths is not None:
        poff = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int32)
        ppts = np.array([w for p in paths for w in p], np.float64).reshape(-1, 3)
    gh = m.get('goal_heading')
    keep = [np.ascontiguousarray(m['ids'], np.int32), np.ascontiguousarray(m['pos']), np.ascontiguousarray(m['vel'], np.float32), np.ascontiguousarray(m['heading']),
            np.ascontiguousarray(m['radius']), np.ascontiguousarray(m['pref_speed']), np.ascontiguousarray(m['goal']), m.get('zaxis'), np.ascontiguousarray(m['max_run_dist']),
            gh, poff, ppts]
    delta = H.rsp_apply(vp(c), vp(policy), vp(path_vpref), k, *[vp(a) for a in keep],
                        vp(st['pos']), vp(st['vel']), vp(st['flags']), vp(defs['radius']), vp(st['heading']), vp(defs['goal']), vp(defs['pref_speed']),
                        vp(defs['max_run_dist']), vp(st['total_dist']), vp(st['step_num']), vp(extra['status']), vp(extra['nbr_n']), vp(extra['near_n']),
                        vp(extra['zaxis']), vp(extra['vpref_mode']), vp(extra['nbr_valid']), vp(extra['vpref_ext']), vp(extra.get('trk_nbr0')),
                        vp(extra.get('trk_goal_heading')), vp(extra.get('path_len')), vp(extra.get('path_rem')), vp(extra.get('now_goal')), vp(extra.get('path_pts')),
                        vp(tracked))
    return delta, tracked


def extras(n, rng, tracker=False, W=0):
    e = dict(status=rng.integers(0, 255, n).astype(np.int32), nbr_n=rng.integers(0, 17, n).astype(np.int32), near_n=rng.integers(0, 9, n).astype(np.int32),
             zaxis=rng.integers(0, 2, n).astype(np.uint8), vpref_mode=rng.integers(0, 2, n).astype(np.uint8), nbr_valid=np.ones(n, np.uint8),
             vpref_ext=rng.normal(0, 1, (n, 3)))
    if tracker:
        e.update(trk_nbr0=rng.uniform(0, 9, n), trk_goal_heading=rng.normal(0, 1, (n, 3)))
    if W:
        e.update(path_len=rng.integers(0, W + 1, n).astype(np.int32), path_rem=np.zeros(n, np.int32), now_goal=rng.normal(0, 1, (n, 3)), path_pts=rng.normal(0, 1, (n, W, 3)))
    return e


def test_respawn_row_against_the_python_rule_on_the_corpus(H, oracle):
    """every mission of the corpus's first 20 scenes through respawn_pack + respawn_row (host-compiled) against respawn_rule.apply: the
    named rows' state and definition are the mission's, the counters zero, the last pass's list invalid, done_delta the rows that were
    done -- and every other row keeps every word it had"""
    rng = np.random.default_rng(1)
    missions = 0
    for seed in RR.SEEDS[:20]:
        scene = F.random_scene(seed)
        n = scene['n']
        policy = np.ascontiguousarray(scene['policy'], np.uint8)
        run = RR.oracle_run(oracle, scene)
        prev = dict(pos=scene['pos'], vel=scene['vel'], heading=scene['heading'], flags=scene['flags'], total_dist=np.zeros(n), step_num=np.zeros(n, np.int32))
        defs_prev = {k: np.array(scene[k], np.float64) for k in RR.DEF_KEYS}
        for st in run:
            m = st['mission']
            if m is not None:
                missions += 1
                got = {k: np.array(prev[k], copy=True) for k in F.STATE_KEYS}
                got_defs = {k: np.array(defs_prev[k], copy=True) for k in RR.DEF_KEYS}
                want = {k: np.array(prev[k], copy=True) for k in F.STATE_KEYS}
                want_defs = {k: np.array(defs_prev[k], copy=True) for k in RR.DEF_KEYS}
                RR.apply(want, want_defs, m)
                e = extras(n, rng)
                e0 = {k: v.copy() for k, v in e.items()}
                delta, tracked = apply_harness(H, n, policy, m, got, got_defs, e)
                assert delta == int(((prev['flags'][m['ids']] & 7) != 0).sum()) == len(m['ids']) and not tracked.any()      # (the corpus respawns finished rows)
                for k in F.STATE_KEYS:
                    assert np.array_equal(got[k], want[k]), (seed, k)
                for k in RR.DEF_KEYS:
                    assert np.array_equal(got_defs[k], want_defs[k]), (seed, k)
                others = np.setdiff1d(np.arange(n), m['ids'])
                for k in e:
                    assert np.array_equal(e[k][others], e0[k][others]), (seed, k)
                ids = m['ids']
                assert not e['status'][ids].any() and not e['nbr_n'][ids].any() and not e['nbr_valid'][ids].any() and (e['near_n'][ids] == -1).all()
                for k in ('zaxis', 'vpref_mode', 'vpref_ext'):                  # no zaxis in the call, no tracker, no lists: the rows keep theirs
                    assert np.array_equal(e[k][ids], e0[k][ids]), (seed, k)
            prev = {k: st[k] for k in F.STATE_KEYS}
            defs_prev = st['defs']
    assert missions > 100


def test_respawn_row_with_tracker_lists_and_zaxis(H):
    """the branches the plain corpus does not reach: a tracked row under the device tracker (initial record, goal_heading, vpref_mode 1,
    vpref_ext 0, first-neighbour distSq -1), rows that are not done (done_delta 0), zaxis given, lists in slot form brought and not"""
    rng = np.random.default_rng(2)
    n, W = 50, 4
    policy = (np.arange(n) % 6).astype(np.uint8)
    st = dict(pos=rng.normal(0, 1, (n, 3)), vel=rng.normal(0, 1, (n, 3)).astype(np.float32), heading=rng.normal(0, 1, (n, 3)), flags=(np.arange(n) % 3 == 0).astype(np.uint8) * 2,
              total_dist=rng.uniform(0, 5, n), step_num=rng.integers(0, 50, n).astype(np.int32))
    defs = dict(radius=np.full(n, 0.3), pref_speed=np.ones(n), goal=rng.normal(0, 1, (n, 3)), max_run_dist=np.full(n, 20.0))
    for brings in (True, False):
        e = extras(n, rng, tracker=True, W=W)
        e0 = {k: v.copy() for k, v in e.items()}
        path_vpref = ((e['path_len'] > 0) & ~np.isin(policy, (0, 5))).astype(np.uint8)
        ids = np.array([7, 0, 5, 12, 30, 31, 2], np.int32)
        k = len(ids)
        m = dict(ids=ids, pos=rng.normal(0, 1, (k, 3)), vel=np.zeros((k, 3), np.float32), heading=rng.normal(0, 1, (k, 3)), radius=np.full(k, 0.5), pref_speed=np.full(k, 0.8),
                 goal=rng.normal(0, 1, (k, 3)), max_run_dist=np.full(k, 7.0), zaxis=np.ones(k, np.uint8), goal_heading=rng.normal(0, 1, (k, 3)))
        paths = [[[float(j), 1.0, 2.0]] * (j % (W + 1)) for j in range(k)] if brings else None
        s2, d2 = {a: v.copy() for a, v in st.items()}, {a: v.copy() for a, v in defs.items()}
        delta, tracked = apply_harness(H, n, policy, m, s2, d2, e, tracker_on=1, W=W, path_vpref=path_vpref, paths=paths)
        assert delta == int((st['flags'][ids] != 0).sum()) == 3
        trk = np.isin(policy[ids], (0, 5))
        assert np.array_equal(tracked.astype(bool), trk) and trk.sum() == 4
        assert (e['zaxis'][ids] == 1).all() and (e['trk_nbr0'][ids] == -1.0).all()
        assert (e['vpref_mode'][ids][trk] == 1).all() and not e['vpref_ext'][ids][trk].any()
        assert np.array_equal(e['trk_goal_heading'][ids][trk], m['goal_heading'][trk]) and np.array_equal(e['trk_goal_heading'][ids][~trk], e0['trk_goal_heading'][ids][~trk])
        reset = path_vpref[ids].astype(bool) & ~trk                             # straight-line rows k_waypoint was feeding: their policy's own rule again
        assert np.array_equal(e['vpref_mode'][ids][~trk], np.where(reset[~trk], 0, e0['vpref_mode'][ids][~trk]))
        assert np.array_equal(e['vpref_ext'][ids][~trk], e0['vpref_ext'][ids][~trk])
        want_len = np.array([len(p) for p in paths], np.int32) if brings else np.zeros(k, np.int32)
        assert np.array_equal(e['path_len'][ids], want_len) and np.array_equal(e['path_rem'][ids], want_len) and np.isnan(e['now_goal'][ids]).all()
        for j, a in enumerate(ids):
            assert np.array_equal(e['path_pts'][a][:want_len[j]], np.array(paths[j], np.float64).reshape(-1, 3) if brings else np.zeros((0, 3)))
            assert np.array_equal(e['path_pts'][a][want_len[j]:], e0['path_pts'][a][want_len[j]:])          # room behind the list keeps what it held
        others = np.setdiff1d(np.arange(n), ids)
        for key in e:
            assert np.array_equal(e[key][others], e0[key][others]), key


# ---- the finished list -----------------------------------------------------------------------------------------------------------------
def test_finished_offsets_against_flatnonzero(H):
    """the ordered compaction as the three kernels run it (a count per tile of 256 rows by ballot and popcount, finished_offsets' scan, a
    row at its tile's offset + its rank): nobody finished, everybody, counts at one tile +- 1, random sets; with a capacity below the count"""
    tile = H.rsp_tile()
    assert tile == 256
    rng = np.random.default_rng(3)
    for n in (1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1, 1000, 70001):
        tiles = (n + tile - 1) // tile
        for kind in ('none', 'all', 'random', 'sparse', 'tile_minus', 'tile', 'tile_plus'):
            if kind.startswith('tile'):
                k = min(n, tile + {'tile_minus': -1, 'tile': 0, 'tile_plus': 1}[kind])
                flags = np.zeros(n, np.uint32)
                flags[rng.choice(n, k, replace=False)] = 2
            else:
                flags = {'none': np.zeros(n), 'all': rng.choice([1, 2, 4, 6], n), 'random': (rng.random(n) < 0.5) * rng.choice([1, 2, 4], n),
                         'sparse': (rng.random(n) < 0.01) * 1}[kind].astype(np.uint32)
            flags |= (rng.integers(0, 2, n) * 8).astype(np.uint32)                  # (bits that are no done flag do not count)
            want = np.flatnonzero(flags & 7)
            for cap in (n, len(want) // 2, 0):
                out, counts, offsets = np.full(max(cap, 1), -1, np.int32), np.zeros(tiles, np.int32), np.zeros(tiles, np.int32)
                total = H.rsp_finished(n, vp(flags), cap, vp(out), vp(counts), vp(offsets))
                assert total == len(want), (n, kind, cap)
                assert np.array_equal(out[:min(cap, total)], want[:cap]), (n, kind, cap)
                assert np.array_equal(counts, np.add.reduceat((flags & 7) != 0, np.arange(0, n, tile)).astype(np.int32))
                assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(counts)[:-1]]))


# ---- the harness as a program under the sanitizers --------------------------------------------------------------------------------------
def test_standalone_under_sanitizers():
    """The rules as a program of their own (its main packs random calls into heap blocks of exactly the layout's size and applies them to
    heap arrays of exactly n rows, then compacts the flags) under -fsanitize=address,undefined.  Host code only; nothing of it is loaded
    into python."""
    exe = os.path.join(harness_util.BUILD, 'respawn_harness_san')
    os.makedirs(harness_util.BUILD, exist_ok=True)
    subprocess.check_call(['g++', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan',
                           '-DRESPAWN_MAIN'] + FLAGS + ['-o', exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'respawn_harness: ok' in r.stdout


# ---- the symbols ---------------------------------------------------------------------------------------------------------------------------
def test_the_struct_and_the_symbols(H):
    from sca_amd import _lib
    assert H.rsp_finished_row_bytes() == 48 == _lib.FINISHED_DTYPE.itemsize == C.sizeof(_lib.FinishedRow)
    assert [(n, _lib.FINISHED_DTYPE.fields[n][1]) for n in _lib.FINISHED_DTYPE.names] == [('id', 0), ('flags', 4), ('step_num', 8), ('reserved', 12), ('total_dist', 16), ('pos', 24)]
    L = _lib.lib()
    for name in ('sca_respawn_agents', 'sca_get_finished'):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    hdr = open(os.path.join(harness_util.ROOT, 'include', 'sca_hip.h')).read()
    assert re.search(r'\bint sca_respawn_agents\(', hdr) and re.search(r'\bint sca_get_finished\(', hdr)
    assert len(_lib.SIGNATURES['sca_respawn_agents'][1]) == 14 and len(_lib.SIGNATURES['sca_get_finished'][1]) == 5
    assert L.sca_version() == 103                                  # the feature is detected by the symbol
    from sca_amd import solver as S, env as E, lifelong
    assert callable(S.BatchedSolver.respawn) and callable(S.BatchedSolver.finished) and callable(E.MACAEnv.respawn) and callable(E.MACAEnv.finished)
    assert callable(lifelong.run_lifelong)


# ---- what the corpus holds ---------------------------------------------------------------------------------------------------------------
def test_what_the_corpus_holds(oracle):
    """Seeds 0-39 x 12 steps, counted from the oracle and the rule alone.  Measured: 36 105 respawns, 27 478 of them repeats, 33 279
    collisions and 264 arrivals of respawned rows, 6 036 ORCA3D-LP and 12 009 tracked rows respawned, 411 306 list entries naming a
    respawned row, a respawn in 33 of the 40 scenes.  The floors are conditions on the corpus, so that no branch passes untested."""
    total = dict.fromkeys(RR.QUANTITIES, 0)
    scenes = 0
    for seed in RR.SEEDS:
        scene = F.random_scene(seed)
        c = RR.corpus_counts(scene, RR.oracle_run(oracle, scene))
        for k in total:
            total[k] += c[k]
        scenes += c['respawns'] > 0
    print('respawn corpus:', total, 'scenes with a respawn:', scenes)
    assert total['respawns'] >= 30000 and total['repeats'] >= 20000
    assert total['collisions'] >= 20000 and total['arrivals'] >= 200
    assert total['lp_rows'] >= 5000 and total['tracked_rows'] >= 10000
    assert total['list_entries'] >= 300000
    assert scenes >= 30
