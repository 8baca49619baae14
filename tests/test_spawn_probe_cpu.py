"""Spawn admission (sca_probe_clearance, sca_respawn_agents_gated) without a GPU: the pure rules of sca_amd/csrc/sca_spawn.h, compiled for
the host behind tests/spawn_harness.cpp -- spawn_tile_partial, spawn_fold and the gate against the Python rule of tests/spawn_rule.py at
two tile sizes, every outcome of spawn_check with its code, the block's layout -- the harness as a program of its own under the
sanitizers, the symbols, and what the gating corpus holds (counted from the oracle and the rule alone)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import clearance_rule as CR
import edge_corpus as E
import form_fuzz as F
import harness_util
import respawn_rule as RR
import spawn_rule as SR

SRC = os.path.join(harness_util.ROOT, 'tests', 'spawn_harness.cpp')
FLAGS = ['-std=c++17', '-ffp-contract=off', '-mfma', '-fno-builtin-pow', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I' + harness_util.CSRC]
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5                   # include/sca_hip.h
(OK, NO_AGENTS, NO_STATE, MID_STEP, BAD_COUNT, NO_ARRAYS, NOT_FINITE, BAD_RADIUS, BAD_IGNORE, BAD_STRUCT, BAD_MARGIN, NO_VERDICT, SCENES, SHARD, COMM,
 PARTITION) = range(16)                                            # SpawnFault
CTX_KEYS = ('agents', 'state', 'mid_step', 'scenes', 'comm', 'partition', 'n', 'shard_count', 'tracker_on', 'paths_block', 'path_W')
SMALL_P = 64                                                       # the second tile size: many tiles at the corpus's sizes


@pytest.fixture(scope='module')
def H():
    out = os.path.join(harness_util.BUILD, 'libspawn_harness.so')
    deps = [SRC, os.path.join(harness_util.ROOT, 'include', 'sca_hip.h')] + \
        [os.path.join(harness_util.CSRC, f) for f in ('sca_spawn.h', 'sca_clearance.h', 'sca_respawn.h', 'sca_scenes.h', 'sca_core.h', 'sca_glibc_math.h',
                                                      'sca_glibc_tables.h', 'sca_constants.h')]
    os.makedirs(harness_util.BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(['g++', '-O2', '-fPIC', '-shared'] + FLAGS + ['-o', out, SRC])
    h = C.CDLL(out)
    h.spn_check.restype = None
    h.spn_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    h.spn_gate_check.restype = None
    h.spn_gate_check.argtypes = [C.c_double, C.c_int, C.c_void_p]
    h.spn_layout.restype = None
    h.spn_layout.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    h.spn_partial_index.restype = C.c_longlong
    h.spn_probe.restype = None
    h.spn_probe.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    h.spn_gate.restype = None
    h.spn_gate.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int,
                           C.c_void_p, C.c_void_p]
    return h


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def world_of(scene_like):
    """(pos, radius, obs_pos, obs_radius) as contiguous float64 arrays"""
    pos, radius, opos, orad = scene_like
    return (np.ascontiguousarray(pos, np.float64).reshape(-1, 3), np.ascontiguousarray(radius, np.float64),
            np.ascontiguousarray(opos, np.float64).reshape(-1, 3), np.ascontiguousarray(orad, np.float64))


def harness_probe(H, w, qpos, qrad, ignore, P):
    pos, radius, opos, orad = w
    qpos, qrad = np.ascontiguousarray(qpos, np.float64).reshape(-1, 3), np.ascontiguousarray(qrad, np.float64)
    ignore = None if ignore is None else np.ascontiguousarray(ignore, np.int32)
    out = np.zeros(len(qrad), CR.DTYPE)
    H.spn_probe(len(radius), vp(pos), vp(radius), len(orad), vp(opos), vp(orad), len(qrad), vp(qpos), vp(qrad), vp(ignore), P, vp(out))
    return out


def harness_gate(H, w, ids, qpos, qrad, margin, P):
    pos, radius, opos, orad = w
    qpos, qrad, ids = np.ascontiguousarray(qpos, np.float64).reshape(-1, 3), np.ascontiguousarray(qrad, np.float64), np.ascontiguousarray(ids, np.int32)
    out, verdict = np.zeros(len(ids), CR.DTYPE), np.full(len(ids), -9, np.int32)
    H.spn_gate(len(radius), vp(pos), vp(radius), len(orad), vp(opos), vp(orad), len(ids), vp(ids), vp(qpos), vp(qrad), float(margin), P, vp(out), vp(verdict))
    return verdict, out


def differ(got, want):
    bad = np.zeros(len(want), bool)
    for f in want.dtype.names:
        bad |= E.differ(got[f], want[f])
    return np.flatnonzero(bad)


def both_tiles(H, w, qpos, qrad, ignore, what):
    """the harness at the library's tile size and at SMALL_P: equal to each other and to the Python rule"""
    want = SR.probe(qpos, qrad, ignore, *w)
    for P in (H.spn_tile(), SMALL_P):
        got = harness_probe(H, w, qpos, qrad, ignore, P)
        bad = differ(got, want)
        assert bad.size == 0, (what, 'P', P, bad[:8].tolist(), got[bad[:3]], want[bad[:3]])
    assert not want['agent_step'].any() and not want['obs_step'].any()
    return want


# ---- the probe against the Python rule ---------------------------------------------------------------------------------------------------
def test_probe_on_the_fuzz_scenes(H, oracle):
    """seeds 0-39 before the first oracle step and after three: queries at every agent's own position with ignore = self -- exactly
    clearance_rule.step_minimum, the closest-approach rule's candidate -- at random points, and exactly on agents with nobody ignored"""
    rng = np.random.default_rng(11)
    own = on_agent = 0
    for seed in RR.SEEDS:
        scene = F.random_scene(seed)
        n = scene['n']
        run = RR.oracle_run(oracle, scene)
        for when, (pos, radius) in ((0, (scene['pos'], scene['radius'])), (3, (run[2]['pos'], run[2]['defs']['radius']))):
            w = world_of((pos, radius, scene['obs_pos'], scene['obs_radius']))
            want = both_tiles(H, w, w[0], w[1], np.arange(n, dtype=np.int32), (seed, when, 'own'))
            for a in range(0, n, max(1, n // 25)):                               # (spelled out: the rule itself is step_minimum)
                c, who, _ = CR.step_minimum(w[0][a], float(w[1][a]), a, w[0], w[1], True)
                assert (want['agent_clear'][a], want['agent_partner'][a]) == (c, who), (seed, when, a)
            own += n
            side = RR.box_of(scene)
            k = min(n, 97)
            both_tiles(H, w, rng.uniform(-side, side, (k, 3)), rng.choice([0.0, 0.3, 1.0], k), None, (seed, when, 'random'))
            pick = rng.choice(n, min(n, 31), replace=False)
            got = both_tiles(H, w, w[0][pick], np.full(len(pick), 0.5), np.full(len(pick), -1, np.int32), (seed, when, 'on agents'))
            assert (got['agent_clear'] <= 0.0 - (0.5 + w[1][pick])).all()        # at distance 0 from agent b: at most -(r_q + r_b)
            on_agent += len(pick)
    assert own > 10000 and on_agent > 500


LATTICES = ('F20_edge_lattice4_s2_orca', 'F20_edge_lattice3_s2_a', 'F20_edge_lattice4_s10_mixed')


@pytest.mark.parametrize('name', LATTICES)
def test_lattice_ties_keep_the_lowest_id(H, name):
    """integer lattices: 6 / 12 / 8 partners at equal distances -- the tied rows are counted and the lowest id wins at both tile sizes"""
    scene = E.step_scene(name, 0)
    w = world_of((scene['pos'], scene['radius'], scene['obs_pos'], scene['obs_radius']))
    n = scene['n']
    ties = []
    want = SR.probe(w[0], w[1], np.arange(n), *w, ties=ties)
    for P in (H.spn_tile(), SMALL_P, 7):
        got = harness_probe(H, w, w[0], w[1], np.arange(n), P)
        assert differ(got, want).size == 0, (name, P)
    tied = [a for a in range(n) if ties[a] > 1]
    assert len(tied) >= 5, (name, len(tied))
    for a in tied:                                                               # nobody below the partner has the same value
        c = want['agent_clear'][a]
        lower = [b for b in range(want['agent_partner'][a]) if b != a and CR.l3norm(w[0][a].tolist(), w[0][b].tolist()) - (w[1][a] + w[1][b]) == c]
        assert not lower, (name, a)


def exp3_obstacles():
    s = E.step_scene('F10_sca_exp3_map', 0)
    assert s['m'] == 1491
    return s['obs_pos'], s['obs_radius']


def test_partner_and_query_counts(H):
    """partner counts 1, 2, P-1, P, P+1 and 2P+1 (P the library's tile and the small one) with 0, 1, 23 and 1491 obstacles, query counts 1, 63,
    64, 65 and 257 -- either side of a tile, of a slice and of a chunk"""
    rng = np.random.default_rng(12)
    eo, er = exp3_obstacles()
    centre = np.asarray(eo, np.float64).reshape(-1, 3).mean(axis=0)
    Ps = (H.spn_tile(), SMALL_P)
    sizes = sorted({1, 2} | {P + d for P in Ps for d in (-1, 0, 1)} | {2 * P + 1 for P in Ps})
    assert H.spn_chunk() == 64 and H.spn_tile() % H.spn_waves() == 0
    for n in sizes:
        for m in (0, 1, 23, 1491):
            pos = rng.uniform(-8, 8, (n, 3)) + (centre if m == 1491 else 0.0)
            radius = rng.choice([0.3, 0.5, 1.0], n)
            opos, orad = (eo, er) if m == 1491 else (rng.uniform(-8, 8, (m, 3)), rng.choice([0.2, 1.0, 2.0], m))
            w = world_of((pos, radius, opos, orad))
            for count in ((1, 63, 64, 65, 257) if m in (0, 23) or n <= 2 else (65,)):
                qpos = rng.uniform(-8, 8, (count, 3)) + (centre if m == 1491 else 0.0)
                ignore = rng.integers(-1, n, count).astype(np.int32)
                want = both_tiles(H, w, qpos, rng.choice([0.0, 0.5], count), ignore, (n, m, count))
                assert np.isfinite(want['obs_clear']).all() == (m > 0) and ((want['obs_partner'] >= 0).all() == (m > 0))
                if n == 1:
                    alone = ignore == 0
                    assert np.isinf(want['agent_clear'][alone]).all() and (want['agent_partner'][alone] == -1).all()      # an empty half: +inf, -1, 0
                assert (want['agent_partner'] != ignore).all() or n == 1
    assert H.spn_tiles(1, 0, 512) == 1 and H.spn_tiles(512, 0, 512) == 1 and H.spn_tiles(512, 1, 512) == 2 and H.spn_tiles(100000, 1491, 512) == 199
    assert H.spn_partial_index(3, 5, 1024) == 3 * 1024 + 5


def test_the_margin_boundary_pair(H):
    """a pair at distance exactly 2.0 with radii 0.5: c = 1.0 -- refused at margin 1.0, admitted at nextafter(1.0, 0.0); the same pair as two
    rows of one call is an entry block at 1.0 and none just below"""
    pos, radius = np.array([[0.0, 0.0, 5.0], [40.0, 0.0, 5.0]]), np.array([0.5, 0.5])
    w = world_of((pos, radius, np.zeros((0, 3)), np.zeros(0)))
    below = float(np.nextafter(1.0, 0.0))
    q = np.array([[2.0, 0.0, 5.0]])
    rec = both_tiles(H, w, q, [0.5], [1], 'boundary')
    assert rec['agent_clear'][0] == 1.0 and rec['agent_partner'][0] == 0
    for P in (H.spn_tile(), SMALL_P):
        v, _ = harness_gate(H, w, [1], q, [0.5], 1.0, P)
        assert v.tolist() == [SR.BLOCKED_AGENT] == SR.gate([1], q, [0.5], 1.0, *w)[0].tolist()
        v, _ = harness_gate(H, w, [1], q, [0.5], below, P)
        assert v.tolist() == [SR.ADMITTED] == SR.gate([1], q, [0.5], below, *w)[0].tolist()
        two = np.array([[100.0, 0.0, 5.0], [102.0, 0.0, 5.0]])
        assert harness_gate(H, w, [0, 1], two, [0.5, 0.5], 1.0, P)[0].tolist() == [SR.ADMITTED, SR.BLOCKED_ENTRY]
        assert harness_gate(H, w, [0, 1], two, [0.5, 0.5], below, P)[0].tolist() == [SR.ADMITTED, SR.ADMITTED]


def test_the_chain(H):
    """a < b < c where b conflicts with both: c is refused although b was (the parallel rule's stated difference from the sequential
    greedy); and where the WORLD blocks a, a blocks nobody: b is admitted"""
    pos, radius = np.array([[0.0, 0.0, 5.0], [50.0, 0.0, 5.0], [60.0, 0.0, 5.0], [70.0, 0.0, 5.0]]), np.full(4, 0.5)
    w = world_of((pos, radius, np.zeros((0, 3)), np.zeros(0)))
    rows = np.array([[100.0, 0.0, 5.0], [101.2, 0.0, 5.0], [102.4, 0.0, 5.0]])
    for P in (H.spn_tile(), SMALL_P):
        v, _ = harness_gate(H, w, [1, 2, 3], rows, np.full(3, 0.5), 0.5, P)
        assert v.tolist() == [SR.ADMITTED, SR.BLOCKED_ENTRY, SR.BLOCKED_ENTRY] == SR.gate([1, 2, 3], rows, np.full(3, 0.5), 0.5, *w)[0].tolist()
        rows2 = np.array([[1.2, 0.0, 5.0], [2.4, 0.0, 5.0]])                      # the first next to agent 0, the second next to the first only
        chains = []
        want = SR.gate([1, 2], rows2, np.full(2, 0.5), 0.5, *w, chains=chains)[0]
        v, _ = harness_gate(H, w, [1, 2], rows2, np.full(2, 0.5), 0.5, P)
        assert v.tolist() == [SR.BLOCKED_AGENT, SR.ADMITTED] == want.tolist() and chains == [(0, 1)]


# ---- the gate on the corpus, and what the corpus holds -----------------------------------------------------------------------------------
def test_gate_on_the_corpus_and_what_it_holds(H, oracle):
    """Seeds 0-39 x 12 steps of spawn_rule.oracle_run_gated at margin 0.5: every offered call through the host-compiled probe, world test
    and gate at two tile sizes against the Python rule.  Counted from the oracle and the rule alone -- measured: 2 528 rows admitted (in 33
    scenes), 30 912 blocked by an agent (21), 1 511 by an obstacle (9), 707 by an earlier row of the call (22), 1 023 chain cases, 283 calls
    of which 190 admit a part and 34 nobody.  The floors are conditions on the corpus, so that no verdict passes untested."""
    total = dict.fromkeys(SR.VERDICTS + ('chains', 'calls', 'calls_none', 'calls_partly'), 0)
    scenes = dict.fromkeys(SR.VERDICTS, 0)
    for seed in RR.SEEDS:
        scene = F.random_scene(seed)
        run = SR.oracle_run_gated(oracle, scene)
        for st in run:
            m = st['offered']
            if m is None:
                continue
            w = world_of((st['pos_at_gate'], st['radius_at_gate'], scene['obs_pos'], scene['obs_radius']))
            for P in (H.spn_tile(), SMALL_P):
                v, rec = harness_gate(H, w, m['ids'], m['pos'], m['radius'], SR.MARGIN, P)
                assert np.array_equal(v, st['verdict']), (seed, P, np.flatnonzero(v != st['verdict'])[:8])
                assert differ(rec, st['probe']).size == 0, (seed, P)
        c = SR.corpus_counts(run)
        for k in total:
            total[k] += c[k]
        for k in SR.VERDICTS:
            scenes[k] += c[k] > 0
    print('gating corpus:', total, 'scenes per verdict:', scenes)
    for k in SR.VERDICTS:
        assert total[k] >= 20 and scenes[k] >= 3, (k, total[k], scenes[k])
    assert total['chains'] >= 1 and total['calls_partly'] >= 20 and total['calls_none'] >= 1


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------
def test_every_outcome_of_spawn_check(H):
    def ctx_of(**state):
        s = dict(agents=1, state=1, mid_step=0, scenes=0, comm=0, partition=0, n=10, shard_count=10, tracker_on=0, paths_block=0, path_W=0)
        s.update(state)
        return np.array([s[k] for k in CTX_KEYS], np.int32)

    def check(count=4, pos='ok', radius='ok', ignore=None, have_out=1, struct_bytes=32, **state):
        pos = np.ones((4, 3)) if isinstance(pos, str) else pos
        radius = np.full(4, 0.5) if isinstance(radius, str) else radius
        ignore = None if ignore is None else np.ascontiguousarray(ignore, np.int32)
        out = np.zeros(3, np.int32)
        H.spn_check(vp(ctx_of(**state)), count, vp(pos), vp(radius), vp(ignore), have_out, struct_bytes, vp(out))
        return tuple(int(x) for x in out)
    assert check()[:2] == (OK, 0) and check(ignore=[-1, 0, 9, 3])[:2] == (OK, 0)
    # the state of the context, in the order the rules look at it (respawn_context_check's)
    assert check(agents=0, state=0)[:2] == (NO_AGENTS, ERR_STATE) and check(state=0)[:2] == (NO_STATE, ERR_STATE) and check(mid_step=1)[:2] == (MID_STEP, ERR_STATE)
    assert check(scenes=1)[:2] == (SCENES, ERR_UNSUPPORTED) and check(comm=1)[:2] == (COMM, ERR_UNSUPPORTED)
    assert check(partition=1)[:2] == (PARTITION, ERR_UNSUPPORTED) and check(shard_count=9)[:2] == (SHARD, ERR_UNSUPPORTED)
    # the arguments
    assert check(count=0)[:2] == (BAD_COUNT, ERR_ARG) and check(count=-2)[:2] == (BAD_COUNT, ERR_ARG)
    assert check(pos=None)[:2] == (NO_ARRAYS, ERR_ARG) and check(radius=None)[:2] == (NO_ARRAYS, ERR_ARG) and check(have_out=0)[:2] == (NO_ARRAYS, ERR_ARG)
    for bad in (np.nan, np.inf, -np.inf):
        p = np.ones((4, 3))
        p[2, 1] = bad
        assert check(pos=p) == (NOT_FINITE, ERR_ARG, 2), bad
    for bad in (-1e-9, -1.0, np.nan, np.inf):
        r = np.full(4, 0.5)
        r[3] = bad
        assert check(radius=r) == (BAD_RADIUS, ERR_ARG, 3), bad
    assert check(radius=np.zeros(4))[:2] == (OK, 0)                              # a point probe
    assert check(ignore=[0, -2, 1, 1]) == (BAD_IGNORE, ERR_ARG, 1) and check(ignore=[0, 1, 2, 10]) == (BAD_IGNORE, ERR_ARG, 3)
    assert check(struct_bytes=24)[:2] == (BAD_STRUCT, ERR_ARG) and check(struct_bytes=40)[:2] == (BAD_STRUCT, ERR_ARG)
    # what the gated respawn adds to respawn_check
    def gate(margin, have_verdict=1):
        out = np.zeros(2, np.int32)
        H.spn_gate_check(margin, have_verdict, vp(out))
        return int(out[0]), int(out[1])
    assert gate(0.0) == (OK, 0) and gate(0.5) == (OK, 0)
    for bad in (-1e-9, -1.0, np.nan, np.inf, -np.inf):
        assert gate(bad) == (BAD_MARGIN, ERR_ARG), bad
    assert gate(0.5, 0) == (NO_VERDICT, ERR_ARG)


def test_spawn_layout(H):
    """queries of 32 bytes, ignore words, records of 32 bytes, verdict words: sections in this order, each aligned to 64 bytes"""
    for cap in (1, 3, 64, 1024, 100000):
        off, total = np.zeros(4, np.int64), np.zeros(1, np.int64)
        H.spn_layout(cap, vp(off), vp(total))
        at = 0
        for s, b in enumerate((32, 4, 32, 4)):
            assert off[s] == at and at % 64 == 0, (cap, s)
            at += (b * cap + 63) // 64 * 64
        assert total[0] == at


# ---- the harness as a program under the sanitizers --------------------------------------------------------------------------------------
def test_standalone_under_sanitizers():
    """The rules as a program of their own (its main probes and gates random worlds through heap blocks of exactly the layout's size and
    partials of exactly tiles x queries records, at two tile sizes) under -fsanitize=address,undefined.  Host code only; nothing of it is
    loaded into python."""
    exe = os.path.join(harness_util.BUILD, 'spawn_harness_san')
    os.makedirs(harness_util.BUILD, exist_ok=True)
    subprocess.check_call(['g++', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan',
                           '-DSPAWN_MAIN'] + FLAGS + ['-o', exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'spawn_harness: ok' in r.stdout


# ---- the symbols ---------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_and_the_python_layers():
    from sca_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(harness_util.ROOT, 'include', 'sca_hip.h')).read()
    for name in ('sca_probe_clearance', 'sca_respawn_agents_gated'):
        assert name in _lib.SIGNATURES and hasattr(L, name) and re.search(r'\bint %s\(' % name, hdr)
    assert len(_lib.SIGNATURES['sca_probe_clearance'][1]) == 7 and len(_lib.SIGNATURES['sca_respawn_agents_gated'][1]) == 18
    assert _lib.SIGNATURES['sca_respawn_agents_gated'][1][:14] == _lib.SIGNATURES['sca_respawn_agents'][1]
    assert L.sca_version() == 103                                  # the feature is detected by the symbols
    vals = {k: int(v) for k, v in re.findall(r'\b(SCA_SPAWN_[A-Z_]+)\s*=\s*(\d+)', hdr)}
    assert vals == dict(SCA_SPAWN_ADMITTED=0, SCA_SPAWN_BLOCKED_AGENT=1, SCA_SPAWN_BLOCKED_OBSTACLE=2, SCA_SPAWN_BLOCKED_ENTRY=3)
    import inspect
    from sca_amd import solver as S, env as E2, lifelong
    assert (S.SPAWN_ADMITTED, S.SPAWN_BLOCKED_AGENT, S.SPAWN_BLOCKED_OBSTACLE, S.SPAWN_BLOCKED_ENTRY) == (SR.ADMITTED, SR.BLOCKED_AGENT, SR.BLOCKED_OBSTACLE, SR.BLOCKED_ENTRY)
    assert callable(S.BatchedSolver.probe_clearance) and callable(E2.MACAEnv.probe)
    assert inspect.signature(S.BatchedSolver.respawn).parameters['margin'].default is None
    assert inspect.signature(E2.MACAEnv.respawn).parameters['margin'].default is None
    assert inspect.signature(lifelong.run_lifelong).parameters['spawn_margin'].default is None
