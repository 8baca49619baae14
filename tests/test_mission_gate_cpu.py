"""The mission tables' admission gate (sca_set_mission_gate) without a GPU: the pure rules of sca_amd/csrc/sca_missions.h compiled for the
host behind tests/mission_gate_harness.cpp -- every outcome of mission_gate_check and of the getters' checks with its code, place / query /
settle and a whole step's gate (the tiles' counts, the places, the probe through partials, the gate walk, the words) against the Python rule
of tests/mission_gate_rule.py on the corpus, the harness as a program of its own under the sanitizers, the symbols, and what the corpus
holds at margin 0.5 with and without a cap (counted from the oracle and the rule alone)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import form_fuzz as F
import harness_util
import mission_gate_rule as GR
import mission_rule as MR
import spawn_rule as SR

SRC = os.path.join(harness_util.ROOT, 'tests', 'mission_gate_harness.cpp')
FLAGS = ['-std=c++17', '-ffp-contract=off', '-mfma', '-fno-builtin-pow', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I' + harness_util.CSRC]
OK, NO_TABLES, MID_STEP, NEVER_SET, BAD_MARGIN, BAD_CAP, TOO_LARGE, GET_ARGS = range(8)          # MissionGateFault
ERR_ARG, ERR_STATE = -1, -3


@pytest.fixture(scope='module')
def H():
    out = os.path.join(harness_util.BUILD, 'libmission_gate_harness.so')
    deps = [SRC, os.path.join(harness_util.ROOT, 'include', 'sca_hip.h')] + \
        [os.path.join(harness_util.CSRC, f) for f in ('sca_missions.h', 'sca_spawn.h', 'sca_respawn.h', 'sca_clearance.h', 'sca_scenes.h', 'sca_core.h')]
    os.makedirs(harness_util.BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(['g++', '-O2', '-fPIC', '-shared'] + FLAGS + ['-o', out, SRC])
    h = C.CDLL(out)
    for name in ('mg_sizes', 'mg_check', 'mg_getter_checks', 'mg_query', 'mg_settle'):
        getattr(h, name).restype = None
    h.mg_check.argtypes = [C.c_int] * 5 + [C.c_double, C.c_int32, C.c_void_p, C.c_void_p]
    h.mg_getter_checks.argtypes = [C.c_int] * 8 + [C.c_void_p]
    h.mg_class.argtypes = [C.c_int32, C.c_int]
    h.mg_place.argtypes = [C.c_int] * 3
    h.mg_query.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    h.mg_settle.argtypes = [C.c_int32] * 3 + [C.c_void_p]
    h.mg_step.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int] + [C.c_void_p] * 9
    return h


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def sizes(H):
    out = np.zeros(8, np.int32)
    H.mg_sizes(vp(out))
    return out


def check(H, tables=1, mid_step=0, n=100, m=3, on=1, margin=0.5, cap=0):
    out, scratch = np.zeros(3, np.int32), np.zeros(1, np.int64)
    H.mg_check(tables, mid_step, n, m, on, margin, cap, vp(out), vp(scratch))
    return int(out[0]), int(out[1]), int(out[2]), int(scratch[0])


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------------
def test_every_outcome_of_mission_gate_check(H):
    z = sizes(H)
    batch, tile = int(z[2]), int(z[3])
    assert check(H) == (OK, 0, 100, -(-103 // tile) * 100 * 32)
    assert check(H, n=5000, m=0)[:3] == (OK, 0, batch)                      # max_per_step 0: min(n, SPAWN_BATCH)
    assert check(H, n=100, cap=100)[:3] == (OK, 0, 100) and check(H, n=100, cap=1)[:3] == (OK, 0, 1)
    assert check(H, tables=0)[:2] == (NO_TABLES, ERR_STATE)
    assert check(H, tables=0, mid_step=1)[:2] == (NO_TABLES, ERR_STATE)     # the first that applies
    assert check(H, mid_step=1)[:2] == (MID_STEP, ERR_STATE)
    for bad in (-1e-9, -1.0, float('nan'), float('inf'), -float('inf')):
        assert check(H, margin=bad)[:2] == (BAD_MARGIN, ERR_ARG), bad
    assert check(H, margin=0.0)[:2] == (OK, 0)
    assert check(H, cap=-1)[:2] == (BAD_CAP, ERR_ARG) and check(H, cap=101)[:2] == (BAD_CAP, ERR_ARG)
    # partials above 1 GiB: tiles x cap x 32 bytes
    n = 1 << 20
    tiles = -(-n // tile)
    cap_ok = (1 << 30) // (32 * tiles)
    assert check(H, n=n, m=0, cap=cap_ok) == (OK, 0, cap_ok, tiles * cap_ok * 32)
    assert check(H, n=n, m=0, cap=cap_ok + 1)[:3] == (TOO_LARGE, ERR_ARG, cap_ok + 1)
    assert check(H, n=1 << 24, m=0, cap=0)[:2] == (TOO_LARGE, ERR_ARG)      # 32768 tiles x 4096 x 32 bytes = 4 GiB
    # going off reads neither the margin nor the cap, but still needs tables and a finished step
    assert check(H, on=0, margin=float('nan'), cap=-5)[:2] == (OK, 0)
    assert check(H, on=0, tables=0)[:2] == (NO_TABLES, ERR_STATE) and check(H, on=0, mid_step=1)[:2] == (MID_STEP, ERR_STATE)


def test_every_outcome_of_the_getters_checks(H):
    z = sizes(H)

    def g(tables=1, ever=1, n=10, begin=0, count=10, have_outputs=1, have_out=1, struct_bytes=int(z[0])):
        out = np.zeros(4, np.int32)
        H.mg_getter_checks(tables, ever, n, begin, count, have_outputs, have_out, struct_bytes, vp(out))
        return tuple(int(v) for v in out)
    assert g() == (OK, 0, OK, 0)
    assert g(tables=0) == (NO_TABLES, ERR_STATE, NO_TABLES, ERR_STATE)
    assert g(ever=0) == (NEVER_SET, ERR_STATE, NEVER_SET, ERR_STATE)
    for kw in (dict(begin=-1), dict(count=-1), dict(begin=11, count=0), dict(begin=4, count=7), dict(have_outputs=0)):
        assert g(**kw)[:2] == (GET_ARGS, ERR_ARG), kw
    assert g(begin=10, count=0, have_outputs=0)[:2] == (OK, 0)
    assert g(have_out=0)[2:] == (GET_ARGS, ERR_ARG) and g(struct_bytes=56)[2:] == (GET_ARGS, ERR_ARG)


def test_the_struct_the_verdict_and_the_symbols(H):
    from sca_amd import _lib
    z = sizes(H)
    assert z[0] == 64 == C.sizeof(_lib.MissionGateTotals) and z[1] == GR.OVER_CAP == 4 and z[2] == GR.SPAWN_BATCH and z[5] == 8 and z[6] == 1024
    assert tuple(k for k, _ in _lib.MissionGateTotals._fields_) == GR.GATE_TOTALS + ('reserved',)
    hdr = open(os.path.join(harness_util.ROOT, 'include', 'sca_hip.h')).read()
    for name in ('sca_set_mission_gate', 'sca_get_mission_gate_state', 'sca_get_mission_gate_totals'):
        assert re.search(r'\bint %s\(' % name, hdr) and name in _lib.SIGNATURES, name
    assert re.search(r'\bSCA_SPAWN_OVER_CAP = SCA_SPAWN_BLOCKED_ENTRY \+ 1\b', hdr)                   # (4: mg_sizes above has the compiled value)
    assert 'The admission gate stays a host call' not in hdr
    import sca_amd.solver as S
    assert S.SPAWN_OVER_CAP == 4
    for name in ('set_mission_gate', 'mission_gate_state', 'mission_gate_totals'):
        assert callable(getattr(S.BatchedSolver, name)), name


# ---- place, query, settle ------------------------------------------------------------------------------------------------------------------
def test_place_query_settle_against_the_rule(H):
    assert [H.mg_class(w, f) for w, f in ((-1, 0), (-1, 1), (0, 0), (2, 0), (0, 1), (5, 1))] == [0, 0, 1, 1, 2, 2]
    for wt in (0, 1, 7, 300):
        for rank in (0, 1, 63, 64, 1000):
            assert H.mg_place(1, rank, wt) == GR.place(False, rank, wt) == rank
            assert H.mg_place(2, rank, wt) == GR.place(True, rank, wt) == wt + rank
    rng = np.random.default_rng(5)
    e = np.zeros(4, MR.MISSION)
    e['pos'] = rng.uniform(-5, 5, (4, 3))
    e['flags'] = [0, MR.START_HERE, MR.KEEP_ZAXIS, MR.START_HERE | MR.KEEP_ZAXIS]
    pos = rng.uniform(-5, 5, 3)
    T = GR.GatedTables(e.reshape(1, 4), [0], [0], 0.5)
    for j in range(4):
        out = np.zeros(4)
        H.mg_query(C.c_void_p(e.ctypes.data + j * e.itemsize), vp(pos), 0.37, vp(out))
        assert np.array_equal(out[:3], T.query(0, j, dict(pos=pos[None, :]))) and out[3] == 0.37, j
        assert np.array_equal(out[:3], pos if j % 2 else e['pos'][j])
    for v in range(5):
        for entry in (0, 2, 126):
            for refusals in (0, 3):
                out = np.zeros(5, np.int32)
                H.mg_settle(v, entry, refusals, vp(out))
                w, word, ref, name, take = GR.settle(v, entry, refusals)
                assert tuple(out[:3]) == (w, word, ref) and GR.GATE_TOTALS[out[3]] == name and bool(out[4]) == take, (v, entry, refusals, out)
    assert GR.settle(0, 2, 3) == (-1, 0, 3, 'admitted', True) and GR.settle(4, 2, 3) == (2, 4, 4, 'over_cap', False)


def step_through_harness(H, run, st, T, cap):
    """one step of the run through mg_step, from the rule's words in FRONT of the step's gate; returns what the harness leaves"""
    n = len(T['waiting'])
    saw = st['saw']
    waiting, verdict, refusals = T['waiting'].copy(), T['verdict'].copy(), T['refusals'].copy()
    fresh = np.zeros(n, np.int32)
    for a, j in saw['order'][saw['n_waiting']:]:
        fresh[a], waiting[a] = 1, j
    room = max(1, saw['tested'])
    ids, ent, ver = np.full(room, -7, np.int32), np.full(room, -7, np.int32), np.full(room, -7, np.int32)
    probe = np.zeros(room, MR.CLEAR)
    totals = np.zeros(8, np.uint64)
    es = st['ended_state']
    pos, radius = np.ascontiguousarray(es['pos'], np.float64), np.ascontiguousarray(st['defs']['radius'], np.float64)
    entries = np.ascontiguousarray(run['entries'])
    sc = run['scene']
    got = H.mg_step(n, MR.M, vp(entries), vp(pos), vp(radius), len(sc['obs_radius']), vp(np.ascontiguousarray(sc['obs_pos'], np.float64)),
                    vp(np.ascontiguousarray(sc['obs_radius'], np.float64)), GR.MARGIN, cap, vp(waiting), vp(verdict), vp(refusals), vp(fresh), vp(ids), vp(ent), vp(ver),
                    vp(probe), vp(totals))
    return got, waiting, verdict, refusals, ids, ent, ver, probe, totals


@pytest.mark.parametrize('cap', [0, 8])
def test_a_steps_gate_against_the_python_rule_on_the_corpus(H, oracle, cap):
    """the host-compiled tiles' counts, places, probe, gate walk and settle (the functions the kernels call, in the kernels' order) against
    mission_gate_rule step by step: the list in offer order, the verdicts, the world records, the words and the counters"""
    steps = 0
    for seed in MR.SEEDS[::3]:
        scene = F.random_scene(seed)
        run = dict(GR.oracle_run(oracle, scene, cap=cap), scene=scene)
        n = scene['n']
        T = dict(waiting=np.full(n, -1, np.int32), verdict=np.zeros(n, np.int32), refusals=np.zeros(n, np.int32))
        tot = dict.fromkeys(GR.GATE_TOTALS, 0)
        for t, st in enumerate(run['steps']):
            saw = st['saw']
            at = (seed, t, cap)
            got, waiting, verdict, refusals, ids, ent, ver, probe, totals = step_through_harness(H, run, st, T, run['cap'])
            assert got == len(saw['order']), at
            k = saw['tested']
            assert [(int(a), int(j)) for a, j in zip(ids[:k], ent[:k])] == saw['order'][:k], at
            assert np.array_equal(ver[:k], saw['verdict']), at
            if k:
                assert probe[:k].tobytes() == np.ascontiguousarray(saw['probe']).astype(MR.CLEAR).tobytes(), at
            assert np.array_equal(waiting, st['waiting']) and np.array_equal(verdict, st['verdict']) and np.array_equal(refusals, st['refusals']), at
            for i, name in enumerate(GR.GATE_TOTALS):
                tot[name] += int(totals[i])
            assert tot == st['gate_totals'], at + (tot, st['gate_totals'])
            T = dict(waiting=st['waiting'], verdict=st['verdict'], refusals=st['refusals'])
            steps += bool(saw['order'])
    assert steps > 50, steps


# ---- the harness as a program under the sanitizers ---------------------------------------------------------------------------------------
def test_standalone_under_sanitizers():
    """The rules as a program of their own (its main draws tables, records and obstacles into heap arrays of exactly their size, lets rows
    end, and runs the step's gate with lists of exactly min(candidates, cap) entries and partials of exactly tiles x cap records) under
    -fsanitize=address,undefined.  Host code only; nothing of it is loaded into python."""
    exe = os.path.join(harness_util.BUILD, 'mission_gate_harness_san')
    os.makedirs(harness_util.BUILD, exist_ok=True)
    subprocess.check_call(['g++', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan',
                           '-DMISSION_GATE_MAIN'] + FLAGS + ['-o', exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'mission_gate_harness: ok' in r.stdout


# ---- what the corpus holds -----------------------------------------------------------------------------------------------------------------
# the fuzz scenes of seeds 0 .. 39 x 12 steps with mission_rule.draw_tables at margin 0.5
CORPUS = dict(steps_with_candidates=248, steps_all=6, steps_part=122, steps_none=120,
              new_admitted=536, new_blocked_agent=4130, new_blocked_obstacle=132, new_blocked_entry=375, new_over_cap=0,
              wait_admitted=149, wait_admitted_after_refusals=415, wait_blocked_agent=47955, wait_blocked_obstacle=1400, wait_blocked_entry=162, wait_over_cap=0,
              chains=575, here_admitted=145, here_refused=29363, waiting_at_end=4488, scenes_wait_admitted=14, scenes_wait_blocked_entry=2, overtaken=0)
CORPUS_CAP8 = dict(steps_with_candidates=248, steps_all=6, steps_part=73, steps_none=169,
                   new_admitted=77, new_blocked_agent=95, new_blocked_obstacle=14, new_blocked_entry=1, new_over_cap=4820,
                   wait_admitted=79, wait_admitted_after_refusals=178, wait_blocked_agent=1430, wait_blocked_obstacle=177, wait_blocked_entry=0, wait_over_cap=51673,
                   chains=2, here_admitted=40, here_refused=1110, waiting_at_end=4851, scenes_wait_admitted=13, scenes_wait_blocked_entry=0, overtaken=0)
NEVER = {0: ('new_over_cap', 'wait_over_cap', 'overtaken'), 8: ('wait_blocked_entry', 'scenes_wait_blocked_entry', 'overtaken')}


def corpus_total(oracle, cap):
    total = dict.fromkeys(GR.CLASSES, 0)
    for seed in MR.SEEDS:
        c = GR.corpus_counts(GR.oracle_run(oracle, F.random_scene(seed), cap=cap))
        for k in total:
            total[k] += c[k]
    return total


def test_what_the_corpus_holds(oracle):
    """counted from the oracle's records and the Python rule alone: every class the gate distinguishes occurs"""
    total = corpus_total(oracle, 0)
    assert all(v > 0 for k, v in total.items() if k not in NEVER[0]), total
    assert total == CORPUS, total


def test_what_the_corpus_holds_at_a_cap_of_8(oracle):
    """max_per_step = 8: rows wait over the cap, new and waiting ones, and no tested waiting row stands behind a new one"""
    total = corpus_total(oracle, 8)
    assert total['new_over_cap'] > 0 and total['wait_over_cap'] > 0 and total['overtaken'] == 0, total
    assert all(v > 0 for k, v in total.items() if k not in NEVER[8]), total
    assert total == CORPUS_CAP8, total


def test_the_rule_keeps_its_invariants(oracle):
    """offered == admitted + blocked_* + over_cap, and endings == taken + stopped + dropped + waiting, behind every step"""
    for cap in (0, 8):
        for seed in MR.SEEDS[:12]:
            for st in GR.oracle_run(oracle, F.random_scene(seed), cap=cap)['steps']:
                g, t = st['gate_totals'], st['totals']
                assert g['offered'] == sum(g[k] for k in GR.VERDICT_TOTAL)
                assert g['admitted'] == t['taken']
                assert t['arrived'] + t['collided'] + t['timed_out'] == t['taken'] + t['stopped'] + g['dropped'] + int((st['waiting'] >= 0).sum())
                assert not ((st['waiting'] >= 0) & ((st['flags'] & 7) == 0)).any()       # who waits is finished
    assert SR.ADMITTED == 0
