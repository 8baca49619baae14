"""Vacant rows in a plain context without a GPU: the pure rules of sca_amd/csrc/sca_vacancy.h compiled for the host behind
tests/vacancy_harness.cpp -- every outcome of vacancy_check with its code, the row rule k_vacate calls per lane against the Python rule of
tests/vacancy_rule.py, the tiled permutation edit at tile sizes 256 and 64 against Python's list.remove / append, the mode and plan rows of
sca_forms.h with vacancy_on -- the harness as a program of its own under the sanitizers, the symbols, and what the corpus holds (counted from
the oracle and the rule alone)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import form_fuzz as F
import harness_util
import vacancy_rule as V

SRC = os.path.join(harness_util.ROOT, 'tests', 'vacancy_harness.cpp')
FLAGS = ['-std=c++17', '-ffp-contract=off', '-mfma', '-fno-builtin-pow', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I' + harness_util.CSRC]
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5                   # include/sca_hip.h
(OK, NO_AGENTS, NO_STATE, MID_STEP, BAD_COUNT, NO_IDS, BAD_ID, REPEATED_ID, ALREADY_VACANT, LAST_ROW, LIST_ARGS, SCENES, SHARD, COMM, PARTITION,
 PATH_BLOCK) = range(16)                                           # VacancyFault
CTX_KEYS = ('agents', 'state', 'mid_step', 'scenes', 'comm', 'partition', 'n', 'shard_count', 'tracker_on', 'paths_block', 'path_W')
KEEP, TAIL, ADMIT = 0, 1, 2                                        # VacMode
HEADERS = ('sca_vacancy.h', 'sca_respawn.h', 'sca_scenes.h', 'sca_core.h', 'sca_forms.h', 'sca_glibc_math.h', 'sca_glibc_tables.h', 'sca_constants.h')


@pytest.fixture(scope='module')
def H():
    out = os.path.join(harness_util.BUILD, 'libvacancy_harness.so')
    deps = [SRC, os.path.join(harness_util.ROOT, 'include', 'sca_hip.h')] + [os.path.join(harness_util.CSRC, f) for f in HEADERS]
    os.makedirs(harness_util.BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(['g++', '-O2', '-fPIC', '-shared'] + FLAGS + ['-o', out, SRC])
    h = C.CDLL(out)
    for f in (h.vac_check, h.vac_list_check, h.vac_vacate, h.vac_plan_auto, h.vac_plan_step):
        f.restype = None
    h.vac_check.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    h.vac_list_check.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    h.vac_vacate.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 20
    h.vac_compact.restype = C.c_int
    h.vac_compact.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    h.vac_plan_auto.argtypes = [C.c_int] * 9 + [C.c_void_p]
    h.vac_plan_step.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    h.vac_finished_listed.restype = C.c_int
    h.vac_finished_listed.argtypes = [C.c_uint]
    return h


def p(a):
    return None if a is None else a.ctypes.data


def ctx(**kw):
    c = dict(agents=1, state=1, mid_step=0, scenes=0, comm=0, partition=0, n=8, shard_count=8, tracker_on=0, paths_block=0, path_W=0)
    c.update(kw)
    return np.array([c[k] for k in CTX_KEYS], np.int32)


def check(H, c, vacant, occupied, ids, count=None):
    out = np.zeros(3, np.int32)
    ids = None if ids is None else np.asarray(ids, np.int32)
    vac = None if vacant is None else np.asarray(vacant, np.uint8)
    H.vac_check(p(c), p(vac), occupied, len(ids) if count is None else count, p(ids), p(out))
    return tuple(int(x) for x in out)


# ---- the refusals --------------------------------------------------------------------------------------------------------------------------
def test_every_outcome_of_vacancy_check(H):
    ok = [1, 2]
    assert check(H, ctx(), None, 8, ok) == (OK, -1, 0)
    for kw, fault, code in ((dict(agents=0), NO_AGENTS, ERR_STATE), (dict(state=0), NO_STATE, ERR_STATE), (dict(mid_step=1), MID_STEP, ERR_STATE),
                            (dict(scenes=1), SCENES, ERR_UNSUPPORTED), (dict(comm=1), COMM, ERR_UNSUPPORTED), (dict(partition=1), PARTITION, ERR_UNSUPPORTED),
                            (dict(shard_count=4), SHARD, ERR_UNSUPPORTED), (dict(paths_block=1), PATH_BLOCK, ERR_UNSUPPORTED)):
        assert check(H, ctx(**kw), None, 8, ok) == (fault, -1, code), kw
    assert check(H, ctx(), None, 8, ok, count=0) == (BAD_COUNT, -1, ERR_ARG)
    assert check(H, ctx(), None, 8, ok, count=-3) == (BAD_COUNT, -1, ERR_ARG)
    assert check(H, ctx(), None, 8, None, count=2) == (NO_IDS, -1, ERR_ARG)
    assert check(H, ctx(), None, 8, [1, 8]) == (BAD_ID, 1, ERR_ARG)
    assert check(H, ctx(), None, 8, [-1, 2]) == (BAD_ID, 0, ERR_ARG)
    assert check(H, ctx(), None, 8, [5, 2, 7, 2, 5]) == (REPEATED_ID, 3, ERR_ARG)
    vac = np.zeros(8, np.uint8)
    vac[[2, 6]] = 1
    assert check(H, ctx(), vac, 6, [1, 6]) == (ALREADY_VACANT, 1, ERR_ARG)
    assert check(H, ctx(), vac, 6, [0, 1, 3, 4, 5, 7]) == (LAST_ROW, -1, ERR_ARG)
    assert check(H, ctx(), vac, 6, [0, 1, 3, 4, 5]) == (OK, -1, 0)
    assert check(H, ctx(), None, 8, list(range(8))) == (LAST_ROW, -1, ERR_ARG)
    assert check(H, ctx(n=1, shard_count=1), None, 1, [0]) == (LAST_ROW, -1, ERR_ARG)
    # the order: the context before the call's arguments, an id before a repeat before a vacancy before the last row
    assert check(H, ctx(state=0, scenes=1), None, 8, [9], count=0)[0] == NO_STATE
    assert check(H, ctx(), vac, 6, [2, 9])[0] == BAD_ID and check(H, ctx(), vac, 6, [2, 2])[0] == REPEATED_ID
    # a mid-step getter is legal, a mid-step retire is not; the getter's own arguments
    out = np.zeros(3, np.int32)
    for args, want in (((1, 4, 1), (OK, 0)), ((0, 0, 1), (OK, 0)), ((0, 4, 1), (LIST_ARGS, ERR_ARG)), ((1, -1, 1), (LIST_ARGS, ERR_ARG)), ((1, 4, 0), (LIST_ARGS, ERR_ARG))):
        H.vac_list_check(p(ctx(mid_step=1)), *args, p(out))
        assert (int(out[0]), int(out[2])) == want, args
    H.vac_list_check(p(ctx(scenes=1)), 1, 4, 1, p(out))
    assert (int(out[0]), int(out[2])) == (SCENES, ERR_UNSUPPORTED)
    H.vac_list_check(p(ctx(state=0)), 1, 4, 1, p(out))
    assert (int(out[0]), int(out[2])) == (NO_STATE, ERR_STATE)


def test_a_vacant_row_has_not_finished(H):
    for f in range(16):
        assert H.vac_finished_listed(f) == int((f & 7) != 0 and not f & 8), f


# ---- the row rule --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slots,clear', [(False, False), (True, True)])
def test_the_row_rule_against_the_python_rule(H, slots, clear):
    """k_vacate's per-lane body on host arrays against vacancy_rule.retire: the named rows' state words, and that every other word of
    every row stays; done_delta is -1 exactly for the rows that were live"""
    rng = np.random.default_rng(4)
    for n in (1, 5, 64, 300):
        flags = ((rng.random(n) < 0.4) * rng.choice([1, 2, 4, 3], n)).astype(np.uint8)
        st = dict(pos=rng.normal(0, 5, (n, 3)), vel=rng.normal(0, 1, (n, 3)).astype(np.float32), heading=rng.normal(0, 1, (n, 3)), flags=flags,
                  total_dist=rng.uniform(0, 9, n), step_num=rng.integers(0, 50, n).astype(np.int32))
        radius = rng.choice([0.3, 0.5], n)
        action, diag = rng.normal(0, 1, (n, 8)).astype(np.float32), rng.integers(0, 9, (n, 8)).astype(np.int32)
        status, nbr_n, near_n = (rng.integers(1, 5, n).astype(np.int32) for _ in range(3))
        nbr_valid = np.ones(n, np.uint8)
        now_goal, plen, prem = rng.normal(0, 1, (n, 3)), rng.integers(1, 4, n).astype(np.int32), rng.integers(0, 2, n).astype(np.int32)
        ca, cp = rng.uniform(0, 3, n), rng.integers(0, n, n).astype(np.int32)
        ids = rng.permutation(n)[:max(1, n // 3)].astype(np.int32)
        want = {k: v.copy() for k, v in st.items()}
        V.retire(want, np.arange(n, dtype=np.int32), np.zeros(n, bool), ids)
        held = dict(radius=radius.copy(), action=action.copy(), diag=diag.copy(), status=status.copy(), nbr_n=nbr_n.copy(), near_n=near_n.copy(), nbr_valid=nbr_valid.copy(),
                    now_goal=now_goal.copy(), plen=plen.copy(), prem=prem.copy(), ca=ca.copy(), cp=cp.copy())
        got = {k: v.copy() for k, v in st.items()}
        delta = np.zeros(len(ids), np.int32)
        H.vac_vacate(n, len(ids), p(ids), p(got['pos']), p(got['vel']), p(got['flags']), p(radius), p(got['heading']), p(got['total_dist']), p(action), p(diag),
                     p(got['step_num']), p(status), p(nbr_n), p(near_n), p(nbr_valid), p(now_goal) if slots else None, p(plen) if slots else None,
                     p(prem) if slots else None, p(ca) if clear else None, p(cp) if clear else None, p(delta))
        for k in F.STATE_KEYS:
            assert np.array_equal(got[k], want[k]), (n, k)
        assert np.array_equal(delta, -((flags[ids] & 7) == 0).astype(np.int32)), n
        others = np.setdiff1d(np.arange(n), ids)
        assert np.array_equal(radius, held['radius'])
        for name, arr in (('action', action), ('diag', diag), ('status', status), ('nbr_n', nbr_n), ('near_n', near_n), ('nbr_valid', nbr_valid), ('now_goal', now_goal),
                          ('plen', plen), ('prem', prem), ('ca', ca), ('cp', cp)):
            assert np.array_equal(arr[others], held[name][others]), (n, name, 'another row was written')
        assert not action[ids][:, :7].any() and np.array_equal(action[ids][:, 7], held['action'][ids][:, 7]) and (diag[ids] == -1).all()
        assert not status[ids].any() and not nbr_n[ids].any() and not nbr_valid[ids].any() and (near_n[ids] == -1).all()
        if slots:
            assert np.isnan(now_goal[ids]).all() and not plen[ids].any() and not prem[ids].any()
        else:
            assert np.array_equal(now_goal, held['now_goal']) and np.array_equal(plen, held['plen'])
        if clear:
            assert np.isinf(ca[ids]).all() and (cp[ids] == -1).all()
        else:
            assert np.array_equal(ca, held['ca'])


# ---- the permutation edit ------------------------------------------------------------------------------------------------------------------
def compact(H, tile, mode, flags, perm, n, m, out, base, ids=None, verdict=None):
    ids = None if ids is None else np.ascontiguousarray(ids, np.int32)
    verdict = None if verdict is None else np.ascontiguousarray(verdict, np.int32)
    return H.vac_compact(tile, mode, p(flags), p(perm), p(ids), p(verdict), n, m, 0 if ids is None else len(ids), p(out), base)


@pytest.mark.parametrize('tile', (256, 64))
def test_the_tiled_edit_against_the_list_edit(H, tile):
    """retire: list.remove of the named ids, the vacant ids ascending behind the prefix; admit: list.append in call order under a verdict.
    Position counts either side of a tile, and 0 (a pure tail rewrite), 1 and all-but-one rows named"""
    rng = np.random.default_rng(tile)
    for n in sorted({1, 2, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1, 5 * tile + 7}):
        for named in sorted({0, 1, n // 2, n - 1}):
            if named >= n:
                continue
            perm = rng.permutation(n).astype(np.int32)
            flags = ((rng.random(n) < 0.3) * rng.choice([1, 2, 4], n)).astype(np.uint8)
            ids = rng.permutation(n)[:named].astype(np.int32)
            # -- the retire
            flags[ids] = V.VACANT
            want = [int(a) for a in perm]
            for a in ids:
                want.remove(int(a))
            want += sorted(int(a) for a in ids)
            tmp, got = np.full(n, -7, np.int32), perm.copy()
            kept = compact(H, tile, KEEP, flags, perm, n, n, tmp, 0)
            assert kept == n - named and (tmp[kept:] == -7).all()
            tail = compact(H, tile, TAIL, flags, perm, n, n, got, kept)
            got[:kept] = tmp[:kept]
            assert kept + tail == n and got.tolist() == want, (n, named)
            # -- an admission of half of them and of occupied rows, shuffled, a third refused by the verdict
            perm, m = got, kept
            call = rng.permutation(n)[:max(1, (n + 1) // 2)].astype(np.int32)
            verdict = (rng.random(len(call)) < 0.33).astype(np.int32) * rng.choice([1, 2, 3], len(call)).astype(np.int32)
            for use in (None, verdict):
                ok = np.ones(len(call), bool) if use is None else use == 0
                admitted = [int(a) for a, v in zip(call, ok) if v and flags[a] & 8]
                want = perm[:m].tolist() + admitted
                after = flags.copy()
                after[admitted] = 0
                want += [int(a) for a in np.flatnonzero(after & 8)]
                got = perm.copy()
                k = compact(H, tile, ADMIT, flags, perm, n, m, got, m, call, use)
                assert k == len(admitted)
                tail = compact(H, tile, TAIL, after, perm, n, m, got, m + k)
                assert m + k + tail == n and got.tolist() == want, (n, named, use is None)


# ---- the mode and the plan -----------------------------------------------------------------------------------------------------------------
def test_mode_resolution_and_plan_step_with_vacancy_on(H):
    out = np.zeros(4, np.int32)
    for fits in (0, 1):
        for tracked in (0, 1):
            for backoff in (0, 3):
                for last in (-1, 0, 5000):
                    base = np.zeros(4, np.int32)
                    H.vac_plan_auto(fits, tracked, 0, last, 8, backoff, 4096, 0, 0, p(base))
                    H.vac_plan_auto(fits, tracked, 0, last, 8, backoff, 4096, 0, 1, p(out))
                    assert np.array_equal(out, base), 'vacancy_on = false is the defaulted form'
                    H.vac_plan_auto(fits, tracked, 0, last, 8, backoff, 4096, 1, 1, p(out))
                    assert out[0] == 0 and out[3] == 0, 'no AUTO pass, and none planned ahead, while a row is vacant'
                    assert out[1] == backoff and out[2] == last, 'the back-off is not touched'
    H.vac_plan_auto(1, 0, 0, 0, 8, 0, 4096, 0, 1, p(out))
    assert out[0] == 1 and out[3] == 1
    # plan_step: SCA_NBR_AUTO with another step to follow and everything that lets both events ride
    i = np.array([3, 0, 4, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 8, 0, 4096, 0], np.int32)
    o = np.zeros(3, np.int32)
    H.vac_plan_step(p(i), 0, 0, p(o))
    assert o.tolist() == [1, 1, 0]
    H.vac_plan_step(p(i), 0, 1, p(o))
    assert o.tolist() == [1, 1, 0]
    H.vac_plan_step(p(i), 1, 1, p(o))
    assert o.tolist() == [0, 0, 0]
    i[0], i[7], i[8], i[9] = 0, 1, 1, 1                                   # kd mode with the tracker in the pass: the fork still rides
    H.vac_plan_step(p(i), 1, 1, p(o))
    assert o.tolist() == [0, 0, 1]


# ---- the harness as a program under the sanitizers --------------------------------------------------------------------------------------
def test_standalone_under_sanitizers():
    """The rules as a program of their own (its main retires and admits random rows of heap arrays of exactly n rows and edits the
    permutation at both tile sizes) under -fsanitize=address,undefined.  Host code only; nothing of it is loaded into python."""
    exe = os.path.join(harness_util.BUILD, 'vacancy_harness_san')
    os.makedirs(harness_util.BUILD, exist_ok=True)
    subprocess.check_call(['g++', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan',
                           '-DVACANCY_MAIN'] + FLAGS + ['-o', exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'vacancy_harness: ok' in r.stdout


# ---- the symbols ---------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_and_the_flag():
    hdr = open(os.path.join(harness_util.ROOT, 'include', 'sca_hip.h')).read()
    for sym in ('sca_retire_agents', 'sca_get_vacant', 'sca_get_population'):
        assert re.search(r'\bint %s\(sca_ctx \*ctx' % sym, hdr), sym
    assert re.search(r'SCA_FLAG_VACANT = 8\b', hdr) and re.search(r'#define SCA_FORM_VACANCY 2048\b', hdr)
    from sca_amd import _lib
    import sca_amd.solver as S
    for sym in ('sca_retire_agents', 'sca_get_vacant', 'sca_get_population'):
        assert sym in _lib.SIGNATURES
    assert S.FLAG_VACANT == 8 and S.FORM_VACANCY == 2048 and V.VACANT == 11
    for name in ('retire', 'vacant', 'population'):
        assert callable(getattr(S.BatchedSolver, name))


# ---- what the corpus holds -----------------------------------------------------------------------------------------------------------------
def test_what_the_corpus_holds(oracle):
    """counted from the rule and the oracle alone; a condition, not a measurement: the GPU tests leave out no occupied row and no step"""
    total = dict.fromkeys(V.QUANTITIES, 0)
    for seed in V.SEEDS:
        scene = F.random_scene(seed)
        run = V.oracle_run(oracle, scene)
        assert len(run) == V.STEPS
        for st in run:
            m = int((~st['vacant']).sum())
            assert m >= 1 and sorted(st['perm'][:m].tolist()) == np.flatnonzero(~st['vacant']).tolist()
            assert st['perm'][m:].tolist() == np.flatnonzero(st['vacant']).tolist()
            assert (st['flags'][st['vacant']] == V.VACANT).all() and not (st['flags'][~st['vacant']] & 8).any()
        for k, v in V.corpus_counts(scene, run).items():
            total[k] += v
    for k in V.QUANTITIES:
        assert total[k] > 0, (k, total)
    # the figures the README quotes: the corpus is seeded, so they are exact
    assert total == dict(retired_finished=13310, retired_live=7017, admissions=14694, respawns=12604, repeats=13152, list_entries=119770, retired_tracked=6701,
                         retired_lp=3402, steps_below_half=72, single_leaf=10, admitted_collisions=15184, mixed_calls=224), total
    from sca_amd import _lib                                               # (what the corpus is for: the entry points it is run through)
    assert 'sca_retire_agents' in _lib.SIGNATURES
