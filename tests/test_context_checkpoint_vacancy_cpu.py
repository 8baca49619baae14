"""Context checkpoints with vacant rows, without a GPU (sca_checkpoint.h behind tests/context_checkpoint_vacancy_harness.cpp): every fault
the check gains with vacancy allowed, with its code and entry, at 1 / 63 / 64 / 65 / 257 rows; the answers the check gives WITHOUT the flag
on the same blobs, which are today's; the byte identity of a blob without vacant rows; the load's row move over plain arrays (save -> load
into zeroed arrays -> save reproduces the blob, the vacant rows' outputs are vacate_write_row's); and what the GPU corpus holds at its
three save points.  Expectations are literals worked out from include/sca_hip.h and sca_vacancy.h's contract -- none comes from the code
under test.  The harness then runs as a program of its own under AddressSanitizer and UBSan, every blob in a buffer of exactly its size."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import form_fuzz as F
import vacancy_rule as V
from harness_util import BUILD, CSRC, ROOT
from test_context_checkpoint_cpu import (BLOCK, CXXFLAGS, ERR_ARG, FLAGS, FULL, HEADER_RANGE, NONE, OK, POL, SEC, SLOTS, TRK_WORDS, damaged, shape8, vp, want_layout)

SRC = os.path.join(ROOT, 'tests', 'context_checkpoint_vacancy_harness.cpp')
VACANT_FLAGS, VACANT_COUNT, VACANT_PERM, VACANT_BLOCK, VACANT_WORDS = range(28, 33)      # appended to CtxFault: the numbers before them are pinned
HAS_VACANCY = 32
PRESENT_AT, OCCUPIED_AT = 24, 52                                    # the header's `present` word and the word that was reserved


@pytest.fixture(scope='module')
def H():
    out = os.path.join(BUILD, 'libcontext_checkpoint_vacancy_harness.so')
    deps = [SRC, os.path.join(ROOT, 'tests', 'context_checkpoint_harness.cpp'), os.path.join(ROOT, 'include', 'sca_hip.h')] + \
           [os.path.join(CSRC, f) for f in ('sca_checkpoint.h', 'sca_vacancy.h', 'sca_respawn.h', 'sca_scenes.h', 'sca_core.h', 'sca_dubins.hpp', 'sca_constants.h')]
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(['g++', '-O2', '-fPIC', '-shared'] + CXXFLAGS + ['-o', out, SRC])
    h = C.CDLL(out)
    h.cx_make.restype = C.c_int64
    h.cxv_make.restype = C.c_int64
    return h


def shape_for(n, **s):
    return dict(FULL, n=n, **s)


def policy_for(n):
    return np.resize(POL, n).astype(np.uint8)


def make(H, vacant, **s):
    n = len(vacant)
    s = shape_for(n, **s)
    total = want_layout(**s)[1]
    blob = np.zeros(total, np.uint8)
    assert H.cxv_make(vp(shape8(**s)), vp(policy_for(n)), vp(np.ascontiguousarray(vacant, np.uint8)), vp(blob)) == total
    return blob


def check(H, blob, allow, ctx=True, block_len=None, **s):
    n = s.pop('n')
    s = shape_for(n, **s)
    exact = np.ascontiguousarray(blob).copy()
    bl = None if block_len is None else np.ascontiguousarray(block_len, np.int32)
    out = (C.c_int64 * 2)()
    rc = H.cxv_check(vp(exact), C.c_int64(len(exact)), 1 if allow else 0, 1 if ctx else 0, vp(shape8(**s)), vp(policy_for(n)), None if bl is None else vp(bl), 0, out)
    return out[0], out[1], rc


def word(v):
    return [(k, (v >> (8 * k)) & 255) for k in range(4)]


def put(at, v):
    return [(at + k, b) for k, b in word(v & 0xffffffff)]


def vacant_mask(n):
    """every third row from row 1 on, and the last row: vacant rows either side of every boundary of the sizes; n >= 2"""
    v = np.zeros(n, np.uint8)
    v[1::3] = 1
    v[n - 1] = 1
    if v.all():
        v[0] = 0
    return v


def test_the_new_faults_are_appended(H):
    out = (C.c_int * 5)()
    assert H.cxv_faults(out) == HAS_VACANCY and list(out) == [VACANT_FLAGS, VACANT_COUNT, VACANT_PERM, VACANT_BLOCK, VACANT_WORDS]


# ---- the faults ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [63, 64, 65, 257])
def test_every_new_fault_with_its_code_and_entry(H, n):
    vac = vacant_mask(n)
    ids, occ = np.flatnonzero(vac), np.flatnonzero(vac == 0)
    m = len(occ)
    blob = make(H, vac)
    off = want_layout(**shape_for(n))[0]
    rec, perm = off[SEC['rec']], off[SEC['perm']]
    for ctx in (True, False):
        assert check(H, blob, True, ctx=ctx, n=n) == (OK, -1, 0)
    last = int(ids[-1])

    def bad(edits, allow=True, **kw):
        return check(H, damaged(H, blob, edits), allow, n=n, **kw)
    # the header: the bit with occupied outside 1 .. n-1, occupied without the bit, the bit where it is not allowed
    assert bad(put(OCCUPIED_AT, 0)) == (HEADER_RANGE, -1, ERR_ARG)
    assert bad(put(OCCUPIED_AT, n)) == (HEADER_RANGE, -1, ERR_ARG)
    assert bad(put(OCCUPIED_AT, -1)) == (HEADER_RANGE, -1, ERR_ARG)
    assert bad([(PRESENT_AT, 31)]) == (HEADER_RANGE, -1, ERR_ARG)
    assert bad([(PRESENT_AT, 127)]) == (HEADER_RANGE, -1, ERR_ARG)
    assert check(H, blob, False, n=n) == (HEADER_RANGE, -1, ERR_ARG)
    # a vacant bit on a flag word that is not 11 (the first such row is named); bit 16 stays unknown
    assert bad([(rec + 48 * last + 36, 9)]) == (VACANT_FLAGS, last, ERR_ARG)
    assert bad([(rec + 48 * int(occ[0]) + 36, 8)]) == (VACANT_FLAGS, int(occ[0]), ERR_ARG)
    assert bad([(rec + 48 * last + 36, 27)]) == (FLAGS, last, ERR_ARG)
    # the count: the header says one more or one less, or an occupied row reads 11
    assert bad(put(OCCUPIED_AT, m - 1)) == (VACANT_COUNT, -1, ERR_ARG)
    assert bad(put(OCCUPIED_AT, m + 1) if m + 1 < n else put(OCCUPIED_AT, m - 1)) == (VACANT_COUNT, -1, ERR_ARG)
    assert bad([(rec + 48 * int(occ[0]) + 36, 11)]) == (VACANT_COUNT, -1, ERR_ARG)
    # the permutation: a vacant id in the prefix (swapped with an occupied one: still a permutation), the tail not ascending
    p0, pm = int(np.frombuffer(blob[perm:perm + 4].tobytes(), np.int32)[0]), int(np.frombuffer(blob[perm + 4 * m:perm + 4 * m + 4].tobytes(), np.int32)[0])
    assert pm == ids[0] and p0 == occ[-1]
    assert bad(put(perm, pm) + put(perm + 4 * m, p0)) == (VACANT_PERM, 0, ERR_ARG)
    mid = m // 2
    pmid = int(np.frombuffer(blob[perm + 4 * mid:perm + 4 * mid + 4].tobytes(), np.int32)[0])
    assert bad(put(perm + 4 * mid, pm) + put(perm + 4 * m, pmid)) == (VACANT_PERM, mid, ERR_ARG)
    assert bad(put(perm + 4 * m, int(ids[1])) + put(perm + 4 * (m + 1), int(ids[0]))) == (VACANT_PERM, m, ERR_ARG)
    assert bad(put(perm + 4 * (n - 2), int(ids[-1])) + put(perm + 4 * (n - 1), int(ids[-2]))) == (VACANT_PERM, n - 2, ERR_ARG)
    # a vacant row that is not as a retire leaves it: velocity, heading, total_dist, len, rem, the gate's waiting word
    sl = shape_for(n)
    assert bad([(rec + 48 * last + 27, 0x3f)]) == (VACANT_WORDS, last, ERR_ARG)
    assert bad([(rec + 48 * last + 35, 0xbf)]) == (VACANT_WORDS, last, ERR_ARG)
    assert bad([(off[SEC['heading']] + 24 * last + 15, 0x3f)]) == (VACANT_WORDS, last, ERR_ARG)
    assert bad([(off[SEC['total_dist']] + 8 * last + 7, 0x3f)]) == (VACANT_WORDS, last, ERR_ARG)
    assert bad([(off[SEC['len']] + 4 * last, 1)]) == (VACANT_WORDS, last, ERR_ARG)
    assert bad([(off[SEC['len']] + 4 * int(ids[0]), 2), (off[SEC['rem']] + 4 * int(ids[0]), 1)]) == (VACANT_WORDS, int(ids[0]), ERR_ARG)
    assert bad(put(off[SEC['gate_words']] + 4 * last, 1)) == (VACANT_WORDS, last, ERR_ARG)
    assert bad([(rec + 48 * last + 27, 0x80)]) == (OK, -1, 0)       # (-0.0 is zero)
    assert sl['form'] == SLOTS and sl['gate'] == 1
    # what the check does not ask of a vacant row: step_num, status, the mission cursor -- the blob is taken
    assert bad([(off[SEC['step_num']] + 4 * last, 9), (off[SEC['status']] + 4 * last, 1)]) == (OK, -1, 0)


@pytest.mark.parametrize('n', [63, 64, 65, 257])
def test_vacancy_with_block_form_lists(H, n):
    vac = vacant_mask(n)
    s = dict(form=BLOCK, W=0)
    blob = make(H, vac, **s)
    assert check(H, blob, True, block_len=np.full(n, 2), n=n, **s) == (VACANT_BLOCK, -1, ERR_ARG)
    assert check(H, blob, True, ctx=False, n=n, **s) == (VACANT_BLOCK, -1, ERR_ARG)
    none = dict(form=NONE, W=0, M=0, R=0, gate=0, clear=0, tw=0)
    assert check(H, make(H, vac, **none), True, n=n, **none) == (OK, -1, 0)


def test_one_row_cannot_be_vacant(H):
    """n = 1: the header's bit has no legal occupied count, and the one row with flag word 11 is one vacant row too many"""
    blob = make(H, np.zeros(1, np.uint8))
    off = want_layout(**shape_for(1))[0]
    assert check(H, blob, True, n=1) == (OK, -1, 0)
    for occupied in (0, 1):
        assert check(H, damaged(H, blob, [(PRESENT_AT, 63)] + put(OCCUPIED_AT, occupied)), True, n=1) == (HEADER_RANGE, -1, ERR_ARG)
    assert check(H, damaged(H, blob, [(off[SEC['rec']] + 36, 11)]), True, n=1) == (VACANT_COUNT, -1, ERR_ARG)
    assert check(H, damaged(H, blob, [(off[SEC['rec']] + 36, 11)]), False, n=1) == (FLAGS, 0, ERR_ARG)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_without_the_flag_the_check_answers_as_it_did(H, n):
    """the same damaged blobs: bit 8 of a flag word is CXF_FLAGS at the row, the header's bit and a word in the reserved place are
    CXF_HEADER_RANGE, and a blob without vacant rows is taken with and without the flag"""
    plain = make(H, np.zeros(n, np.uint8))
    off = want_layout(**shape_for(n))[0]
    rec = off[SEC['rec']]
    for allow in (False, True):
        assert check(H, plain, allow, n=n) == (OK, -1, 0)
    assert check(H, damaged(H, plain, [(PRESENT_AT, 63)]), False, n=n) == (HEADER_RANGE, -1, ERR_ARG)
    assert check(H, damaged(H, plain, put(OCCUPIED_AT, 1)), False, n=n) == (HEADER_RANGE, -1, ERR_ARG)
    assert check(H, damaged(H, plain, put(OCCUPIED_AT, 1)), True, n=n) == (HEADER_RANGE, -1, ERR_ARG)      # occupied without the bit
    for row in {0, n // 2, n - 1}:
        for flags in (8, 9, 11):
            assert check(H, damaged(H, plain, [(rec + 48 * row + 36, flags)]), False, n=n) == (FLAGS, row, ERR_ARG)
    if n >= 2:
        vac = vacant_mask(n)
        assert check(H, make(H, vac), False, n=n) == (HEADER_RANGE, -1, ERR_ARG)
        # ... and with the header's words taken out again the first vacant row's flag word is what the check names
        assert check(H, damaged(H, make(H, vac), [(PRESENT_AT, 31)] + put(OCCUPIED_AT, 0)), False, n=n) == (FLAGS, 1, ERR_ARG)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_a_blob_without_vacant_rows_is_byte_for_byte_the_old_blob(H, n):
    """cxv_make with no row named writes what cx_make writes: the header's bit and the occupied word appear only where m < n"""
    s = shape_for(n)
    total = want_layout(**s)[1]
    old = np.zeros(total, np.uint8)
    assert H.cx_make(vp(shape8(**s)), vp(policy_for(n)), vp(old)) == total
    new = make(H, np.zeros(n, np.uint8))
    assert new.tobytes() == old.tobytes() and old[PRESENT_AT] == 31 and not old[OCCUPIED_AT:OCCUPIED_AT + 4].any()
    if n >= 2:
        vac = vacant_mask(n)
        with_rows = make(H, vac)
        assert with_rows[PRESENT_AT] == 63 and int(np.frombuffer(with_rows[OCCUPIED_AT:OCCUPIED_AT + 4].tobytes(), np.int32)[0]) == n - int(vac.sum())


# ---- the row move ----------------------------------------------------------------------------------------------------------------------------------
def outputs(n):
    return [np.zeros(8 * n, np.float32), np.zeros(8 * n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)]


@pytest.mark.parametrize('n', [2, 63, 64, 65, 257, 700])
def test_the_row_move_with_vacant_rows(H, n):
    """save -> load into zeroed arrays -> save, byte for byte, by 1, 64 and 1000 threads; behind the load a vacant row's action row is
    zero, its diag -1, nbr_n 0, nbr_valid 0, near_n -1 -- literally, and as vacate_write_row leaves the same arrays -- and an occupied
    row's outputs are untouched (7.5, 5, 3, 1, 4: what the harness fills them with)"""
    vac = vacant_mask(n)
    for s in (dict(), dict(form=NONE, W=0, M=0, R=0, gate=0, clear=0, tw=0)):
        sh = shape_for(n, **s)
        blob = make(H, vac, **s)
        want = outputs(n)
        H.cxv_retired_outputs(vp(shape8(**sh)), vp(vac), *(vp(a) for a in want))
        for threads in (1, 64, 1000):
            back, got, done = np.zeros_like(blob), outputs(n), np.zeros(256, np.int32)
            H.cxv_roundtrip(vp(shape8(**sh)), vp(blob), threads, vp(back), *(vp(a) for a in got), vp(done))
            assert back.tobytes() == blob.tobytes(), (n, s, threads)
            for g, w in zip(got, want):
                assert g.tobytes() == w.tobytes(), (n, s, threads)
            action, diag, nbr_n, near_n, valid = got
            v = vac.astype(bool)
            assert not action.reshape(n, 8)[v, :7].any() and (action.reshape(n, 8)[v, 7] == 7.5).all() and (action.reshape(n, 8)[~v] == 7.5).all()
            assert (diag.reshape(n, 8)[v] == -1).all() and (diag.reshape(n, 8)[~v] == 5).all()
            assert not nbr_n[v].any() and not valid[v].any() and (near_n[v] == -1).all()
            assert (nbr_n[~v] == 3).all() and (valid[~v] == 1).all() and (near_n[~v] == 4).all()
            running = np.flatnonzero((np.arange(n) % 3 != 2) & ~v)                      # cx_make flags every third row from row 2 on as arrived
            assert done.tolist() == np.bincount(running & 255, minlength=256).tolist(), (n, threads)


# ---- the harness as a program of its own under the sanitizers ---------------------------------------------------------------------------------
def test_the_harness_alone_under_asan_and_ubsan():
    probe = subprocess.run(['gcc', '-print-file-name=libasan.so'], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip('libasan.so not found')
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, 'context_checkpoint_vacancy_asan')
    subprocess.check_call(['g++', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-DCONTEXT_CHECKPOINT_VACANCY_MAIN'] + CXXFLAGS + ['-o', exe, SRC])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1'))
    out = run.stdout[-4000:] + '\n' + run.stderr[-6000:]
    assert run.returncode == 0 and 'AddressSanitizer' not in out and 'runtime error' not in out, out
    # seven rows, 1, 4 and 5 vacant, 2 arrived: the permutation reads 6 3 2 0 | 1 4 5; rows 0, 3 and 6 run: stripes 0, 3 and 6
    want = [('valid', 0, OK, -1), ('not allowed', -1, HEADER_RANGE, -1), ('occupied 0', -1, HEADER_RANGE, -1), ('occupied n', -1, HEADER_RANGE, -1),
            ('flags 9', -1, VACANT_FLAGS, 4), ('count', -1, VACANT_COUNT, -1), ('prefix', -1, VACANT_PERM, 0), ('tail', -1, VACANT_PERM, 4),
            ('velocity', -1, VACANT_WORDS, 1), ('len', -1, VACANT_WORDS, 5), ('waiting', -1, VACANT_WORDS, 4)]
    lines = run.stdout.strip().split('\n')
    assert lines[:len(want)] == ['%s: rc %d fault %d entry %d' % w for w in want], lines
    assert lines[len(want):] == ['roundtrip by 1: equal, outputs equal, done 1 0 0', 'roundtrip by 5: equal, outputs equal, done 1 0 0'], lines


# ---- what the GPU corpus holds at its save points ----------------------------------------------------------------------------------------------
SAVE_POINTS = (1, 6, 11)                                            # tests/test_gpu_context_checkpoint_vacancy.py saves behind these steps
CORPUS = {1: dict(vacant=1683, seeds=33, below_half=0, tracked=575, back=0),
          6: dict(vacant=5415, seeds=32, below_half=5, tracked=1870, back=4311),
          11: dict(vacant=5610, seeds=32, below_half=9, tracked=1896, back=6266)}


def test_what_the_corpus_holds_at_the_save_points(oracle):
    """counted from tests/vacancy_rule.py and the oracle alone, over seeds 0 .. 39 (1 .. 1600 agents), behind steps 1, 6 and 11: vacant rows,
    the seeds that hold any, the seeds whose occupied rows are fewer than half, vacant rows of the tracked policies (SCA, RVO3D+Dubins),
    and occupied rows that had been vacant at an earlier step; the smallest occupied count anywhere is 1"""
    got = {k: dict.fromkeys(CORPUS[k], 0) for k in SAVE_POINTS}
    least = None
    for seed in V.SEEDS:
        scene = F.random_scene(seed)
        run = V.oracle_run(oracle, scene)
        n = scene['n']
        ever = np.zeros(n, bool)
        for t, st in enumerate(run):
            vac = st['vacant']
            if t + 1 in got:
                c, m = got[t + 1], int((~vac).sum())
                c['vacant'] += n - m
                c['seeds'] += int(m < n)
                c['below_half'] += int(2 * m < n)
                c['tracked'] += int(np.isin(scene['policy'][vac], (0, 5)).sum())
                c['back'] += int((ever & ~vac).sum())
                least = m if least is None else min(least, m)
            ever |= vac
    assert got == CORPUS and least == 1, (got, least)
