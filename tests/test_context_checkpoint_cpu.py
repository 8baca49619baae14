"""Context checkpoints without a GPU (sca_checkpoint.h behind tests/context_checkpoint_harness.cpp, and the library's two pure exports): the
blob's layout for every combination of present sections, every refusal of the check a load makes before any device work with its code,
truncation at every section boundary, the calls' own rules, the kernels' row move over plain arrays (save -> load into zeroed arrays ->
save reproduces the blob byte for byte), and what the GPU corpus holds at its save step.  Expectations are literals worked out by hand from
the layout and the rules in include/sca_hip.h -- none comes from the code under test.  The same harness then runs as a program of its own
under AddressSanitizer and UBSan, every blob and every array in a buffer of exactly its size."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from harness_util import BUILD, CSRC, ROOT

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5
(OK, SHORT, MAGIC, FORMAT, RECORD, HEADER_RANGE, BYTES, CHECKSUM, N_, POLICY, TRACKER, LISTS, LIST_W, TABLES, GATE, CLEARANCE, PERM, FLAGS, NOT_FINITE,
 NOT_POSITIVE, COUNTERS, LEN_RANGE, REM_RANGE, MISSION_RANGE, COLLECTED, VERDICT, CLEAR_PARTNER, TRACK_RANGE) = range(28)      # CtxFault
CALL_OK, NO_AGENTS, NO_STATE, MID_STEP, SCENES, SHARD, COMM, PARTITION, NO_BUFFER = range(9)                                 # CtxCallFault
SRC = os.path.join(ROOT, 'tests', 'context_checkpoint_harness.cpp')
CXXFLAGS = ['-std=c++17', '-ffp-contract=off', '-mfma', '-fno-builtin-pow', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-Wno-unused-function',
            '-I' + CSRC]
HEADER = 128
SECTIONS = 26
TRK_WORDS = 112                                                    # sizeof(AgentTrack) / 4: the record is 448 bytes
NONE, BLOCK, SLOTS = 0, 1, 2
SEC = dict(policy=0, rec=1, heading=2, goal=3, pref_speed=4, max_run_dist=5, zaxis=6, vpref=7, mode=8, total_dist=9, step_num=10, status=11, perm=12,
           goal_heading=13, nbr0=14, track=15, rem=16, now_goal=17, len=18, rooms=19, ms_words=20, ms_results=21, ms_totals=22, gate_words=23,
           gate_totals=24, clear=25)
POL = np.array([0, 1, 5, 3, 4, 0, 2], np.uint8)                    # SCA, RVO3D, RVO3D+Dubins, ORCA3D, ORCA3D-LP, SCA, ORCA
FULL = dict(n=7, tw=TRK_WORDS, form=SLOTS, W=3, M=2, R=2, gate=1, clear=1)


def section_bytes(n, tw, form, W, M, R, gate, clear):
    """bytes of the 26 sections, from include/sca_hip.h's list: per row 1 / 48 / 24 / 24 / 8 / 8 / 4 / 24 / 4 / 8 / 4 / 4 / 4, the tracker's
    24 / 8 / 4 tw, the lists' 4 / 24 and in slot form 4 / 24 W, the tables' 28 / 96 R and 64 bytes of totals, the gate's 16 and 64, 32"""
    t, ls, sl, tb = bool(tw), form != NONE, form == SLOTS, M > 0
    return [n, 48 * n, 24 * n, 24 * n, 8 * n, 8 * n, 4 * n, 24 * n, 4 * n, 8 * n, 4 * n, 4 * n, 4 * n,
            24 * n * t, 8 * n * t, 4 * tw * n, 4 * n * ls, 24 * n * ls, 4 * n * sl, 24 * W * n * sl,
            28 * n * tb, 96 * R * n * tb, 64 * tb, 16 * n * bool(gate), 64 * bool(gate), 32 * n * bool(clear)]


def want_layout(**s):
    off, at = [], HEADER
    for b in section_bytes(**s):
        off.append(at)
        at += (b + 15) // 16 * 16
    return off, at


def shape8(n, tw, form, W, M, R, gate, clear):
    return np.array([n, tw, form, W, M, R, gate, clear], np.int32)


@pytest.fixture(scope='module')
def H():
    out = os.path.join(BUILD, 'libcontext_checkpoint_harness.so')
    deps = [SRC, os.path.join(ROOT, 'include', 'sca_hip.h')] + [os.path.join(CSRC, f) for f in ('sca_checkpoint.h', 'sca_scenes.h', 'sca_core.h', 'sca_dubins.hpp', 'sca_constants.h')]
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(['g++', '-O2', '-fPIC', '-shared'] + CXXFLAGS + ['-o', out, SRC])
    h = C.CDLL(out)
    h.cx_layout.restype = C.c_int64
    h.cx_make.restype = C.c_int64
    return h


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def layout(H, **s):
    off, ln = (C.c_int64 * SECTIONS)(), (C.c_int64 * SECTIONS)()
    total = H.cx_layout(vp(shape8(**s)), off, ln)
    return list(off), list(ln), total


def make(H, policy=POL, **s):
    s = dict(FULL, **s)
    total = want_layout(**s)[1]
    blob = np.zeros(total, np.uint8)
    policy = np.ascontiguousarray(policy[:s['n']] if len(policy) >= s['n'] else np.resize(policy, s['n']), np.uint8)
    assert H.cx_make(vp(shape8(**s)), vp(policy), vp(blob)) == total
    return blob


def check(H, blob, ctx=True, policy=POL, block_len=None, n_obs=0, nbytes=None, **s):
    """(fault, entry, code) of ctx_checkpoint_check; the blob is passed in a buffer of exactly nbytes"""
    s = dict(FULL, **s)
    nbytes = len(blob) if nbytes is None else nbytes
    exact = np.ascontiguousarray(blob[:nbytes]).copy()
    policy = np.ascontiguousarray(policy, np.uint8)
    bl = None if block_len is None else np.ascontiguousarray(block_len, np.int32)
    out = (C.c_int64 * 2)()
    rc = H.cx_check(vp(exact), C.c_int64(nbytes), 1 if ctx else 0, vp(shape8(**s)), vp(policy), None if bl is None else vp(bl), n_obs, out)
    return out[0], out[1], rc


def damaged(H, blob, edits, seal=True):
    b = blob.copy()
    for at, v in edits:
        b[at] = v
    if seal:
        H.cx_seal(vp(b), C.c_int64(len(b)))
    return b


# ---- the layout ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_sections_are_aligned_disjoint_and_the_total_is_right(H, n):
    """every combination of present sections: tracker x (no lists, block form, slot form W = 3) x (no tables, tables, tables + gate) x
    closest-approach records; the library's export (sca_context_checkpoint_bytes' arithmetic) says the same"""
    from sca_amd import solver as S
    assert H.cx_sections() == SECTIONS and H.cx_header_bytes() == HEADER and H.cx_track_words() == TRK_WORDS
    for tw, (form, W), (M, R, gate), clear in itertools.product((0, TRK_WORDS), ((NONE, 0), (BLOCK, 0), (SLOTS, 3)), ((0, 0, 0), (3, 2, 0), (3, 1, 1)), (0, 1)):
        s = dict(n=n, tw=tw, form=form, W=W, M=M, R=R, gate=gate, clear=clear)
        off, ln, total = layout(H, **s)
        want_off, want_total = want_layout(**s)
        assert off == want_off and total == want_total and ln == section_bytes(**s), s
        assert off[0] == HEADER and total % 16 == 0
        for k in range(SECTIONS):
            assert off[k] % 16 == 0, (s, k)
            assert off[k] + ln[k] <= (off[k + 1] if k < SECTIONS - 1 else total), (s, k)
        lib_off, lib_total = S.context_checkpoint_layout(n, tw, form, W, M, R, gate, clear)
        assert lib_off.tolist() == want_off and lib_total == want_total, s


def test_the_layout_by_hand(H):
    """7 rows with everything: 128 + 16 + 336 + 176 + 176 + 64 + 64 + 32 + 176 + 32 + 64 + 32 + 32 + 32 (always) + 176 + 64 + 3136 (tracker)
    + 32 + 176 + 32 + 512 (lists, W = 3) + 208 + 1344 + 64 (tables, R = 2) + 112 + 64 (gate) + 224 (closest approach) = 7504; one bare row:
    128 + 16 + 48 + 32 + 32 + 32 (header, policy, record, heading, goal, v_pref) + 8 x 16 (the eight columns of 4 or 8 bytes) = 416"""
    from sca_amd import solver as S
    bare = dict(n=1, tw=0, form=0, W=0, M=0, R=0, gate=0, clear=0)
    assert layout(H, **FULL)[2] == 7504 and layout(H, **bare)[2] == 416
    assert S.context_checkpoint_layout(7, TRK_WORDS, SLOTS, 3, 2, 2, 1, 1)[1] == 7504 and S.context_checkpoint_layout(1)[1] == 416


def test_shapes_the_layout_refuses(H):
    from sca_amd import solver as S
    good = dict(n=4, tw=0, form=NONE, W=0, M=0, R=0, gate=0, clear=0)
    for bad in (dict(n=0), dict(tw=-1), dict(form=3), dict(form=-1), dict(form=SLOTS, W=0), dict(form=BLOCK, W=2), dict(W=1), dict(M=128, R=1), dict(M=-1), dict(M=2, R=0),
                dict(R=1), dict(gate=1), dict(gate=2, M=1, R=1), dict(clear=2)):
        s = dict(good, **bad)
        assert layout(H, **s)[2] == -1, bad
        with pytest.raises(S.ScaError):
            S.context_checkpoint_layout(s['n'], s['tw'], s['form'], s['W'], s['M'], s['R'], s['gate'], s['clear'])


# ---- the check ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_valid_blob_passes_with_and_without_a_context(H):
    blob = make(H)
    assert check(H, blob) == (OK, -1, 0)
    assert check(H, blob, ctx=False) == (OK, -1, 0)
    for s in (dict(tw=0), dict(form=NONE, W=0), dict(form=BLOCK, W=0), dict(M=0, R=0, gate=0), dict(gate=0), dict(clear=0), dict(n=1, tw=0, form=NONE, W=0, M=0, R=0, gate=0, clear=0)):
        b = make(H, **s)
        assert check(H, b, block_len=np.full(7, 2, np.int32), **s) == (OK, -1, 0), s
        assert check(H, b, ctx=False, **s) == (OK, -1, 0), s


def test_the_envelope(H):
    blob = make(H)
    total = len(blob)
    assert check(H, blob, nbytes=127) == (SHORT, -1, ERR_ARG)
    assert check(H, blob, nbytes=0) == (SHORT, -1, ERR_ARG)
    assert check(H, blob, nbytes=total - 1) == (BYTES, -1, ERR_ARG)
    assert check(H, np.concatenate([blob, np.zeros(16, np.uint8)])) == (BYTES, -1, ERR_ARG)
    off = want_layout(**FULL)[0]
    for k in range(1, SECTIONS):                                       # truncation at every section boundary
        assert check(H, blob, nbytes=off[k]) == (BYTES, -1, ERR_ARG), k
    assert check(H, blob, nbytes=HEADER) == (BYTES, -1, ERR_ARG)
    assert check(H, damaged(H, blob, [(0, 0)])) == (MAGIC, -1, ERR_ARG)
    assert check(H, damaged(H, blob, [(4, 9)])) == (FORMAT, -1, ERR_ARG)
    assert check(H, damaged(H, blob, [(16, 111)])) == (RECORD, -1, ERR_ARG)            # trk_words
    assert check(H, damaged(H, blob, [(20, 40)])) == (RECORD, -1, ERR_ARG)             # the public record's bytes
    assert check(H, damaged(H, blob, [(12, 0)])) == (HEADER_RANGE, -1, ERR_ARG)        # n = 0
    assert check(H, damaged(H, blob, [(24, 63)])) == (HEADER_RANGE, -1, ERR_ARG)       # an unknown `present` bit
    assert check(H, damaged(H, blob, [(24, 27)])) == (HEADER_RANGE, -1, ERR_ARG)       # tables absent by the bits, M = 2 by the word
    assert check(H, damaged(H, blob, [(28, 1)])) == (HEADER_RANGE, -1, ERR_ARG)        # block form with W = 3
    assert check(H, damaged(H, blob, [(48, 2)])) == (HEADER_RANGE, -1, ERR_ARG)        # state_fresh = 2
    assert check(H, damaged(H, blob, [(12, 8)])) == (BYTES, -1, ERR_ARG)               # the header says eight rows: the byte count is seven rows'
    assert check(H, damaged(H, blob, [(off[SEC['heading']] + 3, 1)], seal=False)) == (CHECKSUM, -1, ERR_ARG)   # the checksum left stale
    assert check(H, damaged(H, blob, [(total - 1, 1)], seal=False)) == (CHECKSUM, -1, ERR_ARG)
    assert check(H, damaged(H, blob, [(72, blob[72] ^ 1)], seal=False)) == (CHECKSUM, -1, ERR_ARG)


def test_the_blob_against_the_context(H):
    blob = make(H)
    assert check(H, blob, n=8, policy=np.resize(POL, 8)) == (N_, -1, ERR_ARG)
    other = POL.copy()
    other[4] = 3
    assert check(H, blob, policy=other) == (POLICY, 4, ERR_ARG)
    assert check(H, blob, tw=0) == (TRACKER, -1, ERR_ARG)
    assert check(H, make(H, tw=0)) == (TRACKER, -1, ERR_ARG)
    assert check(H, blob, form=NONE, W=0) == (LISTS, -1, ERR_ARG)
    assert check(H, blob, form=BLOCK, W=0) == (LISTS, -1, ERR_ARG)
    assert check(H, make(H, form=BLOCK, W=0)) == (LISTS, -1, ERR_ARG)
    assert check(H, blob, W=4) == (LIST_W, -1, ERR_ARG)                                 # W = 3 into W = 4
    assert check(H, blob, M=0, R=0, gate=0) == (TABLES, -1, ERR_ARG)
    assert check(H, blob, M=3) == (TABLES, -1, ERR_ARG)
    assert check(H, blob, R=1) == (TABLES, -1, ERR_ARG)
    assert check(H, blob, gate=0) == (GATE, -1, ERR_ARG)
    assert check(H, make(H, gate=0)) == (GATE, -1, ERR_ARG)
    assert check(H, blob, clear=0) == (CLEARANCE, -1, ERR_ARG)
    assert check(H, make(H, clear=0)) == (CLEARANCE, -1, ERR_ARG)
    # block form: a cursor beyond the list's length as the context has it set (cx_make: rem = i % 3)
    b = make(H, form=BLOCK, W=0)
    assert check(H, b, form=BLOCK, W=0, block_len=[2, 2, 2, 2, 2, 2, 2]) == (OK, -1, 0)
    assert check(H, b, form=BLOCK, W=0, block_len=[2, 2, 1, 2, 2, 2, 2]) == (REM_RANGE, 2, ERR_ARG)


def test_the_payload(H):
    blob = make(H)
    off = want_layout(**FULL)[0]
    o = lambda k: off[SEC[k]]
    n = 7
    fo = (C.c_int * 12)()
    H.cx_track_offsets(fo)
    cases = [
        ('a repeated permutation entry', [(o('perm'), 5)], (PERM, 1)),                   # position 0 holds 5, as position 1 does
        ('a permutation entry out of range', [(o('perm') + 1, 1)], (PERM, 0)),           # position 0 holds 262
        ('an unknown flag bit', [(o('rec') + 36, 8)], (FLAGS, 0)),
        ('a vpref_mode of 2', [(o('mode') + 4 * 3, 2)], (FLAGS, 3)),
        ('a z-axis word of 2', [(o('zaxis') + 4 * 4, 2)], (FLAGS, 4)),
        ('x = +inf', [(o('rec') + 48 * 2 + 6, 0xf0), (o('rec') + 48 * 2 + 7, 0x7f)], (NOT_FINITE, 2)),
        ('a radius of -0.5', [(o('rec') + 48 * 5 + 47, 0xbf)], (NOT_POSITIVE, 5)),
        ('a pref_speed of 0', [(o('pref_speed') + 8 * 1 + 6, 0), (o('pref_speed') + 8 * 1 + 7, 0)], (NOT_POSITIVE, 1)),
        ('a max_run_dist of NaN', [(o('max_run_dist') + 8 * 6 + 6, 0xf8), (o('max_run_dist') + 8 * 6 + 7, 0x7f)], (NOT_POSITIVE, 6)),
        ('a negative step_num', [(o('step_num') + 4 * 2 + 3, 0x80)], (COUNTERS, 2)),
        ('a negative clear_step', [(47, 0x80)], (COUNTERS, -1)),
        ('negative updates', [(63, 0x80)], (COUNTERS, -1)),
        ('len above W', [(o('len') + 4 * 1, 4)], (LEN_RANGE, 1)),
        ('a negative len', [(o('len') + 4 * 5 + 3, 0x80)], (LEN_RANGE, 5)),
        ('rem above len', [(o('rem') + 4 * 2, 3)], (REM_RANGE, 2)),                      # row 2: len 2
        ('a negative rem', [(o('rem') + 4 * 4 + 3, 0x80)], (REM_RANGE, 4)),
        ('first_ok = M', [(o('ms_words') + 4 * (0 * n + 6), 2)], (MISSION_RANGE, 6)),
        ('first_fail = -2', [(o('ms_words') + 4 * (1 * n + 3), 0xfe)], (MISSION_RANGE, 3)),
        ('a cursor = M', [(o('ms_words') + 4 * (2 * n + 1), 2)], (MISSION_RANGE, 1)),
        ('flying = M', [(o('ms_words') + 4 * (3 * n + 0), 2), (o('ms_words') + 4 * (3 * n + 0) + 1, 0), (o('ms_words') + 4 * (3 * n + 0) + 2, 0), (o('ms_words') + 4 * (3 * n + 0) + 3, 0)],
         (MISSION_RANGE, 0)),
        ('collected above ended', [(o('ms_words') + 4 * (5 * n + 0), 1)], (COLLECTED, 0)),   # row 0 has ended 0 times
        ('waiting = M', [(o('gate_words') + 4 * (0 * n + 5), 2)], (MISSION_RANGE, 5)),
        ('a verdict above SCA_SPAWN_OVER_CAP', [(o('gate_words') + 4 * (1 * n + 3), 5)], (VERDICT, 3)),
        ('negative refusals', [(o('gate_words') + 4 * (2 * n + 2) + 3, 0x80)], (VERDICT, 2)),
        ('a closest-approach partner = n', [(o('clear') + 32 * 2 + 16, n)], (CLEAR_PARTNER, 2)),
        ('an obstacle partner where there are no obstacles', [(o('clear') + 32 * 4 + 24 + k, 0) for k in range(4)], (CLEAR_PARTNER, 4)),
        ('a negative closest-approach step', [(o('clear') + 32 * 1 + 23, 0x80)], (CLEAR_PARTNER, 1)),
        ('the tracker cursor behind the samples', [(o('track') + 448 * 3 + fo[11], 41)], (TRACK_RANGE, 3)),
        ('a negative sample count', [(o('track') + 448 * 4 + fo[10] + 7, 0x80)], (TRACK_RANGE, 4)),
        ('a Dubins word that is none', [(o('track') + fo[4], ord('X'))], (TRACK_RANGE, 0)),
        ('a bool of 2', [(o('track') + 448 * 6 + fo[0], 2)], (TRACK_RANGE, 6)),
        ('negative re-plans', [(o('track') + 448 * 2 + fo[9] + 3, 0x80)], (TRACK_RANGE, 2)),
    ]
    for what, edits, (fault, entry) in cases:
        assert check(H, damaged(H, blob, edits)) == (fault, entry, ERR_ARG), what
    # the same values are refused without a context -- the obstacle bound is the context's alone
    assert check(H, damaged(H, blob, cases[0][1]), ctx=False) == (PERM, 1, ERR_ARG)
    assert check(H, damaged(H, blob, cases[25][1]), ctx=False) == (OK, -1, 0)
    assert check(H, damaged(H, blob, cases[25][1]), n_obs=1) == (OK, -1, 0)
    # an unknown policy byte: against a context the comparison names the row, without one the range does
    assert check(H, damaged(H, blob, [(o('policy') + 2, 6)]), ctx=False) == (POLICY, 2, ERR_ARG)


def test_the_calls_rules_in_their_order(H):
    def call(agents=1, state=1, mid=0, scenes=0, comm=0, part=0, n=8, shard=8, buffer=1):
        f = C.c_int(0)
        rc = H.cx_call(agents, state, mid, scenes, comm, part, n, shard, buffer, C.byref(f))
        return f.value, rc
    assert call() == (CALL_OK, 0)
    assert call(agents=0, state=0, mid=1, scenes=1, buffer=0) == (NO_AGENTS, ERR_STATE)
    assert call(state=0, mid=1, scenes=1, buffer=0) == (NO_STATE, ERR_STATE)
    assert call(mid=1, scenes=1, buffer=0) == (MID_STEP, ERR_STATE)
    assert call(scenes=1, comm=1, buffer=0) == (SCENES, ERR_UNSUPPORTED)
    assert call(comm=1, part=1, shard=4, buffer=0) == (COMM, ERR_UNSUPPORTED)
    assert call(part=1, shard=4, buffer=0) == (PARTITION, ERR_UNSUPPORTED)
    assert call(shard=7, buffer=0) == (SHARD, ERR_UNSUPPORTED)
    assert call(buffer=0) == (NO_BUFFER, ERR_ARG)


# ---- the row move ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 7, 63, 64, 65, 257, 700])
def test_save_load_save_reproduces_the_blob(H, n):
    """the kernels' row move over plain arrays of exactly the rows' sizes, by 1, 3 and 64 threads: a blob loaded into zeroed arrays and saved
    from them again is the blob; K4's stripes hold the rows without a flag (cx_make: every third row has one), the "entered live" column
    follows the flags"""
    for s in (dict(FULL, n=n), dict(n=n, tw=0, form=BLOCK, W=0, M=3, R=1, gate=0, clear=0), dict(n=n, tw=TRK_WORDS, form=NONE, W=0, M=0, R=0, gate=0, clear=1),
              dict(n=n, tw=0, form=NONE, W=0, M=0, R=0, gate=0, clear=0)):
        blob = make(H, **s)
        for threads in (1, 3, 64):
            back, live, done = np.zeros_like(blob), np.full(n, -1, np.int32), np.zeros(256, np.int32)
            H.cx_roundtrip(vp(shape8(**s)), vp(blob), threads, vp(back), vp(live), vp(done))
            assert back.tobytes() == blob.tobytes(), (s, threads, np.flatnonzero(back != blob)[:8])
            flagged = np.arange(n) % 3 == 2
            want = np.bincount(np.arange(n)[~flagged] & 255, minlength=256)
            assert done.tolist() == want.tolist(), (s, threads)
            if s['M']:
                assert live.tolist() == (~flagged).astype(int).tolist(), (s, threads)


# ---- the library's pure export ---------------------------------------------------------------------------------------------------------------------
def test_checkpoint_info_reads_the_header_behind_the_whole_check(H):
    from sca_amd import solver as S
    blob = make(H)
    info = S.context_checkpoint_info(blob)
    assert {k: info[k] for k in ('format', 'lib_version', 'n', 'trk_words', 'record_bytes', 'has_tracker', 'list_form', 'W', 'M', 'R', 'has_gate', 'has_clearance',
                                 'clear_step', 'state_fresh', 'updates', 'total_bytes')} == \
        dict(format=1, lib_version=103, n=7, trk_words=TRK_WORDS, record_bytes=48, has_tracker=1, list_form=SLOTS, W=3, M=2, R=2, has_gate=1, has_clearance=1,
             clear_step=6, state_fresh=0, updates=6, total_bytes=7504)
    assert info['policy'].tolist() == POL.tolist() and info['offsets'].tolist() == want_layout(**FULL)[0]
    assert S.context_checkpoint_info(blob.tobytes())['checksum'] == info['checksum']
    perm = want_layout(**FULL)[0][SEC['perm']]
    for bad in (blob[:-1], damaged(H, blob, [(perm, 5)]), damaged(H, blob, [(200, 1)], seal=False)):
        with pytest.raises(S.ScaError):
            S.context_checkpoint_info(bad)


# ---- the harness as a program of its own under the sanitizers ---------------------------------------------------------------------------------
def test_the_harness_alone_under_asan_and_ubsan():
    probe = subprocess.run(['gcc', '-print-file-name=libasan.so'], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip('libasan.so not found')
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, 'context_checkpoint_asan')
    subprocess.check_call(['g++', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-DCONTEXT_CHECKPOINT_MAIN'] + CXXFLAGS + ['-o', exe, SRC])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1'))
    out = run.stdout[-4000:] + '\n' + run.stderr[-6000:]
    assert run.returncode == 0 and 'AddressSanitizer' not in out and 'runtime error' not in out, out
    want = [('valid', 0, OK, -1), ('valid, no context', 0, OK, -1), ('short', -1, SHORT, -1), ('one byte less', -1, BYTES, -1), ('header alone', -1, BYTES, -1)] + \
           [('cut at %d' % k, -1, BYTES, -1) for k in range(1, SECTIONS)] + \
           [('magic', -1, MAGIC, -1), ('checksum', -1, CHECKSUM, -1), ('permutation', -1, PERM, 1), ('len', -1, LEN_RANGE, 1), ('rem', -1, REM_RANGE, 2),
            ('cursor', -1, MISSION_RANGE, 1), ('collected', -1, COLLECTED, 0), ('verdict', -1, VERDICT, 3), ('partner', -1, CLEAR_PARTNER, 2),
            ('tracker next', -1, TRACK_RANGE, 3)]
    lines = run.stdout.strip().split('\n')
    assert lines[:len(want)] == ['%s: rc %d fault %d entry %d' % w for w in want], lines
    # seven rows, every third flagged: rows 0, 1, 3, 4, 6 run -- stripes 0 and 1 hold one row each, stripe 2 none
    assert lines[len(want):] == ['roundtrip by 1: equal, done 1 1 0', 'roundtrip by 5: equal, done 1 1 0', 'one row: rc 0 fault 0 entry -1', 'one row roundtrip: equal',
                                 'bytes 7504 416'], lines


# ---- what the GPU corpus holds at its save step --------------------------------------------------------------------------------------------------
CORPUS_SEEDS = (3, 5, 8, 10, 12, 19, 22, 28, 31, 36)               # tests/test_gpu_context_checkpoint.py resumes these at step 6 of 12
CORPUS_SAVE = 6
CORPUS_COUNTS = dict(finished_without_successor=506, rows_waiting=816, results_not_collected=1131, rows_mid_list=1259,
                     rooms_rewritten_by_a_take=52, rows_respawned_twice=11)


def corpus_counts(oracle):
    """counted from tests/mission_paths_rule.py alone, with the gate at margin 0.5, behind step 6 of 12, summed over the seeds: finished
    rows whose flight named no successor; rows with a mission waiting at the gate; results written so far (the GPU test collects none
    before it saves); rows in the middle of a list (rem < len, a now_goal); rows whose room a take has rewritten with a list of its own;
    rows taken at least twice"""
    import form_fuzz as F
    import mission_paths_rule as PR
    c = dict.fromkeys(CORPUS_COUNTS, 0)
    for seed in CORPUS_SEEDS:
        scene = F.random_scene(seed)
        run = PR.oracle_run(oracle, scene, 12, gate=(PR.GATE_MARGIN, 0))
        st, n = run['steps'][CORPUS_SAVE - 1], scene['n']
        c['finished_without_successor'] += int((((st['flags'] & 7) != 0) & (st['flying'] < 0)).sum())
        c['rows_waiting'] += int((st['waiting'] >= 0).sum())
        c['results_not_collected'] += sum(len(s['results']) for s in run['steps'][:CORPUS_SAVE])
        c['rows_mid_list'] += int(((st['path_left_after'] < st['path_len_after']) & ~np.isnan(st['now_goal_after'][:, 0])).sum())
        takes, rewritten = np.zeros(n, int), np.zeros(n, bool)
        for s in run['steps'][:CORPUS_SAVE]:
            takes[s['taken']] += 1
            for a, j in zip(s['taken'], s['taken_entry']):
                rewritten[a] |= bool(run['lists'][a][int(j)])
        c['rooms_rewritten_by_a_take'] += int(rewritten.sum())
        c['rows_respawned_twice'] += int((takes >= 2).sum())
    return c


def test_what_the_corpus_holds_at_the_save_step(oracle):
    c = corpus_counts(oracle)
    assert all(v >= 1 for v in c.values()), c
    assert c == CORPUS_COUNTS, c
