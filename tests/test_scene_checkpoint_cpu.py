"""Scene checkpoints without a GPU (sca_scenes.h behind tests/scene_checkpoint_harness.cpp, and the library's two pure exports): the blob's
layout, every refusal of the check a load makes before any device work with its code, the calls' own rules, the checksum, and
SceneCheckpoint's file form.  Expectations are literals worked out by hand from the layout and the rules in include/sca_hip.h -- none comes
from the code under test.  The same harness then runs as a program of its own under AddressSanitizer and UBSan, every blob in a buffer of
exactly its size."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from harness_util import BUILD, CSRC, ROOT

ERR_ARG, ERR_STATE = -1, -3
(OK, SHORT, MAGIC, FORMAT, RECORD, SIZE_RANGE, BYTES, CHECKSUM, SCENE_SIZE, POLICY, TRACKER, NO_LISTS, REM_RANGE, PERM, FLAGS, NOT_FINITE, COUNTERS,
 TRACK_RANGE) = range(18)                                          # CkptFault
CALL_OK, NO_SCENES, NO_STATE, MID_STEP, BAD_COUNT, BAD_ID, REPEATED_ID, NO_BUFFER = range(8)     # CkptCallFault
SRC = os.path.join(ROOT, 'tests', 'scene_checkpoint_harness.cpp')
# (sca_dubins.hpp, included for the tracker record's real offsets, defines static functions this harness does not call)
CXXFLAGS = ['-std=c++17', '-ffp-contract=off', '-mfma', '-fno-builtin-pow', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-Wno-unused-function',
            '-I' + CSRC]
HEADER = 64
TRK_WORDS = 112                                                    # sizeof(AgentTrack) / 4: the record is 448 bytes
# bytes per row of the 14 sections: policy, record, heading, kept heading, v_pref, total_dist, step_num, status, permutation, v_pref mode,
# tracker distSq, tracker record, remaining, now_goal
ROW = lambda tw, hp: [1, 48, 24, 24, 24, 8, 4, 4, 4, 4, 8 if tw else 0, 4 * tw, 4 if hp else 0, 24 if hp else 0]
SEC = dict(policy=0, rec=1, heading=2, perm=8, mode=9, nbr0=10, track=11, rem=12, now_goal=13)
POL = np.array([0, 1, 5, 3, 4], np.uint8)                          # SCA, RVO3D, RVO3D+Dubins, ORCA3D, ORCA3D-LP
LEN = np.full(5, 2, np.int32)


@pytest.fixture(scope='module')
def H():
    out = os.path.join(BUILD, 'libscene_checkpoint_harness.so')
    deps = [SRC, os.path.join(ROOT, 'include', 'sca_hip.h')] + [os.path.join(CSRC, f) for f in ('sca_scenes.h', 'sca_dubins.hpp', 'sca_constants.h')]
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(['g++', '-O2', '-fPIC', '-shared'] + CXXFLAGS + ['-o', out, SRC])
    h = C.CDLL(out)
    h.ckpt_layout.restype = C.c_int64
    h.ckpt_make.restype = C.c_int64
    h.ckpt_sum.restype = C.c_uint64
    return h


def want_layout(size, tw, hp):
    off, at = [], HEADER
    for row in ROW(tw, hp):
        off.append(at)
        at += (row * size + 15) // 16 * 16
    return off, at


def layout(H, size, tw, hp):
    off, ln = (C.c_int64 * 14)(), (C.c_int64 * 14)()
    total = H.ckpt_layout(size, tw, hp, off, ln)
    return list(off), list(ln), total


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def make(H, size=5, policy=POL, tracked=1, has_paths=1):
    _, _, total = layout(H, size, TRK_WORDS if tracked else 0, has_paths)
    blob = np.zeros(total, np.uint8)
    policy = np.ascontiguousarray(policy, np.uint8)
    assert H.ckpt_make(size, vp(policy), tracked, has_paths, vp(blob)) == total
    return blob


def check(H, blob, scene=True, size=5, policy=POL, tracker_on=1, paths_on=1, path_len=LEN, nbytes=None):
    """(fault, entry, code) of scene_checkpoint_check; the blob is passed in a buffer of exactly nbytes"""
    nbytes = len(blob) if nbytes is None else nbytes
    exact = np.ascontiguousarray(blob[:nbytes]).copy()
    policy = np.ascontiguousarray(policy, np.uint8)
    path_len = None if path_len is None else np.ascontiguousarray(path_len, np.int32)
    out = (C.c_int * 2)()
    rc = H.ckpt_check(vp(exact), C.c_int64(nbytes), 1 if scene else 0, size, vp(policy), tracker_on, paths_on, None if path_len is None else vp(path_len), out)
    return out[0], out[1], rc


def damaged(H, blob, edits, seal=True):
    b = blob.copy()
    for at, v in edits:
        b[at] = v
    if seal:
        H.ckpt_seal(vp(b), C.c_int64(len(b)))
    return b


# ---- the layout ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [1, 63, 64, 65, 1536])
@pytest.mark.parametrize('tw,hp', [(0, 0), (TRK_WORDS, 0), (0, 1), (TRK_WORDS, 1)])
def test_sections_are_aligned_disjoint_and_the_total_is_right(H, size, tw, hp):
    off, ln, total = layout(H, size, tw, hp)
    want_off, want_total = want_layout(size, tw, hp)
    assert H.ckpt_sections() == 14 and H.ckpt_header_bytes() == HEADER and H.ckpt_track_words() == TRK_WORDS
    assert off == want_off and total == want_total and ln == [r * size for r in ROW(tw, hp)]
    assert off[0] == HEADER and total % 16 == 0
    for k in range(14):
        assert off[k] % 16 == 0, k
        assert off[k] + ln[k] <= (off[k + 1] if k < 13 else total), k
    # the library's export says the same
    from sca_amd import solver as S
    lib_off, lib_total = S.scene_checkpoint_layout(size, tw, hp)
    assert lib_off.tolist() == want_off and lib_total == want_total


def test_two_totals_by_hand(H):
    # five rows with tracker records and cursors: 64 + 16 + 240 + 3 * 128 + 48 + 4 * 32 + 48 + 2240 + 32 + 128
    assert layout(H, 5, TRK_WORDS, 1)[2] == 3328
    # one row, neither: 64 + 16 + 48 + 3 * 32 + 16 + 4 * 16
    assert layout(H, 1, 0, 0)[2] == 304


def test_the_layout_export_refuses_bad_arguments():
    from sca_amd import solver as S
    for args in [(0, 0, 0), (1537, 0, 0), (5, -1, 0), (5, 0, 2)]:
        with pytest.raises(S.ScaError):
            S.scene_checkpoint_layout(*args)


# ---- the check -----------------------------------------------------------------------------------------------------------------------------------
def test_a_valid_blob_is_accepted_with_and_without_a_scene(H):
    blob = make(H)
    assert check(H, blob) == (OK, -1, 0)
    assert check(H, blob, scene=False) == (OK, -1, 0)
    one = make(H, 1, [3], tracked=0, has_paths=0)
    assert check(H, one, size=1, policy=[3], tracker_on=1, paths_on=0, path_len=None) == (OK, -1, 0)      # an untracked row needs no records
    assert check(H, one, size=1, policy=[3], tracker_on=0, paths_on=1, path_len=[0]) == (OK, -1, 0)       # lists set, this row's empty


def test_the_envelope(H):
    blob = make(H)
    off = want_layout(5, TRK_WORDS, 1)[0]
    assert check(H, blob, nbytes=63) == (SHORT, -1, ERR_ARG)
    assert check(H, blob, nbytes=0) == (SHORT, -1, ERR_ARG)
    assert check(H, blob, nbytes=len(blob) - 1) == (BYTES, -1, ERR_ARG)
    assert check(H, blob, nbytes=HEADER) == (BYTES, -1, ERR_ARG)
    assert check(H, np.concatenate([blob, np.zeros(16, np.uint8)])) == (BYTES, -1, ERR_ARG)
    assert check(H, damaged(H, blob, [(0, 0)])) == (MAGIC, -1, ERR_ARG)
    assert check(H, damaged(H, blob, [(4, 2)])) == (FORMAT, -1, ERR_ARG)
    assert check(H, damaged(H, blob, [(16, 111)])) == (RECORD, -1, ERR_ARG)                  # trk_words 111
    assert check(H, damaged(H, blob, [(20, 40)])) == (RECORD, -1, ERR_ARG)                   # a 40-byte record
    assert check(H, damaged(H, blob, [(12, 0)])) == (SIZE_RANGE, -1, ERR_ARG)                # size 0
    assert check(H, damaged(H, blob, [(12, 1), (13, 6)])) == (SIZE_RANGE, -1, ERR_ARG)       # size 1537
    assert check(H, damaged(H, blob, [(28, 2)])) == (SIZE_RANGE, -1, ERR_ARG)                # has_paths 2
    assert check(H, damaged(H, blob, [(24, 0)])) == (SIZE_RANGE, -1, ERR_ARG)                # records' words without the flag
    assert check(H, damaged(H, blob, [(12, 6)])) == (BYTES, -1, ERR_ARG)                     # six rows' header on five rows' bytes
    for at in (off[SEC['policy']], off[SEC['heading']] + 3, len(blob) - 1, HEADER + 5 + 8):  # (the last: a byte between two sections)
        assert check(H, damaged(H, blob, [(at, 77)], seal=False)) == (CHECKSUM, -1, ERR_ARG), at
    assert check(H, damaged(H, blob, [(56, blob[56] ^ 1)], seal=False)) == (CHECKSUM, -1, ERR_ARG)       # the sum itself


def test_the_blob_against_the_scene(H):
    blob = make(H)
    assert check(H, blob, size=6, policy=list(POL) + [1], path_len=[2] * 6) == (SCENE_SIZE, -1, ERR_ARG)
    assert check(H, blob, size=4) == (SCENE_SIZE, -1, ERR_ARG)
    assert check(H, blob, policy=[0, 1, 5, 3, 3]) == (POLICY, 4, ERR_ARG)
    assert check(H, blob, policy=[5, 2, 5, 3, 4]) == (POLICY, 0, ERR_ARG)                    # the first row that differs is named
    assert check(H, blob, tracker_on=0) == (TRACKER, -1, ERR_ARG)                            # records present, no tracker here
    bare = make(H, tracked=0)
    assert check(H, bare) == (TRACKER, -1, ERR_ARG)                                          # ... absent, tracked rows and a tracker here
    assert check(H, bare, tracker_on=0) == (OK, -1, 0)
    assert check(H, blob, paths_on=0, path_len=None) == (NO_LISTS, 1, ERR_ARG)               # row 1 has one waypoint left
    assert check(H, blob, path_len=[2, 0, 2, 2, 2]) == (REM_RANGE, 1, ERR_ARG)
    assert check(H, blob, path_len=[2, 1, 1, 2, 2]) == (REM_RANGE, 2, ERR_ARG)               # row 2 has two left, its list is one long
    no_cursors = make(H, has_paths=0)
    assert check(H, no_cursors, path_len=[0, 0, 0, 1, 0]) == (REM_RANGE, 3, ERR_ARG)         # the scene has a list the blob knows nothing of
    assert check(H, no_cursors, path_len=[0] * 5) == (OK, -1, 0)
    assert check(H, no_cursors, paths_on=0, path_len=None) == (OK, -1, 0)
    spent = damaged(H, blob, [(want_layout(5, TRK_WORDS, 1)[0][SEC['rem']] + 4 * i, 0) for i in range(5)])
    assert check(H, spent, paths_on=0, path_len=None) == (OK, -1, 0)                         # every cursor spent: no lists needed


def test_the_payload(H):
    blob = make(H)
    off = want_layout(5, TRK_WORDS, 1)[0]
    rec, perm, rem = off[SEC['rec']], off[SEC['perm']], off[SEC['rem']]
    for scene in (True, False):
        assert check(H, damaged(H, blob, [(perm, 3)]), scene=scene) == (PERM, 1, ERR_ARG)            # 3 3 2 1 0
        assert check(H, damaged(H, blob, [(perm + 1, 1)]), scene=scene) == (PERM, 0, ERR_ARG)        # 260
        assert check(H, damaged(H, blob, [(perm + 16, 5)]), scene=scene) == (PERM, 4, ERR_ARG)       # 5 is not a row of five
        assert check(H, damaged(H, blob, [(perm + 4 * 2 + 3, 0x80)]), scene=scene) == (PERM, 2, ERR_ARG)     # negative
        assert check(H, damaged(H, blob, [(rec + 36, 8)]), scene=scene) == (FLAGS, 0, ERR_ARG)
        assert check(H, damaged(H, blob, [(rec + 48 * 3 + 39, 1)]), scene=scene) == (FLAGS, 3, ERR_ARG)
        assert check(H, damaged(H, blob, [(off[SEC['mode']] + 8, 2)]), scene=scene) == (FLAGS, 2, ERR_ARG)
        assert check(H, damaged(H, blob, [(rec + 48 * 2 + 6, 0xf0), (rec + 48 * 2 + 7, 0x7f)]), scene=scene) == (NOT_FINITE, 2, ERR_ARG)     # x = +inf
        assert check(H, damaged(H, blob, [(rec + 48 + 16 + 6, 0xf8), (rec + 48 + 16 + 7, 0xff)]), scene=scene) == (NOT_FINITE, 1, ERR_ARG)   # z = NaN
        assert check(H, damaged(H, blob, [(rec + 40 + 7, 0xbf)]), scene=scene) == (NOT_FINITE, 0, ERR_ARG)                                   # radius -0.5
        assert check(H, damaged(H, blob, [(rec + 36, 1)]), scene=scene) == (COUNTERS, -1, ERR_ARG)   # row 0 done: three run, the header says four
        assert check(H, damaged(H, blob, [(36, 5)]), scene=scene) == (COUNTERS, -1, ERR_ARG)         # live 5
        assert check(H, damaged(H, blob, [(40, 6)]), scene=scene) == (COUNTERS, -1, ERR_ARG)         # prev 6 of five rows
        assert check(H, damaged(H, blob, [(35, 0x80)]), scene=scene) == (COUNTERS, -1, ERR_ARG)      # steps negative
    assert check(H, damaged(H, blob, [(rem + 4 + 3, 0x80)])) == (REM_RANGE, 1, ERR_ARG)              # a negative cursor


def test_every_tracker_integer_a_kernel_uses(H):
    blob = make(H)
    track = want_layout(5, TRK_WORDS, 1)[0][SEC['track']]
    fo = (C.c_int * 12)()
    H.ckpt_track_offsets(fo)
    use, plan_ok, h_ok, v_ok, h_mode, v_mode, plan_mode, iters, rounds, replans, count, nxt = list(fo)
    rec = lambda row: track + 4 * TRK_WORDS * row
    cases = [(3, nxt, 41), (4, count + 7, 0x80), (1, nxt + 7, 0x80), (0, count + 3, 1),      # cursor past the count; negative count; negative cursor; count 2^24 + 40
             (0, h_mode, ord('X')), (2, v_mode + 2, 1), (1, plan_mode + 5, ord('l')),
             (0, use, 2), (2, plan_ok, 3), (3, h_ok, 255), (4, v_ok, 2),
             (1, iters + 3, 0x80), (2, rounds + 3, 0x80), (3, replans + 3, 0x80)]
    for row, at, v in cases:
        for scene in (True, False):
            assert check(H, damaged(H, blob, [(rec(row) + at, v)]), scene=scene) == (TRACK_RANGE, row, ERR_ARG), (row, at, v)
    assert check(H, damaged(H, blob, [(rec(0) + nxt, 40)])) == (OK, -1, 0)                   # the cursor AT the count: the path is spent
    assert check(H, damaged(H, blob, [(rec(0) + nxt, 0), (rec(0) + count, 0)])) == (OK, -1, 0)


def test_the_checksum_is_fnv1a_over_64_bit_words(H):
    data = np.arange(64, dtype=np.uint8)
    h = 0xcbf29ce484222325
    for w in data.view('<u8'):
        h = ((h ^ int(w)) * 0x100000001b3) % 2 ** 64
    assert H.ckpt_sum(vp(data), C.c_int64(64)) == h
    assert H.ckpt_sum(vp(data), C.c_int64(0)) == 0xcbf29ce484222325


# ---- the two calls' own rules ---------------------------------------------------------------------------------------------------------------------
def call(H, nscenes=4, state_set=1, begun=0, count=2, ids=(1, 3), bufs=(1, 1), sizes=(8, 8)):
    keep = [np.zeros(8, np.uint8) for _ in bufs or ()]
    ptrs = None if bufs is None else (C.c_void_p * max(1, len(bufs)))(*[k.ctypes.data if b else None for k, b in zip(keep, bufs)])
    ids_a = None if ids is None else np.ascontiguousarray(ids, np.int32)
    sz = None if sizes is None else np.ascontiguousarray(sizes, np.int64)
    out = (C.c_int * 2)()
    rc = H.ckpt_call(nscenes, state_set, begun, count, None if ids_a is None else vp(ids_a), ptrs, None if sz is None else vp(sz), out)
    return out[0], out[1], rc


def test_the_calls_rules_in_their_order(H):
    assert call(H) == (CALL_OK, -1, 0)
    assert call(H, nscenes=0, state_set=0, begun=1, count=0) == (NO_SCENES, -1, ERR_STATE)
    assert call(H, state_set=0, begun=1, count=0) == (NO_STATE, -1, ERR_STATE)
    assert call(H, begun=1, count=0) == (MID_STEP, -1, ERR_STATE)
    for kw in (dict(count=0), dict(count=-1), dict(ids=None), dict(bufs=None), dict(sizes=None)):
        assert call(H, **kw) == (BAD_COUNT, -1, ERR_ARG), kw
    assert call(H, ids=(1, 4)) == (BAD_ID, 1, ERR_ARG)
    assert call(H, ids=(-1, 3)) == (BAD_ID, 0, ERR_ARG)
    assert call(H, ids=(3, 3)) == (REPEATED_ID, 1, ERR_ARG)
    assert call(H, bufs=(1, 0)) == (NO_BUFFER, 1, ERR_ARG)


# ---- the library's pure export ---------------------------------------------------------------------------------------------------------------------
def test_checkpoint_info_reads_the_header_behind_the_whole_check(H):
    from sca_amd import solver as S
    blob = make(H)
    info = S.scene_checkpoint_info(blob)
    assert {k: info[k] for k in ('format', 'lib_version', 'size', 'trk_words', 'record_bytes', 'has_tracker', 'has_paths', 'steps', 'live', 'prev', 'total_bytes')} == \
        dict(format=1, lib_version=103, size=5, trk_words=TRK_WORDS, record_bytes=48, has_tracker=1, has_paths=1, steps=11, live=4, prev=4, total_bytes=3328)
    assert info['policy'].tolist() == POL.tolist() and info['offsets'].tolist() == want_layout(5, TRK_WORDS, 1)[0]
    assert S.scene_checkpoint_info(blob.tobytes())['checksum'] == info['checksum']
    perm = want_layout(5, TRK_WORDS, 1)[0][SEC['perm']]
    for bad in (blob[:-1], damaged(H, blob, [(perm, 3)]), damaged(H, blob, [(100, 1)], seal=False)):
        with pytest.raises(S.ScaError):
            S.scene_checkpoint_info(bad)


# ---- the harness as a program of its own under the sanitizers ---------------------------------------------------------------------------------
def test_the_harness_alone_under_asan_and_ubsan():
    probe = subprocess.run(['gcc', '-print-file-name=libasan.so'], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip('libasan.so not found')
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, 'scene_checkpoint_asan')
    subprocess.check_call(['g++', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-DSCENE_CHECKPOINT_MAIN'] + CXXFLAGS + ['-o', exe, SRC])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1'))
    out = run.stdout[-4000:] + '\n' + run.stderr[-6000:]
    assert run.returncode == 0 and 'AddressSanitizer' not in out and 'runtime error' not in out, out
    want = [('valid', 0, OK, -1), ('valid, no scene', 0, OK, -1), ('short', -1, SHORT, -1), ('one byte less', -1, BYTES, -1), ('header alone', -1, BYTES, -1),
            ('magic', -1, MAGIC, -1), ('format', -1, FORMAT, -1), ('checksum', -1, CHECKSUM, -1), ('size', -1, BYTES, -1), ('permutation', -1, PERM, 1),
            ('permutation range', -1, PERM, 0), ('flags', -1, FLAGS, 0), ('position', -1, NOT_FINITE, 2), ('cursor', -1, REM_RANGE, 1),
            ('tracker next', -1, TRACK_RANGE, 3), ('tracker count', -1, TRACK_RANGE, 4), ('tracker word', -1, TRACK_RANGE, 0), ('tracker bool', -1, TRACK_RANGE, 0),
            ('policy', -1, POLICY, 4), ('scene size', -1, SCENE_SIZE, -1), ('tracker off', -1, TRACKER, -1), ('no lists', -1, NO_LISTS, 1), ('one row', 0, OK, -1)]
    lines = run.stdout.strip().split('\n')
    assert lines[:-1] == ['%s: rc %d fault %d entry %d' % w for w in want], lines
    assert lines[-1] == 'bytes 3328 304'


# ---- SceneCheckpoint's file form, without a device ---------------------------------------------------------------------------------------------
def test_a_checkpoint_file_round_trip(H, tmp_path):
    """write / read: one .npz of plain arrays (no pickle); the agents and obstacles come back through their constructors with every
    attribute the episode defines, the lists as they were handed to the device, the blob byte for byte, steps and the log rows"""
    from sca_amd import env as E, scenes
    agents = E.build_circle_agents(5, policy=E.SCAPolicy)
    agents[3] = E.Agent(start_pos=list(agents[3].initial_pos), goal_pos=list(agents[3].goal_pos), vel=[0.0, 0.0, 0.0], radius=0.4, pref_speed=1.2,
                        policy=E.ORCA3DPolicyOfficial, id=3)
    agents[1].neighborDist, agents[1].maxNeighbors, agents[2].turning_radius, agents[2].pitchlims = 7.5, 9, 2.0, [-0.5, 0.25]
    agents[4].max_run_dist, agents[0].timeStep, agents[0].max_heading_change = 33.0, 0.2, 0.5
    lists = [[], [[1.0, 2.0, 3.0], [4.0, 5.0, 6.5]], [], [[0.5, 0.25, 8.0]], []]
    obstacles = [E.Obstacle([1.0, 2.0, 3.0], dict(shape='sphere', feature=1.5), 0), E.Obstacle([-4.0, 0.0, 9.0], dict(shape='sphere', feature=0.75), 1)]
    blob = make(H)
    log = dict(pos=np.arange(7 * 5 * 3, dtype=np.float64).reshape(7, 5, 3), heading=np.ones((7, 5, 3)), vel=np.full((7, 5, 3), 0.5, np.float32))
    ck = scenes.SceneCheckpoint(scenes.SceneCheckpoint.define(agents, lists, obstacles), blob, 7, log, [0.0, 0.25, 0.5])
    path = ck.write(str(tmp_path / 'episode.npz'))
    with np.load(path, allow_pickle=False) as z:                      # plain arrays: readable with pickle refused
        assert all(z[k].dtype != object for k in z.files)
    back = scenes.SceneCheckpoint.read(path)
    assert len(back) == 5 and back.steps == 7 and back.time_cum == [0.0, 0.25, 0.5]
    assert np.array_equal(back.blob, blob) and back.blob.dtype == np.uint8
    assert all(np.array_equal(back.log[k], log[k]) and back.log[k].dtype == log[k].dtype for k in log)
    for a, b, p in zip(agents, back.agents(), lists):
        assert type(b.policy) is type(a.policy) and b.id == a.id and b._path == p
        for key in ('radius', 'pref_speed', 'turning_radius', 'maxNeighbors', 'neighborDist', 'timeStep', 'timeHorizon', 'maxSpeed', 'dt_nominal',
                    'max_heading_change', 'min_heading_change', 'max_run_dist', 'pitchlims', 'straight_path_length', 'desire_steps'):
            assert getattr(b, key) == getattr(a, key), (a.id, key)
        for key in ('initial_pos', 'goal_pos', 'goal_global_frame', 'goal_heading_frame'):
            assert np.array_equal(getattr(b, key), getattr(a, key)), (a.id, key)
        assert isinstance(b.maxNeighbors, int)
    got = back.obstacles()
    assert [o.radius for o in got] == [1.5, 0.75] and all(np.array_equal(o.pos_global_frame, w.pos_global_frame) for o, w in zip(got, obstacles))
    assert scenes.SceneCheckpoint.read(scenes.SceneCheckpoint(back.definition, blob, 0).write(str(tmp_path / 'bare.npz'))).log is None
    with pytest.raises(ValueError):                                   # (only spheres are kept as arrays)
        scenes.SceneCheckpoint.define(agents, lists, [E.Obstacle([0.0, 0.0, 0.0], dict(shape='cube', feature=[1.0, 1.0, 1.0]), 0)])
