"""The host side of one sca_restart_scenes call without a GPU (sca_amd/csrc/sca_scene_restart.h, behind tests/scenes_harness.cpp):
restart_pack's whole staging block, byte for byte, and its plan against a numpy restatement written here from the section table of
sca_scenes.h; the block's layout (restart_block_layout) against the same table; every refusal's text, copied literally from the library
as it stood before the texts moved; and the harness as a program of its own under the sanitizers.

The block starts as 0xA5 throughout and is compared WHOLE: a section the call does not write (an optional array that is NULL, the
obstacle trees and the attribute sections, which sca_hip.hip fills) must still hold 0xA5, so nothing is masked out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import harness_util
from harness_util import load_harness

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5                   # include/sca_hip.h
MAX_N, MAX_M = 8, 4
OFFSETS = [0, 3, 4, 8]                                             # three scenes of capacities 3, 1 and 4
OBS_CAP = [0, 2, 2, 4]                                             # their obstacle capacities: 2, 0 and 2
POLICY_NOW = [0, 4, 3, 4, 1, 5, 4, 2]                              # ORCA3D-LP (4) at rows 1, 3 and 6; tracked (0, 5) at rows 0 and 5
LP, TRACKED = 4, (0, 5)
HAS = dict(radius=1, pref_speed=2, goal=4, zaxis=8, max_run_dist=16, goal_heading=32, attrs=64, planner=128, path_slots=256, paths=512)
FILL = 0xA5
# the section table: name, bytes per row of max_n (agent and attribute sections) or bytes in all; every section starts on a 64-byte boundary
AGENT = [('ids', 4), ('start', 4), ('pos', 24), ('heading', 24), ('goal', 24), ('goal_heading', 24), ('radius', 8), ('pref_speed', 8),
         ('max_run_dist', 8), ('vel', 12), ('policy', 1), ('zaxis', 1), ('vpref_mode', 1)]
ARGS = ('ids', 'pos', 'vel', 'heading', 'radius', 'pref_speed', 'goal', 'policy', 'zaxis', 'max_run_dist', 'goal_heading', 'sizes', 'obs_counts',
        'obs_pos', 'obs_radius', 'path_offsets', 'path_points')
DTYPE = dict(ids=np.int32, vel=np.float32, policy=np.uint8, zaxis=np.uint8, sizes=np.int32, obs_counts=np.int32, path_offsets=np.int32)


def section_table(max_n, max_m, W):
    t = [(name, row * max_n) for name, row in AGENT]
    t += [('new_size', 4 * max_n)]
    t += [('obs_head', 16 * max_n), ('obs_rec', 32 * max_m), ('obs_sorted', 32 * max_m), ('obs_perm', 4 * max_m), ('obs_tree', 128 * max_m), ('obs_wide', 256 * max_m)]
    t += [('attr_par', 64 * max_n), ('attr_nd', 8 * max_n), ('attr_triple', 24 * max_n), ('attr_class', max_n)]
    t += [('path_off', 4 * (max_n + 1) if W > 0 else 0), ('path_pts', 24 * W * max_n if W > 0 else 0)]
    begin, at = {}, 0
    for name, size in t:
        begin[name] = at
        at += (size + 63) // 64 * 64
    return t, begin, at


@pytest.fixture(scope='module')
def H():
    h = load_harness('scenes_harness', ('sca_forms.h', 'sca_scenes.h', 'sca_scene_restart.h'))
    h.restart_block_sections.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    h.restart_pack_block.restype = None
    h.restart_pack_block.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8
    h.restart_refusal.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int]
    return h


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pointers(call):
    keep = [None if call.get(k) is None else np.ascontiguousarray(call[k], DTYPE.get(k, np.float64)) for k in ARGS]
    return keep, (C.c_void_p * len(ARGS))(*[None if a is None else a.ctypes.data for a in keep])


@pytest.mark.parametrize('max_n,max_m,W', [(MAX_N, MAX_M, 0), (MAX_N, MAX_M, 2), (1, 0, 0), (130, 9, 5), (1536, 1491, 3)])
def test_block_layout_is_the_section_table(H, max_n, max_m, W):
    """restart_block_layout against the table: the order of the parts, the new sizes one int32 per row of max_n behind the agent sections,
    every section on a 64-byte boundary, none overlapping, the total the end of the last"""
    t, begin, total = section_table(max_n, max_m, W)
    b, s, tot = (C.c_int64 * 32)(), (C.c_int64 * 32)(), C.c_int64(0)
    k = H.restart_block_sections(max_n, max_m, W, b, s, C.byref(tot))
    assert k == len(t) == 26
    assert [(b[i], s[i]) for i in range(k)] == [(begin[name], size) for name, size in t]
    assert tot.value == total
    for i in range(k):
        assert b[i] % 64 == 0 and b[i] + s[i] <= (b[i + 1] if i + 1 < k else tot.value)


def restate(call, h_size, tracker_on, W):
    """the block and the plan of a call that has passed the checks, from the section table and include/sca_hip.h"""
    _, begin, total = section_table(MAX_N, MAX_M, W)
    blk = np.full(total, FILL, np.uint8)

    def put(name, a, dt):
        raw = np.ascontiguousarray(a, dt).reshape(-1).view(np.uint8)
        blk[begin[name]:begin[name] + raw.size] = raw
    ids, sizes = list(call['ids']), call.get('sizes')
    rows = [int(sizes[e]) if sizes is not None else OFFSETS[s + 1] - OFFSETS[s] for e, s in enumerate(ids)]
    start = [sum(rows[:e]) for e in range(len(ids))]
    T = sum(rows)
    put('ids', ids, np.int32); put('start', start, np.int32); put('new_size', rows, np.int32)
    after, size_now = list(POLICY_NOW), list(h_size)
    pol = np.zeros(T, np.uint8)
    for e, s in enumerate(ids):
        size_now[s] = rows[e]
        for j in range(rows[e]):
            pol[start[e] + j] = after[OFFSETS[s] + j] = POLICY_NOW[OFFSETS[s] + j] if call.get('policy') is None else call['policy'][start[e] + j]
    put('policy', pol, np.uint8)
    put('vpref_mode', [1 if tracker_on and p in TRACKED else 0 for p in pol], np.uint8)
    put('pos', call['pos'], np.float64); put('heading', call['heading'], np.float64)
    put('vel', np.zeros((T, 3)) if call.get('vel') is None else call['vel'], np.float32)
    has = 0
    for name in ('goal', 'goal_heading', 'radius', 'pref_speed', 'max_run_dist', 'zaxis'):
        if call.get(name) is not None:
            put(name, call[name], DTYPE.get(name, np.float64))
            has |= HAS[name]
    path_len, path_vpref = [], []
    if W > 0:
        has |= HAS['path_slots']
        po = call.get('path_offsets')
        if po is not None:
            has |= HAS['paths']
            put('path_off', po, np.int32)
            if po[-1] > 0:
                put('path_pts', call['path_points'], np.float64)
        for e, s in enumerate(ids):
            for j in range(OFFSETS[s + 1] - OFFSETS[s]):
                n = int(po[start[e] + j + 1] - po[start[e] + j]) if po is not None and j < rows[e] else 0
                path_len.append(n)
                path_vpref.append(1 if n > 0 and pol[start[e] + j] not in TRACKED else 0)
    head, at = [], 0
    for e, s in enumerate(ids):
        ms = -1 if call.get('obs_counts') is None else int(call['obs_counts'][e])
        base = OBS_CAP[s] if ms >= 0 else 0
        head += [ms, base, at, 2 * base if ms > 0 else -1]
        at += max(ms, 0)
    put('obs_head', head, np.int32)
    policy_changed, size_changed = after != POLICY_NOW, any(rows[e] != h_size[s] for e, s in enumerate(ids))
    lp = [a for s in range(3) for a in range(OFFSETS[s], OFFSETS[s] + size_now[s]) if after[a] == LP] if policy_changed or size_changed else []
    plan = dict(has=has, policy_changed=policy_changed, size_changed=size_changed, T=T, size_now=size_now, lp=lp, path_len=path_len, path_vpref=path_vpref,
                max_radius=0.0 if call.get('radius') is None else float(np.max(call['radius'])),
                max_pref_speed=0.0 if call.get('pref_speed') is None else float(np.max(call['pref_speed'])))
    return blk, plan


def packed(H, call, h_size, tracker_on, W):
    total = section_table(MAX_N, MAX_M, W)[2]
    blk = np.full(total, FILL, np.uint8)
    keep, ptrs = pointers(call)
    out, size_now, lp = np.zeros(6, np.int32), np.zeros(3, np.int32), np.full(8, -7, np.int32)
    plen, pvp, mx = np.full(8, -7, np.int32), np.full(8, 9, np.uint8), np.zeros(2)
    H.restart_pack_block(MAX_N, MAX_M, W, 3, vp(np.array(OFFSETS, np.int32)), int(tracker_on), vp(np.array(POLICY_NOW, np.uint8)), vp(np.array(h_size, np.int32)),
                         vp(np.array(OBS_CAP, np.int32)), len(call['ids']), ptrs, vp(blk), vp(out), vp(size_now), vp(lp), vp(plen), vp(pvp), vp(mx))
    del keep
    plan = dict(has=int(out[0]), policy_changed=bool(out[1]), size_changed=bool(out[2]), T=int(out[3]), size_now=size_now.tolist(), lp=lp[:out[4]].tolist(),
                path_len=plen[:out[5]].tolist(), path_vpref=pvp[:out[5]].tolist(), max_radius=float(mx[0]), max_pref_speed=float(mx[1]))
    return blk, plan


def episode(T, seed, optional=True, vel=True, policy=None):
    r = np.random.default_rng(seed)
    e = dict(pos=r.normal(size=(T, 3)), heading=r.normal(size=(T, 3)), vel=r.normal(size=(T, 3)).astype(np.float32) if vel else None, policy=policy)
    if optional:
        e.update(goal=r.normal(size=(T, 3)), goal_heading=r.normal(size=(T, 3)), radius=r.uniform(0.2, 0.9, T), pref_speed=r.uniform(0.5, 2.0, T),
                 max_run_dist=r.uniform(10.0, 50.0, T), zaxis=r.integers(0, 2, T).astype(np.uint8))
    return e


FULL = [3, 1, 4]
ALL_SIX = 1 | 2 | 4 | 8 | 16 | 32
# name: (the call, the sizes as they stand, tracker on, W, what the plan must say beside the restatement -- worked out by hand)
CASES = {
    'a_all_full_out_of_order': (dict(ids=[2, 0, 1], **episode(8, 1)), FULL, True, 0, dict(has=ALL_SIX, T=8, lp=[], size_changed=False, policy_changed=False)),
    'b_sized_partial_and_full': (dict(ids=[2, 1], sizes=[2, 1], **episode(3, 2)), FULL, False, 0, dict(T=3, size_now=[3, 1, 2], size_changed=True, lp=[1, 3])),
    'c_every_optional_null': (dict(ids=[0], **episode(3, 3, optional=False, vel=False)), FULL, True, 0, dict(has=0, T=3, max_radius=0.0, max_pref_speed=0.0)),
    'd_every_optional_present': (dict(ids=[1, 2], **episode(5, 4, policy=[4, 1, 5, 4, 2])), FULL, True, 0, dict(has=ALL_SIX, T=5, policy_changed=False)),
    'e_slots_without_path_arrays': (dict(ids=[0, 2], **episode(7, 5, optional=False)), FULL, True, 2, dict(has=256, path_len=[0] * 7, path_vpref=[0] * 7)),
    'e_slots_with_lists_0_1_2': (dict(ids=[0], path_offsets=[0, 0, 1, 3], path_points=np.arange(9.0).reshape(3, 3), **episode(3, 6, optional=False)), FULL, True, 2,
                                 dict(has=256 | 512, path_len=[0, 1, 2], path_vpref=[0, 1, 1])),
    'e_lists_in_a_partial_scene': (dict(ids=[2, 0], sizes=[2, 3], path_offsets=[0, 2, 2, 3, 3, 5], path_points=np.arange(15.0).reshape(5, 3),
                                        **episode(5, 7, optional=False, policy=[0, 1, 5, 3, 2])), FULL, True, 2,
                                   dict(path_len=[2, 0, 0, 0, 1, 0, 2], path_vpref=[0, 0, 0, 0, 0, 0, 1], size_now=[3, 1, 2])),
    'f_obstacle_counts_keep_0_2': (dict(ids=[0, 1, 2], obs_counts=[-1, 0, 2], obs_pos=np.ones((2, 3)), obs_radius=np.ones(2), **episode(8, 8, optional=False)), FULL, True, 0,
                                   dict(has=0)),
    'f_two_sets_replaced': (dict(ids=[2, 0], obs_counts=[2, 1], obs_pos=np.ones((3, 3)), obs_radius=np.ones(3), **episode(7, 9, optional=False)), FULL, True, 0, dict(T=7)),
    'g_policy_moves_agents_in_and_out': (dict(ids=[0], **episode(3, 10, policy=[4, 1, 3])), FULL, True, 0,
                                         dict(policy_changed=True, size_changed=False, lp=[0, 3, 6], size_now=FULL)),
    'g_size_drops_an_lp_agent': (dict(ids=[2], sizes=[2], **episode(2, 11)), FULL, True, 0, dict(policy_changed=False, size_changed=True, lp=[1, 3], size_now=[3, 1, 2])),
    'g_size_brings_it_back': (dict(ids=[2], **episode(4, 12)), [3, 1, 2], False, 0, dict(policy_changed=False, size_changed=True, lp=[1, 3, 6], size_now=FULL)),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_pack_against_the_restatement(H, name):
    call, h_size, tracker_on, W, by_hand = CASES[name]
    want_blk, want = restate(call, h_size, tracker_on, W)
    got_blk, got = packed(H, call, h_size, tracker_on, W)
    for k, v in by_hand.items():
        assert want[k] == v, (k, want[k])                            # the restatement itself against the figures worked out by hand
    assert got == want
    diff = np.flatnonzero(got_blk != want_blk)
    assert diff.size == 0, 'the block differs first at byte %d' % diff[0]


def test_head_words_of_the_three_counts(H):
    """obs_counts -1, 0 and 2 for scenes of obstacle base 0, 2 and 2: {-1, 0, at, -1}, {0, base, at, -1} and {2, base, at, 2 * base}"""
    call = CASES['f_obstacle_counts_keep_0_2'][0]
    blk, _ = packed(H, call, FULL, True, 0)
    begin = section_table(MAX_N, MAX_M, 0)[1]['obs_head']
    assert blk[begin:begin + 48].view(np.int32).tolist() == [-1, 0, 0, -1, 0, 2, 0, -1, 2, 2, 0, 4]
    blk, _ = packed(H, CASES['f_two_sets_replaced'][0], FULL, True, 0)
    assert blk[begin:begin + 32].view(np.int32).tolist() == [2, 2, 0, 4, 1, 0, 2, 0]              # the second set's rows start behind the first's two


# ---- the refusals' texts --------------------------------------------------------------------------------------------------------------------
# (which check, fault, entry, total): the text, literally as sca_hip.hip's restart_scenes() held it before the texts moved to
# sca_scene_restart.h, for scene_ids = [2, 7, 2], sizes = [9, 1, 1], obs_counts = [5, -3, 0], path_offsets = [0, 4, 3], struct_bytes 12, W 2
REFUSALS = [
    ((0, 1, -1, 0), ERR_STATE, 'sca_restart_scenes: no scenes -- sca_set_scenes first'),
    ((0, 2, -1, 0), ERR_STATE, 'sca_restart_scenes: no state yet -- sca_set_state first'),
    ((0, 3, -1, 0), ERR_STATE, 'sca_restart_scenes between a policy pass and its env update: finish the step first'),
    ((0, 4, -1, 0), ERR_ARG, 'sca_restart_scenes: count must be positive and scene_ids not NULL'),
    ((0, 5, 1, 0), ERR_ARG, 'sca_restart_scenes: scene_ids[1] = 7 is not a scene of this context (0 .. 2)'),
    ((0, 6, 2, 0), ERR_ARG, 'sca_restart_scenes: scene_ids[2] = 2 is named twice'),
    ((0, 7, -1, 8), ERR_ARG, 'sca_restart_scenes: pos and heading must not be NULL'),
    ((0, 8, 5, 8), ERR_ARG, 'sca_restart_scenes: row 5 holds a number that is not finite'),
    ((0, 9, 6, 8), ERR_ARG, 'sca_restart_scenes: row 6 has a policy above SCA_POLICY_RVO3D_DUBINS'),
    ((0, 10, 7, 8), ERR_ARG, 'sca_restart_scenes: row 7 has a radius, pref_speed or max_run_dist that is not positive'),
    ((0, 11, -1, 8), ERR_ARG, 'sca_restart_scenes: goal_heading without a device tracker (sca_device_tracker_enable)'),
    ((0, 12, -1, 8), ERR_UNSUPPORTED, 'sca_restart_scenes with waypoint lists set (sca_set_paths): the lists are one block, replacing a scene\'s lists is not available'),
    ((0, 13, 3, 8), ERR_UNSUPPORTED, 'sca_restart_scenes: row 3 changes an agent between a tracked and an untracked policy while per-agent tracker attributes are set '
                                     '(sca_device_tracker_set_agent_params): the tracker\'s classes are cut by policy'),
    ((0, 14, 0, 0), ERR_ARG, 'sca_restart_scenes_sized: sizes[0] = 9: scene 2 holds 1 .. 4 agents (its capacity)'),
    ((1, 1, 0, 0), ERR_STATE, 'sca_restart_scenes_obstacles: obs_counts[0] = 5 but the context has no obstacle slots -- sca_set_scene_obstacle_slots first'),
    ((1, 2, 0, 0), ERR_ARG, 'sca_restart_scenes_obstacles: obs_counts[0] = 5: scene 2 keeps its set (-1) or takes 0 .. its obstacle capacity 2'),
    ((1, 3, -1, 6), ERR_ARG, 'sca_restart_scenes_obstacles: obs_pos and obs_radius must not be NULL with 6 obstacles'),
    ((1, 4, 4, 6), ERR_ARG, 'sca_restart_scenes_obstacles: obstacle row 4 has a position that is not finite'),
    ((1, 5, 3, 6), ERR_ARG, 'sca_restart_scenes_obstacles: obstacle row 3 has a radius that is not positive'),
    ((2, 1, -1, 0), ERR_ARG, 'sca_restart_scenes_attrs: attrs->struct_bytes = 12 is not a size of sca_restart_attrs (8 .. 88, whole pointers)'),
    ((2, 2, -1, 0), ERR_ARG, 'sca_restart_scenes_attrs: attrs->reserved must be 0'),
    ((2, 3, -1, 0), ERR_ARG, 'sca_restart_scenes_attrs: turning_radius / pitch_lo / pitch_hi without a device tracker (sca_device_tracker_enable)'),
    ((2, 4, 5, 0), ERR_ARG, 'sca_restart_scenes_attrs: row 5 has an attribute out of range (see sca_params)'),
    ((2, 5, 2, 0), ERR_ARG, 'sca_restart_scenes_attrs: row 2 has a turning radius / pitch limits out of range (R > 0, pitch_lo < pitch_hi)'),
    ((3, 1, -1, 0), ERR_STATE, 'sca_restart_scenes_paths: path arrays, but the context\'s lists are not in slot form -- sca_set_path_slots first'),
    ((3, 2, 0, 0), ERR_ARG, 'sca_restart_scenes_paths: path_offsets[0] must be 0'),
    ((3, 3, 1, 0), ERR_ARG, 'sca_restart_scenes_paths: path_offsets decrease at row 1'),
    ((3, 4, 0, 0), ERR_ARG, 'sca_restart_scenes_paths: row 0 brings a list of 4 waypoints, a row has room for 2 (sca_set_path_slots)'),
    ((3, 5, -1, 9), ERR_ARG, 'sca_restart_scenes_paths: path_points is NULL with 9 waypoints'),
    ((3, 6, 1, 9), ERR_ARG, 'sca_restart_scenes_paths: row 1 has a waypoint that is not finite'),
]


def test_every_refusal_text(H):
    assert sorted(k[:2] for k, _, _ in REFUSALS) == [(0, f) for f in range(1, 15)] + [(1, f) for f in range(1, 6)] + [(2, f) for f in range(1, 6)] + [(3, f) for f in range(1, 7)]
    keep, ptrs = pointers(dict(ids=[2, 7, 2], sizes=[9, 1, 1], obs_counts=[5, -3, 0], path_offsets=[0, 4, 3]))
    off, cap = np.array(OFFSETS, np.int32), np.array(OBS_CAP, np.int32)
    for (which, fault, entry, total), code, text in REFUSALS:
        out = C.create_string_buffer(512)
        rc = H.restart_refusal(which, fault, entry, total, 3, vp(off), 3, ptrs, vp(cap), 12, 2, out, 512)
        assert (rc, out.value.decode()) == (code, text), (which, fault)
    # without obstacle slots the capacity is not named
    out = C.create_string_buffer(512)
    H.restart_refusal(1, 2, 1, 0, 3, vp(off), 3, ptrs, None, 12, 2, out, 512)
    assert out.value.decode() == 'sca_restart_scenes_obstacles: obs_counts[1] = -3: scene 7 keeps its set (-1) or takes 0 .. its obstacle capacity'
    del keep


def test_restart_scenes_holds_no_text_and_the_harnesses_no_chain():
    """the entry point's body names no message, and no harness restates the block's chain with a literal size of the new sizes"""
    src = open(os.path.join(harness_util.CSRC, 'sca_hip.hip')).read()
    body = src[src.index('static int restart_scenes('):]
    body = body[:body.index('\n}\n') + 3]
    code = '\n'.join(line.split('//')[0] for line in body.split('\n'))
    assert '"' not in code and body.count('\n') < 100
    tests = os.path.join(harness_util.ROOT, 'tests')
    for f in os.listdir(tests):
        if f.endswith('.cpp'):
            assert '4 * (int64_t)max_n' not in open(os.path.join(tests, f)).read(), f


# ---- the harness as a program under the sanitizers --------------------------------------------------------------------------------------
def test_standalone_under_sanitizers():
    """restart_block_layout and restart_pack as a program of their own (its main packs the cases above from heap arrays of exactly the rows
    a call may read into a heap block of exactly the layout's bytes) under -fsanitize=address,undefined.  Host code only; nothing of it is
    loaded into python."""
    exe = os.path.join(harness_util.BUILD, 'scenes_harness_san')
    os.makedirs(harness_util.BUILD, exist_ok=True)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan',
                           '-static-libubsan', '-DSCENES_MAIN', '-Wall', '-Wextra', '-Werror', '-I' + harness_util.CSRC, '-o', exe,
                           os.path.join(harness_util.ROOT, 'tests', 'scenes_harness.cpp')])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'scenes_harness: ok' in r.stdout and 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr
