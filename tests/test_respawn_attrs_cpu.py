"""A respawn that brings policy and solver attributes (sca_respawn_agents_attrs) without a GPU: the pure rules of
sca_amd/csrc/sca_respawn_attrs.h, compiled for the host behind tests/respawn_attrs_harness.cpp -- every outcome of respawn_attrs_check with
its code, the block layout, the host-compiled row write (the functions k_respawn_attrs calls per row) against the Python rule of
tests/respawn_attrs_rule.py over the corpus, the ORCA3D-LP list, the harness as a program of its own under the sanitizers, the symbols,
and what the corpus holds (counted from the oracle and the rule alone)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import form_fuzz as F
import harness_util
import respawn_attrs_rule as RA
import respawn_rule as RR

SRC = os.path.join(harness_util.ROOT, 'tests', 'respawn_attrs_harness.cpp')
FLAGS = ['-std=c++17', '-ffp-contract=off', '-mfma', '-fno-builtin-pow', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I' + harness_util.CSRC]
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5                   # include/sca_hip.h
RSP_OK, RSP_NO_AGENTS, RSP_MID_STEP, RSP_BAD_COUNT, RSP_NO_ARRAYS, RSP_BAD_ID, RSP_REPEATED_ID, RSP_GOAL_HEADING, RSP_SCENES = 0, 1, 3, 4, 5, 6, 7, 10, 16   # RespawnFault
OK, BAD_POLICY, STRUCT, RESERVED, NO_TRACKER, SOLVER, PLANNER = range(7)                                  # RespawnAttrFault
CTX_KEYS = ('agents', 'state', 'mid_step', 'scenes', 'comm', 'partition', 'n', 'shard_count', 'tracker_on', 'paths_block', 'path_W')
PAR_DTYPE = np.dtype([('neighbor_dist', np.float64), ('time_step', np.float64), ('time_horizon', np.float64), ('max_speed', np.float64),
                      ('cos_heading_thr', np.float64), ('dt_nominal', np.float64), ('max_neighbors', np.int32), ('pad', np.int32), ('range_sq', np.float64)])


class Attrs(C.Structure):                                          # sca_restart_attrs
    _fields_ = [('struct_bytes', C.c_int32), ('reserved', C.c_int32)] + \
               [(k, C.c_void_p) for k in ('neighbor_dist', 'max_neighbors', 'time_step', 'time_horizon', 'max_speed', 'max_heading_change', 'dt_nominal',
                                          'turning_radius', 'pitch_lo', 'pitch_hi')]


@pytest.fixture(scope='module')
def H():
    out = os.path.join(harness_util.BUILD, 'librespawn_attrs_harness.so')
    deps = [SRC, os.path.join(harness_util.ROOT, 'include', 'sca_hip.h')] + \
        [os.path.join(harness_util.CSRC, f) for f in ('sca_respawn_attrs.h', 'sca_respawn.h', 'sca_scenes.h', 'sca_core.h')]
    os.makedirs(harness_util.BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(['g++', '-O2', '-fPIC', '-shared'] + FLAGS + ['-o', out, SRC])
    h = C.CDLL(out)
    h.rsa_layout.restype = None
    h.rsa_layout.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    h.rsa_check.restype = None
    h.rsa_check.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    h.rsa_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 32 + [C.c_int] + [C.c_void_p] * 10
    h.rsa_table_new.restype = C.c_void_p
    h.rsa_table_free.argtypes = [C.c_void_p]
    h.rsa_table_step.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
    h.rsa_lp_list.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return h


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def ctx_of(**state):
    s = dict(agents=1, state=1, mid_step=0, scenes=0, comm=0, partition=0, n=10, shard_count=10, tracker_on=0, paths_block=0, path_W=0)
    s.update(state)
    return np.array([s[k] for k in CTX_KEYS], np.int32)


def check(H, ids=(0, 1, 2, 3), policy=None, desc=None, struct_bytes=None, reserved=0, policy_now=None, radius='ok', goal_heading=1, count=None, **state):
    """-> ((base fault, entry, code), (fault, entry, code), merged policies)"""
    c = ctx_of(**state)
    n = int(c[6])
    ids = np.ascontiguousarray(ids, np.int32)
    count = len(ids) if count is None else count
    policy_now = np.full(n, 3, np.uint8) if policy_now is None else np.ascontiguousarray(policy_now, np.uint8)
    policy = None if policy is None else np.ascontiguousarray(policy, np.uint8)
    radius = np.full(max(count, 1), 0.5) if isinstance(radius, str) else radius
    d, held = None, []
    if desc is not None:
        d = Attrs(struct_bytes=C.sizeof(Attrs) if struct_bytes is None else struct_bytes, reserved=reserved)
        for k, v in desc.items():
            held.append(np.ascontiguousarray(v, RA.dtype_of(k)))
            setattr(d, k, held[-1].ctypes.data)
    out, merged = np.zeros(6, np.int32), np.full(n, 255, np.uint8)
    H.rsa_check(vp(c), vp(policy_now), count, vp(ids), vp(policy), None if d is None else C.addressof(d), vp(radius), goal_heading, vp(out), vp(merged))
    return tuple(int(x) for x in out[:3]), tuple(int(x) for x in out[3:]), merged


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def test_every_outcome_of_the_check(H):
    assert check(H)[:2] == ((RSP_OK, -1, 0), (OK, -1, 0))
    # what respawn_check refuses comes first, with its codes -- the policy bytes are not even looked at
    six = [0, 6, 0, 0]
    assert check(H, policy=six, agents=0)[0] == (RSP_NO_AGENTS, -1, ERR_STATE)
    assert check(H, policy=six, mid_step=1)[0] == (RSP_MID_STEP, -1, ERR_STATE)
    assert check(H, policy=six, scenes=1)[0] == (RSP_SCENES, -1, ERR_UNSUPPORTED)
    assert check(H, policy=six, count=0)[0] == (RSP_BAD_COUNT, -1, ERR_ARG)
    assert check(H, policy=six, radius=None)[0] == (RSP_NO_ARRAYS, -1, ERR_ARG)
    assert check(H, ids=[0, 10, 2, 3], policy=six)[0] == (RSP_BAD_ID, 1, ERR_ARG)
    assert check(H, ids=[0, 1, 2, 1], policy=six)[0] == (RSP_REPEATED_ID, 3, ERR_ARG)
    # the policy byte
    assert check(H, policy=six)[1] == (BAD_POLICY, 1, ERR_ARG)
    assert check(H, policy=[5, 4, 3, 255])[1] == (BAD_POLICY, 3, ERR_ARG)
    # goal_heading is judged by the NEW policy: rows 3 (ORCA3D) become SCA under the tracker
    assert check(H, policy=[3, 3, 0, 3], goal_heading=0, tracker_on=1)[0] == (RSP_GOAL_HEADING, 2, ERR_ARG)
    assert check(H, policy=[3, 3, 0, 3], goal_heading=0, tracker_on=0)[:2] == ((RSP_OK, -1, 0), (OK, -1, 0))
    now = np.array([0, 5, 0, 5, 3, 3, 3, 3, 3, 3], np.uint8)          # tracked rows that all leave: no goal_heading needed; without policy: needed
    assert check(H, policy=[3, 1, 2, 4], policy_now=now, goal_heading=0, tracker_on=1)[:2] == ((RSP_OK, -1, 0), (OK, -1, 0))
    assert check(H, policy_now=now, goal_heading=0, tracker_on=1)[0] == (RSP_GOAL_HEADING, 0, ERR_ARG)
    # the descriptor
    nd = dict(neighbor_dist=np.full(4, 4.0))
    full = C.sizeof(Attrs)
    for sb in (0, 4, 7, 12, 20, full + 8, full + 1):
        assert check(H, desc=nd, struct_bytes=sb)[1] == (STRUCT, -1, ERR_ARG), sb
    for sb in (8, 16, 8 + 7 * 8, full):
        assert check(H, desc=nd, struct_bytes=sb)[1] == (OK, -1, 0), sb
    assert check(H, desc=nd, reserved=2)[1] == (RESERVED, -1, ERR_ARG)
    # (a size that ends in front of the planner's arrays: they read as NULL)
    assert check(H, desc=dict(turning_radius=np.full(4, 2.0)), struct_bytes=8 + 7 * 8)[1] == (OK, -1, 0)
    assert check(H, desc=dict(turning_radius=np.full(4, 2.0)))[1] == (NO_TRACKER, -1, ERR_ARG)
    # planner attributes under the tracker: judged for the rows whose NEW policy is tracked, by sca_device_tracker_set_agent_params' rules
    trk = dict(tracker_on=1, policy=[3, 0, 3, 5])
    assert check(H, desc=dict(pitch_hi=np.full(4, 0.5)), **trk)[1] == (OK, -1, 0)
    assert check(H, desc=dict(turning_radius=[0.0, 2.0, -1.0, 2.0]), **trk)[1] == (OK, -1, 0)            # (rows 0 and 2 are untracked: ignored)
    assert check(H, desc=dict(turning_radius=[2.0, 0.0, 2.0, 2.0]), **trk)[1] == (PLANNER, 1, ERR_ARG)
    assert check(H, desc=dict(turning_radius=[2.0, 2.0, 2.0, np.nan]), **trk)[1] == (PLANNER, 3, ERR_ARG)
    assert check(H, desc=dict(pitch_lo=[0.0, 0.8, 0.0, 0.0]), **trk)[1] == (PLANNER, 1, ERR_ARG)          # (pitch_hi NULL: the tracker's 0.785)
    assert check(H, desc=dict(pitch_lo=np.full(4, -0.5), pitch_hi=[0.5, 0.5, 0.5, np.inf]), **trk)[1] == (PLANNER, 3, ERR_ARG)
    assert check(H, desc=dict(turning_radius=[2.0, 0.0, 2.0, 2.0]), tracker_on=1)[1] == (OK, -1, 0)       # (the rows keep ORCA3D: nobody is tracked)
    bad = lambda v, j: np.concatenate([np.full(j, v[0]), [v[1]], np.full(3 - j, v[0])])
    for k, (good, wrong) in dict(neighbor_dist=(4.0, 0.0), max_neighbors=(4, 0), time_step=(0.1, -0.1), time_horizon=(3.0, np.inf), max_speed=(1.0, np.nan),
                                 max_heading_change=(0.3, 3.2), dt_nominal=(0.1, 0.0)).items():
        for j in (0, 3):
            assert check(H, desc={k: bad((good, wrong), j)})[1] == (SOLVER, j, ERR_ARG), (k, j)
    assert check(H, desc=dict(max_neighbors=[1, 16, 17, 1]))[1] == (SOLVER, 2, ERR_ARG)
    assert check(H, desc=dict(max_heading_change=[0.0, np.pi, 0.3, 0.3]))[1] == (OK, -1, 0)
    # the merged policies
    merged = check(H, ids=[7, 2, 9, 0], policy=[0, 1, 2, 4])[2]
    assert merged.tolist() == [4, 3, 1, 3, 3, 3, 3, 0, 3, 2]
    assert check(H, ids=[7, 2, 9, 0])[2].tolist() == [3] * 10


def test_layout(H):
    assert H.rsa_sections() == 5
    for cap in (1, 63, 64, 65, 257):
        off, total = np.zeros(5, np.int64), np.zeros(1, np.int64)
        H.rsa_layout(cap, vp(off), vp(total))
        sizes = [cap, 64 * cap, 8 * cap, 24 * cap, cap]
        assert off[0] == 0 and all(o % 64 == 0 for o in off) and total[0] % 64 == 0, cap
        for s in range(5):
            end = off[s + 1] if s < 4 else total[0]
            assert off[s] + sizes[s] <= end < off[s] + sizes[s] + 64, (cap, s)


def test_lp_list(H):
    rng = np.random.default_rng(2)
    for n in (1, 9, 300):
        policy = rng.integers(0, 6, n).astype(np.uint8)
        want = np.flatnonzero(policy == 4).astype(np.int32)
        for now in (want, want[:-1] if len(want) else np.array([0], np.int32), np.zeros(0, np.int32)):
            now = np.ascontiguousarray(now, np.int32)
            out, ln = np.zeros(n, np.int32), C.c_int(0)
            changed = H.rsa_lp_list(vp(policy), n, vp(now), len(now), vp(out), C.byref(ln))
            assert np.array_equal(out[:ln.value], want) and changed == (not np.array_equal(now, want)), n


# ---- the row write -----------------------------------------------------------------------------------------------------------------------
def par_rows(table_rows):
    """AgentPar records of attribute rows (the test's own derivation: range_sq the square, the threshold the cosine -- the harness only
    carries the records)"""
    k = len(table_rows['neighbor_dist'])
    p = np.zeros(k, PAR_DTYPE)
    for nm in ('neighbor_dist', 'time_step', 'time_horizon', 'max_speed', 'dt_nominal', 'max_neighbors'):
        p[nm] = table_rows[nm]
    p['cos_heading_thr'] = np.cos(table_rows['max_heading_change'])
    p['range_sq'] = table_rows['neighbor_dist'] ** 2
    return p


def apply_harness(H, n, policy_now, m, par, st, defs, dev, tracker_on=0, path_vpref=None, trip=None, cls=None):
    c = ctx_of(n=n, shard_count=n, tracker_on=tracker_on)
    k = len(m['ids'])
    path_vpref = np.zeros(n, np.uint8) if path_vpref is None else path_vpref
    bits = np.zeros(k, np.uint8)
    pol = None if m.get('policy') is None else np.ascontiguousarray(m['policy'], np.uint8)
    keep = [np.ascontiguousarray(m[q], np.float32 if q == 'vel' else np.float64) for q in ('pos', 'vel', 'heading', 'radius', 'pref_speed', 'goal', 'max_run_dist')]
    gh = np.ascontiguousarray(m.get('goal_heading', np.zeros((k, 3))), np.float64)
    delta = H.rsa_apply(vp(c), vp(policy_now), vp(path_vpref), k, vp(m['ids']), vp(pol), vp(par), *[vp(x) for x in keep], vp(gh),
                        vp(st['pos']), vp(st['vel']), vp(st['flags']), vp(defs['radius']), vp(st['heading']), vp(defs['goal']), vp(defs['pref_speed']), vp(defs['max_run_dist']),
                        vp(st['total_dist']), vp(st['step_num']), vp(dev['status']), vp(dev['nbr_n']), vp(dev['near_n']), vp(dev['zaxis']), vp(dev['vpref_mode']),
                        vp(dev['nbr_valid']), vp(dev['vpref_ext']), vp(dev.get('trk_nbr0')), vp(dev.get('trk_goal_heading')), vp(dev.get('trk_st')), vp(dev.get('trk_init')),
                        dev.get('trk_words', 0), vp(dev['policy']), vp(dev['ap']), vp(dev['ap_nd']), vp(bits),
                        vp(trip), vp(cls), vp(dev.get('trk_R')), vp(dev.get('trk_plo')), vp(dev.get('trk_phi')), vp(dev.get('trk_cls')))
    return delta, bits


def device_rows(n, policy, table, tracker=False, words=37):
    dev = dict(status=np.full(n, 8, np.int32), nbr_n=np.full(n, 4, np.int32), near_n=np.full(n, 2, np.int32), zaxis=np.zeros(n, np.uint8),
               vpref_mode=RA.vmode_of(policy) if tracker else np.full(n, 1, np.uint8), nbr_valid=np.ones(n, np.uint8), vpref_ext=np.full((n, 3), 7.0),
               policy=policy.copy(), ap=par_rows(table), ap_nd=table['neighbor_dist'].copy())
    if tracker:
        dev.update(trk_nbr0=np.full(n, 2.0), trk_goal_heading=np.zeros((n, 3)), trk_st=np.full((n, words), 9, np.uint32), trk_init=np.arange(1, words + 1, dtype=np.uint32),
                   trk_words=words, trk_R=np.full(n, 1.5), trk_plo=np.full(n, -0.7), trk_phi=np.full(n, 0.7), trk_cls=np.full(n, 15, np.uint8))
    return dev


def test_row_write_against_the_python_rule_on_the_corpus(H, oracle):
    """every call of the corpus (seeds 0 .. 39) through the host-compiled row write: the state and the definition become respawn_rule.apply's,
    policy and records respawn_attrs_rule.apply_brings', every other row keeps every word; with a tracker, rows that enter take the
    initial record, mode 1 and a zero v_pref, rows that leave the initial record, mode 0 and a zero v_pref"""
    calls = 0
    for seed in RR.SEEDS:
        scene = F.random_scene(seed)
        n = scene['n']
        if n > 400 and seed % 4:
            continue                                                       # (the largest scenes: every fourth)
        run = RA.oracle_run(oracle, scene, RR.STEPS)
        for tracker in (0, 1):
            for t, r in enumerate(run):
                m = r['mission']
                if m is None:
                    continue
                calls += 1
                ids = m['ids']
                before = run[t - 1] if t else None
                st = {k: np.array((before or dict(scene, total_dist=np.zeros(n), step_num=np.zeros(n, np.int32)))[k], copy=True) for k in F.STATE_KEYS}
                st['flags'] = np.ascontiguousarray(st['flags'], np.uint8)
                defs = {k: np.array((before['defs'] if before else scene)[k], np.float64, copy=True) for k in RR.DEF_KEYS}
                dev = device_rows(n, r['policy_before'], r['table_before'], tracker=bool(tracker))
                was_done = int(((st['flags'][ids] & 7) != 0).sum())
                want_st, want_defs = {k: v.copy() for k, v in st.items()}, {k: v.copy() for k, v in defs.items()}
                RR.apply(want_st, want_defs, m)
                rows = {nm: r['table'][nm][ids] for nm in RA.ATTR_NAMES}
                par = par_rows(rows) if m['attrs'] is not None else None
                others = np.setdiff1d(np.arange(n), ids)
                keep_dev = {k: np.array(v, copy=True) for k, v in dev.items() if isinstance(v, np.ndarray)}
                trip = cls = None
                if tracker and m['planner'] is not None:                # the planner triples travel, with class bytes of the test's own
                    trip, cls = np.ascontiguousarray(m['planner']), (np.arange(len(ids)) % 16).astype(np.uint8)
                delta, bits = apply_harness(H, n, r['policy_before'], m, par, st, defs, dev, tracker_on=tracker, trip=trip, cls=cls)
                at = (seed, t, tracker)
                assert delta == was_done, at
                for k in F.STATE_KEYS:
                    assert np.array_equal(st[k], want_st[k]), at + (k,)
                for k in RR.DEF_KEYS:
                    assert np.array_equal(defs[k], want_defs[k]), at + (k,)
                assert np.array_equal(dev['policy'], r['policy']), at
                want_ap = par_rows(r['table']) if m['attrs'] is not None else keep_dev['ap']
                assert dev['ap'].tobytes() == want_ap.tobytes() and np.array_equal(dev['ap_nd'], want_ap['neighbor_dist']), at
                for k, v in keep_dev.items():
                    if k != 'trk_init':
                        assert np.array_equal(dev[k][others], v[others]), at + (k, 'a row that was not named')
                assert not dev['nbr_valid'][ids].any() and not dev['status'][ids].any() and (dev['near_n'][ids] == -1).all(), at
                was, now = np.isin(r['policy_before'][ids], RA.TRACKED), np.isin(m['policy'], RA.TRACKED)
                if tracker:
                    moved = was | now
                    assert np.array_equal(bits, now * 1 + (was & ~now) * 6), at
                    assert np.array_equal(dev['vpref_mode'][ids], now.astype(np.uint8)), at
                    assert (dev['vpref_ext'][ids][moved] == 0.0).all() and (dev['vpref_ext'][ids][~moved] == 7.0).all(), at
                    assert (dev['trk_st'][ids][moved] == dev['trk_init']).all() and (dev['trk_st'][ids][~moved] == 9).all(), at
                    assert (dev['trk_nbr0'][ids] == -1.0).all(), at
                    if trip is not None:
                        assert np.array_equal(np.stack([dev['trk_R'][ids], dev['trk_plo'][ids], dev['trk_phi'][ids]], 1), trip) and np.array_equal(dev['trk_cls'][ids], cls), at
                    else:
                        assert (dev['trk_R'][ids] == 1.5).all() and (dev['trk_cls'][ids] == 15).all(), at
                else:
                    assert not bits.any() and (dev['vpref_mode'][ids] == 1).all() and (dev['vpref_ext'][ids] == 7.0).all(), at
    assert calls >= 300, calls                                             # (each call of the corpus twice: without and with a tracker)


def test_mode_reset_follows_the_old_list_state_and_the_new_policy(H):
    """RSP_BIT_MODE_RESET: a straight-line row whose v_pref k_waypoint was writing goes back to mode 0 whatever it becomes -- unless the device
    tracker takes it (mode 1)"""
    n = 6
    policy_now = np.array([3, 3, 3, 0, 3, 1], np.uint8)
    path_vpref = np.array([1, 1, 1, 0, 0, 1], np.uint8)
    m = dict(ids=np.arange(6, dtype=np.int32), pos=np.ones((6, 3)), vel=np.zeros((6, 3), np.float32), heading=np.zeros((6, 3)), radius=np.full(6, 0.5),
             pref_speed=np.ones(6), goal=np.full((6, 3), 4.0), max_run_dist=np.full(6, 9.0), policy=np.array([3, 0, 5, 3, 0, 1], np.uint8), attrs=None)
    for tracker, want_bits, want_mode in ((0, [2, 2, 2, 0, 0, 2], [0, 0, 0, 1, 1, 0]), (1, [2, 1, 1, 6, 1, 2], [0, 1, 1, 0, 1, 0])):
        st = dict(pos=np.zeros((n, 3)), vel=np.zeros((n, 3), np.float32), heading=np.zeros((n, 3)), flags=np.zeros(n, np.uint8), total_dist=np.zeros(n),
                  step_num=np.zeros(n, np.int32))
        defs = dict(radius=np.ones(n), pref_speed=np.ones(n), goal=np.zeros((n, 3)), max_run_dist=np.ones(n))
        dev = device_rows(n, policy_now, RA.context_table(n), tracker=bool(tracker))
        dev['vpref_mode'][:] = 1
        _, bits = apply_harness(H, n, policy_now, m, None, st, defs, dev, tracker_on=tracker, path_vpref=path_vpref)
        assert bits.tolist() == want_bits and dev['vpref_mode'].tolist() == want_mode, tracker


# ---- the tracker's classes in a plain context ----------------------------------------------------------------------------------------------
def test_class_table_on_a_masked_plain_context(H, oracle):
    """scene_class_table's rule over a plain context by a mask (plain_class_table), call after call over the corpus' planner draws: against
    the scene form on the same rows compacted (classes, users, the masked tracked rows' bytes), and against the model's count of distinct
    triples -- more than 16 go to the per-agent form, 16 or fewer come back, a class keeps its index while a row uses it"""
    passed = back = 0
    for seed in RR.SEEDS:
        scene = F.random_scene(seed)
        n = scene['n']
        run = RA.oracle_run(oracle, scene, RR.STEPS)
        for masked in (False, True):
            mask = (np.random.default_rng(seed).random(n) < 0.7).astype(np.uint8) if masked else None
            if masked and not mask.any():
                continue
            h = H.rsa_table_new()
            try:
                cls, many, out = np.zeros(n, np.uint8), False, np.zeros(3, np.int32)
                for t, r in enumerate(run):
                    if r['mission'] is None:
                        continue
                    before = cls.copy()
                    pol, trip = np.ascontiguousarray(r['policy']), np.ascontiguousarray(r['trip'])
                    assert H.rsa_table_step(h, n, vp(mask), vp(pol), vp(trip), vp(cls), None, vp(out)) == 0, (seed, masked, t)
                    counted = np.isin(pol, RA.TRACKED) & (mask.astype(bool) if masked else True)
                    want = len({tuple(x) for x in trip[counted]})
                    assert bool(out[1]) == (want > RA.CLASS_CAP) and (out[1] or out[0] == want), (seed, masked, t, out, want)
                    if not out[1]:
                        assert (cls[counted] < 16).all() and len(set(cls[counted].tolist())) == want, (seed, masked, t)
                        for k in set(cls[counted].tolist()):           # one class, one triple
                            assert len({tuple(x) for x in trip[counted & (cls == k)]}) == 1, (seed, masked, t, k)
                        assert np.array_equal(cls[~counted], before[~counted]), (seed, masked, t, 'a row that does not count')
                    if not masked:
                        passed += int(out[1] and not many)
                        back += int(many and not out[1])
                    many = bool(out[1])
            finally:
                H.rsa_table_free(h)
    assert (passed, back) == (CORPUS['classes_pass_16'], CORPUS['classes_come_back']), (passed, back)


# ---- a program of its own ----------------------------------------------------------------------------------------------------------------
def test_standalone_under_sanitizers():
    """the harness as a stand-alone program (100 random calls, 1 / 63 / 64 / 65 / 257 rows first, every array on the heap in exactly its size)
    under -fsanitize=address,undefined.  Host code only; nothing of it is loaded into Python."""
    exe = os.path.join(harness_util.BUILD, 'respawn_attrs_harness_asan')
    os.makedirs(harness_util.BUILD, exist_ok=True)
    subprocess.check_call(['g++', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan',
                           '-DRESPAWN_ATTRS_MAIN'] + FLAGS + ['-o', exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and 'respawn_attrs_harness: ok' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the public face ---------------------------------------------------------------------------------------------------------------------
def test_the_symbols_and_the_kernel():
    hdr = open(os.path.join(harness_util.ROOT, 'include', 'sca_hip.h')).read()
    flat = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name, tail in (('sca_respawn_agents_attrs', r'path_points\s*\)'), ('sca_respawn_agents_gated_attrs', r'admitted\s*\)')):
        mm = re.search(name + r'\s*\(([^;]*?)' + tail, flat)
        assert mm, name
        args = [a.strip() for a in mm.group(0).split('(', 1)[1].split(',')]
        assert args[3].startswith('const uint8_t *policy') and args[4].startswith('const sca_restart_attrs *attrs'), args[:6]
        plain = re.search(name.replace('_attrs', '') + r'\s*\(([^;]*?)' + tail, flat).group(0).split('(', 1)[1].split(',')
        assert [a.strip() for a in plain] == args[:3] + args[5:], name     # sca_respawn_agents' arrays, unchanged, in its order
    kern = open(os.path.join(harness_util.CSRC, 'sca_respawn.hip.h')).read()
    body = kern[kern.index('void k_respawn_attrs('):kern.index('// ---- the finished list')]
    assert body.count('atomicAdd') == 1 and '__shared__' not in body and 'respawn_attrs_write_row' in body and 'respawn_write_row' in body


# ---- what the corpus holds ---------------------------------------------------------------------------------------------------------------
def test_what_the_corpus_holds(oracle):
    """the counts the GPU corpus test rests on, pinned: every one of the 36 ordered policy pairs and every other category occurs, and the
    grid's condition holds for every scene and step, so the grid leg leaves no scene out for its cell size"""
    total = dict.fromkeys(RA.QUANTITIES, 0)
    pairs = np.zeros((6, 6), np.int64)
    for seed in RR.SEEDS:
        scene = F.random_scene(seed)
        run = RA.oracle_run(oracle, scene, RR.STEPS)
        c, p = RA.corpus_counts(scene, run)
        for k in total:
            total[k] += c[k]
        pairs += p
        assert RA.grid_fits(scene, run), seed
    print('corpus', total, pairs.tolist())
    assert pairs.min() >= 1, pairs
    assert all(v >= 1 for v in total.values()), total
    assert pairs.sum() == total['respawns'] and total['policy_changes'] == pairs.sum() - np.trace(pairs)
    assert total == CORPUS and pairs.tolist() == PAIRS, (total, pairs.tolist())


# seeds 0 .. 39 x 12 steps
CORPUS = {'respawns': 35883, 'policy_changes': 29951, 'lp_enter': 5000, 'lp_leave': 5004, 'tracked_enter': 8002, 'tracked_leave': 7946,
          'max_neighbors_below_list': 9623, 'full_rows': 130, 'partial_descriptors': 76, 'no_descriptor': 69, 'grow_neighbor_dist': 28, 'grow_max_speed': 27,
          'grow_dt_nominal': 26, 'planner_calls': 95, 'classes_pass_16': 15, 'classes_come_back': 6}
# (old policy, new policy) over the respawned rows
PAIRS = [[983, 964, 1007, 1001, 997, 1001], [987, 984, 996, 1003, 1022, 1038], [1002, 1080, 1082, 955, 995, 1003], [996, 943, 1014, 976, 988, 981],
         [1015, 1021, 1022, 966, 955, 980], [997, 987, 985, 1007, 998, 952]]
