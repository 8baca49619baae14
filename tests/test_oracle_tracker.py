"""The oracle's Dubins planner and v_pref tracker (oracle/sca_dubins_oracle.c: dubinsmaneuver2d / dubinsmaneuver3d / compute_v_pref
restated from the reference on the host's own libm) -- first pinned to the reference's recorded plans and tracked episodes, bit for bit,
then used as the independent side against the product's host planner on seeded pose families (tests/tracker_poses.py).

Why a second restatement: the product's tracker (sca_amd/csrc/sca_dubins.hpp) runs on the restated glibc (sca_glibc_math.h) on the host
AND on the device, so the device-vs-host tests cannot see a fault the two builds share (a word, mod2pi, the candidate order, a libm
branch).  The oracle shares no code with it: a disagreement here is a fault on one side, and the recorded vectors say which."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN, fixture_agent_params, fixture_params, fixture_tracker_agent_params, load, static_inputs, tracked_param_fixtures
from tracker_poses import FAMILIES, poses, tracker_inputs

TRACKED_EPISODES = ['F1_sca_circle8', 'F2_sca_circle100', 'F2_rvodubins_circle100', 'F4_sca_takeoff16', 'F4_mixed_takeoff16',
                    'F10_sca_exp3_map', 'F13_fuzz_track_00', 'F13_fuzz_track_01', 'F13_fuzz_track_02', 'F13_fuzz_track_03',
                    'F15_sca_circle1024'] + tracked_param_fixtures()
# the fields of a sca_tracker_debug record the oracle restates (10: search rounds of the speculative kernels, 11: unused)
RECORD_FIELDS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23]


def _words(mode):
    return [sum(ord(c) << s for c, s in zip(mode[k:k + 3], (16, 8, 0))) for k in (0, 3)]


def test_oracle_planner_equals_reference_kats(oracle):
    """F7: the reference's planner on 42 poses (incl. the paper instance RLRRSL / 976.79)"""
    kats = json.load(open(os.path.join(GOLDEN, 'F7_dubins_kat.json')))
    for k in kats:
        r = oracle.dubins_plan(k['qi'], k['qf'], k['R'], k['pl'], ks=[0, k['n'] // 2, k['n'] - 1])
        assert r['mode'] == k['mode'] and r['length'] == k['length'] and r['count'] == k['n'], (k['mode'], r['mode'], r['length'], k['length'])
        assert np.array_equal(r['samples'], [k['first'], k['mid'], k['last']])


def _check_long_kats(oracle, k, rmin_of, pl_of, samples_of_c4=True):
    off = k['samples_off']
    for i in range(len(k['length'])):
        keep = off[i + 1] > off[i]
        n = int(k['n'][i])
        ks = np.arange(n) if keep else [0, n // 2, n - 1]
        r = oracle.dubins_plan(k['qi'][i], k['qf'][i], rmin_of(i), pl_of(i), ks=ks)
        assert r['mode'].encode() == k['mode'][i], (i, r['mode'], k['mode'][i])
        assert r['length'] == k['length'][i], (i, r['length'], k['length'][i])           # all 64 bits
        assert r['count'] == n and r['sampling'] == k['sampling'][i], i
        assert r['h_r'] == k['radii'][i, 0] and r['v_r'] == k['radii'][i, 1], i
        got_tpq = [r['h_t'], r['h_p'], r['h_q'], r['v_t'], r['v_p'], r['v_q']]
        assert np.array_equal(got_tpq, k['tpq'][i]), (i, got_tpq, k['tpq'][i])
        if keep:
            assert np.array_equal(r['samples'], k['samples'][off[i]:off[i + 1]]), i
        else:                                                                           # c4: first / mid / last of the 1001
            assert np.array_equal(r['samples'], [k['first'][i], k['mid'][i], k['last'][i]]), i


def test_oracle_planner_equals_reference_at_baseline_geometry(oracle):
    """F7b: 48 c4 plans (4.7 .. 39.8 km), 20 c2, 24 c5 -- every sample of the c2 / c5 plans"""
    k = dict(np.load(os.path.join(GOLDEN, 'F7b_dubins_kat_long.npz')))
    assert (k['samples_off'][1:] > k['samples_off'][:-1]).sum() >= 40
    _check_long_kats(oracle, k, lambda i: float(k['rmin']), lambda i: tuple(k['pitchlims']))


def test_oracle_planner_equals_reference_off_the_default_parameters(oracle):
    """F7c: Rmin 0.8 / 3 / 10 with four pitch-limit pairs, every sample"""
    k = dict(np.load(os.path.join(GOLDEN, 'F7c_dubins_kat_params.npz')))
    _check_long_kats(oracle, k, lambda i: float(k['set_rmin'][k['set'][i]]), lambda i: tuple(k['set_pitchlims'][k['set'][i]]))


@pytest.mark.parametrize('name', TRACKED_EPISODES)
def test_oracle_tracker_reproduces_reference_v_pref(name, oracle):
    """The replay of tests/test_tracker.py::test_tracker_reproduces_reference_v_pref with the oracle's tracker: open loop on the solver
    (states from the fixture), closed loop on the tracker's state; every V_des of the episode is the reference's bit for bit."""
    fx = load(name)
    st = static_inputs(fx)
    n = len(st['radius'])
    ext = st['vpref_mode'].astype(bool)
    params, trk = fixture_params(fx)
    tr = oracle.Tracker(fx['goal'][0], fx['goal6'][:, 3:6], st['pref_speed'], st['zaxis'],
                        neighbor_dist=params.get('neighbor_dist', 10.0), **trk)
    ap, tp = fixture_agent_params(fx), fixture_tracker_agent_params(fx)
    if 'neighbor_dist' in ap or tp:                                   # F17 / F18: every agent its own attributes
        tr.set_params(neighbor_dist=ap.get('neighbor_dist'), **tp)
    T = len(fx['step'])
    assert np.array_equal(fx['step'], np.arange(T))
    ever = np.zeros(n, bool)
    for t in range(T):
        active = fx['called'][t].astype(bool) & ext
        ever |= active
        got = tr.vpref(fx['pos'][t], fx['vel'][t], fx['heading'][t], active.astype(np.uint8), nthreads=4)
        assert np.array_equal(got[active], fx['vpref'][t][active]), (name, t, np.abs(got[active] - fx['vpref'][t][active]).max())
        tr.note_neighbors(fx['nbr_valid'][t], fx['nbr_n'][t], fx['nbr_dsq'][t])
    assert tr.replans()[ever].min() >= 1
    tr.close()


def records(get, n):
    o = np.zeros((n, 24))
    for i in range(n):
        get(i, o[i])
    return o


def compare_records(a, b, what):
    """two [n, 24] record arrays (product / oracle) on RECORD_FIELDS; returns the number of rows compared"""
    a, b = a[:, RECORD_FIELDS], b[:, RECORD_FIELDS]
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    bad = np.flatnonzero(~same.all(1))
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), [np.array(RECORD_FIELDS)[~same[i]].tolist() for i in bad[:3]])
    return len(a)


def oracle_first_plans(oracle, P, nthreads=0):
    """every pose's first compute_v_pref in the oracle's tracker: (V_des [n, 3], records [n, 24])"""
    pos, head, goal, gh = tracker_inputs(P)
    n = len(pos)
    tr = oracle.Tracker(goal, gh, 1.0, np.zeros(n, np.uint8))
    tr.set_params(turning_radius=P['rmin'], pitch_lo=P['pitch_lo'], pitch_hi=P['pitch_hi'])
    v = tr.vpref(pos, np.zeros((n, 3), np.float32), head, np.ones(n, np.uint8), nthreads=nthreads)
    rec = np.stack([tr.debug(i) for i in range(n)])
    tr.close()
    return v, rec


@pytest.mark.parametrize('family', FAMILIES)
def test_host_planner_equals_oracle_on_pose_families(family, oracle):
    """The product's host tracker (sca_tracker_vpref: the literal search on the restated glibc) against the oracle's (the reference's
    statements on the host's libm) on 6000 seeded poses: the whole plan record -- radii, t / p and length of both maneuvers, sampling
    size, sample count, the tracked node, v_pref, both words, candidates tried -- and the first V_des.  Then every sample of 60 of the
    plans through sca_dubins_plan, and the device's lean search compiled for the host on all of them."""
    from sca_amd import _lib, tracker
    P = poses(family, 6000, seed=1)
    n = len(P['q'])
    pos, head, goal, gh = tracker_inputs(P)
    vo, ro = oracle_first_plans(oracle, P)
    assert (ro[:, 11] == 0).all()                                     # every pose has a plan the reference would return
    tr = tracker.DubinsTracker(goal, gh, 1.0, np.zeros(n, np.uint8), nthreads=8)
    tr.set_agent_params(turning_radius=P['rmin'], pitch_lo=P['pitch_lo'], pitch_hi=P['pitch_hi'])
    vh = tr.vpref(pos, np.zeros((n, 3), np.float32), head, np.ones(n, np.uint8))
    L = _lib.lib()
    rh = records(lambda i, o: L.sca_tracker_debug(tr.h, i, _lib.ptr(o, C.c_double)), n)
    tr.close()
    assert np.array_equal(vh, vo), family
    compare_records(rh, ro, family)
    for i in np.random.default_rng(3).choice(n, 60, replace=False):
        cnt = int(ro[i, 13])
        length, mode, samples, ns = tracker.dubins_plan(P['q'][i, :5], P['q'][i, 5:], P['rmin'][i], (P['pitch_lo'][i], P['pitch_hi'][i]),
                                                        max_samples=cnt)
        r = oracle.dubins_plan(P['q'][i, :5], P['q'][i, 5:], P['rmin'][i], (P['pitch_lo'][i], P['pitch_hi'][i]), ks=np.arange(cnt))
        assert length == r['length'] and mode == r['mode'] and ns == cnt, (family, i)
        assert np.array_equal(samples, r['samples']), (family, i)
    # the lean search (what the device's lane kernels run) equals the literal one on these poses, for each (Rmin, pitch) set
    sets = np.stack([P['rmin'], P['pitch_lo'], P['pitch_hi']], 1)
    for s in np.unique(sets, axis=0):
        sel = np.flatnonzero((sets == s).all(1))
        q = np.ascontiguousarray(P['q'][sel])
        bad, lean, lit = C.c_int64(-1), C.c_int64(0), C.c_int64(0)
        assert L.sca_selftest_plan3d_lean(len(q), _lib.ptr(q, C.c_double), float(s[0]), float(s[1]), float(s[2]), C.byref(bad),
                                          C.byref(lean), C.byref(lit)) == 0
        assert bad.value == 0, (family, s)
    print(f'{family}: {n} plans, host tracker == oracle')


def test_pose_families_reach_their_cases(oracle):
    """the families do what tracker_poses.py says they do (so that a quiet change of the generator cannot empty a case)"""
    far = poses('far', 2000, seed=1)
    o = oracle.dubins_plan_batch(far['q'], far['rmin'], far['pitch_lo'], far['pitch_hi'])
    assert o[:, 0].min() > 5000 and (o[:, 14] == 0).all()
    assert (far['q'][:, 7] == far['q'][:, 2]).sum() > 100                          # exactly level
    st = poses('steep', 2000, seed=1)
    o = oracle.dubins_plan_batch(st['q'], st['rmin'], st['pitch_lo'], st['pitch_hi'])
    assert (o[:, 1] > 4 * st['rmin']).mean() > 0.3                                # the doubling ran: radii well above Rmin
    z = poses('zaxis', 500, seed=1)
    assert (z['q'][:, 5:7] == z['q'][:, 0:2]).all()
    hd = poses('headings', 2000, seed=1)
    o = oracle.dubins_plan_batch(hd['q'], hd['rmin'], hd['pitch_lo'], hd['pitch_hi'])
    assert ((o[:, 2] == 0) | (o[:, 4] == 0)).sum() > 100                           # t or q of the horizontal maneuver exactly 0
    pr = poses('params', 2000, seed=1)
    assert len(np.unique(np.stack([pr['rmin'], pr['pitch_lo'], pr['pitch_hi']], 1), axis=0)) == 16
