"""The device's Dubins tracker against the ORACLE's (oracle/sca_dubins_oracle.c: the reference's planner and compute_v_pref restated on the
host's own libm, pinned to the reference's recorded plans and episodes by tests/test_oracle_tracker.py).

The other device tracker tests compare the device with the host build of the same source (sca_dubins.hpp on the restated glibc) wherever
no recorded vector reaches -- c4 at N = 100 000, the re-plan kernel forms, random scenes.  A fault both builds share passes those.  Here the
other side shares no code with the product:
  * the first plan of tens of thousands of seeded poses per family (tests/tracker_poses.py) through every re-plan kernel form
    (k_replan_group<64 / 32 / 16 / 4>, the lane-per-plan k_replan; picked with the SCA_TRK_*_MAX ranges) and the per-agent form (more
    than 16 (turning radius, pitch limits) classes): the whole sca_device_tracker_debug record and the first V_des;
  * free-running SCA episodes (c2, c5 at 1024 agents, the 160-agent circle to the end): the product stepping resident with the tracker inside the pass, the oracle stepping its own loop (tracker ->
    orc_policy_step -> orc_env_update), nothing fed across; every step's state, the v_pref the pass used, the kd permutation, and the
    re-plan counts at the end;
  * c4 (N = 100 000) for four steps, open loop on the state: the v_pref the resident pass used against the oracle's."""
import ctypes as C

import numpy as np
import pytest

from test_oracle_tracker import compare_records, oracle_first_plans
from tracker_poses import FAMILIES, poses, tracker_inputs

pytestmark = pytest.mark.gpu

N_POSES = 20000
FORM_KEYS = ('SCA_TRK_SPEC4_MAX', 'SCA_TRK_SPEC3_MAX', 'SCA_TRK_SPEC2_MAX', 'SCA_TRK_MID_MAX')
# the re-plan ranges that hand every plan of a pass to one form (the launches are sized by the plan count)
FORM_ENV = {'spec4': ('1000000', None, None, None), 'spec3': ('0', '1000000', None, None), 'spec2': ('0', '0', '1000000', None),
            'quad': ('0', '0', '0', '1000000'), 'lane': ('0', '0', '0', '0')}
_ORACLE = {}


def _oracle_plans(oracle, family, P):
    if family not in _ORACLE:
        _ORACLE[family] = oracle_first_plans(oracle, P)
    return _ORACLE[family]


def _set_form(monkeypatch, form):
    for key, v in zip(FORM_KEYS, FORM_ENV[form]):
        if v is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, v)


def _device_first_plans(P, per_agent):
    from sca_amd import _lib, solver as S
    pos, head, goal, gh = tracker_inputs(P)
    n = len(pos)
    sol = S.BatchedSolver(max_agents=n)
    sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
    start6, goal6 = np.concatenate([pos, head], 1), np.concatenate([goal, gh], 1)
    sol.set_agents(np.full(n, 0.5), np.ones(n), goal, np.zeros(n, np.uint8), S.zaxis_flags(start6, goal6), np.full(n, 1e9))
    sol.set_state(pos, np.zeros((n, 3), np.float32), head, np.zeros(n, np.uint8))
    sets = np.unique(np.stack([P['rmin'], P['pitch_lo'], P['pitch_hi']], 1), axis=0)
    if len(sets) == 1 and not per_agent:
        sol.device_tracker_enable(gh, turning_radius=float(sets[0, 0]), pitchlims=(float(sets[0, 1]), float(sets[0, 2])), in_pass=False)
    else:
        sol.device_tracker_enable(gh, in_pass=False)
        sol.device_tracker_set_agent_params(P['rmin'], P['pitch_lo'], P['pitch_hi'])
    v = sol.device_tracker_vpref(np.full(n, -1.0))
    assert np.array_equal(sol.device_tracker_replans(), np.ones(n, np.int32))
    forms = sol.pass_forms()
    rec = np.zeros((n, 24))
    for i in range(n):
        assert sol.L.sca_device_tracker_debug(sol.ctx, i, _lib.ptr(rec[i], C.c_double)) == 0
    sol.close()
    return v, rec, forms


@pytest.mark.parametrize('form', list(FORM_ENV))
@pytest.mark.parametrize('family', FAMILIES)
def test_device_first_plans_equal_oracle(family, form, oracle, monkeypatch):
    from sca_amd import solver as S
    P = poses(family, N_POSES, seed=2)
    vo, ro = _oracle_plans(oracle, family, P)
    _set_form(monkeypatch, form)
    vd, rd, forms = _device_first_plans(P, per_agent=False)
    assert forms & (S.FORM_REPLAN_LANE if form == 'lane' else S.FORM_REPLAN_FEW), (form, forms)
    assert np.array_equal(vd, vo), (family, form, int((vd != vo).any(1).sum()))
    n = compare_records(rd, ro, (family, form))
    print(f'{family} / {form}: {n} first plans and V_des equal to the oracle')


@pytest.mark.parametrize('family', ['params', 'handover', 'steep'])
def test_device_per_agent_plans_equal_oracle(family, oracle):
    """every re-plan a wavefront of its own with its agent's turning radius and pitch limits: 20 and more classes"""
    P = poses(family, N_POSES, seed=3)
    rng = np.random.default_rng(4)
    P['rmin'] = P['rmin'] * rng.choice([1.0, 1.25, 0.8, 2.0, 0.6], N_POSES)
    k = rng.random(N_POSES) < 0.5
    P['pitch_lo'] = np.where(k, rng.choice([-np.pi / 4, -np.pi / 6, -0.5, -0.2], N_POSES), P['pitch_lo'])
    P['pitch_hi'] = np.where(k, rng.choice([np.pi / 4, np.pi / 6, 0.9, 0.2], N_POSES), P['pitch_hi'])
    assert len(np.unique(np.stack([P['rmin'], P['pitch_lo'], P['pitch_hi']], 1), axis=0)) > 16
    vo, ro = oracle_first_plans(oracle, P)
    vd, rd, _ = _device_first_plans(P, per_agent=True)
    assert np.array_equal(vd, vo), (family, int((vd != vo).any(1).sum()))
    n = compare_records(rd, ro, (family, 'per-agent'))
    print(f'{family} / per-agent: {n} first plans and V_des equal to the oracle')


# (kind, N, steps; negative: until every agent is done, at most that many).  The oracle's env step is the reference's all-pairs collision
# check, serial (mampenv.py:61-80, N^2 distances): c5 runs at 1024 agents (64 take-off / landing cells), to the end; c4 is below.
SCENES = [('circle', 1024, 300), ('takeoff', 1024, -1500), ('circle', 160, -4000)]


@pytest.mark.parametrize('mode', ['kd', 'auto'])
@pytest.mark.parametrize('kind,n,steps', SCENES)
def test_free_running_tracked_episode_equals_oracle_run(kind, n, steps, mode, oracle):
    from sca_amd import solver as S
    from test_gpu_value_parity import _scene, _solver
    to_the_end = steps < 0
    steps = abs(steps)
    nbr = S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE
    scene = _scene(kind, n)
    sc, n = scene['sc'], scene['n']
    ext = np.isin(scene['policy'], (0, 5))
    sol = _solver(scene)
    sol.device_tracker_enable(sc['goal'][:, 3:6], in_pass=True)
    radius, ps, goal = np.full(n, 0.5), np.ones(n), np.ascontiguousarray(sc['goal'][:, :3])
    tr = oracle.Tracker(goal, sc['goal'][:, 3:6], ps, scene['zaxis'])
    pos, vel, head = sc['start'][:, :3].copy(), np.zeros((n, 3), np.float32), sc['start'][:, 3:6].copy()
    flags, td, sn, perm = np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.int32), np.arange(n, dtype=np.int32)
    agent_steps = 0
    for t in range(steps):
        active = ((flags & 7) == 0) & ext
        vp = tr.vpref(pos, vel, head, active.astype(np.uint8), nthreads=16)
        r = oracle.policy_step(pos, vel, head, radius, ps, flags, goal, scene['policy'], scene['zaxis'], vp, ext.astype(np.uint8), perm,
                               sc['obs_pos'], sc['obs_radius'], nthreads=16)
        tr.note_neighbors(r['nbr_valid'], r['nbr_n'], r['nbr_dsq'])
        perm = r['perm']
        u = oracle.env_update(pos, vel, head, radius, r['flags'], goal, r['action'], td, scene['mrd'], sn, sc['obs_pos'], sc['obs_radius'])
        agent_steps += int(((flags & 7) == 0).sum())
        pos, vel, head, flags, td, sn = u['pos'], u['vel'], u['heading'], u['flags'], u['total_dist'], u['step_num']
        sol.run_steps(1, nbr)
        sol.synchronize()
        g = sol.get_state()
        for key, want in (('pos', pos), ('vel', vel), ('heading', head), ('flags', flags), ('total_dist', td), ('step_num', sn)):
            assert np.array_equal(g[key], want), (kind, n, mode, t, key, int((g[key] != want).sum()))
        vd = sol.diag()['vpref']
        assert np.array_equal(vd[active], r['vpref'][active]), (kind, n, mode, t, 'vpref', int((vd[active] != r['vpref'][active]).any(1).sum()))
        if mode == 'kd':
            assert np.array_equal(sol.get_kd_perm(), perm), (kind, n, t, 'kd perm')
        if to_the_end and not ((flags & 7) == 0).any():
            steps = t + 1
            break
    if to_the_end:
        assert not ((flags & 7) == 0).any(), f'{kind} N={n}: {int(((flags & 7) == 0).sum())} agents still flying after {steps} steps'
        assert (flags & 1).mean() > 0.9
    ro, rd = tr.replans()[ext], sol.device_tracker_replans()[ext]
    assert np.array_equal(rd, ro), (kind, n, mode, int((rd != ro).sum()))
    assert ro.sum() >= ext.sum()
    print(f'{kind} N={n} {mode}: {steps} steps, {agent_steps} agent-steps, {int(ro.sum())} re-plans: equal to the oracle')
    tr.close()
    sol.close()


def test_c4_tracker_in_the_pass_equals_oracle_tracker():
    """BASELINE config 4 (N = 100 000 circle, 40-km plans, ~97 % of the agents re-planning every step), the tracker inside the resident
    pass, 4 steps.  Open loop on the state: the oracle's tracker reads the device's state before each step (its env step is N^2 at this
    size) and must give the v_pref the device's pass used, every agent, every step; the re-plan counts equal at the end."""
    from sca_amd import solver as S
    from oracle import oracle
    from test_gpu_value_parity import _scene, _solver
    scene = _scene('circle', 100000)
    sc, n = scene['sc'], scene['n']
    sol = _solver(scene)
    sol.device_tracker_enable(sc['goal'][:, 3:6], in_pass=True)
    tr = oracle.Tracker(sc['goal'][:, :3], sc['goal'][:, 3:6], np.ones(n), scene['zaxis'])
    replanned = 0
    for t in range(4):
        st = sol.get_state()
        active = (st['flags'] & 7) == 0
        before = tr.replans()
        vo = tr.vpref(st['pos'], st['vel'], st['heading'], active.astype(np.uint8), nthreads=16)
        replanned += int((tr.replans() != before).sum())
        sol.run_steps(1, S.NBR_KDTREE)
        sol.synchronize()
        tr.note_nbr0(sol.nbr0())
        vd = sol.diag()['vpref']
        assert np.array_equal(vd[active], vo[active]), (t, int((vd[active] != vo[active]).any(1).sum()))
    assert np.array_equal(sol.device_tracker_replans(), tr.replans())
    assert replanned > 2.5 * n                             # (every agent at step 0, then about two in three per step)
    print(f'c4 N={n}: 4 steps, {replanned} re-plans, v_pref equal to the oracle')
    tr.close()
    sol.close()
