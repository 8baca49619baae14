"""The random-scene fuzz of tests/test_gpu_parity.py through EVERY kernel form of sca_forms.h against the oracle (-m gpu).

The fuzz scenes (tests/form_fuzz.py: 1 .. 1600 agents, counts that are no multiple of four, agents done from the start, dense boxes with more
than 16 in range, collisions, zero velocities, z-axis goals, obstacles, mixed radii and policies) run by default as a small shard runs: one
agent per wavefront in K1, the one-launch k_solve, k_solve_lpw, k_action_fb.  Here the tunables force the other forms at the same sizes --
the packed K1, the two-launch solve, the lane-per-agent LP, the fallback launch, k_solve_fb, the level passes of the kd build, and the
combination every large shard runs -- on the plain scenes and on those with per-agent solver attributes.  Free-running, one resident step at a
time; after every step flags, step counts, the kd permutation, float32 velocities, positions, headings, travelled distance, the action rows,
the neighbour lists entry for entry and the decisions' diagnostics EQUAL the oracle's.  No tolerance, nothing left out.  Each row proves the
form it ran: the bits of sca_last_pass_forms against plan_solve of tests/forms_harness.cpp for the scene's counts and the row's switches
(packed K1 and the kd-build shape have no bit: tests/test_form_fuzz_cpu.py checks their plans).

One oracle run per scene and variant (form_fuzz.oracle_run), shared by the rows: the tests of a block follow one another."""
import ctypes as C
import os

import numpy as np
import pytest

import form_fuzz as F
from test_forms_cpu import H, from_env, solve                                       # noqa: F401 (H: fixture)

pytestmark = pytest.mark.gpu

STEPS = 6
SOLVE_BITS = 1 | 16 | 32 | 64                  # SCA_FORM_SOLVE_SPLIT | LP_LANE | SOLVE_FB | ACTION_FB


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


@pytest.fixture(scope='module')
def simds(S):
    """the SIMDs of the running device, as sca_create counts them: four per compute unit"""
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture()
def row_env(monkeypatch):
    """only the row's switches are set while its contexts are created"""
    def set_row(row):
        for k in list(os.environ):
            if k.startswith('SCA_') and k != 'SCA_QUIET':
                monkeypatch.delenv(k)
        for k, v in F.ROWS[row].items():
            monkeypatch.setenv(k, v)
    return set_row


def planned(H, simds, scene):
    """plan_solve for this scene under the environment of the moment"""
    t = from_env(H, simds)
    lp = int((scene['policy'] == 4).sum())
    return solve(H, scene['n'], simds=simds, lp=lp, lp_total=lp, t=(C.c_int * len(t))(*t.values())), t


def context_of(S, scene, per_agent=None, paths=None, state=True, perm=True):
    """a context that holds the scene as its oracle run starts from it: obstacles, agents, per-agent attributes, the lists (paths: what
    form_fuzz.random_paths returned; set_vpref behind set_paths is legal, only a straight-line agent with a list refuses mode 1), the fed
    v_pref of the tracked agents, the state and the identity permutation (state=False: the caller brings the state, sca_step_host;
    perm=False: the permutation is left alone, SCA_NBR_GRID builds no tree)"""
    s, n = scene, scene['n']
    sol = S.BatchedSolver(max_agents=n, max_obstacles=max(1, s['m']), params=per_agent[1] if per_agent else None)
    try:
        sol.set_obstacles(s['obs_pos'], s['obs_radius'])
        sol.set_agents(s['radius'], s['pref_speed'], s['goal'], s['policy'], F.zaxis_of(s), s['max_run_dist'])
        if per_agent and not per_agent[2]:
            sol.set_agent_params(**per_agent[0])
        if paths is not None:
            sol.set_paths(paths)
        sol.set_vpref(s['vpref'], s['vmode'])
        if state:
            sol.set_state(s['pos'], s['vel'], s['heading'], s['flags'], np.zeros(n), np.zeros(n, np.int32))
            if perm:
                sol.set_kd_perm(np.arange(n, dtype=np.int32))
    except BaseException:
        sol.close()
        raise
    return sol


def compare_with_oracle(sol, r, scene, at, rows=slice(None), eq=np.array_equal):
    """what a context holds after a step against the oracle's record `r` of it: flags, step counts, the kd permutation, float32 velocities,
    positions, headings, travelled distance, the action rows, the neighbour lists entry for entry, the decisions' diagnostics.  rows: the
    agents whose rows are compared (a shard; the permutation is the whole swarm's).  eq: how the floating-point arrays are compared --
    np.array_equal; golden_util.equal_for of the degenerate-geometry family lets a NaN equal a NaN at the same place"""
    lp = (scene['policy'] == 4)[rows]
    g = sol.get_state()
    assert np.array_equal(g['flags'][rows], r['flags'][rows]), at + ('flags', np.flatnonzero(g['flags'][rows] != r['flags'][rows])[:8])
    assert np.array_equal(g['step_num'][rows], r['step_num'][rows]), at + ('step_num',)
    assert np.array_equal(sol.get_kd_perm(), r['perm']), at + ('perm',)
    assert eq(g['vel'][rows], r['vel'][rows]), at + ('vel', np.flatnonzero((g['vel'][rows] != r['vel'][rows]).any(axis=1))[:8])
    for k in ('pos', 'heading', 'total_dist'):
        assert eq(g[k][rows], r[k][rows]), at + (k,)
    compare_pass_with_oracle(sol, r, at, lp, rows, eq=eq)


def compare_pass_with_oracle(sol, r, at, lp, rows=slice(None), ref_rows=None, id_base=(0, 0), eq=np.array_equal):
    """the policy pass's own results: action rows, neighbour lists, diagnostics (lp: the ORCA3D-LP agents among the rows).  rows: the
    context's rows that are compared, ref_rows: the record's (None: the same rows -- a shard; a scene of a batch is rows [lo, hi) of the
    context and the whole record of its own run, its ids in the lists global: id_base = (lo, the scene's first obstacle))"""
    rr = rows if ref_rows is None else ref_rows
    a = sol.actions()[rows]
    assert eq(a, r['action'][rr]), at + ('action', np.flatnonzero((a != r['action'][rr]).any(axis=1))[:8])
    nb = {k: v[rows] for k, v in sol.neighbors().items()}
    nb['nbr_id'] = nb['nbr_id'] - np.where(nb['nbr_id'] >= 0, np.where(nb['nbr_kind'] == 1, id_base[1], id_base[0]), 0)
    valid = r['nbr_valid'][rr].astype(bool)
    assert np.array_equal(nb['nbr_valid'].astype(bool), valid), at + ('nbr_valid',)
    for k in ('nbr_n', 'nbr_id', 'nbr_kind', 'nbr_dsq'):
        assert np.array_equal(nb[k][valid], r[k][rr][valid]), at + (k,)
    dg, want = sol.diag()['diag'][rows], r['diag'][rr]
    assert np.array_equal(dg[:, :2], want[:, :2]), at + ('n_suit / fallback', np.flatnonzero((dg[:, :2] != want[:, :2]).any(axis=1))[:8])
    assert np.array_equal(dg[lp, 3:5], want[lp, 3:5]), at + ('planeFail / lp4',)


def check_paths(sol, r, scene, at, rows=slice(None), ref_rows=None):
    """the waypoint lists behind a pass against the record `r` of an oracle run with lists: what is left of every list and now_goal (NaN rows
    included) are the rule's, and the v_pref the pass used is the rule's on the served rows it aims at a waypoint and the fed one on the
    served tracked rows.  rows / ref_rows: as in compare_pass_with_oracle (`scene` is the record's)"""
    rr = rows if ref_rows is None else ref_rows
    rem, ng = sol.get_path_state()
    assert np.array_equal(rem[rows], r['path_left'][rr]), at + ('path_left', np.flatnonzero(rem[rows] != r['path_left'][rr])[:8])
    assert np.array_equal(ng[rows], r['now_goal'][rr], equal_nan=True), at + ('now_goal',)
    served = ((r['before'] & 7) == 0)[rr]
    aimed, tracked = served & r['path_mode'][rr].astype(bool), served & scene['vmode'][rr].astype(bool)
    vp = sol.diag()['vpref'][rows]
    differ = (vp != r['vpref_rule'][rr]).any(axis=1)
    assert not (aimed & differ).any(), at + ('v_pref toward the waypoint', np.flatnonzero(aimed & differ)[:8])
    assert np.array_equal(vp[tracked], scene['vpref'][rr][tracked]), at + ('fed v_pref of the tracked agents',)


def run_against_oracle(S, oracle, scene, steps, nbr, per_agent, plan, ctx, require=0, paths=None):
    """one context, `steps` resident steps, everything compared after each (`require`: form bits every pass must report, whatever the plan says;
    paths: the scene's waypoint lists -- the oracle run is the one with lists, every pass reports FORM_WAYPOINTS and the lists, now_goal and
    the v_pref used are compared too); the context is closed before the caller makes the next"""
    s, n = scene, scene['n']
    ref = F.oracle_run(oracle, s, steps, per_agent, paths=paths)
    if paths is not None:
        require |= S.FORM_WAYPOINTS
    sol = context_of(S, s, per_agent, paths)
    try:
        for t, r in enumerate(ref):
            sol.run_steps(1, nbr)
            sol.synchronize()
            at = ctx + ('n', n, 'step', t)
            forms = sol.pass_forms()
            assert (forms & SOLVE_BITS) == plan['forms'] and (forms & require) == require, at + ('forms', forms, plan)
            assert paths is not None or not forms & S.FORM_WAYPOINTS, at + ('forms', forms)
            compare_with_oracle(sol, r, s, at)
            if paths is not None:
                check_paths(sol, r, s, at)
    finally:
        sol.close()


def _blocks(seeds, rows):
    """block-major: all rows of a block one after the other, so that its oracle runs are made once and dropped when the next block's come"""
    out = []
    for b in range(len(seeds) // F.BLOCK):
        for row in rows:
            for mode in (('kd', 'auto') if row == 'large_shard' else ('kd',)):
                out.append(pytest.param(row, mode, b, id='%s-%s-%d' % (row, mode, b)))
    return out


@pytest.mark.parametrize('row,mode,block', _blocks(F.PLAIN_SEEDS, list(F.ROWS)))
def test_form_rows_on_the_plain_scenes(S, H, oracle, simds, row_env, row, mode, block):
    """20 scenes of the plain corpus (seeds 0-119) through one row's forms; `solve_fb`: their no_lp variant, FORM_SOLVE_FB on every pass"""
    row_env(row)
    nbr = S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE
    for seed in F.PLAIN_SEEDS[F.BLOCK * block: F.BLOCK * (block + 1)]:
        s = F.random_scene(seed)
        if row == 'solve_fb':
            s = F.no_lp(s)
        plan, tun = planned(H, simds, s)
        require = S.FORM_SOLVE_FB if row == 'solve_fb' and s['n'] <= tun['SCA_SOLVE_FB_MAX'] else 0
        run_against_oracle(S, oracle, s, STEPS, nbr, None, plan, (row, mode, 'seed', seed), require)


@pytest.mark.parametrize('row,mode,block', _blocks(F.PER_AGENT_SEEDS, F.PER_AGENT_ROWS))
def test_form_rows_on_the_scenes_with_per_agent_attributes(S, H, oracle, simds, row_env, row, mode, block):
    """20 scenes of the per-agent corpus (seeds 1000-1059: maxNeighbors, neighborDist, timeStep, timeHorizon, maxSpeed, max_heading_change and
    dt_nominal drawn per agent, or every third scene one non-default value of each per scene) through the forms that read them somewhere else
    than the default forms do: the packed K1 (range and list length), k_lp (time horizon, time step, maximum speed) and the two-launch solve"""
    row_env(row)
    nbr = S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE
    for seed in F.PER_AGENT_SEEDS[F.BLOCK * block: F.BLOCK * (block + 1)]:
        s = F.random_scene(seed)
        plan, _ = planned(H, simds, s)
        run_against_oracle(S, oracle, s, STEPS, nbr, F.per_agent_attributes(seed, s['n']), plan, (row, mode, 'seed', seed))


@pytest.mark.parametrize('n', F.SWITCH_SIZES)
def test_one_real_switch_at_default_tunables(S, H, oracle, simds, row_env, n):
    """No switch set: scenes of 2047 / 2049 agents without LP agents on either side of k_solve_fb's bound (FORM_SOLVE_FB set / clear), and of
    6143 / 6145 agents on either side of the packed K1's, drawn as tests/fuzz_oracle.py draws its scenes; two free-running steps.  The
    bounds scale with the device's SIMD count: on a device where these sizes do not straddle them the pair is skipped."""
    row_env('solve_fb')
    pair = F.SWITCH_SIZES[:2] if n in F.SWITCH_SIZES[:2] else F.SWITCH_SIZES[2:]
    scenes = {k: (F.no_lp(F.switch_scene(k)) if k < 3000 else F.switch_scene(k)) for k in pair}
    plans = {k: planned(H, simds, scenes[k])[0] for k in pair}
    what, sides = ('solve_fb', [1, 0]) if n < 3000 else ('packed', [0, 1])
    if [plans[k][what] for k in pair] != sides:
        pytest.skip('%d SIMDs: %s does not switch between %d and %d agents here' % ((simds, what) + tuple(pair)))
    if what == 'solve_fb':
        assert bool(plans[n]['forms'] & S.FORM_SOLVE_FB) == (n == pair[0]), plans[n]          # (and every pass reports the plan's bits)
    run_against_oracle(S, oracle, scenes[n], 2, S.NBR_KDTREE, None, plans[n], ('switch',), S.FORM_SOLVE_FB if n == F.SWITCH_SIZES[0] else 0)


def test_packed_k1_at_a_ragged_shard_end_inside_the_swarm(S, oracle, row_env):
    """The last wavefront of the packed K1 holds one, two or three agents of the shard and, behind them, agents that exist but belong to somebody
    else (sca_set_shard): its idle groups must read a valid record and write nothing.  A 100-agent fuzz scene with 30 obstacles, shards
    [0, 97), [0, 98), [0, 99) on fresh contexts, one policy pass: the shard's lists and action rows equal the oracle's, and the agents behind
    the shard's end -- all three served in the oracle's pass of the whole swarm -- are left without a list."""
    row_env('packed')
    s = F.random_scene(28)
    n = s['n']
    r = F.oracle_run(oracle, s, 1)[0]
    assert n == 100 and s['m'] == 30 and r['nbr_valid'][-3:].all() and (r['nbr_n'][-3:] > 0).all()      # (the scene: what the test needs of it)
    for c in (n - 3, n - 2, n - 1):
        sol = S.BatchedSolver(max_agents=n, max_obstacles=s['m'])
        try:
            sol.set_obstacles(s['obs_pos'], s['obs_radius'])
            sol.set_agents(s['radius'], s['pref_speed'], s['goal'], s['policy'], F.zaxis_of(s), s['max_run_dist'])
            sol.set_vpref(s['vpref'], s['vmode'])
            sol.set_state(s['pos'], s['vel'], s['heading'], s['flags'], np.zeros(n), np.zeros(n, np.int32))
            sol.set_kd_perm(np.arange(n, dtype=np.int32))
            sol.set_shard(0, c)
            sol.policy_pass(S.NBR_KDTREE)
            nb, a = sol.neighbors(), sol.actions()
            assert np.array_equal(sol.get_kd_perm(), r['perm']), c
            assert not nb['nbr_valid'][c:].any() and not nb['nbr_n'][c:].any(), (c, nb['nbr_valid'][c:], nb['nbr_n'][c:])
            valid = r['nbr_valid'][:c].astype(bool)
            assert np.array_equal(nb['nbr_valid'][:c].astype(bool), valid), c
            for k in ('nbr_n', 'nbr_id', 'nbr_kind', 'nbr_dsq'):
                assert np.array_equal(nb[k][:c][valid], r[k][:c][valid]), (c, k)
            assert np.array_equal(a[:c], r['action'][:c]), c
        finally:
            sol.close()
