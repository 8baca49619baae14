"""The degenerate-geometry family (tests/golden/F20_edge_*.npz: coincident and touching agents, integer lattices, rings, agents on
obstacles and goals, parallel ORCA planes, scenes 1e6 m and one grid-key wrap from zero) through every kernel form against the oracle
(-m gpu).  tests/test_oracle_golden.py holds the oracle to the reference on these very recordings, tests/test_edge_corpus_cpu.py counts
what they contain; the parity tests' glob runs them through the default forms.  Here, by equality through the C ABI:

(a) every recorded step of every scene from its recorded state -- kd permutation, travelled distance and fed v_pref included -- through
    every form row of form_fuzz.ROWS in kd mode, one context per scene: state, action rows, lists entry for entry, diagnostics, status words,
    the v_pref used, the permutation, and the form bits that prove the row ran;
(b) the same in SCA_NBR_AUTO, and in SCA_NBR_GRID against list rule 1 (ties by id, overflow flagged) -- alone, packed several scenes to a
    context (tests/test_edge_corpus_cpu.py: a packed scene is what it is alone under that rule), and with the lattice one key wrap out
    beside its copy at the origin, whose cells share their keys;
(c) all scenes as ONE scene batch in both K1 forms with the clearance records on, every scene against its recording and its records
    against tests/clearance_rule.py over the recorded positions;
(d) the recorded episodes free-running for their recorded length under sca_run_steps(3) and under sca_step_host, the tracker of the
    SCA / RVO3D+Dubins agents on the device, against the recordings;
(e) the lattices and the touching pairs behind three ranks of the cell-owner partition, a lattice plane exactly on a cut.

The one relaxation is golden_util.equal_for's: a NaN equals a NaN at the same place (the reference's own 0 / 0 among exactly parallel
planes).  The grid refuses none of these scenes."""
import numpy as np
import pytest

import clearance_rule as R
import edge_corpus as E
import form_fuzz as F
import partition_ranks as PR
from golden_util import edge_fixtures, equal_for, static_inputs
from test_forms_cpu import H                                                         # noqa: F401 (fixture)
from test_gpu_form_fuzz import S, SOLVE_BITS, compare_with_oracle, planned, row_env, simds       # noqa: F401 (fixtures)
from test_gpu_grid_fuzz import compare_grid_step
from test_gpu_partition_fuzz import run_ranks_against_oracle

pytestmark = pytest.mark.gpu

EQ = equal_for('F20_')
NAMES = edge_fixtures()
EPISODES = [n for n in NAMES if E.steps_of(n) > 1]


def context(S, scene):
    """a context that holds the scene's constants (obstacles, agents); the state comes with every step"""
    s = scene
    sol = S.BatchedSolver(max_agents=s['n'], max_obstacles=max(1, s['m']))
    try:
        sol.set_obstacles(s['obs_pos'], s['obs_radius'])
        sol.set_agents(s['radius'], s['pref_speed'], s['goal'], s['policy'], s['zaxis'], s['max_run_dist'])
    except BaseException:
        sol.close()
        raise
    return sol


def put(sol, scene, perm=True):
    s = scene
    sol.set_state(s['pos'], s['vel'], s['heading'], s['flags'], s['total_dist'], np.zeros(s['n'], np.int32))
    if perm:
        sol.set_kd_perm(s['perm'])
    sol.set_vpref(s['vpref'], s['vmode'])


def check_kd_step(sol, r, scene, at, rows=slice(None)):
    compare_with_oracle(sol, r, scene, at, rows, eq=EQ)
    dg = sol.diag()
    assert np.array_equal(dg['status'][rows], r['status'][rows]), at + ('status', dg['status'][rows], r['status'][rows])
    served = ((r['before'] & 7) == 0)[rows]
    assert np.array_equal(dg['vpref'][rows][served], r['vpref'][rows][served]), at + ('v_pref used',)


@pytest.mark.parametrize('row', list(F.ROWS))
def test_every_form_row_on_every_recorded_step(S, H, oracle, simds, row_env, row):
    """`solve_fb`: the scenes' no_lp variant, FORM_SOLVE_FB on every pass"""
    row_env(row)
    steps = 0
    for name in NAMES:
        sol, plan = None, None
        try:
            for t in range(E.steps_of(name)):
                s = E.step_scene(name, t)
                if row == 'solve_fb':
                    s = F.no_lp(s)
                if sol is None:
                    sol = context(S, s)
                    plan, tun = planned(H, simds, s)
                r = E.oracle_step(oracle, s)
                assert not r['status'].any(), (name, t)
                put(sol, s)
                sol.run_steps(1, S.NBR_KDTREE)
                sol.synchronize()
                at = (row, name, 'step', t)
                forms = sol.pass_forms()
                assert (forms & SOLVE_BITS) == plan['forms'], at + ('forms', forms, plan)
                assert row != 'solve_fb' or forms & S.FORM_SOLVE_FB, at + ('forms', forms)
                check_kd_step(sol, r, s, at)
                steps += 1
        finally:
            if sol is not None:
                sol.close()
    assert steps == 105, steps


def test_auto_mode_on_every_recorded_step(S, H, oracle, simds, row_env):
    row_env('solve_fb')                                                              # (no switch set: the default forms)
    for name in NAMES:
        sol = context(S, E.step_scene(name, 0))
        try:
            for t in range(E.steps_of(name)):
                s = E.step_scene(name, t)
                put(sol, s)
                sol.run_steps(1, S.NBR_AUTO)
                sol.synchronize()
                check_kd_step(sol, E.oracle_step(oracle, s), s, ('auto', name, 'step', t))
        finally:
            sol.close()


def grid_step(S, oracle, sol, s, at):
    put(sol, s, perm=False)
    sol.run_steps(1, S.NBR_GRID)                                                     # (a refusal would raise here: none of these scenes is refused)
    sol.synchronize()
    return compare_grid_step(sol, E.oracle_step(oracle, s, list_rule=1), s, at, vpref=True, nan_equal=True)


def test_grid_mode_on_every_recorded_step(S, oracle, row_env):
    row_env('solve_fb')
    overflowed = 0
    for name in NAMES:
        sol = context(S, E.step_scene(name, 0))
        try:
            for t in range(E.steps_of(name)):
                overflowed += grid_step(S, oracle, sol, E.step_scene(name, t), ('grid', name, 'step', t))
        finally:
            sol.close()
    assert overflowed > 500, overflowed                                              # (the 4 x 4 x 4 lattices: 63 in range, ties at the cut)


@pytest.mark.parametrize('mode', ['grid', 'kd'])
def test_scenes_packed_into_one_context(S, oracle, row_env, mode):
    """groups of at most 600 agents, scene j moved 4096 (j + 1) m along an axis where that is exact; the first recorded state of each"""
    row_env('solve_fb')
    for g, group in enumerate(E.concat_groups()):
        scenes = [E.step_scene(name) for name in group]
        whole, off, ooff = E.concat(scenes, [E.concat_shift(s, j) for j, s in enumerate(scenes)])
        sol = context(S, whole)
        try:
            if mode == 'grid':
                grid_step(S, oracle, sol, whole, ('packed grid', g))
            else:
                put(sol, whole)
                sol.run_steps(1, S.NBR_KDTREE)
                sol.synchronize()
                check_kd_step(sol, E.oracle_step(oracle, whole), whole, ('packed kd', g))
        finally:
            sol.close()


def test_grid_cells_one_key_wrap_apart_in_one_context(S, oracle, row_env):
    """F20_edge_farwrap_lattice3_mixed beside its own copy moved back to the origin: cells 2^21 apart along x share their 63-bit keys"""
    row_env('solve_fb')
    far = E.step_scene('F20_edge_farwrap_lattice3_mixed')
    back = np.array([-far['pos'][:, 0].min(), 0.0, 0.0])
    assert back[0] == np.rint(back[0]) and (far['pos'] == np.rint(far['pos'])).all()
    near = dict(far, key=far['key'] + ('near',))
    whole, off, ooff = E.concat([far, near], [np.zeros(3), back])
    inv = PR.inv_cell_of(10.0)
    cells = PR.cell_of(whole['pos'][:, 0], inv)
    assert set((cells[:27] - cells[27:]).tolist()) == {1 << 21}, 'the two copies are not one key wrap apart'
    sol = context(S, whole)
    try:
        grid_step(S, oracle, sol, whole, ('key wrap',))
    finally:
        sol.close()


# ---- (c) one scene batch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', ['packed', 'solve_fb'])
def test_all_scenes_as_one_scene_batch_with_clearance(S, row_env, row):
    """every fixture a scene of one context with its own obstacles, from its first recorded state with the recorded v_pref fed; one step in
    the packed K1 (`packed`) and in the wave-per-agent K1 (`solve_fb`: no switch set).  Every scene equals its recording, and its clearance
    records the rule over the recorded positions: coincident agents (c < 0 at distance 0), touching ones (c == 0), the lattices' partners
    at equal distance (the lowest id)."""
    row_env(row)
    fxs = [E.fixture(n) for n in NAMES]
    sts = [static_inputs(f) for f in fxs]
    off = np.concatenate([[0], np.cumsum([len(st['radius']) for st in sts])]).astype(np.int32)
    n = int(off[-1])
    cat = lambda key: np.concatenate([st[key] for st in sts])
    catx = lambda key: np.concatenate([f[key][0] for f in fxs])
    sol = S.BatchedSolver(max_agents=n, max_obstacles=max(1, sum(len(st['obs_radius']) for st in sts)))
    try:
        sol.set_agents(cat('radius'), cat('pref_speed'), catx('goal'), cat('policy'), cat('zaxis'), cat('max_run_dist'))
        sol.set_scenes(off)
        sol.set_scene_obstacles([(st['obs_pos'].reshape(-1, 3), st['obs_radius']) for st in sts])
        sol.scene_clearance_enable()
        sol.set_state(catx('pos'), catx('vel'), catx('heading'), catx('flags'), catx('total_dist'), np.zeros(n, np.int32))
        sol.set_vpref(np.nan_to_num(catx('vpref')), cat('vpref_mode'))
        sol.run_steps(1, S.NBR_KDTREE)
        sol.synchronize()
        g, a, dg, nb = sol.get_state(), sol.actions(), sol.diag()['diag'], sol.neighbors()
        ooff = np.concatenate([[0], np.cumsum([len(st['obs_radius']) for st in sts])])
        for s, (name, f, st) in enumerate(zip(NAMES, fxs, sts)):
            rows = slice(int(off[s]), int(off[s + 1]))
            called = f['called'][0].astype(bool)
            assert EQ(a[rows][called], f['action'][0][called]), (row, name, 'action')
            sel, lp = f['n_suit'][0] >= 0, f['plane_fail'][0] >= 0
            assert np.array_equal(dg[rows][sel, 0], f['n_suit'][0][sel]) and np.array_equal(dg[rows][sel, 1], f['fallback'][0][sel]), (row, name, 'n_suit / fallback')
            assert np.array_equal(dg[rows][lp, 3], f['plane_fail'][0][lp]) and np.array_equal(dg[rows][lp, 4], f['lp4'][0][lp]), (row, name, 'planeFail / lp4')
            valid = f['nbr_valid'][0].astype(bool)
            ids = nb['nbr_id'][rows] - np.where(nb['nbr_id'][rows] >= 0, np.where(nb['nbr_kind'][rows] == 1, ooff[s], off[s]), 0)   # (global ids)
            assert np.array_equal(nb['nbr_valid'][rows].astype(bool), valid) and np.array_equal(nb['nbr_n'][rows][valid], f['nbr_n'][0][valid]), (row, name, 'nbr_n')
            assert np.array_equal(ids[valid], f['nbr_id'][0][valid]) and np.array_equal(nb['nbr_dsq'][rows][valid], f['nbr_dsq'][0][valid]), (row, name, 'lists')
            for key, want in (('pos', 'pos_after'), ('vel', 'vel_after'), ('heading', 'heading_after'), ('total_dist', 'total_dist_after'), ('flags', 'flags_after')):
                assert EQ(g[key][rows], f[want][0]), (row, name, key)
            want = R.empty(len(st['radius']))
            R.step(want, f['pos_after'][0], st['radius'], f['flags'][0], st['obs_pos'].reshape(-1, 3), st['obs_radius'], 1)
            got = sol.scene_clearance(s)
            for field in want.dtype.names:
                assert EQ(got[field], want[field]), (row, name, 'clearance', field, np.flatnonzero(E.differ(got[field], want[field])).tolist()[:8])
    finally:
        sol.close()


# ---- (d) free-running ---------------------------------------------------------------------------------------------------------------------------
def _free_context(S, fx, st):
    sol = S.BatchedSolver(max_agents=len(st['radius']), max_obstacles=max(len(st['obs_radius']), 1))
    sol.set_obstacles(st['obs_pos'], st['obs_radius'])
    sol.set_agents(st['radius'], st['pref_speed'], fx['goal'][0], st['policy'], st['zaxis'], st['max_run_dist'])
    if st['vpref_mode'].any():
        sol.device_tracker_enable(fx['goal6'][:, 3:6], in_pass=True)
    return sol


AFTER = (('pos', 'pos_after'), ('vel', 'vel_after'), ('heading', 'heading_after'), ('total_dist', 'total_dist_after'), ('flags', 'flags_after'))


@pytest.mark.parametrize('how', ['bursts_of_3', 'step_host'])
def test_recorded_episodes_free_running(S, row_env, how):
    """from the first recorded state (velocities as recorded), nothing fed: the tracked agents' v_pref is the device tracker's, as in
    tests/test_gpu_tracker_oracle.py's loop -- coincident starts, agents at rest, poses 1e6 m out.  Compared with the recording wherever a
    burst ends / after every host step."""
    row_env('solve_fb')
    for name in EPISODES:
        fx = E.fixture(name)
        st = static_inputs(fx)
        T, n = len(fx['step']), len(st['radius'])
        sol = _free_context(S, fx, st)
        try:
            if how == 'bursts_of_3':
                sol.set_state(fx['pos'][0], fx['vel'][0], fx['heading'][0], fx['flags'][0], fx['total_dist'][0], np.zeros(n, np.int32))
                sol.set_kd_perm(fx['perm'][0])
                done = 0
                while done < T:
                    k = min(3, T - done)
                    sol.run_steps(k, S.NBR_KDTREE)
                    sol.synchronize()
                    done += k
                    g = sol.get_state()
                    for key, want in AFTER:
                        assert EQ(g[key], fx[want][done - 1]), (how, name, 'after step', done - 1, key)
                    assert np.array_equal(sol.get_kd_perm(), fx['perm_after'][done - 1]), (how, name, done - 1, 'perm')
                    called = fx['called'][done - 1].astype(bool)
                    assert EQ(sol.actions()[called], fx['action'][done - 1][called]), (how, name, done - 1, 'action')
            else:
                blk = sol.host_state()
                for key in ('pos', 'vel', 'heading', 'flags', 'total_dist'):
                    blk[key][:] = fx[key][0]
                for t in range(T):
                    sol.step_host(S.NBR_KDTREE, state=(t == 0))
                    called = fx['called'][t].astype(bool)
                    assert EQ(blk['action'][called], fx['action'][t][called]), (how, name, t, 'action')
                    for key, want in AFTER:
                        assert EQ(blk[key], fx[want][t]), (how, name, 'after step', t, key)
        finally:
            sol.close()


# ---- (e) three ranks, a lattice plane on a cut ----------------------------------------------------------------------------------------------------
CUT_SCENES = ('F20_edge_lattice4_s2_rvo', 'F20_edge_lattice4_s2_srvo', 'F20_edge_lattice4_s2_orca', 'F20_edge_lattice4_s2_orcalp',
              'F20_edge_lattice_plane_mixed', 'F20_edge_touching_cone')


@pytest.mark.parametrize('name', CUT_SCENES)
def test_three_ranks_with_a_lattice_plane_on_the_cut(S, oracle, row_env, name):
    """the scene moved along x so that its plane x = 2 (the touching pairs: x = 0, the agents at rest there) is the first double of cell 1,
    where the cut between ranks 1 and 2 is: agents sit exactly on the boundary, their neighbours at equal distances on either side.  Rank 0
    owns nobody.  Four steps against list rule 1 and the ownership model, as tests/test_gpu_partition_fuzz.py does."""
    row_env('solve_fb')
    s = dict(E.step_scene(name))
    inv = PR.inv_cell_of(10.0)
    b = PR.first_double_of_cell(1, inv)
    plane = 2.0 if 'lattice' in name else 0.0
    on = s['pos'][:, 0] == plane
    assert on.any()
    pos, goal, obs = s['pos'].copy(), s['goal'].copy(), s['obs_pos'].copy()
    pos[:, 0] += b - plane
    pos[on, 0] = b
    goal[:, 0] += b - plane
    if len(obs):
        obs[:, 0] += b - plane
    # (the fed v_pref of the tracked copies of the mixed plane and the pairs stays what the reference's tracker gave at this state)
    s.update(pos=pos, goal=goal, obs_pos=obs, flags=s['flags'].copy(), key=('edge cut', name))
    assert (PR.cell_of(pos[on, 0], inv) == 1).all() and (PR.cell_of(np.nextafter(pos[on, 0], -np.inf), inv) == 0).all()
    run_ranks_against_oracle(S, oracle, s, 3, 0, [-5.0, 15.0], 4, ('edge cut', name))
