"""Waypoint lists (Agent.path) through every kernel form, the grid, bursts, sca_step_host, a shard and a scene batch, against the oracle fed
from the rule (-m gpu).

k_waypoint hands the straight-line path agents their v_pref through vpref_ext / vpref_mode, which every prologue site reads in a kernel of
its own (prep_agent, solve_one, the packed K1's gather, track_store): right only while k_waypoint precedes all of them on every stream.  The
random scenes of tests/form_fuzz.py get lists of their own (form_fuzz.random_paths: waypoints within the radius, behind the agent, ahead of
it, on the goal, around the radius' edge; tests/test_form_fuzz_cpu.py counts what the rule does with them) and run free under every row of
form_fuzz.ROWS, with per-agent attributes, in SCA_NBR_GRID and SCA_NBR_KDTREE_HOSTBUILD, in bursts of several steps per call (kd, and AUTO
where the next pass's tree is built ahead), through sca_step_host, as a shard inside the swarm and as the scenes of one batch.  The oracle
takes each pass with the v_pref of tests/path_rule.py on the rows the rule aims at a waypoint and the scene's fed v_pref on the tracked
rows, whose lists advance all the same.

After every resident step everything tests/test_gpu_form_fuzz.py compares (state, permutation, action rows, lists entry for entry,
diagnostics, the solve bits against plan_solve) EQUALS the oracle's, and so do what is left of every list, now_goal (None rows included)
and the v_pref the pass used; every pass reports FORM_WAYPOINTS.  No tolerance, nothing left out.  The recorded F19 episodes -- the
reference's own values, with the device tracker's side stream beside k_waypoint -- run under every row too, and in SCA_NBR_GRID."""
import numpy as np
import pytest

import form_fuzz as F
import scene_util as U
from test_forms_cpu import H                                                          # noqa: F401 (fixture)
from test_gpu_form_fuzz import (S, SOLVE_BITS, check_paths, compare_pass_with_oracle, compare_with_oracle, context_of, planned,     # noqa: F401
                                row_env, run_against_oracle, simds)
from test_gpu_grid_fuzz import planned as grid_planned, run_grid_against_oracle
from test_gpu_paths import FIXTURES, load as load_episode, run_recorded_episode
from test_grid_rule_cpu import GRID_MAY_REFUSE

pytestmark = pytest.mark.gpu

STEPS = 6
PLAIN_SEEDS = F.PLAIN_SEEDS[:40]               # the path corpus: two blocks of the plain scenes ...
PER_AGENT_SEEDS = F.PER_AGENT_SEEDS[:20]       # ... and one of those with per-agent attributes (tests/test_form_fuzz_cpu.py counts both)


def block_of(seeds, block):
    return seeds[F.BLOCK * block: F.BLOCK * (block + 1)]


def _rows(blocks, rows):
    """block-major, as in tests/test_gpu_form_fuzz.py: the rows of a block share its oracle runs"""
    return [pytest.param(row, mode, b, id='%s-%s-%d' % (row, mode, b)) for b in range(blocks) for row in rows
            for mode in (('kd', 'auto') if row == 'large_shard' else ('kd',))]


@pytest.mark.parametrize('row,mode,block', _rows(2, list(F.ROWS)))
def test_form_rows_with_lists(S, H, oracle, simds, row_env, row, mode, block):
    """20 plain scenes with their lists through one row's forms; `solve_fb`: their no_lp variant, FORM_SOLVE_FB on every pass"""
    row_env(row)
    nbr = S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE
    for seed in block_of(PLAIN_SEEDS, block):
        s = F.random_scene(seed)
        paths = F.random_paths(seed, s)
        if row == 'solve_fb':
            s = F.no_lp(s)
        plan, tun = planned(H, simds, s)
        require = S.FORM_SOLVE_FB if row == 'solve_fb' and s['n'] <= tun['SCA_SOLVE_FB_MAX'] else 0
        run_against_oracle(S, oracle, s, STEPS, nbr, None, plan, (row, mode, 'seed', seed), require, paths=paths)


@pytest.mark.parametrize('row,mode,block', _rows(1, F.PER_AGENT_ROWS))
def test_form_rows_with_lists_and_per_agent_attributes(S, H, oracle, simds, row_env, row, mode, block):
    """the scenes of seeds 1000-1019 (sca_set_agent_params, or one non-default value of each attribute per scene) with their lists"""
    row_env(row)
    nbr = S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE
    for seed in block_of(PER_AGENT_SEEDS, block):
        s = F.random_scene(seed)
        plan, _ = planned(H, simds, s)
        run_against_oracle(S, oracle, s, STEPS, nbr, F.per_agent_attributes(seed, s['n']), plan, (row, mode, 'seed', seed),
                           paths=F.random_paths(seed, s))


@pytest.mark.parametrize('leg,block', [pytest.param(leg, b, id='%s-%d' % (leg, b)) for b in range(2) for leg in ('default', 'large_shard')])
def test_grid_with_lists(S, H, oracle, simds, row_env, leg, block):
    """SCA_NBR_GRID against the oracle of its own list rule, the plain scenes with their lists: at the default forms and under the
    large-shard switches.  No plain scene is refused."""
    row_env('large_shard' if leg == 'large_shard' else 'solve_fb')                  # (`solve_fb`: no switch set)
    for seed in block_of(PLAIN_SEEDS, block):
        s = F.random_scene(seed)
        got = run_grid_against_oracle(S, oracle, s, STEPS, None, grid_planned(H, simds, s), (leg, 'seed', seed), paths=F.random_paths(seed, s))
        assert got is not None, (leg, seed)


def test_grid_with_lists_and_per_agent_attributes(S, H, oracle, simds, row_env):
    """... and the per-agent scenes of seeds 1000-1019: max_neighbors and neighbor_dist per agent.  The library may refuse what it refuses
    without lists (GRID_MAY_REFUSE of tests/test_grid_rule_cpu.py) and nothing else."""
    row_env('solve_fb')
    ran = 0
    for seed in PER_AGENT_SEEDS:
        s = F.random_scene(seed)
        got = run_grid_against_oracle(S, oracle, s, STEPS, F.per_agent_attributes(seed, s['n']), grid_planned(H, simds, s),
                                      ('per_agent', 'seed', seed), may_refuse=seed in GRID_MAY_REFUSE, paths=F.random_paths(seed, s))
        ran += got is not None
    assert ran >= len(PER_AGENT_SEEDS) - len(set(PER_AGENT_SEEDS) & set(GRID_MAY_REFUSE)), ran


def test_host_built_tree_with_lists(S, H, oracle, simds, row_env):
    """SCA_NBR_KDTREE_HOSTBUILD: k_waypoint in front of the host build's k_prep"""
    row_env('solve_fb')
    for seed in block_of(PLAIN_SEEDS, 0):
        s = F.random_scene(seed)
        run_against_oracle(S, oracle, s, STEPS, S.NBR_KDTREE_HOSTBUILD, None, planned(H, simds, s)[0], ('hostbuild', 'seed', seed),
                           paths=F.random_paths(seed, s))


def burst_against_oracle(S, oracle, scene, paths, nbr, plan, ctx, burst=3, calls=2):
    """`calls` sca_run_steps calls of `burst` steps each: after each call the state, the permutation, the last pass's results, the lists and
    now_goal are the oracle's after as many steps.  Returns the context, open, for what the caller wants to know of it."""
    ref = F.oracle_run(oracle, scene, burst * calls, paths=paths)
    sol = context_of(S, scene, None, paths)
    try:
        for c in range(calls):
            sol.run_steps(burst, nbr)
            sol.synchronize()
            r = ref[burst * (c + 1) - 1]
            at = ctx + ('n', scene['n'], 'after step', burst * (c + 1))
            forms = sol.pass_forms()
            assert (forms & SOLVE_BITS) == plan['forms'] and forms & S.FORM_WAYPOINTS, at + ('forms', forms, plan)
            compare_with_oracle(sol, r, scene, at)
            check_paths(sol, r, scene, at)
    except BaseException:
        sol.close()
        raise
    return sol


@pytest.mark.parametrize('mode', ['kd', 'auto'])
def test_bursts_with_lists(S, H, oracle, simds, row_env, mode):
    """three steps per library call, twice, on the first block: no fork rides on the previous step's last kernel while lists are set, and
    k_waypoint of step k + 1 follows the integrate stage of step k on the same stream"""
    row_env('solve_fb')
    nbr = S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE
    for seed in block_of(PLAIN_SEEDS, 0):
        s = F.random_scene(seed)
        burst_against_oracle(S, oracle, s, F.random_paths(seed, s), nbr, planned(H, simds, s)[0], ('burst', mode, 'seed', seed)).close()


@pytest.mark.parametrize('div', [None, 1])
def test_auto_burst_with_the_next_tree_built_ahead(S, H, oracle, simds, row_env, monkeypatch, div):
    """form_fuzz.switch_scene(2049) with lists, SCA_NBR_AUTO, three steps per call: behind the first and second pass of a call sca_run_steps
    enqueues the NEXT pass's kd build ahead of that pass's k_waypoint ("an AUTO build enqueued ahead computes no prologue").  The scene
    lists some 260 agents per pass for the kd query, more than an eighth of it: at the default tunables (div None) the back-off takes the
    second call's passes to the plain kd form, compared all the same.  With SCA_AUTO_BACKOFF_DIV=1 no count can start the back-off, and
    all six passes must be AUTO passes (sca_auto_stats): fewer would mean the scene no longer fits the grid, which fails.

    No counter or form bit of the library distinguishes a pass whose tree was built ahead from one that built its own: sca_auto_stats counts
    AUTO passes and listed agents, sca_last_pass_forms has no bit for it, the builds are not counted where a caller can read them.  That the
    branch ran is therefore NOT observed here.  It follows only from the host code: with six AUTO passes and nothing listed beyond what
    auto_lists_too_many allows, auto_next() of sca_forms.h holds behind every pass that has a successor in its call, which is the
    condition of the branch in sca_run_steps.  What the test observes is that bursts in which this condition holds equal the oracle."""
    row_env('solve_fb')
    if div is not None:
        monkeypatch.setenv('SCA_AUTO_BACKOFF_DIV', str(div))                          # read by sca_create
    n = 2049
    s = F.switch_scene(n)
    plan, tun = planned(H, simds, s)
    sol = burst_against_oracle(S, oracle, s, F.random_paths(n, s), S.NBR_AUTO, plan, ('auto burst', div))
    try:
        st = sol.auto_stats()
    finally:
        sol.close()
    assert st['auto_passes'] >= 1, st                                                 # (the scene fits: the first pass is an AUTO pass)
    if div is not None:
        assert st['auto_passes'] == 6 and st['listed_per_pass_max'] * tun['SCA_AUTO_BACKOFF_DIV'] <= n, (st, tun['SCA_AUTO_BACKOFF_DIV'])


def test_step_host_with_lists(S, H, oracle, simds, row_env):
    """sca_step_host(state, vpref) on the first block: the block's vpref_mode carries the tracked rows only, so the ingest rewrites every path
    agent's mode to 0 each step and k_waypoint has to set it again.  The block's state and action rows, and everything else, are the oracle's."""
    row_env('solve_fb')
    for seed in block_of(PLAIN_SEEDS, 0):
        s = F.random_scene(seed)
        n = s['n']
        paths = F.random_paths(seed, s)
        ref = F.oracle_run(oracle, s, STEPS, paths=paths)
        plan = planned(H, simds, s)[0]
        sol = context_of(S, s, None, paths, state=False)
        try:
            blk = sol.host_state()
            for k in ('pos', 'vel', 'heading', 'flags'):
                blk[k][...] = s[k]
            blk['total_dist'][:] = 0.0
            blk['step_num'][:] = 0
            blk['vpref'][...] = s['vpref']
            blk['vpref_mode'][:] = s['vmode']
            sol.set_kd_perm(np.arange(n, dtype=np.int32))
            for t, r in enumerate(ref):
                active = sol.step_host(S.NBR_KDTREE, state=True, vpref=True)
                at = ('step_host', 'seed', seed, 'n', n, 'step', t)
                forms = sol.pass_forms()
                assert (forms & SOLVE_BITS) == plan['forms'] and forms & S.FORM_WAYPOINTS, at + ('forms', forms, plan)
                assert active == int(((r['flags'] & 7) == 0).sum()), at + ('active', active)
                for k in F.STATE_KEYS:
                    assert np.array_equal(blk[k], r[k]), at + ('block', k)
                assert np.array_equal(blk['action'], r['action']), at + ('block', 'action')
                compare_with_oracle(sol, r, s, at)
                check_paths(sol, r, s, at)
        finally:
            sol.close()


@pytest.mark.parametrize('row', ['packed', 'solve_fb'])
def test_a_shard_inside_the_swarm_with_lists(S, oracle, row_env, row):
    """Seed 28 (100 agents, 30 obstacles), sca_set_shard(33, 50), one policy pass under the packed K1 and under no switch: the shard's action
    rows, neighbour lists, lists and now_goal are those of the oracle's pass over the whole swarm; nobody else's list was touched."""
    row_env(row)
    s = F.random_scene(28)
    n, lo, hi = s['n'], 33, 83
    paths = F.random_paths(28, s)
    r = F.oracle_run(oracle, s, 1, paths=paths)[0]
    shard, length = slice(lo, hi), np.array([len(p) for p in paths])
    served = ((r['before'] & 7) == 0)
    assert n == 100 and s['m'] == 30 and (r['path_left'] < length)[shard].any() and r['path_mode'][shard].any()       # (the scene: what the test needs of it)
    assert (served & (length > 0))[:lo].any() and (served & (length > 0))[hi:].any()                                   # ... somebody outside would have popped
    sol = context_of(S, s, None, paths)
    try:
        sol.set_shard(lo, hi - lo)
        sol.policy_pass(S.NBR_KDTREE)
        at = ('shard', row)
        assert sol.pass_forms() & S.FORM_WAYPOINTS, at
        assert np.array_equal(sol.get_kd_perm(), r['perm']), at
        compare_pass_with_oracle(sol, r, at, (s['policy'] == 4)[shard], shard)
        check_paths(sol, r, s, at, shard)
        rem, ng = sol.get_path_state()
        outside = np.r_[0:lo, hi:n]
        assert np.array_equal(rem[outside], length[outside]) and np.isnan(ng[outside]).all(), at + ('a list outside the shard moved',)
        nb = sol.neighbors()
        assert not nb['nbr_valid'][outside].any() and not nb['nbr_n'][outside].any(), at
    finally:
        sol.close()


@pytest.mark.parametrize('name', FIXTURES)
@pytest.mark.parametrize('row', list(F.ROWS))
def test_recorded_episodes_under_every_row(S, row_env, row, name):
    """the five F19 episodes, free-running, the device tracker in the pass where the episode has tracked agents (its neighbour branch on
    the side stream beside k_waypoint in the split and packed forms): the reference's own values under every row"""
    row_env(row)
    assert run_recorded_episode(S, name, S.NBR_KDTREE, (name, row)) == len(load_episode(name)['step'])


GRID_OVERFLOWS = {'F19_path_orca_circle16_obs': 52}      # the first step at which a list of the episode holds more than max_neighbors objects


@pytest.mark.parametrize('name', FIXTURES)
def test_recorded_episodes_in_the_grid(S, row_env, name):
    """... and in SCA_NBR_GRID (no tree: the permutation is not compared).  An episode the grid refuses is refused at its first pass with the
    grid's own words.  Four episodes never fill a list and equal the reference to their last record.  In the circle of 16 with obstacles
    three lists overflow in the pass of step 52 (status 32 on agents 4, 9 and 15): from there the grid's contract is its own list rule, not
    the reference's visit-order-dependent list (include/sca_hip.h) -- measured on the MI355X, the action rows leave the recorded ones at
    step 60 -- so this episode is compared up to that pass, 52 steps, and the rule-1 oracle legs above are what holds overflowed lists
    with waypoints to a reference."""
    row_env('solve_fb')
    refused, overflowed = [], []

    def on_refusal(e):
        assert 'SCA_NBR_GRID needs radius + collision reach <= neighbor_dist' in str(e), (name, str(e))
        refused.append(name)
    got = run_recorded_episode(S, name, S.NBR_GRID, (name, 'grid'), grid=True, on_refusal=on_refusal, on_overflow=overflowed.append)
    assert (got > 0) != bool(refused), (name, got, refused)
    if not refused:
        assert overflowed == ([GRID_OVERFLOWS[name]] if name in GRID_OVERFLOWS else []), (name, overflowed)
        steps = [int(t) for t in load_episode(name)['step']]
        assert got == (steps.index(overflowed[0]) if overflowed else len(steps)), (name, got)


BATCH_SEEDS = (23, 11, 4, 10)                  # 1 agent + 5 obstacles, 2 agents + none, 257 + 30, 400 + 30


@pytest.mark.parametrize('packed', [0, 1])
def test_one_scene_batch_with_lists(S, H, oracle, simds, row_env, monkeypatch, packed):
    """four corpus scenes with their lists as the scenes of ONE context (sca_set_scenes, one obstacle set per scene), in both K1 scene forms:
    every scene equals its own oracle run, alone"""
    row_env('solve_fb')
    monkeypatch.setenv('SCA_K1_PACKED', str(packed))                                  # read by sca_create
    scenes = [F.random_scene(seed) for seed in BATCH_SEEDS]
    lists = [F.random_paths(seed, s) for seed, s in zip(BATCH_SEEDS, scenes)]
    assert [(s['n'], s['m']) for s in scenes] == [(1, 5), (2, 0), (257, 30), (400, 30)]
    refs = [F.oracle_run(oracle, s, STEPS, paths=p) for s, p in zip(scenes, lists)]
    eps = [dict(s, zaxis=F.zaxis_of(s)) for s in scenes]
    sol, off = U.context(S, eps, obstacles=[(s['obs_pos'], s['obs_radius']) for s in scenes], tracker=False)
    try:
        cat = lambda key: np.concatenate([s[key] for s in scenes])                    # noqa: E731
        n = int(off[-1])
        obs_off = sol.scene_obstacle_offsets
        sol.set_paths([p for ps in lists for p in ps])
        sol.set_vpref(cat('vpref'), cat('vmode'))
        sol.set_state(cat('pos'), cat('vel'), cat('heading'), cat('flags'), np.zeros(n), np.zeros(n, np.int32))
        whole = dict(n=n, policy=cat('policy'))
        plan = planned(H, simds, whole)[0]
        for t in range(STEPS):
            sol.run_steps(1, S.NBR_KDTREE)
            sol.synchronize()
            forms = sol.pass_forms()
            want = S.FORM_WAYPOINTS | S.FORM_SCENES | S.FORM_SCENE_OBSTACLES
            assert (forms & SOLVE_BITS) == plan['forms'] and (forms & want) == want, ('batch', packed, t, forms, plan)
            got = U.everything(sol)
            for k, (s, r) in enumerate(zip(scenes, refs)):
                lo, hi, at = int(off[k]), int(off[k + 1]), ('batch', 'packed', packed, 'scene', k, 'seed', BATCH_SEEDS[k], 'step', t)
                r = r[t]
                U.assert_scene_equals_alone(got, lo, hi, int(obs_off[k]), {key: r[key] for key in F.STATE_KEYS + ('action', 'perm')}, at)
                compare_pass_with_oracle(sol, r, at, s['policy'] == 4, slice(lo, hi), slice(None), (lo, int(obs_off[k])))
                check_paths(sol, r, s, at, slice(lo, hi), slice(None))
    finally:
        sol.close()
