"""The cell-owner partition (sca_partition_*, sca_amd/csrc/sca_partition.hip.h) with all ranks in one process, against the rule-1 oracle and a
model of ownership (-m gpu).

tests/partition_ranks.py drives `world` contexts as the ranks of one swarm and hands their packed buffers over directly; the scenes are
form_fuzz.cut_scene's: a few hundred agents placed on the cuts (tests/test_partition_fuzz_cpu.py counts what they hold).  The oracle's rule-1
run of the whole swarm does not depend on who holds what, so after EVERY step of every scene, for every agent:

    owner sets      partition_owned() of rank r is the model's owner set (a function of the position: the sets partition the swarm)
    halo counts     partition_counts() is (model owned, model halo) on every rank
    state           the rank that owns the agent AFTER the step holds the oracle's flags, step_num, vel, pos, heading, total_dist
    travelled       ... and its action row, n_suit / fallback, planeFail / lp4, the v_pref used and the status word (overflow rule of
                    test_gpu_grid_fuzz.compare_grid_step) -- for a migrant what travelled in PartMig
    lists           the rank that owned it BEFORE the step ran the pass: nbr_valid, nbr_n and the list entry for entry in the grid's order
    headers         the first 16 bytes of every outgoing buffer: the model's n_halo and n_mig, and the caps

All comparisons are equality.  A failure names scene, step, rank, agent ids and quantity.

Legs: (a) the 24 plain cut scenes at the default forms and under the `large_shard` row; (b) 8 with per-agent attributes (cells of 4 m);
(c) the 80 m-box scenes of the random corpus with the library's own cuts, refused exactly where the model says; (d) the device tracker
beside a plain-grid context; (e) sca_set_state under a standing partition; (f) message capacities: the overflow is an error return at the step
the model names, and the smallest sufficient caps run clean; (g) one rank, the in-library path."""
import numpy as np
import pytest

import form_fuzz as F
import partition_ranks as PR
import test_partition_fuzz_cpu as CPU
from test_gpu_form_fuzz import S, context_of, row_env                                # noqa: F401 (fixtures)
from test_gpu_grid_fuzz import compare_grid_step

pytestmark = pytest.mark.gpu

STEPS = CPU.STEPS
SCA_ERR_ARG = -1


def msg(at, *parts):
    """a failure's message as one string (a long tuple is cut short in a report): scene, step, rank, agents, quantity"""
    return ' '.join(str(x) for x in tuple(at) + parts)


def default_caps(n):
    """the entries per message sca_partition_init takes for cap_halo = cap_mig = 0 (include/sca_hip.h)"""
    return max(1024, n // 4), max(256, n // 16)


def check_step(ranks, M, scene, r, p0, own_before, at, caps):
    """everything of the module's head after one step; r: the oracle's record of the step, p0: the positions it started from, own_before:
    the owner sets it started from.  Returns the owner sets after it."""
    p1 = r['pos']
    owner = M.owner(p1)
    got = ranks.owned()
    for k, sol in enumerate(ranks.sols):
        want = np.flatnonzero(owner == k)
        assert np.array_equal(got[k], want), msg(at, 'rank', k, 'owned: agents', sorted(set(got[k].tolist()) ^ set(want.tolist()))[:8])
        counts = (len(want), int(M.halo(p1, k).sum()))
        assert sol.partition_counts() == counts, msg(at, 'rank', k, 'owned / halo counts', sol.partition_counts(), counts)
    heads = ranks.headers()
    for k in range(ranks.world):
        want = M.headers(k, p0, p1)
        for side in (0, 1):
            assert (heads[k][side] is None) == (want[side] is None), msg(at, 'rank', k, 'side', side)
            if want[side] is not None:
                assert heads[k][side].tolist() == list(want[side]) + list(caps), msg(at, 'rank', k, 'side', side, 'header', heads[k][side].tolist(),
                                                                                     list(want[side]) + list(caps))
    for k, sol in enumerate(ranks.sols):
        compare_grid_step(sol, r, scene, at + ('rank', k), rows=got[k], list_rows=own_before[k], vpref=True)
    return got


def run_ranks_against_oracle(S, oracle, scene, world, axis, cuts, steps, ctx, per_agent=None, nd=10.0, cap_halo=0, cap_mig=0, cell_cuts=None):
    """`world` ranks, `steps` steps, check_step after each.  cuts=None with cell_cuts: the library cuts by itself, the model is given what
    the rule says.  Returns the agents that changed owner."""
    ref = F.oracle_run(oracle, scene, steps, per_agent, list_rule=1)
    M = PR.Model(world, axis, cuts, nd, cell_cuts=cell_cuts)
    caps = tuple(c or d for c, d in zip((cap_halo, cap_mig), default_caps(scene['n'])))
    ranks = PR.Ranks(S, scene, world, axis, cuts, per_agent, cap_halo, cap_mig)
    moved = 0
    try:
        p0 = scene['pos']
        own = ranks.owned()
        owner = M.owner(p0)
        for k, sol in enumerate(ranks.sols):
            want = np.flatnonzero(owner == k)
            assert np.array_equal(own[k], want), msg(ctx, 'init', 'rank', k, 'owned: agents', sorted(set(own[k].tolist()) ^ set(want.tolist()))[:8])
            assert sol.partition_counts() == (len(want), int(M.halo(p0, k).sum())), msg(ctx, 'init', 'rank', k, 'counts', sol.partition_counts())
        for t, r in enumerate(ref):
            ranks.step()
            moved += int((M.owner(r['pos']) != M.owner(p0)).sum())
            own = check_step(ranks, M, scene, r, p0, own, ctx + ('n', scene['n'], 'step', t), caps)
            p0 = r['pos']
    finally:
        ranks.close()
    return moved


# ---- (a) --------------------------------------------------------------------------------------------------------------------------------------
PLAIN = CPU.CASES['plain']
PER_TEST = 6


@pytest.mark.parametrize('block,row', [(b, row) for b in range(len(PLAIN) // PER_TEST) for row in ('solve_fb', 'large_shard')])
def test_ranks_on_the_plain_cut_scenes(S, oracle, row_env, block, row):
    """six of the 24 plain cut scenes (one world per block: axes 0, 1, 2 x two seeds), 12 steps, at the default forms (`solve_fb`: no switch
    set) and under the `large_shard` row (packed K1, two-launch solve, fallback launch: what every large shard runs)"""
    row_env(row)
    moved = 0
    for w, a, sd in PLAIN[PER_TEST * block: PER_TEST * (block + 1)]:
        s, cuts = F.cut_scene(sd, w, a)
        moved += run_ranks_against_oracle(S, oracle, s, w, a, cuts, STEPS, (row, 'cut scene', (w, a, sd)))
    assert moved > 0, (block, row)


# ---- (b) --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('half', (0, 1))
def test_ranks_on_the_cut_scenes_with_per_agent_attributes(S, oracle, row_env, half):
    """four of the 8 per-agent cut scenes: neighbor_dist 1.5 / 2.5 / 4.0 per agent (cells of about 4 m), time_step up to 0.2, max_speed up to 3.0"""
    row_env('solve_fb')
    moved = 0
    for case in CPU.CASES['per_agent'][4 * half: 4 * half + 4]:
        s, cuts, pa, nd = CPU.scene_of('per_agent', case)
        moved += run_ranks_against_oracle(S, oracle, s, case[0], case[1], cuts, STEPS, ('per agent', 'cut scene', case), per_agent=pa, nd=nd)
    assert moved > 0, half


# ---- (c) --------------------------------------------------------------------------------------------------------------------------------------
NULL_CASES = CPU.null_cut_cases()


@pytest.mark.parametrize('block', (0, 1))
def test_the_librarys_own_cuts_on_the_80_m_scenes(S, oracle, row_env, block):
    """cuts = NULL (equal shares of the agents as they stand), world 2 .. 4, six steps against the memoised rule-1 runs of the random corpus.
    Where the model of the rule says an interior rank gets fewer than two layers, sca_partition_init refuses with SCA_ERR_ARG on every rank;
    nowhere else does it raise."""
    row_env('solve_fb')
    inv = PR.inv_cell_of(10.0)
    ran = 0
    for seed, w, ok in NULL_CASES:
        if seed // F.BLOCK != block:
            continue
        s = F.random_scene(seed)
        ctx = ('NULL cuts', 'seed', seed, 'world', w)
        if ok:
            run_ranks_against_oracle(S, oracle, s, w, 0, None, 6, ctx, cell_cuts=PR.equal_share_cells(s['pos'], w, 0, inv))
            ran += 1
            continue
        for r in range(w):
            sol = context_of(S, s, perm=False)
            try:
                with pytest.raises(S.ScaError, match=r'fewer than two layers.*rc=%d\)' % SCA_ERR_ARG):
                    sol.partition_init(r, w, 0, None)
            finally:
                sol.close()
    assert ran > 0, block


@pytest.mark.parametrize('world,cuts', CPU.REFUSED_CUTS)
def test_cuts_that_leave_an_interior_rank_fewer_than_two_layers_are_refused(S, world, cuts):
    s, _ = F.cut_scene(0, 3, 0)
    sol = context_of(S, s, perm=False)
    try:
        for r in range(world):
            with pytest.raises(S.ScaError, match=r'fewer than two layers.*rc=%d\)' % SCA_ERR_ARG):
                sol.partition_init(r, world, 0, cuts)
    finally:
        sol.close()


# ---- (d) --------------------------------------------------------------------------------------------------------------------------------------
def _state_equal(sol, ref, rows, at):
    got, want = sol.get_state(), ref.get_state()
    for k in F.STATE_KEYS:
        differ = (got[k][rows] != want[k][rows]).reshape(len(rows), got[k][0].size).any(axis=1)
        assert not differ.any(), msg(at, k, 'agents', rows[np.flatnonzero(differ)][:8].tolist())
    differ = (sol.actions()[rows] != ref.actions()[rows]).any(axis=1)
    assert not differ.any(), msg(at, 'action', 'agents', rows[np.flatnonzero(differ)][:8].tolist())


@pytest.mark.parametrize('world,axis,seed', F.CUT_TRACKED)
def test_ranks_with_the_device_tracker(S, row_env, world, axis, seed):
    """policy 0 agents under device_tracker_enable: the tracker's record travels with a migrant.  The reference is one plain-grid context with
    the device tracker stepped beside the ranks (that pairing is oracle-checked by tests/test_gpu_tracker_oracle.py): state, action rows and
    re-plan counts of the owned rows every step, and at least one agent with a re-plan behind it crossed a cut."""
    row_env('solve_fb')
    s, cuts = F.cut_scene(seed, world, axis, policies=(0,))
    n = s['n']
    M = PR.Model(world, axis, cuts)
    goal_heading = np.zeros((n, 3))
    ranks, ref = PR.Ranks(S, s, world, axis, cuts, tracker=goal_heading), context_of(S, s, perm=False)
    crossed_after_a_replan = 0
    try:
        ref.device_tracker_enable(goal_heading)
        before = M.owner(s['pos'])
        for t in range(STEPS):
            ranks.step()
            ref.run_steps(1, S.NBR_GRID)
            ref.synchronize()
            at = ('tracked cut scene', (world, axis, seed), 'n', n, 'step', t)
            owner = M.owner(ref.get_state()['pos'])
            replans = ref.device_tracker_replans()
            for k, (sol, own) in enumerate(zip(ranks.sols, ranks.owned())):
                want = np.flatnonzero(owner == k)
                assert np.array_equal(own, want), msg(at, 'rank', k, 'owned: agents', sorted(set(own.tolist()) ^ set(want.tolist()))[:8])
                _state_equal(sol, ref, own, at + ('rank', k))
                differ = sol.device_tracker_replans()[own] != replans[own]
                assert not differ.any(), msg(at, 'rank', k, 're-plans', 'agents', own[np.flatnonzero(differ)][:8].tolist())
            crossed_after_a_replan += int(((owner != before) & (replans > 0)).sum())
            before = owner
    finally:
        ranks.close()
        ref.close()
    assert crossed_after_a_replan > 0, (world, axis, seed)


# ---- (e) --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('world,axis,seed', [(3, 0, 0), (4, 1, 1), (5, 2, 0)])
def test_set_state_under_a_standing_partition(S, row_env, world, axis, seed):
    """after step 6 the owned rows of all ranks, gathered into one complete state, go to every rank and to a plain-grid context that ran
    beside them (sca_set_state: ownership is derived a second time); ownership equals the model right after the call, and every one of
    six more steps equals the plain context"""
    row_env('solve_fb')
    s, cuts = F.cut_scene(seed, world, axis)
    M = PR.Model(world, axis, cuts)
    ranks, ref = PR.Ranks(S, s, world, axis, cuts), context_of(S, s, perm=False)
    try:
        for t in range(12):
            if t == 6:
                state = ranks.gather(lambda sol: sol.get_state())
                for k in F.STATE_KEYS:
                    assert np.array_equal(state[k], ref.get_state()[k]), ('gathered', k)
                ranks.set_state(state)
                ref.set_state(state['pos'], state['vel'], state['heading'], state['flags'], state['total_dist'], state['step_num'])
                owner = M.owner(state['pos'])
                for k, (sol, own) in enumerate(zip(ranks.sols, ranks.owned())):
                    assert np.array_equal(own, np.flatnonzero(owner == k)), ('after set_state', 'rank', k)
                    assert sol.partition_counts() == (int((owner == k).sum()), int(M.halo(state['pos'], k).sum())), ('after set_state', 'rank', k)
            ranks.step()
            ref.run_steps(1, S.NBR_GRID)
            ref.synchronize()
            at = ('cut scene', (world, axis, seed), 'step', t)
            owner = M.owner(ref.get_state()['pos'])
            for k, (sol, own) in enumerate(zip(ranks.sols, ranks.owned())):
                assert np.array_equal(own, np.flatnonzero(owner == k)), msg(at, 'rank', k, 'owned')
                _state_equal(sol, ref, own, at + ('rank', k))
    finally:
        ranks.close()
        ref.close()


# ---- (f) --------------------------------------------------------------------------------------------------------------------------------------
CAP_SCENE = (4, 1, 1)                                                                # 257 agents, four ranks


def _first_step_over(M, positions, cap_halo, cap_mig):
    """the first step at which, by the model, some message holds more halo entries or more migrants than the caps"""
    for t, (a, b) in enumerate(zip(positions[:-1], positions[1:])):
        for r in range(M.world):
            for h in M.headers(r, a, b):
                if h is not None and (h[0] > cap_halo or h[1] > cap_mig):
                    return t
    return None


@pytest.mark.parametrize('which', ('cap_halo', 'cap_mig'))
def test_a_message_over_its_capacity_is_an_error_return(S, oracle, row_env, which):
    """cap_halo = 1, then cap_mig = 1, on a scene that by the model sends at least 2 halo entries and at least 2 migrants in one message:
    partition_commit or the next synchronize() raises, naming the overflow, at the first step at which the model has a message over the cap
    (k_part_pack writes only the entries below the cap, k_part_unpack clamps both counts to its own caps); nothing is stepped afterwards and
    the contexts close"""
    row_env('solve_fb')
    w, a, sd = CAP_SCENE
    s, cuts = F.cut_scene(sd, w, a)
    M = PR.Model(w, a, cuts)
    positions = [s['pos']] + [r['pos'] for r in F.oracle_run(oracle, s, STEPS, list_rule=1)]
    assert max(h[0] for x, y in zip(positions[:-1], positions[1:]) for r in range(w) for h in M.headers(r, x, y) if h) >= 2
    assert max(h[1] for x, y in zip(positions[:-1], positions[1:]) for r in range(w) for h in M.headers(r, x, y) if h) >= 2
    dh, dm = default_caps(s['n'])
    caps = dict(cap_halo=1) if which == 'cap_halo' else dict(cap_mig=1)
    first = _first_step_over(M, positions, caps.get('cap_halo', dh), caps.get('cap_mig', dm))
    assert first is not None
    ranks = PR.Ranks(S, s, w, a, cuts, **caps)
    try:
        for t in range(first):
            ranks.step()
        with pytest.raises(S.ScaError, match='overflowed its capacity'):
            ranks.step()
        assert ranks.dead
        with pytest.raises(AssertionError):
            ranks.step()
    finally:
        ranks.close()


def test_the_smallest_caps_the_model_says_suffice_run_clean(S, oracle, row_env):
    row_env('solve_fb')
    w, a, sd = CAP_SCENE
    s, cuts = F.cut_scene(sd, w, a)
    positions = [s['pos']] + [r['pos'] for r in F.oracle_run(oracle, s, STEPS, list_rule=1)]
    nh, nm = PR.Model(w, a, cuts).caps_needed(positions)
    assert nh >= 2 and nm >= 2, (nh, nm)
    assert run_ranks_against_oracle(S, oracle, s, w, a, cuts, STEPS, ('smallest caps', (nh, nm)), cap_halo=nh, cap_mig=nm) > 0


# ---- (g) --------------------------------------------------------------------------------------------------------------------------------------
def test_one_rank_on_cut_scenes(S, oracle, row_env):
    """world = 1: the in-library path (sca_run_steps does the commit itself) under the same comparison -- nothing is sent, everything is owned"""
    row_env('solve_fb')
    for w, a, sd in ((2, 0, 0), (4, 1, 1), (5, 2, 1)):
        s, _ = F.cut_scene(sd, w, a)
        assert run_ranks_against_oracle(S, oracle, s, 1, a, [], STEPS, ('one rank', 'cut scene', (w, a, sd))) == 0
