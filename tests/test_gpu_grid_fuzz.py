"""SCA_NBR_GRID on the random-scene corpus and beyond the first overflow, against an oracle of its own list rule (-m gpu).

The grid's contract (include/sca_hip.h, the head of sca_grid.hip.h) is deterministic: lists sorted by (distSq, obstacles first, agent id), the
nearest max_neighbors kept, the collision rule order-free.  oracle.set_list_rule(1) computes exactly that in front of the unchanged rest of the
policy pass (tests/test_grid_rule_cpu.py pins it to the reference's rule and to an all-pairs search), so every row has an expected list and an
expected action row, overflowed or not.  Here the fuzz scenes of tests/form_fuzz.py run free for six resident steps in SCA_NBR_GRID, one
context per scene; after every step flags, step counts, float32 velocities, positions, headings, travelled distance, the action rows, the
lists entry for entry in the grid's own order and the decisions' diagnostics EQUAL the rule-1 oracle's.  No row is left out, nothing is sorted,
no tolerance.  The kd permutation is not compared: the grid builds no tree.

Status words: no bit outside 32 | 64 | 128; SCA_ST_NBR_OVERFLOW wherever the oracle sets it, and beyond that only on rows whose collision
flag this very pass raised (the kernel may have seen a full list before it met the first colliding object; the oracle counts what is admitted
after it).

Legs: the plain scenes at the default forms and under the `large_shard` row (overflowed lists are what feeds the fallback launch and the
two-launch solve), the per-agent scenes at the default forms (max_neighbors 1 .. 16 and neighbor_dist per agent), two plain blocks behind the
one-rank cell-owner partition, and two episodes that go on long after their first overflow."""
import ctypes as C

import numpy as np
import pytest

import form_fuzz as F
from test_forms_cpu import H, from_env, solve                                       # noqa: F401 (H: fixture)
from test_gpu_form_fuzz import S, SOLVE_BITS, check_paths, context_of, row_env, simds       # noqa: F401 (fixtures)
from test_grid_rule_cpu import GRID_MAY_REFUSE

pytestmark = pytest.mark.gpu

STEPS = 6
OVERFLOW = 32
K = F.K


def planned(H, simds, scene, part_on=0):
    """plan_solve for this scene under the environment of the moment"""
    t = from_env(H, simds)
    lp = int((scene['policy'] == 4).sum())
    return solve(H, scene['n'], simds=simds, part_on=part_on, nranks=1, lp=lp, lp_total=lp, t=(C.c_int * len(t))(*t.values()))


def compare_grid_step(sol, r, scene, at, rows=None, list_rows=None, vpref=False, nan_equal=False):
    """What a context holds after a resident step in SCA_NBR_GRID against the rule-1 oracle's record `r` of that step; failures name the
    agents.  rows: the ids of the agents whose state (flags, step counts, float32 velocities, positions, headings, travelled distance) and
    results (action rows, diagnostics, status words) are compared -- None: every agent; under the cell-owner partition the agents the rank owns
    AFTER the step (a migrant's results travelled with it).  list_rows: the ids whose neighbour lists are compared entry for entry in the
    grid's own order (None: `rows`; under the partition the agents the rank owned BEFORE the step: it ran the pass).  vpref: the v_pref the
    pass used is compared too, on the served rows.  Returns how many of list_rows the oracle has overflowed.  nan_equal: a NaN equals a NaN
    at the same place (the degenerate-geometry family's one relaxation, golden_util.equal_for)."""
    rows = np.arange(scene['n']) if rows is None else np.asarray(rows, np.int64)

    def ne(got, want):
        d = got != want
        if nan_equal and got.dtype.kind == 'f':
            d &= ~(np.isnan(got) & np.isnan(want))
        return d

    lrows = rows if list_rows is None else np.asarray(list_rows, np.int64)

    def same(bad, what, of=rows, got=None, want=None):
        """no row of `bad`; else the failure names the place, the quantity, the agents and the first one's two values"""
        if np.any(bad):
            k = np.flatnonzero(bad)
            first = () if got is None else ('agent', int(of[k[0]]), 'holds', got[k[0]].tolist(), 'oracle', want[k[0]].tolist())
            raise AssertionError(' '.join(str(x) for x in at + (what, 'agents', of[k][:8].tolist()) + first))
    g = sol.get_state()
    for k in ('flags', 'step_num', 'vel', 'pos', 'heading', 'total_dist'):
        got, want = g[k][rows], r[k][rows]
        same(ne(got, want).reshape(len(rows), got[0].size if len(rows) else 1).any(axis=1), k, got=got, want=want)
    a = sol.actions()[rows]
    same(ne(a, r['action'][rows]).any(axis=1), 'action', got=a, want=r['action'][rows])
    nb = {k: v[lrows] for k, v in sol.neighbors().items()}
    valid, want_n = r['nbr_valid'][lrows].astype(bool), r['nbr_n'][lrows]
    same(nb['nbr_valid'].astype(bool) != valid, 'nbr_valid', lrows)
    same(valid & (nb['nbr_n'] != want_n), 'nbr_n', lrows, nb['nbr_n'], want_n)
    live = valid[:, None] & (np.arange(K)[None, :] < want_n[:, None])
    for k in ('nbr_id', 'nbr_kind', 'nbr_dsq'):
        same((live & (nb[k] != r[k][lrows])).any(axis=1), k, lrows, nb[k], r[k][lrows])
    dg = sol.diag()
    lp = (scene['policy'] == 4)[rows]
    got, want = dg['diag'][rows], r['diag'][rows]
    same((got[:, :2] != want[:, :2]).any(axis=1), 'n_suit / fallback', got=got, want=want)
    same(lp & (got[:, 3:5] != want[:, 3:5]).any(axis=1), 'planeFail / lp4', got=got, want=want)
    st = dg['status'][rows]
    same((st & ~(OVERFLOW | 64 | 128)) != 0, 'status bits', got=st, want=r['status'][rows])
    over, over_ref = (st & OVERFLOW) != 0, (r['status'][rows] & OVERFLOW) != 0
    same(over_ref & ~over, 'overflow not reported')
    collided_now = (((r['flags_policy'] & 2) != 0) & ((r['before'] & 2) == 0))[rows]
    same(over & ~over_ref & ~collided_now, 'spurious overflow')
    if vpref:
        served = ((r['before'] & 7) == 0)[rows]
        same(served & (dg['vpref'][rows] != r['vpref'][rows]).any(axis=1), 'v_pref used', got=dg['vpref'][rows], want=r['vpref'][rows])
    return int((((r['status'][lrows] & OVERFLOW) != 0) & valid).sum())


def run_grid_against_oracle(S, oracle, scene, steps, per_agent, plan, ctx, partition=False, may_refuse=False, paths=None):
    """One context, `steps` resident steps in SCA_NBR_GRID, everything compared with the rule-1 oracle after each.  Returns None where the
    library refused the scene at its first pass (may_refuse), else the overflowed rows the oracle had per step.  paths: the scene's waypoint
    lists (form_fuzz.random_paths) -- the rule-1 run with lists, and the lists, now_goal and the v_pref used are compared too."""
    s, n = scene, scene['n']
    ref = F.oracle_run(oracle, s, steps, per_agent, list_rule=1, paths=paths)
    sol = context_of(S, s, per_agent, paths, perm=False)
    overflowed = []
    try:
        if partition:
            sol.partition_init(0, 1, axis=0)
            assert sol.partition_counts() == (n, 0), ctx
        for t, r in enumerate(ref):
            at = ctx + ('n', n, 'step', t)
            try:
                sol.run_steps(1, S.NBR_GRID)
            except S.ScaError as e:
                assert may_refuse and t == 0 and 'SCA_NBR_GRID needs' in str(e), at + (str(e),)
                return None
            sol.synchronize()
            if partition:
                assert sol.partition_counts() == (n, 0), at
            forms = sol.pass_forms()
            assert (forms & SOLVE_BITS) == plan['forms'], at + ('forms', forms, plan)
            assert bool(forms & S.FORM_WAYPOINTS) == (paths is not None), at + ('forms', forms)
            overflowed.append(compare_grid_step(sol, r, s, at))
            if paths is not None:
                check_paths(sol, r, s, at)
    finally:
        sol.close()
    return overflowed


def _legs():
    """block-major: the legs of a block one after the other share its oracle runs (form_fuzz.oracle_run keeps a block or two)"""
    out = []
    for b in range(len(F.PLAIN_SEEDS) // F.BLOCK):
        for leg in ('default', 'large_shard') + (('partition',) if b in (0, 3) else ()):
            out.append(pytest.param(leg, b, id='%s-%d' % (leg, b)))
    return out


@pytest.mark.parametrize('leg,block', _legs())
def test_grid_on_the_plain_scenes(S, H, oracle, simds, row_env, leg, block):
    """20 scenes of the plain corpus (seeds 0-119): n = 1 .. 1600 with ragged 16-lane groups, 4 m boxes with far more than 16 in range and
    more than max_neighbors colliding, 80 m boxes around the origin (cells below zero, a thousand cells in a few thousand buckets), obstacles"""
    row_env('large_shard' if leg == 'large_shard' else 'solve_fb')                  # (`solve_fb`: no switch set)
    seen = 0
    for seed in F.PLAIN_SEEDS[F.BLOCK * block: F.BLOCK * (block + 1)]:
        s = F.random_scene(seed)
        plan = planned(H, simds, s, part_on=int(leg == 'partition'))
        if leg == 'large_shard':
            assert plan['forms'] == (S.FORM_SOLVE_SPLIT | (S.FORM_LP_LANE if (s['policy'] == 4).any() else 0)), (seed, plan)
        seen += sum(run_grid_against_oracle(S, oracle, s, STEPS, None, plan, (leg, 'seed', seed), partition=leg == 'partition'))
    assert seen > 0, (leg, block)


@pytest.mark.parametrize('block', range(len(F.PER_AGENT_SEEDS) // F.BLOCK))
def test_grid_on_the_scenes_with_per_agent_attributes(S, H, oracle, simds, row_env, block):
    """20 scenes of the per-agent corpus (seeds 1000-1059): max_neighbors 1 .. 16 and neighbor_dist per agent (or one value of each per scene).
    The library may refuse a scene whose largest neighbor_dist cannot hold the collision check's partners -- those of GRID_MAY_REFUSE
    (tests/test_grid_rule_cpu.py derives the set from the corpus) and no other."""
    row_env('solve_fb')
    seen, refused = 0, []
    for seed in F.PER_AGENT_SEEDS[F.BLOCK * block: F.BLOCK * (block + 1)]:
        s = F.random_scene(seed)
        pa = F.per_agent_attributes(seed, s['n'])
        got = run_grid_against_oracle(S, oracle, s, STEPS, pa, planned(H, simds, s), ('per_agent', 'seed', seed), may_refuse=seed in GRID_MAY_REFUSE)
        if got is None:
            refused.append(seed)
        else:
            seen += sum(got)
    assert set(refused) <= set(GRID_MAY_REFUSE), refused                              # (every other scene ran: a refusal there fails inside)
    assert seen > 0, block


def _episode(kind):
    from sca_amd import scenarios
    if kind == 'takeoff':                                                            # test_gpu_grid's episode: overflows from step 3 on
        n = 1024
        sc = scenarios.takeoff_landing(n)
        policy = np.where(np.arange(n) % 2 == 0, 0, 2).astype(np.uint8)
    else:                                                                            # test_gpu_auto's dense blob: ~40 agents within neighborDist
        from test_gpu_auto import _scene
        sc, policy, n = _scene('dense', 600, 5)
    return dict(n=n, m=len(sc['obs_radius']), pos=sc['start'][:, :3].copy(), goal=sc['goal'][:, :3].copy(), heading=sc['start'][:, 3:6].copy(),
                vel=np.zeros((n, 3), np.float32), radius=np.full(n, 0.5), pref_speed=np.ones(n), policy=policy, flags=np.zeros(n, np.uint8),
                obs_pos=sc['obs_pos'].reshape(-1, 3), obs_radius=sc['obs_radius'], vpref=np.zeros((n, 3)), vmode=np.zeros(n, np.uint8),
                max_run_dist=scenarios.max_run_dist(sc['start'], sc['goal']), key=('episode', kind))


@pytest.mark.parametrize('kind,steps', [('takeoff', 40), ('dense', 12)])
def test_grid_episode_beyond_the_first_overflow(S, H, oracle, simds, row_env, kind, steps):
    """scenarios.takeoff_landing(1024), policies 0 / 2 alternating (a lattice of identical cells: equal distances everywhere, 8 obstacles per
    cell), 40 steps, and the 600-agent dense blob, 12 steps: the comparison with the kd-tree run ends at the first overflow (step 3 of the
    take-off); this one goes on, every row at every step"""
    row_env('solve_fb')
    s = _episode(kind)
    got = run_grid_against_oracle(S, oracle, s, steps, None, planned(H, simds, s), (kind,))
    assert sum(got[4:]) > 0, got
