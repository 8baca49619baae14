"""The kd QUERIES on deep, lopsided trees, up to the stack limits and one entry beyond (-m gpu).

tests/kd_shapes.py holds the scenes -- piles of finished agents or of obstacles on one point, a pile and a geometric progression inside a
crowd, lattices, a slab, two clusters 10^6 m apart -- and a model of the reference's tree and walk that counts the subtrees a walk has
waiting (tests/test_kd_shapes_cpu.py pins it to the host replica and the scenes to the limits).  The walks queue them on fixed stacks: 48
in the one-wavefront K1 and the kd answer of SCA_NBR_AUTO, 64 in the packed K1, K4's fallback walk and the closest-approach descent.

Equality throughout, after every resident step: a row WITHOUT ST_KD_STACK (16) equals the oracle in full -- lists entry for entry, action
rows, diagnostics, state, and the permutation of the whole swarm -- and the rows WITH the bit are exactly the rows the model names for the
form's stack.  A row with the bit is asserted on the bit alone (its lists are invalid), and a run ends with the step in which one appears:
from there the states part.  In a pile every pair is equally far and every box ties, so the lists' order is the visit order and nothing
else."""
import numpy as np
import pytest

import edge_corpus as E
import form_fuzz as F
import kd_shapes as K
import scene_util as U
from test_gpu_clearance import Run
from test_gpu_form_fuzz import S, compare_pass_with_oracle, compare_with_oracle, context_of, row_env       # noqa: F401 (S, row_env: fixtures)
from test_gpu_vacancy import Rule, check_step

pytestmark = pytest.mark.gpu

STEPS = 3
BIT = K.ST_KD_STACK
CORPUS = tuple(n for n in K.NAMES if not n.startswith('touch'))            # (the touch scenes serve nobody in K1: they are K4's)
# form -> (the row of form_fuzz.ROWS, the neighbour mode, the stack its K1 walks have)
FORMS = {'kd': ('solve_fb', 'NBR_KDTREE', K.KD_RSTACK), 'packed': ('packed', 'NBR_KDTREE', K.KD_STACK),
         'hostbuild': ('solve_fb', 'NBR_KDTREE_HOSTBUILD', K.KD_RSTACK), 'auto': ('solve_fb', 'NBR_AUTO', K.KD_RSTACK)}
FLANKS = (11, 23)                                                          # form_fuzz.random_scene: 2 agents + no obstacle, 1 agent + 5 obstacles


def split_rows(status, want, at):
    """the rows with the bit are the model's; returns the mask of the rows without it, whose status words are clear"""
    got = np.flatnonzero(status & BIT)
    assert np.array_equal(got, want), at + ('rows with ST_KD_STACK', got.tolist(), 'the model', want.tolist())
    keep = np.ones(len(status), bool)
    keep[want] = False
    assert not status[keep].any(), at + ('status', status[keep][status[keep] != 0][:8])
    return keep


def run_scene(S, oracle, scene, nbr, cap, ctx):
    ref = F.oracle_run(oracle, scene, STEPS)
    sol = context_of(S, scene)
    try:
        for t, r in enumerate(ref):
            want = K.bit_rows(scene, cap, **K.state_before(scene, ref, t))
            sol.run_steps(1, nbr)
            sol.synchronize()
            at = ctx + ('step', t)
            keep = split_rows(sol.diag()['status'], want, at)
            compare_with_oracle(sol, r, scene, at, rows=slice(None) if keep.all() else keep)
            if not keep.all():
                break
    finally:
        sol.close()


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('name', CORPUS)
def test_every_scene_in_every_query_form(S, oracle, row_env, name, form):
    row, mode, cap = FORMS[form]
    row_env(row)
    run_scene(S, oracle, K.scene(name), getattr(S, mode), cap, (name, form))


def test_the_large_shard_row_across_the_build_switch(S, oracle, row_env):
    row_env('large_shard')
    run_scene(S, oracle, K.scene('lattice_2049'), S.NBR_KDTREE, K.KD_STACK, ('lattice_2049', 'large_shard'))


@pytest.mark.parametrize('packed', [0, 1])
@pytest.mark.parametrize('name', [n for n in CORPUS if K.scene(n)['n'] <= 1536])
def test_the_scene_as_the_middle_one_of_a_batch(S, oracle, row_env, monkeypatch, name, packed):
    """three scenes in one context (sca_set_scenes, one obstacle set per scene), both K1 scene forms: the walk starts at the scene's own roots
    in a forest, ids are global"""
    row_env('solve_fb')
    monkeypatch.setenv('SCA_K1_PACKED', str(packed))                                   # read by sca_create
    cap = K.KD_STACK if packed else K.KD_RSTACK
    scenes = [F.random_scene(FLANKS[0]), K.scene(name), F.random_scene(FLANKS[1])]
    refs = [F.oracle_run(oracle, s, STEPS) for s in scenes]
    sol, off = U.context(S, [dict(s, zaxis=F.zaxis_of(s)) for s in scenes], obstacles=[(s['obs_pos'], s['obs_radius']) for s in scenes], tracker=False)
    try:
        cat = lambda key: np.concatenate([s[key] for s in scenes])                     # noqa: E731
        n = int(off[-1])
        obs_off = sol.scene_obstacle_offsets
        sol.set_vpref(cat('vpref'), cat('vmode'))
        sol.set_state(cat('pos'), cat('vel'), cat('heading'), cat('flags'), np.zeros(n), np.zeros(n, np.int32))
        for t in range(STEPS):
            sol.run_steps(1, S.NBR_KDTREE)
            sol.synchronize()
            assert sol.pass_forms() & S.FORM_SCENES
            got, status = U.everything(sol), sol.diag()['status']
            ended = False
            for j, (s, ref) in enumerate(zip(scenes, refs)):
                lo, hi, at = int(off[j]), int(off[j + 1]), (name, 'packed', packed, 'scene', j, 'step', t)
                want = K.bit_rows(s, cap, **K.state_before(s, ref, t)) if j == 1 else np.zeros(0, np.int64)
                keep = np.flatnonzero(split_rows(status[lo:hi], want, at))
                r = ref[t]
                compare_pass_with_oracle(sol, r, at, (s['policy'] == 4)[keep], lo + keep, keep, (lo, int(obs_off[j])))
                for key in F.STATE_KEYS:
                    assert np.array_equal(got[key][lo:hi][keep], r[key][keep]), at + (key,)
                assert np.array_equal(got['perm'][lo:hi] - lo, r['perm']), at + ('perm',)
                ended |= len(keep) < s['n']
            if ended:
                break
    finally:
        sol.close()


@pytest.mark.parametrize('form', ['kd', 'packed'])
@pytest.mark.parametrize('name', sorted(K.FIXTURES))
def test_the_recordings_of_the_reference(S, row_env, name, form):
    """F21: every recorded step from its recorded state -- lists, action rows and the permutation behind the pass, the state behind the update"""
    row, mode, cap = FORMS[form]
    row_env(row)
    fx = E.fixture(name)
    for t in range(E.steps_of(name)):
        sc = E.step_scene(name, t)
        want = K.bit_rows(sc, cap, perm=sc['perm'], tag=0)
        sol = context_of(S, sc)
        try:
            sol.set_state(sc['pos'], sc['vel'], sc['heading'], sc['flags'], sc['total_dist'], np.zeros(sc['n'], np.int32))
            sol.set_kd_perm(sc['perm'])
            sol.policy_pass(getattr(S, mode))
            at = (name, form, t)
            keep = split_rows(sol.diag()['status'], want, at)
            assert np.array_equal(sol.get_kd_perm(), fx['perm_after'][t]), at
            nb = sol.neighbors()
            valid = fx['nbr_valid'][t].astype(bool)
            assert np.array_equal(nb['nbr_valid'].astype(bool), valid), at
            for k in ('nbr_n', 'nbr_id', 'nbr_kind', 'nbr_dsq'):
                assert np.array_equal(nb[k][valid & keep], fx[k][t][valid & keep]), at + (k,)
            assert np.array_equal(sol.actions()[keep], fx['action'][t][keep]), at + ('action',)
            sol.env_update()
            g = sol.get_state()
            for k in ('pos', 'vel', 'heading', 'total_dist', 'flags'):
                assert np.array_equal(g[k][keep], fx[k + '_after'][t][keep]), at + (k,)
        finally:
            sol.close()


def _touch_batch(S, s):
    flank = F.random_scene(FLANKS[0])
    scenes = [flank, s]
    sol, off = U.context(S, [dict(x, zaxis=F.zaxis_of(x)) for x in scenes], tracker=False)
    sol.set_vpref(np.concatenate([x['vpref'] for x in scenes]), np.concatenate([x['vmode'] for x in scenes]))
    return sol, int(off[1]), [np.concatenate([x[k] for x in scenes]) for k in ('pos', 'vel', 'heading', 'flags')]


@pytest.mark.parametrize('form', ['plain', 'scenes'])
@pytest.mark.parametrize('k', K.TOUCHES)
def test_k4s_fallback_walk_never_drops_a_subtree_silently(S, oracle, row_env, k, form):
    """The env update with no policy pass in front of it: the near lists are invalid and every unsettled row walks (collide_traverse).  The
    tree is the one a pass built over these very positions -- a pass that listed nobody, the live agents being at rest (kd_shapes.touch):
    every status word is clear behind it, then the state is set again.  With 64 subtrees waiting the flags are the oracle's update's, the
    touching row's collision among them; with 65 the touching row carries ST_KD_STACK and the six rows the model clears do not.
    `scenes`: the same as the second scene of a batch (k_collide_finish_scenes, the walk from the scene's own root)."""
    row_env('solve_fb')
    s = K.scene('touch_%d' % k)
    r = F.oracle_run(oracle, s, 1)[0]
    over = np.flatnonzero(K.k4_pending(s) > K.KD_STACK)
    assert over.tolist() == ([6] if k == K.TOUCHES[1] else [])
    if form == 'plain':
        sol, lo, state = context_of(S, s), 0, [s[key] for key in ('pos', 'vel', 'heading', 'flags')]
    else:
        sol, lo, state = _touch_batch(S, s)
    try:
        n = sol.n
        sol.set_state(*state, np.zeros(n), np.zeros(n, np.int32))
        sol.policy_pass(S.NBR_KDTREE)
        assert not sol.diag()['status'].any() and not sol.neighbors()['nbr_valid'][lo:].any()
        sol.set_state(*state, np.zeros(n), np.zeros(n, np.int32))
        sol.env_update()
        at = ('touch', k, form)
        status = sol.diag()['status']
        assert not status[:lo].any(), at
        keep = split_rows(status[lo:], over, at)
        g = sol.get_state()
        for key in F.STATE_KEYS:
            assert np.array_equal(g[key][lo:][keep], r[key][keep]), at + (key,)
        assert (r['flags'][6] & 2) and (over.size or (g['flags'][lo + 6] & 2)), at
    finally:
        sol.close()


@pytest.mark.parametrize('name', ['pile_in_crowd', 'pile_70'])
def test_closest_approach_beside_a_pile(S, row_env, name):
    """sca_clearance_enable: the records equal an all-pairs search with the reference's rounded norm (tests/clearance_rule.py) and no row has
    the bit (Run.check) -- the descent's stack holds 64, the pile's own rows queue about k - 10.  Under `packed`: K1 keeps 64 too"""
    row_env('packed')
    s = K.scene(name)
    sol = context_of(S, s)
    try:
        run = Run(S, sol, s, S.NBR_KDTREE)
        run.steps(STEPS, name)
        assert np.isfinite(run.rule['agent_clear'][s['flags'] == 0]).all()
    finally:
        sol.close()


def test_a_retired_part_of_the_pile_takes_the_bit_away(S, oracle, row_env):
    """pile_71 with 20 members of the pile retired: the tree holds the occupied rows alone (51 on the point), no walk overflows any more and
    every occupied row equals the oracle on the compacted scene (tests/vacancy_rule.py) -- the default kd forms, whose stack holds 48"""
    row_env('solve_fb')
    s = K.scene('pile_71')
    gone = np.arange(s['n'] - 20, s['n'], dtype=np.int32)
    left = dict(s, n=s['n'] - 20, key=s['key'] + ('retired', 20), **{k: s[k][:-20] for k in ('pos', 'vel', 'flags', 'policy')})
    assert K.bit_rows(s, K.KD_RSTACK).size == 6 and K.bit_rows(left, K.KD_RSTACK).size == 0
    rule, sol = Rule(oracle, s), context_of(S, s)
    try:
        rule.retire(gone)
        sol.retire(gone)
        rule.check_calls(sol, ('retired',))
        for t in range(STEPS):
            sol.run_steps(1, S.NBR_KDTREE)
            sol.synchronize()
            assert sol.pass_forms() & S.FORM_VACANCY
            check_step(sol, rule.step(), s, ('retired', 'step', t))             # (status included: the oracle's words are clear)
    finally:
        sol.close()
