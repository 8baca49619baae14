"""What tests/test_gpu_kd_shapes.py stands on, checked without a GPU.

(a) The model of tests/kd_shapes.py builds the tree the library's host replica builds (sca_kd_build_host): nodes and permutation, on every
    scene of the corpus, the obstacle trees included.
(b) The scenes stand where they were built to stand: the pending counts of the live rows of the piles on both sides of 48 and 64, those of
    K4's fallback walk on both sides of 64, and every legal scene within 47 at each of the steps the GPU test runs.
(c) What the corpus feeds the queries with, counted from the oracle alone: rows whose list is cut inside a run of equal distSq (the
    survivors are then the tree's visit order and nothing else), and rows with an obstacle in the list.
(d) The oracle's lists against an all-pairs numpy search, as sets, on the rows without a tie at the cut -- the oracle has only ever been
    pinned on recorded shapes.
(e) The oracle against the F21 recordings of the reference: lists entry for entry, action rows, state and permutation, free-running."""
import ctypes as C

import numpy as np
import pytest

import edge_corpus as E
import form_fuzz as F
import kd_shapes as K
from golden_util import shape_fixtures, static_inputs

STEPS = 3                                       # what tests/test_gpu_kd_shapes.py runs
PILE_NAMES = tuple('pile_%d' % k for k in K.PILES)
LEGAL = ('pile_in_crowd', 'chain_in_crowd', 'lattice_900', 'slab_600', 'two_clusters', 'lattice_2049')


@pytest.fixture(scope='module')
def L():
    from sca_amd import _lib
    return _lib.lib()                                              # (loads without a GPU: sca_kd_build_host is host code)


def host_tree(L, pos):
    n = len(pos)
    pts = np.ascontiguousarray(pos, np.float64)
    perm, tree = np.arange(n, dtype=np.int32), np.zeros((2 * n - 1, 10))
    assert L.sca_kd_build_host(n, pts.ctypes.data_as(C.POINTER(C.c_double)), perm.ctypes.data_as(C.POINTER(C.c_int32)),
                               tree.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return tree, perm


def reached(tree):
    used, todo = np.zeros(len(tree), bool), [0]
    while todo:
        i = todo.pop()
        used[i] = True
        if tree[i, 1] - tree[i, 0] > K.MAX_LEAF:
            todo += [int(tree[i, 2]), int(tree[i, 3])]
    return used


@pytest.mark.parametrize('name', K.NAMES)
def test_the_model_builds_the_host_replicas_tree(L, name):
    s = K.scene(name)
    for what, pos in (('agents', s['pos']), ('obstacles', s['obs_pos'])):
        if len(pos) == 0:
            continue
        want, want_perm = host_tree(L, pos)
        got, got_perm = K.build(pos)
        assert np.array_equal(got_perm, want_perm), (name, what, 'permutation')
        used = reached(want)
        assert np.array_equal(reached(got), used), (name, what, 'shape')
        assert np.array_equal(got[used], want[used]), (name, what, 'nodes', np.flatnonzero((got[used] != want[used]).any(axis=1))[:8])


def test_the_piles_stand_on_both_sides_of_each_limit():
    """the design values the GPU test relies on.  Rows 0-5 are the live agents; the walk may queue `capacity` subtrees, one more overflows"""
    want = {54: (48, 47), 55: (49, 48), 70: (64, 63), 71: (65, 64)}
    for k, (hi, lo) in want.items():
        s = K.scene('pile_%d' % k)
        p = K.pending_counts(s)
        assert sorted(set(p[:6, 0].tolist())) == [lo, hi] and (p[6:] == -1).all() and (p[:6, 1] == 0).all(), (k, p[:6])
    assert K.bit_rows(K.scene('pile_54'), K.KD_RSTACK).size == 0 and K.bit_rows(K.scene('pile_70'), K.KD_STACK).size == 0
    assert K.bit_rows(K.scene('pile_55'), K.KD_RSTACK).tolist() == [0, 1, 3, 4] and K.bit_rows(K.scene('pile_55'), K.KD_STACK).size == 0
    assert K.bit_rows(K.scene('pile_70'), K.KD_RSTACK).tolist() == [0, 1, 2, 3, 4, 5]
    assert K.bit_rows(K.scene('pile_71'), K.KD_STACK).tolist() == [0, 1, 3, 4] and K.bit_rows(K.scene('pile_71'), K.KD_RSTACK).tolist() == [0, 1, 2, 3, 4, 5]
    for k, cap in ((55, K.KD_RSTACK), (71, K.KD_STACK)):               # the obstacle tree: the six agents around the pile, on both sides of the limit
        s = K.scene('obstacle_pile_%d' % k)
        p = K.pending_counts(s)
        assert p[:, 0].max() <= 10 and p[6:, 1].max() <= 10, (k, p.max(axis=0))
        assert p[:6, 1].min() == cap and p[:6, 1].max() > cap, (k, p[:6, 1])
        assert set(K.bit_rows(s, cap).tolist()) == set(np.flatnonzero(p[:6, 1] > cap).tolist()) and 0 < K.bit_rows(s, cap).size < 6
    assert K.bit_rows(K.scene('obstacle_pile_55'), K.KD_STACK).size == 0
    for k, count in zip(K.TOUCHES, (64, 65)):                         # K4's fallback walk: the touching row (6) alone comes near the pile
        s = K.scene('touch_%d' % k)
        p = K.k4_pending(s)
        assert p[:7].tolist() == [0, 0, 0, 0, 0, 0, count] and (p[7:] == -1).all(), (k, p[:7])
        assert not K.served_rows(s).any()                             # (the policy pass builds no list: every status word is clear behind it)


@pytest.mark.parametrize('name', LEGAL)
def test_the_legal_scenes_stay_within_47(oracle, name):
    s = K.scene(name)
    ref = F.oracle_run(oracle, s, STEPS)
    most = 0
    for t in range(STEPS):
        p = K.pending_counts(s, **K.state_before(s, ref, t))
        most = max(most, int(p.max()))
        assert not ref[t]['status'].any(), (name, t)
    print(name, 'largest pending count', most)
    assert most <= 47, (name, most)
    if name in ('pile_in_crowd', 'chain_in_crowd'):
        assert most >= 44, (name, most)                               # ... and the two crowds come close to the limit


# measured over the first step of every scene but the touch scenes (the oracle's records):
#   rows cut inside a run of equal distSq 1 620, rows with an obstacle in the list 12
FLOORS = dict(cut_inside_a_tie=800, obstacle_in_list=6)


def test_what_the_corpus_feeds_the_queries_with(oracle):
    total = dict.fromkeys(FLOORS, 0)
    for name in K.NAMES:
        s = K.scene(name)
        if name.startswith('touch'):
            continue
        r = F.oracle_run(oracle, s, 1)[0]
        pairs = K.all_pairs_lists(s)
        full = (r['nbr_valid'] != 0) & (r['nbr_n'] == F.K) & ((r['flags_policy'] & 2) == 0)
        cut = sum(1 for i in np.flatnonzero(full) if s['m'] == 0 and pairs[int(i)][1])      # (the 16th and 17th nearest in range tie)
        in_list = np.arange(F.K)[None, :] < r['nbr_n'][:, None]
        obst = int(((r['nbr_kind'] == 1) & in_list).any(axis=1).sum())
        print(name, 'cut inside a tie', cut, 'obstacle in list', obst)
        total['cut_inside_a_tie'] += cut
        total['obstacle_in_list'] += obst
        if name in PILE_NAMES:
            assert cut == 6, name                                     # every live row: the 16 survivors of k equal distances
    print(total)
    for k, floor in FLOORS.items():
        assert total[k] >= floor, (k, total[k], floor)


@pytest.mark.parametrize('name', [n for n in K.NAMES if not n.startswith(('touch', 'obstacle'))])
def test_the_oracles_lists_against_an_all_pairs_search(oracle, name):
    """As sets, where a set is defined without the tree (kd_shapes.all_pairs_lists says why the k nearest are not): a row with at most 16
    agents in range lists exactly those; a row with more has a full list of agents in range."""
    s = K.scene(name)
    r = F.oracle_run(oracle, s, 1)[0]
    pairs = K.all_pairs_lists(s)
    assert set(pairs) == set(np.flatnonzero(r['nbr_valid']).tolist()), name
    exact = overfull = 0
    for i, (near, _) in pairs.items():
        if r['flags_policy'][i] & 2:
            continue                                                  # (a collision inside the pass keeps only the colliding neighbours, agent.py:83-85)
        k = int(r['nbr_n'][i])
        got = r['nbr_id'][i][:k].tolist()
        assert (r['nbr_kind'][i][:k] == 0).all() and len(set(got)) == k, (name, i)
        if len(near) <= F.K:
            assert set(got) == set(near.tolist()), (name, i)
            exact += 1
        else:
            assert k == F.K and set(got) <= set(near.tolist()), (name, i)
            overfull += 1
    print(name, 'rows with the whole set', exact, 'rows with a full list', overfull)
    assert exact + overfull > 0, name
    assert exact > 0 or name not in ('pile_in_crowd', 'chain_in_crowd', 'slab_600'), name          # (the sparse scenes: most rows have the whole set)


def test_the_fixtures_are_the_scenes():
    assert shape_fixtures() == sorted(K.FIXTURES)
    for fx_name, name in K.FIXTURES.items():
        fx, s = E.fixture(fx_name), K.scene(name)
        st = static_inputs(fx)
        assert len(fx['step']) == K.FIXTURE_STEPS
        for key, want in (('pos', s['pos']), ('vel', s['vel']), ('heading', s['heading']), ('flags', s['flags']), ('goal', s['goal'])):
            assert np.array_equal(fx[key][0], want), (fx_name, key)
        for key in ('radius', 'pref_speed', 'policy', 'obs_pos', 'obs_radius'):
            assert np.array_equal(st[key], s[key]), (fx_name, key)
        assert np.array_equal(fx['perm'][0], np.arange(s['n'])) and not st['vpref_mode'].any(), fx_name


@pytest.mark.parametrize('name', sorted(K.FIXTURES))
def test_the_oracle_free_running_equals_the_recording(oracle, name):
    fx = E.fixture(name)
    st = static_inputs(fx)
    n = len(st['radius'])
    p, ve, he, fl, td, perm = fx['pos'][0], fx['vel'][0], fx['heading'][0], fx['flags'][0], fx['total_dist'][0], fx['perm'][0]
    sn = np.zeros(n, np.int32)
    for t in range(len(fx['step'])):
        ctx = (name, t)
        r = oracle.policy_step(p, ve, he, st['radius'], st['pref_speed'], fl, fx['goal'][t], st['policy'], st['zaxis'], np.nan_to_num(fx['vpref'][t]),
                               st['vpref_mode'], perm, st['obs_pos'], st['obs_radius'], nthreads=4)
        valid = fx['nbr_valid'][t].astype(bool)
        assert valid.sum() == 6 if 'obstacle' not in name else valid.sum() == 40, ctx
        assert np.array_equal(r['nbr_valid'].astype(bool), valid), ctx
        for k in ('nbr_n', 'nbr_id', 'nbr_kind', 'nbr_dsq'):
            assert np.array_equal(r[k][valid], fx[k][t][valid]), ctx + (k,)
        assert np.array_equal(r['action'], fx['action'][t]), ctx + ('action',)
        assert not r['status'].any(), ctx
        u = oracle.env_update(p, ve, he, st['radius'], r['flags'], fx['goal'][t], r['action'], td, st['max_run_dist'], sn, st['obs_pos'], st['obs_radius'])
        p, ve, he, fl, td, sn, perm = u['pos'], u['vel'], u['heading'], u['flags'], u['total_dist'], u['step_num'], r['perm']
        for got, key in ((p, 'pos_after'), (ve, 'vel_after'), (he, 'heading_after'), (fl, 'flags_after'), (td, 'total_dist_after'), (perm, 'perm_after')):
            assert np.array_equal(got, fx[key][t]), ctx + ('after', key)


def test_the_touching_row_collides_in_the_oracles_update(oracle):
    """what the K4 test of tests/test_gpu_kd_shapes.py needs of its scenes: the env update flags the touching row (6) and nobody else"""
    for k in K.TOUCHES:
        s = K.scene('touch_%d' % k)
        r = F.oracle_run(oracle, s, 1)[0]
        assert not (r['flags_policy'][:7] & 2).any() and not r['nbr_valid'].any(), k
        assert (r['flags'][:7] & 2).tolist() == [0, 0, 0, 0, 0, 0, 2], (k, r['flags'][:7])
