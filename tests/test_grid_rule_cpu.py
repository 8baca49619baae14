"""What tests/test_gpu_grid_fuzz.py stands on, checked without a GPU: the oracle's list rule 1 (oracle.set_list_rule), the restatement of the
list SCA_NBR_GRID documents -- sorted by (distSq, obstacles first, agent id), the nearest max_neighbors kept, status bit 32 where more objects
were admitted than the list holds.

(a) Rule 1 against rule 0 (the reference's lists, pinned by the golden suite) on all 180 fuzz scenes, three steps, each pass from the state of
    the rule-0 run: the same agents get a list, the same agents collide, every list has the same length; where rule 1 reports no overflow the
    two lists hold the same entries; where in addition no two entries share a distSq they are the same list, and the action row and the
    decision's diagnostics are the same.  (A row that overflowed is left out of the last two on purpose: there rule 0 keeps what the kd visit
    order left, which is the difference between the rules.)
(b) "The nearest", stated independently: the lists at max_neighbors 4 are the first four entries of the lists at 16 from the same state, with
    the overflow bit that follows from the longer list; and on the scenes without obstacles the lists are what numpy finds over all pairs
    (test_gpu_grid.brute_lists, with the collision rule).
(c) What the corpus feeds the grid, counted from the free-running rule-1 oracle: overflowing rows with and without a collision, of ORCA3D-LP
    agents, with obstacles in the list, at max_neighbors below 16, and lists with two equal distances.  Floors at about half of what the oracle
    gives: conditions on the inputs, not measurements of the library.
(d) Which per-agent scenes SCA_NBR_GRID may refuse, from the corpus's own attributes.
(e) Rule 1 in a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer (tests/grid_rule_asan.c)."""
import math
import os
import subprocess

import numpy as np
import pytest

import form_fuzz as F
from test_gpu_grid import brute_lists, canonical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 3
K = F.K
OVERFLOW = 32
# the per-agent seeds whose largest neighbor_dist is below 4.0: radius + collision reach does not fit into a cell, SCA_NBR_GRID says so
GRID_MAY_REFUSE = (1014, 1023, 1041, 1047, 1053, 1056, 1059)
CORPORA = {'plain': F.PLAIN_SEEDS, 'per_agent': F.PER_AGENT_SEEDS}


def attributes(corpus, seed, n):
    return F.per_agent_attributes(seed, n) if corpus == 'per_agent' else None


def max_neighbors_of(per_agent, n):
    """max_neighbors of every agent of a scene (per_agent: what per_agent_attributes returned, or None)"""
    if per_agent is None:
        return np.full(n, 16, np.int32)
    per, params, uniform = per_agent
    return np.full(n, params['max_neighbors'], np.int32) if uniform else per['max_neighbors']


def range_sq_of(per_agent, n):
    if per_agent is None:
        return np.full(n, 100.0)
    per, params, uniform = per_agent
    nd = np.full(n, params['neighbor_dist']) if uniform else per['neighbor_dist']
    return np.array([math.pow(x, 2.0) for x in nd])                                   # scaPolicy.py:112


def states_of(scene, run):
    """the state every step of an oracle run started from: (pos, vel, heading, flags, perm)"""
    out = [(scene['pos'], scene['vel'], scene['heading'], scene['flags'], np.arange(scene['n'], dtype=np.int32))]
    for st in run[:-1]:
        out.append((st['pos'], st['vel'], st['heading'], st['flags'], st['perm']))
    return out


def one_pass(oracle, scene, state, per_agent, list_rule, max_neighbors=None):
    """one policy pass from `state` under a list rule; max_neighbors: that value for every agent instead of the scene's own"""
    s, n = scene, scene['n']
    p, ve, he, fl, perm = state
    try:
        oracle.set_list_rule(list_rule)
        params, per = {}, None
        if per_agent is not None:
            per, params, uniform = per_agent
            params, per = dict(params), (None if uniform else dict(per))
        if max_neighbors is not None:
            params['max_neighbors'] = max_neighbors
            if per is not None:
                per['max_neighbors'] = np.full(n, max_neighbors, np.int32)
        oracle.set_params(**params)
        if per is not None:
            oracle.set_agent_params(n, **per)
        return oracle.policy_step(p, ve, he, s['radius'], s['pref_speed'], fl, s['goal'], s['policy'], F.zaxis_of(s), s['vpref'], s['vmode'], perm,
                                  s['obs_pos'], s['obs_radius'], nthreads=8)
    finally:
        oracle.set_params()
        oracle.set_agent_params()
        oracle.set_list_rule(0)


def live(r):
    return np.arange(K)[None, :] < r['nbr_n'][:, None]


def tied(r):
    """rows with two entries of one distSq in their list (a sorted list: two neighbours in it)"""
    lv = live(r)
    return ((r['nbr_dsq'][:, 1:] == r['nbr_dsq'][:, :-1]) & lv[:, 1:]).any(axis=1)


@pytest.fixture(scope='module')
def survey(oracle):
    """Every scene of both corpora once: the rule-0 run, the rule-1 passes from its states at the scene's max_neighbors, at 16 and at 4, and the
    all-pairs lists where the scene has no obstacles.  What does not hold is collected per check (the tests below assert the lists empty), with
    how many rows each check saw."""
    bad = {k: [] for k in ('valid', 'collision', 'length', 'entries', 'same_list', 'action', 'diag', 'prefix', 'overflow4', 'brute', 'full')}
    seen = dict.fromkeys(('rows', 'no_overflow', 'no_tie', 'prefix', 'brute', 'brute_collide', 'brute_overflow'), 0)
    for corpus, seeds in CORPORA.items():
        for seed in seeds:
            s = F.random_scene(seed)
            n = s['n']
            pa = attributes(corpus, seed, n)
            maxn = max_neighbors_of(pa, n)
            run0 = F.oracle_run(oracle, s, STEPS, pa)
            for t, state in enumerate(states_of(s, run0)):
                at = (corpus, seed, t)
                r0 = run0[t]
                r1 = one_pass(oracle, s, state, pa, 1)
                valid = r0['nbr_valid'].astype(bool)
                over = (r1['status'] & OVERFLOW) != 0
                seen['rows'] += int(valid.sum())
                if not np.array_equal(r1['nbr_valid'], r0['nbr_valid']):
                    bad['valid'].append(at)
                if not np.array_equal(r1['flags'], r0['flags_policy']):
                    bad['collision'].append(at)
                if not np.array_equal(r1['nbr_n'][valid], r0['nbr_n'][valid]) or (over & ~valid).any():
                    bad['length'].append(at)
                if not np.array_equal(r1['nbr_n'][over], maxn[over]):                  # an overflowed list is a full list
                    bad['full'].append(at)
                rows = valid & ~over
                seen['no_overflow'] += int(rows.sum())
                c1 = canonical(r1['nbr_n'], r1['nbr_id'], r1['nbr_kind'], r1['nbr_dsq'])
                c0 = canonical(r0['nbr_n'], r0['nbr_id'], r0['nbr_kind'], r0['nbr_dsq'])
                if not all(np.array_equal(a[rows], b[rows]) for a, b in zip(c1, c0)):
                    bad['entries'].append(at)
                plain = rows & ~tied(r1)
                seen['no_tie'] += int(plain.sum())
                lv = live(r1)
                if not all(np.array_equal(np.where(lv, r1[k], 0)[plain], np.where(lv, r0[k], 0)[plain]) for k in ('nbr_id', 'nbr_kind', 'nbr_dsq')):
                    bad['same_list'].append(at)
                same = plain | ~valid                                                  # (without a list there is nothing a rule could change)
                if not np.array_equal(r1['action'][same], r0['action'][same]):
                    bad['action'].append(at)
                if not np.array_equal(r1['diag'][same], r0['diag'][same]):
                    bad['diag'].append(at)
                # ---- (b) max_neighbors 4 against 16, both by rule 1 from this state
                r16 = r1 if corpus == 'plain' else one_pass(oracle, s, state, pa, 1, max_neighbors=16)
                r4 = one_pass(oracle, s, state, pa, 1, max_neighbors=4)
                head = np.arange(K)[None, :] < np.minimum(r16['nbr_n'], 4)[:, None]
                ok = np.array_equal(r4['nbr_n'], np.minimum(r16['nbr_n'], 4)) and np.array_equal(r4['nbr_valid'], r16['nbr_valid'])
                ok = ok and all(np.array_equal(np.where(head, r4[k], 0), np.where(head, r16[k], 0)) for k in ('nbr_id', 'nbr_kind', 'nbr_dsq'))
                if not ok:
                    bad['prefix'].append(at)
                if not np.array_equal((r4['status'] & OVERFLOW) != 0, (r16['nbr_n'] > 4) | ((r16['status'] & OVERFLOW) != 0)):
                    bad['overflow4'].append(at)
                seen['prefix'] += int((valid & (r16['nbr_n'] > 4)).sum())
                # ---- (b) all pairs in numpy, where there is no obstacle
                if s['m'] == 0:
                    rows_v = np.flatnonzero(valid)
                    ref = brute_lists(state[0], s['radius'], rows_v, range_sq_of(pa, n), collide=True)
                    for i in rows_v:
                        order, dsq = ref[i]
                        k = min(int(maxn[i]), len(order))
                        if (bool(over[i]) != (len(order) > maxn[i]) or r1['nbr_n'][i] != k or not np.array_equal(r1['nbr_id'][i, :k], order[:k])
                                or not np.array_equal(r1['nbr_dsq'][i, :k], dsq[:k]) or r1['nbr_kind'][i, :k].any()):
                            bad['brute'].append(at + (int(i),))
                        seen['brute'] += 1
                        seen['brute_overflow'] += int(over[i])
                        seen['brute_collide'] += int((r1['flags'][i] & 2) != 0)
    print('survey', seen, {k: len(v) for k, v in bad.items()})
    return bad, seen


def test_rule_1_lists_the_agents_rule_0_lists_and_finds_the_same_collisions(survey):
    bad, seen = survey
    assert not bad['valid'] and not bad['collision'], (bad['valid'][:5], bad['collision'][:5])
    assert not bad['length'] and not bad['full'], (bad['length'][:5], bad['full'][:5])
    assert seen['rows'] > 50000, seen                                   # (three steps of ~44 000 agents, a part of them done or on the bootstrap step)


def test_rule_1_holds_rule_0s_entries_where_nothing_overflowed(survey):
    bad, seen = survey
    assert not bad['entries'], bad['entries'][:5]
    assert seen['no_overflow'] > 20000, seen


def test_rule_1_is_rule_0_where_no_distance_comes_twice(survey):
    bad, seen = survey
    assert not bad['same_list'] and not bad['action'] and not bad['diag'], (bad['same_list'][:5], bad['action'][:5], bad['diag'][:5])
    assert seen['no_tie'] > 20000, seen


def test_a_short_list_is_the_head_of_the_long_one(survey):
    bad, seen = survey
    assert not bad['prefix'] and not bad['overflow4'], (bad['prefix'][:5], bad['overflow4'][:5])
    assert seen['prefix'] > 20000, seen                                 # rows where four entries are fewer than the list at 16 holds


def test_rule_1_against_all_pairs_in_numpy(survey):
    bad, seen = survey
    assert not bad['brute'], bad['brute'][:5]
    assert seen['brute'] > 10000 and seen['brute_overflow'] > 2000 and seen['brute_collide'] > 1000, seen


# ---- (c) --------------------------------------------------------------------------------------------------------------------------------------
QUANTITIES = ('listed', 'overflow_free', 'overflow_collided', 'overflow_lp', 'overflow_obstacle', 'overflow_small_list', 'equal_distances')
# measured (rule-1 oracle, free-running, 3 steps): plain seeds 0-119 | the 53 per-agent seeds of 1000-1059 that the grid takes
#   listed 72 373 | 24 202, overflow_free 35 545 | 8 780, overflow_collided 4 027 | 1 604, overflow_lp 6 954 | 1 832, overflow_obstacle 4 979 | 496,
#   overflow_small_list 0 | 9 575, equal_distances 6 | 1.  Per block of 20 plain seeds everything is above zero but overflow_collided (block 2: 0;
#   block 3: 28) and equal_distances (blocks 2, 4, 5: 0): random coordinates hardly ever give one rounded distSq twice -- the lists with many equal
#   distances are those of the take-off lattice in tests/test_gpu_grid_fuzz.py.
FLOORS = {
    'plain': dict(listed=36000, overflow_free=17000, overflow_collided=2000, overflow_lp=3400, overflow_obstacle=2400, equal_distances=3),
    'per_agent': dict(listed=12000, overflow_free=4300, overflow_collided=800, overflow_lp=900, overflow_obstacle=240, overflow_small_list=4700),
}
EVERY_BLOCK = ('listed', 'overflow_free', 'overflow_lp', 'overflow_obstacle')


def grid_counts(scene, run, maxn):
    c = dict.fromkeys(QUANTITIES, 0)
    for st in run:
        valid = st['nbr_valid'].astype(bool)
        over = valid & ((st['status'] & OVERFLOW) != 0)
        collided = (st['flags_policy'] & 2) != 0                                       # (a row with a list was active: the pass raised it)
        in_list = live(st)
        c['listed'] += int(valid.sum())
        c['overflow_free'] += int((over & ~collided).sum())
        c['overflow_collided'] += int((over & collided).sum())
        c['overflow_lp'] += int((over & (scene['policy'] == 4)).sum())
        c['overflow_obstacle'] += int((over & ((st['nbr_kind'] == 1) & in_list).any(axis=1)).sum())
        c['overflow_small_list'] += int((over & (maxn < 16)).sum())
        c['equal_distances'] += int((valid & tied(st)).sum())
    return c


@pytest.mark.parametrize('corpus', list(CORPORA))
def test_the_corpus_feeds_the_grid(oracle, corpus):
    seeds = [sd for sd in CORPORA[corpus] if sd not in GRID_MAY_REFUSE]
    total = dict.fromkeys(QUANTITIES, 0)
    blocks = [dict.fromkeys(QUANTITIES, 0) for _ in range(len(CORPORA[corpus]) // F.BLOCK)]
    for seed in seeds:
        s = F.random_scene(seed)
        pa = attributes(corpus, seed, s['n'])
        run = F.oracle_run(oracle, s, STEPS, pa, list_rule=1)
        for k, v in grid_counts(s, run, max_neighbors_of(pa, s['n'])).items():
            total[k] += v
            blocks[(seed - CORPORA[corpus][0]) // F.BLOCK][k] += v
    print(corpus, len(seeds), 'scenes', total, blocks)
    for k, floor in FLOORS[corpus].items():
        assert total[k] >= floor, (corpus, k, total[k])
    if corpus == 'plain':
        for b, counts in enumerate(blocks):
            for k in EVERY_BLOCK:
                assert counts[k] > 0, (corpus, 'block', b, k)
    else:
        assert len(seeds) == 53


def test_the_rule_is_part_of_the_memo_and_is_restored(oracle):
    s = F.random_scene(7)
    a = F.oracle_run(oracle, s, 1)
    b = F.oracle_run(oracle, s, 1, list_rule=1)
    assert b[0] is not a[0] and F.oracle_run(oracle, s, 1, list_rule=1)[0] is b[0] and F.oracle_run(oracle, s, 1)[0] is a[0]
    assert (b[0]['status'] & OVERFLOW).any() and not (a[0]['status'] & OVERFLOW).any()
    F._RUNS.pop(s['key'] + (False,))
    c = F.oracle_run(oracle, s, 1)                                       # after a rule-1 run the oracle is back on rule 0
    assert c[0] is not a[0] and all(np.array_equal(a[0][k], c[0][k]) for k in ('nbr_n', 'nbr_id', 'nbr_dsq', 'action', 'status'))
    with pytest.raises(ValueError):
        oracle.set_list_rule(2)


# ---- (d) --------------------------------------------------------------------------------------------------------------------------------------
def test_the_scenes_the_grid_may_refuse():
    """the largest neighbor_dist of the scene is the grid's cell; below 4.0 it cannot hold the collision check's partners (the largest radius
    of the corpus is 1.0).  All seven are `uniform` scenes with 1.5 or 2.5."""
    small = []
    for seed in F.PER_AGENT_SEEDS:
        per, params, uniform = F.per_agent_attributes(seed, F.random_scene(seed)['n'])
        largest = params['neighbor_dist'] if uniform else float(per['neighbor_dist'].max())
        if largest < 4.0:
            assert uniform and largest in (1.5, 2.5), (seed, largest)
            small.append(seed)
    assert tuple(small) == GRID_MAY_REFUSE


# ---- (e) --------------------------------------------------------------------------------------------------------------------------------------
SANITIZER_SCENES = (('plain', 100), ('per_agent', 1045))    # dense with obstacles | max_neighbors per agent, with obstacles


def _checksum(arrays):
    b = np.concatenate([np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8) for a in arrays]).astype(np.uint64)
    at = np.arange(len(b), dtype=np.uint64)
    with np.errstate(over='ignore'):
        return int(((b + np.uint64(1)) * (at * np.uint64(2654435761) + np.uint64(1))).sum(dtype=np.uint64))


def _dump(path, s, per_agent):
    n = s['n']
    per, params, uniform = per_agent if per_agent is not None else (None, {}, True)
    p = dict(F_DEFAULTS, **params)
    with open(path, 'wb') as f:
        f.write(np.array([n, s['m'], 0 if uniform else 1], np.int32).tobytes())
        for a, dt in ((s['pos'], np.float64), (s['vel'], np.float32), (s['heading'], np.float64), (s['radius'], np.float64), (s['pref_speed'], np.float64),
                      (s['flags'], np.uint8), (s['goal'], np.float64), (s['policy'], np.uint8), (F.zaxis_of(s), np.uint8), (s['vpref'], np.float64),
                      (s['vmode'], np.uint8), (s['obs_pos'], np.float64), (s['obs_radius'], np.float64)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
        f.write(np.array([p[k] for k in ('neighbor_dist', 'max_neighbors', 'time_step', 'time_horizon', 'max_speed', 'max_heading_change',
                                         'near_goal_threshold', 'dt_nominal')], np.float64).tobytes())
        if not uniform:
            for k in ('neighbor_dist', 'max_neighbors', 'time_step', 'time_horizon', 'max_speed', 'max_heading_change', 'dt_nominal'):
                f.write(np.ascontiguousarray(per[k], np.int32 if k == 'max_neighbors' else np.float64).tobytes())


F_DEFAULTS = dict(neighbor_dist=10.0, max_neighbors=16, time_step=0.1, time_horizon=10.0, max_speed=1.0, max_heading_change=math.pi / 4,
                  near_goal_threshold=0.5, dt_nominal=0.1)              # agent.py:27-41 / config.py:3, as oracle.DEFAULT_PARAMS


def test_rule_1_in_a_program_of_its_own_under_asan_and_ubsan(oracle, tmp_path):
    """tests/grid_rule_asan.c + oracle/sca_oracle.c, -fsanitize=address,undefined: one pass by rule 1 over two scenes dumped as raw arrays -- a
    dense one with obstacles and one with max_neighbors per agent --, no report, and the checksum of lists, action rows, diagnostics, status
    words, flags and permutation is the one of the same pass through liboracle.so"""
    probe = subprocess.run(['gcc', '-print-file-name=libasan.so'], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(probe) and os.path.exists(probe)):
        pytest.skip('libasan.so not found')
    assert F_DEFAULTS == oracle.DEFAULT_PARAMS
    build = os.path.join(ROOT, 'tests', '_build')
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, 'grid_rule_asan')
    subprocess.check_call(['gcc', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-ffp-contract=off', '-fno-fast-math', '-fno-builtin-pow', '-fno-builtin-powf', '-o', exe,
                           os.path.join(ROOT, 'tests', 'grid_rule_asan.c'), os.path.join(ROOT, 'oracle', 'sca_oracle.c'), '-lm'])
    files, want = [], []
    for corpus, seed in SANITIZER_SCENES:
        s = F.random_scene(seed)
        pa = attributes(corpus, seed, s['n'])
        r = one_pass(oracle, s, states_of(s, [None])[0], pa, 1)
        over = (r['status'] & OVERFLOW) != 0
        assert s['m'] > 0 and over.sum() > 20 and (over & ((r['flags'] & 2) != 0)).any() and ((r['nbr_kind'] == 1) & live(r)).any(), (corpus, seed)
        if corpus == 'per_agent':
            assert not pa[2] and (over & (pa[0]['max_neighbors'] < 16)).any(), seed
        files.append(str(tmp_path / ('scene_%d.bin' % seed)))
        _dump(files[-1], s, pa)
        want.append('checksum %016x' % _checksum([r[k] for k in ('nbr_valid', 'nbr_n', 'nbr_id', 'nbr_kind', 'nbr_dsq', 'action', 'diag', 'status',
                                                                 'flags', 'perm')]))
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1'))
    out = run.stdout[-2000:] + '\n' + run.stderr[-6000:]
    assert run.returncode == 0 and 'AddressSanitizer' not in out and 'runtime error' not in out, out
    assert run.stdout.split('\n')[:2] == want, (run.stdout, want)
