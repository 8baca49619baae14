"""What tests/test_gpu_form_fuzz.py stands on, checked without a GPU.

(a) The corpus feeds the forms: counted from the oracle alone over the first three steps of the fuzz scenes -- enough active ORCA3D-LP agents,
    LP4 hand-overs, obstacle planes, fallback sweeps, full neighbour lists, collisions, agents done from the start, and scene sizes that leave
    the last wavefront of the packed neighbour query with one, two and three agents.  The floors are about half of what the oracle gives
    today: conditions on the inputs, not measurements of the library.
(b) Every row's plan is the row's name: plan_solve / plan_kd_build of sca_forms.h (tests/forms_harness.cpp) under the row's switches, at agent
    counts of the corpus.  Packed K1 and the kd-build shape have no bit in sca_last_pass_forms: for them this is the evidence that the row ran
    what it says.
(c) The path corpus of tests/test_gpu_path_fuzz.py (form_fuzz.random_paths beside the same scenes) feeds the waypoint rule: counted from the
    oracle and tests/path_rule.py alone over six free-running steps -- first takes, passes that pop twice, pops in a later pass because the
    waypoint was reached and because it lies behind, lists that run out, pops under either distance measure, tracked agents whose lists
    advance, rows aimed at a waypoint and zeroed at the goal; every branch of get_trajectory in a first and in a later pass under both
    measures; and no row at which the rule is undefined (the agent on its waypoint: the reference's own int(nan) raises there).  The
    array form of the rule, from which the oracle is fed, equals the per-agent loop on these very inputs."""
import ctypes as C

import numpy as np
import pytest

import form_fuzz as F
import path_rule as R
from test_forms_cpu import H, SPLIT, LP_LANE, SOLVE_FB, ACTION_FB, clean_env, from_env, kd, solve       # noqa: F401 (H, clean_env: fixtures)

STEPS = 3
# measured (oracle, 3 steps): plain seeds 0-119 | per-agent seeds 1000-1059
#   lp_active 12 547 | 4 557, lp4 2 444 | 861, lp_obstacle 1 176 | 205, fallback 9 039 | 2 390, full_lists 40 225 | 825,
#   new_collisions 14 498 | 5 972, done_at_start 3 897 | 1 546; scene sizes n % 4 = 0 / 1 / 2 / 3: 57 / 44 / 13 / 6 | 26 / 28 / 3 / 3
FLOORS = {
    'plain': dict(lp_active=6000, lp4=1000, lp_obstacle=500, fallback=4000, full_lists=20000, new_collisions=5000, done_at_start=1500),
    'per_agent': dict(lp_active=2000, lp4=400, lp_obstacle=100, fallback=1000, full_lists=400, new_collisions=3000, done_at_start=700),
}
RAGGED_FLOORS = {'plain': (5, 5, 5), 'per_agent': (10, 2, 2)}          # scenes with n % 4 = 1, 2, 3


@pytest.mark.parametrize('corpus', ['plain', 'per_agent'])
def test_the_corpus_feeds_the_forms(oracle, corpus):
    seeds = F.PLAIN_SEEDS if corpus == 'plain' else F.PER_AGENT_SEEDS
    total = dict.fromkeys(F.QUANTITIES, 0)
    blocks = [dict.fromkeys(F.QUANTITIES, 0) for _ in range(len(seeds) // F.BLOCK)]
    ragged = [0, 0, 0, 0]
    for i, seed in enumerate(seeds):
        s = F.random_scene(seed)
        run = F.oracle_run(oracle, s, STEPS, F.per_agent_attributes(seed, s['n']) if corpus == 'per_agent' else None)
        for k, v in F.corpus_counts(s, run).items():
            total[k] += v
            blocks[i // F.BLOCK][k] += v
        ragged[s['n'] % 4] += 1
    print(corpus, total, ragged, blocks)
    for k, floor in FLOORS[corpus].items():
        assert total[k] >= floor, (corpus, k, total[k])
    for r, floor in zip((1, 2, 3), RAGGED_FLOORS[corpus]):
        assert ragged[r] >= floor, (corpus, 'n % 4 ==', r, ragged)
    for b, counts in enumerate(blocks):
        for k in F.QUANTITIES:
            assert counts[k] > 0, (corpus, 'block', b, k)


def test_the_variants_and_the_memo(oracle):
    s = F.random_scene(7)
    v = F.no_lp(s)
    assert (s['policy'] == 4).any() and not (v['policy'] == 4).any() and ((v['policy'] == 3) == ((s['policy'] == 3) | (s['policy'] == 4))).all()
    assert all(v[k] is s[k] for k in s if k not in ('policy', 'key')) and v['key'] != s['key']
    a = F.oracle_run(oracle, s, 2)
    assert F.oracle_run(oracle, s, 2)[0] is a[0] and F.oracle_run(oracle, s, 1)[0] is a[0]       # one run per scene and variant
    assert F.oracle_run(oracle, v, 1)[0] is not a[0]
    per = F.per_agent_attributes(1001, F.random_scene(1001)['n'])
    assert not per[2] and not per[1] and F.per_agent_attributes(1002, 5)[2]                       # every third scene: one value per scene
    # ... and the oracle is back on its defaults afterwards: the plain run of a scene is the same before and after a per-agent run
    s2 = F.random_scene(1001)
    F.oracle_run(oracle, s2, 1, per)
    F._RUNS.pop(s['key'] + (False,))
    b = F.oracle_run(oracle, s, 2)
    assert b[0] is not a[0] and all((a[t][k] == b[t][k]).all() for t in range(2) for k in F.STATE_KEYS + ('action', 'diag'))
    sw = F.switch_scene(2047)
    assert sw['n'] == 2047 and sw['m'] == 40 and len(set(sw['policy'])) == 6 and 0.02 < ((sw['flags'] & 7) != 0).mean() < 0.08


def _tun(H, monkeypatch, row, simds=1024):
    for k, v in F.ROWS[row].items():
        monkeypatch.setenv(k, v)
    t = from_env(H, simds)
    return (C.c_int * len(t))(*t.values())


COUNTS = ((1, 0), (1, 1), (3, 1), (9, 2), (257, 40), (1600, 0), (1600, 270))            # (agents, of them ORCA3D-LP) as the corpus has them


@pytest.mark.parametrize('row', list(F.ROWS))
def test_every_rows_plan_is_the_rows_name(H, clean_env, row):
    t = _tun(H, clean_env, row)
    for n, lp in COUNTS:
        if row == 'solve_fb':
            lp = 0                                                                       # the no_lp variant
        p = solve(H, n, lp=lp, lp_total=lp, t=t)
        ctx = (row, n, lp, p)
        assert p['forms'] == (SPLIT * p['split'] | SOLVE_FB * p['solve_fb'] | LP_LANE * p['lp_kernel'] | ACTION_FB * p['action_fb']), ctx
        if row in ('packed', 'large_shard'):
            assert p['packed'] == 1, ctx
        else:
            assert p['packed'] == 0, ctx                                                 # (below 6144 agents: one agent per wavefront)
        if row in ('split', 'large_shard'):
            assert p['split'] == 1 and p['lp_kernel'] == (lp > 0) and not p['lpw'] and not p['solve_fb'], ctx
        if row == 'lp_lane':
            assert p['lp_kernel'] == (lp > 0) and not p['split'] and not p['lpw'], ctx
        if row in ('fallback_launch', 'large_shard'):
            assert not p['solve_fb'] and not p['action_fb'], ctx
        if row == 'large_shard':
            assert p['forms'] == (SPLIT | (LP_LANE if lp else 0)), ctx                   # what a shard above 16 384 agents runs beside the re-plans
        if row == 'solve_fb':
            assert p['solve_fb'] == 1 and p['forms'] == SOLVE_FB, ctx
        if row in ('packed', 'kd_levels'):                                               # the other forms stay the small shard's defaults
            assert p == dict(packed=int(row == 'packed'), split=0, solve_fb=int(lp == 0), lpw=int(lp > 0), lp_kernel=0, action_fb=int(lp > 0),
                             forms=ACTION_FB if lp else SOLVE_FB), ctx
    for n in (1, 3, 256, 257, 400, 900, 1600):
        p = kd(H, n, t=t)
        if row == 'kd_levels':
            assert p['top'] == 0 and p['block'] == 256 and p['wave_max'] <= 256, (n, p)
            assert (p['level_passes'], p['ticket']) == ((1, 1) if n > 256 else (0, 0)), (n, p)
        else:
            assert p['top'] == 1 and not p['level_passes'] and not p['ticket'], (row, n, p)


def test_the_switch_sizes_straddle_the_default_thresholds(H, clean_env):
    t = _tun(H, clean_env, 'solve_fb')
    assert [solve(H, n, t=t)['solve_fb'] for n in F.SWITCH_SIZES[:2]] == [1, 0]
    assert [solve(H, n, lp=n // 6, lp_total=n // 6, t=t)['packed'] for n in F.SWITCH_SIZES[2:]] == [0, 1]


# ---- (c) the path corpus ------------------------------------------------------------------------------------------------------------------------
PATH_STEPS = 6
PATH_CORPUS = {'plain': range(0, 40), 'per_agent': range(1000, 1020)}       # the seeds tests/test_gpu_path_fuzz.py runs
# measured (oracle + rule, 6 steps, lists from default_rng(5000 + seed)): plain seeds 0-39 | per-agent seeds 1000-1019
#   served 56 867 | 13 631, first_takes 9 933 | 2 940, double_pops 3 178 | 997, later_pops_reached 609 | 122, later_pops_behind 539 | 97,
#   steps_with_later_pop 96 of 240 | 35 of 120, exhausted 4 001 | 1 119, orca_pops 3 727 | 1 029, tracked_with_list 8 841 | 2 267,
#   aimed 25 522 | 6 154, aimed_zeroed_at_goal 37 | 24, at_waypoint 0 | 0, non_finite 0 | 0
# The floors are half of that (a numpy release may change Generator.choice); tracked_with_list on the plain seeds is half of 3 624.
PATH_FLOORS = {
    'plain': dict(served=28433, first_takes=4966, double_pops=1589, later_pops_reached=304, later_pops_behind=269, steps_with_later_pop=48,
                  exhausted=2000, orca_pops=1863, tracked_with_list=1812, aimed=12761, aimed_zeroed_at_goal=18),
    'per_agent': dict(served=6815, first_takes=1470, double_pops=498, later_pops_reached=61, later_pops_behind=48, steps_with_later_pop=17,
                      exhausted=559, orca_pops=514, tracked_with_list=1133, aimed=3077, aimed_zeroed_at_goal=12),
}
PATH_CAPS = ('at_waypoint', 'non_finite')                                     # none at all: the rule is undefined there


@pytest.fixture(scope='module')
def path_runs(oracle):
    """the oracle runs with lists of both corpora, made once: [(seed, scene, lists, run)]"""
    out = {}
    for corpus, seeds in PATH_CORPUS.items():
        out[corpus] = []
        for seed in seeds:
            s = F.random_scene(seed)
            paths = F.random_paths(seed, s)
            per = F.per_agent_attributes(seed, s['n']) if corpus == 'per_agent' else None
            out[corpus].append((seed, s, paths, F.oracle_run(oracle, s, PATH_STEPS, per, paths=paths)))
    return out


@pytest.mark.parametrize('corpus', list(PATH_CORPUS))
def test_the_path_corpus_feeds_the_rule(path_runs, corpus):
    total = dict.fromkeys(F.PATH_QUANTITIES + F.BRANCHES, 0)
    for seed, s, paths, run in path_runs[corpus]:
        counts = F.corpus_counts(s, run)
        for k in total:
            total[k] += counts[k]
    print(corpus, total)
    for k, floor in PATH_FLOORS[corpus].items():
        assert total[k] >= floor, (corpus, k, total[k], floor)
    for k in PATH_CAPS:
        assert total[k] == 0, (corpus, k, total[k])
    for k in F.BRANCHES:
        assert total[k] > 0, (corpus, 'a branch of get_trajectory the corpus never takes', k)


def test_lists_leave_the_scenes_and_the_plain_runs_alone(oracle):
    s = F.random_scene(7)
    before = {k: np.copy(v) for k, v in s.items() if isinstance(v, np.ndarray)}
    paths = F.random_paths(7, s)
    assert all(np.array_equal(F.random_scene(7)[k], v) and np.array_equal(s[k], v) for k, v in before.items())
    assert paths == F.random_paths(7, s) and len(paths) == s['n'] and {len(p) for p in paths} <= {0, 1, 2, 3, 5}
    assert all(w == [round(x, 3) for x in w] for p in paths for w in p)
    plain = F.oracle_run(oracle, s, 2)
    with_lists = F.oracle_run(oracle, s, 2, paths=paths)
    assert with_lists[0] is not plain[0] and 'path_left' in with_lists[0] and 'path_left' not in plain[0]
    assert F.oracle_run(oracle, s, 2, paths=paths)[0] is with_lists[0] and F.oracle_run(oracle, s, 1)[0] is plain[0]       # one run per variant
    # the fed rows of the run with lists: the rule's on the rows it aims, the scene's on the tracked rows
    st = with_lists[0]
    aimed, tracked = st['path_mode'].astype(bool), s['vmode'].astype(bool) & ((st['before'] & 7) == 0)
    assert aimed.any() and tracked.any() and not (aimed & s['vmode'].astype(bool)).any()
    assert np.array_equal(st['path_left_before'], [len(p) for p in paths]) and np.isnan(st['now_goal_before']).all()


def test_the_two_forms_of_the_rule_agree_on_the_corpus(path_runs):
    """pass_rule_csr (what oracle_run feeds the oracle from) against the per-agent pass_rule, from the state every step of every corpus scene
    of at most 400 agents started from"""
    compared = 0
    for corpus in PATH_CORPUS:
        for seed, s, paths, run in path_runs[corpus]:
            if s['n'] > 400:
                continue
            off, pts = R.csr(paths)
            given = np.diff(off) > 0
            for t, st in enumerate(run):
                lists = R.lists_from_csr(off, pts, st['path_left_before'])
                ng = st['now_goal_before'].copy()
                vp, mode = R.pass_rule(lists, ng, st['pos_before'], s['goal'], s['radius'], s['pref_speed'], s['policy'], st['before'], given)
                ctx = (corpus, seed, t)
                assert np.array_equal(st['path_left'], [len(p) for p in lists]), ctx
                assert np.array_equal(st['now_goal'], ng, equal_nan=True), ctx
                assert np.array_equal(st['path_mode'], mode) and st['vpref_rule'].tobytes() == vp.tobytes(), ctx       # (bytes: -0.0 is not 0.0)
                compared += int(mode.sum())
    assert compared > 2000, compared
