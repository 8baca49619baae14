"""What tests/test_gpu_form_fuzz.py stands on, checked without a GPU.

(a) The corpus feeds the forms: counted from the oracle alone over the first three steps of the fuzz scenes -- enough active ORCA3D-LP agents,
    LP4 hand-overs, obstacle planes, fallback sweeps, full neighbour lists, collisions, agents done from the start, and scene sizes that leave
    the last wavefront of the packed neighbour query with one, two and three agents.  The floors are about half of what the oracle gives
    today: conditions on the inputs, not measurements of the library.
(b) Every row's plan is the row's name: plan_solve / plan_kd_build of sca_forms.h (tests/forms_harness.cpp) under the row's switches, at agent
    counts of the corpus.  Packed K1 and the kd-build shape have no bit in sca_last_pass_forms: for them this is the evidence that the row ran
    what it says."""
import ctypes as C

import pytest

import form_fuzz as F
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
