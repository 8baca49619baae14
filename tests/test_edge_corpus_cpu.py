"""What tests/test_gpu_edge_corpus.py stands on, checked without a GPU.

(a) The degenerate-geometry family (tests/golden/F20_edge_*.npz) holds what it was made for: counted from the recorded rows and the oracle
    alone -- lists with three and more equal distSq, full lists whose 16th and 17th candidate tie, pairs at and inside the combined radius,
    coincident pairs, pairs at exactly distSq == rangeSq, collisions of the env's own test at exactly dis == radius sum, fallback sweeps, LP4 hand-overs, lp1 calls that took
    the parallel branch (the host harness' linearProgram3 over the recorded neighbours, counted in tests/core_harness.cpp), agents more
    than 1e6 m from zero, NaN action rows.  The floors are about half of what the recordings hold: conditions on the inputs, not
    measurements of the library.  Every fixture contributes to at least one of them.
(b) The oracle FREE-RUNNING from a recording's first state equals the recording at every step (only the v_pref of the SCA / RVO3D+Dubins
    rows is the reference tracker's, fed per step).
(c) A scene inside a concatenation (tests/edge_corpus.py::concat, what the GPU test packs into one context) is bit for bit what it is alone,
    on the oracle's side and under the grid's list rule: lists, decisions, action rows, velocities, headings, travelled distance, flags --
    and positions but for the one coordinate the scene was moved along."""
import ctypes as C

import numpy as np
import pytest

import edge_corpus as E
from golden_util import edge_fixtures, static_inputs
from test_core_harness import harness                                                # noqa: F401 (fixture)

# measured (37 fixtures, every recorded step):
#   pair_ties 777, triple_ties 1 105, ties_at_the_cut 760, dist_eq_R 66, dist_lt_R 282, relpos_zero 82, dist_eq_range 480,
#   collisions_at_equality 122, fallback 214, lp4 32, lp1_parallel 43, far_agents 262, nan_action_rows 4
# sqrt_domain 0, and it stays 0: where the oracle would set ST_SQRT_DOMAIN the reference raises (math.sqrt of a negative discriminant,
# scaPolicy.py:159), and a scene the reference raises on is not part of the family (tools/gen_golden.py::edge_scenes lists them).
FLOORS = dict(pair_ties=380, triple_ties=550, ties_at_the_cut=380, dist_eq_R=31, dist_lt_R=140, relpos_zero=41, dist_eq_range=240,
              collisions_at_equality=61, fallback=106, lp4=15, lp1_parallel=21, far_agents=131, nan_action_rows=2)
CAPS = ('sqrt_domain',)


def _lp_parallel(H):
    dp, fp, bp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)

    def count(fx, st, t, i):
        k = int(fx['nbr_n'][t][i])
        if k == 0 or not fx['vel'][t][i].any():
            return 0                                                                 # (the bootstrap branch runs no linear program)
        ids, kinds = fx['nbr_id'][t][i][:k], fx['nbr_kind'][t][i][:k]
        nb_pos = np.array([st['obs_pos'][j] if o else fx['pos'][t][j] for j, o in zip(ids, kinds)], np.float64)
        nb_vel = np.array([np.zeros(3) if o else fx['vel'][t][j] for j, o in zip(ids, kinds)], np.float32)
        nb_rad = np.array([st['obs_radius'][j] if o else st['radius'][j] for j, o in zip(ids, kinds)], np.float64)
        nb_ob = np.ascontiguousarray(kinds, np.uint8)
        par = np.array([10.0, 0.1, 10.0, 1.0])
        pos, vel = np.ascontiguousarray(fx['pos'][t][i]), np.ascontiguousarray(fx['vel'][t][i], np.float32)
        vp = np.ascontiguousarray(fx['vpref'][t][i])
        pf = np.zeros(1, np.int32)
        got = H.core_lp1_parallel_calls(par.ctypes.data_as(dp), pos.ctypes.data_as(dp), vel.ctypes.data_as(fp), float(st['radius'][i]),
                                        vp.ctypes.data_as(dp), k, nb_pos.ctypes.data_as(dp), nb_vel.ctypes.data_as(fp), nb_rad.ctypes.data_as(dp),
                                        nb_ob.ctypes.data_as(bp), pf.ctypes.data_as(ip))
        assert pf[0] == fx['plane_fail'][t][i], ('the counted linearProgram3 is not the recorded one', t, i, pf[0], fx['plane_fail'][t][i])
        return got
    return count


def test_the_family_holds_what_it_is_for(oracle, harness):                          # noqa: F811
    names = edge_fixtures()
    assert len(names) == 37
    total = dict.fromkeys(E.QUANTITIES, 0)
    count = _lp_parallel(harness)
    for name in names:
        c = E.census(name, oracle, count)
        print(name, {k: v for k, v in c.items() if v})
        assert any(c.values()), (name, 'contributes to no counter')
        for k, v in c.items():
            total[k] += v
    print(total)
    for k, floor in FLOORS.items():
        assert total[k] >= floor, (k, total[k], floor)
    for k in CAPS:
        assert total[k] == 0, (k, total[k])


def test_every_scene_is_small(oracle):
    for name in edge_fixtures():
        fx = E.fixture(name)
        assert len(fx['radius']) <= 64 and len(fx['obs_radius']) <= 16, name


@pytest.mark.parametrize('name', [n for n in edge_fixtures() if E.steps_of(n) > 1])
def test_the_oracle_free_running_equals_the_recording(oracle, name):
    fx = E.fixture(name)
    st = static_inputs(fx)
    n = len(st['radius'])
    assert [int(x) for x in fx['step']] == list(range(len(fx['step'])))
    p, ve, he, fl, td, perm = fx['pos'][0], fx['vel'][0], fx['heading'][0], fx['flags'][0], fx['total_dist'][0], fx['perm'][0]
    sn = np.zeros(n, np.int32)
    for t in range(len(fx['step'])):
        ctx = (name, t)
        for got, key in ((p, 'pos'), (ve, 'vel'), (he, 'heading'), (fl, 'flags'), (td, 'total_dist'), (perm, 'perm')):
            assert E.same(got, fx[key][t]), ctx + ('before', key)
        r = oracle.policy_step(p, ve, he, st['radius'], st['pref_speed'], fl, fx['goal'][t], st['policy'], st['zaxis'], np.nan_to_num(fx['vpref'][t]),
                               st['vpref_mode'], perm, st['obs_pos'], st['obs_radius'], nthreads=4)
        assert E.same(r['action'], fx['action'][t]), ctx + ('action',)
        assert not r['status'].any(), ctx
        u = oracle.env_update(p, ve, he, st['radius'], r['flags'], fx['goal'][t], r['action'], td, st['max_run_dist'], sn, st['obs_pos'], st['obs_radius'])
        p, ve, he, fl, td, sn, perm = u['pos'], u['vel'], u['heading'], u['flags'], u['total_dist'], u['step_num'], r['perm']
        for got, key in ((p, 'pos_after'), (ve, 'vel_after'), (he, 'heading_after'), (fl, 'flags_after'), (td, 'total_dist_after'), (perm, 'perm_after')):
            assert E.same(got, fx[key][t]), ctx + ('after', key)


def test_a_scene_in_a_concatenation_is_what_it_is_alone(oracle):
    """Every fixture's first recorded state, packed as tests/test_gpu_edge_corpus.py packs them (groups of at most 600 agents), under list
    rule 1 -- the grid's: ties by id, the nearest kept.  Under the reference's own rule (0) the claim does not hold and cannot: the order of
    equal distances and the survivors of a full list follow the kd-tree's visit order (agent.py:87-99), and the tree of a concatenation is
    another tree (first seen on F20_edge_far1e6_lattice3_mixed).  So the packed contexts carry the grid leg; under the kd-tree every scene
    also runs alone, and a packed context is compared with the oracle's run of the packed scene."""
    for group in E.concat_groups():
        scenes = [E.step_scene(name) for name in group]
        shifts = [E.concat_shift(s, j) for j, s in enumerate(scenes)]
        assert all(sh is not None for sh in shifts), group
        whole, off, ooff = E.concat(scenes, shifts)
        assert whole['n'] <= 600
        r = E.oracle_step(oracle, whole, list_rule=1)
        for j, (name, s) in enumerate(zip(group, scenes)):
            alone = E.oracle_step(oracle, s, list_rule=1)
            rows = slice(int(off[j]), int(off[j + 1]))
            ids = r['nbr_id'][rows] - np.where(r['nbr_id'][rows] >= 0, np.where(r['nbr_kind'][rows] == 1, ooff[j], off[j]), 0)
            live = np.arange(E.K)[None, :] < alone['nbr_n'][:, None]
            assert np.array_equal(r['nbr_n'][rows], alone['nbr_n']) and np.array_equal(r['nbr_valid'][rows], alone['nbr_valid']), name
            assert np.array_equal(np.where(live, ids, -1), np.where(live, alone['nbr_id'], -1)), (name, 'list order')
            assert np.array_equal(np.where(live, r['nbr_dsq'][rows], 0), np.where(live, alone['nbr_dsq'], 0)), name
            for k in ('action', 'diag', 'status', 'vel', 'heading', 'total_dist', 'flags', 'flags_policy'):
                assert E.same(r[k][rows], alone[k]), (name, k)
            moved = shifts[j] != 0                                  # ((x + s) + dx rounds where x + dx did: that coordinate is not compared)
            assert E.same(r['pos'][rows][:, ~moved], alone['pos'][:, ~moved]), (name, 'pos')
