"""What tests/test_gpu_partition_fuzz.py stands on, checked without a GPU: the cut scenes of form_fuzz.cut_scene, their rule-1 oracle runs
and the ownership model of tests/partition_ranks.py.  Nothing here calls the library.

(a) Under the model ownership stays a partition at every step of every scene, every set of cuts passes the model of sca_partition_init's
    check (interior ranks have at least two layers of cells), and no per-agent cut scene is one SCA_NBR_GRID may refuse.
(b) What the corpus holds, counted per leg from the oracle and the model alone (QUANTITIES): conditions on the inputs of the GPU test, not
    measurements of the library.  Every quantity is at least 1 in the plain leg; FLOORS are about half of what the oracle gives.
(c) The model against sca_partition_init's refusals: sets of cuts that leave an interior rank fewer than two layers (REFUSED_CUTS), and for
    the 80 m-box scenes of the first two plain blocks which world in 2 .. 4 the rule without cuts (equal shares) accepts (null_cut_cases:
    tests/test_gpu_partition_fuzz.py asserts the library refuses exactly the others)."""
import numpy as np
import pytest

import clearance_rule
import form_fuzz as F
import partition_ranks as PR

STEPS = 12
K = F.K
OVERFLOW = 32
PER_AGENT_ND = 4.0


def plain_cases():
    """block-major, as the GPU legs run them: (world, axis, seed)"""
    return [(w, a, sd) for w in F.CUT_WORLDS for a in (0, 1, 2) for sd in F.CUT_SEEDS]


def scene_of(leg, case):
    """(scene, cuts, per-agent attributes or None, the largest neighbor_dist) of a case of a leg"""
    w, a, sd = case
    if leg == 'plain':
        s, cuts = F.cut_scene(sd, w, a)
        return s, cuts, None, 10.0
    s, cuts = F.cut_scene(sd, w, a, nd=PER_AGENT_ND)
    pa = F.cut_attributes(sd, s['n'])
    return s, cuts, pa, float(pa[0]['neighbor_dist'].max())


CASES = {'plain': plain_cases(), 'per_agent': list(F.CUT_PER_AGENT)}

QUANTITIES = ('cross_up', 'cross_down', 'cross_and_back', 'cross_at_goal', 'cross_collided', 'collide_other_owner', 'collide_partner_migrates',
              'obstacle_collide_migrant', 'at_goal_as_halo_copy', 'list_other_rank', 'list_other_rank_overflow', 'list_other_rank_lp',
              'immigrant_two_cell_slab', 'rank_empty_at_start', 'rank_becomes_empty', 'rank_gains_first', 'boundary_first_pos',
              'boundary_first_neg', 'boundary_last_pos', 'boundary_last_neg', 'finished_in_edge_layer')
PER_AGENT_NEEDS = ('cross_up', 'cross_down', 'cross_and_back', 'cross_at_goal', 'cross_collided', 'collide_other_owner', 'collide_partner_migrates',
                   'list_other_rank', 'immigrant_two_cell_slab')
# measured (rule-1 oracle, free-running, 12 steps; the model): the 24 plain cut scenes | the 8 per-agent ones
#   cross_up 383 | 41, cross_down 400 | 39, cross_and_back 14 | 2, cross_at_goal 149 | 15, cross_collided 415 | 42, collide_other_owner 621 | 112,
#   collide_partner_migrates 891 | 92, obstacle_collide_migrant 10 | 5, at_goal_as_halo_copy 295 | 30, list_other_rank 10 581 | 653,
#   list_other_rank_overflow 8 719 | 235, list_other_rank_lp 1 567 | 114, immigrant_two_cell_slab 276 | 38, rank_empty_at_start 20 | 3,
#   rank_becomes_empty 11 | 3, rank_gains_first 15 | 3, boundary_first_pos 9 | 4, boundary_first_neg 6 | 5, boundary_last_pos 9 | 4,
#   boundary_last_neg 6 | 5, finished_in_edge_layer 157 | 44; crossings per cut of the plain leg: 34 .. 87 for worlds 3 .. 5, 249 for world 2.
# Floors at about half of that: conditions on the corpus, measured against the oracle and the model only, never against the library.
FLOORS = {
    'plain': dict(cross_up=190, cross_down=200, cross_and_back=7, cross_at_goal=75, cross_collided=200, collide_other_owner=300,
                  collide_partner_migrates=440, obstacle_collide_migrant=5, at_goal_as_halo_copy=150, list_other_rank=5200,
                  list_other_rank_overflow=4300, list_other_rank_lp=780, immigrant_two_cell_slab=138, rank_empty_at_start=10, rank_becomes_empty=5,
                  rank_gains_first=7, boundary_first_pos=4, boundary_first_neg=3, boundary_last_pos=4, boundary_last_neg=3, finished_in_edge_layer=78),
    'per_agent': dict(cross_up=20, cross_down=19, cross_and_back=1, cross_at_goal=7, cross_collided=21, collide_other_owner=56,
                      collide_partner_migrates=46, list_other_rank=320, immigrant_two_cell_slab=19),
}


def _partners(p1, radius, a):
    """the agents whose moved position collides with a's by the env's test (mampenv.py:61-80: l3norm <= the radius sum)"""
    rs = radius[a] + radius
    rough = clearance_rule._unrounded(p1[a][None, :], p1)[0] - rs
    rough[a] = np.inf
    pa = [float(x) for x in p1[a]]
    return [int(b) for b in np.flatnonzero(rough <= 2e-5) if clearance_rule.l3norm(pa, [float(x) for x in p1[b]]) <= float(rs[b])]


def cut_counts(scene, run, M):
    """QUANTITIES of one scene's run under the model M, and the crossings per cut"""
    s, n = scene, scene['n']
    c = dict.fromkeys(QUANTITIES, 0)
    per_cut = np.zeros(max(M.world - 1, 1), np.int64)
    x0 = s['pos'][:, M.axis]
    cell0 = M.cells(s['pos'])
    for k in np.unique(cell0):
        first = PR.first_double_of_cell(int(k), M.inv_cell)
        last = float(np.nextafter(PR.first_double_of_cell(int(k) + 1, M.inv_cell), -np.inf))
        c['boundary_first_pos' if k > 0 else 'boundary_first_neg'] += int(((x0 == first) & (k != 0)).sum())
        c['boundary_last_pos' if k + 1 > 0 else 'boundary_last_neg'] += int(((x0 == last) & (k + 1 != 0)).sum())
    own0 = M.owner(s['pos'])
    done0 = (s['flags'] & 7) != 0
    c['finished_in_edge_layer'] = int(sum((done0 & (own0 == r) & M.edge(s['pos'], r)).sum() for r in range(M.world)))
    held = np.bincount(own0, minlength=M.world)
    c['rank_empty_at_start'] = int((held == 0).sum())
    owners = [own0]
    p0, f0 = s['pos'], s['flags']
    for st in run:
        p1, f1 = st['pos'], st['flags']
        o0, o1 = owners[-1], M.owner(p1)
        assert (np.abs(o1 - o0) <= 1).all()                                    # nobody moves a whole slab in one step
        moved = o1 != o0
        c['cross_up'] += int((o1 > o0).sum())
        c['cross_down'] += int((o1 < o0).sum())
        for a in np.flatnonzero(moved):
            per_cut[min(o0[a], o1[a])] += 1
        gains_goal, gains_coll = ((f1 & 1) != 0) & ((f0 & 1) == 0), ((f1 & 2) != 0) & ((f0 & 2) == 0)
        c['cross_at_goal'] += int((moved & gains_goal).sum())
        c['cross_collided'] += int((moved & gains_coll).sum())
        for a in np.flatnonzero(gains_coll):
            partners = _partners(p1, s['radius'], a)
            c['collide_other_owner'] += int(any(o0[b] != o0[a] for b in partners))
            c['collide_partner_migrates'] += int(bool(partners) and (moved[a] or any(moved[b] for b in partners)))
            if moved[a] and s['m']:
                pa = [float(x) for x in p1[a]]
                c['obstacle_collide_migrant'] += int(any(clearance_rule.l3norm(pa, [float(x) for x in s['obs_pos'][o]]) <= s['radius'][a] + s['obs_radius'][o]
                                                         for o in range(s['m'])))
        copies = np.zeros(n, bool)
        for r in range(M.world):
            copies |= M.halo(p1, r) & (o1 != r)
        c['at_goal_as_halo_copy'] += int((gains_goal & copies).sum())
        valid = st['nbr_valid'].astype(bool)
        agents = (np.arange(K)[None, :] < st['nbr_n'][:, None]) & (st['nbr_kind'] == 0) & valid[:, None]
        other = (agents & (o0[np.where(agents, st['nbr_id'], 0)] != o0[:, None])).any(axis=1)
        c['list_other_rank'] += int(other.sum())
        c['list_other_rank_overflow'] += int((other & ((st['status'] & OVERFLOW) != 0)).sum())
        c['list_other_rank_lp'] += int((other & (s['policy'] == 4)).sum())
        two = np.array([0 < r < M.world - 1 and M.layers(r) == 2 for r in range(M.world)])
        c['immigrant_two_cell_slab'] += int((moved & two[o1]).sum())
        now = np.bincount(o1, minlength=M.world)
        c['rank_becomes_empty'] += int(((held > 0) & (now == 0)).sum())
        c['rank_gains_first'] += int(((held == 0) & (now > 0)).sum())
        held = now
        owners.append(o1)
        p0, f0 = p1, f1
    seq = np.array(owners)
    for a in range(n):
        o = seq[:, a]
        change = np.flatnonzero(o[1:] != o[:-1])
        c['cross_and_back'] += int(len(change) >= 2 and any(o[t2 + 1] == o[t1] for i, t1 in enumerate(change) for t2 in change[i + 1:]))
    return c, per_cut


@pytest.fixture(scope='module')
def survey(oracle):
    """every cut scene of both legs once: the model's checks and the counts"""
    out = {}
    for leg, cases in CASES.items():
        total = dict.fromkeys(QUANTITIES, 0)
        per_cut, bad, seen_empty = {}, [], {w: set() for w in F.CUT_WORLDS}
        for case in cases:
            s, cuts, pa, nd = scene_of(leg, case)
            M = PR.Model(case[0], case[1], cuts, nd)
            if not M.accepted():
                bad.append(('cuts', case))
            if pa is not None and not (nd >= 4.0 and s['radius'].max() <= 1.0):
                bad.append(('the grid may refuse it', case))
            run = F.oracle_run(oracle, s, STEPS, pa, list_rule=1)
            for t, st in enumerate(run):
                own = M.owner(st['pos'])
                if not ((own >= 0) & (own < M.world)).all() or sum(int((own == r).sum()) for r in range(M.world)) != s['n']:
                    bad.append(('partition', case, t))
            c, cut = cut_counts(s, run, M)
            for k, v in c.items():
                total[k] += v
            if c['rank_gains_first']:
                seen_empty[case[0]].add('gains')
            if c['rank_becomes_empty']:
                seen_empty[case[0]].add('loses')
            for i, v in enumerate(cut[:M.world - 1]):
                per_cut[(case[0], i)] = per_cut.get((case[0], i), 0) + int(v)
        print(leg, len(cases), 'scenes', total, 'crossings per (world, cut)', per_cut)
        out[leg] = (total, per_cut, bad, seen_empty)
    return out


def test_ownership_stays_a_partition_and_every_cut_set_is_accepted(survey):
    for leg in CASES:
        assert not survey[leg][2], (leg, survey[leg][2][:5])


@pytest.mark.parametrize('leg', list(CASES))
def test_the_corpus_feeds_the_partition(survey, leg):
    total, per_cut, _, seen_empty = survey[leg]
    need = QUANTITIES if leg == 'plain' else PER_AGENT_NEEDS
    for k in need:
        assert total[k] >= max(1, FLOORS[leg].get(k, 1)), (leg, k, total[k])
    if leg == 'plain':
        for w in F.CUT_WORLDS:
            assert seen_empty[w] == {'gains', 'loses'}, (w, seen_empty[w])        # per world: a rank gains its first agent, a rank loses its last
            for i in range(w - 1):
                assert per_cut[(w, i)] >= 1, ('no crossing of cut', i, 'world', w)
        assert any(M_adjacent(w) for w in F.CUT_WORLDS if w >= 4)


def M_adjacent(world):
    """two interior slabs of exactly two cells side by side, in both variants of the cuts"""
    out = True
    for ks in F._CUT_CELLS[world]:
        two = [ks[r + 1] - ks[r] == 2 for r in range(len(ks) - 1)]
        out = out and any(a and b for a, b in zip(two[:-1], two[1:]))
    return out


def test_every_cut_scene_has_a_two_cell_interior_slab_and_cells_on_both_sides_of_zero():
    for w in (3, 4, 5):
        for ks in F._CUT_CELLS[w]:
            assert any(ks[r + 1] - ks[r] == 2 for r in range(len(ks) - 1)), (w, ks)
    for w in F.CUT_WORLDS:
        assert M_adjacent(w) == (w >= 4), w
    for leg, cases in CASES.items():
        for case in cases:
            s, cuts, pa, nd = scene_of(leg, case)
            cells = PR.cell_of(s['pos'][:, case[1]], PR.inv_cell_of(nd))
            assert s['n'] <= 400 and (s['n'] < 9 or (cells.min() < 0 <= cells.max())), (leg, case)
            assert [int(np.floor(c * PR.inv_cell_of(nd))) for c in cuts] == list(F._CUT_CELLS[case[0]][case[2] % 2]), (leg, case)


# ---- (c) --------------------------------------------------------------------------------------------------------------------------------------
CELL = 1.0 / PR.inv_cell_of(10.0)
# (world, cuts in metres; the cell is a little more than 10 m, so 10.0 lies in cell 0 and -10.0 in cell -1): an interior rank with no layer,
# one between -10.0 and 10.0, with one layer, the same below zero, with one layer between two wide ones
REFUSED_CUTS = ((3, [2.0, 7.0]), (3, [-10.0, 10.0]), (3, [5.0, 15.0]), (3, [-15.0, -5.0]), (4, [-25.0, 5.0, 12.0]), (4, [-5.0, 5.0, 30.0]), (5, [-30.0, -10.0, 10.0, 15.0]))
ACCEPTED_CUTS = ((2, [0.0]), (3, [5.0, 25.0]), (3, [-15.0, 5.0]), (4, [-25.0, -5.0, 15.0]), (5, [-30.0, -10.0, 15.0, 35.0]))


def test_the_model_refuses_cuts_that_leave_an_interior_rank_fewer_than_two_layers():
    for w, cuts in REFUSED_CUTS:
        assert not PR.Model(w, 0, cuts).accepted(), (w, cuts)
    for w, cuts in ACCEPTED_CUTS:
        assert PR.Model(w, 0, cuts).accepted(), (w, cuts)
    assert abs(CELL - 10.0) < 1e-5 and PR.cell_of(CELL, PR.inv_cell_of(10.0)) in (0, 1)


def box_side(seed):
    """the box of form_fuzz.random_scene(seed): its third draw"""
    rng = np.random.default_rng(seed)
    rng.choice([1, 2, 3, 9, 17, 33, 64, 100, 257, 400, 900, 1600])
    rng.choice([0, 0, 1, 5, 30])
    return float(rng.choice([4.0, 10.0, 30.0, 80.0]))


def null_cut_cases():
    """[(seed, world, accepted)] for the 80 m-box scenes of the first two plain blocks and world 2 .. 4: what the rule without cuts (equal
    shares of the agents as they stand, cells_sorted[r * n / world], along axis 0) gives and whether the model accepts it"""
    out = []
    for seed in F.PLAIN_SEEDS[:2 * F.BLOCK]:
        if box_side(seed) != 80.0:
            continue
        s = F.random_scene(seed)
        for w in (2, 3, 4):
            M = PR.Model(w, 0, nd=10.0, cell_cuts=PR.equal_share_cells(s['pos'], w, 0, PR.inv_cell_of(10.0)))
            out.append((seed, w, M.accepted()))
    return out


def test_which_worlds_the_rule_without_cuts_accepts_on_the_80_m_scenes():
    cases = null_cut_cases()
    seeds = sorted({c[0] for c in cases})
    print('80 m scenes', seeds, 'refused', [(sd, w) for sd, w, ok in cases if not ok])
    for sd in seeds:
        assert np.abs(F.random_scene(sd)['pos'][:, :2]).max() <= 80.0 and box_side(sd) == 80.0
    assert len(seeds) >= 4 and all(ok for sd, w, ok in cases if w == 2)           # (two ranks have no interior rank)
    assert any(ok for sd, w, ok in cases if w == 4) and any(not ok for sd, w, ok in cases), cases
