"""Spawn admission on the GPU (-m gpu): sca_probe_clearance against the Python rule of tests/spawn_rule.py over the positions THE DEVICE
ITSELF reports, and sca_respawn_agents_gated against that rule, against a twin context that plainly respawns the admitted subset (word
for word) and against the gated oracle run (spawn_rule.oracle_run_gated).  Equality, no tolerance; nothing expected comes from the code
under test."""
import ctypes as C
import math

import numpy as np
import pytest

import clearance_rule as CR
import clearance_scenes as CS
import edge_corpus as E
import form_fuzz as F
import respawn_rule as RR
import spawn_rule as SR
from test_gpu_form_fuzz import check_paths, compare_with_oracle, context_of
from test_gpu_respawn import mission_for, respawn, snapshot

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5
P = 512                                                                     # SPAWN_TILE (tests/test_spawn_probe_cpu.py reads it off the harness)
COUNTS = (1, 63, 64, 65, 257)


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


def differ(got, want):
    bad = np.zeros(len(want), bool)
    for f in want.dtype.names:
        bad |= E.differ(got[f], want[f])
    return np.flatnonzero(bad)


def mode_of(S, name):
    return {'kd': S.NBR_KDTREE, 'auto': S.NBR_AUTO, 'host': S.NBR_KDTREE_HOSTBUILD, 'grid': S.NBR_GRID}[name]


def probe_check(sol, radius, scene, qpos, qrad, ignore, what, ties=None):
    """the device's probe against the rule over the positions the device reports"""
    pos = sol.get_state()['pos']
    got = sol.probe_clearance(qpos, qrad, ignore)
    want = SR.probe(qpos, qrad, ignore, pos, np.asarray(radius, np.float64), scene['obs_pos'], scene['obs_radius'], ties=ties)
    bad = differ(got, want)
    assert bad.size == 0, (what, bad[:8].tolist(), got[bad[:3]], want[bad[:3]])
    assert not got['agent_step'].any() and not got['obs_step'].any()
    return got


def probe_all_counts(sol, scene, rng, what):
    """query counts 1, 63, 64, 65 and 257: agents' own positions (ignore = self), random points, points exactly on agents"""
    n = scene['n']
    pos = sol.get_state()['pos']
    lo, hi = pos.min(axis=0) - 1.0, pos.max(axis=0) + 1.0
    for count in COUNTS:
        own = rng.integers(0, n, count).astype(np.int32)
        got = probe_check(sol, scene['radius'], scene, pos[own], scene['radius'][own], own, what + ('own', count))
        assert (got['agent_partner'] != own).all()
        assert np.isfinite(got['agent_clear']).all() == (n > 1) and np.isfinite(got['obs_clear']).all() == (scene['m'] > 0), what
        probe_check(sol, scene['radius'], scene, rng.uniform(lo, hi, (count, 3)), rng.choice([0.0, 0.3, 1.0], count), None, what + ('random', count))
        got = probe_check(sol, scene['radius'], scene, pos[own], np.full(count, 0.5), np.full(count, -1, np.int32), what + ('on agents', count))
        assert (got['agent_clear'] <= 0.0 - (0.5 + scene['radius'][own])).all()


# ---- the probe against the Python rule ---------------------------------------------------------------------------------------------------
SIZED = [(1, 0, 'kd'), (2, 1, 'kd'), (P - 1, 23, 'kd'), (P, 0, 'auto'), (P + 1, 23, 'host'), (2 * P + 1, 1, 'auto'), (2049, 23, 'kd'), (6145, 23, 'auto')]


@pytest.mark.parametrize('n,m,mode', SIZED)
def test_probe_sizes_and_modes(S, n, m, mode):
    """either side of a tile, more tiles than one, the first form switches; before the first step and after three"""
    scene = CS.sized_scene(n, m)
    rng = np.random.default_rng(n + m)
    sol = context_of(S, scene)
    try:
        probe_all_counts(sol, scene, rng, (n, m, mode, 'before'))
        for _ in range(3):
            sol.env_step(mode_of(S, mode))
        probe_all_counts(sol, scene, rng, (n, m, mode, 'after 3'))
    finally:
        sol.close()


def test_probe_more_queries_than_one_launch_takes(S):
    """a call's queries go through the kernels in batches of 4096 behind its one synchronisation: 4095, 4096, 4097 and 8193 queries, and a
    gated call naming 6145 rows (the gate walks all of them in one launch)"""
    scene = CS.sized_scene(6145, 23)
    n = scene['n']
    sol = context_of(S, scene)
    try:
        sol.env_step(S.NBR_AUTO)
        pos = sol.get_state()['pos']
        rng = np.random.default_rng(8)
        for count in (4095, 4096, 4097, 8193):
            own = rng.integers(0, n, count).astype(np.int32)
            probe_check(sol, scene['radius'], scene, pos[own] + rng.normal(0, 0.3, (count, 3)), scene['radius'][own], own, ('batches', count))
        m = mission_for(scene, np.arange(n, dtype=np.int32), 3)
        m['pos'][::2] = m['pos'][::2] + np.array([400.0, 0.0, 0.0])          # every other row far outside the swarm, where only rows of the call are
        want_v, want_rec = SR.gate(m['ids'], m['pos'], m['radius'], SR.MARGIN, pos, scene['radius'], scene['obs_pos'], scene['obs_radius'])
        v, rec = sol.respawn(m['ids'], m['pos'], m['vel'], m['heading'], m['radius'], m['pref_speed'], m['goal'], m['max_run_dist'], margin=SR.MARGIN)
        assert np.array_equal(v, want_v) and differ(rec, want_rec).size == 0
        assert all((v == k).sum() > 20 for k in (SR.ADMITTED, SR.BLOCKED_AGENT, SR.BLOCKED_ENTRY)), np.bincount(v)
        got = sol.get_state()['pos']
        assert np.array_equal(got[v == 0], m['pos'][v == 0]) and np.array_equal(got[v != 0], pos[v != 0])
    finally:
        sol.close()


def test_probe_among_the_1491_spheres_of_the_exp3_map(S):
    scene = E.step_scene('F10_sca_exp3_map', 0)
    assert scene['m'] == 1491
    sol = context_of(S, scene)
    try:
        rng = np.random.default_rng(3)
        probe_all_counts(sol, scene, rng, ('exp3', 'before'))
        for _ in range(3):
            sol.env_step(S.NBR_KDTREE)
        probe_all_counts(sol, scene, rng, ('exp3', 'after 3'))
    finally:
        sol.close()


def test_probe_in_grid_mode(S):
    """SCA_NBR_GRID builds no agent tree at all: the probe reads the records.  The fuzz scenes the grid takes for three steps."""
    done = 0
    for seed in RR.SEEDS[:20]:
        scene = F.random_scene(seed)
        sol = context_of(S, scene, perm=False)
        try:
            try:
                for _ in range(3):
                    sol.env_step(S.NBR_GRID)
            except S.ScaError as e:
                assert 'SCA_NBR_GRID needs' in str(e), str(e)
                continue
            probe_all_counts(sol, scene, np.random.default_rng(seed), ('grid', seed))
            done += 1
        finally:
            sol.close()
        if done >= 4:
            break
    assert done >= 4, done


@pytest.mark.parametrize('name', ['F20_edge_lattice4_s2_orca', 'F20_edge_lattice3_s2_a', 'F20_edge_lattice4_s10_mixed'])
def test_probe_lattice_ties(S, name):
    """equal distances to 6 / 12 / 8 partners: the lowest id wins"""
    scene = E.step_scene(name, 0)
    n = scene['n']
    sol = context_of(S, scene)
    try:
        sol.set_kd_perm(scene['perm'])
        ties = []
        probe_check(sol, scene['radius'], scene, scene['pos'], scene['radius'], np.arange(n, dtype=np.int32), (name, 0), ties=ties)
        assert sum(1 for t in ties if t > 1) >= 5, name
        for _ in range(3):
            sol.env_step(S.NBR_KDTREE)
        probe_check(sol, scene['radius'], scene, sol.get_state()['pos'], scene['radius'], np.arange(n, dtype=np.int32), (name, 3))
    finally:
        sol.close()


# ---- freshness ---------------------------------------------------------------------------------------------------------------------------
def test_probe_sees_a_respawn_and_a_new_state_at_once(S):
    """directly behind sca_respawn_agents and directly behind sca_set_state, no step in between, in AUTO mode (whose bursts build ahead)"""
    scene = F.random_scene(5)
    n = scene['n']
    radius = scene['radius'].copy()
    sol = context_of(S, scene)
    try:
        sol.run_steps(3, S.NBR_AUTO)
        sol.synchronize()
        ids = np.array([3, 40, 41, 200], np.int32)
        m = mission_for(scene, ids, 9)
        m['pos'] = m['pos'] + np.array([[500.0 + 50.0 * k, 0.0, 0.0] for k in range(4)])      # far from everybody: only the probe's own partner is there
        respawn(sol, m)
        radius[ids] = m['radius']
        got = probe_check(sol, radius, scene, m['pos'], np.full(4, 0.25), None, 'behind the respawn')
        assert np.array_equal(got['agent_partner'], ids) and np.array_equal(got['agent_clear'], 0.0 - (0.25 + m['radius']))
        old = probe_check(sol, radius, scene, scene['pos'][ids], np.full(4, 0.25), None, 'where they were')
        assert not np.isin(old['agent_partner'], ids).any()
        st = sol.get_state()
        moved = st['pos'] + np.array([0.0, 1000.0, 0.0])
        sol.set_state(moved, st['vel'], st['heading'], st['flags'], st['total_dist'], st['step_num'])
        pick = np.arange(0, n, 7, dtype=np.int32)
        got = probe_check(sol, radius, scene, moved[pick], radius[pick], pick, 'behind set_state')
        gone = probe_check(sol, radius, scene, st['pos'][pick], radius[pick], None, 'the old places')
        assert (gone['agent_clear'] > 100.0).all() and np.isfinite(got['agent_clear']).all()
    finally:
        sol.close()


# ---- the gated respawn on the corpus -----------------------------------------------------------------------------------------------------
def gated(sol, m, margin=SR.MARGIN, **kw):
    return sol.respawn(m['ids'], m['pos'], m['vel'], m['heading'], m['radius'], m['pref_speed'], m['goal'], m['max_run_dist'], margin=margin, **kw)


def words(sol, lists=False, clearance=False, twin=False, grid=False):
    """every word the tests can read.  twin: for the comparison of two contexts -- what no pass has written (list entries behind nbr_n, the
    rows no pass has served) is taken out: it is whatever the allocation held.  grid: SCA_ST_NBR_OVERFLOW is taken out of the status words
    too -- on a row whose collision flag the pass raised the bit depends on the order the grid met the objects in (the grid's stated
    contract, tests/test_gpu_grid_fuzz.py), which two contexts do not share"""
    out = snapshot(sol)
    if grid:
        out['diag_status'] = out['diag_status'] & ~32
    if twin:
        valid = out['nbr_nbr_valid'].astype(bool)
        in_list = valid[:, None] & (np.arange(out['nbr_nbr_id'].shape[1])[None, :] < out['nbr_nbr_n'][:, None])
        for k in ('nbr_nbr_id', 'nbr_nbr_kind', 'nbr_nbr_dsq'):
            out[k] = np.where(in_list, out[k], 0)
        out['nbr_nbr_n'] = np.where(valid, out['nbr_nbr_n'], 0)
        for k in ('diag_diag', 'diag_vpref'):
            out[k] = np.where(valid[:, None], out[k], 0)
    if lists:
        out['path_left'], out['now_goal'] = sol.get_path_state()
    if clearance:
        rec = sol.clearance()
        out.update({'clear_' + f: rec[f] for f in rec.dtype.names})
    return out


def same_words(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == 'f'), what + (k,)


def run_gated_corpus(S, oracle, scene, nbr, ctx, steps=RR.STEPS, grid=False):
    """context A takes the offered missions through the gate, its twin B plainly respawns the admitted subset: the verdicts and the world
    test's records are the rule's, A and B are equal word for word behind the call and behind the step, and both equal the gated oracle run"""
    ref = SR.oracle_run_gated(oracle, scene, steps, list_rule=1 if grid else 0)
    if grid:
        from test_gpu_grid_fuzz import compare_grid_step
    a, b = context_of(S, scene, perm=not grid), context_of(S, scene, perm=not grid)
    whole = True
    try:
        for t, r in enumerate(ref):
            at = ctx + ('n', scene['n'], 'step', t)
            if r['offered'] is not None:
                v, rec = gated(a, r['offered'])
                assert np.array_equal(v, r['verdict']), at + ('verdict', np.flatnonzero(v != r['verdict'])[:8].tolist())
                assert differ(rec, r['probe']).size == 0, at + ('probe',)
                if r['mission'] is not None:
                    respawn(b, r['mission'])
                if t > 0:
                    assert a.active_count() == r['active_before'], at + ('active_count behind the call',)
                    same_words(words(a, twin=True, grid=grid), words(b, twin=True, grid=grid), at + ('behind the call',))
            try:
                a.run_steps(1, nbr)
                b.run_steps(1, nbr)
            except S.ScaError as e:
                assert grid and 'SCA_NBR_GRID needs' in str(e), at + (str(e),)
                whole = False
                break
            a.synchronize()
            b.synchronize()
            for sol in (a, b):
                (compare_grid_step if grid else compare_with_oracle)(sol, r, scene, at)
                assert sol.active_count() == scene['n'] - len(r['finished']), at
                assert np.array_equal(sol.finished()['id'], r['finished']), at
            same_words(words(a, twin=True, grid=grid), words(b, twin=True, grid=grid), at + ('behind the step',))
    finally:
        a.close()
        b.close()
    return whole


@pytest.mark.parametrize('block', range(4))
def test_gated_corpus_kd(S, oracle, block):
    for seed in RR.SEEDS[10 * block:10 * block + 10]:
        run_gated_corpus(S, oracle, F.random_scene(seed), S.NBR_KDTREE, ('kd', 'seed', seed))


def test_gated_corpus_auto(S, oracle):
    for seed in RR.SEEDS[:10]:
        run_gated_corpus(S, oracle, F.random_scene(seed), S.NBR_AUTO, ('auto', 'seed', seed))


def test_gated_corpus_grid(S, oracle):
    whole = sum(run_gated_corpus(S, oracle, F.random_scene(seed), S.NBR_GRID, ('grid', 'seed', seed), steps=6, grid=True) for seed in RR.SEEDS[:16])
    assert whole >= 6, whole


def partly(scene, ids, seed, blocked, pos_now, line=0):
    """a mission for the rows ids: the rows `blocked` (places in ids) start on top of another agent where it stands now, the others on a
    line of free places far outside the scene, 4 m apart (line: which one -- a later call finds the earlier line occupied)"""
    m = mission_for(scene, np.asarray(ids, np.int32), seed)
    others = np.setdiff1d(np.arange(scene['n']), ids)
    blocked = set(blocked)
    for j in range(len(m['ids'])):
        if j in blocked:
            m['pos'][j] = pos_now[others[(7 * j) % len(others)]] + np.array([0.05, 0.0, 0.0])
        else:
            m['pos'][j] = [300.0 + 4.0 * j, 50.0 * line, 6.0]
    m['max_run_dist'] = 3.0 * np.linalg.norm(m['pos'] - m['goal'], axis=1) + 1.0
    return m


def test_gated_lists_in_slot_form(S, oracle):
    """slot-form lists: the call's CSR is cut down to the admitted rows -- a refused row keeps its list, its cursor and its now_goal"""
    W = 5
    cut = 0
    for seed in (3, 5, 12):
        scene = F.random_scene(seed)
        ref = SR.oracle_run_gated(oracle, scene, 9, lists=W)
        a, b = context_of(S, scene), context_of(S, scene)
        try:
            for sol in (a, b):
                sol.set_path_slots(W, [lst[:W] for lst in F.random_paths(seed, scene)])
                sol.set_vpref(scene['vpref'], scene['vmode'])
            for t, r in enumerate(ref):
                at = ('lists', 'seed', seed, 'step', t)
                if r['offered'] is not None:
                    v, _ = gated(a, r['offered'], paths=r['offered']['paths'])
                    assert np.array_equal(v, r['verdict']), at
                    if r['mission'] is not None:
                        respawn(b, r['mission'], paths=r['mission']['paths'])
                    cut += int(r['offered']['paths'] is not None and (v != 0).any() and (v == 0).any())
                    same_words(words(a, lists=True, twin=True), words(b, lists=True, twin=True), at + ('behind the call',))
                a.run_steps(1, S.NBR_KDTREE)
                b.run_steps(1, S.NBR_KDTREE)
                for sol in (a, b):
                    sol.synchronize()
                    compare_with_oracle(sol, r, scene, at)
                    check_paths(sol, r, scene, at)
        finally:
            a.close()
            b.close()
    assert cut >= 3, cut


def test_gated_clearance_records_and_step_forms(S, oracle):
    """closest-approach records on: emptied for the admitted rows only.  Behind a gated call sca_run_steps(3) and sca_policy_pass +
    sca_env_update run as behind the plain respawn of the admitted subset."""
    scene = F.random_scene(5)
    n = scene['n']
    a, b = context_of(S, scene), context_of(S, scene)
    try:
        for sol in (a, b):
            sol.clearance_enable()
            sol.run_steps(2, S.NBR_KDTREE)
            sol.synchronize()
        radius = scene['radius'].copy()
        for k, form in enumerate(('burst3', 'pass_update', 'env_step')):
            pos = a.get_state()['pos']
            ids = np.sort(np.random.default_rng(k).choice(n, 24, replace=False)).astype(np.int32)
            m = partly(scene, ids, 70 + k, range(0, 24, 3), pos, line=k)
            want_v, want_rec = SR.gate(m['ids'], m['pos'], m['radius'], SR.MARGIN, pos, radius, scene['obs_pos'], scene['obs_radius'])
            before = a.clearance()
            v, rec = gated(a, m)
            assert np.array_equal(v, want_v) and differ(rec, want_rec).size == 0, form
            ok = v == 0
            assert ok.any() and (~ok).sum() >= 8, (form, v)
            respawn(b, SR.cut(m, ok))
            radius[ids[ok]] = m['radius'][ok]
            after = a.clearance()
            keep = np.setdiff1d(np.arange(n), ids[ok])
            assert np.array_equal(after[keep], before[keep]) and np.array_equal(after[ids[ok]], CR.empty(int(ok.sum()))), form
            same_words(words(a, clearance=True, twin=True), words(b, clearance=True, twin=True), (form, 'behind the call'))
            for sol in (a, b):
                if form == 'burst3':
                    sol.run_steps(3, S.NBR_KDTREE)
                elif form == 'pass_update':
                    sol.policy_pass(S.NBR_KDTREE)
                    with pytest.raises(S.ScaError, match='between a policy pass'):
                        gated(sol, m)
                    with pytest.raises(S.ScaError, match='between a policy pass'):
                        sol.probe_clearance(m['pos'], m['radius'])
                    sol.env_update()
                else:
                    sol.env_step(S.NBR_KDTREE)
                sol.synchronize()
            same_words(words(a, clearance=True, twin=True), words(b, clearance=True, twin=True), (form, 'behind the step'))
    finally:
        a.close()
        b.close()


def test_gated_host_state_block_follows_a_partly_refused_call(S, oracle):
    """the state block handed out by sca_host_state_get: the admitted rows' columns are the call's, a refused row's stay; a
    SCA_HOST_IN_STATE step then runs as the plain twin's"""
    scene = F.random_scene(12)
    n = scene['n']
    a, b = context_of(S, scene), context_of(S, scene)
    try:
        blocks = []
        for sol in (a, b):
            h = sol.host_state()
            g = sol.get_state()
            for k in F.STATE_KEYS:
                h[k][...] = g[k]
            assert sol.step_host(S.NBR_KDTREE, state=True) >= 0
            blocks.append(h)
        pos = a.get_state()['pos']
        ids = np.arange(2, n, 5, dtype=np.int32)
        m = partly(scene, ids, 5, range(1, len(ids), 2), pos)
        keep = {k: blocks[0][k].copy() for k in F.STATE_KEYS}
        v, _ = gated(a, m)
        assert np.array_equal(v, SR.gate(m['ids'], m['pos'], m['radius'], SR.MARGIN, pos, scene['radius'], scene['obs_pos'], scene['obs_radius'])[0])
        ok = v == 0
        assert ok.any() and (~ok).any()
        respawn(b, SR.cut(m, ok))
        h = blocks[0]
        assert np.array_equal(h['pos'][ids[ok]], m['pos'][ok]) and not h['flags'][ids[ok]].any() and not h['total_dist'][ids[ok]].any()
        rest = np.setdiff1d(np.arange(n), ids[ok])
        for k in F.STATE_KEYS:
            assert np.array_equal(h[k][rest], keep[k][rest]), k
            assert np.array_equal(blocks[0][k], blocks[1][k]), k
        for _ in range(3):
            assert a.step_host(S.NBR_KDTREE, state=True) == b.step_host(S.NBR_KDTREE, state=True)
            for k in F.STATE_KEYS:
                assert np.array_equal(blocks[0][k], blocks[1][k]), k
        same_words(words(a, twin=True), words(b, twin=True), ('step_host',))
    finally:
        a.close()
        b.close()


def test_gated_tracked_rows_among_tracked_others(S):
    """the device tracker inside the pass: admitted tracked rows take the initial record, refused tracked rows and everybody else keep
    their plans and re-plan counts word for word; the twins fly on equal"""
    from test_gpu_respawn import tracked_scene
    n = 48
    sc_ = tracked_scene(n, n)
    sc = sc_['sc']
    ext = np.isin(sc_['policy'], (0, 5))
    radius, ps, goal, gh = np.full(n, 0.5), np.ones(n), np.ascontiguousarray(sc['goal'][:, :3]), np.ascontiguousarray(sc['goal'][:, 3:6])
    sols = []
    try:
        for _ in range(2):
            sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
            sols.append(sol)
            sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
            sol.set_agents(radius, ps, goal, sc_['policy'], sc_['zaxis'], np.array(sc_['mrd'], np.float64))
            sol.set_state(sc['start'][:, :3], np.zeros((n, 3), np.float32), sc['start'][:, 3:6], np.zeros(n, np.uint8))
            sol.device_tracker_enable(gh, in_pass=True)
            sol.run_steps(5, S.NBR_KDTREE)
            sol.synchronize()
        a, b = sols
        rng = np.random.default_rng(4)
        pos = a.get_state()['pos']
        ids = np.sort(rng.choice(n, 18, replace=False)).astype(np.int32)
        k = len(ids)
        ang = rng.uniform(0, 2 * np.pi, k)
        new_pos = np.stack([30.0 + 3.0 * np.arange(k), np.zeros(k), np.full(k, 10.0)], 1)          # a row of free places ...
        others = np.setdiff1d(np.arange(n), ids)
        for j in range(0, k, 3):                                                                    # ... every third one on top of somebody
            new_pos[j] = pos[others[j]] + np.array([0.0, 0.1, 0.0])
        new_goal = np.stack([-10.0 * np.cos(ang), -10.0 * np.sin(ang), np.full(k, 10.0)], 1)
        new_head = np.stack([ang, np.zeros(k), np.zeros(k)], 1)
        args = (new_pos, np.zeros((k, 3), np.float32), new_head, np.full(k, 0.5), np.ones(k), new_goal, 3.0 * np.linalg.norm(new_pos - new_goal, axis=1) + 1.0)
        dbg = [a.device_tracker_debug(i) for i in range(n)]
        rep = a.device_tracker_replans()
        v, _ = a.respawn(ids, *args, goal_heading=new_head, margin=SR.MARGIN)
        assert np.array_equal(v, SR.gate(ids, new_pos, np.full(k, 0.5), SR.MARGIN, pos, radius, np.zeros((0, 3)), np.zeros(0))[0])
        ok = v == 0
        assert (ok & ext[ids]).any() and (~ok & ext[ids]).any() and ext[others].any()               # tracked ones admitted and refused, among tracked others
        b.respawn(ids[ok], *[x[ok] for x in args], goal_heading=new_head[ok])
        kept = np.setdiff1d(np.arange(n), ids[ok])
        rep2 = a.device_tracker_replans()
        assert np.array_equal(rep2[kept], rep[kept]) and not rep2[ids[ok]][ext[ids[ok]]].any()
        for i in range(n):
            da, db = a.device_tracker_debug(i), b.device_tracker_debug(i)
            assert np.array_equal(da, db, equal_nan=True), i
            if i in kept:
                assert np.array_equal(da, dbg[i], equal_nan=True), i
        for t in range(6):
            for sol in sols:
                sol.run_steps(1, S.NBR_KDTREE)
                sol.synchronize()
            same_words(words(a, twin=True), words(b, twin=True), ('tracked', t))
            assert np.array_equal(a.device_tracker_replans(), b.device_tracker_replans()), t
    finally:
        for sol in sols:
            sol.close()


def small_world(S):
    """four ORCA3D drones far from each other, no obstacles"""
    n = 4
    pos = np.array([[0.0, 0.0, 5.0], [50.0, 0.0, 5.0], [60.0, 0.0, 5.0], [70.0, 0.0, 5.0]])
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
    sol.set_agents(np.full(n, 0.5), 1.0, pos + np.array([0.0, 30.0, 0.0]), 3)
    sol.set_state(pos, np.zeros((n, 3), np.float32), np.zeros((n, 3)), np.zeros(n, np.uint8))
    return sol, pos


def small_call(sol, ids, pos, margin):
    k = len(ids)
    return sol.respawn(np.asarray(ids, np.int32), pos, np.zeros((k, 3), np.float32), np.zeros((k, 3)), np.full(k, 0.5), np.ones(k), np.asarray(pos) + np.array([0.0, 30.0, 0.0]),
                       np.full(k, 100.0), margin=margin)


def test_the_margin_boundary_pair_and_the_chain(S):
    below = float(np.nextafter(1.0, 0.0))
    sol, pos = small_world(S)
    try:
        q = np.array([[2.0, 0.0, 5.0]])
        rec = sol.probe_clearance(q, 0.5, [1])
        assert rec['agent_clear'][0] == 1.0 and rec['agent_partner'][0] == 0 and np.isinf(rec['obs_clear'][0]) and rec['obs_partner'][0] == -1
        before = words(sol)
        v, rec = small_call(sol, [1], q, 1.0)                                 # c == margin: refused, and nothing has changed
        assert v.tolist() == [SR.BLOCKED_AGENT] and rec['agent_clear'][0] == 1.0
        same_words(before, words(sol), ('refused at the margin',))
        v, _ = small_call(sol, [1], q, below)
        assert v.tolist() == [SR.ADMITTED] and np.array_equal(sol.get_state()['pos'][1], q[0])
        # two rows of one call at distance 2.0: an entry block at 1.0, none just below
        two = np.array([[100.0, 0.0, 5.0], [102.0, 0.0, 5.0]])
        assert small_call(sol, [2, 3], two, 1.0)[0].tolist() == [SR.ADMITTED, SR.BLOCKED_ENTRY]
        assert np.array_equal(sol.get_state()['pos'][[2, 3]], [two[0], pos[3]])
        assert small_call(sol, [3], two[1:], below)[0].tolist() == [SR.ADMITTED]
    finally:
        sol.close()
    sol, pos = small_world(S)
    try:
        # a < b < c, b within the margin of both: c is refused although b was
        rows = np.array([[100.0, 0.0, 5.0], [101.2, 0.0, 5.0], [102.4, 0.0, 5.0]])
        assert small_call(sol, [1, 2, 3], rows, 0.5)[0].tolist() == [SR.ADMITTED, SR.BLOCKED_ENTRY, SR.BLOCKED_ENTRY]
        # an earlier row the WORLD blocked blocks nobody
        rows2 = np.array([[1.2, 0.0, 5.0], [2.4, 0.0, 5.0]])
        assert small_call(sol, [2, 3], rows2, 0.5)[0].tolist() == [SR.BLOCKED_AGENT, SR.ADMITTED]
        got = sol.get_state()['pos']
        assert np.array_equal(got, [pos[0], rows[0], pos[2], rows2[1]])
    finally:
        sol.close()


def test_a_call_that_admits_nobody_changes_nothing(S):
    for mode, seed in (('kd', 12), ('auto', 12), ('grid', 4)):
        scene = F.random_scene(seed)
        n = scene['n']
        sol = context_of(S, scene, perm=mode != 'grid')
        try:
            if mode == 'kd':
                sol.clearance_enable()
            sol.host_state()
            sol.run_steps(2, mode_of(S, mode))
            sol.synchronize()
            pos = sol.get_state()['pos']
            ids = np.arange(0, n, 3, dtype=np.int32)
            m = partly(scene, ids, 8, range(len(ids)), pos)
            before = words(sol, clearance=mode == 'kd')
            block = {k: v.copy() for k, v in sol.host_state().items()}
            v, _ = gated(sol, m)
            assert (v == SR.BLOCKED_AGENT).all(), mode
            same_words(before, words(sol, clearance=mode == 'kd'), (mode, 'nobody admitted'))
            for k, x in sol.host_state().items():
                assert np.array_equal(x, block[k], equal_nan=True), (mode, k)
            sol.run_steps(1, mode_of(S, mode))
            sol.synchronize()
        finally:
            sol.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_both_calls_change_nothing(S):
    import sca_amd._lib as _lib
    scene = F.random_scene(12)
    n = scene['n']
    m = mission_for(scene, np.array([3, 7, 20, 41], np.int32), 1)
    ip, dp, fp = (lambda x: _lib.ptr(x, C.c_int32)), (lambda x: _lib.ptr(x, C.c_double)), (lambda x: _lib.ptr(x, C.c_float))
    out = np.zeros(8, _lib.CLEARANCE_DTYPE)
    op = out.ctypes.data_as(C.POINTER(_lib.SceneClearance))
    verdict = np.zeros(8, np.int32)

    def probe(sol, count=4, pos=m['pos'], radius=m['radius'], ignore=None, outp=op, struct_bytes=32):
        keep = [None if x is None else np.ascontiguousarray(x, t) for x, t in ((pos, np.float64), (radius, np.float64), (ignore, np.int32))]
        rc = sol.L.sca_probe_clearance(sol.ctx, count, None if keep[0] is None else dp(keep[0]), None if keep[1] is None else dp(keep[1]),
                                       None if keep[2] is None else ip(keep[2]), outp, struct_bytes)
        return rc, sol.L.sca_last_error(sol.ctx).decode()

    def gate(sol, margin=0.5, have_verdict=True, **kw):
        a = dict(m, zaxis=None, goal_heading=None, path_offsets=None, path_points=None, count=len(m['ids']))
        a.update(kw)
        keep = {k: (None if a[k] is None else np.ascontiguousarray(a[k], {'ids': np.int32, 'vel': np.float32, 'path_offsets': np.int32, 'zaxis': np.uint8}.get(k, np.float64)))
                for k in a if k not in ('count', 'paths')}
        p = lambda k, f: None if keep[k] is None else f(keep[k])
        rc = sol.L.sca_respawn_agents_gated(sol.ctx, a['count'], p('ids', ip), p('pos', dp), p('vel', fp), p('heading', dp), p('radius', dp), p('pref_speed', dp),
                                            p('goal', dp), p('zaxis', lambda z: _lib.ptr(z, C.c_uint8)), p('max_run_dist', dp), p('goal_heading', dp),
                                            p('path_offsets', ip), p('path_points', dp), margin, ip(verdict) if have_verdict else None, None, None)
        return rc, sol.L.sca_last_error(sol.ctx).decode()

    sol = S.BatchedSolver(max_agents=n, max_obstacles=max(1, scene['m']))
    try:
        assert probe(sol)[0] == ERR_STATE and gate(sol)[0] == ERR_STATE                              # no agents
        sol.set_obstacles(scene['obs_pos'], scene['obs_radius'])
        sol.set_agents(scene['radius'], scene['pref_speed'], scene['goal'], scene['policy'], F.zaxis_of(scene), scene['max_run_dist'])
        assert probe(sol)[0] == ERR_STATE and gate(sol)[0] == ERR_STATE                              # no state
    finally:
        sol.close()
    sol = context_of(S, scene)
    try:
        sol.run_steps(2, S.NBR_KDTREE)
        sol.synchronize()
        before = words(sol)

        def unchanged(what):
            same_words(before, words(sol), (what,))
        bad = lambda k, v, j=1: np.concatenate([np.asarray(m[k])[:j], [v], np.asarray(m[k])[j + 1:]])
        nan_pos = m['pos'].copy()
        nan_pos[2, 1] = np.nan
        for what, kw in [('count 0', dict(count=0)), ('count -1', dict(count=-1)), ('NULL pos', dict(pos=None)), ('NULL radius', dict(radius=None)),
                         ('NULL out', dict(outp=None)), ('nan position', dict(pos=nan_pos)), ('inf position', dict(pos=np.where(np.isnan(nan_pos), -np.inf, nan_pos))),
                         ('radius < 0', dict(radius=bad('radius', -0.1))), ('radius nan', dict(radius=bad('radius', np.nan))), ('radius inf', dict(radius=bad('radius', np.inf))),
                         ('ignore -2', dict(ignore=[0, -2, 1, 2])), ('ignore n', dict(ignore=[0, 1, 2, n])), ('struct 24', dict(struct_bytes=24)), ('struct 40', dict(struct_bytes=40))]:
            rc, msg = probe(sol, **kw)
            assert rc == ERR_ARG and 'sca_probe_clearance' in msg, (what, rc, msg)
            unchanged(what)
        assert probe(sol, radius=np.zeros(4))[0] == 0 and probe(sol, ignore=[-1, 0, n - 1, 5])[0] == 0          # a point probe; the whole range of ignore
        unchanged('legal probes')
        cases = [('count 0', dict(count=0), ERR_ARG)] + [('NULL ' + k, {k: None}, ERR_ARG) for k in ('ids', 'pos', 'vel', 'heading', 'radius', 'pref_speed', 'goal', 'max_run_dist')]
        cases += [('id n', dict(ids=bad('ids', n)), ERR_ARG), ('repeated id', dict(ids=bad('ids', 3)), ERR_ARG), ('nan position', dict(pos=nan_pos), ERR_ARG),
                  ('radius 0', dict(radius=bad('radius', 0.0)), ERR_ARG), ('pref_speed < 0', dict(pref_speed=bad('pref_speed', -1.0)), ERR_ARG),
                  ('offsets alone', dict(path_offsets=np.zeros(5, np.int32)), ERR_ARG),
                  ('paths without slots', dict(path_offsets=np.zeros(5, np.int32), path_points=np.zeros(3)), ERR_UNSUPPORTED),
                  ('margin < 0', dict(margin=-0.1), ERR_ARG), ('margin nan', dict(margin=float('nan')), ERR_ARG), ('margin inf', dict(margin=float('inf')), ERR_ARG),
                  ('NULL verdict', dict(have_verdict=False), ERR_ARG)]
        for what, kw, code in cases:
            rc, msg = gate(sol, **kw)
            assert rc == code and 'sca_respawn_agents_gated' in msg, (what, rc, msg)
            unchanged(what)
        # between a policy pass and its env update
        sol.policy_pass(S.NBR_KDTREE)
        assert probe(sol)[0] == ERR_STATE and gate(sol)[0] == ERR_STATE
        sol.env_update()
        sol.synchronize()
        before = words(sol)
        # lists in block form; a tracked row without goal_heading
        sol.set_paths([[] for _ in range(n)][:-1] + [[[1.0, 2.0, 3.0]]])
        rc, msg = gate(sol)
        assert rc == ERR_UNSUPPORTED and 'sca_set_path_slots' in msg, msg
        assert probe(sol)[0] == 0                                                                    # (the probe does not mind the lists)
        sol.set_paths(None)
        unchanged('lists')
        tracked = np.flatnonzero(np.isin(scene['policy'], (0, 5)))[:4].astype(np.int32)
        sol.device_tracker_enable(np.zeros((n, 3)))
        before = words(sol)                                                                          # (enabling the tracker invalidates the last pass's lists)
        rc, msg = gate(sol, ids=tracked)
        assert rc == ERR_ARG and 'goal_heading' in msg, msg
        assert probe(sol)[0] == 0
        unchanged('tracker')
        sol.device_tracker_disable()
        # a shard, the cell-owner partition, scenes
        sol.set_shard(0, n - 1)
        for rc, msg in (probe(sol), gate(sol)):
            assert rc == ERR_UNSUPPORTED and 'shard' in msg, msg
        sol.set_shard(0, n)
        sol.partition_init(0, 1)
        for rc, msg in (probe(sol), gate(sol)):
            assert rc == ERR_UNSUPPORTED and 'partition' in msg, msg
        sol.partition_disable()
        sol.set_scenes([0, n // 2, n])
        for rc, msg in (probe(sol), gate(sol)):
            assert rc == ERR_UNSUPPORTED and 'scenes' in msg, msg
    finally:
        sol.close()


# ---- the Python layers -------------------------------------------------------------------------------------------------------------------
def circle_env(E):
    n = 16
    agents = E.build_circle_agents(n, policy=E.RVO3DPolicy, rad=4.0)
    obstacles = [E.Obstacle(pos=[round(1.5 * math.cos(2 * j * math.pi / 8), 2), round(1.5 * math.sin(2 * j * math.pi / 8), 2), 10.0],
                            shape_dict={'shape': 'sphere', 'feature': 0.3}, id=j) for j in range(8)]
    env = E.MACAEnv()
    env.set_agents(agents, obstacles=obstacles)
    return env, agents, obstacles


def world_of_env(env, obstacles):
    return (np.array(env.pos), np.array([a.radius for a in env.agents], np.float64), np.array([o.pos_global_frame for o in obstacles], np.float64).reshape(-1, 3),
            np.array([o.radius for o in obstacles], np.float64))


def test_env_probe_and_respawn_with_a_margin(S):
    from sca_amd import env as E
    env, agents, obstacles = circle_env(E)
    for _ in range(5):
        env.step()
    w = world_of_env(env, obstacles)
    q = np.array([[0.0, 0.0, 10.0], list(w[0][3]), [1.5, 0.0, 10.0]])
    got = env.probe(q, 0.5, ignore=[-1, 3, -1])
    assert differ(got, SR.probe(q, np.full(3, 0.5), [-1, 3, -1], *w)).size == 0
    assert got['obs_partner'][2] == 0 and got['obs_clear'][2] == -0.8
    mk = lambda i, start: E.Agent(start_pos=list(start) + [0.0, 0.0, 0.0], goal_pos=list(agents[i].goal_pos), vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0,
                                  policy=E.RVO3DPolicy, id=i)
    new = [mk(2, [20.0, 0.0, 10.0]), mk(5, w[0][6] + np.array([0.1, 0.0, 0.0])), mk(9, [1.5, 0.0, 10.0]), mk(11, [20.9, 0.0, 10.0]), mk(12, [40.0, 0.0, 10.0])]
    old = list(env.agents)
    admitted = env.respawn(new, margin=0.5)
    v, rec = env.last_spawn
    assert v.tolist() == [SR.ADMITTED, SR.BLOCKED_AGENT, SR.BLOCKED_OBSTACLE, SR.BLOCKED_ENTRY, SR.ADMITTED]
    want_v, want_rec = SR.gate([2, 5, 9, 11, 12], [a._pos for a in new], np.full(5, 0.5), 0.5, *w)
    assert np.array_equal(v, want_v) and differ(rec, want_rec).size == 0
    assert admitted == [new[0], new[4]] and env.agents[2] is new[0] and env.agents[12] is new[4]
    for i in (5, 9, 11):
        assert env.agents[i] is old[i] and np.array_equal(env.pos[i], w[0][i])                      # refused: the row's object and its words stay
    assert np.array_equal(env.pos[2], [20.0, 0.0, 10.0]) and np.array_equal(env.pos[12], [40.0, 0.0, 10.0])
    assert env.respawn([], margin=0.5) == [] and env.respawn([]) is None
    env.step()


def old_run_lifelong(env, next_mission, steps, S):
    """run_lifelong as it stood before the gate, restated: what `spawn_margin=None` must reproduce"""
    n = len(env.agents)
    stats = dict(steps=0, arrived=0, collided=0, timed_out=0, respawned=0, retired=0, agent_steps=0, live_fraction=0.0)
    retired = set()
    active = env._active
    for _ in range(int(steps)):
        if active == 0:
            break
        stats['agent_steps'] += active
        env.step()
        stats['steps'] += 1
        if env._active < active:
            new = []
            for row in env.finished():
                i = int(row['id'])
                if i in retired:
                    continue
                f = int(row['flags'])
                stats['collided' if f & S.FLAG_COLLISION else 'arrived' if f & S.FLAG_AT_GOAL else 'timed_out'] += 1
                nxt = next_mission(env.agents[i], row)
                if nxt is None:
                    retired.add(i)
                    stats['retired'] += 1
                else:
                    new.append(nxt)
            if new:
                env.respawn(new)
                stats['respawned'] += len(new)
        active = env._active
    stats['live_fraction'] = stats['agent_steps'] / float(n * stats['steps']) if stats['steps'] else 0.0
    return stats


def test_run_lifelong_with_a_spawn_margin(S):
    """the 16-drone circle among eight spheres: the stats identity, every admitted start recomputed from env.pos with the Python rule just
    before its respawn is clear by more than the margin; without a margin the run is what run_lifelong gave before"""
    from sca_amd import env as E
    from sca_amd.lifelong import run_lifelong

    def missions(env, agents):
        first = {a.id: (list(a.initial_pos), list(a.goal_pos)) for a in agents}
        count = {}

        def next_mission(agent, row):
            count[agent.id] = count.get(agent.id, 0) + 1
            if count[agent.id] >= 4:
                return None
            start, goal = first[agent.id]
            if int(row['flags']) == 1:
                start, goal = list(row['pos']) + list(agent.heading_global_frame), list(agent.initial_pos)
            return E.Agent(start_pos=start, goal_pos=goal, vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=E.RVO3DPolicy, id=agent.id)
        return next_mission

    env, agents, obstacles = circle_env(E)
    plain = env.respawn
    seen = dict(admitted=0, refused=0)

    def watched(new, margin=None):
        w = world_of_env(env, obstacles)
        ids = [a.id for a in new]
        want_v, _ = SR.gate(ids, [a._pos for a in new], [a.radius for a in new], margin, *w)
        out = plain(new, margin=margin)
        assert np.array_equal(env.last_spawn[0], want_v) and [a.id for a in out] == [i for i, v in zip(ids, want_v) if v == 0]
        for a in out:                                                                            # clear of the world as it stood, by more than the margin
            rec = SR.probe([a._pos], [a.radius], [a.id], *w)
            assert rec['agent_clear'][0] > margin and rec['obs_clear'][0] > margin, (a.id, rec)
        seen['admitted'] += len(out)
        seen['refused'] += len(new) - len(out)
        return out
    env.respawn = watched
    stats = run_lifelong(env, missions(env, agents), 400, spawn_margin=0.5)
    done = stats['arrived'] + stats['collided'] + stats['timed_out']
    assert done == stats['respawned'] + stats['retired'] + stats['waiting'], stats
    assert stats['respawned'] == seen['admitted'] > 0 and stats['deferred'] == seen['refused'], (stats, seen)
    assert set(stats) == {'steps', 'arrived', 'collided', 'timed_out', 'respawned', 'retired', 'agent_steps', 'live_fraction', 'deferred', 'waiting'}
    # without a margin: the loop and its dict are what they were
    env1, agents1, _ = circle_env(E)
    env2, agents2, _ = circle_env(E)
    s1 = run_lifelong(env1, missions(env1, agents1), 300)
    s2 = old_run_lifelong(env2, missions(env2, agents2), 300, S)
    assert s1 == s2 and list(s1) == list(s2), (s1, s2)
    for k in ('pos', 'flags', 'total_dist', 'step_num'):
        assert np.array_equal(getattr(env1, k), getattr(env2, k)), k
