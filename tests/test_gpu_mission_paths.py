"""Mission tables whose entries bring their own waypoint lists (sca_set_missions_paths) on the GPU (-m gpu).  Equality, no tolerance.

Two references, as in tests/test_gpu_missions.py.  The corpus of tests/mission_paths_rule.py: the fuzz scenes stepped free-running by the
oracle with the v_pref tests/path_rule.py yields, every row carrying a drawn table whose entries bring lists of 0 .. W points, the rule
applied behind every step -- state, action rows, neighbour lists, diag, permutation, sca_active_count, cursors, `ended`, results, totals,
what is left of every list, now_goal and the v_pref the pass used equal the rule's after every call, ungated and behind the gate.  And a
TWIN context without tables that does the same through sca_get_finished + sca_respawn_agents (plain or gated) WITH the entry's list as its
path arrays between its steps, equal word for word.  What a context holds of a row's room and length shows in what its later passes pop
(now_goal) and in the host calls that read the lengths (sca_set_vpref, sca_set_path_state), and is read word for word through
sca_get_path_slot_lists (the lengths and the rooms) and sca_get_vpref_mode."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import form_fuzz as F
import mission_paths_rule as PR
import mission_rule as MR
from test_gpu_form_fuzz import compare_with_oracle, context_of
from test_gpu_mission_gate import GateTwin, check_gate_words, same_gated
from test_gpu_missions import Twin, behind, by_row, check_words, context_for, edge_scene, same, snapshot, traffic_scene

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5
W = PR.W
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


@pytest.fixture()
def row_env(monkeypatch):
    """only the row's switches (form_fuzz.ROWS) are set while its contexts are created"""
    def set_row(row):
        for k in list(os.environ):
            if k.startswith('SCA_') and k != 'SCA_QUIET':
                monkeypatch.delenv(k)
        for k, v in (F.ROWS[row] if row else {}).items():
            monkeypatch.setenv(k, v)
    return set_row


# ---- the corpus ----------------------------------------------------------------------------------------------------------------------------
def corpus_context(S, scene, run, R=2, perm=True, gate=None):
    sol = context_of(S, scene, perm=perm)
    try:
        sol.set_path_slots(run['w'], run['initial'])
        sol.set_vpref(scene['vpref'], scene['vmode'])
        flat = PR.flat_lists(run['lists'])
        sol.set_missions(MR.M, R, run['entries'], run['first_ok'], run['first_fail'], paths=flat)
        assert sol.mission_paths() == (run['w'], sum(len(p) for p in flat))
        if gate is not None:
            sol.set_mission_gate(*gate)
    except BaseException:
        sol.close()
        raise
    return sol


def check_lists(sol, r, scene, at):
    """behind a step and its takes: what is left of every list and now_goal are the rule's; the v_pref the step's pass used is the rule's on
    the served rows it aims at a waypoint and the fed one on the served rows with a fed mode (test_gpu_form_fuzz.check_paths' rule)"""
    rem, ng = sol.get_path_state()
    assert np.array_equal(rem, r['path_left_after']), at + ('remaining', np.flatnonzero(rem != r['path_left_after'])[:8])
    assert np.array_equal(ng, r['now_goal_after'], equal_nan=True), at + ('now_goal',)
    served = (r['before'] & 7) == 0
    aimed, fed = served & r['path_mode'].astype(bool), served & scene['vmode'].astype(bool) & ~r['path_mode'].astype(bool)
    vp = sol.diag()['vpref']
    differ = (vp != r['vpref_rule']).any(axis=1)
    assert not (aimed & differ).any(), at + ('v_pref toward the waypoint', np.flatnonzero(aimed & differ)[:8])
    assert np.array_equal(vp[fed], scene['vpref'][fed]), at + ('fed v_pref',)
    rest = served & ~aimed & ~fed                                           # its policy's own rule: a row whose take reset the mode is here
    assert np.array_equal(vp[rest], r['vpref'][rest], equal_nan=True), at + ('the policy\'s own v_pref', np.flatnonzero(rest & (vp != r['vpref']).any(axis=1))[:8])
    # the device words themselves: every row's length, the first `len` points of its room, and the vpref_mode byte the next pass will read
    ln, rooms = sol.path_slot_lists()
    assert np.array_equal(ln, r['path_len_after']), at + ('len', np.flatnonzero(ln != r['path_len_after'])[:8])
    for a, lst in enumerate(r['rooms_after']):
        assert np.array_equal(rooms[a, :len(lst)], np.asarray(lst, np.float64).reshape(-1, 3)), at + ('room', a)
    mode = sol.vpref_mode()
    assert np.array_equal(mode, r['vpref_mode_after']), at + ('vpref_mode', np.flatnonzero(mode != r['vpref_mode_after'])[:8])


def run_corpus(S, oracle, scene, nbr, ctx, steps=PR.STEPS, R=2, per_call=1, gate=None):
    run = PR.oracle_run(oracle, scene, steps, gate=gate)
    sol = corpus_context(S, scene, run, R, gate=gate)
    try:
        for t0 in range(0, steps, per_call):
            at = ctx + ('n', scene['n'], 'step', t0)
            sol.run_steps(per_call, nbr)
            sol.synchronize()
            assert sol.pass_forms() & S.FORM_WAYPOINTS, at
            r = run['steps'][t0 + per_call - 1]
            compare_with_oracle(sol, behind(r), scene, at)
            check_lists(sol, r, scene, at)
            assert sol.active_count() == r['active'], at + ('active_count', sol.active_count(), r['active'])
            assert np.array_equal(sol.finished()['id'], r['finished']), at + ('finished ids',)
            check_words(sol, r, at)
            if gate is not None:
                check_gate_words(sol, r['waiting'], r['verdict'], r['refusals'], r['gate_totals'], at)
            want = by_row([s['results'] for s in run['steps'][t0:t0 + per_call]])
            if R < per_call:                                                # a row's last R results of the burst
                keep = np.ones(len(want), bool)
                for a in np.unique(want['id']):
                    keep[np.flatnonzero(want['id'] == a)[:-R]] = False
                want = want[keep]
            assert sol.mission_results().tobytes() == want.tobytes(), at + ('results',)
    finally:
        sol.close()


@pytest.mark.parametrize('block', range(4))
def test_corpus_kd_default_forms(S, oracle, row_env, block):
    """kd mode, default forms, all 40 seeds (1 .. 1600 agents), 12 steps, everything compared behind every step"""
    row_env(None)
    for seed in PR.SEEDS[10 * block:10 * block + 10]:
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_KDTREE, ('kd', 'seed', seed))


@pytest.mark.parametrize('row,mode,block', [(row, mode, b) for b in range(4) for row, mode in ((None, 'auto'), ('large_shard', 'kd'), ('large_shard', 'auto'))])
def test_corpus_auto_and_large_shard(S, oracle, row_env, row, mode, block):
    """SCA_NBR_AUTO and the forms every large shard runs, all 40 seeds"""
    row_env(row)
    for seed in PR.SEEDS[10 * block:10 * block + 10]:
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE, (row, mode, 'seed', seed))


def test_corpus_hostbuild(S, oracle, row_env):
    """SCA_NBR_KDTREE_HOSTBUILD: the host builds the tree from positions it fetches behind the device-side takes"""
    row_env(None)
    for seed in (3, 5, 12):
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_KDTREE_HOSTBUILD, ('hostbuild', 'seed', seed), steps=6)


def test_corpus_grid(S, oracle, row_env):
    """SCA_NBR_GRID against the oracle under list rule 1, on the scenes the grid takes (a scene it refuses ends at the refusal)"""
    from test_gpu_grid_fuzz import compare_grid_step
    row_env(None)
    whole = 0
    for seed in PR.SEEDS[:12]:
        scene = F.random_scene(seed)
        run = PR.oracle_run(oracle, scene, 6, list_rule=1)
        sol = corpus_context(S, scene, run, 1, perm=False)
        try:
            for t, r in enumerate(run['steps']):
                at = ('grid', 'seed', seed, 'step', t)
                try:
                    sol.run_steps(1, S.NBR_GRID)
                except S.ScaError as e:
                    assert 'SCA_NBR_GRID needs' in str(e), at + (str(e),)
                    break
                sol.synchronize()
                compare_grid_step(sol, behind(r), scene, at)
                check_lists(sol, r, scene, at)
                check_words(sol, r, at)
                assert sol.mission_results().tobytes() == r['results'].tobytes(), at + ('results',)
            else:
                whole += 1
        finally:
            sol.close()
    assert whole >= 6, whole


@pytest.mark.parametrize('per_call', [3, 12])
def test_corpus_bursts(S, oracle, row_env, per_call):
    """sca_run_steps(3) and (12) with no host call in between, kd and AUTO: a row taken inside the burst pops from its new list in the
    burst's later passes"""
    row_env(None)
    for seed, nbr, R in ((5, S.NBR_KDTREE, 12), (12, S.NBR_AUTO, 12), (17, S.NBR_AUTO, 1), (33, S.NBR_KDTREE, 1)):
        run_corpus(S, oracle, F.random_scene(seed), nbr, ('burst', per_call, 'seed', seed, 'R', R), R=R, per_call=per_call)


@pytest.mark.parametrize('cap,per_call', [(0, 1), (8, 1), (0, 3)])
def test_corpus_gated(S, oracle, row_env, cap, per_call):
    """the same corpus behind the gate (margin 0.5; the default cap and a cap of 8) in kd, step by step and in bursts of 3: an admitted row
    gets the entry's list, a candidate that waits keeps list, cursor and now_goal"""
    row_env(None)
    for seed in (3, 5, 12, 17, 21, 33):
        run_corpus(S, oracle, F.random_scene(seed), S.NBR_KDTREE, ('gated', cap, per_call, 'seed', seed), R=4, per_call=per_call, gate=(PR.GATE_MARGIN, cap))


# ---- the twin ------------------------------------------------------------------------------------------------------------------------------
def lists_for(sc, w=W, full=False):
    """one list per entry of a hand-built scene (sc['entries'] (n, m)): (a + j) % (w + 1) points -- neighbouring rows hold a full room
    beside an empty list -- between the row's start and the entry's goal, set off by 0.36 m and more (a waypoint ON the spot a row stands
    on makes the reference's v_pref 0 / 0), 2 cm apart per entry so that no two entries of a row share a list; full: every list holds w
    points.  And the rows' initial lists: (a + 1) % (w + 1) points"""
    n, m = sc['entries'].shape
    def pts(a, j, k):
        p, g = sc['start'][a], sc['entries']['goal'][a, j]
        return [[float(x) for x in np.round(p + (g - p) * (q + 1) / (k + 1) + [0.3 + 0.02 * j, 0.01 * q, 0.2], 3)] for q in range(k)]
    lists = [[pts(a, j, w if full else (a + j) % (w + 1)) for j in range(m)] for a in range(n)]
    initial = [pts(a, 0, w if full else (a + 1) % (w + 1)) for a in range(n)]
    return lists, initial


class WithLists:
    """a twin's context whose respawn brings, for every named row, the list of the entry the call's values are (matched by goal,
    pref_speed, max_run_dist and velocity: the hand-built tables hold no two such entries in a row)"""
    def __init__(self, sol, entries, lists):
        self._sol, self._e, self._lists = sol, entries, lists

    def __getattr__(self, name):
        return getattr(self._sol, name)

    def respawn(self, ids, pos, vel, heading, radius, pref_speed, goal, max_run_dist, **kw):
        paths = []
        for k, a in enumerate(ids):
            e = self._e[a]
            hit = [j for j in range(len(e)) if np.array_equal(e['goal'][j], goal[k]) and e['pref_speed'][j] == pref_speed[k] and e['max_run_dist'][j] == max_run_dist[k] and
                   np.array_equal(e['vel'][j], vel[k])]
            assert len(hit) == 1 or all(self._lists[a][j] == self._lists[a][hit[0]] for j in hit), (a, hit)
            paths.append(self._lists[a][hit[0]])
        return self._sol.respawn(ids, pos, vel, heading, radius, pref_speed, goal, max_run_dist, paths=paths, **kw)


def same_lists(A, B, at):
    (ra, ga), (rb, gb) = A.get_path_state(), B.get_path_state()
    assert np.array_equal(ra, rb), at + ('remaining', np.flatnonzero(ra != rb)[:8])
    assert np.array_equal(ga, gb, equal_nan=True), at + ('now_goal',)
    assert np.array_equal(A.diag()['vpref'], B.diag()['vpref'], equal_nan=True), at + ('the v_pref the pass used',)
    (la, pa), (lb, pb) = A.path_slot_lists(), B.path_slot_lists()           # the rooms whole: what stands behind a list is equal too
    assert np.array_equal(la, lb), at + ('len', np.flatnonzero(la != lb)[:8])
    assert np.array_equal(pa, pb), at + ('rooms', np.flatnonzero((pa != pb).reshape(len(pa), -1).any(1))[:8])
    assert np.array_equal(A.vpref_mode(), B.vpref_mode()), at + ('vpref_mode', np.flatnonzero(A.vpref_mode() != B.vpref_mode())[:8])


def twin_pair(S, sc, lists, initial, w=W, M=None, R=2, tracker_in_pass=True, clearance=False, gate=None):
    """A (tables with lists) and B (the twin's, without tables) from one scene, both in slot form with the same initial lists"""
    A = B = None
    try:
        A, B = context_for(S, sc, tracker_in_pass, clearance), context_for(S, sc, tracker_in_pass, clearance)
        for sol in (A, B):
            sol.set_path_slots(w, initial)
        m = sc['entries'].shape[1] if M is None else M
        A.set_missions(m, R, sc['entries'], sc['first_ok'], sc['first_fail'], paths=PR.flat_lists(lists))
        proxy = WithLists(B, sc['entries'], lists)
        if gate is None:
            tw = Twin(proxy, sc, clearance)
        else:
            A.set_mission_gate(*gate)
            tw = GateTwin(proxy, sc['n'], sc['entries'], sc['first_ok'], sc['first_fail'], sc['radius'], sc['zaxis'], gate[0], gate[1], tracker=sc['tracker'], clearance=clearance)
            tw.sc = sc
    except BaseException:
        for s in (A, B):
            if s is not None:
                s.close()
        raise
    return A, B, tw


def run_twin(S, sc, nbr, steps, at, w=W, full=False, gate=None, clearance=False, **kw):
    lists, initial = lists_for(sc, w, full)
    A, B, tw = twin_pair(S, sc, lists, initial, w, gate=gate, clearance=clearance, **kw)
    try:
        for t in range(steps):
            served = tw.running.copy()
            A.run_steps(1, nbr)
            res = tw.step(nbr)
            (same if gate is None else same_gated)(A, B, tw, at + ('step', t), served, sc['tracker'], res)
            same_lists(A, B, at + ('step', t))
    except BaseException:
        A.close()
        B.close()
        raise
    return A, B, tw


@pytest.mark.parametrize('seed', PR.SEEDS[::2])
def test_twin_on_the_corpus(S, oracle, row_env, seed):
    """every second kd seed of the fuzz corpus: the twin respawns with the drawn lists"""
    row_env(None)
    scene = F.random_scene(seed)
    run = PR.oracle_run(oracle, scene, 8)
    A = B = None
    try:
        A, B = corpus_context(S, scene, run), context_of(S, scene)
        B.set_path_slots(W, run['initial'])
        B.set_vpref(scene['vpref'], scene['vmode'])
        sc = dict(n=scene['n'], entries=run['entries'], first_ok=run['first_ok'], first_fail=run['first_fail'], zaxis=np.array(F.zaxis_of(scene), np.uint8),
                  radius=scene['radius'], tracker=False)
        tw = Twin(WithLists(B, run['entries'], run['lists']), sc)
        tw.running = (scene['flags'] & 7) == 0
        for t in range(8):
            served = tw.running.copy()
            A.run_steps(1, S.NBR_KDTREE)
            res = tw.step(S.NBR_KDTREE)
            same(A, B, tw, ('corpus twin', seed, 'step', t), served, False, res)
            same_lists(A, B, ('corpus twin', seed, 'step', t))
    finally:
        for s in (A, B):
            if s is not None:
                s.close()


@pytest.mark.parametrize('n,mode', [(48, 'kd'), (64, 'kd'), (33, 'auto')])
def test_twin_with_the_device_tracker(S, row_env, n, mode):
    """tracked rows among RVO3D, ORCA3D and ORCA3D-LP rows, the tracker inside the pass: a taken tracked row keeps mode 1 and the tracker's
    v_pref while its new list advances; plans and re-plan counts equal the twin's after every step"""
    row_env(None)
    sc = traffic_scene(n, True)
    A, B, tw = run_twin(S, sc, S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE, 14, ('tracker', n, mode), clearance=mode == 'kd')
    try:
        took = by_row(tw.results)
        took = took[took['next'] >= 0]
        assert tw.totals['taken'] > n // 2 and np.isin(sc['policy'][took['id']], (0, 5)).any() and (sc['policy'][took['id']] == 4).any()
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize('n,mode', [(48, 'kd'), (33, 'auto')])
def test_twin_under_the_gate(S, row_env, n, mode):
    """the gate at margin 0.5: the twin does sca_respawn_agents_gated with the lists as path arrays; a refused candidate keeps its list"""
    row_env(None)
    sc = traffic_scene(n, mode == 'kd')
    A, B, tw = run_twin(S, sc, S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE, 12, ('gate twin', n, mode), gate=(0.5, 0))
    try:
        assert tw.gate_totals['admitted'] > 0 and tw.gate_totals['offered'] > tw.gate_totals['admitted'], tw.gate_totals
    finally:
        A.close()
        B.close()


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_twin_sizes(S, row_env, n):
    """one row, one wavefront less one, exactly one, one more, and more than one workgroup; a full room beside an empty list in
    neighbouring rows (lists_for)"""
    row_env(None)
    sc = traffic_scene(n, False)
    sc['mrd'][0] = 0.25
    A, B, tw = run_twin(S, sc, S.NBR_KDTREE, 8, ('size', n))
    try:
        assert tw.totals['taken'] > 0
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize('n,count', [(n, c) for n in (2049, 6145) for c in (0, 1, 64, 65, -1)])
def test_twin_form_switches(S, row_env, n, count):
    """2049 / 6145 rows with 0, 1, 64, 65 and all rows ending in one step, each bringing a list of W points"""
    row_env(None)
    k = n if count < 0 else count
    sc = edge_scene(n, k)
    lists, initial = lists_for(sc, W, full=True)
    A, B, tw = twin_pair(S, sc, lists, initial, R=1)
    try:
        for t in range(3):
            served = tw.running.copy()
            A.run_steps(1, S.NBR_KDTREE)
            res = tw.step(S.NBR_KDTREE)
            if t == 0:
                assert len(res) == k and (res['next'] >= 0).all(), (n, count, len(res))
            same(A, B, tw, ('edge', n, count, 'step', t), served, False, res)
            same_lists(A, B, ('edge', n, count, 'step', t))
    finally:
        A.close()
        B.close()


def test_w1_and_m1(S, row_env):
    """a room of one point, and tables of one entry that retries itself"""
    row_env(None)
    sc = traffic_scene(80, False)
    A, B, tw = run_twin(S, sc, S.NBR_KDTREE, 8, ('W = 1',), w=1)
    A.close()
    B.close()
    assert tw.totals['taken'] > 0
    sc = traffic_scene(80, False)
    sc['entries'] = sc['entries'][:, 2:3].copy()
    sc['entries']['next_ok'], sc['entries']['next_fail'] = -1, 0
    sc['first_ok'], sc['first_fail'] = np.zeros(80, np.int32), np.zeros(80, np.int32)
    A, B, tw = run_twin(S, sc, S.NBR_KDTREE, 8, ('M = 1',), R=1)
    A.close()
    B.close()
    assert tw.totals['taken'] > 0 and tw.totals['stopped'] > 0


# ---- the hand-built shuttle ------------------------------------------------------------------------------------------------------------------
def shuttle():
    """one RVO3D drone, pad A -> two waypoints -> pad B, next_ok the reversed route back, both legs explicit starts at the pads"""
    a, b = np.array([0.0, 0.0, 5.0]), np.array([6.0, 0.0, 5.0])
    way = [[2.0, 1.0, 5.0], [4.0, 1.0, 5.0]]
    scene = dict(n=1, m=0, pos=a[None].copy(), goal=b[None].copy(), heading=np.zeros((1, 3)), vel=np.zeros((1, 3), np.float32), radius=np.array([0.5]),
                 pref_speed=np.array([1.0]), policy=np.array([1], np.uint8), flags=np.zeros(1, np.uint8), vpref=np.zeros((1, 3)), vmode=np.zeros(1, np.uint8),
                 obs_pos=np.zeros((0, 3)), obs_radius=np.zeros(0), max_run_dist=np.array([40.0]), key=('shuttle', 0))
    e = np.zeros((1, 2), MR.MISSION)
    e['pos'][0], e['goal'][0] = [b, a], [a, b]
    e['heading'][0, 0, 0] = math.pi
    e['pref_speed'], e['max_run_dist'] = 1.0, 40.0
    e['next_ok'][0], e['next_fail'][0] = [1, 0], [-1, -1]
    lists = [[way[:], way[::-1]]]                                           # (pop() takes the last: back B -> 4 -> 2 -> A, out again A -> 2 -> 4 -> B)
    return scene, (e, np.zeros(1, np.int32), np.full(1, -1, np.int32), lists, [way[::-1]])


@pytest.mark.parametrize('per_call', [1, 0])
def test_hand_built_shuttle(S, oracle, row_env, per_call):
    """until two arrivals, against the oracle + path_rule at every step; per_call 0: the same in ONE burst"""
    row_env(None)
    scene, tables = shuttle()
    steps = 220
    run = PR.oracle_run(oracle, scene, steps, w=2, tables=tables)
    arrivals = np.cumsum([int((s['results']['next'] >= 0).sum()) for s in run['steps']])
    assert arrivals[-1] >= 2 and run['steps'][-1]['totals']['arrived'] >= 2, arrivals[-1]
    steps = int(np.searchsorted(arrivals, 2)) + 3                           # two arrivals and the first passes of the third leg
    pops = sum(int((s['path_left'] < s['path_left_before']).sum()) for s in run['steps'][:steps])
    assert pops >= 5, pops                                                  # both waypoints of both legs
    sol = context_of(S, scene)
    try:
        sol.set_path_slots(2, tables[4])
        sol.set_missions(2, 4, tables[0], tables[1], tables[2], paths={(0, 0): tables[3][0][0], (0, 1): tables[3][0][1]})
        assert sol.mission_paths() == (2, 4)
        per = per_call or steps
        for t0 in range(0, steps, per):
            at = ('shuttle', per, 'step', t0)
            sol.run_steps(per, S.NBR_KDTREE)
            sol.synchronize()
            r = run['steps'][t0 + per - 1]
            compare_with_oracle(sol, behind(r), scene, at)
            check_lists(sol, r, scene, at)
            check_words(sol, r, at)
        assert sol.mission_results().tobytes() == by_row([s['results'] for s in run['steps'][:steps]]).tobytes()     # (R = 4: no ring overflows)
    finally:
        sol.close()


# ---- the mirrors -----------------------------------------------------------------------------------------------------------------------------
def exchange_scene():
    """four RVO3D rows 10 m apart that time out in their first step (max_run_dist 5 cm) and take entry 0, which flies on; row 0 holds a list
    and its entry brings the empty one, row 1 the other way round, row 2 exchanges a list of one point for one of two, row 3 has no table"""
    n = 4
    start = np.stack([10.0 * np.arange(n), np.zeros(n), np.full(n, 5.0)], 1)
    goal = start + [0.0, 30.0, 0.0]
    e = np.zeros((n, 1), MR.MISSION)
    e['goal'][:, 0] = goal
    e['pref_speed'], e['max_run_dist'] = 1.0, 200.0
    e['flags'] = MR.START_HERE | MR.KEEP_ZAXIS
    e['next_ok'], e['next_fail'] = -1, -1
    sc = dict(n=n, start=start, goal=goal, heading=np.zeros((n, 3)), mrd=np.full(n, 0.05), policy=np.ones(n, np.uint8), zaxis=np.zeros(n, np.uint8), radius=np.full(n, 0.5),
              entries=e, first_ok=np.array([0, 0, 0, -1], np.int32), first_fail=np.array([0, 0, 0, -1], np.int32), gh=np.zeros((n, 3)), tracker=False)
    mid = lambda a, k: [[float(x) for x in start[a] + [0.5, 5.0 * (q + 1), 0.0]] for q in range(k)]
    lists = [[[]], [mid(1, 2)], [mid(2, 2)], [[]]]
    initial = [mid(0, 2), [], mid(2, 1), mid(3, 1)]
    return sc, lists, initial


def test_the_host_mirrors_follow_the_takes(S, row_env):
    """after a burst in which row 0 exchanged a list for the empty one and row 1 the other way round: sca_set_vpref with mode 1 is accepted
    for exactly the first and refused for the second, sca_set_path_state is bounded by the new lengths, and a host respawn of the taken
    rows packs the mode bit of the lists they hold NOW -- the context equals the twin's behind the respawn and three more steps"""
    row_env(None)
    sc, lists, initial = exchange_scene()
    A, B, tw = twin_pair(S, sc, lists, initial, w=2)
    try:
        zero = np.zeros((4, 3))
        for sol in (A, B):
            with pytest.raises(S.ScaError, match='follows a waypoint list'): # in front of the burst: row 0 follows its list
                sol.set_vpref(zero, [1, 0, 0, 0])
            sol.set_vpref(zero, [0, 1, 0, 0])
            sol.set_vpref(zero, [0, 0, 0, 0])
        A.run_steps(3, S.NBR_KDTREE)
        for t in range(3):
            tw.step(S.NBR_KDTREE)
        assert tw.totals['taken'] == 3, tw.totals
        same(A, B, tw, ('exchange', 'burst'), None, False, by_row(tw.results))
        same_lists(A, B, ('exchange', 'burst'))
        before = snapshot(A)
        for mode, ok in (([1, 0, 0, 0], True), ([0, 1, 0, 0], False), ([0, 0, 1, 0], False), ([0, 0, 0, 1], False)):
            for sol in (A, B):                                              # (B's mirrors followed its host respawns: the same answers)
                if ok:
                    sol.set_vpref(zero, mode)
                    sol.set_vpref(zero, [0, 0, 0, 0])
                else:
                    with pytest.raises(S.ScaError, match='follows a waypoint list'):
                        sol.set_vpref(zero, mode)
        rem, ng = A.get_path_state()
        for sol in (A, B):
            for a, room in ((0, 0), (1, 2), (2, 2), (3, 1)):                # the bound is the NEW length: row 0's is 0, row 2's grew from 1 to 2
                over = rem.copy()
                over[a] = room + 1
                with pytest.raises(S.ScaError, match='remaining'):
                    sol.set_path_state(over, ng)
                fits = rem.copy()
                fits[a] = room
                sol.set_path_state(fits, ng)
            sol.set_path_state(rem, ng)
        after = snapshot(A)
        for k in before:
            assert np.array_equal(before[k], after[k], equal_nan=before[k].dtype.kind == 'f'), k
        # a host respawn without path arrays: row 1 (it holds a list now) goes back to its policy's own v_pref, row 0 had none
        ids = np.array([0, 1], np.int32)
        m = dict(pos=sc['start'][ids] + [0.0, 0.0, 2.0], vel=np.zeros((2, 3), np.float32), heading=np.zeros((2, 3)), radius=np.full(2, 0.5), pref_speed=np.ones(2),
                 goal=sc['goal'][ids], max_run_dist=np.full(2, 100.0))
        for sol in (A, B):
            sol.respawn(ids, m['pos'], m['vel'], m['heading'], m['radius'], m['pref_speed'], m['goal'], m['max_run_dist'])
        tw.host_respawn(ids)
        for t in range(3):
            served = tw.running.copy()
            A.run_steps(1, S.NBR_KDTREE)
            res = tw.step(S.NBR_KDTREE)
            same(A, B, tw, ('exchange', 'behind the respawn', t), served, False, res)
            same_lists(A, B, ('exchange', 'behind the respawn', t))
        assert A.get_path_state()[0][:2].tolist() == [0, 0]
    finally:
        A.close()
        B.close()


# ---- refusals and lifecycle ------------------------------------------------------------------------------------------------------------------
def test_refusals_and_lifecycle(S, oracle, row_env):
    """every refusal of sca_set_missions_paths with its code and message, the context unchanged; block form; no slot form with offsets;
    sca_set_paths(None) under standing lists; sca_set_missions with lists still refused; dropping; sca_set_state under standing tables"""
    import sca_amd._lib as _lib
    row_env(None)
    scene = F.random_scene(5)
    n = scene['n']
    run = PR.oracle_run(oracle, scene)
    ent, fok, ffail = run['entries'], run['first_ok'], run['first_fail']
    off, pts = S.paths_csr(PR.flat_lists(run['lists']))
    ip = lambda a: None if a is None else _lib.ptr(a, C.c_int32)
    dp = lambda a: None if a is None else _lib.ptr(a, C.c_double)
    keep = []

    def raw(sol, M=MR.M, R=2, n_=n, entries=ent, first_ok=fok, first_fail=ffail, offsets=off, points=pts):
        e = None if entries is None else np.ascontiguousarray(entries).reshape(-1)
        o = None if offsets is None else np.ascontiguousarray(offsets, np.int32)
        p = None if points is None else np.ascontiguousarray(points, np.float64)
        keep.append((e, o, p))
        rc = sol.L.sca_set_missions_paths(sol.ctx, M, R, n_, None if e is None else e.ctypes.data_as(C.POINTER(_lib.Mission)), ip(first_ok), ip(first_fail), ip(o), dp(p))
        return rc, sol.L.sca_last_error(sol.ctx).decode()

    def unchanged(sol, before, what, missions=True, plain=True):
        after = snapshot(sol, missions, plain)
        after['rem'], after['ng'] = sol.get_path_state()
        for k in before:
            assert np.array_equal(before[k], after[k], equal_nan=before[k].dtype.kind == 'f'), (what, k)

    def snap(sol, missions=True, plain=True):
        out = snapshot(sol, missions, plain)
        out['rem'], out['ng'] = sol.get_path_state()
        return out
    reach = np.flatnonzero(fok >= 0)
    a0 = int(reach[0])
    fe = MR.M * a0 + int(fok[a0])                                           # a reachable flat entry
    sol = context_of(S, scene)
    try:
        # no lists at all: with offsets SCA_ERR_STATE; without, the call is sca_set_missions
        rc, msg = raw(sol)
        assert rc == ERR_STATE and 'sca_set_missions_paths' in msg and 'slot form' in msg, (rc, msg)
        assert sol.L.sca_get_mission_paths(sol.ctx, C.byref(C.c_int()), C.byref(C.c_int64())) == ERR_STATE      # no tables
        assert raw(sol, offsets=None, points=None)[0] == 0
        assert sol.mission_paths() == (0, 0) and sol.mission_totals()['updates'] == 0
        assert sol.L.sca_get_mission_paths(sol.ctx, None, None) == ERR_ARG
        sol.set_missions(0, 0, None, None, None)
        # block form
        sol.set_paths([[] for _ in range(n - 1)] + [[[1.0, 2.0, 3.0]]])
        for kw in (dict(), dict(offsets=None, points=None)):
            rc, msg = raw(sol, **kw)
            assert rc == ERR_UNSUPPORTED and 'waypoint' in msg, (rc, msg)
        sol.set_paths(None)
        # slot form: every refusal, the context unchanged
        sol.set_path_slots(W, run['initial'])
        sol.set_vpref(scene['vpref'], scene['vmode'])
        sol.run_steps(2, S.NBR_KDTREE)
        sol.synchronize()
        before = snap(sol, False)
        with pytest.raises(S.ScaError, match='waypoint'):                  # sca_set_missions itself keeps refusing lists
            sol.set_missions(MR.M, 2, ent, fok, ffail)
        unchanged(sol, before, 'sca_set_missions', False)

        lowered = off.copy()
        lowered[7] = lowered[6] - 1                                          # entry 6 ends in front of its own start
        long_off = off.copy()
        long_off[fe + 1:] += W + 1 - (off[fe + 1] - off[fe])
        long_pts = np.zeros((int(long_off[-1]), 3))
        nan_pts = pts.copy()
        grown = off.copy()
        if off[fe + 1] == off[fe]:                                          # (the reachable entry needs a point to spoil)
            grown[fe + 1:] += 1
            nan_pts = np.zeros((int(grown[-1]), 3))
        nan_pts[grown[fe]] = np.nan
        bad_e = ent.copy()
        bad_e['goal'][a0, fok[a0]] = np.nan
        cases = [('M 0', dict(M=0), ERR_ARG, 'M must be'), ('n', dict(n_=n - 1), ERR_ARG, 'agent count'), ('NULL entries', dict(entries=None), ERR_ARG, 'NULL'),
                 ('nan goal', dict(entries=bad_e), ERR_ARG, 'not finite'), ('offsets[0]', dict(offsets=off + 1), ERR_ARG, 'path_offsets[0]'),
                 ('decreasing', dict(offsets=lowered), ERR_ARG, 'decrease'),
                 ('NULL points', dict(points=None), ERR_ARG, 'path_points is NULL'), ('too long', dict(offsets=long_off, points=long_pts), ERR_ARG, 'longer than the room'),
                 ('nan point', dict(offsets=grown, points=nan_pts), ERR_ARG, 'waypoint that is not finite')]
        for what, kw, code, word in cases:
            rc, msg = raw(sol, **kw)
            assert rc == code and 'sca_set_missions_paths' in msg and word in msg, (what, rc, msg)
            unchanged(sol, before, what, False)
        sol.policy_pass(S.NBR_KDTREE)
        assert raw(sol)[0] == ERR_STATE                                     # between a policy pass and its env update
        sol.env_update()
        sol.synchronize()
        # tables with lists stand
        assert raw(sol)[0] == 0
        sol._missions = (MR.M, 2)
        assert sol.mission_paths() == (W, int(off[-1]))
        sol.run_steps(2, S.NBR_KDTREE)
        sol.synchronize()
        sol.mission_results()
        before = snap(sol)
        for what, call, word in (('sca_set_paths', lambda: sol.set_paths(None), 'rooms away'),
                                 ('sca_set_paths', lambda: sol.set_paths([[] for _ in range(n - 1)] + [[[1.0, 2.0, 3.0]]]), 'waypoint'),
                                 ('sca_set_path_slots', lambda: sol.set_path_slots(2), 'waypoint'),
                                 ('sca_step_host', lambda: sol.step_host(S.NBR_KDTREE, state=False), 'host owns the state')):
            with pytest.raises(S.ScaError, match=word) as ei:
                call()
            assert '(rc=%d)' % ERR_UNSUPPORTED in str(ei.value) and what in str(ei.value), (what, str(ei.value))
            unchanged(sol, before, what)
        rc, msg = raw(sol, offsets=off + 1)                                  # a refused replacement leaves the standing tables and lists
        assert rc == ERR_ARG
        unchanged(sol, before, 'a refused replacement')
        assert sol.mission_paths() == (W, int(off[-1]))
        # a new state under standing tables with lists: tables, cursors, lists and their cursors stay
        g = sol.get_state()
        sol.set_state(g['pos'], g['vel'], g['heading'], np.zeros(n, np.uint8), g['total_dist'], g['step_num'])
        cursor, ended = sol.mission_state()
        assert np.array_equal(cursor, before['cursor']) and np.array_equal(ended, before['ended'])
        rem, ng = sol.get_path_state()
        assert np.array_equal(rem, before['rem']) and np.array_equal(ng, before['ng'], equal_nan=True)
        sol.run_steps(1, S.NBR_KDTREE)
        # dropping, by either call: the slot form and the rows' current lists stay, and the host follows them again
        rem, ng = sol.get_path_state()
        assert raw(sol, M=0, entries=None)[0] == 0
        with pytest.raises(S.ScaError, match='no mission tables'):
            sol.mission_paths()
        assert sol.path_slots == W
        r2, g2 = sol.get_path_state()
        assert np.array_equal(r2, rem) and np.array_equal(g2, ng, equal_nan=True)
        sol.set_path_state(rem, ng)                                         # (the bound is the lists the takes left)
        sol.run_steps(1, S.NBR_KDTREE)
        assert raw(sol, offsets=None, points=None)[0] == 0                  # slot form, no offsets: every entry brings the empty list
        assert sol.mission_paths() == (W, 0)
        sol.run_steps(3, S.NBR_KDTREE)
        cursor, _ = sol.mission_state()
        rem, _ = sol.get_path_state()
        assert (cursor >= 0).any() and not rem[cursor >= 0].any()
        sol.set_missions(0, 0, None, None, None)
        sol.set_paths(None)                                                 # no tables: clearing the lists is legal again
        assert sol.path_slots == 0
    finally:
        sol.close()


# ---- the Python layers -------------------------------------------------------------------------------------------------------------------
def agent6(E, i, start, goal, policy=None):
    return E.Agent(start_pos=list(start), goal_pos=list(goal), vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=policy or E.RVO3DPolicy, id=i)


def test_mission_table_paths_and_the_env_mirrors(row_env):
    """MissionTable(path=...): refused without MACAEnv(path_slots=W) and above W before any device call; behind the step that takes an
    entry agent.path is the entry's whole list and policy.now_goal None, after the next pass what the passes left"""
    import sca_amd.env as E
    row_env(None)
    n = 4
    start = [[10.0 * i, 0.0, 5.0, 0.0, 0.0, 0.0] for i in range(n)]
    near = [[10.0 * i + 0.25, 0.0, 5.0, 0.0, 0.0, 0.0] for i in range(n)]
    far = [[10.0 * i, 20.0, 5.0, 0.0, 0.0, 0.0] for i in range(n)]
    route = lambda i: [[10.0 * i + 0.5, 12.0, 5.0], [10.0 * i + 0.5, 0.1, 5.0]]        # (the last one stands within the radius: popped at once, then the next)

    def tables(E, k=2):
        return {i: E.MissionTable([agent6(E, i, near[i], far[i])], next_ok=[-1], next_fail=[-1], first_ok=0, first_fail=0, start_here=True,
                                  path=[route(i)[:k] + ([[1.0, 1.0, 1.0]] if k > 2 else [])]) for i in range(n)}
    env = E.MACAEnv()
    try:
        env.set_agents([agent6(E, i, start[i], near[i]) for i in range(n)], obstacles=[])
        with pytest.raises(ValueError, match='path_slots'):
            env.set_missions(tables(E))
        assert env.solver.active_count() >= 0
    finally:
        env.solver.close()
    env = E.MACAEnv(path_slots=2)
    try:
        env.set_agents([agent6(E, i, start[i], near[i]) for i in range(n)], obstacles=[])
        with pytest.raises(ValueError, match='path_slots'):
            env.set_missions(tables(E, 3))
        with pytest.raises(E.S.ScaError, match='no mission tables'):
            env.solver.mission_paths()                                      # (nothing reached the device)
        env.set_missions(tables(E))
        assert env.solver.mission_paths() == (2, 2 * n)
        with pytest.raises(RuntimeError, match='read-only'):                # (the upload would be refused by the library in the middle of a step)
            env.agents[0].path = [[1.0, 2.0, 3.0]]
        took = False
        for _ in range(12):
            env.run_steps(1)
            res = env.mission_results()
            if len(res):
                assert len(res) == n and (res['next'] == 0).all(), res
                took = True
                break
        assert took
        for i in range(n):
            assert env.agents[i].path == route(i) and env.agents[i].policy.now_goal is None, (i, env.agents[i].path)
            assert np.array_equal(env.agents[i].goal_pos, far[i])
        env.run_steps(1)
        rem, ng = env.solver.get_path_state()
        for i in range(n):
            assert env.agents[i].path == route(i)[:int(rem[i])] and rem[i] < 2, (i, rem[i])
            assert np.array_equal(env.agents[i].policy.now_goal, ng[i])
        env.step()                                                          # the stepwise form goes on from there
        assert env.solver.mission_totals()['taken'] == n
    finally:
        env.solver.close()


def routes_world(how, steps, burst=1):
    """32 RVO3D drones on the example's circle with obstacles, the three-entry ping-pong table whose entries bring routes of two waypoints:
    by lifelong.run_lifelong with a next_mission that follows the same table and hands out the same routes, or by lifelong.run_missions"""
    from sca_amd import env as E
    from sca_amd.lifelong import run_lifelong, run_missions
    n = 32
    agents = E.build_circle_agents(n, policy=E.RVO3DPolicy, rad=8.0)
    obstacles = [E.Obstacle(pos=[round(2.5 * math.cos(2 * j * math.pi / 8), 2), round(2.5 * math.sin(2 * j * math.pi / 8), 2), 10.0],
                            shape_dict={'shape': 'sphere', 'feature': 0.3}, id=j) for j in range(8)]
    first = {a.id: (list(a.initial_pos), list(a.goal_pos)) for a in agents}
    route = {}
    for i, (s, g) in first.items():
        p, q = np.asarray(s[:3]), np.asarray(g[:3])
        side = np.array([-(q - p)[1], (q - p)[0], 0.0]) / max(1e-9, float(np.linalg.norm((q - p)[:2])))
        route[i] = [[float(x) for x in np.round(p + (q - p) * f + side * 1.5, 3)] for f in (0.3, 0.7)]
    out, back = {i: r[::-1] for i, r in route.items()}, {i: r[:] for i, r in route.items()}
    for a in agents:
        a.path = [w[:] for w in out[a.id]]
    env = E.MACAEnv(path_slots=2)
    env.set_agents(agents, obstacles=obstacles)
    T = {i: E.MissionTable([agent6(E, i, g, s), agent6(E, i, s, g), agent6(E, i, s, g)], next_ok=[1, 0, 0], next_fail=[2, 2, 2], first_ok=0, first_fail=2,
                           start_here=[True, True, False], path=[back[i], out[i], out[i]]) for i, (s, g) in first.items()}
    if how == 'host':
        state = {i: -1 for i in first}

        def next_mission(a, row):
            f = int(row['flags'])
            arrived = bool(f & 1) and not f & 2
            j = (T[a.id].first_ok if arrived else T[a.id].first_fail) if state[a.id] < 0 else (T[a.id].next_ok[state[a.id]] if arrived else T[a.id].next_fail[state[a.id]])
            state[a.id] = j
            src, here, _ = T[a.id].entries[j]
            new = agent6(E, a.id, list(row['pos']) + list(a.heading_global_frame) if here else list(src.initial_pos), src.goal_pos)
            new.max_run_dist = src.max_run_dist
            new.path = [w[:] for w in T[a.id].paths[j]]
            return new
        stats = run_lifelong(env, next_mission, steps)
    else:
        stats = run_missions(env, T, steps, burst=burst)
    got = env.solver.get_state(), env.solver.get_path_state(), [list(a.path) for a in env.agents]
    env.solver.close()
    return stats, got


def test_run_missions_against_run_lifelong_with_routes(row_env):
    """run_missions with tables whose entries bring routes, at burst 1 and 8: run_lifelong's stats, final state, list cursors and agent.path"""
    row_env(None)
    want, (state, (rem, ng), paths) = routes_world('host', 400)
    assert want['respawned'] >= 32 and want['retired'] == 0, want
    for burst in (1, 8):
        got, (g, (r2, n2), p2) = routes_world('device', 400, burst)
        assert got == want, (burst, got, want)
        for k in state:
            assert np.array_equal(g[k], state[k]), (burst, k)
        assert np.array_equal(r2, rem) and np.array_equal(n2, ng, equal_nan=True), burst
        assert p2 == paths, burst


def test_the_example_takes_waypoints(row_env):
    """examples/run_sca.py --lifelong --device-missions --waypoints as a fresh child process, plain and with a burst and the gate"""
    row_env(None)
    base = [sys.executable, os.path.join(ROOT, 'examples', 'run_sca.py'), '--scenario', 'circle', '--agents', '32', '--policy', 'orca', '--no-obstacles', '--lifelong', '120']
    for extra in (['--device-missions', '--waypoints', '2', '--burst', '8', '--spawn-margin', '0.5'], ['--waypoints', '2']):
        out = subprocess.run(base + extra, capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        assert 'lifelong: 120 steps' in out.stdout and 'missions' in out.stdout, out.stdout[-2000:]
