"""Waypoint lists in slot form and restarts that bring lists (-m gpu): sca_set_path_slots, sca_get_path_slots, sca_restart_scenes_paths,
SceneBatch(path_slots=...) and run_episodes(path_slots=...).

In slot form every agent row owns room for W waypoints, so a restarted slot can take the episode's own Agent.path lists.  What is held here:
the slot form computes what the block form (sca_set_paths) computes, without scenes and in every step form; recorded F19 episodes run
through slots that are refilled in flight and when they finish, each against the reference's records of the episode the slot holds; a
restarted scene is bit for bit a context of that episode alone after sca_set_agents + sca_set_paths + sca_set_state, and no other scene
can tell the call happened; rows that change their kind; every refusal leaves the context as it was; and the Python layers.  Every
comparison is array_equal (equal_nan only for now_goal and v_pref)."""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import form_fuzz as F
import scene_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5
MIX = [0, 1, 2, 3, 4, 5]
PATH_FIXTURES = ('F19_path_rvo_circle16', 'F19_path_orcalp_random30', 'F19_path_srvo_circle16', 'F19_path_orca_circle16_obs', 'F19_path_edge10')


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


def path_state(sol):
    rem, ng = sol.get_path_state()
    return dict(remaining=rem, now_goal=ng)


def whole(sol, trk=()):
    """scene_util.everything plus what is left of every list and now_goal"""
    out = U.everything(sol, trk)
    out.update(path_state(sol))
    return out


def load_fx(name):
    return U.load_any(('paths/' + name) if name in PATH_FIXTURES else name)


def lists_of(fx):
    """a recorded episode's lists (none: an episode recorded without any)"""
    n = len(fx['radius'])
    if 'path_off' not in fx:
        return [[] for _ in range(n)]
    off, pts = fx['path_off'], fx['path_pts']
    return [[list(map(float, pts[k])) for k in range(off[i], off[i + 1])] for i in range(n)]


# ---- 1: the slot form equals the block form, without scenes ----------------------------------------------------------------------------------
CORPUS = [(seed, per) for seed, per in [(s, False) for s in range(0, 8)] + [(s, True) for s in range(1000, 1004)]
          if F.random_scene(seed)['n'] <= 400]                     # plain path-fuzz seeds 0-7, per-agent seeds 1000-1003: the scenes of at most 400 agents


def corpus_scene(seed, per_agent):
    s = F.random_scene(seed)
    return s, F.random_paths(seed, s), (F.per_agent_attributes(seed, s['n']) if per_agent else None)


def two_forms(S, s, lists, per, W, state=True):
    """(block, slots): two contexts of the same scene, the lists through sca_set_paths and through sca_set_path_slots"""
    from test_gpu_form_fuzz import context_of
    block = context_of(S, s, per, lists, state=state)
    try:
        slots = context_of(S, s, per, None, state=state)
        slots.set_path_slots(W, lists)
    except BaseException:
        block.close()
        raise
    assert block.path_slots == 0 and slots.path_slots == W
    return block, slots


def assert_forms_equal(S, block, slots, at):
    for x in (block, slots):
        assert x.pass_forms() & S.FORM_WAYPOINTS, at + ('FORM_WAYPOINTS',)
    assert block.pass_forms() == slots.pass_forms(), at + ('forms', block.pass_forms(), slots.pass_forms())
    U.same(whole(block), whole(slots), at, nan_keys=('vpref', 'now_goal'))


def longest(lists):
    return max([1] + [len(p) for p in lists])


@pytest.mark.parametrize('seed,per_agent', CORPUS)
def test_slot_form_equals_block_form(S, seed, per_agent):
    """six resident kd steps of a corpus scene of at most 400 agents in both forms; W the longest list, or three more on the odd seeds"""
    s, lists, per = corpus_scene(seed, per_agent)
    W = longest(lists) + 3 * (seed % 2)
    block, slots = two_forms(S, s, lists, per, W)
    try:
        before = path_state(slots)
        assert np.array_equal(before['remaining'], [len(p) for p in lists]) and np.isnan(before['now_goal']).all()
        popped = 0
        for t in range(6):
            U.step_all(S, block, slots)
            assert_forms_equal(S, block, slots, ('seed', seed, 'step', t))
            popped = int((before['remaining'] - path_state(slots)['remaining']).sum())
        assert popped > 0 or not any(lists), ('nothing popped', seed)
    finally:
        block.close(), slots.close()


def test_the_corpus_scenes_that_run():
    """(CORPUS is cut by the scenes' sizes alone: a change of the corpus must not empty it)"""
    assert len(CORPUS) >= 6 and any(per for _, per in CORPUS) and any(not per for _, per in CORPUS), CORPUS


@pytest.mark.parametrize('form', ['auto_burst3', 'grid', 'step_host', 'shard'])
def test_slot_form_equals_block_form_in_every_step_form(S, form):
    """seed 28 (100 agents, 30 obstacles, lists of 0-5): SCA_NBR_AUTO in bursts of three steps, SCA_NBR_GRID, sca_step_host, and one policy
    pass on the shard [33, 83) inside the swarm"""
    s, lists, _ = corpus_scene(28, False)
    n, W = s['n'], longest(lists) + 1
    assert n == 100 and any(len(p) == 5 for p in lists)
    block, slots = two_forms(S, s, lists, None, W, state=form != 'step_host')
    try:
        if form == 'auto_burst3':
            for c in range(2):
                for x in (block, slots):
                    x.run_steps(3, S.NBR_AUTO)
                    x.synchronize()
                assert_forms_equal(S, block, slots, (form, 'call', c))
        elif form == 'grid':
            for t in range(6):
                for x in (block, slots):
                    x.run_steps(1, S.NBR_GRID)
                    x.synchronize()
                assert_forms_equal(S, block, slots, (form, 'step', t))
        elif form == 'step_host':
            blocks = []
            for x in (block, slots):
                blk = x.host_state()
                for k in ('pos', 'vel', 'heading', 'flags'):
                    blk[k][...] = s[k]
                blk['total_dist'][:] = 0.0
                blk['step_num'][:] = 0
                blk['vpref'][...] = s['vpref']
                blk['vpref_mode'][:] = s['vmode']
                x.set_kd_perm(np.arange(n, dtype=np.int32))
                blocks.append(blk)
            for t in range(6):
                active = [x.step_host(S.NBR_KDTREE, state=True, vpref=True) for x in (block, slots)]
                assert active[0] == active[1], (form, t, active)
                for k in F.STATE_KEYS + ('action',):
                    assert np.array_equal(blocks[0][k], blocks[1][k]), (form, t, 'block', k)
                assert_forms_equal(S, block, slots, (form, 'step', t))
        else:
            lo, hi = 33, 83
            for x in (block, slots):
                x.set_shard(lo, hi - lo)
                x.policy_pass(S.NBR_KDTREE)
            assert_forms_equal(S, block, slots, (form,))
            got, length = path_state(slots), np.array([len(p) for p in lists])
            outside = np.r_[0:lo, hi:n]
            assert (got['remaining'] < length)[lo:hi].any(), (form, 'nobody in the shard popped')
            assert np.array_equal(got['remaining'][outside], length[outside]) and np.isnan(got['now_goal'][outside]).all(), (form, 'a list outside the shard moved')
    finally:
        block.close(), slots.close()


def test_the_edge_episode_free_running_in_slot_form(S):
    """F19_path_edge10 (lists of 0 ... 30, all six policies, the device tracker in the pass) against its records, path_left_* and now_goal_*
    included, the lists in slot form with W = 30: tests/test_gpu_paths.py's loop over a solver whose set_paths is sca_set_path_slots"""
    from test_gpu_paths import load, run_recorded_episode
    seen = []

    class SlotSolver(S.BatchedSolver):
        def set_paths(self, paths):
            self.set_path_slots(30, paths)

        def close(self):
            seen.append(self.path_slots)
            super().close()
    ns = types.SimpleNamespace(**{k: v for k, v in vars(S).items() if not k.startswith('__')})
    ns.BatchedSolver = SlotSolver
    fx = load('F19_path_edge10')
    assert sorted(np.diff(fx['path_off']))[0] == 0 and np.diff(fx['path_off']).max() == 30 and sorted(set(fx['policy'].tolist())) == MIX
    assert run_recorded_episode(ns, 'F19_path_edge10', S.NBR_KDTREE, ('edge10', 'slots')) == len(fx['step'])
    assert seen == [30]


# ---- 2: recorded episodes through refilled slots ----------------------------------------------------------------------------------------------
class PathSlots(U.SizedSlots):
    """B slots of `cap` agent rows, room for W waypoints per row and `ocap` obstacle rows each, the device tracker in the pass; slot s starts
    with the recorded episode names[s] (one sized restart of all slots, which brings their lists and obstacles); restart() gives slots
    other recorded episodes.  Held against the records like scene_util.Slots, and path_left / now_goal before and after each step."""

    def __init__(self, S, names, cap=30, W=30, ocap=8):
        self.S, self.B, self.W = S, len(names), W
        self.names = list(names)
        self.fx = [load_fx(n) for n in names]
        ep = [U.recorded_arrays(f) for f in self.fx]
        self.tracker, self.obstacles = True, None
        self.sol, self.off = U.context(S, [U.padded(e, cap) for e in ep], obs_slots=[ocap] * self.B)
        self.sol.set_path_slots(W)
        self.size = np.array([e['n'] for e in ep])
        self.n = int(self.off[-1])
        self.t, self.t0, self.steps_want = 0, [0] * self.B, np.zeros(self.B, np.int64)
        self.path_records = {s: 0 for s in range(self.B)}           # records of the slot's episode at which its lists were compared ...
        self.path_pops = {s: 0 for s in range(self.B)}              # ... and the pops those records hold
        self._send(list(range(self.B)), self.fx, ep)
        self._bind()

    def _send(self, ids, fxs, eps):
        U.restart_all(self.sol, ids, eps, sizes='own', obstacles=[(e['obs_pos'], e['obs_radius']) for e in eps],
                      paths=[p for f in fxs for p in lists_of(f)])

    def restart(self, plan):
        ids = sorted(plan)
        fx = {s: load_fx(plan[s]) for s in ids}
        ep = [U.recorded_arrays(fx[s]) for s in ids]
        self._send(ids, [fx[s] for s in ids], ep)
        for s, e in zip(ids, ep):
            self.fx[s], self.names[s], self.t0[s], self.steps_want[s], self.size[s] = fx[s], plan[s], self.t, 0, e['n']
            self.path_records[s] = self.path_pops[s] = 0
        self._bind()

    def snapshot(self):
        return dict(super().snapshot(), **path_state(self.sol))

    def check_state(self, snap, s, k, when, ctx):
        super().check_state(snap, s, k, when, ctx)
        f, sl = self.fx[s], self.sl(s)
        ctx = ctx + (s, self.names[s], 'record', k, when or 'before')
        if 'path_off' in f:
            suffix = '_after' if when else '_before'
            assert np.array_equal(snap['remaining'][sl], f['path_left' + suffix][k]), ctx + ('path_left',)
            assert np.array_equal(snap['now_goal'][sl], f['now_goal' + suffix][k], equal_nan=True), ctx + ('now_goal',)
            if when and 'inert' not in ctx:
                self.path_records[s] += 1
                self.path_pops[s] += int((f['path_left_before'][k] - f['path_left_after'][k]).sum())
        else:
            assert not snap['remaining'][sl].any(), ctx + ('an episode without lists',)
        vacant = slice(sl.stop, int(self.off[s + 1]))
        assert not snap['remaining'][vacant].any() and np.isnan(snap['now_goal'][vacant]).all(), ctx + ('vacant rows',)


def test_recorded_episodes_through_refilled_slots(S):
    """Three slots of 30 rows, W = 30, obstacle slots of 8.  At batch step 20 slot 0 takes F19_path_srvo_circle16 and slot 2
    F19_path_orca_circle16_obs with its 8 spheres, both in flight; the first slot that finishes takes F19_path_edge10, and when that has
    finished its slot takes F4_sca_takeoff16, an episode without any list.  Conditions: every restarted path episode is compared at >= 40 of
    its records, and those hold >= 13 pops."""
    b = PathSlots(S, ['F19_path_rvo_circle16', 'F19_path_orcalp_random30', 'F1_sca_circle8'])
    done = {}                                                       # episode -> (records, pops) when it left its slot, or at the end
    queue = ['F19_path_edge10', 'F4_sca_takeoff16']

    def leave(s):
        if 'path_off' in b.fx[s]:
            done[b.names[s]] = (b.path_records[s], b.path_pops[s])
    try:
        compared = b.run_and_check(20, label='start')
        assert compared.tolist() == [10, 10, 20]                    # the circles' records are two steps apart
        leave(0), leave(2)
        b.restart({0: 'F19_path_srvo_circle16', 2: 'F19_path_orca_circle16_obs'})
        slot, last = None, None                                     # the slot that is refilled; steps the last episode has run
        for _ in range(700):                                        # (bounded: the three episodes in a row take some 480 batch steps)
            b.run_and_check(1, label='stream')
            if last is not None:
                last += 1
                if last >= 24:
                    break
                continue
            active = b.sol.scene_state()['active']
            if slot is None and (active[[0, 2]] == 0).any():
                slot = 0 if active[0] == 0 else 2
            if slot is not None and active[slot] == 0:
                leave(slot)
                b.restart({slot: queue.pop(0)})
                last = None if queue else 0
        assert not queue and last == 24, (queue, slot, last, b.t)
        for s in range(3):
            leave(s)
        for name in ('F19_path_srvo_circle16', 'F19_path_orca_circle16_obs', 'F19_path_edge10'):
            records, pops = done[name]
            assert records >= 40 and pops >= 13, (name, records, pops)
        assert done['F19_path_rvo_circle16'][0] == 10 and done['F19_path_orcalp_random30'][0] >= 40
    finally:
        b.sol.close()


# ---- 3: the contract against contexts alone ----------------------------------------------------------------------------------------------------
def seeded_lists(ep, seed, W):
    """lists for a synthetic episode, deterministic per seed: lengths 0, 1 and exactly W on the first rows, then drawn from 0 .. W; waypoints
    of form_fuzz.random_paths' five kinds (within the radius, behind, ahead, the goal, around the radius' edge), rounded to 3 places"""
    rng = np.random.default_rng(7000 + seed)
    out = []
    for i in range(ep['n']):
        p, g, r = ep['pos'][i], ep['goal'][i], float(ep['radius'][i])
        d = float(np.linalg.norm(g - p))
        u = (g - p) / d if d > 0 else np.zeros(3)
        k = (W, 0, 1)[i] if i < 3 else int(rng.integers(0, W + 1))
        lst = []
        for _ in range(k):
            kind = int(rng.integers(0, 5))
            w = (p + u * rng.uniform(0, r + 0.8) + rng.normal(0, 0.05, 3) if kind == 0 else p - u * rng.uniform(0.5, 5) if kind == 1
                 else p + (g - p) * rng.uniform(0.1, 0.9) + rng.normal(0, 1, 3) if kind == 2 else g if kind == 3 else p + rng.normal(0, r, 3))
            lst.append([float(x) for x in np.round(w, 3)])
        out.append(lst)
    return out


def episode(S, n, seed, W=5, policy=MIX, lists=True, near_goal=False, rad=None):
    e = U.circle_scene(S, n, np.resize(np.asarray(policy, np.uint8), n), rad=rad, turn=seed)
    if near_goal:
        e['goal'] = e['pos'] + [0.2, 0.0, 0.0]
    e.update(obs_pos=np.zeros((0, 3)), obs_radius=np.zeros(0))
    e['paths'] = seeded_lists(e, seed, W) if lists else [[] for _ in range(n)]
    return e


ARRAYS = ('n', 'pos', 'heading', 'vel', 'radius', 'pref_speed', 'goal', 'policy', 'zaxis', 'max_run_dist', 'goal_heading')


def alone(S, e, tracker=True, paths=True, log=0):
    """the contract's context: sca_set_agents + sca_set_paths(those lists) + sca_set_state (+ the tracker); paths=False: a context that never
    had sca_set_paths"""
    sol = S.BatchedSolver(max_agents=e['n'], max_obstacles=1)
    sol.set_agents(e['radius'], e['pref_speed'], e['goal'], e['policy'], e['zaxis'], e['max_run_dist'])
    sol.set_scenes(np.array([0, e['n']], np.int32))
    if paths:
        sol.set_paths(e['paths'])
    sol.set_state(e['pos'], e['vel'], e['heading'], np.zeros(e['n'], np.uint8))
    if tracker:
        sol.device_tracker_enable(e['goal_heading'], in_pass=True)
    if log:
        sol.scene_history_enable(log)
    return sol


def send(sol, ids, eps, tracker=True, paths='own', **kw):
    U.restart_all(sol, ids, [{k: e[k] for k in ARRAYS} for e in eps], sizes='own', tracker=tracker,
                  paths=[p for e in eps for p in e['paths']] if paths == 'own' else paths, **kw)


def batch_of(S, base, cap, W, tracker=True, log=0, harvest=False):
    """len(base) slots of `cap` rows holding base[s], the lists in slot form with room for W: a full batch of padded episodes,
    sca_set_path_slots, and ONE restart of all slots that brings the episodes and their lists"""
    sol, off = U.context(S, [U.padded({k: e[k] for k in ARRAYS}, cap) for e in base], tracker=tracker)
    sol.set_path_slots(W)
    if log:
        sol.scene_history_enable(log)
    if harvest:
        sol.scene_harvest_enable()
    send(sol, list(range(len(base))), base, tracker)
    return sol, off


def assert_slot_equals_alone(got, off, s, e, x, ctx, paths=True, tracker=True):
    lo, trk = int(off[s]), (U.tracked(e) if tracker else ())
    hi = lo + e['n']
    U.assert_scene_equals_alone(got, lo, hi, 0, U.everything(x, trk), ctx + ('slot', s))
    if paths:
        want = path_state(x)
        assert np.array_equal(got['remaining'][lo:hi], want['remaining']), ctx + ('slot', s, 'remaining')
        assert np.array_equal(got['now_goal'][lo:hi], want['now_goal'], equal_nan=True), ctx + ('slot', s, 'now_goal')
    else:                                                          # a context without lists has no path state: the slot's rows have empty lists,
        assert not got['remaining'][lo:hi].any(), ctx + ('slot', s, 'remaining')       # and now_goal is the goal once the row was served
    vac = slice(hi, int(off[s + 1]))
    assert not got['remaining'][vac].any() and np.isnan(got['now_goal'][vac]).all(), ctx + ('slot', s, 'vacant rows')


STEP_FORMS = {'run_steps_1': (1, lambda S, x: (x.run_steps(1, S.NBR_KDTREE), x.synchronize())),
              'run_steps_3': (3, lambda S, x: (x.run_steps(3, S.NBR_KDTREE), x.synchronize())),
              'env_step': (1, lambda S, x: x.env_step(S.NBR_KDTREE))}


@pytest.mark.parametrize('form', list(STEP_FORMS))
def test_a_restarted_scene_is_its_context_alone(S, form):
    """Slots of 130 rows, W = 5, holding circles of 1 (it finishes in its first step), 63, 64, 65 and 129 agents with seeded lists of
    0 .. W waypoints.  After two steps ONE call restarts three slots in flight: the finished slot 0 takes 65 agents on top of its vacant
    rows, slot 1 grows from 63 to 129, slot 4 shrinks from 129 to 63.  Over six steps each named slot equals its context alone in every
    value of the contract; slots 2 and 3 equal a twin batch that never saw the call; vacant rows read remaining 0 and now_goal None.  The
    log per scene and the harvest are on."""
    k, step = STEP_FORMS[form]
    W, cap = 5, 130
    base = [episode(S, 1, 0, near_goal=True), episode(S, 63, 1), episode(S, 64, 2), episode(S, 65, 3), episode(S, 129, 4)]
    assert {len(p) for e in base[1:] for p in e['paths']} == set(range(W + 1))
    new = {0: episode(S, 65, 10), 1: episode(S, 129, 11), 4: episode(S, 63, 12)}
    rows = 2 + 6 * k
    sol, off = batch_of(S, base, cap, W, log=rows, harvest=True)
    twin, _ = batch_of(S, base, cap, W, log=rows, harvest=True)
    solos = {}
    try:
        for _ in range(2):
            U.step_all(S, sol, twin)
        assert sol.scene_state()['active'][0] == 0 and sol.scene_harvest_collect() == [0]
        before = whole(sol)
        send(sol, sorted(new), [new[s] for s in sorted(new)])
        solos = {s: alone(S, e, log=rows) for s, e in new.items()}
        assert np.array_equal(sol.scene_sizes(), [65, 129, 64, 65, 63])
        at_call = whole(sol)
        for s, e in new.items():                                   # directly behind the call: what sca_set_paths + sca_set_state leave
            lo = int(off[s])
            assert np.array_equal(at_call['remaining'][lo:lo + e['n']], [len(p) for p in e['paths']]), ('at the call', s)
            assert not at_call['remaining'][lo + e['n']:int(off[s + 1])].any() and np.isnan(at_call['now_goal'][lo:int(off[s + 1])]).all(), ('at the call', s)
        others = slice(int(off[2]), int(off[4]))
        for key in before:                                          # no other scene can tell the call happened
            if key != 'track':
                assert np.array_equal(before[key][others], at_call[key][others], equal_nan=True), ('at the call', 'slots 2, 3', key)
        for t in range(6):
            step(S, sol), step(S, twin)
            for x in solos.values():
                step(S, x)
            ctx = (form, 'step', t)
            got = whole(sol, [int(off[s]) + a for s, e in new.items() for a in U.tracked(e)])
            for s, e in new.items():
                assert_slot_equals_alone(got, off, s, e, solos[s], ctx)
            U.assert_vacant(got, off, [65, 129, 64, 65, 63], ctx)
            want = whole(twin)
            for key in want:
                if key != 'track':
                    assert np.array_equal(got[key][others], want[key][others], equal_nan=True), ctx + ('slots 2, 3 against the twin', key)
            assert np.array_equal(sol.scene_state()['steps'][[2, 3]], twin.scene_state()['steps'][[2, 3]]), ctx
        popped = sum(int(sum(len(p) for p in e['paths']) - path_state(solos[s])['remaining'].sum()) for s, e in new.items())
        assert popped >= 20, ('the restarted scenes hardly popped', popped)
        for s, x in solos.items():                                  # the log per scene starts over with the episode
            a, w = sol.scene_history(s), x.scene_history(0)
            assert len(w['pos']) == 6 * k
            for key in w:
                assert np.array_equal(a[key], w[key]), ('log per scene', s, key)
    finally:
        for x in [sol, twin] + list(solos.values()):
            x.close()


def test_step_host_behind_a_restart_with_lists(S):
    """sca_step_host wants every slot full: three slots of 40, W = 4; one call restarts slots 0 and 2 with lists, slot 1 keeps running"""
    W = 4
    base = [episode(S, 40, s, W=W, rad=9.0) for s in range(3)]
    new = {0: episode(S, 40, 20, W=W, rad=9.0), 2: episode(S, 40, 21, W=W, rad=9.0, near_goal=True)}
    sol, off = batch_of(S, base, 40, W, log=6, harvest=True)
    held = {0: new[0], 1: base[1], 2: new[2]}
    solos = {}
    try:
        sol.host_state()
        send(sol, [0, 2], [new[0], new[2]])
        solos = {s: alone(S, e, log=6) for s, e in held.items()}
        for t in range(4):
            active = sol.step_host(S.NBR_KDTREE, state=False)
            U.step_all(S, *solos.values())
            got = whole(sol, [int(off[s]) + a for s, e in held.items() for a in U.tracked(e)])
            for s, e in held.items():
                assert_slot_equals_alone(got, off, s, e, solos[s], ('step_host', t))
            blk = sol.host_state()
            for key in ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num'):
                assert np.array_equal(blk[key], got[key]), ('block against the device state', t, key)
            assert active == sol.active_count() == int(((got['flags'] & 7) == 0).sum())
            if t == 0:
                assert sol.scene_harvest_collect() == [2]           # the near-goal episode finished in its first step
        for s, x in solos.items():
            a, w = sol.scene_history(s), x.scene_history(0)
            for key in w:
                assert np.array_equal(a[key], w[key]), ('log per scene', s, key)
    finally:
        for x in [sol] + list(solos.values()):
            x.close()


# ---- 4: rows that change their kind --------------------------------------------------------------------------------------------------------------
def run_against_alone(S, sol, off, held, solos, steps, label, paths=True, tracker=True):
    for t in range(steps):
        U.step_all(S, sol, *solos.values())
        got = whole(sol, [int(off[s]) + a for s, e in held.items() for a in U.tracked(e)] if tracker else ())
        for s, e in held.items():
            assert_slot_equals_alone(got, off, s, e, solos[s], (label, 'step', t), paths=paths if isinstance(paths, bool) else paths[s], tracker=tracker)


def test_a_straight_line_row_loses_its_list_and_gets_one_back(S):
    """slot 0: RVO3D / ORCA3D rows with lists -> the same rows without any -> with lists again; each time the slot is its context alone,
    v_pref included: k_waypoint_slots stops feeding a row whose list is gone (vpref_mode is reset by the restart) and feeds it again"""
    W = 3
    with_lists = episode(S, 24, 1, W=W, policy=[1, 3, 2, 4], rad=6.0)
    without = dict(with_lists, paths=[[] for _ in range(24)])
    other = episode(S, 24, 2, W=W, policy=[1, 3, 2, 4], rad=6.0)
    sol, off = batch_of(S, [with_lists, other], 24, W, tracker=False)
    solos = {0: alone(S, with_lists, tracker=False), 1: alone(S, other, tracker=False)}
    try:
        held = {0: with_lists, 1: other}
        run_against_alone(S, sol, off, held, solos, 3, 'with lists', tracker=False)
        for label, e in (('without', without), ('with lists again', with_lists)):
            send(sol, [0], [e], tracker=False)
            solos[0].close()
            solos[0], held[0] = alone(S, e, tracker=False), e
            run_against_alone(S, sol, off, held, solos, 3, label, tracker=False)
    finally:
        for x in [sol] + list(solos.values()):
            x.close()


def test_a_tracked_row_with_a_list_becomes_an_untracked_row_with_a_list(S):
    """through `attrs` (a policy may then move a row between tracked and untracked): SCA rows with lists -> RVO3D rows with lists, whose
    v_pref k_waypoint_slots now writes, and back"""
    W = 3
    sca = episode(S, 20, 1, W=W, policy=[0, 5], rad=6.0)
    rvo = dict(episode(S, 20, 1, W=W, policy=[1, 3], rad=6.0), paths=sca['paths'])
    other = episode(S, 20, 2, W=W, policy=MIX, rad=6.0)
    sol, off = batch_of(S, [sca, other], 20, W)
    solos = {0: alone(S, sca), 1: alone(S, other)}
    try:
        held = {0: sca, 1: other}
        run_against_alone(S, sol, off, held, solos, 2, 'tracked')
        for label, e in (('untracked', rvo), ('tracked again', sca)):
            send(sol, [0], [e], attrs={})
            solos[0].close()
            solos[0], held[0] = alone(S, e), e
            run_against_alone(S, sol, off, held, solos, 3, label)
    finally:
        for x in [sol] + list(solos.values()):
            x.close()


def test_a_restart_without_path_arrays_gives_empty_lists(S):
    """sca_restart_scenes proper on a context in slot form: the named rows get empty lists, and the scene equals a context alone that
    never had sca_set_paths"""
    W = 3
    base = [episode(S, 24, s, W=W, policy=[1, 3, 2, 4], rad=6.0) for s in range(2)]
    sol, off = batch_of(S, base, 24, W, tracker=False)
    bare = episode(S, 24, 5, W=W, policy=[1, 3, 2, 4], rad=6.0, lists=False)
    solos = {}
    try:
        U.step_all(S, sol, k=2)
        assert (path_state(sol)['remaining'][:24] > 0).any()
        U.restart_all(sol, [0], [{k: bare[k] for k in ARRAYS}], tracker=False)          # no sizes, no obstacles, no attrs, no paths: sca_restart_scenes
        got = path_state(sol)
        assert not got['remaining'][:24].any() and np.isnan(got['now_goal'][:24]).all()
        solos = {0: alone(S, bare, tracker=False, paths=False)}
        run_against_alone(S, sol, off, {0: bare}, solos, 4, 'no lists', paths=False, tracker=False)
        assert np.array_equal(path_state(sol)['now_goal'][:24], bare['goal'])          # served rows with an empty list aim at their goal
    finally:
        for x in [sol] + list(solos.values()):
            x.close()


# ---- 5: refusals -------------------------------------------------------------------------------------------------------------------------------------
def raw_restart(sol, e, path_off, path_pts, scene=0):
    """sca_restart_scenes_paths itself, with the path arrays as given"""
    from sca_amd import _lib
    keep = [np.array([scene], np.int32), np.array([e['n']], np.int32), np.ascontiguousarray(e['pos'], np.float64), np.ascontiguousarray(e['heading'], np.float64)]
    po = None if path_off is None else np.ascontiguousarray(path_off, np.int32)
    pp = None if path_pts is None else np.ascontiguousarray(path_pts, np.float64)
    return sol.L.sca_restart_scenes_paths(sol.ctx, 1, _lib.ptr(keep[0], C.c_int32), _lib.ptr(keep[1], C.c_int32), None, None, None, None,
                                          None if po is None else _lib.ptr(po, C.c_int32), None if pp is None else _lib.ptr(pp, C.c_double),
                                          _lib.ptr(keep[2], C.c_double), None, _lib.ptr(keep[3], C.c_double), None, None, None, None, None, None, None)


def test_refusals_leave_the_context_as_it_was(S):
    from sca_amd import _lib
    W = 3
    base = [episode(S, 12, s, W=W, policy=[1, 3, 0], rad=4.0) for s in range(2)]
    sol, off = batch_of(S, base, 12, W)
    e = episode(S, 12, 9, W=W, policy=[1, 3, 0], rad=4.0)
    poff, ppts = S.paths_csr(e['paths'])
    try:
        U.step_all(S, sol, k=2)
        before, seen, lists = whole(sol), U.observe(sol), path_state(sol)
        bad_start, decreasing, too_long = poff.copy(), poff.copy(), poff.copy()
        bad_start[0] = 1
        decreasing[5] = decreasing[4] - 1
        too_long[7:] += W + 1 - (poff[7] - poff[6])                 # row 6 brings W + 1
        long_pts = np.zeros((int(too_long[-1]), 3))
        not_finite = ppts.copy()
        row = int(np.flatnonzero(np.diff(poff) > 0)[2])
        not_finite[poff[row], 1] = np.inf
        cases = [(bad_start, ppts, ERR_ARG, 'path_offsets[0]'), (decreasing, ppts, ERR_ARG, 'row 4'), (too_long, long_pts, ERR_ARG, 'row 6'),
                 (poff, None, ERR_ARG, 'path_points is NULL'), (poff, not_finite, ERR_ARG, 'row %d' % row)]
        for po, pp, code, words in cases:
            assert raw_restart(sol, e, po, pp) == code, words
            assert words in sol.L.sca_last_error(sol.ctx).decode(), (words, sol.L.sca_last_error(sol.ctx))
        # sca_set_path_slots' own: a refused call changes nothing either -- the context stays in slot form with its lists
        n = 24
        flat = [p for x in base for p in x['paths']]
        o2, p2 = S.paths_csr(flat)
        ip, dp = (lambda a: _lib.ptr(a, C.c_int32)), (lambda a: _lib.ptr(a, C.c_double))
        bad0, dec = o2.copy(), o2.copy()
        bad0[0] = 2
        dec[3] = dec[2] - 1
        inf = p2.copy()
        inf[1, 2] = np.nan
        for args, words in [((0, n, ip(o2), dp(p2)), 'at least 1'), ((-3, n, ip(o2), dp(p2)), 'at least 1'), ((W - 1, n, ip(o2), dp(p2)), 'room for %d' % (W - 1)),
                            ((2 ** 31 - 1, n, ip(o2), dp(p2)), 'not addressable'), ((W, n - 1, ip(o2), dp(p2)), 'agent count'),
                            ((W, n, ip(bad0), dp(p2)), 'offsets[0]'), ((W, n, ip(dec), dp(p2)), 'decrease at agent 2'), ((W, n, ip(o2), None), 'points is NULL'),
                            ((W, n, ip(o2), dp(inf)), 'waypoint 1 is not finite')]:
            assert sol.L.sca_set_path_slots(sol.ctx, *args) == ERR_ARG, words
            assert words in sol.L.sca_last_error(sol.ctx).decode(), (words, sol.L.sca_last_error(sol.ctx))
        assert sol.path_slots == W
        U.same(before, whole(sol), ('after the refusals',), nan_keys=('vpref', 'now_goal'))
        U.same(seen, U.observe(sol), ('after the refusals', 'counters'))
        U.same(lists, path_state(sol), ('after the refusals', 'lists'))
        # sca_set_paths on a slot-form context switches the form back: the block form's refusal of a restart returns
        sol.set_paths(flat)
        assert sol.path_slots == 0
        assert raw_restart(sol, e, None, None) == ERR_UNSUPPORTED
        assert raw_restart(sol, e, poff, ppts) == ERR_UNSUPPORTED
        assert U.rc_of(S, lambda: send(sol, [0], [e])) == ERR_UNSUPPORTED
        sol.set_paths(None)                                         # no lists at all: path arrays are a matter of state
        assert sol.path_slots == 0 and raw_restart(sol, e, poff, ppts) == ERR_STATE
        assert 'slot form' in sol.L.sca_last_error(sol.ctx).decode()
        sol.set_path_slots(W + 2)                                   # ... and back, with more room: the staging block grows
        assert sol.path_slots == W + 2 and raw_restart(sol, e, poff, ppts) == 0
        assert np.array_equal(path_state(sol)['remaining'][:12], np.diff(poff))
    finally:
        sol.close()


def test_the_partition_is_refused_in_slot_form(S):
    """sca_partition_init with lists in slot form: SCA_ERR_UNSUPPORTED, as with sca_set_paths"""
    s, lists, _ = corpus_scene(28, False)
    from test_gpu_form_fuzz import context_of
    sol = context_of(S, s, None, None)
    try:
        sol.set_path_slots(longest(lists), lists)
        assert U.rc_of(S, lambda: sol.partition_init(0, 2)) == ERR_UNSUPPORTED
        assert 'waypoint lists' in sol.L.sca_last_error(sol.ctx).decode()
        assert sol.path_slots == longest(lists)
    finally:
        sol.close()


# ---- 6: Python ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mods():
    from sca_amd import env as E, metrics, scenarios, scenes
    return E, metrics, scenarios, scenes


def drones(E, scenarios, seed, n=16, policy=None, longest_list=3):
    """a circle of n drones of one policy, every drone carrying 0 .. longest_list seeded waypoints around its straight line"""
    pols = [E.SCAPolicy, E.RVO3DPolicy, E.SRVO3DPolicy, E.ORCA3DPolicy, E.ORCA3DPolicyOfficial, E.RVO3dDubinsPolicy]
    sc = scenarios.circle(n, rad=6.0, z=12.0)
    agents = U.agents_of(sc, policy or pols[seed % 6])
    rng = np.random.default_rng(9000 + seed)
    for a, p, g in zip(agents, sc['start'], sc['goal']):
        k = int(rng.integers(0, longest_list + 1))
        a.path = [[float(x) for x in np.round(p[:3] + (g[:3] - p[:3]) * f + rng.normal(0, 0.4, 3), 3)] for f in sorted(rng.uniform(0.1, 0.9, k), reverse=True)]
    return agents


def test_scene_batch_with_path_slots(mods):
    E, metrics, scenarios, scenes = mods
    first = [drones(E, scenarios, s) for s in range(3)]
    batch = scenes.SceneBatch(first, [], device_tracker=True, path_slots='max')
    try:
        assert batch.path_slots == max(len(a.path) for e in first for a in e) == batch.solver.path_slots == 3
        for _ in range(5):
            batch.step()
        new = drones(E, scenarios, 7)
        whole_lists = [list(a.path) for a in new]
        batch.restart({1: new})
        assert [a.path for a in new] == whole_lists and all(a.policy.now_goal is None for a in new)      # until the scene's next pass
        alone_env = E.MACAEnv(device_tracker=True)
        twin = drones(E, scenarios, 7)
        alone_env.set_agents(twin, obstacles=[])
        for t in range(6):
            batch.step(), alone_env.step()
            for a, b in zip(new, twin):
                assert a.path == b.path and np.array_equal(a.pos_global_frame, b.pos_global_frame), (t, a.id)
                ga, gb = a.policy.now_goal, b.policy.now_goal
                assert (ga is None and gb is None) or np.array_equal(ga, gb), (t, a.id)
        # a later assignment keeps working through the slot form, here and in the env alone
        for x in (new[3], twin[3]):
            x.path = [[1.0, 2.0, 12.0], [0.5, 0.5, 12.5]]
        for t in range(4):
            batch.step(), alone_env.step()
            assert new[3].path == twin[3].path and np.array_equal(new[3].pos_global_frame, twin[3].pos_global_frame), t
        assert batch.solver.path_slots == 3
        alone_env.solver.close()
        # a list longer than the room: ValueError before any device call
        before = batch.solver.get_state()
        long_one = drones(E, scenarios, 8)
        long_one[2].path = [[0.0, 0.0, 12.0]] * 4
        with pytest.raises(ValueError):
            batch.restart({0: long_one})
        for k, v in batch.solver.get_state().items():
            assert np.array_equal(before[k], v), k
    finally:
        batch.close()
    with pytest.raises(ValueError):
        scenes.SceneBatch(first, [], path_slots=0)


def test_run_episodes_with_path_slots_equals_one_env_per_episode(mods):
    """12 episodes of 16 drones, the six policies in turn, through 4 slots: metrics, final state and remaining lists"""
    E, metrics, scenarios, scenes = mods
    eps = [drones(E, scenarios, s) for s in range(12)]
    stats, order = {}, []
    got = scenes.run_episodes(eps, 4, device_tracker=True, path_slots='max', on_done=lambda r: order.append(r['episode']), stats=stats, max_steps=20000)
    assert sorted(order) == list(range(12)) and 0.0 < stats['live_fraction'] <= 1.0
    for i in range(12):
        agents = drones(E, scenarios, i)
        env = E.MACAEnv(device_tracker=True)
        env.set_agents(agents, obstacles=[])
        steps = 1
        while not env.step():
            steps += 1
            assert steps < 5000, i
        want, st = metrics.episode_metrics(env), env.solver.get_state()
        assert got[i]['steps'] == steps, (i, got[i]['steps'], steps)
        for key in want:
            if key != 'AverageCost':                                # wall time of the policy calls
                assert np.array_equal(got[i]['metrics'][key], want[key], equal_nan=True), (i, key, got[i]['metrics'][key], want[key])
        for key in got[i]['state']:
            assert np.array_equal(got[i]['state'][key], st[key]), (i, key)
        assert got[i]['path_left'] == [len(a.path) for a in agents], i
        env.solver.close()
    long_one = drones(E, scenarios, 0)
    long_one[0].path = [[0.0, 0.0, 12.0]] * 5
    with pytest.raises(ValueError):                                 # before any batch is built
        scenes.run_episodes([long_one], 1, path_slots=2)


def test_the_example_with_waypoints_runs_to_its_table():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'run_scenes.py'), '--waypoints', '3', '--seeds', '2', '--slots', '4'],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'waypoints' in out.stdout, out.stdout[-3000:]
