"""A restarted slot takes the episode's own attributes (-m gpu): sca_restart_scenes_attrs.  The bar is the scene contract extended to the
attributes: after the call a named scene is bit for bit a context that holds that episode alone after sca_set_agents +
sca_set_agent_params + its obstacles + sca_set_state + sca_device_tracker_enable + sca_device_tracker_set_agent_params -- every read-back
scene_util.everything gathers -- and, where the episode was recorded from the reference, the recording; no other scene can tell the call
happened.  The batches are created with DEFAULT sca_params and a tracker enabled at its default values: every attribute arrives with a
restart.  No tolerance anywhere."""
import math

import numpy as np
import pytest

import form_fuzz as F
from golden_util import fixture_agent_params, fixture_params, fixture_tracker_agent_params
from scene_util import (assert_scene_equals_alone, assert_slots_equal_alone, assert_vacant, circle_scene, context, everything, load_any, loop_summary, observe, padded, rc_of,
                        recorded_arrays, restart_all, same, step_all, tracked)

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5                 # include/sca_hip.h
DEFAULTS = dict(neighbor_dist=10.0, max_neighbors=16, time_step=0.1, time_horizon=10.0, max_speed=1.0, max_heading_change=math.pi / 4, dt_nominal=0.1)
TRK_DEFAULTS = dict(turning_radius=1.5, pitch_lo=-math.pi / 4, pitch_hi=math.pi / 4)
MIX = [0, 1, 2, 3, 4, 5]


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


# ---- episodes with their attributes --------------------------------------------------------------------------------------------------------
_EPISODES = {}


def recorded(name):
    """a recorded episode's arrays (scene_util.recorded_arrays) with `solver` / `planner`: the attributes the reference's agents carried,
    one array per name (fixture_agent_params where they differ from agent to agent, else the scene's one value), and `fx`, the records"""
    if name not in _EPISODES:
        fx = load_any(name)
        e = recorded_arrays(fx)
        n, (scene, trk) = e['n'], fixture_params(fx)
        own, own_trk = fixture_agent_params(fx), fixture_tracker_agent_params(fx)
        e['solver'] = {k: np.asarray(own[k]) if k in own else np.full(n, scene.get(k, d), np.int32 if k == 'max_neighbors' else np.float64)
                       for k, d in DEFAULTS.items()}
        one = dict(turning_radius=trk['turning_radius'], pitch_lo=trk['pitchlims'][0], pitch_hi=trk['pitchlims'][1]) if trk else TRK_DEFAULTS
        e['planner'] = {k: np.asarray(own_trk[k]) if k in own_trk else np.full(n, one[k]) for k in TRK_DEFAULTS}
        e.update(fx=fx, name=name, index={int(t): k for k, t in enumerate(fx['step'])})
        _EPISODES[name] = e
    return _EPISODES[name]


def synthetic(S, n, policy=MIX, rad=None, turn=0, solver=None, planner=None, near_goal=False):
    """a circle episode (no records) with the given attributes; None: the defaults a context alone has.  near_goal: every goal 0.2 m from
    its start -- the episode finishes in its first step"""
    e = circle_scene(S, n, np.resize(np.asarray(policy, np.uint8), n), rad=rad, turn=turn)
    if near_goal:
        e['goal'] = e['pos'] + [0.2, 0.0, 0.0]
    e.update(obs_pos=np.zeros((0, 3)), obs_radius=np.zeros(0), solver=solver, planner=planner, fx=None, name='synthetic', index={})
    return e


AT_CALL = ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num', 'perm', 'nbr_n', 'nbr_valid')
ARRAYS = ('n', 'pos', 'heading', 'vel', 'radius', 'pref_speed', 'goal', 'policy', 'zaxis', 'max_run_dist', 'goal_heading')


def arrays(e):
    """the episode without what this module added: what scene_util.padded copies row by row"""
    return {k: e[k] for k in ARRAYS}


def attrs_of(eps, tracker=True):
    """the `attrs` of one restart call for these episodes, packed in their order; an episode without attributes brings the defaults"""
    out = {}
    for k, d in DEFAULTS.items():
        out[k] = np.concatenate([e['solver'][k] if e['solver'] else np.full(e['n'], d) for e in eps]).astype(np.int32 if k == 'max_neighbors' else np.float64)
    if tracker:
        for k, d in TRK_DEFAULTS.items():
            out[k] = np.concatenate([e['planner'][k] if e['planner'] else np.full(e['n'], d) for e in eps])
    return out


def alone(S, e, tracker=True):
    """the contract's context: this episode alone, its attributes handed over by the two per-agent calls"""
    sol = S.BatchedSolver(max_agents=e['n'], max_obstacles=max(len(e['obs_radius']), 1))
    sol.set_agents(e['radius'], e['pref_speed'], e['goal'], e['policy'], e['zaxis'], e['max_run_dist'])
    if e['solver']:
        sol.set_agent_params(**e['solver'])
    sol.set_scenes(np.array([0, e['n']], np.int32))
    if len(e['obs_radius']):
        sol.set_scene_obstacles([(e['obs_pos'], e['obs_radius'])])
    sol.set_state(e['pos'], e['vel'], e['heading'], np.zeros(e['n'], np.uint8))
    if tracker:
        sol.device_tracker_enable(e['goal_heading'], in_pass=True)
        if e['planner']:
            sol.device_tracker_set_agent_params(**e['planner'])
    return sol


class AttrSlots:
    """B slots of `cap` agent rows and `ocap` obstacle rows in a context with default sca_params; slot s starts full with base[s] (default
    attributes).  put() restarts slots through the new call; run() steps the batch and every slot's context alone, and holds each slot
    against that context and, where there is one, its recording."""

    def __init__(self, S, base, cap, ocap=1, tracker=True):
        self.S, self.tracker, self.cap = S, tracker, cap
        self.sol, self.off = context(S, [padded(arrays(e), cap) for e in base], obs_slots=[ocap] * len(base), tracker=tracker)
        self.obs_lo = [ocap * s for s in range(len(base))]
        self.held, self.solos, self.local = {}, {}, {}
        if any(e['n'] < cap for e in base):
            restart_all(self.sol, list(range(len(base))), base, sizes='own', tracker=tracker)
        for s, e in enumerate(base):
            self._hold(s, e)

    def _hold(self, s, e):
        if s in self.solos:
            self.solos[s].close()
        self.held[s], self.solos[s], self.local[s] = e, alone(self.S, e, self.tracker), 0

    def put(self, plan, attrs='own', **drop):
        """{slot: episode}: ONE restart call; attrs 'own': the episodes' attributes, else what restart_scenes takes ('keep', {}, a dict)"""
        ids = sorted(plan)
        eps = [plan[s] for s in ids]
        restart_all(self.sol, ids, eps, sizes='own', obstacles=[(e['obs_pos'], e['obs_radius']) for e in eps], tracker=self.tracker,
                    attrs=attrs_of(eps, self.tracker) if attrs == 'own' else attrs, **drop)
        for s, e in zip(ids, eps):
            self._hold(s, e)

    def check_at_call(self, named, ctx):
        """directly behind a restart: the named slots are what sca_set_state leaves -- the state, the identity permutation, no lists (action
        rows, diagnostics and list entries are whatever the last step wrote, in the slot as in any context before its first step) --, every
        other slot is its context alone in every value"""
        got = everything(self.sol, [int(self.off[s]) + a for s in self.solos if s not in named for a in tracked(self.held[s])])
        for s, x in self.solos.items():
            lo, fresh = int(self.off[s]), s in named
            want = everything(x, () if fresh else tracked(self.held[s]))
            if fresh:
                want = {k: want[k] for k in AT_CALL}
            assert_scene_equals_alone(got, lo, lo + self.held[s]['n'], self.obs_lo[s], want, ctx + ('at the call', 'slot', s))
        # (the rows a restart has just vacated keep the action row of the last step until the next one: assert_vacant comes behind every step)

    def check(self, ctx):
        got = assert_slots_equal_alone(self.sol, self.off, self.held, self.solos, ctx, self.obs_lo)
        assert_vacant(got, self.off, [self.held[s]['n'] for s in range(len(self.held))], ctx)
        for s, e in self.held.items():                             # the recording: the state behind the episode's step local[s] - 1
            k = e['index'].get(self.local[s] - 1)
            if k is None:
                continue
            fx, lo = e['fx'], int(self.off[s])
            sl = slice(lo, lo + e['n'])
            for key in ('pos', 'heading', 'total_dist', 'flags', 'vel'):
                assert np.array_equal(got[key][sl], fx[key + '_after'][k]), ctx + (s, e['name'], 'record', k, key)
            assert np.array_equal(got['perm'][sl] - lo, fx['perm_after'][k]), ctx + (s, e['name'], 'record', k, 'perm')
            called = fx['called'][k].astype(bool)
            assert np.array_equal(got['action'][sl][called], fx['action'][k][called]), ctx + (s, e['name'], 'record', k, 'action')
            assert not got['status'][sl].any(), ctx + (s, e['name'], 'status')
        return got

    def run(self, steps, label, step_fn=None, k=1):
        """step_fn(solver): k steps of the batch (default: sca_run_steps(1) and a synchronisation)"""
        for t in range(steps):
            if step_fn is None:
                step_all(self.S, self.sol)
            else:
                step_fn(self.sol)
            step_all(self.S, *self.solos.values(), k=k)
            for s in self.local:
                self.local[s] += k
            got = self.check((label, 'step', t))
        return got

    def close(self):
        for x in [self.sol] + list(self.solos.values()):
            x.close()


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------------------
def test_reference_recordings_through_refilled_slots(S):
    """F17 (attributes per agent) and the F16 episodes whose settings are Agent attributes enter slots of a default context: into slots that
    are in flight, into one that has finished, and over each other.  Every step of each is the recording and the context alone."""
    base = [synthetic(S, 60, rad=14.0), synthetic(S, 24, rad=6.0, turn=1), synthetic(S, 12, near_goal=True)] + [synthetic(S, 36, rad=9.0, turn=s) for s in (2, 3, 4)]
    b = AttrSlots(S, base, cap=60, ocap=5)
    b.run(2, 'base')
    assert b.sol.scene_state()['active'][2] == 0                   # slot 2 has finished
    b.put({0: recorded('F17_hetero_circle60'), 1: recorded('F17_hetero_dense40'), 2: recorded('F17_hetero_mixed48'),
           3: recorded('F16_params_nbr4_dense40')})
    b.check_at_call({0, 1, 2, 3}, ('first refill',))
    b.run(5, 'first refill')
    b.put({4: recorded('F16_params_nbr8_far60'), 0: recorded('F16_params_dt005'), 5: recorded('F16_params_timestep02')})
    b.run(5, 'second refill')
    b.put({1: recorded('F16_params_orca_h3_v15'), 3: recorded('F16_params_turn3_sca16')})
    b.run(5, 'third refill')
    b.close()


# ---- 2, 3 -------------------------------------------------------------------------------------------------------------------------------------
def test_first_attributes_in_a_plain_batch_and_back_to_defaults(S):
    """No per-agent array exists before the call.  One scene takes F17 attributes while two others are mid-episode: they are what their
    contexts alone are -- which never saw a call -- at the call and on every later step.  Then the slot takes a default episode through a
    struct whose arrays are all NULL and is a plain context; restarted once more WITHOUT attrs it keeps what it has."""
    base = [synthetic(S, 36, rad=8.0), synthetic(S, 20, rad=5.0), synthetic(S, 48, rad=11.0, turn=3)]
    b = AttrSlots(S, base, cap=48, ocap=5)
    b.run(3, 'plain')
    b.put({1: recorded('F17_hetero_mixed48')})
    b.check_at_call({1}, ('first attributes',))
    b.run(4, 'first attributes')
    b.put({1: synthetic(S, 30, rad=7.0, turn=5)}, attrs={})
    b.check_at_call({1}, ('all NULL',))
    b.run(3, 'all NULL')
    b.put({1: synthetic(S, 30, rad=10.0, turn=1)}, attrs='keep')     # attrs == NULL: the rows keep the defaults they were given
    b.run(3, 'kept defaults')
    dense = recorded('F17_hetero_dense40')
    b.put({1: dense})
    b.run(2, 'dense40')
    b.put({1: dense}, attrs='keep')                                # the same episode again, its attributes kept by the slot
    b.run(4, 'kept dense40')
    b.close()


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_envelope_only_feeds_filters(S):
    """a live scene at neighborDist 10 beside a slot that takes neighborDist 15, then maxSpeed 2 and dt_nominal 0.2: the context's envelope
    grows, the live scene is its context alone"""
    base = [synthetic(S, 60, rad=7.0), synthetic(S, 60, rad=14.0, turn=2)]
    b = AttrSlots(S, base, cap=60)
    b.run(2, 'base')
    b.put({1: recorded('F16_params_nbr8_far60')})
    b.run(3, 'neighborDist 15')
    fast = dict(DEFAULTS, max_speed=2.0, dt_nominal=0.2)
    b.put({1: synthetic(S, 40, rad=6.0, solver={k: np.full(40, v, np.int32 if k == 'max_neighbors' else np.float64) for k, v in fast.items()})})
    b.run(3, 'maxSpeed 2, dt_nominal 0.2')
    b.close()


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------------------
def test_shrinking_max_neighbors_leaves_no_stale_entry(S):
    base = [synthetic(S, 40, rad=7.0), synthetic(S, 24, rad=6.0)]      # 40 on a circle of 7 m: twenty neighbours within 10 m, 1.1 m apart
    b = AttrSlots(S, base, cap=40, ocap=2)
    got = b.run(2, 'sixteen')
    assert (got['nbr_n'][:40] == 16).all()                         # the slot's lists are full
    b.put({0: recorded('F16_params_nbr4_dense40')})
    for t in range(3):
        got = b.run(1, 'four')
        assert got['nbr_n'][:40].max() == 4                        # (entry for entry the context alone: AttrSlots.check)
    b.close()


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------------------
def test_row_strides(S):
    """slots of 130 rows holding 1, 63, 64, 65 and 129 agents, every row with attribute values of its own (drawn from F17's sets): the 64-byte
    records, the doubles and the bytes land on their rows, and the vacant rows read as vacant"""
    rng = np.random.default_rng(17)
    f17 = [recorded(n) for n in ('F17_hetero_circle60', 'F17_hetero_dense40', 'F17_hetero_mixed48')]
    f18 = recorded('F18_hetero_track_mixed36')
    pool = {k: np.unique(np.concatenate([e['solver'][k] for e in f17])) for k in DEFAULTS}
    trips = np.unique(np.stack([f18['planner'][k] for k in TRK_DEFAULTS], axis=1), axis=0)
    sizes = [1, 63, 64, 65, 129]
    base = [synthetic(S, 130, rad=30.0, turn=s) for s in range(5)]
    b = AttrSlots(S, base, cap=130)
    eps = {}
    for s, n in enumerate(sizes):
        pick = trips[rng.integers(0, len(trips), n)]
        eps[s] = synthetic(S, n, policy=np.roll(MIX, s), rad=max(2.0, n / 5.0), turn=s,
                           solver={k: rng.choice(pool[k], n).astype(np.int32 if k == 'max_neighbors' else np.float64) for k in DEFAULTS},
                           planner={k: pick[:, i].copy() for i, k in enumerate(TRK_DEFAULTS)})
    b.put(eps)
    b.check_at_call({0, 1, 2, 3, 4}, ('strides',))
    b.run(4, 'strides')
    b.close()


# ---- 7, 8 -------------------------------------------------------------------------------------------------------------------------------------
def test_planner_attributes_classes_on_the_fly(S):
    """the tracker is enabled at one value; the F18 episodes bring classes, circle30_each (30 triples) pushes the context past 16 classes while
    the others are in flight, a uniform episode brings it back.  Then tracked <-> untracked with planner attributes set: accepted with
    attrs, refused by the old entry points as before."""
    base = [synthetic(S, 36, rad=9.0, turn=s) for s in range(5)]
    b = AttrSlots(S, base, cap=36, ocap=8)
    b.run(2, 'one value')
    b.put({0: recorded('F18_hetero_track_circle24'), 1: recorded('F18_hetero_track_takeoff16'), 2: recorded('F18_hetero_track_mixed36')})
    b.check_at_call({0, 1, 2}, ('classes',))
    b.run(4, 'classes')
    b.put({3: recorded('F18_hetero_track_circle30_each')})
    b.run(4, 'per-agent form')
    b.put({3: synthetic(S, 30, policy=[0, 5], rad=8.0)}, attrs={})
    b.run(4, 'classes again')
    # tracked <-> untracked
    flip = dict(synthetic(S, 36, policy=[3, 0, 4, 5, 1], rad=9.0, turn=1), planner={k: np.full(36, v) for k, v in dict(turning_radius=2.5, pitch_lo=-0.4, pitch_hi=0.6).items()})
    before = everything(b.sol)
    rc = rc_of(S, lambda: restart_all(b.sol, [4], [flip], sizes='own'))
    assert rc == ERR_UNSUPPORTED
    same(before, everything(b.sol), ('refused by the old entry point',))
    rc = rc_of(S, lambda: restart_all(b.sol, [4], [flip], sizes='own', attrs='keep'))
    assert rc == ERR_UNSUPPORTED                                   # the new call without attrs is the old one
    b.put({4: flip})
    b.check_at_call({4}, ('tracked <-> untracked',))
    b.run(4, 'tracked <-> untracked')
    b.close()


# ---- 9 ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', ['default', 'packed', 'lp_lane'])
def test_kernel_forms_behind_an_attribute_restart(S, monkeypatch, row):
    """both K1 scene forms and both LP forms (the switches sca_create reads), stepped by sca_run_steps(k) and by sca_env_step"""
    for k, v in ({} if row == 'default' else F.ROWS[row]).items():
        monkeypatch.setenv(k, v)
    base = [synthetic(S, 48, rad=11.0, turn=s) for s in range(3)]
    b = AttrSlots(S, base, cap=48, ocap=5)
    b.put({0: recorded('F17_hetero_mixed48'), 2: recorded('F17_hetero_dense40')})
    b.run(2, row)
    b.run(1, row + ' run_steps(3)', step_fn=lambda x: (x.run_steps(3, S.NBR_KDTREE), x.synchronize()), k=3)
    b.run(2, row + ' env_step', step_fn=lambda x: x.env_step(S.NBR_KDTREE))
    b.close()


def test_step_host_log_and_harvest_behind_an_attribute_restart(S):
    """sca_step_host on a batch whose slots are full; the log per scene and the harvest of restarted scenes"""
    base = [synthetic(S, 40, rad=9.0, turn=s) for s in range(3)]
    sol, off = context(S, base, obs_slots=[2] * 3)
    sol.host_state()
    sol.scene_history_enable(6)
    sol.scene_harvest_enable()
    dense, quick = recorded('F17_hetero_dense40'), synthetic(S, 40, rad=9.0, near_goal=True,
                                                             solver={k: np.full(40, v, np.int32 if k == 'max_neighbors' else np.float64)
                                                                     for k, v in dict(DEFAULTS, neighbor_dist=4.0, max_neighbors=3).items()})
    held = {0: base[0], 1: dense, 2: quick}
    restart_all(sol, [1, 2], [dense, quick], sizes='own', obstacles=[(e['obs_pos'], e['obs_radius']) for e in (dense, quick)], attrs=attrs_of([dense, quick]))
    solos = {s: alone(S, e) for s, e in held.items()}
    for x in solos.values():
        x.scene_history_enable(6)
    for t in range(3):
        active = sol.step_host(S.NBR_KDTREE, state=False)
        step_all(S, *solos.values())
        got = assert_slots_equal_alone(sol, off, held, solos, ('step_host', t), [0, 2, 4])
        blk = sol.host_state()
        for key in ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num'):
            assert np.array_equal(blk[key], got[key]), ('block against the device state', t, key)
        assert active == sol.active_count() == int(((got['flags'] & 7) == 0).sum())
        if t == 0:                                                 # the quick episode finished in its first step: its harvest
            assert sol.scene_harvest_collect() == [2]
            h = sol.scene_harvest()
            want = loop_summary(solos[2].get_state(), 0, 40)
            rec = h['summary'][2]
            for k, v in want.items():
                assert rec[k].item() == v, ('harvest', k)
            assert int(rec['steps']) == 1 and np.array_equal(h['pos'][80:120], solos[2].get_state()['pos'])
    for s, x in solos.items():
        a, w = sol.scene_history(s), x.scene_history(0)
        assert len(w['pos']) == (1 if s == 2 else 3)
        for key in w:
            assert np.array_equal(a[key], w[key]), ('log per scene', s, key)
    for x in [sol] + list(solos.values()):
        x.close()


# ---- 10 ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was(S):
    base = [synthetic(S, 24, rad=6.0, turn=s) for s in range(3)]
    b = AttrSlots(S, base, cap=24, ocap=2)
    b.put({1: recorded('F16_params_dt005')})
    b.run(2, 'before')
    ep = recorded('F16_params_dt005')
    good = attrs_of([ep])
    tracked_row = int(tracked(ep)[0])

    def bad(key, row, value):
        a = dict(good)
        a[key] = a[key].copy()
        a[key][row] = value
        return a
    cases = [(bad('neighbor_dist', 3, 0.0), 'row 3'), (bad('max_neighbors', 23, 17), 'row 23'), (bad('time_step', 0, float('nan')), 'row 0'),
             (bad('time_horizon', 5, -1.0), 'row 5'), (bad('max_speed', 7, float('inf')), 'row 7'), (bad('max_heading_change', 9, 3.2), 'row 9'),
             (bad('dt_nominal', 11, 0.0), 'row 11'), (bad('turning_radius', tracked_row, 0.0), 'row %d' % tracked_row),
             (bad('pitch_lo', tracked_row, 1.0), 'row %d' % tracked_row)]
    before, seen = everything(b.sol, tracked(ep) + 24), observe(b.sol)
    for a, names in cases:
        with pytest.raises(S.ScaError) as e:
            b.put({2: ep}, attrs=a)
        assert 'rc=%d' % ERR_ARG in str(e.value) and names in str(e.value), (names, str(e.value))
    # struct_bytes and reserved, through the C entry point itself
    import ctypes as C
    from sca_amd import _lib
    ids, sizes = np.array([2], np.int32), np.array([24], np.int32)
    for sb, reserved in ((4, 0), (12, 0), (C.sizeof(_lib.RestartAttrs) + 8, 0), (C.sizeof(_lib.RestartAttrs), 1)):
        d = _lib.RestartAttrs(struct_bytes=sb, reserved=reserved)
        rc = b.sol.L.sca_restart_scenes_attrs(b.sol.ctx, 1, _lib.ptr(ids, C.c_int32), _lib.ptr(sizes, C.c_int32), None, None, None, C.byref(d),
                                              _lib.ptr(np.ascontiguousarray(ep['pos']), C.c_double), None, _lib.ptr(np.ascontiguousarray(ep['heading']), C.c_double),
                                              None, None, None, None, None, None, None)
        assert rc == ERR_ARG, (sb, reserved)
    same(before, everything(b.sol, tracked(ep) + 24), ('after the refusals',))
    same(seen, observe(b.sol), ('after the refusals', 'counters'))
    b.run(2, 'after')                                              # ... and every slot goes on as its context alone
    b.close()
    # planner arrays without a device tracker
    plain = AttrSlots(S, [synthetic(S, 12, policy=[1, 2, 3], rad=4.0)] * 2, cap=12, tracker=False)
    before = everything(plain.sol)
    with pytest.raises(S.ScaError) as e:
        plain.put({0: synthetic(S, 12, policy=[1, 2, 3], rad=4.0)}, attrs=dict(turning_radius=2.0))
    assert 'rc=%d' % ERR_ARG in str(e.value) and 'tracker' in str(e.value)
    same(before, everything(plain.sol), ('no tracker',))
    plain.close()


# ---- 11 ---------------------------------------------------------------------------------------------------------------------------------------
def test_per_agent_fuzz_scenes_against_the_oracle(S, oracle):
    """independent of the library: the per-agent scenes of tests/form_fuzz.py (attributes drawn per agent, obstacles, all six policies) are
    restarted into slots of a default context and stepped 3 steps; every slot is the oracle's run of that scene alone (oracle_run: the
    oracle's policy_step / env_update with set_agent_params).  A restart starts an episode -- zero flags -- and this batch has no tracker,
    so the oracle runs the scenes from zero flags with the straight-line v_pref rule."""
    scenes = []
    for seed in F.PER_AGENT_SEEDS:                                 # the first five of 9 .. 100 agents with attributes per agent, two at least among obstacles
        sc = F.random_scene(seed)
        per, _, uniform = F.per_agent_attributes(seed, sc['n'])
        with_obs = sum(1 for x, _ in scenes if x['m'])
        if 9 <= sc['n'] <= 100 and not uniform and (sc['m'] or len(scenes) - with_obs < 3):
            n = sc['n']
            sc = dict(sc, flags=np.zeros(n, np.uint8), vmode=np.zeros(n, np.uint8), vpref=np.zeros((n, 3)), key=sc['key'] + ('restart',))
            scenes.append((sc, per))
        if len(scenes) == 5:
            break
    assert len(scenes) == 5 and sum(1 for sc, _ in scenes if sc['m']) >= 2
    cap, ocap = max(sc['n'] for sc, _ in scenes), max(max(sc['m'] for sc, _ in scenes), 1)
    base = synthetic(S, cap, policy=[1, 2, 3, 4], rad=cap / 4.0)
    sol, off = context(S, [base] * len(scenes), obs_slots=[ocap] * len(scenes), tracker=False)
    sol.run_steps(2, S.NBR_KDTREE)
    eps = [dict(n=sc['n'], pos=sc['pos'], heading=sc['heading'], vel=sc['vel'], radius=sc['radius'], pref_speed=sc['pref_speed'], goal=sc['goal'],
                policy=sc['policy'], zaxis=F.zaxis_of(sc), max_run_dist=sc['max_run_dist'], goal_heading=np.zeros((sc['n'], 3))) for sc, _ in scenes]
    restart_all(sol, list(range(len(scenes))), eps, sizes='own', obstacles=[(sc['obs_pos'], sc['obs_radius']) for sc, _ in scenes], tracker=False,
                attrs={k: np.concatenate([per[k] for _, per in scenes]) for k in DEFAULTS})
    runs = [F.oracle_run(oracle, sc, 3, per_agent=(per, {}, False)) for sc, per in scenes]
    for t in range(3):
        step_all(S, sol)
        got = everything(sol)
        for s, (sc, _) in enumerate(scenes):
            lo, n, w = int(off[s]), sc['n'], runs[s][t]
            sl = slice(lo, lo + n)
            for key in F.STATE_KEYS:
                assert np.array_equal(got[key][sl], w[key]), (t, s, key)
            live = (w['before'] & 7) == 0
            assert np.array_equal(got['action'][sl][live], w['action'][live]), (t, s, 'action')
            assert np.array_equal(got['perm'][sl] - lo, w['perm']), (t, s, 'perm')
            assert np.array_equal(got['nbr_n'][sl][live], w['nbr_n'][live]), (t, s, 'nbr_n')
            inl = (np.arange(F.K)[None, :] < w['nbr_n'][:, None]) & live[:, None]
            ids = got['nbr_id'][sl] - np.where(got['nbr_kind'][sl] == 1, ocap * s, lo)
            assert np.array_equal(ids[inl], w['nbr_id'][inl]) and np.array_equal(got['nbr_kind'][sl][inl], w['nbr_kind'][inl]), (t, s, 'lists')
            assert np.array_equal(got['nbr_dsq'][sl][inl], w['nbr_dsq'][inl]), (t, s, 'distSq')
    sol.close()
