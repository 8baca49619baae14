"""Finished scenes hand over their result with the step (-m gpu): sca_scene_harvest_enable / _get / _collect, SceneBatch(harvest=True),
run_episodes(harvest=True).  Every comparison is equality.  The rows of a harvested scene are held against sca_get_state's rows of that
scene directly after the finishing step and against a fresh context holding that episode alone, stepped to its end; the summary against
the Python loop of metrics.episode_metrics over sca_get_state; active / steps in the block against sca_get_scene_state.

The synthetic episodes end quickly: agents on a lattice spaced 12 m (beyond the neighbour distance of 10 m), each with its goal `reach`
metres ahead.  An agent alone moves 0.1 m a step and arrives within 0.5 m of its goal, so a scene whose farthest goal is `reach` ahead takes
round((reach - 0.5) / 0.1) + 1 steps: 3 for 0.7 m .. 9 for 1.3 m.  The counts in STEPS_OF were taken from the CPU oracle (policy_step +
env_update to `done`, ORCA3D and RVO3D alike); so were those of the three summary scenes (collision 1, timeout 3, mixed 4)."""
import ctypes as C
import math

import numpy as np
import pytest

from scene_util import Slots, assert_summary, context, everything, loop_summary, partial_batch, rc_of, restart_all

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -3                                         # include/sca_hip.h
ORCA, RVO = 3, 1                                                    # SCA_POLICY_ORCA3D, SCA_POLICY_RVO3D: straight-line v_pref, no tracker
STEPS_OF = {0.7: 3, 0.8: 4, 0.9: 5, 1.0: 6, 1.1: 7, 1.2: 8, 1.3: 9}  # scene steps by its farthest goal [m]
COLUMNS = ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num')
SENTINEL = dict(pos=-7.25, vel=-3.5, heading=-9.125, flags=0xAB, total_dist=-11.5, step_num=-77)


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


def lattice_scene(S, n, reach, pos=None, max_run_dist=None):
    """n agents 12 m apart (or at `pos`), agent i's goal reach[i] metres ahead; policies ORCA3D / RVO3D in turn.  A scalar reach: the scene's
    farthest goal, agent i's is 0, 0.1 or 0.2 m nearer (never below 0.7 m), so total_dist and step_num differ inside the scene."""
    from sca_amd import scenarios
    i = np.arange(n)
    if np.ndim(reach) == 0:
        reach = np.maximum(0.7, np.round(reach - 0.1 * (i % 3), 1))
    side = int(math.ceil(math.sqrt(n)))
    pos = np.stack([(i % side) * 12.0, (i // side) * 12.0, np.full(n, 10.0)], 1) if pos is None else np.asarray(pos, float)
    goal = pos + np.stack([np.asarray(reach, float), np.zeros(n), np.zeros(n)], 1)
    start6, goal6 = np.hstack([pos, np.zeros((n, 3))]), np.hstack([goal, np.zeros((n, 3))])
    mrd = scenarios.max_run_dist(start6, goal6) if max_run_dist is None else np.asarray(max_run_dist, float)
    return dict(n=n, pos=pos, heading=np.zeros((n, 3)), vel=np.zeros((n, 3), np.float32), radius=np.full(n, 0.5), pref_speed=np.ones(n), goal=goal,
                policy=np.where(i % 2 == 0, ORCA, RVO).astype(np.uint8), zaxis=S.zaxis_flags(start6, goal6), max_run_dist=mrd, goal_heading=np.zeros((n, 3)))


def enable(sol, sentinel=True):
    """the harvest on, its views, and every row section pre-filled with a value no state holds"""
    sol.scene_harvest_enable()
    hv = sol.scene_harvest()
    if sentinel:
        for k, v in SENTINEL.items():
            hv[k][...] = v
    return hv


def rows(hv, lo, hi):
    return {k: hv[k][lo:hi].copy() for k in COLUMNS}


def assert_rows(got, st, lo, hi, ctx):
    for k in COLUMNS:
        assert got[k].dtype == st[k].dtype and np.array_equal(got[k], st[k][lo:hi]), ctx + (k,)


def assert_sentinel(hv, lo, hi, ctx):
    for k, v in SENTINEL.items():
        assert (hv[k][lo:hi] == np.array(v).astype(hv[k].dtype)).all(), ctx + ('rows nobody may write', k)


def assert_counters(sol, hv, ctx):
    sc = sol.scene_state()
    assert np.array_equal(hv['active'], sc['active']) and np.array_equal(hv['steps'], sc['steps']), ctx + (hv['active'].tolist(), sc['active'].tolist())
    return sc


def alone_final(S, ep, steps, tracker=False):
    """the episode in a context of its own, stepped to its end"""
    solo = context(S, [ep], tracker=tracker)[0]
    solo.run_steps(steps, S.NBR_KDTREE)
    solo.synchronize()
    st = solo.get_state()
    assert solo.scene_state()['active'][0] == 0 and solo.scene_state()['steps'][0] == steps
    solo.close()
    return st


SIZES = (1, 63, 64, 65, 255, 256, 257)                              # the workgroup's 256-thread stride and its edges, a wavefront's, one agent
REACH = (0.9, 0.7, 0.8, 0.7, 1.0, 0.9, 0.8)                         # scenes 1 and 3 finish together at step 3, 2 and 6 at 4, 0 and 5 at 5, 4 at 6


def test_scene_sizes_step_by_step(S):
    eps = [lattice_scene(S, n, r) for n, r in zip(SIZES, REACH)]
    sol, off = context(S, eps, tracker=False)
    hv = enable(sol)
    assert_counters(sol, hv, ('at enable',))
    assert hv['active'].tolist() == list(SIZES) and not hv['steps'].any()
    want_steps = [STEPS_OF[r] for r in REACH]
    kept, finished = {}, set()
    for t in range(1, 7):
        total = sol.env_step(S.NBR_KDTREE)
        fresh_words = hv['summary']['fresh'].copy()                 # readable behind the step's own synchronisation, before any other call
        active_now, steps_now = hv['active'].copy(), hv['steps'].copy()
        st = sol.get_state()
        sc = assert_counters(sol, hv, ('step', t))
        assert np.array_equal(active_now, sc['active']) and np.array_equal(steps_now, sc['steps']) and total == int(sc['active'].sum())
        want = [s for s, k in enumerate(want_steps) if k == t]
        assert np.flatnonzero(fresh_words).tolist() == want, ('fresh words', t)
        assert sol.scene_harvest_collect() == want, ('collect', t)
        assert not hv['summary']['fresh'].any() and sol.scene_harvest_collect() == []
        for s in want:
            lo, hi = int(off[s]), int(off[s + 1])
            kept[s] = rows(hv, lo, hi)
            assert_rows(kept[s], st, lo, hi, ('step', t, 'scene', s))
            assert_summary(hv['summary'][s], loop_summary(st, lo, hi), t, t, ('step', t, 'scene', s))
            assert hv['summary'][s]['arrived'] == SIZES[s] == hv['summary'][s]['successful_num']
            finished.add(s)
        for s in range(len(SIZES)):
            if s not in finished:
                assert_sentinel(hv, int(off[s]), int(off[s + 1]), ('step', t, 'scene', s))
    assert finished == set(range(len(SIZES))) and not hv['active'].any() and hv['steps'].tolist() == want_steps
    st = sol.get_state()
    for s, ep in enumerate(eps):                                    # the rows stay what they were, and are the episode's alone
        lo, hi = int(off[s]), int(off[s + 1])
        assert_rows(rows(hv, lo, hi), kept[s], 0, hi - lo, ('kept', s))
        assert_rows(kept[s], st, lo, hi, ('inert', s))
        assert_rows(kept[s], alone_final(S, ep, want_steps[s]), 0, hi - lo, ('alone', s))
    sol.close()


def test_a_capacity_slot_writes_its_occupied_rows_only(S):
    """two slots of capacity 130 holding 5 and 11 agents: slot 1 begins at row 130, not a multiple of four -- the flag bytes at its edges"""
    eps = [lattice_scene(S, 5, 0.7), lattice_scene(S, 11, 0.9)]
    sol, off = partial_batch(S, eps, 130)
    hv = enable(sol)
    assert off.tolist() == [0, 130, 260] and hv['active'].tolist() == [5, 11]
    got = []
    for t in range(1, 6):
        sol.env_step(S.NBR_KDTREE)
        got += [(t, s) for s in sol.scene_harvest_collect()]
    assert got == [(3, 0), (5, 1)]
    st = sol.get_state()
    for s, ep in enumerate(eps):
        lo = int(off[s])
        assert_rows(rows(hv, lo, lo + ep['n']), st, lo, lo + ep['n'], ('slot', s))
        assert_sentinel(hv, lo + ep['n'], int(off[s + 1]), ('slot', s))
        assert_summary(hv['summary'][s], loop_summary(st, lo, lo + ep['n']), STEPS_OF[(0.7, 0.9)[s]], (3, 5)[s], ('slot', s))
        assert hv['summary'][s]['arrived'] == ep['n']              # the vacant rows (flags at-goal | collision) are not counted
        assert_rows(rows(hv, lo, lo + ep['n']), alone_final(S, ep, STEPS_OF[(0.7, 0.9)[s]], tracker=True), 0, ep['n'], ('alone', s))
    sol.close()


def test_finishing_patterns_and_a_burst(S):
    reach = (1.0, 0.7, 0.9, 0.7)                                    # steps 6, 3, 5, 3
    eps = [lattice_scene(S, 3, r) for r in reach]
    sol, off = context(S, eps, tracker=False)
    hv = enable(sol)
    for t in (1, 2):                                                # steps in which nobody finishes
        sol.env_step(S.NBR_KDTREE)
        assert not hv['summary']['fresh'].any()
        assert_counters(sol, hv, ('quiet step', t))
        assert sol.scene_harvest_collect() == []
    assert_sentinel(hv, 0, int(off[-1]), ('quiet steps',))
    sol.run_steps(5, S.NBR_KDTREE)                                  # batch steps 3 .. 7: scenes 1 and 3 end in 3, scene 2 in 5, scene 0 in 6
    assert sol.scene_harvest_collect() == [1, 3, 2, 0]              # ascending (batch_step, id)
    st = sol.get_state()
    assert_counters(sol, hv, ('behind the burst',))
    for s, r in enumerate(reach):
        lo, hi = int(off[s]), int(off[s + 1])
        assert_rows(rows(hv, lo, hi), st, lo, hi, ('burst', s))
        assert_summary(hv['summary'][s], loop_summary(st, lo, hi), STEPS_OF[r], STEPS_OF[r], ('burst', s))
    assert sol.scene_harvest_collect() == [] and not hv['active'].any()
    sol.close()


def _summary_scenes(S):
    collision = lattice_scene(S, 2, [1.0, 1.0], pos=[[0, 0, 10.0], [0.3, 0, 10.0]])             # 0.3 m apart, radii 0.5: overlapping
    timeout = lattice_scene(S, 1, [3.0], max_run_dist=[0.15])
    mixed = lattice_scene(S, 4, [1.0, 1.0, 0.8, 3.0], pos=[[0, 0, 10.0], [0.3, 0, 10.0], [12.0, 0, 10.0], [24.0, 0, 10.0]], max_run_dist=[3.0, 3.0, 2.4, 0.15])
    return [collision, timeout, mixed]


def test_summary(S):
    eps = _summary_scenes(S)
    sol, off = context(S, eps, tracker=False)
    hv = enable(sol)
    want_steps = [1, 3, 4]
    literal = [dict(arrived=0, collided=2, timed_out=0, successful_num=0, all_step_num=0, all_distance=0.0),
               dict(arrived=0, collided=0, timed_out=1, successful_num=0, all_step_num=0, all_distance=0.0),
               dict(arrived=1, collided=2, timed_out=1, successful_num=1, all_step_num=4)]
    for t in range(1, 5):
        sol.env_step(S.NBR_KDTREE)
        ids = sol.scene_harvest_collect()
        assert ids == [s for s, k in enumerate(want_steps) if k == t], t
        st = sol.get_state()
        for s in ids:
            lo, hi = int(off[s]), int(off[s + 1])
            assert_rows(rows(hv, lo, hi), st, lo, hi, ('summary scene', s))
            assert_summary(hv['summary'][s], loop_summary(st, lo, hi), t, t, ('summary scene', s))
            assert_summary(hv['summary'][s], literal[s], t, t, ('summary scene, by hand', s))
    assert hv['summary'][2]['all_distance'] > 0.0
    sol.close()


def test_a_recorded_episode_harvested_restarted_and_harvested_again(S):
    """F4_sca_circle16_obs (289 steps) and F4_sca_takeoff16 (285) among the take-off field's 8 spheres, device tracker in the pass: one batch
    with the harvest, one without.  Whatever can be asked of the two contexts is equal throughout."""
    names = ['F4_sca_circle16_obs', 'F4_sca_takeoff16']
    a, p = Slots(S, names), Slots(S, names)
    assert len(a.obs_radius) == 8 and a.tracker
    hv = enable(a.sol)
    ids = list(range(a.n))

    def both(k):
        for b in (a, p):
            b.sol.run_steps(k, S.NBR_KDTREE)
            b.sol.synchronize()

    def same(ctx):
        x, y = everything(a.sol, ids), everything(p.sol, ids)
        for key in x:
            if key == 'track':
                assert all(np.array_equal(x[key][i], y[key][i], equal_nan=True) for i in ids), ctx + (key,)
            else:
                assert np.array_equal(x[key], y[key], equal_nan=True), ctx + (key,)
        return x
    both(285)
    assert a.sol.scene_harvest_collect() == [1] and (hv['summary'][1]['steps'], hv['summary'][1]['batch_step']) == (285, 285)
    both(4)
    assert a.sol.scene_harvest_collect() == [0] and (hv['summary'][0]['steps'], hv['summary'][0]['batch_step']) == (289, 289)
    st = same(('first finish',))
    fx = a.fx[0]
    assert int(fx['done_step']) == 288 == int(fx['step'][-1])
    first = rows(hv, 0, 16)
    assert_rows(first, st, 0, 16, ('first finish',))
    for key in ('pos', 'heading', 'total_dist', 'flags'):           # ... which are the reference's records of the episode's last step
        assert np.array_equal(first[key], fx[key + '_after'][-1]), key
    assert_summary(hv['summary'][0], loop_summary(st, 0, 16), 289, 289, ('first finish',))
    assert_rows(rows(hv, 16, 32), st, 16, 32, ('slot 1',))
    for b in (a, p):
        b.restart({0: 'F4_sca_circle16_obs'})
    assert hv['summary'][0]['fresh'] == 0 and a.sol.scene_harvest_collect() == []
    both(100)
    assert hv['summary'][0]['fresh'] == 0 and a.sol.scene_harvest_collect() == [] and hv['active'][0] > 0 and hv['steps'].tolist() == [100, 285]
    same(('second episode, under way',))
    assert_rows(rows(hv, 0, 16), first, 0, 16, ('the block keeps the first harvest until the slot finishes again',))
    both(189)
    assert a.sol.scene_harvest_collect() == [0] and (hv['summary'][0]['steps'], hv['summary'][0]['batch_step']) == (289, 578)
    st = same(('second finish',))
    assert_rows(rows(hv, 0, 16), st, 0, 16, ('second finish',))
    assert_rows(rows(hv, 0, 16), first, 0, 16, ('the same episode again',))
    assert_rows(rows(hv, 16, 32), st, 16, 32, ('slot 1 untouched',))
    for b in (a, p):
        b.sol.close()


def _collected(S, sol, off, hv, step, steps):
    out = []
    for t in range(1, steps + 1):
        step(sol)
        ids = sol.scene_harvest_collect()
        out.append((t, ids, [(rows(hv, int(off[s]), int(off[s + 1])), hv['summary'][s].copy()) for s in ids], hv['active'].copy(), hv['steps'].copy()))
    return out


def test_step_forms(S):
    """the harvest behind sca_env_step, sca_step_host, sca_step_begin / sca_step_end, sca_policy_pass + sca_env_update and an sca_env_update
    of its own inside sca_run_steps(1): the same scenes at the same steps with the same rows"""
    reach = (0.8, 0.7, 1.0)
    forms = dict(env_step=lambda x: x.env_step(S.NBR_KDTREE),
                 step_host=lambda x: x.step_host(S.NBR_KDTREE, state=False),
                 begin_end=lambda x: (x.step_begin(S.NBR_KDTREE), x.step_end(), x.synchronize()),
                 split=lambda x: (x.policy_pass(S.NBR_KDTREE), x.env_update()),
                 run_steps=lambda x: (x.run_steps(1, S.NBR_KDTREE), x.synchronize()))
    results = {}
    for name, form in forms.items():
        sol, off = context(S, [lattice_scene(S, 5, r) for r in reach], tracker=False)
        hv = enable(sol)
        if name == 'step_host':
            sol.host_state()
        results[name] = _collected(S, sol, off, hv, form, 6)
        assert [(t, ids) for t, ids, *_ in results[name] if ids] == [(3, [1]), (4, [0]), (6, [2])], name
        assert_counters(sol, hv, (name,))
        sol.close()
    ref = results['env_step']
    for name, got in results.items():
        for (t, ids, taken, active, steps), (_, _, want, active_w, steps_w) in zip(got, ref):
            assert np.array_equal(active, active_w) and np.array_equal(steps, steps_w), (name, t)
            for (r, sm), (rw, smw) in zip(taken, want):
                assert_rows(r, rw, 0, 5, (name, t))
                assert sm.tobytes() == smw.tobytes(), (name, t, sm, smw)


def test_fresh_words_cleared_without_a_collect(S):
    eps = [lattice_scene(S, 4, 0.7), lattice_scene(S, 4, 0.7), lattice_scene(S, 4, 1.0)]
    # sca_restart_scenes: the named scenes' words only
    sol, off = context(S, eps, tracker=False)
    hv = enable(sol, sentinel=False)
    sol.run_steps(3, S.NBR_KDTREE)
    sol.synchronize()
    assert hv['summary']['fresh'].tolist() == [1, 1, 0]
    restart_all(sol, [1], [eps[1]], tracker=False)
    assert hv['summary']['fresh'].tolist() == [1, 0, 0]             # an uncollected harvest of a restarted scene is gone
    assert sol.scene_harvest_collect() == [0]
    sol.run_steps(3, S.NBR_KDTREE)                                  # batch steps 4 .. 6: the restarted scene ends in 6, after its own 3; so does scene 2
    assert sol.scene_harvest_collect() == [1, 2]
    assert hv['summary']['steps'].tolist() == [3, 3, 6] and hv['summary']['batch_step'].tolist() == [3, 6, 6]
    # sca_set_state: all of them
    restart_all(sol, [0, 1], [eps[0], eps[1]], tracker=False)
    sol.run_steps(3, S.NBR_KDTREE)
    sol.synchronize()
    assert hv['summary']['fresh'].tolist() == [1, 1, 0]
    st = sol.get_state()
    sol.set_state(st['pos'], st['vel'], st['heading'], st['flags'], st['total_dist'], st['step_num'])
    assert not hv['summary']['fresh'].any() and sol.scene_harvest_collect() == []
    sol.env_step(S.NBR_KDTREE)                                      # scenes that came in finished never finish
    assert sol.scene_harvest_collect() == [] and not hv['active'].any()
    # sca_step_host with SCA_HOST_IN_STATE: all of them, before the step's own harvest
    restart_all(sol, [0, 2], [eps[0], eps[2]], tracker=False)
    sol.run_steps(3, S.NBR_KDTREE)
    sol.synchronize()
    assert hv['summary']['fresh'].tolist() == [1, 0, 0]
    st, hs = sol.get_state(), sol.host_state()
    for k in COLUMNS:
        hs[k][...] = st[k]
    sol.step_host(S.NBR_KDTREE, state=True)                         # scene 2's fourth step; scene 0 came in finished
    assert not hv['summary']['fresh'].any() and hv['active'].tolist() == [0, 0, 3] and hv['steps'][2] == 4     # (the agent 0.8 m from its goal arrived)
    assert_counters(sol, hv, ('behind a state from the block',))
    sol.step_host(S.NBR_KDTREE, state=False)
    sol.step_host(S.NBR_KDTREE, state=False)
    assert sol.scene_harvest_collect() == [2] and hv['summary'][2]['steps'] == 6
    sol.close()


def test_refusals_and_lifetime(S):
    from sca_amd import _lib
    eps = [lattice_scene(S, 3, 0.7), lattice_scene(S, 3, 0.8)]
    ep = lattice_scene(S, 6, 0.7)
    sol = S.BatchedSolver(max_agents=6, max_obstacles=1)
    sol.set_agents(ep['radius'], ep['pref_speed'], ep['goal'], ep['policy'], ep['zaxis'], ep['max_run_dist'])
    L, ctx = sol.L, sol.ctx
    ids, count, h = np.zeros(2, np.int32), C.c_int32(7), _lib.SceneHarvest()
    i32 = lambda a: _lib.ptr(a, C.c_int32)
    # no scenes
    assert L.sca_scene_harvest_enable(ctx, 1) == ERR_STATE and L.sca_scene_harvest_enable(ctx, 0) == ERR_STATE
    assert L.sca_scene_harvest_get(ctx, C.byref(h), C.sizeof(h)) == ERR_STATE
    assert L.sca_scene_harvest_collect(ctx, i32(ids), C.byref(count)) == ERR_STATE and count.value == 7
    sol.close()
    sol, off = context(S, eps, tracker=False)
    L, ctx = sol.L, sol.ctx
    # not enabled
    assert L.sca_scene_harvest_get(ctx, C.byref(h), C.sizeof(h)) == ERR_STATE
    assert L.sca_scene_harvest_collect(ctx, i32(ids), C.byref(count)) == ERR_STATE
    assert rc_of(S, sol.scene_harvest) == ERR_STATE and rc_of(S, sol.scene_harvest_collect) == ERR_STATE
    assert L.sca_scene_harvest_enable(ctx, 0) == 0                  # off while off: nothing to free
    # between a policy pass and its env update
    sol.policy_pass(S.NBR_KDTREE)
    assert L.sca_scene_harvest_enable(ctx, 1) == ERR_STATE and b'env update' in L.sca_last_error(ctx)
    assert L.sca_scene_harvest_get(ctx, C.byref(h), C.sizeof(h)) == ERR_STATE            # ... and changed nothing
    sol.env_update()
    hv = enable(sol)
    assert hv['active'].tolist() == [3, 3] and hv['steps'].tolist() == [1, 1]            # the counters as the scenes stand at enable
    # arguments
    assert L.sca_scene_harvest_get(ctx, None, C.sizeof(h)) == ERR_ARG
    assert L.sca_scene_harvest_get(ctx, C.byref(h), 15) == ERR_ARG and L.sca_scene_harvest_get(ctx, C.byref(h), C.sizeof(h) + 1) == ERR_ARG
    assert L.sca_scene_harvest_collect(ctx, None, C.byref(count)) == ERR_ARG and L.sca_scene_harvest_collect(ctx, i32(ids), None) == ERR_ARG
    part = _lib.SceneHarvest()
    assert L.sca_scene_harvest_get(ctx, C.byref(part), 32) == 0     # the integers and two pointers: nothing behind them is written
    assert (part.struct_bytes, part.nscenes, part.n) == (32, 2, 6) and bool(part.counters) and bool(part.summary) and not bool(part.pos)
    offs, total = (C.c_int64 * 8)(), C.c_int64(0)
    assert L.sca_scene_harvest_layout(2, 6, offs, C.byref(total)) == 0 and list(offs) == [0, 128, 256, 512, 640, 896, 1024, 1152] and total.value == 1280
    assert L.sca_scene_harvest_get(ctx, C.byref(h), C.sizeof(h)) == 0
    assert C.addressof(h.step_num.contents) - C.addressof(h.counters.contents) == 1152
    for bad in ((0, 6), (7, 6), (-1, 6)):
        assert L.sca_scene_harvest_layout(bad[0], bad[1], offs, C.byref(total)) == ERR_ARG
    assert L.sca_scene_harvest_layout(2, 6, None, C.byref(total)) == ERR_ARG and L.sca_scene_harvest_layout(2, 6, offs, None) == ERR_ARG
    # mid-step: the pointers and a collect are fine, enable / disable are not
    sol.policy_pass(S.NBR_KDTREE)
    assert L.sca_scene_harvest_enable(ctx, 0) == ERR_STATE and L.sca_scene_harvest_get(ctx, C.byref(h), C.sizeof(h)) == 0
    assert sol.scene_harvest_collect() == []
    sol.env_update()
    assert hv['steps'].tolist() == [2, 2] and hv['summary']['batch_step'].tolist() == [0, 0]
    # disable, step without, enable again: batch_step counts from the second enable
    sol.scene_harvest_enable(False)
    assert rc_of(S, sol.scene_harvest_collect) == ERR_STATE
    sol.env_step(S.NBR_KDTREE)                                      # scene 0 (0.7 m: 3 steps) finishes unobserved
    hv = enable(sol)
    assert hv['active'].tolist() == [0, 1] and hv['steps'].tolist() == [3, 3] and sol.scene_harvest_collect() == []      # (scene 1: the two agents 0.7 m from their goals arrived too)
    sol.env_step(S.NBR_KDTREE)
    assert sol.scene_harvest_collect() == [1] and (hv['summary'][1]['steps'], hv['summary'][1]['batch_step']) == (4, 1)
    assert_sentinel(hv, 0, 3, ('a scene that finished while the harvest was off',))
    st = sol.get_state()
    assert_rows(rows(hv, 3, 6), st, 3, 6, ('enabled again',))
    # whatever redefines or clears the scenes drops the harvest
    hv = None
    sol.set_scenes(off)
    assert L.sca_scene_harvest_get(ctx, C.byref(h), C.sizeof(h)) == ERR_STATE
    sol.set_state(st['pos'], st['vel'], st['heading'], np.zeros(6, np.uint8))
    enable(sol, sentinel=False)
    sol.set_scenes(None)
    assert L.sca_scene_harvest_get(ctx, C.byref(h), C.sizeof(h)) == ERR_STATE and L.sca_scene_harvest_enable(ctx, 1) == ERR_STATE
    sol.close()


# ---- SceneBatch(harvest=True) and run_episodes(harvest=True) ------------------------------------------------------------------------------------
def _lattice_agents(n, reach, policy, collide=False, tired=False):
    """Agent objects of a lattice episode; collide: agent 1 starts 0.3 m from agent 0; tired: the last agent times out after two steps"""
    from sca_amd.env import Agent
    side = int(math.ceil(math.sqrt(n)))
    out = []
    for i in range(n):
        p = [(i % side) * 12.0, (i // side) * 12.0, 10.0]
        if collide and i == 1:
            p = [0.3, 0.0, 10.0]
        r = max(0.7, round(reach - 0.1 * (i % 3), 1))
        a = Agent(start_pos=p + [0.0, 0.0, 0.0], goal_pos=[p[0] + r, p[1], p[2], 0.0, 0.0, 0.0], vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0,
                  policy=policy, id=i)
        if tired and i == n - 1:
            a.max_run_dist = 0.15
        out.append(a)
    return out


def _queue():
    from sca_amd.env import ORCA3DPolicy, RVO3DPolicy, SRVO3DPolicy
    spec = [(20, 0.9, ORCA3DPolicy, False, False), (50, 0.7, RVO3DPolicy, True, False), (100, 1.1, ORCA3DPolicy, False, True),
            (100, 0.8, SRVO3DPolicy, True, True), (20, 1.3, RVO3DPolicy, False, False), (50, 1.0, ORCA3DPolicy, False, True),
            (20, 0.7, SRVO3DPolicy, True, False), (100, 0.7, RVO3DPolicy, False, False), (50, 1.2, SRVO3DPolicy, False, False)]
    return [_lattice_agents(*s) for s in spec]


WALL = ('AverageCost', 'all_compute_time')                          # wall time of the policy calls: differs from run to run


def test_run_episodes_with_the_harvest_equals_without():
    """nine episodes of 20 / 50 / 100 drones through three capacity slots with history_rows set: results, on_done order and stats"""
    from sca_amd.scenes import run_episodes
    out = {}
    for harvest in (False, True):
        stats, order = {}, []
        res = run_episodes(_queue(), 3, on_done=lambda r: order.append((r['episode'], r['slot'])), stats=stats, history_rows=16, capacities='max',
                           harvest=harvest, max_steps=200)
        out[harvest] = (res, stats, order)
    (want, stats_w, order_w), (got, stats_g, order_g) = out[False], out[True]
    assert order_g == order_w and len(order_w) == 9 and stats_g == stats_w
    assert {len(r['state']['flags']) for r in want} == {20, 50, 100}
    assert any(r['metrics']['successful_num'] < len(r['state']['flags']) for r in want)             # the collisions and timeouts count
    for i, (g, w) in enumerate(zip(got, want)):
        assert list(g) == list(w), i
        assert (g['episode'], g['slot'], g['steps'], g['rows_dropped']) == (w['episode'], w['slot'], w['steps'], w['rows_dropped']), i
        assert list(g['metrics']) == list(w['metrics']) and list(g['info']) == list(w['info']), i
        for key, v in w['metrics'].items():
            if key not in WALL:
                assert np.array_equal(g['metrics'][key], v, equal_nan=True), (i, key, g['metrics'][key], v)
        for key, v in w['info'].items():
            if key not in WALL:
                assert g['info'][key] == v or (v != v and g['info'][key] != g['info'][key]), (i, 'info', key)
        assert list(g['state']) == list(w['state'])
        for key, v in w['state'].items():
            assert g['state'][key].dtype == v.dtype and np.array_equal(g['state'][key], v), (i, key)
        assert np.array_equal(g['trajectories'], w['trajectories']), i


def test_scene_batch_reads_the_block_instead_of_the_scene_state():
    from sca_amd.env import ORCA3DPolicy
    from sca_amd.scenes import SceneBatch
    make = lambda: [_lattice_agents(5, 0.7, ORCA3DPolicy), _lattice_agents(9, 0.9, ORCA3DPolicy, collide=True)]
    batch, plain = SceneBatch(make(), harvest=True), SceneBatch(make())
    with pytest.raises(RuntimeError):
        plain.finished()
    seen = []
    for t in range(1, 6):
        done, done_w = batch.step(), plain.step()
        assert done == done_w and np.array_equal(batch.active, plain.active) and np.array_equal(batch.steps, plain.steps), t
        seen += [(t, s) for s in batch.finished()]
    assert seen == [(3, 0), (5, 1)] and done
    for s in (0, 1):
        h = batch.harvested(s)
        lo, hi = int(plain.offsets[s]), int(plain.offsets[s + 1])
        for k in COLUMNS:
            assert np.array_equal(h[k], plain._state(k)[lo:hi]), (s, k)
        assert h['summary']['steps'] == int(plain.steps[s])
    assert batch.harvested(1)['summary']['collided'] == 2
    batch.restart({0: _lattice_agents(5, 0.8, ORCA3DPolicy)})
    plain.restart({0: _lattice_agents(5, 0.8, ORCA3DPolicy)})
    assert np.array_equal(batch.active, plain.active) and np.array_equal(batch.steps, plain.steps) and batch.active.tolist() == [5, 0]
    for t in range(4):
        batch.step(), plain.step()
        assert np.array_equal(batch.active, plain.active) and np.array_equal(batch.steps, plain.steps)
    assert batch.finished() == [0] and batch.harvested(0)['summary']['steps'] == 4
    batch.close(), plain.close()
