"""Scene checkpoints (-m gpu): sca_save_scenes / sca_load_scenes and the Python layers over them.

The contract (include/sca_hip.h): after restart(E) + load(a blob taken from a scene holding E after its k-th step) the scene is bit for bit
the scene the blob was taken from, from there on, and no other scene can tell.  What is held here: recorded episodes resumed in another
context with another slot order and other capacities, against the reference's records of the steps behind k AND against the source batch
running on; k = 0, k = 1 and a finished scene; a fork inside one context beside a twin batch that never saw the calls; sizes around the
wavefront and the workgroup; every step form, the log per scene and the harvest behind a load; a checkpoint written by another process;
every refusal, which leaves the context as it was; and the Python layers.  Every comparison is array_equal (NaN equals NaN where a value
may be None: v_pref of a row that was not served, now_goal)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import scene_util as U
import test_gpu_scene_attrs as A
import test_gpu_scene_paths as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -1, -3
MIX = [0, 1, 2, 3, 4, 5]
# what a load restores (the outputs of the last pass -- action rows, neighbour lists, diag, vpref_used -- follow with the next pass)
STATE = ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num', 'perm', 'status', 'remaining', 'now_goal', 'replans', 'track', 'steps', 'active')
SEC = dict(policy=0, rec=1, heading=2, perm=8, mode=9, nbr0=10, track=11, rem=12, now_goal=13)     # sca_scene_checkpoint_layout's sections


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


# ---- episodes and batches ---------------------------------------------------------------------------------------------------------------------
def recorded(name):
    """a recorded episode with its attributes (test_gpu_scene_attrs.recorded) and its waypoint lists"""
    e = A.recorded(name)
    if 'paths' not in e:
        e['paths'] = P.lists_of(e['fx'])
    return e


def synthetic(S, n, seed=0, policy=MIX, W=0, rad=None, goal_shift=None):
    """a circle episode without records; W > 0: seeded lists of up to W waypoints; goal_shift: every goal that far along x from its start"""
    e = A.synthetic(S, n, policy=policy, rad=rad, turn=seed)
    if goal_shift is not None:
        e['goal'] = e['pos'] + [goal_shift, 0.0, 0.0]
    e['paths'] = P.seeded_lists(e, seed, W) if W else [[] for _ in range(n)]
    return e


def tracked3(e):
    """the tracked agents whose records are read: the first three"""
    return [int(a) for a in U.tracked(e)[:3]]


class Batch:
    """B slots of `cap` agent rows, room for W waypoints per row and `ocap` obstacles each, the device tracker in the pass.  put() is ONE
    restart that brings everything an episode defines: size, constants, obstacles, attributes, lists."""

    def __init__(self, S, eps, cap, W=30, ocap=8, log=0, harvest=False, tracker=True, path_slots=True):
        self.S, self.B, self.tracker = S, len(eps), tracker
        filler = synthetic(S, 4, goal_shift=0.2)                     # (finishes in its first step)
        self.sol, self.off = U.context(S, [U.padded(A.arrays(filler), cap)] * self.B, obs_slots=[ocap] * self.B, tracker=tracker)
        self.path_slots = path_slots
        if path_slots:
            self.sol.set_path_slots(W)
        if log:
            self.sol.scene_history_enable(log)
        if harvest:
            self.sol.scene_harvest_enable()
        self.obs_lo = [ocap * s for s in range(self.B)]
        self.held = {}
        self.put({s: e for s, e in enumerate(eps)})

    def put(self, plan):
        ids = sorted(plan)
        eps = [plan[s] for s in ids]
        U.restart_all(self.sol, ids, eps, sizes='own', obstacles=[(e['obs_pos'], e['obs_radius']) for e in eps], tracker=self.tracker,
                      attrs=A.attrs_of(eps, self.tracker), paths=[p for e in eps for p in e['paths']] if self.path_slots else None)
        self.held.update(plan)

    def resume(self, plan, blobs):
        """{slot: episode} and the blobs, in the order of the sorted slots: the restart, then ONE load"""
        self.put(plan)
        self.sol.load_scenes(sorted(plan), blobs)

    def step(self, k=1):
        self.sol.run_steps(k, self.S.NBR_KDTREE)
        self.sol.synchronize()

    def views(self, slots=None):
        """{slot: every value of the contract for the slot's occupied rows, in scene-local terms}"""
        slots = sorted(self.held) if slots is None else slots
        sol = self.sol
        trk = {s: tracked3(self.held[s]) for s in slots}
        got = U.everything(sol, [int(self.off[s]) + a for s in slots for a in trk[s]] if self.tracker else ())
        if self.path_slots:
            rem, ng = sol.get_path_state()
        sc = sol.scene_state()
        replans = sol.device_tracker_replans() if self.tracker else None
        out = {}
        for s in slots:
            lo, n = int(self.off[s]), self.held[s]['n']
            sl = slice(lo, lo + n)
            v = {k: x[sl] for k, x in got.items() if k not in ('track', 'replans')}
            v['perm'] = v['perm'] - lo
            v['nbr_id'] = v['nbr_id'] - np.where(v['nbr_id'] >= 0, np.where(v['nbr_kind'] == 1, self.obs_lo[s], lo), 0)
            if self.tracker:
                v['track'] = {a: got['track'][lo + a] for a in trk[s]} if trk[s] else {}
                v['replans'] = replans[sl]
            if self.path_slots:
                v.update(remaining=rem[sl], now_goal=ng[sl])
            v.update(steps=sc['steps'][s:s + 1], active=sc['active'][s:s + 1])
            out[s] = v
        return out

    def close(self):
        self.sol.close()


def same_scene(a, b, ctx, keys=None):
    U.same(a, b, ctx, keys=[k for k in (keys or a) if k in a])


def check_record(v, e, local, ctx, outputs=True):
    """a slot's view behind `local` steps of its episode against the reference's record of that step, if there is one; outputs=False: the
    state alone (directly behind a load the action rows are not the episode's)"""
    k = e['index'].get(local - 1)
    if k is None:
        return 0
    fx = e['fx']
    ctx = ctx + (e['name'], 'record', k)
    for key in ('pos', 'heading', 'total_dist', 'flags'):
        assert np.array_equal(v[key], fx[key + '_after'][k]), ctx + (key,)
    assert np.array_equal(v['vel'][:, :3], fx['vel_after'][k]), ctx + ('vel',)
    assert np.array_equal(v['perm'], fx['perm_after'][k]), ctx + ('perm',)
    if outputs:
        called = fx['called'][k].astype(bool)
        assert np.array_equal(v['action'][called], fx['action'][k][called]), ctx + ('action',)
        assert not v['status'].any(), ctx + ('status',)
    if 'path_off' in fx:
        assert np.array_equal(v['remaining'], fx['path_left_after'][k]), ctx + ('path_left',)
        assert np.array_equal(v['now_goal'], fx['now_goal_after'][k], equal_nan=True), ctx + ('now_goal',)
    return 1


# ---- 1: recorded episodes, resumed against the reference and against the source running on ----------------------------------------------------
RECORDED = [('F4_sca_takeoff16', 200), ('F4_mixed_takeoff16', 150), ('paths/F19_path_edge10', 100), ('F17_hetero_mixed48', 10),
            ('F18_hetero_track_mixed36', 12), ('F6_orcalp_circle100_long', 30)]
SOME_DONE = ('F4_sca_takeoff16', 'F4_mixed_takeoff16', 'paths/F19_path_edge10')


def test_recorded_episodes_resumed_in_another_context(S):
    """The six episodes run in slots of 100; each is saved behind its k-th step and resumed in a second context -- slots of 130, the slot
    order reversed, other obstacle bases -- whose other slots are at other points of their own episodes.  From the resume on the resumed
    slot is held against the reference's records and, at every step to the end of the recording, against the source batch running on."""
    eps = [recorded(n) for n, _ in RECORDED]
    ks = [k for _, k in RECORDED]
    src = Batch(S, eps, cap=100)
    dst = Batch(S, [synthetic(S, 4, goal_shift=0.2) for _ in eps], cap=130, ocap=9)
    to = {s: len(eps) - 1 - s for s in range(len(eps))}
    last = max(int(e['fx']['step'][-1]) for e in eps) + 1
    records = {s: 0 for s in to}
    try:
        for t in range(last + 1):
            if t:
                src.step(), dst.step()
            now = [s for s in to if ks[s] == t]
            on = [s for s in to if ks[s] < t]
            if not now and not on:
                continue
            want = src.views(now + on)
            for s in now:                                             # what makes this k worth saving at, asserted from the recording
                e, name = eps[s], RECORDED[s][0]
                flags = e['fx']['flags'][e['index'][t]]
                assert np.array_equal(want[s]['flags'], flags), (name, 'the source is the recording at k')
                if name in SOME_DONE:
                    assert (flags & 7).any() and not (flags & 7).all(), (name, 'some done, some live')
                if name.startswith('F4'):
                    assert (want[s]['replans'][U.tracked(e)] > 0).any(), (name, 're-plans')
                if 'path_off' in e['fx']:
                    left, length = e['fx']['path_left_before'][e['index'][t]], np.diff(e['fx']['path_off'])
                    assert ((left > 0) & (left < length)).any(), (name, 'a list partly popped')
                    assert np.array_equal(want[s]['remaining'], left)
                dst.resume({to[s]: e}, src.sol.save_scenes([s]))
            got = dst.views([to[s] for s in now + on])
            for s in now:
                same_scene(want[s], got[to[s]], ('at the load', t, RECORDED[s][0]), STATE)
            for s in on:
                ctx = ('step', t, RECORDED[s][0])
                same_scene(want[s], got[to[s]], ctx)
                records[s] += check_record(got[to[s]], eps[s], t, ctx)
        # every resumed episode met its records behind k: all of them for the episodes recorded step by step, the strided one's rows
        assert [records[s] for s in range(6)] == [85, 181, 54, 20, 18, 57], records
    finally:
        src.close(), dst.close()


# ---- 2: the edges of k ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['F1_sca_circle8', 'paths/F19_path_rvo_circle16'])
@pytest.mark.parametrize('k', [0, 1])
def test_saved_before_any_step_and_behind_the_first(S, name, k):
    """k = 0: the blob of a scene that has not stepped (its counters come from the recount); k = 1: every agent's first step is behind it,
    the bootstrap rule of the policies is not.  20 steps behind the load, against the source and the records."""
    e = recorded(name)
    src = Batch(S, [synthetic(S, 9, seed=1), e], cap=16, W=4)
    dst = Batch(S, [e, synthetic(S, 7, seed=2, W=3)], cap=20, W=5, ocap=2)
    try:
        if k:
            src.step(), dst.step()
        dst.put({0: synthetic(S, 11, seed=3)})                       # (the slot held something else in between)
        dst.resume({0: e}, src.sol.save_scenes([1]))
        same_scene(src.views([1])[1], dst.views([0])[0], (name, k, 'at the load'), STATE)
        seen = 0
        for t in range(k + 1, k + 21):
            src.step(), dst.step()
            got = dst.views([0])[0]
            same_scene(src.views([1])[1], got, (name, k, 'step', t))
            seen += check_record(got, e, t, (name, k, 'step', t))
        assert seen >= 10
    finally:
        src.close(), dst.close()


def test_a_finished_scene(S):
    """F1_sca_circle8 run to its end, then saved: the resumed scene loads with active == 0, stays inert, keeps the source's steps and is
    not harvested a second time"""
    e = recorded('F1_sca_circle8')
    done = int(e['fx']['done_step'])
    src = Batch(S, [e], cap=8, harvest=True)
    dst = Batch(S, [synthetic(S, 10, seed=1), synthetic(S, 8, seed=2)], cap=12, harvest=True)
    try:
        src.step(done + 1)
        assert src.sol.scene_harvest_collect() == [0]
        sc = src.sol.scene_state()
        assert sc['active'][0] == 0 and sc['steps'][0] == done + 1
        dst.step(3)
        dst.resume({1: e}, src.sol.save_scenes([0]))
        want = src.views([0])[0]
        same_scene(want, dst.views([1])[1], ('finished', 'at the load'), STATE)
        assert dst.sol.scene_state()['active'].tolist() == [10, 0] and dst.sol.active_count() == 10
        for t in range(3):
            dst.step()
            got = dst.views([1])[1]
            same_scene(want, got, ('finished', 'inert', t), STATE)
            assert not got['action'].any() and dst.sol.scene_harvest_collect() == []
        assert check_record(dst.views([1])[1], e, done + 1, ('finished',), outputs=False) == 1
    finally:
        src.close(), dst.close()


# ---- 3: a fork inside one context -----------------------------------------------------------------------------------------------------------------
def test_a_fork_inside_one_context(S):
    """scene 0 is saved and scene 2 restarted with the same episode and loaded: the two agree at every step from there; a twin batch that
    never saw the calls agrees on the scenes that were not named at the call and at every step"""
    eps = [synthetic(S, 14, seed=1, W=4), synthetic(S, 9, seed=2, W=3), synthetic(S, 20, seed=3), synthetic(S, 12, seed=4, W=5)]
    b, twin = Batch(S, eps, cap=20, W=5), Batch(S, eps, cap=20, W=5)
    try:
        b.step(7), twin.step(7)
        blob = b.sol.save_scenes([0])
        same_scene_all = lambda ctx, keys=None: [same_scene(x, y, ctx + (s,), keys) for (s, x), y in zip(b.views([0, 1, 3]).items(), twin.views([0, 1, 3]).values())]
        same_scene_all(('the save',))
        b.resume({2: eps[0]}, blob)
        same_scene_all(('the load',))
        v = b.views([0, 2])
        same_scene(v[0], v[2], ('fork', 'at the load'), STATE)
        for t in range(8):
            b.step(), twin.step()
            v = b.views([0, 2])
            same_scene(v[0], v[2], ('fork', 'step', t))
            same_scene_all(('twin', 'step', t))
        assert (v[0]['replans'] > 0).any() and (v[0]['remaining'] < [len(p) for p in eps[0]['paths']]).any()
    finally:
        b.close(), twin.close()


# ---- 4: sizes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('policy,W', [(0, 0), (3, 4)])
def test_sizes_around_the_wavefront_and_the_workgroup(S, policy, W):
    """1, 63, 64, 65 and 129 agents (SCA with the tracker; ORCA3D with lists in slot form): six steps, the save, six steps behind a resume in
    slots of 130 of another context in another order, against the source and against a context of each episode alone"""
    sizes = [1, 63, 64, 65, 129]
    eps = [synthetic(S, n, seed=i, policy=[policy], W=W) for i, n in enumerate(sizes)]
    src = Batch(S, eps, cap=129, W=max(W, 1))
    dst = Batch(S, [synthetic(S, 5, seed=9) for _ in sizes], cap=130, W=max(W, 1) + 1)
    solos = [P.alone(S, e) for e in eps]
    to = [3, 0, 4, 1, 2]
    try:
        src.step(6), dst.step(6)
        for x in solos:
            x.run_steps(6, S.NBR_KDTREE)
        dst.resume({to[s]: e for s, e in enumerate(eps)}, [b for _, b in sorted(zip(to, src.sol.save_scenes(list(range(5)))))])
        for t in range(6):
            src.step(), dst.step()
            U.step_all(S, *solos)
            want, got = src.views(), dst.views()
            for s, e in enumerate(eps):
                same_scene(want[s], got[to[s]], ('size', e['n'], 'step', t))
            held = {to[s]: e for s, e in enumerate(eps)}
            U.assert_slots_equal_alone(dst.sol, dst.off, held, {to[s]: x for s, x in enumerate(solos)}, ('alone', t), dst.obs_lo)
            U.assert_vacant(U.everything(dst.sol), dst.off, [held[s]['n'] for s in range(5)], ('vacant', t))
    finally:
        for x in [src.sol, dst.sol] + solos:
            x.close()


# ---- 5: every step form, the log per scene and the harvest behind a load ---------------------------------------------------------------------
@pytest.mark.parametrize('form', ['run_steps_1', 'run_steps_3', 'env_step', 'step_host'])
def test_every_step_form_behind_a_load(S, form):
    """three full slots of 12 (step_host needs a batch at capacity), the log per scene and the harvest on.  Slot 1's episode -- every goal
    1.5 m away, RVO3D agents, it finishes some steps behind the save -- is saved behind six steps and resumed in slot 2 of a second batch; both step on in
    the form.  Rows >= k of the log and the harvest's summary at the finish equal the source's."""
    k = 6
    eps = [synthetic(S, 12, seed=1), synthetic(S, 12, seed=2, policy=[1], goal_shift=1.5), synthetic(S, 12, seed=3)]
    other = [synthetic(S, 12, seed=4), synthetic(S, 12, seed=5), synthetic(S, 12, seed=6)]
    src, dst = Batch(S, eps, cap=12, log=40, harvest=True), Batch(S, other, cap=12, log=40, harvest=True)
    step = {'run_steps_1': lambda x: (x.run_steps(1, S.NBR_KDTREE), x.synchronize()), 'run_steps_3': lambda x: (x.run_steps(3, S.NBR_KDTREE), x.synchronize()),
            'env_step': lambda x: x.env_step(S.NBR_KDTREE), 'step_host': lambda x: x.step_host(S.NBR_KDTREE, state=False)}[form]
    try:
        if form == 'step_host':
            src.sol.host_state(), dst.sol.host_state()
        src.step(k), dst.step(k)
        assert src.sol.scene_state()['active'][1] > 0
        dst.resume({2: eps[1]}, src.sol.save_scenes([1]))
        finished = None
        for t in range(20):
            if finished is not None and t > finished + 2:
                break
            step(src.sol), step(dst.sol)
            same_scene(src.views([1])[1], dst.views([2])[2], (form, 'call', t))
            a, b = src.sol.scene_harvest_collect(), dst.sol.scene_harvest_collect()
            if 1 in a:
                assert 2 in b and finished is None
                finished = t
                ha, hb = src.sol.scene_harvest(), dst.sol.scene_harvest()
                for key in ha['summary'].dtype.names:
                    assert ha['summary'][1][key].tolist() == hb['summary'][2][key].tolist(), (form, 'summary', key)
                for key in ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num'):
                    assert np.array_equal(ha[key][12:24], hb[key][24:36]), (form, 'harvested rows', key)
        assert finished is not None, 'the episode did not finish behind the save'
        steps = int(src.sol.scene_state()['steps'][1])
        assert steps > k and int(dst.sol.scene_state()['steps'][2]) == steps
        want, got = src.sol.scene_history(1, first_row=k), dst.sol.scene_history(2, first_row=k)
        assert len(want['pos']) == steps - k
        for key in want:
            assert np.array_equal(want[key], got[key]), (form, 'log rows >= k', key)
    finally:
        src.close(), dst.close()


# ---- 6: every refusal leaves the context as it was ------------------------------------------------------------------------------------------
def seal(blob):
    """the header's checksum from the bytes as they stand: FNV-1a over the 64-bit words behind the 64-byte header"""
    h = 0xcbf29ce484222325
    for w in blob[64:].view('<u8'):
        h = ((h ^ int(w)) * 0x100000001b3) % 2 ** 64
    blob[56:64] = np.frombuffer(np.uint64(h).tobytes(), np.uint8)
    return blob


def damaged(blob, edits, resealed=True):
    b = blob.copy()
    for at, v in edits:
        b[at] = v
    return seal(b) if resealed else b


def test_refusals_leave_the_context_as_it_was(S):
    eps = [synthetic(S, 8, seed=1, W=3), recorded('F1_sca_circle8'), synthetic(S, 5, seed=2, policy=[1, 3])]
    b = Batch(S, eps, cap=8, W=3)
    bare = Batch(S, [eps[1]], cap=8, tracker=False, path_slots=False)      # no tracker, no lists
    try:
        b.step(4), bare.step(4)
        before = U.observe(b.sol)
        good = b.sol.save_scenes([0, 1])
        info = [S.scene_checkpoint_info(x) for x in good]
        assert [i['size'] for i in info] == [8, 8] and all(i['has_tracker'] == 1 and i['has_paths'] == 1 and i['steps'] == 4 for i in info)
        assert [len(x) for x in good] == [b.sol.scene_checkpoint_bytes(0), b.sol.scene_checkpoint_bytes(1)] == [i['total_bytes'] for i in info]
        off = info[0]['offsets']
        tw = info[0]['trk_words']

        def refused(fn, code, *words):
            with pytest.raises(S.ScaError) as err:
                fn()
            msg = str(err.value)
            assert msg.endswith('(rc=%d)' % code) and all(w in msg for w in words), msg
            U.same(before, U.observe(b.sol), ('refused', msg))
        load = lambda blob, s=0: (lambda: b.sol.load_scenes([s], [blob]))
        # the calls' arguments
        for who, fn in (('sca_save_scenes', lambda ids: b.sol.save_scenes(ids)), ('sca_load_scenes', lambda ids: b.sol.load_scenes(ids, good[:len(ids)]))):
            refused(lambda: fn([]), ERR_ARG, who, 'count')
            refused(lambda: fn([3]), ERR_ARG, who, 'scene_ids[0] = 3')
            refused(lambda: fn([0, -1]), ERR_ARG, who, 'scene_ids[1] = -1')
            refused(lambda: fn([1, 1]), ERR_ARG, who, 'named twice')
        refused(lambda: b.sol._save_into(np.array([1], np.int32), [np.zeros(len(good[1]) - 1, np.uint8)]), ERR_ARG, 'sca_save_scenes', 'needs %d' % len(good[1]))
        # between a policy pass and its env update
        b.sol.policy_pass(S.NBR_KDTREE)
        for fn, who in ((lambda: b.sol.save_scenes([0]), 'sca_save_scenes'), (load(good[0]), 'sca_load_scenes')):
            with pytest.raises(S.ScaError) as err:
                fn()
            assert str(err.value).endswith('(rc=%d)' % ERR_STATE) and who in str(err.value)
        b.sol.env_update()
        before = U.observe(b.sol)
        good = b.sol.save_scenes([0, 1])
        # the envelope
        refused(load(damaged(good[0], [(0, 0)])), ERR_ARG, 'sca_load_scenes', 'magic')
        refused(load(damaged(good[0], [(4, 2)])), ERR_ARG, 'format version')
        refused(load(good[0][:-16]), ERR_ARG, 'byte count')
        refused(load(np.concatenate([good[0], np.zeros(16, np.uint8)])), ERR_ARG, 'byte count')
        refused(load(damaged(good[0], [(off[SEC['heading']] + 1, good[0][off[SEC['heading']] + 1] ^ 1)], resealed=False)), ERR_ARG, 'checksum')
        refused(load(damaged(good[0], [(16, tw - 1)])), ERR_ARG, 'record')
        refused(load(damaged(good[0], [(20, 40)])), ERR_ARG, 'record')
        # the blob against the scene
        refused(load(good[0], 2), ERR_ARG, "scene's current size")                              # scene 2 holds five agents
        refused(load(good[0], 1), ERR_ARG, 'policy')                                            # the mixed episode into the SCA scene
        with pytest.raises(S.ScaError) as err:                                                  # tracker records into a context without a tracker
            bare.sol.load_scenes([0], [good[1]])
        assert 'tracker records' in str(err.value) and str(err.value).endswith('(rc=%d)' % ERR_ARG)
        plain = bare.sol.save_scenes([0])[0]                                                    # ... and none where the scene needs them
        assert S.scene_checkpoint_info(plain)['has_tracker'] == 0 and S.scene_checkpoint_info(plain)['has_paths'] == 0
        refused(load(plain, 1), ERR_ARG, 'tracker records')
        rem = off[SEC['rem']]
        left = good[0][rem:rem + 32].view('<i4')
        row = int(np.argmax(left > 0))
        assert left[row] > 0
        mixed_only = Batch(S, [eps[0]], cap=8, tracker=True, path_slots=False)                  # the same episode, no lists set
        try:
            with pytest.raises(S.ScaError) as err:
                mixed_only.sol.load_scenes([0], [good[0]])
            assert 'no waypoint lists' in str(err.value) and 'row %d' % row in str(err.value)
        finally:
            mixed_only.close()
        refused(load(damaged(good[0], [(rem + 4 * row, 4)])), ERR_ARG, 'row %d' % row, 'cursor')          # four left of a list of at most three
        # the payload
        perm = off[SEC['perm']]
        first = int(good[0][perm:perm + 4].view('<i4')[0])
        refused(load(damaged(good[0], [(perm + 4, first)])), ERR_ARG, 'permutation')                      # positions 0 and 1 hold the same row
        refused(load(damaged(good[0], [(perm, 8)])), ERR_ARG, 'permutation')
        rec = off[SEC['rec']]
        refused(load(damaged(good[0], [(rec + 48 * 2 + 36, good[0][rec + 48 * 2 + 36] | 16)])), ERR_ARG, 'row 2', 'flag bits')
        refused(load(damaged(good[0], [(rec + 48 * 5 + 14, 0xf0), (rec + 48 * 5 + 15, 0x7f)])), ERR_ARG, 'row 5', 'not finite')     # y = inf or NaN
        trk = [int(a) for a in U.tracked(eps[0])]
        track = off[SEC['track']] + 4 * tw * trk[0]
        refused(load(damaged(good[0], [(track + 376 + 7, 0x80)])), ERR_ARG, 'row %d' % trk[0], 'tracker record')                    # a negative cursor
        refused(load(damaged(good[0], [(track + 376 + 2, 0x7f)])), ERR_ARG, 'row %d' % trk[0], 'tracker record')                    # a cursor far behind the samples
        # and the good blobs still load
        b.sol.load_scenes([0, 1], good)
        U.same(before, U.observe(b.sol), ('a scene loaded with its own blob',))
    finally:
        b.close(), bare.close()


def test_refusals_without_scenes_and_without_a_state(S):
    e = synthetic(S, 6, seed=1)
    sol = S.BatchedSolver(max_agents=6, max_obstacles=1)
    try:
        sol.set_agents(e['radius'], e['pref_speed'], e['goal'], e['policy'], e['zaxis'], e['max_run_dist'])
        blob = np.zeros(64, np.uint8)
        assert U.rc_of(S, lambda: sol._save_into(np.array([0], np.int32), [blob])) == ERR_STATE
        assert U.rc_of(S, lambda: sol.load_scenes([0], [blob])) == ERR_STATE
        sol.set_scenes(np.array([0, 6], np.int32))
        assert U.rc_of(S, lambda: sol._save_into(np.array([0], np.int32), [blob])) == ERR_STATE                # no state yet
        assert U.rc_of(S, lambda: sol.load_scenes([0], [blob])) == ERR_STATE
    finally:
        sol.close()


# ---- 7: another process -------------------------------------------------------------------------------------------------------------------------
CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_scene_checkpoint as T
mods = T.python_mods()
batch = T.recorded_batch(mods, 'F4_sca_takeoff16')
for _ in range(200):
    batch.step()
assert int(batch.steps[0]) == 200 and 0 < int(batch.active[0]) < 16
batch.checkpoint(0).write(sys.argv[2])
batch.close()
print('written')
'''


def python_mods():
    from sca_amd import env as E, metrics, scenes
    return E, metrics, scenes


def recorded_agents(E, fx):
    """the agents and obstacles of a recorded episode, as the reference's scripts build them"""
    from golden_util import static_inputs
    st = static_inputs(fx)
    pol = {c.policy_id: c for c in (E.SCAPolicy, E.RVO3DPolicy, E.SRVO3DPolicy, E.ORCA3DPolicy, E.ORCA3DPolicyOfficial, E.RVO3dDubinsPolicy)}
    agents = [E.Agent(start_pos=list(fx['start'][i]), goal_pos=list(fx['goal6'][i]), vel=[0.0, 0.0, 0.0], radius=float(st['radius'][i]),
                      pref_speed=float(st['pref_speed'][i]), policy=pol[int(st['policy'][i])], id=i) for i in range(len(st['radius']))]
    for a, d in zip(agents, st['max_run_dist']):
        a.max_run_dist = float(d)
    obs = [E.Obstacle(list(map(float, p)), dict(shape='sphere', feature=float(r)), id=i)
           for i, (p, r) in enumerate(zip(st['obs_pos'].reshape(-1, 3), st['obs_radius']))]
    return agents, obs


def recorded_batch(mods, name, extra=(), **kw):
    """a SceneBatch whose scene 0 is the recorded episode (obstacle slots of 8, capacities of 20); extra: further Agent lists"""
    E, metrics, scenes = mods
    agents, obs = recorded_agents(E, U.load_any(name))
    lists = [agents] + [list(x) for x in extra]
    return scenes.SceneBatch(lists, scene_obstacles=[obs] + [[] for _ in extra], obstacle_capacities=[8] * len(lists), capacities=[20] * len(lists),
                             device_tracker=True, **kw)


def test_an_episode_written_by_another_process(tmp_path):
    """a fresh child process steps F4_sca_takeoff16 to its step 200 and writes the checkpoint; this process reads the file, resumes the
    episode in another slot of a batch that is busy with another episode, and finishes it: the final state and the metrics are the
    recording's and those of the episode run here without a break"""
    mods = python_mods()
    E, metrics, scenes = mods
    path = str(tmp_path / 'takeoff.npz')
    run = subprocess.run([sys.executable, '-c', CHILD, ROOT, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and 'written' in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
    ck = scenes.SceneCheckpoint.read(path)
    fx = U.load_any('F4_sca_takeoff16')
    assert ck.steps == 200 and len(ck) == 16 and len(ck.obstacles()) == 8
    whole = recorded_batch(mods, 'F4_sca_takeoff16')
    batch = recorded_batch(mods, 'F1_sca_circle8', extra=[E.build_circle_agents(12, policy=E.RVO3DPolicy)])
    try:
        for _ in range(5):
            batch.step()
        batch.restart({1: ck})
        assert int(batch.steps[1]) == 200 and int(batch.active[1]) == int(((fx['flags'][200] & 7) == 0).sum())
        while not whole.done[0]:
            whole.step()
        while not batch.done[1]:
            batch.step()
        last = len(fx['step']) - 1
        view, ref = batch.env(1), whole.env(0)
        assert int(batch.steps[1]) == int(whole.steps[0]) == int(fx['done_step']) + 1
        for key, rec in (('pos', 'pos_after'), ('heading', 'heading_after'), ('flags', 'flags_after'), ('total_dist', 'total_dist_after')):
            assert np.array_equal(getattr(view, key), fx[rec][last]) and np.array_equal(getattr(view, key), getattr(ref, key)), key
        assert np.array_equal(view.step_num, ref.step_num) and np.array_equal(view.vel, ref.vel)
        m, w = metrics.episode_metrics(view), metrics.episode_metrics(ref)
        assert set(m) == set(w) and all(np.array_equal(m[k], w[k], equal_nan=True) for k in m if k != 'AverageCost'), (m, w)
    finally:
        whole.close(), batch.close()


# ---- 8: the Python layers -------------------------------------------------------------------------------------------------------------------------
def circle_agents(E, n, policy, seed, waypoints=0):
    from sca_amd import scenarios
    sc = scenarios.random_cube(n, seed=seed)
    agents = [E.Agent(start_pos=list(sc['start'][i]), goal_pos=list(sc['goal'][i]), vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0, policy=policy, id=i)
              for i in range(n)]
    rng = np.random.default_rng(300 + seed)
    for a in agents[:waypoints]:
        p, g = a.initial_pos[:3], a.goal_pos[:3]
        a.path = [[float(x) for x in np.round(p + (g - p) * f + rng.normal(0, 1.0, 3), 3)] for f in (0.7, 0.4, 0.2)]
    return agents


def test_the_mirrors_and_the_stitched_log_behind_a_restart_from_a_checkpoint(tmp_path):
    """SceneBatch.checkpoint(s) -> write -> read -> SceneBatch.restart({s: checkpoint}) in another batch: agent.pos_global_frame, path,
    policy.now_goal and .steps[s] show the checkpoint's values at once; from there the two scenes agree, and metrics.trajectories of the
    resumed scene is the whole episode -- the saved rows in front of the device's"""
    E, metrics, scenes = python_mods()
    mk = lambda: [circle_agents(E, 14, E.RVO3DPolicy, 1, waypoints=6), circle_agents(E, 10, E.SCAPolicy, 2)]
    src = scenes.SceneBatch(mk(), device_tracker=True, capacities=[16, 16], path_slots=3, scene_history=80)
    dst = scenes.SceneBatch([circle_agents(E, 9, E.SCAPolicy, 3), circle_agents(E, 7, E.RVO3DPolicy, 4)], device_tracker=True, capacities=[16, 16],
                            path_slots=4, scene_history=80)
    try:
        for _ in range(12):
            src.step(), dst.step()
        ck = scenes.SceneCheckpoint.read(src.checkpoint(0).write(str(tmp_path / 'a.npz')))
        assert ck.steps == 12 and ck.log['pos'].shape == (12, 14, 3)
        dst.restart({1: ck})
        a, b = src.env(0), dst.env(1)
        assert int(dst.steps[1]) == 12 and int(dst.active[1]) == int(src.active[0])
        popped = 0
        for x, y in zip(a.agents, b.agents):
            assert np.array_equal(x.pos_global_frame, y.pos_global_frame) and np.array_equal(x.vel_global_frame, y.vel_global_frame)
            assert x.path == y.path and x.step_num == y.step_num == 12
            assert np.array_equal(x.policy.now_goal, y.policy.now_goal)
            popped += 3 - len(x.path) if x.id < 6 else 0
        assert popped > 0, 'no list was partly popped at the save'
        for t in range(30):
            src.step(), dst.step()
            for key in ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num'):
                assert np.array_equal(getattr(a, key), getattr(b, key)), (t, key)
            assert [x.path for x in a.agents] == [y.path for y in b.agents] and a.kdTree.agentIDs == b.kdTree.agentIDs
        assert np.array_equal(metrics.trajectories(a), metrics.trajectories(b)) and metrics.trajectories(b).shape[:2] == (14, 42)
        paths = metrics.write_episode_log(b, str(tmp_path / 'log'), xlsx=False)
        assert np.array_equal(np.load(paths['trajs'])['agent3'], metrics.trajectories(a)[3])
        # what a slot cannot take is refused before any device call
        small = scenes.SceneBatch([circle_agents(E, 5, E.RVO3DPolicy, 5)], device_tracker=True)
        try:
            with pytest.raises(ValueError):
                small.restart({0: ck})
        finally:
            small.close()
    finally:
        src.close(), dst.close()


def test_a_queue_finished_across_two_runs(tmp_path):
    """eight 20-agent episodes through four slots: run_episodes(checkpoint_at=(60, dir)) stops behind 60 batch steps; a second run over the
    written checkpoints, in slot order, plus the pending episodes gives the results, the on_done contents and the final states of one
    uninterrupted run"""
    E, metrics, scenes = python_mods()
    pols = [E.SCAPolicy, E.RVO3DPolicy, E.ORCA3DPolicyOfficial, E.RVO3dDubinsPolicy]
    mk = lambda: [circle_agents(E, 20, pols[i % 4], 10 + i, waypoints=4 if i % 2 else 0) for i in range(8)]
    seen_whole, seen_a, seen_b, stats = [], [], [], {}
    whole = scenes.run_episodes(mk(), 4, device_tracker=True, on_done=seen_whole.append, path_slots=3, history_rows=1500)
    first = scenes.run_episodes(mk(), 4, device_tracker=True, on_done=seen_a.append, path_slots=3, history_rows=1500, stats=stats,
                                checkpoint_at=(60, str(tmp_path)))
    assert stats['batch_steps'] == 60 and sorted(stats['checkpoints']) == [0, 1, 2, 3]
    order = [i for _, (i, _) in sorted(stats['checkpoints'].items())] + stats['pending']
    assert all(first[i] is None for i in order) and sorted(order + [r['episode'] for r in seen_a]) == list(range(8))
    fresh = mk()
    queue = [scenes.SceneCheckpoint.read(path) for _, (_, path) in sorted(stats['checkpoints'].items())] + [fresh[i] for i in stats['pending']]
    assert any(0 < ck.steps for ck in queue[:4])
    second = scenes.run_episodes(queue, 4, device_tracker=True, on_done=seen_b.append, path_slots=3, history_rows=1500)
    got = {r['episode']: r for r in seen_a}
    got.update({order[r['episode']]: r for r in seen_b})
    assert [r is not None for r in second] == [True] * len(order)
    for w in seen_whole:
        g = got[w['episode']]
        assert g['steps'] == w['steps'] and g['slot'] == w['slot'] and g['path_left'] == w['path_left'], w['episode']
        for key in w['metrics']:
            if key != 'AverageCost':
                assert np.array_equal(g['metrics'][key], w['metrics'][key], equal_nan=True), (w['episode'], key)
        for key in w['state']:
            assert np.array_equal(g['state'][key], w['state'][key]), (w['episode'], key)
        assert np.array_equal(g['trajectories'], w['trajectories']) and g['rows_dropped'] == w['rows_dropped'] == 0, w['episode']
    assert [order[r['episode']] for r in seen_b] == [r['episode'] for r in seen_whole[len(seen_a):]]      # ... in the order one run finishes them


def test_the_example_finishes_its_table_across_two_runs(tmp_path):
    """examples/run_scenes.py --save-at / --resume: the rows of the two runs together are the rows of one run"""
    base = [sys.executable, os.path.join(ROOT, 'examples', 'run_scenes.py'), '--agents', '12', '--seeds', '1', '--slots', '4', '--waypoints', '2']
    rows = lambda out: [line for line in out.split('\n') if ' slot ' in line and ' steps ' in line]

    def run(extra):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout
    one = rows(run([]))
    first = run(['--save-at', '40', '--save-dir', str(tmp_path / 'ck')])
    assert 'stopped behind 40 batch steps' in first
    second = run(['--resume', str(tmp_path / 'ck')])
    assert len(one) == 12 and rows(first) + rows(second) == one
