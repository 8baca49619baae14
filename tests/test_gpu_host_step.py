"""sca_step_host on the GPU (-m gpu): the env loop with the HOST as the owner of the state (mampenv.py:27-59) -- a pinned state block the caller
reads and writes in place and one call per step -- against the resident loop, against INTEGRATION.md's five-call stub B and against a recorded
episode of the reference.  Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

from golden_util import fixture_params, load, static_inputs

pytestmark = pytest.mark.gpu

STATE_KEYS = ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num')
OK, ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 0, -1, -3, -5


@pytest.fixture(scope='module')
def S():
    import sca_amd.solver as S
    return S


def _scene(S, scene):
    """the three scenes of test_host_buffer_loop_of_integration_stub_b_equals_the_resident_loop (tests/test_gpu_parity.py)"""
    from sca_amd import scenarios
    if scene == 'sca_circle_tracker':
        sc, n, policy, tracked = scenarios.circle(300), 300, np.zeros(300, np.uint8), True
    elif scene == 'mixed_takeoff_obstacles':
        sc = scenarios.takeoff_landing(160)
        n = len(sc['start'])
        policy, tracked = np.where(np.arange(n) % 2 == 0, 0, 2).astype(np.uint8), True
    else:
        sc, n, policy, tracked = scenarios.random_cube(700, seed=5), 700, np.full(700, 3, np.uint8), False
    zaxis = S.zaxis_flags(sc['start'], sc['goal'])
    mrd = scenarios.max_run_dist(sc['start'], sc['goal'])

    def mk(with_state=True, max_agents=None, device_tracker=True):
        sol = S.BatchedSolver(max_agents=max_agents or n, max_obstacles=max(1, len(sc['obs_radius'])))
        sol.set_obstacles(sc['obs_pos'], sc['obs_radius'])
        sol.set_agents(np.full(n, 0.5), np.ones(n), sc['goal'][:, :3], policy, zaxis, mrd)
        if with_state:
            sol.set_state(sc['start'][:, :3], np.zeros((n, 3), np.float32), sc['start'][:, 3:6], np.zeros(n, np.uint8))
        if tracked and device_tracker:
            sol.device_tracker_enable(sc['goal'][:, 3:6])
        return sol
    return sc, n, policy, tracked, mk


def _write_start(blk, sc, n):
    blk['pos'][:] = sc['start'][:, :3]
    blk['vel'][:] = 0
    blk['heading'][:] = sc['start'][:, 3:6]
    blk['flags'][:] = 0
    blk['total_dist'][:] = 0
    blk['step_num'][:] = 0


def _same(a, blk, ctx):
    ra = a.get_state()
    for k in STATE_KEYS:
        assert np.array_equal(ra[k], blk[k]), ctx + (k,)
    assert np.array_equal(a.actions(), blk['action']), ctx + ('action',)


def test_the_block_is_views_of_one_allocation_in_the_layout(S):
    from sca_amd import _lib
    sc, n, policy, tracked, mk = _scene(S, 'orca_random')
    b = mk(with_state=False)
    blk = b.host_state()
    assert blk is b.host_state()                                  # made once per set_agents
    off = (C.c_int64 * 9)()
    total = C.c_int64(0)
    assert _lib.lib().sca_host_state_layout(n, off, C.byref(total)) == 0
    keys = ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num', 'vpref', 'vpref_mode', 'action')
    base = blk['pos'].ctypes.data
    assert [blk[k].ctypes.data - base for k in keys] == [int(x) for x in off]
    want = dict(pos=((n, 3), np.float64), vel=((n, 3), np.float32), heading=((n, 3), np.float64), flags=((n,), np.uint8),
                total_dist=((n,), np.float64), step_num=((n,), np.int32), vpref=((n, 3), np.float64), vpref_mode=((n,), np.uint8),
                action=((n, 7), np.float32))
    for k in keys:
        assert (blk[k].shape, blk[k].dtype) == (want[k][0], np.dtype(want[k][1])) and blk[k].flags.writeable and not blk[k].flags.owndata, k
        assert not blk[k].any(), k                                # the block starts zeroed
    b.close()


@pytest.mark.parametrize('form', ['direct', 'staged'])
@pytest.mark.parametrize('feed', ['state_every_step', 'state_once'])
@pytest.mark.parametrize('mode', ['kd', 'auto'])
@pytest.mark.parametrize('scene', ['sca_circle_tracker', 'mixed_takeoff_obstacles', 'orca_random'])
def test_block_loop_walks_through_the_resident_loops_states(S, scene, mode, feed, form, monkeypatch):
    """context A: sca_run_steps(1); context B: sca_step_host on its block -- with SCA_HOST_IN_STATE every step (the block as the step left it goes
    up again), or on the first call only and in_mask == 0 afterwards.  After every step the block IS A's state, its action rows are A's, the kd
    permutation is A's and the returned count is A's; at the end the tracker's re-plan counts.  `direct`: the form that ships (the two kernels
    read and write the page-locked block across the link); `staged`: SCA_HOST_STEP_STAGED=1, copies into / out of a device staging buffer."""
    nbr = S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE
    sc, n, policy, tracked, mk = _scene(S, scene)
    a = mk()
    if form == 'staged':
        monkeypatch.setenv('SCA_HOST_STEP_STAGED', '1')         # read by sca_create
    b = mk(with_state=False)
    monkeypatch.delenv('SCA_HOST_STEP_STAGED', raising=False)
    blk = b.host_state()
    _write_start(blk, sc, n)
    for t in range(25):
        a.run_steps(1, nbr)
        a.synchronize()
        active = b.step_host(nbr, state=(feed == 'state_every_step' or t == 0))
        _same(a, blk, (scene, mode, feed, t))
        assert active == a.active_count() == int(((blk['flags'] & 7) == 0).sum()), (scene, mode, feed, t)
        assert np.array_equal(a.get_kd_perm(), b.get_kd_perm()), (scene, mode, feed, t)
    if tracked:
        assert np.array_equal(a.device_tracker_replans(), b.device_tracker_replans())
    assert ((blk['flags'] & 7) == 0).any()                      # (the loop was still doing something at the end)
    a.close()
    b.close()


@pytest.mark.parametrize('form', ['direct', 'staged'])
@pytest.mark.parametrize('mode', ['kd', 'auto'])
def test_the_host_has_the_last_word(S, mode, form, monkeypatch):
    """at steps 5 and 12 the host moves 10 agents, retires 5 (flags, velocity zero) in the block and says so; A gets the same edit through
    sca_get_state / sca_set_state.  In between B runs with in_mask == 0."""
    nbr = S.NBR_AUTO if mode == 'auto' else S.NBR_KDTREE
    sc, n, policy, tracked, mk = _scene(S, 'mixed_takeoff_obstacles')
    a = mk()
    if form == 'staged':
        monkeypatch.setenv('SCA_HOST_STEP_STAGED', '1')
    b = mk(with_state=False)
    monkeypatch.delenv('SCA_HOST_STEP_STAGED', raising=False)
    blk = b.host_state()
    _write_start(blk, sc, n)
    rng = np.random.default_rng(3)
    for t in range(25):
        edit = t in (5, 12)
        if edit:
            ids = rng.permutation(n)[:15]
            move, retire = ids[:10], ids[10:]
            shift = rng.uniform(-0.4, 0.4, (10, 3))
            st = a.get_state()
            for tgt in (st, blk):
                tgt['pos'][move] += shift
                tgt['flags'][retire] |= S.FLAG_AT_GOAL
                tgt['vel'][retire] = 0
            a.set_state(st['pos'], st['vel'], st['heading'], st['flags'], st['total_dist'], st['step_num'])
        a.run_steps(1, nbr)
        a.synchronize()
        active = b.step_host(nbr, state=(t == 0 or edit))
        _same(a, blk, (mode, t))
        assert active == a.active_count(), (mode, t)
        assert np.array_equal(a.get_kd_perm(), b.get_kd_perm()), (mode, t)
    assert np.array_equal(a.device_tracker_replans(), b.device_tracker_replans())
    assert ((blk['flags'] & 7) == 0).any()
    a.close()
    b.close()


@pytest.mark.parametrize('form', ['direct', 'staged'])
def test_vpref_through_the_block_equals_sca_set_vpref_and_stub_b(S, form, monkeypatch):
    """the host tracker's v_pref (sca_tracker_vpref) written into the block every step against a context fed through sca_set_vpref + the five
    calls of stub B; no device tracker on either side."""
    from sca_amd.tracker import DubinsTracker
    sc, n, policy, tracked, mk = _scene(S, 'sca_circle_tracker')
    a = mk(device_tracker=False)
    if form == 'staged':
        monkeypatch.setenv('SCA_HOST_STEP_STAGED', '1')
    b = mk(with_state=False, device_tracker=False)
    monkeypatch.delenv('SCA_HOST_STEP_STAGED', raising=False)
    zaxis = S.zaxis_flags(sc['start'], sc['goal'])
    trk = [DubinsTracker(sc['goal'][:, :3], sc['goal'][:, 3:6], np.ones(n), zaxis, nthreads=8) for _ in range(2)]
    blk = b.host_state()
    _write_start(blk, sc, n)
    blk['vpref_mode'][:] = 1
    st = a.get_state()
    seen = False
    for t in range(25):
        va = trk[0].vpref(st['pos'], st['vel'], st['heading'], ((st['flags'] & 7) == 0).astype(np.uint8))
        a.set_state(st['pos'], st['vel'], st['heading'], st['flags'], st['total_dist'], st['step_num'])
        a.set_vpref(va, np.ones(n, np.uint8))
        a.policy_pass(S.NBR_KDTREE)
        act = a.actions()
        a.env_update(True)
        st = a.get_state()
        trk[0].note_nbr0(a.nbr0())

        blk['vpref'][:] = np.nan_to_num(trk[1].vpref(blk['pos'], blk['vel'], blk['heading'], ((blk['flags'] & 7) == 0).astype(np.uint8)))
        seen = seen or bool(blk['vpref'].any())
        b.step_host(S.NBR_KDTREE, state=True, vpref=True)
        trk[1].note_nbr0(b.nbr0())
        for k in STATE_KEYS:
            assert np.array_equal(st[k], blk[k]), (t, k)
        assert np.array_equal(act, blk['action']), t
        assert np.array_equal(b.diag()['vpref'], a.diag()['vpref']), t
    assert seen and np.array_equal(trk[0].replans(), trk[1].replans())
    a.close()
    b.close()


def test_vpref_mode_for_an_agent_with_a_waypoint_list_is_refused_with_set_vprefs_message(S):
    from sca_amd import scenarios
    n = 40
    sc = scenarios.circle(n)
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
    sol.set_agents(np.full(n, 0.5), np.ones(n), sc['goal'][:, :3], np.full(n, 1, np.uint8), S.zaxis_flags(sc['start'], sc['goal']),
                   scenarios.max_run_dist(sc['start'], sc['goal']))
    paths = [[] for _ in range(n)]
    paths[3] = [[1.0, 2.0, 3.0]]
    sol.set_paths(paths)
    blk = sol.host_state()
    _write_start(blk, sc, n)
    mode = np.zeros(n, np.uint8); mode[3] = 1
    with pytest.raises(S.ScaError) as e1:
        sol.set_vpref(np.zeros((n, 3)), mode)
    blk['vpref_mode'][:] = mode
    with pytest.raises(S.ScaError, match='waypoint') as e2:
        sol.step_host(S.NBR_KDTREE, state=True, vpref=True)
    assert str(e1.value).split(': ', 1)[1] == str(e2.value).split(': ', 1)[1] and 'rc=-1' in str(e2.value)
    blk['vpref_mode'][:] = 0
    blk['vpref_mode'][4] = 1                                     # an agent without a list: accepted
    assert sol.step_host(S.NBR_KDTREE, state=True, vpref=True) > 0
    sol.close()


def test_recorded_episode_of_the_reference_driven_by_step_host_alone(S):
    """tests/golden/F1_sca_circle8.npz, the whole c1 episode (246 steps to `done`), from its start state, device tracker in the pass, set up as
    test_free_running_episode_is_the_reference_bit_for_bit sets it up: after every recorded step the block is the reference's state after that
    step, `action` its rows where find_next_action was called, and the returned count is 0 exactly when nobody is left running."""
    fx = load('F1_sca_circle8')
    st = static_inputs(fx)
    n = len(st['radius'])
    steps = [int(x) for x in fx['step']]
    assert steps == list(range(len(steps))) and len(steps) == 246 and int(fx['done_step']) == 245
    left = [int(((fx['flags_after'][k] & 7) == 0).sum()) for k in range(len(steps))]
    assert [k for k in range(len(steps)) if left[k] == 0] == [245]        # (checked on the CPU: only the last recorded step ends the episode)
    sol = S.BatchedSolver(max_agents=n, max_obstacles=max(len(st['obs_radius']), 1), params=fixture_params(fx)[0])
    sol.set_obstacles(st['obs_pos'], st['obs_radius'])
    sol.set_agents(st['radius'], st['pref_speed'], fx['goal'][0], st['policy'], st['zaxis'], st['max_run_dist'])
    assert st['vpref_mode'].any()
    sol.device_tracker_enable(fx['goal6'][:, 3:6], in_pass=True, **fixture_params(fx)[1])
    blk = sol.host_state()
    blk['pos'][:] = fx['start'][:, :3]
    blk['heading'][:] = fx['start'][:, 3:6]
    for k in steps:
        for key, want in (('pos', fx['pos'][k]), ('heading', fx['heading'][k]), ('total_dist', fx['total_dist'][k]), ('flags', fx['flags'][k]),
                          ('vel', fx['vel'][k])):
            assert np.array_equal(blk[key], want), (k, 'before', key)
        active = sol.step_host(S.NBR_KDTREE, state=(k == 0))
        called = fx['called'][k].astype(bool)
        assert np.array_equal(blk['action'][called], fx['action'][k][called]), (k, 'action')
        for key, want in (('pos', fx['pos_after'][k]), ('vel', fx['vel_after'][k]), ('heading', fx['heading_after'][k]),
                          ('total_dist', fx['total_dist_after'][k]), ('flags', fx['flags_after'][k])):
            assert np.array_equal(blk[key], want), (k, 'after', key)
        assert active == left[k] and (active == 0) == (k == 245), (k, active)
    sol.close()


def test_mixing_with_the_five_calls(S):
    """sca_get_state / sca_get_actions after sca_step_host return what the block holds; a sca_set_state between two sca_step_host calls with
    in_mask == 0 is honoured (the block then shows the step FROM that state)."""
    sc, n, policy, tracked, mk = _scene(S, 'orca_random')
    a, b = mk(), mk(with_state=False)
    blk = b.host_state()
    _write_start(blk, sc, n)
    for t in range(3):
        a.run_steps(1)
        b.step_host(state=(t == 0))
    _same(b, blk, ('own',))
    _same(a, blk, ('resident',))
    st = a.get_state()
    st['pos'][::7] += 0.25
    st['flags'][::50] |= S.FLAG_TIMEOUT
    for sol in (a, b):
        sol.set_state(st['pos'], st['vel'], st['heading'], st['flags'], st['total_dist'], st['step_num'])
    assert not np.array_equal(blk['pos'], st['pos'])              # (sca_set_state does not write the block)
    a.run_steps(1)
    assert b.step_host(state=False) == a.active_count()
    _same(a, blk, ('after set_state',))
    _same(b, blk, ('own after set_state',))
    a.close()
    b.close()


def test_misuse_is_refused_and_the_context_steps_correctly_afterwards(S):
    from sca_amd import _lib
    L = _lib.lib()
    sc, n, policy, tracked, mk = _scene(S, 'orca_random')
    a, b = mk(), mk(with_state=False)
    v = C.c_int(0)

    def refused(rc_want, call):
        rc = call()
        assert rc == rc_want, (rc, rc_want, L.sca_last_error(b.ctx))
        msg = L.sca_last_error(b.ctx).decode()
        assert msg
        return msg

    fresh = S.BatchedSolver(max_agents=n, max_obstacles=1)
    h = _lib.HostState()
    assert L.sca_host_state_get(fresh.ctx, C.byref(h), C.sizeof(h)) == ERR_STATE and L.sca_last_error(fresh.ctx)     # before sca_set_agents
    assert L.sca_step_host(fresh.ctx, 0, 1, C.byref(v)) == ERR_STATE
    fresh.close()
    # before any state, nothing said to have been written
    assert 'state' in refused(ERR_STATE, lambda: L.sca_step_host(b.ctx, 0, 0, C.byref(v)))
    # something said to have been written into a block nobody fetched
    assert 'sca_host_state_get' in refused(ERR_STATE, lambda: L.sca_step_host(b.ctx, 0, 1, C.byref(v)))
    # struct_bytes: negative, too small for the two integers, larger than the library's struct
    for bad in (-8, 0, 4, C.sizeof(h) + 8, 1 << 20):
        assert 'struct_bytes' in refused(ERR_ARG, lambda: L.sca_host_state_get(b.ctx, C.byref(h), bad))
    assert refused(ERR_ARG, lambda: L.sca_host_state_get(b.ctx, None, C.sizeof(h)))
    # a shorter struct of an older caller: only the members that fit are written
    buf = (C.c_ubyte * C.sizeof(h))(*([0xA5] * C.sizeof(h)))
    assert L.sca_host_state_get(b.ctx, C.cast(buf, C.POINTER(_lib.HostState)), 32) == OK
    part = _lib.HostState.from_buffer_copy(bytes(buf))
    assert (part.struct_bytes, part.n) == (32, n) and bytes(buf[32:]) == bytes([0xA5] * (C.sizeof(h) - 32))
    blk = b.host_state()
    assert C.addressof(part.pos.contents) == blk['pos'].ctypes.data and C.addressof(part.heading.contents) == blk['heading'].ctypes.data
    _write_start(blk, sc, n)
    assert refused(ERR_ARG, lambda: L.sca_step_host(b.ctx, 0, 1, None))
    assert refused(ERR_ARG, lambda: L.sca_step_host(b.ctx, 0, 4, C.byref(v)))
    assert 'mode' in refused(ERR_UNSUPPORTED, lambda: L.sca_step_host(b.ctx, 7, 1, C.byref(v))).lower()
    b.set_shard(0, n // 2)
    assert 'shard' in refused(ERR_STATE, lambda: L.sca_step_host(b.ctx, 0, 1, C.byref(v)))
    b.set_shard(0, n)
    b.set_state(sc['start'][:, :3], np.zeros((n, 3), np.float32), sc['start'][:, 3:6], np.zeros(n, np.uint8))   # (the partition wants a state)
    b.partition_init(0, 1)
    assert 'partition' in refused(ERR_UNSUPPORTED, lambda: L.sca_step_host(b.ctx, S.NBR_GRID, 1, C.byref(v)))
    b.partition_disable()
    # none of the refused calls changed anything: the loop equals a context that never saw one
    for t in range(6):
        a.run_steps(1)
        assert b.step_host(state=True) == a.active_count()
        _same(a, blk, ('after misuse', t))
    a.close()
    b.close()


def test_a_smaller_agent_set_on_the_same_context_and_memory_given_back(S):
    """sca_set_agents with a smaller n: host_state() again, the layout of the new n in the SAME allocation, the loop equal to a fresh context's;
    and 20 contexts that each fetched a block give their memory back."""
    from sca_amd import _lib, scenarios
    big, small = 900, 333
    sol = S.BatchedSolver(max_agents=big, max_obstacles=1)
    sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
    base = None
    for n in (big, small):
        sc = scenarios.random_cube(n, seed=n)
        args = (np.full(n, 0.5), np.ones(n), sc['goal'][:, :3], np.full(n, 3, np.uint8), S.zaxis_flags(sc['start'], sc['goal']),
                scenarios.max_run_dist(sc['start'], sc['goal']))
        sol.set_agents(*args)
        blk = sol.host_state()
        assert blk['pos'].shape == (n, 3) and blk['action'].shape == (n, 7)
        base = base or blk['pos'].ctypes.data
        off = (C.c_int64 * 9)()
        total = C.c_int64(0)
        assert _lib.lib().sca_host_state_layout(n, off, C.byref(total)) == 0
        assert blk['pos'].ctypes.data == base and blk['action'].ctypes.data - base == int(off[8])     # never reallocated, laid out for this n
        fresh = S.BatchedSolver(max_agents=n, max_obstacles=1)
        fresh.set_obstacles(np.zeros((0, 3)), np.zeros(0))
        fresh.set_agents(*args)
        fresh.set_state(sc['start'][:, :3], np.zeros((n, 3), np.float32), sc['start'][:, 3:6], np.zeros(n, np.uint8))
        _write_start(blk, sc, n)
        for t in range(8):
            fresh.run_steps(1, S.NBR_AUTO)
            assert sol.step_host(S.NBR_AUTO, state=(t % 3 == 0)) == fresh.active_count()
            _same(fresh, blk, (n, t))
        fresh.close()
    sol.close()

    hip = C.CDLL('libamdhip64.so.7')                              # by SONAME: the runtime this process already has

    def free_bytes():
        free, total = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value

    n = 100000                                                    # 15 MB of staging per context
    sc = scenarios.random_cube(n, seed=1)
    args = (np.full(n, 0.5), np.ones(n), sc['goal'][:, :3], np.full(n, 3, np.uint8), S.zaxis_flags(sc['start'], sc['goal']),
            scenarios.max_run_dist(sc['start'], sc['goal']))

    def once():
        s = S.BatchedSolver(max_agents=n, max_obstacles=1)
        s.set_obstacles(np.zeros((0, 3)), np.zeros(0))
        s.set_agents(*args)
        blk = s.host_state()
        _write_start(blk, sc, n)
        assert s.step_host(S.NBR_KDTREE, state=True) > 0
        del blk
        s.close()

    for _ in range(2):
        once()
    free0 = free_bytes()
    for _ in range(20):
        once()
    free1 = free_bytes()
    assert free0 - free1 < 64 << 20, (free0, free1)               # 20 leaked staging buffers alone would be 300 MB


def test_on_a_caller_stream_behind_torch_work(S):
    """sca_set_stream: copies, kernels and the synchronisation go to the caller's stream, behind whatever is enqueued there."""
    import torch
    sc, n, policy, tracked, mk = _scene(S, 'sca_circle_tracker')
    a, b = mk(), mk(with_state=False)
    stream = torch.cuda.Stream()
    b.set_stream(stream.cuda_stream)
    blk = b.host_state()
    _write_start(blk, sc, n)
    x = torch.ones(2048, 2048, device='cuda')
    for t in range(10):
        with torch.cuda.stream(stream):
            for _ in range(4):
                x = (x @ x) * (1.0 / 2048.0)                      # a backlog in front of the step
        a.run_steps(1, S.NBR_AUTO)
        assert b.step_host(S.NBR_AUTO, state=(t % 2 == 0)) == a.active_count()
        _same(a, blk, ('stream', t))
    b.use_own_stream()
    for t in range(3):
        a.run_steps(1, S.NBR_AUTO)
        b.step_host(S.NBR_AUTO, state=False)
        _same(a, blk, ('own stream again', t))
    torch.cuda.synchronize()
    assert float(x[0, 0]) == 1.0
    a.close()
    b.close()
