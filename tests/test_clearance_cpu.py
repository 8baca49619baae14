"""Closest approach per agent of a whole context (sca_clearance_enable) without a GPU: the host-compiled descent of sca_clearance.h --
clearance_descend, run lane by lane behind tests/clearance_harness.cpp, the very code k_clearance runs per wavefront -- against the all-pairs
rule of sca_scenes.h (scene_clearance_step) and against the rule restated in Python (tests/clearance_rule.py).  The agent tree is built by
the library's exported host routine (sca_kd_build_host) over the positions a step BEGAN with; the moved positions and the entry flags are
the oracle's.  Every comparison is equality; no expected value comes from the code under test.  Also: the bound on its own, every child
the descent skipped checked by brute force, the stack's overflow bit, every outcome of clearance_check, and the harness as a program of its
own under the sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import clearance_rule as R
import clearance_scenes as CS
import edge_corpus as E
import form_fuzz as F
import harness_util
from golden_util import edge_fixtures

SRC = os.path.join(harness_util.ROOT, 'tests', 'clearance_harness.cpp')
# the arithmetic of sca_core.h as the library builds it (unfused; the restated libm with -mfma); the header's `#pragma unroll` is hipcc's
FLAGS = ['-std=c++17', '-ffp-contract=off', '-mfma', '-fno-builtin-pow', '-Wall', '-Wextra', '-Werror', '-Wno-unknown-pragmas', '-I' + harness_util.CSRC]
KD_STACK = 64                                                      # sca_kernels.hip.h: the depth k_clearance's LDS stack has
STEPS = 6


@pytest.fixture(scope='module')
def H():
    out = os.path.join(harness_util.BUILD, 'libclearance_harness.so')
    deps = [SRC, os.path.join(harness_util.ROOT, 'include', 'sca_hip.h')] + \
        [os.path.join(harness_util.CSRC, f) for f in ('sca_clearance.h', 'sca_scenes.h', 'sca_core.h', 'sca_glibc_math.h', 'sca_glibc_tables.h', 'sca_constants.h')]
    os.makedirs(harness_util.BUILD, exist_ok=True)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(['g++', '-O2', '-fPIC', '-shared'] + FLAGS + ['-o', out, SRC])
    h = C.CDLL(out)
    h.clr_bound.restype = C.c_double
    h.clr_bound.argtypes = [C.c_double, C.c_double]
    h.clr_skips.argtypes = [C.c_double, C.c_double, C.c_double]
    h.clr_box_dist_sq.restype = C.c_double
    h.clr_box_dist_sq.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double]
    h.clr_step.restype = None
    h.clr_step.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4 + [C.c_double, C.c_double, C.c_int, C.c_int] + [C.c_void_p] * 3
    h.clr_all_pairs.restype = None
    h.clr_all_pairs.argtypes = [C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int, C.c_void_p]
    return h


@pytest.fixture(scope='module')
def L():
    from sca_amd import _lib
    return _lib.lib()                                              # (loads without a GPU: sca_kd_build_host is host code)


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def host_tree(L, pts):
    """the library's host build over pts (k, 3): (tree as 10 doubles per node, the permutation)"""
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    k = len(pts)
    perm = np.arange(k, dtype=np.int32)
    tree = np.zeros((max(2 * k - 1, 1), 10))
    assert L.sca_kd_build_host(k, pts.ctypes.data_as(C.POINTER(C.c_double)), perm.ctypes.data_as(C.POINTER(C.c_int32)),
                               tree.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return tree, perm


class Episode:
    """one context's records under the three implementations, step by step"""

    def __init__(self, H, L, scene, per_agent=None, stack_cap=KD_STACK, python_rule=True):
        self.H, self.L, self.s = H, L, scene
        n = scene['n']
        self.radius = np.ascontiguousarray(scene['radius'], np.float64)
        self.opos = np.ascontiguousarray(scene['obs_pos'], np.float64).reshape(-1, 3)
        self.orad = np.ascontiguousarray(scene['obs_radius'], np.float64)
        self.otree, self.operm = host_tree(L, self.opos)
        self.reach = CS.reaches(scene, per_agent)
        self.got, self.pairs, self.rule = R.empty(n), R.empty(n), R.empty(n) if python_rule else None
        self.status = np.zeros(n, np.int32)
        self.stats = np.zeros(5, np.int64)
        self.cap, self.step_no, self.ties = stack_cap, 0, []

    def step(self, old, new, entry_flags):
        """the tree over `old`, the rule over `new`"""
        s, n = self.s, self.s['n']
        self.step_no += 1
        old, new = np.ascontiguousarray(old, np.float64), np.ascontiguousarray(new, np.float64)
        flags = np.ascontiguousarray(entry_flags, np.uint32)
        tree, perm = host_tree(self.L, old)
        self.H.clr_step(n, vp(tree), vp(perm), vp(new), vp(self.radius), vp(flags), s['m'], vp(self.otree), vp(self.operm), vp(self.opos), vp(self.orad),
                        self.reach[0], self.reach[1], self.step_no, self.cap, vp(self.got), vp(self.status), vp(self.stats))
        self.H.clr_all_pairs(n, vp(new), vp(self.radius), vp(flags), s['m'], vp(self.opos), vp(self.orad), self.step_no, vp(self.pairs))
        if self.rule is not None:
            R.step(self.rule, new, self.radius, flags, self.opos, self.orad, self.step_no, self.ties)

    def check(self, what):
        bad = np.flatnonzero(self.got != self.pairs)
        assert bad.size == 0, (what, 'step', self.step_no, 'descent against all pairs', bad[:8].tolist(), self.got[bad[:3]], self.pairs[bad[:3]])
        if self.rule is not None:
            bad = np.flatnonzero(self.got != self.rule)
            assert bad.size == 0, (what, 'step', self.step_no, 'descent against the Python rule', bad[:8].tolist(), self.got[bad[:3]], self.rule[bad[:3]])
        assert not self.status.any(), (what, 'status', np.flatnonzero(self.status)[:8].tolist())
        assert self.stats[1] == 0, (what, 'members of skipped children at or below the value they were skipped against', int(self.stats[1]))


def run_fuzz(H, L, oracle, scene, per_agent=None, steps=STEPS, python_rule=True):
    ep = Episode(H, L, scene, per_agent, python_rule=python_rule)
    run = F.oracle_run(oracle, scene, steps, per_agent=per_agent)
    old = scene['pos']
    for st in run:
        ep.step(old, st['pos'], st['before'])
        ep.check(scene['key'])
        old = st['pos']
    return ep, run


# ---- the tie corpus: F20 ---------------------------------------------------------------------------------------------------------------
TIED_FLOOR = 650                                                    # half of what the family holds (counted by the Python rule alone)


def test_descent_on_the_edge_family_and_its_ties(H, L, oracle):
    """Coincident and touching agents, integer lattices with 6 / 12 / 8 equal distances, separations an ulp either side of the radius sum.
    Every recorded step of every fixture: the tree over the recorded state, the oracle's step as the move.  The rows with more than one
    partner at the winning value are counted with the Python rule alone: measured 1 302 over the family (4 005 updated rows), the floor is
    half of it -- a condition on the corpus, so that the lowest-id rule cannot pass untested."""
    tied = rows = skipped = 0
    for name in edge_fixtures():
        ep = None
        for t in range(E.steps_of(name)):
            scene = E.step_scene(name, t)
            if ep is None:
                ep = Episode(H, L, scene)
            st = E.oracle_step(oracle, scene)
            ep.step(scene['pos'], st['pos'], scene['flags'])
            ep.check((name, t))
        tied += sum(1 for _, ties, _, _ in ep.ties if ties > 1)
        rows += len(ep.ties)
        skipped += int(ep.stats[0])
    print('edge family: rows updated', rows, 'rows with a tie at the winning value', tied, 'children skipped', skipped)
    assert tied >= TIED_FLOOR and rows >= 2 * TIED_FLOOR




# ---- the fuzz scenes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('block', range(4))
def test_descent_on_the_plain_fuzz_scenes(H, L, oracle, block):
    skipped = 0
    for seed in range(10 * block, 10 * block + 10):
        scene = F.random_scene(seed)
        ep, _ = run_fuzz(H, L, oracle, scene, python_rule=scene['n'] <= 400)      # (the Python rule on the scenes it is quick on; all pairs on all)
        skipped += int(ep.stats[0])
    assert skipped > 0                                                          # the bound did prune


@pytest.mark.parametrize('block', range(2))
def test_descent_on_the_per_agent_fuzz_scenes(H, L, oracle, block):
    for seed in list(F.PER_AGENT_SEEDS)[10 * block:10 * block + 10]:
        scene = F.random_scene(seed)
        run_fuzz(H, L, oracle, scene, per_agent=F.per_agent_attributes(seed, scene['n']), python_rule=scene['n'] <= 400)


# ---- the stale tree --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['plain', 'pref', 'max_speed'])
def test_descent_on_a_stale_tree(H, L, oracle, kind):
    """agents closing head-on with gaps of 1 .. 3 steps: the nearest partner after the move is not the nearest in the tree"""
    scene, per_agent = CS.stale_scene(kind)
    ep, run = run_fuzz(H, L, oracle, scene, per_agent=per_agent)
    old, flips, moved = scene['pos'], 0, 0.0
    for st in run:
        flips += int((CS.nearest(old) != CS.nearest(st['pos'])).sum())
        moved = max(moved, float(np.linalg.norm(st['pos'] - old, axis=1).max()))
        old = st['pos']
    assert flips >= 8, flips
    assert 0.9 * scene['pref_speed'].max() * CS.DT <= moved <= CS.max_step(scene, per_agent), (moved, CS.max_step(scene, per_agent))
    if kind != 'plain':
        assert moved > 1.01 * CS.MAX_SPEED * CS.DT                                  # faster than the context's max_speed alone allows for


# ---- sizes and obstacle counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', CS.SIZES)
def test_descent_sizes_and_obstacle_counts(H, L, oracle, n):
    for m in CS.OBSTACLES:
        ep, _ = run_fuzz(H, L, oracle, CS.sized_scene(n, m))
        live = ~np.isin(np.arange(n), np.flatnonzero(CS.sized_scene(n, m)['flags']))
        assert np.isfinite(ep.got['agent_clear'][live]).all() == (n > 1)
        assert np.isfinite(ep.got['obs_clear'][live]).all() == (m > 0)
        if n == 1:
            assert (ep.got['agent_partner'] == -1).all() and not ep.got['agent_step'].any()
        if m == 0:
            assert (ep.got['obs_partner'] == -1).all() and not ep.got['obs_step'].any() and np.isinf(ep.got['obs_clear']).all()


# ---- the bound, the stack ---------------------------------------------------------------------------------------------------------------
def test_the_bound_function(H):
    for dsq, reach in ((0.0, 0.5), (4.0, 0.75), (2.0, 1.2501), (1e12, 3.0)):
        assert H.clr_bound(dsq, reach) == np.sqrt(dsq) - reach
    # skipped only where STRICTLY above the best value; +inf never skips
    assert H.clr_skips(4.0, 0.5, 1.5) == 0 and H.clr_skips(4.0, 0.5, np.nextafter(1.5, 0.0)) == 1 and H.clr_skips(4.0, 0.5, np.nextafter(1.5, 2.0)) == 0
    assert H.clr_skips(1e300, 0.0, np.inf) == 0 and H.clr_skips(0.0, 1.0, -2.0) == 1
    # the box distance in KdWide's layout, both sides, against the six terms written out
    rng = np.random.default_rng(3)
    for _ in range(50):
        lo, hi = np.sort(rng.uniform(-5, 5, (2, 2, 3)), axis=0)                     # [side][axis]
        bx = np.zeros(12)
        for side in range(2):
            for k in range(3):
                bx[(2 * k + 0) * 2 + side], bx[(2 * k + 1) * 2 + side] = lo[side][k], hi[side][k]
        p = rng.uniform(-8, 8, 3)
        for side in range(2):
            want = 0.0
            for k in range(3):
                want = want + max(0.0, lo[side][k] - p[k]) ** 2
                want = want + max(0.0, p[k] - hi[side][k]) ** 2
            assert H.clr_box_dist_sq(vp(bx), side, p[0], p[1], p[2]) == want


def test_the_bound_holds_for_every_box_of_a_tree(H, L, oracle):
    """clearance_bound on its own: for every node of a host-built tree over the old positions and every agent, no member's clearance after
    the move lies below the bound of the node's box (the stale-tree scenes: everybody moves by nearly the largest step)"""
    scene, per_agent = CS.stale_scene('pref')
    run = F.oracle_run(oracle, scene, 1, per_agent=per_agent)
    old, new = scene['pos'], run[0]['pos']
    tree, perm = host_tree(L, old)
    reach = CS.reaches(scene, per_agent)[0]
    checked = 0
    for node in tree:
        members = perm[int(node[0]):int(node[1])]
        for a in range(scene['n']):
            d = np.maximum(0.0, node[4:7] - new[a]) ** 2 + np.maximum(0.0, new[a] - node[7:10]) ** 2
            bound = H.clr_bound(float(d[0] + d[1] + d[2]), reach + float(scene['radius'][a]))
            for b in members:
                if b != a:
                    c = R.l3norm([float(x) for x in new[a]], [float(x) for x in new[b]]) - float(scene['radius'][a] + scene['radius'][b])
                    assert c >= bound, (a, int(b), c, bound)
                    checked += 1
    assert checked > 1000


def test_a_full_stack_sets_the_status_bit(H, L, oracle):
    """never silently: with room for one deferred child a descent that needs more sets ST_KD_STACK on its row; rows without the bit are
    right.  With the kernel's 64 entries no row of the corpus comes near the cap."""
    scene = CS.sized_scene(257, 23)
    run = F.oracle_run(oracle, scene, 1)
    small, full = Episode(H, L, scene, stack_cap=1, python_rule=False), Episode(H, L, scene, python_rule=False)
    small.step(scene['pos'], run[0]['pos'], run[0]['before'])
    full.step(scene['pos'], run[0]['pos'], run[0]['before'])
    full.check('cap 64')
    assert H.clr_stack_bit() == 16 and H.clr_max_leaf() == 10
    over = (small.status & 16) != 0
    assert over.any() and not (small.status & ~16).any()
    assert np.array_equal(small.got[~over], small.pairs[~over])
    assert 1 < full.stats[4] <= 12 < KD_STACK                                       # deferred children at once: far below the cap


def test_far_obstacles_end_at_the_root(H, L):
    """the descent starts from the row's running record: once it is set, an obstacle tree whose two top boxes both lie beyond record + reach is
    left at its root (one node loaded for it per row)"""
    rng = np.random.default_rng(5)
    scene = dict(n=1, m=23, radius=np.array([0.5]), pref_speed=np.array([1.0]), obs_pos=rng.uniform(0, 4, (23, 3)) + [0.0, 0.0, 5.0], obs_radius=np.full(23, 0.5))
    ep = Episode(H, L, scene)
    pos = np.array([[1.0, 1.0, 1.0]])
    ep.step(pos, pos, np.zeros(1))
    first = int(ep.stats[2])
    ep.step(pos + [0.0, 0.0, -2.95], pos + [0.0, 0.0, -3.0], np.zeros(1))          # further away than before by more than the reach
    ep.check('far obstacles')
    assert first > 2 and int(ep.stats[2]) - first == 2                              # the one-leaf agent tree and the obstacle root
    assert ep.got['obs_step'][0] == 1


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
ENABLE, DISABLE, GET, PASS, UPDATE, SET_SHARD, COMM_INIT, PARTITION_INIT, SET_SCENES = range(9)        # ClearanceCall
(OK, NO_AGENTS, NO_STATE, MID_STEP, OFF, RANGE, NO_OUT, BAD_STRUCT, SCENES, SHARD, COMM, PARTITION, GRID_PASS, NO_PASS) = range(14)   # ClearanceFault
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -3, -5                   # include/sca_hip.h
NBR_KDTREE, NBR_GRID, NBR_HOSTBUILD, NBR_AUTO = 0, 1, 2, 3


def test_every_outcome_of_clearance_check(H):
    def check(call, a=0, b=0, have_out=1, struct_bytes=32, **state):
        s = dict(enabled=0, agents=1, state=1, mid_step=0, scenes=0, comm=0, partition=0, n=10, shard_count=10)
        s.update(state)
        st = (C.c_int * 9)(*[s[k] for k in ('enabled', 'agents', 'state', 'mid_step', 'scenes', 'comm', 'partition', 'n', 'shard_count')])
        out = (C.c_int * 2)()
        H.clr_check(call, st, a, b, have_out, struct_bytes, out)
        return out[0], out[1]
    # enable
    assert check(ENABLE) == (OK, 0) and check(ENABLE, enabled=1) == (OK, 0)
    assert check(ENABLE, agents=0, state=0) == (NO_AGENTS, ERR_STATE) and check(ENABLE, state=0) == (NO_STATE, ERR_STATE)
    assert check(ENABLE, mid_step=1) == (MID_STEP, ERR_STATE)
    assert check(ENABLE, scenes=1) == (SCENES, ERR_UNSUPPORTED) and check(ENABLE, comm=1) == (COMM, ERR_UNSUPPORTED)
    assert check(ENABLE, partition=1) == (PARTITION, ERR_UNSUPPORTED) and check(ENABLE, shard_count=9) == (SHARD, ERR_UNSUPPORTED)
    # disable: the state faults only
    assert check(DISABLE, enabled=1) == (OK, 0) and check(DISABLE) == (OK, 0) and check(DISABLE, enabled=1, mid_step=1) == (MID_STEP, ERR_STATE)
    assert check(DISABLE, agents=0) == (NO_AGENTS, ERR_STATE) and check(DISABLE, scenes=1) == (OK, 0)
    # get
    assert check(GET, 0, 10) == (OFF, ERR_STATE)
    assert check(GET, 0, 10, enabled=1) == (OK, 0) and check(GET, 10, 0, enabled=1) == (OK, 0) and check(GET, 3, 7, enabled=1, mid_step=1) == (OK, 0)
    for a, b in ((-1, 1), (0, 11), (10, 1), (11, 0), (0, -1), (5, 2 ** 31 - 1)):
        assert check(GET, a, b, enabled=1) == (RANGE, ERR_ARG), (a, b)
    assert check(GET, 0, 10, have_out=0, enabled=1) == (NO_OUT, ERR_ARG)
    assert check(GET, 0, 10, struct_bytes=24, enabled=1) == (BAD_STRUCT, ERR_ARG) and check(GET, 0, 10, struct_bytes=40, enabled=1) == (BAD_STRUCT, ERR_ARG)
    # while on (and never while off)
    for mode in (NBR_KDTREE, NBR_HOSTBUILD, NBR_AUTO):
        assert check(PASS, mode, enabled=1) == (OK, 0)
    assert check(PASS, NBR_GRID, enabled=1) == (GRID_PASS, ERR_UNSUPPORTED) and check(PASS, NBR_GRID) == (OK, 0)
    assert check(UPDATE, 1, 0, enabled=1) == (OK, 0) and check(UPDATE, 0, 0, enabled=1) == (NO_PASS, ERR_UNSUPPORTED)
    assert check(UPDATE, 1, 1, enabled=1) == (GRID_PASS, ERR_UNSUPPORTED) and check(UPDATE, 0, 0) == (OK, 0) and check(UPDATE, 1, 1) == (OK, 0)
    assert check(SET_SHARD, 9, enabled=1) == (SHARD, ERR_UNSUPPORTED) and check(SET_SHARD, 10, enabled=1) == (OK, 0) and check(SET_SHARD, 9) == (OK, 0)
    assert check(COMM_INIT, enabled=1) == (COMM, ERR_UNSUPPORTED) and check(COMM_INIT) == (OK, 0)
    assert check(PARTITION_INIT, enabled=1) == (PARTITION, ERR_UNSUPPORTED) and check(PARTITION_INIT) == (OK, 0)
    assert check(SET_SCENES, enabled=1) == (SCENES, ERR_UNSUPPORTED) and check(SET_SCENES) == (OK, 0)


def test_the_struct_and_the_symbols(H):
    from sca_amd import _lib
    assert H.clr_struct_bytes() == 32 == _lib.CLEARANCE_DTYPE.itemsize and _lib.CLEARANCE_DTYPE == R.DTYPE
    assert 'sca_clearance_enable' in _lib.SIGNATURES and 'sca_get_clearance' in _lib.SIGNATURES
    assert _lib.lib().sca_version() == 103                          # the feature is detected by the symbol


def test_standalone_under_sanitizers():
    """The descent as a program of its own (its main builds its trees and runs the descent against the all-pairs rule on heap arrays of
    exactly the sizes it may read) under -fsanitize=address,undefined.  Host code only; nothing of it is loaded into python."""
    exe = os.path.join(harness_util.BUILD, 'clearance_harness_san')
    os.makedirs(harness_util.BUILD, exist_ok=True)
    subprocess.check_call(['g++', '-O1', '-g', '-fno-omit-frame-pointer', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan',
                           '-DCLEARANCE_MAIN'] + FLAGS + ['-o', exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'clearance_harness: ok' in r.stdout
