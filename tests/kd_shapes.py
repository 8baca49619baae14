"""Deep and lopsided kd-trees for the kd QUERIES, and a model of the reference's tree and walk that says how many subtrees a walk has waiting.

The query kernels keep the subtrees they still have to visit on fixed stacks: 48 records in the one-wavefront K1 and the kd answer of
SCA_NBR_AUTO (KD_RSTACK), 64 nodes in the packed K1, the grid's obstacle walk, K4's fallback walk and the closest-approach descent
(KD_STACK).  A full stack drops the subtree and sets ST_KD_STACK (16) in the row's status word.  The scenes here are built to stand on
both sides of each limit; the model -- kdTree.py:60-122 (build) and kdTree.py:127-156 (walk) restated in plain Python, sharing no code with
the kernels, sca_kd_build_host or the oracle -- says on which side every served row stands.

k agents on ONE point make a chain k - 9 levels deep (every level peels one member off: leftSize == 0 -> 1), and every level queues the other
child for a walker within neighborDist.  In such a pile all pairs are at equal distance, both children's boxes tie at every level and the
cut at 16 falls inside a run of equal distSq: the list order is the visit order and nothing else.

Scenes are dicts in form_fuzz.random_scene's layout (context_of, oracle_run and compare_with_oracle take them unchanged).  Pile members carry
flag 2 (collided) from the start: they stand in the tree and are served by nobody.  Live agents have policies 1-4 (no fed v_pref).
Shared by tests/test_kd_shapes_cpu.py and tests/test_gpu_kd_shapes.py.  Test infrastructure: the product never imports it."""
import math

import numpy as np

MAX_LEAF = 10                                   # kdTree.py:53
KD_RSTACK, KD_STACK = 48, 64                    # sca_kernels.hip.h
ST_KD_STACK = 16
RANGE_SQ = 100.0                                # neighborDist 10 (agent.py:27), squared (scaPolicy.py:112)
PILE_AT = (3.0, -2.0, 7.0)
LIVE6 = np.array([[6.0, -2.0, 7.0], [3.0, 2.0, 7.0], [3.0, -2.0, 11.5], [-1.0, -2.0, 7.0], [3.0, -7.0, 7.0], [5.0, 0.5, 9.0]])
PILES = (54, 55, 70, 71)
TOUCHES = (74, 75)                              # (K4 walks within about 1.2 m: only the pile's own chain queues, k - 10 subtrees)
OBSTACLE_PILES = (55, 71)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def build(pos, perm=None):
    """kdTree.py:60-122 over positions [n, 3] from the carried permutation (None: the identity): the box of the node's members, the longest
    axis (x only where it is strictly the longest, else y where it is strictly longer than z, else z), the midpoint, the two-pointer
    partition (`< split` stays left, `>= split` goes right), leftSize == 0 -> 1, left = node + 1, right = node + 2 * leftSize.
    Returns (nodes [2n - 1, 10]: begin, end, left, right, min3, max3 -- rows the build never reached stay zero --, the permutation)."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    n = len(pos)
    ids = list(range(n)) if perm is None else [int(a) for a in perm]
    nodes = np.zeros((max(2 * n - 1, 0), 10))
    todo = [(0, n, 0)] if n else []
    while todo:
        begin, end, node = todo.pop()
        p = pos[ids[begin:end]]
        mn, mx = p.min(axis=0), p.max(axis=0)
        nodes[node, 0], nodes[node, 1] = begin, end
        nodes[node, 4:7], nodes[node, 7:10] = mn, mx
        if end - begin <= MAX_LEAF:
            continue
        d = mx - mn
        c = 0 if (d[0] > d[1] and d[0] > d[2]) else (1 if d[1] > d[2] else 2)
        split = 0.5 * (mx[c] + mn[c])
        x = pos[:, c]
        left, right = begin, end
        while left < right:
            while left < right and x[ids[left]] < split:
                left += 1
            while right > left and x[ids[right - 1]] >= split:
                right -= 1
            if left < right:
                ids[left], ids[right - 1] = ids[right - 1], ids[left]
                left += 1
                right -= 1
        if left == begin:
            left += 1
        nodes[node, 2], nodes[node, 3] = node + 1, node + 2 * (left - begin)
        todo.append((begin, left, node + 1))
        todo.append((left, end, node + 2 * (left - begin)))
    return nodes, np.array(ids, np.int32)


def as_lists(nodes):
    """the node table as Python lists (the walk below reads single numbers: lists are several times faster than array rows)"""
    return nodes.tolist()


def _box(nd, p):
    """kdTree.py:132-138, the six terms in the reference's order"""
    t = nd[4] - p[0]
    s = t * t if t > 0.0 else 0.0
    t = p[0] - nd[7]
    s = s + (t * t if t > 0.0 else 0.0)
    t = nd[5] - p[1]
    s = s + (t * t if t > 0.0 else 0.0)
    t = p[1] - nd[8]
    s = s + (t * t if t > 0.0 else 0.0)
    t = nd[6] - p[2]
    s = s + (t * t if t > 0.0 else 0.0)
    t = p[2] - nd[9]
    return s + (t * t if t > 0.0 else 0.0)


def pending(tree, p, range_sq=RANGE_SQ, root=0):
    """The walk of kdTree.py:127-156 from `root` for a walker at p: the nearer child first, a tie goes right, the other child is queued only
    when both are in range.  Returns the largest number of subtrees queued at once.  tree: as_lists(nodes)."""
    if not tree:
        return 0
    px, py, pz = float(p[0]), float(p[1]), float(p[2])
    q = (px, py, pz)
    stack, most, node = [], 0, root
    while True:
        nd = tree[node]
        go = False
        if nd[1] - nd[0] > MAX_LEAF:
            le, ri = int(nd[2]), int(nd[3])
            dl, dr = _box(tree[le], q), _box(tree[ri], q)
            if dl < dr:
                first, second, dfirst, dsecond = le, ri, dl, dr
            else:
                first, second, dfirst, dsecond = ri, le, dr, dl
            if dfirst < range_sq:
                if dsecond < range_sq:
                    stack.append(second)
                    most = max(most, len(stack))
                node, go = first, True
        if not go:
            if not stack:
                return most
            node = stack.pop()


def served_rows(scene, flags=None, vel=None):
    """the rows whose computeNeighbors runs (mampenv.py:35, scaPolicy.py:34, orca3dPolicy.py:51): not finished, and moving unless ORCA"""
    flags = scene['flags'] if flags is None else flags
    vel = scene['vel'] if vel is None else vel
    orca = np.isin(scene['policy'], (3, 4))
    speed = np.sqrt((np.asarray(vel, np.float64) ** 2).sum(axis=1))
    return ((flags & 7) == 0) & (orca | (speed > 1e-5))


_PENDING = {}


def pending_counts(scene, pos=None, perm=None, flags=None, vel=None, tag=0):
    """Per row: (the largest pending count of its walk in the agent tree, the same in the obstacle tree), -1 where the row is not served.
    The state defaults to the scene's own (the identity permutation); `tag` names another state of the scene for the memo (a step)."""
    key = (scene['key'], tag)
    if key in _PENDING:
        return _PENDING[key]
    pos = scene['pos'] if pos is None else pos
    atree = as_lists(build(pos, perm)[0])
    otree = as_lists(build(scene['obs_pos'])[0]) if scene['m'] else []
    out = np.full((scene['n'], 2), -1, np.int64)
    for i in np.flatnonzero(served_rows(scene, flags, vel)):
        out[i, 0] = pending(atree, pos[i])
        out[i, 1] = pending(otree, pos[i])
    _PENDING[key] = out
    return out


def bit_rows(scene, capacity, **state):
    """the served rows whose agent-tree or obstacle-tree walk has more than `capacity` subtrees waiting: the rows that carry ST_KD_STACK"""
    return np.flatnonzero(pending_counts(scene, **state).max(axis=1) > capacity)


def state_before(scene, ref, t):
    """the state step t of form_fuzz.oracle_run's record `ref` started from, as pending_counts' keywords"""
    if t == 0:
        return dict(tag=0)
    r = ref[t - 1]
    return dict(pos=r['pos'], perm=r['perm'], flags=r['flags'], vel=r['vel'], tag=t)


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------
def _scene(key, pos, goal, vel, policy, flags, radius, obs_pos=None, obs_radius=None):
    pos, goal, vel = np.asarray(pos, np.float64), np.asarray(goal, np.float64), np.asarray(vel, np.float64)
    n = len(pos)
    head = np.zeros((n, 3))
    head[:, 0] = np.arctan2(vel[:, 1], vel[:, 0])
    head[:, 1] = np.clip(np.arctan2(vel[:, 2], np.hypot(vel[:, 0], vel[:, 1])), -0.5, 0.5)
    obs_pos = np.zeros((0, 3)) if obs_pos is None else np.asarray(obs_pos, np.float64).reshape(-1, 3)
    obs_radius = np.zeros(0) if obs_radius is None else np.asarray(obs_radius, np.float64)
    policy = np.asarray(policy, np.uint8)
    return dict(n=n, m=len(obs_radius), pos=pos, goal=goal, heading=head, vel=vel.astype(np.float32), radius=np.asarray(radius, np.float64),
                pref_speed=np.ones(n), policy=policy, flags=np.asarray(flags, np.uint8), obs_pos=obs_pos, obs_radius=obs_radius,
                vpref=np.zeros((n, 3)), vmode=np.zeros(n, np.uint8), max_run_dist=3.0 * np.linalg.norm(pos - goal, axis=1) + 1.0, key=key)


def _live6():
    """the six live agents around PILE_AT: 3 .. 5 m from it, flying away from it at 0.5 m/s, policies 1-4"""
    away = LIVE6 - np.array(PILE_AT)
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    goal = LIVE6 + 20.0 * away + np.array([2.0, 3.0, 1.0])
    vel = goal - LIVE6
    vel = 0.5 * vel / np.linalg.norm(vel, axis=1, keepdims=True)
    return LIVE6.copy(), goal, vel, [1, 2, 3, 4, 1, 3]


def _with_pile(pos, goal, vel, policy, radius, k, at=PILE_AT):
    """the agents given and, behind them, k finished ones (flag 2) on the point `at`, at rest, their goal where they are"""
    pile = np.tile(np.asarray(at, np.float64), (k, 1))
    n = len(pos)
    return (np.vstack([pos, pile]), np.vstack([goal, pile]), np.vstack([vel, np.zeros((k, 3))]), list(policy) + [1 + i % 4 for i in range(k)],
            np.concatenate([np.zeros(n, np.uint8), np.full(k, 2, np.uint8)]), np.concatenate([radius, np.full(k, 0.5)]))


def pile(k):
    """the six live agents and a pile of k: the live rows' walks queue about k - 6 subtrees"""
    pos, goal, vel, pol = _live6()
    return _scene(('pile', k), *_with_pile(pos, goal, vel, pol, np.full(6, 0.5), k))


def touch(k):
    """pile(k) and one more live agent 0.9 m from the pile with radius 0.5: it touches the pile (0.9 <= 0.5 + 0.5) and lies inside any
    correct K4 reach.  For K4's fallback walk: the seven live agents are at rest with policies 1 / 2, so the policy pass builds no list for
    them (the bootstrap step, scaPolicy.py:34), their status words are clear behind it and the env update must walk for every one"""
    pos, goal, _, _ = _live6()
    pos = np.vstack([pos, [[3.9, -2.0, 7.0]]])
    goal = np.vstack([goal, [[3.9, 18.0, 8.0]]])
    return _scene(('touch', k), *_with_pile(pos, goal, np.zeros((7, 3)), [1, 2, 1, 2, 1, 2, 1], np.full(7, 0.5), k))


def k4_pending(scene):
    """Per row: the largest pending count of K4's fallback walk in the agent tree (the positions the step began with, within the row's radius
    + the largest radius + two largest steps + 1e-4, the bound sca_hip.hip's collide_reach states: a step is at most 1.01 * the largest of
    the preferred speeds and maxSpeed 1.0, times dt_nominal 0.1); -1 where the row was settled (arrived or collided) before the step.
    Scenes without obstacles."""
    assert scene['m'] == 0
    step = 1.01 * max(float(scene['pref_speed'].max()), 1.0) * 0.1
    reach = float(scene['radius'].max()) + 2.0 * step + 1e-4
    tree = as_lists(build(scene['pos'])[0])
    out = np.full(scene['n'], -1, np.int64)
    for i in np.flatnonzero((scene['flags'] & 3) == 0):
        out[i] = pending(tree, scene['pos'][i], (float(scene['radius'][i]) + reach) ** 2)
    return out


def _crowd(seed, n, side, z0=0.0):
    """n live agents uniform in a box, as form_fuzz.random_scene draws them but for the policies (1-4) and the velocities (none at rest)"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-side, side, (n, 3))
    pos[:, 2] = np.abs(pos[:, 2]) + z0
    return (pos,) + _flights(rng, pos, side)


def _flights(rng, pos, side):
    n = len(pos)
    goal = pos + rng.uniform(-side, side, (n, 3))
    goal[:, 2] = np.abs(goal[:, 2]) + 1.0
    v = rng.normal(0, 1, (n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v *= rng.uniform(0.2, 1.0, (n, 1))
    return goal, v, rng.integers(1, 5, n).tolist()


def pile_in_crowd():
    """300 uniform agents and a finished pile of 52"""
    pos, goal, vel, pol = _crowd(1, 300, 30.0)
    return _scene(('pile_in_crowd',), *_with_pile(pos, goal, vel, pol, np.full(300, 0.5), 52))


def chain_in_crowd():
    """300 uniform agents and 360 finished ones on the progression x = 12 + 16 * 2^(-i / 8): every split peels a few points off"""
    pos, goal, vel, pol = _crowd(2, 300, 30.0)
    k = 360
    q = np.zeros((k, 3))
    q[:, 0] = 12.0 + 2.0 ** (-np.arange(k) / 8.0) * 16.0
    q[:, 1], q[:, 2] = -5.0, 9.0
    return _scene(('chain_in_crowd',), np.vstack([pos, q]), np.vstack([goal, q]), np.vstack([vel, np.zeros((k, 3))]), pol + [1 + i % 4 for i in range(k)],
                  np.concatenate([np.zeros(300, np.uint8), np.full(k, 2, np.uint8)]), np.full(300 + k, 0.5))


def obstacle_pile(k):
    """40 agents -- the six of _live6 and 34 uniform ones -- and k obstacles on the point PILE_AT, with six more around it where the agent
    scenes have their live agents mirrored: the OBSTACLE tree's walk in K1's obstacle phase"""
    pos, goal, vel, pol = _live6()
    cp, cg, cv, cpol = _crowd(5, 34, 30.0)
    far = np.linalg.norm(cp - np.array(PILE_AT), axis=1) > 12.0            # (the uniform ones stay out of the pile's range)
    cp[~far] += np.array([0.0, 40.0, 0.0])
    opos = np.vstack([2.0 * np.array(PILE_AT) - LIVE6, np.tile(np.array(PILE_AT), (k, 1))])
    return _scene(('obstacle_pile', k), np.vstack([pos, cp]), np.vstack([goal, cg]), np.vstack([vel, cv]), pol + cpol, np.zeros(40, np.uint8), np.full(40, 0.5),
                  opos, np.full(6 + k, 0.2))


def _lattice(seed, n, half):
    """n DISTINCT points of the integer lattice [-half, half)^2 x [0, 2 * half): ties on every split plane and at the cut, nobody coincident"""
    rng = np.random.default_rng(seed)
    side = 2 * half
    cells = rng.permutation(side ** 3)[:n]
    pos = np.stack([cells // (side * side) - half, (cells // side) % side - half, cells % side], axis=1).astype(np.float64)
    goal, vel, pol = _flights(rng, pos, float(half))
    return pos, goal, vel, pol


def lattice(n):
    """n agents on distinct integer points, radius 0.3 (a metre apart: nobody touches)"""
    half = 6 if n <= 1000 else 8
    pos, goal, vel, pol = _lattice(3, n, half)
    return _scene(('lattice', n), pos, goal, vel, pol, np.zeros(n, np.uint8), np.full(n, 0.3))


def slab():
    """600 agents in one horizontal plane: a degenerate axis"""
    rng = np.random.default_rng(4)
    pos = np.column_stack([rng.uniform(-30, 30, (600, 2)), np.full(600, 10.0)])
    goal, vel, pol = _flights(rng, pos, 30.0)
    return _scene(('slab',), pos, goal, vel, pol, np.zeros(600, np.uint8), np.full(600, 0.3))


def two_clusters():
    """2 x 300 agents, the clusters 10^6 m apart: the root's box is enormous, its children's are not"""
    rng = np.random.default_rng(6)
    pos = np.vstack([rng.normal(0, 3, (300, 3)), rng.normal(0, 3, (300, 3)) + np.array([1.0e6, 1.0e6, 0.0])])
    pos[:, 2] += 20.0
    goal, vel, pol = _flights(rng, pos, 10.0)
    return _scene(('two_clusters',), pos, goal, vel, pol, np.zeros(600, np.uint8), np.full(600, 0.3))


_SCENES = {}
NAMES = tuple('pile_%d' % k for k in PILES) + ('pile_in_crowd', 'chain_in_crowd') + tuple('obstacle_pile_%d' % k for k in OBSTACLE_PILES) + \
    ('lattice_900', 'slab_600', 'two_clusters', 'lattice_2049') + tuple('touch_%d' % k for k in TOUCHES)
FIXTURES = {'F21_shape_pile%d' % k: 'pile_%d' % k for k in PILES}
FIXTURES['F21_shape_obstacle_pile55'] = 'obstacle_pile_55'
FIXTURE_STEPS = 2


def scene(name):
    """the corpus by name (NAMES); memoised, nobody writes to the arrays"""
    if name not in _SCENES:
        kind, _, arg = name.rpartition('_')
        make = {'pile': pile, 'touch': touch, 'obstacle_pile': obstacle_pile, 'lattice': lattice}
        if kind in make and arg.isdigit():
            _SCENES[name] = make[kind](int(arg))
        else:
            _SCENES[name] = {'pile_in_crowd': pile_in_crowd, 'chain_in_crowd': chain_in_crowd, 'slab_600': slab, 'two_clusters': two_clusters}[name]()
    return _SCENES[name]


def all_pairs_lists(scene, k=16):
    """For every served row: (the ids of ALL agents within neighborDist by the reference's rounded distSq (util.py:100), nearest first,
    whether the k-th and the (k + 1)-th of them tie).  Agents only: a plain numpy search, nothing of the tree.
    What such a search can say about a list: with at most k agents in range the list is exactly these, whatever the order of the visit.
    With more it is NOT the k nearest: agent.py:87-99 drops the farthest entry of a full list for every newcomer in range, nearer or not
    (the `rangeSq = ...` behind it assigns to a local), so the survivors follow the tree's visit order -- all that is left to say without
    the tree is that the list is full and names agents in range."""
    pos = scene['pos']
    out = {}
    for i in np.flatnonzero(served_rows(scene)):
        d = pos - pos[i]
        s = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        s = s + d[:, 2] * d[:, 2]
        s = np.rint(s * 1e5) / 1e5
        s[i] = math.inf
        near = np.flatnonzero(s < RANGE_SQ)
        near = near[np.argsort(s[near], kind='stable')]
        tie = len(near) > k and s[near[k - 1]] == s[near[k]]
        out[int(i)] = (near, bool(tie))
    return out
