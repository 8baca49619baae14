"""The random-scene corpus of the fuzz tests and its oracle runs, shared by tests/test_gpu_parity.py (the default kernel forms),
tests/test_gpu_form_fuzz.py (every other form of sca_forms.h forced at the same small sizes), tests/test_gpu_path_fuzz.py (the same forms with
waypoint lists: random_paths, oracle_run(paths=...)) and tests/test_form_fuzz_cpu.py (what the corpus holds, counted from the oracle and the
rule of tests/path_rule.py alone).  Test infrastructure: it drives the oracle, the product never imports it."""
import collections
import math

import numpy as np

import path_rule as R

K = 16
STATE_KEYS = ('pos', 'vel', 'heading', 'flags', 'total_dist', 'step_num')
BLOCK = 20                                     # seeds per test
PLAIN_SEEDS = range(0, 120)
PER_AGENT_SEEDS = range(1000, 1060)
SWITCH_SIZES = (2047, 2049, 6143, 6145)        # either side of k_solve_fb's and of packed K1's default threshold at 1024 SIMDs

# the form rows: the SCA_* switches of sca_forms.h that force a form at any size (read by sca_create)
ROWS = {
    'packed': {'SCA_K1_PACKED': '1'},
    'split': {'SCA_SOLVE_SPLIT': '1'},                                   # with LP agents in the scene this also routes them to k_lp
    'lp_lane': {'SCA_LP_FORM': 'lane'},
    'fallback_launch': {'SCA_SOLVE_FB_MAX': '0', 'SCA_ACTION_FB_MAX': '0'},
    'solve_fb': {},                                                      # the default of a shard without LP agents: the no_lp variant
    'large_shard': {'SCA_K1_PACKED': '1', 'SCA_SOLVE_SPLIT': '1', 'SCA_SOLVE_FB_MAX': '0', 'SCA_ACTION_FB_MAX': '0'},
    'kd_levels': {'SCA_KD_TOP': '0', 'SCA_KD_WAVE_CAP': '256', 'SCA_KD_TICKET': '1'},
}
PER_AGENT_ROWS = ('packed', 'split', 'lp_lane', 'large_shard')


def random_scene(seed):
    """A random scene for the fuzz test: any agent count, obstacles, mixed policies, agents that are done from the start,
    dense boxes (collisions, > 16 in range), agents on the ground, zero velocities, goals straight above the start."""
    rng = np.random.default_rng(seed)
    n = int(rng.choice([1, 2, 3, 9, 17, 33, 64, 100, 257, 400, 900, 1600]))
    m = int(rng.choice([0, 0, 1, 5, 30]))
    side = float(rng.choice([4.0, 10.0, 30.0, 80.0]))
    pos = rng.uniform(-side, side, (n, 3))
    pos[:, 2] = np.abs(pos[:, 2]) + rng.choice([0.0, 1.0, 20.0])
    goal = rng.uniform(-side, side, (n, 3))
    goal[:, 2] = np.abs(goal[:, 2]) + 1.0
    if rng.random() < 0.3:
        goal[: n // 2, :2] = pos[: n // 2, :2]                             # is_zAxis agents (scaPolicy.py:188-190)
    head = np.zeros((n, 3))
    head[:, 0] = rng.uniform(0, 2 * np.pi, n)
    head[:, 1] = rng.uniform(-0.5, 0.5, n)
    v = rng.normal(0, 1, (n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v *= rng.uniform(0, 1, (n, 1))
    if rng.random() < 0.3:
        v[rng.random(n) < 0.3] = 0.0                                       # bootstrap branch for some
    policy = rng.integers(0, 6, n).astype(np.uint8)
    flags = ((rng.random(n) < 0.1) * rng.choice([1, 2, 4], n)).astype(np.uint8)
    obs_pos = rng.uniform(-side, side, (m, 3))
    obs_pos[:, 2] = np.abs(obs_pos[:, 2])
    vpx = np.trunc(rng.normal(0, 0.6, (n, 3)) * 1e5) / 1e5                 # "tracker output" for SCA / RVO3D+Dubins
    return dict(n=n, m=m, pos=pos, goal=goal, heading=head, vel=v.astype(np.float32), radius=rng.choice([0.3, 0.5, 1.0], n),
                pref_speed=rng.choice([1.0, 1.0, 0.8, 1.5], n), policy=policy, flags=flags, obs_pos=obs_pos,
                obs_radius=rng.choice([0.2, 1.0, 2.0], m), vpref=vpx, vmode=np.isin(policy, (0, 5)).astype(np.uint8),
                max_run_dist=3.0 * np.linalg.norm(pos - goal, axis=1) + 1.0, key=('random', seed))


def per_agent_attributes(seed, n):
    """The solver attributes of the per-agent fuzz for random_scene(seed): (per, params, uniform).  `per`: one draw per agent; every third
    scene is `uniform` -- agent 0's draw for the whole scene, as `params` (sca_params), and no per-agent arrays."""
    rng = np.random.default_rng(77 + seed)
    mhc = rng.choice([0.3, math.pi / 6, math.pi / 4, 1.2, math.pi / 2], n)
    per = dict(neighbor_dist=rng.choice([1.5, 2.5, 4.0, 10.0, 15.0, 30.0], n), max_neighbors=rng.choice([1, 2, 4, 8, 12, 16], n).astype(np.int32),
               time_step=rng.choice([0.05, 0.1, 0.2], n), time_horizon=rng.choice([1.0, 3.0, 10.0, 20.0], n), max_speed=rng.choice([0.7, 1.0, 1.5, 3.0], n),
               max_heading_change=mhc, dt_nominal=rng.choice([0.05, 0.1], n))
    uniform = seed % 3 == 0
    params = {k: (int(v[0]) if k == 'max_neighbors' else float(v[0])) for k, v in per.items()} if uniform else {}
    return per, params, uniform


PATH_SEED = 5000                               # random_paths draws from default_rng(PATH_SEED + seed): the scenes themselves do not change


def random_paths(seed, scene):
    """Waypoint lists (Agent.path) for random_scene(seed) / switch_scene(seed): 0-5 waypoints per agent, each one of five kinds, rounded to 3
    places (p = start, g = goal, u = the unit vector from p to g, r = radius):
        0 near     p + u * U(0, r + 0.8) + N(0, 0.05)    within the radius now or after a few steps
        1 behind   p - u * U(0.5, 5)
        2 ahead    p + (g - p) * U(0.1, 0.9) + N(0, 1)
        3 the goal itself
        4 around the radius' edge   p + N(0, r)
    A list is in list order: get_trajectory pops from its end."""
    rng = np.random.default_rng(PATH_SEED + seed)
    paths = []
    for i in range(scene['n']):
        p, g, r = scene['pos'][i], scene['goal'][i], float(scene['radius'][i])
        d = float(np.linalg.norm(g - p))
        u = (g - p) / d if d > 0 else np.zeros(3)
        lst = []
        for _ in range(int(rng.choice([0, 0, 1, 2, 3, 5]))):
            kind = int(rng.integers(0, 5))
            if kind == 0:
                w = p + u * rng.uniform(0, r + 0.8) + rng.normal(0, 0.05, 3)
            elif kind == 1:
                w = p - u * rng.uniform(0.5, 5)
            elif kind == 2:
                w = p + (g - p) * rng.uniform(0.1, 0.9) + rng.normal(0, 1, 3)
            elif kind == 3:
                w = g
            else:
                w = p + rng.normal(0, r, 3)
            lst.append([float(x) for x in np.round(w, 3)])
        paths.append(lst)
    return paths


def switch_scene(n):
    """A scene of n agents drawn as tests/fuzz_oracle.py draws its scenes, at one setting: 0.05 agents per cubic metre, 40 obstacles, all six
    policies mixed, 5 % of the agents done from the start (seeded by n)."""
    rng = np.random.default_rng(n)
    m = 40
    side = max(2.0, 0.5 * (n / 0.05) ** (1.0 / 3.0))
    pos = rng.uniform(-side, side, (n, 3))
    pos[:, 2] = np.abs(pos[:, 2]) + float(rng.choice([0.0, 1.0, 20.0]))
    goal = rng.uniform(-side, side, (n, 3))
    goal[:, 2] = np.abs(goal[:, 2]) + 1.0
    if rng.random() < 0.3:
        goal[: n // 2, :2] = pos[: n // 2, :2]
    head = np.zeros((n, 3))
    head[:, 0] = rng.uniform(0, 2 * np.pi, n)
    head[:, 1] = rng.uniform(-0.5, 0.5, n)
    v = rng.normal(0, 1, (n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v *= rng.uniform(0, 1, (n, 1))
    if rng.random() < 0.3:
        v[rng.random(n) < 0.3] = 0.0
    policy = rng.integers(0, 6, n).astype(np.uint8)
    flags = ((rng.random(n) < 0.05) * rng.choice([1, 2, 4], n)).astype(np.uint8)
    obs_pos = rng.uniform(-side, side, (m, 3))
    obs_pos[:, 2] = np.abs(obs_pos[:, 2])
    vpx = np.trunc(rng.normal(0, 0.6, (n, 3)) * 1e5) / 1e5
    return dict(n=n, m=m, pos=pos, goal=goal, heading=head, vel=v.astype(np.float32), radius=rng.choice([0.3, 0.5, 1.0], n),
                pref_speed=rng.choice([1.0, 1.0, 0.8, 1.5], n), policy=policy, flags=flags, obs_pos=obs_pos,
                obs_radius=rng.choice([0.2, 1.0, 2.0], m), vpref=vpx, vmode=np.isin(policy, (0, 5)).astype(np.uint8),
                max_run_dist=3.0 * np.linalg.norm(pos - goal, axis=1) + 1.0, key=('switch', n))


CUT_N = (2, 9, 33, 64, 100, 257, 400)
CUT_SEEDS = (0, 1)                             # per (world, axis): 24 plain cut scenes
CUT_WORLDS = (2, 3, 4, 5)
CUT_PER_AGENT = tuple((w, a, 10 + k) for k, (w, a) in enumerate([(2, 0), (3, 1), (4, 2), (5, 0), (2, 1), (3, 2), (4, 0), (5, 1)]))
CUT_TRACKED = ((2, 0, 22), (2, 2, 20), (4, 1, 21), (4, 0, 24))               # (d): policy 0 agents under the device tracker; 100, 257, 64, 257 agents
# the cuts in cells per world (two variants by seed): every interior slab of worlds 3 and 4 is two cells wide, the least sca_partition_init
# accepts, and from world 4 on two such slabs are adjacent; cells below and above zero either way
_CUT_CELLS = {2: ([-1], [1]), 3: ([-1, 1], [-2, 0]), 4: ([-2, 0, 2], [-3, -1, 1]), 5: ([-3, -1, 1, 3], [-4, -1, 1, 3])}


def cut_attributes(seed, n):
    """per-agent solver attributes for cut_scene(seed, ..., nd=4.0), as per_agent_attributes returns them: neighbor_dist 1.5 / 2.5 / 4.0 with
    4.0 present (the cell is then about 4 m), time_step up to 0.2, max_speed up to 3.0"""
    rng = np.random.default_rng(177 + seed)
    per = dict(neighbor_dist=rng.choice([1.5, 2.5, 4.0], n), max_neighbors=rng.choice([1, 2, 4, 8, 12, 16], n).astype(np.int32),
               time_step=rng.choice([0.05, 0.1, 0.2], n), time_horizon=rng.choice([1.0, 3.0, 10.0, 20.0], n), max_speed=rng.choice([0.7, 1.0, 1.5, 3.0], n),
               max_heading_change=rng.choice([0.3, math.pi / 6, math.pi / 4, 1.2, math.pi / 2], n), dt_nominal=rng.choice([0.05, 0.1], n))
    per['neighbor_dist'][0] = 4.0
    return per, {}, False


def cut_scene(seed, world, axis, nd=10.0, policies=None):
    """A scene made for the cell-owner partition's cuts, with random_scene's keys: (scene, cuts).  `world` slabs along `axis`, the cuts given
    in metres somewhere inside the cell they are moved to the boundary of (_CUT_CELLS; the cell is the grid's for the largest neighbor_dist
    `nd`).  About a third of the agents are uniform in the box; the others are placed, in this order until two thirds of n are used:
        the empty-rank agents (seed-dependent: an end rank owns nothing and gains its first agents, or holds only agents that leave)
        head-on pairs straddling a cut, r_a + r_b + 0.1 .. 0.4 apart, one of them about to cross; the same against an obstacle on the cut
        crossers within 0.4 m of a cut with velocity, heading, fed v_pref and goal across it (the goal far away or 0.2 .. 0.5 m beyond)
        boundary agents: the first double of cell k and the last one of cell k - 1, for a positive and a negative k
        returners (goal on the near side, velocity across), finished agents inside the edge layers
        a clump of 18 .. 24 agents within neighbor_dist of each other, centred on a cut
    and then more crossers, pairs and returners over all cuts.  policies: the policy values to draw from (None: 0 .. 5)."""
    import partition_ranks as PR
    rng = np.random.default_rng([seed, world, axis, 4242])
    n = int(rng.choice(CUT_N))
    inv = PR.inv_cell_of(nd)
    cell = 1.0 / inv
    ks = _CUT_CELLS[world][seed % 2]
    cuts = [float((k + rng.uniform(0.05, 0.95)) * cell) for k in ks]
    bound = [PR.first_double_of_cell(k, inv) for k in ks]                     # where the cuts really are
    side = float(rng.choice([3.0, 6.0])) * max(1.0, math.sqrt(n / 64.0))          # (the placed agents sit near the cuts: room across)
    lo, hi = bound[0] - 1.2 * cell, bound[-1] + 1.2 * cell
    empty = (None, 'gains', 'loses')[(seed + axis) % 3]                       # per world every mode comes with two of the six scenes
    # (an end rank: the last one for `gains`, the first for `loses`; with two ranks the one whose cells lie further from zero)
    top = (ks[0] > 0) if world == 2 else empty == 'gains'
    if empty is not None and top:
        hi = bound[-1] - 0.5                                                  # that rank owns nothing, or only what is placed there below
    if empty is not None and not top:
        lo = bound[0] + 0.5
    zoff = float(rng.choice([0.0, 1.0, 20.0]))
    pol_set = np.arange(6) if policies is None else np.asarray(policies)

    def point(x):
        p = rng.uniform(-side, side, 3)
        if axis != 2:
            p[2] = abs(p[2]) + zoff
        p[axis] = x
        return p

    pos = np.array([point(rng.uniform(lo, hi)) for _ in range(n)])
    goal = np.array([point(rng.uniform(lo, hi)) for _ in range(n)])
    if axis != 2:
        goal[:, 2] += 1.0
    v = rng.normal(0, 1, (n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v *= rng.uniform(0, 1, (n, 1))
    if rng.random() < 0.3:
        v[rng.random(n) < 0.3] = 0.0
    head = np.zeros((n, 3))
    head[:, 0] = rng.uniform(0, 2 * np.pi, n)
    head[:, 1] = rng.uniform(-0.5, 0.5, n)
    policy = rng.choice(pol_set, n).astype(np.uint8)
    flags = ((rng.random(n) < 0.1) * rng.choice([1, 2, 4], n)).astype(np.uint8)
    radius = rng.choice([0.3, 0.5, 1.0], n)
    vpx = np.trunc(rng.normal(0, 0.6, (n, 3)) * 1e5) / 1e5
    obs = [(point(rng.uniform(lo, hi)), float(rng.choice([0.2, 1.0, 2.0]))) for _ in range(int(rng.choice([0, 1, 5])))]
    e = np.zeros(3)
    e[axis] = 1.0
    used = [0]
    quota = n - n // 3

    def put(x, d, far=True, speed=None, p=None, returner=False):
        """the next agent at coordinate x along the axis (p: its other coordinates), moving in direction d = +-1 along the axis, its goal
        on the other side of x + d * (its distance) -- or behind it (returner); False when the quota is used up"""
        if used[0] >= quota:
            return -1
        i = used[0]
        used[0] += 1
        pos[i] = point(x) if p is None else p
        pos[i, axis] = x
        flags[i] = 0
        sp = rng.uniform(0.6, 1.0) if speed is None else speed
        v[i] = d * e * sp
        head[i] = 0.0
        if axis == 0:
            head[i, 0] = 0.0 if d > 0 else np.pi
        elif axis == 1:
            head[i, 0] = d * np.pi / 2
        else:
            head[i, 1] = d * 0.7                                              # (inside the pitch limits)
        g = pos[i] + d * e * (rng.uniform(15.0, 40.0) if far else rng.uniform(0.2, 0.5))
        if returner:
            g = pos[i] - d * e * rng.uniform(2.0, 20.0)
        goal[i] = g + (0.0 if not far or returner else 1.0) * rng.normal(0, 0.3, 3) * (1.0 - e)
        vpx[i] = np.trunc(d * e * rng.uniform(0.7, 1.0) * 1e5) / 1e5
        return i

    def crosser(b, d, far):
        """within 0.4 m of boundary b on the side it leaves (d = +1: below it); a near goal lies 0.2 .. 0.5 m beyond the cut"""
        gap = rng.uniform(0.01, 0.4 if far else 0.15)
        i = put(b - d * gap, d, far=True)
        if i >= 0 and not far:
            goal[i] = pos[i]
            goal[i, axis] = b + d * rng.uniform(0.2, 0.5)
        return i

    def pair(b, d):
        """head on across boundary b: a moves in direction d and is about to cross, c comes the other way on the far side"""
        ga = rng.uniform(0.01, 0.06)
        a = put(b - d * ga, d)
        if a < 0 or used[0] >= quota:
            return
        sep = radius[a] + radius[used[0]] + rng.uniform(0.1, 0.4)
        put(pos[a, axis] + d * sep, -d, p=pos[a].copy())

    def against_obstacle(b, d):
        r_o = float(rng.choice([0.2, 1.0]))
        a = put(b - d * rng.uniform(0.01, 0.06), d)
        if a >= 0:
            c = pos[a].copy()
            c[axis] = pos[a, axis] + d * (radius[a] + r_o + rng.uniform(0.1, 0.3))
            obs.append((c, r_o))

    # ---- the empty rank
    leavers = []
    if empty == 'gains':
        for _ in range(2):
            crosser(bound[-1] if top else bound[0], +1 if top else -1, True)
    elif empty == 'loses':
        for _ in range(2):
            i = put(bound[-1] + rng.uniform(0.01, 0.05), -1, speed=1.0) if top else put(bound[0] - rng.uniform(0.01, 0.05), +1, speed=1.0)
            if i >= 0:
                leavers.append(i)
                policy[i] = 3 if policies is None else policy[i]             # (ORCA3D, straight-line v_pref at pref_speed: it leaves for certain)
    order = list(range(len(bound)))
    for c in order:                                                           # one pair per cut first: the smallest scenes get them
        pair(bound[c], +1 if (c + seed) % 2 == 0 else -1)
    for c in order:
        crosser(bound[c], -1 if (c + seed) % 2 == 0 else +1, far=bool((c + seed) % 2))
    # ---- boundary agents: the first double of a cell and the last one of the cell below, a positive and a negative k (the cuts when they fit)
    for k in ([k for k in ks if k > 0][:1] or [1]) + ([k for k in ks if k < 0][:1] or [-1]):
        b = PR.first_double_of_cell(k, inv)
        if lo < b < hi:
            put(b, +1 if rng.random() < 0.5 else -1)
            put(float(np.nextafter(b, -np.inf)), +1 if rng.random() < 0.5 else -1)
    for c in order:
        against_obstacle(bound[c], +1 if (c + seed) % 2 else -1)
        d = +1 if rng.random() < 0.5 else -1
        put(bound[c] - d * rng.uniform(0.01, 0.1), d, returner=True)
        for d in (+1, -1):                                                    # finished from the start inside the edge layers of both sides
            i = put(bound[c] - d * rng.uniform(0.0, 0.9) * cell, d)
            if i >= 0 and lo < pos[i, axis] < hi:
                flags[i] = rng.choice([1, 2, 4])
    # ---- a clump on a cut: more than 16 within neighbor_dist of one another, members on both sides
    if quota - used[0] >= 24:
        b = bound[int(rng.integers(0, len(bound)))]
        centre = point(b)
        for _ in range(int(rng.integers(18, 25))):
            i = put(b, +1)
            off = rng.normal(0, 1, 3)
            off *= rng.uniform(0.2, 0.45) * min(nd, 10.0) / np.linalg.norm(off)
            pos[i] = centre + off
            d = +1 if pos[i, axis] < b else -1
            v[i] = d * e * rng.uniform(0.2, 1.0)
            vpx[i] = np.trunc(v[i] * 1e5) / 1e5
            goal[i] = centre + d * e * rng.uniform(3.0, 20.0)
    while used[0] < quota:
        c = int(rng.integers(0, len(bound)))
        d = +1 if rng.random() < 0.5 else -1
        what = rng.integers(0, 4)
        if what == 0:
            pair(bound[c], d)
        elif what == 1:
            put(bound[c] - d * rng.uniform(0.01, 0.2), d, returner=True)
        else:
            crosser(bound[c], d, far=bool(what == 2))
    # ---- the empty rank stays what it was made: whoever else was placed into it is mirrored at its cut, with what it aims at
    if empty is not None:
        b = bound[-1] if top else bound[0]
        inside = pos[:, axis] >= b if top else pos[:, axis] < b
        inside[leavers] = False
        for i in np.flatnonzero(inside):
            pos[i, axis] = (float(np.nextafter(b, -np.inf)) - (pos[i, axis] - b)) if top else b + (b - pos[i, axis])
            goal[i, axis] = 2 * b - goal[i, axis]
            v[i, axis], vpx[i, axis] = -v[i, axis], -vpx[i, axis]
            if axis == 0:
                head[i, 0] = np.pi - head[i, 0]
            else:
                head[i, int(axis == 2)] = -head[i, int(axis == 2)]
    if empty == 'loses':                                                      # ... and who comes toward it arrives after its last agent has left
        late = (np.abs(pos[:, axis] - b) < 0.4) & (v[:, axis] * (1 if top else -1) > 0)
        late[leavers] = False
        pos[late, axis] += -0.4 if top else 0.4
    m = len(obs)
    obs_pos = np.array([o[0] for o in obs]).reshape(m, 3)
    obs_radius = np.array([o[1] for o in obs]).reshape(m)
    return dict(n=n, m=m, pos=pos, goal=goal, heading=head, vel=v.astype(np.float32), radius=radius,
                pref_speed=rng.choice([1.0, 1.0, 0.8, 1.5], n), policy=policy, flags=flags, obs_pos=obs_pos, obs_radius=obs_radius,
                vpref=vpx, vmode=np.isin(policy, (0, 5)).astype(np.uint8), max_run_dist=3.0 * np.linalg.norm(pos - goal, axis=1) + 1.0,
                key=('cut', seed, world, axis, nd, None if policies is None else tuple(policies))), cuts


def no_lp(scene):
    """the same scene with the ORCA3D-LP agents (policy 4) as ORCA3D agents (3): a shard without LP agents, which k_solve_fb may take"""
    s = dict(scene)
    s['policy'] = np.where(scene['policy'] == 4, 3, scene['policy']).astype(np.uint8)
    s['key'] = scene['key'] + ('no_lp',)
    return s


def zaxis_of(scene):
    """is_zAxis of scaPolicy.py:188-189 (sca_amd.solver.zaxis_flags, restated: this module runs without the product)"""
    d = scene['goal'] - scene['pos']
    return ((np.abs(d[:, 0]) <= 1e-5) & (np.abs(d[:, 1]) <= 1e-5)).astype(np.uint8)


_RUNS = collections.OrderedDict()
_RUNS_MAX = 3 * BLOCK                          # the rows of one block run one after the other: a block or two stay, the rest goes


def oracle_run(oracle, scene, steps, per_agent=None, list_rule=0, paths=None):
    """The free-running oracle trajectory of a scene: policy_step then env_update per step, from the scene's own state.  One dict per step:
    action, nbr_valid, nbr_n, nbr_id, nbr_kind, nbr_dsq, diag, perm, vpref (the v_pref the pass used), `before` (the flags the step started from), `flags_policy` (the flags after
    the policy pass) and the state after the step (STATE_KEYS).  per_agent: what per_agent_attributes returned.  list_rule: 0 the reference's lists
    (what SCA_NBR_KDTREE and SCA_NBR_AUTO return), 1 the lists SCA_NBR_GRID documents (oracle.set_list_rule); `status` then carries bit 32 on the
    rows that overflowed.  paths: what random_paths returned -- before each policy_step the rule (path_rule.pass_rule_csr) advances the lists; its
    v_pref goes in on the rows it aims at a waypoint (mode 1), the scene's fed vpref / vmode stay on the tracked rows (their lists advance, their
    v_pref stays fed, as in k_waypoint) and every other row gets mode 0; each step then also records path_left, now_goal, vpref_rule and path_mode
    (after the rule), path_left_before, now_goal_before, pos_before (what the rule started from) and the lists' CSR form (path_off, path_pts).  Memoised per scene and variant: every form
    row of a block compares against one run.  The arrays are shared: nobody writes to them."""
    key = scene['key'] + (per_agent is not None,) + (('rule', list_rule) if list_rule else ()) + (('paths',) if paths is not None else ())
    have = _RUNS.get(key)
    if have is not None and len(have) >= steps:
        _RUNS.move_to_end(key)
        return have[:steps]
    s, n = scene, scene['n']
    zaxis = zaxis_of(s)
    p, ve, he, fl = s['pos'].copy(), s['vel'].copy(), s['heading'].copy(), s['flags'].copy()
    td, sn, perm = np.zeros(n), np.zeros(n, np.int32), np.arange(n, dtype=np.int32)
    out = []
    if paths is not None:
        off, pts = R.csr(paths)
        rem, ng = np.diff(off).astype(np.int32), np.full((n, 3), np.nan)
    try:
        oracle.set_list_rule(list_rule)
        if per_agent is not None:
            per, params, uniform = per_agent
            oracle.set_params(**params)
            if uniform:
                oracle.set_agent_params()
            else:
                oracle.set_agent_params(n, **per)
        for _ in range(steps):
            vpref, vmode, path = s['vpref'], s['vmode'], {}
            if paths is not None:
                path = dict(path_left_before=rem, now_goal_before=ng, pos_before=p, path_off=off, path_pts=pts)
                rem, ng, vp, mode = R.pass_rule_csr(off, pts, rem, ng, p, s['goal'], s['radius'], s['pref_speed'], s['policy'], fl)
                aimed = mode.astype(bool)
                vpref, vmode = np.where(aimed[:, None], vp, s['vpref']), np.where(aimed, 1, s['vmode']).astype(np.uint8)
                path.update(path_left=rem, now_goal=ng, vpref_rule=vp, path_mode=mode)
            r = oracle.policy_step(p, ve, he, s['radius'], s['pref_speed'], fl, s['goal'], s['policy'], zaxis, vpref, vmode,
                                   perm, s['obs_pos'], s['obs_radius'], nthreads=8)
            perm = r['perm']
            u = oracle.env_update(p, ve, he, s['radius'], r['flags'], s['goal'], r['action'], td, s['max_run_dist'], sn,
                                  s['obs_pos'], s['obs_radius'])
            step = {k: r[k] for k in ('action', 'nbr_valid', 'nbr_n', 'nbr_id', 'nbr_kind', 'nbr_dsq', 'diag', 'perm', 'status', 'vpref')}
            step['before'], step['flags_policy'] = fl, r['flags']
            step.update(path)
            p, ve, he, fl, td, sn = u['pos'], u['vel'], u['heading'], u['flags'], u['total_dist'], u['step_num']
            step.update(pos=p, vel=ve, heading=he, flags=fl, total_dist=td, step_num=sn)
            out.append(step)
    finally:
        oracle.set_params()
        oracle.set_agent_params()
        oracle.set_list_rule(0)
    _RUNS[key] = out
    while len(_RUNS) > _RUNS_MAX:
        _RUNS.popitem(last=False)
    return out


QUANTITIES = ('lp_active', 'lp4', 'lp_obstacle', 'fallback', 'full_lists', 'new_collisions', 'done_at_start')
# ... and of a run with lists: what the rule did, counted from the rule's own inputs and outputs
PATH_QUANTITIES = ('served', 'first_takes', 'double_pops', 'later_pops_reached', 'later_pops_behind', 'steps_with_later_pop', 'exhausted',
                   'orca_pops', 'tracked_with_list', 'aimed', 'aimed_zeroed_at_goal', 'at_waypoint', 'non_finite')
# the branches of get_trajectory, per distance measure (l3norm / distance) and per pass (`first`: now_goal was None, `later`): the waypoint is
# within the radius, it is not but lies behind, neither (kept); within or behind with nothing left to pop (a first pass only: a later pass
# with an empty list takes the next branch); the list is empty and now_goal the goal (`first`: it was never given one, `later`: it ran out)
BRANCHES = tuple((m, w, b) for m in ('l3norm', 'distance') for w in ('first', 'later') for b in ('empty', 'near', 'behind', 'keep')) + \
    (('l3norm', 'first', 'nothing_left'), ('distance', 'first', 'nothing_left'))


def path_counts(scene, run):
    """PATH_QUANTITIES and BRANCHES of a run with lists (oracle_run(paths=...)), summed over its steps: rows, but steps_with_later_pop
    (steps of the scene).  orca_pops: passes in which an ORCA3D / ORCA3D-LP agent popped; tracked_with_list: served SCA / RVO3D+Dubins
    rows whose list is not empty when the pass begins."""
    s = scene
    c = dict.fromkeys(PATH_QUANTITIES + BRANCHES, 0)
    orca, tracked = np.isin(s['policy'], R.ORCA), np.isin(s['policy'], R.TRACKED)
    for st in run:
        served = (st['before'] & 7) == 0
        given = np.diff(st['path_off']) > 0
        rem0, rem1, ng0, ng1, pos = st['path_left_before'], st['path_left'], st['now_goal_before'], st['now_goal'], st['pos_before']
        first = served & (rem0 > 0) & np.isnan(ng0[:, 0])
        later = served & (rem0 > 0) & ~np.isnan(ng0[:, 0])
        popped = rem0 - rem1
        # the waypoint the pass tested: the one it took (first pass) or the one it had
        took = np.where(first[:, None], _last(st, rem0), ng0)
        with np.errstate(invalid='ignore'):
            near = R._dist(pos, took, orca) <= s['radius']
            behind = R._dist(took, s['goal'], orca) >= R._dist(pos, s['goal'], orca)
        left = rem0 - first                                                       # what the list held when the test was made
        c['served'] += int(served.sum())
        c['first_takes'] += int(first.sum())
        c['double_pops'] += int((popped == 2).sum())
        c['later_pops_reached'] += int((later & (popped == 1) & near).sum())
        c['later_pops_behind'] += int((later & (popped == 1) & ~near).sum())
        c['steps_with_later_pop'] += int((later & (popped == 1)).any())
        c['exhausted'] += int(((rem0 > 0) & (rem1 == 0)).sum())
        c['orca_pops'] += int((orca & (popped > 0)).sum())
        c['tracked_with_list'] += int((served & tracked & (rem0 > 0)).sum())
        aimed = st['path_mode'].astype(bool)
        c['aimed'] += int(aimed.sum())
        c['aimed_zeroed_at_goal'] += int((aimed & (R._dist(s['goal'], pos, np.zeros(s['n'], bool)) < 0.2)).sum())
        c['at_waypoint'] += int((aimed & (np.linalg.norm(np.nan_to_num(ng1) - pos, axis=1) < 1e-4)).sum())
        c['non_finite'] += int((~np.isfinite(st['vpref_rule'])).any(axis=1).sum())
        for m, sel in (('l3norm', ~orca), ('distance', orca)):
            c[(m, 'first', 'empty')] += int((served & (rem0 == 0) & sel & ~given).sum())
            c[(m, 'later', 'empty')] += int((served & (rem0 == 0) & sel & given).sum())
            for w, rows in (('first', first & sel), ('later', later & sel)):
                c[(m, w, 'near')] += int((rows & near & (left > 0)).sum())
                c[(m, w, 'behind')] += int((rows & ~near & behind & (left > 0)).sum())
                c[(m, w, 'keep')] += int((rows & ~near & ~behind).sum())
            c[(m, 'first', 'nothing_left')] += int((first & sel & (near | behind) & (left == 0)).sum())
    return c


def _last(st, rem0):
    """the last element of every list as the pass found it (NaN where the list was empty)"""
    off, pts = st['path_off'].astype(np.int64), st['path_pts']
    out = np.full((len(rem0), 3), np.nan)
    have = rem0 > 0
    out[have] = pts[off[:-1][have] + rem0[have] - 1]
    return out


def corpus_counts(scene, run):
    """what a scene's oracle run feeds the forms with, summed over the steps of `run` (QUANTITIES; of a run with lists also PATH_QUANTITIES
    and BRANCHES)"""
    c = dict.fromkeys(QUANTITIES, 0)
    if run and 'path_left' in run[0]:
        c.update(path_counts(scene, run))
    c['done_at_start'] = int(((scene['flags'] & 7) != 0).sum())
    for st in run:
        active = (st['before'] & 7) == 0
        lp = active & (scene['policy'] == 4)
        lp4 = lp & (st['diag'][:, 4] == 1)                                      # planeFail < K: linearProgram4
        in_list = np.arange(K)[None, :] < st['nbr_n'][:, None]
        c['lp_active'] += int(lp.sum())
        c['lp4'] += int(lp4.sum())
        c['lp_obstacle'] += int((lp & ((st['nbr_kind'] == 1) & in_list).any(axis=1)).sum())     # isob planes among the LP's
        c['fallback'] += int((st['diag'][:, 1] == 1).sum())
        c['full_lists'] += int(((st['nbr_valid'] != 0) & (st['nbr_n'] == K)).sum())
        c['new_collisions'] += int((((st['flags_policy'] & 2) != 0) & ((st['before'] & 2) == 0)).sum())      # set by the policy pass (agent.py:83-85)
    return c
