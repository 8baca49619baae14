"""Scenes and small helpers shared by tests/test_clearance_cpu.py and tests/test_gpu_clearance.py (the closest approach per agent of a whole
context, sca_clearance_enable).  A scene has form_fuzz.random_scene's keys.  Nothing here calls the library."""
import numpy as np

SIZES = (1, 2, 10, 11, 63, 64, 65, 257)
OBSTACLES = (0, 1, 11, 23)
MAX_SPEED, DT = 1.0, 0.1                        # the context's defaults (agent.py:27-41)


def max_step(scene, per_agent=None):
    """collide_reach's max_step: 1.01 x the largest of pref_speed and max_speed x dt_nominal; with per-agent attributes the context's values
    are their envelope (sca_set_agent_params), with uniform ones the scene's params"""
    ms, dt = MAX_SPEED, DT
    if per_agent is not None:
        per, params, uniform = per_agent
        ms = float(params['max_speed']) if uniform else float(np.max(per['max_speed']))
        dt = float(params['dt_nominal']) if uniform else float(np.max(per['dt_nominal']))
    return 1.01 * max(float(np.max(scene['pref_speed'])), ms) * dt


def reaches(scene, per_agent=None):
    """(agent_reach, obs_reach) as k_clearance takes them: the kernel adds the agent's own radius"""
    return (max_step(scene, per_agent) + float(np.max(scene['radius'])) + 1e-4,
            (float(np.max(scene['obs_radius'])) if scene['m'] else 0.0) + 1e-4)


def sized_scene(n, m, seed=0):
    """n agents and m obstacles in a box dense enough that several lie within a few radii: mixed policies, a few done from the start"""
    rng = np.random.default_rng(9000 + 131 * n + 7 * m + seed)
    side = max(2.0, 1.2 * n ** (1.0 / 3.0))
    pos = rng.uniform(-side, side, (n, 3))
    pos[:, 2] = np.abs(pos[:, 2]) + 1.0
    goal = -pos.copy()
    goal[:, 2] = np.abs(goal[:, 2]) + 1.0
    head = np.zeros((n, 3))
    head[:, 0] = rng.uniform(0, 2 * np.pi, n)
    v = goal - pos
    v /= np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-9)
    v *= rng.uniform(0.2, 1.0, (n, 1))
    policy = rng.integers(0, 6, n).astype(np.uint8)
    flags = ((rng.random(n) < 0.08) * rng.choice([1, 2, 4], n)).astype(np.uint8)
    flags[0] = 0
    obs_pos = rng.uniform(-side, side, (m, 3))
    obs_pos[:, 2] = np.abs(obs_pos[:, 2])
    return dict(n=n, m=m, pos=pos, goal=goal, heading=head, vel=v.astype(np.float32), radius=rng.choice([0.3, 0.5, 1.0], n),
                pref_speed=rng.choice([1.0, 0.8, 1.5], n), policy=policy, flags=flags, obs_pos=obs_pos, obs_radius=rng.choice([0.2, 1.0, 2.0], m),
                vpref=np.trunc(rng.normal(0, 0.6, (n, 3)) * 1e5) / 1e5, vmode=np.isin(policy, (0, 5)).astype(np.uint8),
                max_run_dist=3.0 * np.linalg.norm(pos - goal, axis=1) + 1.0, key=('clearance_sized', n, m, seed))


def stale_scene(kind):
    """The "stale tree" family, placed by hand: triples on a line, 40 m apart from each other.  In a triple the middle agent flies +x
    towards the right one, which flies -x towards it, while the left one flies away to -x; the left gap is the smaller one before the move
    and the larger one after it, so the middle agent's nearest partner after the move is not its nearest in the tree, which holds the
    positions the step began with.  Gaps between 1x and 3x the largest step.  ORCA3D agents (policy 3) with a velocity already: no
    bootstrap step.  kind: 'plain' (pref_speed 1.0), 'pref' (pref_speed 1.5, above the context's max_speed 1.0), 'max_speed' (a per-agent
    max_speed of 3.0 on every second triple, above the context's 1.0; pref_speed 2.5 there).  Returns (scene, per_agent or None)."""
    triples = 8
    n = 3 * triples
    speed = np.full(n, {'plain': 1.0, 'pref': 1.5, 'max_speed': 1.0}[kind])
    per_agent = None
    if kind == 'max_speed':
        fast = (np.arange(n) // 3) % 2 == 1
        speed[fast] = 2.5
        per = dict(neighbor_dist=np.full(n, 10.0), max_neighbors=np.full(n, 16, np.int32), time_step=np.full(n, 0.1), time_horizon=np.full(n, 10.0),
                   max_speed=np.where(fast, 3.0, 1.0), max_heading_change=np.full(n, np.pi / 4), dt_nominal=np.full(n, 0.1))
        per_agent = (per, {}, False)
    step = 1.01 * max(float(speed.max()), 3.0 if kind == 'max_speed' else MAX_SPEED) * DT
    pos, goal, vel = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3), np.float32)
    for t in range(triples):
        left_gap, right_gap = (1.0 + 0.2 * t) * step, (1.3 + 0.2 * t) * step            # 1.0 .. 2.4 and 1.3 .. 2.7 steps
        y = 40.0 * t
        xs = (-left_gap, 0.0, right_gap)
        dirs = (-1.0, 1.0, -1.0)
        for k in range(3):
            i = 3 * t + k
            pos[i] = (xs[k], y, 10.0)
            goal[i] = (xs[k] + 30.0 * dirs[k], y, 10.0)
            vel[i] = (dirs[k] * speed[i], 0.0, 0.0)
    head = np.zeros((n, 3))
    head[:, 0] = np.where(vel[:, 0] > 0, 0.0, np.pi)
    policy = np.full(n, 3, np.uint8)
    return dict(n=n, m=0, pos=pos, goal=goal, heading=head, vel=vel, radius=np.full(n, 0.02), pref_speed=speed, policy=policy,
                flags=np.zeros(n, np.uint8), obs_pos=np.zeros((0, 3)), obs_radius=np.zeros(0), vpref=np.zeros((n, 3)), vmode=np.zeros(n, np.uint8),
                max_run_dist=np.full(n, 200.0), key=('clearance_stale', kind)), per_agent


def nearest(pos):
    """the index of every agent's nearest other agent (unrounded distances; -1 for a single agent)"""
    n = len(pos)
    if n < 2:
        return np.full(n, -1)
    d = np.linalg.norm(pos[:, None, :] - pos[None, :, :], axis=2)
    d[np.arange(n), np.arange(n)] = np.inf
    return d.argmin(axis=1)


def all_pairs_chunked(rec, pos, radius, entry_flags, obs_pos, obs_radius, step_no, rule, chunk=512):
    """clearance_rule.step for a large swarm: numpy finds, per chunk of rows and from the unrounded distances, the partners within 2e-5 of the
    row's smallest value; only those take the exact rounding (clearance_rule.l3norm).  Same result as clearance_rule.step, rows updated in
    place."""
    n = len(radius)
    live = np.flatnonzero((np.asarray(entry_flags) & 7) == 0)
    for half, pts, radii, skip_self in (('agent', pos, radius, True), ('obs', obs_pos.reshape(-1, 3), obs_radius, False)):
        if len(radii) == 0 or (skip_self and n == 1):
            continue
        for lo in range(0, len(live), chunk):
            rows = live[lo:lo + chunk]
            d = pos[rows][:, None, :] - pts[None, :, :]
            s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
            s = s + d[..., 2] * d[..., 2]
            rough = np.sqrt(s) - (radius[rows][:, None] + radii[None, :])
            if skip_self:
                rough[np.arange(len(rows)), rows] = np.inf
            lim = rough.min(axis=1) + 2e-5
            for k, a in enumerate(rows):
                best, who = np.inf, -1
                for b in np.flatnonzero(rough[k] <= lim[k]):
                    c = rule.l3norm([float(x) for x in pos[a]], [float(x) for x in pts[b]]) - float(radius[a] + radii[b])
                    if c < best:
                        best, who = c, int(b)
                if best < rec[half + '_clear'][a]:
                    rec[half + '_clear'][a], rec[half + '_partner'][a], rec[half + '_step'][a] = best, who, step_no
    return rec
