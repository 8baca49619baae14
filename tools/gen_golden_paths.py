#!/usr/bin/env python3
"""Golden episodes with waypoint lists (Agent.path, agent.py:44) -- runs ONLY in the build container, never on the GPU box.

Imports the read-only reference checkout at run time, as tools/gen_golden.py does, and reuses that script's recorder
(run_env_episode: the per-step arrays of every other episode fixture) without changing what it writes.  Around it:
  * MACAEnv.set_agents is wrapped to give every agent its waypoint list before the env sees it (the way a user of the reference sets
    agent.path after building the agents);
  * MACAEnv.step is wrapped to read every agent's policy.now_goal and len(agent.path) before and after the step.
Each fixture gets, besides the usual arrays: path_off [n + 1] / path_pts [total, 3] (the lists in CSR form, list order: the reference
pops from the end), now_goal_before / now_goal_after [rec, n, 3] (NaN rows: None) and path_left_before / path_left_after [rec, n].

They go to tests/golden/paths/: the episode suites glob tests/golden/F[1-69]*_*.npz and run every match WITHOUT lists.

Usage:  python tools/gen_golden_paths.py [--only NAME ...] [--ref /root/reference]
"""
import argparse
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G  # noqa: E402

POL_SCA, POL_RVO, POL_SRVO, POL_ORCA, POL_ORCA_LP, POL_RVO_DUBINS = range(6)
PATHS = None            # the lists of the scene being recorded, per agent id
TRACE = []              # per env.step: (now_goal before, path left before, now_goal after, path left after)


def _path_state(agents):
    n = len(agents)
    ng = np.full((n, 3), np.nan)
    left = np.zeros(n, np.int32)
    for a in agents:
        g = a.policy.now_goal
        if g is not None:
            ng[a.id] = np.asarray(g, dtype=np.float64)[:3]
        left[a.id] = len(a.path)
    return ng, left


def _install(env_mod):
    cls = env_mod.MACAEnv
    orig_set, orig_step = cls.set_agents, cls.step

    def set_agents(self, agents, obstacles=None):
        for a in agents:
            a.path = [list(map(float, w)) for w in PATHS[a.id]]
        return orig_set(self, agents, obstacles=obstacles)

    def step(self, actions):
        before = _path_state(self.agents)
        out = orig_step(self, actions)
        TRACE.append(before + _path_state(self.agents))
        return out
    cls.set_agents = set_agents
    cls.step = step


def record(agent_mod, env_mod, classes, name, pos, goal, policy, obs, steps, paths, outdir, **kw):
    global PATHS
    PATHS = paths
    TRACE.clear()
    G.run_env_episode(agent_mod, env_mod, classes, name, pos, goal, policy, obs, steps, outdir=outdir, **kw)
    path = os.path.join(outdir, name + '.npz')
    out = dict(np.load(path, allow_pickle=False))
    sel = [int(s) for s in out['step']]
    for j, key in enumerate(('now_goal_before', 'path_left_before', 'now_goal_after', 'path_left_after')):
        out[key] = np.array([TRACE[s][j] for s in sel])
    lens = [len(p) for p in paths]
    off = np.zeros(len(paths) + 1, np.int32)
    off[1:] = np.cumsum(lens)
    pts = np.array([w for p in paths for w in p], dtype=np.float64).reshape(-1, 3)
    out['path_off'], out['path_pts'] = off, pts
    np.savez_compressed(path, **out)
    print(f'  {name}: {int(off[-1])} waypoints, {os.path.getsize(path) / 1e3:.0f} kB with the path arrays', flush=True)


def detours(pos, goal, seed, kmin=2, kmax=4, lateral=2.5):
    """2-4 waypoints per agent off the straight line start -> goal (sideways and up / down), in the order the reference's list holds
    them: the first one to fly to LAST (list.pop())."""
    rng = np.random.default_rng(seed)
    out = []
    for s, g in zip(pos, goal):
        s, g = np.asarray(s[:3], float), np.asarray(g[:3], float)
        d = g - s
        side = np.cross(d, [0.0, 0.0, 1.0])
        nrm = np.linalg.norm(side)
        side = side / nrm if nrm > 1e-9 else np.array([1.0, 0.0, 0.0])
        k = int(rng.integers(kmin, kmax + 1))
        ts = np.sort(rng.uniform(0.15, 0.85, k))
        wps = []
        for t in ts:
            w = s + t * d + rng.uniform(-lateral, lateral) * side + np.array([0.0, 0.0, rng.uniform(-1.0, 1.0)])
            wps.append([round(float(x), 2) for x in w])
        out.append(wps[::-1])
    return out


def edge_scene():
    """Ten agents, far enough apart to meet only late, one case of the rule each (see the list in the fixture's docstring below)."""
    P = []
    # (start xyz, goal xyz, policy, radius, pref_speed, path in list order)
    S = [([0, 0, 5], [12, 0, 5]), ([0, 6, 5], [12, 6, 5]), ([0, 12, 5], [12, 12, 5]), ([0, 18, 5], [12, 18, 5]), ([0, 24, 5], [12, 24, 5]),
         ([0, 30, 5], [12, 30, 5]), ([0, 36, 5], [12, 36, 5]), ([0, 42, 5], [12, 42, 5]), ([0, 48, 5], [12, 48, 5]), ([0, 54, 5], [12, 54, 5])]
    cases = [
        (POL_RVO, 0.5, 1.0, []),                                                   # 0: an empty list: now_goal = goal
        (POL_RVO, 0.4, 1.2, [[6.0, 8.0, 6.0]]),                                     # 1: a single waypoint
        (POL_SRVO, 0.6, 0.9, [[8.0, 14.5, 5.0], [0.3, 12.2, 5.0]]),                # 2: first waypoint within radius of the start: double pop
        (POL_ORCA, 0.5, 1.0, [[7.0, 20.0, 5.5], [-3.0, 18.0, 5.0]]),               # 3: a waypoint behind the start (the elif branch)
        (POL_ORCA_LP, 0.45, 1.1, [[5.0, 26.0, 5.0], [5.0, 26.0, 5.0], [5.0, 26.0, 5.0]]),   # 4: duplicate waypoints
        (POL_RVO, 0.5, 0.8, [[12.0, 30.0, 5.0], [4.0, 32.0, 6.0]]),                 # 5: the last waypoint is the goal
        (POL_SCA, 0.5, 1.0, [[8.0, 37.0, 5.0], [4.0, 35.0, 5.0]]),                 # 6: SCA: the list advances, v_pref stays the tracker's
        (POL_RVO_DUBINS, 0.5, 1.0, [[8.0, 43.0, 5.0], [4.0, 41.0, 5.0]]),          # 7: RVO3D+Dubins likewise
        (POL_SRVO, 0.5, 1.0, [[12.3, 48.0, 5.0]] * 30),                            # 8: at its goal with waypoints left
        (POL_ORCA, 0.55, 1.3, [[9.0, 52.0, 4.0], [6.0, 57.0, 6.0], [3.0, 55.0, 5.0], [1.5, 53.0, 5.0]]),  # 9: four in a row
    ]
    pos = [np.array(s + [0.0, 0.0, 0.0], float) for s, _ in S]
    goal = [np.array(g + [0.0, 0.0, 0.0], float) for _, g in S]
    pol = [c[0] for c in cases]
    rad = [c[1] for c in cases]
    psp = [c[2] for c in cases]
    P = [c[3] for c in cases]
    return pos, goal, pol, rad, psp, P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default='/root/reference')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'paths'))
    ap.add_argument('--only', nargs='*', default=None)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    agent_mod, env_mod, mods, classes = G._import_reference(args.ref)
    G._install_wrappers(mods)
    _install(env_mod)
    import run_sca as rs
    import run_orca as ro

    def want(nm):
        return args.only is None or any(nm.startswith(o) for o in args.only)

    od = args.out
    ring = [([round(4.0 * np.cos(2 * j * np.pi / 8), 2), round(4.0 * np.sin(2 * j * np.pi / 8), 2), 5.0], 1.0) for j in range(8)]
    for pid, nm in ((POL_RVO, 'F19_path_rvo_circle16'), (POL_SRVO, 'F19_path_srvo_circle16')):
        if want(nm):
            pos, goal = rs.set_circle_pos((0, 0), 10.0, 16)
            record(agent_mod, env_mod, classes, nm, pos, goal, [pid] * 16, [], 400, detours(pos, goal, seed=190 + pid), od, record_every=2)
    if want('F19_path_orca_circle16_obs'):
        pos, goal = rs.set_circle_pos((0, 0), 10.0, 16)
        record(agent_mod, env_mod, classes, 'F19_path_orca_circle16_obs', pos, goal, [POL_ORCA] * 16, ring, 400,
               detours(pos, goal, seed=193), od, record_every=2)
    if want('F19_path_orcalp_random30'):
        random.seed(19)
        pos, goal, _ = ro.set_random_pos(30)
        record(agent_mod, env_mod, classes, 'F19_path_orcalp_random30', pos, goal, [POL_ORCA_LP] * 30, [], 200,
               detours(pos, goal, seed=194, kmin=0, kmax=4), od, record_every=2)
    if want('F19_path_edge10'):
        pos, goal, pol, rad, psp, paths = edge_scene()
        record(agent_mod, env_mod, classes, 'F19_path_edge10', pos, goal, pol, [], 300, paths, od, radius=rad, pref_speed=psp)


if __name__ == '__main__':
    main()
