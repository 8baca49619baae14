#!/usr/bin/env python
"""What respawning agents in place (sca_respawn_agents, sca_get_finished) costs.  ONE process; the parent commit's library is loaded beside
this build's (--root: the parent's checkout, built).  Three parts, merged into profiles/respawn_cost.json:

    step      the step time of a context that NEVER respawns, parent against this build: the two enqueue the same kernels.  The legs are
              alternated window by window; a window = start state, `--warm` untimed steps, one timed sca_run_steps burst of `--window` steps
              + synchronise.  Reported: the windows, medians, and whether this build's median lies inside the parent's own min-max.
    call      one sca_respawn_agents call naming 1 / 64 / 4096 rows (wall time around the Python call, `--samples` samples), beside the only
              route the parent has -- sca_set_agents + sca_set_state (+ sca_device_tracker_enable) -- and beside one step of the same context;
              sca_get_finished with 0 / 64 / all rows finished.
    lifelong  the ping-pong circle of examples/run_sca.py --lifelong at N = 4096 for `--lifelong-steps` steps: missions per second and live
              fraction, beside the parent re-running whole episodes (sca_set_agents again when everybody has finished) for as many steps.

workloads
    c3_auto   circle, N = 4096, ORCA3D, SCA_NBR_AUTO
    c4        circle, N = 100 000, SCA, the device tracker, SCA_NBR_KDTREE"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from scenes_cost import host, load_package                                            # noqa: E402

WORKLOADS = {
    'c3_auto': dict(n=4096, policy=3, mode='auto', tracked=False, desc='circle N=4096, ORCA3D, SCA_NBR_AUTO'),
    'c4': dict(n=100000, policy=0, mode='kd', tracked=True, desc='circle N=100000, SCA, device tracker, SCA_NBR_KDTREE'),
}


def make_leg(S, scenarios, w):
    sc = scenarios.circle(w['n'])
    n = len(sc['start'])
    policy = np.full(n, w['policy'], np.uint8)
    zaxis, mrd = S.zaxis_flags(sc['start'], sc['goal']), scenarios.max_run_dist(sc['start'], sc['goal'])
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
    mode = {'kd': S.NBR_KDTREE, 'auto': S.NBR_AUTO}[w['mode']]

    def define():
        sol.set_agents(np.full(n, 0.5), np.ones(n), sc['goal'][:, :3], policy, zaxis, mrd)

    def reset(flags=None):
        sol.set_state(sc['start'][:, :3], np.zeros((n, 3), np.float32), sc['start'][:, 3:6], np.zeros(n, np.uint8) if flags is None else flags)
        if w['tracked']:
            sol.device_tracker_enable(sc['goal'][:, 3:6])
    define()
    return dict(sol=sol, define=define, reset=reset, mode=mode, n=n, sc=sc)


def summary(ms):
    return {'samples_ms': [round(x, 5) for x in ms], 'median_ms': round(float(np.median(ms)), 5), 'min_ms': round(min(ms), 5), 'max_ms': round(max(ms), 5)}


def step_window(leg, args):
    leg['reset']()
    leg['sol'].run_steps(args.warm, leg['mode'])
    leg['sol'].synchronize()
    t0 = time.perf_counter()
    leg['sol'].run_steps(args.window, leg['mode'])
    leg['sol'].synchronize()
    return (time.perf_counter() - t0) * 1e3 / args.window


def part_step(here, parent, w, args):
    legs = {}
    if parent:
        legs['parent'] = make_leg(parent[0], parent[1], w)
    legs['here'] = make_leg(here[0], here[1], w)
    for leg in legs.values():
        step_window(leg, args)                                                        # every leg once untimed
    ms = {k: [] for k in legs}
    for _ in range(args.alternations):
        for k, leg in legs.items():
            ms[k].append(step_window(leg, args))
    out = {k: summary(v) for k, v in ms.items()}
    if parent:
        p, h = out['parent'], out['here']
        out['here_against_parent'] = {'here_median_ms': h['median_ms'], 'parent_median_ms': p['median_ms'], 'difference_ms': round(h['median_ms'] - p['median_ms'], 5),
                                      'parent_min_ms': p['min_ms'], 'parent_max_ms': p['max_ms'], 'inside_parent_spread': bool(p['min_ms'] <= h['median_ms'] <= p['max_ms'])}
    for leg in legs.values():
        leg['sol'].close()
    return out


def part_call(here, parent, w, args):
    leg = make_leg(here[0], here[1], w)
    sol, n, sc = leg['sol'], leg['n'], leg['sc']
    rng = np.random.default_rng(0)
    leg['reset']()
    sol.run_steps(args.warm, leg['mode'])
    sol.synchronize()
    out = {'respawn': {}, 'finished': {}}
    for count in (1, 64, 4096):
        ms = []
        for s in range(args.samples + 1):
            ids = np.sort(rng.choice(n, count, replace=False)).astype(np.int32)
            a = (ids, sc['start'][ids, :3], np.zeros((count, 3), np.float32), sc['start'][ids, 3:6], np.full(count, 0.5), np.ones(count), sc['goal'][ids, :3],
                 np.full(count, 1e6))
            t0 = time.perf_counter()
            sol.respawn(*a, goal_heading=sc['goal'][ids, 3:6] if w['tracked'] else None)
            if s:                                                                     # (the first call allocates the block)
                ms.append((time.perf_counter() - t0) * 1e3)
            sol.run_steps(1, leg['mode'])                                             # a step between the calls, as a lifelong loop has
            sol.synchronize()
        out['respawn'][str(count)] = summary(ms)
    ms = []
    for _ in range(args.samples):
        t0 = time.perf_counter()
        sol.run_steps(1, leg['mode'])
        sol.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    out['one_step'] = summary(ms)
    for name, k in (('0', 0), ('64', 64), ('all', n)):
        flags = np.zeros(n, np.uint8)
        flags[rng.choice(n, k, replace=False)] = 1
        leg['reset'](flags)
        ms = []
        for s in range(args.samples + 1):
            t0 = time.perf_counter()
            rows = sol.finished()
            if s:
                ms.append((time.perf_counter() - t0) * 1e3)
        assert len(rows) == k
        out['finished'][name] = summary(ms)
    t0 = time.perf_counter()
    sol.get_state()
    out['get_state_once_ms'] = round((time.perf_counter() - t0) * 1e3, 5)
    sol.close()
    # the only route the parent has to give one drone a new mission: the whole definition and state again
    for who, pkg in (('parent', parent), ('here', here)):
        if not pkg:
            continue
        leg = make_leg(pkg[0], pkg[1], w)
        leg['reset']()
        ms = []
        for _ in range(max(3, args.samples // 6)):
            t0 = time.perf_counter()
            leg['define']()
            leg['reset']()
            ms.append((time.perf_counter() - t0) * 1e3)
        out['set_agents_route_' + who] = summary(ms)
        leg['sol'].close()
    return out


def part_lifelong(here_root, parent_root, args):
    n, steps = 4096, args.lifelong_steps
    out = {}

    def agents_of(E):
        return E.build_circle_agents(n, policy=E.ORCA3DPolicy)
    E = importlib.import_module('sca_here.env')
    LL = importlib.import_module('sca_here.lifelong')
    env = E.MACAEnv()
    agents = agents_of(E)
    env.set_agents(agents, obstacles=[])
    first = {a.id: (list(a.initial_pos), list(a.goal_pos)) for a in agents}

    def next_mission(agent, row):
        if int(row['flags']) & 2 or not int(row['flags']) & 1:
            start, goal = first[agent.id]
        else:
            start, goal = list(row['pos']) + list(agent.heading_global_frame), list(agent.initial_pos)
        return E.Agent(start_pos=start, goal_pos=goal, vel=[0.0, 0.0, 0.0], radius=agent.radius, pref_speed=agent.pref_speed, policy=E.ORCA3DPolicy, id=agent.id)
    t0 = time.perf_counter()
    stats = LL.run_lifelong(env, next_mission, steps)
    dt = time.perf_counter() - t0
    missions = stats['arrived'] + stats['collided'] + stats['timed_out']
    out['here_lifelong'] = dict(stats, seconds=round(dt, 3), missions=missions, missions_per_s=round(missions / dt, 2), steps_per_s=round(stats['steps'] / dt, 1))
    env.solver.close()
    if parent_root:                                                                   # whole episodes, one after the other, for as many steps
        EP = importlib.import_module('sca_parent.env')
        t0 = time.perf_counter()
        done_steps = missions = agent_steps = episodes = 0
        while done_steps < steps:
            env = EP.MACAEnv()
            env.set_agents(agents_of(EP), obstacles=[])
            episodes += 1
            while done_steps < steps:
                agent_steps += env._active
                finished = env.step()
                done_steps += 1
                if finished:
                    break
            missions += int((env.flags & 7 != 0).sum())
            env.solver.close()
        dt = time.perf_counter() - t0
        out['parent_episodes'] = dict(steps=done_steps, episodes_begun=episodes, missions=missions, seconds=round(dt, 3), missions_per_s=round(missions / dt, 2),
                                      steps_per_s=round(done_steps / dt, 1), agent_steps=agent_steps, live_fraction=round(agent_steps / float(n * done_steps), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=None, help="the parent commit's checkout (built)")
    ap.add_argument('--parts', default='step,call,lifelong')
    ap.add_argument('--workloads', default=','.join(WORKLOADS))
    ap.add_argument('--window', type=int, default=200)
    ap.add_argument('--warm', type=int, default=20)
    ap.add_argument('--alternations', type=int, default=5)
    ap.add_argument('--samples', type=int, default=30)
    ap.add_argument('--lifelong-steps', type=int, default=2000)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'respawn_cost.json'))
    args = ap.parse_args()
    here = load_package(REPO, 'sca_here')
    parent = load_package(args.root, 'sca_parent') if args.root else None
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result.update(host=host(), window_steps=args.window, warm_steps=args.warm, alternations=args.alternations, samples=args.samples)
    parts = args.parts.split(',')

    def save():                                                                       # after every part: a later part that fails loses nothing
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write('\n')
    for name in args.workloads.split(','):
        w = WORKLOADS[name]
        entry = result.setdefault('workloads', {}).setdefault(name, {'desc': w['desc'], 'n': w['n']})
        if 'step' in parts:
            entry['step'] = part_step(here, parent, w, args)
            print(name, 'step', json.dumps(entry['step']), flush=True)
            save()
        if 'call' in parts:
            entry['call'] = part_call(here, parent, w, args)
            print(name, 'call', json.dumps(entry['call']), flush=True)
            save()
    if 'lifelong' in parts:
        key = 'lifelong_circle_4096_%d_steps' % args.lifelong_steps
        result[key] = part_lifelong(REPO, args.root, args)
        print(key, json.dumps(result[key]), flush=True)
    save()


if __name__ == '__main__':
    main()
