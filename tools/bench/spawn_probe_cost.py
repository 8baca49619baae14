#!/usr/bin/env python
"""What spawn admission (sca_probe_clearance, sca_respawn_agents_gated) costs.  ONE process; the parent commit's library is loaded beside
this build's (--root: the parent's checkout, built).  Three parts, merged into profiles/spawn_probe_cost.json:

    step      the step time of a context that NEVER probes, parent against this build: the two enqueue the same kernels.  The legs are
              alternated window by window (respawn_cost.py's windows); reported: the windows, medians, and whether this build's median
              lies inside the parent's own min-max -- no fixed number.
    call      one call at both sizes, `--samples` samples, wall time around the Python call: probe_clearance with 1 / 64 / 4096 queries,
              the gated respawn naming 1 / 64 / 4096 rows beside respawn naming the same rows, and one step of the same context.
    lifelong  the ping-pong circle of examples/run_sca.py --lifelong at N = 4096 ORCA3D for `--lifelong-steps` steps, without a margin and
              with --spawn-margin: missions, arrivals, collisions, deferred, missions per second.

workloads: respawn_cost.py's (c3_auto: circle N = 4096 ORCA3D SCA_NBR_AUTO; c4: circle N = 100 000 SCA, device tracker, SCA_NBR_KDTREE)"""
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
from respawn_cost import WORKLOADS, make_leg, step_window, summary                    # noqa: E402
from scenes_cost import host, load_package                                            # noqa: E402


def part_step(here, parent, w, args):
    """respawn_cost.py's part_step with the order of the two legs as an option: the context made first and timed first in every round is
    the parent's, or with --here-first this build's -- two contexts of one process differ by more than one context's windows spread"""
    order = [('here', here), ('parent', parent)] if args.here_first else [('parent', parent), ('here', here)]
    legs = {k: make_leg(pkg[0], pkg[1], w) for k, pkg in order if pkg}
    for leg in legs.values():
        step_window(leg, args)                                                        # every leg once untimed
    ms = {k: [] for k in legs}
    for _ in range(args.alternations):
        for k, leg in legs.items():
            ms[k].append(step_window(leg, args))
    out = {k: summary(v) for k, v in ms.items()}
    out['order'] = list(legs)
    if parent:
        p, h = out['parent'], out['here']
        out['here_against_parent'] = {'here_median_ms': h['median_ms'], 'parent_median_ms': p['median_ms'], 'difference_ms': round(h['median_ms'] - p['median_ms'], 5),
                                      'parent_min_ms': p['min_ms'], 'parent_max_ms': p['max_ms'], 'inside_parent_spread': bool(p['min_ms'] <= h['median_ms'] <= p['max_ms'])}
    for leg in legs.values():
        leg['sol'].close()
    return out


def part_call(here, w, args):
    leg = make_leg(here[0], here[1], w)
    sol, n, sc = leg['sol'], leg['n'], leg['sc']
    rng = np.random.default_rng(0)
    leg['reset']()
    sol.run_steps(args.warm, leg['mode'])
    sol.synchronize()
    out = {'probe': {}, 'respawn_gated': {}, 'respawn': {}, 'admitted_of': {}}
    lo, hi = sc['start'][:, :3].min(axis=0), sc['start'][:, :3].max(axis=0)
    for count in (1, 64, 4096):
        ms = []
        for s in range(args.samples + 1):
            q = rng.uniform(lo, hi, (count, 3))
            t0 = time.perf_counter()
            sol.probe_clearance(q, 0.5)
            if s:                                                                     # (the first call allocates the block and the scratch)
                ms.append((time.perf_counter() - t0) * 1e3)
        out['probe'][str(count)] = summary(ms)
    for count in (1, 64, 4096):
        gated, plain, admitted = [], [], 0
        for s in range(args.samples + 1):
            for which, ms in (('gated', gated), ('plain', plain)):
                ids = np.sort(rng.choice(n, count, replace=False)).astype(np.int32)
                a = (ids, sc['start'][ids, :3], np.zeros((count, 3), np.float32), sc['start'][ids, 3:6], np.full(count, 0.5), np.ones(count), sc['goal'][ids, :3],
                     np.full(count, 1e6))
                gh = sc['goal'][ids, 3:6] if w['tracked'] else None
                t0 = time.perf_counter()
                got = sol.respawn(*a, goal_heading=gh, margin=args.margin if which == 'gated' else None)
                if s:
                    ms.append((time.perf_counter() - t0) * 1e3)
                    admitted += int((got[0] == 0).sum()) if which == 'gated' else 0
                sol.run_steps(1, leg['mode'])                                         # a step between the calls, as a lifelong loop has
                sol.synchronize()
        out['respawn_gated'][str(count)], out['respawn'][str(count)] = summary(gated), summary(plain)
        out['admitted_of'][str(count)] = [admitted, count * args.samples]
    ms = []
    for _ in range(args.samples):
        t0 = time.perf_counter()
        sol.run_steps(1, leg['mode'])
        sol.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    out['one_step'] = summary(ms)
    sol.close()
    return out


def part_lifelong(args):
    n, steps = 4096, args.lifelong_steps
    E = importlib.import_module('sca_here.env')
    LL = importlib.import_module('sca_here.lifelong')
    out = {}
    for name, margin in (('no_margin', None), ('spawn_margin_%g' % args.margin, args.margin)):
        env = E.MACAEnv()
        agents = E.build_circle_agents(n, policy=E.ORCA3DPolicy)
        env.set_agents(agents, obstacles=[])
        first = {a.id: (list(a.initial_pos), list(a.goal_pos)) for a in agents}

        def next_mission(agent, row):
            if int(row['flags']) & 2 or not int(row['flags']) & 1:
                start, goal = first[agent.id]
            else:
                start, goal = list(row['pos']) + list(agent.heading_global_frame), list(agent.initial_pos)
            return E.Agent(start_pos=start, goal_pos=goal, vel=[0.0, 0.0, 0.0], radius=agent.radius, pref_speed=agent.pref_speed, policy=E.ORCA3DPolicy, id=agent.id)
        t0 = time.perf_counter()
        stats = LL.run_lifelong(env, next_mission, steps) if margin is None else LL.run_lifelong(env, next_mission, steps, spawn_margin=margin)
        dt = time.perf_counter() - t0
        missions = stats['arrived'] + stats['collided'] + stats['timed_out']
        out[name] = dict(stats, seconds=round(dt, 3), missions=missions, missions_per_s=round(missions / dt, 2), steps_per_s=round(stats['steps'] / dt, 1))
        env.solver.close()
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
    ap.add_argument('--margin', type=float, default=0.5)
    ap.add_argument('--here-first', action='store_true', help='step part: this build\'s context is made and timed first')
    ap.add_argument('--lifelong-steps', type=int, default=20000)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'spawn_probe_cost.json'))
    args = ap.parse_args()
    here = load_package(REPO, 'sca_here')
    parent = load_package(args.root, 'sca_parent') if args.root else None
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result.update(host=host(), window_steps=args.window, warm_steps=args.warm, alternations=args.alternations, samples=args.samples, margin=args.margin)
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
            entry['step_here_first' if args.here_first else 'step'] = step = part_step(here, parent, w, args)
            print(name, 'step', json.dumps(step), flush=True)
            save()
        if 'call' in parts:
            entry['call'] = part_call(here, w, args)
            print(name, 'call', json.dumps(entry['call']), flush=True)
            save()
    if 'lifelong' in parts:
        key = 'lifelong_circle_4096_%d_steps' % args.lifelong_steps
        result[key] = part_lifelong(args)
        print(key, json.dumps(result[key]), flush=True)
    save()


if __name__ == '__main__':
    main()
