#!/usr/bin/env python
"""What mission tables (sca_set_missions: finished rows take their next mission inside the step) cost.  ONE process; the parent commit's
library is loaded beside this build's (--root: the parent's checkout, built).  Four parts, merged into profiles/mission_cost.json:

    step      the step time of a context that NEVER sets tables, parent against this build: the two enqueue the same kernels.  The legs are
              alternated window by window (spawn_probe_cost.py's part_step; --here-first swaps the context that is made first); reported:
              the windows, medians, and whether this build's median lies inside the parent's own min-max -- no fixed number.
    tables    this build, tables set and nobody ending against no tables, alternated the same way, in two step forms: `burst` (one
              sca_run_steps of the window: with tables an AUTO burst builds no tree ahead and lets no event ride) and `stepwise`
              (sca_run_steps(1) per step, which plans none of that in either leg: what is left is the dispatch and the read of the flag words).
    lifelong  the ping-pong circle at N = 4096 ORCA3D for `--lifelong-steps` steps under ONE rule (the three-entry table of
              examples/run_sca.py --device-missions): run_lifelong driven by that rule on the host, run_missions at burst 1 and at burst 64;
              steps/s, missions/s and whether the three stats are identical.
    collect   sca_get_mission_results with 0 / 64 / all rows holding a new result beside sca_get_finished listing as many rows, N = 4096.

--gate (the admission gate on the device, sca_set_mission_gate; merged into profiles/mission_gate_cost.json):
    step      as above, and beside it `step_tables`: both builds with idle tables set and no gate -- they enqueue the same kernels
    tables    becomes `gate`: idle tables in both legs, the gate (margin 0.5) on against off, nobody ending: the five kernels in place of
              k_mission_advance, four dependent dispatches more
    lifelong  run_lifelong(spawn_margin=0.5) against run_missions(spawn_margin=0.5) at burst 1 and 64, refusals and waiting beside the rates
    collect   left out
    bench     (only when named in --parts, with --root) `bench.py --gpus 1 --steps 200 --warmup 20` as a child process, the parent's checkout and
              this one alternated twice, in front of everything else: the ms_per_step of each run's JSON line

--paths (tables whose entries bring their own waypoint lists, sca_set_missions_paths; merged into profiles/mission_paths_cost.json):
    step      as above, and `step_tables` as under --gate: idle tables WITHOUT lists in both builds -- the same kernels apart from the changed
              symbols (k_mission_advance's take goes through the shared helper)
    tables    becomes `paths`: both legs in slot form (W = 2, every row holds a list of two points, so k_waypoint_slots runs in both) with
              idle tables set through sca_set_missions_paths, nobody ending -- `off`: every entry brings the empty list,
              `on`: every entry brings a list of two points.  The two enqueue the same kernels: the work rides in the take
    lifelong  the circle with routes of two waypoints per leg, reversed on the way back (examples/run_sca.py --waypoints 2): run_lifelong
              whose next_mission hands out the routes against run_missions whose entries bring them, at burst 1 and 64
    collect   left out
    bench     as under --gate

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
from spawn_probe_cost import part_step                                                # noqa: E402


def idle_tables(_lib, sc, n):
    """one entry per row that nobody takes before the window ends: from where it stands to its start, after an arrival"""
    e = np.zeros((n, 1), _lib.MISSION_DTYPE)
    e['goal'][:, 0], e['goal_heading'][:, 0] = sc['start'][:, :3], sc['start'][:, 3:6]
    e['pref_speed'], e['max_run_dist'], e['flags'] = 1.0, 1e6, 1
    e['next_ok'], e['next_fail'] = 0, 0
    return e, np.zeros(n, np.int32), np.zeros(n, np.int32)


def stepwise_window(leg, args):
    leg['reset']()
    sol, mode = leg['sol'], leg['mode']
    for _ in range(args.warm):
        sol.run_steps(1, mode)
    sol.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.window):
        sol.run_steps(1, mode)
    sol.synchronize()
    return (time.perf_counter() - t0) * 1e3 / args.window


def part_step_tables(here, parent, w, args):
    """part_step with idle tables set in both builds' contexts and no gate anywhere"""
    order = [('here', here), ('parent', parent)] if args.here_first else [('parent', parent), ('here', here)]
    legs = {}
    for k, pkg in order:
        leg = make_leg(pkg[0], pkg[1], w)
        e, ok, fail = idle_tables(importlib.import_module('sca_here._lib'), leg['sc'], leg['n'])
        leg['sol'].set_missions(1, 1, e, ok, fail)
        legs[k] = leg
    for leg in legs.values():
        step_window(leg, args)
    ms = {k: [] for k in legs}
    for _ in range(args.alternations):
        for k, leg in legs.items():
            ms[k].append(step_window(leg, args))
    out = {k: summary(v) for k, v in ms.items()}
    out['order'] = list(legs)
    p, h = out['parent'], out['here']
    out['here_against_parent'] = {'here_median_ms': h['median_ms'], 'parent_median_ms': p['median_ms'], 'difference_ms': round(h['median_ms'] - p['median_ms'], 5),
                                  'parent_min_ms': p['min_ms'], 'parent_max_ms': p['max_ms'], 'inside_parent_spread': bool(p['min_ms'] <= h['median_ms'] <= p['max_ms'])}
    for leg in legs.values():
        leg['sol'].close()
    return out


def part_tables(here, w, args):
    S, scenarios = here[0], here[1]
    _lib = importlib.import_module('sca_here._lib')
    order = ['on', 'off'] if args.here_first else ['off', 'on']
    legs = {k: make_leg(S, scenarios, w) for k in order}
    e, ok, fail = idle_tables(_lib, legs['on']['sc'], legs['on']['n'])
    if args.paths:                                                                    # slot form and tables in both legs, the entries' lists in one
        for k, leg in legs.items():
            sc, n = leg['sc'], leg['n']
            mid = [[list(map(float, sc['start'][i, :3] + (sc['goal'][i, :3] - sc['start'][i, :3]) * f)) for f in (0.7, 0.3)] for i in range(n)]
            leg['sol'].set_path_slots(2, mid)
            leg['sol'].set_missions(1, 1, e, ok, fail, paths=mid if k == 'on' else {})
            reset = leg['reset']
            leg['reset'] = lambda reset=reset, sol=leg['sol'], n=n: (reset(), sol.set_path_state(np.full(n, 2, np.int32), np.full((n, 3), np.nan)))
    else:
        legs['on']['sol'].set_missions(1, 1, e, ok, fail)
    if args.gate:                                                                     # tables in both legs, the gate in one
        legs['off']['sol'].set_missions(1, 1, e, ok, fail)
        legs['on']['sol'].set_mission_gate(0.5)
    out = {'order': order}
    for form, window in (('burst', step_window), ('stepwise', stepwise_window)):
        for leg in legs.values():
            window(leg, args)
        ms = {k: [] for k in legs}
        for _ in range(args.alternations):
            for k, leg in legs.items():
                ms[k].append(window(leg, args))
        o = {k: summary(v) for k, v in ms.items()}
        o['on_minus_off_ms'] = round(o['on']['median_ms'] - o['off']['median_ms'], 5)
        o['inside_off_spread'] = bool(o['off']['min_ms'] <= o['on']['median_ms'] <= o['off']['max_ms'])
        out[form] = o
    t = legs['on']['sol'].mission_totals()
    out['endings_in_the_on_leg'] = t['arrived'] + t['collided'] + t['timed_out']
    if args.gate:
        out['offered_in_the_on_leg'] = legs['on']['sol'].mission_gate_totals()['offered']
        out['added_dependent_dispatches'] = 4
    for leg in legs.values():
        leg['sol'].close()
    return out


def part_lifelong(args):
    n, steps = 4096, args.lifelong_steps
    E = importlib.import_module('sca_here.env')
    LL = importlib.import_module('sca_here.lifelong')

    def world():
        env = E.MACAEnv(path_slots=2) if args.paths else E.MACAEnv()
        agents = E.build_circle_agents(n, policy=E.ORCA3DPolicy)
        first = {a.id: (list(a.initial_pos), list(a.goal_pos)) for a in agents}
        route = {}
        if args.paths:                                                                # two seeded waypoints per leg, reversed on the way back (the example's --waypoints 2)
            for i, (s, g) in first.items():
                rng = np.random.default_rng(1000 + i)
                p, q = np.asarray(s[:3], float), np.asarray(g[:3], float)
                route[i] = [[float(x) for x in np.round(p + (q - p) * (k + 1) / 3 + rng.normal(0.0, 0.5, 3), 3)] for k in range(2)]
            for a in agents:
                a.path = route[a.id][::-1]
        env.set_agents(agents, obstacles=[])

        def entry(i, start, goal):
            return E.Agent(start_pos=start, goal_pos=goal, vel=[0.0, 0.0, 0.0], radius=agents[i].radius, pref_speed=agents[i].pref_speed, policy=E.ORCA3DPolicy, id=i)
        tables = {i: E.MissionTable([entry(i, goal, start), entry(i, start, goal), entry(i, start, goal)], next_ok=[1, 0, 0], next_fail=[2, 2, 2], first_ok=0, first_fail=2,
                                    start_here=[True, True, False], path=[route[i][:], route[i][::-1], route[i][::-1]] if args.paths else None)
                  for i, (start, goal) in first.items()}
        return env, tables, entry
    out = {}
    for name in ('run_lifelong', 'run_missions_burst_1', 'run_missions_burst_64'):
        env, T, entry = world()
        t0 = time.perf_counter()
        if name == 'run_lifelong':
            state = dict.fromkeys(T, -1)

            def next_mission(a, row):
                f = int(row['flags'])
                arrived = bool(f & 1) and not f & 2
                t, c = T[a.id], state[a.id]
                j = (t.first_ok if arrived else t.first_fail) if c < 0 else (t.next_ok[c] if arrived else t.next_fail[c])
                state[a.id] = j
                src, here, _ = t.entries[j]
                new = entry(a.id, list(row['pos']) + list(a.heading_global_frame) if here else list(src.initial_pos), list(src.goal_pos))
                new.max_run_dist = src.max_run_dist
                if args.paths:
                    new.path = [w[:] for w in t.paths[j]]
                return new
            stats = LL.run_lifelong(env, next_mission, steps, **({'spawn_margin': 0.5} if args.gate else {}))
        else:
            stats = LL.run_missions(env, T, steps, burst=int(name.rsplit('_', 1)[1]), **({'spawn_margin': 0.5} if args.gate else {}))
        dt = time.perf_counter() - t0
        missions = stats['arrived'] + stats['collided'] + stats['timed_out']
        out[name] = dict(stats, seconds=round(dt, 3), missions=missions, missions_per_s=round(missions / dt, 2), steps_per_s=round(stats['steps'] / dt, 1))
        env.solver.close()
    keys = ('steps', 'arrived', 'collided', 'timed_out', 'respawned', 'retired', 'agent_steps', 'live_fraction') + (('deferred', 'waiting') if args.gate else ())
    out['stats_identical'] = all(out[a][k] == out['run_lifelong'][k] for a in out for k in keys)
    return out


def part_bench(args):
    """bench.py of both checkouts as child processes, parent / here alternated twice"""
    import subprocess
    out = {'order': [], 'parent': [], 'here': [], 'command': 'bench.py --gpus 1 --steps 200 --warmup 20'}
    for _ in range(2):
        for name, root in (('parent', os.path.abspath(args.root)), ('here', REPO)):
            r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '200', '--warmup', '20'], cwd=root, capture_output=True, text=True,
                               check=True)
            line = [x for x in r.stdout.splitlines() if x.startswith('{"metric"')][-1]
            out['order'].append(name)
            out[name].append(json.loads(line)['ms_per_step'])
    return out


def part_collect(here, args):
    S, scenarios = here[0], here[1]
    _lib = importlib.import_module('sca_here._lib')
    n = 4096
    sc = scenarios.circle(n)
    zaxis = S.zaxis_flags(sc['start'], sc['goal'])
    out = {}
    for count in (0, 64, n):
        mrd = np.full(n, 1e6)
        mrd[np.linspace(0, n - 1, count).astype(int) if count else []] = 0.05          # these rows time out in their first step and stop
        sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
        sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
        sol.set_agents(np.full(n, 0.5), np.ones(n), sc['goal'][:, :3], np.full(n, 3, np.uint8), zaxis, mrd)
        e, ok, fail = idle_tables(_lib, sc, n)
        e['next_ok'], e['next_fail'] = -1, -1
        sol.set_missions(1, 1, e, np.where(mrd < 1.0, 0, -1).astype(np.int32), np.full(n, -1, np.int32))   # (these rows have a table; a failure stops them)
        fin, res = [], []
        for s in range(args.samples + 1):
            sol.set_state(sc['start'][:, :3], np.zeros((n, 3), np.float32), sc['start'][:, 3:6], np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.int32))
            sol.run_steps(2, S.NBR_KDTREE)
            sol.synchronize()
            t0 = time.perf_counter()
            f = sol.finished()
            t1 = time.perf_counter()
            r = sol.mission_results()
            t2 = time.perf_counter()
            if s:
                fin.append((t1 - t0) * 1e3)
                res.append((t2 - t1) * 1e3)
            got = len(r)
        out[str(count)] = {'get_finished': summary(fin), 'get_mission_results': summary(res), 'results': got, 'finished_rows': len(f)}
        sol.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=None, help="the parent commit's checkout (built)")
    ap.add_argument('--parts', default='step,tables,lifelong,collect')
    ap.add_argument('--workloads', default=','.join(WORKLOADS))
    ap.add_argument('--window', type=int, default=200)
    ap.add_argument('--warm', type=int, default=20)
    ap.add_argument('--alternations', type=int, default=5)
    ap.add_argument('--samples', type=int, default=30)
    ap.add_argument('--here-first', action='store_true', help='step and tables parts: this build\'s (the tables\') context is made and timed first')
    ap.add_argument('--lifelong-steps', type=int, default=20000)
    ap.add_argument('--gate', action='store_true', help='the admission gate on the device: see above; --out defaults to profiles/mission_gate_cost.json')
    ap.add_argument('--paths', action='store_true', help='tables whose entries bring waypoint lists: see above; --out defaults to profiles/mission_paths_cost.json')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.gate and args.paths:
        ap.error('--gate and --paths are two legs: one at a time')
    if args.out is None:
        args.out = os.path.join(REPO, 'profiles', 'mission_gate_cost.json' if args.gate else 'mission_paths_cost.json' if args.paths else 'mission_cost.json')
    bench = part_bench(args) if 'bench' in args.parts.split(',') and args.root else None      # (in front of everything that opens the GPU here)
    here = load_package(REPO, 'sca_here')
    parent = load_package(args.root, 'sca_parent') if args.root else None
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result.update(host=host(), window_steps=args.window, warm_steps=args.warm, alternations=args.alternations, samples=args.samples)
    parts = args.parts.split(',')
    if bench:
        result['bench_py_gpus_1_steps_200_warmup_20_ms_per_step'] = bench
        print('bench', json.dumps(bench), flush=True)
    suffix = '_here_first' if args.here_first else ''

    def save():                                                                       # after every part: a later part that fails loses nothing
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write('\n')
    for name in args.workloads.split(','):
        w = WORKLOADS[name]
        entry = result.setdefault('workloads', {}).setdefault(name, {'desc': w['desc'], 'n': w['n']})
        if 'step' in parts:
            entry['step' + suffix] = part_step(here, parent, w, args)
            print(name, 'step', json.dumps(entry['step' + suffix]), flush=True)
            save()
            if (args.gate or args.paths) and parent:
                entry['step_tables' + suffix] = part_step_tables(here, parent, w, args)
                print(name, 'step_tables', json.dumps(entry['step_tables' + suffix]), flush=True)
                save()
        if 'tables' in parts:
            key = ('gate' if args.gate else 'paths' if args.paths else 'tables') + suffix
            entry[key] = part_tables(here, w, args)
            print(name, key, json.dumps(entry[key]), flush=True)
            save()
    if 'lifelong' in parts:
        key = 'lifelong_circle_4096_%d_steps' % args.lifelong_steps + ('_margin_0.5' if args.gate else '_waypoints_2' if args.paths else '')
        result[key] = part_lifelong(args)
        print(key, json.dumps(result[key]), flush=True)
        save()
    if 'collect' in parts and not args.gate and not args.paths:
        result['collect_4096'] = part_collect(here, args)
        print('collect', json.dumps(result['collect_4096']), flush=True)
    save()


if __name__ == '__main__':
    main()
