#!/usr/bin/env python
"""What vacant rows in a plain context (sca_retire_agents / sca_get_vacant, a respawn that admits) cost.  ONE process; the parent commit's
library is loaded beside this build's (--root: the parent's checkout, built).  Parts, merged into profiles/vacancy_cost.json:

    bench     `bench.py --gpus 1 --steps 200 --warmup 20` as a child process, the parent's checkout and this one alternated twice, in front
              of everything else: the ms_per_step of each run's JSON line.
    step      the step time of a context that NEVER retires, parent against this build: the two enqueue the same kernels
              (profiles/vacancy_resource_usage.txt).  Alternated windows behind warm-up steps, the median ms per step, each pair once in
              either order of creation (`step`, `step_here_first`); reported: the windows, the medians, and whether this build's median lies
              inside the parent's own min-max -- no fixed number.
    half      this build: one step of a context with every second row vacant, beside a context that holds the occupied half alone (the same
              positions and missions) and beside the full context; alternated windows, medians.  The expectation is the smaller context's
              step plus the skip of n - m done rows.
    calls     this build: one retire and one admitting respawn naming 1 / 64 / 4096 rows, the wall time around the Python call, and
              sca_get_vacant beside them.

    ring      examples/run_sca.py --scenario circle --agents 4096 --policy orca --no-obstacles --lifelong 20000 as child processes: as it
              was (an arrived drone flies back), with --traffic RATE (an arrived drone leaves, seeded arrivals enter at vacant rows), and
              with --traffic RATE --spawn-margin 0.5; the example's own lines, parsed: missions, arrivals, collisions, the drones that
              left and entered, the population's minimum, maximum and mean over the steps.

workloads: respawn_cost.py's (c3_auto: circle N = 4096 ORCA3D SCA_NBR_AUTO; c4: circle N = 100 000 SCA, device tracker, SCA_NBR_KDTREE)."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from mission_cost import part_bench                                                   # noqa: E402
from respawn_cost import WORKLOADS, make_leg, step_window, summary                    # noqa: E402
from scenes_cost import load_package                                                  # noqa: E402
from spawn_probe_cost import part_step                                                # noqa: E402


def half_leg(S, scenarios, w):
    """the occupied half alone: the even rows of the workload's circle as a context of their own"""
    sc = scenarios.circle(w['n'])
    keep = np.arange(0, len(sc['start']), 2)
    start, goal = np.ascontiguousarray(sc['start'][keep]), np.ascontiguousarray(sc['goal'][keep])
    n = len(keep)
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
    sol.set_agents(np.full(n, 0.5), np.ones(n), goal[:, :3], np.full(n, w['policy'], np.uint8), S.zaxis_flags(start, goal),
                   np.asarray(scenarios.max_run_dist(sc['start'], sc['goal']))[keep])

    def reset():
        sol.set_state(start[:, :3], np.zeros((n, 3), np.float32), start[:, 3:6], np.zeros(n, np.uint8))
        if w['tracked']:
            sol.device_tracker_enable(goal[:, 3:6])
    return dict(sol=sol, reset=reset, mode={'kd': S.NBR_KDTREE, 'auto': S.NBR_AUTO}[w['mode']], n=n)


def part_ring(args):
    import ast
    import re
    import subprocess
    base = [sys.executable, os.path.join(REPO, 'examples', 'run_sca.py'), '--scenario', 'circle', '--agents', '4096', '--policy', 'orca', '--no-obstacles', '--lifelong',
            str(args.ring_steps)]
    legs = {'ping_pong': [], 'traffic': ['--traffic', str(args.traffic)], 'traffic_spawn_margin_0.5': ['--traffic', str(args.traffic), '--spawn-margin', '0.5']}
    out = {'command': ' '.join(['examples/run_sca.py'] + base[2:]), 'traffic_rate_per_step': args.traffic}
    for name, extra in legs.items():
        r = subprocess.run(base + extra, cwd=REPO, capture_output=True, text=True, check=True, env=dict(os.environ, PYTHONPATH=REPO))
        lines = [x for x in r.stdout.splitlines() if x.startswith(('lifelong:', '{', 'spawn margin', 'traffic'))]
        leg = {'lines': lines}
        for x in lines:
            if x.startswith('{'):
                leg.update(ast.literal_eval(x[:x.index('}') + 1]))
                leg['live_fraction'] = float(x.rsplit(' ', 1)[1])
            m = re.match(r'lifelong: (\d+) steps, ([0-9.]+) s, (\d+) missions', x)
            if m:
                leg.update(steps=int(m.group(1)), seconds=float(m.group(2)), missions=int(m.group(3)))
            m = re.match(r'traffic .*: (\d+) drones left, (\d+) entered, population (\d+) \.\. (\d+) \(mean ([0-9.]+)\)', x)
            if m:
                leg.update(left=int(m.group(1)), entered=int(m.group(2)), population_min=int(m.group(3)), population_max=int(m.group(4)), population_mean=float(m.group(5)))
            m = re.match(r'spawn margin .*: (\d+) refusals, (\d+) missions still waiting', x)
            if m:
                leg.update(refusals=int(m.group(1)), waiting=int(m.group(2)))
        out[name] = leg
    return out


def part_half(here, w, args):
    S, scenarios = here
    full, vacant, half = make_leg(S, scenarios, w), make_leg(S, scenarios, w), half_leg(S, scenarios, w)
    odd = np.arange(1, vacant['n'], 2, dtype=np.int32)
    plain = vacant['reset']

    def reset_and_retire():
        if vacant['sol'].population() < vacant['n']:                                   # (sca_set_state is refused while a row is vacant: a new agent set drops vacancy)
            vacant['define']()
        plain()
        vacant['sol'].retire(odd)
    vacant['reset'] = reset_and_retire
    legs = {'full': full, 'half_vacant': vacant, 'occupied_half_alone': half}
    if w['mode'] != 'kd':                                                              # (while a row is vacant the pass is the kd pass: the half alone in that mode too)
        legs['occupied_half_alone_kd'] = dict(half_leg(S, scenarios, w), mode=S.NBR_KDTREE)
        legs['full_kd'] = dict(make_leg(S, scenarios, w), mode=S.NBR_KDTREE)
    for leg in legs.values():
        step_window(leg, args)
    ms = {k: [] for k in legs}
    for _ in range(args.alternations):
        for k, leg in legs.items():
            ms[k].append(step_window(leg, args))
    out = {k: summary(v) for k, v in ms.items()}
    out['n'], out['m'] = vacant['n'], vacant['n'] - len(odd)
    for leg in legs.values():
        leg['sol'].close()
    return out


def part_calls(here, w, args):
    S, scenarios = here
    leg = make_leg(S, scenarios, w)
    sol, sc, n = leg['sol'], leg['sc'], leg['n']
    leg['reset']()
    sol.run_steps(args.warm, leg['mode'])
    sol.synchronize()
    out = {}
    for count in (1, 64, 4096):
        if count >= n:
            continue
        ids = np.arange(0, count, dtype=np.int32) * (n // count)
        ms = {'retire': [], 'admit': [], 'get_vacant': []}
        for _ in range(args.samples):
            t0 = time.perf_counter()
            sol.retire(ids)
            t1 = time.perf_counter()
            sol.vacant()
            t2 = time.perf_counter()
            sol.respawn(ids, sc['start'][ids, :3], np.zeros((count, 3), np.float32), sc['start'][ids, 3:6], 0.5, 1.0, sc['goal'][ids, :3], 1000.0,
                        goal_heading=sc['goal'][ids, 3:6] if w['tracked'] else None)
            t3 = time.perf_counter()
            for k, dt in zip(ms, (t1 - t0, t3 - t2, t2 - t1)):
                ms[k].append(dt * 1e3)
        out[str(count)] = {k: summary(v[1:]) for k, v in ms.items()}                 # (the first sample allocates)
    sol.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=None, help="the parent commit's checkout (built)")
    ap.add_argument('--parts', default='bench,ring,step,half,calls')
    ap.add_argument('--ring-steps', type=int, default=20000)
    ap.add_argument('--traffic', type=float, default=0.3, help='the ring: arrivals per step (the ping-pong ring ends 0.28 missions per step)')
    ap.add_argument('--workloads', default=','.join(WORKLOADS))
    ap.add_argument('--window', type=int, default=200)
    ap.add_argument('--warm', type=int, default=20)
    ap.add_argument('--alternations', type=int, default=5)
    ap.add_argument('--samples', type=int, default=21)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'vacancy_cost.json'))
    args = ap.parse_args()
    parts = args.parts.split(',')
    bench = part_bench(args) if 'bench' in parts and args.root else None             # (in front of everything that opens the GPU here)
    ring = part_ring(args) if 'ring' in parts else None
    here = load_package(REPO, 'sca_here')
    parent = load_package(args.root, 'sca_parent') if args.root else None
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result.update(window_steps=args.window, warm_steps=args.warm, alternations=args.alternations, samples=args.samples)
    if ring:
        result['ring_n_4096_orca3d'] = ring
        for k, v in ring.items():
            if isinstance(v, dict):
                print('ring', k, json.dumps({a: b for a, b in v.items() if a != 'lines'}), flush=True)
    if bench:
        result['bench_py_gpus_1_steps_200_warmup_20_ms_per_step'] = bench
        print('bench', json.dumps(bench), flush=True)

    def save():                                                                       # after every part: a later part that fails loses nothing
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write('\n')
    for name in args.workloads.split(','):
        w = WORKLOADS[name]
        entry = result.setdefault('workloads', {}).setdefault(name, {'desc': w['desc'], 'n': w['n']})
        if 'step' in parts and parent:
            for here_first in (False, True):
                args.here_first = here_first
                key = 'step_here_first' if here_first else 'step'
                entry[key] = part_step(here, parent, w, args)
                print(name, key, json.dumps(entry[key]['here_against_parent']), flush=True)
                save()
        if 'half' in parts:
            entry['half'] = part_half(here, w, args)
            print(name, 'half', json.dumps({k: v['median_ms'] for k, v in entry['half'].items() if isinstance(v, dict)}), flush=True)
            save()
        if 'calls' in parts:
            entry['calls'] = part_calls(here, w, args)
            print(name, 'calls', json.dumps({c: {k: v['median_ms'] for k, v in d.items()} for c, d in entry['calls'].items()}), flush=True)
            save()
    save()


if __name__ == '__main__':
    main()
