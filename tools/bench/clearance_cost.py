#!/usr/bin/env python
"""What the closest approach per agent of a whole context (sca_clearance_enable, k_clearance) costs per step.  ONE process, the legs
alternated window by window; every window starts from the workload's start state, runs `--warm` untimed steps and then times ONE burst of
`--window` steps (sca_run_steps + a synchronise, the host clock around both).

    python tools/bench/clearance_cost.py --root /path/to/parent/checkout      # all workloads, merged into profiles/clearance_cost.json
    python tools/bench/clearance_cost.py --workloads c3_auto                   # one workload (entries are merged per workload)

workloads
    c3_auto     circle, N = 4096, ORCA3D, SCA_NBR_AUTO
    c5          take-off / landing, N = 16 384, SCA on even ids / S-RVO3D on odd ids, the device tracker, SCA_NBR_KDTREE
    c4          circle, N = 100 000, SCA, the device tracker, SCA_NBR_KDTREE
legs
    parent      the library of --root (the parent commit's checkout, loaded beside this one); left out without --root
    off         this build without the feature: it enqueues what the parent enqueued -- `off_against_parent`: its median inside the min-max of
                the parent's own windows, or not; the windows are reported either way
    on          this build with the feature, enabled behind the warm-up steps: `first_step_ms` is the first step after enabling (every record
                at +inf: a full nearest search), `windows_ms` the steady state.  Recorded as measured.
Per leg: ms per step of each of the `--alternations` windows, their median and min-max."""
import argparse
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
    'c3_auto': dict(kind='circle', n=4096, policy='orca', mode='auto', tracked=False, desc='circle N=4096, ORCA3D, SCA_NBR_AUTO'),
    'c5': dict(kind='takeoff', n=16384, policy='mixed', mode='kd', tracked=True, desc='take-off/landing N=16384, SCA even ids / S-RVO3D odd ids, device tracker, SCA_NBR_KDTREE'),
    'c4': dict(kind='circle', n=100000, policy='sca', mode='kd', tracked=True, desc='circle N=100000, SCA, device tracker, SCA_NBR_KDTREE'),
}
POLICY = {'sca': 0, 'orca': 3}


def make_leg(S, scenarios, w):
    sc = scenarios.circle(w['n']) if w['kind'] == 'circle' else scenarios.takeoff_landing(w['n'])
    n = len(sc['start'])
    policy = np.where(np.arange(n) % 2 == 0, 0, 2).astype(np.uint8) if w['policy'] == 'mixed' else np.full(n, POLICY[w['policy']], np.uint8)
    sol = S.BatchedSolver(max_agents=n, max_obstacles=max(1, len(sc['obs_radius'])))
    sol.set_obstacles(sc['obs_pos'], sc['obs_radius'])
    sol.set_agents(np.full(n, 0.5), np.ones(n), sc['goal'][:, :3], policy, S.zaxis_flags(sc['start'], sc['goal']), scenarios.max_run_dist(sc['start'], sc['goal']))
    mode = {'kd': S.NBR_KDTREE, 'auto': S.NBR_AUTO}[w['mode']]

    def reset():
        sol.set_state(sc['start'][:, :3], np.zeros((n, 3), np.float32), sc['start'][:, 3:6], np.zeros(n, np.uint8))
        if w['tracked']:
            sol.device_tracker_enable(sc['goal'][:, 3:6])
    return sol, reset, mode, n


def window(sol, reset, mode, args, feature):
    """ms per step of one window; with the feature also the first step after enabling"""
    reset()
    if feature:
        sol.clearance_enable(False)                                                   # (the window before left it on; off is a no-op the first time)
    sol.run_steps(args.warm, mode)
    sol.synchronize()
    first = None
    if feature:
        sol.clearance_enable()
        t0 = time.perf_counter()
        sol.run_steps(1, mode)
        sol.synchronize()
        first = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    sol.run_steps(args.window, mode)
    sol.synchronize()
    return (time.perf_counter() - t0) * 1e3 / args.window, first


def summary(ms):
    return {'windows_ms': [round(x, 5) for x in ms], 'median_ms': round(float(np.median(ms)), 5), 'min_ms': round(min(ms), 5), 'max_ms': round(max(ms), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=None, help="the parent commit's checkout (built): the `parent` leg")
    ap.add_argument('--workloads', default=','.join(WORKLOADS))
    ap.add_argument('--window', type=int, default=200)
    ap.add_argument('--warm', type=int, default=20)
    ap.add_argument('--alternations', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'clearance_cost.json'))
    args = ap.parse_args()
    here = load_package(REPO, 'sca_here')
    parent = load_package(args.root, 'sca_parent') if args.root else None
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result.update(host=host(), window_steps=args.window, warm_steps=args.warm, alternations=args.alternations,
                  method='one process, legs alternated window by window; a window = start state, warm-up steps, one timed sca_run_steps burst + synchronise')
    result.setdefault('workloads', {})
    for name in args.workloads.split(','):
        w = WORKLOADS[name]
        legs = {}
        if parent:
            legs['parent'] = make_leg(parent[0], parent[1], w) + (False,)
        legs['off'] = make_leg(here[0], here[1], w) + (False,)
        legs['on'] = make_leg(here[0], here[1], w) + (True,)
        for sol, reset, mode, _, feature in legs.values():                             # every leg once untimed
            window(sol, reset, mode, args, feature)
        ms = {k: [] for k in legs}
        first = []
        for _ in range(args.alternations):
            for k, (sol, reset, mode, _, feature) in legs.items():
                per_step, f = window(sol, reset, mode, args, feature)
                ms[k].append(per_step)
                if f is not None:
                    first.append(f)
        entry = {'desc': w['desc'], 'n': legs['off'][3], 'legs': {k: summary(v) for k, v in ms.items()}}
        entry['legs']['on']['first_step_ms'] = [round(x, 5) for x in first]
        entry['legs']['on']['first_step_median_ms'] = round(float(np.median(first)), 5)
        off, on = entry['legs']['off'], entry['legs']['on']
        entry['on_minus_off_ms'] = round(on['median_ms'] - off['median_ms'], 5)
        entry['on_over_off'] = round(on['median_ms'] / off['median_ms'], 4)
        if parent:
            p = entry['legs']['parent']
            entry['off_against_parent'] = {'off_median_ms': off['median_ms'], 'parent_min_ms': p['min_ms'], 'parent_max_ms': p['max_ms'],
                                           'inside_parent_spread': bool(p['min_ms'] <= off['median_ms'] <= p['max_ms'])}
        result['workloads'][name] = entry
        print(name, json.dumps(entry))
        for sol, *_ in legs.values():
            sol.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
