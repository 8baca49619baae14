#!/usr/bin/env python
"""What a respawn that brings policy and attributes (sca_respawn_agents_attrs) costs.  tools/bench/respawn_cost.py's method: ONE process,
the parent commit's library loaded beside this build's (--root: the parent's checkout, built), alternated windows, medians.  Two parts,
merged into profiles/respawn_attrs_cost.json:

    step      the step time of a context that NEVER calls the new entry points, parent against this build (the two enqueue the same
              kernels; windows of `--window` steps behind `--warm` warm-up steps, alternated), each pair once in either order of
              creation: `parent_first` and `here_first`.
    call      one call naming 1 / 64 / 4096 rows (wall time around the Python call, `--samples` samples, a step between the calls) in three
              cases -- both arguments None (sca_respawn_agents through the new symbol's front door), a policy only, a policy and all seven
              solver attribute arrays -- beside sca_respawn_agents naming the same rows in both builds, and beside the only other route:
              sca_set_agents + sca_set_agent_params + sca_set_state (+ the tracker's enable call).

workloads: respawn_cost's c3_auto (circle N = 4096, ORCA3D, SCA_NBR_AUTO) and c4 (circle N = 100 000, SCA, device tracker, kd)."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from respawn_cost import WORKLOADS, make_leg, step_window, summary                      # noqa: E402
from scenes_cost import host, load_package                                            # noqa: E402

ATTRS = dict(neighbor_dist=8.0, max_neighbors=12, time_step=0.1, time_horizon=8.0, max_speed=1.0, max_heading_change=0.7, dt_nominal=0.1)


def part_step(here, parent, w, args):
    out = {}
    for order in ('parent_first', 'here_first'):
        legs = {}
        for who in (('parent', 'here') if order == 'parent_first' else ('here', 'parent')):
            pkg = parent if who == 'parent' else here
            if pkg:
                legs[who] = make_leg(pkg[0], pkg[1], w)
        for leg in legs.values():
            step_window(leg, args)                                                    # every leg once untimed
        ms = {k: [] for k in legs}
        for _ in range(args.alternations):
            for k, leg in legs.items():
                ms[k].append(step_window(leg, args))
        res = {k: summary(v) for k, v in ms.items()}
        if parent:
            p, h = res['parent'], res['here']
            res['here_against_parent'] = {'difference_ms': round(h['median_ms'] - p['median_ms'], 5), 'parent_min_ms': p['min_ms'], 'parent_max_ms': p['max_ms'],
                                          'inside_parent_spread': bool(p['min_ms'] <= h['median_ms'] <= p['max_ms'])}
        for leg in legs.values():
            leg['sol'].close()
        out[order] = res
    return out


def timed_calls(leg, w, args, count, **brings):
    sol, n, sc = leg['sol'], leg['n'], leg['sc']
    rng = np.random.default_rng(count)
    ms = []
    for s in range(args.samples + 1):
        ids = np.sort(rng.choice(n, count, replace=False)).astype(np.int32)
        a = (ids, sc['start'][ids, :3], np.zeros((count, 3), np.float32), sc['start'][ids, 3:6], np.full(count, 0.5), np.ones(count), sc['goal'][ids, :3],
             np.full(count, 1e6))
        kw = {k: (np.full(count, v, np.uint8) if k == 'policy' else {q: np.full(count, x) for q, x in v.items()}) for k, v in brings.items()}
        t0 = time.perf_counter()
        sol.respawn(*a, goal_heading=sc['goal'][ids, 3:6] if w['tracked'] else None, **kw)
        if s:                                                                         # (the first call allocates the blocks and, with attributes, the per-agent arrays)
            ms.append((time.perf_counter() - t0) * 1e3)
        sol.run_steps(1, leg['mode'])                                                 # a step between the calls, as a lifelong loop has
        sol.synchronize()
    return summary(ms)


def part_call(here, parent, w, args):
    out = {}
    cases = {'plain': {}, 'policy_only': dict(policy=w['policy']), 'policy_and_attributes': dict(policy=w['policy'], attrs=ATTRS)}
    for who, pkg in (('parent', parent), ('here', here)):
        if not pkg:
            continue
        for case, brings in cases.items():
            if who == 'parent' and brings:
                continue                                                              # (the parent has sca_respawn_agents alone)
            leg = make_leg(pkg[0], pkg[1], w)
            leg['reset']()
            leg['sol'].run_steps(args.warm, leg['mode'])
            leg['sol'].synchronize()
            out[who + '_' + case] = {str(count): timed_calls(leg, w, args, count, **brings) for count in (1, 64, 4096)}
            leg['sol'].close()
    # the only other route to another policy or attribute: the whole definition and state again
    leg = make_leg(here[0], here[1], w)
    leg['reset']()
    ms = []
    for _ in range(max(3, args.samples // 6)):
        t0 = time.perf_counter()
        leg['define']()
        leg['sol'].set_agent_params(**{k: np.full(leg['n'], v) for k, v in ATTRS.items()})
        leg['reset']()
        ms.append((time.perf_counter() - t0) * 1e3)
    out['set_agents_route'] = summary(ms)
    leg['sol'].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=None, help="the parent commit's checkout (built)")
    ap.add_argument('--parts', default='step,call')
    ap.add_argument('--workloads', default=','.join(WORKLOADS))
    ap.add_argument('--window', type=int, default=200)
    ap.add_argument('--warm', type=int, default=20)
    ap.add_argument('--alternations', type=int, default=5)
    ap.add_argument('--samples', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'respawn_attrs_cost.json'))
    args = ap.parse_args()
    here = load_package(REPO, 'sca_here')
    parent = load_package(args.root, 'sca_parent') if args.root else None
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result.update(host=host(), window_steps=args.window, warm_steps=args.warm, alternations=args.alternations, samples=args.samples)

    def save():                                                                       # after every part: a later part that fails loses nothing
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write('\n')
    for name in args.workloads.split(','):
        w = WORKLOADS[name]
        entry = result.setdefault('workloads', {}).setdefault(name, {'desc': w['desc'], 'n': w['n']})
        for part, fn in (('step', part_step), ('call', part_call)):
            if part in args.parts.split(','):
                entry[part] = fn(here, parent, w, args)
                print(name, part, json.dumps(entry[part]), flush=True)
                save()


if __name__ == '__main__':
    main()
