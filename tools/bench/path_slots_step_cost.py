#!/usr/bin/env python3
"""What the waypoint lists' slot form (sca_set_path_slots, k_waypoint_slots) costs a step beside the block form (sca_set_paths, k_waypoint),
on the two legs of profiles/paths_cost.json: N = 4096 ORCA3D in SCA_NBR_AUTO (100 steps per call) and N = 100 000 RVO3D on the kd-tree (40).

One context per leg; the two forms alternate on it `--alternations` times.  A window: the lists set in the form (which resets every cursor),
sca_set_state from the start, 5 warm-up steps, then ONE sca_run_steps call, synchronised; the figure is wall time per step.  Medians with the
spread.  0-6 seeded waypoints per agent around its straight line; the slot form's room is W = 6.

    python tools/bench/path_slots_step_cost.py                      # both forms -> the `step` entry of profiles/scene_paths_cost.json
    python tools/bench/path_slots_step_cost.py --forms block --package-root <a built checkout of the parent commit> --out parent_step.json
    python tools/bench/path_slots_step_cost.py --parent-json parent_step.json      # ... and the block form held against the parent's samples
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LEGS = {'orca4096_auto': dict(n=4096, policy=3, mode='NBR_AUTO', steps=100), 'rvo100000_kd': dict(n=100000, policy=1, mode='NBR_KDTREE', steps=40)}
W = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--forms', default='block,slots')
    ap.add_argument('--alternations', type=int, default=5)
    ap.add_argument('--package-root', default=None, help='import sca_amd from this checkout instead of the one the tool stands in')
    ap.add_argument('--parent-json', default=None, help="this tool's --forms block output from the parent commit's library, same machine and session")
    ap.add_argument('--out', default=None, help='default: the `step` entry of profiles/scene_paths_cost.json')
    args = ap.parse_args()
    sys.path.insert(0, args.package_root or REPO)
    from sca_amd import scenarios, solver as S
    forms = args.forms.split(',')
    doc = {'tool': 'tools/bench/path_slots_step_cost.py', 'alternations': args.alternations, 'points_per_agent': W,
           'what': 'wall ms per step of one sca_run_steps call behind 5 warm-up steps, the forms alternated on one context per leg; 0-6 seeded waypoints per agent',
           'per_step_ms': {}}
    for name, leg in LEGS.items():
        n = leg['n']
        sc = scenarios.circle(n)
        start, goal = sc['start'], sc['goal']
        rng = np.random.default_rng(n)
        counts = rng.integers(0, W + 1, n)
        lists = []
        for i in range(n):
            f = np.sort(rng.uniform(0.1, 0.9, counts[i]))[::-1]
            lists.append((start[i, :3] + (goal[i, :3] - start[i, :3]) * f[:, None] + rng.normal(0, 1.0, (counts[i], 3))).tolist())
        sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
        sol.set_agents(np.full(n, 0.5), np.ones(n), goal[:, :3], np.full(n, leg['policy'], np.uint8), S.zaxis_flags(start, goal), scenarios.max_run_dist(start, goal))
        samples = {f: [] for f in forms}
        for _ in range(args.alternations):
            for f in forms:
                if f == 'block':
                    sol.set_paths(lists)
                else:
                    sol.set_path_slots(W, lists)
                sol.set_state(start[:, :3], np.zeros((n, 3), np.float32), start[:, 3:6], np.zeros(n, np.uint8))
                sol.run_steps(5, getattr(S, leg['mode']))
                sol.synchronize()
                t0 = time.perf_counter()
                sol.run_steps(leg['steps'], getattr(S, leg['mode']))
                sol.synchronize()
                samples[f].append((time.perf_counter() - t0) * 1e3 / leg['steps'])
        left = sol.get_path_state()[0]
        sol.close()
        doc['per_step_ms'][name] = {f: {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v)), 'all': v} for f, v in samples.items()}
        doc['per_step_ms'][name]['waypoints_popped_in_the_last_window'] = int(counts.sum() - left.sum())
        print(name, {f: round(float(np.median(v)), 4) for f, v in samples.items()}, flush=True)
    if args.parent_json:
        with open(args.parent_json) as f:
            parent = json.load(f)
        for name in LEGS:
            p, mine = parent['per_step_ms'][name]['block'], doc['per_step_ms'][name]['block']['median']
            doc['per_step_ms'][name]['parent_commit_block'] = p
            doc['per_step_ms'][name]['block_inside_parent_spread'] = bool(p['min'] <= mine <= p['max'])
    if args.out:
        out, whole = args.out, doc
    else:
        out = os.path.join(REPO, 'profiles', 'scene_paths_cost.json')
        whole = {}
        if os.path.exists(out):
            with open(out) as f:
                whole = json.load(f)
        whole['step'] = doc
    with open(out, 'w') as f:
        json.dump(whole, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
