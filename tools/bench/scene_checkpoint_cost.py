#!/usr/bin/env python
"""What scene checkpoints (sca_save_scenes / sca_load_scenes) cost, and that a batch which never calls them steps as it did.  ONE process
on one GPU, the legs alternated, medians with their ranges.

    python tools/bench/scene_checkpoint_cost.py --parent-lib <parent build>/libsca_hip.so     # -> profiles/scene_checkpoint_cost.json

step    `--slots` x `--agents` drones (the six policies in turn, seeded random scenes, the device tracker in the pass: the queue of
        tools/bench/scene_refill_cost.py as one full batch) stepped by sca_run_steps in windows of `--steps` steps, each window from the
        same start state, alternately through the PARENT commit's library (--parent-lib; without it the leg is left out and said so) and
        this build's.  ms per step per window; the claim to check is that this build's median lies inside the spread of the parent's own
        windows.  Neither leg saves or loads.
calls   a batch of `--slots` scenes of `--agents` SCA drones (every drone tracked), `--warm` steps in: ONE sca_save_scenes call naming 1
        and 16 scenes, ONE sca_load_scenes call with those blobs, ONE sca_restart_scenes call naming the same scenes, wall time of each
        (median of `--repeats`), beside the batch's ms per step and the bytes per scene."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sca_amd import _lib, scenarios                                # noqa: E402
from sca_amd import solver as S                                    # noqa: E402


def library(path):
    """another build of the library, with the signatures of the symbols it has"""
    L = C.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    return L


def batch(L, slots, agents, policies):
    """(solver, arrays): `slots` full scenes of `agents` drones in a context of the library L (None: this build's)"""
    eps = []
    for s in range(slots):
        sc = scenarios.random_cube(agents, seed=s)
        eps.append(dict(start=sc['start'], goal=sc['goal'], policy=np.full(agents, policies[s % len(policies)], np.uint8)))
    start, goal = np.concatenate([e['start'] for e in eps]), np.concatenate([e['goal'] for e in eps])
    n = len(start)
    a = dict(pos=start[:, :3].copy(), heading=start[:, 3:6].copy(), vel=np.zeros((n, 3), np.float32), radius=np.full(n, 0.5), pref_speed=np.ones(n),
             goal=goal[:, :3].copy(), policy=np.concatenate([e['policy'] for e in eps]), zaxis=S.zaxis_flags(start, goal),
             max_run_dist=scenarios.max_run_dist(start, goal), goal_heading=goal[:, 3:6].copy(), off=np.arange(slots + 1, dtype=np.int32) * agents)
    keep = _lib._LIB
    if L is not None:
        _lib.lib()
        keep, _lib._LIB = _lib._LIB, L                               # (a solver keeps the library it was made with)
    try:
        sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    finally:
        if L is not None:
            _lib._LIB = keep
    sol.set_agents(a['radius'], a['pref_speed'], a['goal'], a['policy'], a['zaxis'], a['max_run_dist'])
    sol.set_scenes(a['off'])
    sol.device_tracker_enable(a['goal_heading'], in_pass=True)
    return sol, a


def reset(sol, a):
    n = len(a['pos'])
    sol.set_state(a['pos'], a['vel'], a['heading'], np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.int32))
    sol.set_kd_perm(np.arange(n, dtype=np.int32))


def window(sol, a, steps, warm):
    reset(sol, a)
    sol.run_steps(warm, S.NBR_KDTREE)
    sol.synchronize()
    t0 = time.perf_counter()
    sol.run_steps(steps, S.NBR_KDTREE)
    sol.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def spread(x):
    return dict(median=statistics.median(x), min=min(x), max=max(x), all=list(x))


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return spread(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slots', type=int, default=64)
    ap.add_argument('--agents', type=int, default=100)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warm', type=int, default=50)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--repeats', type=int, default=21)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scene_checkpoint_cost.json'))
    args = ap.parse_args()
    rec = dict(tool='tools/bench/scene_checkpoint_cost.py', slots=args.slots, agents_per_scene=args.agents, steps_per_window=args.steps, warm_steps=args.warm,
               policies='SCA, RVO3D, S-RVO3D, ORCA3D, ORCA3D-LP, RVO3D+Dubins in turn; seeded random scenes; device tracker in the pass')
    # ---- the step of a batch that never saves or loads ----
    this, a = batch(None, args.slots, args.agents, [0, 1, 2, 3, 4, 5])
    parent = batch(library(args.parent_lib), args.slots, args.agents, [0, 1, 2, 3, 4, 5])[0] if args.parent_lib else None
    legs = {'this': [], 'parent': []}
    for _ in range(args.windows):
        if parent is not None:
            legs['parent'].append(window(parent, a, args.steps, args.warm))
        legs['this'].append(window(this, a, args.steps, args.warm))
    step = dict(this_ms_per_step=spread(legs['this']))
    if parent is not None:
        same = all(np.array_equal(x, y) for x, y in zip(this.get_state().values(), parent.get_state().values()))
        p = spread(legs['parent'])
        step.update(parent_ms_per_step=p, this_over_parent=step['this_ms_per_step']['median'] / p['median'], final_states_identical=bool(same),
                    this_median_inside_parent_spread=bool(p['min'] <= step['this_ms_per_step']['median'] <= p['max']))
        parent.close()
    else:
        step['parent_ms_per_step'] = 'not measured: no --parent-lib'
    this.close()
    rec['step_without_checkpoints'] = step
    # ---- one save, one load, one restart ----
    sol, a = batch(None, args.slots, args.agents, [0])
    reset(sol, a)
    sol.run_steps(args.warm, S.NBR_KDTREE)
    sol.synchronize()
    calls = {}
    for k in (1, 16):
        ids = np.arange(min(k, args.slots), dtype=np.int32)
        rows = np.concatenate([np.arange(a['off'][s], a['off'][s + 1]) for s in ids])
        blobs = sol.save_scenes(ids)
        bufs = [np.zeros_like(b) for b in blobs]
        calls['scenes_%d' % k] = dict(
            save_ms=timed(lambda: sol._save_into(ids, bufs), args.repeats), load_ms=timed(lambda: sol.load_scenes(ids, blobs), args.repeats),
            restart_ms=timed(lambda: sol.restart_scenes(ids, a['pos'][rows], a['heading'][rows], vel=a['vel'][rows], radius=a['radius'][rows],
                                                        pref_speed=a['pref_speed'][rows], goal=a['goal'][rows], policy=a['policy'][rows], zaxis=a['zaxis'][rows],
                                                        max_run_dist=a['max_run_dist'][rows], goal_heading=a['goal_heading'][rows]), args.repeats),
            bytes_per_scene=int(len(blobs[0])))
        sol.load_scenes(ids, blobs)                                  # (the scenes go on where they were)
    t0 = time.perf_counter()
    sol.run_steps(args.steps, S.NBR_KDTREE)
    sol.synchronize()
    calls['step_ms'] = 1e3 * (time.perf_counter() - t0) / args.steps
    sol.close()
    rec['one_call'] = calls
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(json.dumps(rec, sort_keys=True))


if __name__ == '__main__':
    main()
