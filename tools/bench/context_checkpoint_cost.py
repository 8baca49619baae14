#!/usr/bin/env python
"""What context checkpoints (sca_save_context / sca_load_context) cost.  ONE process; the parent commit's library is loaded beside this
build's (--root: the parent's checkout, built).  Three parts, merged into profiles/context_checkpoint_cost.json:

    step      the step time of a context that NEVER saves, parent against this build: the two enqueue the same kernels
              (profiles/context_checkpoint_resource_usage.txt).  Five alternated windows of 200 steps behind 20 warm-up steps, the median ms
              per step, each pair once in either order of creation (`step`, `step_here_first`); reported: the windows, the medians, and
              whether this build's median lies inside the parent's own min-max -- no fixed number.
    calls     this build: one save_context and one load_context, the wall time around the Python call, 21 samples each, beside one step of
              the same context and beside get_state + get_kd_perm, the parent's partial route; the blob's bytes.
    bench     `bench.py --gpus 1 --steps 200 --warmup 20` as a child process, the parent's checkout and this one alternated twice, in front
              of everything else: the ms_per_step of each run's JSON line.

--vacancy: one more part, into profiles/context_checkpoint_vacancy_cost.json (reported only):

    vacancy   this build: save_context(vacancy=True) and load_context(blob, vacancy=True) with every second row vacant, beside the same
              two calls with no vacant row (the blob is then sca_save_context's; the load is k_ctx_load_vacancy's launch all the same),
              the old calls on that context and one step of each; the wall time around the Python call, 21 samples each.

workloads: respawn_cost.py's (c3_auto: circle N = 4096 ORCA3D SCA_NBR_AUTO; c4: circle N = 100 000 SCA, device tracker, SCA_NBR_KDTREE)"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from mission_cost import part_bench                                                   # noqa: E402
from respawn_cost import WORKLOADS, make_leg, summary                                 # noqa: E402
from scenes_cost import load_package                                            # noqa: E402
from spawn_probe_cost import part_step                                                # noqa: E402


def part_calls(here, w, args):
    leg = make_leg(here[0], here[1], w)
    sol, mode = leg['sol'], leg['mode']
    leg['reset']()
    sol.run_steps(args.warm, mode)
    sol.synchronize()
    ms = {'save_context': [], 'load_context': [], 'one_step': [], 'get_state_and_kd_perm': []}
    blob = sol.save_context()                                                         # (untimed: the page-locked block's allocation)
    sol.load_context(blob)
    for _ in range(args.samples):
        t0 = time.perf_counter()
        blob = sol.save_context()
        t1 = time.perf_counter()
        sol.load_context(blob)
        t2 = time.perf_counter()
        sol.get_state()
        sol.get_kd_perm()
        t3 = time.perf_counter()
        sol.run_steps(1, mode)
        sol.synchronize()
        t4 = time.perf_counter()
        for k, dt in zip(ms, (t1 - t0, t2 - t1, t4 - t3, t3 - t2)):
            ms[k].append(dt * 1e3)
    out = {k: summary(v) for k, v in ms.items()}
    out['blob_bytes'] = int(blob.size)
    sol.close()
    return out


def part_vacancy(here, w, args):
    import numpy as np
    out = {}
    for name, retire in (('no_vacant_row', False), ('every_second_row_vacant', True)):
        leg = make_leg(here[0], here[1], w)
        sol, mode = leg['sol'], leg['mode']
        leg['reset']()
        sol.run_steps(args.warm, mode)
        sol.synchronize()
        if retire:
            sol.retire(np.arange(1, sol.n, 2, dtype=np.int32))
            sol.run_steps(2, mode)
            sol.synchronize()
        ms = {'save_context_vacancy': [], 'load_context_vacancy': [], 'one_step': []}
        if not retire:
            ms.update(save_context=[], load_context=[])
        sol.load_context(sol.save_context(vacancy=True), vacancy=True)              # (untimed: the page-locked block's allocation)
        for _ in range(args.samples):
            t0 = time.perf_counter()
            blob = sol.save_context(vacancy=True)
            t1 = time.perf_counter()
            sol.load_context(blob, vacancy=True)
            t2 = time.perf_counter()
            sol.run_steps(1, mode)
            sol.synchronize()
            t3 = time.perf_counter()
            for k, dt in zip(('save_context_vacancy', 'load_context_vacancy', 'one_step'), (t1 - t0, t2 - t1, t3 - t2)):
                ms[k].append(dt * 1e3)
            if not retire:
                t0 = time.perf_counter()
                old = sol.save_context()
                t1 = time.perf_counter()
                sol.load_context(old)
                t2 = time.perf_counter()
                ms['save_context'].append((t1 - t0) * 1e3)
                ms['load_context'].append((t2 - t1) * 1e3)
        out[name] = {k: summary(v) for k, v in ms.items()}
        out[name].update(blob_bytes=int(blob.size), occupied=int(sol.population()))
        sol.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=None, help="the parent commit's checkout (built)")
    ap.add_argument('--parts', default='bench,step,calls')
    ap.add_argument('--workloads', default=','.join(WORKLOADS))
    ap.add_argument('--window', type=int, default=200)
    ap.add_argument('--warm', type=int, default=20)
    ap.add_argument('--alternations', type=int, default=5)
    ap.add_argument('--samples', type=int, default=21)
    ap.add_argument('--vacancy', action='store_true', help='the vacancy part alone, into profiles/context_checkpoint_vacancy_cost.json')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(REPO, 'profiles', 'context_checkpoint_vacancy_cost.json' if args.vacancy else 'context_checkpoint_cost.json')
    parts = ['vacancy'] if args.vacancy else args.parts.split(',')
    bench = part_bench(args) if 'bench' in parts and args.root else None             # (in front of everything that opens the GPU here)
    here = load_package(REPO, 'sca_here')
    parent = load_package(args.root, 'sca_parent') if args.root else None
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result.update(window_steps=args.window, warm_steps=args.warm, alternations=args.alternations, samples=args.samples)
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
                print(name, key, json.dumps(entry[key]), flush=True)
                save()
        if 'vacancy' in parts:
            entry['vacancy'] = part_vacancy(here, w, args)
            print(name, 'vacancy', json.dumps(entry['vacancy']), flush=True)
            save()
        if 'calls' in parts:
            entry['calls'] = part_calls(here, w, args)
            print(name, 'calls', json.dumps(entry['calls']), flush=True)
            save()
    save()


if __name__ == '__main__':
    main()
