#!/usr/bin/env python
"""What a step costs when the HOST owns the state (INTEGRATION.md stub B, mampenv.py:27-59): the five calls of the portable stub against
sca_step_host on the pinned state block, beside the resident step.  ONE process per configuration, the legs alternated; every window starts
from the scene's start state (bench.py's reset_state, travelled distance and step counters zeroed, tracker re-enabled), runs `--warm` untimed steps and then times the SAME `--window`
steps of the episode in every leg -- the host clock around calls that each end in their own synchronise, step by step.

    python tools/bench/host_step_cost.py --config c2            # c2 | c3 | c4: merges its entry into profiles/host_step_cost.json
    python tools/bench/host_step_cost.py --config c2 --root /path/to/parent/checkout --legs stub_b --record-as stub_b_parent

legs
    stub_b                  sca_set_state -> sca_policy_pass -> sca_get_actions -> sca_env_update -> sca_get_state, as bench.py::host_handover_leg
    block_state_every_step  sca_step_host(SCA_HOST_IN_STATE): the block goes up and comes down every step (the two kernels read and write the
                            page-locked block across the link: the form that ships)
    block_staged            the same on a second context created under SCA_HOST_STEP_STAGED=1: copies into / out of a device staging buffer,
                            the kernels on the copy (the A/B switch)
    block_read_only         sca_step_host(0): the block only comes down
    resident                sca_env_step: nothing crosses but the count

Per leg: the median step time of each of the `--alternations` windows, their min-max (the spread), the windows' means, the bytes that cross
the link per step (the block legs: from sca_host_state_layout) and link_floor_ms = those bytes over the host link's 63 GB/s (PCIe Gen5 x16,
spec) + the resident step: a lower bound, reported as a share, never a target.  Where fewer than half of the agents are still running at the
end of the window the window is shortened until half are; the length used is written."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
LINK_GBS = 63.0
LEGS = ('stub_b', 'block_state_every_step', 'block_staged', 'block_read_only', 'resident')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', required=True, choices=['c2', 'c3', 'c4'])
    ap.add_argument('--window', type=int, default=200)
    ap.add_argument('--warm', type=int, default=20)
    ap.add_argument('--alternations', type=int, default=5)
    ap.add_argument('--legs', default=','.join(LEGS))
    ap.add_argument('--root', default=REPO, help='checkout whose sca_amd and bench.py are measured (default: this one)')
    ap.add_argument('--record-as', default=None, help='with one leg: the name it is stored under (e.g. stub_b_parent)')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'host_step_cost.json'))
    args = ap.parse_args()
    legs = [x for x in args.legs.split(',') if x]
    assert all(x in LEGS for x in legs), legs
    assert args.record_as is None or len(legs) == 1

    sys.path.insert(0, os.path.abspath(args.root))
    bench = importlib.import_module('bench')
    from sca_amd import _lib, solver as S
    assert os.path.abspath(os.path.dirname(bench.__file__)) == os.path.abspath(args.root)

    w = bench.WORKLOADS[args.config]
    scene = bench.build_scene(w, w['n'])
    sc, n = scene['sc'], scene['n']
    tracked = w['policy'] in ('sca', 'mixed')                     # as bench.py's env_api legs: tracked scenes on the kd-tree, the others AUTO
    mode = bench.NBR['kd'] if tracked else bench.NBR['auto']
    sol = bench.make_solver(S, scene, 0)
    sol_staged = None
    if 'block_staged' in legs:
        os.environ['SCA_HOST_STEP_STAGED'] = '1'                  # read by sca_create
        sol_staged = bench.make_solver(S, scene, 0)
        del os.environ['SCA_HOST_STEP_STAGED']

    def reset(sol=sol):
        bench.reset_state(sol, scene)                             # (leaves total_dist and step_num as the previous window left them ...
        st = sol.get_state()                                      # ... and agents then time out earlier from window to window: zero them too)
        sol.set_state(st['pos'], st['vel'], st['heading'], st['flags'], np.zeros(n), np.zeros(n, np.int32))
        if tracked:
            sol.device_tracker_enable(sc['goal'][:, 3:6])
        else:
            sol.device_tracker_disable()

    # ---- how long may the window be?  at least half of the agents still running at its end (resident steps, untimed)
    reset()
    left = [sol.env_step(mode) for _ in range(args.warm + args.window)]
    window = args.window
    while window > 10 and left[args.warm + window - 1] < n / 2:
        window -= 10
    steps_total = args.warm + window

    have_block = 'sca_step_host' in _lib.SIGNATURES
    main_blk = sol.host_state() if have_block and any(x.startswith('block') for x in legs) else None

    def run(leg, sol=sol):
        """one window: (per-step seconds of the timed steps, agents still running at its end)"""
        blk = main_blk
        if leg == 'block_staged':
            sol, blk = sol_staged, sol_staged.host_state()
        reset(sol)
        dts = np.zeros(window)
        if leg == 'stub_b':
            st = sol.get_state()
            for k in range(steps_total):
                t0 = time.perf_counter()
                sol.set_state(st['pos'], st['vel'], st['heading'], st['flags'], st['total_dist'], st['step_num'])
                sol.policy_pass(mode)
                a = sol.actions()                                  # noqa: F841
                sol.env_update(True)
                st = sol.get_state()
                if k >= args.warm:
                    dts[k - args.warm] = time.perf_counter() - t0
            active = int(np.count_nonzero((st['flags'] & 7) == 0))
        elif leg in ('block_state_every_step', 'block_staged', 'block_read_only'):
            every = leg != 'block_read_only'
            if every:                                              # the block is the state the host owns: it starts at the start state too
                blk['pos'][:] = sc['start'][:, :3]
                blk['vel'][:] = 0
                blk['heading'][:] = sc['start'][:, 3:6]
                blk['flags'][:] = 0
                blk['total_dist'][:] = 0
                blk['step_num'][:] = 0
            for k in range(steps_total):
                t0 = time.perf_counter()
                active = sol.step_host(mode, state=every)
                if k >= args.warm:
                    dts[k - args.warm] = time.perf_counter() - t0
        else:
            for k in range(steps_total):
                t0 = time.perf_counter()
                active = sol.env_step(mode)
                if k >= args.warm:
                    dts[k - args.warm] = time.perf_counter() - t0
        return dts, int(active)

    for leg in legs:                                              # code objects, pinned buffers, the allocator: once per leg, untimed
        run(leg)
    rows = {leg: dict(median_ms=[], mean_ms=[], active_at_end=[]) for leg in legs}
    for _ in range(args.alternations):
        for leg in legs:
            dts, active = run(leg)
            assert active == left[steps_total - 1], (leg, active, left[steps_total - 1])   # every leg walked through the same steps
            rows[leg]['median_ms'].append(float(np.median(dts)) * 1e3)
            rows[leg]['mean_ms'].append(float(dts.mean()) * 1e3)
            rows[leg]['active_at_end'].append(active)

    if have_block:
        off = (C.c_int64 * 9)()
        total = C.c_int64(0)
        assert _lib.lib().sca_host_state_layout(n, off, C.byref(total)) == 0
        state_bytes, action_bytes = int(off[6] - off[0]), int(total.value - off[8])
    else:
        state_bytes = action_bytes = None
    count_bytes = 256 * 32 * 4                                    # the active count's pinned read-back (every leg that asks for it)
    traffic = {'stub_b': (n * 73, n * (73 + 28) + count_bytes),
               'block_state_every_step': (state_bytes, None if state_bytes is None else state_bytes + action_bytes + count_bytes),
               'block_staged': (state_bytes, None if state_bytes is None else state_bytes + action_bytes + count_bytes),
               'block_read_only': (0, None if state_bytes is None else state_bytes + action_bytes + count_bytes),
               'resident': (0, count_bytes)}
    for leg in legs:
        r = rows[leg]
        r['ms_per_step'] = float(np.median(r['median_ms']))
        r['spread_ms'] = [min(r['median_ms']), max(r['median_ms'])]
        r['host_to_device_bytes_per_step'], r['device_to_host_bytes_per_step'] = traffic[leg]
    if 'resident' in rows:
        res = rows['resident']['ms_per_step']
        for leg in legs:
            r = rows[leg]
            r['over_resident'] = r['ms_per_step'] / res
            if leg != 'resident' and r['host_to_device_bytes_per_step'] is not None:
                r['link_floor_ms'] = (r['host_to_device_bytes_per_step'] + r['device_to_host_bytes_per_step']) / (LINK_GBS * 1e9) * 1e3 + res
                r['link_floor_share'] = r['link_floor_ms'] / r['ms_per_step']
    entry = {'workload': w['desc'], 'agents': n, 'neighbor_search': 'kd' if tracked else 'auto', 'device_tracker': tracked,
             'warm_steps': args.warm, 'window_steps': window, 'window_steps_asked': args.window, 'alternations': args.alternations,
             'active_after_window_resident_probe': int(left[steps_total - 1]), 'host_link_gb_per_s': LINK_GBS, 'legs': {}}
    if 'stub_b' in rows and 'block_state_every_step' in rows:
        a, b = rows['stub_b'], rows['block_state_every_step']
        margin = (a['spread_ms'][1] - a['spread_ms'][0]) + (b['spread_ms'][1] - b['spread_ms'][0])
        entry['verdict'] = {'stub_b_minus_block_ms': a['ms_per_step'] - b['ms_per_step'], 'sum_of_spreads_ms': margin,
                            'block_below_stub_b_by_more_than_the_spreads': bool(a['ms_per_step'] - b['ms_per_step'] > margin)}

    if 'block_staged' in rows and 'block_state_every_step' in rows:
        a, b = rows['block_staged'], rows['block_state_every_step']
        margin = (a['spread_ms'][1] - a['spread_ms'][0]) + (b['spread_ms'][1] - b['spread_ms'][0])
        entry['staged_vs_direct'] = {'staged_minus_direct_ms': a['ms_per_step'] - b['ms_per_step'], 'sum_of_spreads_ms': margin,
                                     'direct_faster_by_more_than_the_spreads': bool(a['ms_per_step'] - b['ms_per_step'] > margin)}

    try:
        with open(args.out) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {'tool': 'tools/bench/host_step_cost.py', 'unit': 'ms per step; median_ms: the median step time of each window', 'configs': {}}
    cur = doc['configs'].get(args.config)
    if args.record_as and cur:                                    # one leg measured elsewhere (the parent's library), stored beside
        cur['legs'][args.record_as] = rows[legs[0]]
        cur['legs'][args.record_as]['window_steps'] = window
    else:
        entry['legs'] = {(args.record_as or leg): rows[leg] for leg in legs}
        if cur:
            for k, v in cur['legs'].items():
                entry['legs'].setdefault(k, v)
        doc['configs'][args.config] = entry
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    for leg in legs:
        r = rows[leg]
        print('%s %-24s %.4f ms/step  spread %.4f .. %.4f  active at end %s' % (args.config, args.record_as or leg, r['ms_per_step'], r['spread_ms'][0],
                                                                              r['spread_ms'][1], r['active_at_end'][-1]), flush=True)
    for key in ('verdict', 'staged_vs_direct'):
        if key in entry:
            print(args.config, 'window', window, key, json.dumps(entry[key]), flush=True)
    sol.close()
    if sol_staged is not None:
        sol_staged.close()


if __name__ == '__main__':
    main()
