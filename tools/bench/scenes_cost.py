#!/usr/bin/env python
"""What B small episodes cost as ONE batch (sca_set_scenes) against B contexts of one scene each.  ONE process, the legs alternated; every
window starts from the scenes' start states, runs `--warm` untimed steps and then times the SAME `--window` steps in every leg -- the host clock
around sca_env_step, which ends in its own synchronise.

    python tools/bench/scenes_cost.py --root /path/to/parent/checkout              # all workloads, merged into profiles/scenes_cost.json
    python tools/bench/scenes_cost.py --scenes 256 --policy sca --root ...          # one workload (entries are merged per workload)

workloads: B x 100-agent circle scenes, B in --scenes (default 1,16,256,1024), once ORCA3D (untracked) and once SCA with the device tracker
legs
    batch             one context holding the B scenes, one sca_env_step per step
    one_by_one        the same scenes through B contexts of one scene each, by the library of --root (the parent commit's checkout, loaded
                      beside this one): per step the wall time of all B sca_env_step calls.  Left out without --root.
    one_by_one_here   the same with this checkout's library: should equal one_by_one within the spread -- if not, something existing moved
    batch_root        the same batch through the library of --root: what a change to the scene path itself is held against -- `batch` must not
                      be above it by more than the two legs' spreads together (entry `batch_path`).  Left out without --root.
                      --batch-only leaves the one_by_one legs out (B contexts cost minutes at B = 1024).
Per leg: the median step time of each of the `--alternations` windows, their min-max (the spread); per workload: agent-steps/s of the batch and
the ratio one_by_one / batch with the condition "beats it by more than the two spreads together".

    python tools/bench/scenes_cost.py --obstacles --root /path/to/parent/checkout   # per-scene obstacle sets, into profiles/scene_obstacles_cost.json

--obstacles: what one obstacle set per scene (sca_set_scene_obstacles) costs.  B copies of the take-off/landing scene (16 drones, 8 spheres; SCA
with the device tracker), legs
    scene_sets        one batch, every scene with its own copy of the 8 spheres (the obstacle forest, the per-scene-obstacle kernel forms)
    shared_set        the same batch with ONE shared set of the 8 spheres, by the library of --root: the same values (the copies coincide), the same
                      launch count.  Left out without --root.
    shared_set_here   the same with this checkout's library: should equal shared_set within the spread
    batch_root        scene_sets through the library of --root, as above.  Left out without --root.
and the difference scene_sets - shared_set is the feature's cost (expected: two dependent loads per agent).

    python tools/bench/scenes_cost.py --log --scenes 16,256,1024                    # the log per scene, into profiles/scene_log_cost.json

--log: what the trajectory log per scene (sca_scene_history_enable) costs.  The circle workloads above, legs
    log_off           the batch without the log: what the parent commit ran -- held against the `batch` leg of profiles/scenes_cost.json, the
                      parent's figure for the same shapes (entry `log_off_against_parent`: within the two spreads together, or the log-off path moved)
    log_on            the same batch with a log of warm + window rows per scene: one more dispatch per step (k_scene_log), 64 B per live agent
Both legs are this build's; every window starts from sca_set_scenes (new step counters: the log starts at row 0) and the start states.  Beside
them the wall time of reading one scene's whole log back (sca_get_scene_history), next to a step of the same batch.

    python tools/bench/scenes_cost.py --clearance --scenes 16,256,1024 --root /path/to/parent/checkout   # into profiles/scene_clearance_cost.json

--clearance: what the closest approach per agent (sca_scene_clearance_enable) costs.  The circle workloads above, legs
    clearance_off     the batch without the feature: it enqueues what the parent commit enqueued
    clearance_on      the same batch with the feature: one more dispatch per step (k_scene_clearance), O(size^2) rounded norms per live scene
    parent            the same batch through the library of --root in the same process (left out without --root): the off leg has to lie
                      inside the spread of the parent's own windows (entry `off_against_parent`)
All legs alternate window by window; every window starts from sca_set_scenes and the start states.  The on leg is reported as measured."""
import argparse
import importlib
import importlib.util
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SCENE_AGENTS = 100
POLICY = {'orca': 3, 'sca': 0}


def load_package(root, alias):
    """<root>/sca_amd under the module name `alias`: two checkouts' libraries side by side in one process"""
    pkg = os.path.join(os.path.abspath(root), 'sca_amd')
    spec = importlib.util.spec_from_file_location(alias, os.path.join(pkg, '__init__.py'), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[alias] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module(alias + '.solver'), importlib.import_module(alias + '.scenarios')


def make_context(S, scenarios, sc, copies, policy, scenes):
    n1 = len(sc['start'])
    n = n1 * copies
    tile = lambda a: np.tile(a, (copies,) + (1,) * (a.ndim - 1))
    sol = S.BatchedSolver(max_agents=n, max_obstacles=1)
    sol.set_obstacles(np.zeros((0, 3)), np.zeros(0))
    sol.set_agents(np.full(n, 0.5), np.ones(n), tile(sc['goal'][:, :3]), np.full(n, POLICY[policy], np.uint8), tile(S.zaxis_flags(sc['start'], sc['goal'])),
                   tile(scenarios.max_run_dist(sc['start'], sc['goal'])))
    if scenes:
        sol.set_scenes(np.arange(copies + 1, dtype=np.int32) * n1)
    start = tile(sc['start'])

    def reset():
        sol.set_state(start[:, :3], np.zeros((n, 3), np.float32), start[:, 3:6], np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.int32))
        sol.set_kd_perm(np.arange(n, dtype=np.int32))
        if policy == 'sca':
            sol.device_tracker_enable(tile(sc['goal'][:, 3:6]))
    return sol, reset


def make_obstacle_context(S, scenarios, copies, per_scene):
    """`copies` take-off/landing scenes in one batch: per_scene -- every scene its own copy of the 8 spheres, else one shared set"""
    sc = scenarios.takeoff_landing(16)
    n1, m1 = len(sc['start']), len(sc['obs_radius'])
    n = n1 * copies
    tile = lambda a: np.tile(a, (copies,) + (1,) * (a.ndim - 1))
    sol = S.BatchedSolver(max_agents=n, max_obstacles=m1 * copies if per_scene else m1)
    if not per_scene:
        sol.set_obstacles(sc['obs_pos'], sc['obs_radius'])
    sol.set_agents(np.full(n, 0.5), np.ones(n), tile(sc['goal'][:, :3]), np.zeros(n, np.uint8), tile(S.zaxis_flags(sc['start'], sc['goal'])),
                   tile(scenarios.max_run_dist(sc['start'], sc['goal'])))
    sol.set_scenes(np.arange(copies + 1, dtype=np.int32) * n1)
    if per_scene:
        sol.set_scene_obstacles([(sc['obs_pos'], sc['obs_radius'])] * copies)
    start = tile(sc['start'])

    def reset():
        sol.set_state(start[:, :3], np.zeros((n, 3), np.float32), start[:, 3:6], np.zeros(n, np.uint8), np.zeros(n), np.zeros(n, np.int32))
        sol.set_kd_perm(np.arange(n, dtype=np.int32))
        sol.device_tracker_enable(tile(sc['goal'][:, 3:6]))
    return sol, reset, n1


def host():
    """where the numbers were taken: the machine's name and the device's"""
    import platform
    out = {'hostname': platform.node()}
    try:
        import torch
        out['gpu'] = torch.cuda.get_device_name(0)
    except Exception as e:                                        # (the numbers stand without the device's name)
        out['gpu'] = 'unknown (%s)' % type(e).__name__
    return out


def time_legs(legs, args, mode):
    """every leg once untimed, then `--alternations` rounds of all legs in turn; per leg the median step time of every window"""
    steps_total = args.warm + args.window

    def run(leg):
        sols, resets = legs[leg]
        for r in resets:
            r()
        dts = np.zeros(args.window)
        active = 0
        for k in range(steps_total):
            t0 = time.perf_counter()
            active = 0
            for sol in sols:
                active += sol.env_step(mode)
            if k >= args.warm:
                dts[k - args.warm] = time.perf_counter() - t0
        return dts, active

    rows = {leg: dict(median_ms=[], mean_ms=[], active_at_end=[]) for leg in legs}
    for leg in legs:                                              # code objects, pinned buffers, the allocator: once per leg, untimed
        run(leg)
    for _ in range(args.alternations):
        for leg in legs:
            dts, active = run(leg)
            rows[leg]['median_ms'].append(float(np.median(dts)) * 1e3)
            rows[leg]['mean_ms'].append(float(dts.mean()) * 1e3)
            rows[leg]['active_at_end'].append(active)
    assert len({tuple(r['active_at_end']) for r in rows.values()}) == 1, rows      # every leg walked through the same steps
    for r in rows.values():
        r['ms_per_step'] = float(np.median(r['median_ms']))
        r['spread_ms'] = [min(r['median_ms']), max(r['median_ms'])]
    return rows


def batch_path(rows):
    """the scene path of this checkout against the same batch through --root's library: not slower beyond the two spreads together"""
    a, b = rows['batch' if 'batch' in rows else 'scene_sets'], rows['batch_root']
    margin = (a['spread_ms'][1] - a['spread_ms'][0]) + (b['spread_ms'][1] - b['spread_ms'][0])
    return {'here_minus_root_ms': a['ms_per_step'] - b['ms_per_step'], 'here_over_root': a['ms_per_step'] / b['ms_per_step'], 'sum_of_spreads_ms': margin,
            'not_above_root_by_more_than_the_spreads': bool(a['ms_per_step'] - b['ms_per_step'] <= margin)}


def obstacle_workloads(args, S, scenarios, Sp, scp):
    out = args.out if args.out_given else os.path.join(REPO, 'profiles', 'scene_obstacles_cost.json')
    for B in [int(x) for x in args.scenes.split(',') if x]:
        legs = {}
        sol, reset, n1 = make_obstacle_context(S, scenarios, B, True)
        legs['scene_sets'] = ([sol], [reset])
        if Sp is not None:
            sol, reset, _ = make_obstacle_context(Sp, scp, B, True)
            legs['batch_root'] = ([sol], [reset])
            sol, reset, _ = make_obstacle_context(Sp, scp, B, False)
            legs['shared_set'] = ([sol], [reset])
        sol, reset, _ = make_obstacle_context(S, scenarios, B, False)
        legs['shared_set_here'] = ([sol], [reset])
        rows = time_legs(legs, args, S.NBR_KDTREE)
        states = {leg: sols[0].get_state() for leg, (sols, _) in legs.items()}     # the same values: every leg ended on the same state
        for leg, st in states.items():
            for key in st:
                assert np.array_equal(st[key], states['scene_sets'][key]), (leg, key)
        n = B * n1
        ref = 'shared_set' if 'shared_set' in rows else 'shared_set_here'
        a, b = rows['scene_sets'], rows[ref]
        margin = (a['spread_ms'][1] - a['spread_ms'][0]) + (b['spread_ms'][1] - b['spread_ms'][0])
        entry = {'workload': '%d x take-off/landing scene of %d drones and 8 spheres, SCA + device tracker' % (B, n1), 'scenes': B, 'agents': n,
                 'obstacles_per_scene': 8, 'warm_steps': args.warm, 'window_steps': args.window, 'alternations': args.alternations, 'legs': rows,
                 'scene_sets_agent_steps_per_s': n / (a['ms_per_step'] * 1e-3),
                 'cost': {'against': ref, 'scene_sets_minus_shared_set_ms': a['ms_per_step'] - b['ms_per_step'],
                          'ratio_scene_sets_over_shared_set': a['ms_per_step'] / b['ms_per_step'], 'sum_of_spreads_ms': margin,
                          'within_the_spreads': bool(abs(a['ms_per_step'] - b['ms_per_step']) <= margin)}}
        if 'batch_root' in rows:
            entry['batch_path'] = batch_path(rows)
        try:
            with open(out) as f:
                doc = json.load(f)
        except (OSError, ValueError):
            doc = {'tool': 'tools/bench/scenes_cost.py --obstacles', 'unit': 'ms per step of all B scenes; median_ms: the median step time of each window',
                   'workloads': {}}
        doc['host'] = host()
        doc['workloads']['takeoff_x%d' % B] = entry
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write('\n')
        for leg, r in rows.items():
            print('takeoff B=%-5d %-16s %9.4f ms/step  spread %.4f .. %.4f  active at end %s' % (B, leg, r['ms_per_step'], r['spread_ms'][0], r['spread_ms'][1],
                                                                                             r['active_at_end'][-1]), flush=True)
        print('takeoff', B, json.dumps(entry['cost']), json.dumps(entry.get('batch_path')), flush=True)
        for sols, _ in legs.values():
            for sol in sols:
                sol.close()


def log_workloads(args, S, scenarios):
    out = args.out if args.out_given else os.path.join(REPO, 'profiles', 'scene_log_cost.json')
    try:
        with open(os.path.join(REPO, 'profiles', 'scenes_cost.json')) as f:
            parent = json.load(f)['workloads']
    except (OSError, ValueError, KeyError):
        parent = {}
    sc = scenarios.circle(SCENE_AGENTS)
    rows_cap = args.warm + args.window
    for policy in [p for p in args.policy.split(',') if p]:
        for B in [int(x) for x in args.scenes.split(',') if x]:
            legs = {}
            off = np.arange(B + 1, dtype=np.int32) * SCENE_AGENTS
            for leg, on in (('log_off', False), ('log_on', True)):
                sol, reset_state = make_context(S, scenarios, sc, B, policy, True)

                def reset(sol=sol, reset_state=reset_state, on=on):
                    sol.set_scenes(off)                               # new step counters (sca_set_state leaves them alone); frees the log
                    if on:
                        sol.scene_history_enable(rows_cap)
                    reset_state()
                legs[leg] = ([sol], [reset])
            rows = time_legs(legs, args, S.NBR_KDTREE)
            states = {leg: sols[0].get_state() for leg, (sols, _) in legs.items()}     # the log changes no value
            for key in states['log_off']:
                assert np.array_equal(states['log_on'][key], states['log_off'][key]), key
            on_sol = legs['log_on'][0][0]
            logged = on_sol.scene_history_rows()
            assert not logged['dropped'].any()
            # one scene's whole log back to the host, beside a step of this batch
            reads = []
            for _ in range(20):
                t0 = time.perf_counter()
                h = on_sol.scene_history(B // 2)
                reads.append(time.perf_counter() - t0)
            a, b = rows['log_on'], rows['log_off']
            margin = (a['spread_ms'][1] - a['spread_ms'][0]) + (b['spread_ms'][1] - b['spread_ms'][0])
            n = B * SCENE_AGENTS
            entry = {'workload': '%d x circle of %d, %s' % (B, SCENE_AGENTS, 'SCA + device tracker' if policy == 'sca' else 'ORCA3D'),
                     'scenes': B, 'agents': n, 'warm_steps': args.warm, 'window_steps': args.window, 'alternations': args.alternations, 'legs': rows,
                     'log_rows_per_scene': rows_cap, 'log_bytes': 64 * rows_cap * n,
                     'cost': {'log_on_minus_log_off_us': 1e3 * (a['ms_per_step'] - b['ms_per_step']), 'ratio_log_on_over_log_off': a['ms_per_step'] / b['ms_per_step'],
                              'sum_of_spreads_us': 1e3 * margin, 'within_the_spreads': bool(abs(a['ms_per_step'] - b['ms_per_step']) <= margin),
                              'bytes_per_step': 64 * n},
                     'readback_one_scene': {'rows': int(h['pos'].shape[0]), 'agents': int(h['pos'].shape[1]), 'bytes': 64 * int(h['pos'].shape[0]) * int(h['pos'].shape[1]),
                                            'median_ms': float(np.median(reads)) * 1e3, 'min_ms': float(min(reads)) * 1e3,
                                            'note': 'sca_scene_history_rows + sca_get_scene_history + the unpack into three numpy arrays'}}
            p = parent.get('%s_x%d' % (policy, B), {}).get('legs', {}).get('batch')
            if p is not None:
                m2 = (p['spread_ms'][1] - p['spread_ms'][0]) + (b['spread_ms'][1] - b['spread_ms'][0])
                entry['log_off_against_parent'] = {'parent_batch_ms': p['ms_per_step'], 'parent_spread_ms': p['spread_ms'], 'log_off_minus_parent_ms': b['ms_per_step'] - p['ms_per_step'],
                                                   'sum_of_spreads_ms': m2, 'within_the_spreads': bool(abs(b['ms_per_step'] - p['ms_per_step']) <= m2)}
            try:
                with open(out) as f:
                    doc = json.load(f)
            except (OSError, ValueError):
                doc = {'tool': 'tools/bench/scenes_cost.py --log', 'unit': 'ms per step of all B scenes; median_ms: the median step time of each window', 'workloads': {}}
            doc['host'] = host()
            doc['workloads']['%s_x%d' % (policy, B)] = entry
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, 'w') as f:
                json.dump(doc, f, indent=1, sort_keys=True)
                f.write('\n')
            for leg, r in rows.items():
                print('%-5s B=%-5d %-16s %9.4f ms/step  spread %.4f .. %.4f  active at end %s' % (policy, B, leg, r['ms_per_step'], r['spread_ms'][0],
                                                                                                r['spread_ms'][1], r['active_at_end'][-1]), flush=True)
            print(policy, B, json.dumps(entry['cost']), json.dumps(entry['readback_one_scene']), json.dumps(entry.get('log_off_against_parent')), flush=True)
            for sols, _ in legs.values():
                for sol in sols:
                    sol.close()


def clearance_workloads(args, S, scenarios, Sp, scp):
    out = args.out if args.out_given else os.path.join(REPO, 'profiles', 'scene_clearance_cost.json')
    sc = scenarios.circle(SCENE_AGENTS)
    for policy in [p for p in args.policy.split(',') if p]:
        for B in [int(x) for x in args.scenes.split(',') if x]:
            legs = {}
            off = np.arange(B + 1, dtype=np.int32) * SCENE_AGENTS
            for leg, mod, scn, on in (('clearance_off', S, scenarios, False), ('clearance_on', S, scenarios, True), ('parent', Sp, scp, False)):
                if mod is None:
                    continue
                sol, reset_state = make_context(mod, scn, sc, B, policy, True)

                def reset(sol=sol, reset_state=reset_state, on=on):
                    sol.set_scenes(off)                               # new step counters; drops the records
                    reset_state()
                    if on:
                        sol.scene_clearance_enable()
                legs[leg] = ([sol], [reset])
            rows = time_legs(legs, args, S.NBR_KDTREE)
            states = {leg: sols[0].get_state() for leg, (sols, _) in legs.items()}     # the feature changes no value
            for leg in states:
                for key in states['clearance_off']:
                    assert np.array_equal(states[leg][key], states['clearance_off'][key]), (leg, key)
            rec = legs['clearance_on'][0][0].scene_clearance(B // 2)
            a, b = rows['clearance_on'], rows['clearance_off']
            margin = (a['spread_ms'][1] - a['spread_ms'][0]) + (b['spread_ms'][1] - b['spread_ms'][0])
            n = B * SCENE_AGENTS
            entry = {'workload': '%d x circle of %d, %s' % (B, SCENE_AGENTS, 'SCA + device tracker' if policy == 'sca' else 'ORCA3D'),
                     'scenes': B, 'agents': n, 'warm_steps': args.warm, 'window_steps': args.window, 'alternations': args.alternations, 'legs': rows,
                     'pair_norms_per_step_at_most': B * SCENE_AGENTS * (SCENE_AGENTS - 1),
                     'min_clearance_of_the_middle_scene': float(rec['agent_clear'].min()),
                     'cost': {'on_minus_off_us': 1e3 * (a['ms_per_step'] - b['ms_per_step']), 'ratio_on_over_off': a['ms_per_step'] / b['ms_per_step'],
                              'sum_of_spreads_us': 1e3 * margin, 'within_the_spreads': bool(abs(a['ms_per_step'] - b['ms_per_step']) <= margin)}}
            if 'parent' in rows:
                p = rows['parent']
                entry['off_against_parent'] = {'off_minus_parent_us': 1e3 * (b['ms_per_step'] - p['ms_per_step']), 'parent_spread_ms': p['spread_ms'],
                                               'off_inside_the_parents_spread': bool(p['spread_ms'][0] <= b['ms_per_step'] <= p['spread_ms'][1]),
                                               'off_not_above_the_parents_spread': bool(b['ms_per_step'] <= p['spread_ms'][1])}
            try:
                with open(out) as f:
                    doc = json.load(f)
            except (OSError, ValueError):
                doc = {'tool': 'tools/bench/scenes_cost.py --clearance', 'unit': 'ms per step of all B scenes; median_ms: the median step time of each window', 'workloads': {}}
            doc['host'] = host()
            doc['workloads']['%s_x%d' % (policy, B)] = entry
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, 'w') as f:
                json.dump(doc, f, indent=1, sort_keys=True)
                f.write('\n')
            for leg, r in rows.items():
                print('%-5s B=%-5d %-16s %9.4f ms/step  spread %.4f .. %.4f  active at end %s' % (policy, B, leg, r['ms_per_step'], r['spread_ms'][0],
                                                                                                r['spread_ms'][1], r['active_at_end'][-1]), flush=True)
            print(policy, B, json.dumps(entry['cost']), json.dumps(entry.get('off_against_parent')), flush=True)
            for sols, _ in legs.values():
                for sol in sols:
                    sol.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', default='1,16,256,1024')
    ap.add_argument('--policy', default='orca,sca')
    ap.add_argument('--window', type=int, default=200)
    ap.add_argument('--warm', type=int, default=5)
    ap.add_argument('--alternations', type=int, default=5)
    ap.add_argument('--root', default=None, help="the parent commit's checkout (built): the one_by_one leg runs its library")
    ap.add_argument('--out', default=None, help='default: profiles/scenes_cost.json (profiles/scene_obstacles_cost.json with --obstacles)')
    ap.add_argument('--batch-only', action='store_true', help='without the one_by_one legs: the batch against batch_root alone (needs --root)')
    ap.add_argument('--obstacles', action='store_true', help='the per-scene obstacle sets against one shared set, instead of the batch against B contexts')
    ap.add_argument('--log', action='store_true', help='the trajectory log per scene off and on in this build, into profiles/scene_log_cost.json')
    ap.add_argument('--clearance', action='store_true', help='the closest approach per agent off and on in this build, beside the library of --root, '
                                                             'into profiles/scene_clearance_cost.json')
    args = ap.parse_args()
    args.out_given = args.out is not None
    if not args.out_given:
        args.out = os.path.join(REPO, 'profiles', 'scenes_cost.json')

    sys.path.insert(0, REPO)
    from sca_amd import scenarios, solver as S
    Sp = scp = None
    assert args.root or not args.batch_only, '--batch-only compares with the library of --root'
    if args.root:
        assert os.path.abspath(args.root) != REPO
        Sp, scp = load_package(args.root, 'sca_amd_parent')
        assert Sp._lib._build.LIB != S._lib._build.LIB
    if args.obstacles:
        return obstacle_workloads(args, S, scenarios, Sp, scp)
    if args.log:
        return log_workloads(args, S, scenarios)
    if args.clearance:
        return clearance_workloads(args, S, scenarios, Sp, scp)
    KD = S.NBR_KDTREE
    sc = scenarios.circle(SCENE_AGENTS)

    for policy in [p for p in args.policy.split(',') if p]:
        for B in [int(x) for x in args.scenes.split(',') if x]:
            legs = {}
            batch, batch_reset = make_context(S, scenarios, sc, B, policy, True)
            legs['batch'] = ([batch], [batch_reset])
            if Sp is not None:
                sol, reset = make_context(Sp, scp, sc, B, policy, True)
                legs['batch_root'] = ([sol], [reset])
            if Sp is not None and not args.batch_only:
                made = [make_context(Sp, scp, sc, 1, policy, False) for _ in range(B)]
                legs['one_by_one'] = ([m[0] for m in made], [m[1] for m in made])
            if not args.batch_only:
                made = [make_context(S, scenarios, sc, 1, policy, False) for _ in range(B)]
                legs['one_by_one_here'] = ([m[0] for m in made], [m[1] for m in made])

            rows = time_legs(legs, args, KD)
            n = B * SCENE_AGENTS
            entry = {'workload': '%d x circle of %d, %s' % (B, SCENE_AGENTS, 'SCA + device tracker' if policy == 'sca' else 'ORCA3D'),
                     'scenes': B, 'agents': n, 'warm_steps': args.warm, 'window_steps': args.window, 'alternations': args.alternations, 'legs': rows,
                     'batch_agent_steps_per_s': n / (rows['batch']['ms_per_step'] * 1e-3)}
            if 'batch_root' in rows:
                entry['batch_path'] = batch_path(rows)
            if not args.batch_only:
                ref = 'one_by_one' if 'one_by_one' in rows else 'one_by_one_here'
                a, b = rows[ref], rows['batch']
                margin = (a['spread_ms'][1] - a['spread_ms'][0]) + (b['spread_ms'][1] - b['spread_ms'][0])
                entry['verdict'] = {'against': ref, 'ratio_one_by_one_over_batch': a['ms_per_step'] / b['ms_per_step'],
                                    'one_by_one_minus_batch_ms': a['ms_per_step'] - b['ms_per_step'], 'sum_of_spreads_ms': margin,
                                    'batch_faster_by_more_than_the_spreads': bool(a['ms_per_step'] - b['ms_per_step'] > margin),
                                    'batch_within_the_spreads': bool(abs(a['ms_per_step'] - b['ms_per_step']) <= margin)}
                if 'one_by_one' in rows:
                    h = rows['one_by_one_here']
                    m2 = (a['spread_ms'][1] - a['spread_ms'][0]) + (h['spread_ms'][1] - h['spread_ms'][0])
                    entry['existing_path'] = {'here_minus_parent_ms': h['ms_per_step'] - a['ms_per_step'], 'sum_of_spreads_ms': m2,
                                              'within_the_spreads': bool(abs(h['ms_per_step'] - a['ms_per_step']) <= m2)}
            try:
                with open(args.out) as f:
                    doc = json.load(f)
            except (OSError, ValueError):
                doc = {'tool': 'tools/bench/scenes_cost.py', 'unit': 'ms per step of all B scenes; median_ms: the median step time of each window', 'workloads': {}}
            doc['workloads']['%s_x%d' % (policy, B)] = entry
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                json.dump(doc, f, indent=1, sort_keys=True)
                f.write('\n')
            for leg, r in rows.items():
                print('%-5s B=%-5d %-16s %9.4f ms/step  spread %.4f .. %.4f  active at end %s' % (policy, B, leg, r['ms_per_step'], r['spread_ms'][0],
                                                                                                r['spread_ms'][1], r['active_at_end'][-1]), flush=True)
            print(policy, B, 'agent-steps/s %.3g' % entry['batch_agent_steps_per_s'], json.dumps(entry.get('verdict')), json.dumps(entry.get('existing_path')),
                  json.dumps(entry.get('batch_path')), flush=True)
            for sols, _ in legs.values():
                for sol in sols:
                    sol.close()


if __name__ == '__main__':
    main()
