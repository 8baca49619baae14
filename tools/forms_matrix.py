"""Which kernel forms the library picks by itself (no forcing switch) over a fixed, seeded matrix of scenes: the five BASELINE configs and
shard sizes on both sides of every threshold of sca_amd/csrc/sca_forms.h, with the kd-tree, the grid and SCA_NBR_AUTO, with the tracker in
the pass and without.  Every row is stepped STEPS times from its start state with a device-wide synchronise after every step -- so the
asynchronous count readbacks have landed before the next pass decides -- and sca_last_pass_forms is recorded per step.

  python tools/forms_matrix.py --out forms.json [--label TEXT]       (needs a GPU)
  python tools/forms_matrix.py --compare parent_a.json parent_b.json new.json [--out merged.json]

--compare: rows on which the first two files (two runs of one library) disagree are unstable by construction and are listed and left
out (more than one row in twenty: the tool is missing a synchronise, exit 2); every other row of the third file must equal the first's
(exit 1 otherwise).  Two libraries are compared by running the tool from two trees: the library is the one of the tree it runs in.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = 12
MODES = {'kd': 0, 'grid': 1, 'auto': 3}
POL = {'sca': 0, 'srvo': 2, 'orca': 3, 'orcalp': 4}


def matrix():
    """(name, scene kind, agents, policy, tracker in the pass, neighbour mode)"""
    rows = []
    for name, kind, n, pol in (('c1', 'circle10', 8, 'sca'), ('c2', 'circle', 1024, 'sca'), ('c3', 'random', 4096, 'orca'),
                               ('c4', 'circle', 100000, 'sca'), ('c5', 'takeoff', 16384, 'mixed')):
        for mode in MODES:
            for trk in ((False, True) if pol != 'orca' else (False,)):
                rows.append((name, kind, n, pol, trk, mode))
    # group fuse 1024 | k_solve_fb 2048 | k_kd_top 4096 | packed K1 6144 | k_action_fb 16 384: both sides, tracker in the pass and not
    for n in (1024, 1025, 2048, 2049, 4096, 4097, 6143, 6144, 16384, 16385):
        for trk in (False, True):
            rows.append(('size', 'circle', n, 'sca', trk, 'kd'))
        rows.append(('size', 'circle', n, 'orca', False, 'auto'))
    for n in (2048, 2049, 16384, 16385):
        rows.append(('size', 'circle', n, 'sca', True, 'grid'))
    # the re-plan forms' ranges (nearly every agent of the circle re-plans per step) and the two-launch solve: 32 768 | 61 440 | 65 536 | 114 688
    for n in (8192, 8193, 32768, 32769, 61440, 61441, 65536, 65537, 114688, 114689):
        rows.append(('size', 'circle', n, 'sca', True, 'kd'))
    # the LP lane form from 16 384 LP agents
    for n in (16383, 16384):
        for mode in ('kd', 'auto'):
            rows.append(('size', 'circle', n, 'orcalp', False, mode))
    return rows


_scenes = {}


def scene(kind, n):
    from sca_amd import scenarios
    if (kind, n) not in _scenes:
        _scenes.clear()                                                  # (rows of one scene follow each other: keep one)
        _scenes[(kind, n)] = (scenarios.circle(n, rad=10.0) if kind == 'circle10' else scenarios.circle(n) if kind == 'circle'
                              else scenarios.random_cube(n, seed=0) if kind == 'random' else scenarios.takeoff_landing(n))
    return _scenes[(kind, n)]


def run_row(S, torch, kind, n, pol, trk, mode):
    from sca_amd import scenarios
    sc = scene(kind, n)
    n = len(sc['start'])
    policy = np.where(np.arange(n) % 2 == 0, POL['sca'], POL['srvo']).astype(np.uint8) if pol == 'mixed' else np.full(n, POL[pol], np.uint8)
    sol = S.BatchedSolver(max_agents=n, max_obstacles=max(1, len(sc['obs_radius'])))
    try:
        sol.set_obstacles(sc['obs_pos'], sc['obs_radius'])
        sol.set_agents(np.full(n, 0.5), np.ones(n), sc['goal'][:, :3], policy, S.zaxis_flags(sc['start'], sc['goal']),
                       scenarios.max_run_dist(sc['start'], sc['goal']))
        sol.set_state(sc['start'][:, :3], np.zeros((n, 3), np.float32), sc['start'][:, 3:6], np.zeros(n, np.uint8))
        if trk:
            sol.device_tracker_enable(sc['goal'][:, 3:6])
        forms = []
        for _ in range(STEPS):
            sol.run_steps(1, MODES[mode])
            sol.synchronize()
            torch.cuda.synchronize()                                     # every stream of the device: the side streams' count copies too
            forms.append(int(sol.pass_forms()))
        return forms
    finally:
        sol.close()


def run(out, label):
    import torch
    from sca_amd import solver as S
    for k in list(os.environ):
        if k.startswith('SCA_') and k != 'SCA_QUIET':
            del os.environ[k]                                            # unforced
    rows = {}
    for name, kind, n, pol, trk, mode in matrix():
        key = '%s %s n=%d %s %s %s' % (name, kind, n, pol, 'tracked' if trk else 'plain', mode)
        rows[key] = run_row(S, torch, kind, n, pol, trk, mode)
        print(key, rows[key], flush=True)
    with open(out, 'w') as f:
        json.dump(dict(label=label, steps=STEPS, rows=rows), f, indent=0)
    return 0


def compare(files, out):
    a, b, c = [json.load(open(f)) for f in files]
    assert set(a['rows']) == set(b['rows']) == set(c['rows']), 'the three runs are not of the same matrix'
    unstable = sorted(k for k in a['rows'] if a['rows'][k] != b['rows'][k])
    differ = sorted(k for k in a['rows'] if k not in unstable and a['rows'][k] != c['rows'][k])
    print('%d rows x %d steps; unstable between the reference library\'s two runs: %d; differing: %d' % (len(a['rows']), a['steps'], len(unstable), len(differ)))
    for k in unstable:
        print('  unstable:', k, a['rows'][k], b['rows'][k])
    for k in differ:
        print('  DIFFERS:', k, a['rows'][k], c['rows'][k])
    if out:
        with open(out, 'w') as f:
            json.dump(dict(reference=a['label'], compared=c['label'], steps=a['steps'], unstable_rows=unstable, differing_rows=differ,
                           rows={k: v for k, v in c['rows'].items() if k not in unstable}), f, indent=0)
    if 20 * len(unstable) > len(a['rows']):
        return 2
    return 1 if differ else 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None)
    ap.add_argument('--label', default='')
    ap.add_argument('--compare', nargs=3, metavar='JSON', default=None)
    args = ap.parse_args()
    sys.exit(compare(args.compare, args.out) if args.compare else run(args.out or 'forms_matrix.json', args.label))
