#!/usr/bin/env python
"""What streaming an episode queue through B slots (scenes.run_episodes, sca_restart_scenes) buys over running it in waves of B.  ONE process,
the two ways alternated, the median of the alternations taken; every run builds its Agent objects afresh.

    python tools/bench/scene_refill_cost.py                       # 4 x 64 episodes of 100 drones -> profiles/scene_refill_cost.json
    python tools/bench/scene_refill_cost.py --slots 16 --waves 3 --alternations 2

queue: `--waves` x `--slots` episodes of `--agents` drones, the six policies in turn, each a seeded random scene (scenarios.random_cube).  An
episode ends when every drone has arrived, collided or run out of distance, and a drone that stands still in a deadlock does none of these
(ORCA3D-LP leaves one such drone in a few seeds): an episode without an end cannot stand in a queue, in waves or streamed.  So the candidates
(seed c, policy c mod 6) are first run together in one batch for `--episode-cap` steps, untimed, and the queue is the first that finished;
the seeds left out are written beside the figures.
legs
    waves     the queue B at a time, each wave a fresh SceneBatch stepped until its slowest scene is done: the only way there was
    stream    scenes.run_episodes through B slots: a finished slot restarts with the next episode while the others keep running
Both legs must leave identical final states per episode (asserted).  Per leg: wall time, episodes/s, agent-steps/s (agents served, summed over
the steps), batch steps, the mean live fraction per step.  Beside them: the wall time of ONE sca_restart_scenes call naming 1 scene and
B / 4 scenes, and the step time of the same batch.

    python tools/bench/scene_refill_cost.py --mixed               # 256 episodes of 20 / 50 / 100 drones, 64 slots -> profiles/scene_sizes_cost.json

--mixed: the queue mixes agent counts (`--sizes`, drawn per episode from a seeded generator; policies in turn as above) and is streamed through
the same B slots in the two ways scenes.run_episodes has, alternated:
    fixed     capacities=None: a slot keeps its size, so the queue falls apart into one sub-queue per count and the slots of a count that is
              exhausted idle to the end
    capacity  capacities='max': every slot holds up to the largest count and takes the first pending episode (sca_restart_scenes_sized)
Identical final states per episode in both legs (asserted); per leg episodes/s, batch steps and the live fraction (agents served / batch steps x
the batch's agent rows).  Beside them one sized restart call naming 1 and B / 4 scenes of that batch."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slots', type=int, default=64)
    ap.add_argument('--waves', type=int, default=4)
    ap.add_argument('--agents', type=int, default=100)
    ap.add_argument('--alternations', type=int, default=3)
    ap.add_argument('--max-steps', type=int, default=200000)
    ap.add_argument('--episode-cap', type=int, default=4000, help='candidate episodes that have not ended after this many steps are left out of the queue')
    ap.add_argument('--mixed', action='store_true', help='a queue of mixed agent counts: fixed-size slots against capacity slots')
    ap.add_argument('--sizes', default='20,50,100', help='--mixed: the agent counts the episodes are drawn from')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, 'profiles', 'scene_sizes_cost.json' if args.mixed else 'scene_refill_cost.json')
    sys.path.insert(0, REPO)
    from sca_amd import env as E, scenarios, scenes, solver as sol_mod
    pols = [E.SCAPolicy, E.RVO3DPolicy, E.SRVO3DPolicy, E.ORCA3DPolicy, E.ORCA3DPolicyOfficial, E.RVO3dDubinsPolicy]
    B, n1 = args.slots, args.agents
    count = B * args.waves

    candidates = list(range(count + max(8, count // 8)))
    choices = [int(v) for v in args.sizes.split(',')] if args.mixed else [n1]
    size_of = np.random.default_rng(2024).choice(choices, size=len(candidates))      # the agent count of candidate c

    def episode(c):
        n = int(size_of[c])
        sc = scenarios.random_cube(n, seed=c)
        return [E.Agent(start_pos=list(sc['start'][i]), goal_pos=list(sc['goal'][i]), vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0,
                        policy=pols[c % len(pols)], id=i) for i in range(n)]

    # the candidates that end: all of them as one batch, untimed
    batch = scenes.SceneBatch([episode(c) for c in candidates], [], device_tracker=True)
    for _ in range(args.episode_cap):
        if batch.step():
            break
    ended = [c for c in candidates if batch.done[c]]
    batch.close()
    assert len(ended) >= count, 'only %d of %d candidate episodes ended within %d steps' % (len(ended), len(candidates), args.episode_cap)
    chosen = ended[:count]
    left_out = [c for c in range(chosen[-1]) if c not in set(chosen)]
    print('queue: seeds 0 .. %d without %s' % (chosen[-1], left_out), flush=True)

    def queue():
        return [episode(c) for c in chosen]

    def run_waves():
        eps = queue()
        t0 = time.perf_counter()
        states, steps, served = [], 0, 0
        for w in range(0, count, B):
            batch = scenes.SceneBatch(eps[w:w + B], [], device_tracker=True)
            done = False
            while not done:
                served += int(batch.active.sum())
                done = batch.step()
                steps += 1
                assert steps < args.max_steps
            for s in range(len(batch)):
                lo, hi = int(batch.offsets[s]), int(batch.offsets[s + 1])
                states.append({k: batch._state(k)[lo:hi].copy() for k in batch._mirror})
            batch.close()
        return time.perf_counter() - t0, states, dict(batch_steps=steps, agent_steps=served, live_fraction=served / (steps * B * n1))

    def run_stream(capacities=None):
        eps = queue()
        stats = {}
        t0 = time.perf_counter()
        res = scenes.run_episodes(eps, B, device_tracker=True, max_steps=args.max_steps, stats=stats, capacities=capacities)
        return time.perf_counter() - t0, [r['state'] for r in res], stats

    legs = {'fixed': run_stream, 'capacity': lambda: run_stream('max')} if args.mixed else {'waves': run_waves, 'stream': run_stream}
    walls = {k: [] for k in legs}
    stats, first = {}, None
    for _ in range(args.alternations):
        for name, fn in legs.items():
            wall, states, st = fn()
            walls[name].append(wall)
            stats[name] = st
            if first is None:
                first = states
            for i, (a, b) in enumerate(zip(first, states)):     # every run of either leg: the same final state per episode
                for key in a:
                    assert np.array_equal(a[key], b[key]), (name, 'episode', i, key)
            print('%-8s %.3f s, %d batch steps, live fraction %.3f' % (name, wall, st['batch_steps'], st['live_fraction']), flush=True)

    # one restart call beside one step of the same batch (--mixed: slots of the largest count, the restarts sized)
    eps = queue()
    cap = max(choices)
    batch = scenes.SceneBatch(eps[:B], [], device_tracker=True, capacities=[cap] * B if args.mixed else None)
    for _ in range(20):
        batch.step()
    sol = batch.solver
    t_step = []
    for _ in range(50):
        t0 = time.perf_counter()
        sol.env_step(batch.neighbor_mode)
        t_step.append(time.perf_counter() - t0)

    def restart_ms(k):
        ids = list(range(k))
        flat = [a for s in ids for a in eps[B + s]]
        T = len(flat)
        start = np.array([a.initial_pos for a in flat]).reshape(T, 6)
        goal6 = np.array([a.goal_pos for a in flat]).reshape(T, 6)
        kw = dict(vel=np.zeros((T, 3), np.float32), radius=np.full(T, 0.5), pref_speed=np.ones(T), goal=np.ascontiguousarray(goal6[:, :3]),
                  policy=np.array([a.policy.policy_id for a in flat], np.uint8), zaxis=sol_mod.zaxis_flags(start, goal6),
                  max_run_dist=np.array([a.max_run_dist for a in flat]), goal_heading=np.ascontiguousarray(goal6[:, 3:6]))
        pos, head = np.ascontiguousarray(start[:, :3]), np.ascontiguousarray(start[:, 3:6])
        ts = []
        for _ in range(30):
            t0 = time.perf_counter()
            sol.restart_scenes(ids, pos, head, sizes=[len(eps[B + s]) for s in ids] if args.mixed else None, **kw)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3
    restart = {'scenes_1_ms': restart_ms(1), 'scenes_%d_ms' % max(1, B // 4): restart_ms(max(1, B // 4)), 'step_ms': float(np.median(t_step)) * 1e3}
    batch.close()

    doc = {'tool': 'tools/bench/scene_refill_cost.py' + (' --mixed' if args.mixed else ''), 'slots': B, 'episodes': count,
           'agents_per_episode': {str(n): int((size_of[chosen] == n).sum()) for n in choices} if args.mixed else n1, 'alternations': args.alternations,
           'episode_cap': args.episode_cap, 'last_seed': chosen[-1], 'seeds_left_out_no_end_within_cap': left_out,
           'policies': 'SCA, RVO3D, S-RVO3D, ORCA3D, ORCA3D-LP, RVO3D+Dubins in turn; seeded random scenes; device tracker in the pass',
           'final_states_identical': True, 'legs': {}, 'restart_call': restart}
    for name in legs:
        wall = float(np.median(walls[name]))
        st = stats[name]
        doc['legs'][name] = {'wall_s': wall, 'wall_s_all': walls[name], 'episodes_per_s': count / wall, 'agent_steps_per_s': st['agent_steps'] / wall,
                             'batch_steps': st['batch_steps'], 'agent_steps': st['agent_steps'], 'mean_live_fraction': st['live_fraction']}
    ratio = 'capacity_over_fixed_episodes_per_s' if args.mixed else 'stream_over_waves_episodes_per_s'
    over, under = ('capacity', 'fixed') if args.mixed else ('stream', 'waves')
    doc[ratio] = doc['legs'][over]['episodes_per_s'] / doc['legs'][under]['episodes_per_s']
    if args.mixed:
        doc['restart_call']['note'] = 'sca_restart_scenes_sized, the named slots of capacity %d taking the queue\'s next episodes' % cap
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps({k: doc[k] for k in ('legs', 'restart_call', ratio)}), flush=True)


if __name__ == '__main__':
    main()
