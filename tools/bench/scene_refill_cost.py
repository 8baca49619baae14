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
the batch's agent rows).  Beside them one sized restart call naming 1 and B / 4 scenes of that batch.

    python tools/bench/scene_refill_cost.py --harvest                             # 64 slots / 256 episodes -> profiles/scene_harvest_cost.json
    python tools/bench/scene_refill_cost.py --harvest --slots 1024 --waves 4      # 1024 slots / 4096 episodes, added to the same file
    python tools/bench/scene_refill_cost.py --harvest --parent-json parent.json   # ... held against the parent commit's `stream` windows

--harvest: the same queue streamed with run_episodes(harvest=False) and run_episodes(harvest=True), alternated:
    stream    the finished scene's state is cut out of a read-back of the whole batch, active / steps come with a second synchronisation
    harvest   the step that finishes a scene hands its rows and summary over (sca_scene_harvest_enable)
Identical final states per episode in both legs (asserted).  Per leg, beside the figures above: ms per batch step, the library's
synchronisations per batch step (counted per call: sca_env_step 1, sca_get_scene_state 1, sca_get_state 2, sca_scene_harvest_collect 1 -- on
a stream sca_env_step has just drained --, sca_restart_scenes 1) and the bytes that crossed the link per finished episode for its result
(sca_get_state: 84 B for every agent row of the batch, once per step in which a scene finished; the harvest: 77 B per row of the episode
and its 64-byte summary).  --parent-json: a scene_refill_cost.json written by the PARENT commit's tool on the same machine (same --slots,
--waves; --alternations 5); its `stream` windows are copied into the record, with whether this build's harvest=False leg lies inside their
min .. max.  The file keeps one entry per --slots under `runs`.

    python tools/bench/scene_refill_cost.py --episode-obstacles   # 256 episodes of 100 drones, 64 slots -> profiles/scene_obstacle_refill_cost.json

--episode-obstacles: every episode brings its own obstacle list -- a third of the queue none, a third 8 spheres, a third 1-5 spheres, all
seeded per episode (candidate c: c mod 3) -- and the queue runs in the two ways there are, alternated:
    waves     fresh SceneBatch(scene_obstacles=...) B at a time: the only way such a queue could run before the obstacle slots
    stream    run_episodes(episode_obstacles=..., obstacle_capacities='max'): a finished slot takes the next episode AND its obstacles
              (sca_restart_scenes_obstacles)
Identical final states per episode in both legs (asserted).  Beside them, on one batch of B slots (slot 0 of obstacle capacity 1491, the
others 8), the wall time of one restart call: sca_restart_scenes_sized naming 1 and B / 4 scenes, sca_restart_scenes_obstacles naming the
same scenes with 8 obstacles each, with -1 (keep) for each, and naming slot 0 with 1491 obstacles.

    python tools/bench/scene_refill_cost.py --attributes          # 256 episodes of 100 drones, 64 slots -> profiles/scene_attrs_cost.json

--attributes: a parameter study -- the same queue with `--values` of neighborDist dealt round-robin over the candidates -- in the two ways
there are, alternated:
    waves     B episodes at a time, ONE FRESH SceneBatch PER PARAMETER VALUE per wave: what a user had to do while a slot kept its attributes
    stream    run_episodes(attributes=True): a finished slot takes the next episode and its attributes (sca_restart_scenes_attrs)
Identical final states per episode in both legs (asserted).  Beside them the wall time of one restart call on one batch of B slots, naming 1
and 16 scenes, without attrs and with every attribute array: 30 samples each, median, min and max.  --parent-json: the samples of the same
call measured on the PARENT commit's library on the same machine (--restart-only, below); the record then says whether this build's call
without attrs lies inside the spread of the parent's own samples (median <= the parent's max).

    python tools/bench/scene_refill_cost.py --restart-only parent.json --package-root <a checkout of the parent commit, built>

--restart-only: nothing but the 30 samples of the restart call without attrs (1 and 16 scenes) on the library found under --package-root --
only calls every commit since sca_restart_scenes has.

    python tools/bench/scene_refill_cost.py --paths               # 256 episodes of 100 drones, 64 slots -> the `queue` entry of profiles/scene_paths_cost.json

--paths: the same queue with every drone carrying 0-5 seeded waypoints (Agent.path), in the two ways a user can run it:
    waves     B episodes at a time, one fresh SceneBatch per wave (the lists one block): what a user had to do while a slot refused lists
    stream    run_episodes(path_slots='max'): a finished slot takes the next episode and its lists (sca_restart_scenes_paths)
alternated, final states per episode identical.  Then one restart call naming 1 and 16 scenes, 30 samples each: on a batch in slot form
without path arrays and with the episodes' lists, and on a batch that is not in slot form.  --parent-json: the parent commit's
--restart-only samples; the entry records whether this build's medians without path arrays lie inside the parent's spread.
"""
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
    ap.add_argument('--harvest', action='store_true', help='the streamed queue with and without the scene harvest')
    ap.add_argument('--episode-obstacles', action='store_true', help='a queue whose episodes bring their own obstacles: waves of fresh batches against the streamed queue')
    ap.add_argument('--parent-json', default=None, help="--harvest: the parent commit's scene_refill_cost.json of the same queue on the same machine; "
                                                        "--attributes: the parent commit's --restart-only samples")
    ap.add_argument('--attributes', action='store_true', help='a parameter study: waves of one fresh batch per value against the streamed queue with attribute slots')
    ap.add_argument('--values', default='5,10,15', help='--attributes: the neighborDist values, dealt round-robin')
    ap.add_argument('--paths', action='store_true', help='a queue whose drones carry waypoint lists: waves of fresh batches against the streamed queue with path slots')
    ap.add_argument('--restart-only', default=None, metavar='OUT', help='write only the samples of one restart call (1 and 16 scenes, no attrs) to OUT')
    ap.add_argument('--package-root', default=None, help='import sca_amd from this checkout instead of the one the tool stands in')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.harvest + args.mixed + args.episode_obstacles + args.attributes + args.paths > 1:
        ap.error('--harvest, --mixed, --episode-obstacles, --attributes and --paths are five comparisons: one at a time')
    if args.out is None:
        args.out = os.path.join(REPO, 'profiles', 'scene_harvest_cost.json' if args.harvest else 'scene_sizes_cost.json' if args.mixed else
                                'scene_obstacle_refill_cost.json' if args.episode_obstacles else 'scene_attrs_cost.json' if args.attributes else
                                'scene_paths_cost.json' if args.paths else 'scene_refill_cost.json')
    sys.path.insert(0, args.package_root or REPO)
    from sca_amd import env as E, scenarios, scenes, solver as sol_mod
    pols = [E.SCAPolicy, E.RVO3DPolicy, E.SRVO3DPolicy, E.ORCA3DPolicy, E.ORCA3DPolicyOfficial, E.RVO3dDubinsPolicy]
    B, n1 = args.slots, args.agents
    count = B * args.waves

    candidates = list(range(count + max(8, count // (2 if args.episode_obstacles else 8))))      # (spheres in the way: more episodes without an end)
    choices = [int(v) for v in args.sizes.split(',')] if args.mixed else [n1]
    size_of = np.random.default_rng(2024).choice(choices, size=len(candidates))      # the agent count of candidate c

    values = [float(v) for v in args.values.split(',')]

    def value_of(c):
        return values[c % len(values)]                            # --attributes: candidate c's neighborDist

    def episode(c, lists=None):
        """lists: whether the drones carry waypoints (None: as --paths says)"""
        n = int(size_of[c])
        sc = scenarios.random_cube(n, seed=c)
        agents = [E.Agent(start_pos=list(sc['start'][i]), goal_pos=list(sc['goal'][i]), vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0,
                          policy=pols[c % len(pols)], id=i) for i in range(n)]
        if args.attributes:
            for a in agents:
                a.neighborDist = value_of(c)
        if args.paths if lists is None else lists:                  # 0-5 waypoints around the drone's straight line, seeded by the candidate
            rng = np.random.default_rng(3000 + c)
            for a, p, g in zip(agents, sc['start'], sc['goal']):
                fr = sorted(rng.uniform(0.1, 0.9, int(rng.integers(0, 6))), reverse=True)       # (list.pop() takes the last: the nearest)
                a.path = [[float(x) for x in np.round(p[:3] + (g[:3] - p[:3]) * f + rng.normal(0, 1.0, 3), 3)] for f in fr]
        return agents

    RESTART_SAMPLES = 30

    def restart_samples(sol, eps, k, attrs=None, sizes=None, obstacles=None, paths=False):
        """the wall time of RESTART_SAMPLES restart calls naming scenes 0 .. k - 1 with the episodes eps[0 .. k - 1], in seconds"""
        ids = list(range(k))
        flat = [a for s in ids for a in eps[s]]
        T = len(flat)
        start = np.array([a.initial_pos for a in flat]).reshape(T, 6)
        goal6 = np.array([a.goal_pos for a in flat]).reshape(T, 6)
        kw = dict(vel=np.zeros((T, 3), np.float32), radius=np.full(T, 0.5), pref_speed=np.ones(T), goal=np.ascontiguousarray(goal6[:, :3]),
                  policy=np.array([a.policy.policy_id for a in flat], np.uint8), zaxis=sol_mod.zaxis_flags(start, goal6),
                  max_run_dist=np.array([a.max_run_dist for a in flat]), goal_heading=np.ascontiguousarray(goal6[:, 3:6]))
        if attrs is not None:
            kw['attrs'] = attrs(flat)
        if paths:
            kw['paths'] = [[list(map(float, w[:3])) for w in a._path] for a in flat]
        pos, head = np.ascontiguousarray(start[:, :3]), np.ascontiguousarray(start[:, 3:6])
        ts = []
        for _ in range(RESTART_SAMPLES):
            t0 = time.perf_counter()
            sol.restart_scenes(ids, pos, head, sizes=sizes, obstacles=obstacles, **kw)
            ts.append(time.perf_counter() - t0)
        return ts

    def spread(ts):
        return {'median_ms': float(np.median(ts)) * 1e3, 'min_ms': float(min(ts)) * 1e3, 'max_ms': float(max(ts)) * 1e3, 'samples_ms': [t * 1e3 for t in ts]}

    if args.restart_only:
        # default attributes throughout: the batch and the call every commit since sca_restart_scenes has
        args.attributes = args.paths = False
        eps = [episode(c) for c in range(B + 16)]
        batch = scenes.SceneBatch(eps[:B], [], device_tracker=True)
        for _ in range(20):
            batch.step()
        doc = {'tool': 'tools/bench/scene_refill_cost.py --restart-only', 'slots': B, 'agents_per_episode': n1, 'samples': RESTART_SAMPLES,
               'no_attrs': {'scenes_1': spread(restart_samples(batch.solver, eps[B:], 1)), 'scenes_16': spread(restart_samples(batch.solver, eps[B:], 16))}}
        batch.close()
        with open(args.restart_only, 'w') as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write('\n')
        print(json.dumps({k: {q: v[q] for q in ('median_ms', 'min_ms', 'max_ms')} for k, v in doc['no_attrs'].items()}), flush=True)
        return

    def spheres(pos, radius):
        return [E.Obstacle(pos=list(map(float, p)), shape_dict={'shape': 'sphere', 'feature': float(r)}, id=i) for i, (p, r) in enumerate(zip(pos, radius))]

    def obstacles_of(c):
        """--episode-obstacles: candidate c's own list -- none, 8 or 1-5 spheres of radius 1 (c mod 3) inside the scene's cube, none within
        3 m of a start or a goal"""
        m = (0, 8, 1 + (c // 3) % 5)[c % 3]
        sc = scenarios.random_cube(int(size_of[c]), seed=c)
        ends = np.concatenate([sc['start'][:, :3], sc['goal'][:, :3]])
        lo, hi = ends.min(0), ends.max(0)
        rng, pts = np.random.default_rng(10 ** 6 + c), []
        while len(pts) < m:
            q = rng.uniform(lo, hi)
            if np.linalg.norm(ends - q, axis=1).min() > 3.0:
                pts.append(q)
        return spheres(pts, [1.0] * m)

    def batch_of(cs, eps=None, **kw):
        eps = [episode(c) for c in cs] if eps is None else eps
        if args.episode_obstacles:
            return scenes.SceneBatch(eps, scene_obstacles=[obstacles_of(c) for c in cs], device_tracker=True, **kw)
        return scenes.SceneBatch(eps, [], device_tracker=True, **kw)

    # the candidates that end: all of them as one batch, untimed
    batch = batch_of(candidates)
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
        states, steps, served, rows = [None] * count, 0, 0, 0
        for w in range(0, count, B):
            wave = list(range(w, min(w + B, count)))
            # --attributes: a slot keeps its attributes, so the wave falls apart into one fresh batch per parameter value
            groups = [[i for i in wave if value_of(chosen[i]) == v] for v in values] if args.attributes else [wave]
            for group in [g for g in groups if g]:
                batch = batch_of([chosen[i] for i in group], [eps[i] for i in group])
                done = False
                while not done:
                    served += int(batch.active.sum())
                    done = batch.step()
                    steps += 1
                    rows += len(group) * n1
                    assert steps < args.max_steps
                for s, i in enumerate(group):
                    lo, hi = int(batch.offsets[s]), int(batch.offsets[s + 1])
                    states[i] = {k: batch._state(k)[lo:hi].copy() for k in batch._mirror}
                batch.close()
        return time.perf_counter() - t0, states, dict(batch_steps=steps, agent_steps=served, live_fraction=served / rows)

    # --harvest: the library calls that synchronise, counted at the solver's methods while a leg runs (weights: synchronisations per call)
    SYNCS = dict(env_step=1, scene_state=1, get_state=2, scene_harvest_collect=1, restart_scenes=1)

    def counted(fn):
        calls = {k: 0 for k in SYNCS}
        keep = {k: getattr(sol_mod.BatchedSolver, k) for k in SYNCS}

        def wrap(name, inner):
            def method(self, *a, **kw):
                calls[name] += 1
                return inner(self, *a, **kw)
            return method
        for k, inner in keep.items():
            setattr(sol_mod.BatchedSolver, k, wrap(k, inner))
        try:
            return fn(), calls
        finally:
            for k, inner in keep.items():
                setattr(sol_mod.BatchedSolver, k, inner)

    def run_stream(capacities=None, harvest=None):
        eps = queue()
        stats = {}
        kw = {} if harvest is None else dict(harvest=harvest)
        if args.attributes:
            kw.update(attributes=True)
        if args.paths:
            kw.update(path_slots='max')
        if args.episode_obstacles:
            kw.update(episode_obstacles=[obstacles_of(c) for c in chosen], obstacle_capacities='max')
        t0 = time.perf_counter()
        res, calls = counted(lambda: scenes.run_episodes(eps, B, device_tracker=True, max_steps=args.max_steps, stats=stats, capacities=capacities, **kw))
        wall = time.perf_counter() - t0
        if harvest is not None:
            rows = sum(len(r['state']['flags']) for r in res)
            stats['calls'] = calls
            stats['syncs_per_batch_step'] = sum(SYNCS[k] * v for k, v in calls.items()) / stats['batch_steps']
            stats['readback_bytes_per_episode'] = (77 * rows + 64 * len(res)) / len(res) if harvest else 84 * B * n1 * calls['get_state'] / len(res)
        return wall, [r['state'] for r in res], stats

    legs = {'fixed': run_stream, 'capacity': lambda: run_stream('max')} if args.mixed else \
        {'stream': lambda: run_stream(harvest=False), 'harvest': lambda: run_stream(harvest=True)} if args.harvest else {'waves': run_waves, 'stream': run_stream}
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
    if args.episode_obstacles:                                       # slot 0 may hold a map's worth of obstacles, the others a field's
        batch = batch_of(chosen[:B], eps[:B], obstacle_capacities=[1491] + [8] * (B - 1))
    else:
        batch = scenes.SceneBatch(eps[:B], [], device_tracker=True, capacities=[cap] * B if args.mixed else None, **(dict(path_slots=5) if args.paths else {}))
    for _ in range(20):
        batch.step()
    sol = batch.solver
    t_step = []
    for _ in range(50):
        t0 = time.perf_counter()
        sol.env_step(batch.neighbor_mode)
        t_step.append(time.perf_counter() - t0)

    def restart_ms(k, obstacles=None):
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
            sol.restart_scenes(ids, pos, head, sizes=[len(eps[B + s]) for s in ids] if args.mixed else None, obstacles=obstacles, **kw)
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)) * 1e3
    if args.paths:
        # one restart call, 1 and 16 scenes: on the batch in slot form without path arrays (the named rows get empty lists) and with the
        # episodes' 0-5 waypoints per row, and on a batch without lists that is not in slot form (the call every earlier commit has)
        bare = [episode(c, lists=False) for c in chosen[:B + 16]]
        plain = scenes.SceneBatch(bare[:B], [], device_tracker=True)
        for _ in range(20):
            plain.step()
        call = {'slot_form_no_path_arrays': {'scenes_1': spread(restart_samples(sol, eps[B:], 1)), 'scenes_16': spread(restart_samples(sol, eps[B:], 16))},
                'slot_form_lists_0_5': {'scenes_1': spread(restart_samples(sol, eps[B:], 1, paths=True)), 'scenes_16': spread(restart_samples(sol, eps[B:], 16, paths=True))},
                'not_slot_form': {'scenes_1': spread(restart_samples(plain.solver, bare[B:], 1)), 'scenes_16': spread(restart_samples(plain.solver, bare[B:], 16))},
                'step_ms': float(np.median(t_step)) * 1e3,
                'note': 'one restart call on a batch of %d slots of %d drones, wall time around the Python call, %d samples each; slot form: room for 5 waypoints '
                        'per row' % (B, n1, RESTART_SAMPLES)}
        plain.close()
        if args.parent_json:
            with open(args.parent_json) as f:
                parent = json.load(f)
            assert (parent['slots'], parent['agents_per_episode']) == (B, n1), 'the parent measured another batch'
            call['parent_commit'] = parent['no_attrs']
            call['median_inside_parent_spread'] = {case: {k: bool(parent['no_attrs'][k]['min_ms'] <= call[case][k]['median_ms'] <= parent['no_attrs'][k]['max_ms'])
                                                          for k in ('scenes_1', 'scenes_16')} for case in ('slot_form_no_path_arrays', 'not_slot_form')}
        restart = call
    else:
        restart = {'scenes_1_ms': restart_ms(1), 'scenes_%d_ms' % max(1, B // 4): restart_ms(max(1, B // 4)), 'step_ms': float(np.median(t_step)) * 1e3}
    if args.episode_obstacles:
        rng = np.random.default_rng(7)
        eight = lambda: (rng.uniform(-20.0, 20.0, (8, 3)) + [0.0, 0.0, 30.0], np.ones(8))
        many = (rng.uniform(-40.0, 40.0, (1491, 3)) * [1.0, 1.0, 0.05], np.full(1491, 0.2))      # a map's worth, on the ground below the scene
        q = max(1, B // 4)
        restart = {'step_ms': restart['step_ms'], 'sized': {'scenes_1_ms': restart['scenes_1_ms'], 'scenes_%d_ms' % q: restart['scenes_%d_ms' % q]},
                   'obstacles_8_each': {'scenes_1_ms': restart_ms(1, [eight()]), 'scenes_%d_ms' % q: restart_ms(q, [eight() for _ in range(q)])},
                   'keep': {'scenes_1_ms': restart_ms(1, [None]), 'scenes_%d_ms' % q: restart_ms(q, [None] * q)},
                   'obstacles_1491': {'scenes_1_ms': restart_ms(1, [many])},
                   'note': 'sca_restart_scenes_sized / sca_restart_scenes_obstacles on one batch of %d slots, slot 0 of obstacle capacity 1491, the others 8; '
                           'median of 30 calls, wall time around the call' % B}
    if args.attributes:
        # one restart call, 1 and 16 scenes: without attrs (the call every earlier commit has) and with every attribute array
        names = dict(neighbor_dist='neighborDist', max_neighbors='maxNeighbors', time_step='timeStep', time_horizon='timeHorizon', max_speed='maxSpeed',
                     max_heading_change='max_heading_change', dt_nominal='dt_nominal')

        def every(flat):
            out = {k: [getattr(a, v) for a in flat] for k, v in names.items()}
            out.update(turning_radius=[a.turning_radius for a in flat], pitch_lo=[a.pitchlims[0] for a in flat], pitch_hi=[a.pitchlims[1] for a in flat])
            return out
        same_value = [e for e, c in zip(eps[B:], chosen[B:]) if value_of(c) == value_of(chosen[0])][:16]      # (without attrs a slot keeps its own)
        plain = scenes.SceneBatch([e for e, c in zip(eps, chosen) if value_of(c) == value_of(chosen[0])][:B], [], device_tracker=True)
        for _ in range(20):
            plain.step()
        call = {'no_attrs': {'scenes_1': spread(restart_samples(plain.solver, same_value, 1)), 'scenes_16': spread(restart_samples(plain.solver, same_value, 16))},
                'attrs': {'scenes_1': spread(restart_samples(sol, eps[B:], 1, attrs=every)), 'scenes_16': spread(restart_samples(sol, eps[B:], 16, attrs=every))},
                'step_ms': restart['step_ms'],
                'note': 'one restart call on a batch of %d slots of %d drones, wall time around the call, %d samples each; no_attrs: sca_restart_scenes on a batch '
                        'of one parameter value; attrs: sca_restart_scenes_attrs with all ten arrays' % (B, n1, RESTART_SAMPLES)}
        plain.close()
        if args.parent_json:
            with open(args.parent_json) as f:
                parent = json.load(f)
            assert (parent['slots'], parent['agents_per_episode']) == (B, n1), 'the parent measured another batch'
            call['parent_commit_no_attrs'] = parent['no_attrs']
            call['no_attrs_not_slower_than_parent_beyond_its_spread'] = {
                k: bool(call['no_attrs'][k]['median_ms'] <= parent['no_attrs'][k]['max_ms']) for k in ('scenes_1', 'scenes_16')}
        restart = call
    batch.close()

    doc = {'tool': 'tools/bench/scene_refill_cost.py' + (' --mixed' if args.mixed else ' --harvest' if args.harvest else ' --episode-obstacles' if args.episode_obstacles else
                                                         ' --attributes' if args.attributes else ' --paths' if args.paths else ''),
           'slots': B, 'episodes': count,
           'agents_per_episode': {str(n): int((size_of[chosen] == n).sum()) for n in choices} if args.mixed else n1, 'alternations': args.alternations,
           'episode_cap': args.episode_cap, 'last_seed': chosen[-1], 'seeds_left_out_no_end_within_cap': left_out,
           'policies': 'SCA, RVO3D, S-RVO3D, ORCA3D, ORCA3D-LP, RVO3D+Dubins in turn; seeded random scenes; device tracker in the pass',
           'final_states_identical': True, 'legs': {}, 'restart_call': restart}
    for name in legs:
        wall = float(np.median(walls[name]))
        st = stats[name]
        doc['legs'][name] = {'wall_s': wall, 'wall_s_all': walls[name], 'episodes_per_s': count / wall, 'agent_steps_per_s': st['agent_steps'] / wall,
                             'batch_steps': st['batch_steps'], 'agent_steps': st['agent_steps'], 'mean_live_fraction': st['live_fraction']}
        if args.harvest:
            doc['legs'][name].update(ms_per_batch_step=1e3 * wall / st['batch_steps'], syncs_per_batch_step=st['syncs_per_batch_step'],
                                     readback_bytes_per_episode=st['readback_bytes_per_episode'], library_calls=st['calls'])
    if args.attributes:
        doc['neighborDist_values'] = values
        doc['episodes_per_value'] = {str(v): int(sum(value_of(c) == v for c in chosen)) for v in values}
    if args.paths:
        doc['waypoints_per_drone'] = '0-5, seeded by the episode; stream: run_episodes(path_slots="max")'
    if args.episode_obstacles:
        doc['obstacles_per_episode'] = {str(m): int(sum(len(obstacles_of(c)) == m for c in chosen)) for m in (0, 1, 2, 3, 4, 5, 8)}
    ratio = 'capacity_over_fixed_episodes_per_s' if args.mixed else 'harvest_over_stream_episodes_per_s' if args.harvest else 'stream_over_waves_episodes_per_s'
    over, under = ('capacity', 'fixed') if args.mixed else ('harvest', 'stream') if args.harvest else ('stream', 'waves')
    doc[ratio] = doc['legs'][over]['episodes_per_s'] / doc['legs'][under]['episodes_per_s']
    if args.harvest and args.parent_json:
        with open(args.parent_json) as f:
            parent = json.load(f)
        assert (parent['slots'], parent['episodes'], parent['last_seed']) == (B, count, chosen[-1]), 'the parent ran another queue'
        windows = parent['legs']['stream']['wall_s_all']
        mine = doc['legs']['stream']['wall_s']
        doc['parent_commit_stream'] = {'wall_s_all': windows, 'wall_s': parent['legs']['stream']['wall_s'], 'min_s': min(windows), 'max_s': max(windows),
                                       'this_build_stream_wall_s': mine, 'inside_parent_spread': bool(min(windows) <= mine <= max(windows))}
    if args.harvest:                                                 # one entry per --slots in the file
        runs = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                runs = json.load(f).get('runs', {})
        runs[str(B)] = doc
        doc = {'tool': 'tools/bench/scene_refill_cost.py --harvest', 'runs': runs}
    if args.paths:                                                   # beside the `step` entry of tools/bench/path_slots_step_cost.py
        whole = {}
        if os.path.exists(args.out):
            with open(args.out) as f:
                whole = json.load(f)
        whole['queue'] = doc
        doc = whole
    if args.mixed:
        doc['restart_call']['note'] = 'sca_restart_scenes_sized, the named slots of capacity %d taking the queue\'s next episodes' % cap
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    shown = doc['runs'][str(B)] if args.harvest else doc['queue'] if args.paths else doc
    print(json.dumps({k: shown[k] for k in ('legs', 'restart_call', ratio, 'parent_commit_stream') if k in shown}), flush=True)


if __name__ == '__main__':
    main()
