#!/usr/bin/env python3
"""Many small episodes as ONE batch: the six policies x circle / random scenes of 100 drones, stepped by one context (sca_amd.scenes),
one metrics row per scene -- what a loop over the reference's run_example/run_*.py scripts produces, scene by scene.

    python examples/run_scenes.py
    python examples/run_scenes.py --agents 50 --seeds 8 --max-steps 3000
    python examples/run_scenes.py --obstacles          # ... and a take-off/landing scene (16 drones, 8 spheres) per policy in the same batch:
                                                       # every scene meets its own obstacles only (SceneBatch(scene_obstacles=...))
    python examples/run_scenes.py --seeds 8 --slots 16 # the same table -- policies x (circle + 8 seeds) -- as a QUEUE streamed through 16 slots
                                                       # (scenes.run_episodes): a slot that finishes restarts with the next episode
    python examples/run_scenes.py --seeds 2 --slots 8 --log-dir out    # ... and one folder per episode under out/: env_cfg.json + trajs.npz, what
                                                       # run_example/run_*.py write (the log per scene, SceneBatch(scene_history=...))
    python examples/run_scenes.py --sizes 20,50,100 --slots 16 --capacity max   # the scenarios at several drone counts through ONE queue: every
                                                       # slot holds up to the largest count and takes the next episode that fits
                                                       # (without --capacity a slot keeps its size: one slot at least per count)
    python examples/run_scenes.py --obstacles --seeds 8 --slots 16    # the obstacle scenarios as ONE queue: every episode brings its own
                                                       # obstacles into the slot it takes (run_episodes(episode_obstacles=...)) -- the
                                                       # random scenes 1-5 spheres that differ per seed, the take-off field its 8, and
                                                       # with --map <binvox> the exp3 search among the map's spheres
    python examples/run_scenes.py --seeds 8 --slots 16 --harvest      # the streamed queue with the finished scenes handed over by the step that
                                                       # finishes them (sca_scene_harvest_enable): the same rows, one synchronisation a step
    python examples/run_scenes.py --sweep neighborDist=5,10,15 --seeds 4 --slots 16    # a PARAMETER TABLE as one queue: every scenario at
                                                       # every value of one Agent attribute (neighborDist, maxNeighbors, timeStep, timeHorizon,
                                                       # maxSpeed, max_heading_change, dt_nominal, turning_radius); a slot takes the episode's
                                                       # own attributes with the restart (run_episodes(attributes=True)); one row per episode,
                                                       # the value in the row
    python examples/run_scenes.py --waypoints 3 --seeds 8 --slots 16    # every drone routed through 3 waypoints (Agent.path), the table still
                                                       # ONE queue: a slot takes the episode's own lists with the restart
                                                       # (run_episodes(path_slots=...))
    python examples/run_scenes.py --seeds 8 --slots 16 --save-at 150 --save-dir ckpt   # a table across TWO runs: behind 150 batch steps every
    python examples/run_scenes.py --seeds 8 --slots 16 --resume ckpt                   # running episode is written as a checkpoint (scenes.SceneCheckpoint)
                                                       # and the run stops; the second run resumes them in their slots and
                                                       # streams the rest of the queue -- together the rows of one run
    python examples/run_scenes.py --clearance --margin 0.1            # ... and how close the drones came: every row gains the smallest
                                                       # agent-agent and agent-obstacle clearance (distance - radius sum) and the drones that
                                                       # came within the margin, kept on the device with the step (sca_scene_clearance_enable);
                                                       # with or without --slots
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sca_amd import env as E, metrics, read_map, scenarios            # noqa: E402
from sca_amd.scenes import SceneBatch, SceneCheckpoint, run_episodes  # noqa: E402

SWEEPABLE = {'neighborDist': float, 'maxNeighbors': int, 'timeStep': float, 'timeHorizon': float, 'maxSpeed': float, 'max_heading_change': float,
             'dt_nominal': float, 'turning_radius': float}        # the Agent attributes a slot takes with a restart (agent.py:24-41)

POLICIES = {'sca': E.SCAPolicy, 'rvo': E.RVO3DPolicy, 'srvo': E.SRVO3DPolicy, 'orca': E.ORCA3DPolicy, 'orca-lp': E.ORCA3DPolicyOfficial,
            'rvo-dubins': E.RVO3dDubinsPolicy}


def build_agents(sc, policy):
    return [E.Agent(start_pos=list(sc['start'][i]), goal_pos=list(sc['goal'][i]), vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0,
                    policy=policy, id=i) for i in range(len(sc['start']))]


def spheres(pos, radius):
    return [E.Obstacle(pos=list(p), shape_dict={'shape': 'sphere', 'feature': float(r)}, id=i) for i, (p, r) in enumerate(zip(pos, radius))]


def random_spheres(sc, seed):
    """1-5 spheres of radius 1 that differ per seed, inside the box of the scene's starts, none within 3 m of a start or a goal"""
    rng = np.random.default_rng(1000 + seed)
    lo, hi = sc['start'][:, :3].min(0), sc['start'][:, :3].max(0)
    ends = np.concatenate([sc['start'][:, :3], sc['goal'][:, :3]])
    out = []
    while len(out) < 1 + seed % 5:
        p = rng.uniform(lo, hi)
        if np.linalg.norm(ends - p, axis=1).min() > 3.0:
            out.append(p)
    return spheres(out, [1.0] * len(out))


def add_waypoints(agents, k, seed):
    """every drone gets k waypoints (Agent.path) scattered 1.5 m around its straight line, deterministic per seed; get_trajectory pops from
    the END of the list, so the list runs from the goal's side to the start's"""
    rng = np.random.default_rng(2000 + seed)
    for a in agents:
        p, g = np.asarray(a.initial_pos[:3], dtype=np.float64), np.asarray(a.goal_pos[:3], dtype=np.float64)
        fractions = sorted(rng.uniform(0.15, 0.85, k), reverse=True)
        a.path = [[float(x) for x in np.round(p + (g - p) * f + rng.normal(0, 1.5, 3) * [1, 1, 0.3], 3)] for f in fractions]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=100)
    ap.add_argument('--seeds', type=int, default=3, help='random scenes per policy (beside one circle scene)')
    ap.add_argument('--max-steps', type=int, default=20000)
    ap.add_argument('--obstacles', action='store_true', help='add a take-off/landing scene with its 8 spheres per policy (one obstacle list per scene); '
                                                             'with --slots also 1-5 spheres per random scene, and the exp3 search where --map is given')
    ap.add_argument('--map', default=None, help='with --obstacles --slots: binvox map of the exp3 scenario (16 drones among its spheres), as for run_sca.py')
    ap.add_argument('--slots', type=int, default=0, help='stream the table through this many slots instead of holding it as one batch')
    ap.add_argument('--sizes', default=None, help='drone counts, e.g. 20,50,100: every scenario at each of them (instead of --agents)')
    ap.add_argument('--capacity', default=None, help="with --slots: 'max' makes every slot hold up to the largest episode, so a slot takes any "
                                                     'episode of the queue; a number is the capacity of every slot')
    ap.add_argument('--harvest', action='store_true', help='with --slots: finished scenes hand over their result with the step (run_episodes(harvest=True))')
    ap.add_argument('--sweep', default=None, help='with --slots: NAME=v1,v2,...: every scenario once per value of this Agent attribute (%s), '
                                                  'all of them one queue' % ', '.join(SWEEPABLE))
    ap.add_argument('--waypoints', type=int, default=0, help='route every drone through this many seeded waypoints (Agent.path); with --slots the '
                                                             "queue's slots take every episode's own lists (run_episodes(path_slots=...))")
    ap.add_argument('--save-at', type=int, default=0, help='with --slots and --save-dir: stop behind this many batch steps and write every running '
                                                           'episode there as a checkpoint')
    ap.add_argument('--save-dir', default=None, help='where --save-at writes the checkpoints and queue.json')
    ap.add_argument('--resume', default=None, help='with --slots and the arguments of the run that saved: resume the checkpoints of this directory in '
                                                   'their slots and stream the rest of the queue')
    ap.add_argument('--clearance', action='store_true', help='add MinClearance, MinObstacleClearance and the near-miss count to every row '
                                                             '(SceneBatch(clearance=True) / run_episodes(clearance=True))')
    ap.add_argument('--margin', type=float, default=0.0, help='with --clearance: a drone whose smallest clearance is at most this many metres is a near miss')
    ap.add_argument('--log-dir', default=None, help='write one folder per episode here: env_cfg.json + trajs.npz (the first --max-steps steps of each)')
    args = ap.parse_args()
    if args.map and not (args.slots and args.obstacles):
        ap.error('--map adds the exp3 episodes to the streamed obstacle queue: give --obstacles and --slots')
    if args.capacity and not args.slots:
        ap.error('--capacity is about the slots of a streamed queue: give --slots')
    if args.harvest and not args.slots:
        ap.error('--harvest is about the streamed queue: give --slots')
    if (args.save_at or args.save_dir or args.resume) and not args.slots:
        ap.error('--save-at / --save-dir / --resume are about the streamed queue: give --slots')
    if args.margin and not args.clearance:
        ap.error('--margin is about --clearance')
    if bool(args.save_at) != bool(args.save_dir):
        ap.error('--save-at STEP and --save-dir DIR go together')
    sweep_name, sweep_values = None, [None]
    if args.sweep:
        if not args.slots:
            ap.error('--sweep streams a parameter table as one queue: give --slots')
        sweep_name, _, vals = args.sweep.partition('=')
        if sweep_name not in SWEEPABLE or not vals:
            ap.error('--sweep NAME=v1,v2,... with NAME one of ' + ', '.join(SWEEPABLE))
        sweep_values = [SWEEPABLE[sweep_name](v) for v in vals.split(',')]
    counts = [int(v) for v in args.sizes.split(',')] if args.sizes else [args.agents]
    many = len(counts) > 1
    if many and not args.slots:
        ap.error('--sizes with several counts streams one queue: give --slots (and --capacity max)')
    capacities = None if not args.capacity else 'max' if args.capacity == 'max' else [int(args.capacity)] * args.slots

    names, scenes, obstacles = [], [], []
    for pname, pol in POLICIES.items():
        for n in counts:
            tag = ' x%d' % n if many else ''
            names.append((pname, 'circle' + tag))
            scenes.append(build_agents(scenarios.circle(n), pol))
            for seed in range(args.seeds):
                names.append((pname, 'random seed %d' % seed + tag))
                sc = scenarios.random_cube(n, seed=seed)
                scenes.append(build_agents(sc, pol))
                obstacles.append(random_spheres(sc, seed) if args.obstacles and args.slots else [])
            obstacles.insert(len(obstacles) - args.seeds, [])         # (the circle: open)
        if args.obstacles:
            sc = scenarios.takeoff_landing(16)
            names.append((pname, 'take-off'))
            scenes.append(build_agents(sc, pol))
            obstacles.append(spheres(sc['obs_pos'], sc['obs_radius']))
        if args.map:
            names.append((pname, 'exp3'))
            scenes.append(build_agents(scenarios.spawn_n_drones(16), pol))
            obstacles.append(read_map.read_obstacle(center=(35, 30), environ='exp3', obs_path=args.map))
    if sweep_name:                                                    # the table once per value: fresh Agent objects, the value on every agent
        base_names, base_scenes, base_obstacles = names, scenes, obstacles
        names, scenes, obstacles = [], [], []
        for v in sweep_values:
            for (pname, what), agents, obs in zip(base_names, base_scenes, base_obstacles):
                fresh = [E.Agent(start_pos=list(a.initial_pos), goal_pos=list(a.goal_pos), vel=[0.0, 0.0, 0.0], radius=a.radius, pref_speed=a.pref_speed,
                                 policy=type(a.policy), id=a.id) for a in agents]
                for a in fresh:
                    setattr(a, sweep_name, v)
                names.append((pname, '%s %s=%g' % (what, sweep_name, v)))
                scenes.append(fresh)
                obstacles.append(obs)
    if args.waypoints:
        for k, agents in enumerate(scenes):
            add_waypoints(agents, args.waypoints, k)

    def closest(rec):
        """the clearance columns of a printed row"""
        c = metrics.clearance_metrics(rec, args.margin)
        return '  MinClearance %.5f  MinObstacleClearance %.5f  NearMisses %d' % (c['MinClearance'], c['MinObstacleClearance'], len(c['NearMisses']))

    def folder(k):
        return os.path.join(args.log_dir, '%03d_%s_%s' % (k, names[k][0], names[k][1].replace(' ', '_')))

    if args.slots:
        t0, stats = time.time(), {}
        queue, queue_obstacles, order = scenes, obstacles, list(range(len(scenes)))
        if args.resume:                                               # the saved run's slots first, in slot order, then the episodes that never started
            with open(os.path.join(args.resume, 'queue.json')) as f:
                saved = json.load(f)
            order = [i for _, i, _ in saved['checkpoints']] + saved['pending']
            queue = [SceneCheckpoint.read(os.path.join(args.resume, name)) for _, _, name in saved['checkpoints']] + [scenes[i] for i in saved['pending']]
            queue_obstacles = [obstacles[i] for i in order]

        def row(r):
            r = dict(r, episode=order[r['episode']])
            pname, what = names[r['episode']]
            print('%-10s %-*s slot %3d steps %5d  ' % (pname, 40 if sweep_name else 20, what, r['slot'], r['steps']) +
                  '  '.join('%s %.4g' % (k, r['metrics'][k]) for k in ('SuccessRate', 'ExtraTime', 'ExtraDistance', 'AverageSpeed')) +
                  (closest(r['clearance']) if args.clearance else ''), flush=True)
            if args.log_dir:
                metrics.write_log_files(folder(r['episode']), scenes[r['episode']], r['trajectories'], r['info'], xlsx=False)
                if r['rows_dropped']:
                    print('    (the log holds the first %d steps: %d more did not fit --max-steps rows)' % (r['trajectories'].shape[1], r['rows_dropped']))
        run_episodes(queue, args.slots, device_tracker=True, on_done=row, max_steps=args.max_steps, stats=stats,
                     history_rows=args.max_steps if args.log_dir else 0, capacities=capacities, harvest=args.harvest,
                     episode_obstacles=queue_obstacles if args.obstacles else None, attributes=bool(sweep_name),
                     path_slots=args.waypoints or None, checkpoint_at=(args.save_at, args.save_dir) if args.save_at else None, clearance=args.clearance)
        if 'checkpoints' in stats:
            with open(os.path.join(args.save_dir, 'queue.json'), 'w') as f:
                json.dump(dict(batch_step=args.save_at, checkpoints=[[s, order[i], os.path.basename(path)] for s, (i, path) in sorted(stats['checkpoints'].items())],
                               pending=[order[i] for i in stats['pending']]), f)
            print('stopped behind %d batch steps: %d running episodes written to %s, %d more pending (--resume %s)' %
                  (args.save_at, len(stats['checkpoints']), args.save_dir, len(stats['pending']), args.save_dir))
            return
        print('%d episodes through %d slots: %d batch steps, mean live fraction %.2f, %.2f s' %
              (len(scenes), args.slots, stats['batch_steps'], stats['live_fraction'], time.time() - t0) +
              (' (%d waypoints per drone, the lists in slot form)' % args.waypoints if args.waypoints else ''))
        return
    rows = args.max_steps if args.log_dir else 0
    batch = SceneBatch(scenes, scene_obstacles=obstacles, device_tracker=True, scene_history=rows, clearance=args.clearance) if args.obstacles else \
        SceneBatch(scenes, [], device_tracker=True, scene_history=rows, clearance=args.clearance)
    t0, steps = time.time(), 0
    while steps < args.max_steps and not batch.step():
        steps += 1
    print('%d scenes, %d agents: %d batch steps, %.2f s' % (len(batch), sum(len(s) for s in scenes), steps + 1, time.time() - t0))
    for s, (pname, what) in enumerate(names):
        m = metrics.episode_metrics(batch.env(s))
        print('%-10s %-14s steps %5d %s  ' % (pname, what, batch.steps[s], 'done' if batch.done[s] else 'RUNNING') +
              '  '.join('%s %.4g' % (k, m[k]) for k in ('SuccessRate', 'ExtraTime', 'ExtraDistance', 'AverageSpeed')) +
              (closest(batch.env(s).clearance) if args.clearance else ''))
        if args.log_dir:
            metrics.write_episode_log(batch.env(s), folder(s), xlsx=False)
    batch.close()


if __name__ == '__main__':
    main()
