#!/usr/bin/env python3
"""The reference's run_example/run_sca.py, on the MI355X path: same scenario builders, same `while env.step(...)` loop, same
log files -- only the imports differ (sca_amd.env instead of mamp.*).

    python examples/run_sca.py                     # circle, 16 drones, 8 obstacle spheres (the reference's default run)
    python examples/run_sca.py --scenario takeoff  # exp2: take-off / landing
    python examples/run_sca.py --scenario exp3 --map tests/golden/exp3_map.binvox   # low-altitude search among 1491 spheres
    python examples/run_sca.py --scenario circle --agents 2000 --no-obstacles --policy orca
    python examples/run_sca.py --clearance --margin 0.2   # ... and how close the drones came (sca_clearance_enable)
    python examples/run_sca.py --lifelong 2000 --traffic 0.05 --spawn-margin 0.5   # drones leave when they arrive, new ones enter where there is room
    python examples/run_sca.py --lifelong 2000 --traffic 0.05 --save-at 1000 --save-file cut.npz   # ... cut behind step 1000, vacant rows and all,
    python examples/run_sca.py --lifelong 2000 --traffic 0.05 --resume cut.npz                     # and taken up again: the uncut run's summary
"""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sca_amd import env as E, metrics, read_map, scenarios, solver as S, tracker          # noqa: E402

POLICIES = {'sca': E.SCAPolicy, 'rvo': E.RVO3DPolicy, 'srvo': E.SRVO3DPolicy, 'orca': E.ORCA3DPolicy,
            'orca-lp': E.ORCA3DPolicyOfficial, 'rvo-dubins': E.RVO3dDubinsPolicy}


def build_obstacles():
    """run_sca.py:129-155 (exp2): eight spheres of radius 1 on a ring of radius 4 at z = 5."""
    out = []
    for j in range(8):
        out.append(E.Obstacle(pos=[round(4.0 * math.cos(2 * j * math.pi / 8), 2), round(4.0 * math.sin(2 * j * math.pi / 8), 2), 5.0],
                              shape_dict={'shape': 'sphere', 'feature': 1.0}, id=j))
    return out


def lifelong(args, agents, obstacles, pol, dubins):
    """--lifelong STEPS: ping-pong.  An arrived drone flies back to where its mission began; a collided or timed-out one starts its
    original mission again.  --waypoints K: every leg follows a route of K seeded waypoints (Agent.path), reversed on the way back."""
    from sca_amd.lifelong import run_lifelong
    K = args.waypoints
    fleet = [POLICIES[name] for name in args.fleet.split(',')] if args.fleet else None
    ck = None
    if args.resume and args.traffic is not None:                   # the env as --save-at left it, vacant rows and all; the host loop's state is in the file too
        from sca_amd.checkpoint import ContextCheckpoint
        ck = ContextCheckpoint.read(args.resume)
        env = E.MACAEnv.from_checkpoint(ck)
    elif fleet:                                                      # a mixed fleet: an arriving drone brings its own policy (MACAEnv(attribute_slots=True))
        dubins = dubins or any(p in (E.SCAPolicy, E.RVO3dDubinsPolicy) for p in fleet)
        env = E.MACAEnv(device_tracker=dubins, clearance=args.clearance, path_slots=K, attribute_slots=True)
    else:
        env = E.MACAEnv(device_tracker=dubins, clearance=args.clearance, path_slots=K)
    per_policy = {p.__name__: dict(entered=0, arrived=0, collided=0, timed_out=0) for p in fleet or ()}

    def line_of(agent):
        return per_policy.setdefault(type(agent.policy).__name__, dict(entered=0, arrived=0, collided=0, timed_out=0))
    if fleet:                                                      # entered: counted where env.respawn admits an arrival (a vacant row's new drone)
        respawn = env.respawn

        def counting_respawn(new, margin=None):
            new = list(new)
            were_vacant = {a.id for a in new if env.agents[a.id].is_vacant}
            got = respawn(new, margin=margin)
            for a in (new if margin is None else got):
                if a.id in were_vacant:
                    line_of(a)['entered'] += 1
            return got
        env.respawn = counting_respawn
    first = {a.id: (list(a.initial_pos), list(a.goal_pos)) for a in agents}
    route = {}                                                     # id -> the K waypoints from its start to its goal, in flying order
    for i, (start, goal) in first.items():
        rng = np.random.default_rng(1000 + i)
        p, g = np.asarray(start[:3], float), np.asarray(goal[:3], float)
        route[i] = [[float(x) for x in np.round(p + (g - p) * (k + 1) / (K + 1) + rng.normal(0.0, 0.5, 3), 3)] for k in range(K)]
    out_list = {i: r[::-1] for i, r in route.items()}              # (get_trajectory pops from the end: the first waypoint stands last)
    back_list = {i: r[:] for i, r in route.items()}
    if K:
        for a in agents:
            a.path = [w[:] for w in out_list[a.id]]
    if ck is None:
        env.set_agents(agents, obstacles=obstacles)

    def next_mission(agent, row):
        i = agent.id
        if int(row['flags']) & S.FLAG_COLLISION or not int(row['flags']) & S.FLAG_AT_GOAL:
            start, goal = first[i]
            back = False
        else:
            start = list(row['pos']) + list(agent.heading_global_frame)
            goal = list(agent.initial_pos)
            g, (s0, g0) = np.asarray(goal[:3], float), first[i]
            back = np.linalg.norm(g - np.asarray(s0[:3], float)) <= np.linalg.norm(g - np.asarray(g0[:3], float))
        new = E.Agent(start_pos=start, goal_pos=goal, vel=[0.0, 0.0, 0.0], radius=agent.radius, pref_speed=agent.pref_speed,
                      policy=type(agent.policy) if fleet else pol, id=i)          # (a mixed fleet: the drone keeps the policy it came with)
        if K:
            new.path = [w[:] for w in (back_list if back else out_list)[i]]
        return new

    t0 = time.time()
    if args.device_missions:
        # the same rule as a table of three entries per drone, taken on the device inside the step (MACAEnv.set_missions): from where it
        # stands to its start, from where it stands to its goal, and the original mission again as every failure's successor
        from sca_amd.lifelong import run_missions

        def entry(i, start, goal):
            a = agents[i]
            return E.Agent(start_pos=start, goal_pos=goal, vel=[0.0, 0.0, 0.0], radius=a.radius, pref_speed=a.pref_speed, policy=pol, id=i)
        tables = {i: E.MissionTable([entry(i, goal, start), entry(i, start, goal), entry(i, start, goal)], next_ok=[1, 0, 0], next_fail=[2, 2, 2],
                                    first_ok=0, first_fail=2, start_here=[True, True, False], path=[back_list[i], out_list[i], out_list[i]] if K else None)
                  for i, (start, goal) in first.items()}
        if args.resume:                                            # the env as --save-at left it; its tables stand, the run goes on for what is left
            from sca_amd.checkpoint import ContextCheckpoint
            ck = ContextCheckpoint.read(args.resume)
            env = E.MACAEnv.from_checkpoint(ck)
            stats = run_missions(env, None, args.lifelong - ck.steps, burst=args.burst)
        else:
            stats = run_missions(env, tables, args.lifelong, burst=args.burst, spawn_margin=args.spawn_margin,
                                 checkpoint_at=(args.save_at, args.save_file) if args.save_at else None)
            if args.save_at:
                print('saved behind step', args.save_at, 'as', args.save_file)
    elif args.traffic is not None:
        # a changing population: an arrived drone leaves the airspace (its row becomes vacant, MACAEnv.retire), and seeded arrivals -- a
        # Poisson number per step -- enter at vacant rows with those rows' original missions; with --spawn-margin only where the start is free
        import json
        from sca_amd.lifelong import RETIRE, resume_user_state
        trng = np.random.default_rng(2024)
        if ck is not None:                                         # the arrivals' generator and the per-policy lines go on where they were cut
            kept = json.loads(resume_user_state(ck))
            trng.bit_generator.state = kept['trng']
            per_policy.update(kept['per_policy'])

        def leave_or_restart(agent, row):
            f = int(row['flags'])
            if fleet:
                line_of(agent)['collided' if f & S.FLAG_COLLISION else 'arrived' if f & S.FLAG_AT_GOAL else 'timed_out'] += 1
            return RETIRE if f & S.FLAG_AT_GOAL and not f & S.FLAG_COLLISION else next_mission(agent, row)

        def arrivals(step, vacant_ids):
            k = min(len(vacant_ids), int(trng.poisson(args.traffic)))
            out = []
            for i in sorted(int(x) for x in trng.permutation(vacant_ids)[:k]):
                start, goal = first[i]
                old = env.agents[i]
                kind = fleet[int(trng.integers(len(fleet)))] if fleet else pol        # (seeded: the arrival's policy is drawn from --fleet)
                new = E.Agent(start_pos=start, goal_pos=goal, vel=[0.0, 0.0, 0.0], radius=old.radius, pref_speed=old.pref_speed, policy=kind, id=i)
                if K:
                    new.path = [w[:] for w in out_list[i]]
                out.append(new)
            return out
        stats = run_lifelong(env, leave_or_restart, args.lifelong - (ck.steps if ck is not None else 0), spawn_margin=args.spawn_margin, arrivals=arrivals,
                             checkpoint_at=(args.save_at, args.save_file) if args.save_at else None, resume=ck,
                             user_state=lambda: json.dumps(dict(trng=trng.bit_generator.state, per_policy=per_policy)))
        if args.save_at:
            print('saved behind step', args.save_at, 'as', args.save_file)
    else:
        stats = run_lifelong(env, next_mission, args.lifelong) if args.spawn_margin is None else \
            run_lifelong(env, next_mission, args.lifelong, spawn_margin=args.spawn_margin)
    cost = time.time() - t0
    missions = stats['arrived'] + stats['collided'] + stats['timed_out']
    print('lifelong:', stats['steps'], 'steps,', f'{cost:.2f} s,', missions, 'missions,', f'{missions / cost:.1f} missions/s')
    print({k: stats[k] for k in ('arrived', 'collided', 'timed_out', 'respawned', 'retired', 'agent_steps')}, f"live fraction {stats['live_fraction']:.3f}")
    if args.spawn_margin is not None:
        print('spawn margin', args.spawn_margin, 'm:', stats['deferred'], 'refusals,', stats['waiting'], 'missions still waiting')
    if args.traffic is not None:
        print('traffic', args.traffic, 'arrivals/step:', stats['retired_rows'], 'drones left,', stats['admitted'], 'entered, population',
              stats['population_min'], '..', stats['population_max'], f"(mean {stats['population_mean']:.1f})")
    for name in sorted(per_policy):
        print(f'  {name}:', per_policy[name]['entered'], 'entered,', per_policy[name]['arrived'], 'arrived,', per_policy[name]['collided'], 'collided')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenario', default='circle', choices=['circle', 'takeoff', 'exp3', 'sphere', 'random'])
    ap.add_argument('--agents', type=int, default=16)
    ap.add_argument('--policy', default='sca', choices=sorted(POLICIES))
    ap.add_argument('--no-obstacles', action='store_true')
    ap.add_argument('--map', default=None, help='binvox map for --scenario exp3')
    ap.add_argument('--max-steps', type=int, default=100000)
    ap.add_argument('--log-dir', default='visualization/sca/log')
    ap.add_argument('--tracker', default='host', choices=['host', 'device'],
                    help='where the Dubins v_pref tracker of SCA / RVO3D+Dubins runs: host = native threads, bit-exact against '
                         'the reference; device = kernels inside every step (large swarms)')
    ap.add_argument('--clearance', action='store_true',
                    help='keep every drone\'s closest approach to another drone and to an obstacle with the step, and print the minima')
    ap.add_argument('--margin', type=float, default=0.0, help='with --clearance: a drone whose smaller clearance is <= this counts as a near miss')
    ap.add_argument('--lifelong', type=int, default=0, metavar='STEPS',
                    help='continuous traffic for STEPS steps instead of one episode: a drone that arrives flies back, one that collided or '
                         'timed out starts again from its original start (MACAEnv.respawn; the Dubins tracker then runs on the device)')
    ap.add_argument('--spawn-margin', type=float, default=None, metavar='M',
                    help='with --lifelong: a drone is respawned only where its start is free by M metres (of every other drone, of every '
                         'obstacle and of the drones admitted with it); otherwise its mission waits and is offered again after every step '
                         '(with --device-missions the gate runs on the device too: MACAEnv.set_missions(spawn_margin=))')
    ap.add_argument('--traffic', type=float, default=None, metavar='RATE',
                    help='with --lifelong: a changing population -- a drone that arrives leaves the airspace (MACAEnv.retire), and a seeded '
                         'Poisson number of new drones, RATE per step on average, enters at vacant rows (with --spawn-margin only where free)')
    ap.add_argument('--fleet', default=None, metavar='P,P,...',
                    help='with --traffic: a mixed fleet -- every arriving drone draws its policy (seeded) from this comma-separated list of '
                         '--policy names and brings it into whatever row is vacant (MACAEnv(attribute_slots=True)); the summary gains a line per policy')
    ap.add_argument('--device-missions', action='store_true',
                    help='with --lifelong: the ping-pong rule as a mission table per drone on the device -- a drone that ends takes its next '
                         'mission inside the step, no host call per step (MACAEnv.set_missions)')
    ap.add_argument('--burst', type=int, default=1, metavar='K', help='with --device-missions: K resident steps per library call')
    ap.add_argument('--waypoints', type=int, default=0, metavar='K',
                    help='with --lifelong: every leg follows a route of K seeded waypoints, reversed on the way back (with --device-missions '
                         'the entries bring the routes: MissionTable(path=), sca_set_missions_paths)')
    ap.add_argument('--save-at', type=int, default=0, metavar='K', help='with --device-missions or --traffic: stop behind step K and write the running env '
                    '(MACAEnv.checkpoint: definition + sca_save_context; with --traffic the vacant rows and the host loop\'s state too) to --save-file')
    ap.add_argument('--save-file', default='run_sca_checkpoint.npz', metavar='F')
    ap.add_argument('--resume', default=None, metavar='F', help='with --lifelong S and --device-missions or --traffic: go on from the file --save-at wrote, up to step S '
                    '(MACAEnv.from_checkpoint); the last line is that of the run that was never cut')
    args = ap.parse_args()
    if (args.save_at or args.resume) and not (args.device_missions or args.traffic is not None):
        ap.error('--save-at / --resume go with --lifelong STEPS --device-missions or --lifelong STEPS --traffic RATE')
    if args.device_missions and args.lifelong <= 0:
        ap.error('--device-missions goes with --lifelong STEPS')
    if args.traffic is not None and (args.lifelong <= 0 or args.device_missions or args.traffic < 0):
        ap.error('--traffic RATE (RATE >= 0) goes with --lifelong STEPS, without --device-missions')
    if args.fleet is not None and (args.traffic is None or not args.fleet or any(name not in POLICIES for name in args.fleet.split(','))):
        ap.error('--fleet P,P,... (names of --policy) goes with --lifelong STEPS --traffic RATE')
    if args.waypoints < 0 or (args.waypoints and args.lifelong <= 0):
        ap.error('--waypoints K (K >= 0) goes with --lifelong STEPS')

    n = args.agents
    if args.scenario == 'circle':
        sc = scenarios.circle(n, rad=10.0 if n <= 16 else None)
        obstacles = [] if args.no_obstacles else build_obstacles()
    elif args.scenario == 'takeoff':
        sc = scenarios.takeoff_landing(n)
        obstacles = [] if args.no_obstacles else [E.Obstacle(pos=list(p), shape_dict={'shape': 'sphere', 'feature': float(r)}, id=j)
                                                  for j, (p, r) in enumerate(zip(sc['obs_pos'], sc['obs_radius']))]
    elif args.scenario == 'exp3':
        sc = scenarios.spawn_n_drones(n)
        obstacles = read_map.read_obstacle(center=(35, 30), environ='exp3', obs_path=args.map or 'visualization/map/map.binvox')
    elif args.scenario == 'sphere':
        sc = scenarios.sphere(n)
        obstacles = []
    else:
        sc = scenarios.random_cube(n)
        obstacles = []
    pol = POLICIES[args.policy]
    agents = [E.Agent(start_pos=list(sc['start'][i]), goal_pos=list(sc['goal'][i]), vel=[0.0, 0.0, 0.0], radius=0.5, pref_speed=1.0,
                      policy=pol, id=i) for i in range(n)]

    v_pref_fn = None
    dubins = pol in (E.SCAPolicy, E.RVO3dDubinsPolicy)          # these two follow a Dubins path (scaPolicy.py:264-338)
    if args.lifelong > 0:
        return lifelong(args, agents, obstacles, pol, dubins)
    if dubins and args.tracker == 'host':
        v_pref_fn = tracker.DubinsTracker(sc['goal'][:, :3], sc['goal'][:, 3:6], np.ones(n), S.zaxis_flags(sc['start'], sc['goal']))
    env = E.MACAEnv(v_pref_fn=v_pref_fn, history_capacity=args.max_steps, device_tracker=dubins and args.tracker == 'device', clearance=args.clearance)
    env.set_agents(agents, obstacles=obstacles)

    step, t0 = 0, time.time()
    while step < args.max_steps:
        done = env.step({})
        step += 1
        if done:
            break
    cost = time.time() - t0
    print('All agents finished!' if done else 'step limit reached', step, 'steps,', f'{cost:.2f} s')
    paths = metrics.write_episode_log(env, args.log_dir)                  # AverageCost from agent.total_time, as run_sca.py:241-250
    info = metrics.episode_metrics(env)
    print({k: info[k] for k in ('SuccessRate', 'ExtraTime', 'ExtraDistance', 'AverageSpeed', 'AverageCost')})
    if args.clearance:
        cm = metrics.clearance_metrics(env, args.margin)
        print({'MinClearance': cm['MinClearance'], 'MinClearancePair': cm['MinClearancePair'], 'MinClearanceStep': cm['MinClearanceStep'],
               'MinObstacleClearance': cm['MinObstacleClearance'], 'MinObstacleClearanceAgent': cm['MinObstacleClearanceAgent'],
               'MinObstacleClearanceObstacle': cm['MinObstacleClearanceObstacle'], 'MinObstacleClearanceStep': cm['MinObstacleClearanceStep'],
               'NearMisses': len(cm['NearMisses'])})
    print('wrote', ', '.join(sorted(paths.values())))


if __name__ == '__main__':
    main()
