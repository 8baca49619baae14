"""Episode log of the reference's run scripts, produced from device state.

  * `episode_metrics(env)`  — SuccessRate / ExtraTime / ExtraDistance / AverageSpeed / AverageCost, the formulas of
    run_example/run_sca.py:223-251 (identical blocks in run_rvo.py, run_srvo.py, run_orca.py, run_rvodubins.py).
  * `episode_info(env)`     — the dict the reference dumps to `env_cfg.json` (run_sca.py:199-259), same keys and order, which
    visualization/draw_episode.py:17-32 reads (`all_agent_info`, `all_obstacle`).
  * `trajectories(env)`     — `agent.history_info` (agent.py:75-77,126-148): the 13 ANIMATION_COLUMNS per agent per env step,
    read back from the log the integrate kernel keeps in HBM (`sca_history_enable`), so a resident run needs no per-step
    readback.  For one scene of a SceneBatch (`batch.env(s)`) the rows come from the log per scene (`sca_scene_history_enable`).
  * `write_episode_log(env, dir)` — `env_cfg.json` + `trajs.npz` (one [rows, 13] array per agent under the reference's
    sheet name `agent<id>`); `trajs.xlsx` as well when openpyxl is importable (it is what the reference writes).

  * `clearance_metrics(view)` / `merge_clearance(before, after)` — how close the drones came (MinClearance, MinObstacleClearance,
    NearMisses) from the closest-approach records the device keeps with the step (`sca_scene_clearance_enable`; `batch.env(s).clearance`
    of a SceneBatch(clearance=True); `sca_clearance_enable`: `env.clearance` of a MACAEnv(clearance=True), any number of agents): the column the reference's table lacks, without an all-pairs search over the trajectory log.

AverageCost is the reference's wall time of find_next_action per agent-step (run_sca.py:250): by default the sum of
`agent.total_time`, which MACAEnv.step maintains (a step's policy wall time shared among the agents it served); a measured
total can be passed instead.
"""
import json
import os

import numpy as np

from .env import DT

ANIMATION_COLUMNS = ['pos_x', 'pos_y', 'pos_z', 'alpha', 'beta', 'gamma', 'vel_x', 'vel_y', 'vel_z',
                     'gol_x', 'gol_y', 'gol_z', 'radius']                                     # agent.py:75-76


def episode_metrics(env, total_policy_time_s=None):
    agents = env.agents
    n = len(agents)
    ok = np.array([(not a.is_collision) and (not a.is_out_of_max_time) for a in agents])
    num = int(ok.sum())
    # the reference accumulates in agent order with Python floats (run_sca.py:232-240): keep the same summation order
    straight = 0.0
    dist = 0.0
    desire = 0
    steps = 0
    for a, k in zip(agents, ok):
        if k:
            straight += a.straight_path_length
            dist += float(a.total_dist)
            desire += a.desire_steps
            steps += int(a.step_num)
    out = {
        'successful_num': num, 'all_straight_distance': straight, 'all_distance': dist, 'all_desire_step_num': desire,
        'all_step_num': steps, 'SuccessRate': num / n,
        'ExtraTime': ((steps - desire) * DT) / num if num else float('nan'),
        'ExtraDistance': (dist - straight) / num if num else float('nan'),
        'AverageSpeed': dist / steps / DT if steps else float('nan'),
    }
    if total_policy_time_s is None:                      # run_sca.py:241-250: sum of agent.total_time over the successful agents
        total_policy_time_s = sum(a.total_time for a, k in zip(agents, ok) if k)
    if steps:
        out['AverageCost'] = 1000 * total_policy_time_s / steps
    return out


def episode_metrics_from_harvest(agents, harvested, total_policy_time_s):
    """episode_metrics(batch.env(s)) -- same keys, same values -- from what the step that finished the scene handed over
    (SceneBatch.harvested(s)) instead of a read-back of the batch: successful_num, all_distance and all_step_num are the summary's (the
    device adds the distances in agent order, as the loop above does), the straight distances and the desired steps are the agents' host
    constants, masked by the harvested flags and summed in agent order.  total_policy_time_s: the episode's policy wall time (there is
    no agent.total_time without the batch's mirrors; scenes.run_episodes passes the same sum)."""
    from . import solver as S
    summary, flags = harvested['summary'], harvested['flags']
    n = len(agents)
    num = int(summary['successful_num'])
    straight = 0.0
    desire = 0
    for a, f in zip(agents, flags):
        if not (int(f) & (S.FLAG_COLLISION | S.FLAG_TIMEOUT)):
            straight += a.straight_path_length
            desire += a.desire_steps
    dist = float(summary['all_distance'])
    steps = int(summary['all_step_num'])
    out = {
        'successful_num': num, 'all_straight_distance': straight, 'all_distance': dist, 'all_desire_step_num': desire,
        'all_step_num': steps, 'SuccessRate': num / n,
        'ExtraTime': ((steps - desire) * DT) / num if num else float('nan'),
        'ExtraDistance': (dist - straight) / num if num else float('nan'),
        'AverageSpeed': dist / steps / DT if steps else float('nan'),
    }
    if steps:
        out['AverageCost'] = 1000 * total_policy_time_s / steps
    return out


def merge_clearance(before, after):
    """Two closest-approach records of the same agents (structured arrays in sca_scene_clearance's layout), `after` covering later steps
    than `before` -- a saved episode's record and the record of the slot it was resumed in.  Field by field, `after` wins only where it is
    strictly smaller: the earlier step keeps a tie, as it does on the device, so the result equals the uninterrupted run's.  Returns a new
    array."""
    before, after = np.asarray(before), np.asarray(after)
    if before.shape != after.shape or before.dtype != after.dtype:
        raise ValueError('merge_clearance: records of %s %s and %s %s' % (before.shape, before.dtype, after.shape, after.dtype))
    out = before.copy()
    for half in ('agent', 'obs'):
        later = after[half + '_clear'] < before[half + '_clear']
        for field in ('_clear', '_partner', '_step'):
            out[half + field][later] = after[half + field][later]
    return out


def clearance_metrics(view, margin=0.0):
    """How close an episode's drones came, from its closest-approach records: `view` is a scene view of a SceneBatch(clearance=True)
    (`batch.env(s)`: its `.clearance`), a MACAEnv(clearance=True) (the whole context's records, sca_clearance_enable: partners are agent
    ids and indices into the env's obstacle list, the step counts env.step() calls) or the structured array itself.  clearance = rounded distance - radius sum, the env's own collision
    test (mampenv.py:61-75), so a value <= 0 is a touch.  MinClearance with its pair (the agent that holds the record, its partner) and the
    scene's step; MinObstacleClearance with agent, obstacle (index in the scene's set) and step; on equal values the lowest agent.  An
    episode of one agent, or without obstacles, has +inf, None, 0 there.  NearMisses: the agents whose smaller clearance is <= margin."""
    rec = np.asarray(getattr(view, 'clearance', view))
    out = {'MinClearance': float('inf'), 'MinClearancePair': None, 'MinClearanceStep': 0,
           'MinObstacleClearance': float('inf'), 'MinObstacleClearanceAgent': None, 'MinObstacleClearanceObstacle': None, 'MinObstacleClearanceStep': 0}
    if len(rec) and np.isfinite(rec['agent_clear']).any():
        a = int(np.argmin(rec['agent_clear']))
        out.update(MinClearance=float(rec['agent_clear'][a]), MinClearancePair=(a, int(rec['agent_partner'][a])), MinClearanceStep=int(rec['agent_step'][a]))
    if len(rec) and np.isfinite(rec['obs_clear']).any():
        a = int(np.argmin(rec['obs_clear']))
        out.update(MinObstacleClearance=float(rec['obs_clear'][a]), MinObstacleClearanceAgent=a, MinObstacleClearanceObstacle=int(rec['obs_partner'][a]),
                   MinObstacleClearanceStep=int(rec['obs_step'][a]))
    out['NearMisses'] = [int(i) for i in np.flatnonzero(np.minimum(rec['agent_clear'], rec['obs_clear']) <= margin)]
    return out


def episode_info(env, total_policy_time_s=None, m=None):
    """The `info_dict_to_visualize` of run_sca.py:199-259.  m: the episode's metrics where the caller has them already
    (episode_metrics_from_harvest, with total_policy_time_s): nothing is read of the agents' state then."""
    if total_policy_time_s is None:                      # run_sca.py:241: all_compute_time sums agent.total_time
        ok = [(not a.is_collision) and (not a.is_out_of_max_time) for a in env.agents]
        total_policy_time_s = sum(a.total_time for a, k in zip(env.agents, ok) if k)
    if m is None:
        m = episode_metrics(env, total_policy_time_s)
    info = {
        'all_agent_info': [{'id': a.id, 'gp': a.group, 'radius': a.radius, 'goal_pos': np.asarray(a.goal_global_frame).tolist()}
                           for a in env.agents],
        'all_obstacle': [],
        'all_compute_time': float(total_policy_time_s),
        'all_straight_distance': m['all_straight_distance'],
        'all_distance': m['all_distance'],
        'successful_num': m['successful_num'],
        'all_desire_step_num': m['all_desire_step_num'],
        'all_step_num': m['all_step_num'],
        'SuccessRate': m['SuccessRate'],
        'ExtraTime': m['ExtraTime'],
        'ExtraDistance': m['ExtraDistance'],
        'AverageSpeed': m['AverageSpeed'],
        'AverageCost': m.get('AverageCost', 0.0),
    }
    for o in env.obstacles:
        info['all_obstacle'].append({'position': list(o.pos), 'shape': o.shape, 'feature': o.feature})
    return info


def trajectories(env, agent_begin=0, agent_count=None, rows=None):
    """[agents, rows, 13] array of the ANIMATION_COLUMNS, read from the device log (needs MACAEnv(history_capacity=...), or, for a scene view
    `batch.env(s)`, SceneBatch(scene_history=...): then the rows are that scene's own steps).  rows: the first `rows` logged rows, whether or not later steps were
    dropped (default: all of them, RuntimeError when steps were dropped)."""
    if rows is None:
        rows, dropped = env.solver.history_rows()
        if dropped:
            raise RuntimeError(f'{dropped} env steps did not fit the trajectory log: raise history_capacity')
    n = len(env.agents)
    if agent_count is None:
        agent_count = n - agent_begin
    h = env.solver.history(0, rows, agent_begin, agent_count)
    out = np.empty((agent_count, rows, len(ANIMATION_COLUMNS)))
    out[:, :, 0:3] = h['pos'].transpose(1, 0, 2)
    out[:, :, 3:6] = h['heading'].transpose(1, 0, 2)
    out[:, :, 6:9] = h['vel'].transpose(1, 0, 2)            # float32 values, as agent.vel_global_frame holds them
    out[:, :, 9:12] = env.goal[agent_begin:agent_begin + agent_count, None, :]
    out[:, :, 12] = np.array([a.radius for a in env.agents[agent_begin:agent_begin + agent_count]])[:, None]
    return out


def write_episode_log(env, log_dir, total_policy_time_s=None, xlsx=None):
    """Writes what run_sca.py:181-259 writes: the trajectories and env_cfg.json.  Returns the paths.  env: a MACAEnv, or one scene of a
    SceneBatch (`batch.env(s)`)."""
    return write_log_files(log_dir, env.agents, trajectories(env), episode_info(env, total_policy_time_s), xlsx)


def write_log_files(log_dir, agents, traj, info, xlsx=None):
    """The files of write_episode_log from their contents: traj [agents, rows, 13] (trajectories), info (episode_info).  What a caller
    that was handed both -- scenes.run_episodes(history_rows=...) -- writes an episode's folder with."""
    os.makedirs(log_dir, exist_ok=True)
    paths = {}
    paths['trajs'] = os.path.join(log_dir, 'trajs.npz')
    np.savez_compressed(paths['trajs'], columns=np.array(ANIMATION_COLUMNS),
                        **{'agent' + str(a.id): traj[i] for i, a in enumerate(agents)})
    if xlsx is None or xlsx:
        try:
            import openpyxl  # noqa: F401
            import pandas as pd
            paths['xlsx'] = os.path.join(log_dir, 'trajs.xlsx')
            with pd.ExcelWriter(paths['xlsx']) as writer:
                for i, a in enumerate(agents):
                    pd.DataFrame(traj[i], columns=ANIMATION_COLUMNS).to_excel(writer, sheet_name='agent' + str(a.id))
        except ImportError:
            if xlsx:
                raise
    paths['env_cfg'] = os.path.join(log_dir, 'env_cfg.json')
    with open(paths['env_cfg'], 'w') as f:
        f.write(json.dumps(info, indent=4))
    return paths


def read_trajs(path):
    """trajs.npz -> what draw_episode.get_agent_traj builds from the xlsx: list of {column: list} per agent, in file order."""
    z = np.load(path)
    cols = [str(c) for c in z['columns']]
    keys = sorted((k for k in z.files if k.startswith('agent')), key=lambda k: int(k[5:]))
    return [{c: z[k][:, j].tolist() for j, c in enumerate(cols)} for k in keys]
