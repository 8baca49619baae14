"""Continuous traffic on one MACAEnv: drones land, new ones take off (MACAEnv.respawn / MACAEnv.finished).

    stats = run_lifelong(env, next_mission, steps, on_done=None, spawn_margin=None)

steps the env; whenever the number of running agents dropped it reads the finished rows from the device (sca_get_finished: only those
rows cross the link), hands each to on_done(agent, row) and respawns it with the Agent next_mission(agent, row) returns -- None retires
the agent, which then stays where it is for the rest of the run.  `row` is one record of _lib.FINISHED_DTYPE (id, flags, step_num,
total_dist, pos).

spawn_margin (metres): an admission gate in front of every respawn (MACAEnv.respawn(margin=), sca_respawn_agents_gated) -- a mission
whose start is not free by that margin WAITS: its row stays finished where it is, and the mission is offered again in front of every
later step, together with that step's new ones, waiting ones first, in ascending id.

    stats = run_missions(env, tables, steps, burst=1, on_result=None, spawn_margin=None, checkpoint_at=None)

is the same traffic with the missions on the device (MACAEnv.set_missions, sca_set_missions): a row that ends takes its table's
successor inside the step, so the env is stepped in bursts of `burst` resident steps with one synchronisation each, and only the results
cross the link.  spawn_margin: the same admission gate on the device (MACAEnv.set_missions(spawn_margin=), sca_set_mission_gate), with
run_lifelong's offer order: the traffic is the host loop's under the same rule.

Interrupting such a run: run_missions(..., checkpoint_at=(step, path)) cuts the run at that step and writes the running env
(MACAEnv.checkpoint: the definition as plain arrays beside the library's blob, sca_save_context) as one .npz; MACAEnv.from_checkpoint
brings it back, in this or another process, and run_missions(env, None, the remaining steps) goes on with the standing tables and returns
the stats of the run that was never cut.  run_lifelong's host loop is out of scope for checkpoints: its waiting and retired sets are
Python objects of the caller's rule, which no blob can carry."""
from . import solver as S


def run_lifelong(env, next_mission, steps, on_done=None, spawn_margin=None):
    """Returns dict(steps, arrived, collided, timed_out: missions that ended that way (a collision wins over an arrival, an arrival over a
    time-out), respawned, retired, agent_steps: agents served summed over the steps, live_fraction: agent_steps / (agents x steps)).
    The run ends early when every agent is retired.  With spawn_margin the dict gains `deferred`, the refusals counted per attempt, and
    `waiting`, the missions still pending at the end: arrived + collided + timed_out == respawned + retired + waiting; the run then ends
    early too when nobody runs: the world is then still, and who waits would wait for ever."""
    n = len(env.agents)
    stats = dict(steps=0, arrived=0, collided=0, timed_out=0, respawned=0, retired=0, agent_steps=0, live_fraction=0.0)
    gated = spawn_margin is not None
    if gated:
        stats.update(deferred=0, waiting=0)
    retired = set()
    waiting = {}                                                 # id -> the Agent whose start was not free
    active = env._active
    for _ in range(int(steps)):
        if active == 0:
            break
        stats['agent_steps'] += active
        env.step()
        stats['steps'] += 1
        new = []
        if env._active < active:                                 # somebody finished in this step
            for row in env.finished():
                i = int(row['id'])
                if i in retired or i in waiting:
                    continue
                f = int(row['flags'])
                stats['collided' if f & S.FLAG_COLLISION else 'arrived' if f & S.FLAG_AT_GOAL else 'timed_out'] += 1
                agent = env.agents[i]
                if on_done is not None:
                    on_done(agent, row)
                nxt = next_mission(agent, row)
                if nxt is None:
                    retired.add(i)
                    stats['retired'] += 1
                else:
                    new.append(nxt)
        if gated:
            offer = [waiting[i] for i in sorted(waiting)] + new  # the waiting ones first, in ascending id, then this step's new ones
            if offer:
                admitted = env.respawn(offer, margin=spawn_margin)
                stats['respawned'] += len(admitted)
                stats['deferred'] += len(offer) - len(admitted)
                waiting = {a.id: a for a in offer}
                for a in admitted:
                    del waiting[a.id]
        elif new:
            env.respawn(new)
            stats['respawned'] += len(new)
        active = env._active
    if gated:
        stats['waiting'] = len(waiting)
    stats['live_fraction'] = stats['agent_steps'] / float(n * stats['steps']) if stats['steps'] else 0.0
    return stats


def run_missions(env, tables, steps, burst=1, on_result=None, spawn_margin=None, checkpoint_at=None):
    """tables: a dict from agent id to an env.MissionTable.  Steps the env in env.run_steps(burst) chunks and collects the results behind
    each chunk (on_result(agent, result) per result, a record of _lib.MISSION_RESULT_DTYPE).  Returns run_lifelong's stats keys from the
    device's totals: `respawned` the missions taken, `retired` the endings without a successor (such a row stays finished; the host may
    respawn it).  The run ends early, at a chunk's end, when nobody runs.  With spawn_margin the dict gains `deferred`, the refusals
    counted per attempt (offered - admitted), and `waiting`, the missions still pending at the end, as run_lifelong's does.
    tables=None: the run goes on with the tables that stand (an env from MACAEnv.from_checkpoint, or one an earlier call left), which are
    not set again: cursors, results and totals continue, and so do the stats -- the device's totals since the tables were set; whether
    `deferred` / `waiting` are reported then follows the standing gate.
    checkpoint_at=(step, path): the chunk is cut at that step of this call; behind it the results are collected, env.checkpoint() is
    written to `path` and the stats so far are returned.  MACAEnv.from_checkpoint(ContextCheckpoint.read(path)) and run_missions(env,
    None, the remaining steps) then return the stats of the run that was never cut."""
    n = len(env.agents)
    burst = max(1, int(burst))
    if tables is None:
        if env._missions is None:
            raise RuntimeError('run_missions(tables=None): no mission tables stand -- pass the tables')
    else:
        env.set_missions(tables, results=max(4, burst), spawn_margin=spawn_margin)
    gated = env._mission_gate
    cut = None if checkpoint_at is None else int(checkpoint_at[0])
    done = 0
    while done < int(steps) and env._active > 0:
        k = min(burst, int(steps) - done)
        if cut is not None and done < cut:
            k = min(k, cut - done)
        env.run_steps(k)
        done += k
        res = env.mission_results()
        if on_result is not None:
            for r in res:
                on_result(env.agents[int(r['id'])], r)
        if cut is not None and done == cut:
            env.checkpoint().write(checkpoint_at[1])
            break
    t = env.solver.mission_totals()
    stats = dict(steps=t['updates'], arrived=t['arrived'], collided=t['collided'], timed_out=t['timed_out'], respawned=t['taken'], retired=t['stopped'],
                 agent_steps=t['agent_steps'], live_fraction=0.0)
    if gated:
        g = env.solver.mission_gate_totals()
        stats.update(deferred=g['offered'] - g['admitted'], waiting=int((env.solver.mission_gate_state()[0] >= 0).sum()))
    stats['live_fraction'] = stats['agent_steps'] / float(n * stats['steps']) if stats['steps'] else 0.0
    return stats
