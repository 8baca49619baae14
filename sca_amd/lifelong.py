"""Continuous traffic on one MACAEnv: drones land, new ones take off (MACAEnv.respawn / MACAEnv.finished).

    stats = run_lifelong(env, next_mission, steps, on_done=None)

steps the env; whenever the number of running agents dropped it reads the finished rows from the device (sca_get_finished: only those
rows cross the link), hands each to on_done(agent, row) and respawns it with the Agent next_mission(agent, row) returns -- None retires
the agent, which then stays where it is for the rest of the run.  `row` is one record of _lib.FINISHED_DTYPE (id, flags, step_num,
total_dist, pos)."""
from . import solver as S


def run_lifelong(env, next_mission, steps, on_done=None):
    """Returns dict(steps, arrived, collided, timed_out: missions that ended that way (a collision wins over an arrival, an arrival over a
    time-out), respawned, retired, agent_steps: agents served summed over the steps, live_fraction: agent_steps / (agents x steps)).
    The run ends early when every agent is retired."""
    n = len(env.agents)
    stats = dict(steps=0, arrived=0, collided=0, timed_out=0, respawned=0, retired=0, agent_steps=0, live_fraction=0.0)
    retired = set()
    active = env._active
    for _ in range(int(steps)):
        if active == 0:
            break
        stats['agent_steps'] += active
        env.step()
        stats['steps'] += 1
        if env._active < active:                                 # somebody finished in this step
            new = []
            for row in env.finished():
                i = int(row['id'])
                if i in retired:
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
            if new:
                env.respawn(new)
                stats['respawned'] += len(new)
        active = env._active
    stats['live_fraction'] = stats['agent_steps'] / float(n * stats['steps']) if stats['steps'] else 0.0
    return stats
