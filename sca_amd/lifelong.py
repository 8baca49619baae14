"""Continuous traffic on one MACAEnv: drones land, new ones take off (MACAEnv.respawn / MACAEnv.finished).

    stats = run_lifelong(env, next_mission, steps, on_done=None, spawn_margin=None)

steps the env; whenever the number of running agents dropped it reads the finished rows from the device (sca_get_finished: only those
rows cross the link), hands each to on_done(agent, row) and respawns it with the Agent next_mission(agent, row) returns -- None retires
the agent, which then stays where it is for the rest of the run.  `row` is one record of _lib.FINISHED_DTYPE (id, flags, step_num,
total_dist, pos).

spawn_margin (metres): an admission gate in front of every respawn (MACAEnv.respawn(margin=), sca_respawn_agents_gated) -- a mission
whose start is not free by that margin WAITS: its row stays finished where it is, and the mission is offered again in front of every
later step, together with that step's new ones, waiting ones first, in ascending id.

A changing population (MACAEnv.retire, sca_retire_agents): next_mission may return lifelong.RETIRE -- the drone leaves the airspace, its
row becomes vacant and is nobody's neighbour or collision partner any more -- and arrivals(step, vacant_ids) -> [Agent] offers new drones
for vacant rows (Agent.id names the row) behind every step; they go through spawn_margin when it is set, and a refused arrival waits as a
refused mission does.

    stats = run_missions(env, tables, steps, burst=1, on_result=None, spawn_margin=None, checkpoint_at=None)

is the same traffic with the missions on the device (MACAEnv.set_missions, sca_set_missions): a row that ends takes its table's
successor inside the step, so the env is stepped in bursts of `burst` resident steps with one synchronisation each, and only the results
cross the link.  spawn_margin: the same admission gate on the device (MACAEnv.set_missions(spawn_margin=), sca_set_mission_gate), with
run_lifelong's offer order: the traffic is the host loop's under the same rule.

Interrupting such a run: run_missions(..., checkpoint_at=(step, path)) cuts the run at that step and writes the running env
(MACAEnv.checkpoint: the definition as plain arrays beside the library's blob, sca_save_context) as one .npz; MACAEnv.from_checkpoint
brings it back, in this or another process, and run_missions(env, None, the remaining steps) goes on with the standing tables and returns
the stats of the run that was never cut.

run_lifelong(..., checkpoint_at=(step, path)) cuts the host loop the same way, behind the whole iteration of that step -- its retire and
respawn calls included -- with vacant rows in the blob (sca_save_context_opt) and the loop's own state beside it as plain arrays: the
stats and traffic counters, the retired, vacant and arriving id sets, the waiting missions as the fields MACAEnv.respawn reads of an Agent,
and the string user_state() returns (the caller's rule: a generator's state, say).  run_lifelong(MACAEnv.from_checkpoint(ck), next_mission,
the remaining steps, ..., resume=ck) goes on and returns the stats of the run that was never cut; `arrivals` keeps seeing the run's step
numbers; resume_user_state(ck) hands the string back."""
import numpy as np

from . import solver as S

RETIRE = object()                                                # what next_mission returns for a drone that leaves the airspace (MACAEnv.retire)


_STAT_KEYS = ('steps', 'arrived', 'collided', 'timed_out', 'respawned', 'retired', 'agent_steps', 'deferred')
_TRAFFIC_KEYS = ('retired_rows', 'admitted', 'changing', 'pop_min', 'pop_max', 'pop_sum')


def _loop_state(stats, traffic, retired, vacant, arriving, waiting, active, user):
    """the host loop's state as plain arrays, under the `lifelong_` keys of a checkpoint's definition"""
    from . import scenes as _scenes
    ids = sorted(waiting)
    ents = [waiting[i] for i in ids]
    d = {'lifelong_stats': np.array([stats.get(k, 0) for k in _STAT_KEYS], np.int64), 'lifelong_traffic': np.array([int(traffic[k]) for k in _TRAFFIC_KEYS], np.int64),
         'lifelong_active': np.array([active], np.int64), 'lifelong_retired': np.array(sorted(retired), np.int32), 'lifelong_vacant': np.array(sorted(vacant), np.int32),
         'lifelong_arriving': np.array(sorted(arriving), np.int32), 'lifelong_waiting_ids': np.array(ids, np.int32),
         'lifelong_waiting_vel': np.array([a._vel for a in ents], np.float32).reshape(len(ents), 3),
         'lifelong_user': np.frombuffer(('' if user is None else str(user)).encode(), np.uint8).copy()}
    d.update({'lifelong_waiting_' + k: np.asarray(v) for k, v in _scenes.SceneCheckpoint.define(ents, [a._path for a in ents], []).items()})
    return d


def resume_user_state(ckpt):
    """the string user_state() returned at the cut ('' where there was none)"""
    return bytes(ckpt.definition['lifelong_user'].astype(np.uint8)).decode() if 'lifelong_user' in ckpt.definition else ''


def _loop_resume(ckpt):
    from . import scenes as _scenes
    d = ckpt.definition
    if 'lifelong_stats' not in d:
        raise ValueError('run_lifelong(resume=): the checkpoint was not written by run_lifelong(checkpoint_at=)')
    pre = 'lifelong_waiting_'
    ents = _scenes.SceneCheckpoint({k[len(pre):]: v for k, v in d.items() if k.startswith(pre) and k[len(pre):] not in ('ids', 'vel')}, np.zeros(0, np.uint8), 0).agents()
    for a, i, v in zip(ents, d[pre + 'ids'], d[pre + 'vel']):
        a.id, a._vel = int(i), np.array(v, np.float32)
    sets = [set(int(i) for i in d['lifelong_' + k]) for k in ('retired', 'vacant', 'arriving')]
    return ({k: int(v) for k, v in zip(_STAT_KEYS, d['lifelong_stats'])}, {k: int(v) for k, v in zip(_TRAFFIC_KEYS, d['lifelong_traffic'])}, sets,
            {a.id: a for a in ents}, int(d['lifelong_active'][0]))


def run_lifelong(env, next_mission, steps, on_done=None, spawn_margin=None, arrivals=None, checkpoint_at=None, resume=None, user_state=None):
    """Returns dict(steps, arrived, collided, timed_out: missions that ended that way (a collision wins over an arrival, an arrival over a
    time-out), respawned, retired, agent_steps: agents served summed over the steps, live_fraction: agent_steps / (agents x steps)).
    The run ends early when every agent is retired.  With spawn_margin the dict gains `deferred`, the refusals counted per attempt, and
    `waiting`, the missions still pending at the end: arrived + collided + timed_out == respawned + retired + waiting; the run then ends
    early too when nobody runs: the world is then still, and who waits would wait for ever.
    A changing population -- next_mission returned RETIRE at least once, or `arrivals` is given -- adds retired_rows (rows vacated: such an
    ending counts in `retired` too), admitted (arrivals that entered; not in `respawned`), arrivals_waiting (with spawn_margin: arrivals
    still refused at the end; `waiting` counts missions only) and population_min / population_max / population_mean over the steps.  With
    `arrivals` the run does not end early while nobody runs: the next arrival may change that.
    checkpoint_at=(step, path): behind the whole iteration of that step of the RUN the env (MACAEnv.checkpoint) and the loop's state are
    written to `path` as one .npz and the stats so far are returned.  resume=ckpt (ContextCheckpoint.read(path), with env =
    MACAEnv.from_checkpoint(ckpt)): the loop goes on where it was cut for `steps` more steps, with the same next_mission / on_done /
    spawn_margin / arrivals, and returns the stats of the run that was never cut.  user_state(): a string kept in the file for the caller
    (resume_user_state)"""
    n = len(env.agents)
    stats = dict(steps=0, arrived=0, collided=0, timed_out=0, respawned=0, retired=0, agent_steps=0, live_fraction=0.0)
    gated = spawn_margin is not None
    if gated:
        stats.update(deferred=0, waiting=0)
    retired = set()
    waiting = {}                                                 # id -> the Agent whose start was not free
    vacant = set(int(i) for i in env.vacant) if arrivals is not None else set()   # the vacant rows, followed here
    arriving = set()                                             # ids in `waiting` that are arrivals, not missions
    traffic = dict(retired_rows=0, admitted=0, changing=arrivals is not None, pop_min=n - len(vacant), pop_max=n - len(vacant), pop_sum=0)
    active = env._active
    if resume is not None:
        kept, tr, (retired, vacant, arriving), waiting, active = _loop_resume(resume)
        stats.update({k: v for k, v in kept.items() if k in stats})
        traffic.update(tr, changing=bool(tr['changing']))
    cut = None if checkpoint_at is None else int(checkpoint_at[0])
    for _ in range(int(steps)):
        if active == 0 and arrivals is None:
            break
        stats['agent_steps'] += active
        env.step()
        stats['steps'] += 1
        new, leaving = [], []
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
                elif nxt is RETIRE:
                    leaving.append(i)
                    stats['retired'] += 1
                else:
                    new.append(nxt)
        if leaving:                                              # (the last occupied row stays: a context keeps one)
            if len(leaving) >= n - len(vacant):
                retired.add(leaving.pop())
            if leaving:
                env.retire(leaving)
                vacant.update(leaving)
                traffic['retired_rows'] += len(leaving)
                traffic['changing'] = True
        if arrivals is not None:
            free = sorted(vacant - set(waiting))
            came = list(arrivals(stats['steps'], free)) if free else []
            arriving.update(int(a.id) for a in came)
            new = new + came
        if gated:
            offer = [waiting[i] for i in sorted(waiting)] + new  # the waiting ones first, in ascending id, then this step's new ones
            if offer:
                admitted = env.respawn(offer, margin=spawn_margin)
                stats['respawned'] += len(admitted)
                stats['deferred'] += len(offer) - len(admitted)
                waiting = {a.id: a for a in offer}
                for a in admitted:
                    del waiting[a.id]
                entered = [a.id for a in admitted if a.id in arriving]
                stats['respawned'] -= len(entered)               # (an arrival that entered is no mission taken)
                stats['deferred'] -= sum(1 for i in waiting if i in arriving)
                traffic['admitted'] += len(entered)
                vacant.difference_update(entered)
                arriving.difference_update(entered)
        elif new:
            env.respawn(new)
            entered = [a.id for a in new if a.id in arriving]
            stats['respawned'] += len(new) - len(entered)
            traffic['admitted'] += len(entered)
            vacant.difference_update(entered)
            arriving.difference_update(entered)
        active = env._active
        pop = n - len(vacant)
        traffic['pop_min'], traffic['pop_max'] = min(traffic['pop_min'], pop), max(traffic['pop_max'], pop)
        traffic['pop_sum'] += pop
        if cut is not None and stats['steps'] == cut:
            ck = env.checkpoint()
            ck.definition.update(_loop_state(stats, traffic, retired, vacant, arriving, waiting, active, user_state() if user_state is not None else None))
            ck.write(checkpoint_at[1])
            break
    if gated:
        stats['waiting'] = len(waiting) - len(arriving)
    if traffic['changing']:
        stats.update(retired_rows=traffic['retired_rows'], admitted=traffic['admitted'], population_min=traffic['pop_min'], population_max=traffic['pop_max'],
                     population_mean=traffic['pop_sum'] / float(stats['steps']) if stats['steps'] else float(n - len(vacant)))
        if gated:
            stats['arrivals_waiting'] = len(arriving)
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
