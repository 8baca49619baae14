"""The closest-approach rule of include/sca_hip.h (sca_scene_clearance) restated in Python, for tests/test_scene_clearance_cpu.py and
tests/test_gpu_scene_clearance.py.  Nothing here calls the library.  The rounded norm is Python's round(math.sqrt(...), 5) per pair
(np.round is not correctly rounded and differs); numpy only finds, from the unrounded distances, the pairs that can be a step's minimum
-- the rounding moves a distance by at most 0.5e-5, so everything more than 2e-5 above the smallest unrounded value cannot win or tie."""
import math

import numpy as np

# struct sca_scene_clearance { double agent_clear, obs_clear; int32_t agent_partner, agent_step, obs_partner, obs_step; }: 32 bytes
DTYPE = np.dtype([('agent_clear', '<f8'), ('obs_clear', '<f8'), ('agent_partner', '<i4'), ('agent_step', '<i4'), ('obs_partner', '<i4'),
                  ('obs_step', '<i4')])
INF = float('inf')


def empty(n):
    out = np.zeros(n, DTYPE)
    out['agent_clear'] = INF
    out['obs_clear'] = INF
    out['agent_partner'] = -1
    out['obs_partner'] = -1
    return out


def l3norm(a, b):
    """util.py:104 on two points (Python floats)"""
    dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
    return round(math.sqrt(dx * dx + dy * dy + dz * dz), 5)


def _unrounded(p, q):
    """|p_i - q_j| for all pairs, the sum in l3norm's order"""
    d = p[:, None, :] - q[None, :, :]
    s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    s = s + d[..., 2] * d[..., 2]
    return np.sqrt(s)


def step_minimum(pa, ra, a, pts, radii, skip_self):
    """agent a against the partners (pts, radii), ascending: (the smallest c, the lowest partner that has it, how many have it); (inf, -1, 0)
    without partners"""
    if len(radii) == 0 or (skip_self and len(radii) == 1):
        return INF, -1, 0
    rs = ra + radii                                                # the radius sum first
    rough = _unrounded(pa[None, :], pts)[0] - rs
    if skip_self:
        rough[a] = INF
    best, who, ties = INF, -1, 0
    known = rough[~np.isnan(rough)]                                # (a partner at a NaN position has a NaN c, which is below nothing: `c < best`)
    if len(known) == 0:
        return INF, -1, 0
    for b in np.flatnonzero(rough <= known.min() + 2e-5):
        c = l3norm([float(x) for x in pa], [float(x) for x in pts[b]]) - float(rs[b])
        if c < best:
            best, who, ties = c, int(b), 1
        elif c == best:
            ties += 1
    return best, who, ties


def step(rec, pos, radius, entry_flags, obs_pos, obs_radius, step_no, count_ties=None):
    """One step of one scene, rec updated in place: pos (n, 3) the moved positions, entry_flags (n,) the flags the agents entered the step
    with, step_no the scene's own step count (1-based).  count_ties: a list that receives, per updated agent, (agent, the partners that
    share the step's agent minimum, that minimum, the step's obstacle minimum)."""
    n = len(radius)
    for a in range(n):
        if int(entry_flags[a]) & 7:
            continue
        c, who, ties = step_minimum(pos[a], float(radius[a]), a, pos, radius, True)
        if c < rec['agent_clear'][a]:
            rec['agent_clear'][a], rec['agent_partner'][a], rec['agent_step'][a] = c, who, step_no
        co, who, _ = step_minimum(pos[a], float(radius[a]), a, obs_pos.reshape(-1, 3), obs_radius, False)
        if co < rec['obs_clear'][a]:
            rec['obs_clear'][a], rec['obs_partner'][a], rec['obs_step'][a] = co, who, step_no
        if count_ties is not None:
            count_ties.append((a, ties, c, co))
    return rec


def whole_episode(fx):
    """a recorded episode whose records are its steps 0, 1, 2, ... from the start"""
    return int(fx['step'][0]) == 0 and np.array_equal(fx['step'], np.arange(len(fx['step']))) and np.array_equal(fx['pos'][0], fx['start'][:, :3])


def over_records(fx, upto=None, per_step=None, count_ties=None):
    """the rule over a recorded episode's records 0 .. upto - 1 (all of them): pos_after, the entry flags, the radii and the obstacles of the
    fixture; record k is the scene's step k + 1.  per_step(k, rec): called behind every record."""
    n = len(fx['radius'])
    rec = empty(n)
    for k in range(len(fx['step']) if upto is None else upto):
        if (fx['flags'][k] & 7).all():
            break                                                  # nobody live: the scene takes no step
        ties = [] if count_ties is not None else None
        step(rec, fx['pos_after'][k], fx['radius'], fx['flags'][k], fx['obs_pos'], fx['obs_radius'], k + 1, ties)
        if count_ties is not None:
            count_ties.extend((k,) + x for x in ties)
        if per_step is not None:
            per_step(k, rec)
    return rec
