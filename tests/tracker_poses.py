"""Seeded pose families for the Dubins planner / tracker comparisons against the oracle's restatement (oracle/sca_dubins_oracle.c):
tests/test_oracle_tracker.py (the product's host planner) and tests/test_gpu_tracker_oracle.py (the device's re-plan kernels) draw
the same families.  Each family is where a planner goes wrong in a way the reference's few hundred recorded plans may not show:

  far       near-level 5 .. 40 km plans (the benchmark circle's geometry), dz exactly 0, 1e-14 .. 1e-9 m, and metres
  handover  3 .. 30 turning radii: where the lean search's far block gives way to the literal way
  steep     climbs and descents beyond the pitch limits: the pitch checks reject and the radius doubling runs
  zaxis     no horizontal offset (take-off / landing: is_zAxis, the horizontal problem of length 0); the goal heading never equals
            the start's (the reference's search does not end there)
  headings  yaw exactly 0, pi, just below 2 pi and 2 pi, along the line of sight (t or q = 0, alpha = beta), goals straight
            along an axis (the bearing exactly 0, pi / 2, pi)
  params    Rmin 0.8 / 1.5 / 3 / 10 with the pitch-limit pairs of tests/golden/F7c_dubins_kat_params.npz

poses(family, n, seed) -> dict(q=[n, 10] (qi[5] | qf[5]), rmin=[n], pitch_lo=[n], pitch_hi=[n]).
"""
import math

import numpy as np

FAMILIES = ('far', 'handover', 'steep', 'zaxis', 'headings', 'params')
PITCH_PAIRS = ((-math.pi / 4, math.pi / 4), (-math.pi / 6, math.pi / 6), (-0.5, 0.9), (-0.2, 0.2))
RMINS = (0.8, 1.5, 3.0, 10.0)
BELOW_2PI = float(np.nextafter(2 * np.pi, 0))


def _pair(rng, n, d, dz=None):
    """start poses around the origin, goals d away at a random bearing, dz above (default: level)"""
    p0 = rng.uniform(-50, 50, (n, 3)) + np.array([0.0, 0.0, 100.0])
    az = rng.uniform(0, 2 * np.pi, n)
    p1 = p0 + np.stack([d * np.cos(az), d * np.sin(az), np.zeros(n) if dz is None else dz], 1)
    return p0, p1, az


def poses(family, n, seed=0):
    rng = np.random.default_rng([FAMILIES.index(family), seed])
    rmin = np.full(n, 1.5)
    plo = np.full(n, -math.pi / 4)
    phi = np.full(n, math.pi / 4)
    yaw0 = rng.uniform(0, 2 * np.pi, n)
    yaw1 = rng.uniform(0, 2 * np.pi, n)
    pit0 = rng.uniform(-0.2, 0.2, n)
    pit1 = np.zeros(n)
    if family == 'far':
        d = rng.uniform(5000.0, 40000.0, n)
        dz = rng.choice([0.0, 1e-14, -3e-14, 2e-12, 1e-9, 0.5, -3.0, 25.0], n)
        p0, p1, az = _pair(rng, n, d, dz)
        # most of them fly roughly towards the goal, level, as the circle's agents do
        near = rng.random(n) < 0.7
        yaw0[near] = np.mod(az[near] + rng.normal(0, 0.2, near.sum()), 2 * np.pi)
        yaw1[near] = np.mod(az[near] + rng.normal(0, 0.05, near.sum()), 2 * np.pi)
        pit0[near] = rng.choice([0.0, 1e-9, -1e-7, 0.01], near.sum())
    elif family == 'handover':
        d = 1.5 * rng.uniform(3.0, 30.0, n)
        p0, p1, _ = _pair(rng, n, d, rng.uniform(-3, 3, n) * (rng.random(n) < 0.5))
        pit1 = rng.uniform(-0.1, 0.1, n)
    elif family == 'steep':
        d = 1.5 * 10 ** rng.uniform(0.3, 2.5, n)
        slope = np.tan(rng.uniform(0.6, 1.45, n)) * rng.choice([-1.0, 1.0], n)
        p0, p1, _ = _pair(rng, n, d, d * slope)
        p0[:, 2] += 500.0
        p1[:, 2] += 500.0
        pit0 = rng.uniform(-0.7, 0.7, n)
    elif family == 'zaxis':
        p0 = rng.uniform(-50, 50, (n, 3))
        p1 = p0.copy()
        p1[:, 2] += rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 40.0, n)
        # half of them as run_sca.py's take-off / landing cell: +-round(pi / 2, 5), the goal turned by pi (with the goal's heading
        # EQUAL to the start's the reference's radius doubling never ends: every horizontal word is a full circle)
        c5 = rng.random(n) < 0.5
        yaw0[c5] = rng.choice([round(np.pi / 2, 5), round(-np.pi / 2, 5)], c5.sum())
        yaw1[c5] = -yaw0[c5]
        pit0 = np.zeros(n)
    elif family == 'headings':
        d = 1.5 * 10 ** rng.uniform(0.5, 4.0, n)
        p0, p1, az = _pair(rng, n, d, rng.choice([0.0, 0.0, 1.0, -2.0], n))
        axis = rng.random(n) < 0.25                                  # goal straight along +x / -x / +y: the bearing exactly 0, pi, pi/2
        p1[axis, :2] = p0[axis, :2] + d[axis, None] * np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0]])[rng.integers(0, 3, axis.sum())]
        special = np.array([0.0, np.pi, BELOW_2PI, 2 * np.pi])
        yaw0 = rng.choice(special, n)
        yaw1 = rng.choice(special, n)
        los = rng.random(n) < 0.4                                    # along the line of sight: alpha = beta = 0
        bearing = np.mod(np.arctan2(p1[:, 1] - p0[:, 1], p1[:, 0] - p0[:, 0]), 2 * np.pi)
        yaw0[los] = bearing[los]
        yaw1[los] = bearing[los]
        same = rng.random(n) < 0.2                                   # alpha = beta off the line of sight
        yaw1[same] = yaw0[same]
        pit0 = rng.choice([0.0, 0.0, 0.1, -0.1], n)
    else:                                                            # params
        rmin = rng.choice(np.array(RMINS), n)
        pr = np.array(PITCH_PAIRS)[rng.integers(0, len(PITCH_PAIRS), n)]
        plo, phi = pr[:, 0].copy(), pr[:, 1].copy()
        d = rmin * 10 ** rng.uniform(-0.3, 2.2, n)
        dz = d * np.tan(rng.uniform(-1.0, 1.0, n)) * (rng.random(n) < 0.6)
        p0, p1, _ = _pair(rng, n, d, dz)
        pit0 = rng.uniform(plo, phi) * (rng.random(n) < 0.5)
        pit1 = rng.uniform(plo, phi) * (rng.random(n) < 0.3)
    q = np.concatenate([p0, yaw0[:, None], pit0[:, None], p1, yaw1[:, None], pit1[:, None]], 1)
    return dict(q=np.ascontiguousarray(q), rmin=rmin, pitch_lo=plo, pitch_hi=phi)


def tracker_inputs(P):
    """The first compute_v_pref of a tracker whose agent i stands at pose qi, headed for qf: (pos, heading, goal, goal_heading)
    (heading / goal heading = [yaw, pitch, 0], as agent.py keeps them)"""
    q = P['q']
    n = len(q)
    z = np.zeros((n, 1))
    return (np.ascontiguousarray(q[:, 0:3]), np.ascontiguousarray(np.concatenate([q[:, 3:5], z], 1)),
            np.ascontiguousarray(q[:, 5:8]), np.ascontiguousarray(np.concatenate([q[:, 8:10], z], 1)))
