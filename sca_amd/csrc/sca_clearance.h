// sca_clearance.h -- closest approach per agent for a whole context, by kd-tree descent (sca_clearance_enable, include/sca_hip.h).
//
// The rule is the scene rule (sca_scenes.h: clearance_pair, sca_scene_clearance) with the context as the one "scene": agent a, at every
// step it ENTERED unfinished, keeps the smallest c = l3norm(p_a, p_b) - (r_a + r_b) over every other agent b (the moved positions, whatever
// b's flags), the lowest b on equal values, replacing its record only where strictly smaller; the same over the obstacles in set order.
// What differs is the search: not all pairs, but a descent of the trees the step already has -- the agent tree over the positions the
// step BEGAN with (d.awide / d.aperm) and the static obstacle tree (d.owide / d.operm).
//
// Everything here is pure and compiles for the host (tests/clearance_harness.cpp runs the very same descent lane by lane):
//   clearance_bound    the least c any member of a box can give
//   clearance_descend  the descent, a template over "load node", "measure a leaf's members and reduce", "push / pop" and "skipped"
//   clearance_member   one lane's member of a leaf (clearance_pair, the scene rule's own per-pair function)
//   clearance_better   the lexicographic order on (c, id) a step's candidate is reduced with
//   clearance_check    every refusal of the feature, with its code
#pragma once
#include "sca_scenes.h"

namespace sca {

// ---- the bound ---------------------------------------------------------------------------------------------------------------------------
// A box B of the agent tree encloses the positions its members had when the step began; a member b has moved by at most max_step since
// (collide_reach's max_step: 1.01 x the largest speed x dt_nominal; a finished agent has not moved at all).  With p'_a the moved position
// of a:  |p'_a - p'_b| >= |p'_a - p_b| - |p_b - p'_b| >= dist(p'_a, B) - max_step, the rounded norm is at most 0.5e-5 below the true one,
// and r_b <= max_radius, hence
//     c(a, b) >= dist(p'_a, B) - max_step - r_a - max_radius - 1e-4            reach = max_step + r_a + max_radius + 1e-4
// (the 1e-4 covers the 5-decimal rounding and the rounding of dist itself, as in collide_reach).  The obstacle tree is static: its reach
// is r_a + max_obs_radius + 1e-4.  dist_sq is box_dist_sq's sum (kdTree.py:132-145).
SCA_SCENES_HD double clearance_bound(double dist_sq, double reach) { return __builtin_sqrt(dist_sq) - reach; }
// A child is skipped only where its bound is STRICTLY above the best value so far: a member with an equal value and a lower id must
// still be found.  best == +inf never skips.
SCA_SCENES_HD bool clearance_skips(double dist_sq, double reach, double best) { return clearance_bound(dist_sq, reach) > best; }

// squared distance from p to the box of child `side` of a node record in KdWide's layout: bx[(2 * axis + is_max) * 2 + side], the six
// terms in kdTree.py's order
SCA_SCENES_HD double clearance_box_dist_sq(const double *bx, int side, double px, double py, double pz) {
    const double p[3] = {px, py, pz};
    double s = 0.0;
    for (int k = 0; k < 3; k++) {
        double t = bx[(2 * k + 0) * 2 + side] - p[k];
        t = t > 0.0 ? t : 0.0;
        s = s + t * t;
        t = p[k] - bx[(2 * k + 1) * 2 + side];
        t = t > 0.0 ? t : 0.0;
        s = s + t * t;
    }
    return s;
}

// ---- a step's candidate: the smallest c of the step so far and the lowest partner that has it -----------------------------------------------
struct ClearBest { double c; int32_t id; };
constexpr int32_t CLEAR_NO_ID = 0x7fffffff;
SCA_SCENES_HD ClearBest clearance_none() { ClearBest b; b.c = __builtin_huge_val(); b.id = CLEAR_NO_ID; return b; }
SCA_SCENES_HD bool clearance_better(double c1, int32_t id1, double c2, int32_t id2) { return c1 < c2 || (c1 == c2 && id1 < id2); }
// One lane's member: c where it can still matter, else (+inf, CLEAR_NO_ID).  `limit` is the smaller of the row's record and the step's
// candidate; clearance_pair takes the exact rounding only for a pair that can come below limit + 1e-5, so every pair at or below the
// limit -- an equal value with a lower id among them -- is measured exactly, and what lies above it loses the reduction anyway.
template <class Norm>
SCA_SCENES_HD ClearBest clearance_member(const ClearPoint &a, const ClearPoint &b, int32_t id, double limit, Norm norm) {
    double c = limit + 1e-5;
    int32_t who = -1, when = 0;
    clearance_pair(a, b, id, 0, c, who, when, norm);
    ClearBest r = clearance_none();
    if (who >= 0) { r.c = c; r.id = who; }
    return r;
}

// ---- the descent -------------------------------------------------------------------------------------------------------------------------
// Nearest child first; the bound shrinks as the descent goes and starts at the row's own record, so a step in which nobody can beat the
// record ends at the root.  A deferred child is kept with its box distance and tested again when it is popped: the bound has shrunk
// since it was pushed.  Ops:
//   node(i)                 the node record: .begin .end .left .right and .bx[12] (KdWide's layout, both children's boxes)
//   leaf(begin, end, limit) measures the members at tree positions begin .. end - 1 (one per lane) and returns their (c, id) minimum
//   push(sp, node, dsq) / pop(sp, node, dsq)   the wave-uniform stack, at most stack_cap deep
//   skipped(node, dsq, limit)                  a child that was pruned (the host's brute-force check of the bound; nothing on the device)
// Returns ST_KD_STACK's bit (status_overflow) where a push found the stack full -- never silently.
template <class Ops>
SCA_SCENES_HD int clearance_descend(Ops &ops, int root, double px, double py, double pz, double reach, double record, ClearBest &best, int max_leaf,
                                    int stack_cap, int status_overflow) {
    int sp = 0, st = 0, node = root;
    bool have = true;
    while (have) {
        const auto nd = ops.node(node);
        have = false;
        double limit = record < best.c ? record : best.c;
        if (nd.end - nd.begin <= max_leaf) {
            const ClearBest got = ops.leaf(nd.begin, nd.end, limit);
            if (clearance_better(got.c, got.id, best.c, best.id)) best = got;
        } else {
            const double dl = clearance_box_dist_sq(nd.bx, 0, px, py, pz), dr = clearance_box_dist_sq(nd.bx, 1, px, py, pz);
            int first, second;
            double dfirst, dsecond;
            if (dl < dr) { first = nd.left; second = nd.right; dfirst = dl; dsecond = dr; }
            else { first = nd.right; second = nd.left; dfirst = dr; dsecond = dl; }
            if (clearance_skips(dsecond, reach, limit)) ops.skipped(second, dsecond, limit);
            if (clearance_skips(dfirst, reach, limit)) ops.skipped(first, dfirst, limit);
            else {
                if (!clearance_skips(dsecond, reach, limit)) {
                    if (sp < stack_cap) { ops.push(sp, second, dsecond); sp++; }
                    else st |= status_overflow;
                }
                node = first;
                have = true;
            }
        }
        while (!have && sp > 0) {
            double dsq;
            sp--;
            ops.pop(sp, node, dsq);
            limit = record < best.c ? record : best.c;
            if (clearance_skips(dsq, reach, limit)) ops.skipped(node, dsq, limit);
            else have = true;
        }
    }
    return st;
}
// the step's candidate against one half of the record: strictly smaller only, so the earliest step keeps a tie
SCA_SCENES_HD bool clearance_commit(const ClearBest &best, int step, double &clear, int32_t &who, int32_t &when) {
    if (!(best.c < clear)) return false;
    clear = best.c; who = best.id; when = step;
    return true;
}

// ---- the refusals ------------------------------------------------------------------------------------------------------------------------
enum ClearanceCall {
    CLR_ENABLE = 0,         // sca_clearance_enable(on != 0)
    CLR_DISABLE,            // sca_clearance_enable(0)
    CLR_GET,                // sca_get_clearance: a = agent_begin, b = agent_count
    CLR_PASS,               // a policy pass or a step about to be enqueued: a = its neighbour mode
    CLR_UPDATE,             // sca_env_update: a = 1 where a policy pass opened the step, b = 1 where that pass searched the grid alone
    CLR_SET_SHARD,          // sca_set_shard: a = count
    CLR_COMM_INIT, CLR_PARTITION_INIT, CLR_SET_SCENES
};
struct ClearanceState {
    bool enabled;           // the records exist
    bool agents, state;     // sca_set_agents / a state has been given
    bool mid_step;          // between a policy pass and its env update
    bool scenes, comm, partition;
    int n, shard_count;
};
enum ClearanceFault {
    CLRF_OK = 0,
    CLRF_NO_AGENTS,         // enable: no agents yet                                                          } SCA_ERR_STATE
    CLRF_NO_STATE,          // enable: no state yet                                                           }
    CLRF_MID_STEP,          // enable / disable between a policy pass and its env update                      }
    CLRF_OFF,               // get: the feature is not enabled                                                }
    CLRF_RANGE,             // get: agent_begin / agent_count outside 0 .. n                                  } SCA_ERR_ARG
    CLRF_NO_OUT,            // get: out is NULL                                                               }
    CLRF_BAD_STRUCT,        // get: struct_bytes is not sizeof(sca_scene_clearance)                           }
    CLRF_SCENES,            // enable with scenes set; sca_set_scenes while on                                } SCA_ERR_UNSUPPORTED
    CLRF_SHARD,             // enable on a shard with count < n; sca_set_shard(count < n) while on            }
    CLRF_COMM,              // enable with a communicator; sca_comm_init while on                             }
    CLRF_PARTITION,         // enable under the cell-owner partition; sca_partition_init while on             }
    CLRF_GRID_PASS,         // while on: a pass in SCA_NBR_GRID mode -- no agent tree of this step            }
    CLRF_NO_PASS            // while on: an env update without a policy pass -- no agent tree of this step    }
};
inline ClearanceFault clearance_check(ClearanceCall call, const ClearanceState &s, int a, int b, bool have_out, int struct_bytes) {
    switch (call) {
    case CLR_ENABLE:
    case CLR_DISABLE:
        if (!s.agents) return CLRF_NO_AGENTS;
        if (!s.state) return CLRF_NO_STATE;
        if (s.mid_step) return CLRF_MID_STEP;
        if (call == CLR_DISABLE) return CLRF_OK;
        if (s.scenes) return CLRF_SCENES;
        if (s.comm) return CLRF_COMM;
        if (s.partition) return CLRF_PARTITION;
        if (s.shard_count < s.n) return CLRF_SHARD;
        return CLRF_OK;
    case CLR_GET:
        if (!s.enabled) return CLRF_OFF;
        if (a < 0 || b < 0 || a > s.n || b > s.n - a) return CLRF_RANGE;
        if (!have_out) return CLRF_NO_OUT;
        if (struct_bytes != (int)sizeof(sca_scene_clearance)) return CLRF_BAD_STRUCT;
        return CLRF_OK;
    case CLR_PASS: return s.enabled && a == SCA_NBR_GRID ? CLRF_GRID_PASS : CLRF_OK;
    case CLR_UPDATE: return !s.enabled ? CLRF_OK : !a ? CLRF_NO_PASS : b ? CLRF_GRID_PASS : CLRF_OK;
    case CLR_SET_SHARD: return s.enabled && a < s.n ? CLRF_SHARD : CLRF_OK;
    case CLR_COMM_INIT: return s.enabled ? CLRF_COMM : CLRF_OK;
    case CLR_PARTITION_INIT: return s.enabled ? CLRF_PARTITION : CLRF_OK;
    case CLR_SET_SCENES: return s.enabled ? CLRF_SCENES : CLRF_OK;
    }
    return CLRF_OK;
}
inline int clearance_error_code(ClearanceFault f) { return f == CLRF_OK ? SCA_OK : f <= CLRF_OFF ? SCA_ERR_STATE : f <= CLRF_BAD_STRUCT ? SCA_ERR_ARG : SCA_ERR_UNSUPPORTED; }

}  // namespace sca
