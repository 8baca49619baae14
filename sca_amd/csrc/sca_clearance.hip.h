// sca_clearance.hip.h -- k_clearance: closest approach per agent for a whole context (sca_clearance_enable; the rule, the bound and the
// descent are sca_clearance.h's, the per-pair function is sca_scenes.h's clearance_pair).
//
// Enqueued by launch_collide_finish in front of the step's last kernel, only while the feature is on: d.rec_new holds the moved records,
// d.rec the records the step began with, d.awide / d.aperm the agent tree over the latter, d.owide / d.operm the obstacle tree.
// One wavefront per agent, as in collide_traverse: the stack is wave-uniform and lives in LDS (node and box distance per entry), node
// records come through the scalar path (a uniform index), a leaf's <= MAX_LEAF members are measured one per lane and reduced on (c, id)
// over the 16 lanes that can hold one.  Every store is the wavefront's own 32-byte record (lane 0, two 16-byte pieces); no atomics.
// The flags an agent ENTERED the step with: the policy epilogue of this step has already put a collision found by the neighbour
// insertion into d.rec (action_one), and K1 sets coll_new[a] for exactly those agents -- unflagged at entry -- and clears it for
// everybody else; so an agent entered unfinished where d.rec has no flag or coll_new[a] is set (k_scene_clearance reads the same).
#pragma once
#include "sca_kernels.hip.h"
#include "sca_clearance.h"

namespace sca {

constexpr int CLR_WAVES = 4;
static_assert(MAX_LEAF <= 16, "a leaf's members are reduced over 16 lanes");

// the Ops of clearance_descend on the device; Member(pos) -> (the partner's point, its id, whether it counts)
template <class Tree, class Member>
struct ClearDevOps {
    const Tree *tree;
    int *nstack;
    double *dstack;
    int lane;
    ClearPoint me;
    Member member;
    __device__ __forceinline__ Tree node(int i) const { return tree[__builtin_amdgcn_readfirstlane(i)]; }
    __device__ __forceinline__ ClearBest leaf(int begin, int end, double limit) const {
        ClearBest got = clearance_none();
        if (lane < end - begin) {
            ClearPoint p;
            int32_t id;
            if (member(begin + lane, p, id)) got = clearance_member(me, p, id, limit, L3Norm{});
        }
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {                               // lanes 0 .. 15 hold the members: four exchanges, lane 0 has the minimum
            const double oc = __shfl_xor(got.c, m);
            const int32_t oi = __shfl_xor(got.id, m);
            if (clearance_better(oc, oi, got.c, got.id)) { got.c = oc; got.id = oi; }
        }
        ClearBest r;
        r.c = readlane_f64(got.c, 0);
        r.id = __builtin_amdgcn_readlane(got.id, 0);
        return r;
    }
    __device__ __forceinline__ void push(int sp, int node, double dsq) const { if (lane == 0) { nstack[sp] = node; dstack[sp] = dsq; } }
    __device__ __forceinline__ void pop(int sp, int &node, double &dsq) const {
        __builtin_amdgcn_wave_barrier();
        node = __builtin_amdgcn_readfirstlane(nstack[sp]);
        dsq = dstack[sp];
    }
    __device__ __forceinline__ void skipped(int, double, double) const {}
};
template <class Tree, class Member>
__device__ __forceinline__ ClearDevOps<Tree, Member> clear_dev_ops(const Tree *tree, int *nstack, double *dstack, int lane, const ClearPoint &me, Member member) {
    return ClearDevOps<Tree, Member>{tree, nstack, dstack, lane, me, member};
}

// agent_reach = max_step + max_radius + 1e-4, obs_reach = max_obs_radius + 1e-4 (clearance_reach, beside collide_reach): the kernel adds
// the agent's own radius.  step: the context's env updates since the enable call, 1-based, from the host's counter.
__global__ __launch_bounds__(CLR_WAVES * 64) void k_clearance(DeviceView d, sca_scene_clearance *rec, double agent_reach, double obs_reach, int step) {
    __shared__ int nstack[CLR_WAVES][KD_STACK];
    __shared__ double dstack[CLR_WAVES][KD_STACK];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int agent = __builtin_amdgcn_readfirstlane((int)blockIdx.x * CLR_WAVES + wid);
    if (agent >= d.n) return;                                            // (wave-uniform)
    if ((d.rec[agent].flags & CLEAR_DONE_FLAGS) && !d.coll_new[agent]) return;   // entered finished: the record stays
    const PubRec mr = d.rec_new[agent];
    ClearPoint me; me.x = mr.px; me.y = mr.py; me.z = mr.pz; me.r = mr.radius;
    sca_scene_clearance r = rec[agent];
    int st = 0;
    bool changed = false;
    {
        auto ops = clear_dev_ops(d.awide, nstack[wid], dstack[wid], lane, me, [&](int pos, ClearPoint &p, int32_t &id) {
            id = d.aperm[pos];
            const PubRec q = d.rec_new[id];
            p.x = q.px; p.y = q.py; p.z = q.pz; p.r = q.radius;
            return id != agent;
        });
        ClearBest best = clearance_none();
        st |= clearance_descend(ops, 0, me.x, me.y, me.z, agent_reach + me.r, r.agent_clear, best, MAX_LEAF, KD_STACK, ST_KD_STACK);
        changed = clearance_commit(best, step, r.agent_clear, r.agent_partner, r.agent_step);
    }
    if (d.m > 0) {
        auto ops = clear_dev_ops(d.owide, nstack[wid], dstack[wid], lane, me, [&](int pos, ClearPoint &p, int32_t &id) {
            id = d.operm[pos];
            const ObsRec q = d.obs[id];
            p.x = q.px; p.y = q.py; p.z = q.pz; p.r = q.radius;
            return true;
        });
        ClearBest best = clearance_none();
        st |= clearance_descend(ops, 0, me.x, me.y, me.z, obs_reach + me.r, r.obs_clear, best, MAX_LEAF, KD_STACK, ST_KD_STACK);
        changed = clearance_commit(best, step, r.obs_clear, r.obs_partner, r.obs_step) || changed;
    }
    if (lane == 0) {
        if (changed) rec[agent] = r;
        if (st) d.status[agent] |= st;
    }
}

}  // namespace sca
