// Test-only: the closest-approach descent of a whole context (sca_amd/csrc/sca_clearance.h: clearance_descend over clearance_member /
// clearance_pair, clearance_bound, clearance_check -- what k_clearance runs per wavefront) behind a C interface for
// tests/test_clearance_cpu.py.  Plain C++, no HIP.  Not part of the product (sca_amd never loads it).  The descent is run LANE BY LANE: a
// leaf's members go to lanes 0 .. 15, each lane measures its own with clearance_member, and the lanes are reduced on (c, id) by the same
// four exchanges as on the device.  Every child the descent skips is checked by brute force: no member of it may reach the value it was
// skipped against.  With -DCLEARANCE_MAIN it is a program of its own (trees of its own making, the all-pairs rule scene_clearance_step as
// the answer) on heap arrays of exactly the sizes the code may read, for a build under -fsanitize=address,undefined.
#include <vector>

#include "sca_core.h"
#include "sca_clearance.h"

using namespace sca;

namespace {

struct HNode { int begin, end, left, right; double bx[12]; };
// the query view of a tree given as 10 doubles per node (begin, end, left, right, mn[3], mx[3]: what sca_kd_build_host writes): node
// headers + both children's boxes in KdWide's layout
std::vector<HNode> widen(int count, const double *t10) {
    std::vector<HNode> w((size_t)(count > 0 ? 2 * count - 1 : 0));
    for (size_t i = 0; i < w.size(); i++) {
        const double *t = t10 + 10 * i;
        HNode &nd = w[i];
        nd.begin = (int)t[0]; nd.end = (int)t[1]; nd.left = (int)t[2]; nd.right = (int)t[3];
        for (double &b : nd.bx) b = 0.0;
        if (nd.end - nd.begin > MAX_LEAF)
            for (int side = 0; side < 2; side++) {
                const double *ch = t10 + 10 * (size_t)(side ? nd.right : nd.left);
                for (int k = 0; k < 3; k++) { nd.bx[(2 * k + 0) * 2 + side] = ch[4 + k]; nd.bx[(2 * k + 1) * 2 + side] = ch[7 + k]; }
            }
    }
    return w;
}

struct Stats { long long skipped = 0, violations = 0, visited = 0, leaves = 0, max_depth = 0; };

// the Ops of clearance_descend on the host: one wavefront's lanes, one after the other
struct HostOps {
    const std::vector<HNode> &tree;
    const int32_t *perm;
    const double *pts, *radii;          // the partners' points [count * 3] and radii, by id
    int self;                           // the id that is never a partner (-1: none)
    ClearPoint me;
    int stack_cap;
    std::vector<int> nstack;
    std::vector<double> dstack;
    Stats &S;
    ClearPoint point(int id) const { return ClearPoint{pts[3 * id], pts[3 * id + 1], pts[3 * id + 2], radii[id]}; }
    const HNode &node(int i) { S.visited++; return tree[(size_t)i]; }
    ClearBest leaf(int begin, int end, double limit) {
        S.leaves++;
        ClearBest lanes[16];
        for (int lane = 0; lane < 16; lane++) {
            lanes[lane] = clearance_none();
            if (lane < end - begin) {
                const int32_t id = perm[begin + lane];
                if (id != self) lanes[lane] = clearance_member(me, point(id), id, limit, L3Norm{});
            }
        }
        for (int m = 1; m < 16; m <<= 1) {
            ClearBest next[16];
            for (int lane = 0; lane < 16; lane++) {
                const ClearBest &o = lanes[lane ^ m];
                next[lane] = clearance_better(o.c, o.id, lanes[lane].c, lanes[lane].id) ? o : lanes[lane];
            }
            for (int lane = 0; lane < 16; lane++) lanes[lane] = next[lane];
        }
        return lanes[0];
    }
    void push(int sp, int node, double dsq) { nstack[(size_t)sp] = node; dstack[(size_t)sp] = dsq; if (sp + 1 > S.max_depth) S.max_depth = sp + 1; }
    void pop(int sp, int &node, double &dsq) { node = nstack[(size_t)sp]; dsq = dstack[(size_t)sp]; }
    // brute force: every member of a skipped child lies strictly above the value it was skipped against, and at or above the bound
    void skipped(int node, double, double limit) {
        S.skipped++;
        const HNode &nd = tree[(size_t)node];
        for (int i = nd.begin; i < nd.end; i++) {
            const int32_t id = perm[i];
            if (id == self) continue;
            const ClearPoint b = point(id);
            const double c = L3Norm{}(me.x, me.y, me.z, b.x, b.y, b.z) - (me.r + b.r);
            if (c <= limit) S.violations++;                                  // (a NaN position -- the edge family has some -- is nobody's partner under the rule)
        }
    }
};

// one step of the whole context: the descent per agent row in the agent tree (over the OLD positions; the partners' points are the moved
// ones) and in the obstacle tree
void descend_step(int n, const double *atree10, const int32_t *aperm, const double *pos_new, const double *radius, const uint32_t *entry_flags, int m,
                  const double *otree10, const int32_t *operm, const double *obs_pos, const double *obs_radius, double agent_reach, double obs_reach,
                  int step, int stack_cap, sca_scene_clearance *rec, int32_t *status, Stats &S) {
    const std::vector<HNode> aw = widen(n, atree10), ow = widen(m, otree10);
    for (int a = 0; a < n; a++) {
        if (entry_flags[a] & CLEAR_DONE_FLAGS) continue;
        const ClearPoint me = {pos_new[3 * a], pos_new[3 * a + 1], pos_new[3 * a + 2], radius[a]};
        sca_scene_clearance r = rec[a];
        int st = 0;
        {
            HostOps ops{aw, aperm, pos_new, radius, a, me, stack_cap, std::vector<int>((size_t)stack_cap), std::vector<double>((size_t)stack_cap), S};
            ClearBest best = clearance_none();
            st |= clearance_descend(ops, 0, me.x, me.y, me.z, agent_reach + me.r, r.agent_clear, best, MAX_LEAF, stack_cap, ST_KD_STACK);
            clearance_commit(best, step, r.agent_clear, r.agent_partner, r.agent_step);
        }
        if (m > 0) {
            HostOps ops{ow, operm, obs_pos, obs_radius, -1, me, stack_cap, std::vector<int>((size_t)stack_cap), std::vector<double>((size_t)stack_cap), S};
            ClearBest best = clearance_none();
            st |= clearance_descend(ops, 0, me.x, me.y, me.z, obs_reach + me.r, r.obs_clear, best, MAX_LEAF, stack_cap, ST_KD_STACK);
            clearance_commit(best, step, r.obs_clear, r.obs_partner, r.obs_step);
        }
        rec[a] = r;
        if (status) status[a] |= st;
    }
}

}  // namespace

extern "C" {

int clr_struct_bytes() { return (int)sizeof(sca_scene_clearance); }
int clr_max_leaf() { return MAX_LEAF; }
int clr_stack_bit() { return ST_KD_STACK; }
double clr_bound(double dist_sq, double reach) { return clearance_bound(dist_sq, reach); }
int clr_skips(double dist_sq, double reach, double best) { return clearance_skips(dist_sq, reach, best) ? 1 : 0; }
double clr_box_dist_sq(const double *bx, int side, double px, double py, double pz) { return clearance_box_dist_sq(bx, side, px, py, pz); }
// stats5: children skipped, members of skipped children that did not lie above the value (must stay 0), nodes loaded, leaves measured, the
// deepest stack
void clr_step(int n, const double *atree10, const int32_t *aperm, const double *pos_new, const double *radius, const uint32_t *entry_flags, int m,
              const double *otree10, const int32_t *operm, const double *obs_pos, const double *obs_radius, double agent_reach, double obs_reach, int step,
              int stack_cap, sca_scene_clearance *rec, int32_t *status, long long *stats5) {
    Stats S;
    descend_step(n, atree10, aperm, pos_new, radius, entry_flags, m, otree10, operm, obs_pos, obs_radius, agent_reach, obs_reach, step, stack_cap, rec, status, S);
    if (stats5) { stats5[0] += S.skipped; stats5[1] += S.violations; stats5[2] += S.visited; stats5[3] += S.leaves; if (S.max_depth > stats5[4]) stats5[4] = S.max_depth; }
}
// the all-pairs rule (sca_scenes.h), the context as one scene
void clr_all_pairs(int n, const double *pos_new, const double *radius, const uint32_t *entry_flags, int m, const double *obs_pos, const double *obs_radius, int step,
                   sca_scene_clearance *rec) {
    scene_clearance_step(n, pos_new, radius, entry_flags, m, obs_pos, obs_radius, step, rec, L3Norm{});
}
// state9: enabled, agents, state, mid_step, scenes, comm, partition, n, shard_count; out2: fault, the error code the entry points give for it
void clr_check(int call, const int *state9, int a, int b, int have_out, int struct_bytes, int *out2) {
    ClearanceState s;
    s.enabled = state9[0] != 0; s.agents = state9[1] != 0; s.state = state9[2] != 0; s.mid_step = state9[3] != 0; s.scenes = state9[4] != 0;
    s.comm = state9[5] != 0; s.partition = state9[6] != 0; s.n = state9[7]; s.shard_count = state9[8];
    const ClearanceFault f = clearance_check((ClearanceCall)call, s, a, b, have_out != 0, struct_bytes);
    out2[0] = f; out2[1] = clearance_error_code(f);
}

}  // extern "C"

#ifdef CLEARANCE_MAIN
#include <cstdio>
#include <cstring>
#include <memory>
// a kd-tree in the layout above (children at node + 1 and node + 2 * leftSize, leaves of at most MAX_LEAF, tight boxes), split at the
// middle of the longest axis by position rank: any tree of that shape serves the descent
static void build(const double *pos, int32_t *ids, int begin, int end, int node, double *t10) {
    double *t = t10 + 10 * (size_t)node;
    t[0] = begin; t[1] = end; t[2] = 0; t[3] = 0;
    for (int k = 0; k < 3; k++) { t[4 + k] = t[7 + k] = pos[3 * ids[begin] + k]; }
    for (int i = begin + 1; i < end; i++)
        for (int k = 0; k < 3; k++) { const double v = pos[3 * ids[i] + k]; if (v < t[4 + k]) t[4 + k] = v; if (v > t[7 + k]) t[7 + k] = v; }
    if (end - begin <= MAX_LEAF) return;
    int ax = 0;
    for (int k = 1; k < 3; k++) if (t[7 + k] - t[4 + k] > t[7 + ax] - t[4 + ax]) ax = k;
    for (int i = begin + 1; i < end; i++)                                   // insertion sort by the axis: the sizes here are small
        for (int j = i; j > begin && pos[3 * ids[j] + ax] < pos[3 * ids[j - 1] + ax]; j--) { const int32_t x = ids[j]; ids[j] = ids[j - 1]; ids[j - 1] = x; }
    const int left = (end - begin) / 2;
    t[2] = node + 1; t[3] = node + 2 * left;
    build(pos, ids, begin, begin + left, node + 1, t10);
    build(pos, ids, begin + left, end, node + 2 * left, t10);
}
static unsigned g_seed = 12345u;
static double draw(int cells) { g_seed = g_seed * 1664525u + 1013904223u; return (double)((g_seed >> 8) % (unsigned)cells); }
// n agents on a lattice of half metres (equal distances on purpose) that move by less than max_step per step, m obstacles; three steps of
// the descent against three steps of the all-pairs rule.  Every array has exactly the elements the code may read.
static int episode(int n, int m) {
    const double max_step = 0.3;
    std::unique_ptr<double[]> pos(new double[3 * (size_t)n]), moved(new double[3 * (size_t)n]), radius(new double[(size_t)n]);
    std::unique_ptr<uint32_t[]> flags(new uint32_t[(size_t)n]);
    std::unique_ptr<int32_t[]> perm(new int32_t[(size_t)n]), status(new int32_t[(size_t)n]);
    std::unique_ptr<double[]> tree(new double[10 * (size_t)(2 * n - 1)]);
    std::unique_ptr<double[]> opos(m ? new double[3 * (size_t)m] : nullptr), orad(m ? new double[(size_t)m] : nullptr), otree(m ? new double[10 * (size_t)(2 * m - 1)] : nullptr);
    std::unique_ptr<int32_t[]> operm(m ? new int32_t[(size_t)m] : nullptr);
    std::unique_ptr<sca_scene_clearance[]> got(new sca_scene_clearance[(size_t)n]), want(new sca_scene_clearance[(size_t)n]);
    for (int i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) pos[3 * i + k] = 0.5 * draw(16);
        radius[i] = i % 3 ? 0.25 : 0.5; flags[i] = i % 7 == 5 ? 2u : 0u; status[i] = 0;
        got[i] = want[i] = scene_clearance_empty();
    }
    for (int j = 0; j < m; j++) { for (int k = 0; k < 3; k++) opos[3 * j + k] = 0.5 * draw(16); orad[j] = j % 2 ? 1.0 : 0.5; operm[j] = j; }
    if (m) build(opos.get(), operm.get(), 0, m, 0, otree.get());
    Stats S;
    for (int step = 1; step <= 3; step++) {
        for (int i = 0; i < n; i++) perm[i] = i;
        build(pos.get(), perm.get(), 0, n, 0, tree.get());                    // the tree over the positions the step begins with
        for (int i = 0; i < 3 * n; i++) moved[i] = flags[i / 3] ? pos[i] : pos[i] + (draw(3) - 1.0) * 0.5 * max_step;   // |move| <= sqrt(3) / 2 * max_step
        descend_step(n, tree.get(), perm.get(), moved.get(), radius.get(), flags.get(), m, otree.get(), operm.get(), opos.get(), orad.get(),
                     max_step + 0.5 + 1e-4, 1.0 + 1e-4, step, 64, got.get(), status.get(), S);
        scene_clearance_step(n, moved.get(), radius.get(), flags.get(), m, opos.get(), orad.get(), step, want.get(), L3Norm{});
        if (std::memcmp(got.get(), want.get(), sizeof(sca_scene_clearance) * (size_t)n)) return 1;
        for (int i = 0; i < 3 * n; i++) pos[i] = moved[i];
    }
    for (int i = 0; i < n; i++) if (status[i]) return 2;
    return S.violations ? 3 : 0;
}
int main() {
    int bad = 0;
    const int cases[][2] = {{1, 0}, {1, 1}, {2, 0}, {10, 11}, {11, 1}, {63, 23}, {64, 0}, {65, 11}, {257, 23}};
    for (const auto &c : cases)
        if (!bad) { bad = episode(c[0], c[1]); if (bad) bad += 10 * c[0]; }
    std::printf(bad ? "clearance_harness: FAILED (%d)\n" : "clearance_harness: ok\n", bad);
    return bad ? 1 : 0;
}
#endif
