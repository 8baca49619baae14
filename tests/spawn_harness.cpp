// The pure rules of sca_amd/csrc/sca_spawn.h behind C entry points (tests/test_spawn_probe_cpu.py), and -- with -DSPAWN_MAIN -- as a
// program of its own for the sanitizers: every buffer on the heap in exactly the size the rules may touch.  The walk is the kernels' own:
// spn_probe stages each tile as k_spawn_probe does (ClearPoint plus id), lets every "lane" run spawn_tile_partial over each wavefront's
// slice, folds the slices, stores the one partial at [tile][query] and folds the tiles with spawn_fold; spn_gate runs spawn_gate_walk with
// 64 strided lanes per row and a ballot.  The tile size P is a parameter here (the library's is SPAWN_TILE): the result must not depend on it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sca_spawn.h"

using namespace sca;

namespace {

RespawnCtx ctx_of(const int *c) {
    RespawnCtx X;
    X.agents = c[0]; X.state = c[1]; X.mid_step = c[2]; X.scenes = c[3]; X.comm = c[4]; X.partition = c[5];
    X.n = c[6]; X.shard_count = c[7]; X.tracker_on = c[8]; X.paths_block = c[9]; X.path_W = c[10];
    X.policy_now = nullptr;
    return X;
}

// the probe of `count` queries packed in a block of exactly `count` queries' room, through partials of exactly tiles x count records
void probe(int n, const double *pos, const double *radius, int m, const double *obs_pos, const double *obs_radius, int count, const uint8_t *blk,
           const SpawnLayout &L, int P, sca_scene_clearance *out) {
    const int tiles = spawn_tiles(n, m, P), slice = (P + SPAWN_WAVES - 1) / SPAWN_WAVES;
    std::vector<SpawnPartial> partials((size_t)spawn_partials(n, m, count, P));
    const ClearPoint *query = (const ClearPoint *)(blk + L.off[SPB_QUERY]);
    const int32_t *ignore = (const int32_t *)(blk + L.off[SPB_IGNORE]);
    const int64_t total = (int64_t)n + m;
    for (int tile = 0; tile < tiles; tile++) {
        const int64_t g0 = (int64_t)tile * P;
        const int have = (int)(total - g0 < P ? total - g0 : P);
        std::vector<ClearPoint> pts((size_t)have);
        std::vector<int32_t> ids((size_t)have);
        for (int j = 0; j < have; j++) {
            const int64_t g = g0 + j;
            const double *p = g < n ? pos + 3 * g : obs_pos + 3 * (g - n);
            pts[(size_t)j] = ClearPoint{p[0], p[1], p[2], g < n ? radius[g] : obs_radius[g - n]};
            ids[(size_t)j] = spawn_partner_id(g, n);
        }
        for (int q = 0; q < count; q++) {
            SpawnPartial acc = spawn_partial_none();
            for (int wave = SPAWN_WAVES - 1; wave >= 0; wave--) {          // (any order: the last wavefront's slice first)
                SpawnPartial mine = spawn_partial_none();
                const int begin = wave * slice, end = begin + slice < have ? begin + slice : have;
                spawn_tile_partial(query[q], ignore[q], pts.data(), ids.data(), begin, end, g0, n, mine, L3Norm{});
                spawn_merge(acc, mine);
            }
            partials[(size_t)spawn_partial_index(tile, q, count)] = acc;
        }
    }
    for (int q = 0; q < count; q++) out[q] = spawn_fold(partials.data(), tiles, q, count);
}

}  // namespace

extern "C" {

int spn_tile() { return SPAWN_TILE; }
int spn_chunk() { return SPAWN_CHUNK; }
int spn_waves() { return SPAWN_WAVES; }
int spn_tiles(int n, int m, int P) { return spawn_tiles(n, m, P); }
long long spn_partial_index(int tile, int query, int cap) { return spawn_partial_index(tile, query, cap); }
void spn_layout(int cap, long long *off, long long *total) {
    const SpawnLayout L = spawn_layout(cap);
    for (int s = 0; s < SPB_SECTIONS; s++) off[s] = L.off[s];
    *total = L.total;
}
// out: fault, its code, entry
void spn_check(const int *c, int count, const double *pos, const double *radius, const int32_t *ignore, int have_out, int struct_bytes, int *out) {
    const SpawnCheck k = spawn_check(ctx_of(c), count, pos, radius, ignore, have_out != 0, struct_bytes);
    out[0] = k.fault; out[1] = spawn_error_code(k.fault); out[2] = k.entry;
}
void spn_gate_check(double margin, int have_verdict, int *out) {
    const SpawnFault f = spawn_gate_check(margin, have_verdict != 0);
    out[0] = f; out[1] = spawn_error_code(f);
}
void spn_probe(int n, const double *pos, const double *radius, int m, const double *obs_pos, const double *obs_radius, int count, const double *qpos,
               const double *qrad, const int32_t *ignore, int P, sca_scene_clearance *out) {
    const SpawnLayout L = spawn_layout(count);
    std::vector<uint8_t> blk((size_t)L.total);
    spawn_pack(blk.data(), L, count, qpos, qrad, ignore);
    probe(n, pos, radius, m, obs_pos, obs_radius, count, blk.data(), L, P, out);
}
// the gated call's rule: the world test of every row (ignore = its id), the world words, the entry test, the verdicts
void spn_gate(int n, const double *pos, const double *radius, int m, const double *obs_pos, const double *obs_radius, int count, const int32_t *ids,
              const double *qpos, const double *qrad, double margin, int P, sca_scene_clearance *out, int32_t *verdict) {
    const SpawnLayout L = spawn_layout(count);
    std::vector<uint8_t> blk((size_t)L.total);
    spawn_pack(blk.data(), L, count, qpos, qrad, ids);
    probe(n, pos, radius, m, obs_pos, obs_radius, count, blk.data(), L, P, out);
    std::vector<int32_t> world((size_t)count);
    for (int r = 0; r < count; r++) world[(size_t)r] = spawn_world(out[r], margin);
    const ClearPoint *rows = (const ClearPoint *)(blk.data() + L.off[SPB_QUERY]);
    for (int r = 0; r < count; r++) {
        unsigned long long ballot = 0;
        if (world[(size_t)r] == SCA_SPAWN_ADMITTED)
            for (int lane = 0; lane < 64; lane++) if (spawn_gate_walk(rows, world.data(), r, margin, lane, 64, L3Norm{})) ballot |= 1ull << lane;
        verdict[r] = spawn_verdict(world[(size_t)r], ballot != 0);
    }
}

}  // extern "C"

#ifdef SPAWN_MAIN
namespace {
double uni(double lo, double hi) { return lo + (hi - lo) * (std::rand() / (double)RAND_MAX); }
}
int main() {
    std::srand(7);
    long long checked = 0;
    const int sizes[] = {1, 2, 63, 64, 65, 300};
    for (int n : sizes) for (int m : {0, 1, 23}) for (int count : {1, 63, 64, 65, 257}) for (int P : {64, 512}) {
        std::vector<double> pos((size_t)3 * n), radius((size_t)n), opos((size_t)3 * m), orad((size_t)m), qpos((size_t)3 * count), qrad((size_t)count);
        std::vector<int32_t> ids((size_t)count);
        for (double &x : pos) x = uni(-6, 6);
        for (double &x : radius) x = uni(0.2, 1.0);
        for (double &x : opos) x = uni(-6, 6);
        for (double &x : orad) x = uni(0.2, 2.0);
        for (double &x : qpos) x = uni(-6, 6);
        for (double &x : qrad) x = uni(0.0, 1.0);
        for (int q = 0; q < count; q++) ids[(size_t)q] = q < n ? q : -1;
        std::vector<sca_scene_clearance> a((size_t)count), b((size_t)count);
        std::vector<int32_t> va((size_t)count), vb((size_t)count);
        spn_probe(n, pos.data(), radius.data(), m, opos.data(), orad.data(), count, qpos.data(), qrad.data(), nullptr, P, a.data());
        spn_gate(n, pos.data(), radius.data(), m, opos.data(), orad.data(), count, ids.data(), qpos.data(), qrad.data(), 0.5, P, b.data(), vb.data());
        spn_gate(n, pos.data(), radius.data(), m, opos.data(), orad.data(), count, ids.data(), qpos.data(), qrad.data(), 0.5, 2 * P + 1, a.data(), va.data());
        for (int q = 0; q < count; q++) {
            if (std::memcmp(&a[(size_t)q].agent_clear, &b[(size_t)q].agent_clear, 8) || a[(size_t)q].agent_partner != b[(size_t)q].agent_partner ||
                a[(size_t)q].obs_partner != b[(size_t)q].obs_partner || va[(size_t)q] != vb[(size_t)q]) { std::printf("spawn_harness: tile sizes disagree\n"); return 1; }
            if (m == 0 && (b[(size_t)q].obs_partner != -1 || !std::isinf(b[(size_t)q].obs_clear))) { std::printf("spawn_harness: an empty half is not empty\n"); return 1; }
            checked++;
        }
    }
    std::printf("spawn_harness: ok (%lld records)\n", checked);
    return 0;
}
#endif
