// Test-only: the host-side rules of the scene harvest (sca_amd/csrc/sca_scenes.h: scene_harvest_layout, scene_harvest_check,
// scene_harvest_order) behind a C interface for tests/test_scene_harvest_cpu.py.  Plain C++, no HIP.  Not part of the product (sca_amd never
// loads it).  With -DSCENE_HARVEST_MAIN it is a program of its own that walks the same functions over whole blocks, for a build under
// -fsanitize=address,undefined.
#include "sca_scenes.h"

using namespace sca;

extern "C" {

// out9: the eight section offsets and the total
void hv_layout(int nscenes, int n, int64_t *out9) {
    const HarvestLayout L = scene_harvest_layout(nscenes, n);
    for (int s = 0; s < HV_SECTIONS; s++) out9[s] = L.off[s];
    out9[HV_SECTIONS] = L.total;
}
int64_t hv_section_bytes(int s, int nscenes, int n) { return harvest_section_bytes(s, nscenes, n); }
// out3: sizeof(sca_scene_summary), sizeof(sca_scene_harvest), offsetof(sca_scene_harvest, counters)
void hv_struct_sizes(int *out3) { out3[0] = (int)sizeof(sca_scene_summary); out3[1] = (int)sizeof(sca_scene_harvest); out3[2] = (int)offsetof(sca_scene_harvest, counters); }
// out1: the fault.  Returns the error code the entry point gives for it.
int hv_check(int op, int nscenes, int scene_begun, int enabled, int have_out, int struct_bytes, int *out1) {
    const HarvestFault f = scene_harvest_check((HarvestOp)op, nscenes, scene_begun != 0, enabled != 0, have_out != 0, struct_bytes);
    out1[0] = f;
    return scene_harvest_error_code(f);
}
// summaries with the given fresh / batch_step words; ids[nscenes]; returns the count
int hv_order(int nscenes, const int32_t *fresh, const int32_t *batch_step, int32_t *ids) {
    std::vector<sca_scene_summary> sum((std::size_t)nscenes);
    for (int s = 0; s < nscenes; s++) { sum[s] = sca_scene_summary{}; sum[s].fresh = fresh[s]; sum[s].batch_step = batch_step[s]; }
    return scene_harvest_order(nscenes, sum.data(), ids);
}

}  // extern "C"

#ifdef SCENE_HARVEST_MAIN
#include <cstdio>
// Every byte a scene owns in the block -- its counters, its summary, its rows in every per-agent section -- is marked on an array of exactly
// the block's size (the sanitizer sees any byte outside it): no byte is owned twice, every section starts on its boundary, and the block of
// fewer agents lies inside the block of more.
static int walk(const std::vector<int32_t> &off) {
    const int B = (int)off.size() - 1, n = off[B];
    const HarvestLayout L = scene_harvest_layout(B, n);
    std::vector<uint8_t> owner((std::size_t)L.total, (uint8_t)0);
    const auto mark = [&](int64_t at, int64_t bytes) { for (int64_t b = at; b < at + bytes; b++) if (owner[(std::size_t)b]++) return false; return true; };
    for (int s = 0; s < HV_SECTIONS; s++) {
        if (L.off[s] % HV_ALIGN) return 1;
        const int64_t end = s + 1 < HV_SECTIONS ? L.off[s + 1] : L.total;
        if (L.off[s] + harvest_section_bytes(s, B, n) > end) return 2;
    }
    for (int sc = 0; sc < B; sc++) {
        if (!mark(L.off[HV_COUNTERS] + 8 * (int64_t)sc, 8)) return 3;
        if (!mark(L.off[HV_SUMMARY] + (int64_t)sizeof(sca_scene_summary) * sc, sizeof(sca_scene_summary))) return 4;
        for (int s = HV_POS; s < HV_SECTIONS; s++) {
            const int64_t row = harvest_section_bytes(s, B, 1);
            if (!mark(L.off[s] + row * off[sc], row * (off[sc + 1] - off[sc]))) return 5;       // the scene's rows at offsets[sc]
        }
    }
    const HarvestLayout M = scene_harvest_layout(B, n + 1000);
    for (int s = 0; s < HV_SECTIONS; s++) if (L.off[s] > M.off[s]) return 6;
    if (L.total > M.total) return 7;
    return 0;
}
static int order() {
    sca_scene_summary sum[6] = {};
    const int32_t fresh[6] = {1, 0, 1, 1, 0, 1}, step[6] = {7, 3, 2, 7, 1, 2};
    for (int s = 0; s < 6; s++) { sum[s].fresh = fresh[s]; sum[s].batch_step = step[s]; }
    int32_t ids[6] = {-1, -1, -1, -1, -1, -1};
    if (scene_harvest_order(6, sum, ids) != 4) return 1;
    const int32_t want[4] = {2, 5, 0, 3};
    for (int k = 0; k < 4; k++) if (ids[k] != want[k]) return 2;
    if (ids[4] != -1 || ids[5] != -1) return 3;
    sca_scene_summary none[3] = {};
    if (scene_harvest_order(3, none, ids) != 0) return 4;
    return 0;
}
int main() {
    int bad = walk({0, 3, 8, 10});
    if (!bad) bad = walk({0, 1}) ? 10 : 0;
    if (!bad) bad = walk({0, 1, 64, 129, 384, 641, 1000}) ? 20 : 0;
    if (!bad) bad = order() ? 30 + order() : 0;
    // 64 bits: 1024 scenes over 200 million rows, the positions alone pass 2^32 bytes
    if (!bad && scene_harvest_layout(1024, 200000000).off[HV_VEL] - scene_harvest_layout(1024, 200000000).off[HV_POS] != INT64_C(4800000000)) bad = 40;
    std::printf(bad ? "scene_harvest_harness: FAILED (%d)\n" : "scene_harvest_harness: ok\n", bad);
    return bad ? 1 : 0;
}
#endif
