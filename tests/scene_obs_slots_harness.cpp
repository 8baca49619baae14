// tests/scene_obs_slots_harness.cpp -- the host-side rules of obstacle slots (sca_set_scene_obstacle_slots, sca_restart_scenes_obstacles;
// sca_scenes.h) behind tests/test_scene_obs_slots_cpu.py.  Plain C++, no HIP.  Not part of the library.  With -DSCENE_OBS_SLOTS_MAIN it is
// a program of its own, for a build under -fsanitize=address,undefined: its main walks the same rules on heap arrays of exactly the sizes
// the rules may read.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "sca_scenes.h"

using namespace sca;

extern "C" {

int count_ok(int count, int capacity) { return obs_slot_count_ok(count, capacity) ? 1 : 0; }
// out7 = fault, the offsets' fault, scene, row, total, capacity, error code
void slots_check(int ctx_nscenes, int max_obstacles, int nscenes, const int32_t *cap_offsets, const int32_t *counts, const double *pos,
                 const double *radius, int *out7) {
    const ObsSlotCheck k = obstacle_slots_check(ctx_nscenes, max_obstacles, nscenes, cap_offsets, counts, pos, radius);
    out7[0] = k.fault; out7[1] = k.offsets; out7[2] = k.scene; out7[3] = k.row; out7[4] = k.total; out7[5] = k.capacity;
    out7[6] = obstacle_slots_error_code(k.fault);
}
void slot_roots(int nscenes, const int32_t *cap_offsets, const int32_t *counts, int32_t *roots) {
    for (int s = 0; s < nscenes; s++) roots[s] = obstacle_slot_root(cap_offsets, counts, s);
}
// out5 = fault, entry, total, replaced, error code
void restart_obs_check(int slots_on, const int32_t *cap_offsets, int count, const int32_t *scene_ids, const int32_t *obs_counts, const double *obs_pos,
                       const double *obs_radius, int *out5) {
    const RestartObsCheck k = restart_obstacles_check(slots_on != 0, cap_offsets, count, scene_ids, obs_counts, obs_pos, obs_radius);
    out5[0] = k.fault; out5[1] = k.entry; out5[2] = k.total; out5[3] = k.replaced; out5[4] = restart_obstacles_error_code(k.fault);
}
// off: [RO_SECTIONS + 1] the sections' offsets and the block's end; bytes: [RO_SECTIONS] what each section must hold; returns where the
// agent sections and the sizes behind them end (what the obstacle sections are laid behind)
long long obs_layout(int max_n, int max_obstacles, long long *off, long long *bytes) {
    const RestartBlock B = restart_block_layout(max_n, max_obstacles, 0);
    for (int s = 0; s < RO_SECTIONS; s++) { off[s] = B.OL.off[s]; bytes[s] = restart_obs_section_bytes(s, max_n, max_obstacles); }
    off[RO_SECTIONS] = B.OL.total;
    return B.new_size_off + (int64_t)sizeof(int32_t) * max_n;          // one int32 per named scene, at most max_n of them
}
void obs_layout_constants(int *out6) {
    out6[0] = RO_SECTIONS; out6[1] = RO_HEAD_WORDS; out6[2] = (int)RO_REC_BYTES; out6[3] = (int)RO_TREE_BYTES; out6[4] = (int)RO_WIDE_BYTES; out6[5] = (int)RS_ALIGN;
}
// a tree built over a slot's obstacles alone, as it stands at the slot's place (scene_obstacle_shift with the slot's obstacle base)
struct Node4 { int32_t begin, end, left, right; };
void slot_shift(int32_t *nodes4, int nnodes, int obs_begin) { scene_obstacle_shift(reinterpret_cast<Node4 *>(nodes4), nnodes, obs_begin, 10); }   // MAX_LEAF, kdTree.py:53

}  // extern "C"

#ifdef SCENE_OBS_SLOTS_MAIN
#define EXPECT(c) do { if (!(c)) { std::printf("scene_obs_slots_harness: FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main() {
    // three slots of obstacle capacity 8, 0 and 5
    const std::vector<int32_t> cap{0, 8, 8, 13};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    {   // the slots call reads exactly nscenes counts and sum(counts) rows
        const std::vector<int32_t> counts{2, 0, 1};
        std::vector<double> pos(9, 1.5), radius(3, 0.5);
        ObsSlotCheck k = obstacle_slots_check(3, 13, 3, cap.data(), counts.data(), pos.data(), radius.data());
        EXPECT(k.fault == OBS_SLOT_OK && k.total == 3 && k.capacity == 13);
        k = obstacle_slots_check(3, 13, 3, cap.data(), nullptr, nullptr, nullptr);
        EXPECT(k.fault == OBS_SLOT_OK && k.total == 0);
        k = obstacle_slots_check(3, 12, 3, cap.data(), counts.data(), pos.data(), radius.data());
        EXPECT(k.fault == OBS_SLOT_OFFSETS && k.offsets == SCENE_OBS_TOO_MANY && obstacle_slots_error_code(k.fault) == SCA_ERR_ARG);
        const std::vector<int32_t> over{2, 1, 1};                   // slot 1 holds none
        k = obstacle_slots_check(3, 13, 3, cap.data(), over.data(), pos.data(), radius.data());
        EXPECT(k.fault == OBS_SLOT_BAD_COUNT && k.scene == 1);
        k = obstacle_slots_check(3, 13, 3, cap.data(), counts.data(), nullptr, radius.data());
        EXPECT(k.fault == OBS_SLOT_NO_ARRAYS && k.total == 3);
        pos[8] = inf;
        k = obstacle_slots_check(3, 13, 3, cap.data(), counts.data(), pos.data(), radius.data());
        EXPECT(k.fault == OBS_SLOT_NOT_FINITE && k.row == 2 && k.scene == 2);
        pos[8] = 1.5; radius[1] = nan;
        k = obstacle_slots_check(3, 13, 3, cap.data(), counts.data(), pos.data(), radius.data());
        EXPECT(k.fault == OBS_SLOT_BAD_RADIUS && k.row == 1 && k.scene == 0);
        std::vector<int32_t> roots(3, 7);
        for (int s = 0; s < 3; s++) roots[s] = obstacle_slot_root(cap.data(), counts.data(), s);
        EXPECT(roots[0] == 0 && roots[1] == -1 && roots[2] == 16);
    }
    {   // the restart's check: `count` entries, the replaced scenes' rows only
        const std::vector<int32_t> ids{2, 0}, counts{5, -1};
        std::vector<double> pos(15, 0.25), radius(5, 1.0);
        RestartObsCheck k = restart_obstacles_check(true, cap.data(), 2, ids.data(), counts.data(), pos.data(), radius.data());
        EXPECT(k.fault == RESTART_OBS_OK && k.total == 5 && k.replaced == 1);
        k = restart_obstacles_check(false, nullptr, 2, ids.data(), counts.data(), pos.data(), radius.data());
        EXPECT(k.fault == RESTART_OBS_NO_SLOTS && k.entry == 0 && restart_obstacles_error_code(k.fault) == SCA_ERR_STATE);
        k = restart_obstacles_check(false, nullptr, 2, ids.data(), nullptr, nullptr, nullptr);
        EXPECT(k.fault == RESTART_OBS_OK && k.replaced == 0);
        const std::vector<int32_t> keep{-1, -1};
        k = restart_obstacles_check(false, nullptr, 2, ids.data(), keep.data(), nullptr, nullptr);
        EXPECT(k.fault == RESTART_OBS_OK && k.replaced == 0 && k.total == 0);
        const std::vector<int32_t> six{6, -1}, low{-1, -2};
        EXPECT(restart_obstacles_check(true, cap.data(), 2, ids.data(), six.data(), pos.data(), radius.data()).fault == RESTART_OBS_BAD_COUNT);
        EXPECT(restart_obstacles_check(true, cap.data(), 2, ids.data(), low.data(), pos.data(), radius.data()).entry == 1);
        radius[4] = 0.0;
        k = restart_obstacles_check(true, cap.data(), 2, ids.data(), counts.data(), pos.data(), radius.data());
        EXPECT(k.fault == RESTART_OBS_BAD_RADIUS && k.entry == 4 && restart_obstacles_error_code(k.fault) == SCA_ERR_ARG);
    }
    {   // the block's obstacle sections
        for (int max_n : {1, 16, 100}) for (int max_m : {0, 1, 8, 1491}) {
            const RestartBlock B = restart_block_layout(max_n, max_m, 0);
            const RestartObsLayout &L = B.OL;
            EXPECT(L.off[0] >= B.new_size_off + (int64_t)sizeof(int32_t) * max_n);
            for (int s = 0; s < RO_SECTIONS; s++) {
                EXPECT(L.off[s] % 16 == 0);
                EXPECT(L.off[s] + restart_obs_section_bytes(s, max_n, max_m) <= (s + 1 < RO_SECTIONS ? L.off[s + 1] : L.total));
            }
        }
    }
    std::printf("scene_obs_slots_harness: ok\n");
    return 0;
}
#endif
