// tests/scene_sizes_harness.cpp -- the host-side rules of slots of a capacity (sca_restart_scenes_sized, sca_scenes.h) behind
// tests/test_scene_sizes_cpu.py.  Plain C++, no HIP.  Not part of the library.  With -DSCENE_SIZES_MAIN it is a program of its own, for
// a build under -fsanitize=address,undefined: its main walks the same rules on heap arrays of exactly the sizes the rules may read.
#include <cstdio>
#include <vector>

#include "sca_scenes.h"

using namespace sca;

extern "C" {

int size_ok(int size, int capacity) { return scene_size_ok(size, capacity) ? 1 : 0; }
// start: [count]; returns T
int restart_starts(int count, const int32_t *offsets, const int32_t *scene_ids, const int32_t *sizes, int32_t *start) {
    return scene_restart_starts(count, offsets, scene_ids, sizes, start);
}
int any_partial(int nscenes, const int32_t *offsets, const int32_t *size) { return scenes_any_partial(nscenes, offsets, size) ? 1 : 0; }
int log_agents_ok(int size, int agent_begin, int agent_count) { return scene_log_agents_ok(size, agent_begin, agent_count) ? 1 : 0; }
// scene_restart_check of a valid context (state set, tracker on) with `rows` rows of valid arrays: out3 = fault, entry, T; returns the error code
int sized_check(int nscenes, const int32_t *offsets, const uint8_t *policy_now, int per_agent, int count, const int32_t *scene_ids, const int32_t *sizes,
                int rows, const uint8_t *policy, int *out3) {
    const std::vector<double> three((size_t)3 * rows, 1.0);
    const RestartCtx X{nscenes, offsets, true, false, true, false, per_agent != 0, policy_now};
    RestartArgs A{count, scene_ids, three.data(), nullptr, three.data(), nullptr, nullptr, nullptr, policy, nullptr, nullptr, nullptr};
    A.sizes = sizes;
    const RestartCheck k = scene_restart_check(X, A);
    out3[0] = k.fault; out3[1] = k.entry; out3[2] = k.total;
    return scene_restart_error_code(k.fault);
}
// the window check of sca_get_scene_history with the scenes' sizes (size may be NULL: every scene full); out2 = fault, scene
int log_window(int nscenes, const int32_t *offsets, const int32_t *size, int capacity, int scene, int steps, int first_row, int nrows, int agent_begin,
               int agent_count, int *out2) {
    const SceneLogCheck k = scene_log_check(nscenes, offsets, true, capacity, true, scene, steps, first_row, nrows, agent_begin, agent_count, size);
    out2[0] = k.fault; out2[1] = k.scene;
    return scene_log_error_code(k.fault);
}

}  // extern "C"

#ifdef SCENE_SIZES_MAIN
#define EXPECT(c) do { if (!(c)) { std::printf("scene_sizes_harness: FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main() {
    // three slots of capacity 3, 5 and 2
    const std::vector<int32_t> off{0, 3, 8, 10};
    const std::vector<uint8_t> now{0, 1, 2, 3, 4, 5, 0, 1, 2, 3};
    for (int cap : {1, 2, 130}) {
        EXPECT(!scene_size_ok(0, cap) && !scene_size_ok(-1, cap) && !scene_size_ok(cap + 1, cap) && scene_size_ok(cap, cap) && scene_size_ok(1, cap));
    }
    {   // packed-row starts: arrays of exactly `count` entries
        const std::vector<int32_t> ids{2, 0, 1}, sizes{1, 3, 4};
        std::vector<int32_t> start(3, -7);
        EXPECT(scene_restart_starts(3, off.data(), ids.data(), sizes.data(), start.data()) == 8 && start[0] == 0 && start[1] == 1 && start[2] == 4);
        EXPECT(scene_restart_starts(3, off.data(), ids.data(), nullptr, start.data()) == 10 && start[0] == 0 && start[1] == 2 && start[2] == 5);
        EXPECT(scene_restart_starts(3, off.data(), ids.data(), sizes.data(), nullptr) == 8);
    }
    {   // the check reads exactly T rows of every array, and policy_now only under the rows an episode occupies
        const std::vector<int32_t> ids{1, 2}, sizes{2, 1};
        const std::vector<double> three(9, 0.5);                     // T = 3 rows
        const std::vector<uint8_t> pol{3, 4, 2};
        const RestartCtx X{3, off.data(), true, false, true, false, true, now.data()};
        RestartArgs A{2, ids.data(), three.data(), nullptr, three.data(), nullptr, nullptr, nullptr, pol.data(), nullptr, nullptr, nullptr};
        A.sizes = sizes.data();
        RestartCheck k = scene_restart_check(X, A);
        EXPECT(k.fault == RESTART_OK && k.total == 3);
        const std::vector<int32_t> bad{2, 3};                         // scene 2 holds at most 2
        A.sizes = bad.data();
        k = scene_restart_check(X, A);
        EXPECT(k.fault == RESTART_BAD_SIZE && k.entry == 1 && scene_restart_error_code(k.fault) == SCA_ERR_ARG);
        const std::vector<int32_t> zero{0, 1};
        A.sizes = zero.data();
        k = scene_restart_check(X, A);
        EXPECT(k.fault == RESTART_BAD_SIZE && k.entry == 0);
    }
    {
        const std::vector<int32_t> full{3, 5, 2}, part{3, 4, 2};
        EXPECT(!scenes_any_partial(3, off.data(), full.data()) && scenes_any_partial(3, off.data(), part.data()));
        EXPECT(scene_log_agents_ok(4, 0, 4) && !scene_log_agents_ok(4, 0, 5) && !scene_log_agents_ok(4, 4, 1) && scene_log_agents_ok(4, 4, 0));
        EXPECT(!scene_log_agents_ok(4, 2147483647, 1) && !scene_log_agents_ok(4, -1, 1) && !scene_log_agents_ok(4, 0, -1));
        EXPECT(scene_log_check(3, off.data(), true, 8, true, 1, 3, 0, 3, 0, 4, part.data()).fault == SCENE_LOG_OK);
        EXPECT(scene_log_check(3, off.data(), true, 8, true, 1, 3, 0, 3, 0, 5, part.data()).fault == SCENE_LOG_BAD_AGENTS);
        EXPECT(scene_log_check(3, off.data(), true, 8, true, 1, 3, 0, 3, 0, 5, nullptr).fault == SCENE_LOG_OK);
    }
    std::printf("scene_sizes_harness: ok\n");
    return 0;
}
#endif
