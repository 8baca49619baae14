// Test-only: the host-side rules of the trajectory log per scene (sca_amd/csrc/sca_scenes.h: scene_log_index, scene_log_bytes,
// scene_log_enable_check, scene_log_check) behind a C interface for tests/test_scene_log_cpu.py.  Plain C++, no HIP.  Not part of the
// product (sca_amd never loads it).  With -DSCENE_LOG_MAIN it is a program of its own that walks the same functions over whole layouts, for
// a build under -fsanitize=address,undefined.
#include "sca_scenes.h"

using namespace sca;

extern "C" {

int64_t slog_index(int capacity, int scene_begin, int scene_size, int r, int i) { return scene_log_index(capacity, scene_begin, scene_size, r, i); }
int64_t slog_bytes(int capacity, int n) { return scene_log_bytes(capacity, n); }
void slog_rows(int steps, int capacity, int *out2) { out2[0] = scene_log_rows_logged(steps, capacity); out2[1] = scene_log_rows_dropped(steps, capacity); }
// out2: fault, scene.  Returns the error code sca_scene_history_enable gives for the fault.
int slog_enable_check(int nscenes, int scene_begun, const int32_t *steps, int capacity, int *out2) {
    const SceneLogCheck k = scene_log_enable_check(nscenes, scene_begun != 0, steps, capacity);
    out2[0] = k.fault; out2[1] = k.scene;
    return scene_log_error_code(k.fault);
}
// out2: fault, scene.  Returns the error code sca_scene_history_rows (window == 0) / sca_get_scene_history give for the fault.
int slog_check(int nscenes, const int32_t *offsets, int enabled, int capacity, int window, int scene, int steps_of_scene, int first_row, int nrows,
               int agent_begin, int agent_count, int *out2) {
    const SceneLogCheck k = scene_log_check(nscenes, offsets, enabled != 0, capacity, window != 0, scene, steps_of_scene, first_row, nrows, agent_begin, agent_count);
    out2[0] = k.fault; out2[1] = k.scene;
    return scene_log_error_code(k.fault);
}

}  // extern "C"

#ifdef SCENE_LOG_MAIN
#include <cstdio>
// Every row of every agent of every scene lands on a cell of its own inside capacity x n, and every window the check lets through stays
// inside its scene's part -- on an array of exactly that size, so that the sanitizer sees any index outside it.
static int walk(int capacity, const std::vector<int32_t> &off) {
    const int B = (int)off.size() - 1, n = off[B];
    std::vector<uint8_t> cell((std::size_t)(scene_log_bytes(capacity, n) / SCENE_LOG_ROW_BYTES), (uint8_t)0);
    for (int s = 0; s < B; s++)
        for (int r = 0; r < capacity; r++)
            for (int i = 0; i < off[s + 1] - off[s]; i++) {
                const int64_t at = scene_log_index(capacity, off[s], off[s + 1] - off[s], r, i);
                if (at < (int64_t)capacity * off[s] || at >= (int64_t)capacity * off[s + 1]) return 1;      // outside the scene's part
                if (cell[(std::size_t)at]++) return 2;                                                        // two rows on one cell
            }
    for (uint8_t c : cell) if (c != 1) return 3;                                                              // a cell nobody owns
    for (int s = -1; s <= B; s++)
        for (int steps = 0; steps <= capacity + 2; steps++)
            for (int first = -1; first <= capacity + 1; first++)
                for (int nrows = -1; nrows <= capacity + 1; nrows++)
                    for (int ab = -1; ab <= 2; ab++)
                        for (int ac = -1; ac <= 6; ac++) {
                            const SceneLogCheck k = scene_log_check(B, off.data(), true, capacity, true, s, steps, first, nrows, ab, ac);
                            if (k.fault != SCENE_LOG_OK || nrows == 0 || ac == 0) continue;
                            const int ns = off[s + 1] - off[s];
                            cell[(std::size_t)scene_log_index(capacity, off[s], ns, first, ab)] = 2;                  // the window's corners
                            cell[(std::size_t)scene_log_index(capacity, off[s], ns, first + nrows - 1, ab + ac - 1)] = 2;
                            if (first + nrows > steps || first + nrows > capacity || ab + ac > ns) return 4;
                        }
    return 0;
}
int main() {
    int bad = walk(4, {0, 3, 8, 10});
    if (!bad) bad = walk(1, {0, 1}) ? 10 : 0;
    if (!bad) bad = walk(7, {0, 1, 2, 19, 20}) ? 20 : 0;
    // 64 bits: capacity 100 000 x n 1 000 000 rows, 6.4e12 bytes
    if (!bad && scene_log_bytes(100000, 1000000) != INT64_C(6400000000000)) bad = 30;
    if (!bad && scene_log_index(100000, 999000, 1000, 99999, 999) != INT64_C(99999999999)) bad = 31;
    std::printf(bad ? "scene_log_harness: FAILED (%d)\n" : "scene_log_harness: ok\n", bad);
    return bad ? 1 : 0;
}
#endif
