// sca_scenes.h -- scene batches (sca_set_scenes): the host-side rules, as pure functions.  No HIP, no sca_ctx: sca_hip.hip calls them and
// turns their answers into error codes and messages; tests/scenes_harness.cpp checks them without a GPU.
//
// One context holds B scenes; scene s is the contiguous agent range [offsets[s], offsets[s + 1]).  Each scene is one job of k_kd_block
// (its whole tree by one workgroup in LDS), hence at most KD_WAVE_CAP agents per scene.
#pragma once
#include <cstdint>

#include "../../include/sca_hip.h"
#include "sca_constants.h"

namespace sca {

enum SceneFault {
    SCENES_OK = 0,
    SCENES_NONE,            // nscenes == 0 or offsets == NULL: the context is a plain one
    SCENES_BAD_COUNT,       // nscenes < 0 or more scenes than agents
    SCENES_BAD_START,       // offsets[0] != 0
    SCENES_NOT_INCREASING,  // an empty scene, or offsets that decrease
    SCENES_BAD_END,         // offsets[nscenes] != n
    SCENES_TOO_LARGE        // a scene of more than KD_WAVE_CAP agents
};
// fault: which rule failed; scene: the first scene that breaks it (-1: none in particular); largest: the largest scene's agent count (SCENES_OK)
struct SceneCheck { SceneFault fault; int scene; int largest; };
inline SceneCheck scenes_check(int n, int nscenes, const int32_t *offsets) {
    if (nscenes == 0 || offsets == nullptr) return {SCENES_NONE, -1, 0};
    if (nscenes < 0 || nscenes > n) return {SCENES_BAD_COUNT, -1, 0};
    if (offsets[0] != 0) return {SCENES_BAD_START, 0, 0};
    int largest = 0;
    for (int s = 0; s < nscenes; s++) {
        if (offsets[s + 1] <= offsets[s]) return {SCENES_NOT_INCREASING, s, 0};
        if (offsets[s + 1] > n) return {SCENES_BAD_END, s, 0};          // (also keeps every later read of a per-agent array in bounds)
        const int size = offsets[s + 1] - offsets[s];
        if (size > KD_WAVE_CAP) return {SCENES_TOO_LARGE, s, size};
        if (size > largest) largest = size;
    }
    if (offsets[nscenes] != n) return {SCENES_BAD_END, nscenes - 1, 0};
    return {SCENES_OK, -1, largest};
}
// what sca_set_scenes returns for a fault
inline int scenes_error_code(SceneFault f) {
    return f == SCENES_OK || f == SCENES_NONE ? SCA_OK : (f == SCENES_TOO_LARGE ? SCA_ERR_UNSUPPORTED : SCA_ERR_ARG);
}

// kdTree.agentIDs of a context with scenes carries global ids, and a scene's positions hold that scene's ids only (a build permutes inside
// a job's range).  The first position whose id lies outside its scene, -1: none.  (offsets: checked by scenes_check)
inline int scenes_perm_fault(int nscenes, const int32_t *offsets, const int32_t *perm) {
    for (int s = 0; s < nscenes; s++)
        for (int p = offsets[s]; p < offsets[s + 1]; p++)
            if (perm[p] < offsets[s] || perm[p] >= offsets[s + 1]) return p;
    return -1;
}

// the neighbour mode a context with scenes runs for the one that was asked for: the forest of kd-trees is the scene form, SCA_NBR_AUTO
// resolves to it (one more place where the grid cannot help: its cell key carries no scene id), the grid and the host build have none (-1)
inline int scenes_neighbor_mode(int requested) {
    return requested == SCA_NBR_KDTREE || requested == SCA_NBR_AUTO ? (int)SCA_NBR_KDTREE : -1;
}

}  // namespace sca
