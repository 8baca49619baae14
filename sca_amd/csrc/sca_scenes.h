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

// ---- per-scene obstacle sets (sca_set_scene_obstacles) ---------------------------------------------------------------------------------------
// Scene s meets obstacles [obs_offsets[s], obs_offsets[s + 1]) and no others; a scene may have none.  The obstacle tree becomes a forest
// like the agents': one tree per scene, built over that scene's obstacles alone with local ids 0 .. m_s - 1 (what makes every value the
// single-scene context's), laid side by side in otree[2M] / owide[2M] with scene s's nodes numbered from 2 * obs_offsets[s] (a tree over k
// members occupies 2k - 1 nodes: the ranges are disjoint).
enum SceneObsFault {
    SCENE_OBS_OK = 0,
    SCENE_OBS_BAD_COUNT,    // nscenes is not the context's scene count
    SCENE_OBS_NO_OFFSETS,   // obs_offsets == NULL
    SCENE_OBS_BAD_START,    // obs_offsets[0] != 0
    SCENE_OBS_DECREASING,   // obs_offsets[s + 1] < obs_offsets[s] (equal is fine: a scene without obstacles)
    SCENE_OBS_TOO_MANY,     // obs_offsets[nscenes] > sca_create's max_obstacles
    SCENE_OBS_NO_ARRAYS     // a positive total with pos == NULL or radius == NULL
};
// fault: which rule failed; scene: the first scene that breaks it (-1: none in particular); total: obs_offsets[nscenes] (SCENE_OBS_OK, _TOO_MANY, _NO_ARRAYS)
struct SceneObsCheck { SceneObsFault fault; int scene; int total; };
inline SceneObsCheck scene_obstacles_check(int ctx_nscenes, int max_obstacles, int nscenes, const int32_t *obs_offsets, bool have_pos, bool have_radius) {
    if (nscenes != ctx_nscenes || nscenes <= 0) return {SCENE_OBS_BAD_COUNT, -1, 0};
    if (obs_offsets == nullptr) return {SCENE_OBS_NO_OFFSETS, -1, 0};
    if (obs_offsets[0] != 0) return {SCENE_OBS_BAD_START, 0, 0};
    for (int s = 0; s < nscenes; s++)
        if (obs_offsets[s + 1] < obs_offsets[s]) return {SCENE_OBS_DECREASING, s, 0};
    const int total = obs_offsets[nscenes];
    if (total > max_obstacles) return {SCENE_OBS_TOO_MANY, -1, total};
    if (total > 0 && !(have_pos && have_radius)) return {SCENE_OBS_NO_ARRAYS, -1, total};
    return {SCENE_OBS_OK, -1, total};
}
// what sca_set_scene_obstacles returns for a fault
inline int scene_obstacles_error_code(SceneObsFault f) { return f == SCENE_OBS_OK ? SCA_OK : SCA_ERR_ARG; }

// where scene s's obstacle walks start: the root record of its tree in the forest, -1: the scene has no obstacles (no walk at all)
inline int scene_obstacle_root(const int32_t *obs_offsets, int s) {
    return obs_offsets[s + 1] - obs_offsets[s] > 0 ? 2 * obs_offsets[s] : -1;
}

// A tree built over one scene's obstacles alone (nodes numbered from 0, members 0 .. m_s - 1; Node: begin, end, left, right) as it stands
// in the forest: member ranges shifted by obs_begin = obs_offsets[s], child links by the node base 2 * obs_begin.  A leaf (at most max_leaf
// members, kdTree.py:53) keeps its links at 0, the "no children" the build writes; unused records (begin == end) stay as they are.  The
// caller copies nodes[i] to 2 * obs_begin + i.
template <class Node>
inline void scene_obstacle_shift(Node *nodes, int nnodes, int obs_begin, int max_leaf) {
    for (int i = 0; i < nnodes; i++) {
        Node &nd = nodes[i];
        if (nd.end == nd.begin) continue;
        const bool inner = nd.end - nd.begin > max_leaf;
        nd.begin += obs_begin; nd.end += obs_begin;
        if (inner) { nd.left += 2 * obs_begin; nd.right += 2 * obs_begin; }
    }
}

}  // namespace sca
