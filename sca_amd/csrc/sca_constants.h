// sca_constants.h -- the sizes the kernels are built with AND the host prices its launches with (sca_forms.h).  Plain C++, no HIP.
#pragma once

namespace sca {

constexpr int K1_WAVES = 4;                // wavefronts (= agents) per workgroup of k_neighbors_kd / k_neighbors_kd_auto
constexpr int KDQ_BLOCKS = 1024, KDQ_BLOCKS_FEW = 64;   // (the few: while the counts that came back say a wavefront each is enough -- an empty launch of 64 workgroups is half as long)

// A node of <= wave_max members (KdScratch::wave_max, chosen per build) is finished, whole subtree, by ONE WORKGROUP in LDS
// (k_kd_block).  The host picks it between these bounds so that the node sizes of a level (n / 2^k, within a few per cent)
// do not straddle it: with a fixed 1024 the 4096- and 16384-agent trees needed a whole level pass for the half of their
// ~1024-member nodes that were a little larger.
constexpr int KD_WAVE_MIN = 768, KD_WAVE_CAP = 1536;   // the defaults; SCA_KD_WAVE_CAP picks a smaller workgroup form (Tunables::kd_wave_cap)
constexpr int KD_WAVE_FLOOR = 128;                     // tables are sized for subtrees handed over at this size or above
constexpr int KD_MAX_LEVELS = 40;
constexpr int KD_CHUNK = 2048;         // positions per workgroup in the level passes over larger nodes
constexpr int KT_M = 4096;             // k_kd_top: the largest tree whose top one workgroup builds in LDS

// re-plans of a pass up to which each re-plan form is the one that works (at 1024 SIMDs; Tunables::spec4_max ... mid_max)
constexpr int TRK_MID_MAX = 32768;         // k_replan_group<4>: four lanes per plan, two wavefronts per SIMD (217 registers): 32 768 plans = 2048 wavefronts
constexpr int TRK_SPEC2_MAX = 8192;        // <= this many re-plans in the pass: 3 candidates per round, 16 lanes per plan (2048 wavefronts: two per SIMD)
constexpr int TRK_SPEC3_MAX = 4096;        // <= this many: 7 per round, 32 lanes per plan (2048 wavefronts)
constexpr int TRK_SPEC4_MAX = 1024;        // <= this many: 15 per round, a whole wavefront per plan -- and a SIMD per wavefront (the kernel sits at the 256-register edge)

}  // namespace sca
