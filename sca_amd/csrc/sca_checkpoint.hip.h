// sca_checkpoint.hip.h -- the kernels behind sca_save_context and sca_load_context (the layout, the check and the row move:
// sca_checkpoint.h).  Launched on the context's stream only by those two entry points: a context that never calls them enqueues exactly
// what it did.
#pragma once
#include "sca_kernels.hip.h"
#include "sca_checkpoint.h"

namespace sca {

// Between two steps, one launch per call at any n: the grid strides over every section with ctx_checkpoint_move, consecutive lanes on
// consecutive 4-byte words (the records, the tracker records, the rings and the closest-approach records as 16-byte pieces), every index
// 64-bit.  `blob` is the library's page-locked block, mapped and coherent: k_ctx_save stores straight into it and k_ctx_load reads it in
// place, as k_scene_save / k_scene_load and k_host_egress do with theirs -- no device staging buffer, no copy behind the kernel.
// k_ctx_load scatters a blob the host has CHECKED (ctx_checkpoint_check: the permutation, the cursors, the lengths and the tracker's
// integers are in range before this kernel sees them).  It also stores K4's striped done_count from the counters the host derived from
// the blob's flags (`stripes`, behind the blob in the same block) and the missions' "entered live" column from the same flags.  Vector
// stores throughout, no atomics, no LDS.  The kd-tree, the neighbour lists, action rows, diag and vpref_used are not state: the next pass
// rebuilds them from what is here before it reads them.
constexpr int CTXCK_T = 256;
constexpr int CTXCK_MAX_BLOCKS = 2048;             // 256 CUs x 8 workgroups; the grid strides beyond
__global__ __launch_bounds__(CTXCK_T) void k_ctx_save(CtxDev d, uint8_t *blob, CtxLayout L, CtxShape S) {
    ctx_checkpoint_move<false>(d, blob, L, S, nullptr, (int64_t)blockIdx.x * CTXCK_T + (int64_t)threadIdx.x, (int64_t)gridDim.x * CTXCK_T);
}
__global__ __launch_bounds__(CTXCK_T) void k_ctx_load(CtxDev d, const uint8_t *blob, CtxLayout L, CtxShape S, const int32_t *stripes) {
    ctx_checkpoint_move<true>(d, const_cast<uint8_t *>(blob), L, S, stripes, (int64_t)blockIdx.x * CTXCK_T + (int64_t)threadIdx.x, (int64_t)gridDim.x * CTXCK_T);
}
// sca_load_context_opt with SCA_CHECKPOINT_VACANCY: k_ctx_load's move plus, for every vacant row of the checked blob, the outputs a retire
// left and no pass writes again (ctx_checkpoint_move_vacancy).  A symbol of its own, so that k_ctx_load stays what it was; still one
// launch and one synchronisation at any n.
__global__ __launch_bounds__(CTXCK_T) void k_ctx_load_vacancy(CtxDev d, CtxVacDev o, const uint8_t *blob, CtxLayout L, CtxShape S, const int32_t *stripes) {
    ctx_checkpoint_move_vacancy(d, o, const_cast<uint8_t *>(blob), L, S, stripes, (int64_t)blockIdx.x * CTXCK_T + (int64_t)threadIdx.x, (int64_t)gridDim.x * CTXCK_T);
}
// workgroups for a blob of `bytes`: a lane per 16 bytes, capped
inline int ctx_checkpoint_blocks(int64_t bytes) {
    const int64_t want = (bytes / 16 + CTXCK_T - 1) / CTXCK_T;
    return (int)(want < 1 ? 1 : want > CTXCK_MAX_BLOCKS ? CTXCK_MAX_BLOCKS : want);
}

}  // namespace sca
