// sca_hostio.hip.h -- the two data-movement kernels of sca_step_host (include/sca_hip.h): the env loop of mampenv.py:27-59 with the HOST as
// the owner of the state, which then crosses the link twice per step.
//
//   k_host_ingest   the pinned host state block -- read across the link, or its device copy in the staged form (SCA_HOST_STEP_STAGED) -- (AoS rows: pos 24 B, vel 12 B, heading 24 B, flags 1 B, total_dist 8 B,
//                   step_num 4 B; v_pref 24 B, vpref_mode 1 B)  ->  the 48-byte PubRec array + heading / total_dist / step_num (+ vpref_ext /
//                   vpref_mode).  What sca_set_state's host loop (one thread, all agents) and its four pageable copies did.
//   k_host_egress   the moved records, heading, total_dist, step_num and the 7 used floats of every 8-float action row -> the block's layout.
//                   What sca_get_state's host loop and sca_get_actions' re-packing loop did.
//
// One workgroup of 256 lanes per tile of 256 agents.  A tile's rows are contiguous in every section and in the record array, so everything is
// moved as 4-byte words (16-byte vectors for the records), lane i next to lane i + 1: the records of the tile are staged in LDS (12 KB),
// the AoS sections are scattered into / gathered from that copy word by word (pos: word w of the tile is word w % 6 of record w / 6; vel:
// w % 3 of record w / 3; flags: one word = the flag bytes of four agents), and the tile goes back with 16-byte stores -- `radius`, which the
// block does not carry, rides along untouched.  No lane issues a byte access except for the up-to-three agents of a vpref_mode tail.
// flags round-trip as sca_set_state / sca_get_state do it: up rec.flags = flags[i], down (uint8_t)rec.flags.
//
// The row arithmetic (hio_*) is plain C++ on pointers and compiles for the host too: tests/hostio_harness.cpp runs it lane by lane.
#pragma once
#include "sca_core.h"

namespace sca {

constexpr int HIO_TILE = 256;             // agents per workgroup = lanes per workgroup
constexpr int HIO_REC_WORDS = 12;         // sizeof(PubRec) / 4
constexpr uint32_t HOST_IN_STATE = 1, HOST_IN_VPREF = 2;   // SCA_HOST_IN_* of include/sca_hip.h

typedef uint32_t __attribute__((may_alias)) hio_u32;
struct __attribute__((may_alias, aligned(16))) HioVec { uint32_t x, y, z, w; };

// the device arrays the two kernels touch (DeviceView's, sca_kernels.hip.h)
struct HostIoDev {
    PubRec *rec;             // [n] the CURRENT records
    double *heading;         // [n*3]
    double *total_dist;      // [n]
    int32_t *step_num;       // [n]
    double *vpref_ext;       // [n*3]
    uint8_t *vpref_mode;     // [n]
    const float *action;     // [n*8] (7 used)
};

// Every function below is lane t of HIO_TILE working on the tile of agents [base, base + cnt), base a multiple of HIO_TILE.

// records of the tile <-> their copy (LDS on the device), 16 bytes per lane and access
SCA_HD void hio_tile_load_rec(hio_u32 *tile, const PubRec *rec, int base, int cnt, int t) {
    const HioVec *src = (const HioVec *)(rec + base);
    HioVec *dst = (HioVec *)tile;
    for (int q = t; q < cnt * 3; q += HIO_TILE) dst[q] = src[q];
}
SCA_HD void hio_tile_store_rec(PubRec *rec, const hio_u32 *tile, int base, int cnt, int t) {
    const HioVec *src = (const HioVec *)tile;
    HioVec *dst = (HioVec *)(rec + base);
    for (int q = t; q < cnt * 3; q += HIO_TILE) dst[q] = src[q];
}

// block -> record copy: px, py, pz (words 0-5), vx, vy, vz (6-8), flags (9); radius (10-11) stays
SCA_HD void hio_tile_ingest(hio_u32 *tile, const uint8_t *blk, const HostLayout &L, int base, int cnt, int t) {
    const hio_u32 *pos = (const hio_u32 *)(blk + L.off[HS_POS]) + (int64_t)base * 6;
    for (int w = t; w < cnt * 6; w += HIO_TILE) tile[(w / 6) * HIO_REC_WORDS + w % 6] = pos[w];
    const hio_u32 *vel = (const hio_u32 *)(blk + L.off[HS_VEL]) + (int64_t)base * 3;
    for (int w = t; w < cnt * 3; w += HIO_TILE) tile[(w / 3) * HIO_REC_WORDS + 6 + w % 3] = vel[w];
    const hio_u32 *fl = (const hio_u32 *)(blk + L.off[HS_FLAGS] + base);   // (the section is padded to 64 bytes: the tail word is inside)
    for (int w = t; w < (cnt + 3) / 4; w += HIO_TILE) {
        const uint32_t v = fl[w];
        for (int b = 0; b < 4; b++)
            if (4 * w + b < cnt) tile[(4 * w + b) * HIO_REC_WORDS + 9] = (v >> (8 * b)) & 0xffu;          // rec.flags = flags[i]
    }
}
// record copy -> block
SCA_HD void hio_tile_egress(const hio_u32 *tile, uint8_t *blk, const HostLayout &L, int base, int cnt, int t) {
    hio_u32 *pos = (hio_u32 *)(blk + L.off[HS_POS]) + (int64_t)base * 6;
    for (int w = t; w < cnt * 6; w += HIO_TILE) pos[w] = tile[(w / 6) * HIO_REC_WORDS + w % 6];
    hio_u32 *vel = (hio_u32 *)(blk + L.off[HS_VEL]) + (int64_t)base * 3;
    for (int w = t; w < cnt * 3; w += HIO_TILE) vel[w] = tile[(w / 3) * HIO_REC_WORDS + 6 + w % 3];
    hio_u32 *fl = (hio_u32 *)(blk + L.off[HS_FLAGS] + base);
    for (int w = t; w < (cnt + 3) / 4; w += HIO_TILE) {
        uint32_t v = 0;
        for (int b = 0; b < 4; b++)
            if (4 * w + b < cnt) v |= (tile[(4 * w + b) * HIO_REC_WORDS + 9] & 0xffu) << (8 * b);        // (uint8_t)rec.flags
        fl[w] = v;                                                                                         // (tail: zeros into the padding)
    }
}

// the private state is AoS on the device as well: straight copies, one element per lane
SCA_HD void hio_tile_state_up(const HostIoDev &d, const uint8_t *blk, const HostLayout &L, int base, int cnt, int t) {
    const double *h = (const double *)(blk + L.off[HS_HEADING]) + (int64_t)base * 3;
    for (int q = t; q < cnt * 3; q += HIO_TILE) d.heading[(int64_t)base * 3 + q] = h[q];
    if (t < cnt) {
        d.total_dist[base + t] = ((const double *)(blk + L.off[HS_TOTAL_DIST]))[base + t];
        d.step_num[base + t] = ((const int32_t *)(blk + L.off[HS_STEP_NUM]))[base + t];
    }
}
SCA_HD void hio_tile_vpref_up(const HostIoDev &d, const uint8_t *blk, const HostLayout &L, int base, int cnt, int t) {
    const double *v = (const double *)(blk + L.off[HS_VPREF]) + (int64_t)base * 3;
    for (int q = t; q < cnt * 3; q += HIO_TILE) d.vpref_ext[(int64_t)base * 3 + q] = v[q];
    const uint8_t *m = blk + L.off[HS_VPREF_MODE] + base;
    if (t < cnt / 4) ((hio_u32 *)(d.vpref_mode + base))[t] = ((const hio_u32 *)m)[t];
    else if (t < cnt / 4 + cnt % 4) {                       // the last one to three agents of the swarm: the device array ends at n bytes
        const int a = (cnt / 4) * 4 + (t - cnt / 4);
        d.vpref_mode[base + a] = m[a];
    }
}
SCA_HD void hio_tile_state_down(const HostIoDev &d, uint8_t *blk, const HostLayout &L, int base, int cnt, int t) {
    double *h = (double *)(blk + L.off[HS_HEADING]) + (int64_t)base * 3;
    for (int q = t; q < cnt * 3; q += HIO_TILE) h[q] = d.heading[(int64_t)base * 3 + q];
    if (t < cnt) {
        ((double *)(blk + L.off[HS_TOTAL_DIST]))[base + t] = d.total_dist[base + t];
        ((int32_t *)(blk + L.off[HS_STEP_NUM]))[base + t] = d.step_num[base + t];
    }
    // action rows 32 -> 28 bytes: the writes are contiguous, the reads skip every eighth word
    float *out = (float *)(blk + L.off[HS_ACTION]) + (int64_t)base * 7;
    for (int w = t; w < cnt * 7; w += HIO_TILE) out[w] = d.action[((int64_t)base + w / 7) * 8 + w % 7];
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(HIO_TILE) void k_host_ingest(HostIoDev d, const uint8_t *blk, int n, uint32_t mask) {
    __shared__ HioVec tile_v[HIO_TILE * HIO_REC_WORDS / 4];
    hio_u32 *tile = (hio_u32 *)tile_v;
    const HostLayout L = host_state_layout(n);
    const int base = (int)blockIdx.x * HIO_TILE, t = (int)threadIdx.x;
    const int cnt = n - base < HIO_TILE ? n - base : HIO_TILE;
    if (mask & HOST_IN_STATE) {                             // (uniform over the launch)
        hio_tile_load_rec(tile, d.rec, base, cnt, t);
        hio_tile_state_up(d, blk, L, base, cnt, t);
        __syncthreads();
        hio_tile_ingest(tile, blk, L, base, cnt, t);
        __syncthreads();
        hio_tile_store_rec(d.rec, tile, base, cnt, t);
    }
    if (mask & HOST_IN_VPREF) hio_tile_vpref_up(d, blk, L, base, cnt, t);
}

__global__ __launch_bounds__(HIO_TILE) void k_host_egress(HostIoDev d, uint8_t *blk, int n) {
    __shared__ HioVec tile_v[HIO_TILE * HIO_REC_WORDS / 4];
    hio_u32 *tile = (hio_u32 *)tile_v;
    const HostLayout L = host_state_layout(n);
    const int base = (int)blockIdx.x * HIO_TILE, t = (int)threadIdx.x;
    const int cnt = n - base < HIO_TILE ? n - base : HIO_TILE;
    hio_tile_load_rec(tile, d.rec, base, cnt, t);
    hio_tile_state_down(d, blk, L, base, cnt, t);
    __syncthreads();
    hio_tile_egress(tile, blk, L, base, cnt, t);
}
#endif

}  // namespace sca
