// Test-only: the row arithmetic of k_host_ingest / k_host_egress (sca_amd/csrc/sca_hostio.hip.h) compiled for the host.  One "workgroup" per
// tile of HIO_TILE agents, its lanes run one after the other, phase by phase -- the barriers of the kernels are the ends of the lane loops.
// Not part of the product (sca_amd never loads it).
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../include/sca_hip.h"
#include "sca_hostio.hip.h"

using namespace sca;

extern "C" {

int hio_sizeof_host_state(void) { return (int)sizeof(sca_host_state); }
int hio_sizeof_pubrec(void) { return (int)sizeof(PubRec); }
int hio_tile(void) { return HIO_TILE; }

int hio_layout(int n, int64_t *offsets, int64_t *total) {
    const HostLayout L = host_state_layout(n);
    for (int s = 0; s < HS_SECTIONS; s++) offsets[s] = L.off[s];
    *total = L.total;
    return HS_SECTIONS;
}

// rec: n PubRec (48 bytes each) -- the caller looks at them as raw bytes
void hio_ingest(void *rec, double *heading, double *total_dist, int32_t *step_num, double *vpref_ext, uint8_t *vpref_mode,
                const uint8_t *blk, int n, uint32_t mask) {
    const HostIoDev d{(PubRec *)rec, heading, total_dist, step_num, vpref_ext, vpref_mode, nullptr};
    const HostLayout L = host_state_layout(n);
    std::vector<HioVec> tile_v(HIO_TILE * HIO_REC_WORDS / 4);
    hio_u32 *tile = (hio_u32 *)tile_v.data();
    for (int base = 0; base < n; base += HIO_TILE) {
        const int cnt = n - base < HIO_TILE ? n - base : HIO_TILE;
        if (mask & HOST_IN_STATE) {
            for (int t = 0; t < HIO_TILE; t++) { hio_tile_load_rec(tile, d.rec, base, cnt, t); hio_tile_state_up(d, blk, L, base, cnt, t); }
            for (int t = 0; t < HIO_TILE; t++) hio_tile_ingest(tile, blk, L, base, cnt, t);
            for (int t = 0; t < HIO_TILE; t++) hio_tile_store_rec(d.rec, tile, base, cnt, t);
        }
        if (mask & HOST_IN_VPREF)
            for (int t = 0; t < HIO_TILE; t++) hio_tile_vpref_up(d, blk, L, base, cnt, t);
    }
}

void hio_egress(const void *rec, const double *heading, const double *total_dist, const int32_t *step_num, const float *action8,
                uint8_t *blk, int n) {
    const HostIoDev d{(PubRec *)rec, (double *)heading, (double *)total_dist, (int32_t *)step_num, nullptr, nullptr, action8};
    const HostLayout L = host_state_layout(n);
    std::vector<HioVec> tile_v(HIO_TILE * HIO_REC_WORDS / 4);
    hio_u32 *tile = (hio_u32 *)tile_v.data();
    for (int base = 0; base < n; base += HIO_TILE) {
        const int cnt = n - base < HIO_TILE ? n - base : HIO_TILE;
        for (int t = 0; t < HIO_TILE; t++) { hio_tile_load_rec(tile, d.rec, base, cnt, t); hio_tile_state_down(d, blk, L, base, cnt, t); }
        for (int t = 0; t < HIO_TILE; t++) hio_tile_egress(tile, blk, L, base, cnt, t);
    }
}

}  // extern "C"
