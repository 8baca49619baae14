// The host-side rules of sca_restart_scenes_attrs (sca_amd/csrc/sca_scenes.h) behind a C surface: the descriptor's checks, the attribute
// sections of the staging block and the tracker's class table.  Built twice by tests/test_scene_attrs_cpu.py: as a shared library for
// ctypes, and -- with -DSCENE_ATTRS_MAIN -- as a program of its own under AddressSanitizer and UBSan, which walks one fixed scenario through
// the same entry points and prints what they answer.
#include <cstdio>
#include <cstring>
#include <vector>

#include "sca_scenes.h"

using namespace sca;

extern "C" {

// ctx_bits: 1 state set, 2 mid-step, 4 tracker on, 8 paths on.  defaults: neighbor_dist, time_step, time_horizon, max_speed,
// max_heading_change, dt_nominal, max_neighbors, turning_radius, pitch_lo, pitch_hi.  ptrs: the ten arrays of sca_restart_attrs in the
// struct's order (NULL entries stay NULL).  out: fault, entry, and which of the ten members the library would read (a bit each).
int attrs_check(int nscenes, const int32_t *offsets, int ctx_bits, const uint8_t *policy_now, int count, const int32_t *ids, const int32_t *sizes,
                const uint8_t *policy, int struct_bytes, int reserved, const void *const *ptrs, const double *defaults, int *out) {
    RestartArgs A{count, ids, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, policy, nullptr, nullptr, nullptr};
    A.sizes = sizes;
    const RestartCtx X{nscenes, offsets, (ctx_bits & 1) != 0, (ctx_bits & 2) != 0, (ctx_bits & 4) != 0, (ctx_bits & 8) != 0, false, policy_now};
    sca_restart_attrs in;
    in.struct_bytes = struct_bytes; in.reserved = reserved;
    in.neighbor_dist = (const double *)ptrs[0]; in.max_neighbors = (const int32_t *)ptrs[1]; in.time_step = (const double *)ptrs[2];
    in.time_horizon = (const double *)ptrs[3]; in.max_speed = (const double *)ptrs[4]; in.max_heading_change = (const double *)ptrs[5];
    in.dt_nominal = (const double *)ptrs[6]; in.turning_radius = (const double *)ptrs[7]; in.pitch_lo = (const double *)ptrs[8];
    in.pitch_hi = (const double *)ptrs[9];
    const AttrDefaults D{defaults[0], defaults[1], defaults[2], defaults[3], defaults[4], defaults[5], (int)defaults[6], defaults[7], defaults[8], defaults[9]};
    RestartAttrs R;
    const RestartAttrCheck k = restart_attrs_check(X, A, &in, D, &R);
    out[0] = (int)k.fault; out[1] = k.entry;
    const void *got[10] = {R.neighbor_dist, R.max_neighbors, R.time_step, R.time_horizon, R.max_speed, R.max_heading_change, R.dt_nominal,
                           R.turning_radius, R.pitch_lo, R.pitch_hi};
    out[2] = 0;
    for (int i = 0; i < 10; i++) if (got[i]) out[2] |= 1 << i;
    return restart_attrs_error_code(k.fault);
}
int attrs_struct_bytes(void) { return (int)sizeof(sca_restart_attrs); }

// every section of the restart's block as sca_restart_scenes lays it out for (max_n, max_m): begin and byte length of the agent sections,
// the new sizes, the obstacle sections and the attribute sections, in that order; returns the section count, *total: the block's bytes
int block_sections(int max_n, int max_m, int64_t *begin, int64_t *bytes, int64_t *total) {
    int k = 0;
    const RestartBlock B = restart_block_layout(max_n, max_m, 0);      // (no slot form: the path sections behind are empty, the block ends with the attributes')
    for (int s = 0; s < RS_SECTIONS; s++, k++) { begin[k] = B.L.off[s]; bytes[k] = restart_section_row_bytes(s) * (int64_t)max_n; }
    begin[k] = B.new_size_off; bytes[k] = (int64_t)sizeof(int32_t) * max_n; k++;
    for (int s = 0; s < RO_SECTIONS; s++, k++) { begin[k] = B.OL.off[s]; bytes[k] = restart_obs_section_bytes(s, max_n, max_m); }
    for (int s = 0; s < RA_SECTIONS; s++, k++) { begin[k] = B.AL.off[s]; bytes[k] = restart_attr_row_bytes(s) * (int64_t)max_n; }
    *total = B.AL.total;
    return k;
}
int attr_section_count(void) { return RA_SECTIONS; }

void *class_table_new(void) { return new ClassTable(); }
void class_table_free(void *t) { delete (ClassTable *)t; }
// trip: [n][3]; cls: [n] in / out; travels: [n] or NULL.  out: classes, many, moved
void class_table_update(void *t, int nscenes, const int32_t *offsets, const int32_t *size, const uint8_t *policy, const double *trip, int n, uint8_t *cls,
                        const uint8_t *travels, int *out) {
    std::vector<TrackTriple> tv((size_t)n);
    for (int i = 0; i < n; i++) tv[i] = TrackTriple{trip[3 * i], trip[3 * i + 1], trip[3 * i + 2]};
    const ClassUpdate u = scene_class_table(*(ClassTable *)t, nscenes, offsets, size, policy, tv.data(), cls, travels);
    out[0] = u.classes; out[1] = u.many ? 1 : 0; out[2] = u.moved ? 1 : 0;
}
// val: [16][3], users: [16]; returns the classes in use, *only: the one index in use or -1
int class_table_get(void *t, double *val, int32_t *users, int *many, int *only) {
    const ClassTable &T = *(ClassTable *)t;
    for (int k = 0; k < TRK_CLASS_CAP; k++) { val[3 * k] = T.val[k].R; val[3 * k + 1] = T.val[k].lo; val[3 * k + 2] = T.val[k].hi; users[k] = T.users[k]; }
    *many = T.many ? 1 : 0;
    return class_table_used(T, only);
}

}  // extern "C"

#ifdef SCENE_ATTRS_MAIN
// One fixed walk: three scenes of 4, 20 and 6 rows; checks with every kind of fault; the layout at two sizes; a class table that grows to
// the cap, passes it, comes back and ends on one class.  Every answer is printed: the test compares the lines with the same calls made
// through the shared library.
int main() {
    const int32_t off[4] = {0, 4, 24, 30};
    std::vector<uint8_t> pol(30, 0);
    for (int i = 0; i < 30; i++) pol[i] = (uint8_t)(i % 6);
    const double defaults[10] = {10.0, 0.1, 10.0, 1.0, 0.785398163397448279, 0.1, 16.0, 1.5, -0.5, 0.5};
    const int sb = attrs_struct_bytes();
    std::vector<double> good(24, 2.0), bad(24, 2.0), lo(24, -0.3), hi(24, 0.3);
    std::vector<int32_t> mn(24, 8);
    bad[17] = -1.0;
    std::vector<double> bad_tracked(24, 2.0);
    bad_tracked[17] = -1.0; bad_tracked[19] = -1.0;              // context rows 21 (policy 3: untracked, ignored) and 23 (policy 5)
    const int32_t ids[2] = {1, 0}, sizes[2] = {20, 4};
    int out[3];
    {
        const void *p[10] = {good.data(), mn.data(), nullptr, nullptr, nullptr, nullptr, nullptr, good.data(), lo.data(), hi.data()};
        for (int bytes : {sb, sb - 24, 8, 4, sb + 8, 12}) {
            const int rc = attrs_check(3, off, 1 | 4, pol.data(), 2, ids, sizes, nullptr, bytes, 0, p, defaults, out);
            std::printf("check bytes %d: rc %d fault %d entry %d read %d\n", bytes - sb, rc, out[0], out[1], out[2]);
        }
        int rc = attrs_check(3, off, 1, pol.data(), 2, ids, sizes, nullptr, sb, 0, p, defaults, out);
        std::printf("check no tracker: rc %d fault %d entry %d\n", rc, out[0], out[1]);
        rc = attrs_check(3, off, 1 | 4, pol.data(), 2, ids, sizes, nullptr, sb, 7, p, defaults, out);
        std::printf("check reserved: rc %d fault %d entry %d\n", rc, out[0], out[1]);
        p[0] = bad.data();
        rc = attrs_check(3, off, 1 | 4, pol.data(), 2, ids, sizes, nullptr, sb, 0, p, defaults, out);
        std::printf("check solver row: rc %d fault %d entry %d\n", rc, out[0], out[1]);
        p[0] = good.data(); p[7] = bad_tracked.data();
        rc = attrs_check(3, off, 1 | 4, pol.data(), 2, ids, sizes, nullptr, sb, 0, p, defaults, out);
        std::printf("check planner row: rc %d fault %d entry %d\n", rc, out[0], out[1]);
    }
    for (int max_n : {1, 130}) {
        int64_t begin[32], bytes[32], total = 0;
        const int k = block_sections(max_n, 9, begin, bytes, &total);
        std::printf("layout %d:", max_n);
        for (int i = 0; i < k; i++) std::printf(" %lld+%lld", (long long)begin[i], (long long)bytes[i]);
        std::printf(" total %lld\n", (long long)total);
    }
    void *t = class_table_new();
    std::vector<double> trip(90, 0.0);
    std::vector<uint8_t> cls(30, 0), all_tracked(30, 0);
    int32_t size[3] = {4, 20, 6};
    const auto show = [&](const char *what) {
        int u[3];
        class_table_update(t, 3, off, size, all_tracked.data(), trip.data(), 30, cls.data(), nullptr, u);
        double val[48]; int32_t users[16]; int many = 0, only = 0;
        const int used = class_table_get(t, val, users, &many, &only);
        std::printf("table %s: classes %d many %d moved %d used %d only %d cls", what, u[0], u[1], u[2], used, only);
        for (int i = 0; i < 30; i++) std::printf(" %d", cls[i]);
        std::printf("\n");
    };
    for (int i = 0; i < 30; i++) { trip[3 * i] = 1.0 + i % 3; trip[3 * i + 1] = -0.5; trip[3 * i + 2] = 0.5; }
    show("three");
    for (int i = 4; i < 24; i++) trip[3 * i] = 10.0 + i;              // scene 1: twenty triples of its own
    show("many");
    size[1] = 10;                                                     // ... of which ten rows stay occupied
    show("back");
    for (int i = 0; i < 30; i++) trip[3 * i] = 2.0;
    show("one");
    class_table_free(t);
    return 0;
}
#endif
