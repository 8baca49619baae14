// scene_checkpoint_harness.cpp -- TEST-ONLY host build of the scene checkpoints' pure rules (sca_scenes.h): the blob's layout
// (scene_checkpoint_layout), its checksum, THE check a load makes before any device work (scene_checkpoint_check) and the rules of the
// two calls (scene_checkpoint_call_check), so that all of it can be checked on a machine without a GPU.  The tracker record's field
// offsets come from the real type (sca_dubins.hpp), as sca_hip.hip takes them.  ckpt_make writes a small valid blob by the layout alone.
// With -DSCENE_CHECKPOINT_MAIN it is a program of its own (for the sanitizers): every blob it checks lives in a heap buffer of exactly the
// byte count it passes, so a check that reads past the bytes it was given is the sanitizer's.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sca_dubins.hpp"
#include "sca_scenes.h"

using namespace sca;

namespace {
CkptTrackFields fields() {
    using sca_dubins::AgentTrack; using sca_dubins::Plan3D; using sca_dubins::Maneuver2D;
    const int plan = (int)offsetof(AgentTrack, plan);
    CkptTrackFields F;
    F.words = (int)(sizeof(AgentTrack) / 4);
    F.use_dubins = (int)offsetof(AgentTrack, is_use_dubins);
    F.plan_ok = plan + (int)offsetof(Plan3D, ok);
    F.h_ok = plan + (int)offsetof(Plan3D, h) + (int)offsetof(Maneuver2D, ok); F.v_ok = plan + (int)offsetof(Plan3D, v) + (int)offsetof(Maneuver2D, ok);
    F.h_mode = plan + (int)offsetof(Plan3D, h) + (int)offsetof(Maneuver2D, mode); F.v_mode = plan + (int)offsetof(Plan3D, v) + (int)offsetof(Maneuver2D, mode);
    F.plan_mode = plan + (int)offsetof(Plan3D, mode);
    F.iters = plan + (int)offsetof(Plan3D, iters); F.rounds = plan + (int)offsetof(Plan3D, rounds); F.replans = (int)offsetof(AgentTrack, replans);
    F.count = plan + (int)offsetof(Plan3D, count); F.next = (int)offsetof(AgentTrack, next);
    return F;
}
template <class T> void put(unsigned char *at, T v) { std::memcpy(at, &v, sizeof v); }
}  // namespace

extern "C" {

int ckpt_sections() { return CK_SECTIONS; }
int ckpt_header_bytes() { return (int)sizeof(CkptHeader); }
int ckpt_track_words() { return fields().words; }
// the byte offsets of the tracker record's checked fields, in CkptTrackFields' order behind `words`
void ckpt_track_offsets(int *out12) {
    const CkptTrackFields F = fields();
    const int v[12] = {F.use_dubins, F.plan_ok, F.h_ok, F.v_ok, F.h_mode, F.v_mode, F.plan_mode, F.iters, F.rounds, F.replans, F.count, F.next};
    for (int k = 0; k < 12; k++) out12[k] = v[k];
}
int64_t ckpt_layout(int size, int trk_words, int has_paths, int64_t *off, int64_t *len) {
    const CkptLayout L = scene_checkpoint_layout(size, trk_words, has_paths);
    for (int s = 0; s < CK_SECTIONS; s++) { off[s] = L.off[s]; len[s] = L.len[s]; }
    return L.total;
}
uint64_t ckpt_sum(const void *bytes, int64_t count) { return scene_checkpoint_sum(bytes, count); }
// the header's checksum from the bytes as they stand (a blob damaged on purpose in ONE place reaches the rule for that place)
void ckpt_seal(void *blob, int64_t bytes) {
    unsigned char *b = (unsigned char *)blob;
    put<uint64_t>(b + offsetof(CkptHeader, checksum), scene_checkpoint_sum(b + sizeof(CkptHeader), bytes - (int64_t)sizeof(CkptHeader)));
}
// A valid blob of `size` rows into blob[total]: row i at (i, 2 i, 5), radius 0.5, policy policy[i]; every third row arrived (flag 1); the
// permutation reversed; the tracker records (where tracked != 0) with a plan of 40 samples, the cursor at 7, words "LSL" / "RSR"; the
// cursors (where has_paths) rem = i % 3 and now_goal None.  steps = 11, prev = live.  Returns the total.
int64_t ckpt_make(int size, const uint8_t *policy, int tracked, int has_paths, void *blob) {
    const CkptTrackFields F = fields();
    const int tw = tracked ? F.words : 0;
    const CkptLayout L = scene_checkpoint_layout(size, tw, has_paths);
    unsigned char *b = (unsigned char *)blob;
    std::memset(b, 0, (size_t)L.total);
    int live = 0;
    for (int i = 0; i < size; i++) {
        b[L.off[CK_POLICY] + i] = policy[i];
        unsigned char *r = b + L.off[CK_REC] + (int64_t)CKPT_REC_BYTES * i;
        put<double>(r, (double)i); put<double>(r + 8, 2.0 * i); put<double>(r + 16, 5.0);
        put<float>(r + 24, 0.25f); put<uint32_t>(r + 36, i % 3 == 2 ? 1u : 0u); put<double>(r + 40, 0.5);
        live += i % 3 == 2 ? 0 : 1;
        put<double>(b + L.off[CK_TOTAL_DIST] + 8 * (int64_t)i, 0.5 * i);
        put<int32_t>(b + L.off[CK_STEP_NUM] + 4 * (int64_t)i, 11);
        put<int32_t>(b + L.off[CK_PERM] + 4 * (int64_t)i, size - 1 - i);
        put<uint32_t>(b + L.off[CK_VPREF_MODE] + 4 * (int64_t)i, policy[i] == 0 || policy[i] == 5 ? 1u : 0u);
        if (tw) {
            put<double>(b + L.off[CK_TRK_NBR0] + 8 * (int64_t)i, -1.0);
            unsigned char *t = b + L.off[CK_TRACK] + 4 * (int64_t)tw * i;
            t[F.use_dubins] = 1; t[F.plan_ok] = 1; t[F.h_ok] = 1; t[F.v_ok] = 1;
            std::memcpy(t + F.h_mode, "LSL", 3); std::memcpy(t + F.v_mode, "RSR", 3); std::memcpy(t + F.plan_mode, "LSLRSR", 6);
            put<int32_t>(t + F.iters, 48); put<int32_t>(t + F.rounds, 0); put<int32_t>(t + F.replans, 2);
            put<int64_t>(t + F.count, 40); put<int64_t>(t + F.next, 7);
        }
        if (has_paths) {
            put<int32_t>(b + L.off[CK_REM] + 4 * (int64_t)i, i % 3);
            for (int k = 0; k < 3; k++) put<double>(b + L.off[CK_NOW_GOAL] + 24 * (int64_t)i + 8 * k, __builtin_nan(""));
        }
    }
    CkptHeader H{};
    H.magic = CKPT_MAGIC; H.format = CKPT_FORMAT; H.lib_version = CKPT_LIB_VERSION; H.size = size; H.trk_words = tw; H.rec_bytes = CKPT_REC_BYTES;
    H.has_track = tw ? 1 : 0; H.has_paths = has_paths; H.steps = 11; H.live = live; H.prev = live; H.total_bytes = L.total;
    std::memcpy(b, &H, sizeof H);
    ckpt_seal(b, L.total);
    return L.total;
}
// with_scene == 0: the envelope and the payload alone (sca_scene_checkpoint_info).  out: fault, entry; returns the error code
int ckpt_check(const void *blob, int64_t bytes, int with_scene, int scene_size, const uint8_t *policy, int tracker_on, int paths_on, const int32_t *path_len, int *out) {
    const CkptScene X{scene_size, policy, tracker_on != 0, paths_on != 0, path_len};
    const CkptCheck k = scene_checkpoint_check(blob, bytes, fields(), with_scene ? &X : nullptr, nullptr);
    out[0] = (int)k.fault; out[1] = k.entry;
    return scene_checkpoint_error_code(k.fault);
}
int ckpt_call(int nscenes, int state_set, int scene_begun, int count, const int32_t *scene_ids, const void *const *bufs, const int64_t *sizes, int *out) {
    const CkptCallCheck k = scene_checkpoint_call_check(nscenes, state_set != 0, scene_begun != 0, count, scene_ids, bufs, sizes);
    out[0] = (int)k.fault; out[1] = k.entry;
    return scene_checkpoint_call_error_code(k.fault);
}

}  // extern "C"

#ifdef SCENE_CHECKPOINT_MAIN
namespace {
// the check on a heap buffer of exactly `bytes` bytes holding the blob's first `bytes` bytes
void run(const char *what, const std::vector<unsigned char> &blob, int64_t bytes, int with_scene, int scene_size, const uint8_t *policy, int tracker_on, int paths_on,
         const int32_t *path_len) {
    unsigned char *exact = new unsigned char[(size_t)(bytes > 0 ? bytes : 1)];
    std::memcpy(exact, blob.data(), (size_t)bytes);
    int out[2];
    const int rc = ckpt_check(exact, bytes, with_scene, scene_size, policy, tracker_on, paths_on, path_len, out);
    std::printf("%s: rc %d fault %d entry %d\n", what, rc, out[0], out[1]);
    delete[] exact;
}
}  // namespace
int main() {
    const int N = 5;
    const uint8_t pol[N] = {0, 1, 5, 3, 4};
    const int32_t len[N] = {2, 2, 2, 2, 2};
    int64_t off[CK_SECTIONS], ln[CK_SECTIONS];
    const int tw = ckpt_track_words();
    const int64_t total = ckpt_layout(N, tw, 1, off, ln);
    std::vector<unsigned char> good((size_t)total);
    ckpt_make(N, pol, 1, 1, good.data());
    int fo[12];
    ckpt_track_offsets(fo);
    run("valid", good, total, 1, N, pol, 1, 1, len);
    run("valid, no scene", good, total, 0, 0, nullptr, 0, 0, nullptr);
    run("short", good, 63, 0, 0, nullptr, 0, 0, nullptr);
    run("one byte less", good, total - 1, 0, 0, nullptr, 0, 0, nullptr);
    run("header alone", good, 64, 0, 0, nullptr, 0, 0, nullptr);
    struct Byte { int64_t at; unsigned char v; };
    auto damaged = [&](const char *what, std::vector<Byte> bytes, bool seal) {
        std::vector<unsigned char> b = good;
        for (const Byte &x : bytes) b[(size_t)x.at] = x.v;
        if (seal) ckpt_seal(b.data(), total);
        run(what, b, total, 1, N, pol, 1, 1, len);
    };
    damaged("magic", {{0, 0}}, true);
    damaged("format", {{4, 9}}, true);
    damaged("checksum", {{off[CK_HEADING] + 3, 1}}, false);
    damaged("size", {{12, 6}}, true);                                  // the header says six rows: the byte count is five rows'
    damaged("permutation", {{off[CK_PERM], 3}}, true);                 // position 0 holds 3, as position 1 does
    damaged("permutation range", {{off[CK_PERM] + 1, 1}}, true);       // position 0 holds 260
    damaged("flags", {{off[CK_REC] + 36, 8}}, true);
    damaged("position", {{off[CK_REC] + CKPT_REC_BYTES * 2 + 6, 0xf0}, {off[CK_REC] + CKPT_REC_BYTES * 2 + 7, 0x7f}}, true);   // row 2: x = +inf
    damaged("cursor", {{off[CK_REM] + 4, 3}}, true);                   // row 1: rem 3 above its list's 2
    damaged("tracker next", {{off[CK_TRACK] + 4 * (int64_t)tw * 3 + fo[11], 41}}, true);        // row 3: the cursor behind the 40 samples
    damaged("tracker count", {{off[CK_TRACK] + 4 * (int64_t)tw * 4 + fo[10] + 7, 0x80}}, true); // row 4: a negative count
    damaged("tracker word", {{off[CK_TRACK] + fo[4], 'X'}}, true);
    damaged("tracker bool", {{off[CK_TRACK] + fo[0], 2}}, true);
    const uint8_t other[N] = {0, 1, 5, 3, 3};
    run("policy", good, total, 1, N, other, 1, 1, len);
    run("scene size", good, total, 1, N + 1, pol, 1, 1, len);
    run("tracker off", good, total, 1, N, pol, 0, 1, len);
    run("no lists", good, total, 1, N, pol, 1, 0, nullptr);
    // a blob without tracker records and cursors, one row
    const int64_t small = ckpt_layout(1, 0, 0, off, ln);
    std::vector<unsigned char> one((size_t)small);
    const uint8_t p1[1] = {3};
    ckpt_make(1, p1, 0, 0, one.data());
    run("one row", one, small, 1, 1, p1, 1, 0, nullptr);
    std::printf("bytes %lld %lld\n", (long long)total, (long long)small);
    return 0;
}
#endif
