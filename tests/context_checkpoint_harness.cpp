// context_checkpoint_harness.cpp -- TEST-ONLY host build of the context checkpoints' pure rules (sca_checkpoint.h): the blob's layout
// (ctx_checkpoint_layout), THE check a load makes before any device work (ctx_checkpoint_check), the calls' rules
// (ctx_checkpoint_call_check), K4's counters for a blob's flags (ctx_checkpoint_stripes) and the row move both kernels are
// (ctx_checkpoint_move), run here over plain arrays of exactly the rows' sizes, so that all of it can be checked on a machine without a
// GPU.  The tracker record's field offsets come from the real type (sca_dubins.hpp), as sca_hip.hip takes them.  cx_make writes a small
// valid blob by the layout alone.  With -DCONTEXT_CHECKPOINT_MAIN it is a program of its own (for the sanitizers): every blob it checks
// or moves lives in a heap buffer of exactly the byte count it passes.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sca_dubins.hpp"
#include "sca_checkpoint.h"

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
CtxShape shape_of(const int32_t *s8) { return CtxShape{s8[0], s8[1], s8[2], s8[3], s8[4], s8[5], s8[6], s8[7]}; }
}  // namespace

extern "C" {

int cx_sections() { return CX_SECTIONS; }
int cx_header_bytes() { return (int)sizeof(CtxHeader); }
int cx_track_words() { return fields().words; }
void cx_track_offsets(int *out12) {
    const CkptTrackFields F = fields();
    const int v[12] = {F.use_dubins, F.plan_ok, F.h_ok, F.v_ok, F.h_mode, F.v_mode, F.plan_mode, F.iters, F.rounds, F.replans, F.count, F.next};
    for (int k = 0; k < 12; k++) out12[k] = v[k];
}
// shape8: n, trk_words, list_form, W, M, R, has_gate, has_clearance.  Returns the total, -1 for a shape the layout refuses
int64_t cx_layout(const int32_t *shape8, int64_t *off, int64_t *len) {
    const CtxShape S = shape_of(shape8);
    if (!ctx_shape_ok(S)) return -1;
    const CtxLayout L = ctx_checkpoint_layout(S);
    for (int s = 0; s < CX_SECTIONS; s++) { off[s] = L.off[s]; len[s] = L.len[s]; }
    return L.total;
}
// the header's checksum from the bytes as they stand (a blob damaged on purpose in ONE place reaches the rule for that place)
void cx_seal(void *blob, int64_t bytes) {
    unsigned char *b = (unsigned char *)blob;
    put<uint64_t>(b + offsetof(CtxHeader, checksum), scene_checkpoint_sum(b + sizeof(CtxHeader), bytes - (int64_t)sizeof(CtxHeader)));
}
// A valid blob for the shape into blob[total].  Row i: at (i, 2 i, 5), radius 0.5, policy policy[i], goal (i, 0, 1), pref_speed 1,
// max_run_dist 50, z-axis i & 1, every third row arrived (flag 1), step_num 11; the permutation reversed.  Tracker: nbr0 -1, a plan of 40
// samples, the cursor at 7, words "LSL" / "RSR".  Lists: slot form len = i % (W + 1), rem = min(len, i % 2), the rooms 0.5 k; block form
// rem = i % 3 (lists of 2 .. as the caller says).  Tables: first_ok 0, first_fail -1, cursor = flying = i % (M + 1) - 1, ended i % 4,
// collected min(ended, i % 2), live from the flag, the rings' ids, the totals 1 .. 8.  Gate: every fifth row waits for entry 0 with verdict
// 1, refusals i % 2.  Closest approach: partner (i + 1) % n at step 3, no obstacle.  clear_step 6, updates 6.  Returns the total.
int64_t cx_make(const int32_t *shape8, const uint8_t *policy, void *blob) {
    const CkptTrackFields F = fields();
    const CtxShape S = shape_of(shape8);
    const CtxLayout L = ctx_checkpoint_layout(S);
    const int n = S.n, M = S.M;
    unsigned char *b = (unsigned char *)blob;
    std::memset(b, 0, (size_t)L.total);
    for (int i = 0; i < n; i++) {
        const uint32_t flag = i % 3 == 2 ? 1u : 0u;
        b[L.off[CX_POLICY] + i] = policy[i];
        unsigned char *r = b + L.off[CX_REC] + (int64_t)CKPT_REC_BYTES * i;
        put<double>(r, (double)i); put<double>(r + 8, 2.0 * i); put<double>(r + 16, 5.0);
        put<float>(r + 24, 0.25f); put<uint32_t>(r + 36, flag); put<double>(r + 40, 0.5);
        put<double>(b + L.off[CX_HEADING] + 24 * (int64_t)i, 1.0);
        put<double>(b + L.off[CX_GOAL] + 24 * (int64_t)i, (double)i); put<double>(b + L.off[CX_GOAL] + 24 * (int64_t)i + 16, 1.0);
        put<double>(b + L.off[CX_PREF_SPEED] + 8 * (int64_t)i, 1.0);
        put<double>(b + L.off[CX_MAX_RUN_DIST] + 8 * (int64_t)i, 50.0);
        put<uint32_t>(b + L.off[CX_ZAXIS] + 4 * (int64_t)i, (uint32_t)(i & 1));
        put<uint32_t>(b + L.off[CX_VPREF_MODE] + 4 * (int64_t)i, policy[i] == 0 || policy[i] == 5 ? 1u : 0u);
        put<double>(b + L.off[CX_TOTAL_DIST] + 8 * (int64_t)i, 0.5 * i);
        put<int32_t>(b + L.off[CX_STEP_NUM] + 4 * (int64_t)i, 11);
        put<int32_t>(b + L.off[CX_PERM] + 4 * (int64_t)i, n - 1 - i);
        if (S.trk_words) {
            put<double>(b + L.off[CX_GOAL_HEADING] + 24 * (int64_t)i + 8, 1.0);
            put<double>(b + L.off[CX_TRK_NBR0] + 8 * (int64_t)i, -1.0);
            unsigned char *t = b + L.off[CX_TRACK] + 4 * (int64_t)S.trk_words * i;
            t[F.use_dubins] = 1; t[F.plan_ok] = 1; t[F.h_ok] = 1; t[F.v_ok] = 1;
            std::memcpy(t + F.h_mode, "LSL", 3); std::memcpy(t + F.v_mode, "RSR", 3); std::memcpy(t + F.plan_mode, "LSLRSR", 6);
            put<int32_t>(t + F.iters, 48); put<int32_t>(t + F.rounds, 0); put<int32_t>(t + F.replans, 2);
            put<int64_t>(t + F.count, 40); put<int64_t>(t + F.next, 7);
        }
        if (S.list_form != CTXCK_LISTS_NONE) {
            int32_t rem = i % 3;
            if (S.list_form == CTXCK_LISTS_SLOTS) {
                const int32_t len = i % (S.W + 1);
                rem = len < i % 2 ? len : i % 2;
                put<int32_t>(b + L.off[CX_LEN] + 4 * (int64_t)i, len);
                for (int k = 0; k < 3 * S.W; k++) put<double>(b + L.off[CX_ROOMS] + 8 * (3 * (int64_t)S.W * i + k), 0.5 * k);
            }
            put<int32_t>(b + L.off[CX_REM] + 4 * (int64_t)i, rem);
            for (int k = 0; k < 3; k++) put<double>(b + L.off[CX_NOW_GOAL] + 24 * (int64_t)i + 8 * k, __builtin_nan(""));
        }
        if (M > 0) {
            unsigned char *w = b + L.off[CX_MS_WORDS];
            const int32_t cur = i % (M + 1) - 1, ended = i % 4;
            const int32_t v[CTXCK_MS_WORDS] = {0, -1, cur, cur, ended, ended < i % 2 ? ended : i % 2, flag ? 0 : 1};
            for (int c = 0; c < CTXCK_MS_WORDS; c++) put<int32_t>(w + 4 * ((int64_t)c * n + i), v[c]);
            for (int k = 0; k < S.R; k++) put<int32_t>(b + L.off[CX_MS_RESULTS] + CTXCK_RESULT_BYTES * ((int64_t)S.R * i + k), i);
        }
        if (S.has_gate) {
            unsigned char *w = b + L.off[CX_GATE_WORDS];
            const int32_t wait = i % 5 == 0 ? 0 : -1;
            const int32_t v[CTXCK_GATE_WORDS] = {wait, wait >= 0 ? 1 : 0, i % 2, 0};
            for (int c = 0; c < CTXCK_GATE_WORDS; c++) put<int32_t>(w + 4 * ((int64_t)c * n + i), v[c]);
        }
        if (S.has_clearance) {
            unsigned char *r2 = b + L.off[CX_CLEAR] + CTXCK_CLEAR_BYTES * (int64_t)i;
            put<double>(r2, 0.75); put<double>(r2 + 8, __builtin_inf());
            put<int32_t>(r2 + 16, n > 1 ? (i + 1) % n : -1); put<int32_t>(r2 + 20, n > 1 ? 3 : 0); put<int32_t>(r2 + 24, -1); put<int32_t>(r2 + 28, 0);
        }
    }
    if (M > 0) for (int k = 0; k < CTXCK_TOTAL_WORDS; k++) put<uint64_t>(b + L.off[CX_MS_TOTALS] + 8 * k, (uint64_t)(k + 1));
    if (S.has_gate) for (int k = 0; k < CTXCK_TOTAL_WORDS; k++) put<uint64_t>(b + L.off[CX_GATE_TOTALS] + 8 * k, (uint64_t)(10 + k));
    CtxHeader H{};
    H.magic = CTXCK_MAGIC; H.format = CTXCK_FORMAT; H.lib_version = CKPT_LIB_VERSION; H.n = n; H.trk_words = S.trk_words; H.rec_bytes = CKPT_REC_BYTES;
    H.present = ctx_shape_present(S); H.list_form = S.list_form; H.W = S.W; H.M = S.M; H.R = S.R; H.clear_step = S.has_clearance ? 6 : 0;
    H.updates = M > 0 ? 6 : 0; H.total_bytes = L.total;
    std::memcpy(b, &H, sizeof H);
    cx_seal(b, L.total);
    return L.total;
}
// with_ctx == 0: the envelope and the payload alone (sca_context_checkpoint_info).  out: fault, entry; returns the error code
int cx_check(const void *blob, int64_t bytes, int with_ctx, const int32_t *shape8, const uint8_t *policy, const int32_t *block_len, int n_obs, int64_t *out) {
    CtxExpect X{};
    if (with_ctx) { X.shape = shape_of(shape8); X.policy = policy; X.block_len = block_len; X.n_obs = n_obs; }
    const CtxCheck k = ctx_checkpoint_check(blob, bytes, fields(), with_ctx ? &X : nullptr, nullptr);
    out[0] = (int64_t)k.fault; out[1] = k.entry;
    return ctx_checkpoint_error_code(k.fault);
}
int cx_call(int agents, int state, int mid_step, int scenes, int comm, int partition, int n, int shard_count, int buffer, int *fault) {
    const CtxCallFault f = ctx_checkpoint_call_check(CtxCallState{agents != 0, state != 0, mid_step != 0, scenes != 0, comm != 0, partition != 0, n, shard_count}, buffer != 0);
    *fault = (int)f;
    return ctx_checkpoint_call_error_code(f);
}
// The kernels' row move over plain arrays: `blob` (a valid one for the shape) is loaded by `threads` threads into zeroed arrays of exactly
// the rows' sizes, then saved from them into out[total] (zeroed; the host's part -- the header and the policies -- copied over as
// sca_save_context does).  live[n] (with tables) and done[256] receive what the load left in the "entered live" column and K4's stripes.
void cx_roundtrip(const int32_t *shape8, const void *blob, int threads, void *out, int32_t *live, int32_t *done) {
    const CtxShape S = shape_of(shape8);
    const CtxLayout L = ctx_checkpoint_layout(S);
    const size_t n = (size_t)S.n;
    const bool trk = S.trk_words > 0, lists = S.list_form != CTXCK_LISTS_NONE, slots = S.list_form == CTXCK_LISTS_SLOTS, tables = S.M > 0;
    std::vector<PubRec> rec(n);
    std::memset(rec.data(), 0, sizeof(PubRec) * n);
    std::vector<double> heading(3 * n), goal(3 * n), ps(n), mrd(n), vpref(3 * n), td(n), gh(trk ? 3 * n : 0), nbr0(trk ? n : 0), now_goal(lists ? 3 * n : 0), rooms(slots ? 3 * n * (size_t)S.W : 0);
    std::vector<int32_t> step(n), status(n), perm(n), done_count((size_t)CTXCK_STRIPES * CTXCK_STRIPE_PITCH, -7), rem(lists ? n : 0), len(slots ? n : 0);
    std::vector<int32_t> msw(tables ? n * CTXCK_MS_WORDS : 0), gw(S.has_gate ? n * CTXCK_GATE_WORDS : 0);
    std::vector<uint8_t> zaxis(n), mode(n);
    std::vector<uint32_t> track(trk ? n * (size_t)S.trk_words : 0);
    std::vector<sca_mission_result> results(tables ? n * (size_t)S.R : 0);
    std::vector<unsigned long long> mst(tables ? CTXCK_TOTAL_WORDS : 0), mgt(S.has_gate ? CTXCK_TOTAL_WORDS : 0);
    std::vector<sca_scene_clearance> clear(S.has_clearance ? n : 0);
    if (!results.empty()) std::memset(results.data(), 0, sizeof(sca_mission_result) * results.size());
    if (!clear.empty()) std::memset(clear.data(), 0, sizeof(sca_scene_clearance) * clear.size());
    const auto ptr = [](auto &v) { return v.empty() ? nullptr : v.data(); };
    CtxDev d{};
    d.rec = rec.data(); d.heading = heading.data(); d.goal = goal.data(); d.pref_speed = ps.data(); d.max_run_dist = mrd.data(); d.vpref_ext = vpref.data(); d.total_dist = td.data();
    d.step_num = step.data(); d.status = status.data(); d.aperm = perm.data(); d.zaxis = zaxis.data(); d.vpref_mode = mode.data(); d.done_count = done_count.data();
    d.trk_goal_heading = ptr(gh); d.trk_nbr0 = ptr(nbr0); d.trk_st = (ctx_u32 *)ptr(track); d.rem = ptr(rem); d.now_goal = ptr(now_goal); d.len = ptr(len); d.rooms = ptr(rooms);
    d.ms_words = ptr(msw); d.ms_results = ptr(results); d.ms_totals = ptr(mst); d.gate_words = ptr(gw); d.gate_totals = ptr(mgt); d.clear = ptr(clear);
    std::vector<unsigned char> in((const unsigned char *)blob, (const unsigned char *)blob + L.total);     // exactly the blob's bytes
    int32_t stripes[CTXCK_STRIPES];
    ctx_checkpoint_stripes(in.data(), L, S.n, stripes);
    for (int t = 0; t < threads; t++) ctx_checkpoint_move<true>(d, in.data(), L, S, stripes, t, threads);
    for (int s = 0; s < CTXCK_STRIPES; s++) done[s] = done_count[(size_t)s * CTXCK_STRIPE_PITCH];
    if (tables) for (size_t i = 0; i < n; i++) live[i] = msw[CTXCK_MS_LIVE * n + i];
    std::vector<unsigned char> o((size_t)L.total, 0);
    for (int t = 0; t < threads; t++) ctx_checkpoint_move<false>(d, o.data(), L, S, nullptr, t, threads);
    std::memcpy(o.data(), in.data(), sizeof(CtxHeader));
    std::memcpy(o.data() + L.off[CX_POLICY], in.data() + L.off[CX_POLICY], n);
    std::memcpy(out, o.data(), (size_t)L.total);
}

}  // extern "C"

#ifdef CONTEXT_CHECKPOINT_MAIN
namespace {
// the check on a heap buffer of exactly `bytes` bytes holding the blob's first `bytes` bytes
void run(const char *what, const std::vector<unsigned char> &blob, int64_t bytes, int with_ctx, const int32_t *shape8, const uint8_t *policy, const int32_t *block_len, int n_obs) {
    unsigned char *exact = new unsigned char[(size_t)(bytes > 0 ? bytes : 1)];
    std::memcpy(exact, blob.data(), (size_t)bytes);
    int64_t out[2];
    const int rc = cx_check(exact, bytes, with_ctx, shape8, policy, block_len, n_obs, out);
    std::printf("%s: rc %d fault %d entry %d\n", what, rc, (int)out[0], (int)out[1]);
    delete[] exact;
}
}  // namespace
int main() {
    const int N = 7;
    const uint8_t pol[N] = {0, 1, 5, 3, 4, 0, 2};
    const int tw = cx_track_words();
    const int32_t full[8] = {N, tw, CTXCK_LISTS_SLOTS, 3, 2, 2, 1, 1};
    int64_t off[CX_SECTIONS], ln[CX_SECTIONS];
    const int64_t total = cx_layout(full, off, ln);
    std::vector<unsigned char> good((size_t)total);
    cx_make(full, pol, good.data());
    int fo[12];
    cx_track_offsets(fo);
    run("valid", good, total, 1, full, pol, nullptr, 0);
    run("valid, no context", good, total, 0, nullptr, nullptr, nullptr, 0);
    run("short", good, 127, 0, nullptr, nullptr, nullptr, 0);
    run("one byte less", good, total - 1, 0, nullptr, nullptr, nullptr, 0);
    run("header alone", good, 128, 0, nullptr, nullptr, nullptr, 0);
    for (int s = 1; s < CX_SECTIONS; s++) {                              // truncation at every section boundary
        char what[32];
        std::snprintf(what, sizeof what, "cut at %d", s);
        run(what, good, off[s], 0, nullptr, nullptr, nullptr, 0);
    }
    struct Byte { int64_t at; unsigned char v; };
    auto damaged = [&](const char *what, std::vector<Byte> bytes, bool seal) {
        std::vector<unsigned char> b = good;
        for (const Byte &x : bytes) b[(size_t)x.at] = x.v;
        if (seal) cx_seal(b.data(), total);
        run(what, b, total, 1, full, pol, nullptr, 0);
    };
    damaged("magic", {{0, 0}}, true);
    damaged("checksum", {{off[CX_HEADING] + 3, 1}}, false);
    damaged("permutation", {{off[CX_PERM], 5}}, true);
    damaged("len", {{off[CX_LEN] + 4, 4}}, true);
    damaged("rem", {{off[CX_REM] + 4 * 2, 3}}, true);
    damaged("cursor", {{off[CX_MS_WORDS] + 4 * (2 * N + 1), 2}}, true);
    damaged("collected", {{off[CX_MS_WORDS] + 4 * (5 * N + 0), 1}}, true);
    damaged("verdict", {{off[CX_GATE_WORDS] + 4 * (1 * N + 3), 5}}, true);
    damaged("partner", {{off[CX_CLEAR] + 32 * 2 + 16, (unsigned char)N}}, true);
    damaged("tracker next", {{off[CX_TRACK] + 4 * (int64_t)tw * 3 + fo[11], 41}}, true);
    // the row move, in buffers of exactly the rows' sizes, by 1 and by 5 threads
    for (int threads : {1, 5}) {
        std::vector<unsigned char> back((size_t)total);
        std::vector<int32_t> live(N), done(CTXCK_STRIPES);
        cx_roundtrip(full, good.data(), threads, back.data(), live.data(), done.data());
        std::printf("roundtrip by %d: %s, done %d %d %d\n", threads, std::memcmp(back.data(), good.data(), (size_t)total) == 0 ? "equal" : "DIFFERENT", done[0], done[1], done[2]);
    }
    const int32_t bare[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    const int64_t small = cx_layout(bare, off, ln);
    std::vector<unsigned char> one((size_t)small), back((size_t)small);
    const uint8_t p1[1] = {3};
    cx_make(bare, p1, one.data());
    run("one row", one, small, 1, bare, p1, nullptr, 0);
    int32_t live1[1], done1[CTXCK_STRIPES];
    cx_roundtrip(bare, one.data(), 3, back.data(), live1, done1);
    std::printf("one row roundtrip: %s\n", std::memcmp(back.data(), one.data(), (size_t)small) == 0 ? "equal" : "DIFFERENT");
    std::printf("bytes %lld %lld\n", (long long)total, (long long)small);
    return 0;
}
#endif
