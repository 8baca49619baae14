// sca_checkpoint.h -- context checkpoints (sca_save_context / sca_load_context): the blob's layout, THE check a load makes before any
// device work, the fault -> code map and the row move both kernels are (sca_checkpoint.hip.h), as pure functions.  No HIP, no sca_ctx:
// sca_hip.hip calls them and turns their answers into error codes and messages; tests/context_checkpoint_harness.cpp checks them -- the
// row move over plain arrays -- without a GPU.
//
// A blob is a plain context's whole MUTABLE state: what sca_set_state / sca_set_kd_perm / sca_set_path_state can set, plus every word
// respawn_write_row (sca_respawn.h), a take (sca_missions.hip.h, sca_mission_gate.hip.h), the device tracker and k_clearance leave in the
// rows between two steps.  The run's definition (sca_create's parameters, policies, attributes, obstacles, the tracker's parameters, the
// lists as set, the tables and their lists, the gate's margin and cap) is not in it: a resume is the definition, then a load.  The blob
// is pointer-free and speaks of rows 0 .. n-1, so it loads into any context of max_agents >= n, in any process.
// Layout: a fixed 128-byte header, then the sections in the order of CtxSection, each on a 16-byte boundary, offsets 64-bit; a section
// the blob does not carry has length 0.  Everything per row is whole 4-byte words -- the records 16-byte pieces -- so the kernels move a
// section as consecutive words by consecutive lanes; the byte-sized columns (z-axis, vpref_mode) travel as a word per row for that reason.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/sca_hip.h"
#include "sca_core.h"
#include "sca_scenes.h"
#include "sca_vacancy.h"

namespace sca {

constexpr uint32_t CTXCK_MAGIC = 0x504b4343u;      // "CCKP"
constexpr int32_t CTXCK_FORMAT = 1;
enum CtxPresent : uint32_t { CTXCK_HAS_TRACKER = 1, CTXCK_HAS_LISTS = 2, CTXCK_HAS_TABLES = 4, CTXCK_HAS_GATE = 8, CTXCK_HAS_CLEARANCE = 16, CTXCK_HAS_ALL = 31,
                             CTXCK_HAS_VACANCY = 32 };     // rows of the blob are vacant (sca_vacancy.h): set exactly when occupied < n at the save, by the _opt entry points alone
enum CtxListForm : int32_t { CTXCK_LISTS_NONE = 0, CTXCK_LISTS_BLOCK = 1, CTXCK_LISTS_SLOTS = 2 };
struct CtxHeader {                                 // 128 bytes
    uint32_t magic; int32_t format, lib_version, n;
    int32_t trk_words, rec_bytes; uint32_t present; int32_t list_form;
    int32_t W, M, R, clear_step;                   // room per row (slot form), the tables' M and R, k_clearance's step number
    int32_t state_fresh, occupied;                 // 1: taken directly behind sca_set_state -- the one-time obstacle check is still pending; the occupied rows m with
                                                   // CTXCK_HAS_VACANCY (1 .. n-1), else 0 -- the word was reserved and 0 before: a blob without vacant rows is what it always was
    int64_t updates;                               // env updates since sca_set_missions
    int64_t total_bytes;                           // header + sections
    uint64_t checksum;                             // scene_checkpoint_sum over the bytes behind the header
    int64_t reserved[6];
};
static_assert(sizeof(CtxHeader) == 128 && offsetof(CtxHeader, checksum) == 72, "the context checkpoint's header is 128 bytes");
enum CtxSection : int {
    CX_POLICY = 0,                                 // [n] u8: the rows' policies, which the loading context must have (written by the host, compared, not loaded)
    CX_REC, CX_HEADING, CX_GOAL, CX_PREF_SPEED, CX_MAX_RUN_DIST, CX_ZAXIS, CX_VPREF_EXT, CX_VPREF_MODE, CX_TOTAL_DIST, CX_STEP_NUM, CX_STATUS, CX_PERM,
    CX_GOAL_HEADING, CX_TRK_NBR0, CX_TRACK,        // with the device tracker
    CX_REM, CX_NOW_GOAL,                           // with lists
    CX_LEN, CX_ROOMS,                              // ... in slot form: the lengths and the rooms whole, W points a row
    CX_MS_WORDS, CX_MS_RESULTS, CX_MS_TOTALS,      // with tables: the seven words per row (column-major, as the device holds them), the rings, the totals
    CX_GATE_WORDS, CX_GATE_TOTALS,                 // with a gate: its four words per row, its totals
    CX_CLEAR,                                      // with closest-approach records
    CX_SECTIONS };
constexpr int CTXCK_MS_WORDS = 7, CTXCK_MS_LIVE = 6, CTXCK_GATE_WORDS = 4, CTXCK_TOTAL_WORDS = 8;    // (sca_hip.hip asserts them against MissionWord / MissionGateWord / MST_WORDS / MGT_WORDS)
constexpr int CTXCK_MS_FIRST_OK = 0, CTXCK_MS_FIRST_FAIL = 1, CTXCK_MS_CURSOR = 2, CTXCK_MS_FLYING = 3, CTXCK_MS_ENDED = 4, CTXCK_MS_COLLECTED = 5;
constexpr int CTXCK_GATE_WAITING = 0, CTXCK_GATE_VERDICT = 1, CTXCK_GATE_REFUSALS = 2;
constexpr int64_t CTXCK_RESULT_BYTES = 96, CTXCK_CLEAR_BYTES = 32;
static_assert(sizeof(sca_mission_result) == CTXCK_RESULT_BYTES && sizeof(sca_scene_clearance) == CTXCK_CLEAR_BYTES, "the records travel as 16-byte pieces");
constexpr int CTXCK_STRIPES = 256, CTXCK_STRIPE_PITCH = 32;      // K4's striped done_count (DeviceView::done_count)

// what a layout depends on (include/sca_hip.h: sca_context_checkpoint_shape without its struct_bytes)
struct CtxShape { int32_t n, trk_words, list_form, W, M, R, has_gate, has_clearance; };
struct CtxLayout { int64_t off[CX_SECTIONS]; int64_t len[CX_SECTIONS]; int64_t total; };
inline bool ctx_shape_ok(const CtxShape &S) {
    const bool slots = S.list_form == CTXCK_LISTS_SLOTS, tables = S.M > 0;
    return S.n >= 1 && S.trk_words >= 0 && S.list_form >= CTXCK_LISTS_NONE && S.list_form <= CTXCK_LISTS_SLOTS && (slots ? S.W >= 1 && path_slots_addressable(S.W, S.n) : S.W == 0) &&
           S.M >= 0 && S.M <= 127 && (tables ? S.R >= 1 : S.R == 0) && (S.has_gate == 0 || (S.has_gate == 1 && tables)) && (S.has_clearance == 0 || S.has_clearance == 1);
}
SCA_HD int64_t ctx_section_bytes(int s, const CtxShape &S) {
    const int64_t n = S.n;
    const bool trk = S.trk_words > 0, lists = S.list_form != CTXCK_LISTS_NONE, slots = S.list_form == CTXCK_LISTS_SLOTS, tables = S.M > 0;
    switch (s) {
    case CX_POLICY: return n;
    case CX_REC: return CKPT_REC_BYTES * n;
    case CX_HEADING: case CX_GOAL: case CX_VPREF_EXT: return 24 * n;
    case CX_PREF_SPEED: case CX_MAX_RUN_DIST: case CX_TOTAL_DIST: return 8 * n;
    case CX_ZAXIS: case CX_VPREF_MODE: case CX_STEP_NUM: case CX_STATUS: case CX_PERM: return 4 * n;
    case CX_GOAL_HEADING: return trk ? 24 * n : 0;
    case CX_TRK_NBR0: return trk ? 8 * n : 0;
    case CX_TRACK: return trk ? 4 * (int64_t)S.trk_words * n : 0;
    case CX_REM: return lists ? 4 * n : 0;
    case CX_NOW_GOAL: return lists ? 24 * n : 0;
    case CX_LEN: return slots ? 4 * n : 0;
    case CX_ROOMS: return slots ? 24 * (int64_t)S.W * n : 0;
    case CX_MS_WORDS: return tables ? 4 * (int64_t)CTXCK_MS_WORDS * n : 0;
    case CX_MS_RESULTS: return tables ? CTXCK_RESULT_BYTES * (int64_t)S.R * n : 0;
    case CX_MS_TOTALS: return tables ? 8 * (int64_t)CTXCK_TOTAL_WORDS : 0;
    case CX_GATE_WORDS: return S.has_gate ? 4 * (int64_t)CTXCK_GATE_WORDS * n : 0;
    case CX_GATE_TOTALS: return S.has_gate ? 8 * (int64_t)CTXCK_TOTAL_WORDS : 0;
    default: return S.has_clearance ? CTXCK_CLEAR_BYTES * n : 0;
    }
}
// a pure function of the shape: the host and the tests call it, the kernels receive its answer
inline CtxLayout ctx_checkpoint_layout(const CtxShape &S) {
    CtxLayout L;
    int64_t at = (int64_t)sizeof(CtxHeader);
    for (int s = 0; s < CX_SECTIONS; s++) {
        L.off[s] = at;
        L.len[s] = ctx_section_bytes(s, S);
        at += (L.len[s] + CKPT_ALIGN - 1) / CKPT_ALIGN * CKPT_ALIGN;
    }
    L.total = at;
    return L;
}
inline CtxShape ctx_header_shape(const CtxHeader &H) {
    return CtxShape{H.n, H.trk_words, H.list_form, H.W, H.M, H.R, (H.present & CTXCK_HAS_GATE) ? 1 : 0, (H.present & CTXCK_HAS_CLEARANCE) ? 1 : 0};
}
inline uint32_t ctx_shape_present(const CtxShape &S) {
    // (without CTXCK_HAS_VACANCY, which is no part of a shape: it changes no section)
    return (S.trk_words > 0 ? CTXCK_HAS_TRACKER : 0u) | (S.list_form != CTXCK_LISTS_NONE ? CTXCK_HAS_LISTS : 0u) | (S.M > 0 ? CTXCK_HAS_TABLES : 0u) |
           (S.has_gate ? CTXCK_HAS_GATE : 0u) | (S.has_clearance ? CTXCK_HAS_CLEARANCE : 0u);
}

enum CtxFault {
    CXF_OK = 0,
    CXF_SHORT,              // fewer bytes than a header, or a NULL blob                               } the envelope: SCA_ERR_ARG
    CXF_MAGIC,              // not a context checkpoint                                                }
    CXF_FORMAT,             // another format version                                                  }
    CXF_RECORD,             // trk_words or the record size are not this library's                     }
    CXF_HEADER_RANGE,       // n < 1, unknown `present` bits, words that contradict each other         }
    CXF_BYTES,              // the byte count is not the layout's                                      }
    CXF_CHECKSUM,           // the payload's sum is not the header's                                   }
    CXF_N,                  // n is not the context's agent count                                      } against the context: SCA_ERR_ARG
    CXF_POLICY,             // a row's policy byte differs from the context's (entry: the row)         }
    CXF_TRACKER,            // tracker records present / absent against the context's device tracker   }
    CXF_LISTS,              // lists present / absent, or in the other form                            }
    CXF_LIST_W,             // slot form with another room per row                                     }
    CXF_TABLES,             // tables present / absent, or another M or R                              }
    CXF_GATE,               // the gate's words present / absent                                       }
    CXF_CLEARANCE,          // closest-approach records present / absent                               }
    CXF_PERM,               // the permutation is not one of 0 .. n-1 (entry: the position)            } the payload: SCA_ERR_ARG
    CXF_FLAGS,              // unknown flag bits, a vpref_mode or z-axis word other than 0 / 1         }
    CXF_NOT_FINITE,         // a position that is not finite (entry: the row)                          }
    CXF_NOT_POSITIVE,       // a radius, pref_speed or max_run_dist that is not positive and finite    }
    CXF_COUNTERS,           // a negative step_num, clear_step or updates                              }
    CXF_LEN_RANGE,          // len outside 0 .. W (entry: the row)                                     }
    CXF_REM_RANGE,          // rem outside 0 .. len (block form: the list's length as set)             }
    CXF_MISSION_RANGE,      // first_ok / first_fail / cursor / flying / waiting outside -1 .. M-1     }
    CXF_COLLECTED,          // collected above ended                                                   }
    CXF_VERDICT,            // a verdict word above SCA_SPAWN_OVER_CAP, or negative refusals           }
    CXF_CLEAR_PARTNER,      // a closest-approach partner outside its range, or a negative step        }
    CXF_TRACK_RANGE,        // an AgentTrack integer outside its range (entry: the row)                }
    // with vacancy allowed (the _opt entry points with SCA_CHECKPOINT_VACANCY; without it bit 8 is CXF_FLAGS and the header's bit CXF_HEADER_RANGE)
    CXF_VACANT_FLAGS,       // a row with the vacant bit whose flag word is not 11 (entry: the row)    } the payload: SCA_ERR_ARG
    CXF_VACANT_COUNT,       // the rows with the vacant bit are not n - occupied                       }
    CXF_VACANT_PERM,        // a position < m names a vacant id, or [m, n) is not the vacant ids ascending (entry: the position)   }
    CXF_VACANT_BLOCK,       // vacant rows together with lists in block form, which a retire refuses   }
    CXF_VACANT_WORDS        // a vacant row whose words are not a retired row's (entry: the row)       }
};
struct CtxCheck { CtxFault fault; int64_t entry; };
inline int ctx_checkpoint_error_code(CtxFault f) { return f == CXF_OK ? SCA_OK : SCA_ERR_ARG; }
// what the rules read of the loading context; NULL: the envelope and the payload alone (sca_context_checkpoint_info)
struct CtxExpect {
    CtxShape shape;                                // as the context stands
    const uint8_t *policy;                         // [n]
    const int32_t *block_len;                      // [n] block form: the lists' lengths as set
    int32_t n_obs;                                 // obstacles set (a closest-approach partner's bound)
};
// A vacant row of a blob must be what sca_retire_agents leaves (vacant_row, vacate_write_row, missions_retired) and what every later step
// keeps, wherever a kernel or the host would act on the word.  Checked, beside the flag word (11: every policy kernel, K4, the tracker
// and the compactions go by it):
//   velocity, heading   zero: the integrate stage and the host state block carry them on as they stand
//   total_dist          0.0: K4 adds no flag to a settled row only because 0 never passes max_run_dist
//   len, rem            0 in slot form: a take and the host's length mirrors go by them; a respawn that admits the row writes them anew
//   gate waiting        -1: k_mission_gate_take would admit a mission into a row that is not in the airspace
// Not checked, because nothing acts on them while the row is vacant and an admitting respawn writes them: step_num, status, now_goal (no
// kernel reads a list of length 0), the mission words other than the gate's (the row is done and "entered live" is 0: k_mission_advance
// passes over it; a retire keeps them too), the closest-approach record (k_clearance measures occupied rows only; a value, not an index --
// its partners' ranges are checked for every row), the tracker record (tracker_owns wants flags 0; its integers are in range as every
// row's).  Kept by a retire and checked as for every row: position, radius, goal, pref_speed, max_run_dist, z-axis, the v_pref mode.
inline bool ctx_vacant_row_fault(const unsigned char *b, const CtxLayout &L, const CtxShape &S, int i) {
    const unsigned char *r = b + L.off[CX_REC] + (int64_t)CKPT_REC_BYTES * i;
    if (!vacant_flag((uint32_t)ckpt_i32(r + 36))) return false;
    for (int k = 0; k < 3; k++) if ((ckpt_i32(r + 24 + 4 * k) & 0x7fffffff) != 0) return true;                       // vx, vy, vz: +-0
    for (int k = 0; k < 3; k++) if ((ckpt_i64(b + L.off[CX_HEADING] + 24 * (int64_t)i + 8 * k) & INT64_MAX) != 0) return true;
    if (ckpt_i64(b + L.off[CX_TOTAL_DIST] + 8 * (int64_t)i) != 0) return true;
    if (S.list_form == CTXCK_LISTS_SLOTS && (ckpt_i32(b + L.off[CX_LEN] + 4 * (int64_t)i) != 0 || ckpt_i32(b + L.off[CX_REM] + 4 * (int64_t)i) != 0)) return true;
    if (S.has_gate && ckpt_i32(b + L.off[CX_GATE_WORDS] + 4 * ((int64_t)CTXCK_GATE_WAITING * S.n + i)) != -1) return true;
    return false;
}
// THE check of a blob, whole: envelope, then the blob against the context, then every payload value a kernel would use as an index, a
// count or a switch.  Reads bytes [0, bytes) of `blob` and nothing else; head (nullable) receives the header once the envelope holds.
// allow_vacancy: the blob may hold vacant rows (CTXCK_HAS_VACANCY, flag bit 8), which then must be what sca_retire_agents leaves and every
// later step keeps -- see ctx_vacant_row_fault for the words.
inline CtxCheck ctx_checkpoint_check(const void *blob, int64_t bytes, const CkptTrackFields &F, const CtxExpect *X, CtxHeader *head, bool allow_vacancy = false) {
    if (blob == nullptr || bytes < (int64_t)sizeof(CtxHeader)) return {CXF_SHORT, -1};
    const unsigned char *b = (const unsigned char *)blob;
    CtxHeader H;
    { unsigned char *q = (unsigned char *)&H; for (std::size_t k = 0; k < sizeof(CtxHeader); k++) q[k] = b[k]; }
    if (H.magic != CTXCK_MAGIC) return {CXF_MAGIC, -1};
    if (H.format != CTXCK_FORMAT) return {CXF_FORMAT, -1};
    if (H.rec_bytes != CKPT_REC_BYTES || (H.trk_words != 0 && H.trk_words != F.words)) return {CXF_RECORD, -1};
    const CtxShape S = ctx_header_shape(H);
    const uint32_t known = (uint32_t)CTXCK_HAS_ALL | (allow_vacancy ? (uint32_t)CTXCK_HAS_VACANCY : 0u);
    const bool vacancy = (H.present & CTXCK_HAS_VACANCY) != 0;
    if ((H.present & ~known) != 0 || !ctx_shape_ok(S) || ctx_shape_present(S) != (H.present & (uint32_t)CTXCK_HAS_ALL) || (H.state_fresh != 0 && H.state_fresh != 1) ||
        (vacancy ? H.occupied < 1 || H.occupied >= H.n : H.occupied != 0))
        return {CXF_HEADER_RANGE, -1};
    const CtxLayout L = ctx_checkpoint_layout(S);
    if (H.total_bytes != L.total || bytes != L.total) return {CXF_BYTES, -1};
    if (scene_checkpoint_sum(b + sizeof(CtxHeader), L.total - (int64_t)sizeof(CtxHeader)) != H.checksum) return {CXF_CHECKSUM, -1};
    if (head) *head = H;
    const int N = H.n, M = H.M, occupied = vacancy ? H.occupied : N;
    const unsigned char *pol = b + L.off[CX_POLICY];
    if (X) {
        const CtxShape &C = X->shape;
        if (C.n != N) return {CXF_N, -1};
        for (int i = 0; i < N; i++) if (pol[i] != X->policy[i]) return {CXF_POLICY, i};
        if ((C.trk_words > 0) != (S.trk_words > 0)) return {CXF_TRACKER, -1};
        if (C.list_form != S.list_form) return {CXF_LISTS, -1};
        if (C.W != S.W) return {CXF_LIST_W, -1};
        if (C.M != S.M || C.R != S.R) return {CXF_TABLES, -1};
        if (C.has_gate != S.has_gate) return {CXF_GATE, -1};
        if (C.has_clearance != S.has_clearance) return {CXF_CLEARANCE, -1};
    }
    for (int i = 0; i < N; i++) if (pol[i] > SCA_POLICY_RVO3D_DUBINS) return {CXF_POLICY, i};
    if (H.clear_step < 0 || H.updates < 0 || (!S.has_clearance && H.clear_step != 0) || (M == 0 && H.updates != 0)) return {CXF_COUNTERS, -1};
    {
        std::vector<uint8_t> seen((std::size_t)N, (uint8_t)0);
        for (int p = 0; p < N; p++) {
            const int32_t a = ckpt_i32(b + L.off[CX_PERM] + 4 * (int64_t)p);
            if (a < 0 || a >= N || seen[(std::size_t)a]) return {CXF_PERM, p};
            seen[(std::size_t)a] = 1;
        }
    }
    for (int i = 0; i < N; i++) {
        const unsigned char *r = b + L.off[CX_REC] + (int64_t)CKPT_REC_BYTES * i;
        const uint32_t flags = (uint32_t)ckpt_i32(r + 36);
        const uint32_t mode = (uint32_t)ckpt_i32(b + L.off[CX_VPREF_MODE] + 4 * (int64_t)i), z = (uint32_t)ckpt_i32(b + L.off[CX_ZAXIS] + 4 * (int64_t)i);
        if ((flags & ~(allow_vacancy ? 15u : 7u)) != 0 || mode > 1u || z > 1u) return {CXF_FLAGS, i};
        if (vacant_flag(flags) && flags != VACANT_FLAGS) return {CXF_VACANT_FLAGS, i};
        for (int k = 0; k < 3; k++) if (!restart_finite(ckpt_f64(r + 8 * k))) return {CXF_NOT_FINITE, i};
        const double radius = ckpt_f64(r + 40), ps = ckpt_f64(b + L.off[CX_PREF_SPEED] + 8 * (int64_t)i), mrd = ckpt_f64(b + L.off[CX_MAX_RUN_DIST] + 8 * (int64_t)i);
        if (!(restart_finite(radius) && radius > 0.0 && restart_finite(ps) && ps > 0.0 && restart_finite(mrd) && mrd > 0.0)) return {CXF_NOT_POSITIVE, i};
        if (ckpt_i32(b + L.off[CX_STEP_NUM] + 4 * (int64_t)i) < 0) return {CXF_COUNTERS, i};
    }
    if (allow_vacancy) {
        const auto vacant = [&](int a) { return vacant_flag((uint32_t)ckpt_i32(b + L.off[CX_REC] + (int64_t)CKPT_REC_BYTES * a + 36)); };
        int count = 0;
        for (int i = 0; i < N; i++) count += vacant(i) ? 1 : 0;
        if (count != N - occupied) return {CXF_VACANT_COUNT, -1};
        if (count > 0) {
            // sca_vacancy.h's contract: [0, m) the occupied ids in carried order, [m, n) the vacant ids ascending
            int next = 0;
            for (int p = 0; p < N; p++) {
                const int32_t a = ckpt_i32(b + L.off[CX_PERM] + 4 * (int64_t)p);
                if (p < occupied) { if (vacant(a)) return {CXF_VACANT_PERM, p}; continue; }
                while (next < N && !vacant(next)) next++;
                if (a != next) return {CXF_VACANT_PERM, p};
                next++;
            }
            if (S.list_form == CTXCK_LISTS_BLOCK) return {CXF_VACANT_BLOCK, -1};
        }
    }
    if (S.list_form != CTXCK_LISTS_NONE)
        for (int i = 0; i < N; i++) {
            int32_t len;
            if (S.list_form == CTXCK_LISTS_SLOTS) {
                len = ckpt_i32(b + L.off[CX_LEN] + 4 * (int64_t)i);
                if (len < 0 || len > S.W) return {CXF_LEN_RANGE, i};
            } else {
                len = X ? X->block_len[i] : INT32_MAX;                     // (without a context the list's length is not known: the sign alone)
            }
            const int32_t rem = ckpt_i32(b + L.off[CX_REM] + 4 * (int64_t)i);
            if (rem < 0 || rem > len) return {CXF_REM_RANGE, i};
        }
    if (M > 0) {
        const unsigned char *w = b + L.off[CX_MS_WORDS];
        const auto word = [&](int col, int i) { return ckpt_i32(w + 4 * ((int64_t)col * N + i)); };
        for (int i = 0; i < N; i++) {
            for (int col : {CTXCK_MS_FIRST_OK, CTXCK_MS_FIRST_FAIL, CTXCK_MS_CURSOR, CTXCK_MS_FLYING}) { const int32_t v = word(col, i); if (v < -1 || v >= M) return {CXF_MISSION_RANGE, i}; }
            if ((uint32_t)word(CTXCK_MS_COLLECTED, i) > (uint32_t)word(CTXCK_MS_ENDED, i)) return {CXF_COLLECTED, i};
        }
    }
    if (S.has_gate) {
        const unsigned char *w = b + L.off[CX_GATE_WORDS];
        for (int i = 0; i < N; i++) {
            const int32_t wait = ckpt_i32(w + 4 * ((int64_t)CTXCK_GATE_WAITING * N + i)), verdict = ckpt_i32(w + 4 * ((int64_t)CTXCK_GATE_VERDICT * N + i));
            if (wait < -1 || wait >= M) return {CXF_MISSION_RANGE, i};
            if (verdict < 0 || verdict > SCA_SPAWN_OVER_CAP || ckpt_i32(w + 4 * ((int64_t)CTXCK_GATE_REFUSALS * N + i)) < 0) return {CXF_VERDICT, i};
        }
    }
    if (S.has_clearance)
        for (int i = 0; i < N; i++) {
            const unsigned char *r = b + L.off[CX_CLEAR] + CTXCK_CLEAR_BYTES * (int64_t)i;
            const int32_t ap = ckpt_i32(r + 16), as = ckpt_i32(r + 20), op = ckpt_i32(r + 24), os = ckpt_i32(r + 28);
            if (ap < -1 || ap >= N || op < -1 || (X && op >= X->n_obs) || as < 0 || os < 0) return {CXF_CLEAR_PARTNER, i};
        }
    if (S.trk_words > 0)
        for (int i = 0; i < N; i++) {
            const unsigned char *t = b + L.off[CX_TRACK] + 4 * (int64_t)F.words * i;
            const int64_t count = ckpt_i64(t + F.count), next = ckpt_i64(t + F.next);
            const bool ok = t[F.use_dubins] <= 1 && t[F.plan_ok] <= 1 && t[F.h_ok] <= 1 && t[F.v_ok] <= 1 && ckpt_word_ok(t + F.h_mode, 3) && ckpt_word_ok(t + F.v_mode, 3) &&
                            ckpt_word_ok(t + F.plan_mode, 7) && ckpt_i32(t + F.iters) >= 0 && ckpt_i32(t + F.rounds) >= 0 && ckpt_i32(t + F.replans) >= 0 &&
                            count >= 0 && count <= CKPT_COUNT_MAX && next >= 0 && next <= count;
            if (!ok) return {CXF_TRACK_RANGE, i};
        }
    if (vacancy)
        for (int i = 0; i < N; i++) if (ctx_vacant_row_fault(b, L, S, i)) return {CXF_VACANT_WORDS, i};
    return {CXF_OK, -1};
}

// the calls' own rules, for both entry points, in the order they are held
enum CtxCallFault {
    CXC_OK = 0,
    CXC_NO_AGENTS,          // sca_set_agents first                                                    } SCA_ERR_STATE
    CXC_NO_STATE,           // no state yet                                                            }
    CXC_MID_STEP,           // between a policy pass and its env update                                }
    CXC_SCENES,             // scenes have checkpoints of their own                                    } SCA_ERR_UNSUPPORTED
    CXC_SHARD,              // a shard with count < n                                                  }
    CXC_COMM,               // a communicator                                                          }
    CXC_PARTITION,          // the cell-owner partition                                                }
    CXC_NO_BUFFER           // a NULL buffer                                                           } SCA_ERR_ARG
};
struct CtxCallState { bool agents, state, mid_step, scenes, comm, partition; int n, shard_count; };
inline CtxCallFault ctx_checkpoint_call_check(const CtxCallState &s, bool buffer) {
    if (!s.agents) return CXC_NO_AGENTS;
    if (!s.state) return CXC_NO_STATE;
    if (s.mid_step) return CXC_MID_STEP;
    if (s.scenes) return CXC_SCENES;
    if (s.comm) return CXC_COMM;
    if (s.partition) return CXC_PARTITION;
    if (s.shard_count < s.n) return CXC_SHARD;
    if (!buffer) return CXC_NO_BUFFER;
    return CXC_OK;
}
inline int ctx_checkpoint_call_error_code(CtxCallFault f) { return f == CXC_OK ? SCA_OK : f <= CXC_MID_STEP ? SCA_ERR_STATE : f <= CXC_PARTITION ? SCA_ERR_UNSUPPORTED : SCA_ERR_ARG; }

// K4's counters for a set of flags: stripe a & 255 counts the rows without a done flag (the host fills them from the checked blob, the
// load kernel stores them -- no atomics, and right whatever the counters held before)
inline void ctx_checkpoint_stripes(const void *blob, const CtxLayout &L, int n, int32_t *stripes /*CTXCK_STRIPES*/) {
    for (int s = 0; s < CTXCK_STRIPES; s++) stripes[s] = 0;
    const unsigned char *rec = (const unsigned char *)blob + L.off[CX_REC];
    for (int a = 0; a < n; a++) if (!((uint32_t)ckpt_i32(rec + (int64_t)CKPT_REC_BYTES * a + 36) & 7u)) stripes[a & (CTXCK_STRIPES - 1)]++;
}

// ---- the row move ---------------------------------------------------------------------------------------------------------------------------
// What thread `tid` of `stride` moves between the rows' arrays and a blob: k_ctx_save / k_ctx_load are this function over the grid
// (sca_checkpoint.hip.h), the harness runs it over plain arrays.  Consecutive threads move consecutive 4-byte words; the public records,
// the tracker records, the result rings and the closest-approach records move as 16-byte pieces (a section's bytes behind its last whole
// piece as words).  Every index is 64-bit.  Null arrays belong to sections of length 0.  Two accesses are NOT consecutive words: the byte
// columns (z-axis, vpref_mode) are single-byte stores into the rows' arrays on the way in (single-byte loads on the way out; the blob's
// side is a word per row), and the load derives the "entered live" column from the flag word of every record in the blob, a 4-byte read at
// a 48-byte stride from the page-locked block.  Both are one access per row of a rare call.
typedef uint32_t __attribute__((may_alias)) ctx_u32;
struct __attribute__((may_alias, aligned(16))) CtxPiece { uint32_t w[4]; };
struct CtxDev {
    PubRec *rec;
    double *heading, *goal, *pref_speed, *max_run_dist, *vpref_ext, *total_dist;
    int32_t *step_num, *status, *aperm;
    uint8_t *zaxis, *vpref_mode;
    int32_t *done_count;            // [CTXCK_STRIPES * CTXCK_STRIPE_PITCH]: written by the load
    double *trk_goal_heading, *trk_nbr0;
    ctx_u32 *trk_st;
    int32_t *rem; double *now_goal;
    int32_t *len; double *rooms;
    int32_t *ms_words; void *ms_results; unsigned long long *ms_totals;
    int32_t *gate_words; unsigned long long *gate_totals;
    sca_scene_clearance *clear;
};
template <bool LOAD> SCA_HD void ctx_words(void *arr, uint8_t *sec, int64_t words, int64_t tid, int64_t stride) {
    ctx_u32 *a = (ctx_u32 *)arr, *b = (ctx_u32 *)sec;
    for (int64_t w = tid; w < words; w += stride) { if (LOAD) a[w] = b[w]; else b[w] = a[w]; }
}
template <bool LOAD> SCA_HD void ctx_pieces(void *arr, uint8_t *sec, int64_t bytes, int64_t tid, int64_t stride) {
    CtxPiece *a = (CtxPiece *)arr, *b = (CtxPiece *)sec;
    const int64_t pieces = bytes / 16;
    for (int64_t p = tid; p < pieces; p += stride) { if (LOAD) a[p] = b[p]; else b[p] = a[p]; }
    ctx_words<LOAD>((uint8_t *)arr + 16 * pieces, sec + 16 * pieces, (bytes - 16 * pieces) / 4, tid, stride);
}
template <bool LOAD> SCA_HD void ctx_byte_column(uint8_t *arr, uint8_t *sec, int64_t rows, int64_t tid, int64_t stride) {
    ctx_u32 *b = (ctx_u32 *)sec;
    for (int64_t i = tid; i < rows; i += stride) { if (LOAD) arr[i] = (uint8_t)b[i]; else b[i] = arr[i]; }
}
// stripes: the load's CTXCK_STRIPES counters (ctx_checkpoint_stripes), unused by a save
template <bool LOAD> SCA_HD void ctx_checkpoint_move(const CtxDev &d, uint8_t *blob, const CtxLayout &L, const CtxShape &S, const int32_t *stripes, int64_t tid, int64_t stride) {
    const int64_t n = S.n;
    ctx_pieces<LOAD>(d.rec, blob + L.off[CX_REC], L.len[CX_REC], tid, stride);
    ctx_words<LOAD>(d.heading, blob + L.off[CX_HEADING], 6 * n, tid, stride);
    ctx_words<LOAD>(d.goal, blob + L.off[CX_GOAL], 6 * n, tid, stride);
    ctx_words<LOAD>(d.pref_speed, blob + L.off[CX_PREF_SPEED], 2 * n, tid, stride);
    ctx_words<LOAD>(d.max_run_dist, blob + L.off[CX_MAX_RUN_DIST], 2 * n, tid, stride);
    ctx_byte_column<LOAD>(d.zaxis, blob + L.off[CX_ZAXIS], n, tid, stride);
    ctx_words<LOAD>(d.vpref_ext, blob + L.off[CX_VPREF_EXT], 6 * n, tid, stride);
    ctx_byte_column<LOAD>(d.vpref_mode, blob + L.off[CX_VPREF_MODE], n, tid, stride);
    ctx_words<LOAD>(d.total_dist, blob + L.off[CX_TOTAL_DIST], 2 * n, tid, stride);
    ctx_words<LOAD>(d.step_num, blob + L.off[CX_STEP_NUM], n, tid, stride);
    ctx_words<LOAD>(d.status, blob + L.off[CX_STATUS], n, tid, stride);
    ctx_words<LOAD>(d.aperm, blob + L.off[CX_PERM], n, tid, stride);
    if (S.trk_words > 0) {
        ctx_words<LOAD>(d.trk_goal_heading, blob + L.off[CX_GOAL_HEADING], 6 * n, tid, stride);
        ctx_words<LOAD>(d.trk_nbr0, blob + L.off[CX_TRK_NBR0], 2 * n, tid, stride);
        ctx_pieces<LOAD>(d.trk_st, blob + L.off[CX_TRACK], L.len[CX_TRACK], tid, stride);
    }
    if (S.list_form != CTXCK_LISTS_NONE) {
        ctx_words<LOAD>(d.rem, blob + L.off[CX_REM], n, tid, stride);
        ctx_words<LOAD>(d.now_goal, blob + L.off[CX_NOW_GOAL], 6 * n, tid, stride);
    }
    if (S.list_form == CTXCK_LISTS_SLOTS) {
        ctx_words<LOAD>(d.len, blob + L.off[CX_LEN], n, tid, stride);
        ctx_words<LOAD>(d.rooms, blob + L.off[CX_ROOMS], 6 * (int64_t)S.W * n, tid, stride);
    }
    if (S.M > 0) {
        // a load leaves the "entered live" column to the flags it brings (k_mission_live's rule), as every change of flags between two steps does
        ctx_words<LOAD>(d.ms_words, blob + L.off[CX_MS_WORDS], (LOAD ? CTXCK_MS_LIVE : CTXCK_MS_WORDS) * n, tid, stride);
        if (LOAD) {
            const ctx_u32 *rec = (const ctx_u32 *)(blob + L.off[CX_REC]);
            for (int64_t a = tid; a < n; a += stride) d.ms_words[CTXCK_MS_LIVE * n + a] = (rec[a * (CKPT_REC_BYTES / 4) + 9] & 7u) ? 0 : 1;
        }
        ctx_pieces<LOAD>(d.ms_results, blob + L.off[CX_MS_RESULTS], L.len[CX_MS_RESULTS], tid, stride);
        ctx_words<LOAD>(d.ms_totals, blob + L.off[CX_MS_TOTALS], 2 * CTXCK_TOTAL_WORDS, tid, stride);
    }
    if (S.has_gate) {
        ctx_words<LOAD>(d.gate_words, blob + L.off[CX_GATE_WORDS], CTXCK_GATE_WORDS * n, tid, stride);
        ctx_words<LOAD>(d.gate_totals, blob + L.off[CX_GATE_TOTALS], 2 * CTXCK_TOTAL_WORDS, tid, stride);
    }
    if (S.has_clearance) ctx_pieces<LOAD>(d.clear, blob + L.off[CX_CLEAR], L.len[CX_CLEAR], tid, stride);
    if (LOAD) for (int64_t s = tid; s < CTXCK_STRIPES; s += stride) d.done_count[s * CTXCK_STRIPE_PITCH] = stripes[s];
}

// ---- the load with vacant rows ----------------------------------------------------------------------------------------------------------------
// The outputs of the last pass are not in a blob: they follow with the next pass.  A vacant row never gets one, so a load that brings
// vacant rows leaves for each of them what vacate_write_row left on the source and no pass has touched since: a zero action row, nbr_n 0,
// nbr_valid 0, near_n -1, diag -1 (vacate_write_outputs, sca_vacancy.h).  Which rows: the flag word of the CHECKED blob, one 4-byte read
// per row at the record's stride, as the "entered live" column takes it; never the rows' own records, which other threads of the same
// launch are writing.  A thread serves a row's eight lanes: two runs of 32 bytes and three words per vacant row, vector stores, no atomics.
struct CtxVacDev {
    float *action;                  // [n*8]
    int32_t *diag;                  // [n*8]
    int32_t *nbr_n, *near_n;
    uint8_t *nbr_valid;
};
SCA_HD void ctx_checkpoint_move_vacancy(const CtxDev &d, const CtxVacDev &o, uint8_t *blob, const CtxLayout &L, const CtxShape &S, const int32_t *stripes, int64_t tid, int64_t stride) {
    ctx_checkpoint_move<true>(d, blob, L, S, stripes, tid, stride);
    const ctx_u32 *rec = (const ctx_u32 *)(blob + L.off[CX_REC]);
    const VacantRow w = vacant_row(VACANT_FLAGS, S.list_form == CTXCK_LISTS_SLOTS);
    for (int64_t a = tid; a < (int64_t)S.n; a += stride) {
        if (!vacant_flag(rec[a * (CKPT_REC_BYTES / 4) + 9])) continue;
        for (int lane = 0; lane < 8; lane++) vacate_write_outputs(o, a, lane, w);
    }
}

}  // namespace sca
