// context_checkpoint_vacancy_harness.cpp -- TEST-ONLY host build of what context checkpoints with vacant rows add to sca_checkpoint.h: the
// check with vacancy allowed (ctx_checkpoint_check's last argument) and the load's row move with the vacant rows' outputs
// (ctx_checkpoint_move_vacancy), over plain arrays of exactly the rows' sizes.  The blobs come from context_checkpoint_harness.cpp's
// cx_make, included here whole; cxv_make then retires the named rows in the blob as sca_retire_agents leaves them.  With
// -DCONTEXT_CHECKPOINT_VACANCY_MAIN it is a program of its own (for the sanitizers): every blob lives in a heap buffer of exactly its size.
#include "context_checkpoint_harness.cpp"

namespace {
// every per-row array a load writes, of exactly the rows' sizes, zeroed; the outputs hold values no retire writes
struct Rows {
    CtxShape S; CtxLayout L; size_t n;
    std::vector<PubRec> rec;
    std::vector<double> heading, goal, ps, mrd, vpref, td, gh, nbr0, now_goal, rooms;
    std::vector<int32_t> step, status, perm, done_count, rem, len, msw, gw, diag, nbr_n, near_n;
    std::vector<uint8_t> zaxis, mode, nbr_valid;
    std::vector<uint32_t> track;
    std::vector<sca_mission_result> results;
    std::vector<unsigned long long> mst, mgt;
    std::vector<sca_scene_clearance> clear;
    std::vector<float> action;
    explicit Rows(const CtxShape &s) : S(s), L(ctx_checkpoint_layout(s)), n((size_t)s.n) {
        const bool trk = S.trk_words > 0, lists = S.list_form != CTXCK_LISTS_NONE, slots = S.list_form == CTXCK_LISTS_SLOTS, tables = S.M > 0;
        rec.resize(n); std::memset(rec.data(), 0, sizeof(PubRec) * n);
        heading.assign(3 * n, 0); goal.assign(3 * n, 0); ps.assign(n, 0); mrd.assign(n, 0); vpref.assign(3 * n, 0); td.assign(n, 0);
        gh.assign(trk ? 3 * n : 0, 0); nbr0.assign(trk ? n : 0, 0); now_goal.assign(lists ? 3 * n : 0, 0); rooms.assign(slots ? 3 * n * (size_t)S.W : 0, 0);
        step.assign(n, 0); status.assign(n, 0); perm.assign(n, 0); done_count.assign((size_t)CTXCK_STRIPES * CTXCK_STRIPE_PITCH, -7);
        rem.assign(lists ? n : 0, 0); len.assign(slots ? n : 0, 0); msw.assign(tables ? n * CTXCK_MS_WORDS : 0, 0); gw.assign(S.has_gate ? n * CTXCK_GATE_WORDS : 0, 0);
        zaxis.assign(n, 0); mode.assign(n, 0); track.assign(trk ? n * (size_t)S.trk_words : 0, 0);
        results.resize(tables ? n * (size_t)S.R : 0); if (!results.empty()) std::memset(results.data(), 0, sizeof(sca_mission_result) * results.size());
        mst.assign(tables ? CTXCK_TOTAL_WORDS : 0, 0); mgt.assign(S.has_gate ? CTXCK_TOTAL_WORDS : 0, 0);
        clear.resize(S.has_clearance ? n : 0); if (!clear.empty()) std::memset(clear.data(), 0, sizeof(sca_scene_clearance) * clear.size());
        action.assign(8 * n, 7.5f); diag.assign(8 * n, 5); nbr_n.assign(n, 3); near_n.assign(n, 4); nbr_valid.assign(n, 1);
    }
    template <class V> static auto ptr(V &v) { return v.empty() ? nullptr : v.data(); }
    CtxDev dev() {
        CtxDev d{};
        d.rec = rec.data(); d.heading = heading.data(); d.goal = goal.data(); d.pref_speed = ps.data(); d.max_run_dist = mrd.data(); d.vpref_ext = vpref.data(); d.total_dist = td.data();
        d.step_num = step.data(); d.status = status.data(); d.aperm = perm.data(); d.zaxis = zaxis.data(); d.vpref_mode = mode.data(); d.done_count = done_count.data();
        d.trk_goal_heading = ptr(gh); d.trk_nbr0 = ptr(nbr0); d.trk_st = (ctx_u32 *)ptr(track); d.rem = ptr(rem); d.now_goal = ptr(now_goal); d.len = ptr(len); d.rooms = ptr(rooms);
        d.ms_words = ptr(msw); d.ms_results = ptr(results); d.ms_totals = ptr(mst); d.gate_words = ptr(gw); d.gate_totals = ptr(mgt); d.clear = ptr(clear);
        return d;
    }
    CtxVacDev out() { return CtxVacDev{action.data(), diag.data(), nbr_n.data(), near_n.data(), nbr_valid.data()}; }
};
// what vacate_write_row writes (sca_vacancy.h): the retire's view of the same arrays
struct RetireDev {
    PubRec *rec; double *heading, *total_dist, *now_goal; float *action; int32_t *diag, *step_num, *status, *nbr_n, *near_n, *path_len, *path_rem; uint8_t *nbr_valid;
    sca_scene_clearance *clear;
};
}  // namespace

extern "C" {

int cxv_faults(int *out5) {
    const int v[5] = {CXF_VACANT_FLAGS, CXF_VACANT_COUNT, CXF_VACANT_PERM, CXF_VACANT_BLOCK, CXF_VACANT_WORDS};
    for (int k = 0; k < 5; k++) out5[k] = v[k];
    return CTXCK_HAS_VACANCY;
}
// cx_make's blob with the rows named in vacant[n] retired: flag word 11, zero velocity, heading and total_dist, step_num and status 0, in
// slot form len = rem = 0 and now_goal None, the gate's waiting word -1, "entered live" 0, an empty closest-approach record; the
// permutation: the occupied ids descending (cx_make's order with the vacant ids deleted), then the vacant ids ascending; the header's bit
// and the occupied count where a row is vacant.  Returns the total.
int64_t cxv_make(const int32_t *shape8, const uint8_t *policy, const uint8_t *vacant, void *blob) {
    const CtxShape S = shape_of(shape8);
    const CtxLayout L = ctx_checkpoint_layout(S);
    const int n = S.n;
    cx_make(shape8, policy, blob);
    unsigned char *b = (unsigned char *)blob;
    int at = 0, m = 0;
    for (int i = n - 1; i >= 0; i--) if (!vacant[i]) { put<int32_t>(b + L.off[CX_PERM] + 4 * (int64_t)at++, i); m++; }
    for (int i = 0; i < n; i++) {
        if (!vacant[i]) continue;
        put<int32_t>(b + L.off[CX_PERM] + 4 * (int64_t)at++, i);
        unsigned char *r = b + L.off[CX_REC] + (int64_t)CKPT_REC_BYTES * i;
        std::memset(r + 24, 0, 12); put<uint32_t>(r + 36, VACANT_FLAGS);
        std::memset(b + L.off[CX_HEADING] + 24 * (int64_t)i, 0, 24);
        put<double>(b + L.off[CX_TOTAL_DIST] + 8 * (int64_t)i, 0.0);
        put<int32_t>(b + L.off[CX_STEP_NUM] + 4 * (int64_t)i, 0);
        if (S.list_form == CTXCK_LISTS_SLOTS) { put<int32_t>(b + L.off[CX_LEN] + 4 * (int64_t)i, 0); put<int32_t>(b + L.off[CX_REM] + 4 * (int64_t)i, 0); }
        if (S.M > 0) put<int32_t>(b + L.off[CX_MS_WORDS] + 4 * ((int64_t)CTXCK_MS_LIVE * n + i), 0);
        if (S.has_gate) { put<int32_t>(b + L.off[CX_GATE_WORDS] + 4 * ((int64_t)CTXCK_GATE_WAITING * n + i), -1); put<int32_t>(b + L.off[CX_GATE_WORDS] + 4 * ((int64_t)CTXCK_GATE_VERDICT * n + i), 0); }
        if (S.has_clearance) { const sca_scene_clearance e = scene_clearance_empty(); std::memcpy(b + L.off[CX_CLEAR] + CTXCK_CLEAR_BYTES * (int64_t)i, &e, sizeof e); }
    }
    if (m < n) { put<uint32_t>(b + offsetof(CtxHeader, present), ctx_shape_present(S) | CTXCK_HAS_VACANCY); put<int32_t>(b + offsetof(CtxHeader, occupied), m); }
    cx_seal(b, L.total);
    return L.total;
}
int cxv_check(const void *blob, int64_t bytes, int allow, int with_ctx, const int32_t *shape8, const uint8_t *policy, const int32_t *block_len, int n_obs, int64_t *out) {
    CtxExpect X{};
    if (with_ctx) { X.shape = shape_of(shape8); X.policy = policy; X.block_len = block_len; X.n_obs = n_obs; }
    const CtxCheck k = ctx_checkpoint_check(blob, bytes, fields(), with_ctx ? &X : nullptr, nullptr, allow != 0);
    out[0] = (int64_t)k.fault; out[1] = k.entry;
    return ctx_checkpoint_error_code(k.fault);
}
// The load's row move with vacant rows, by `threads` threads, into zeroed arrays whose outputs hold other values; then k_ctx_save's move
// out of them into out[total] (the header and the policies copied over, as sca_save_context does).  The outputs as the load left them:
// action[8 n], diag[8 n], nbr_n[n], near_n[n], nbr_valid[n]; done[256]: K4's stripes.
void cxv_roundtrip(const int32_t *shape8, const void *blob, int threads, void *out, float *action, int32_t *diag, int32_t *nbr_n, int32_t *near_n, uint8_t *nbr_valid, int32_t *done) {
    Rows R(shape_of(shape8));
    const CtxLayout &L = R.L;
    std::vector<unsigned char> in((const unsigned char *)blob, (const unsigned char *)blob + L.total);     // exactly the blob's bytes
    int32_t stripes[CTXCK_STRIPES];
    ctx_checkpoint_stripes(in.data(), L, R.S.n, stripes);
    const CtxDev d = R.dev();
    for (int t = 0; t < threads; t++) ctx_checkpoint_move_vacancy(d, R.out(), in.data(), L, R.S, stripes, t, threads);
    for (int s = 0; s < CTXCK_STRIPES; s++) done[s] = R.done_count[(size_t)s * CTXCK_STRIPE_PITCH];
    std::vector<unsigned char> o((size_t)L.total, 0);
    for (int t = 0; t < threads; t++) ctx_checkpoint_move<false>(d, o.data(), L, R.S, nullptr, t, threads);
    std::memcpy(o.data(), in.data(), sizeof(CtxHeader));
    std::memcpy(o.data() + L.off[CX_POLICY], in.data() + L.off[CX_POLICY], R.n);
    std::memcpy(out, o.data(), (size_t)L.total);
    std::memcpy(action, R.action.data(), sizeof(float) * 8 * R.n); std::memcpy(diag, R.diag.data(), sizeof(int32_t) * 8 * R.n);
    std::memcpy(nbr_n, R.nbr_n.data(), sizeof(int32_t) * R.n); std::memcpy(near_n, R.near_n.data(), sizeof(int32_t) * R.n); std::memcpy(nbr_valid, R.nbr_valid.data(), R.n);
}
// the same outputs as vacate_write_row leaves them: the rows named in vacant[n] retired by all 64 lanes, the others as Rows fills them
void cxv_retired_outputs(const int32_t *shape8, const uint8_t *vacant, float *action, int32_t *diag, int32_t *nbr_n, int32_t *near_n, uint8_t *nbr_valid) {
    Rows R(shape_of(shape8));
    const bool slots = R.S.list_form == CTXCK_LISTS_SLOTS;
    RetireDev d{R.rec.data(), R.heading.data(), R.td.data(), slots ? R.now_goal.data() : nullptr, R.action.data(), R.diag.data(), R.step.data(), R.status.data(), R.nbr_n.data(),
                R.near_n.data(), slots ? R.len.data() : nullptr, slots ? R.rem.data() : nullptr, R.nbr_valid.data(), Rows::ptr(R.clear)};
    for (int a = 0; a < R.S.n; a++) {
        if (!vacant[a]) continue;
        const VacantRow w = vacant_row(R.rec[(size_t)a].flags, slots);
        for (int lane = 0; lane < 64; lane++) vacate_write_row(d, a, lane, w);
    }
    std::memcpy(action, R.action.data(), sizeof(float) * 8 * R.n); std::memcpy(diag, R.diag.data(), sizeof(int32_t) * 8 * R.n);
    std::memcpy(nbr_n, R.nbr_n.data(), sizeof(int32_t) * R.n); std::memcpy(near_n, R.near_n.data(), sizeof(int32_t) * R.n); std::memcpy(nbr_valid, R.nbr_valid.data(), R.n);
}

}  // extern "C"

#ifdef CONTEXT_CHECKPOINT_VACANCY_MAIN
namespace {
void vrun(const char *what, const std::vector<unsigned char> &blob, int allow, const int32_t *shape8, const uint8_t *policy) {
    const int64_t bytes = (int64_t)blob.size();
    unsigned char *exact = new unsigned char[(size_t)bytes];
    std::memcpy(exact, blob.data(), (size_t)bytes);
    int64_t out[2];
    const int rc = cxv_check(exact, bytes, allow, 1, shape8, policy, nullptr, 0, out);
    std::printf("%s: rc %d fault %d entry %d\n", what, rc, (int)out[0], (int)out[1]);
    delete[] exact;
}
}  // namespace
int main() {
    const int N = 7;
    const uint8_t pol[N] = {0, 1, 5, 3, 4, 0, 2};
    const uint8_t vac[N] = {0, 1, 0, 0, 1, 1, 0};
    const int32_t full[8] = {N, cx_track_words(), CTXCK_LISTS_SLOTS, 3, 2, 2, 1, 1};
    int64_t off[CX_SECTIONS], ln[CX_SECTIONS];
    const int64_t total = cx_layout(full, off, ln);
    std::vector<unsigned char> good((size_t)total);
    cxv_make(full, pol, vac, good.data());
    vrun("valid", good, 1, full, pol);
    vrun("not allowed", good, 0, full, pol);
    struct Byte { int64_t at; unsigned char v; };
    auto damaged = [&](const char *what, std::vector<Byte> bytes) {
        std::vector<unsigned char> b = good;
        for (const Byte &x : bytes) b[(size_t)x.at] = x.v;
        cx_seal(b.data(), total);
        vrun(what, b, 1, full, pol);
    };
    damaged("occupied 0", {{offsetof(CtxHeader, occupied), 0}});
    damaged("occupied n", {{offsetof(CtxHeader, occupied), N}});
    damaged("flags 9", {{off[CX_REC] + 48 * 4 + 36, 9}});
    damaged("count", {{offsetof(CtxHeader, occupied), 3}});
    damaged("prefix", {{off[CX_PERM], 1}, {off[CX_PERM] + 4 * 4, 6}});
    damaged("tail", {{off[CX_PERM] + 4 * 4, 4}, {off[CX_PERM] + 4 * 5, 1}});
    damaged("velocity", {{off[CX_REC] + 48 * 1 + 27, 0x3f}});
    damaged("len", {{off[CX_LEN] + 4 * 5, 1}});
    damaged("waiting", {{off[CX_GATE_WORDS] + 4 * 4, 0}, {off[CX_GATE_WORDS] + 4 * 4 + 1, 0}, {off[CX_GATE_WORDS] + 4 * 4 + 2, 0}, {off[CX_GATE_WORDS] + 4 * 4 + 3, 0}});
    for (int threads : {1, 5}) {
        std::vector<unsigned char> back((size_t)total);
        std::vector<float> action(8 * N), want_action(8 * N);
        std::vector<int32_t> diag(8 * N), nbr_n(N), near_n(N), done(CTXCK_STRIPES), want_diag(8 * N), want_nbr_n(N), want_near_n(N);
        std::vector<uint8_t> valid(N), want_valid(N);
        cxv_roundtrip(full, good.data(), threads, back.data(), action.data(), diag.data(), nbr_n.data(), near_n.data(), valid.data(), done.data());
        cxv_retired_outputs(full, vac, want_action.data(), want_diag.data(), want_nbr_n.data(), want_near_n.data(), want_valid.data());
        const bool outputs = action == want_action && diag == want_diag && nbr_n == want_nbr_n && near_n == want_near_n && valid == want_valid;
        std::printf("roundtrip by %d: %s, outputs %s, done %d %d %d\n", threads, std::memcmp(back.data(), good.data(), (size_t)total) == 0 ? "equal" : "DIFFERENT",
                    outputs ? "equal" : "DIFFERENT", done[0], done[1], done[2]);
    }
    return 0;
}
#endif
