// sca_respawn_attrs.h -- a respawn that brings the arriving agent's own policy, solver and planner attributes (sca_respawn_agents_attrs,
// sca_respawn_agents_gated_attrs; include/sca_hip.h).
//
// sca_respawn_agents keeps the row's policy and attributes; the reference keeps both as plain fields of the Agent object (agent.py:24-41),
// assigned between two env.step() calls like a new start.  Here a named row also takes a policy byte and the 64-byte AgentPar record
// sca_set_agent_params derives, so that afterwards it is what sca_set_agents(that policy) + sca_set_agent_params + sca_set_state
// (+ sca_device_tracker_enable) leave for such an agent; every other row keeps every word.
//
// Everything here is pure and compiles for the host (tests/respawn_attrs_harness.cpp):
//   respawn_attrs_check      the refusals the two entry points add to respawn_check's, with their codes, and the merged policies
//   respawn_attrs_layout     the sections of the page-locked block the new arrays travel in (a block of its own: the call's other arrays
//                            stay in RespawnLayout's, so a context that never brings attributes allocates nothing of this)
//   respawn_attrs_pack       policy bytes, records, neighborDist, planner triples and class bytes into that block; respawn_attrs_bits: the rows' bytes of RSB_BITS
//   respawn_attrs_write_row  what one lane of the wavefront that serves a row stores: the function k_respawn_attrs calls per row
//   plain_class_table        scene_class_table's rule over a plain context's rows, by a mask
//   respawn_lp_list          the ORCA3D-LP list behind a call (ascending ids)
#pragma once
#include <vector>

#include "sca_respawn.h"

namespace sca {

// ---- the refusals ------------------------------------------------------------------------------------------------------------------------
enum RespawnAttrFault {
    RSA_OK = 0,
    RSA_BAD_POLICY,         // a policy byte above SCA_POLICY_RVO3D_DUBINS (entry: the packed row)                      } SCA_ERR_ARG
    RSA_STRUCT,             // struct_bytes below the leading integers, above the library's struct, or cutting a pointer  }
    RSA_RESERVED,           // reserved != 0                                                                             }
    RSA_NO_TRACKER,         // turning_radius / pitch_lo / pitch_hi while no device tracker is enabled                   }
    RSA_SOLVER,             // a solver attribute out of sca_set_agent_params' range (entry: the packed row)             }
    RSA_PLANNER             // a row whose NEW policy is tracked and whose turning radius / pitch limits break            }
                            // sca_device_tracker_set_agent_params' rules (entry: the packed row)
};
inline int respawn_attrs_error_code(RespawnAttrFault f) { return f == RSA_OK ? SCA_OK : SCA_ERR_ARG; }
// respawn_check's verdicts that are reached only behind its look at every id: the rows can be read by id then
inline bool respawn_ids_checked(RespawnFault f) {
    return f == RSP_OK || f == RSP_GOAL_HEADING || f == RSP_PATH_HALF || f == RSP_PATH_OFFSETS || f == RSP_PATH_TOO_LONG || f == RSP_PATH_NOT_FINITE ||
           f == RSP_PATH_BLOCK || f == RSP_PATH_NO_SLOTS;
}
// base: respawn_check's verdict, judged by the NEW policies (goal_heading == NULL is refused for a row whose new policy is tracked);
// fault: this header's, looked at only where base is RSP_OK or a verdict behind the ids
struct RespawnAttrCheck { RespawnCheck base; RespawnAttrFault fault; int entry; };
// the descriptor as far as struct_bytes reaches (restart_attrs_check's rule, sca_scenes.h)
inline RespawnAttrFault respawn_attrs_read(const sca_restart_attrs *in, RestartAttrs *out) {
    const int sb = in->struct_bytes;
    if (sb < RESTART_ATTR_HEAD_BYTES || sb > (int)sizeof(sca_restart_attrs) || (sb - RESTART_ATTR_HEAD_BYTES) % (int)sizeof(void *) != 0) return RSA_STRUCT;
    if (in->reserved != 0) return RSA_RESERVED;
    sca_restart_attrs full{};                                          // (members behind struct_bytes stay NULL)
    std::memcpy(&full, in, (std::size_t)sb);
    RestartAttrs R;
    R.neighbor_dist = full.neighbor_dist; R.max_neighbors = full.max_neighbors; R.time_step = full.time_step; R.time_horizon = full.time_horizon;
    R.max_speed = full.max_speed; R.max_heading_change = full.max_heading_change; R.dt_nominal = full.dt_nominal;
    R.turning_radius = full.turning_radius; R.pitch_lo = full.pitch_lo; R.pitch_hi = full.pitch_hi;
    *out = R;
    return RSA_OK;
}
// C: the context with the policies AS THEY STAND; policy (nullable): the call's bytes; in (nullable): the descriptor.  merged: [n] the
// policies behind the call, filled where the ids could be read.  The order: respawn_check's refusals up to the ids, the policy bytes, respawn_check's remaining ones by
// the new policies, the descriptor, the rows' attributes.
inline RespawnAttrCheck respawn_attrs_check(const RespawnCtx &C, const RespawnArgs &A, const uint8_t *policy, const sca_restart_attrs *in,
                                            const AttrDefaults &D, std::vector<uint8_t> &merged, RestartAttrs *out) {
    RespawnCheck base = respawn_check(C, A);
    if (!respawn_ids_checked(base.fault)) return {base, RSA_OK, -1};
    if (policy) {
        for (int r = 0; r < A.count; r++) if (policy[r] > SCA_POLICY_RVO3D_DUBINS) return {RespawnCheck{RSP_OK, -1, 0}, RSA_BAD_POLICY, r};
        merged.assign(C.policy_now, C.policy_now + C.n);
        for (int r = 0; r < A.count; r++) merged[(std::size_t)A.ids[r]] = policy[r];
        RespawnCtx N = C;
        N.policy_now = merged.data();
        base = respawn_check(N, A);
    } else merged.assign(C.policy_now, C.policy_now + C.n);
    if (base.fault != RSP_OK) return {base, RSA_OK, -1};
    RestartAttrs R;
    if (in) {
        if (const RespawnAttrFault f = respawn_attrs_read(in, &R)) return {base, f, -1};
        if (R.planner() && !C.tracker_on) return {base, RSA_NO_TRACKER, -1};
        if (R.solver())
            for (int r = 0; r < A.count; r++)
                if (!restart_attr_solver_ok(R.neighbor_dist ? R.neighbor_dist[r] : D.neighbor_dist, R.max_neighbors ? R.max_neighbors[r] : D.max_neighbors,
                                            R.time_step ? R.time_step[r] : D.time_step, R.time_horizon ? R.time_horizon[r] : D.time_horizon,
                                            R.max_speed ? R.max_speed[r] : D.max_speed, R.max_heading_change ? R.max_heading_change[r] : D.max_heading_change,
                                            R.dt_nominal ? R.dt_nominal[r] : D.dt_nominal))
                    return {base, RSA_SOLVER, r};
    }
    if (in && R.planner())                                             // (planner entries of rows whose new policy is untracked are ignored)
        for (int r = 0; r < A.count; r++)
            if (restart_policy_tracked(merged[(std::size_t)A.ids[r]]) &&
                !restart_attr_planner_ok(R.turning_radius ? R.turning_radius[r] : D.turning_radius, R.pitch_lo ? R.pitch_lo[r] : D.pitch_lo,
                                         R.pitch_hi ? R.pitch_hi[r] : D.pitch_hi))
                return {base, RSA_PLANNER, r};
    *out = R;
    return {base, RSA_OK, -1};
}

// ---- the block ---------------------------------------------------------------------------------------------------------------------------
// One section per array, aligned to 64 bytes like RespawnLayout's: the policy bytes, the AgentPar records (64 bytes, derived on the host
// exactly as sca_set_agent_params derives them; the kernel copies them as 16-byte pieces) and the rows' neighborDist alone (the tracker's
// array, TrackView::nd_per_agent), the planner triple (turning radius, pitch_lo, pitch_hi) and the row's class byte.
enum RespawnAttrSection : int { RAB_POLICY = 0, RAB_PAR, RAB_ND, RAB_TRIPLE, RAB_CLASS, RAB_SECTIONS };
constexpr int RSP_PAR_BYTES = 64;
static_assert(sizeof(AgentPar) == RSP_PAR_BYTES, "the block's records are AgentPar records");
struct RespawnAttrLayout { int64_t off[RAB_SECTIONS]; int64_t total; };
inline int64_t respawn_attrs_section_bytes(int s, int cap) {
    return (s == RAB_POLICY || s == RAB_CLASS ? 1 : s == RAB_PAR ? RSP_PAR_BYTES : s == RAB_ND ? 8 : 24) * (int64_t)cap;
}
inline RespawnAttrLayout respawn_attrs_layout(int cap) {
    RespawnAttrLayout L;
    int64_t at = 0;
    for (int s = 0; s < RAB_SECTIONS; s++) {
        L.off[s] = at;
        at += (respawn_attrs_section_bytes(s, cap) + RSP_ALIGN - 1) / RSP_ALIGN * RSP_ALIGN;
    }
    L.total = at;
    return L;
}
// further bits of the call's `has` word (respawn_row reads the lower ones alone)
constexpr uint32_t RESPAWN_HAS_POLICY = 8,       // the rows take the call's policy bytes (else they keep theirs)
                   RESPAWN_HAS_ATTRS = 16,       // the rows take the block's AgentPar records and neighborDist (else they keep theirs)
                   RESPAWN_HAS_PLANNER = 32;     // the rows take the block's planner triples and class bytes (else they keep theirs)
// a further bit of a row's byte in RSB_BITS
constexpr uint8_t RSP_BIT_UNTRACK = 4;           // the device tracker is on and the row LEAVES the tracked policies: what k_scene_restart leaves for
                                                 // that transition -- vpref_ext 0, the initial AgentTrack, and (RSP_BIT_MODE_RESET with it) vpref_mode 0
// policy / par / trip with cls (each nullable): [count] in the call's order
inline uint32_t respawn_attrs_pack(uint8_t *blk, const RespawnAttrLayout &L, int count, const uint8_t *policy, const AgentPar *par, const TrackTriple *trip = nullptr,
                                   const uint8_t *cls = nullptr) {
    uint32_t has = 0;
    if (policy) { std::memcpy(blk + L.off[RAB_POLICY], policy, (std::size_t)count); has |= RESPAWN_HAS_POLICY; }
    if (par) {
        std::memcpy(blk + L.off[RAB_PAR], par, sizeof(AgentPar) * (std::size_t)count);
        double *nd = (double *)(blk + L.off[RAB_ND]);
        for (int r = 0; r < count; r++) nd[r] = par[r].neighbor_dist;
        has |= RESPAWN_HAS_ATTRS;
    }
    if (trip) {
        double *t = (double *)(blk + L.off[RAB_TRIPLE]);
        for (int r = 0; r < count; r++) { t[3 * r] = trip[r].R; t[3 * r + 1] = trip[r].lo; t[3 * r + 2] = trip[r].hi; }
        std::memcpy(blk + L.off[RAB_CLASS], cls, (std::size_t)count);
        has |= RESPAWN_HAS_PLANNER;
    }
    return has;
}
// The rows' bytes of RSB_BITS behind respawn_pack, which was given the NEW policies: RSP_BIT_TRACKED follows the new policy, and
// RSP_BIT_MODE_RESET the old list state and the new policy.  Here the rows that leave the tracker get their two bits.
inline void respawn_attrs_bits(uint8_t *bits, int count, const int32_t *ids, const uint8_t *policy_old, const uint8_t *policy_new, bool tracker_on) {
    if (!tracker_on) return;
    for (int r = 0; r < count; r++)
        if (restart_policy_tracked(policy_old[ids[r]]) && !restart_policy_tracked(policy_new[ids[r]])) bits[r] |= RSP_BIT_UNTRACK | RSP_BIT_MODE_RESET;
}

// ---- the row write -------------------------------------------------------------------------------------------------------------------------
// What one lane of the wavefront that serves row `a` stores BESIDE respawn_write_row (sca_respawn.h), all plain vector stores:
//   AgentPar          four 16-byte pieces by lanes 0 .. 3
//   policy, ap_nd     lane 0
//   planner triple    turning radius, pitch_lo, pitch_hi into their three arrays by lanes 0 .. 2; the class byte by lane 0
//   leaving the tracker   vpref_ext: one component per lane 0 .. 2; the AgentTrack record word by word from the one initial record
// Dev: RespawnDev's members (vpref_ext, trk_st, trk_init, trk_words); At: the arrays only this call writes (RespawnAttrDev in
// sca_respawn.hip.h; plain host arrays in the tests' harness); the planner's four arrays are read only with RESPAWN_HAS_PLANNER.
struct RespawnAttrSrc {
    const uint8_t *blk; const RespawnAttrLayout &L; int r;
    SCA_HD uint8_t policy() const { return (blk + L.off[RAB_POLICY])[r]; }
    SCA_HD RespawnPiece par_piece(int lane) const { return ((const RespawnPiece *)(blk + L.off[RAB_PAR] + (int64_t)RSP_PAR_BYTES * r))[lane]; }
    SCA_HD double nd() const { return ((const double *)(blk + L.off[RAB_ND]))[r]; }
    SCA_HD double triple(int k) const { return ((const double *)(blk + L.off[RAB_TRIPLE]))[3 * (int64_t)r + k]; }
    SCA_HD uint8_t cls() const { return (blk + L.off[RAB_CLASS])[r]; }
};
template <class Dev, class At, class Src>
SCA_HD void respawn_attrs_write_row(const Dev &d, const At &at, int a, int lane, uint8_t bits, uint32_t has, const Src &s) {
    if ((has & RESPAWN_HAS_ATTRS) && lane < RSP_PAR_BYTES / 16) ((RespawnPiece *)(at.ap + a))[lane] = s.par_piece(lane);
    if (lane == 0) {
        if (has & RESPAWN_HAS_POLICY) at.policy[a] = s.policy();
        if (has & RESPAWN_HAS_ATTRS) at.ap_nd[a] = s.nd();
        if (has & RESPAWN_HAS_PLANNER) at.trk_cls[a] = s.cls();
    }
    if ((has & RESPAWN_HAS_PLANNER) && lane < 3) (lane == 0 ? at.trk_R : lane == 1 ? at.trk_plo : at.trk_phi)[a] = s.triple(lane);
    if (bits & RSP_BIT_UNTRACK) {
        if (lane < 3) d.vpref_ext[3 * (int64_t)a + lane] = 0.0;
        if (d.trk_st) for (int k = lane; k < d.trk_words; k += 64) d.trk_st[(int64_t)a * d.trk_words + k] = d.trk_init[k];
    }
}

// ---- the tracker's classes in a plain context ----------------------------------------------------------------------------------------------
// scene_class_table's rule (sca_scenes.h) over the rows of `mask` (null: every row) of a plain context: the context is one scene of n rows
// in which a row outside the mask stands as an untracked one -- it is no user of any class and its byte is left alone.  More than
// TRK_CLASS_CAP triples: the per-agent form; at or below it the table comes back; a class keeps its index while a masked tracked row uses it.
inline ClassUpdate plain_class_table(ClassTable &tab, int n, const uint8_t *mask, const uint8_t *policy, const TrackTriple *trip, uint8_t *cls, const uint8_t *travels) {
    const int32_t off[2] = {0, n}, size[1] = {n};
    if (!mask) return scene_class_table(tab, 1, off, size, policy, trip, cls, travels);
    std::vector<uint8_t> pol(policy, policy + n);
    for (int i = 0; i < n; i++) if (!mask[i]) pol[(std::size_t)i] = SCA_POLICY_ORCA3D;
    return scene_class_table(tab, 1, off, size, pol.data(), trip, cls, travels);
}

// ---- the ORCA3D-LP list ------------------------------------------------------------------------------------------------------------------
// [n] policies -> the ids whose policy is ORCA3D-LP, ascending (what sca_set_agents builds); returns whether it differs from `now`
inline bool respawn_lp_list(const uint8_t *policy, int n, const std::vector<int32_t> &now, std::vector<int32_t> &out) {
    out.clear();
    for (int i = 0; i < n; i++) if (policy[i] == SCA_POLICY_ORCA3D_LP) out.push_back(i);
    return out != now;
}

}  // namespace sca
