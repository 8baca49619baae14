/*
 * sca_dubins_oracle.c -- CPU restatement of SCA's Dubins v_pref tracker and its 3-D Dubins planner.  TEST INFRASTRUCTURE ONLY.
 *
 * The second checker of the tracker.  The product's tracker (sca_amd/csrc/sca_dubins.hpp) runs on a restatement of glibc's
 * sin / cos / atan2 / acos / pow on the host AND on the device, so a device-vs-host comparison cannot see a fault the two builds
 * share.  This file is written from the reference's Python, not from the product: it includes nothing of sca_amd/ and calls the
 * running libm's sin, cos, atan2, acos, sqrt, pow and floor directly.  Where a Python / numpy semantic was in doubt, the
 * recorded KATs (tests/golden/F7*, the tracked episodes) decided (tests/test_oracle_tracker.py pins this file to them).
 *
 * Restated (paths relative to the reference's mamp/):
 *   util.py:113 mod2pi                                 -> orc_mod2pi (sca_oracle.c)
 *   policies/sca/dubinsmaneuver2d.py:33-145 the six words, :148-176 dubins_path_planning_from_origin, :179-218
 *   dubins_path_planning, :260-280 get_coordinates, :283-297 get_position_in_segment
 *   policies/sca/dubinsmaneuver3d.py:34-113 dubinsmaneuver3d (the literal radius search), :116-132 compute_sampling,
 *   :135-162 try_to_construct
 *   policies/sca/scaPolicy.py:92-104 compute_dubins, :243-250 update_dubins, :253-261 dubins_path_node_pop,
 *   :264-338 compute_v_pref, util.py:23 reached, util.py:125-137 is_parallel
 * Not restated:
 *   generate_course (dubinsmaneuver2d.py:221-257) and the px / py / pyaw of dubins_path_planning (:212-214): the 3-D planner
 *   never reads them (it reads t, p, q, mode, length and the start yaw of each 2-D maneuver).  pi_2_pi is only used there.
 *   compute_v_pref's is_back2start branch (:280-289): agent.is_back2start is False from agent.py:59 on and nothing sets it.
 * The stored path: the reference materialises all samples of a plan and pops them in order; a sample is a pure function of
 * its index, so an agent keeps its two 2-D maneuvers and a cursor, and a sample is computed when it is popped.
 *
 * Arithmetic idioms (the same as sca_oracle.c's, see its header): x ** 2 == pow(x, 2.0); np.dot(float64[3], float64[3]) ==
 * fma(a2, b2, fma(a1, b1, a0 * b0)); np.linalg.norm(float32[3]) in float32 with the products summed in double.
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

/* from sca_oracle.c (same library) */
double orc_mod2pi(double theta);
double orc_round5_py(double x);
double orc_round5_np(double x);
double orc_trunc5(double x);
double orc_l3norm(const double *p1, const double *p2);

#define DUB_MAX_DOUBLINGS 1100   /* dubinsmaneuver3d.py:76-78 loops forever when no radius works; b = 2^1100 overflowed long before */

/* status bits of a plan / a tracker call (the reference raises or loops forever in these cases) */
#define DST_NO_MANEUVER 1        /* the doubling loop hit DUB_MAX_DOUBLINGS, or no word was feasible (generate_course would raise) */
#define DST_EMPTY_POP   2        /* agent.dubins_path.pop() on an empty list (scaPolicy.py:278 / :326 raise IndexError) */
#define DST_ACOS_DOMAIN 4        /* acos argument below -1 (scaPolicy.py:297 raises ValueError); clamped */

static const double PI = 3.141592653589793;   /* math.pi */

static inline double mod2pi(double x) { return orc_mod2pi(x); }
static inline double dot3(const double *a, const double *b) { return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0])); }
static inline float norm3f(const float *a) {
    double s = (double)(float)(a[0] * a[0]);
    s += (double)(float)(a[1] * a[1]);
    s += (double)(float)(a[2] * a[2]);
    return sqrtf((float)s);
}

/* ------------------------------------------------------------------ 2-D maneuver (dubinsmaneuver2d.py) */
/* What DubinsManeuver holds that anything downstream reads: qi[2] (yaw), r_min, t, p, q, mode, length. */
typedef struct { double yaw, r_min, t, p, q, length; char mode[3]; int ok; } Man2;

/* :33-145, one function per word; returns 0 where the reference returns None.  Statements in the reference's order. */
static int LSL(double alpha, double beta, double d, double *t, double *p, double *q) {
    double sa = sin(alpha), sb = sin(beta), ca = cos(alpha), cb = cos(beta), c_ab = cos(alpha - beta);
    double tmp0 = d + sa - sb;
    double p_squared = 2 + (d * d) - (2 * c_ab) + (2 * d * (sa - sb));
    if (p_squared < 0) return 0;
    double tmp1 = atan2((cb - ca), tmp0);
    *t = mod2pi(-alpha + tmp1);
    *p = sqrt(p_squared);
    *q = mod2pi(beta - tmp1);
    return 1;
}
static int RSR(double alpha, double beta, double d, double *t, double *p, double *q) {
    double sa = sin(alpha), sb = sin(beta), ca = cos(alpha), cb = cos(beta), c_ab = cos(alpha - beta);
    double tmp0 = d - sa + sb;
    double p_squared = 2 + (d * d) - (2 * c_ab) + (2 * d * (sb - sa));
    if (p_squared < 0) return 0;
    double tmp1 = atan2((ca - cb), tmp0);
    *t = mod2pi(alpha - tmp1);
    *p = sqrt(p_squared);
    *q = mod2pi(-beta + tmp1);
    return 1;
}
static int LSR(double alpha, double beta, double d, double *t, double *p, double *q) {
    double sa = sin(alpha), sb = sin(beta), ca = cos(alpha), cb = cos(beta), c_ab = cos(alpha - beta);
    double p_squared = -2 + (d * d) + (2 * c_ab) + (2 * d * (sa + sb));
    if (p_squared < 0) return 0;
    *p = sqrt(p_squared);
    double tmp2 = atan2((-ca - cb), (d + sa + sb)) - atan2(-2.0, *p);
    *t = mod2pi(-alpha + tmp2);
    *q = mod2pi(-mod2pi(beta) + tmp2);
    return 1;
}
static int RSL(double alpha, double beta, double d, double *t, double *p, double *q) {
    double sa = sin(alpha), sb = sin(beta), ca = cos(alpha), cb = cos(beta), c_ab = cos(alpha - beta);
    double p_squared = (d * d) - 2 + (2 * c_ab) - (2 * d * (sa + sb));
    if (p_squared < 0) return 0;
    *p = sqrt(p_squared);
    double tmp2 = atan2((ca + cb), (d - sa - sb)) - atan2(2.0, *p);
    *t = mod2pi(alpha - tmp2);
    *q = mod2pi(beta - tmp2);
    return 1;
}
static int RLR(double alpha, double beta, double d, double *t, double *p, double *q) {
    double sa = sin(alpha), sb = sin(beta), ca = cos(alpha), cb = cos(beta), c_ab = cos(alpha - beta);
    double tmp_rlr = (6.0 - d * d + 2.0 * c_ab + 2.0 * d * (sa - sb)) / 8.0;
    if (fabs(tmp_rlr) > 1.0) return 0;
    *p = mod2pi(2 * PI - acos(tmp_rlr));
    *t = mod2pi(alpha - atan2(ca - cb, d - sa + sb) + mod2pi(*p / 2.0));
    *q = mod2pi(alpha - beta - *t + mod2pi(*p));
    return 1;
}
static int LRL(double alpha, double beta, double d, double *t, double *p, double *q) {
    double sa = sin(alpha), sb = sin(beta), ca = cos(alpha), cb = cos(beta), c_ab = cos(alpha - beta);
    double tmp_lrl = (6. - d * d + 2 * c_ab + 2 * d * (-sa + sb)) / 8.;
    if (fabs(tmp_lrl) > 1) return 0;
    *p = mod2pi(2 * PI - acos(tmp_lrl));
    *t = mod2pi(-alpha - atan2(ca - cb, d + sa - sb) + *p / 2.);
    *q = mod2pi(mod2pi(beta) - alpha - *t + mod2pi(*p));
    return 1;
}

typedef int (*WordFn)(double, double, double, double *, double *, double *);
static const WordFn PLANNERS[6] = {LSL, RSR, LSR, RSL, RLR, LRL};      /* :159, in this order */
static const char *const WORDS[6] = {"LSL", "RSR", "LSR", "RSL", "RLR", "LRL"};

/* :179-218 dubins_path_planning with :148-176 dubins_path_planning_from_origin inlined */
static void dubins_path_planning(const double start[3], const double end[3], double c, Man2 *m) {
    double sx = start[0], sy = start[1], syaw = start[2];
    double ex = end[0] - sx, ey = end[1] - sy, eyaw = end[2];
    double D = sqrt(pow(ex, 2.0) + pow(ey, 2.0));
    double d = D / c;
    double theta = mod2pi(atan2(ey, ex));
    double alpha = mod2pi(syaw - theta);
    double beta = mod2pi(eyaw - theta);
    double bcost = INFINITY;
    m->yaw = syaw; m->r_min = c; m->ok = 0;
    m->t = m->p = m->q = -1.0;
    m->mode[0] = m->mode[1] = m->mode[2] = 0;
    for (int w = 0; w < 6; w++) {
        double t, p, q;
        if (!PLANNERS[w](alpha, beta, d, &t, &p, &q)) continue;
        double cost = c * (fabs(t) + fabs(p) + fabs(q));
        if (bcost > cost) {                                          /* strict: the first of equal costs stays */
            m->t = t; m->p = p; m->q = q; memcpy(m->mode, WORDS[w], 3); bcost = cost; m->ok = 1;
        }
    }
    m->length = bcost;                                               /* maneuver.length = clen = bcost */
}

/* :283-297 get_position_in_segment */
static void get_position_in_segment(double offset, const double qi[3], char mode, double q[3]) {
    q[0] = q[1] = q[2] = 0.0;
    if (mode == 'L') {
        q[0] = qi[0] + sin(qi[2] + offset) - sin(qi[2]);
        q[1] = qi[1] - cos(qi[2] + offset) + cos(qi[2]);
        q[2] = qi[2] + offset;
    } else if (mode == 'R') {
        q[0] = qi[0] - sin(qi[2] - offset) + sin(qi[2]);
        q[1] = qi[1] + cos(qi[2] - offset) - cos(qi[2]);
        q[2] = qi[2] - offset;
    } else if (mode == 'S') {
        q[0] = qi[0] + cos(qi[2]) * offset;
        q[1] = qi[1] + sin(qi[2]) * offset;
        q[2] = qi[2];
    }
}
/* :260-280 get_coordinates */
static void get_coordinates(const Man2 *m, double offset, double q[3]) {
    double noffset = offset / m->r_min;
    double qi[3] = {0., 0., m->yaw};
    double l1 = m->t, l2 = m->p, q1[3], q2[3];
    get_position_in_segment(l1, qi, m->mode[0], q1);
    get_position_in_segment(l2, q1, m->mode[1], q2);
    if (noffset < l1) get_position_in_segment(noffset, qi, m->mode[0], q);
    else if (noffset < (l1 + l2)) get_position_in_segment(noffset - l1, q1, m->mode[1], q);
    else get_position_in_segment(noffset - l1 - l2, q2, m->mode[2], q);
    q[0] = q[0] * m->r_min + qi[0];
    q[1] = q[1] * m->r_min + qi[1];
    q[2] = mod2pi(q[2]);
}

/* ------------------------------------------------------------------ 3-D planner (dubinsmaneuver3d.py) */
typedef struct {
    Man2 h, v;                   /* maneuvers2d = fb */
    double qi[5];
    double length, sampling_size;
    int64_t count;               /* len(np.arange(0, length + sampling_size, sampling_size)) */
    int iters;                   /* try_to_construct calls the search made after `fa` (statistics, compared with the product's) */
    int status;                  /* DST_* */
    char mode[7];
} Plan3;

/* :135-162 try_to_construct; returns len() of its result (0 or 2) */
static int try_to_construct(const double qi[5], const double qf[5], double Rmin, const double pitchlims[2], double horizontal_radius,
                            Man2 *mh, Man2 *mv) {
    double qi2D[3] = {qi[0], qi[1], qi[3]}, qf2D[3] = {qf[0], qf[1], qf[3]};
    dubins_path_planning(qi2D, qf2D, horizontal_radius, mh);
    double qi3D[3] = {0.0, qi[2], qi[4]}, qf3D[3] = {mh->length, qf[2], qf[4]};
    double vertical_curvature = sqrt(1.0 / pow(Rmin, 2.0) - 1.0 / pow(horizontal_radius, 2.0));
    if (vertical_curvature < 1e-5) return 0;
    double vertical_radius = 1.0 / vertical_curvature;
    dubins_path_planning(qi3D, qf3D, vertical_radius, mv);
    if (mv->mode[0] == 'R' && mv->mode[1] == 'L' && mv->mode[2] == 'R') return 0;
    if (mv->mode[0] == 'R') { if (qi[4] - mv->t < pitchlims[0]) return 0; }
    else { if (qi[4] + mv->t > pitchlims[1]) return 0; }
    return 2;
}

/* :116-132 compute_sampling: the grid (the samples themselves: plan_sample) */
static void compute_sampling(Plan3 *P) {
    double sampling_size = 0.1;                                       /* called with sampling_size=0.1 (:111) */
    if (P->length > 100) sampling_size = P->length / 1000;
    P->sampling_size = sampling_size;
    /* np.arange(0, stop, step): ceil((stop - 0) / step) elements, element i = 0 + i * step */
    double n = ceil((P->length + sampling_size) / sampling_size);
    P->count = n > 0 ? (int64_t)n : 0;
}
/* element k of maneuver3d.path (:123-132) */
static void plan_sample(const Plan3 *P, int64_t k, double s[5]) {
    double offset = (double)k * P->sampling_size, qSZ[3], qXY[3];
    get_coordinates(&P->v, offset, qSZ);
    get_coordinates(&P->h, qSZ[0], qXY);
    s[0] = qXY[0] + P->qi[0]; s[1] = qXY[1] + P->qi[1]; s[2] = qSZ[1] + P->qi[2]; s[3] = qXY[2]; s[4] = qSZ[2];
}

/* :34-113 dubinsmaneuver3d, the literal search */
static void dubinsmaneuver3d(const double qi[5], const double qf[5], double Rmin, const double pitchlims[2], Plan3 *P) {
    memset(P, 0, sizeof *P);
    memcpy(P->qi, qi, sizeof P->qi);
    P->length = -1.0;
    double b = 1.0;
    Man2 fbh, fbv, fch, fcv;
    /* fa = try_to_construct(Rmin * 1.0) (:74): its result is overwritten at :101 before anything reads it; not computed */
    int nfb = try_to_construct(qi, qf, Rmin, pitchlims, Rmin * b, &fbh, &fbv);
    P->iters = 1;
    int doublings = 0;
    while (nfb < 2) {
        if (++doublings > DUB_MAX_DOUBLINGS) { P->status |= DST_NO_MANEUVER; return; }
        b *= 2.0;
        nfb = try_to_construct(qi, qf, Rmin, pitchlims, Rmin * b, &fbh, &fbv);
        P->iters++;
    }
    double step = 0.1;                                                /* local optimisation (:86-100) */
    while (fabs(step) > 1e-10) {
        double c = b + step;
        if (c < 1.0) c = 1.0;
        int nfc = try_to_construct(qi, qf, Rmin, pitchlims, Rmin * c, &fch, &fcv);
        P->iters++;
        if (nfc > 0) {
            if (fcv.length < fbv.length) { b = c; fbh = fch; fbv = fcv; step *= 2.; continue; }
        }
        step *= -0.1;
    }
    P->h = fbh; P->v = fbv;
    P->length = fbv.length;
    if (!fbh.ok || !fbv.ok) P->status |= DST_NO_MANEUVER;
    memcpy(P->mode, fbh.mode, 3); memcpy(P->mode + 3, fbv.mode, 3); P->mode[6] = 0;
    compute_sampling(P);
}

/* One plan.  out[12] = length, h.r_min, h.t, h.p, h.q, v.r_min, v.t, v.p, v.q, sampling_size, count, iters; mode7 = the six letters
 * + NUL; samples[5 * j] = path element ks[j] (0 <= ks[j] < count).  Returns the DST_* status. */
int orc_dubins_plan(const double *qi, const double *qf, double rmin, double pitch_lo, double pitch_hi, double *out, char *mode7,
                    const int64_t *ks, int nk, double *samples) {
    const double pl[2] = {pitch_lo, pitch_hi};
    Plan3 P;
    dubinsmaneuver3d(qi, qf, rmin, pl, &P);
    const double o[12] = {P.length, P.h.r_min, P.h.t, P.h.p, P.h.q, P.v.r_min, P.v.t, P.v.p, P.v.q, P.sampling_size, (double)P.count, (double)P.iters};
    memcpy(out, o, sizeof o);
    memcpy(mode7, P.mode, 7);
    if (P.status) return P.status;
    for (int j = 0; j < nk; j++) {
        if (ks[j] < 0 || ks[j] >= P.count) return -1;
        plan_sample(&P, ks[j], samples + 5 * (size_t)j);
    }
    return 0;
}

/* Many plans (the pose fuzz): q[10 * i] = qi[5], qf[5]; rmin / pitch_lo / pitch_hi per plan; out[16 * i] = the 12 values of
 * orc_dubins_plan, then the two words packed as 65536 * c0 + 256 * c1 + c2, the status, and 0. */
int orc_dubins_plan_batch(int n, const double *q, const double *rmin, const double *pitch_lo, const double *pitch_hi, double *out,
                          int nthreads) {
    int bad = 0;
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : bad)
#endif
    for (int i = 0; i < n; i++) {
        const double pl[2] = {pitch_lo[i], pitch_hi[i]};
        Plan3 P;
        dubinsmaneuver3d(q + 10 * (size_t)i, q + 10 * (size_t)i + 5, rmin[i], pl, &P);
        double *o = out + 16 * (size_t)i;
        const double r[16] = {P.length, P.h.r_min, P.h.t, P.h.p, P.h.q, P.v.r_min, P.v.t, P.v.p, P.v.q, P.sampling_size, (double)P.count,
                              (double)P.iters, P.mode[0] * 65536.0 + P.mode[1] * 256.0 + P.mode[2],
                              P.mode[3] * 65536.0 + P.mode[4] * 256.0 + P.mode[5], (double)P.status, 0.0};
        memcpy(o, r, sizeof r);
        bad += P.status != 0;
    }
    return bad;
}

/* ------------------------------------------------------------------ the tracker (scaPolicy.py:243-338) */
typedef struct {
    int is_use_dubins;
    Plan3 plan;
    int64_t next;                /* agent.dubins_path == elements [next, plan.count) of the plan, popped in this order */
    double now_goal[3];          /* agent.dubins_now_goal */
    double sampling_size;        /* agent.dubins_sampling_size */
    double v_pref[3];            /* agent.v_pref (before the truncation of :337) */
    int replans;
    int status;                  /* DST_* seen by this agent so far */
} OTrack;

typedef struct {
    int n;
    double *goal, *goal_heading, *pref_speed;
    uint8_t *zaxis;              /* is_zAxis (:300-301), a function of the agent's start and goal */
    double turning_radius, pitch_lo, pitch_hi, neighbor_dist;
    double *nd_pa, *R_pa, *plo_pa, *phi_pa;   /* per agent (agent.neighborDist / turning_radius / pitchlims), NULL: the values above */
    OTrack *st;
} OTracker;

static double *dup_or_null(const double *a, int n) {
    if (!a) return NULL;
    double *r = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    memcpy(r, a, sizeof(double) * (size_t)n);
    return r;
}

void *orc_tracker_create(int n, const double *goal, const double *goal_heading, const double *pref_speed, const uint8_t *zaxis,
                         double turning_radius, double pitch_lo, double pitch_hi, double neighbor_dist) {
    if (n < 0 || !goal || !goal_heading || !pref_speed || !zaxis) return NULL;
    OTracker *T = (OTracker *)calloc(1, sizeof(OTracker));
    T->n = n;
    T->goal = dup_or_null(goal, 3 * n);
    T->goal_heading = dup_or_null(goal_heading, 3 * n);
    T->pref_speed = dup_or_null(pref_speed, n);
    T->zaxis = (uint8_t *)malloc((size_t)(n > 0 ? n : 1));
    memcpy(T->zaxis, zaxis, (size_t)n);
    T->turning_radius = turning_radius; T->pitch_lo = pitch_lo; T->pitch_hi = pitch_hi; T->neighbor_dist = neighbor_dist;
    T->st = (OTrack *)calloc((size_t)(n > 0 ? n : 1), sizeof(OTrack));
    return T;
}
void orc_tracker_destroy(void *h) {
    OTracker *T = (OTracker *)h;
    if (!T) return;
    free(T->goal); free(T->goal_heading); free(T->pref_speed); free(T->zaxis);
    free(T->nd_pa); free(T->R_pa); free(T->plo_pa); free(T->phi_pa);
    free(T->st); free(T);
}
/* per-agent attributes (arrays of n; NULL: the create-time value for everybody) */
int orc_tracker_set_params(void *h, const double *neighbor_dist, const double *turning_radius, const double *pitch_lo, const double *pitch_hi) {
    OTracker *T = (OTracker *)h;
    if (!T) return -1;
    free(T->nd_pa); free(T->R_pa); free(T->plo_pa); free(T->phi_pa);
    T->nd_pa = dup_or_null(neighbor_dist, T->n);
    T->R_pa = dup_or_null(turning_radius, T->n);
    T->plo_pa = dup_or_null(pitch_lo, T->n);
    T->phi_pa = dup_or_null(pitch_hi, T->n);
    return 0;
}

static inline double agent_R(const OTracker *T, int i) { return T->R_pa ? T->R_pa[i] : T->turning_radius; }

/* :92-104 compute_dubins + :253-261 dubins_path_node_pop + `dubins_now_goal = path.pop()[:3]` (:276-278, :323-326) */
static void replan(const OTracker *T, OTrack *a, int i, const double *pos, const double *heading) {
    const double qi[5] = {pos[0], pos[1], pos[2], heading[0], heading[1]};             /* np.hstack((pos, heading))[:5] */
    const double *g = &T->goal[3 * i], *gh = &T->goal_heading[3 * i];
    const double qf[5] = {g[0], g[1], g[2], gh[0], gh[1]};
    const double pl[2] = {T->plo_pa ? T->plo_pa[i] : T->pitch_lo, T->phi_pa ? T->phi_pa[i] : T->pitch_hi};
    dubinsmaneuver3d(qi, qf, agent_R(T, i), pl, &a->plan);
    a->status |= a->plan.status;
    a->sampling_size = a->plan.sampling_size;
    a->next = 0;
    a->replans++;
    for (int k = 0; k < 4; k++) if (a->next < a->plan.count) a->next++;           /* four guarded pops, values unused */
    if (a->next < a->plan.count) {
        double s[5];
        plan_sample(&a->plan, a->next++, s);
        a->now_goal[0] = s[0]; a->now_goal[1] = s[1]; a->now_goal[2] = s[2];
    } else {
        a->status |= DST_EMPTY_POP;                                                    /* the reference raises; now_goal kept */
    }
}
/* :243-250 update_dubins */
static void update_dubins(const OTracker *T, OTrack *a, int i, const double *pos) {
    double dis = orc_l3norm(pos, a->now_goal);
    if (dis < a->sampling_size * 2) {
        if (a->next < a->plan.count) {
            double s[5];
            plan_sample(&a->plan, a->next++, s);
            a->now_goal[0] = s[0]; a->now_goal[1] = s[1]; a->now_goal[2] = s[2];
        } else {
            memcpy(a->now_goal, &T->goal[3 * i], sizeof a->now_goal);
        }
    }
}
/* util.py:125-137 is_parallel(vA float32, v_pref float64) */
static int is_parallel(const float *vec1, const double *vec2) {
    float norm_vec1 = norm3f(vec1);
    double norm_vec2 = sqrt(dot3(vec2, vec2));
    float v1n[3] = {vec1[0] / norm_vec1, vec1[1] / norm_vec1, vec1[2] / norm_vec1};               /* float32 / float32 */
    double v2n[3] = {vec2[0] / norm_vec2, vec2[1] / norm_vec2, vec2[2] / norm_vec2};
    if ((double)norm_vec1 <= 1e-5 || norm_vec2 <= 1e-5) return 1;
    double v1d[3] = {(double)v1n[0], (double)v1n[1], (double)v1n[2]};                          /* np.dot promotes to float64 */
    return orc_round5_np(1.0 - fabs(dot3(v1d, v2n))) < 3e-3;                                     /* np.float64: numpy's round */
}

/* :264-338 compute_v_pref for agent i; nbr0_dsq < 0: agent.neighbors is empty */
static void compute_v_pref(const OTracker *T, OTrack *a, int i, const double *pos, const float *vel, const double *heading, double nbr0_dsq,
                           double *V_des) {
    const double *goal = &T->goal[3 * i];
    double dif_x[3];
    double dis_goal = orc_l3norm(pos, goal);
    double k = 3.0 * agent_R(T, i);
    if (!a->is_use_dubins) {                                                       /* first (:273-279) */
        a->is_use_dubins = 1;
        replan(T, a, i, pos, heading);
        for (int q = 0; q < 3; q++) dif_x[q] = a->now_goal[q] - pos[q];
    } else {
        update_dubins(T, a, i, pos);
        double dis = orc_l3norm(pos, a->now_goal);
        double max_size = orc_round5_py(6 * a->sampling_size);
        double pApG[3] = {goal[0] - pos[0], goal[1] - pos[1], goal[2] - pos[2]};
        double vA64[3] = {(double)vel[0], (double)vel[1], (double)vel[2]};
        double x = dot3(vA64, pApG) / ((double)norm3f(vel) * sqrt(dot3(pApG, pApG)));
        if (1.0 < x) x = 1.0;                                                       /* Python min(x, 1.0): nan stays nan */
        if (x < -1.0) { a->status |= DST_ACOS_DOMAIN; x = -1.0; }
        double theta = orc_round5_py(acos(x));                                      /* round(nan, 5) is nan */
        double deg100 = orc_round5_np(100.0 * (PI / 180.0));                       /* np.deg2rad(100), numpy's round */
        double nd = T->nd_pa ? T->nd_pa[i] : T->neighbor_dist;
        double min_dist_ob = nbr0_dsq >= 0 ? orc_round5_py(sqrt(nbr0_dsq)) : rint(nd);   /* round(x): half to even */
        int condition_dist = T->zaxis[i] ? (min_dist_ob >= 2.0 * agent_R(T, i)) : 0;
        if (((is_parallel(vel, a->v_pref) || dis_goal <= k) && dis < max_size) || (theta >= deg100) || condition_dist) {
            update_dubins(T, a, i, pos);
            if (a->next < a->plan.count) for (int q = 0; q < 3; q++) dif_x[q] = a->now_goal[q] - pos[q];
            else for (int q = 0; q < 3; q++) dif_x[q] = goal[q] - pos[q];
        } else {
            replan(T, a, i, pos, heading);
            for (int q = 0; q < 3; q++) dif_x[q] = a->now_goal[q] - pos[q];
        }
    }
    const double zero[3] = {0, 0, 0};
    double norm = orc_l3norm(dif_x, zero);
    double v[3];
    for (int q = 0; q < 3; q++) v[q] = dif_x[q] * T->pref_speed[i] / norm;
    if (orc_l3norm(goal, pos) < 0.2) v[0] = v[1] = v[2] = 0.0;                    /* reached(goal, pos, bound=0.2) */
    for (int q = 0; q < 3; q++) { a->v_pref[q] = v[q]; V_des[q] = orc_trunc5(v[q]); }
}

/* One compute_v_pref for every active agent (out rows of inactive agents are left alone).  nbr0_dsq[i] = agent.neighbors[0][1] of
 * the previous pass, negative when the list is empty.  Returns the number of agents that carry a DST_* status. */
int orc_tracker_vpref(void *h, const double *pos, const float *vel, const double *heading, const uint8_t *active, const double *nbr0_dsq,
                      double *out, int nthreads) {
    OTracker *T = (OTracker *)h;
    if (!T) return -1;
    int bad = 0;
#ifdef _OPENMP
    if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : bad)
#endif
    for (int i = 0; i < T->n; i++) {
        if (!active[i]) continue;
        compute_v_pref(T, &T->st[i], i, pos + 3 * (size_t)i, vel + 3 * (size_t)i, heading + 3 * (size_t)i, nbr0_dsq[i], out + 3 * (size_t)i);
        bad += T->st[i].status != 0;
    }
    return bad;
}
int orc_tracker_replans(void *h, int32_t *replans) {
    OTracker *T = (OTracker *)h;
    if (!T) return -1;
    for (int i = 0; i < T->n; i++) replans[i] = T->st[i].replans;
    return 0;
}
/* agent i's state in the layout of the product's sca_tracker_debug record (24 doubles): h.r_min, h.t, h.p, h.length, v.r_min, v.t, v.p,
 * v.length, length, sampling_size, 0, next, count, now_goal[3], v_pref[3], word h, word v, 64 * iters, replans; o[11] = status */
int orc_tracker_debug(void *h, int i, double *o) {
    OTracker *T = (OTracker *)h;
    if (!T || i < 0 || i >= T->n) return -1;
    const OTrack *a = &T->st[i];
    const Plan3 *P = &a->plan;
    o[0] = P->h.r_min; o[1] = P->h.t; o[2] = P->h.p; o[3] = P->h.length; o[4] = P->v.r_min; o[5] = P->v.t; o[6] = P->v.p; o[7] = P->v.length;
    o[8] = P->length; o[9] = P->sampling_size; o[10] = 0.0; o[11] = (double)a->status; o[12] = (double)a->next; o[13] = (double)P->count;
    for (int q = 0; q < 3; q++) { o[14 + q] = a->now_goal[q]; o[17 + q] = a->v_pref[q]; }
    o[20] = P->mode[0] * 65536.0 + P->mode[1] * 256.0 + P->mode[2];
    o[21] = P->mode[3] * 65536.0 + P->mode[4] * 256.0 + P->mode[5];
    o[22] = 64.0 * P->iters; o[23] = (double)a->replans;
    return 0;
}
