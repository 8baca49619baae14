/* grid_rule_asan.c -- list rule 1 of the oracle (oracle/sca_oracle.c) in a program of its own, for a sanitizer build.
 *
 * tests/test_grid_rule_cpu.py compiles this file together with oracle/sca_oracle.c under -fsanitize=address,undefined, dumps fuzz scenes as
 * raw arrays and compares the checksum printed here with the one of the same pass through liboracle.so.
 *
 * usage: grid_rule_asan scene.bin ...      one line "checksum <hex>" per scene
 * scene.bin: int32 n, m, per_agent; then float64 pos[3n], float32 vel[3n], float64 heading[3n], radius[n], pref_speed[n], uint8 flags[n],
 *   float64 goal[3n], uint8 policy[n], zaxis[n], float64 vpref[3n], uint8 vmode[n], float64 obs_pos[3m], obs_radius[m], float64 params[8]
 *   (neighbor_dist, max_neighbors, time_step, time_horizon, max_speed, max_heading_change, near_goal_threshold, dt_nominal) and, with
 *   per_agent, float64 neighbor_dist[n], int32 max_neighbors[n], float64 time_step[n], time_horizon[n], max_speed[n],
 *   max_heading_change[n], dt_nominal[n]. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

void orc_set_list_rule(int rule);
void orc_set_params(double neighbor_dist, int max_neighbors, double time_step, double time_horizon, double max_speed,
                    double max_heading_change, double near_goal_threshold);
void orc_set_dt_nominal(double dt_nominal);
void orc_set_agent_params(int n, const double *neighbor_dist, const int32_t *max_neighbors, const double *time_step, const double *time_horizon,
                          const double *max_speed, const double *max_heading_change, const double *dt_nominal);
int orc_policy_step(int n, int m, const double *pos, const float *vel, const double *heading, const double *radius,
                    const double *pref_speed, uint8_t *flags, const double *goal, const uint8_t *policy,
                    const uint8_t *zaxis, const double *vpref_ext, const uint8_t *vpref_mode, int32_t *perm,
                    const double *obs_pos, const double *obs_radius, double *action64, float *action32,
                    int32_t *nbr_n, int32_t *nbr_id, uint8_t *nbr_kind, double *nbr_dsq, uint8_t *nbr_valid,
                    double *vpref_used, int32_t *diag, int32_t *status, int nthreads);

#define K 16

static void *take(FILE *f, size_t count, size_t size) {
    void *p = malloc(count * size);                   /* exactly what the scene has: a read past an array is the sanitizer's to find */
    if ((!p && count) || fread(p, size, count, f) != count) { fprintf(stderr, "short scene file\n"); exit(2); }
    return p;
}

static uint64_t g_sum, g_at;
static void sum(const void *p, size_t bytes) {
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < bytes; i++, g_at++) g_sum += ((uint64_t)b[i] + 1u) * (g_at * 2654435761u + 1u);
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { perror(argv[a]); return 2; }
        int32_t *hd = (int32_t *)take(f, 3, 4);
        const size_t n = (size_t)hd[0], m = (size_t)hd[1];
        const int per_agent = hd[2];
        double *pos = take(f, 3 * n, 8); float *vel = take(f, 3 * n, 4); double *heading = take(f, 3 * n, 8);
        double *radius = take(f, n, 8), *pref_speed = take(f, n, 8); uint8_t *flags = take(f, n, 1);
        double *goal = take(f, 3 * n, 8); uint8_t *policy = take(f, n, 1), *zaxis = take(f, n, 1);
        double *vpref = take(f, 3 * n, 8); uint8_t *vmode = take(f, n, 1);
        double *obs_pos = take(f, 3 * m, 8), *obs_radius = take(f, m, 8);
        double *par = take(f, 8, 8);
        orc_set_params(par[0], (int)par[1], par[2], par[3], par[4], par[5], par[6]);
        orc_set_dt_nominal(par[7]);
        double *nd = NULL, *ts = NULL, *th = NULL, *ms = NULL, *mh = NULL, *dn = NULL; int32_t *mn = NULL;
        if (per_agent) {
            nd = take(f, n, 8); mn = take(f, n, 4); ts = take(f, n, 8); th = take(f, n, 8); ms = take(f, n, 8); mh = take(f, n, 8); dn = take(f, n, 8);
        }
        orc_set_agent_params(per_agent ? (int)n : 0, nd, mn, ts, th, ms, mh, dn);
        fclose(f);
        int32_t *perm = malloc(4 * n);
        for (size_t i = 0; i < n; i++) perm[i] = (int32_t)i;
        double *action64 = malloc(8 * 7 * n); float *action32 = malloc(4 * 7 * n);
        int32_t *nbr_n = malloc(4 * n), *nbr_id = malloc(4 * K * n); uint8_t *nbr_kind = malloc(K * n);
        double *nbr_dsq = malloc(8 * K * n); uint8_t *nbr_valid = malloc(n);
        double *vused = malloc(8 * 3 * n); int32_t *diag = malloc(4 * 5 * n), *status = malloc(4 * n);
        for (size_t i = 0; i < K * n; i++) { nbr_id[i] = -1; nbr_kind[i] = 0; nbr_dsq[i] = 0.0; }      /* (rows of agents that are done stay so) */
        orc_set_list_rule(1);
        orc_policy_step((int)n, (int)m, pos, vel, heading, radius, pref_speed, flags, goal, policy, zaxis, vpref, vmode, perm, obs_pos, obs_radius,
                        action64, action32, nbr_n, nbr_id, nbr_kind, nbr_dsq, nbr_valid, vused, diag, status, 1);
        g_sum = 0; g_at = 0;
        sum(nbr_valid, n); sum(nbr_n, 4 * n); sum(nbr_id, 4 * K * n); sum(nbr_kind, K * n); sum(nbr_dsq, 8 * K * n);
        sum(action32, 4 * 7 * n); sum(diag, 4 * 5 * n); sum(status, 4 * n); sum(flags, n); sum(perm, 4 * n);
        printf("checksum %016llx\n", (unsigned long long)g_sum);
        orc_set_agent_params(0, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
        free(hd); free(pos); free(vel); free(heading); free(radius); free(pref_speed); free(flags); free(goal); free(policy); free(zaxis);
        free(vpref); free(vmode); free(obs_pos); free(obs_radius); free(par); free(nd); free(mn); free(ts); free(th); free(ms); free(mh); free(dn);
        free(perm); free(action64); free(action32); free(nbr_n); free(nbr_id); free(nbr_kind); free(nbr_dsq); free(nbr_valid); free(vused);
        free(diag); free(status);
    }
    return 0;
}
