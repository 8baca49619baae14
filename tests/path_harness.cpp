// path_harness.cpp -- TEST-ONLY host build of the waypoint helpers of sca_amd/csrc/sca_core.h (waypoint_advance, straight_v_pref2), the
// arithmetic k_waypoint runs per agent, so that it can be checked against tests/path_rule.py on a machine without a GPU.
#include <cstdint>

#include "sca_core.h"

using namespace sca;

extern "C" {

// one get_trajectory call: pts[3 * rem] in list order, *rem and now_goal[3] (NaN x: None) updated in place
void path_advance(const double *pts, int32_t *rem, double *now_goal, const double *pos, const double *goal, double radius, int use_distance) {
    int32_t r = *rem;
    V3 g = waypoint_advance(pts, r, v3(now_goal[0], now_goal[1], now_goal[2]), v3(pos[0], pos[1], pos[2]), v3(goal[0], goal[1], goal[2]),
                            radius, use_distance != 0);
    *rem = r;
    now_goal[0] = g.x; now_goal[1] = g.y; now_goal[2] = g.z;
}

void path_vpref(const double *aim, const double *goal, const double *pos, double pref_speed, int use_distance, double *out) {
    V3 v = straight_v_pref2(v3(aim[0], aim[1], aim[2]), v3(goal[0], goal[1], goal[2]), v3(pos[0], pos[1], pos[2]), pref_speed, use_distance != 0);
    out[0] = v.x; out[1] = v.y; out[2] = v.z;
}

}  // extern "C"
