// tr_points.h -- the per-point decision of contains_points (include/triro_points.h), host + device: the box test and
// what the two hit counts of a point say (ray_optix.py:238-267 of the reference).  Shared by k_contains_points
// (points.hip) and the host simulation (tests/host_sim/points_sim.cpp).
#pragma once
#include "tr_math.h"

// strictly inside the box on every axis (ray_optix.py:238-240: `~(~(p > lo)).any() | (~(p < hi)).any()`); a NaN
// component compares false.  lo == NULL (and hi == NULL): no box test, every point passes.
TR_HD bool tr_point_in_box(float px, float py, float pz, const float* lo, const float* hi) {
    if (!lo || !hi) return true;
    return px > lo[0] && py > lo[1] && pz > lo[2] && px < hi[0] && py < hi[1] && pz < hi[2];
}

// cp / cm = hit counts of (p, d) / (p, -d).  inside: in the box and both counts odd (ray_optix.py:265-267); broken: the
// parities do not both say "inside" and one of the rays hit nothing -- a hole in the mesh (ray_optix.py:268)
TR_HD void tr_point_decide(bool in_box, int32_t cp, int32_t cm, bool& inside, bool& broken) {
    const bool agree = (cp & 1) != 0 && (cm & 1) != 0;
    inside = in_box && agree;
    broken = !agree && (cp == 0 || cm == 0);
}
