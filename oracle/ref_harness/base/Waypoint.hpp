/*
 * Stand-in for Rock base-types' <base/Waypoint.hpp>: value carriers only, written for
 * the reference harness (oracle/ref_harness/README in DESIGN.md s3).  The planner under
 * test uses position[k] of a Waypoint / Pose2D, heading / orientation, and nothing else.
 * Everything is zero-initialised, as base-types' own constructors do.
 *
 * The real header reaches <cmath>, <algorithm>, <string>, <limits> and <iostream>
 * through Eigen; the planner's sources rely on that, so this one includes them too.
 */
#ifndef REF_HARNESS_BASE_WAYPOINT_HPP
#define REF_HARNESS_BASE_WAYPOINT_HPP

#include <math.h>
#include <stdint.h>
#include <sys/types.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <string>

namespace base
{
template <int N> struct FixedVector
{
    double v[N];
    FixedVector()
    {
        for (int k = 0; k < N; k++) v[k] = 0.0;
    }
    double& operator[](int k) { return v[k]; }
    const double& operator[](int k) const { return v[k]; }
};

typedef FixedVector<3> Position;
typedef FixedVector<2> Position2D;

struct Pose2D
{
    Position2D position;
    double orientation;
    Pose2D() : orientation(0.0) {}
};

struct Waypoint
{
    Position position;
    double heading;
    double tol_position;
    double tol_heading;
    Waypoint() : heading(0.0), tol_position(0.0), tol_heading(0.0) {}
};
}  // namespace base

#endif
