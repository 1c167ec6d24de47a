// path_simplify.h -- the one simplification rule of the arriving descent
// (arrive_kernels.hip's simplified instantiations and planner.cpp's descendArriving;
// DyMuPathPlanner::getSimplifiedPaths).  include/dymu_fim.h states the
// rule and its guarantee with dymu_arrive_simplified_device.
//
// A streaming opening-window simplifier: O(1) state per path, one pass, no waypoint kept
// back but the previous one.  From the anchor A (the last kept waypoint) it holds the cone
// of directions in which a ray from A passes within eps of every waypoint seen since, and
// far2, the squared distance of the last of them.  A waypoint outside the cone, or nearer
// to A than its predecessor, ends the window: the predecessor is kept and becomes A.
//
// Only + - * and sqrt, every expression in one fixed order, and the files that include
// this header are built with -ffp-contract=off: the host threads, the kernel and the
// plain-Python restatement (tests/simplify_ref.py) keep the same waypoints.  A change here
// must be made there too.  Everything is inline and takes values: in the kernel the state
// stays in registers.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DYMU_SIMPLIFY_FN __host__ __device__ __forceinline__
#else
#define DYMU_SIMPLIFY_FN inline
#endif

namespace dymu {

struct PathSimplifier {
  double ax = 0, ay = 0;                  // the anchor
  double lx = 0, ly = 0, hx = 0, hy = 0;  // the cone from l (lower) round to h (upper)
  double far2 = 0;                        // |P - A|^2 of the last admitted waypoint
  bool open = true;                       // no constraint yet: l and h are unset

  DYMU_SIMPLIFY_FN static double cross(double ux, double uy, double vx, double vy) {
    return ux * vy - uy * vx;
  }

  // (x, y) is kept and becomes the anchor
  DYMU_SIMPLIFY_FN void anchor(double x, double y) {
    ax = x;
    ay = y;
    open = true;
    far2 = 0;
  }

  // steps 1, 2 and 4: whether P = (x, y) is admissible from the anchor; if so the cone
  // takes it in.  eps2 = eps * eps.
  DYMU_SIMPLIFY_FN bool admit(double x, double y, double eps, double eps2) {
    const double vx = x - ax, vy = y - ay;
    const double d2 = vx * vx + vy * vy;
    if (!(d2 >= far2)) return false;
    if (!open && !(cross(lx, ly, vx, vy) >= 0 && cross(vx, vy, hx, hy) >= 0)) return false;
    far2 = d2;
    if (d2 > eps2) {
      const double c = std::sqrt(d2 - eps2);
      const double tlx = vx * c + vy * eps, tly = vy * c - vx * eps;
      const double thx = vx * c - vy * eps, thy = vy * c + vx * eps;
      if (open) {
        lx = tlx, ly = tly, hx = thx, hy = thy;
        open = false;
      } else {
        if (cross(lx, ly, tlx, tly) > 0) lx = tlx, ly = tly;
        if (cross(thx, thy, hx, hy) > 0) hx = thx, hy = thy;
      }
    }
    return true;
  }

  // One further waypoint P = (x, y) whose predecessor is (px, py).  True: the predecessor
  // is kept (step 3: it is the anchor now, and P, the first waypoint after an anchor, was
  // admitted against it).
  DYMU_SIMPLIFY_FN bool next(double px, double py, double x, double y, double eps, double eps2) {
    if (admit(x, y, eps, eps2)) return false;
    anchor(px, py);
    (void)admit(x, y, eps, eps2);
    return true;
  }
};

}  // namespace dymu
