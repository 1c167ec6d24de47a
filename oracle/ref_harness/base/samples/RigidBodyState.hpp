/*
 * Stand-in for Rock base-types' <base/samples/RigidBodyState.hpp>: only `position` is
 * read (by the cost-ratio code, which the harness does not drive).
 */
#ifndef REF_HARNESS_BASE_SAMPLES_RIGIDBODYSTATE_HPP
#define REF_HARNESS_BASE_SAMPLES_RIGIDBODYSTATE_HPP

#include <base/Waypoint.hpp>

namespace base
{
namespace samples
{
struct RigidBodyState
{
    Position position;
};
}  // namespace samples
}  // namespace base

#endif
