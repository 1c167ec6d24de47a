/*
 * Stand-in for Rock base-types' <base/samples/Frame.hpp> and <base/Time.hpp>: the image
 * carrier the local layer reads (four getters and the byte vector) and the wall clock of
 * its bail-outs.  Written for the reference harness; see base/Waypoint.hpp.
 */
#ifndef REF_HARNESS_BASE_SAMPLES_FRAME_HPP
#define REF_HARNESS_BASE_SAMPLES_FRAME_HPP

#include <stdint.h>

#include <chrono>
#include <vector>

namespace base
{
class Time
{
    int64_t us_;

  public:
    Time() : us_(0) {}
    static Time now()
    {
        Time t;
        t.us_ = std::chrono::duration_cast<std::chrono::microseconds>(
                    std::chrono::steady_clock::now().time_since_epoch())
                    .count();
        return t;
    }
    Time operator-(const Time& o) const
    {
        Time t;
        t.us_ = us_ - o.us_;
        return t;
    }
    double toSeconds() const { return (double)us_ / 1e6; }
};

namespace samples
{
namespace frame
{
struct Frame
{
    std::vector<uint8_t> image;
    uint16_t width, height;
    uint32_t pixel_size, row_size;
    Frame() : width(0), height(0), pixel_size(1), row_size(0) {}
    uint16_t getWidth() const { return width; }
    uint16_t getHeight() const { return height; }
    uint32_t getPixelSize() const { return pixel_size; }
    uint32_t getRowSize() const { return row_size; }
};
}  // namespace frame
}  // namespace samples
}  // namespace base

#endif
