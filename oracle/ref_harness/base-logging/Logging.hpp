/*
 * Stand-in for Rock's <base-logging/Logging.hpp>: every LOG_*_S stream swallows what is
 * shifted into it.  Messages carry no state, so dropping them changes no result.
 */
#ifndef REF_HARNESS_BASE_LOGGING_HPP
#define REF_HARNESS_BASE_LOGGING_HPP

namespace ref_harness
{
struct NullLog
{
    template <class T> NullLog& operator<<(const T&) { return *this; }
};
}  // namespace ref_harness

#define LOG_DEBUG_S ::ref_harness::NullLog()
#define LOG_INFO_S ::ref_harness::NullLog()
#define LOG_WARN_S ::ref_harness::NullLog()
#define LOG_ERROR_S ::ref_harness::NullLog()
#define LOG_FATAL_S ::ref_harness::NullLog()

#endif
