// TEST INFRASTRUCTURE: stand-in for <spdlog/spdlog.h>, enough for the reference's worker sources to compile
// (oracle/Makefile, target `ref-host`). Logging is dropped; the standard headers the real one brings in are kept.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <functional>
#include <limits>
#include <mutex>
#include <optional>
#include <stack>
#include <thread>
#include <unordered_map>
#include <unordered_set>

namespace spdlog {
template <typename... A> inline void info(A&&...) {}
template <typename... A> inline void warn(A&&...) {}
template <typename... A> inline void error(A&&...) {}
}  // namespace spdlog
