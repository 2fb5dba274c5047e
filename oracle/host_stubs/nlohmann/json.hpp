// TEST INFRASTRUCTURE: stand-in for <nlohmann/json.hpp>. The worker's message types declare JSON conversions that the
// stage functions never call; this lets those declarations compile and does nothing.
#pragma once
#include <initializer_list>

namespace nlohmann {
struct json {
	json() {}
	template <typename T> json(const T&) {}
	json(std::initializer_list<json>) {}
	const json& at(const char*) const { return *this; }
	template <typename T> T get() const { return T{}; }
};
}  // namespace nlohmann

#define NLOHMANN_DEFINE_TYPE_INTRUSIVE(...)
