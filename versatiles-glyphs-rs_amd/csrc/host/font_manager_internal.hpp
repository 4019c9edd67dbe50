// font_manager_internal.hpp — what the translation units behind font_manager.hpp share and nobody else needs.
#pragma once
#include <chrono>

namespace vg {

inline double now_s()
{
	using namespace std::chrono;
	return duration<double>(steady_clock::now().time_since_epoch()).count();
}

} // namespace vg
