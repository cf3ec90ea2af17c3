// From a run-time patch size / z-slab count to the template instantiation of a 3D launch: the one place that maps them (see
// gmg_ghosts3d.hpp for the slab rules and the grid). Plain C++17, no HIP header: tests/dispatch_host.cpp builds it with a host
// compiler alone.
#pragma once
#include <type_traits>

namespace tei
{
// f(std::integral_constant<int, N>) for the patch size n = 4, 8, 16; anything else is 32 (te_gmg_create admits no other size)
template <class F> inline auto dispatchN(int n, F f)
{
	switch (n) {
		case 4: return f(std::integral_constant<int, 4>{});
		case 8: return f(std::integral_constant<int, 8>{});
		case 16: return f(std::integral_constant<int, 16>{});
		default: return f(std::integral_constant<int, 32>{});
	}
}

// f(std::integral_constant<int, ZS>) for the slab count of a patch of size N: 1, 2 (N >= 8), 8 (N >= 32), anything else is 4
// (N >= 16). A slab is at least four planes thick, so a count the patch size does not admit launches nothing -- and, the guards
// being `if constexpr`, a generic lambda is never instantiated for such a pair: no kernel instantiation exists for it.
template <int N, class F> inline void dispatchSlabs(int slabs, F f)
{
	switch (slabs) {
		case 1: f(std::integral_constant<int, 1>{}); break;
		case 2:
			if constexpr (N >= 8) f(std::integral_constant<int, 2>{});
			break;
		case 8:
			if constexpr (N >= 32) f(std::integral_constant<int, 8>{});
			break;
		default:
			if constexpr (N >= 16) f(std::integral_constant<int, 4>{});
			break;
	}
}
} // namespace tei
