// From a run-time patch size / z-slab count to the template instantiation of a 3D launch: the one place that maps them, and the
// rules that choose the slab count (see gmg_ghosts3d.hpp for the grid) and the post-sweep's variant. Plain C++17, no HIP header: tests/dispatch_host.cpp
// builds it with a host compiler alone.
#pragma once
#include <cstddef>
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

// f(std::bool_constant<b>) for a run-time flag that is a template argument of the launch
template <class F> inline auto dispatchBool(bool b, F f)
{
	return b ? f(std::true_type{}) : f(std::false_type{});
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

// The slab rules as plain arithmetic (gmg_ghosts3d.hpp stencilSlabs<N> / rbgsSlabs<N> read the switches from the solver and call
// these; te_gmg_slab_count reports them). SlabSwitches::pin (TE_ZS_PIN: 0 = not set, else 1, 2, 4 or 8) overrides both rules
// whatever the patch count: the pinned count, clamped down to the largest one the patch size admits -- never a count that
// dispatchSlabs<N> would drop.
struct SlabSwitches {
	bool zs_force = false, rbgs_noslab = false, no_zs8 = false; // TE_ZS_FORCE, TE_RBGS_NOSLAB, TE_NO_ZS8
	int  pin = 0;
};

// the largest slab count a patch of size n admits: a slab is at least four planes thick, and no kernel has more than eight
inline int maxSlabs(int n) { return n >= 32 ? 8 : (n >= 16 ? 4 : (n >= 8 ? 2 : 1)); }

inline bool slabPinValid(int pin) { return pin == 1 || pin == 2 || pin == 4 || pin == 8; }

inline int pinnedSlabs(int n, int pin) { return pin < maxSlabs(n) ? pin : maxSlabs(n); }

// z-slabs per patch for the stencil kernels (and the MAC operators, the interpolators, the regrid transfer): enough workgroups to
// fill 256 CUs a few times over when the level has few patches
inline int stencilSlabCount(int n, int P, const SlabSwitches &s)
{
	if (s.pin) return pinnedSlabs(n, s.pin);
	int zs = 1;
	if (n >= 8) {
		while (zs < 4 && (s.zs_force || (size_t) P * zs < 2048) && n / (zs * 2) >= 4) zs *= 2;
		if (zs == 4 && n == 32 && P <= 64 && !s.no_zs8) zs = 8; // (see rbgsSlabCount)
	}
	return zs;
}

// z-slabs per patch for the RB-GS kernels: enough workgroups to occupy 256 CUs x 4 when the level has few patches
inline int rbgsSlabCount(int n, int count, const SlabSwitches &s)
{
	if (s.pin) return pinnedSlabs(n, s.pin);
	int zs = 1;
	while (zs < 4 && !s.rbgs_noslab && (size_t) count * zs < 1024 && n / (zs * 2) >= 4) zs *= 2;
	// very few patches (the coarsest levels of a cycle): a kernel is one patch's march, a dependent chain of plane steps of
	// ~1-2 us each that nothing hides -- eight slabs of four planes (six steps) instead of four of eight (ten steps)
	if (zs == 4 && n == 32 && count <= 64 && !s.no_zs8) zs = 8;
	return zs;
}

// Which variant V of the recomputing post-sweep (march3d.hpp k_rbgs_resweep_prolong3d<N, V, FCORR, CFP>; all bit-identical) a
// level runs. Each default was measured:
//   * exported_terms (the level's right-hand side carries ghost terms: FCORR; level 1 of 512^3): 3, ordinary loads and stores --
//     its u is the correction the finer level's post-sweep reads next (64.5 us, against 68.7 with non-temporal stores);
//   * a coarser level otherwise: 27, non-temporal loads of f and stores of u;
//   * the finest level stores u non-temporally (nobody re-reads it) and loads f non-temporally unless f can still be in the
//     Infinity Cache from the pre-sweep that read it -- up to 160 MiB: 19 (256^3, a rank's share at eight ranks; 53.4 -> 49.0 us
//     at 256^3); a larger one runs two workgroups per CU with four planes of f in flight each instead of three with two: 59
//     (450 -> 443 us at 512^3; slower at 256^3).
// refined (CFP: copy-through patches / coarse-fine ghost slots) has no 19: it runs 27. pin (TE_RESWEEP_V: 0 = not set, else 19,
// 27 or 59) replaces the default on levels without exported terms -- how a small test shape reaches the kernel of a large level.
// 0: no such kernel -- a level with exported terms is never a refined one.
constexpr size_t kResweepCacheBytes = (size_t) 160 << 20;

inline bool resweepPinValid(int pin) { return pin == 19 || pin == 27 || pin == 59; }

inline int resweepVariant(bool exported_terms, bool refined, int index, size_t level_bytes, int pin)
{
	if (exported_terms) return refined ? 0 : 3;
	const int v = pin ? pin : (index != 0 ? 27 : (level_bytes <= kResweepCacheBytes ? 19 : 59));
	return (refined && v == 19) ? 27 : v;
}
} // namespace tei
