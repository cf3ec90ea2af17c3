// Stand-alone host check of csrc/dispatch.hpp (tests/test_dispatch_host.py builds it with g++ and the sanitizers): dispatchN maps
// a run-time patch size, dispatchSlabs<N> a run-time slab count, to the integral constant the launch sites instantiate with.
#include "dispatch.hpp"
#include <cstdio>
#include <initializer_list>

namespace
{
int failures = 0;

void check(bool ok, const char *what, int a, int b)
{
	if (ok) return;
	failures++;
	std::printf("FAIL %s (%d, %d)\n", what, a, b);
}

// the slab counts a patch of size N admits: a slab is at least four planes thick
constexpr bool allowed(int N, int ZS) { return ZS == 1 || (ZS == 2 && N >= 8) || (ZS == 4 && N >= 16) || (ZS == 8 && N >= 32); }

template <int N> void checkSlabs()
{
	for (int zs : {1, 2, 4, 8}) {
		int calls = 0, got = -1;
		tei::dispatchSlabs<N>(zs, [&](auto z) {
			constexpr int ZS = decltype(z)::value;
			static_assert(allowed(N, ZS), "dispatchSlabs instantiated its functor for a slab count the patch size does not admit");
			calls++;
			got = ZS;
		});
		if (allowed(N, zs)) {
			check(calls == 1, "dispatchSlabs: exactly one call", N, zs);
			check(got == zs, "dispatchSlabs: ZS == zs", N, zs);
		} else
			check(calls == 0, "dispatchSlabs: no call for a forbidden pair", N, zs);
	}
}
} // namespace

int main()
{
	for (int n : {4, 8, 16, 32}) {
		int calls = 0;
		const int got = tei::dispatchN(n, [&](auto c) {
			calls++;
			return (int) decltype(c)::value;
		});
		check(calls == 1 && got == n, "dispatchN: the size itself", n, got);
	}
	for (int n : {64, 0, -1, 5, 33}) {
		const int got = tei::dispatchN(n, [](auto c) { return (int) decltype(c)::value; });
		check(got == 32, "dispatchN: any other size is 32", n, got);
	}
	{ // a functor without a result
		int seen = 0;
		tei::dispatchN(16, [&](auto c) { seen = decltype(c)::value; });
		check(seen == 16, "dispatchN: void functor", 16, seen);
	}
	checkSlabs<4>();
	checkSlabs<8>();
	checkSlabs<16>();
	checkSlabs<32>();
	if (failures) return 1;
	std::printf("DISPATCH_OK\n");
	return 0;
}
