// Stand-alone host check of csrc/dispatch.hpp (tests/test_dispatch_host.py builds it with g++ and the sanitizers): dispatchN maps
// a run-time patch size, dispatchSlabs<N> a run-time slab count, to the integral constant the launch sites instantiate with;
// stencilSlabCount / rbgsSlabCount choose that count -- for every patch size, 1 ... 5000 patches, every combination of
// TE_ZS_FORCE / TE_RBGS_NOSLAB / TE_NO_ZS8 and every TE_ZS_PIN they return a count dispatchSlabs<N> runs (never one it drops),
// the written-out table without a pin, min(pin, largest admitted) with one. resweepVariant chooses the post-sweep's kernel variant:
// a table of every default cell and every TE_RESWEEP_V.
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

// how often dispatchSlabs<N> runs its functor for `zs`, and with which ZS
template <int N> int dispatched(int zs, int &got)
{
	int calls = 0;
	got       = -1;
	tei::dispatchSlabs<N>(zs, [&](auto z) {
		calls++;
		got = decltype(z)::value;
	});
	return calls;
}

// The rules without a pin, written out as tables of thresholds (from the loops of stencilSlabCount / rbgsSlabCount as they stood
// when the rules moved into dispatch.hpp): doubling stops where count * zs reaches 2048 (stencil) or 1024 (sweep), so four slabs
// need count * 2 below that, and eight go to 32^3 patches on levels of at most 64.
int stencilTable(int n, int P, bool force, bool no_zs8)
{
	if (n == 4) return 1;
	if (n == 8) return (force || P < 2048) ? 2 : 1;
	const int zs = force ? 4 : (P < 1024 ? 4 : (P < 2048 ? 2 : 1));
	return (n == 32 && zs == 4 && P <= 64 && !no_zs8) ? 8 : zs;
}

int sweepTable(int n, int count, bool noslab, bool no_zs8)
{
	if (n == 4 || noslab) return 1;
	if (n == 8) return count < 1024 ? 2 : 1;
	const int zs = count < 512 ? 4 : (count < 1024 ? 2 : 1);
	return (n == 32 && zs == 4 && count <= 64 && !no_zs8) ? 8 : zs;
}

// the largest count a patch of size n admits, by the definition (a slab is at least four planes thick; at most eight slabs)
int largestAdmitted(int n)
{
	int zs = 1;
	while (zs < 8 && n / (zs * 2) >= 4) zs *= 2;
	return zs;
}

template <int N> void checkRules()
{
	check(tei::maxSlabs(N) == largestAdmitted(N), "maxSlabs: the largest admitted count", N, tei::maxSlabs(N));
	for (int sw = 0; sw < 8; sw++)
		for (int pin : {0, 1, 2, 4, 8}) {
			tei::SlabSwitches s;
			s.zs_force = sw & 1, s.rbgs_noslab = sw & 2, s.no_zs8 = sw & 4, s.pin = pin;
			for (int count = 1; count <= 5000; count++) {
				const int st = tei::stencilSlabCount(N, count, s), rb = tei::rbgsSlabCount(N, count, s);
				int       got;
				check(dispatched<N>(st, got) == 1 && got == st, "stencil rule: a count dispatchSlabs runs exactly once", N, count);
				check(dispatched<N>(rb, got) == 1 && got == rb, "sweep rule: a count dispatchSlabs runs exactly once", N, count);
				if (pin) {
					const int want = pin < largestAdmitted(N) ? pin : largestAdmitted(N);
					check(st == want, "stencil rule: min(pin, largest admitted)", N, count);
					check(rb == want, "sweep rule: min(pin, largest admitted)", N, count);
				} else {
					check(st == stencilTable(N, count, s.zs_force, s.no_zs8), "stencil rule: the table", N, count);
					check(rb == sweepTable(N, count, s.rbgs_noslab, s.no_zs8), "sweep rule: the table", N, count);
				}
			}
		}
	for (int pin = -2; pin <= 20; pin++)
		check(tei::slabPinValid(pin) == (pin == 1 || pin == 2 || pin == 4 || pin == 8), "slabPinValid", N, pin);
}

// The post-sweep's variant, written out cell by cell. A level: exported terms?, refined?, index, bytes; then what it runs
// without a pin and with TE_RESWEEP_V = 19, 27, 59. 0: no kernel (exported terms never meet a refined level).
void checkResweep()
{
	constexpr size_t MiB = (size_t) 1 << 20;
	struct Row {
		bool   exported, refined;
		int    index;
		size_t bytes;
		int    dflt, pin19, pin27, pin59;
	};
	const Row rows[] = {
	    // plain levels: the finest up to 160 MiB, above it, a coarser one of either size
	    {false, false, 0, 128 * MiB, 19, 19, 27, 59},
	    {false, false, 0, 160 * MiB, 19, 19, 27, 59},
	    {false, false, 0, 160 * MiB + 8, 59, 19, 27, 59},
	    {false, false, 0, 1024 * MiB, 59, 19, 27, 59},
	    {false, false, 1, 16 * MiB, 27, 19, 27, 59},
	    {false, false, 2, 1024 * MiB, 27, 19, 27, 59},
	    // refined levels: 59 where a plain level runs it, 27 otherwise -- also where the pin says 19
	    {false, true, 0, 1024 * MiB, 59, 27, 27, 59},
	    {false, true, 0, 128 * MiB, 27, 27, 27, 59},
	    {false, true, 1, 1024 * MiB, 27, 27, 27, 59},
	    // exported terms: 3 whatever the level and the pin
	    {true, false, 1, 128 * MiB, 3, 3, 3, 3},
	    {true, false, 1, 1024 * MiB, 3, 3, 3, 3},
	    {true, false, 0, 1024 * MiB, 3, 3, 3, 3},
	    {true, true, 1, 128 * MiB, 0, 0, 0, 0},
	};
	int i = 0;
	for (const Row &r : rows) {
		check(tei::resweepVariant(r.exported, r.refined, r.index, r.bytes, 0) == r.dflt, "resweepVariant: the default", i, r.dflt);
		check(tei::resweepVariant(r.exported, r.refined, r.index, r.bytes, 19) == r.pin19, "resweepVariant: pin 19", i, r.pin19);
		check(tei::resweepVariant(r.exported, r.refined, r.index, r.bytes, 27) == r.pin27, "resweepVariant: pin 27", i, r.pin27);
		check(tei::resweepVariant(r.exported, r.refined, r.index, r.bytes, 59) == r.pin59, "resweepVariant: pin 59", i, r.pin59);
		i++;
	}
	for (int pin = -2; pin <= 70; pin++) check(tei::resweepPinValid(pin) == (pin == 19 || pin == 27 || pin == 59), "resweepPinValid", 0, pin);
	{ // dispatchBool: the flag itself, one call
		int calls = 0;
		check(tei::dispatchBool(true, [&](auto b) { return calls++, (int) decltype(b)::value; }) == 1, "dispatchBool: true", 1, calls);
		check(tei::dispatchBool(false, [&](auto b) { return calls++, (int) decltype(b)::value; }) == 0, "dispatchBool: false", 0, calls);
		check(calls == 2, "dispatchBool: exactly one call each", 2, calls);
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
	checkRules<4>();
	checkRules<8>();
	checkRules<16>();
	checkRules<32>();
	checkResweep();
	if (failures) return 1;
	std::printf("DISPATCH_OK\n");
	return 0;
}
