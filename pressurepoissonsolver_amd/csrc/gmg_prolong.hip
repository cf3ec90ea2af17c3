// The linear interpolator (prolongkernels.hpp; see gmg_internal.hpp): its launches, te_prolong_linear_add, the solver's choice
// of interpolator (te_gmg_set_interpolator), and the quadratic FMG interpolation te_prolong_quadratic. The prolongation reads the COARSE level's ghosts, made current exactly as te_apply
// makes them (withGhosts / prepareGhosts2d). Single rank: on a sharded hierarchy the parent's ring block of a child on another
// rank would have to travel, and the bit-identity with the single-rank run would have to be shown first.
#include "gmg_ghosts3d.hpp"
#include "prolongkernels.hpp"

namespace tei
{
static const char *const kShardedWhy =
	": linear prolongation on a sharded hierarchy is not implemented (the ring of the parent's block for children on another rank, and "
	"the proof of bit-identity with the single-rank run, are missing); TE_INTERP_DIRECT works there";

template <int N> static int prolongLinearN(te_gmg *g, LevelHost &L, LevelHost &C, const double *coarse, double *fine)
{
	const int zs     = stencilSlabs<N>(g, L.P);
	auto      launch = [&](LevelDev D) {
		Timed t(g, KC_PROLONG_LINEAR, (size_t) L.P * L.nc);
		dispatchSlabs<N>(zs, [&](auto z) {
			hipLaunchKernelGGL((k_prolong_linear3d<N, decltype(z)::value>), slabGrid(L.P, zs), dim3(Tile3<N>::TPB), 0, g->stream, L.P, D, L.parent.p,
			                   L.orth.p, coarse, fine);
		});
	};
	// (one rank: the coarse level has no remote face, so withGhosts launches once, over the whole level's tables)
	int rc = withGhosts<N>(g, C, {coarse}, launch);
	if (rc) return rc;
	HIPCHK(hipGetLastError());
	return TE_OK;
}

int doProlongLinear(te_gmg *g, int fine_level, const double *coarse, double *fine)
{
	if (g->nranks > 1) return te::fail(TE_ESTATE, std::string("te_prolong_linear_add") + kShardedWhy);
	LevelHost &L = *g->levels[fine_level], &C = *g->levels[fine_level + 1];
	if (L.P == 0) return TE_OK;
	if (L.xf_valid_for == fine) L.xf_valid_for = nullptr; // fine changes in place
	if (L.dim == 2) {
		int rc = prepareGhosts2d(g, C, coarse);
		if (rc) return rc;
		Timed t(g, KC_PROLONG_LINEAR, (size_t) L.P * L.nc);
		hipLaunchKernelGGL(k_prolong_linear2d, dim3(gridFor((size_t) L.P * L.nc / 2, 256, 65536)), dim3(256), 0, g->stream, C.dev2(), L.P,
		                   L.parent.p, L.orth.p, coarse, fine);
		HIPCHK(hipGetLastError());
		return TE_OK;
	}
	return dispatchN(L.n, [&](auto n) { return prolongLinearN<decltype(n)::value>(g, L, C, coarse, fine); });
}

// ---- the quadratic FMG interpolation (te_prolong_quadratic): fine = Pi coarse
template <int N> static int prolongQuadraticN(te_gmg *g, LevelHost &L, LevelHost &C, const double *coarse, double *fine)
{
	const int zs     = stencilSlabs<N>(g, L.P);
	auto      launch = [&](LevelDev D) {
		Timed t(g, KC_PROLONG_QUADRATIC, (size_t) L.P * L.nc);
		dispatchSlabs<N>(zs, [&](auto z) {
			hipLaunchKernelGGL((k_prolong_quadratic3d<N, decltype(z)::value>), slabGrid(L.P, zs), dim3(Tile3<N>::TPB), 0, g->stream, L.P, D, L.parent.p,
			                   L.orth.p, coarse, fine);
		});
	};
	int rc = withGhosts<N>(g, C, {coarse}, launch);
	if (rc) return rc;
	HIPCHK(hipGetLastError());
	return TE_OK;
}

int doProlongQuadratic(te_gmg *g, int fine_level, const double *coarse, double *fine)
{
	if (g->nranks > 1)
		return te::fail(TE_ESTATE, "te_prolong_quadratic: not implemented on a sharded hierarchy (the ring of the parent's block for children on another rank is missing)");
	LevelHost &L = *g->levels[fine_level], &C = *g->levels[fine_level + 1];
	if (L.P == 0) return TE_OK;
	if (L.xf_valid_for == fine) L.xf_valid_for = nullptr; // fine is overwritten
	if (L.dim == 2) {
		int rc = prepareGhosts2d(g, C, coarse);
		if (rc) return rc;
		Timed t(g, KC_PROLONG_QUADRATIC, (size_t) L.P * L.nc);
		hipLaunchKernelGGL(k_prolong_quadratic2d, dim3(gridFor((size_t) L.P * L.nc / 2, 256, 65536)), dim3(256), 0, g->stream, C.dev2(), L.P,
		                   L.parent.p, L.orth.p, coarse, fine);
		HIPCHK(hipGetLastError());
		return TE_OK;
	}
	return dispatchN(L.n, [&](auto n) { return prolongQuadraticN<decltype(n)::value>(g, L, C, coarse, fine); });
}
} // namespace tei

extern "C" {
int te_prolong_quadratic(te_gmg *g, int fine_level, const te_vec *coarse, te_vec *fine)
{
	return guarded([&]() -> int {
		int rc;
		if ((rc = checkLevelVec(g, fine_level, fine, "te_prolong_quadratic"))
		    || (rc = checkLevelVec(g, fine_level + 1, coarse, "te_prolong_quadratic")))
			return rc;
		return doProlongQuadratic(g, fine_level, coarse->d, fine->d);
	});
}

int te_prolong_linear_add(te_gmg *g, int fine_level, const te_vec *coarse, te_vec *fine)
{
	return guarded([&]() -> int {
		int rc;
		if ((rc = checkLevelVec(g, fine_level, fine, "te_prolong_linear_add"))
		    || (rc = checkLevelVec(g, fine_level + 1, coarse, "te_prolong_linear_add")))
			return rc;
		return doProlongLinear(g, fine_level, coarse->d, fine->d);
	});
}

int te_gmg_set_interpolator(te_gmg *g, int kind)
{
	return guarded([&]() -> int {
		if (!g) return te::fail(TE_EINVAL, "te_gmg_set_interpolator: null solver");
		if (kind != TE_INTERP_DIRECT && kind != TE_INTERP_LINEAR) return te::fail(TE_EINVAL, "te_gmg_set_interpolator: unknown interpolator");
		if (kind == TE_INTERP_LINEAR && g->nranks > 1) return te::fail(TE_ESTATE, std::string("te_gmg_set_interpolator") + kShardedWhy);
		g->interp = kind;
		return TE_OK;
	});
}

int te_gmg_interpolator(const te_gmg *g)
{
	return guarded([&]() -> int {
		if (!g) return te::fail(TE_EINVAL, "te_gmg_interpolator: null solver");
		return g->interp;
	});
}
} // extern "C"
