// 3D kernel launches: stencil (apply, residual, Jacobi, residual + restriction), red-black sweeps, restriction, prolongation (see gmg_internal.hpp).
#include "gmg_ghosts3d.hpp"

namespace tei
{
// one launch of k_stencil3d<N, MODE, ZS> with or without fused sums (RED: march3d.hpp StencilRed)
template <int N, int MODE, int ZS>
void launchStencilZS(te_gmg *g, dim3 grid, const LevelDev &D_, const double *u, const double *f, double *out, double omega,
                     const RestrictDst &rd, int redmode, const RedSrc &rs)
{
	const dim3 blk(Tile3<N>::TPB);
	const LevelDev &D = stamped(g, D_, MODE == MODE_RESID_RESTRICT ? "stencil resid+restrict" : "stencil", grid.x);
	if constexpr (MODE == MODE_APPLY) {
		if (redmode == RED_OUT_A) {
			hipLaunchKernelGGL((k_stencil3d<N, MODE, ZS, RED_OUT_A>), grid, blk, 0, g->stream, D, u, f, out, omega, rd, rs);
			return;
		}
		if (redmode == RED_OUT_A_OUT) {
			hipLaunchKernelGGL((k_stencil3d<N, MODE, ZS, RED_OUT_A_OUT>), grid, blk, 0, g->stream, D, u, f, out, omega, rd, rs);
			return;
		}
	}
	if constexpr (MODE == MODE_RESID) {
		if (redmode == RED_OUT_OUT) {
			hipLaunchKernelGGL((k_stencil3d<N, MODE, ZS, RED_OUT_OUT>), grid, blk, 0, g->stream, D, u, f, out, omega, rd, rs);
			return;
		}
	}
	hipLaunchKernelGGL((k_stencil3d<N, MODE, ZS, RED_NONE>), grid, blk, 0, g->stream, D, u, f, out, omega, rd, rs);
}

// redmode != RED_NONE: the kernel leaves one pair of partial sums per work item in g->partial (red_a: the second operand
// of the dot product); *red_items = their number (the caller runs k_reduce_final2 over them)
template <int N, int MODE> int launchStencilN(te_gmg *g, LevelHost &L, const double *u, const double *f, double *out, double omega,
                                              RestrictDst rd = RestrictDst(), const double *xf_in = nullptr, int redmode = RED_NONE,
                                              const double *red_a = nullptr, int *red_items = nullptr, bool patch_op = false)
{
	const int zs = stencilSlabs<N>(g, L.P);
	if (redmode != RED_NONE) {
		if ((size_t) 2 * L.P * zs > g->partial.n) return te::fail(TE_ESTATE, "launchStencil: partial-sum buffer too small");
		if (red_items) *red_items = L.P * zs;
	}
	auto launch = [&](LevelDev D) {
		if (D.count == 0) return;
		Timed t(g, zs > 1 ? KC_STENCIL_SLABS
		                  : (MODE == MODE_APPLY ? (redmode != RED_NONE ? KC_APPLY_DOT : KC_APPLY)
		                                        : (MODE == MODE_RESID ? KC_RESID : (MODE == MODE_JACOBI ? KC_JACOBI : KC_RESID_RESTRICT))),
		        (size_t) D.count * L.nc);
		const RedSrc rs{red_a, g->partial.p, D.first * zs}; // (interior patches are launched before the boundary patches)
		dispatchSlabs<N>(zs, [&](auto z) {
			launchStencilZS<N, MODE, decltype(z)::value>(g, slabGrid(D.count, zs), D, u, f, out, omega, rd, redmode, rs);
		});
	};
	int rc = withGhosts<N>(g, L, {u}, launch, xf_in, nullptr, patch_op);
	if (rc) return rc;
	HIPCHK(hipGetLastError());
	return TE_OK;
}

template <int MODE> int launchStencil(te_gmg *g, LevelHost &L, const double *u, const double *f, double *out, double omega,
                                      RestrictDst rd, const double *xf_in, int redmode, const double *red_a, int *red_items, bool patch_op)
{
	if (red_items) *red_items = 0;
	if (L.P == 0) return TE_OK;
	if (L.dim == 2) {
		if constexpr (MODE == MODE_RESID_RESTRICT)
			return te::fail(TE_EUNSUPPORTED, "fused residual+restrict has no 2D kernel");
		else
			return launchStencil2d<MODE>(g, L, u, f, out, omega, redmode, red_a, red_items, patch_op);
	}
	return dispatchN(L.n, [&](auto n) {
		return launchStencilN<decltype(n)::value, MODE>(g, L, u, f, out, omega, rd, xf_in, redmode, red_a, red_items, patch_op);
	});
}

template <int N, bool ZERO, bool PROLONG>
void launchRbgsKernel(te_gmg *g, const LevelDev &D_, const double *u, const double *f, double *out, const ProlongSrc &ps)
{
	const int  zs = rbgsSlabs<N>(g, D_.count);
	const dim3 grid = slabGrid(D_.count, zs), blk(Tile3<N>::TPB);
	const LevelDev &D = stamped(g, D_, ZERO ? "rbgs from zero" : (PROLONG ? "rbgs on u + P e" : "rbgs"), grid.x);
	dispatchSlabs<N>(zs, [&](auto z) {
		hipLaunchKernelGGL((k_rbgs3d<N, ZERO, PROLONG, decltype(z)::value>), grid, blk, 0, g->stream, D, u, f, out, ps);
	});
}

template <int N> int launchRbgsN(te_gmg *g, LevelHost &L, const double *u, const double *f, double *out, bool zero_guess,
                                 const double *prolong_from, const double *xf_in, double *xf_out)
{
	if (prolong_from) { // u + P(coarse) is formed on the fly: only for levels without coarse/fine faces (checked by the caller)
		ProlongSrc ps = prolongSrc(L, prolong_from);
		ps.cbase      = L.cbase.p; // (null unless every patch is an octant child of a local parent)
		const bool cfp = (L.ncf > 0 || L.has_copy); // refined level: copy-through patches / coarse-fine ghost slots
		if (!cfp && !ps.cbase) return te::fail(TE_ESTATE, "launchRbgs: fused prolongation on a level without its coarse-base table");
		auto launch = [&](LevelDev D) {
			if (D.count == 0) return;
			if (cfp) {
				Timed t(g, KC_RBGS_PROLONG, (size_t) D.count * L.nc);
				hipLaunchKernelGGL((k_rbgs3d<N, false, true, 1, true>), slabGrid(D.count), dim3(Tile3<N>::TPB), 0, g->stream, D, u, f, out, ps);
				return;
			}
			Timed t(g, rbgsSlabs<N>(g, D.count) > 1 ? KC_RBGS_SLABS : KC_RBGS_PROLONG, (size_t) D.count * L.nc);
			launchRbgsKernel<N, false, true>(g, D, u, f, out, ps);
		};
		// neighbours on other ranks receive this rank's face layers of u + P(coarse) (exchange under the interior)
		int rc = withGhosts<N>(g, L, {u, nullptr, &ps}, launch, xf_in, xf_out);
		if (rc) return rc;
		HIPCHK(hipGetLastError());
		return TE_OK;
	}
	if (zero_guess) { // a zero iterate has zero ghosts everywhere: nothing to exchange or build
		Timed    t(g, rbgsSlabs<N>(g, L.P) > 1 ? KC_RBGS_SLABS : KC_RBGS_ZERO, (size_t) L.P * L.nc);
		LevelDev D = L.dev();
		D.xf_out   = xf_out;
		launchRbgsKernel<N, true, false>(g, D, u, f, out, ProlongSrc());
		HIPCHK(hipGetLastError());
		return TE_OK;
	}
	auto launch = [&](LevelDev D) {
		if (D.count == 0) return;
		Timed t(g, rbgsSlabs<N>(g, D.count) > 1 ? KC_RBGS_SLABS : KC_RBGS, (size_t) D.count * L.nc);
		launchRbgsKernel<N, false, false>(g, D, u, f, out, ProlongSrc());
	};
	int rc = withGhosts<N>(g, L, {u}, launch, xf_in, xf_out);
	if (rc) return rc;
	HIPCHK(hipGetLastError());
	return TE_OK;
}

int launchRbgs(te_gmg *g, LevelHost &L, const double *u, const double *f, double *out, bool zero_guess, const double *prolong_from,
               const double *xf_in, double *xf_out)
{
	if (L.P == 0) return TE_OK;
	if (L.dim == 2) return launchRbgs2d(g, L, u, f, out, zero_guess, prolong_from);
	return dispatchN(L.n, [&](auto n) { return launchRbgsN<decltype(n)::value>(g, L, u, f, out, zero_guess, prolong_from, xf_in, xf_out); });
}

// Cycle.h:59-65 in one pass: coarse f = AvgRstr(f - A u), r never stored. Children whose parent is
// on another rank write their block into upbuf; received blocks are placed by k_restrict_unpack3d.
template <int N> int residRestrictN(te_gmg *g, LevelHost &L, const double *u, const double *f, double *coarse, const double *xf_in)
{
	int rc = TE_OK;
	if (L.P > 0) rc = launchStencilN<N, MODE_RESID_RESTRICT>(g, L, u, f, L.r->d, 0.0, restrictDst(L, coarse), xf_in);
	if (rc) return rc;
	if ((rc = shipRestricted<N>(g, L, coarse))) return rc;
	HIPCHK(hipGetLastError());
	return TE_OK;
}

int residRestrict(te_gmg *g, LevelHost &L, const double *u, const double *f, double *coarse, const double *xf_in)
{
	if (L.dim == 2) return residRestrict2d(g, L, u, f, coarse);
	return dispatchN(L.n, [&](auto n) { return residRestrictN<decltype(n)::value>(g, L, u, f, coarse, xf_in); });
}

template <int N> int restrictN(te_gmg *g, LevelHost &L, const double *fine, double *coarse)
{
	if (L.n_up > 0) {
		Timed t(g, KC_PACK, (size_t) L.n_up * L.nc / 8);
		hipLaunchKernelGGL(k_restrict_pack3d<N>, dim3(L.n_up), dim3(256), 0, g->stream, L.up_desc.p, L.up_off.p, fine,
		                   L.upbuf.p);
	}
	int rc = doExchange(g, 2, L.tx_up, L.upbuf.p, L.downbuf.p);
	if (rc) return rc;
	if (L.Pc == 0) return TE_OK;
	Timed t(g, KC_RESTRICT, (size_t) L.P * L.nc);
	hipLaunchKernelGGL(k_restrict3d<N>, dim3(gridFor((size_t) L.Pc * L.nc, 256)), dim3(256), 0, g->stream, L.Pc,
	                   L.child.p, L.copy.p, fine, L.downbuf.p, L.down_off.p, coarse);
	HIPCHK(hipGetLastError());
	return TE_OK;
}

template <int N> int prolongN(te_gmg *g, LevelHost &L, const double *coarse, double *fine)
{
	if (L.n_down > 0 && !L.repl_up) { // (repl_up: those blocks were received for the restriction; every parent is local)
		Timed t(g, KC_PACK, (size_t) L.n_down * L.nc / 8);
		hipLaunchKernelGGL(k_prolong_pack3d<N>, dim3(L.n_down), dim3(256), 0, g->stream, L.down_desc.p, L.down_off.p,
		                   coarse, L.downbuf.p);
	}
	int rc = doExchange(g, 3, L.tx_down, L.downbuf.p, L.upbuf.p);
	if (rc) return rc;
	if (L.P == 0) return TE_OK;
	Timed t(g, KC_PROLONG, (size_t) L.P * L.nc);
	hipLaunchKernelGGL(k_prolong3d<N>, dim3(gridFor((size_t) L.P * L.nc / 2, 256)), dim3(256), 0, g->stream, L.P,
	                   L.parent.p, L.orth.p, coarse, L.upbuf.p, L.up_off.p, fine);
	HIPCHK(hipGetLastError());
	return TE_OK;
}

int doRestrict(te_gmg *g, int fine_level, const double *fine, double *coarse)
{
	LevelHost &L = *g->levels[fine_level];
	if (L.dim == 2) return restrict2d(g, L, fine, coarse);
	return dispatchN(L.n, [&](auto n) { return restrictN<decltype(n)::value>(g, L, fine, coarse); });
}

int doProlong(te_gmg *g, int fine_level, const double *coarse, double *fine)
{
	LevelHost &L = *g->levels[fine_level];
	if (L.dim == 2) return prolong2d(g, L, coarse, fine);
	return dispatchN(L.n, [&](auto n) { return prolongN<decltype(n)::value>(g, L, coarse, fine); });
}

template int launchStencil<MODE_APPLY>(te_gmg *, LevelHost &, const double *, const double *, double *, double, RestrictDst, const double *, int, const double *, int *, bool);
template int launchStencil<MODE_RESID>(te_gmg *, LevelHost &, const double *, const double *, double *, double, RestrictDst, const double *, int, const double *, int *, bool);
template int launchStencil<MODE_JACOBI>(te_gmg *, LevelHost &, const double *, const double *, double *, double, RestrictDst, const double *, int, const double *, int *, bool);
} // namespace tei

