// Transport of a cell field by a face velocity on the device (advectkernels.hpp): the donor-cell flux
// (te_advect_flux), the update c - alpha div(U c_upwind) in one pass (te_advect), the matching of a face vector across coarse/fine
// faces (te_faces_match) and the largest |U_a| / h_a (te_faces_max_rate). All four are additive and single rank: none reads or changes
// the solver's coefficient, reaction term, interpolator or options. te_advect_flux and te_advect fill the level's coarse/fine ghost
// slots themselves (with fluxes, no exchange); the next te_apply refills the slots from its own iterate, as every operator call does.
#include "gmg_ghosts3d.hpp"
#include "advectkernels.hpp" // (last: FMA contraction is off from there on)

namespace tei
{
static int checkKindA(te_gmg *g, int level, const te_vec *v, bool faces, bool bnd, const char *who, const char *what)
{
	if (!g || !v || level < 0 || level >= (int) g->levels.size() || v->g != g || v->level != level || v->faces != faces || v->bnd != bnd || v->iface)
		return te::fail(TE_EINVAL, std::string(who) + ": " + what + " of this level expected");
	return TE_OK;
}
static int refuseShardedAdvect(const te_gmg *g, const char *who)
{
	if (g->nranks > 1) return te::fail(TE_ESTATE, std::string(who) + ": not implemented on a sharded hierarchy (single rank only)");
	return TE_OK;
}

// h, and the boundary vector with the level's table of physical faces where one is given
static int advectGeom(LevelHost &L, const te_vec *bvec, FaceGeom *F)
{
	int rc;
	F->h = L.geom_h.p, F->bface = nullptr, F->bdata = nullptr;
	if (!bvec || L.nbf == 0) return TE_OK;
	if (!L.bface.p && !L.bface_host.empty() && (rc = L.bface.upload(L.bface_host))) return rc;
	F->bface = L.bface.p, F->bdata = bvec->d;
	return TE_OK;
}

template <int N, bool FUSED> static int advectN(te_gmg *g, LevelHost &L, const FaceGeom &F, const double *c, const double *U, double *out, double alpha)
{
	L.ghost_has_v = false; // the slots hold fluxes from here on
	if (L.ncf > 0) {
		Timed t(g, KC_CFGHOST, (size_t) L.ncf * L.nf);
		hipLaunchKernelGGL(k_cf_flux3d<N>, dim3(L.ncf), dim3(N * N < 256 ? N * N : 256), 0, g->stream, L.cf_desc.p, L.cf_slots.p, U, c, L.ghostCur());
	}
	const int zs = stencilSlabs<N>(g, L.P);
	Timed     t(g, FUSED ? KC_ADVECT : KC_ADVECT_FLUX, (size_t) L.P * L.nc);
	dispatchSlabs<N>(zs, [&](auto z) {
		if constexpr (FUSED)
			hipLaunchKernelGGL((k_advect3d<N, decltype(z)::value>), slabGrid(L.P, zs), dim3(Tile3<N>::TPB), 0, g->stream, L.dev(), F, c, U, out, alpha);
		else
			hipLaunchKernelGGL((k_advflux3d<N, decltype(z)::value>), slabGrid(L.P, zs), dim3(Tile3<N>::TPB), 0, g->stream, L.dev(), F, c, U, out);
	});
	HIPCHK(hipGetLastError());
	return TE_OK;
}

// the checks and the launches te_advect_flux (FUSED = false: out = F) and te_advect share
template <bool FUSED> static int advect(te_gmg *g, int level, double alpha, const te_vec *U, const te_vec *c, const te_vec *cb, te_vec *out, const char *who)
{
	int rc;
	if ((rc = checkKindA(g, level, U, true, false, who, "U: a face vector")) || (rc = checkKindA(g, level, c, false, false, who, "c: a domain vector"))
	    || (cb && (rc = checkKindA(g, level, cb, false, true, who, "cb: a boundary vector")))
	    || (rc = FUSED ? checkKindA(g, level, out, false, false, who, "out: a domain vector") : checkKindA(g, level, out, true, false, who, "F: a face vector")))
		return rc;
	if (FUSED && (out == c || out->d == c->d)) return te::fail(TE_EINVAL, std::string(who) + ": out and c must be different vectors");
	if (!FUSED && (out == U || out->d == U->d)) return te::fail(TE_EINVAL, std::string(who) + ": F and U must be different vectors");
	if ((rc = refuseShardedAdvect(g, who))) return rc;
	LevelHost &L = *g->levels[level];
	if (L.P == 0) return TE_OK;
	FaceGeom G;
	if ((rc = advectGeom(L, cb, &G))) return rc;
	if (FUSED && L.xf_valid_for == out->d) L.xf_valid_for = nullptr; // out changes
	if (L.dim == 2) {
		L.ghost_has_v = false;
		if (L.ncf > 0) {
			Timed t(g, KC_CFGHOST, (size_t) L.ncf * L.nf);
			hipLaunchKernelGGL(k_cf_flux2d, dim3(L.ncf), dim3(64), 0, g->stream, L.n, L.cf_desc.p, L.cf_slots.p, (const double *) U->d,
			                   (const double *) c->d, L.ghostCur());
		}
		Timed t(g, FUSED ? KC_ADVECT : KC_ADVECT_FLUX, (size_t) L.P * L.nc);
		hipLaunchKernelGGL(k_advect2d<FUSED>, dim3(gridFor((size_t) L.P * L.nc / 2, 256, 65536)), dim3(256), 0, g->stream, L.dev2(), G,
		                   (const double *) c->d, (const double *) U->d, out->d, alpha);
		HIPCHK(hipGetLastError());
		return TE_OK;
	}
	return dispatchN(L.n, [&](auto n) { return advectN<decltype(n)::value, FUSED>(g, L, G, c->d, U->d, out->d, alpha); });
}
} // namespace tei

extern "C" {
int te_advect_flux(te_gmg *g, int level, const te_vec *U, const te_vec *c, const te_vec *cb, te_vec *F)
{
	return guarded([&]() -> int { return advect<false>(g, level, 0.0, U, c, cb, F, "te_advect_flux"); });
}

int te_advect(te_gmg *g, int level, double alpha, const te_vec *U, const te_vec *c, const te_vec *cb, te_vec *out)
{
	return guarded([&]() -> int { return advect<true>(g, level, alpha, U, c, cb, out, "te_advect"); });
}

int te_faces_match(te_gmg *g, int level, te_vec *F)
{
	return guarded([&]() -> int {
		const char *who = "te_faces_match";
		int         rc;
		if ((rc = checkKindA(g, level, F, true, false, who, "F: a face vector")) || (rc = refuseShardedAdvect(g, who))) return rc;
		LevelHost &L = *g->levels[level];
		if (L.P == 0 || L.ncf == 0) return TE_OK;
		Timed t(g, KC_FACES_MATCH, (size_t) L.ncf * L.nf);
		if (L.dim == 2)
			hipLaunchKernelGGL(k_faces_match2d, dim3(L.ncf), dim3(64), 0, g->stream, L.n, L.cf_desc.p, F->d);
		else
			dispatchN(L.n, [&](auto n) {
				constexpr int N = decltype(n)::value;
				hipLaunchKernelGGL(k_faces_match3d<N>, dim3(L.ncf), dim3(N * N < 256 ? N * N : 256), 0, g->stream, L.cf_desc.p, F->d);
			});
		HIPCHK(hipGetLastError());
		return TE_OK;
	});
}

int te_faces_max_rate(te_gmg *g, int level, const te_vec *U, double *rate)
{
	return guarded([&]() -> int {
		const char *who = "te_faces_max_rate";
		int         rc;
		if (!rate) return te::fail(TE_EINVAL, std::string(who) + ": rate is NULL");
		if ((rc = checkKindA(g, level, U, true, false, who, "U: a face vector")) || (rc = refuseShardedAdvect(g, who))) return rc;
		LevelHost &L = *g->levels[level];
		*rate        = 0.0;
		if (L.P == 0) return TE_OK;
		const int blocks = gridFor(U->n, 256, g->red_blocks);
		{
			Timed t(g, KC_FACES_RATE, U->n);
			hipLaunchKernelGGL(k_faces_rate, dim3(blocks), dim3(256), 0, g->stream, U->n, (int) (L.dim * L.nc + L.dim * L.nf), (int) (L.dim * L.nc),
			                   (int) L.nc, (int) L.nf, (const double *) U->d, (const double *) L.geom_h.p, g->partial.p);
			hipLaunchKernelGGL(k_reduce_final<RED_MAXABS>, dim3(1), dim3(256), 0, g->stream, blocks, g->partial.p, g->result.p);
		}
		HIPCHK(hipGetLastError());
		if ((rc = finishReduce(g, 1, 1, false))) return rc;
		*rate = g->result_host[0];
		return TE_OK;
	});
}
} // extern "C"
