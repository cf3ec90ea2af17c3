// Second-order limited (MUSCL) transport of a cell field on the device (musclkernels.hpp): the limited slopes
// of a cell field (te_cell_slopes), the flux from edge states (te_advect_flux_muscl) and the update in one pass (te_advect_muscl).
// All three are additive and single rank: none reads or changes the solver's coefficient, reaction term, interpolator or options.
// They fill the level's coarse/fine ghost slots themselves (raw cells for the slopes, then fluxes; no exchange); the next te_apply
// refills the slots from its own iterate, as every operator call does.
#include "gmg_ghosts3d.hpp"
#include "musclkernels.hpp" // (last: FMA contraction is off from there on)

namespace tei
{
static int checkKindM(te_gmg *g, int level, const te_vec *v, bool faces, bool bnd, const char *who, const char *what)
{
	if (!g || !v || level < 0 || level >= (int) g->levels.size() || v->g != g || v->level != level || v->faces != faces || v->bnd != bnd || v->iface)
		return te::fail(TE_EINVAL, std::string(who) + ": " + what + " of this level expected");
	return TE_OK;
}
static int checkSlopeKind(int kind, const char *who)
{
	if (kind != SLOPE_ZERO && kind != SLOPE_MINMOD && kind != SLOPE_MC && kind != SLOPE_CENTRAL)
		return te::fail(TE_EINVAL, std::string(who) + ": unknown kind (TE_SLOPE_ZERO, TE_SLOPE_MINMOD, TE_SLOPE_MC or TE_SLOPE_CENTRAL)");
	return TE_OK;
}
static int refuseShardedMuscl(const te_gmg *g, const char *who)
{
	if (g->nranks > 1) return te::fail(TE_ESTATE, std::string(who) + ": not implemented on a sharded hierarchy (single rank only)");
	return TE_OK;
}

// h, and the boundary vector with the level's table of physical faces where one is given
static int musclGeom(LevelHost &L, const te_vec *bvec, FaceGeom *F)
{
	int rc;
	F->h = L.geom_h.p, F->bface = nullptr, F->bdata = nullptr;
	if (!bvec || L.nbf == 0) return TE_OK;
	if (!L.bface.p && !L.bface_host.empty() && (rc = L.bface.upload(L.bface_host))) return rc;
	F->bface = L.bface.p, F->bdata = bvec->d;
	return TE_OK;
}

// the raw ghost fill where the level has coarse/fine faces, then one pass that reads c once and writes all slopes
static int slopesLaunch(te_gmg *g, LevelHost &L, const FaceGeom &G, int kind, const double *c, double *sx, double *sy, double *sz)
{
	L.ghost_has_v = false; // the slots hold cells of c from here on
	for (double *s : {sx, sy, sz})
		if (s && L.xf_valid_for == s) L.xf_valid_for = nullptr; // s changes
	if (L.dim == 2) {
		if (L.ncf > 0) {
			Timed t(g, KC_CFGHOST, (size_t) L.ncf * L.nf);
			hipLaunchKernelGGL(k_cf_raw2d, dim3(L.ncf), dim3(64), 0, g->stream, L.n, L.cf_desc.p, L.cf_slots.p, c, L.ghostCur());
		}
		Timed t(g, KC_CELL_SLOPES, (size_t) L.P * L.nc);
		hipLaunchKernelGGL(k_slopes2d, dim3(gridFor((size_t) L.P * L.nc / 2, 256, 65536)), dim3(256), 0, g->stream, L.dev2(), G, c, sx, sy, kind);
		HIPCHK(hipGetLastError());
		return TE_OK;
	}
	return dispatchN(L.n, [&](auto n) {
		constexpr int N = decltype(n)::value;
		if (L.ncf > 0) {
			Timed t(g, KC_CFGHOST, (size_t) L.ncf * L.nf);
			hipLaunchKernelGGL(k_cf_raw3d<N>, dim3(L.ncf), dim3(N * N < 256 ? N * N : 256), 0, g->stream, L.cf_desc.p, L.cf_slots.p, c, L.ghostCur());
		}
		const int zs = stencilSlabs<N>(g, L.P);
		Timed     t(g, KC_CELL_SLOPES, (size_t) L.P * L.nc);
		dispatchSlabs<N>(zs, [&](auto z) {
			hipLaunchKernelGGL((k_slopes3d<N, decltype(z)::value>), slabGrid(L.P, zs), dim3(Tile3<N>::TPB), 0, g->stream, L.dev(), G, c, sx, sy, sz, kind);
		});
		HIPCHK(hipGetLastError());
		return TE_OK;
	});
}

// the flux ghost fill where the level has coarse/fine faces, then the march
template <bool FUSED>
static int marchLaunch(te_gmg *g, LevelHost &L, const FaceGeom &G, const double *U, const double *c, const double *sx, const double *sy,
                       const double *sz, double *out, double alpha)
{
	L.ghost_has_v = false; // the slots hold fluxes from here on
	if (L.dim == 2) {
		if (L.ncf > 0) {
			Timed t(g, KC_CFGHOST, (size_t) L.ncf * L.nf);
			hipLaunchKernelGGL(k_cf_flux_muscl2d, dim3(L.ncf), dim3(64), 0, g->stream, L.n, L.cf_desc.p, L.cf_slots.p, U, c, sx, sy, L.ghostCur());
		}
		Timed t(g, FUSED ? KC_ADVECT_MUSCL : KC_ADVECT_FLUX_MUSCL, (size_t) L.P * L.nc);
		hipLaunchKernelGGL(k_advect_muscl2d<FUSED>, dim3(gridFor((size_t) L.P * L.nc / 2, 256, 65536)), dim3(256), 0, g->stream, L.dev2(), G, c, U,
		                   sx, sy, out, alpha);
		HIPCHK(hipGetLastError());
		return TE_OK;
	}
	return dispatchN(L.n, [&](auto n) {
		constexpr int N = decltype(n)::value;
		if (L.ncf > 0) {
			Timed t(g, KC_CFGHOST, (size_t) L.ncf * L.nf);
			hipLaunchKernelGGL(k_cf_flux_muscl3d<N>, dim3(L.ncf), dim3(N * N < 256 ? N * N : 256), 0, g->stream, L.cf_desc.p, L.cf_slots.p, U, c, sx,
			                   sy, sz, L.ghostCur());
		}
		const int zs = stencilSlabs<N>(g, L.P);
		Timed     t(g, FUSED ? KC_ADVECT_MUSCL : KC_ADVECT_FLUX_MUSCL, (size_t) L.P * L.nc);
		dispatchSlabs<N>(zs, [&](auto z) {
			if constexpr (FUSED)
				hipLaunchKernelGGL((k_advect_muscl3d<N, decltype(z)::value>), slabGrid(L.P, zs), dim3(Tile3<N>::TPB), 0, g->stream, L.dev(), G, c, U, sx,
				                   sy, sz, out, alpha);
			else
				hipLaunchKernelGGL((k_advflux_muscl3d<N, decltype(z)::value>), slabGrid(L.P, zs), dim3(Tile3<N>::TPB), 0, g->stream, L.dev(), G, c, U, sx,
				                   sy, sz, out);
		});
		HIPCHK(hipGetLastError());
		return TE_OK;
	});
}

// the checks and the launches te_advect_flux_muscl (FUSED = false: out = F) and te_advect_muscl share
template <bool FUSED>
static int advectMuscl(te_gmg *g, int level, double alpha, int kind, const te_vec *U, const te_vec *c, const te_vec *cb, te_vec *out, const char *who)
{
	int rc;
	if ((rc = checkKindM(g, level, U, true, false, who, "U: a face vector")) || (rc = checkKindM(g, level, c, false, false, who, "c: a domain vector"))
	    || (cb && (rc = checkKindM(g, level, cb, false, true, who, "cb: a boundary vector")))
	    || (rc = FUSED ? checkKindM(g, level, out, false, false, who, "out: a domain vector") : checkKindM(g, level, out, true, false, who, "F: a face vector")))
		return rc;
	if (FUSED && (out == c || out->d == c->d)) return te::fail(TE_EINVAL, std::string(who) + ": out and c must be different vectors");
	if (!FUSED && (out == U || out->d == U->d)) return te::fail(TE_EINVAL, std::string(who) + ": F and U must be different vectors");
	if ((rc = checkSlopeKind(kind, who)) || (rc = refuseShardedMuscl(g, who))) return rc;
	LevelHost &L = *g->levels[level];
	if (L.P == 0) return TE_OK;
	FaceGeom G;
	if ((rc = musclGeom(L, cb, &G))) return rc;
	for (int a = 0; a < L.dim; a++) // the level's own slope vectors, made at first use (te_gmg_release_workspace frees them)
		if (!L.muscl_s[a].p && (rc = L.muscl_s[a].alloc((size_t) L.P * L.nc))) return rc;
	if (FUSED && L.xf_valid_for == out->d) L.xf_valid_for = nullptr; // out changes
	double *sx = L.muscl_s[0].p, *sy = L.muscl_s[1].p, *sz = L.dim == 3 ? L.muscl_s[2].p : nullptr;
	if ((rc = slopesLaunch(g, L, G, kind, c->d, sx, sy, sz))) return rc;
	return marchLaunch<FUSED>(g, L, G, U->d, c->d, sx, sy, sz, out->d, alpha);
}
} // namespace tei

extern "C" {
int te_cell_slopes(te_gmg *g, int level, int kind, const te_vec *c, const te_vec *cb, te_vec *sx, te_vec *sy, te_vec *sz)
{
	return guarded([&]() -> int {
		const char *who = "te_cell_slopes";
		int         rc;
		if ((rc = checkKindM(g, level, c, false, false, who, "c: a domain vector")) || (cb && (rc = checkKindM(g, level, cb, false, true, who, "cb: a boundary vector")))
		    || (rc = checkKindM(g, level, sx, false, false, who, "sx: a domain vector")) || (rc = checkKindM(g, level, sy, false, false, who, "sy: a domain vector")))
			return rc;
		LevelHost &L = *g->levels[level];
		if (L.dim == 3 && (rc = checkKindM(g, level, sz, false, false, who, "sz: a domain vector"))) return rc;
		if (L.dim == 2 && sz) return te::fail(TE_EINVAL, std::string(who) + ": sz must be NULL on a 2D hierarchy");
		const te_vec *v[4] = {c, sx, sy, sz};
		for (int i = 0; i < 4; i++)
			for (int j = i + 1; j < 4; j++)
				if (v[i] && v[j] && (v[i] == v[j] || v[i]->d == v[j]->d)) return te::fail(TE_EINVAL, std::string(who) + ": c, sx, sy and sz must be different vectors");
		if ((rc = checkSlopeKind(kind, who)) || (rc = refuseShardedMuscl(g, who))) return rc;
		if (L.P == 0) return TE_OK;
		FaceGeom G;
		if ((rc = musclGeom(L, cb, &G))) return rc;
		return slopesLaunch(g, L, G, kind, c->d, sx->d, sy->d, sz ? sz->d : nullptr);
	});
}

int te_advect_flux_muscl(te_gmg *g, int level, int kind, const te_vec *U, const te_vec *c, const te_vec *cb, te_vec *F)
{
	return guarded([&]() -> int { return advectMuscl<false>(g, level, 0.0, kind, U, c, cb, F, "te_advect_flux_muscl"); });
}

int te_advect_muscl(te_gmg *g, int level, double alpha, int kind, const te_vec *U, const te_vec *c, const te_vec *cb, te_vec *out)
{
	return guarded([&]() -> int { return advectMuscl<true>(g, level, alpha, kind, U, c, cb, out, "te_advect_muscl"); });
}
} // extern "C"
