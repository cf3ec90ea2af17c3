// The device side of a variable-density projection step (densitykernels.hpp): face coefficients from a cell
// field (te_faces_from_cells), the weighted projection in one pass (te_project_weighted) and the fold of boundary data under a face
// weight (te_add_boundary_rhs_weighted). All three are additive: none reads or changes the coefficient of te_gmg_set_coefficient.
// te_faces_from_cells fills the level's coarse/fine ghost slots itself (raw cells, no exchange: single rank); te_project_weighted
// makes the level's ghosts current exactly as te_project does (withGhosts / prepareGhosts2d: collective on a sharded hierarchy, the
// launch runs per interior / boundary subset and reads w and U of its own patches only). Either way the next te_apply refills
// the slots from its own iterate, as every operator call does.
#include "gmg_ghosts3d.hpp"
#include "densitykernels.hpp"

namespace tei
{
static int checkKind(te_gmg *g, int level, const te_vec *v, bool faces, bool bnd, const char *who, const char *what)
{
	if (!g || !v || level < 0 || level >= (int) g->levels.size() || v->g != g || v->level != level || v->faces != faces || v->bnd != bnd || v->iface)
		return te::fail(TE_EINVAL, std::string(who) + ": " + what + " of this level expected");
	return TE_OK;
}
static int refuseShardedDensity(const te_gmg *g, const char *who)
{
	if (g->nranks > 1) return te::fail(TE_ESTATE, std::string(who) + ": not implemented on a sharded hierarchy (single rank only)");
	return TE_OK;
}

// h, and the boundary vector with the level's table of physical faces where one is given
static int densityGeom(LevelHost &L, const te_vec *bvec, FaceGeom *F)
{
	int rc;
	F->h = L.geom_h.p, F->bface = nullptr, F->bdata = nullptr;
	if (!bvec || L.nbf == 0) return TE_OK;
	if (!L.bface.p && !L.bface_host.empty() && (rc = L.bface.upload(L.bface_host))) return rc;
	F->bface = L.bface.p, F->bdata = bvec->d;
	return TE_OK;
}

template <int N> static int cellFaceN(te_gmg *g, LevelHost &L, const FaceGeom &F, const double *c, double *out, int mode)
{
	L.ghost_has_v = false; // the slots hold cells of c from here on
	if (L.ncf > 0) {
		Timed t(g, KC_CFGHOST, (size_t) L.ncf * L.nf);
		hipLaunchKernelGGL(k_cf_raw3d<N>, dim3(L.ncf), dim3(N * N < 256 ? N * N : 256), 0, g->stream, L.cf_desc.p, L.cf_slots.p, c, L.ghostCur());
	}
	const int zs = stencilSlabs<N>(g, L.P);
	Timed     t(g, KC_FACES_FROM_CELLS, (size_t) L.P * L.nc);
	dispatchSlabs<N>(zs, [&](auto z) {
		hipLaunchKernelGGL((k_cellface3d<N, decltype(z)::value>), slabGrid(L.P, zs), dim3(Tile3<N>::TPB), 0, g->stream, L.dev(), F, c, out, mode);
	});
	HIPCHK(hipGetLastError());
	return TE_OK;
}

template <int N> static int wprojectN(te_gmg *g, LevelHost &L, const FaceGeom &F, const double *p, const double *w, double *U, double alpha)
{
	const int zs     = stencilSlabs<N>(g, L.P);
	auto      launch = [&](LevelDev D) {
		if (D.count == 0) return;
		Timed t(g, KC_PROJECT_WEIGHTED, (size_t) D.count * L.nc);
		dispatchSlabs<N>(zs, [&](auto z) {
			hipLaunchKernelGGL((k_wproject3d<N, decltype(z)::value>), slabGrid(D.count, zs), dim3(Tile3<N>::TPB), 0, g->stream, D, F, p, w, U, alpha);
		});
	};
	int rc = withGhosts<N>(g, L, {p}, launch);
	if (rc) return rc;
	HIPCHK(hipGetLastError());
	return TE_OK;
}
} // namespace tei

extern "C" {
int te_faces_from_cells(te_gmg *g, int level, int mode, const te_vec *c, const te_vec *cb, te_vec *F)
{
	return guarded([&]() -> int {
		const char *who = "te_faces_from_cells";
		int         rc;
		if ((rc = checkKind(g, level, c, false, false, who, "c: a domain vector")) || (cb && (rc = checkKind(g, level, cb, false, true, who, "cb: a boundary vector")))
		    || (rc = checkKind(g, level, F, true, false, who, "F: a face vector")))
			return rc;
		if (mode != FACE_MODE_MEAN && mode != FACE_MODE_HARMONIC && mode != FACE_MODE_RECIP_MEAN)
			return te::fail(TE_EINVAL, std::string(who) + ": unknown mode (TE_FACE_MEAN, TE_FACE_HARMONIC or TE_FACE_RECIP_MEAN)");
		if ((rc = refuseShardedDensity(g, who))) return rc;
		LevelHost &L = *g->levels[level];
		if (L.P == 0) return TE_OK;
		FaceGeom G;
		if ((rc = densityGeom(L, cb, &G))) return rc;
		if (L.dim == 2) {
			if (L.ncf > 0) {
				Timed t(g, KC_CFGHOST, (size_t) L.ncf * L.nf);
				hipLaunchKernelGGL(k_cf_raw2d, dim3(L.ncf), dim3(64), 0, g->stream, L.n, L.cf_desc.p, L.cf_slots.p, (const double *) c->d, L.ghostCur());
			}
			Timed t(g, KC_FACES_FROM_CELLS, (size_t) L.P * L.nc);
			hipLaunchKernelGGL(k_cellface2d, dim3(gridFor((size_t) L.P * L.nc / 2, 256, 65536)), dim3(256), 0, g->stream, L.dev2(), G,
			                   (const double *) c->d, F->d, mode);
			HIPCHK(hipGetLastError());
			return TE_OK;
		}
		return dispatchN(L.n, [&](auto n) { return cellFaceN<decltype(n)::value>(g, L, G, c->d, F->d, mode); });
	});
}

int te_project_weighted(te_gmg *g, int level, double alpha, const te_vec *p, const te_vec *bdata, const te_vec *w, te_vec *U)
{
	return guarded([&]() -> int {
		const char *who = "te_project_weighted";
		int         rc;
		if ((rc = checkKind(g, level, p, false, false, who, "p: a domain vector"))
		    || (bdata && (rc = checkKind(g, level, bdata, false, true, who, "bdata: a boundary vector")))
		    || (rc = checkKind(g, level, w, true, false, who, "w: a face vector")) || (rc = checkKind(g, level, U, true, false, who, "U: a face vector")))
			return rc;
		if (w == U || w->d == U->d) return te::fail(TE_EINVAL, std::string(who) + ": w and U must be different vectors");
		if ((rc = shardedNeedsTransport(g, who))) return rc;
		LevelHost &L = *g->levels[level];
		if (L.P == 0) return TE_OK;
		FaceGeom G;
		if ((rc = densityGeom(L, bdata, &G))) return rc;
		if (L.dim == 2) {
			if ((rc = prepareGhosts2d(g, L, p->d))) return rc;
			Timed t(g, KC_PROJECT_WEIGHTED, (size_t) L.P * L.nc);
			hipLaunchKernelGGL(k_wproject2d, dim3(gridFor((size_t) L.P * L.nc / 2, 256, 65536)), dim3(256), 0, g->stream, L.dev2(), G,
			                   (const double *) p->d, (const double *) w->d, U->d, alpha);
			HIPCHK(hipGetLastError());
			return TE_OK;
		}
		return dispatchN(L.n, [&](auto n) { return wprojectN<decltype(n)::value>(g, L, G, p->d, w->d, U->d, alpha); });
	});
}

int te_add_boundary_rhs_weighted(te_gmg *g, int level, const te_vec *bdata, const te_vec *w, te_vec *f)
{
	return guarded([&]() -> int {
		const char *who = "te_add_boundary_rhs_weighted";
		int         rc;
		if ((rc = checkKind(g, level, bdata, false, true, who, "bdata: a boundary vector")) || (rc = checkKind(g, level, w, true, false, who, "w: a face vector"))
		    || (rc = checkKind(g, level, f, false, false, who, "f: a domain vector")))
			return rc;
		LevelHost &L = *g->levels[level];
		if (L.P == 0 || L.nbf == 0) return TE_OK;
		if (!L.bface.p && !L.bface_host.empty() && (rc = L.bface.upload(L.bface_host))) return rc;
		BcGeom G;
		G.n = L.n, G.P = L.P;
		G.starts = L.geom_starts.p, G.h = L.geom_h.p, G.face_kind = L.face_kind.p, G.bface = L.bface.p;
		if (L.xf_valid_for == f->d) L.xf_valid_for = nullptr; // f changes in place
		Timed      t(g, KC_BOUNDARY_RHS_W, (size_t) L.nbf * L.nf);
		const dim3 grid(L.P * 2 * L.dim), blk(256);
		if (L.dim == 3)
			hipLaunchKernelGGL(k_boundary_rhs_w<3>, grid, blk, 0, g->stream, G, (const double *) bdata->d, (const double *) w->d, f->d);
		else
			hipLaunchKernelGGL(k_boundary_rhs_w<2>, grid, blk, 0, g->stream, G, (const double *) bdata->d, (const double *) w->d, f->d);
		HIPCHK(hipGetLastError());
		return TE_OK;
	});
}
} // extern "C"
