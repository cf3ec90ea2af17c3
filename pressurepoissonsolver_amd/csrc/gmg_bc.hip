// Boundary data on the device (bckernels.hpp): boundary vectors, the fold of boundary data into a right-hand side, the canned
// problems' boundary data and Init with one boundary kind per side of the domain (see gmg_internal.hpp).
#include "gmg_internal.hpp"

namespace tei
{
// the level's table of physical faces on the device, made at the first call that needs it
static int bcGeom(LevelHost &L, BcGeom *G)
{
	int rc;
	if (!L.bface.p && !L.bface_host.empty() && (rc = L.bface.upload(L.bface_host))) return rc;
	G->n = L.n, G->P = L.P;
	G->starts = L.geom_starts.p, G->h = L.geom_h.p, G->face_kind = L.face_kind.p, G->bface = L.bface.p;
	return TE_OK;
}

static int checkBoundaryVec(te_gmg *g, int level, const te_vec *v, const char *who)
{
	if (!g || !v || level < 0 || level >= (int) g->levels.size() || v->g != g || v->level != level || !v->bnd)
		return te::fail(TE_EINVAL, std::string(who) + ": not a boundary vector of this level");
	return TE_OK;
}

static const char *const kBrSharded = "te_boundary_restrict: on a sharded hierarchy the blocks of children on another rank would have to travel: not implemented";

int doBoundaryRestrict(te_gmg *g, int fine_level, const double *fine_bdata, double *coarse_bdata)
{
	if (g->nranks > 1) return te::fail(TE_ESTATE, kBrSharded);
	LevelHost &L = *g->levels[fine_level], &C = *g->levels[fine_level + 1];
	if (C.nbf == 0) return TE_OK;
	int rc;
	if (!L.brestrict.p && (rc = L.brestrict.upload(L.brestrict_host))) return rc;
	if (L.brestrict.n != (size_t) C.nbf * 5) return te::fail(TE_ESTATE, "te_boundary_restrict: the level has no restriction table");
	Timed t(g, KC_BOUNDARY_RESTRICT, (size_t) C.nbf * C.nf);
	if (L.dim == 3)
		hipLaunchKernelGGL(k_boundary_restrict<3>, dim3(C.nbf), dim3(256), 0, g->stream, L.n, C.nbf, L.brestrict.p, fine_bdata, coarse_bdata);
	else
		hipLaunchKernelGGL(k_boundary_restrict<2>, dim3(C.nbf), dim3(256), 0, g->stream, L.n, C.nbf, L.brestrict.p, fine_bdata, coarse_bdata);
	HIPCHK(hipGetLastError());
	return TE_OK;
}
} // namespace tei

extern "C" {
int te_boundary_restrict(te_gmg *g, int fine_level, const te_vec *fine_bdata, te_vec *coarse_bdata)
{
	return guarded([&]() -> int {
		int rc;
		if ((rc = checkBoundaryVec(g, fine_level, fine_bdata, "te_boundary_restrict"))
		    || (rc = checkBoundaryVec(g, fine_level + 1, coarse_bdata, "te_boundary_restrict")))
			return rc;
		return doBoundaryRestrict(g, fine_level, fine_bdata->d, coarse_bdata->d);
	});
}

int te_vec_create_boundary(te_gmg *g, int level, te_vec **out)
{
	return guarded([&]() -> int {
		if (!g || !out || level < 0 || level >= (int) g->levels.size()) return te::fail(TE_EINVAL, "te_vec_create_boundary: bad argument");
		LevelHost &L = *g->levels[level];
		HIPCHK(hipSetDevice(g->device));
		auto v   = std::make_unique<te_vec>();
		v->g     = g;
		v->level = level;
		v->bnd   = true;
		v->n     = (size_t) L.nbf * L.nf;
		HIPCHK(hipMalloc(&v->d, sizeof(double) * std::max<size_t>(v->n, 2)));
		hipError_t e = hipMemsetAsync(v->d, 0, sizeof(double) * v->n, g->stream);
		if (e != hipSuccess) {
			(void) hipFree(v->d);
			return te::fail(TE_EHIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
		}
		*out = v.release();
		return TE_OK;
	});
}

// Init.cpp:186-240 / :89-146 with the face data taken from a boundary vector: f -= 2 g / h^2 on Dirichlet faces, f +- g_n / h on
// Neumann faces, in place
int te_add_boundary_rhs(te_gmg *g, int level, const te_vec *bdata, te_vec *f)
{
	return guarded([&]() -> int {
		int rc;
		if ((rc = checkBoundaryVec(g, level, bdata, "te_add_boundary_rhs")) || (rc = checkLevelVec(g, level, f, "te_add_boundary_rhs"))) return rc;
		LevelHost &L = *g->levels[level];
		if (L.P == 0 || L.nbf == 0) return TE_OK;
		BcGeom G;
		if ((rc = bcGeom(L, &G))) return rc;
		if (L.xf_valid_for == f->d) L.xf_valid_for = nullptr; // f changes in place
		Timed      t(g, KC_VECOP, (size_t) L.nbf * L.nf);
		const dim3 grid(L.P * 2 * L.dim), blk(256);
		if (L.dim == 3)
			hipLaunchKernelGGL(k_boundary_rhs<3>, grid, blk, 0, g->stream, G, (const double *) bdata->d, f->d);
		else
			hipLaunchKernelGGL(k_boundary_rhs<2>, grid, blk, 0, g->stream, G, (const double *) bdata->d, f->d);
		HIPCHK(hipGetLastError());
		return TE_OK;
	});
}

int te_boundary_sample(te_gmg *g, int level, int problem, te_vec *bdata)
{
	return guarded([&]() -> int {
		int rc;
		if ((rc = checkBoundaryVec(g, level, bdata, "te_boundary_sample"))) return rc;
		if (problem != PROBLEM_TRIG && problem != PROBLEM_GAUSS) return te::fail(TE_EINVAL, "te_boundary_sample: unknown problem (TE_PROBLEM_TRIG or TE_PROBLEM_GAUSS)");
		LevelHost &L = *g->levels[level];
		if (L.P == 0 || L.nbf == 0) return TE_OK;
		BcGeom G;
		if ((rc = bcGeom(L, &G))) return rc;
		Timed      t(g, KC_VECOP, bdata->n);
		const dim3 grid(L.P * 2 * L.dim), blk(256);
		if (L.dim == 3 && problem == PROBLEM_TRIG)
			hipLaunchKernelGGL((k_boundary_sample<3, PROBLEM_TRIG>), grid, blk, 0, g->stream, G, bdata->d);
		else if (L.dim == 3)
			hipLaunchKernelGGL((k_boundary_sample<3, PROBLEM_GAUSS>), grid, blk, 0, g->stream, G, bdata->d);
		else if (problem == PROBLEM_TRIG)
			hipLaunchKernelGGL((k_boundary_sample<2, PROBLEM_TRIG>), grid, blk, 0, g->stream, G, bdata->d);
		else
			hipLaunchKernelGGL((k_boundary_sample<2, PROBLEM_GAUSS>), grid, blk, 0, g->stream, G, bdata->d);
		HIPCHK(hipGetLastError());
		return TE_OK;
	});
}

// te_init_problem with the kind of every physical face read from the level's face_kind (the hierarchy's neumann_sides)
int te_init_problem_sides(te_gmg *g, int level, int problem, te_vec *f, te_vec *exact)
{
	return guarded([&]() -> int {
		int rc;
		if ((rc = checkLevelVec(g, level, f, "te_init_problem_sides"))) return rc;
		if (exact && (rc = checkLevelVec(g, level, exact, "te_init_problem_sides"))) return rc;
		if (exact == f) return te::fail(TE_EINVAL, "te_init_problem_sides: f and exact must be different vectors");
		if (problem == PROBLEM_RANDOM) return te_init_problem(g, level, problem, 0, f, exact); // (no boundary data in it)
		if (problem != PROBLEM_TRIG && problem != PROBLEM_GAUSS) return te::fail(TE_EINVAL, "te_init_problem_sides: unknown problem");
		LevelHost &L = *g->levels[level];
		if (L.xf_valid_for == f->d || (exact && L.xf_valid_for == exact->d)) L.xf_valid_for = nullptr;
		if (L.P == 0) return TE_OK;
		InitGeom G;
		G.dim = L.dim, G.n = L.n, G.P = L.P;
		G.starts = L.geom_starts.p, G.h = L.geom_h.p, G.face_kind = L.face_kind.p, G.ids = L.node_ids.p;
		const dim3 grid(gridFor(f->n, 256, 1 << 20)), blk(256);
		double    *e = exact ? exact->d : nullptr;
		Timed      t(g, KC_VECOP, f->n);
		if (L.dim == 3 && problem == PROBLEM_TRIG)
			hipLaunchKernelGGL((k_init3d<PROBLEM_TRIG, INIT_SIDES>), grid, blk, 0, g->stream, G, f->d, e);
		else if (L.dim == 3)
			hipLaunchKernelGGL((k_init3d<PROBLEM_GAUSS, INIT_SIDES>), grid, blk, 0, g->stream, G, f->d, e);
		else if (problem == PROBLEM_TRIG)
			hipLaunchKernelGGL((k_init2d<PROBLEM_TRIG, INIT_SIDES>), grid, blk, 0, g->stream, G, f->d, e);
		else
			hipLaunchKernelGGL((k_init2d<PROBLEM_GAUSS, INIT_SIDES>), grid, blk, 0, g->stream, G, f->d, e);
		HIPCHK(hipGetLastError());
		return TE_OK;
	});
}
} // extern "C"
