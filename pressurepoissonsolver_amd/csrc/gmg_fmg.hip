// The full-multigrid solve te_fmg (nested iteration; see gmg_internal.hpp): right-hand sides and boundary
// vectors on every level, the exact solve on the one-patch coarsest level, then per level the quadratic FMG interpolation of the
// solution and a fixed number of cycles entered at that level. Nothing of it exists in the reference. Single rank.
#include "gmg_internal.hpp"

// te_fmg's own vectors, per level l: F = f_l + boundary terms, U (level 0: the caller's u), r, e (not on the coarsest level),
// b = the level's boundary vector (level 0: the caller's). The levels' f / u / r / t belong to the cycles that run above them.
struct FmgWs {
	std::vector<te_vec *> F, U, r, e, b;
};

namespace tei
{
void fmgFree(te_gmg *g)
{
	if (!g->fmg) return;
	for (auto *vs : {&g->fmg->F, &g->fmg->U, &g->fmg->r, &g->fmg->e, &g->fmg->b})
		for (te_vec *v : *vs)
			if (v) te_vec_destroy(v);
	delete g->fmg;
	g->fmg = nullptr;
}

static int fmgWorkspace(te_gmg *g)
{
	if (g->fmg) return TE_OK;
	const int nl = (int) g->levels.size();
	g->fmg       = new FmgWs;
	FmgWs &W     = *g->fmg;
	for (auto *vs : {&W.F, &W.U, &W.r, &W.e, &W.b}) vs->assign(nl, nullptr);
	int rc;
	for (int l = 0; l < nl; l++) {
		if ((rc = newVec(g, l, &W.F[l]))) return rc;
		if (l > 0 && ((rc = newVec(g, l, &W.U[l])) || (rc = te_vec_create_boundary(g, l, &W.b[l])))) return rc;
		if (l + 1 < nl && ((rc = newVec(g, l, &W.r[l])) || (rc = newVec(g, l, &W.e[l])))) return rc;
	}
	return TE_OK;
}
} // namespace tei

extern "C" {
int te_fmg(te_gmg *g, const te_cycle_opts *o, const te_vec *f, const te_vec *bdata, te_vec *u, int cycles, double *rel_resid)
{
	return guarded([&]() -> int {
		int rc;
		if (!g || !o) return te::fail(TE_EINVAL, "te_fmg: null solver or options");
		if ((rc = checkLevelVec(g, 0, f, "te_fmg")) || (rc = checkLevelVec(g, 0, u, "te_fmg"))) return rc;
		if (f == u) return te::fail(TE_EINVAL, "te_fmg: f and u must be different vectors");
		if (bdata && (bdata->g != g || bdata->level != 0 || !bdata->bnd)) return te::fail(TE_EINVAL, "te_fmg: bdata is not a boundary vector of level 0");
		if (cycles < 0) return te::fail(TE_EINVAL, "te_fmg: cycles must not be negative");
		if ((rc = coefRefuse(g, "te_fmg"))) return rc; // (the coarsest level's exact solve and the fold of boundary data are the Laplacian's)
		if (g->nranks > 1)
			return te::fail(TE_ESTATE, "te_fmg: not implemented on a sharded hierarchy (te_prolong_quadratic and te_boundary_restrict are single-rank); "
			                           "te_bicgstab works there");
		const int nl = (int) g->levels.size();
		if (g->levels[nl - 1]->P_global != 1)
			return te::fail(TE_ESTATE, "te_fmg: the coarsest level has " + std::to_string(g->levels[nl - 1]->P_global)
			                               + " patches (a max_levels or patches_per_proc cut-off); nested iteration starts from the exact solve of a "
			                                 "one-patch level");
		WatchdogBatch batch(g);
		if ((rc = fmgWorkspace(g))) {
			fmgFree(g);
			return rc;
		}
		FmgWs &W = *g->fmg;
		for (auto &L : g->levels) L->xf_valid_for = nullptr;
		// f_l+1 = AvgRstr f_l, b_l+1 = the restricted boundary vector; then F_l = f_l + the fold of b_l on every level (the fold
		// of a restricted right-hand side is not the coarse discretisation: -2 g / h^2 averages to -4 g / h_c^2)
		if ((rc = te_vec_copy(W.F[0], f))) return rc;
		for (int l = 0; l + 1 < nl; l++) {
			if ((rc = doRestrict(g, l, W.F[l]->d, W.F[l + 1]->d))) return rc;
			if (bdata && (rc = doBoundaryRestrict(g, l, l ? W.b[l]->d : bdata->d, W.b[l + 1]->d))) return rc;
		}
		for (int l = 0; bdata && l < nl; l++)
			if ((rc = te_add_boundary_rhs(g, l, l ? W.b[l] : bdata, W.F[l]))) return rc;
		// the exact patch solve of the coarsest level from zero: the sweep visit() runs there under exact_coarse
		te_vec *Uc = nl == 1 ? u : W.U[nl - 1];
		if ((rc = te_vec_set(Uc, 0.0)) || (rc = te_smooth(g, nl - 1, W.F[nl - 1], Uc, TE_SMOOTH_PATCH_SOLVE, o->omega, 1))) return rc;
		for (int l = nl - 2; l >= 0; l--) {
			te_vec *Ul = l ? W.U[l] : u;
			if ((rc = doProlongQuadratic(g, l, W.U[l + 1]->d, Ul->d))) return rc;
			for (int c = 0; c < cycles; c++) {
				if ((rc = te_residual(g, l, Ul, W.F[l], W.r[l])) || (rc = cycleFrom(g, o, l, W.r[l], W.e[l])) || (rc = te_vec_add(Ul, W.e[l])))
					return rc;
			}
		}
		if (rel_resid) {
			double rsq = 0, fsq = 0;
			te_vec *r0 = nl > 1 ? W.r[0] : W.U[0]; // (one level: no cycle ran, U[0] does not exist either -- a vector for the residual)
			if (!r0) {
				if ((rc = newVec(g, 0, &W.U[0]))) return rc;
				r0 = W.U[0];
			}
			if ((rc = te_residual_norm_sq(g, 0, u, W.F[0], r0, &rsq)) || (rc = te_vec_two_norm_sq(W.F[0], &fsq))) return rc;
			*rel_resid = fsq > 0 ? std::sqrt(rsq / fsq) : 0.0;
		}
		return TE_OK;
	});
}
} // extern "C"
