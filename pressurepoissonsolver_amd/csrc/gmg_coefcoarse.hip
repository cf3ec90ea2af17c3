// The sub-patch coarse solve of the variable-coefficient path (te_gmg_set_coef_coarse): a coarsest level of one
// patch of n^D cells is the same grid as a uniform tree of (n / s)^D patches of s^D cells, and on that tree the path's own kernels and
// its own coarse levels exist. The parent solver owns an AUXILIARY solver on that tree -- an ordinary te_gmg that borrows the parent's
// stream (gmgCreate) -- and visitCoef hands its coarsest level to coefCoarseSolve: split f and u, `cycles` cycles of visitCoef on the
// auxiliary solver with the caller's options, merge u. No event and no host synchronisation inside a cycle. On a sharded hierarchy the
// auxiliary solver stays single rank and exchanges nothing: the ranks that hold the one coarsest patch (every rank where the level is
// replicated, its owner otherwise) build and run it, the others do nothing at that point of the cycle.
#include "gmg_internal.hpp"
#include "coefcoarsekernels.hpp"

struct CoefCoarseWs {
	te_gmg         *aux = nullptr;
	int             sub_n = 0;
	DevBuf<int32_t> origin;                                                // [Q][3] cell offsets of the auxiliary level-0 patches in the big patch
	te_vec         *f = nullptr, *u = nullptr;                             // auxiliary level-0 vectors of the sub-solve
	te_vec         *beta = nullptr, *sigma = nullptr;                      // ... the split coefficient and reaction term, handed to the auxiliary solver's own set calls
};

namespace tei
{
void coefCoarseFree(te_gmg *g)
{
	CoefCoarseWs *W = g->cc;
	if (!W) return;
	for (te_vec *v : {W->f, W->u, W->beta, W->sigma})
		if (v) te_vec_destroy(v);
	if (W->aux) te_gmg_destroy(W->aux); // (synchronises the shared stream; leaves it alone)
	delete W;
	g->cc     = nullptr;
	g->cc_aux = nullptr;
}

void coefCoarseRelease(te_gmg *g)
{
	if (g->cc_kind == TE_COEF_COARSE_SWEEPS) coefCoarseFree(g);
}

static bool pow2(int v) { return v >= 1 && (v & (v - 1)) == 0; }

// the shape of a sub-patch size alone: even, >= 4, in 3D one the kernels are instantiated for
static bool subShapeOk(int dim, int s) { return s >= 4 && (s & 1) == 0 && (dim == 2 || s == 4 || s == 8 || s == 16); }
// ... and it divides the one-patch level into a power of two >= 2 patches per axis
static bool subValid(int dim, int n, int s) { return subShapeOk(dim, s) && n % s == 0 && n / s >= 2 && pow2(n / s); }

static CoefCoarseGeom geomOf(const te_gmg *g)
{
	const CoefCoarseWs *W = g->cc;
	CoefCoarseGeom      G;
	G.D      = g->dim;
	G.n      = g->n;
	G.s      = W->sub_n;
	G.Q      = W->aux->levels[0]->P;
	G.origin = W->origin.p;
	return G;
}

static int splitCells(te_gmg *g, const double *big_a, double *aux_a, const double *big_b, double *aux_b)
{
	const CoefCoarseGeom G = geomOf(g);
	const size_t         pairs = (size_t) G.Q * g->cc->aux->levels[0]->nc / 2;
	Timed                t(g, KC_COEF_SPLIT, 2 * pairs * (big_b ? 2 : 1));
	hipLaunchKernelGGL(k_cc_cells<false>, dim3(gridFor(pairs, 256, 1 << 20)), dim3(256), 0, g->stream, G,
	                   reinterpret_cast<double2 *>(const_cast<double *>(big_a)), reinterpret_cast<double2 *>(aux_a),
	                   reinterpret_cast<const double2 *>(big_b), reinterpret_cast<double2 *>(aux_b));
	HIPCHK(hipGetLastError());
	return TE_OK;
}

static int mergeCells(te_gmg *g, const double *aux_a, double *big_a)
{
	const CoefCoarseGeom G = geomOf(g);
	const size_t         pairs = (size_t) G.Q * g->cc->aux->levels[0]->nc / 2;
	Timed                t(g, KC_COEF_MERGE, 2 * pairs);
	hipLaunchKernelGGL(k_cc_cells<true>, dim3(gridFor(pairs, 256, 1 << 20)), dim3(256), 0, g->stream, G, reinterpret_cast<double2 *>(big_a),
	                   reinterpret_cast<double2 *>(const_cast<double *>(aux_a)), (const double2 *) nullptr, (double2 *) nullptr);
	HIPCHK(hipGetLastError());
	return TE_OK;
}

static int splitFaces(te_gmg *g, const double *big, double *aux)
{
	const CoefCoarseGeom G = geomOf(g);
	const LevelHost     &A = *g->cc->aux->levels[0];
	const size_t         items = (size_t) G.Q * ((size_t) G.D * A.nc / 2 + (size_t) G.D * A.nf);
	Timed                t(g, KC_COEF_SPLIT, (size_t) G.Q * ((size_t) G.D * A.nc + (size_t) G.D * A.nf));
	hipLaunchKernelGGL(k_cc_split_faces, dim3(gridFor(items, 256, 1 << 20)), dim3(256), 0, g->stream, G, big, aux);
	HIPCHK(hipGetLastError());
	return TE_OK;
}

int coefCoarseRefresh(te_gmg *g, bool with_beta)
{
	CoefCoarseWs *W = g->cc;
	if (!W || g->cc_kind != TE_COEF_COARSE_SUBCYCLE) return TE_OK; // (te_gmg_set_coef_coarse refreshes when the kind comes back)
	te_gmg *x = W->aux;
	int     rc;
	if (!g->coef_on || !g->coef) return te_gmg_set_coefficient(x, nullptr); // (clears the auxiliary sigma as well)
	const int lc = (int) g->levels.size() - 1;
	if (with_beta) {
		if ((rc = splitFaces(g, g->coef->beta[lc]->d, W->beta->d)) || (rc = te_gmg_set_coefficient(x, W->beta))) return rc;
	}
	if (!g->coef->sigma_on) return te_gmg_set_reaction(x, nullptr);
	if ((rc = splitCells(g, g->coef->sigma[lc]->d, W->sigma->d, nullptr, nullptr))) return rc;
	return te_gmg_set_reaction(x, W->sigma);
}

int coefCoarseSolve(te_gmg *g, const te_cycle_opts *o, const te_vec *f, te_vec *u)
{
	// a rank without the coarsest patch has no part in it; the schedule check's dry run skips it (it exchanges nothing)
	if (g->levels.back()->P == 0 || g->recording) return TE_OK;
	CoefCoarseWs *W = g->cc;
	if (!W || !W->aux || !W->aux->coef_on || !W->aux->coef)
		return te::fail(TE_ESTATE, "te_vcycle: the sub-patch coarse solve has no coefficient (te_gmg_set_coef_coarse)");
	te_gmg *x = W->aux;
	int     rc;
	// a te_gmg_set_coefficient / te_gmg_set_reaction of the parent that was refused after it had cleared sigma never got to its refresh
	if (x->coef->sigma_on && !g->coef->sigma_on && (rc = te_gmg_set_reaction(x, nullptr))) return rc;
	if (x->coef->sigma_on != g->coef->sigma_on) return te::fail(TE_ESTATE, "te_vcycle: the sub-patch coarse solve's reaction term is stale");
	LevelHost &L = *g->levels.back();
	for (auto &A : x->levels) A->xf_valid_for = nullptr, A->ps_faces = false;
	x->interp = g->interp;
	if ((rc = splitCells(g, f->d, W->f->d, u->d, W->u->d))) return rc;
	for (int c = 0; c < g->cc_cycles; c++)
		if ((rc = visitCoef(x, o, 0, W->f, W->u))) return rc;
	x->cur_level = 0;
	if (L.xf_valid_for == u->d) L.xf_valid_for = nullptr; // u changes in place
	return mergeCells(g, W->u->d, u->d);
}

// the auxiliary tree, hierarchy and solver for sub-patch size s, with the offset table from the hierarchy's own level-0 starts
static int coefCoarseBuild(te_gmg *g, int s)
{
	const int    D = g->dim, n = g->n, refs = (int) std::lround(std::log2((double) (n / s)));
	te::Tree     tree = te::Tree::boxRoot(D, g->coarse_starts.data(), g->coarse_lengths.data());
	for (int i = 0; i < refs; i++) tree.refineLeaves();
	te_hier hier{te::Hierarchy::buildSides(tree, s, (int) g->placement[4], 0, 0.0, 0, 1)};
	auto    W = std::make_unique<CoefCoarseWs>();
	W->sub_n  = s;
	int rc;
	if ((rc = gmgCreate(&hier, g->device, g->stream, &W->aux))) return rc;
	struct Guard { // a failure below frees what exists so far
		std::unique_ptr<CoefCoarseWs> &W;
		bool                           keep = false;
		~Guard()
		{
			if (keep || !W) return;
			for (te_vec *v : {W->f, W->u, W->beta, W->sigma})
				if (v) te_vec_destroy(v);
			if (W->aux) te_gmg_destroy(W->aux);
		}
	} guard{W};
	te_gmg *x = W->aux;
	// the same switches, profile state and interpolator as the parent (te_gmg_create read the environment; te_gmg_set_option may have changed one since)
	x->cfg = g->cfg, x->zs_pin = g->zs_pin, x->resweep_pin = g->resweep_pin;
	x->profiling = g->profiling, x->prof_only = g->prof_only, x->prof_stride = g->prof_stride;
	const te::Level &lv = hier.h.levels[0];
	const int        Q  = n / s;
	if ((int) x->levels.back()->P != 1 || lv.P != (D == 3 ? Q * Q * Q : Q * Q))
		return te::fail(TE_ESTATE, "te_gmg_set_coef_coarse: the auxiliary hierarchy does not have the expected shape");
	std::vector<int32_t> origin((size_t) lv.P * 3, 0);
	for (int q = 0; q < lv.P; q++) {
		const int gq = lv.l2g[q];
		for (int a = 0; a < D; a++) {
			const double len = lv.g_lengths[(size_t) gq * D + a];
			const long   k   = std::lround((lv.g_starts[(size_t) gq * D + a] - g->coarse_starts[a]) / len);
			if (k < 0 || k >= Q) return te::fail(TE_ESTATE, "te_gmg_set_coef_coarse: an auxiliary patch lies outside the coarsest patch");
			origin[(size_t) q * 3 + a] = (int32_t) k * s;
		}
	}
	if ((rc = W->origin.upload(origin)) || (rc = te_vec_create(x, 0, &W->f)) || (rc = te_vec_create(x, 0, &W->u))
	    || (rc = te_vec_create(x, 0, &W->sigma)) || (rc = te_vec_create_faces(x, 0, &W->beta)))
		return rc;
	guard.keep = true;
	g->cc      = W.release();
	g->cc_aux  = g->cc->aux;
	return TE_OK;
}
} // namespace tei

extern "C" {
int te_gmg_set_coef_coarse(te_gmg *g, int kind, int sub_n, int cycles)
{
	return guarded([&]() -> int {
		int rc;
		if (!g) return te::fail(TE_EINVAL, "te_gmg_set_coef_coarse: null solver");
		if (kind != TE_COEF_COARSE_SWEEPS && kind != TE_COEF_COARSE_SUBCYCLE) return te::fail(TE_EINVAL, "te_gmg_set_coef_coarse: unknown kind");
		if (cycles < 1) return te::fail(TE_EINVAL, "te_gmg_set_coef_coarse: cycles must be at least 1");
		if (kind == TE_COEF_COARSE_SWEEPS) { // (the auxiliary solver stays until te_gmg_release_workspace; its coefficient may go stale meanwhile)
			g->cc_kind   = kind;
			g->cc_cycles = cycles;
			return TE_OK;
		}
		const int D = g->dim, n = g->n;
		if (sub_n != 0 && !subShapeOk(D, sub_n))
			return te::fail(TE_EINVAL, std::string("te_gmg_set_coef_coarse: sub_n must be even and at least 4") + (D == 3 ? ", in 3D one of 4, 8, 16" : ""));
		if ((rc = shardedNeedsTransport(g, "te_gmg_set_coef_coarse"))) return rc;
		if (g->coarse_P_global != 1) // (the global count: every rank of a sharded hierarchy returns the same code)
			return te::fail(TE_EUNSUPPORTED, "te_gmg_set_coef_coarse: the coarsest level has " + std::to_string(g->coarse_P_global)
			                                     + " patches; the sub-patch coarse solve needs a coarsest level of one patch");
		if (sub_n != 0 && !subValid(D, n, sub_n))
			return te::fail(TE_EINVAL, "te_gmg_set_coef_coarse: n / sub_n must be a power of two, at least 2 (n = " + std::to_string(n) + ")");
		// sub_n = 0: in 3D 8 where valid (at 512^3 and on 2refine.bin --divide 3 two cycles on 4^3 patches cost an iteration and lose to
		// 64 plain sweeps, on 8^3 patches they win: DESIGN.md section 20); otherwise the smallest valid size, which is 4 where 4 is valid
		int s = sub_n;
		if (s == 0 && D == 3 && subValid(D, n, 8)) s = 8;
		for (int c = 4; s == 0 && c <= n / 2; c += 2)
			if (subValid(D, n, c)) s = c;
		if (s == 0)
			return te::fail(TE_EUNSUPPORTED, "te_gmg_set_coef_coarse: no valid sub-patch size for patches of n = " + std::to_string(n) + " cells per axis");
		HIPCHK(hipSetDevice(g->device));
		if (g->cc && g->cc->sub_n != s) {
			HIPCHK(hipStreamSynchronize(g->stream));
			coefCoarseFree(g);
		}
		// (sharded: only a rank that holds the one coarsest patch has an auxiliary solver; the others keep the settings alone)
		if (!g->cc && g->levels.back()->P == 1 && (rc = coefCoarseBuild(g, s))) return rc;
		g->cc_sub_n        = s; // (what the auxiliary solver has, whatever follows)
		const int old_kind = g->cc_kind;
		g->cc_kind         = kind;
		if ((rc = coefCoarseRefresh(g, true))) { // (with a coefficient set: its split copies, now)
			g->cc_kind = old_kind;
			return rc;
		}
		g->cc_cycles = cycles;
		return TE_OK;
	});
}

int te_gmg_coef_coarse(const te_gmg *g, int *kind, int *sub_n, int *cycles)
{
	return guarded([&]() -> int {
		if (!g) return te::fail(TE_EINVAL, "te_gmg_coef_coarse: null solver");
		if (kind) *kind = g->cc_kind;
		if (sub_n) *sub_n = g->cc_sub_n;
		if (cycles) *cycles = g->cc_cycles;
		return TE_OK;
	});
}
} // extern "C"
