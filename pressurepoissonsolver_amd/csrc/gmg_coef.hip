// The variable-coefficient operator A_b = div(beta grad .) next to the Laplacian (coefkernels.hpp): the solver's
// copy of the coefficient on every level (te_gmg_set_coefficient, te_faces_restrict), the operator, residual and sweeps that te_apply /
// te_residual / te_smooth hand over while a coefficient is set, and the plain cycle driver visitCoef behind te_vcycle. A second,
// unfused path: nothing here touches the kernels or the driver of the constant-coefficient one. Single rank.
// The reaction term sigma (te_gmg_set_reaction) lives here too: per-level cell vectors beside beta's, and every
// launch below picks its kernel's SIG instantiation by g->coef->sigma_on -- A_b,sigma = A_b - sigma in operator, residual and sweeps.
#include "gmg_ghosts3d.hpp"
#include "coefkernels.hpp" // (with faceregridkernels.hpp: the LAST include, FMA contraction is off from there on)

namespace tei
{
static void sigmaFree(CoefWs *W)
{
	for (te_vec *v : W->sigma)
		if (v) te_vec_destroy(v);
	W->sigma.clear();
	W->sigma_on = false;
}

void coefFree(te_gmg *g)
{
	if (!g->coef) return;
	sigmaFree(g->coef);
	for (te_vec *v : g->coef->beta)
		if (v) te_vec_destroy(v);
	delete g->coef;
	g->coef    = nullptr;
	g->coef_on = false;
}

// te_gmg_release_workspace: everything while no coefficient is set; with one set, the sigma buffers while sigma is cleared
void coefRelease(te_gmg *g)
{
	if (!g->coef_on)
		coefFree(g);
	else if (g->coef && !g->coef->sigma_on)
		sigmaFree(g->coef);
}

// the level's sigma while one is set, else nullptr (the launches pick their SIG instantiation by it)
static const double *sigmaOf(const te_gmg *g, const LevelHost &L)
{
	return g->coef->sigma_on ? g->coef->sigma[L.index]->d : nullptr;
}

static int checkFaces(te_gmg *g, int level, const te_vec *v, const char *who)
{
	if (!v || level < 0 || level >= (int) g->levels.size() || v->g != g || v->level != level || !v->faces)
		return te::fail(TE_EINVAL, std::string(who) + ": not a face vector of level " + std::to_string(level) + " of this solver");
	return TE_OK;
}

// g->coef, and on a sharded hierarchy the device side of every level's face restriction across ranks (CoefWs::fxfer): block offsets,
// send and receive buffer, sized from the level's face totals. A level on which this rank sends and receives nothing allocates nothing.
static int coefWorkspace(te_gmg *g)
{
	if (!g->coef) g->coef = new CoefWs;
	CoefWs &W = *g->coef;
	if (g->nranks == 1 || !W.fxfer.empty()) return TE_OK;
	HIPCHK(hipSetDevice(g->device));
	std::vector<std::unique_ptr<CoefFaceXfer>> fx;
	for (auto &L : g->levels) {
		auto X = std::make_unique<CoefFaceXfer>();
		int  rc;
		if ((rc = X->up_foff.upload(L->up_foff_host)) || (rc = X->down_foff.upload(L->down_foff_host))
		    || (rc = X->up.alloc((size_t) L->up_ftotal)) || (rc = X->down.alloc((size_t) L->down_ftotal)))
			return rc;
		fx.push_back(std::move(X));
	}
	W.fxfer = std::move(fx);
	return TE_OK;
}

// coarse = the face average of fine (level l -> l + 1), through level l's child / copy tables. Sharded: children whose parent lives
// on another rank (under repl_up: every local patch, one copy for everybody) restrict themselves into their block of the send
// buffer, the blocks travel through the attached back-end under a tag of their own, and the coarse side picks its entries from
// local children and received blocks alike (coefkernels.hpp). Recording: nothing moves, the exchange is recorded.
static int facesRestrict(te_gmg *g, int l, const double *fine, double *coarse)
{
	LevelHost    &L = *g->levels[l];
	CoefFaceXfer *X = nullptr;
	int           rc;
	if (g->nranks > 1) {
		if ((rc = coefWorkspace(g))) return rc;
		X = g->coef->fxfer[l].get();
		if (L.n_up > 0 && L.up_ftotal > 0) {
			Timed t(g, KC_PACK, (size_t) L.up_ftotal);
			if (L.dim == 2)
				hipLaunchKernelGGL(k_faces_restrict_pack2d, dim3(L.n_up), dim3(256), 0, g->stream, L.n, L.up_desc.p, X->up_foff.p, fine, X->up.p);
			else
				dispatchN(L.n, [&](auto n) {
					hipLaunchKernelGGL(k_faces_restrict_pack3d<decltype(n)::value>, dim3(L.n_up), dim3(256), 0, g->stream, L.up_desc.p, X->up_foff.p, fine,
					                   X->up.p);
				});
			HIPCHK(hipGetLastError());
		}
		if ((rc = doExchange(g, 4, L.tx_fup, X->up.p, X->down.p))) return rc; // (tags 1 - 3: faces, restriction, prolongation)
	}
	if (L.Pc == 0) return TE_OK;
	Timed t(g, KC_FACES_RESTRICT, (size_t) L.Pc * L.nc);
	if (X && L.n_down > 0) { // some child's block was received: the form that reads local children and blocks alike
		const size_t FV   = (size_t) L.dim * L.nc + (size_t) L.dim * L.nf;
		const dim3   grid(gridFor((size_t) L.Pc * FV, 256, 65536));
		if (L.dim == 2)
			hipLaunchKernelGGL(k_faces_restrict_recv2d, grid, dim3(256), 0, g->stream, L.n, L.Pc, L.child.p, L.copy.p, fine, (const double *) X->down.p,
			                   X->down_foff.p, coarse);
		else
			dispatchN(L.n, [&](auto n) {
				hipLaunchKernelGGL(k_faces_restrict_recv3d<decltype(n)::value>, grid, dim3(256), 0, g->stream, L.Pc, L.child.p, L.copy.p, fine,
				                   (const double *) X->down.p, X->down_foff.p, coarse);
			});
		HIPCHK(hipGetLastError());
		return TE_OK;
	}
	if (L.dim == 2)
		hipLaunchKernelGGL(k_faces_restrict2d, dim3(gridFor((size_t) L.Pc * L.nc / 2, 256, 65536)), dim3(256), 0, g->stream, L.n, L.Pc, L.child.p,
		                   L.copy.p, fine, coarse);
	else
		dispatchN(L.n, [&](auto n) {
			hipLaunchKernelGGL(k_faces_restrict3d<decltype(n)::value>, dim3(L.Pc), dim3(256), 0, g->stream, L.Pc, L.child.p, L.copy.p, fine, coarse);
		});
	HIPCHK(hipGetLastError());
	return TE_OK;
}

static CoefLevel coefLevel(const te_gmg *g, const LevelHost &L)
{
	CoefLevel C;
	C.P         = L.P;
	C.n         = L.n;
	C.face_kind = L.face_kind.p;
	C.face_src  = L.face_src.p;
	C.face_kadj = L.face_kadj.p;
	C.rh2       = L.rh2.p;
	C.ghost     = L.ghostCur();
	C.beta      = g->coef->beta[L.index]->d;
	return C;
}

// the level's ghost slots from u, exactly as te_apply makes them current
static int coefGhosts(te_gmg *g, LevelHost &L, const double *u)
{
	if (L.dim == 2) return prepareGhosts2d(g, L, u);
	return dispatchN(L.n, [&](auto n) { return prepareGhosts<decltype(n)::value>(g, L, GhostSrc{u}); });
}

template <bool SIG>
static void stencil2d(te_gmg *g, const CoefLevel &C, dim3 grid, int mode, const double *u, const double *f, double *out, double omega, const double *sigma)
{
	if (mode == COEF_APPLY)
		hipLaunchKernelGGL((k_coef_stencil2d<COEF_APPLY, SIG>), grid, dim3(256), 0, g->stream, C, u, f, out, omega, sigma);
	else if (mode == COEF_RESID)
		hipLaunchKernelGGL((k_coef_stencil2d<COEF_RESID, SIG>), grid, dim3(256), 0, g->stream, C, u, f, out, omega, sigma);
	else
		hipLaunchKernelGGL((k_coef_stencil2d<COEF_JACOBI, SIG>), grid, dim3(256), 0, g->stream, C, u, f, out, omega, sigma);
}

// 3D: the plane march k_coef_stencil3d<N, MODE, ZS>, slabs by the stencil kernels' rule, ghosts through withGhosts as for te_apply
template <int N, int MODE> static int coefStencilN(te_gmg *g, LevelHost &L, const double *u, const double *f, double *out, double omega)
{
	const int     zs   = stencilSlabs<N>(g, L.P);
	const double *beta = g->coef->beta[L.index]->d, *sigma = sigmaOf(g, L);
	auto          launch = [&](LevelDev D) {
		if (D.count == 0) return;
		Timed t(g, MODE == COEF_APPLY ? KC_APPLY_COEF : (MODE == COEF_RESID ? KC_RESID_COEF : KC_JACOBI_COEF), (size_t) D.count * L.nc);
		dispatchSlabs<N>(zs, [&](auto z) {
			if (sigma)
				hipLaunchKernelGGL((k_coef_stencil3d<N, MODE, decltype(z)::value, true>), slabGrid(D.count, zs), dim3(Tile3<N>::TPB), 0, g->stream, D,
				                   beta, u, f, out, omega, sigma);
			else
				hipLaunchKernelGGL((k_coef_stencil3d<N, MODE, decltype(z)::value, false>), slabGrid(D.count, zs), dim3(Tile3<N>::TPB), 0, g->stream, D,
				                   beta, u, f, out, omega, sigma);
		});
	};
	int rc = withGhosts<N>(g, L, {u}, launch);
	if (rc) return rc;
	HIPCHK(hipGetLastError());
	return TE_OK;
}

int coefStencil(te_gmg *g, LevelHost &L, int mode, const double *u, const double *f, double *out, double omega)
{
	if (!g->coef || !g->coef_on) return te::fail(TE_ESTATE, "coefStencil: no coefficient is set");
	if (L.xf_valid_for == out) L.xf_valid_for = nullptr; // out changes
	if (L.P == 0) return TE_OK;
	if (L.dim == 3)
		return dispatchN(L.n, [&](auto n) {
			constexpr int N = decltype(n)::value;
			if (mode == COEF_APPLY) return coefStencilN<N, COEF_APPLY>(g, L, u, f, out, omega);
			if (mode == COEF_RESID) return coefStencilN<N, COEF_RESID>(g, L, u, f, out, omega);
			return coefStencilN<N, COEF_JACOBI>(g, L, u, f, out, omega);
		});
	int rc = coefGhosts(g, L, u);
	if (rc) return rc;
	Timed      t(g, mode == COEF_APPLY ? KC_APPLY_COEF : (mode == COEF_RESID ? KC_RESID_COEF : KC_JACOBI_COEF), (size_t) L.P * L.nc);
	const dim3 grid(gridFor((size_t) L.P * L.nc, 256, 1 << 30)); // (one cell per thread: a flat grid in address order, see vecop)
	if (const double *sigma = sigmaOf(g, L))
		stencil2d<true>(g, coefLevel(g, L), grid, mode, u, f, out, omega, sigma);
	else
		stencil2d<false>(g, coefLevel(g, L), grid, mode, u, f, out, omega, nullptr);
	HIPCHK(hipGetLastError());
	return TE_OK;
}

// 3D: the lagged single-pass march k_coef_rbgs3d<N, ZS>, slabs by the sweep kernels' rule
template <int N> static int coefRbgsN(te_gmg *g, LevelHost &L, const double *u, const double *f, double *out)
{
	const double *beta = g->coef->beta[L.index]->d, *sigma = sigmaOf(g, L);
	auto          launch = [&](LevelDev D) {
		if (D.count == 0) return;
		const int zs = rbgsSlabs<N>(g, D.count);
		Timed     t(g, KC_RBGS_COEF, (size_t) D.count * L.nc);
		dispatchSlabs<N>(zs, [&](auto z) {
			if (sigma)
				hipLaunchKernelGGL((k_coef_rbgs3d<N, decltype(z)::value, true>), slabGrid(D.count, zs), dim3(Tile3<N>::TPB), 0, g->stream, D, beta, u,
				                   f, out, sigma);
			else
				hipLaunchKernelGGL((k_coef_rbgs3d<N, decltype(z)::value, false>), slabGrid(D.count, zs), dim3(Tile3<N>::TPB), 0, g->stream, D, beta, u,
				                   f, out, sigma);
		});
	};
	int rc = withGhosts<N>(g, L, {u}, launch);
	if (rc) return rc;
	HIPCHK(hipGetLastError());
	return TE_OK;
}

// one red-black sweep: out = S(u, f), u != out
static int coefRbgs(te_gmg *g, LevelHost &L, const double *u, const double *f, double *out)
{
	if (L.xf_valid_for == out) L.xf_valid_for = nullptr;
	if (L.P == 0) return TE_OK;
	if (L.dim == 3) return dispatchN(L.n, [&](auto n) { return coefRbgsN<decltype(n)::value>(g, L, u, f, out); });
	int rc = coefGhosts(g, L, u);
	if (rc) return rc;
	Timed           t(g, KC_RBGS_COEF, (size_t) L.P * L.nc);
	const CoefLevel C = coefLevel(g, L);
	const double   *sigma = sigmaOf(g, L);
	auto            launch = [&](auto sig) {
		constexpr bool SIG = decltype(sig)::value;
		if (L.n <= 64) { // the patch and its ring fit in LDS: both colours in one launch
			hipLaunchKernelGGL(k_coef_rbgs2d_lds<SIG>, dim3(L.P), dim3(256), sizeof(double) * (size_t) (L.n + 2) * (L.n + 2), g->stream, C, u, f, out,
			                   sigma);
		} else {
			const dim3 grid(gridFor((size_t) L.P * L.nc, 256, 1 << 30));
			hipLaunchKernelGGL((k_coef_rbgs2d<0, SIG>), grid, dim3(256), 0, g->stream, C, u, f, out, sigma);
			hipLaunchKernelGGL((k_coef_rbgs2d<1, SIG>), grid, dim3(256), 0, g->stream, C, u, f, out, sigma);
		}
	};
	if (sigma)
		launch(std::true_type{});
	else
		launch(std::false_type{});
	HIPCHK(hipGetLastError());
	return TE_OK;
}

int coefSmoothOnce(te_gmg *g, int level, const te_vec *f, te_vec *u, int smoother, double omega)
{
	LevelHost &L = *g->levels[level];
	int        rc;
	L.xf_valid_for = nullptr;
	switch (smoother) {
		case TE_SMOOTH_JACOBI: rc = coefStencil(g, L, COEF_JACOBI, u->d, f->d, L.t->d, omega); break;
		case TE_SMOOTH_RBGS: rc = coefRbgs(g, L, u->d, f->d, L.t->d); break;
		case TE_SMOOTH_PATCH_SOLVE:
		case TE_SMOOTH_PATCH_BCGS:
			return te::fail(TE_EUNSUPPORTED, "te_smooth: with a coefficient set only TE_SMOOTH_RBGS and TE_SMOOTH_JACOBI exist (the patch solves invert "
			                                 "the constant-coefficient patch operator)");
		default: return te::fail(TE_EINVAL, "te_smooth: unknown smoother");
	}
	if (rc) return rc;
	swapData(u, L.t.get());
	return TE_OK;
}

// GMG/Cycle.h:56-126 with VCycle.h:44-62 / WCycle.h:45-68, statement for statement, on A_b: no fused form, no exact coarse solve
// (the coarsest level runs coarse_sweeps sweeps of o->smoother, or with TE_COEF_COARSE_SUBCYCLE the sub-patch cycles of
// gmg_coefcoarse.hip). The transfers are the constant-coefficient cycle's own.
int visitCoef(te_gmg *g, const te_cycle_opts *o, int l, const te_vec *f, te_vec *u)
{
	const int  nl = (int) g->levels.size();
	LevelHost &L  = *g->levels[l];
	int        rc;
	g->cur_level  = l;
	auto smooth = [&](int sweeps) -> int {
		for (int i = 0; i < sweeps; i++)
			if (int r = coefSmoothOnce(g, l, f, u, o->smoother, o->omega)) return r;
		return TE_OK;
	};
	if (l == nl - 1) return g->cc_kind == TE_COEF_COARSE_SUBCYCLE ? coefCoarseSolve(g, o, f, u) : smooth(o->coarse_sweeps);
	LevelHost &C = *g->levels[l + 1];
	auto descend = [&]() -> int {
		int r;
		if ((r = coefStencil(g, L, COEF_RESID, u->d, f->d, L.r->d, 0.0))) return r; // prepCoarser: r = f - A_b u
		if ((r = doRestrict(g, l, L.r->d, C.f->d))) return r;
		if ((r = vecop<VOP_SET>(C.u.get(), nullptr, nullptr, 0.0, 0.0, 0.0))) return r;
		if ((r = visitCoef(g, o, l + 1, C.f.get(), C.u.get()))) return r;
		g->cur_level   = l;
		L.xf_valid_for = nullptr; // prepFiner: u changes in place
		return g->interp == TE_INTERP_DIRECT ? doProlong(g, l, C.u->d, u->d) : doProlongLinear(g, l, C.u->d, u->d);
	};
	if ((rc = smooth(o->pre_sweeps)) || (rc = descend())) return rc;
	if (o->cycle_type == 1 && ((rc = smooth(o->mid_sweeps)) || (rc = descend()))) return rc;
	return smooth(o->post_sweeps);
}

int vcycleCoef(te_gmg *g, const te_cycle_opts *o, const te_vec *f, te_vec *u)
{
	int rc;
	if (!o) return te::fail(TE_EINVAL, "te_vcycle: null options");
	if ((rc = checkLevelVec(g, 0, f, "te_vcycle")) || (rc = checkLevelVec(g, 0, u, "te_vcycle"))) return rc;
	if (o->smoother != TE_SMOOTH_RBGS && o->smoother != TE_SMOOTH_JACOBI)
		return te::fail(TE_EUNSUPPORTED, "te_vcycle: with a coefficient set only TE_SMOOTH_RBGS and TE_SMOOTH_JACOBI exist");
	// several ranks: the placement check and, with new options, the dry run of the driver below (gmg_cycle.hip), as te_vcycle does
	// without a coefficient
	if ((rc = verifyBeforeCycle(g, o))) return rc;
	// (what CycleScope does around visit(): this driver keeps no compact x faces and no face-layer iterates, so nothing but the reset)
	for (auto &L : g->levels) L->xf_valid_for = nullptr, L->ps_faces = false;
	if ((rc = te_vec_set(u, 0.0))) return rc; // Cycle.h:118
	rc           = visitCoef(g, o, 0, f, u);
	g->cur_level = 0;
	return rc;
}
} // namespace tei

extern "C" {
int te_faces_restrict(te_gmg *g, int fine_level, const te_vec *fine, te_vec *coarse)
{
	return guarded([&]() -> int {
		int rc;
		if (!g) return te::fail(TE_EINVAL, "te_faces_restrict: null solver");
		if ((rc = shardedNeedsTransport(g, "te_faces_restrict"))) return rc;
		if (fine_level < 0 || fine_level + 1 >= (int) g->levels.size()) return te::fail(TE_EINVAL, "te_faces_restrict: no coarser level below this one");
		if ((rc = checkFaces(g, fine_level, fine, "te_faces_restrict")) || (rc = checkFaces(g, fine_level + 1, coarse, "te_faces_restrict"))) return rc;
		return facesRestrict(g, fine_level, fine->d, coarse->d);
	});
}

int te_gmg_set_coefficient(te_gmg *g, const te_vec *beta)
{
	return guarded([&]() -> int {
		int rc;
		if (!g) return te::fail(TE_EINVAL, "te_gmg_set_coefficient: null solver");
		for (auto &L : g->levels) L->xf_valid_for = nullptr; // (the operator changes)
		if (g->coef) g->coef->sigma_on = false; // every call clears sigma: never a new beta with a stale sigma (the order per step is beta, then sigma)
		if (!beta) { // (nothing to clear where none is set)
			g->coef_on = false;
			return coefCoarseRefresh(g, true);
		}
		if ((rc = shardedNeedsTransport(g, "te_gmg_set_coefficient"))) return rc;
		if ((rc = checkFaces(g, 0, beta, "te_gmg_set_coefficient"))) return rc;
		const int nl = (int) g->levels.size();
		if ((rc = coefWorkspace(g))) return rc;
		if (g->coef->beta.empty()) {
			g->coef->beta.assign(nl, nullptr);
			for (int l = 0; l < nl; l++)
				if ((rc = te_vec_create_faces(g, l, &g->coef->beta[l]))) {
					coefFree(g);
					return rc;
				}
		}
		// from here on the per-level copies are being rewritten: a failure leaves NO coefficient set (never a partly updated one)
		g->coef_on = false;
		auto &B    = g->coef->beta;
		if (beta->n) HIPCHK(hipMemcpyAsync(B[0]->d, beta->d, sizeof(double) * beta->n, hipMemcpyDeviceToDevice, g->stream));
		for (int l = 0; l + 1 < nl; l++)
			if ((rc = facesRestrict(g, l, B[l]->d, B[l + 1]->d))) return rc;
		g->coef_on = true;
		if ((rc = coefCoarseRefresh(g, true))) g->coef_on = false; // (the sub-patch coarse solve's copies: never a stale one)
		return rc;
	});
}

int te_gmg_has_coefficient(const te_gmg *g)
{
	return guarded([&]() -> int { return (g && g->coef_on) ? 1 : 0; });
}

int te_gmg_coefficient(te_gmg *g, int level, te_vec *out)
{
	return guarded([&]() -> int {
		int rc;
		if (!g) return te::fail(TE_EINVAL, "te_gmg_coefficient: null solver");
		if (!g->coef_on || !g->coef) return te::fail(TE_ESTATE, "te_gmg_coefficient: no coefficient is set");
		if ((rc = checkFaces(g, level, out, "te_gmg_coefficient"))) return rc;
		if (out->n) HIPCHK(hipMemcpyAsync(out->d, g->coef->beta[level]->d, sizeof(double) * out->n, hipMemcpyDeviceToDevice, g->stream));
		return TE_OK;
	});
}

int te_gmg_set_reaction(te_gmg *g, const te_vec *sigma)
{
	return guarded([&]() -> int {
		int rc;
		if (!g) return te::fail(TE_EINVAL, "te_gmg_set_reaction: null solver");
		for (auto &L : g->levels) L->xf_valid_for = nullptr; // (the operator changes)
		if (!sigma) { // (also where none can be set: nothing to clear)
			if (g->coef) g->coef->sigma_on = false;
			return coefCoarseRefresh(g, false);
		}
		if ((rc = shardedNeedsTransport(g, "te_gmg_set_reaction"))) return rc;
		if (!g->coef_on || !g->coef)
			return te::fail(TE_ESTATE, "te_gmg_set_reaction: no coefficient is set (sigma lives on the coefficient path: te_gmg_set_coefficient first, "
			                           "a face vector of ones for the Laplacian)");
		if ((rc = checkLevelVec(g, 0, sigma, "te_gmg_set_reaction"))) return rc;
		const int nl = (int) g->levels.size();
		auto     &S  = g->coef->sigma;
		// from here on the per-level copies are being rewritten: a failure leaves NO sigma set
		g->coef->sigma_on = false;
		if (S.empty()) {
			S.assign(nl, nullptr);
			for (int l = 0; l < nl; l++)
				if ((rc = te_vec_create(g, l, &S[l]))) {
					sigmaFree(g->coef);
					return rc;
				}
		}
		if (sigma->n) HIPCHK(hipMemcpyAsync(S[0]->d, sigma->d, sizeof(double) * sigma->n, hipMemcpyDeviceToDevice, g->stream));
		for (int l = 0; l + 1 < nl; l++)
			if ((rc = doRestrict(g, l, S[l]->d, S[l + 1]->d))) return rc; // te_restrict's average; copy-through patches bit for bit
		g->coef->sigma_on = true;
		if ((rc = coefCoarseRefresh(g, false))) g->coef->sigma_on = false;
		return rc;
	});
}

int te_gmg_has_reaction(const te_gmg *g)
{
	return guarded([&]() -> int { return (g && g->coef_on && g->coef && g->coef->sigma_on) ? 1 : 0; });
}

int te_gmg_reaction(te_gmg *g, int level, te_vec *out)
{
	return guarded([&]() -> int {
		int rc;
		if (!g) return te::fail(TE_EINVAL, "te_gmg_reaction: null solver");
		if (!g->coef_on || !g->coef || !g->coef->sigma_on) return te::fail(TE_ESTATE, "te_gmg_reaction: no reaction term is set");
		if ((rc = checkLevelVec(g, level, out, "te_gmg_reaction"))) return rc;
		if (out->n) HIPCHK(hipMemcpyAsync(out->d, g->coef->sigma[level]->d, sizeof(double) * out->n, hipMemcpyDeviceToDevice, g->stream));
		return TE_OK;
	});
}
} // extern "C"
