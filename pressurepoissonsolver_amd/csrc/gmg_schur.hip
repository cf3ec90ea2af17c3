// The Schur-complement route, single rank (include/te_hip.h "Schur-complement interface route"):
// SchurHelper.h:280-397, Operators/SchurWrapOp.h, PolyChebPrec.cpp and BiCGStab<D-1> on the interface vector.
//   T gamma = Interp(Solve(0, gamma)), S = I - T, g = Interp(Solve(f, 0)); S gamma* = g; u = Solve(f, gamma*).
// Solve(f, gamma) is the exact patch solve of the reference smoother with right-hand side f - 2 gamma / h^2 on the face layers.
// Two forms of T:
//   faces-only  32^3 patches whose solve takes the single-pass kernel with pure axes on every patch: k_iface_corr, then
//               k_ps_sym<CORR, FACES, NOF> (no right-hand side read, only the six face layers of the result written), then
//               k_iface_interp from those face layers -- 3 B per site of patch-solve traffic instead of 16
//   full        everything else (other patch sizes, 2D, mixed Dirichlet/Neumann patches, few patches, TE_SCHUR_FULL): the
//               right-hand side f - corr into a scratch domain vector (k_iface_rhs), the level's own zero-guess patch solve
//               (patchSolve, whatever kernel it picks), k_iface_interp from the result
#include "gmg_internal.hpp"
#include "schurkernels.hpp"

namespace tei
{
struct SchurLevel {
	bool            ready = false;
	DevBuf<int32_t> own, start;
	DevBuf<int4>    contrib;
	DevBuf<double>  corr, f6; // [P][2D][n^(D-1)], [P][6][n^2] (faces-only form)
	te_vec         *w = nullptr, *ws = nullptr; // domain scratch: right-hand side / solution of the full form
	te_vec         *iv[12] = {nullptr};         // interface work vectors: BiCGStab (8), Chebyshev (3), g (1)
};
} // namespace tei

struct SchurWs {
	std::vector<std::unique_ptr<tei::SchurLevel>> lv;
	bool                                          attr = false; // dynamic-LDS attribute of k_ps_sym<true, true, true> set
};

namespace tei
{
void schurFree(te_gmg *g)
{
	if (!g->schur) return;
	for (auto &s : g->schur->lv) {
		if (!s) continue;
		for (te_vec *v : {s->w, s->ws})
			if (v) te_vec_destroy(v);
		for (te_vec *v : s->iv)
			if (v) te_vec_destroy(v);
	}
	delete g->schur;
	g->schur = nullptr;
}

// the level's device tables and scratch, made at the first call that needs them
static int schurLevel(te_gmg *g, int level, SchurLevel **out)
{
	if (!g || level < 0 || level >= (int) g->levels.size()) return te::fail(TE_EINVAL, "Schur route: bad level");
	LevelHost &L = *g->levels[level];
	if (g->nranks > 1 || L.nif < 0) return te::fail(TE_ESTATE, "Schur route: single-rank hierarchies only");
	if (!g->schur) g->schur = new SchurWs;
	auto &V = g->schur->lv;
	if ((int) V.size() < (int) g->levels.size()) V.resize(g->levels.size());
	if (!V[level]) V[level] = std::make_unique<SchurLevel>();
	SchurLevel &S = *V[level];
	if (!S.ready) { // (a failed first attempt leaves what it allocated in place; the next one fills in only what is missing)
		int rc;
		HIPCHK(hipSetDevice(g->device));
		std::vector<int4> c(L.if_contrib.size() / 4);
		for (size_t k = 0; k < c.size(); k++)
			c[k] = int4{L.if_contrib[4 * k], L.if_contrib[4 * k + 1], L.if_contrib[4 * k + 2], L.if_contrib[4 * k + 3]};
		if ((rc = S.own.upload(L.if_own)) || (rc = S.start.upload(L.if_start)) || (rc = S.contrib.upload(c))
		    || (rc = S.corr.alloc((size_t) L.P * 2 * L.dim * L.nf)))
			return rc; // (DevBuf::alloc / upload release an earlier allocation first)
		if (L.dim == 3 && L.n == 32 && (rc = S.f6.alloc((size_t) L.P * 6 * L.nf))) return rc;
		if ((!S.w && (rc = newVec(g, level, &S.w))) || (!S.ws && (rc = newVec(g, level, &S.ws)))) return rc;
		for (te_vec *&v : S.iv)
			if (!v && (rc = te_vec_create_iface(g, level, &v))) return rc;
		S.ready = true;
	}
	*out = &S;
	return TE_OK;
}

static int checkIface(te_gmg *g, int level, const te_vec *v, const char *who)
{
	if (!v || v->g != g || v->level != level || !v->iface)
		return te::fail(TE_EINVAL, std::string(who) + ": an interface vector of this level is needed");
	return TE_OK;
}

// gamma -> S.corr
static int ifaceCorr(te_gmg *g, LevelHost &L, SchurLevel &S, const double *gamma)
{
	if (L.P == 0) return TE_OK;
	Timed t(g, KC_PATCH_RHS, (size_t) L.P * 2 * L.dim * L.nf);
	if (L.dim == 3)
		hipLaunchKernelGGL(k_iface_corr<3>, dim3(L.P * 6), dim3(256), 0, g->stream, L.n, S.own.p, L.rh2.p, gamma, S.corr.p);
	else
		hipLaunchKernelGGL(k_iface_corr<2>, dim3(L.P * 4), dim3(256), 0, g->stream, L.n, S.own.p, L.rh2.p, gamma, S.corr.p);
	HIPCHK(hipGetLastError());
	return TE_OK;
}

// out = f -+ S.corr on the face layers (f may be null: zero; may equal out)
static int ifaceRhs(te_gmg *g, LevelHost &L, SchurLevel &S, const double *f, double *out, bool add)
{
	const size_t total = (size_t) L.P * L.nc;
	if (total == 0) return TE_OK;
	Timed      t(g, KC_PATCH_RHS, total);
	const dim3 grid(gridFor(total, 256, 1 << 20)), blk(256);
	if (L.dim == 3) {
		if (add) hipLaunchKernelGGL((k_iface_rhs<3, true>), grid, blk, 0, g->stream, total, L.n, f, S.corr.p, out);
		else hipLaunchKernelGGL((k_iface_rhs<3, false>), grid, blk, 0, g->stream, total, L.n, f, S.corr.p, out);
	} else {
		if (add) hipLaunchKernelGGL((k_iface_rhs<2, true>), grid, blk, 0, g->stream, total, L.n, f, S.corr.p, out);
		else hipLaunchKernelGGL((k_iface_rhs<2, false>), grid, blk, 0, g->stream, total, L.n, f, S.corr.p, out);
	}
	HIPCHK(hipGetLastError());
	return TE_OK;
}

// gamma = Interp(src); f6: src holds the six face layers per patch
static int ifaceInterp(te_gmg *g, LevelHost &L, SchurLevel &S, const double *src, double *gamma, bool f6)
{
	if (L.nif <= 0) return TE_OK;
	Timed t(g, KC_PATCH_RHS, (size_t) L.nif * L.nf);
	if (L.dim == 3) {
		if (f6) hipLaunchKernelGGL((k_iface_interp<3, true>), dim3(L.nif), dim3(256), 0, g->stream, L.n, S.start.p, S.contrib.p, src, gamma);
		else hipLaunchKernelGGL((k_iface_interp<3, false>), dim3(L.nif), dim3(256), 0, g->stream, L.n, S.start.p, S.contrib.p, src, gamma);
	} else {
		hipLaunchKernelGGL((k_iface_interp<2, false>), dim3(L.nif), dim3(256), 0, g->stream, L.n, S.start.p, S.contrib.p, src, gamma);
	}
	HIPCHK(hipGetLastError());
	return TE_OK;
}

// u = Solve(f, gamma) (f, gamma may be null: zero); returns in *res where the solution is (u, or the level's scratch in 2D)
static int solveWith(te_gmg *g, LevelHost &L, SchurLevel &S, const double *f, const double *gamma, double *u, const double **res)
{
	int rc;
	*res = u;
	if (L.P == 0) return TE_OK;
	if (gamma) {
		if ((rc = ifaceCorr(g, L, S, gamma)) || (rc = ifaceRhs(g, L, S, f, S.w->d, false))) return rc;
		f = S.w->d;
	} else if (!f) {
		HIPCHK(hipMemsetAsync(S.w->d, 0, sizeof(double) * S.w->n, g->stream));
		f = S.w->d;
	}
	bool swapped = false;
	if ((rc = patchSolve(g, L, f, u, {true}, &swapped))) return rc;
	if (swapped) *res = L.t->d; // (2D: the solve's result stays in its scratch)
	return TE_OK;
}

// the faces-only form of T applies where the full form's patch solve would run k_ps_sym on every patch (patchSolveN's own
// routing, psAllSym32): the two forms then run the same transforms and are bit-identical
static bool facesOnly(te_gmg *g, const LevelHost &L) { return !g->cfg.has(O_SCHUR_FULL) && L.matsym.p && psAllSym32(g, L); }

// y = T x
static int applyT(te_gmg *g, LevelHost &L, SchurLevel &S, const double *x, double *y)
{
	int rc;
	if (L.nif <= 0) return TE_OK;
	if (facesOnly(g, L)) {
		if (!g->schur->attr) {
			HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_ps_sym<true, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
			                           PSS_LDS_BYTES));
			g->schur->attr = true;
		}
		if (!g->ncu) {
			int dev = 0;
			HIPCHK(hipGetDevice(&dev));
			HIPCHK(hipDeviceGetAttribute(&g->ncu, hipDeviceAttributeMultiprocessorCount, dev));
		}
		if ((rc = ifaceCorr(g, L, S, x))) return rc;
		{
			Timed t(g, KC_PS_MFMA_FACES, (size_t) L.P * L.nc, true);
			launchT(t, (k_ps_sym<true, true, true>), dim3(std::min(L.P, g->ncu)), dim3(512), PSS_LDS_BYTES, g->stream, L.P, L.plan.p,
			        L.matsym.p, L.psinv.p, L.psitab.p, (const double *) S.w->d, (const double *) S.corr.p, S.ws->d,
			        (double *) nullptr, (const int32_t *) nullptr, S.f6.p); // (in / out: valid buffers that NOF / FACES never touch)
			HIPCHK(hipGetLastError());
		}
		return ifaceInterp(g, L, S, S.f6.p, y, true);
	}
	const double *res;
	if ((rc = solveWith(g, L, S, nullptr, x, S.ws->d, &res))) return rc;
	return ifaceInterp(g, L, S, res, y, false);
}

template <int OP> static int vop(te_vec *v, const te_vec *a, const te_vec *b, double alpha, double beta = 0, double gamma = 0)
{
	return vecop<OP>(v, a, b, alpha, beta, gamma);
}

// y = x - T x
static int applyS(te_gmg *g, LevelHost &L, SchurLevel &S, const te_vec *x, te_vec *y)
{
	int rc;
	if ((rc = applyT(g, L, S, x->d, y->d))) return rc;
	return vop<VOP_SCALE_THEN_ADD>(y, x, nullptr, -1.0); // y = -T x + x
}

// PolyChebPrec::apply (PolyChebPrec.cpp): Clenshaw over the Chebyshev series of 1 / (1 - t) on [0, interval]; with
// t = interval (1 + s) / 2, 1 / (1 - t) = 1 / (a - b s), a = 1 - interval / 2, b = interval / 2, whose coefficients have the
// closed form c_0 = 1 / r, c_k = 2 q^k / r (r = sqrt(a^2 - b^2), q = (a - r) / b); degree 15 as in the reference.
constexpr int    CHEB_TERMS    = 16;
constexpr double CHEB_INTERVAL = 0.95;
static void chebCoeffs(double *c)
{
	const double a = 1.0 - CHEB_INTERVAL / 2, b = CHEB_INTERVAL / 2, r = std::sqrt(a * a - b * b), q = (a - r) / b;
	c[0] = 1.0 / r;
	for (int k = 1; k < CHEB_TERMS; k++) c[k] = 2.0 * std::pow(q, k) / r;
}

static int applyCheb(te_gmg *g, LevelHost &L, SchurLevel &S, const te_vec *x, te_vec *y)
{
	int    rc;
	double c[CHEB_TERMS];
	chebCoeffs(c);
	te_vec *bk = S.iv[8], *bk1 = S.iv[9], *bk2 = S.iv[10];
	if ((rc = vop<VOP_SET>(bk1, nullptr, nullptr, 0.0)) || (rc = vop<VOP_SET>(bk2, nullptr, nullptr, 0.0))) return rc;
	for (int i = CHEB_TERMS - 1; i > 0; i--) {
		// bk = (4 / interval) T bk1 - 2 bk1 + c_i x - bk2
		if ((rc = applyT(g, L, S, bk1->d, bk->d)) || (rc = vop<VOP_SCALE_THEN_ADD_SCALED>(bk, bk1, nullptr, 4 / CHEB_INTERVAL, -2))
		    || (rc = vop<VOP_ADD_SCALED2>(bk, x, bk2, c[i], -1)))
			return rc;
		te_vec *tmp = bk2;
		bk2 = bk1, bk1 = bk, bk = tmp;
	}
	// y = (2 / interval) T bk1 - bk1 + c_0 x - bk2
	if ((rc = applyT(g, L, S, bk1->d, y->d)) || (rc = vop<VOP_SCALE_THEN_ADD_SCALED>(y, bk1, nullptr, 2 / CHEB_INTERVAL, -1))
	    || (rc = vop<VOP_ADD_SCALED2>(y, x, bk2, c[0], -1)))
		return rc;
	S.iv[8] = bk, S.iv[9] = bk1, S.iv[10] = bk2; // (the three rotate; keep every one owned)
	return TE_OK;
}

static int sdot(const te_vec *a, const te_vec *b, double *out) { return reduce<RED_DOT>(a, b, out); }

// BiCGStab.h:45-106 on S gamma = g, right-preconditioned (Mr = applyCheb when cheb); statement order of te_bicgstab
static int bicgstabS(te_gmg *g, LevelHost &L, SchurLevel &S, bool cheb, te_vec *x, const te_vec *b, int max_it, double tol, int *its_out,
                     double *rel_out)
{
	int     rc;
	te_vec *resid = S.iv[0], *rhat = S.iv[1], *p = S.iv[2], *ap = S.iv[3], *as = S.iv[4], *s = S.iv[5], *ms = S.iv[6], *mp = S.iv[7];
	auto    A = [&](const te_vec *in, te_vec *out) { return applyS(g, L, S, in, out); };
	auto    M = [&](const te_vec *in, te_vec *out) { return applyCheb(g, L, S, in, out); };
	double  r0sq, rho;
	if ((rc = A(x, resid)) || (rc = vop<VOP_SCALE_THEN_ADD>(resid, b, nullptr, -1.0)) || (rc = reduce<RED_SUMSQ>(resid, nullptr, &r0sq))
	    || (rc = vop<VOP_COPY>(rhat, resid, nullptr, 0)) || (rc = vop<VOP_COPY>(p, resid, nullptr, 0)) || (rc = sdot(rhat, resid, &rho)))
		return rc;
	const double r0 = std::sqrt(r0sq);
	double       rnorm = r0;
	int          its   = 0;
	while (r0 > 0 && rnorm / r0 > tol && its < max_it) {
		if (cheb) {
			if ((rc = M(p, mp)) || (rc = A(mp, ap))) return rc;
		} else if ((rc = A(p, ap))) {
			return rc;
		}
		double rap;
		if ((rc = sdot(rhat, ap, &rap))) return rc;
		const double alpha = rho / rap;
		if ((rc = vop<VOP_COPY>(s, resid, nullptr, 0)) || (rc = vop<VOP_ADD_SCALED>(s, ap, nullptr, -alpha))) return rc;
		if (cheb) {
			if ((rc = M(s, ms)) || (rc = A(ms, as))) return rc;
		} else if ((rc = A(s, as))) {
			return rc;
		}
		double num, den;
		if ((rc = sdot(as, s, &num)) || (rc = sdot(as, as, &den))) return rc;
		const double omega = num / den;
		if ((rc = vop<VOP_ADD_SCALED2>(x, cheb ? mp : p, cheb ? ms : s, alpha, omega))
		    || (rc = vop<VOP_ADD_SCALED2>(resid, ap, as, -alpha, -omega)))
			return rc;
		double rho_new, rsq;
		if ((rc = sdot(resid, rhat, &rho_new)) || (rc = reduce<RED_SUMSQ>(resid, nullptr, &rsq))) return rc;
		const double beta = rho_new * alpha / (rho * omega);
		if ((rc = vop<VOP_ADD_SCALED>(p, ap, nullptr, -omega)) || (rc = vop<VOP_SCALE_THEN_ADD>(p, resid, nullptr, beta))) return rc;
		its++;
		rho   = rho_new;
		rnorm = std::sqrt(rsq);
	}
	if (its_out) *its_out = its;
	if (rel_out) *rel_out = r0 > 0 ? rnorm / r0 : 0.0;
	return TE_OK;
}

// common checks of the entry points; *L, *S on success
static int enter(te_gmg *g, int level, const char *who, LevelHost **L, SchurLevel **S)
{
	if (!g || level < 0 || level >= (int) g->levels.size()) return te::fail(TE_EINVAL, std::string(who) + ": bad level");
	int rc = coefRefuse(g, who); // (the Schur route's patch solves invert the constant-coefficient patch operator)
	if (rc || (rc = schurLevel(g, level, S))) return rc;
	*L = g->levels[level].get();
	(*L)->xf_valid_for = nullptr; // (the level's scratch is rewritten)
	return TE_OK;
}
} // namespace tei

extern "C" {
int te_iface_interp(te_gmg *g, int level, const te_vec *u, te_vec *gamma)
{
	return guarded([&]() -> int {
		LevelHost  *L;
		SchurLevel *S;
		int         rc;
		if ((rc = enter(g, level, "te_iface_interp", &L, &S)) || (rc = checkLevelVec(g, level, u, "te_iface_interp"))
		    || (rc = checkIface(g, level, gamma, "te_iface_interp")))
			return rc;
		return ifaceInterp(g, *L, *S, u->d, gamma->d, false);
	});
}

int te_apply_with_interface(te_gmg *g, int level, const te_vec *u, const te_vec *gamma, te_vec *f)
{
	return guarded([&]() -> int {
		LevelHost  *L;
		SchurLevel *S;
		int         rc;
		if ((rc = enter(g, level, "te_apply_with_interface", &L, &S)) || (rc = checkLevelVec(g, level, u, "te_apply_with_interface"))
		    || (rc = checkIface(g, level, gamma, "te_apply_with_interface")) || (rc = checkLevelVec(g, level, f, "te_apply_with_interface")))
			return rc;
		if (u == f) return te::fail(TE_EINVAL, "te_apply_with_interface: in-place apply is not supported");
		// the patch operator (neighbour faces closed as homogeneous Dirichlet), then + 2 gamma / h^2 on the face layers
		rc = launchStencil<MODE_APPLY>(g, *L, u->d, nullptr, f->d, 0.0, RestrictDst(), nullptr, RED_NONE, nullptr, nullptr, true);
		if (rc || (rc = ifaceCorr(g, *L, *S, gamma->d))) return rc;
		return ifaceRhs(g, *L, *S, f->d, f->d, true);
	});
}

int te_add_iface_rhs(te_gmg *g, int level, const te_vec *gamma, te_vec *f)
{
	return guarded([&]() -> int {
		LevelHost  *L;
		SchurLevel *S;
		int         rc;
		if ((rc = enter(g, level, "te_add_iface_rhs", &L, &S)) || (rc = checkIface(g, level, gamma, "te_add_iface_rhs"))
		    || (rc = checkLevelVec(g, level, f, "te_add_iface_rhs")) || (rc = ifaceCorr(g, *L, *S, gamma->d)))
			return rc;
		return ifaceRhs(g, *L, *S, f->d, f->d, false);
	});
}

int te_solve_with_interface(te_gmg *g, int level, const te_vec *f, te_vec *u, const te_vec *gamma, te_vec *diff)
{
	return guarded([&]() -> int {
		LevelHost  *L;
		SchurLevel *S;
		int         rc;
		if ((rc = enter(g, level, "te_solve_with_interface", &L, &S)) || (rc = checkLevelVec(g, level, f, "te_solve_with_interface"))
		    || (rc = checkLevelVec(g, level, u, "te_solve_with_interface")) || (rc = checkIface(g, level, gamma, "te_solve_with_interface"))
		    || (diff && (rc = checkIface(g, level, diff, "te_solve_with_interface"))))
			return rc;
		if (u == f) return te::fail(TE_EINVAL, "te_solve_with_interface: u and f must be different vectors");
		if (diff == gamma) return te::fail(TE_EINVAL, "te_solve_with_interface: diff and gamma must be different vectors");
		const double *res;
		if ((rc = solveWith(g, *L, *S, f->d, gamma->d, u->d, &res))) return rc;
		if (res != u->d && u->n) HIPCHK(hipMemcpyAsync(u->d, res, sizeof(double) * u->n, hipMemcpyDeviceToDevice, g->stream));
		if (!diff) return TE_OK;
		if ((rc = ifaceInterp(g, *L, *S, u->d, diff->d, false))) return rc;
		return vop<VOP_ADD_SCALED>(diff, gamma, nullptr, -1.0);
	});
}

int te_schur_apply(te_gmg *g, int level, const te_vec *x, te_vec *y)
{
	return guarded([&]() -> int {
		LevelHost  *L;
		SchurLevel *S;
		int         rc;
		if ((rc = enter(g, level, "te_schur_apply", &L, &S)) || (rc = checkIface(g, level, x, "te_schur_apply"))
		    || (rc = checkIface(g, level, y, "te_schur_apply")))
			return rc;
		if (x == y) return te::fail(TE_EINVAL, "te_schur_apply: x and y must be different vectors");
		return applyS(g, *L, *S, x, y);
	});
}

int te_schur_cheb(te_gmg *g, int level, const te_vec *x, te_vec *y)
{
	return guarded([&]() -> int {
		LevelHost  *L;
		SchurLevel *S;
		int         rc;
		if ((rc = enter(g, level, "te_schur_cheb", &L, &S)) || (rc = checkIface(g, level, x, "te_schur_cheb"))
		    || (rc = checkIface(g, level, y, "te_schur_cheb")))
			return rc;
		if (x == y) return te::fail(TE_EINVAL, "te_schur_cheb: x and y must be different vectors");
		return applyCheb(g, *L, *S, x, y);
	});
}

int te_schur_solve(te_gmg *g, int level, int prec, const te_vec *f, te_vec *u, te_vec *gamma, int max_it, double tol, int *iterations,
                   double *rel_resid)
{
	return guarded([&]() -> int {
		LevelHost  *L;
		SchurLevel *S;
		int         rc;
		if ((rc = enter(g, level, "te_schur_solve", &L, &S)) || (rc = checkLevelVec(g, level, f, "te_schur_solve"))
		    || (rc = checkLevelVec(g, level, u, "te_schur_solve")) || (rc = checkIface(g, level, gamma, "te_schur_solve")))
			return rc;
		if (u == f) return te::fail(TE_EINVAL, "te_schur_solve: u and f must be different vectors");
		if (prec != TE_SCHUR_PREC_NONE && prec != TE_SCHUR_PREC_CHEB) return te::fail(TE_EINVAL, "te_schur_solve: unknown preconditioner");
		int    its = 0;
		double rel = 0.0;
		if (L->nif > 0) {
			// g = Interp(Solve(f, 0))
			te_vec       *b = S->iv[11];
			const double *res;
			if ((rc = solveWith(g, *L, *S, f->d, nullptr, S->ws->d, &res)) || (rc = ifaceInterp(g, *L, *S, res, b->d, false))) return rc;
			if ((rc = bicgstabS(g, *L, *S, prec == TE_SCHUR_PREC_CHEB, gamma, b, max_it, tol, &its, &rel))) return rc;
		}
		const double *res;
		if ((rc = solveWith(g, *L, *S, f->d, L->nif > 0 ? gamma->d : nullptr, u->d, &res))) return rc;
		if (res != u->d && u->n) HIPCHK(hipMemcpyAsync(u->d, res, sizeof(double) * u->n, hipMemcpyDeviceToDevice, g->stream));
		HIPCHK(hipStreamSynchronize(g->stream));
		if (iterations) *iterations = its;
		if (rel_resid) *rel_resid = rel;
		return TE_OK;
	});
}
} // extern "C"
