// Level tables on the device, solver and vector life cycle, options, profiling, Init kernels (see gmg_internal.hpp).
#include "gmg_internal.hpp"

namespace tei
{
const char *kclassName[KC_COUNT] = {"stencil_apply", "stencil_resid", "stencil_jacobi", "stencil_rbgs",
                                    "cf_ghost", "restrict", "prolong_add", "patch_rhs", "dst_axis",
                                    "vecop", "reduce", "pack", "exchange", "stencil_rbgs_zero", "resid_restrict", "patch_solve_mfma", "stencil_rbgs_prolong",
                                    "stencil_rbgs_slabs", "stencil_slabs", "patch_solve_3pass", "rbgs_zero_resid_restrict",
                                    "restrict_fixup", "rbgs_resweep_prolong", "rbgs_zero_resid_restrict_faces",
                                    "rbgs_resweep_prolong_fcorr", "rbgs_zero_resid_restrict_faces_fcorr", "fcorr_gather", "patch_solve_mfma_faces",
                                    "bicg_update", "bicg_s", "bicg_p", "stencil_apply_dot", "patch_bcgs", "gradient", "divergence", "project", "prolong_linear", "prolong_quadratic", "boundary_restrict",
                                    "indicator", "regrid", "regrid_faces",
                                    "apply_coef", "resid_coef", "jacobi_coef", "rbgs_coef", "faces_restrict",
                                    "coef_split", "coef_merge",
                                    "faces_from_cells", "project_weighted", "boundary_rhs_w",
                                    "advect_flux", "advect", "faces_match", "faces_max_rate",
                                    "cell_slopes", "advect_flux_muscl", "advect_muscl"};
const char *optName[O_COUNT] = {"TE_2D_SIMPLE", "TE_2D_NO_MFMA", "TE_2D_NO_PF", "TE_2D_NO_MR_FUSE", "TE_2D_TPB", "TE_NO_FUSE2", "TE_NO_FUSE3",
                                "TE_NO_FUSE3_CF", "TE_NO_CFP", "TE_NO_XF", "TE_NO_FCORR", "TE_NO_FCORR_CF", "TE_NO_OVERLAP",
                                "TE_OVERLAP_MIN", "TE_NO_PS_FACES", "TE_PS_MODE", "TE_PS_SLOW", "TE_RBGS_NOSLAB", "TE_ZS_FORCE", "TE_NO_ZS8",
                                "TE_RESWEEP_V", "TE_EXCHANGE_TIMEOUT", "TE_NO_VERIFY", "TE_RCCL_LOOPBACK", "TE_NO_BICG_FUSE", "TE_POST_EXCHANGE", "TE_REPL_BLOCKS", "TE_PACK_FACES", "TE_OVERLAP_MODE", "TE_PUSH_TIMEOUT", "TE_NO_BICG_XF", "TE_PUSH_FAULT", "TE_2D_NO_FOLD", "TE_2D_NO_SYM", "TE_PUSH_NONFATAL", "TE_PS_NO_HALF", "TE_PS_HALF_MAX", "TE_NO_RS6_CF", "TE_NO_RS6_FIXUP", "TE_SCHUR_FULL", "TE_ZS_PIN"};

void drainEvents(te_gmg *g)
{
	if (g->ev_used == 0) return;
	(void) hipStreamSynchronize(g->stream);
	for (size_t i = 0; i < g->ev_used; i++) {
		float ms = 0;
		if (g->ev_pool[i].valid && hipEventElapsedTime(&ms, g->ev_pool[i].a, g->ev_pool[i].b) == hipSuccess) {
			g->calls[g->ev_pool[i].kc]++;
			g->total_ms[g->ev_pool[i].kc] += ms;
		}
	}
	g->ev_used = 0;
}

void Cfg::fromEnv()
{
	for (int o = 0; o < O_COUNT; o++) set(o, getenv(optName[o]));
}

// the value of TE_ZS_PIN: "1", "2", "4" or "8" and nothing else (0: not one of them)
static int parseSlabPin(const char *v)
{
	if (!v || !v[0] || v[1]) return 0;
	const int pin = v[0] - '0';
	return slabPinValid(pin) ? pin : 0;
}

// the value of TE_RESWEEP_V: "19", "27" or "59" and nothing else (0: not one of them)
static int parseResweepPin(const char *v)
{
	if (!v || !v[0] || !v[1] || v[2]) return 0;
	const int pin = (v[0] - '0') * 10 + (v[1] - '0');
	return resweepPinValid(pin) ? pin : 0;
}

// places the tables of level li (level_tables.cpp) on the device; the order of the allocations is part of the set-up's behaviour
int buildLevel(te_gmg *g, const Hierarchy &H, int li)
{
	const int n = H.levels[li].n, D = H.levels[li].dim;
	if (D == 3 && n != 4 && n != 8 && n != 16 && n != 32)
		return te::fail(TE_EUNSUPPORTED, "te_gmg_create: 3D patches must have n = 4, 8, 16 or 32 cells per axis");
	if (D == 2 && (n < 4 || (n & 1))) return te::fail(TE_EUNSUPPORTED, "te_gmg_create: 2D patches need an even n >= 4");
	LevelBuildOpts o;
	o.simple_2d     = g->cfg.has(O_2D_SIMPLE);
	o.no_cfp        = g->cfg.has(O_NO_CFP);
	o.no_mr_fuse_2d = g->cfg.has(O_2D_NO_MR_FUSE);
	LevelTables T;
	int         rc;
	if ((rc = computeLevelTables(H, li, o, T))) return rc;

	auto L = std::make_unique<LevelHost>();
	L->index = li;
	L->dim = T.dim, L->n = T.n, L->P = T.P, L->P_global = T.P_global, L->nc = T.nc, L->nf = T.nf;
	L->replicated = T.replicated, L->gathered = T.gathered;
	L->nif = T.nif, L->if_own = std::move(T.if_own), L->if_start = std::move(T.if_start), L->if_contrib = std::move(T.if_contrib);
	L->nbf = T.nbf, L->bface_host = std::move(T.bface), L->brestrict_host = std::move(T.brestrict);
	L->fx = std::move(T.fx), L->nremote = T.nremote;
	L->nslots = T.nslots, L->ncf = T.ncf, L->n_int = T.n_int, L->n_bnd = T.n_bnd;
	L->lds2d = T.lds2d, L->fuse2d = T.fuse2d, L->fuse2_ok = T.fuse2_ok;
	L->patch_vol = std::move(T.patch_vol);
	L->sym_ok = T.sym_ok, L->n_pure = T.n_pure, L->n_pure2 = T.n_pure2;
	L->Pc = T.Pc, L->n_up = T.n_up, L->n_down = T.n_down;
	L->tx_up = std::move(T.tx_up), L->tx_down = std::move(T.tx_down), L->tx_direct = std::move(T.tx_direct);
	L->prolong_fusable = T.prolong_fusable, L->prolong_fusable_cf = T.prolong_fusable_cf, L->has_copy = T.has_copy;
	L->repl_up = T.repl_up, L->repl_direct = T.repl_direct, L->post_exchange_free = T.post_exchange_free;
	L->tx_fup = std::move(T.tx_fup), L->up_foff_host = std::move(T.up_foff), L->down_foff_host = std::move(T.down_foff);
	L->up_ftotal = T.up_ftotal, L->down_ftotal = T.down_ftotal;

	// (an empty table allocates nothing)
	const size_t P1 = (size_t) std::max(T.P, 1), nf = T.nf;
	const bool   fused3d = (D == 3 && T.fuse2_ok && T.P > 0);
	if ((rc = L->send_faces.upload(T.send_faces)) || (rc = L->sendbuf.alloc((size_t) std::max(T.nremote, 1) * nf))
	    || (rc = L->f6off.upload(T.f6off)) || (rc = L->order.upload(T.order)))
		return rc;
	if (D == 3 && ((rc = L->xfbuf[0].alloc(P1 * 2 * nf)) || (rc = L->xfbuf[1].alloc(P1 * 2 * nf)) || (rc = L->f6buf.alloc(P1 * 6 * nf))))
		return rc;
	if (fused3d && li > 0) { // a level that can read its right-hand side with FCORR
		if ((rc = L->fcorr.alloc((size_t) T.P * 4 * nf))) return rc;
		HIPCHK(hipMemset(L->fcorr.p, 0, sizeof(double) * L->fcorr.n));
	}
	if (fused3d && (rc = L->rs6.alloc((size_t) T.P * 6 * nf / 4))) return rc;
	if ((rc = L->geom_starts.upload(T.geom_starts)) || (rc = L->geom_h.upload(T.geom_h)) || (rc = L->node_ids.upload(T.node_ids))
	    || (rc = L->cellvol.upload(T.cellvol)) || (rc = L->face_kind_patch.upload(T.face_kind_patch))
	    || (rc = L->face_kind.upload(T.face_kind)) || (rc = L->face_src.upload(T.face_src)) || (rc = L->face_kadj.upload(T.face_kadj))
	    || (rc = L->rh2.upload(T.rh2)) || (rc = L->cf_desc.upload(T.cf_desc)) || (rc = L->cf_slots.upload(T.cf_slots))
	    || (rc = L->ghost.alloc((size_t) std::max(T.nslots, 1) * nf)))
		return rc;
	// patch solve
	if ((rc = L->matfrag.upload(T.matfrag)) || (rc = L->matsym.upload(T.matsym)) || (rc = L->matsT.upload(T.matsT))
	    || (rc = L->psinv.upload(T.psinv)) || (rc = L->psitab.upload(T.psitab)) || (rc = L->ps_list.upload(T.ps_list))
	    || (rc = L->mat2sym.upload(T.mat2sym)) || (rc = L->ps2_list.upload(T.ps2_list))
	    || (rc = L->corr.alloc(P1 * 2 * D * nf)) || (rc = L->plan.upload(T.plan)) || (rc = L->mats.upload(T.mats))
	    || (rc = L->lam.upload(T.lam)) || (rc = L->zero_mode.upload(T.zero_mode)))
		return rc;
	// transfers to level li + 1
	if (T.coarser
	    && ((D == 2 && T.fuse2_ok && (rc = L->e4buf.alloc(P1 * 4 * n))) || (rc = L->slot_parent.upload(T.slot_parent))
	        || (rc = L->slot_orth.upload(T.slot_orth)) || (rc = L->bc_desc.upload(T.bc_desc)) || (rc = L->cbase.upload(T.cbase))
	        || (rc = L->parent.upload(T.parent)) || (rc = L->orth.upload(T.orth)) || (rc = L->child.upload(T.child))
	        || (rc = L->copy.upload(T.copy)) || (rc = L->up_desc.upload(T.up_desc)) || (rc = L->down_desc.upload(T.down_desc))
	        || (rc = L->up_off.upload(T.up_off)) || (rc = L->down_off.upload(T.down_off))
	        || (rc = L->upbuf.alloc((size_t) std::max<int64_t>(T.up_total, 1)))
	        || (rc = L->downbuf.alloc((size_t) std::max<int64_t>(T.down_total, 1)))))
		return rc;
	g->levels.push_back(std::move(L));
	return TE_OK;
}

int newVec(te_gmg *g, int level, te_vec **out)
{
	LevelHost &L = *g->levels[level];
	auto       v = new te_vec;
	v->g         = g;
	v->level     = level;
	v->n         = (size_t) L.P * L.nc;
	hipError_t e = hipMalloc(&v->d, sizeof(double) * std::max<size_t>(v->n, 2));
	if (e != hipSuccess) {
		delete v;
		return te::fail(TE_EHIP, std::string("hipMalloc(vector): ") + hipGetErrorString(e));
	}
	e = hipMemsetAsync(v->d, 0, sizeof(double) * v->n, g->stream);
	if (e != hipSuccess) {
		(void) hipFree(v->d);
		delete v;
		return te::fail(TE_EHIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
	}
	*out = v;
	return TE_OK;
}

} // namespace tei

extern "C" {
void te_cycle_opts_default(te_cycle_opts *o)
{
	if (!o) return;
	o->pre_sweeps = o->post_sweeps = o->coarse_sweeps = o->mid_sweeps = 1; // CycleOpts.h:64-79
	o->cycle_type   = 0;
	o->smoother     = TE_SMOOTH_PATCH_SOLVE;
	o->omega        = 6.0 / 7.0;
	o->exact_coarse = 1;
	o->fuse         = 3;
}

int te_gmg_create(const te_hier *h, int device, te_gmg **out)
{
	return guarded([&]() -> int { return tei::gmgCreate(h, device, nullptr, out); });
}
} // extern "C"

namespace tei
{
int gmgCreate(const te_hier *h, int device, hipStream_t borrowed, te_gmg **out)
{
	return guarded([&]() -> int {
		if (!h || !out) return te::fail(TE_EINVAL, "te_gmg_create: null argument");
		using clk = std::chrono::steady_clock;
		auto ms   = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
		const auto t_begin = clk::now();
		SetupAcc   acc;
		struct AccScope { // (the allocations and uploads of THIS call, whichever way it ends)
			explicit AccScope(SetupAcc *a) { g_setup_acc = a; }
			~AccScope() { g_setup_acc = nullptr; }
		} acc_scope(&acc);
		int ndev = 0;
		if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
			return te::fail(TE_EHIP, "te_gmg_create: no HIP device visible (this library has no CPU fallback)");
		if (device < 0) HIPCHK(hipGetDevice(&device));
		HIPCHK(hipSetDevice(device));
		auto g    = std::make_unique<te_gmg>();
		g->device = device;
		g->dim    = h->h.dim;
		g->n      = h->h.n;
		g->rank   = h->h.rank;
		g->nranks = h->h.nranks;
		g->placement[0] = h->h.agglomerate, g->placement[1] = h->h.agglomerate_max, g->placement[2] = h->h.replicate;
		g->placement[3] = (double) h->h.levels.size();
		g->placement[4] = (double) h->h.neumann_sides;
		g->leaf_id = h->h.leaf_id, g->leaf_parent = h->h.leaf_parent, g->leaf_orth = h->h.leaf_orth;
		g->leaf_starts = h->h.levels[0].g_starts, g->leaf_lengths = h->h.levels[0].g_lengths;
		g->coarse_P_global = h->h.levels.back().P_global;
		g->coarse_starts = h->h.levels.back().g_starts, g->coarse_lengths = h->h.levels.back().g_lengths;
		memset(g->calls, 0, sizeof(g->calls));
		memset(g->cells, 0, sizeof(g->cells));
		memset(g->total_ms, 0, sizeof(g->total_ms));
		g->cfg.fromEnv();
		if (g->cfg.has(O_ZS_PIN) && !(g->zs_pin = parseSlabPin(g->cfg.str(O_ZS_PIN)))) // (before the solver owns anything)
			return te::fail(TE_EINVAL, "te_gmg_create: TE_ZS_PIN must be 1, 2, 4 or 8");
		if (g->cfg.has(O_RESWEEP_V) && !(g->resweep_pin = parseResweepPin(g->cfg.str(O_RESWEEP_V))))
			return te::fail(TE_EINVAL, "te_gmg_create: TE_RESWEEP_V must be 19, 27 or 59");
		if (borrowed)
			g->stream = borrowed, g->stream_borrowed = true;
		else
			HIPCHK(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
		HIPCHK(hipStreamCreateWithFlags(&g->comm_stream, hipStreamNonBlocking));
		HIPCHK(hipEventCreateWithFlags(&g->ev_pack, hipEventDisableTiming));
		HIPCHK(hipEventCreateWithFlags(&g->ev_recv, hipEventDisableTiming));
		g->overlap = !g->cfg.has(O_NO_OVERLAP);
		const auto t_ctx = clk::now();
		int rc;
		for (int li = 0; li < (int) h->h.levels.size(); li++)
			if ((rc = buildLevel(g.get(), h->h, li))) return rc;
		const auto     t_levels = clk::now();
		const SetupAcc acc_levels = acc;
		{ // partial sums: the reduction kernels' blocks, or one pair per work item of a stencil launch with fused sums. A 3D level
			// gets room for the largest slab count its patch size admits (dispatch.hpp maxSlabs), whatever the rule gives it now:
			// no switch set later (TE_ZS_FORCE, TE_ZS_PIN) can ask for more
			size_t items = (size_t) g->red_blocks;
			for (auto &L : g->levels)
				if (L->dim == 3) items = std::max(items, (size_t) L->P * maxSlabs(L->n));
			// 2D: one pair per workgroup of k_stencil2d's FLAT grid (one x-pair per thread: a capped grid-stride loop streams a third
			// slower on this chip and cost the fused sums more than the passes they replace)
			for (auto &L : g->levels)
				if (L->dim == 2) items = std::max(items, ((size_t) L->P * L->nc / 2 + 255) / 256);
			if ((rc = g->partial.alloc(2 * items)) || (rc = g->result.alloc(8))) return rc;
		}
		HIPCHK(hipHostMalloc((void **) &g->result_host, 8 * sizeof(double), hipHostMallocDefault));
		for (int li = 0; li < (int) g->levels.size(); li++) {
			LevelHost &L = *g->levels[li];
			te_vec    *v;
			if ((rc = newVec(g.get(), li, &v))) return rc;
			L.r.reset(v);
			if ((rc = newVec(g.get(), li, &v))) return rc;
			L.t.reset(v);
			if (li > 0) {
				if ((rc = newVec(g.get(), li, &v))) return rc;
				L.u.reset(v);
				if ((rc = newVec(g.get(), li, &v))) return rc;
				L.f.reset(v);
			}
		}
		const auto t_vecs = clk::now();
		HIPCHK(hipStreamSynchronize(g->stream));
		const auto t_end = clk::now();
		g->setup_ms[0]   = ms(t_begin, t_ctx);
		g->setup_ms[1]   = ms(t_ctx, t_levels) - acc_levels.malloc_ms - acc_levels.copy_ms;
		g->setup_ms[2]   = acc.malloc_ms;
		g->setup_ms[3]   = acc.nmalloc;
		g->setup_ms[4]   = acc.copy_ms;
		g->setup_ms[5]   = ms(t_levels, t_vecs) - (acc.malloc_ms - acc_levels.malloc_ms) - (acc.copy_ms - acc_levels.copy_ms);
		g->setup_ms[6]   = ms(t_vecs, t_end);
		g->setup_ms[7]   = ms(t_begin, t_end);
		*out = g.release();
		return TE_OK;
	});
}
} // namespace tei

extern "C" {
int te_gmg_setup_ms(const te_gmg *g, double *out, int n)
{
	return guarded([&]() -> int {
		if (!g || !out || n < 0) return te::fail(TE_EINVAL, "te_gmg_setup_ms: bad argument");
		for (int i = 0; i < std::min(n, 8); i++) out[i] = g->setup_ms[i];
		return TE_OK;
	});
}

void te_gmg_destroy(te_gmg *g)
{
	if (!g) return;
	watchdogStop(g);
	(void) hipStreamSynchronize(g->stream);
	if (g->comm_stream) (void) hipStreamSynchronize(g->comm_stream);
	pushTeardown(g, true); // (the coarse vectors get their own storage back before they are freed below)
	for (auto &L : g->levels) {
		for (te_vec *v : {L->u.get(), L->f.get(), L->r.get(), L->t.get()})
			if (v && v->d) (void) hipFree(v->d);
	}
	for (te_vec *v : g->bicg_work)
		if (v) te_vec_destroy(v);
	fmgFree(g);
	schurFree(g);
	regridFree(g);
	coefCoarseFree(g); // (the auxiliary solver runs on this solver's stream: it goes first)
	coefFree(g);
	for (auto &e : g->ev_pool) {
		(void) hipEventDestroy(e.a);
		(void) hipEventDestroy(e.b);
	}
	if (g->rccl.comm && g->rccl.CommDestroy) (void) g->rccl.CommDestroy(g->rccl.comm);
	if (g->result_host) (void) hipHostFree(g->result_host);
	if (g->ev_pack) (void) hipEventDestroy(g->ev_pack);
	if (g->ev_recv) (void) hipEventDestroy(g->ev_recv);
	if (g->comm_stream) (void) hipStreamDestroy(g->comm_stream);
	if (!g->stream_borrowed) (void) hipStreamDestroy(g->stream);
	delete g;
}

int   te_gmg_num_levels(const te_gmg *g) { return guarded([&]() -> int { return g ? (int) g->levels.size() : TE_EINVAL; }); }

int   te_gmg_sync(te_gmg *g)
{
	return guarded([&]() -> int {
		if (!g) return te::fail(TE_EINVAL, "te_gmg_sync: null");
		HIPCHK(hipStreamSynchronize(g->stream));
		return TE_OK;
	});
}

void *te_gmg_stream(te_gmg *g) { return g ? (void *) g->stream : nullptr; }

int te_vec_create(te_gmg *g, int level, te_vec **out)
{
	return guarded([&]() -> int {
		if (!g || !out || level < 0 || level >= (int) g->levels.size())
			return te::fail(TE_EINVAL, "te_vec_create: bad argument");
		HIPCHK(hipSetDevice(g->device));
		return newVec(g, level, out);
	});
}

int te_vec_create_iface(te_gmg *g, int level, te_vec **out)
{
	return guarded([&]() -> int {
		if (!g || !out || level < 0 || level >= (int) g->levels.size())
			return te::fail(TE_EINVAL, "te_vec_create_iface: bad argument");
		LevelHost &L = *g->levels[level];
		if (g->nranks > 1 || L.nif < 0) return te::fail(TE_ESTATE, "te_vec_create_iface: interface vectors exist on single-rank hierarchies only");
		HIPCHK(hipSetDevice(g->device));
		auto v   = std::make_unique<te_vec>();
		v->g     = g;
		v->level = level;
		v->iface = true;
		v->n     = (size_t) L.nif * L.nf;
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

void te_vec_destroy(te_vec *v)
{
	if (!v) return;
	(void) hipStreamSynchronize(v->g->stream);
	(void) hipFree(v->d);
	delete v;
}

size_t te_vec_size(const te_vec *v) { return v ? v->n : 0; }

int    te_vec_upload(te_vec *v, const double *host)
{
	return guarded([&]() -> int {
		if (!v || !host) return te::fail(TE_EINVAL, "te_vec_upload: null");
		HIPCHK(hipMemcpyAsync(v->d, host, sizeof(double) * v->n, hipMemcpyHostToDevice, v->g->stream));
		HIPCHK(hipStreamSynchronize(v->g->stream));
		return TE_OK;
	});
}

int te_vec_download(const te_vec *v, double *host)
{
	return guarded([&]() -> int {
		if (!v || !host) return te::fail(TE_EINVAL, "te_vec_download: null");
		HIPCHK(hipMemcpyAsync(host, v->d, sizeof(double) * v->n, hipMemcpyDeviceToHost, v->g->stream));
		HIPCHK(hipStreamSynchronize(v->g->stream));
		return TE_OK;
	});
}

void *te_vec_device_ptr(te_vec *v) { return v ? v->d : nullptr; }

// Init::initDirichlet / initNeumann for the drivers' canned problems, on the device (initkernels.hpp)
int te_init_problem(te_gmg *g, int level, int problem, int neumann, te_vec *f, te_vec *exact)
{
	return guarded([&]() -> int {
		int rc;
		if ((rc = checkLevelVec(g, level, f, "te_init_problem"))) return rc;
		if (exact && (rc = checkLevelVec(g, level, exact, "te_init_problem"))) return rc;
		if (exact == f) return te::fail(TE_EINVAL, "te_init_problem: f and exact must be different vectors");
		LevelHost &L = *g->levels[level];
		if (L.xf_valid_for == f->d || (exact && L.xf_valid_for == exact->d)) L.xf_valid_for = nullptr;
		if (L.P == 0) return TE_OK;
		InitGeom G;
		G.dim = L.dim, G.n = L.n, G.P = L.P;
		G.starts = L.geom_starts.p, G.h = L.geom_h.p, G.face_kind = L.face_kind.p, G.ids = L.node_ids.p;
		const dim3 grid(gridFor(f->n, 256, 1 << 20)), blk(256);
		double    *e = exact ? exact->d : nullptr;
		Timed      t(g, KC_VECOP, f->n);
#define TE_INIT(K, PROB)                                                                              \
		if (neumann)                                                                                      \
			hipLaunchKernelGGL((K<PROB, 1>), grid, blk, 0, g->stream, G, f->d, e);                     \
		else                                                                                              \
			hipLaunchKernelGGL((K<PROB, 0>), grid, blk, 0, g->stream, G, f->d, e);
		if (problem == PROBLEM_RANDOM) {
			hipLaunchKernelGGL(k_init_random, grid, blk, 0, g->stream, G, L.nc, (uint64_t) 0x5EED, f->d, e);
		} else if (problem == PROBLEM_TRIG) {
			if (L.dim == 3) {
				TE_INIT(k_init3d, PROBLEM_TRIG)
			} else {
				TE_INIT(k_init2d, PROBLEM_TRIG)
			}
		} else if (problem == PROBLEM_GAUSS) {
			if (L.dim == 3) {
				TE_INIT(k_init3d, PROBLEM_GAUSS)
			} else {
				TE_INIT(k_init2d, PROBLEM_GAUSS)
			}
		} else {
			return te::fail(TE_EINVAL, "te_init_problem: unknown problem");
		}
#undef TE_INIT
		HIPCHK(hipGetLastError());
		return TE_OK;
	});
}

// Vector<D>::getLocalData(i) for a run of patches (PetscVector.h:87-98): what Init::initDirichlet, the writers and
// the C++ adaptor's host mirror move -- never the whole vector for one patch.
int te_vec_upload_patches(te_vec *v, int first_patch, int npatches, const double *host)
{
	return guarded([&]() -> int {
		if (!v || !host) return te::fail(TE_EINVAL, "te_vec_upload_patches: null");
		const size_t nc = vecBlock(v);
		if (first_patch < 0 || npatches < 0 || ((size_t) first_patch + npatches) * nc > v->n)
			return te::fail(TE_EINVAL, "te_vec_upload_patches: patch range outside the vector");
		if (npatches == 0) return TE_OK;
		LevelHost &L = *v->g->levels[v->level];
		if (L.xf_valid_for == v->d) L.xf_valid_for = nullptr;
		HIPCHK(hipMemcpyAsync(v->d + (size_t) first_patch * nc, host, sizeof(double) * nc * npatches, hipMemcpyHostToDevice, v->g->stream));
		HIPCHK(hipStreamSynchronize(v->g->stream));
		return TE_OK;
	});
}

int te_vec_download_patches(const te_vec *v, int first_patch, int npatches, double *host)
{
	return guarded([&]() -> int {
		if (!v || !host) return te::fail(TE_EINVAL, "te_vec_download_patches: null");
		const size_t nc = vecBlock(v);
		if (first_patch < 0 || npatches < 0 || ((size_t) first_patch + npatches) * nc > v->n)
			return te::fail(TE_EINVAL, "te_vec_download_patches: patch range outside the vector");
		if (npatches == 0) return TE_OK;
		HIPCHK(hipMemcpyAsync(host, v->d + (size_t) first_patch * nc, sizeof(double) * nc * npatches, hipMemcpyDeviceToHost, v->g->stream));
		HIPCHK(hipStreamSynchronize(v->g->stream));
		return TE_OK;
	});
}

int te_gmg_profile(te_gmg *g, int enable)
{
	return guarded([&]() -> int {
		if (!g) return te::fail(TE_EINVAL, "te_gmg_profile: null");
		drainEvents(g);
		g->profiling = enable != 0;
		if (g->cc_aux) return te_gmg_profile(g->cc_aux, enable); // (the sub-patch coarse solve's launches are part of this solver's cycle)
		return TE_OK;
	});
}

int te_integrate(te_gmg *g, int level, const te_vec *v, double *out)
{
	return guarded([&]() -> int {
		int rc;
		if (!out) return te::fail(TE_EINVAL, "te_integrate: null result");
		if ((rc = checkLevelVec(g, level, v, "te_integrate"))) return rc;
		LevelHost &L = *g->levels[level];
		*out         = 0.0;
		if (L.P == 0 || (L.replicated && g->rank != 0)) return TE_OK; // (a level on every rank counts once: rank 0's)
		DevBuf<double> part;
		if ((rc = part.alloc(L.P))) return rc;
		hipLaunchKernelGGL(k_patch_integrals, dim3(L.P), dim3(256), 0, g->stream, (int) L.nc, v->d, L.cellvol.p, part.p);
		HIPCHK(hipGetLastError());
		std::vector<double> h(L.P);
		HIPCHK(hipMemcpyAsync(h.data(), part.p, sizeof(double) * L.P, hipMemcpyDeviceToHost, g->stream));
		HIPCHK(hipStreamSynchronize(g->stream));
		double sum = 0.0;
		for (double x : h) sum += x; // patch order, as the reference's loop over its patch map
		*out = sum;
		return TE_OK;
	});
}

int te_volume(te_gmg *g, int level, double *out)
{
	return guarded([&]() -> int {
		if (!g || !out || level < 0 || level >= (int) g->levels.size()) return te::fail(TE_EINVAL, "te_volume: bad argument");
		double sum = 0.0;
		if (!(g->levels[level]->replicated && g->rank != 0)) // (a level on every rank counts once: rank 0's)
			for (double x : g->levels[level]->patch_vol) sum += x;
		*out = sum;
		return TE_OK;
	});
}

int te_gmg_profile_select(te_gmg *g, const char *name)
{
	return guarded([&]() -> int {
		if (!g) return te::fail(TE_EINVAL, "te_gmg_profile_select: null");
		drainEvents(g);
		g->prof_only = -1;
		if (g->cc_aux) drainEvents(g->cc_aux), g->cc_aux->prof_only = -1;
		if (!name || !*name) return TE_OK;
		for (int k = 0; k < KC_COUNT; k++)
			if (!strcmp(name, kclassName[k])) {
				g->prof_only = k;
				if (g->cc_aux) g->cc_aux->prof_only = k;
				return TE_OK;
			}
		return te::fail(TE_EINVAL, std::string("te_gmg_profile_select: unknown kernel class ") + name);
	});
}

int te_gmg_profile_stride(te_gmg *g, int stride)
{
	return guarded([&]() -> int {
		if (!g) return te::fail(TE_EINVAL, "te_gmg_profile_stride: null");
		drainEvents(g);
		g->prof_stride = stride > 1 ? stride : 1;
		memset(g->prof_seq, 0, sizeof(g->prof_seq));
		if (g->cc_aux) return te_gmg_profile_stride(g->cc_aux, stride);
		return TE_OK;
	});
}

int te_gmg_profile_reset(te_gmg *g)
{
	return guarded([&]() -> int {
		if (!g) return te::fail(TE_EINVAL, "te_gmg_profile_reset: null");
		drainEvents(g);
		memset(g->calls, 0, sizeof(g->calls));
		memset(g->cells, 0, sizeof(g->cells));
		memset(g->total_ms, 0, sizeof(g->total_ms));
		if (g->cc_aux) return te_gmg_profile_reset(g->cc_aux);
		return TE_OK;
	});
}

int te_gmg_profile_rows(te_gmg *g, int max_rows, char (*name)[64], int64_t *calls, double *total_ms,
                        int64_t *cells)
{
	return guarded([&]() -> int {
		if (!g || !name || !calls || !total_ms || !cells) return te::fail(TE_EINVAL, "te_gmg_profile_rows: null");
		drainEvents(g);
		const te_gmg *x = g->cc_aux; // the auxiliary solver of the sub-patch coarse solve: its launches count under their own class names
		if (x) drainEvents(g->cc_aux);
		int n = 0;
		for (int k = 0; k < KC_COUNT && n < max_rows; k++) {
			if (g->calls[k] + (x ? x->calls[k] : 0) == 0) continue;
			strncpy(name[n], kclassName[k], 63);
			name[n][63] = 0;
			calls[n]    = g->calls[k] + (x ? x->calls[k] : 0);
			total_ms[n] = g->total_ms[k] + (x ? x->total_ms[k] : 0.0);
			cells[n]    = g->cells[k] + (x ? x->cells[k] : 0);
			n++;
		}
		return n;
	});
}

#if TE_STAMPS
// diagnostic build only (not in include/te_hip.h): te_stamps_begin clears and arms the collection; te_stamps_read returns the number of
// instrumented launches since then and copies their stamps ([launch][1024][8] ticks of 10 ns), names and workgroup counts
int te_stamps_begin(te_gmg *g)
{
	return guarded([&]() -> int {
		auto &S = g->stamps;
		int   rc;
		if (!S.buf.p && (rc = S.buf.alloc((size_t) S.MAXL * S.MAXWG * TE_NSTAMP))) return rc;
		HIPCHK(hipStreamSynchronize(g->stream));
		HIPCHK(hipMemset(S.buf.p, 0, sizeof(unsigned long long) * S.buf.n));
		S.names.clear(), S.wgs.clear();
		S.on = true;
		return TE_OK;
	});
}
int te_stamps_read(te_gmg *g, unsigned long long *out, char (*names)[64], int *wgs, int max_launches)
{
	return guarded([&]() -> int {
		auto &S = g->stamps;
		S.on    = false;
		HIPCHK(hipStreamSynchronize(g->stream));
		const int n = std::min((int) S.names.size(), max_launches);
		if (n > 0) HIPCHK(hipMemcpy(out, S.buf.p, sizeof(unsigned long long) * (size_t) n * S.MAXWG * TE_NSTAMP, hipMemcpyDeviceToHost));
		for (int i = 0; i < n; i++) {
			strncpy(names[i], S.names[i].c_str(), 63);
			names[i][63] = 0;
			wgs[i]       = S.wgs[i];
		}
		return n;
	});
}
#endif

// te_bicgstab keeps its eight level-0 work vectors between solves (8 GiB at 512^3), te_fmg its own (three of level 0 and four of
// every coarser level); a caller that is done solving hands them back with this call (the next solve allocates them again)
int te_gmg_release_workspace(te_gmg *g)
{
	return guarded([&]() -> int {
			if (!g) return te::fail(TE_EINVAL, "te_gmg_release_workspace: null");
			for (te_vec *&v : g->bicg_work) {
				if (v) te_vec_destroy(v);
				v = nullptr;
			}
			fmgFree(g);
			coefRelease(g); // (a coefficient or a reaction term that is set stays: the solver's operator depends on it)
			coefCoarseRelease(g); // (the auxiliary solver goes while the kind is TE_COEF_COARSE_SWEEPS, else it stays)
			for (auto &L : g->levels) // the slope vectors of te_advect_flux_muscl / te_advect_muscl
				for (auto &s : L->muscl_s) (void) s.alloc(0);
			return TE_OK;
	});
}

// One TE_* switch (docs/SWITCHES.md) of this solver: value == NULL clears it (back to the default). te_gmg_create reads all of
// them from the environment once; afterwards this is the only way to change one. Switches that shape the level tables
// (TE_2D_SIMPLE, TE_NO_CFP, TE_2D_NO_MR_FUSE, TE_NO_OVERLAP, TE_EXCHANGE_TIMEOUT) are fixed at creation: TE_ESTATE.
int te_gmg_set_option(te_gmg *g, const char *name, const char *value)
{
	return guarded([&]() -> int {
			if (!g || !name) return te::fail(TE_EINVAL, "te_gmg_set_option: null argument");
			for (int o = 0; o < O_COUNT; o++)
				if (!strcmp(name, optName[o])) {
					if (optStructural(o))
						return te::fail(TE_ESTATE, std::string("te_gmg_set_option: ") + name + " is read when the solver is created; set it in the environment before te_gmg_create");
					if (o == O_ZS_PIN) {
						const int pin = parseSlabPin(value);
						if (value && !pin) return te::fail(TE_EINVAL, "te_gmg_set_option: TE_ZS_PIN must be 1, 2, 4 or 8");
						g->zs_pin = pin;
					}
					if (o == O_RESWEEP_V) {
						const int pin = parseResweepPin(value);
						if (value && !pin) return te::fail(TE_EINVAL, "te_gmg_set_option: TE_RESWEEP_V must be 19, 27 or 59");
						g->resweep_pin = pin;
					}
					g->cfg.set(o, value);
					if (g->cc_aux) (void) te_gmg_set_option(g->cc_aux, name, value); // (the auxiliary solver picks its kernels by the same switches)
					if (o == O_PUSH_TIMEOUT) g->push.timeout_s = value ? std::max(0.1, atof(value)) : (g->wd.timeout_s > 0 ? g->wd.timeout_s : 300.0);
					g->verified_opts.clear(); // (an option may change which exchanges a cycle issues)
					return TE_OK;
				}
			return te::fail(TE_EINVAL, std::string("te_gmg_set_option: unknown option ") + name);
	});
}

// what stencilSlabs<N> / rbgsSlabs<N> (gmg_ghosts3d.hpp) give a launch over the whole level as the switches stand
int te_gmg_slab_count(const te_gmg *g, int level, int kind, int *zs)
{
	return guarded([&]() -> int {
			if (!g || !zs || level < 0 || level >= (int) g->levels.size() || (kind != TE_SLABS_STENCIL && kind != TE_SLABS_SWEEP))
				return te::fail(TE_EINVAL, "te_gmg_slab_count: bad argument");
			const LevelHost &L = *g->levels[level];
			if (L.dim != 3)
				*zs = 1;
			else
				*zs = kind == TE_SLABS_STENCIL ? stencilSlabCount(L.n, L.P, slabSwitches(g)) : rbgsSlabCount(L.n, L.P, slabSwitches(g));
			return TE_OK;
	});
}
} // extern "C"
