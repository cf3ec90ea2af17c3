// 3D kernel launches of the fused cycle (opts.fuse = 2, 3): sweep from zero + residual + restriction, the recomputing post-sweep,
// the interface-only residual of the block-Jacobi smoother (see gmg_internal.hpp).
#include "gmg_ghosts3d.hpp"

namespace tei
{
// opts.fuse = 2: first pre-smoothing sweep from a zero iterate + residual + restriction (march3d.hpp,
// k_rbgs_zero_resid3d / k_restrict_fixup3d). out = S(0, f) with its x faces in xf_out, coarse = AvgRstr(f - A out).
// store_u = false (opts.fuse = 3): the new iterate is left in L.f6buf as its six face layers only
template <int N>
int zeroSweepResidN(te_gmg *g, LevelHost &L, const double *f, double *out, double *coarse, double *xf_out, bool store_u,
                    double *fcorr_out, const double *fcorr_in, const PendingRhs *fs)
{
	RestrictDst rd = restrictDst(L, coarse);
	// the patches export the 2x2 sums of their face layers (rs6); what lies behind a ghost slot, and a copy-through patch's own faces,
	// the gather kernel forms from the slot / the face layers
	// (round 6: on refined levels too -- the kernel's export does not look at what a patch is, a same-level neighbour's finished sums
	// are what the gather needs behind every FACE_LOCAL face, and they are a quarter of the face layers it read instead:
	// 141 -> 107 (descriptors) -> ... us per launch on `2refine --divide 3`; TE_NO_RS6_CF: as before)
	// ... and (round 6, last) also when a fix-up pass follows instead of the gather (the coarser level is not a fused one): it reads the
	// finished sums of same-level neighbours instead of their face layers (TE_NO_RS6_FIXUP: the layers, as before). Not on a level that
	// itself reads exported terms (fcorr_in): the kernel variant that does both is slower by more than the fix-up gains (measured at
	// 512^3, level 1: +3.5 us per cycle; 256^3, level 0, without fcorr_in: -2.3 us)
	const bool export_rs6 = L.rs6.p && !store_u
	                        && (fcorr_out ? (L.prolong_fusable || !g->cfg.has(O_NO_RS6_CF))
	                                      : (L.Pc > 0 || L.n_up > 0) && !fcorr_in && !g->cfg.has(O_NO_RS6_FIXUP));
	rd.rs6                = export_rs6 ? L.rs6.p : nullptr;
	int rc;
	if (L.P > 0) {
		Timed      t(g, store_u ? KC_ZERO_RESID : (fcorr_in ? KC_ZERO_RESID_FACES_FCORR : KC_ZERO_RESID_FACES), (size_t) L.P * L.nc, true);
		if (!store_u) L.f6_tab = L.f6off.p != nullptr && !g->cfg.has(O_PACK_FACES); // the face layers go where the level's table puts them
		LevelDev   D = L.dev();
		const dim3 grid = slabGrid(L.P), blk(Tile3<N>::TPB);
		if (store_u) {
			D.xf_out = xf_out;
			launchT(t, (k_rbgs_zero_resid3d<N, true>), grid, blk, 0, g->stream, D, f, out, rd, FSrc());
		} else {
			D.f6_out = L.f6buf.p;
			D.fcorr  = fcorr_in;
			dispatchBool(export_rs6, [&](auto ex) {
				constexpr bool EXP = decltype(ex)::value;
				if (fs) { // the right-hand side is a pending vector statement of te_bicgstab (march3d.hpp FSrc): formed and stored here
					// (level 0 only, whose right-hand side never carries exported terms: FS != 0 is never combined with FCORR)
					if (fs->kind == 1)
						launchT(t, (k_rbgs_zero_resid3d<N, false, EXP, false, 1>), grid, blk, 0, g->stream, D, f, out, rd, fs->args);
					else
						launchT(t, (k_rbgs_zero_resid3d<N, false, EXP, false, 2>), grid, blk, 0, g->stream, D, f, out, rd, fs->args);
				} else
					dispatchBool(fcorr_in != nullptr, [&](auto fc) {
						launchT(t, (k_rbgs_zero_resid3d<N, false, EXP, decltype(fc)::value>), grid, blk, 0, g->stream, D, f, out, rd, FSrc());
					});
			});
		}
	}
	// the new face layers of neighbours on other ranks (no-op on one rank)
	if ((rc = prepareGhosts<N>(g, L, {out, store_u ? nullptr : L.f6buf.p}))) return rc;
	L.ghost_has_v = !store_u; // (the slots of neighbours on other ranks hold their face layers of v until the next exchange of the level)
	if (fcorr_out) { // the ghost terms were formed by the patches that own the face values: sort them into the coarse
		// level's side array (a permutation copy of 6/128 of a vector instead of the fix-up pass)
		if (L.Pc > 0) { // descriptors once per level, then 16-byte data loads only (k_fcorr_gather3d_v2)
			LevelDev   D       = L.dev();
			const int  key     = (export_rs6 ? 1 : 0) | (D.f6off ? 2 : 0);
			const bool rebuild = L.gdesc_key != key; // (built once; again if the face layers change their layout: TE_PACK_FACES)
			if (rebuild) {
				int rc2 = L.gdesc.p ? TE_OK : L.gdesc.alloc((size_t) L.Pc * 48);
				if (rc2) return rc2;
				hipLaunchKernelGGL(k_gather_desc3d<N>, dim3(L.Pc), dim3(64), 0, g->stream, D, L.child.p, L.copy.p, export_rs6 ? 1 : 0, L.gdesc.p);
				L.gdesc_key = key;
			}
			// the gather never stores a plane without a term: the side array's zeros are set here, for every new set of descriptors
			// and every new side array (LevelHost::fcorr: the gather is its only writer)
			if (rebuild || L.fcorr_zeroed_for != fcorr_out) {
				HIPCHK(hipMemsetAsync(fcorr_out, 0, sizeof(double) * (size_t) L.Pc * 4 * N * N, g->stream));
				L.fcorr_zeroed_for = fcorr_out;
			}
			Timed t(g, KC_FCORR_GATHER, (size_t) L.P * 6 * L.nf / 4);
			hipLaunchKernelGGL(k_fcorr_gather3d_v2<N>, dim3(L.Pc * 12), dim3(256), 0, g->stream, D, (const GatherDesc *) L.gdesc.p,
			                   export_rs6 ? (const double *) L.rs6.p : (const double *) nullptr, (const double *) L.f6buf.p, coarse, fcorr_out);
		}
	} else if (L.P > 0) {
		Timed    t(g, KC_FIXUP, (size_t) L.P * 6 * L.nf);
		LevelDev D = L.dev();
		if (store_u)
			D.xf = xf_out;
		else
			D.f6 = L.f6buf.p;
		hipLaunchKernelGGL((k_restrict_fixup3d<N, false>), dim3(L.P), dim3(256), 0, g->stream, D, out, rd);
	}
	// children whose parent lives on another rank: ship the finished blocks (as residRestrictN)
	if ((rc = shipRestricted<N>(g, L, coarse))) return rc;
	HIPCHK(hipGetLastError());
	return TE_OK;
}

// opts.fuse = 3, post-smoothing: out = S(v + P(prolong_from), f) with v = S(0, f) recomputed (its faces in L.f6buf)
template <int N>
int resweepProlongN(te_gmg *g, LevelHost &L, const double *f, double *out, const double *prolong_from, double *xf_out, const double *fcorr_in)
{
	ProlongSrc ps      = prolongSrc(L, prolong_from);
	const bool refined = L.ncf > 0 || L.has_copy; // copy-through patches / coarse-fine ghost slots
	// the kernel's tuning variant (dispatch.hpp resweepVariant: the defaults and what each was measured against; all bit-identical)
	const int v = resweepVariant(fcorr_in != nullptr, refined, L.index, (size_t) L.P * L.nc * sizeof(double), g->resweep_pin);
	if (!v) return te::fail(TE_ESTATE, "resweepProlong: exported ghost terms on a refined level");
	auto launch = [&](LevelDev D) {
		if (D.count == 0) return;
		Timed t(g, fcorr_in ? KC_RESWEEP_FCORR : KC_RESWEEP, (size_t) D.count * L.nc, true);
		D.f6    = L.f6buf.p;
		D.fcorr = fcorr_in;
		const dim3 grid = slabGrid(D.count), blk(Tile3<N>::TPB);
		if (refined) {
			if (v == 59)
				launchT(t, (k_rbgs_resweep_prolong3d<N, 59, false, true>), grid, blk, 0, g->stream, D, f, out, ps);
			else
				launchT(t, (k_rbgs_resweep_prolong3d<N, 27, false, true>), grid, blk, 0, g->stream, D, f, out, ps);
		} else if (v == 3) {
			launchT(t, (k_rbgs_resweep_prolong3d<N, 3, true>), grid, blk, 0, g->stream, D, f, out, ps);
		} else if (v == 19) {
			launchT(t, (k_rbgs_resweep_prolong3d<N, 19>), grid, blk, 0, g->stream, D, f, out, ps);
		} else if (v == 59) {
			launchT(t, (k_rbgs_resweep_prolong3d<N, 59>), grid, blk, 0, g->stream, D, f, out, ps);
		} else {
			launchT(t, (k_rbgs_resweep_prolong3d<N, 27>), grid, blk, 0, g->stream, D, f, out, ps);
		}
	};
	if (L.post_exchange_free && L.ghost_has_v && !refined && !g->cfg.has(O_POST_EXCHANGE)) {
		// every neighbour's parent is local (the coarser level lives on every rank) and the ghost slots still hold the neighbours'
		// face layers of v: the kernel forms v + P e for them as for local neighbours; nothing travels (a global decision: all
		// ranks of the level take it together)
		ps.gparent    = L.slot_parent.p;
		ps.gorth      = L.slot_orth.p;
		L.ghost_has_v = false;
		LevelDev D    = L.dev();
		D.xf_out      = xf_out;
		launch(D);
		HIPCHK(hipGetLastError());
		return TE_OK;
	}
	// neighbours on other ranks receive the face layers of v + P(coarse)
	int rc = withGhosts<N>(g, L, {nullptr, L.f6buf.p, &ps}, launch, nullptr, xf_out);
	if (rc) return rc;
	HIPCHK(hipGetLastError());
	return TE_OK;
}

int resweepProlong(te_gmg *g, LevelHost &L, const double *f, double *out, const double *prolong_from, double *xf_out,
                   const double *fcorr_in)
{
	if (L.dim == 2) return resweepProlong2d(g, L, f, out, prolong_from);
	return dispatchN(L.n, [&](auto n) { return resweepProlongN<decltype(n)::value>(g, L, f, out, prolong_from, xf_out, fcorr_in); });
}

// opts.fuse = 2 with the block-Jacobi smoother: after an exact patch solve from the zero iterate the residual
// vanishes inside every patch (A_patch u = f is what was solved) and equals -(g + m)/h^2 = -2 gamma/h^2 on the face
// layers (the patch operator closes interface faces with ghost = -m, the level operator with the neighbour's g), so
// coarse f = AvgRstr(f - A u) is k_restrict_fixup3d<OWN> applied to a zeroed coarse vector: no pass over u and f
// at all. (What is dropped is the rounding noise of the solve, ~1e-13 |f|.) u: the new iterate, xf: its
// compact x faces or null; coarse: the coarse level's f with `coarse_n` entries.
template <int N> int interfaceResidRestrictN(te_gmg *g, LevelHost &L, const double *u, const double *xf, double *coarse, size_t coarse_n)
{
	RestrictDst rd = restrictDst(L, coarse);
	int rc;
	if ((rc = prepareGhosts<N>(g, L, {u, L.ps_faces ? L.f6buf.p : nullptr}))) return rc;
	{
		Timed t(g, KC_VECOP, coarse_n);
		// (blocks exchanged in place: only this rank's run -- the others' runs are received, and with the direct-store transport a
		// peer that is ahead may have stored its run already)
		if (L.repl_up && L.repl_direct && !g->cfg.has(O_REPL_BLOCKS) && !L.tx_direct.empty()) {
			if (L.tx_direct.send_cnt[0] > 0)
				HIPCHK(hipMemsetAsync(coarse + L.tx_direct.send_off[0], 0, sizeof(double) * (size_t) L.tx_direct.send_cnt[0], g->stream));
		} else
			HIPCHK(hipMemsetAsync(coarse, 0, sizeof(double) * coarse_n, g->stream));
		if (L.n_up > 0) HIPCHK(hipMemsetAsync(L.upbuf.p, 0, sizeof(double) * L.upbuf.n, g->stream));
	}
	if (L.P > 0) {
		Timed    t(g, KC_FIXUP, (size_t) L.P * 6 * L.nf);
		LevelDev D = L.dev();
		D.xf       = L.ps_faces ? nullptr : xf;
		D.f6       = L.ps_faces ? L.f6buf.p : nullptr;
		hipLaunchKernelGGL((k_restrict_fixup3d<N, true>), dim3(L.P), dim3(256), 0, g->stream, D, u, rd);
	}
	if ((rc = shipRestricted<N>(g, L, coarse))) return rc;
	HIPCHK(hipGetLastError());
	return TE_OK;
}

int interfaceResidRestrict(te_gmg *g, LevelHost &L, const double *u, const double *xf, double *coarse, size_t coarse_n)
{
	return dispatchN(L.n, [&](auto n) { return interfaceResidRestrictN<decltype(n)::value>(g, L, u, xf, coarse, coarse_n); });
}

int zeroSweepResid(te_gmg *g, LevelHost &L, const double *f, double *out, double *coarse, double *xf_out, bool store_u,
                   double *fcorr_out, const double *fcorr_in, const PendingRhs *fs, const Fold2DHost *fold_in, bool skip_fixup)
{
	if (L.dim == 2) return zeroSweepResid2d(g, L, f, out, coarse, store_u, fold_in, skip_fixup);
	if ((fold_in && fold_in->fine) || skip_fixup) return te::fail(TE_ESTATE, "zeroSweepResid: the folded fix-up exists in 2D only");
	return dispatchN(L.n, [&](auto n) {
		return zeroSweepResidN<decltype(n)::value>(g, L, f, out, coarse, xf_out, store_u, fcorr_out, fcorr_in, fs);
	});
}
} // namespace tei
