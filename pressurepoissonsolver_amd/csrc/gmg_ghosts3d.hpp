// Shared by the 3D launch units (gmg_launch3d.hip, gmg_fused3d.hip, gmg_patchsolve.hip): making a level's ghost planes current
// around a kernel launch -- pack, face exchange (or the interior / boundary split around it), coarse/fine ghosts -- and shipping
// restricted blocks to the ranks that hold the parents. Templates on the patch size, instantiated where they are used. Also what
// every 3D launch site shares: the slab rules, the grid, the builders of the kernels' argument structs (dispatch.hpp: the dispatch).
#pragma once
#include "dispatch.hpp"
#include "gmg_internal.hpp"

namespace tei
{
struct GhostSrc { // the iterate whose faces one ghost update reads
	const double     *u;            // the stored iterate
	const double     *f6 = nullptr; // non-null: the iterate exists only as its six face layers, there (LevelHost::f6buf)
	const ProlongSrc *ps = nullptr; // the faces are those of the iterate + P(ps->coarse), which is never stored
};

// make every ghost plane of `src` current: remote same-level faces (pack -> exchange -> ghost slots
// [0, nremote)), then the coarse/fine planes. Replaces SchurHelper.h:145-150 updateInterfaceDist.
// may_push: the exchange that follows is on the solver stream -- with the direct-store transport the pack kernel then stores the
// layers into the receivers' ghost slots itself and raises their flags (PackPush); returns true when it did (the caller finishes
// with pushFinish instead of an exchange of the send buffer)
template <int N> bool packFaces(te_gmg *g, LevelHost &L, const GhostSrc &src, bool may_push = false)
{
	const bool push = may_push && g->push.on && L.push_faces && !g->recording && L.push_face_dst[0].p;
	Timed      t(g, push ? KC_EXCHANGE : KC_PACK, (size_t) L.nremote * L.nf);
	const dim3 grid(L.nremote), blk(N * N < 256 ? N * N : 256);
	PackPush   pp;
	if (push) {
		pushBegin(g, L, 1);
		pp.dst    = L.push_face_dst[L.push_par].p;
		pp.flags  = L.push_face_flags.p;
		pp.nflags = (int) L.push_face_flags.n;
		pp.epoch  = L.push_ep;
		pp.raise  = pushRaiseValue(g, L.push_ep);
		pp.done   = L.push_done.p;
		pp.err    = g->push.err;
		pp.err_host = g->push.err_host;
	}
	if (src.f6) {
		ProlongSrc none{nullptr, nullptr, nullptr};
		hipLaunchKernelGGL(k_pack_faces6_3d<N>, grid, blk, 0, g->stream, L.send_faces.p, src.f6, src.ps ? *src.ps : none, L.sendbuf.p, L.f6Off(), pp);
	} else if (src.ps)
		hipLaunchKernelGGL(k_pack_faces_prolong3d<N>, grid, blk, 0, g->stream, L.send_faces.p, src.u, *src.ps, L.sendbuf.p, pp);
	else
		hipLaunchKernelGGL(k_pack_faces3d<N>, grid, blk, 0, g->stream, L.send_faces.p, src.u, L.sendbuf.p, pp);
	return push;
}

// ghost planes of the coarse/fine faces from the current iterate
template <int N> void cfGhosts(te_gmg *g, LevelHost &L, const GhostSrc &src)
{
	Timed      t(g, KC_CFGHOST, (size_t) L.ncf * L.nf);
	const dim3 grid(L.ncf), blk(N * N < 256 ? N * N : 256);
	if (src.f6) {
		if (src.ps)
			hipLaunchKernelGGL((k_cf_ghost6_3d<N, true>), grid, blk, 0, g->stream, L.cf_desc.p, L.cf_slots.p, src.f6, *src.ps, L.ghostCur(), L.f6Off());
		else
			hipLaunchKernelGGL((k_cf_ghost6_3d<N, false>), grid, blk, 0, g->stream, L.cf_desc.p, L.cf_slots.p, src.f6, ProlongSrc(), L.ghostCur(), L.f6Off());
	} else if (src.ps)
		hipLaunchKernelGGL(k_cf_ghost_prolong3d<N>, grid, blk, 0, g->stream, L.cf_desc.p, L.cf_slots.p, src.u, *src.ps, L.ghostCur());
	else
		hipLaunchKernelGGL(k_cf_ghost3d<N>, grid, blk, 0, g->stream, L.cf_desc.p, L.cf_slots.p, src.u, L.ghostCur());
}

template <int N> int prepareGhosts(te_gmg *g, LevelHost &L, const GhostSrc &src, bool patch_op = false)
{
	if (patch_op) return TE_OK; // the patch operator (LevelHost::dev) reads no neighbour
	L.ghost_has_v = false;
	if (L.nremote > 0) {
		// the face layers of an iterate that exists only as such already sit in send order (LevelHost::f6off): sent from there
		const bool direct = src.f6 && !src.ps && L.f6Off();
		const bool pushed = !direct && packFaces<N>(g, L, src, true);
		int        rc     = pushed ? pushFinish(g, L, 1, g->stream) : faceExchange(g, L, direct ? src.f6 : L.sendbuf.p);
		if (rc) return rc;
	}
	if (L.ncf == 0) return TE_OK;
	cfGhosts<N>(g, L, src);
	return TE_OK;
}

// Run `launch(subset)` over all patches of the level with current ghosts. With off-rank neighbours the
// exchange goes to the communication stream and the interior patches (no ghost-slot face) are computed
// underneath it; the boundary patches follow once the receive has landed. (north star: "ghost-cell
// exchange ... overlapped with interior smoothing")
template <int N, class F> int withGhosts(te_gmg *g, LevelHost &L, const GhostSrc &src, F launch_, const double *xf_in = nullptr,
                                         double *xf_out = nullptr, bool patch_op = false)
{
	auto launch = [&](LevelDev D) {
		D.xf     = xf_in;
		D.xf_out = xf_out;
		launch_(D);
	};
	// (levels with few local patches: nothing worth hiding under the exchange, and the second stream and its two
	// events only add host calls and latency)
	// TE_OVERLAP_MIN (tests set 0 so that their small levels take the overlapped path). The split costs a second launch -- no
	// launch is shorter than one patch march, about 30 us -- and two cross-stream event hand-overs of about 20 us each, so it
	// pays only where the interior launch is much longer than that: more local patches than the chip holds workgroups at once
	// (3 x 256). Measured per rank with the exchanges in loop-back (tools/mr8_budget.py): at 512 local patches (512^3 on eight
	// ranks) the cycle is 525 us with the split and 475 us without it.
	L.ghost_has_v = false;
	const int mode = L.overlap_mode >= 0 ? L.overlap_mode : (L.P < g->cfg.num(O_OVERLAP_MIN, 768) ? 0 : (g->cfg.num(O_OVERLAP_MODE, 1) == 2 ? 2 : 1));
	if (patch_op || g->recording || L.nremote == 0 || !g->overlap || L.n_int == 0 || mode == 0) {
		int rc = prepareGhosts<N>(g, L, src, patch_op);
		if (rc) return rc;
		launch(L.dev(patch_op));
		return TE_OK;
	}
	if (mode == 2) {
		// the interior patches go to the second stream (they wait for nothing but what the solver stream has done so far); pack,
		// exchange, coarse/fine ghosts and the boundary patches stay on the solver stream, which then waits for the interior
		HIPCHK(hipEventRecord(g->ev_pack, g->stream));
		HIPCHK(hipStreamWaitEvent(g->comm_stream, g->ev_pack, 0));
		std::swap(g->stream, g->comm_stream); // (every launch helper launches on g->stream)
		launch(L.devPart(false));
		hipError_t e = hipEventRecord(g->ev_recv, g->stream);
		std::swap(g->stream, g->comm_stream);
		HIPCHK(e);
		const bool pushed = packFaces<N>(g, L, src, true);
		int        rc     = pushed ? pushFinish(g, L, 1, g->stream) : faceExchange(g, L, L.sendbuf.p);
		if (rc) return rc;
		if (L.ncf > 0) cfGhosts<N>(g, L, src);
		launch(L.devPart(true));
		HIPCHK(hipStreamWaitEvent(g->stream, g->ev_recv, 0));
		return TE_OK;
	}
	packFaces<N>(g, L, src);
	HIPCHK(hipEventRecord(g->ev_pack, g->stream));
	HIPCHK(hipStreamWaitEvent(g->comm_stream, g->ev_pack, 0));
	int rc = faceExchange(g, L, L.sendbuf.p, g->comm_stream);
	if (rc) return rc;
	HIPCHK(hipEventRecord(g->ev_recv, g->comm_stream));
	launch(L.devPart(false)); // interior, concurrent with the exchange
	HIPCHK(hipStreamWaitEvent(g->stream, g->ev_recv, 0));
	if (L.ncf > 0) cfGhosts<N>(g, L, src);
	launch(L.devPart(true)); // boundary
	return TE_OK;
}

// z-slabs per patch for the stencil kernels (and the MAC operators, the interpolators, the regrid transfer): enough workgroups to
// fill 256 CUs a few times over when the level has few patches
// (the rule itself is dispatch.hpp stencilSlabCount; this reads the solver's switches)
template <int N> inline int stencilSlabs(const te_gmg *g, int P) { return stencilSlabCount(N, P, slabSwitches(g)); }

// z-slabs per patch for the RB-GS kernels: enough workgroups to occupy 256 CUs x 4 when the level has few patches
// (dispatch.hpp rbgsSlabCount)
template <int N> inline int rbgsSlabs(const te_gmg *g, int count) { return rbgsSlabCount(N, count, slabSwitches(g)); }

// the grid of a launch over `count` patches in `zs` slabs each with Tile3<N>::TPB threads: whole multiples of eight workgroups
inline dim3 slabGrid(int count, int zs = 1) { return dim3(8 * ((count * zs + 7) / 8)); }

// where the restricting kernels put a patch's coarse block (kernels3d.hpp RestrictDst; rs6 stays the caller's business)
inline RestrictDst restrictDst(const LevelHost &L, double *coarse)
{
	RestrictDst rd = RestrictDst();
	rd.parent     = L.parent.p;
	rd.orth       = L.orth.p;
	rd.coarse     = coarse;
	rd.remote     = L.upbuf.p;
	rd.remote_off = L.up_off.p;
	return rd;
}

// the iterate is u + P(coarse) (march3d.hpp ProlongSrc; cbase and gparent / gorth are set by the callers whose kernels read them)
inline ProlongSrc prolongSrc(const LevelHost &L, const double *coarse)
{
	ProlongSrc ps;
	ps.parent = L.parent.p;
	ps.orth   = L.orth.p;
	ps.coarse = coarse;
	return ps;
}

// The restricted blocks of this rank's patches to the other ranks (the kernels before this have written them into the local
// coarse patches or into upbuf), the other ranks' blocks into the local coarse patches. repl_up (the coarse level lives on
// every rank): the finished octants are copied out of the coarse patches first -- one copy, sent to everybody.
template <int N> int shipRestricted(te_gmg *g, LevelHost &L, double *coarse)
{
	// every rank's blocks are whole coarse patches in one run of the coarse vector: run to run, in place
	if (L.repl_up && L.repl_direct && !g->cfg.has(O_REPL_BLOCKS)) {
		if (g->push.on && L.push_blocks && !g->recording) return pushExchange(g, L, 2, coarse);
		return doExchange(g, 2, L.tx_direct, coarse, coarse);
	}
	if (L.repl_up && L.n_up > 0) {
		Timed t(g, KC_PACK, (size_t) L.n_up * L.nc / 8);
		hipLaunchKernelGGL(k_prolong_pack3d<N>, dim3(L.n_up), dim3(256), 0, g->stream, L.bc_desc.p, L.up_off.p, coarse, L.upbuf.p);
	}
	int rc = doExchange(g, 2, L.tx_up, L.upbuf.p, L.downbuf.p);
	if (rc) return rc;
	if (L.n_down > 0) {
		Timed t(g, KC_PACK, (size_t) L.n_down * L.nc / 8);
		hipLaunchKernelGGL(k_restrict_unpack3d<N>, dim3(L.n_down), dim3(256), 0, g->stream, L.down_desc.p, L.down_off.p,
		                   L.downbuf.p, coarse);
	}
	return TE_OK;
}
} // namespace tei
