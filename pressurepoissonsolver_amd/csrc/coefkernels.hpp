// The variable-coefficient operator A_b u = div(beta grad u) and what a cycle needs of it (include/te_hip.h
// restates the definitions). Nothing in the reference has a coefficient. beta is a FACE vector of the level (projkernels.hpp: per
// patch LO_a, a = 0..D-1, then HI_a), positive, its two copies of a shared face equal; nothing here checks that.
//
//   apply     (A_b u)[c] = sum over a = x, y, z in that order of (b_hi (u_hi - u_c) - b_lo (u_c - u_lo)) * rh2_a
//             u_lo / u_hi across a patch face: the ghost te_apply reads there (neighbour cell, ghost slot, -m Dirichlet, +m Neumann);
//             b_lo = LO_a[c], b_hi = LO_a[c + e_a], or HI_a on the patch's upper face
//   residual  f - A_b u
//   Jacobi    u + omega (f - A_b u) / (-d_J),  d_J = sum over sides of b_s (1 + adj_s) rh2_a, adj_s = face_kadj on a patch face, else 0
//   RB-GS     patch-local, red = (x + y + z) even first, ghosts of faces with a neighbour frozen at the old iterate:
//             u_c <- (o - f_c) / d,  o = sum over sides of b_s v_s rh2_a (interior neighbours and frozen ghosts; physical faces 0),
//             d = sum over sides of b_s kappa_s rh2_a, kappa = 1 (interior or neighbour face), 2 (Dirichlet), 0 (Neumann)
// With beta = 1 these are k_stencil3d's / k_rbgs3d's numbers up to rounding.
//
// 3D: k_coef_stencil3d<N, MODE, ZS> (operator, residual, Jacobi) and k_coef_rbgs3d<N, ZS> (the sweep) are the plane marches of
// k_stencil3d / k_rbgs3d with the coefficient planes riding along (see there). 2D: k_coef_stencil2d<MODE> has the simple shape of
// k_stencil2d (one thread per cell, neighbours, ghosts and the coefficient from global memory); the sweep is k_coef_rbgs2d_lds for
// n <= 64 (the patch and its ring in LDS, both colours in one launch) and the two colour launches k_coef_rbgs2d<0 / 1> above that,
// the second one in place on `out` with neighbour patches and ghost slots still read from the old iterate u. The level's ghost
// slots are made current by the caller (withGhosts / prepareGhosts2d) exactly as for te_apply.
//
// The restriction of the coefficient, k_faces_restrict3d<N> / k_faces_restrict2d: level l + 1's beta = the face average of level
// l's -- te_faces_regrid's "coarsen" rule (faceregridkernels.hpp coarsenPairX / coarsenPairT / face2d) through the level's child / copy
// tables. One writer per entry; a patch that copies through hands its block on bit for bit. Sharded hierarchies: a child whose parent
// lives on another rank restricts itself into a block that travels (k_faces_restrict_pack3d / 2d), and the parent's rank picks its
// entries from local children and received blocks alike (k_faces_restrict_recv3d / 2d): the same means, the same bits (see there).
//
// The reaction term: every operator / sweep kernel has a compile-time SIG and a pointer to the level's cell
// vector sigma >= 0. SIG = true: apply (A_b u)[c] - sigma_c u_c (A_b as above, then one multiplication and one subtraction), residual
// f - that, Jacobi's diagonal d_J + sigma_c, RB-GS's d + sigma_c. Every load and use of sigma sits under `if constexpr (SIG)`:
// SIG = false is the code as it was before the term existed.
//
// FMA contraction is off for this file (it is included behind faceregridkernels.hpp, whose pragma holds to the end of the unit): the
// sums above are evaluated as written.
#pragma once
#include "faceregridkernels.hpp"
#include "march3d.hpp"

namespace te
{
#pragma clang fp contract(off)

struct CoefLevel {
	int32_t        P, n;
	const int32_t *face_kind; // [P * 2 D]
	const int32_t *face_src;  // [P * 2 D]
	const double  *face_kadj; // [P * 2 D]
	const double  *rh2;       // [P * 3]
	const double  *ghost;     // [nslots * n^(D-1)]
	const double  *beta;      // the level's coefficient, a face vector
};


// One cell c of patch p. `in` = the patch's block of the iterate the interior neighbours are read from, `u` = the whole vector the
// neighbour patches are read from (the old iterate), m = the cell's own value (RELAX: not used).
// RELAX = false: acc = (A_b u)[c], diag = d_J.   RELAX = true: acc = o, diag = d.
template <bool RELAX>
__device__ __forceinline__ void coefCell2d(const CoefLevel &L, const double *__restrict__ u, const double *in, int p, int c, double m, double &acc,
                                         double &diag)
{
	constexpr int D = 2;
	const int     n = L.n, nc = n * n, nf = n;
	const size_t  FV = (size_t) D * nc + (size_t) D * nf;
	const double *bp = L.beta + (size_t) p * FV;
	acc = 0.0, diag = 0.0;
	int sa = 1;
#pragma unroll
	for (int a = 0; a < D; a++, sa *= n) {
		const int    ca = (c / sa) % n;
		const int    tl = c % sa, th = c / (sa * n), t = tl + th * sa; // the face coordinate: the other axes in order
		const double rh = L.rh2[(size_t) p * 3 + a];
		const double blo = bp[(size_t) a * nc + c];
		const double bhi = ca < n - 1 ? bp[(size_t) a * nc + c + sa] : bp[(size_t) D * nc + (size_t) a * nf + t];
		double       v[2], kap[2] = {1.0, 1.0}, adj[2] = {0.0, 0.0};
		bool         phys[2] = {false, false};
#pragma unroll
		for (int hi = 0; hi < 2; hi++) {
			const bool inside = hi ? ca < n - 1 : ca > 0;
			if (inside) {
				v[hi] = in[hi ? c + sa : c - sa];
				continue;
			}
			const int s = 2 * a + hi, kind = L.face_kind[(size_t) p * 2 * D + s], src = L.face_src[(size_t) p * 2 * D + s];
			adj[hi]     = L.face_kadj[(size_t) p * 2 * D + s];
			if (kind == FACE_DIRICHLET) {
				v[hi] = -m, kap[hi] = 2.0, phys[hi] = true;
			} else if (kind == FACE_NEUMANN) {
				v[hi] = m, kap[hi] = 0.0, phys[hi] = true;
			} else if (kind == FACE_GHOST) {
				v[hi] = L.ghost[(size_t) src * nf + t];
			} else { // the neighbour's facing cell
				v[hi] = u[(size_t) src * nc + tl + (hi ? 0 : n - 1) * sa + th * sa * n];
			}
		}
		if (RELAX) {
			if (!phys[0]) acc += blo * v[0] * rh;
			if (!phys[1]) acc += bhi * v[1] * rh;
			diag += blo * kap[0] * rh;
			diag += bhi * kap[1] * rh;
		} else {
			acc += (bhi * (v[1] - m) - blo * (m - v[0])) * rh;
			diag += blo * (1.0 + adj[0]) * rh;
			diag += bhi * (1.0 + adj[1]) * rh;
		}
	}
}

template <int MODE, bool SIG = false>
__global__ __launch_bounds__(256) void k_coef_stencil2d(CoefLevel L, const double *__restrict__ u, const double *__restrict__ f,
                                                      double *__restrict__ out, double omega, const double *__restrict__ sigma = nullptr)
{
	const int    nc = L.n * L.n;
	const size_t total = (size_t) L.P * nc;
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int    p = (int) (idx / nc), c = (int) (idx % nc);
		const double m = u[idx];
		double       au, dj;
		coefCell2d<false>(L, u, u + (size_t) p * nc, p, c, m, au, dj);
		if constexpr (SIG) { // A_b,sigma u = A_b u - sigma u; the Jacobi diagonal d_J + sigma
			const double sg = sigma[idx];
			au              = au - sg * m;
			dj              = dj + sg;
		}
		if (MODE == COEF_APPLY)
			out[idx] = au;
		else if (MODE == COEF_RESID)
			out[idx] = f[idx] - au;
		else
			out[idx] = m + omega * (f[idx] - au) / (-dj);
	}
}

// ---- 3D operator, residual, Jacobi: the plane march of k_stencil3d (march3d.hpp) with the coefficient planes riding along.
// One workgroup per patch or z-slab, a thread owns a 2 x 2 column: u exactly as in k_stencil3d (planes z-1, z, z+1 in registers,
// z+2 / z+3 in a two-slot ring, x / y neighbours through the LDS tile, halos through haloSrc / zPlaneSrc). beta: the three LO planes
// of plane z and this thread's HI_x / HI_y pairs are requested ONE step ahead (as k_gradient3d<PROJECT> requests U), LO_z of plane
// z + 1 one step ahead as well (it is this step's upper and the next step's lower z-face), the plane above the slab -- LO_z of the
// next slab's first plane, or HI_z -- two steps before the end. The upper x-face of a pair is the next lane's LO_x (HI_x on the
// row's last pair), the upper y-face of the upper row the next row pair's LO_y through LDS (HI_y on the last row), as in
// k_divergence3d. Nothing a step requests is consumed by the same step; every load of the loop is unconditional, from a pointer and
// stride chosen before the loop. Algorithmic bytes per site at N = 32: u 8 + 6/32 * 8 = 9.5, beta 24.75, out 8 -> 42.25 (apply),
// + 8 for f -> 50.25 (residual, Jacobi).
//
// SIG (te_gmg_set_reaction): the cell vector sigma rides along exactly as f does -- the thread's own two
// pairs of plane z + 2 requested in the refill, consumed two steps later; (A_b u)[c] - sigma_c u_c, the Jacobi diagonal d_J + sigma_c.
// + 8 B/site. Every load and use of sigma sits under `if constexpr (SIG)`: SIG = false is the kernel as it was.
template <int N, int MODE, int ZS, bool SIG = false>
__global__ __launch_bounds__(Tile3<N>::TPB) void k_coef_stencil3d(LevelDev L, const double *__restrict__ beta, const double *__restrict__ u,
                                                                  const double *__restrict__ f, double *__restrict__ out, double omega,
                                                                  const double *__restrict__ sigma = nullptr)
{
	using T           = Tile3<N>;
	constexpr int TPB = T::TPB, NP = T::NP, H = T::H;
	constexpr int NN = N * N, NNN = N * N * N;
	constexpr int ZL = N / ZS;
	constexpr size_t FV = 3 * (size_t) NNN + 3 * NN;
	constexpr bool HAS_F = MODE != COEF_APPLY;
	const int nblocks = L.count * ZS;
	const int work    = xcdRemap(blockIdx.x, nblocks);
	if (work >= nblocks) return;
	const int  pid = L.order ? L.order[L.first + work / ZS] : L.first + work / ZS;
	const int  z0  = (work % ZS) * ZL;
	const int  tid = threadIdx.x;
	const bool last = z0 + ZL == N;

	__shared__ __attribute__((aligned(16))) double tile[2][T::LSZ];
	__shared__ double2 brow[2][TPB + H];

	const Reg6     fk(L.face_kind + (size_t) pid * 6), fs(L.face_src + (size_t) pid * 6);
	const double   rhx = L.rh2[(size_t) pid * 3], rhy = L.rh2[(size_t) pid * 3 + 1], rhz = L.rh2[(size_t) pid * 3 + 2];
	const double  *up  = u + (size_t) pid * NNN;
	const double2 *up2 = reinterpret_cast<const double2 *>(up);
	const double2 *fp2 = reinterpret_cast<const double2 *>((HAS_F ? f : u) + (size_t) pid * NNN);
	double2       *op2 = reinterpret_cast<double2 *>(out + (size_t) pid * NNN);
	const double2 *sp2 = reinterpret_cast<const double2 *>((SIG ? sigma : u) + (size_t) pid * NNN);
	const double2 *lo2 = reinterpret_cast<const double2 *>(beta + (size_t) pid * FV);                    // LO_a plane z: lo2[a * NNN / 2 + z * NP + q]
	const double2 *hi2 = reinterpret_cast<const double2 *>(beta + (size_t) pid * FV + 3 * (size_t) NNN); // HI_a: hi2[a * NN / 2 + ...]

	const bool act = (T::NT == TPB) || tid < T::NT;
	const int  X = act ? tid % H : 0, Yp = act ? tid / H : 0;
	int        q[2], lds[2];
	const int  ldo[2] = {T::row(2 * Yp) + 2 * X + 2, T::row(2 * Yp + 3) + 2 * X + 2};
#pragma unroll
	for (int k = 0; k < 2; k++) {
		q[k]   = (2 * Yp + k) * H + X;
		lds[k] = T::row(2 * Yp + k + 1) + 2 * X + 2;
	}
	const bool     east = X == H - 1, north = Yp == H - 1;
	const double2 *hxp = east ? hi2 + Yp : lo2; // HI_x[y + N z], rows 2 Yp and 2 Yp + 1 (a harmless address and stride 0 for the others)
	const double2 *hyp = north ? hi2 + NN / 2 + X : lo2; // HI_y[x + N z]
	const int      hxs = east ? H : 0, hys = north ? H : 0;

	// Jacobi: 1 + adj of the six sides where this thread's cells touch them
	double wW = 1.0, wE = 1.0, wS = 1.0, wN = 1.0, wB = 1.0, wT = 1.0;
	if (MODE == COEF_JACOBI) {
		const double *kp = L.face_kadj + (size_t) pid * 6;
		double        ka[6];
#pragma unroll
		for (int s6 = 0; s6 < 6; s6++) ka[s6] = kp[s6];
		wW = 1.0 + (X == 0 ? ka[0] : 0.0), wE = 1.0 + (east ? ka[1] : 0.0);
		wS = 1.0 + (Yp == 0 ? ka[2] : 0.0), wN = 1.0 + (north ? ka[3] : 0.0);
		wB = 1.0 + ka[4], wT = 1.0 + ka[5];
	}

	const HaloSrc  hs  = haloSrc<N>(tid, fk, fs, u, up, L.ghost, -1.0, 1.0, L.xf);
	const PlaneSrc bot = zPlaneSrc<N>(fk[4], fs[4], false, u, up, L.ghost, -1.0, 1.0);
	const PlaneSrc top = zPlaneSrc<N>(fk[5], fs[5], true, u, up, L.ghost, -1.0, 1.0);

	double2 um[2], uc[2], un[2], fc[2], sc[2];
	double2 ur[2][2], fr[2][2], sr[2][2];
	double2 bx[2], by[2], bzc[2], bzn[2], Rx[2], Ry[2], Rz[2], Rhx, Rhy, hx, hy;
	auto uPlane = [&](int p) { return (p < 0) ? bot.p : (p < N ? up2 + p * NP : top.p); }; // p = z0 - 1 .. N
	auto uScale = [&](int p) { return (p < 0) ? bot.s : (p < N ? 1.0 : top.s); };
	auto clampP = [&](int p) { return p < N ? p : N - 1; };
	auto zPl    = [&](int p) { return lo2 + 2 * (NNN / 2) + p * NP; }; // LO_z plane p < N
#pragma unroll
	for (int k = 0; k < 2; k++) {
		const double2 a  = uPlane(z0 - 1)[q[k]];
		const double  sm = uScale(z0 - 1);
		uc[k]  = double2{sm * a.x, sm * a.y};
		un[k]  = up2[z0 * NP + q[k]];
		bzn[k] = zPl(z0)[q[k]];
	}
	double hraw = hs.p[z0 * hs.stride];
	__builtin_amdgcn_sched_barrier(0);
#pragma unroll
	for (int i = 0; i < 2; i++) { // oldest first
#pragma unroll
		for (int k = 0; k < 2; k++) {
			ur[(i + 1) & 1][k] = uPlane(z0 + 1 + i)[q[k]];
			if (HAS_F) fr[i][k] = fp2[clampP(z0 + i) * NP + q[k]];
			if constexpr (SIG) sr[i][k] = sp2[clampP(z0 + i) * NP + q[k]];
		}
		__builtin_amdgcn_sched_barrier(0);
	}
#pragma unroll
	for (int k = 0; k < 2; k++) {
		Rx[k] = lo2[z0 * NP + q[k]];
		Ry[k] = lo2[NNN / 2 + z0 * NP + q[k]];
		Rz[k] = zPl(z0 + 1)[q[k]];
	}
	Rhx = hxp[z0 * hxs];
	Rhy = hyp[z0 * hys];
	__builtin_amdgcn_sched_barrier(0);
	double2 tz[2] = {}; // the coefficient plane above the slab

	auto step = [&](auto par, auto refill, int zz) {
		constexpr int  PAR    = decltype(par)::value; // zz & 1
		constexpr bool REFILL = decltype(refill)::value;
		constexpr bool FINAL  = !REFILL && PAR == 1; // the slab's last plane
		const int      z      = z0 + zz;
		const double   hv     = hs.s * takeReg(hraw);
		if (REFILL || PAR == 0) hraw = hs.p[clampP(z + 1) * hs.stride];
		__builtin_amdgcn_sched_barrier(0);
		const double sn = uScale(z + 1);
#pragma unroll
		for (int k = 0; k < 2; k++) {
			um[k] = uc[k];
			uc[k] = un[k];
			const double2 a = takeRegs(ur[1 - PAR][k]); // plane z + 1
			un[k]           = double2{sn * a.x, sn * a.y};
			if (HAS_F) fc[k] = takeRegs(fr[PAR][k]);
			if constexpr (SIG) sc[k] = takeRegs(sr[PAR][k]);
			bx[k]  = takeRegs(Rx[k]);
			by[k]  = takeRegs(Ry[k]);
			bzc[k] = bzn[k];
			bzn[k] = FINAL ? tz[k] : takeRegs(Rz[k]);
			if (REFILL) {
				ur[1 - PAR][k] = uPlane(z + 3)[q[k]];
				if (HAS_F) fr[PAR][k] = fp2[clampP(z + 2) * NP + q[k]];
				if constexpr (SIG) sr[PAR][k] = sp2[clampP(z + 2) * NP + q[k]];
				Rz[k] = zPl(z + 2)[q[k]];
			}
			if (REFILL || PAR == 0) {
				Rx[k] = lo2[clampP(z + 1) * NP + q[k]];
				Ry[k] = lo2[NNN / 2 + clampP(z + 1) * NP + q[k]];
			}
		}
		hx = takeRegs(Rhx);
		hy = takeRegs(Rhy);
		if (REFILL || PAR == 0) {
			Rhx = hxp[clampP(z + 1) * hxs];
			Rhy = hyp[clampP(z + 1) * hys];
		}

		double *tl = tile[PAR];
		if (act) {
			ldsStore2(tl + lds[0], uc[0]);
			ldsStore2(tl + lds[1], uc[1]);
		}
		if (hs.lds >= 0) tl[hs.lds] = hv;
		brow[PAR][tid] = by[0];
		ldsBarrier();

		const double2 ylo = ldsLoad2(tl + ldo[0]);
		const double2 yhi = ldsLoad2(tl + ldo[1]);
		const double2 byn = brow[PAR][tid + H]; // LO_y of row 2 Yp + 2 (the last row pair reads a slot nobody needs)
		const double2 byu = north ? hy : byn;
		// the next pair's lower x-face: the next lane (pairs of a row are consecutive lanes; the row's last pair takes HI_x)
		const double nx0 = __shfl_down(bx[0].x, 1), nx1 = __shfl_down(bx[1].x, 1);
		const double bxe[2] = {east ? hx.x : nx0, east ? hx.y : nx1};
		const double wb = (z == 0) ? wB : 1.0, wt = (z == N - 1) ? wT : 1.0;
		double2      r[2];
#pragma unroll
		for (int k = 0; k < 2; k++) {
			const double *t0 = tl + lds[k];
			const double2 c  = uc[k];
			const double2 ym = (k == 0) ? ylo : uc[0];
			const double2 yp = (k == 0) ? uc[1] : yhi;
			const double2 bl = by[k], bh = (k == 0) ? by[1] : byu;
			const double  xl = t0[-1], xr = t0[2];
			const double  bxl = bx[k].x, bxm = bx[k].y, bxh = bxe[k];
			double2       a;
			a.x = (bxm * (c.y - c.x) - bxl * (c.x - xl)) * rhx;
			a.y = (bxh * (xr - c.y) - bxm * (c.y - c.x)) * rhx;
			a.x += (bh.x * (yp.x - c.x) - bl.x * (c.x - ym.x)) * rhy;
			a.y += (bh.y * (yp.y - c.y) - bl.y * (c.y - ym.y)) * rhy;
			a.x += (bzn[k].x * (un[k].x - c.x) - bzc[k].x * (c.x - um[k].x)) * rhz;
			a.y += (bzn[k].y * (un[k].y - c.y) - bzc[k].y * (c.y - um[k].y)) * rhz;
			if constexpr (SIG) {
				a.x = a.x - sc[k].x * c.x;
				a.y = a.y - sc[k].y * c.y;
			}
			if (MODE == COEF_APPLY) {
				r[k] = a;
			} else if (MODE == COEF_RESID) {
				r[k].x = fc[k].x - a.x;
				r[k].y = fc[k].y - a.y;
			} else {
				const double ws = (k == 0) ? wS : 1.0, wn = (k == 1) ? wN : 1.0;
				double2      d;
				d.x = bxl * wW * rhx;
				d.x += bxm * 1.0 * rhx;
				d.y = bxm * 1.0 * rhx;
				d.y += bxh * wE * rhx;
				d.x += bl.x * ws * rhy;
				d.x += bh.x * wn * rhy;
				d.y += bl.y * ws * rhy;
				d.y += bh.y * wn * rhy;
				d.x += bzc[k].x * wb * rhz;
				d.x += bzn[k].x * wt * rhz;
				d.y += bzc[k].y * wb * rhz;
				d.y += bzn[k].y * wt * rhz;
				if constexpr (SIG) {
					d.x = d.x + sc[k].x;
					d.y = d.y + sc[k].y;
				}
				r[k].x = c.x + omega * (fc[k].x - a.x) / (-d.x);
				r[k].y = c.y + omega * (fc[k].y - a.y) / (-d.y);
			}
		}
		if (act) {
			op2[z * NP + q[0]] = r[0];
			op2[z * NP + q[1]] = r[1];
		}
	};
	using B0 = std::integral_constant<int, 0>;
	using B1 = std::integral_constant<int, 1>;
	static_assert(ZL % 2 == 0 && ZL >= 4, "the march is unrolled over the two ring slots and ends with two steps of its own");
#pragma unroll 1
	for (int zz = 0; zz < ZL - 2; zz += 2) {
		step(B0{}, std::true_type{}, zz);
		step(B1{}, std::true_type{}, zz + 1);
	}
	{ // requested two steps before the slab's last plane needs it
		const double2 *tp = last ? hi2 + NN : zPl(z0 + ZL);
#pragma unroll
		for (int k = 0; k < 2; k++) tz[k] = tp[q[k]];
	}
	__builtin_amdgcn_sched_barrier(0);
	step(B0{}, std::false_type{}, ZL - 2);
	step(B1{}, std::false_type{}, ZL - 1);
}

// PHASE 0: red cells relaxed from u, black cells copied; PHASE 1: black cells relaxed in `out` from the new red values there
template <int PHASE, bool SIG = false>
__global__ __launch_bounds__(256) void k_coef_rbgs2d(CoefLevel L, const double *__restrict__ u, const double *__restrict__ f, double *out,
                                                     const double *__restrict__ sigma = nullptr)
{
	const int    n = L.n, nc = n * n;
	const size_t total = (size_t) L.P * nc;
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int p = (int) (idx / nc), c = (int) (idx % nc);
		const int par = c % n + c / n;
		if ((par & 1) != PHASE) {
			if (PHASE == 0) out[idx] = u[idx];
			continue;
		}
		double o, d;
		coefCell2d<true>(L, u, (PHASE == 0 ? u : out) + (size_t) p * nc, p, c, 0.0, o, d);
		if constexpr (SIG) d = d + sigma[idx];
		out[idx] = (o - f[idx]) / d;
	}
}

// ---- 3D sweep: the lagged red/black march of k_rbgs3d (march3d.hpp) in its plain form, with the coefficient planes riding along.
// Plane z gets its red update from old black values, plane z - 1 then its black update from new red values: output lags one plane,
// one pass over u, f and beta (50.25 B/site at N = 32). Three LDS tiles rotate (planes z - 1, z, z + 1), one barrier per plane.
// Neighbour patches and ghost slots are read from the old iterate (haloSrc / zPlaneSrc with sign 0 on physical faces: they
// contribute 0 to o and kappa = 2 / 0 to d). ZS > 1: a slab recomputes the red values of the planes just below and above it, as
// k_rbgs3d does. beta of a plane -- LO_x, LO_y pairs, the thread's HI_x pair or (by shuffle) the next lane's LO_x, LO_y of the row
// above the pair (HI_y on the last row pair; straight from memory: the neighbouring thread asks for the same line) -- is
// requested one step ahead and kept for two steps (red of plane z, black of plane z at the next step); LO_z runs as a chain of
// four planes z - 1 .. z + 2, HI_z above the last. Every load of the loop is unconditional, from a pointer and stride chosen
// before the loop. d is formed per cell from the same planes (no table: it depends on beta).
//
// SIG (te_gmg_set_reaction): d + sigma_c in both updates. sigma runs beside f as gm / gc (planes z - 1, z): the
// red update of plane z and, one step later, the black update of the same plane read it. The pairs of plane z + 1 are requested at the
// END of step z, when those of plane z - 1 are dead, and consumed by step z + 1: two planes of sigma are live during the updates, not
// three (a third, requested at the top of the step as f's is, puts EVERY instantiation past 256 registers and at one wave per SIMD;
// this form only the ZS = 1 ones of N >= 8). The slab rule is unchanged. + 8 B/site. SIG = false is the kernel as it was.
struct BetaPlane {
	double2 bx[2], by[2], byu, hx; // LO_x, LO_y of the two rows; LO_y of the row above the pair / HI_y; HI_x of the two rows (east threads)
};
template <int N, int ZS, bool SIG = false>
__global__ __launch_bounds__(Tile3<N>::TPB) void k_coef_rbgs3d(LevelDev L, const double *__restrict__ beta, const double *__restrict__ u,
                                                               const double *__restrict__ f, double *__restrict__ out,
                                                               const double *__restrict__ sigma = nullptr)
{
	using T           = Tile3<N>;
	constexpr int TPB = T::TPB, NP = T::NP, H = T::H;
	constexpr int NN = N * N, NNN = N * N * N;
	constexpr int ZL = N / ZS;
	constexpr size_t FV = 3 * (size_t) NNN + 3 * NN;
	static_assert(ZL % 2 == 0 && ZL >= 2, "slabs start on even planes");
	const int nwork = L.count * ZS;
	const int work  = xcdRemap(blockIdx.x, nwork);
	if (work >= nwork) return;
	const int slot = work / ZS;
	const int z0 = (work % ZS) * ZL, z1 = z0 + ZL; // planes this workgroup stores
	const int zs = (z0 > 0) ? z0 - 1 : 0;          // first plane it relaxes (red only when zs < z0)
	const int pid = L.order ? L.order[L.first + slot] : L.first + slot;
	const int tid = threadIdx.x;

	__shared__ __attribute__((aligned(16))) double tile[3][T::LSZ]; // planes z-1, z, z+1 rotate

	const Reg6     fk(L.face_kind + (size_t) pid * 6), fs(L.face_src + (size_t) pid * 6);
	const double   rhx = L.rh2[(size_t) pid * 3], rhy = L.rh2[(size_t) pid * 3 + 1], rhz = L.rh2[(size_t) pid * 3 + 2];
	const double  *up  = u + (size_t) pid * NNN;
	const double2 *up2 = reinterpret_cast<const double2 *>(up);
	const double2 *fp2 = reinterpret_cast<const double2 *>(f + (size_t) pid * NNN);
	double2       *op2 = reinterpret_cast<double2 *>(out + (size_t) pid * NNN);
	const double2 *sp2 = reinterpret_cast<const double2 *>((SIG ? sigma : u) + (size_t) pid * NNN);
	const double2 *lo2 = reinterpret_cast<const double2 *>(beta + (size_t) pid * FV);
	const double2 *hi2 = reinterpret_cast<const double2 *>(beta + (size_t) pid * FV + 3 * (size_t) NNN);

	const HaloSrc  hs  = haloSrc<N>(tid, fk, fs, u, up, L.ghost, 0.0, 0.0, L.xf);
	const PlaneSrc bot = zPlaneSrc<N>(fk[4], fs[4], false, u, up, L.ghost, 0.0, 0.0);
	const PlaneSrc top = zPlaneSrc<N>(fk[5], fs[5], true, u, up, L.ghost, 0.0, 0.0);

	const bool act = (T::NT == TPB) || tid < T::NT;
	const int  X = act ? tid % H : 0, Yp = act ? tid / H : 0;
	int        q[2], lds[2];
	const int  ldo[2] = {T::row(2 * Yp) + 2 * X + 2, T::row(2 * Yp + 3) + 2 * X + 2};
#pragma unroll
	for (int k = 0; k < 2; k++) {
		q[k]   = (2 * Yp + k) * H + X;
		lds[k] = T::row(2 * Yp + k + 1) + 2 * X + 2;
	}
	const bool     east = X == H - 1, north = Yp == H - 1;
	const double2 *hxp = east ? hi2 + Yp : lo2;
	const int      hxs = east ? H : 0;
	const double2 *byp = north ? hi2 + NN / 2 + X : lo2 + NNN / 2 + (2 * Yp + 2) * H + X; // HI_y[x + N z], or LO_y of row 2 Yp + 2
	const int      bys = north ? H : NP;
	// kappa of the six sides where this thread's cells touch them
	auto         kap = [&](int s) { return fk[s] == FACE_DIRICHLET ? 2.0 : (fk[s] == FACE_NEUMANN ? 0.0 : 1.0); };
	const double wW = X == 0 ? kap(0) : 1.0, wE = east ? kap(1) : 1.0, wS = Yp == 0 ? kap(2) : 1.0, wN = north ? kap(3) : 1.0;
	const double wB = kap(4), wT = kap(5);

	auto loadSet = [&](BetaPlane &B, int p) { // p < N
#pragma unroll
		for (int k = 0; k < 2; k++) {
			B.bx[k] = lo2[p * NP + q[k]];
			B.by[k] = lo2[NNN / 2 + p * NP + q[k]];
		}
		B.byu = byp[p * bys];
		B.hx  = hxp[p * hxs];
	};
	auto zPlane = [&](int p) { return p < N ? lo2 + 2 * (NNN / 2) + p * NP : hi2 + NN; }; // LO_z plane p, HI_z above the last

	// planes: umm = z-2, um = z-1, uc = z, un = z+1, un2 = z+2 (values are updated in place); start at z = zs
	double2   umm[2], um[2], uc[2], un[2], un2[2], fm[2], fc[2], fn[2];
	double2   zm[2], zc[2], zn[2], zn2[2]; // LO_z of planes z-1, z, z+1, z+2
	double2   gm[2], gc[2];                // SIG: sigma of planes z-1, z
	BetaPlane Bm, Bc, Bn;
	double    bxeM[2] = {0.0, 0.0}, bxeC[2];
#pragma unroll
	for (int k = 0; k < 2; k++) {
		const double2 *pm = (zs > 0) ? up2 + (zs - 1) * NP : bot.p; // zs + 1 < N always (a slab has >= 2 planes)
		const double   sm = (zs > 0) ? 1.0 : bot.s;
		uc[k]     = up2[zs * NP + q[k]];
		double2 a = pm[q[k]];
		um[k]     = double2{sm * a.x, sm * a.y};
		un[k]     = up2[(zs + 1) * NP + q[k]];
		fc[k]     = fp2[zs * NP + q[k]];
		umm[k]    = double2{0.0, 0.0};
		fm[k]     = double2{0.0, 0.0};
		if constexpr (SIG) {
			gc[k] = sp2[zs * NP + q[k]];
			gm[k] = double2{0.0, 0.0};
		}
		zc[k]     = zPlane(zs)[q[k]];
		zn[k]     = zPlane(zs + 1)[q[k]];
		zm[k]     = double2{0.0, 0.0};
	}
	loadSet(Bc, zs);
	Bm = Bc; // (never used before it is replaced)
	double hv = hs.s * hs.p[zs * hs.stride];

	// relax cell CB (0: even x, 1: odd x) of row K of plane Z held in `cen` (LDS copy in tl): v = (o - f) / d
	auto relax = [&](auto kk, auto cbb, double *tl, int Z, double2(&cen)[2], const double2(&below)[2], const double2(&above)[2],
	                 const double2(&rhs)[2], const BetaPlane &B, const double(&bxe)[2], const double2(&zlo)[2], const double2(&zhi)[2],
	                 const double2(&sig)[2]) {
		constexpr int K = decltype(kk)::value, CB = decltype(cbb)::value;
		auto          c = [&](const double2 &v) { return CB ? v.y : v.x; };
		const double side  = CB ? tl[lds[K] + 2] : tl[lds[K] - 1]; // the x-neighbour outside the pair
		const double mate  = CB ? cen[K].x : cen[K].y;
		const double inner = c(cen[1 - K]);                                 // other row of the pair: a register
		const double outer = (K == 0) ? tl[ldo[0] + CB] : tl[ldo[1] + CB]; // row y-1 / y+2: LDS
		const double xl = CB ? mate : side, xr = CB ? side : mate;
		const double ym = (K == 0) ? outer : inner, yp = (K == 0) ? inner : outer;
		const double bxl = CB ? B.bx[K].y : B.bx[K].x, bxh = CB ? bxe[K] : B.bx[K].y;
		const double byl = c(B.by[K]), byh = (K == 0) ? c(B.by[1]) : c(B.byu);
		const double bzl = c(zlo[K]), bzh = c(zhi[K]);
		const double wxl = CB ? 1.0 : wW, wxh = CB ? wE : 1.0, wyl = (K == 0) ? wS : 1.0, wyh = (K == 0) ? 1.0 : wN;
		const double wzl = (Z == 0) ? wB : 1.0, wzh = (Z == N - 1) ? wT : 1.0;
		double       o = bxl * xl * rhx;
		o += bxh * xr * rhx;
		o += byl * ym * rhy;
		o += byh * yp * rhy;
		o += bzl * c(below[K]) * rhz;
		o += bzh * c(above[K]) * rhz;
		double d = bxl * wxl * rhx;
		d += bxh * wxh * rhx;
		d += byl * wyl * rhy;
		d += byh * wyh * rhy;
		d += bzl * wzl * rhz;
		d += bzh * wzh * rhz;
		if constexpr (SIG) d = d + c(sig[K]);
		const double v = (o - c(rhs[K])) / d;
		if (CB)
			cen[K].y = v;
		else
			cen[K].x = v;
		if (act) tl[lds[K] + CB] = v;
	};
	using I0 = std::integral_constant<int, 0>;
	using I1 = std::integral_constant<int, 1>;

	int bz = 0; // z % 3
	// one plane step; ZPAR = z & 1 is a compile-time constant so that every cell's colour is static
	auto step = [&](auto zpar, int z) {
		constexpr int ZPAR = decltype(zpar)::value;
		// the next step's loads (clamped / redirected on the last steps)
		const int      zc1 = (z + 1 < N) ? z + 1 : N - 1;
		const double2 *pn  = (z + 2 < N) ? up2 + (z + 2) * NP : top.p;
		const double   sn  = (z + 2 < N) ? 1.0 : top.s;
		const double2 *pz  = zPlane(z + 2 < N ? z + 2 : N);
#pragma unroll
		for (int k = 0; k < 2; k++) {
			const double2 a = pn[q[k]];
			un2[k]          = double2{sn * a.x, sn * a.y};
			fn[k]           = fp2[zc1 * NP + q[k]];
			zn2[k]          = pz[q[k]];
		}
		const double hvn = hs.s * hs.p[zc1 * hs.stride];
		loadSet(Bn, zc1);
		double *tz = tile[bz];                   // plane z
		double *tm = tile[bz == 0 ? 2 : bz - 1]; // plane z-1
		if (z < N) {
			if (act) {
				ldsStore2(tz + lds[0], uc[0]);
				ldsStore2(tz + lds[1], uc[1]);
			}
			if (hs.lds >= 0) tz[hs.lds] = hv;
		}
		// one barrier per plane: buffer z%3 was last read two steps ago (black of plane z-3)
		ldsBarrier();
		// the upper x-face of the pair: the next lane's LO_x (pairs of a row are consecutive lanes), HI_x on the row's last pair
		const double n0 = __shfl_down(Bc.bx[0].x, 1), n1 = __shfl_down(Bc.bx[1].x, 1);
		bxeC[0] = east ? Bc.hx.x : n0;
		bxeC[1] = east ? Bc.hx.y : n1;
		if (z < N) { // red cells of plane z from old black values: cell parity = (0 + k + z) & 1
			relax(I0{}, std::integral_constant<int, (0 + ZPAR) & 1>{}, tz, z, uc, um, un, fc, Bc, bxeC, zc, zn, gc);
			relax(I1{}, std::integral_constant<int, (1 + ZPAR) & 1>{}, tz, z, uc, um, un, fc, Bc, bxeC, zc, zn, gc);
		}
		if (z > z0) { // black cells of plane z-1 from new red values (the plane below a slab only lends its red values)
			relax(I0{}, std::integral_constant<int, (1 + 0 + 1 - ZPAR) & 1>{}, tm, z - 1, um, umm, uc, fm, Bm, bxeM, zm, zc, gm);
			relax(I1{}, std::integral_constant<int, (1 + 1 + 1 - ZPAR) & 1>{}, tm, z - 1, um, umm, uc, fm, Bm, bxeM, zm, zc, gm);
			if (act) {
				op2[(z - 1) * NP + q[0]] = um[0];
				op2[(z - 1) * NP + q[1]] = um[1];
			}
		}
#pragma unroll
		for (int k = 0; k < 2; k++) {
			umm[k] = um[k];
			um[k]  = uc[k];
			uc[k]  = un[k];
			un[k]  = un2[k];
			fm[k]  = fc[k];
			fc[k]  = fn[k];
			if constexpr (SIG) {
				gm[k] = gc[k];
				gc[k] = sp2[zc1 * NP + q[k]]; // plane z + 1, for the next step
			}
			zm[k]  = zc[k];
			zc[k]  = zn[k];
			zn[k]  = zn2[k];
			bxeM[k] = bxeC[k];
		}
		Bm = Bc;
		Bc = Bn;
		hv = hvn;
		bz = (bz == 2) ? 0 : bz + 1;
	};
	if (ZS > 1 && z0 > 0) step(I1{}, z0 - 1); // red values of the plane below the slab
#pragma unroll 1
	for (int z = z0; z < z1; z += 2) {
		step(I0{}, z);
		step(I1{}, z + 1);
	}
	step(I0{}, z1); // black update and store of the last plane (and, inside a patch, the red values above it)
}

// ---- 2D sweep for patches that fit in LDS (n <= 64: (n + 2)^2 doubles): one workgroup per patch, the patch and its ghost ring in
// LDS, both colours in one launch, as k_rbgs2d_lds. The ring holds the frozen ghosts of the old iterate (0 on physical faces);
// the same sums, in the same order, as k_coef_rbgs2d<0> + <1>. beta and f come from global memory (every entry is read by the one
// or two cells that use it). Dynamic LDS: (n + 2)^2 doubles.
template <bool SIG = false>
static __global__ __launch_bounds__(256) void k_coef_rbgs2d_lds(CoefLevel L, const double *__restrict__ u, const double *__restrict__ f,
                                                                double *__restrict__ out, const double *__restrict__ sigma = nullptr)
{
	extern __shared__ double t2[];
	const int     n = L.n, nn = n * n, W = n + 2, h = n / 2, p = blockIdx.x, tid = threadIdx.x, TPB = blockDim.x;
	const size_t  FV = 2 * (size_t) nn + 2 * n;
	const double *up = u + (size_t) p * nn, *fp = f + (size_t) p * nn, *bp = L.beta + (size_t) p * FV;
	const double  rhx = L.rh2[(size_t) p * 3], rhy = L.rh2[(size_t) p * 3 + 1];
	int           kind[4];
	double        kap[4];
#pragma unroll
	for (int s = 0; s < 4; s++) {
		kind[s] = L.face_kind[p * 4 + s];
		kap[s]  = kind[s] == FACE_DIRICHLET ? 2.0 : (kind[s] == FACE_NEUMANN ? 0.0 : 1.0);
	}
	for (int i = tid; i < nn; i += TPB) t2[(i / n + 1) * W + i % n + 1] = up[i];
	for (int i = tid; i < 4 * n; i += TPB) { // the ring: side s at face coordinate t
		const int s = i / n, t = i % n, src = L.face_src[p * 4 + s];
		double    g = 0.0; // physical faces contribute nothing to o
		if (kind[s] == FACE_GHOST) g = L.ghost[(size_t) src * n + t];
		if (kind[s] == FACE_LOCAL) g = u[(size_t) src * nn + (s == 0 ? (n - 1) + n * t : (s == 1 ? n * t : (s == 2 ? t + n * (n - 1) : t)))];
		t2[s == 0 ? (t + 1) * W : (s == 1 ? (t + 1) * W + n + 1 : (s == 2 ? t + 1 : (n + 1) * W + t + 1))] = g;
	}
	__syncthreads();
#pragma unroll 1
	for (int colour = 0; colour < 2; colour++) {
		for (int i = tid; i < n * h; i += TPB) {
			const int    y = i / h, x = 2 * (i % h) + ((y + colour) & 1), c = x + n * y;
			double      *tc = t2 + (y + 1) * W + x + 1;
			const double bxl = bp[c], bxh = x < n - 1 ? bp[c + 1] : bp[2 * nn + y];
			const double byl = bp[nn + c], byh = y < n - 1 ? bp[nn + c + n] : bp[2 * nn + n + x];
			double       o = bxl * tc[-1] * rhx;
			o += bxh * tc[1] * rhx;
			o += byl * tc[-W] * rhy;
			o += byh * tc[W] * rhy;
			double d = bxl * (x == 0 ? kap[0] : 1.0) * rhx;
			d += bxh * (x == n - 1 ? kap[1] : 1.0) * rhx;
			d += byl * (y == 0 ? kap[2] : 1.0) * rhy;
			d += byh * (y == n - 1 ? kap[3] : 1.0) * rhy;
			if constexpr (SIG) d = d + sigma[(size_t) p * nn + c];
			tc[0] = (o - fp[c]) / d;
		}
		__syncthreads();
	}
	for (int i = tid; i < nn; i += TPB) out[(size_t) p * nn + i] = t2[(i / n + 1) * W + i % n + 1];
}

// ---- the coefficient on the next level
template <int N>
__global__ __launch_bounds__(256) void k_faces_restrict3d(int Pc, const int32_t *__restrict__ child, const int32_t *__restrict__ copy,
                                                          const double *__restrict__ fine, double *__restrict__ coarse)
{
	constexpr int    H = N / 2, NP = N * N / 2, NN = N * N, NNN = N * N * N;
	constexpr size_t FV = 3 * (size_t) NNN + 3 * NN;
	const int        pc = blockIdx.x, tid = threadIdx.x, TPB = blockDim.x;
	if (pc >= Pc) return;
	double2 *lo2 = reinterpret_cast<double2 *>(coarse + (size_t) pc * FV);
	double2 *hi2 = reinterpret_cast<double2 *>(coarse + (size_t) pc * FV + 3 * (size_t) NNN);
	if (copy[pc]) {
		const double2 *e2 = reinterpret_cast<const double2 *>(fine + (size_t) child[(size_t) pc * 8] * FV);
		for (int i = tid; i < (int) (FV / 2); i += TPB) lo2[i] = e2[i];
		return;
	}
	auto ch = [&](int ox, int oy, int oz) { return fine + (size_t) child[(size_t) pc * 8 + ox + 2 * oy + 4 * oz] * FV; };
	for (int i = tid; i < N * NP; i += TPB) { // a pair of coarse faces per component: both lie in one child (N / 2 is even)
		const int     x = 2 * (i % H), y = (i / H) % N, z = i / NP;
		const int     ox = x >= H, oy = y >= H, oz = z >= H;
		const double *q = ch(ox, oy, oz) + (2 * x - ox * N) + N * (2 * y - oy * N) + NN * (2 * z - oz * N);
		lo2[i]                 = coarsenPairX<N>(q);
		lo2[NNN / 2 + i]       = coarsenPairT(q + NNN, NN);
		lo2[2 * (NNN / 2) + i] = coarsenPairT(q + 2 * NNN, N);
	}
	for (int i = tid; i < N * H; i += TPB) { // HI_x by (y, z), HI_y by (x, z), HI_z by (x, y): the upper children's HI blocks
		const int t = 2 * (i % H), w = i / H;
		const int ot = t >= H, ow = w >= H;
		const int f = (2 * t - ot * N) + N * (2 * w - ow * N);
		hi2[i]          = coarsenPairT(ch(1, ot, ow) + 3 * NNN + f, N);
		hi2[NN / 2 + i] = coarsenPairT(ch(ot, 1, ow) + 3 * NNN + NN + f, N);
		hi2[NN + i]     = coarsenPairT(ch(ot, ow, 1) + 3 * NNN + 2 * NN + f, N);
	}
}

static __global__ __launch_bounds__(256) void k_faces_restrict2d(int n, int Pc, const int32_t *__restrict__ child, const int32_t *__restrict__ copy,
                                                                 const double *__restrict__ fine, double *__restrict__ coarse)
{
	const int    h = n / 2, nn = n * n;
	const size_t total = (size_t) Pc * n * h, FV = 2 * (size_t) nn + 2 * n;
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int      pc = (int) (idx / ((size_t) n * h)), q = (int) (idx % ((size_t) n * h));
		const int      y = q / h, x = 2 * (q % h);
		const int32_t *row = child + (size_t) pc * 4;
		const bool     cp = copy[pc] != 0;
		double        *dp = coarse + (size_t) pc * FV;
		auto value = [&](int a, int I, int t) { // F_a(I; t) of the coarse patch (coarsenFace2d's rule with the level's child table)
			if (cp) return face2d(fine + (size_t) row[0] * FV, n, a, I, t);
			const int     oa = I >= h, ob = t >= h;
			const double *e = fine + (size_t) row[a == 0 ? oa + 2 * ob : ob + 2 * oa] * FV;
			return faceMean2(face2d(e, n, a, 2 * I - oa * n, 2 * t - ob * n), face2d(e, n, a, 2 * I - oa * n, 2 * t - ob * n + 1));
		};
		*reinterpret_cast<double2 *>(dp + x + n * y)      = double2{value(0, x, y), value(0, x + 1, y)};
		*reinterpret_cast<double2 *>(dp + nn + x + n * y) = double2{value(1, y, x), value(1, y, x + 1)};
		if (x + 2 == n) dp[2 * nn + y] = value(0, n, y);
		if (y == n - 1) *reinterpret_cast<double2 *>(dp + 2 * nn + n + x) = double2{value(1, n, x), value(1, n, x + 1)};
	}
}

// ---- the coefficient on the next level when children live on other ranks. A child whose parent is not local
// restricts ITSELF: its block is the face vector of a patch of m = n / 2 cells per axis (LO_a, a = 0 .. D-1, m^D each, then HI_a,
// m^(D-1) each) -- every coarse face the child covers, its own lower plane 0 and its own HI_a included -- or, for a patch that
// copies through, its n-cell face vector bit for bit. The parent's rank then only picks entries: nothing is averaged twice and
// nothing is averaged on the other side of the wire, so every coarse entry is faceMean4 / faceMean2 of the same fine faces in the
// same order as k_faces_restrict3d / 2d form it from a local child.

// doubles of a face vector per patch of m cells per axis
template <int D> __device__ __forceinline__ int faceVecSize(int m) { return D == 3 ? 3 * m * m * m + 3 * m * m : 2 * m * m + 2 * m; }

// entry e of the face vector of m = n / 2 cells per axis that the fine patch fp (n cells per axis) restricts to
template <int D> __device__ __forceinline__ double packedFaceEntry(const double *__restrict__ fp, int n, int e)
{
	const int m = n / 2, nn = n * n;
	const int mc = D == 3 ? m * m * m : m * m, mf = D == 3 ? m * m : m;
	const int nc = D == 3 ? nn * n : nn, nf = D == 3 ? nn : n;
	if (e < D * mc) { // LO_a[c]: the fine LO_a faces of plane 2 c_a over the 2^(D-1) fine positions of the remaining axes
		const int a = e / mc, c = e % mc;
		if (D == 3) {
			const double *q  = fp + (size_t) a * nc + 2 * (c % m) + n * 2 * ((c / m) % m) + nn * 2 * (c / (m * m));
			const int     s0 = a == 0 ? n : 1, s1 = a == 2 ? n : nn; // strides of the lower / higher remaining axis
			return faceMean4(q[0], q[s0], q[s1], q[s0 + s1]);
		}
		const double *q = fp + (size_t) a * nc + 2 * (c % m) + n * 2 * (c / m);
		return faceMean2(q[0], q[a == 0 ? n : 1]);
	}
	const int     h = e - D * mc, a = h / mf, t = h % mf; // HI_a[t]: the same over the fine patch's HI_a block
	const double *q = fp + (size_t) D * nc + (size_t) a * nf;
	if (D == 3) {
		q += 2 * (t % m) + n * 2 * (t / m);
		return faceMean4(q[0], q[1], q[n], q[n + 1]);
	}
	return faceMean2(q[2 * t], q[2 * t + 1]);
}

// one workgroup per up block (fine patch, orthant or -1) of the level's transfer tables: out + foff[block] <- the block
template <int D>
__device__ __forceinline__ void facesPackBlock(int n, const int32_t *__restrict__ desc, const int64_t *__restrict__ foff, const double *__restrict__ fine,
                                               double *__restrict__ out)
{
	const int     b = blockIdx.x, tid = threadIdx.x, TPB = blockDim.x;
	const int     p = desc[2 * b], o = desc[2 * b + 1];
	const int     FVn = faceVecSize<D>(n), FVm = faceVecSize<D>(n / 2);
	const double *fp  = fine + (size_t) p * FVn;
	double       *dst = out + foff[b];
	if (o < 0) { // a patch that copies through: bit for bit
		for (int i = tid; i < FVn; i += TPB) dst[i] = fp[i];
		return;
	}
	for (int e = tid; e < FVm; e += TPB) dst[e] = packedFaceEntry<D>(fp, n, e);
}
template <int N>
__global__ __launch_bounds__(256) void k_faces_restrict_pack3d(const int32_t *__restrict__ desc, const int64_t *__restrict__ foff,
                                                               const double *__restrict__ fine, double *__restrict__ out)
{
	facesPackBlock<3>(N, desc, foff, fine, out);
}
static __global__ __launch_bounds__(256) void k_faces_restrict_pack2d(int n, const int32_t *__restrict__ desc, const int64_t *__restrict__ foff,
                                                                      const double *__restrict__ fine, double *__restrict__ out)
{
	facesPackBlock<2>(n, desc, foff, fine, out);
}

// The coarse side on a rank that received blocks: entry e of coarse patch pc (row = its children, >= 0 a local fine patch, <= -2
// block -(row[o] + 2) of recv at foff). The child that covers a coarse face (a, I, t): o_a = (I >= m), the other bits from t; in its
// restricted face vector the face is local plane I - o_a m of LO_a -- for I = m that is plane 0 of the UPPER child -- and for
// I = n the upper child's HI_a. A local child: packedFaceEntry of its fine patch, the bits of k_faces_restrict3d / 2d.
template <int D>
__device__ __forceinline__ double coarseFaceEntry(int n, const int32_t *__restrict__ row, bool cp, const double *__restrict__ fine,
                                                  const double *__restrict__ recv, const int64_t *__restrict__ foff, int e)
{
	const int m = n / 2, nn = n * n, FVn = faceVecSize<D>(n);
	const int mc = D == 3 ? m * m * m : m * m, mf = D == 3 ? m * m : m;
	const int nc = D == 3 ? nn * n : nn, nf = D == 3 ? nn : n;
	if (cp) {
		const int ch = row[0];
		return ch >= 0 ? fine[(size_t) ch * FVn + e] : recv[foff[-(ch + 2)] + e];
	}
	int o, em;
	if (e < D * nc) {
		const int a = e / nc, c = e % nc;
		const int cx = c % n, cy = D == 3 ? (c / n) % n : c / n, cz = D == 3 ? c / nn : 0;
		const int ox = cx >= m, oy = cy >= m, oz = cz >= m;
		o  = ox + 2 * oy + 4 * oz;
		em = a * mc + (cx - ox * m) + m * (cy - oy * m) + m * m * (cz - oz * m);
	} else {
		const int h = e - D * nc, a = h / nf, t = h % nf;
		const int t0 = D == 3 ? t % n : t, t1 = D == 3 ? t / n : 0; // the remaining axes, the lower one first
		const int o0 = t0 >= m, o1 = t1 >= m;
		if (D == 3)
			o = a == 0 ? 1 + 2 * o0 + 4 * o1 : (a == 1 ? o0 + 2 + 4 * o1 : o0 + 2 * o1 + 4);
		else
			o = a == 0 ? 1 + 2 * o0 : o0 + 2;
		em = D * mc + a * mf + (t0 - o0 * m) + m * (t1 - o1 * m);
	}
	const int ch = row[o];
	return ch >= 0 ? packedFaceEntry<D>(fine + (size_t) ch * FVn, n, em) : recv[foff[-(ch + 2)] + em];
}

// one thread per coarse entry, in address order: one writer per entry, stores along x
template <int D>
__device__ __forceinline__ void facesRestrictRecv(int n, int Pc, const int32_t *__restrict__ child, const int32_t *__restrict__ copy,
                                                  const double *__restrict__ fine, const double *__restrict__ recv, const int64_t *__restrict__ foff,
                                                  double *__restrict__ coarse)
{
	const size_t FVn = (size_t) faceVecSize<D>(n), total = (size_t) Pc * FVn;
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int pc = (int) (idx / FVn), e = (int) (idx % FVn);
		coarse[idx]  = coarseFaceEntry<D>(n, child + (size_t) pc * (1 << D), copy[pc] != 0, fine, recv, foff, e);
	}
}
template <int N>
__global__ __launch_bounds__(256) void k_faces_restrict_recv3d(int Pc, const int32_t *__restrict__ child, const int32_t *__restrict__ copy,
                                                               const double *__restrict__ fine, const double *__restrict__ recv,
                                                               const int64_t *__restrict__ foff, double *__restrict__ coarse)
{
	facesRestrictRecv<3>(N, Pc, child, copy, fine, recv, foff, coarse);
}
static __global__ __launch_bounds__(256) void k_faces_restrict_recv2d(int n, int Pc, const int32_t *__restrict__ child, const int32_t *__restrict__ copy,
                                                                      const double *__restrict__ fine, const double *__restrict__ recv,
                                                                      const int64_t *__restrict__ foff, double *__restrict__ coarse)
{
	facesRestrictRecv<2>(n, Pc, child, copy, fine, recv, foff, coarse);
}
} // namespace te
