// A variable-density projection step on the device: face coefficients from a cell field, the weighted
// projection U -= alpha (w (.) grad p) in one pass, and the fold of boundary data under a face weight. Nothing in the reference
// computes these; they close the time step around the variable-coefficient solve of coefkernels.hpp. Vector layouts: projkernels.hpp
// (face vector), bckernels.hpp (boundary vector).
//
//   faces_from_cells   every LO_a / HI_a entry from the two operands of its face, lo on the lower-coordinate side, hi on the upper:
//                        TE_FACE_MEAN        (lo + hi) * 0.5
//                        TE_FACE_HARMONIC    (2.0 * (lo * hi)) / (lo + hi)
//                        TE_FACE_RECIP_MEAN  2.0 / (lo + hi)
//                      interior face, same-level neighbour: the two adjacent cells (both stored copies get the same bits);
//                      physical face: v = the boundary vector's entry (cb) or, without one, the cell just inside -- v itself for the
//                      first two modes, 1.0 / v for the third, whatever the side's kind (a coefficient has no boundary condition);
//                      coarse/fine face: plain averages, NOT the operator's ghost 2 gamma - m (its weights of -1/12 can turn a
//                      positive field negative across a jump): on the fine side the coarse cell that covers the face, on the coarse
//                      side ((f00 + f10) + (f01 + f11)) * 0.25 of the four fine cells that cover the coarse cell (2D: (f0 + f1) * 0.5).
//                      These operands come from the level's ghost slots, filled by k_cf_raw3d / k_cf_raw2d (single rank).
//   project_weighted   U = fma(-alpha, w * G, U), G exactly te_gradient's value (k_gradient3d's expressions), never stored
//   boundary_rhs_w     k_boundary_rhs with the datum multiplied first by w on that physical face
//
// 3D: the plane marches of projkernels.hpp (one workgroup per patch or z-slab, a thread owns a 2x2 column, cell planes in a
// register ring requested two steps ahead, x/y neighbours through the LDS tile). Nothing a step requests is consumed by the same
// step; every load of the loop is unconditional, from a pointer chosen before the loop.
// k_wproject3d streams U and w beside the cell planes. A second ring as deep as k_gradient3d<N, true>'s for U (a set in flight and
// a copy being consumed) does not fit in the register budget, so each of the two streams keeps ONE live set: a step consumes the
// set of its plane in its stores and only then requests the next plane's into the same registers -- a whole step ahead of its use.
//
// Algorithmic bytes per site, n = 32, 3D (a face layer is 1/32 of a patch):
//   faces_from_cells   read 8 + 6/32 * 8 = 9.5,              written 24.75             -> 34.25
//   project_weighted   read 9.5 + 24.75 (U) + 24.75 (w),     written 24.75             -> 83.75
//
// FMA contraction is off for this file: the expressions above are evaluated as written, the one fma is explicit.
#pragma once
#include "projkernels.hpp"
#include "bckernels.hpp"

namespace te
{
#pragma clang fp contract(off)

enum FaceMode : int { FACE_MODE_MEAN = 0, FACE_MODE_HARMONIC = 1, FACE_MODE_RECIP_MEAN = 2 };

// the value on a face with operands lo (lower-coordinate side) and hi
__device__ __forceinline__ double faceValue(int mode, double lo, double hi)
{
	const double s = lo + hi;
	if (mode == FACE_MODE_MEAN) return s * 0.5;
	const double num = mode == FACE_MODE_HARMONIC ? 2.0 * (lo * hi) : 2.0;
	return num / s;
}
// ... on a physical face with the one value v
__device__ __forceinline__ double faceValuePhys(int mode, double v) { return mode == FACE_MODE_RECIP_MEAN ? 1.0 / v : v; }

// Ghost slots of the coarse/fine faces for te_faces_from_cells: the raw coarse cell (fine side) or the four-cell average (coarse
// side) instead of k_cf_ghost3d's 2 gamma - m. One workgroup per coarse/fine face, desc / slots as for k_cf_ghost3d. A neighbour
// on another rank (desc < 0) does not occur: the entry point refuses a sharded hierarchy.
template <int N>
__global__ void k_cf_raw3d(const int32_t *__restrict__ desc, const int32_t *__restrict__ slots, const double *__restrict__ c, double *__restrict__ ghost)
{
	constexpr int  NN = N * N, NNN = N * N * N;
	const int32_t *d = desc + (size_t) blockIdx.x * 8;
	const int      s = d[1], kind = d[2], q = d[3];
	const int      ax = s >> 1;
	const int      sa = (ax == 0) ? N : 1, sb = (ax == 2) ? N : NN, sn = (ax == 0) ? 1 : (ax == 1 ? N : NN);
	const int      oth = (s & 1) ? 0 : (N - 1) * sn; // the neighbour's facing layer
	double        *g = ghost + (size_t) slots[blockIdx.x] * NN;
	for (int i = threadIdx.x; i < NN; i += blockDim.x) {
		const int a = i % N, b = i / N;
		if (kind == 2) {
			const int ca = (a + ((q & 1) ? N : 0)) / 2, cb = (b + ((q & 2) ? N : 0)) / 2;
			if (d[4] >= 0) g[i] = c[(size_t) d[4] * NNN + oth + ca * sa + cb * sb];
		} else {
			const int qa = (a >= N / 2), qb = (b >= N / 2);
			const int nbq = d[4 + qa + 2 * qb];
			const int fa = 2 * (a - qa * (N / 2)), fb = 2 * (b - qb * (N / 2));
			if (nbq >= 0) {
				const double *f = c + (size_t) nbq * NNN + oth + fa * sa + fb * sb;
				g[i]            = ((f[0] + f[sa]) + (f[sb] + f[sa + sb])) * 0.25;
			}
		}
	}
}

// F = the face values of the cell field c: the march and the store pattern of k_gradient3d<N, false, ZS>. The halo value of a
// physical side is the boundary vector's entry where one is given, else the cell just inside; which sides are physical is uniform
// per patch (pW .. pT).
template <int N, int ZS>
__global__ __launch_bounds__(Tile3<N>::TPB) void k_cellface3d(LevelDev L, FaceGeom fg, const double *__restrict__ c, double *__restrict__ F, int mode)
{
	using T           = Tile3<N>;
	constexpr int TPB = T::TPB, NP = T::NP, H = T::H;
	constexpr int NN = N * N, NNN = N * N * N;
	constexpr int ZL = N / ZS;
	constexpr size_t FV = 3 * (size_t) NNN + 3 * NN;
	const int nblocks = L.count * ZS;
	const int work    = xcdRemap(blockIdx.x, nblocks);
	if (work >= nblocks) return;
	const int pid = L.order ? L.order[L.first + work / ZS] : L.first + work / ZS;
	const int z0  = (work % ZS) * ZL;
	const int tid = threadIdx.x;
	const bool last = z0 + ZL == N;

	__shared__ __attribute__((aligned(16))) double tile[2][T::LSZ];

	const Reg6     fk(L.face_kind + (size_t) pid * 6), fs(L.face_src + (size_t) pid * 6);
	const bool     has_b = fg.bdata != nullptr;
	const Reg6     bf(has_b ? fg.bface + (size_t) pid * 6 : L.face_kind + (size_t) pid * 6);
	const double  *cp  = c + (size_t) pid * NNN;
	const double2 *cp2 = reinterpret_cast<const double2 *>(cp);
	double        *Fp  = F + (size_t) pid * FV;
	double2       *lo2 = reinterpret_cast<double2 *>(Fp);
	double2       *hi2 = reinterpret_cast<double2 *>(Fp + 3 * (size_t) NNN);

	const bool act = (T::NT == TPB) || tid < T::NT;
	const int  X = act ? tid % H : 0, Yp = act ? tid / H : 0;
	int        q[2], lds[2];
	const int  ldo[2] = {T::row(2 * Yp) + 2 * X + 2, T::row(2 * Yp + 3) + 2 * X + 2};
#pragma unroll
	for (int k = 0; k < 2; k++) {
		q[k]   = (2 * Yp + k) * H + X;
		lds[k] = T::row(2 * Yp + k + 1) + 2 * X + 2;
	}
	auto phys = [](int kind) { return kind == FACE_DIRICHLET || kind == FACE_NEUMANN; };
	const bool pW = phys(fk[0]) && X == 0, pE = phys(fk[1]), pS = phys(fk[2]) && Yp == 0, pN = phys(fk[3]);
	const bool pB = phys(fk[4]), pT = phys(fk[5]);
	const bool east = act && X == H - 1, north = act && Yp == H - 1;

	// halos, all taken as they are: a neighbour's cell, a ghost slot, the boundary vector's entry or the own cell
	HaloSrc hs = haloSrc<N>(tid, fk, fs, c, cp, L.ghost, 1.0, 1.0);
	if (tid < 4 * N && has_b) {
		const int side = tid / N, t = tid % N, b = bf[side];
		if (phys(fk[side]) && b >= 0) hs.p = fg.bdata + (size_t) b * NN + t, hs.stride = N;
	}
	PlaneSrc bot = zPlaneSrc<N>(fk[4], fs[4], false, c, cp, L.ghost, 1.0, 1.0);
	PlaneSrc top = zPlaneSrc<N>(fk[5], fs[5], true, c, cp, L.ghost, 1.0, 1.0);
	if (has_b) {
		if (pB && bf[4] >= 0) bot.p = reinterpret_cast<const double2 *>(fg.bdata + (size_t) bf[4] * NN);
		if (pT && bf[5] >= 0) top.p = reinterpret_cast<const double2 *>(fg.bdata + (size_t) bf[5] * NN);
	}

	// ---- register pipeline over z: um, uc = planes z-1, z; planes z+1, z+2 in flight in a two-slot ring (plane p in slot p & 1)
	double2 um[2], uc[2], ur[2][2];
	auto clampP = [&](int p) { return p < N ? p : N - 1; };
	{
		const double2 *pm = z0 == 0 ? bot.p : cp2 + (z0 - 1) * NP;
#pragma unroll
		for (int k = 0; k < 2; k++) uc[k] = pm[q[k]];
	}
	double hraw = hs.p[z0 * hs.stride];
	__builtin_amdgcn_sched_barrier(0);
#pragma unroll
	for (int i = 0; i < 2; i++) {
#pragma unroll
		for (int k = 0; k < 2; k++) ur[i][k] = cp2[(z0 + i) * NP + q[k]];
		__builtin_amdgcn_sched_barrier(0);
	}
	auto pair = [&](double2 lo, double2 hi) { return double2{faceValue(mode, lo.x, hi.x), faceValue(mode, lo.y, hi.y)}; };
	auto pairPhys = [&](double2 v) { return double2{faceValuePhys(mode, v.x), faceValuePhys(mode, v.y)}; };

	auto step = [&](auto par, auto refill, int zz) {
		constexpr int  PAR    = decltype(par)::value;
		constexpr bool REFILL = decltype(refill)::value;
		const int      z      = z0 + zz;
		const double   hv     = takeReg(hraw);
		if (REFILL || PAR == 0) hraw = hs.p[clampP(z + 1) * hs.stride];
		__builtin_amdgcn_sched_barrier(0);
#pragma unroll
		for (int k = 0; k < 2; k++) {
			um[k] = uc[k];
			uc[k] = takeRegs(ur[PAR][k]);
			if (REFILL) ur[PAR][k] = cp2[(z + 2) * NP + q[k]];
		}

		double *tl = tile[PAR];
		if (act) {
			ldsStore2(tl + lds[0], uc[0]);
			ldsStore2(tl + lds[1], uc[1]);
		}
		if (hs.lds >= 0) tl[hs.lds] = hv;
		ldsBarrier();

		const double2 ylo = ldsLoad2(tl + ldo[0]);
		const double2 yhi = ldsLoad2(tl + ldo[1]);
		const bool    zb  = pB && z == 0;
		double        hx[2];
#pragma unroll
		for (int k = 0; k < 2; k++) {
			const double *t0 = tl + lds[k];
			const double2 v  = uc[k];
			const double2 ym = (k == 0) ? ylo : uc[0];
			const double  xl = t0[-1], xr = t0[2];
			double2       fx, fy, fz;
			fx.x = pW ? faceValuePhys(mode, xl) : faceValue(mode, xl, v.x);
			fx.y = faceValue(mode, v.x, v.y);
			fy   = (k == 0 && pS) ? pairPhys(ym) : pair(ym, v);
			fz   = zb ? pairPhys(um[k]) : pair(um[k], v);
			hx[k] = pE ? faceValuePhys(mode, xr) : faceValue(mode, v.y, xr);
			if (act) {
				lo2[z * NP + q[k]]                 = fx;
				lo2[NNN / 2 + z * NP + q[k]]       = fy;
				lo2[2 * (NNN / 2) + z * NP + q[k]] = fz;
			}
		}
		if (east) hi2[Yp + H * z] = double2{hx[0], hx[1]}; // HI_x[y + N z], rows 2 Yp and 2 Yp + 1
		if (north) hi2[NN / 2 + X + H * z] = pN ? pairPhys(yhi) : pair(uc[1], yhi); // HI_y[x + N z]
	};
	using B0 = std::integral_constant<int, 0>;
	using B1 = std::integral_constant<int, 1>;
	static_assert(ZL % 2 == 0 && ZL >= 4, "the march is unrolled over the two ring slots and ends with two steps of its own");
#pragma unroll 1
	for (int zz = 0; zz < ZL - 2; zz += 2) {
		step(B0{}, std::true_type{}, zz);
		step(B1{}, std::true_type{}, zz + 1);
	}
	// the plane above the patch is requested two steps before the last slab needs it
	double2 tp[2];
#pragma unroll
	for (int k = 0; k < 2; k++) tp[k] = top.p[q[k]];
	__builtin_amdgcn_sched_barrier(0);
	step(B0{}, std::false_type{}, ZL - 2);
	step(B1{}, std::false_type{}, ZL - 1);
	if (last && act) {
#pragma unroll
		for (int k = 0; k < 2; k++) hi2[NN + q[k]] = pT ? pairPhys(tp[k]) : pair(uc[k], tp[k]); // HI_z[x + N y]
	}
}

// U = fma(-alpha, w * G, U), G = k_gradient3d's value: its march and its expressions, with U's and w's three LO planes and their
// HI_x / HI_y pairs streamed beside the cell planes, one live set each (see the head of this file).
template <int N, int ZS>
__global__ __launch_bounds__(Tile3<N>::TPB) void k_wproject3d(LevelDev L, FaceGeom fg, const double *__restrict__ u, const double *__restrict__ w,
                                                               double *U, double alpha)
{
	using T           = Tile3<N>;
	constexpr int TPB = T::TPB, NP = T::NP, H = T::H;
	constexpr int NN = N * N, NNN = N * N * N;
	constexpr int ZL = N / ZS;
	constexpr size_t FV = 3 * (size_t) NNN + 3 * NN;
	const int nblocks = L.count * ZS;
	const int work    = xcdRemap(blockIdx.x, nblocks);
	if (work >= nblocks) return;
	const int pid = L.order ? L.order[L.first + work / ZS] : L.first + work / ZS;
	const int z0  = (work % ZS) * ZL;
	const int tid = threadIdx.x;
	const bool last = z0 + ZL == N;

	__shared__ __attribute__((aligned(16))) double tile[2][T::LSZ];

	const Reg6     fk(L.face_kind + (size_t) pid * 6), fs(L.face_src + (size_t) pid * 6);
	const bool     has_b = fg.bdata != nullptr;
	const Reg6     bf(has_b ? fg.bface + (size_t) pid * 6 : L.face_kind + (size_t) pid * 6);
	const double   ihx = 1.0 / fg.h[(size_t) pid * 3], ihy = 1.0 / fg.h[(size_t) pid * 3 + 1], ihz = 1.0 / fg.h[(size_t) pid * 3 + 2];
	const double  *up  = u + (size_t) pid * NNN;
	const double2 *up2 = reinterpret_cast<const double2 *>(up);
	double2       *lo2 = reinterpret_cast<double2 *>(U + (size_t) pid * FV); // LO_a plane z: lo2[a * NNN / 2 + z * NP + q]
	double2       *hi2 = reinterpret_cast<double2 *>(U + (size_t) pid * FV + 3 * (size_t) NNN);
	const double2 *wlo = reinterpret_cast<const double2 *>(w + (size_t) pid * FV);
	const double2 *whi = reinterpret_cast<const double2 *>(w + (size_t) pid * FV + 3 * (size_t) NNN);

	const bool act = (T::NT == TPB) || tid < T::NT;
	const int  X = act ? tid % H : 0, Yp = act ? tid / H : 0;
	int        q[2], lds[2];
	const int  ldo[2] = {T::row(2 * Yp) + 2 * X + 2, T::row(2 * Yp + 3) + 2 * X + 2};
#pragma unroll
	for (int k = 0; k < 2; k++) {
		q[k]   = (2 * Yp + k) * H + X;
		lds[k] = T::row(2 * Yp + k + 1) + 2 * X + 2;
	}
	// a Neumann face carries its datum itself: these threads take the halo value instead of a difference
	const bool nW = fk[0] == FACE_NEUMANN && X == 0, nE = fk[1] == FACE_NEUMANN, nS = fk[2] == FACE_NEUMANN && Yp == 0, nN = fk[3] == FACE_NEUMANN;
	const bool nB = fk[4] == FACE_NEUMANN, nT = fk[5] == FACE_NEUMANN;
	const bool east = act && X == H - 1, north = act && Yp == H - 1;

	// halos: Dirichlet ghost = -m + 2 g, Neumann "ghost" = g_n, a neighbour's cell or a ghost slot as it is
	HaloSrc  hs = haloSrc<N>(tid, fk, fs, u, up, L.ghost, -1.0, 0.0, L.xf);
	BHaloSrc hb{up, 0, 0.0};
	if (tid < 4 * N && has_b) {
		const int side = tid / N, t = tid % N, kind = fk[side], b = bf[side];
		if (kind == FACE_DIRICHLET && b >= 0) hb.p = fg.bdata + (size_t) b * NN + t, hb.stride = N, hb.s = 2.0;
		if (kind == FACE_NEUMANN && b >= 0) hs.p = fg.bdata + (size_t) b * NN + t, hs.stride = N, hs.s = 1.0;
	}
	PlaneSrc bot = zPlaneSrc<N>(fk[4], fs[4], false, u, up, L.ghost, -1.0, 0.0);
	PlaneSrc top = zPlaneSrc<N>(fk[5], fs[5], true, u, up, L.ghost, -1.0, 0.0);
	PlaneSrc botb{up2, 0.0}, topb{up2, 0.0};
	if (has_b) {
		if (fk[4] == FACE_DIRICHLET && bf[4] >= 0) botb.p = reinterpret_cast<const double2 *>(fg.bdata + (size_t) bf[4] * NN), botb.s = 2.0;
		if (fk[4] == FACE_NEUMANN && bf[4] >= 0) bot.p = reinterpret_cast<const double2 *>(fg.bdata + (size_t) bf[4] * NN), bot.s = 1.0;
		if (fk[5] == FACE_DIRICHLET && bf[5] >= 0) topb.p = reinterpret_cast<const double2 *>(fg.bdata + (size_t) bf[5] * NN), topb.s = 2.0;
		if (fk[5] == FACE_NEUMANN && bf[5] >= 0) top.p = reinterpret_cast<const double2 *>(fg.bdata + (size_t) bf[5] * NN), top.s = 1.0;
	}
	// where this thread's HI_x / HI_y pairs sit, as an offset into a HI block (the threads that own none: entry 0, stride 0, of LO)
	const int hxo = east ? Yp : 0, hyo = north ? NN / 2 + X : 0;
	const int hxs = east ? H : 0, hys = north ? H : 0;
	const double2 *Uhxp = east ? hi2 : lo2, *Uhyp = north ? hi2 : lo2;
	const double2 *Whxp = east ? whi : wlo, *Whyp = north ? whi : wlo;

	// ---- register pipeline over z: um, uc = planes z-1, z; planes z+1, z+2 in flight in a two-slot ring (plane p in slot p & 1).
	// Ul, Wl, Uhx .. Why: U's and w's values of the plane the NEXT step stores, requested by the step before, behind its own stores.
	double2 um[2], uc[2], ur[2][2];
	double2 Ul[3][2], Wl[3][2], Uhx, Uhy, Whx, Why;
	auto clampP = [&](int p) { return p < N ? p : N - 1; };
	{
		const double2 *pm = z0 == 0 ? bot.p : up2 + (z0 - 1) * NP;
		const double   sm = z0 == 0 ? bot.s : 1.0, sb = z0 == 0 ? botb.s : 0.0;
#pragma unroll
		for (int k = 0; k < 2; k++) {
			const double2 a = pm[q[k]], b = botb.p[q[k]];
			uc[k] = double2{sm * a.x + sb * b.x, sm * a.y + sb * b.y};
		}
	}
	double hraw = hs.p[z0 * hs.stride], braw = hb.p[z0 * hb.stride];
	__builtin_amdgcn_sched_barrier(0);
#pragma unroll
	for (int i = 0; i < 2; i++) {
#pragma unroll
		for (int k = 0; k < 2; k++) ur[i][k] = up2[(z0 + i) * NP + q[k]];
		__builtin_amdgcn_sched_barrier(0);
	}
	auto request = [&](int z) { // U and w of plane z
#pragma unroll
		for (int a = 0; a < 3; a++)
#pragma unroll
			for (int k = 0; k < 2; k++) {
				Ul[a][k] = lo2[a * (NNN / 2) + z * NP + q[k]];
				Wl[a][k] = wlo[a * (NNN / 2) + z * NP + q[k]];
			}
		Uhx = Uhxp[hxo + z * hxs];
		Whx = Whxp[hxo + z * hxs];
		Uhy = Uhyp[hyo + z * hys];
		Why = Whyp[hyo + z * hys];
	};
	request(z0);
	__builtin_amdgcn_sched_barrier(0);
	auto upd = [&](double2 Uv, double2 wv, double2 g) { // U - alpha (w g): one product, one fma, the same on every path
		const double tx = wv.x * g.x, ty = wv.y * g.y;
		return double2{__builtin_fma(-alpha, tx, Uv.x), __builtin_fma(-alpha, ty, Uv.y)};
	};

	auto step = [&](auto par, auto refill, auto more, int zz) {
		constexpr int  PAR    = decltype(par)::value;
		constexpr bool REFILL = decltype(refill)::value;
		constexpr bool MORE   = decltype(more)::value; // another step of this slab follows
		const int      z      = z0 + zz;
		const double   hv     = hs.s * takeReg(hraw) + hb.s * takeReg(braw);
		if (REFILL || PAR == 0) {
			hraw = hs.p[clampP(z + 1) * hs.stride];
			braw = hb.p[clampP(z + 1) * hb.stride];
		}
		__builtin_amdgcn_sched_barrier(0);
#pragma unroll
		for (int k = 0; k < 2; k++) {
			um[k] = uc[k];
			uc[k] = takeRegs(ur[PAR][k]);
			if (REFILL) ur[PAR][k] = up2[(z + 2) * NP + q[k]];
		}

		double *tl = tile[PAR];
		if (act) {
			ldsStore2(tl + lds[0], uc[0]);
			ldsStore2(tl + lds[1], uc[1]);
		}
		if (hs.lds >= 0) tl[hs.lds] = hv;
		ldsBarrier();

		const double2 ylo = ldsLoad2(tl + ldo[0]);
		const double2 yhi = ldsLoad2(tl + ldo[1]);
		const bool    zb  = nB && z == 0;
		double        hx[2];
#pragma unroll
		for (int k = 0; k < 2; k++) {
			const double *t0 = tl + lds[k];
			const double2 c  = uc[k];
			const double2 ym = (k == 0) ? ylo : uc[0];
			const double  xl = t0[-1], xr = t0[2];
			double2       gx, gy, gz;
			gx.x = nW ? xl : (c.x - xl) * ihx;
			gx.y = (c.y - c.x) * ihx;
			gy.x = (k == 0 && nS) ? ym.x : (c.x - ym.x) * ihy;
			gy.y = (k == 0 && nS) ? ym.y : (c.y - ym.y) * ihy;
			gz.x = zb ? um[k].x : (c.x - um[k].x) * ihz;
			gz.y = zb ? um[k].y : (c.y - um[k].y) * ihz;
			hx[k] = nE ? xr : (xr - c.y) * ihx;
			if (act) {
				lo2[z * NP + q[k]]                 = upd(Ul[0][k], Wl[0][k], gx);
				lo2[NNN / 2 + z * NP + q[k]]       = upd(Ul[1][k], Wl[1][k], gy);
				lo2[2 * (NNN / 2) + z * NP + q[k]] = upd(Ul[2][k], Wl[2][k], gz);
			}
		}
		if (east) hi2[Yp + H * z] = upd(Uhx, Whx, double2{hx[0], hx[1]}); // HI_x[y + N z], rows 2 Yp and 2 Yp + 1
		if (north) {
			double2 gy;
			gy.x = nN ? yhi.x : (yhi.x - uc[1].x) * ihy;
			gy.y = nN ? yhi.y : (yhi.y - uc[1].y) * ihy;
			hi2[NN / 2 + X + H * z] = upd(Uhy, Why, gy); // HI_y[x + N z]
		}
		// this plane's U and w are consumed: the next plane's into the same registers, one step ahead of their use
		__builtin_amdgcn_sched_barrier(0);
		if (MORE) request(z + 1);
		__builtin_amdgcn_sched_barrier(0);
	};
	using B0 = std::integral_constant<int, 0>;
	using B1 = std::integral_constant<int, 1>;
	static_assert(ZL % 2 == 0 && ZL >= 4, "the march is unrolled over the two ring slots and ends with two steps of its own");
#pragma unroll 1
	for (int zz = 0; zz < ZL - 2; zz += 2) {
		step(B0{}, std::true_type{}, std::true_type{}, zz);
		step(B1{}, std::true_type{}, std::true_type{}, zz + 1);
	}
	// the plane above the patch (and its boundary data, and U's and w's HI_z) is requested two steps before the last slab needs it
	double2 tp[2], tb[2], Ut[2], Wt[2];
#pragma unroll
	for (int k = 0; k < 2; k++) {
		tp[k] = top.p[q[k]];
		tb[k] = topb.p[q[k]];
		Ut[k] = hi2[NN + q[k]];
		Wt[k] = whi[NN + q[k]];
	}
	__builtin_amdgcn_sched_barrier(0);
	step(B0{}, std::false_type{}, std::true_type{}, ZL - 2);
	step(B1{}, std::false_type{}, std::false_type{}, ZL - 1);
	if (last && act) {
#pragma unroll
		for (int k = 0; k < 2; k++) {
			const double2 t{top.s * tp[k].x + topb.s * tb[k].x, top.s * tp[k].y + topb.s * tb[k].y};
			double2       gz;
			gz.x = nT ? t.x : (t.x - uc[k].x) * ihz;
			gz.y = nT ? t.y : (t.y - uc[k].y) * ihz;
			hi2[NN + q[k]] = upd(Ut[k], Wt[k], gz); // HI_z[x + N y]
		}
	}
}

// ---- 2D twins, in the simple form of k_gradient2d: one thread per pair of x-adjacent cells, neighbours from global memory.
// ghost slots of the coarse/fine faces, raw (k_cf_ghost2d's descriptors): the coarse cell, or (f0 + f1) * 0.5
static __global__ void k_cf_raw2d(int n, const int32_t *__restrict__ desc, const int32_t *__restrict__ slots, const double *__restrict__ c,
                                  double *__restrict__ ghost)
{
	const int32_t *d = desc + (size_t) blockIdx.x * 8;
	const int      s = d[1], kind = d[2], q = d[3];
	const int      ax = s >> 1;
	const int      sa = (ax == 0) ? n : 1, sn = (ax == 0) ? 1 : n;
	const int      oth = (s & 1) ? 0 : (n - 1) * sn;
	double        *g = ghost + (size_t) slots[blockIdx.x] * n;
	for (int a = threadIdx.x; a < n; a += blockDim.x) {
		if (kind == 2) {
			const int ca = (a + (q ? n : 0)) / 2;
			if (d[4] >= 0) g[a] = c[(size_t) d[4] * n * n + oth + ca * sa];
		} else {
			const int qa = (a >= n / 2), nbq = d[4 + qa];
			const int fa = 2 * (a - qa * (n / 2));
			if (nbq >= 0) {
				const double *f = c + (size_t) nbq * n * n + oth + fa * sa;
				g[a]            = (f[0] + f[sa]) * 0.5;
			}
		}
	}
}

// the face value on side s of patch p at face coordinate t, m = the cell just inside
__device__ __forceinline__ double faceCell2d(const Level2D &L, const FaceGeom &fg, const double *c, int mode, int p, int s, int t, double m)
{
	const int n = L.n, kind = L.face_kind[p * 4 + s];
	if (kind == FACE_DIRICHLET || kind == FACE_NEUMANN) {
		const int b = fg.bdata ? fg.bface[p * 4 + s] : -1;
		return faceValuePhys(mode, b >= 0 ? fg.bdata[(size_t) b * n + t] : m);
	}
	const double o = ghost2d(L, c, p, s, t, m, false); // the neighbour's cell or the ghost slot
	return (s & 1) ? faceValue(mode, m, o) : faceValue(mode, o, m);
}
static __global__ __launch_bounds__(256) void k_cellface2d(Level2D L, FaceGeom fg, const double *__restrict__ c, double *__restrict__ F, int mode)
{
	const int    n = L.n, h = n / 2;
	const size_t total = (size_t) L.P * n * h, FV = 2 * (size_t) n * n + 2 * n;
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int     p = (int) (idx / ((size_t) n * h)), q = (int) (idx % ((size_t) n * h));
		const int     y = q / h, x = 2 * (q % h);
		const double *cp = c + (size_t) p * n * n;
		double       *Fp = F + (size_t) p * FV;
		const double2 v  = *reinterpret_cast<const double2 *>(cp + x + n * y);
		double2       fx, fy;
		fx.x = (x > 0) ? faceValue(mode, cp[x - 1 + n * y], v.x) : faceCell2d(L, fg, c, mode, p, 0, y, v.x);
		fx.y = faceValue(mode, v.x, v.y);
		if (y > 0) {
			const double2 ym = *reinterpret_cast<const double2 *>(cp + x + n * (y - 1));
			fy = double2{faceValue(mode, ym.x, v.x), faceValue(mode, ym.y, v.y)};
		} else {
			fy = double2{faceCell2d(L, fg, c, mode, p, 2, x, v.x), faceCell2d(L, fg, c, mode, p, 2, x + 1, v.y)};
		}
		*reinterpret_cast<double2 *>(Fp + x + n * y)                  = fx;
		*reinterpret_cast<double2 *>(Fp + (size_t) n * n + x + n * y) = fy;
		if (x + 2 == n) Fp[2 * (size_t) n * n + y] = faceCell2d(L, fg, c, mode, p, 1, y, v.y);
		if (y == n - 1)
			*reinterpret_cast<double2 *>(Fp + 2 * (size_t) n * n + n + x) =
			    double2{faceCell2d(L, fg, c, mode, p, 3, x, v.x), faceCell2d(L, fg, c, mode, p, 3, x + 1, v.y)};
	}
}

// k_gradient2d<true> with the weight: w is read where U is
static __global__ __launch_bounds__(256) void k_wproject2d(Level2D L, FaceGeom fg, const double *__restrict__ u, const double *__restrict__ w, double *U,
                                                    double alpha)
{
	const int    n = L.n, h = n / 2;
	const size_t total = (size_t) L.P * n * h, FV = 2 * (size_t) n * n + 2 * n;
	auto         upd = [&](double Uv, double wv, double g) {
		const double t = wv * g;
		return __builtin_fma(-alpha, t, Uv);
	};
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int     p = (int) (idx / ((size_t) n * h)), q = (int) (idx % ((size_t) n * h));
		const int     y = q / h, x = 2 * (q % h);
		const double *up = u + (size_t) p * n * n;
		double       *Up = U + (size_t) p * FV;
		const double *wp = w + (size_t) p * FV;
		const double  ihx = 1.0 / fg.h[(size_t) p * 3], ihy = 1.0 / fg.h[(size_t) p * 3 + 1];
		const double2 c = *reinterpret_cast<const double2 *>(up + x + n * y);
		double2       gx, gy;
		gx.x = (x > 0) ? (c.x - up[x - 1 + n * y]) * ihx : faceGrad2d(L, fg, u, p, 0, y, c.x, ihx);
		gx.y = (c.y - c.x) * ihx;
		if (y > 0) {
			const double2 ym = *reinterpret_cast<const double2 *>(up + x + n * (y - 1));
			gy = double2{(c.x - ym.x) * ihy, (c.y - ym.y) * ihy};
		} else {
			gy = double2{faceGrad2d(L, fg, u, p, 2, x, c.x, ihy), faceGrad2d(L, fg, u, p, 2, x + 1, c.y, ihy)};
		}
		const size_t  ix = x + (size_t) n * y, iy = (size_t) n * n + x + (size_t) n * y;
		double2      *ox = reinterpret_cast<double2 *>(Up + ix), *oy = reinterpret_cast<double2 *>(Up + iy);
		const double2 Ux = *ox, Uy = *oy;
		const double2 wx = *reinterpret_cast<const double2 *>(wp + ix), wy = *reinterpret_cast<const double2 *>(wp + iy);
		*ox = double2{upd(Ux.x, wx.x, gx.x), upd(Ux.y, wx.y, gx.y)};
		*oy = double2{upd(Uy.x, wy.x, gy.x), upd(Uy.y, wy.y, gy.y)};
		if (x + 2 == n) {
			const size_t i = 2 * (size_t) n * n + y;
			Up[i]          = upd(Up[i], wp[i], faceGrad2d(L, fg, u, p, 1, y, c.y, ihx));
		}
		if (y == n - 1) {
			const size_t  i  = 2 * (size_t) n * n + n + x;
			double2      *o  = reinterpret_cast<double2 *>(Up + i);
			const double2 Uh = *o, wh = *reinterpret_cast<const double2 *>(wp + i);
			*o = double2{upd(Uh.x, wh.x, faceGrad2d(L, fg, u, p, 3, x, c.x, ihy)), upd(Uh.y, wh.y, faceGrad2d(L, fg, u, p, 3, x + 1, c.y, ihy))};
		}
	}
}

// k_boundary_rhs (bckernels.hpp) with b <- w_face * b first: w_face = LO_a of the layer's cell on a lower side, HI_a at the datum's
// place in the block on an upper side. Owner rule, side order and the one-writer guarantee as there.
template <int D>
__global__ __launch_bounds__(256) void k_boundary_rhs_w(BcGeom G, const double *__restrict__ bdata, const double *__restrict__ w, double *__restrict__ f)
{
	constexpr int NS = 2 * D;
	const int     n = G.n, p = blockIdx.x / NS, s = blockIdx.x % NS;
	if (p >= G.P) return;
	// which sides are physical / Neumann, as bit masks (the two table rows themselves are read again where a term is formed: twelve
	// uniform values held across the loop do not fit in the scalar registers next to the addresses)
	const int32_t *bfrow = G.bface + (size_t) p * NS;
	int            physm = 0, neum = 0;
#pragma unroll
	for (int t = 0; t < NS; t++) {
		physm |= (bfrow[t] >= 0) << t;
		neum |= (G.face_kind[(size_t) p * NS + t] == FACE_NEUMANN) << t;
	}
	if (!physm) return; // (an interior patch)
	int nf = 1, nc = 1;
#pragma unroll
	for (int a = 0; a < D; a++) {
		nc *= n;
		if (a) nf *= n;
	}
	const double *h  = G.h + (size_t) p * 3;
	const double *wp = w + (size_t) p * ((size_t) D * nc + (size_t) D * nf);
	for (int j = threadIdx.x; j < nf; j += 256) {
		int ci[D];
		bcFaceCell<D>(n, s, j, ci);
		bool owner = true, touched = false;
#pragma unroll
		for (int t = 0; t < NS; t++) {
			const bool on = ci[t >> 1] == ((t & 1) ? n - 1 : 0);
			if (t < s && on) owner = false;
			touched |= on && ((physm >> t) & 1);
		}
		if (!owner || !touched) continue;
		size_t c = 0, m = 1;
#pragma unroll
		for (int a = 0; a < D; a++) {
			c += m * ci[a];
			m *= n;
		}
		const size_t at = (size_t) p * nc + c;
		double       v  = f[at];
#pragma unroll
		for (int t = 0; t < NS; t++) {
			const int ax = t >> 1, hi = t & 1;
			if (ci[ax] != (hi ? n - 1 : 0) || !((physm >> t) & 1)) continue;
			const int    pos = bcBlockPos<D>(n, t, ci);
			const double wf  = hi ? wp[(size_t) D * nc + (size_t) ax * nf + pos] : wp[(size_t) ax * nc + c];
			const double b   = wf * bdata[(size_t) bfrow[t] * nf + pos];
			if ((neum >> t) & 1) {
				const double g = b / h[ax];
				v              = hi ? v - g : v + g;
			} else {
				v -= 2 * b / (h[ax] * h[ax]);
			}
		}
		f[at] = v;
	}
}
} // namespace te
