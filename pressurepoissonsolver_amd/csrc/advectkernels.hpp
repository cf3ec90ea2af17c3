// Conservative upwind transport of a cell field by a MAC face velocity: the donor-cell flux F = U (.) c_upwind
// as a face vector, the update out = c - alpha div(U c_upwind) in one pass, the matching of a face vector's coarse/fine copies, and
// the largest |U_a| / h_a of a face vector. Nothing in the reference computes these; they close the variable-density step of
// densitykernels.hpp around the solve. Vector layouts: projkernels.hpp (face vector), bckernels.hpp (boundary vector).
//
//   flux of a face     lo, hi = the operands on the lower- and the upper-coordinate side, U = this patch's stored entry of the face:
//                        s = (U >= 0.0) ? lo : hi,  F = U * s
//                      interior face, same-level neighbour: the two adjacent cells (te_faces_from_cells' operands; both stored
//                      copies get the same bits when U's copies agree);
//                      physical face, Dirichlet or Neumann alike: outside the domain stands the boundary vector's entry (cb) or,
//                      without one, the cell just inside; inside stands that cell -- inflow carries the datum, outflow the cell;
//                      coarse/fine face, fine side: the other operand is the coarse cell that covers the face (k_cf_raw3d's kind 2);
//                      coarse/fine face, coarse side: ((F00 + F10) + (F01 + F11)) * 0.25 (2D: (F0 + F1) * 0.5) of the fine-side
//                      fluxes of the covering fine faces, first index along the face's lower remaining axis -- each formed here
//                      from the fine patch's own copy of U, its facing-layer cell and this coarse cell, the operands and the
//                      expression of the fine side: the coarse copy IS the mean of the fine copies, bit for bit. The coarse copy
//                      of U on such a face is never read.
//                      Both sides of a coarse/fine face come from the level's ghost slots, which k_cf_flux3d / k_cf_flux2d fill with
//                      these FLUXES (one workgroup per coarse/fine face, k_cf_ghost3d's descriptors; single rank).
//   advect             out = c - d, d = te_divergence(alpha, F)'s value (k_divergence3d / k_divergence2d), F never stored
//   faces_match        on a coarse/fine face the coarse side's entries <- faceMean4 / faceMean2 of the covering fine copies
//   faces_max_rate     max |U_a| / h_a over all stored entries
//
// 3D, advectMarch<N, ZS, FUSED>: the plane march of k_cellface3d (one workgroup per patch or z-slab, a thread owns a 2x2 column, cell
// planes in a register ring requested two steps ahead, x/y neighbours through the LDS tile) with U's three LO planes, the thread's
// HI_x pair and the U_y pair of the row above its column (LO_y of row 2 Yp + 2, HI_y on the last row pair) streamed beside them by
// k_wproject3d's one-live-set rule: a step forms its fluxes from the set and only then requests the next plane's into the same
// registers, a whole step ahead of its use. Nothing a step requests is consumed by the same step; every load of the loop is
// unconditional, from a pointer chosen before the loop. FUSED: the upper x flux of a pair is the next lane's lower one (HI_x on the
// row's last pair), the upper y flux is formed by the thread itself from the row above (the same operands, the same expression as
// that row's owner), the upper z flux is the next plane's lower one -- so plane z - 1 is stored by step z, and the last plane behind
// the march with the plane above the slab (LO_z of the next slab's first plane, or HI_z).
//
// Algorithmic bytes per site, n = 32, 3D (a face layer is 1/32 of a patch):
//   advect_flux   read 8 + 6/32 * 8 = 9.5 and 24.75 (U),   written 24.75    -> 59
//   advect        read 9.5 + 24.75,                         written 8        -> 42.25   (the three-call composition: about 116)
//
// FMA contraction is off for this file: the expressions above are evaluated as written; the fma's of the divergence are explicit.
#pragma once
#include "projkernels.hpp"
#include "bckernels.hpp"
#include "faceregridkernels.hpp" // faceMean4 / faceMean2 (and FMA contraction is off from there to the end of the unit)

namespace te
{
#pragma clang fp contract(off)

// the donor-cell flux of a face with operands lo (lower-coordinate side) and hi
__device__ __forceinline__ double upwindFlux(double U, double lo, double hi)
{
	const double s = (U >= 0.0) ? lo : hi;
	return U * s;
}
__device__ __forceinline__ double2 upwindFlux2(double2 U, double2 lo, double2 hi)
{
	return double2{upwindFlux(U.x, lo.x, hi.x), upwindFlux(U.y, lo.y, hi.y)};
}

// te_divergence's value of a cell before alpha, from the flux differences along x, y, z. k_divergence3d writes
// (dx * ihx + dy * ihy) + dz * ihz and is compiled with FMA contraction on; what the compiler makes of it is one product, rounded,
// and two fma's, and WHICH of the first two products stays a product differs between the four cells of a thread's 2x2 column
// (read in the generated code of all ten instantiations; tests/test_gpu_advect.py holds the fused kernel to te_divergence's bits):
//   YFIRST = false   fma(dz, ihz, fma(dx, ihx, dy * ihy))     the cells with even x
//   YFIRST = true    fma(dz, ihz, fma(dy, ihy, dx * ihx))     odd x in the column's first row; in its second row for N >= 16 only
template <bool YFIRST> __device__ __forceinline__ double divPart(double dx, double dy, double ihx, double ihy)
{
	return YFIRST ? __builtin_fma(dy, ihy, dx * ihx) : __builtin_fma(dx, ihx, dy * ihy);
}

// Ghost slots of the coarse/fine faces for te_advect_flux / te_advect: the face's flux. One workgroup per coarse/fine face, desc /
// slots as for k_cf_ghost3d. A neighbour on another rank (desc < 0) does not occur: the entry points refuse a sharded hierarchy.
template <int N>
__global__ void k_cf_flux3d(const int32_t *__restrict__ desc, const int32_t *__restrict__ slots, const double *__restrict__ U,
                            const double *__restrict__ c, double *__restrict__ ghost)
{
	constexpr int    NN = N * N, NNN = N * N * N;
	constexpr size_t FV = 3 * (size_t) NNN + 3 * NN;
	const int32_t   *d = desc + (size_t) blockIdx.x * 8;
	const int        p = d[0], s = d[1], kind = d[2], q = d[3];
	const int        ax = s >> 1, up = s & 1;
	const int        sa = (ax == 0) ? N : 1, sb = (ax == 2) ? N : NN, sn = (ax == 0) ? 1 : (ax == 1 ? N : NN);
	const int        mine = up ? (N - 1) * sn : 0, oth = up ? 0 : (N - 1) * sn; // my face layer, the neighbour's facing layer
	double          *g  = ghost + (size_t) slots[blockIdx.x] * NN;
	const double    *cm = c + (size_t) p * NNN + mine;
	// patch r's stored entry of its lower (upper = 0) or upper a-face at face point (a, b)
	auto faceU = [&](int r, int upper, int a, int b) {
		const double *Ur = U + (size_t) r * FV;
		return upper ? Ur[3 * (size_t) NNN + ax * NN + a + N * b] : Ur[(size_t) ax * NNN + a * sa + b * sb];
	};
	for (int i = threadIdx.x; i < NN; i += blockDim.x) {
		const int    a = i % N, b = i / N;
		const double m = cm[a * sa + b * sb];
		if (kind == 2) {
			const int ca = (a + ((q & 1) ? N : 0)) / 2, cb = (b + ((q & 2) ? N : 0)) / 2;
			if (d[4] < 0) continue;
			const double C = c[(size_t) d[4] * NNN + oth + ca * sa + cb * sb], Uf = faceU(p, up, a, b);
			g[i]           = up ? upwindFlux(Uf, m, C) : upwindFlux(Uf, C, m);
		} else {
			const int qa = (a >= N / 2), qb = (b >= N / 2);
			const int nbq = d[4 + qa + 2 * qb];
			const int fa = 2 * (a - qa * (N / 2)), fb = 2 * (b - qb * (N / 2));
			if (nbq < 0) continue;
			const double *f = c + (size_t) nbq * NNN + oth + fa * sa + fb * sb;
			double        F[2][2]; // [along a][along b]: the fine side's fluxes (the fine patch's side is s ^ 1)
#pragma unroll
			for (int bb = 0; bb < 2; bb++)
#pragma unroll
				for (int aa = 0; aa < 2; aa++) {
					const double Uf = faceU(nbq, !up, fa + aa, fb + bb), fc = f[aa * sa + bb * sb];
					F[aa][bb]       = up ? upwindFlux(Uf, m, fc) : upwindFlux(Uf, fc, m);
				}
			g[i] = faceMean4(F[0][0], F[1][0], F[0][1], F[1][1]);
		}
	}
}

// te_faces_match: the coarse side's stored entries of every coarse/fine face <- the mean of the covering fine copies. One workgroup
// per coarse/fine face (the fine sides return at once); an entry has one writer, and no entry that is written is read.
template <int N> __global__ void k_faces_match3d(const int32_t *__restrict__ desc, double *F)
{
	constexpr int    NN = N * N, NNN = N * N * N;
	constexpr size_t FV = 3 * (size_t) NNN + 3 * NN;
	const int32_t   *d = desc + (size_t) blockIdx.x * 8;
	const int        p = d[0], s = d[1], kind = d[2];
	if (kind != 3) return;
	const int ax = s >> 1, up = s & 1;
	const int sa = (ax == 0) ? N : 1, sb = (ax == 2) ? N : NN;
	for (int i = threadIdx.x; i < NN; i += blockDim.x) {
		const int a = i % N, b = i / N;
		const int qa = (a >= N / 2), qb = (b >= N / 2);
		const int nbq = d[4 + qa + 2 * qb];
		const int fa = 2 * (a - qa * (N / 2)), fb = 2 * (b - qb * (N / 2));
		if (nbq < 0) continue;
		const double *Ff = F + (size_t) nbq * FV;
		double        v;
		if (up) { // the fine patches' lower a-faces: LO_a of their first layer
			const double *f = Ff + (size_t) ax * NNN + fa * sa + fb * sb;
			v               = faceMean4(f[0], f[sa], f[sb], f[sa + sb]);
		} else { // their HI_a blocks
			const double *f = Ff + 3 * (size_t) NNN + ax * NN + fa + N * fb;
			v               = faceMean4(f[0], f[1], f[N], f[N + 1]);
		}
		double *Fp = F + (size_t) p * FV;
		if (up)
			Fp[3 * (size_t) NNN + ax * NN + a + N * b] = v;
		else
			Fp[(size_t) ax * NNN + a * sa + b * sb] = v;
	}
}

// The march of te_advect_flux (FUSED = false: out is the face vector F) and of te_advect (FUSED = true: out is the cell vector).
template <int N, int ZS, bool FUSED>
__device__ __forceinline__ void advectMarch(const LevelDev &L, const FaceGeom &fg, const double *__restrict__ c, const double *__restrict__ U,
                                            double *__restrict__ out, double alpha)
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
	const double  *cp  = c + (size_t) pid * NNN;
	const double2 *cp2 = reinterpret_cast<const double2 *>(cp);
	const double2 *ulo = reinterpret_cast<const double2 *>(U + (size_t) pid * FV); // LO_a plane z: ulo[a * NNN / 2 + z * NP + q]
	const double2 *uhi = reinterpret_cast<const double2 *>(U + (size_t) pid * FV + 3 * (size_t) NNN);
	double2       *lo2 = reinterpret_cast<double2 *>(out + (size_t) pid * FV);                     // (FUSED = false)
	double2       *hi2 = reinterpret_cast<double2 *>(out + (size_t) pid * FV + 3 * (size_t) NNN); // (FUSED = false)
	double2       *op2 = reinterpret_cast<double2 *>(out + (size_t) pid * NNN);                    // (FUSED = true)

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
	// on a coarse/fine side the halo value is the face's flux itself (k_cf_flux3d), everywhere else the operand beyond the face
	const bool gW = fk[0] == FACE_GHOST && X == 0, gE = fk[1] == FACE_GHOST, gS = fk[2] == FACE_GHOST && Yp == 0,
	           gN = fk[3] == FACE_GHOST && Yp == H - 1;
	const bool gB = fk[4] == FACE_GHOST, gT = fk[5] == FACE_GHOST && last;
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
		if (phys(fk[4]) && bf[4] >= 0) bot.p = reinterpret_cast<const double2 *>(fg.bdata + (size_t) bf[4] * NN);
		if (phys(fk[5]) && bf[5] >= 0) top.p = reinterpret_cast<const double2 *>(fg.bdata + (size_t) bf[5] * NN);
	}
	// the plane above the slab and U on the faces below it: the next slab's first plane and its LO_z, or the plane above the patch and HI_z
	const double2 *ctop = last ? top.p : cp2 + (z0 + ZL) * NP;
	const double2 *utop = last ? uhi + NN : ulo + 2 * (NNN / 2) + (z0 + ZL) * NP;
	// where this thread's HI_x pair sits (the threads that own none: entry 0, stride 0, of LO), and U_y above its column: LO_y of row
	// 2 Yp + 2 or, on the last row pair, HI_y (FUSED = false needs it there only)
	const double2 *Uhxp = east ? uhi + Yp : ulo, *Uyup = north ? uhi + NN / 2 + X : (FUSED ? ulo + NNN / 2 + q[1] + H : ulo);
	const int      hxs = east ? H : 0, uys = north ? H : (FUSED ? NP : 0);

	// ---- register pipeline over z: um, uc = planes z-1, z; planes z+1, z+2 in flight in a two-slot ring (plane p in slot p & 1).
	// Ul, Uhx, Uyu: U of the plane the NEXT step works on, requested by the step before, behind its fluxes.
	double2 um[2], uc[2], ur[2][2];
	double2 Ul[3][2], Uhx, Uyu;
	double2 pt[2] = {}, pfz[2] = {}; // (FUSED) the x/y part of the divergence and the lower z fluxes of the plane one step back
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
	auto request = [&](int z) { // U of plane z
#pragma unroll
		for (int a = 0; a < 3; a++)
#pragma unroll
			for (int k = 0; k < 2; k++) Ul[a][k] = ulo[a * (NNN / 2) + z * NP + q[k]];
		Uhx = Uhxp[z * hxs];
		Uyu = Uyup[z * uys];
	};
	request(z0);
	__builtin_amdgcn_sched_barrier(0);
	// (FUSED) plane zp = c - alpha * div, the upper z fluxes fzu given
	auto finish = [&](int zp, const double2 *cc, const double2 *fzu) {
#pragma unroll
		for (int k = 0; k < 2; k++) {
			const double rx = __builtin_fma(fzu[k].x - pfz[k].x, ihz, pt[k].x), ry = __builtin_fma(fzu[k].y - pfz[k].y, ihz, pt[k].y);
			const double dx = alpha * rx, dy = alpha * ry;
			if (act) op2[zp * NP + q[k]] = double2{cc[k].x - dx, cc[k].y - dy};
		}
	};

	auto step = [&](auto par, auto refill, auto more, int zz) {
		constexpr int  PAR    = decltype(par)::value;
		constexpr bool REFILL = decltype(refill)::value;
		constexpr bool MORE   = decltype(more)::value; // another step of this slab follows
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
		const bool    zb  = gB && z == 0;
		double2       fx[2], fy[2], fz[2];
		double        hx[2];
#pragma unroll
		for (int k = 0; k < 2; k++) {
			const double *t0 = tl + lds[k];
			const double2 v  = uc[k];
			const double2 ym = (k == 0) ? ylo : uc[0];
			const double  xl = t0[-1], xr = t0[2];
			fx[k].x = gW ? xl : upwindFlux(Ul[0][k].x, xl, v.x);
			fx[k].y = upwindFlux(Ul[0][k].y, v.x, v.y);
			fy[k]   = (k == 0 && gS) ? ym : upwindFlux2(Ul[1][k], ym, v);
			fz[k]   = zb ? um[k] : upwindFlux2(Ul[2][k], um[k], v);
			hx[k]   = gE ? xr : upwindFlux(k == 0 ? Uhx.x : Uhx.y, v.y, xr);
		}
		const double2 fyu = gN ? yhi : upwindFlux2(Uyu, uc[1], yhi); // the y faces above the column
		// this plane's U is consumed: the next plane's into the same registers, one step ahead of its use
		__builtin_amdgcn_sched_barrier(0);
		if (MORE) request(z + 1);
		__builtin_amdgcn_sched_barrier(0);
		if (!FUSED) {
#pragma unroll
			for (int k = 0; k < 2; k++)
				if (act) {
					lo2[z * NP + q[k]]                 = fx[k];
					lo2[NNN / 2 + z * NP + q[k]]       = fy[k];
					lo2[2 * (NNN / 2) + z * NP + q[k]] = fz[k];
				}
			if (east) hi2[Yp + H * z] = double2{hx[0], hx[1]}; // HI_x[y + N z], rows 2 Yp and 2 Yp + 1
			if (north) hi2[NN / 2 + X + H * z] = fyu;          // HI_y[x + N z]
		} else {
			if (zz > 0) finish(z - 1, um, fz);
			// the next pair's lower x flux: the next lane (pairs of a row are consecutive lanes; the row's last pair takes HI_x)
			const double nx0 = __shfl_down(fx[0].x, 1), nx1 = __shfl_down(fx[1].x, 1);
			const double xu0 = east ? hx[0] : nx0, xu1 = east ? hx[1] : nx1;
			pt[0].x = divPart<false>(fx[0].y - fx[0].x, fy[1].x - fy[0].x, ihx, ihy);
			pt[0].y = divPart<true>(xu0 - fx[0].y, fy[1].y - fy[0].y, ihx, ihy);
			pt[1].x = divPart<false>(fx[1].y - fx[1].x, fyu.x - fy[1].x, ihx, ihy);
			pt[1].y = divPart<(N >= 16)>(xu1 - fx[1].y, fyu.y - fy[1].y, ihx, ihy);
			pfz[0] = fz[0], pfz[1] = fz[1];
		}
	};
	using B0 = std::integral_constant<int, 0>;
	using B1 = std::integral_constant<int, 1>;
	static_assert(ZL % 2 == 0 && ZL >= 4, "the march is unrolled over the two ring slots and ends with two steps of its own");
#pragma unroll 1
	for (int zz = 0; zz < ZL - 2; zz += 2) {
		step(B0{}, std::true_type{}, std::true_type{}, zz);
		step(B1{}, std::true_type{}, std::true_type{}, zz + 1);
	}
	// the plane above the slab and U below it are requested two steps before the last plane needs them
	double2 tp[2], Ut[2];
#pragma unroll
	for (int k = 0; k < 2; k++) {
		tp[k] = ctop[q[k]];
		Ut[k] = utop[q[k]];
	}
	__builtin_amdgcn_sched_barrier(0);
	step(B0{}, std::false_type{}, std::true_type{}, ZL - 2);
	step(B1{}, std::false_type{}, std::false_type{}, ZL - 1);
	double2 ft[2];
#pragma unroll
	for (int k = 0; k < 2; k++) ft[k] = gT ? tp[k] : upwindFlux2(Ut[k], uc[k], tp[k]);
	if (FUSED) {
		finish(z0 + ZL - 1, uc, ft);
	} else if (last && act) {
#pragma unroll
		for (int k = 0; k < 2; k++) hi2[NN + q[k]] = ft[k]; // HI_z[x + N y]
	}
}

template <int N, int ZS>
__global__ __launch_bounds__(Tile3<N>::TPB) void k_advflux3d(LevelDev L, FaceGeom fg, const double *__restrict__ c, const double *__restrict__ U,
                                                              double *__restrict__ F)
{
	advectMarch<N, ZS, false>(L, fg, c, U, F, 0.0);
}
template <int N, int ZS>
__global__ __launch_bounds__(Tile3<N>::TPB) void k_advect3d(LevelDev L, FaceGeom fg, const double *__restrict__ c, const double *__restrict__ U,
                                                             double *__restrict__ out, double alpha)
{
	advectMarch<N, ZS, true>(L, fg, c, U, out, alpha);
}

// ---- 2D twins, in the simple form of k_cellface2d: one thread per pair of x-adjacent cells, neighbours from global memory.
// Per patch: LO_x n^2, LO_y n^2, HI_x n (by y), HI_y n (by x).
static __global__ void k_cf_flux2d(int n, const int32_t *__restrict__ desc, const int32_t *__restrict__ slots, const double *__restrict__ U,
                                   const double *__restrict__ c, double *__restrict__ ghost)
{
	const int32_t *d = desc + (size_t) blockIdx.x * 8;
	const int      p = d[0], s = d[1], kind = d[2], q = d[3];
	const int      ax = s >> 1, up = s & 1, nn = n * n;
	const size_t   FV = 2 * (size_t) nn + 2 * n;
	const int      sa = (ax == 0) ? n : 1, sn = (ax == 0) ? 1 : n;
	const int      mine = up ? (n - 1) * sn : 0, oth = up ? 0 : (n - 1) * sn;
	double        *g = ghost + (size_t) slots[blockIdx.x] * n;
	auto faceU = [&](int r, int upper, int a) {
		const double *Ur = U + (size_t) r * FV;
		return upper ? Ur[2 * (size_t) nn + ax * n + a] : Ur[(size_t) ax * nn + a * sa];
	};
	for (int a = threadIdx.x; a < n; a += blockDim.x) {
		const double m = c[(size_t) p * nn + mine + a * sa];
		if (kind == 2) {
			const int ca = (a + (q ? n : 0)) / 2;
			if (d[4] < 0) continue;
			const double C = c[(size_t) d[4] * nn + oth + ca * sa], Uf = faceU(p, up, a);
			g[a]           = up ? upwindFlux(Uf, m, C) : upwindFlux(Uf, C, m);
		} else {
			const int qa = (a >= n / 2), nbq = d[4 + qa];
			const int fa = 2 * (a - qa * (n / 2));
			if (nbq < 0) continue;
			const double *f = c + (size_t) nbq * nn + oth + fa * sa;
			double        F[2];
#pragma unroll
			for (int aa = 0; aa < 2; aa++) {
				const double Uf = faceU(nbq, !up, fa + aa), fc = f[aa * sa];
				F[aa]           = up ? upwindFlux(Uf, m, fc) : upwindFlux(Uf, fc, m);
			}
			g[a] = faceMean2(F[0], F[1]);
		}
	}
}

static __global__ void k_faces_match2d(int n, const int32_t *__restrict__ desc, double *F)
{
	const int32_t *d = desc + (size_t) blockIdx.x * 8;
	const int      p = d[0], s = d[1], kind = d[2];
	if (kind != 3) return;
	const int    ax = s >> 1, up = s & 1, nn = n * n;
	const size_t FV = 2 * (size_t) nn + 2 * n;
	const int    sa = (ax == 0) ? n : 1;
	for (int a = threadIdx.x; a < n; a += blockDim.x) {
		const int qa = (a >= n / 2), nbq = d[4 + qa];
		const int fa = 2 * (a - qa * (n / 2));
		if (nbq < 0) continue;
		const double *Ff = F + (size_t) nbq * FV;
		const double  v  = up ? faceMean2(Ff[(size_t) ax * nn + fa * sa], Ff[(size_t) ax * nn + (fa + 1) * sa])
		                      : faceMean2(Ff[2 * (size_t) nn + ax * n + fa], Ff[2 * (size_t) nn + ax * n + fa + 1]);
		double       *Fp = F + (size_t) p * FV;
		if (up)
			Fp[2 * (size_t) nn + ax * n + a] = v;
		else
			Fp[(size_t) ax * nn + a * sa] = v;
	}
}

// the flux through side s of patch p at face coordinate t: m = the cell just inside, Uf = the patch's stored entry of that face
__device__ __forceinline__ double sideFlux2d(const Level2D &L, const FaceGeom &fg, const double *c, int p, int s, int t, double m, double Uf)
{
	const int n = L.n, kind = L.face_kind[p * 4 + s], src = L.face_src[p * 4 + s];
	if (kind == FACE_GHOST) return L.ghost[(size_t) src * n + t]; // (k_cf_flux2d)
	double o;
	if (kind == FACE_DIRICHLET || kind == FACE_NEUMANN) {
		const int b = fg.bdata ? fg.bface[p * 4 + s] : -1;
		o           = b >= 0 ? fg.bdata[(size_t) b * n + t] : m;
	} else {
		const int cell = s == 0 ? (n - 1) + n * t : (s == 1 ? n * t : (s == 2 ? t + n * (n - 1) : t));
		o              = c[(size_t) src * n * n + cell];
	}
	return (s & 1) ? upwindFlux(Uf, m, o) : upwindFlux(Uf, o, m);
}
template <bool FUSED>
__global__ __launch_bounds__(256) void k_advect2d(Level2D L, FaceGeom fg, const double *__restrict__ c, const double *__restrict__ U,
                                                  double *__restrict__ out, double alpha)
{
	const int    n = L.n, h = n / 2, nn = n * n;
	const size_t total = (size_t) L.P * n * h, FV = 2 * (size_t) nn + 2 * n;
	for (size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t) gridDim.x * blockDim.x) {
		const int     p = (int) (idx / ((size_t) n * h)), q = (int) (idx % ((size_t) n * h));
		const int     y = q / h, x = 2 * (q % h);
		const double *cp = c + (size_t) p * nn;
		const double *ux = U + (size_t) p * FV, *uy = ux + nn, *uhx = uy + nn, *uhy = uhx + n;
		const double2 v  = *reinterpret_cast<const double2 *>(cp + x + n * y);
		const double2 Ux = *reinterpret_cast<const double2 *>(ux + x + n * y), Uy = *reinterpret_cast<const double2 *>(uy + x + n * y);
		double2       fx, fy;
		fx.x = (x > 0) ? upwindFlux(Ux.x, cp[x - 1 + n * y], v.x) : sideFlux2d(L, fg, c, p, 0, y, v.x, Ux.x);
		fx.y = upwindFlux(Ux.y, v.x, v.y);
		if (y > 0)
			fy = upwindFlux2(Uy, *reinterpret_cast<const double2 *>(cp + x + n * (y - 1)), v);
		else
			fy = double2{sideFlux2d(L, fg, c, p, 2, x, v.x, Uy.x), sideFlux2d(L, fg, c, p, 2, x + 1, v.y, Uy.y)};
		// the faces above the pair: of the patch (HI_x, HI_y) or of the next cells
		const bool xe = x + 2 == n, ye = y == n - 1;
		double     xu = 0.0;
		double2    yu{0.0, 0.0};
		if (xe) xu = sideFlux2d(L, fg, c, p, 1, y, v.y, uhx[y]);
		if (ye) {
			const double2 Uh = *reinterpret_cast<const double2 *>(uhy + x);
			yu               = double2{sideFlux2d(L, fg, c, p, 3, x, v.x, Uh.x), sideFlux2d(L, fg, c, p, 3, x + 1, v.y, Uh.y)};
		}
		if (!FUSED) {
			double *Fp = out + (size_t) p * FV;
			*reinterpret_cast<double2 *>(Fp + x + n * y)      = fx;
			*reinterpret_cast<double2 *>(Fp + nn + x + n * y) = fy;
			if (xe) Fp[2 * (size_t) nn + y] = xu;
			if (ye) *reinterpret_cast<double2 *>(Fp + 2 * (size_t) nn + n + x) = yu;
		} else {
			if (!xe) xu = upwindFlux(ux[x + 2 + n * y], v.y, cp[x + 2 + n * y]);
			if (!ye)
				yu = upwindFlux2(*reinterpret_cast<const double2 *>(uy + x + n * (y + 1)), v, *reinterpret_cast<const double2 *>(cp + x + n * (y + 1)));
			const double ihx = 1.0 / fg.h[(size_t) p * 3], ihy = 1.0 / fg.h[(size_t) p * 3 + 1];
			// k_divergence2d's value as the compiler contracts it: the y product rounded, the x product fused
			const double rx = divPart<false>(fx.y - fx.x, yu.x - fy.x, ihx, ihy), ry = divPart<false>(xu - fx.y, yu.y - fy.y, ihx, ihy);
			const double dx = alpha * rx, dy = alpha * ry;
			*reinterpret_cast<double2 *>(out + (size_t) p * nn + x + n * y) = double2{v.x - dx, v.y - dy};
		}
	}
}

// te_faces_max_rate: one partial per block = the largest |U_a| / h_a of its entries (blockReduce: wave shuffles, then LDS);
// k_reduce_final<RED_MAXABS> combines the partials. nlo = dim n^dim (the LO blocks of a patch), fv = nlo + dim n^(dim-1).
static __global__ __launch_bounds__(256) void k_faces_rate(size_t total, int fv, int nlo, int nc, int nf, const double *__restrict__ U,
                                                           const double *__restrict__ hgeom, double *__restrict__ partial)
{
	double acc = 0.0;
	for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t) gridDim.x * blockDim.x) {
		const size_t p = i / (size_t) fv;
		const int    r = (int) (i % (size_t) fv);
		const int    a = r < nlo ? r / nc : (r - nlo) / nf;
		acc            = fmax(acc, fabs(U[i]) / hgeom[p * 3 + a]);
	}
	acc = blockReduce<RED_MAXABS>(acc);
	if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
} // namespace te
